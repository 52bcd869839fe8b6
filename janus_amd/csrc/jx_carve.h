// jx_carve.h — one rule for laying regions out of a device slab: each region starts 256-aligned from the base and
// takes at least 256 bytes, so an empty region still has a pointer of its own. A layout is written once, as a
// function of the base, and run twice: from null to size the slab, then from the slab to set the pointers.
// Host only and free of HIP, so it compiles alone (tests/csrc/hosttest_carve.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace jxi {

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

class Carver {
 public:
  explicit Carver(void* base) : base_(static_cast<uint8_t*>(base)) {}  // null: only size the layout
  template <class T>
  void take(T*& p, size_t bytes) {
    if (base_) p = reinterpret_cast<T*>(base_ + off_);
    off_ += align256(bytes ? bytes : 1);
  }
  size_t bytes() const { return off_; }
  // The regions taken so far are a prefix that something treats as one (a handle's pinned host copy): its length.
  size_t mark() { return mark_ = off_; }
  size_t marked() const { return mark_; }

 private:
  uint8_t* base_;
  size_t off_ = 0, mark_ = 0;
};

// Where p, a pointer into the buffer at `base`, lies in a second buffer at `other` that holds a copy of it.
template <class T>
const T* same_offset(const T* p, const void* base, const void* other) {
  return reinterpret_cast<const T*>(static_cast<const uint8_t*>(other) +
                                    (reinterpret_cast<const uint8_t*>(p) - static_cast<const uint8_t*>(base)));
}

}  // namespace jxi
