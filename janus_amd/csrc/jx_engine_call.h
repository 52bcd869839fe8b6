// jx_engine_call.h — the call plumbing the call families share (included at the end of jx_engine_internal.h): taking
// and carving a call's scratch and a handle's slab, the wait for a device-form call's uploads, the handle that keeps a
// pinned host copy of its small arrays, its guard and its release, and the limits every family states the same way.
#pragma once

namespace jxi {

// a sealed input share: the PlaintextInputShare's 6 bytes of framing around the share, then the AEAD tag
inline uint64_t sealed_lis_bytes(const Cfg& c) { return 6ull + c.lis_bytes + 16; }
inline uint64_t sealed_his_bytes(const Cfg& c) { return 6ull + c.his_bytes + 16; }

// the kernels index a call's elements with 32 bits and keep one value aside: at most 2^31 - 2 of them
inline bool call_count_fits(uint64_t n) { return n < 0x7FFFFFFFull; }
inline int32_t call_count_ok(jx_engine* e, uint64_t n, const char* call, const char* noun) {
  if (call_count_fits(n)) return JX_OK;
  return fail(e, JX_E_UNSUPPORTED, std::string(call) + ": more than 2^31 - 2 " + noun + " in one call");
}

// The row stride of leader input shares that kernels write or read as uint4 rows: 0 stands for packed rows.
inline int32_t lis_stride_ok(jx_engine* e, uint64_t* stride, const char* call) {
  const uint64_t lis = e->cfg.lis_bytes;
  if (*stride == 0) *stride = lis;
  if (*stride >= lis && (*stride == lis || !(*stride & 15u))) return JX_OK;
  return fail(e, JX_E_INVALID,
              std::string(call) + ": the row stride must be 0, or >= the leader input share and a multiple of 16");
}

// A slab that outlives the call (a handle's arrays): never waits for the arena, the call holds scratch already.
inline int32_t slab_get(jx_engine* e, size_t bytes, Slab& out, const char* what) {
  const hipError_t st = arena_get(e->arena, bytes, e->stream, false, false, out);
  if (st == hipErrorOutOfMemory) return fail(e, JX_E_NOMEM, std::string(what) + ": the device arena cannot hold it");
  HIPCHK(e, st);
  return JX_OK;
}
// A layout (jx_carve.h: a function of the base that returns its bytes) run twice: from null to size the scratch or
// the slab, then from the memory to set the pointers.
template <class Lay>
int32_t scratch_carve(jx_engine* e, Scratch& mem, Lay&& lay, bool may_wait = false) {
  if (const int32_t rc = scratch_get(e, lay(nullptr), mem, may_wait)) return rc;
  lay(mem.p());
  return JX_OK;
}
template <class Lay>
int32_t slab_carve(jx_engine* e, Slab& out, Lay&& lay, const char* what) {
  if (const int32_t rc = slab_get(e, lay(nullptr), out, what)) return rc;
  lay(out.p);
  return JX_OK;
}

// An event recorded behind the uploads of a device-form call's host arrays and waited for before the call returns:
// the arrays have left pageable memory by then, and the kernels queued after the event stay queued.
struct Uploads {
  hipEvent_t ev = nullptr;
  ~Uploads() {
    if (ev) (void)hipEventDestroy(ev);
  }
  hipError_t queued(hipStream_t s) {
    const hipError_t st = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    return st == hipSuccess ? hipEventRecord(ev, s) : st;
  }
  hipError_t consumed() { return hipEventSynchronize(ev); }
};
// recorded and waited for at one point: behind everything the call queued
inline hipError_t wait_uploads(jx_engine* e) {
  Uploads up;
  const hipError_t st = up.queued(e->stream);
  return st == hipSuccess ? up.consumed() : st;
}

// A handle's device arrays (carved with slab_carve) with a pinned host copy of their first host_bytes: the layout
// calls Carver::mark() behind the last region the host reads and stores what it returns in host_bytes.
struct Mirror {
  Slab slab;
  void* host = nullptr;
  size_t host_bytes = 0;
  // the one copy to the pinned buffer, behind everything queued; waits for it
  int32_t download(jx_engine* e) {
    HIPCHK(e, hipHostMalloc(&host, host_bytes, hipHostMallocDefault));
    HIPCHK(e, hipMemcpyAsync(host, slab.p, host_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return JX_OK;
  }
  template <class T>
  const T* host_of(const T* d) const {
    return same_offset(d, slab.p, host);
  }
  void put(jx_engine* e) { arena_put(e->arena, slab, e->stream); }  // the slab goes back stream-ordered
  void free(jx_engine* e) {
    put(e);
    if (host) (void)hipHostFree(host);
    host = nullptr;
  }
};

// frees the handle unless the call hands it out
template <class R, void (*Free)(R*)>
struct HandleGuard {
  R* r;
  ~HandleGuard() { Free(r); }
  R* give() {
    R* x = r;
    r = nullptr;
    return x;
  }
};
// a handle's release entry point: the owning engine's mutex and device, then its free
template <class R>
void handle_release(R* r, void (*free_fn)(R*)) {
  if (!r) return;
  std::lock_guard<FairMutex> lk(r->e->mu);
  (void)hipSetDevice(r->e->device);
  free_fn(r);
}

}  // namespace jxi
