// Host build of janus_amd/csrc/jx_ntt.h for tests/test_ntt_host.py: the transforms one lane at a time, data
// and tables as 16-byte little-endian words.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../janus_amd/csrc/jx_ntt.h"

using namespace jx;

namespace {
f128 ld(const uint8_t* p) {
  f128 v;
  memcpy(&v.lo, p, 8);
  memcpy(&v.hi, p + 8, 8);
  return v;
}
void st(uint8_t* p, f128 v) {
  memcpy(p, &v.lo, 8);
  memcpy(p + 8, &v.hi, 8);
}
std::vector<f128> load(const uint8_t* p, uint32_t n) {
  std::vector<f128> a(n);
  for (uint32_t i = 0; i < n; i++) a[i] = ld(p + 16 * i);
  return a;
}
const auto nosync = [] {};
}  // namespace

extern "C" {

// the table of size 2^logP, entries out of Montgomery form (canonical), ntt_table_len(P) of them
void nt_table(uint32_t logP, uint8_t* out) {
  const uint32_t P = 1u << logP;
  std::vector<f128> t(ntt_table_len(P));
  ntt_build_table(logP, t.data());
  for (uint32_t i = 0; i < t.size(); i++) st(out + 16 * i, from_mont128(t[i]));
}

// op 0: ntt_dif with the inverse twiddles; 1: ntt_dit with the forward twiddles; 2: ntt_odd_points. In place.
void nt_transform(int op, uint32_t logP, uint8_t* data) {
  const uint32_t P = 1u << logP;
  std::vector<f128> t(ntt_table_len(P)), a = load(data, P);
  ntt_build_table(logP, t.data());
  if (op == 0) ntt_dif(a.data(), P, t.data() + P / 2, 0u, 1u, nosync);
  if (op == 1) ntt_dit(a.data(), P, t.data(), 0u, 1u, nosync);
  if (op == 2) ntt_odd_points(a.data(), P, t.data(), 0u, 1u, nosync);
  for (uint32_t i = 0; i < P; i++) st(data + 16 * i, a[i]);
}

// G = sum over pairs of wire_2i * wire_2i+1 from `npairs` pairs of P wire values each: out[2P] coefficients
void nt_gpoly(uint32_t logP, uint32_t npairs, const uint8_t* wires, uint8_t* out) {
  const uint32_t P = 1u << logP;
  std::vector<f128> t(ntt_table_len(P)), E(P, make128(0, 0)), O(P, make128(0, 0));
  ntt_build_table(logP, t.data());
  for (uint32_t i = 0; i < npairs; i++) {
    std::vector<f128> a = load(wires + 16ull * P * (2 * i), P), b = load(wires + 16ull * P * (2 * i + 1), P);
    for (uint32_t k = 0; k < P; k++) E[k] = add128(E[k], mont128(a[k], b[k]));
    ntt_odd_points(a.data(), P, t.data(), 0u, 1u, nosync);
    ntt_odd_points(b.data(), P, t.data(), 0u, 1u, nosync);
    for (uint32_t k = 0; k < P; k++) O[k] = add128(O[k], mont128(a[k], b[k]));
  }
  ntt_gpoly_finish(E.data(), O.data(), P, logP, t.data(), 0u, 1u, nosync,
                   [&](uint32_t j, f128 g) { st(out + 16 * j, g); });
}
}
