// jx_hpke_seal.h — RFC 9180 base-mode single-shot seal (sequence number 0, nonce = base_nonce) under every X25519
// suite: what jx_hpke_seal.hip shares with the units that hold the C ABI (jx_hpke.hip, jx_engine_seal.cpp), and the
// serial pieces of the seal. The P-256 KEM (0x0010) is out of scope for sealing: a sender context of that KEM is
// refused when it is created. The serial pieces are __host__ __device__: tests/csrc/hosttest_hpke_seal.cpp runs the
// same code on the CPU.
//
//   Encap(pkR):  enc = X25519(skE, 9), dh = X25519(skE, pkR), shared_secret = ExtractAndExpand(dh, enc || pkR)
//   key, base_nonce = the suite's key schedule over the recipient context's key_schedule_context
//   ct = AEAD.Seal(key, base_nonce, aad, pt)
// The ephemeral key skE is the caller's (the engine draws no randomness) and is a secret: it goes through
// x25519_ladder's masked swaps only. The two ladders of a report share the scalar and nothing else, so the kernels
// run them in neighbouring lanes (hpke_seal_pair_context of jx_hpke_seal.hip); here they run one after the other.
#pragma once
#include "jx_chapoly_lanes.h"
#include "jx_hpke_suites.h"
#include "jx_keyreg.h"

namespace jx {

// RFC 7748 §5 decodeScalar25519 on 8 little-endian words
JX_HD void x25519_clamp(uint32_t k[8]) {
  k[0] &= ~7u;
  k[7] = (k[7] & 0x7fffffffu) | 0x40000000u;
}
JX_HD void x25519_base_point(uint32_t u[8]) {
  u[0] = 9;
  for (int i = 1; i < 8; i++) u[i] = 0;
}

// The AEAD key and base nonce of one seal from the two ladders' outputs (enc, dh: 8 LE words each) and the
// recipient's public key, key_schedule_context and suite: ExtractAndExpand, then hpke_key_schedule. False when dh is
// all zero (a low-order recipient key: no seal).
JX_HD bool hpke_seal_context(const uint32_t enc[8], const uint32_t dh[8], const uint32_t pk[8], const uint8_t* ksc,
                             uint32_t kdf, uint32_t aead, const uint32_t zist[8], const uint32_t zost[8],
                             uint8_t key[32], uint8_t nonce[12]) {
  uint32_t nz = 0;
  for (int i = 0; i < 8; i++) nz |= dh[i];
  uint32_t ss[8];
  hpke_extract_and_expand(ss, dh, pk, zist, zost, enc);
  uint8_t ssb[32];
  for (int i = 0; i < 32; i++) ssb[i] = (uint8_t)(ss[i >> 2] >> (24 - 8 * (i & 3)));
  hpke_key_schedule(ssb, ksc, kdf, aead, key, nonce);
  return nz != 0;
}

// ---- the AEADs, one message per lane (the counterpart of suite_aead_open, jx_hpke_open.h). The plaintext and the
// associated data come a byte at a time from pt_byte(i) / aad_byte(i); ct gets plen + 16 bytes. A ciphertext block is
// folded into the MAC as it is made: nothing is read back from ct.

template <int NR, class AadByte, class PtByte>
JX_HD void gcm_seal(const uint8_t* sbox, const uint32_t* rk, const uint32_t nonce3[3], uint64_t alen, AadByte aad_byte,
                    uint64_t plen, PtByte pt_byte, uint8_t* ct) {
  uint32_t h[4], y[4] = {0, 0, 0, 0}, ks[4];
  {
    const uint32_t zero4[4] = {0, 0, 0, 0};
    aes_encrypt_nr<NR>(sbox, rk, zero4, ks);
    for (int i = 0; i < 4; i++) h[i] = bswap32(ks[i]);
  }
  for (uint64_t i = 0; i < alen; i += 16) {
    for (int w = 0; w < 4; w++) {
      uint32_t v = 0;
      for (int k = 0; k < 4; k++) {
        const uint64_t j = i + 4 * w + k;
        v = (v << 8) | (j < alen ? (uint32_t)aad_byte(j) : 0u);
      }
      y[w] ^= v;
    }
    ghash_mul(y, h);
  }
  // counter blocks: nonce (12 bytes) || BE32 counter; J0 has counter 1, the data starts at 2
  uint32_t cb[4] = {nonce3[0], nonce3[1], nonce3[2], 0};
  for (uint64_t i = 0; i < plen; i += 16) {
    cb[3] = bswap32((uint32_t)(2 + i / 16));
    aes_encrypt_nr<NR>(sbox, rk, cb, ks);
    uint32_t x[4] = {0, 0, 0, 0};
    for (uint64_t j = 0; j < 16 && i + j < plen; j++) {
      const uint8_t c = (uint8_t)(pt_byte(i + j) ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3))));
      ct[i + j] = c;
      x[j >> 2] |= (uint32_t)c << (24 - 8 * (j & 3));
    }
    for (int w = 0; w < 4; w++) y[w] ^= x[w];
    ghash_mul(y, h);
  }
  y[0] ^= (uint32_t)((8 * alen) >> 32);
  y[1] ^= (uint32_t)(8 * alen);
  y[2] ^= (uint32_t)((8 * plen) >> 32);
  y[3] ^= (uint32_t)(8 * plen);
  ghash_mul(y, h);
  cb[3] = bswap32(1u);
  aes_encrypt_nr<NR>(sbox, rk, cb, ks);
  for (int k = 0; k < 4; k++) {
    const uint32_t t = bswap32(ks[k]) ^ y[k];
    for (int q = 0; q < 4; q++) ct[plen + 4 * k + q] = (uint8_t)(t >> (24 - 8 * q));
  }
}

template <class AadByte, class PtByte>
JX_HD void chapoly_seal(const uint32_t key[8], const uint32_t nonce[3], uint64_t alen, AadByte aad_byte, uint64_t plen,
                        PtByte pt_byte, uint8_t* ct) {
  uint32_t ks[16];
  chacha20_block(key, 0, nonce, ks);
  Poly1305 p;
  poly1305_init(p, ks);
  for (uint64_t i = 0; i < alen; i += 16) {
    uint32_t m[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16 && i + k < alen; k++) m[k >> 2] |= (uint32_t)aad_byte(i + k) << (8 * (k & 3));
    poly1305_block(p, m, 1);
  }
  for (uint64_t i = 0; i < plen; i += 64) {
    chacha20_block(key, (uint32_t)(1 + i / 64), nonce, ks);
    for (uint64_t q = 0; q < 64 && i + q < plen; q += 16) {
      uint32_t m[4] = {0, 0, 0, 0};
      for (uint64_t j = q; j < q + 16 && i + j < plen; j++) {
        const uint8_t c = (uint8_t)(pt_byte(i + j) ^ (uint8_t)(ks[j >> 2] >> (8 * (j & 3))));
        ct[i + j] = c;
        m[(j - q) >> 2] |= (uint32_t)c << (8 * (j & 3));
      }
      poly1305_block(p, m, 1);
    }
  }
  const uint32_t lens[4] = {(uint32_t)alen, (uint32_t)(alen >> 32), (uint32_t)plen, (uint32_t)(plen >> 32)};
  poly1305_block(p, lens, 1);
  uint32_t tag[4];
  poly1305_finish(p, tag);
  for (int j = 0; j < 16; j++) ct[plen + j] = (uint8_t)(tag[j >> 2] >> (8 * (j & 3)));
}

// The suite's AEAD under key kb (Nk bytes used) and nonce nb.
template <class AadByte, class PtByte>
JX_HD void suite_aead_seal(const uint8_t* sbox, uint32_t aead, const uint8_t kb[32], const uint8_t nb[12], uint64_t alen,
                           AadByte aad_byte, uint64_t plen, PtByte pt_byte, uint8_t* ct) {
  uint32_t kw[8], nw[3];  // little-endian words
  for (int i = 0; i < 8; i++)
    kw[i] = (uint32_t)kb[4 * i] | ((uint32_t)kb[4 * i + 1] << 8) | ((uint32_t)kb[4 * i + 2] << 16) |
            ((uint32_t)kb[4 * i + 3] << 24);
  for (int i = 0; i < 3; i++)
    nw[i] = (uint32_t)nb[4 * i] | ((uint32_t)nb[4 * i + 1] << 8) | ((uint32_t)nb[4 * i + 2] << 16) |
            ((uint32_t)nb[4 * i + 3] << 24);
  if (aead == HPKE_AEAD_CHACHA20POLY1305) {
    chapoly_seal(kw, nw, alen, aad_byte, plen, pt_byte, ct);
    return;
  }
  uint32_t rk[60];
  if (aead == HPKE_AEAD_AES128GCM) {
    aes128_expand_key(sbox, kw, rk);
    gcm_seal<10>(sbox, rk, nw, alen, aad_byte, plen, pt_byte, ct);
  } else {
    aes256_expand_key(sbox, kw, rk);
    gcm_seal<14>(sbox, rk, nw, alen, aad_byte, plen, pt_byte, ct);
  }
}

// ---- ChaCha20-Poly1305 seal of one long message by the 64 lanes of a wave. Lane j owns the 64-byte ChaCha20 blocks
// j, j + 64, ..., and with each of them the four 16-byte MAC blocks of the ciphertext it has just made, so the MAC
// needs no second pass and no exchange. (The open's split, MAC block k to lane k mod 64, would hand the four pieces
// of a keystream block to four lanes.)
//
// The MAC input after the associated data is the sequence of T = nc + 1 blocks: the nc = ceil(plen / 16) ciphertext
// blocks, then the length block; block m's term is c_m r^(T - m). Group b holds blocks 4b .. 4b + 3 of them (those
// <= nc; the length block is the last group's last piece, or a group of its own). Lane j runs Horner over its
// groups in order: a step of r inside a group, a step of r^253 from one group's last block to the next group's first
// (4 * 64 - 3 blocks further), and a last product by r^(d_j), d_j = T - (its last block) in [1, 253]. A lane without
// a group contributes zero. The accumulator of the associated data's blocks, A = sum_i a_i r^(na - i), enters as
// RFC 8439's running sum does: added to block 0.
constexpr uint32_t SL_GAP = 4 * GL_LANES - 3;

// sum: the limb-wise sum of up to 64 lane terms (pl_lane_term). out: the same value, carried.
JX_HD void pl_sum_carry(const uint32_t sum[5], uint32_t out[5]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    c += sum[i];
    out[i] = (uint32_t)(c & PL_M26);
    c >>= 26;
  }
  out[0] += 5 * (uint32_t)c;  // c <= 64
}

// how many of the sequence's blocks group b holds (4b <= nc)
JX_HD uint32_t sl_group_blocks(uint64_t nc, uint64_t b) { return nc + 1 - 4 * b < 4 ? (uint32_t)(nc + 1 - 4 * b) : 4u; }

// Lane j's Horner partial over its groups, and d_j (0: no group). begin(b): the caller makes ChaCha20 block b;
// piece(b, q, uint32_t m[4]) -> block 4b + q of the sequence as 4 little-endian words, zero padded (the caller
// encrypts and stores that piece, or gives the length block where it falls). r1: r; rgap: r^253; a0: A, carried
// (zeros without associated data). Out: p loose, as pl_lane_partial leaves it.
template <class Begin, class Piece>
JX_HD uint32_t sl_lane_partial(uint64_t nc, uint32_t j, Begin begin, Piece piece, const uint32_t r1[5],
                               const uint32_t rgap[5], const uint32_t a0[5], uint32_t p[5]) {
  p[0] = p[1] = p[2] = p[3] = p[4] = 0;
  uint64_t last = 0;
  bool any = false;
  for (uint64_t b = j; 4 * b <= nc; b += GL_LANES) {
    const uint32_t np = sl_group_blocks(nc, b);
    begin(b);
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {  // (unrolled: q is a constant in piece)
      if (q >= np) break;
      if (any) pl_mul(p, q == 0 ? rgap : r1);
      uint32_t m[4], c[5];
      piece(b, q, m);
      pl_block_limbs(m, c);
#pragma unroll
      for (int i = 0; i < 5; i++) p[i] += c[i];
      if (b == 0 && q == 0) {
#pragma unroll
        for (int i = 0; i < 5; i++) p[i] += a0[i];  // carried + a block: < 2^27
      }
      any = true;
      last = 4 * b + q;
    }
  }
  return any ? (uint32_t)(nc + 1 - last) : 0u;
}

// ---- kernel arguments and launchers (jx_hpke_seal.hip)

// jx_hpke_seal_batch[_device] / jx_hpke_seal_long_batch[_device]: n seals under the recipient key of registry row
// `slot`. Ciphertext i goes to cts + pt_off[i] + 16 i.
struct SealArgs {
  uint64_t n;
  const HpkeKeyRow* keys;  // the device's key registry
  uint32_t slot;
  const uint8_t* sks;  // n x 32: the ephemeral private keys, clamped here
  const uint8_t* pts;
  const uint64_t* pt_off;
  const uint8_t* aads;
  const uint64_t* aad_off;
  uint8_t* encs;  // n x 32
  uint8_t* cts;
  uint8_t* ok;
  void* ctx;  // long form: scratch, n x 64 bytes (LongCtxRow of jx_hpke_long.h); short form: unused
  uint32_t zero_ist[8], zero_ost[8];  // HMAC-SHA256 pads of the empty salt
};
constexpr size_t SEAL_CTX_BYTES = 64;

// jx_client_seal_*: both shares of n reports from the rows jx_client_shard_* wrote. Scratch: 2n x 64 bytes of context
// rows (the leader's n, then the helper's n) and the n times.
struct ClientSealArgs {
  uint64_t n;
  const HpkeKeyRow* keys;
  uint32_t slot_leader, slot_helper;
  uint32_t ps_bytes, his_bytes, lis_bytes;
  uint64_t lis_stride;
  uint8_t task_id[32];
  const uint8_t* ids;          // n x 16
  const uint64_t* times;       // n (device copy of the caller's host array)
  const uint8_t* ps;           // n x ps_bytes
  const uint8_t* lis;          // n rows, lis_stride apart
  const uint8_t* his;          // n x his_bytes
  const uint8_t* sks;          // n x 64: the leader's ephemeral key, then the helper's
  const uint8_t* shard_status;  // nullable: non-zero skips the report
  uint8_t* leader_encs;        // n x 32
  uint8_t* leader_cts;         // n x (6 + lis_bytes + 16)
  uint8_t* helper_encs;        // n x 32
  uint8_t* helper_cts;         // n x (6 + his_bytes + 16)
  uint8_t* status;             // n: 0 or JX_SEAL_*
  void* ctx;
  uint32_t zero_ist[8], zero_ost[8];
};
constexpr size_t CLIENT_SEAL_CTX_BYTES = 2 * 64;

#ifdef __HIPCC__
hipError_t launch_hpke_seal(const SealArgs& a, bool long_form, hipStream_t s);
hipError_t launch_client_seal(const ClientSealArgs& a, hipStream_t s);
#endif

}  // namespace jx
