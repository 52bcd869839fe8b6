// TEST INFRASTRUCTURE ONLY: brute-force search for XOF streams with a rejected Field64 sample.
//
// A raw 8-byte little-endian sample is rejected when it is >= p64 = 2^64 - 2^32 + 1, i.e. when its
// high word is 0xFFFFFFFF and its low word is nonzero: a 2^-32 event. tests/golden/make_reject_golden.py
// builds this program (cc -O3 -march=native -mno-avx -pthread; an x86-64 host with AES-NI) and runs it with --search;
// nothing it prints is trusted, every hit is re-derived with the C oracle and with pyref before it is used.
//
// Both VDAF-08 XOFs are restated here from their definitions (they share no code with the oracle):
//   ts  : TurboSHAKE128(len(dst) || dst || seed || binder, D = 1), one rate block of output
//   hmac: tag = HMAC-SHA256(seed, len(dst) || dst || binder); AES-128-CTR, key tag[0:16], counter
//         block tag[16:32] with its low 64 bits a big-endian counter
//
// usage: reject_search THREADS LOG2_MAX_TRIES START MODE ...      (all byte strings in hex)
//   ts   MSG OFF NS COND...              MSG is the whole sponge input; an 8-byte counter goes at OFF
//   hmac KEY MSG k|m OFF NS COND...      counter at OFF of the key (k) or of the message (m)
//   hj   MSG1 PRE2 PART1 MSG3 NS COND... counter at byte 0 of a 32-byte blind:
//          part0 = xof(blind, MSG1)[0:32]; seed = xof(0^32, PRE2 || part0 || PART1)[0:32];
//          samples = xof(seed, MSG3)
// COND = LO:HI:MOD:REM wants one hit at a raw index i with LO <= i < HI and i % MOD == REM. The search
// ends when every COND has its own hit, or after 2^LOG2_MAX_TRIES counters from START. Each hit prints
// "HIT <cond> <counter> <index>".
#include <immintrin.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int lo, hi, mod, rem; volatile int done; } cond_t;
static cond_t conds[16];
static int nconds, nthreads, mode, ns, off, in_key;
static uint64_t start, max_tries;
static uint8_t bufA[512], bufB[512], bufC[512], bufD[512];
static size_t lenA, lenB, lenC, lenD;
static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static volatile int all_done;

#ifdef REJECT_SEARCH_SELFTEST  // 2^-12 "hits": make_reject_golden.py's preflight() checks them against the oracle
static inline int rejected(uint64_t v) { return (v >> 52) == 0xFFF; }
#else
static inline int rejected(uint64_t v) { return (uint32_t)(v >> 32) == 0xFFFFFFFFu && (uint32_t)v != 0; }
#endif

static void report(uint64_t ctr, int idx) {
    pthread_mutex_lock(&mu);
    for (int c = 0; c < nconds; c++) {
        cond_t *k = &conds[c];
        if (!k->done && idx >= k->lo && idx < k->hi && idx % k->mod == k->rem) {
            k->done = 1;
            printf("HIT %d %llu %d\n", c, (unsigned long long)ctr, idx);
            fflush(stdout);
            break;
        }
    }
    int all = 1;
    for (int c = 0; c < nconds; c++) all &= conds[c].done;
    if (all) all_done = 1;
    pthread_mutex_unlock(&mu);
}

// ---------------------------------------------------------------- Keccak-p[1600, 12]
static const uint64_t RC[12] = {
    0x000000008000808BULL, 0x800000000000008BULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800AULL, 0x800000008000000AULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
static const int RHO[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
static const int PI[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
#define ROL(v, n) (((v) << (n)) | ((v) >> (64 - (n))))

static inline void keccak12(uint64_t s[25]) {
    for (int r = 0; r < 12; r++) {
        uint64_t bc[5], t;
#pragma GCC unroll 5
        for (int i = 0; i < 5; i++) bc[i] = s[i] ^ s[i + 5] ^ s[i + 10] ^ s[i + 15] ^ s[i + 20];
#pragma GCC unroll 5
        for (int i = 0; i < 5; i++) {
            t = bc[(i + 4) % 5] ^ ROL(bc[(i + 1) % 5], 1);
#pragma GCC unroll 5
            for (int j = 0; j < 25; j += 5) s[j + i] ^= t;
        }
        t = s[1];
#pragma GCC unroll 24
        for (int i = 0; i < 24; i++) {
            uint64_t b = s[PI[i]];
            s[PI[i]] = ROL(t, RHO[i]);
            t = b;
        }
#pragma GCC unroll 5
        for (int j = 0; j < 25; j += 5) {
#pragma GCC unroll 5
            for (int i = 0; i < 5; i++) bc[i] = s[j + i];
#pragma GCC unroll 5
            for (int i = 0; i < 5; i++) s[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
        }
        s[0] ^= RC[r];
    }
}

// ---------------------------------------------------------------- SHA-256 / HMAC
static const uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
#define ROR32(v, n) (((v) >> (n)) | ((v) << (32 - (n))))

// The SHA extensions, four rounds per pair of sha256rnds2. (They have no VEX form here: in a build with AVX on,
// every switch between the two encodings stalls, and this runs twenty times slower. Hence -mno-avx.)
#ifdef __SHA__
static void sha_block(uint32_t h[8], const uint8_t *p) {
    const __m128i be = _mm_set_epi64x(0x0c0d0e0f08090a0bULL, 0x0405060700010203ULL);
    __m128i t = _mm_shuffle_epi32(_mm_loadu_si128((const __m128i *)h), 0xB1);        // CDAB
    __m128i s1 = _mm_shuffle_epi32(_mm_loadu_si128((const __m128i *)(h + 4)), 0x1B);  // EFGH
    __m128i s0 = _mm_alignr_epi8(t, s1, 8);                                           // ABEF
    s1 = _mm_blend_epi16(s1, t, 0xF0);                                                // CDGH
    const __m128i a0 = s0, a1 = s1;
    __m128i m[4];
    for (int i = 0; i < 4; i++) m[i] = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i *)(p + 16 * i)), be);
    for (int i = 0; i < 16; i++) {
        __m128i w = _mm_add_epi32(m[i & 3], _mm_loadu_si128((const __m128i *)(K256 + 4 * i)));
        s1 = _mm_sha256rnds2_epu32(s1, s0, w);
        s0 = _mm_sha256rnds2_epu32(s0, s1, _mm_shuffle_epi32(w, 0x0E));
        if (i < 12) {  // the four schedule words of round group i + 4
            t = _mm_add_epi32(_mm_sha256msg1_epu32(m[i & 3], m[(i + 1) & 3]),
                              _mm_alignr_epi8(m[(i + 3) & 3], m[(i + 2) & 3], 4));
            m[i & 3] = _mm_sha256msg2_epu32(t, m[(i + 3) & 3]);
        }
    }
    s0 = _mm_add_epi32(s0, a0);
    s1 = _mm_add_epi32(s1, a1);
    t = _mm_shuffle_epi32(s0, 0x1B);   // FEBA
    s1 = _mm_shuffle_epi32(s1, 0xB1);  // DCHG
    _mm_storeu_si128((__m128i *)h, _mm_blend_epi16(t, s1, 0xF0));
    _mm_storeu_si128((__m128i *)(h + 4), _mm_alignr_epi8(s1, t, 8));
}
#else
static void sha_block(uint32_t h[8], const uint8_t *p) {
    uint32_t w[64], a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | p[4 * i + 1] << 16 | p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
        uint32_t s0 = ROR32(w[i - 15], 7) ^ ROR32(w[i - 15], 18) ^ (w[i - 15] >> 3);
        uint32_t s1 = ROR32(w[i - 2], 17) ^ ROR32(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    for (int i = 0; i < 64; i++) {
        uint32_t t1 = hh + (ROR32(e, 6) ^ ROR32(e, 11) ^ ROR32(e, 25)) + ((e & f) ^ (~e & g)) + K256[i] + w[i];
        uint32_t t2 = (ROR32(a, 2) ^ ROR32(a, 13) ^ ROR32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
#endif

static const uint32_t SHA_IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

// h continues a hash that has already taken `done` bytes (a multiple of 64)
static void sha_finish(uint32_t h[8], size_t done, const uint8_t *m, size_t len, uint8_t out[32]) {
    uint8_t blk[128];
    uint64_t bits = (uint64_t)(done + len) * 8;
    while (len >= 64) { sha_block(h, m); m += 64; len -= 64; }
    memset(blk, 0, sizeof blk);
    memcpy(blk, m, len);
    blk[len] = 0x80;
    size_t n = len + 9 <= 64 ? 64 : 128;
    for (int i = 0; i < 8; i++) blk[n - 1 - i] = (uint8_t)(bits >> (8 * i));
    sha_block(h, blk);
    if (n == 128) sha_block(h, blk + 64);
    for (int i = 0; i < 8; i++) { out[4 * i] = h[i] >> 24; out[4 * i + 1] = h[i] >> 16; out[4 * i + 2] = h[i] >> 8; out[4 * i + 3] = h[i]; }
}

typedef struct { uint32_t in[8], outer[8]; } hkey_t;
static void hmac_key(hkey_t *k, const uint8_t key[32]) {
    uint8_t pad[64];
    memcpy(k->in, SHA_IV, 32); memcpy(k->outer, SHA_IV, 32);
    for (int i = 0; i < 64; i++) pad[i] = (i < 32 ? key[i] : 0) ^ 0x36;
    sha_block(k->in, pad);
    for (int i = 0; i < 64; i++) pad[i] = (i < 32 ? key[i] : 0) ^ 0x5c;
    sha_block(k->outer, pad);
}
static void hmac_tag(const hkey_t *k, const uint8_t *m, size_t len, uint8_t tag[32]) {
    uint32_t h[8]; uint8_t inner[32];
    memcpy(h, k->in, 32); sha_finish(h, 64, m, len, inner);
    memcpy(h, k->outer, 32); sha_finish(h, 64, inner, 32, tag);
}

// ---------------------------------------------------------------- AES-128-CTR (AES-NI)
#define KEXP(k, rc) aes_kexp(k, _mm_aeskeygenassist_si128(k, rc))
static inline __m128i aes_kexp(__m128i k, __m128i g) {
    g = _mm_shuffle_epi32(g, 0xFF);
    k = _mm_xor_si128(k, _mm_slli_si128(k, 4));
    k = _mm_xor_si128(k, _mm_slli_si128(k, 4));
    k = _mm_xor_si128(k, _mm_slli_si128(k, 4));
    return _mm_xor_si128(k, g);
}
// nblk blocks of keystream = nblk * 2 raw samples
static void aes_ctr(const uint8_t tag[32], int nblk, uint64_t *out) {
    __m128i rk[11];
    rk[0] = _mm_loadu_si128((const __m128i *)tag);
    rk[1] = KEXP(rk[0], 0x01); rk[2] = KEXP(rk[1], 0x02); rk[3] = KEXP(rk[2], 0x04); rk[4] = KEXP(rk[3], 0x08);
    rk[5] = KEXP(rk[4], 0x10); rk[6] = KEXP(rk[5], 0x20); rk[7] = KEXP(rk[6], 0x40); rk[8] = KEXP(rk[7], 0x80);
    rk[9] = KEXP(rk[8], 0x1B); rk[10] = KEXP(rk[9], 0x36);
    uint64_t ctr = 0;
    for (int i = 0; i < 8; i++) ctr = ctr << 8 | tag[24 + i];
    uint8_t blk[16];
    memcpy(blk, tag + 16, 8);
    for (int b = 0; b < nblk; b++, ctr++) {
        for (int i = 0; i < 8; i++) blk[8 + i] = (uint8_t)(ctr >> (56 - 8 * i));
        __m128i x = _mm_xor_si128(_mm_loadu_si128((const __m128i *)blk), rk[0]);
        for (int r = 1; r < 10; r++) x = _mm_aesenc_si128(x, rk[r]);
        x = _mm_aesenclast_si128(x, rk[10]);
        _mm_storeu_si128((__m128i *)(out + 2 * b), x);
    }
}
static void hxof(const uint8_t key[32], const uint8_t *m, size_t len, int nblk, uint64_t *out) {
    hkey_t k; uint8_t tag[32];
    hmac_key(&k, key); hmac_tag(&k, m, len, tag); aes_ctr(tag, nblk, out);
}

// ---------------------------------------------------------------- search
static inline void put_ctr(uint8_t *p, uint64_t c) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(c >> (8 * i)); }

static void *worker(void *arg) {
    int tid = (int)(intptr_t)arg;
    uint64_t out[260];
    int nblk = (ns + 1) / 2;
    if (mode == 0) {
        uint8_t blk[168];
        memset(blk, 0, sizeof blk);
        memcpy(blk, bufA, lenA);
        blk[lenA] ^= 0x01;
        blk[167] ^= 0x80;
        for (uint64_t t = tid; t < max_tries && !all_done; t += nthreads) {
            uint64_t s[25] = {0};
            put_ctr(blk + off, start + t);
            memcpy(s, blk, 168);
            keccak12(s);
            for (int i = 0; i < ns; i++) if (rejected(s[i])) report(start + t, i);
        }
    } else if (mode == 1) {
        uint8_t key[32], msg[512];
        hkey_t hk;
        memcpy(key, bufA, 32); memcpy(msg, bufB, lenB);
        hmac_key(&hk, key);
        for (uint64_t t = tid; t < max_tries && !all_done; t += nthreads) {
            uint8_t tag[32];
            if (in_key) { put_ctr(key + off, start + t); hmac_key(&hk, key); } else put_ctr(msg + off, start + t);
            hmac_tag(&hk, msg, lenB, tag);
            aes_ctr(tag, nblk, out);
            for (int i = 0; i < ns; i++) if (rejected(out[i])) report(start + t, i);
        }
    } else {
        uint8_t blind[32] = {0}, zero[32] = {0}, m2[512];
        hkey_t zk;
        hmac_key(&zk, zero);
        memcpy(m2, bufB, lenB);
        memcpy(m2 + lenB + 32, bufC, 32);
        for (uint64_t t = tid; t < max_tries && !all_done; t += nthreads) {
            uint8_t tag[32], seed[32];
            put_ctr(blind, start + t);
            hxof(blind, bufA, lenA, 2, (uint64_t *)(m2 + lenB));
            hmac_tag(&zk, m2, lenB + 64, tag);
            aes_ctr(tag, 2, (uint64_t *)seed);
            hxof(seed, bufD, lenD, nblk, out);
            for (int i = 0; i < ns; i++) if (rejected(out[i])) report(start + t, i);
        }
    }
    return NULL;
}

static size_t unhex(const char *h, uint8_t *out) {
    size_t n = strlen(h) / 2;
    if (n > 400) { fprintf(stderr, "hex string too long\n"); exit(2); }
    for (size_t i = 0; i < n; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); out[i] = (uint8_t)v; }
    return n;
}

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "see the head of reject_search.c\n"); return 2; }
    nthreads = atoi(argv[1]);
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    max_tries = 1ULL << atoi(argv[2]);
    start = strtoull(argv[3], NULL, 10);
    int a = 5;
    if (!strcmp(argv[4], "ts")) {
        mode = 0; lenA = unhex(argv[a++], bufA); off = atoi(argv[a++]);
        if (lenA > 166) return 2;
    } else if (!strcmp(argv[4], "hmac")) {
        mode = 1; lenA = unhex(argv[a++], bufA); lenB = unhex(argv[a++], bufB);
        in_key = argv[a++][0] == 'k'; off = atoi(argv[a++]);
        if (lenA != 32) return 2;
    } else if (!strcmp(argv[4], "hj")) {
        mode = 2; lenA = unhex(argv[a++], bufA); lenB = unhex(argv[a++], bufB); lenC = unhex(argv[a++], bufC);
        lenD = unhex(argv[a++], bufD);
        if (lenC != 32) return 2;
    } else return 2;
    ns = atoi(argv[a++]);
    if (ns < 1 || ns > 256 || (mode == 0 && ns > 21)) return 2;
    for (; a < argc && nconds < 16; a++, nconds++)
        if (sscanf(argv[a], "%d:%d:%d:%d", &conds[nconds].lo, &conds[nconds].hi, &conds[nconds].mod, &conds[nconds].rem) != 4) return 2;
    if (!nconds) return 2;
    pthread_t th[16];
    for (int i = 0; i < nthreads; i++) pthread_create(&th[i], NULL, worker, (void *)(intptr_t)i);
    for (int i = 0; i < nthreads; i++) pthread_join(th[i], NULL);
    printf(all_done ? "DONE\n" : "EXHAUSTED\n");
    return 0;
}
