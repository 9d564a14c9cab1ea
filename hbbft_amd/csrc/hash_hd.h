// SHA3-256 and the rand 0.4 ChaChaRng of threshold_crypto's hashes (hash_g2, hash_g1_g2,
// hash_bytes), host + device: the host paths of hbtc_hash.hip, the GPU candidate kernel
// (k_hash_cand) and the encryption pad kernel (hbtc_enc.hip k_enc_pad) all run this one code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HASH_HD __host__ __device__ inline
#else
#define HASH_HD inline
#endif

namespace hbtc {

// ------------------------------------------------------------------ SHA3-256 (FIPS 202)
HASH_HD uint64_t keccak_rc(int i) {
  const uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  return RC[i];
}

HASH_HD uint64_t rotl64(uint64_t v, int c) { return c ? (v << c) | (v >> (64 - c)) : v; }

HASH_HD void keccak_f(uint64_t a[25]) {
  const int ROT[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                       25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
  for (int round = 0; round < 24; ++round) {
    uint64_t c[5], b[25];
    for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
    for (int x = 0; x < 5; ++x) {
      const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
      for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
    }
    // rho + pi: b[y, 2x + 3y] = rot(a[x, y])
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], ROT[x + 5 * y]);
    for (int y = 0; y < 25; y += 5)
      for (int x = 0; x < 5; ++x) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
    a[0] ^= keccak_rc(round);
  }
}

// SHA3-256 of the concatenation p1 || p2, absorbed byte by byte (no buffer).
struct Sha3 {
  uint64_t a[25];
  int pos;
  HASH_HD Sha3() : pos(0) {
    for (int i = 0; i < 25; ++i) a[i] = 0;
  }
  HASH_HD void absorb(const uint8_t* p, size_t len) {
    for (size_t i = 0; i < len; ++i) {
      a[pos >> 3] ^= (uint64_t)p[i] << (8 * (pos & 7));
      if (++pos == 136) {
        keccak_f(a);
        pos = 0;
      }
    }
  }
  HASH_HD void finish(uint8_t out[32]) {
    a[pos >> 3] ^= (uint64_t)0x06 << (8 * (pos & 7));
    a[135 >> 3] ^= (uint64_t)0x80 << (8 * (135 & 7));
    keccak_f(a);
    for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(a[i / 8] >> (8 * (i % 8)));
  }
};

HASH_HD void sha3_256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  Sha3 h;
  h.absorb(msg, len);
  h.finish(out);
}

// ------------------------------------------------------------------ rand 0.4 ChaChaRng
struct ChaCha04 {
  uint32_t state[16], buf[16];
  int index = 16;
  HASH_HD explicit ChaCha04(const uint32_t seed[8]) {
    state[0] = 0x61707865u;
    state[1] = 0x3320646eu;
    state[2] = 0x79622d32u;
    state[3] = 0x6b206574u;
    for (int i = 0; i < 8; ++i) state[4 + i] = seed[i];
    for (int i = 12; i < 16; ++i) state[i] = 0;
  }
  static HASH_HD uint32_t rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
  static HASH_HD void qr(uint32_t* s, int a, int b, int c, int d) {
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12);
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7);
  }
  HASH_HD void refill() {
    uint32_t s[16];
    for (int i = 0; i < 16; ++i) s[i] = state[i];
    for (int i = 0; i < 10; ++i) {
      qr(s, 0, 4, 8, 12); qr(s, 1, 5, 9, 13); qr(s, 2, 6, 10, 14); qr(s, 3, 7, 11, 15);
      qr(s, 0, 5, 10, 15); qr(s, 1, 6, 11, 12); qr(s, 2, 7, 8, 13); qr(s, 3, 4, 9, 14);
    }
    for (int i = 0; i < 16; ++i) buf[i] = s[i] + state[i];
    index = 0;
    for (int i = 12; i < 16; ++i)  // 128-bit block counter
      if (++state[i] != 0) break;
  }
  HASH_HD uint32_t next_u32() {
    if (index == 16) refill();
    return buf[index++];
  }
  HASH_HD uint64_t next_u64() {  // rand 0.4's default: the first word is the high half
    const uint64_t hi = next_u32();
    return (hi << 32) | next_u32();
  }
};

HASH_HD void seed_of_digest(const uint8_t d[32], uint32_t seed[8]) {
  for (int i = 0; i < 8; ++i)
    seed[i] = ((uint32_t)d[4 * i] << 24) | ((uint32_t)d[4 * i + 1] << 16) |
              ((uint32_t)d[4 * i + 2] << 8) | d[4 * i + 3];
}

}  // namespace hbtc
