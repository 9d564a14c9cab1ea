// Stand-alone driver of own_host.h's host build (hbtc_own_hosttest.cpp), meant for a sanitizer
// build (`make sanitize-own`): scalar_mod_r, split_by_x2, gls_u_digits, wipe_words and the
// SecretScalar a call holds, on the edge scalars and on random ones.  Checks that need no
// big-integer library: known values (0, 1, |x|, x^2 -+ 1, r - 1 = x^2 (x^2 - 1), r, r + 1), the
// digit bounds, and the recomposition k0 + k1 x^2 == sum d_j |x|^j == k mod r on 32-bit limbs.
// Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void oh_mod_r(const uint8_t* sk_le32, uint8_t* out_le32);
void oh_split_x2(const uint8_t* k_le32, uint8_t* k0_le16, uint8_t* k1_le16);
void oh_u_digits(const uint8_t* k_le32, uint64_t* d4);
uint32_t oh_secret_scalar(const uint8_t* sk_le32, uint8_t* k_le32, uint8_t* k0_le16, uint8_t* k1_le16,
                          uint64_t* d4, uint8_t* after, uint32_t after_cap);
void oh_wipe(uint32_t* p, uint64_t n);
}

namespace {
const uint64_t U = 0xd201000000010000ull;  // |x|
const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                       0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
const uint32_t X2[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};

// a = a * m + add over 8 limbs; returns nonzero when the value does not fit 256 bits
uint64_t mul_add(uint32_t a[8], uint64_t m, uint64_t add) {
  unsigned __int128 c = add;
  for (int i = 0; i < 8; ++i) {
    const unsigned __int128 t = (unsigned __int128)a[i] * m + c;  // < 2^96 + 2^66
    a[i] = (uint32_t)t;
    c = t >> 32;
  }
  return c != 0;
}

bool less(const uint32_t* a, const uint32_t* b, int n) {
  for (int i = n - 1; i >= 0; --i)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}

// every check of one input; want (may be null): the expected residue
int check(const uint8_t in[32], const uint8_t* want) {
  int bad = 0;
  std::vector<uint8_t> k(32), k0(16), k1(16), k2(32), k02(16), k12(16);
  std::vector<uint64_t> d(4), d2(4);
  oh_mod_r(in, k.data());
  uint32_t kw[8];
  memcpy(kw, k.data(), 32);
  if (!less(kw, R, 8)) ++bad;
  if (want && memcmp(k.data(), want, 32) != 0) ++bad;
  oh_split_x2(k.data(), k0.data(), k1.data());
  oh_u_digits(k.data(), d.data());
  uint32_t k0w[4], k1w[4];
  memcpy(k0w, k0.data(), 16);
  memcpy(k1w, k1.data(), 16);
  if (!less(k0w, X2, 4)) ++bad;
  for (int j = 0; j < 4; ++j)
    if (d[j] >= U) ++bad;
  // sum d_j u^j by Horner
  uint32_t acc[8] = {0};
  uint64_t carry = 0;
  for (int j = 3; j >= 0; --j) carry |= mul_add(acc, U, d[j]);
  if (carry || memcmp(acc, kw, 32) != 0) ++bad;
  // k0 + k1 u^2: (k1 u) u, then k0 added in two 64-bit halves (the high one times 2^64)
  uint32_t b[8] = {0};
  memcpy(b, k1w, 16);
  carry = mul_add(b, U, 0);
  carry |= mul_add(b, U, ((uint64_t)k0w[1] << 32) | k0w[0]);
  uint32_t hi[8] = {0, 0, k0w[2], k0w[3], 0, 0, 0, 0};
  uint64_t c = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)b[i] + hi[i] + c;
    b[i] = (uint32_t)t;
    c = t >> 32;
  }
  if (carry || c || memcmp(b, kw, 32) != 0) ++bad;
  // the object a call holds gives the same forms and leaves zeros behind
  std::vector<uint8_t> after(256, 0xAA);
  const uint32_t sz = oh_secret_scalar(in, k2.data(), k02.data(), k12.data(), d2.data(), after.data(), 256);
  if (k2 != k || k02 != k0 || k12 != k1 || d2 != d || sz > 256) ++bad;
  for (uint32_t i = 0; i < sz && i < 256; ++i)
    if (after[i]) {
      ++bad;
      break;
    }
  if (bad) {
    printf("scalar ");
    for (int i = 31; i >= 0; --i) printf("%02x", in[i]);
    printf(": %d mismatches\n", bad);
  }
  return bad;
}

void put(uint8_t out[32], const uint32_t* limbs, int n) {
  memset(out, 0, 32);
  memcpy(out, limbs, 4 * (size_t)n);
}
}  // namespace

int main() {
  int bad = 0;
  uint8_t in[32], want[32];
  uint64_t d[4];
  // 0, 1, |x| - 1, |x|, x^2 - 1, x^2, x^2 + 1 are their own residues
  const uint32_t small[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {(uint32_t)(U - 1), (uint32_t)((U - 1) >> 32), 0, 0},
                               {(uint32_t)U, (uint32_t)(U >> 32), 0, 0},
                               {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u},
                               {X2[0], X2[1], X2[2], X2[3]}, {X2[0] + 1, X2[1], X2[2], X2[3]}};
  const uint64_t small_d[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {U - 1, 0, 0, 0}, {0, 1, 0, 0},
                                 {U - 1, U - 1, 0, 0}, {0, 0, 1, 0}, {1, 0, 1, 0}};
  for (size_t i = 0; i < sizeof(small) / sizeof(small[0]); ++i) {
    put(in, small[i], 4);
    bad += check(in, in);
    oh_u_digits(in, d);
    if (memcmp(d, small_d[i], 32) != 0) {
      printf("digits of small case %zu\n", i);
      ++bad;
    }
  }
  {  // r - 1 = x^2 (x^2 - 1): digits (0, 0, u - 1, u - 1), k0 = 0, k1 = x^2 - 1
    uint32_t rm1[8];
    memcpy(rm1, R, 32);
    rm1[0] -= 1;
    put(in, rm1, 8);
    bad += check(in, in);
    oh_u_digits(in, d);
    uint8_t k0[16], k1[16], zero[16] = {0};
    oh_split_x2(in, k0, k1);
    if (d[0] || d[1] || d[2] != U - 1 || d[3] != U - 1 || memcmp(k0, zero, 16) != 0 ||
        memcmp(k1, small[4], 16) != 0) {
      printf("r - 1\n");
      ++bad;
    }
  }
  {  // r -> 0, r + 1 -> 1, 2 r -> 0, 2^256 - 1 (two subtractions)
    put(in, R, 8);
    memset(want, 0, 32);
    bad += check(in, want);
    uint32_t t[8];
    memcpy(t, R, 32);
    t[0] += 1;
    put(in, t, 8);
    want[0] = 1;
    bad += check(in, want);
    uint32_t c = 0;
    for (int i = 0; i < 8; ++i) {
      const uint64_t s = ((uint64_t)R[i] << 1) | c;
      t[i] = (uint32_t)s;
      c = (uint32_t)(s >> 32);
    }
    put(in, t, 8);
    memset(want, 0, 32);
    bad += check(in, want);
    memset(in, 0xff, 32);
    bad += check(in, nullptr);
  }
  uint64_t s = 0x9e3779b97f4a7c15ull;  // random scalars, any 256-bit value
  for (int rep = 0; rep < 2000; ++rep) {
    for (int i = 0; i < 32; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      in[i] = (uint8_t)(s >> 56);
    }
    if (rep % 4 == 1) memset(in + 16, 0, 16);        // below 2^128
    if (rep % 4 == 2) memset(in, 0xff, rep % 32);    // runs of ones
    bad += check(in, nullptr);
  }
  {  // wipe_words on a heap buffer of exactly its size, and on none
    std::vector<uint32_t> w(37, 0xdeadbeefu);
    oh_wipe(w.data(), w.size());
    for (uint32_t v : w) bad += v != 0;
    oh_wipe(w.data(), 0);
  }
  printf("own-shares host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
