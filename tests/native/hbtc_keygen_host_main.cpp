// Stand-alone driver of keygen.h's host build (hbtc_keygen_hosttest.cpp: the bodies of the
// hbtc_keygen.hip kernels replayed lane by lane), meant for a sanitizer build (`make
// sanitize-keygen`): every buffer is a heap allocation of exactly its size, so a read or write
// past a Part's values, a column or a batch is reported.  Checks that need no big-integer
// arithmetic: the interpolation at 0 of a quadratic with small coefficients through 0 .. 300
// points, a repeated x, and the point identities [G, G] and [G, -G] through the column sum and
// through the Horner evaluation at x = 1.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
uint32_t kh_block_size(void);
uint32_t kh_segment_len(void);
int kh_interp(uint32_t m, const uint32_t* x, const uint8_t* vals_le32, uint8_t* out_le32);
int kh_eval(uint32_t t1, const uint8_t* commit_c48, uint32_t n_x, const uint32_t* xs, uint8_t* out48);
int kh_colsum(uint32_t n_parts, uint32_t t1, const uint8_t* row0_c48, uint8_t* out48);
}

namespace {
const uint8_t GEN[48] = {0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c,
                         0x4f, 0xa9, 0xac, 0x0f, 0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05,
                         0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58, 0x6c, 0x55, 0xe8, 0x3f,
                         0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};

// f(x) = 7 + 3 x + 5 x^2 as 32 little-endian bytes (x < 2^20: below 2^64)
void f_le32(uint8_t* out, uint64_t x) {
  const uint64_t v = 7 + 3 * x + 5 * x * x;
  memset(out, 0, 32);
  for (int i = 0; i < 8; ++i) out[i] = (uint8_t)(v >> (8 * i));
}
}  // namespace

int main() {
  int bad = 0;
  const uint32_t bs = kh_block_size();
  // interpolation: any m >= 3 points of f give f(0) = 7; m = 0 gives 0; one point gives its value
  const uint32_t counts[] = {0, 1, 3, 4, bs - 1, bs, bs + 1, 300};
  for (uint32_t m : counts) {
    std::vector<uint32_t> x(m);
    std::vector<uint8_t> vals((size_t)32 * m), out(32, 0xAA);
    for (uint32_t i = 0; i < m; ++i) {
      x[i] = 3 * i + 2;  // gapped, increasing
      f_le32(vals.data() + 32 * (size_t)i, x[i]);
    }
    if (kh_interp(m, x.data(), vals.data(), out.data()) != 0) ++bad;
    uint8_t want[32] = {0};
    if (m == 1) f_le32(want, x[0]);
    if (m >= 3) want[0] = 7;
    if (memcmp(out.data(), want, 32) != 0) {
      printf("interpolation through %u points: wrong value\n", m);
      ++bad;
    }
  }
  {  // a repeated x is flagged
    std::vector<uint32_t> x = {5, 9, 5};
    std::vector<uint8_t> vals(96, 1), out(32);
    if (kh_interp(3, x.data(), vals.data(), out.data()) != 1) ++bad;
  }
  // points: 2 G through the column sum of [G], [G] and through [G, G] at x = 1 must agree;
  // [G] + [-G] and [G, -G] at x = 1 are the point at infinity
  std::vector<uint8_t> neg(GEN, GEN + 48), inf(48, 0);
  neg[0] ^= 0x20;
  inf[0] = 0xC0;
  std::vector<uint8_t> gg(96), gn(96), a(48), b(48);
  memcpy(gg.data(), GEN, 48);
  memcpy(gg.data() + 48, GEN, 48);
  memcpy(gn.data(), GEN, 48);
  memcpy(gn.data() + 48, neg.data(), 48);
  const uint32_t one = 1;
  if (kh_colsum(2, 1, gg.data(), a.data()) != 0 || kh_eval(2, gg.data(), 1, &one, b.data()) != 0 ||
      memcmp(a.data(), b.data(), 48) != 0 || memcmp(a.data(), inf.data(), 48) == 0)
    ++bad;
  if (kh_colsum(2, 1, gn.data(), a.data()) != 0 || kh_eval(2, gn.data(), 1, &one, b.data()) != 0 ||
      memcmp(a.data(), inf.data(), 48) != 0 || memcmp(b.data(), inf.data(), 48) != 0)
    ++bad;
  {  // a commitment one coefficient longer than two segments, evaluated at a batch of points
    const uint32_t t1 = 2 * kh_segment_len() + 1, n_x = 5;
    std::vector<uint8_t> cm((size_t)48 * t1), out((size_t)48 * n_x);
    for (uint32_t j = 0; j < t1; ++j) memcpy(cm.data() + 48 * (size_t)j, j % 3 == 1 ? inf.data() : GEN, 48);
    std::vector<uint32_t> xs = {1, 2, 255, 256, 0xffffffffu};
    if (kh_eval(t1, cm.data(), n_x, xs.data(), out.data()) != 0) ++bad;
    // 70 Parts of three columns: more Parts than the 64 lanes of a column sum
    std::vector<uint8_t> rows((size_t)48 * 70 * 3), cols(48 * 3);
    for (uint32_t i = 0; i < 70 * 3; ++i) memcpy(rows.data() + 48 * (size_t)i, i % 3 == 2 ? neg.data() : GEN, 48);
    if (kh_colsum(70, 3, rows.data(), cols.data()) != 0 || memcmp(cols.data(), cols.data() + 48, 48) != 0) ++bad;
  }
  printf("keygen host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
