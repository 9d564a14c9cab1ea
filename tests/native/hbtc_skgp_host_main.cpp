// Stand-alone driver of skgp.h's host build (hbtc_skgp_hosttest.cpp: the bodies of the
// hbtc_skgp.hip kernels replayed lane by lane), meant for a sanitizer build (`make sanitize-skgp`):
// every buffer is a heap allocation of exactly its size, so a read past the packed triangle or a
// write past a frame is reported.  Checks that need no big-integer arithmetic: commitments to 0, 1
// and r + 1 in odd and even counts, the rows of a bivariate polynomial and the values of a row
// with small coefficients, and rows without coefficients.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
uint32_t sh_coeff_pos(uint32_t i, uint32_t j);
uint64_t sh_row_bytes(uint32_t t1);
void sh_commit(uint32_t n, const uint8_t* bcoef_le32, uint8_t* out48, uint8_t* ref48);
void sh_rows(uint32_t n_rows, uint32_t t1, const uint8_t* bcoef_le32, uint8_t* out);
void sh_vals(uint32_t n_rows, uint32_t n_nodes, uint32_t n_coeff, const uint8_t* rows_le32, uint8_t* out);
}

namespace {
const uint8_t GEN[48] = {0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c,
                         0x4f, 0xa9, 0xac, 0x0f, 0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05,
                         0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58, 0x6c, 0x55, 0xe8, 0x3f,
                         0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
// r + 1, little-endian
const uint8_t R_PLUS_1[32] = {0x02, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe,
                              0xff, 0x02, 0xa4, 0xbd, 0x53, 0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8,
                              0x39, 0x33, 0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73};

void small_le32(uint8_t* out, uint64_t v) {
  memset(out, 0, 32);
  for (int i = 0; i < 8; ++i) out[i] = (uint8_t)(v >> (8 * i));
}
// the FieldWrap of a value below 2^64
bool frame_is(const uint8_t* f, uint64_t v) {
  uint8_t want[40] = {0};
  want[0] = 32;
  for (int i = 0; i < 8; ++i) want[39 - i] = (uint8_t)(v >> (8 * i));
  return memcmp(f, want, 40) == 0;
}
}  // namespace

int main() {
  int bad = 0;
  std::vector<uint8_t> inf(48, 0);
  inf[0] = 0xC0;
  // commitments: [0, 1, r + 1, 1, 0] in counts 1 .. 5 (a zero paired with a non-zero, odd counts)
  for (uint32_t n = 1; n <= 5; ++n) {
    std::vector<uint8_t> b((size_t)32 * n, 0), out((size_t)48 * n, 0xAA), ref((size_t)48 * n);
    const int kind[5] = {0, 1, 2, 1, 0};
    for (uint32_t i = 0; i < n; ++i) {
      if (kind[i] == 1) b[32 * (size_t)i] = 1;
      if (kind[i] == 2) memcpy(b.data() + 32 * (size_t)i, R_PLUS_1, 32);
    }
    sh_commit(n, b.data(), out.data(), ref.data());
    if (memcmp(out.data(), ref.data(), out.size()) != 0) ++bad;
    for (uint32_t i = 0; i < n; ++i)
      if (memcmp(out.data() + 48 * (size_t)i, kind[i] ? GEN : inf.data(), 48) != 0) {
        printf("commitment %u of %u: wrong point\n", i, n);
        ++bad;
      }
  }
  {  // rows: b(x, y) = 1 + 2 (x + y) + 3 x y, so row x = (1 + 2 x) + (2 + 3 x) y
    const uint32_t t1 = 2, n_rows = 5;
    std::vector<uint8_t> b(32 * 3);
    small_le32(b.data() + 32 * sh_coeff_pos(0, 0), 1);
    small_le32(b.data() + 32 * sh_coeff_pos(0, 1), 2);
    small_le32(b.data() + 32 * sh_coeff_pos(1, 1), 3);
    const size_t rb = (size_t)sh_row_bytes(t1);
    std::vector<uint8_t> out(rb * n_rows);
    sh_rows(n_rows, t1, b.data(), out.data());
    for (uint32_t x = 1; x <= n_rows; ++x) {
      const uint8_t* f = out.data() + rb * (x - 1);
      const uint8_t head[8] = {2, 0, 0, 0, 0, 0, 0, 0};
      if (rb != 88 || memcmp(f, head, 8) != 0 || !frame_is(f + 8, 1 + 2 * x) || !frame_is(f + 48, 2 + 3 * x)) {
        printf("row %u: wrong frame\n", x);
        ++bad;
      }
    }
    // a constant polynomial: one coefficient, every row is it
    std::vector<uint8_t> c(32), o1(48 * 3);
    small_le32(c.data(), 9);
    sh_rows(3, 1, c.data(), o1.data());
    for (uint32_t x = 0; x < 3; ++x)
      if (o1[48 * x] != 1 || !frame_is(o1.data() + 48 * x + 8, 9)) ++bad;
  }
  {  // values: rows 7 + 3 x + 5 x^2 and 11 at 300 nodes (more than one 256-lane block)
    const uint32_t n_nodes = 300;
    std::vector<uint8_t> rows(32 * 6, 0), out((size_t)40 * 2 * n_nodes);
    small_le32(rows.data(), 7);
    small_le32(rows.data() + 32, 3);
    small_le32(rows.data() + 64, 5);
    small_le32(rows.data() + 96, 11);
    sh_vals(2, n_nodes, 3, rows.data(), out.data());
    for (uint64_t i = 0; i < n_nodes; ++i) {
      const uint64_t x = i + 1;
      if (!frame_is(out.data() + 40 * i, 7 + 3 * x + 5 * x * x) || !frame_is(out.data() + 40 * (n_nodes + i), 11)) {
        printf("value %u: wrong frame\n", (unsigned)i);
        ++bad;
      }
    }
    // rows without coefficients: every value is 0, and nothing is read
    std::vector<uint8_t> o0(40 * 3, 0xAA);
    sh_vals(1, 3, 0, nullptr, o0.data());
    for (int i = 0; i < 3; ++i)
      if (!frame_is(o0.data() + 40 * i, 0)) ++bad;
  }
  printf("skgp host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
