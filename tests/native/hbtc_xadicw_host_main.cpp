// Stand-alone driver of hbtc_xadicw_hosttest.cpp (the item pass's x-adic multiplication on the
// redundant 13 x 30 form, every bound asserted), meant for a sanitizer build (`make sanitize-xadicw`).
// With a file argument it runs the table tests/xadicw_cases.py wrote (n, then n items of 18 words; m,
// then m values of 13 limbs) and prints every flag and output word, which tests/test_xadicw_host.py
// compares with the unsanitized library's.  Without one it runs checks that need no big integers, the
// 12 x 32 multiplication serving as the reference: the generator and its negative, digits of 16 and
// 32 bits, lane 5 and lane 63, the edge digit vectors and 200 random ones; pack -> unpack of 0, 1 and
// p - 1.  Exit status 0 = ran to the end (and, without a file, all as expected).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int xadicw_mul(uint32_t n, const uint32_t* items, uint32_t* out, uint32_t* flags);
int xadicw_pack(uint32_t n, const uint32_t* in, uint32_t* out);
}

namespace {
uint64_t rng_state = 0x243f6a8885a308d3ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}
// the compressed G1 generator
const uint8_t GEN[48] = {0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f,
                         0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58,
                         0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
const uint32_t P30[13] = {0x3fffaaabu, 0x27fbffffu, 0x153ffffbu, 0x2affffacu, 0x30f6241eu, 0x034a83dau, 0x112bf673u,
                          0x12e13ce1u, 0x2cd76477u, 0x1ed90d2eu, 0x29a4b1bau, 0x3a8e5ff9u, 0x001a0111u};

int run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t n = 0, m = 0;
  if (fread(&n, 4, 1, f) != 1 || n > 100000) return 2;
  std::vector<uint32_t> items(18 * (size_t)n + 1), out(72 * (size_t)n + 1), flags(n + 1);
  if (n && fread(items.data(), 72, n, f) != n) return 2;
  if (fread(&m, 4, 1, f) != 1 || m > 100000) return 2;
  std::vector<uint32_t> in(13 * (size_t)m + 1), po(25 * (size_t)m + 1);
  if (m && fread(in.data(), 52, m, f) != m) return 2;
  fclose(f);
  xadicw_mul(n, items.data(), out.data(), flags.data());
  xadicw_pack(m, in.data(), po.data());
  for (uint32_t i = 0; i < n; ++i) {
    printf("%u", flags[i]);
    for (int k = 0; k < 72; ++k) printf(" %u", out[72 * (size_t)i + k]);
    printf("\n");
  }
  for (uint32_t i = 0; i < m; ++i) {
    for (int k = 0; k < 25; ++k) printf(k ? " %u" : "%u", po[25 * (size_t)i + k]);
    printf("\n");
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) return run_file(argv[1]);
  int bad = 0;
  std::vector<uint32_t> items;
  auto push = [&](int neg, uint32_t nbits, uint32_t lane, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    uint8_t e[48];
    memcpy(e, GEN, 48);
    if (neg) e[0] ^= 0x20;
    uint32_t w[18];
    memcpy(w, e, 48);
    const uint32_t mask = nbits == 32 ? 0xffffffffu : 0xffffu;
    w[12] = d0 & mask;
    w[13] = d1 & mask;
    w[14] = d2 & mask;
    w[15] = d3 & mask;
    w[16] = nbits;
    w[17] = lane;
    items.insert(items.end(), w, w + 18);
  };
  const uint32_t top16 = 0x8000u, top32 = 0x80000000u;
  for (int neg = 0; neg < 2; ++neg)
    for (uint32_t nbits = 16; nbits <= 32; nbits += 16)
      for (uint32_t lane = 5; lane <= 63; lane += 58) {
        const uint32_t top = nbits == 32 ? top32 : top16;
        push(neg, nbits, lane, 0, 0, 0, 0);
        push(neg, nbits, lane, 1, 0, 0, 0);
        push(neg, nbits, lane, 2, 0, 0, 0);
        push(neg, nbits, lane, 0x1234u * 2, 77, 5, 9);
        push(neg, nbits, lane, 0, 3, 70000, 12345);
        push(neg, nbits, lane, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        push(neg, nbits, lane, top, top, top, top);
        push(neg, nbits, lane, 1, 1, 1, 1);
      }
  for (int i = 0; i < 200; ++i) push(i & 1, (i & 2) ? 32 : 16, (i & 4) ? 5 : 63, rnd(), rnd(), rnd(), rnd());
  const uint32_t n = (uint32_t)(items.size() / 18);
  std::vector<uint32_t> out(72 * (size_t)n), flags(n);
  xadicw_mul(n, items.data(), out.data(), flags.data());
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* it = &items[18 * (size_t)i];
    const bool zero = (it[12] | it[13] | it[14] | it[15]) == 0;
    uint32_t z = 0;
    for (int k = 24; k < 36; ++k) z |= out[72 * (size_t)i + k];
    if (flags[i] != 3u || (z == 0) != zero) {
      ++bad;
      printf("item %u: flags %u, z %s\n", i, flags[i], z ? "nonzero" : "zero");
    }
  }
  {  // pack -> unpack gives the limbs back
    uint32_t in[3 * 13] = {0}, po[3 * 25];
    in[13] = 1;
    memcpy(in + 26, P30, sizeof P30);
    in[26] -= 1;
    xadicw_pack(3, in, po);
    for (int i = 0; i < 3; ++i)
      if (memcmp(in + 13 * i, po + 25 * i + 12, 52) != 0) {
        ++bad;
        printf("round trip %d\n", i);
      }
  }
  printf("x-adic multiplication on 13 x 30, host check: %u items, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
