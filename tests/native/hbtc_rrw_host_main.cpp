// Stand-alone driver of the redundant 13 x 30 form's host build (hbtc_rrw_hosttest.cpp), meant for a
// sanitizer build (`make sanitize-rrw`).  With a file argument it runs the case table that
// tests/rrw_cases.py wrote (the table of tests/test_rrw_host.py: n, then per item the op and 78 input
// words; then m and m encodings of 48 bytes) and prints every flag and output word, which the test
// compares with the unsanitized library's.  Without one it runs checks that need no big integers,
// the 12 x 32 chains serving as the reference: the subgroup test and t1 = [|x|] P on random
// encodings, (0, 2) and (0, -2).  Exit status 0 = ran to the end (and, without a file, all as expected).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int rrw_ops(uint32_t n, const uint32_t* ops, const uint32_t* in, uint32_t* out, uint32_t* flag);
int rrw_subgroup(uint32_t n, const uint8_t* c48, uint32_t* out, uint32_t* flags);
}

namespace {
uint64_t rng_state = 0x13198a2e03707344ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}

int run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t n = 0, m = 0;
  if (fread(&n, 4, 1, f) != 1 || n > 100000) return 2;
  std::vector<uint32_t> ops(n), in(78 * (size_t)n), out(39 * (size_t)n), flag(n);
  for (uint32_t i = 0; i < n; ++i)
    if (fread(&ops[i], 4, 1, f) != 1 || fread(&in[78 * (size_t)i], 4, 78, f) != 78) return 2;
  if (fread(&m, 4, 1, f) != 1 || m > 100000) return 2;
  std::vector<uint8_t> c(48 * (size_t)m + 1);
  if (m && fread(c.data(), 48, m, f) != m) return 2;
  fclose(f);
  std::vector<uint32_t> so(72 * (size_t)m + 1), sf(m + 1);
  rrw_ops(n, ops.data(), in.data(), out.data(), flag.data());
  rrw_subgroup(m, c.data(), so.data(), sf.data());
  for (uint32_t i = 0; i < n; ++i) {
    printf("%u", flag[i]);
    for (int k = 0; k < 39; ++k) printf(" %u", out[39 * (size_t)i + k]);
    printf("\n");
  }
  for (uint32_t i = 0; i < m; ++i) {
    printf("%u", sf[i]);
    for (int k = 0; k < 72; ++k) printf(" %u", so[72 * (size_t)i + k]);
    printf("\n");
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) return run_file(argv[1]);
  int bad = 0;
  const int n = 12;
  std::vector<uint8_t> c(48 * n);
  for (int i = 0; i < n; ++i) {
    uint8_t* e = &c[48 * (size_t)i];
    for (int k = 0; k < 48; ++k) e[k] = (uint8_t)(rnd() >> 24);
    e[0] = (uint8_t)(0x80 | ((i & 1) ? 0x20 : 0) | (e[0] & 0x0f));  // compressed, x < 2^380
    if (i == 0) { memset(e, 0, 48); e[0] = 0x80; }                    // (0, 2): order 3
    if (i == 1) { memset(e, 0, 48); e[0] = 0xa0; }                    // (0, -2)
  }
  std::vector<uint32_t> out(72 * n), flags(n);
  rrw_subgroup(n, c.data(), out.data(), flags.data());
  int decoded = 0;
  for (int i = 0; i < n; ++i) {
    if (!(flags[i] & 1)) continue;
    ++decoded;
    const bool w = flags[i] & 4, ref = flags[i] & 8, same = flags[i] & 16;
    if (w != ref || !same) { ++bad; printf("subgroup %d: %u\n", i, flags[i]); }
    if (w) { ++bad; printf("a random curve point or a point of order 3 passed the test: %d\n", i); }
  }
  if (decoded < 4) { ++bad; printf("only %d encodings decoded\n", decoded); }
  printf("redundant 13 x 30 host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
