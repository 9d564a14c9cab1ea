// Stand-alone driver of rlc_tree.h's host build (hbtc_tree_hosttest.cpp: the body of k_rlc_tree
// replayed merge by merge), meant for a sanitizer build (`make sanitize-tree`): the shares' slots,
// the sender table, the P nodes and the sums are heap allocations of exactly their size, so a
// read or write past a ragged last tile, a node array or a tile's sums is reported.  Every output
// is checked against the plain restatement inside th_run.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
uint32_t th_group_tiles(void);
uint32_t th_sums_points(void);
int th_run(uint32_t n_tiles, const uint32_t* counts, const uint64_t* masks, const uint64_t* s_scal,
           const uint32_t* idx, uint32_t n_pk, const uint64_t* p_scal, int reverse, uint8_t* out48);
}

namespace {
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
uint64_t all_of(uint32_t count) { return count == 64 ? ~0ull : (1ull << count) - 1ull; }

constexpr uint32_t N_PK = 70;

// one group; identity_s: the S input of every masked-out lane AND of lane 0 is the identity
int run(const std::vector<uint32_t>& counts, const std::vector<uint64_t>& masks, bool identity_s, int reverse) {
  std::vector<uint64_t> s_scal, p_scal(N_PK);
  std::vector<uint32_t> idx;
  for (size_t t = 0; t < counts.size(); ++t)
    for (uint32_t i = 0; i < counts[t]; ++i) {
      const bool in = (masks[t] >> i) & 1u;
      s_scal.push_back(in && !(identity_s && i == 0) ? next() | 1u : 0u);
      idx.push_back((uint32_t)(next() % N_PK));
    }
  for (auto& k : p_scal) k = next() | 1u;
  std::vector<uint8_t> out((size_t)counts.size() * th_sums_points() * 48);
  return th_run((uint32_t)counts.size(), counts.data(), masks.data(), s_scal.data(), idx.data(), N_PK,
                p_scal.data(), reverse, out.data());
}
}  // namespace

int main() {
  int bad = 0;
  const uint32_t G = th_group_tiles();
  const uint32_t counts[] = {1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64};
  for (uint32_t c : counts) {
    const uint64_t a = all_of(c);
    const uint64_t masks[] = {a, 0, 1ull << (c / 2), a & 0x5555555555555555ull, 1ull << (c - 1)};
    for (uint64_t m : masks) {
      const int r = run({c}, {m}, false, 0);
      if (r != 0) {
        printf("count %u mask %016llx: %d\n", c, (unsigned long long)m, r);
        ++bad;
      }
    }
    if (run({c}, {a}, true, 1) != 0) ++bad;  // an identity S beside a non-identity P, merges backwards
  }
  // groups of G, G - 1 and 1 tiles with mixed counts and masks
  for (uint32_t n : {G, G - 1, 1u}) {
    if (n == 0) continue;
    std::vector<uint32_t> cs;
    std::vector<uint64_t> ms;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t c = counts[(t * 7 + n) % 11];
      cs.push_back(c);
      ms.push_back(t % 3 == 0 ? all_of(c) : next() & all_of(c));
    }
    if (run(cs, ms, false, 0) != 0 || run(cs, ms, true, 1) != 0) {
      printf("group of %u tiles\n", n);
      ++bad;
    }
  }
  // bad arguments are refused
  {
    const uint32_t c = 65;
    const uint64_t m = 0, s = 0;
    const uint32_t i = 0;
    uint8_t o;
    if (th_run(1, &c, &m, &s, &i, 1, &s, 0, &o) != -1) ++bad;
  }
  printf("tile tree host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
