// Stand-alone driver of msm_walk.h's host build (hbtc_msm_hosttest.cpp: one wave of the lane-uniform
// bucket walk replayed in lockstep), meant for a sanitizer build (`make sanitize-msm`): the rank
// offsets, the sorted lists, the points and the snapshot slots are heap allocations of exactly
// their size, so a read past ro[B], past a slice or past a lane's slots is reported.  The toy
// group's lanes are checked against plain arithmetic here, G1's against the nested loops inside
// mh_g1.  The cases are those of tests/test_msm_walk_host.py.  Exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
uint64_t mh_toy_modulus(void);
int mh_toy(uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots, const int16_t* digits,
           const uint64_t* vals, const uint8_t* inf, uint64_t* out, uint32_t* stats);
int mh_g1(uint32_t n_win, uint32_t n, uint32_t B, uint32_t S, uint32_t slots, const int16_t* digits,
          const uint64_t* scal, uint8_t* out48, uint32_t* stats);
}

namespace {
uint64_t rng_state = 0x243f6a8885a308d3ull;
uint64_t next() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr uint32_t B = 64;

struct Case {
  const char* name;
  uint32_t n_win, n, S;  // S = 1: one lane walks the whole window
  std::vector<int16_t> digits;  // [n_win][n]
  std::vector<uint64_t> scal;   // [n]; 0 = the identity
};

Case random_case(const char* name, uint32_t n_win, uint32_t n) {
  Case c{name, n_win, n, 8, {}, {}};
  for (uint32_t i = 0; i < n_win * n; ++i) c.digits.push_back((int16_t)((int)(next() % (2 * B + 1)) - (int)B));
  for (uint32_t i = 0; i < n; ++i) c.scal.push_back(next() | 1u);
  return c;
}

std::vector<Case> cases() {
  std::vector<Case> cs;
  cs.push_back(random_case("random", 8, 334));
  {
    Case c = random_case("total = 0", 2, 20);
    for (auto& d : c.digits) d = 0;
    cs.push_back(c);
  }
  {
    Case c = random_case("total < S", 1, 20);
    for (uint32_t i = 0; i < c.n; ++i) c.digits[i] = i == 3 ? 5 : i == 9 ? -64 : i == 17 ? 1 : 0;
    cs.push_back(c);
  }
  {
    Case c = random_case("one bucket", 1, 100);
    for (uint32_t i = 0; i < c.n; ++i) c.digits[i] = (i & 1) ? 17 : -17;
    cs.push_back(c);
  }
  {
    Case c = random_case("bucket B, then bucket 1", 1, 84);
    for (uint32_t i = 0; i < c.n; ++i) c.digits[i] = i == 40 ? (int16_t)B : 1;
    cs.push_back(c);
  }
  {
    Case c = random_case("walks of 0, 1 and 84", 3, 672);
    for (uint32_t i = 0; i < c.n; ++i) {
      c.digits[i] = 0;
      c.digits[c.n + i] = i < 8 ? (int16_t)(1 + 9 * i) : 0;
      if (!c.digits[2 * c.n + i]) c.digits[2 * c.n + i] = 1;
    }
    cs.push_back(c);
  }
  {
    // P then -P at the head of a bucket, the same point twice in the next, and an empty rank after
    // a rank of one point (tot == snapshot when the second snapshot arrives)
    Case c{"P - P, doubling", 1, 8, 1, {33, -33, 20, 20, 7, 5, 5, 0}, {11, 11, 23, 23, 5, 9, 9, 3}};
    cs.push_back(c);
    Case d{"tot == snapshot", 1, 2, 1, {64, 62}, {7, 1}};
    d.scal[1] = 0;
    cs.push_back(d);
    Case e{"one point, bucket B - 2", 1, 1, 1, {62}, {7}};
    cs.push_back(e);
  }
  return cs;
}

// sum over the window of d_i v_i, modulo p
uint64_t toy_window(const Case& c, uint32_t w, uint64_t p) {
  unsigned __int128 acc = 0;
  for (uint32_t i = 0; i < c.n; ++i) {
    const int d = c.digits[(size_t)w * c.n + i];
    if (!c.scal[i]) continue;
    const uint64_t v = c.scal[i] % p;
    const uint64_t t = (uint64_t)((unsigned __int128)v * (uint64_t)(d < 0 ? -d : d) % p);
    acc = (acc + (d < 0 ? (p - t) % p : t)) % p;
  }
  return (uint64_t)acc;
}
}  // namespace

int main() {
  int bad = 0;
  const uint64_t p = mh_toy_modulus();
  for (const Case& c : cases())
    for (uint32_t slots : {1u, 2u, 4u}) {
      uint32_t stats[4];
      std::vector<uint64_t> out((size_t)c.n_win * c.S);
      std::vector<uint8_t> inf(c.n);
      for (uint32_t i = 0; i < c.n; ++i) inf[i] = c.scal[i] == 0;
      int r = mh_toy(c.n_win, c.n, B, c.S, slots, c.digits.data(), c.scal.data(), inf.data(), out.data(), stats);
      for (uint32_t w = 0; r == 0 && w < c.n_win; ++w) {
        uint64_t sum = 0;
        for (uint32_t s = 0; s < c.S; ++s) sum = (sum + out[w * c.S + s]) % p;
        if (sum != toy_window(c, w, p)) r = 1;
      }
      if (r != 0) {
        printf("toy %s, %u slots: %d\n", c.name, slots, r);
        ++bad;
      }
      std::vector<uint8_t> out48((size_t)c.n_win * 48);
      r = mh_g1(c.n_win, c.n, B, c.S, slots, c.digits.data(), c.scal.data(), out48.data(), stats);
      if (r != 0) {
        printf("g1 %s, %u slots: %d\n", c.name, slots, r);
        ++bad;
      }
    }
  // bad arguments are refused
  {
    const int16_t d = 65;
    const uint64_t v = 1;
    const uint8_t i = 0;
    uint64_t o[8];
    uint32_t st[4];
    if (mh_toy(1, 1, B, 8, 1, &d, &v, &i, o, st) != -1) ++bad;  // |digit| > B
    if (mh_toy(9, 1, B, 8, 1, &d, &v, &i, o, st) != -1) ++bad;  // more than 64 lanes
  }
  printf("msm walk host check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
