// Stand-alone driver of the decryption pad's host build (hbtc_dec_hosttest.cpp dh_dec_pad: the
// bodies of k_dec_seed and k_enc_pad), meant for a sanitizer build (`make sanitize-dec`): every
// buffer is a heap allocation of exactly its size, so a read or write past an item's range is
// reported.  The batch holds a gated-out item, zero-length items, the infinity encoding, lengths
// around the 16-byte block and one long item; open items are compared with the serial stream of
// hash_bytes, closed ones must be zero.  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void dh_dec_pad(uint32_t n, const uint8_t* g48, const int32_t* gate, const uint32_t* offsets, const uint8_t* v,
                uint8_t* out, int32_t* gate_out);
void dh_pad_serial(const uint8_t* g48, uint64_t len, uint8_t* out);
}

int main() {
  const uint32_t lens[] = {0, 1, 15, 16, 17, 40, 0, 64, 65, 136, 137, 1000, 4099, 0};
  const uint32_t n = sizeof(lens) / sizeof(lens[0]);
  std::vector<uint32_t> off(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
  const uint32_t total = off[n];
  std::vector<uint8_t> g((size_t)48 * n), v(total), out(total, 0xAA);
  uint32_t x = 12345;
  auto next = [&x]() { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  for (auto& b : g) b = next();  // any 48 bytes: the seed is a hash of the bytes as they are
  for (auto& b : v) b = next();
  memset(g.data() + 48 * 3, 0, 48);  // the infinity encoding
  g[48 * 3] = 0xC0;
  std::vector<int32_t> gate(n, 0), gate_out(n, -1);
  gate[4] = 5;   // NOT_ENOUGH_SHARES: closed
  gate[11] = 6;  // DUPLICATE_ENTRY: closed
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {  // with the gate, then with a null gate
    const int32_t* gt = pass == 0 ? gate.data() : nullptr;
    std::fill(out.begin(), out.end(), 0xAA);
    dh_dec_pad(n, g.data(), gt, off.data(), v.data(), out.data(), gate_out.data());
    for (uint32_t i = 0; i < n; ++i) {
      const bool open = !gt || gt[i] == 0;
      if ((gate_out[i] == 0) != open) ++bad;
      std::vector<uint8_t> pad(lens[i]);
      dh_pad_serial(g.data() + 48 * i, lens[i], pad.data());
      for (uint32_t j = 0; j < lens[i]; ++j) {
        const uint8_t want = open ? (uint8_t)(v[off[i] + j] ^ pad[j]) : (uint8_t)0;
        if (out[off[i] + j] != want) ++bad;
      }
    }
  }
  printf("dec pad host check: %u items, %u bytes, %d mismatches\n", n, total, bad);
  return bad ? 1 : 0;
}
