// Host build of the decryption pad (enc.h dec_seed_item = k_dec_seed's item, enc_pad_lane =
// k_enc_pad's lane) behind a tiny C ABI, so the CPU suite can check it against the oracle's
// hash_bytes without a GPU (tests/test_dec_host.py) and a sanitizer build can run it as a
// stand-alone program (hbtc_dec_host_main.cpp, `make sanitize-dec`).  Test infrastructure only:
// never linked into the product library.
#include <cstring>
#include <vector>

#include "enc.h"

using namespace hbtc;

extern "C" {

// The decryption half as the GPU runs it: k_dec_seed's item for each of the n ciphertexts, gated
// on gate[i] == 0 (gate null: every item passes), then every pad block by k_enc_pad's lane, last
// block first -- lanes are independent.  out has the layout of v; gate_out[i] = the pad's gate
// (0 = open).
void dh_dec_pad(uint32_t n, const uint8_t* g48, const int32_t* gate, const uint32_t* offsets, const uint8_t* v,
                uint8_t* out, int32_t* gate_out) {
  std::vector<uint32_t> seeds((size_t)8 * n), blk((size_t)n + 1);
  uint32_t nb = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[12];
    for (int j = 0; j < 12; ++j) {
      const uint8_t* b = g48 + 48 * (size_t)i + 4 * j;
      w[j] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    gate_out[i] = dec_seed_item(seeds.data() + 8 * (size_t)i, w, !gate || gate[i] == 0);
    blk[i] = nb;
    nb += (uint32_t)enc_pad_blocks(offsets[i + 1] - offsets[i]);
  }
  blk[n] = nb;
  for (uint32_t b = nb; b-- > 0;) enc_pad_lane(b, n, blk.data(), offsets, seeds.data(), gate_out, v, out);
}

// the serial stream of the host hash_bytes (hbtc_hash.hip): one next_u32 per byte, seeded through
// the byte-wise SHA3 (not enc_pad_seed's lane form)
void dh_pad_serial(const uint8_t* g48, uint64_t len, uint8_t* out) {
  uint8_t d[32];
  uint32_t seed[8];
  sha3_256(g48, 48, d);
  seed_of_digest(d, seed);
  ChaCha04 rng(seed);
  for (uint64_t i = 0; i < len; ++i) out[i] = (uint8_t)rng.next_u32();
}

}  // extern "C"
