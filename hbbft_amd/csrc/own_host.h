// Host-side handling of the one secret scalar of hbtc_decrypt, hbtc_decrypt_shares and
// hbtc_sign_shares: its reduction mod r, its two splits (x^2 for k_pb_mul_glv, the base-|x| digits
// of curve.h gls_u_digits for k_sig_share) and the wiping of every host copy.  Host code only;
// tests/native/hbtc_own_hosttest.cpp compiles it for tests/test_own_host.py (against Python
// integers) and for `make sanitize-own`.
#pragma once
#include <cstring>

#include "curve.h"

namespace hbtc {

// k mod r for a 256-bit little-endian scalar (k < 2^256 < 3r: at most two subtractions)
inline void scalar_mod_r(uint32_t* out, const uint8_t* in) {
  static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  uint32_t k[8];
  memcpy(k, in, 32);
  for (int rep = 0; rep < 2; ++rep) {
    bool ge = true;
    for (int i = 7; i >= 0; --i)
      if (k[i] != R[i]) {
        ge = k[i] > R[i];
        break;
      }
    if (!ge) break;
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
      const uint64_t d = (uint64_t)k[i] - R[i] - borrow;
      k[i] = (uint32_t)d;
      borrow = (d >> 63) & 1u;
    }
  }
  memcpy(out, k, 32);
}

// k (canonical, < r, 8 little-endian limbs) = k1 x^2 + k0 with k0 < x^2 and k1 < 2^128 (k < r <
// x^4): binary long division by x^2 = 0xac45a4010001a4020000000100000000.
inline void split_by_x2(const uint32_t* k, uint32_t* k0, uint32_t* k1) {
  static const uint32_t X2[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};
  uint32_t rem[5] = {0, 0, 0, 0, 0};
  uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int bit = 255; bit >= 0; --bit) {
    for (int j = 4; j > 0; --j) rem[j] = (rem[j] << 1) | (rem[j - 1] >> 31);  // rem = 2 rem + bit
    rem[0] = (rem[0] << 1) | ((k[bit >> 5] >> (bit & 31)) & 1u);
    bool ge = rem[4] != 0;
    if (!ge) {
      ge = true;
      for (int j = 3; j >= 0; --j)
        if (rem[j] != X2[j]) {
          ge = rem[j] > X2[j];
          break;
        }
    }
    if (ge) {
      uint64_t borrow = 0;
      for (int j = 0; j < 5; ++j) {
        const uint64_t d = (uint64_t)rem[j] - (j < 4 ? X2[j] : 0u) - borrow;
        rem[j] = (uint32_t)d;
        borrow = (d >> 63) & 1u;
      }
      q[bit >> 5] |= 1u << (bit & 31);
    }
  }
  for (int j = 0; j < 4; ++j) {
    k0[j] = rem[j];
    k1[j] = q[j];
  }
}

inline void wipe_words(uint32_t* p, size_t n) {
  volatile uint32_t* v = p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

// The secret scalar of one call in every form a kernel takes it.  A call constructs it first and
// returns last, so the wipe runs after the call's final wait on every exit path: no copy that the
// device may still be reading from is cleared early.
struct SecretScalar {
  uint32_t k[8];         // sk mod r, canonical
  uint32_t k0[4], k1[4];  // k = k0 + k1 x^2
  uint64_t d[4];         // k = sum_j d[j] |x|^j
  explicit SecretScalar(const uint8_t* sk_le32) {
    scalar_mod_r(k, sk_le32);
    split_by_x2(k, k0, k1);
    gls_u_digits(k, d);
  }
  SecretScalar(const SecretScalar&) = delete;
  SecretScalar& operator=(const SecretScalar&) = delete;
  ~SecretScalar() {
    wipe_words(k, 8);
    wipe_words(k0, 4);
    wipe_words(k1, 4);
    wipe_words(reinterpret_cast<uint32_t*>(d), 8);
  }
};

}  // namespace hbtc
