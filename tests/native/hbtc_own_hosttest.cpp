// Host build of own_host.h (the secret scalar of hbtc_decrypt_shares / hbtc_sign_shares: reduction
// mod r, the x^2 split, the base-|x| digits of curve.h gls_u_digits, the wiping) behind a tiny C
// ABI, so the CPU suite can check it against Python integers without a GPU
// (tests/test_own_host.py) and a sanitizer build can run it as a stand-alone program
// (hbtc_own_host_main.cpp, `make sanitize-own`).  Test infrastructure only: never linked into the
// product library.
#include <cstring>
#include <new>

#include "own_host.h"

using namespace hbtc;

extern "C" {

// 32 little-endian bytes, any value < 2^256 -> its residue mod r (32 LE bytes)
void oh_mod_r(const uint8_t* sk_le32, uint8_t* out_le32) {
  uint32_t k[8];
  scalar_mod_r(k, sk_le32);
  memcpy(out_le32, k, 32);
}

// a canonical k (32 LE bytes, < r) -> k0, k1 (16 LE bytes each): k = k0 + k1 x^2
void oh_split_x2(const uint8_t* k_le32, uint8_t* k0_le16, uint8_t* k1_le16) {
  uint32_t k[8], k0[4], k1[4];
  memcpy(k, k_le32, 32);
  split_by_x2(k, k0, k1);
  memcpy(k0_le16, k0, 16);
  memcpy(k1_le16, k1, 16);
}

// a canonical k (32 LE bytes, < r) -> its four base-|x| digits
void oh_u_digits(const uint8_t* k_le32, uint64_t* d4) {
  uint32_t k[8];
  memcpy(k, k_le32, 32);
  gls_u_digits(k, d4);
}

// The scalar as a call holds it: every form of SecretScalar copied out (k 32 bytes, k0 and k1 16
// each, d four words), then, after its destructor has run, the object's own storage copied to
// `after` (sizeof(SecretScalar) bytes at most `after_cap`): all zeros when the wipe works.
// Returns sizeof(SecretScalar).
uint32_t oh_secret_scalar(const uint8_t* sk_le32, uint8_t* k_le32, uint8_t* k0_le16, uint8_t* k1_le16,
                          uint64_t* d4, uint8_t* after, uint32_t after_cap) {
  alignas(SecretScalar) unsigned char store[sizeof(SecretScalar)];
  SecretScalar* s = new (store) SecretScalar(sk_le32);
  memcpy(k_le32, s->k, 32);
  memcpy(k0_le16, s->k0, 16);
  memcpy(k1_le16, s->k1, 16);
  memcpy(d4, s->d, 32);
  s->~SecretScalar();
  memcpy(after, store, sizeof(SecretScalar) < after_cap ? sizeof(SecretScalar) : after_cap);
  return (uint32_t)sizeof(SecretScalar);
}

void oh_wipe(uint32_t* p, uint64_t n) { wipe_words(p, (size_t)n); }

}  // extern "C"
