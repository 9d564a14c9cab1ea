// Device build of the arithmetic headers (hbbft_amd/csrc/*.h) behind a tiny C ABI, so the GPU
// suite can run single field / lane-pair / GT operations on chosen operands and compare them
// with the integer reference of tests/devarith_cases.py.  Test infrastructure only: never linked
// into the product library.
//
// The file is compiled once per product variant of the Fq multiplication (Makefile `devtest`),
// with the product's own flags, and the three objects link into tests/native/libhbtc_devtest.so:
//   sr    -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -DHBTC_GT_INLINE   shared subroutines on fixed registers
//   inl   -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE                the one-block inline product
//   call  (no define)                                          the out-of-line fq_mul_call
// Every kernel and entry point carries the variant's suffix (dt_fq_sr, dt_fq_inl, dt_fq_call, ...).
// Families: Fq (all variants), lane pairs (sr, inl), lazy accumulators and GT on real lanes (sr).
//
// Operands and results are RAW little-endian 32-bit limbs (12 per Fq), no Montgomery conversion,
// so the tests can feed lazy representatives in [p, 2p).  Every entry returns 0, -1 for a
// malformed request, or the first failing HIP call's status.
#include <hip/hip_runtime.h>

#include <vector>

#include "pair.h"
#if defined(HBTC_FQMUL_SR)
#include "gt6.h"
#define DT_SFX sr
#define DT_PAIR 1
#define DT_SR 1
#elif defined(HBTC_FQMUL_INLINE)
#define DT_SFX inl
#define DT_PAIR 1
#define DT_SR 0
#else
#define DT_SFX call
#define DT_PAIR 0
#define DT_SR 0
#endif
#define DT_CAT2(a, b) a##_##b
#define DT_CAT(a, b) DT_CAT2(a, b)
#define DT_NAME(x) DT_CAT(x, DT_SFX)

using namespace hbtc;

namespace {

constexpr uint32_t MILLER_LINES = 68;  // pair.h g2p_walk_lines: 63 doublings + 5 additions

// device buffers of one request; the first failing HIP status sticks
struct Dev {
  std::vector<void*> bufs;
  hipError_t err = hipSuccess;
  template <class T>
  T* up(const void* host, size_t bytes) {  // host == nullptr: zero-filled
    if (err != hipSuccess) return nullptr;
    void* p = nullptr;
    err = hipMalloc(&p, bytes ? bytes : 4);
    if (err != hipSuccess) return nullptr;
    bufs.push_back(p);
    if (bytes) err = host ? hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
    return static_cast<T*>(p);
  }
  void down(void* host, const void* dev, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  int done() {
    for (void* p : bufs) {
      const hipError_t e = hipFree(p);
      if (err == hipSuccess) err = e;
    }
    return (int)err;
  }
};

}  // namespace

// number of visible devices, or minus the HIP status of the query
extern "C" int DT_NAME(dt_devices)() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : -(int)e;
}

// ------------------------------------------------------------------------------------------ Fq
// One item per lane.  Lanes past n leave before the operation, so in the last block the product
// subroutines / calls run under a partial EXEC mask; the per-item op code diverges waves at the
// seams between operations.
__global__ void __launch_bounds__(64)
DT_NAME(k_dt_fq)(uint32_t n, const uint32_t* ops, const Fq* a, const Fq* b, const Fq* c, const Fq* d,
                 Fq* out, uint32_t* flag) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const Fq A = a[i], B = b[i];
  Fq r;
  fq_zero(r);
  uint32_t f = 0;
  switch (ops[i]) {
    case 0: fq_mul(r, A, B); break;
    case 1: fq_sqr(r, A); break;
    case 2: fq_mul_ol(r, A, B); break;
    case 3: fq_add(r, A, B); break;
    case 4: fq_sub(r, A, B); break;
    case 5: fq_dbl(r, A); break;
    case 6: fq_neg(r, A); break;
    case 7: fq_canon(r, A); break;
    case 8: f = fq_is_zero(A); break;
    case 9: f = fq_eq(A, B); break;
    case 10: fq_from_mont(r, A); break;
    case 11: f = fq_is_lex_largest(A); break;
    case 12: fq_inv_binary(r, A); break;
    case 13: f = fq_sqrt(r, A); break;
    default: fq_mul2(r, A, B, c[i], d[i]); break;
  }
  out[i] = r;
  flag[i] = f;
}

extern "C" int DT_NAME(dt_fq)(uint32_t n, const uint32_t* ops, const uint32_t* a, const uint32_t* b,
                              const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t* flag) {
  if (n == 0) return -1;
  for (uint32_t i = 0; i < n; ++i)
    if (ops[i] > 14) return -1;
  Dev dv;
  const size_t fb = sizeof(Fq) * n;
  uint32_t* d_ops = dv.up<uint32_t>(ops, 4 * (size_t)n);
  Fq* d_a = dv.up<Fq>(a, fb);
  Fq* d_b = dv.up<Fq>(b, fb);
  Fq* d_c = dv.up<Fq>(c, fb);
  Fq* d_d = dv.up<Fq>(d, fb);
  Fq* d_out = dv.up<Fq>(nullptr, fb);
  uint32_t* d_flag = dv.up<uint32_t>(nullptr, 4 * (size_t)n);
  if (dv.err == hipSuccess) {
    hipLaunchKernelGGL(DT_NAME(k_dt_fq), dim3((n + 63) / 64), dim3(64), 0, 0, n, d_ops, d_a, d_b, d_c,
                       d_d, d_out, d_flag);
    dv.launched();
  }
  dv.down(out, d_out, fb);
  dv.down(flag, d_flag, 4 * (size_t)n);
  return dv.done();
}

#if DT_SR
// --------------------------------------------------------------------------- lazy accumulators
// 12 operand slots per item in a and b.  mode 0: nt x fq_acc_mac -> fq_acc_redc (out0);
// 1: nt x fq_acc_mac2 -> fq_acc_redc2 (out1); 2: x = 0, y = 24 p^2, nt x fq_acc_macsub;
// 3: x = y = 24 p^2, nt x fq_acc_subsub; 4 (the GT code's Karatsuba form): x = 24 p^2, y = 0,
// nt x fq_acc_kara with term t in slots 2t, 2t + 1 (a0, a1 / b0, b1).  out0 = redc(x),
// out1 = redc2(y).  nt differs per lane: the subroutines run under partial EXEC masks.
__global__ void __launch_bounds__(64)
DT_NAME(k_dt_acc)(uint32_t n, const uint32_t* mode, const uint32_t* nt, const Fq* a, const Fq* b,
                  Fq* out0, Fq* out1) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = mode[i], cnt = nt[i];
  const Fq* pa = a + 12 * (size_t)i;
  const Fq* pb = b + 12 * (size_t)i;
  FqAcc x, y;
  fq_acc_zero(x);
  fq_acc_zero(y);
  if (m == 3 || m == 4) fq_acc_k24(x);
  if (m == 2 || m == 3) fq_acc_k24(y);
#pragma unroll 1
  for (uint32_t t = 0; t < cnt; ++t) {
    switch (m) {
      case 0: fq_acc_mac(x, pa[t], pb[t]); break;
      case 1: fq_acc_mac2(y, pa[t], pb[t]); break;
      case 2: fq_acc_macsub(x, y, pa[t], pb[t]); break;
      case 3: fq_acc_subsub(x, y, pa[t], pb[t]); break;
      default: fq_acc_kara(x, y, pa[2 * t], pa[2 * t + 1], pb[2 * t], pb[2 * t + 1]); break;
    }
  }
  Fq r0, r1;
  fq_acc_redc(r0, x);
  fq_acc_redc2(r1, y);
  out0[i] = r0;
  out1[i] = r1;
}

extern "C" int DT_NAME(dt_acc)(uint32_t n, const uint32_t* mode, const uint32_t* nt, const uint32_t* a,
                               const uint32_t* b, uint32_t* out0, uint32_t* out1) {
  if (n == 0) return -1;
  for (uint32_t i = 0; i < n; ++i)
    if (mode[i] > 4 || nt[i] > (mode[i] == 4 ? 6u : 12u)) return -1;
  Dev dv;
  const size_t fb = sizeof(Fq) * n;
  uint32_t* d_mode = dv.up<uint32_t>(mode, 4 * (size_t)n);
  uint32_t* d_nt = dv.up<uint32_t>(nt, 4 * (size_t)n);
  Fq* d_a = dv.up<Fq>(a, 12 * fb);
  Fq* d_b = dv.up<Fq>(b, 12 * fb);
  Fq* d_o0 = dv.up<Fq>(nullptr, fb);
  Fq* d_o1 = dv.up<Fq>(nullptr, fb);
  if (dv.err == hipSuccess) {
    hipLaunchKernelGGL(DT_NAME(k_dt_acc), dim3((n + 63) / 64), dim3(64), 0, 0, n, d_mode, d_nt, d_a, d_b,
                       d_o0, d_o1);
    dv.launched();
  }
  dv.down(out0, d_o0, fb);
  dv.down(out1, d_o1, fb);
  return dv.done();
}
#endif  // DT_SR

#if DT_PAIR
// ---------------------------------------------------------------------------------- lane pairs
// item = lane / 2 (pair.h: lane 2j + e holds component c_e).  Items sit at even and odd pair
// slots; lanes past the last item leave in whole pairs.
__global__ void __launch_bounds__(64)
DT_NAME(k_dt_f2)(uint32_t n, const uint32_t* ops, const Fq2* a, const Fq2* b, const Fq* c, Fq2* out,
                 uint32_t* flag) {
  const uint32_t i = (blockIdx.x * 64 + threadIdx.x) >> 1;
  if (i >= n) return;
  Fq2p A, B, r;
  fq2p_load(A, a + i);
  fq2p_load(B, b + i);
  fzero(r);
  bool f = false;
  switch (ops[i]) {
    case 0: fmul(r, A, B); break;
    case 1: fsqr(r, A); break;
    case 2: finv_fast(r, A); break;
    case 3: fconj(r, A); break;
    case 4: fneg(r, A); break;
    case 5: f = fis_zero(A); break;
    case 6: f = feq(A, B); break;
    case 7: fmul_by_fq(r, A, c[i]); break;
    default: fone(r); break;
  }
  fq2p_store(out + i, r);
  if (!pair_odd()) flag[i] = f ? 1u : 0u;
}

extern "C" int DT_NAME(dt_f2)(uint32_t n, const uint32_t* ops, const uint32_t* a, const uint32_t* b,
                              const uint32_t* c, uint32_t* out, uint32_t* flag) {
  if (n == 0) return -1;
  for (uint32_t i = 0; i < n; ++i)
    if (ops[i] > 8) return -1;
  Dev dv;
  const size_t f2b = sizeof(Fq2) * n;
  uint32_t* d_ops = dv.up<uint32_t>(ops, 4 * (size_t)n);
  Fq2* d_a = dv.up<Fq2>(a, f2b);
  Fq2* d_b = dv.up<Fq2>(b, f2b);
  Fq* d_c = dv.up<Fq>(c, sizeof(Fq) * n);
  Fq2* d_out = dv.up<Fq2>(nullptr, f2b);
  uint32_t* d_flag = dv.up<uint32_t>(nullptr, 4 * (size_t)n);
  if (dv.err == hipSuccess) {
    hipLaunchKernelGGL(DT_NAME(k_dt_f2), dim3((2 * n + 63) / 64), dim3(64), 0, 0, n, d_ops, d_a, d_b, d_c,
                       d_out, d_flag);
    dv.launched();
  }
  dv.down(out, d_out, f2b);
  dv.down(flag, d_flag, 4 * (size_t)n);
  return dv.done();
}

// G2 in pair form.  aff: G2A (x, y, inf: 49 words), j1 / j2 / out: G2J (72 words).
//   0 jac_dbl(j1)  1 jac_add_aff(j1, aff)  2 jac_add(j1, j2)  3 g2p_psi(aff) (out.z = 1)
//   4 g2p_psi_jac(j1)  5 g2p_walk_lines(aff) (out = T = [|x|] aff, flag = g2p_psi_test)
//   6 g2p_clear_cofactor(aff)
// lines: 68 x 3 Fq2 per item, written by op 5 (the projective line triples), zero elsewhere.
__global__ void __launch_bounds__(64)
DT_NAME(k_dt_g2)(uint32_t n, const uint32_t* ops, const G2A* aff, const G2J* j1, const G2J* j2, G2J* out,
                 uint32_t* flag, Fq2* lines) {
  const uint32_t i = (blockIdx.x * 64 + threadIdx.x) >> 1;
  if (i >= n) return;
  G2Ap P;
  G2Jp A, B, r;
  g2p_load_aff(P, aff + i);
  g2p_load_jac(A, j1 + i);
  g2p_load_jac(B, j2 + i);
  jac_set_inf(r);
  bool f = false;
  switch (ops[i]) {
    case 0: jac_dbl(r, A); break;
    case 1: jac_add_aff(r, A, P); break;
    case 2: jac_add(r, A, B); break;
    case 3:
      g2p_psi(r.x, r.y, P);
      fone(r.z);
      break;
    case 4: g2p_psi_jac(r, A); break;
    case 5:
      g2p_walk_lines(lines + 3 * MILLER_LINES * (size_t)i, r, P);
      f = g2p_psi_test(r, P);
      break;
    default: g2p_clear_cofactor(r, P); break;
  }
  g2p_store_jac(out + i, r);
  if (!pair_odd()) flag[i] = f ? 1u : 0u;
}

extern "C" int DT_NAME(dt_g2)(uint32_t n, const uint32_t* ops, const uint32_t* aff, const uint32_t* j1,
                              const uint32_t* j2, uint32_t* out, uint32_t* flag, uint32_t* lines) {
  static_assert(sizeof(G2A) == 4 * 49 && sizeof(G2J) == 4 * 72, "marshalling layout");
  if (n == 0) return -1;
  for (uint32_t i = 0; i < n; ++i) {
    if (ops[i] > 6) return -1;
    // op 5 walks the Miller lines of a point that is not infinity (pair.h precondition)
    if (ops[i] == 5 && aff[49 * (size_t)i + 48] != 0) return -1;
  }
  Dev dv;
  uint32_t* d_ops = dv.up<uint32_t>(ops, 4 * (size_t)n);
  G2A* d_aff = dv.up<G2A>(aff, sizeof(G2A) * n);
  G2J* d_j1 = dv.up<G2J>(j1, sizeof(G2J) * n);
  G2J* d_j2 = dv.up<G2J>(j2, sizeof(G2J) * n);
  G2J* d_out = dv.up<G2J>(nullptr, sizeof(G2J) * n);
  uint32_t* d_flag = dv.up<uint32_t>(nullptr, 4 * (size_t)n);
  Fq2* d_lines = dv.up<Fq2>(nullptr, sizeof(Fq2) * 3 * MILLER_LINES * n);
  if (dv.err == hipSuccess) {
    hipLaunchKernelGGL(DT_NAME(k_dt_g2), dim3((2 * n + 63) / 64), dim3(64), 0, 0, n, d_ops, d_aff, d_j1,
                       d_j2, d_out, d_flag, d_lines);
    dv.launched();
  }
  dv.down(out, d_out, sizeof(G2J) * n);
  dv.down(flag, d_flag, 4 * (size_t)n);
  dv.down(lines, d_lines, sizeof(Fq2) * 3 * MILLER_LINES * n);
  return dv.done();
}
#endif  // DT_PAIR

#if DT_SR
// ------------------------------------------------------------------------------ GT on real lanes
// One wave per block (gt6.h: the LDS stage is one array per wave).  rep = 1: 10 groups of 6 lanes
// per wave, lanes 60..63 a partial group; rep = 3: 3 groups of 18.  A block runs ONE operation
// (blk_op) on blk_cnt live groups, items blk_first .. blk_first + blk_cnt - 1; the idle groups and
// the partial group repeat the last live item (every lane takes part in every exchange) and store
// nothing.  a, b: six Fq2 coefficients f_0..f_5 per item; out: rep copies per item (one per
// sub-lane: [item][sub][k]), which must agree.
__global__ void __launch_bounds__(64)
DT_NAME(k_dt_gt)(uint32_t rep, const uint32_t* blk_op, const uint32_t* blk_first, const uint32_t* blk_cnt,
                 const Fq2* a, const Fq2* b, Fq2* out) {
  const gt::Pos ps = gt::pos(rep);
  const uint32_t gs = 6u * rep;
  const uint32_t g = threadIdx.x / gs;
  const uint32_t cnt = blk_cnt[blockIdx.x];
  const bool live = g < cnt;
  const uint32_t item = blk_first[blockIdx.x] + (live ? g : cnt - 1);
  const Fq2 x = a[6 * (size_t)item + ps.k], y = b[6 * (size_t)item + ps.k];
  Fq2 r;
  switch (blk_op[blockIdx.x]) {  // block-uniform
    case 0: gt::mul(r, x, y, ps); break;
    case 1: gt::sqr(r, x, ps); break;
    case 2: r = x; gt::cyc_sqr(r, ps); break;
    case 3: r = x; gt::frob(r, 1, ps); break;
    case 4: r = x; gt::frob(r, 2, ps); break;
    case 5: r = x; gt::frob(r, 3, ps); break;
    case 6: r = x; gt::conj(r, ps); break;
    case 7: gt::final_exp(r, x, ps); break;
    case 8: gt::easy_part(r, x, ps); break;
    default: gt::exp_by_x(r, x, ps); break;
  }
  if (live) out[(rep * (size_t)item + ps.sub) * 6 + ps.k] = r;
}

extern "C" int DT_NAME(dt_gt)(uint32_t nblk, uint32_t nitems, uint32_t rep, const uint32_t* blk_op,
                              const uint32_t* blk_first, const uint32_t* blk_cnt, const uint32_t* a,
                              const uint32_t* b, uint32_t* out) {
  if (nblk == 0 || nitems == 0 || (rep != 1 && rep != 3)) return -1;
  const uint32_t full = 64u / (6u * rep);  // whole groups in a wave: 10 or 3
  for (uint32_t i = 0; i < nblk; ++i)
    if (blk_op[i] > 9 || blk_cnt[i] == 0 || blk_cnt[i] > full || blk_first[i] >= nitems ||
        blk_cnt[i] > nitems - blk_first[i])
      return -1;
  Dev dv;
  const size_t ib = sizeof(Fq2) * 6 * nitems;
  uint32_t* d_op = dv.up<uint32_t>(blk_op, 4 * (size_t)nblk);
  uint32_t* d_first = dv.up<uint32_t>(blk_first, 4 * (size_t)nblk);
  uint32_t* d_cnt = dv.up<uint32_t>(blk_cnt, 4 * (size_t)nblk);
  Fq2* d_a = dv.up<Fq2>(a, ib);
  Fq2* d_b = dv.up<Fq2>(b, ib);
  Fq2* d_out = dv.up<Fq2>(nullptr, ib * rep);
  if (dv.err == hipSuccess) {
    hipLaunchKernelGGL(DT_NAME(k_dt_gt), dim3(nblk), dim3(64), 0, 0, rep, d_op, d_first, d_cnt, d_a, d_b,
                       d_out);
    dv.launched();
  }
  dv.down(out, d_out, ib * rep);
  return dv.done();
}
#endif  // DT_SR
