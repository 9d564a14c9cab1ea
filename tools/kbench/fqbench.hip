// Fq Montgomery-multiplication shape microbenchmark for gfx950 (tool, not product code).
// Variants: rolled CIOS (round-1 default), fully unrolled CIOS, and product-scanning (FIPS)
// with the 64-bit multiply-add's carry-out feeding a 32-bit column-overflow counter
// (grouped inline-asm MACs), and the carry-free 13 x 30 product / squaring of fq_rr.h against the
// one-block 12 x 32 forms at 1 / 2 / 3 waves per SIMD, and one jac_dbl step on 12 x 32 (curve.h jac_dbl)
// against the redundant 13 x 30 form (jacw_dbl) at the same occupancies (for this A/B build with
// -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE, the flags of k_rlc_decode's object: the 12 x 32 doubling then
// has its products inlined as in that kernel), and one column of k_rlc_items' double-and-add (doubling,
// select tree over five register and three LDS entries, mixed addition) on 12 x 32 against the packed
// table + redundant form of xadic_mul_sac8_w, on 64-lane workgroups as in that kernel.  Prints time, Fqm/s and the fraction of the measured
// v_mad_u64_u32 roofline (29.51e12 / 288 Fqm/s), plus a cross-check of the three results.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "curve.h"
#include "fq_fips.h"
#include "fq_fips_asm.h"
using namespace hbtc;
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)
constexpr int ITERS = 512;

// V 0-2: products (rolled / unrolled CIOS, C++-glued FIPS); 3: one-block asm FIPS product;
// 4: squaring through the FIPS product; 5: one-block asm FIPS squaring (b ignored); 6 / 7: the
// product / squaring as the shared subroutine of fq_fips_sr.h (build with -DHBTC_FQMUL_SR)
template <int V>
__device__ __forceinline__ void mulv(Fq& r, const Fq& a, const Fq& b) {
  if constexpr (V == 0) mont_mul<12, 1>(r, a, b, FQ_P, FQ_NP);
  else if constexpr (V == 1) mont_mul<12, 12>(r, a, b, FQ_P, FQ_NP);
  else if constexpr (V == 2) mont_mul_fips(r.v, a.v, b.v, FQ_P, FQ_NP);
  else if constexpr (V == 4) mont_mul_fips(r.v, a.v, a.v, FQ_P, FQ_NP);
#if defined(__HIP_DEVICE_COMPILE__)
  else if constexpr (V == 3) fips::mont_mul_asm(r.v, a.v, b.v);
  else if constexpr (V == 5) fips::mont_sqr_asm(r.v, a.v);
#if defined(HBTC_FQMUL_SR)
  else if constexpr (V == 6) fips::mont_mul_sr(r.v, a.v, b.v);  // subroutine (fq_fips_sr.h)
  else fips::mont_sqr_sr(r.v, a.v);
#else  // built with -DHBTC_FQMUL_INLINE (the flags of k_rlc_decode's object): 6 / 7 repeat 3 / 5
  else if constexpr (V == 6) fips::mont_mul_asm(r.v, a.v, b.v);
  else fips::mont_sqr_asm(r.v, a.v);
#endif
#endif
}

template <int V, int ILP, int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_mul(const Fq* in, Fq* out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  Fq x[ILP];
  const Fq y = in[(i + 1) & 1023];
#pragma unroll
  for (int j = 0; j < ILP; ++j) x[j] = in[(i + 7 * j) & 1023];
#pragma unroll 1
  for (int it = 0; it < ITERS; ++it)
#pragma unroll
    for (int j = 0; j < ILP; ++j) mulv<V>(x[j], x[j], y);
#pragma unroll
  for (int j = 1; j < ILP; ++j)
#pragma unroll
    for (int l = 0; l < 12; ++l) x[0].v[l] ^= x[j].v[l];
  out[i] = x[0];
}

// The product / squaring of fq_rr.h on field.h's FqR (13 limbs of 30 bits): V 0 product, 1 squaring.
template <int V>
__device__ __forceinline__ void mulr(FqR& r, const FqR& a, const FqR& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (V == 0) rr::mont_mul_asm(r.v, a.v, b.v);
  else rr::mont_sqr_asm(r.v, a.v);
#endif
}
template <int V, int ILP, int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_mul_rr(const FqR* in, FqR* out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  FqR x[ILP];
  const FqR y = in[(i + 1) & 1023];
#pragma unroll
  for (int j = 0; j < ILP; ++j) x[j] = in[(i + 7 * j) & 1023];
#pragma unroll 1
  for (int it = 0; it < ITERS; ++it)
#pragma unroll
    for (int j = 0; j < ILP; ++j) mulr<V>(x[j], x[j], y);
#pragma unroll
  for (int j = 1; j < ILP; ++j)
#pragma unroll
    for (int l = 0; l < 13; ++l) x[0].v[l] ^= x[j].v[l];
  out[i] = x[0];
}
template <int V>
__global__ void k_check_rr(const FqR* in, FqR* out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  FqR r;
  mulr<V>(r, in[i], in[(i * 7 + 3) & 1023]);
  out[i] = r;
}

// One G1 doubling per iteration: V 0 jac_dbl on 12 x 32 (in: three Fq), V 1 jacw_dbl on the redundant
// 13 x 30 form (in: three entry-bound FqW: limbs < 2^30, below 2^384 < 12p).  N iterations.
constexpr int DBL_ITERS = 128;
template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_dbl12(const Fq* in, Fq* out, int n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  G1J p;
  p.x = in[i & 1023];
  p.y = in[(i + 1) & 1023];
  p.z = in[(i + 2) & 1023];
#pragma unroll 1
  for (int it = 0; it < n; ++it) jac_dbl(p, p);
  fq_canon(out[3 * (size_t)i], p.x);
  fq_canon(out[3 * (size_t)i + 1], p.y);
  fq_canon(out[3 * (size_t)i + 2], p.z);
}
template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_dblw(const FqR* in, FqR* out, int n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  JacW p;
#pragma unroll
  for (int l = 0; l < 13; ++l) {
    p.x.v[l] = in[i & 1023].v[l];
    p.y.v[l] = in[(i + 1) & 1023].v[l];
    p.z.v[l] = in[(i + 2) & 1023].v[l];
  }
#pragma unroll 1
  for (int it = 0; it < n; ++it) jacw_dbl(p, p);
#pragma unroll
  for (int l = 0; l < 13; ++l) {
    out[3 * (size_t)i].v[l] = p.x.v[l];
    out[3 * (size_t)i + 1].v[l] = p.y.v[l];
    out[3 * (size_t)i + 2].v[l] = p.z.v[l];
  }
}

// One COLUMN of k_rlc_items' double-and-add per iteration: a doubling, the select tree over the 8-entry
// table (five entries in registers, three in LDS laid out [entry][word][lane], 64-lane workgroups as in
// the kernel), the sign, the branch-free mixed addition.  RRW false: jac_dbl + jac_madd_generic on 12 x 32
// (curve.h xadic_mul_sac8<Fq, true>'s column); true: the packed table, the selected entry unpacked,
// jacw_dbl + jacw_madd_generic (xadic_mul_sac8_w's column).  The entries are arbitrary field elements
// below 2^380 (the cost does not depend on their being curve points); bit k of `bits` is the column's
// u_(k+1), bit 3 its sign.
constexpr int COL_ITERS = 32;
HD uint32_t col_bits(uint32_t i, int it) { return (i * 2654435761u + (uint32_t)it * 0x9e3779b9u) >> 27; }
HD void col_entry(XY<Fq>& t, const XY<Fq> tab[5], const uint32_t* lds, uint32_t lane, uint32_t bits) {
  const bool b1 = bits & 1u, b2 = bits & 2u, b3 = bits & 4u;
  XY<Fq> e0, e1;
  {
    XY<Fq> a, b;
    xy_sel(a, b1, tab[1], tab[0]);
    xy_sel(b, b1, tab[3], tab[2]);
    xy_sel(e0, b2, b, a);
  }
  {
    const uint32_t j = (b1 ? 1u : 0u) + (b2 ? 2u : 0u);
    const uint32_t li = j ? j - 1u : 0u;
    XY<Fq> l;
    uint32_t* dst = reinterpret_cast<uint32_t*>(&l);
#pragma unroll
    for (int w = 0; w < 24; ++w) dst[w] = lds[(li * 24 + w) * 64 + lane];
    xy_sel(e1, j != 0, l, tab[4]);
  }
  xy_sel(t, b3, e1, e0);
}
HD void col12(G1J& acc, const XY<Fq> tab[5], const uint32_t* lds, uint32_t lane, uint32_t bits) {
  jac_dbl(acc, acc);
  XY<Fq> t;
  col_entry(t, tab, lds, lane, bits);
  Fq ny;
  fneg(ny, t.y);
  fsel(t.y, (bits & 8u) != 0, ny, t.y);
  jac_madd_generic(acc, acc, t.x, t.y);
}
HD void colw(JacW& acc, const XY<Fq> tab[5], const uint32_t* lds, uint32_t lane, uint32_t bits) {
  jacw_dbl(acc, acc);
  XY<Fq> t;
  col_entry(t, tab, lds, lane, bits);
  XYW w;
  xyw_unpack(w, t);
  FqW ny;
  fw_neg(ny, w.y);
  fw_sel(w.y, (bits & 8u) != 0, ny, w.y);
  jacw_madd_generic(acc, acc, w.x, w.y);
}
// the table of item i from the 1024 inputs: entries 0..4 to tab, 5..7 to the lane's LDS column
HD void col_table(XY<Fq> tab[5], uint32_t* lds, uint32_t lane, uint32_t i, const Fq* in) {
  for (int e = 0; e < 8; ++e) {
    XY<Fq> v;
    v.x = in[(i + 2 * e) & 1023];
    v.y = in[(i + 2 * e + 1) & 1023];
    if (e < 5) tab[e] = v;
    else xy_lds_put(lds, lane, e - 5, v);
  }
}
HD void col_run12(uint32_t* o, uint32_t i, uint32_t lane, uint32_t* lds, const Fq* in, int n) {
  XY<Fq> tab[5];
  col_table(tab, lds, lane, i, in);
  G1J p;
  p.x = in[(i + 16) & 1023];
  p.y = in[(i + 17) & 1023];
  p.z = in[(i + 18) & 1023];
#pragma unroll 1
  for (int it = 0; it < n; ++it) col12(p, tab, lds, lane, col_bits(i, it));
  Fq c[3];
  fq_canon(c[0], p.x);
  fq_canon(c[1], p.y);
  fq_canon(c[2], p.z);
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < 12; ++l) o[12 * j + l] = c[j].v[l];
}
HD void col_runw(uint32_t* o, uint32_t i, uint32_t lane, uint32_t* lds, const Fq* in, const FqR* in13, int n) {
  XY<Fq> tab[5];
  col_table(tab, lds, lane, i, in);
  JacW p;
  for (int l = 0; l < 13; ++l) {
    p.x.v[l] = in13[i & 1023].v[l];
    p.y.v[l] = in13[(i + 1) & 1023].v[l];
    p.z.v[l] = in13[(i + 2) & 1023].v[l];
  }
#pragma unroll 1
  for (int it = 0; it < n; ++it) colw(p, tab, lds, lane, col_bits(i, it));
  for (int l = 0; l < 13; ++l) {
    o[l] = p.x.v[l];
    o[13 + l] = p.y.v[l];
    o[26 + l] = p.z.v[l];
  }
}
template <int WAVES, bool RRW>
__global__ void __launch_bounds__(64, WAVES) k_col(const Fq* in, const FqR* in13, uint32_t* out, int n) {
  __shared__ uint32_t lds[3 * 24 * 64];
  const uint32_t lane = threadIdx.x, i = blockIdx.x * 64 + lane;
  uint32_t o[39];
  if constexpr (RRW) {
    col_runw(o, i, lane, lds, in, in13, n);
    for (int k = 0; k < 39; ++k) out[39 * (size_t)i + k] = o[k];
  } else {
    col_run12(o, i, lane, lds, in, n);
    for (int k = 0; k < 36; ++k) out[36 * (size_t)i + k] = o[k];
  }
}

template <int V>
__global__ void k_check(const Fq* in, Fq* out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  Fq r;
  mulv<V>(r, in[i], in[(i * 7 + 3) & 1023]);
  Fq c;
  fq_canon(c, r);
  out[i] = c;
}

int main() {
  hipDeviceProp_t prop;
  CHK(hipGetDeviceProperties(&prop, 0));
  printf("device %s CUs=%d\n", prop.gcnArchName, prop.multiProcessorCount);
  std::vector<Fq> h(1024);
  uint64_t s = 0x1234567;
  for (auto& f : h) {
    for (int l = 0; l < 12; ++l) { s = s * 6364136223846793005ull + 1442695040888963407ull; f.v[l] = (uint32_t)(s >> 32); }
    f.v[11] &= 0x0fffffffu;  // < 2^380 < 2p
  }
  Fq *d_in, *d_out;
  const int nthreads = 256 * 2048;
  CHK(hipMalloc(&d_in, sizeof(Fq) * 1024));
  CHK(hipMalloc(&d_out, sizeof(Fq) * 3 * nthreads));
  CHK(hipMemcpy(d_in, h.data(), sizeof(Fq) * 1024, hipMemcpyHostToDevice));
  // cross-check
  std::vector<Fq> rv[8];
  auto chk = [&](auto kern, int v) {
    rv[v].resize(1024);
    hipLaunchKernelGGL(kern, dim3(16), dim3(64), 0, 0, d_in, d_out);
    CHK(hipMemcpy(rv[v].data(), d_out, sizeof(Fq) * 1024, hipMemcpyDeviceToHost));
  };
  chk(k_check<0>, 0);
  chk(k_check<1>, 1);
  chk(k_check<2>, 2);
  chk(k_check<3>, 3);
  chk(k_check<4>, 4);
  chk(k_check<5>, 5);
  chk(k_check<6>, 6);
  chk(k_check<7>, 7);
  int bad = 0, bad_sq = 0;
  for (int i = 0; i < 1024; ++i) {
    Fq hr, hs;
    mont_mul<12, 1>(hr, h[i], h[(i * 7 + 3) & 1023], FQ_P, FQ_NP);
    fq_canon(hr, hr);
    mont_mul<12, 1>(hs, h[i], h[i], FQ_P, FQ_NP);
    fq_canon(hs, hs);
    for (int l = 0; l < 12; ++l) {
      for (int v : {0, 1, 2, 3, 6}) bad += rv[v][i].v[l] != hr.v[l];
      for (int v : {4, 5, 7}) bad_sq += rv[v][i].v[l] != hs.v[l];
    }
  }
  printf("cross-check vs host CIOS: products %s (%d limb mismatches), squarings %s (%d)\n",
         bad ? "FAIL" : "ok", bad, bad_sq ? "FAIL" : "ok", bad_sq);
  // the reduced-radix forms: limbs < 2^30, values < 2^384 < 16p; bit-for-bit against the same
  // schedule in plain C++ (rr::mont_mul_cxx / mont_sqr_cxx)
  std::vector<FqR> hr13(1024);
  for (auto& f : hr13) {
    for (int l = 0; l < 13; ++l) { s = s * 6364136223846793005ull + 1442695040888963407ull; f.v[l] = (uint32_t)(s >> 34); }
    f.v[12] &= 0x00ffffffu;
  }
  FqR *d_in13, *d_out13;
  CHK(hipMalloc(&d_in13, sizeof(FqR) * 1024));
  CHK(hipMalloc(&d_out13, sizeof(FqR) * 3 * nthreads));
  CHK(hipMemcpy(d_in13, hr13.data(), sizeof(FqR) * 1024, hipMemcpyHostToDevice));
  {
    std::vector<FqR> got(1024);
    int bad_rr[2] = {0, 0};
    for (int v = 0; v < 2; ++v) {
      if (v == 0) hipLaunchKernelGGL(k_check_rr<0>, dim3(16), dim3(64), 0, 0, d_in13, d_out13);
      else hipLaunchKernelGGL(k_check_rr<1>, dim3(16), dim3(64), 0, 0, d_in13, d_out13);
      CHK(hipMemcpy(got.data(), d_out13, sizeof(FqR) * 1024, hipMemcpyDeviceToHost));
      for (int i = 0; i < 1024; ++i) {
        FqR want;
        if (v == 0) rr::mont_mul_cxx(want.v, hr13[i].v, hr13[(i * 7 + 3) & 1023].v);
        else rr::mont_sqr_cxx(want.v, hr13[i].v);
        for (int l = 0; l < 13; ++l) bad_rr[v] += got[i].v[l] != want.v[l];
      }
    }
    printf("cross-check 13x30 vs host schedule: product %s (%d limb mismatches), squaring %s (%d)\n",
           bad_rr[0] ? "FAIL" : "ok", bad_rr[0], bad_rr[1] ? "FAIL" : "ok", bad_rr[1]);
  }
  hipEvent_t a, b;
  CHK(hipEventCreate(&a));
  CHK(hipEventCreate(&b));
  const double peak = 29.51e12 / 288.0;
  auto run = [&](const char* name, auto kern, int blocks, int ilp) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d_in, d_out);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(a));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d_in, d_out);
    CHK(hipEventRecord(b));
    CHK(hipEventSynchronize(b));
    float ms;
    CHK(hipEventElapsedTime(&ms, a, b));
    const double fqm = (double)blocks * 256 * ITERS * ilp;
    printf("%-40s blocks=%5d %8.3f ms %9.3e Fqm/s %.3f of mad roofline  %.1f ns/Fqm/wave\n", name, blocks, ms,
           fqm / (ms * 1e-3), fqm / (ms * 1e-3) / peak, ms * 1e6 / (ITERS * ilp));
  };
  auto run13 = [&](const char* name, auto kern, int blocks, int ilp) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d_in13, d_out13);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(a));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d_in13, d_out13);
    CHK(hipEventRecord(b));
    CHK(hipEventSynchronize(b));
    float ms;
    CHK(hipEventElapsedTime(&ms, a, b));
    const double fqm = (double)blocks * 256 * ITERS * ilp;
    printf("%-40s blocks=%5d %8.3f ms %9.3e Fqm/s %.3f of mad roofline  %.1f ns/Fqm/wave\n", name, blocks, ms,
           fqm / (ms * 1e-3), fqm / (ms * 1e-3) / peak, ms * 1e6 / (ITERS * ilp));
  };
  // blocks of 256 threads = 4 waves; 256 CUs x W blocks -> W waves per SIMD
#define RUNV(V, NAME)                                                                   \
  run(NAME " ILP1 1w/SIMD", k_mul<V, 1, 1>, 256, 1);                                   \
  run(NAME " ILP2 1w/SIMD", k_mul<V, 2, 1>, 256, 2);                                   \
  run(NAME " ILP1 2w/SIMD", k_mul<V, 1, 2>, 512, 1);                                   \
  run(NAME " ILP1 4w/SIMD", k_mul<V, 1, 4>, 1024, 1);                                  \
  run(NAME " ILP2 4w/SIMD", k_mul<V, 2, 4>, 1024, 2);                                  \
  run(NAME " ILP1 8w/SIMD", k_mul<V, 1, 8>, 2048, 1);
  RUNV(2, "FIPS asm (C++ glued)")
  RUNV(3, "FIPS one-block asm")
  RUNV(4, "sqr via FIPS product")
  RUNV(5, "sqr one-block asm")
  RUNV(6, "FIPS subroutine (s_swappc)")
  RUNV(7, "sqr subroutine (s_swappc)")
  // 13 x 30 (fq_rr.h) against the one-block 12 x 32 forms above, the same run, 1 / 2 / 3 waves
  // per SIMD (k_rlc_decode runs at 3)
#define RUNW(KERN, V, NAME, RUN)                          \
  RUN(NAME " ILP1 1w/SIMD", (KERN<V, 1, 1>), 256, 1);     \
  RUN(NAME " ILP1 2w/SIMD", (KERN<V, 1, 2>), 512, 1);     \
  RUN(NAME " ILP1 3w/SIMD", (KERN<V, 1, 3>), 768, 1);
  RUNW(k_mul, 3, "A/B 12x32 product (one-block asm)", run)
  RUNW(k_mul_rr, 0, "A/B 13x30 product (fq_rr.h)", run13)
  RUNW(k_mul, 5, "A/B 12x32 squaring (one-block asm)", run)
  RUNW(k_mul_rr, 1, "A/B 13x30 squaring (fq_rr.h)", run13)
  // one G1 doubling: 4 doublings cross-checked against the host build of the same functions (canonical
  // limbs for 12 x 32; the redundant form bit for bit, its host product being the same schedule)
  {
    const int K = 4;
    std::vector<Fq> g12(3 * 256);
    std::vector<FqR> gw(3 * 256);
    hipLaunchKernelGGL(k_dbl12<1>, dim3(1), dim3(256), 0, 0, d_in, d_out, K);
    CHK(hipMemcpy(g12.data(), d_out, sizeof(Fq) * 3 * 256, hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(k_dblw<1>, dim3(1), dim3(256), 0, 0, d_in13, d_out13, K);
    CHK(hipMemcpy(gw.data(), d_out13, sizeof(FqR) * 3 * 256, hipMemcpyDeviceToHost));
    int bad12 = 0, badw = 0;
    for (int i = 0; i < 256; ++i) {
      G1J p;
      p.x = h[i & 1023];
      p.y = h[(i + 1) & 1023];
      p.z = h[(i + 2) & 1023];
      JacW q;
      for (int l = 0; l < 13; ++l) {
        q.x.v[l] = hr13[i & 1023].v[l];
        q.y.v[l] = hr13[(i + 1) & 1023].v[l];
        q.z.v[l] = hr13[(i + 2) & 1023].v[l];
      }
      for (int k = 0; k < K; ++k) {
        jac_dbl(p, p);
        jacw_dbl(q, q);
      }
      Fq c[3];
      fq_canon(c[0], p.x);
      fq_canon(c[1], p.y);
      fq_canon(c[2], p.z);
      const FqW* w[3] = {&q.x, &q.y, &q.z};
      for (int j = 0; j < 3; ++j) {
        for (int l = 0; l < 12; ++l) bad12 += g12[3 * i + j].v[l] != c[j].v[l];
        for (int l = 0; l < 13; ++l) badw += gw[3 * i + j].v[l] != w[j]->v[l];
      }
    }
    printf("cross-check jac_dbl vs host: 12x32 %s (%d limb mismatches), redundant 13x30 %s (%d)\n",
           bad12 ? "FAIL" : "ok", bad12, badw ? "FAIL" : "ok", badw);
  }
  auto rund = [&](const char* name, auto launch, int blocks) {
    launch(blocks);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(a));
    launch(blocks);
    CHK(hipEventRecord(b));
    CHK(hipEventSynchronize(b));
    float ms;
    CHK(hipEventElapsedTime(&ms, a, b));
    printf("%-40s blocks=%5d %8.3f ms %9.3e doublings/s\n", name, blocks, ms,
           (double)blocks * 256 * DBL_ITERS / (ms * 1e-3));
  };
#define RUND(W)                                                                                              \
  rund("A/B jac_dbl 12x32 " #W "w/SIMD",                                                                     \
       [&](int bl) { hipLaunchKernelGGL(k_dbl12<W>, dim3(bl), dim3(256), 0, 0, d_in, d_out, DBL_ITERS); }, 256 * W); \
  rund("A/B jacw_dbl 13x30 redundant " #W "w/SIMD",                                                          \
       [&](int bl) { hipLaunchKernelGGL(k_dblw<W>, dim3(bl), dim3(256), 0, 0, d_in13, d_out13, DBL_ITERS); }, 256 * W);
  RUND(1)
  RUND(2)
  RUND(3)
  // one column of k_rlc_items (64-lane workgroups, 18,432 B of LDS each): 4 columns of 64 lanes
  // cross-checked against the host build of the same functions, then 12 x 32 against the redundant form in
  // the same run; blocks = 256 CUs x 4 SIMDs x W
  {
    const int K = 4;
    std::vector<uint32_t> g12(36 * 64), gw(39 * 64), lds(3 * 24 * 64);
    uint32_t* o12 = reinterpret_cast<uint32_t*>(d_out);
    uint32_t* ow = reinterpret_cast<uint32_t*>(d_out13);
    hipLaunchKernelGGL((k_col<1, false>), dim3(1), dim3(64), 0, 0, d_in, d_in13, o12, K);
    CHK(hipMemcpy(g12.data(), o12, 4 * 36 * 64, hipMemcpyDeviceToHost));
    hipLaunchKernelGGL((k_col<1, true>), dim3(1), dim3(64), 0, 0, d_in, d_in13, ow, K);
    CHK(hipMemcpy(gw.data(), ow, 4 * 39 * 64, hipMemcpyDeviceToHost));
    int bad12 = 0, badw = 0;
    for (uint32_t i = 0; i < 64; ++i) {
      uint32_t o[39];
      col_run12(o, i, i, lds.data(), h.data(), K);
      for (int k = 0; k < 36; ++k) bad12 += o[k] != g12[36 * i + k];
      col_runw(o, i, i, lds.data(), h.data(), hr13.data(), K);
      for (int k = 0; k < 39; ++k) badw += o[k] != gw[39 * i + k];
    }
    printf("cross-check column vs host: 12x32 %s (%d limb mismatches), redundant 13x30 %s (%d)\n",
           bad12 ? "FAIL" : "ok", bad12, badw ? "FAIL" : "ok", badw);
    auto runc = [&](const char* name, auto launch, int blocks) {
      launch(blocks);
      CHK(hipDeviceSynchronize());
      CHK(hipEventRecord(a));
      launch(blocks);
      CHK(hipEventRecord(b));
      CHK(hipEventSynchronize(b));
      float ms;
      CHK(hipEventElapsedTime(&ms, a, b));
      printf("%-40s blocks=%5d %8.3f ms %9.3e columns/s\n", name, blocks, ms,
             (double)blocks * 64 * COL_ITERS / (ms * 1e-3));
    };
#define RUNC(W)                                                                                                   \
  runc("A/B column 12x32 " #W "w/SIMD",                                                                           \
       [&](int bl) { hipLaunchKernelGGL((k_col<W, false>), dim3(bl), dim3(64), 0, 0, d_in, d_in13, o12, COL_ITERS); }, \
       1024 * W);                                                                                                 \
  runc("A/B column 13x30 redundant " #W "w/SIMD",                                                                 \
       [&](int bl) { hipLaunchKernelGGL((k_col<W, true>), dim3(bl), dim3(64), 0, 0, d_in, d_in13, ow, COL_ITERS); },  \
       1024 * W);
    RUNC(1)
    RUNC(2)
    RUNC(3)
  }
  return 0;
}
