// Test-only device harness of the 13 x 30 Fq code (field.h FqR over fq_rr.h's inline-asm product
// and squaring): the operations of hbtc_rr_ops.h, one item per lane, one 64-lane workgroup per 64
// items, and k_rlc_decode's G1 decode with and without the 30-bit square root.  Built with the
// flags of hbtc_rlc.p6.o (tests/test_gpu_rr.py).
#include <hip/hip_runtime.h>

#include "hbtc_rr_ops.h"

using namespace hbtc;

__global__ void __launch_bounds__(64) k_rr_ops(uint32_t n, const uint32_t* __restrict__ ops,
                                               const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                               uint32_t* __restrict__ out, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t la[13], lb[13], lo[13], f;
  for (int k = 0; k < 13; ++k) {
    la[k] = a[13 * (size_t)i + k];
    lb[k] = b[13 * (size_t)i + k];
  }
  rr_apply(ops[i], la, lb, lo, &f);
  for (int k = 0; k < 13; ++k) out[13 * (size_t)i + k] = lo[k];
  flag[i] = f;
}

template <bool RR>
__global__ void __launch_bounds__(64) k_rr_decode(uint32_t n, const uint32_t* __restrict__ c48,
                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[12], o[24], f;
  for (int k = 0; k < 12; ++k) w[k] = c48[12 * (size_t)i + k];
  rr_decode<RR>(w, o, &f);
  for (int k = 0; k < 24; ++k) out[24 * (size_t)i + k] = o[k];
  flags[i] = f;
}

namespace {
struct Dev {
  hipError_t err = hipSuccess;
  void* ptrs[8];
  int np = 0;
  template <typename T>
  T* up(const T* h, size_t count) {
    void* p = nullptr;
    if (err != hipSuccess) return nullptr;
    err = hipMalloc(&p, count ? count * sizeof(T) : 4);
    if (err != hipSuccess) return nullptr;
    ptrs[np++] = p;
    if (h) err = hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
    else err = hipMemset(p, 0, count ? count * sizeof(T) : 4);
    return static_cast<T*>(p);
  }
  template <typename T>
  void down(T* h, const T* d, size_t count) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  int done() {
    for (int i = 0; i < np; ++i) (void)hipFree(ptrs[i]);
    return (int)err;
  }
};
}  // namespace

extern "C" {
int rd_devices() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : -(int)e;
}

int rd_ops(uint32_t n, const uint32_t* ops, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_ops = d.up(ops, n);
  uint32_t* d_a = d.up(a, 13 * (size_t)n);
  uint32_t* d_b = d.up(b, 13 * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, 13 * (size_t)n);
  uint32_t* d_flag = d.up<uint32_t>(nullptr, n);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_rr_ops, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_ops, d_a, d_b, d_out, d_flag);
    d.down(out, d_out, 13 * (size_t)n);
    d.down(flag, d_flag, n);
  }
  return d.done();
}

int rd_decode_g1(uint32_t n, int rr, const uint8_t* c48, uint32_t* out, uint32_t* flags) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_in = d.up(reinterpret_cast<const uint32_t*>(c48), 12 * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, 24 * (size_t)n);
  uint32_t* d_flags = d.up<uint32_t>(nullptr, n);
  if (d.err == hipSuccess) {
    if (rr) hipLaunchKernelGGL(k_rr_decode<true>, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out, d_flags);
    else hipLaunchKernelGGL(k_rr_decode<false>, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out, d_flags);
    d.down(out, d_out, 24 * (size_t)n);
    d.down(flags, d_flags, n);
  }
  return d.done();
}
}  // extern "C"
