// Test-only device harness of the redundant 13 x 30 form (field.h FqW over fq_rr.h's relaxed-bound
// inline-asm blocks, curve.h jacw_*): the operations of hbtc_rrw_ops.h, one item per lane, one
// 64-lane workgroup per 64 items, and the subgroup test with both chains on the redundant form beside
// the 12 x 32 one.  Built with the flags of hbtc_rlc.p6.o (tests/test_gpu_rrw.py).
#include <hip/hip_runtime.h>

#include "hbtc_rrw_ops.h"

using namespace hbtc;

__global__ void __launch_bounds__(64) k_rrw_ops(uint32_t n, const uint32_t* __restrict__ ops,
                                                const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t li[78], lo[39], f;
  for (int k = 0; k < 78; ++k) li[k] = in[78 * (size_t)i + k];
  rrw_apply(ops[i], li, lo, &f);
  for (int k = 0; k < 39; ++k) out[39 * (size_t)i + k] = lo[k];
  flag[i] = f;
}

__global__ void __launch_bounds__(64) k_rrw_subgroup(uint32_t n, const uint32_t* __restrict__ c48,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[12], o[72], f;
  for (int k = 0; k < 12; ++k) w[k] = c48[12 * (size_t)i + k];
  rrw_subgroup_one(w, o, &f);
  for (int k = 0; k < 72; ++k) out[72 * (size_t)i + k] = o[k];
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
int rwd_devices() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : -(int)e;
}

int rwd_ops(uint32_t n, const uint32_t* ops, const uint32_t* in, uint32_t* out, uint32_t* flag) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_ops = d.up(ops, n);
  uint32_t* d_in = d.up(in, 78 * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, 39 * (size_t)n);
  uint32_t* d_flag = d.up<uint32_t>(nullptr, n);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_rrw_ops, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_ops, d_in, d_out, d_flag);
    d.down(out, d_out, 39 * (size_t)n);
    d.down(flag, d_flag, n);
  }
  return d.done();
}

int rwd_subgroup(uint32_t n, const uint8_t* c48, uint32_t* out, uint32_t* flags) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_in = d.up(reinterpret_cast<const uint32_t*>(c48), 12 * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, 72 * (size_t)n);
  uint32_t* d_flags = d.up<uint32_t>(nullptr, n);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_rrw_subgroup, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out, d_flags);
    d.down(out, d_out, 72 * (size_t)n);
    d.down(flags, d_flags, n);
  }
  return d.done();
}
}  // extern "C"
