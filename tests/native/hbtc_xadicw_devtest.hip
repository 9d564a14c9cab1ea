// Test-only device harness of the item pass's x-adic multiplication on the redundant 13 x 30 form
// (curve.h xadic_mul_sac8_w over fq_rr.h's relaxed-bound inline-asm blocks): hbtc_xadicw_ops.h, one
// item per lane on 64-lane workgroups, the table's three LDS entries laid out [entry][word][lane] in
// the workgroup's own LDS as in k_rlc_items; the item's lane word is replaced by the lane that runs
// it.  Built with the flags of hbtc_rlc.p6.o (tests/test_gpu_xadicw.py).
#include <hip/hip_runtime.h>

#include "hbtc_xadicw_ops.h"

using namespace hbtc;

__global__ void __launch_bounds__(64) k_xadicw_mul(uint32_t n, const uint32_t* __restrict__ items,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
  __shared__ uint32_t lds[XW_LDS_WORDS];
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t it[XW_ITEM_WORDS], o[XW_OUT_WORDS], f;
  for (uint32_t k = 0; k < XW_ITEM_WORDS; ++k) it[k] = items[XW_ITEM_WORDS * (size_t)i + k];
  it[17] = threadIdx.x;
  xadicw_one(it, o, &f, lds, false);
  for (uint32_t k = 0; k < XW_OUT_WORDS; ++k) out[XW_OUT_WORDS * (size_t)i + k] = o[k];
  flags[i] = f;
}

__global__ void __launch_bounds__(64) k_xadicw_pack(uint32_t n, const uint32_t* __restrict__ in,
                                                    uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t a[13], o[25];
  for (int k = 0; k < 13; ++k) a[k] = in[13 * (size_t)i + k];
  xadicw_roundtrip(a, o);
  for (int k = 0; k < 25; ++k) out[25 * (size_t)i + k] = o[k];
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
int xwd_devices() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : -(int)e;
}

int xwd_mul(uint32_t n, const uint32_t* items, uint32_t* out, uint32_t* flags) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_in = d.up(items, XW_ITEM_WORDS * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, XW_OUT_WORDS * (size_t)n);
  uint32_t* d_flags = d.up<uint32_t>(nullptr, n);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_xadicw_mul, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out, d_flags);
    d.down(out, d_out, XW_OUT_WORDS * (size_t)n);
    d.down(flags, d_flags, n);
  }
  return d.done();
}

int xwd_pack(uint32_t n, const uint32_t* in, uint32_t* out) {
  if (n == 0) return -1;
  Dev d;
  uint32_t* d_in = d.up(in, 13 * (size_t)n);
  uint32_t* d_out = d.up<uint32_t>(nullptr, 25 * (size_t)n);
  if (d.err == hipSuccess) {
    hipLaunchKernelGGL(k_xadicw_pack, dim3((n + 63) / 64), dim3(64), 0, 0, n, d_in, d_out);
    d.down(out, d_out, 25 * (size_t)n);
  }
  return d.done();
}
}  // extern "C"
