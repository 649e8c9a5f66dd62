// gfx950 check of sfrt::sqrt_cr_normal (sfrt_device.h: v_sqrt_f32, then the root selected by
// the sign bits of the two fma residuals) against the compare-and-select form it replaced,
// kept here as sqrt_cr_normal_selects:
//   - every binary32 pattern from 2^-96 to +inf (0x0f800000 .. 0x7f800000): the same bits;
//   - every pattern of [0, 2^-96), where the two differ once a residual is denormal: the march's
//     pass body only needs rad - q there, which must equal rad - sqrtf(x) for the radii that
//     tests/native/wave_check.hip uses, and +0 must give +0.
// Built and run by tests/test_sqrt_select.py:
//   hipcc --offload-arch=gfx950 -O3 sqrt_select_check.hip -o sqrt_select_check && ./sqrt_select_check
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../sfml-software-raytracer_amd/csrc/sfrt_device.h"

#pragma clang fp contract(off)

__device__ __forceinline__ float sqrt_cr_normal_selects(float x) {
  const float r = __builtin_amdgcn_sqrtf(x);
  const float rm = __uint_as_float(__float_as_uint(r) - 1u);
  const float rp = __uint_as_float(__float_as_uint(r) + 1u);
  float q = __builtin_fmaf(-rm, r, x) <= 0.0f ? rm : r;
  q = __builtin_fmaf(-rp, r, x) > 0.0f ? rp : q;
  return q;
}

constexpr uint32_t kTinyBits = 0x0f800000u;  // 2^-96
constexpr uint32_t kInfBits = 0x7f800000u;

__global__ void k_sweep(unsigned long long* bad) {
  unsigned long long nbad = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t u = (uint64_t)kTinyBits + blockIdx.x * blockDim.x + threadIdx.x; u <= kInfBits; u += stride) {
    const float x = __uint_as_float((uint32_t)u);
    if (__float_as_uint(sfrt::sqrt_cr_normal(x)) != __float_as_uint(sqrt_cr_normal_selects(x))) nbad++;
  }
  if (nbad) atomicAdd(bad, nbad);
}

__global__ void k_tiny(unsigned long long* bad) {
  const float rads[] = {0.01f, 0.0100001f, 0.015625f, 0.0156250019f, 0.5f, 1.0f, 2.0f,
                        3.99999976f, 4.0f, 7.0f, 1.0e6f, 3.0e38f};
  unsigned long long nbad = 0;
  for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < kTinyBits; u += gridDim.x * blockDim.x) {
    const float x = __uint_as_float(u);
    const float q = sfrt::sqrt_cr_normal(x), ref = __builtin_sqrtf(x);
    if (u == 0u && __float_as_uint(q) != 0u) nbad++;
    for (float rad : rads)
      if (__float_as_uint(rad - q) != __float_as_uint(rad - ref)) nbad++;
  }
  if (nbad) atomicAdd(bad, nbad);
}

int main() {
  unsigned long long* d_bad = nullptr;
  unsigned long long sweep = 0, all = 0;
  if (hipMalloc(&d_bad, sizeof(*d_bad)) != hipSuccess) return 2;
  if (hipMemset(d_bad, 0, sizeof(*d_bad)) != hipSuccess) return 2;
  hipLaunchKernelGGL(k_sweep, dim3(8192), dim3(256), 0, 0, d_bad);
  if (hipMemcpy(&sweep, d_bad, sizeof(sweep), hipMemcpyDeviceToHost) != hipSuccess) return 2;
  hipLaunchKernelGGL(k_tiny, dim3(8192), dim3(256), 0, 0, d_bad);
  if (hipMemcpy(&all, d_bad, sizeof(all), hipMemcpyDeviceToHost) != hipSuccess) return 2;
  std::printf("sweep [2^-96, +inf]: %llu values, %llu differ from the select form\n",
              (unsigned long long)(kInfBits - kTinyBits) + 1ull, sweep);
  std::printf("tiny [0, 2^-96): %llu mismatches of rad - q\n", all - sweep);
  std::printf("mismatches=%llu\n", all);
  (void)hipFree(d_bad);
  return all ? 1 : 0;
}
