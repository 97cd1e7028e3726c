// Activation recomputation (ops.BlockFn, levels "light" and "full"): what the backward rebuilds instead of keeping.  The LayerNorm
// outputs come from octmae_ln_apply (layernorm.hip); this file holds the GELU output rebuilt from the stored pre-activation.
//
// HBM-bound stream: 2 (pre) read + 2 (act) write bytes per element, eight elements (16 bytes) per lane and access, non-temporal both
// ways (each value is touched once), four loads in flight per lane as in cast_f32_bf16_kernel.
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

// gelu_f2 of the 16-bit value, packed the way the fc1 epilogue of gemm.hip packs it: bit-equal to that epilogue's second output
__device__ __forceinline__ u32x4 gelu8(const u32x4 w) {
  u32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x2 y = gelu_f2(f32x2{bflo(w[e]), bfhi(w[e])});
    r[e] = pack2bf(y[0], y[1]);
  }
  return r;
}

__global__ __launch_bounds__(256) void gelu_apply_kernel(const bf16_t* __restrict__ pre, bf16_t* __restrict__ act, size_t n8) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n8; i += 4 * stride) {
    u32x4 w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pre + 8 * (i + u * stride)));
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(gelu8(w[u]), reinterpret_cast<u32x4*>(act + 8 * (i + u * stride)));
  }
  for (; i < n8; i += stride) {
    const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pre + 8 * i));
    __builtin_nontemporal_store(gelu8(w), reinterpret_cast<u32x4*>(act + 8 * i));
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_gelu_apply(const void* pre_bf16, void* act_bf16, long long n, void* stream) {
  OCTMAE_CHECK_ARG(pre_bf16 && act_bf16 && n > 0 && n % 8 == 0);
  // 512 workgroups at the most, two per CU with four loads in flight per lane: the grid of octmae_cast_f32_bf16 (tokens.hip)
  const size_t n8 = (size_t)n / 8;
  size_t blocks = (n8 + 255) / 256;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(gelu_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16_t*>(pre_bf16), reinterpret_cast<bf16_t*>(act_bf16), n8);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
