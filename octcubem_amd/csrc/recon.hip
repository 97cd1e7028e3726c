// Reconstruction volumes of the 3-D MAE's validation pass: the reference's get_visible_images chain (Pre-training/custom_util/misc.py:
// 1225-1299: unpatchify of pred and of the mask, index_select of the frames, untransform_image :727-728, the two blends) as one pass.
//   octmae_mae_compose   pred f32 [B][L][PD] (any batch stride) + imgs f32 [B][1][T][H][W] + mask f32 [B][L]  ->  uint8 [B][4][Tp][H][W]
//                        panels: 0 original frames, 1 masked input, 2 reconstruction, 3 reconstruction pasted with the visible patches
// The walk is mse_kernel's (csrc/tokens.hip): one wave per token, float4 groups along (u, py, px), which are contiguous in pred and four
// adjacent pixels of one image row; the output differs.  No 16-bit operand: the two builds of the library hold the same code.
//   bytes per output voxel: 4 (pred) + 4 (frame) read, 4 x 1 written; denorm reads the target patch twice more (cache-resident)
// Store shape: a lane's float4 group becomes 4 bytes per panel; at p = 16 four lanes fill a 16-byte patch row and the wave's 64 lanes
// cover 16 rows of one frame, so one store instruction writes 16 pieces of 16 bytes, W bytes apart.  The neighbouring tokens (wx + 1,
// the next wave of the same workgroup) write the adjacent pieces of the same lines at about the same time.  That these pieces are
// combined in L2 before they leave it is an ASSUMPTION: no write counter has been collected for this kernel; the end-to-end rate is in
// profiles/recon_bench.txt.  If the stores turn out to be the limit, one wave per row of gw tokens (full 4 W-byte rows per store) is next.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// untransform_image: (int) clip((v * IMG_STD + IMG_MEAN) * 255, 0, 255).  The reference computes it as three tensor ops, so every step is
// rounded on its own; an fma of the first two flips the truncation wherever the exact value lies within an ulp of an integer.  HIP's
// __fmul_rn / __fadd_rn are the plain operators, which the build's -ffp-contract=fast fuses all the same (v_fmamk_f32 in the ISA): the
// empty asm makes the product a value the compiler cannot look through.  A non-finite v gives 0 (the reference's .int() of NaN is undefined).
__device__ __forceinline__ unsigned grey(float v) {
  const float s = (float)(76.03 / 255), m = (float)(45.79 / 255);
  float a = __fmul_rn(v, s);
  asm("" : "+v"(a));
  float t = __fmul_rn(__fadd_rn(a, m), 255.0f);
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return finite_f32(v) ? (unsigned)(int)t : 0u;
}

__device__ __forceinline__ unsigned pack4(unsigned a, unsigned b, unsigned c, unsigned d) { return a | (b << 8) | (c << 16) | (d << 24); }

// the source frame of predicted frame fo; an index from device memory is clamped into the volume
__device__ __forceinline__ int src_frame(const int* __restrict__ frame_idx, int fo, int T) {
  return frame_idx ? min(max(frame_idx[fo], 0), T - 1) : fo;
}

template <bool DENORM>
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ pred, long long pred_bs, const float* __restrict__ imgs,
                                                      const int* __restrict__ frame_idx, const float* __restrict__ mask,
                                                      uint8_t* __restrict__ out, int B, int T, int H, int W, int u_sz, int p, int L,
                                                      int Tp) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int gh = H / p, gw = W / p;
  const int PD = u_sz * p * p;
  const int nq = PD >> 2;  // float4 groups along (u,py,px); contiguous in pred
  const int rows = B * L;
  const size_t panel = (size_t)Tp * H * W;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / L, l = row - b * L;
    const bool removed = mask[row] != 0.0f;
    const int t = l / (gh * gw), hy = (l / gw) % gh, wx = l % gw;
    const float* pr = pred + (size_t)b * (size_t)pred_bs + (size_t)l * PD;
    const float* vol = imgs + (size_t)b * T * H * W;
    // per-patch statistics of the target (the norm_pix branch of the loss: mean, unbiased variance), fp32, two passes
    float mu = 0.f, sd = 1.f;
    if (DENORM) {
      float s = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int px = e % p, py = (e / p) % p, u = e / (p * p);
        const int f = src_frame(frame_idx, t * u_sz + u, T);
        const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
        s += (iv[0] + iv[1]) + (iv[2] + iv[3]);
      }
      mu = wave_sum(s) / (float)PD;
      float s2 = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int px = e % p, py = (e / p) % p, u = e / (p * p);
        const int f = src_frame(frame_idx, t * u_sz + u, T);
        const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
#pragma unroll
        for (int k = 0; k < 4; ++k) s2 = fmaf(iv[k] - mu, iv[k] - mu, s2);
      }
      sd = sqrtf(wave_sum(s2) / (float)(PD - 1) + 1.0e-6f);
    }
    for (int q = lane; q < nq; q += 64) {
      const int e = 4 * q;
      const int px = e % p, py = (e / p) % p, u = e / (p * p);
      const int fo = t * u_sz + u;
      const int f = src_frame(frame_idx, fo, T);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pr + e);
      const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
      unsigned gx[4], gp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gx[k] = grey(iv[k]);
        gp[k] = grey(DENORM ? __fmaf_rn(pv[k], sd, mu) : pv[k]);
      }
      const unsigned wx4 = pack4(gx[0], gx[1], gx[2], gx[3]), wp4 = pack4(gp[0], gp[1], gp[2], gp[3]);
      uint8_t* o = out + (size_t)b * 4 * panel + ((size_t)fo * H + hy * p + py) * W + wx * p + px;
      *reinterpret_cast<unsigned*>(o) = wx4;
      *reinterpret_cast<unsigned*>(o + panel) = removed ? 0u : wx4;
      *reinterpret_cast<unsigned*>(o + 2 * panel) = wp4;
      *reinterpret_cast<unsigned*>(o + 3 * panel) = removed ? wp4 : wx4;
    }
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_mae_compose(const float* pred, long long pred_batch_stride, const float* imgs, const int* frame_idx,
                                  const float* mask, uint8_t* out, int B, int T, int H, int W, int u_sz, int p, int L, int denorm,
                                  void* stream) {
  OCTMAE_CHECK_ARG(pred && imgs && mask && out);
  OCTMAE_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && u_sz > 0 && p > 0 && L > 0);
  OCTMAE_CHECK_ARG(p % 4 == 0 && W % 4 == 0 && H % p == 0 && W % p == 0);
  const long long PD = (long long)u_sz * p * p, grid = (long long)(H / p) * (W / p);
  OCTMAE_CHECK_ARG(PD % 4 == 0 && L % grid == 0);
  const long long Tp = (L / grid) * u_sz;
  OCTMAE_CHECK_ARG(pred_batch_stride >= (long long)L * PD && pred_batch_stride % 4 == 0);
  OCTMAE_CHECK_ARG(frame_idx != nullptr || Tp <= T);            // identity frame map: every predicted frame must exist
  // 16-byte loads of pred and of the volume's rows, 4-byte stores
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(pred) & 15u) == 0 && (reinterpret_cast<uintptr_t>(imgs) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 3u) == 0);
  if (denorm != 0 && denorm != 1) return -2;
  if ((long long)B * L > 0x7fffffffLL || PD > 0x7fffffffLL || Tp > 0x7fffffffLL) return -2;   // token and element indices are ints
  long long blocks = ((long long)B * L + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (denorm)
    hipLaunchKernelGGL(compose_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, pred, pred_batch_stride, imgs, frame_idx, mask, out,
                       B, T, H, W, u_sz, p, L, (int)Tp);
  else
    hipLaunchKernelGGL(compose_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, pred, pred_batch_stride, imgs, frame_idx, mask, out,
                       B, T, H, W, u_sz, p, L, (int)Tp);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
