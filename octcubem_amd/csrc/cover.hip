// Full-coverage reconstruction of the 3-D MAE: K forwards over complementary masks (models_mae.cover_noise) predict every token at least
// once while it is hidden; the masked predictions are summed per token and one finishing pass turns the sums into a reconstruction
// volume, a squared-error volume and per-token scores.  The project's own: the reference has no counterpart.
//   octmae_cover_accumulate  pred f32 [B][L][PD] (any batch stride) + mask f32 [B][L]  ->  sum f32 [B][L][PD] (+=), cnt int32 [B][L] (+= 1)
//   octmae_cover_finish      sum, cnt + imgs f32 [B][1][T][H][W]  ->  recon uint8 [B][Tp][H][W], err f32 [B][Tp][H][W], score f32 [B][L]
// The walk is compose_kernel's (csrc/recon.hip): one wave per token, float4 groups along (u, py, px), which are contiguous in pred / sum
// and four adjacent pixels of one image row; a capped grid whose waves make several trips.  No 16-bit operand: the two builds of the
// library hold the same code.  No atomics; a token's outputs depend on that token's inputs alone.
//   bytes per element and pass, accumulate: first 4 read (masked rows only) + 4 written; later 8 read + 4 written on the masked rows,
//   nothing on the others.  finish per voxel: 4 (sum) + 4 (frame) read, 1 + 4 written; denorm reads the target patch twice more (cached).
// Every formula here is stated operation by operation (tests/cover_ref.py restates it in torch): the file is compiled with
// -ffp-contract=off (Makefile), so v * s + m of the grey level, d * d + the running score and the like stay separate roundings; the
// two fused multiply-adds of the denorm statistics are explicit fmaf calls, the same arithmetic as compose_kernel<true>.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

__device__ __forceinline__ bool cv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// untransform_image, as grey() of csrc/recon.hip: (int) clip((v * s + m) * 255, 0, 255), three roundings; a non-finite v gives 0
__device__ __forceinline__ unsigned cv_grey(float v) {
  const float s = (float)(76.03 / 255), m = (float)(45.79 / 255);
  float t = __fmul_rn(__fadd_rn(__fmul_rn(v, s), m), 255.0f);
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return cv_finite(v) ? (unsigned)(int)t : 0u;
}

__device__ __forceinline__ int cv_src_frame(const int* __restrict__ frame_idx, int fo, int T) {
  return frame_idx ? min(max(frame_idx[fo], 0), T - 1) : fo;
}

// FIRST: every row of sum and every cnt is written (no zero fill in front).  Otherwise only the masked rows are read and written.
template <bool FIRST>
__global__ __launch_bounds__(256) void cover_accum_kernel(const float* __restrict__ pred, long long pred_bs, const float* __restrict__ mask,
                                                          float* __restrict__ sum, int* __restrict__ cnt, int B, int L, int PD) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int nq = PD >> 2;
  const int rows = B * L;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / L, l = row - b * L;
    const bool removed = mask[row] != 0.0f;      // wave-uniform
    if (!FIRST && !removed) continue;
    const float* pr = pred + (size_t)b * (size_t)pred_bs + (size_t)l * PD;
    float* sr = sum + (size_t)row * PD;
    if (FIRST) {
      for (int q = lane; q < nq; q += 64) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (removed) v = *reinterpret_cast<const f32x4*>(pr + 4 * q);
        *reinterpret_cast<f32x4*>(sr + 4 * q) = v;
      }
      if (lane == 0) cnt[row] = removed ? 1 : 0;
    } else {
      for (int q = lane; q < nq; q += 64) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(sr + 4 * q);
        const f32x4 v = *reinterpret_cast<const f32x4*>(pr + 4 * q);
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __fadd_rn(a[k], v[k]);
        *reinterpret_cast<f32x4*>(sr + 4 * q) = r;
      }
      if (lane == 0) cnt[row] += 1;
    }
  }
}

template <bool DENORM>
__global__ __launch_bounds__(256) void cover_finish_kernel(const float* __restrict__ sum, const int* __restrict__ cnt,
                                                           const float* __restrict__ imgs, const int* __restrict__ frame_idx,
                                                           uint8_t* __restrict__ recon, float* __restrict__ err, float* __restrict__ score,
                                                           int B, int T, int H, int W, int u_sz, int p, int L, int Tp) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int gh = H / p, gw = W / p;
  const int PD = u_sz * p * p;
  const int nq = PD >> 2;
  const int rows = B * L;
  const size_t vol_out = (size_t)Tp * H * W;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / L, l = row - b * L;
    const int c = cnt[row];                      // wave-uniform
    const bool pred_ok = c > 0;
    const float fc = (float)c;
    const int t = l / (gh * gw), hy = (l / gw) % gh, wx = l % gw;
    const float* sr = sum + (size_t)row * PD;
    const float* vol = imgs + (size_t)b * T * H * W;
    // per-patch statistics of the target, exactly compose_kernel<true>'s: fp32, two passes, unbiased variance + 1e-6
    float mu = 0.f, sd = 1.f;
    if (DENORM && pred_ok) {
      float s = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int px = e % p, py = (e / p) % p, u = e / (p * p);
        const int f = cv_src_frame(frame_idx, t * u_sz + u, T);
        const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
        s += (iv[0] + iv[1]) + (iv[2] + iv[3]);
      }
      mu = wave_sum(s) / (float)PD;
      float s2 = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int px = e % p, py = (e / p) % p, u = e / (p * p);
        const int f = cv_src_frame(frame_idx, t * u_sz + u, T);
        const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
#pragma unroll
        for (int k = 0; k < 4; ++k) s2 = fmaf(iv[k] - mu, iv[k] - mu, s2);
      }
      sd = sqrtf(wave_sum(s2) / (float)(PD - 1) + 1.0e-6f);
    }
    float part = 0.f;
    for (int q = lane; q < nq; q += 64) {
      const int e = 4 * q;
      const int px = e % p, py = (e / p) % p, u = e / (p * p);
      const int fo = t * u_sz + u;
      const int f = cv_src_frame(frame_idx, fo, T);
      const f32x4 iv = *reinterpret_cast<const f32x4*>(vol + ((size_t)f * H + hy * p + py) * W + wx * p + px);
      f32x4 sq = {0.f, 0.f, 0.f, 0.f};
      unsigned g[4];
      if (pred_ok) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(sr + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float v = __fdiv_rn(sv[k], fc);
          if (DENORM) v = __fmaf_rn(v, sd, mu);
          const float d = __fsub_rn(v, iv[k]);
          sq[k] = __fmul_rn(d, d);
          g[k] = cv_grey(v);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = cv_grey(iv[k]);
      }
      const size_t o = (size_t)b * vol_out + ((size_t)fo * H + hy * p + py) * W + wx * p + px;
      *reinterpret_cast<unsigned*>(recon + o) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
      if (err) *reinterpret_cast<f32x4*>(err + o) = sq;
      part = __fadd_rn(part, __fadd_rn(__fadd_rn(sq[0], sq[1]), __fadd_rn(sq[2], sq[3])));
    }
    if (score) {
      const float tot = wave_sum(part);
      if (lane == 0) score[row] = pred_ok ? __fdiv_rn(tot, (float)PD) : 0.0f;
    }
  }
}

static long long cover_blocks(long long rows) {
  long long blocks = (rows + 3) / 4;
  return blocks > 4096 ? 4096 : blocks;
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_cover_accumulate(const float* pred, long long pred_batch_stride, const float* mask, float* sum, int* cnt, int B, int L,
                                       int PD, int first, void* stream) {
  OCTMAE_CHECK_ARG(pred && mask && sum && cnt);
  OCTMAE_CHECK_ARG(B > 0 && L > 0 && PD > 0 && PD % 4 == 0);
  OCTMAE_CHECK_ARG(pred_batch_stride >= (long long)L * PD && pred_batch_stride % 4 == 0);
  // 16-byte loads and stores of pred and sum
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(pred) & 15u) == 0 && (reinterpret_cast<uintptr_t>(sum) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(mask) & 3u) == 0 && (reinterpret_cast<uintptr_t>(cnt) & 3u) == 0);
  OCTMAE_CHECK_ARG(static_cast<const void*>(pred) != static_cast<const void*>(sum));
  if ((long long)B * L > 0x7fffffffLL) return -2;   // token rows are ints
  const unsigned blocks = (unsigned)cover_blocks((long long)B * L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (first)
    hipLaunchKernelGGL(cover_accum_kernel<true>, dim3(blocks), dim3(256), 0, st, pred, pred_batch_stride, mask, sum, cnt, B, L, PD);
  else
    hipLaunchKernelGGL(cover_accum_kernel<false>, dim3(blocks), dim3(256), 0, st, pred, pred_batch_stride, mask, sum, cnt, B, L, PD);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_cover_finish(const float* sum, const int* cnt, const float* imgs, const int* frame_idx, uint8_t* recon, float* err,
                                   float* score, int B, int T, int H, int W, int u_sz, int p, int L, int denorm, void* stream) {
  OCTMAE_CHECK_ARG(sum && cnt && imgs && recon);
  OCTMAE_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && u_sz > 0 && p > 0 && L > 0);
  OCTMAE_CHECK_ARG(p % 4 == 0 && W % 4 == 0 && H % p == 0 && W % p == 0);
  const long long PD = (long long)u_sz * p * p, grid = (long long)(H / p) * (W / p);
  OCTMAE_CHECK_ARG(PD % 4 == 0 && L % grid == 0);
  const long long Tp = (L / grid) * u_sz;
  OCTMAE_CHECK_ARG(frame_idx != nullptr || Tp <= T);            // identity frame map: every predicted frame must exist
  // 16-byte loads of sum and of the volume's rows, 16-byte stores of err, 4-byte stores of recon
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(sum) & 15u) == 0 && (reinterpret_cast<uintptr_t>(imgs) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(err) & 15u) == 0 && (reinterpret_cast<uintptr_t>(recon) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(cnt) & 3u) == 0 && (reinterpret_cast<uintptr_t>(score) & 3u) == 0);
  if (denorm != 0 && denorm != 1) return -2;
  if ((long long)B * L > 0x7fffffffLL || PD > 0x7fffffffLL || Tp > 0x7fffffffLL) return -2;   // token and element indices are ints
  const unsigned blocks = (unsigned)cover_blocks((long long)B * L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (denorm)
    hipLaunchKernelGGL(cover_finish_kernel<true>, dim3(blocks), dim3(256), 0, st, sum, cnt, imgs, frame_idx, recon, err, score, B, T, H, W,
                       u_sz, p, L, (int)Tp);
  else
    hipLaunchKernelGGL(cover_finish_kernel<false>, dim3(blocks), dim3(256), 0, st, sum, cnt, imgs, frame_idx, recon, err, score, B, T, H, W,
                       u_sz, p, L, (int)Tp);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
