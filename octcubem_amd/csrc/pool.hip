// Slice-pooling head of the RETFound-all model (OCTCube/models_vit_3dhead_flash_attn.py:47-65 on models_vit_flash_attn.py:143-149):
// every B-scan of a volume runs through the 2-D ViT as its own image; its patch tokens are mean-pooled (or its cls token taken),
// LayerNorm'd by fc_norm, and the normalised rows are averaged over the S slices of the volume.
//
// All fp32.  Forward, mean mode: a column sum over the T-1 patch tokens of every slice, split over several workgroups per slice
// (one workgroup per slice would leave most CUs idle at B*S ~ 24); per-split partials go to a caller-provided workspace and are
// folded in split order by the per-slice statistics kernel (no atomics: two runs are bit-identical).
//   fwd bytes/element of x: 4 read (mean mode; cls mode reads one row per slice)
//   bwd bytes/element of dx: 4 written [+2 (bf16 copy)]; everything else is O(B*S*D)
#include <cstdlib>
#include "rowwave.hpp"
#include "../../include/octmae.h"

namespace octmae {

// Split of a slice's L = T-1 patch tokens over workgroups: ~2 workgroups per CU over all slices, >= 16 rows (4 per wave) each.
static inline int pool_nsplit(int BS, int T) {
  const int L = T - 1;
  if (L <= 0) return 1;
  int ns = (512 + BS - 1) / BS;
  const int max_ns = (L + 15) / 16;
  if (ns > max_ns) ns = max_ns;
  if (ns < 1) ns = 1;
  return ns;
}

// partial[s][k][:] = sum of x[s][t][:] over the tokens t of split k (t >= 1); grid (nsplit, BS), four waves per workgroup
template <int NC>
__global__ __launch_bounds__(256) void pool_colsum_kernel(const float* __restrict__ x, float* __restrict__ partial, int T, int D,
                                                          int rows_per_split) {
  __shared__ RowRed red[1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x, s = blockIdx.y, nsplit = gridDim.x;
  const int nchunk = D >> 2;
  const int t0 = 1 + k * rows_per_split;
  int t1 = t0 + rows_per_split;
  if (t1 > T) t1 = T;
  const float* xs = x + (size_t)s * T * D;
  f32x4 a0[NC], a1[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) { a0[c][e] = 0.f; a1[c][e] = 0.f; }
  // two rows per wave and iteration (separate accumulators, added in a fixed order at the end): 2 x NC float4 loads in flight
  int t = t0 + w;
  for (; t + 4 < t1; t += 8) {
    f32x4 v0[NC], v1[NC];
    ROW_CHUNKS(c, ci) {
      v0[c] = ROW_LD(f32x4, xs + (size_t)t * D + 4 * ci);
      v1[c] = ROW_LD(f32x4, xs + (size_t)(t + 4) * D + 4 * ci);
    }
    ROW_CHUNKS(c, ci) { a0[c] += v0[c]; a1[c] += v1[c]; }
  }
  if (t < t1) ROW_CHUNKS(c, ci) a0[c] += ROW_LD(f32x4, xs + (size_t)t * D + 4 * ci);
  float* dst = partial + ((size_t)s * nsplit + k) * D;
#pragma unroll
  for (int c = 0; c < NC; ++c) {      // written out: every slot takes part in the barriers of ROW_FOLD4
    const int ci = lane + 64 * c;
    ROW_FOLD4(1, ci, dst + 4 * ci, a0[c][e] + a1[c][e]);
  }
}

// One wave per slice: pooled row (split partials folded in order, / (T-1); or token 0), its LayerNorm statistics.
template <int NC>
__global__ __launch_bounds__(256) void pool_stats_kernel(const float* __restrict__ x, const float* __restrict__ partial, int nsplit,
                                                         float* __restrict__ pooled, float* __restrict__ mean, float* __restrict__ rstd,
                                                         int BS, int T, int D, int cls, float eps) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= BS) return;
  const int nchunk = D >> 2;
  const float invD = 1.0f / (float)D;
  f32x4 p[NC];
  float sum = 0.f;
  if (cls) {
    const float* xr = x + (size_t)s * T * D;
    ROW_CHUNKS(c, ci) p[c] = *reinterpret_cast<const f32x4*>(xr + 4 * ci);
  } else {
    const float invL = 1.0f / (float)(T - 1);
    const float* src = partial + (size_t)s * nsplit * D;
    ROW_CHUNKS(c, ci) {
      f32x4 a = *reinterpret_cast<const f32x4*>(src + 4 * ci);
      for (int k = 1; k < nsplit; ++k) a += *reinterpret_cast<const f32x4*>(src + (size_t)k * D + 4 * ci);
      p[c] = a * invL;
    }
  }
  ROW_CHUNKS(c, ci) sum += ROW_SUM4(p[c]);
  const float mu = wave_sum(sum) * invD;
  float q = 0.f;
  ROW_CHUNKS(c, ci) {
    ROW_SQDEV4(q, p[c], mu);
    *reinterpret_cast<f32x4*>(pooled + (size_t)s * D + 4 * ci) = p[c];
  }
  const float rs = rsqrtf(wave_sum(q) * invD + eps);
  if (lane == 0) {
    mean[s] = mu;
    rstd[s] = rs;
  }
}

// out[b][c] = (1/S) sum_s (xhat[b*S+s][c] * gamma[c] + beta[c]), slices in order; grid (ceil(D/256), B)
__global__ __launch_bounds__(256) void pool_slice_mean_kernel(const float* __restrict__ pooled, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ out, int S, int D) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= D) return;
  const float g = gamma[c], bt = beta[c];
  float acc = 0.f;
  for (int j = 0; j < S; ++j) {
    const int s = b * S + j;
    acc += LN_AFFINE(pooled[(size_t)s * D + c], mean[s], rstd[s], g, bt);
  }
  out[(size_t)b * D + c] = acc / (float)S;
}

// Backward, one wave per slice: dy = dout[b] / S, dp = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma.
// dps[s] = dp * scale (what every pooled token row of dx receives); part[s] = (dy xhat, dy, dp): the slice's dgamma / dbeta / column
// sum of dx, folded over the slices by pool_bwd_finish_kernel.
template <int NC>
__global__ __launch_bounds__(256) void pool_bwd_rows_kernel(const float* __restrict__ dout, const float* __restrict__ pooled,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, float* __restrict__ dps,
                                                            float* __restrict__ part, int BS, int S, int D, float scale) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= BS) return;
  const int b = s / S;
  const int nchunk = D >> 2;
  const float invD = 1.0f / (float)D, invS = 1.0f / (float)S;
  const float mu = mean[s], rs = rstd[s];
  f32x4 dy[NC], xh[NC], g[NC];
  float s1 = 0.f, s2 = 0.f;
  ROW_CHUNKS(c, ci) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + (size_t)b * D + 4 * ci);
    const f32x4 p = *reinterpret_cast<const f32x4*>(pooled + (size_t)s * D + 4 * ci);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * ci);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dy[c][e] = d[e] * invS;
      xh[c][e] = (p[e] - mu) * rs;
      g[c][e] = dy[c][e] * gm[e];
      s1 += g[c][e];
      s2 = fmaf(g[c][e], xh[c][e], s2);
    }
  }
  const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD;
  float* pr = part + (size_t)s * 3 * D;
  ROW_CHUNKS(c, ci) {
    f32x4 dp, dg, dsc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dp[e] = LN_DX(rs, g[c][e], m1, xh[c][e], m2);
      dg[e] = dy[c][e] * xh[c][e];
      dsc[e] = dp[e] * scale;
    }
    *reinterpret_cast<f32x4*>(dps + (size_t)s * D + 4 * ci) = dsc;
    *reinterpret_cast<f32x4*>(pr + 4 * ci) = dg;
    *reinterpret_cast<f32x4*>(pr + D + 4 * ci) = dy[c];
    *reinterpret_cast<f32x4*>(pr + 2 * D + 4 * ci) = dp;
  }
}

// dst_k[c] += sum_s part[s][k][c] for k = 0 (dgamma), 1 (dbeta), 2 (column sums of dx); 64 columns x 16 slice-groups per
// workgroup, fixed summation order (as ln_bwd_finish_kernel)
__global__ __launch_bounds__(1024) void pool_bwd_finish_kernel(const float* __restrict__ part, int BS, int D, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float* __restrict__ dxsum) {
  __shared__ float red[16][64];
  const int k = blockIdx.y;
  float* dst = (k == 0) ? dgamma : (k == 1) ? dbeta : dxsum;
  if (dst == nullptr) return;
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float a = 0.f;
  if (c < D)
    for (int s = grp; s < BS; s += 16) a += part[((size_t)s * 3 + k) * D + c];
  red[grp][cl] = a;
  __syncthreads();
  if (grp == 0 && c < D) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g][cl];
    dst[c] += t;
  }
}

// The dense dx [BS][T][D]: dps[s] on the pooled token rows (1..T-1, or 0 in cls mode), exact zeros elsewhere; the optional 16-bit
// copy is what the producing Block's backward would otherwise make in a pass of its own.  One wave per row, grid-stride.
template <int NC>
__global__ __launch_bounds__(256) void pool_dx_kernel(const float* __restrict__ dps, float* __restrict__ dx, bf16_t* __restrict__ dxb,
                                                      int M, int T, int D, int cls) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  for (int row = wave; row < M; row += nwaves) {
    const int s = row / T, t = row - s * T;
    const bool pooled_row = cls ? (t == 0) : (t != 0);
    ROW_CHUNKS(c, ci) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pooled_row) v = *reinterpret_cast<const f32x4*>(dps + (size_t)s * D + 4 * ci);
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dx + (size_t)row * D + 4 * ci));
      if (dxb != nullptr) {
        u32x2 wv = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        __builtin_nontemporal_store(wv, reinterpret_cast<u32x2*>(dxb + (size_t)row * D + 4 * ci));
      }
    }
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_slice_pool_ws_floats(int BS, int T, int D) {
  if (BS <= 0 || T <= 0 || D <= 0) return -1;
  const long long fwd = (long long)BS * pool_nsplit(BS, T) * D;
  const long long bwd = 4LL * BS * D;
  const long long n = fwd > bwd ? fwd : bwd;
  return n > 0x7fffffffLL ? -1 : (int)n;
}

extern "C" int octmae_slice_pool_fwd(const float* x, const float* gamma, const float* beta, float* out, float* pooled, float* mean,
                                     float* rstd, float* ws, int B, int S, int T, int D, int cls, float eps, void* stream) {
  OCTMAE_CHECK_ARG(x && gamma && beta && out && pooled && mean && rstd && ws);
  OCTMAE_CHECK_ARG(S > 0 && T > 0 && row_shape_ok(B, D) && (cls == 0 || cls == 1));
  OCTMAE_CHECK_ARG(cls == 1 || T >= 2);
  OCTMAE_CHECK_ARG((long long)B * S * T * D < (1LL << 40));
  // B * S is the grid's y of the column-sum launch, and the rows B * S * T are counted in int (docs/OFFSET_RANGES.md)
  OCTMAE_CHECK_ARG((long long)B * S <= 65535 && (long long)B * S * T <= 0x7FFFFFFFLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int BS = B * S;
  const int nc = row_nc(D);
  const int nsplit = cls ? 1 : pool_nsplit(BS, T);
  if (!cls) {
    const int rps = (T - 1 + nsplit - 1) / nsplit;
    ROW_DISPATCH(pool_colsum_kernel, dim3(nsplit, BS), dim3(256), x, ws, T, D, rps);
    OCTMAE_LAUNCH_CHECK();
  }
  ROW_DISPATCH(pool_stats_kernel, dim3((BS + 3) / 4), dim3(256), x, ws, nsplit, pooled, mean, rstd, BS, T, D, cls, eps);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_slice_mean_kernel, dim3((D + 255) / 256, B), dim3(256), 0, st, pooled, mean, rstd, gamma, beta, out, S, D);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_slice_pool_bwd(const float* dout, const float* pooled, const float* mean, const float* rstd, const float* gamma,
                                     float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* dxsum, float* ws, int B, int S,
                                     int T, int D, int cls, void* stream) {
  OCTMAE_CHECK_ARG(dout && pooled && mean && rstd && gamma && dx && ws);
  OCTMAE_CHECK_ARG(S > 0 && T > 0 && row_shape_ok(B, D) && (cls == 0 || cls == 1));
  OCTMAE_CHECK_ARG(cls == 1 || T >= 2);
  OCTMAE_CHECK_ARG((long long)B * S * T * D < (1LL << 40));
  // B * S is the grid's y of the column-sum launch, and the rows B * S * T are counted in int (docs/OFFSET_RANGES.md)
  OCTMAE_CHECK_ARG((long long)B * S <= 65535 && (long long)B * S * T <= 0x7FFFFFFFLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int BS = B * S;
  const int M = BS * T;
  const int nc = row_nc(D);
  float* dps = ws;                         // [BS][D]
  float* part = ws + (size_t)BS * D;       // [BS][3][D]
  const float scale = cls ? 1.0f : 1.0f / (float)(T - 1);
  ROW_DISPATCH(pool_bwd_rows_kernel, dim3((BS + 3) / 4), dim3(256), dout, pooled, mean, rstd, gamma, dps, part, BS, S, D, scale);
  OCTMAE_LAUNCH_CHECK();
  if (dgamma != nullptr || dbeta != nullptr || dxsum != nullptr) {
    hipLaunchKernelGGL(pool_bwd_finish_kernel, dim3((D + 63) / 64, 3), dim3(1024), 0, st, part, BS, D, dgamma, dbeta, dxsum);
    OCTMAE_LAUNCH_CHECK();
  }
  // a pure write stream: enough waves in flight to keep the write queues full (8 per CU), not one per row
  int blocks = (M + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  bf16_t* dxb = reinterpret_cast<bf16_t*>(dx_bf16);
  ROW_DISPATCH(pool_dx_kernel, dim3(blocks), dim3(256), dps, dx, dxb, M, T, D, cls);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
