// LayerNorm forward / backward over the fp32 residual stream (reference K5: nn.LayerNorm eps=1e-6,
// Pre-training/models_mae_joint_res_flash_attn.py:799; applied at video_vit.py:181-184, :489, :592).
//
// HBM-bound: one wave owns one token row, lane t holds float4 chunks t, t+64, ... (16-byte coalesced
// loads), statistics by wave64 butterfly shuffles, bf16 output packed 8 bytes per chunk.
//   fwd bytes/element: 4 (x) read + 2 (y) write
//   bwd bytes/element: 2 (dy) + 4 (x) read, 4 (dx) [+2 (dx bf16)] write; dgamma/dbeta/column sums are
//   accumulated per lane across the rows a wave walks, reduced over the block in LDS, written as per-block
//   partials to a caller-provided workspace and folded by a second small kernel (deterministic, no atomics).
#include <cstdlib>
#ifdef LN_PLAIN_LOADS      // A/B builds: ordinary loads of the row operands, in this file only
#define ROW_PLAIN_LOADS
#endif
#include "rowwave.hpp"
#include "../../include/octmae.h"

namespace octmae {

template <int NC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int M, int D,
                                                     float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  const float invD = 1.0f / (float)D;
  f32x4 g[NC], b[NC];
  ROW_CHUNKS(c, ci) {
    g[c] = *reinterpret_cast<const f32x4*>(gamma + 4 * ci);
    b[c] = *reinterpret_cast<const f32x4*>(beta + 4 * ci);
  }
  // the next row of the wave is requested before the current one is reduced (as in the backward kernel)
  f32x4 vn[NC];
  auto issue = [&](int row) {
    const float* xr = x + (size_t)row * D;
    ROW_CHUNKS(c, ci) vn[c] = ROW_LD(f32x4, xr + 4 * ci);
  };
  if (wave < M) issue(wave);
  for (int row = wave; row < M; row += nwaves) {
    f32x4 v[NC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = vn[c];
    if (row + nwaves < M) issue(row + nwaves);
    ROW_CHUNKS(c, ci) s += ROW_SUM4(v[c]);
    const float mu = wave_sum(s) * invD;
    float q = 0.f;
    ROW_CHUNKS(c, ci) ROW_SQDEV4(q, v[c], mu);
    const float var = wave_sum(q) * invD;
    const float rs = rsqrtf(var + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    bf16_t* yr = y + (size_t)row * D;
    ROW_CHUNKS(c, ci) LN_AFFINE_STORE(v[c], mu, rs, g[c], b[c], yr + 4 * ci);
  }
}

// y = the LayerNorm output rebuilt from the SAVED row statistics (activation recomputation: ops.BlockFn at level "light" drops y1 / y2
// and calls this in its backward) through the LN_AFFINE_STORE that ln_fwd_kernel uses: that kernel's y bit for bit.  Without the two reductions
// a row costs one pass: 4 (x) read + 2 (y) write bytes per element, the row pipelined the same way.
template <int NC>
__global__ __launch_bounds__(256) void ln_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, bf16_t* __restrict__ y, int M, int D) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  f32x4 g[NC], b[NC];
  ROW_CHUNKS(c, ci) {
    g[c] = *reinterpret_cast<const f32x4*>(gamma + 4 * ci);
    b[c] = *reinterpret_cast<const f32x4*>(beta + 4 * ci);
  }
  f32x4 vn[NC];
  float mu_n = 0.f, rs_n = 0.f;
  auto issue = [&](int row) {
    mu_n = mean[row];
    rs_n = rstd[row];
    const float* xr = x + (size_t)row * D;
    ROW_CHUNKS(c, ci) vn[c] = ROW_LD(f32x4, xr + 4 * ci);
  };
  if (wave < M) issue(wave);
  for (int row = wave; row < M; row += nwaves) {
    const float mu = mu_n, rs = rs_n;
    f32x4 v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = vn[c];
    if (row + nwaves < M) issue(row + nwaves);
    bf16_t* yr = y + (size_t)row * D;
    ROW_CHUNKS(c, ci) LN_AFFINE_STORE(v[c], mu, rs, g[c], b[c], yr + 4 * ci);
  }
}

// dx = [dres +] rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy * gamma
template <int NC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ dres,
                                                     float* __restrict__ dx, bf16_t* __restrict__ dxb,
                                                     float* __restrict__ partial, bool want_dxsum, int M, int D) {
  __shared__ RowRed red[3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wave = blockIdx.x * 4 + w;
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  const float invD = 1.0f / (float)D;
  f32x4 g[NC], ag[NC], ab[NC], as[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {      // written out: the accumulators of every slot are zeroed, inside the row or not
    const int ci = lane + 64 * c;
    if (ci < nchunk) g[c] = *reinterpret_cast<const f32x4*>(gamma + 4 * ci);
#pragma unroll
    for (int e = 0; e < 4; ++e) { ag[c][e] = 0.f; ab[c][e] = 0.f; as[c][e] = 0.f; }
  }
  // Software-pipelined over rows: the loads of the NEXT row are issued before the current row is reduced, so every
  // wave keeps two rows (12-20 KB) in flight -- with one row per wave the kernel sat at ~35 % of HBM bandwidth.
  // The incoming residual-stream gradient is part of the prefetch: vmcnt retires in order, so a load issued after the
  // next row's requests and needed now would drain them all and leave one row in flight.
  f32x4 xn[NC], rn[NC];
  u32x2 dn[NC];
  float mu_n = 0.f, rs_n = 0.f;
  auto issue = [&](int row) {
    mu_n = mean[row];
    rs_n = rstd[row];
    ROW_CHUNKS(c, ci) {
      xn[c] = ROW_LD(f32x4, x + (size_t)row * D + 4 * ci);
      dn[c] = ROW_LD(u32x2, dy + (size_t)row * D + 4 * ci);
      if (dres != nullptr) rn[c] = ROW_LD(f32x4, dres + (size_t)row * D + 4 * ci);
    }
  };
  if (wave < M) issue(wave);
  for (int row = wave; row < M; row += nwaves) {
    const float mu = mu_n, rs = rs_n;
    f32x4 xh[NC], rv[NC];
    u32x2 dw[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { xh[c] = xn[c]; dw[c] = dn[c]; rv[c] = rn[c]; }
    if (row + nwaves < M) issue(row + nwaves);
    float s1 = 0.f, s2 = 0.f;
    ROW_CHUNKS(c, ci) {
      const float d[4] = {bflo(dw[c][0]), bfhi(dw[c][0]), bflo(dw[c][1]), bfhi(dw[c][1])};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xhat = (xh[c][e] - mu) * rs;
        const float gy = d[e] * g[c][e];
        xh[c][e] = xhat;
        s1 += gy;
        s2 = fmaf(gy, xhat, s2);
        ag[c][e] = fmaf(d[e], xhat, ag[c][e]);
        ab[c][e] += d[e];
      }
    }
    const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD;
    ROW_CHUNKS(c, ci) {
      const float d[4] = {bflo(dw[c][0]), bfhi(dw[c][0]), bflo(dw[c][1]), bfhi(dw[c][1])};
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = LN_DX(rs, d[e] * g[c][e], m1, xh[c][e], m2);
      if (dres != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += rv[c][e];
      }
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(dx + (size_t)row * D + 4 * ci));
      if (dxb != nullptr) {
        u32x2 wv = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
        __builtin_nontemporal_store(wv, reinterpret_cast<u32x2*>(dxb + (size_t)row * D + 4 * ci));
      }
      if (want_dxsum) {
#pragma unroll
        for (int e = 0; e < 4; ++e) as[c][e] += o[e];
      }
    }
  }
  // block reduction of the per-lane column partials, one chunk slot at a time; each block writes its [3][D] partial
  // sums to the workspace (a second tiny kernel folds them): 1024 workgroups adding atomically into the same 3 x D
  // words ran at the contended-atomic rate and took 3/4 of this kernel's time.
#pragma unroll
  for (int c = 0; c < NC; ++c) {      // written out: every slot takes part in the barriers of ROW_FOLD4
    const int ci = lane + 64 * c;
    ROW_FOLD4(3, ci, partial + ((size_t)blockIdx.x * 3 + w) * D + 4 * ci, ag[c][e], ab[c][e], as[c][e]);
  }
}

// out_k[c] += sum_b partial[b][k][c] for k = 0 (dgamma), 1 (dbeta), 2 (dxsum); 64 columns x 16 block-groups per workgroup,
// fixed summation order (the result does not depend on scheduling)
__global__ __launch_bounds__(1024) void ln_bwd_finish_kernel(const float* __restrict__ partial, int nblocks, int D,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             float* __restrict__ dxsum) {
  __shared__ float red[16][64];
  const int k = blockIdx.y;
  float* dst = (k == 0) ? dgamma : (k == 1) ? dbeta : dxsum;
  if (dst == nullptr) return;
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < D) {
    const float* src = partial + (size_t)k * D + c;
    const size_t stride = (size_t)3 * D;
    int b = grp;
    for (; b + 48 < nblocks; b += 64) {
      s0 += src[(size_t)b * stride];
      s1 += src[(size_t)(b + 16) * stride];
      s2 += src[(size_t)(b + 32) * stride];
      s3 += src[(size_t)(b + 48) * stride];
    }
    for (; b < nblocks; b += 16) s0 += src[(size_t)b * stride];
  }
  red[grp][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (grp == 0 && c < D) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g][cl];
    dst[c] += t;
  }
}

// Grid: whole multiples of the 256 CUs, and FEW of them -- two workgroups per CU forward (8 waves per CU, two rows in flight each), one
// backward.  With every wave slot filled (2048 / 512 blocks: rounds 1-3) the same kernels read 5.0-5.5 TB/s; with 512 / 256 blocks
// 5.75-5.99 (round 4, in the step: ln_bwd d512 1034 -> 887 us, d1024 486 -> 455; ln_fwd d512 405 -> 350, d1024 185 -> 173; step
// +0.55 %): a wave streams one contiguous row at a time, and fewer concurrent row streams keep more DRAM pages open.  Grids that
// are not multiples of 256 (768, 384, 192) lose to imbalance; one block per CU forward starves the D = 512 rows (3.96 TB/s).
// OCTMAE_LN_FWD_GRID / OCTMAE_LN_BWD_GRID override the caps for A/B runs (profiles/r04_layernorm_grid.txt).
static inline int ln_grid(int M, bool bwd = false) {
  static const int capf = getenv("OCTMAE_LN_FWD_GRID") ? atoi(getenv("OCTMAE_LN_FWD_GRID")) : 512;
  static const int capb = getenv("OCTMAE_LN_BWD_GRID") ? atoi(getenv("OCTMAE_LN_BWD_GRID")) : 256;
  const int cap = bwd ? capb : capf;
  int blocks = (M + 3) / 4;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return blocks;
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                    float* rstd, int M, int D, float eps, void* stream) {
  OCTMAE_CHECK_ARG(x && gamma && beta && y_bf16 && mean && rstd);
  OCTMAE_CHECK_ARG(row_shape_ok(M, D));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nc = row_nc(D);
  bf16_t* y = reinterpret_cast<bf16_t*>(y_bf16);
  dim3 grid(ln_grid(M)), blk(256);
  ROW_DISPATCH(ln_fwd_kernel, grid, blk, x, gamma, beta, y, mean, rstd, M, D, eps);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_ln_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                               void* y_bf16, int M, int D, void* stream) {
  OCTMAE_CHECK_ARG(x && mean && rstd && gamma && beta && y_bf16);
  OCTMAE_CHECK_ARG(row_shape_ok(M, D));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nc = row_nc(D);
  bf16_t* y = reinterpret_cast<bf16_t*>(y_bf16);
  dim3 grid(ln_grid(M)), blk(256);
  ROW_DISPATCH(ln_apply_kernel, grid, blk, x, mean, rstd, gamma, beta, y, M, D);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_layernorm_bwd_ws_floats(int M, int D) {
  int blocks = ln_grid(M, true);
  if (blocks > 512) blocks = 512;
  return blocks * 3 * D;
}

extern "C" int octmae_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                    const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgamma,
                                    float* dbeta, float* dxsum, float* partial_ws, int M, int D, void* stream) {
  OCTMAE_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && dx && partial_ws);
  OCTMAE_CHECK_ARG(row_shape_ok(M, D));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nc = row_nc(D);
  const bf16_t* dy = reinterpret_cast<const bf16_t*>(dy_bf16);
  bf16_t* dxb = reinterpret_cast<bf16_t*>(dx_bf16);
  int blocks = ln_grid(M, true);
  if (blocks > 512) blocks = 512;
  dim3 grid(blocks), blk(256);
  const bool ws = dxsum != nullptr;
  ROW_DISPATCH(ln_bwd_kernel, grid, blk, dy, x, mean, rstd, gamma, dres, dx, dxb, partial_ws, ws, M, D);
  OCTMAE_LAUNCH_CHECK();
  if (dgamma != nullptr || dbeta != nullptr || dxsum != nullptr) {
    hipLaunchKernelGGL(ln_bwd_finish_kernel, dim3((D + 63) / 64, 3), dim3(1024), 0, st, partial_ws, blocks, D, dgamma, dbeta, dxsum);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
