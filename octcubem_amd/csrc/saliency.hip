// Saliency side of the fine-tuned models: the gradient of a class score with respect to the input volume, Grad-CAM's reduction over the
// token stream, and the heat volume a viewer overlays (retinal-COEM/src/oph_vis_util/base_cam_retclip_3mod.py is the reference's
// Grad-CAM base class; pytorch_grad_cam does its reductions as ATen / numpy chains).
//   octmae_patch_scatter  dpatch 16-bit [B*nkeep][C*tp*p*p]  ->  dimgs f32 [B][C][T][H][W]      the adjoint of octmae_patch_gather
//   octmae_cam_weights    G f32 [B][n_prefix+L][C]           ->  w f32 [B][C] = mean over the L patch rows
//   octmae_cam_tokens     A f32 [B][n_prefix+L][C], w        ->  cam f32 [B][L] = max(0, w . A row)
//   octmae_heatmap        m f32 [B][t][h][w]                 ->  uint8 [B][F][H][W], per-sample min-max, linear (t) x bilinear (h, w)
//   octmae_cam_eigen      A f32 [B][n_prefix+L][C], w        ->  cam f32 [B][L] = Mc v1 by power iterations (eigen_smooth), residual [B]
//   octmae_cam_accumulate cam f32 [B][n]                     ->  acc (+)= weight * min-max-normalised cam, rows mirrored or not (aug_smooth)
// Everything is deterministic: no floating-point atomic anywhere; sums are folded in a fixed order.
// Only octmae_patch_scatter touches the 16-bit operand type (it widens it); the others are the same code in the two builds.
//
// patch_scatter walks as patch_gather_kernel (csrc/tokens.hip) does: one thread per 8-pixel chunk of a patch row, one 16-byte load of
// the 16-bit gradient, two f32x4 stores to one image row.  At p = 16 a lane writes 32 bytes and its neighbour the adjacent 32 bytes of
// the same row; the next patch row is W floats away.  That these 32-byte pieces are combined in L2 before they leave it is an
// ASSUMPTION: no write counter has been collected for this kernel (csrc/recon.hip makes the same assumption for its 16-byte pieces).
// If the stores turn out to be the limit, one wave per row of gw tokens (whole image rows per store) is next.
// With ids and nkeep < L the image gradient is zero-filled by a pass of its own first (the dropped tokens are not enumerable from
// ids_keep alone); the scatter then overwrites the kept patches on the same stream.  Without ids the walk covers all L tokens and
// writes the zeros itself; with nkeep == L every voxel is written by the scatter and nothing is filled.
// CONTRACT: the ids of one sample are distinct (the masking kernel produces a permutation prefix).  There is no device check; a
// repeated id would make two threads store to the same voxels and the later one win.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

__global__ __launch_bounds__(256) void fill_zero_kernel(float* __restrict__ dst, size_t n4) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
    *reinterpret_cast<f32x4*>(dst + 4 * i) = z;
}

// rows = tokens walked per sample: nkeep with ids (or when nkeep == L), L without ids (rows i >= nkeep write zeros)
template <typename IdxT>
__global__ __launch_bounds__(256) void patch_scatter_kernel(const bf16_t* __restrict__ dpatch, const IdxT* __restrict__ ids,
                                                            float* __restrict__ dimgs, int B, int C, int T, int H, int W, int tp, int p,
                                                            int nkeep, int rows, int L) {
  const int gh = H / p, gw = W / p;
  const int pc = p >> 3;                   // 8-px chunks per patch row
  const int kdim = C * tp * p * p;
  const int chunks_per_tok = kdim >> 3;
  const size_t total = (size_t)B * rows * chunks_per_tok;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
    const int ch = (int)(q % chunks_per_tok);
    const size_t row = q / chunks_per_tok;
    const int b = (int)(row / rows), i = (int)(row % rows);
    const int id = ids ? min(max((int)ids[(size_t)b * nkeep + i], 0), L - 1) : i;    // an id from device memory never leaves the volume
    const int t = id / (gh * gw), hy = (id / gw) % gh, wx = id % gw;
    const int px8 = ch % pc;
    int rest = ch / pc;
    const int py = rest % p; rest /= p;
    const int u = rest % tp;
    const int c = rest / tp;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
    if (i < nkeep) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(dpatch + ((size_t)b * nkeep + i) * kdim + (size_t)ch * 8);
      a[0] = bflo(w[0]); a[1] = bfhi(w[0]); a[2] = bflo(w[1]); a[3] = bfhi(w[1]);
      d[0] = bflo(w[2]); d[1] = bfhi(w[2]); d[2] = bflo(w[3]); d[3] = bfhi(w[3]);
    }
    float* dst = dimgs + ((((size_t)b * C + c) * T + (t * tp + u)) * H + (hy * p + py)) * W + wx * p + px8 * 8;
    *reinterpret_cast<f32x4*>(dst) = a;
    *reinterpret_cast<f32x4*>(dst + 4) = d;
  }
}

// ---------------------------------------------------------------------------------------------
// Grad-CAM channel weights, stage 1: part[b][s][c] = sum over the rows of split s of G[b][n_prefix + l][c].
// Block = 64 column lanes of 4 columns (one 1 KiB line of a row per wave) x 4 row lanes; a row lane adds its rows in ascending order,
// the four row lanes are folded 0, 1, 2, 3.
__global__ __launch_bounds__(256) void cam_weights_part_kernel(const float* __restrict__ G, float* __restrict__ part, int L, int n_prefix,
                                                               int C, int rows_per_split) {
  __shared__ f32x4 red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 64 + cl) * 4;
  const int s = blockIdx.y, b = blockIdx.z, S = gridDim.y;
  const int r0 = s * rows_per_split;
  const int r1 = min(r0 + rows_per_split, L);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c0 < C) {
    const float* base = G + ((size_t)b * (n_prefix + L) + n_prefix) * C + c0;
    for (int r = r0 + rl; r < r1; r += 4) acc += *reinterpret_cast<const f32x4*>(base + (size_t)r * C);
  }
  red[rl][cl] = acc;
  __syncthreads();
  if (rl == 0 && c0 < C) {
    const f32x4 v = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    *reinterpret_cast<f32x4*>(part + ((size_t)b * S + s) * C + c0) = v;
  }
}

// stage 2: w[b][c] = (part[b][0][c] + part[b][1][c] + ...) / L, splits in ascending order
__global__ __launch_bounds__(256) void cam_weights_fold_kernel(const float* __restrict__ part, float* __restrict__ w, int B, int S, int C,
                                                               int L) {
  const int c4 = C >> 2;
  const size_t total = (size_t)B * c4;
  const float fl = (float)L;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
    const int b = (int)(q / c4), c0 = (int)(q % c4) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) acc += *reinterpret_cast<const f32x4*>(part + ((size_t)b * S + s) * C + c0);
    f32x4 o = {acc[0] / fl, acc[1] / fl, acc[2] / fl, acc[3] / fl};
    *reinterpret_cast<f32x4*>(w + (size_t)b * C + c0) = o;
  }
}

// cam[b][l] = max(0, sum_c w[b][c] * A[b][n_prefix + l][c]); one wave per token row
__global__ __launch_bounds__(256) void cam_tokens_kernel(const float* __restrict__ A, const float* __restrict__ w, float* __restrict__ cam,
                                                         int B, int L, int n_prefix, int C) {
  const int lane = threadIdx.x & 63;
  const size_t nwaves = (size_t)gridDim.x * 4;
  const size_t rows = (size_t)B * L;
  const int c4 = C >> 2;
  for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const int b = (int)(row / L), l = (int)(row % L);
    const float* a = A + ((size_t)b * (n_prefix + L) + n_prefix + l) * C;
    const float* wb = w + (size_t)b * C;
    float s = 0.f;
    for (int q = lane; q < c4; q += 64) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + 4 * q);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wb + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) s = fmaf(wv[k], av[k], s);
    }
    s = wave_sum(s);
    if (lane == 0) cam[row] = fmaxf(s, 0.f);
  }
}

// ---------------------------------------------------------------------------------------------
// Heat volume.  Stage 1: mnmx[b] = {min, max} of the coarse map of sample b (one workgroup per sample; min / max do not depend on order).
__global__ __launch_bounds__(256) void heat_minmax_kernel(const float* __restrict__ m, float* __restrict__ mnmx, int n) {
  __shared__ float smn[4], smx[4];
  const float* src = m + (size_t)blockIdx.x * n;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = src[i];
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mn = -wave_max(-mn); mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mnmx[2 * blockIdx.x] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    mnmx[2 * blockIdx.x + 1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

// F.interpolate's align_corners=False source position: src = (dst + 0.5) * in / out - 0.5, negative -> 0; lower neighbour, clamped
// upper neighbour and the weight of the upper one.  in == out gives src = dst exactly (weight 0): the identity.
__device__ __forceinline__ void src_pos(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// Stage 2: one thread per 4 output voxels of a row, one 4-byte store.  The coarse map is normalised as it is read (8 corner values per
// voxel, all cache hits: the map is (F H W) / (t h w) times smaller than the output), interpolated along t, then bilinearly.
__global__ __launch_bounds__(256) void heatmap_kernel(const float* __restrict__ m, const float* __restrict__ mnmx, uint8_t* __restrict__ out,
                                                      int B, int t, int h, int w, int F, int H, int W) {
  const int w4 = W >> 2;
  const size_t total = (size_t)B * F * H * w4;
  const float st = (float)t / (float)F, sh = (float)h / (float)H, sw = (float)w / (float)W;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
    const int x4 = (int)(q % w4);
    size_t rest = q / w4;
    const int y = (int)(rest % H); rest /= H;
    const int f = (int)(rest % F);
    const int b = (int)(rest / F);
    const float mn = mnmx[2 * b], mx = mnmx[2 * b + 1];
    const float den = 1e-7f + (mx - mn);
    int t0, t1, y0, y1;
    float lt, ly;
    src_pos(f, st, t, t0, t1, lt);
    src_pos(y, sh, h, y0, y1, ly);
    const float* mb = m + (size_t)b * t * h * w;
    const float* r00 = mb + ((size_t)t0 * h + y0) * w;
    const float* r01 = mb + ((size_t)t0 * h + y1) * w;
    const float* r10 = mb + ((size_t)t1 * h + y0) * w;
    const float* r11 = mb + ((size_t)t1 * h + y1) * w;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int x0, x1;
      float lx;
      src_pos(4 * x4 + k, sw, w, x0, x1, lx);
      // along t first, on the four (y, x) corners
      const float a00 = (1.f - lt) * ((r00[x0] - mn) / den) + lt * ((r10[x0] - mn) / den);
      const float a01 = (1.f - lt) * ((r00[x1] - mn) / den) + lt * ((r10[x1] - mn) / den);
      const float a10 = (1.f - lt) * ((r01[x0] - mn) / den) + lt * ((r11[x0] - mn) / den);
      const float a11 = (1.f - lt) * ((r01[x1] - mn) / den) + lt * ((r11[x1] - mn) / den);
      const float v = (1.f - ly) * ((1.f - lx) * a00 + lx * a01) + ly * ((1.f - lx) * a10 + lx * a11);
      const float g = fminf(fmaxf(floorf(255.f * v), 0.f), 255.f);      // a NaN (inf in the map) becomes 0
      word |= (unsigned)g << (8 * k);
    }
    *reinterpret_cast<unsigned*>(out + (((size_t)b * F + f) * H + y) * W + 4 * x4) = word;
  }
}

// ---------------------------------------------------------------------------------------------
// Eigen-smoothed CAM: power iterations on Mc^T Mc, Mc = M - mean_l M, M[l][c] = w[c] A[l][c], without M or Mc (octmae.h has the
// algebra).  Three launches per iteration: the token rows (one wave per row, as cam_tokens_kernel), the row splits of the transposed
// product (as cam_weights_part_kernel), and one workgroup per sample that folds the splits and normalises.
// sum of `x` over the 256 threads of a workgroup, the same value in every thread: lanes by wave_sum, the four waves 0, 1, 2, 3
__device__ __forceinline__ float block_sum(float x, float* sm) {
  x = wave_sum(x);
  __syncthreads();                                   // sm may still be read from the sum before this one
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__global__ __launch_bounds__(256) void eig_init_kernel(float* __restrict__ v, float* __restrict__ flag, int B, size_t n, float v0) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    v[i] = v0;
    if (i < (size_t)B) flag[i] = 0.f;
  }
}

// u[b][l] = sum_c q[c] A[b][n_prefix + l][c] - sum_c q[c] abar[b][c], q = v o w (v == nullptr: q = w, the centred plain CAM).  The two
// sums run over the same columns in the same order with the same operation, so a row equal to abar gives exactly 0.
__global__ __launch_bounds__(256) void eig_rows_kernel(const float* __restrict__ A, const float* __restrict__ w, const float* __restrict__ v,
                                                       const float* __restrict__ abar, float* __restrict__ u, int B, int L, int n_prefix,
                                                       int C) {
  const int lane = threadIdx.x & 63;
  const size_t nwaves = (size_t)gridDim.x * 4;
  const size_t rows = (size_t)B * L;
  const int c4 = C >> 2;
  for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const int b = (int)(row / L), l = (int)(row % L);
    const float* a = A + ((size_t)b * (n_prefix + L) + n_prefix + l) * C;
    const float* wb = w + (size_t)b * C;
    const float* mb = abar + (size_t)b * C;
    float s = 0.f, m = 0.f;
    for (int q = lane; q < c4; q += 64) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + 4 * q);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(mb + 4 * q);
      f32x4 qv = *reinterpret_cast<const f32x4*>(wb + 4 * q);
      if (v) qv *= *reinterpret_cast<const f32x4*>(v + (size_t)b * C + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s = fmaf(qv[k], av[k], s);
        m = fmaf(qv[k], bv[k], m);
      }
    }
    s = wave_sum(s);
    m = wave_sum(m);
    if (lane == 0) u[row] = s - m;
  }
}

// part[b][s][c] = sum over the rows of split s of u[b][l] A[b][n_prefix + l][c], partu[b][s] = the sum of u over the same rows; the
// block, the row lanes and their fold are cam_weights_part_kernel's
__global__ __launch_bounds__(256) void eig_tpart_kernel(const float* __restrict__ A, const float* __restrict__ u, float* __restrict__ part,
                                                        float* __restrict__ partu, int L, int n_prefix, int C, int rows_per_split) {
  __shared__ f32x4 red[4][64];
  __shared__ float redu[4];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 64 + cl) * 4;
  const int s = blockIdx.y, b = blockIdx.z, S = gridDim.y;
  const int r0 = s * rows_per_split;
  const int r1 = min(r0 + rows_per_split, L);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float us = 0.f;
  if (c0 < C) {
    const float* base = A + ((size_t)b * (n_prefix + L) + n_prefix) * C + c0;
    const float* ub = u + (size_t)b * L;
    for (int r = r0 + rl; r < r1; r += 4) {
      const float ur = ub[r];
      const f32x4 av = *reinterpret_cast<const f32x4*>(base + (size_t)r * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = fmaf(ur, av[k], acc[k]);
      us += ur;
    }
  }
  red[rl][cl] = acc;
  if (cl == 0) redu[rl] = us;                        // column lane 0 of the first block of columns always has c0 = 0 < C
  __syncthreads();
  if (rl == 0 && c0 < C) {
    const f32x4 v = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    *reinterpret_cast<f32x4*>(part + ((size_t)b * S + s) * C + c0) = v;
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) partu[(size_t)b * S + s] = ((redu[0] + redu[1]) + redu[2]) + redu[3];
}

// t[b][c] = w[c] (sum_s part[b][s][c] - abar[c] sum_s partu[b][s]) for the columns of this thread, splits in ascending order; returns
// the thread's share of sum_c t^2.  One workgroup per sample.
__device__ __forceinline__ float eig_fold(const float* __restrict__ part, const float* __restrict__ partu, const float* __restrict__ w,
                                          const float* __restrict__ abar, float* __restrict__ t, int b, int S, int C) {
  float su = 0.f;
  for (int s = 0; s < S; ++s) su += partu[(size_t)b * S + s];
  float ss = 0.f;
  for (int q = threadIdx.x; q < (C >> 2); q += 256) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) acc += *reinterpret_cast<const f32x4*>(part + ((size_t)b * S + s) * C + 4 * q);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)b * C + 4 * q);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(abar + (size_t)b * C + 4 * q);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = wv[k] * (acc[k] - bv[k] * su);
      ss = fmaf(o[k], o[k], ss);
    }
    *reinterpret_cast<f32x4*>(t + (size_t)b * C + 4 * q) = o;
  }
  return ss;
}

// v = t / ||t||; a zero norm leaves v as it is, a norm that is not finite raises the sample's flag (and leaves v as well)
__global__ __launch_bounds__(256) void eig_fold_norm_kernel(const float* __restrict__ part, const float* __restrict__ partu,
                                                            const float* __restrict__ w, const float* __restrict__ abar,
                                                            float* __restrict__ t, float* __restrict__ v, float* __restrict__ flag, int S,
                                                            int C) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  const float nrm = sqrtf(block_sum(eig_fold(part, partu, w, abar, t, b, S, C), sm));
  if (!(nrm <= 3.4028234664e38f)) {                  // inf or NaN
    if (threadIdx.x == 0) flag[b] = 1.f;
    return;
  }
  if (nrm > 0.f)
    for (int q = threadIdx.x; q < (C >> 2); q += 256) {    // the quads this thread wrote itself
      const f32x4 tv = *reinterpret_cast<const f32x4*>(t + (size_t)b * C + 4 * q);
      const f32x4 o = {tv[0] / nrm, tv[1] / nrm, tv[2] / nrm, tv[3] / nrm};
      *reinterpret_cast<f32x4*>(v + (size_t)b * C + 4 * q) = o;
    }
}

// after the last iteration: u = Mc v, t = Mc^T u (folded here), c1 = Mc 1 -> the residual, the sign and the map of sample blockIdx.x
__global__ __launch_bounds__(256) void eig_final_kernel(const float* __restrict__ part, const float* __restrict__ partu,
                                                        const float* __restrict__ w, const float* __restrict__ abar, float* __restrict__ t,
                                                        const float* __restrict__ v, const float* __restrict__ flag,
                                                        const float* __restrict__ u, const float* __restrict__ c1, float* __restrict__ cam,
                                                        float* __restrict__ residual, int S, int L, int C, int relu) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  eig_fold(part, partu, w, abar, t, b, S, C);
  const float* ub = u + (size_t)b * L;
  const float* cb = c1 + (size_t)b * L;
  float lam = 0.f, dot = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) {
    const float x = ub[l];
    lam = fmaf(x, x, lam);
    dot = fmaf(x, cb[l], dot);
  }
  lam = block_sum(lam, sm);
  dot = block_sum(dot, sm);
  float rr = 0.f;
  for (int q = threadIdx.x; q < (C >> 2); q += 256) {
    const f32x4 tv = *reinterpret_cast<const f32x4*>(t + (size_t)b * C + 4 * q);
    const f32x4 vv = *reinterpret_cast<const f32x4*>(v + (size_t)b * C + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = tv[k] - lam * vv[k];
      rr = fmaf(d, d, rr);
    }
  }
  rr = block_sum(rr, sm);
  float res = lam == 0.f ? 0.f : sqrtf(rr) / lam;
  if (flag[b] != 0.f || !(lam <= 3.4028234664e38f) || !(res <= 3.4028234664e38f)) res = NAN;
  if (threadIdx.x == 0) residual[b] = res;
  const float sign = dot < 0.f ? -1.f : 1.f;
  for (int l = threadIdx.x; l < L; l += 256) {
    const float p = sign * ub[l];
    cam[(size_t)b * L + l] = relu ? fmaxf(p, 0.f) : p;
  }
}

// acc[b][j] (first ? = : +=) weight * (cam[b][j'] - mn_b) / (1e-7f + (mx_b - mn_b)), j' = j mirrored within its row of `width` when flip
__global__ __launch_bounds__(256) void cam_accum_kernel(float* __restrict__ acc, const float* __restrict__ cam,
                                                        const float* __restrict__ mnmx, size_t total, int n, int width, int flip,
                                                        float weight, int first) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / n;
    const int j = (int)(i % n);
    const int x = j % width;
    const int src = flip ? j - x + (width - 1 - x) : j;
    const float mn = mnmx[2 * b], mx = mnmx[2 * b + 1];
    const float val = weight * ((cam[b * n + src] - mn) / (1e-7f + (mx - mn)));
    acc[i] = first ? val : acc[i] + val;
  }
}

static inline int blocks_for(size_t work_items, int per_block, int cap) {
  size_t g = (work_items + per_block - 1) / per_block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// rows per split of the weight reduction: at least 64 rows, at most 64 splits -- a function of L alone
static inline int cam_rows_per_split(int L) {
  int rps = (L + 63) / 64;
  if (rps < 64) rps = 64;
  return rps;
}
static inline int cam_splits(int L) { const int rps = cam_rows_per_split(L); return (L + rps - 1) / rps; }

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_patch_scatter(const void* dpatch_lp, const void* ids, int ids_is_i64, float* dimgs, int B, int C, int T, int H, int W,
                                    int tp, int p, int nkeep, void* stream) {
  OCTMAE_CHECK_ARG(dpatch_lp && dimgs && B > 0 && C > 0 && nkeep > 0);
  OCTMAE_CHECK_ARG(T > 0 && H > 0 && W > 0 && tp > 0 && p > 0);
  OCTMAE_CHECK_ARG(p % 8 == 0 && H % p == 0 && W % p == 0 && T % tp == 0 && W % 4 == 0);
  const int L = (T / tp) * (H / p) * (W / p);
  OCTMAE_CHECK_ARG(nkeep <= L);
  OCTMAE_CHECK_ARG(aligned16(dpatch_lp) && aligned16(dimgs));
  const long long kdim = (long long)C * tp * p * p;
  if (kdim > 0x7fffffffLL || (long long)B * L > 0x7fffffffLL) return -2;      // token rows and patch elements are ints
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t* src = reinterpret_cast<const bf16_t*>(dpatch_lp);
  const int rows = ids ? nkeep : L;
  if (ids && nkeep < L) {
    const size_t n4 = (size_t)B * C * T * H * W / 4;                          // W % 4 == 0
    hipLaunchKernelGGL(fill_zero_kernel, dim3(blocks_for(n4, 256, 8192)), dim3(256), 0, st, dimgs, n4);
    OCTMAE_LAUNCH_CHECK();
  }
  const size_t total = (size_t)B * rows * (size_t)(kdim / 8);
  if (ids && ids_is_i64)
    hipLaunchKernelGGL(patch_scatter_kernel<long long>, dim3(blocks_for(total, 256, 8192)), dim3(256), 0, st, src,
                       reinterpret_cast<const long long*>(ids), dimgs, B, C, T, H, W, tp, p, nkeep, rows, L);
  else
    hipLaunchKernelGGL(patch_scatter_kernel<int>, dim3(blocks_for(total, 256, 8192)), dim3(256), 0, st, src,
                       reinterpret_cast<const int*>(ids), dimgs, B, C, T, H, W, tp, p, nkeep, rows, L);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_cam_ws_floats(int B, int L, int C) {
  if (B <= 0 || L <= 0 || C <= 0) return -1;
  const long long n = (long long)B * cam_splits(L) * C;
  return n > 0x7fffffffLL ? -2 : (int)n;
}

extern "C" int octmae_cam_weights(const float* G, float* w, float* ws, int B, int L, int n_prefix, int C, void* stream) {
  OCTMAE_CHECK_ARG(G && w && ws && B > 0 && L > 0 && n_prefix >= 0 && C > 0 && C % 4 == 0);
  OCTMAE_CHECK_ARG(aligned16(G) && aligned16(w) && aligned16(ws));
  if (B > 65535 || (long long)n_prefix + L > 0x7fffffffLL) return -2;
  const int rps = cam_rows_per_split(L), S = cam_splits(L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cam_weights_part_kernel, dim3((C + 255) / 256, S, B), dim3(256), 0, st, G, ws, L, n_prefix, C, rps);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(cam_weights_fold_kernel, dim3(blocks_for((size_t)B * (C / 4), 256, 4096)), dim3(256), 0, st, ws, w, B, S, C, L);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_cam_tokens(const float* A, const float* w, float* cam, int B, int L, int n_prefix, int C, void* stream) {
  OCTMAE_CHECK_ARG(A && w && cam && B > 0 && L > 0 && n_prefix >= 0 && C > 0 && C % 4 == 0);
  OCTMAE_CHECK_ARG(aligned16(A) && aligned16(w));
  if ((long long)n_prefix + L > 0x7fffffffLL) return -2;
  hipLaunchKernelGGL(cam_tokens_kernel, dim3(blocks_for((size_t)B * L, 4, 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), A, w,
                     cam, B, L, n_prefix, C);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

static inline long long pad4(long long n) { return (n + 3) & ~3LL; }

// workspace of octmae_cam_eigen, in floats: part [B][S][C], partu [B][S], abar / v / t [B][C], u / c1 [B][L], flag [B]; every piece
// starts on a multiple of 4 floats
extern "C" int octmae_cam_eigen_ws_floats(int B, int L, int C) {
  if (B <= 0 || L <= 0 || C <= 0) return -1;
  const long long S = cam_splits(L);
  const long long n = pad4((long long)B * S * C) + pad4((long long)B * S) + 3 * pad4((long long)B * C) + 2 * pad4((long long)B * L) + pad4(B);
  return n > 0x7fffffffLL ? -2 : (int)n;
}

extern "C" int octmae_cam_eigen(const float* A, const float* w, float* cam, float* residual, float* ws, int B, int L, int n_prefix, int C,
                                int iters, int relu, void* stream) {
  OCTMAE_CHECK_ARG(A && w && cam && residual && ws && B > 0 && L > 0 && n_prefix >= 0 && C > 0 && C % 4 == 0 && iters > 0);
  OCTMAE_CHECK_ARG(aligned16(A) && aligned16(w) && aligned16(ws));
  if (B > 65535 || (long long)n_prefix + L > 0x7fffffffLL || octmae_cam_eigen_ws_floats(B, L, C) < 0) return -2;
  const int rps = cam_rows_per_split(L), S = cam_splits(L);
  float* part = ws;
  float* partu = part + pad4((long long)B * S * C);
  float* abar = partu + pad4((long long)B * S);
  float* v = abar + pad4((long long)B * C);
  float* t = v + pad4((long long)B * C);
  float* u = t + pad4((long long)B * C);
  float* c1 = u + pad4((long long)B * L);
  float* flag = c1 + pad4((long long)B * L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 gpart((C + 255) / 256, S, B);
  const int grows = blocks_for((size_t)B * L, 4, 8192);
  // abar = the mean of A over its patch rows: the channel-weight reduction, on A
  hipLaunchKernelGGL(cam_weights_part_kernel, gpart, dim3(256), 0, st, A, part, L, n_prefix, C, rps);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(cam_weights_fold_kernel, dim3(blocks_for((size_t)B * (C / 4), 256, 4096)), dim3(256), 0, st, part, abar, B, S, C, L);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(eig_init_kernel, dim3(blocks_for((size_t)B * C, 256, 4096)), dim3(256), 0, st, v, flag, B, (size_t)B * C,
                     1.f / sqrtf((float)C));
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(eig_rows_kernel, dim3(grows), dim3(256), 0, st, A, w, (const float*)nullptr, abar, c1, B, L, n_prefix, C);
  OCTMAE_LAUNCH_CHECK();
  for (int it = 0; it <= iters; ++it) {               // the pass after the last iteration leaves u = Mc v and the splits of Mc^T u
    hipLaunchKernelGGL(eig_rows_kernel, dim3(grows), dim3(256), 0, st, A, w, (const float*)v, abar, u, B, L, n_prefix, C);
    OCTMAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(eig_tpart_kernel, gpart, dim3(256), 0, st, A, u, part, partu, L, n_prefix, C, rps);
    OCTMAE_LAUNCH_CHECK();
    if (it < iters) {
      hipLaunchKernelGGL(eig_fold_norm_kernel, dim3(B), dim3(256), 0, st, part, partu, w, abar, t, v, flag, S, C);
      OCTMAE_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(eig_final_kernel, dim3(B), dim3(256), 0, st, part, partu, w, abar, t, v, flag, u, c1, cam, residual, S, L, C, relu);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_cam_accumulate(float* acc, const float* cam, float* mnmx, int B, int n, int width, int flip, float weight, int first,
                                     void* stream) {
  OCTMAE_CHECK_ARG(acc && cam && mnmx && B > 0 && n > 0 && width > 0 && n % width == 0);
  if (n > 0x7fffffff - 256) return -2;                                        // heat_minmax_kernel's index strides by 256
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(heat_minmax_kernel, dim3(B), dim3(256), 0, st, cam, mnmx, n);
  OCTMAE_LAUNCH_CHECK();
  const size_t total = (size_t)B * n;
  hipLaunchKernelGGL(cam_accum_kernel, dim3(blocks_for(total, 256, 4096)), dim3(256), 0, st, acc, cam, mnmx, total, n, width, flip, weight,
                     first);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_heatmap(const float* m, float* mnmx, uint8_t* out, int B, int t, int h, int w, int F, int H, int W, void* stream) {
  OCTMAE_CHECK_ARG(m && mnmx && out);
  OCTMAE_CHECK_ARG(B > 0 && t > 0 && h > 0 && w > 0 && F > 0 && H > 0 && W > 0);
  OCTMAE_CHECK_ARG(W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0);
  if ((long long)t * h * w > 0x7fffffffLL) return -2;                         // the coarse map of a sample is indexed by an int
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(heat_minmax_kernel, dim3(B), dim3(256), 0, st, m, mnmx, t * h * w);
  OCTMAE_LAUNCH_CHECK();
  const size_t total = (size_t)B * F * H * (W / 4);
  hipLaunchKernelGGL(heatmap_kernel, dim3(blocks_for(total, 256, 16384)), dim3(256), 0, st, m, mnmx, out, B, t, h, w, F, H, W);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
