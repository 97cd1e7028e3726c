// Slab LayerNorm: the patch embedding of the SLIViT head on top of the spatio-temporal trunk (reference
// OCTCube/models_vit_st_flash_attn_slivit.py:245-257 -> models_slivit_head.py:37-38 -> vit-pytorch's to_patch_embedding[1]).
//
// For volume n and temporal slice t the reference takes the L = h w tokens of the slice, x[n][n_prefix + t L ..][0..C), transposes them
// to [C][L], flattens and applies LayerNorm(C L).  Row r = n T + t of that patch matrix is therefore the CONTIGUOUS slab
// S_r = x[n][n_prefix + t L .. n_prefix + (t + 1) L)[0..C) read transposed: element k = c L + l of the row is S_r[l][c].  The statistics do
// not depend on the order and are taken over the contiguous slab; only the affine part and the 16-bit store need the transposed order.
//
// All kernels are HBM-bound and use 256 threads.
//   statistics   a row is cut into chunks of 16384 floats that one workgroup holds in registers (16 float4 per thread): the chunk mean,
//                then the sum of squared deviations from it (two passes over registers, never E[x^2] - E[x]^2); a one-thread-per-row
//                kernel combines the chunk pairs (n_c, mean_c, M2_c) in ascending order in double (Chan et al.).
//   transposing  64 (l) x 64 (c) tiles through LDS, rows padded by one word: the slab is read along c in float4 (256-byte runs), the
//                16-bit row is written along l, 8 elements = 16 bytes per thread (128-byte runs) when L % 8 == 0, element by element
//                otherwise.  LDS banks: the fill puts 4 rows x 16 float4 of a wave at (row + column) mod 64, all different; the
//                transposed read of lane (c' = lane / 8, l' = lane % 8) touches word (8 l' + i) * 65 + c', bank 8 l' + c' + i: all different.
//   backward     row sums of g and g xhat per (row, tile) into the workspace, folded per row in ascending tile order in double; the dx
//                kernel recomputes xhat in the transposed order, puts dS back into the tile in place and stores it along c.  The
//                dgamma / dbeta sums over rows are kept per thread (the thread owns its k) over the rows r = g, g + G, ... a workgroup
//                walks, written as G partial rows to the workspace and folded in ascending order by a last launch: no float atomics,
//                every sum has a fixed order, two runs are bit-equal.
//   bytes/element: forward 4 + 4 (x twice; the second read follows the first closely) + 2 (A) + 8 (gamma, beta, per row of the batch);
//                  backward 2 x (2 + 4) read + 4 (gamma) x 2 + 4 (dx) written.
#include "rowwave.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int SN_TL = 64, SN_TC = 64;       // tile: l rows x c columns
constexpr int SN_LD = SN_TC + 1;            // words per LDS row
constexpr int SN_CHUNK = 16384;             // floats per statistics chunk = 256 threads x 16 float4
constexpr int SN_BLOCKS = 512;              // the dx kernel's grid is filled up to about this many workgroups by splitting the rows

struct SlabGeom {
  int C, L, T, n_prefix, K;                 // K = C L
  int tiles_l, tiles_c;
};

__device__ __forceinline__ size_t slab_offset(const SlabGeom& g, int r) {
  const int n = r / g.T, t = r - n * g.T;
  return ((size_t)n * ((size_t)g.n_prefix + (size_t)g.T * g.L) + (size_t)g.n_prefix + (size_t)t * g.L) * (size_t)g.C;
}

// the sum over the 256 threads of a workgroup, the same in every thread; red: 4 words of LDS
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- statistics ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slab_stats_kernel(const float* __restrict__ x, float* __restrict__ part, SlabGeom g, int nchunks) {
  __shared__ float red[4];
  const int r = blockIdx.x / nchunks, ch = blockIdx.x - r * nchunks;
  const float* s = x + slab_offset(g, r) + (size_t)ch * SN_CHUNK;
  const int n = min(SN_CHUNK, g.K - ch * SN_CHUNK);          // a multiple of 8
  f32x4 v[16];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = 4 * ((int)threadIdx.x + 256 * i);
    if (e < n) {
      v[i] = *reinterpret_cast<const f32x4*>(s + e);
      sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
  }
  const float mu = block_sum256(sum, red) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = 4 * ((int)threadIdx.x + 256 * i);
    if (e < n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mu;
        q = fmaf(d, d, q);
      }
    }
  }
  const float m2 = block_sum256(q, red);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = mu;
    part[2 * (size_t)blockIdx.x + 1] = m2;
  }
}

__global__ __launch_bounds__(256) void slab_stats_fold_kernel(const float* __restrict__ part, float* __restrict__ mean,
                                                              float* __restrict__ rstd, int rows, int K, int nchunks, float eps) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* p = part + 2 * (size_t)r * nchunks;
  double m = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) m += (double)min(SN_CHUNK, K - ch * SN_CHUNK) * (double)p[2 * ch];
  m /= (double)K;
  double M2 = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) {
    const double d = (double)p[2 * ch] - m;
    M2 += (double)p[2 * ch + 1] + (double)min(SN_CHUNK, K - ch * SN_CHUNK) * d * d;
  }
  mean[r] = (float)m;
  rstd[r] = (float)(1.0 / sqrt(M2 / (double)K + (double)eps));
}

// ---- tiles -----------------------------------------------------------------------------------------
// tile[l'][c'] = S[l0 + l'][c0 + c'], zero outside the slab
__device__ __forceinline__ void slab_load_tile(const float* __restrict__ s, int l0, int c0, const SlabGeom& g, float* tile) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = (int)threadIdx.x + 256 * i;
    const int ll = idx >> 4, cj = (idx & 15) * 4;
    const int l = l0 + ll, c = c0 + cj;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (l < g.L && c < g.C) v = *reinterpret_cast<const f32x4*>(s + (size_t)l * g.C + c);      // C % 8 == 0: c + 3 < C
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[ll * SN_LD + cj + e] = v[e];
  }
}

__device__ __forceinline__ void slab_store_tile(float* __restrict__ s, int l0, int c0, const SlabGeom& g, const float* tile) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = (int)threadIdx.x + 256 * i;
    const int ll = idx >> 4, cj = (idx & 15) * 4;
    const int l = l0 + ll, c = c0 + cj;
    if (l < g.L && c < g.C) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = tile[ll * SN_LD + cj + e];
      *reinterpret_cast<f32x4*>(s + (size_t)l * g.C + c) = v;
    }
  }
}

// eight consecutive elements of a row in the transposed order (k .. k + 7, the same c); nv of them lie inside the row
template <bool VEC>
__device__ __forceinline__ void load8_f32(const float* __restrict__ p, int nv, float* o) {
  if (VEC) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = i < nv ? p[i] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void load8_lp(const bf16_t* __restrict__ p, int nv, float* o) {
  if (VEC) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[2 * i] = bflo(w[i]); o[2 * i + 1] = bfhi(w[i]); }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = i < nv ? bf2f(p[i]) : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void store8_f32(float* __restrict__ p, int nv, const float* o) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{o[4], o[5], o[6], o[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nv) p[i] = o[i];
  }
}

// The piece of the transposed tile a thread owns in pass `it` (0, 1): column cc of the tile, rows lb .. lb + 7
#define SLAB_PIECE(it)                                        \
  const int cc = (it) * 32 + ((int)threadIdx.x >> 3);         \
  const int lb = 8 * ((int)threadIdx.x & 7);                  \
  const int c = c0 + cc, l = l0 + lb;                         \
  const bool live = c < g.C && l < g.L;                       \
  const int nv = min(8, g.L - l);                             \
  const int k = c * g.L + l

// ---- forward ---------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void slab_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, bf16_t* __restrict__ A, SlabGeom g) {
  __shared__ float tile[SN_TL * SN_LD];
  const int tiles = g.tiles_l * g.tiles_c;
  const int r = blockIdx.x / tiles, tt = blockIdx.x - r * tiles;
  const int l0 = (tt % g.tiles_l) * SN_TL, c0 = (tt / g.tiles_l) * SN_TC;
  slab_load_tile(x + slab_offset(g, r), l0, c0, g, tile);
  __syncthreads();
  const float mu = mean[r], rs = rstd[r];
  bf16_t* Ar = A + (size_t)r * g.K;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    SLAB_PIECE(it);
    if (live) {
      float gm[8], bt[8], o[8];
      load8_f32<VEC>(gamma + k, nv, gm);
      load8_f32<VEC>(beta + k, nv, bt);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = LN_AFFINE(tile[(lb + i) * SN_LD + cc], mu, rs, gm[i], bt[i]);
      if (VEC) {
        const u32x4 w = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7])};
        *reinterpret_cast<u32x4*>(Ar + k) = w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < nv) Ar[k + i] = f2bf(o[i]);
      }
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------
// part[(r tiles + tile)][2] = the tile's sums of g and of g xhat, g = dA gamma
template <bool VEC>
__global__ __launch_bounds__(256) void slab_bwd_sums_kernel(const bf16_t* __restrict__ dA, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, float* __restrict__ part, SlabGeom g) {
  __shared__ float tile[SN_TL * SN_LD];
  __shared__ float red[4];
  const int tiles = g.tiles_l * g.tiles_c;
  const int r = blockIdx.x / tiles, tt = blockIdx.x - r * tiles;
  const int l0 = (tt % g.tiles_l) * SN_TL, c0 = (tt / g.tiles_l) * SN_TC;
  slab_load_tile(x + slab_offset(g, r), l0, c0, g, tile);
  __syncthreads();
  const float mu = mean[r], rs = rstd[r];
  const bf16_t* dr = dA + (size_t)r * g.K;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    SLAB_PIECE(it);
    if (live) {
      float gm[8], d[8];
      load8_f32<VEC>(gamma + k, nv, gm);
      load8_lp<VEC>(dr + k, nv, d);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xh = (tile[(lb + i) * SN_LD + cc] - mu) * rs;
        const float gy = d[i] * gm[i];
        s1 += gy;
        s2 = fmaf(gy, xh, s2);
      }
    }
  }
  const float S1 = block_sum256(s1, red);
  const float S2 = block_sum256(s2, red);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = S1;
    part[2 * (size_t)blockIdx.x + 1] = S2;
  }
}

// m12[r][2] = mean_k(g), mean_k(g xhat): the tile sums of a row added in ascending tile order
__global__ __launch_bounds__(256) void slab_bwd_fold_kernel(const float* __restrict__ part, float* __restrict__ m12, int rows, int tiles,
                                                            int K) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* p = part + 2 * (size_t)r * tiles;
  double a = 0.0, b = 0.0;
  for (int t = 0; t < tiles; ++t) {
    a += (double)p[2 * t];
    b += (double)p[2 * t + 1];
  }
  m12[2 * r] = (float)(a / (double)K);
  m12[2 * r + 1] = (float)(b / (double)K);
}

// dS = rstd (g - mean(g) - xhat mean(g xhat)) for the rows rg, rg + G, ... of one tile; pg / pb [G][K]: this workgroup's sums over
// those rows of dA xhat and dA (NULL: not wanted)
template <bool VEC>
__global__ __launch_bounds__(256) void slab_bwd_dx_kernel(const bf16_t* __restrict__ dA, const float* __restrict__ x,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ m12,
                                                          float* __restrict__ dx, float* __restrict__ pg, float* __restrict__ pb,
                                                          SlabGeom g, int rows, int G) {
  __shared__ float tile[SN_TL * SN_LD];
  const int tiles = g.tiles_l * g.tiles_c;
  const int rg = blockIdx.x / tiles, tt = blockIdx.x - rg * tiles;
  const int l0 = (tt % g.tiles_l) * SN_TL, c0 = (tt / g.tiles_l) * SN_TC;
  float gm[2][8], ag[2][8], ab[2][8];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    SLAB_PIECE(it);
#pragma unroll
    for (int i = 0; i < 8; ++i) { gm[it][i] = 0.f; ag[it][i] = 0.f; ab[it][i] = 0.f; }
    if (live) load8_f32<VEC>(gamma + k, nv, gm[it]);
  }
  for (int r = rg; r < rows; r += G) {
    const size_t off = slab_offset(g, r);
    slab_load_tile(x + off, l0, c0, g, tile);
    __syncthreads();
    const float mu = mean[r], rs = rstd[r], m1 = m12[2 * r], m2 = m12[2 * r + 1];
    const bf16_t* dr = dA + (size_t)r * g.K;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      SLAB_PIECE(it);
      if (live) {
        float d[8];
        load8_lp<VEC>(dr + k, nv, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float* w = tile + (lb + i) * SN_LD + cc;           // read and rewritten by this thread alone
          const float xh = (*w - mu) * rs;
          const float gy = d[i] * gm[it][i];
          ag[it][i] = fmaf(d[i], xh, ag[it][i]);
          ab[it][i] += d[i];
          *w = LN_DX(rs, gy, m1, xh, m2);
        }
      }
    }
    __syncthreads();
    slab_store_tile(dx + off, l0, c0, g, tile);
    __syncthreads();
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    SLAB_PIECE(it);
    if (live) {
      if (pg != nullptr) store8_f32<VEC>(pg + (size_t)rg * g.K + k, nv, ag[it]);
      if (pb != nullptr) store8_f32<VEC>(pb + (size_t)rg * g.K + k, nv, ab[it]);
    }
  }
}

// dgamma[k] += sum_g pg[g][k], dbeta[k] += sum_g pb[g][k], g ascending
__global__ __launch_bounds__(256) void slab_bwd_params_kernel(const float* __restrict__ pg, const float* __restrict__ pb,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int K, int G) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  if (dgamma != nullptr) {
    float t = 0.f;
    for (int j = 0; j < G; ++j) t += pg[(size_t)j * K + k];
    dgamma[k] += t;
  }
  if (dbeta != nullptr) {
    float t = 0.f;
    for (int j = 0; j < G; ++j) t += pb[(size_t)j * K + k];
    dbeta[k] += t;
  }
}

// the n_prefix leading token rows of every volume of dx
__global__ __launch_bounds__(256) void slab_zero_prefix_kernel(float* __restrict__ dx, int N, int per4, size_t vol_floats) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N * per4) return;
  const size_t n = i / per4, j = i - n * per4;
  reinterpret_cast<f32x4*>(dx + n * vol_floats)[j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- host ------------------------------------------------------------------------------------------
struct SlabPlan {
  SlabGeom g;
  int rows, nchunks, tiles, G;
  long long fwd_floats, sums_floats, bwd_floats;      // sums_floats: offset of the dgamma / dbeta partials inside the workspace
};

static bool slab_plan(int N, int T, int L, int C, int n_prefix, SlabPlan* p) {
  if (N < 1 || T < 1 || L < 1 || C < 8 || C % 8 != 0 || n_prefix < 0) return false;
  const long long K = (long long)C * L, rows = (long long)N * T, lim = 1ll << 30;
  if (K > lim || rows > (1ll << 24) || (long long)n_prefix * C > lim) return false;
  const long long tl = (L + SN_TL - 1) / SN_TL, tc = (C + SN_TC - 1) / SN_TC, tiles = tl * tc, nchunks = (K + SN_CHUNK - 1) / SN_CHUNK;
  if (tiles > (1 << 20) || rows * tiles > lim || rows * nchunks > lim) return false;
  p->g = SlabGeom{C, L, T, n_prefix, (int)K, (int)tl, (int)tc};
  p->rows = (int)rows;
  p->nchunks = (int)nchunks;
  p->tiles = (int)tiles;
  long long G = (SN_BLOCKS + tiles - 1) / tiles;
  if (G > rows) G = rows;
  p->G = (int)G;
  p->fwd_floats = 2 * rows * nchunks;
  p->sums_floats = (2 * rows * tiles + 2 * rows + 3) / 4 * 4;
  p->bwd_floats = p->sums_floats + 2 * G * K;
  return (p->fwd_floats > p->bwd_floats ? p->fwd_floats : p->bwd_floats) <= 0x7fffffffll;
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_slabnorm_ws_floats(int N, int T, int L, int C) {
  SlabPlan p;
  if (!slab_plan(N, T, L, C, 0, &p)) return -1;
  return (int)(p.fwd_floats > p.bwd_floats ? p.fwd_floats : p.bwd_floats);
}

extern "C" int octmae_slab_norm_fwd(const float* x, const float* gamma, const float* beta, void* a_lp, float* mean, float* rstd, float* ws,
                                    int N, int T, int L, int C, int n_prefix, float eps, void* stream) {
  SlabPlan p;
  OCTMAE_CHECK_ARG(x && gamma && beta && a_lp && mean && rstd && ws);
  OCTMAE_CHECK_ARG(slab_plan(N, T, L, C, n_prefix, &p) && eps >= 0.f);
  OCTMAE_CHECK_ARG(al16(x) && al16(gamma) && al16(beta) && al16(a_lp) && al16(ws));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bf16_t* A = reinterpret_cast<bf16_t*>(a_lp);
  hipLaunchKernelGGL(slab_stats_kernel, dim3(p.rows * p.nchunks), dim3(256), 0, st, x, ws, p.g, p.nchunks);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_stats_fold_kernel, dim3((p.rows + 255) / 256), dim3(256), 0, st, ws, mean, rstd, p.rows, p.g.K, p.nchunks, eps);
  OCTMAE_LAUNCH_CHECK();
  const dim3 grid(p.rows * p.tiles), blk(256);
  if (L % 8 == 0)
    hipLaunchKernelGGL(slab_apply_kernel<true>, grid, blk, 0, st, x, mean, rstd, gamma, beta, A, p.g);
  else
    hipLaunchKernelGGL(slab_apply_kernel<false>, grid, blk, 0, st, x, mean, rstd, gamma, beta, A, p.g);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_slab_norm_bwd(const void* da_lp, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                                    float* dgamma, float* dbeta, float* ws, int N, int T, int L, int C, int n_prefix, void* stream) {
  SlabPlan p;
  OCTMAE_CHECK_ARG(da_lp && x && mean && rstd && gamma && dx && ws);
  OCTMAE_CHECK_ARG(slab_plan(N, T, L, C, n_prefix, &p));
  OCTMAE_CHECK_ARG(al16(da_lp) && al16(x) && al16(gamma) && al16(dx) && al16(ws));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t* dA = reinterpret_cast<const bf16_t*>(da_lp);
  float* part = ws;
  float* m12 = ws + 2 * (size_t)p.rows * p.tiles;
  float* pg = dgamma != nullptr ? ws + p.sums_floats : nullptr;
  float* pb = dbeta != nullptr ? ws + p.sums_floats + (size_t)p.G * p.g.K : nullptr;
  const bool vec = L % 8 == 0;
  const dim3 blk(256);
  if (n_prefix > 0) {
    const int per4 = n_prefix * C / 4;
    const size_t total = (size_t)N * per4;
    hipLaunchKernelGGL(slab_zero_prefix_kernel, dim3((unsigned)((total + 255) / 256)), blk, 0, st, dx, N, per4,
                       ((size_t)n_prefix + (size_t)T * L) * (size_t)C);
    OCTMAE_LAUNCH_CHECK();
  }
  if (vec)
    hipLaunchKernelGGL(slab_bwd_sums_kernel<true>, dim3(p.rows * p.tiles), blk, 0, st, dA, x, mean, rstd, gamma, part, p.g);
  else
    hipLaunchKernelGGL(slab_bwd_sums_kernel<false>, dim3(p.rows * p.tiles), blk, 0, st, dA, x, mean, rstd, gamma, part, p.g);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_bwd_fold_kernel, dim3((p.rows + 255) / 256), blk, 0, st, part, m12, p.rows, p.tiles, p.g.K);
  OCTMAE_LAUNCH_CHECK();
  if (vec)
    hipLaunchKernelGGL(slab_bwd_dx_kernel<true>, dim3(p.G * p.tiles), blk, 0, st, dA, x, mean, rstd, gamma, m12, dx, pg, pb, p.g, p.rows, p.G);
  else
    hipLaunchKernelGGL(slab_bwd_dx_kernel<false>, dim3(p.G * p.tiles), blk, 0, st, dA, x, mean, rstd, gamma, m12, dx, pg, pb, p.g, p.rows, p.G);
  OCTMAE_LAUNCH_CHECK();
  if (pg != nullptr || pb != nullptr) {
    hipLaunchKernelGGL(slab_bwd_params_kernel, dim3((p.g.K + 255) / 256), blk, 0, st, pg, pb, dgamma, dbeta, p.g.K, p.G);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
