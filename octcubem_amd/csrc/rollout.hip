// One step of attention rollout (Abnar & Zuidema 2020) as a vector chain: the start row of Ahat_L ... Ahat_1 needs, per block, only
//   r_out[j] = sum_i (r_in[i] / rho[i]) (F[i, j] + [i == j]),   F = fuse_h P^h,   rho[i] = 1 + sum_j F[i, j],
// a weighted column sum of a softmax matrix.  The attention kernels never store a probability, so P is recomputed here from the q, k
// the model's attention consumed, on the f32 tile of csrc/simtile.hpp (its fourth consumer), and nothing of size N N exists anywhere.
//   octmae_rollout_step   q, k f32, row b N + i, head h at columns h HD .. h HD + HD - 1 (row strides >= H HD);  r_in, r_out f32 [B][N]
// Arithmetic, every rounding as written (the Makefile compiles this file with -ffp-contract=off; no fast-math flag):
//   s^h(i, j) the tile's chain acc = 0; for kk = 0 .. HD-1: acc = fmaf(q[i][h HD + kk], k[j][h HD + kk], acc)  (SIM_SCORE_TILE with d = HD;
//             the same bits with the operands swapped: a product of two floats commutes)
//   z = scale * s                                   one f32 multiply
//   per (b, h, i): an online (M, S) over the 64-column tiles in ascending order, S = sum_j expf(z - M), rescaled by expf(M_old - M_new)
//             when the maximum rises (factor 1 without an exp when it does not); the four partials of a row (two half-waves, two waves)
//             merge in a fixed order;  lse = M + logf(S)
//   P = expf(z - lse)                               expf / logf are the device library's (1 ulp)
//   F: mean: ((P^0 + P^1) + ...) * (1.0f / H), ascending h;  max / min: the running maximum / minimum in ascending h (a NaN stays)
//   rho: mean: 2, by definition (c = r_in * 0.5f);  max / min: 1.0f + sum_j F[i, j], the columns of a lane in ascending order over
//             the column tiles the workgroup walks, then the two half-waves, then the two waves, then the workgroups' slabs in
//             ascending order;  c[i] = r_in[i] / rho[i]
//   r_out[j] = sum_i c[i] * t,  t = F[i, j] (+ 1.0f where i == j): product rounded, then added; the rows of a lane in ascending order
//             over the row tiles the workgroup walks, then the two half-waves, then the two waves
// Passes per step: ro_stats_kernel (lse of every head: 64 rows of q against all column tiles), for max / min ro_rho_kernel (the fused
// row sums: per column tile the heads in ascending order), then ro_colsum_kernel with the operands swapped -- a workgroup owns 64
// COLUMNS j (rows of k as the tile's rows, so a lane holds 16 rows i of one column j and sums them in registers) and walks the row
// tiles of q.  Small N: in the two summing passes the tiles of a block are dealt round-robin to gridDim.y = split workgroups
// (sim_split under RO_MAX_SPLIT, a function of N alone: r_out[b] does not depend on B); each writes its partial sums to slab y of
// ws and ro_fold_kernel adds the slabs in ascending y (the pattern of retrieval_topk.hip's merge and gemm.hip's wgrad_fold_kernel;
// the row sums are folded and consumed before the column sums reuse the slabs).  No atomics at all: two launches give the same bits.
// Tails are masked by index: the LDS image of a row past N is zero, its lse and weight read as 0, and an index test keeps it out of
// every sum.  A non-finite q or k comes out as NaN in r_out, never as a fault.  Grids are flat in x (b, h and the block index folded:
// the entry point refuses more than 2^31 - 1 workgroups); every global offset is long long.  No 16-bit operand: the two builds of
// the library hold the same code.
//   work: (2 or 3) B H N N (2 HD flop on the matrix cores + one expf);  ws: (B H N + [max / min] B N + [split > 1] split B N) floats
#include <cstdint>
#include <cmath>
#include "common.hpp"
#include "simtile.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int RO_MAX_HD = 128;
constexpr int RO_MAX_SPLIT = 64;    // the cap on the tile split of the two summing passes: ws holds one slab [B][N] per split
constexpr int RO_MEAN = 0, RO_MAX = 1, RO_MIN = 2;

// (m1, s1) + (m2, s2) of two partial log-sum-exps (csrc/cliploss.hip's merge): an empty partial is (-inf, 0), equal maxima take the
// factor 1 without an exp
__device__ __forceinline__ void ro_merge(float& m1, float& s1, float m2, float s2) {
  const float M = fmaxf(m1, m2);
  const float e1 = m1 == M ? 1.0f : expf(m1 - M);
  const float e2 = m2 == M ? 1.0f : expf(m2 - M);
  s1 = s1 * e1 + s2 * e2;
  m1 = M;
}

// a NaN in either operand stays (fmaxf / fminf would drop it and a poisoned head would come out clean)
__device__ __forceinline__ float ro_fuse(float f, float p, int fusion) {
  if (fusion == RO_MEAN) return f + p;
  if (fusion == RO_MAX) return (p > f || p != p) ? p : f;
  return (p < f || p != p) ? p : f;
}

// the four partials of a row, held by lane (wr, r) of half-wave h in wave column wc: h 0 + h 1, then wc 0 + wc 1; the result is in
// the lanes with wc == 0 && h == 0 (ends with a barrier before `red` is read; the caller puts one behind its last use)
__device__ __forceinline__ float ro_row_sum(float v, float* red, int il, int wc, int h) {
  const float o = __shfl_xor(v, 32, 64);
  v = h == 0 ? v + o : o + v;
  if (wc == 1 && h == 0) red[il] = v;
  __syncthreads();
  return v + red[il];
}

// lse[(b H + hd) N + i] for the 64 rows i of one row block of one (b, hd)
__global__ __launch_bounds__(SIM_THREADS) void ro_stats_kernel(const float* __restrict__ q, long long qs, const float* __restrict__ k,
                                                             long long ks, long long N, int H, int d, float scale, long long row_blocks,
                                                             float* __restrict__ lse) {
  __shared__ float smem[2 * SIM_ROWS * SIM_LD];
  __shared__ float red[SIM_ROWS * 2];
  float* As = smem;
  float* Bs = smem + SIM_ROWS * SIM_LD;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long bh = (long long)blockIdx.x / row_blocks;
  const long long i0 = ((long long)blockIdx.x % row_blocks) * SIM_ROWS;
  const long long b = bh / H;
  const int hd = (int)(bh % H);
  const float* qh = q + b * N * qs + (long long)hd * d;
  const float* kh = k + b * N * ks + (long long)hd * d;
  const long long col_tiles = (N + SIM_COLS - 1) / SIM_COLS;
  auto q_row = [&](int rr) -> long long { return i0 + rr < N ? i0 + rr : -1; };

  const int il = wr * 32 + r;
  float mx = -INFINITY, sm = 0.0f;
  for (long long ct = 0; ct < col_tiles; ++ct) {
    const long long j0 = ct * SIM_COLS;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    auto k_row = [&](int cc) -> long long { return j0 + cc < N ? j0 + cc : -1; };
    SIM_SCORE_TILE(acc, As, Bs, qh, qs, q_row, kh, ks, k_row);
    float z[16];
    float tmax = -INFINITY;
    bool any = false;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const bool in = SIM_COL(j0 + wc * 32, g, h) < N;
      z[g] = scale * acc[g];
      if (in) tmax = fmaxf(tmax, z[g]);
      any |= in;
    }
    if (any) {
      const float nm = fmaxf(mx, tmax);
      float s = sm * (mx == nm ? 1.0f : expf(mx - nm));
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const bool in = SIM_COL(j0 + wc * 32, g, h) < N;
        if (in) s += expf(z[g] - nm);
      }
      sm = s;
      mx = nm;
    }
  }
  {
    const float om = __shfl_xor(mx, 32, 64), os = __shfl_xor(sm, 32, 64);
    if (h == 0) {
      ro_merge(mx, sm, om, os);
    } else {
      float m2 = om, s2 = os;
      ro_merge(m2, s2, mx, sm);
      mx = m2;
      sm = s2;
    }
  }
  if (wc == 1 && h == 0) {
    red[il * 2] = mx;
    red[il * 2 + 1] = sm;
  }
  __syncthreads();
  if (wc == 0 && h == 0 && i0 + il < N) {
    ro_merge(mx, sm, red[il * 2], red[il * 2 + 1]);
    lse[bh * N + i0 + il] = mx + logf(sm);
  }
}

// out[(y B + b) N + i] = sum over the column tiles ct = y, y + gridDim.y, ... of sum_j fuse_h P^h[i, j] for the 64 rows i of one row
// block of one b (max / min fusion only); with one workgroup per block out is rho itself and the leading 1.0f is added here
__global__ __launch_bounds__(SIM_THREADS) void ro_rho_kernel(const float* __restrict__ q, long long qs, const float* __restrict__ k,
                                                           long long ks, long long N, int H, int d, float scale, int fusion,
                                                           long long row_blocks, const float* __restrict__ lse, int B,
                                                           float* __restrict__ out) {
  __shared__ float smem[2 * SIM_ROWS * SIM_LD];
  __shared__ float red[SIM_ROWS];
  float* As = smem;
  float* Bs = smem + SIM_ROWS * SIM_LD;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long b = (long long)blockIdx.x / row_blocks;
  const long long i0 = ((long long)blockIdx.x % row_blocks) * SIM_ROWS;
  const long long col_tiles = (N + SIM_COLS - 1) / SIM_COLS;
  auto q_row = [&](int rr) -> long long { return i0 + rr < N ? i0 + rr : -1; };
  const int il = wr * 32 + r;
  const bool iin = i0 + il < N;

  float rs = 0.0f;
  for (long long ct = blockIdx.y; ct < col_tiles; ct += gridDim.y) {
    const long long j0 = ct * SIM_COLS;
    auto k_row = [&](int cc) -> long long { return j0 + cc < N ? j0 + cc : -1; };
    float f[16];
    for (int hd = 0; hd < H; ++hd) {
      const float* qh = q + b * N * qs + (long long)hd * d;
      const float* kh = k + b * N * ks + (long long)hd * d;
      const float l = iin ? lse[(b * H + hd) * N + i0 + il] : 0.0f;
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
      SIM_SCORE_TILE(acc, As, Bs, qh, qs, q_row, kh, ks, k_row);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float z = scale * acc[g];
        const float p = expf(z - l);
        f[g] = hd == 0 ? p : ro_fuse(f[g], p, fusion);
      }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g)
      if (SIM_COL(j0 + wc * 32, g, h) < N) rs += f[g];
  }
  const float total = ro_row_sum(rs, red, il, wc, h);
  if (wc == 0 && h == 0 && iin) out[((long long)blockIdx.y * B + b) * N + i0 + il] = gridDim.y == 1 ? 1.0f + total : total;
}

// out[(y B + b) N + j] = sum over the row tiles it = y, y + gridDim.y, ... of sum_i c[i] (F[i, j] + [i == j]) for the 64 columns j of
// one column block of one b; the tile's rows are rows of k (the columns j), its columns rows of q (the rows i)
__global__ __launch_bounds__(SIM_THREADS) void ro_colsum_kernel(const float* __restrict__ q, long long qs, const float* __restrict__ k,
                                                              long long ks, int B, long long N, int H, int d, float scale, int fusion,
                                                              float inv_h, long long col_blocks, const float* __restrict__ lse,
                                                              const float* __restrict__ rho, const float* __restrict__ r_in,
                                                              float* __restrict__ out) {
  __shared__ float smem[2 * SIM_ROWS * SIM_LD];
  __shared__ float red[SIM_ROWS];
  __shared__ float cs[SIM_COLS];      // c[i] of the row tile; 0 past N
  __shared__ float ls[SIM_COLS];      // lse[b][hd][i] of the row tile; 0 past N
  float* As = smem;
  float* Bs = smem + SIM_ROWS * SIM_LD;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long b = (long long)blockIdx.x / col_blocks;
  const long long j0 = ((long long)blockIdx.x % col_blocks) * SIM_ROWS;
  const long long row_tiles = (N + SIM_COLS - 1) / SIM_COLS;
  auto k_row = [&](int rr) -> long long { return j0 + rr < N ? j0 + rr : -1; };
  const int jl = wr * 32 + r;
  const long long j = j0 + jl;

  float cacc = 0.0f;
  for (long long it = blockIdx.y; it < row_tiles; it += gridDim.y) {
    const long long i0 = it * SIM_COLS;
    auto q_row = [&](int cc) -> long long { return i0 + cc < N ? i0 + cc : -1; };
    if (tid < SIM_COLS) {
      const long long i = i0 + tid;
      float c = 0.0f;
      if (i < N) c = fusion == RO_MEAN ? r_in[b * N + i] * 0.5f : r_in[b * N + i] / rho[b * N + i];
      cs[tid] = c;
    }
    float f[16];
    for (int hd = 0; hd < H; ++hd) {
      const float* qh = q + b * N * qs + (long long)hd * d;
      const float* kh = k + b * N * ks + (long long)hd * d;
      if (tid < SIM_COLS) ls[tid] = i0 + tid < N ? lse[(b * H + hd) * N + i0 + tid] : 0.0f;
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
      SIM_SCORE_TILE(acc, As, Bs, kh, ks, k_row, qh, qs, q_row);     // its first barrier publishes cs and ls
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float z = scale * acc[g];
        const float p = expf(z - ls[SIM_COL(wc * 32, g, h)]);
        f[g] = hd == 0 ? p : ro_fuse(f[g], p, fusion);
      }
      __syncthreads();                                               // the next head rewrites ls
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int li = SIM_COL(wc * 32, g, h);
      const long long i = i0 + li;
      if (i < N) {
        float t = fusion == RO_MEAN ? f[g] * inv_h : f[g];
        if (i == j) t = t + 1.0f;
        cacc += cs[li] * t;
      }
    }
    __syncthreads();                                                 // the next row tile rewrites cs
  }
  const float total = ro_row_sum(cacc, red, jl, wc, h);
  if (wc == 0 && h == 0 && j < N) out[((long long)blockIdx.y * B + b) * N + j] = total;
}

// out[e] = ((slab 0 + slab 1) + ...)[e], ascending; with `lead_one` 1.0f + that sum (rho)
__global__ __launch_bounds__(SIM_THREADS) void ro_fold_kernel(const float* __restrict__ slabs, int split, long long n, int lead_one,
                                                            float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (e >= n) return;
  float v = slabs[e];
  for (int y = 1; y < split; ++y) v += slabs[(long long)y * n + e];
  out[e] = lead_one ? 1.0f + v : v;
}

struct RoPlan {
  long long blocks;      // blocks of 64 rows (or columns) of one sample
  int split;             // workgroups that share a column block's row tiles
  long long lse_floats, rho_floats, slab_floats;
};

static bool ro_plan(int B, long long N, int H, int fusion, RoPlan* p) {
  if (B <= 0 || N <= 0 || H <= 0 || N > 0x7fffffffLL || fusion < RO_MEAN || fusion > RO_MIN) return false;
  p->blocks = (N + SIM_ROWS - 1) / SIM_ROWS;
  const long long bh = (long long)B * H;                           // < 2^62
  if (bh > 0x7fffffffLL || bh * p->blocks > 0x7fffffffLL) return false;   // the statistics' grid: (b, h, row block) folded into x
  p->split = (int)sim_split(p->blocks, p->blocks, RO_MAX_SPLIT);   // of N alone
  p->lse_floats = bh * N;                                          // < 2^62
  p->rho_floats = fusion == RO_MEAN ? 0 : (long long)B * N;
  p->slab_floats = p->split > 1 ? (long long)p->split * B * N : 0;
  return true;
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_rollout_ws(int B, long long N, int H, int fusion) {
  RoPlan p;
  if (!ro_plan(B, N, H, fusion, &p)) return -2;
  const unsigned __int128 bytes = ((unsigned __int128)p.lse_floats + p.rho_floats + p.slab_floats) * 4u;   // each count is below 2^62
  return bytes > (unsigned __int128)0x7fffffff ? -2 : (int)bytes;
}

extern "C" int octmae_rollout_step(const float* q, long long q_stride, const float* k, long long k_stride, int B, long long N, int H,
                                   int HD, float scale, int fusion, const float* r_in, float* r_out, void* ws, long long ws_bytes,
                                   void* stream) {
  if (!q || !k || !r_in || !r_out || !ws) return -2;
  if (r_in == r_out) return -2;
  if (HD < 1 || HD > RO_MAX_HD) return -2;
  RoPlan p;
  if (!ro_plan(B, N, H, fusion, &p)) return -2;
  const long long width = (long long)H * HD;
  if (q_stride < width || k_stride < width) return -2;
  const long long need = octmae_rollout_ws(B, N, H, fusion);
  if (need < 0 || ws_bytes < need) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* lse = reinterpret_cast<float*>(ws);
  float* rho = lse + p.lse_floats;
  float* slabs = rho + p.rho_floats;
  const long long bn = (long long)B * N;
  hipLaunchKernelGGL(ro_stats_kernel, dim3((unsigned)((long long)B * H * p.blocks)), dim3(SIM_THREADS), 0, st, q, q_stride, k, k_stride, N, H,
                     HD, scale, p.blocks, lse);
  OCTMAE_LAUNCH_CHECK();
  if (fusion != RO_MEAN) {
    hipLaunchKernelGGL(ro_rho_kernel, dim3((unsigned)(B * p.blocks), (unsigned)p.split), dim3(SIM_THREADS), 0, st, q, q_stride, k, k_stride,
                       N, H, HD, scale, fusion, p.blocks, lse, B, p.split > 1 ? slabs : rho);
    OCTMAE_LAUNCH_CHECK();
    if (p.split > 1) {
      hipLaunchKernelGGL(ro_fold_kernel, dim3((unsigned)((bn + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, st, slabs, p.split, bn,
                         1, rho);
      OCTMAE_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(ro_colsum_kernel, dim3((unsigned)(B * p.blocks), (unsigned)p.split), dim3(SIM_THREADS), 0, st, q, q_stride, k, k_stride,
                     B, N, H, HD, scale, fusion, 1.0f / (float)H, p.blocks, lse, fusion != RO_MEAN ? rho : (const float*)nullptr, r_in,
                     p.split > 1 ? slabs : r_out);
  OCTMAE_LAUNCH_CHECK();
  if (p.split > 1) {
    hipLaunchKernelGGL(ro_fold_kernel, dim3((unsigned)((bn + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, st, slabs, p.split, bn,
                       0, r_out);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
