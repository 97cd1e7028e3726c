// The contrastive loss of the COEM training step (retinal-COEM/src/open_clip/loss.py:148-230 ClipLoss, :230-385 ThreeModalityClipLoss):
// logit_scale * a @ b.T, its transpose, two cross entropies and their autograd, as one walk over f32 MFMA tiles of a . b^T that keeps
// no [n][m] array -- csrc/retrieval.hip's walk (the tile, its staging and its k loop are csrc/simtile.hpp's) with a log-sum-exp in
// place of its counts, plus a backward.
//   a f32 [n][d], b f32 [m][d] (row strides >= d);  s(i, j) = the f32 chain acc = fmaf(a[i][k], b[j][k], acc), k = 0 .. d-1 (retrieval.hip's
//   score, from v_mfma_f32_32x32x2_f32);  z = scale * s (one rounding; scale is read from device memory);  t_i = i + offset
//     L = sum_i wr_i (lse_j z(i, j) - z(i, t_i))  +  sum_i wc_i (lse_i' z(i', t_i) - z(i, t_i))          (second sum only with wc)
//     G(i, j) = wr_i (p_ij - [j == t_i]) + wc_{j - offset} (q_ij - [j == t_i]),  p = exp(z - lse_row_i), q = exp(z - lse_col_j)
//     da = g scale G b,  db = g scale G^T a,  dscale = g sum G o s
// Forward: clip_lse_kernel owns 64 rows of one side and walks 64-column tiles of the other with an online (max, sum) per row; the column
// tiles are dealt round-robin to gridDim.y workgroups per row block, each writes its (max, sum) partial and clip_finish_kernel merges them
// IN ORDER (no float crosses a workgroup through an atomic).  The same kernel with the sides swapped gives the column log-sum-exps.  The
// target scores come from the VALU chain over the staged rows (the tile's own bits, as in retrieval.hip).  clip_loss_kernel sums L in one
// workgroup, float64, fixed order.
// Backward: clip_grad_kernel owns 64 rows of the side it differentiates and one chunk of CL_DC = 256 feature columns (gridDim.y); per
// tile of the other side it recomputes s from the operands (16 k-steps of 32 through LDS), forms G from the saved log-sum-exps, parks the
// 64 x 64 G tile in LDS (over the operand images, which are dead by then) and adds G . y[:, chunk] into four 32 x 32 accumulators per
// wave with the same f32 MFMA (y straight from global memory: each value feeds one MFMA of the wave).  db is the same kernel with the
// sides swapped.  dscale: one partial per row of a from the a-side workgroups of chunk 0, summed by clip_dscale_kernel in float64, fixed order.
// Every output element is summed in a fixed order: two runs are bit-equal.  No 16-bit operand, no fast-math flag and no contraction
// (the Makefile compiles this file with -ffp-contract=off: the roundings are the ones written here); exp / log are the device library's
// expf / logf (1 ulp).  Tails are masked by index, never by a sentinel score; a non-finite feature comes out as NaN, not as a fault.
#include <cstdint>
#include <cmath>
#include "common.hpp"
#include "simtile.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int CL_GLD = SIM_COLS + 1;   // LDS row pitch of the G tile
constexpr int CL_DC = 256;         // feature columns per backward workgroup: 2 column halves (waves) x CL_NQ accumulators x 32
constexpr int CL_NQ = 4;
constexpr int CL_MAX_SPLIT = 64;   // the cap on the forward's column split: its workspace holds one (max, sum) per split and row
constexpr int CL_SMEM = 2 * SIM_ROWS * SIM_LD;   // floats: the two operand images; the G tile lies over them
static_assert(SIM_ROWS * CL_GLD <= CL_SMEM, "the G tile fits over the operand images");
static_assert(CL_DC == 2 * CL_NQ * 32, "two waves side by side, CL_NQ accumulators each");

// acc[g] = s(x, y) for x = i0 + wr * 32 + r (this lane's row) and y = SIM_COL(j0 + wc * 32, g, h): the tile of csrc/simtile.hpp, the
// other side as the MFMA's A operand.  Ends with a barrier: the images may be rewritten.
__device__ __forceinline__ f32x16 cl_score_tile(float* As, float* Bs, const float* __restrict__ x, long long xs, long long i0, long long nx,
                                                const float* __restrict__ y, long long ys, long long j0, long long ny, int d) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
  auto x_row = [&](int rr) -> long long { return i0 + rr < nx ? i0 + rr : -1; };
  auto y_row = [&](int cc) -> long long { return j0 + cc < ny ? j0 + cc : -1; };
  SIM_SCORE_TILE(acc, As, Bs, x, xs, x_row, y, ys, y_row);
  return acc;
}

// (m1, s1) + (m2, s2) of two partial log-sum-exps, sum_j exp(z_j) = s exp(m).  An empty partial is (-inf, 0); equal maxima take the
// factor 1 without an exp, so -inf - -inf never forms from two empty partials and a NaN sum stays NaN.
__device__ __forceinline__ void cl_merge(float& m1, float& s1, float m2, float s2) {
  const float M = fmaxf(m1, m2);
  const float e1 = m1 == M ? 1.0f : expf(m1 - M);
  const float e2 = m2 == M ? 1.0f : expf(m2 - M);
  s1 = s1 * e1 + s2 * e2;
  m1 = M;
}

// part[(blockIdx.y * nx + i) * 2 + {0, 1}] = (max, sum) of row i of x over the column tiles this workgroup walks;
// tsc[i] = s(i, i + offset) from the workgroups with blockIdx.y == 0 when tsc is given
__global__ __launch_bounds__(SIM_THREADS) void clip_lse_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ y,
                                                             long long ys, const float* __restrict__ scale_p, float* __restrict__ part,
                                                             float* __restrict__ tsc, long long offset, long long nx, long long ny, int d,
                                                             int col_tiles) {
  __shared__ float smem[CL_SMEM];
  __shared__ float red[SIM_ROWS * 2];
  float* As = smem;
  float* Bs = smem + SIM_ROWS * SIM_LD;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;
  const float scale = *scale_p;

  if (tsc != nullptr && blockIdx.y == 0) {                      // workgroup-uniform
    float t = 0.0f;
    auto x_row = [&](int rr) -> long long { return i0 + rr < nx ? i0 + rr : -1; };
    auto t_row = [&](int rr) -> long long { return i0 + rr < nx ? i0 + rr + offset : -1; };   // n + offset <= m: checked
    SIM_TARGET_CHAIN(t, As, Bs, x, xs, x_row, y, ys, t_row);
    if (tid < SIM_ROWS && i0 + tid < nx) tsc[i0 + tid] = t;
  }

  const int il = wr * 32 + r;
  float mx = -INFINITY, sm = 0.0f;
  for (int ct = (int)blockIdx.y; ct < col_tiles; ct += (int)gridDim.y) {
    const long long j0 = (long long)ct * SIM_COLS;
    const f32x16 acc = cl_score_tile(As, Bs, x, xs, i0, nx, y, ys, j0, ny, d);
    float z[16];
    float tmax = -INFINITY;
    bool any = false;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const bool in = SIM_COL(j0 + wc * 32, g, h) < ny;
      z[g] = scale * acc[g];
      if (in) tmax = fmaxf(tmax, z[g]);
      any |= in;
    }
    if (any) {
      const float nm = fmaxf(mx, tmax);
      float s = sm * (mx == nm ? 1.0f : expf(mx - nm));
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const bool in = SIM_COL(j0 + wc * 32, g, h) < ny;
        if (in) s += expf(z[g] - nm);
      }
      sm = s;
      mx = nm;
    }
  }
  // a row's columns lie in the two half-waves of two waves: h first, then wc, always in this order
  {
    const float om = __shfl_xor(mx, 32, 64), os = __shfl_xor(sm, 32, 64);
    if (h == 0) {
      cl_merge(mx, sm, om, os);
    } else {
      float m2 = om, s2 = os;
      cl_merge(m2, s2, mx, sm);
      mx = m2;
      sm = s2;
    }
  }
  if (wc == 1 && h == 0) {
    red[il * 2] = mx;
    red[il * 2 + 1] = sm;
  }
  __syncthreads();
  if (wc == 0 && h == 0 && i0 + il < nx) {
    cl_merge(mx, sm, red[il * 2], red[il * 2 + 1]);
    float* o = part + ((long long)blockIdx.y * nx + i0 + il) * 2;
    o[0] = mx;
    o[1] = sm;
  }
}

// lse[i] = log sum over the `split` partials of row i, merged in order
__global__ __launch_bounds__(SIM_THREADS) void clip_finish_kernel(const float* __restrict__ part, int split, long long nx,
                                                                float* __restrict__ lse) {
  const long long i = (long long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= nx) return;
  float m = part[i * 2], s = part[i * 2 + 1];
  for (int p = 1; p < split; ++p) cl_merge(m, s, part[((long long)p * nx + i) * 2], part[((long long)p * nx + i) * 2 + 1]);
  lse[i] = m + logf(s);
}

// fixed-order float64 sum of one value per thread-strided index: v(i) for i = tid, tid + 256, ...; then a tree over the 256 threads
template <class F>
__device__ __forceinline__ double cl_block_sum(long long n, F v) {
  __shared__ double acc[SIM_THREADS];
  double t = 0.0;
  for (long long i = threadIdx.x; i < n; i += SIM_THREADS) t += v(i);
  acc[threadIdx.x] = t;
  __syncthreads();
  for (int w = SIM_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
    __syncthreads();
  }
  return acc[0];
}

__global__ __launch_bounds__(SIM_THREADS) void clip_loss_kernel(const float* __restrict__ scale_p, const float* __restrict__ wr,
                                                              const float* __restrict__ wc, const float* __restrict__ lse_row,
                                                              const float* __restrict__ lse_col, const float* __restrict__ tsc,
                                                              long long offset, long long n, float* __restrict__ loss) {
  const float scale = *scale_p;
  const double L = cl_block_sum(n, [&](long long i) -> double {
    const float zt = scale * tsc[i];
    double t = (double)(wr[i] * (lse_row[i] - zt));
    if (wc != nullptr) t += (double)(wc[i] * (lse_col[i + offset] - zt));
    return t;
  });
  if (threadIdx.x == 0) *loss = (float)L;
}

__global__ __launch_bounds__(SIM_THREADS) void clip_dscale_kernel(const float* __restrict__ gout, const float* __restrict__ dsp, long long n,
                                                                float* __restrict__ dscale) {
  const double S = cl_block_sum(n, [&](long long i) -> double { return (double)dsp[i]; });
  if (threadIdx.x == 0) *dscale = (float)((double)*gout * S);
}

// weight table `w` of `cnt` entries seen at index idx - shift; 0 outside it or without a table
__device__ __forceinline__ float cl_weight(const float* __restrict__ w, long long shift, long long cnt, long long idx) {
  const long long k = idx - shift;
  return (w != nullptr && k >= 0 && k < cnt) ? w[k] : 0.0f;
}

// dx[x][c] = g scale sum_y G(x, y) y[y][c] for the 64 rows x of blockIdx.x and the CL_DC columns c of blockIdx.y, with
//   G(x, y) = wx_x (exp(z - lx_x) - [y - x == delta]) + wy_y (exp(z - ly_y) - [y - x == delta])
// (a term whose weight table is NULL is left out: its log-sum-exps are not read).  dsp[x] = sum_y G(x, y) s(x, y) from the
// workgroups of chunk 0 when dsp is given.  dx == NULL: only dsp.
__global__ __launch_bounds__(SIM_THREADS) void clip_grad_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ y,
                                                              long long ys, const float* __restrict__ scale_p,
                                                              const float* __restrict__ gout, const float* __restrict__ wx, long long wx_shift,
                                                              long long wx_cnt, const float* __restrict__ lx, const float* __restrict__ wy,
                                                              long long wy_shift, long long wy_cnt, const float* __restrict__ ly,
                                                              long long delta, float* __restrict__ dx, long long dxs,
                                                              float* __restrict__ dsp, long long nx, long long ny, int d) {
  __shared__ float smem[CL_SMEM];
  __shared__ double redd[SIM_ROWS];
  float* As = smem;
  float* Bs = smem + SIM_ROWS * SIM_LD;
  float* Gs = smem;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;
  const int c0 = (int)blockIdx.y * CL_DC;
  const float scale = *scale_p;
  const int il = wr * 32 + r;
  const long long xi = i0 + il;
  const bool xin = xi < nx;
  const float wxv = xin ? cl_weight(wx, wx_shift, wx_cnt, xi) : 0.0f;
  const float lxv = (xin && wx != nullptr) ? lx[xi] : 0.0f;
  const bool want_ds = dsp != nullptr && blockIdx.y == 0;          // workgroup-uniform
  const bool want_dx = dx != nullptr;
  double ds = 0.0;
  f32x16 out[CL_NQ];
#pragma unroll
  for (int q = 0; q < CL_NQ; ++q)
#pragma unroll
    for (int g = 0; g < 16; ++g) out[q][g] = 0.0f;

  const long long tiles = (ny + SIM_COLS - 1) / SIM_COLS;
  for (long long ct = 0; ct < tiles; ++ct) {
    const long long j0 = ct * SIM_COLS;
    const f32x16 acc = cl_score_tile(As, Bs, x, xs, i0, nx, y, ys, j0, ny, d);      // ends with a barrier: Gs may be written
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int yl = SIM_COL(wc * 32, g, h);
      const long long yj = j0 + yl;
      float G = 0.0f;
      if (xin && yj < ny) {
        const float s = acc[g];
        const float z = scale * s;
        const float hit = (yj - xi == delta) ? 1.0f : 0.0f;
        if (wx != nullptr) G = wxv * (expf(z - lxv) - hit);
        if (wy != nullptr) G = G + cl_weight(wy, wy_shift, wy_cnt, yj) * (expf(z - ly[yj]) - hit);
        ds += (double)G * (double)s;
      }
      Gs[il * CL_GLD + yl] = G;
    }
    __syncthreads();
    if (want_dx) {
      const float* pg = &Gs[il * CL_GLD + h];                    // MFMA A operand: lane = row x of the block, k = y = 2 step + h
#pragma unroll 8
      for (int s = 0; s < SIM_COLS / 2; ++s) {
        const float ga = pg[2 * s];
        const long long yrow = j0 + 2 * s + h;
        const bool yok = yrow < ny;
#pragma unroll
        for (int q = 0; q < CL_NQ; ++q) {
          const int cb = c0 + wc * (CL_NQ * 32) + q * 32;        // wave-uniform
          if (cb < d) {
            const int c = cb + r;                                // MFMA B operand: lane = feature column
            const float bv = (yok && c < d) ? y[yrow * ys + c] : 0.0f;
            out[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, bv, out[q], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();                                             // the next tile's images overwrite Gs
  }

  if (want_dx) {
    const float coef = *gout * scale;
#pragma unroll
    for (int q = 0; q < CL_NQ; ++q) {
      const int c = c0 + wc * (CL_NQ * 32) + q * 32 + r;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const long long row = SIM_COL(i0 + wr * 32, g, h);
        if (row < nx && c < d) dx[row * dxs + c] = coef * out[q][g];
      }
    }
  }
  if (want_ds) {
    ds += __shfl_xor(ds, 32, 64);                                // a + b == b + a: both halves hold the same bits
    if (wc == 1 && h == 0) redd[il] = ds;
    __syncthreads();
    if (wc == 0 && h == 0 && xin) dsp[xi] = (float)(ds + redd[il]);
  }
}

struct ClPlan {
  long long row_blocks_a, row_blocks_b;
  int tiles_a, tiles_b;        // column tiles seen from the a side (over m) and from the b side (over n)
  int split_a, split_b;
};

static bool cl_plan(long long n, long long m, ClPlan* p) {
  if (n <= 0 || m <= 0 || n > 0x7fffffffLL || m > 0x7fffffffLL) return false;
  p->row_blocks_a = (n + SIM_ROWS - 1) / SIM_ROWS;
  p->row_blocks_b = (m + SIM_ROWS - 1) / SIM_ROWS;
  p->tiles_a = (int)((m + SIM_COLS - 1) / SIM_COLS);
  p->tiles_b = (int)((n + SIM_COLS - 1) / SIM_COLS);
  p->split_a = (int)sim_split(p->row_blocks_a, p->tiles_a, CL_MAX_SPLIT);
  p->split_b = (int)sim_split(p->row_blocks_b, p->tiles_b, CL_MAX_SPLIT);
  return true;
}

static long long cl_ws_floats(const ClPlan& p, long long n, long long m) {
  return 2 * ((long long)p.split_a * n + (long long)p.split_b * m);   // >= n: the backward's dscale partials fit too
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_clip_loss_ws_floats(long long n, long long m) {
  ClPlan p;
  if (!cl_plan(n, m, &p)) return -2;
  const long long f = cl_ws_floats(p, n, m);
  return f > 0x7fffffffLL ? -2 : (int)f;
}

extern "C" int octmae_clip_loss_fwd(const float* a, long long a_stride, const float* b, long long b_stride, const float* scale,
                                    const float* wr, const float* wc, long long offset, float* lse_row, float* lse_col, float* tscore,
                                    float* loss, float* ws, long long ws_floats, long long n, long long m, int d, void* stream) {
  if (!a || !b || !scale || !wr || !lse_row || !tscore || !loss || !ws) return -2;
  if (wc && !lse_col) return -2;
  if (n <= 0 || m <= 0 || d <= 0 || a_stride < d || b_stride < d) return -2;
  if (offset < 0 || n + offset > m) return -2;
  ClPlan p;
  if (!cl_plan(n, m, &p) || ws_floats < cl_ws_floats(p, n, m)) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* part_a = ws;
  float* part_b = ws + 2 * (long long)p.split_a * n;
  hipLaunchKernelGGL(clip_lse_kernel, dim3((unsigned)p.row_blocks_a, (unsigned)p.split_a), dim3(SIM_THREADS), 0, st, a, a_stride, b, b_stride,
                     scale, part_a, tscore, offset, n, m, d, p.tiles_a);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(clip_finish_kernel, dim3((unsigned)((n + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, st, part_a, p.split_a, n,
                     lse_row);
  OCTMAE_LAUNCH_CHECK();
  if (wc) {
    hipLaunchKernelGGL(clip_lse_kernel, dim3((unsigned)p.row_blocks_b, (unsigned)p.split_b), dim3(SIM_THREADS), 0, st, b, b_stride, a, a_stride,
                       scale, part_b, (float*)nullptr, 0LL, m, n, d, p.tiles_b);
    OCTMAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(clip_finish_kernel, dim3((unsigned)((m + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, st, part_b, p.split_b, m,
                       lse_col);
    OCTMAE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(clip_loss_kernel, dim3(1), dim3(SIM_THREADS), 0, st, scale, wr, wc, lse_row, lse_col, tscore, offset, n, loss);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_clip_loss_bwd(const float* a, long long a_stride, const float* b, long long b_stride, const float* scale,
                                    const float* wr, const float* wc, long long offset, const float* lse_row, const float* lse_col,
                                    const float* gout, float* da, long long da_stride, float* db, long long db_stride, float* dscale,
                                    float* ws, long long ws_floats, long long n, long long m, int d, void* stream) {
  if (!a || !b || !scale || !wr || !lse_row || !gout) return -2;
  if (wc && !lse_col) return -2;
  if (dscale && !ws) return -2;
  if (n <= 0 || m <= 0 || d <= 0 || a_stride < d || b_stride < d) return -2;
  if ((da && da_stride < d) || (db && db_stride < d)) return -2;
  if (offset < 0 || n + offset > m) return -2;
  ClPlan p;
  if (!cl_plan(n, m, &p) || (dscale && ws_floats < n)) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned chunks = (unsigned)((d + CL_DC - 1) / CL_DC);
  if (da || dscale) {
    // the a side: x = a (own term: wr, lse_row), y = b (wc seen at j - offset, lse_col); partner y - x == offset
    hipLaunchKernelGGL(clip_grad_kernel, dim3((unsigned)p.row_blocks_a, da ? chunks : 1u), dim3(SIM_THREADS), 0, st, a, a_stride, b, b_stride,
                       scale, gout, wr, 0LL, n, lse_row, wc, offset, n, lse_col, offset, da, da_stride, dscale ? ws : (float*)nullptr, n, m, d);
    OCTMAE_LAUNCH_CHECK();
  }
  if (db) {
    // the b side: x = b (own term: wc seen at j - offset, lse_col), y = a (wr, lse_row); partner y - x == -offset
    hipLaunchKernelGGL(clip_grad_kernel, dim3((unsigned)p.row_blocks_b, chunks), dim3(SIM_THREADS), 0, st, b, b_stride, a, a_stride, scale, gout,
                       wc, offset, n, lse_col, wr, 0LL, n, lse_row, -offset, db, db_stride, (float*)nullptr, m, n, d);
    OCTMAE_LAUNCH_CHECK();
  }
  if (dscale) {
    hipLaunchKernelGGL(clip_dscale_kernel, dim3(1), dim3(SIM_THREADS), 0, st, gout, ws, n, dscale);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
