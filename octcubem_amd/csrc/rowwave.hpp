// The row-per-wave LayerNorm skeleton shared by layernorm.hip, pool.hip and join.hip: one wave owns one row of D floats, lane t holds
// the float4 chunks t, t + 64, ... in NC register slots.  Every expression whose bits two kernels must agree on (the row statistics,
// the affine output, dx, the four-wave column fold) is stated here once; a new row-per-wave kernel starts from this header.
#pragma once
#include "common.hpp"

// The chunk slots of a lane: `ROW_CHUNKS(c, ci) stmt` runs stmt for slot c = 0 .. NC - 1 whose chunk ci = lane + 64 c lies inside the
// row.  NC (a template parameter: the loop unrolls fully), lane and nchunk = D / 4 are the caller's.  A macro, not a function taking
// a lambda: the lambda form changes register allocation wholesale (ln_fwd_kernel<8>: 396 -> 144 VGPRs), a change to be measured.
#define ROW_CHUNKS(c, ci) _Pragma("unroll") for (int c = 0; c < NC; ++c) if (const int ci = lane + 64 * c; ci < nchunk)

// Row operands are read exactly once: their loads are non-temporal, like the stores of the outputs.  Measured same box
// (profiles/r04_layernorm_nt_loads.txt): forward 5.85 -> 6.10 TB/s, backward 5.91 -> 6.12 at D = 1024 inside the training step,
// +0.17 % on the step.  ROW_PLAIN_LOADS (defined by the including file before the include): ordinary loads, for A/B builds.
#ifndef ROW_PLAIN_LOADS
#define ROW_LD(T, p) __builtin_nontemporal_load(reinterpret_cast<const T*>(p))
#else
#define ROW_LD(T, p) (*reinterpret_cast<const T*>(p))
#endif

namespace octmae {

constexpr int ROW_MAXC = 8;  // float4 chunks per lane -> D <= 2048

// The arithmetic below is stated as macros, not functions: hipcc optimises a function (unrolls its loops, picks its operand order and
// contractions) BEFORE it inlines it, and the calling kernels then come out scheduled differently from the same text written in place
// (seen with ln_fwd_kernel<1>, every ln_bwd_kernel and pool_bwd_rows_kernel).  Textual substitution leaves the device code what it was.

// ---- row statistics: a lane's share of sum(v) and of sum((v - mu)^2) for one chunk; the caller reduces with wave_sum ----
#define ROW_SUM4(v) (((v)[0] + (v)[1]) + ((v)[2] + (v)[3]))
#define ROW_SQDEV4(q, v, mu)                      \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) { \
    const float d_ = (v)[e] - (mu);               \
    (q) = fmaf(d_, d_, (q));                      \
  }

// ---- y = xhat * gamma + beta; LN_AFFINE_STORE: four columns, rounded to the 16-bit operand type, stored non-temporally (8 bytes) ----
#define LN_AFFINE(v, mu, rs, g, b) fmaf(((v) - (mu)) * (rs), g, b)
#define LN_AFFINE_STORE(v, mu, rs, g, b, dst)                                                              \
  do {                                                                                                     \
    float o_[4];                                                                                           \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) o_[e] = LN_AFFINE((v)[e], mu, rs, (g)[e], (b)[e]);       \
    u32x2 w_ = {pack2bf(o_[0], o_[1]), pack2bf(o_[2], o_[3])};                                             \
    __builtin_nontemporal_store(w_, reinterpret_cast<u32x2*>(dst));                                        \
  } while (0)

// ---- dx = rstd * (gy - mean(gy) - xhat * mean(gy * xhat)),  gy = dy * gamma ----
#define LN_DX(rs, gy, m1, xhat, m2) ((rs) * ((gy) - (m1) - (xhat) * (m2)))

// ---- column sums over the four waves of a workgroup ----
// Every lane holds, for the chunk slot of chunk ci, K per-lane column partials.  ROW_FOLD4(K, ci, DST, v0, .., vK-1) is executed by
// all 256 threads (it has barriers): element e of quantity k is the expression vk (in e); wave k < K then owns quantity k, adds the
// four waves' values as (w0 + w1) + (w2 + w3) and, where ci lies inside the row, stores the float4 to DST (an expression in w).
// The caller's names: `__shared__ RowRed red[K]`, lane, w = the wave of the workgroup, nchunk.
typedef float RowRed[4][64 * 4 + 4];
template <int K, typename... V>
__device__ __forceinline__ void row_fold_put(RowRed (&red)[K], int w, int i, V... v) {
  static_assert(sizeof...(V) == K, "one value per quantity");
  int k = 0;
  ((red[k++][w][i] = v), ...);
}
#define ROW_FOLD4(K, ci, DST, ...)                                                                                               \
  do {                                                                                                                           \
    __syncthreads();                                                                                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) row_fold_put(red, w, lane * 4 + e, __VA_ARGS__);                               \
    __syncthreads();                                                                                                             \
    if (w < K && ci < nchunk) {                                                                                                  \
      f32x4 t;                                                                                                                   \
      _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                              \
        t[e] = (red[w][0][lane * 4 + e] + red[w][1][lane * 4 + e]) + (red[w][2][lane * 4 + e] + red[w][3][lane * 4 + e]);        \
      *reinterpret_cast<f32x4*>(DST) = t;                                                                                        \
    }                                                                                                                            \
  } while (0)

// ---- host side ----
static inline int row_nc(int D) { return (D / 4 + 63) / 64; }      // chunk slots a lane needs
static inline bool row_shape_ok(int M, int D) { return M > 0 && D > 0 && D % 4 == 0 && D <= 256 * ROW_MAXC; }

}  // namespace octmae

// Launches KERNEL<NC> with the smallest NC of 1, 2, 4, 8 that holds `nc` chunk slots, on the stream `st` (both the caller's names).
#define ROW_DISPATCH(KERNEL, GRID, BLK, ...)                                                  \
  switch (nc) {                                                                               \
    case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, BLK, 0, st, __VA_ARGS__); break;              \
    case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, BLK, 0, st, __VA_ARGS__); break;              \
    case 3: case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, BLK, 0, st, __VA_ARGS__); break;      \
    default: hipLaunchKernelGGL(KERNEL<8>, GRID, BLK, 0, st, __VA_ARGS__); break;             \
  }
