// The f32 similarity tile shared by retrieval.hip, retrieval_topk.hip and cliploss.hip: one workgroup of 256 threads (2 x 2 waves) owns
// SIM_ROWS = 64 rows of a and walks column tiles of SIM_COLS = 64 rows of b; per tile it walks d in LDS steps of SIM_K = 32 (two
// [64][33] f32 images).  A wave holds one 32 x 32 accumulator of v_mfma_f32_32x32x2_f32, TRANSPOSED: b is the MFMA's A operand and a its
// B operand, so a lane's 16 registers are 16 columns of ONE row.  s(i, j) is bit for bit the chain acc = 0; for k = 0 .. d-1:
// acc = fmaf(a[i][k], b[j][k], acc) -- the MFMA and the VALU chain below give the same bits, and so do the three files: every expression
// they must agree on is stated here once, and a new consumer of the tile starts from this header.  Tails are masked by index: the LDS
// image of a row past the end is zero, not a sentinel score, and the k loop ends at d (an odd d runs its last step with one zero operand
// pair: fmaf(0, 0, acc) == acc under IEEE comparison).
#pragma once
#include "common.hpp"

namespace octmae {

constexpr int SIM_ROWS = 64;        // R: rows of a per workgroup
constexpr int SIM_COLS = 64;        // C: rows of b (columns of the score matrix) per tile
constexpr int SIM_K = 32;           // K: k per LDS step (16 MFMA steps of 2)
constexpr int SIM_LD = SIM_K + 1;   // LDS row pitch in floats: the 32 rows a half-wave reads land on 32 banks
constexpr int SIM_THREADS = 256;
constexpr int SIM_TARGET_WGS = 1024;   // workgroups wanted in flight before the columns stop being split (256 CUs x 4)
static_assert(SIM_ROWS == SIM_COLS && SIM_ROWS == 64 && SIM_THREADS == 256, "2 x 2 waves of 32 x 32, one staging routine for both operands");
static_assert(SIM_K % 2 == 0 && (SIM_ROWS * SIM_K) % SIM_THREADS == 0, "whole MFMA steps, whole staging passes");

// dst[r][k] = src[row_of(r)][k0 + k] for the 64 x SIM_K image; 0 where row_of(r) < 0 or k0 + k >= d (masked again by index downstream)
template <class RowOf>
__device__ __forceinline__ void sim_stage(float* __restrict__ dst, const float* __restrict__ src, long long stride, RowOf row_of, int k0,
                                          int d) {
#pragma unroll
  for (int s = 0; s < SIM_ROWS * SIM_K / SIM_THREADS; ++s) {
    const int e = s * SIM_THREADS + (int)threadIdx.x;
    const int r = e / SIM_K, k = e % SIM_K;
    const long long row = row_of(r);
    float v = 0.0f;
    if (row >= 0 && k0 + k < d) v = src[row * stride + k0 + k];
    dst[r * SIM_LD + k] = v;
  }
}

// The loops below are macros, not functions: hipcc optimises a function before it inlines it, and the kernels then come out with other
// registers and another block layout than the same text written in place (as csrc/rowwave.hpp found for the row kernels).  Their names
// from the caller: wr, wc (the wave's place in the 2 x 2), r = lane & 31, h = lane >> 5, and d.

// acc[g] of a lane is s(i, j) for i = wr * 32 + r and j = SIM_COL(wc * 32, g, h) of the tile.  The base is inside the sum, which stays
// left to right: the other grouping of the same sum comes out with other registers.
#define SIM_COL(base, g, h) ((base) + ((g) & 3) + 8 * ((g) >> 2) + 4 * (h))

// acc += the tile's scores: x rows x_row(0 .. 63) against y rows y_row(0 .. 63) (row functions as sim_stage's), through the images As
// and Bs.  Executed by all 256 threads; ends with a barrier, so the images may be rewritten.
#define SIM_SCORE_TILE(acc, As, Bs, x, xs, x_row, y, ys, y_row)                                                                      \
  for (int k0 = 0; k0 < d; k0 += SIM_K) {                                                                                            \
    sim_stage(As, x, xs, x_row, k0, d);                                                                                              \
    sim_stage(Bs, y, ys, y_row, k0, d);                                                                                              \
    __syncthreads();                                                                                                                 \
    const float* pb = &(Bs)[(wc * 32 + r) * SIM_LD + h];      /* MFMA A operand: lane = score column j, k = 2 step + h */            \
    const float* pa = &(As)[(wr * 32 + r) * SIM_LD + h];      /* MFMA B operand: lane = score row i */                               \
    if (d - k0 >= SIM_K) {                                                                                                           \
      _Pragma("unroll") for (int s = 0; s < SIM_K / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pb[2 * s], pa[2 * s], acc, 0, 0, 0); \
    } else {                                                                                                                         \
      const int steps = (d - k0 + 1) / 2;                     /* the k past d of an odd tail is a zero pair */                       \
      for (int s = 0; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pb[2 * s], pa[2 * s], acc, 0, 0, 0);                \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
  }

// t (of thread tid < 64) += s(x_row(tid), y_row(tid)): the same chain on the VALU over the same staged images, so a score and the tile
// entry of the same two rows hold the same bits.  Executed by all 256 threads; ends with a barrier.
#define SIM_TARGET_CHAIN(t, As, Bs, x, xs, x_row, y, ys, y_row)                                                                      \
  for (int k0 = 0; k0 < d; k0 += SIM_K) {                                                                                            \
    sim_stage(As, x, xs, x_row, k0, d);                                                                                              \
    sim_stage(Bs, y, ys, y_row, k0, d);                                                                                              \
    __syncthreads();                                                                                                                 \
    if (tid < SIM_ROWS) {                                                                                                            \
      const int kc = d - k0 < SIM_K ? d - k0 : SIM_K;                                                                                \
      for (int k = 0; k < kc; ++k) t = __builtin_fmaf((As)[tid * SIM_LD + k], (Bs)[tid * SIM_LD + k], t);                            \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
  }

// ---- host side ----
// The workgroups per row block that share its column tiles: ceil of the target over the row blocks, then the two caps (`cap`: the
// grid's y limit, or what the caller's workspace allows).
static inline long long sim_split(long long row_blocks, long long col_tiles, long long cap) {
  long long split = (SIM_TARGET_WGS + row_blocks - 1) / row_blocks;
  if (split > col_tiles) split = col_tiles;
  if (split > cap) split = cap;
  return split < 1 ? 1 : split;
}

}  // namespace octmae
