// Both directions of up to three square retrieval problems from ONE walk over the tiles of each product (the six directions of
// train_retclip_3modalities.py:561-604, get_metrics_3modalities, are three products read by row and by column; six launches of
// octmae_retrieval_ranks compute every product twice).
//   octmae_retrieval_pair_ranks   P pairs (1 .. 3) of a_p, b_p f32 [n][d] (row strides >= d)  ->  out int32 [P][2][n][2]
//     s_p(i, j) = the f32 chain of csrc/simtile.hpp, t_p(i) = s_p(i, i)
//     out[p][0][i] = { #{j != i: s_p(i, j) > t_p(i)},  #{j < i: s_p(i, j) == t_p(i)} }      rows:    retrieval_ranks(a_p, b_p)[:, :2]
//     out[p][1][j] = { #{i != j: s_p(i, j) > t_p(j)},  #{i < j: s_p(i, j) == t_p(j)} }      columns: retrieval_ranks(b_p, a_p)[:, :2]
// s_p(i, j) is the same fmaf chain whichever operand is called a (a product of two floats commutes), so the column direction holds the
// bits the second launch would have formed, and the counts are equal -- not close -- to the two launches'.
//
// The tile is csrc/simtile.hpp's.  A pre-pass writes t_p(i) to the workspace with the VALU chain (the header: the same bits as the
// tile's entry).  The main walk keeps a lane's two row counters in registers across the column loop as retrieval.hip does; for the
// column direction the same accumulator register is compared with t_p(j): the 32 rows of a column sit across the 32 lanes of a
// half-wave, so one ballot per register and predicate and a popcount of each half count them.  The two row-waves of a column leave
// their counts in LDS and one thread per (column, counter) adds the sum into `out` -- one integer atomicAdd per column, counter and
// tile (cdna_hip_programming.md, guideline 12: reduce before the atomic).  The row blocks of a column and, for small n, the column
// tiles of a row block are different workgroups (gridDim.y of them per row block, sim_split): integer atomicAdd into the zeroed `out`,
// order-free, so the result is deterministic.  No float crosses a workgroup except the read-only t_p.
//   work: 2 P n^2 d flop on the matrix cores, half of what six per-direction launches do.  No 16-bit operand: the two builds of the
//   library hold the same code.  No fast-math flag on this file.
#include <cstdint>
#include "common.hpp"
#include "simtile.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int RP_MAX_PAIRS = 3;

struct RpOperands {                     // by value in the kernel arguments; pair p is chosen with selects, never by indexing
  const float* a0; const float* b0; const float* a1; const float* b1; const float* a2; const float* b2;
  long long as0, bs0, as1, bs1, as2, bs2;
};

#define RP_PICK(o, p, f) ((p) == 0 ? (o).f##0 : (p) == 1 ? (o).f##1 : (o).f##2)

// diag[p][i] = s_p(i, i): 64 rows per workgroup, grid (row blocks, P)
__global__ __launch_bounds__(SIM_THREADS) void retrieval_pair_diag_kernel(RpOperands o, float* __restrict__ diag, long long n, int d) {
  __shared__ float As[SIM_ROWS * SIM_LD];
  __shared__ float Bs[SIM_COLS * SIM_LD];
  const int tid = (int)threadIdx.x, p = (int)blockIdx.y;
  const float* __restrict__ a = RP_PICK(o, p, a);
  const float* __restrict__ b = RP_PICK(o, p, b);
  const long long as = RP_PICK(o, p, as), bs = RP_PICK(o, p, bs);
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;
  auto row = [&](int rr) -> long long { return i0 + rr < n ? i0 + rr : -1; };
  float t = 0.0f;
  SIM_TARGET_CHAIN(t, As, Bs, a, as, row, b, bs, row);
  if (tid < SIM_ROWS && i0 + tid < n) diag[(long long)p * n + i0 + tid] = t;
}

// grid (row blocks, split, P)
__global__ __launch_bounds__(SIM_THREADS) void retrieval_pair_ranks_kernel(RpOperands o, const float* __restrict__ diag,
                                                                         int* __restrict__ out, long long n, int d, int col_tiles) {
  __shared__ float As[SIM_ROWS * SIM_LD];
  __shared__ float Bs[SIM_COLS * SIM_LD];
  __shared__ float ts[SIM_ROWS];          // t(i) of the row block, 0 past n
  __shared__ float tcs[SIM_COLS];         // t(j) of the column tile, 0 past n
  __shared__ int cc[2][SIM_COLS][2];      // [row-wave][column][greater, equal-and-before]: a tile's column counts
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const int p = (int)blockIdx.z;
  const float* __restrict__ a = RP_PICK(o, p, a);
  const float* __restrict__ b = RP_PICK(o, p, b);
  const long long as = RP_PICK(o, p, as), bs = RP_PICK(o, p, bs);
  const float* __restrict__ tp = diag + (long long)p * n;
  int* __restrict__ out_row = out + (long long)p * 4 * n;      // out[p][0]
  int* __restrict__ out_col = out_row + 2 * n;                 // out[p][1]
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;

  if (tid < SIM_ROWS) ts[tid] = i0 + tid < n ? tp[i0 + tid] : 0.0f;
  __syncthreads();
  auto a_row = [&](int rr) -> long long { return i0 + rr < n ? i0 + rr : -1; };

  const int il = wr * 32 + r;                   // this lane's row of the block (both half-waves: they split its columns)
  const long long i = i0 + il;
  const bool row_in = i < n;
  const float ti = ts[il];
  int c0 = 0, c1 = 0;

  for (int ct = (int)blockIdx.y; ct < col_tiles; ct += (int)gridDim.y) {
    const long long j0 = (long long)ct * SIM_COLS;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    if (tid < SIM_COLS) tcs[tid] = j0 + tid < n ? tp[j0 + tid] : 0.0f;
    auto b_row = [&](int cc_) -> long long { return j0 + cc_ < n ? j0 + cc_ : -1; };
    SIM_SCORE_TILE(acc, As, Bs, a, as, a_row, b, bs, b_row);
    int kg = 0, ke = 0;                         // lane r < 16 of half h keeps the counts of column SIM_COL(wc * 32, r, h)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int jl = SIM_COL(wc * 32, g, h);
      const long long j = j0 + jl;
      const float s = acc[g];
      const bool in = row_in && j < n;          // both indices inside: an LDS image past the end is zero, not a score
      c0 += (in && j != i && s > ti) ? 1 : 0;
      c1 += (in && j < i && s == ti) ? 1 : 0;
      const float tj = tcs[jl];
      // a column's 32 rows are the 32 lanes of this half-wave: bits 0 .. 31 belong to h = 0's column, bits 32 .. 63 to h = 1's
      const unsigned long long mg = __ballot(in && i != j && s > tj);
      const unsigned long long me = __ballot(in && i < j && s == tj);
      const int ng = h ? __popc((unsigned)(mg >> 32)) : __popc((unsigned)mg);
      const int ne = h ? __popc((unsigned)(me >> 32)) : __popc((unsigned)me);
      if (r == g) {
        kg = ng;
        ke = ne;
      }
    }
    if (r < 16) {
      const int jl = SIM_COL(wc * 32, r, h);
      cc[wr][jl][0] = kg;
      cc[wr][jl][1] = ke;
    }
    __syncthreads();
    if (tid < 2 * SIM_COLS) {                   // the two row-waves of a column, then one atomic per (column, counter)
      const int jl = tid >> 1, k = tid & 1;
      const int v = cc[0][jl][k] + cc[1][jl][k];
      if (v && j0 + jl < n) atomicAdd(out_col + (j0 + jl) * 2 + k, v);
    }
    // the next tile rewrites tcs after this barrier and cc after the two barriers of its first k step
  }
  // the two half-waves hold the two halves of a row's columns
  c0 += __shfl_xor(c0, 32, 64);
  c1 += __shfl_xor(c1, 32, 64);
  if (h == 0 && row_in) {
    if (c0) atomicAdd(out_row + i * 2 + 0, c0);
    if (c1) atomicAdd(out_row + i * 2 + 1, c1);
  }
}

static inline bool rp_shape_ok(long long n, int pairs) {
  return n > 0 && n <= 0x7fffffffLL && pairs >= 1 && pairs <= RP_MAX_PAIRS;    // a count can reach n
}

}  // namespace octmae
using namespace octmae;

extern "C" long long int octmae_retrieval_pair_ws(long long n, int pairs) {
  if (!rp_shape_ok(n, pairs)) return -1;
  return (long long)pairs * n * (long long)sizeof(float);
}

extern "C" int octmae_retrieval_pair_ranks(const float* a0, long long a0_stride, const float* b0, long long b0_stride, const float* a1,
                                           long long a1_stride, const float* b1, long long b1_stride, const float* a2,
                                           long long a2_stride, const float* b2, long long b2_stride, int pairs, int* out, void* ws,
                                           long long ws_bytes, long long n, int d, void* stream) {
  if (!rp_shape_ok(n, pairs) || d <= 0 || !out || !ws) return -1;
  if (ws_bytes < octmae_retrieval_pair_ws(n, pairs) || (reinterpret_cast<uintptr_t>(ws) & 3) != 0) return -1;
  const float* as_[RP_MAX_PAIRS] = {a0, a1, a2};
  const float* bs_[RP_MAX_PAIRS] = {b0, b1, b2};
  const long long sa[RP_MAX_PAIRS] = {a0_stride, a1_stride, a2_stride}, sb[RP_MAX_PAIRS] = {b0_stride, b1_stride, b2_stride};
  for (int p = 0; p < pairs; ++p)
    if (!as_[p] || !bs_[p] || sa[p] < d || sb[p] < d) return -1;
  RpOperands o{};
  o.a0 = a0; o.b0 = b0; o.as0 = a0_stride; o.bs0 = b0_stride;
  if (pairs > 1) { o.a1 = a1; o.b1 = b1; o.as1 = a1_stride; o.bs1 = b1_stride; }
  if (pairs > 2) { o.a2 = a2; o.b2 = b2; o.as2 = a2_stride; o.bs2 = b2_stride; }
  const long long row_blocks = (n + SIM_ROWS - 1) / SIM_ROWS;     // <= 2^25: the grid's x
  const int col_tiles = (int)row_blocks;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, (size_t)pairs * 4 * (size_t)n * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  float* diag = static_cast<float*>(ws);
  hipLaunchKernelGGL(retrieval_pair_diag_kernel, dim3((unsigned)row_blocks, (unsigned)pairs), dim3(SIM_THREADS), 0, st, o, diag, n, d);
  OCTMAE_LAUNCH_CHECK();
  const long long split = sim_split(row_blocks * pairs, col_tiles, 65535);   // the grid's y; the pairs are the grid's z
  hipLaunchKernelGGL(retrieval_pair_ranks_kernel, dim3((unsigned)row_blocks, (unsigned)split, (unsigned)pairs), dim3(SIM_THREADS), 0, st, o,
                     diag, out, n, d, col_tiles);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
