// Retrieval ranks of the COEM validation (retinal-COEM/src/training/train_retclip.py:409-469: get_metrics, get_corrected_metrics, and
// get_metrics_3modalities of train_retclip_3modalities.py).  The reference forms the [n][m] logit matrix on the CPU and sorts every row
// twice; every metric it reports is a function of a few integers per row, so this kernel counts them off the tiles of a . b^T and never
// stores a score.
//   octmae_retrieval_ranks   a f32 [n][d], b f32 [m][d] (row strides >= d)  ->  out int32 [n][4]
//     s(i, j) = the f32 chain acc = 0; for k = 0 .. d-1: acc = fmaf(a[i][k], b[j][k], acc); t_i = s(i, target[i])
//     out[i] = { #{j kept, j != target[i]: s > t_i},  #{j kept, j < target[i]: s == t_i},
//                #{j: col_group[j] == row_group[i], s >= 0},  #{j: col_group[j] == row_group[i]} }
//     out[i][0] + out[i][1] is the target's position under a STABLE descending sort (ties by column index).
// Scores come from v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, bit for bit the k-ordered fmaf chain above with one rounding per
// product and no wider accumulation -- deterministic, symmetric in its operands (s(i, j) of (a, b) is s(j, i) of (b, a)), and what a
// plain VALU fmaf chain yields, which is how t_i is made: the workgroup stages its 64 rows of a beside the 64 TARGET rows of b through
// the same LDS tiles and 64 threads run the chain.  A bit copy of the target row elsewhere in b therefore ties exactly.
//
// The tile is csrc/simtile.hpp's, which retrieval_topk.hip and cliploss.hip walk too: one workgroup of 256 threads (2 x 2 waves) owns
// SIM_ROWS = 64 rows of a and walks column tiles of SIM_COLS = 64 rows of b; per tile it walks d in LDS steps of SIM_K = 32 (two
// [64][33] f32 images, 16.5 KiB: eight workgroups per CU).  A wave holds one 32 x 32 accumulator,
// TRANSPOSED: b is the MFMA's A operand and a its B operand, so a lane's 16 registers are 16 columns j of ONE row i and the four counters
// of that row live in four registers across the whole column loop.  Tails are masked by index: a row past n or a column past m takes no
// part in any count (its LDS image is zero, not a sentinel score -- any f32 is a legal score), and the k loop ends at d (an odd d runs
// its last step with one zero operand pair: fmaf(0, 0, acc) == acc under IEEE comparison).
// Small n: the column tiles are dealt round-robin to gridDim.y workgroups per row block, each adds its partial counts into the zeroed
// `out` with integer atomicAdd -- order-free, so the result stays deterministic; no float crosses a workgroup.
//   work: 2 n m d flop on the matrix cores (64 flop / clk / SIMD); the [n][m] matrix never exists.  No 16-bit operand: the two builds
//   of the library hold the same code.  No fast-math flag on this file.
#include <cstdint>
#include "common.hpp"
#include "simtile.hpp"
#include "../../include/octmae.h"

namespace octmae {

// out[0] = 1 where a target is no column of b or is not kept (the entry point reads it back before the main launch)
__global__ __launch_bounds__(SIM_THREADS) void retrieval_check_kernel(const int* __restrict__ target, const uint8_t* __restrict__ keep,
                                                                    long long n, int m, int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= n) return;
  const long long t = target ? (long long)target[i] : i;
  if (t < 0 || t >= m || (keep && keep[t] == 0)) *flag = 1;
}

__global__ __launch_bounds__(SIM_THREADS) void retrieval_ranks_kernel(const float* __restrict__ a, long long as,
                                                                    const float* __restrict__ b, long long bs,
                                                                    const int* __restrict__ target, const uint8_t* __restrict__ keep,
                                                                    const int* __restrict__ row_group, const int* __restrict__ col_group,
                                                                    int* __restrict__ out, long long n, int m, int d, int col_tiles) {
  __shared__ float As[SIM_ROWS * SIM_LD];
  __shared__ float Bs[SIM_COLS * SIM_LD];
  __shared__ float ts[SIM_ROWS];      // t_i
  __shared__ int tg[SIM_ROWS];        // target[i], -1 past n
  __shared__ int cgs[SIM_COLS];       // col_group[j]
  __shared__ int flg[SIM_COLS];       // bit 0: j takes part in the ranking, bit 1: j < m
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;
  const bool grouped = row_group != nullptr;

  if (tid < SIM_ROWS) {
    const long long i = i0 + tid;
    tg[tid] = i < n ? (target ? target[i] : (int)i) : -1;
  }
  __syncthreads();
  auto a_row = [&](int rr) -> long long { return i0 + rr < n ? i0 + rr : -1; };

  // ---- t_i: the same chain on the VALU, a rows against their target rows of b
  {
    float t = 0.0f;
    auto t_row = [&](int rr) -> long long { return (long long)tg[rr]; };
    SIM_TARGET_CHAIN(t, As, Bs, a, as, a_row, b, bs, t_row);
    if (tid < SIM_ROWS) ts[tid] = t;
  }
  __syncthreads();

  const int il = wr * 32 + r;                   // this lane's row of the block (both half-waves: they split its columns)
  const long long i = i0 + il;
  const float ti = ts[il];
  const int tgt = tg[il];
  const int rg = grouped && i < n ? row_group[i] : 0;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;

  for (int ct = (int)blockIdx.y; ct < col_tiles; ct += (int)gridDim.y) {
    const long long j0 = (long long)ct * SIM_COLS;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    if (tid < SIM_COLS) {
      const long long j = j0 + tid;
      const bool in = j < m;
      flg[tid] = in ? (2 | ((keep == nullptr || keep[j] != 0) ? 1 : 0)) : 0;
      cgs[tid] = in && grouped ? col_group[j] : 0;
    }
    auto b_row = [&](int cc) -> long long { return j0 + cc < m ? j0 + cc : -1; };
    SIM_SCORE_TILE(acc, As, Bs, a, as, a_row, b, bs, b_row);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int jl = SIM_COL(wc * 32, g, h);
      const int f = flg[jl];
      const long long j = j0 + jl;
      const float s = acc[g];
      const bool kept = (f & 1) != 0;
      c0 += (kept && j != tgt && s > ti) ? 1 : 0;
      c1 += (kept && j < tgt && s == ti) ? 1 : 0;
      if (grouped) {
        const bool same = (f & 2) != 0 && cgs[jl] == rg;
        c2 += (same && s >= 0.0f) ? 1 : 0;
        c3 += same ? 1 : 0;
      }
    }
    __syncthreads();                                          // the next tile rewrites flg / cgs
  }
  // the two half-waves hold the two halves of a row's columns
  c0 += __shfl_xor(c0, 32, 64);
  c1 += __shfl_xor(c1, 32, 64);
  c2 += __shfl_xor(c2, 32, 64);
  c3 += __shfl_xor(c3, 32, 64);
  if (h == 0 && i < n) {
    int* o = out + i * 4;
    if (c0) atomicAdd(o + 0, c0);
    if (c1) atomicAdd(o + 1, c1);
    if (c2) atomicAdd(o + 2, c2);
    if (c3) atomicAdd(o + 3, c3);
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_retrieval_ranks(const float* a, long long a_stride, const float* b, long long b_stride, const int* target,
                                      const uint8_t* keep, const int* row_group, const int* col_group, int* out, long long n,
                                      long long m, int d, void* stream) {
  if (!a || !b || !out) return -2;
  if (n <= 0 || m <= 0 || d <= 0 || a_stride < d || b_stride < d) return -2;
  if (m > 0x7fffffffLL) return -2;                        // a count can reach m; target holds int column indices
  if (!target && n != m) return -2;
  if ((row_group == nullptr) != (col_group == nullptr)) return -2;
  const long long row_blocks = (n + SIM_ROWS - 1) / SIM_ROWS;
  if (row_blocks > 0x7fffffffLL) return -2;               // the row block is the grid's x
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 4 * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  if (target || keep) {
    // every target must be a kept column of b (an index past m would also be read as a row of b): one flag through out[0]
    hipLaunchKernelGGL(retrieval_check_kernel, dim3((unsigned)((n + SIM_THREADS - 1) / SIM_THREADS)), dim3(SIM_THREADS), 0, st, target, keep,
                       n, (int)m, out);
    OCTMAE_LAUNCH_CHECK();
    int bad = 0;
    e = hipMemcpyAsync(&bad, out, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (bad) {
      e = hipMemsetAsync(out, 0, sizeof(int), st);
      return e != hipSuccess ? (int)e : -2;
    }
  }
  const int col_tiles = (int)((m + SIM_COLS - 1) / SIM_COLS);
  const long long split = sim_split(row_blocks, col_tiles, 65535);   // the grid's y
  hipLaunchKernelGGL(retrieval_ranks_kernel, dim3((unsigned)row_blocks, (unsigned)split), dim3(SIM_THREADS), 0, st, a, a_stride, b, b_stride,
                     target, keep, row_group, col_group, out, n, (int)m, d, col_tiles);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
