// Top-k cross-modal retrieval (retinal-COEM/src/retDisease_eval/evaluate_results_test_train_visualize_all_models_top3_col_aireadi_
// laterality.py:186-270): the reference forms logit_scale * image @ text^T on the CPU, masks the query's own patient and takes
// torch.topk.  This kernel walks the same product on the tiles of octmae_retrieval_ranks (csrc/retrieval.hip) and keeps, per row, the
// k best candidates in LDS; a score leaves the chip only as one of those k.
//   octmae_retrieval_topk   a f32 [n][d], b f32 [m][d] (row strides >= d)  ->  out_idx int32 [n][k], out_score f32 [n][k]
//     s(i, j) = the f32 chain acc = 0; for kk = 0 .. d-1: acc = fmaf(a[i][kk], b[j][kk], acc)   (v_mfma_f32_32x32x2_f32, as the ranks)
//     j is a candidate of row i iff j < m, keep[j] != 0 (keep given), col_group[j] != row_group[i] (groups given), s(i, j) is no NaN
//     (s1, j1) comes before (s2, j2) iff s1 > s2 || (s1 == s2 && j1 < j2): IEEE comparisons, a STRICT order on the candidates of a row
//     out[i][0 .. k) = the first k candidates in that order; a row with c < k candidates has idx -1, score -inf in slots c .. k-1
//
// The walk is retrieval_ranks_kernel's, from the same header (csrc/simtile.hpp): 256 threads as 2 x 2 waves, SIM_ROWS = 64 rows of a
// per workgroup, column tiles of SIM_COLS = 64 rows of b, d in LDS steps of SIM_K = 32, the accumulator transposed so that a lane
// holds 16 columns of one row; tails are masked by index, an odd d ends on a zero operand pair.
// Selection: per row a sorted list of k (score, index) pairs in LDS (pitch RT_KMAX + 1: the 32 rows a half-wave touches at one
// position land on 32 banks).  After a tile's k loop every lane tests its 16 scores against the row's k-th entry and sets one bit
// per passing column in the row's 64-bit mask (an integer OR in LDS), and the tile is spilled to a [64][65] LDS image that ALIASES the
// two operand images (4160 of their 4224 floats; a barrier on each side).  Then 64 threads take one row each and insert the columns
// whose bits are set serially, in ascending column order -- most rows have none once their list is full.  A workgroup walks its tiles
// in ascending order, so a new index is above every index of its list: a score equal to an entry goes behind it, and a full list
// admits s only where s > its last score.
// Small n: the column tiles are dealt round-robin to gridDim.y = split workgroups per row block.  With split == 1 the lists go
// straight to out_*; otherwise to ws as [split][n][k] (score, index) pairs, and retrieval_topk_merge_kernel -- one wave per row --
// folds them in ascending split order: 32 lanes hold the current list, 32 the next partial list, every entry finds its place as its
// own position plus the entries of the other list that come before it (the order is strict and the lists share no column, so the
// places are distinct), and the first k are kept.  The one atomic is the integer OR of the masks; no float crosses a workgroup except
// through that ordered merge: the result does not depend on which workgroup saw which tile, and two launches give the same bits.
//   work: 2 n m d flop on the matrix cores; nothing of size n m exists anywhere.  No 16-bit operand: the two builds of the library
//   hold the same code.  No fast-math flag on this file.
#include <cstdint>
#include "common.hpp"
#include "simtile.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int RT_KMAX = 32;        // the largest k: one list entry per lane of a half-wave in the merge
constexpr int RT_LP = RT_KMAX + 1; // list pitch
constexpr int RT_SP = SIM_COLS + 1; // pitch of the spilled score tile
constexpr int RT_MERGE_THREADS = 64;
static_assert(SIM_ROWS * RT_SP <= (SIM_ROWS + SIM_COLS) * SIM_LD, "the spilled tile fits the two operand images it aliases");
static_assert(2 * RT_KMAX == RT_MERGE_THREADS, "the merge holds two lists of RT_KMAX, one entry per lane");

struct RtPair {
  float s;
  int j;
};
static_assert(sizeof(RtPair) == 8, "ws holds [split][n][k] pairs of 8 bytes");

// (s1, j1) before (s2, j2): the strict order of the contract
__device__ __forceinline__ bool rt_before(float s1, int j1, float s2, int j2) { return s1 > s2 || (s1 == s2 && j1 < j2); }

// pairs == nullptr: the lists are final and go to out_idx / out_score; otherwise list y of row i goes to pairs[(y n + i) k ..]
__global__ __launch_bounds__(SIM_THREADS) void retrieval_topk_kernel(const float* __restrict__ a, long long as,
                                                                   const float* __restrict__ b, long long bs,
                                                                   const uint8_t* __restrict__ keep, const int* __restrict__ row_group,
                                                                   const int* __restrict__ col_group, int kk, int* __restrict__ out_idx,
                                                                   float* __restrict__ out_score, RtPair* __restrict__ pairs, long long n,
                                                                   int m, int d, int col_tiles) {
  __shared__ float ops[(SIM_ROWS + SIM_COLS) * SIM_LD];   // the operand images; between two barriers the spilled score tile [64][RT_SP]
  __shared__ float ls[SIM_ROWS * RT_LP];                // the lists: scores, descending
  __shared__ int lj[SIM_ROWS * RT_LP];                  //            and their columns
  __shared__ int cnt[SIM_ROWS];                         // filled entries of a list
  __shared__ unsigned pass[SIM_ROWS * 2];               // the columns of this tile that passed the row's prefilter, one bit each
  __shared__ int rgs[SIM_ROWS];                         // row_group[i]
  __shared__ int cgs[SIM_COLS];                         // col_group[j]
  __shared__ int flg[SIM_COLS];                         // 1: j < m and kept
  float* As = ops;
  float* Bs = ops + SIM_ROWS * SIM_LD;
  float* St = ops;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave & 1, wc = wave >> 1, r = lane & 31, h = lane >> 5;
  const long long i0 = (long long)blockIdx.x * SIM_ROWS;
  const bool grouped = row_group != nullptr;

  if (tid < SIM_ROWS) {
    const long long i = i0 + tid;
    cnt[tid] = 0;
    pass[2 * tid] = pass[2 * tid + 1] = 0u;
    rgs[tid] = grouped && i < n ? row_group[i] : 0;
    for (int p = 0; p < RT_LP; ++p) {
      ls[tid * RT_LP + p] = -__builtin_inff();
      lj[tid * RT_LP + p] = -1;
    }
  }
  __syncthreads();
  auto a_row = [&](int rr) -> long long { return i0 + rr < n ? i0 + rr : -1; };
  const int il = wr * 32 + r;                   // this lane's row of the block (both half-waves: they split its columns)
  const int rg = rgs[il];

  for (int ct = (int)blockIdx.y; ct < col_tiles; ct += (int)gridDim.y) {
    const long long j0 = (long long)ct * SIM_COLS;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    if (tid < SIM_COLS) {
      const long long j = j0 + tid;
      const bool in = j < m;
      flg[tid] = in && (keep == nullptr || keep[j] != 0) ? 1 : 0;
      cgs[tid] = in && grouped ? col_group[j] : 0;
    }
    auto b_row = [&](int cc) -> long long { return j0 + cc < m ? j0 + cc : -1; };
    SIM_SCORE_TILE(acc, As, Bs, a, as, a_row, b, bs, b_row);
    // Prefilter against the row's k-th entry, spill the tile.
    {
      const bool full = cnt[il] == kk;
      const float thr = ls[il * RT_LP + kk - 1];
      unsigned bits = 0u;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int cl = SIM_COL(0, g, h);                      // the column within this wave's 32
        const int jl = wc * 32 + cl;
        const float s = acc[g];
        if (flg[jl] != 0 && (!grouped || cgs[jl] != rg) && s == s && (!full || s > thr)) bits |= 1u << cl;
        St[il * RT_SP + jl] = s;
      }
      if (bits != 0u) atomicOr(&pass[2 * il + wc], bits);     // the two half-waves share the word; an integer OR is order-free
    }
    __syncthreads();
    if (tid < SIM_ROWS && i0 + tid < n && (pass[2 * tid] | pass[2 * tid + 1]) != 0u) {
      float* S = &ls[tid * RT_LP];
      int* J = &lj[tid * RT_LP];
      int c = cnt[tid];
      unsigned long long todo = ((unsigned long long)pass[2 * tid + 1] << 32) | pass[2 * tid];
      while (todo != 0ull) {                                  // the survivors in ascending column order
        const int jl = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const float s = St[tid * RT_SP + jl];
        if (c == kk && !(s > S[kk - 1])) continue;             // the list has moved on since the prefilter
        int p = c < kk ? c : kk - 1;                          // the slot that opens: behind the list, or its last entry drops out
        while (p > 0 && S[p - 1] < s) {                       // an equal score stays in front: its column is lower
          S[p] = S[p - 1];
          J[p] = J[p - 1];
          --p;
        }
        S[p] = s;
        J[p] = (int)(j0 + jl);
        if (c < kk) ++c;
      }
      cnt[tid] = c;
    }
    if (tid < SIM_ROWS) pass[2 * tid] = pass[2 * tid + 1] = 0u;
    __syncthreads();                                          // the next tile rewrites flg / cgs and the operand images under St
  }
  if (tid < SIM_ROWS && i0 + tid < n) {
    const long long i = i0 + tid;
    const int c = cnt[tid];
    if (pairs == nullptr) {
      for (int p = 0; p < kk; ++p) {
        out_idx[i * kk + p] = p < c ? lj[tid * RT_LP + p] : -1;
        out_score[i * kk + p] = p < c ? ls[tid * RT_LP + p] : -__builtin_inff();
      }
    } else {
      RtPair* o = pairs + ((long long)blockIdx.y * n + i) * kk;
      for (int p = 0; p < kk; ++p) {
        RtPair e;
        e.s = p < c ? ls[tid * RT_LP + p] : -__builtin_inff();
        e.j = p < c ? lj[tid * RT_LP + p] : -1;
        o[p] = e;
      }
    }
  }
}

// one wave per row: fold the `split` partial lists of the row, each sorted and padded with (-inf, -1), into the first k of their union
__global__ __launch_bounds__(RT_MERGE_THREADS) void retrieval_topk_merge_kernel(const RtPair* __restrict__ pairs, int split, int kk,
                                                                               int* __restrict__ out_idx, float* __restrict__ out_score,
                                                                               long long n) {
  __shared__ float xs[2 * RT_KMAX];     // [0]: the current list, [1]: the next partial list
  __shared__ int xj[2 * RT_KMAX];
  __shared__ float ns[RT_KMAX];         // the merged list
  __shared__ int nj[RT_KMAX];
  const int lane = (int)threadIdx.x, half = lane >> 5, p = lane & 31;
  const long long i = blockIdx.x;
  const bool loads = half == 1 && p < kk;
  const float none_s = -__builtin_inff();
  const int none_j = -1;
  if (half == 0) {
    ns[p] = none_s;
    nj[p] = none_j;
  }
  float next_s = none_s;                                    // list y + 1 is in flight while list y is merged
  int next_j = none_j;
  if (loads) {
    next_s = pairs[i * kk + p].s;
    next_j = pairs[i * kk + p].j;
  }
  for (int y = 0; y < split; ++y) {
    if (half == 0) {                    // the merged list becomes the current one and empties (this lane alone touches ns[p] here)
      xs[p] = ns[p];
      xj[p] = nj[p];
      ns[p] = none_s;
      nj[p] = none_j;
    } else {
      xs[RT_KMAX + p] = next_s;
      xj[RT_KMAX + p] = next_j;
      if (loads && y + 1 < split) {
        const RtPair* e = pairs + ((long long)(y + 1) * n + i) * kk + p;
        next_s = e->s;
        next_j = e->j;
      }
    }
    __syncthreads();
    const float s = xs[lane];
    const int j = xj[lane];
    int place = p;                      // the entries of its own list in front of it: the filled entries are a prefix
    const int other = (1 - half) * RT_KMAX;
    for (int q = 0; q < kk; ++q) {
      const int oj = xj[other + q];
      place += (oj >= 0 && rt_before(xs[other + q], oj, s, j)) ? 1 : 0;
    }
    if (j >= 0 && place < kk) {
      ns[place] = s;
      nj[place] = j;
    }
    __syncthreads();
  }
  if (half == 0 && p < kk) {
    out_idx[i * kk + p] = nj[p];
    out_score[i * kk + p] = ns[p];
  }
}

static long long rt_split(long long n, long long m) {
  return sim_split((n + SIM_ROWS - 1) / SIM_ROWS, (m + SIM_COLS - 1) / SIM_COLS, 65535);   // the grid's y
}

}  // namespace octmae
using namespace octmae;

extern "C" long long octmae_retrieval_topk_ws(long long n, long long m, int k) {
  if (n <= 0 || m <= 0 || m > 0x7fffffffLL || k < 1 || k > RT_KMAX) return -2;
  const long long split = rt_split(n, m);
  return split > 1 ? split * n * k * (long long)sizeof(RtPair) : 0;
}

extern "C" int octmae_retrieval_topk(const float* a, long long a_stride, const float* b, long long b_stride, const uint8_t* keep,
                                     const int* row_group, const int* col_group, int k, int* out_idx, float* out_score, void* ws,
                                     long long ws_bytes, long long n, long long m, int d, void* stream) {
  if (!a || !b || !out_idx || !out_score) return -2;
  if (n <= 0 || m <= 0 || d <= 0 || a_stride < d || b_stride < d) return -2;
  if (k < 1 || k > RT_KMAX) return -2;
  if (m > 0x7fffffffLL) return -2;                        // out_idx holds int column indices
  if ((row_group == nullptr) != (col_group == nullptr)) return -2;
  const long long row_blocks = (n + SIM_ROWS - 1) / SIM_ROWS;
  if (row_blocks > 0x7fffffffLL) return -2;               // the row block is the grid's x
  const long long need = octmae_retrieval_topk_ws(n, m, k);
  if (need > 0 && (!ws || ws_bytes < need)) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int col_tiles = (int)((m + SIM_COLS - 1) / SIM_COLS);
  const long long split = rt_split(n, m);
  RtPair* pairs = split > 1 ? reinterpret_cast<RtPair*>(ws) : nullptr;
  hipLaunchKernelGGL(retrieval_topk_kernel, dim3((unsigned)row_blocks, (unsigned)split), dim3(SIM_THREADS), 0, st, a, a_stride, b, b_stride,
                     keep, row_group, col_group, k, out_idx, out_score, pairs, n, (int)m, d, col_tiles);
  OCTMAE_LAUNCH_CHECK();
  if (split > 1) {
    // split > 1 only below SIM_TARGET_WGS row blocks: n fits the grid's x
    hipLaunchKernelGGL(retrieval_topk_merge_kernel, dim3((unsigned)n), dim3(RT_MERGE_THREADS), 0, st, pairs, (int)split, k, out_idx,
                       out_score, n);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
