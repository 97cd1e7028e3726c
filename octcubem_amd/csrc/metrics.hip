// Rank counts for the ranking metrics of the fine-tune evaluation (OCTCube/engine_finetune.py:251-343, :786-792: roc_auc_score,
// average_precision_score, precision_recall_curve + auc, all of scikit-learn).  Every one of them is a function of four integers per
// sample and class, so the device counts and the host finishes in float64 (octcubem_amd/metrics.py): no sort, no float accumulation,
// the same counts whatever the launch order.
//   octmae_rank_counts   scores f32 [n][C] (row stride >= C) + labels uint8 [n][C] (own row stride)  ->  counts int32 [n][C][4]
//                        {gt_all, gt_pos, ge_all, ge_pos}: the samples j of class c with s[j] > s[i] / s[j] >= s[i], and how many of
//                        them carry a label != 0.  IEEE comparisons: -0.0 ties with 0.0, +-inf are ordinary values; a NaN compares
//                        false with everything (octcubem_amd/ops.py refuses NaN scores before the launch).
//   octmae_rank_counts_masked   the same over a per-column population: + valid uint8 [n][C] (own row stride).  Column c ranks the
//                        samples with valid[j][c] != 0 among themselves (OCTCube/engine_finetune.py:130-139: every task of the
//                        multi-task evaluation keeps the samples that carry the normal label or its own); a sample outside the
//                        population counts for nobody and its own four counts are written as zeros.
// One workgroup of 256 threads owns 256 values of i of one class and streams all j through LDS in tiles of 1024 (score and flags
// together, 5 KiB); every thread of a wave reads the same LDS address at the same time (a broadcast, no bank conflict), four scores per
// ds_read_b128 and their four flag bytes in one dword.  The four counters stay in registers.  The tails are MASKED -- the j loop ends
// at the tile's count and a thread past n stores nothing -- never padded with a sentinel score, because +inf and -inf are legal inputs.
// The masked form is the same template: the flag byte of j holds label & valid in bit 0 and valid in bit 1, and valid takes the place
// of the constant 1 that a true comparison selects: a pair costs the same two compares and four adds, plus the extraction of the
// valid bit and one more and per counter.  The unmasked instantiation compiles to the instruction sequence it had before the
// template (compared in the ISA): no extra load, compare or select.
//   work: n * n * C comparisons pairs, 2 compares + 4 integer adds each; O(n^2 C) on purpose (tools/bench_metrics.py measures it
//   against a sort composed from ATen ops).  No 16-bit operand: the two builds of the library hold the same code.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int RC_BLOCK = 256;   // values of i per workgroup
constexpr int RC_TILE = 1024;   // values of j per LDS tile (a multiple of RC_BLOCK and of 4)

// vj: 1 for a j that takes part, 0 otherwise (the constant 1 without a mask); lj: its label, already 0 where vj is 0
__device__ __forceinline__ void rc_count(float sj, unsigned lj, unsigned vj, float si, int& gt_all, int& gt_pos, int& ge_all, int& ge_pos) {
  const unsigned gt = sj > si ? vj : 0u, ge = sj >= si ? vj : 0u;
  gt_all += (int)gt;
  gt_pos += (int)(gt & lj);
  ge_all += (int)ge;
  ge_pos += (int)(ge & lj);
}

template <bool MASKED>
__global__ __launch_bounds__(RC_BLOCK) void rank_counts_kernel(const float* __restrict__ scores, long long ss,
                                                              const uint8_t* __restrict__ labels, long long ls,
                                                              const uint8_t* __restrict__ valid, long long vs,
                                                              int* __restrict__ counts, int n, int C) {
  __shared__ __attribute__((aligned(16))) float ts[RC_TILE];
  __shared__ __attribute__((aligned(16))) uint8_t tl[RC_TILE];     // bit 0: label (& valid), bit 1: valid (MASKED only)
  const int c = blockIdx.y;
  const long long i = (long long)blockIdx.x * RC_BLOCK + threadIdx.x;
  const bool live = i < n;
  const float si = live ? scores[i * ss + c] : 0.0f;
  bool vi = true;
  if constexpr (MASKED) vi = live && valid[i * vs + c] != 0;
  int gt_all = 0, gt_pos = 0, ge_all = 0, ge_pos = 0;
  for (long long j0 = 0; j0 < n; j0 += RC_TILE) {
    const int cnt = (int)(n - j0 < RC_TILE ? n - j0 : RC_TILE);
#pragma unroll
    for (int k = 0; k < RC_TILE / RC_BLOCK; ++k) {
      const int t = k * RC_BLOCK + (int)threadIdx.x;
      if (t < cnt) {                                   // the tile's tail is left unwritten and is never read
        ts[t] = scores[(j0 + t) * ss + c];
        const uint8_t l = labels[(j0 + t) * ls + c] != 0 ? 1 : 0;
        if constexpr (MASKED) tl[t] = valid[(j0 + t) * vs + c] != 0 ? (uint8_t)(2 | l) : (uint8_t)0;
        else tl[t] = l;
      }
    }
    __syncthreads();
    const int full = cnt & ~3;
    for (int t = 0; t < full; t += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&ts[t]);
      const unsigned l4 = *reinterpret_cast<const unsigned*>(&tl[t]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        rc_count(v[k], (l4 >> (8 * k)) & 1u, MASKED ? (l4 >> (8 * k + 1)) & 1u : 1u, si, gt_all, gt_pos, ge_all, ge_pos);
    }
    for (int t = full; t < cnt; ++t) rc_count(ts[t], tl[t] & 1u, MASKED ? (tl[t] >> 1) & 1u : 1u, si, gt_all, gt_pos, ge_all, ge_pos);
    __syncthreads();                                   // the next tile overwrites ts / tl
  }
  if (live) {
    int* o = counts + ((size_t)i * C + c) * 4;
    if (MASKED && !vi) gt_all = gt_pos = ge_all = ge_pos = 0;      // outside the population: defined zeros, not leftover bytes
    o[0] = gt_all; o[1] = gt_pos; o[2] = ge_all; o[3] = ge_pos;
  }
}

}  // namespace octmae
using namespace octmae;

static int rc_launch(const float* scores, long long score_stride, const uint8_t* labels, long long label_stride, const uint8_t* valid,
                     long long valid_stride, bool masked, int* counts, long long n, int C, void* stream) {
  if (!scores || !labels || !counts || (masked && !valid)) return -2;
  if (n <= 0 || C <= 0 || score_stride < C || label_stride < C || (masked && valid_stride < C)) return -2;
  if (n > 0x7fffffffLL) return -2;      // a count can reach n
  if (C > 65535) return -2;             // the class is the grid's y
  const long long blocks = (n + RC_BLOCK - 1) / RC_BLOCK;
  const dim3 grid((unsigned)blocks, (unsigned)C);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (masked)
    hipLaunchKernelGGL(rank_counts_kernel<true>, grid, dim3(RC_BLOCK), 0, st, scores, score_stride, labels, label_stride, valid,
                       valid_stride, counts, (int)n, C);
  else
    hipLaunchKernelGGL(rank_counts_kernel<false>, grid, dim3(RC_BLOCK), 0, st, scores, score_stride, labels, label_stride,
                       (const uint8_t*)nullptr, 0LL, counts, (int)n, C);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_rank_counts(const float* scores, long long score_stride, const uint8_t* labels, long long label_stride,
                                  int* counts, long long n, int C, void* stream) {
  return rc_launch(scores, score_stride, labels, label_stride, nullptr, 0, false, counts, n, C, stream);
}

extern "C" int octmae_rank_counts_masked(const float* scores, long long score_stride, const uint8_t* labels, long long label_stride,
                                         const uint8_t* valid, long long valid_stride, int* counts, long long n, int C, void* stream) {
  return rc_launch(scores, score_stride, labels, label_stride, valid, valid_stride, true, counts, n, C, stream);
}
