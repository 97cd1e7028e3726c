// Bootstrap resamples of the ranking metrics of the fine-tune evaluation (octcubem_amd/metrics.py: bootstrap_rank_metrics): AUROC,
// average precision, trapezoid AUPRC and the reference's best F1 of R resamples of one evaluation set, from ONE sort.
// A resample never moves a sample: it gives every resampling unit (a sample, or a patient with all its samples) a multiplicity, and
// every metric of octcubem_amd/metrics.py is a function of weighted cumulative counts along the descending score order.  The host
// (octcubem_amd/ops.py: bootstrap_rank_metrics) sorts each class column once and hands over, per class c and position p of that order,
//   unit_sorted int32 [C][n]   the resampling unit of the sample at p
//   flags       uint8 [C][n]   bit 0 label, bit 1 last position of a tie group (s[p] != s[p+1] or p == n - 1), bit 2 valid
//   mult        int32 [R][U]   how often unit u is drawn in resample r
// The weight of p in resample r is w = valid ? mult[r][unit] : 0.  Per (r, c), with TP / ALL the weighted cumulative positives / samples
// at a tie-group end g, posw_g / negw_g the group's own weights and FP_g = ALL_g - TP_g:
//   P, N     int64   weighted positives and negatives
//   U2       int64   sum_g posw_g (2 (N - FP_g) + negw_g): twice the Mann-Whitney statistic.  Accumulated as 2 N P - sum_g posw_g
//                    (2 FP_g - negw_g), the same integer, so that N is needed only once
//   ap_sum   f64     sum_g posw_g * (TP_g / ALL_g)                                   (average precision times P: the host divides)
//   auprc    f64     sum_g (posw_g / P) * (prec_g + prec_(g-1)) * 0.5, prec_g = TP_g / ALL_g, 1 where ALL_g == 0 and before the first
//                    group: the trapezoid rule over the points (TP_g / P, prec_g) from (0, 1)
//   max_f1   f64     max_g 2 p r / (p + r + 1e-8), p = prec_g, r = TP_g / P, and 0 (the start point)
// A group whose weight is zero in the resample repeats the previous point (zero width, the same F1), so nothing here asks whether a
// threshold is "distinct" in the resample.  P == 0 leaves the three floats 0; the host reports P == 0 or N == 0 as undefined.
//
// One workgroup of BS_BLOCK = 256 threads owns ONE resample (grid.x = R, no cap and no grid-stride loop) and loops over the classes, so
// the copy of mult[r] it stages in LDS is read C times over.  The row is staged when U <= BS_LDS_UNITS (48 KiB); a longer row is
// gathered from global memory (it is 4 U bytes per workgroup and stays in L2).  An id outside [0, U) weighs 0: the gather never
// leaves the row, whatever the caller passes.
// A class column is walked twice.  Pass 1 sums the weights: P and N (recall and the trapezoid's widths need P at every point).
// Pass 2 walks chunks of BS_CHUNK = 1024 positions, BS_ITEMS = 4 consecutive ones per thread.  Per chunk ONE block-wide inclusive scan of
// the packed pair (allw << 32 | posw) -- thread-local, then shuffles inside a wave, then the four wave totals through LDS -- and one
// block-wide "value at the latest tie-group end before me", which is a max-scan because the cumulative pair never decreases.  Both ride
// on one barrier: a wave publishes its total and its latest end RELATIVE to its own start, and every thread rebuilds the absolute
// values from the four pairs.  The running pair and the latest end are carried from chunk to chunk (the latest end may lie any number
// of chunks back: all scores tied is one group), the LDS slots alternate by chunk parity.  The four reductions (an int64 sum, two f64
// sums, one f64 max) stay in registers over all chunks and are folded once per column in a fixed order: the same bits every run.
// Running sums are 32-bit halves of one 64-bit word: the caller guarantees that the weights of a column sum to less than 2^31
// (ops.py checks largest cluster x largest row sum of mult) and that no multiplicity is negative.
//   work: 2 R C n gathered weights and flag bytes, R C n / 1024 barriers; no 16-bit operand: the two builds of the library hold the
//   same code.  Plain C++, vector stores only.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int BS_BLOCK = 256;          // threads per workgroup
constexpr int BS_ITEMS = 4;            // consecutive positions per thread and chunk
constexpr int BS_CHUNK = 1024;         // positions per chunk
constexpr int BS_WAVES = BS_BLOCK / 64;
constexpr int BS_LDS_UNITS = 12288;    // the longest row of mult that is staged in LDS (48 KiB)
static_assert(BS_CHUNK == BS_BLOCK * BS_ITEMS, "a chunk is one round of the workgroup");

typedef unsigned long long u64;

template <bool STAGED>
__device__ __forceinline__ u64 bs_weight(const int* __restrict__ row, const int* srow, int unit, unsigned flag, int U) {
  if (!(flag & 4u) || (unsigned)unit >= (unsigned)U) return 0;
  const unsigned w = (unsigned)(STAGED ? srow[unit] : row[unit]);
  return ((u64)w << 32) | ((flag & 1u) ? (u64)w : 0);            // all << 32 | positive
}

template <bool STAGED>
__global__ __launch_bounds__(BS_BLOCK) void bootstrap_rank_kernel(const int* __restrict__ unit_sorted, const uint8_t* __restrict__ flags,
                                                                 const int* __restrict__ mult, long long* __restrict__ out_p,
                                                                 long long* __restrict__ out_n, long long* __restrict__ out_u2,
                                                                 double* __restrict__ out_ap, double* __restrict__ out_area,
                                                                 double* __restrict__ out_f1, int n, int C, int U) {
  extern __shared__ __attribute__((aligned(16))) int srow[];      // mult[r], STAGED only
  __shared__ u64 w_tot[2][BS_WAVES];        // by chunk parity: a wave's packed total
  __shared__ u64 w_end[2][BS_WAVES];        //                  1 + the packed pair at its latest group end, relative to its start; 0: none
  __shared__ u64 red_u[BS_WAVES];
  __shared__ double red_d[3][BS_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const int* row = mult + r * (size_t)U;
  if constexpr (STAGED) {
    for (int u = tid; u < U; u += BS_BLOCK) srow[u] = row[u];
    __syncthreads();
  }
  for (int c = 0; c < C; ++c) {
    const int* us = unit_sorted + (size_t)c * (size_t)n;
    const uint8_t* fl = flags + (size_t)c * (size_t)n;

    // ---- pass 1: the column's total weights
    u64 tot = 0;
    for (long long p0 = tid; p0 < n; p0 += BS_CHUNK) {      // four positions a round, BS_BLOCK apart, their loads issued together
      int un[BS_ITEMS];
      unsigned fg[BS_ITEMS];
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j) {
        const long long p = p0 + j * BS_BLOCK;
        const bool in = p < n;
        fg[j] = in ? fl[p] : 0u;                           // flag 0: not valid, weighs nothing
        un[j] = in ? us[p] : 0;
      }
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j) tot += bs_weight<STAGED>(row, srow, un[j], fg[j], U);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d, 64);
    if (lane == 0) red_u[wave] = tot;
    __syncthreads();
    tot = 0;
#pragma unroll
    for (int w = 0; w < BS_WAVES; ++w) tot += red_u[w];
    const unsigned P = (unsigned)tot, ALLT = (unsigned)(tot >> 32);
    const double dP = (double)P;

    // ---- pass 2: the walk
    u64 carry = 0, carry_end = 0;           // the packed pair after the chunks so far; the pair at the latest group end so far
    long long acc_s = 0;                    // sum_g posw_g (2 FP_g - negw_g)
    double acc_ap = 0.0, acc_area = 0.0, acc_f1 = 0.0;
    int par = 0;
    for (long long base = 0; base < n; base += BS_CHUNK, par ^= 1) {  // 64-bit: n may be 2^31 - 1
      const long long p0 = base + tid * BS_ITEMS;
      u64 s[BS_ITEMS];
      bool e[BS_ITEMS];
      int un[BS_ITEMS];
      unsigned fg[BS_ITEMS];
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j) {
        const long long p = p0 + j;
        const bool in = p < n;
        fg[j] = in ? fl[p] : 0u;            // flag 0 past the end: weighs nothing, ends no group
        un[j] = in ? us[p] : 0;
      }
      u64 run = 0;
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j) {
        run += bs_weight<STAGED>(row, srow, un[j], fg[j], U);
        e[j] = (fg[j] & 2u) != 0;
        s[j] = run;
      }
      u64 incl = run;                       // inclusive over the wave's threads
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
      }
      const u64 excl = incl - run;          // relative to the wave's start
      u64 last = 0;
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j)
        if (e[j]) last = excl + s[j] + 1;
      u64 mincl = last;                     // the pair never decreases: the latest end is the largest
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(mincl, d, 64);
        if (lane >= d && t > mincl) mincl = t;
      }
      u64 before = __shfl_up(mincl, 1, 64);  // the latest end of the wave's earlier threads
      if (lane == 0) before = 0;
      if (lane == 63) { w_tot[par][wave] = incl; w_end[par][wave] = mincl; }
      __syncthreads();                      // the only barrier of a chunk: the slots of the other parity are being read meanwhile
      u64 off = carry, prev = carry_end, o = carry, pv = carry_end;
#pragma unroll
      for (int w = 0; w < BS_WAVES; ++w) {
        if (w == wave) { off = o; prev = pv; }
        const u64 en = w_end[par][w];
        if (en) pv = o + en - 1;
        o += w_tot[par][w];
      }
      carry = o;
      carry_end = pv;
      if (before) prev = off + before - 1;
#pragma unroll
      for (int j = 0; j < BS_ITEMS; ++j) {
        if (!e[j]) continue;
        const u64 cur = off + excl + s[j];
        const unsigned tp = (unsigned)cur, all = (unsigned)(cur >> 32), ptp = (unsigned)prev, pall = (unsigned)(prev >> 32);
        const unsigned posw = tp - ptp, negw = (all - pall) - posw, fp = all - tp;
        acc_s += (long long)posw * (2ll * (long long)fp - (long long)negw);
        if (all != 0) {
          const double prec = (double)tp / (double)all;
          if (posw != 0) {                  // then P > 0
            const double pprec = pall != 0 ? (double)ptp / (double)pall : 1.0;
            acc_ap += (double)posw * prec;
            acc_area += ((double)posw / dP) * (prec + pprec) * 0.5;
          }
          if (P != 0) {
            const double rec = (double)tp / dP;
            const double f = 2.0 * prec * rec / (prec + rec + 1e-8);
            acc_f1 = f > acc_f1 ? f : acc_f1;
          }
        }
        prev = cur;
      }
    }

    // ---- fold the four reductions: lanes by shuffles, then the waves in order
    u64 fs = (u64)acc_s;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      fs += __shfl_xor(fs, d, 64);
      acc_ap += __shfl_xor(acc_ap, d, 64);
      acc_area += __shfl_xor(acc_area, d, 64);
      const double t = __shfl_xor(acc_f1, d, 64);
      acc_f1 = t > acc_f1 ? t : acc_f1;
    }
    __syncthreads();                        // every thread has read red_u of pass 1
    if (lane == 0) { red_u[wave] = fs; red_d[0][wave] = acc_ap; red_d[1][wave] = acc_area; red_d[2][wave] = acc_f1; }
    __syncthreads();
    if (tid == 0) {
      u64 S = 0;
      double ap = 0.0, area = 0.0, f1 = 0.0;
      for (int w = 0; w < BS_WAVES; ++w) {
        S += red_u[w];
        ap += red_d[0][w];
        area += red_d[1][w];
        f1 = red_d[2][w] > f1 ? red_d[2][w] : f1;
      }
      const long long lp = (long long)P, ln = (long long)(ALLT - P);
      const size_t o = r * (size_t)C + (size_t)c;
      out_p[o] = lp;
      out_n[o] = ln;
      out_u2[o] = (long long)((u64)(2ll * ln * lp) - S);
      out_ap[o] = ap;
      out_area[o] = area;
      out_f1[o] = f1;
    }
    __syncthreads();                        // red_u / red_d are rewritten by the next column
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_bootstrap_rank_metrics(const int* unit_sorted, const uint8_t* flags, const int* mult, long long* p, long long* n_neg,
                                             long long* u2, double* ap_sum, double* auprc, double* max_f1, long long n, int C,
                                             long long R, long long U, void* stream) {
  if (!unit_sorted || !flags || !mult || !p || !n_neg || !u2 || !ap_sum || !auprc || !max_f1) return -2;
  if (n <= 0 || C <= 0 || R <= 0 || U <= 0) return -2;
  if (n > 0x7fffffffLL || U > 0x7fffffffLL) return -2;      // positions and unit ids are int32
  if (C > 65535) return -2;                                  // as the rank counts
  if (R > 0xffffffLL) return -2;                             // one workgroup per resample: R * 256 threads must stay below 2^32
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)R);
  if (U <= BS_LDS_UNITS)
    hipLaunchKernelGGL(bootstrap_rank_kernel<true>, grid, dim3(BS_BLOCK), (size_t)U * sizeof(int), st, unit_sorted, flags, mult, p, n_neg,
                       u2, ap_sum, auprc, max_f1, (int)n, C, (int)U);
  else
    hipLaunchKernelGGL(bootstrap_rank_kernel<false>, grid, dim3(BS_BLOCK), 0, st, unit_sorted, flags, mult, p, n_neg, u2, ap_sum, auprc,
                       max_f1, (int)n, C, (int)U);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
