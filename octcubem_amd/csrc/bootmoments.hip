// Bootstrap resamples of the regression metrics of the fine-tune evaluation (octcubem_amd/metrics.py: bootstrap_regression_measures):
// Pearson r, R^2, explained variance, MSE and MAE of R resamples of one evaluation set, from ONE f64 matrix product.
// Every one of those metrics is a function of eight weighted sums over the samples, and a resample is a row of int32 multiplicities,
// one per resampling unit (a sample, or a patient with all its samples).  So
//   stage 1  unit_moments_kernel       F[u][8 c + e]  the eight sums of unit u and column c over the unit's valid samples
//   stage 2  bootstrap_moments_kernel  D[r][j] = sum_u (double)mult[r][u] * F[u][j]      on v_mfma_f64_16x16x4_f64
// and the host finishes D in float64 (variances are differences of these sums: nothing narrower than f64 will do).  mult is never
// materialised as doubles: a lane converts the one multiplicity it feeds the instruction.
//
// Stage 1.  With a = (double)x - cx[c], b = (double)y - cy[c], e = (double)y - (double)x the entries are
//   0 count, 1 sum a, 2 sum b, 3 sum a^2, 4 sum b^2, 5 sum a b, 6 sum e^2, 7 sum |e|.
// One thread owns one (unit, column) and adds the unit's samples one after the other in ascending sample index (order[] is sorted
// stably by unit), so the sums do not depend on the launch.  The row of F is Cpad8 = 8 C rounded up to a multiple of 16 wide; the
// eight pad columns of an odd C are written as zero by a thread of their own.  A unit without samples gives zeros.  An entry of
// order[] outside [0, n) and a start[] outside [0, n] are never followed: nothing past an operand's edge is read.
//
// Stage 2.  Operand layout of the instruction (one f64 per lane): A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; C/D hold four f64 per
// lane, col = lane & 15, row = (lane >> 4) + 4 * reg.  A wave owns BM_ROWS = 16 resamples and up to BM_TILES = 8 feature tiles of 16
// columns (64 accumulator registers), so mult is read once for up to 16 target columns; a workgroup is BM_WAVES = 4 such waves on
// neighbouring resamples, which share nothing but the cache lines of F.  The kernel is a template on the tiles of a wave: tiles / 8
// columns of full waves in one launch, the remaining tiles % 8 in a second one, so no accumulator is indexed at run time.
// Units are walked in ascending steps of 4.  Rows past R, units past the end of the part and columns at or past 8 C enter as LITERAL zeros -- selected, never multiplied in: 0 * NaN is NaN inside
// the instruction, and what lies beside the operands is none of the kernel's business.
// The units are split over workgroups in parts of BM_SPLIT = 1024 units: the split points depend on U alone, never on R or on the
// device.  With one part the tile is stored to D; with more every part stores its tile to the workspace ws[part][R][Cpad8] and
// bootstrap_fold_kernel adds the parts in ascending order, one thread per element: a plain store-then-sum, no floating-point atomic.
// The same bits come out on every run, and row r does not depend on R or on the other rows.
// No grid is capped: the launcher refuses what its grids cannot index.  The product's grid is (ceil(R / 64), tiles / 8 or 1, parts),
// at most (2^14, 256, 2^14) under C <= 4096, R <= 2^20, U <= 2^24; the fold runs one thread per element of D, so R * Cpad8 >= 2^32 is
// refused (D alone would be 32 GiB there).
//   no 16-bit operand: the two builds of the library hold the same code.  Plain C++ plus the MFMA builtin, vector stores only.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int BM_BLOCK = 256;          // threads per workgroup, both stages
constexpr int BM_WAVES = BM_BLOCK / 64;
constexpr int BM_ROWS = 16;            // resamples per wave
constexpr int BM_TILES = 8;            // 16-column feature tiles per wave
constexpr int BM_SPLIT = 1024;         // units per part
constexpr int BM_UNROLL = 4;           // k-steps whose loads are issued together
constexpr int BM_MAX_C = 4096;
constexpr long long BM_MAX_R = 1ll << 20;
constexpr long long BM_MAX_U = 1ll << 24;
static_assert(BM_TILES == 8, "the launcher's switch lists the remainders of 8 tiles");
static_assert(BM_SPLIT % 4 == 0, "a part is a whole number of k-steps");

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(BM_BLOCK) void unit_moments_kernel(const float* __restrict__ pred, long long pred_stride,
                                                                const float* __restrict__ target, long long target_stride,
                                                                const uint8_t* __restrict__ valid, long long valid_stride,
                                                                const double* __restrict__ centre, const int* __restrict__ order,
                                                                const int* __restrict__ start, double* __restrict__ F, int n, int C, int U,
                                                                int Cpad8) {
  const long long u = (long long)blockIdx.x * BM_BLOCK + threadIdx.x;
  const int c = (int)blockIdx.y;                               // 0 .. Cpad8 / 8 - 1; c == C is the pad of an odd C
  if (u >= U) return;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (c < C) {
    int lo = start[u], hi = start[u + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double cx = centre[c], cy = centre[C + c];
    for (int p = lo; p < hi; ++p) {
      const int i = order[p];
      if ((unsigned)i >= (unsigned)n) continue;
      if (valid && !valid[(size_t)i * (size_t)valid_stride + c]) continue;
      const double x = (double)pred[(size_t)i * (size_t)pred_stride + c], y = (double)target[(size_t)i * (size_t)target_stride + c];
      const double a = x - cx, b = y - cy, e = y - x;
      s[0] += 1.0;
      s[1] += a;
      s[2] += b;
      s[3] += a * a;
      s[4] += b * b;
      s[5] += a * b;
      s[6] += e * e;
      s[7] += e < 0.0 ? -e : e;
    }
  }
  double* out = F + (size_t)u * (size_t)Cpad8 + (size_t)c * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = s[k];
}

// One k-step of the wave's NT tiles.  GUARD: the step may reach past the end of the part (the ragged last step).
template <int NT, bool GUARD>
__device__ __forceinline__ void bm_load(const int* __restrict__ mrow, const double* __restrict__ F, int u, int uend, bool row_in, int Cpad8,
                                        const int (&colc)[NT], const bool (&col_in)[NT], double& a, double (&b)[NT]) {
  const bool in = !GUARD || u < uend;
  const int uc = in ? u : uend - 1;                           // a load never leaves the operand; what it fetched is dropped below
  const int m = mrow[uc];
  a = (row_in && in) ? (double)m : 0.0;
  const double* frow = F + (size_t)uc * (size_t)Cpad8;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const double v = frow[colc[t]];
    b[t] = (in && col_in[t]) ? v : 0.0;
  }
}

template <int NT>
__global__ __launch_bounds__(BM_BLOCK) void bootstrap_moments_kernel(const int* __restrict__ mult, const double* __restrict__ F,
                                                                     double* __restrict__ out, int R, int U, int Cpad8, int cols,
                                                                     int tile0) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int r0 = ((int)blockIdx.x * BM_WAVES + wave) * BM_ROWS;
  if (r0 >= R) return;                                         // the whole wave; the kernel has no barrier
  const int t0 = tile0 + (int)blockIdx.y * NT;
  const int ubeg = (int)blockIdx.z * BM_SPLIT;
  const int uend = U - ubeg < BM_SPLIT ? U : ubeg + BM_SPLIT;
  const int idx = lane & 15, grp = lane >> 4;                  // A: row idx, k grp.  B: k grp, column idx
  const bool row_in = r0 + idx < R;
  const int* mrow = mult + (size_t)(row_in ? r0 + idx : r0) * (size_t)U;
  int colc[NT];
  bool col_in[NT];
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = (t0 + t) * 16 + idx;
    col_in[t] = col < cols;
    colc[t] = col_in[t] ? col : cols - 1;
    acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  int u0 = ubeg;
  for (; u0 + 4 * BM_UNROLL <= uend; u0 += 4 * BM_UNROLL) {    // whole k-steps: the loads of BM_UNROLL steps in flight together
    double a[BM_UNROLL], b[BM_UNROLL][NT];
#pragma unroll
    for (int s = 0; s < BM_UNROLL; ++s) bm_load<NT, false>(mrow, F, u0 + 4 * s + grp, uend, row_in, Cpad8, colc, col_in, a[s], b[s]);
#pragma unroll
    for (int s = 0; s < BM_UNROLL; ++s)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s][t], acc[t], 0, 0, 0);
  }
  for (; u0 < uend; u0 += 4) {                                 // up to BM_UNROLL steps more, the last one possibly ragged
    double a, b[NT];
    bm_load<NT, true>(mrow, F, u0 + grp, uend, row_in, Cpad8, colc, col_in, a, b);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
  }
  double* base = out + (size_t)blockIdx.z * (size_t)R * (size_t)Cpad8;   // part 0 of one is D itself
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = r0 + grp + 4 * reg;
      if (r < R) base[(size_t)r * (size_t)Cpad8 + (size_t)((t0 + t) * 16 + idx)] = acc[t][reg];
    }
  }
}

template <int NT>
static void bm_launch(hipStream_t st, const int* mult, const double* F, double* out, int R, int U, int Cpad8, int cols, int tile0,
                      unsigned groups, unsigned parts) {
  const dim3 grid((unsigned)((R + BM_WAVES * BM_ROWS - 1) / (BM_WAVES * BM_ROWS)), groups, parts);
  hipLaunchKernelGGL(bootstrap_moments_kernel<NT>, grid, dim3(BM_BLOCK), 0, st, mult, F, out, R, U, Cpad8, cols, tile0);
}

__global__ __launch_bounds__(BM_BLOCK) void bootstrap_fold_kernel(const double* __restrict__ ws, double* __restrict__ D, long long elems,
                                                                  int parts) {
  const long long i = (long long)blockIdx.x * BM_BLOCK + threadIdx.x;
  if (i >= elems) return;
  double s = ws[i];
  for (int p = 1; p < parts; ++p) s += ws[(size_t)p * (size_t)elems + (size_t)i];
  D[i] = s;
}

static inline int bm_cpad8(int C) { return (8 * C + 15) / 16 * 16; }
static inline long long bm_parts(long long U) { return (U + BM_SPLIT - 1) / BM_SPLIT; }
// one thread of the fold per element of D, 256 to a workgroup: the elements must index a one-dimensional grid of fewer than 2^32 threads
static inline bool bm_sizes_ok(long long R, long long U, int C) {
  if (R <= 0 || U <= 0 || C <= 0 || R > BM_MAX_R || U > BM_MAX_U || C > BM_MAX_C) return false;
  return R * (long long)bm_cpad8(C) < (1ll << 32);
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_unit_moments(const float* pred, long long pred_stride, const float* target, long long target_stride,
                                   const uint8_t* valid, long long valid_stride, const double* centre, const int* order, const int* start,
                                   double* F, long long n, int C, long long U, void* stream) {
  if (!pred || !target || !centre || !order || !start || !F) return -2;
  if (n <= 0 || C <= 0 || U <= 0) return -2;
  if (n > 0x7fffffffLL || U > BM_MAX_U || C > BM_MAX_C) return -2;
  if (pred_stride < C || target_stride < C || (valid && valid_stride < C)) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Cpad8 = bm_cpad8(C);
  const dim3 grid((unsigned)((U + BM_BLOCK - 1) / BM_BLOCK), (unsigned)(Cpad8 / 8));
  hipLaunchKernelGGL(unit_moments_kernel, grid, dim3(BM_BLOCK), 0, st, pred, pred_stride, target, target_stride, valid, valid_stride,
                     centre, order, start, F, (int)n, C, (int)U, Cpad8);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" long long int octmae_bootstrap_moments_ws(long long R, long long U, int C) {
  if (!bm_sizes_ok(R, U, C)) return -2;
  const long long parts = bm_parts(U);
  return parts == 1 ? 0 : parts * R * (long long)bm_cpad8(C);
}

extern "C" int octmae_bootstrap_moments(const int* mult, const double* F, double* D, double* ws, long long R, long long U, int C,
                                        void* stream) {
  if (!mult || !F || !D) return -2;
  if (!bm_sizes_ok(R, U, C)) return -2;
  const unsigned parts = (unsigned)bm_parts(U);
  if (parts > 1 && !ws) return -2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Cpad8 = bm_cpad8(C), tiles = Cpad8 / 16, cols = 8 * C;
  double* out = parts == 1 ? D : ws;
  const int full = tiles / BM_TILES, rest = tiles % BM_TILES, t1 = full * BM_TILES;   // waves of BM_TILES tiles; one column of waves with the rest
  if (full) bm_launch<BM_TILES>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, 0, (unsigned)full, parts);
  switch (rest) {
    case 1: bm_launch<1>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 2: bm_launch<2>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 3: bm_launch<3>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 4: bm_launch<4>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 5: bm_launch<5>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 6: bm_launch<6>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    case 7: bm_launch<7>(st, mult, F, out, (int)R, (int)U, Cpad8, cols, t1, 1, parts); break;
    default: break;
  }
  OCTMAE_LAUNCH_CHECK();
  if (parts > 1) {
    const long long elems = R * (long long)Cpad8;
    hipLaunchKernelGGL(bootstrap_fold_kernel, dim3((unsigned)((elems + BM_BLOCK - 1) / BM_BLOCK)), dim3(BM_BLOCK), 0, st, ws, D, elems,
                       (int)parts);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
