// Low-rank adapters (LoRA) on the four Linears of a fused Block: the merged operand and the adapter gradients.  The project's own: the
// reference fine-tunes every weight.
//   octmae_lora_merge   W f32 [O][I], A f32 [r][I], B f32 [O][r], s  ->  out_w [O][I] = W + s B A (f32, or rounded once to the 16-bit
//                       operand type), A_lp [rp][I] and B_lp [O][rp]: the 16-bit operand copies, zero in rows / columns r .. rp - 1
//   octmae_lora_wgrad   X [M][I], dY [M][O] (16 bit, the operands of the weight-gradient GEMM this replaces)  ->
//                       gA f32 [r][I] += s (dY B)^T X,   gB f32 [O][r] += s dY^T (X A^T)        -- no [O][I] weight gradient anywhere
// rp = r rounded up to 16 (one 16x16x32 MFMA column tile per 16 ranks), r <= 64.
//
// The gradient is the TWO-PASS form: X and dY are read twice.
//   1 lora_bt_kernel       Bt [rp][O] = B_lp^T (16 bit, in the workspace): both projections then read k-contiguous operands
//   2 lora_project_kernel  T = X A_lp^T, U = dY Bt^T: one wave per 16 token rows, operands straight from global memory (16-byte loads,
//                          the MFMA's own fragment shape), fp32 accumulators, ONE rounding to the operand type, [M][rp] in the workspace
//   3 lora_outer_kernel    P_c [I + O][rp] = (X | dY)^T (U | T) over row chunk c: both products reduce over the token index, which is the
//                          ROW index of all four row-major operands, so a 32-row tile of each goes to LDS as it lies and the fragments come
//                          back through ds_read_b64_tr_b16; a workgroup owns 64 columns of X or dY and one row chunk; plain stores of its
//                          fp32 partial into the chunk's slab
//   4 lora_fold_kernel     g = fma(s, ((P_0 + P_1) + ...) + P_{n-1}, g): ascending chunk order, no atomics anywhere -- two calls give the same bits
// The one-pass form (a workgroup keeps its chunk's T and U in LDS and reads X and dY once) needs the [rp][I] and [O][rp] partials of a
// chunk resident while the chunk streams by: 320 KB at fc1 with rp = 16, more than a workgroup holds; it is not built.
// Bytes: 2 * 2 M (I + O) read, 2 * 2 M rp * 2 for T and U, 2 * 4 n (I + O) rp for the slabs (n chunks of >= 256 rows).
//
// Compiled with -ffp-contract=off (Makefile): the merge states its roundings -- delta = fmaf(B[o][k], A[k][i], delta) in ascending k,
// v = fmaf(s, delta, W[o][i]) -- and tests/lora_ref.py bounds them; the fold's is the one fmaf above.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int LORA_MAX_RANK = 64;
constexpr int LORA_COLS = 64;        // columns of X or dY per workgroup of the outer-product kernel (16 per wave)
constexpr int LORA_KROWS = 32;       // token rows per MFMA step
constexpr int LORA_MIN_CHUNK = 256;  // rows per chunk at least: the slab of a chunk is 4 rp bytes per column against 2 * chunk read
constexpr int LORA_TARGET_WG = 1024; // workgroups the plan aims for (4 per CU of 256)
constexpr int LORA_GROWB = (LORA_COLS + 8) * 2;   // LDS row of the X / dY tile in bytes: 128 + 16 of padding

struct LoraPlan {
  int chunk, nchunks, tiles_x, tiles_y;
};

static inline LoraPlan lora_plan(int M, int I, int O) {
  LoraPlan p;
  p.tiles_x = (I + LORA_COLS - 1) / LORA_COLS;
  p.tiles_y = (O + LORA_COLS - 1) / LORA_COLS;
  const int tiles = p.tiles_x + p.tiles_y;
  const int want = (LORA_TARGET_WG + tiles - 1) / tiles;
  long long rows = ((long long)M + want - 1) / want;
  rows = (rows + LORA_KROWS - 1) / LORA_KROWS * LORA_KROWS;
  if (rows < LORA_MIN_CHUNK) rows = LORA_MIN_CHUNK;
  p.chunk = (int)rows;
  p.nchunks = (int)(((long long)M + rows - 1) / rows);
  return p;
}

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct LoraWs {
  size_t t_off, u_off, bt_off, slab_off, total;
};

static inline LoraWs lora_ws(int M, int I, int O, int rp) {
  const LoraPlan p = lora_plan(M, I, O);
  LoraWs w;
  const size_t proj = up256((size_t)M * rp * 2);
  w.t_off = 0;
  w.u_off = proj;
  w.bt_off = 2 * proj;
  w.slab_off = w.bt_off + up256((size_t)rp * O * 2);
  w.total = w.slab_off + (size_t)p.nchunks * ((size_t)I + O) * rp * 4;
  return w;
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
template <bool OUT_F32>
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ B,
                                                         float s, int O, int I, int r, int rp, void* __restrict__ out_w,
                                                         bf16_t* __restrict__ A_lp, bf16_t* __restrict__ B_lp) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  const size_t quads = (size_t)O * I / 4;
  const int iq = I / 4;
  for (size_t q = tid; q < quads; q += nthreads) {
    const int o = (int)(q / iq), i = (int)(q % iq) * 4;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < r; ++k) {
      const float b = B[(size_t)o * r + k];
      const f32x4 a = *reinterpret_cast<const f32x4*>(A + (size_t)k * I + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = fmaf(b, a[e], d[e]);
    }
    const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)o * I + i);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(s, d[e], w[e]);
    if (OUT_F32) {
      *reinterpret_cast<f32x4*>(static_cast<float*>(out_w) + (size_t)o * I + i) = v;
    } else {
      u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *reinterpret_cast<u32x2*>(static_cast<bf16_t*>(out_w) + (size_t)o * I + i) = pk;
    }
  }
  if (A_lp) {
    const size_t n = (size_t)rp * I;
    for (size_t e = tid; e < n; e += nthreads) {
      const int k = (int)(e / I);
      A_lp[e] = k < r ? f2bf(A[e]) : (bf16_t)0;      // rows < r of [rp][I] and of [r][I] lie at the same offsets
    }
  }
  if (B_lp) {
    const size_t n = (size_t)O * rp;
    for (size_t e = tid; e < n; e += nthreads) {
      const size_t o = e / rp;
      const int k = (int)(e % rp);
      B_lp[e] = k < r ? f2bf(B[o * r + k]) : (bf16_t)0;
    }
  }
}

// ---- gradient, pass 1 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lora_bt_kernel(const bf16_t* __restrict__ B_lp, bf16_t* __restrict__ Bt, int O, int rp) {
  const size_t n = (size_t)rp * O;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t j = e / O, o = e % O;
    Bt[e] = B_lp[o * rp + j];
  }
}

struct LoraProj {
  const bf16_t* G;     // [M][ld] token rows
  const bf16_t* Wt;    // [rp][K]
  bf16_t* out;         // [M][rp]
  int ld, K;
};

// P[m][j] = sum_k G[m][k] Wt[j][k].  mfma16x16 (16x16x32): lane l, c = l & 15, g = l >> 4 holds A[row c][k = 8 g + e] and B[k = 8 g + e][col c],
// e = 0 .. 7 -- 16 contiguous bytes of a row of G and of a row of Wt; D register e = D[row 4 g + e][col c].  A row past M reads row M - 1
// (its products stay in its own D row, which is not stored); 8-element groups past K enter as zeros on both sides.
template <int NJ>
__global__ __launch_bounds__(256) void lora_project_kernel(LoraProj p0, LoraProj p1, int M) {
  const LoraProj p = blockIdx.y == 0 ? p0 : p1;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (m0 >= M) return;                                          // the whole wave; the kernel has no barrier
  const long long row = m0 + c < M ? m0 + c : M - 1;
  const bf16_t* grow = p.G + (size_t)row * p.ld;
  f32x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = 0; k0 < p.K; k0 += 32) {
    const int k = k0 + 8 * g;
    const bool ok = k < p.K;
    const int kc = ok ? k : 0;
    bf16x8 a = *reinterpret_cast<const bf16x8*>(grow + kc);
    a = ok ? a : zero;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      bf16x8 b = *reinterpret_cast<const bf16x8*>(p.Wt + (size_t)(16 * j + c) * p.K + kc);
      b = ok ? b : zero;
      acc[j] = mfma16x16(a, b, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long m = m0 + 4 * g + e;
      if (m < M) p.out[(size_t)m * (16 * NJ) + 16 * j + c] = f2bf(acc[j][e]);
    }
}

// ---- gradient, pass 2 ------------------------------------------------------------------------------------------------------------------
// 8 operand elements of a 16x16x32 MFMA from a plain row-major LDS tile through two transposed reads: lane 4q + p of each 16-lane group
// supplies row (row0 + q), columns col0 + 4p .. + 3, and lane i of the group receives column col0 + i of those 4 rows; the second read
// takes the 4 rows below.  With row0 = 8 (lane >> 4): element e = tile[8 (lane >> 4) + e][col0 + (lane & 15)].  Every lane must be active.
__device__ __forceinline__ bf16x8 lora_tr_frag(const char* base, int rowb, int col0, int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3, row0 = 8 * (lane >> 4);
  const char* a = base + (row0 + q) * rowb + (col0 + 4 * p) * 2;
  return cat4(lds_tr_read(a), lds_tr_read(a + 4 * rowb));
}

// P[col][j] = sum over the chunk's rows m of G[m][col] S[m][j]; G = X with S = U (tiles 0 .. tiles_x - 1; P rows 0 .. I - 1) or G = dY with
// S = T (the tiles behind; P rows I .. I + O - 1).  MFMA A operand = G^T (row = column of G), B operand = S; D register e = P[4 g + e][c].
// Rows past the chunk or M and columns past the operand's width enter as zeros (selected, never loaded).
template <int NJ>
__global__ __launch_bounds__(256) void lora_outer_kernel(const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ dY, int ldy,
                                                         const bf16_t* __restrict__ T, const bf16_t* __restrict__ U, float* __restrict__ slabs,
                                                         int M, int I, int O, int chunk, int tile0, int tiles_x) {
  constexpr int RP = 16 * NJ, SROWB = (RP + 8) * 2, SPIECES = RP / 8;
  __shared__ __attribute__((aligned(16))) char smem[LORA_KROWS * LORA_GROWB + LORA_KROWS * SROWB];
  char* Gs = smem;
  char* Ss = smem + LORA_KROWS * LORA_GROWB;
  const int tile = tile0 + blockIdx.x;
  const bool is_x = tile < tiles_x;
  const bf16_t* G = is_x ? X : dY;
  const bf16_t* S = is_x ? U : T;
  const int ldg = is_x ? ldx : ldy, ncols = is_x ? I : O;
  const int col0 = (is_x ? tile : tile - tiles_x) * LORA_COLS;
  const long long mbeg = (long long)blockIdx.y * chunk;
  const long long mend = mbeg + chunk < M ? mbeg + chunk : M;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int grow = t >> 3, gcol = col0 + (t & 7) * 8;
  const bool gcol_ok = gcol < ncols;
  const int srow = t / SPIECES, spiece = t % SPIECES;
  const bool s_thread = t < LORA_KROWS * SPIECES;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 gv = zero, sv = zero;
  auto fetch = [&](long long m0) {
    gv = zero;
    sv = zero;
    if (gcol_ok && m0 + grow < mend) gv = *reinterpret_cast<const bf16x8*>(G + (size_t)(m0 + grow) * ldg + gcol);
    if (s_thread && m0 + srow < mend) sv = *reinterpret_cast<const bf16x8*>(S + (size_t)(m0 + srow) * RP + spiece * 8);
  };
  fetch(mbeg);
  for (long long m0 = mbeg; m0 < mend; m0 += LORA_KROWS) {
    __syncthreads();                                            // the previous step's fragment reads are done
    *reinterpret_cast<bf16x8*>(Gs + grow * LORA_GROWB + (t & 7) * 16) = gv;
    if (s_thread) *reinterpret_cast<bf16x8*>(Ss + srow * SROWB + spiece * 16) = sv;
    __syncthreads();
    if (m0 + LORA_KROWS < mend) fetch(m0 + LORA_KROWS);
    const bf16x8 a = lora_tr_frag(Gs, LORA_GROWB, 16 * wave, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = mfma16x16(a, lora_tr_frag(Ss, SROWB, 16 * j, lane), acc[j]);
  }
  const int c = lane & 15, g = lane >> 4;
  float* slab = slabs + (size_t)blockIdx.y * ((size_t)I + O) * RP + (is_x ? (size_t)0 : (size_t)I * RP);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int col = col0 + 16 * wave + 4 * g + e;
    if (col < ncols) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) slab[(size_t)col * RP + 16 * j + c] = acc[j][e];
    }
  }
}

// gA[j][i] = fma(s, sum_c P_c[i][j], gA[j][i]) for j < r;  gB[o][j] = fma(s, sum_c P_c[I + o][j], gB[o][j]) for j < r; chunks ascending
__global__ __launch_bounds__(256) void lora_fold_kernel(const float* __restrict__ slabs, int nchunks, float s, int I, int O, int r, int rp,
                                                        float* __restrict__ gA, int ldga, float* __restrict__ gB, int ldgb) {
  const size_t na = gA ? (size_t)r * I : 0, nb = gB ? (size_t)O * r : 0;
  const size_t stride = ((size_t)I + O) * rp;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < na + nb; e += (size_t)gridDim.x * 256) {
    size_t src;
    float* dst;
    if (e < na) {
      const size_t j = e / I, i = e % I;
      src = i * rp + j;
      dst = gA + j * (size_t)ldga + i;
    } else {
      const size_t o = (e - na) / r, j = (e - na) % r;
      src = ((size_t)I + o) * rp + j;
      dst = gB + o * (size_t)ldgb + j;
    }
    float p = slabs[src];
    for (int c = 1; c < nchunks; ++c) p = __fadd_rn(p, slabs[(size_t)c * stride + src]);
    *dst = fmaf(s, p, *dst);
  }
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static inline unsigned lora_blocks(size_t n) {
  const size_t b = (n + 255) / 256;
  return (unsigned)(b > 8192 ? 8192 : b < 1 ? 1 : b);
}
// the contract both entry points and the two queries share: I and O are the widths of 16-bit GEMM operands (multiples of 8)
static inline bool lora_dims_ok(long long I, long long O) { return I >= 8 && O >= 8 && I % 8 == 0 && O % 8 == 0; }

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_lora_merge(const float* W, const float* A, const float* B, float s, int O, int I, int r, void* out_w, int out_is_f32,
                                 void* A_lp, void* B_lp, void* stream) {
  OCTMAE_CHECK_ARG(r >= 1 && r <= LORA_MAX_RANK);
  OCTMAE_CHECK_ARG(lora_dims_ok(I, O));
  OCTMAE_CHECK_ARG(W && A && B && out_w);
  OCTMAE_CHECK_ARG(out_is_f32 == 0 || out_is_f32 == 1);
  // 16-byte loads of W and A, 16- or 8-byte stores of out_w; 4-byte loads of B; 2-byte stores of the operand copies
  OCTMAE_CHECK_ARG(al16(W) && al16(A) && al4(B) && al16(out_w));
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(A_lp) & 1u) == 0 && (reinterpret_cast<uintptr_t>(B_lp) & 1u) == 0);
  OCTMAE_CHECK_ARG(s == s);
  const int rp = (r + 15) / 16 * 16;
  const unsigned blocks = lora_blocks((size_t)O * I / 4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (out_is_f32)
    hipLaunchKernelGGL(lora_merge_kernel<true>, dim3(blocks), dim3(256), 0, st, W, A, B, s, O, I, r, rp, out_w, static_cast<bf16_t*>(A_lp),
                       static_cast<bf16_t*>(B_lp));
  else
    hipLaunchKernelGGL(lora_merge_kernel<false>, dim3(blocks), dim3(256), 0, st, W, A, B, s, O, I, r, rp, out_w, static_cast<bf16_t*>(A_lp),
                       static_cast<bf16_t*>(B_lp));
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

static inline bool lora_rp_ok(int rp) { return rp >= 16 && rp <= LORA_MAX_RANK && rp % 16 == 0; }

extern "C" int octmae_lora_plan(int M, int I, int O, int rp, int* out) {
  OCTMAE_CHECK_ARG(out && M >= 1 && lora_rp_ok(rp) && lora_dims_ok(I, O));
  const LoraPlan p = lora_plan(M, I, O);
  out[0] = p.chunk;
  out[1] = p.nchunks;
  out[2] = p.tiles_x;
  out[3] = p.tiles_y;
  return 0;
}

extern "C" int octmae_lora_ws_bytes(int M, int I, int O, int rp, long long* bytes) {
  OCTMAE_CHECK_ARG(bytes && M >= 1 && lora_rp_ok(rp) && lora_dims_ok(I, O));
  *bytes = (long long)lora_ws(M, I, O, rp).total;
  return 0;
}

template <int NJ>
static int lora_wgrad_launch(const bf16_t* X, int ldx, const bf16_t* dY, int ldy, const bf16_t* A_lp, const bf16_t* B_lp, float s, int M, int I,
                             int O, int r, float* gA, int ldga, float* gB, int ldgb, char* ws, hipStream_t st) {
  constexpr int RP = 16 * NJ;
  const LoraPlan pl = lora_plan(M, I, O);
  const LoraWs w = lora_ws(M, I, O, RP);
  bf16_t* T = reinterpret_cast<bf16_t*>(ws + w.t_off);
  bf16_t* U = reinterpret_cast<bf16_t*>(ws + w.u_off);
  bf16_t* Bt = reinterpret_cast<bf16_t*>(ws + w.bt_off);
  float* slabs = reinterpret_cast<float*>(ws + w.slab_off);
  const LoraProj pt = {X, A_lp, T, ldx, I}, pu = {dY, Bt, U, ldy, O};
  const unsigned rowblocks = (unsigned)(((long long)M + 63) / 64);
  if (gA) hipLaunchKernelGGL(lora_bt_kernel, dim3(lora_blocks((size_t)RP * O)), dim3(256), 0, st, B_lp, Bt, O, RP);
  // T serves gB, U serves gA: with one of the two absent only the other projection runs
  if (gA && gB)
    hipLaunchKernelGGL(lora_project_kernel<NJ>, dim3(rowblocks, 2), dim3(256), 0, st, pt, pu, M);
  else if (gB)
    hipLaunchKernelGGL(lora_project_kernel<NJ>, dim3(rowblocks, 1), dim3(256), 0, st, pt, pt, M);
  else
    hipLaunchKernelGGL(lora_project_kernel<NJ>, dim3(rowblocks, 1), dim3(256), 0, st, pu, pu, M);
  const int tile0 = gA ? 0 : pl.tiles_x;
  const int ntiles = (gA ? pl.tiles_x : 0) + (gB ? pl.tiles_y : 0);
  hipLaunchKernelGGL(lora_outer_kernel<NJ>, dim3(ntiles, pl.nchunks), dim3(256), 0, st, X, ldx, dY, ldy, T, U, slabs, M, I, O, pl.chunk, tile0,
                     pl.tiles_x);
  const size_t nfold = (gA ? (size_t)r * I : 0) + (gB ? (size_t)O * r : 0);
  hipLaunchKernelGGL(lora_fold_kernel, dim3(lora_blocks(nfold)), dim3(256), 0, st, slabs, pl.nchunks, s, I, O, r, RP, gA, ldga, gB, ldgb);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_lora_wgrad(const void* X, int ldx, const void* dY, int ldy, const void* A_lp, const void* B_lp, float s, int M, int I,
                                 int O, int r, float* gA, int ldga, float* gB, int ldgb, void* ws, long long ws_bytes, void* stream) {
  OCTMAE_CHECK_ARG(r >= 1 && r <= LORA_MAX_RANK);
  OCTMAE_CHECK_ARG(M >= 1 && lora_dims_ok(I, O));
  OCTMAE_CHECK_ARG(X && dY && A_lp && B_lp && ws && (gA || gB));
  OCTMAE_CHECK_ARG(ldx >= I && ldy >= O && ldx % 8 == 0 && ldy % 8 == 0);
  OCTMAE_CHECK_ARG(!gA || ldga >= I);
  OCTMAE_CHECK_ARG(!gB || ldgb >= r);
  // 16-byte loads of X, dY and the operand copies; the workspace holds 16-byte-loaded tensors at multiples of 256 bytes
  OCTMAE_CHECK_ARG(al16(X) && al16(dY) && al16(A_lp) && al16(B_lp) && al16(ws) && al4(gA) && al4(gB));
  OCTMAE_CHECK_ARG(s == s);
  const int rp = (r + 15) / 16 * 16;
  OCTMAE_CHECK_ARG(ws_bytes >= (long long)lora_ws(M, I, O, rp).total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t *x = static_cast<const bf16_t*>(X), *dy = static_cast<const bf16_t*>(dY), *a = static_cast<const bf16_t*>(A_lp),
               *b = static_cast<const bf16_t*>(B_lp);
  char* w = static_cast<char*>(ws);
  switch (rp / 16) {
    case 1: return lora_wgrad_launch<1>(x, ldx, dy, ldy, a, b, s, M, I, O, r, gA, ldga, gB, ldgb, w, st);
    case 2: return lora_wgrad_launch<2>(x, ldx, dy, ldy, a, b, s, M, I, O, r, gA, ldga, gB, ldgb, w, st);
    case 3: return lora_wgrad_launch<3>(x, ldx, dy, ldy, a, b, s, M, I, O, r, gA, ldga, gB, ldgb, w, st);
    default: return lora_wgrad_launch<4>(x, ldx, dy, ldy, a, b, s, M, I, O, r, gA, ldga, gB, ldgb, w, st);
  }
}
