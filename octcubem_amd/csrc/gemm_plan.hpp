// Which kernel a GEMM entry point of gemm.hip launches, and with what parameters: plain host C++ (no HIP, no launches, no device
// pointers), so that every decision is written once, can be queried without a GPU (octmae_gemm_plan, octmae_wgrad_pair_plan) and is
// tested there (tests/test_cpu_host.py).  gemm.hip checks arguments, asks plan_gemm / plan_wgrad_pair and launches what the plan names.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>

namespace octmae {
// tiles: gemm_kernel (register-staged) TA x TB x TK, gemm256_kernel / gemm256p_kernel T2 x T2 x TK,
// gemm128d_kernel (small launches) T1 x T1 x TK
constexpr int TA = 128, TB = 128, TK = 64, T2 = 256, T1 = 128, D_SLOT_FLOATS = T1 * T1;
// Split-K workspace of the small-launch kernel (caller-owned, lent per call, one per stream): [D_WS_SLOTS partial tiles of 64 KiB]
// [D_WS_TILES arrival counters].  The counters must be zero when the workspace is first lent; every launch leaves them zero.
constexpr int D_WS_SLOTS = 1024, D_WS_TILES = 4096;
inline long long d_ws_bytes() { return (long long)D_WS_SLOTS * D_SLOT_FLOATS * 4 + (long long)D_WS_TILES * 4; }
enum Epi : int {
  EPI_BF16 = 0,      // C bf16 = X (+bias[a])
  EPI_F32 = 1,       // C f32  = X (+bias[a])
  EPI_GELU = 2,      // C bf16 = X+bias (pre-activation), C2 bf16 = gelu(X+bias)
  EPI_RESID = 3,     // C f32  = aux_f32 + X + bias
  EPI_DGELU = 4,     // C bf16 = X * gelu'(aux_bf16)
  EPI_ACCUM = 5,     // C f32 += X   (OUT_AB; atomics when split-K > 1)
  EPI_DELTA = 6,     // C bf16 = X, C2 f32 [NB][ldc2]: C2[b][a / hd] = -sum_{j < hd} bf16(X[b][a0 + j]) * aux_bf16[b][a0 + j]
                     //   (the attention backward's per-query delta = rowsum(dO * O), from the proj dgrad that produces dO;
                     //   256-tile LDS-transposing epilogue only)
  EPI_ACCUM_SLAB = 7,   // C f32 = X, C the slab of one k slice (deterministic mode; inside gemm.hip only, never an entry point's `epilogue`)
};

// ---- variant bits ---------------------------------------------------------------------------------------------------------------
// Tests and A/B runs exercise every kernel on the same problem through bits 8-18 of octmae_gemm_bf16's `epilogue` and of the fused
// entry points' `variant` (include/octmae.h; octcubem_amd/ops.py: _variant_bits).  This is the only place C++ knows the layout.
struct GemmVariant {
  bool tile128;          // bit 8: the 128-tile register-staged kernel
  bool two_stage;        // bit 9: the two-stage (un-phased) 256-tile main loop wherever the problem takes 256-tiles
  bool phased_forced;    // bit 10: the phased one (also the default; wins over bit 9)
  bool never_small;      // bit 14: never the small-launch kernel (the pre-round-6 choice)
  bool dgelu_stored;     // bit 15: the fc1 forward stores gelu'(pre) / the fc2 dgrad multiplies with it
  int force_small_nst;   // bit 12 / 13: the small-launch kernel with a 4- / 2-stage ring (0: not forced)
  int forced_split;      // bits 16-18: the forced kernel's k split where the entry point has no `splitk` (0: use `splitk`)
  // phased main loop by default (dgrad, wgrad: +10..25 % over the two-stage loop; forward, re-measured in round 2 after the
  // epilogue work: qkv -4 %, proj -11 %, fc2 -8 %, fc1 + GELU -1.5 %, decoder fc1 + GELU +0.6 % -- in round 1 the two-stage loop
  // had still been 12 % faster at K = 1024).
  bool phased() const { return phased_forced || !two_stage; }
};
inline GemmVariant decode_variant(int bits) {
  return {((bits >> 8) & 1) != 0, ((bits >> 9) & 1) != 0, ((bits >> 10) & 1) != 0, ((bits >> 14) & 1) != 0, ((bits >> 15) & 1) != 0,
          ((bits >> 12) & 1) ? 4 : ((bits >> 13) & 1) ? 2 : 0, (bits >> 16) & 7};
}

// ---- options ---------------------------------------------------------------------------------------------------------------------
// octmae_set_option atomics (defined in gemm.hip, set in attn_bwd.hip); an environment variable, read once per process, wins.
extern std::atomic<int> g_gemm_small, g_wgrad_stagger, g_wgrad_s1_atomic, g_deterministic;
struct GemmOptions {
  int gemm_small;        // "gemm_small" / OCTMAE_GEMM_SMALL: the small-launch kernels where the cost models pick them
  int wgrad_stagger;     // "wgrad_stagger" / OCTMAE_WGRAD_STAGGER: see wgrad_stagger_for
  int wgrad_s1_atomic;   // "wgrad_s1_atomic" / OCTMAE_WGRAD_S1_ATOMIC: GemmParams::atomic1 of the phased weight-gradient kernels
  int cgroup_force;      // OCTMAE_CGROUP (A/B runs): column-tile group of forward / dgrad launches, 0 = the rule of cgroup_for
  int wgrad128_maxkt;    // OCTMAE_WGRAD128_MAXKT (A/B runs): longest reduction the 128-tile weight-gradient pair takes, default 96
  int deterministic;     // "deterministic" / OCTMAE_DETERMINISTIC: no float is added in the order workgroups finish (det_* below; optim.hip)
};
inline GemmOptions current_options() {
  auto env = [](const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; };
  static const GemmOptions e{env("OCTMAE_GEMM_SMALL", -1), env("OCTMAE_WGRAD_STAGGER", -1), env("OCTMAE_WGRAD_S1_ATOMIC", -1),
                             env("OCTMAE_CGROUP", 0), env("OCTMAE_WGRAD128_MAXKT", 96), env("OCTMAE_DETERMINISTIC", -1)};
  return {e.gemm_small >= 0 ? e.gemm_small : g_gemm_small.load(std::memory_order_relaxed),
          e.wgrad_stagger >= 0 ? e.wgrad_stagger : g_wgrad_stagger.load(std::memory_order_relaxed),
          e.wgrad_s1_atomic >= 0 ? e.wgrad_s1_atomic : g_wgrad_s1_atomic.load(std::memory_order_relaxed), e.cgroup_force, e.wgrad128_maxkt,
          (e.deterministic >= 0 ? e.deterministic : g_deterministic.load(std::memory_order_relaxed)) != 0};
}

// ---- shared rules ----------------------------------------------------------------------------------------------------------------
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// what both LDS-DMA kernel families ask of the operands: whole k-tiles of a k-contiguous operand, each inside a 32-bit buffer range
inline bool dma_operands_ok(int NA, int NB, int K, int lda, int ldb, bool a_ks, bool b_ks) {
  if ((!a_ks || !b_ks) && (K % TK) != 0) return false;
  const size_t a_bytes = (size_t)(a_ks ? K : NA) * lda * 2, b_bytes = (size_t)(b_ks ? K : NB) * ldb * 2;
  return a_bytes < 0xFFF00000ull && b_bytes < 0xFFF00000ull;
}
// the problem takes the 256-tile LDS-DMA kernels: at least one full tile each way; otherwise the 128-tile register-staged kernel
inline bool fits_256(int NA, int NB, int K, int lda, int ldb, bool a_ks, bool b_ks) {
  return NA >= T2 && NB >= T2 && dma_operands_ok(NA, NB, K, lda, ldb, a_ks, b_ks);
}
// operands the small-launch kernel can take (the epilogue transposes 8-column chunks; forward and dgrad layouts only)
inline bool gemm128_ok(int NA, int NB, int K, int lda, int ldb, bool a_ks, bool b_ks) {
  return (NA & 7) == 0 && !(a_ks && b_ks) && dma_operands_ok(NA, NB, K, lda, ldb, a_ks, b_ks);
}
// Column-tile group of the 256-tile kernels' tile order (tile_coord).  Forward / dgrad: groups of 4 column tiles when there are
// >= 16 of them and 4 weight panels fit half the L2 (K <= 1024: the fc1 forward and the fc2 dgrad of ViT-L).  Measured same-box:
// fc1 forward 891 -> 871 us, fc2 dgrad+dgelu 801 -> 790 us; narrower groups (K >= 3072, one panel per group) lose 3-5 % to the
// activation re-reads and 12 column tiles (qkv) gain nothing, so those keep the plain order.  Weight gradients: the ~32 workgroups
// an XCD runs at a time should form a compact rectangle of tiles (8 x 4 rather than 16 x 2 for fc1's 16 x 4 tiles): c column tiles
// x all row tiles, c = 32 / tiles_b rounded down to a divisor of tiles_a.
inline int cgroup_for(int epi, int tiles_a, int tiles_b, int K, const GemmOptions& o) {
  if (epi != EPI_ACCUM) {
    if (o.cgroup_force > 0) return tiles_a % o.cgroup_force == 0 ? o.cgroup_force : tiles_a;
    return tiles_a >= 16 && tiles_a % 4 == 0 && 4 * (size_t)T2 * K * 2 <= (2u << 20) ? 4 : tiles_a;
  }
  if (tiles_a * tiles_b <= 32) return tiles_a;
  int c = tiles_b > 32 ? 1 : 32 / tiles_b;
  while (c > 1 && tiles_a % c != 0) --c;
  return c;
}
// a requested k split as the kernels run it: at most one slice per k-tile, equal lengths, no empty slice
struct Split { int slices, per; };
inline Split normalise_split(int ktiles, int splitk) {
  splitk = splitk < 1 ? 1 : splitk > ktiles ? ktiles : splitk;
  const int per = cdiv(ktiles, splitk);
  return {cdiv(ktiles, per), per};
}
inline bool last_slice_empty(int ktiles, int S) { return (long long)(S - 1) * cdiv(ktiles, S) >= ktiles; }
// The k split of a weight gradient whose caller leaves it to the planner (splitk <= 0): as many k slices as keep tiles x slices within
// ONE round of workgroups over the chip (target: 256 blocks of 256-tiles, 1024 of 128-tiles; a second, partly filled round costs more
// than the slightly lower fill), and >= 8 k-tiles (512 token rows) per slice --
// unless, on 256-tiles, the split costs more than it saves (round 6, small batches): every workgroup ends with 256 KiB of fp32
// atomics, which the L2s retire at ~1.2 TB/s in all -- 0.22 us per tile and slice -- against ~1.4 us per k-tile of the main loop (fitted
// on graph-replayed launches, tools/gemm_small_fit.py / profiles/r06_gemm_small_fit.txt).  One volume per step (21 k-tiles): the
// fc1 + fc2 pair as 128 tiles x 2 slices was 68 us, unsplit (one atomic add per element) it is 54 us.  From 32 volumes per micro-batch
// on the minimum is the old choice (the most slices that fit one round).  The first minimum wins.
inline int auto_wgrad_split(int out_tiles, int ktiles, int target_blocks) {
  int s = std::max(1, std::min(target_blocks / out_tiles, ktiles >= 8 ? ktiles / 8 : 1));
  if (s > 1 && target_blocks == 256) {
    double best = 1e30;
    for (int k = 1, most = s; k <= most; ++k) {
      const double cost = 1.4 * cdiv(ktiles, k) + 0.22 * out_tiles * k;
      if (cost < best) { best = cost; s = k; }
    }
  }
  return s;
}
// the k split of a FORCED small launch: 1 .. 4 as asked; less without a workspace, with an empty slice or with more partial
// tiles than slots
inline int clamp_forced_split(int S, int ktiles, long long nt128, bool have_ws) {
  S = S < 1 ? 1 : S > 4 ? 4 : S;
  while (S > 1 && (!have_ws || last_slice_empty(ktiles, S) || nt128 * S > D_WS_SLOTS)) --S;
  return S;
}
// Staggered split-K slices of the 256-tile weight-gradient kernel (split_range): v = the length step between neighbouring slices in
// 1/256 k-tiles PER OUTPUT TILE of the launch (the atomic time of a slice grows with its tile count: 256 KiB at 1.35 TB/s = 0.19 us
// per tile against 1.7 us per k-tile, i.e. v = 29); 0 = equal slices.  octmae_set_option("wgrad_stagger", v) / OCTMAE_WGRAD_STAGGER.
// Applied only to splits of >= 8 slices with <= 96 k-tiles each (the [C x C] proj gradients at <= 32 volumes per rank): measured
// (profiles/r04_wgrad_stagger.txt) -9 / -11 % there, and nothing or a loss for the 4- and 5-way splits
// and for every shape at 128 volumes -- their workgroups do not end together anyway.
// Returns GemmParams::kstagger of an S-way split over `ktiles` k-tiles of a launch with `tiles` output tiles (0: equal slices).
inline int wgrad_stagger_for(int ktiles, int splitk, int tiles, int v) {
  if (!(v > 0 && splitk >= 8 && ktiles <= 96 * splitk)) return 0;
  // the shortest slice (ktiles / S - d (S - 1) / 2) keeps at least half the mean length and 8 k-tiles
  const long long mean_q8 = ((long long)ktiles << 8) / splitk;
  long long d = (long long)v * tiles;
  const long long dmax = (mean_q8 - (8 << 8) < mean_q8 / 2 ? mean_q8 - (8 << 8) : mean_q8 / 2) * 2 / (splitk - 1);
  if (d > dmax) d = dmax;
  return d > 0 ? (int)d : 0;
}
// ---- deterministic mode ("deterministic") ----------------------------------------------------------------------------------------
// A weight gradient split S > 1 ways over k adds nothing into gW from the GEMM: slice z leaves its fp32 partial as slab z of a lent
// workspace -- fp32 [S][NA][NB], rows packed, plain stores, need not be initialised -- and wgrad_fold_kernel (one launch of its own,
// both outputs of a pair) computes gW = (...((gW + P_0) + P_1) ... + P_{S-1}): what S unsplit launches over the slices' row ranges,
// issued in order, would leave.  GemmParams::atomic1 of such a launch is ATOMIC1_SLABS.  The split is the one chosen without the mode,
// capped so that the slabs fit (down to 1: never atomics), and unstaggered (the stagger spreads atomic epilogues).
constexpr int ATOMIC1_SLABS = 3;
inline long long det_slab_bytes(long long out_elems, int slices) { return slices > 1 ? out_elems * 4 * slices : 0; }
inline int det_cap_split(int slices, long long out_elems, long long ws_bytes) {
  const long long fit = ws_bytes / (out_elems * 4);
  return fit < 2 ? 1 : fit < slices ? (int)fit : slices;
}
// the bytes of a lent split-K workspace the slabs may take: everything in front of the arrival counters of the small-launch kernel
inline long long det_usable_ws(long long bytes) {
  const long long slots = (long long)D_WS_SLOTS * D_SLOT_FLOATS * 4;
  return bytes <= 0 ? 0 : bytes < slots ? bytes : slots;
}

// use = 1: gemm128d_kernel; S: k slices per tile (1: no workspace needed); nst: ring stages, 4 (one workgroup per CU) or 2 (two)
struct Plan128 { int use, S, nst; };
// Which kernel a forward / dgrad launch of NA x NB x K takes on G CUs (fitted on MI355X with tools/gemm_small_fit.py: device times of
// graph-replayed launches, profiles/r06_gemm_small_fit.txt).
//  * At most one round of 256-tiles (nt256 <= G, the regime the kernel was built for): a latency model in microseconds.  A workgroup of
//    the 256-tile kernel takes ~1.05 us per k-tile + ~6.5 us (prologue, epilogue, launch); one of this kernel ~0.5 us per k-tile + ~4.5 us
//    alone on its CU (4-stage ring) and ~0.85 us per k-tile + ~5.5 us in rounds of two per CU (2-stage ring); a k split adds the publish
//    and the last arriver's gather, ~5.5 us + ~1.5 us per slice beyond the second.
//  * More than one round: both kernels stream, and what differs is how much of their LAST round is empty.  Per 128 x 128 x 64 block of
//    work the 256-tile kernel costs 1.18 / 4 us and this kernel's 2-stage form 0.64 / 2 us; with eff = tiles / (rounds x slots) of each
//    (slots: G and 2 G) it is taken when 0.32 / eff128 < 0.9 x 0.295 / eff256 -- e.g. the decoder's [8 x 5121 rows] x K -> 512 dgrads:
//    322 tiles of 256 = 1.26 rounds of CUs against 1284 of 128 = 2.5 rounds of 512 slots, 82 against 96 us.  The 128-volume shapes of
//    the headline step sit at eff256 >= 0.83 and keep the 256-tile kernel (tests/test_cpu_host.py).
inline Plan128 plan128(int NA, int NB, int K, int G, bool have_ws, bool big256_ok, const GemmOptions& o) {
  Plan128 pl{0, 1, 4};
  if (!o.gemm_small) return pl;
  const int ktiles = cdiv(K, TK);
  const long long nt128 = (long long)cdiv(NA, T1) * cdiv(NB, T1);
  const long long nt256 = (long long)cdiv(NA, T2) * cdiv(NB, T2);
  if (big256_ok && nt256 > G) {
    const double eff256 = (double)nt256 / (double)(((nt256 + G - 1) / G) * G);
    const double eff128 = (double)nt128 / (double)(((nt128 + 2 * G - 1) / (2 * G)) * 2 * G);
    if (0.32 / eff128 < 0.9 * 0.295 / eff256) { pl.use = 1; pl.S = 1; pl.nst = 2; }
    return pl;
  }
  const double t256 = big256_ok ? 1.05 * ktiles + 6.5 : 1e30;
  double best = 1e30;
  for (int S = 1; S <= 4; ++S) {
    if (S > 1 && (!have_ws || ktiles / S < 8 || nt128 * S > D_WS_SLOTS || nt128 > D_WS_TILES)) break;
    if (S > 1 && last_slice_empty(ktiles, S)) continue;
    const int kper = cdiv(ktiles, S);
    const long long wg = nt128 * S;
    const double split = S > 1 ? 5.5 + 1.5 * (S - 2) : 0.0;
    const double t4 = (double)((wg + G - 1) / G) * (0.5 * kper + 4.5 + split);
    const double t2 = wg > G ? (double)((wg + 2 * G - 1) / (2 * G)) * (0.85 * kper + 5.5 + split) : 1e30;
    if (t4 < best) { best = t4; pl.S = S; pl.nst = 4; }
    if (t2 < best) { best = t2; pl.S = S; pl.nst = 2; }
  }
  pl.use = best < 0.92 * t256;
  if (!pl.use) { pl.S = 1; pl.nst = 4; }
  return pl;
}

// ---- the plan of one launch ------------------------------------------------------------------------------------------------------
enum class GemmKernel : int { Tile128 = 0, TwoStage256 = 1, Phased256 = 2, Small128d = 3 };
// where the column sums come from that ride along with a GEMM (EPI_DGELU: of the output, fc1's bias gradient; EPI_ACCUM: of dY)
enum class Colsum : int {
  None = 0,
  Fused = 1,        // inside the kernel, fp32 atomics into the [NA] vector
  FoldWs = 2,       // the kernel stores one row of partial sums per 64-row slab (ws_rows rows); octmae_colsum_accum folds them
  PassBefore = 3,   // octmae_colsum_accum over dY before the GEMM (weight gradients outside the phased 256-tile kernel)
  PassAfter = 4,    // octmae_colsum_accum over the output after the GEMM (EPI_DGELU on the 128-tile register-staged kernel)
};
constexpr int PLAN_FALLBACK = -2;   // layout / epilogue combination not built, or: the caller falls back to another entry point
struct GemmProblem {
  int NA, NB, K, lda, ldb;
  bool a_ks, b_ks;
  int epi, splitk;       // Epi (EPI_DELTA included); the k split the caller asks for (weight gradients: <= 0 = auto_wgrad_split)
  bool have_c2;          // EPI_DGELU / EPI_ACCUM: column sums are wanted
  bool have_colsum_ws;   // EPI_DGELU: a per-slab workspace for them was given
  long long slab_bytes = 0;   // EPI_ACCUM in deterministic mode: bytes of the workspace lent for the slices' slabs
};
struct GemmPlan {
  int status;            // 0, or PLAN_FALLBACK
  GemmKernel kernel;
  int tiles_a, tiles_b, cgroup, slices, ktiles_per_split, kstagger, atomic1;      // as in GemmParams; slices: k slices of the launch
  int nst;               // Small128d: ring depth (4 or 2)
  int ws_rows;           // Colsum::FoldWs: rows of partial sums the grid that runs writes (octmae_dgelu_colsum_ws_rows covers both)
  Colsum colsum;
  int grid() const { return tiles_a * tiles_b * slices; }   // workgroups (256 threads; 512 for the 256-tile kernels)
};
// cus: a callable that returns the CU count of the device; asked only where the cost model (plan128) is consulted
template <class Cus>
inline GemmPlan plan_gemm(const GemmProblem& q, const GemmVariant& v, const GemmOptions& o, Cus&& cus, bool have_ws) {
  GemmPlan pl{};
  const bool fwd = !q.a_ks && !q.b_ks, dgrad = q.a_ks && !q.b_ks, wgrad = q.a_ks && q.b_ks;
  const bool built = (fwd && q.epi >= EPI_BF16 && q.epi <= EPI_RESID) || (wgrad && q.epi == EPI_ACCUM) ||
                     (dgrad && (q.epi == EPI_BF16 || q.epi == EPI_F32 || q.epi == EPI_DGELU || q.epi == EPI_DELTA));
  if (!built) { pl.status = PLAN_FALLBACK; return pl; }
  const int ktiles = cdiv(q.K, TK);
  const bool big = !v.tile128 && fits_256(q.NA, q.NB, q.K, q.lda, q.ldb, q.a_ks, q.b_ks);
  // The small-launch kernel (forward / dgrad kinds): forced (bits 12, 13), or when the cost model says so (plan128).  Bits 8 and 14
  // bar it; a forced 256-tile main loop (bits 9, 10) means that kernel where the problem takes 256-tiles and the register-staged
  // one elsewhere, never the cost model's small launch.
  Plan128 sm{0, 1, 4};
  if (!wgrad && !v.tile128 && !v.never_small && gemm128_ok(q.NA, q.NB, q.K, q.lda, q.ldb, q.a_ks, q.b_ks)) {
    const long long nt128 = (long long)cdiv(q.NA, T1) * cdiv(q.NB, T1);
    if (v.force_small_nst)
      sm = {1, clamp_forced_split(v.forced_split ? v.forced_split : q.splitk, ktiles, nt128, have_ws), v.force_small_nst};
    else if (!v.two_stage && !v.phased_forced)
      sm = plan128(q.NA, q.NB, q.K, cus(), have_ws, big, o);
  }
  if (sm.use) {
    pl.kernel = GemmKernel::Small128d;
    pl.tiles_a = cdiv(q.NA, T1); pl.tiles_b = cdiv(q.NB, T1); pl.cgroup = pl.tiles_a;
    pl.slices = sm.S; pl.ktiles_per_split = cdiv(ktiles, sm.S); pl.nst = sm.nst;
    pl.ws_rows = 2 * pl.tiles_b;
  } else {
    if (q.epi == EPI_DELTA && !big) { pl.status = PLAN_FALLBACK; return pl; }      // only the LDS-transposing epilogues build it
    pl.kernel = !big ? GemmKernel::Tile128 : (v.phased() || q.epi == EPI_DELTA) ? GemmKernel::Phased256 : GemmKernel::TwoStage256;
    const int tile = big ? T2 : TA;
    pl.tiles_a = cdiv(q.NA, tile); pl.tiles_b = cdiv(q.NB, tile);
    pl.cgroup = big ? cgroup_for(q.epi, pl.tiles_a, pl.tiles_b, q.K, o) : pl.tiles_a;
    Split s = normalise_split(ktiles, !wgrad ? 1 : q.splitk > 0 ? q.splitk : auto_wgrad_split(pl.tiles_a * pl.tiles_b, ktiles, big ? 256 : 1024));
    // deterministic mode: as many of those slices as have a slab; the two-stage loop (A/B runs only) has no slab form and runs unsplit
    if (wgrad && o.deterministic && s.slices > 1)
      s = normalise_split(ktiles, pl.kernel == GemmKernel::TwoStage256 ? 1 : det_cap_split(s.slices, (long long)q.NA * q.NB, q.slab_bytes));
    pl.slices = s.slices; pl.ktiles_per_split = s.per;
    pl.kstagger = (big && wgrad && !o.deterministic) ? wgrad_stagger_for(ktiles, s.slices, pl.tiles_a * pl.tiles_b, o.wgrad_stagger) : 0;
    pl.atomic1 = (pl.kernel == GemmKernel::Phased256 && wgrad) ? o.wgrad_s1_atomic : 0;
    if (wgrad && o.deterministic && s.slices > 1) pl.atomic1 = ATOMIC1_SLABS;
    pl.ws_rows = 4 * pl.tiles_b;
  }
  // EPI_DGELU: fused into the LDS-transposing epilogues (256-tile kernels, small-launch kernel); the 128-tile register-staged
  // kernel is followed by the stand-alone column-sum kernel.  EPI_ACCUM: fused into the phased 256-tile kernel's main loop.
  if (q.have_c2 && q.epi == EPI_DGELU)
    pl.colsum = (pl.kernel == GemmKernel::Tile128 || (q.NA & 7) != 0) ? Colsum::PassAfter
                                                                      : q.have_colsum_ws ? Colsum::FoldWs
                                                                      : o.deterministic ? Colsum::PassAfter : Colsum::Fused;
  else if (q.have_c2 && q.epi == EPI_ACCUM)
    pl.colsum = (pl.kernel == GemmKernel::Phased256 && !o.deterministic) ? Colsum::Fused : Colsum::PassBefore;
  return pl;
}

// ---- the weight-gradient pair ----------------------------------------------------------------------------------------------------
struct PairPlan {
  int status;            // 0, or PLAN_FALLBACK: either problem does not take the 256-tile kernel (two octmae_gemm_bf16 calls instead)
  GemmKernel kernel;     // Phased256 (gemm256p_wgrad_pair_kernel) or Small128d (gemm128d_wgrad_kernel)
  int tiles_a[2], tiles_b[2], cgroup[2], slices, ktiles_per_split, kstagger, atomic1, nst;
  Colsum colsum;         // of a problem that wants its bias gradient: Fused (256) or PassBefore (128)
  int grid() const { return (tiles_a[0] * tiles_b[0] + tiles_a[1] * tiles_b[1]) * slices; }
};
// gW_i[N_i][K_i] += dY_i[M][N_i]^T X_i[M][K_i], i = 0, 1, sharing one split over the M rows
// slab_bytes: deterministic mode, the workspace lent for the slices' slabs (0: none, the pair runs unsplit there)
inline PairPlan plan_wgrad_pair(const int N[2], const int K[2], const int ldy[2], const int ldx[2], int M, int splitk,
                                const GemmOptions& o, int cus, long long slab_bytes = 0) {
  PairPlan pl{};
  for (int i = 0; i < 2; ++i)
    if (!fits_256(N[i], K[i], M, ldy[i], ldx[i], true, true)) { pl.status = PLAN_FALLBACK; return pl; }
  const int ktiles = cdiv(M, TK);
  const int nt256 = cdiv(N[0], T2) * cdiv(K[0], T2) + cdiv(N[1], T2) * cdiv(K[1], T2);
  Split s = normalise_split(ktiles, splitk > 0 ? splitk : auto_wgrad_split(nt256, ktiles, 256));   // splitk <= 0: the planner's own
  if (o.deterministic && s.slices > 1)
    s = normalise_split(ktiles, det_cap_split(s.slices, (long long)N[0] * K[0] + (long long)N[1] * K[1], slab_bytes));
  const long long nt128 = (long long)cdiv(N[0], T1) * cdiv(K[0], T1) + (long long)cdiv(N[1], T1) * cdiv(K[1], T1);
  pl.atomic1 = o.wgrad_s1_atomic;
  pl.colsum = o.deterministic ? Colsum::PassBefore : Colsum::Fused;
  // Small launches (round 6): 128 x 128 tiles when the cost model prices them faster.  Microseconds, fitted with tools/gemm_small_fit.py:
  // the 256-tile pair ~1.4 per k-tile of a slice + 0.22 per tile and slice of fp32 atomics (split) or ~10 of read-modify-write
  // (unsplit); a 128-tile workgroup (both operands through transposing LDS reads) ~0.6 per k-tile alone on its CU (4-stage ring), ~1.05
  // two per CU (2-stage), + ~8, + 0.055 per tile and slice of atomics.  Measured (profiles/r06_gemm_small_fit.txt): one volume, encoder
  // fc pair 40 -> 32 us, qkv + proj 40 -> 26, decoder 52 -> 39 and 40 -> 32; four volumes 113 -> 90 and 77 -> 64.  Short reductions only
  // (<= 96 k-tiles per launch): beyond, both kernels stream and the larger tile wins.
  // Deterministic mode keeps these prices although a split launch no longer ends in atomics there (both sides store slabs, and the fold
  // that follows costs the same for either tile size): the terms were fitted for the default mode, the mode's own have not been
  // measured, so the kernel family may differ from the default's for a split launch -- a matter of speed only.  A split 128-tile pair
  // takes the 4-stage ring there: the 2-stage ring never wins with a split (S2 <= 4, kper >= 8: one more slice on the 4-stage ring is
  // cheaper), so its slab form is not built.
  if (o.gemm_small && ktiles <= o.wgrad128_maxkt && nt128 <= 2 * cus) {
    const double c256 = 1.4 * s.per + (s.slices > 1 ? 0.22 * nt256 * s.slices : 10.0);
    double best = 1e30;
    int bS = 1, bN = 4;
    for (int S2 = 1; S2 <= 4 && S2 <= s.slices; ++S2) {        // never more slices than the caller allows (splitk = 1: no atomics)
      const int kper = cdiv(ktiles, S2);
      if (S2 > 1 && (kper < 8 || last_slice_empty(ktiles, S2))) continue;
      const long long wg = nt128 * S2;
      const double at = S2 > 1 ? 0.055 * nt128 * S2 : 0.0;
      if (wg <= cus && 0.6 * kper + 8.0 + at < best) { best = 0.6 * kper + 8.0 + at; bS = S2; bN = 4; }
      if (wg > cus && wg <= 2 * cus && !(o.deterministic && S2 > 1) && 1.05 * kper + 8.0 + at < best) { best = 1.05 * kper + 8.0 + at; bS = S2; bN = 2; }
    }
    if (best < 0.9 * c256) {
      // the bias gradients ride in the 256-tile kernel's main loop; on this path they are a pass of their own over dY
      pl.kernel = GemmKernel::Small128d; pl.colsum = Colsum::PassBefore;
      pl.slices = bS; pl.ktiles_per_split = cdiv(ktiles, bS); pl.nst = bN;
      if (o.deterministic && bS > 1) pl.atomic1 = ATOMIC1_SLABS;
      for (int i = 0; i < 2; ++i) { pl.tiles_a[i] = cdiv(N[i], T1); pl.tiles_b[i] = cdiv(K[i], T1); pl.cgroup[i] = pl.tiles_a[i]; }
      return pl;
    }
  }
  pl.kernel = GemmKernel::Phased256;
  pl.slices = s.slices; pl.ktiles_per_split = s.per;
  pl.kstagger = o.deterministic ? 0 : wgrad_stagger_for(ktiles, s.slices, nt256, o.wgrad_stagger);
  if (o.deterministic && s.slices > 1) pl.atomic1 = ATOMIC1_SLABS;
  for (int i = 0; i < 2; ++i) {
    pl.tiles_a[i] = cdiv(N[i], T2); pl.tiles_b[i] = cdiv(K[i], T2);
    pl.cgroup[i] = cgroup_for(EPI_ACCUM, pl.tiles_a[i], pl.tiles_b[i], M, o);
  }
  return pl;
}

}  // namespace octmae
