// Pieces shared by the one-wave-per-SIMD attention backward kernels (attn_bwd1w.hip: head_dim 32, attn_bwd1w64.hip: head_dim 64):
// helpers, the ablation and stamp macros, the tile loop's macros and the launcher body.  The text of the kernel function the two
// share is attn_bwd1w_frame.hpp.
#pragma once
#include "attn_tile.hpp"

namespace octmae {
namespace bwd1w_util {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return mfma16x16(a, b, c); }

template <int CNT>
__device__ __forceinline__ void wait_vm() {
  static_assert(CNT >= 0 && CNT < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt((CNT & 15) | ((CNT >> 4) << 14) | (7 << 4) | (15 << 8));
}
__device__ __forceinline__ void lds_dma16(unsigned m0v, unsigned voff, i32x4_t rsrc) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(m0v), "v"(voff), "s"(rsrc) : "memory", "m0");
}
// the workspace traffic (fp32 dQ partial sums, read-modify-written once per key block) with its own cache policy switches:
// BWD1W_WS_ST_AUX = aux bits of the store (0 default, 2 = nt), -DBWD1W_WS_LD_NT = nt on the LDS-DMA loads of the old values
#ifndef BWD1W_WS_ST_AUX
#define BWD1W_WS_ST_AUX 0
#endif
// timing-only experiment (-DBWD1W_ST_SMALL): every write-out store lands in the first 64 KB of the (batch, head)'s workspace
#ifdef BWD1W_ST_SMALL
#define BWD1W_RVO(x) ((x) & 0xFFFFu)
#else
#define BWD1W_RVO(x) (x)
#endif
__device__ __forceinline__ void lds_dma16_ws(unsigned m0v, unsigned voff, i32x4_t rsrc) {
#ifdef BWD1W_WS_LD_NT
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, 0 offen nt lds" ::"s"(m0v), "v"(voff), "s"(rsrc) : "memory", "m0");
#else
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(m0v), "v"(voff), "s"(rsrc) : "memory", "m0");
#endif
}
__device__ __forceinline__ void lds_dma4(unsigned m0v, unsigned voff, i32x4_t rsrc) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dword %1, %2, 0 offen lds" ::"s"(m0v), "v"(voff), "s"(rsrc) : "memory", "m0");
}
__device__ __forceinline__ i32x4_t make_rsrc(const void* base, unsigned bytes) {
  const unsigned long long a = (unsigned long long)base;
  i32x4_t r = {(int)(unsigned)a, (int)(unsigned)(a >> 32), (int)bytes, 0x00020000};
  r[0] = __builtin_amdgcn_readfirstlane(r[0]);
  r[1] = __builtin_amdgcn_readfirstlane(r[1]);
  r[2] = __builtin_amdgcn_readfirstlane(r[2]);
  r[3] = __builtin_amdgcn_readfirstlane(r[3]);
  return r;
}
// 8-byte chunk c8 (4 bf16) of row `row` of a [rows][64 B] image: ds_write_b64 by 16 consecutive rows and the transposed reads of
// 4 consecutive rows (one aligned 256-byte line) are both conflict-free for any within-row permutation that separates the 8
// even (odd) rows of a 16-row run
__device__ __forceinline__ int img_off(int row, int c8) { return row * 64 + ((c8 ^ ((row >> 1) & 7)) << 3); }
constexpr int IMG_KSTEP = 32 * 64;      // bytes of the 32 image rows (keys) of one k-step of the dQ^T product

// Timing-only ablations (-DABL_NO_..., make abl: results are wrong, the instruction stream is otherwise unchanged).  The generated
// bodies wrap each statement a switch removes in the macro of that switch; variadic, because the statements contain commas.
#define BWD1W_KEEP(...) __VA_ARGS__
#define BWD1W_DROP(...)
#ifdef ABL_NO_WR                        // the dS image writes
#define ABL_WR BWD1W_DROP
#else
#define ABL_WR BWD1W_KEEP
#endif
#ifdef ABL_NO_WP                        // the whole write-out: old value, add, store
#define ABL_WP BWD1W_DROP
#else
#define ABL_WP BWD1W_KEEP
#endif
#if defined(ABL_NO_WP) || defined(ABL_NO_RST)      // the write-out's store alone
#define ABL_RST BWD1W_DROP
#else
#define ABL_RST BWD1W_KEEP
#endif
#ifdef ABL_NO_EXP
#define ABL_EXP BWD1W_DROP
#else
#define ABL_EXP BWD1W_KEEP
#endif
#ifdef ABL_NO_ACC                       // the dV^T / dK^T MFMAs
#define ABL_ACC BWD1W_DROP
#else
#define ABL_ACC BWD1W_KEEP
#endif
#ifdef ABL_NO_MD                        // the dQ^T product and its image reads
#define ABL_MD BWD1W_DROP
#else
#define ABL_MD BWD1W_KEEP
#endif

// dV^T / dK^T accumulate in the ACCUMULATOR half of the register file (128 of this wave's 512 registers), where only MFMAs touch
// them; the MFMAs whose results the vector ALU consumes (S, dP, dQ^T) are the compiler's builtins with VGPR destinations
// (-mllvm -amdgpu-mfma-vgpr-form, see the Makefile).  One function cannot have both forms from builtins, hence the asm.  Hazards
// (the compiler pads nothing inside asm): the A / B operands are written by v_cvt_pk at least two instructions earlier (the
// generator pins their last producer), the accumulate chain needs no wait states, and the read-out after the loop sits behind
// explicit s_nops.
#define MFMA_ACC(acc, a, b) asm volatile(OCTMAE_MFMA32_ASM " %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
// The lane id, computed where it is asked for (volatile: not merged with other copies, not hoisted): code behind the tile loop
// that needs per-lane addresses derives them from this instead of keeping them -- or the lane id -- in registers across the loop.
__device__ __forceinline__ int lane_id_fresh() {
  int x;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x));
  return x;
}
// end of a sub-step: this wave's dS image rows are written (LDS operations complete in order: at most the N reads issued after
// the last image write may still be pending), then the workgroup barrier
#ifdef ABL_NO_BARRIER
#define SUBSTEP_END(N) __builtin_amdgcn_s_waitcnt(0xC07F | 0)
#else
#define SUBSTEP_END(N)                                            \
  do {                                                            \
    __builtin_amdgcn_s_waitcnt(0xC07F | ((N) << 8));              \
    __builtin_amdgcn_s_barrier();                                 \
  } while (0)
#endif

// ---- diagnostic build (-DBWD1W_STAMP, make stamp): s_memtime at the start and the middle of every group-step, before the
// end-of-sub-step wait and behind the barrier (STAMP(k), placed by the generator); per-wave sums of the NSTAMP intervals of each
// sub-step in rows of NSTAMP_ACC counters (tools/attn_bwd1w_stamps.py).  The stamps go to a buffer of their own and no output depends
// on them.  The kernel's file provides NSTAMP, NSTAMP_ACC and BWD1W_STAMP_REGS (the "+s" operands st_[0] .. st_[NSTAMP - 1]).
#ifdef BWD1W_STAMP
#define STAMP(k) asm volatile("s_memtime %0" : "=s"(st_[k]))
#define STAMP_ACCUM(s)                                                                                                   \
  do {                                                                                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" : BWD1W_STAMP_REGS);                                                             \
    _Pragma("unroll") for (int k_ = 0; k_ < NSTAMP - 1; ++k_) acc_[s][k_] += (unsigned)st_[k_ + 1] - (unsigned)st_[k_]; \
    acc_[s][NSTAMP - 1] += (unsigned)st_[0] - last_;                                                                     \
    last_ = (unsigned)st_[NSTAMP - 1];                                                                                   \
  } while (0)
#define BWD1W_STAMP_BEGIN                                            \
  unsigned long long st_[NSTAMP];                                    \
  unsigned acc_[2][NSTAMP_ACC] = {};                                 \
  unsigned last_ = 0;                                                \
  STAMP(NSTAMP - 1);                                                 \
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(st_[NSTAMP - 1]));      \
  last_ = (unsigned)st_[NSTAMP - 1];
#define BWD1W_STAMP_FLUSH(buf)                        \
  if (kb == 1 && lane == 0 && blockIdx.x < 512)       \
    for (int s_ = 0; s_ < 2; ++s_)                    \
      for (int k_ = 0; k_ < NSTAMP_ACC; ++k_) buf[((blockIdx.x * 4 + wid) * 2 + s_) * NSTAMP_ACC + k_] = acc_[s_][k_];
#else
#define STAMP(k)
#define STAMP_ACCUM(s)
#define BWD1W_STAMP_BEGIN
#define BWD1W_STAMP_FLUSH(buf)
#endif

// ---- the tile loop's shared text (attn_bwd1w_frame.hpp declares what these name)
// per-iteration scalars (ring slots, write-out offsets) and the request of tile t + 3 / the workspace values of tile t + 1.
// BWD1W_SLOT_OFFSETS, of the kernel's file: the offsets s_x0 / s_x1 / s_xn (Q ring: sub-tiles of tile t, tile t + 1) and s_pc1 / s_pcn
// (constants ring) its generated body uses -- per file, because the scalar register allocation of the stamp builds follows the order
// of these declarations and the two kernels were recorded with different ones.
#define BWD1W_TILE_SETUP                                                                                                        \
  [[maybe_unused]] const int slot = t & (NB - 1), slotn = (t + 1) & (NB - 1);                                                   \
  BWD1W_SLOT_OFFSETS                                                                                                            \
  [[maybe_unused]] const unsigned s_oldr = (unsigned)(((t + 2) % NOLD) * OLD_TILE);                                             \
  [[maybe_unused]] const unsigned s_redoff0 = t > 0 ? (unsigned)(t - 1) * WS_TILE : DROP;                                       \
  [[maybe_unused]] const unsigned s_redoff1 = t > 0 ? (unsigned)(t - 1) * WS_TILE + WS_SUB : DROP;                              \
  [[maybe_unused]] auto issue_tile = [&]() {                                                                                    \
    const int tn = t + LA;                                                                                                      \
    issue(BWD1W_DMA_TILE(tn), tn < ntiles ? tn : ntiles, tn & (NB - 1));                                                        \
    oldreq(t + 1, (t + 1) % NOLD, BWD1W_OLD_BASE);                                                                              \
  };
#ifdef ABL_NO_TILE_DMA                  // every request of the loop fetches tile 0
#define BWD1W_DMA_TILE(tn) 0
#else
#define BWD1W_DMA_TILE(tn) ((tn) < ntiles ? (tn) : (tn) - ntiles)
#endif
#ifdef ABL_NO_OLDREQ                    // the loop's workspace-value requests fall outside the descriptor
#define BWD1W_OLD_BASE DROP
#else
#define BWD1W_OLD_BASE oldbase
#endif
#define BWD1W_DRAIN_ADDRS \
  [[maybe_unused]] const unsigned a_imglo = opaque(o_imglo), a_imghi = opaque(o_imghi), a_old = opaque(o_old), wsoff = opaque(o_wsoff);
// The wait at the top of iteration t retires the vector-memory operations of iteration t - 2 and earlier (VM_ITER per iteration:
// its stores, its tile request, its workspace-value requests) -- except that iteration's LAST operations, the write-out stores of
// its sub-step 1: nothing issued behind them is needed yet, and vmcnt retires in order, so letting those stores (HBM write latency
// under load) stay pending costs no correctness and gives every store one more iteration to complete (BWD1W_VMWAIT_EXTRA = NST / 2).
// t = 1 keeps the plain count: the prologue's last request, the workspace values of tile 0, is read in that iteration.
#ifndef BWD1W_VMWAIT_EXTRA
#define BWD1W_VMWAIT_EXTRA (NST / 2)
#endif
#define BWD1W_WAIT(t_) do { if ((t_) > 1) wait_vm<VM_ITER + BWD1W_VMWAIT_EXTRA>(); else wait_vm<VM_ITER>(); } while (0)

}  // namespace bwd1w_util

// launcher body of both kernels
template <auto KERNEL, int LDS_BYTES, class... A>
int launch_bwd1w(int nblocks, hipStream_t st, A... args) {
  static DynLdsOnce once;
  if (int rc = once.ensure(reinterpret_cast<const void*>(KERNEL), LDS_BYTES)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(nblocks), dim3(256), LDS_BYTES, st, args...);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
}  // namespace octmae
