// Fused (single-pass) attention backward, head_dim 64, ONE WAVE PER SIMD: the main kernel of octmae_attn_bwd_fused at head_dim 64
// (encoder: 16 heads x 64, N = 1281).  Same algorithm, inputs, outputs and rounding points as attn_bwd.hip's
// attn_bwd_fused_kernel<64>; the structure is attn_bwd1w.hip's (head_dim 32) with the shapes of head_dim 64:
//   * a workgroup is 4 waves with 512 registers each; a wave owns 64 keys (two 32-key groups) of the 256-key block: dK^T / dV^T
//     of those keys (128 accumulator registers), their pre-scaled K and V fragments (64) and the K^T fragments of ITS 16 head
//     dims over all 256 keys (32) stay in registers for the whole sweep over the queries;
//   * per 32-query sub-tile a wave does S, dP (4 k-steps each), exp2, dS, dV^T, dK^T (2 head-dim blocks x 2 k-steps each) for
//     its two key groups -- 16 32x32x16 MFMAs per group for 16 exp2 per lane, twice the matrix work per exp of head_dim 32 --
//     and writes dS into the workgroup's [256 keys][32 queries] image;
//   * one sub-step later (behind the workgroup barrier) it multiplies K^T of its 16 head dims with the whole image: its
//     16 x 32 slice of dQ^T, as two 16 x 16 tiles over 8 k-steps of 32 keys -- complete sums, nothing crosses waves in fp32 --
//     adds the workspace value of the previous key blocks (brought in by LDS-DMA a tile ahead) and stores, another sub-step
//     later;
//   * Q / dO / row-constant tiles arrive by LDS-DMA through a 4-deep ring, retired by counted vmcnt.
// The body of the tile loop is generated (tools/gen_attn_bwd1w.py, sub_step64): it fixes the instruction order.  This file holds
// what differs from head_dim 32: the shapes, the pipeline prologue, which generated body and drain run when, the dK / dV
// write-out.  The rest is the shared frame, attn_bwd1w_frame.hpp.
// Reference op: backward of softmax((q k^T) scale) v, Pre-training/custom_util/video_vit.py:130-134 under autograd.
#include "attn_bwd1w.hpp"
#include "attn_bwd_tail1.hpp"
#ifndef BWD1W_TAIL_DEPTH
#define BWD1W_TAIL_DEPTH 4      // passes of rows in flight in the single-key tail (8: measured equal)
#endif
#include "../../include/octmae.h"
#define BWD1W_BODY "attn_bwd1w_body_hd64.inc"
#define BWD1W_DRAIN "attn_bwd1w_drain_hd64.inc"
#define BWD1W_SLOT_OFFSETS                                                                                                                \
  [[maybe_unused]] const unsigned s_x0 = (unsigned)(slot * T::BYTES), s_x1 = s_x0 + 32 * T::ROWB, s_xn = (unsigned)(slotn * T::BYTES); \
  [[maybe_unused]] const unsigned s_pc1 = (unsigned)(slot * 512 + 128), s_pcn = (unsigned)(slotn * 512);
#ifdef ABL_TILED_WS             // experiment of this file alone: the workspace as 1-KiB quads in lane order (results are wrong)
#define BWD1W_WSOFF (unsigned)(wid * 1024 + lane * 16)
#endif

namespace octmae {

namespace bwd1w64 {

constexpr int HD = 64, NW = 4, KW = 64, NG = 2, KB = NW * KW;
constexpr int NP = 4;                                   // 1-KiB pieces of Q or dO per wave and tile
constexpr int NQT = 2, NOLDREQ = 4, NST = 4;            // a wave owns TWO 16 x 16 tiles of a sub-step's dQ^T: two old values, two stores
constexpr int LA = 3;                                   // tiles requested ahead of the one being computed
constexpr int NB = LA + 1;                              // Q / dO / constants ring depth
constexpr int NOLD = 3;                                 // workspace-value buffers: requested one tile before their tile, read one after
using T = Tile<HD>;                                     // 64 rows x 128 B, XOR-swizzled 16-byte chunks
constexpr int QR = 0;                                   // Q ring      [NB][8192]
constexpr int OR_ = QR + NB * T::BYTES;                 // dO ring     [NB][8192]
constexpr int CR = OR_ + NB * T::BYTES;                 // constants   [NB][2][64] f32
constexpr int IMG = CR + NB * 512;                      // dS images [2 sub-steps][256 keys][32 queries] bf16 (64-byte rows); wave w
constexpr int IMG_BUF = KB * 64;                        //   writes rows 64 w .. 64 w + 63, every wave reads all rows (transposed)
constexpr int OLD = IMG + 2 * IMG_BUF;                  // workspace values   [NOLD tiles][2 sub-tiles][2 query tiles][NW][64 lanes] f32x4
constexpr int OLD_QUAD = NW * 1024, OLD_TILE = 2 * 2 * OLD_QUAD;
constexpr int LDS = OLD + NOLD * OLD_TILE;
constexpr int STG = IMG;                                // K rows of the block [256][128 B], staged once per block for the K^T reads

using namespace bwd1w_util;

// 8-byte chunk c (of 16) of staged K row `row` (128-byte rows): conflict-free transposed reads of rows {0..3, 8..11} /
// {4..7, 12..15} (attn_bwd.hip, BwdCfg<64>::kst_off)
__device__ __forceinline__ int kst_off(int row, int c) {
  const int sw = (row & 1) | (((row >> 2) & 1) << 1) | (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 3);
  return row * 128 + ((c ^ sw) << 3);
}
// wave w owns head dims 16 w .. 16 w + 15 of every sub-step's dQ^T[64 head dims][32 queries] as two 16 x 16 tiles (queries 0..15, 16..31)
__device__ __forceinline__ int dq_dtile(int wid) { return wid; }
__device__ __forceinline__ int dq_qtile(int) { return 0; }
// byte offset in OLD of wave `wid`'s quad u of buffer `buf` (the same value in both kernels, each in its own association: see the frame)
__device__ __forceinline__ int old_quad(int buf, int u, int wid) { return buf * OLD_TILE + (u * NW + wid) * 1024; }

#ifdef BWD1W_STAMP      // 6 intervals per sub-step; [6]: the vmcnt wait at the top of the tile (sub-step 0 only); [7]: whole-kernel ticks
__device__ unsigned g_bwd1w64_stamp[512 * 4 * 2 * 8];
constexpr int NSTAMP = 6, NSTAMP_ACC = 8;
#define BWD1W_STAMP_REGS "+s"(st_[0]), "+s"(st_[1]), "+s"(st_[2]), "+s"(st_[3]), "+s"(st_[4]), "+s"(st_[5])
#endif

}  // namespace bwd1w64

__global__ __launch_bounds__(256, 1) void attn_bwd_fused1w64_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                    const float* __restrict__ rowc, float* __restrict__ dq_ws,
                                                                    bf16_t* __restrict__ dqkv, int N, int NPAD, int H, int nkb,
                                                                    float scale, int tail_key) {
  using namespace bwd1w64;
#define BWD1W_FRAME_SETUP
#include "attn_bwd1w_frame.hpp"

#ifdef BWD1W_STAMP
  unsigned long long k0_, r0_;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(k0_), "=s"(r0_));
#endif
  for (int kb = 0; kb < nkb; ++kb) {
#define BWD1W_FRAME_KEY_BLOCK
#include "attn_bwd1w_frame.hpp"
    // dk{g}{d} / dv{g}{d}: key group g, head dims 32 d .. 32 d + 31
    f32x16 dk00 = zero16, dk01 = zero16, dk10 = zero16, dk11 = zero16, dv00 = zero16, dv01 = zero16, dv10 = zero16, dv11 = zero16;
#define BWD1W_FRAME_KT
#include "attn_bwd1w_frame.hpp"

    // ---- pipeline prologue: fragments of sub-step (0, 0), S / dP of its first key group; everything the first C1 / D / write-out
    // of the loop consume without a producer is zero or is dropped (the dQ^T tiles of "sub-steps -2, -1": stores outside the range)
    f32x16 lse_t, dlt_t, saA, dpA, saB = zero16, dpB = zero16;
    f32x4 dqA0 = zero4, dqA1 = zero4, dqB0 = zero4, dqB1 = zero4;
    bf16x8 qrow0, qrow1, qrow2, qrow3, orow0, orow1, orow2, orow3, qT0d0, qT0d1, oT0d0, oT0d1, qT1d0, qT1d1, oT1d0, oT1d1;
    u32x4 pf0 = {0u, 0u, 0u, 0u}, pf1 = pf0, dsf0 = pf0, dsf1 = pf0;
    {
#pragma unroll
      for (int G = 0; G < 4; ++G) {
        const f32x4 a = lds_ld<f32x4>(a_const + 32 * G);
        const f32x4 d = lds_ld<f32x4>(a_const + 256 + 32 * G);
#pragma unroll
        for (int e = 0; e < 4; ++e) { lse_t[4 * G + e] = a[e]; dlt_t[4 * G + e] = d[e]; }
      }
      qrow0 = lds_ld<bf16x8>(a_row);
      orow0 = lds_ld<bf16x8>(a_row + (OR_ - QR));
      qrow1 = lds_ld<bf16x8>(a_row ^ 32u);
      orow1 = lds_ld<bf16x8>((a_row ^ 32u) + (OR_ - QR));
      qrow2 = lds_ld<bf16x8>(a_row ^ 64u);
      orow2 = lds_ld<bf16x8>((a_row ^ 64u) + (OR_ - QR));
      qrow3 = lds_ld<bf16x8>(a_row ^ 96u);
      orow3 = lds_ld<bf16x8>((a_row ^ 96u) + (OR_ - QR));
      qT0d0 = cat4(lds_tr_ld(a_trlo), lds_tr_ld(a_trhi));
      oT0d0 = cat4(lds_tr_ld(a_trlo + (OR_ - QR)), lds_tr_ld(a_trhi + (OR_ - QR)));
      qT0d1 = cat4(lds_tr_ld(a_trlo ^ 64u), lds_tr_ld(a_trhi ^ 64u));
      oT0d1 = cat4(lds_tr_ld((a_trlo ^ 64u) + (OR_ - QR)), lds_tr_ld((a_trhi ^ 64u) + (OR_ - QR)));
      qT1d0 = qT1d1 = oT1d0 = oT1d1 = __builtin_bit_cast(bf16x8, pf0);
      saA = mfma32(qrow0, kS[0][0], lse_t);
      dpA = mfma32(orow0, vS[0][0], dlt_t);
      saA = mfma32(qrow1, kS[0][1], saA);
      dpA = mfma32(orow1, vS[0][1], dpA);
      saA = mfma32(qrow2, kS[0][2], saA);
      dpA = mfma32(orow2, vS[0][2], dpA);
      saA = mfma32(qrow3, kS[0][3], saA);
      dpA = mfma32(orow3, vS[0][3], dpA);
    }

#define BWD1W_FRAME_RING
#include "attn_bwd1w_frame.hpp"
#ifdef BWD1W_STAMP
    unsigned long long sw_[2];
#endif
    // (the drain code runs only for lengths whose last tile has no row in its second half -- every length of this model; other
    // lengths drain through two padding iterations in full: a second copy of the drain code costs this kernel register spills)
    const int nloop = half_drain ? ntiles - 1 : ntiles + 1;
    for (int t = 0; t < nloop; ++t) {
#ifdef BWD1W_STAMP
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(sw_[0]));
#endif
      if (t > 0) BWD1W_WAIT(t);
#ifdef BWD1W_STAMP
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(sw_[1]));
      acc_[0][6] += (unsigned)sw_[1] - (unsigned)sw_[0];
#endif
      BWD1W_TILE_SETUP
#include BWD1W_BODY
    }
#define BWD1W_FRAME_HALF_DRAIN
#include "attn_bwd1w_frame.hpp"
    BWD1W_STAMP_FLUSH(g_bwd1w64_stamp)
    // ---- dK, dV of this wave's keys (the last MFMAs into them are more than a sub-step behind; the nops keep the read-out of
    // the accumulators clear of them whatever the compiler places here)
    asm volatile("s_nop 15\n\ts_nop 15" : "+a"(dk00), "+a"(dk01), "+a"(dk10), "+a"(dk11), "+a"(dv00), "+a"(dv01), "+a"(dv10), "+a"(dv11));
#ifdef ABL_NO_EPI               // experiment of this file alone: no dK / dV write-out
    if (N < 0)
#endif
    {
      // through a wave-private [64 keys][128 B] LDS image (the dS image region: free behind the loop's last barrier), so that a
      // store instruction writes 8 whole 128-byte rows of dK (dV) instead of 8 bytes per lane on 32 rows.  8-byte slots XORed
      // with the low 4 row bits: the 16 lanes of a ds_write_b64 group (16 consecutive rows, one slot) cover all banks.
      const f32x16* dks[2][2] = {{&dk00, &dk01}, {&dk10, &dk11}};
      const f32x16* dvs[2][2] = {{&dv00, &dv01}, {&dv10, &dv11}};
      // (addresses derived from an opaque copy of the lane id: computed here, once per key block, instead of living in registers
      // across the tile loop)
      const int le = (int)opaque((unsigned)lane);
      const int re = le & 31, he = le >> 5;
      char* stg = smem + IMG + wid * (KW * 128);
      bf16_t* dbase = dqkv + ((size_t)b * N + key0 + wid * KW) * rs + (size_t)head * HD;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const f32x16& acc = which ? *dvs[g][d] : *dks[g][d];
            const float sc = which ? 1.0f : scale;
            const int row = 32 * g + re;
#pragma unroll
            for (int G = 0; G < 4; ++G) {
              const u32x2 w = {pack2bf(acc[4 * G] * sc, acc[4 * G + 1] * sc), pack2bf(acc[4 * G + 2] * sc, acc[4 * G + 3] * sc)};
              *reinterpret_cast<u32x2*>(stg + row * 128 + (((8 * d + 2 * G + he) ^ (row & 15)) << 3)) = w;
            }
          }
#pragma unroll
        for (int i = 0; i < KW / 8; ++i) {
          const int row = 8 * i + (le >> 3), j = le & 7, x = row & 15;
          const u32x4 v = *reinterpret_cast<const u32x4*>(stg + row * 128 + ((j ^ (x >> 1)) << 4));
          const u32x4 o = (x & 1) ? u32x4{v[2], v[3], v[0], v[1]} : v;
          *reinterpret_cast<u32x4*>(dbase + (size_t)row * rs + (size_t)(1 + which) * H * HD + 8 * j) = o;
        }
      }
    }
    // the next block's K staging overwrites the image region: every wave is done reading its part of it
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    // next block: its workspace read-modify-write of a row is done by the same lane as this block's (program order: a wave's
    // vector-memory operations complete in issue order); the dK / dV stores above are nobody's input
  }
#define BWD1W_FRAME_TAIL
#include "attn_bwd1w_frame.hpp"
#ifdef BWD1W_STAMP
  {
    unsigned long long k1_, r1_;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(k1_), "=s"(r1_));
    if (lane == 0 && blockIdx.x < 512) {      // whole-kernel shader-clock ticks and 100 MHz ticks of this wave
      g_bwd1w64_stamp[((blockIdx.x * 4 + wid) * 2 + 0) * 8 + 7] = (unsigned)(k1_ - k0_);
      g_bwd1w64_stamp[((blockIdx.x * 4 + wid) * 2 + 1) * 8 + 7] = (unsigned)(r1_ - r0_);
    }
  }
#endif
}

#ifdef BWD1W_STAMP
extern "C" int octmae_debug_bwd1w64_stamps(void* host, int nbytes) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(octmae::bwd1w64::g_bwd1w64_stamp), (size_t)nbytes);
}
#endif

// launcher used by attn_bwd.hip's run_fused<64>
int launch_attn_bwd_fused1w64(const bf16_t* qkv, const bf16_t* dout, const float* rowc, float* dq_ws, bf16_t* dqkv, int B, int N, int NPAD,
                              int H, int nkb, float scale, int tail_key, hipStream_t st) {
  return launch_bwd1w<attn_bwd_fused1w64_kernel, bwd1w64::LDS>(B * H, st, qkv, dout, rowc, dq_ws, dqkv, N, NPAD, H, nkb, scale, tail_key);
}

}  // namespace octmae
