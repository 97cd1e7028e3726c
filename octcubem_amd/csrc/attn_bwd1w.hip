// Fused (single-pass) attention backward, head_dim 32, ONE WAVE PER SIMD: the main kernel of octmae_attn_bwd_fused at head_dim 32
// (decoder: 16 heads x 32, N = 5121).  Same algorithm, inputs, outputs and rounding points as attn_bwd.hip's
// attn_bwd_fused_kernel<32> (5 matrix products and 1 exp per score, no atomics, bit-reproducible), re-structured for the issue
// port: that kernel ran two waves per SIMD with two workgroup barriers per 64-query tile and spent ~880-1050 cycles per 32 x 32
// score block against ~400 of instruction issue; here
//   * a workgroup is 4 waves with 512 registers each (one per SIMD); a wave owns 128 keys of the 512-key block: dK^T / dV^T of
//     those keys (128 accumulator registers), their pre-scaled K and V fragments (64) and their K^T fragments (32) stay in
//     registers for the whole sweep over the queries;
//   * per 32-query sub-tile a wave does S, dP, exp2, dS, dV^T, dK^T for its four 32-key groups AND the dQ^T product over its
//     OWN 128 keys: its dS goes through a wave-private LDS image (no barrier: a wave's LDS operations execute in order) and
//     comes back through transposed reads as the B operand of 8 more 32x32x16 MFMAs;
//   * the four waves' dQ^T partial tiles (fp32, 4 KB each) are summed through LDS in a fixed order -- wave w sums register quad
//     w of all four, adds the workspace value of the previous key blocks (brought in by LDS-DMA a tile ahead) and stores -- one
//     tile LATER, behind the single workgroup barrier of the tile, so no wave ever waits for another's arithmetic;
//   * Q / dO / row-constant tiles arrive by LDS-DMA through a 3-deep ring two tiles ahead, retired by counted vmcnt.
// This file holds what differs from head_dim 64 (attn_bwd1w64.hip): the shapes, the pipeline prologue, which generated body and
// drains run when, the dK / dV write-out.  The rest is the shared frame, attn_bwd1w_frame.hpp.
// Reference op: backward of softmax((q k^T) scale) v, Pre-training/custom_util/video_vit.py:130-134 under autograd.
#include "attn_bwd1w.hpp"
#include "attn_bwd_tail1.hpp"
#ifndef BWD1W_TAIL_DEPTH
#define BWD1W_TAIL_DEPTH 4      // passes of rows in flight in the single-key tail (8: measured equal)
#endif
#include "../../include/octmae.h"
#define BWD1W_BODY "attn_bwd1w_body.inc"
#define BWD1W_DRAIN "attn_bwd1w_drain.inc"
#define BWD1W_SLOT_OFFSETS                                                                                                \
  [[maybe_unused]] const unsigned s_pc1 = (unsigned)(slot * 512 + 128), s_x1 = (unsigned)(slot * T::BYTES + 32 * T::ROWB); \
  [[maybe_unused]] const unsigned s_pcn = (unsigned)(slotn * 512), s_xn = (unsigned)(slotn * T::BYTES);

namespace octmae {

namespace bwd1w {

constexpr int HD = 32, NW = 4, KW = 128, NG = 4, KB = NW * KW;
constexpr int NP = 2;                                   // 1-KiB pieces of Q or dO per wave and tile
constexpr int NQT = 1, NOLDREQ = 2, NST = 2;            // a wave owns ONE 16 x 16 tile of a sub-step's dQ^T: one old value, one store
constexpr int LA = 3;                                   // tiles requested ahead of the one being computed
constexpr int NB = LA + 1;                              // Q / dO / constants ring depth
constexpr int NOLD = 3;                                 // workspace-value buffers: requested one tile before their tile, read one after
using T = Tile<HD>;                                     // 64 rows x 64 B, XOR-swizzled 16-byte chunks
constexpr int QR = 0;                                   // Q ring      [NB][4096]
constexpr int OR_ = QR + NB * T::BYTES;                 // dO ring     [NB][4096]
constexpr int CR = OR_ + NB * T::BYTES;                 // constants   [NB][2][64] f32
constexpr int IMG = CR + NB * 512;                      // dS images [2 sub-steps][512 keys][32 queries] bf16 (64-byte rows); wave w writes
                                                        //   rows 128 w .. 128 w + 127, every wave reads all rows (transposed)
constexpr int IMG_BUF = KB * 64;
constexpr int OLD = IMG + 2 * IMG_BUF;                  // workspace values   [NOLD tiles][2 sub-tiles][NW][64 lanes] f32x4
constexpr int OLD_QUAD = NW * 1024, OLD_TILE = 2 * OLD_QUAD;
constexpr int LDS = OLD + NOLD * OLD_TILE;
constexpr int STG = IMG;                                // K rows of the block [512][64 B], staged once per block for the K^T reads

using namespace bwd1w_util;

__device__ __forceinline__ int kst_off(int row, int c) { return img_off(row, c); }      // staged K rows are image rows
// wave w owns head dims 16 (w & 1) .. + 15 of queries 16 (w >> 1) .. + 15 of every sub-step's dQ^T[32 head dims][32 queries]
__device__ __forceinline__ int dq_dtile(int wid) { return wid & 1; }
__device__ __forceinline__ int dq_qtile(int wid) { return wid >> 1; }
// byte offset in OLD of wave `wid`'s quad u of buffer `buf` (the same value in both kernels, each in its own association: see the frame)
__device__ __forceinline__ int old_quad(int buf, int u, int wid) { return ((buf * 2 + u) * NW + wid) * 1024; }

#ifdef BWD1W_STAMP      // 10 intervals per sub-step
__device__ unsigned g_bwd1w_stamp[512 * 4 * 2 * 10];
constexpr int NSTAMP = 10, NSTAMP_ACC = 10;
#define BWD1W_STAMP_REGS "+s"(st_[0]), "+s"(st_[1]), "+s"(st_[2]), "+s"(st_[3]), "+s"(st_[4]), "+s"(st_[5]), "+s"(st_[6]), "+s"(st_[7]), "+s"(st_[8]), "+s"(st_[9])
#endif

}  // namespace bwd1w

__global__ __launch_bounds__(256, 1) void attn_bwd_fused1w_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ rowc, float* __restrict__ dq_ws,
                                                                  bf16_t* __restrict__ dqkv, int N, int NPAD, int H, int nkb,
                                                                  float scale, int tail_key) {
  using namespace bwd1w;
#define BWD1W_FRAME_SETUP
#include "attn_bwd1w_frame.hpp"

  for (int kb = 0; kb < nkb; ++kb) {
#define BWD1W_FRAME_KEY_BLOCK
#include "attn_bwd1w_frame.hpp"
    f32x16 dk0 = zero16, dk1 = zero16, dk2 = zero16, dk3 = zero16, dv0 = zero16, dv1 = zero16, dv2 = zero16, dv3 = zero16;
#define BWD1W_FRAME_KT
#include "attn_bwd1w_frame.hpp"

    // ---- pipeline prologue: fragments of sub-step (0, 0), S / dP of its first key group; everything the first C1 / D / reduce
    // of the loop consume without a producer is zero or is dropped (the dQ^T tile of "sub-step -1": a store outside the range)
    f32x16 lse_a, dlt_a, lse_b = zero16, dlt_b = zero16, saA, dpA, saB, dpB;
    f32x4 dqA = zero4, dqB = zero4;
    bf16x8 qrowa0, qrowa1, orowa0, orowa1, qrowb0, qrowb1, orowb0, orowb1, qTa0, qTa1, oTa0, oTa1, qTb0, qTb1, oTb0, oTb1;
    u32x4 pf0 = {0u, 0u, 0u, 0u}, pf1 = pf0, dsf0 = pf0, dsf1 = pf0;
    {
#pragma unroll
      for (int G = 0; G < 4; ++G) {
        const f32x4 a = lds_ld<f32x4>(a_const + 32 * G);
        const f32x4 d = lds_ld<f32x4>(a_const + 256 + 32 * G);
#pragma unroll
        for (int e = 0; e < 4; ++e) { lse_a[4 * G + e] = a[e]; dlt_a[4 * G + e] = d[e]; }
      }
      qrowa0 = lds_ld<bf16x8>(a_row);
      orowa0 = lds_ld<bf16x8>(a_row + (OR_ - QR));
      qrowa1 = lds_ld<bf16x8>(a_row ^ 32u);
      orowa1 = lds_ld<bf16x8>((a_row ^ 32u) + (OR_ - QR));
      qTa0 = cat4(lds_tr_ld(a_trlo), lds_tr_ld(a_trhi));
      oTa0 = cat4(lds_tr_ld(a_trlo + (OR_ - QR)), lds_tr_ld(a_trhi + (OR_ - QR)));
      qTa1 = cat4(lds_tr_ld(a_trlo + 16 * 64), lds_tr_ld(a_trhi + 16 * 64));
      oTa1 = cat4(lds_tr_ld(a_trlo + 16 * 64 + (OR_ - QR)), lds_tr_ld(a_trhi + 16 * 64 + (OR_ - QR)));
      qTb0 = qTb1 = oTb0 = oTb1 = qrowb0 = qrowb1 = orowb0 = orowb1 = __builtin_bit_cast(bf16x8, pf0);
      saA = mfma32(qrowa0, kS[0][0], lse_a);
      dpA = mfma32(orowa0, vS[0][0], dlt_a);
      saA = mfma32(qrowa1, kS[0][1], saA);
      dpA = mfma32(orowa1, vS[0][1], dpA);
      saB = zero16; dpB = zero16;
    }

#define BWD1W_FRAME_RING
#include "attn_bwd1w_frame.hpp"
    const int nloop = half_drain ? ntiles - 1 : ntiles;
    for (int t = 0; t < nloop; ++t) {
      if (t > 0) BWD1W_WAIT(t);
      BWD1W_TILE_SETUP
#include BWD1W_BODY
    }
#define BWD1W_FRAME_HALF_DRAIN
#include "attn_bwd1w_frame.hpp"
    else {      // the last tile has rows in its second half: the drain behind sub-step (ntiles - 1, 1)
      const int t = ntiles;
      BWD1W_WAIT(t);
      BWD1W_TILE_SETUP
      BWD1W_DRAIN_ADDRS
#define BWD1W_DRAIN_SLIM0
#include BWD1W_DRAIN
#undef BWD1W_DRAIN_SLIM0
#define BWD1W_DRAIN_TINY1
#include BWD1W_DRAIN
#undef BWD1W_DRAIN_TINY1
    }
    BWD1W_STAMP_FLUSH(g_bwd1w_stamp)
    // ---- dK, dV of this wave's keys (the last MFMAs into them are more than a sub-step behind; the nops keep the read-out of
    // the accumulators clear of them whatever the compiler places here)
    asm volatile("s_nop 15\n\ts_nop 15" : "+a"(dk0), "+a"(dk1), "+a"(dk2), "+a"(dk3), "+a"(dv0), "+a"(dv1), "+a"(dv2), "+a"(dv3));
    {
      const f32x16* dks[4] = {&dk0, &dk1, &dk2, &dk3};
      const f32x16* dvs[4] = {&dv0, &dv1, &dv2, &dv3};
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        bf16_t* drow = dqkv + ((size_t)b * N + key0 + wid * KW + 32 * g + r) * rs + (size_t)head * HD;
        const f32x16& dkg = *dks[g];
        const f32x16& dvg = *dvs[g];
#pragma unroll
        for (int G = 0; G < 4; ++G) {
          const u32x2 wk = {pack2bf(dkg[4 * G] * scale, dkg[4 * G + 1] * scale), pack2bf(dkg[4 * G + 2] * scale, dkg[4 * G + 3] * scale)};
          const u32x2 wv = {pack2bf(dvg[4 * G], dvg[4 * G + 1]), pack2bf(dvg[4 * G + 2], dvg[4 * G + 3])};
          *reinterpret_cast<u32x2*>(drow + (size_t)H * HD + 8 * G + 4 * h) = wk;
          *reinterpret_cast<u32x2*>(drow + (size_t)2 * H * HD + 8 * G + 4 * h) = wv;
        }
      }
    }
    // next block: its workspace read-modify-write of a row is done by the same lane as this block's (program order: a wave's
    // vector-memory operations complete in issue order), the dK / dV stores above are nobody's input; its K staging overwrites
    // the image region, which every wave has finished reading behind the loop's last barrier
  }
#define BWD1W_FRAME_TAIL
#include "attn_bwd1w_frame.hpp"
}

#ifdef BWD1W_STAMP
extern "C" int octmae_debug_bwd1w_stamps(void* host, int nbytes) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(octmae::bwd1w::g_bwd1w_stamp), (size_t)nbytes);
}
#endif

// launcher used by attn_bwd.hip's run_fused<32>
int launch_attn_bwd_fused1w(const bf16_t* qkv, const bf16_t* dout, const float* rowc, float* dq_ws, bf16_t* dqkv, int B, int N, int NPAD,
                            int H, int nkb, float scale, int tail_key, hipStream_t st) {
  return launch_bwd1w<attn_bwd_fused1w_kernel, bwd1w::LDS>(B * H, st, qkv, dout, rowc, dq_ws, dqkv, N, NPAD, H, nkb, scale, tail_key);
}
}  // namespace octmae
