// Mixup / cutmix of a fine-tune batch (timm.data.Mixup's three modes: batch, elem, pair), in place, in one launch.
//   octmae_mix_batch   x f32 [B][S] (S = C (T) H W, B even) + kind int32 [B] + lam, oml f32 [B] + box int32 [B][4]  ->  x
//                      kind 0: untouched   1: x[i] = x[i] * lam[i] + x0[j] * oml[i]   2: x[i][.., yl:yh, xl:xh] = x0[j][.., yl:yh, xl:xh]
//                      j = B - 1 - i, x0 the batch as it was before the launch
// Sample i and its partner j are one workgroup row (blockIdx.y) and every element offset e of the pair is visited by exactly one
// thread, which loads x[i][e] and x[j][e] before it stores either: no thread ever reads a value another one has replaced, so there is
// no clone of the batch (timm's elem / pair modes clone it; its batch mode flips and scales a copy) and no barrier.
//   bytes per element of a pair: mixup on one or both sides: 4 + 4 read, 4 written per side that mixes -- two passes over the batch
//                                (timm's flip / mul_ / mul_ / add_ is about nine, plus the temporary);
//                                cutmix on both sides (batch, pair mode): 4 read + 4 written per box element of either side, nothing
//                                outside the boxes is loaded or stored; kind 0 on both sides: nothing.
// Access width: 16 bytes wherever the four elements lie in range (the box's columns for cutmix) and x[i], x[j] share their phase
// against a 16-byte line ((j - i) * S % 4 == 0: always when S % 4 == 0); the ends of a row segment, of a sample and a pair out of
// phase take the scalar path.  The products of kind 1 are rounded one by one and then added, as torch's mul followed by add: the
// build's -ffp-contract=fast would fuse them (see grey() in csrc/recon.hip), the empty asm statements keep it from doing so.
// No 16-bit operand: the two builds of the library hold the same code.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

struct MixBox { int yl, yh, xl, xh; };

// the box of sample s, clamped into the image: the host refuses a box outside it (octcubem_amd/ops.py), the device never leaves x
__device__ __forceinline__ MixBox mix_box(const int* __restrict__ box, int s, int H, int W) {
  MixBox b;
  b.yl = min(max(box[4 * s + 0], 0), H);
  b.yh = min(max(box[4 * s + 1], b.yl), H);
  b.xl = min(max(box[4 * s + 2], 0), W);
  b.xh = min(max(box[4 * s + 3], b.xl), W);
  return b;
}

__device__ __forceinline__ float mix2(float a, float la, float b, float lb) {
  float pa = __fmul_rn(a, la);
  asm("" : "+v"(pa));
  float pb = __fmul_rn(b, lb);
  asm("" : "+v"(pb));
  return __fadd_rn(pa, pb);
}

// One side of a pair in the full pass: what sample d becomes at element e, given the originals (own, other).  Returns whether to store.
struct MixSide {
  int kind;
  float lam, oml;
  MixBox b;
  int HW, W;
  __device__ __forceinline__ bool in_box(int e) const {
    const int r = e % HW, y = r / W, x = r - y * W;
    return y >= b.yl && y < b.yh && x >= b.xl && x < b.xh;
  }
  template <bool BOTH_MIX>
  __device__ __forceinline__ bool apply(int e, float own, float other, float& out) const {
    if (BOTH_MIX || kind == 1) { out = mix2(own, lam, other, oml); return true; }
    if (kind == 2 && in_box(e)) { out = other; return true; }
    return false;
  }
};

// Full pass over the S elements of a pair of which at least one side mixes (kind 1).  Chunk c is the 16-byte line c of x[i]:
// elements [4c - ph, 4c - ph + 4) of the sample, ph the phase of the sample's first element.  BOTH_MIX: both sides are kind 1 (every
// pair of batch-mode mixup), the loop without the per-element questions.
template <bool BOTH_MIX>
__device__ void mix_full(float* __restrict__ xi, float* __restrict__ xj, int S, const MixSide& si, const MixSide& sj, int ph, bool vec_ok,
                         int t0, int nthreads) {
  const int nchunk = (S + ph + 3) >> 2;
  for (int c = t0; c < nchunk; c += nthreads) {
    const int e0 = 4 * c - ph;
    if (vec_ok && e0 >= 0 && e0 + 4 <= S) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xi + e0);
      const f32x4 b = *reinterpret_cast<const f32x4*>(xj + e0);
      f32x4 na, nb;
      bool wa[4], wb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float va = a[k], vb = b[k];
        wa[k] = si.template apply<BOTH_MIX>(e0 + k, a[k], b[k], va);
        wb[k] = sj.template apply<BOTH_MIX>(e0 + k, b[k], a[k], vb);
        na[k] = va; nb[k] = vb;
      }
      if (wa[0] && wa[1] && wa[2] && wa[3]) *reinterpret_cast<f32x4*>(xi + e0) = na;
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (wa[k]) xi[e0 + k] = na[k];
      }
      if (wb[0] && wb[1] && wb[2] && wb[3]) *reinterpret_cast<f32x4*>(xj + e0) = nb;
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (wb[k]) xj[e0 + k] = nb[k];
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e < 0 || e >= S) continue;
        const float a = xi[e], b = xj[e];
        float v;
        if (si.template apply<BOTH_MIX>(e, a, b, v)) xi[e] = v;
        if (sj.template apply<BOTH_MIX>(e, b, a, v)) xj[e] = v;
      }
    }
  }
}

// Box pass: xd[e] = xs0[e] for the elements of box P (over the last two dimensions, in every one of the S / (H W) planes).
//   EXCHANGE: where e also lies in box Q, xs[e] = xd0[e] (both sides of a pair cut: the overlap of the two boxes swaps);
//   otherwise the elements inside Q are SKIPPED (they were exchanged by the partner's pass).  Q may be empty.
// The two passes of a pair touch disjoint elements (P, and Q \ P), so they need no order.
template <bool EXCHANGE>
__device__ void mix_boxes(float* __restrict__ xd, float* __restrict__ xs, int S, int H, int W, MixBox P, MixBox Q, int phd, bool vec_ok,
                          int t0, int nthreads) {
  const int bh = P.yh - P.yl, bw = P.xh - P.xl;
  if (bh <= 0 || bw <= 0) return;
  const int HW = H * W;
  const unsigned rows = (unsigned)(S / HW) * bh;
  const unsigned nchunk = (bw + 3) / 4 + 1;     // 16-byte lines a row segment can touch, whatever its phase
  // rows * bw <= S <= 2^30, so rows * nchunk <= S / 4 + 2 S and w + nthreads stay below 2^32: unsigned 32-bit divisions
  for (unsigned w = t0; w < rows * nchunk; w += nthreads) {
    const unsigned r = w / nchunk;
    const int c = (int)(w - r * nchunk);
    const unsigned plane = r / bh;
    const int y = P.yl + (int)(r - plane * bh);
    const int o0 = (int)plane * HW + y * W + P.xl, o1 = o0 + bw;     // the row segment [o0, o1) of the sample
    const int e0 = o0 - ((o0 + phd) & 3) + 4 * c;
    const bool qrow = y >= Q.yl && y < Q.yh;
    // the columns of Q on this row, as element offsets
    const int q0 = o0 - P.xl + Q.xl, q1 = qrow ? o0 - P.xl + Q.xh : q0;
    if (e0 >= o1) continue;
    if (vec_ok && e0 >= o0 && e0 + 4 <= o1) {
      const bool all_q = e0 >= q0 && e0 + 4 <= q1, none_q = e0 + 4 <= q0 || e0 >= q1;
      if (none_q) {
        *reinterpret_cast<f32x4*>(xd + e0) = *reinterpret_cast<const f32x4*>(xs + e0);
        continue;
      }
      if (all_q) {
        if (EXCHANGE) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(xs + e0);
          const f32x4 a = *reinterpret_cast<const f32x4*>(xd + e0);
          *reinterpret_cast<f32x4*>(xd + e0) = b;
          *reinterpret_cast<f32x4*>(xs + e0) = a;
        }
        continue;
      }
    }
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k;
      if (e < o0 || e >= o1) continue;
      const bool inq = e >= q0 && e < q1;
      if (!inq) xd[e] = xs[e];
      else if (EXCHANGE) {
        const float b = xs[e], a = xd[e];
        xd[e] = b;
        xs[e] = a;
      }
    }
  }
}

__global__ __launch_bounds__(256) void mix_batch_kernel(float* __restrict__ x, const int* __restrict__ kind,
                                                        const float* __restrict__ lam, const float* __restrict__ oml,
                                                        const int* __restrict__ box, int B, long long S, int H, int W) {
  const int i = blockIdx.y, j = B - 1 - i;
  const int ki = kind[i], kj = kind[j];
  const bool mi = ki == 1, mj = kj == 1, ci = ki == 2, cj = kj == 2;
  if (!(mi || mj || ci || cj)) return;
  float* xi = x + (size_t)i * (size_t)S;
  float* xj = x + (size_t)j * (size_t)S;
  const int phi = (int)((reinterpret_cast<uintptr_t>(xi) >> 2) & 3), phj = (int)((reinterpret_cast<uintptr_t>(xj) >> 2) & 3);
  const bool vec_ok = phi == phj;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;      // at most 4096 x 256
  const MixBox bi = ci ? mix_box(box, i, H, W) : MixBox{0, 0, 0, 0};
  const MixBox bj = cj ? mix_box(box, j, H, W) : MixBox{0, 0, 0, 0};
  if (mi || mj) {
    const MixSide si{ki, lam[i], oml[i], bi, H * W, W}, sj{kj, lam[j], oml[j], bj, H * W, W};
    if (mi && mj) mix_full<true>(xi, xj, (int)S, si, sj, phi, vec_ok, t0, nthreads);
    else mix_full<false>(xi, xj, (int)S, si, sj, phi, vec_ok, t0, nthreads);
    return;
  }
  if (ci) mix_boxes<true>(xi, xj, (int)S, H, W, bi, bj, phi, vec_ok, t0, nthreads);
  if (cj) mix_boxes<false>(xj, xi, (int)S, H, W, bj, bi, phj, vec_ok, t0, nthreads);
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_mix_batch(float* x, const int* kind, const float* lam, const float* oml, const int* box, int B, long long S,
                                int H, int W, void* stream) {
  OCTMAE_CHECK_ARG(x && kind && lam && oml && box);
  OCTMAE_CHECK_ARG(B > 0 && B % 2 == 0 && S > 0 && H > 0 && W > 0);
  OCTMAE_CHECK_ARG((long long)H * W <= S && S % ((long long)H * W) == 0);
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0);
  if (S > (1LL << 30) || B / 2 > 65535) return -2;      // element offsets and line counts of a sample are 32-bit; the pair is the grid's y
  // memory-bound: at most ~4096 workgroups in all, the rest of a pair's 16-byte lines by grid stride
  const int pairs = B / 2;
  long long blocks = ((S + 3) / 4 + 1 + 255) / 256;
  const long long cap = (4096 + pairs - 1) / pairs;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(mix_batch_kernel, dim3((unsigned)blocks, (unsigned)pairs), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     kind, lam, oml, box, B, S, H, W);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
