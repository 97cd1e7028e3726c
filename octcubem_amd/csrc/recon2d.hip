// The 2-D half of the validation pass: the panels of the reference's get_visible_images_2d (Pre-training/custom_util/misc.py:1134-1223)
// for any channel count and any affine grey scale, and its border blanking find_and_convert_large_white_region (:1438-1484).
//   octmae_mae_compose_nc  pred f32 [B][L][PD] (any batch stride) + imgs f32 [B][C][T][H][W] + mask f32 [B][L] -> uint8 [B][4][Tp][H][W][C]
//   octmae_white_border    imgs f32 [B][T][H][W] blanked in place, region uint8 [B][T][H][W]
// No 16-bit operand: the two builds of the library hold the same code.  The file is compiled with -ffp-contract=off (csrc/Makefile):
// the grey level and the blanking threshold are stated as separately rounded operations, and a fused multiply-add of two of them
// gives another level (another threshold) wherever the exact value lies within an ulp of the boundary.
//
// compose_nc_kernel is compose_kernel's walk (csrc/recon.hip): one wave per token, float4 groups of pred.  The order inside a patch is
// (a < u, py, px, c < C), channels innermost, and so is the output: four consecutive pred elements are four consecutive output bytes
// of one image row (p % 4 == 0, so a group never leaves its patch row), written with one 4-byte store per panel.  For C = 1 the target
// is one float4 of the frame; for C = 3 the four elements come from the three channel planes, one scalar load each.
//   bytes per output byte: 4 (pred) + 4 (image) read, 4 x 1 written; denorm reads the target patch twice more (cache-resident)
//
// white_border is TWO launches on the caller's stream, no host synchronisation in between:
//   wb_extremes_kernel  up to 64 workgroups per image: min, max and a NaN flag of their share of all T frames -> ws
//   wb_rows_kernel      one wave per row of frame 0: folds its image's partial extremes (at most 64, one per lane), forms the threshold,
//                       finds the two runs and writes the blanked row into every frame and the marks into every frame of `region`
// rather than one workgroup per image: a batch of the joint recipe is 64 triplets of 3 x 512 x 512, 3 MB each, and 64 workgroups that
// each stream 3 MB twice would leave three quarters of the chip idle for the whole pass, where the second launch costs microseconds.
// The rows kernel reads frame 0 only and the extremes kernel has finished by then (stream order), so the in-place update has no
// reader left: a lane reads and writes its own four columns.
//
// What the reference does with an image that holds a NaN: torch.max / torch.min propagate it, the threshold is NaN and no pixel is
// white, so nothing is marked -- and the frames still become copies of frame 0 (its repeat_interleave is unconditional).  fmaxf does
// not propagate a NaN, hence the flag.
#include <cstdint>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

__device__ __forceinline__ bool finite2d(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct Levels {
  float s[3], m[3];
};

// (int) clip(((v * s) + m) * 255, 0, 255): three roundings (no contraction in this file).  A non-finite v gives 0.
__device__ __forceinline__ unsigned level(float v, float s, float m) {
  const float a = v * s;
  float t = (a + m) * 255.0f;
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return finite2d(v) ? (unsigned)(int)t : 0u;
}

__device__ __forceinline__ float pick3(const float (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// the four target values of pred elements rem .. rem + 3 of patch row y (rem: offset inside the row of p * C elements, a multiple of 4)
template <int C>
__device__ __forceinline__ f32x4 load_target(const float* __restrict__ vol, size_t plane, int T, int W, int f, int y, int x0, int rem) {
  if (C == 1) return *reinterpret_cast<const f32x4*>(vol + (size_t)f * plane + (size_t)y * W + x0 + rem);
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ee = rem + k, c = ee % C, px = ee / C;
    r[k] = vol[((size_t)c * T + f) * plane + (size_t)y * W + x0 + px];
  }
  return r;
}

template <int C, bool DENORM>
__global__ __launch_bounds__(256) void compose_nc_kernel(const float* __restrict__ pred, long long pred_bs, const float* __restrict__ imgs,
                                                         const float* __restrict__ mask, uint8_t* __restrict__ out, Levels lv, int B,
                                                         int T, int H, int W, int u_sz, int p, int L, int Tp) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int gh = H / p, gw = W / p;
  const int rowlen = p * C;           // one patch row, channels innermost: a multiple of 4
  const int PD = u_sz * p * rowlen;
  const int nq = PD >> 2;
  const int rows = B * L;
  const size_t plane = (size_t)H * W;
  const size_t panel = (size_t)Tp * plane * C;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / L, l = row - b * L;
    const bool removed = mask[row] != 0.0f;
    const int t = l / (gh * gw), hy = (l / gw) % gh, wx = l % gw;
    const float* pr = pred + (size_t)b * (size_t)pred_bs + (size_t)l * PD;
    const float* vol = imgs + (size_t)b * C * T * plane;
    // per-patch statistics of the target over all PD elements (the norm_pix branch of the loss), fp32, two passes
    float mu = 0.f, sd = 1.f;
    if (DENORM) {
      float s = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int rem = e % rowlen, py = (e / rowlen) % p, a = e / (rowlen * p);
        const f32x4 iv = load_target<C>(vol, plane, T, W, t * u_sz + a, hy * p + py, wx * p, rem);
        s += (iv[0] + iv[1]) + (iv[2] + iv[3]);
      }
      mu = wave_sum(s) / (float)PD;
      float s2 = 0.f;
      for (int q = lane; q < nq; q += 64) {
        const int e = 4 * q;
        const int rem = e % rowlen, py = (e / rowlen) % p, a = e / (rowlen * p);
        const f32x4 iv = load_target<C>(vol, plane, T, W, t * u_sz + a, hy * p + py, wx * p, rem);
#pragma unroll
        for (int k = 0; k < 4; ++k) s2 = fmaf(iv[k] - mu, iv[k] - mu, s2);
      }
      sd = sqrtf(wave_sum(s2) / (float)(PD - 1) + 1.0e-6f);
    }
    for (int q = lane; q < nq; q += 64) {
      const int e = 4 * q;
      const int rem = e % rowlen, py = (e / rowlen) % p, a = e / (rowlen * p);
      const int fo = t * u_sz + a, y = hy * p + py;
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pr + e);
      const f32x4 iv = load_target<C>(vol, plane, T, W, fo, y, wx * p, rem);
      unsigned gx[4], gp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = C == 1 ? 0 : (rem + k) % C;
        const float sc = pick3(lv.s, c), sh = pick3(lv.m, c);
        gx[k] = level(iv[k], sc, sh);
        gp[k] = level(DENORM ? fmaf(pv[k], sd, mu) : pv[k], sc, sh);
      }
      const unsigned wx4 = gx[0] | (gx[1] << 8) | (gx[2] << 16) | (gx[3] << 24);
      const unsigned wp4 = gp[0] | (gp[1] << 8) | (gp[2] << 16) | (gp[3] << 24);
      uint8_t* o = out + (size_t)b * 4 * panel + (((size_t)fo * H + y) * W + wx * p) * C + rem;
      *reinterpret_cast<unsigned*>(o) = wx4;
      *reinterpret_cast<unsigned*>(o + panel) = removed ? 0u : wx4;
      *reinterpret_cast<unsigned*>(o + 2 * panel) = wp4;
      *reinterpret_cast<unsigned*>(o + 3 * panel) = removed ? wp4 : wx4;
    }
  }
}

// ---- border blanking --------------------------------------------------------------------------------------------------------------
constexpr int WB_PARTS = 64;   // partial extremes per image at most: one per lane of the wave that folds them

__device__ __forceinline__ float wv_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wv_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wv_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wv_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__host__ __device__ inline int wb_parts(long long quads) {
  const long long n = (quads + 255) / 256;
  return (int)(n < WB_PARTS ? (n < 1 ? 1 : n) : WB_PARTS);
}

// workgroup (b, part): (max, min, NaN flag) of the float4 groups part * 256 + tid, + parts * 256, ... of image b  ->  ws[(b * parts + part) * 3]
__global__ __launch_bounds__(256) void wb_extremes_kernel(const float* __restrict__ imgs, float* __restrict__ ws, long long quads, int parts) {
  const int b = blockIdx.x / parts, part = blockIdx.x - b * parts;
  const float* img = imgs + (size_t)b * (size_t)quads * 4;
  float mx = -INFINITY, mn = INFINITY, bad = 0.0f;
  for (long long q = (long long)part * 256 + threadIdx.x; q < quads; q += (long long)parts * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(img + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mx = fmaxf(mx, v[k]);
      mn = fminf(mn, v[k]);
      bad = v[k] != v[k] ? 1.0f : bad;
    }
  }
  mx = wv_max(mx), mn = wv_min(mn), bad = wv_max(bad);
  __shared__ float red[3][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[0][w] = mx, red[1][w] = mn, red[2][w] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = ws + (size_t)blockIdx.x * 3;
    o[0] = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    o[1] = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
    o[2] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
  }
}

struct WbLimits {
  int left_idle_from;    // the left run is followed iff first white column < this        (the reference: not (f > 0.01 * W))
  int left_ext_from;     // ... and extended by 5 columns iff its end e >= this             (e > 0.05 * W)
  int right_live_from;   // the right run is followed iff last white column >= this         (not (l < W - 0.01 * W))
  int right_ext_below;   // ... and the slice [s : s - 5] is assigned iff its stop s < this (s < W - 0.05 * W)
};

// one wave per row y of frame 0 of image b; a lane owns the columns 4 * (64 * chunk + lane) .. + 3
__global__ __launch_bounds__(256) void wb_rows_kernel(float* __restrict__ imgs, uint8_t* __restrict__ region, const float* __restrict__ ws,
                                                      int B, int T, int H, int W, int parts, WbLimits lim) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int rows = B * H;
  const int nq = W >> 2;
  const size_t plane = (size_t)H * W;
  const float k = (float)(15.0 / 255.0);
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / H, y = row - b * H;
    float mx = -INFINITY, mn = INFINITY, bad = 0.0f;
    if (lane < parts) {
      const float* q = ws + ((size_t)b * parts + lane) * 3;
      mx = q[0], mn = q[1], bad = q[2];
    }
    mx = wv_max(mx), mn = wv_min(mn), bad = wv_max(bad);
    const float gap = mx - mn;
    const float prod = k * gap;
    const float thresh = bad != 0.0f ? __uint_as_float(0x7fc00000u) : mx - prod;
    float* r0 = imgs + (size_t)b * T * plane + (size_t)y * W;
    // first and last white column
    int f = W, l = -1;
    for (int q = lane; q < nq; q += 64) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r0 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j] > thresh) f = min(f, 4 * q + j), l = max(l, 4 * q + j);
    }
    f = wv_imin(f), l = wv_imax(l);
    const bool left = l >= 0 && f < lim.left_idle_from;
    const bool right = l >= 0 && l >= lim.right_live_from;
    // e: first column >= f that is not white (W: none); s: last column <= l that is not white (-1: none)
    int e = W, s = -1;
    if (left || right) {
      for (int q = lane; q < nq; q += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(r0 + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = 4 * q + j;
          if (!(v[j] > thresh)) {
            if (x >= f) e = min(e, x);
            if (x <= l) s = max(s, x);
          }
        }
      }
      e = wv_imin(e), s = wv_imax(s);
    }
    const int e2 = (left && e < W && e >= lim.left_ext_from) ? min(e + 5, W) : e;      // [e, e + 5) joins the left run
    // the reference's connected_region[row, s : s - 5]: empty for s >= 5, [s, W + s - 5) for s <= 4 (a negative stop counts from the end)
    const bool rext = right && s >= 0 && s < lim.right_ext_below && s <= 4;
    const int r2 = W + s - 5;
    for (int q = lane; q < nq; q += 64) {
      // Written as selects into scalars: with `if (m) v[j] = 0.0f` on the loaded vector, hipcc (ROCm 7) kept element 0 of a group
      // that the right run marked (seen in the ISA, and as 192 unblanked pixels in tests/test_gpu_recon2d.py's w128 case).
      const f32x4 in = *reinterpret_cast<const f32x4*>(r0 + 4 * q);
      float o[4];
      unsigned marks = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = 4 * q + j;
        const bool m = (left && x >= f && x < e2) || (right && x > s && x <= l) || (rext && x >= s && x < r2);
        o[j] = m ? 0.0f : in[j];
        marks |= m ? 1u << (8 * j) : 0u;
      }
      const f32x4 v = {o[0], o[1], o[2], o[3]};
      for (int t = 0; t < T; ++t) {
        *reinterpret_cast<f32x4*>(r0 + (size_t)t * plane + 4 * q) = v;
        *reinterpret_cast<unsigned*>(region + ((size_t)b * T + t) * plane + (size_t)y * W + 4 * q) = marks;
      }
    }
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_mae_compose_nc(const float* pred, long long pred_batch_stride, const float* imgs, const float* mask, uint8_t* out,
                                     int B, int C, int T, int H, int W, int u_sz, int p, int L, float scale0, float scale1, float scale2,
                                     float shift0, float shift1, float shift2, int denorm, void* stream) {
  OCTMAE_CHECK_ARG(pred && imgs && mask && out);
  OCTMAE_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && u_sz > 0 && p > 0 && L > 0);
  OCTMAE_CHECK_ARG(C == 1 || C == 3);
  OCTMAE_CHECK_ARG(p % 4 == 0 && W % 4 == 0 && H % p == 0 && W % p == 0);
  const long long PD = (long long)u_sz * p * p * C, grid = (long long)(H / p) * (W / p);
  OCTMAE_CHECK_ARG(L % grid == 0);
  const long long Tp = (L / grid) * u_sz;
  OCTMAE_CHECK_ARG(pred_batch_stride >= (long long)L * PD && pred_batch_stride % 4 == 0);
  OCTMAE_CHECK_ARG(Tp <= T);                                     // the frame map is the identity: every predicted frame must exist
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(pred) & 15u) == 0 && (reinterpret_cast<uintptr_t>(imgs) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 3u) == 0);
  Levels lv = {{scale0, scale1, scale2}, {shift0, shift1, shift2}};
  for (int c = 0; c < 3; ++c) OCTMAE_CHECK_ARG(lv.s[c] - lv.s[c] == 0.0f && lv.m[c] - lv.m[c] == 0.0f);      // finite
  if (u_sz > 1 && C > 1) return -2;                              // no caller, and no statement of that element order to test against
  if (denorm != 0 && denorm != 1) return -2;
  if ((long long)B * L > 0x7fffffffLL || PD > 0x7fffffffLL || Tp > 0x7fffffffLL) return -2;   // token and element indices are ints
  long long blocks = ((long long)B * L + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define OCTMAE_NC_LAUNCH(CC, DD)                                                                                                       \
  hipLaunchKernelGGL((compose_nc_kernel<CC, DD>), dim3((unsigned)blocks), dim3(256), 0, st, pred, pred_batch_stride, imgs, mask, out, lv, \
                     B, T, H, W, u_sz, p, L, (int)Tp)
  if (C == 1) {
    if (denorm) OCTMAE_NC_LAUNCH(1, true); else OCTMAE_NC_LAUNCH(1, false);
  } else {
    if (denorm) OCTMAE_NC_LAUNCH(3, true); else OCTMAE_NC_LAUNCH(3, false);
  }
#undef OCTMAE_NC_LAUNCH
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_white_border_ws_floats(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || W % 4 != 0) return -1;
  const long long quads = (long long)T * H * (W / 4);
  const long long n = 3LL * B * wb_parts(quads);
  return n > 0x7fffffffLL ? -2 : (int)n;
}

extern "C" int octmae_white_border(float* imgs, uint8_t* region, float* ws, int B, int T, int H, int W, int left_idle_from,
                                   int left_ext_from, int right_live_from, int right_ext_below, void* stream) {
  OCTMAE_CHECK_ARG(imgs && region && ws);
  OCTMAE_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && W % 4 == 0);
  OCTMAE_CHECK_ARG(left_idle_from >= 0 && left_idle_from <= W + 1 && left_ext_from >= 0 && left_ext_from <= W + 1 &&
                   right_live_from >= 0 && right_live_from <= W + 1 && right_ext_below >= 0 && right_ext_below <= W + 1);
  // 16-byte loads and stores of the rows, 4-byte stores of the marks
  OCTMAE_CHECK_ARG((reinterpret_cast<uintptr_t>(imgs) & 15u) == 0 && (reinterpret_cast<uintptr_t>(region) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(ws) & 3u) == 0);
  const long long quads = (long long)T * H * (W / 4);
  const int parts = wb_parts(quads);
  if ((long long)B * H > 0x7fffffffLL || (long long)B * parts > 0x7fffffffLL) return -2;      // row and workgroup indices are ints
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(wb_extremes_kernel, dim3((unsigned)((long long)B * parts)), dim3(256), 0, st, imgs, ws, quads, parts);
  OCTMAE_LAUNCH_CHECK();
  long long blocks = ((long long)B * H + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  WbLimits lim = {left_idle_from, left_ext_from, right_live_from, right_ext_below};
  hipLaunchKernelGGL(wb_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, imgs, region, ws, B, T, H, W, parts, lim);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
