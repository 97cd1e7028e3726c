// RandAugment's image operations behind the 2-D resize: the reference's OCTCube/util/rand_augment.py (timm's auto_augment on Pillow)
//   util/datasets.py build_transform('train')   RandomResizedCrop -> flip -> RandAugment rand-m9-mstd0.5-inc1 -> ToTensor -> Normalize
// on n equally sized uint8 [H][W][3] images in device memory, bit-equal to Pillow for the same decisions (which the host draws:
// octcubem_amd/rand_augment.py).  Two kernels:
//
//   image_stats_kernel     per image that asks for it, the 256-bin histograms of R, G, B and L = convert("L").  A workgroup counts a
//                          strip of pixels into LDS and adds its non-empty bins to global memory with vector atomics.
//   image_augment_kernel   ONE op per image, read from the image's descriptor (augment2d_plan.hpp).  A workgroup owns AUG_TH x AUG_TW
//                          pixels of one image, a thread a pixel (three channels) at a time.  Prologue: the ToTensor -> Normalize table
//                          into LDS when the launch writes float32; for a table op the 3 x 256 byte table, built from the descriptor and
//                          -- AutoContrast, Equalize, the Contrast mean -- from the image's histograms, so nothing returns to the host.
//                            none        copy
//                            table       Invert, Posterize, Solarize, SolarizeAdd, Brightness, Contrast, AutoContrast, Equalize
//                            colour      blend(L, pixel)
//                            sharpness   blend(SMOOTH 3 x 3, pixel) from an LDS tile with a one-pixel halo
//                            affine      Image.transform(AFFINE) with the bilinear / bicubic filter in double, fill outside the source
//                          The store is uint8 [n][H][W][3], or through the table float32 [n][3][H][W] (ToTensor -> Normalize fused).
//
// Every float and double expression here is Pillow's, operation by operation: csrc/Makefile compiles this file with
// -ffp-contract=off (as image2d.hip; see there).  No 16-bit operand: the two builds of the library hold the same code.
//   bytes/image: 3 H W read + 3 H W (or 12 H W) written; the affine kinds read up to 16 taps per pixel, nearly all from cache
#include "common.hpp"
#include "augment2d_plan.hpp"
#include "../../include/octmae.h"

namespace octmae {

struct AugParams {
  const uint8_t* src;
  void* dst;
  const octmae_aug_desc* desc;
  const unsigned* hist;      // [n][4][256] or null
  const float* lut;          // [3][256] or null
  int H, W;
  int tiles_x, tiles_y;
};

// ---- statistics ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void image_stats_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ needed,
                                                                  unsigned* __restrict__ hist, long long pixels, int strips) {
  __shared__ unsigned s_h[4 * 256];
  const int img = blockIdx.x / strips, strip = blockIdx.x - img * strips;
  if (needed && !needed[img]) return;                // uniform over the workgroup
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * 256; i += AUG_THREADS) s_h[i] = 0;
  __syncthreads();
  const uint8_t* s = src + (size_t)img * pixels * 3;
  for (long long i = (long long)strip * AUG_THREADS + tid; i < pixels; i += (long long)strips * AUG_THREADS) {
    const int r = s[i * 3], g = s[i * 3 + 1], b = s[i * 3 + 2];
    atomicAdd(&s_h[r], 1u);
    atomicAdd(&s_h[256 + g], 1u);
    atomicAdd(&s_h[512 + b], 1u);
    atomicAdd(&s_h[768 + aug_luma(r, g, b)], 1u);
  }
  __syncthreads();
  unsigned* h = hist + (size_t)img * 1024;
  for (int i = tid; i < 4 * 256; i += AUG_THREADS)
    if (s_h[i]) atomicAdd(&h[i], s_h[i]);
}

// ---- the table of a table op: s_tab [3][256] bytes; s_w: 3 * 256 + 8 words of scratch ---------------------------------------------------------
__device__ void build_table(const octmae_aug_desc& d, const unsigned* __restrict__ h, uint8_t* s_tab, unsigned* s_w, int tid) {
  const int op = d.mode;
  if (op == AUG_LUT_AUTOCONTRAST || op == AUG_LUT_EQUALIZE) {
    int* s_lo = reinterpret_cast<int*>(s_w + 768);        // [3] lowest, [3] highest non-empty bin
    if (tid < 3) { s_lo[tid] = 256; s_lo[3 + tid] = -1; }
    for (int c = 0; c < 3; ++c) s_w[c * 256 + tid] = h ? h[c * 256 + tid] : 0u;
    __syncthreads();
    for (int c = 0; c < 3; ++c)
      if (s_w[c * 256 + tid]) { atomicMin(&s_lo[c], tid); atomicMax(&s_lo[3 + c], tid); }
    __syncthreads();
    if (op == AUG_LUT_AUTOCONTRAST) {
      for (int c = 0; c < 3; ++c) {
        const int lo = s_lo[c], hi = s_lo[3 + c];
        int v = tid;
        if (hi > lo) {
          const double scale = 255.0 / (double)(hi - lo);
          const double offset = (double)(-lo) * scale;
          const double t = (double)tid * scale + offset;
          v = (int)t;
          v = v < 0 ? 0 : v > 255 ? 255 : v;
        }
        s_tab[c * 256 + tid] = (uint8_t)v;
      }
      return;
    }
    // Equalize: an inclusive scan of each channel's 256 bins (Hillis-Steele in place, read - barrier - write - barrier)
    unsigned last[3];
    for (int c = 0; c < 3; ++c) last[c] = s_lo[3 + c] >= 0 ? s_w[c * 256 + s_lo[3 + c]] : 0u;
    unsigned own[3];
    for (int c = 0; c < 3; ++c) own[c] = s_w[c * 256 + tid];
    for (int off = 1; off < 256; off <<= 1) {
      unsigned add[3];
      for (int c = 0; c < 3; ++c) add[c] = tid >= off ? s_w[c * 256 + tid - off] : 0u;
      __syncthreads();
      for (int c = 0; c < 3; ++c) s_w[c * 256 + tid] += add[c];
      __syncthreads();
    }
    for (int c = 0; c < 3; ++c) {
      const unsigned total = s_w[c * 256 + 255];
      const unsigned step = s_lo[3 + c] > s_lo[c] ? (total - last[c]) / 255u : 0u;      // one non-empty bin at the most: identity
      int v = tid;
      if (step) {
        const unsigned long long n = (unsigned long long)(step / 2u) + (s_w[c * 256 + tid] - own[c]);   // the bins below this one
        const unsigned long long q = n / step;
        v = q > 255ull ? 255 : (int)q;
      }
      s_tab[c * 256 + tid] = (uint8_t)v;
    }
    return;
  }
  int v;
  if (op == AUG_LUT_CONTRAST) {
    // mean = int(sum(i hL[i]) / count + 0.5): the sum is an exact integer below 2^53, as Pillow's float accumulation of it
    unsigned long long* s_s = reinterpret_cast<unsigned long long*>(s_w);      // 256 x 8 bytes of the 3 x 256 words
    unsigned long long* s_n = s_s + 256;                                       // 128 x 8 bytes
    const unsigned hv = h ? h[768 + tid] : 0u;
    s_s[tid] = (unsigned long long)tid * hv;
    __syncthreads();
    if (tid < 128) s_n[tid] = (unsigned long long)hv + (h ? h[768 + 128 + tid] : 0u);
    for (int off = 128; off >= 1; off >>= 1) {
      __syncthreads();
      if (tid < off) {
        s_s[tid] += s_s[tid + off];
        if (off < 128) s_n[tid] += s_n[tid + off];
      }
    }
    __syncthreads();
    const double cnt = (double)s_n[0];
    const int mean = cnt > 0.0 ? (int)((double)s_s[0] / cnt + 0.5) : 0;
    v = aug_blend(mean, tid, d.factor);
  } else if (op == AUG_LUT_INVERT) {
    v = 255 - tid;
  } else if (op == AUG_LUT_POSTERIZE) {
    v = d.iarg >= 8 ? tid : tid & ~((1 << (8 - d.iarg)) - 1) & 0xff;
  } else if (op == AUG_LUT_SOLARIZE) {
    v = tid < d.iarg ? tid : 255 - tid;
  } else if (op == AUG_LUT_SOLARIZE_ADD) {
    v = tid < 128 ? min(255, tid + d.iarg) : tid;
  } else {                                            // AUG_LUT_BRIGHTNESS
    v = aug_blend(0, tid, d.factor);
  }
  s_tab[tid] = s_tab[256 + tid] = s_tab[512 + tid] = (uint8_t)v;
}

// ---- the affine kinds: Geometry.c's bilinear_filter32RGB / bicubic_filter32RGB ---------------------------------------------------------------
__device__ __forceinline__ int aug_floor(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }
__device__ __forceinline__ int aug_clampi(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }
__device__ __forceinline__ double aug_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// false: the source position lies outside the image (the pixel keeps the fill colour)
__device__ bool aug_affine(const uint8_t* __restrict__ s, int H, int W, const octmae_aug_desc& d, int ox, int oy, int out[3]) {
  const double xc = (double)ox + 0.5, yc = (double)oy + 0.5;
  double xin = d.m[0] * xc + d.m[1] * yc + d.m[2];
  double yin = d.m[3] * xc + d.m[4] * yc + d.m[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return false;     // a NaN is outside as well
  xin -= 0.5;
  yin -= 0.5;
  const int x = aug_floor(xin), y = aug_floor(yin);
  const double dx = xin - (double)x, dy = yin - (double)y;
  if (d.mode == AUG_BILINEAR) {
    const int x0 = aug_clampi(x, W) * 3, x1 = aug_clampi(x + 1, W) * 3;
    const uint8_t* r0 = s + (size_t)aug_clampi(y, H) * W * 3;
    const uint8_t* r1 = s + (size_t)aug_clampi(y + 1, H) * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a0 = r0[x0 + c], b0 = r0[x1 + c], a1 = r1[x0 + c], b1 = r1[x1 + c];
      const double v1 = a0 + (b0 - a0) * dx;
      const double v2 = a1 + (b1 - a1) * dx;
      out[c] = (int)(v1 + (v2 - v1) * dy);
    }
    return true;
  }
  int xo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) xo[k] = aug_clampi(x - 1 + k, W) * 3;
  double acc[3][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint8_t* r = s + (size_t)aug_clampi(y - 1 + k, H) * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c][k] = aug_cubic(r[xo[0] + c], r[xo[1] + c], r[xo[2] + c], r[xo[3] + c], dx);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = aug_cubic(acc[c][0], acc[c][1], acc[c][2], acc[c][3], dy);
    out[c] = v <= 0.0 ? 0 : v >= 255.0 ? 255 : (int)v;
  }
  return true;
}

template <bool LUT>
__global__ __launch_bounds__(AUG_THREADS) void image_augment_kernel(const AugParams p) {
  __shared__ float s_lut[LUT ? 3 * 256 : 1];
  __shared__ __attribute__((aligned(8))) unsigned s_w[3 * 256 + 8];
  __shared__ uint8_t s_tab[3 * 256];
  __shared__ uint8_t s_tile[(AUG_TH + 2) * (AUG_TW + 2) * 3];

  const int tid = threadIdx.x;
  const int tx = blockIdx.x % p.tiles_x, t = blockIdx.x / p.tiles_x;
  const int ty = t % p.tiles_y, img = t / p.tiles_y;
  const int x0 = tx * AUG_TW, y0 = ty * AUG_TH;
  const int ncol = min(AUG_TW, p.W - x0), nrow = min(AUG_TH, p.H - y0);
  const int H = p.H, W = p.W;
  const octmae_aug_desc d = p.desc[img];              // uniform over the workgroup
  const int kind = d.kind;
  const uint8_t* s = p.src + (size_t)img * H * W * 3;

  if (LUT)
    for (int i = tid; i < 3 * 256; i += AUG_THREADS) s_lut[i] = p.lut[i];
  if (kind == AUG_KIND_TABLE) {
    build_table(d, p.hist ? p.hist + (size_t)img * 1024 : nullptr, s_tab, s_w, tid);
  } else if (kind == AUG_KIND_SHARPNESS) {
    // the tile with a one-pixel halo, clamped at the image's edges (clamped entries are read by border pixels only, which are copies)
    const int tw3 = (ncol + 2) * 3;
    for (int i = tid; i < (nrow + 2) * tw3; i += AUG_THREADS) {
      const int r = i / tw3, j = i - r * tw3;
      const int col = j / 3, c = j - col * 3;
      const int yy = aug_clampi(y0 - 1 + r, H), xx = aug_clampi(x0 - 1 + col, W);
      s_tile[r * (AUG_TW + 2) * 3 + j] = s[((size_t)yy * W + xx) * 3 + c];
    }
  }
  __syncthreads();

  for (int i = tid; i < nrow * ncol; i += AUG_THREADS) {
    const int r = i / ncol, col = i - r * ncol;
    const int oy = y0 + r, ox = x0 + col;
    int v[3];
    if (kind == AUG_KIND_AFFINE) {
      if (!aug_affine(s, H, W, d, ox, oy, v)) { v[0] = d.fill[0]; v[1] = d.fill[1]; v[2] = d.fill[2]; }
    } else if (kind == AUG_KIND_SHARPNESS) {
      const uint8_t* c0 = s_tile + ((r + 1) * (AUG_TW + 2) + col + 1) * 3;
      const bool border = oy == 0 || ox == 0 || oy == H - 1 || ox == W - 1;
      constexpr int RS = (AUG_TW + 2) * 3;
      const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int px = c0[c];
        int sm = px;
        if (!border) {
          const uint8_t* q = c0 + c;
          float ss = 0.5f;
          ss += (float)q[RS - 3] * k1 + (float)q[RS] * k1 + (float)q[RS + 3] * k1;       // Filter.c: the row below first
          ss += (float)q[-3] * k1 + (float)q[0] * k5 + (float)q[3] * k1;
          ss += (float)q[-RS - 3] * k1 + (float)q[-RS] * k1 + (float)q[-RS + 3] * k1;
          sm = ss <= 0.0f ? 0 : ss >= 255.0f ? 255 : (int)ss;
        }
        v[c] = aug_blend(sm, px, d.factor);
      }
    } else {
      const uint8_t* q = s + ((size_t)oy * W + ox) * 3;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
      if (kind == AUG_KIND_TABLE) {
        v[0] = s_tab[v[0]]; v[1] = s_tab[256 + v[1]]; v[2] = s_tab[512 + v[2]];
      } else if (kind == AUG_KIND_COLOR) {
        const int l = aug_luma(v[0], v[1], v[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = aug_blend(l, v[c], d.factor);
      }
    }
    if (LUT) {
      float* out = static_cast<float*>(p.dst);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        __builtin_nontemporal_store(s_lut[c * 256 + v[c]], out + (((size_t)img * 3 + c) * H + oy) * W + ox);
    } else {
      uint8_t* out = static_cast<uint8_t*>(p.dst) + (((size_t)img * H + oy) * W + ox) * 3;
      out[0] = (uint8_t)v[0]; out[1] = (uint8_t)v[1]; out[2] = (uint8_t)v[2];
    }
  }
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_image_stats(const void* src, int n, int H, int W, const unsigned char* needed, unsigned* hist, void* stream) {
  OCTMAE_CHECK_ARG(src && hist && n > 0 && H > 0 && W > 0);
  const long long pixels = (long long)H * W;
  OCTMAE_CHECK_ARG(pixels <= AUG_MAX_PIXELS);
  const int strips = aug_stats_strips(pixels);
  OCTMAE_CHECK_ARG((long long)strips * n <= 0x7fffffffLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 1024 * sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(image_stats_kernel, dim3((unsigned)(strips * n)), dim3(AUG_THREADS), 0, st, static_cast<const uint8_t*>(src), needed,
                     hist, pixels, strips);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_image_augment(const void* src, int n, int H, int W, const octmae_aug_desc* desc, const octmae_aug_desc* desc_host,
                                    const unsigned* hist, const float* lut, void* dst, void* stream) {
  OCTMAE_CHECK_ARG(src && dst && desc && src != dst && n > 0 && H > 0 && W > 0);
  OCTMAE_CHECK_ARG((long long)H * W <= AUG_MAX_PIXELS);
  if (desc_host)
    for (int i = 0; i < n; ++i) OCTMAE_CHECK_ARG(aug_desc_ok(desc_host[i], hist != nullptr));
  AugParams p;
  p.src = static_cast<const uint8_t*>(src);
  p.dst = dst;
  p.desc = desc;
  p.hist = hist;
  p.lut = lut;
  p.H = H; p.W = W;
  p.tiles_x = (W + AUG_TW - 1) / AUG_TW;
  p.tiles_y = (H + AUG_TH - 1) / AUG_TH;
  const long long blocks = (long long)p.tiles_x * p.tiles_y * n;
  OCTMAE_CHECK_ARG(blocks <= 0x7fffffffLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (lut)
    hipLaunchKernelGGL(image_augment_kernel<true>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL(image_augment_kernel<false>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, st, p);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}
