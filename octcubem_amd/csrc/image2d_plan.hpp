// The 2-D image resample (image2d.hip): Pillow's per-axis coefficient rule and the tile plan, as plain C++ that the host and the
// kernel both compile (no launches, no device pointers), so that the window of an output index is written once, the plan can be
// queried without a GPU (octmae_image_resample_plan) and is tested there (tests/test_cpu_transform2d.py).
//
// Everything in this file is IEEE double evaluated operation by operation: one fused multiply-add in the centre or in a weight moves
// a 22-bit coefficient by one unit, and the result would no longer be Pillow's.  The library's -ffp-contract=fast ignores the pragma
// below, so csrc/Makefile compiles image2d.hip with -ffp-contract=off; the pragma covers a build with any pragma-honouring setting.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OCTMAE_HD __host__ __device__ __forceinline__
#else
#define OCTMAE_HD inline
#endif

#pragma clang fp contract(off)

namespace octmae {

constexpr int IMG_TW = 64;                 // output columns of a tile: one wave stores 256 contiguous bytes of a float32 plane row
constexpr int IMG_THREADS = 256;
constexpr int IMG_LUT_BYTES = 3 * 256 * 4; // the ToTensor -> Normalize table, always reserved
// LDS budget of one workgroup.  A CU has 160 KiB: 64 KiB leaves room for two workgroups (eight waves) per CU even for the widest
// reductions the plan accepts, and is what a launch gets without raising the kernel's dynamic-LDS attribute.  The B-scan shapes need
// 6-10 KiB, so there the wave slots (eight workgroups of four waves), not the LDS, bound the occupancy.
constexpr int IMG_LDS_BUDGET = 64 * 1024;
constexpr int IMG_PRECISION_BITS = 22;     // Pillow: PRECISION_BITS = 32 - 8 - 2

// One axis of Pillow's precompute_coeffs (Resample.c) for the bicubic filter (support 2, a = -0.5) with in0 = 0: the crop is a
// pointer offset and `in` is its extent, which is what torchvision's resized_crop computes (crop, then resize).
struct ImgAxis {
  double scale, filterscale, support, ss;
  int ksize;                               // 2 * ceil(support) + 1: the longest window
};
OCTMAE_HD ImgAxis img_axis(int in, int out) {
  ImgAxis a;
  a.scale = (double)in / (double)out;
  a.filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 2.0 * a.filterscale;
  a.ss = 1.0 / a.filterscale;
  const long long c = (long long)a.support;                      // support >= 2 and far below 2^62
  const long long k = 2 * (c + ((double)c < a.support ? 1 : 0)) + 1;
  a.ksize = k > 0x3fffffffLL ? 0x3fffffff : (int)k;
  return a;
}
// the window [xmin, xmin + xmax) of output index xx; returns the centre
OCTMAE_HD double img_window(const ImgAxis& a, int in, int xx, int& xmin, int& xmax) {
  const double center = ((double)xx + 0.5) * a.scale;
  int lo = (int)(center - a.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + a.support + 0.5);
  if (hi > in) hi = in;
  xmin = lo;
  xmax = hi - lo;
  return center;
}
OCTMAE_HD double img_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
// The fixed-point coefficients of output index xx into k[0], k[stride], ...: the weights are summed in tap order, divided by the
// sum and rounded half away from zero at 22 bits (normalize_coeffs_8bpc).  Two passes over the taps instead of a stored double per
// tap: the weight is a pure function of its argument, so evaluating it again gives the same bits.
template <typename K>
OCTMAE_HD void img_coeffs(const ImgAxis& a, int in, int xx, K* k, int stride, int& xmin, int& xmax) {
  const double center = img_window(a, in, xx, xmin, xmax);
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += img_bicubic(((double)(x + xmin) - center + 0.5) * a.ss);
  for (int x = 0; x < xmax; ++x) {
    double w = img_bicubic(((double)(x + xmin) - center + 0.5) * a.ss);
    if (ww != 0.0) w /= ww;
    k[(long long)x * stride] = (K)(w < 0.0 ? (int)(-0.5 + w * (double)(1 << IMG_PRECISION_BITS))
                                           : (int)(0.5 + w * (double)(1 << IMG_PRECISION_BITS)));
  }
}

// ---- the tile plan -------------------------------------------------------------------------------------------------------------------
// A workgroup owns th x tw output pixels (tw = min(IMG_TW, OW) unless the plan narrows it; edge tiles are smaller).  Its LDS holds, in this order: the table; the column
// coefficients [ksize_x][tw] int32 with xmin[tw], xmax[tw]; the row coefficients [ksize_y][th] with ymin[th], ymax[th]; and the
// horizontal pass of the input rows the tile's windows span, uint8 [rows][tw * C] (rounded up to whole dwords).
struct ImgPlan {
  int th, tw, ksx, ksy, rows;              // rows: the longest row span over the tiles of this th
  int lds_bytes;
};
inline long long img_lds_bytes(int th, int tw, int ksx, int ksy, int rows, int C) {
  const long long tmp = ((long long)rows * tw * C + 3) / 4 * 4;
  return IMG_LUT_BYTES + 4LL * tw * ((long long)ksx + 2) + 4LL * th * ((long long)ksy + 2) + tmp;
}
// the longest span of input rows [ymin(first row), ymin(last row) + ymax(last row)) over the tiles of th output rows
inline int img_row_span(int in, int out, int th) {
  const ImgAxis a = img_axis(in, out);
  int span = 0;
  for (int y0 = 0; y0 < out; y0 += th) {
    const int y1 = (y0 + th < out ? y0 + th : out) - 1;
    int lo, n0, hi, n1;
    img_window(a, in, y0, lo, n0);
    img_window(a, in, y1, hi, n1);
    span = hi + n1 - lo > span ? hi + n1 - lo : span;
  }
  return span;
}
// The largest th of {32, 16, 8, 4, 2, 1} whose LDS fits the budget.  Where not even th = 1 fits at the full tile width -- a strong
// vertical reduction, whose row span is most of the image -- the tile is narrowed instead (tw = 32, 16, ... 1, again with the largest th
// that fits): the stores get shorter, the launch stays possible.  false when one output pixel's two windows alone do not fit.
inline bool plan_image(int in_h, int in_w, int C, int OH, int OW, ImgPlan& p) {
  p.ksx = img_axis(in_w, OW).ksize;
  p.ksy = img_axis(in_h, OH).ksize;
  for (int tw = IMG_TW; tw >= 1; tw >>= 1) {
    if (tw != IMG_TW && tw >= OW) continue;       // the same tile as the one before
    p.tw = OW < tw ? OW : tw;
    for (p.th = 32; p.th >= 1; p.th >>= 1) {
      p.rows = img_row_span(in_h, OH, p.th);
      const long long b = img_lds_bytes(p.th, p.tw, p.ksx, p.ksy, p.rows, C);
      if (b <= IMG_LDS_BUDGET) {
        p.lds_bytes = (int)b;
        return true;
      }
    }
  }
  return false;
}

}  // namespace octmae
