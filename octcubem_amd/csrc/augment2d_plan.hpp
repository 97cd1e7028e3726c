// The image augmentation kernels (augment2d.hip): the constants of a launch, the descriptor's codes and its argument rules, and the two
// per-pixel rules every kind shares -- Pillow's convert("L") and its blend -- as plain C++ that host and kernel both compile.
//
// The blend is IEEE float evaluated operation by operation (Blend.c, compiled without fused multiply-adds): csrc/Makefile compiles
// augment2d.hip with -ffp-contract=off, and the pragma covers a build with any pragma-honouring setting (see image2d_plan.hpp).
#pragma once
#include <cstdint>

#include "../../include/octmae.h"

#ifndef OCTMAE_HD
#if defined(__HIPCC__)
#define OCTMAE_HD __host__ __device__ __forceinline__
#else
#define OCTMAE_HD inline
#endif
#endif

#pragma clang fp contract(off)

namespace octmae {

constexpr int AUG_THREADS = 256;           // the table prologue gives every thread one grey level
constexpr int AUG_TW = 64;                 // a wave stores 256 contiguous bytes of a float32 plane row
constexpr int AUG_TH = 16;
constexpr long long AUG_MAX_PIXELS = 1LL << 30;    // histogram bins are 32 bit, 3 H W an int

// octmae_aug_desc.kind, and .mode of a table op / of an affine op (Pillow's resampling numbers)
enum { AUG_KIND_NONE = 0, AUG_KIND_TABLE = 1, AUG_KIND_COLOR = 2, AUG_KIND_SHARPNESS = 3, AUG_KIND_AFFINE = 4 };
enum { AUG_LUT_INVERT = 0, AUG_LUT_POSTERIZE = 1, AUG_LUT_SOLARIZE = 2, AUG_LUT_SOLARIZE_ADD = 3, AUG_LUT_BRIGHTNESS = 4,
       AUG_LUT_CONTRAST = 5, AUG_LUT_AUTOCONTRAST = 6, AUG_LUT_EQUALIZE = 7 };
enum { AUG_BILINEAR = 2, AUG_BICUBIC = 3 };

// Image.convert("L") of an RGB pixel
OCTMAE_HD int aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// ImagingBlend with a C float alpha: truncated for alpha in [0, 1] (the value cannot leave [0, 255] there), clipped and truncated
// outside.  alpha == 1 gives in2 exactly, which is Pillow's copy shortcut.
OCTMAE_HD int aug_blend(int in1, int in2, float alpha) {
  const float t = (float)in1 + alpha * (float)(in2 - in1);
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

inline bool aug_needs_hist(const octmae_aug_desc& d) {
  return d.kind == AUG_KIND_TABLE && d.mode >= AUG_LUT_CONTRAST && d.mode <= AUG_LUT_EQUALIZE;
}

// the argument rules of one descriptor; have_hist: the launch was given histograms
inline bool aug_desc_ok(const octmae_aug_desc& d, bool have_hist) {
  switch (d.kind) {
    case AUG_KIND_NONE:
      return true;
    case AUG_KIND_TABLE:
      if (d.mode < AUG_LUT_INVERT || d.mode > AUG_LUT_EQUALIZE) return false;
      if (d.mode == AUG_LUT_POSTERIZE && d.iarg < 0) return false;
      if (d.mode == AUG_LUT_SOLARIZE_ADD && (d.iarg < 0 || d.iarg > 255)) return false;
      if ((d.mode == AUG_LUT_BRIGHTNESS || d.mode == AUG_LUT_CONTRAST) && !(d.factor == d.factor)) return false;
      return have_hist || !aug_needs_hist(d);
    case AUG_KIND_COLOR:
    case AUG_KIND_SHARPNESS:
      return d.factor == d.factor;
    case AUG_KIND_AFFINE:
      for (int i = 0; i < 6; ++i)
        if (!(d.m[i] - d.m[i] == 0.0)) return false;         // finite
      return d.mode == AUG_BILINEAR || d.mode == AUG_BICUBIC;
    default:
      return false;
  }
}

// workgroups per image of the statistics launch: 16 pixels per thread, at most 64 strips (their merges are 1024 atomics each)
inline int aug_stats_strips(long long pixels) {
  const long long s = (pixels + AUG_THREADS * 16 - 1) / (AUG_THREADS * 16);
  return s < 1 ? 1 : s > 64 ? 64 : (int)s;
}

}  // namespace octmae
