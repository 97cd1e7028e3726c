// Volume transforms in front of every model: the reference's MONAI pipeline (Pre-training/custom_util/PatientDataset_inhouse.py:48-84,
// create_3d_transforms) as two kernels over the raw [D][H][W] scan.
//   octmae_volume_box       CropForegroundd (select_fn = x > 0, margin 0): the bounding box of the voxels > 0, left in device memory
//   octmae_volume_resample  Resized(trilinear) = F.interpolate(mode="trilinear", align_corners=False) of the (boxed) volume, then
//                           RandFlipd on axis 0 / 2 as an index reversal of the store, then NormalizeIntensityd(nonzero=True) as an
//                           epilogue: one pass, 8 taps of the raw volume per output voxel, nothing returns to the host between the two.
// Neither depends on the 16-bit operand type: the two builds of the library hold the same code.
//   box bytes/voxel: 1 (uint8) or 4 (float32) read        resample: <= 8 taps read (cache-resident neighbours), 4 B written per output
#include <climits>
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {

template <typename T>
struct VolVec;
template <>
struct VolVec<uint8_t> { static constexpr int EPV = 16; };
template <>
struct VolVec<float> { static constexpr int EPV = 4; };

// first / last element > 0 of one aligned 16-byte chunk, as offsets into the chunk; false when it holds none
__device__ __forceinline__ bool chunk_extent(const uint8_t* p, int& lo, int& hi) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(p);
  lo = 16; hi = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] != 0u) {
      const int first = 4 * k + ((__builtin_ctz(v[k])) >> 3), last = 4 * k + ((31 - __builtin_clz(v[k])) >> 3);
      lo = first < lo ? first : lo;
      hi = last > hi ? last : hi;
    }
  }
  return hi >= 0;
}
__device__ __forceinline__ bool chunk_extent(const float* p, int& lo, int& hi) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
  lo = 4; hi = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] > 0.0f) {          // negative values and NaN are background, as (x > 0) says
      lo = k < lo ? k : lo;
      hi = k;
    }
  }
  return hi >= 0;
}

__global__ void box_init_kernel(int* __restrict__ box, int D, int H, int W) {
  if (threadIdx.x < 6) {
    const int ext = threadIdx.x < 2 ? D : threadIdx.x < 4 ? H : W;
    box[threadIdx.x] = (threadIdx.x & 1) ? 0 : ext;     // {min = extent, max + 1 = 0}: nothing found yet
  }
}

// no voxel > 0: the full extent (the reference would fail on the empty crop; documented deviation)
__global__ void box_finish_kernel(int* __restrict__ box, int D, int H, int W) {
  if (threadIdx.x == 0 && box[1] == 0) {
    box[0] = 0; box[1] = D; box[2] = 0; box[3] = H; box[4] = 0; box[5] = W;
  }
}

// Rows of W elements; 2^lg lanes share a row (64 >> lg rows per wave and pass), a lane takes 16-byte chunks of the row's aligned body
// and single elements of its unaligned head and tail.  Per-thread min / max of (d, h, w) over the voxels > 0, folded over the wave by
// shuffles, over the four waves through LDS, and into box[] by six integer atomics per workgroup (order-independent: deterministic).
template <typename T>
__global__ __launch_bounds__(256) void box_reduce_kernel(const T* __restrict__ vol, int* __restrict__ box, int rows, int H, int W, int lg) {
  constexpr int EPV = VolVec<T>::EPV;
  __shared__ int red[4][6];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int L = 1 << lg, sub = lane & (L - 1), slot = lane >> lg;
  const int rows_per_wave = 64 >> lg;
  int dlo = INT_MAX, hlo = INT_MAX, wlo = INT_MAX, dhi = -1, hhi = -1, whi = -1;
  const long long stride = (long long)gridDim.x * 4 * rows_per_wave;
  for (long long r0 = ((long long)blockIdx.x * 4 + wv) * rows_per_wave + slot; r0 < rows; r0 += stride) {
    const int r = (int)r0;
    const T* row = vol + (size_t)r * W;
    int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (int)sizeof(T);
    if (head > W) head = W;
    const int nvec = (W - head) / EPV;
    const int tail0 = head + nvec * EPV;
    int lo = INT_MAX, hi = -1;
    for (int c = sub; c < nvec; c += L) {
      int a, b;
      if (chunk_extent(row + head + c * EPV, a, b)) {
        a += head + c * EPV; b += head + c * EPV;
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
      }
    }
    for (int i = sub; i < head; i += L)
      if (row[i] > (T)0) { lo = i < lo ? i : lo; hi = i > hi ? i : hi; }
    for (int i = tail0 + sub; i < W; i += L)
      if (row[i] > (T)0) { lo = i < lo ? i : lo; hi = i > hi ? i : hi; }
    if (hi >= 0) {
      const int d = r / H, h = r - d * H;
      dlo = d < dlo ? d : dlo; dhi = d > dhi ? d : dhi;
      hlo = h < hlo ? h : hlo; hhi = h > hhi ? h : hhi;
      wlo = lo < wlo ? lo : wlo; whi = hi > whi ? hi : whi;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dlo = min(dlo, __shfl_xor(dlo, o, 64)); dhi = max(dhi, __shfl_xor(dhi, o, 64));
    hlo = min(hlo, __shfl_xor(hlo, o, 64)); hhi = max(hhi, __shfl_xor(hhi, o, 64));
    wlo = min(wlo, __shfl_xor(wlo, o, 64)); whi = max(whi, __shfl_xor(whi, o, 64));
  }
  if (lane == 0) {
    red[wv][0] = dlo; red[wv][1] = dhi; red[wv][2] = hlo; red[wv][3] = hhi; red[wv][4] = wlo; red[wv][5] = whi;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    int v = red[0][k];
    for (int w = 1; w < 4; ++w) v = (k & 1) ? max(v, red[w][k]) : min(v, red[w][k]);
    // Most workgroups cannot move the box any more (after the first few, w and h are at their extremes): an agent-scope load first, the
    // atomic only where it would change the value.  The values move one way only, so a value read late can cost an atomic, never skip one.
    const int cur = __hip_atomic_load(box + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k & 1) {
      if (v + 1 > cur) atomicMax(box + k, v + 1);      // half-open; nothing found: v + 1 = 0, never above cur
    } else if (v < cur) {                               // nothing found: v = INT_MAX, never below cur
      atomicMin(box + k, v);
    }
  }
}

// One axis of F.interpolate(align_corners=False): the two taps and the weight of the second (area_pixel_compute_source_index).
// The source coordinate is ONE fused multiply-add, spelled with the intrinsic so that it is an fma under any -ffp-contract setting: that is
// what ATen's CPU kernel computes (its index / weight table is compiled with contraction; measured: the fused form reproduces torch's
// weights bit for bit at 61 -> 60, 120 -> 64, 130 -> 64, 496 -> 256 and 37 -> 32, a separately rounded multiply and subtract is 1.9e-6
// off at 61 -> 60, the one inexact scale among them -- an ulp of the coordinate, which the weight inherits whole).
__device__ __forceinline__ void lin_taps(int dst, int in, float scale, int& i0, int& i1, float& l1) {
  float src = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i0 = i0 < in - 1 ? i0 : in - 1;
  i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
  l1 = src - (float)i0;       // exact: src and i0 lie within a factor of two of each other, or i0 is 0
}

// Plain arithmetic: the build's -ffp-contract=fast may turn the sum into an fma (two roundings per interpolation instead of three).
// Either form is within the error budget (7 interpolations of at most 3 roundings), and an all-zero neighbourhood gives an exact 0 in both.
__device__ __forceinline__ float lerp(float a, float b, float l1) { return a * (1.0f - l1) + b * l1; }

// One thread per output voxel, consecutive lanes on consecutive stored w of one output row (t, oh).  A wave's tap loads then cover one
// contiguous span of a source row (64 * scale elements: four 128-byte lines for float32 at scale 2, one or two for uint8), and the two
// w taps of a lane fall into the same lines; its store is 256 contiguous bytes.  (Four outputs per thread and a 16-byte store put the
// lanes of a load 4 * scale elements apart -- 16 lines per load instruction at scale 2 -- and measured 2.4 x slower on float32: DESIGN.md section 4.)
// The d and h taps and the box are the row's; they are a few dozen VALU instructions beside eight loads and are recomputed per thread.
template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(const T* __restrict__ vol, int D, int H, int W, const int* __restrict__ box,
                                                       float* __restrict__ out, int Tn, int OH, int OW, unsigned nthreads,
                                                       int flip_d, int flip_w, int normalize, float sub, float div) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= nthreads) return;
  const int row = (int)(idx / (unsigned)OW), ws = (int)(idx - (unsigned)row * (unsigned)OW);
  const int ts = row / OH, oh = row - ts * OH;
  int d0 = 0, d1 = D, h0 = 0, h1 = H, w0 = 0, w1 = W;
  if (box != nullptr) {       // clamped into the volume: whatever the six ints hold, every tap stays inside it
    d0 = min(max(box[0], 0), D - 1); d1 = min(max(box[1], d0 + 1), D);
    h0 = min(max(box[2], 0), H - 1); h1 = min(max(box[3], h0 + 1), H);
    w0 = min(max(box[4], 0), W - 1); w1 = min(max(box[5], w0 + 1), W);
  }
  const int Din = d1 - d0, Hin = h1 - h0, Win = w1 - w0;
  const float sd = (float)Din / (float)Tn, sh = (float)Hin / (float)OH, sw = (float)Win / (float)OW;
  int da, db, ha, hb, wa, wb;
  float ld, lh, lw;
  lin_taps(flip_d ? Tn - 1 - ts : ts, Din, sd, da, db, ld);
  lin_taps(oh, Hin, sh, ha, hb, lh);
  lin_taps(flip_w ? OW - 1 - ws : ws, Win, sw, wa, wb, lw);
  const T* r00 = vol + ((size_t)(d0 + da) * H + (h0 + ha)) * W + w0;
  const T* r01 = vol + ((size_t)(d0 + da) * H + (h0 + hb)) * W + w0;
  const T* r10 = vol + ((size_t)(d0 + db) * H + (h0 + ha)) * W + w0;
  const T* r11 = vol + ((size_t)(d0 + db) * H + (h0 + hb)) * W + w0;
  const float x000 = (float)r00[wa], x001 = (float)r00[wb], x010 = (float)r01[wa], x011 = (float)r01[wb];
  const float x100 = (float)r10[wa], x101 = (float)r10[wb], x110 = (float)r11[wa], x111 = (float)r11[wb];
  float v = lerp(lerp(lerp(x000, x001, lw), lerp(x010, x011, lw), lh), lerp(lerp(x100, x101, lw), lerp(x110, x111, lw), lh), ld);
  if (normalize && v != 0.0f) v = (v - sub) / div;
  __builtin_nontemporal_store(v, out + (size_t)row * OW + ws);
}

template <typename T>
static int launch_box(const void* vol, int D, int H, int W, int* box, hipStream_t st) {
  const int rows = D * H;
  const long long chunks = ((long long)W * (long long)sizeof(T)) / 16;
  int lg = 0;
  while (lg < 6 && (1LL << lg) < chunks) ++lg;
  const int rows_per_block = 4 * (64 >> lg);
  long long blocks = ((long long)rows + rows_per_block - 1) / rows_per_block;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(64), 0, st, box, D, H, W);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(box_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const T*>(vol), box, rows, H, W, lg);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(box_finish_kernel, dim3(1), dim3(64), 0, st, box, D, H, W);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int launch_resample(const void* vol, int D, int H, int W, const int* box, float* out, int Tn, int OH, int OW, int flip_d,
                           int flip_w, int normalize, float sub, float div, hipStream_t st) {
  const long long nthreads = (long long)Tn * OH * OW;
  if (nthreads > 0x7fffffffLL) return -1;
  const long long blocks = (nthreads + 255) / 256;
  hipLaunchKernelGGL(resample_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const T*>(vol), D, H, W, box, out, Tn, OH,
                     OW, (unsigned)nthreads, flip_d, flip_w, normalize, sub, div);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_volume_box(const void* vol, int dtype, int D, int H, int W, int* box6, void* stream) {
  OCTMAE_CHECK_ARG(vol && box6 && D > 0 && H > 0 && W > 0);
  OCTMAE_CHECK_ARG((long long)D * H <= 0x7fffffffLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == 0) return launch_box<uint8_t>(vol, D, H, W, box6, st);
  if (dtype == 1) return launch_box<float>(vol, D, H, W, box6, st);
  return -2;
}

extern "C" int octmae_volume_resample(const void* vol, int dtype, int D, int H, int W, const int* box6, float* out, int T, int OH, int OW,
                                      int flip_d, int flip_w, int normalize, float subtrahend, float divisor, void* stream) {
  OCTMAE_CHECK_ARG(vol && out && D > 0 && H > 0 && W > 0 && T > 0 && OH > 0 && OW > 0);
  OCTMAE_CHECK_ARG((long long)T * OH <= 0x7fffffffLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == 0)
    return launch_resample<uint8_t>(vol, D, H, W, box6, out, T, OH, OW, flip_d != 0, flip_w != 0, normalize != 0, subtrahend, divisor, st);
  if (dtype == 1)
    return launch_resample<float>(vol, D, H, W, box6, out, T, OH, OW, flip_d != 0, flip_w != 0, normalize != 0, subtrahend, divisor, st);
  return -2;
}
