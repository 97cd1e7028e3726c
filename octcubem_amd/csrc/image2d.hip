// 2-D image transforms in front of the 2-D towers: the reference's torchvision-on-PIL chains
//   Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:313-317    Resize((S, S), interpolation=3) -> ToTensor -> Normalize
//   OCTCube/main_pretrain_oph_new.py:151-156, OCTCube/main_pretrain.py:133-137
//                                                                       RandomResizedCrop(S, interpolation=3) -> RandomHorizontalFlip -> ToTensor -> Normalize
//   OCTCube/util/PatientDataset_inhouse_pretrain.py:247-252             frame.resize((512, h))
// as ONE launch over n equally shaped uint8 images: crop (a pointer offset) -> Pillow's two-pass 8-bit bicubic resize, bit for bit ->
// horizontal flip (an index reversal of the store) -> ToTensor + Normalize (a 3 x 256 table).
//
// Pillow's 8-bit resize (Resample.c) is an integer algorithm: per axis, double-precision bicubic weights over a window of
// 2 * ceil(2 * max(scale, 1)) + 1 taps, normalised and rounded to 22-bit fixed point; a horizontal pass whose sums are rounded and
// clamped to uint8; then a vertical pass over those uint8 values, rounded and clamped again.  The coefficient rule lives in
// image2d_plan.hpp (host and device compile the same text, without contraction).
//
// A workgroup owns th x tw output pixels (image2d_plan.hpp picks th).  Prologue: one thread per output column and one per output row
// of the tile compute that index's window and coefficients into LDS.  Stage A: the horizontal pass of the input rows that the tile's
// row windows span, for the tile's columns, from global memory into uint8 LDS -- the intermediate image never goes to HBM.  Stage B:
// the vertical pass from LDS, the clamp, the table, and stores in which consecutive lanes write consecutive elements of one output
// row.  Independent of the 16-bit operand type: the two builds of the library hold the same code.
//   bytes/image: the crop read (1 + rows / (th * scale_y)) times (row windows of neighbouring tiles overlap), the output written once
#include "common.hpp"
#include "image2d_plan.hpp"
#include "../../include/octmae.h"

namespace octmae {

struct ImgParams {
  const uint8_t* src;        // first pixel of image 0's crop
  void* dst;
  const float* lut;
  size_t img_stride;         // bytes between images of src
  int row_stride;            // bytes between rows of src (W * C)
  int ih, iw;                // the crop's extent
  int OH, OW, flip;
  int th, tw, ksx, ksy, rows;
  int tiles_x, tiles_y;
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> IMG_PRECISION_BITS;        // arithmetic shift, as Pillow's clip8
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

template <int C, bool LUT>
__global__ __launch_bounds__(IMG_THREADS) void image_resample_kernel(const ImgParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char img_lds[];
  const int th = p.th, tw = p.tw;
  float* s_lut = reinterpret_cast<float*>(img_lds);
  int* s_kx = reinterpret_cast<int*>(img_lds + IMG_LUT_BYTES);        // [ksx][tw]
  int* s_xmin = s_kx + p.ksx * tw;
  int* s_xmax = s_xmin + tw;
  int* s_ky = s_xmax + tw;                                             // [ksy][th]
  int* s_ymin = s_ky + p.ksy * th;
  int* s_ymax = s_ymin + th;
  uint8_t* s_tmp = reinterpret_cast<uint8_t*>(s_ymax + th);            // [rows][tw * C]

  const int tid = threadIdx.x;
  const int tx = blockIdx.x % p.tiles_x, t = blockIdx.x / p.tiles_x;
  const int ty = t % p.tiles_y, img = t / p.tiles_y;
  const int x0 = tx * tw, y0 = ty * th;
  const int ncol = min(tw, p.OW - x0), nrow = min(th, p.OH - y0);

  // ---- prologue: wave 0 the columns, wave 1 the rows (th <= 32), everybody the table
  if (tid < ncol) {
    int lo, n;
    img_coeffs(img_axis(p.iw, p.OW), p.iw, x0 + tid, s_kx + tid, tw, lo, n);
    s_xmin[tid] = lo;
    s_xmax[tid] = n;
  } else if (tid >= 64 && tid - 64 < nrow) {
    const int r = tid - 64;
    int lo, n;
    img_coeffs(img_axis(p.ih, p.OH), p.ih, y0 + r, s_ky + r, th, lo, n);
    s_ymin[r] = lo;
    s_ymax[r] = n;
  }
  if (LUT)
    for (int i = tid; i < 3 * 256; i += IMG_THREADS) s_lut[i] = p.lut[i];
  __syncthreads();

  // the windows move monotonically with the output index: the tile's rows span [first row's ymin, last row's ymin + ymax)
  const int row0 = s_ymin[0];
  const int rows = min(s_ymin[nrow - 1] + s_ymax[nrow - 1] - row0, p.rows);      // == without the min: the host planned with the same rule
  const uint8_t* src = p.src + (size_t)img * p.img_stride + (size_t)row0 * p.row_stride;

  // ---- stage A: horizontal pass, consecutive lanes on consecutive (column, channel) of one input row
  const int rowlen = ncol * C, tmp_stride = tw * C;
  for (int i = tid; i < rows * rowlen; i += IMG_THREADS) {
    const int r = i / rowlen, j = i - r * rowlen;
    const int col = j / C, c = j - col * C;
    const uint8_t* s = src + (size_t)r * p.row_stride + s_xmin[col] * C + c;
    const int n = s_xmax[col];
    int acc = 1 << (IMG_PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) acc += (int)s[x * C] * s_kx[x * tw + col];
    s_tmp[r * tmp_stride + j] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // ---- stage B: vertical pass from LDS, consecutive lanes on consecutive columns of one (output row, channel)
  for (int i = tid; i < nrow * C * ncol; i += IMG_THREADS) {
    const int col = i % ncol, u = i / ncol;
    const int c = u % C, r = u / C;
    const int n = s_ymax[r], r0 = s_ymin[r] - row0;
    const uint8_t* s = s_tmp + col * C + c;
    int acc = 1 << (IMG_PRECISION_BITS - 1);
    for (int y = 0; y < n; ++y) acc += (int)s[min(r0 + y, rows - 1) * tmp_stride] * s_ky[y * th + r];
    const int v = clip8(acc);
    const int oy = y0 + r, ox = p.flip ? p.OW - 1 - (x0 + col) : x0 + col;
    if (LUT) {
      float* out = static_cast<float*>(p.dst);
      if (C == 1) {            // convert("RGB") of a grey image: three equal channels through the resize, three table rows here
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          __builtin_nontemporal_store(s_lut[ch * 256 + v], out + (((size_t)img * 3 + ch) * p.OH + oy) * p.OW + ox);
      } else {
        __builtin_nontemporal_store(s_lut[c * 256 + v], out + (((size_t)img * 3 + c) * p.OH + oy) * p.OW + ox);
      }
    } else {
      static_cast<uint8_t*>(p.dst)[(((size_t)img * p.OH + oy) * p.OW + ox) * C + c] = (uint8_t)v;
    }
  }
}

template <int C, bool LUT>
static int launch_image(const ImgParams& p, unsigned blocks, int lds_bytes, hipStream_t st) {
  hipLaunchKernelGGL((image_resample_kernel<C, LUT>), dim3(blocks), dim3(IMG_THREADS), (size_t)lds_bytes, st, p);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

// the argument rules shared by the entry point and the plan query; the crop's extent comes back in ih, iw
static bool image_geometry_ok(int H, int W, int C, int top, int left, int ch, int cw, int OH, int OW, int& ih, int& iw) {
  if (H < 1 || W < 1 || OH < 1 || OW < 1 || (C != 1 && C != 3)) return false;
  if (top < 0 || left < 0 || ch < 0 || cw < 0 || (ch == 0) != (cw == 0)) return false;
  if (ch == 0) {
    if (top != 0 || left != 0) return false;
    ih = H; iw = W;
    return true;
  }
  if ((long long)top + ch > H || (long long)left + cw > W) return false;
  ih = ch; iw = cw;
  return true;
}

}  // namespace octmae
using namespace octmae;

extern "C" int octmae_image_resample_plan(int H, int W, int C, int ch, int cw, int OH, int OW, int* tile_h, int* lds_bytes) {
  int ih, iw;
  OCTMAE_CHECK_ARG(tile_h && lds_bytes);
  OCTMAE_CHECK_ARG(image_geometry_ok(H, W, C, 0, 0, ch, cw, OH, OW, ih, iw));
  ImgPlan pl;
  OCTMAE_CHECK_ARG(plan_image(ih, iw, C, OH, OW, pl));
  *tile_h = pl.th;
  *lds_bytes = pl.lds_bytes;
  return 0;
}

extern "C" int octmae_image_resample(const void* src, int n, int H, int W, int C, int top, int left, int ch, int cw, int OH, int OW,
                                     int flip_w, const float* lut, void* dst, void* stream) {
  int ih, iw;
  OCTMAE_CHECK_ARG(src && dst && n > 0);
  OCTMAE_CHECK_ARG(image_geometry_ok(H, W, C, top, left, ch, cw, OH, OW, ih, iw));
  OCTMAE_CHECK_ARG((long long)W * C <= 0x7fffffffLL);
  ImgPlan pl;
  OCTMAE_CHECK_ARG(plan_image(ih, iw, C, OH, OW, pl));
  ImgParams p;
  p.row_stride = W * C;
  p.img_stride = (size_t)H * p.row_stride;
  p.src = static_cast<const uint8_t*>(src) + (size_t)top * p.row_stride + (size_t)left * C;
  p.dst = dst;
  p.lut = lut;
  p.ih = ih; p.iw = iw;
  p.OH = OH; p.OW = OW; p.flip = flip_w != 0;
  p.th = pl.th; p.tw = pl.tw; p.ksx = pl.ksx; p.ksy = pl.ksy; p.rows = pl.rows;
  p.tiles_x = (OW + pl.tw - 1) / pl.tw;
  p.tiles_y = (OH + pl.th - 1) / pl.th;
  const long long blocks = (long long)p.tiles_x * p.tiles_y * n;
  OCTMAE_CHECK_ARG(blocks <= 0x7fffffffLL);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (C == 1) return lut ? launch_image<1, true>(p, (unsigned)blocks, pl.lds_bytes, st) : launch_image<1, false>(p, (unsigned)blocks, pl.lds_bytes, st);
  return lut ? launch_image<3, true>(p, (unsigned)blocks, pl.lds_bytes, st) : launch_image<3, false>(p, (unsigned)blocks, pl.lds_bytes, st);
}
