// ConvNeXt layer kernels (the SLIViT baseline's feature extractor, OCTCube/model_slivit_baseline.py through HF ConvNextLayer):
// the depthwise 7x7 convolution with its two gradients, and the per-channel layer scale around the residual add.
//
// Layout: channels-last fp32 [B][H][W][C], the [M = B H W][C] rows the row LayerNorm and the GEMMs take.  Lanes run along C, four
// channels (16 bytes) per lane, so every global access of a wave is a run of whole pixels' channel vectors.  Nothing here rounds to
// 16 bits except dbranch of octmae_layer_scale_bwd, which IS the 16-bit operand of the pwconv2 gradients.
//
// Convolution tile: a workgroup owns 8 x 16 output pixels of 32 channels and stages the 14 x 22 input pixels around them (the 3-pixel
// halo; zero outside the map) and the 49 x 32 filter taps in LDS (45 KiB).  A thread owns one pixel column of one channel vector: per
// filter column it reads the 14 input rows once and feeds 7 x 8 multiply-adds from them, so an output element costs 49 fused multiply-adds
// and 49 * 21 / 56 = 18 LDS words, not 49 global loads.  Global traffic per output element: 4 B written, 4 B read algorithmically;
// with the halo (14 * 22) / (8 * 16) = 2.4 words leave the caches per element, the overlap of neighbouring tiles coming from L2.
// The input gradient is the same kernel with the taps stored back to front (FLIP).
//
// Weight gradient: the same tiles of x (with halo) and dz; a thread owns (channel vector, filter row i, quarter of the tile's rows)
// and keeps the 7 taps of its filter row in registers while it slides along the pixel rows.  A workgroup walks tiles g, g + G, ... in that
// order, folds its four row quarters in order, and leaves 50 x C partial sums (49 taps + the bias) in the workspace; a second launch adds the
// G partials in order into gw / gb.  No float atomics anywhere: the order of every addition is fixed by the shape, two runs are bit-equal.
//
// This file is compiled with -ffp-contract=off (Makefile): out = res + gamma * branch and dbranch = lp(gamma * dout) are stated as one
// multiply and one add / one rounding each, bit-equal to the fp32 mul and add they replace; the convolution sums call fmaf explicitly.
#include "common.hpp"
#include "../../include/octmae.h"

namespace octmae {
namespace {

constexpr int DW_TH = 8, DW_TW = 16;            // output pixels per tile
constexpr int DW_CB = 32, DW_CV = DW_CB / 4;    // channels per tile; channel vectors (float4) = lanes along C
constexpr int DW_IH = DW_TH + 6, DW_IW = DW_TW + 6;
constexpr int DW_NT = DW_CV * DW_TW;            // 128 threads: (channel vector, pixel column)
constexpr int DW_WS = DW_CV + 1;                // float4 stride of a tap row in LDS (one slot of padding against the transposing fill)
constexpr int DWW_NT = 256;                     // weight gradient: 8 channel vectors x 7 filter rows x 4 row quarters = 224 active
constexpr int DWW_ROWS = 50;                    // 49 taps + the bias sum per channel

__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the (DW_TH + 6) x (DW_TW + 6) pixels around tile (h0, w0) of sample b, channels c0 .. c0 + 31: zero outside the map / beyond C.
// Every thread requests all its pieces (halo_request) before it stores the first (halo_commit): one memory latency per tile, not one
// per piece.
constexpr int DW_HALO = DW_IH * DW_IW * DW_CV;
template <int NT>
struct HaloRegs {
  static constexpr int NL = (DW_HALO + NT - 1) / NT;
  float4 v[NL];
};
template <int NT>
__device__ __forceinline__ void halo_request(HaloRegs<NT>& r, const float* __restrict__ x, int b, int h0, int w0, int c0, int H, int W, int C) {
#pragma unroll
  for (int k = 0; k < HaloRegs<NT>::NL; ++k) {
    const int e = threadIdx.x + k * NT;
    const int cv = e % DW_CV, p = e / DW_CV;
    const int h = h0 + p / DW_IW - 3, w = w0 + p % DW_IW - 3, c = c0 + cv * 4;
    r.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < DW_HALO && h >= 0 && h < H && w >= 0 && w < W && c < C) r.v[k] = *reinterpret_cast<const float4*>(x + (((size_t)b * H + h) * W + w) * C + c);
  }
}
template <int NT>
__device__ __forceinline__ void halo_commit(const HaloRegs<NT>& r, float4* s_in) {
#pragma unroll
  for (int k = 0; k < HaloRegs<NT>::NL; ++k) {
    const int e = threadIdx.x + k * NT;
    if (e < DW_HALO) s_in[e] = r.v[k];
  }
}

// out[b,h,w,c] = addc[c] + adde[b,h,w,c] + sum_ij wt[c, i, j] * in[b, h + i - 3, w + j - 3, c]   (FLIP: wt[c, 6 - i, 6 - j]); the tap
// sum is formed first and the optional addends are added to it, adde last: with adde the result is (result without) + adde exactly.
template <bool FLIP>
__global__ __launch_bounds__(DW_NT) void dwconv7_kernel(const float* __restrict__ in, const float* __restrict__ wt,
                                                         const float* __restrict__ addc, const float* __restrict__ adde,
                                                         float* __restrict__ out, int H, int W, int C, int tilesH, int tilesW) {
  __shared__ float4 s_in[DW_IH * DW_IW * DW_CV];
  __shared__ float4 s_w[49 * DW_WS];
  int t = blockIdx.x;
  const int w0 = (t % tilesW) * DW_TW; t /= tilesW;
  const int h0 = (t % tilesH) * DW_TH;
  const int b = t / tilesH;
  const int c0 = blockIdx.y * DW_CB;
  constexpr int NW = (49 * DW_CB + DW_NT - 1) / DW_NT;
  float wv[NW];                                                     // wt[c][49]: consecutive e are consecutive words of global memory
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int e = threadIdx.x + k * DW_NT;
    wv[k] = (e < 49 * DW_CB && c0 + e / 49 < C) ? wt[(size_t)c0 * 49 + e] : 0.f;
  }
  HaloRegs<DW_NT> halo;
  halo_request(halo, in, b, h0, w0, c0, H, W, C);
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int e = threadIdx.x + k * DW_NT;
    const int cl = e / 49, tap = e % 49;
    if (e < 49 * DW_CB) reinterpret_cast<float*>(s_w)[(FLIP ? 48 - tap : tap) * (DW_WS * 4) + cl] = wv[k];
  }
  halo_commit(halo, s_in);
  __syncthreads();
  const int cv = threadIdx.x % DW_CV, col = threadIdx.x / DW_CV;
  float4 acc[DW_TH];
#pragma unroll
  for (int r = 0; r < DW_TH; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
  for (int j = 0; j < 7; ++j) {
    float4 v[DW_IH];
#pragma unroll
    for (int r = 0; r < DW_IH; ++r) v[r] = s_in[(r * DW_IW + col + j) * DW_CV + cv];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const float4 w4 = s_w[(i * 7 + j) * DW_WS + cv];
#pragma unroll
      for (int r = 0; r < DW_TH; ++r) acc[r] = fma4(w4, v[r + i], acc[r]);
    }
  }
  const int w = w0 + col, c = c0 + cv * 4;
  if (w >= W || c >= C) return;
  float4 bc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (addc != nullptr) bc = *reinterpret_cast<const float4*>(addc + c);
#pragma unroll
  for (int r = 0; r < DW_TH; ++r) {
    const int h = h0 + r;
    if (h < H) {
      const size_t o = (((size_t)b * H + h) * W + w) * C + c;
      float4 y = acc[r];
      if (addc != nullptr) y = add4(y, bc);
      if (adde != nullptr) y = add4(y, *reinterpret_cast<const float4*>(adde + o));
      *reinterpret_cast<float4*>(out + o) = y;
    }
  }
}

// ws[g][k][c], k < 49: sum over the tiles g, g + G, ... of dz[b,h,w,c] * x[b, h + i - 3, w + j - 3, c] (k = 7 i + j);  k = 49: sum of dz
__global__ __launch_bounds__(DWW_NT) void dwconv7_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ ws,
                                                               int H, int W, int C, int tilesH, int tilesW, int ntiles) {
  __shared__ float4 s_x[DW_IH * DW_IW * DW_CV];       // reused for the fold of the four row quarters (4 * 50 * 8 float4 < 14 * 22 * 8)
  __shared__ float4 s_d[DW_TH * DW_TW * DW_CV];
  static_assert(4 * DWW_ROWS * DW_CV <= DW_IH * DW_IW * DW_CV, "fold buffer");
  const int c0 = blockIdx.y * DW_CB;
  const int tid = threadIdx.x;
  const bool active = tid < DW_CV * 7 * 4;
  const int cv = tid % DW_CV, fi = (tid / DW_CV) % 7, q = tid / (DW_CV * 7);
  float4 acc[7], accb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < 7; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int t = tile;
    const int w0 = (t % tilesW) * DW_TW; t /= tilesW;
    const int h0 = (t % tilesH) * DW_TH;
    const int b = t / tilesH;
    __syncthreads();                                   // the previous tile's readers are done
    HaloRegs<DWW_NT> halo;
    halo_request(halo, x, b, h0, w0, c0, H, W, C);
    for (int e = tid; e < DW_TH * DW_TW * DW_CV; e += DWW_NT) {
      const int v = e % DW_CV, p = e / DW_CV;
      const int h = h0 + p / DW_TW, w = w0 + p % DW_TW, c = c0 + v * 4;
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
      if (h < H && w < W && c < C) d = *reinterpret_cast<const float4*>(dz + (((size_t)b * H + h) * W + w) * C + c);
      s_d[e] = d;
    }
    halo_commit(halo, s_x);
    __syncthreads();
    if (active) {
#pragma unroll 1
      for (int rr = 0; rr < DW_TH / 4; ++rr) {
        const int r = q + 4 * rr;
        float4 xr[DW_IW];
#pragma unroll
        for (int k = 0; k < DW_IW; ++k) xr[k] = s_x[((r + fi) * DW_IW + k) * DW_CV + cv];
#pragma unroll
        for (int w = 0; w < DW_TW; ++w) {
          const float4 d = s_d[(r * DW_TW + w) * DW_CV + cv];
#pragma unroll
          for (int j = 0; j < 7; ++j) acc[j] = fma4(d, xr[w + j], acc[j]);
          if (fi == 0) accb = add4(accb, d);
        }
      }
    }
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int j = 0; j < 7; ++j) s_x[(q * DWW_ROWS + fi * 7 + j) * DW_CV + cv] = acc[j];
    if (fi == 0) s_x[(q * DWW_ROWS + 49) * DW_CV + cv] = accb;
  }
  __syncthreads();
  for (int e = tid; e < DWW_ROWS * DW_CV; e += DWW_NT) {
    const int v = e % DW_CV, k = e / DW_CV, c = c0 + v * 4;
    if (c >= C) continue;
    float4 s = s_x[(0 * DWW_ROWS + k) * DW_CV + v];
    s = add4(s, s_x[(1 * DWW_ROWS + k) * DW_CV + v]);
    s = add4(s, s_x[(2 * DWW_ROWS + k) * DW_CV + v]);
    s = add4(s, s_x[(3 * DWW_ROWS + k) * DW_CV + v]);
    *reinterpret_cast<float4*>(ws + ((size_t)blockIdx.x * DWW_ROWS + k) * C + c) = s;
  }
}

// gw[c][k] += sum_g ws[g][k][c] (k < 49), gb[c] += sum_g ws[g][49][c]: g ascending, one thread per (k, c)
__global__ __launch_bounds__(256) void dwconv7_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ gw, float* __restrict__ gb, int G, int C) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= DWW_ROWS * C) return;
  const int c = e % C, k = e / C;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += ws[((size_t)g * DWW_ROWS + k) * C + c];
  if (k < 49) gw[(size_t)c * 49 + k] += s; else gb[c] += s;
}

__global__ __launch_bounds__(256) void layer_scale_fwd_kernel(const float* __restrict__ res, const float* __restrict__ branch, const float* __restrict__ gamma,
                                                             float* __restrict__ out, size_t n4, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 g = *reinterpret_cast<const float4*>(gamma + (i * 4) % (size_t)C);
  const float4 r = reinterpret_cast<const float4*>(res)[i], v = reinterpret_cast<const float4*>(branch)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(r.x + g.x * v.x, r.y + g.y * v.y, r.z + g.z * v.z, r.w + g.w * v.w);
}

// A workgroup of 256 = RP rows x CVB channel vectors (RP * CVB <= 256) walks rows (g RP + part), + G RP, ...: dbranch for every row it
// meets, and (with ws) its column sums of dout * branch, the RP parts folded in order.
__global__ __launch_bounds__(256) void layer_scale_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ branch, const float* __restrict__ gamma,
                                                             bf16_t* __restrict__ dbranch, float* __restrict__ ws, int M, int C, int CVB, int RP) {
  __shared__ float4 s_red[256];
  const int tid = threadIdx.x;
  const int cvl = tid % CVB, part = tid / CVB;
  const int c = (blockIdx.y * CVB + cvl) * 4;
  const bool active = part < RP && c < C;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    const float4 g = *reinterpret_cast<const float4*>(gamma + c);
    for (size_t row = (size_t)blockIdx.x * RP + part; row < (size_t)M; row += (size_t)gridDim.x * RP) {
      const size_t o = row * C + c;
      const float4 d = *reinterpret_cast<const float4*>(dout + o);
      u32x2 p;
      p[0] = pack2bf(g.x * d.x, g.y * d.y);
      p[1] = pack2bf(g.z * d.z, g.w * d.w);
      *reinterpret_cast<u32x2*>(dbranch + o) = p;
      if (ws != nullptr) acc = fma4(d, *reinterpret_cast<const float4*>(branch + o), acc);
    }
  }
  if (ws == nullptr) return;
  s_red[tid] = acc;
  __syncthreads();
  if (active && part == 0) {
    float4 s = s_red[cvl];
    for (int p = 1; p < RP; ++p) s = add4(s, s_red[p * CVB + cvl]);
    *reinterpret_cast<float4*>(ws + (size_t)blockIdx.x * C + c) = s;
  }
}

__global__ __launch_bounds__(256) void colfold_kernel(const float* __restrict__ ws, float* __restrict__ dst, int G, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += ws[(size_t)g * C + c];
  dst[c] += s;
}

struct DwShape {
  int tilesH, tilesW, cblocks;
  long long ntiles;
};
// false: not a shape these kernels take (C % 8, empty, or beyond the grid / 32-bit ranges)
inline bool dw_shape(int B, int H, int W, int C, DwShape* s) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return false;
  s->tilesH = (H + DW_TH - 1) / DW_TH;
  s->tilesW = (W + DW_TW - 1) / DW_TW;
  s->cblocks = (C + DW_CB - 1) / DW_CB;
  s->ntiles = (long long)B * s->tilesH * s->tilesW;
  return s->ntiles <= 0x7fffffffLL && s->cblocks <= 65535 && (long long)B * H * W <= 0x7fffffffLL;
}
inline int dw_wgrad_groups(const DwShape& s) {
  int cap = 1024 / s.cblocks;
  if (cap < 1) cap = 1;
  return (int)(s.ntiles < cap ? s.ntiles : cap);
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct LsShape {
  int CVB, RP, ncb, G;
};
inline bool ls_shape(int M, int C, LsShape* s) {
  if (M <= 0 || C <= 0 || C % 8 != 0) return false;
  const int CV = C / 4;
  s->CVB = CV < 256 ? CV : 256;
  s->RP = 256 / s->CVB;
  s->ncb = (CV + s->CVB - 1) / s->CVB;
  if (s->ncb > 65535) return false;
  int cap = 1024 / s->ncb;
  if (cap < 1) cap = 1;
  const int need = (M + s->RP - 1) / s->RP;
  s->G = need < cap ? need : cap;
  return true;
}

}  // namespace
}  // namespace octmae
using namespace octmae;

extern "C" int octmae_dwconv7_fwd(const float* x, const float* wt, const float* bias, float* z, int B, int H, int W, int C, void* stream) {
  DwShape s;
  OCTMAE_CHECK_ARG(x && wt && bias && z && dw_shape(B, H, W, C, &s));
  OCTMAE_CHECK_ARG(aligned16(x) && aligned16(z) && aligned16(bias));
  hipLaunchKernelGGL(dwconv7_kernel<false>, dim3((unsigned)s.ntiles, s.cblocks), dim3(DW_NT), 0, reinterpret_cast<hipStream_t>(stream), x, wt,
                     bias, (const float*)nullptr, z, H, W, C, s.tilesH, s.tilesW);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_dwconv7_bwd_input(const float* dz, const float* wt, const float* dres, float* dx, int B, int H, int W, int C, void* stream) {
  DwShape s;
  OCTMAE_CHECK_ARG(dz && wt && dx && dw_shape(B, H, W, C, &s));
  OCTMAE_CHECK_ARG(aligned16(dz) && aligned16(dx) && aligned16(dres));
  hipLaunchKernelGGL(dwconv7_kernel<true>, dim3((unsigned)s.ntiles, s.cblocks), dim3(DW_NT), 0, reinterpret_cast<hipStream_t>(stream), dz, wt,
                     (const float*)nullptr, dres, dx, H, W, C, s.tilesH, s.tilesW);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_dwconv7_bwd_weight_ws_floats(int B, int H, int W, int C) {
  DwShape s;
  if (!dw_shape(B, H, W, C, &s)) return -1;
  const long long n = (long long)dw_wgrad_groups(s) * DWW_ROWS * C;
  return n <= 0x7fffffffLL ? (int)n : -1;
}

extern "C" int octmae_dwconv7_bwd_weight(const float* dz, const float* x, float* gw, float* gb, float* ws, int B, int H, int W, int C, void* stream) {
  DwShape s;
  OCTMAE_CHECK_ARG(dz && x && gw && gb && ws && dw_shape(B, H, W, C, &s));
  OCTMAE_CHECK_ARG(aligned16(dz) && aligned16(x) && aligned16(ws) && octmae_dwconv7_bwd_weight_ws_floats(B, H, W, C) > 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int G = dw_wgrad_groups(s);
  hipLaunchKernelGGL(dwconv7_wgrad_kernel, dim3(G, s.cblocks), dim3(DWW_NT), 0, st, dz, x, ws, H, W, C, s.tilesH, s.tilesW, (int)s.ntiles);
  OCTMAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(dwconv7_wgrad_fold_kernel, dim3((DWW_ROWS * C + 255) / 256), dim3(256), 0, st, ws, gw, gb, G, C);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_layer_scale_fwd(const float* res, const float* branch, const float* gamma, float* out, int M, int C, void* stream) {
  OCTMAE_CHECK_ARG(res && branch && gamma && out && M > 0 && C > 0 && C % 8 == 0);
  OCTMAE_CHECK_ARG(aligned16(res) && aligned16(branch) && aligned16(gamma) && aligned16(out));
  const size_t n4 = (size_t)M * C / 4;
  OCTMAE_CHECK_ARG((n4 + 255) / 256 <= 0x7fffffffULL);
  hipLaunchKernelGGL(layer_scale_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), res, branch,
                     gamma, out, n4, C);
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_layer_scale_bwd_ws_floats(int M, int C) {
  LsShape s;
  if (!ls_shape(M, C, &s)) return -1;
  return s.G * C;
}

extern "C" int octmae_layer_scale_bwd(const float* dout, const float* branch, const float* gamma, void* dbranch_lp, float* ggamma, float* ws,
                                      int M, int C, void* stream) {
  LsShape s;
  OCTMAE_CHECK_ARG(dout && gamma && dbranch_lp && ls_shape(M, C, &s));
  OCTMAE_CHECK_ARG(ggamma == nullptr || (branch != nullptr && ws != nullptr));
  OCTMAE_CHECK_ARG(aligned16(dout) && aligned16(gamma) && aligned16(branch) && aligned16(ws) && (reinterpret_cast<uintptr_t>(dbranch_lp) & 7) == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(layer_scale_bwd_kernel, dim3(s.G, s.ncb), dim3(256), 0, st, dout, branch, gamma, reinterpret_cast<bf16_t*>(dbranch_lp),
                     ggamma != nullptr ? ws : (float*)nullptr, M, C, s.CVB, s.RP);
  OCTMAE_LAUNCH_CHECK();
  if (ggamma != nullptr) {
    hipLaunchKernelGGL(colfold_kernel, dim3((C + 255) / 256), dim3(256), 0, st, ws, ggamma, s.G, C);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
