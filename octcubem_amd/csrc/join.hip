// The join between the COEM towers and the classification head (retinal-COEM/src/open_clip/model.py:741-809): per sample the
// reference runs F.normalize on each tower output, zeros_like for an absent modality, cat, and ClassificationHead.input_norm =
// LayerNorm(M * D) -- seven ATen launches forward, more backward.  Here: one kernel each way, and fc1 gets its 16-bit operand directly.
//
//   n_k = f_k / max(||f_k||_2, 1e-12)  (zeros where modality k is absent)      y = LayerNorm(concat_k n_k; gamma, beta, eps)
//
// One wave owns one sample: lane t holds float4 chunks t, t + 64, ... of each modality slice (M * D <= 4096 floats: at most 64 per
// lane), the M norms and the LayerNorm statistics are wave reductions over those registers (DPP, no LDS round trip for the row).
//   fwd bytes / sample: 4 P D (f, P = modalities present) read, 4 M D (n_out) + 2 M D (y) written
//   bwd bytes / sample: 4 M D (dy) + 4 P D (f) [+ 4 P D (dn_extra)] read, 4 P D (df) written; dgamma / dbeta through per-workgroup
//   partials in the caller's workspace folded in a fixed order by a second small kernel, as layernorm.hip does (no float atomics).
//
// Scaling of the norm: ||f||^2 as a plain f32 sum of squares leaves the format for |f| around 1e-20 (squares below the smallest
// normal) and 1e18 (the sum above the largest).  The squares are therefore taken of f * s, s = 2^(127 - E) with E the exponent field
// of max |f| over the slice: a power of two, so f * s is exact and its largest element lies in [1, 2) -- the sum lies in [1, 4 D).
// n = (f * s) * (1 / sqrt(sum)) never forms the norm itself; the norm sqrt(sum) / s is formed once, only to compare it with 1e-12
// (below it: n = f * 1e12, what F.normalize's clamp gives).  inv_norm = s / sqrt(sum) (or 1e12) is what the backward multiplies with.
#include "rowwave.hpp"
#include "../../include/octmae.h"

namespace octmae {

constexpr int JOIN_MAXM = 3;
constexpr float JOIN_NORM_EPS = 1e-12f;      // F.normalize's eps
constexpr float JOIN_INV_EPS = 1e12f;        // 1 / eps: what a row below the clamp is multiplied with, forward and backward

struct JoinSrc {
  const float* p[JOIN_MAXM];
};

__device__ __forceinline__ float join_ld_inv_s(float amax, float& s) {
  const uint32_t E = (__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu;
  const uint32_t fs = E >= 254u ? 1u : 254u - E;          // s = 2^(127 - E); E = 0 (zero, subnormal): 2^127; E >= 254: 2^-126
  const uint32_t fi = E < 1u ? 1u : (E > 254u ? 254u : E);  // 1 / s, kept a normal number
  s = __builtin_bit_cast(float, fs << 23);
  return __builtin_bit_cast(float, fi << 23);
}

template <int M, int NC>
__global__ __launch_bounds__(256) void join_fwd_kernel(JoinSrc src, unsigned mask, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ n_out,
                                                       float* __restrict__ inv_norm, bf16_t* __restrict__ y,
                                                       float* __restrict__ mean, float* __restrict__ rstd, int B, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  const float invMD = 1.0f / (float)(M * D);
  for (int row = wave; row < B; row += nwaves) {
    f32x4 v[M][NC];
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const bool present = (mask >> k) & 1u;
#pragma unroll
      for (int c = 0; c < NC; ++c) {      // written out: a slot past the row, or of an absent modality, holds zeros
        const int ci = lane + 64 * c;
        v[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (present && ci < nchunk) v[k][c] = ROW_LD(f32x4, src.p[k] + (size_t)row * D + 4 * ci);
      }
    }
    float s1 = 0.f;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      float inv = 0.f;
      if ((mask >> k) & 1u) {      // wave-uniform
        float am = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) am = fmaxf(am, __builtin_fabsf(v[k][c][e]));
        float s;
        const float inv_s = join_ld_inv_s(wave_max(am), s);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = v[k][c][e] * s;
            q = fmaf(t, t, q);
          }
        const float r = sqrtf(wave_sum(q));
        const bool tiny = !(r * inv_s >= JOIN_NORM_EPS);
        const float a = tiny ? 1.0f : s, b = tiny ? JOIN_INV_EPS : 1.0f / r;
        inv = tiny ? JOIN_INV_EPS : b * s;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[k][c][e] = (v[k][c][e] * a) * b;
            s1 += v[k][c][e];            // slots past the row hold zeros
          }
      }
      if (lane == 0) inv_norm[(size_t)row * M + k] = inv;
      ROW_CHUNKS(c, ci) __builtin_nontemporal_store(v[k][c], reinterpret_cast<f32x4*>(n_out + ((size_t)k * B + row) * D + 4 * ci));
    }
    const float mu = wave_sum(s1) * invMD;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < M; ++k) ROW_CHUNKS(c, ci) ROW_SQDEV4(q, v[k][c], mu);
    const float var = wave_sum(q) * invMD;
    const float rs = rsqrtf(var + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    bf16_t* yr = y + (size_t)row * M * D;
#pragma unroll
    for (int k = 0; k < M; ++k) ROW_CHUNKS(c, ci) {
      const int col = k * D + 4 * ci;
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + col);
      LN_AFFINE_STORE(v[k][c], mu, rs, g, b, yr + col);
    }
  }
}

// dn = rstd * (g - mean(g) - xhat * mean(g * xhat)) [+ dn_extra],  g = dy * gamma, xhat = (n - mean) * rstd, the means over all M * D
// columns (an absent slot is a column of zeros: it has an xhat and takes part in both means, and gets no gradient written);
// df_k = inv_norm_k * (dn_k - n_k (n_k . dn_k))   or   dn_k * 1e12 for a row below the clamp (no projection term)
template <int M, int NC>
__global__ __launch_bounds__(256) void join_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dn_extra, JoinSrc src,
                                                       const float* __restrict__ inv_norm, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma, unsigned mask,
                                                       float* __restrict__ df, float* __restrict__ partial, bool want_w, int B, int D) {
  __shared__ RowRed red[2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wave = blockIdx.x * 4 + w;
  const int nwaves = gridDim.x * 4;
  const int nchunk = D >> 2;
  const float invMD = 1.0f / (float)(M * D);
  f32x4 ag[M][NC], ab[M][NC];
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      ag[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
      ab[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  for (int row = wave; row < B; row += nwaves) {
    const float mu = mean[row], rs = rstd[row];
    f32x4 n[M][NC], d[M][NC];
    float inv[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const bool present = (mask >> k) & 1u;
      inv[k] = present ? inv_norm[(size_t)row * M + k] : 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {      // written out: as in join_fwd_kernel
        const int ci = lane + 64 * c;
        n[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        d[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ci < nchunk) {
          if (present) n[k][c] = ROW_LD(f32x4, src.p[k] + (size_t)row * D + 4 * ci);
          d[k][c] = ROW_LD(f32x4, dy + (size_t)row * M * D + k * D + 4 * ci);
        }
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < M; ++k) ROW_CHUNKS(c, ci) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + k * D + 4 * ci);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        n[k][c][e] *= inv[k];
        const float xhat = (n[k][c][e] - mu) * rs;
        if (want_w) {
          ag[k][c][e] = fmaf(d[k][c][e], xhat, ag[k][c][e]);
          ab[k][c][e] += d[k][c][e];
        }
        const float gy = d[k][c][e] * g[e];
        d[k][c][e] = gy;
        s1 += gy;
        s2 = fmaf(gy, xhat, s2);
      }
    }
    const float m1 = wave_sum(s1) * invMD, m2 = wave_sum(s2) * invMD;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      if (!((mask >> k) & 1u)) continue;      // wave-uniform
      float dot = 0.f;
      ROW_CHUNKS(c, ci) {
        f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
        if (dn_extra != nullptr) x = ROW_LD(f32x4, dn_extra + ((size_t)k * B + row) * D + 4 * ci);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xhat = (n[k][c][e] - mu) * rs;
          const float dn = LN_DX(rs, d[k][c][e], m1, xhat, m2) + x[e];
          d[k][c][e] = dn;
          dot = fmaf(n[k][c][e], dn, dot);
        }
      }
      dot = wave_sum(dot);
      if (inv[k] >= JOIN_INV_EPS) dot = 0.f;      // below the clamp: d / 1e-12, no projection term
      ROW_CHUNKS(c, ci) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = inv[k] * (d[k][c][e] - n[k][c][e] * dot);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(df + ((size_t)k * B + row) * D + 4 * ci));
      }
    }
  }
  if (!want_w) return;      // uniform over the grid
  // block reduction of the per-lane column partials, one chunk slot at a time; each block writes its [2][M * D] partial sums
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) {      // written out: every slot takes part in the barriers of ROW_FOLD4
      const int ci = lane + 64 * c;
      ROW_FOLD4(2, ci, partial + ((size_t)blockIdx.x * 2 + w) * M * D + k * D + 4 * ci, ag[k][c][e], ab[k][c][e]);
    }
}

// out_k[c] += sum_b partial[b][k][c], k = 0 (dgamma), 1 (dbeta): one thread per column, blocks in ascending order
__global__ __launch_bounds__(256) void join_bwd_finish_kernel(const float* __restrict__ partial, int nblocks, int W,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int k = blockIdx.y;
  float* dst = k == 0 ? dgamma : dbeta;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (dst == nullptr || c >= W) return;
  float t = 0.f;
  for (int b = 0; b < nblocks; ++b) t += partial[((size_t)b * 2 + k) * W + c];
  dst[c] += t;
}

static inline int join_grid(int B) {
  int blocks = (B + 3) / 4;
  return blocks > 256 ? 256 : blocks;
}

// every row operand is read and written in 16-byte pieces (8-byte ones for the 16-bit row): the base pointers must allow it
static inline bool join_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static inline bool join_shape_ok(int B, int D, int M, int mask) {
  return B > 0 && D > 0 && D % 4 == 0 && (M == 2 || M == 3) && (long long)M * D <= 4096 && mask > 0 && mask < (1 << M);
}

}  // namespace octmae
using namespace octmae;

// NC: float4 chunks per lane and modality slice -- 1, 2, 4, 6, 8 (8 only with M = 2: M * D <= 4096)
#define JOIN_DISPATCH(KERNEL, MM, ...)                                                                      \
  switch (nc) {                                                                                             \
    case 1: hipLaunchKernelGGL((KERNEL<MM, 1>), grid, blk, 0, st, __VA_ARGS__); break;                      \
    case 2: hipLaunchKernelGGL((KERNEL<MM, 2>), grid, blk, 0, st, __VA_ARGS__); break;                      \
    case 3: case 4: hipLaunchKernelGGL((KERNEL<MM, 4>), grid, blk, 0, st, __VA_ARGS__); break;              \
    case 5: case 6: hipLaunchKernelGGL((KERNEL<MM, 6>), grid, blk, 0, st, __VA_ARGS__); break;              \
    default:                                                                                                \
      if (MM == 2) hipLaunchKernelGGL((KERNEL<2, 8>), grid, blk, 0, st, __VA_ARGS__);                       \
      else return -1;                                                                                       \
      break;                                                                                                \
  }

extern "C" int octmae_join_fwd(const float* f0, const float* f1, const float* f2, int present_mask, const float* gamma,
                               const float* beta, float* n_out, float* inv_norm, void* y_lp, float* mean, float* rstd, int B, int D,
                               int M, float eps, void* stream) {
  OCTMAE_CHECK_ARG(join_shape_ok(B, D, M, present_mask));
  OCTMAE_CHECK_ARG(gamma && beta && n_out && inv_norm && y_lp && mean && rstd);
  JoinSrc src = {{f0, f1, M == 3 ? f2 : nullptr}};
  for (int k = 0; k < M; ++k) OCTMAE_CHECK_ARG(!((present_mask >> k) & 1) || (src.p[k] != nullptr && join_aligned(src.p[k], 16)));
  OCTMAE_CHECK_ARG(join_aligned(gamma, 16) && join_aligned(beta, 16) && join_aligned(n_out, 16) && join_aligned(y_lp, 8));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nc = row_nc(D);
  bf16_t* y = reinterpret_cast<bf16_t*>(y_lp);
  const unsigned mask = (unsigned)present_mask;
  dim3 grid(join_grid(B)), blk(256);
  if (M == 2) {
    JOIN_DISPATCH(join_fwd_kernel, 2, src, mask, gamma, beta, n_out, inv_norm, y, mean, rstd, B, D, eps)
  } else {
    JOIN_DISPATCH(join_fwd_kernel, 3, src, mask, gamma, beta, n_out, inv_norm, y, mean, rstd, B, D, eps)
  }
  OCTMAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int octmae_join_ws_floats(int B, int D, int M) {
  if (!join_shape_ok(B, D, M, 1)) return -1;
  return join_grid(B) * 2 * M * D;
}

extern "C" int octmae_join_bwd(const float* dy, const float* dn_extra, const float* f0, const float* f1, const float* f2,
                               const float* inv_norm, const float* mean, const float* rstd, const float* gamma, int present_mask,
                               float* df_out, float* dgamma, float* dbeta, float* ws, int B, int D, int M, void* stream) {
  OCTMAE_CHECK_ARG(join_shape_ok(B, D, M, present_mask));
  OCTMAE_CHECK_ARG(dy && inv_norm && mean && rstd && gamma && df_out);
  const bool want_w = dgamma != nullptr || dbeta != nullptr;
  OCTMAE_CHECK_ARG(!want_w || ws != nullptr);
  JoinSrc src = {{f0, f1, M == 3 ? f2 : nullptr}};
  for (int k = 0; k < M; ++k) OCTMAE_CHECK_ARG(!((present_mask >> k) & 1) || (src.p[k] != nullptr && join_aligned(src.p[k], 16)));
  OCTMAE_CHECK_ARG(join_aligned(dy, 16) && join_aligned(dn_extra, 16) && join_aligned(gamma, 16) && join_aligned(df_out, 16) &&
                   join_aligned(ws, 16));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nc = row_nc(D);
  const unsigned mask = (unsigned)present_mask;
  const int blocks = join_grid(B);
  dim3 grid(blocks), blk(256);
  if (M == 2) {
    JOIN_DISPATCH(join_bwd_kernel, 2, dy, dn_extra, src, inv_norm, mean, rstd, gamma, mask, df_out, ws, want_w, B, D)
  } else {
    JOIN_DISPATCH(join_bwd_kernel, 3, dy, dn_extra, src, inv_norm, mean, rstd, gamma, mask, df_out, ws, want_w, B, D)
  }
  OCTMAE_LAUNCH_CHECK();
  if (want_w) {
    hipLaunchKernelGGL(join_bwd_finish_kernel, dim3((M * D + 255) / 256, 2), dim3(256), 0, st, ws, blocks, M * D, dgamma, dbeta);
    OCTMAE_LAUNCH_CHECK();
  }
  return 0;
}
