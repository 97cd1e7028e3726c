// The frame of the one-wave-per-SIMD attention backward kernels: what attn_bwd1w.hip (head_dim 32) and attn_bwd1w64.hip (head_dim 64)
// have in common, as text of the kernel function.  A kernel includes this file once per PART (#define BWD1W_FRAME_<PART> in front;
// undefined again here), in the order SETUP, [per key block:] KEY_BLOCK, <its dK^T / dV^T accumulators>, KT, <its pipeline
// prologue>, RING, <its tile loop>, HALF_DRAIN, <its dK / dV write-out>, [behind the key blocks:] TAIL.  The parts declare the
// locals under the names the generated bodies use (tools/gen_attn_bwd1w.py).  Text, not templates: the device code of both kernels
// is held to what it was before they shared it (make digest), and that follows the order of the declarations (the accumulators'
// place between two parts is one such order).  The including file's namespace is the configuration:
//   HD, NW, KW, NG, KB     head dim, waves, keys per wave, 32-key groups per wave, keys per block
//   NP                     1-KiB pieces of Q (waves 0, 1) or dO (waves 2, 3) a wave requests per tile
//   NQT                    16-query tiles of a sub-step's dQ^T a wave owns; NOLDREQ = NST = 2 NQT workspace-value requests / write-out
//                          stores per tile
//   LA, NB, NOLD, T, QR, OR_, CR, IMG, IMG_BUF, OLD, OLD_QUAD, OLD_TILE, LDS, STG     the LDS layout
//   kst_off(row, c)        byte offset of 8-byte chunk c of staged K row `row`
//   dq_dtile(wid), dq_qtile(wid)     the 16-head-dim tile / the first 16-query tile of dQ^T[HD][32 queries] wave `wid` owns
//   old_quad(buf, u, wid)  byte offset in OLD of quad u of buffer buf of wave wid: ((buf NOLDREQ + u) NW + wid) 1024 in both files,
//                          each in the association its device code was recorded with
//   BWD1W_BODY, BWD1W_DRAIN          file names of its generated body and drain
//   BWD1W_SLOT_OFFSETS               see BWD1W_TILE_SETUP
// The macros BWD1W_TILE_SETUP, BWD1W_DRAIN_ADDRS, BWD1W_WAIT and the stamp plumbing are in attn_bwd1w.hpp.

#if defined(BWD1W_FRAME_SETUP)
#undef BWD1W_FRAME_SETUP
  extern __shared__ __attribute__((aligned(128))) char smem[];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  static_assert(KB * HD * 2 <= 2 * IMG_BUF, "K staging must fit the two images");
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static_assert((CR % 128) == 0 && (IMG % 128) == 0 && (OLD % 128) == 0, "XOR chunk selectors act on address bits 0..6");
  static_assert((OR_ - QR) % 128 == 0 && T::BYTES % 128 == 0, "slot / region offsets leave the low 7 address bits alone");
  static_assert(NOLDREQ == 2 * NQT && NST == 2 * NQT && OLD_TILE == NOLDREQ * OLD_QUAD && OLD_QUAD == NW * 1024, "one old-value quad and one store per owned dQ^T tile");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int bh = xcd_remap((int)blockIdx.x, (int)gridDim.x);      // an XCD gets whole samples: their Q / dO rows share lines
  const int b = bh / H, head = bh % H;
  const size_t rs = (size_t)3 * H * HD, os = (size_t)H * HD;
  const bf16_t* qb = qkv + (size_t)b * N * rs + (size_t)head * HD;
  const bf16_t* kb_ = qb + (size_t)H * HD;
  const bf16_t* vb_ = qb + (size_t)2 * H * HD;
  const bf16_t* dob = dout + (size_t)b * N * os + (size_t)head * HD;
  const float sc2 = scale * LOG2E;
  const bool half_drain = ((N - 1) & 63) < 32;    // the last tile's rows 32 .. 63 are all >= N
  const int ntiles = (N + 63) / 64;               // NPAD = 64 (ntiles + 1): one all-padding tile of row constants behind the last

  // ---- LDS-DMA plan: a tile is 2 NP Q pieces + 2 NP dO pieces of 1 KiB; waves 0, 1 bring Q, waves 2, 3 dO (NP pieces each) and
  // every wave one row of constants (-lse*log2e: even waves, -delta: odd)
  const bool isq = wid < 2;                                       // wave-uniform
  const i32x4_t rsD = isq ? make_rsrc(qb, (unsigned)(((size_t)(N - 1) * rs + HD) * 2)) : make_rsrc(dob, (unsigned)(((size_t)(N - 1) * os + HD) * 2));
  unsigned dvoff[NP], dlds[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int piece = (wid & 1) * NP + i;
    const int q = piece * 64 + lane;
    const int row = q / T::CHUNKS, c = (q % T::CHUNKS) ^ T::sw(row);
    dvoff[i] = (unsigned)(((size_t)row * (isq ? rs : os) + c * 8) * 2);
    dlds[i] = (unsigned)((isq ? QR : OR_) + piece * 1024);
  }
  const unsigned dstride = (unsigned)(64 * (isq ? rs : os) * 2);
  const i32x4_t rsC = make_rsrc(rowc + (size_t)(wid & 1) * gridDim.x * NPAD + (size_t)bh * NPAD, (unsigned)((size_t)NPAD * 4));
  // Q / dO of tile `dt` and the constants of tile `ct` -> ring slot   (NP + 1 operations)
  auto issue = [&](int dt, int ct, int slot) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + dlds[i] + (unsigned)(slot * T::BYTES)));
      lds_dma16(m0v, dvoff[i] + (unsigned)dt * dstride, rsD);
    }
    const unsigned m0c = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + CR + slot * 512 + (wid & 1) * 256));
    lds_dma4(m0c, (unsigned)((ct * 64 + lane) * 4), rsC);
  };

  // ---- dQ workspace of this (batch, head): fp32 [N][HD]; rows >= N fall outside the descriptor (loads 0, stores dropped).
  // Of every sub-step's dQ^T[HD head dims][32 queries] a wave owns NQT 16 x 16 tiles: head dims 16 dq_dtile + 4 (lane >> 4) .. + 3
  // of query 16 (dq_qtile + u) + (lane & 15) of the sub-tile, u < NQT (the C / D layout of the 16x16x32 MFMA).
  float* wsb = dq_ws + (size_t)bh * N * HD;
  const i32x4_t rsW = make_rsrc(wsb, (unsigned)((size_t)N * HD * 4));
  const __amdgpu_buffer_rsrc_t rsWs = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void*>(((unsigned long long)(unsigned)rsW[1] << 32) | (unsigned)rsW[0]), 0, rsW[2], 0x00020000);
  [[maybe_unused]] const int dt = dq_dtile(wid), qt = dq_qtile(wid), g16 = lane >> 4, c16 = lane & 15;
#ifdef BWD1W_WSOFF                       // (an experiment of the kernel's file with another workspace layout)
  const unsigned wsoff = BWD1W_WSOFF;
#else
  const unsigned wsoff = (unsigned)(((16 * qt + c16) * HD + 16 * dt + 4 * g16) * 4);
#endif
  constexpr unsigned WS_QT = 16 * HD * 4, WS_SUB = 32 * HD * 4, WS_TILE = 64 * HD * 4, DROP = 0x80000000u;   // DROP: an offset outside every descriptor
  // workspace values of this wave's quads of `tile` -> OLD buffer   (NOLDREQ operations; `base` = DROP in the first key block: zeros)
  auto oldreq = [&](int tile, int buf, unsigned base) {
#pragma unroll
    for (int u = 0; u < NOLDREQ; ++u) {
      const unsigned m0o = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + OLD + old_quad(buf, u, wid)));
      lds_dma16_ws(m0o, wsoff + base + (unsigned)tile * WS_TILE + (unsigned)(u / NQT) * WS_SUB + (unsigned)(u % NQT) * WS_QT, rsW);
    }
  };

  // ---- per-lane LDS address parts, fixed for the whole kernel (opaque: not re-derived from the lane id inside the loops)
  const int tq_ = (lane >> 2) & 3, tp_ = lane & 3, tgi = (lane >> 4) & 1;
  const unsigned a_const = opaque(lds0 + (unsigned)(CR + 16 * h));
  const unsigned a_row = opaque(lds0 + (unsigned)(QR + T::off(r, h)));
  const unsigned a_trlo = opaque(lds0 + (unsigned)(QR + T::off(4 * h + tq_, 2 * tgi + (tp_ >> 1)) + (tp_ & 1) * 8));
  const unsigned a_trhi = opaque(lds0 + (unsigned)(QR + T::off(4 * h + tq_ + 8, 2 * tgi + (tp_ >> 1)) + (tp_ & 1) * 8));
  // dS image: this lane's key row KW wid + r (+ 32 g), chunk h (^ 32 half + 16 k for the query chunk 4 half + 2 k + h) (+ image buffer)
  const unsigned a_imgw = opaque(lds0 + (unsigned)(IMG + img_off(wid * KW + r, h)));
  // transposed reads of 4-key x 16-query blocks for the 16x16x32 B operand dS^T[k = key 32 ks + 8 g16 + e][col q = 16 qt + c16]:
  // keys 8 g16 + tq_ (+ 4) (+ 32 ks), query chunk 4 qt + tp_ (^ 32: the second query tile) (+ image buffer)
  const unsigned a_imglo = opaque(lds0 + (unsigned)(IMG + img_off(8 * g16 + tq_, 4 * qt + tp_)));
  const unsigned a_imghi = opaque(lds0 + (unsigned)(IMG + img_off(8 * g16 + tq_ + 4, 4 * qt + tp_)));
  const unsigned a_old = opaque(lds0 + (unsigned)(OLD + wid * 1024 + lane * 16));
  f32x16 zero16;
#pragma unroll
  for (int e = 0; e < 16; ++e) zero16[e] = 0.f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

#elif defined(BWD1W_FRAME_KEY_BLOCK)
#undef BWD1W_FRAME_KEY_BLOCK
    const int key0 = kb * KB;
    const unsigned oldbase = kb > 0 ? 0u : DROP;
    // ---- ring prologue: tiles 0 .. 2, workspace values of tile 0 -- requested first, their latency runs beside the K staging.
    // (The ring, the constants and the workspace-value buffers are not the image region; LDS-DMA writes of one wave land in
    // issue order, so the surplus tiles the previous block's loop left in flight need no drain.)
    issue(0, 0, 0);
    issue(1, 1, 1);
    issue(2, 2, 2);
    oldreq(0, 0, oldbase);
    // ---- stage this block's K rows for the transposed reads of the loop-invariant K^T fragments
    {
#pragma unroll
      for (int i = 0; i < KB * T::CHUNKS / 256; ++i) {
        const int c = tid + 256 * i;
        const int row = c / T::CHUNKS, cc = c % T::CHUNKS;
        const u32x4 v = *reinterpret_cast<const u32x4*>(kb_ + (size_t)(key0 + row) * rs + 8 * cc);
        *reinterpret_cast<u32x2*>(smem + STG + kst_off(row, 2 * cc)) = u32x2{v[0], v[1]};
        *reinterpret_cast<u32x2*>(smem + STG + kst_off(row, 2 * cc + 1)) = u32x2{v[2], v[3]};
      }
    }
    // ---- this wave's keys: B operands of S (pre-scaled) and dP
    bf16x8 kS[NG][HD / 16], vS[NG][HD / 16];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const size_t krow = (size_t)(key0 + wid * KW + 32 * g + r) * rs;
#pragma unroll
      for (int s = 0; s < HD / 16; ++s) {
        const u32x4 kv = *reinterpret_cast<const u32x4*>(kb_ + krow + 16 * s + 8 * h);
        const u32x4 vv = *reinterpret_cast<const u32x4*>(vb_ + krow + 16 * s + 8 * h);
        kS[g][s] = scale_frag(kv, sc2);
        vS[g][s] = __builtin_bit_cast(bf16x8, vv);
      }
    }

#elif defined(BWD1W_FRAME_KT)
#undef BWD1W_FRAME_KT
    __syncthreads();                              // K staging visible
    // A operand of dQ^T = K^T dS^T (16x16x32): K^T[row d = 16 dt + c16][k = key 32 ks + 8 g16 + e], all KB keys, loop invariant
    bf16x8 kT[KB / 32];
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks)
      kT[ks] = cat4(lds_tr_read(smem + STG + kst_off(8 * g16 + tq_, 4 * dt + tp_) + ks * 32 * T::ROWB),
                    lds_tr_read(smem + STG + kst_off(8 * g16 + tq_ + 4, 4 * dt + tp_) + ks * 32 * T::ROWB));
    __builtin_amdgcn_s_waitcnt(0xC07F);           // lgkmcnt(0)
    __syncthreads();                              // every wave has its K^T fragments: the image region is free

    // (every load the compiler tracks has returned: without this it carries "loads pending" into the tile loop and waits there
    // with a vmcnt that also drains the hand-counted LDS-DMA ring; the ring prologue, requested before the K staging, is
    // complete with them)
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();

#elif defined(BWD1W_FRAME_RING)
#undef BWD1W_FRAME_RING
    // Vector-memory operations of this wave in issue order (vmcnt retires in order): prologue 3 (NP + 1) + NOLDREQ; iteration t:
    // [NST / 2 stores of the write-out, sub-step 0] [tile t+3: NP + 1] [workspace values of tile t+1: NOLDREQ] [NST / 2 stores,
    // sub-step 1] = VM_ITER.  Iteration t (tile t; t = ntiles is the all-padding tile that drains the pipeline: P = 0 there)
    // needs, before its mid-tile barrier, tile t+1 complete, and in its write-outs the workspace values of tile t-1: both were
    // requested in iteration t-2 or earlier, so "all but the last iteration's VM_ITER" covers them (BWD1W_WAIT).  The generated body
    // asserts the stores and requests it places against NST and the one issue_tile() counted here.
    constexpr int VM_ITER = NST + (NP + 1) + NOLDREQ;
    BWD1W_STAMP_BEGIN
    // The pipeline drains behind the last real sub-step X of the block -- (ntiles - 1, 0) when rows 32 .. 63 of the last tile are
    // all >= N (N = 64 m + 1 .. 64 m + 32: the cls token makes the model's lengths 64 m + 1), else (ntiles - 1, 1): one more
    // sub-step's worth of dV^T / dK^T (X's last group, second half) and the dQ^T product of X, and two write-outs.  Those run as
    // straight-line code behind the loop, reduced to exactly that (SLIM / TINY, generated from the same bundle table), instead of
    // as padding sub-steps in full: ~1.7 sub-steps less per key block (of 43 at N = 1281, of 163 at N = 5121).
    // (the drain code works from opaque copies of the per-lane address constants: derived addresses are then computed there,
    // not hoisted above the tile loop and kept in registers across it)
    const unsigned o_imglo = a_imglo, o_imghi = a_imghi, o_old = a_old, o_wsoff = wsoff;

#elif defined(BWD1W_FRAME_HALF_DRAIN)
#undef BWD1W_FRAME_HALF_DRAIN
    if (half_drain) {
      {
        const int t = ntiles - 1;
        BWD1W_WAIT(t);
        BWD1W_TILE_SETUP
#define BWD1W_ONLY_SUBSTEP0
#include BWD1W_BODY
#undef BWD1W_ONLY_SUBSTEP0
      {
        BWD1W_DRAIN_ADDRS
#define BWD1W_DRAIN_SLIM1
#include BWD1W_DRAIN
#undef BWD1W_DRAIN_SLIM1
      }
      }
      {
        const int t = ntiles;
        BWD1W_WAIT(t);
        BWD1W_TILE_SETUP
        BWD1W_DRAIN_ADDRS
#define BWD1W_DRAIN_TINY0
#include BWD1W_DRAIN
#undef BWD1W_DRAIN_TINY0
      }
    }

#elif defined(BWD1W_FRAME_TAIL)
#undef BWD1W_FRAME_TAIL
  wait_vm<0>();
  // ---- the key past the last full block (N = nkb * KB + 1: the cls token) and the workspace -> bf16 conversion, for this
  // (batch, head), by the workgroup that has just written the workspace rows and streamed Q / dO (attn_bwd_tail1.hpp)
  if (tail_key >= 0) {
    __syncthreads();
    // (the thread id re-derived from the lane count: nothing of the tail's per-lane state lives in registers across the tile loop)
    const int lane_t = lane_id_fresh();
    attn_bwd_tail1_body<HD, BWD1W_TAIL_DEPTH>(qkv, dout, rowc, dq_ws, dqkv, N, NPAD, H, tail_key, 1, scale, bh, (int)gridDim.x, reinterpret_cast<float*>(smem),
                               wid * 64 + lane_t);
  }

#else
#error "attn_bwd1w_frame.hpp: no part selected"
#endif
