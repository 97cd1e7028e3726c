/* liboctmae -- C ABI of the MI355X-native 3-D MAE hot path (gfx950 only).
 *
 * The reference (ZucksLiu/OCTCubeM) has no FFI layer: every GPU operation it performs arrives through
 * PyTorch/ATen, cuDNN/cuBLAS and flash-attn from Python modules.  These entry points are what a binding
 * for that path binds instead; each one names the reference call site it replaces (paths relative to
 * /root/reference).  The Python host side (octcubem_amd/_lib.py, ctypes) is the only caller.
 *
 * Conventions
 *   - plain pointers and sizes, no torch types; all pointers are DEVICE pointers unless noted
 *   - the caller owns every buffer (incl. workspaces); nothing is allocated or retained by the library
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*); no host synchronisation
 *   - return value: 0 ok, <0 argument error (-1 bad argument, -2 unsupported combination), >0 hipError_t
 *   - "bf16" buffers are raw 16-bit bfloat16 values; row-major; leading dimensions in ELEMENTS
 *   - re-entrant, no thread-local state: forward runs on the main thread, backward on autograd's thread
 */
#ifndef OCTMAE_H_
#define OCTMAE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ONE place the ABI number lives: octmae_abi_version() returns it (csrc/probe.hip), octcubem_amd/_lib.py parses it
 * from this header and refuses a library that reports another number, __graft_entry__.build() and the tests compare the two.
 * 4: octmae_attn_bwd_dq_rowconst.  5: octmae_comm_* (RCCL), octmae_attn_bwd_fused + workspace query.  7: octmae_set_option, octmae_scatter_add_rows, octmae_dec_assemble_bwd.
 * 8: octmae_linear_dgrad_delta, octmae_attn_bwd_fused_delta.  9: octmae_wgrad_accum_pair, octmae_wgrad_split_plan.
 * 10: octmae_lp_dtype, octmae_comm_stream, octmae_mt_adamw_fused, octmae_gemm_bf16_ws + workspace arguments.
 * 11: the small-launch GEMM kernel and its split-K workspace (octmae_gemm_split_ws_kib, octmae_gemm_small_plan, "gemm_small");
 *     the stream-K and 16x16x32 variants of round 4 / 5 left the library (octmae_gemm_streamk_*, "gemm_mfma16", "gemm_streamk").
 * 12: octmae_slice_pool_fwd / _bwd / _ws_floats (the slice-pooling head of the RETFound-all model).
 * 13: octmae_gemm_plan, octmae_wgrad_pair_plan (the GEMM launch planner of csrc/gemm_plan.hpp, queried without a GPU); variant bits 9 / 10
 *     now force the 256-tile main loop they name for forward and dgrad launches too, and never the small-launch kernel.
 * 14: splitk = 0 of a weight gradient (octmae_gemm_bf16[_ws] epilogue 5, octmae_wgrad_accum_pair and the two plan queries) means
 *     "chosen by the planner" (csrc/gemm_plan.hpp: auto_wgrad_split); until now 0 ran as 1.  No new entry points.
 * 15: octmae_volume_box, octmae_volume_resample (the volume transforms in front of the models, csrc/transform3d.hip).
 * 16: octmae_mae_compose (the reconstruction volumes of the validation pass, csrc/recon.hip).
 * 17: octmae_image_resample, octmae_image_resample_plan (the 2-D image transforms in front of the 2-D towers, csrc/image2d.hip).
 * 18: octmae_rank_counts (the rank counts behind AUROC / average precision of the fine-tune evaluation, csrc/metrics.hip).
 * 19: octmae_retrieval_ranks (the retrieval ranks of the COEM validation off f32 MFMA tiles, csrc/retrieval.hip; the tile itself is
 *     csrc/simtile.hpp, shared with 24 and 29 since 31 without a change to any entry point or to the device code).
 * 20: octmae_mix_batch (mixup / cutmix of a fine-tune batch in place, csrc/mixup.hip).
 * 21: octmae_rank_counts_masked (rank counts over a per-column population: the multi-task evaluation, csrc/metrics.hip).
 * 22: octmae_image_stats, octmae_image_augment, octmae_aug_desc (RandAugment's image operations on the device, csrc/augment2d.hip).
 * 23: octmae_patch_scatter, octmae_cam_weights (+ octmae_cam_ws_floats), octmae_cam_tokens, octmae_heatmap (input gradients, Grad-CAM
 *     and heat volumes, csrc/saliency.hip).
 * 24: octmae_clip_loss_fwd, octmae_clip_loss_bwd (+ octmae_clip_loss_ws_floats): the contrastive loss of the COEM training step and its
 *     gradients off the f32 MFMA tiles of 19, csrc/cliploss.hip.
 * 25: octmae_join_fwd, octmae_join_bwd (+ octmae_join_ws_floats): normalise, concatenate and LayerNorm the tower outputs in front of
 *     the COEM classification head, csrc/join.hip.
 * 26: octmae_ln_apply (csrc/layernorm.hip), octmae_gelu_apply (csrc/recompute.hip): the LayerNorm and GELU outputs rebuilt in the
 *     backward of a Block that did not keep them (activation recomputation, ops.BlockFn); octmae_colsum_accum_ws (+ octmae_colsum_ws_rows):
 *     the bias-gradient column sums with a fixed order of additions.
 * 27: octmae_dwconv7_fwd / _bwd_input / _bwd_weight (+ _ws_floats), octmae_layer_scale_fwd / _bwd (+ _ws_floats): the depthwise 7x7
 *     convolution and the layer scale of a ConvNeXt layer (the SLIViT baseline's feature extractor, csrc/convnext.hip).
 * 28: octmae_slab_norm_fwd, octmae_slab_norm_bwd (+ octmae_slabnorm_ws_floats): the LayerNorm over a transposed token slab in front of
 *     the SLIViT head's patch projection (the OCTCube trunk with the SLIViT slice head, csrc/slabnorm.hip).
 * 29: octmae_retrieval_topk (+ octmae_retrieval_topk_ws): the k best candidates per query off the tiles of octmae_retrieval_ranks, with a
 *     strict tie order (top-k cross-modal retrieval of the COEM evaluation, csrc/retrieval_topk.hip).
 * 30: octmae_mae_compose_nc, octmae_white_border (+ octmae_white_border_ws_floats): the RGB / raw-level panels and the border blanking of
 *     the 2-D half of the validation pass (csrc/recon2d.hip).
 * 31: octmae_cam_eigen (+ octmae_cam_eigen_ws_floats), octmae_cam_accumulate: the eigen-smoothed Grad-CAM map by matrix-free power
 *     iterations and the normalise-flip-fold of test-time-augmentation smoothing (csrc/saliency.hip).
 * 32: octmae_retrieval_pair_ranks (+ octmae_retrieval_pair_ws): both directions of up to three square retrieval problems from one walk
 *     over the tiles of 19 (the six directions of the three-modality COEM validation, csrc/retrieval_pair.hip).
 * 33: octmae_bootstrap_rank_metrics (bootstrap resamples of AUROC / average precision / AUPRC / best F1 from one sort and a weighted
 *     prefix walk per resample, csrc/bootstrap.hip).
 * 34: octmae_unit_moments, octmae_bootstrap_moments (+ octmae_bootstrap_moments_ws): bootstrap resamples of the regression metrics as
 *     one int32 x f64 matrix product on v_mfma_f64_16x16x4_f64, in a fixed summation order (csrc/bootmoments.hip).
 * 35: deterministic mode ("deterministic" of octmae_set_option, octmae_deterministic): k-split weight gradients through slabs and
 *     octmae_wgrad_fold's kernel instead of fp32 atomics (octmae_wgrad_accum_pair_ws, octmae_wgrad_det_ws_bytes, octmae_gemm_plan_ws,
 *     octmae_wgrad_pair_plan_ws), the gradient norm through per-chunk partials (octmae_mt_sumsq_ws, octmae_mt_adamw_fused_ws).
 *     Added under 35 (new entry points only; no caller of an earlier 35 breaks): octmae_rollout_step (+ octmae_rollout_ws), one step of
 *     attention rollout as a weighted column sum of a recomputed softmax off the tiles of 19 (csrc/rollout.hip).
 *     Added under 35 in the same way: octmae_cover_accumulate, octmae_cover_finish, the per-token sums of the masked predictions over
 *     complementary masks and their finishing pass into a reconstruction volume, a squared-error volume and token scores
 *     (csrc/cover.hip).
 *     Added under 35 in the same way: octmae_lora_merge, octmae_lora_wgrad (+ octmae_lora_plan, octmae_lora_ws_bytes), the merged
 *     operand of a Linear with a low-rank adapter and the adapter gradients without a weight gradient (csrc/lora.hip).
 *     The number stays 35 because tests/test_cpu_deterministic.py pins it; the next change to an existing entry point takes 36. */
#define OCTMAE_ABI_VERSION 35
int octmae_abi_version(void);

/* The 16-bit operand type this library was built for: 0 = bfloat16 (liboctmae.so, the shipped build; BASELINE's headline type),
 * 1 = IEEE half (`make -C octcubem_amd/csrc F16=1` -> liboctmae_f16.so: the same kernels with the type, the conversions and the
 * MFMA opcodes switched in csrc/common.hpp).  The reference's own default arithmetic is fp16 autocast + GradScaler
 * (Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:259-263, custom_util/misc.py:311-312); the half build is how the
 * north star's 1e-3 on pred / gradients is shown directly (tests/test_gpu_f16_parity.py).  Every "bf16" buffer of this header is
 * a buffer of THIS type; the host side allocates with the matching torch dtype (octcubem_amd/ops.py: BF16). */
int octmae_lp_dtype(void);

/* Kernel-selection switches for same-process A/B measurements and for tests that cover both forms of a kernel (no reference
 * counterpart: the reference's kernels come from its libraries).  Returns the previous value, -1 for an unknown key.
 *   "attn_bwd_hd32_form"   1 (default): one wave per SIMD, 4 x 128 keys per workgroup (csrc/attn_bwd1w.hip)
 *                          0: two waves per SIMD, 8 x 64 keys (csrc/attn_bwd.hip) -- the round-2 kernel
 *   "attn_bwd_hd64_form"   1 (default): one wave per SIMD, 4 x 64 keys per workgroup (csrc/attn_bwd1w64.hip)
 *                          0: two waves per SIMD, 8 x 32 keys (csrc/attn_bwd.hip); the two forms agree bit for bit
 *   "attn_bwd_tail_fused"  1 (default): the one-wave kernels also take the single key past the last full key block and the
 *                          workspace -> bf16 conversion of their (batch, head); 0: the separate launch (same results)
 *   "gemm_small"           1 (default): forward / dgrad launches whose 256 x 256 tiles would leave most CUs idle take the
 *                          small-launch kernel (gemm128d_kernel: 128 x 128 tiles, deterministic split-K) where the cost model of
 *                          csrc/gemm_plan.hpp (plan128) prices it faster; 0: never (the choice before round 6).  Bits 12 / 13 (0x1000 /
 *                          0x2000) of octmae_gemm_bf16's `epilogue` argument force that kernel with a 4- / 2-stage ring for one
 *                          call (its k split is then `splitk`, 1 .. 4), bit 14 (0x4000) forbids it (bits 8-10: the other variants)
 *   "gemm_small_launches", "gemm_small_split_launches", "gemm_small_wgrad_launches"   read-only: how many GEMM launches of this process
 *                          took that kernel / took it with a k split / how many weight-gradient pairs took its 128-tile form (tests)
 *   "wgrad_s1_atomic"      the epilogue of an UNSPLIT weight-gradient launch: 2 (default) read-modify-write in batches of 16 registers
 *                          through a buffer descriptor, 1 the fp32 atomics of a split launch, 0 one guarded load + store per register
 *   "wgrad_stagger"        v >= 0 (default 29): split-K weight gradients of >= 8 slices with <= 96 k-tiles each run with slice
 *                          lengths rising by v / 256 k-tiles per output tile of the launch from one slice to the next, so that the
 *                          slices' fp32-atomic epilogues follow one another instead of colliding; 0: equal slices
 *   "deterministic"        0 (default) / 1: DETERMINISTIC MODE -- no float of a training step is added in the order workgroups happen
 *                          to finish.  The environment variable OCTMAE_DETERMINISTIC, read once per process, wins.  Under it
 *                          (csrc/gemm_plan.hpp): a weight gradient (epilogue 5, octmae_wgrad_accum_pair[_ws]) with S > 1 k slices stores
 *                          slice z as slab z of the lent workspace (fp32 [S][NA][NB], plain stores, need not be initialised: the
 *                          split_ws of octmae_gemm_bf16_ws, whose counters are not touched) and one more launch folds
 *                          gW = (...((gW + P_0) + P_1) ... + P_{S-1}) -- what S unsplit launches over the slices' rows, in order, leave;
 *                          S is the split of the default mode capped to the slabs that fit (1 without a workspace: never atomics),
 *                          the slices are equal (no stagger); the bias gradient of a weight gradient is octmae_colsum_accum over dY
 *                          before the GEMM, that of epilogue 4 the per-slab workspace or octmae_colsum_accum over the output;
 *                          octmae_mt_sumsq_ws / octmae_mt_adamw_fused_ws leave one partial per chunk and add them in chunk order. */
int octmae_set_option(const char* key, int value);
int octmae_deterministic(void);         /* the mode as the library sees it (the environment variable included): 0 / 1 */

/* ---- GEMM with fused epilogues ------------------------------------------------------------------
 * X[a][b] = sum_k A[a][k] * B[b][k],  A has NA rows, B has NB rows, reduction length K.
 * a_kstrided / b_kstrided = 0: operand stored [rows][K] (nn.Linear layout); 1: stored [K][rows].
 * epilogue (output is C[b][a], i.e. NB rows x NA contiguous columns, unless noted):
 *   0  C bf16 = X + bias[a]                       nn.Linear forward        video_vit.py:114-135, timm Mlp fc1/fc2
 *   1  C f32  = X + bias[a]                       decoder_pred             models_mae_joint_res_flash_attn.py:595
 *   2  C bf16 = X + bias, C2 bf16 = gelu(C)       Mlp fc1 + nn.GELU        video_vit.py:174-179 (timm Mlp)
 *   3  C f32  = aux_f32[b][a] + X + bias[a]       proj / fc2 + residual    video_vit.py:182-183
 *   4  C bf16 = X * gelu'(aux_bf16[b][a])         backward of 2 (dgrad of fc2 fused with GELU'); a non-NULL C2 is an fp32 [NA]
 *                                                 vector that receives += the column sums of C (fc1's bias gradient)
 *   5  C f32[a][b] += X  (NA rows x NB columns; split-K over `splitk` workgroup slices, fp32 atomics
 *                         when there is more than one; splitk = 0: chosen by the planner, csrc/gemm_plan.hpp:
 *                         auto_wgrad_split)       weight gradients (autograd of nn.Linear)
 *                         a non-NULL C2 is an fp32 [NA] vector that receives += sum_k A[a][k]: with A = dY this is the
 *                         bias gradient of the same Linear, taken from the operand tiles the kernel stages anyway
 * bias may be NULL.  Requirements: lda, ldb multiples of 8; NA multiple of 4 (epilogues 0-4); epilogue 5: NA * ldc * 4 < 2^32 bytes.
 * Operands of up to 0xFFF00000 bytes run on the LDS-DMA kernels (32-bit buffer offsets), larger ones on the register-staged kernel
 * with 64-bit pointers; outputs and aux of any size (docs/OFFSET_RANGES.md). */
int octmae_gemm_bf16(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux,
                     int NA, int NB, int K, int lda, int ldb, int ldc, int ldaux, int a_kstrided, int b_kstrided,
                     int epilogue, int splitk, void* stream);

/* octmae_gemm_bf16 (splitk = 0 included) with a split-K workspace lent for this one call (also the trailing `split_ws, split_ws_bytes` of the three
 * fused entry points below; NULL / 0 = no k split).  The reference's cuBLAS / hipBLASLt picks split-K / stream-K kernels by itself
 * for such shapes (nn.Linear forward and backward: video_vit.py:114-135, timm Mlp); its shipped recipe runs ONE volume per GPU
 * (scripts/run_chunks_pretraining_vitl_oph_joint_flash_attn.sh:25-30), where a [1281 x 4096] x [4096 x 1024] Linear is 24 tiles of
 * 256 x 256 for 256 CUs.  Forward / dgrad launches that the cost model prices faster that way run on 128 x 128 tiles
 * (gemm128d_kernel), long reductions on few tiles additionally split 2-4 ways over k: every slice leaves its fp32 partial tile in
 * `split_ws`, the slice that ARRIVES last (an arrival counter per tile) adds the partials in slice order and runs the SAME fused
 * epilogue -- deterministic, no workgroup ever waits for another.  split_ws: octmae_gemm_split_ws_kib() KiB of device memory
 * whose counters (the last 16 KiB) were ZERO when it was first lent; every launch leaves them zero; contents need not be preserved
 * between calls, but two launches that may run CONCURRENTLY (different streams) must not share one workspace. */
int octmae_gemm_split_ws_kib(void);     /* size of that workspace in KiB */
/* host-side arithmetic only (tests of the planner): 1 if a forward / dgrad launch of NA x NB x K on `cus` CUs takes the small-launch
 * kernel under the current "gemm_small" option (*slices = its k split, *stages = its ring depth, 4 or 2), 0 otherwise.
 * have_ws: a split workspace is lent; big_ok: the problem qualifies for the 256-tile kernels */
int octmae_gemm_small_plan(int NA, int NB, int K, int cus, int have_ws, int big_ok, int* slices, int* stages);
/* The whole launch plan of one GEMM call (csrc/gemm_plan.hpp: plan_gemm), host-side arithmetic only: what octmae_gemm_bf16[_ws] and the
 * fused entry points below would launch for X[a][b] = sum_k A[a][k] B[b][k] (NA, NB, K, lda, ldb as there) on `cus` CUs under the
 * current options.  kind: 0 forward (epilogues 0-3 plan alike), 1 dgrad, 2 dgrad x GELU' with the column sums by atomics (epilogue 4
 * with C2), 3 the same through the per-slab workspace (octmae_linear_dgrad_dgelu), 4 dgrad + delta (octmae_linear_dgrad_delta),
 * 5 wgrad, 6 wgrad with the bias gradient (epilogue 5 with C2).  variant: the kernel-selection bits
 *   bit 8 (0x100) the 128-tile register-staged kernel; bit 9 (0x200) / bit 10 (0x400) the two-stage / phased 256-tile main loop wherever
 *   the problem takes 256-tiles (the register-staged kernel elsewhere, never the small-launch kernel); bit 12 / 13 (0x1000 / 0x2000)
 *   the small-launch kernel with a 4- / 2-stage ring wherever its operands allow (it wins over bits 9 / 10; bits 8 and 14 win over
 *   it), split `splitk` ways or, where bits 16-18 are set,
 *   that many (1 .. 4; fewer without a workspace or when a slice would be empty); bit 14 (0x4000) never the small-launch kernel;
 *   bit 15 (0x8000) epilogues 2 / 4 store / read gelu'(pre).
 * Returns 0 and writes 13 ints to out, or -2 where the entry point would (combination not built / the caller falls back):
 *   out[0] kernel family: 0 gemm_kernel (128-tile register-staged), 1 gemm256_kernel (two-stage), 2 gemm256p_kernel (phased),
 *          3 gemm128d_kernel (small launch);  [1] workgroups;  [2] tiles_a  [3] tiles_b  [4] cgroup  [5] k slices  [6] k-tiles per slice
 *   [7] kstagger  [8] atomic1  [9] ring depth (small launch, else 0)  [10] the small launch's k split (else 1)
 *   [11] rows of the column-sum workspace that are folded (route 2)  [12] column-sum route: 0 none, 1 atomics inside the kernel,
 *   2 per-slab rows + a folding launch, 3 / 4 a separate octmae_colsum_accum launch before / after the GEMM.
 * splitk as in octmae_gemm_bf16 (kinds 5 / 6: 0 = chosen by the planner, so that the answer is what a weight gradient launches). */
int octmae_gemm_plan(int kind, int NA, int NB, int K, int lda, int ldb, int variant, int splitk, int have_ws, int cus, int* out);
/* The same with the SIZE of the lent workspace (have_ws = ws_bytes >= octmae_gemm_split_ws_kib() KiB): in deterministic mode the k split of
 * kinds 5 / 6 is capped to the slabs that fit into ws_bytes (at most the workspace's 64 MiB in front of its counters), and
 * out[8] == 3 says that the launch stores slabs and is followed by the fold (out[7] == 0 and out[12] != 1 there). */
int octmae_gemm_plan_ws(int kind, int NA, int NB, int K, int lda, int ldb, int variant, int splitk, long long ws_bytes, int cus, int* out);
int octmae_gemm_bf16_ws(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux,
                        int NA, int NB, int K, int lda, int ldb, int ldc, int ldaux, int a_kstrided, int b_kstrided,
                        int epilogue, int splitk, void* split_ws, long long split_ws_bytes, void* stream);

/* Backward of epilogue 2 together with fc1's bias gradient, WITHOUT atomics (timm Mlp backward: fc2 dgrad, nn.GELU backward,
 * fc1.bias.grad; video_vit.py:174-179 under autograd):
 *   dX bf16 [M][K] = (dY[M][N] @ W[N][K]) * gelu'(pre[M][K]),   bias_grad[K] += column sums of dX   (bias_grad may be NULL).
 * Every 64-row slab of dX leaves its column sums as one row of `ws` (fp32 [octmae_dgelu_colsum_ws_rows(M)][K], caller-owned,
 * need not be initialised) with plain stores; a second launch (octmae_colsum_accum over `ws`) folds the rows into bias_grad:
 * at most 128 atomic adds per address instead of one per 64-row slab -- thousands of slabs adding to one [K] vector serialise
 * per address (~60 ns each: +0.67 ms on the decoder's fc2 at micro-batch 128, +0.13 ms on the encoder's).  Same result as
 * octmae_gemm_bf16(epilogue 4) up to the order of the fp32 additions.  Problems that take the 128-tile register-staged kernel ignore `ws`
 * and sum the columns of dX in a separate pass.  variant: kernel-selection bits as in octmae_linear_resid_rowscale, 0 = automatic. */
int octmae_dgelu_colsum_ws_rows(int M);
int octmae_linear_dgrad_dgelu(const void* W, const void* dY, void* dX, const void* pre, float* ws, float* bias_grad,
                              int M, int N, int K, int ldw, int ldy, int ldx, int ldpre, int variant, void* split_ws,
                              long long split_ws_bytes, void* stream);

/* Two weight gradients over the SAME token rows in one launch (the fc1 / fc2 and the qkv / proj Linears of a Block; backward of
 * video_vit.py:114-135 and timm Mlp under autograd):
 *   gW0 f32 [N0][K0] += dY0[M][N0]^T @ X0[M][K0],   gW1 f32 [N1][K1] += dY1[M][N1]^T @ X1[M][K1]      (dY, X bf16, row-major)
 *   gB0 / gB1: NULL, or f32 [N] += the column sums of dY (the bias gradient, as epilogue 5 of octmae_gemm_bf16 with C2)
 * The output tiles of both problems share one split over M: half the fp32-atomic epilogues of two separate launches and k-loops
 * twice as long.  splitk as in octmae_gemm_bf16 (0: chosen by the planner for the pair's tiles).  Short reductions on few tiles (one or two volumes per step: M <= 96 k-tiles of 64 rows)
 * run on 128 x 128 tiles instead when the cost model of csrc/gemm.hip prices that faster ("gemm_small"; gB is then a launch of its own).
 * Returns -2 when either problem does not take the 256-tile kernel (N or K < 256, an operand beyond a 32-bit buffer range): the
 * caller then issues two octmae_gemm_bf16 calls. */
int octmae_wgrad_accum_pair(const void* dY0, const void* X0, float* gW0, float* gB0, int N0, int K0, int ldy0, int ldx0, int ldw0,
                            const void* dY1, const void* X1, float* gW1, float* gB1, int N1, int K1, int ldy1, int ldx1, int ldw1,
                            int M, int splitk, void* stream);
/* The same with a workspace lent for the call: in deterministic mode the slabs of a k-split pair live there (those of gW0, then those
 * of gW1, behind the column-sum rows; octmae_wgrad_det_ws_bytes) and one fold launch serves both outputs; without one (or through the entry point above) the pair
 * runs unsplit there.  The split-K workspace of octmae_gemm_bf16_ws serves: only the bytes in front of its counters are written.
 * Outside deterministic mode the workspace is not looked at. */
int octmae_wgrad_accum_pair_ws(const void* dY0, const void* X0, float* gW0, float* gB0, int N0, int K0, int ldy0, int ldx0, int ldw0,
                               const void* dY1, const void* X1, float* gW1, float* gB1, int N1, int K1, int ldy1, int ldx1, int ldw1,
                               int M, int splitk, void* split_ws, long long split_ws_bytes, void* stream);
/* host side only: *bytes = the workspace to lend so that a weight gradient [N0][K0] over M rows (and its partner [N1][K1] of a pair;
 * 0, 0: a single launch) runs `slices` k slices in deterministic mode: the slabs (none for one slice) behind the head of the workspace,
 * which holds the rows of the bias gradient's fixed-order column sums (octmae_colsum_ws_rows(M) x N floats, rounded up to 256 bytes:
 * for a single launch when want_bias is set, for a pair always and for its wider dY).  With less lent the planner runs fewer slices,
 * and column sums whose rows do not fit take the form that needs no workspace; the plan queries report what runs. */
int octmae_wgrad_det_ws_bytes(int N0, int K0, int N1, int K1, int M, int want_bias, int slices, long long* bytes);
/* The fold of deterministic mode on its own: gW fp32 [NA][ldc] <- (...((gW + P_0) + P_1) ... + P_{S-1}) over [NA][NB], P_z = slabs +
 * z * slab_stride, fp32 [NA][ld_slab]; nothing outside [NA][NB] is read or written.  16-byte accesses when NB, ldc, ld_slab, slab_stride
 * are multiples of 4 and both pointers 16-byte aligned, element by element otherwise; any size (docs/OFFSET_RANGES.md). */
int octmae_wgrad_fold(float* gW, const float* slabs, int S, int NA, int NB, int ldc, int ld_slab, long long slab_stride, void* stream);

/* Planning arithmetic of the split-K weight gradients, host side only (no GPU is touched; for tests): the number of k slices a launch of
 * `tiles` output tiles over M token rows uses for a requested splitk (-> *slices), the first 64-row k-tile of every slice
 * (bounds[0 .. *slices], bounds[*slices] = ceil(M / 64); room for splitk + 1 ints), and -- the return value -- the length step between
 * neighbouring slices in 1/256 k-tiles (0 = equal slices; see "wgrad_stagger" above).  Negative: argument error. */
int octmae_wgrad_split_plan(int M, int splitk, int tiles, int* slices, int* bounds);
/* (in deterministic mode the slices are equal: ask with splitk = the k slices a plan query reports to get the bounds its launch runs) */
/* The launch plan of octmae_wgrad_accum_pair (csrc/gemm_plan.hpp: plan_wgrad_pair, with the 128- against 256-tile cost model), host side
 * only.  Returns 0 and writes 14 ints, or -2 as the entry point does:  out[0] kernel family (2: gemm256p_wgrad_pair_kernel,
 * 3: gemm128d_wgrad_kernel)  [1] workgroups  [2] k slices  [3] k-tiles per slice  [4] kstagger  [5] atomic1  [6] ring depth (family 3)
 * [7] bias-gradient route (1 inside the kernel, 3 a launch of its own before)  [8..10] / [11..13] tiles_a, tiles_b, cgroup of each problem.
 * splitk = 0: chosen by the planner, as in the entry point. */
int octmae_wgrad_pair_plan(int N0, int K0, int ldy0, int ldx0, int N1, int K1, int ldy1, int ldx1, int M, int splitk, int cus, int* out);
/* the plan of octmae_wgrad_accum_pair_ws with ws_bytes lent (the query above: none); out[5] == 3: slabs + the fold, as octmae_gemm_plan_ws */
int octmae_wgrad_pair_plan_ws(int N0, int K0, int ldy0, int ldx0, int N1, int K1, int ldy1, int ldx1, int M, int splitk,
                              long long ws_bytes, int cus, int* out);

/* The proj dgrad of an attention block together with the attention backward's per-query constant delta (flash-attn's `dsoftmax_sum`,
 * the backward of video_vit.py:130-134 under autograd):
 *   dX bf16 [M][K] = dY[M][N] @ W[N][K],   delta f32 [M][H] = -sum over each head's hd columns of dX * O     (O bf16 [M][K], K = H hd)
 * dX is the gradient of the attention output O; the fused attention backward needs rowsum(dO * O) per query and head, which is a
 * full extra pass over O and dO when computed on its own (0.13 / 0.25 ms per call at the ViT-L shapes) and 8 multiply-adds per
 * lane in this GEMM's epilogue, whose tiles hold whole heads.  delta is computed from the bf16-ROUNDED dX (what the attention
 * backward reads).  Returns -2 when the problem takes neither LDS-transposing kernel (N % 64 != 0, K % 8 != 0; M or K < 256
 * with the small-launch kernel off): the caller then uses octmae_gemm_bf16 and octmae_attn_bwd_fused.  variant: kernel-selection
 * bits (bit 8 forces "not applicable", bits 12-14 as above). */
int octmae_linear_dgrad_delta(const void* W, const void* dY, void* dX, const void* O, float* delta, int M, int N, int K, int ldw,
                              int ldy, int ldx, int ldo, int H, int hd, int variant, void* split_ws, long long split_ws_bytes, void* stream);

/* Stochastic depth (timm DropPath around both Block branches, video_vit.py:181-184 with drop_path > 0; fine-tune drivers use
 * 0.1-0.2): out f32 [M][N] = res + rowscale[m / rows_per_scale] * (X[M][K] @ W[N][K]^T + bias) -- the per-sample keep mask
 * (0 or 1/keep_prob) applied to the branch inside the residual epilogue.  nn.Linear layouts; variant: the kernel-selection bits of `epilogue` above (0x100 ... 0x4000), 0 = automatic. */
int octmae_linear_resid_rowscale(const void* W, const void* X, float* out, const float* bias, const float* res,
                                 const float* rowscale, int rows_per_scale, int N, int M, int K, int ldw, int ldx, int ldout,
                                 int ldres, int variant, void* split_ws, long long split_ws_bytes, void* stream);

/* ---- LayerNorm over the fp32 residual stream ---------------------------------------------------
 * nn.LayerNorm(eps=1e-6): models_mae_joint_res_flash_attn.py:799, video_vit.py:161,172,181-184, :489, :592.
 * fwd: y bf16 = (x - mean) * rstd * gamma + beta; saves mean, rstd (fp32 [M]).
 * bwd: dx f32 = (dres ? dres : 0) + LN'(dy); optional bf16 copy of dx; dgamma/dbeta/dxsum (column sums of
 *      dx = bias gradient of the preceding Linear) are ACCUMULATED (+=) when non-NULL (two-stage, deterministic, through the
 *      caller-provided workspace partial_ws).  D % 4 == 0, D <= 2048. */
int octmae_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean, float* rstd,
                         int M, int D, float eps, void* stream);
/* y bf16 = fmaf((x - mean[r]) * rstd[r], gamma, beta) from SAVED statistics: bit-equal to the y octmae_layernorm_fwd wrote for the same
 * x, gamma, beta when mean / rstd are the ones it saved.  Same domain (D % 4 == 0, D <= 2048), -1 otherwise. */
int octmae_ln_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y_bf16,
                    int M, int D, void* stream);
int octmae_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                         const float* dres, float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* dxsum,
                         float* partial_ws, int M, int D, void* stream);
/* number of floats `partial_ws` must hold for (M, D) */
int octmae_layernorm_bwd_ws_floats(int M, int D);

/* ---- slice-pooling head ----------------------------------------------------------------------------
 * RETFound-all (OCTCube/models_vit_3dhead_flash_attn.py:47-65 over models_vit_flash_attn.py:143-149): every slice of a volume is
 * its own image; x f32 [B*S][T][D] is the final token stream of all B*S slices (T = 1 + L, token 0 = cls).
 *   pooled[s] = mean of x[s][1..T-1]  (cls = 0)   or   x[s][0]  (cls = 1; LayerNorm of the cls row alone = norm(x)[:, 0])
 *   out f32 [B][D] = (1/S) sum over the S slices of volume b of LayerNorm(pooled[s]; gamma, beta, eps)     (fc_norm, slice mean)
 * fwd saves pooled f32 [B*S][D] and its LayerNorm statistics mean / rstd f32 [B*S] for the backward.
 * bwd: dx f32 [B*S][T][D] (written densely: the LayerNorm backward of dout[b] / S, divided by T-1 on tokens 1..T-1 and exact zeros
 *      on token 0 -- or on token 0 only in cls mode); optional 16-bit copy of dx (dx_bf16, NULL = none); dgamma / dbeta / dxsum
 *      (the column sums of dx over all rows) are ACCUMULATED (+=) when non-NULL.  All reductions run in a fixed order through the
 *      caller's workspace `ws` (no atomics: results are bit-reproducible).  D % 4 == 0, D <= 2048; B * S <= 65 535 (a grid dimension)
 *      and B * S * T <= 2^31 - 1 (rows are counted in int), -1 otherwise. */
int octmae_slice_pool_ws_floats(int BS, int T, int D);     /* floats `ws` must hold (forward and backward), BS = B * S */
int octmae_slice_pool_fwd(const float* x, const float* gamma, const float* beta, float* out, float* pooled, float* mean,
                          float* rstd, float* ws, int B, int S, int T, int D, int cls, float eps, void* stream);
int octmae_slice_pool_bwd(const float* dout, const float* pooled, const float* mean, const float* rstd, const float* gamma,
                          float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* dxsum, float* ws, int B, int S, int T,
                          int D, int cls, void* stream);

/* ---- volume transforms ------------------------------------------------------------------------------
 * The MONAI pipeline of Pre-training/custom_util/PatientDataset_inhouse.py:48-84 (create_3d_transforms; inference_utils.py:10 imports
 * it) over one raw scan: vol is one contiguous [D][H][W] device volume, dtype 0 = uint8, 1 = float32.  Both entry points are the
 * same code in the two builds of the library (no 16-bit operands).  -1: a non-positive size or a NULL vol / box6 / out; -2: another dtype.
 *   octmae_volume_box       CropForegroundd (select_fn = x > 0, margin 0): box6 = int32 {d0, d1, h0, h1, w0, w1} in DEVICE memory,
 *                           half-open, the bounding box of the voxels > 0 (negative values and NaN are background).  box6 is
 *                           initialised here; integer atomic min / max only, so the result does not depend on the order.  A volume
 *                           without a voxel > 0 gives the full extent {0, D, 0, H, 0, W} (MONAI would fail on the empty crop).
 *   octmae_volume_resample  out f32 [T][OH][OW] = Resized(mode="trilinear") = F.interpolate(align_corners=False) of the volume, or of
 *                           the sub-volume box6 names when box6 != NULL (read on the device: nothing returns to the host between the
 *                           two entry points; the six values are clamped into the volume).  Per axis scale = float(in) / float(out),
 *                           src = max(fma(scale, dst + 0.5f, -0.5f), 0) (one rounding, as ATen's CPU kernel computes it), taps
 *                           min(floor(src), in - 1) and the next one (clamped), weight src - floor.  flip_d / flip_w reverse the
 *                           output's first / last axis (RandFlipd spatial_axis 0 / 2, after the resize); normalize != 0 applies
 *                           NormalizeIntensityd(subtrahend, divisor, nonzero=True): y = (y - subtrahend) / divisor where y != 0. */
int octmae_volume_box(const void* vol, int dtype, int D, int H, int W, int* box6, void* stream);
int octmae_volume_resample(const void* vol, int dtype, int D, int H, int W, const int* box6, float* out, int T, int OH, int OW,
                           int flip_d, int flip_w, int normalize, float subtrahend, float divisor, void* stream);

/* ---- 2-D image transforms ---------------------------------------------------------------------------
 * The reference's torchvision-on-PIL chains over B-scans and fundus / en-face images, in one launch for n equally shaped images:
 *   Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:313-317   Resize((S, S), interpolation=3) -> ToTensor -> Normalize
 *   OCTCube/main_pretrain_oph_new.py:151-156, OCTCube/main_pretrain.py:133-137
 *                                       RandomResizedCrop(S, scale=(0.2, 1.0), interpolation=3) -> RandomHorizontalFlip -> ToTensor -> Normalize
 *   OCTCube/util/PatientDataset_inhouse_pretrain.py:247-252            frame.resize((512, h))  (Pillow's default filter: bicubic)
 * crop -> Pillow's two-pass 8-bit bicubic resize -> horizontal flip -> table, bit-equal to Pillow (Resample.c): per axis, with `in`
 * the crop's extent, scale = in / out, support = 2 max(scale, 1), window [xmin, xmin + xmax) = [max((int)(c - support + 0.5), 0),
 * min((int)(c + support + 0.5), in)) around c = (xx + 0.5) scale, bicubic (a = -0.5) weights in IEEE double summed in tap order,
 * k = (int)(w / sum * 2^22 +- 0.5); a pass is clamp((2^21 + sum pixel * k) >> 22, 0, 255) in 32-bit integers; the horizontal pass
 * runs first and is rounded to uint8, the vertical pass runs over those values.  The crop is torchvision's resized_crop of a PIL
 * image (crop, then resize): the windows clamp at the crop's edges.  Same code in the two builds of the library.
 *   src   uint8 [n][H][W] (C = 1) or [n][H][W][3] (C = 3, interleaved), contiguous
 *   top, left, ch, cw   the crop rectangle inside H x W; ch = cw = 0 (with top = left = 0): the whole image
 *   flip_w  reverse the output's last spatial axis (RandomHorizontalFlip, after the resize)
 *   lut   float32 [3][256] in DEVICE memory: ToTensor -> Normalize of every grey level per output channel; dst is then
 *         float32 [n][3][OH][OW] (a grey image is replicated: convert("RGB")).  NULL: dst is uint8 [n][OH][OW] / [n][OH][OW][3].
 * -1, before any launch: a NULL src / dst, n or a size < 1, C not 1 or 3, a crop outside the image or with exactly one of ch, cw
 * zero, or a reduction so strong that one output row's windows do not fit the kernel's 64 KiB of LDS (a factor in the hundreds).
 * octmae_image_resample_plan is HOST ONLY: the output rows of a workgroup's tile (32, 16, 8, 4, 2 or 1) and the LDS bytes of the
 * launch octmae_image_resample would make for this geometry (csrc/image2d_plan.hpp); -1 as above. */
int octmae_image_resample(const void* src, int n, int H, int W, int C, int top, int left, int ch, int cw, int OH, int OW, int flip_w,
                          const float* lut, void* dst, void* stream);
int octmae_image_resample_plan(int H, int W, int C, int ch, int cw, int OH, int OW, int* tile_h, int* lds_bytes);

/* ---- RandAugment's image operations (csrc/augment2d.hip) -------------------------------------------
 * The Pillow operations of the reference's OCTCube/util/rand_augment.py (timm's auto_augment; the train chain of util/datasets.py
 * build_transform), on n equally sized uint8 [n][H][W][3] images in device memory, bit-equal to Pillow.  The host draws the
 * decisions (octcubem_amd/rand_augment.py) and writes one descriptor per image; nothing returns to the host in between.
 *
 * octmae_aug_desc, one per image:
 *   kind 0 none       copy (or normalise only)
 *        1 table      mode 0 Invert, 1 Posterize(iarg bits), 2 Solarize(iarg threshold), 3 SolarizeAdd(iarg, threshold 128),
 *                     4 Brightness(factor), 5 Contrast(factor), 6 AutoContrast, 7 Equalize; modes 5-7 read the image's histograms
 *        2 colour     blend(L replicated, pixel, factor)
 *        3 sharpness  blend(ImageFilter.SMOOTH, pixel, factor)
 *        4 affine     Image.transform(size, AFFINE, m, mode, fillcolor = fill): mode 2 bilinear, 3 bicubic (Pillow's numbers);
 *                     source position m0 (x + 0.5) + m1 (y + 0.5) + m2, m3 (x + 0.5) + m4 (y + 0.5) + m5 in double
 *   blend = Pillow's ImagingBlend with factor as a C float.
 *
 * octmae_image_stats: hist uint32 [n][4][256] (device) = the histograms of R, G, B and L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
 * of every image i with needed[i] != 0 (needed: n device bytes, or NULL = all); the rows of the other images are zero.
 * octmae_image_augment: dst = the image's op applied; uint8 [n][H][W][3], or with lut (float32 [3][256], device: ToTensor -> Normalize
 * as in octmae_image_resample) float32 [n][3][H][W].  desc: n descriptors in DEVICE memory; desc_host: the same n descriptors in host
 * memory, or NULL -- when given they are checked before the launch.  hist: octmae_image_stats' output, NULL when no op reads it.
 * src and dst must not overlap.
 * -1, before any launch: a NULL src / dst / desc / hist (stats), src == dst, n or a size < 1, H W > 2^30; for desc_host, an unknown
 * kind or mode, a negative Posterize, a SolarizeAdd outside 0..255, a NaN factor, a non-finite matrix, or a mode 5-7 table op
 * without hist. */
typedef struct {
  int kind, mode;
  double m[6];
  float factor;
  int iarg;
  unsigned char fill[4];     /* R, G, B, unused */
  int reserved;
} octmae_aug_desc;           /* 72 bytes */
int octmae_image_stats(const void* src, int n, int H, int W, const unsigned char* needed, unsigned* hist, void* stream);
int octmae_image_augment(const void* src, int n, int H, int W, const octmae_aug_desc* desc, const octmae_aug_desc* desc_host,
                         const unsigned* hist, const float* lut, void* dst, void* stream);

/* ---- attention -----------------------------------------------------------------------------------
 * softmax(q k^T * scale) v, non-causal, no dropout: video_vit.py:130-134 (flash path: flash_attn MHA,
 * models_mae_joint_res_flash_attn.py:131-149).  qkv bf16 [B][N][3][H][HD]; o, dout bf16 [B][N][H][HD];
 * lse f32 [B][H][N] (natural log); rowc_ws f32 [2][B][H][N] workspace; dqkv bf16 like qkv.  HD in {32, 64}.
 * flag_ws: one int of device workspace, or NULL.  Non-NULL enables the optimistic forward: a kernel without running-max
 * tracking runs first and raises *flag_ws if any softmax row sum is not a finite positive number; the online-max kernel is
 * always enqueued behind it and returns immediately unless the flag is set (no host synchronisation).  In the half build
 * (octmae_lp_dtype() == 1) flag_ws is ignored and only the online-max kernel runs: the optimistic kernel's un-normalised P does not
 * fit half's range (P = e^-20 rounds to zero, e^+12 overflows) and its give-up test assumes bfloat16's exponent range.
 * Address ranges (docs/OFFSET_RANGES.md): one SAMPLE's qkv rows are reached through 32-bit byte offsets, everything across samples
 * through 64-bit pointers.  -1, before any launch: (N + 512) * 3 * H * HD * 2 >= 2^32 bytes, B or H above 65 535 (forward and the
 * dQ / dK/dV pair: the grid's z and y), B * N >= 2^31 - 65 536 (octmae_attn_bwd_rowconst); the fused forms: the same per-sample range, B * H >= 2^23 (one workgroup of
 * 512 threads per (b, h); a launch holds fewer than 2^32 threads), B * (N / 64 + 2) above 2^31 - 1. */
int octmae_attn_fwd(const void* qkv, void* o, float* lse, int* flag_ws, int B, int N, int H, int HD, float scale, void* stream);
int octmae_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, float* rowc_ws, void* dqkv, int B,
                    int N, int H, int HD, float scale, void* stream);
/* octmae_attn_bwd = octmae_attn_bwd_dq_rowconst + octmae_attn_bwd_dkv: the dQ kernel computes the per-query constants the
 * gradient kernels start their accumulators from, rowc[0] = -lse * log2(e), rowc[1] = -rowsum(dO * O), for its own query rows
 * and WRITES them to rowc [2][B][H][N] for the dK/dV kernel.  The separate pre-pass (rowconst) followed by octmae_attn_bwd_dq,
 * which only reads rowc, is the same computation in three launches. */
int octmae_attn_bwd_dq_rowconst(const void* qkv, const void* o, const void* dout, const float* lse, float* rowc, void* dqkv, int B,
                                int N, int H, int HD, float scale, void* stream);
int octmae_attn_bwd_rowconst(const void* o, const void* dout, const float* lse, float* rowc, int B, int N, int H, int HD,
                             void* stream);
int octmae_attn_bwd_dq(const void* qkv, const void* dout, const float* rowc, void* dqkv, int B, int N, int H, int HD, float scale,
                       void* stream);
int octmae_attn_bwd_dkv(const void* qkv, const void* dout, const float* rowc, void* dqkv, int B, int N, int H, int HD, float scale,
                        void* stream);

/* Fused backward (csrc/attn_bwd.hip): S, dP and exp once per score for all three gradients (5 matrix products and 1 exp per
 * score instead of 7 and 2), dQ summed over key blocks in an fp32 workspace by one workgroup per (batch, head) in program
 * order -- no atomics, bit-reproducible.  Same inputs and outputs as octmae_attn_bwd; `ws` is a device workspace of
 * octmae_attn_bwd_fused_ws_kib(B, N, H, HD) KiB (dQ fp32 [B][H][N][HD] + the padded per-query constants), contents
 * irrelevant on entry.  Three launches: per-query constants, full key blocks (512 keys at HD 32, 256 at HD 64), remaining keys
 * + conversion of dQ to bf16. */
int octmae_attn_bwd_fused_ws_kib(int B, int N, int H, int HD);
int octmae_attn_bwd_fused(const void* qkv, const void* o, const void* dout, const float* lse, void* ws, void* dqkv, int B, int N,
                          int H, int HD, float scale, void* stream);
/* octmae_attn_bwd_fused with delta (fp32 [B * N][H], from octmae_linear_dgrad_delta) supplied instead of O: the per-query constants are
 * transposed and padded from it, no pass over O and dO.  Same workspace, same outputs. */
int octmae_attn_bwd_fused_delta(const void* qkv, const void* dout, const float* lse, const float* delta, void* ws, void* dqkv, int B,
                                int N, int H, int HD, float scale, void* stream);

/* ---- random masking indices ---------------------------------------------------------------------
 * MaskedAutoencoderViT.random_masking index part, models_mae_joint_res_flash_attn.py:349-369:
 * ids_shuffle = argsort(noise) with ties -> lower index, ids_restore = its inverse, ids_keep = first len_keep,
 * mask = 0 keep / 1 remove in original order.  int64 outputs (torch index dtype).  ids_shuffle may be NULL.
 * L <= 16384. */
int octmae_random_masking_ids(const float* noise, long long* ids_restore, long long* ids_keep, long long* ids_shuffle,
                              float* mask, int B, int L, int len_keep, void* stream);

/* ---- activation recomputation --------------------------------------------------------------------
 * act[i] = lp(gelu(float(pre[i]))) over n 16-bit values: bit-equal to the second output of the GELU epilogue (octmae_gemm_bf16
 * epilogue 2) whose first output is `pre`.  n % 8 == 0, 16-byte aligned pointers; -1 otherwise. */
int octmae_gelu_apply(const void* pre_bf16, void* act_bf16, long long n, void* stream);

/* ---- token plumbing ------------------------------------------------------------------------------ */
int octmae_cast_f32_bf16(const float* src, void* dst_bf16, long long n, void* stream);
/* dst bf16 [R][D] = rowscale[r / rows_per_scale] * src f32 [R][D]: the gradient entering a stochastic-depth branch */
int octmae_cast_rowscale_f32_bf16(const float* src, const float* rowscale, void* dst_bf16, long long R, int D,
                                  int rows_per_scale, void* stream);
/* out[c] += sum_r in[r][c]  (nn.Linear bias gradient) */
int octmae_colsum_accum(const void* in, int in_is_bf16, float* out, int M, int N, int ld, void* stream);
/* Both forms add in a fixed order (until ABI 26 the row splits of more than 256 rows added to `out` atomically, in the order they
 * finished: an ACCUMULATED gradient depended on that order in its last bit).  Without a workspace one workgroup owns 8 columns and all
 * the rows; with one the rows are split over workgroups, every split leaves one row of `ws` (fp32 [octmae_colsum_ws_rows(M)][N],
 * caller-owned, need not be initialised; 0 rows: ws may be NULL) and a second launch adds the rows to `out` in their order: the
 * form for many rows. */
int octmae_colsum_ws_rows(int M);
int octmae_colsum_accum_ws(const void* in, int in_is_bf16, float* out, float* ws, int M, int N, int ld, void* stream);
/* im2col of the kept tokens for PatchEmbed's Conv3d(k = s = (tp,p,p)), video_vit.py:70-83 + the gather at
 * models_mae_joint_res_flash_attn.py:363: out bf16 [B*nkeep][C*tp*p*p] in conv-weight order (c,u,py,px).
 * ids: [B][nkeep] int64 (ids_is_i64=1) or int32, NULL = tokens 0..nkeep-1. */
int octmae_patch_gather(const float* imgs, const void* ids, int ids_is_i64, void* out_bf16, int B, int C, int T, int H,
                        int W, int tp, int p, int nkeep, void* stream);
/* encoder input: cls concat + gathered sep pos-embed add, models_mae_joint_res_flash_attn.py:409-478 */
int octmae_enc_assemble(const void* tok_bf16, const float* pos, const float* cls, const float* pos_cls,
                        const long long* ids_keep, float* x, int B, int nkeep, int D, void* stream);
/* decoder input: mask tokens + un-shuffle + cls + pos-embed, models_mae_joint_res_flash_attn.py:515-573.
 * emb_has_cls = 1 (2-D MAE, OCTCube/models_mae.py:175-178): emb has 1 + nkeep rows per sample, row 0 is the cls row. */
int octmae_dec_assemble(const void* emb_bf16, const float* mask_token, const float* dpos, const float* dcls,
                        const float* dpos_cls, const long long* ids_restore, float* x, int B, int nkeep, int L, int D,
                        int emb_has_cls, void* stream);
/* out bf16[b*n+i][:] = src f32[b][1+ids[b][i]][:]  (backward of both assemblies w.r.t. the token rows) */
int octmae_gather_rows_cast(const float* src, const long long* ids, void* out_bf16, int B, int n, int src_rows, int D,
                            void* stream);
/* backward of the keep-gather w.r.t. the positional table (autograd of torch.gather at models_mae_joint_res_flash_attn.py:442-447;
 * ATen: index_add_): out f32 [L][D] (+)= sum over samples b that kept token l (ids_restore[b][l] < nkeep) of
 * src f32 [b][row0 + ids_restore[b][l]][:], src has src_rows rows per sample.  Deterministic (ascending b), no atomics. */
int octmae_scatter_add_rows(const float* src, const long long* ids_restore, float* out, int B, int nkeep, int L, int D,
                            int src_rows, int row0, int accumulate, void* stream);
/* backward of the decoder assembly w.r.t. decoder_pos_embed and mask_token in one pass over dx f32 [B][1 + L][D]
 * (models_mae_joint_res_flash_attn.py:515-573 under autograd): ddpos [L][D] = sum_b dx[b][1 + l], dmask_part [L][D] = the same sum
 * over the samples in which token l was masked; the mask-token gradient is the column sum of dmask_part. */
int octmae_dec_assemble_bwd(const float* dx, const long long* ids_restore, float* ddpos, float* dmask_part, int B, int nkeep, int L,
                            int D, void* stream);
/* fused patchify + per-token MSE, models_mae_joint_res_flash_attn.py:289-314, :613-650.  pred f32 [B][L+1][PD]
 * (row 0 = cls, ignored); loss_tok f32 [B][L].  frame_idx int32 [pred_t_dim] or NULL (identity).  The B * (L + 1) token rows
 * are counted in int: -1 beyond 2^31 - 1 (both entry points); the elements are reached through 64-bit pointers. */
int octmae_mse_fwd(const float* pred, const float* imgs, const int* frame_idx, float* loss_tok, int B, int C, int T, int H,
                   int W, int u_sz, int p, int L, int norm_pix, void* stream);
/* dpred bf16 [B][L+1][PD] = *coef * mask * (pred - target), cls rows zero (backward of :649-663) */
int octmae_mse_bwd(const float* pred, const float* imgs, const int* frame_idx, const float* mask, const float* coef,
                   void* dpred_bf16, int B, int C, int T, int H, int W, int u_sz, int p, int L, int norm_pix, void* stream);
/* The reconstruction volumes of the validation pass (Pre-training/engine_pretrain.py:207-357 eval_one_epoch ->
 * custom_util/misc.py:1225-1299 get_visible_images: unpatchify of pred and of the mask, index_select of the frames,
 * untransform_image :727-728, the two blends) in one pass.  One channel only.
 *   pred       f32, token 0 of sample 0; [L][PD] per sample, PD = u_sz * p * p, samples pred_batch_stride FLOATS apart (>= L * PD,
 *              a multiple of 4): a contiguous [B][L][PD] tensor, or the [:, 1:, :] view of the decoder's [B][1 + L][PD] output
 *   imgs       f32 [B][1][T][H][W];  mask f32 [B][L], != 0 = removed
 *   frame_idx  NULL (predicted frame f is frame f of the volume; then Tp <= T) or Tp = (L / ((H/p) * (W/p))) * u_sz int32 source
 *              frames, as octmae_mse_fwd takes them (clamped into [0, T) on the device)
 *   out        uint8 [B][4][Tp][H][W]: 0 = g(x), 1 = mask ? 0 : g(x), 2 = g(pred), 3 = mask ? g(pred) : g(x), pred un-shuffled from
 *              (t, h, w | u, py, px) to (frame, y, x);  g(v) = (int) clip((v * s + m) * 255, 0, 255), s = float(76.03 / 255),
 *              m = float(45.79 / 255), the multiply, the add and the second multiply each rounded to fp32 on its own: bit-equal to
 *              the reference's three tensor ops.  A non-finite v gives 0 (the reference's .int() of a NaN is undefined).
 *   denorm     0: the reference's behaviour (the raw prediction, also for a norm_pix_loss model).  1: pred * sqrt(var + 1e-6) + mean
 *              first, mean / unbiased var of that token's target patch as the norm_pix branch of the loss takes them (fp32).
 * pred_batch_stride is a long long, as every 64-bit count of this header (octmae_cast_f32_bf16's n): the same type as long on LP64.
 * -1: NULL / non-positive / misaligned arguments, p % 4, W % 4, PD % 4, H % p, W % p, L not a multiple of the (H/p) * (W/p) grid,
 * a batch stride below L * PD.  -2: denorm outside {0, 1}, more than 2^31 - 1 tokens. */
int octmae_mae_compose(const float* pred, long long pred_batch_stride, const float* imgs, const int* frame_idx, const float* mask,
                       uint8_t* out, int B, int T, int H, int W, int u_sz, int p, int L, int denorm, void* stream);

/* ---- the 2-D half of the validation pass (csrc/recon2d.hip) -------------------------------------------
 * The four panels of octmae_mae_compose for C channels and any affine grey scale (custom_util/misc.py:1134-1223 get_visible_images_2d
 * with untransform_image_no_normalization :730-731, or the inverse of a Normalize transform).
 *   pred       f32 [L][PD] per sample, PD = u_sz * p * p * C in the order (a < u_sz, py, px, c < C), samples pred_batch_stride floats
 *              apart as in octmae_mae_compose.  u_sz = 1, T = 1: models_mae_2d.patchify's order; C = 1: models_mae.patchify's.
 *   imgs       f32 [B][C][T][H][W];  mask f32 [B][L], != 0 = removed.  Predicted frame f is frame f of the volume (Tp <= T).
 *   out        uint8 [B][4][Tp][H][W][C], channels innermost; panels as octmae_mae_compose.
 *   level      g_c(v) = (int) clip(((v * scale_c) + shift_c) * 255, 0, 255), each operation rounded to fp32 on its own; a non-finite v
 *              gives 0.  scale 1, shift 0: untransform_image_no_normalization bit for bit.  C = 1: only scale0 / shift0 are used.
 *   denorm     as octmae_mae_compose: mean / unbiased variance (+ 1e-6) of the target patch over all PD elements.
 * -1: what octmae_mae_compose answers with -1, C outside {1, 3}, a non-finite scale or shift, more predicted frames than T.
 * -2: u_sz > 1 with C > 1 (no caller states that element order), denorm outside {0, 1}, more than 2^31 - 1 tokens. */
int octmae_mae_compose_nc(const float* pred, long long pred_batch_stride, const float* imgs, const float* mask, uint8_t* out, int B, int C,
                          int T, int H, int W, int u_sz, int p, int L, float scale0, float scale1, float scale2, float shift0,
                          float shift1, float shift2, int denorm, void* stream);
/* find_and_convert_large_white_region(image, 'tensor') (custom_util/misc.py:1438-1484) for a batch, in place, two launches on `stream`.
 *   imgs    f32 [B][T][H][W], 16-byte aligned, W % 4 == 0.  white = frame 0 > max - k * (max - min) over all T frames, k = float(15 / 255),
 *           the difference, the product and the second difference each rounded to fp32; a NaN anywhere: nothing is white.
 *           Per row of frame 0: the run of white columns from the first white column f (followed iff f < left_idle_from; when it ends at
 *           a column e >= left_ext_from, [e, e + 5) is marked too) and the run down from the last white column l (followed iff
 *           l >= right_live_from; when it ends at a column s < right_ext_below the reference assigns [s : s - 5], which is
 *           [s, W + s - 5) for s <= 4 and empty otherwise).  Marked pixels become 0, then every frame becomes a copy of frame 0.
 *   region  uint8 [B][T][H][W], written in full: 1 = marked, the same for every frame.
 *   ws      octmae_white_border_ws_floats(B, T, H, W) floats (caller-owned, need not be initialised); the query returns -1 for
 *           non-positive sizes or W % 4, -2 past 2^31 - 1.
 * The four limits are the reference's comparisons with 0.01 * W, 0.05 * W, W - 0.01 * W and W - 0.05 * W, evaluated by the caller in
 * double (octcubem_amd/ops.py: white_border_limits); each lies in [0, W + 1].  -1: NULL / non-positive / misaligned arguments, W % 4,
 * a limit outside its range.  -2: more than 2^31 - 1 rows. */
int octmae_white_border_ws_floats(int B, int T, int H, int W);
int octmae_white_border(float* imgs, uint8_t* region, float* ws, int B, int T, int H, int W, int left_idle_from, int left_ext_from,
                        int right_live_from, int right_ext_below, void* stream);

/* ---- full-coverage reconstruction and error maps of the 3-D MAE (csrc/cover.hip) -----------------------
 * No counterpart in the reference, whose validation pass predicts the masked three quarters of a volume once.  K forwards over
 * complementary masks (models_mae.cover_noise) hide every token at least once; the masked predictions are summed per token and one
 * finishing pass gives the mean prediction as grey levels, its squared error against the scan and a score per token.
 * Shapes and conventions are octmae_mae_compose's: one channel; pred f32 [L][PD] per sample, PD = u_sz * p * p, samples
 * pred_batch_stride FLOATS apart (>= L * PD, a multiple of 4: the [:, 1:, :] view of the decoder's output is read in place); mask f32
 * [B][L], != 0 = removed; frame_idx NULL or Tp int32 source frames, clamped on the device; 64-bit element offsets, token rows in int.
 *
 * octmae_cover_accumulate: one pass into the running sums.
 *   sum   f32 [B][L][PD], contiguous, 16-byte aligned;  cnt int32 [B][L]
 *   first != 0: every row is written -- a removed token's row of sum is its row of pred (a copy) and its cnt 1, every other row is
 *               +0.0f and its cnt 0; nothing has to be zeroed in front.
 *   first == 0: a removed token gets sum += pred (one fp32 add per element) and cnt += 1; the rows of the other tokens are neither read
 *               from pred nor written.  Pass by pass the result has the bits of torch.where(mask, sum + pred, sum).
 * -1: NULL / non-positive / misaligned arguments, PD % 4, a batch stride below L * PD or not a multiple of 4, pred == sum.
 * -2: more than 2^31 - 1 tokens.
 *
 * octmae_cover_finish: the sums into volumes.  For a token with cnt > 0:
 *   v      = sum / (float) cnt, a correctly rounded fp32 division; with denorm == 1 then v = fma(v, sqrt(var + 1e-6), mean) with the
 *            mean / unbiased variance of the token's target patch, the arithmetic of octmae_mae_compose with denorm == 1
 *   recon  uint8 [B][Tp][H][W] = g(v), un-shuffled from (t, h, w | u, py, px) to (frame, y, x): what panel 2 of octmae_mae_compose
 *            holds for pred = v (g: see there; a non-finite v gives 0)
 *   err    f32 [B][Tp][H][W] or NULL: d * d with d = v - x, x the source frame's voxel; the subtraction and the product each rounded on
 *            their own (no fused multiply-add in any formula of this entry point but the denorm one above)
 *   score  f32 [B][L] or NULL: the mean of the token's PD squared errors (computed whether or not err is stored): per lane the float4
 *            groups q = lane, lane + 64, ... as ((e0 + e1) + (e2 + e3)) added in ascending order, the 64 lanes by the wave reduction,
 *            one division by PD.  A fixed order: two calls give the same bits.
 * A token with cnt == 0 draws the input: recon = g(x), err = 0, score = 0.  No atomics; a token's outputs depend on its own inputs only.
 * -1: NULL sum / cnt / imgs / recon, non-positive or misaligned arguments (sum, imgs, err: 16 bytes), p % 4, W % 4, PD % 4, H % p,
 * W % p, L not a multiple of the (H/p) * (W/p) grid, more predicted frames than T without frame_idx.
 * -2: denorm outside {0, 1}, more than 2^31 - 1 tokens.  Same code in the two builds of the library. */
int octmae_cover_accumulate(const float* pred, long long pred_batch_stride, const float* mask, float* sum, int* cnt, int B, int L, int PD,
                            int first, void* stream);
int octmae_cover_finish(const float* sum, const int* cnt, const float* imgs, const int* frame_idx, uint8_t* recon, float* err, float* score,
                        int B, int T, int H, int W, int u_sz, int p, int L, int denorm, void* stream);

/* ---- low-rank adapters on the Block's Linears (csrc/lora.hip) -------------------------------------------
 * No counterpart in the reference, which fine-tunes every weight.  An adapted Linear computes with W + s B A (W f32 [O][I], A f32
 * [r][I], B f32 [O][r], s = alpha / r); its GEMMs run unchanged on a merged 16-bit operand, and the adapter gradients come from skinny
 * products over the X and dY the weight-gradient GEMM would have read -- no [O][I] gradient exists.  rp = r rounded up to 16.
 * The contract of every entry point below: 1 <= r <= 64; I and O are the widths of 16-bit GEMM operands, multiples of 8 (16-byte operand
 * loads), and so are the leading dimensions ldx, ldy; W, A, out_w, X, dY, A_lp, B_lp and ws are 16-byte aligned, B, gA, gB 4-byte.
 * -1 before any launch otherwise.  Row offsets are 64-bit ((size_t) row * ld): operands of any size (docs/OFFSET_RANGES.md).
 *
 * octmae_lora_merge: delta = fmaf(B[o][k], A[k][i], delta) for k = 0 .. r - 1 in that order (from +0), v = fmaf(s, delta, W[o][i]);
 *   out_w [O][I] = v (out_is_f32 = 1) or v rounded once to the 16-bit operand type (0): the SAME v, so the cast of the f32 output has the
 *   bits of the 16-bit output.  A_lp [rp][I] / B_lp [O][rp] (either may be NULL): A and B rounded to the operand type, +0 in rows /
 *   columns r .. rp - 1.  With B == 0 the 16-bit output has the value of cvt(W).
 *
 * octmae_lora_wgrad: X [M][I] (rows ldx apart), dY [M][O] (rows ldy apart), A_lp, B_lp as written by the merge ->
 *   gA f32 (rows ldga >= I apart; rows 0 .. r - 1 touched) += s U^T X,  U = dY B_lp   [M][rp]
 *   gB f32 (rows ldgb >= r apart; columns 0 .. r - 1 touched) += s dY^T T,  T = X A_lp^T [M][rp]
 *   T and U: fp32 MFMA accumulation, one rounding to the operand type.  The two outer products reduce over row chunks of
 *   octmae_lora_plan's size; each chunk's fp32 partial is stored to a slab of ws, and g = fmaf(s, ((P_0 + P_1) + ...) + P_{n-1}, g)
 *   in ascending chunk order.  No atomics: two calls give the same bits, in and out of deterministic mode.  gA or gB may be NULL (not
 *   both).  This is the two-pass form: X and dY are read twice (projection, then outer products).
 *   ws: at least *bytes of octmae_lora_ws_bytes(M, I, O, rp, &bytes), need not be initialised; ws_bytes below that: -1.
 * octmae_lora_plan: host side only; out[0] rows per chunk (a multiple of 32, at least 256), [1] chunks, [2] / [3] the 64-column tiles of
 *   X / dY (workgroups of the outer-product launch = ([2] + [3]) * [1]).  octmae_lora_ws_bytes: host side only, as
 *   octmae_wgrad_det_ws_bytes; -1 on bad arguments. */
int octmae_lora_merge(const float* W, const float* A, const float* B, float s, int O, int I, int r, void* out_w, int out_is_f32,
                      void* A_lp, void* B_lp, void* stream);
int octmae_lora_wgrad(const void* X, int ldx, const void* dY, int ldy, const void* A_lp, const void* B_lp, float s, int M, int I, int O,
                      int r, float* gA, int ldga, float* gB, int ldgb, void* ws, long long ws_bytes, void* stream);
int octmae_lora_plan(int M, int I, int O, int rp, int* out);
int octmae_lora_ws_bytes(int M, int I, int O, int rp, long long* bytes);

/* ---- saliency: input gradients, Grad-CAM, heat volumes (csrc/saliency.hip) ---------------------------
 * retinal-COEM/src/oph_vis_util/base_cam_retclip_3mod.py (the reference's Grad-CAM base class over pytorch_grad_cam) and its
 * compute_input_gradient=True.  All of them are deterministic (no floating-point atomics).
 *
 * The adjoint of octmae_patch_gather: dimgs f32 [B][C][T][H][W] receives, at the voxels of kept token ids[b][i], row b * nkeep + i of
 * dpatch ([B*nkeep][C*tp*p*p] of the library's 16-bit operand type, conv-weight order (c,u,py,px): what the PatchEmbed dgrad GEMM
 * writes), widened exactly; every voxel of a token that was not kept is +0.0f.  The result does not depend on what dimgs held before:
 * with ids and nkeep < L a zero-fill pass runs first on `stream`; with ids == NULL (tokens 0..nkeep-1) or nkeep == L the one pass
 * writes every voxel.  CONTRACT: the ids of one sample are distinct (the masking kernel's); not checked on the device (an id outside
 * [0, L) is clamped into the volume).  -1: the argument rules of octmae_patch_gather (NULL, p % 8, H % p, W % p, T % tp, W % 4,
 * nkeep > L), non-positive sizes, pointers that are not 16-byte aligned.  -2: C*tp*p*p or B * L above 2^31 - 1. */
int octmae_patch_scatter(const void* dpatch_lp, const void* ids, int ids_is_i64, float* dimgs, int B, int C, int T, int H, int W,
                         int tp, int p, int nkeep, void* stream);
/* Grad-CAM's reduction (pytorch_grad_cam GradCAM.get_cam_weights + BaseCAM.get_cam_image + the ReLU) over f32 token streams
 * [B][n_prefix + L][C]; the n_prefix leading rows (the cls token; 0 allowed) are never read.
 *   w[b][c]   = (sum_l G[b][n_prefix + l][c]) / L          f32 [B][C]; rows split over workgroups, the partial sums in ws folded in
 *               ascending order by a second launch.  ws: octmae_cam_ws_floats(B, L, C) floats (-1 / -2 for sizes it refuses).
 *   cam[b][l] = max(0, sum_c w[b][c] * A[b][n_prefix + l][c])   f32 [B][L]; one wave per token row.
 * -1, before any launch: NULL, non-positive B / L / C, n_prefix < 0, C % 4, pointers not 16-byte aligned.  -2: B above 65535. */
int octmae_cam_ws_floats(int B, int L, int C);
int octmae_cam_weights(const float* G, float* w, float* ws, int B, int L, int n_prefix, int C, void* stream);
int octmae_cam_tokens(const float* A, const float* w, float* cam, int B, int L, int n_prefix, int C, void* stream);
/* Eigen-smoothed Grad-CAM (pytorch_grad_cam's eigen_smooth: get_2d_projection on the weighted activations) without the [L][C] product
 * and without an SVD.  Per sample, with M[l][c] = w[c] A[n_prefix + l][c] and Mc = M - (mean over l of M), the map is Mc v1, v1 the
 * first right singular vector of Mc, found by `iters` power iterations on Mc^T Mc.  Neither M nor Mc is ever stored:
 *   abar[c] = mean_l A[l][c]                       (the two launches of octmae_cam_weights, on A)
 *   v = 1 / sqrt(C) in every column, then `iters` times
 *     u[l] = sum_c q[c] A[l][c] - sum_c q[c] abar[c],  q = v o w          one wave per token row; both sums in the same order
 *     t[c] = w[c] (sum_l u[l] A[l][c] - abar[c] sum_l u[l])              row splits, folded in ascending order
 *     v    = t / ||t||_2                                                 one workgroup per sample; ||t|| = 0 leaves v as it is
 *   proj = Mc v (the u of one more pass), lambda = ||proj||^2, residual = ||Mc^T proj - lambda v||_2 / lambda
 *   proj is negated when sum_l proj[l] (Mc 1)[l] < 0: the map correlates positively with the centred plain CAM.  (LAPACK's sign is
 *   arbitrary and pytorch_grad_cam keeps whatever it gets: a deliberate departure.)
 *   cam[b][l] = relu ? max(0, proj) : proj          f32 [B][L];  residual f32 [B]
 * 3 launches per iteration and 7 around them; the iteration count is fixed by the argument, there is no convergence test on the device:
 * `residual` is how a caller sees a map that has not converged (it falls as (sigma2 / sigma1)^(2 iters)).  lambda == 0 (L == 1, constant
 * columns whose mean is exact, w == 0): the map is all zero and the residual 0.  A non-finite value in the patch rows or the weights of
 * sample b makes residual[b] NaN (the map of that sample is then unspecified); every other sample is untouched by it.  Deterministic:
 * no floating-point atomics, every sum in a fixed order.  The n_prefix leading rows are never read.
 * ws: octmae_cam_eigen_ws_floats(B, L, C) floats (-1 / -2 for sizes it refuses), 16-byte aligned.
 * -1, before any launch: NULL, non-positive B / L / C / iters, n_prefix < 0, C % 4, A / w / ws not 16-byte aligned.  -2: B above 65535. */
int octmae_cam_eigen_ws_floats(int B, int L, int C);
int octmae_cam_eigen(const float* A, const float* w, float* cam, float* residual, float* ws, int B, int L, int n_prefix, int C,
                     int iters, int relu, void* stream);
/* One pass of test-time-augmentation smoothing folded into an accumulator (pytorch_grad_cam: scale_cam_image on the map of each
 * augmented pass, the augmentation undone, then the mean): cam, acc f32 [B][n], n = rows x width,
 *   acc[b][r][x] (first ? = : +=) weight * (cam[b][r][x'] - mn_b) / (1e-7f + (mx_b - mn_b)),   x' = flip ? width - 1 - x : x,
 * mn_b / mx_b the minimum / maximum of cam[b] (written to mnmx f32 [B][2] by a first launch).  A constant map contributes 0.
 * acc and cam must not overlap.  -1, before any launch: NULL, non-positive B / n / width, n % width.  -2: n above 2^31 - 1 - 256. */
int octmae_cam_accumulate(float* acc, const float* cam, float* mnmx, int B, int n, int width, int flip, float weight, int first,
                          void* stream);
/* Heat volume of a coarse saliency map: m f32 [B][t][h][w] -> out uint8 [B][F][H][W].  Per sample mn = min m, mx = max m (written to
 * mnmx f32 [B][2] by a first launch), v = (m - mn) / (1e-7f + (mx - mn)) on the COARSE map, then v resampled linearly along t -> F and
 * bilinearly over (h, w) -> (H, W) with F.interpolate's align_corners=False positions (src = (dst + 0.5) in / out - 0.5, negative -> 0,
 * upper neighbour clamped; equal sizes on an axis are the identity on it), out = (uint8) floorf(255 v).  A constant map gives 0.
 * pytorch_grad_cam upsamples before it scales; here the order is the other way round so that min / max run over the coarse map only.
 * -1, before any launch: NULL, a non-positive size, W % 4, out not 4-byte aligned.  -2: t * h * w above 2^31 - 1. */
int octmae_heatmap(const float* m, float* mnmx, uint8_t* out, int B, int t, int h, int w, int F, int H, int W, void* stream);

/* ---- ranking metrics of the fine-tune evaluation (csrc/metrics.hip) ---------------------------------
 * OCTCube/engine_finetune.py:251-343 and :786-792 judge a run by scikit-learn's roc_auc_score, average_precision_score and
 * precision_recall_curve.  All of them follow exactly, ties included, from four integers per sample i and class c:
 *   counts[i][c] = {gt_all, gt_pos, ge_all, ge_pos}: the samples j with s[j][c] > s[i][c], how many of those have a label != 0, and
 *                  the same for >= (i counts itself there).
 * With P positives and N negatives of a class: AUROC = sum over positives of (neg_lt + neg_eq / 2) / (P N), neg_ge = ge_all - ge_pos,
 * neg_gt = gt_all - gt_pos, neg_lt = N - neg_ge, neg_eq = neg_ge - neg_gt; average precision = sum over positives of ge_pos / ge_all / P;
 * the precision-recall curve has the points (ge_pos / P, ge_pos / ge_all), one per distinct ge_all (octcubem_amd/metrics.py finishes
 * on the host in float64).  Integer counting: deterministic, no sort, no float accumulation; O(n^2 C) comparisons.
 *   scores  f32 [n][C], rows score_stride ELEMENTS apart (>= C: a column slice of a wider buffer passes)
 *   labels  uint8 [n][C], != 0 = positive, rows label_stride elements apart (>= C)
 *   counts  int32 [n][C][4], contiguous
 * Comparisons are IEEE: -0.0 ties with 0.0, +-inf are ordinary values; a NaN compares false with everything, so the caller keeps
 * NaN out (octcubem_amd.ops.rank_counts raises).  Same code in the two builds of the library.
 * -2, before any launch: a NULL pointer, n <= 0, C <= 0, a stride below C, n above 2^31 - 1 (a count can reach n), C above 65535. */
int octmae_rank_counts(const float* scores, long long score_stride, const uint8_t* labels, long long label_stride, int* counts,
                       long long n, int C, void* stream);

/* OCTCube/engine_finetune.py:130-157 (misc_measures_multi_task): every task ranks its own subset of the samples -- those that carry
 * the shared "normal" label or the task's label -- which the reference selects by boolean indexing on the CPU before one scikit-learn
 * call per task.  Here the subset is a per-sample, per-column mask and all tasks are counted in one launch:
 *   valid   uint8 [n][C], != 0 = the sample belongs to column c's population, rows valid_stride elements apart (>= C)
 *   counts[i][c] as octmae_rank_counts, over the j with valid[j][c] != 0 only, for an i with valid[i][c] != 0; {0, 0, 0, 0} for an i
 *                outside the population (every byte of counts is written).
 * Everything else -- strides, IEEE comparisons, the caller keeping NaN out of VALID positions, the same code in the two builds -- as
 * octmae_rank_counts.  -2, before any launch: the conditions of octmae_rank_counts, a NULL valid, valid_stride below C. */
int octmae_rank_counts_masked(const float* scores, long long score_stride, const uint8_t* labels, long long label_stride,
                              const uint8_t* valid, long long valid_stride, int* counts, long long n, int C, void* stream);

/* ---- bootstrap resamples of the ranking metrics (csrc/bootstrap.hip) ----------------------------------
 * R resamples of AUROC, average precision, trapezoid AUPRC and best F1 from one sort: a resample gives every resampling unit (a
 * sample, or a patient with all its samples) a multiplicity, and each metric is a function of the weighted cumulative counts along
 * the descending score order.  The caller sorts every class column once (octcubem_amd.ops.bootstrap_rank_metrics) and passes
 *   unit_sorted int32 [C][n]   the unit of the sample at position p of class c's descending order
 *   flags       uint8 [C][n]   bit 0 label, bit 1 last position of a tie group (s[p] != s[p+1] under IEEE comparison, or p == n - 1),
 *                              bit 2 valid (the sample belongs to class c's population)
 *   mult        int32 [R][U]   how often unit u is drawn in resample r; the weight of p is valid ? mult[r][unit] : 0
 * all contiguous.  Outputs, contiguous [R][C]: p / n_neg int64 (weighted positives / negatives), u2 int64 (twice the Mann-Whitney
 * statistic, sum over tie groups of posw (2 (N - FP) + negw)), ap_sum f64 (sum of posw TP / ALL: average precision times P), auprc f64
 * (the trapezoid rule over the points (TP / P, TP / ALL), one per tie-group end, from (0, 1); ALL == 0 reads as precision 1) and max_f1
 * f64 (max of 2 p r / (p + r + 1e-8) over those points, at least 0).  A pair (r, c) with p == 0 or n_neg == 0 is undefined for the
 * caller; with p == 0 the three floats are 0.  Deterministic: integers, and float sums folded in a fixed order.
 * The caller guarantees: every multiplicity >= 0, and the weights of a column sum to less than 2^31 (largest cluster x largest row sum
 * of mult); the running sums are 32-bit.  A unit id outside [0, U) weighs 0 (no read outside mult).  Same code in the two builds.
 * -2, before any launch: a NULL pointer, n <= 0, C <= 0, R <= 0, U <= 0, n or U above 2^31 - 1, C above 65535, R above 2^24 - 1 (one
 * workgroup of 256 threads per resample). */
int octmae_bootstrap_rank_metrics(const int* unit_sorted, const uint8_t* flags, const int* mult, long long* p, long long* n_neg,
                                  long long* u2, double* ap_sum, double* auprc, double* max_f1, long long n, int C, long long R,
                                  long long U, void* stream);

/* ---- bootstrap resamples of the regression metrics (csrc/bootmoments.hip) ------------------------------
 * Pearson r, R^2, explained variance, MSE and MAE of one resample are functions of eight weighted sums over the samples, and a
 * resample is a row of multiplicities: all R resamples are the product mult [R][U] x F [U][Cpad8], Cpad8 = 8 C rounded up to a
 * multiple of 16.  The caller (octcubem_amd.ops.bootstrap_moments) finishes the sums in float64 on the host.
 *
 * octmae_unit_moments fills F f64 [U][Cpad8], contiguous.  With a = (double)x - centre[0][c], b = (double)y - centre[1][c] and
 * e = (double)y - (double)x, entry 8 c + k of row u is, over the valid samples of unit u:
 *   k = 0 count, 1 sum a, 2 sum b, 3 sum a^2, 4 sum b^2, 5 sum a b, 6 sum e^2, 7 sum |e|;
 * columns 8 C .. Cpad8 - 1 are written as zero, a unit without samples gives zeros (every byte of F is written).
 *   pred, target  f32 [n][C], unit column stride, rows pred_stride / target_stride ELEMENTS apart (>= C)
 *   valid         uint8 [n][C] (!= 0: the sample counts for the column), rows valid_stride bytes apart (>= C), or NULL: all valid
 *   centre        f64 [2][C]: a shift only, any finite value is mathematically correct
 *   order         int32 [n]: the sample indices sorted stably by unit;  start int32 [U + 1]: unit u owns order[start[u] .. start[u+1])
 * Each (unit, column) is summed sequentially in ascending position, i.e. ascending sample index.  An order[] entry outside [0, n) is
 * skipped and start[] is clamped to [0, n]: nothing past an operand's edge is read.
 *
 * octmae_bootstrap_moments computes D[r][j] = sum_u (double)mult[r][u] * F[u][j], f64 [R][Cpad8] contiguous, mult int32 [R][U]
 * contiguous, on v_mfma_f64_16x16x4_f64.  Units are walked in ascending steps of 4; rows past R, units past U and columns at or past
 * 8 C enter as literal zeros (selected, not multiplied: F's pad columns are not read).  The units are split in parts of 1024, a
 * function of U alone; with more than one part each part is stored to ws (octmae_bootstrap_moments_ws(R, U, C) doubles; 0 for one
 * part, then ws may be NULL) and the parts are added in ascending order by a second launch: no floating-point atomic, the same bits
 * on every run, and row r does not depend on R or on the other rows.  The caller keeps F finite (0 * NaN is NaN).
 * Same code in the two builds.  -2, before any launch: a NULL pointer (valid excepted; ws excepted for one part), n, C, R or U <= 0,
 * n above 2^31 - 1, C above 4096, R above 2^20, U above 2^24, R * Cpad8 >= 2^32 (the product and its _ws query: one thread of the
 * second launch per element of D), a stride below C; the _ws query returns -2 for the same sizes.  It counts DOUBLES, not bytes. */
int octmae_unit_moments(const float* pred, long long pred_stride, const float* target, long long target_stride, const uint8_t* valid,
                        long long valid_stride, const double* centre, const int* order, const int* start, double* F, long long n, int C,
                        long long U, void* stream);
long long int octmae_bootstrap_moments_ws(long long R, long long U, int C);
int octmae_bootstrap_moments(const int* mult, const double* F, double* D, double* ws, long long R, long long U, int C, void* stream);

/* ---- retrieval ranks of the COEM validation (csrc/retrieval.hip) -------------------------------------
 * retinal-COEM/src/training/train_retclip.py:409-469 ranks every sample's partner among all candidates by sorting the rows of the
 * [n][m] logit matrix on the CPU.  Mean / median rank, R@k and the corrected variants need four integers per row; this entry point
 * counts them off f32-input MFMA tiles of a . b^T and stores no score.
 *   a       f32 [n][d], rows a_stride ELEMENTS apart (>= d);  b  f32 [m][d], rows b_stride elements apart (>= d)
 *   s(i, j) the f32 chain acc = 0; for k = 0 .. d-1: acc = fmaf(a[i][k], b[j][k], acc)  (what v_mfma_f32_32x32x2_f32 computes, bit
 *           for bit; symmetric in a and b);  t_i = s(i, target[i]), the same bits as the tile's value
 *   target  int32 [n], a column in [0, m); NULL: target[i] = i (needs n == m)
 *   keep    uint8 [m], != 0: the column takes part in the ranking; NULL: all
 *   row_group int32 [n], col_group int32 [m]: both NULL or both given
 *   out     int32 [n][4], contiguous:
 *             0  #{ j kept, j != target[i] : s(i, j) >  t_i }
 *             1  #{ j kept, j <  target[i] : s(i, j) == t_i }          0 + 1 = the target's place in a STABLE descending sort
 *             2  #{ j : col_group[j] == row_group[i] and s(i, j) >= 0 }   (0 without groups)
 *             3  #{ j : col_group[j] == row_group[i] }                    (0 without groups)
 * IEEE comparisons; the caller keeps non-finite features out (octcubem_amd.ops.retrieval_ranks raises).  Deterministic: integer
 * counts, combined across workgroups with integer atomics into the zeroed `out`.  Same code in the two builds of the library.
 * -2: a NULL a / b / out, n, m or d <= 0, a stride below d, m above 2^31 - 1, target == NULL with n != m, one group pointer without
 * the other (all before any launch), and a target that is no column of b or is not kept (found by a check launch whose flag is read
 * back on `stream` -- one synchronisation, only when target or keep is given; `out` is left zeroed). */
int octmae_retrieval_ranks(const float* a, long long a_stride, const float* b, long long b_stride, const int* target,
                           const uint8_t* keep, const int* row_group, const int* col_group, int* out, long long n, long long m,
                           int d, void* stream);

/* ---- top-k cross-modal retrieval (csrc/retrieval_topk.hip) -------------------------------------------
 * retinal-COEM/src/retDisease_eval/evaluate_results_test_train_visualize_all_models_top3_col_aireadi_laterality.py:186-270 forms the
 * [n][n] logits on the CPU, masks the columns of the query's own patient and takes torch.topk.  This entry point walks the tiles of
 * octmae_retrieval_ranks and keeps the k best candidates of every row on the chip; nothing of size n m is stored, in `ws` either.
 *   a, b, s(i, j), keep, row_group, col_group: as octmae_retrieval_ranks (the same bits for the same operands)
 *   candidates of row i: the columns j < m with keep[j] != 0 (keep given), col_group[j] != row_group[i] (groups given; self-exclusion
 *           without groups is arange as both) and s(i, j) not NaN; -inf and +inf are ordinary scores
 *   order   (s1, j1) before (s2, j2) iff s1 > s2 || (s1 == s2 && j1 < j2), IEEE comparisons (-0.0 ties with 0.0): a stable descending
 *           sort, the order out[i][0] + out[i][1] of octmae_retrieval_ranks implies
 *   k       1 .. 32
 *   out_idx int32 [n][k], out_score f32 [n][k], contiguous: the first k candidates of the row in that order and their scores, bit for
 *           bit; a row with c < k candidates holds idx -1, score -inf in slots c .. k-1 (emptiness is the index, never a score)
 *   ws      workspace of at least octmae_retrieval_topk_ws(n, m, k) BYTES, 8-byte aligned: the partial lists [split][n][k] of
 *           (score, index) pairs where the column tiles of a row block are split over several workgroups (small n); the query returns 0
 *           where no split happens (ws may then be NULL) and -2 for n or m <= 0, m above 2^31 - 1 or k outside 1 .. 32
 * Deterministic: the order is strict, the partial lists are merged in a fixed order by a second launch, no atomics; two launches give
 * the same bits.  The library allocates nothing and does not synchronise.  Same code in the two builds of the library.
 * -2, before any launch and with nothing written: a NULL a / b / out_idx / out_score, n, m or d <= 0, a stride below d, k outside
 * 1 .. 32, m above 2^31 - 1, more than 2^31 - 1 row blocks of 64, one group pointer without the other, ws NULL or ws_bytes below the
 * query where it is not 0.  (`long long int`: the query's value is a byte count.) */
long long int octmae_retrieval_topk_ws(long long n, long long m, int k);
int octmae_retrieval_topk(const float* a, long long a_stride, const float* b, long long b_stride, const uint8_t* keep,
                          const int* row_group, const int* col_group, int k, int* out_idx, float* out_score, void* ws,
                          long long ws_bytes, long long n, long long m, int d, void* stream);

/* ---- one step of attention rollout (csrc/rollout.hip) -------------------------------------------------
 * Abnar & Zuidema 2020: R = Ahat_L ... Ahat_1 with Ahat_l = (F_l + I) / rho_l, F_l = fuse_h softmax_j(scale q_i . k_j), rho_l[i] =
 * 1 + sum_j F_l[i, j].  The map of a start row w is w^T R, a chain of L vector-times-matrix steps; this entry point is one of them,
 *   r_out[b][j] = sum_i (r_in[b][i] / rho[b][i]) (F[b][i, j] + [i == j]),
 * with the probabilities recomputed on the tiles of octmae_retrieval_ranks; nothing of size N N is stored, in `ws` either.
 *   q, k    f32; row b N + i, head h at columns h HD .. h HD + HD - 1; rows q_stride / k_stride ELEMENTS apart (>= H HD).  The caller
 *           widens the 16-bit q | k of the packed qkv its attention consumed (exact for bfloat16 and for half)
 *   s, z, P s^h(i, j) = the f32 chain of octmae_retrieval_ranks over the head's HD columns (the same bits); z = scale * s (one
 *           rounding); lse = M + logf(sum_j expf(z - M)) with an online maximum; P = expf(z - lse)
 *   fusion  0 mean: ((P^0 + P^1) + ...) * (1.0f / H), rho = 2 by definition;  1 max, 2 min over the heads in ascending order (a NaN
 *           stays), rho summed
 *   r_in, r_out  f32 [B][N], contiguous, distinct
 *   ws      at least octmae_rollout_ws(B, N, H, fusion) BYTES, 4-byte aligned: lse [B][H][N], for max / min rho [B][N], and where the
 *           rows of a column block are split over `split` workgroups (a function of N alone, at most 64) the partial sums
 *           [split][B][N].  The query returns -2 for B, N or H <= 0, N above 2^31 - 1, fusion outside 0 .. 2, more than
 *           2^31 - 1 (b, h, block of 64 rows) triples, or a workspace above 2^31 - 1 bytes (an `int`, like octmae_clip_loss_ws_floats:
 *           3600 ViT-L volumes of 5121 tokens fit)
 * Deterministic: no atomics; the partial sums are added in ascending order by a finishing launch; two launches give the same bits
 * and r_out[b] depends neither on B nor on the other samples.  A non-finite q or k of sample b makes r_out[b] NaN.  The library
 * allocates nothing and does not synchronise.  Same code in the two builds of the library.
 * -2, before any launch and with nothing written: a NULL q / k / r_in / r_out / ws, B, N or H <= 0, HD outside 1 .. 128, a stride below
 * H HD, fusion outside 0 .. 2, N above 2^31 - 1, r_in == r_out, a size the query refuses, ws_bytes below the query. */
int octmae_rollout_ws(int B, long long N, int H, int fusion);
int octmae_rollout_step(const float* q, long long q_stride, const float* k, long long k_stride, int B, long long N, int H, int HD,
                        float scale, int fusion, const float* r_in, float* r_out, void* ws, long long ws_bytes, void* stream);

/* ---- both directions of up to three retrieval problems (csrc/retrieval_pair.hip) -----------------------
 * retinal-COEM/src/training/train_retclip_3modalities.py:561-604 (get_metrics_3modalities) ranks six directions: three [n][n] products,
 * each read by row and by column.  This entry point walks the tiles of each product once and counts both directions.
 *   pairs   P = 1 .. 3; pair p is a_p, b_p, both f32 [n][d] with rows a_p_stride / b_p_stride ELEMENTS apart (>= d); the pointers and
 *           strides of the pairs at and past P are not read (NULL / 0).  Two pairs may share an operand.
 *   s_p(i, j) the f32 chain of octmae_retrieval_ranks on a_p, b_p (the same bits);  t_p(i) = s_p(i, i), the tile's own bits
 *   out     int32 [P][2][n][2], contiguous:
 *             out[p][0][i] = { #{ j != i : s_p(i, j) > t_p(i) },  #{ j < i : s_p(i, j) == t_p(i) } }
 *             out[p][1][j] = { #{ i != j : s_p(i, j) > t_p(j) },  #{ i < j : s_p(i, j) == t_p(j) } }
 *           out[p][0] is columns 0 and 1 of octmae_retrieval_ranks(a_p, b_p) with the diagonal as target and no keep, out[p][1] those of
 *           octmae_retrieval_ranks(b_p, a_p), bit for bit: a product of two floats commutes, so the chain is the same either way.
 *   ws      workspace of at least octmae_retrieval_pair_ws(n, pairs) BYTES, 4-byte aligned: the P n diagonal scores, written by a
 *           pre-pass; the query returns -1 for n <= 0, n above 2^31 - 1 or pairs outside 1 .. 3
 * IEEE comparisons; the caller keeps non-finite features out (octcubem_amd.ops.retrieval_pair_ranks raises).  Deterministic: integer
 * counts, combined across workgroups with integer atomics into the zeroed `out`; no float crosses a workgroup but the read-only
 * diagonal.  The library allocates nothing and does not synchronise.  Same code in the two builds of the library.
 * -1, before any launch and with nothing written: pairs outside 1 .. 3, n or d <= 0, n above 2^31 - 1, a NULL out / ws, a NULL operand
 * or a stride below d among the first P pairs, ws not 4-byte aligned or ws_bytes below the query.  (`long long int`: a byte count.) */
long long int octmae_retrieval_pair_ws(long long n, int pairs);
int octmae_retrieval_pair_ranks(const float* a0, long long a0_stride, const float* b0, long long b0_stride, const float* a1,
                                long long a1_stride, const float* b1, long long b1_stride, const float* a2, long long a2_stride,
                                const float* b2, long long b2_stride, int pairs, int* out, void* ws, long long ws_bytes, long long n,
                                int d, void* stream);

/* ---- contrastive loss of the COEM training step (csrc/cliploss.hip) ---------------------------------
 * retinal-COEM/src/open_clip/loss.py:148-230 (ClipLoss) and :230-385 (ThreeModalityClipLoss) form logit_scale * a @ b.T, its transpose,
 * cross entropies of both and leave the backward to autograd: the [n][m] logits, their softmax and their gradient are stored each time.
 * These entry points walk the same product on f32 MFMA tiles (the walk of octmae_retrieval_ranks) and store none of them.
 *   a       f32 [n][d], rows a_stride ELEMENTS apart (>= d);  b  f32 [m][d], rows b_stride elements apart (>= d)
 *   s(i, j) the f32 chain acc = 0; for k = 0 .. d-1: acc = fmaf(a[i][k], b[j][k], acc), as octmae_retrieval_ranks
 *   z(i, j) = scale[0] * s(i, j), one f32 rounding; scale is a DEVICE pointer (no host synchronisation)
 *   the partner of row i is column t_i = i + offset (offset: a host integer, 0 except for local_loss on a rank > 0)
 *   wr      f32 [n] row weights;  wc  f32 [n] pair weights of the column direction, NULL = that direction is off
 *     L = sum_i wr[i] (lse_j z(i, j) - z(i, t_i))  +  sum_i wc[i] (lse_i' z(i', t_i) - z(i, t_i))
 *   n == m, offset 0, wr = wc = 1 / (2 n): the reference's ClipLoss; wc == NULL: one cross entropy of a rectangular logit block.
 * octmae_clip_loss_fwd writes lse_row f32 [n], lse_col f32 [m] (over ALL n rows, for every column; only with wc), tscore f32 [n] =
 * s(i, t_i) (the tile's own bits) and loss f32 [1].  Online maximum and sum over 64-column tiles: any finite z works, whatever its range.
 * octmae_clip_loss_bwd, with G(i, j) = wr[i] (p - [j == t_i]) + wc[j - offset] (q - [j == t_i]), p = exp(z - lse_row[i]),
 * q = exp(z - lse_col[j]) (0 for a column that is nobody's partner), writes
 *   da f32 [n][d] = gout[0] scale G b,  db f32 [m][d] = gout[0] scale G^T a  (rows da_stride / db_stride elements apart),
 *   dscale f32 [1] = gout[0] sum G o s;  gout: the upstream scalar, a DEVICE pointer.  Each of da, db, dscale may be NULL (not computed).
 * s is recomputed per tile from the saved log-sum-exps.  DETERMINISTIC: no float atomics, every output element is summed in a fixed
 * order (the loss and dscale in float64 by one workgroup), two runs are bit-equal.  A NaN or Inf feature gives a NaN loss and NaN in
 * the gradients it reaches; nothing raises or waits on the values.  exp / log: the device library's expf / logf.  No 16-bit operand,
 * no fast-math flag, no contraction: the same code in the two builds of the library.
 *   ws      f32 workspace of at least octmae_clip_loss_ws_floats(n, m) elements (the forward's per-workgroup (max, sum) partials; the
 *           backward keeps its n dscale partials there); the query returns -2 where n or m is <= 0 or the count passes 2^31 - 1.
 * -2, before any launch: a NULL a / b / scale / wr / output (lse_col only with wc) / ws, n, m or d <= 0, a stride below d,
 * offset < 0 or n + offset > m (host integers: no device read), n or m above 2^31 - 1, a workspace below the query. */
int octmae_clip_loss_ws_floats(long long n, long long m);
int octmae_clip_loss_fwd(const float* a, long long a_stride, const float* b, long long b_stride, const float* scale, const float* wr,
                         const float* wc, long long offset, float* lse_row, float* lse_col, float* tscore, float* loss, float* ws,
                         long long ws_floats, long long n, long long m, int d, void* stream);
int octmae_clip_loss_bwd(const float* a, long long a_stride, const float* b, long long b_stride, const float* scale, const float* wr,
                         const float* wc, long long offset, const float* lse_row, const float* lse_col, const float* gout, float* da,
                         long long da_stride, float* db, long long db_stride, float* dscale, float* ws, long long ws_floats, long long n,
                         long long m, int d, void* stream);

/* ---- the join in front of the COEM classification head (csrc/join.hip) --------------------------------
 * retinal-COEM/src/open_clip/model.py:741-809 (CustomTextCLIPClassification / CustomTextCLIP3ModClassification): F.normalize of each
 * tower output, zeros for an absent modality, cat, ClassificationHead.input_norm = LayerNorm(M * D).  One kernel each way.
 *   f_k     f32 [B][D], the RAW output of tower k (k < M; f2 = NULL when M == 2; an absent modality's pointer may be NULL)
 *   present_mask   bit k set: modality k takes part; a clear bit puts zeros into slot k (single_modality)
 *   n_out   f32 [M][B][D]: n_k = f_k / max(||f_k||_2, 1e-12), zeros in absent slots (the norm is taken of the slice scaled by a power
 *           of two, so rows of size 1e-20 or 1e18 neither under- nor overflow);  inv_norm f32 [B][M] = 1 / max(||f_k||, 1e-12), 0 if absent
 *   y_lp    [B][M * D] in the library's 16-bit operand type (octmae_lp_dtype) = LayerNorm(concat_k n_k; gamma, beta, eps), the
 *           statistics over all M * D columns;  mean / rstd f32 [B]
 * octmae_join_bwd: dy f32 [B][M * D] (the gradient at y), dn_extra f32 [M][B][D] or NULL (a gradient arriving at n_out from elsewhere;
 * absent slots are not read), df_out f32 [M][B][D]: the gradient at f_k through LayerNorm and normalisation in one pass -- slices of
 * absent modalities are NOT written.  A present row whose norm is below 1e-12 gets d / 1e-12 without the projection term (autograd's
 * result for F.normalize).  dgamma / dbeta f32 [M * D] are ACCUMULATED (+=) when non-NULL, through per-workgroup partials in `ws`
 * (at least octmae_join_ws_floats(B, D, M) floats; may be NULL when both are) folded in a fixed order: no float atomics, two runs are
 * bit-equal, and df_out is bit-identical with and without them.
 * Alignment: rows are moved in 16-byte pieces, so f_k, gamma, beta, n_out, dy, dn_extra, df_out and ws must be 16-byte aligned and
 * y_lp 8-byte aligned (with D % 4 == 0 every row then is); inv_norm, mean, rstd, dgamma and dbeta are accessed word by word.
 * -1, before any launch: D % 4 != 0, M not 2 or 3, M * D > 4096, B <= 0, present_mask == 0 or with a bit at or above M, a NULL
 * pointer where one is needed, a pointer that is not aligned as above (octmae_join_ws_floats returns -1 for such a shape). */
int octmae_join_ws_floats(int B, int D, int M);
int octmae_join_fwd(const float* f0, const float* f1, const float* f2, int present_mask, const float* gamma, const float* beta,
                    float* n_out, float* inv_norm, void* y_lp, float* mean, float* rstd, int B, int D, int M, float eps, void* stream);
int octmae_join_bwd(const float* dy, const float* dn_extra, const float* f0, const float* f1, const float* f2, const float* inv_norm,
                    const float* mean, const float* rstd, const float* gamma, int present_mask, float* df_out, float* dgamma,
                    float* dbeta, float* ws, int B, int D, int M, void* stream);

/* ---- slab LayerNorm: the SLIViT head's patch embedding on the spatio-temporal token stream (csrc/slabnorm.hip) ----
 * OCTCube/models_vit_st_flash_attn_slivit.py:245-257 hands x[:, 1:] viewed [N, T, L, C] and transposed to [N, T, C, L] to
 * models_slivit_head.py:37-38, whose Rearrange 'b c (h p1) (w p2) -> b (c h w) (p1 p2)' (p1 = C, p2 = L) flattens every [C, L] slice into
 * one row for vit-pytorch's to_patch_embedding: LayerNorm(C L) -> Linear(C L, dim) -> LayerNorm(dim).  These two entry points are the
 * first LayerNorm and its backward, off the token stream as it lies in memory.
 *   x       f32 [N][n_prefix + T L][C], contiguous: n_prefix leading tokens per volume (the cls token) that take no part
 *   row r = n T + t is the contiguous slab S_r = x[n][n_prefix + t L .. n_prefix + (t + 1) L)[0..C) read transposed: element
 *           k = c L + l of the row is S_r[l][c];  K = C L
 *   mean, rstd   f32 [N T]: over the K elements of the slab, biased variance, rstd = 1 / sqrt(var + eps); the variance is the sum of
 *           squared deviations from the mean (chunks of 16384 elements combined pairwise in double), so it survives a common offset
 *   a_lp    [N T][K] in the library's 16-bit operand type (octmae_lp_dtype), row-major: a_lp[r][c L + l] =
 *           lp(fmaf((S_r[l][c] - mean_r) * rstd_r, gamma[c L + l], beta[c L + l])) -- the GEMM's operand as it is
 *   gamma, beta  f32 [K] in the order of k
 * octmae_slab_norm_bwd: da_lp [N T][K] in the 16-bit operand type (what the dgrad GEMM writes); with g_k = da[r][k] gamma[k] and
 *   xh_k = (S_r[l][c] - mean_r) rstd_r:  dx's slab element [l][c] = rstd_r (g_k - mean_k(g) - xh_k mean_k(g xh)); dx f32 of x's shape,
 *   written densely: the n_prefix leading token rows of every volume are zeros.  dgamma[k] += sum_r da[r][k] xh_k and
 *   dbeta[k] += sum_r da[r][k] (f32 [K], ACCUMULATED) when the pointer is not NULL; nothing is computed for a NULL one.
 * No float atomics: every sum runs in a fixed order (per-tile and per-row-group partials in ws, folded in ascending order), two runs
 * are bit-equal, and dx is bit-identical with and without dgamma / dbeta.
 *   ws      at least octmae_slabnorm_ws_floats(N, T, L, C) floats, for either call; caller-owned, needs no initialisation
 * Alignment: x, gamma, beta, a_lp, da_lp, dx and ws 16-byte aligned; mean, rstd, dgamma, dbeta are accessed word by word.
 * -1, before any launch: C % 8 != 0 or C < 8, L < 1, T < 1, N < 1, n_prefix < 0, eps < 0, K above 2^30, N T above 2^24, a NULL pointer
 * where one is needed, a pointer that is not aligned as above (octmae_slabnorm_ws_floats returns -1 for such a shape). */
int octmae_slabnorm_ws_floats(int N, int T, int L, int C);
int octmae_slab_norm_fwd(const float* x, const float* gamma, const float* beta, void* a_lp, float* mean, float* rstd, float* ws, int N,
                         int T, int L, int C, int n_prefix, float eps, void* stream);
int octmae_slab_norm_bwd(const void* da_lp, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                         float* dgamma, float* dbeta, float* ws, int N, int T, int L, int C, int n_prefix, void* stream);

/* ---- ConvNeXt layer: depthwise 7x7 convolution and layer scale (csrc/convnext.hip) -------------------------
 * What HF's ConvNextLayer (transformers/models/convnext/modeling_convnext.py, reached from OCTCube/model_slivit_baseline.py:72-85) gets
 * from nn.Conv2d(C, C, 7, padding=3, groups=C), its autograd, and `residual + layer_scale_parameter * x`.
 * All tensors are channels-last fp32: x, z, dz, dx, dres [B][H][W][C] = [M = B H W][C] rows; wt f32 [C][7][7], bias f32 [C]; C % 8 == 0,
 * any H, W >= 1 (also maps smaller than the filter).  Nothing is rounded to 16 bits except dbranch_lp.
 *   octmae_dwconv7_fwd        z[b,h,w,c]  = bias[c] + sum_{i,j in 0..6} wt[c,i,j] x[b, h+i-3, w+j-3, c], zero outside the map (cross-
 *                             correlation, as nn.Conv2d computes)
 *   octmae_dwconv7_bwd_input  dx[b,h,w,c] = dres[b,h,w,c] + sum_{i,j} wt[c,i,j] dz[b, h-i+3, w-j+3, c]; dres (may be NULL) is the gradient
 *                             arriving on the residual path, added LAST: the result is (the result without dres) + dres exactly
 *   octmae_dwconv7_bwd_weight gw[c,i,j] += sum_{b,h,w} dz[b,h,w,c] x[b, h+i-3, w+j-3, c],  gb[c] += sum dz[b,h,w,c]: per-workgroup partial
 *                             sums in ws (at least octmae_dwconv7_bwd_weight_ws_floats(B, H, W, C) floats = G * 50 * C, G the number of
 *                             partials) folded in ascending order by a second launch; no float atomics, two runs are bit-equal
 *   octmae_layer_scale_fwd    out[m,c] = res[m,c] + gamma[c] * branch[m,c]: one fp32 multiply, one fp32 add (not fused)
 *   octmae_layer_scale_bwd    dbranch_lp[m,c] = gamma[c] * dout[m,c] rounded once to the 16-bit operand type (octmae_lp_dtype);
 *                             ggamma[c] += sum_m dout[m,c] * branch[m,c] when ggamma is not NULL (then branch and ws, at least
 *                             octmae_layer_scale_bwd_ws_floats(M, C) floats = G * C, are needed), folded in a fixed order as above
 * Every fp32 pointer must be 16-byte aligned (wt, gw, gb, ggamma: word accesses, 4 bytes), dbranch_lp 8-byte aligned.
 * -1, before any launch: C % 8 != 0, an empty or out-of-range shape, a NULL or misaligned pointer (the _ws_floats queries return -1). */
int octmae_dwconv7_fwd(const float* x, const float* wt, const float* bias, float* z, int B, int H, int W, int C, void* stream);
int octmae_dwconv7_bwd_input(const float* dz, const float* wt, const float* dres, float* dx, int B, int H, int W, int C, void* stream);
int octmae_dwconv7_bwd_weight_ws_floats(int B, int H, int W, int C);
int octmae_dwconv7_bwd_weight(const float* dz, const float* x, float* gw, float* gb, float* ws, int B, int H, int W, int C, void* stream);
int octmae_layer_scale_fwd(const float* res, const float* branch, const float* gamma, float* out, int M, int C, void* stream);
int octmae_layer_scale_bwd_ws_floats(int M, int C);
int octmae_layer_scale_bwd(const float* dout, const float* branch, const float* gamma, void* dbranch_lp, float* ggamma, float* ws, int M, int C,
                           void* stream);

/* ---- mixup / cutmix of a fine-tune batch (csrc/mixup.hip) ---------------------------------------------
 * timm.data.Mixup's three modes on the device, in place, in one launch; the decisions are the host's (octcubem_amd/mixup.py).
 *   x     f32 [B][S], contiguous, B even; S = C (T) H W, the box is taken over the last two dimensions (H, W) of every plane
 *   kind  int32 [B]: 0 = sample untouched (neither read nor written on its own account), 1 = mixup, 2 = cutmix
 *   lam, oml  f32 [B]: kind 1 gives x[i] = x[i] * lam[i] + x0[j] * oml[i], j = B - 1 - i, x0 the batch before the launch; each product
 *         rounded to fp32 on its own, then the sum: bit-equal to torch's mul followed by add.  oml is the host's 1 - lam.
 *   box   int32 [B][4] = yl, yh, xl, xh: kind 2 gives x[i][.., yl:yh, xl:xh] = x0[j][.., yl:yh, xl:xh]; nothing outside the box is
 *         loaded or stored for it.  A box is clamped into [0, H] x [0, W] on the device (the caller refuses one outside it).
 * Both samples of a pair are handled by the same threads, originals loaded before either store: no copy of the batch, and the two
 * may differ in kind, lam and box (timm's elem mode).  16-byte accesses where x[i] and x[j] share their phase against a 16-byte
 * line, scalar ones at the ends and otherwise; any S, W and box.  All tables are DEVICE pointers.  Same code in the two builds.
 * -1, before any launch: a NULL pointer, B odd or <= 0, S, H or W <= 0, H * W not dividing S, x not 4-byte aligned.
 * -2: S above 2^30 elements, more than 65535 pairs. */
int octmae_mix_batch(float* x, const int* kind, const float* lam, const float* oml, const int* box, int B, long long S, int H, int W,
                     void* stream);

/* ---- optimizer side --------------------------------------------------------------------------------
 * Multi-tensor tables: tensor_table = device array of {float* p, g, m, v; int64 n}; chunk_tensor/chunk_off map
 * each chunk of octmae_mt_chunk_elems() elements to (tensor, element offset).
 * get_grad_norm_ / clip_grad_norm_: custom_util/misc.py:328-336, :356-373.  AdamW: main_pretrain_oph_joint_2d512_flash_attn.py:451. */
int octmae_mt_chunk_elems(void);
int octmae_mt_sumsq(const void* tensor_table, const int* chunk_tensor, const long long* chunk_off, int nchunks, float* sumsq,
                    void* stream);
int octmae_mt_finish_norm(const float* sumsq, int ntensors, float max_norm, float* out_norm, float* out_coef, void* stream);
int octmae_mt_adamw(const void* tensor_table, const int* chunk_tensor, const long long* chunk_off, int nchunks,
                    const float* gscale, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    void* stream);
/* The same update with two optional by-products of the one pass it makes over the parameters and gradients (both may be NULL):
 *   lp_table  device array of one pointer per tensor of the table: where to write the 16-bit operand copy (octmae_lp_dtype) of the
 *             UPDATED parameter, NULL entries skipped -- replaces the per-forward cast of the whole parameter arena
 *             (the bf16 weights autocast re-derives per forward in the reference, engine_pretrain.py:110);
 *   sumsq     fp32 [ntensors], += sum of squares of the RAW gradient per tensor (before gscale): get_grad_norm_
 *             (custom_util/misc.py:356-373) without its own pass over the gradients; finish with octmae_mt_finish_norm. */
int octmae_mt_adamw_fused(const void* tensor_table, const int* chunk_tensor, const long long* chunk_off, int nchunks,
                          const float* gscale, void* const* lp_table, float* sumsq, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, void* stream);
/* octmae_mt_sumsq / octmae_mt_adamw_fused with a workspace for deterministic mode ("deterministic" above): partial = fp32 [nchunks],
 * lent for the call, need not be initialised.  Under the mode every chunk stores the sum it would have added atomically -- the bits a
 * one-chunk tensor gets today -- as partial[chunk], and a finish launch computes sumsq[t] = (...((sumsq[t] + partial[c0]) +
 * partial[c0 + 1]) ...) over the chunks of tensor t in ascending order; the chunks of a tensor must be consecutive in the table.  There a
 * call without `partial` -- the two entry points above, when a sumsq is asked for -- is refused with -1: the mode never falls back to adding
 * in finishing order.  Outside the mode `partial` is not looked at. */
int octmae_mt_sumsq_ws(const void* tensor_table, const int* chunk_tensor, const long long* chunk_off, int nchunks, float* sumsq,
                       float* partial, void* stream);
int octmae_mt_adamw_fused_ws(const void* tensor_table, const int* chunk_tensor, const long long* chunk_off, int nchunks,
                             const float* gscale, void* const* lp_table, float* sumsq, float* partial, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, void* stream);

/* ---- data-parallel exchange over RCCL (xGMI) -----------------------------------------------------------
 * What the reference gets from torch.distributed's NCCL backend on this path:
 *   init_process_group("nccl") + barrier                    Pre-training/custom_util/misc.py:283-296
 *   DistributedDataParallel: bucketed gradient mean          Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:434-439
 *   DDP's constructor broadcast of the parameters            (same wrap site)
 *   all_reduce_mean of the logged loss                       Pre-training/custom_util/misc.py:622-630
 *   open_clip's feature all-gather (+ its reduce-scatter backward)   retinal-COEM/src/open_clip/loss.py:51-63
 * One process per GPU.  Bootstrap: rank 0 calls octmae_comm_unique_id() into a HOST buffer of OCTMAE_COMM_ID_BYTES, the host
 * side hands those bytes to every rank (the launcher's key-value store: MASTER_ADDR/MASTER_PORT of torchrun), every rank calls
 * octmae_comm_init().  The handle is opaque and owns one communication stream; it is the one object this library retains
 * between calls (freed by octmae_comm_destroy).  Every *_async call enqueues ONE collective on the communication stream,
 * ordered behind everything `after_stream` (the caller's compute stream) holds at the time of the call, and returns without
 * synchronising the host; octmae_comm_wait() makes `stream` wait for every collective enqueued so far.  In-place (`buf`)
 * unless send/recv are given.  Calls may come from any host thread (autograd's worker thread reports finished gradient
 * slices); they are serialised per communicator.  Buffers are DEVICE pointers and must stay alive until a later
 * octmae_comm_wait()'s stream has passed it.
 * Return codes: as above, plus -3 = librccl not found at run time, and 10000 + ncclResult_t for an RCCL error. */
#define OCTMAE_COMM_ID_BYTES 128
enum { OCTMAE_COMM_F32 = 0, OCTMAE_COMM_BF16 = 1, OCTMAE_COMM_F64 = 2, OCTMAE_COMM_F16 = 3 /* IEEE half: the 16-bit tensors of liboctmae_f16.so */ };
enum { OCTMAE_COMM_SUM = 0, OCTMAE_COMM_AVG = 1, OCTMAE_COMM_MAX = 2 };
int octmae_comm_available(void);                       /* 1 when librccl could be loaded, 0 otherwise (never fails) */
int octmae_comm_unique_id(void* id_bytes_host);
int octmae_comm_init(void** comm_out, const void* id_bytes_host, int rank, int world, int device);
int octmae_comm_destroy(void* comm);
int octmae_comm_rank(void* comm);                      /* plain values, not status codes; -1 for a NULL handle */
int octmae_comm_world(void* comm);
int octmae_comm_allreduce_async(void* comm, void* buf, long long count, int dtype, int op, void* after_stream);
int octmae_comm_broadcast_async(void* comm, void* buf, long long count, int dtype, int root, void* after_stream);
int octmae_comm_allgather_async(void* comm, const void* send, void* recv, long long count_per_rank, int dtype,
                                void* after_stream);
int octmae_comm_reduce_scatter_async(void* comm, const void* send, void* recv, long long count_per_rank, int dtype, int op,
                                     void* after_stream);
int octmae_comm_wait(void* comm, void* stream);
/* The communication stream itself (a hipStream_t written to *stream_out), for MEASUREMENT only: the host side records timing
 * events on it around a collective (bench.py's exposed-communication fields; DDP offers the same through its logging hooks,
 * torch/nn/parallel/distributed.py `_get_ddp_logging_data`).  Nothing may be enqueued on it that a collective would wait for. */
int octmae_comm_stream(void* comm, void** stream_out);

/* ---- hardware layout probes (tests only: pin the MFMA / ds_read_b64_tr_b16 lane maps the kernels assume) */
int octmae_probe_mfma32(const void* a_frag_bf16, const void* b_frag_bf16, float* d_regs, void* stream);
int octmae_probe_trread(const void* tile_bf16_16x16, void* out_bf16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCTMAE_H_ */
