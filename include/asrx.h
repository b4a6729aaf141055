/*
 * asrx — C-ABI of the MI355X (gfx950) Speech-Transformer attention path.
 *
 * The reference (shockless/asr-transformer) has no FFI: every hot-path op is an ATen call made from the
 * Python modules in modules/Transformer/{layers,model}.py.  Each entry point below replaces the ATen
 * call sequence cited next to it; the drop-in nn.Modules in asr-transformer_amd/asrx bind these symbols
 * through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions (all entry points):
 *   - plain device pointers, element counts/strides in ELEMENTS (not bytes), int64 sizes;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); every call is asynchronous
 *     on that stream; the library never allocates, frees or synchronises (graph-capturable);
 *   - return 0 on success, a negative ASRX_ERR_* code on bad arguments or launch failure;
 *   - dtype codes: ASRX_BF16 (bfloat16 storage) or ASRX_F32.
 */
#ifndef ASRX_H
#define ASRX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASRX_OK 0
#define ASRX_ERR_ARG (-1)
#define ASRX_ERR_LAUNCH (-2)
#define ASRX_ERR_UNSUPPORTED (-3)

#define ASRX_BF16 0
#define ASRX_F32 1
#define ASRX_BITS 2   /* gate operand only: 1 bit per element, uint32 words (ld in words; see mask_out) */

/* Library version / build identification (3: dq_acc holds one slab per key block, asrx_attn_dq_acc_elems;
 * asrx_adam_spans takes bounds that are not multiples of 4.  4: asrx_beam_step and asrx_gather_rows, the device half
 * of beam-search decoding.  5: asrx_ctc_loss, asrx_ctc_workspace_elems, asrx_ctc_targets, asrx_ctc_greedy.
 * 6: joint CTC/attention beam search: asrx_ctc_prefix_init, asrx_ctc_prefix_score, asrx_ctc_prefix_advance,
 * asrx_beam_step_joint.  7: two-pass decoding: asrx_ctc_prefix_beam, asrx_hyp_tokens, asrx_seq_logprob,
 * asrx_rescore_rank.  8: forced alignment: asrx_ctc_align, asrx_ctc_align_workspace_words.  9: token error rates and
 * minimum-Bayes-risk selection: asrx_edit_distance, asrx_mbr_rank.  10: n-gram LM shallow fusion: asrx_ngram_score,
 * asrx_ngram_advance, asrx_ngram_seq_logprob.  11: SpecAugment while the spectrogram is copied: asrx_specaug.
 * 12: log-mel filterbank features and CMVN: asrx_logmel, asrx_logmel_pass, asrx_stft_power, asrx_cmvn,
 * asrx_feature_stats.  13: padded batches: asrx_length_mask turns lengths into the key-validity bytes of mask mode
 * 1).  14: label-smoothed cross-entropy over vocabularies up to 2^20, with fp32 or bf16 gradients and perplexity /
 * accuracy statistics: asrx_cross_entropy_ls, asrx_xent_workspace_elems.  15: asrx_attn_kernel_name, the kernels an
 * attention call would enqueue).  16: transcripts beyond 255 labels: asrx_ctc_loss_long, asrx_ctc_long_workspace_elems,
 * asrx_ctc_align_long, asrx_ctc_align_long_workspace_words, asrx_edit_distance_long). */
int asrx_version(void);

/* sizeof of the descriptor structs as this library was compiled (binding check: a ctypes / cgo mirror of a
 * struct must have the same size): out[0] = asrx_gemm_desc, out[1] = asrx_attn_desc, out[2] =
 * asrx_gemm_group_dev, out[3] = asrx_rowsum_group, out[4] = asrx_adam_desc.  Returns the number of entries written
 * (<= n). */
int asrx_struct_sizes(int64_t* out, int32_t n);

/* ---------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:   C[z][m][n] = epi( alpha * sum_k A(z,m,k) * B(z,n,k) )
 *   A(m,k) = a_trans ? A[k*lda + m] : A[m*lda + k]
 *   B(n,k) = b_trans ? B[k*ldb + n] : B[n*ldb + k]          (b_trans=0 is the nn.Linear weight layout)
 *   batch index z in [0, batch): element offsets (z / batch_inner)*s?_outer + (z % batch_inner)*s?_inner
 *   epi order: +bias[n] -> +rowadd[(m % rowadd_mod)*ld_rowadd + n] -> relu -> dropout(p, seed, idx =
 *              (z*M + m)*N + n) -> *gate (keep where gate[m][n] > 0) -> +resid[m][n] -> +beta*C_old -> store
 * Replaces: nn.Linear (layers.py:10-12,36,48,51; model.py:32,102) = aten::addmm/linear, the per-head
 * q@k^T and attn@v aten::bmm (layers.py:20,27), and the conv2 implicit GEMM (model.py:168-171).
 * Split-K (splitk > 1, batch == 1) needs workspace of splitk*M*N floats (reduced in fixed split order).  A split
 * covers ceil(ceil(K / 64) / splitk) * 64 reduction elements (16-deep steps for fp32 operands), so trailing splits
 * can be left without a K range (K = 576, splitk = 7: splits 5 and 6); they contribute zero.  The workspace (and
 * rowsum_ws) needs no initialisation: every element the reduction reads is written by the same call, and nothing
 * outside the first splitk*M*N (splitk*M) elements is touched.
 * ------------------------------------------------------------------------------------------------- */
typedef struct asrx_gemm_desc {
  int32_t m, n, k;
  int32_t in_dtype;             /* dtype of A and B */
  const void* a; int64_t lda; int32_t a_trans;
  const void* b; int64_t ldb; int32_t b_trans;
  void* c; int64_t ldc; int32_t c_dtype;
  int32_t batch, batch_inner;
  int64_t sa_outer, sa_inner, sb_outer, sb_inner, sc_outer, sc_inner;
  float alpha, beta;
  const float* bias;
  const float* rowadd; int64_t ld_rowadd; int32_t rowadd_mod;
  int32_t relu;
  float dropout_p; uint64_t seed;
  const void* gate; int64_t ld_gate; int32_t gate_dtype;
  const void* resid; int64_t ld_resid; int32_t resid_dtype;
  int32_t splitk; float* workspace; int64_t workspace_elems;
  int32_t tile;                 /* 0 = auto, 64 or 128 = forced square tile (bf16 path) */
  /* rowsum_a[m] += sum_k A(m,k)  (a_trans = 1 only): the bias gradient of a weight-gradient GEMM
   * dW = dY^T X is the row sum of its A operand dY^T — fused into the staging loads, no extra HBM pass.
   * With splitk > 1 the per-split partials use rowsum_ws[splitk*M]. */
  float* rowsum_a; float* rowsum_ws;
  /* mask_out (optional; bf16 C with relu only): the bits C[m][n] > 0 as stored — the ReLU/dropout mask of an
   * FFN hidden layer, read back by its data gradient as a gate_dtype = ASRX_BITS gate (1 bit instead of 2 bytes
   * per element).  Layout (also that of ASRX_BITS gates): uint32 word [m][n / 32] (row stride ld_mask words),
   * column c = n % 32 at bit 8*((c & 15) >> 2) + 4*(c >> 4) + (c & 3), i.e. byte q holds columns 4q..4q+3 and
   * 16+4q..16+4q+3.  Requires N % 32 == 0, ldc % 8 == 0, 16-B aligned C and the fast fused epilogue; else
   * ASRX_ERR_UNSUPPORTED. */
  uint32_t* mask_out; int64_t ld_mask;
  /* kernel family (tests / A-B), one of the ASRX_GEMM_* codes below — honoured where the family's preconditions
   * hold, else auto.  Every other value plans as auto too: the retired codes 2, 7, 9, 11 and 12 (9 and 11, round
   * 4's persistent ws variants, were removed in version 3) and unknown ones.  Every family is a hand-written kernel
   * of this library. */
  int32_t kernel;
} asrx_gemm_desc;

/* asrx_gemm_desc.kernel */
#define ASRX_GEMM_AUTO 0
#define ASRX_GEMM_P3 1        /* 256x128 LDS-DMA ring */
#define ASRX_GEMM_REG 3       /* register-staged tiles, 64x64 or 128x128 (asrx_gemm_desc.tile) */
#define ASRX_GEMM_RING 4      /* 64x64 LDS-DMA ring (A k-contiguous) */
#define ASRX_GEMM_RING128 5   /* 128x64 LDS-DMA ring (A k-contiguous) */
#define ASRX_GEMM_P4 6        /* 256x256 LDS-DMA ring */
#define ASRX_GEMM_WS 8        /* warp-specialised 256x128 tiles (4 MFMA waves + 4 LDS-DMA loader waves; A k-contiguous,
                               * N % 128 == 0) */
#define ASRX_GEMM_WS64 10     /* ws on 64x128 tiles (the 4096-row decoder GEMMs) */

/* asrx_gemm_grouped_xcd: common->tile */
#define ASRX_GROUP_TILE_P3 3     /* p3 LDS-DMA ring, 256x128 tiles */
#define ASRX_GROUP_TILE_P4 4     /* p4 LDS-DMA ring, 256x256 tiles */
#define ASRX_GROUP_TILE_WS 5     /* warp-specialised ws kernel, 256x128 tiles */
#define ASRX_GROUP_TILE_REG 128  /* register-staged 128x128 tiles */

int asrx_gemm(const asrx_gemm_desc* d, void* stream);

/* Grouped GEMM: `count` independent problems C_i = epi(alpha * op(A_i) op(B_i)^T) in ONE launch (no split-K),
 * the group table in DEVICE memory: entries of 64 B; group i's output tiles are numbered consecutively from
 * tile_start; tile_group[t] (device) = the group of tile t.  Layout flags, dtypes, alpha/beta come from
 * `common` (its pointers/shapes are ignored).  Supported: bf16 in, a_trans = b_trans = 1 (weight gradients
 * dW = dY^T X), 16-byte aligned operand rows (the table is not inspected on the host).
 * Replaces: the per-layer weight-gradient aten::mm + bias-gradient sum of autograd's nn.Linear backward
 * (layers.py:10-12,36,48,51; model.py:32) — issued together once the backward has produced every dY. */
typedef struct asrx_gemm_group_dev {
  const void* a; const void* b; void* c; float* rowsum_a;
  int32_t lda, ldb, ldc, m, n, k, tile_start, reserved;
} asrx_gemm_group_dev;

/* Launch with an explicit workgroup -> tile map: block_tile[b] (device, `blocks` entries, 0xFFFF = idle) names
 * the tile workgroup b computes.  Workgroup b runs on XCD b % 8, so a host that lays the tiles of one group on
 * one XCD at the same time lets them share that XCD's L2 (the operand panels of dW = dY^T X are re-read by
 * every tile of the group).  common->tile selects the tile (ASRX_GROUP_TILE_*): 3 = the p3 LDS-DMA ring, 256x128 tiles (m x n;
 * fp32 C with 16-byte aligned rows, every group's n % 4 == 0, alpha 1, beta 0 or 1), 4 = the p4 ring, 256x256
 * tiles (same conditions), 5 = the warp-specialised ws kernel, 256x128 tiles (4 MFMA waves + 4 LDS-DMA loader
 * waves, 3-stage ring; same conditions; with common->workspace set and common->workspace_elems >= 16 it is read
 * as int32 counters, ZERO on entry — [0, 8) per-XCD queues, [16, 16 + P) one per 256-row panel of the groups that
 * carry a rowsum_a (group entry `reserved` = its first panel's index, panels numbered over those groups) — and
 * common->rowsum_ws as [tiles][256] fp32 scratch: the launch runs min(blocks, 256) persistent workgroups that take
 * the slots x, x + 8, x + 16, ... of block_tile from per-XCD queues (x = b % 8; blocks % 8 == 0; an empty queue
 * takes the others' last slots), and each panel's column tiles share its row sums (the last to finish adds them in
 * column order); the counters are left non-zero: zero them before the next launch), 128 = register-staged
 * 128x128 tiles (any alignment-checked table; common->relu carries its "every C row 16-byte aligned" flag).
 * Replaces the weight/bias-gradient mm + sum of autograd for every nn.Linear (layers.py:10-12,36,48,51). */
int asrx_gemm_grouped_xcd(const asrx_gemm_desc* common, const asrx_gemm_group_dev* groups,
                          const uint16_t* tile_group, const uint16_t* block_tile, int32_t count, int32_t tiles,
                          int32_t blocks, void* stream);

/* AdamW state for asrx_gemm_grouped_xcd_adam: flat fp32 parameter / moment buffers (and the optional bf16 shadow)
 * laid out like the gradient buffer whose base is g_base — the update of gradient element g_base[i] goes to
 * p[i], m[i], v[i], p_bf16[i].  Hyper-parameters as asrx_adam (hyp: device {lr, bias_corr1, bias_corr2} or null). */
typedef struct asrx_adam_desc {
  float* p; float* m; float* v; void* p_bf16; const float* g_base; const float* hyp;
  float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale;
  int32_t decoupled, reserved;
} asrx_adam_desc;

/* asrx_gemm_grouped_xcd (tile 5, the persistent queue launch: fp32 C, beta 0, workspace counters and rowsum_ws
 * slabs) with the optimizer step fused into the epilogue: each dW element and each group's bias gradient (rowsum_a)
 * is stored and the AdamW update of its parameter applied at once, the parameter / moment / shadow bytes moving
 * while the other tiles compute (single-GPU training: the gradients need no exchange first).  Replaces the
 * optimizer.step() (train.py:35) of every nn.Linear parameter together with its gradient mm + sum. */
int asrx_gemm_grouped_xcd_adam(const asrx_gemm_desc* common, const asrx_gemm_group_dev* groups,
                               const uint16_t* tile_group, const uint16_t* block_tile, int32_t count, int32_t tiles,
                               int32_t blocks, const asrx_adam_desc* adam, void* stream);

/* Name of the kernel instantiation asrx_gemm would launch for d (as rocprofv3 lists it, without the
 * namespace/argument list), e.g. "gemm_bf16_p3_kernel<false, false, 1>".  Host-only: no launch, no GPU
 * needed.  Used by bench.py to time exactly the kernel the roofline names. */
int asrx_gemm_kernel_name(const asrx_gemm_desc* d, char* buf, int32_t len);

/* Diagnostics only (tools/, never the product path): process-wide GEMM debug flags, overriding the ASRX_GEMM_DBG
 * environment variable — 1 = skip the epilogue stores, 4 = issue each LDS-DMA stage in one block, 8 = skip the
 * operand loads (compute on stale LDS); 0 = normal.  Results are garbage while any flag is set. */
int asrx_gemm_set_debug(int32_t flags);

/* Process-wide kernel-variant switches (value 0 = back to the default; there is no environment fallback since
 * round 5).  key ASRX_TUNE_SOFTMAX_U: rows per lane group of the short-row softmax kernels (1, 2, 4; default 1);
 * key ASRX_TUNE_LN_RW: rows per wave of the LayerNorm forward (1, 2, 4; default 2).  Every variant computes the same
 * values; the switch exists so tests and tools can run each one in one process. */
#define ASRX_TUNE_SOFTMAX_U 1
#define ASRX_TUNE_LN_RW 2
#define ASRX_TUNE_LN_PF 3    /* rows in flight per wave of the d = 512 LayerNorm kernels (1, 2, 4; 8 = the general kernels) */
#define ASRX_TUNE_LN_BPC 4   /* blocks per CU of the d = 512 LayerNorm forward (1..16; 0 = default 4) */
int asrx_set_tuning(int32_t key, int32_t value);

/* ---------------------------------------------------------------------------------------------------
 * Fused multi-head attention (bf16 in/out, fp32 softmax): per (batch b, head h)
 *   S = scale * Q K^T ; masked -> -inf ; P = nan_to_num(softmax(S)) ; O = dropout(P) V
 * Tensors are token-major: row r of batch b of X starts at X + b*x_bstride + r*x_rstride; head h's dh
 * columns start at +h*dh.  lse[(b*heads+h)*lq + q] receives the log2-domain log-sum-exp (+inf for a
 * fully-masked row, whose output is 0 exactly as layers.py:25 nan_to_num gives).
 * mask_mode: 0 none (encoder self / cross, model.py:21,71);
 *            1 structured: causal (if causal) OR key invalid (kvalid[b*valid_bstride+key]==0) OR query
 *              invalid (qvalid[...]==0) — the decoder mask of model.py:108-115 without materialising it;
 *              any lk, valid_bstride >= lk and kvalid address give the same result: rows on 4-byte boundaries
 *              (kvalid % 4 == 0, valid_bstride % 4 == 0) may take the streamed kernels, which read up to 3 bytes
 *              past byte lk - 1 inside its aligned word and ignore them; other rows are read byte by byte;
 *            2 dense bytes: masked where mask[b*mask_sb + q*mask_sq + key*mask_sk] != 0 (layers.py:22-23).
 * Replaces MHAHead.forward's bmm/mul/masked_fill/softmax/nan_to_num/dropout/bmm (layers.py:20-27).
 * Supported dh: 32, 64.
 * ------------------------------------------------------------------------------------------------- */
typedef struct asrx_attn_desc {
  int32_t batch, heads, lq, lk, dh;
  const void* q; int64_t q_rstride, q_bstride;
  const void* k; int64_t k_rstride, k_bstride;
  const void* v; int64_t v_rstride, v_bstride;
  void* o; int64_t o_rstride, o_bstride;
  float* lse;
  float scale;
  int32_t mask_mode, causal;
  const uint8_t* kvalid; const uint8_t* qvalid; int64_t valid_bstride;
  const uint8_t* mask; int64_t mask_sb, mask_sq, mask_sk;
  float dropout_p; uint64_t seed;
  /* backward only */
  const void* dout; int64_t do_rstride, do_bstride;
  void* dq; int64_t dq_rstride, dq_bstride;
  void* dk; int64_t dk_rstride, dk_bstride;
  void* dv; int64_t dv_rstride, dv_bstride;
  float* delta;                 /* [batch*heads*lq] workspace */
  float* dq_acc;                /* optional fp32 workspace of asrx_attn_dq_acc_elems() floats (version >= 3:
                                 * ceil(lk/128)*batch*lq*heads*dh): dQ partials, one [batch*lq*heads*dh] slab per key
                                 * block of the kernel (required for lk > 256; version 2 and earlier took ONE slab, a
                                 * caller sized by that rule overflows it; the tiled fallback accumulates into the
                                 * first slab) */
  /* optional dropout keep-bit workspace (dh = 64, dropout_p > 0, any lk): key-major words
   * [batch*heads][ceil(lq/32)][lk] (bit i = query 32c+i) followed by query-major words
   * [batch*heads][lq][qmaj_stride(lk)] (bit j = key 32c+j), where qmaj_stride(lk) = ceil(lk/32) for lk <= 256 and
   * ceil(lk/32) rounded up to a multiple of 4 for lk > 256 (the streamed kernels move 4 words per query and
   * 128-key chunk).  Total size: batch*heads*(ceil(lq/32)*lk + lq*qmaj_stride(lk)) 32-bit words — the value
   * asrx_attn_dropmask_words() returns; size the buffer from it.  Generated by the forward (or
   * asrx_attn_dropgen) and read by the backward instead of re-hashing.  The bits equal the counter-based RNG's
   * decisions, so results do not depend on it; without it the forward uses the tiled kernel. */
  uint32_t* dropmask;
  int32_t dropmask_ready;       /* nonzero: the forward finds the bits already generated (asrx_attn_dropgen) */
  /* optional (training): bf16 buffer with o's strides; the forward writes the rounding residual O - bf16(O)
   * there and the backward forms delta = rowsum(dO * (O + residual)), i.e. sum_key P dP to fp32 accuracy.
   * (With the d_model^-1/2 scale the softmax rows are flat and dS = P (dP - delta) is a small difference: the
   * bf16 rounding of O alone perturbs dQ by delta's error times the mean key.) */
  void* o_lo;
} asrx_attn_desc;

int asrx_attention_fwd(const asrx_attn_desc* d, void* stream);
/* Number of 32-bit words of the dropmask workspace for these shapes (see asrx_attn_desc.dropmask); -1 on bad
 * arguments.  Host-only arithmetic, no device access. */
int64_t asrx_attn_dropmask_words(int32_t batch, int32_t heads, int32_t lq, int32_t lk);
/* Number of fp32 elements of the dq_acc workspace asrx_attention_bwd needs for these shapes (0: none needed, lk <=
 * 128; -1 on bad arguments).  Host-only arithmetic.  Size dq_acc from it (the rule changed in version 3). */
int64_t asrx_attn_dq_acc_elems(int32_t batch, int32_t heads, int32_t lq, int32_t lk, int32_t dh);
/* Fill d->dropmask with the dropout keep bits of (seed, dropout_p, shapes) — both layouts (see dropmask).  Only
 * the shape/dropout fields of d are read; independent of the Q/K/V data, so it can run ahead on another stream. */
int asrx_attn_dropgen(const asrx_attn_desc* d, void* stream);
/* asrx_layernorm_fwd (x fp32 [rows][512], y bf16) and asrx_attn_dropgen(d) in ONE launch (their block types share
 * the CUs: the VALU-bound hashing runs in the HBM-bound LayerNorm's memory waits).  Replaces the pre-attention
 * nn.LayerNorm (model.py:20,66) and the keep-bit draw of the attention dropout (layers.py:26). */
int asrx_layernorm_fwd_attn_dropgen(const float* x, void* y, const float* gamma, const float* beta, float* mean,
                                    float* rstd, int64_t rows, int32_t d_model, float eps, const asrx_attn_desc* d,
                                    void* stream);
int asrx_attention_bwd(const asrx_attn_desc* d, void* stream);
/* The kernels asrx_attention_fwd (backward == 0) or asrx_attention_bwd would enqueue for d, in order, joined by " + ",
 * named as rocprofv3 lists them; returns the code the call itself would return. Host arithmetic only: no pointer in d is
 * dereferenced, no device is touched. */
int asrx_attn_kernel_name(const asrx_attn_desc* d, int32_t backward, char* buf, int32_t len);

/* ---------------------------------------------------------------------------------------------------
 * Row softmax over materialised scores (the unfused path; HBM-roofline kernel of BASELINE.md §3):
 *   rows = nbh*lq rows of length lk (row stride ld); row r -> (bh = r / lq, q = r % lq, b = bh / heads)
 *   p = nan_to_num(softmax(scale * s  masked -> -inf)); if pd != NULL also pd = dropout(p)
 * Replaces layers.py:20 (scale), :22-23 masked_fill, :25 softmax+nan_to_num, :26 dropout.
 * bwd: ds = p * (dpd*keep/(1-p_drop) - sum_k p*dpd*keep/(1-p_drop)) * scale
 * Outputs (p, pd, ds) get zeros in the padding columns [lk, ld) of every row but the last: whole 16-B stores, no
 * partially written HBM sectors.  Inputs' padding is ignored.
 * ------------------------------------------------------------------------------------------------- */
int asrx_softmax_fwd(int32_t dtype, const void* s, void* p, void* pd, int64_t nbh, int32_t heads, int32_t lq,
                     int32_t lk, int64_t ld, float scale, int32_t mask_mode, int32_t causal,
                     const uint8_t* kvalid, const uint8_t* qvalid, int64_t valid_bstride, const uint8_t* mask,
                     int64_t mask_sb, int64_t mask_sq, int64_t mask_sk, float dropout_p, uint64_t seed,
                     void* stream);
int asrx_softmax_bwd(int32_t dtype, const void* p, const void* dpd, void* ds, int64_t nbh, int32_t lq, int32_t lk,
                     int64_t ld, float scale, float dropout_p, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim d (nn.LayerNorm, eps, affine: model.py:14,16,33,59,61,63,101).
 * fwd: y = (x - mean) * rstd * gamma + beta; saves mean/rstd (fp32, one per row).
 * bwd: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy*gamma;  dx_out = dx + dres (dres nullable)
 *      if dx_drop != NULL also dx_drop = (drop_dtype)(dx_out * keep/(1-p))  (upstream sublayer's dropout bwd)
 *      per-block partial dgamma/dbeta go to part[nblocks][2][d]; finish with asrx_reduce_rows.
 * Any d <= 2048 and any element-aligned pointers: the vector kernels (16-B fp32 / 8-B bf16 accesses) serve the
 * calls whose tensor pointers are aligned to their access width, every other call takes the any-width kernels.
 * ------------------------------------------------------------------------------------------------- */
int asrx_layernorm_fwd(int32_t x_dtype, const void* x, int32_t y_dtype, void* y, const float* gamma,
                       const float* beta, float* mean, float* rstd, int64_t rows, int32_t d, float eps,
                       void* stream);
int asrx_layernorm_bwd(int32_t x_dtype, const void* x, int32_t dy_dtype, const void* dy, const float* gamma,
                       const float* mean, const float* rstd, const float* dres, float* dx_out, void* dx_drop,
                       int32_t drop_dtype, float dropout_p, uint64_t seed, float* part, int32_t nblocks,
                       int64_t rows, int32_t d, void* stream);

/* out[c] (+)= sum_r in[r*ld + c] for r < rows (fp32 or bf16 in, fp32 out). Deterministic two-level sum.
 * Used for bias gradients (column sums of dY) and to finish LayerNorm/conv partials. */
int asrx_reduce_rows(int32_t dtype, const void* in, int64_t rows, int32_t cols, int64_t ld, float* out,
                     int32_t accumulate, float* part, int32_t nblocks, void* stream);

/* Grouped version for many fp32 [rows][cols] matrices in ONE launch (count <= 64): out_g[c] (+)= sum_r in_g[r][c],
 * rows summed in a fixed order (deterministic).  Used for the LayerNorm dgamma|dbeta partials of a whole backward
 * pass, deferred like the weight gradients. */
typedef struct asrx_rowsum_group {
  const float* in; int64_t rows; int32_t cols; float* out; int32_t accumulate;
} asrx_rowsum_group;

int asrx_reduce_rows_grouped(const asrx_rowsum_group* groups, int32_t count, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Conv2d front-end (model.py:168-171): conv(1->64,3x3,s2)+ReLU -> conv(64->64,3x3,s2)+ReLU, no padding.
 * conv1_fwd: x (B,1,F,T) fp32 -> y1 channels-last (B,F1,T1,64) in y_dtype (bf16 or fp32); y1_mask (optional,
 *            (B,F1,T1,8) bytes): bit c of byte q = y1[..][8q + c] > 0 as stored (the ReLU gate of the backward)
 * im2col_conv2: y1 -> cols [(b,t2,f2)][(kh,kw,c)] (B*T2*F2, 576), same dtype: conv2 = GEMM(cols, W2p^T)
 * col2im_conv2: dcols -> dy1 (B,F1,T1,64) fp32, gated by y1 > 0 (ReLU backward)
 * conv1_bwd_w: dW1[c][kh*3+kw] += sum dy1*x, db1[c] += sum dy1 (partials in part[nblocks][64*10])
 * ------------------------------------------------------------------------------------------------- */
int asrx_conv1_fwd(const float* x, int32_t B, int32_t F, int32_t T, const float* w, const float* b, void* y1,
                   int32_t y_dtype, uint8_t* y1_mask, void* stream);
/* conv2 (Conv2d(64,64,3,s2) + bias + ReLU, model.py:170-171) as an implicit GEMM over the channels-last conv1
 * output y1 (B, F1, T1, 64) bf16, no im2col image: out[(b*T2 + t2)*F2 + f2][64] bf16 — the encoder input rows.
 * w2: [64][576] bf16, columns (kh, kw, c); bias fp32 [64].  y1 must be < 2 GiB (32-bit DMA offsets). */
int asrx_conv2_fwd(const void* y1, const void* w2, const float* bias, void* out, int32_t B, int32_t F1, int32_t T1,
                   void* stream);
/* conv2 weight/bias gradient (+=, fp32) without an im2col image: dw[64][576] += dy2^T im2col(y1), db[64] +=
 * colsum(dy2); dy2 [B*T2*F2][64] bf16, y1 (B, F1, T1, 64) bf16.  ws: >= splitk*64*576 floats, rws: splitk*64
 * floats (when db).  model.py:170 Conv2d backward. */
int asrx_conv2_wgrad(const void* dy2, const void* y1, int32_t B, int32_t F1, int32_t T1, float* dw, float* db,
                     float* ws, int64_t ws_elems, float* rws, int32_t splitk, void* stream);
/* conv1 weight/bias gradient (+=) straight from the conv2 output gradient: dy1 = relu'(y1) * conv2^T(dy2) is
 * formed on the fly, neither the column gradient nor dy1 is stored (model.py:168-171 backward).  dy2
 * [B*T2*F2][64] bf16 (ReLU-gated), w2 [64][576] bf16, y1_mask = conv1_fwd's sign bits, x (B,1,F,T) fp32; part:
 * [nblocks + 128][640] workspace, nblocks >= 2 persistent workgroups (about 2/3 take the even-f1 rows).
 * Accepted while T1 <= 1024 and 48 KiB + roundup16(T1*8) B + 12*T B of dynamic LDS <= 80 KiB, else
 * ASRX_ERR_UNSUPPORTED: the LDS sum binds first, T <= 2048 (T1 = 1023, exactly 80 KiB; launches above 64 KiB need no
 * attribute on gfx950).  asrx.kernels.conv_bwd_implicit_fits mirrors the rule. */
int asrx_conv_bwd_implicit(const void* dy2, const void* w2, const uint8_t* y1_mask, const float* x, int32_t B, int32_t F,
                           int32_t T, float* part, int32_t nblocks, float* dw, float* db, void* stream);
int asrx_im2col_conv2(int32_t dtype, const void* y1, int32_t B, int32_t F1, int32_t T1, void* cols, void* stream);
int asrx_col2im_conv2(int32_t dcols_dtype, const void* dcols, int32_t y1_dtype, const void* y1, int32_t B,
                      int32_t F1, int32_t T1, float* dy1, void* stream);
int asrx_conv1_bwd_w(const float* x, const float* dy1, int32_t B, int32_t F, int32_t T, float* part,
                     int32_t nblocks, float* dw, float* db, void* stream);

/* Fused conv1 backward (dW1 += sum dy1 * x-taps, db1 += sum dy1) straight from the conv2 column gradient:
 * dy1 = relu'(y1) * col2im(dcols) is formed on the fly and never stored (replaces col2im + conv1_bwd_w on the
 * training path; model.py:168-169).  nblocks = ceil(B * F1 * 8 / 4) (8 waves per conv1 output row), part:
 * [nblocks + 128][640] workspace (per-block partials, then the finish's first-pass rows). */
int asrx_conv1_bwd_fused(int32_t dcols_dtype, const void* dcols, int32_t y1_dtype, const void* y1, const float* x,
                         int32_t B, int32_t F, int32_t T, float* part, int32_t nblocks, float* dw, float* db,
                         void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Decoder embedding (model.py:94-96,117): out[t] = dropout(E[tok[t]] + pe[t % L]) (fp32 residual stream);
 * bwd: dE[v] += sum over tokens == v (v != pad_id) of dropout_bwd(dout)   (padding_idx row gets none).
 * ------------------------------------------------------------------------------------------------- */
int asrx_embed_fwd(const int64_t* tok, int64_t ntok, int32_t L, const float* table, int32_t d, const float* pe,
                   float dropout_p, uint64_t seed, float* out, void* stream);
int asrx_embed_bwd(const int64_t* tok, int64_t ntok, int32_t L, const float* dout, int32_t d, int32_t vocab,
                   int32_t pad_id, float dropout_p, uint64_t seed, float* dtable, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Cross-entropy over V classes (train.py:32, caller-supplied CE): logits fp32 rows (stride ld);
 * loss = mean over rows with target != ignore_index of (lse - logit[target]);
 * dlogits (bf16, stride ld, padded columns zeroed) = grad_scale*(softmax - onehot)/count; argmax (nullable).
 * ws: >= rows + 2 floats.
 * ------------------------------------------------------------------------------------------------- */
int asrx_cross_entropy(const float* logits, int64_t rows, int32_t V, int64_t ld, const int64_t* target,
                       int64_t ignore_index, float grad_scale, float* loss, void* dlogits, int64_t* argmax,
                       float* ws, void* stream);

/* Label-smoothed cross-entropy over any V <= 2^20 (nn.CrossEntropyLoss(ignore_index=, label_smoothing=eps), mean
 * reduction).  n = #rows with target != ignore_index; per valid row, lse = logsumexp over c < V:
 *   nll = lse - x[t],  smooth = lse - mean_{c<V} x[c],  row = (1 - eps) * nll + eps * smooth
 *   loss = sum row / n                                   (0 when n == 0)
 *   dlogits[r][c] = grad_scale / n * (softmax_c - (1 - eps) * [c == t] - eps / V)   for c < V; 0 for V <= c < ld and
 *                   in every column of an ignored row (nullable; grad_dtype ASRX_BF16 or ASRX_F32, row stride ld)
 *   argmax[r]  first index of the row maximum over c < V, ignored rows included (nullable)
 *   stats[0]   mean unsmoothed nll over the valid rows (log perplexity), stats[1] = #(valid, argmax == t) / n
 *              (nullable [2]; both 0 when n == 0)
 * The uniform mass is over the V classes, never over ld; columns [V, ld) of logits are never read.  eps > 0 assumes
 * finite logits; at eps == 0, -inf in a non-target class is a class of probability 0.  Row sums are finished in a
 * fixed order (no float atomics): the loss is bit-reproducible.  Rows of ld <= 16384 are read once; longer rows
 * twice.  16-B loads where ld % 4 == 0 and logits / dlogits are 16-B aligned, 4-B ones otherwise.
 * ws: asrx_xent_workspace_elems(rows) floats (3 rows + 4; -1 for rows < 0 and for rows beyond ASRX_XENT_MAX_ROWS, the
 * most whose count an int holds, which asrx_cross_entropy_ls refuses as well).
 * ASRX_ERR_ARG: null logits / target / loss / ws, V <= 0, ld < V, rows < 0, eps outside [0, 1), an unknown
 * grad_dtype; ASRX_ERR_UNSUPPORTED: V > 2^20 or rows > ASRX_XENT_MAX_ROWS (all before any launch).  rows == 0 writes loss 0. */
#define ASRX_XENT_MAX_ROWS 715827881
int asrx_xent_workspace_elems(int64_t rows);
int asrx_cross_entropy_ls(const float* logits, int64_t rows, int32_t V, int64_t ld, const int64_t* target,
                          int64_t ignore_index, float label_smoothing, float grad_scale, float* loss, float* stats,
                          int32_t grad_dtype, void* dlogits, int64_t* argmax, float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Elementwise utilities.
 * ------------------------------------------------------------------------------------------------- */
int asrx_cast(int32_t src_dtype, const void* src, int32_t dst_dtype, void* dst, int64_t n, void* stream);
/* out[i] (dtype_out) = op(a[i], b[i]) over n contiguous elements (any of a, b, out may alias; ASRX_F32 / ASRX_BF16):
 *   ASRX_EW_RELU_GRAD  b[i] > 0 ? a[i] : 0        ReLU backward gated by its output b (the standalone FrontEnd's
 *                                                   conv2 ReLU, model.py:170, torch.where in round 2)
 *   ASRX_EW_DROPOUT    keep(seed, i) ? a[i] / (1 - p) : 0   dropout backward with the element mask of the GEMM
 *                                                   dropout epilogues (layers.py:40, the standalone MHA's output)
 *   ASRX_EW_ADD        a[i] + b[i]                  gradient accumulation (the standalone MHA's K/V input, split
 *                                                   LayerNorm gradients) */
#define ASRX_EW_RELU_GRAD 0
#define ASRX_EW_DROPOUT 1
#define ASRX_EW_ADD 2
int asrx_ewise(int32_t op, int32_t dtype_a, const void* a, int32_t dtype_b, const void* b, int32_t dtype_out,
               void* out, int64_t n, float p, uint64_t seed, void* stream);

/* Power spectrogram of a batch of waveforms (the featuriser of modules/dataset.py:34-55:
 * torchaudio.transforms.Spectrogram(n_fft, center=False) -> |STFT|^power):
 *   audio  fp32 [batch][samples] (row stride batch_stride), frames = (samples - n_fft) / hop + 1
 *   basis  fp32 [2 nbins][n_fft]: rows 2n / 2n+1 = window[k] * cos / -sin(2 pi n k / n_fft) (the caller's window,
 *          zero-padded to n_fft as torch.stft does; see asrx.features)
 *   out    fp32 [batch][nbins][frames] = scale * (re^2 + im^2)^(power/2), power 1 or 2
 *   ws     fp32 workspace of >= batch * frames * 2 nbins elements (the DFT GEMM's output)
 * One fp32 MFMA GEMM (frames as overlapping rows of the waveform, lda = hop) plus a square/transpose pass. */
int asrx_spectrogram(const float* audio, int64_t batch, int64_t samples, int64_t batch_stride, const float* basis,
                     int32_t n_fft, int32_t hop, int32_t nbins, int32_t power, float scale, float* ws,
                     int64_t ws_elems, float* out, void* stream);

/* Greedy decode step (Decoder.evaluate, model.py:144 `prob.argmax(dim=-1)[:, -1]`): for each of `rows` logit rows
 * (fp32, row stride ld, V used columns) the first index of the maximum, stored as int64 at tok[r * tok_stride] and,
 * if cur != NULL, at cur[r] (the next step's embedding input). */
int asrx_greedy_argmax(const float* logits, int64_t rows, int32_t V, int64_t ld, int64_t* tok, int64_t tok_stride,
                       int64_t* cur, void* stream);

/* One beam-search decode step for B samples x W beams (Decoder.beam_search; the reference decodes greedily only,
 * model.py:125-151): the per-sample top-W over the W x V continuation scores, one launch, no host round trip.
 *   logits    fp32, B*W rows (sample b, beam w at row b*W + w), row stride ld >= V; only columns [0, V) are read
 *   score_in  fp32 [B*W] running log-probabilities, fin_in uint8 [B*W] finished flags, len_in int32 [B*W] lengths
 * Candidates of sample b: a live beam w offers every v < V at score_in[w] + logits[w][v] - logsumexp(logits[w][:V])
 * (max-subtracted, fp32); a finished beam offers exactly (w, eos) at score_in[w].  A NaN score reads as -inf.  The W
 * best by descending score, ties by ascending flat index w*V + v (the first-index rule of asrx_greedy_argmax, which
 * W = 1 reduces to), go to slots b*W + j, j = 0 the best; -inf candidates are legal and rank last in index order.
 * Per slot: score_out, tok_out (int64; also cur[slot] if cur != NULL, the next step's embedding input), parent_out
 * (int32 in [0, W)), src_row_out = b*W + parent (the asrx_gather_rows index), fin_out = fin_in[parent] | (tok ==
 * eos), len_out = len_in[parent] + (fin_in[parent] ? 0 : 1).  n_live (optional, device int32): the number of
 * unfinished slots over the whole batch is ADDED to it (integer atomics, deterministic), so it must hold 0 before
 * the call.  Outputs must not alias inputs (the caller ping-pongs two state sets).
 * 1 <= W <= 16, 0 <= eos < V, any ld; V above 2^20 returns ASRX_ERR_UNSUPPORTED.  One workgroup per sample; the
 * candidates are held in LDS while W*V <= 16128, else formed again from the logits in every round. */
int asrx_beam_step(const float* logits, int32_t B, int32_t W, int32_t V, int64_t ld, const float* score_in,
                   const uint8_t* fin_in, const int32_t* len_in, int64_t eos, float* score_out, int64_t* tok_out,
                   int64_t* cur, int32_t* parent_out, int32_t* src_row_out, uint8_t* fin_out, int32_t* len_out,
                   int32_t* n_live, void* stream);
/* Row gather, the beam reorder of the K/V caches: dst[o][r][0:count) = src[o][index[r]][0:count) for o < outer,
 * r < rows; both buffers share one layout (row_stride >= count and outer_stride in elements of esize = 2 or 4
 * bytes), index = device int32 row numbers in [0, rows) (a row with any other index is left untouched).  Elements
 * of dst beyond count in a row are not written.  16-byte accesses when both bases, the strides and count allow it,
 * element accesses otherwise.  src and dst must not overlap (ASRX_ERR_ARG): the caller double-buffers.  One launch
 * covers every decoder layer: outer = layers, rows = B*W, count = the filled prefix of a cache row. */
int asrx_gather_rows(const void* src, void* dst, const int32_t* index, int32_t esize, int32_t outer, int32_t rows,
                     int64_t count, int64_t row_stride, int64_t outer_stride, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * CTC (version >= 5): the second term of the hybrid objective (1 - w) * CE + w * CTC on a linear head over the encoder
 * output.  The reference trains on cross-entropy alone (train.py:32); the user-side alternative these replace is
 * log_softmax + F.ctc_loss + autograd.
 * ------------------------------------------------------------------------------------------------- */
#define ASRX_CTC_SUM 0    /* loss = sum_b nll_b,                              per-sample weight w_b = 1 */
#define ASRX_CTC_MEAN 1   /* loss = mean_b(nll_b / max(target_len_b, 1)),     w_b = 1 / (B * max(target_len_b, 1)) */

/* Number of fp32 workspace elements asrx_ctc_loss needs (row statistics, per-sample tables, and log2 alpha / beta of
 * every (b, t) row: 128 * ceil((max_target_len + 1) / 64) values each); -1 on bad arguments (B, T <= 0,
 * max_target_len outside [0, 255]).  Host-only arithmetic, no device access. */
int64_t asrx_ctc_workspace_elems(int32_t B, int32_t T, int32_t max_target_len);

/* CTC negative log-likelihood and its gradient with respect to the LOGITS (the log-softmax is fused; no
 * log-probability tensor exists).  F.ctc_loss(F.log_softmax(logits, -1).transpose(0, 1), targets, input_lengths,
 * target_lengths, blank, reduction, zero_infinity) and its backward.
 *   logits          fp32, row b*T + t at logits + (b*T + t)*ld, ld >= V; only columns [0, V) are read
 *   targets         int64 [B][tgt_stride]; sample b's labels are its first target_lengths[b] entries
 *   input_lengths   device int32 [B], nullable (null = T for every sample); clamped to [0, T]
 *   target_lengths  device int32 [B]
 *   max_target_len  host-side bound of every target length, 0 <= max_target_len <= tgt_stride.  The lengths live on
 *                   the device, so this is what the host checks: above 255 (511 extended states) the call returns
 *                   ASRX_ERR_UNSUPPORTED before any device access.  It sizes the workspace and picks the kernel (each
 *                   lane of a wave64 holds ceil((max_target_len + 1) / 64) <= 4 blank/label state pairs).
 *   blank           0 <= blank < V, else ASRX_ERR_ARG (before any device access)
 *   nll[B]          fp32 per sample; +inf where no alignment exists.  That is also the result of a sample the host
 *                   cannot see to be malformed: a length outside [0, max_target_len], a label equal to blank or
 *                   outside [0, V).  Such a label is never used as an index.
 *   loss[1]         loss_add_scale * loss_add[0] + loss_scale * sum_b w_b nll_b  (loss_add nullable: the first term is
 *                   dropped).  With zero_infinity, +inf terms count as 0.  Summed over b in a fixed order.
 *                   The training step takes (1 - w) * CE + w * CTC from the finishing launch this way (a factor on
 *                   both terms), with no torch arithmetic in the captured step.
 *   dlogits         nullable; ASRX_BF16 or ASRX_F32 [B*T][ld]: grad_scale * w_b * (softmax - occupancy) in columns
 *                   [0, V), zero in [V, ld) and in the rows t >= input_length_b.  grad_scale does not scale loss.  The
 *                   rows of a sample without alignment are zero with zero_infinity and NaN without (as torch's).
 *   ws              asrx_ctc_workspace_elems(B, T, max_target_len) floats, 16-B aligned; contents undefined after
 * Deterministic: no floating-point atomics; the occupancy of a label that occurs several times in a target is summed
 * in order of position, the batch in order of b — two calls on the same inputs give the same bits.  Four launches, no
 * synchronisation, graph-capturable.  16-B accesses where ld % 4 == 0 and the bases are aligned, element accesses
 * otherwise.  ld <= 8192, B <= 65535. */
int asrx_ctc_loss(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                  int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                  int32_t max_target_len, int32_t blank, int32_t reduction, int32_t zero_infinity, float grad_scale,
                  float* nll, float* loss, void* dlogits, int32_t dlogits_dtype, const float* loss_add,
                  float loss_add_scale, float loss_scale, float* ws, int64_t ws_elems, void* stream);

/* CTC beyond 255 labels (version >= 16): asrx_ctc_loss for 0 <= max_target_len <= ASRX_CTC_LONG_MAX_TARGET.  Same
 * parameter list, semantics, reductions, outputs and argument checks (in the same order, before any device access) as
 * asrx_ctc_loss; only the bound differs: max_target_len > 4095 returns ASRX_ERR_UNSUPPORTED and the size helper -1.
 * One workgroup of NW = ceil((max_target_len + 1) / 256) wave64s per (sample, direction), lane i of the workgroup
 * owning the (blank, label) pairs 4i .. 4i + 3; the neighbour value crosses a wave seam through LDS slots
 * double-buffered by frame parity, one workgroup barrier per frame.  The workspace holds the row statistics, 4100 ints
 * per sample (rank | count << 16 per label, the lengths), and log2 alpha / beta rows of 512 * NW floats.
 * asrx_ctc_long_workspace_elems writes that number of fp32 elements to *elems and returns ASRX_OK; on bad arguments
 * (B, T <= 0, max_target_len outside [0, 4095], a NULL elems) it returns -1 (ASRX_ERR_ARG) and writes -1.  The count is
 * an int64 (more than 2^31 elements at B 64, T 4000, L 4095), hence the pointer: the result type stays every entry's
 * int.  Host-only arithmetic.  The short range is accepted too (NW = 1); results agree with asrx_ctc_loss within
 * rounding, not in bits.  Deterministic, no atomics, no allocation, no synchronisation, four launches,
 * graph-capturable.  ld <= 8192, B <= 65535. */
#define ASRX_CTC_LONG_MAX_TARGET 4095
int asrx_ctc_long_workspace_elems(int32_t B, int32_t T, int32_t max_target_len, int64_t* elems);
int asrx_ctc_loss_long(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                       int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                       int32_t max_target_len, int32_t blank, int32_t reduction, int32_t zero_infinity,
                       float grad_scale, float* nll, float* loss, void* dlogits, int32_t dlogits_dtype,
                       const float* loss_add, float loss_add_scale, float loss_scale, float* ws, int64_t ws_elems,
                       void* stream);

/* CTC targets of a teacher-forced batch: text int64 [B][n] (row stride ld_text; n = L + 1 columns of the step's token
 * rows) and the float pad mask [B][n] (row stride ld_mask).  Per sample, in order, the tokens at positions with
 * mask >= 1 that are none of drop[0 .. ndrop) (HOST array, ndrop <= 4: BOS, EOS, PAD / blank) go left-packed to
 * targets[b][0 ..], the rest of the n columns are filled with `blank`; target_lengths[b] (int32) = the count.  One
 * launch (cf. asrx_step_tokens). */
int asrx_ctc_targets(const int64_t* text, int64_t ld_text, const float* mask, int64_t ld_mask, int32_t B, int32_t n,
                     const int64_t* drop, int32_t ndrop, int64_t blank, int64_t* targets, int64_t ld_targets,
                     int32_t* target_lengths, void* stream);

/* CTC best-path decoding: per sample the first-index arg-max (asrx_greedy_argmax's tie rule) of every frame
 * t < input_lengths[b] (nullable: T) over columns [0, V) of logits row b*T + t (fp32, row stride ld), repeated frames
 * collapsed, blanks removed: tok[b][0 .. len[b]) (int64 [B][T], the rest = blank), len int32 [B].  One launch, no
 * host round trip.  T <= 15360. */
int asrx_ctc_greedy(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int32_t* input_lengths,
                    int32_t blank, int64_t* tok, int32_t* len, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Joint CTC/attention beam search (version >= 6; Watanabe et al. 2017): every hypothesis is ranked by
 * (1 - lambda) * log p_att(h) + lambda * log p_ctc(h...), the second term the CTC PREFIX probability psi of the
 * generated labels under the CTC head.  Per decode step: asrx_ctc_prefix_score (all W x V continuations, a reduction
 * over the frames), asrx_beam_step_joint (selection), asrx_ctc_prefix_advance (the forward state of the W survivors).
 * Prefix state of slot b*W + w, two sets that the caller ping-pongs like the beam state:
 *   state   fp32 [B*W][T][2], 8-B aligned: (log2(gn_t + gb_t), log2 gb_t), gn_t / gb_t = the probability of all paths
 *           over frames 0..t that collapse to the slot's labels and end in a non-blank / in the blank; -inf at t >= T_b
 *   logpsi  fp32 [B*W]: log2 psi of the slot's labels (0 for the empty prefix)
 *   last    int32 [B*W]: the last label, -1 for the empty prefix
 * Everything is fp32 in the log2 domain, every log-sum-exp max-subtracted, no floating-point atomics (the same inputs
 * give the same bits), no allocation or synchronisation, graph-capturable.  1 <= W <= 16, T >= 1, 0 <= blank < V and
 * (score / advance) 0 <= eos < V, eos != blank, else ASRX_ERR_ARG before any device access.
 * ------------------------------------------------------------------------------------------------- */

/* Once per utterance batch (two launches).  logits: the CTC head's fp32 rows b*T + t, row stride ld >= V, columns
 * [0, V) read; input_lengths: device int32 [B], nullable (T), clamped to [0, T].  Writes logp [B*T][V] = log2 softmax
 * of every row, frames [B] = T_b, and the empty prefix's state, logpsi = 0 and last = -1 for all B*W slots. */
int asrx_ctc_prefix_init(const float* logits, int32_t B, int32_t W, int32_t T, int32_t V, int64_t ld,
                         const int32_t* input_lengths, int32_t blank, float* logp, int32_t* frames, float* state,
                         float* logpsi, int32_t* last, void* stream);

/* Once per step (one launch): delta[b*W + w][c] (fp32, NATURAL log, row stride ld_delta >= V, columns >= V untouched)
 * = log psi(g.c) - log psi(g) for an ordinary label c of slot g; the eos column holds the end score
 * log(gn_{T_b-1}(g) + gb_{T_b-1}(g)) - log psi(g); the blank column holds -inf.  A slot whose psi is 0 gives -inf
 * everywhere (never NaN).  T_b = 0: -inf for every label, 0 at eos for the empty prefix.  Summed along a finished
 * hypothesis the terms telescope to its CTC log-likelihood. */
int asrx_ctc_prefix_score(const float* logp, const int32_t* frames, int32_t B, int32_t W, int32_t T, int32_t V,
                          int32_t blank, int32_t eos, const float* state, const float* logpsi, const int32_t* last,
                          float* delta, int64_t ld_delta, void* stream);

/* Once per step after the selection (one launch, one wave per slot): slot j of sample b extends slot parent[j] (int32
 * in [0, W), asrx_beam_step*'s parent_out) by tok[j] (int64, tok_out).  If the parent had finished (fin_prev [B*W]:
 * the selection's fin_in) or the token is eos, the parent's state, logpsi and last are copied; otherwise the state of
 * the extended prefix is built over t < T_b.  The parent gather happens here: *_out must not overlap *_in. */
int asrx_ctc_prefix_advance(const float* logp, const int32_t* frames, int32_t B, int32_t W, int32_t T, int32_t V,
                            int32_t blank, int32_t eos, const int32_t* parent, const int64_t* tok,
                            const uint8_t* fin_prev, const float* state_in, const float* logpsi_in,
                            const int32_t* last_in, float* state_out, float* logpsi_out, int32_t* last_out,
                            void* stream);

/* asrx_beam_step with a second score per candidate: a live beam w offers v at
 * score_in[w] + att_weight * (logits[w][v] - logsumexp(logits[w][:V])) + extra_weight * extra[w][v] (two fused
 * multiply-adds, fp32; extra fp32 [B*W][ld_extra >= V], columns [0, V) read; NaN reads as -inf).  A finished beam
 * still offers exactly (w, eos) at score_in[w]; order, outputs, limits and the LDS / re-read paths are those of
 * asrx_beam_step, which att_weight = 1, extra_weight = 0 over a zero matrix reproduces bit for bit.  The operand is
 * generic: the CTC prefix scores, a language model's (asrx_ngram_score, version 10), or both fused by that launch. */
int asrx_beam_step_joint(const float* logits, int32_t B, int32_t W, int32_t V, int64_t ld, const float* extra,
                         int64_t ld_extra, float att_weight, float extra_weight, const float* score_in,
                         const uint8_t* fin_in, const int32_t* len_in, int64_t eos, float* score_out, int64_t* tok_out,
                         int64_t* cur, int32_t* parent_out, int32_t* src_row_out, uint8_t* fin_out, int32_t* len_out,
                         int32_t* n_live, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Two-pass decoding (version >= 7; "attention rescoring"): CTC prefix beam search over the encoder frames yields W
 * complete hypotheses per utterance without the decoder, ONE teacher-forced decoder forward over all B*W of them
 * gives each its attention log-probability, and they are re-ranked by att_weight * log p_att + ctc_weight * log p_ctc.
 * ------------------------------------------------------------------------------------------------- */
/* The whole first pass in one launch, one workgroup per utterance.  logits as for asrx_ctc_greedy (fp32 rows b*T + t,
 * row stride ld >= V, columns [0, V) read; input_lengths device int32 [B], nullable, clamped to [0, T]).  Prefix
 * beam search over the full vocabulary (no per-frame token pruning) with W in 1..16 hypotheses of at most
 * max_labels >= 1 labels: a
 * hypothesis g carries (pb, pnb), the log-probability of the paths so far that collapse to g and end in the blank /
 * in a non-blank; per frame its stay (with the mass of its parent's extension, if the parent is in the beam) and its
 * extensions by every non-blank column compete, and the W best by log(pb + pnb) survive under asrx_beam_step's total
 * order (score descending, flat index w*V + c ascending, NaN read as -inf; -inf is never selected, so fewer than W
 * may live).  A prefix is known by a 64-bit hash of its label string (a prefix that is pruned and selected again
 * later is the same prefix to its children that stayed; two different strings of one beam collide with probability
 * about 2^-64 per pair).  One departure from the order above: two DIFFERENT logits of a frame whose candidate scores
 * round to the same fp32 value are taken larger logit first, not lower column first (equal logits: lower column
 * first), so among equal scores at the boundary the survivor may differ from the flat-index rule's.
 * fp32, every frame renormalised by its best score with the offset kept in a double; deterministic.
 * Outputs per slot b*W + j in final rank order, dead slots last: tok int64 [B*W][max_labels] (the rest = blank),
 * len int32, score fp32 = log(pb + pnb) after the last frame in natural-log units (dead: len 0, score -inf), n_hyp
 * int32 [B] = the live count.  No frames (T_b = 0): one hypothesis, the empty prefix, score 0.
 * ws: device workspace of ws_words >= B * T * (6 * W + 1) 4-byte words, 4-byte aligned (per frame the row's
 * logsumexp and its 2W best columns, and the trie of the selected extensions that the final phase walks back).
 * ASRX_ERR_ARG for W outside 1..16, T <= 0, blank outside [0, V), max_labels < 1, before any device access. */
int asrx_ctc_prefix_beam(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld,
                         const int32_t* input_lengths, int32_t blank, int32_t W, int32_t max_labels, void* ws,
                         int64_t ws_words, int64_t* tok, int32_t* len, float* score, int32_t* n_hyp, void* stream);
/* Decoder-ready rows of width L from the first pass (tok row stride ld_tok; n = min(len, L - 1)): dec_in = bos, the n
 * labels, pad...; dec_tgt = the n labels, eos, ignore...; mask (float) = 1 over the first n + 1 positions.  A dead
 * slot (j >= n_hyp[b]; n_hyp nullable) is all pad / all ignore with mask 0.  One launch. */
int asrx_hyp_tokens(const int64_t* tok, int64_t ld_tok, const int32_t* len, const int32_t* n_hyp, int32_t B, int32_t W,
                    int32_t L, int64_t bos, int64_t eos, int64_t pad, int64_t ignore, int64_t* dec_in,
                    int64_t* dec_tgt, float* mask, void* stream);
/* out[n] = sum over positions i, in order, of logits[n*L + i][tgt[n][i]] - logsumexp(logits[n*L + i][0 .. V)) where
 * tgt[n][i] != ignore (fp32 rows of stride ld; a target outside [0, V) is skipped too).  With n_hyp (int32
 * [N / W], nullable) sequence n = b*W + j is dead for j >= n_hyp[b]: out = -inf, its rows are not read. */
int asrx_seq_logprob(const float* logits, int32_t N, int32_t L, int32_t V, int64_t ld, const int64_t* tgt,
                     int64_t ignore, const int32_t* n_hyp, int32_t W, float* out, void* stream);
/* score[b*W + j] = att_weight * att + ctc_weight * ctc (-inf where either term is -inf or the sum is NaN) and
 * order[b][r] (int32 [B][W]) = the slot of rank r under the total order above (score descending, slot ascending). */
int asrx_rescore_rank(const float* att, const float* ctc, int32_t B, int32_t W, float att_weight, float ctc_weight,
                      float* score, int32_t* order, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Forced alignment (version >= 8): the best CTC path through the frames that collapses to a given transcript, and
 * from it per-frame positions, per-token frame spans and confidences.
 * ------------------------------------------------------------------------------------------------- */
/* 4-byte words of workspace asrx_ctc_align needs: 2 * B * T (every row's logsumexp, the path's states), and for
 * T > 1008, where the backpointers no longer fit in LDS, 32 * B * T more.  Host-only arithmetic; -1 on bad arguments
 * (B <= 0, T <= 0, max_target_len outside [0, 255]). */
int64_t asrx_ctc_align_workspace_words(int32_t B, int32_t T, int32_t max_target_len);
/* Inputs and limits are asrx_ctc_loss's: fp32 logits rows b*T + t of stride ld >= V (the log-softmax is fused:
 * lp[t][c] = logits[t][c] - logsumexp(logits[t][0 .. V))), targets int64 [B][tgt_stride >= max_target_len],
 * input_lengths nullable and clamped to [0, T], target_lengths int32 [B]; max_target_len > 255 returns
 * ASRX_ERR_UNSUPPORTED, blank outside [0, V), T <= 0 or B <= 0 ASRX_ERR_ARG, all before any device access.
 * Over the extended states s in [0, 2L] (even: blank, odd 2u + 1: label u):
 *   a[0][0] = lp[0][blank], a[0][1] = lp[0][y_0], -inf elsewhere,
 *   a[t][s] = lp[t][ext_s] + max(a[t-1][s], a[t-1][s-1], a[t-1][s-2]), s - 2 only for an odd s with ext_s != ext_{s-2};
 * ties: the skip s - 2 only if strictly greater than both others, else s - 1 only if strictly greater than the stay;
 * the path ends in state 2L only if a[T_b-1][2L] > a[T_b-1][2L-1] (L = 0: state 0) and is the backtrace from there.
 * Outputs (all of every one written by every call; Lmax = max_target_len):
 *   frame_pos   int32 [B][T]     target position u emitted at frame t < T_b, -1 for the blank and for t >= T_b
 *   frame_logp  fp32  [B][T]     lp[t][emitted symbol], 0 for t >= T_b
 *   tok_start / tok_end  int32 [B][Lmax]   first frame and one past the last frame of label u's run; -1 for u >= L_b
 *   tok_conf    fp32  [B][Lmax]  exp(mean of frame_logp over the run), summed in frame order; 0 for u >= L_b
 *   score       fp32  [B]        the path's log-probability (natural log)
 * No alignment (T_b < L_b + the number of adjacent equal labels; a target length outside [0, max_target_len]; a label
 * that is the blank or outside [0, V), which is never used as an index; no path of finite score): score = -inf,
 * frame_pos all -1, frame_logp all 0, the token outputs -1 / -1 / 0.  L_b = 0 with T_b = 0: the empty alignment,
 * score 0.  One wave64 per sample after a row-parallel logsumexp launch; the states are renormalised every four
 * frames with the offset kept in a double; backpointers (3 bits per (blank, label) pair and frame) in LDS while
 * T <= 1008, in ws above.  ws: asrx_ctc_align_workspace_words() 4-byte words, 4-byte aligned, contents undefined
 * after the call.  No host round trip, no allocation, graph-capturable, deterministic. */
int asrx_ctc_align(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                   int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                   int32_t max_target_len, int32_t blank, void* ws, int64_t ws_words, int32_t* frame_pos,
                   float* frame_logp, int32_t* tok_start, int32_t* tok_end, float* tok_conf, float* score,
                   void* stream);

/* Forced alignment beyond 255 labels (version >= 16): asrx_ctc_align for 0 <= max_target_len <=
 * ASRX_CTC_LONG_MAX_TARGET, with the same parameter list, outputs, tie rule, "no alignment" conventions and argument
 * checks; max_target_len > 4095 returns ASRX_ERR_UNSUPPORTED and the size helper -1.  One workgroup of NW =
 * ceil((max_target_len + 1) / 256) wave64s per sample (the layout of asrx_ctc_loss_long); the renormalising maximum is
 * a workgroup maximum; the backpointers, one 16-bit word per lane and frame, [frame][64 * NW], always live in the
 * workspace: asrx_ctc_align_long_workspace_words writes 2 * B * T + 32 * NW * B * T (4-byte words, an int64) to *words
 * by asrx_ctc_long_workspace_elems's convention.  The backtrace is a plain dependent walk over the backpointer words.
 * Deterministic, no allocation, no synchronisation, two launches. */
int asrx_ctc_align_long_workspace_words(int32_t B, int32_t T, int32_t max_target_len, int64_t* words);
int asrx_ctc_align_long(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                        int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                        int32_t max_target_len, int32_t blank, void* ws, int64_t ws_words, int32_t* frame_pos,
                        float* frame_logp, int32_t* tok_start, int32_t* tok_end, float* tok_conf, float* score,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Edit distance and minimum-Bayes-risk ranking (version >= 9): how many errors a decoder's output holds against a
 * transcript, and which hypothesis of an n-best list has the smallest expected distance to the others.
 * ------------------------------------------------------------------------------------------------- */
#define ASRX_ED_PAIRS 0   /* pair n = hyp row n against ref row n */
#define ASRX_ED_GROUP 1   /* pair n = hyp row n against ref row n / W: B * W hypotheses against B references */
#define ASRX_ED_CROSS 2   /* N = G * W * W, pair (g, i, j) = hyp row g * W + i against hyp row g * W + j; ref unused */
/* Levenshtein alignment of N pairs of token rows.  A row is int64 [cols] of row stride ld >= cols with an optional
 * int32 length (NULL: cols; clamped to [0, cols]); its SEQUENCE is its first `len` entries, cut before the first one
 * equal to stop_id (stop_id < 0: no stop), without every entry equal to one of drop[0 .. ndrop) (a HOST array,
 * ndrop <= 4, as in asrx_ctc_targets).  That covers `text` rows (BOS, labels, EOS, PAD...), beam-search rows (prompt,
 * tokens, EOS fill) and CTC rows (labels, blank fill).  Tokens are only compared, never used as an index.  In CROSS
 * mode both rows are hyp rows (hyp_cols, ld_hyp, hyp_len) and ref / ld_ref / ref_cols / ref_len are ignored.
 * n_hyp (GROUP and CROSS; nullable, int32 [N / W] and [N / W^2]): slots j >= n_hyp[g] of group g are absent.
 * Minimised is the pair (edits, substitutions) lexicographically: among the alignments with the fewest edits one
 * with the fewest substitutions, i.e. the most exact matches.  That is an optimum, not a backtrace rule, so any
 * two implementations agree exactly: hyp (a, b) against ref (b, c) is 2 edits = 0 sub + 1 del + 1 ins, not 2 sub.
 * A deletion is a reference token without a hypothesis counterpart, an insertion a hypothesis token without a
 * reference counterpart.
 * Outputs (every element written by every call):
 *   dist    int32 [N]      edits; -1: the pair involves an absent slot; -2: a sequence of more than 255 tokens
 *   counts  int32 [N][4]   (sub, del, ins, reference tokens), -1 where dist < 0; nullable
 * In CROSS mode dist is symmetric with a zero diagonal, and (i, j) and (j, i) have del and ins swapped.
 * ASRX_ERR_ARG, before any device access, for N <= 0, cols <= 0, ld < cols, ndrop outside 0..4, ndrop > 0 with a NULL
 * drop, a NULL hyp or dist, a NULL ref in PAIRS or GROUP mode, W < 1 (GROUP) or outside 1..16 (CROSS), N no multiple
 * of W (GROUP) or W * W (CROSS), an unknown mode.  One wave64 per pair, integer arithmetic only; no host round trip,
 * no allocation, graph-capturable, deterministic. */
int asrx_edit_distance(const int64_t* hyp, int64_t ld_hyp, int32_t hyp_cols, const int32_t* hyp_len,
                       const int64_t* ref, int64_t ld_ref, int32_t ref_cols, const int32_t* ref_len, int32_t N,
                       int32_t mode, int32_t W, const int32_t* n_hyp, const int64_t* drop, int32_t ndrop,
                       int64_t stop_id, int32_t* dist, int32_t* counts, void* stream);
/* asrx_edit_distance for sequences of up to ASRX_ED_LONG_MAX_TOKENS kept tokens (version >= 16): the same parameter
 * list, modes, filtering, argument checks, -1 convention and lexicographic (edits, substitutions) optimum; dist -2
 * marks a sequence of more than 4095 tokens.  The same wavefront, one pair (one wave64) per workgroup with both rows
 * and the column boundary in 80 KiB of dynamic LDS, the cost packed as edits << 13 | substitutions.  On inputs
 * asrx_edit_distance accepts, the integers are identical. */
#define ASRX_ED_LONG_MAX_TOKENS 4095
int asrx_edit_distance_long(const int64_t* hyp, int64_t ld_hyp, int32_t hyp_cols, const int32_t* hyp_len,
                            const int64_t* ref, int64_t ld_ref, int32_t ref_cols, const int32_t* ref_len, int32_t N,
                            int32_t mode, int32_t W, const int32_t* n_hyp, const int64_t* drop, int32_t ndrop,
                            int64_t stop_id, int32_t* dist, int32_t* counts, void* stream);
/* Minimum-Bayes-risk ranking of B n-best lists from their pairwise distances (asrx_edit_distance in CROSS mode):
 * dist int32 [B][W][W], score fp32 [B][W], n_hyp int32 [B] or NULL.  Slot j is live if j < n_hyp[b], its score is
 * finite and dist[b][j][j] >= 0 (an absent or unsupported hypothesis is dead).  With p_j = exp(scale * (s_j - max live
 * s)) / (sum over the live slots), risk_i = sum over the live j, ascending, of p_j * dist[b][i][j], in fp32; a dead
 * slot has risk +inf.  scale = 0 weighs the live slots equally (the medoid).
 *   risk   fp32  [B][W]
 *   order  int32 [B][W]   slots by (risk ascending, slot ascending), dead slots last: asrx_rescore_rank's convention
 * Two slots with identical dist rows get bitwise-equal risks and so stay in slot order.  1 <= W <= 16; ASRX_ERR_ARG,
 * before any device access, for W outside that, B <= 0, a negative or NaN scale, a NULL dist, score, risk or order.
 * One wave per sample, one launch; graph-capturable, deterministic. */
int asrx_mbr_rank(const int32_t* dist, const float* score, const int32_t* n_hyp, int32_t B, int32_t W, float scale,
                  float* risk, int32_t* order, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * N-gram language model on the device (version >= 10): the `extra` operand of asrx_beam_step_joint for shallow fusion
 * in beam search, and whole-sequence LM scores for two-pass rescoring.  A back-off n-gram over the model's token ids.
 * The table (host-built, device-resident, natural-log units) is a forward trie in breadth-first order:
 *   node 0 the empty context; nodes 1 .. V the unigrams, dense (token v is node 1 + v, present for every id; ids the
 *   model does not cover carry its out-of-vocabulary log-probability); higher orders level by level, so the children
 *   of a node are contiguous and sorted by ascending token.
 *   first_child int32 [n_nodes + 1]   the children of node i are the nodes [first_child[i], first_child[i + 1])
 *   token       int32 [n_nodes]
 *   logp        fp32  [n_nodes]       log p(token | the context the parent spells)
 *   backoff     fp32  [n_nodes]       log back-off weight of the context the node spells, 0 where the model has none
 *   n_nodes > V, 1 <= order <= ASRX_NGRAM_MAX_ORDER, 1 <= V <= 2^20 (above: ASRX_ERR_UNSUPPORTED)
 * Hypothesis state: ctx int32 [R][order - 1]; ctx[r][k - 1] = the node that spells the last k tokens of hypothesis r,
 * or -1 if that k-gram is not in the table.  The orders are looked up independently ("a b c" may exist without
 * "b c").  The root state is data the caller writes: ctx[r][0] = 1 + bos (-1 without a sentence-start token), the
 * rest -1.  With k* the largest k in 0 .. order - 1 such that k = 0, or ctx[r][k - 1] is valid and has a child with
 * token v:
 *   lm(v) = logp[that child] + sum over the valid j > k* of backoff[ctx[r][j - 1]]       (k* = 0: logp[1 + v])
 * the back-off weights added to logp one by one in ascending j, in fp32.
 * The host never reads the table, and the kernels are memory-safe against a malformed one: a ctx entry outside
 * [0, n_nodes) reads as -1, a child range is clamped to [0, n_nodes], a token[] value outside [0, V) is skipped and
 * never used as an index.  No workspace, allocation or synchronisation; graph-capturable; no floating-point atomics,
 * so the same inputs give the same bits.  Every count, order, V, ld, non-finite weight and null pointer is refused
 * with ASRX_ERR_ARG before any device access; B, R or N = 0 returns 0.
 * ------------------------------------------------------------------------------------------------- */
#define ASRX_NGRAM_MAX_ORDER 6
#define ASRX_NGRAM_LDS_V 8192   /* asrx_ngram_score builds rows of up to this many columns in LDS */

/* Once per step (one launch, one workgroup per slot): out[r][v] = base_weight * base[r][v] + lm_weight * lm(v) + bonus
 * for v < V (fp32 rows of stride ld_out >= V; columns [V, ld_out) are not written).  base (fp32 [R][ld_base >= V]) is
 * nullable, and a zero weight drops its term (also lm_weight = 0 the LM term), so there is no 0 * -inf.  out must not
 * overlap base.  The row is built by filling the unigram level and overwriting, order by order, the columns of each
 * existing context's children, a workgroup barrier between two orders; in LDS for V <= ASRX_NGRAM_LDS_V, else in
 * the out row itself. */
int asrx_ngram_score(const int32_t* first_child, const int32_t* token, const float* logp, const float* backoff,
                     int32_t n_nodes, int32_t order, int32_t V, const int32_t* ctx, int32_t R, const float* base,
                     int64_t ld_base, float base_weight, float lm_weight, float bonus, float* out, int64_t ld_out,
                     void* stream);
/* Once per step after the selection (one launch): slot j of sample b extends slot parent[j] by tok[j], the contract
 * of asrx_ctc_prefix_advance (parent int32 in [0, W), tok int64, fin_prev uint8 [B*W] the selection's fin_in): a
 * finished parent or tok == eos copies the parent's state; otherwise ctx_out[j][0] = 1 + tok and ctx_out[j][k - 1] =
 * the child of ctx_in[parent][k - 2] with token tok for k >= 2 (binary search over the sorted child list; -1 if there
 * is none, or for a token outside [0, V)).  W >= 1, 0 <= eos < V; ctx_out must not overlap ctx_in. */
int asrx_ngram_advance(const int32_t* first_child, const int32_t* token, const float* logp, const float* backoff,
                       int32_t n_nodes, int32_t order, int32_t V, int32_t B, int32_t W, int32_t eos,
                       const int32_t* parent, const int64_t* tok, const uint8_t* fin_prev, const int32_t* ctx_in,
                       int32_t* ctx_out, void* stream);
/* Whole sequences (one launch, one workgroup per row): tgt int64 [N][ld_tgt >= L] as for asrx_seq_logprob.
 * lm_out[n] = the sum, in position order, of log p(tgt[n][i] | bos, the earlier scored tokens) (bos = -1: no
 * sentence-start token); positions equal to `ignore` or outside [0, V) are skipped and do not enter the context.
 * out[n] = add_scale * add[n] + lm_weight * lm_out[n] + bonus * (scored positions); add (fp32 [N]) is nullable, and
 * a zero scale drops its term.  With n_hyp (int32 [N / W], nullable) row n = b*W + j is dead for j >= n_hyp[b]: -inf
 * in both outputs, its row is not read.  L <= 4096 (above: ASRX_ERR_UNSUPPORTED). */
int asrx_ngram_seq_logprob(const int32_t* first_child, const int32_t* token, const float* logp, const float* backoff,
                           int32_t n_nodes, int32_t order, int32_t V, const int64_t* tgt, int64_t ld_tgt, int32_t N,
                           int32_t L, int64_t ignore, int32_t bos, const int32_t* n_hyp, int32_t W, const float* add,
                           float add_scale, float lm_weight, float bonus, float* lm_out, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * SpecAugment while the spectrogram is copied (version >= 11): a time warp, then frequency and time masks, one launch.
 * src, dst: fp32 [B][F][T], time innermost, rows T apart, utterances src_bstride / dst_bstride elements apart
 * (>= F * T); lengths (int32 [B], nullable): valid frames, L = clamp(lengths[b], 0, T), T without it.
 * s = seed for step 0, else the seed of offset `step` (the mix asrx_set_seed_offset's readers apply; step comes by
 * value, the device-resident offset is not read).  D = 2 + 2 * (freq_masks + time_masks); draw j of utterance b is
 * h = rng_hash(s, b * D + j); U[0, n) = (uint64(h) * n) >> 32.  A draw that is not taken leaves the others' indices.
 *   warp (draws 0, 1; only if time_warp = W > 0 and L > 2W): w0 = W + U[0, L - 2W), c = w0 - W + 1 + U[0, 2W); output
 *     frame t < L reads position base + num / den: (0, t * w0, c) for t < c, else (w0, (t - c) * (L - w0), L - c);
 *     i = base + num / den and r = num % den in integers, frac = float(r) / float(den),
 *     out[f][t] = a + frac * (b - a) with a = x[f][i], b = x[f][min(i + 1, L - 1)]
 *   frequency mask j (draws 2 + 2j, 3 + 2j): w = U[0, min(freq_width, F) + 1), f0 = U[0, F - w + 1); rows
 *     [f0, f0 + w) take mask_value on frames [0, L)
 *   time mask j (draws 2 + 2 freq_masks + 2j, + 1): cap = min(time_width, (int)floorf(time_ratio * (float)L)),
 *     w = U[0, cap + 1), t0 = U[0, L - w + 1); output frames [t0, t0 + w) take mask_value in every row
 *   frames t >= L are copied bit for bit.
 * plan_out (int32 [B][4 + 2 * (freq_masks + time_masks)], nullable): L, w0, c (0, 0 without a warp), 0, the (f0, w)
 * pairs, the (t0, w) pairs.  Masked elements are not read; without a warp, 16-B aligned rows (both bases, both
 * strides and T multiples of 4 elements) move 16 B per lane.  A workgroup covers ASRX_SPECAUG_RUN frames.
 * Before any device access: a null, misaligned, equal or overlapping src / dst, F < 1, T < 1, a negative count or
 * width, a batch stride below F * T or time_ratio outside [0, 1] return ASRX_ERR_ARG; more than
 * ASRX_SPECAUG_MAX_MASKS masks of a kind, B > 65535 or F > 262140 ASRX_ERR_UNSUPPORTED; B = 0 returns 0.
 * ------------------------------------------------------------------------------------------------- */
#define ASRX_SPECAUG_MAX_MASKS 8
#define ASRX_SPECAUG_RUN 1024
int asrx_specaug(const float* src, float* dst, int32_t B, int32_t F, int32_t T, int64_t src_bstride,
                 int64_t dst_bstride, const int32_t* lengths, int32_t freq_masks, int32_t freq_width,
                 int32_t time_masks, int32_t time_width, float time_ratio, int32_t time_warp, float mask_value,
                 uint64_t seed, uint64_t step, int32_t* plan_out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Log-mel filterbank features and CMVN (version >= 12).
 *
 * asrx_logmel: waveform -> (log-)mel features, the STFT of asrx_spectrogram (same arguments, same fp32 GEMM into ws)
 * followed by ONE pass that reads ws once and stores out; the nbins-wide power spectrogram is never written.
 *   wave_lengths  int32 [batch], nullable (device): valid samples of each row; frames_b = len >= n_fft ?
 *                 (len - n_fft) / hop + 1 : 0, clamped to frames = (samples - n_fft) / hop + 1; null: frames
 *   fb            fp32 [nbins][n_mels] (device), any real matrix
 *   fb_range      int32 [n_mels][2] in HOST memory, read during the call: the half-open bin range [lo, hi) outside
 *                 which column m of fb is zero ([0, nbins) for a dense one).  The kernel sums
 *                 p[n] * fb[n][m] over n = lo .. hi - 1 in ascending order in fp32 (fused multiply-adds) and nothing
 *                 else, p[n] = scale * (re^2 + im^2)^(power / 2); lo == hi gives energy 0
 *   log_mode      0: v = e;  1: v = log_mul * logf(e + log_eps);  2: v = log_mul * logf(fmaxf(e, log_eps))
 *                 (log_mul 1 for ln, 1 / ln 10 for log10)
 *   mean, istd    fp32 [n_mels], nullable (device): v = (v - mean[m]) * istd[m]; mean alone subtracts only
 *   pad_value     every frame f >= frames_b of out, after the CMVN
 *   out           fp32 [batch][n_mels][frames], time innermost (what the front end and asrx_specaug read)
 *   frame_lengths int32 [batch], nullable (device): receives frames_b
 * Workgroups whose 32 frames all lie at or beyond frames_b load nothing.  Before any device access: a null audio,
 * basis, fb, fb_range, ws or out, a bad n_fft / hop / nbins / power, n_mels < 1, samples < n_fft, log_mode outside
 * 0..2, log_eps <= 0 with a log mode, istd without mean, a range with lo < 0, lo > hi or hi > nbins, or a ws below
 * batch * frames * 2 nbins elements return ASRX_ERR_ARG; n_mels > ASRX_LOGMEL_MAX_MELS, nbins > 65535,
 * batch > 65535 or frames > 2^31 - 1 ASRX_ERR_UNSUPPORTED; batch = 0 returns 0.
 *
 * asrx_cmvn: out[b][f][t] = (x[b][f][t] - mean) * istd over t < L_b = clamp(lengths[b], 0, T) (T without lengths),
 * pad_value on t >= L_b; x, out fp32 [B][F][T], rows T apart, utterances x_bstride / out_bstride apart (>= F * T).
 *   mean == NULL (per utterance): per (b, f) row, mean = sum / L, var = sum((x - mean)^2) / L (two passes, never
 *     E[x^2] - E[x]^2), istd = norm_var ? 1 / max(sqrt(var), eps) : 1; both sums in a fixed tree (deterministic)
 *   mean != NULL (given statistics, global CMVN): mean[f], istd[f] (1 when istd is NULL); norm_var, eps unused
 * out == x is allowed (in place, equal batch strides); any other overlap of the two extents, a null or misaligned
 * pointer, F < 1, T < 1, B < 0, a batch stride below F * T, istd without mean or eps <= 0 where it is used return
 * ASRX_ERR_ARG; B > 65535 ASRX_ERR_UNSUPPORTED; B = 0 returns 0.
 *
 * asrx_feature_stats: sum[f] += sum of x, sumsq[f] += sum of x^2 (fp64 [F] each) and count[0] += sum of L_b (int64)
 * over the valid frames of x fp32 [B][F][T]; the accumulators are the caller's (zeroed by it), not atomic: calls on
 * one accumulator set are ordered by the stream.  Fixed order, deterministic.
 * ------------------------------------------------------------------------------------------------- */
#define ASRX_LOGMEL_MAX_MELS 256
int asrx_logmel(const float* audio, int64_t batch, int64_t samples, int64_t batch_stride, const int32_t* wave_lengths,
                const float* basis, int32_t n_fft, int32_t hop, int32_t nbins, int32_t power, float scale,
                const float* fb, const int32_t* fb_range, int32_t n_mels, int32_t log_mode, float log_mul,
                float log_eps, const float* mean, const float* istd, float pad_value, float* ws, int64_t ws_elems,
                float* out, int32_t* frame_lengths, void* stream);
/* The two second passes alone, on a workspace ws ([batch][frames][2 nbins]) that a DFT GEMM has filled:
 * asrx_logmel_pass is asrx_logmel without its GEMM (same arguments, `frames` given instead of derived, same checks),
 * asrx_stft_power is asrx_spectrogram's square/transpose pass into out [batch][nbins][frames].  For callers that
 * keep an STFT of their own, and for tools/fbank_bench.py, which times the one against the other. */
int asrx_logmel_pass(const float* ws, int64_t batch, int64_t frames, const int32_t* wave_lengths, int32_t n_fft,
                     int32_t hop, int32_t nbins, int32_t power, float scale, const float* fb, const int32_t* fb_range,
                     int32_t n_mels, int32_t log_mode, float log_mul, float log_eps, const float* mean,
                     const float* istd, float pad_value, float* out, int32_t* frame_lengths, void* stream);
int asrx_stft_power(const float* ws, int64_t batch, int64_t frames, int32_t nbins, int32_t power, float scale,
                    float* out, void* stream);
int asrx_cmvn(const float* x, float* out, int32_t B, int32_t F, int32_t T, int64_t x_bstride, int64_t out_bstride,
              const int32_t* lengths, const float* mean, const float* istd, int32_t norm_var, float eps,
              float pad_value, void* stream);
int asrx_feature_stats(const float* x, int32_t B, int32_t F, int32_t T, int64_t x_bstride, const int32_t* lengths,
                       double* sum, double* sumsq, int64_t* count, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Padded batches (version >= 13): lengths -> the encoder's row counts and the per-batch key-validity
 * bytes that mask mode 1 of asrx_attention_fwd / asrx_attention_bwd / asrx_softmax_fwd takes as kvalid (qvalid NULL,
 * not causal: every query row attends to the valid keys only).  One launch, no host synchronisation, safe under
 * stream capture: a captured training step replays with new lengths.
 *
 * lengths int32 [B] (device) -> enc_lengths int32 [B] and valid uint8 [B][valid_bstride] (either may be NULL, not
 * both).
 * subsample = k >= 0: the unpadded kernel-3 stride-2 length arithmetic n -> (n - 3) / 2 + 1 (0 for n < 3) applied k
 * times (the front end is k = 2, asrx.subsampled; k = 0: lengths are rows already).  The result is clamped to [0, T];
 * valid[b*valid_bstride + t] = t < enc_lengths[b] for t < T; columns [T, valid_bstride) are not written.
 * Negative lengths give 0.  Before any HIP call: null lengths, B < 0, T <= 0, subsample outside 0..8, both outputs
 * null or valid_bstride < T return ASRX_ERR_ARG; B = 0 returns 0 with nothing launched.
 * ------------------------------------------------------------------------------------------------- */
int asrx_length_mask(const int32_t* lengths, int32_t B, int32_t T, int32_t subsample, int32_t* enc_lengths,
                     uint8_t* valid, int64_t valid_bstride, void* stream);

/* Data-parallel gradient exchange on a bf16 wire (asrx.dist.GradAllReduce, wire="bf16"; the reference trains on one
 * device, train.py:16-35, so this is the build's own DDP step): in = the W peers' bf16 copies of one chunk of c
 * elements, [world][chunk]; out[i] = bf16(sum over w of in[w][i]) with the sum in fp32 and one final rounding. */
int asrx_sum_chunks_bf16(const void* in, int32_t world, int64_t chunk, void* out, void* stream);
/* Fused Adam/AdamW over flat fp32 buffers; optionally refreshes the bf16 shadow copy of the params.
 * Replaces optimizer.step() (train.py:35).  hyp (optional, device): {lr, bias_corr1, bias_corr2} read at run
 * time instead of the scalar arguments, so a captured step (HIP graph) takes the current step's values. */
int asrx_adam(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
              float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
              int32_t decoupled, const float* hyp, void* stream);
/* AdamW (as asrx_adam) over the element ranges [spans[2i], spans[2i+1]) of the flat buffers, one workgroup per
 * range (device int64 table, nspans pairs): the parameters a fused weight-gradient launch
 * (asrx_gemm_grouped_xcd_adam) did not update.  Bounds that are multiples of 4 take the 16-B path only; since
 * version 3 any other bound is handled too (head / tail elements one at a time; version 2 skipped them). */
int asrx_adam_spans(float* p, const float* g, float* m, float* v, void* p_bf16, const int64_t* spans, int32_t nspans,
                    float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                    float bias_corr2, float grad_scale, int32_t decoupled, const float* hyp, void* stream);
/* Zero the spans [spans[2i], spans[2i+1]) (element offsets, device int64 table of nspans pairs) of an fp32 buffer
 * (16-B aligned base), one workgroup per span.  The training step zeroes the accumulating gradient regions with it
 * (optimizer.zero_grad, train.py:27, for everything a weight-gradient GEMM does not overwrite). */
int asrx_zero_spans(float* base, const int64_t* spans, int32_t nspans, void* stream);

/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (new/train.py:31, round 5): spans = device int64 table
 * [count][2] of {address of an fp32 gradient tensor, numel}; the total 2-norm over all of them, then every element
 * times min(max_norm / (norm + 1e-6), 1) (always applied, as torch does).  Deterministic: part = device workspace of
 * nparts floats (1..4096; one workgroup each, a fixed share of every tensor), out = device float[2] {norm, coef}.
 * Two launches, no host synchronisation. */
int asrx_clip_grad_norm(const int64_t* spans, int32_t count, float max_norm, float* part, int32_t nparts, float* out,
                        void* stream);
/* new/train.py:122-128 remove_after_eos on the device: for each sample i, pred[i][t] = eos_token for t >= eoses[i]
 * (pred int64 [batch][pred_len]) and logits[i][t][:] = the one-hot row of index eoses[i] for t >= eoses[i] (fp32
 * [batch][logit_len][vocab]; the reference writes the EOS *position* as the hot index, kept here). */
int asrx_remove_after_eos(int64_t* pred, int32_t batch, int32_t pred_len, float* logits, int32_t logit_len,
                          int32_t vocab, const int64_t* eoses, int64_t eos_token, void* stream);
/* Teacher-forced step inputs (train.py:22-24,32 without the index_put quirk; model.py:108-115): from the (B, L+1)
 * token rows `text` (targets) and `inp` (decoder input; = text unless shifted), row strides in elements, and the
 * float pad mask (B, L+1): dec_in[b*L+t] = inp[b][t], tgt[b*L+t] = text[b][t+1], valid[b*L+t] = mask[b][t] >= 1. */
int asrx_step_tokens(const int64_t* text, int64_t ld_text, const int64_t* inp, int64_t ld_inp, const float* mask,
                     int64_t ld_mask, int32_t B, int32_t L, int64_t* dec_in, int64_t* tgt, uint8_t* valid,
                     void* stream);
/* Row-wise fp32 ops of the post-LN model family (modules/Transformer/new/model.py, asrx.new): op 0 (ROWSCALE)
 * out[r][c] = a[r][c] * b[r] (the non_pad_mask products, new/model.py:25,28,83-89); op 1 (ROWADD) out[r][c] =
 * a[r][c] + b[r % period][c] (the positional table, new/model.py:60).  out may alias a. */
int asrx_rowwise(int32_t op, const float* a, const float* b, float* out, int64_t rows, int32_t d, int64_t period,
                 void* stream);
/* out[b][c][r] = x[b][r][c] (fp32, batch <= 65535): the encoder input's view/transpose (new/model.py:53-55). */
int asrx_transpose_last2(const float* x, int64_t batch, int32_t R, int32_t C, float* out, void* stream);
/* delta[(b*heads+h)*lq+q] = sum_d dO*O (attention backward prologue). */
int asrx_attn_delta(const asrx_attn_desc* d, void* stream);
/* y = dropout(x) with the library RNG (idx = element index); used for tests of the RNG stream. */
int asrx_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * HIP-graph support.  A captured training step replays every launch with the arguments recorded at capture.
 * ------------------------------------------------------------------------------------------------- */
/* Copy nbytes (multiple of 4) of HOST memory to dst (device, 4-byte aligned) through kernel arguments, ordered
 * on `stream`; the host buffer may be reused as soon as the call returns, and the copy is capturable (a replay
 * writes the same bytes again).  Used for grouped-launch tables and per-step scalars. */
int asrx_upload(void* dst, const void* src, int64_t nbytes, void* stream);
/* Device-resident dropout seed offset folded into the seed of every dropout-drawing kernel at its start
 * (offset 0 = seeds used as given).  Set once per training step, BEFORE the step's forward: a replayed graph
 * then draws fresh masks each step while forward and backward of one step still agree. */
int asrx_set_seed_offset(uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASRX_H */
