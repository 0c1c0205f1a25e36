/* medmoe_hip.h - C ABI of the MI355X (gfx950) MedMoE hot-path library libmedmoe_hip.so.
 *
 * The reference (shivangchopra11/MedMoE) has no native plugin interface: its boundary is Python
 * object construction via Hydra `_target_` strings.  These entry points
 * are the operator layer a maintainer binds (ctypes) underneath the
 * reference's own modules; each comment names the reference code (file:line under
 * /root/reference/src or .../components) the call replaces.
 *
 * Conventions: plain device pointers + sizes, no allocation, no host sync; every call enqueues
 * on `stream` and returns 0, or -1 bad argument, -2 unsupported shape, -3 launch error.  The one
 * piece of process-global state is medmoe_set_option (kernel-selection switches for tests and
 * measurements; the defaults are the fastest measured and the product path never changes them).  bf16 data is raw uint16 bits; "f32" is IEEE float.  All buffers are
 * caller-owned device memory; inputs are never modified unless documented (in-place residual).
 */
#ifndef MEDMOE_HIP_H
#define MEDMOE_HIP_H
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

/* F.scaled_dot_product_attention over the fused QKV buffer (multi_head_attention.py:62-78)
 * key_mask: NULL (every key valid) or uint8 [B][N], one byte per key, non-zero = valid.  Any pattern is supported, holes and whole
 * masked blocks included (tests/test_attention_gpu.py); every sequence must keep at least one valid key.  The contents of masked K / V
 * rows do not influence any output as long as they are finite, and the backward writes zeros into their dK / dV rows. */
int medmoe_attn_fwd(const void* qkv, void* out, float* lse, const unsigned char* key_mask, int B, int N, int H, int head_dim, hipStream_t stream);

/* backward of the same (dQ, dK, dV written into a [B*N,3D] buffer) */
int medmoe_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const unsigned char* key_mask, void* dqkv, float* delta, int B, int N, int H, int head_dim, hipStream_t stream);

/* ViT patch extraction in Conv2d weight order (build-defined front-end) */
int medmoe_patchify(const void* img, void* out, int B, int C, int H, int W, int patch, int in_f32, hipStream_t stream);
/* the same with a row pitch ld >= C*patch*patch for `out` (rows padded to the GEMM k-step, e.g. patch 14: 588 -> 640) */
int medmoe_patchify_ld(const void* img, void* out, int B, int C, int H, int W, int patch, int in_f32, int ld, hipStream_t stream);

/* CLS + position embedding fill (build-defined front-end) */
int medmoe_init_tokens(void* x, const float* cls, const float* pos, int B, int Nt, int D, hipStream_t stream);

/* gradient of the position / CLS embeddings */
int medmoe_pos_cls_grad(const void* dx, float* dpos, float* dcls, int B, int Nt, int D, hipStream_t stream);

/* BERT-style embedding gather + LayerNorm (text tower front-end, text_encoder.py:94) */
int medmoe_text_embed_ln(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type, const float* gamma, const float* beta, void* out, int B, int T, int D, int vocab, float eps, hipStream_t stream);

/* last-4-layer sum + word-piece segment-sum + sentence mean (text_encoder.py:32-90,97-117) */
int medmoe_text_aggregate(const void* h0, const void* h1, const void* h2, const void* h3, int n_layers, const int* seg, void* word_bf16, float* word_f32, float* sent, int B, int T, int D, hipStream_t stream);

/* bf16 MFMA GEMM C = epi(A B^T): every nn.Linear / Conv1d(k=1) forward and dgrad on the path (multi_head_attention.py:35-36,61,80; mlp.py:55-64; swin.py:18-30,40-41,62).
   epi: 0 none, 1 GELU (aux <- pre-activation), 2 ReLU, 3 x GELU'(aux), 4 x ReLU'(aux), 5 GELU (aux <- GELU'(pre-activation)), 6 x aux;
   order: alpha*acc + bias -> activation -> + residual -> x derivative factor */
int medmoe_gemm_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias, const void* residual, int ldr, void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap, const int* tiles, const int* tile_count, int max_tiles, long long strideB, long long strideBias, float alpha, int epi, int out_f32, int col_perm, hipStream_t stream);

/* medmoe_gemm_nt for grouped / row-mapped operands on the 256x256 kernel: `tiles` holds 256-row tiles (the second table
   medmoe_dispatch writes); bf16 C, alpha = 1, no col_perm.  Expert Linear layers swin.py:32-60 and the local-loss Gram gradient. */
int medmoe_gemm_nt_tiles256(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias, const void* residual, int ldr, void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap, const int* tiles, const int* tile_count, int max_tiles, long long strideB, long long strideBias, float alpha, int epi, int out_f32, int col_perm, hipStream_t stream);

/* wgrad dW += G^T X (+ bias grad), replaces autograd of the same Linear layers */
int medmoe_gemm_tn(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, float* db, int M, int Nn, int Kk, const int* x_rowmap, const int* g_rowmap, const int* row_off, int n_groups, long long strideW, long long strideDb, int nsplit, hipStream_t stream);
/* the plain wgrad (no row maps, no groups) in two stages when the shape allows (Nn, Kk multiples of 256, M % 32 == 0, M >= 4096): the
   workgroups STORE their partial 256 x 256 tiles into `scratch` (scratch_floats >= slots x 65536, slots = tiles x row ranges <= 256; owned by
   the caller, one per stream) and a second kernel sums them into dW in a fixed order - no fp32 atomics on dW (deterministic, and ~20 us
   cheaper per launch than 64 MB of memory-side atomics).  db: with scratch_floats >= slots x (65536 + 512) every partial tile also stores its
   512 column sums of G behind the tiles and the summing kernel (tn_reduce_det_kernel then) adds them to db in range order - no atomics at
   all; with a scratch between the two sizes dW is staged and db keeps its atomicAdd (counted by medmoe_nondet_launches).  256 x (65536 + 512)
   floats serve every shape.  Any other shape, or scratch below slots x 65536 / null: medmoe_gemm_tn with nsplit 16 */
int medmoe_gemm_tn_staged(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, float* db, int M, int Nn, int Kk, float* scratch, long long scratch_floats, hipStream_t stream);

/* cross entropy over rows/columns of a similarity matrix + gradient (losses.py:789-794,1017-1021,582-584) */
int medmoe_ce_strided(const float* X, float* dX, int rows, int cols, long long rs, long long cs, int label_off, float xscale, float w, int accumulate, float* loss_acc, hipStream_t stream);

/* Soft-GLoRIA head over the rows (or, with swapped strides, the columns) of a similarity matrix: positives soft > t1, negatives soft <= t2,
   per positive -log_softmax([x_pos, x_negatives])[0] / (1 + #negatives), averaged over positives, weighted by w; soft is [rows, cols] fp32
   row-major (losses.py:861-883 SoftGLORIAGlobalContrastiveLoss, :1180-1208 SoftGLORIALocalContrastiveLoss, softXEnt :796-803) */
int medmoe_soft_xent_strided(const float* X, float* dX, const float* soft, int rows, int cols, long long rs, long long cs, float xscale, float t1, float t2, float w, int accumulate, float* loss_acc, hipStream_t stream);

/* HardNegativeContrastiveLoss head (losses.py:885-927, nmax = 1) over the rows / columns of a cosine matrix: relu(hardest negative + margin -
   diagonal) summed with weight w, and its sub-gradient; the diagonal competes as its own negative (scores - 2 diag(diag), :903) */
int medmoe_hardneg_strided(const float* X, float* dX, int rows, int cols, long long rs, long long cs, float margin, float w, int accumulate, float* loss_acc, hipStream_t stream);

/* row L2 norms (losses.py:778-779) */
int medmoe_rownorm(const float* x, float* n, int rows, int D, hipStream_t stream);

/* cosine normalisation with eps clamp (losses.py:781-785) */
int medmoe_cos_scale(float* S, const float* na, const float* nb, int M, int N, float eps, hipStream_t stream);

/* backward of cos_scale */
int medmoe_cos_scale_bwd(float* dC, const float* C, const float* na, const float* nb, float* ca, float* cb, int M, int N, float eps, hipStream_t stream);

/* dst += coef[row] * src (norm-gradient term of the cosine) */
int medmoe_add_rowscaled(float* dst, const float* src, const float* coef, int rows, int D, hipStream_t stream);

/* word norms + transposed word matrix for the local loss (losses.py:690-695,985) */
int medmoe_words_prep(const void* words, float* wn, void* wT, int Bc, int T, int Tp, int D, hipStream_t stream);

/* fp32 padded -> bf16 dense copy of the local-loss context gradient */
int medmoe_unpad_cast(const float* src, void* dst, int B, int HW, int HWp, int D, hipStream_t stream);

/* GLoRIA local loss for one (image, caption) pair per workgroup, fwd / recomputing bwd (losses.py:979-1012, attention_fn :698-736) */
int medmoe_local_pair(const void* ctx, const void* words, const void* gmp, const float* wnorm, const int* cap_lens, const float* gsim, float* sim, void* dS, void* A, void* U, float* att, const void* a1_pre, const float* lse_pre, int B, int Bc, int HW, int T, int D, float temp1, float temp2, float eps, int backward, hipStream_t stream);

/* all word-region scores as one tiled GEMM with the word-softmax fused: A1 (bf16) + row log-sum-exp (losses.py:713-716) */
int medmoe_local_scores(const void* ctx, const void* words, const int* cap_lens, void* a1, float* lse, int B, int Bc, int HW, int T, int D, hipStream_t stream);

/* lean per-pair kernel on the local_scores tiles: sim + dS/A/U in one pass (losses.py:724-1012 after the word softmax) */
int medmoe_local_pair2(void* a1_io, const float* lse_pre, const void* gmp, const float* wnorm, const int* cap_lens, const float* gsim, float* sim, void* dS, void* U, float* att, int B, int Bc, int HW, int T, float temp1, float temp2, float eps, hipStream_t stream);

/* per-(image,caption)-block scaling of the local-loss gradient matrices by dL/dsim (single-pass mode) */
int medmoe_scale_blocks(void* X0, void* X1, const float* g, int B, int Bc, int HWp, int Tp, hipStream_t stream);

/* RAGGED local-loss layout: captions are grouped into length classes (<= 16, 32, ... words); class c holds its members
   side by side, 16*c columns each, so the B x B pair matrices are sum_i pad16(len_i) columns wide instead of B * Tp.
   Same math as the uniform entry points above (losses.py:690-695,713-716,724-1012), one launch per class.
   medmoe_words_prep_ragged with wT = null writes the word norms only (the transposed pair matrices take the words row-major). */
int medmoe_words_prep_ragged(const void* words, float* wn, void* wT, int Bc, int T, int Tp, int D, const int* col_of_cap, const int* tp_of_cap, long long ldw, hipStream_t stream);
int medmoe_local_scores_ragged(const void* ctx, const void* words, const int* cap_lens, void* a1, float* lse, int B, int Bc, int HW, int T, int D, const int* cap_list, int n_cap, int ntt, long long col_base, long long ldp, hipStream_t stream);
int medmoe_local_pair2_ragged(void* a1_io, const float* lse_pre, const void* gmp, const float* wnorm, const int* cap_lens, const float* gsim, float* sim, void* dS, void* U, int B, int Bc, int HW, int T, float temp1, float temp2, float eps, const int* cap_list, int n_cap, int ntt, long long col_base, long long ldp, hipStream_t stream);
int medmoe_scale_blocks_ragged(void* X0, void* X1, const float* g, int B, int Bc, int HWp, const int* cap_of_chunk, long long ld, hipStream_t stream);

/* TRANSPOSED pair matrices (element (row, image b, region hw < pw) at row * ld + b * bstride + hw, row = row_base + j * 16 ntt + t; the
   engine uses the image-major form ld = pw = 32 ceil(HW / 32), bstride = rows * pw: one (image, caption, word tile) unit is 16 x 448 contiguous bytes): the pair
   stage of the local loss with one wave per (image, caption, 16-word tile) (losses.py:979-1012 after the word softmax).
   lp: fp16 LOG2-probabilities of the word softmax (medmoe_local_scores_t); lse: [B][Bc][HWp]; gm: [B][GR][GR] bf16 Gram matrices ctx_b ctx_b^T, GR = 32 ceil(HW / 32),
   zero outside [HW][HW]; stats: [B][stat_rows][2] fp32.  dS == NULL: the forward launch (writes sim, A, stats, att of the matching pairs).
   Otherwise the backward launch over the same class: reads lp, A, stats, sim and writes dS (may be lp itself) and the Gram-matrix
   gradient's operand in either form: U = d2 * A as a matrix (U != NULL; d2 = 2 dL/dn2 per word row) and / or the row weights d2 alone,
   fp32 [B][stat_rows] (d2 != NULL: medmoe_gemm_tn_gram multiplies the A rows by them); everything scaled by gsim = dL/dsim (NULL: 1). */
int medmoe_local_pair3(const void* lp, void* dS, void* A, void* U, const float* lse, const void* gm, const float* wnorm, const int* cap_lens, const float* gsim, float* sim, float* att, float* stats, long long stat_rows, int B, int Bc, int HW, int T, float temp1, float temp2, float eps, const int* cap_list, int n_cap, int ntt, long long row_base, long long ld, long long bstride, int pw, float* d2, hipStream_t stream);
/* the backward launch of medmoe_local_pair3 that ALSO writes dwn [B][stat_rows] fp32: per (image, caption word) the coefficient of w_t in
   d loss / d w_t that comes from the word's own norm in the cosine, -dL/dcos * cos / ||w_t||^2 (losses.py:690-695, 1002); the caller sums it over
   the images.  The part of the word gradient that goes through the scores is dS^T ctx (one NT GEMM over the row-major pair matrix). */
int medmoe_local_pair3_wgrad(const void* lp, void* dS, void* A, void* U, const float* lse, const void* gm, const float* wnorm, const int* cap_lens, const float* gsim, float* sim, float* att, float* stats, long long stat_rows, int B, int Bc, int HW, int T, float temp1, float temp2, float eps, const int* cap_list, int n_cap, int ntt, long long row_base, long long ld, long long bstride, int pw, float* d2, float* dwn, hipStream_t stream);
/* the score GEMM of one caption length class with the word softmax fused (losses.py:713-716), TRANSPOSED output for medmoe_local_pair3:
   lpT[(row_base + j * 16 ntt + t) * ld + b * bstride + hw] = fp16 ((S - lse) / ln 2), lse[b][caption][hw] fp32.  HW % 4 == 0, D % 32 == 0, D >= 128. */
int medmoe_local_scores_t(const void* ctx, const void* words, const int* cap_lens, void* lpT, float* lse, int B, int Bc, int HW, int T, int D, const int* cap_list, int n_cap, int ntt, long long row_base, long long ld, long long bstride, hipStream_t stream);
/* dW[g][Nn][Kk] += G[:, g*gcol_stride + (0..Nn)]^T X[:, g*xcol_stride + (0..Kk)], g < n_groups, over ALL M rows (fp32 atomics: zero dW first).
   bf16 operands, M % 32 == 0, rows addressed with 64-bit bases (M * ld may exceed 4 GB).  The two wgrad-shaped GEMMs of the transposed
   local loss: d ctx = dS^T words (one group) and dGm_b = U_b^T A_b (one group per image).  g_chunk_w > 0: G's columns are stored in chunks of
   g_chunk_w columns, chunk j at G + j * g_chunk_stride (image-major pair matrices as one [M][B * HWp] operand). */
int medmoe_gemm_tn_cols(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk, int n_groups, long long gcol_stride, long long xcol_stride, long long strideW, int g_chunk_w, long long g_chunk_stride, hipStream_t stream);

/* weighted Gram products dW[g] += A_g^T diag(w_g) A_g over the column blocks A_g = A + g*col_stride of one [M][lda] bf16 matrix; w_g[m] =
   w[g*w_gstride + m*w_ld] fp32.  The local loss' dGm_b = sum over caption words of d2 * a a^T (backward of the weighted-context norm in
   attention_fn / cosine_similarity, losses.py:690-736) without a stored d2 * A matrix.  fp32 atomics into dW (zero it first). */
int medmoe_gemm_tn_gram(const void* A, int lda, const float* w, long long w_gstride, int w_ld, float* dW, int ldw, int M, int Nn, int n_groups, long long col_stride, long long strideW, hipStream_t stream);
/* the local similarity FORWARD ONLY (the evaluation step; losses.py:979-1012 with attention_fn :698-736), one launch per caption length class:
   sim[b][i] = log sum_{t < len_i} exp(temp2 cos(w_it, sum_p a_pt ctx_bp)) for the n_cap captions i in cap_list (16 (ntt - 1) < len <= 16 ntt),
   fp32 [B][Bc], BEFORE temp3.  ctx bf16 [B*HW][D], words bf16 [Bc][T][D], gm bf16 [B][GR][GR] Gram matrices ctx_b ctx_b^T (GR = 32 ceil(HW / 32),
   zero outside [HW][HW]), wnorm fp32 [Bc][T].  Scores, probabilities, attention and per-word sums stay in registers / LDS: sim is the only
   global store, one owner per element, no atomics (two launches give the same bits).  There is no pair matrix, hence no column base.
   Geometries of medmoe_local_pair3_supported, D % 64 == 0; anything else returns -2 before a launch. */
int medmoe_local_sim_fwd(const void* ctx, const void* words, const int* cap_lens, const void* gm, const float* wnorm, float* sim, int B, int Bc, int HW, int T, int D, float temp1, float temp2, float eps, const int* cap_list, int n_cap, int ntt, hipStream_t stream);
/* the same similarity for a LIST of (image, caption) pairs grouped by image (candidate re-ranking), one launch per caption
   length class ntt: units int32 [n_units][4] = (image b, first list entry, entry count, 0); one workgroup per unit stages image b's Gram
   fragments once and walks its entries; entry e is the pair (b, pair_cap[e]) and its similarity goes to out[pair_slot[e]].  The device
   code is medmoe_local_sim_fwd's: a pair's value equals that kernel's bit for bit.  One owner per written slot, no atomics; slots that
   no entry names are not written.  The kernel trusts its tables - validate on the host.  n_units == 0 returns 0 without a launch;
   geometries as medmoe_local_sim_fwd, anything else returns -2 before a launch. */
int medmoe_local_sim_pairs(const void* ctx, const void* words, const int* cap_lens, const void* gm, const float* wnorm, float* out, const int* units, int n_units, const int* pair_cap, const int* pair_slot, int B, int Bc, int HW, int T, int D, float temp1, float temp2, float eps, int ntt, hipStream_t stream);
/* tests: caption chunks per image of medmoe_local_sim_fwd (0 = automatic) */
int medmoe_local_sim_chunks(int n);
/* tests: caption chunks per image of medmoe_local_pair3 (0 = automatic) */
int medmoe_local_pair3_chunks(int n);
/* 1: medmoe_local_pair3 has an instantiation for (HW regions, T words) */
int medmoe_local_pair3_supported(int HW, int T);

/* word-piece segment map + caption lengths on the device (text_encoder.py:45-76 token loop; cap_lens of medmoe_module.py:221-223): seg[b,t] = word
 * index of token t or -1 (dropped), cap[b] = #words not starting with '[' + 1; is_cont / starts_bracket: one byte per vocabulary id; ids int64
 * (ids64 != 0) or int32 */
int medmoe_segment_map(const void* ids, int ids64, const unsigned char* is_cont, const unsigned char* starts_bracket, int* seg, int* cap, int B, int T, int vocab, int sep_id, hipStream_t stream);

/* trainable text tower (reference freeze_bert: false, text_encoder.py:27-30): backward of the word-piece aggregation (text_encoder.py:32-117) -
 * every selected layer's hidden state receives dH[b,t] = d_word[b, seg[b,t]] + d_sent[b] / T (kept tokens), 0 (dropped) - and of the embedding
 * front-end y = LN(word[id] + pos[t] + type[tt]): dx (fp32 [B*T, D], for the position / token-type tables), fp32 atomics into the word table's
 * gradient rows, dgamma / dbeta accumulated */
int medmoe_text_aggregate_bwd(const float* d_word, const float* d_sent, const int* seg, void* dH, int B, int T, int D, hipStream_t stream);
int medmoe_text_embed_ln_bwd(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type, const float* gamma, const void* dy, float* dx, float* dgamma, float* dbeta, float* g_word, int B, int T, int D, int vocab, float eps, hipStream_t stream);

/* Variable-length text batches (the frozen text tower on the tokens with attention mask 1 only, packed in (caption, position) order;
   reference text_encoder.py:97-117 computes all B x T positions): medmoe_text_pack builds tok_row[b*T+t] (packed row or -1),
   src_of_row[r] (= b*T+t), seq_off[B+1] and count[1] on the device (B <= 1024); the *_packed / *_rows / *_varlen entry points take them, so no
   row count ever travels to the host. */
int medmoe_text_pack(const unsigned char* mask, int* tok_row, int* src_of_row, int* seq_off, int* count, int B, int T, hipStream_t stream);
int medmoe_text_embed_ln_packed(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type, const float* gamma, const float* beta, void* out, int B, int T, int D, int vocab, float eps, const int* src_of_row, const int* count, hipStream_t stream);
int medmoe_text_aggregate_packed(const void* h0, const void* h1, const void* h2, const void* h3, int n_layers, const int* seg, const int* tok_row, void* word_bf16, float* word_f32, float* sent, int B, int T, int D, hipStream_t stream);
int medmoe_layernorm_fwd_rows(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int D, float eps, int out_f32, const int* rows_dev, hipStream_t stream);
int medmoe_attn_fwd_varlen(const void* qkv, void* out, float* lse, const int* seq_off, int B, int Nmax, int H, int head_dim, hipStream_t stream);
/* medmoe_gemm_nt (plain operands) on the first *m_dev rows (device int, <= M) */
int medmoe_gemm_nt_rows(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias, const void* residual, int ldr, void* aux, int ldaux, float alpha, int epi, int out_f32, const int* m_dev, hipStream_t stream);

/* Swin-T tower pieces (reference swin.py:119-149 = HF SwinModel, transformers modeling_swin.py):
   (shifted-)window attention on token-major qkv [B*H*W, 3C] (q | k | v, head h at columns h*32; 7x7 windows, head dim 32): the cyclic shift,
   window partition and their inverses are row arithmetic inside the kernels.  bias: [heads][64][64] fp32 = relative position bias of the
   49 x 49 token pairs, key columns >= 49 = -30000, rest 0; lse: [B*(H/7)*(W/7)*heads][64] fp32.  bwd: dqkv fully written; dbias (or NULL):
   [B*(H/7)*(W/7)*heads][64][64] fp32, dS of every (image, window, head) - its sum over images and windows is the bias gradient. */
int medmoe_win_attn_fwd(const void* qkv, const float* bias, void* out, float* lse, int B, int H, int W, int C, int heads, int shift, hipStream_t stream);
int medmoe_win_attn_bwd(const void* qkv, const float* bias, const void* dout, const float* lse, void* dqkv, float* dbias, int B, int H, int W, int C, int heads, int shift, hipStream_t stream);
/* stochastic depth: out[b] = res[b] + scale[b] * branch[b] over per_sample bf16 elements per image (res == NULL: out = scale[b] * branch[b]) */
int medmoe_drop_path(const void* branch, const void* res, const float* scale, void* out, int B, long long per_sample, hipStream_t stream);
/* SwinPatchMerging's 2x2 concat: y[b, Y, X, q*C + c] = x[b, 2Y + (q & 1), 2X + (q >> 1), c] (scatter = 0) or its transpose (scatter = 1) */
int medmoe_patch_merge(const void* src, void* dst, int B, int H, int W, int C, int scatter, hipStream_t stream);

/* image preprocessing on the device: B uint8 HWC images (device pointers src_ptrs[b], sizes src_hw[2b], src_hw[2b+1]) ->
   bilinear resize (half-pixel centres) -> x rescale -> (x - mean) / std -> bf16 [B,3,Ho,Wo].  Replaces the per-step CPU
   AutoImageProcessor call of swin.py:131.  mean3 / std3 are HOST arrays. */
int medmoe_preprocess(const void* const* src_ptrs, const int* src_hw, void* dst, int B, int Ho, int Wo, float rescale, const float* mean3, const float* std3, hipStream_t stream);
/* the reference's own filter: Pillow BICUBIC resize on uint8 (HF image processor of swin-tiny, swin.py:131), horizontal then vertical
   pass in 22-bit fixed point, then x rescale, (x - mean) / std -> bf16 [B,3,Ho,Wo].  meta[b][9] = {Hs, Ws, ksize_h, ksize_v, offsets of the
   horizontal bounds / weights and vertical bounds / weights in coef, first row of image b in tmp}; tmp: uint8 [total_src_rows][Wo][3];
   u8_out (may be NULL): the resized uint8 image [B][Ho][Wo][3] before normalisation; dst may be NULL when u8_out is not (the resize only) */
int medmoe_preprocess_bicubic(const void* const* src_ptrs, const long long* meta, const int* coef, void* tmp, void* dst, void* u8_out, int B, int Ho, int Wo, long long total_src_rows, float rescale, const float* mean3, const float* std3, hipStream_t stream);

/* train-time augmentation behind the resize above (the reference's `transformations` block, src/utils/utils.py:16-68): per-sample
   parameters drawn on the device from the Philox stream of the dropout kernels (site 0x20000000; sample sample0 + b owns the groups
   4 (sample0 + b) + {0 crop x0, y0, flip, order | 1 angle, tx, ty, scale | 2 brightness, contrast}), then crop -> flip -> nearest-neighbour
   affine about the crop's centre -> brightness / contrast in pixel space -> (x - mean) / std -> bf16 [B][3][C][C].
   params[b][16] = {m00 m01 m02 m10 m11 m12, brightness, contrast, order bit, flip bit, angle (degrees), tx, ty, scale, x0, y0}: output pixel
   (x, y) reads crop pixel (rint(m00 x + m01 y + m02), rint(m10 x + m11 y + m12)), mirrored in x when the flip bit is set, at offset
   (x0, y0) of the source; outside the crop the pixel is normalised zero.  S: the resized size, C <= S the crop's; train = 0 writes the
   centre crop and identity everything else; flip_thresh = floor(p 2^32); angle ~ U(d0, d1) degrees, tx = rint(U(-tr_x C, tr_x C)), ty
   likewise, scale ~ U(s0, s1), brightness ~ U(b0, b1), contrast ~ U(c0, c1).  apply takes any params buffer (the crop box is clamped into
   the source); mean3 / std3 are HOST arrays; dst must be 16-byte aligned.  Both are pure functions of their inputs (no atomics). */
int medmoe_augment_params(float* params, int B, long long sample0, long long seed, long long step, int S, int C, int train, unsigned flip_thresh, float d0, float d1, float tr_x, float tr_y, float s0, float s1, float b0, float b1, float c0, float c1, hipStream_t stream);
int medmoe_augment_apply(const void* src_u8, const float* params, void* dst, int B, int Hs, int Ws, int C, float rescale, const float* mean3, const float* std3, hipStream_t stream);

/* padded geometry (HWp, Tp, Gm row width) the local-loss kernels were instantiated for */
int medmoe_local_geometry(int HW, int T, int* HWp, int* Tp, int* GW);
/* 1: the LDS-tiled pair kernels exist for (HW regions, T words); 0: the generic path below (any HW, T <= 80) */
int medmoe_local_fast_path(int HW, int T);

/* generic-geometry GLoRIA local loss (losses.py:698-736, 985-1012 as grouped GEMMs + these elementwise kernels over the uniform pair
   matrices [B*HWp, Bc*Tp]): region-softmax A from the word log-probabilities; cosine / exp / log-sum per pair from wctx = A^T ctx;
   d wctx after the CE over sim; dS from dA (in place); sum of two padded fp32 gradients -> bf16 */
int medmoe_local_gen_fwd_a(const void* lp, const int* cap_lens, void* A, int B, int Bc, int HW, int HWp, int T, int Tp, float temp1, long long ldp, hipStream_t stream);
int medmoe_local_gen_cos(const float* wc, const void* words, const float* wnorm, const int* cap_lens, float* sim, float* stats, float* sume, int B, int Bc, int T, int Tp, int D, float temp2, float eps, long long Kp, hipStream_t stream);
int medmoe_local_gen_dwctx(const float* wc, const void* words, const float* wnorm, const int* cap_lens, const float* gsim, const float* stats, const float* sume, void* dwc, int B, int Bc, int T, int Tp, int D, float temp2, float eps, long long Kp, hipStream_t stream);
/* d loss / d words of the generic-geometry local loss (trainable text tower), fp32 [Bc][T][D]: dws (fp32 [Kp][D] = dS^T ctx, the path through
   the word-softmax scores; NULL: none) + the cosine term summed over the B images in a fixed order; words t >= cap_lens[i] exactly 0 */
int medmoe_local_gen_dwords(const float* wc, const void* words, const float* wnorm, const int* cap_lens, const float* gsim, const float* stats, const float* sume, const float* dws, float* d_words, int B, int Bc, int T, int Tp, int D, float temp2, float eps, long long Kp, hipStream_t stream);
int medmoe_local_gen_bwd_s(const void* lp, const void* A, void* dA_io, const int* cap_lens, int B, int Bc, int HW, int HWp, int T, int Tp, float temp1, long long ldp, hipStream_t stream);
int medmoe_unpad_cast2(const float* src, const float* src2, void* dst, int B, int HW, int HWp, int D, hipStream_t stream);

/* mean over tokens: router input (swin.py:137) and global feature (swin.py:112) */
int medmoe_mean_tokens(const void* x, float* out, int B, int Nt, int D, int t0, int cnt, hipStream_t stream);

/* backward of mean_tokens */
int medmoe_broadcast_tokens(const float* g, void* dy, int B, int Nt, int D, int t0, int cnt, float scale, hipStream_t stream);

/* MoE router softmax + top-k (swin.py:88-92,98-100); fixed fp32 order => bit-exact indices */
int medmoe_router_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* probs, int* idx, float* gates, int B, int Dv, int Hd, int E, int k, hipStream_t stream);

/* CE on router probabilities (medmoe_module.py:235-237) + gate gradients -> dlogits, dh */
int medmoe_router_bwd(const float* probs, const float* h, const float* w2, const int* idx, const float* dgates, const int* labels, const float* dprobs_ext, float ce_scale, float* dlogits, float* dh, float* loss_acc, int B, int Hd, int E, int k, hipStream_t stream);

/* the two values medmoe_router_bwd accumulates, without a gradient (the evaluation step): loss_acc[0] = mean CE on the router probabilities,
   loss_acc[1] = accuracy; one workgroup, plain stores */
int medmoe_router_eval(const float* probs, const int* labels, float* loss_acc, int B, int E, hipStream_t stream);

/* small strided fp32 GEMM (router wgrad/dgrad, global-loss similarity and its gradients) */
int medmoe_sgemm(const float* A, const float* Bm, float* C, int M, int N, int K, long long sam, long long sak, long long sbk, long long sbn, long long ldc, float alpha, float beta, hipStream_t stream);

/* sort (sample,choice) pairs by expert; row maps + tile table for the grouped expert GEMMs (replaces the dense all-experts + gather of swin.py:105-108) */
int medmoe_dispatch(const int* idx, int B, int k, int E, int P, int Nt, int* slot_of, int* item_of_slot, int* expert_of_slot, int* row_off, int* tiles, int* tile_count, int max_tiles, int* rowmap, hipStream_t stream);

/* Expert scale attention + weighted sum (swin.py:62-80) */
int medmoe_scale_attn_fwd(const void* G, const void* H1, const float* w2, const float* b2, const int* expert_of_slot, int P, void* out, float* wts, int R, int Do, int Dh, hipStream_t stream);

/* combine selected experts into img_l (swin.py:106-113) */
int medmoe_combine_fwd(const void* expert_out, const int* slot_of, const float* gates, void* img_l, int B, int k, int P, int Do, hipStream_t stream);

/* backward of combine + scale attention */
int medmoe_scale_attn_bwd(const void* d_img_l, const float* d_img_g, const void* G, const void* H1, const float* wts, const float* w2, const void* expert_out, const int* expert_of_slot, const int* item_of_slot, const float* gates, int k, int P, void* dG, void* dH1, float* dw2, float* db2, float* dgate, int R, int Do, int Dh, hipStream_t stream);

/* pyramid-geometry experts: F.interpolate(size = Pout, mode = 'linear', align_corners = False) along the token axis (swin.py:42),
   bf16 [n, Pin, D] -> [n, Pout, D]; backward in gather form, optionally times ReLU'(relu_aux) of the interpolated projection's source */
int medmoe_lerp_tokens_fwd(const void* x, void* y, int n, int Pin, int Pout, int D, hipStream_t stream);
int medmoe_lerp_tokens_bwd(const void* dy, const void* relu_aux, void* dx, int n, int Pin, int Pout, int D, hipStream_t stream);
/* the same with the incoming gradient given as two summands dy + dy2 (Pin == Pout: dx = (dy + dy2) ReLU'(relu_aux)) */
int medmoe_lerp_tokens_bwd2(const void* dy, const void* dy2, const void* relu_aux, void* dx, int n, int Pin, int Pout, int D, hipStream_t stream);

/* scatter-add stage-feature gradients into the ViT residual-stream gradient */
int medmoe_stage_grad_add(const void* dF, const int* slot_of, void* dx, int B, int k, int P, int Nt, int D, hipStream_t stream);

/* Fp32LayerNorm forward (normalizations.py:8-19; transformer.py:78-79) */
int medmoe_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int D, float eps, int out_f32, hipStream_t stream);

/* y = bf16((x - mean) * rstd * gamma + beta) from the per-row statistics a LayerNorm forward launch saved: bit-identical to the y that launch
   wrote (activation recomputation).  x, y bf16 [rows, D]; D % 8 == 0, D <= 2048.  One streaming pass, no atomics. */
int medmoe_layernorm_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y, int rows, int D, hipStream_t stream);

/* Fp32LayerNorm backward (+ fused residual-gradient add) */
int medmoe_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const void* add, void* dx, float* dgamma, float* dbeta, int rows, int D, hipStream_t stream);

/* sum of squares of the flat gradient (clip_grad_norm_, pretraining_medmoe.yaml:23) */
int medmoe_sumsq(const float* g, long long n, float* out, hipStream_t stream);
/* the same with a fixed summation order (bit-identical on every data-parallel rank): out[0] = sum g^2; scratch >= 2049 floats, scratch[2048] zero on entry */
int medmoe_sumsq_det(const float* g, long long n, float* out, float* scratch, hipStream_t stream);

/* host scheduling aid, no reference counterpart (the reference trains on one stream under torch autograd): stream `to` waits for everything
   enqueued on `from` so far - how the hand-scheduled backward forks its weight-gradient GEMMs onto a second stream and joins them */
int medmoe_stream_fork(hipStream_t from, hipStream_t to);

/* fused clip + torch.optim.Adam step + bf16 down-cast (med-moe_pretraining.yaml:7-11) */
int medmoe_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);

/* the same step with parameter groups, one launch per arena: the arena is cut into n_runs contiguous runs (run_end: device int64[n_runs],
   ascending, last == n; a boundary may fall on any element), run r steps with (lr / bc1) * run_lr_mult[r] and decays with
   weight_decay * run_wd_mult[r] (device float[n_runs] each).  decoupled 0 = torch.optim.Adam (L2 decay added to the gradient, the update
   of medmoe_adam_step), 1 = torch.optim.AdamW (p *= 1 - lr_r * wd_r, then Adam on the undecayed gradient).  No atomics. */
int medmoe_adam_groups_step(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);

/* bf16 gradient exchange (no reference counterpart; what torch DDP's bf16_compress_hook does): out[i] = bf16(g[i] * scale), the product in
   fp32, round to nearest even; NaN / Inf pass through, -0 stays -0.  16-byte accesses: both pointers 16-byte aligned (MM_ERR_ARG otherwise;
   arena entries are padded to 8 elements), any n (a scalar tail covers n % 8).  6 B of HBM traffic per element. */
int medmoe_grad_pack_bf16(const float* g, void* out_bf16, long long n, float scale, hipStream_t stream);
/* medmoe_sumsq_det over a bf16 buffer (8-byte aligned): same grid, element order and partial-sum tree, so out[0] is bit-identical to
   medmoe_sumsq_det on the fp32 up-cast of the buffer - the clip coefficient of the bf16-reduced gradient stays identical on every rank */
int medmoe_sumsq_det_bf16(const void* g_bf16, long long n, float* out, float* scratch, hipStream_t stream);
/* medmoe_adam_step / medmoe_adam_groups_step reading the gradient as bf16 (8-byte aligned, the arena's layout): the update is bit-identical
   to theirs on float(g_bf16), and no pass widens the reduced gradient back to fp32.  No atomics. */
int medmoe_adam_step_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);
int medmoe_adam_groups_step_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);

/* weight EMA inside the optimiser launch (no reference counterpart): the four steps above with two more arguments, `ema` (fp32, the
   arena's layout) and `one_minus_decay` (1 - decay of THIS update, formed by the host in double and rounded once; in [0, 1], MM_ERR_ARG
   otherwise).  p, m, v and the bf16 copy are bit-identical to the sibling's; behind the update of an element the same lane computes
   ema = fadd_rn(ema, fmul_rn(one_minus_decay, fsub_rn(p_new, ema))) - three separately rounded fp32 operations, no contraction - and moves
   the average as whole float4s next to p, m, v (8 B/param more).  No atomics, nothing read from the host. */
int medmoe_adam_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay, hipStream_t stream);
int medmoe_adam_groups_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay, hipStream_t stream);
int medmoe_adam_step_ema_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay, hipStream_t stream);
int medmoe_adam_groups_step_ema_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay, hipStream_t stream);

/* LAMB on a flat arena (csrc/lamb.hip; You et al. 2019, apex FusedLAMB use_nvlamb = 0): three launches per arena and step.
   Segments: seg_end (device int64[n_segs], ascending, last == n; a boundary may fall on any element), one per parameter tensor, with
   seg_lr_mult / seg_wd_mult (device fp32[n_segs]) and rec_base (device int64[n_segs], from medmoe_lamb_plan on the HOST copy of seg_end).
     moments: g' = g grad_scale clip (medmoe_adam_step's coefficient, kept in scratch[medmoe_lamb_coef_slot]), m, v as Adam's (m formed in
              double and rounded once); u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) +
              weight_decay wd_mult p stays in registers, the partial sums of p^2 and u^2 per (chunk of medmoe_lamb_chunk() elements, segment)
              go to `scratch` (scratch_floats >= medmoe_lamb_scratch_floats(n, n_segs)) with plain stores
     ratios:  ratios[s] = |p_s| / |u_s| where both are > 0 and (always_adapt or weight_decay wd_mult_s != 0), else 1; min(., 1) with
              trust_clip; a segment's records are added in index order.  ratios: 3 n_segs floats (the ratios, then (sum p^2, sum u^2) pairs)
     apply:   p -= ((lr lr_mult_s) ratios[s]) u with u recomputed to the same bits, p_bf16 = bf16_rne(p); the _ema form averages as
              medmoe_adam_step_ema does
   No floating-point atomics, nothing read from the host: two runs from the same inputs give the same bits. */
long long medmoe_lamb_chunk(void);
long long medmoe_lamb_threads(void);
long long medmoe_lamb_ratio_threads(void);
long long medmoe_lamb_scratch_floats(long long n, long long n_segs);
long long medmoe_lamb_coef_slot(long long n, long long n_segs);   /* scratch[slot]: the clip coefficient the last moments launch used */
long long medmoe_lamb_plan(const long long* seg_end_host, long long n_segs, long long n, long long* rec_base_host);
int medmoe_lamb_moments(const float* p, const float* g, float* m, float* v, long long n, const long long* seg_end, const float* seg_wd_mult, const long long* rec_base, int n_segs, float* scratch, long long scratch_floats, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);
int medmoe_lamb_moments_g16(const float* p, const void* g_bf16, float* m, float* v, long long n, const long long* seg_end, const float* seg_wd_mult, const long long* rec_base, int n_segs, float* scratch, long long scratch_floats, double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream);
int medmoe_lamb_ratios(const float* scratch, long long scratch_floats, const long long* seg_end, const float* seg_wd_mult, const long long* rec_base, int n_segs, long long n, double weight_decay, int always_adapt, int trust_clip, float* ratios, hipStream_t stream);
int medmoe_lamb_apply(float* p, const float* m, const float* v, void* p_bf16, long long n, const long long* seg_end, const float* seg_lr_mult, const float* seg_wd_mult, int n_segs, const float* ratios, double lr, double beta1, double beta2, double eps, double weight_decay, int step, hipStream_t stream);
int medmoe_lamb_apply_ema(float* p, const float* m, const float* v, void* p_bf16, long long n, const long long* seg_end, const float* seg_lr_mult, const float* seg_wd_mult, int n_segs, const float* ratios, double lr, double beta1, double beta2, double eps, double weight_decay, int step, float* ema, float one_minus_decay, hipStream_t stream);

/* fp32 -> bf16 copy of the master weights */
int medmoe_cast_bf16(const float* src, void* dst, long long n, hipStream_t stream);

/* batched bf16 transposes: W^T copies read by the dgrad GEMMs */
int medmoe_transpose_many(const void* src, void* dst, const long long* table, int n_entries, int max_tiles, hipStream_t stream);

/* kernel-selection switches for tests and measurements (the defaults are the fastest measured):
 *   1 gemm_nt256 on/off   2 256x256 NT tiles on/off   3 256x256 wgrad tiles on/off   4 rows per range of the grouped wgrad (>= 256)
 *   5 largest NT grid (1..256, experiments on fewer CUs)   6 scores512 on/off
 *   7 gemm_nt4w (four-wave NT GEMM; 0 = the eight-wave gemm_nt512)   8 gemm_tn4w (0 = gemm_tn512)
 *   9 fewest rows per M range of the plain wgrad (>= 64, default 2048)
 * Returns MM_ERR_ARG for an unknown key or a value out of range. */
int medmoe_set_option(int key, int value);
/* measurement aid (bench.py labels its per-launch timings with it): the kernel the most recent medmoe_gemm_nt / _rows / _tiles256 call of this
 * process launched - 0 gemm_nt_kernel (128x128 tile), 1 gemm_nt256_kernel, 2 gemm_nt512_kernel, 3 gemm_nt512_kernel GROUPED,
 * 4 gemm_nt4w_kernel, 5 gemm_nt4w_kernel GROUPED; -1 before the first call */
int medmoe_last_gemm_nt_kernel(void);
/* the same for the weight-gradient family: the kernel the most recent medmoe_gemm_tn / _staged / _det / _cols / _cols_det / _gram / _gram_det
 * call of this process launched, generation * 8 + build * 2 + staged - generation 0 gemm_tn_kernel (128x128 tile), 1 gemm_tn512_kernel,
 * 2 gemm_tn4w_kernel; build 0 plain, 1 MAPPED, 2 COLG, 3 COLG + SCALE; staged 1 when the partial tiles went through a scratch and a summing
 * kernel; -1 before the first call.  A refused call leaves it unchanged.  split (may be NULL) receives that launch's nsplit: the row ranges
 * per tile, or the ROWS per range in the grouped four-wave form. */
int medmoe_last_gemm_tn_kernel(int* split);

/* ---- fp8 (OCP e4m3fn) expert weights on the CDNA4 fp8 MFMA (BASELINE.json configs[4]; reference swin.py:18-30 projections) ---- */
/* bf16 rows (gathered through rowmap when given; times colscale[slot_expert[row / rows_per_slot]][k] when given) -> e4m3 rows q[M][K]
   + one dequantisation scale per row s[M] = amax / 448 */
int medmoe_quant_rows_e4m3(const void* x, int ldx, const int* rowmap, const float* colscale, const int* slot_expert, int rows_per_slot, void* q, float* s, int M, int K, hipStream_t stream);
/* fp32 master weights [G][N][K] -> e4m3 q[G][N][K], transposed qT[G][K][N] (may be NULL), scales s[G][N] = amax_k / 448 */
int medmoe_quant_weights_e4m3(const float* w, void* q, void* qT, float* s, int G, int N, int K, hipStream_t stream);
/* grouped C[m][n] = epi(sa[m] * sb[g][n] * sum_k Aq[m][k] Bq[g][n][k] (+ bias[g][n])) over the 128-row tile table {group, m0, m_end, -};
   epi 0 none, 1 ReLU, 2 (. + residual) * (aux > 0); C / residual / aux bf16 with row pitch ldc; sb may be NULL (scales folded into A) */
int medmoe_gemm_fp8_grouped(const void* Aq, const float* sa, const void* Bq, const float* sb, const float* bias, void* C, int ldc, const void* residual, const void* aux, const int* tiles, const int* tile_count, int max_tiles, int N, int K, long long strideB, long long strideSb, long long strideBias, int epi, hipStream_t stream);

/* ---- MXFP8 expert weights on the CDNA4 block-scaled MFMA (OCP Microscaling: e4m3 elements, one E8M0 scale byte per block of 32 along
   the contraction dimension; DESIGN.md "MXFP8 expert weights") ---- */
/* bf16 rows (gathered through rowmap when given) -> e4m3 rows q[M][K] + scale bytes s[M][K/32]; K % 32 == 0 */
int medmoe_quant_rows_mx(const void* x, int ldx, const int* rowmap, void* q, void* s, int M, int K, hipStream_t stream);
/* fp32 master weights [G][N][K] -> e4m3 q[G][N][K] + scale bytes sq[G][N][K/32] (blocks along K) and, quantised again with blocks
   along N, e4m3 qT[G][K][N] + scale bytes sT[G][K][N/32]; K % 32 == 0, N % 32 == 0 */
int medmoe_quant_weights_mx(const float* w, void* q, void* sq, void* qT, void* sT, int G, int N, int K, hipStream_t stream);
/* grouped C[m][n] = epi(sum_k 2^(sa[m][k/32] - 127) Aq[m][k] * 2^(sb[g][n][k/32] - 127) Bq[g][n][k] (+ bias[g][n])) over the 128-row
   tile table {group, m0, m_end, -}; any K % 32 == 0; epi 0 none, 1 ReLU, 2 (. + residual) * (aux > 0); C / residual / aux bf16 with
   row pitch ldc.  Cq / Csq (both or neither; epi 1, N % 32 == 0): the bf16 result MX-quantised along n, Cq[M][N] + Csq[M][N/32],
   bit-identical to medmoe_quant_rows_mx of C.  strideSb: scale bytes per group. */
int medmoe_gemm_mx_grouped(const void* Aq, const void* sa, const void* Bq, const void* sb, const float* bias, void* C, int ldc, const void* residual, const void* aux, void* Cq, void* Csq, const int* tiles, const int* tile_count, int max_tiles, int N, int K, long long strideB, long long strideSb, long long strideBias, int epi, hipStream_t stream);

/* Dropout of the trainable text tower (csrc/dropout.hip, csrc/philox.h).  The keep mask is a pure function of (seed, step, site, element):
   Philox4x32-10 with key = the two halves of `seed`, counter = (group lo, group hi, site, step), one call per group of 4 consecutive
   elements along the fastest axis (element (row, col) of [rows][cols_padded]: group row * cols_padded / 4 + col / 4, word col % 4);
   an element survives iff its word >= thresh = floor(p * 2^32) and is scaled by `scale` = 1 / (1 - p).  step, site and thresh are
   32-bit values.  No kernel stores a mask except medmoe_dropout_mask (tests, debugging): out_u8[rows][cols] = 1 where kept. */
int medmoe_dropout_mask(unsigned char* out_u8, long long rows, int cols, int cols_padded, long long seed, long long step, long long site, long long thresh, hipStream_t stream);
/* y = keep * x * scale over [rows][cols] (cols % 4 == 0), bf16 or (is_f32) fp32; y may be x */
int medmoe_dropout_apply(const void* x, void* y, long long rows, int cols, int is_f32, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
/* x1 = residual + keep * z * scale (bf16, stored for medmoe_layernorm_bwd), y = LayerNorm(x1) with medmoe_layernorm_fwd's layout and statistics */
int medmoe_dropout_add_layernorm_fwd(const void* z, const void* residual, const float* gamma, const float* beta, void* x1, void* y, float* mean, float* rstd, int rows, int D, float eps, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
/* medmoe_attn_fwd / medmoe_attn_bwd for N <= 80, head_dim 64 (anything else: MM_ERR_SHAPE) with dropout on the probabilities: lse is of the
   undropped softmax, out = (keep * P * scale) V; the mask row of query q of (b, h) is (b * H + h) * N + q, its key axis padded to a multiple of 4 */
int medmoe_attn_drop_fwd(const void* qkv, void* out, float* lse, const unsigned char* key_mask, int B, int N, int H, int head_dim, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
int medmoe_attn_drop_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const unsigned char* key_mask, void* dqkv, float* delta, int B, int N, int H, int head_dim, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);

/* Stochastic depth of the image tower (csrc/dropout.hip; the engine's sites are 0x40000000 + 2 * layer + {0 attention, 1 feed-forward}).  out[n_sites][B] fp32 = 0 | (float)(1 / (1 - p[s])): sample b survives at
   site s iff medmoe_dropout_mask(rows 1, site site0 + s, thresh floor(p[s] * 2^32)) keeps column sample0 + b.  p_host: n_sites <= 128
   probabilities in [0, 1) in HOST memory - they travel to the kernel by value, nothing is read back from the device. */
int medmoe_drop_path_scales(float* out, const double* p_host, int n_sites, int B, long long sample0, long long seed, long long step, long long site0, hipStream_t stream);
/* x1 = bf16(residual + scale[row / rows_per_sample] * z) (fp32 product and sum; a row whose scale is 0 copies residual and never reads z),
   y = LayerNorm(x1) with medmoe_layernorm_fwd's layout and statistics.  rows % rows_per_sample == 0, D % 8 == 0, D <= 2048.  No atomics. */
int medmoe_scale_add_layernorm_fwd(const void* z, const void* residual, const float* scale, int rows_per_sample, const float* gamma, const float* beta, void* x1, void* y, float* mean, float* rstd, int rows, int D, float eps, hipStream_t stream);

/* ---- deterministic mode (MedMoEConfig.deterministic): the same results as the entry points they are named after, up to summation order, with
   no sum whose order depends on which workgroup or wave arrives first.  Two forms: STAGED - partial results leave with plain stores into a
   scratch buffer of the caller's (one per stream: launches that may overlap must not share it) and a second kernel adds them in index order;
   SINGLE WRITER - the launch is shaped so that one workgroup adds to an output element.  A scratch that is too small is MM_ERR_ARG, never a
   fall-back to the atomic form.  No process-global switch: the caller chooses the entry point. */
/* medmoe_gemm_tn (dW and db): staged on the four-wave kernel for plain rows / one row map / router groups with Kk % 256 == 0, Nn % 128 == 0
   (plain: % 256, M % 32 == 0, M >= 4096) and at least 2048 rows per group - a group's ranges are enumerated from row_off on the device by the
   GEMM and by the summing kernel alike; every other shape: one workgroup per (group, 128 x 128 tile).  scratch_floats >=
   medmoe_gemm_tn_det_scratch(M, Nn, Kk, x_rowmap != NULL, g_rowmap != NULL, row_off != NULL, n_groups) (0: the shape needs none) */
int medmoe_gemm_tn_det(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, float* db, int M, int Nn, int Kk, const int* x_rowmap, const int* g_rowmap, const int* row_off, int n_groups, long long strideW, long long strideDb, float* scratch, long long scratch_floats, hipStream_t stream);
long long medmoe_gemm_tn_det_scratch(int M, int Nn, int Kk, int x_mapped, int g_mapped, int grouped, int n_groups);
/* medmoe_gemm_tn_cols, staged when a tile has more than one row range; scratch_floats >= medmoe_gemm_tn_cols_det_scratch(M, Nn, Kk, n_groups) */
int medmoe_gemm_tn_cols_det(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk, int n_groups, long long gcol_stride, long long xcol_stride, long long strideW, int g_chunk_w, long long g_chunk_stride, float* scratch, long long scratch_floats, hipStream_t stream);
long long medmoe_gemm_tn_cols_det_scratch(int M, int Nn, int Kk, int n_groups);
/* medmoe_gemm_tn_gram with a single writer per output tile (no split over the rows) */
int medmoe_gemm_tn_gram_det(const void* A, int lda, const float* w, long long w_gstride, int w_ld, float* dW, int ldw, int M, int Nn, int n_groups, long long col_stride, long long strideW, hipStream_t stream);
/* medmoe_layernorm_bwd, dgamma / dbeta staged per workgroup; scratch_floats >= medmoe_layernorm_bwd_det_scratch(D) */
int medmoe_layernorm_bwd_det(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const void* add, void* dx, float* dgamma, float* dbeta, int rows, int D, float* scratch, long long scratch_floats, hipStream_t stream);
long long medmoe_layernorm_bwd_det_scratch(int D);
/* medmoe_scale_attn_bwd, dw2 / db2 / dgate staged per wave (a wave's rows lie in one slot); row_off [E + 1]: medmoe_dispatch's first slot row
   of every expert; scratch_floats >= medmoe_scale_attn_bwd_det_scratch(R, P, Dh) */
int medmoe_scale_attn_bwd_det(const void* d_img_l, const float* d_img_g, const void* G, const void* H1, const float* wts, const float* w2, const void* expert_out, const int* expert_of_slot, const int* item_of_slot, const float* gates, int k, int P, void* dG, void* dH1, float* dw2, float* db2, float* dgate, int R, int Do, int Dh, const int* row_off, int E, float* scratch, long long scratch_floats, hipStream_t stream);
long long medmoe_scale_attn_bwd_det_scratch(int R, int P, int Dh);
/* medmoe_router_bwd with the cross-entropy and the accuracy summed in sample order; parts: 2 * B floats */
int medmoe_router_bwd_det(const float* probs, const float* h, const float* w2, const int* idx, const float* dgates, const int* labels, const float* dprobs_ext, float ce_scale, float* dlogits, float* dh, float* loss_acc, int B, int Hd, int E, int k, float* parts, hipStream_t stream);
/* the three loss heads with loss_acc += the rows' terms in row order; parts: `rows` floats */
int medmoe_ce_strided_det(const float* X, float* dX, int rows, int cols, long long rs, long long cs, int label_off, float xscale, float w, int accumulate, float* loss_acc, float* parts, hipStream_t stream);
int medmoe_soft_xent_strided_det(const float* X, float* dX, const float* soft, int rows, int cols, long long rs, long long cs, float xscale, float t1, float t2, float w, int accumulate, float* loss_acc, float* parts, hipStream_t stream);
int medmoe_hardneg_strided_det(const float* X, float* dX, int rows, int cols, long long rs, long long cs, float margin, float w, int accumulate, float* loss_acc, float* parts, hipStream_t stream);
/* medmoe_cos_scale_bwd with cb summed by one thread per column in row order */
int medmoe_cos_scale_bwd_det(float* dC, const float* C, const float* na, const float* nb, float* ca, float* cb, int M, int N, float eps, hipStream_t stream);
/* how many launches of this process took an order-dependent form so far (an atomic epilogue with more than one writer per element, an atomic
   loss sum): counted on the host, one add per such launch.  A deterministic step leaves it unchanged. */
long long medmoe_nondet_launches(void);

/* LoRA adapters on the text tower's fused q / k / v projection (csrc/lora.hip).  n targets (1..3) own the D columns of a qkv row
   (pitch ldq) from c0 / c1 / c2 on (multiples of 8, not overlapping; D % 64 == 0).  Adapters are stored padded to rank 16 and stacked over the
   targets: A [n*16][D], Bw [n*D][16] (pad rows of A / pad columns of Bw zero), At [D][n*16] and Bt [16][n*D] their transposes; U and dU are
   [M][n*16] bf16; s = lora_alpha / r.  Dropout on the side path's input: the (seed, step, site, thresh, scale) of medmoe_dropout_apply over
   the [M][D] array, thresh = 0 for none.
   fwd: U = (keep X scale) A^T, qkv[:, c_t : c_t + D] = bf16(qkv + s U_t B_t^T), one launch. */
int medmoe_lora_fwd(const void* X, const void* A, const void* Bw, void* U, void* qkv, int ldq, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
/* dU_t = bf16(s dqkv_t B_t); dy [M][D] (bf16, may be null: nothing below trains) += keep scale (dU A) */
int medmoe_lora_bwd_dx(const void* dqkv, int ldq, const void* Bt, const void* At, void* dU, void* dy, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
/* gB [n*D][16] += s dqkv_t^T U_t, gA [n*16][D] += dU_t^T (keep X scale): partial sums per 256 rows in `scratch`
   (scratch_floats >= medmoe_lora_wgrad_scratch(M, D, n)), added up in a fixed order by a second kernel - no atomics */
int medmoe_lora_bwd_wgrad(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB, float* scratch, long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
long long medmoe_lora_wgrad_scratch(int M, int D, int n);
/* the same sums at the image tower's row counts: a workgroup accumulates over `run` (>= 1) consecutive 256-row chunks before it
   stores one partial, ceil(chunks / run) partials are added in run order - no atomics, two launches are bit-identical, run = 1 gives the bits
   of medmoe_lora_bwd_wgrad.  scratch_floats >= medmoe_lora_wgrad_runs_scratch(M, D, n, run) */
int medmoe_lora_bwd_wgrad_runs(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB, float* scratch, long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, int run, float s, long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream);
long long medmoe_lora_wgrad_runs_scratch(int M, int D, int n, int run);
/* W (bf16 [>= c_t + D rows][ldw], a copy of the fused projection's weight): rows c_t .. c_t + D - 1 = bf16(W + s B_t A_t) */
int medmoe_lora_merge(void* W, int ldw, const void* A, const void* Bw, int D, int n, int c0, int c1, int c2, float s, hipStream_t stream);

/* Variable-length backward of a TRAINABLE text tower: the text pass on the packed non-padding tokens of medmoe_text_pack.  Every
   entry point takes the row count as a DEVICE int (count / rows_dev, 1 <= value <= the host-side bound that sizes the grid); rows at and past
   the count are neither read for a result nor written, and reach no sum.
   attn_bwd_varlen: medmoe_attn_bwd on medmoe_attn_fwd_varlen's layout - qkv / dqkv [sum len][3*H*64], out / dout [sum len][H*64], lse and
   delta [B][H][Nmax]; Nmax <= 80, no key mask (every key of a sequence is valid). */
int medmoe_attn_bwd_varlen(const void* qkv, const void* out, const void* dout, const float* lse, const int* seq_off, void* dqkv, float* delta, int B, int Nmax, int H, int head_dim, hipStream_t stream);
/* medmoe_layernorm_bwd over the first min(rows, *rows_dev) rows; dgamma / dbeta may both be null */
int medmoe_layernorm_bwd_rows(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const void* add, void* dx, float* dgamma, float* dbeta, int rows, int D, const int* rows_dev, hipStream_t stream);
/* dH[r] = d_word[b, seg[src]] + d_sent[b] / T (0 where seg[src] < 0) for packed row r < *count, src = src_of_row[r], b = src / T */
int medmoe_text_aggregate_bwd_packed(const float* d_word, const float* d_sent, const int* seg, const int* src_of_row, const int* count, void* dH, int B, int T, int D, hipStream_t stream);
/* medmoe_text_embed_ln_bwd on packed dy rows: ids / type_ids read at src = src_of_row[r], position src % T; dx (fp32 [B*T][D], zeroed by the
   caller) is written at row src; g_word / dgamma / dbeta accumulate (fp32 atomics) */
int medmoe_text_embed_ln_bwd_packed(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type, const float* gamma, const void* dy, float* dx, float* dgamma, float* dbeta, float* g_word, int B, int T, int D, int vocab, float eps, const int* src_of_row, const int* count, hipStream_t stream);
/* medmoe_lora_fwd / _bwd_dx / _bwd_wgrad over the first min(M, *rows_dev) rows; the wgrad scratch is sized for M, a 256-row chunk past the
   count adds exact zeros in the same fixed order */
int medmoe_lora_fwd_rows(const void* X, const void* A, const void* Bw, void* U, void* qkv, int ldq, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, const int* rows_dev, hipStream_t stream);
int medmoe_lora_bwd_dx_rows(const void* dqkv, int ldq, const void* Bt, const void* At, void* dU, void* dy, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, const int* rows_dev, hipStream_t stream);
int medmoe_lora_bwd_wgrad_rows(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB, float* scratch, long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale, const int* rows_dev, hipStream_t stream);

/* Retrieval and zero-shot evaluation (csrc/retrieval.hip).
   y[r] = x[r] / max(|x[r]|_2, eps) over the rows of fp32 [rows][D]; y may be x; a zero row stays zero.  The norm is rounded to fp32 once
   (its sum of squares runs in double) and the quotient once. */
int medmoe_l2_normalize(const float* x, float* y, int rows, int D, float eps, hipStream_t stream);
/* For every row of q (fp32 [Nq][D]) the K best rows of keys (fp32 [Nk][D]) under the total order (score descending, key index ascending);
   the score is the fp32 dot product, nothing is normalised here.  top_val fp32 [Nq][K], top_idx int32 [Nq][K]; positions past min(K, Nk) hold
   -inf / -1.  Scores are single v_mfma_f32_16x16x4_f32 chains over D in ascending order (the bits of an fmaf chain), so a score depends on its
   (query, key) pair alone; the [Nq][Nk] matrix is never stored.  The keys are split into S contiguous chunks (grid = query tiles x S); with
   S > 1 the partial lists go to `scratch` (scratch_elems >= medmoe_sim_topk_scratch(Nq, Nk, D, K)) and a second launch merges them.  The
   result does not depend on S, bit for bit; no atomics, two launches give the same bits.  A NaN score is never listed.
   1 <= K <= 16, D % 64 == 0; anything else returns -2 before a launch. */
int medmoe_sim_topk(const float* q, const float* keys, int Nq, int Nk, int D, int K, float* top_val, int* top_idx, float* scratch, long long scratch_elems, hipStream_t stream);
/* scratch elements (4 bytes each) of medmoe_sim_topk at the current split setting, 0 when no scratch is needed; medmoe_sim_rank needs no
   more than medmoe_sim_topk_scratch(Nq, Nk, D, 1) */
long long medmoe_sim_topk_scratch(int Nq, int Nk, int D, int K);
/* tests: key splits S of medmoe_sim_topk / medmoe_sim_rank (0 = automatic, at most 64) */
int medmoe_sim_topk_splits(int n);
/* rank[i] (int32) = the number of keys ordered before keys[target[i]] for query i under the order of medmoe_sim_topk:
   #{j : s_ij > s_it} + #{j < t : s_ij == s_it}.  The same main loop as medmoe_sim_topk with a counting epilogue; the target's score is the
   diagonal of a gathered tile run through that loop, so an exact duplicate of the target row compares equal.  Per-split counts are summed as
   integers.  A target outside [0, Nk) is scored as a zero row (no fault, the count is meaningless).  D % 64 == 0, else -2 before a launch. */
int medmoe_sim_rank(const float* q, const float* keys, const int* target, int Nq, int Nk, int D, int* rank, float* scratch, long long scratch_elems, hipStream_t stream);

/* Supervised classification (csrc/classify.hip).  A linear head on fp32 features: x [N][D], W [C][D], b [C], z = x W^T + b [N][C].
   D % 64 == 0, 64 <= D <= 2048, 1 <= C <= 64, N >= 1 - anything else returns -2 before a launch; x, W, dx, the targets and the scratch must be 16-byte aligned.
   medmoe_cls_head_logits writes z alone (evaluation). */
int medmoe_cls_head_logits(const float* x, const float* W, const float* b, float* z, int N, int D, int C, hipStream_t stream);
/* Forward + loss + backward of the head in one call.  task 0, multiclass: targets int32 [N] in [0, C), -1 = the row is not counted; V the
   counted rows, q_n = (1 - label_smoothing) onehot(y_n) + label_smoothing / C, L = loss_scale / |V| sum_V -sum_c q_nc log softmax(z_n)_c,
   dz_n = loss_scale / |V| (softmax(z_n) - q_n) on V and 0 elsewhere.  task 1, multilabel: targets int8 [N][C] in {0, 1, -1}, -1 = the
   element is not counted; K the counted elements, pos_weight fp32 [C] or null (= 1), l = pw_c t softplus(-z) + (1 - t) softplus(z) with
   softplus(z) = max(z, 0) + log1p(exp(-|z|)), L = loss_scale / |K| sum_K l, dz = loss_scale / |K| ((1 - t) sigmoid(z) - pw_c t sigmoid(-z))
   on K and 0 elsewhere; label_smoothing is not used.
   Written: z [N][C]; *loss; counts[0] = |V| or |K|, counted on the device; counts[1] = multiclass: the rows of V whose argmax z (ties: the
   lowest class) is the target, multilabel: the elements of K with (z > 0) == (t == 1); dx = dz W [N][D] when dx is not null (written, not
   accumulated).  Accumulated: dW [C][D] += dz^T x, db [C] += sum_n dz.  A count of 0 gives L = 0, dz = 0 and no NaN.
   No fp32 atomics: the loss is summed from per-row terms in a fixed order (segments of 1024 rows, then the segments), dW / db from per-row-range records in range order (scratch_floats >=
   medmoe_cls_head_scratch(N, D, C), which also holds dz) - two calls give the same bits.  x is read twice (rows, then dW). */
int medmoe_cls_head_step(const float* x, const float* W, const float* b, const void* targets, const float* pos_weight, int task, float label_smoothing, float loss_scale, float* z, float* dx, float* dW, float* db, float* loss, int* counts, float* scratch, long long scratch_floats, int N, int D, int C, hipStream_t stream);
/* scratch floats of medmoe_cls_head_step, 0 for a shape it refuses */
long long medmoe_cls_head_scratch(int N, int D, int C);
/* Pair counts of the Mann-Whitney AUROC per class: scores fp32 [N][C] (finite - not checked), targets int8 [N][C] in {0, 1, -1} (-1: the
   element takes no part; multiclass callers pass one-hot rows), out int64 [C][4] = (n_pos, n_neg, n_less, n_equal) with
   n_less = #{(i, j) : t_ic = 1, t_jc = 0, s_jc < s_ic} and n_equal the same pairs with s_jc == s_ic.  The negatives stream past tiles of
   256 positives through LDS, nothing of size [N][N] is stored; the counts are 64-bit integer adds: exact and repeatable. */
int medmoe_auroc_counts(const float* scores, const signed char* targets, long long* out, int N, int C, hipStream_t stream);

/* Masked-language-model objective of the text tower (csrc/mlm.hip).
   The step's mask, drawn on the chip.  ids int32 [B][T], attn uint8 [B][T]; a token is a candidate iff attn != 0 and its id is none of
   cls_id / sep_id / pad_id.  Token t of global sample g = sample_offset + b owns the Philox group g * T + t of (seed, step, site
   DROPOUT_SITE_MLM): word 0 selects it iff word0 < thresh (= floor(p * 2^32)); word 1 picks the action - below floor(0.8 * 2^32) the id
   becomes mask_id, below floor(0.9 * 2^32) it becomes mulhi(word2, V), else it is kept.  A pure function of (seed, step, global sample,
   position): no launch geometry, no padded / packed layout enters.
   Written: ids_masked [B][T]; labels [B][T] = the original id where selected, -1 elsewhere; rows [B*T] = the selected tokens' row indices,
   ascending - b * T + t, or tok_row[b * T + t] (medmoe_text_pack) when tok_row is not null; row_labels aligned with rows; count [1].  The
   tails of rows / row_labels past the count are not written.  One workgroup, the list positions come from a scan: no atomics, nothing is
   read back.  B * T < 2^31, V >= 2, 0 <= mask_id < V, sample_offset >= 0, 0 <= thresh < 2^32 - anything else returns -2 before a launch. */
int medmoe_mlm_mask(const int* ids, const unsigned char* attn, const int* tok_row, int* ids_masked, int* labels, int* rows, int* row_labels, int* count, int B, int T, int V, int cls_id, int sep_id, int pad_id, int mask_id, long long sample_offset, long long seed, long long step, long long thresh, hipStream_t stream);
/* bf16 rows of D elements (D % 8 == 0, 16-byte aligned), k < min(*count, M_bound); the listed rows are distinct, so the add has one writer:
   gather       dst[k] = src[rows[k]]                    scatter_add  dst[rows[k]] = bf16(dst[rows[k]] + src[k])
   mul          dst[k] = bf16(a[k] * b[k]), and dst[k] = 0 for count <= k < M_bound */
int medmoe_rows_gather(const void* src, const int* rows, const int* count, void* dst, int M_bound, int D, hipStream_t stream);
int medmoe_rows_scatter_add(const void* src, const int* rows, const int* count, void* dst, int M_bound, int D, hipStream_t stream);
int medmoe_rows_mul(const void* a, const void* b, const int* count, void* dst, int M_bound, int D, hipStream_t stream);
/* The tied decoder fused with its cross-entropy.  z bf16 [M_bound][D], the first n = min(*count, M_bound) rows live (count on the device); E
   bf16 [V][D]; bias fp32 [V]; row_labels int32 [M_bound] in [0, V) on the live rows.  logits = z E^T + bias on the bf16 MFMA with fp32
   accumulation; no [M][V] array is written anywhere: a workgroup reduces its 64 x 256 tile to one (max, sum exp) pair per row, a second
   kernel merges a row's ceil(V / 256) pairs in tile order, a third sums the rows in a fixed order.
   Written: lse [M_bound] and terms [M_bound] = lse - logit[target] (both 0 at and past n); loss [1] = loss_scale / n * sum of the live
   terms, 0 when n = 0; counts[0] = n, counts[1] = the live rows whose target logit equals the row's maximum.  A row at or past n is never
   read into a result (its z is replaced by zeros as it is staged).  No atomics: two calls give the same bits.
   D % 64 == 0, 64 <= D <= 1024, V >= 2, M_bound >= 1 - anything else returns -2 before a launch; z and E 16-byte aligned;
   scratch_floats >= medmoe_vocab_ce_scratch(M_bound, V, D) = (2 ceil(V / 256) + 2) M_bound. */
int medmoe_vocab_ce_fwd(const void* z, const void* E, const float* bias, const int* row_labels, const int* count, float loss_scale, float* lse, float* terms, float* loss, int* counts, float* scratch, long long scratch_floats, int M_bound, int V, int D, hipStream_t stream);
/* scratch floats of medmoe_vocab_ce_fwd, 0 for a shape it refuses */
long long medmoe_vocab_ce_scratch(int M_bound, int V, int D);
/* Its backward, P = (softmax(logits) - onehot(target)) loss_scale / n recomputed tile by tile from lse (fp32, rounded to bf16 for the second
   product) and never stored: _dx owns 64 token rows per workgroup, streams the vocabulary and WRITES dz = P E (bf16 [M_bound][D], rows at
   and past n untouched); _dw owns 64 vocabulary rows, streams the token rows and ACCUMULATES dE [V][D] += P^T z, dbias [V] += sum over rows
   of P (fp32).  Every output element has one owner: no atomics, two calls give the same bits; n = 0 launches nothing that writes.  Shapes
   and refusals as medmoe_vocab_ce_fwd. */
int medmoe_vocab_ce_bwd_dx(const void* z, const void* E, const float* bias, const int* row_labels, const float* lse, const int* count, float loss_scale, void* dz, int M_bound, int V, int D, hipStream_t stream);
int medmoe_vocab_ce_bwd_dw(const void* z, const void* E, const float* bias, const int* row_labels, const float* lse, const int* count, float loss_scale, float* dE, float* dbias, int M_bound, int V, int D, hipStream_t stream);

/* ---- semantic segmentation on the region features (csrc/segment.hip) ----
   A linear decoder with independent sigmoids per class.  1 <= C <= 8, D % 64 == 0, 64 <= D <= 2048, 1 <= g <= 64 patches per axis,
   H >= g and W >= g (anything else returns -2 before a launch).  No fp32 atomic: every sum leaves as per-workgroup records added in index
   order, two calls give the same bits and medmoe_nondet_launches() never moves.
   z [N][C] fp32 = feat [N][D] (bf16, 16-byte aligned) W^T [C][D] + b [C] (fp32), fp32 arithmetic. */
int medmoe_seg_head_fwd(const void* feat, const float* W, const float* b, float* z, int N, int D, int C, hipStream_t stream);
/* z [B][g g][C] against masks int8 [B][C][H][W] in {0, 1, -1} (-1: ignored, enters no sum and no gradient; 16-byte aligned).  zf[b][c][y][x] is
   the bilinear upsample of z to H x W (torch interpolate, align_corners = false: src = (dst + 0.5) g / H - 0.5 clamped at 0), recomputed per
   pixel and never stored.  loss [1] = loss_scale (w_bce L_bce + w_dice L_dice) is WRITTEN:
     L_bce  = 1 / |K| sum over the valid (pixel, class) pairs of pos_weight_c t softplus(-zf) + (1 - t) softplus(zf)   (pos_weight NULL: 1)
     L_dice = 1 - mean over the classes with a valid pixel of (2 I_c + eps) / (P_c + T_c + eps),  I = sum p t, P = sum p, T = sum t, p = sigmoid(zf)
   |K| = 0: loss 0, dz 0.  counts int64 [C][4] = (n_valid, TP, FP, FN) at the threshold zf > 0 is WRITTEN (|K| = sum of n_valid).
   dz [B][g g][C] (NULL: evaluation, no gradient pass) is WRITTEN with d loss / d z, the adjoint of the upsample in gather form.
   scratch_floats >= medmoe_seg_scratch(B, g, H, W, D, C) for any D (-1 otherwise). */
int medmoe_seg_loss(const float* z, const signed char* masks, const float* pos_weight, float w_bce, float w_dice, float dice_eps, float loss_scale, float* dz, float* loss, long long* counts, float* scratch, long long scratch_floats, int B, int g, int H, int W, int C, hipStream_t stream);
/* dfeat [N][D] bf16 = dz W is WRITTEN (NULL: not formed); dW [C][D] += dz^T feat and db [C] += sum dz through records per row range, added
   in range order.  scratch as for medmoe_seg_loss (the two launches may share it: they run one after the other). */
int medmoe_seg_head_bwd(const float* dz, const void* feat, const float* W, void* dfeat, float* dW, float* db, float* scratch, long long scratch_floats, int N, int D, int C, hipStream_t stream);
/* masks uint8 [B][C][H][W] = (zf > 0) (16-byte aligned); zf fp32 [B][C][H][W] is written too when not NULL */
int medmoe_seg_predict(const float* z, unsigned char* masks, float* zf, int B, int g, int H, int W, int C, hipStream_t stream);
/* scratch floats of medmoe_seg_loss / medmoe_seg_head_bwd, 0 for a shape they refuse */
long long medmoe_seg_scratch(int B, int g, int H, int W, int D, int C);
/* the share of it medmoe_seg_head_bwd alone needs (it knows no mask size): the records of dW / db, 0 for a shape it refuses */
long long medmoe_seg_head_bwd_scratch(int N, int D, int C);

/* ---- phrase grounding: word-region heat maps scored against boxes (csrc/ground.hip) ----
   One owner per output element, nothing is combined through memory: two calls give the same bits and medmoe_nondet_launches() never moves.
   h fp32 [n][P] is WRITTEN for the n entries (image b, caption i, word_lo, word_hi) of `entries` (device int32 [n][4], 16-byte aligned; the
   span is half-open, 0 <= word_lo < word_hi <= cap_lens[i]; the caller validates the table, the kernel trusts it).  ctx bf16 [B][P][D], words
   bf16 [Bc][T][D] (16-byte aligned), cap_lens int32 [Bc].  s_raw[t][p] = <ctx[b][p], words[i][t]>: bf16 products, fp32 accumulation on
   v_mfma_f32_16x16x32_bf16, fp32 after it.
     mode 0 (attention): s[.][p] = softmax of s_raw[.][p] over the words t < cap_lens[i]; a[t][.] = softmax of temp1 s[t][.] over the regions;
                         h[p] = mean of a[t][p] over the span (a one-word span over a matched pair: a row of the local loss's attention map).
     mode 1 (cosine):    h[p] = <ctx_p, u> / max(|ctx_p| |u|, eps), u = the sum of words[i][t] over the span.
   P = g g with g <= 32, 1 <= T <= 80, D % 64 == 0, 64 <= D <= 2048 (anything else returns -2 before a launch); 0 <= temp1 <= 64, mode in
   {0, 1} (-1 otherwise); n == 0 returns 0 without a launch. */
int medmoe_ground_maps(const void* ctx, const void* words, const int* cap_lens, const int* entries, float* h, int n, int B, int Bc, int P, int T, int D, int mode, float temp1, float eps, hipStream_t stream);
/* Scores n grid maps h fp32 [n][g g] (any map, not only medmoe_ground_maps') against boxes int32 [n][NB][4] = (x0, y0, x1, y1), half-open pixel
   rectangles of the H x W frame (x1 <= x0 or y1 <= y0: absent), 1 <= NB <= 8, at the thresholds theta fp32 [NTH], 0 <= NTH <= 4; 1 <= g <= 32,
   H >= g, W >= g, H W <= 2^30 (-2 otherwise).  hf[y][x] is the bilinear upsample of h to H x W - the map of medmoe_seg_loss (seg_plan.h) -
   recomputed per pixel; hf fp32 [n][H][W], when not NULL, is WRITTEN with exactly the values the statistics saw.
     rec_f fp32 [n][2 + NTH]    = (max, min, thr_0, ...), thr_k = min + theta_k (max - min)
     rec_i int32 [n][4 + 2 NTH] = (y, x, hit, area, inter_0, pred_0, ...): (y, x) the first maximal pixel in row-major order, hit = it lies in the
                                  union of the boxes, area = the union's pixels, pred_k = #{hf >= thr_k}, inter_k = #{hf >= thr_k, in the union}
     rec_d fp64 [n][4]          = (S_in, Q_in, S_all, Q_all): the sums of hf and hf^2 over the union and over the frame, in a fixed order */
int medmoe_ground_score(const float* h, const int* boxes, const float* theta, float* hf, float* rec_f, int* rec_i, double* rec_d, int n, int g, int H, int W, int NB, int NTH, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MEDMOE_HIP_H */
