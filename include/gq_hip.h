/*
 * gq_hip.h -- C ABI of libgq_hip.so, the MI355X (gfx950) implementation of
 * GuidedQuant's quantized-linear decode path.
 *
 * Plain pointers + sizes, no torch types.  Every device pointer must be
 * resident on the current HIP device; work is enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream).  No entry point
 * allocates, frees, synchronises or retains a pointer, so all of them are
 * hipGraph-capturable.  Return value: 0 on success, a negative GQ_E* code on
 * error (never exit()/abort(), unlike the reference's HANDLE_ERROR,
 * inference/ap_gemv/gemv.cu:20-27); gq_last_error() returns a thread-local
 * message for the last failure.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * the upstream snu-mllab/GuidedQuant tree).  The reference-side bindings a
 * maintainer would add are shown in INTEGRATION.md.
 */
#ifndef GQ_HIP_H
#define GQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_OK 0
#define GQ_EINVAL (-22)   /* bad argument (shape / bitwidth / alignment) */
#define GQ_ENOTSUP (-95)  /* valid request this build has no kernel for */
#define GQ_EHIP (-5)      /* HIP runtime error, see gq_last_error() */

#define GQ_DTYPE_F16 0

/* epilogue / prologue flags of the fused GEMV entry point */
#define GQ_EPI_NONE 0u
#define GQ_EPI_RESIDUAL 1u  /* out[n] = residual[n] + y[n]          (fp16 add) */
#define GQ_PRO_SILU_MUL 2u  /* prologue: x holds 2K values (gate|up), the GEMV input is silu(x[0:K]) * x[K:2K] */
#define GQ_EPI_SILU_PAIRS 4u /* epilogue: the rows are (gate_i, up_i) pairs (row 2i, row 2i+1); out has N/2 elements,
                              * out[i] = silu(y[2i]) * y[2i+1] with the reference's fp16 rounding points */

int gq_version(void);
const char *gq_last_error(void);
/* number of HIP devices visible, <0 on error; lets a host check the library is usable */
int gq_device_count(void);

/*
 * Arithmetic mode of the Any-Precision GEMV (process-wide; also env GQ_AP_EXACT=1):
 *   0  fast  (default): bit-plane GEMVs on the matrix cores, exact products, fp32 accumulation -- closer to the
 *            exact result than the reference kernel, within the north-star tolerance of it (bits 2..4, K % 256 == 0;
 *            other shapes fall back to the exact kernels)
 *   1  exact: reproduces the reference kernel's fp16 accumulation order bit for bit (anyprec.cu:495-512)
 *  -1  reset to the default / environment
 */
int gq_set_ap_mode(int mode);

/*
 * Any-Precision LUT-GEMV.   out[m][n] = sum_k x[m][k] * lut[n][code(n,k)]
 * Replaces ap_gemv.anyprec_gemv -> anyprec_gemv_stream -> anyprec_matmul ->
 * matmul_kbit_32<M,bits,ksplit>  (inference/ap_gemv/bindings.cpp:14,
 * gemv.cu:56-107, anyprec.cu:372-542,591-620).
 *   x       fp16 [M][K]              (M = 1..8; decode uses M = 1)
 *   out     fp16 [M][N]              written directly, no pre-zeroing needed
 *   qweight u32  [>=bits][N][K/32]   bit-plane packed, MSB plane first
 *                                    (any_precision/quantization/pack.py:304-321);
 *                                    plane stride is N*K/32 words
 *   lut     fp16 [N][2^bits]
 * In exact mode results are bit-identical to the reference kernel's fp16 accumulation order; in fast mode they
 * are within 1e-3 (relative, fp16) of it and closer to the exact product.
 * Requires K % 32 == 0, 2 <= bits <= 8.
 */
int gq_anyprec_gemv(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t M, uint32_t N,
                    uint32_t K, int bits, int dtype, void *stream);

/*
 * Any-Precision dequantise.   W[n][k] = lut[n][code(n,k)]   (fp16 [N][K])
 * Replaces ap_gemv.anyprec_dequant -> anyprec_dequant_kbit -> dequant_kbit_store<bits>
 * (bindings.cpp:15, gemv.cu:109-134, anyprec.cu:294-359,627-645).
 */
int gq_anyprec_dequant(const uint32_t *qweight, const void *lut, void *W, uint32_t N, uint32_t K, int bits,
                       void *stream);

/*
 * Any-Precision packer on the device: codes u8 [N][K] (values < 2^bits) -> qweight u32 [bits][N][K/32], bit-identical to the
 * host packer of a quantization run (any_precision/quantization/pack.py:12-83,101-110,304-321: np.packbits per plane + the
 * warp byte permutation).  codes 8-byte aligned, K % 32 == 0, bits 1..8 (the parent precision).
 */
int gq_anyprec_pack(const uint8_t *codes, uint32_t *qweight, uint32_t N, uint32_t K, int bits, void *stream);

/*
 * LNQ coordinate descent, one 128-column block (any_precision/quantization/layerwise_quantize.py:93-118, the inner loop of
 * update_P): for j = col_start .. col_end - 1 in order, per output row:  sol = W[j] - B[j];  a = argmin_c |sol - C[c]| (lowest
 * index on ties);  assign[j] = a, What[j] = C[a];  B[k] += (C[a] - W[j]) * Hn[j][k] for j < k < col_end.
 *   W, B, What f32 [N][d] (B is read, its running copy lives in LDS);  Hn f32 [groups][d][d] = H with column k divided by
 *   H[k][k];  C f32 [N][n_cluster], 2 <= n_cluster <= 16;  assign u8 [N][d];  group_rows = N / groups, a multiple of 32.
 * fp32, the reference's operation order, no contraction.
 */
int gq_lnq_cd_block(const float *W, const float *B, const float *Hn, const float *C, uint8_t *assign, float *What, uint32_t N,
                    uint32_t d, uint32_t n_cluster, uint32_t group_rows, uint32_t col_start, uint32_t col_end, void *stream);

/*
 * Any-Precision prefill GEMM with the dequantisation fused into the matrix-core loop.
 *   out[s][n] = sum_k x[s][k] * lut[n][code(n,k)]        x fp16 [S][K], out fp16 [S][N] (written)
 * Replaces the seq_len > 1 branch of APLinear.forward / AnyPrecisionLinear.forward (inference/APLinear.py:35-50,
 * any_precision/modules/AnyPrecisionLinear.py:69-71): ap_gemv.anyprec_dequant (dequant_kbit_store, anyprec.cu:294-359) followed
 * by torch.matmul -- without writing and re-reading the dense fp16 copy of W.  fp32 accumulation, one rounding to fp16.
 * bits 2..8, K % 64 == 0 (GQ_ENOTSUP otherwise: the caller keeps the dequant path); qweight may hold more planes than bits.
 * 2..4 bits decode in registers (v_perm byte pools of the row LUT, csrc/ap_gemm.hip); 5..8 bits keep the tile's row LUTs in LDS and
 * decode a weight tile per K stage there (csrc/ap_gemm_wide.hip).  Same argument checks, arithmetic and rounding at every width.
 */
int gq_anyprec_gemm(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t S, uint32_t N, uint32_t K,
                    int bits, void *stream);
/*
 * The same GEMM with a caller-supplied fp32 workspace for SHORT GRIDS (fewer 128 x 128 output tiles than compute units: a
 * prompt of <= 512 tokens on the 4096-row matrices): K is then split over up to 16 ranges, each block leaves fp32 partial sums
 * in the workspace and a second launch adds the ranges in order and rounds once to fp16 (results equal to gq_anyprec_gemm's up
 * to the fp32 summation order).  gq_anyprec_gemm_ws_bytes = the workspace this problem would use (0: no split planned);
 * a null / too small workspace runs the single pass.  workspace 16-byte aligned.  K is split at 2..4 bits only: at 5..8 bits
 * gq_anyprec_gemm_ws_bytes is 0 and gq_anyprec_gemm_ws runs the single pass whatever workspace it is given (as for bits outside
 * 2..8, where gq_anyprec_gemm_ws_bytes is 0 and the GEMM returns GQ_ENOTSUP).
 */
size_t gq_anyprec_gemm_ws_bytes(uint32_t S, uint32_t N, uint32_t K, int bits);
int gq_anyprec_gemm_ws(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t S, uint32_t N, uint32_t K,
                       int bits, void *workspace, size_t ws_bytes, void *stream);

/*
 * QTIP trellis decode to a dense fp16 matrix.  Replaces decode_compressed (qtip/lib/utils/kernel_decompress.py:5-55: index
 * decode, quantlut_sym lookup, m16n8k16 de-swizzle), bit for bit.
 *   W fp16 [M][K] (written), compressed int32 [R*M*K/32] (the packed trellis), codebook fp16 [512][2] (tlut).
 * R 2..4, M and K positive multiples of 32 (GQ_ENOTSUP else); pointers 4-byte aligned.
 */
int gq_qtip_decompress(void *W, const void *compressed, const void *codebook, uint32_t M, uint32_t K, int R, void *stream);
/*
 * QTIP prompt GEMM with the trellis decode fused into the matrix-core loop.
 *   out[s][m] = sum_k decode(compressed)[m][k] * x[s][k]     x fp16 [S][K], out fp32 [S][M] (written), S >= 1
 * Replaces bitshift_linear_kernel (qtip/lib/utils/kernel_decompress.py:82-91), the bs > 8 branch of BitshiftLinear.forward
 * (qtip/lib/codebook/bitshift.py:466-470): decode_compressed + torch.matmul -- without the dense fp16 copy of W.  Exact fp16
 * products, fp32 accumulation, NO fp16 rounding of the output (the reference rounds z to fp16 there; the matvec route keeps it
 * fp32, and this GEMM equals that route up to the fp32 summation order).  Serves every (M, K) gq_qtip_matvec serves: R 2..4,
 * M and K positive multiples of 32 (GQ_ENOTSUP else).  out and x 16-byte aligned, compressed and codebook 4-byte aligned.
 */
int gq_qtip_gemm(void *out, const void *compressed, const void *x, const void *codebook, uint32_t S, uint32_t M, uint32_t K, int R,
                 void *stream);
/*
 * The same GEMM with a caller-supplied fp32 workspace for SHORT GRIDS (fewer 128-row output tiles than compute units): K is then
 * split over up to 16 ranges, each range leaves fp32 partial sums in the workspace and a second launch adds the ranges in
 * ascending K order (deterministic; equal to gq_qtip_gemm's result up to the fp32 summation order).  gq_qtip_gemm_ws_bytes = the
 * workspace this problem would use (0: no split planned); a null / too small workspace runs the single pass.  workspace 16-byte
 * aligned.
 */
size_t gq_qtip_gemm_ws_bytes(uint32_t S, uint32_t M, uint32_t K, int R);
int gq_qtip_gemm_ws(void *out, const void *compressed, const void *x, const void *codebook, uint32_t S, uint32_t M, uint32_t K, int R,
                    void *workspace, size_t ws_bytes, void *stream);

/*
 * The element-wise steps of the prompt pass (seq_len > 1) between the prefill GEMMs, one launch each; fp16 rows, the fp16 rounding
 * points of the tensor expressions they replace (`Transformer.forward`, inference/model.py:206-266):
 *   gq_rmsnorm_rows     RMSNorm.forward (model.py:84-96) on S rows of D: (x.float() * rsqrt(mean(x^2) + eps)).half() * weight;
 *                       delta != NULL: the residual add in front of the norm rides along, x = x + delta (fp16, written back to x)
 *   gq_rope_cache_rows  apply_rotary_pos_emb (model.py:336-341) on the q and k parts of qkv [S][(n_head + 2 n_kv_head) head_dim],
 *                       rotated q -> q_out [n_head][S][head_dim], rotated k and v -> the caches [n_kv_head][max_seq][head_dim] at
 *                       pos[s] (KVCache.update, model.py:69-79; positions >= max_seq are not written)
 *   gq_silu_mul_rows    F.silu(gate) * up (model.py:266) of y [S][2 inter] -> out [S][inter]; paired != 0: (gate_i, up_i) adjacent
 *                       (the decode step's row order of the fused gate/up matrix), else gate = y[:, :inter], up = y[:, inter:]
 * All pointers 16-byte aligned device pointers; D, inter multiples of 8 (D <= 16384), head_dim a multiple of 16.
 * gq_rope_cache_rows, gq_qknorm_rope_cache_rows and gq_rope_cache_rows_kv8 (below) launch instances of ONE kernel
 * (csrc/prefill.hip: rope_cache_rows_kernel<QKN, QB, KV8>); each entry keeps its own checks.
 */
int gq_rmsnorm_rows(void *x, const void *delta, const void *weight, void *out, uint32_t S, uint32_t D, float eps, void *stream);
int gq_rope_cache_rows(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache, void *v_cache,
                       uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, void *stream);
/* gq_rope_cache_rows for Qwen3 layers, ONE launch: the RMSNorm over head_dim of every (row, head) of q and k (Qwen3RMSNorm's
 * rounding points, as gq_attn_decode_split_qknorm below; weights fp16 [head_dim]) in front of the rotation; v copied.  head_dim 64 or 128. */
int gq_qknorm_rope_cache_rows(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                              void *v_cache, uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                              const void *q_norm_weight, const void *k_norm_weight, float eps, void *stream);
int gq_silu_mul_rows(const void *y, void *out, uint32_t S, uint32_t inter, int paired, void *stream);

/*
 * The attention of the prompt pass (csrc/prefill_attn.hip): a flash-attention forward over one batch slot of the KV cache.
 *   q        fp16 [n_head][S][head_dim]           what gq_rope_cache_rows / gq_qknorm_rope_cache_rows write
 *   k_cache, v_cache  fp16 [n_kv_head][max_seq][head_dim], rows [0, start + S) written before the launch
 *   out      fp16 [S][n_head * head_dim]          the rows wo reads
 * Query row i has position p = start + i and attends the cache rows t <= p, with window != 0 also t > p - window (window 0: the
 * whole context).  start + S <= max_seq (GQ_EINVAL else); rows >= start + S of the caches may hold anything and are not read.
 * softmax(scale * q k^T) in fp32, P rounded to fp16 in front of P V at the scale 2^15 (a weight flushes to 0 only under 2^-40 of the
 * row's largest):  |out - exact| <= (2^-9 + (T / 32 + T / 64) 2^-24) max|V| over T = start + S keys.
 * gq_attn_prefill_supported (host logic, launches nothing): 1 for head_dim 64 / 128 and n_head a multiple of n_kv_head (any group
 * size), else 0 -- gq_attn_prefill then returns GQ_ENOTSUP and writes nothing.  All pointers 16-byte aligned.
 * Key tiles of GQ_PREFILL_ATTN_BK rows per block of GQ_PREFILL_ATTN_BQ query rows and one head; tiles wholly above the diagonal or
 * below the window are skipped, so a window layer costs S x window.
 */
#define GQ_PREFILL_ATTN_BQ 64
#define GQ_PREFILL_ATTN_BK 64
int gq_attn_prefill_supported(uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim);
int gq_attn_prefill(const void *q, const void *k_cache, const void *v_cache, void *out, uint32_t S, uint32_t start, uint32_t n_head,
                    uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t window, void *stream);

/*
 * The packed pass: N sequences as ONE run of S rows (varlen attention), fp16 caches.  Packed row i is token pos[i] of the sequence that
 * begins at packed row seg_begin[i]; its k and v live in cache row i.
 * gq_attn_prefill_packed: gq_attn_prefill with start = 0 (the same layouts, tile grid, softmax and store; a further instance of its
 *   kernel) and a segment begin per row: seg_begin int32 [S], device memory, non-decreasing, seg_begin[i] <= i.  Query row i attends
 *   the cache rows max(seg_begin[i], i + 1 - window) <= t <= i (window 0: no window).  The kernel uses min(seg_begin[i], i): a
 *   malformed array gives wrong numbers, never an address outside rows [0, S).  Row i of out is, bit for bit, row i of
 *   gq_attn_prefill(S = i + 1, start = 0, window = min(i - seg_begin[i] + 1, window)) over the same caches, and the cache rows of
 *   another sequence never reach it, whatever they hold (NaN and Inf included).  Governed by gq_attn_prefill_supported (GQ_ENOTSUP,
 *   nothing written); S == 0, S > max_seq and a null seg_begin: GQ_EINVAL.
 * gq_rope_cache_rows_packed: the row write with the cache row apart from the RoPE position: the rotation uses pos[s], k and v go to
 *   cache row row[s] (rows >= max_seq are not written), q_out [n_head][S][head_dim] is indexed by s.  q_norm_weight / k_norm_weight
 *   both given: the rounding points of gq_qknorm_rope_cache_rows (head_dim 64 or 128); neither: those of gq_rope_cache_rows; one
 *   of them: GQ_EINVAL.  A further instance of the row-write kernel.
 */
int gq_attn_prefill_packed(const void *q, const void *k_cache, const void *v_cache, const int *seg_begin, void *out, uint32_t S,
                           uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t window,
                           void *stream);
int gq_rope_cache_rows_packed(const void *qkv, const int *pos, const int *row, const void *cos_table, const void *sin_table, void *q_out,
                              void *k_cache, void *v_cache, uint32_t S, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim,
                              uint32_t max_seq, const void *q_norm_weight, const void *k_norm_weight, float eps, void *stream);

/*
 * The fp8 KV cache (kv_cache_dtype="fp8"): caches of OCP e4m3 codes, one byte per element, [n_kv_head][max_seq][head_dim] per batch
 * slot, with fp32 scales per KV head in device memory (read by the kernels at every launch: new values need no re-capture).
 *   write rule  code  = fp8_rne(clamp(float(x16) * inv, -448, 448)),  inv = 1 / scale computed by the host (no kernel divides);
 *               x16 is the fp16 value the fp16 path would have stored.  The only rounding the format adds.  Non-finite x16: +-Inf
 *               clamps to +-448 (0x7e / 0xfe); a NaN stores a NaN code (0x7f or 0xff), which every read turns into NaN output -- as an
 *               fp16 cache would show it.
 *   read rule   value = float(code) * scale.  Every e4m3 value is an fp16 value, so the conversion is exact: the K scale is one factor
 *               of the score (scale * k_scale[g]), the V scale multiplies the weighted sum in front of the division and the one fp16
 *               rounding.  With scales that are powers of two the results equal, bit for bit, those of the fp16 entries on an fp16
 *               cache that holds code * scale.
 * gq_rope_cache_rows_kv8: gq_rope_cache_rows for S >= 1 rows (the prompt pass, and the decode step with S = 1 and pos the graph's device
 *   word) into fp8 caches.  q_norm_weight / k_norm_weight (both or neither; eps): the rounding points of gq_qknorm_rope_cache_rows.
 *   qkv_bias (fp16 [(n_head + 2 n_kv_head) head_dim]): one fp16 add on q, k and v in front of the rotation, as gq_attn_decode_split_bias.
 *   Norm weights AND a bias: GQ_EINVAL.  q_out fp16 [n_head][S][head_dim], bit for bit what the fp16 entries write; a buffer of its
 *   own (never qkv).  k_inv / v_inv: fp32 [n_kv_head] reciprocal scales.  Positions >= max_seq are not written.  head_dim 64 or 128
 *   (GQ_ENOTSUP else, nothing written); all pointers 16-byte aligned.
 * gq_attn_decode_roped_kv8: gq_attn_decode_roped (window = 0) / gq_attn_decode_roped_window (window >= 1) over fp8 caches that hold
 *   every attended row, the current token's included (its dequantised value is what is attended: a result is a function of the cache
 *   alone).  The same geometry, solo rule, split length, stream assignment and merge order (csrc/attn_core.h); one 8-byte load per lane
 *   and row.  Partials reach the workspace multiplied by v_scale; the combine launch is the fp16 one.  *pos >= max_seq: NaN output.
 * gq_attn_prefill_kv8: gq_attn_prefill over fp8 caches; tiles are converted to fp16 between the global load and LDS, so the LDS image
 *   and both matrix products are those of gq_attn_prefill.  Governed by gq_attn_prefill_supported like it.
 */
int gq_rope_cache_rows_kv8(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *q_out, void *k_cache,
                           void *v_cache, const float *k_inv, const float *v_inv, uint32_t S, uint32_t n_head, uint32_t n_kv_head,
                           uint32_t head_dim, uint32_t max_seq, const void *q_norm_weight, const void *k_norm_weight, float eps,
                           const void *qkv_bias, void *stream);
int gq_attn_decode_roped_kv8(const void *q, const int *pos, const void *k_cache, const void *v_cache, const float *k_scale,
                             const float *v_scale, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                             float scale, uint32_t n_split, float *workspace, uint32_t window, void *stream);
int gq_attn_prefill_kv8(const void *q, const void *k_cache, const void *v_cache, const float *k_scale, const float *v_scale, void *out,
                        uint32_t S, uint32_t start, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale,
                        uint32_t window, void *stream);

/*
 * The scoring head of the prompt pass: per-token log-probabilities without the logits (csrc/head_nll.hip).  What the reference's
 * perplexity loop computes with the module tree and `labels=` (any_precision/evaluate/eval.py:205-226: lm_head logits [1, S, V] in
 * fp16, HF's loss upcasts them to fp32 and takes the cross entropy) from the rows behind the final RMSNorm, in one pass over the
 * vocabulary:
 *   xn fp16 [S][D], W fp16 [V][D] (output.weight as stored), target int [S]
 *   logit[s][v] = fp16(sum_k xn[s][k] W[v][k])     fp32 accumulation, ONE rounding: where the fp16 lm_head rounds
 *   lse[s]      = log sum_v exp(logit[s][v])       fp32
 *   logprob[s]  = logit[s][target[s]] - lse[s]     exactly 0.0f for a negative target ("ignored"); a target >= V is the caller's error
 *   top1[s]     = the lowest id among the largest fp16 logits
 * lse and top1 may be NULL.  Any S >= 1 and V >= 1 (odd V included: only whole rows of W are ragged); D % 64 == 0, else GQ_ENOTSUP.
 * The vocabulary is cut into `splits` ranges of whole 128-row tiles, one block per (128 sequence rows, range); splits == 0 lets the
 * library choose, splits >= 1 forces that many (a range without a tile contributes the neutral element).  The partials -- five words
 * per (row, range) -- go through `ws` (gq_head_nll_ws_bytes for the same S, V, D, splits; smaller: GQ_EINVAL; left as found otherwise)
 * and a second launch folds them in ascending range order: the results depend on `splits`, never on the run.
 */
size_t gq_head_nll_ws_bytes(uint32_t S, uint32_t V, uint32_t D, uint32_t splits);
int gq_head_nll(const void *xn, const void *W, const int *target, uint32_t S, uint32_t V, uint32_t D, float *logprob, float *lse,
                int *top1, uint32_t splits, void *ws, size_t ws_bytes, void *stream);

/*
 * Host (CPU) twins of the two Any-Precision entry points: same arguments with HOST pointers, no stream; `nthreads` <= 0
 * uses the OpenMP default.  They serve BASELINE.json configs[0] ("CPU reference APLinear path via generate.py"): the module
 * semantics of inference/APLinear.py:35-60 with the tensors in host memory (the reference hard-codes 'cuda',
 * APLinear.py:17,22,33, and has no CPU kernel).  Read the packed planes directly (pack.py:304-321).
 * gq_anyprec_gemv_cpu: exact fp16 x fp16 products, fp32 accumulation, one rounding to fp16:
 *     |out - exact| <= 2^-11 |exact| + 1e-5 * sum_k |w_k x_k|      (any M >= 1, bits 2..8, K % 32 == 0)
 * gq_anyprec_dequant_cpu: bit-exact table lookup, W fp16 [N][K].
 */
int gq_anyprec_gemv_cpu(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t M, uint32_t N,
                        uint32_t K, int bits, int dtype, int nthreads);
int gq_anyprec_dequant_cpu(const uint32_t *qweight, const void *lut, void *W, uint32_t N, uint32_t K, int bits,
                           int nthreads);

/*
 * LUT-GEMM (BCQ) GEMV.  Replaces ap_gemv.lutgemm_gemv -> nqmv_bias
 * (bindings.cpp:16, gemv.cu:140-228, lutgemm.cu:24-149).
 *   x fp16 [K], out fp16 [N] (ACCUMULATED INTO, caller zeroes it as LUTGEMMLinear.py:74 does),
 *   qweight u32 [K/32][bits][N], alpha fp16 [K/group][bits][N], q_bias fp16 [K/group][N].
 */
int gq_lutgemm_gemv(const void *x, void *out, const uint32_t *qweight, const void *alpha, const void *q_bias,
                    uint32_t N, uint32_t K, int bits, int group_size, void *stream);
/* Same result (bit for bit), two launches: the 4 x 256 sign-sum tables of every 32-activation tile depend only on x, so
 * they are built once per call into `workspace` (64 bytes per input feature, 16-byte aligned, caller-owned scratch) and
 * the GEMV blocks copy them to LDS instead of rebuilding them 64..448 times. */
int gq_lutgemm_gemv_ws(const void *x, void *out, const uint32_t *qweight, const void *alpha, const void *q_bias,
                       uint32_t N, uint32_t K, int bits, int group_size, void *workspace, uint64_t workspace_bytes,
                       void *stream);

/*
 * QTIP trellis-decoded matvec.  out[m] = sum_k decode(compressed)[m][k] * x[k]
 * Replaces qtip_kernels.decompress_matvec_16_9_{R}_1_{M}_1_{K} -> kernel_decompress_matvec
 * (qtip/qtip-kernels/src/wrapper.cpp:557-645, qtip_torch.cu:14-57, inference.cu:168-471).
 *   out f32 [M], compressed u32 [R*M*K/32], x fp16 [K], codebook fp16 [1024] (tlut [512][2]).
 * One runtime-shaped entry point serves all 73 compile-time shapes of the reference.
 */
int gq_qtip_matvec(float *out, const uint32_t *compressed, const void *x, const void *codebook, uint32_t M,
                   uint32_t K, int R, void *stream);

/*
 * Hadamard transform on the last dim, y = scale * x @ H_n (Sylvester order), n a power of two.
 * Replaces hadamard::hadamard -> fast_hadamard_transform.hadamard_transform
 * (inference/lib/utils/matmul_had.py:96-106).  x,y f32 [rows][n]; in-place allowed.
 */
int gq_hadamard(const float *x, float *y, uint32_t rows, uint32_t n, float scale, void *stream);

/*
 * Fused QTIP linear for one decode row (bs = 1), in two launches.  Replaces the op sequence of
 * BitshiftLinear.forward (inference/lib/codebook/bitshift.py:415-472, eval mode, rcp == 0) around
 * decompress_matvec: x.float() * SU -> hadamard * n^-1/2 / 32 -> .half() -> matvec [gq_qtip_linear_in], then
 * hadamard * m^-1/2 -> * (SV * 32) -> .half() [gq_qtip_linear_out], with the decode step's own element-wise ops
 * folded in: the RMSNorm in front of q/k/v and gate/up (inference/model.py:281-292), silu(gate) * up in front of the
 * down projection (model.py:266), the residual add behind wo / w2 (model.py:311-313).  Up to 3 linears that share the
 * input (q/k/v; gate/up) go in one launch.  K and every M must be powers of two (the reference's non-power-of-two
 * Hadamard factors are data tables this library does not carry: those models run the unfused ops).
 * Same arithmetic and the same butterfly order as gq_hadamard + gq_qtip_matvec: bit-identical to the unfused chain.
 *   x fp16 [K] (prologue SILU_MUL: x = gate, x2 = up), norm_weight fp16 [K];
 *   GqQtipIn : trellis u32 [R*M*K/32], SU f32 [K], tlut fp16 [1024], y32 f32 [M] (written);
 *   GqQtipOut: y32 f32 [M], SV32 f32 [M] (= SV * 32), resid fp16 [M] or NULL, out fp16 [M] (may alias resid).
 * ksplit = 1..4: K ranges per 32-row band; range s of a band writes its partial sums to y32[s M .. (s + 1) M) (y32 must
 * hold ksplit * M floats; gq_qtip_linear_out with parts = ksplit adds them in ascending order).  A launch runs at most one
 * block per compute unit; every block serves ONE linear and walks that linear's (band, K range) items, so a split evens
 * out launches whose band count is not a multiple of the block count (q/k/v: 3 x 128 bands on 256 units -> ksplit 3).
 * gq_qtip_plan_ksplit(n, M[], K, max) returns the split with the fewest band-equivalents per block for this device.
 * Folding: with n_prev = 1 (2 for SILU_MUL) the input vector(s) of gq_qtip_linear_in are NOT read from x / x2 but rebuilt
 * from prev[] -- the transform-out of the linear(s) that produce them (M == K), residual included -- by every block, and
 * stored to prev[i].out (if not NULL; must not alias prev[i].resid) once: gq_qtip_linear_out and its launch are saved for
 * wo -> gate/up, gate/up -> down and down -> next layer's q/k/v.  Bit-identical to the two-launch form.
 */
#define GQ_QPRO_NONE 0
#define GQ_QPRO_RMSNORM 1
#define GQ_QPRO_SILU_MUL 2
#define GQ_QPRO_PRETRANSFORMED 3 /* x is the fp16 output of gq_qtip_transform(input_side): matvec only, any K % 32 == 0 */
typedef struct GqQtipIn {
    const uint32_t *trellis;
    const float *SU;
    const void *tlut;
    float *y32;
    uint32_t M;
} GqQtipIn;
typedef struct GqQtipOut {
    const float *y32;
    const float *SV32;
    const void *resid;
    void *out;
    uint32_t M;
    uint32_t parts; /* 0 / 1: y32 is [M]; 2..4: y32 is [parts][M] split-K partial sums (ksplit of gq_qtip_linear_in) */
} GqQtipOut;
int gq_qtip_linear_in(const void *x, const void *x2, const void *norm_weight, float eps, int prologue, uint32_t K, int R,
                      int n, const GqQtipIn *lin, int n_prev, const GqQtipOut *prev, int ksplit, void *stream);
int gq_qtip_linear_out(int n, const GqQtipOut *lin, void *stream);
/* The same transform-out spread over M / 128 blocks per linear: block s combines the M / 128 segments of the sums with the signs
 * of row s of the Sylvester matrix and runs one 128-point transform (H_M = H_(M/128) (x) H_128).  Equal to gq_qtip_linear_out up to
 * fp32 rounding (the additions of the full transform in another order), 2.9 instead of 4.6 us per launch in the decode step.
 * M a power of two in 128..8192, sums 16-byte aligned (GQ_ENOTSUP / GQ_EINVAL else). */
int gq_qtip_linear_out_seg(int n, const GqQtipOut *lin, void *stream);
/* Round 5: gq_qtip_linear_out of ONE linear (o or down; residual added, prev->out written once) FOLLOWED IN THE SAME LAUNCH by the
 * transform-in of the n_next <= 3 linears that read its output through an RMSNorm (gate / up; the next layer's q / k / v): block j
 * leaves xt_next[j] = half(H(RMSNorm(out) * SU_next[j]) * K^-1/2 / 32), fp16 [K] -- the vector gq_qtip_linear_in's RMSNorm prologue
 * would build in every one of its blocks (BitshiftLinear.forward, inference/lib/codebook/bitshift.py:441-447; RMSNorm of
 * inference/model.py:281-292).  The matvec launch then runs with GQ_QPRO_PRETRANSFORMED and x == NULL: every GqQtipIn.SU field
 * points to ITS pre-transformed vector.  K = prev->M a power of two in 256..8192. */
int gq_qtip_linear_out_in(const GqQtipOut *prev, const void *norm_weight, float eps, int n_next, const float *const *SU_next,
                          void *const *xt_next, void *stream);
int gq_qtip_plan_ksplit(int n, const uint32_t *M, uint32_t K, int max_ksplit); /* host-side helper, launches nothing */
/*
 * gq_qtip_linear_in + gq_qtip_linear_out in ONE launch: the block that finishes a linear LAST (a device-scope counter per
 * linear; no block waits for another one) also runs that linear's transform-out -- the same code as gq_qtip_linear_out, so the
 * results are bit-identical to the two-launch form.  finish[i] describes the output side of lin[i] (its y32 / parts fields are
 * ignored: the launch's own sums and ksplit are used); every M a power of two <= 16384.  counters: u32 [n] in device memory,
 * zero before the first call (the finishing block resets its counter; one array per stream of launches).
 */
int gq_qtip_linear(const void *x, const void *x2, const void *norm_weight, float eps, int prologue, uint32_t K, int R, int n,
                   const GqQtipIn *lin, const GqQtipOut *finish, int ksplit, void *counters, void *stream);

/*
 * Either side of a QTIP linear whose width n = Kf * P carries a non-power-of-two Hadamard factor (inference/lib/utils/
 * matmul_had.py:13-94; Llama-2's MLP width 11008 = 172 * 64): P-point Sylvester transform of every row of the [Kf][P]
 * view, then hadK @ rows (transpose != 0: hadK^T @, matmul_hadUt).  Such a linear runs transform -> gq_qtip_matvec ->
 * transform (the Kf x Kf product is too much to repeat in every block of the fused kernel).
 *   input_side != 0:  out fp16 [n] = half(H(pro(x) * vec) * n^-1/2 / 32),  vec = SU f32 [n], pro as GQ_QPRO_* (x2 / norm_weight)
 *   input_side == 0:  out fp16 [n] = half(H(y32) * n^-1/2 * vec) (+ resid),  vec = SV * 32 f32 [n]
 * Up to 3 linears per launch (same n, Kf; input side: same x, their own SU / table / out).
 * hadK f32 [Kf][Kf] is the caller's table (the reference's data, not shipped here); P a power of two >= 64.
 */
typedef struct GqQtipXf {
    const float *y32;   /* input_side == 0 */
    const float *vec;
    const float *hadK;
    const void *resid;  /* fp16 [n] or NULL */
    void *out;          /* fp16 [n] */
} GqQtipXf;
int gq_qtip_transform(int input_side, const void *x, const void *x2, const void *norm_weight, float eps, int prologue,
                      int n_lin, const GqQtipXf *lin, uint32_t n, uint32_t Kf, int transpose, void *stream);

/*
 * The middle of a gated MLP whose width n = Kf * 64 carries a Hadamard factor (Llama-2-7b: 11008 = 172 * 64), in ONE launch:
 * transform-out of gate and up (bitshift.py:466-470), silu(gate) * up (model.py:266), * SU of down and the FACTOR side of
 * down's transform-in (bitshift.py:441, matmul_had.py:69-94) -- what two gq_qtip_transform launches (output side for gate / up,
 * then input side with GQ_QPRO_SILU_MUL) do, except that the 64-point row transforms of the input side are left to the
 * consumer: z32 [n] (fp32) goes to gq_qtip_linear_in_rows, which runs them in its prologue.  hadK (x) H_64 acts on the two sides
 * of the [Kf][64] view, so the order of the sides is free: gate / up are computed in gq_qtip_transform's order (bit-identical
 * fp16 values; stored to gate_out / up_out when non-NULL), the input side in the other order (equal to the two-launch chain
 * up to fp32 rounding).
 *   hadT_right16    fp16 [Kf][Kf]: the right-side table of gate / up TRANSPOSED (hadT[k][r] = had_right[r][k]; both projections
 *                   have width n, hence the same table -- matmul_had.py get_hadK(n))
 *   had_left_down16 fp16 [Kf][Kf]: the left-side table of down as stored (the input side multiplies with its transpose)
 * The tables are passed in fp16 (every block reads both of them): their entries must be fp16 values -- a Hadamard factor's +-1 are,
 * and with +-1 entries every product is exact and the results are those of the fp32 tables; the caller checks its table.
 * parts: split-K parts of y32_gate / y32_up ([parts][n], added in ascending order).  Kf <= 176, Kf % 4 == 0.
 */
typedef struct GqQtipMid {
    const float *y32_gate, *y32_up;
    const float *SV32_gate, *SV32_up; /* SV * 32, f32 [n] */
    const void *hadT_right16;
    const float *SU_down;             /* f32 [n] */
    const void *had_left_down16;
    float *z32;                       /* out: f32 [n] */
    void *gate_out, *up_out;          /* fp16 [n] or NULL */
} GqQtipMid;
int gq_qtip_mlp_mid(const GqQtipMid *m, uint32_t parts, uint32_t n, uint32_t Kf, void *stream);
/*
 * gq_qtip_linear_in for an input whose transform-in lacks only the row transforms: x = z32 (f32 [K], K = Kf * P, from
 * gq_qtip_mlp_mid) -> P-point Sylvester transform of every row -> * K^-1/2 / 32 -> fp16 -> trellis matvec into lin[i].y32
 * (lin[i].SU is ignored).  Other arguments as gq_qtip_linear_in.
 */
int gq_qtip_linear_in_rows(const float *z32, uint32_t K, uint32_t P, int R, int n, const GqQtipIn *lin, int ksplit, void *stream);

/*
 * Single-query attention of a QTIP model with the transform-out of its q, k and v linears folded in: qkv_lin[0..2] are the
 * descriptors gq_qtip_linear_out would take (y32 sums, SV32, M, parts; resid / out are ignored), every other argument as in
 * gq_attn_decode_split (declared below).  Each head rebuilds its head_dim outputs of q (its KV group's of k and v): the
 * M / head_dim segments of the sums combined with the signs of the head's row of the Sylvester matrix, then one
 * head_dim-point transform, * M^-1/2 * SV32 -> fp16 (inference/lib/codebook/bitshift.py:470, inference/model.py:206-241).
 * The additions of the full transform in another order: equal to gq_qtip_linear_out + gq_attn_decode_split up to fp32
 * rounding (not bit for bit), one launch per layer less.  M[0] = n_head * head_dim, M[1] = M[2] = n_kv_head * head_dim,
 * powers of two (GQ_ENOTSUP else).
 */
int gq_attn_decode_qtip(const GqQtipOut *qkv_lin, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                        void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                        float scale, uint32_t n_split, float *workspace, void *stream);

/*
 * Fused decode-step variant of the AP GEMV, M = 1: optional prologue on x
 * (RMSNorm, or SiLU(gate)*up of a fused gate/up vector) and optional residual-add epilogue, with the same
 * fp16 rounding points as the reference's separate kernels (inference/model.py:151-166,259-266,281-292).
 *   norm_weight  fp16 [K] or NULL (no RMSNorm);  eps used when norm_weight != NULL
 *   flags        GQ_EPI_RESIDUAL: out[n] = residual[n] + y[n]
 *                GQ_PRO_SILU_MUL: x is fp16 [2K]; the GEMV input is silu(x[0:K]) * x[K:2K]
 *                GQ_EPI_SILU_PAIRS: qweight / lut rows are interleaved gate/up pairs (the caller permuted the fused
 *                                 [w1; w3] tensor, model.py:259-266): out fp16 [N/2], out[i] = silu(y[2i]) * y[2i+1];
 *                                 exclusive with GQ_EPI_RESIDUAL; N even
 */
int gq_anyprec_gemv_fused(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                          uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                          uint32_t epilogue, void *stream);
/*
 * The same with a caller-supplied workspace (device memory, 16-byte aligned, private to the stream of launches that use it):
 * rows wider than 16384 activations (Llama-3 70B's down projection, K = 28672) are then split along K over BLOCKS -- fp32 sums
 * per K slice in the workspace, a second launch adds the slices in ascending order and rounds ONCE (anyprec.cu:505-512) --
 * instead of over two launches through the fp16 output (two roundings).  gq_anyprec_gemv_fused_ws_bytes: the bytes this shape
 * wants (0: no workspace form; the call then equals gq_anyprec_gemv_fused).  workspace NULL or too small: gq_anyprec_gemv_fused.
 */
size_t gq_anyprec_gemv_fused_ws_bytes(uint32_t N, uint32_t K, int bits, uint32_t epilogue);
int gq_anyprec_gemv_fused_ws(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                             uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                             uint32_t epilogue, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Round 5: statistics hand-over between the launches of a decode step.  The hidden state an RMSNorm prologue normalises was written
 * by the previous launch (the residual epilogue of wo / w2, or the embedding lookup): that launch leaves the partial sums of squares
 * of the fp16 values it stored next to them, and the consumer adds GQ_SSQ_SLOTS floats instead of exchanging per-wave sums through
 * LDS behind a counter between the activations' arrival and the normalisation (reference rounding points unchanged:
 * inference/model.py:281-292 -- fp32 mean of squares, rsqrt, fp16 rounding, fp16 multiply; only the fp32 summation ORDER differs,
 * as it already did from torch's).
 *   ssq_out  float [GQ_SSQ_SLOTS], 16-byte aligned, or NULL: the launch writes ALL slots (partial sums of squares of its fp16 outputs;
 *            their total is the vector's sum of squares).  Plain / residual epilogue only.  Kernels without the in-epilogue form are
 *            followed by one small launch (gq_ssq_rows) -- the result is there either way.
 *   ssq_in   the slots written by the launch that produced x (the caller's contract), or NULL.  Used by the RMSNorm prologues that
 *            have the hand-over form (the stream kernel, csrc/ap_stream.hip); ignored elsewhere.  GQ_SSQ_HANDOVER=0 ignores it.
 * gq_anyprec_gemv_fused_ho = gq_anyprec_gemv_fused_ws + the two pointers; gq_anyprec_gemv_qkv_rope_ho, gq_embed_lookup_ho likewise
 * (declared below); gq_ssq_rows: the statistics of any fp16 vector.
 */
#define GQ_SSQ_SLOTS 1024
int gq_anyprec_gemv_fused_ho(const void *x, void *out, const uint32_t *qweight, const void *lut, uint32_t N,
                             uint32_t K, int bits, const void *norm_weight, float eps, const void *residual,
                             uint32_t epilogue, void *workspace, size_t workspace_bytes, const float *ssq_in, float *ssq_out,
                             void *stream);
int gq_ssq_rows(const void *x, uint32_t n, float *ssq_out, void *stream);
/* Plan: which form the launch gq_anyprec_gemv_fused_ho(N, K, bits, norm_weight != NULL, epilogue) would take under the current mode /
 * environment -- bit 0: its RMSNorm prologue reads ssq_in; bit 1: its epilogue writes ssq_out itself (no extra launch).  A decode step
 * passes the pointers only where both ends of an edge are free (guidedquant_amd/model.py::native_layers). */
int gq_anyprec_handover_plan(uint32_t N, uint32_t K, int bits, int has_norm, uint32_t epilogue);

/*
 * The non-quantized pieces of one bs=1 decode step (inference/model.py:121-130,151-166,206-241).  Token id and
 * position are read from DEVICE memory so a captured hipGraph can be replayed per token.
 */
/* x = tok_embeddings[token]                    table fp16 [vocab][dim], out fp16 [dim] */
int gq_embed_lookup(const int *token, const void *table, void *out, uint32_t dim, uint32_t vocab, void *stream);
int gq_embed_lookup_ho(const int *token, const void *table, void *out, uint32_t dim, uint32_t vocab, float *ssq_out, void *stream);

/* RoPE(q,k) at *pos, KV-cache update at *pos, softmax(q k^T / sqrt(d)) v over positions 0..*pos.
 * *pos >= max_seq (decoding past the cache): nothing is written to the caches and `out` is filled with NaN, so the step's
 * logits are NaN -- a loud failure instead of silently overwriting the last slot.
 *   qkv fp16 [(n_head + 2 n_kv_head) * head_dim] (fused wqkv output: q | k | v, model.py:211)
 *   cos/sin fp16 [max_seq][head_dim] (LlamaRotaryEmbedding tables, model.py:379-405)
 *   k_cache, v_cache fp16 [n_kv_head][max_seq][head_dim] (KVCache, model.py:63-79);  out fp16 [n_head * head_dim] */
int gq_attn_decode(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                   void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                   float scale, void *stream);
/* Split-KV form for long contexts: n_split blocks per head, each over a contiguous range of the cached positions (whole
 * passes of 128 positions at head_dim 128), partial (max, sum, weighted V) results in `workspace` (f32
 * [n_head][n_split][head_dim + 2]) combined by a second small launch.  One block per head keeps only n_head CUs
 * streaming the cache: 51 us per layer at 4096 positions.  n_split = 1 is gq_attn_decode (no workspace, one launch).
 * n_split in 1..64, for every form below as well.  Splits beyond the context are legal: a split whose range starts behind *pos
 * writes a neutral partial result (max -3e38, sum 0, weighted V 0) that adds exactly nothing in the combine; a context of at most
 * two passes is finished by one block per head and the workspace is neither written nor read. */
int gq_attn_decode_split(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                         void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                         float scale, uint32_t n_split, float *workspace, void *stream);
/* Qwen3 layers: gq_attn_decode_split with the per-head RMSNorm of q and k in front of the rotation, inside the same launch.
 * Restates transformers' modeling_qwen3.Qwen3Attention.forward (q_norm / k_norm on q and k viewed as [.., heads, head_dim], then
 * apply_rotary_pos_emb) with Qwen3RMSNorm's rounding points: sum of squares of a head's head_dim fp16 values in fp32,
 * (x * rsqrt(ssq / head_dim + eps)) rounded to fp16, then the fp16 product with the weight.  v is untouched; the cache receives
 * the normalised, rotated k.  q_norm_weight, k_norm_weight: fp16 [head_dim], shared by all heads.  head_dim 64 or 128; n_split,
 * workspace and the NaN result at *pos >= max_seq as gq_attn_decode_split.  (The reference has no Qwen3 attention of its own:
 * any_precision/analyzer/splitted_models/qwen3.py subclasses transformers' Qwen3Model.) */
int gq_attn_decode_split_qknorm(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                float scale, uint32_t n_split, float *workspace, const void *q_norm_weight, const void *k_norm_weight,
                                float eps, void *stream);
/* Qwen2 / Qwen2.5 layers: gq_attn_decode_split with the bias of the q / k / v linears added in front of the rotation, inside the
 * same launch.  Restates the bias add of the quantized linears (any_precision/modules/AnyPrecisionLinear.py: the GEMV result rounded
 * to fp16, then `output += bias`, ONE fp16 add) for transformers' modeling_qwen2.Qwen2Attention (q_proj / k_proj / v_proj with
 * bias=True, o_proj without): fp16(q[d]) + fp16(bias[d]) for every q, k and v element, then the rotation of q and k; the cache
 * receives the biased, rotated k and the biased v.  Bit-identical to gq_attn_decode_split on a vector the bias was added to in fp16.
 * qkv_bias: fp16 [(n_head + 2 n_kv_head) * head_dim], laid out like the packed q | k | v vector, 16-byte aligned.  head_dim 64 or
 * 128; n_split, workspace and the NaN result at *pos >= max_seq as gq_attn_decode_split. */
int gq_attn_decode_split_bias(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                              void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                              float scale, uint32_t n_split, float *workspace, const void *qkv_bias, void *stream);
/* Sliding-window layers (Mistral; Qwen2 / Qwen3 with use_sliding_window; transformers' masking_utils.sliding_window_overlay on top of the
 * causal mask): the query at *pos attends the cached rows t with *pos - window < t <= *pos -- lo = *pos + 1 > window ? *pos + 1 - window
 * : 0, n = *pos + 1 - lo rows, and no row outside [lo, *pos] reaches a score or a weighted sum (rows below lo hold real rows of the
 * sequence, rows above *pos stale ones).  The caches stay as they are: max_seq rows, row *pos written at *pos.  The geometry is that of
 * the launch without a window at position n - 1, shifted by lo: one block per head while n is at most two passes (the rule is taken on
 * n, in the attention launch and in the combine alike), split s over [lo + s per, ..) with per from n, row t in the slot of row t - lo --
 * bit for bit the old entry on a cache that holds rows [lo, *pos] as rows [0, n - 1].  window = 0 is GQ_EINVAL; window >= max_seq is
 * legal and equals the entry without a window bit for bit.  Every other argument, the NaN result at *pos >= max_seq and the workspace as
 * in the entry of the same name.  gq_attn_decode_roped_window: the rows requested ahead of the position serve only while lo = 0.
 * (gq_attn_decode_qtip and gq_anyprec_gemv_qkv_rope_attn have no window form.) */
int gq_attn_decode_split_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                float scale, uint32_t n_split, float *workspace, uint32_t window, void *stream);
int gq_attn_decode_split_qknorm_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                       void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                       float scale, uint32_t n_split, float *workspace, const void *q_norm_weight,
                                       const void *k_norm_weight, float eps, uint32_t window, void *stream);
int gq_attn_decode_split_bias_window(const void *qkv, const int *pos, const void *cos_table, const void *sin_table, void *k_cache,
                                     void *v_cache, void *out, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                     float scale, uint32_t n_split, float *workspace, const void *qkv_bias, uint32_t window, void *stream);

/*
 * Device-to-device hand-over of the layer pipeline (round 4; reference precedent: the host-side `.to(device)` hops of
 * qtip/lib/utils/shard_model.py:44-68).  gq_hop_send: copy `nbytes` (multiple of 16) from src into dst_remote -- memory of the
 * next stage, mapped into this process (hipIpc / torch's CUDA IPC; same GPU or a peer over xGMI) -- with system-scope stores, then
 * store *seq_remote = *tick + add behind them.  gq_hop_wait: spin (one wave, bounded: max_spins polls of ~1 us, 0 = 2^21) until
 * *seq_local >= *tick + add; on expiry *err = 1 and the launch returns (the GPU never hangs on a missing peer).  `tick` is a word
 * in device memory the caller's graph increments per tick.
 */
int gq_hop_send(const void *src, void *dst_remote, uint32_t nbytes, uint32_t *seq_remote, const uint32_t *tick, uint32_t add, void *stream);
int gq_hop_wait(const uint32_t *seq_local, const uint32_t *tick, uint32_t add, uint32_t *err, uint32_t max_spins, void *stream);
/* Round 5: what a PEER writes -- landing slots and sequence words -- lives in FINE-GRAINED device memory (ordinary
 * allocations are coarse-grained: a peer GPU's writes are not guaranteed visible to kernels running here).  gq_hop_alloc: zeroed
 * fine-grained memory of the current device; gq_hop_export / gq_hop_import: a 64-byte hipIpc handle of it / the mapping in another
 * process; gq_hop_close, gq_hop_free.  gq_hop_wait_copy = gq_hop_wait, then the payload is copied out of the landing slot with
 * system-scope loads into `dst`, the ordinary buffer the stage's kernels read: no kernel but these two touches peer-written memory. */
int gq_hop_alloc(size_t bytes, void **ptr);
int gq_hop_free(void *ptr);
int gq_hop_export(void *ptr, void *handle64);
int gq_hop_import(const void *handle64, void **ptr);
int gq_hop_close(void *ptr);
/* 1 when `ptr` lies in memory THIS process allocated fine-grained (hipPointerGetAttributes: allocationFlags has
 * hipDeviceMallocFinegrained), 0 when not, < 0 on error -- what pipeline.py / tp.py assert of their landing buffers before a
 * rank on another device is given the handle. */
int gq_hop_is_finegrained(const void *ptr);
int gq_hop_wait_copy(const uint32_t *seq_local, const uint32_t *tick, uint32_t add, uint32_t *err, uint32_t max_spins, const void *landed,
                     void *dst, uint32_t nbytes, void *stream);

/* One-time device self-check of a hardware behaviour the plane / QTIP kernels rest on (an LDS read beyond the workgroup's
 * allocation returns zeros: the idle MFMA columns take their zeros from there).  GQ_OK, or GQ_ENOTSUP with the rebuild flags in
 * gq_last_error().  The Python binding calls it once per process on a GPU box. */
int gq_selfcheck(void);
/* Measurement aid: one launch that only reads `bytes` of `buf` once (the one-shot streaming floor bench.py prices the GEMV launches
 * against: `frac_of_stream_floor`).  sink: one device word (never written in practice). */
int gq_debug_stream_read(const void *buf, size_t bytes, uint32_t *sink, void *stream);

/*
 * Round 4: RoPE and the KV-cache write in the EPILOGUE of the fused q / k / v projection, attention without them.
 *
 * gq_anyprec_gemv_qkv_rope = RMSNorm -> Any-Precision GEMV of the fused wqkv tensor (reference row order q | k | v, model.py:211;
 * nothing is permuted in memory: the kernel picks its 16-row groups so that a lane owns both rotation partners d, d + head_dim / 2)
 * -> apply_rotary_pos_emb on the fp16 outputs (model.py:330-341: three fp16-rounded operations, fp16 cos / sin tables) ->
 *   q_out fp16 [n_head * head_dim] rotated queries;  k_cache[g][*pos][:] rotated keys;  v_cache[g][*pos][:] values
 * (KVCache.update, model.py:69-79).  *pos >= max_seq writes nothing to the caches.  Replaces gq_anyprec_gemv_fused(wqkv) + the
 * rotation / cache write inside gq_attn_decode_split; results are bit-identical to that chain (same GEMV arithmetic, same fp16
 * rounding points).  gq_anyprec_qkv_rope_supported: 1 when this build serves (N, K, bits, head_dim) -- the caller keeps the
 * two-launch form otherwise (GQ_ENOTSUP).
 * gq_attn_decode_roped: single-query attention over positions 0..*pos of the caches for queries that are already rotated; the first
 * batch of cached rows is requested together with q and the position (one memory round trip); arguments as gq_attn_decode_split. */
int gq_anyprec_qkv_rope_supported(uint32_t N, uint32_t K, int bits, uint32_t head_dim);
int gq_anyprec_gemv_qkv_rope(const void *x, void *q_out, const uint32_t *qweight, const void *lut, uint32_t N, uint32_t K, int bits,
                             const void *norm_weight, float eps, const int *pos, const void *cos_table, const void *sin_table,
                             void *k_cache, void *v_cache, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                             void *stream);
int gq_anyprec_gemv_qkv_rope_ho(const void *x, void *q_out, const uint32_t *qweight, const void *lut, uint32_t N, uint32_t K, int bits,
                                const void *norm_weight, float eps, const int *pos, const void *cos_table, const void *sin_table,
                                void *k_cache, void *v_cache, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                const float *ssq_in, void *stream);
int gq_attn_decode_roped(const void *q, const int *pos, const void *k_cache, const void *v_cache, void *out, uint32_t n_head,
                         uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split, float *workspace,
                         void *stream);
int gq_attn_decode_roped_window(const void *q, const int *pos, const void *k_cache, const void *v_cache, void *out, uint32_t n_head,
                                uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq, float scale, uint32_t n_split, float *workspace,
                                uint32_t window, void *stream);

/*
 * Round 6: gq_anyprec_gemv_qkv_rope AND gq_attn_decode_roped (n_split = 1) as ONE launch -- the attention heads are extra blocks of the
 * wqkv launch, on compute units the GEMV leaves idle; they fetch the position and the cached rows below it while the GEMV runs and
 * wait on device flags for the rotated q and row *pos of the caches (csrc/ap_stream.hip::ap_qkv_attn_kernel: agent-scope stores /
 * atomics / loads, a bounded poll -- on expiry the head's output is NaN, nothing hangs).  Replaces the two launches
 * (inference/model.py:206-241 between `self.wqkv(x)` and `self.wo(y)`); q_out, the caches and attn_out are bit-identical to theirs.
 *   attn_out  fp16 [n_head * head_dim]: softmax(q k^T * scale) v over positions 0..*pos (*pos >= max_seq: NaN, like the two launches)
 *   flags     uint32 [n_head * GQ_ATTN_FLAG_STRIDE], 128-byte aligned, ZERO before the first launch; every launch leaves them zero
 *             (one 128-byte line per head: agent-scope atomics on one line serialise at the memory side).  One buffer serves every
 *             layer of a model (the launches of a stream are ordered).
 * gq_anyprec_qkv_rope_attn_supported: 1 when this build serves the geometry that way (the fused wqkv launch is served, its grid +
 * n_head blocks fit the device's compute units one each, AND the environment asks for it: GQ_QKV_ATTN=1 -- the form is OFF by default,
 * measured no faster than the two launches, profiles/r06_attention_in_wqkv_launch.txt); the caller keeps the two launches otherwise.
 */
#define GQ_ATTN_FLAG_STRIDE 32
int gq_anyprec_qkv_rope_attn_supported(uint32_t N, uint32_t K, int bits, uint32_t head_dim, uint32_t n_head, uint32_t n_kv_head);
int gq_anyprec_gemv_qkv_rope_attn(const void *x, void *q_out, const uint32_t *qweight, const void *lut, uint32_t N, uint32_t K, int bits,
                                  const void *norm_weight, float eps, const int *pos, const void *cos_table, const void *sin_table,
                                  void *k_cache, void *v_cache, uint32_t n_head, uint32_t n_kv_head, uint32_t head_dim, uint32_t max_seq,
                                  void *attn_out, float scale, uint32_t *flags, void *stream);

/* out[n] = sum_k rmsnorm?(x)[k] * W[n][k]      dense fp16 GEMV (lm_head `output`, model.py:94,128-129); fp32
 * accumulation, fp16 output; norm_weight == NULL skips the RMSNorm prologue.  K % 512 == 0. */
int gq_dense_gemv_f16(const void *x, const void *W, void *out, uint32_t N, uint32_t K, const void *norm_weight, float eps,
                      void *stream);

/* out[n] = fp16( scale[n] * sum_k rmsnorm?(x)[k] * Wq[n][k] )      the opt-in int8 lm_head (csrc/head_q8.hip): weight-only, one fp32
 * scale per output row (guidedquant_amd/head_q8.py::quantize_rows_int8 makes Wq and scale from an fp16 head).
 *   x, norm_weight, eps, out   what they are in gq_dense_gemv_f16; the RMSNorm prologue is that entry's own text, with its rounding points
 *                              (the statistic in fp32, x * scale rounded to fp16, the fp16 product with the weight)
 *   Wq      int8 [N][K], row-major, 16-byte aligned; every code is turned into its signed fp16 value before the product
 *   scale   fp32 [N], 4-byte aligned; the fp32 sum of a row is multiplied by it (one fp32 rounding), then rounded to fp16
 * K % 512 == 0 and the fp16 activations in LDS as in gq_dense_gemv_f16 (K <= 81408); anything else, a null or a misaligned pointer:
 * GQ_EINVAL / GQ_ENOTSUP, nothing launched.  Rows past N are never written, no byte outside Wq[0 .. N*K) or scale[0 .. N) is read.
 * Plan: GQ_DENSE_I8_BPC blocks per compute unit (default 3), GQ_DENSE_I8_RPB rows per block (a multiple of 16) instead. */
int gq_dense_gemv_i8(const void *x, const void *Wq, const float *scale, void *out, uint32_t N, uint32_t K, const void *norm_weight, float eps,
                     void *stream);

/* Top-k sampling with the reference's distribution (inference/generate.py:53-73: logits / max(T,1e-5), top-k, softmax,
 * exponential-race draw).  work_val / work_idx: 128*32 floats / ints of scratch; counter: one int of RNG state in
 * device memory (incremented per call).  If tok_io / pos_io are non-NULL the sampled token is written to *tok_io and
 * *pos_io is incremented, so a captured decode graph advances by itself.  top_k <= 32.
 * vocab <= GQ_SAMPLER_MAX_VOCAB (all three entry points; beyond it: GQ_ENOTSUP).  The grid is 128 blocks and the work buffers are
 * 128 * 32 (128 * 64) elements at every width: up to 131072 logits a block takes a slice of at most 1024, from there to 262144 -- the
 * published Qwen3 vocabulary is 151936 -- a slice of at most 2048 (a second pair of kernel instances; ban ids, seq_out and the embedding
 * row take token ids of the whole range).
 * The draw is a pure function of (logits, top_k, top_p, temperature, seed, *counter, ban list, *pos_io), pinned draw for draw by
 * tests/sampler_model.py:
 *   candidates  the first top_k tokens of the order (fp16 value descending, token id ascending), top_k clamped to [1, 64].  The order is
 *               that of the fp16 bit patterns: -0 sorts directly BELOW +0, so among zeros at the k-th place every +0 is taken before any
 *               -0 (either is a valid top-k among equal values; the nucleus filter and the race compare values, where -0 == +0).
 *               Fewer tokens than top_k (a short vocabulary, banned ids): all of them.  A -inf logit is a candidate like any other and
 *               counts towards top_k; its probability is 0 and it is never drawn while one candidate is finite.
 *   race        score = value / max(T, 1e-5) - log(-log u), u = ((r >> 8) + 1) / 2^24, r = hash32(seed ^ hash32(ctr * 0x9E3779B9 + id + 1))
 *               in 32-bit arithmetic with ctr = (uint32_t)*counter; the largest score wins, equal scores go to the lower id.
 *   counter     *counter = ctr + 1 modulo 2^32: it runs through the sign bit of the int and wraps to 0; the random numbers depend on
 *               the 32 bits alone. */
#define GQ_SAMPLER_MAX_VOCAB 262144
int gq_sample_topk(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter,
                   float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, void *stream);
/* Round 5: the same draw with up to 64 candidates (work_val / work_idx: 128 * 64 elements) and three optional extras for a decode
 * step that runs without the host (guidedquant_amd/generate.py::DecodeGraph, the HF-surface route of AnyPrecisionForCausalLM.generate):
 *   ban      device words {n <= 4, until_pos, id[0..3]} or NULL: while *pos_io < until_pos the listed tokens cannot be drawn -- what HF's
 *            MinNewTokensLengthLogitsProcessor does to EOS (transformers generation, used by inference_example.py:57-67 min_new_tokens);
 *   seq_out  int [seq_cap] or NULL: seq_out[*pos_io + 1] = token (positions as stored BEFORE the increment);
 *   embed_table / x_out / dim / ssq_out: x_out = embed_table[token] (fp16 [dim]) and, with ssq_out, its hand-over statistics
 *            (gq_embed_lookup_ho) -- the next step needs no embedding launch (inference/model.py:121-130). */
int gq_sample_topk_ex(const void *logits, uint32_t vocab, int top_k, float temperature, uint32_t seed, int *counter,
                      float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                      uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, void *stream);
/* Round 6: + nucleus (top-p) filtering of the top-k survivors, as transformers chains its warpers (temperature -> TopKLogitsWarper ->
 * TopPLogitsWarper, generation/logits_process.py): probabilities of the scaled top-k scores, cumulative sum in ascending order, a token
 * is removed when the sum up to and including it is <= 1 - top_p; the most probable token always stays.  top_p in (0, 1]; 1 = exactly
 * gq_sample_topk_ex.  What the HF-surface route needs for `generate(do_sample=True, top_p=0.9)` with the default top_k = 50. */
int gq_sample_topk_p(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                     float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                     uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, void *stream);

/* Token sets: transformers' RepetitionPenaltyLogitsProcessor and SuppressTokensLogitsProcessor inside the fused sampler.
 * A token set is uint32_t [ceil(vocab / 32)] in device memory; token t is bit (t & 31) of word (t >> 5).
 * gq_token_set_build: ONE launch that zeroes the set when clear != 0 and then sets the bits of ids[0 .. n).  Ids outside [0, vocab) are
 * ignored, duplicates are harmless, n == 0 with clear just clears (n == 0 without it launches nothing). */
int gq_token_set_build(const int *ids, uint32_t n, uint32_t vocab, uint32_t *set, int clear, void *stream);
/* gq_sample_topk_p with a repetition penalty over the tokens of `seen` (read, and updated with the drawn token) and the tokens of
 * `suppress` (read only, may be NULL) taken out.  One draw, in this order, pinned draw for draw by tests/sampler_rep_model.py:
 *   suppress   a token of `suppress` is no candidate at all -- exactly like a token of the ban list, which stays and combines with it
 *              (transformers sets such a logit to -inf; here it does not even count towards top_k).  When every token is suppressed or
 *              banned the candidate set is empty and the draw is that of the other entry points with an empty set: the token written
 *              (next_tok, tok_io, seq_out) is INT_MAX (0x7FFFFFFF), the counter and the position advance as always, x_out receives
 *              row 0 of the table, and `seen` is left as it was.
 *   penalty    v = the fp16 logit widened to fp32, rp = repetition_penalty.  A token of `seen` gets s = v < 0 ? fl32(v * rp) : fl32(v / rp),
 *              both correctly rounded, the division a true IEEE division (no reciprocal); -0 is not < 0; +-inf and NaN go through the
 *              same formulas.  Any other token has s = v.  This is the processor applied to the fp32 copy of the logits transformers'
 *              _sample makes, once per distinct token; `seen` holds the prompt and everything drawn so far.
 *   order      everything behind it is gq_sample_topk_p with s in place of the fp16 value: top-k over (s descending AS FP32, token id
 *              ascending), -0 directly below +0 (the order of the fp32 bit patterns), temperature, nucleus, race, counter, ban
 *              expiry, tok_io / pos_io / next_tok / seq_out and the embedding fold.  s is in general NO fp16 value: the selection
 *              keys and the candidate buffer carry all of its 32 bits (work_val / work_idx stay 128 * 64 elements).
 *   state      after the draw the bit of the drawn token is set in `seen` (an atomic OR; the next call reads it behind the kernel
 *              boundary, inside a captured multi-step graph as well).
 * repetition_penalty must be finite and > 0 (GQ_EINVAL otherwise); seen == NULL only with repetition_penalty == 1; top_k > 64 and
 * vocab > GQ_SAMPLER_MAX_VOCAB: GQ_ENOTSUP as above.  With repetition_penalty == 1 and both sets NULL the entry draws the tokens and
 * leaves the state of gq_sample_topk_p.  The kernels are instances of their own: the three entry points above launch what they did. */
int gq_sample_topk_rep(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                       float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                       uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                       uint32_t *seen, const uint32_t *suppress, void *stream);

/* gq_sample_topk_rep that also leaves the drawn token's log-probabilities: every parameter of gq_sample_topk_rep up to `suppress`, then
 *   lp_ws     caller workspace of 2 * 128 floats (the per-block partials of the log-sum-exp), needed when lp_raw != NULL;
 *   lp_raw, lp_drawn   float [lp_cap] each, either may be NULL;
 * pinned draw for draw by tests/sampler_lp_model.py.
 *   draw       gq_sample_topk_rep's.  For the same inputs everything that entry writes -- next_tok, tok_io, pos_io, counter, seq_out,
 *              seen, x_out, ssq_out, the empty-set token INT_MAX included -- is bit-identical, and so are the status codes.  With
 *              repetition_penalty == 1 and both sets NULL it is therefore gq_sample_topk_p's draw as well.
 *   index      p = *pos_io before the increment (0 when pos_io is NULL), i = p + 1 (the index seq_out uses): two floats are written when
 *              i < lp_cap.  No other element of the two arrays is touched.
 *   lp_raw[i]  the drawn token's log-probability under the model's UNPROCESSED distribution, v_tok - lse: v_t the fp16 logit widened to
 *              fp32, lse = log sum_t exp(v_t) over all `vocab` tokens in fp32.  Banned, suppressed and penalised tokens count with their
 *              raw value; a -inf logit contributes 0.  The number score() defines for given text, and the one serving APIs report.
 *   lp_drawn[i]  the log-probability under the distribution the race drew from, a_tok - log sum_{c in C} exp(a_c): C the candidate set
 *              after suppress / ban, penalty, top-k and nucleus, a_c = s_c / max(T, 1e-5) in fp32 as the race forms it.  A one-member C
 *              gives exactly 0.0.  What transformers' compute_transition_scores(..., normalize_logits=True) yields on its processed scores.
 *   special    empty candidate set: both outputs are a quiet NaN.  Logits that are NaN or +inf, or all -inf: the two outputs are
 *              unspecified; the draw stays gq_sample_topk_rep's.
 *   determinism  both outputs are pure functions of the inputs: per-block partials (stage 1: wave reductions and one combine of the four
 *              waves) are combined by stage 2 in a fixed order inside the existing launch, no floating-point atomics; two calls on the
 *              same state give the same bits.  No extra launch, no [steps, vocab] buffer.
 *   NULL forms lp_raw != NULL with lp_ws == NULL is GQ_EINVAL and writes nothing; with both outputs NULL the entry only draws (it then
 *              launches gq_sample_topk_rep's kernels).
 * The kernels are instances of their own: the four entry points above launch what they did.  With repetition_penalty == 1 and both sets
 * NULL the instances with gq_sample_topk_p's 16-bit value keys are launched (the same draw; the fp32 keys of the penalty cost more per
 * token than the two numbers do). */
int gq_sample_topk_lp(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                      float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                      uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                      uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, void *stream);

/* The fused sampler over the WHOLE vocabulary (csrc/sampler_full.hip): gq_sample_topk_lp's draw without the limit of 64 candidates, with
 * min_p.  One draw is a pure function of the inputs, pinned draw for draw by tests/sampler_full_model.py, defined in this order:
 *   live       every token but a NaN logit of either sign, an id of the ban list while *pos_io < until_pos, and a token of `suppress`
 *              (ban and suppress exactly as in gq_sample_topk_rep);
 *   value      s_t = the fp16 logit widened to fp32; for a token of `seen`, s = v < 0 ? fl32(v * rp) : fl32(v / rp) (a true IEEE division,
 *              -0 is not < 0): gq_sample_topk_rep's rule;
 *   order      (s descending as fp32, token id ascending), -0 directly below +0;
 *   top_k      0: no filter.  >= 1: the first n_k = min(top_k, live) tokens of the order stay -- no clamp to 64.  < 0: GQ_EINVAL.  A -inf
 *              logit is a candidate like any other;
 *   scale      T = max(temperature, 1e-5f), a_t = fl32(s_t / T), m = a of the first token of the order;
 *   nucleus    0 < top_p < 1 (1: off, anything else GQ_EINVAL): w_t = exp(a_t - m), Z_k = sum of w over the n_k survivors; the token at
 *              rank j goes when sum_{i >= j} w_i <= (1 - top_p) * Z_k (1 - top_p the fp32 difference); among equal values the higher id
 *              goes first; rank 0 always stays: n_p tokens (transformers' TopPLogitsWarper behind TopKLogitsWarper);
 *   min_p      0 < min_p <= 1 (0: off, anything else GQ_EINVAL): a token goes when w_t < min_p (MinPLogitsWarper: p_t < min_p * p_max);
 *              rank 0 always stays: n_m tokens;
 *   candidates the first n = min(n_p, n_m) tokens of the order -- the chain temperature -> top_k -> top_p -> min_p;
 *   race, counter, publishing, embedding fold: gq_sample_topk_rep's -- score = fl32(fl32(s / T) - logf(-logf(u))) with the same hash32
 *              stream keyed on (seed, counter, token id), the lower id wins a tie, `seen` gets the drawn token's bit; an empty candidate set
 *              publishes 0x7FFFFFFF, embeds row 0 and leaves `seen` alone;
 *   lp_raw / lp_drawn   either may be NULL; gq_sample_topk_lp's meaning and index (*pos_io + 1 < lp_cap).  lp_drawn = a_tok - log sum_C
 *              exp(a_c) over the n candidates; both are a quiet NaN for an empty set.
 * Error model of the two mass cuts: the masses are sums of w * 2^44 in 64-bit integers (order-independent, exact), w = expf(fl32(a - m));
 * tests/sampler_full_model.py derives the grants.  The top_k cut is exact.
 * ws: gq_sample_full_ws_bytes(vocab) bytes, 16-byte aligned, owned by the call (histograms, partials).  gq_sample_full_ws_bytes is host
 * only, launches nothing, and is 0 for vocab > GQ_SAMPLER_MAX_VOCAB.  TEST HOOK: after a call the first 24 bytes of ws hold
 * {uint32 n, uint32 n_k, double Z_k, double Z_kept} -- Z_k, Z_kept the sums of w over the n_k and the n tokens; nothing in the package
 * reads them.
 * Six launches whose grids depend on nothing but the build; no host read-back; counter, pos_io, ban, seen are read from device memory:
 * a captured graph replays it.  Deterministic: integer atomics only.
 * Refusals, nothing launched or written: vocab > GQ_SAMPLER_MAX_VOCAB: GQ_ENOTSUP.  ws_bytes too small, a NULL required pointer (logits,
 * counter, ws, next_tok), repetition_penalty != 1 without seen, ssq_out without x_out, a top_k / top_p / min_p outside the above: GQ_EINVAL. */
size_t gq_sample_full_ws_bytes(uint32_t vocab);
int gq_sample_full(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                   int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                   uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                   uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, void *stream);

/* Top-n alternatives: gq_sample_topk_lp / gq_sample_full that also leave, for the step they draw, the n most probable tokens of the model's
 * UNPROCESSED distribution with their log-probabilities (csrc/topn.hip; serving APIs' top_logprobs = n).  Every parameter of the entry
 * without the suffix up to lp_cap, then
 *   top_n     1 .. GQ_TOPN_MAX;
 *   top_ids   int   [lp_cap * top_n], row-major;
 *   top_lps   float [lp_cap * top_n];
 *   topn_ws   GQ_TOPN_WS_BYTES bytes, 8-byte aligned, owned by the call;
 * pinned by tests/topn_model.py.
 *   draw       the entry's without the suffix: for the same inputs everything it writes -- next_tok, tok_io, pos_io, counter, seq_out, seen,
 *              x_out, ssq_out, lp_raw, lp_drawn, the empty-set token INT_MAX included -- is bit-identical, and so are its status codes.
 *   index      p = *pos_io before the increment, row i = p + 1 (the index seq_out and lp_raw use); pos_io == NULL: row i = 0 (the arrays of a
 *              single draw are 0-based; lp_raw keeps its index 1 there).  The two rows are written when i < lp_cap; no other row is touched.
 *   order      the RAW order: the fp16 logit descending as a bit pattern (-0 directly below +0), the token id ascending among equal patterns.
 *              A NaN logit of either sign is not listed.  Nothing else enters: ban list, suppress, seen / repetition_penalty, temperature,
 *              top_k, top_p and min_p do not -- a suppressed token with the largest logit is listed first, and the rows of a draw with an
 *              empty candidate set are the raw order's like any other.
 *   top_ids[i][j], j < top_n   the first top_n tokens of that order; with fewer than top_n tokens that are no NaN the remaining places hold
 *              id -1 and log-probability -inf.
 *   top_lps[i][j]   fl32(fl32(v - M) - L): v the fp16 logit widened to fp32 and (M, L) = (max, log sum exp(. - max)), the two fp32 numbers
 *              lp_raw of this step is taken against, in lp_raw's two subtractions.  Whenever the drawn token is top_ids[i][j],
 *              top_lps[i][j] == lp_raw[i] bit for bit.  A -inf logit is listed like any other, with -inf.  Where lp_raw is unspecified
 *              (a +inf logit, all -inf, a NaN logit: the sum is NaN) the numbers are the same expression's.
 *   how        two launches of their own behind the sampler's (128 blocks: the best top_n of each slice of <= 1024 logits up to 131072, of
 *              <= 2048 up to 262144; one block: the best of the 128 * top_n), which read the log-sum-exp partials the sampler's launches
 *              left in lp_ws / ws and combine them in the same fixed order.  Grids depend on nothing but the build, the row index is read
 *              from device memory, no host read-back: a captured graph replays them.  Integer maxima only, no atomics: two calls on the
 *              same state give the same bits.
 *   TEST HOOK  after a call the first two floats of topn_ws hold (M, L); nothing in the package reads them.
 * Refusals, nothing launched or written: vocab > GQ_SAMPLER_MAX_VOCAB: GQ_ENOTSUP.  top_n outside 1 .. GQ_TOPN_MAX, a NULL top_ids / top_lps /
 * topn_ws, a topn_ws that is not 8-byte aligned, lp_raw == NULL (or its workspace: lp_ws / ws): GQ_EINVAL.  Then the refusals of the entry
 * without the suffix, with its codes.  The entries without the suffix launch what they launched. */
#define GQ_TOPN_MAX 20
#define GQ_TOPN_WS_BYTES (16 + 128 * GQ_TOPN_MAX * 8)
int gq_sample_topk_lp_topn(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                           float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                           uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                           uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                           int *top_ids, float *top_lps, void *topn_ws, void *stream);
int gq_sample_full_topn(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                        int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                        uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                        uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                        float *top_lps, void *topn_ws, void *stream);

/* Additive adjustments of the logits inside the sampler's launches: a serving API's frequency_penalty, presence_penalty and logit_bias
 * (csrc/sampler.hip, csrc/sampler_full.hip; the exact host model is tests/sampler_adj_model.py).  No [vocab] pass of its own, no host
 * round trip: the counts are read and updated on the device, so a captured multi-step graph replays the entries.
 *   member     token t is a member when its bit is set in bias_set (a listed bias of 0.0 still makes it one) or in out_set (the request has
 *              generated it: out_count[t] > 0).  bias[t] is read for tokens of bias_set only, out_count[t] for tokens of out_set only.
 *   formula    v = the fp16 logit widened to fp32, b = bias[t] (0 when not listed), c = out_count[t] (0 when not generated):
 *                  p  = c > 0 ? fl32(fl32(frequency_penalty * (float)c) + presence_penalty) : 0
 *                  s  = fl32(fl32(v + b) - p)
 *                  h' = fp16(s): round to nearest even, subnormals kept, overflow to +-inf, NaN stays NaN.
 *              Every operation is rounded on its own (no fused multiply-add).  The adjustment is DEFINED to give an fp16 logit: it costs at
 *              most half an fp16 ulp of the logit, the precision the lm_head left in it.  A non-member keeps its bit pattern (-0 and NaN
 *              included; a member's -0 with b = 0, p = 0 becomes +0).
 *   adjusted   everything that draws sees h' in place of the fp16 logit: liveness (a NaN h' is no candidate), suppress / ban, the repetition
 *              penalty (on h' widened, for tokens of `seen`, as in gq_sample_topk_rep), the order, top_k, temperature, nucleus, min_p, the race,
 *              and lp_drawn.  A draw is therefore, bit for bit, the draw of the entry without the suffix on logits the host adjusted by
 *              the formula -- next_tok, tok_io, pos_io, counter, seq_out, seen, x_out, ssq_out, lp_drawn (and gq_sample_full's report).
 *   raw        lp_raw and the top-n rows keep reading the RAW logits: they describe the model's unprocessed distribution.
 *   counts     out_count counts the tokens generated in this request; the prompt does not count (the meaning serving APIs give the two
 *              penalties -- transformers' repetition_penalty, and `seen`, do include the prompt).  The caller clears out_set at the start
 *              of a request; out_count[t] means something for the tokens of out_set only.
 *   state      after the draw the publishing lane sets the token's bit in out_set and adds 1 to out_count[token] -- stores 1 when the bit
 *              was not set before (vector atomics, next to the update of `seen`; the next call reads both behind a kernel boundary).  An
 *              empty candidate set (token INT_MAX) leaves both alone.  Nothing else in the two arrays is written; bias_set and bias are
 *              read only.
 *   order      the additive terms come first, the repetition penalty behind them (vLLM applies its repetition penalty in front of the
 *              frequency and presence terms).  transformers' sequence_bias adds to fp32 scores without the rounding to fp16.
 * GqSampleAdjust: frequency_penalty, presence_penalty finite (0, 0 with out_set NULL: nothing is counted); bias_set (a token set) with bias
 * (float [vocab]): both or neither; out_set (a token set) with out_count (uint32_t [vocab]): both or neither, required when a penalty is != 0.
 * gq_token_bias_build: ONE launch that zeroes bias_set and then, for i < n, sets the bit of ids[i] and stores bias[ids[i]] = values[i].  Ids
 * outside [0, vocab) are ignored; the ids are distinct (two values for one id: either is stored); the values are finite; the other words of
 * bias are not written.  n == 0 just clears the set.
 * gq_sample_topk_adj / gq_sample_full_adj: every parameter of gq_sample_topk_lp_topn / gq_sample_full_topn up to topn_ws, then adj.
 *   top_n == 0   no list: top_ids, top_lps and topn_ws may be NULL and topn.hip's pair is not launched.
 *   adj == NULL, or bias_set and out_set both NULL: the entry draws what the entry without the suffix draws, with its launches.
 *   otherwise    gq_sample_topk_adj launches instances of the two-stage kernels of their own (fp32 keys, the log-probability code, every
 *              pointer of it optional), gq_sample_full_adj instances of its token passes; the entries without the suffix launch what they
 *              launched.
 * Refusals, GQ_EINVAL, nothing launched or written: a penalty that is not finite, one pointer of a pair without the other, a penalty != 0
 * without out_set.  Then the refusals of the entry without the suffix, with its codes (those of the top-n list only when top_n != 0). */
typedef struct {
    float frequency_penalty, presence_penalty; /* finite; 0, 0 with out_set NULL: nothing is counted */
    const uint32_t *bias_set;
    const float *bias; /* both or neither */
    uint32_t *out_set;
    uint32_t *out_count; /* both or neither; required when a penalty != 0 */
} GqSampleAdjust;
int gq_token_bias_build(const int *ids, const float *values, uint32_t n, uint32_t vocab, uint32_t *bias_set, float *bias, void *stream);
int gq_sample_topk_adj(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                       float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                       uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                       uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                       int *top_ids, float *top_lps, void *topn_ws, const GqSampleAdjust *adj, void *stream);
int gq_sample_full_adj(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                       int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                       uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                       uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                       float *top_lps, void *topn_ws, const GqSampleAdjust *adj, void *stream);

/* Constrained decoding: a token-level finite state machine inside the sampler's launches (gq_sample_topk_fsm, gq_sample_full_fsm; tables
 * built by gq_token_fsm_build; guidedquant_amd/token_fsm.py has the host description and its validation).
 *   tables     S states over a vocabulary of V tokens, CSR, all int32 on the device: row_ptr[S + 1]; edge_tok[E], strictly ascending inside
 *              a row; edge_next[E], the state behind the token or -1 = the token is forbidden in this state; default_next[S], what a
 *              token without an edge does: -1 = forbidden, >= 0 = allowed and leads there.
 *   masks      uint32_t [S][words_per_state], words_per_state = ceil(V / 32): row s is the FORBIDDEN set of state s in the layout of
 *              `suppress` (bit t % 32 of word t / 32).  gq_token_fsm_build, ONE launch outside any graph: a row is all ones or all zeros by
 *              the default, then one bit per edge, OR-ed with base_suppress (a token set, or NULL) -- the request's static suppress list --
 *              and the bits at and past V in the last word are set.  An edge token outside [0, V) is ignored.
 *   state      one device word.  Every kernel of a draw that reads `suppress` reads masks + state[0] * words_per_state instead (the
 *              `suppress` argument of the entry is then not read: its set is in the masks); a word outside [0, S) is read as S - 1.
 *   draw       everything that draws sees the mask exactly as it sees `suppress`: a forbidden token takes no top-k place, lp_drawn is
 *              under the masked distribution; lp_raw and the top-n rows keep the unprocessed distribution; the ban list, the repetition
 *              penalty and the additive adjustments compose unchanged.  A draw is, bit for bit, the draw of the entry without the suffix
 *              with `suppress` = the mask row of the current state.
 *   transition the publishing lane of the last kernel searches the drawn token in the state's row (binary search): a hit gives edge_next, a
 *              miss default_next; the result is stored to state[0] (the next call reads it behind a kernel boundary: no launch is added).
 *              The token of an empty candidate set (INT_MAX), or a result of -1, leaves the state as it is.
 * gq_sample_topk_fsm / gq_sample_full_fsm: every parameter of gq_sample_topk_adj / gq_sample_full_adj up to adj, then fsm.  fsm == NULL: the
 * _adj entry serves the call.  Otherwise the _adj entries' own kernel instances run, with adj NULL or neutral as well.
 * Refusals, GQ_EINVAL, nothing launched or written: masks, row_ptr, edge_next, default_next or state NULL (edge_tok may be NULL when no
 * state has an edge), n_states == 0, words_per_state != ceil(vocab / 32); then those of the _adj entry. */
typedef struct {
    const uint32_t *masks; /* [n_states][words_per_state], built by gq_token_fsm_build */
    uint32_t words_per_state, n_states;
    const int32_t *row_ptr, *edge_tok, *edge_next, *default_next;
    int32_t *state; /* one device word: the current state */
} GqTokenFsm;
int gq_token_fsm_build(const int *row_ptr, const int *edge_tok, const int *edge_next, const int *default_next, uint32_t n_states, uint32_t vocab,
                       const uint32_t *base_suppress, uint32_t *masks, void *stream);
int gq_sample_topk_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float temperature, uint32_t seed, int *counter,
                       float *work_val, int *work_idx, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                       uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                       uint32_t *seen, const uint32_t *suppress, float *lp_ws, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n,
                       int *top_ids, float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream);
int gq_sample_full_fsm(const void *logits, uint32_t vocab, int top_k, float top_p, float min_p, float temperature, uint32_t seed,
                       int *counter, void *ws, size_t ws_bytes, int *tok_io, int *pos_io, int *next_tok, const int *ban, int *seq_out,
                       uint32_t seq_cap, const void *embed_table, void *x_out, uint32_t dim, float *ssq_out, float repetition_penalty,
                       uint32_t *seen, const uint32_t *suppress, float *lp_raw, float *lp_drawn, uint32_t lp_cap, int top_n, int *top_ids,
                       float *top_lps, void *topn_ws, const GqSampleAdjust *adj, const GqTokenFsm *fsm, void *stream);

/* Test / tuning hooks (not part of the reference's surface).  gq_reset_env_cache: drop the cached GQ_* environment
 * knobs so that a test can flip them between calls.  gq_debug_set_timing_buffer: device buffer the plane kernels write
 * s_memtime phase stamps into (tools/phase_timing.py); NULL (default) disables it. */
void gq_reset_env_cache(void);
void gq_debug_set_timing_buffer(void *device_buffer);
void gq_debug_set_qtip_timing_buffer(void *device_buffer); /* u64 [16 waves][8] phase stamps of gq_qtip_matvec's middle block */
/* The launch plan of the exact-order AP-GEMV kernel (ap_gemv.hip::pick_quad_cfg) for a shape, without launching: plan[0..5] = threads per
 * block, row slots per step, row steps per block, ring depth, blocks of the launch, and the blocks per CU the instance's occupancy holds at
 * once.  prologue: 0 none, 1 RMSNorm, 2 SiLU * up.  Returns GQ_ENOTSUP when the fast exact path does not serve the shape.  For the test that
 * no plan asks for more resident blocks than fit (a round-6 find: such a launch runs in two rounds). */
int gq_debug_exact_plan(uint32_t N, uint32_t K, int bits, int prologue, uint32_t *plan);
/* The same for a launch with the given epilogue flags (GQ_EPI_SILU_PAIRS plans keep every block on an even number of rows), with the
 * GQ_AP_* knobs applied as the dispatcher applies them: plan[0..5] as above, plan[6] = the kernel the launch runs (0 the v_perm kernel,
 * 1 its instance with the ordered reduction in registers, 2 the 2-bit pair-table kernel). */
int gq_debug_exact_plan_ex(uint32_t N, uint32_t K, int bits, int prologue, uint32_t epilogue, uint32_t *plan);
/* The route of an AP-GEMV dispatch, as its launch site records it: route[0] = the kernel family (GQ_AP_ROUTE_*), route[1] = the launches
 * made, route[2] = the exact kernel that ran (as plan[6] above; 0 for the other families).  gq_debug_ap_last_route: the calling thread's
 * last dispatch (gq_anyprec_gemv*, gq_anyprec_gemv_fused*, gq_anyprec_gemv_qkv_rope*, or a dry one; GQ_AP_ROUTE_NONE after a failed one).
 * gq_debug_ap_plan_route: a dry dispatch of the launch gq_anyprec_gemv (M rows, has_norm = 0, epilogue = 0) or gq_anyprec_gemv_fused_ws
 * (M = 1; ws_bytes: the workspace passed, 0 = none) would make under the current mode / environment: every decision of a real one,
 * nothing launched. */
#define GQ_AP_ROUTE_NONE 0u
#define GQ_AP_ROUTE_GENERIC 1u          /* ap_gemv_generic_kernel */
#define GQ_AP_ROUTE_EXACT 2u            /* ap_gemv_quad_kernel (v_perm, INREG) */
#define GQ_AP_ROUTE_PAIR_TABLE 3u       /* ap_gemv_pt2_kernel */
#define GQ_AP_ROUTE_PLANE 4u            /* ap_plane_kernel: shared image, and the rows-per-pass form of M > 1 */
#define GQ_AP_ROUTE_PLANE_LOCAL 5u      /* ap_plane_local_kernel */
#define GQ_AP_ROUTE_PLANE_CHAIN 6u      /* two ap_plane_kernel launches over the halves of K, the second adding to the first */
#define GQ_AP_ROUTE_STREAM 7u           /* ap_stream_kernel */
#define GQ_AP_ROUTE_STREAM_KSPLIT 8u    /* ap_stream_kernel over K slices + ap_ksplit_reduce_kernel (workspace) */
#define GQ_AP_ROUTE_DQ 9u               /* ap_gemv_dq_kernel */
#define GQ_AP_ROUTE_STREAM_QKV_ROPE 10u /* the stream kernel's q / k / v + RoPE form (gq_anyprec_gemv_qkv_rope*) */
#define GQ_AP_ROUTE_WIDE 11u            /* ap_gemv_wide_kernel: bits 5..8, one batch row, the reference's order */
int gq_debug_ap_last_route(uint32_t *route);
int gq_debug_ap_plan_route(uint32_t N, uint32_t K, int bits, uint32_t M, int has_norm, uint32_t epilogue, size_t ws_bytes, uint32_t *route);

#ifdef __cplusplus
}
#endif
#endif /* GQ_HIP_H */
