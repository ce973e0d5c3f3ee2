/* tell_hip.h - C ABI of libtell_hip.so: the MI355X (gfx950) kernels of the
 * Transform-and-Tell caption hot path.
 *
 * The reference (alasdairtran/transform-and-tell) is pure Python: it has no FFI.
 * Each entry point below replaces the ATen/cuDNN/cuBLAS op *sequence* that the
 * cited reference lines issue; the Python host modules in
 * `transform-and-tell_amd/` (same class names, constructor arguments and
 * state_dict keys as the reference) call these through ctypes.  INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; caller owns all memory; the library
 *     allocates nothing.  Its state, all of it set through this header: a thread-local
 *     error string; four REGISTERED device pointers - two that kernels read while a
 *     hipGraph is recorded / replayed (tell_set_rng_step_ptr, tell_set_pos_step_ptr: the
 *     dropout step and decode position counters), the per-device tile-counter buffer of
 *     the resident GEMM launches (tell_gemm_set_tile_queue) and a thread-local one-shot
 *     hook that arms the next tell_gemm_nt launch with a span stamp (tell_gemm_ts_next);
 *     and the table of named integer OPTIONS below (tell_set_option), which is the only
 *     way to steer a launcher's choice of kernel.  The library reads NO environment
 *     variable;
 *   - every call is asynchronous on `stream` (pass torch's current stream);
 *   - return 0 on success, <0 on error (tell_last_error() explains);
 *   - `dtype`: TELL_F32 = 0 (exact-f32 parity mode, f32 MFMA), TELL_BF16 = 1;
 *     activations / working copies of weights are in `dtype`, statistics, biases,
 *     norm parameters, losses, master weights and gradients of weights are fp32;
 *   - `*_dev` pointers are DEVICE scalars read by the kernel (static shapes, no
 *     host synchronisation: row counts of vocabulary bands, learning rate, ...);
 *   - dropout: keep(idx) = hash(seed, salt, idx) >= p*2^32, scaled by 1/(1-p);
 *     the same (seed, salt) given to the backward call reproduces the mask.
 * All file:line citations are relative to the reference root.
 */
#ifndef TELL_HIP_H
#define TELL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TELL_F32 0
#define TELL_BF16 1
typedef struct ihipStream_t* tell_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------ */
int tell_abi_version(void);
/* Named run-time options (csrc/options.h lists keys and defaults: "gemm_q4", "q4_dynamic", "gemm_s64", "conv_tile", ...).
 * Each is one process-global integer read by the launchers when a launch is ISSUED (a launch recorded into a hipGraph
 * keeps the choice it was recorded with).  Every option selects between kernels that compute the SAME result (to the
 * rounding the parity tests state); the wrong-result timing ablations of tools/probes/ exist only in the probe build
 * (-DTELL_PROBES, libtell_hip_probes.so; tell_probe_build() = 1) - in the shipped library their keys are unknown.
 * tell_set_option -> 0, or -1 for an unknown key (tell_last_error names it); tell_get_option -> the value, or LONG_MIN
 * for an unknown key; tell_option_key(i) / tell_option_default(i) enumerate the table (NULL / LONG_MIN past its end). */
int tell_set_option(const char* key, long value);
long tell_get_option(const char* key);
const char* tell_option_key(int index);
long tell_option_default(int index);
int tell_probe_build(void);
int tell_device_count(void);
const char* tell_last_error(void);
void tell_set_error(const char* msg);
/* host evaluation of the dropout RNG / threshold used by every kernel (csrc/common.h): the 16-bit field element idx
 * is judged by (kept iff field >= threshold) */
uint32_t tell_keep_field_host(uint32_t seed, uint32_t salt, uint64_t idx);
/* hipGraph capture of kernels with dropout: while `counter` (device uint32) is registered, every RNG kernel adds
 * counter * odd-constant to its salt, so a captured graph draws fresh masks after the owner increments it;
 * NULL (default) = eager behaviour.  The stream argument is ignored (uniform binding signature). */
int tell_set_rng_step_ptr(const void* counter, tell_stream_t stream);
/* the same mechanism for the position offset of the embedder (positional.py:170-173 keeps it in incremental_state):
 * while registered, tell_embed_finalize adds *counter to start_pos - one captured decode step serves every position */
int tell_set_pos_step_ptr(const void* counter, tell_stream_t stream);
/* in-graph bookkeeping of a captured decode step: `next` (device uint32, or NULL) holds the position offset of the NEXT
 * step; tell_embed_gather_step - the step's first kernel - reads it and publishes it in the counter registered above,
 * tell_greedy_update / tell_beam_update - its last - write the following offset back (their `counter` argument) */
int tell_set_pos_next_ptr(void* next, tell_stream_t stream);
uint32_t tell_drop_threshold_host(float p);
/* host evaluation of the sampling uniform u(seed, row, step) in [0, 1) (tell_adaptive_logprob_sample, step 3) */
float tell_sample_uniform_host(uint32_t seed, uint32_t row, uint32_t step);
/* measurement aid (bench.py roofline): rate of the device wall clock in kHz (100 000 on MI355X) */
int tell_wall_clock_khz(void);
/* measurement aid (bench.py --cu-hog, the single-GPU rehearsal of what RCCL's channel kernels do to a step whose dominant
 * GEMM needs whole compute units - SURVEY 8e): n workgroups that each hold one CU (64 KB of LDS) for `ticks` of the device
 * wall clock (capped at 4 s), or until *stop (device int32, may be NULL) becomes non-zero, and do nothing else */
int tell_cu_hog(int n_workgroups, long ticks, int* stop, tell_stream_t stream);
/* arm the NEXT tell_gemm_nt launch of this thread: its direct-to-LDS / ping-pong kernel records its execution span
 * into ts[0] (first workgroup in) / ts[1] (last workgroup out), device wall-clock ticks; ts is uint64[3], zero before
 * the first use (ts[2] counts workgroup arrivals: every launch of the same grid re-opens the span by itself) */
int tell_gemm_ts_next(void* ts, tell_stream_t stream);
/* register the tile counters of the RESIDENT 256x256 GEMM launches (gemm_nt_pp2 / q4 / q4e kernels) FOR THE CALLING THREAD'S
 * CURRENT DEVICE: `counters` = n zero-initialised int32 on that device, owned by the caller and alive for as long as GEMMs
 * are launched there (NULL / 0 unregisters: resident launches then walk static tile lists).  The buffer is cut into slots
 * of 8 counters (one per XCD); a launch with more tiles than workgroups takes one slot as its work queues and leaves it
 * zero.  Launches recorded into a hipGraph keep their slot while the graph lives and take it from the first half of the
 * buffer (released slots first, then fresh ones; when the half is used up, later captures use static lists); eager
 * launches walk a ring over the second half.  Hand-out is thread-safe.  The host mirror registers 2^20 counters per device. */
int tell_gemm_set_tile_queue(void* counters, int n, tell_stream_t stream);
/* bookkeeping of the slots captured launches keep (host-only calls, no stream): _log_begin arms a thread-local record of the
 * slot numbers the calling thread's captured launches take from now on; _log_end returns how many were taken (copying at
 * most `cap` of them to `out`) and disarms it; _release gives slots back to the current device's free list (call it when
 * the graph that recorded them is destroyed); _stats: out[0] = slots, out[1] = fresh captured slots handed out so far,
 * out[2] = free-list length. */
int tell_gemm_tile_queue_log_begin(void);
int tell_gemm_tile_queue_log_count(void);   /* slots logged so far (the log stays open): sizes the buffer for _log_end */
int tell_gemm_tile_queue_log_end(int* out, int cap);
int tell_gemm_tile_queue_release(const int* slots, int n);
int tell_gemm_tile_queue_stats(int* out);

/* ---- exact-erf GELU as its own launch (bf16; y may be x) ----------------------
 * the activation between fc1 and fc2 of fairseq's TransformerSentenceEncoderLayer (activation_fn = gelu) when it is kept
 * out of the fc1 GEMM's epilogue (act 2 of tell_gemm_nt is the fused form; same formula). */
int tell_gelu(const void* x, void* y, long n, int dtype, tell_stream_t stream);

/* ---- GEMM with the transformer sub-layer residual in its epilogue -----------
 * out[M,N] = res[M,N] + dropout_p(A[M,K] . B[N,K]^T + bias[n]), bf16, mask = the one tell_layernorm_fwd draws for
 * (seed, salt) over an [M,N] input.  Replaces  x = residual + F.dropout(self.out_proj(attn)) / F.dropout(self.fc2(h))
 * of fairseq's TransformerSentenceEncoderLayer as called by roberta.extract_features
 * (transformer_faces_objects.py:352-353); the LayerNorm that follows then reads ONE tensor.
 * Returns 1 (nothing launched) when the shape is not whole rounds of 256x256 tiles: run tell_gemm_nt +
 * tell_layernorm_fwd(res) instead. */
int tell_gemm_nt_dropout_residual(const void* A, long lda, const void* B, long ldb, const float* bias, const void* res,
                                  long ld_res, void* C, long ldc, int M, int N, int K, float p, uint32_t seed,
                                  uint32_t salt, tell_stream_t stream);

/* ---- GEMM (every nn.Linear / F.linear / 1x1 conv on the path) --------------
 * C[M,N] = act((A[M,K] . B[N,K]^T + bias) * alpha) (+ C if accumulate)
 * Replaces F.linear in tell/modules/linear.py:8-33 (GehringLinear),
 * multi_head.py:488-526 (in_proj_q/k/v, out_proj), dynamic.py:300 (weight_linear),
 * softmax.py:24-40,182-189 (head / tail projections), adaptive.py:73 (band
 * projections) and the convolutions of resnet.py:92-108 (NHWC rows).
 * bias_mode 0 none | 1 bias[n] | 2 bias[m];  act 0 none | 1 relu | 2 gelu(erf) |
 * 3 multiply by (aux[m,n] > 0) (relu backward) | 4 relu(result + aux[m,n]) (residual block);  m_dev: optional device row count.
 * aux has the type of C and the ROW STRIDE of C: aux[m,n] is read at aux + m * ldc + n (there is no stride argument of
 * its own), so an aux next to a strided C must be laid out with the same ldc. */
int tell_gemm_nt(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                 int in_dtype, int out_dtype, const float* bias, int bias_mode, int act, const void* aux,
                 float alpha, int accumulate, const int* m_dev, tell_stream_t stream);

/* The kernel tell_gemm_nt would launch for exactly these arguments, as a readable label ("gemm_nt_pp_kernel<bf16,256,256>",
 * "gemm_nt_glds_kernel<bf16,128,128>", ...); nothing is launched.  Measurement aid (bench.py's roofline block). */
const char* tell_gemm_nt_plan(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                 int in_dtype, int out_dtype, const float* bias, int bias_mode, int act, const void* aux,
                 float alpha, int accumulate, const int* m_dev, tell_stream_t stream);

/* bf16 GEMM with K-major operands (no transposed copies in HBM): trans_a -> A stored [K][M] (lda >= M),
 * trans_b -> B stored [K][N].  The backward forms of the same reference lines: autograd of F.linear gives
 * grad_weight = grad_out^T . x (trans_a = trans_b = 1) and grad_in = grad_out . W (trans_b = 1).
 * a_colsum (trans_a only, may be NULL): a_colsum[m] += a_colsum_scale * sum_k A[k][m] - grad_bias = column sums
 * of grad_out, taken from the tiles the wgrad GEMM stages anyway. */
int tell_gemm_bf16(const void* A, long lda, int trans_a, const void* B, long ldb, int trans_b, void* C, long ldc,
                   int M, int N, int K, int out_dtype, const float* bias, int bias_mode, int act, const void* aux,
                   float alpha, int accumulate, const int* m_dev, float* a_colsum, float a_colsum_scale,
                   tell_stream_t stream);

/* n independent bf16 products in a few launches (the weight gradients of a backward pass queued until its end, the
   query / output projections of a decoder layer's context attentions, their input gradients):
       C_i[M,N] (+)= act((op(A_i) op(B_i)^T + bias_i) * alpha_i)
   trans_a / trans_b as in tell_gemm_bf16: 0/0 the NT form (A [M,K], B [N,K]); 0/1 B stored [K,N] (dX = dY W);
   1/1 A stored [K,M] as well (dW = dY^T X), which may carry asum_i[m] += asum_scale_i * sum_k A_i[k][m] (the bias
   gradient).  bias: fp32 per column (bias_mode 1), NT form only; act: 0 none, 1 relu.  `problems` is a HOST array. */
/* second half of a split-K product whose K slices ran as fp32 problems of tell_gemm_grouped (skinny decode-step GEMMs):
   out[M,N] = act((sum_s partial[s][M][N] + bias) * alpha); partial slice s at partial + s * split_stride floats;
   bias fp32 [N] or NULL; act 0 none / 1 relu / 2 gelu(erf); N and ldc multiples of 4. */
int tell_splitk_reduce(const float* partial, int splits, long split_stride, int M, int N, const float* bias, int act,
                       float alpha, void* out, long ldc, int out_dtype, tell_stream_t stream);
/* the same with a device-side row count: rows >= *m_dev (may be NULL) are neither read nor written */
int tell_splitk_reduce2(const float* partial, int splits, long split_stride, int M, int N, const float* bias, int act,
                       float alpha, void* out, long ldc, int out_dtype, const int* m_dev, tell_stream_t stream);

typedef struct tell_gemm_problem {
  const void* A; long lda;
  const void* B; long ldb;
  void* C; long ldc;
  int M, N, K;
  int trans_a, trans_b;
  int out_dtype;          /* of C: TELL_F32 / TELL_BF16 */
  int accumulate;         /* C += */
  float alpha;
  const float* bias;      /* fp32 [N] or NULL */
  int bias_mode;          /* 0 none, 1 per column */
  int act;
  float* asum;            /* fp32 [M] or NULL */
  float asum_scale;
  const int* lim_dev;     /* device int32 or NULL: the number of VALID ROWS of the batch dimension - rows of A (and C) in the
                           * nt / nn forms (M: tiles past it are skipped, their C rows stay untouched), the reduction
                           * length in the tn form (K: rows past it of both K-major operands are not read).  The adaptive
                           * softmax's tails work on fixed-capacity buffers with a device-side count (adaptive.py:61-76
                           * without the mask.any() / nonzero() host syncs). */
} tell_gemm_problem;
int tell_gemm_grouped(int n, const tell_gemm_problem* problems, tell_stream_t stream);

/* ---- casts / transposes / weight norm -------------------------------------- */
int tell_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, tell_stream_t stream);
/* dst = (dst_dtype)(src * *scale_dev) (scale_dev NULL = 1; dst may alias src for fp32): the fp32 flat gradient on its way
 * to the data-parallel exchange, weighted by the rank's share of the global token count - what scaling the loss
 * before backward() does in the eager schedule (new functionality; ref loop callback_apex_trainer.py:208-247) */
int tell_scale_cast(const float* src, void* dst, int dst_dtype, long n, const float* scale_dev, tell_stream_t stream);
/* dst_t[c][r] = src[r][c] * row_scale[r]; optional dst_plain[r][c] = same value (either may be NULL) */
int tell_transpose(const void* src, long ld_src, int src_dtype, void* dst_t, long ld_t, void* dst_plain,
                   long ld_p, int dst_dtype, const float* row_scale, int rows, int cols, tell_stream_t stream);
/* weight norm, tell/modules/linear.py:33 (torch weight_norm dim=0): scale[r] = g[r]/||v[r]||, norms[r] = ||v[r]|| */
int tell_wn_rowscale(const float* g, const float* v, int rows, int cols, float* scale, float* norms,
                     tell_stream_t stream);
/* the whole working weight in one pass: w[r,:] = g[r] * v[r,:] / ||v[r,:]|| (bf16 or fp32) and norms[r] */
int tell_wn_weight(const float* g, const float* v, int rows, int cols, void* w, int out_dtype, float* norms,
                   tell_stream_t stream);
int tell_wn_backward(const float* dW, const float* g, const float* v, const float* norms, int rows, int cols,
                     float* dg, float* dv, tell_stream_t stream);
/* The same two passes over n GehringLinears in ONE launch (per 32 tensors).  Every array argument is a HOST array of
   n entries: device pointers (g [rows], v [rows, cols], w [rows, cols], norms [rows], dW / dv [rows, cols],
   dg [rows]) or sizes. */
int tell_wn_weight_multi(int n, const void* const* g, const void* const* v, void* const* w, void* const* norms,
                         const int* rows, const int* cols, int out_dtype, tell_stream_t stream);
int tell_wn_backward_multi(int n, const void* const* dW, const void* const* g, const void* const* v,
                           const void* const* norms, const int* rows, const int* cols, void* const* dg,
                           void* const* dv, tell_stream_t stream);
/* store (host int[n], may be NULL): tensor j's dg / dv are written (beta = 0) instead of accumulated - for gradients
 * whose only producer in a step is this launch and that tell_bertadam_step2 was told not to zero (keep_grad). */
int tell_wn_backward_multi2(int n, const void* const* dW, const void* const* g, const void* const* v,
                            const void* const* norms, const int* rows, const int* cols, void* const* dg,
                            void* const* dv, const int* store, tell_stream_t stream);

/* ---- elementwise ------------------------------------------------------------ */
/* nn.GLU, decoder_faces_objects.py:194-195,259-261: h = [a | gate] */
int tell_glu_fwd(const void* h, void* y, long rows, int C, int dtype, tell_stream_t stream);
int tell_glu_bwd(const void* h, const void* dy, void* dh, long rows, int C, int dtype, tell_stream_t stream);
/* F.dropout, decoder_faces_objects.py:106,257 */
int tell_dropout(const void* x, void* y, long n, float p, uint32_t seed, uint32_t salt, int dtype,
                 tell_stream_t stream);
/* bias gradients: out[c] (+)= sum_r x[r][c] */
int tell_colsum_chunks(int rows);
int tell_colsum(const void* x, long ld, int rows, int C, int dtype, float* out, int accumulate,
                const int* m_dev, float scale, float* workspace, tell_stream_t stream);
/* F.relu backward (decoder_faces_objects.py:360): dx = dy * (y > 0) */
int tell_relu_bwd(const void* dy, const void* y, void* dx, long n, int dtype, tell_stream_t stream);
int tell_axpy(const void* x, void* y, long n, float alpha, int dtype, tell_stream_t stream);
/* out = x0 + ... + x[n_in-1] (dense, same shape; unused pointers NULL): the gradient fan-in autograd performs with
 * n-1 pairwise adds where one activation feeds several branches (decoder_faces_objects.py:271-352) */
int tell_sum_n(const void* x0, const void* x1, const void* x2, const void* x3, const void* x4, const void* x5,
               const void* x6, const void* x7, int n_in, void* out, long n, int dtype, tell_stream_t stream);
int tell_fill_f32(float* x, long n, float value, tell_stream_t stream);
int tell_sum_f32(const float* x, int n, const int* m_dev, float* out, int accumulate, tell_stream_t stream);
/* X.index_select(0, idx) / inverse, softmax.py:184-189 */
int tell_gather_rows(const void* src, long ld_src, const int* idx, const int* count_dev, int cap, void* dst,
                     long ld_dst, int C, int dtype, tell_stream_t stream);
int tell_scatter_add_rows(const void* src, long ld_src, const int* idx, const int* count_dev, int cap, void* dst,
                          long ld_dst, int C, int dtype, tell_stream_t stream);
/* NaN-padded face/object rows -> mask + zeros, transformer_faces_objects.py:373-379 */
int tell_nan_rows(const float* x, int rows, int C, void* y, int out_dtype, uint8_t* mask, tell_stream_t stream);
/* softmax(bert_weight)-weighted sum of the 25 RoBERTa layers, transformer_faces_objects.py:355-364 */
int tell_mix_fwd(const void* H, const float* w, int L, long n, void* out, int dtype, tell_stream_t stream);
int tell_mix_bwd(const void* H, const void* dOut, int L, long n, float* partial, int n_blocks, int dtype,
                 tell_stream_t stream);

/* gw[l] += softmax(w)[l] * (d[l] - sum_j softmax(w)[j] d[j]), d = column sums of tell_mix_bwd's partial [n_blocks, L]:
 * the gradient of the mixing logits, one launch (25 scalars). */
int tell_mix_wgrad(const float* partial, int n_blocks, int L, const float* w, float* gw, tell_stream_t stream);
/* out[0] = x[0] / (ln 2 * n_valid[0]): summed cross entropy (nats) -> bits per target token, transformer_faces_objects.py:85-88
 * (and the gradient of the sum from the gradient of the loss). */
int tell_loss_bits(const float* x, const int* n_valid, float* out, tell_stream_t stream);

/* ---- beam search bookkeeping (the loop of transformer_faces_objects.py:443-494 widened to K hypotheses)
 * tk int32 / lp fp32 [B,K,K]: the K best continuations of every hypothesis (tell_adaptive_logprob_topk); per sample the
 * K best of cum[parent] + lp / temperature (a finished hypothesis continues with pad at no cost; lowest index wins a
 * tie); in place: cum fp32 [B,K], finished uint8 [B,K], seqs int64 [B,K,L] (column step + 1 written), lps fp32
 * [B,K,L-1] (column step); out: cur int64 [B*K] next input tokens, rows int64 [B*K] the row each survivor descends from.
 * back (optional): the ancestor table int32 [n_back <= 31][B*K] of the DynamicConv rings (tell_dynconv_step), composed in
 * place with this step's parents: new back[0][r] = rows[r], new back[j][r] = old back[j-1][rows[r]] - the reference's
 * reorder_incremental_state (dynamic.py:338-342) without moving a row.  counter (optional): device int32 that a captured
 * decode step reads as its position offset (tell_set_pos_step_ptr); set to `step`, the offset of step + 1.  step_dev
 * (optional): the launch is PART of a captured step - the step index is *step_dev + 1 instead of `step`. */
int tell_beam_update(const int* tk, const float* lp, float* cum, uint8_t* finished, long* seqs, float* lps, long* cur,
                     long* rows, int B, int K, int L, int step, int pad, int eos, float inv_temp, int* back, int n_back,
                     int* counter, const int* step_dev, tell_stream_t stream);
/* tell_beam_update with a length penalty.  len int32 [B,K], in place: the number of generated tokens
 * of every hypothesis, eos included (a live candidate of step i has i + 1, a finished one keeps its own); inv_norm fp32
 * [L + 1], built by the host: inv_norm[0] = 1, inv_norm[l] = float32(float64(l) ** -alpha).  Per sample the K survivors are
 * the K best of score = (cum[parent] + lp * inv_temp) * inv_norm[len] - ONE fp32 multiply on the raw sum - among the K x K
 * candidates, lowest candidate index first on ties; cum stays the RAW sum, len is written for the survivors; everything else
 * (finished, seqs, lps, cur, rows, the ancestor table, counter / step_dev) as tell_beam_update.  The all-ones table gives
 * tell_beam_update's results bit for bit. */
int tell_beam_update_norm(const int* tk, const float* lp, float* cum, uint8_t* finished, long* seqs, float* lps, long* cur,
                          long* rows, int* len, const float* inv_norm, int B, int K, int L, int step, int pad, int eos,
                          float inv_temp, int* back, int n_back, int* counter, const int* step_dev, tell_stream_t stream);
/* The ban set of every decode row (no_repeat_ngram_size / min_len).  Step i of a row has the history
 * h[0 .. i], h[0] = <s>.  With n = ngram >= 1 and i + 1 >= n: for every p in 0 .. i + 1 - n with
 * h[p .. p + n - 2] == h[i - n + 2 .. i], h[p + n - 1] is banned (n = 1: every token of the history).  i < min_len bans eos.
 * A finished row (finished[r] != 0) bans nothing.  hist int64 [rows, ld_hist] with L <= 256 columns (beam: seqs as
 * [B*K, L]; greedy: ids), finished uint8 [rows] or NULL; i = `step`, or *step_dev + 1 when step_dev is given (the device
 * counter of a captured decode step, as tell_greedy_update / tell_beam_update read it).  out: ban int32 [rows, ld_ban],
 * ld_ban >= L + 1 (duplicates allowed, no order promised), n_ban int32 [rows]. */
int tell_decode_ban_list(const long* hist, long ld_hist, int L, const uint8_t* finished, int rows, int step,
                         const int* step_dev, int ngram, int min_len, int eos, int* ban, long ld_ban, int* n_ban,
                         tell_stream_t stream);
/* The token counts of every decode row (repetition / presence / frequency penalties).  hist, finished,
 * step and step_dev as tell_decode_ban_list.  Step i of a live row: pen_tok[r][0 .. n_pen[r]) holds the distinct tokens of
 * h[0 .. i] in order of first occurrence, pen_cnt[r][e] = c_t, the number of positions of h[0 .. i] that hold pen_tok[r][e];
 * nothing is written behind the list.  A finished row has n_pen[r] = 0.  pen_tok, pen_cnt int32 [rows, ld_pen >= L], n_pen
 * int32 [rows]. */
int tell_decode_token_counts(const long* hist, long ld_hist, int L, const uint8_t* finished, int rows, int step,
                             const int* step_dev, int* pen_tok, int* pen_cnt, long ld_pen, int* n_pen,
                             tell_stream_t stream);
/* VOCABULARY MASKS.  A row's mask is a bitmap over the vocabulary, uint32 [words], words = (vocab + 31)
 * / 32, bit (t & 31) of word t >> 5 set = token t may not be picked.  Under a mask
 *   - a masked token has score -inf: it is never among the k best and is never drawn;
 *   - every other log-prob is exactly what the unmasked kernel reports: the log-sum-exps run over the whole row and nothing is
 *     renormalised;
 *   - ties: value descending, lower id first;
 *   - hypothesis row r uses mask row r / per (beam search: per = K; n sampled captions per image: per = n; otherwise 1);
 *   - the bookkeeping of a finished row and a forced prefix token (tell_adaptive_logprob_forced, which still reports the model's
 *     own log-prob bit for bit) sit behind the pick and never see the mask.
 * The mask of image b is  deny[b] | (cls & ~present[b])  with the eos bit always cleared: present[b] is the set of ids in the
 * row's article ctx[b][0 .. S) (ids equal to `pad`, negative ids and ids >= vocab are ignored), cls the grounded class (tokens
 * of the class may be generated only if they occur in the article), deny the caller's banned set.
 * tell_decode_vocab_mask builds it, one workgroup per image: ctx int64 [rows, S] with leading dimension ld_ctx; cls_bits uint32
 * [words] or NULL (no class); deny8 uint8 [1 or rows, vocab] (non-zero = banned; ld_deny = 0: one row shared by all, else the
 * leading dimension) or NULL; mask uint32 [rows, ld_mask >= words].  Bits past `vocab` in the last word are written as 0,
 * nothing is written behind `words`.  vocab <= 2^18. */
int tell_decode_vocab_mask(const long* ctx, long ld_ctx, int S, int rows, int vocab, const uint32_t* cls_bits,
                           const uint8_t* deny8, long ld_deny, int eos, int pad, uint32_t* mask, long ld_mask,
                           tell_stream_t stream);
/* buf[i][p][r][:] <- buf[i][p][rows[r]][:] in place for n <= 8 bf16 buffers [planes[i], M, 1024] (HOST arrays); rows[r]
 * must lie inside r's group of K consecutive rows (dynamic.py:338-342 reorder_incremental_state, all layers at once) - for
 * input buffers kept in time order (the layer-by-layer fp32 step); the rings of tell_dynconv_step are never moved. */
int tell_reorder_rows(int n, void* const* bufs, const int* planes, const long* rows, int M, int C, int K,
                      tell_stream_t stream);
/* The n sampled hypotheses of every image (generate(n_samples=n)): duplicates flagged, scored and
 * ranked in one launch behind the decode loop, one workgroup per image.  Hypothesis j of image b is row r = b * n + j of
 * ids int64 [B * n, ld_ids >= steps + 1] (column 0 = <s>), lps fp32 [B * n, ld_lps >= steps] and done_step int64 [B * n]
 * (the bookkeeping buffers of tell_greedy_update); 1 <= n <= 16, 1 <= steps <= 256.
 *   len[r]   = min(max(done_step[r], 0), steps): the steps the row took part in, its </s> included;
 *   score[r] = (lps[r][0] + .. + lps[r][len - 1]) * inv_norm[len]: ONE fp32 accumulator, added in ascending order, then one
 *              fp32 multiply (inv_norm fp32 [>= steps + 1], the table of tell_beam_update_norm; NULL: no multiply) - a
 *              sequential fp32 loop on the host gives the same bits;
 *   dup[b][j] = 1 when some j' < j of the image has the same len and the same tokens ids[..][1 .. len] (what lies behind
 *              a row's </s> is not compared);
 *   cons[b][i] (rule 2, or whenever cons is given): with big(i) the MULTISET of token-id bigrams of the generated tokens
 *              ids[r][1 .. len] without a final `eos`, u(i, j) = 2 |big(i) n big(j)| / (|big(i)| + |big(j)|) (counts clipped
 *              to the smaller one; 0 when the denominator is 0; the quotient of two exact fp32 integers), cons = the sum
 *              of u(i, j) over j != i - duplicates included - in ascending j, divided by n - 1; 0 for n = 1.
 *   order[b][.]: the hypotheses of the image, first rank first.  rule 0 (draw): the identity.  rule 1 (score): every
 *              non-duplicate before every duplicate, then score descending, then the lower j.  rule 2 (consensus):
 *              non-duplicates first, then cons descending, then score descending, then the lower j.  A NaN key ranks as -inf.
 * out: order int32, score fp32, dup uint8 [B, n]; cons fp32 [B, n] (may be NULL unless rule = 2); len int32 [B, n] (may be
 * NULL).  `pad` is not read: a row is cut at len.  No atomics, no scratch in global memory; at most 16 x 256 tokens in LDS. */
int tell_sample_rank(const long* ids, long ld_ids, const float* lps, long ld_lps, const long* done_step,
                     const float* inv_norm, int B, int n, int steps, int pad, int eos, int rule, int* order, float* score,
                     uint8_t* dup, float* cons, int* len, tell_stream_t stream);
/* Reward and advantage of the n sampled hypotheses of every image against its reference caption, in one launch (self-critical
 * sequence training).  Hypothesis j of image b is row r = b * n + j of ids int64 [B * n, ld_ids >= steps
 * + 1] (tell_sample_rank's convention), the references are ref int64 [B, ld_ref >= ref_steps + 1]; column 0 of both is <s>.
 * 1 <= n <= 16, 1 <= steps, ref_steps <= 256, n-gram orders 1 .. max_order with max_order in 1 .. 4.
 *   hyp(r)    = ids[r][1 ..] up to, and excluding, the first `eos` or `pad`, at most `steps` tokens; ref(b) alike over ref_steps;
 *   match     = sum over k of |H_k n R_k|, H_k / R_k the MULTISETS of k-grams of hyp(r) / ref(b), counts clipped to the smaller;
 *   th        = sum over k of max(|hyp| - k + 1, 0), tr the same sum for the reference;
 *   reward[r] = float(match) / float(max(th, tr)), 0 when both are 0: the sentence-level GLEU of GNMT, the quotient of two
 *               exact fp32 integers;
 *   adv[r]    = reward[r] - baseline[b] with baseline fp32 [B] given (the reward of the greedy caption, from a call with
 *               n = 1); with baseline == NULL and n > 1 leave-one-out: reward[r] - s / (n - 1), s the sum of the image's OTHER
 *               rewards in ascending j in ONE fp32 accumulator (a sequential fp32 loop on the host gives the same bits); with
 *               baseline == NULL and n == 1 the reward itself.
 * out: reward, adv fp32 [B, n]; counts int32 [B * n, 3] = (match, th, tr), may be NULL.  No float atomics, no scratch in global
 * memory; at most 17 x 256 tokens in LDS. */
int tell_caption_reward(const long* ids, long ld_ids, const long* ref, long ld_ref, const float* baseline, int B, int n,
                        int steps, int ref_steps, int pad, int eos, int max_order, float* reward, float* adv, int* counts,
                        tell_stream_t stream);

/* ---- LayerNorm: y = LN(res + dropout(x)), decoder_faces_objects.py:263-266,367-372 */
int tell_layernorm_fwd(const void* x, long ld_x, const void* res, long ld_r, const float* gamma,
                       const float* beta, void* y, long ld_y, float* mean, float* rstd, int rows, int C,
                       float eps, float p, uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);
int tell_layernorm_bwd_blocks(int rows);
int tell_layernorm_bwd(const void* dy, long ld_dy, const void* x, long ld_x, const void* res, long ld_r,
                       const float* gamma, const float* mean, const float* rstd, void* dx, long ld_dx,
                       void* dres, long ld_dres, int dres_accumulate, float* dgamma, float* dbeta,
                       int dparam_accumulate, float* partial, int rows, int C, float p, uint32_t seed,
                       uint32_t salt, int dtype, tell_stream_t stream);

/* ---- batched small launches of the training step (csrc/multi.hip) ------------------------------------------------
 * n column sums in one launch: dst0[i][c] += sum_r src[i][r][c] for c < w0[i], dst1[i][c - w0[i]] += ... for the rest
 * (fp32, deterministic order).  The jobs: LayerNorm gamma / beta gradients from the per-row-block partials that
 * tell_layernorm_bwd / tell_layernorm_cat_bwd leave when called with dgamma == NULL ([blocks][2C] each), and the
 * bias_k / bias_v gradients of the context attentions (multi_head.py:355-374 backward: per-batch rows [B][2E]).
 * All arrays are HOST arrays of length n. */
int tell_colsum_multi(int n, const void* const* src, const long* ld, const int* rows, const int* width, const int* w0,
                      void* const* dst0, void* const* dst1, tell_stream_t stream);
/* n bf16 transposes in one launch, dst[i][c][r] = src[i][r][c]: the per-step W^T copies of the backward pass's
 * large input-gradient GEMMs (fc2, context_fc, the stacked article K|V projection). */
int tell_transpose_multi(int n, const void* const* src, const long* ld_src, void* const* dst, const long* ld_dst,
                         const int* rows, const int* cols, tell_stream_t stream);
/* out = add + dropout(x) with tell_dropout's mask (same seed / salt / element index): the gradient of a block input
 * that is both the residual and, through the input dropout, the branch input (decoder_faces_objects.py:256-266). */
int tell_dropout_add(const void* x, const void* add, void* out, long n, float p, uint32_t seed, uint32_t salt, int dtype,
                     tell_stream_t stream);
/* ---- the generation step (transformer_faces_objects.py:443-494, decoder_faces_objects.py:224-352 at T = 1), csrc/decode.hip
 * At M = batch x beam <= 128 rows every linear layer is a weight-streaming problem; these three replace the training
 * kernels on that path (12 launches per decoder layer instead of ~24).
 *
 * tell_skinny_linear: out[p] = (act(prologue(in[p]) . w[p]^T + bias[p])) * scale + residual, n_prob <= 4 problems of one
 * shape per launch (HOST arrays of n_prob pointers), bf16 weights [N (2N with GLU), K], M <= 1024, K % 256 == 0.
 *   pro 3 / 4 (round 5): the LayerNorm FOLDED into the product - in = the bf16 PRE-norm rows, w = the weights scaled by the
 *   LayerNorm's gamma along K, gamma[p] / beta[p] carry problem p's fp32 vectors s [K / seg][N (2N)] and c [N (2N)] with
 *   s[g][n] = sum_k w[n][k] over segment g, c[n] = sum_k W[n][k] beta[k]; the kernel gathers mean / rstd of its rows (per
 *   `seg` columns for pro 4: K / seg in {1, 2, 4}, one problem) from its own operands and applies
 *   LN(x) . W^T = rstd (x . w^T) - rstd mean s + c in the epilogue; stats_out (pro 3) receives (mean, rstd); act 0 or 2.
 *   pro 0: in bf16 [M,K].  pro 1: in fp32 [M,K] (a pre-norm `residual + branch`), LayerNorm(gamma[0], beta[0], eps) first;
 *   stats_out (optional, [M][2] fp32) receives (mean, rstd) per row.  pro 2: one LayerNorm per `seg` columns of in
 *   (gamma[s], beta[s], K / seg <= 4): the four LayerNorms that end the context block feeding context_fc.  pro 1 / 2 are
 *   one extra launch into ws (bf16 [M,K], required then, NULL otherwise); all problems must read the same input; rows /
 *   segments of 1024 .. 4096 columns.
 *   act 0 none, 1 ReLU, 2 GLU (gate rows at n + N, fairseq's linear1 + F.glu, dynamic.py / decoder_faces_objects.py:229-233).
 *   residual: res (bf16 [M,N]), LayerNorm(res_raw) rebuilt from res_stats ([M][2]), res_gamma, res_beta, res_f32 (fp32
 *   [M,N]); each may be NULL.
 *   out bf16 or (out_f32) fp32 [M,N]; out2 (optional, bf16): columns n >= out2_from of the result once more, at
 *   out2[m][p * N + n - out2_from] for problem p (the softmax head: cluster logits in fp32 and the tails' projected inputs in bf16 from one
 *   launch).
 *   split_ws (optional, split_ws_bytes >= 64 KB + the partial tiles; 16-byte aligned, ZEROED ONCE when allocated and then
 *   owned by the launches of ONE stream): lets a single-problem launch with few column tiles and a long reduction (N <=
 *   1536, K >= 2048: context_fc, fc2) share the reduction of a tile between 2 / 4 workgroups that combine inside the launch
 *   (write-through partial tiles, an agent-scope arrival counter per tile - never reset -, the last arrival sums the
 *   slices in slice order: deterministic).  NULL = every workgroup owns its whole reduction.  Taken only with option "sk_split"
 *   = 1 (default 0: with the operands staged through LDS the unsplit form is as fast). */
int tell_skinny_linear(int n_prob, const void* const* in, long ld_in, int pro, const void* const* gamma,
                       const void* const* beta, int seg, float eps, float* stats_out, void* ws, const void* const* w,
                       long ldw, const void* const* bias, int act, float scale, const void* res, long ld_res,
                       const float* res_raw, long ld_res_raw, const float* res_stats, const float* res_gamma,
                       const float* res_beta, const float* res_f32, long ld_res_f32, void* out2, long ld_out2,
                       int out2_from, void* const* out, long ld_out, int out_f32, int M, int N, int K, void* split_ws,
                       long split_ws_bytes, tell_stream_t stream);
/* y (bf16) = LayerNorm(x) of fp32 rows [M, C], C = 1024 .. 4096; stats_out (optional): (mean, rstd) per row [M][2]. */
int tell_layernorm_rows(const float* x, long ld_x, const float* gamma, const float* beta, float eps, void* y, long ld_y,
                        float* stats_out, int M, int C, tell_stream_t stream);
/* Front half of the step's token embedding (adaptive.py:61-76 + positional.py:167-211 at T = 1): cat[m] (bf16 [M, ktot])
 * = the token's band-table row placed at columns off_b .. off_b + dim_b - 1 of its band b (zeros elsewhere), pos_out[m]
 * (fp32 [M,E]) = the sinusoid row of this step (pad -> row pos_pad; offset start_pos + the captured step's device
 * counter).  scale * (cat . [proj_0 | proj_1 | ..]^T) + pos_out - one tell_skinny_linear - is the embedding.
 * tables / lo / hi / dim / off: HOST arrays of nb <= 4 bands (ids lo_b .. hi_b - 1). */
/* the step's embedding as a LOOKUP in a pre-projected table (generation: the weights do not move): table fp32 [V, E] =
 * embed_scale * proj_band . table_band[v] for every token (adaptive.py:61-76, built once by the caller);
 * out[m] = bf16(table[ids[m]] + sinusoid[position of this step]) (positional.py:167-211; pad -> row pos_pad).  First kernel
 * of a captured decode step: reads / publishes the position counter like tell_embed_gather_step. */
int tell_embed_lookup_step(const long* ids, int M, const float* table, int V, const float* pos_table, int pos_rows,
                           int pos_pad, int start_pos, void* out, int E, tell_stream_t stream);
int tell_embed_gather_step(const long* ids, int M, int nb, const void* const* tables, const int* lo, const int* hi,
                           const int* dim, const int* off, void* cat, int ktot, const float* pos_table, int pos_rows,
                           int pos_pad, int start_pos, float* pos_out, int E, tell_stream_t stream);
/* DynamicConv1dTBC with an input buffer, one step (dynamic.py:85-120, :285-336 at T = 1): x [M,C] bf16, wt [H*K, C] bf16
 * (weight_linear, no bias), y [M,C] bf16.  C = H * 64, K <= 32.  hist [K][M][C] bf16 is a RING of K planes indexed by
 * time: the input of step s lives in plane s mod K, in the slot its hypothesis had at step s; planes never written hold
 * zeros (cleared by the caller per caption).  t = index of this step (+ the registered decode position counter while a
 * hipGraph of the step is recorded, tell_set_pos_step_ptr); the step reads planes t-1 .. t-K+1 and writes x into plane
 * t mod K.  back (optional): int32 [>= K-1][M], back[j-1][m] = slot, j steps ago, of the hypothesis now in slot m (beam
 * search, maintained by tell_beam_update); NULL = m itself. */
int tell_dynconv_step(const void* x, void* hist, const void* wt, void* y, int M, int C, int H, int K, int t,
                      const int* back, tell_stream_t stream);
/* MultiHeadAttention at Tq = 1 against n_ctx <= 4 static key / value caches in one launch (multi_head.py:330-352,
 * :376-475): HOST arrays of n_ctx entries; q[c] / out[c] [B, H*64] with row strides q_sb / o_sb, element (b,s,h,d) of
 * k[c] at k + s*k_ss + (b / beams)*k_sb + h*64 + d (the `beams` hypotheses of a sample - rows b*beams + j - share its
 * cache), mask[c] [B / beams, S[c]] uint8 or NULL, bias_k[c] / bias_v[c] [H*64] (:355-364) or NULL, has_zero: the zero
 * row (:416-421).  bf16, q pre-scaled, S <= 2048 (S = 0 allowed with a bias / zero row: the empty context :349-374). */
/* The same attention over a PACKED cache, on the matrix cores (the generation loop owns its cache's layout):
 *   both operands in MFMA FRAGMENT ORDER (a wave-wide 16-byte load reads one contiguous KB); the learned bias_k / bias_v row
 *      and the zero row (multi_head.py:355-364, :416-421) are keys S and S + 1, keys up to Sp (a multiple of 32) are zero;
 *   kc [B/beams, H, Sp/16, 2, 64, 8] bf16 keys: per tile of 16 keys and half c of the head width, lane l holds elements
 *      c * 32 + (l >> 4) * 8 .. + 7 of key l & 15;
 *   vt [B/beams, H, Sp/32, 4, 64, 8] bf16 values TRANSPOSED: per block of 32 keys and tile rt of 16 dimensions, lane l holds
 *      dimension rt * 16 + (l & 15) of the keys 4 g + j (j < 4) and 16 + 4 g + j - 4 (j >= 4), g = l >> 4 - the keys whose scores
 *      an MFMA accumulator leaves in k-group g (host mirror: transform-and-tell_amd/decode.py PackedKV.fill);
 *   mask [B/beams, Sp] uint8, 1 = masked (context padding and every position past S + 1).
 * q[c] bf16 [B, H*64] projected and scaled, out[c] bf16 [B, H*64]; head width 64; the beams hypotheses of a sample are
 * columns of one MFMA (any beams).  HOST arrays of n_ctx <= 4 entries. */
int tell_attn_decode_packed(int n_ctx, const void* const* q, const long* q_sb, const void* const* kc, const void* const* vt,
                            const void* const* mask, const int* Sp, void* const* out, const long* o_sb, int B, int H,
                            int beams, tell_stream_t stream);
int tell_attn_decode(int n_ctx, const void* const* q, const long* q_sb, const void* const* k, const long* k_ss,
                     const long* k_sb, const long* k_sh, const void* const* v, const long* v_ss, const long* v_sb,
                     const long* v_sh, const void* const* mask, const void* const* bias_k, const void* const* bias_v,
                     int has_zero, const int* S, void* const* out, const long* o_sb, int B, int H, int beams,
                     tell_stream_t stream);
/* tell_attn_decode + the HEAD-AVERAGED ATTENTION WEIGHTS of the step (multi_head.py:478-482; what the reference's generate()
 * returns per generated word, transformer_faces_objects.py:142-309).  Everything up to `beams` is tell_attn_decode's.  Contract:
 *   - out[c] is bit-identical to what tell_attn_decode writes for the same arguments (the same kernel; its exporting form only
 *     ADDS one store per (context, row, head): the base-2 log-sum-exp, into lse_ws - a workspace of n_ctx * B * H floats);
 *   - row b of context c receives S[c] + 2 floats at w[c] + slot * w_st[c] + b * w_sb[c] (strides in floats, w_sb[c] >=
 *     S[c] + 2): w[s] = (1/H) * sum_h softmax_h(s); columns 0 .. S-1 are the cached keys, column S the learned bias_k key,
 *     column S + 1 the zero key.  A masked key - and the bias / zero column when bias_k[c] is NULL / has_zero is 0 - is exactly
 *     0.0f.  S = 0 writes the two virtual columns only;
 *   - slot = slot_host + *step_dev (step_dev NULL: slot_host - the convention of tell_dynconv_step's t): an eager step passes
 *     its index, a captured step the index it was captured at minus the counter's value then, plus the device word that the
 *     step's bookkeeping launch moves along, so one captured step and a graph of several steps write a fresh slot per replay.
 *     0 <= slot < n_slots is checked on the host (step_dev NULL) and on the device (outside: nothing is written);
 *   - beams == 1 (an error otherwise: beam search would need the ancestor walk of tell_beam_update applied to the slots);
 *   - no atomic on a float: the sum over the heads runs in a register, head 0 first, so a row's weights are the same bits
 *     whatever the batch size, the launch mode (eager, captured) and the run.
 * Two launches: the one-pass attention in its exporting form, then one workgroup per (row, context, 128 columns) that
 * recomputes q_h . k_h[s] head by head from the K cache (never V) and accumulates exp2(score * log2 e - lse2_h).
 * bf16, head width 64, n_ctx <= 4, S <= 2048, row-major [S, B, E] and head-major (k_sh) caches. */
int tell_attn_decode_weights(int n_ctx, const void* const* q, const long* q_sb, const void* const* k, const long* k_ss,
                             const long* k_sb, const long* k_sh, const void* const* v, const long* v_ss, const long* v_sb,
                             const long* v_sh, const void* const* mask, const void* const* bias_k,
                             const void* const* bias_v, int has_zero, const int* S, void* const* out, const long* o_sb,
                             int B, int H, int beams, float* lse_ws, float* const* w, const long* w_st, const long* w_sb,
                             int slot, int n_slots, const int* step_dev, tell_stream_t stream);
/* n LayerNorms over ONE residual in one launch each way - the end of a decoder layer's context block
   (decoder_faces_objects.py:283-352): y[:, i*C:(i+1)*C] = LayerNorm_i(res + dropout_p(x_i)), mean / rstd [n, rows].
   Backward: dx_i (entries may be NULL), dres = sum_i dz_i (may be NULL), dgamma_i / dbeta_i ACCUMULATED; partial is a
   workspace of n * tell_layernorm_bwd_blocks(rows) * 2 * C floats.  x, gamma, beta, dx, dgamma, dbeta, salts are HOST
   arrays of n (<= 8) entries; every x_i / dx_i shares one row stride.  bf16, C = 512 or 1024, 16-byte aligned rows. */
int tell_layernorm_cat_fwd(int n, const void* const* x, long ld_x, const void* res, long ld_r,
                           const float* const* gamma, const float* const* beta, void* y, long ld_y, float* mean,
                           float* rstd, int rows, int C, float eps, float p, uint32_t seed, const uint32_t* salts,
                           int dtype, tell_stream_t stream);
int tell_layernorm_cat_bwd(int n, const void* dcat, long ld_dcat, const void* const* x, long ld_x, const void* res,
                           long ld_r, const float* const* gamma, const float* mean, const float* rstd,
                           void* const* dx, long ld_dx, void* dres, long ld_dres, float* const* dgamma,
                           float* const* dbeta, float* partial, int rows, int C, float p, uint32_t seed,
                           const uint32_t* salts, int dtype, tell_stream_t stream);

/* ---- LSTM decoder of the GloVe/LSTM baseline (tell/models/decoder_flattened_lstm.py) ----
 * nn.LSTMCell (:20-26, :160-161): g1 = x W_ih^T + b_ih and g2 = h W_hh^T + b_hh come from tell_gemm_nt ([B,4H], chunk
 * order i f g o); this applies the gate non-linearities and the state update.  gates: [B,4H] fp32, activated (saved). */
int tell_lstm_cell_fwd(const void* g1, const void* g2, const void* c_prev, void* h, void* c, float* gates, int B, int H,
                       int dtype, tell_stream_t stream);
/* dh / dc may be NULL; dgates ([B,4H], the gradient of both g1 and g2) and dc_prev are written */
int tell_lstm_cell_bwd(const void* dh, const void* dc, const float* gates, const void* c, const void* c_prev,
                       void* dgates, void* dc_prev, int B, int H, int dtype, tell_stream_t stream);
/* AttentionLayer.forward (:40-60) between its two projections: scores[l,b] = <src[l,b,:], x[b,:]>, key-padding mask
 * ([B,L] uint8, may be NULL), softmax over l, ctx[b,:] = sum_l probs[l,b] src[l,b,:].  src element (l,b,d) at
 * l*src_stride_l + b*src_stride_b + d; probs: [L,B] fp32 (the returned attention scores, saved); L <= 1024. */
int tell_dot_attn_fwd(const void* src, long src_stride_l, long src_stride_b, const void* x, const unsigned char* mask,
                      void* ctx, float* probs, int L, int B, int D, int dtype, tell_stream_t stream);
/* gradient w.r.t. the projected query x and - dsrc != NULL, contiguous [L,B,D] - w.r.t. the source states (needed when
 * they are the trainable `weigh_bert` mix of the RoBERTa layers, expt/3_lstm_roberta) */
int tell_dot_attn_bwd(const void* src, long src_stride_l, long src_stride_b, const float* probs, const void* dctx,
                      const void* x, void* dx, void* dsrc, int L, int B, int D, int dtype, tell_stream_t stream);
/* torch.tanh around output_proj (:62) */
int tell_tanh_fwd(const void* x, void* y, long n, int dtype, tell_stream_t stream);
int tell_tanh_bwd(const void* dy, const void* y, void* dx, long n, int dtype, tell_stream_t stream);

/* ---- DynamicConv1dTBC core, tell/modules/convolutions/dynamic.py:285-336 (T x B x C)
 * taps = softmax_K(logits) (:302-304), DropConnect (:305), causal K-tap weighted sum;
 * replaces the band-matrix build + bmm (:318-335).  taps: [T*B*H, K] fp32 (saved for backward). */
int tell_dynconv_fwd(const void* x, const void* logits, void* y, float* taps, int T, int B, int H, int K,
                     int R, float p, uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);
int tell_dynconv_bwd(const void* x, const void* dy, const float* taps, void* dx, int dx_accumulate,
                     void* dlogits, int T, int B, int H, int K, int R, float p, uint32_t seed, uint32_t salt,
                     int dtype, tell_stream_t stream);
/* The core of the decoder's conv block as one launch (decoder_faces_objects.py:259-261 GLU + dynamic.py:300-336):
 * h1 [T*B, 2E] bf16 = linear1's output (a | gate), w_tap [H*K, E] bf16 = DynamicConv.weight_linear (no bias) ->
 * gl = GLU(h1) [T*B, E], y [T*B, E], taps [T*B*H, K] fp32 (softmax of the tap logits, before DropConnect: what
 * tell_dynconv_bwd reads).  Replaces tell_glu_fwd + the tap-logit tell_gemm_nt + tell_dynconv_fwd; the logits stay
 * fp32 on the chip.  Returns 1 (nothing launched) for shapes it does not take: bf16 only, T <= 32, K <= 32, head
 * width 64, E = 1024. */
int tell_dynconv_block_fwd(const void* h1, const void* w_tap, void* gl, void* y, float* taps, int T, int B, int H,
                           int K, float p, uint32_t seed, uint32_t salt, tell_stream_t stream);

/* ---- MultiHeadAttention core, tell/modules/attention/multi_head.py:376-475
 * element (b,h,t,d) of q at q + t*q_st + b*q_sb + h*D + d (k, v, out likewise);
 * bias_k/bias_v (:355-364) and the zero row (:416-421) are virtual keys S, S+1;
 * mask [B,S] uint8 (:442-458); fp32 softmax (:460-462); prob dropout (:463). */
int tell_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse, const uint8_t* mask,
                  const void* bias_k, const void* bias_v, int B, int H, int Tq, int S, int D, long q_st,
                  long q_sb, long k_ss, long k_sb, long v_ss, long v_sb, long o_st, long o_sb, int has_zero,
                  float p, uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);
/* dbias_k / dbias_v: fp32 [B, H*D] per-sample partials of the bias_k / bias_v gradients (the caller sums over B), each
   with row stride H*D - or, when dbias_v == dbias_k + H*D, the two column halves of one [B, 2*H*D] buffer. */
int tell_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                  const float* lse, const uint8_t* mask, const void* bias_k, const void* bias_v, void* dq,
                  void* dk, void* dv, float* dbias_k, float* dbias_v, int B, int H, int Tq, int S, int D,
                  long q_st, long q_sb, long k_ss, long k_sb, long v_ss, long v_sb, long o_st, long o_sb,
                  int has_zero, float p, uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);

/* head-averaged attention weights [B,Tq,S'] for need_weights (multi_head.py:478-482), eval/demo only */
int tell_attn_avg_weights(const void* q, const void* k, const float* lse, const uint8_t* mask,
                          const void* bias_k, float* w, int B, int H, int Tq, int S, int D, long q_st, long q_sb,
                          long k_ss, long k_sb, int has_zero, int dtype, tell_stream_t stream);

/* ---- adaptive input embedding / adaptive softmax ----------------------------
 * tell_adaptive_partition: device-side replacement of the boolean-mask / nonzero()
 * logic of adaptive.py:64-74 and softmax.py:144-167 (adapt_target). */
int tell_adaptive_partition(const long* ids, int N, const int* cutoffs_host, int n_bands, int pad_idx,
                            int* band_rows, int* band_local, int* band_count, int* slot, int* head_target,
                            int* n_valid, tell_stream_t stream);
/* out = scale * band_out[slot] + sinusoid[pos], positional.py:167-211,231-268, sum_text_field_embedder.py:117-118 */
int tell_embed_finalize(const void* band_out, const int* slot, const long* ids, const float* pos_table,
                        int pos_rows, void* out, int B, int T, int E, float scale, int pos_pad, int start_pos,
                        int tbc, int dtype, tell_stream_t stream);
int tell_embed_finalize_bwd(const void* dout, const int* slot, void* dband, int B, int T, int E, float scale,
                            int tbc, int dtype, tell_stream_t stream);
int tell_embed_table_grad(const void* drows, long ld, const int* local, const int* count_dev, int cap,
                          float* demb, int dim, int padding_idx, int dtype, tell_stream_t stream);
/* F.cross_entropy(ignore_index, reduction='sum') per cluster, adaptive_loss.py:55-60 */
int tell_ce_fwd(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                const int* m_dev, int ignore_index, float* lse, float* loss, tell_stream_t stream);
int tell_ce_bwd(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                const int* m_dev, int ignore_index, const float* lse, const float* gscale_dev, void* dlogits,
                long ld_d, int dtype, tell_stream_t stream);
/* The two calls above with one weight per row: w fp32 indexed by UNCOMPACTED row, w_idx int32 or NULL - the weight of
 * compacted row i is w[w_idx ? w_idx[i] : i] (the head passes NULL, a tail the row list tell_gather_rows compacted with).
 * Forward: lse[i] is tell_ce_fwd's value bit for bit, loss[i] ONE fp32 multiply of the weight with the value tell_ce_fwd
 * writes; ignored rows and rows >= *m_dev get 0.  Backward: row i is bit for bit what tell_ce_bwd writes with *gscale
 * replaced by the fp32 product *gscale * weight, formed once per row; ignored rows and rows past *m_dev as in tell_ce_bwd. */
int tell_ce_fwd_weighted(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                         const int* m_dev, int ignore_index, const float* w, const int* w_idx, float* lse, float* loss,
                         tell_stream_t stream);
int tell_ce_bwd_weighted(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                         const int* m_dev, int ignore_index, const float* w, const int* w_idx, const float* lse,
                         const float* gscale_dev, void* dlogits, long ld_d, int dtype, tell_stream_t stream);
/* get_log_prob + topk(1), softmax.py:193-222, transformer_faces_objects.py:443-464 */
/* the k (<= 8) best (token, log-prob) pairs per row, best first - what a beam of k needs from each hypothesis;
 * `tokens`, `lps`: [rows, k] */
int tell_adaptive_logprob_topk(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                               int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                               int rows, int k, int* tokens, float* lps, tell_stream_t stream);
/* tell_adaptive_logprob_topk under a ban list per row: ban int32 [rows, ld_ban], n_ban int32 [rows] (tell_decode_ban_list).
 * The tokens ban[r][0 .. n_ban[r]) have log-prob -inf: they never enter the list.  Every other log-prob is exactly the one
 * tell_adaptive_logprob_topk returns - the log-sum-exps run over the whole row, nothing is renormalised - under the same
 * tie rule (lower id first); n_ban[r] = 0 gives its row bit for bit.  If fewer than k tokens remain, the tail of the list is
 * (-inf, 0x7fffffff).  k = 1..8 (k = 1: the greedy decode under bans); vocab <= 2^18; register and streaming forms as
 * tell_adaptive_logprob_topk (option argmax_regs). */
int tell_adaptive_logprob_topk_banned(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                      int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                      int rows, int k, const int* ban, long ld_ban, const int* n_ban, int* tokens,
                                      float* lps, tell_stream_t stream);
/* tell_adaptive_logprob_topk over PENALISED scores.  pen_tok / pen_cnt int32 [rows, ld_pen], n_pen int32 [rows]: the row's
 * list of (token t, count c_t) pairs (tell_decode_token_counts; at most 256 entries are read, tokens outside the vocabulary
 * are ignored, a token is listed once); sub fp32 [n_sub] on the device, which the host builds as sub[0] = 0,
 * sub[c] = float32(float64(alpha) + float64(beta) * c) (counts are clamped to n_sub - 1); theta finite, >= 1.  With lp_t the
 * log-prob tell_adaptive_logprob_topk / _argmax computes for t (the log-sum-exps run over the whole row, nothing is
 * renormalised), the score is
 *     s_t = lp_t                               for a token that is not listed (c_t = 0)
 *     s_t = min(lp_t, 0) * theta - sub[c_t]    for a listed one: a multiply and a subtract, two fp32 operations rounded one by
 *                                              one (never an FMA); the min keeps s_t <= lp_t
 * and the result is the k best (s, token) of the row, value descending, lower id first on ties; lps holds s.  n_pen[r] = 0
 * gives the row of tell_adaptive_logprob_topk bit for bit, and so does a list with theta = 1 and sub = 0 wherever lp <= 0.
 * k = 1..8 (k = 1: the greedy decode under penalties); vocab <= 2^18; register and streaming forms as
 * tell_adaptive_logprob_topk (option argmax_regs). */
int tell_adaptive_logprob_topk_penalised(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                         int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                         int rows, int k, const int* pen_tok, const int* pen_cnt, long ld_pen,
                                         const int* n_pen, float theta, const float* sub, int n_sub, int* tokens, float* lps,
                                         tell_stream_t stream);
/* tell_adaptive_logprob_topk under a VOCABULARY MASK (definition at tell_decode_vocab_mask): mask uint32 [rows / per, ld_mask >=
 * words], row r reads mask row r / per (rows % per == 0 is required); bits past the vocabulary are ignored.  ban / ld_ban / n_ban
 * as tell_adaptive_logprob_topk_banned, ORed into the row's mask (ban == NULL or n_ban == NULL: no list), so
 * no_repeat_ngram_size / min_len combine with a mask in one launch.  An all-zero mask without a list is
 * tell_adaptive_logprob_topk bit for bit.  A row with fewer than k allowed tokens ends in (-inf, 0x7fffffff) entries.
 * k = 1..8; vocab <= 2^18; register and streaming forms as tell_adaptive_logprob_topk (option argmax_regs). */
int tell_adaptive_logprob_topk_masked(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                      int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                      int rows, int k, const uint32_t* mask, long ld_mask, int per, const int* ban,
                                      long ld_ban, const int* n_ban, int* tokens, float* lps, tell_stream_t stream);
/* CONTEXT GUIDANCE: the pick of a decode step whose batch holds every caption twice.  `rows` conditional
 * rows r = 0 .. rows - 1; the partner of row r - the same caption decoded with some contexts dropped - is row r + pair_offset
 * of the same logit buffers (pair_offset >= rows).  With lp_c, lp_u the full log-probs of the two rows as
 * tell_adaptive_logprob_argmax computes them, and gamma = *gamma_dev (a device float, read by the kernel: a captured step
 * serves every gamma):
 *     d = lp_c - lp_u;  t = (gamma - 1) * d;  s = lp_c + t     three fp32 operations rounded one by one, never an FMA
 *     L = log sum_v exp(s(v)) over the whole vocabulary (max-shifted, fp32);  g = s - L
 * The result is the k best tokens of the pair ranked by s, value descending, lower id first on ties, reported with g (a
 * normalised log-prob), written to tokens / lps [.., k] at row r AND at row r + pair_offset.  gamma = 1, or u == c, makes s
 * equal lp_c bit for bit: the tokens are then those of tell_adaptive_logprob_topk.  s_rows: optional fp32 [rows, ld_s >= vocab],
 * the full s of every pair (NULL: not written).  k = 1..8 (k = 1: the guided arg-max); register and streaming forms as
 * tell_adaptive_logprob_topk (option argmax_regs). */
int tell_adaptive_logprob_topk_guided(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                      int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                      int rows, long pair_offset, int k, const float* gamma_dev, float* s_rows, long ld_s,
                                      int* tokens, float* lps, tell_stream_t stream);
int tell_adaptive_logprob_argmax(const float* head, long ld_head, int c0, int n_tails, const float* tail0,
                                 long ld0, int n0, const float* tail1, long ld1, int n1, const float* tail2,
                                 long ld2, int n2, int rows, float* log_probs, long ld_lp, int* token,
                                 float* token_lp, tell_stream_t stream);
/* forced tokens (caption completion): runs BEHIND the pick kernel of the step (arg-max, banned top-k,
 * sample, nucleus, beam top-k) over the tokens int32 / lps fp32 [rows, k] it has just written, k = 1..8, with the same logits.
 * prefix int64 [n_samples, P] (ld_prefix), plen int32 [n_samples]: the tokens a sample's caption starts with (after <s>).
 * Row r belongs to sample (row_ids ? row_ids[r] : r) / beams; the step index i is `step`, or *step_dev + 1 when step_dev is
 * given (the device counter of a captured decode step).  A row with i < min(plen[sample], P) is FORCED:
 *   tokens[r][0] = prefix[sample][i]; lps[r][0] = that token's log-prob exactly as tell_adaptive_logprob_argmax writes it
 *   (logit - lse_head; a tail token adds head_lsm[c0 + c] - lse_tail; no temperature, no renormalisation, no ban list) -
 *   bit for bit token_lp where the forced token is the arg-max; entries 1 .. k - 1 become (-inf, pad).  `pad` must be a token
 *   of the vocabulary: tell_beam_update lets a (-inf) candidate survive as a filler hypothesis when a sample has fewer than K
 *   finite candidates, and its token is the next step's embedding lookup.
 * Every other row is FREE: left as the pick kernel wrote it, its workgroup leaves before it requests a logit.  Only the head
 * and the forced token's own tail are reduced; register / streaming forms and capacity rule of tell_adaptive_logprob_argmax. */
int tell_adaptive_logprob_forced(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                 int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                 int rows, int k, const long* prefix, long ld_prefix, int P, const int* plen,
                                 int n_samples, const int* row_ids, int beams, int step, const int* step_dev, int pad,
                                 int* tokens, float* lps, tell_stream_t stream);
/* per-token statistics: runs BEHIND the step's pick launch - and behind tell_adaptive_logprob_forced
 * when there is a prefix - over the same logits.  chosen int32 [rows, ld_chosen]: column 0 is the token the step took (the
 * pick kernels' tokens buffer as it stands); finished uint8 [rows] or NULL; n = 1..8 alternatives.  The statistics are those
 * of the MODEL'S OWN distribution (no temperature, penalty, mask or guidance), lp_t as tell_adaptive_logprob_argmax /
 * tell_adaptive_logprob_topk compute it (head: head[t] - lse_h; tail i: tail[j] + ((head[c0 + i] - lse_h) - lse_i); maxima
 * and sums in the order of the top-k kernel of the same form, option argmax_regs).  Slot s of the outputs is `step`, or
 * *step_dev + 1 when step_dev is given (the device counter of a captured decode step - the convention of
 * tell_adaptive_logprob_forced).  Row r, with c = chosen[r][0], writes
 *   alt_tok int32 / alt_lp fp32 [slots, rows, n]: bit for bit what tell_adaptive_logprob_topk(k = n) returns on these buffers
 *     (value descending, lower id first; (0x7fffffff, -inf) where the vocabulary has fewer than n tokens);
 *   chosen_lp fp32 [slots, rows]: lp_c;
 *   rank int32 [slots, rows]: #{t : lp_t > lp_c or (lp_t == lp_c and t < c)} on the kernel's own fp32 values, 0 = the arg-max;
 *     so rank < n implies alt_tok[rank] == c and alt_lp[rank] == chosen_lp, and rank >= n that c is no alternative;
 *   entropy fp32 [slots, rows], in nats, by the chain rule: per cluster H = log s - u / s with s = sum exp(x - m),
 *     u = sum exp(x - m) * (x - m); H = H_head + sum_i exp(head[c0 + i] - lse_h) * H_tail_i; fp32 in a fixed order (a thread's
 *     elements in static order, the wave, the waves).  Logits are finite; nothing is promised for +-inf.
 * A row with finished[r] != 0 writes (pad, 0, -1, 0, 0) to (alt_tok, alt_lp, rank, entropy, chosen_lp) and requests no logit.
 * c outside [0, V): rank = -1 and chosen_lp = 0; alternatives and entropy are still written.  With step_dev, a slot outside
 * [0, slots) writes nothing.  Declined with a negative code and no launch: step outside [0, slots) without step_dev, n
 * outside 1..8, rows < 1, n_tails > 3, a NULL output.  Synchronises nothing, allocates nothing.  Register form (one
 * 1024-thread workgroup per row, the logits requested once) under the capacity rule of tell_adaptive_logprob_argmax;
 * otherwise the streaming form on the streaming top-k kernel's 256 threads. */
int tell_adaptive_logprob_stats(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                int rows, const int* chosen, long ld_chosen, const uint8_t* finished, int n, int slots,
                                int step, const int* step_dev, int pad, int* alt_tok, float* alt_lp, int* rank,
                                float* entropy, float* chosen_lp, tell_stream_t stream);
/* top-k sampling with a temperature (transformer_faces_objects.py:38-55, 443-470: lprobs.topk(k), / T, torch.multinomial).
 * Per row r at step i with seed s:
 *   1. candidates: the k (1..64) largest log-probs of the full adaptive softmax, each computed as in
 *      tell_adaptive_logprob_argmax (v = logit - lse_head; a tail adds head_lsm[c0 + c] - lse_tail), ordered by value
 *      descending, lower token id first on ties - k = 1 is the arg-max token, k <= 8 the list of tell_adaptive_logprob_topk;
 *   2. weights w_j = exp((lp_j - lp_0) * inv_temp) in fp32, cumulative sums c_j added in candidate order (the distribution
 *      of multinomial(exp(topk_lp / T)): multinomial normalises);
 *   3. u in [0, 1): 24 bits of a 32-bit counter-based hash of (s, row, step) (tell_sample_uniform_host);
 *   4. the pick: the smallest j with u * c_{k-1} < c_j, clamped to k - 1;
 *   5. out: tokens[r] = id_j, lps[r] = lp_j WITHOUT the temperature (tell_greedy_update multiplies by inv_temp).
 * row = row_ids[r] (the ORIGINAL batch row of a compacted row) or r when row_ids is NULL; step = *step_dev + 1 when step_dev
 * is given (the device counter of a captured decode step, which holds i - 1 during step i), else `step`; the seed is read
 * from DEVICE memory (*seed_dev), so a captured graph never bakes it in.  The draws are not torch.multinomial's: the
 * distribution and the reported log-probs match the reference, the sampled ids do not match draw for draw.
 * tokens int32 [rows], lps fp32 [rows].  Register-resident rows (the capacity and alignment of the register arg-max) take one
 * kernel; any other row (or option argmax_regs = 0) a streaming kernel with the arithmetic of the full-row arg-max. */
int tell_adaptive_logprob_sample(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                 int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                 int rows, int k, float inv_temp, const uint32_t* seed_dev, const int* row_ids, int step,
                                 const int* step_dev, int* tokens, float* lps, tell_stream_t stream);
/* tell_adaptive_logprob_sample over the penalised scores s of tell_adaptive_logprob_topk_penalised (same list arguments):
 * the candidates are the k (1..64) largest s (value descending, lower id first), the weights exp((s_j - s_0) * inv_temp),
 * u(seed, row, step) and the pick as above; out: the token and its s WITHOUT the temperature.  k = 1 is the penalised
 * arg-max bit for bit.  vocab <= 2^18. */
int tell_adaptive_logprob_sample_penalised(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                           int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2,
                                           int n2, int rows, int k, float inv_temp, const uint32_t* seed_dev,
                                           const int* row_ids, int step, const int* step_dev, const int* pen_tok,
                                           const int* pen_cnt, long ld_pen, const int* n_pen, float theta, const float* sub,
                                           int n_sub, int* tokens, float* lps, tell_stream_t stream);
/* tell_adaptive_logprob_sample under a VOCABULARY MASK (mask, ld_mask, per as tell_adaptive_logprob_topk_masked; launch row r
 * reads mask row r / per whatever row_ids says): the candidates are the k (1..64) best tokens that are not masked, the draw and
 * the reported log-prob as above.  Every row must keep at least k allowed tokens (the host guarantees 64).  k = 1 is the masked
 * arg-max bit for bit.  vocab <= 2^18. */
int tell_adaptive_logprob_sample_masked(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                        int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                        int rows, int k, float inv_temp, const uint32_t* seed_dev, const int* row_ids,
                                        int step, const int* step_dev, const uint32_t* mask, long ld_mask, int per,
                                        int* tokens, float* lps, tell_stream_t stream);
/* steps 2-5 above on given candidates: cand_tokens int32 / cand_lps fp32 [rows, k], each row sorted best first */
int tell_sample_candidates(const int* cand_tokens, const float* cand_lps, int rows, int k, float inv_temp,
                           const uint32_t* seed_dev, const int* row_ids, int step, const int* step_dev, int* tokens,
                           float* lps, tell_stream_t stream);
/* nucleus (top-p) sampling with a temperature over the full adaptive softmax.  Per row, with the
 * log-probs lp_t of tell_adaptive_logprob_argmax, inv_temp = 1 / T, 0 < p <= 1 and k = 0 (no top-k cut) or 2..64:
 *   1. weights w_t = exp((lp_t - lp_max) * inv_temp); with k > 0 only the k best tokens (value descending, lower id first on
 *      ties: the candidates of tell_adaptive_logprob_sample) keep a weight;
 *   2. the nucleus: the shortest prefix of that order whose weight sum reaches p * (total weight); tokens that tie at the
 *      boundary enter in id order until the sum is reached; the best token is always a member;
 *   3. the draw: u(seed, row, step) as above, scaled by the nucleus' weight sum; the pick is the first member IN TOKEN-ID
 *      ORDER whose running weight sum exceeds it (the last member if rounding leaves none).  Id order, not value order, so
 *      that the nucleus - thousands of tokens for a flat distribution - is never sorted.  Consequence: a (k, p = 1) call and
 *      tell_adaptive_logprob_sample(k) draw from the same distribution but map the same u to different ids;
 *   4. out: tokens[r] and lps[r] = lp of the pick WITHOUT the temperature (tell_greedy_update multiplies by inv_temp).
 * p = 1, k = 0 is multinomial sampling from the tempered softmax; p -> 0 is the arg-max (bit for bit).  Weight sums that
 * decide the boundary are exact 64-bit fixed-point sums of the fp32 weights (2^-44 of the largest weight is the unit: a
 * token lighter than that counts as zero), so a row's nucleus does not depend on the batch or on the launch mode.
 * nuc_size / nuc_key (optional, NULL in the product path): per row the number of members and the order-preserving key
 * (u = bits of lp; lp < 0: ~u, else u | 2^31) of the smallest member log-prob.  row_ids, step, step_dev, seed_dev and the
 * register / streaming forms as for tell_adaptive_logprob_sample; vocab < 2^19. */
int tell_adaptive_logprob_nucleus(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                  int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                  int rows, int k, float inv_temp, float p, const uint32_t* seed_dev, const int* row_ids,
                                  int step, const int* step_dev, int* tokens, float* lps, int* nuc_size,
                                  uint32_t* nuc_key, tell_stream_t stream);
/* steps 2-4 above on given candidates (cand_tokens int32 / cand_lps fp32 [rows, k], each row sorted best first, k 1..64) */
int tell_nucleus_candidates(const int* cand_tokens, const float* cand_lps, int rows, int k, float inv_temp, float p,
                            const uint32_t* seed_dev, const int* row_ids, int step, const int* step_dev, int* tokens,
                            float* lps, tell_stream_t stream);
/* two more truncation rules over the full adaptive softmax, no top-k cut.  Shared, per row: lp_t as
 * in tell_adaptive_logprob_argmax; a_t = (lp_t - lp_max) * inv_temp, one fp32 subtract then one fp32 multiply; w_t =
 * exp(a_t).  The draw (u(seed, row, step) scaled by the members' weight sum, the first member IN TOKEN-ID ORDER whose
 * running weight exceeds it, the last member if rounding leaves none), tokens / lps (the pick's lp WITHOUT the temperature),
 * row_ids, step, step_dev, seed_dev, the register / streaming forms and vocab < 2^19 as for tell_adaptive_logprob_nucleus.
 *
 * min-p: a token is a member iff a_t >= log_minp, log_minp = float32(log(m)) formed by the caller in fp64, 0 < m <= 1 (so
 * log_minp <= 0).  The comparison follows the multiply directly - nothing can be contracted, numpy float32 restates the
 * member set exactly.  The best token (a = 0) is always a member; m = 1 keeps the tokens tied with the maximum.  No
 * threshold search: the maximum, the members' weight sum (64-bit fixed point, as the nucleus masses), the id-order draw.
 * nuc_size (optional): the number of members per row. */
int tell_adaptive_logprob_minp(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                               int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                               int rows, float inv_temp, float log_minp, const uint32_t* seed_dev, const int* row_ids,
                               int step, const int* step_dev, int* tokens, float* lps, int* nuc_size,
                               tell_stream_t stream);
/* locally typical sampling, 0 < tau <= 1:
 *   1. W = sum w_t and S = sum w_t * a_t, fp32 in a fixed order (a thread's elements in static order, the wave, the 16 waves
 *      in order); c = -S / W >= 0: the entropy of the tempered distribution minus the surprise of its best token;
 *   2. d_t = |a_t + c| (the add is a single rounded fp32 add, never an FMA with the multiply of a_t: given c, numpy float32
 *      restates d_t bit for bit): the distance between the token's surprise and the entropy;
 *   3. members: the shortest prefix of the order (d ascending, lower id first on ties) whose weight reaches tau * (total
 *      weight); at least one token; tokens that tie at the boundary enter in id order until the mass is reached.  The
 *      boundary is found as the nucleus' (exact 2^44 fixed-point histogram masses over a quarter-nat digit of d, then the
 *      bytes of the key); the key of a token is ~bits(d): larger is better, never 0.  The masses weigh a token with
 *      exp((a_t + c) - c), i.e. a_t after one rounding at the size of c (a relative 2^-24 * c of the weight);
 *   4. the draw and the outputs as above.
 * nuc_size, nuc_key (the key of the worst member) and typ_c (fp32, the c of step 1) are optional, NULL in the product path. */
int tell_adaptive_logprob_typical(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                  int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                  int rows, float inv_temp, float tau, const uint32_t* seed_dev, const int* row_ids,
                                  int step, const int* step_dev, int* tokens, float* lps, int* nuc_size,
                                  uint32_t* nuc_key, float* typ_c, tell_stream_t stream);

/* per-token bookkeeping of the greedy decode loop (transformer_faces_objects.py:443-494) for all B rows in one launch:
   unfinished rows record tok / lp * inv_temp at step i, rows emitting eos are marked finished (done_step = i + 1),
   cur = tok for the next step.  tok int32 [B], lp fp32 [B], finished uint8 [B], ids int64 [B, ld_ids], lps fp32
   [B, ld_lps], done_step int64 [B], cur int64 [B].  counter (optional): device int32 that a captured decode step reads
   as its position offset (tell_set_pos_step_ptr); set to i, the offset of step i + 1.  step_dev (optional): the launch is
   PART of a captured step - the step index is *step_dev + 1 instead of i. */
int tell_greedy_update(const int* tok, const float* lp, uint8_t* finished, long* ids, long ld_ids, float* lps,
                       long ld_lps, long* done_step, long* cur, int B, int i, int eos, float inv_temp, int* counter,
                       const int* step_dev, tell_stream_t stream);

/* ---- BertAdam (config.yaml:126-149), flat fp32 buffers, tensors CHUNK-aligned */
int tell_opt_chunk(void);
/* shadow_bf16 (may be NULL): bf16 copy of the updated parameters, same flat layout - the working weights of the
 * next forward; zero_grad: clear the gradient buffer in the same pass (callback_apex_trainer.py:214);
 * grad_wire_bf16 (may be NULL): the step's gradient in bf16, same flat layout - what a data-parallel exchange with
 * bf16 on the wire leaves behind; it is then READ instead of `grad` (which is still the buffer that gets cleared). */
int tell_bertadam_step(float* param, float* grad, float* m, float* v, const int* chunk_tensor,
                       const long* chunk_begin, long n_chunks, int n_tensors, float* partial, float* norms,
                       const float* lr_dev, float b1, float b2, float eps, float wd, float max_norm,
                       float grad_scale, void* shadow_bf16, int zero_grad, int* skip, const void* grad_wire_bf16,
                       int* step_dev, float lr_base, float warmup, float t_total, tell_stream_t stream);
/* The same step with keep_grad (device int32[n_tensors], may be NULL): tensors with keep_grad[t] != 0 are NOT zeroed by
 * zero_grad - their single weight-gradient product of the next backward pass stores over them (accumulate = 0), which
 * saves the 4 B / parameter zero write here and the 4 B / parameter read there.  The host side (training/optimizers.py,
 * ops.wgrad_target) decides per tensor from who wrote what in an observed first step. */
int tell_bertadam_step2(float* param, float* grad, float* m, float* v, const int* chunk_tensor,
                        const long* chunk_begin, long n_chunks, int n_tensors, float* partial, float* norms,
                        const float* lr_dev, float b1, float b2, float eps, float wd, float max_norm,
                        float grad_scale, void* shadow_bf16, int zero_grad, int* skip, const void* grad_wire_bf16,
                        int* step_dev, float lr_base, float warmup, float t_total, const int* keep_grad,
                        tell_stream_t stream);
/* The same step, which also keeps an exponential moving average of the masters.  ema: flat fp32,
 * same layout as param, 16-byte aligned; ema_omd_dev: one device float, scratch for this step's 1 - d_t.  With n =
 * *step_dev before this launch increments it: d_t = ema_decay when ema_warm <= 0 or step_dev is NULL, else
 * min(ema_decay, (1 + n) / (ema_warm + n)), in double from the fp32 arguments; omd = (float)(1 - d_t) goes to
 * *ema_omd_dev in a single-thread launch next to the learning-rate one; per element e' = fmaf(omd, p' - e, e) in fp32
 * with p' the master this step has just computed.  A skipped step (skip[0] != 0) leaves ema untouched and, as step_dev
 * does not advance, costs no tick of this schedule either.  Everything else is bit for bit what tell_bertadam_step2
 * writes from the same inputs; the padding between tensors stays +0 in ema.  Refused (negative code, nothing launched,
 * nothing written, *lr_dev and *ema_omd_dev included): ema or ema_omd_dev NULL, ema not 16-byte aligned, ema_decay
 * outside [0, 1) or not finite, ema_warm negative or not finite, and whatever tell_bertadam_step2 refuses. */
int tell_bertadam_step_ema(float* param, float* grad, float* m, float* v, const int* chunk_tensor,
                           const long* chunk_begin, long n_chunks, int n_tensors, float* partial, float* norms,
                           const float* lr_dev, float b1, float b2, float eps, float wd, float max_norm,
                           float grad_scale, void* shadow_bf16, int zero_grad, int* skip, const void* grad_wire_bf16,
                           int* step_dev, float lr_base, float warmup, float t_total, const int* keep_grad,
                           float* ema, float* ema_omd_dev, float ema_decay, float ema_warm, tell_stream_t stream);
/* The same step with per-tensor hyperparameters (parameter groups), still one update launch.
 * group_hp: HOST array of n_groups rows (lr_base, warmup, t_total, b1, b2, eps, wd, max_norm), 1 <= n_groups <= 16; it is
 * validated here and travels into the kernels by value, so nothing of the host's has to outlive the call or a captured
 * graph.  tensor_group: device int32[n_tensors], the row of tensor t (an index outside 0..n_groups-1 counts as row 0).
 * lr_dev: n_groups device floats; with step_dev the schedule launch writes lr_dev[g] for every row from the one shared
 * *step_dev, without it the caller's lr_dev[g] are used.  The norm pass runs iff any row has max_norm > 0 and then covers
 * every tensor, as does its non-finite flag; a tensor is clipped iff its own row's max_norm > 0; the skip is global and
 * *step_dev advances once per applied step.  ema and ema_omd_dev may be NULL together: no average, ema_decay / ema_warm
 * ignored.  Within every chunk of a tensor of row g the call writes bit for bit what tell_bertadam_step2 (tell_bertadam_
 * step_ema with an average) writes when called with row g's eight values.  Refused (negative code, nothing launched,
 * nothing written): n_groups outside 1..16, tensor_group / group_hp / lr_dev NULL, a row with eps <= 0, one of ema /
 * ema_omd_dev NULL and the other not, and whatever tell_bertadam_step_ema refuses. */
int tell_bertadam_step_groups(float* param, float* grad, float* m, float* v, const int* chunk_tensor,
                              const long* chunk_begin, long n_chunks, int n_tensors, float* partial, float* norms,
                              float* lr_dev, const int* tensor_group, const float* group_hp, int n_groups,
                              float grad_scale, void* shadow_bf16, int zero_grad, int* skip, const void* grad_wire_bf16,
                              int* step_dev, const int* keep_grad, float* ema, float* ema_omd_dev, float ema_decay,
                              float ema_warm, tell_stream_t stream);
/* One pass over n elements (a whole number of tell_opt_chunk() chunks): param and ema exchange values, shadow_bf16 (may
 * be NULL) becomes the round-to-nearest-even bf16 of the new param.  Applied twice it restores all three buffers bit for
 * bit.  Values move and no pointer changes, so captured graphs that hold these buffers stay valid.  param, ema 16-byte
 * aligned, shadow_bf16 8-byte aligned; a refused call launches nothing and writes nothing. */
int tell_ema_swap(float* param, float* ema, void* shadow_bf16, long n, tell_stream_t stream);
/* step_dev (device int32, may be NULL): the count of updates APPLIED so far.  When given, the library first writes
 * *lr_dev = lr_base * warmup_linear(*step_dev / t_total, warmup) (t_total <= 0: lr_base) and the update kernel
 * increments *step_dev only when the step is not skipped - a skipped batch costs no tick of the schedule, exactly as in
 * the reference, where it never reaches optimizer.step().  NULL: the caller filled *lr_dev itself. */
/* skip (int[2], may be NULL): skip[0] != 0 -> the step leaves parameters / moments untouched (gradient still cleared)
 * and skip[1] counts such steps; tell_loss_flag sets skip[0] = !isfinite(loss) (the NaN-loss skip of
 * callback_apex_trainer.py:225-227 without a host sync), the norm pass ORs in 2 for a non-finite gradient (what apex
 * amp O2's overflow check does).
 * Limits: the gradient is inspected by the norm pass only - with max_norm <= 0 (no clipping) a NaN / Inf gradient is
 * NOT detected and goes into m, v and the parameter of its element (tell_loss_flag still covers a non-finite loss); a
 * finite gradient whose scaled sum of squares overflows fp32 counts as non-finite and skips the step.  eps must be
 * positive (refused otherwise: the zero padding between tensors would become 0 / 0).  param, grad, m, v 16-byte
 * aligned, shadow_bf16 and grad_wire_bf16 8-byte aligned; a refused call launches nothing and writes nothing. */
int tell_loss_flag(const float* loss, int* skip, tell_stream_t stream);

/* ---- ResNet-152 trunk helpers, tell/models/resnet.py:92-108 (NHWC) ----------- */
/* ToTensor + Normalize(mean, std) of the dataset readers (nytimes_faces_ner_matched.py:67-69) on the device:
 * uint8 [B,H,W,3] -> float32 [B,3,H,W] */
int tell_image_normalize(const uint8_t* x, float* y, int B, int H, int W, float m0, float m1, float m2, float s0,
                         float s1, float s2, tell_stream_t stream);
int tell_nchw_to_nhwc(const float* x, void* y, int B, int C, int H, int W, int out_dtype, tell_stream_t stream);
/* fp32 NCHW (C <= 4) -> bf16 NHWC with FOUR channels per pixel (missing ones zero): the input of the implicit 7x7 stem
 * (resnet.py:92-96) - tell_conv_bn_stats / tell_conv_bn_act / tell_conv_bias_act called with Cin = 4, KH = KW = 7,
 * stride 2, pad 3 and w [Cout, 256] laid out as 8 kernel rows (the 8th zero) x 8 window columns (the FIRST zero: the
 * window of output column ow starts at input column 2 ow - 4) x 4 channels (the 4th zero); W must be even. */
int tell_nchw_to_nhwc4(const float* x, void* y, int B, int C, int H, int W, tell_stream_t stream);
/* conv (1x1 / 3x3, stride 1 / 2, Cin = 64 * 2^n; or the 7x7 stem, see tell_nchw_to_nhwc4) as an IMPLICIT GEMM on the matrix cores + the statistics of the
 * train-mode BatchNorm behind it (resnet.py:92-108: torchvision Bottleneck conv -> bn; BN in batch-stat mode per
 * callback_apex_trainer.py:259): no im2col matrix, no statistics pass over the activation.  x [B,H,W,Cin] bf16,
 * w [Cout, KH*KW*Cin] bf16, y [B*OH*OW, Cout] bf16 raw conv output; mean / invstd [Cout] (+ running stats update), or
 * mean == NULL for the convolution alone.  workspace: 2 * ceil(B*OH*OW / 64) * Cout floats; zero_page: >= 16 zero
 * bytes, 16-byte aligned (source of the padding ring). */
int tell_conv_bn_stats(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int KH, int KW, int stride,
                       int pad, int OH, int OW, int Cout, float eps, float momentum, float* mean, float* invstd,
                       float* running_mean, float* running_var, float* workspace, const void* zero_page,
                       tell_stream_t stream);
/* conv -> train-mode BatchNorm (-> + residual) (-> ReLU) of a Bottleneck (resnet.py:92-108 via torchvision; the frozen
 * trunk runs in train mode, callback_apex_trainer.py:259): the implicit-GEMM convolution of tell_conv_bn_stats, then the
 * combine of the per-row-chunk statistics AND the normalisation as ONE launch (two when the activation has more than
 * 128 row chunks).  y [B*OH*OW, Cout] bf16 receives the finished activation; residual (same shape) or NULL;
 * running_mean / running_var get the momentum update.  workspace: 2 * ceil(M / 64) * Cout + 258 * Cout floats (chunk statistics, mean / invstd, and the
 * super-chunk statistics of the > 128-chunk case: one parallel merge launch in front of the fused finish + apply). */
int tell_conv_bn_act(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int KH, int KW, int stride,
                     int pad, int OH, int OW, int Cout, float eps, float momentum, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, const void* residual, int relu, float* workspace,
                     const void* zero_page, tell_stream_t stream);
/* the same block with the trunk in eval mode (running statistics): BatchNorm folded into the convolution by the host
 * (w' = w * gamma / sqrt(running_var + eps), bias = beta - running_mean * that): y = act(conv(x, w') + bias [+ residual])
 * in ONE launch; relu = 1 with a residual gives relu(conv + bias + residual). */
int tell_conv_bias_act(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int KH, int KW, int stride,
                       int pad, int OH, int OW, int Cout, const float* bias, const void* residual, int relu,
                       const void* zero_page, tell_stream_t stream);
int tell_im2col(const void* x, void* col, int B, int H, int W, int Cin, int KH, int KW, int stride, int pad,
                int OH, int OW, int Kp, int dtype, tell_stream_t stream);
/* im2col of y = relu(BatchNorm(x)): the producer's normalisation is applied while gathering (resnet.py Bottleneck:
 * conv1 -> bn1 -> relu -> conv2); padding taps are zeros of the post-activation tensor. */
int tell_im2col_bn(const void* x, void* col, int B, int H, int W, int Cin, int KH, int KW, int stride, int pad,
                   int OH, int OW, const float* mean, const float* invstd, const float* gamma, const float* beta,
                   int relu, int dtype, tell_stream_t stream);
long tell_bn_chunks(long M);
/* conv (as GEMM over NHWC rows) + the batch statistics of the BatchNorm2d that follows it, in one pass: the GEMM
 * epilogue reduces each output tile's columns, a small second kernel combines the tiles (resnet.py:94-108 with
 * the trunk in train mode).  bf16 only; workspace: 2 * ceil(M/64) * N floats. */
int tell_gemm_bn_stats(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                       float eps, float momentum, float* mean, float* invstd, float* running_mean,
                       float* running_var, float* workspace, tell_stream_t stream);
int tell_bn_stats(const void* x, long M, int C, float eps, float momentum, float* mean, float* invstd,
                  float* running_mean, float* running_var, float* workspace, int dtype, tell_stream_t stream);
int tell_bn_apply(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                  const void* residual, void* y, long M, int C, int relu, int dtype, tell_stream_t stream);
int tell_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, int dtype,
                      tell_stream_t stream);

/* ---- RoBERTa input embedding (fairseq roberta.large, call site transformer_faces_objects.py:352) */
int tell_roberta_embed(const long* ids, int B, int S, int pad, const void* word, const void* posemb, int* pos_ws,
                       void* out, int E, int dtype, tell_stream_t stream);

int tell_mask_rows(void* x, const uint8_t* mask, long rows, int C, int dtype, tell_stream_t stream);

/* ---- copy mechanism of transformer_pointer / transformer_pointer_2 (csrc/copy.hip)
 * Copy attention (multi_head.py:14-204 multi_head_attention_score_forward): q [T,B,H*D] already scaled, element
 * (t,b,h,d) at q + t*q_st + b*q_sb + h*D + d; k [S,B,H*D] likewise (k_ss, k_sb); bias_k [H*D] and a zero key are the
 * virtual columns S, S+1; mask [B,S] uint8 (1 = padding -> -inf); fp32 softmax per head; dropout p on the per-head
 * weights (counter-based, index ((b*H+h)*T+t)*(S+2)+s); head mean.  w [B,T,S] fp32 drops the virtual columns and is
 * zero where proper [B,S] int8 < 1 (proper may be NULL).  lse [B,H,T] fp32.  D <= 64, S <= 512. */
int tell_copy_attn_fwd(const void* q, const void* k, const void* bias_k, const uint8_t* mask, const int8_t* proper,
                       float* w, float* lse, int B, int H, int T, int S, int D, long q_st, long q_sb, long k_ss,
                       long k_sb, float p, uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);
/* dw [B,T,S] fp32 -> dq (q's strides), dk (k's strides), dbias_k_rows [B*T, H*D] fp32 per-row partials of the bias_k
 * gradient (the caller sums the rows); delta [B,H,T] fp32 scratch.  The per-head probabilities are recomputed. */
int tell_copy_attn_bwd(const void* q, const void* k, const void* bias_k, const uint8_t* mask, const int8_t* proper,
                       const float* lse, const float* dw, void* dq, void* dk, float* dbias_k_rows, float* delta,
                       int B, int H, int T, int S, int D, long q_st, long q_sb, long k_ss, long k_sb, float p,
                       uint32_t seed, uint32_t salt, int dtype, tell_stream_t stream);
/* V = the number of distinct ids of cat(context_ids, targets) (transformer_pointer.py:264), counted with a bitmap
 * of ceil(vocab/32) words plus one flag word; *count is written on the device, -1 when an id lies outside [0, vocab)
 * (the reference's index_copy_ fails there; tell_copy_loss_fwd variant 2 then yields NaN). */
int tell_copy_vocab_count(const long* ctx_ids, long n_ctx, const long* targets, int B, int T, long tgt_sb, int vocab,
                          uint32_t* bitmap, int* count, tell_stream_t stream);
/* Fused copy loss (pointer_loss :253-313).  w [B,T,S] from tell_copy_attn_fwd, ctx_ids [B,S], targets / copy_mask
 * [B,T] (row strides tgt_sb, cm_sb).  Per entity row (copy_mask >= 1): p_t = the summed weight of the target id,
 * lp = log p_t (0 when p_t = 0); variant 1 (transformer_pointer) term = -lp, variant 2 (transformer_pointer_2)
 * term = -lp + log(sum_{p>0} p + V - n_pos), V = *vcount.  *loss = sum over entity indices i = 1 .. max of the mean term
 * of index i (NaN when an index in that range has no row, as in the reference).  term, p_target, z, scale: [B,T] fp32
 * kept for the backward (scale = 1 / the row index's count). */
int tell_copy_loss_fwd(const float* w, const long* ctx_ids, const long* targets, long tgt_sb, const long* copy_mask,
                       long cm_sb, const int* vcount, int variant, int B, int T, int S, float* term, float* p_target,
                       float* z, float* scale, float* loss, tell_stream_t stream);
/* dw [B,T,S] fp32 (assigned) from the device scalar *dloss */
int tell_copy_loss_bwd(const float* dloss, const float* w, const long* ctx_ids, const long* targets, long tgt_sb,
                       const long* copy_mask, long cm_sb, const float* p_target, const float* z, const float* scale,
                       int variant, int B, int T, int S, float* dw, tell_stream_t stream);
/* entity_fc + CrossEntropy(ignore_index=-1) against min(copy_mask, 1) (:211-228).  x: row (t,b) at t*x_st + b*x_sb,
 * E wide; w [2,E] fp32 (the weight-normed weight), bias [2] fp32.  logits [B,T,2] fp32, *loss, *nvalid fp32. */
int tell_entity_head_fwd(const void* x, long x_st, long x_sb, const float* w, const float* bias, const long* copy_mask,
                         long cm_sb, int B, int T, int E, float* logits, float* loss, float* nvalid, int dtype,
                         tell_stream_t stream);
/* the logits alone (the generation step): logits [B,T,2] fp32 */
int tell_entity_logits(const void* x, long x_st, long x_sb, const float* w, const float* bias, int B, int T, int E,
                       float* logits, int dtype, tell_stream_t stream);
/* dx (x's layout, assigned), dlogits [B,T,2] fp32 scratch, dw [2,E] fp32 (assigned), dbias [2] fp32 (accumulated). */
int tell_entity_head_bwd(const float* dloss, const float* nvalid, const float* logits, const long* copy_mask,
                         long cm_sb, const void* x, long x_st, long x_sb, const float* w, void* dx, long dx_st,
                         long dx_sb, float* dlogits, float* dw, float* dbias, int B, int T, int E, int dtype,
                         tell_stream_t stream);
/* Causal entity attention (self_attention.py, downsampled_single_head.py _mask_future_full + scalar_bias.py): query i
 * at position pos0 + i sees keys s < pos0 + i, plus a slot of logit 0 and value 0; no dropout; logits are
 * scale * q.k (q unscaled, dq likewise).  Layout as
 * tell_attn_fwd; D = 64; lse [B,H,Tq].  pos0 = S - 1, Tq = 1 is the generation step over a K/V history of S rows.
 * k and v hold S rows and no row >= S is read: a query with pos0 + i > S sees all S keys (min(pos0 + i, S)), a query
 * with pos0 + i = 0 sees the zero slot alone (out = 0, lse = 0 exactly).  Every entry point of this section returns a
 * negative code and launches nothing when it declines its arguments (D, S <= 512, p in [0,1), bias_k, dtype, variant,
 * a full history); tell_copy_step with Ba = 0 returns 0 and launches nothing. */
int tell_causal_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int H, int Tq,
                         int S, int D, int pos0, long q_st, long q_sb, long k_ss, long k_sb, long v_ss, long v_sb,
                         long o_st, long o_sb, float scale, int dtype, tell_stream_t stream);
/* training backward (Tq = S = T, pos0 = 0): dq (q's strides), dk / dv (k's / v's strides); delta [B,H,T] scratch */
int tell_causal_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                         const float* lse, void* dq, void* dk, void* dv, float* delta, int B, int H, int T, int D,
                         long q_st, long q_sb, long k_ss, long k_sb, long v_ss, long v_sb, long o_st, long o_sb,
                         float scale, int dtype, tell_stream_t stream);
/* The copy decision of one generation step (_generate :488-590) for Ba alive rows; rows [Ba] int32 = each alive row's
 * batch row.  q [Ba,H*D] (row stride q_sb, scaled); k [S,B,H*D] the article keys projected once per batch; copy
 * attention without dropout, proper mask, per-id sums, arg-max (ties to the lower id), top p < 1e-6 -> p = 1e-6 and no
 * copy, no copy of an id in hist[b, 0 .. n_hist) (hist [B, hist_len] int64), copy only where entity_logits [Ba,2]
 * has logit 1 > logit 0.  Writes tok [Ba] (the copied id or gen_tok), copied [Ba] uint8, prob [Ba] fp32 and
 * hist[b, n_hist] (the copied id, else -1). */
int tell_copy_step(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                   const uint8_t* mask, const int8_t* proper, const long* ctx_ids, const int* rows,
                   const float* entity_logits, const long* gen_tok, long* hist, int hist_len, int n_hist, int Ba, int H,
                   int S, int D, long* tok, uint8_t* copied, float* prob, int dtype, tell_stream_t stream);

/* ---- copy mechanism, cached generation (csrc/copy_decode.hip): the tail of a decode step of the copy
 * models over a batch that keeps its shape.  Both entry points take the step as `step, step_dev`: the step index p is
 * *step_dev + 1 when step_dev is given (the launch is part of a captured step, as in tell_greedy_update), else `step`.  They
 * return a negative code and launch nothing when they decline their arguments, synchronise nothing and allocate nothing.
 *
 * The one-query causal entity attention of step p over a STATIC history: q, k_new, v_new [B, H*64] (row strides q_sb, kn_sb,
 * vn_sb) are this step's projections (q unscaled, logits scale * q.k); k_hist, v_hist [L, B, H*64] (strides h_ss, h_sb; the
 * model dtype).  Row p of both histories is written from k_new / v_new bit for bit, the query sees rows 0 .. p-1 plus a slot
 * of logit 0 and value 0: out [B, H*64] (row stride o_sb) = tell_causal_attn_fwd(Tq = 1, pos0 = p, S = p), exactly 0 at
 * p = 0.  D = 64.  Host path: 0 <= step < L or the call is declined; device path: p >= L attends to all L rows and writes no
 * history row. */
int tell_entity_attn_step(const void* q, long q_sb, const void* k_new, long kn_sb, const void* v_new, long vn_sb,
                          void* k_hist, void* v_hist, long h_ss, long h_sb, void* out, long o_sb, int B, int H, int D,
                          int L, float scale, int step, const int* step_dev, int dtype, tell_stream_t stream);
/* tell_copy_step for a static batch: row r is batch row r (no row map); a row with finished[r] != 0 (uint8 [B], optional)
 * reads and writes nothing.  q [B,H*D] (row stride q_sb, scaled); k [S,B,H*D] by strides as in tell_copy_step; bias_k, mask,
 * proper, ctx_ids as there; entity_logits [B,2]; gen_tok int32 [B] (the head's pick).  The rules are tell_copy_step's, the
 * history check runs over hist[r, 0 .. p].  Unfinished rows get tok[r] (int32: the copied id or gen_tok[r] - what
 * tell_greedy_update takes), hist[r, p + 1] (int32 [B, ld_hist >= L + 1]: the copied id, else -1), copied[r, p + 1] (uint8
 * [B, ld_copied >= L + 1]) and prob[r, p] (fp32 [B, ld_prob >= L]).  Two launches: the per-head probabilities of every
 * (row, head) into scratch (fp32 [B, H, S]), then one workgroup per row.  S <= 512, D <= 64, bias_k required.  Host path:
 * 0 <= step < L or the call is declined; device path: p >= L writes nothing. */
int tell_copy_decide(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                     const uint8_t* mask, const int8_t* proper, const long* ctx_ids, const float* entity_logits,
                     const int* gen_tok, const uint8_t* finished, int* hist, long ld_hist, uint8_t* copied,
                     long ld_copied, float* prob, long ld_prob, int L, int step, const int* step_dev, int B, int H, int S,
                     int D, float* scratch, int* tok, int dtype, tell_stream_t stream);
/* tell_copy_decide for per_image = n hypotheses of every image (1..16; generate(n_samples=n) of the copy models, DESIGN.md
 * section 28): R = B * n rows, hypothesis j of image b is row r = b * n + j (the convention of tell_sample_rank).  R rows
 * tall: q, entity_logits, gen_tok, finished, hist, copied, prob, tok and scratch (fp32 [R, H, S]); B rows, read at
 * b = r / n: k [S,B,H*D], mask, proper, ctx_ids.  Every output of row r is, bit for bit, what tell_copy_decide writes for row
 * r of the same batch with every image's keys, mask, proper mask and ids repeated n times - prob included.  Launch 1, grid
 * (image, head, chunk of 4 hypotheses - all n when n < 4): a key's head slice is loaded once per workgroup and multiplied
 * with every query of the chunk; a workgroup whose hypotheses are all finished returns at once; a finished row reads and
 * writes nothing of its own.  Launch 2: one workgroup per row.  Limits, step / step_dev and declined calls as
 * tell_copy_decide. */
int tell_copy_decide_hyp(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                         const uint8_t* mask, const int8_t* proper, const long* ctx_ids, const float* entity_logits,
                         const int* gen_tok, const uint8_t* finished, int* hist, long ld_hist, uint8_t* copied,
                         long ld_copied, float* prob, long ld_prob, int L, int step, const int* step_dev, int B,
                         int per_image, int H, int S, int D, float* scratch, int* tok, int dtype, tell_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TELL_HIP_H */
