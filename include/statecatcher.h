/*
 * statecatcher.h — C ABI of libstatecatcher_hip.so, the MI355X (gfx950) hot path of the
 * stateful recurrent ASR step (LucyRNN scan fwd/bwd, decay scan, CTC alpha-beta, greedy
 * CTC decode).
 *
 * Every entry point takes plain device pointers, element counts/strides (in ELEMENTS, as the
 * reference's Triton launches do) and a hipStream_t passed as void*.  No torch types cross
 * this boundary.  All calls are asynchronous on `stream` and never synchronise the host.
 *
 * Return value: 0 on success; SC_EINVAL (-1) for an invalid argument (message in
 * sc_last_error()); a positive hipError_t if the launch failed.
 *
 * Reference interfaces replaced (paths under speechcatcher-asr/statecatcher):
 *   sc_lucy_scan_fwd  <- lucyrnn_triton.py:179-244 `rnn_forward_unfused_rmsnorm`,
 *                        launched at lucyrnn_triton.py:61-73 with grid (B, D)
 *   sc_lucy_scan_bwd  <- (absent in the reference) adjoint of the above
 *   sc_decay_scan_fwd <- lucyrnn_triton.py:158-177 `fused_decay_scan`, launched at
 *                        lucyrnn.py:147-151; generalised with an optional initial state
 *   sc_decay_scan_bwd <- (absent) adjoint of the above
 *   sc_layernorm_*    <- nn.LayerNorm between layers, lucyrnn_triton.py:96-97, :136-137
 *   sc_ln_fold_*, sc_lucy_scan_*_ln <- the same LayerNorm folded into the next layer's gate
 *                        projection (LN(h) W^T + b = rstd (h W''^T - mean r) + b')
 *   sc_ctc_*          <- ATen ctc_loss behind nn.CTCLoss(blank=0, zero_infinity=True),
 *                        train.py:142 / model.py:68-71
 *   sc_ctc_greedy_decode <- decoder.py:3-30 `ctc_greedy_decoder`
 *   sc_ctc_greedy_step   <- decoder.py:3-30 applied one frame at a time (streaming)
 *   sc_ctc_greedy_frames <- the same over a block of frames in one launch
 *   sc_fbank          <- make_frontend (model.py:250-279, applied at train.py:473-475):
 *                        torchaudio MFCC / MelSpectrogram + AmplitudeToDB (unpinned, absent)
 *   sc_lucy_step_*    <- the native LucyRNN's infer-mode frame loop, lucyrnn.py:172-184, i.e.
 *                        LucyRNNCell.forward (lucyrnn.py:44-70) at T = 1 (streaming decode)
 *   sc_mlstm_*        <- the xLSTM encoder's mLSTM cell (model.py:214-229, :301-307; fork kernels
 *                        "chunkwise--native_autograd", train.py:643-645), math as
 *                        transformers/models/xlstm/modeling_xlstm.py:74-386 (parity vs the fork
 *                        unpinned)
 *   sc_rnnt_*         <- warp_rnnt `rnnt_loss(log_probs, labels, frames_lengths, labels_lengths,
 *                        blank, compact, gather=True)` called at model.py:97-105 (train.py:38-42,
 *                        :144); the log_softmax of model.py:93 optionally fused
 *   sc_rnnt_greedy_decode <- (absent in the reference: decoder.py is CTC only) greedy decoding
 *                        of RNNTPredictorJoiner (model.py:112-145), offline and streaming
 *   sc_rnnt_beam_*    <- (absent in the reference) transducer beam search of the same joiner,
 *                        n-best with scores, offline and chunked
 *   sc_ctc_align      <- (absent in the reference; its README plans hallucination filtering) CTC
 *                        forced alignment: Viterbi path, token spans, per-frame / per-token scores
 *   sc_wkv_*          <- (planned in the reference's README, absent from its code) the RWKV-4 WKV
 *                        operator with carried state, math as transformers/models/rwkv/
 *                        modeling_rwkv.py `rwkv_linear_attention_cpu`
 *   sc_wkv_step, sc_rwkv_step_mix, sc_relu_sq <- the same model one frame at a time (RwkvBlock,
 *                        RwkvSelfAttention, RwkvFeedForward at T = 1) for streaming decode
 */
#ifndef STATECATCHER_H
#define STATECATCHER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_EINVAL (-1)

/* element types of floating tensors crossing the ABI */
#define SC_F32 0
#define SC_BF16 1
#define SC_F16 2

/*
 * Every `#define SC_NAME <integer>` and every declaration below is also read by the Python
 * binding (statecatcher_amd/_lib.py parses this file at import): keep to int, int64_t, size_t,
 * float, double and pointers.
 */

/* sc_abi_version() returns SC_ABI_VERSION; bump it on any signature or struct change (the
 * binding refuses a library built from another version of this file) */
#define SC_ABI_VERSION 14
int sc_abi_version(void);

/* most jobs one call takes: sc_lucy_frame_gemm_multi / _cellb_multi / sc_lucy_tframe_layer_multi,
 * sc_weight_images, sc_ln_fold_prep (callers with more split the list) */
#define SC_MAX_FRAME_JOBS 8
#define SC_MAX_IMAGE_JOBS 16
#define SC_MAX_FOLD_JOBS 16

/* sc_lucy_frame_gemm's epi */
#define SC_FRAME_PLAIN 0
#define SC_FRAME_STATS 1
#define SC_FRAME_CELL_UNFUSED 2
#define SC_FRAME_CELL_FUSED 3

/* sc_lucy_step_cell's mode */
#define SC_STEP_FUSED 0
#define SC_STEP_UNFUSED_A 1
#define SC_STEP_UNFUSED_B 2

/* sc_fbank's kind */
#define SC_FBANK_MFCC 0
#define SC_FBANK_MEL 1

/* Message for the last SC_EINVAL / launch failure on this thread ("" if none). */
const char* sc_last_error(void);

/* ---------------------------------------------------------------- LucyRNN scan ---------- */

/* Time steps per checkpointed super-chunk (state saved at each super-chunk start). */
int sc_lucy_scan_chunk(void);

/* Floats needed for the forward->backward state checkpoint: B * ceil(T/chunk) * 2 * D. */
int64_t sc_lucy_scan_ckpt_numel(int B, int T, int D);

/*
 * Forward scan.  Mirrors rnn_forward_unfused_rmsnorm(gates_ptr, h0_ptr, s0_ptr, out_ptr,
 * s_out_ptr, B, T, D, stride_g_bt, stride_g_td, stride_g_cd, stride_o_bt, stride_o_bd)
 * (lucyrnn_triton.py:180-194), plus one stride the reference does not have:
 *   gates  gate g (order r,z,k,v,h_pre,decay,alpha) of hidden unit d at step t of row b is at
 *            b*stride_g_bt + t*stride_g_td + g*stride_g_cd + (d/64)*stride_g_cb + d%64
 *          i.e. hidden units come in 64-wide column blocks.  The reference's [B,T,7,D] layout
 *          is stride_g_cb = 64.  The step-blocked layout [B,T,ceil(D/64),7,64] (stride_g_cd = 64,
 *          stride_g_cb = 448; what a projection GEMM writes when its weight rows are permuted
 *          accordingly) puts each step's 7 x 64 gates of one column block in one contiguous
 *          run, which the kernel streams in whole 16-byte pieces.
 *   gate_bias  NULL (gates already include the projection bias, as in the reference), or fp32
 *          [7,D] (logical order g*D + d) added to every step's gates on load (lets the
 *          projection GEMM skip its bias epilogue; the backward then needs the same pointer)
 *   h0,s0  [B,D] fp32 contiguous (read exactly as contiguous; the caller must not pass the
 *          strided out[:, -1] view the reference passes — SURVEY F3)
 *   out    [B,T,D] of gates_dtype, d-stride 1 (strides stride_o_bt, stride_o_bd)
 *   s_out  [B,D] fp32 contiguous: state after the last step
 *   h_out  NULL, or [B,D] fp32 contiguous: h after the last step in fp32 (the reference carries
 *          out[:, -1] in x.dtype = fp32; with a 16-bit out this keeps the carry unrounded)
 *   ckpt   NULL, or sc_lucy_scan_ckpt_numel() floats: (s,h) at every super-chunk start,
 *          consumed by sc_lucy_scan_bwd (training)
 * State arithmetic is fp32 for every gates_dtype.  Any element strides work; 16-byte aligned
 * gates with strides (and D) in multiples of 16 bytes take the wide-piece path.
 */
int sc_lucy_scan_fwd(const void* gates, int gates_dtype, const float* gate_bias,
                     const float* h0, const float* s0,
                     void* out, float* s_out, float* h_out, int B, int T, int D,
                     int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                     int64_t stride_g_cb, int64_t stride_o_bt, int64_t stride_o_bd, float* ckpt,
                     void* stream);

/*
 * sc_lucy_scan_fwd plus two 16-bit planes with out's strides: out_dup (the rounded h again) and
 * out_lo (h minus its rounding, rounded).  With out, out_dup, out_lo as the K blocks of one
 * [B*T][3D] operand, a bf16 GEMM against [W_hi | W_lo | W_hi] gives x.W with the error of an fp32
 * GEMM (the output projection before the CTC lattice, lucyrnn_triton.py:150 / model.py:70).
 * gates_dtype must be bf16 or f16.
 */
int sc_lucy_scan_fwd_split(const void* gates, int gates_dtype, const float* gate_bias,
                           const float* h0, const float* s0, void* out, void* out_dup, void* out_lo,
                           float* s_out, float* h_out, int B, int T, int D,
                           int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                           int64_t stride_g_cb, int64_t stride_o_bt, int64_t stride_o_bd,
                           float* ckpt, void* stream);

/*
 * sc_lucy_scan_fwd(_split) with the inter-layer LayerNorm (lucyrnn_triton.py:96-97, :136-137)
 * folded in.  16-bit gates, 16-byte pieces, D = 512 or 1024.  out_dup / out_lo: NULL, or the
 * split planes of sc_lucy_scan_fwd_split.
 *   ln_r       NULL, or fp32 [7,D]: this layer's gates are u = h W''^T of the RAW previous output h
 *              (W'' the bf16 image of sc_weight_images with col_scale = gamma, row_shift = the
 *              sc_ln_fold_prep shift) and r its row sums (sc_ln_fold_prep rowsum); each gate is
 *              rebuilt on load as rstd (u - mean r) + gate_bias, gate_bias = b' (sc_ln_fold_prep
 *              bias_out), which equals LN(h) W^T + b
 *   ln_rec_in  with ln_r: fp32 [B][T][D/64][2], (mean, M2) of h's 64-unit blocks (the previous
 *              layer's ln_rec_out); combined per row with Chan's formula, eps ln_eps
 *   ln_stat    NULL, or fp32 [B][T][2] out: the rows' (rstd, mean) (what sc_lucy_scan_bwd_ln and
 *              sc_ln_fold_bwd read)
 *   ln_rec_out NULL, or fp32 [B][T][D/64][2] out: (mean, M2) of this layer's 16-bit output
 *              values per 64-unit block, for the next layer's fold
 */
int sc_lucy_scan_fwd_ln(const void* gates, int gates_dtype, const float* gate_bias,
                        const float* h0, const float* s0, void* out, void* out_dup, void* out_lo,
                        float* s_out, float* h_out, int B, int T, int D,
                        int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                        int64_t stride_g_cb, int64_t stride_o_bt, int64_t stride_o_bd,
                        float* ckpt, const float* ln_r, const float* ln_rec_in, float* ln_stat,
                        float* ln_rec_out, float ln_eps, void* stream);

/*
 * Backward scan.  Inputs: the forward's gates and ckpt, dout = dL/d out (same dtype as gates,
 * strides stride_d_bt/stride_d_bd), ds_last = dL/d s_out (fp32 [B,D], may be NULL = zero).
 * Outputs: dgates (gates_dtype, laid out like gates with strides stride_dg_*), dh0, ds0 (fp32
 * [B,D]) and, if dbias is not NULL, dbias fp32 [B,7,D] = sum over t of the stored dgates (per
 * batch row; summing over b gives the gate-projection bias gradient without another pass over
 * dgates).
 */
int sc_lucy_scan_bwd(const void* gates, int gates_dtype, const float* gate_bias, const float* ckpt,
                     const void* dout, const float* ds_last,
                     void* dgates, float* dh0, float* ds0, float* dbias, int B, int T, int D,
                     int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                     int64_t stride_g_cb, int64_t stride_d_bt, int64_t stride_d_bd,
                     int64_t stride_dg_bt, int64_t stride_dg_td, int64_t stride_dg_cd,
                     int64_t stride_dg_cb, void* stream);

/*
 * Backward of sc_lucy_scan_fwd_ln's fold (16-bit, D = 512 or 1024, 16-byte aligned gates / dout /
 * dgates): the gates are rebuilt from ln_r, gate_bias and the forward's ln_stat; dgates =
 * dL/du = rstd dL/dgate (the input and weight gradients of u = h W''^T consume it); dbias keeps
 * dL/dgate (the gradient of b').  ln_r = NULL: the gates are sc_gemm_tn_ln_bf16's output, which
 * already holds rstd (u - mean r); the scan adds gate_bias (= b') alone, ln_stat is that GEMM's
 * stat, and dgates / dbias are as above.
 */
int sc_lucy_scan_bwd_ln(const void* gates, int gates_dtype, const float* gate_bias,
                        const float* ckpt, const void* dout, const float* ds_last, void* dgates,
                        float* dh0, float* ds0, float* dbias, int B, int T, int D,
                        int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                        int64_t stride_g_cb, int64_t stride_d_bt, int64_t stride_d_bd,
                        int64_t stride_dg_bt, int64_t stride_dg_td, int64_t stride_dg_cd,
                        int64_t stride_dg_cb, const float* ln_r, const float* ln_stat,
                        void* stream);

/*
 * The masked scan: sc_lucy_scan_fwd / sc_lucy_scan_fwd_split with a per-frame mask.
 *   mask   uint8 [B,T] contiguous, nonzero = live.  NULL is SC_EINVAL (callers without a mask
 *          use sc_lucy_scan_fwd).
 * A held frame (mask == 0) leaves (h, s) untouched and writes zero to out (and to out_dup /
 * out_lo); its gates are never used (selects, not products: they may hold NaN).  So a row's
 * result is the unmasked scan over its live frames, scattered back; s_out / h_out are the state
 * after the last live frame, and a row with no live frame returns (h0, s0).  h_out is therefore
 * not out[:, T-1].  out_dup / out_lo: both NULL, or the split planes (16-bit gates).  ckpt keeps
 * sc_lucy_scan_fwd's layout.  The LayerNorm-fold variants have no masked form.
 */
int sc_lucy_scan_fwd_masked(const void* gates, int gates_dtype, const float* gate_bias,
                            const float* h0, const float* s0, const uint8_t* mask, void* out,
                            void* out_dup, void* out_lo, float* s_out, float* h_out, int B, int T,
                            int D, int64_t stride_g_bt, int64_t stride_g_td, int64_t stride_g_cd,
                            int64_t stride_g_cb, int64_t stride_o_bt, int64_t stride_o_bd,
                            float* ckpt, void* stream);

/*
 * Backward of sc_lucy_scan_fwd_masked (same mask).  A held frame gets exactly zero in all 7 gate
 * planes of dgates and adds nothing to dbias; neither its gates nor its dout are used.
 *   dh_last  fp32 [B,D] = dL/d h_out, NULL = zero: the initial value of the Gh chain, the way
 *            ds_last starts Gs (it reaches the last LIVE step; it is not added onto dout[:, T-1]).
 * A row with no live frame returns dh0 = dh_last, ds0 = ds_last.
 */
int sc_lucy_scan_bwd_masked(const void* gates, int gates_dtype, const float* gate_bias,
                            const float* ckpt, const void* dout, const float* ds_last,
                            const float* dh_last, const uint8_t* mask, void* dgates, float* dh0,
                            float* ds0, float* dbias, int B, int T, int D, int64_t stride_g_bt,
                            int64_t stride_g_td, int64_t stride_g_cd, int64_t stride_g_cb,
                            int64_t stride_d_bt, int64_t stride_d_bd, int64_t stride_dg_bt,
                            int64_t stride_dg_td, int64_t stride_dg_cd, int64_t stride_dg_cb,
                            void* stream);

/* ---------------------------------------------------------------- decay scan ------------ */

/*
 * s_t = decay_t * s_{t-1} + kv_t with s_{-1} = init (init NULL -> 0, as fused_decay_scan).
 * Mirrors fused_decay_scan(kv_ptr, decay_ptr, output_ptr, B, T, D, stride_b, stride_t,
 * stride_d) (lucyrnn_triton.py:159-163); kv, decay and out share the strides, stride_d == 1.
 * init: fp32 [B,D] contiguous or NULL.  Accumulation fp32 (lucyrnn_triton.py:171).
 */
int sc_decay_scan_fwd(const void* kv, const void* decay, void* out, int dtype,
                      const float* init, int B, int T, int D,
                      int64_t stride_b, int64_t stride_t, int64_t stride_d, void* stream);

/*
 * Adjoint: g_t = dout_t + decay_{t+1} g_{t+1};  dkv_t = g_t;  ddecay_t = g_t * s_{t-1}
 * (s_{-1} = init).  s_all is the forward output.  dinit (fp32 [B,D]) may be NULL.
 */
int sc_decay_scan_bwd(const void* decay, const void* s_all, const void* dout, void* dkv,
                      void* ddecay, int dtype, const float* init, float* dinit,
                      int B, int T, int D, int64_t stride_b, int64_t stride_t, int64_t stride_d,
                      void* stream);

/* ---------------------------------------------------------------- LayerNorm ------------- */

/*
 * The stack's inter-layer nn.LayerNorm(D) (lucyrnn_triton.py:96-97, :136-137; eps 1e-5,
 * biased variance) in the activation dtype with fp32 statistics.  Rows of D contiguous
 * elements, 16-byte aligned; D must be 64 * (16 / element size) * {1, 2, 4, 8}
 * (sc_layernorm_supported).  gamma/beta fp32 [D]; mean/rstd fp32 [rows].
 */
int sc_layernorm_supported(int dtype, int D);
int sc_layernorm_fwd(const void* x, int dtype, const float* gamma, const float* beta, void* y,
                     float* mean, float* rstd, int64_t rows, int D, float eps, void* stream);

/* fp32 workspace floats needed by sc_layernorm_bwd (per-workgroup gamma/beta partial rows). */
int64_t sc_layernorm_bwd_workspace_numel(int64_t rows, int D);

/*
 * dx (dtype of x) and dgamma_dbeta fp32 [2, D] (row 0 dgamma, row 1 dbeta; fixed-order
 * reduction, deterministic) from x, dy and the forward's mean/rstd.
 */
int sc_layernorm_bwd(const void* x, const void* dy, int dtype, const float* gamma,
                     const float* mean, const float* rstd, void* dx, float* dgamma_dbeta,
                     float* workspace, int64_t rows, int D, void* stream);

/*
 * The LayerNorm fold around the scans (see sc_lucy_scan_fwd_ln).  Per job (one gate projection
 * W fp32 [rows = 7D][ld], the preceding LayerNorm's gamma / beta [D], the projection bias [rows]
 * or NULL), in one launch for up to SC_MAX_FOLD_JOBS jobs:
 *   shift[n] = mean_k gamma_k W_nk   (row_shift of the W'' image; W''_nk = bf16(gamma_k W_nk -
 *                                     shift_n), computed unfused, as sc_weight_images computes it)
 *   bias_out[n] = b_n + sum_k W_nk beta_k
 *   rowsum[n] = sum_k W''_nk
 */
typedef struct {
  const float* w;
  const float* gamma;
  const float* beta;
  const float* bias;
  float* shift;
  float* bias_out;
  float* rowsum;
  int64_t ld, rows, D;
} sc_ln_fold_job;
int sc_ln_fold_prep(const sc_ln_fold_job* jobs, int njobs, void* stream);

/*
 * dL/dh [rows][D] bf16 of the LayerNorm input h from g = dL/du W'' (the gate projection's input
 * gradient with the scan's rstd-scaled dgates) and the forward's stat [rows][2] (rstd, mean):
 * dh = g - mean(g) - xhat mean(xhat g), xhat = (h - mean) rstd.  D = 512 or 1024.
 */
int sc_ln_fold_bwd(const void* g, const void* h, int dtype, const float* stat, void* dh,
                   int64_t rows, int D, void* stream);

/* fp32 workspace floats of sc_ln_fold_wgrad. */
int64_t sc_ln_fold_wgrad_workspace_numel(int rows, int D);

/*
 * From M = dL/dW'' fp32 [rows][D] (reference row order) and dL/db' fp32 [rows]:
 * dw [rows][D] = gamma (M - rowmean M) + dL/db' beta^T  (dL/dW), and dgamma_dbeta fp32 [2][D] =
 * (sum_n W (M - rowmean M), sum_n W dL/db') in a fixed order.  (dL/db = dL/db'.)
 */
int sc_ln_fold_wgrad(const float* M, const float* w, int64_t ld, const float* gamma,
                     const float* beta, const float* dbias, int rows, int D, float* dw,
                     float* dgamma_dbeta, float* workspace, void* stream);

/* ---------------------------------------------------------------- CTC ------------------- */

/* Workspace bytes for sc_ctc_fwd / sc_ctc_bwd (alpha, beta, row log-sum-exp, label chains). */
size_t sc_ctc_workspace_bytes(int B, int T, int max_target_len);

/*
 * CTC forward over x [B,T,V] (x_dtype, v-stride 1, strides stride_b/stride_t):
 *   is_logits = 1: x are logits, log_softmax is fused (model.py:70 + ATen ctc_loss);
 *   is_logits = 0: x are log-probabilities (the nn.CTCLoss input convention).
 * targets: int64 [B, max_target_len] padded (train.py:208), row stride target_stride;
 * max_target_len <= 1007.  in_lens/tgt_lens: int64 [B] device arrays.  Writes nll [B] fp32 (+inf when infeasible;
 * the zero_infinity reduction is the caller's) and fills the workspace for sc_ctc_bwd.
 */
int sc_ctc_fwd(const void* x, int x_dtype, int is_logits, int B, int T, int V,
               int64_t stride_b, int64_t stride_t,
               const int64_t* targets, int64_t target_stride, int max_target_len,
               const int64_t* in_lens, const int64_t* tgt_lens, int blank,
               float* nll, void* workspace, size_t workspace_bytes, void* stream);

/*
 * CTC backward: grad [B,T,V] (grad_dtype, contiguous) =
 *   scale[b] * (exp(lp) - exp(lcab + nll - lp))  for t < in_len[b], 0 otherwise,
 * ATen's formula; with is_logits = 1 it is the gradient w.r.t. the logits.  scale: fp32 [B]
 * (dL/dnll_b, already zero where the loss was zeroed).
 */
int sc_ctc_bwd(const void* x, int x_dtype, int is_logits, int B, int T, int V,
               int64_t stride_b, int64_t stride_t,
               const int64_t* targets, int64_t target_stride, int max_target_len,
               const int64_t* in_lens, const int64_t* tgt_lens, int blank,
               const float* nll, const float* scale, void* grad, int grad_dtype,
               const void* workspace, size_t workspace_bytes, void* stream);

/*
 * sc_ctc_fwd / sc_ctc_bwd with the emission columns given exactly (is_logits = 1): ex fp32
 * [B][T][max_target_len + 1] (strides ex_stride_b, ex_stride_t; column stride 1), ex[b][t][0] =
 * the blank's logit, ex[b][t][1 + u] = label u's, replace x's values at those columns in the
 * lattice's emissions and in the gradient row (softmax term and occupancy); the row's
 * log-sum-exp still reads x.  For a bf16 output projection whose emission columns were computed
 * to fp32 accuracy (statecatcher_amd.ops.CTCHeadFn): the same head, model.py:68-71 +
 * lucyrnn_triton.py:150, with the logits' bf16 rounding kept out of the lattice.
 */
int sc_ctc_fwd_ex(const void* x, int x_dtype, int is_logits, int B, int T, int V,
                  int64_t stride_b, int64_t stride_t,
                  const int64_t* targets, int64_t target_stride, int max_target_len,
                  const int64_t* in_lens, const int64_t* tgt_lens, int blank,
                  const float* ex, int64_t ex_stride_b, int64_t ex_stride_t,
                  float* nll, void* workspace, size_t workspace_bytes, void* stream);
int sc_ctc_bwd_ex(const void* x, int x_dtype, int is_logits, int B, int T, int V,
                  int64_t stride_b, int64_t stride_t,
                  const int64_t* targets, int64_t target_stride, int max_target_len,
                  const int64_t* in_lens, const int64_t* tgt_lens, int blank,
                  const float* ex, int64_t ex_stride_b, int64_t ex_stride_t,
                  const float* nll, const float* scale, void* grad, int grad_dtype,
                  const void* workspace, size_t workspace_bytes, void* stream);

/*
 * The operand of the emission-logit GEMM of that head: out bf16 [B][max_target_len + 1][3 K],
 * row (b, c) = [bf16(w_r) | bf16(w_r - bf16(w_r)) | bf16(w_r)] with r = blank (c = 0) or
 * targets[b][c - 1] clamped into [0, V); bias_out fp32 [B][max_target_len + 1] = bias[r] (0 if
 * bias is NULL).  w fp32 [V][ldw], K % 4 == 0.  Against the last scan's [x_hi | x_hi | x_lo]
 * rows one bf16 GEMM gives the emission logits to ~2^-16 relative (lucyrnn_triton.py:150).
 */
int sc_ctc_split_rows(const float* w, int64_t ldw, const float* bias, int V, int K,
                      const int64_t* targets, int64_t target_stride, int max_target_len,
                      int blank, void* out, float* bias_out, int B, void* stream);

/*
 * The reduction nn.CTCLoss(reduction='mean', zero_infinity=True) applies to sc_ctc_fwd's nll
 * (train.py:142): loss[0] = mean_b(nll_b / max(U_b, 1)) with infinite nll_b counted as 0, and
 * factor[b] = d loss / d nll_b (0 for infinite nll_b), the `scale` sc_ctc_bwd takes times the
 * loss's upstream gradient.  nll, factor: fp32 [B]; tgt_lens int64 [B]; loss fp32 [1].
 */
int sc_ctc_mean(const float* nll, const int64_t* tgt_lens, int B, float* loss, float* factor,
                void* stream);

/* ---------------------------------------------------------------- greedy decode --------- */

/*
 * decoder.py:3-30 on device: argmax over V (first maximal index; NaN counts as maximal,
 * as torch.argmax), trim to lengths[b], collapse repeats, drop blank.
 * tokens: int32 [B,T] (first counts[b] entries valid), counts: int32 [B].
 */
int sc_ctc_greedy_decode(const void* log_probs, int dtype, int B, int T, int V,
                         int64_t stride_b, int64_t stride_t, const int64_t* lengths, int blank,
                         int32_t* tokens, int32_t* counts, void* stream);

/*
 * decoder.py:3-30 for ONE frame of B streams (streaming decode): tok = argmax of logits row b
 * (same tie/NaN rule); emit[b*emit_stride] = tok if the frame is live (mask null or mask[b] != 0)
 * and tok != blank and tok != prev[b], else -1; prev[b] = tok for live frames (start streams
 * with prev = -1, decoder.py's prev_token = None).  logits row stride stride_b (elements).
 */
int sc_ctc_greedy_step(const void* logits, int dtype, int B, int V, int64_t stride_b,
                       const float* mask, int blank, int32_t* prev, int32_t* emit,
                       int64_t emit_stride, void* stream);
/*
 * sc_ctc_greedy_step over F consecutive frames in one launch, frame f = 0 .. F-1 in order:
 * logits [F][B][V] (strides stride_f, stride_b), mask [F][B] (stride mask_f) or null, emit
 * [F][B] (strides emit_f, emit_b); prev carried from frame to frame as F calls would.
 */
int sc_ctc_greedy_frames(const void* logits, int dtype, int F, int B, int V, int64_t stride_f,
                         int64_t stride_b, const float* mask, int64_t mask_f, int blank,
                         int32_t* prev, int32_t* emit, int64_t emit_f, int64_t emit_b,
                         void* stream);

/* ---------------------------------------------------------------- streaming LucyRNN step -- */

/*
 * Native LucyRNN, infer mode, one frame (lucyrnn.py:172-184 -> LucyRNNCell.forward :44-70).
 * Per layer the caller runs a = input_proj(x) (GEMM), sc_lucy_step_ln (layernorm_in), the gate
 * GEMM, then sc_lucy_step_cell.  State h, s: fp32 [B,D] contiguous, updated in place.  All other
 * activations share `dtype` (f32/bf16/f16), rows contiguous except g (row stride g_stride).
 * 1 <= D <= 1024.  LayerNorm eps as given (nn.LayerNorm: 1e-5).
 */
int sc_lucy_step_supported(int dtype, int D);

/* y = LayerNorm(x; w, b) per row of D (layernorm_in, lucyrnn.py:45). */
int sc_lucy_step_ln(const void* x, int dtype, const float* w, const float* b, float eps, void* y,
                    int B, int D, void* stream);

/*
 * mode SC_STEP_FUSED (fused_ops, :47-54):  g = [z | k | v | h_pre | decay_logits] (5D per row; the
 *   reference's r chunk is computed and never used, so the caller drops W_fused's first D rows);
 *   s' = sigmoid(dl) s + k v;  c = tanh(LN_h(h_pre + s'));  h' = (1 - z~) c + z~ h with
 *   z~ = sigmoid(LN_z(z));  masked blend (:66-68) with mask[b];  out = new h.
 * mode SC_STEP_UNFUSED_A (unfused, :55-60):  g = [W_z u | W_k u | W_v u | W_decay u];  s updated
 *   as above;  out = u + s' (the input of W_h).
 * mode SC_STEP_UNFUSED_B (unfused, :61-68):  hp = W_h(u + s');  c = tanh(LN_h(hp));  z~ from g as
 *   in the fused mode;  h updated and masked;  out = new h.
 * LayerNorm pointers null = layer_norm False (nn.Identity).  mask: fp32 [B] or null.
 */
int sc_lucy_step_cell(int mode, const void* g, int dtype, int64_t g_stride, const void* u,
                      const void* hp, const float* lnz_w, const float* lnz_b, const float* lnh_w,
                      const float* lnh_b, float eps, float* h, float* s, void* out,
                      const float* mask, int B, int D, void* stream);

/*
 * The same frame as a chain of fused kernels (csrc/lucy_frame.hip; no library GEMM, no separate
 * LayerNorm launch).  Activations fp32; weights fp32 (fp32 MFMA, the reference's arithmetic) or
 * bf16 (bf16 MFMA).  LayerNorm statistics travel as (n, mean, M2, -) float4 records, [nrec][B].
 *
 * sc_lucy_frame_gemm: y[b][j] = sum_k x~[b][k] w[j][k] + bias[j], x~ = x or, when ln_w is given,
 *   LayerNorm(x) from the nst_in records of st_in (lucyrnn.py:45 layernorm_in).  epi:
 *   SC_FRAME_PLAIN  plain;
 *   SC_FRAME_STATS  plain + one statistics record of y per 32 columns into st_out
 *     ([ceil(N/32)][B]);
 *   SC_FRAME_CELL_UNFUSED  unfused gates (N = 4D: z k v decay, lucyrnn.py:55-59): s' =
 *     sigmoid(decay) s + k v into s (masked), y = x~ + s' ([B][D], K == D), z ([B][D]), records of
 *     z per 16 units into st_z;
 *   SC_FRAME_CELL_FUSED  fused gates (N = 5D: z k v h_pre decay; W_fused without its unused r
 *     rows, :47-53): s as above, y = h_pre + s', z, records of y into st_out and of z into st_z
 *     ([D/16][B] each).
 *   x 16-byte aligned with ldx % 4 == 0, K % 4 == 0; w 16-byte aligned with ldw % 8 == 0.
 * sc_lucy_frame_cellb: h = (1 - sigmoid(LN_z z)) tanh(LN_h hp) + sigmoid(LN_z z) h (masked,
 *   :61-68) in place, and out[b][:D] = h (the next layer's input).
 */
int sc_lucy_frame_gemm(int epi, const float* x, int64_t ldx, int K, const float* ln_w,
                       const float* ln_b, const void* st_in, int nst_in, float eps, const void* w,
                       int w_dtype, int64_t ldw, const float* bias, int B, int N, float* y,
                       int64_t ldy, void* st_out, float* z, void* st_z, float* s,
                       const float* mask, void* stream);
int sc_lucy_frame_cellb(const float* z, const void* st_z, int nst_z, const float* hp,
                        const void* st_h, int nst_h, const float* lnz_w, const float* lnz_b,
                        const float* lnh_w, const float* lnh_b, float eps, float* h, float* out,
                        int64_t ldo, const float* mask, int B, int D, void* stream);

/*
 * The same two kernels over up to SC_MAX_FRAME_JOBS independent jobs in ONE launch each: a block
 * of F frames of an L-layer model runs as a wavefront over (frame, layer) -- stage tau computes
 * layer l of frame tau - l for every l at once, since layer l of frame j needs only layer l - 1 of
 * frame j and layer l of frame j - 1 -- so a block takes 4 (F + L - 1) launches instead of 4 F L
 * (statecatcher_amd/streaming.py).  Each job has the arguments of one sc_lucy_frame_gemm / _cellb call; the
 * jobs of one call share epi, w_dtype, eps and the presence of the LayerNorm prologue.
 */
typedef struct sc_frame_gemm_job {
  const float* x;
  int64_t ldx;
  int K;
  const float* ln_w;
  const float* ln_b;
  const void* st_in;
  int nst_in;
  const void* w;
  int64_t ldw;
  const float* bias;
  int B, N;
  float* y;
  int64_t ldy;
  void* st_out;
  float* z;
  void* st_z;
  float* s;
  const float* mask;
} sc_frame_gemm_job;
int sc_lucy_frame_gemm_multi(int epi, int w_dtype, float eps, const sc_frame_gemm_job* jobs,
                             int njobs, void* stream);
typedef struct sc_frame_cell_job {
  const float* z;
  const void* st_z;
  int nst_z;
  const float* hp;
  const void* st_h;
  int nst_h;
  const float *lnz_w, *lnz_b, *lnh_w, *lnh_b;
  float* h;
  float* out;
  int64_t ldo;
  const float* mask;
  int B, D;
} sc_frame_cell_job;
int sc_lucy_frame_cellb_multi(float eps, const sc_frame_cell_job* jobs, int njobs, void* stream);

/*
 * One streaming frame of one LucyRNNtriton layer (lucyrnn_triton.py:27-75 at T = 1) for B streams
 * in ONE launch (csrc/lucy_frame.hip): g = x~ W^T + bias with W [7D][ldw] (fp32 or bf16), gate
 * planes r z k v h_pre decay alpha, x~ = x [B][ldx] over K columns or, when ln_w is given,
 * LayerNorm(x; ln_w, ln_b, eps) from the nst_in (n, mean, M2, -) records st_in [nst_in][B] that
 * the previous layer's launch wrote (the inter-layer nn.LayerNorm); then per (row b, unit d), in
 * fp32 with eps' = 1e-6 (lucyrnn_triton.py:214-242, the offline scan's arithmetic):
 *   rc = sqrt((r^2 + z^2)/2 + eps')   rkv = sqrt((k^2 + v^2)/2 + eps')
 *   z' = sigmoid(z / rc)   decay' = sigmoid(decay / sqrt(decay^2 + eps'))
 *   alpha' = sigmoid(alpha / sqrt(alpha^2 + eps'))   kv = (k/rkv)(v/rkv) / (rkv^2 + eps')
 *   s' = decay' s + alpha' kv   c = tanh(h_pre / sqrt(h_pre^2 + eps') + s')   h' = (1 - z') c + z' h
 * With fp32 weights the projection sums k in ascending order (two K slices, each one chain of
 * fp32 fmas): the rounding of a plain sgemm, which the reference module's goldens need.
 * h, s: fp32 [B][D] state, updated in place (rows with mask[b] == 0 keep both; mask fp32 [B] or
 * null).  out[b*ldo + d] = the new (or kept) h; st_out [D/16][B] float4 receives one record of
 * out per 16 units and row for the next layer's prologue, or is null (last layer).
 * D % 16 == 0; K % 4 == 0 (bf16 weights: % 8), K <= 2048; x, w, ln_w, ln_b 16-byte aligned with
 * ldx % 4 == 0, ldw % 8 == 0, both >= K; ln_w, ln_b and st_in together or not at all.  B == 0 is
 * a no-op.  No allocation, no atomics: captures into a HIP graph.
 *
 * sc_lucy_tframe_layer_multi: up to SC_MAX_FRAME_JOBS such jobs in one launch (blockIdx.z = job),
 * sharing w_dtype and eps; jobs with and without the prologue may mix (layer 0 has none).  A
 * block of F frames of an L-layer model is then F + L - 1 launches: stage tau = layer l of frame
 * tau - l for every l.
 * Within a launch the jobs run concurrently, so the caller double-buffers each layer's out /
 * st_out (the job of layer l - 1 writes frame j + 1 while layer l reads frame j).
 */
int sc_lucy_tframe_layer(const float* x, int64_t ldx, int K, const float* ln_w, const float* ln_b,
                         const void* st_in, int nst_in, float eps, const void* w, int w_dtype,
                         int64_t ldw, const float* bias, int B, int D, float* h, float* s,
                         float* out, int64_t ldo, void* st_out, const float* mask, void* stream);
typedef struct sc_tframe_job {
  const float* x;
  int64_t ldx;
  int K;
  const float* ln_w;
  const float* ln_b;
  const void* st_in;
  int nst_in;
  const void* w;
  int64_t ldw;
  const float* bias;
  int B, D;
  float* h;
  float* s;
  float* out;
  int64_t ldo;
  void* st_out;
  const float* mask;
} sc_tframe_job;
int sc_lucy_tframe_layer_multi(int w_dtype, float eps, const sc_tframe_job* jobs, int njobs,
                               void* stream);

/* ---------------------------------------------------------------- column sums ----------- */

/*
 * out[n] = sum_m x[m][n] in fp32, fixed summation order (deterministic), x row-major [M][ld]
 * (16-byte aligned rows) of dtype f32/bf16/f16.  The step's row reductions: the output
 * projection's bias gradient (dy.sum(0), lucyrnn_triton.py:8-25 Linear backward), split-K
 * weight-gradient partial sums, per-row gate-bias partials.  Optional block transpose of the
 * output index: with N = perm_a * perm_b * C, column (a, b, c) is written at (b, a, c)
 * (perm_a = perm_b = 1: identity).  workspace: sc_colsum_workspace_bytes(M, N) device bytes.
 */
size_t sc_colsum_workspace_bytes(int64_t M, int64_t N);
int sc_colsum(const void* x, int dtype, int64_t M, int64_t N, int64_t ld, int64_t perm_a,
              int64_t perm_b, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- weight-gradient GEMM -- */

/*
 * Split-L weight gradient of a projection: part[s] = A[Ls]^T B[Ls] (fp32 [I][J] slab per
 * L-split s) for A = dY bf16 [L][lda], B = X bf16 [L][ldb] — the backward of LinearSafe
 * (lucyrnn_triton.py:20-25: dW = dgates^T x) and of output_proj (lucyrnn_triton.py:107-109).
 * Sum the S slabs with sc_colsum (fixed order; it also un-permutes step-blocked rows).
 * Needs L % 64 == 0, J % 256 == 0, and I % 256 == 0 -- or I % 224 == 0 only at the 256-workgroup
 * shape (I/224)*(J/256)*8 == 256 (e.g. I = 3584 = 7 * 512 with J = 512) -- plus 16-byte aligned
 * operands and leading dimensions.  Gate on sc_gemm_wgrad_splits: it returns the split count
 * for a shape, 0 when unsupported (use a library GEMM).  part: S * I * J floats.
 */
int sc_gemm_wgrad_splits(int L, int I, int J);
int sc_gemm_wgrad_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, float* part, int L,
                       int I, int J, int S, void* stream);

/*
 * Frame-major projection GEMM C = A B^T, bf16 in / fp32 accumulate / bf16 out, for A [M][lda]
 * and B [N][ldb] both K-contiguous, C [M][ldc].  Replaces the library GEMMs of LinearSafe's
 * forward (lucyrnn_triton.py:20-25, gates = x W^T; layer 0's Din = 80 zero-padded to 128) and of
 * the input gradients (dx = dgates W as dgates (W^T)^T; output_proj's dh = dlogits Wo,
 * lucyrnn_triton.py:107-109).  Needs K % 64 == 0, N % 256 == 0, 16-byte aligned operands and
 * leading dimensions, every operand < 4 GiB.  tile_m: rows per tile, 0 (default 192), 128 or 192.
 * Deterministic (no atomics, fixed K order).  Returns 0, SC_EINVAL, or a HIP error code.
 */
int sc_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                    int M, int N, int K, int tile_m, void* stream);

/*
 * The gate projection of layers 1.. with the inter-layer LayerNorm folded in
 * (lucyrnn_triton.py:96-97 + :20-25: LinearSafe(LayerNorm(h))): C [M][ldc] bf16 =
 *   rstd (h W''^T - mean r) = LN(h) W^T - W beta      (the scan adds b' = b + W beta)
 * for H = the previous layer's RAW output [M][ldh] bf16 (K = D, the LayerNorm width), Wpp = the
 * W'' image [N][ldw] (sc_weight_images with a LayerNorm fold job, step-blocked rows), r [N] =
 * its row sums in the image's row order (sc_ln_fold_prep's rowsum, permuted like the rows).  Each
 * row's mean and rstd = 1 / sqrt(biased variance + eps) come from the rows as they stream
 * through the GEMM; stat [M] (float pairs (rstd, mean)) receives them for the backward
 * (sc_lucy_scan_bwd_ln with ln_r = NULL, sc_ln_fold_bwd).  K % 64 == 0, N % 256 == 0, 16-byte
 * aligned operands.  Replaces sc_layernorm_fwd + the projection GEMM.
 */
int sc_gemm_tn_ln_bf16(const void* H, int64_t ldh, const void* Wpp, int64_t ldw, void* C,
                       int64_t ldc, int M, int N, int K, const float* r, void* stat, float eps,
                       void* stream);

/* ---------------------------------------------------------------- optimizer step -------- */

/*
 * clip_grad_norm_(params, max_norm) followed by torch.optim.Adam / AdamW's step
 * (train.py:543-552, :119-136), fp32 tensors of any length, one launch per pass:
 *   sc_adam_sumsq  sum of squares of the gradients of the clipped tensors into
 *                  part[sc_adam_parts(t, nt)] (fixed order, no atomics);
 *   sc_adam_step   coef = max_norm / (sqrt(sum part) + 1e-6) clamped to <= 1 (part = NULL: 1;
 *                  NaN propagates like torch.clamp), then per element: g *= coef; AdamW
 *                  (decoupled = 1) p *= 1 - lr wd, Adam g += wd p; m = lerp(m, g, 1 - beta1);
 *                  v = v beta2 + (1 - beta2) g g; p -= step_size m / (sqrt(v) / bc2_sqrt + eps),
 *                  step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step).
 *                  norm_out (optional, one float): the total norm clip_grad_norm_ returns.
 * The gradients are only read (p.grad keeps its unclipped values; the step loop discards them).
 * Up to 24 tensors go into one launch's argument table; longer lists take several launches.
 */
typedef struct {
  float* p;        /* parameter */
  const float* g;  /* gradient */
  float* m;        /* exp_avg */
  float* v;        /* exp_avg_sq */
  int64_t n;       /* elements */
} sc_adam_tensor;
int64_t sc_adam_parts(const sc_adam_tensor* t, int nt);
int sc_adam_sumsq(const sc_adam_tensor* t, int nt, float* part, void* stream);
int sc_adam_step(const sc_adam_tensor* t, int nt, const float* part, int64_t nparts,
                 double max_norm, double lr, double beta1, double beta2, double eps,
                 double weight_decay, int decoupled, double step_size, double bc2_sqrt,
                 float* norm_out, void* stream);

/*
 * Per-step bf16 images of the fp32 projection weights, one launch for up to SC_MAX_IMAGE_JOBS
 * weights: the autocast casts of LinearSafe (lucyrnn_triton.py:20-25 under train.py's autocast)
 * plus the layouts the GEMMs want.  Per job: dst bf16 [rows][cols_pad] = src rows (stride ld_src) with
 * zero columns cols..cols_pad-1, rows in step-blocked order (block, gate, unit) when block_d = D
 * > 0 (rows = 7 D, D % 64 == 0; dst row (b, g, u) = src row g D + 64 b + u); dst_t (optional)
 * bf16 [cols][rows] = dst's first cols columns transposed.  Round to nearest even.
 * col_scale [cols] / row_shift [rows] (either may be NULL): the imaged value is
 * col_scale[c] * src - row_shift[source row], computed unfused (the folded LayerNorm's W'',
 * sc_ln_fold_prep).
 */
typedef struct {
  const float* src;
  void* dst;
  void* dst_t;
  int64_t rows, cols, cols_pad, ld_src, block_d;
  const float* col_scale;
  const float* row_shift;
} sc_image_job;
int sc_weight_images(const sc_image_job* jobs, int njobs, void* stream);

/* ---------------------------------------------------------------- xLSTM block glue ------ */

/*
 * The xLSTM-large block's elementwise / row-norm glue (C4 encoder, model.py:214-229; structure
 * as transformers' modeling_xlstm.py:870-1205), one HBM pass each, bf16 tensors, fp32 math,
 * bf16 roundings where the torch module rounds.  Weight gradients come back as fp32 partial rows
 * [sc_xlstm_part_rows(rows)][D] for a fixed-order sum (sc_colsum).
 *   RMSNorm (force_float32_reductions): y = bf16(bf16(x rsqrt(mean x^2 + eps)) w), x/y [rows][D]
 *     contiguous, D in {256, 512, 768, 1024}; rstd fp32 [rows] saved for the backward.
 *   gated head LayerNorm: out[m][n DH + e] = bf16(bf16(sigmoid(o[m][n DH + e])) *
 *     bf16(LN(h[b][n][t][:])[e]) * w[n DH + e]), m = b T + t: MultiHeadLayerNorm of the mLSTM
 *     cell output in the cell's [B][NH][T][DH] layout times sigmoid of the output gate (a
 *     row-strided view, ldo); NH <= 4, DH in {64, 128, 192, 256}; mean/rstd fp32 [M][NH].
 *     Backward: dh in the cell layout, d o into a [M][lddo] view (the fused projection's
 *     gradient).
 *   SwiGLU: y = bf16(bf16(silu(g)) u) for a = [g | u] rows of 2F; the backward writes [dg | du].
 */
int sc_xlstm_part_rows(int64_t rows);
int sc_rmsnorm_fwd(const void* x, const float* w, void* y, float* rstd, int64_t rows, int D,
                   float eps, void* stream);
int sc_rmsnorm_bwd(const void* x, const void* dy, const float* w, const float* rstd, void* dx,
                   float* part, int64_t rows, int D, void* stream);
/* The block's residual add folded into the next RMSNorm (xLSTM block: x + y then norm_ffn, and
 * the previous block's x + ffn(..) then norm_mlstm; modeling_xlstm.py block forward):
 * s = bf16(x + r) (written) and y = RMSNorm(s) as sc_rmsnorm_fwd.  The backward takes s as its x
 * and adds the residual branch's gradient: dx = bf16(bf16(dRMSNorm) + dres), the sum autograd
 * forms for the two bf16 gradients of s. */
int sc_rmsnorm_add_fwd(const void* x, const void* r, void* s, const float* w, void* y, float* rstd,
                       int64_t rows, int D, float eps, void* stream);
int sc_rmsnorm_add_bwd(const void* s, const void* dy, const void* dres, const float* w,
                       const float* rstd, void* dx, float* part, int64_t rows, int D, void* stream);
int sc_mhln_gate_fwd(const void* h, const void* o, int64_t ldo, const float* w, void* out,
                     float* mean, float* rstd, int B, int T, int NH, int DH, float eps,
                     void* stream);
int sc_mhln_gate_bwd(const void* h, const void* o, int64_t ldo, const float* w, const float* mean,
                     const float* rstd, const void* dy, int64_t ldy, void* dh, void* dgo,
                     int64_t lddo, float* part, int B, int T, int NH, int DH, void* stream);
/* The same with h in f16 (an f16 mLSTM cell's output), each element rounded to bf16 on load as
 * h.to(bfloat16) would; dh is written in bf16. */
int sc_mhln_gate_fwd_h16(const void* h, const void* o, int64_t ldo, const float* w, void* out,
                         float* mean, float* rstd, int B, int T, int NH, int DH, float eps,
                         void* stream);
int sc_mhln_gate_bwd_h16(const void* h, const void* o, int64_t ldo, const float* w,
                         const float* mean, const float* rstd, const void* dy, int64_t ldy,
                         void* dh, void* dgo, int64_t lddo, float* part, int B, int T, int NH,
                         int DH, void* stream);
int sc_swiglu_fwd(const void* a, void* y, int64_t rows, int F, void* stream);
int sc_swiglu_bwd(const void* a, const void* dy, void* da, int64_t rows, int F, void* stream);

/* ---------------------------------------------------------------- feature frontend ------ */

/* Frames of a row of n_samples (center=False): 1 + (n - 400) / 160, or 0 below 400 samples. */
int64_t sc_fbank_frames(int64_t n_samples);
size_t sc_fbank_workspace_bytes(void);

/*
 * make_frontend(kind)(audio).transpose(1, 2) (model.py:250-279, train.py:473-475):
 * audio fp32 [B][audio_stride] (n_samples used per row) -> out fp32 [B][frames][80].
 * n_fft = win = 400 (periodic Hann), hop 160, center=False, power 2, 80 HTK mel bands over
 * [0, sample_rate/2], no filter normalisation.
 *   kind SC_FBANK_MFCC: log(mel + 1e-6), orthonormal DCT-II, 80 coefficients;
 *   kind SC_FBANK_MEL:  10 log10(max(mel, 1e-10)), then max(x, max over the whole call - 80)
 *                  (AmplitudeToDB(top_db=80) on a (B, 80, frames) spectrogram).
 * workspace: sc_fbank_workspace_bytes() device bytes (SC_FBANK_MEL only).
 */
int sc_fbank(const float* audio, int B, int64_t n_samples, int64_t audio_stride, int kind,
             float sample_rate, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- mLSTM ----------------- */

/* 1 if the mLSTM kernels are compiled for this compute dtype (bf16/f16) and head dims. */
int sc_mlstm_supported(int dtype, int DQ, int DV);

/* Elements of the forward's chunk-start state image states_C: BH * (T/64) * DQ * DV. */
int64_t sc_mlstm_chunk_state_numel(int BH, int T, int DQ, int DV);

/*
 * mLSTM cell forward over BH = batch x heads independent sequences, chunkwise (chunk 64,
 * T % 64 == 0).  q, k [BH][T][DQ], v [BH][T][DV] of dtype (bf16 or f16; MFMA with fp32
 * accumulation); igate, fgate fp32 [BH][T] pre-activations; optional initial state c0 fp32
 * [BH][DQ][DV], n0 [BH][DQ], m0 [BH] (NULL = zeros).  Outputs: h [BH][T][DV] (dtype);
 * states_C = the stabilised state C~_k at every chunk START k < T/64, in dtype and TRANSPOSED
 * ([BH][T/64][DV][DQ]: exactly the operand image the forward's q C~_k MFMA consumes; the
 * backward's dq reads it);
 * states_n / states_m fp32 at every chunk boundary ([BH][T/64+1][DQ], [BH][T/64+1]; index T/64
 * is the final state); c_last fp32 [BH][DQ][DV] the final state C~ (the carried segment state);
 * m_rows, den_rows fp32 [BH][T] (the row stabiliser and normaliser, consumed by the backward).
 * One launch: each (sequence, 64-column block of C~) walks its chunks with the state in MFMA
 * accumulators (the fp32 chunk states are never written to HBM).  h_t = q~_t C_t / (max(|q~_t n_t|,
 * e^{-m_t}) + eps) with q~ = q DQ^-1/2.
 * layout (optional, 7 int64): {NH, qb, qh, qt, vb, vh, vt} element strides of q / k (and dq /
 * dk) and v (dv) with sequence bh = b NH + h at step t at (bh / NH) qb + (bh % NH) qh + t qt:
 * the xLSTM layer reads them in place from its fused projection output [B][T][N] (qh = DQ,
 * qt = N) and the backward writes the gradients into the projection's gradient the same way.
 * NULL = contiguous [BH][T][D].  Strides multiples of 8 elements, bases 16-byte aligned.
 * T == 0: c_last, states_n[:, 0], states_m[:, 0] = the initial state (zeros without one).
 */
int sc_mlstm_fwd(const void* q, const void* k, const void* v, int dtype, const float* igate,
                 const float* fgate, const float* c0, const float* n0, const float* m0, int BH,
                 int T, int DQ, int DV, float eps, void* h, void* states_C, float* states_n,
                 float* states_m, float* c_last, float* m_rows, float* den_rows,
                 const int64_t* layout, void* stream);

/*
 * Backward of sc_mlstm_fwd given dh (dtype, [BH][T][DV]) and optional gradients of the final
 * state (dcT fp32 [BH][DQ][DV], dnT [BH][DQ]; NULL = zero).  Outputs dq, dk, dv (dtype),
 * dstates_C / dstates_n fp32 [BH][DQ][DV] / [BH][DQ] = the gradient w.r.t. the INITIAL state
 * (c0, n0; the per-chunk state gradients never leave the chip: one 8-wave workgroup per
 * sequence walks the chunks in reverse with dC~ in MFMA accumulators), and the
 * per-step gate terms qdq = q_t.dq_t, kdk = k_t.dk_t (fp32 [BH][T]): d igate = kdk,
 * d fgate_t = sigmoid(-f_t) sum_{r>=t} (qdq_r - kdk_r).  The stabiliser is not differentiated.
 * With dcT / dnT the final state depends on the last forget gate with no query partner: the
 * caller adds <dcT, C~_T> + <dnT, n~_T> per sequence to qdq[T-1] before sc_mlstm_gate_bwd
 * (ops._mlstm_state_grad_term).  T == 0: dstates_C / dstates_n = dcT / dnT (zeros if NULL).
 * layout: as sc_mlstm_fwd's; dq / dk / dv are written with the same strides as q / k / v.
 */
int sc_mlstm_bwd(const void* q, const void* k, const void* v, int dtype, const float* igate,
                 const float* fgate, const void* h, const void* dh, const float* dcT,
                 const float* dnT, const void* states_C, const float* states_n,
                 const float* states_m, const float* m_rows, const float* den_rows, int BH, int T,
                 int DQ, int DV, float eps, float* dstates_C, float* dstates_n, void* dq,
                 void* dk, void* dv, float* qdq, float* kdk, const int64_t* layout,
                 void* stream);

/*
 * sc_mlstm_fwd / sc_mlstm_bwd with the operands in another dtype than the cell computes in:
 * io_dtype is the dtype of q, k, v (and dh, dq, dk, dv); dtype the cell's MFMA dtype and that of h
 * and the chunk-state image.  Supported pairs: (bf16, bf16), (f16, f16), and (f16, bf16) -- the
 * reference's float16 cell (autocast_kernel_dtype, model.py:227) reading a bf16-autocast
 * model's projection in place, each operand rounded to f16 on load as .to(float16) would, and
 * the gradients rounded through f16 to bf16 as the split path's casts are.
 */
int sc_mlstm_fwd_io(const void* q, const void* k, const void* v, int dtype, int io_dtype,
                    const float* igate, const float* fgate, const float* c0, const float* n0,
                    const float* m0, int BH, int T, int DQ, int DV, float eps, void* h,
                    void* states_C, float* states_n, float* states_m, float* c_last,
                    float* m_rows, float* den_rows, const int64_t* layout, void* stream);
int sc_mlstm_bwd_io(const void* q, const void* k, const void* v, int dtype, int io_dtype,
                    const float* igate, const float* fgate, const void* h, const void* dh,
                    const float* dcT, const float* dnT, const void* states_C,
                    const float* states_n, const float* states_m, const float* m_rows,
                    const float* den_rows, int BH, int T, int DQ, int DV, float eps,
                    float* dstates_C, float* dstates_n, void* dq, void* dk, void* dv,
                    float* qdq, float* kdk, const int64_t* layout, void* stream);

/*
 * Gate gradients of the mLSTM cell from sc_mlstm_bwd's qdq / kdk (fp32 [BH][T], T % 64 == 0)
 * and the forget-gate pre-activations fgate (fp32 [BH][T], after any soft cap):
 *   d igate = kdk,  d fgate_t = sigmoid(-fgate_t) sum_{r >= t} (qdq_r - kdk_r).
 * Either dfgate != NULL (fp32 [BH][T]; d igate is kdk itself), or da != NULL: both gradients
 * through the xLSTM gate soft cap (cap > 0; cap <= 0 = none): g (1 - tanh(x / cap)^2) in fp32,
 * rounded once to bf16, written into the projection gradient da at [b][t][io + h] and
 * [b][t][fo + h] (row stride ld elements), a holding the raw bf16 pre-activations at the same
 * positions; sequence bh = b NH + h.
 */
int sc_mlstm_gate_bwd(const float* qdq, const float* kdk, const float* fgate, int BH, int T,
                      float* dfgate, const void* a, void* da, int NH, int64_t ld, int io, int fo,
                      float cap, void* stream);

/* 1 if the mLSTM step kernel is compiled for this operand dtype (fp32/bf16) and head dims. */
int sc_mlstm_step_supported(int io_dtype, int DQ, int DV);

/*
 * The recurrent mLSTM step (streaming / any-length inference): advances BH = batch x heads
 * sequences by K steps from the carried state, in fp32 arithmetic:
 *   m_t = max(logsig(f_t) + m_{t-1}, i_t)
 *   C_t = e^{logsig(f_t)+m_{t-1}-m_t} C_{t-1} + e^{i_t-m_t} k_t v_t^T      (n_t alike)
 *   h_t = (q~_t C_t) / (max(|q~_t . n_t|, e^{-m_t}) + eps),  q~ = q DQ^-1/2.
 * State C fp32 [BH][DQ][DV], n [BH][DQ], m [BH]: sc_mlstm_fwd's c_last / states_n[:, T/64] /
 * states_m[:, T/64] convention (no conversion between the two kernels), updated IN PLACE; it is
 * read once and written once per call whatever K is (C stays in registers over the K steps).
 * q, k [BH][K][DQ], v [BH][K][DV] in io_dtype (fp32 or bf16); h [BH][K][DV] in io_dtype.
 * layout: as sc_mlstm_fwd's (7 int64 {NH, qb, qh, qt, vb, vh, vt}, layout[0] == NH; NULL =
 * contiguous), the same stride and alignment rules.
 * Gates: gate_layout == NULL: igate, fgate fp32 [BH][K] pre-activations.  Else 3 int64
 * {gb, gh, gt}: igate / fgate point into the projection (io_dtype) and sequence bh = b NH + h
 * reads step t at b gb + h gh + t gt.  Either way the soft cap cap tanh(x / cap) is applied in
 * fp32 when cap > 0 (cap <= 0: none).
 * live: optional fp32 [BH / NH][K]; a step with live == 0 leaves C, n, m bitwise untouched and
 * writes a zero output row.  NULL = all live.
 * A step's arithmetic does not depend on K or its position in the call: K steps in one call
 * equal K calls of one step bitwise.  K == 0 or BH == 0: no-op.
 */
int sc_mlstm_step(const void* q, const void* k, const void* v, int io_dtype, const void* igate,
                  const void* fgate, const int64_t* gate_layout, float cap, const float* live,
                  float* C, float* n, float* m, int BH, int K, int NH, int DQ, int DV, float eps,
                  void* h, const int64_t* layout, void* stream);

/* ---------------------------------------------------------------- RNN-T ----------------- */

/* Workspace bytes for sc_rnnt_fwd / sc_rnnt_bwd (gathered log-probs, alpha, beta, offsets). */
size_t sc_rnnt_workspace_bytes(int B, int T, int max_labels);

/*
 * RNN-T negative log-likelihood over the transducer lattice (gather semantics: the blank and
 * next-label log-probs of every node (t, u), t < frames_lengths[b], u <= labels_lengths[b]).
 * x: node (b,t,u)'s V-row (v-stride 1) is at
 *   dense   (row_offsets == NULL): b*stride_b + t*stride_t + u*stride_u   ([B,T,max_labels+1,V])
 *   compact (row_offsets != NULL): (row_offsets[b] + t*(labels_lengths[b]+1) + u) * stride_u,
 *           the packed (sum_b T_b (U_b+1), V) layout of RNNTCompactPredictorJoiner (model.py:147-200)
 *   is_logits = 1: x are joiner logits, log_softmax fused; 0: x are log-probs.
 * labels: int64 [B, max_labels] (row stride label_stride); lengths: int64 [B] device arrays.
 * nll: fp32 [B].  max_labels <= 1007 (16 waves of 63 label positions).
 * -inf log-probs or logits (a masked vocabulary) are allowed.  A sequence without an alignment
 * (frames_lengths[b] == 0, or every path blocked by -inf entries: its final blank, or one label
 * in every frame) gets nll = +inf and an all-zero gradient; the other sequences are unaffected.
 */
int sc_rnnt_fwd(const void* x, int x_dtype, int is_logits, int B, int T, int max_labels, int V,
                int64_t stride_b, int64_t stride_t, int64_t stride_u, const int64_t* row_offsets,
                const int64_t* labels, int64_t label_stride, const int64_t* frames_lengths,
                const int64_t* labels_lengths, int blank, float* nll, void* workspace,
                size_t workspace_bytes, void* stream);

/*
 * Gradient of sum_b scale[b] * nll[b] w.r.t. x (scale of either sign; 0 and sequences without an
 * alignment give exact zeros), written to grad (grad_dtype = fp32 or x_dtype, same layout as x;
 * dense rows outside the lattice are zeroed).  Logits: the softmax-corrected
 * row; log-probs: non-zero only at the blank and label entries (warp_rnnt gather=True).
 */
int sc_rnnt_bwd(const void* x, int x_dtype, int is_logits, int B, int T, int max_labels, int V,
                int64_t stride_b, int64_t stride_t, int64_t stride_u, const int64_t* row_offsets,
                const int64_t* labels, int64_t label_stride, const int64_t* frames_lengths,
                const int64_t* labels_lengths, int blank, const float* scale, void* grad,
                int grad_dtype, const void* workspace, size_t workspace_bytes, void* stream);

/*
 * Fused joiner + RNN-T loss (C5): RNNTPredictorJoiner.forward (model.py:129-145) -> fp32
 * log_softmax (model.py:93) -> the gathered lattice, without the (B, T, U+1, V) logits.
 *   enc   fp32 [B][T][J]       enc_proj(enc_out), contiguous
 *   pred  fp32 [B][U1][J]      pred_proj(embedding(blank-prefixed labels)), U1 = max_labels + 1
 *   W     bf16 [V][J]          joiner.weight (MFMA operand); bias fp32 [V] = joiner.bias
 * J must be 64 (train.py:639's --rnnt-joiner-dim default), V a multiple of 32, <= 1024.
 * Forward: nll fp32 [B] as sc_rnnt_fwd (same workspace, sc_rnnt_workspace_bytes; +inf and zero
 * gradients for a sequence without an alignment, as there).
 * Backward (after the forward, same workspace) of sum_b scale[b] nll[b] (scale of either sign),
 * one pass over the logits (the workgroups split the vocabulary; t_blocks and u_splits count
 * those splits too):
 *   d_enc   fp32 [u_splits][B][T][J]   partials (sum them: d enc)
 *   d_pred  fp32 [B][t_blocks][U1][J]  partials (sum over t_blocks: d pred); zero-filled by
 *                                      the caller (columns outside the lattice are not written)
 *   dW      fp32 [slices][V][J], db fp32 [slices][V]: partials of sum_n dlogits_n z_n^T and
 *           sum_n dlogits_n, dlogits_n = a_n softmax_n - w_blank,n e_blank - w_label,n e_y,
 *           a_n = scale (occ_blank + occ_label) (sum them in a fixed order: d W, d bias)
 * t_blocks / u_splits / slices: sc_rnnt_joint_geometry.
 */
int sc_rnnt_joint_geometry(int B, int T, int max_labels, int V, int* t_blocks, int* u_splits,
                           int* slices);
int sc_rnnt_joint_fwd(const float* enc, const float* pred, const void* W, const float* bias, int B,
                      int T, int max_labels, int V, int J, const int64_t* labels,
                      int64_t label_stride, const int64_t* frames_lengths,
                      const int64_t* labels_lengths, int blank, float* nll, void* workspace,
                      size_t workspace_bytes, void* stream);
int sc_rnnt_joint_bwd(const float* enc, const float* pred, const void* W, const float* bias, int B,
                      int T, int max_labels, int V, int J, const int64_t* labels,
                      int64_t label_stride, const int64_t* frames_lengths,
                      const int64_t* labels_lengths, int blank, const float* scale, float* d_enc,
                      float* d_pred, float* dW, float* db, const void* workspace,
                      size_t workspace_bytes, void* stream);

/*
 * Greedy transducer decoding for the stateless predictor of RNNTPredictorJoiner
 * (model.py:112-145: pred_proj(embedding(prev_token)) depends only on the last emitted token).
 * The reference has no transducer decoder; this is what its CTC-only decoder.py lacks.
 *   enc_p    [B][T][J]  joiner.enc_proj(enc_out); element strides stride_b, stride_t, inner 1
 *   pred_tab [V][J]     joiner.pred_proj(joiner.embedding.weight): the predictor output for every
 *                       possible previous token, contiguous
 *   W        [V][J]     joiner.joiner.weight, contiguous;  bias fp32 [V] = joiner.joiner.bias
 *   enc_p, pred_tab and W share `dtype` (fp32 / bf16 / f16).  All are widened to fp32 on load;
 *   z and the dot products stay fp32 (tanh to ~1e-6 absolute).  This differs on purpose from
 *   sc_rnnt_joint_fwd, which rounds W and z to bf16 for its MFMAs: decoding follows the
 *   reference's fp32 arithmetic on the master weights.
 *   lengths  int64 [B] or null: frames t >= lengths[b] are dead
 *   mask     fp32 or null: frame (b, t) is dead where mask[b*mask_b + t*mask_t] == 0 (the meaning
 *            of sc_ctc_greedy_frames' mask)
 *   prev     int32 [B] or null, in/out: the last emitted token of each stream, read at entry and
 *            written at exit, so a stream decoded in chunks equals the stream decoded whole.  Null
 *            (or a value outside [0, V)) starts the stream at `blank`, the prefix compute_loss
 *            feeds the predictor (model.py:77-83).
 * Per stream b, u = prev[b], for each live frame t in order, at most max_symbols (1..64) times:
 *   z = tanh(enc_p[b][t] + pred_tab[u]);  logit[v] = W[v] . z + bias[v];  k = argmax_v logit
 *   (first maximal index, a NaN counting as maximal, as sc_ctc_greedy_decode);  k == blank: next
 *   frame;  otherwise emit k at frame t, u = k, repeat.
 *   tokens int32 [B][cap]: the emitted tokens in order;  frames int32 [B][cap] or null: the frame
 *   index of each emission;  counts int32 [B]: the number of emissions, even beyond cap.  Nothing
 *   is written at or beyond index cap; entries past counts[b] are left untouched.
 * One persistent workgroup per stream.  J == 64 and V <= 1024 (W 16-byte aligned) keeps a row of W
 * per lane in registers; any other V and J <= 256 reads W from memory at every evaluation.
 * B == 0 and T == 0 launch nothing (T == 0 zeroes counts).  No host sync, no allocation.
 */
int sc_rnnt_greedy_decode(const void* enc_p, const void* pred_tab, const void* W, int dtype,
                          const float* bias, int B, int T, int V, int J, int64_t stride_b,
                          int64_t stride_t, const int64_t* lengths, const float* mask,
                          int64_t mask_b, int64_t mask_t, int blank, int max_symbols,
                          int32_t* prev, int32_t* tokens, int32_t* frames, int cap,
                          int32_t* counts, void* stream);

/*
 * CTC prefix beam search, offline and chunked (csrc/ctc_beam.hip).  The reference's decoder.py is
 * CTC greedy only (its README lists the beam search decoder as planned).  Greedy takes the best
 * frame-wise path; prefix beam search sums every alignment of a hypothesis and returns an n-best
 * list with scores.  All arithmetic is fp32; x (fp32 / bf16 / f16) is widened on load.
 *   lae(a, b) = max(a, b) + log1p(exp(-|a - b|)),  lae(-inf, b) = b
 * Per stream the state is an ordered beam of at most `beam` hypotheses: a token prefix, pb (log-
 * probability of the prefix's alignments that end in blank) and pnb (those that end in a
 * non-blank).  A reset stream holds the empty prefix with pb = 0, pnb = -inf.  For each live
 * frame t in order (live as in sc_rnnt_greedy_decode: t < lengths[b] where lengths is given, and
 * mask[b*mask_b + t*mask_t] != 0 where mask is given):
 *   1. lp[v] = x[v] - logsumexp_v x (is_logits = 1) or x[v] (is_logits = 0)
 *   2. the frame's tokens: the top_k non-blank v with the largest lp, ties to the lower index
 *   3. stay candidates, one per beam entry in beam order:  tot = lae(pb, pnb);
 *      pb' = tot + lp[blank];  pnb' = pnb + lp[last] if the prefix is non-empty and its last token
 *      is one of the frame's tokens, else -inf
 *   4. extension candidates, ordered by (beam rank, top_k rank), prefix l and token c:
 *      pnb' = (c == last(l) ? pb : tot) + lp[c], pb' = -inf.  If l + c is already a beam entry the
 *      extension is no candidate of its own: that entry's stay candidate gets
 *      pnb' = lae(its repeat term, the extension's pnb').  Identity is decided by (64-bit rolling
 *      hash of the tokens, length), not by comparing the token sequences.
 *   5. candidates whose total lae(pb', pnb') is -inf are dropped; the `beam` largest totals (ties
 *      to the earlier candidate in the order above), sorted by total descending, are the new beam.
 * A NaN anywhere in a row makes that stream's result unspecified; the call still completes with
 * every index in range (a NaN ranks last among the lp and a NaN total is dropped).
 * Limits: 1 <= beam <= 32, 1 <= top_k <= min(32, V - 1), 1 <= nbest <= beam, V >= 2,
 * 0 <= blank < V.
 *
 * The state is opaque device memory of sc_ctc_beam_state_bytes(B, beam, max_frames) bytes, 8-byte
 * aligned, per stream: the beam (pb, pnb, trie node, hash, length, last token), the number of live
 * frames consumed, a status word, and the token history as a parent-pointer trie of
 * 1 + max_frames * beam (parent, token) nodes -- node 0 is the empty prefix, the extension kept at
 * rank r of live frame f is node 1 + f * beam + r, so nothing is allocated or counted atomically.
 *   sc_ctc_beam_reset   every stream (streams null) or those with streams[b] != 0 back to the
 *                       fresh state.  Must run once before the first sc_ctc_beam_frames.
 *   sc_ctc_beam_frames  consumes x [B][T][V] (element strides stride_b, stride_t, inner 1): a
 *                       frame-parallel pre-pass (one wave per live row, the row read once: lp[blank]
 *                       and the top_k (index, lp) pairs go to `workspace`, at least
 *                       sc_ctc_beam_workspace_bytes(B, T, top_k) bytes, 4-byte aligned), then one
 *                       workgroup per stream walks the frames.  May be called any number of times
 *                       on one state with the same beam: a stream fed in chunks ends in the state
 *                       of the stream fed whole.  The frame counter lives in the state and no
 *                       argument changes from chunk to chunk, so a captured graph of one chunk call
 *                       can be replayed.  Once a stream has consumed max_frames live frames, further
 *                       live frames are ignored and status bit 0 is set.
 *   sc_ctc_beam_result  reads the state (does not change it): for n < nbest, tokens[b][n][0..cap)
 *                       int32 <- the first min(lens, cap) tokens of beam entry n, lens[b][n] <- its
 *                       full token count (even beyond cap), scores[b][n] <- lae(pb, pnb).  Nothing is
 *                       written at or beyond cap; entries past lens are left untouched.  For n at or
 *                       past the number of hypotheses alive, lens = -1 and scores = -inf.
 *                       status int32 [B] or null <- the status word (bit 0: max_frames reached;
 *                       bit 1: the state was not made for this beam).
 * B == 0 (and T == 0 for sc_ctc_beam_frames) launch nothing and return 0.  The size functions
 * return 0 for arguments outside the limits.  No host sync, no allocation.
 */
size_t sc_ctc_beam_state_bytes(int B, int beam, int max_frames);
size_t sc_ctc_beam_workspace_bytes(int B, int T, int top_k);
int sc_ctc_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_frames,
                      const float* streams, void* stream);
int sc_ctc_beam_frames(const void* x, int dtype, int is_logits, int B, int T, int V,
                       int64_t stride_b, int64_t stride_t, const int64_t* lengths,
                       const float* mask, int64_t mask_b, int64_t mask_t, int blank, int beam,
                       int top_k, void* state, size_t state_bytes, void* workspace,
                       size_t workspace_bytes, void* stream);
int sc_ctc_beam_result(const void* state, size_t state_bytes, int B, int beam, int nbest,
                       int32_t* tokens, int cap, int32_t* lens, float* scores, int32_t* status,
                       void* stream);

/*
 * CTC forced alignment (csrc/ctc_align.hip): the best (Viterbi) alignment of a transcript to the
 * frames, where each token lies, and how well it fits -- per frame, per token and in total.  The
 * reference lists "on-the-fly hallucination detection & filtering" of its subtitle-cut segments as
 * planned; a hallucinated or shifted transcript aligns badly.  sc_ctc_fwd gives one number per
 * sequence; the transducer decoders return the frame of every token; this is the CTC counterpart.
 *
 * Inputs are those of sc_ctc_fwd: x [B][T][V] (fp32 / bf16 / f16, widened exactly on load; element
 * strides stride_b, stride_t, inner 1), is_logits, targets int64 [B][max_target_len] (row stride
 * target_stride), in_lens / tgt_lens int64 [B] (clamped into [0, T] / [0, max_target_len]), blank.
 * max_target_len <= 1007.  A label outside [0, V) reads the nearest column, and a label equal to
 * blank is never skipped into, both as in sc_ctc_fwd.
 *
 * Per sequence (T_b = in_lens[b], U = tgt_lens[b]) the blank-extended states are s = 0 .. 2U,
 * ext[s] = blank for even s and targets[(s - 1) / 2] for odd s.
 *   lp[t][v] = x[v] - logsumexp_v x (is_logits = 1) or x[v] (is_logits = 0); natural log, fp32
 *   v[0][0] = lp[0][blank], v[0][1] = lp[0][ext[1]], every other state -inf
 *   v[t][s] = lp[t][ext[s]] + max(v[t-1][s], v[t-1][s-1], v[t-1][s-2]), the s-2 term only for odd
 *             s >= 3 with ext[s] != ext[s-2]; ties go to the smaller move (stay, step, skip)
 *   the path ends in state 2U or 2U-1, whichever has the larger v[T_b-1] (a tie goes to 2U; U = 0
 *   ends in state 0), and is followed back through the recorded moves.
 * Arithmetic: each frame's emissions are shifted by c_t, the largest lp of that frame among the
 * sequence's states (every path takes one emission per frame, so the path does not depend on it),
 * v is re-centred on its maximum every 16 frames, and the sum of shifts and maxima is carried in
 * fp64: an unshifted fp32 lattice at T = 1500 holds values near 1e4, whose rounding decides close
 * moves.  This is what sc_ctc_fwd does for the loss.  An emission below -1e30 (or NaN) counts as
 * impossible.  logsumexp is summed in pieces of 8 consecutive elements, piece c by lane c % 64,
 * whatever the element type and the row's alignment: a 16-bit tensor aligns bit for bit as the
 * fp32 tensor of the same values.  -inf logits (masked tokens) add exp = 0 to it.
 *
 * Outputs:
 *   states   int32 [B][T]    the path's state at each frame t < T_b; -1 at t >= T_b
 *   frame_lp fp32 [B][T]     lp[t][ext[states[t]]] (unshifted); 0 at t >= T_b
 *   spans    int32 [B][max_target_len][2]  first frame and one past the last frame of the run of
 *                            state 2u + 1; -1, -1 for u >= U
 *   token_lp fp32 [B][max_target_len]  mean of frame_lp over the span, summed in frame order in
 *                            fp32; 0 for u >= U
 *   score    fp32 [B]        the path's total log-probability: fp64 (shifts + maxima) + the final
 *                            value, rounded once
 * A sequence with no valid alignment (T_b < U + the number of adjacent equal labels, or T_b = 0 <
 * U) gets score -inf, states -1, spans -1 and zeros elsewhere; T_b = 0 with U = 0 gives score 0.
 * A NaN in a sequence's rows makes that sequence's result unspecified; the call still completes
 * with every index in range and the other sequences untouched.  B == 0 launches nothing.  Bad
 * arguments return SC_EINVAL with sc_last_error set.
 *
 * workspace: at least sc_ctc_align_workspace_bytes(B, T, max_target_len) bytes, 16-byte aligned
 * (the compact emission rows, the rows' normalisers and shifts, and 2 bits per state and frame of
 * recorded moves); the size function returns 0 for arguments outside the limits.  No host sync, no
 * allocation, no atomics: two runs are bitwise equal and the call captures into a HIP graph.
 */
size_t sc_ctc_align_workspace_bytes(int B, int T, int max_target_len);
int sc_ctc_align(const void* x, int x_dtype, int is_logits, int B, int T, int V,
                 int64_t stride_b, int64_t stride_t,
                 const int64_t* targets, int64_t target_stride, int max_target_len,
                 const int64_t* in_lens, const int64_t* tgt_lens, int blank,
                 int32_t* states, float* frame_lp, int32_t* spans, float* token_lp, float* score,
                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * Transducer beam search for the stateless predictor, offline and chunked (csrc/rnnt_beam.hip).
 * sc_rnnt_greedy_decode follows one path and returns no score; this is the time-synchronous beam
 * search over the same joint, with an n-best list and scores.  Inputs are those of
 * sc_rnnt_greedy_decode: enc_p [B][T][J] (strides stride_b, stride_t, inner 1), pred_tab [V][J]
 * and W [V][J] contiguous, all of `dtype` (fp32 / bf16 / f16) and widened on load; bias fp32 [V];
 * lengths, mask and blank with the same meaning.  All arithmetic is fp32:
 *   z = tanh(enc_p[b][t] + pred_tab[u]) in the greedy kernel's form, u = the last token of the
 *   prefix (`blank` for the empty prefix);  logit = W z + bias;  lp = logit - logsumexp_v logit;
 *   lae as in the CTC beam search above.
 * Parameters: 1 <= beam <= 32;  1 <= top_k <= 32, clipped to V - 1;  1 <= max_symbols <= 8, the
 * most tokens one frame may emit;  1 <= nbest <= beam;  V >= 1;  1 <= J <= 256;  0 <= blank < V.
 * Per stream the state is an ordered beam of at most `beam` entries (prefix, score); a reset stream
 * holds [(empty, 0)].  For each live frame in order:
 *   A = [] (ordered, capacity beam * (max_symbols + 1));  C = the beam
 *   for r = 0 .. max_symbols:
 *     for each (p, s) of C in order:  s' = s + lp_p[blank];  if p is already in A, that entry's
 *       score becomes lae(entry, s'), else (p, s') is appended to A
 *     if r == max_symbols: stop
 *     D = for each (p, s) of C in order, for each of its top_k non-blank tokens c (lp descending,
 *       ties to the lower index, NaN last), in that order: (p + c, s + lp_p[c]);  entries whose
 *       score is -inf or NaN are dropped
 *     C = the `beam` largest of D (ties to the earlier candidate), sorted descending;  empty: stop
 *   A entries whose score is -inf or NaN are dropped;  the beam = the `beam` largest of A (ties to
 *   the earlier insertion), sorted descending
 * Within one D no two candidates spell the same prefix, so merging happens only into A; identity
 * in A is (64-bit rolling hash of the tokens, length), with the CTC beam search's hash.  With
 * nothing pruned the score of a prefix is exactly log P(prefix | x) over every alignment with at
 * most max_symbols emissions per frame.  A NaN makes the affected stream's result unspecified
 * (possibly empty, lens -1); orders stay total, every index stays in range, the call completes.
 *
 * The state is opaque device memory of sc_rnnt_beam_state_bytes(B, beam, max_symbols, max_frames)
 * bytes, 8-byte aligned, per stream: the beam (score, trie node, hash, length, last token), the
 * number of live frames consumed, a status word, and the token history as a parent-pointer trie of
 * 1 + max_frames * max_symbols * beam (parent, token) nodes -- node 0 is the empty prefix, the
 * candidate kept at rank k of round r of live frame f is node 1 + (f * max_symbols + r) * beam + k,
 * so nothing is allocated or counted atomically and a token's frame is read off its node.
 *   sc_rnnt_beam_reset   every stream (streams null) or those with streams[b] != 0 back to the
 *                        fresh state.  Must run once before the first sc_rnnt_beam_frames.
 *   sc_rnnt_beam_frames  one persistent workgroup per stream consumes the call's T frames.
 *                        `workspace`: at least sc_rnnt_beam_workspace_bytes(B, V) bytes, 4-byte
 *                        aligned (the logit image of the path that reads W from memory).  J == 64
 *                        and V <= 1024 (W 16-byte aligned) keeps a row of W per lane in registers;
 *                        any other V and J <= 256 reads W from memory.  beam and max_symbols must be
 *                        the state's.  May be called any number of times on one state: a stream fed
 *                        in chunks ends in the state of the stream fed whole.  The frame counter
 *                        lives in the state and no argument changes from chunk to chunk, so a
 *                        captured graph of one chunk call can be replayed.  Once a stream has
 *                        consumed max_frames live frames, further live frames are ignored and
 *                        status bit 0 is set.
 *   sc_rnnt_beam_result  reads the state (does not change it): for n < nbest, tokens[b][n][0..cap)
 *                        int32 <- the first min(lens, cap) tokens of beam entry n, frames (or null)
 *                        likewise <- the ordinal, counted since reset, of the live frame at which
 *                        each token was emitted (a merged hypothesis keeps the history of the entry
 *                        first inserted into A), lens[b][n] <- the full token count (even beyond
 *                        cap), scores[b][n] <- the score.  Nothing is written at or beyond cap;
 *                        entries past lens are left untouched.  For n at or past the number of
 *                        hypotheses alive, lens = -1 and scores = -inf.  status int32 [B] or null <-
 *                        the status word (bit 0: max_frames reached; bit 1: the state was not made
 *                        for this beam and max_symbols).
 * B == 0 (and T == 0 for sc_rnnt_beam_frames) launch nothing and return 0.  The size functions
 * return 0 for arguments outside the limits.  No host sync, no allocation.
 */
size_t sc_rnnt_beam_state_bytes(int B, int beam, int max_symbols, int max_frames);
size_t sc_rnnt_beam_workspace_bytes(int B, int V);
int sc_rnnt_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_symbols,
                       int max_frames, const float* streams, void* stream);
int sc_rnnt_beam_frames(const void* enc_p, const void* pred_tab, const void* W, int dtype,
                        const float* bias, int B, int T, int V, int J, int64_t stride_b,
                        int64_t stride_t, const int64_t* lengths, const float* mask, int64_t mask_b,
                        int64_t mask_t, int blank, int beam, int top_k, int max_symbols, void* state,
                        size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);
int sc_rnnt_beam_result(const void* state, size_t state_bytes, int B, int beam, int max_symbols,
                        int nbest, int32_t* tokens, int32_t* frames, int cap, int32_t* lens,
                        float* scores, int32_t* status, void* stream);

/* ---- RWKV-4 WKV operator --------------------------------------------------------------------
 * Per batch row b and channel c, with W = -exp(time_decay[c]), u = time_first[c] and the state
 * S = (A, B) held as (num, den, max), A = num e^max, B = den e^max, for t = 0 .. T-1:
 *     y_t     = (A_t + e^{u+k_t} v_t) / (B_t + e^{u+k_t})
 *     S_{t+1} = e^W S_t + e^{k_t} (v_t, 1)
 * evaluated with running maxima (transformers' rwkv_linear_attention_cpu), so no exponential
 * overflows.  k, v, y (and dy, dk, dv) are contiguous [B,T,C] of one dtype, SC_F32 or SC_BF16;
 * time_decay, time_first, their gradients, the state and all arithmetic are fp32.
 *   forward   num_in / den_in / max_in fp32 [B,C], all three or all null: the incoming state (null:
 *             the empty state num = den = 0, max = -1e38, which may also be passed explicitly).
 *             num_out / den_out / max_out <- the state after T steps (T == 0: the incoming one).
 *             They may alias the incoming arrays.  ckpt: null, or fp32 of
 *             sc_wkv_ckpt_numel(B, T, C) elements <- the state at the start of every super-chunk of
 *             sc_wkv_chunk() steps, which is all the backward needs besides its inputs.
 *   backward  dy = dL/dy; the incoming state is a constant and the outgoing state carries no
 *             gradient.  dk, dv <- the input gradients, d_time_decay / d_time_first fp32 [C] <-
 *             the parameter gradients summed over rows and steps in a fixed order (no atomics:
 *             two runs are bitwise equal; B == 0 or T == 0 gives zeros).  ws: fp32 scratch of
 *             sc_wkv_bwd_ws_numel(B, T, C) elements.
 * Any B, T, C >= 0 (B <= 65535); B == 0 or C == 0 launch nothing in the forward.  The size
 * functions return 0 for negative arguments.  No host sync, no allocation.
 */
int sc_wkv_chunk(void);
int64_t sc_wkv_ckpt_numel(int B, int T, int C);
int64_t sc_wkv_bwd_ws_numel(int B, int T, int C);
int sc_wkv_fwd(const float* time_decay, const float* time_first, const void* k, const void* v,
               int dtype, const float* num_in, const float* den_in, const float* max_in, void* y,
               float* num_out, float* den_out, float* max_out, float* ckpt, int B, int T, int C,
               void* stream);
int sc_wkv_bwd(const float* time_decay, const float* time_first, const void* k, const void* v,
               const void* dy, int dtype, const float* ckpt, void* dk, void* dv,
               float* d_time_decay, float* d_time_first, float* ws, int B, int T, int C,
               void* stream);

/* ---- RWKV-4 streaming step (csrc/rwkv_step.hip) ---------------------------------------------
 * What a block of K frames of B concurrent streams needs besides its GEMMs.  Activations are
 * [K][B][width] with explicit frame and row strides in elements (unit inner stride), SC_F32 or
 * SC_BF16; the state and all arithmetic are fp32.  live: fp32 [K][B] contiguous, or null (every
 * frame live); a frame with live == 0 is HELD: it leaves the state bitwise untouched.  A frame's
 * arithmetic does not depend on K or on its position in the call: K frames in one call equal K
 * calls of one frame bitwise.  No host sync, no allocation: safe inside a hipGraph capture.
 *
 *   sc_wkv_step       the recurrence of sc_wkv_fwd, one step at a time in its order, for K steps:
 *                     (num, den, max) fp32 [B,C] are read once, advanced IN PLACE and written
 *                     once (never null: the empty state is num = den = 0, max = -1e38, passed
 *                     explicitly).  k, v [K][B][C] share stride_t / stride_b; r: null, or the
 *                     receptance pre-activation in the same layout, and then y <- sigmoid(r) y.
 *                     y [K][B][C] in the operand dtype with its own strides; a held step writes a
 *                     zero row.  Any C >= 1, B <= 65535; K, B or C == 0 launch nothing.
 *   sc_rwkv_step_mix  per stream, in frame order, on the residual row h (fp32 [K][B][H], IN PLACE):
 *                       h += add, or h += sigmoid(gate) * add   (add / gate [K][B][H] in io_dtype,
 *                                                                sharing add_stride_*; either null)
 *                       h = LayerNorm(h; pre_w, pre_b)          (pre_w / pre_b null: skipped)
 *                       a = LayerNorm(h; ln_w, ln_b)            (fp32 two-pass statistics, eps)
 *                       s = the a of the stream's last live frame before this one, x_prev[b] for
 *                           its first live frame
 *                       out_i = a * mix_i + s * (1 - mix_i),  i < nmix    (mix_i fp32 [H])
 *                       nmix == 0: out_0 = a
 *                       live: x_prev[b] = a
 *                     h is rewritten when an add or pre_ln is given.  out_i [K][B][H] in io_dtype
 *                     share out_stride_*.  x_prev fp32 [B,H] IN PLACE; a stream with no live
 *                     frame leaves its row bitwise untouched; null only with nmix == 0 (nothing
 *                     is carried then).  The output rows of held frames are finite and not
 *                     meaningful.  1 <= H <= 2048, nmix in [0, 3]; K or B == 0 launch nothing.
 *   sc_relu_sq        x <- max(x, 0)^2 in place over n contiguous elements (the feed-forward's
 *                     squared ReLU); n == 0 launches nothing.
 * All return SC_EINVAL with sc_last_error() naming the argument for a dtype other than fp32 /
 * bf16, a shape outside the limits, a null state or a required pointer that is null.
 */
int sc_wkv_step(const float* time_decay, const float* time_first, const void* k, const void* v,
                const void* r, int dtype, int64_t stride_t, int64_t stride_b, const float* live,
                float* num, float* den, float* max, void* y, int64_t y_stride_t,
                int64_t y_stride_b, int K, int B, int C, void* stream);
int sc_rwkv_step_mix(float* h, int64_t h_stride_t, int64_t h_stride_b, const void* add,
                     const void* gate, int64_t add_stride_t, int64_t add_stride_b, int io_dtype,
                     const float* pre_w, const float* pre_b, const float* ln_w, const float* ln_b,
                     float eps, float* x_prev, const float* live, int nmix, const float* mix0,
                     const float* mix1, const float* mix2, void* out0, void* out1, void* out2,
                     int64_t out_stride_t, int64_t out_stride_b, int K, int B, int H, void* stream);
int sc_relu_sq(void* x, int dtype, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STATECATCHER_H */
