/*
 * libscasr - C ABI of the MI355X (gfx950) streaming-ASR hot path.
 *
 * Drop-in boundary for speechcatcher's native decoder path.
 * The reference is pure Python/PyTorch and has no FFI of its own; each entry
 * point below replaces the torch-op call sites of one reference function and
 * cites it (paths relative to the reference repository root).  The host side
 * (speechcatcher_amd/engine.py, Python like the reference) binds these with
 * ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer unless marked HOST.
 *   - all functions are asynchronous launches on `stream` (a hipStream_t
 *     passed as void*); return 0 on success, a negative code on error and
 *     never throw.  sc_last_error() returns a thread-local message.
 *   - caller owns all memory; nothing is allocated or freed by the library.
 *   - "rows" tables are int32 ROW indices into a 2-D buffer (multiplied by the
 *     leading dimension inside the kernel); NULL means the identity mapping;
 *     -1 in a gather table reads a zero row.
 *   - all floating point is fp32 (IEEE, no fast-math); hypothesis scores are
 *     accumulated in fp64 like the reference's Python floats.
 */
#ifndef SCASR_H
#define SCASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_ARG (-1)
#define SC_ERR_LAUNCH (-2)
#define SC_ERR_CAPACITY (-3) /* sc_push, per stream: a capacity limit of the batch (frames, tokens, pcm, chunk length) */
#define SC_ERR_INPUT (-4)    /* sc_push, per stream: an input the reference itself raises on */

/* flags of sc_gemm */
#define SC_GEMM_RELU 1
#define SC_GEMM_RESIDUAL 2
#define SC_GEMM_LN_AT_CROWS 8 /* sc_gemm_ln: ln_out rows follow c_rows instead of 0..M-1 */
#define SC_GEMM_NAIVE 4 /* force the scalar reference kernel (debugging) */
#define SC_GEMM_SPLIT16 16 /* tiled kernels only: fp16 hi | lo split of both operands when the tiles are staged, three fp16
                              MFMAs per product sum, fp32 accumulation - fp32-grade results at a fraction of the f32
                              matrix-pipe time (see sc_ffn_ln_s); the small-M kernels ignore it */

/* beam_prune stop flags (one int32 per stream) */
#define SC_F_ANY_EOS 1
#define SC_F_BEST_EOS 2
#define SC_F_ALL_EOS 4
#define SC_F_REPEAT 8

/* ctrl row (int32[8]) per stream, uploaded by the host before every search op */
#define SC_C_ACTIVE 0 /* stream takes part in this launch */
#define SC_C_CUR 1    /* live ping-pong hypothesis buffer (0/1); outputs go to 1-cur */
#define SC_C_FINAL 2
#define SC_C_T 3    /* encoder frames visible to this decode block */
#define SC_C_L 4    /* tokens per live hypothesis, incl. sos */
#define SC_C_NHYP 5 /* live hypotheses (1 or W) */
#define SC_C_HAS 6  /* live hypotheses carry a CTC state */
#define SC_C_TOLD 7 /* sc_ctc_extend_state: rows the CTC states covered before this block */
/* decode-step launches (sc_ctc_prefix_scan, sc_ctc_gather_state): rows of the CTC table and of the
 * forward variables, when that differs from SC_C_T (0: same).  The reference never clears
 * CTCPrefixScorer.impl on reset() (scorers.py:342-350): the next utterance on the same object is
 * scored over the stale table until its own frames outgrow it, while attention sees SC_C_T frames. */
#define SC_C_TCTC 7

typedef struct sc_enc_layer {
  const float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo;
  const float *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
  const float *w1_p, *w2_p; /* sc_pack_panel_weight of w1, w2 (used when sc_ffn_ln_supported(d, F)) */
  const float *wqkv_p, *wo_p; /* sc_pack_panel_weight of wqkv, wo (used when sc_rowtile_proj_supported(d, d)) */
  const void *w1_h, *w2_h;    /* fp16 copies of w1_p / w2_p (same fragment order) or NULL: the fused FFN then runs
                                 fp16 MFMA inputs with fp32 accumulation (sc_ffn_ln_h) */
  const void *wqkv_h, *wo_h;  /* fp16 copies of wqkv_p / wo_p or NULL: the attention projections with fp16 MFMA inputs
                                 (sc_rowtile_proj_h) */
  const void *w1_s, *w2_s;    /* fp16 hi | lo SPLIT of w1_p / w2_p (weights.py split_panel_weight; same bytes) or NULL: the
                                 fused FFN then computes fp32-grade results with three fp16 MFMAs per product sum
                                 (sc_ffn_ln_s); takes precedence over w1_h / w2_h */
  const void *wqkv_s, *wo_s;  /* the same split of wqkv_p / wo_p or NULL (sc_rowtile_proj_s); precedence over wqkv_h / wo_h */
} sc_enc_layer;

typedef struct sc_dec_layer {
  const float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo;
  const float *ln2_g, *ln2_b, *wq, *bq, *wo2, *bo2;
  const float *ln3_g, *ln3_b, *w1, *b1, *w2, *b2;
  const float *wo_p, *wq_p, *wo2_p; /* sc_pack_lane_weight of wo, wq, wo2 (used when sc_proj_ln_proj_supported(d)) */
  const float *w1_p, *w2_p;         /* sc_pack_panel_weight of w1, w2 (used when sc_ffn_ln_supported(d, F)) */
  const float *wqkv_q;              /* sc_pack_lane_weight of wqkv (sc_ffn_ln_proj of the layer before) */
  const float *wqkv_pp, *wq_pp, *wo_pp, *wo2_pp; /* sc_pack_panel_weight of wqkv, wq, wo, wo2 (sc_dec_layer_self / _cross), or NULL */
  const void *w1_h, *w2_h;          /* fp16 copies of w1_p / w2_p or NULL (see sc_enc_layer) */
  const void *w1_s, *w2_s;          /* fp16 hi | lo split of w1_p / w2_p or NULL (see sc_enc_layer) */
  const void *wqkv_pph, *wq_pph, *wo_pph, *wo2_pph; /* fp16 copies of wqkv_pp / wq_pp / wo_pp / wo2_pp (same fragment order)
                                       or NULL: the layer kernels' projections with fp16 MFMA inputs, fp32 accumulation
                                       (BASELINE configs[4], with sc_search.act_half / out_w_qh; needs kv_half) */
} sc_dec_layer;

/* Search-side buffers of one StreamBatch (S streams, beam W, pre-beam K). */
typedef struct sc_search {
  int32_t S, W, K, V, d, H, F, n_layers, TCAP, LCAP;
  int32_t blank, eos, sos;
  float w_dec, w_ctc, ln_eps;
  const int32_t *ctrl; /* [S][8] */
  int32_t *flags;      /* [S] */
  const float *ctcx;   /* [S][TCAP][V]  CTC posterior table (quirk A1 rows) */
  const float *ckv;    /* [S][n_layers][TCAP][2d] cross-attention K|V */
  float *skv;          /* [S][n_layers][kv_rows][2d] self-attention K|V rows of a stream: a POOL (round 4) - a row holds
                          the K|V of one (position, hypothesis) token; sc_beam_prune hands every NEW hypothesis the row
                          of its newest token (the lowest rows no new hypothesis descends from: rows of pruned
                          hypotheses are free again), `anc` is the index.  The reference keeps a per-hypothesis output
                          cache instead and copies it when hypotheses fork (transformer_decoder.py:210-249).  Hypotheses of a beam share almost all of their
                          history (1.2 distinct rows per position at beam 10), so kv_rows ~ 1.5 x LCAP instead of the
                          W x LCAP of one slot per (position, hypothesis) */
  int32_t *yseq, *xpos; /* [2][S][W][LCAP] */
  int32_t *anc;         /* [2][S][LCAP][W] pool row (of skv) of the K|V row hypothesis h attends to at position p */
  double *score, *sc_dec, *sc_ctc; /* [2][S][W] */
  float *ctc_r;    /* [2][S][TCAP][2][W] forward variables r^n, r^b per hypothesis */
  float *ctc_s;    /* [2][S][W] prefix score log_psi of the chosen token */
  float *ctc_rnew; /* [S][ceil(TCAP/16)][2][W*K] r of every (hypothesis, candidate) at the CHECKPOINT frames t % 16 == 15
                      (row j = frame 16 j + 15): sc_ctc_gather_state rebuilds the winners' r[t] at every frame from them */
  float *dx, *dxn, *dqkv, *datt, *dq, *dffh, *logits, *logp; /* [S*W][...] */
  int32_t *pre_ids;       /* [S*W][K] */
  float *psi, *psi_eos;   /* [S*W][K], [S*W] */
  float *cand_score;      /* [S*W][W] */
  int32_t *cand_tok;      /* [S*W][W] */
  float *cand_ctc;        /* [S*W][W] */
  int32_t *sel;           /* [S][W][2] (parent hypothesis, candidate index) */
  const float *embed, *pe, *dec_norm_g, *dec_norm_b, *out_w, *out_b;
  const sc_dec_layer *layers; /* HOST array [n_layers] */
  /* Ragged-batch compaction of the dense decoder kernels (GEMMs, row panels,
   * LayerNorm): they process the first n_rows entries of rowmap, a permutation
   * of the S*W hypothesis rows that lists the rows of the ACTIVE streams first
   * (streams leave the lock-step decode loop at different steps).  rowmap NULL:
   * all S*W rows in order.  n_rows is a launch parameter (one captured graph
   * per bucket); rowmap is re-uploaded by the host together with ctrl. */
  const int32_t *rowmap;
  int32_t n_rows;
  const float *out_w_q; /* sc_pack_lane_weight of out_w (sc_ffn_ln_proj of the last layer), or NULL */
  /* head-parallel decoder layers (sc_dec_layer_*): per-head partial products of the two attention output
   * projections [S*W][H][d] and the feed-forward partial sums [max_ffn_part][S*W][d]; NULL: not used */
  float *ph1, *ph2, *ffn_part;
  int32_t max_ffn_part;
  /* column-major copy of the CTC table [S][V][tct] (tct = TCAP rounded up to a multiple of 4), maintained by
   * sc_ctc_extend_state and streamed by sc_ctc_prefix_scan (required) */
  int32_t tct;
  float *ctcxT;
  /* 1: the K|V caches ckv / skv hold IEEE fp16 elements (same element offsets, half the bytes); attention
   * arithmetic, softmax and everything else stay fp32.  Written through sc_kv_rows_to_half (cross) and by the
   * self-attention kernels (self); read by the single-pass attention kernels. */
  int32_t kv_half;
  /* measurement aid (bench.py: algorithmic bytes of the self-attention): when not NULL, every self-attention launch
   * adds the DISTINCT (position, slot) K|V rows it walked for a stream (plus its new rows) to stat_rows[0]
   * (sc_dec_self_attn) / stat_rows[1] (sc_dec_layer_self) / stat_rows[2] (sc_dec_layer_stream) - one atomic per (stream, layer) */
  unsigned long long *stat_rows;
  /* fp16 decoder mode (BASELINE configs[4]; opt-in, never the parity mode): out_w_qh = fp16 copy of out_w_q (the
   * output layer with fp16 MFMA inputs) or NULL; act_half bit 0 (1): the layer kernels use the fp16 weight copies
   * (*_pph) with fp16 MFMA inputs; bit 1 (2): the partial products between the decoder's kernels (ph1, ph2, ffn_part)
   * hold fp16 elements (same element offsets); bit 2 (4): the output layer uses out_w_qh.  LayerNorm, softmax,
   * log-softmax, CTC, scores: fp32. */
  const void *out_w_qh;
  int32_t act_half;
  int32_t kv_rows;   /* rows of the self-attention K|V pool per (stream, layer), <= 65536 */
  int32_t *kvflags;  /* [S] written by sc_beam_prune: 1 = the stream's pool is exhausted (its next step would compute
                        garbage: the host fails the stream with SC_ERR_CAPACITY), 0 = fine */
  float *ctc_rs;     /* [2][S][TCAP][W] log(exp r^n + exp r^b) of ctc_r, frame by frame (round 5): written wherever ctc_r is
                        (sc_ctc_extend_state, sc_ctc_gather_state) and read by the prefix scan, whose W x K lanes all
                        needed this sum of THEIR hypothesis at every frame - 2 of the 7 transcendentals per frame and lane */
} sc_search;

const char *sc_last_error(void);
/* ABI revision of this header: bumped whenever a struct layout or a signature changes incompatibly.  sc_version()
 * returns the revision the LIBRARY was built with; a host compares the two before it passes any struct
 * (speechcatcher_amd/_abi.py does at load time, the C hosts in tests/ at start-up). */
#define SC_ABI_VERSION 12
int sc_version(void);

/* hipGraph capture / replay of any sequence of the launches below on a
 * non-default stream: begin, issue the launches, end -> executable graph. */
int sc_graph_capture_begin(void *stream);
int sc_graph_capture_end(void *stream, void **graph_exec /*HOST out*/);
int sc_graph_launch(void *graph_exec, void *stream);
int sc_graph_destroy(void *graph_exec);

/* ---- generic building blocks -------------------------------------------- */

/* C[c_rows[m], n] (+)= sum_k A[a_rows[m]*lda + kofs(k)] * W[n*K + k] + bias[n]
 * (torch.nn.Linear call sites: multi_head_attention.py:81-83,133,
 * feed_forward.py:50, subsampling.py:98, ctc.py:40, transformer_decoder.py:249;
 * with conv_f1 > 0 the second Conv2d of subsampling.py:87-93 as an implicit
 * GEMM: lda = channels, tap = k / lda, kofs = ((tap/3)*conv_f1 + tap%3)*lda + k%lda).
 * f32 MFMA (v_mfma_f32_32x32x2_f32), K must be a multiple of 32. */
int sc_gemm(const float *A, const int32_t *a_rows, int lda, const float *W, const float *bias,
            float *C, const int32_t *c_rows, int ldc, int M, int N, int K, int flags, int conv_f1,
            void *stream);

/* sc_gemm followed by LayerNorm of the produced rows (pre-LN transformer:
 * x += proj(...); xn = LN(x): decoder_layer.py:101-123, transformer_decoder.py:243).
 * ln_out[m*ld_ln ..] = LN(C[c_rows[m]]).  The LayerNorm is fused into the
 * split-K reduce when the workspace is set.  N must be a multiple of 4 and at most 1024, ldc and
 * ld_ln multiples of 4 (what the LayerNorm kernels cover): anything else is refused with SC_ERR_ARG
 * before a launch.  K >= 2560 is cut into 8 slices whatever M is (row slabs when the partial sums of
 * all rows do not fit the workspace), so C has the bits sc_gemm gives. */
int sc_gemm_ln(const float *A, const int32_t *a_rows, int lda, const float *W, const float *bias,
               float *C, const int32_t *c_rows, int ldc, int M, int N, int K, int flags, int conv_f1,
               const float *ln_g, const float *ln_b, float ln_eps, float *ln_out, int ld_ln,
               void *stream);

/* Row-panel form of "attention output projection + residual + LayerNorm
 * (+ next projection)" for the decoder layer (decoder_layer.py:101-123:
 * x = residual + self_attn(..); x = norm2(x); src_attn's linear_q,
 * multi_head_attention.py:58-60):
 *   X[m] += A[m] . W1^T + b1;  XN[m] = LN(X[m]) (if XN);  Q[m] = LN(X[m]) . W2^T + b2 (if W2).
 * One workgroup owns 4, 8 or 16 complete rows (D = 64, 128 or 256), so the LayerNorm
 * and the second projection need no second launch.  v_mfma_f32_4x4x1_16B_f32.
 * A must be 16-byte aligned with lda % 4 == 0.  rows (optional): the M rows of
 * A / X / XN / Q to process (NULL: rows 0..M-1). */
int sc_proj_ln_proj(const float *A, int lda, const float *W1q, const float *b1, float *X, int ldx,
                    const float *ln_g, const float *ln_b, float ln_eps, float *XN, int ldn,
                    const float *W2q, const float *b2, float *Q, int ldq, const int32_t *rows,
                    int M, int D, void *stream);
int sc_proj_ln_proj_supported(int D);
/* W1q / W2q: the [D][D] Linear weights re-ordered ONCE so that lane l of a wave reads
 * W[64*tile + l][4*q .. 4*q+3] as one 16-byte element (N % 64 == 0, K % 4 == 0):
 *   out[((tile*(K/4) + q)*64 + lane)*4 + c] = W[tile*64 + lane][4*q + c]            */
int sc_pack_lane_weight(const float *W, int N, int K, float *out, void *stream);
/* Fragment order of the 16x16x4-MFMA kernels (sc_ffn_ln; N % 16 == 0, K % 32 == 0):
 *   out[((((tile*(K/32) + ki)*2 + half)*64 + lane)*4 + c]
 *       = W[tile*16 + lane%16][ki*32 + 8*(lane/16) + 4*half + c]              */
int sc_pack_panel_weight(const float *W, int N, int K, float *out, void *stream);

/* Fused position-wise feed-forward (feed_forward.py:48-50 + the residual of the
 * encoder / decoder layer, + the LayerNorm that follows when ln_out != NULL):
 *   X[r] += W2 . relu(W1 . XN[r] + b1) + b2;  ln_out[r] = LN(X[r])   for r in rows[0..M)
 * (rows NULL: r = 0..M-1; ln_out may alias XN).  The hidden activations stay in
 * LDS; W1p [F][D] and W2p [D][F] are sc_pack_panel_weight copies.  Needs the
 * split-K workspace (sc_set_workspace / sc_set_stream_workspace). */
int sc_ffn_ln(const float *XN, const int32_t *rows, int M, int D, int F, const float *W1p,
              const float *b1, const float *W2p, const float *b2, float *X, const float *ln_g,
              const float *ln_b, float ln_eps, float *ln_out, void *stream);
int sc_ffn_ln_supported(int D, int F);
/* Row-tile projection with the LayerNorms around it folded in (K = D):
 *   C[r] = LN(A[r]; ln_g, ln_b) . W^T + bias            (ln_g NULL: A[r] as is)
 *   R != NULL or LN2 != NULL (needs N == D):  C[r] += R[r];  LN2[r] = LN(C[r]; g2, b2)
 * the encoder layer's q|k|v Linear behind norm1 (multi_head_attention.py:63-90,
 * contextual_block_encoder_layer.py:190-215) and its attention output Linear + residual
 * followed by norm2 (:216-240), one launch each.  W [N][D] in sc_pack_panel_weight order,
 * N a multiple of 128, D in {128, 256}; R may be C.  LN2 has leading dimension D. */
int sc_rowtile_proj(const float *A, int lda, int M, int D, const float *ln_g, const float *ln_b,
                    float eps, const float *Wp, const float *bias, int N, const float *R, float *C,
                    int ldc, const float *g2, const float *b2, float *LN2, void *stream);
/* ... with fp16 weights (Wh = the fragment-packed copy with 2-byte elements) and fp16 MFMA inputs: BASELINE configs[4] */
int sc_rowtile_proj_h(const float *A, int lda, int M, int D, const float *ln_g, const float *ln_b,
                      float eps, const void *Wh, const float *bias, int N, const float *R, float *C,
                      int ldc, const float *g2, const float *b2, float *LN2, void *stream);
/* ... with the fp16 hi | lo split of the fp32 weights (see sc_ffn_ln_s): fp32-grade results from fp16 MFMA inputs */
int sc_rowtile_proj_s(const float *A, int lda, int M, int D, const float *ln_g, const float *ln_b,
                      float eps, const void *Ws, const float *bias, int N, const float *R, float *C,
                      int ldc, const float *g2, const float *b2, float *LN2, void *stream);
int sc_rowtile_proj_supported(int D, int N);
/* The same feed-forward followed by the projection that consumes its LayerNorm - the next decoder
 * layer's Q|K|V (decoder_layer.py:85-100 of layer l+1) or the output layer
 * (transformer_decoder.py:243-249) - with the split-sum reduce, residual, LayerNorm and projection
 * in ONE row-panel launch:
 *   Xout[r] = Xin[r] + FFN(XN[r]);  ln_out[r] = LN(Xout[r]) (optional);  Q[r] = LN(Xout[r]) . Wq^T + bq
 * Wq [N][D] in sc_pack_lane_weight order, N a multiple of D, Q leading dimension N.  Xin and Xout
 * must be different buffers.  Needs a workspace that holds all M rows (else returns an error). */
int sc_ffn_ln_proj(const float *XN, const int32_t *rows, int M, int D, int F, const float *W1p,
                   const float *b1, const float *W2p, const float *b2, const float *Xin, float *Xout,
                   const float *ln_g, const float *ln_b, float ln_eps, float *ln_out, const float *Wq,
                   const float *bq, float *Q, int N, void *stream);
/* ... with fp16 weights: W1h / W2h = the fragment-packed copies with 2-byte elements; fp16 MFMA inputs (activations
 * rounded to fp16 when staged), fp32 accumulation, bias, ReLU input, partial sums, residual and LayerNorm in fp32 */
int sc_ffn_ln_h(const float *XN, const int32_t *rows, int M, int D, int F, const void *W1h, const float *b1,
                const void *W2h, const float *b2, float *X, const float *ln_g, const float *ln_b, float ln_eps,
                float *ln_out, void *stream);
int sc_ffn_ln_proj_h(const float *XN, const int32_t *rows, int M, int D, int F, const void *W1h, const float *b1,
                     const void *W2h, const float *b2, const float *Xin, float *Xout, const float *ln_g,
                     const float *ln_b, float ln_eps, float *ln_out, const float *Wq, const float *bq, float *Q, int N,
                     void *stream);
/* ... with the fp16 hi | lo SPLIT of the fp32 weights (W1s / W2s: weights.py split_panel_weight - per lane and 32-wide
 * k block the fp16 roundings of its 8 k values in the first slab of the fragment order, fp16((w - hi) * 2^11) in the
 * second; the same bytes as the fp32 copies): every product sum is evaluated as
 * sum(a_hi w_hi) + 2^-11 (sum(a_hi w_lo) + sum(a_lo w_hi)) with fp16 MFMA inputs and fp32 accumulation, the
 * activations split the same way when staged.  Differs from the fp32 kernel by a few fp32 ulp (the dropped
 * a_lo w_lo terms: <= 2^-22 relative), at ~1/5 of its matrix-pipe cycles.  Operands must lie within fp16's range. */
int sc_ffn_ln_s(const float *XN, const int32_t *rows, int M, int D, int F, const void *W1s, const float *b1,
                const void *W2s, const float *b2, float *X, const float *ln_g, const float *ln_b, float ln_eps,
                float *ln_out, void *stream);
int sc_ffn_ln_proj_s(const float *XN, const int32_t *rows, int M, int D, int F, const void *W1s, const float *b1,
                     const void *W2s, const float *b2, const float *Xin, float *Xout, const float *ln_g,
                     const float *ln_b, float ln_eps, float *ln_out, const float *Wq, const float *bq, float *Q, int N,
                     void *stream);
/* bytes of the split-K workspace registered for `stream` (0: none).  sc_decoder_layers /
 * sc_encoder_layers use the fused FFN only when a workspace is available and fall back to
 * two GEMMs otherwise. */
size_t sc_workspace_bytes(void *stream);

/* Workspace (device memory, caller-owned) for the deterministic split-K path of
 * sc_gemm: partial sums [ksplit][M][N] reduced in fixed order.  Without it
 * sc_gemm never splits K. */
int sc_set_workspace(void *ptr, size_t bytes);
/* per-stream workspace (several StreamBatches running concurrently on their own
 * streams must not share partial-sum storage); ptr == NULL unregisters */
int sc_set_stream_workspace(void *stream, void *ptr, size_t bytes);

/* Optional per-launch timing of sc_gemm with HIP events on the launch stream
 * (every `sample_every`-th launch; 0 disables).  sc_prof_collect synchronises
 * and returns, per kernel variant v (0 scalar, 2 = 128x128 tile, 3 = 64x64;
 * 1 stays empty): summed milliseconds, summed algorithmic flops (2*M*N*K) and the
 * number of sampled launches.  All three pointers are HOST arrays of 4. */
/* kernel kinds of the per-launch timing records */
#define SC_PROF_GEMM_NAIVE 0
#define SC_PROF_GEMM_SKINNY 1 /* no kernel records this kind any more; the number stays, callers index the kinds by position */
#define SC_PROF_GEMM_128 2
#define SC_PROF_GEMM_64 3
#define SC_PROF_PROJ_LN_PROJ 4
#define SC_PROF_FFN_FUSED 5
#define SC_PROF_ATTN_SELF 6
#define SC_PROF_ATTN_CROSS 7
#define SC_PROF_ROWTILE_PROJ 8
#define SC_PROF_FFN_PRO 9 /* ffn_fused_kernel<.., PRO>: sc_dec_layer_ffn (head-partial reduce + norm3 prologue) */
#define SC_PROF_LAYER_SELF 10  /* dec_layer_attn_kernel<.., SELF>: sc_dec_layer_self (head-parallel layer, small buckets) */
#define SC_PROF_LAYER_CROSS 11 /* dec_layer_attn_kernel<.., cross>: sc_dec_layer_cross */
#define SC_PROF_LAYER_STREAM 12 /* dec_layer_stream_kernel: sc_dec_layer_stream (stream-resident layer, large buckets; round 6) */
#define SC_PROF_KINDS 13
/* decoder layers run as head-parallel launches (sc_dec_layer_*) for compaction buckets up to this many rows */
#define SC_FUSED_MAX_ROWS 960
/* ... with one head per workgroup; from SC_HPW_MIN_ROWS rows on with FOUR heads per workgroup (1024 threads: the
 * prologue reduce + LayerNorm once per four heads, H/4 partial products per row).  Measured on the default bench
 * (continuous, tools/ab_hpw.sh, SC_HPW_MIN = never / 0 / 160 / 320 / 640 / 800 / 960): 2967 / 3109 / 3074 / 3024 / 3094 /
 * 3055 / 3035 audio-s/s; strict lock-step, where the medium buckets count (tools/ab_hpw_strict.sh, 96 / 320 / 480 / 640 /
 * 960 / never): 2038 / 2137 / 2159 / 2126 / 2195 / 2151 - four heads from half of a 128-stream batch on */
#define SC_HPW_MIN_ROWS 640
/* (round 6) ... and from SC_STREAM_MIN_ROWS rows on in the STREAM-RESIDENT form (decoder_stream.hip: one 512-thread workgroup of
 * 8 waves per stream runs both attentions of a layer for all heads, two launches per layer): buckets of more than 128 streams
 * at beam 10, of at least 257 at beam 5.  A stream then holds one compute unit instead of two, and the encoder groups run beside
 * the decode chain instead of between its kernels.  Same bits as the other two forms (canonical summation, common.h).
 * SC_STREAM_FFN_CUS: compute units its feed-forward launch is sized for (a constant of the build, like the thresholds). */
#define SC_STREAM_MIN_ROWS 1281
#define SC_STREAM_FFN_CUS 256
int sc_prof_collect_kinds(double *ms, double *flops, double *bytes, long long *n, int nkinds);
int sc_prof_enable(int sample_every);
int sc_prof_collect(double *ms, double *flops, long long *n);
/* same, plus summed ALGORITHMIC bytes (A + W read once, C written; C read too with SC_GEMM_RESIDUAL) */
int sc_prof_collect2(double *ms, double *flops, double *bytes, long long *n);
/* median duration (ms) of an empty event pair on `stream`: the bias that event
 * bracketing adds to each sampled launch */
double sc_prof_event_overhead_ms(void *stream);

/* LayerNorm over rows (model/layers/normalization.py:7-24, eps 1e-12). */
int sc_layernorm(const float *src, const int32_t *src_rows, int lds, float *dst,
                 const int32_t *dst_rows, int ldd, int M, int d, const float *gamma,
                 const float *beta, float eps, void *stream);

int sc_copy_rows(const float *src, const int32_t *src_rows, float *dst, const int32_t *dst_rows,
                 int n, int width, void *stream);

/* in-place log_softmax of selected rows (scorers.py:133-134, first block only) */
int sc_log_softmax_rows(float *x, const int32_t *rows, int n, int V, void *stream);

/* ---- CTC forced alignment (align.hip) -------------------------------------
 * Viterbi alignment of a label sequence y[0..L) against T rows of a CTC emission table (the 2L+1 states blank, y0,
 * blank, y1, ..., blank; a path starts in state 0 or 1 and ends in state 2L or 2L-1).  For a state s >= 1:
 *   delta[t][s] = max(delta[t-1][s], delta[t-1][s-1], delta[t-1][s-2] if s is a label state and y != the previous
 *   label) + e[t][label(s)]
 * with the candidates compared in the order s, s-1, s-2, a later one taking over only if strictly greater (the final
 * state: 2L only if strictly greater than 2L-1).  The adds are fp32 in frame order, on the stored values of the table
 * (the path does not change when a row is shifted by a constant).  Per token: its frames [start, end) and logp_mean, the
 * mean over those frames of e[t][y] - logsumexp_v e[t][v].  The table is only read. */
#define SC_ALIGN_OK 0
#define SC_ALIGN_INFEASIBLE 1 /* T < L + number of adjacent repeats in y */
#define SC_ALIGN_NONFINITE 2  /* a row of the table holds a non-finite value */
#define SC_ALIGN_BAD_INPUT 3  /* a label outside [0, V) or equal to blank, a blank outside [0, V), L > SC_ALIGN_MAX_L */
#define SC_ALIGN_MAX_L 1023
typedef struct sc_ctc_align_job {
  const float *emis;       /* row t of the table at emis + t * stride, V floats (device) */
  const int32_t *labels;   /* [L] (device) */
  void *ws;                /* sc_ctc_align_ws_bytes(T) bytes of device workspace, 256-byte aligned */
  int32_t *start;          /* [L] first frame of each token (device; -1 unless status is SC_ALIGN_OK) */
  int32_t *end;            /* [L] one past its last frame */
  float *logp_mean;        /* [L] */
  float *path_score;       /* [1] sum of the emissions along the path (-inf unless SC_ALIGN_OK) */
  int32_t *status;         /* [1] SC_ALIGN_* */
  int64_t stride;          /* floats between two rows */
  int32_t T, L, V, blank;
} sc_ctc_align_job;
size_t sc_ctc_align_ws_bytes(int T);
/* jobs: device table of n_jobs entries; max_T / max_L bound their T and L (max_L <= SC_ALIGN_MAX_L).  Two launches on
 * `stream`: per-row logsumexp, then one wave per job. */
int sc_ctc_align(const sc_ctc_align_job *jobs, int n_jobs, int max_T, int max_L, void *stream);

/* ---- CTC speech activity (activity.hip) ----------------------------------------------------
 * The blank posterior of a CTC row is the acoustic "nothing is being said here" signal.  For a row x[0..V) of an fp32
 * table, promoted to float64:
 *   m = max_v x[v];  lse = m + log(sum_v exp(x[v] - m));  p_blank = exp(x[blank] - lse)
 * (-inf entries contribute 0; a row that holds a NaN or +inf, or nothing but -inf, is a BAD frame: p_blank = NaN).  A frame
 * is SILENCE iff it is bad or p_blank > thr, else SPEECH.  A per-row constant does not enter, so raw-logit rows and rows the
 * search has log-softmaxed in place give the same posteriors up to rounding.  The state of a stream is six int32 over the
 * frames scanned so far in its utterance, numbered in the order they are scanned: */
#define SC_ACT_N_FRAMES 0
#define SC_ACT_N_SPEECH 1
#define SC_ACT_N_BAD 2
#define SC_ACT_FIRST_SPEECH 3  /* -1: none */
#define SC_ACT_LAST_SPEECH 4   /* -1: none */
#define SC_ACT_TRAIL_SILENCE 5 /* n_frames - 1 - last_speech, or n_frames when there was no speech */
typedef struct sc_activity_t {
  int32_t n_frames, n_speech, n_bad, first_speech, last_speech, trail_silence;
} sc_activity_t;
typedef struct sc_ctc_activity_job {
  const float *table;   /* row t of the table at table + t * stride, V floats (device) */
  int32_t *state;       /* [6] SC_ACT_*: read (unless restart), advanced over the span, written back (device) */
  double *track;        /* p_blank of row t -> track[t] for t in [t0, t1) (device; NULL: not kept) */
  int32_t *state_after; /* [6] second copy of the new state, e.g. in host-mapped memory (NULL: none) */
  int64_t stride;       /* floats between two rows */
  double thr;
  int32_t V, blank, t0, t1;
  int32_t restart;      /* != 0: the stored state is ignored, the span starts an utterance (0, 0, 0, -1, -1, 0) */
  int32_t reserved;
} sc_ctc_activity_job;
#define SC_ACTIVITY_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job: float64 sums in one fixed order, no
 * atomics, one writer per output; an empty span (t0 == t1) rewrites the state unchanged.  n_jobs < 0, a null table with
 * n_jobs > 0 or n_jobs > SC_ACTIVITY_MAX_JOBS: SC_ERR_ARG before anything is launched.  A job whose own fields are
 * malformed (null table / state, V < 1, blank outside [0, V), t0 < 0, t1 < t0) writes nothing.  Two jobs of one call
 * must not share a state or overlap in a track. */
int sc_ctc_activity(const sc_ctc_activity_job *jobs, int n_jobs, void *stream);

/* ---- CTC phrase spotting (spot.hip) ---------------------------------------------------------
 * A phrase set holds P <= SC_SPOT_MAX_PHRASES phrases; phrase p is a label sequence y[0..L), 1 <= L <= SC_SPOT_MAX_LEN,
 * labels in [0, V) and not the blank, with a floor min_score <= 0.  It has S = 2L - 1 states (state 2i: token y[i], state
 * 2i + 1: the blank between y[i] and y[i + 1]), each a float64 value and an int32 start; -inf / -1 at the start of an
 * utterance.  For frame n (numbered in the order the frames are scanned) with row x, promoted to float64: a BAD row (a
 * NaN, a +inf, or nothing but -inf) sets every state of every enabled phrase to -inf / -1; else, with m = max_v x[v] and
 * e(s) = x[label(s)] - m, every state takes the best of { stay V[s]; V[s-1]; V[s-2] if s is even, s >= 2 and
 * y[s/2] != y[s/2-1]; for s == 0 a fresh start 0.0 with start n } of the PREVIOUS frame - compared in this order, a later
 * candidate taking over only if strictly greater - plus e(s), and the winner's start (-1 when the value is -inf).  The
 * phrase FIRES iff the new value of its end state 2L - 2 is >= min_score: event (end = n, phrase, start, score), then all
 * its states become -inf / -1.  The score is the log-ratio of the phrase's path to the frame-wise best path: a per-row
 * constant cancels, raw logits and log-softmaxed rows mean the same.  Events are ordered by (end, phrase); the first
 * SC_SPOT_MAX_EVENTS of an utterance are stored, n_events counts all.  tests/ctc_spot_ref.py is the contract; the kernel
 * reproduces it bit for bit. */
#define SC_SPOT_MAX_PHRASES 64
#define SC_SPOT_MAX_LEN 32
#define SC_SPOT_STATES 64      /* entries per phrase in the state block; [2L - 1, 64) stay -inf / -1 */
#define SC_SPOT_MAX_EVENTS 64
typedef struct sc_spot_event {
  int32_t end, phrase, start, reserved; /* frames of the utterance, both inclusive; reserved = 0 */
  double score;
} sc_spot_event;
typedef struct sc_spot_t {
  int32_t n_frames, n_events;
} sc_spot_t;
typedef struct sc_ctc_spot_job {
  const float *table;      /* row t of the table at table + t * stride, V floats (device) */
  const int32_t *labels;   /* [P][SC_SPOT_MAX_LEN] (device) */
  const int32_t *lens;     /* [P] (device) */
  const double *floors;    /* [P] min_score (device) */
  int32_t *counters;       /* [2] n_frames, n_events: read (unless restart), advanced over the span, written back (device) */
  double *values;          /* [P][SC_SPOT_STATES] (device) */
  int32_t *starts;         /* [P][SC_SPOT_STATES] (device) */
  sc_spot_event *events;   /* [SC_SPOT_MAX_EVENTS]: event k of the utterance at events[k] (device) */
  int32_t *state_after;    /* [2] second copy of the new counters, e.g. in host-mapped memory (NULL: none) */
  int64_t stride;          /* floats between two rows, >= V */
  uint64_t mask;           /* bit p: phrase p is enabled; a disabled phrase's states are not touched */
  int32_t V, blank, t0, t1;
  int32_t restart;         /* != 0: the stored state is ignored, the span starts an utterance */
  int32_t P;
} sc_ctc_spot_job;
#define SC_SPOT_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job; no atomics, one writer per
 * output; an empty span (t0 == t1) rewrites the counters unchanged.  n_jobs < 0, a null table with n_jobs > 0 or
 * n_jobs > SC_SPOT_MAX_JOBS: SC_ERR_ARG before anything is launched.  A job whose own fields are malformed (a null
 * pointer other than state_after, V < 1, blank outside [0, V), t0 < 0, t1 < t0, stride < V, P outside [1, 64], a length
 * outside [1, 32], a label outside [0, V) or equal to the blank) writes nothing.  Two jobs of one call must not share
 * a state block or an events array. */
int sc_ctc_spot(const sc_ctc_spot_job *jobs, int n_jobs, void *stream);

/* ---- CTC draft transcript (draft.hip) --------------------------------------------------------
 * The collapsed arg-max path of the CTC rows: token ids with frame times and a posterior, known as soon as the encoder
 * has emitted the frames.  For a row x[0..V) of an fp32 table: a row that holds a NaN or +inf, or nothing but -inf, is a
 * BAD frame; else k = argmax_v x[v] on the fp32 values, the LOWEST index among ties, and p = exp(x[k] - lse) with x
 * promoted to float64 and lse = m + log(sum_v exp(x[v] - m)) as for sc_ctc_activity.  A per-row constant cancels: raw
 * logits and log-softmaxed rows give the same labels unless fp32 rounding creates a tie.  Frames are numbered in the
 * order they are scanned.  For frame n: a bad row or k == blank closes the open token, if any (a bad row also counts in
 * n_bad); k == open_id sets open_end = n and open_conf = max(open_conf, p); any other k closes the open token, if any,
 * and opens (k, n, n, p).  Closed = written to the token store at slot n_closed (counted, not written, at or beyond the
 * capacity), then n_closed += 1; a stored token is never touched again.  The draft of a state is its stored tokens
 * followed by the open token, if any.  tests/ctc_draft_ref.py is the contract: every int32 equal, conf within 1e-12 (the
 * lanes sum in another order than v ascending). */
typedef struct sc_draft_t {
  int32_t n_frames, n_closed, n_bad;
  int32_t open_id, open_start, open_end; /* -1: no open token */
  double open_conf;                      /* 0.0: no open token */
} sc_draft_t;
typedef struct sc_draft_token {
  int32_t id, start, end, reserved; /* frames of the utterance, both inclusive; reserved = 0 */
  double conf;                      /* the largest arg-max posterior among the token's frames */
} sc_draft_token;
typedef struct sc_ctc_draft_job {
  const float *table;      /* row t of the table at table + t * stride, V floats (device) */
  sc_draft_t *state;       /* read (unless restart), advanced over the span, written back (device) */
  sc_draft_token *tokens;  /* [capacity]: token k of the utterance at tokens[k] (device; may be NULL when capacity == 0) */
  sc_draft_t *state_after; /* second copy of the new state, e.g. in host-mapped memory (NULL: none) */
  int64_t stride;          /* floats between two rows, >= V */
  int32_t V, blank, t0, t1;
  int32_t restart;         /* != 0: the stored state is ignored, the span starts an utterance (0, 0, 0, -1, -1, -1, 0.0) */
  int32_t capacity;        /* slots of the token store, >= 0 */
} sc_ctc_draft_job;
#define SC_DRAFT_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job; no atomics, one writer per
 * output; an empty span (t0 == t1) rewrites the state unchanged.  n_jobs < 0, a null table with n_jobs > 0 or
 * n_jobs > SC_DRAFT_MAX_JOBS: SC_ERR_ARG before anything is launched.  A job whose own fields are malformed (null table /
 * state, a null store with capacity > 0, V < 1, blank outside [0, V), t0 < 0, t1 < t0, stride < V, capacity < 0) writes
 * nothing.  Two jobs of one call must not share a state or a token store. */
int sc_ctc_draft(const sc_ctc_draft_job *jobs, int n_jobs, void *stream);

/* ---- CTC prefix beam search (ctc_beam.hip) ----------------------------------------------------
 * An n-best list of token prefixes with their CTC prefix probabilities, from the rows the draft reads.  The state of a
 * stream holds n_entries <= B entries, best first: the prefix `node` of the stream's prefix tree (0: the empty prefix),
 * its last token (-1: none), its length, the node of the prefix without that token (-1: none) and the float64 log
 * probabilities pb / pnb of the prefix with the path ending in blank / in `last`; the unused slots hold
 * (-1, -1, 0, -1, -inf, -inf).  The tree is a store of (parent, token, frame) records, node k of the utterance at slot k
 * ((-1, -1, -1) at slot 0), never touched once stored; a node at or beyond the capacity is counted, not written.  A state
 * of more than B entries is cut to its first B.  Frames are numbered in the order they are scanned.  For frame n with row
 * x[0..V): a BAD row (a NaN, a +inf, or nothing but -inf) counts in n_bad and n_frames and changes nothing else; else,
 * with lse as for sc_ctc_activity, lp(v) = (double)x[v] - lse and lae(a, b) = max + log1p(exp(min - max)) (the other
 * argument when one is -inf):
 *   candidates   the C non-blank tokens with the largest x, compared as fp32, the lowest index among ties, none at -inf
 *   stay         tot_i = lae(pb_i, pnb_i);  pb'_i = tot_i + lp(blank);  pnb'_i = pnb_i + lp(last_i) if last_i is a
 *                candidate, else -inf
 *   extension    of entry i by candidate c: ext = (c == last_i ? pb_i : tot_i) + lp(c); if an entry j has
 *                parent_j == node_i and last_j == c: pnb'_j = lae(pnb'_j, ext), else a new prefix (-inf, ext)
 *   prune        the B best by total = lae(pb', pnb'), none at -inf; total descending, then stays before new prefixes,
 *                then the lower rank i, then the lower token; kept new prefixes become the nodes n_nodes, n_nodes + 1,
 *                ... in that order with the record (node_i, c, n)
 * tests/ctc_beam_ref.py is the contract: every int32 equal wherever no prune decision is a near-tie, pb / pnb within
 * 64 n_frames 2^-53 max(1, |value|) (the lanes sum lse in another order than v ascending); chained spans give the bits
 * of one span. */
#define SC_BEAM_MAX 16             /* B and C are at most this */
typedef struct sc_beam_entry {
  int32_t node, last, len, parent;
  double pb, pnb;
} sc_beam_entry;
typedef struct sc_beam_t {
  int32_t n_frames, n_bad, n_nodes, n_entries;
  sc_beam_entry e[SC_BEAM_MAX];
} sc_beam_t;
typedef struct sc_beam_node {
  int32_t parent, token, frame, reserved; /* frame of the utterance at which the token was first emitted; reserved = 0 */
} sc_beam_node;
typedef struct sc_ctc_beam_job {
  const float *table;      /* row t of the table at table + t * stride, V floats (device) */
  sc_beam_t *state;        /* read (unless restart), advanced over the span, written back (device) */
  sc_beam_node *nodes;     /* [capacity]: node k of the utterance at nodes[k] (device; may be NULL when capacity == 0) */
  sc_beam_t *state_after;  /* second copy of the new state, e.g. in host-mapped memory (NULL: none) */
  int64_t stride;          /* floats between two rows, >= V */
  int32_t V, blank, t0, t1;
  int32_t restart;         /* != 0: the stored state is ignored, the span starts an utterance (node 0 is stored) */
  int32_t capacity;        /* slots of the node store, >= 0; 1 + B * frames of the utterance cannot overflow */
  int32_t B, C;            /* entries kept, candidate tokens per frame: both in [1, SC_BEAM_MAX] */
} sc_ctc_beam_job;
#define SC_BEAM_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job; no atomics, one writer per
 * output; an empty span (t0 == t1) rewrites the state (cut to B entries).  n_jobs < 0, a null table with n_jobs > 0 or
 * n_jobs > SC_BEAM_MAX_JOBS: SC_ERR_ARG before anything is launched.  A job whose own fields are malformed (null table /
 * state, a null store with capacity > 0, V < 1, blank outside [0, V), t0 < 0, t1 < t0, stride < V, capacity < 0, B or C
 * outside [1, SC_BEAM_MAX], a stored n_entries outside [0, SC_BEAM_MAX] without restart) writes nothing.  Two jobs of one
 * call must not share a state or a node store. */
int sc_ctc_beam(const sc_ctc_beam_job *jobs, int n_jobs, void *stream);

/* Entries of beam states as token sequences: entry `rank` of *state, walked up its parent chain.  header[0] = the
 * entry's len (-1 unless SC_BEAM_PACK_OK / _TRUNCATED), header[1] = status, header[2] = node, header[3] = last;
 * scores[0..2) = pb, pnb (NaN without an entry); ids / frames [0, min(len, max_len)): the tokens and the frames of their
 * first emission, in order.  SC_BEAM_PACK_NO_ENTRY: rank outside [0, n_entries); SC_BEAM_PACK_TRUNCATED: len > max_len,
 * the first max_len tokens are written; SC_BEAM_PACK_BROKEN: a node of the chain lies at or beyond the capacity or
 * n_nodes, or the chain does not end at node 0 after len steps - ids and frames are then unspecified inside
 * [0, min(len, max_len)).  Nothing is written outside those sizes. */
#define SC_BEAM_PACK_OK 0
#define SC_BEAM_PACK_NO_ENTRY 1
#define SC_BEAM_PACK_TRUNCATED 2
#define SC_BEAM_PACK_BROKEN 3
typedef struct sc_ctc_beam_pack_job {
  const sc_beam_t *state;    /* (device) */
  const sc_beam_node *nodes; /* [capacity] (device; may be NULL when capacity == 0) */
  int32_t *ids;              /* [max_len] (device; may be NULL when max_len == 0) */
  int32_t *frames;           /* [max_len] */
  int32_t *header;           /* [4] len, status, node, last (device) */
  double *scores;            /* [2] pb, pnb (device) */
  int32_t capacity, rank, max_len, reserved;
} sc_ctc_beam_pack_job;
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one thread per job; the states and stores are only
 * read.  SC_ERR_ARG before anything is launched as for sc_ctc_beam.  A malformed job (a null state / header / scores, a
 * null ids / frames with max_len > 0, a null store with capacity > 0, capacity < 0, max_len < 0) writes nothing. */
int sc_ctc_beam_pack(const sc_ctc_beam_pack_job *jobs, int n_jobs, void *stream);

/* ---- n-gram language model fused into the CTC prefix beam (lm_blob.h, ctc_beam.hip) ---------------
 * The model is a backoff n-gram over the token ids [0, V), order 1..SC_LM_MAX_ORDER, held as a backoff automaton:
 *   state   a context the model holds; state 0 is the empty context.  Per state backoff (float64, natural log) and
 *           bo_state, the state of the longest proper suffix of the context that the model holds (the context without its
 *           oldest token when the model is closed under suffixes).  Following bo_state reaches 0 in at most
 *           SC_LM_MAX_ORDER - 1 steps.
 *   arc     (state, token) -> (logp float64, next): next = the state of the longest suffix of context + token that the
 *           model holds.  State 0's arcs are the dense arrays root_logp[V] / root_next[V], never searched; the arcs of all
 *           other states are the slots of ONE open-addressing hash table: key = ((uint64)state << 32) | token, home slot
 *           (key * SC_LM_HASH_MUL mod 2^64) >> (64 - log2 n_slots), linear probing (slot + 1 mod n_slots); an unused slot has
 *           the key SC_LM_EMPTY.  n_slots is a power of two >= 2 and every probe run ends at an unused slot.
 *   score(s, c):  acc = 0.0;  while s != 0 and (s, c) has no arc: acc = acc + backoff[s], s = bo_state[s];
 *                 -> (acc + logp[s, c], next[s, c])       float64 additions in exactly this order; all values finite
 * The blob (little endian; speechcatcher_amd/ngram.py packs it): sc_lm_header; double backoff[n_states]; int32 bo_state
 * [n_states]; double root_logp[V]; int32 root_next[V]; sc_lm_slot slots[n_slots] - every int32 array padded to a multiple of
 * 8 bytes.  sc_lm_create validates all of it on the host (sizes against the header, every bo_state / next in range, the
 * bo_state chains, finite values, no key twice, an unused slot in every probe run, every key's state and token in range and
 * the key reachable from its home slot) BEFORE a byte reaches the device: SC_ERR_ARG and nothing allocated otherwise.  The
 * model is uploaded once and read-only afterwards; it must outlive every launch and every sc_streams that uses it. */
#define SC_LM_MAX_ORDER 5
#define SC_LM_MAGIC 0x4D4C4353 /* "SCLM" */
#define SC_LM_VERSION 1
#define SC_LM_EMPTY 0xFFFFFFFFFFFFFFFFull
#define SC_LM_HASH_MUL 0x9E3779B97F4A7C15ull
typedef struct sc_lm_header {
  int32_t magic, version, V, order, n_states, n_arcs /* used slots */, n_slots, start_state;
} sc_lm_header;
typedef struct sc_lm_slot {
  uint64_t key;
  double logp;
  int32_t next, reserved; /* reserved = 0 */
} sc_lm_slot;
typedef struct sc_lm_view { /* the automaton as the kernel reads it (device pointers) */
  const double *backoff;
  const int32_t *bo_state;
  const double *root_logp;
  const int32_t *root_next;
  const sc_lm_slot *slots;
  int32_t V, order, n_states, n_slots, start_state, shift; /* shift = 64 - log2 n_slots */
} sc_lm_view;
typedef struct sc_lm sc_lm;
int sc_lm_create(const void *blob /*HOST*/, size_t bytes, sc_lm **out);
void sc_lm_destroy(sc_lm *lm);
/* *device: the view in device memory (what sc_ctc_beam_lm_job.lm takes); *host: a host copy of it.  Either may be NULL.
 * SC_ERR_ARG for a null model. */
int sc_lm_device_view(const sc_lm *lm, const sc_lm_view **device, sc_lm_view *host);

/* The beam search of sc_ctc_beam with the model fused in (tests/ctc_beam_lm_ref.py is the contract, built on
 * tests/ctc_beam_ref.py; nothing of that contract's row pass, candidates, stays, extensions or merges changes, pb / pnb
 * stay the pure CTC prefix probabilities).  Entry i carries besides them lm_i, the raw sum of the score() values along its
 * prefix, and ctx_i, the automaton's state after its prefix; the initial entry has (0.0, start_state), unused slots hold
 * (0.0, 0).  A new prefix made from entry i by candidate c gets (l, s') = score(ctx_i, c): lm = lm_i + l, ctx = s'.  A stay
 * keeps both; an extension that merges into an entry of the beam leaves that entry's alone (the same prefix has the same
 * values).  The B best are kept by fused = total + w, w = alpha * lm + beta * len, each product and each sum rounded on its
 * own (no fused multiply-add), ties as in sc_ctc_beam.  The candidates are still the C best by their fp32 acoustic values.
 * lm == NULL: the job runs unfused, lm_state / lm_state_after are neither read nor written; that, and alpha = beta = 0
 * with a model, give every bit of sc_ctc_beam on the same inputs.  Bars: every int32 and ctx equal wherever no cut between
 * fused totals is a near-tie, lm bit-equal, pb / pnb as for sc_ctc_beam. */
typedef struct sc_beam_lm_t {
  double lm[SC_BEAM_MAX];
  int32_t ctx[SC_BEAM_MAX];
} sc_beam_lm_t;
typedef struct sc_ctc_beam_lm_job {
  sc_ctc_beam_job beam;
  const sc_lm_view *lm;          /* device view; NULL: the job runs unfused */
  sc_beam_lm_t *lm_state;        /* beside beam.state: read (unless restart), written back (device) */
  sc_beam_lm_t *lm_state_after;  /* second copy, beside beam.state_after (NULL: none) */
  double alpha, beta;            /* weight of the model's log probability, bonus per token; finite */
} sc_ctc_beam_lm_job;
/* As sc_ctc_beam (same limits, same errors before a launch).  Malformed besides what is malformed there, and writing
 * nothing: with a model, a null lm_state, a model whose V differs from beam.V, an alpha or beta that is not finite, a stored
 * ctx outside [0, n_states) without restart. */
int sc_ctc_beam_lm(const sc_ctc_beam_lm_job *jobs, int n_jobs, void *stream);

/* ---- grammar-constrained CTC prefix beam (grammar_blob.h, ctc_beam_grammar.hip) ----------------------
 * "Answer only from this list": a grammar is a deterministic finite automaton over the token ids [0, V); the blank is
 * never a label.  State g has the out-arcs arc_tok / arc_next [arc_off[g], arc_off[g + 1]), strictly ascending by token,
 * and an accept flag; there is one start state.
 * The blob (little endian; speechcatcher_amd/grammar.py compiles it from phrases): sc_grammar_header; int32 arc_off
 * [n_states + 1]; int32 arc_tok[n_arcs]; int32 arc_next[n_arcs]; int32 accept[n_states] - every array padded to a
 * multiple of 8 bytes.  sc_grammar_create validates all of it on the host (the size against the header; V >= 1, blank in
 * [0, V), 1 <= n_states <= SC_GRAMMAR_MAX_STATES, 0 <= n_arcs <= SC_GRAMMAR_MAX_ARCS, reserved == 0; arc_off monotone from
 * 0 to n_arcs; the tokens of a state strictly ascending, in [0, V) and not the blank; every next and the start state in
 * [0, n_states); accept flags 0 or 1) BEFORE a byte reaches the device: SC_ERR_ARG and nothing allocated otherwise.  The
 * grammar is uploaded once and read-only afterwards; the handle keeps a host copy of the arrays.  It must outlive every
 * launch that reads it. */
#define SC_GRAMMAR_MAGIC 0x52474353 /* "SCGR" */
#define SC_GRAMMAR_VERSION 1
#define SC_GRAMMAR_MAX_STATES (1 << 20)
#define SC_GRAMMAR_MAX_ARCS (1 << 24)
typedef struct sc_grammar_header {
  int32_t magic, version, V, blank, n_states, n_arcs, start_state, reserved /* 0 */;
} sc_grammar_header;
typedef struct sc_grammar_view { /* the automaton as the kernel reads it (device pointers) */
  const int32_t *arc_off;  /* [n_states + 1] */
  const int32_t *arc_tok;  /* [n_arcs] */
  const int32_t *arc_next; /* [n_arcs] */
  const int32_t *accept;   /* [n_states] */
  int32_t V, blank, n_states, n_arcs, start_state, reserved;
} sc_grammar_view;
typedef struct sc_grammar sc_grammar;
int sc_grammar_create(const void *blob /*HOST*/, size_t bytes, sc_grammar **out);
/* SC_ERR_ARG (and nothing freed) while the grammar's use count is not 0; a null grammar is SC_OK. */
int sc_grammar_destroy(sc_grammar *g);
/* *device: the view in device memory (what sc_ctc_beam_gr_job.grammar takes); *host: a host copy of it (device pointers).
 * Either may be NULL.  SC_ERR_ARG for a null grammar. */
int sc_grammar_device_view(const sc_grammar *g, const sc_grammar_view **device, sc_grammar_view *host);
/* The use count destroy looks at: whoever names the grammar beyond a launch takes a use (+1) and drops it (-1).  Returns
 * the new count; SC_ERR_ARG for a null grammar or a count that would fall below 0. */
int sc_grammar_use(sc_grammar *g, int delta);
/* the handle's host copy: next state of (state, token) or -1 (no such arc, or an argument out of range) / the accept
 * flag (0 or 1; -1 for a state out of range).  Host arithmetic, no launch. */
int sc_grammar_step(const sc_grammar *g, int state, int token);
int sc_grammar_accepts(const sc_grammar *g, int state);

/* The beam search of sc_ctc_beam with the grammar choosing the candidates (tests/ctc_beam_grammar_ref.py is the
 * contract, built on tests/ctc_beam_ref.py).  Unchanged from sc_ctc_beam: the row rule (bad rows, lse, lp), lae, the merge
 * rule, the prune order and its ties, the node records, chained spans.  Entry i carries besides them g_i, the automaton's
 * state after its prefix; the initial entry has start_state, unused slots hold 0.  Three things differ:
 *   candidates   are per entry: the C out-arc tokens of g_i with the largest x, compared as fp32, the lowest token among
 *                ties, none at -inf; fewer than C when the state has fewer arcs - a state without arcs only stays.  Two
 *                entries in one state have the same candidates.
 *   stay         the repeat term is unconditional: pnb'_i = pnb_i + lp(last_i), lp(v) = (double)x[v] - lse for any v
 *                (-inf when x[last_i] is -inf or the entry is the empty prefix).  (With per-entry candidates the rule of
 *                sc_ctc_beam would end every accepted phrase: its last token is seldom an out-arc of the state it led to.)
 *   extension    a new prefix made from entry i by c gets g = next(g_i, c); a stay keeps g; an extension that merges
 *                leaves the target's g alone (the automaton is deterministic: the same prefix has the same state).
 * The free grammar (one state, a self-loop on every non-blank token) with V - 1 <= C gives every byte of sc_ctc_beam on
 * the same inputs.  Bars: every int32 and g equal wherever no prune decision is a near-tie, pb / pnb as for sc_ctc_beam.
 * Not in this revision: weighted arcs, a grammar together with an n-gram model. */
typedef struct sc_beam_gr_t {
  int32_t g[SC_BEAM_MAX];
} sc_beam_gr_t;
typedef struct sc_ctc_beam_gr_job {
  sc_ctc_beam_job beam;
  const sc_grammar_view *grammar; /* device view */
  sc_beam_gr_t *gr_state;         /* beside beam.state: read (unless restart), written back (device) */
  sc_beam_gr_t *gr_state_after;   /* second copy, beside beam.state_after (NULL: none) */
} sc_ctc_beam_gr_job;
/* As sc_ctc_beam (ONE launch, one workgroup per job, same limits, same errors before a launch; no atomics, one writer
 * per output, the table and the grammar only read).  Malformed besides what is malformed there, and writing nothing: a
 * null grammar or gr_state, a grammar whose V or blank differs from the job's, a stored g outside [0, n_states) without
 * restart. */
int sc_ctc_beam_grammar(const sc_ctc_beam_gr_job *jobs, int n_jobs, void *stream);

/* ---- n-gram rescoring of n-best lists, with an </s> term (lm_rescore.hip, lm_score.h) ---------------
 * A job is one list: n_hyp <= SC_RESCORE_MAX_HYPS rows of token ids, row h at yseq + h * row_stride with lens[h] tokens
 * (lens == NULL: L tokens each; a lens[h] outside [0, L] makes the row a bad one, below), their totals at
 * score[h * score_stride].  The LABELS of a row are its tokens without the first `skip` (1 for <sos>) and without ONE
 * trailing token equal to `strip` (-1: none is dropped; as sc_align_hyps drops a trailing <eos>): y_0 .. y_{m-1}.  With
 * score() of the model above:
 *   s_0 = state0 (-1: the model's start_state);  (l_t, s_{t+1}) = score(s_t, y_t);  tok_lm[h * tok_stride + t] = l_t
 *   lm[h]        ((0.0 + l_0) + l_1) + ..., ascending t - what an entry of sc_ctc_beam_lm carries for the same prefix
 *   end_state[h] s_m
 *   eos_lm[h]    score(s_m, lm_eos) when lm_eos >= 0 (the id that stands for </s> in the model), else 0.0
 *   fused[h]     score[h] + (alpha * (lm[h] + eos_lm[h]) + beta * m), every product and sum rounded on its own; a NaN is
 *                stored as the quiet NaN 0x7FF8000000000000
 *   order[r]     the row at rank r: fused descending, ties to the lower row
 * status[h]: SC_RESCORE_NONFINITE when score[h] or fused[h] is not finite; SC_RESCORE_BAD_TOKEN for a label outside
 * [0, V) (or a bad lens[h]): lm = eos_lm = 0.0, every tok_lm of the row 0.0, end_state -1, fused NaN.  Rows of both kinds
 * rank behind all others, in row order among themselves.  SC_RESCORE_SERIAL: the row was walked label by label by one
 * lane and not by the speculate-and-verify form (a row on which a guessed state did not hold, or every row of a job with
 * SC_RESCORE_FORCE_SERIAL) - both forms give the same bits.  tests/lm_rescore_ref.py is the contract: every output bit
 * for bit. */
#define SC_RESCORE_MAX_HYPS 16
#define SC_RESCORE_FORCE_SERIAL 1 /* flags */
#define SC_RESCORE_NONFINITE 1    /* status bits */
#define SC_RESCORE_BAD_TOKEN 2
#define SC_RESCORE_SERIAL 4
typedef struct sc_lm_rescore_job {
  const sc_lm_view *model;  /* device view (sc_lm_device_view) */
  const int32_t *yseq;      /* row h at yseq + h * row_stride (device) */
  const double *score;      /* total of row h at score[h * score_stride] (device) */
  const int32_t *lens;      /* [n_hyp] tokens per row, or NULL: L each (device) */
  double *lm;               /* [n_hyp] (device) */
  double *eos_lm;           /* [n_hyp] (device) */
  double *fused;            /* [n_hyp] (device) */
  int32_t *end_state;       /* [n_hyp] (device) */
  int32_t *order;           /* [n_hyp] (device) */
  int32_t *status;          /* [n_hyp] SC_RESCORE_* (device) */
  double *tok_lm;           /* row h at tok_lm + h * tok_stride, m values; NULL: not wanted (device) */
  int64_t row_stride;       /* int32 elements between two rows, >= L */
  int64_t score_stride;     /* doubles between two rows' scores, >= 1 */
  int64_t tok_stride;       /* doubles between two rows of tok_lm, >= max(0, L - skip) when tok_lm is given */
  double alpha, beta;       /* weight of the model's log probability, bonus per label; finite */
  int32_t n_hyp, L, skip, strip, state0, lm_eos, V, flags;
} sc_lm_rescore_job;
#define SC_RESCORE_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job: no atomics, one writer per
 * output, plain stores; the model, the rows and the scores are only read, nothing outside the sizes above is written.
 * SC_ERR_ARG before anything is launched for n_jobs outside [0, SC_RESCORE_MAX_JOBS] or a null table with n_jobs > 0.  A
 * job whose own fields are malformed (a null pointer other than lens / tok_lm, n_hyp outside [1, SC_RESCORE_MAX_HYPS],
 * L < 0, row_stride < L, score_stride < 1, tok_stride < max(0, L - skip) with tok_lm, skip < 0, strip < -1, a model whose
 * V differs from the job's, state0 outside [-1, n_states), lm_eos outside [-1, V), an alpha or beta that is not finite,
 * unknown flags) writes nothing.  Two jobs of one call must not share outputs. */
int sc_lm_rescore(const sc_lm_rescore_job *jobs, int n_jobs, void *stream);

/* ---- consensus of n-best lists: minimum-Bayes-risk row and slot confidences (mbr.hip) ----------------
 * A job is one list in sc_lm_rescore_job's layout: n_hyp <= SC_MBR_MAX_HYPS rows, row h at yseq + h * row_stride with
 * lens[h] tokens (lens == NULL: L each), its LABELS y_h[0 .. m_h) the tokens without the first `skip` and without ONE
 * trailing token equal to `strip` (-1: none).  Per row EITHER weight[h] (score == NULL) OR score[h * score_stride]
 * (weight == NULL).
 *   status[h]     SC_MBR_BAD_TOKEN: a label outside [0, V) or a lens[h] outside [0, L].  SC_MBR_TOO_LONG: m_h >
 *                 SC_MBR_MAX_LEN.  SC_MBR_NONFINITE: a weight that is NaN, infinite or negative; a score that is NaN or
 *                 +inf, or whose z_h (below) is (-inf is a legal score: weight 0).  A row with any of these is OUT: -1 in
 *                 its row and column of dist, risk the quiet NaN 0x7FF8000000000000, weight 0.0; it ranks behind all
 *                 others, in row order.  SC_MBR_NO_PIVOT: on every row of a list without a pivot (below).
 *   weight_out[h] w_h.  With `weight`: the value itself.  With `score`, over the rows that are in: z_h = scale * score[h]
 *                 (-inf for a score of -inf whatever the scale), M = max z, e_h = exp(z_h - M), Z = ((0 + e_0) + e_1) +
 *                 ... ascending, w_h = e_h / Z; when every z is -inf, w_h = 1 / n_in.
 *   dist[h][j]    [16][16] row-major: Levenshtein distance of y_h and y_j, unit costs; entries of rows or columns at or
 *                 beyond n_hyp are not written
 *   risk[h]       ((0.0 + w_0 dist[h][0]) + w_1 dist[h][1]) + ..., ascending j over the rows that are in, every product and
 *                 sum rounded on its own
 *   order[r]      the row at rank r: risk ascending, ties to the lower row, rows that are out last
 *   header        {P, m_P, n_in, 0}: the pivot P = order[0] when the job's pivot is -1, else the named row; P = -1 and
 *                 m_P = 0 when no row is in or the named row is out
 *   slots[j * slot_stride + t], t in [0, m_P) (wanted only with a non-null pointer): row j, when it is in, aligned
 *                 against the pivot.  D is the full table of (y_P, y_j); from (m_P, m_j): DIAGONAL if i > 0, j > 0 and
 *                 D[i][j] == D[i-1][j-1] + (y_P[i-1] != y_j[j-1]) - slot i-1 gets y_j[j-1]; otherwise UP if i > 0 and
 *                 D[i][j] == D[i-1][j] + 1 - slot i-1 gets -1 (epsilon); otherwise LEFT - row j has an insertion in gap
 *                 i (before the pivot's position i; gap m_P is the end).  A row that is out has -2 in every slot.
 *   conf[t]       t in [0, m_P): the sum over j ascending (rows in) of w_j where slot t of row j equals y_P[t]
 *   alt_tok[t], alt_mass[t]  among the symbols other than y_P[t] in column t (a token id or -1) the one with the largest
 *                 mass (the same kind of sum), ties to the lower symbol; -2 and 0.0 when there is none
 *   gap_mass[g]   g in [0, m_P] (nothing without a pivot): the mass of the rows with at least one insertion in gap g
 * tests/mbr_ref.py is the contract.  With `weight` every output is the contract's bit for bit; with `score` the
 * library's exp() stands in for the host's, and the doubles agree within 64 ulp of max(1, |value|). */
#define SC_MBR_MAX_HYPS 16
#define SC_MBR_MAX_LEN 1024 /* labels per row; a longer row is SC_MBR_TOO_LONG */
#define SC_MBR_NONFINITE 1  /* status bits */
#define SC_MBR_BAD_TOKEN 2
#define SC_MBR_TOO_LONG 4
#define SC_MBR_NO_PIVOT 8
typedef struct sc_mbr_job {
  const int32_t *yseq;   /* row h at yseq + h * row_stride (device) */
  const double *score;   /* total of row h at score[h * score_stride], or NULL (device) */
  const double *weight;  /* [n_hyp] weights, or NULL; exactly one of score and weight is given (device) */
  const int32_t *lens;   /* [n_hyp] tokens per row, or NULL: L each (device) */
  double *weight_out;    /* [n_hyp] (device) */
  double *risk;          /* [n_hyp] (device) */
  int32_t *dist;         /* [16][16] (device) */
  int32_t *order;        /* [n_hyp] (device) */
  int32_t *status;       /* [n_hyp] SC_MBR_* (device) */
  int32_t *header;       /* [4] (device) */
  double *conf;          /* [m_P]; room for min(max(0, L - skip), SC_MBR_MAX_LEN) values (device) */
  double *alt_mass;      /* as conf (device) */
  double *gap_mass;      /* [m_P + 1]; room for one value more than conf (device) */
  int32_t *alt_tok;      /* as conf (device) */
  int32_t *slots;        /* row j at slots + j * slot_stride, m_P values; NULL: not wanted (device) */
  int64_t row_stride;    /* int32 elements between two rows, >= L */
  int64_t score_stride;  /* doubles between two rows' scores, >= 1 when score is given */
  int64_t slot_stride;   /* int32 elements between two rows of slots, >= min(max(0, L - skip), SC_MBR_MAX_LEN) with slots */
  double scale;          /* of the scores; finite, >= 0 */
  int32_t n_hyp, L, skip, strip, V, pivot, flags, reserved;   /* pivot: -1 the minimum-risk row, else the row; flags: 0 */
} sc_mbr_job;
#define SC_MBR_MAX_JOBS 65535
/* Bytes of workspace (direction bits of the backtraces, slots, gap marks) for n_jobs lists of at most max_len labels a
 * row; 0 for arguments out of range. */
size_t sc_mbr_ws_bytes(int n_jobs, int max_len);
/* jobs: device table of n_jobs entries; ws: device workspace of ws_bytes, of which every job gets an equal share.
 * THREE launches on `stream`, no host synchronisation between them: validation, weights and the pair distances (one
 * wave per job and one per pair); risk, order and pivot (one workgroup per job); the backtraces against the pivot (one
 * wave per row) and the column pass.  No atomics, one writer per output, plain stores; the inputs are only read.
 * SC_ERR_ARG before anything is launched for n_jobs outside [0, SC_MBR_MAX_JOBS], a null table or a null workspace with
 * n_jobs > 0.  A job whose own fields are malformed (a null pointer other than lens / slots, both or neither of score
 * and weight, n_hyp outside [1, SC_MBR_MAX_HYPS], L < 0, row_stride < L, score_stride < 1 with score, a slot_stride too
 * small with slots, skip < 0, strip < -1, V < 1, a scale that is not finite or negative, pivot outside [-1, n_hyp),
 * flags or reserved other than 0, a share of the workspace below what sc_mbr_ws_bytes gives for one list of the job's
 * max(0, L - skip) labels) writes nothing.  Two jobs of one call must not share outputs. */
int sc_mbr(const sc_mbr_job *jobs, int n_jobs, void *ws, size_t ws_bytes, void *stream);

/* ---- attention rescoring of n-best lists (dec_rescore.hip) --------------------------------------------
 * Attention of whole sequences (sc_seq_attention).  A job is ONE sequence: Lq query rows against Lk key / value rows, H
 * heads of dk columns each (head h at columns [h * dk, (h + 1) * dk) of a row of q, k, v and o), every buffer with its
 * own row stride:
 *   s_ij = q_i . k_j / sqrt(dk);   key j is MASKED when j >= Lk, or when the job is causal and j > i
 *   o_i  = sum_j softmax_j(s_i)_j v_j over the keys that are not masked
 * fp32 throughout, both products on the matrix cores (v_mfma_f32_16x16x4_f32), keys walked in tiles of 16 from key 0
 * with an online softmax.  A mask is a select: a masked key has weight exactly 0 and neither its k nor its v row reaches
 * an output - rows at or beyond Lk are never read, the rows j > i of a causal job are read (a later query needs them)
 * but their products are discarded by selects.  The bits of o_i depend on q_i and on the rows k_j, v_j the mask leaves
 * to it alone - not on Lq, on the other jobs of the launch or on the workgroup it lands in.  One workgroup of one wave
 * per (job, head, tile of 16 queries); no atomics, one writer per output, plain stores; nothing outside
 * [0, Lq) x [0, H * dk) of o is written, nothing outside the stated sizes is read. */
typedef struct sc_seq_attn_job {
  const float *q, *k, *v;  /* row i at q + i * q_stride, ... (device; 16-byte aligned) */
  float *o;                /* row i at o + i * o_stride (device) */
  int64_t q_stride, k_stride, v_stride, o_stride; /* floats between two rows, multiples of 4, >= H * dk */
  int32_t Lq, Lk;          /* Lq == 0: nothing to do; else Lk >= 1 */
  int32_t H, causal;       /* causal: 0 or 1 */
} sc_seq_attn_job;
#define SC_SEQ_ATTN_MAX_JOBS (1 << 24)
/* jobs: device table of n_jobs entries.  dk: 16, 32 or 64.  max_Lq, max_H: the launch covers query rows below max_Lq and
 * heads below max_H of every job (a job with more is malformed).  forms: bit 0 - the table holds jobs that are not
 * causal, bit 1 - it holds causal jobs (one launch per set bit; a job of a form whose bit is not set is skipped).
 * SC_ERR_ARG before anything is launched for a bad count, dk, max_Lq, max_H or forms; a job whose own fields are
 * malformed (a null or misaligned pointer, a bad stride, Lq < 0, Lq > max_Lq, H outside [1, max_H], Lk < 1 with Lq > 0,
 * causal outside {0, 1}) writes nothing. */
int sc_seq_attention(const sc_seq_attn_job *jobs, int n_jobs, int dk, int max_Lq, int max_H, int forms, void *stream);

/* One teacher-forced pass of the attention decoder over n-best lists (sc_dec_rescore).  A job is one list: n_hyp <=
 * SC_ATT_MAX_HYPS rows of labels (no <sos>, no <eos>), row h at yseq + h * row_stride with m_h = lens[h] labels (lens ==
 * NULL: L each), their first-pass totals at score[h * score_stride], and the T encoder rows E (row t at E + t * e_stride,
 * d floats) the list was decoded from.  Row h is scored as the decoder scores it without a cache (decoder_layer.py:60-132,
 * transformer_decoder.py): inputs [sos, y_0 .. y_{m-1}] at positions 0 .. m, targets [y_0 .. y_{m-1}, eos];
 *   tok_att[h * tok_stride + t]  log-probability of target t, t in [0, m_h] (the last is the <eos> term); float64 =
 *                (double)logit[target] - lse, lse of the fp32 logits row in float64 (csrc/ctc_row.h)
 *   att[h]       ((0.0 + tok_att[0]) + tok_att[1]) + ..., ascending t
 *   fused[h]     (w_ctc * score[h] + w_att * att[h]) + beta * m_h, every product and sum rounded on its own; a NaN is
 *                stored as the quiet NaN 0x7FF8000000000000
 *   order[r]     the row at rank r: fused descending, ties to the lower row
 * status[h], a set of bits: SC_ATT_BAD_TOKEN - lens[h] outside [0, L] (nothing else of the row is examined) or a label
 * outside [0, V); SC_ATT_TOO_LONG - m_h + 1 exceeds pe_rows or the model's LCAP; SC_ATT_NO_FRAMES - T == 0 (every row of
 * the job).  A row with one of these has att = 0.0, fused = NaN and all L + 1 entries of its tok_att row 0.0.
 * SC_ATT_NONFINITE - score[h] is not finite, or the fused total of a row without the bits above is not.  Rows with any
 * status rank behind all others, in row order among themselves.  A label equal to sos / eos is an ordinary label.
 * tests/dec_rescore_ref.py is the contract (float64): integers equal, att within the fp32 decoder's error.
 * fp32 weights only: the model's sc_dec_layer entries wqkv, wo, wq, wo2, w1, w2 (w1_p / w2_p where sc_ffn_ln_supported)
 * with their biases and norms, embed, pe, the after-norm and out_w / out_b; of sc_search nothing else but V, d, H, F,
 * n_layers, LCAP, sos, eos and ln_eps is read.  sc_dec_layer carries no cross-attention K|V weights (the stream engine
 * projects K|V where the encoder runs), so a job names them: wkv [n_layers * 2d][d] and bkv [n_layers * 2d], the
 * layers' linear_k | linear_v one behind the other - the same for every job of a call. */
#define SC_ATT_MAX_HYPS 16
#define SC_ATT_NONFINITE 1 /* status bits */
#define SC_ATT_BAD_TOKEN 2
#define SC_ATT_TOO_LONG 4
#define SC_ATT_NO_FRAMES 8
#define SC_ERR_UNSUPPORTED (-5) /* sc_dec_rescore: the fp32 decoder weights are not resident in this handle */
typedef struct sc_dec_rescore_job {
  const float *E;           /* encoder rows (device); may be NULL when T == 0 */
  const int32_t *yseq;      /* row h at yseq + h * row_stride (device) */
  const double *score;      /* total of row h at score[h * score_stride] (device) */
  const int32_t *lens;      /* [n_hyp] labels per row, or NULL: L each (device) */
  const float *wkv, *bkv;   /* cross-attention K|V weights and biases of all layers (device) */
  double *att;              /* [n_hyp] (device) */
  double *fused;            /* [n_hyp] (device) */
  int32_t *order;           /* [n_hyp] (device) */
  int32_t *status;          /* [n_hyp] SC_ATT_* (device) */
  double *tok_att;          /* row h at tok_att + h * tok_stride, m_h + 1 values; NULL: not wanted (device) */
  int64_t e_stride;         /* floats between two rows of E, a multiple of 4, >= d */
  int64_t row_stride;       /* int32 elements between two rows, >= L */
  int64_t score_stride;     /* doubles between two rows' scores, >= 1 */
  int64_t tok_stride;       /* doubles between two rows of tok_att, >= L + 1 when tok_att is given */
  double w_att, w_ctc, beta; /* finite */
  int32_t n_hyp, L, T, pe_rows; /* pe_rows: rows of the model's position table */
} sc_dec_rescore_job;
#define SC_ATT_MAX_JOBS 65535
/* bytes of workspace a call (or one slab of a call) needs for lists of `rows` = sum n_hyp * (L + 1) token rows, `enc_rows`
 * = sum T encoder rows, `n_seqs` = sum n_hyp and n_jobs jobs; 0 for a model the call refuses */
size_t sc_dec_rescore_ws_bytes(const sc_search *model /*HOST*/, long rows, long enc_rows, int n_seqs, int n_jobs);
/* jobs: HOST table.  Launches on `stream`: the dense work through sc_gemm / sc_gemm_ln / sc_gemm_colblocks / sc_ffn_ln
 * (the feed-forward takes sc_ffn_ln where sc_ffn_ln_supported and the stream has its split-K workspace, else two sc_gemm)
 * over the packed row table of all lists - their canonical sums keep a row's bits independent of the row count -, the
 * two attentions of a layer through sc_seq_attention.  ws: device memory of ws_bytes, 256-byte aligned; a call whose
 * lists need more is processed in slabs of whole jobs, with the same bits; SC_ERR_CAPACITY when one job alone does not
 * fit.  Every error is raised before anything is launched or written: SC_ERR_ARG for a bad count, a null table, a
 * model whose dims the kernels do not cover (d % 32, head dim not 16 / 32 / 64, V > SC_MAX_VOCAB) and for a malformed job
 * (a null pointer other than lens / tok_att / E with T == 0, n_hyp outside [1, SC_ATT_MAX_HYPS], L outside [0, 65535), T outside [0, 65535], pe_rows < 1,
 * a stride below its size, a misaligned E, a weight that is not finite, wkv / bkv differing between jobs);
 * SC_ERR_UNSUPPORTED when a fp32 weight of the model is missing.  Two jobs of one call must not share outputs. */
int sc_dec_rescore(const sc_dec_rescore_job *jobs /*HOST*/, int n_jobs, const sc_search *model /*HOST*/, void *ws,
                   size_t ws_bytes, void *stream);

/* ---- CTC token alternates (alternates.hip) -----------------------------------------------------
 * "What else could this token have been": for each of L token spans [start[k], end[k]) over the T rows of an fp32 CTC
 * table, the K acoustically best tokens of those frames and the rank of the span's own label y[k] among them.  Per span,
 * checked in this order: SC_ALT_NO_SPAN when start < 0, end <= start or end > T (no row is read); SC_ALT_BAD_ROW when a
 * row OF THE SPAN is bad (a NaN, a +inf, or nothing but -inf); else SC_ALT_OK with
 *   S[v] = ((x[start][v] + x[start+1][v]) + ...), promoted to float64 and added in ascending frame order (-inf stays -inf)
 *   candidates: every v in [0, V) but the blank, ordered by S descending, then v ascending
 *   alt_ids[k][j] = the j-th candidate for j < min(K, V - 1), -1 behind them
 *   alt_logp[k][j] = (S[v] - sum_t lse_t) / (end - start), lse_t = m + log(sum_v exp(x[v] - m)) as for sc_ctc_activity,
 *                    summed in frame order; -inf in the unused slots
 *   own_rank[k] = the candidates strictly ahead of y[k] in that order (0: the token is the acoustic best of its own
 *                 frames); -1 when y[k] is outside [0, V) or the blank (the rest of the span is still computed)
 * A status other than SC_ALT_OK: ids -1, logp -inf, own_rank -1.  A per-row constant cancels inside a span: raw logits
 * and log-softmaxed rows give the same order unless fp32 rounding creates a tie.  tests/ctc_alt_ref.py is the contract:
 * every int32 equal (S holds only float64 adds of promoted fp32 values: the same bits), alt_logp within 1e-11. */
#define SC_ALT_OK 0
#define SC_ALT_NO_SPAN 1
#define SC_ALT_BAD_ROW 2
#define SC_ALT_MAX_K 8
typedef struct sc_ctc_alt_job {
  const float *emis;       /* row t of the table at emis + t * stride, V floats (device) */
  const int32_t *labels;   /* [L] (device) */
  const int32_t *start;    /* [L] first frame of each span (device) */
  const int32_t *end;      /* [L] one past its last frame (device) */
  int32_t *alt_ids;        /* [L][K] (device) */
  double *alt_logp;        /* [L][K] (device) */
  int32_t *own_rank;       /* [L] (device) */
  int32_t *status;         /* [L] SC_ALT_* (device) */
  int64_t stride;          /* floats between two rows, >= V */
  int32_t T, V, blank, L;
} sc_ctc_alt_job;
#define SC_ALT_MAX_JOBS 65535
/* jobs: device table of n_jobs entries; max_L bounds their L (max_L <= SC_ALIGN_MAX_L), 1 <= K <= SC_ALT_MAX_K.  ONE
 * launch on `stream`, one workgroup per (job, span): float64 sums in one fixed order, no atomics, one writer per output;
 * nothing past a job's L is written.  SC_ERR_ARG before anything is launched for n_jobs outside [0, SC_ALT_MAX_JOBS], a
 * null table with n_jobs > 0, max_L outside [0, SC_ALIGN_MAX_L], K outside [1, SC_ALT_MAX_K].  A job whose own fields
 * are malformed (a null pointer with L > 0, V outside [1, SC_MAX_VOCAB], blank outside [0, V), T < 0, L outside
 * [0, max_L], stride < V) writes nothing.  Two jobs of one call must not share outputs.  The table, labels and spans are
 * only read. */
int sc_ctc_alternates(const sc_ctc_alt_job *jobs, int n_jobs, int max_L, int K, void *stream);

/* ---- stable partials: committed prefix and token stability of a beam (commit.hip) -----------------
 * A job is the live beam of one stream: n_hyp <= SC_COMMIT_MAX_HYPS hypotheses of one length L, best first, row h at
 * yseq + h * row_stride (only [0, L) of a row is read), their total scores at score[h * score_stride].  Every
 * hypothesis of a later reply descends from one of them, so what all of them share cannot change any more:
 *   agree[h]      length of the common prefix of row h and row 0 (agree[0] = L)
 *   commit        min_h agree[h]; L with SC_COMMIT_FINAL in flags
 *   w[h]          exp(score[h] - the largest finite score); a NaN or an infinity: 0 and SC_COMMIT_NONFINITE in status;
 *                 no finite score at all: every w = 1
 *   Z             ((w[0] + w[1]) + ...), ascending h
 *   stability[i - from], from <= i < L: (the sum, ascending h, of the w[h] with agree[h] > i) / Z - the share of the
 *                 beam's mass that agrees with row 0 up to and including token i; 1.0 with SC_COMMIT_FINAL
 *   ids / pos     yseq[0][from .. L), xpos[0][from .. L); totals: score / score_dec / score_ctc of row 0
 * stability is exactly 1.0 below commit (the same sum as Z) and never rises with i.  tests/hyp_commit_ref.py is the
 * contract: every int32 equal, stability within 1e-12. */
#define SC_COMMIT_MAX_HYPS 16
#define SC_COMMIT_FINAL 1      /* flags */
#define SC_COMMIT_NONFINITE 1  /* status */
typedef struct sc_hyp_commit_job {
  const int32_t *yseq;      /* row h at yseq + h * row_stride, L ids (device) */
  const int32_t *xpos;      /* the same layout */
  const double *score;      /* total of row h at score[h * score_stride] (device) */
  const double *score_dec;  /* the same layout; only row 0's is read */
  const double *score_ctc;
  int32_t *header;          /* [4] L, commit, n_hyp, status (device) */
  int32_t *agree;           /* [n_hyp] (device) */
  int32_t *ids;             /* [L - from] (device) */
  int32_t *pos;             /* [L - from] (device) */
  double *stability;        /* [L - from] (device) */
  double *totals;           /* [3] (device) */
  int64_t row_stride;       /* int32 elements between two rows, >= L */
  int64_t score_stride;     /* doubles between two rows' scores: 1 for separate arrays, 3 for {total, dec, ctc} triples */
  int32_t n_hyp, L, from, flags;
} sc_hyp_commit_job;
#define SC_COMMIT_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup per job: no atomics, one writer per
 * output, float64 sums in ascending h; nothing outside the sizes above is written.  SC_ERR_ARG before anything is
 * launched for n_jobs outside [0, SC_COMMIT_MAX_JOBS] or a null table with n_jobs > 0.  A job whose own fields are
 * malformed (a null pointer, n_hyp outside [1, SC_COMMIT_MAX_HYPS], L < 0, from outside [0, L], row_stride < L,
 * score_stride < 1) writes nothing.  Two jobs of one call must not share outputs.  The rows and scores are only read. */
int sc_hyp_commit(const sc_hyp_commit_job *jobs, int n_jobs, void *stream);

/* ---- wire-format audio in (pcm.hip) -----------------------------------------------------------
 * A chunk is n sample FRAMES of `channels` interleaved little-endian codes, starting at ANY byte address.  Every format
 * but SC_PCM_F32 gives an integer v per code with full scale 2^B:
 *   SC_PCM_S16LE  the int16, B = 15;   SC_PCM_S24LE  3 packed bytes, sign-extended, B = 23;   SC_PCM_U8  b - 128, B = 7
 *   SC_PCM_MULAW  u = ~b & 0xFF; mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84; v = u & 0x80 ? -mag : mag, B = 15
 *   SC_PCM_ALAW   a = b ^ 0x55; e = (a >> 4) & 7; mag = e ? (((a & 15) << 4) + 0x108) << (e - 1) : ((a & 15) << 4) + 8;
 *                 v = a & 0x80 ? mag : -mag, B = 15            (G.711: Python 3.10 audioop.ulaw2lin / alaw2lin)
 * channel in [0, channels): m = v[channel], C = 1;  channel == SC_PCM_MIX: m = the exact integer sum over the channels,
 * C = channels.  x = RN_fp32(m / C), the exact quotient rounded ONCE (m is never rounded to fp32 first).  The sample is
 * x * 2^-B (SC_PCM_SCALE_FULL, exact) or fp32(RN_half(x)) * 2^-15 (SC_PCM_SCALE_SERVER, B = 15 formats only: the
 * reference server's float16 conversion, speechcatcher_server.py).  SC_PCM_F32: a selected channel passes its bits
 * through, NaNs included; a mix is RN_fp32(s / C), s the fp32 sum of the channels in ascending order with every add
 * rounded, and the canonical quiet NaN 0x7fc00000 when that is a NaN; SC_PCM_SCALE_FULL only.
 * The LEVEL of the integer formats, cumulative over an utterance and exact in any order: frames += n,
 * peak = max(peak, |m|), sum_abs += |m|, clipped += frames in which a contributing channel's v sits at its format's
 * extreme (s16 -32768 / 32767, s24 -2^23 / 2^23 - 1, u8 -128 / 127, mu-law |v| = 32124, A-law |v| = 32256),
 * full_scale = C 2^B.  SC_PCM_F32 leaves the counts as they are and sets full_scale = 0.
 * tests/pcm_ref.py is the contract; the kernel reproduces it bit for bit. */
#define SC_PCM_F32 0
#define SC_PCM_S16LE 1
#define SC_PCM_S24LE 2
#define SC_PCM_U8 3
#define SC_PCM_MULAW 4
#define SC_PCM_ALAW 5
#define SC_PCM_N_FORMATS 6
#define SC_PCM_MIX (-1)
#define SC_PCM_MAX_CHANNELS 8
#define SC_PCM_SCALE_FULL 0
#define SC_PCM_SCALE_SERVER 1
typedef struct sc_input_level_t {
  int64_t frames, clipped, sum_abs;
  int32_t peak, full_scale;
} sc_input_level_t;
typedef struct sc_pcm_job {
  const void *src;               /* the coded bytes (device); the chunk starts at src + offset, any alignment */
  float *dst;                    /* [n] decoded samples (device) */
  sc_input_level_t *level;       /* read (unless restart), advanced over the chunk, written back (device) */
  sc_input_level_t *level_after; /* second copy of the new level, e.g. in host-mapped memory (NULL: none) */
  int64_t offset;                /* bytes, >= 0 */
  int32_t format, channels, channel, scale;
  int32_t n;                     /* sample frames, >= 0 */
  int32_t restart;               /* != 0: the stored level is ignored, the chunk starts an utterance (all zero) */
} sc_pcm_job;
#define SC_PCM_MAX_JOBS 65535
/* jobs: device table of n_jobs entries.  ONE launch on `stream`, one workgroup of 256 threads per job; no atomics, one
 * writer per output, nothing is written behind dst + n; n == 0 rewrites the level unchanged.  n_jobs < 0, a null table
 * with n_jobs > 0 or n_jobs > SC_PCM_MAX_JOBS: SC_ERR_ARG before anything is launched.  A job whose own fields are
 * malformed (a null pointer other than level_after, a format outside [0, SC_PCM_N_FORMATS), channels outside [1, 8],
 * channel outside [-1, channels), a scale the format does not take, offset < 0, n < 0) writes nothing.  Two jobs of one
 * call must not share a level or overlap in dst. */
int sc_pcm_decode(const sc_pcm_job *jobs, int n_jobs, void *stream);
/* bytes of one sample frame (pure host); SC_ERR_ARG (< 0) for a format or a channel count out of range */
int sc_pcm_bytes_per_frame(int format, int channels);

/* ---- frontend ------------------------------------------------------------ */

/* STFTFrontend.forward (model/frontend/stft_frontend.py:87-154) fused with the
 * global MVN and frame trimming of Speech2TextStreaming.apply_frontend
 * (speech2text_streaming.py:355-389).  jobs[j] = {stream, seg_start, seg_len,
 * eff_len, keep_lo, keep_n, dst_row0, 0}.  mvn_mode: 0 none, 1 fp32, 2 fp64. */
int sc_logmel(const float *pcm, int pcm_stride, const int32_t *jobs, int n_jobs, int max_keep,
              const float *window, const float *mel_fb, const float *twiddle, const double *mean,
              const double *stdv, int mvn_mode, int n_fft, int hop, int win, int n_mels,
              float *feat, void *stream);

/* ---- sample-rate conversion to 16 kHz (resample.hip) --------------------------------------
 * The reference takes 16 kHz PCM from one ffmpeg pipe per session (speechcatcher.py:574-592, speechcatcher_server.py);
 * here the conversion is a rational polyphase FIR on the GPU, in the staging step of the stream engine:
 *   g = gcd(rate, 16000), L = 16000 / g, M = rate / g;  fc = 0.94 min(1, L / M), W = 24 / fc, Wc = ceil(W), K = 2 Wc
 *   h(x) = fc sinc(fc x) I0(10 sqrt(1 - (x / W)^2)) / I0(10) for |x| <= W, else 0     (Kaiser window, beta 10)
 *   coef[p][k] = h((k - Wc + 1) - p / L), each phase row divided by its float64 sum (DC gain 1), rounded to f32
 *   y[m] = sum_k coef[p][k] x[n0 - Wc + 1 + k],  n0 = (m M) div L, p = (m M) mod L,  x = 0 before the start and, once
 *   the final call has been made, behind the end
 * in fp32 and ONE order: four partial sums over k = 0, 1, 2, 3 (mod 4), each in ascending k, every product rounded
 * before it is added (no fma), combined as (s0 + s1) + (s2 + s3).  Output m is a function of m and the signal alone:
 * how the audio was cut into calls does not enter.  Supported: every rate in [8000, 48000] with L <= 640 (8000, 11025,
 * 12000, 16000, 22050, 24000, 32000, 44100, 48000 among them); the look-ahead is Wc input samples (<= 1.6 ms).
 * After N input samples a stream has produced max(0, ceil((N - Wc) L / M)) outputs, ceil(N L / M) once it is final. */
/* design the library uses for `rate`: L, M, half width Wc, and (coef != NULL) the [L][2*Wc] f32 table.  Pure host;
 * any of the outputs may be NULL.  SC_ERR_ARG for an unsupported rate. */
int sc_resample_design(int rate, int *L, int *M, int *half_width, float *coef);
/* outputs produced after n_in_total input samples (final: after the flush).  Pure host; SC_ERR_ARG (< 0) for an
 * unsupported rate. */
long sc_resample_out_count(int rate, long n_in_total, int is_final);
/* kernel level: a whole signal at once (zero history, flushed), same device code as the stream path; returns n_out
 * (<= y_cap, else SC_ERR_ARG).  16000 runs the design's filter like any other rate (the STREAM path bypasses it).  The
 * coefficient table of a rate is uploaded on first use and kept per device for the life of the process - the one
 * allocation a kernel-level entry point makes. */
long sc_resample(const float *x_dev, long n_in, int rate, float *y_dev, long y_cap, void *stream);

/* measurement aid (tools/resample_bench.py): hipEvent times ms[iters] (HOST) of the launch the staging step of an admission
 * of n_jobs chunks of n_in samples at `rate` issues, after three warm-up launches, on buffers of its own - rate 16000:
 * the scatter copy of n_jobs x n_in floats; another rate: the conversion launch for streams in mid-utterance (history
 * read and left). */
int sc_stage_bench(int rate, int n_jobs, int n_in, int iters, double *ms);

/* ---- energy curve of a long recording (segment.hip) ----------------------------------------
 * File mode cuts a recording of more than 60 s at low-energy points (simple_endpointing.py:81-145); the curve the cut
 * search reads - summed log mel filterbank energies, Gaussian-smoothed, sign flipped - can be computed on the GPU
 * (opt-in: `--segmentation gpu`, segmenter.smoothed_negative_energy(backend="gpu")).  For int16 x[0..n) at 16 kHz:
 *   s[0] = x[0], s[i] = x[i] - 0.97 x[i-1]                      (on the int16 values, not / 32768)
 *   F = 1 if n <= 400 else 1 + ceil((n - 400) / 160)            frames of 400 samples every 160, zeros behind the end
 *   P_f[k] = |rfft_512(frame f, zero padded)[k]|^2 / 512, k = 0..256;  E_f[j] = sum_k P_f[k] fb[j][k], j = 0..25
 *   E_f[j] == 0 -> 2.220446049250313e-16;  p[f] = (sum_j log E_f[j]) / 10
 *   y[f] = - sum_{d=-80..80} w[d] p[refl(f + d)],  w[d] = exp(-d^2 / 800) / sum,  refl(i): i mod 2F, then 2F-1-i if >= F
 * Float64 throughout, every sum in one order (k, j, d ascending), no atomics: the same input gives the same bytes. */
/* frames of n_samples samples (F above).  Pure host; SC_ERR_ARG (< 0) for n_samples < 1. */
long sc_segment_frame_count(long n_samples);
/* tables the library uses: fb [26][257] (the triangular mel filters over the integer bin edges
 * floor(513 mel2hz(m_i) / 16000), 0..8000 Hz) and gauss [161] (w above).  Pure host; either may be NULL. */
int sc_segment_design(double *fb, double *gauss);
/* kernel level: pcm_dev [n_samples] int16 and out_dev [out_cap] doubles are device pointers; smoothed 0 writes p[f],
 * 1 writes y[f]; returns F (SC_ERR_ARG, before anything is launched, for a null pointer, n_samples < 1 or F > out_cap).
 * One launch (smoothed 0) or two on `stream`.  The tables are uploaded on first use and kept per device for the life of
 * the process; with smoothed = 1 the raw curve goes through a workspace of F doubles that is allocated on first use, grows
 * geometrically with the requests and is kept per device as well (so smoothed calls on one device belong on one stream;
 * growing it waits for the device).  No other allocation. */
long sc_segment_energy(const int16_t *pcm_dev, long n_samples, int smoothed, double *out_dev, long out_cap, void *stream);

/* ---- encoder --------------------------------------------------------------- */

/* first Conv2d(1->d,3,stride 2)+ReLU (subsampling.py:87-93), channels-last out.
 * jobs[j] = {src_row0, T_in, c1_row0, T1}. */
int sc_conv1(const float *feat, int n_mels, const int32_t *jobs, int n_jobs, int max_t1,
             const float *w, const float *b, int d, float *c1, void *stream);

/* block assembly (contextual_block_transformer_encoder.py:354-380).
 * jobs[b] = {src_row0, chunk_len, pe_off_frames, pe_off_ctx, short, 0}. */
int sc_block_pack(const float *sub, const int32_t *jobs, int nb, int R, const float *pe, int d,
                  float *xblk, void *stream);

/* context hand-off (contextual_block_encoder_layer.py:253-269).
 * jobs[j] = {b0, nblk, state_row, has_state}; state row used = state_row + layer. */
int sc_ctx_handoff(float *x, int R, const int32_t *jobs, int ns, float *state, int layer, int d,
                   void *stream);

/* masked block self-attention (multi_head_attention.py:92-133 with the mask of
 * contextual_block_transformer_encoder.py:524-528). */
int sc_enc_attention(const float *qkv, float *att, int nblk, int R, int H, int d, int masked,
                     void *stream);

/* all encoder layers on (nblk, R, d) blocks (contextual_block_encoder_layer.py:178-271). */
int sc_encoder_layers(const sc_enc_layer *layers /*HOST*/, int n_layers, float *x, int nblk, int R,
                      int masked, const int32_t *jobs, int ns, float *past_ctx, float *xn,
                      float *qkv, float *att, float *ffh, int d, int H, int F, float eps,
                      void *stream);

/* ---- search ---------------------------------------------------------------- */

/* CTCPrefixScoreTH.extend_state (ctc_prefix_score_full.py:349-368) */
int sc_ctc_extend_state(const sc_search *sb /*HOST*/, void *stream);
/* embed*sqrt(d)+PE of the newest token (transformer_decoder.py:231) */
int sc_dec_embed(const sc_search *sb, void *stream);
/* kv_half: cross-attention K|V rows of all layers from an fp32 staging buffer [n_layers][m][d2] (the output of
 * the K|V projection GEMMs for m new encoder frames) into the fp16 cache: row j of layer li -> row
 * rows[j] + li*TCAP. */
int sc_kv_rows_to_half(const float *stage, const int32_t *rows, int m, int n_layers, int TCAP, int d2,
                       void *ckv_half, void *stream);
/* decoder self-attention with K/V cache + ancestor table (decoder_layer.py:85-101) */
int sc_dec_self_attn(const sc_search *sb, int layer, void *stream);
/* decoder cross-attention over the shared per-stream K/V (decoder_layer.py:106-115) */
int sc_dec_cross_attn(const sc_search *sb, int layer, void *stream);
int sc_decoder_layers(const sc_search *sb, void *stream);
/* Largest vocabulary the search kernels serve: sc_fuse_topw's full-vocabulary path keeps 8 V + 8 nextpow2(V) bytes in
 * LDS (128 KiB at V = 8192, of the 160 KiB of a CU; 8193 would need 192 KiB).  Larger vocabularies are refused when a
 * batch is made (sc_streams_create; speechcatcher_amd.hip_backend.HipBackend.check_supported) and by both kernels. */
#define SC_MAX_VOCAB 8192
/* log_softmax + pre-beam top-K (transformer_decoder.py:249, beam_search.py:150-154) */
int sc_logsoftmax_topk(const sc_search *sb, void *stream);
/* CTCPrefixScoreTH.__call__ on the K candidates (ctc_prefix_score_full.py:88-291) */
int sc_ctc_prefix_scan(const sc_search *sb, void *stream);
/* the same scores; streams with at least split_min (> 0) frames behind their first scanned frame are walked by 16
 * threads per (hypothesis, candidate) - segment-wise affine maps of the recurrence, combined, then re-walked - instead
 * of one: for long tables (T = 4500: a 180 s segment) while few streams are active */
int sc_ctc_prefix_scan_split(const sc_search *sb, int split_min, void *stream);
/* score fusion + per-hypothesis top-W (beam_search.py:113-185,723) */
int sc_fuse_topw(const sc_search *sb, void *stream);
/* expand / prune / bookkeeping / stop flags (beam_search.py:721-809, hypothesis.py:132-142) */
int sc_beam_prune(const sc_search *sb, void *stream);
/* CTCPrefixScorer.select_state (scorers.py:382-431) */
int sc_ctc_gather_state(const sc_search *sb, void *stream);
/* ... behind sc_ctc_prefix_scan_split(sb, split_min): the streams whose scan was split over T (the same rule: at least
 * split_min frames to walk) left the start states of their CTC_NSEG = 32 segments instead of 16-frame checkpoints */
int sc_ctc_gather_state_split(const sc_search *sb, int split_min, void *stream);
/* one full beam-search step = all of the above in order (beam_search.py:701-758) */
int sc_decode_step(const sc_search *sb, void *stream);
/* ... with the CTC prefix scan of streams that have >= scan_split_min frames to walk split over T
 * (sc_ctc_prefix_scan_split; 0: never) */
int sc_decode_step_ex(const sc_search *sb, int scan_split_min, void *stream);
/* ---- head-parallel decoder layers: 3 launches per layer (decoder_layer.py:80-132) --------------------
 * The residual stream x ping-pongs between two [S*W][d] buffers (x_in != x_out in every call): sibling
 * workgroups read x_in while the owner of a row writes x_out.  Grid (stream, head) for the two attention
 * launches; every workgroup sums the producer's partial products itself (fixed order) and recomputes the
 * LayerNorm of its stream's W rows, so neither the LayerNorms nor the attention output projections need
 * launches of their own.  d in {128, 256}, head dim in {16, 32} and (round 6, d = 256) 64 - the reference's geometry when
 * config.yaml names no heads (speech2text_streaming.py:221-227) -, W <= 16, sc_ffn_ln_supported(d, F). */
int sc_dec_layer_fused_supported(int d, int H, int W, int F);
/* A: x = x_in + b2[layer-1] + sum_z ffn_part[z][row]  (layer 0: embed*sqrt(d)+PE, transformer_decoder.py:231;
 * x_in / ffn_part unused) -> x_out; q|k|v = norm1(x) . Wqkv^T + b of every head; K|V row appended to the
 * cache; self-attention through the ancestor table (decoder_layer.py:85-101); ph1 = per-head partial of
 * self_attn.linear_out. */
int sc_dec_layer_self(const sc_search *sb, int layer, const float *x_in, float *x_out, const float *ffn_part,
                      int n_ffn_part, void *stream);
/* B: x = x_in + bo + sum_h ph1 -> x_out; q = norm2(x) . Wq^T + bq; cross-attention over the stream's shared
 * encoder K|V (decoder_layer.py:106-115); ph2 = per-head partial of src_attn.linear_out. */
int sc_dec_layer_cross(const sc_search *sb, int layer, const float *x_in, float *x_out, void *stream);
/* C: x = x_in + bo2 + sum_h ph2 -> x_out; feed-forward of norm3(x) (decoder_layer.py:117-123,
 * feed_forward.py:48-50) as partial sums ffn_part[z][row], z < *n_part (HOST out; <= max_part).  *n_part is F/128 or
 * F/256 (aligned pairs of chunks; always pairs when F/128 is even and > 16): with fp32 partial sums either gives the same
 * bits behind the consumer's tree and the row count picks; with fp16 partial sums (act_half & 2), which are rounded at the
 * store, it is F/256 whenever F/128 is even - a function of F alone. */
int sc_dec_layer_ffn(const sc_search *sb, int layer, const float *x_in, float *x_out, float *ffn_part,
                     int max_part, int *n_part /*HOST*/, void *stream);
/* ---- stream-resident decoder layers: 2 launches per layer (round 6; decoder_layer.py:80-132) -------------------
 * d = 256, 8 heads of 32, W <= 10, fp32 weights.  One workgroup per stream: no partial products between the attentions. */
int sc_dec_layer_stream_supported(int d, int H, int W, int F);
/* A': x = x_in + b2[layer-1] + sum_z ffn_part[z][row] (layer 0: embed*sqrt(d)+PE); self-attention block (norm1, q|k|v of all
 * heads, K|V row appended, attention through the ancestor table, linear_out + residual: decoder_layer.py:85-101);
 * cross-attention block (norm2, q, attention over the stream's encoder K|V, linear_out + residual: :106-115) -> x_out;
 * xn_out = norm3(x_out) (:117). */
int sc_dec_layer_stream(const sc_search *sb, int layer, const float *x_in, float *x_out, float *xn_out,
                        const float *ffn_part, int n_ffn_part, void *stream);
/* C': feed-forward of the rows xn (feed_forward.py:48-50) as partial sums ffn_part[z][row] by row id, z < *n_part. */
int sc_dec_layer_ffn_xn(const sc_search *sb, int layer, const float *xn, float *ffn_part, int max_part,
                        int *n_part /*HOST*/, void *stream);
/* B2 (round 6; the four-head form at large buckets): x = x_in + bo2 + sum_h ph2 -> x_out, xn_out = norm3(x) once per row
 * (decoder_layer.py:113-117) - the feed-forward then runs without prologue (sc_dec_layer_ffn_xn) */
int sc_dec_layer_reduce_ln(const sc_search *sb, int layer, const float *x_in, float *x_out, float *xn_out, void *stream);
/* tail: x = x_in + b2[last] + sum_z ffn_part -> x_out; logits = after_norm(x) . out_w^T + out_b
 * (transformer_decoder.py:243-249); needs sb->out_w_q. */
int sc_dec_output_logits(const sc_search *sb, const float *x_in, float *x_out, const float *ffn_part,
                         int n_ffn_part, void *stream);

/* ---- Conformer building blocks (north-star components, unused by the shipped
 * contextual-block Transformer models: SURVEY.md section 8(f) rank 3) ---------- */

/* GLU -> depthwise Conv1d(ksize, same padding) -> BatchNorm1d(eval) -> Swish of
 * ConvolutionModule.forward (model/layers/convolution.py:103-112); the two
 * pointwise convolutions around it are sc_gemm calls.  y [B][T][2C] -> out [B][T][C]. */
int sc_glu_dwconv_bn_swish(const float *y, int B, int T, int C, int ksize, const float *dw_w,
                           const float *dw_b, const float *bn_g, const float *bn_b,
                           const float *bn_mean, const float *bn_var, float bn_eps, float *out,
                           void *stream);

/* RelPositionMultiHeadedAttention.forward core (model/attention/multi_head_attention.py:
 * 343-378, rel_shift :300-314): qkv [B*T][3d] projected q|k|v, p [T][d] = linear_pos(pos_emb),
 * bias_u / bias_v [H][dk] -> out [B*T][d] (before linear_out).  Any T. */
int sc_relpos_attention(const float *qkv, const float *p, const float *bias_u, const float *bias_v,
                        float *out, int B, int T, int H, int d, void *stream);
/* ... with the reference's attention masks (:366-372): mask_mode 1 = mask [B][T] over keys (batch, 1, time_k),
 * 2 = mask [B][T][T] (batch, time_q, time_k), bytes, 0 = masked out; a fully masked query row gives zeros. */
int sc_relpos_attention_masked(const float *qkv, const float *p, const float *bias_u, const float *bias_v,
                               float *out, int B, int T, int H, int d, const uint8_t *mask, int mask_mode,
                               void *stream);

/* ==== stream-level API: the decoder as a C library ==========================================
 * What a reference maintainer binds instead of Speech2TextStreaming's torch modules:
 *   engine  = one weight replica on one GPU            (load_model, speechcatcher.py:126-227)
 *   streams = S independent recognitions sharing it    (S x Speech2TextStreaming, speech2text_streaming.py:43-263)
 *   sc_push = Speech2TextStreaming.__call__ for the listed streams, batched   (:402-539)
 * The library owns all device memory of these objects.  Handles are not thread-safe: one host thread and
 * one HIP stream per sc_streams.  Functions return SC_OK / a negative code and never throw. */
typedef struct sc_config {
  int32_t d_model, enc_heads, enc_layers, dec_heads, dec_layers, ffn_dim, vocab_size;
  int32_t n_mels, n_fft, win_length, hop_length, sample_rate;
  int32_t block_size, hop_size, look_ahead, subsample, conv_freq1, conv_freq2;
  int32_t blank_id, sos_id, eos_id, pe_max_len;
  int32_t mvn_mode; /* 0: no global MVN, 1: fp32 statistics, 2: fp64 statistics */
  float ln_eps;
} sc_config;

typedef struct sc_named_tensor {
  const char *name; /* PackedWeights names: "window", "conv2_w", "enc.3.wqkv_p", "dec.0.wkv", ... */
  const void *data; /* DEVICE pointer, borrowed for the lifetime of the engine */
  int64_t numel;
  int32_t dtype; /* 0 = f32, 1 = f64 (mean64 / std64), 2 = f16 (w1_h / w2_h) */
} sc_named_tensor;

typedef struct sc_stream_options {
  int32_t n_streams, beam_size;
  float ctc_weight;          /* 0.3 (speechcatcher.py:221) */
  int32_t use_bbd;           /* block boundary detection (beam_search.py:771-790) */
  int32_t max_frames;        /* encoder frames per utterance (capacity) */
  int32_t max_tokens;        /* tokens per hypothesis incl. sos (capacity) */
  int32_t pcm_capacity;      /* samples buffered per stream (0: 1 << 20) */
  int32_t max_chunk_samples; /* longest single call (0: 32768) */
  int32_t strict_reference;  /* reset() leaves the stale CTC table / PE counter like the reference (scorers.py:342-350) */
  int32_t kv_half;           /* K|V caches in fp16 (fp32 arithmetic): BASELINE configs[4]'s storage mode; 0 = fp32 */
  int32_t kv_pool_rows;      /* rows of the self-attention K|V pool per stream and layer (capacity; at most max_tokens x beam =
                                one row per (position, hypothesis)).  0 = default: that maximum - a stream can then never run out
                                of rows before max_tokens - unless it would take more than a quarter of the device's free memory
                                (thousands of streams): then what that budget holds, at least 1.5 x max_tokens + 4 x beam.  A
                                stream that needs more rows than the pool has fails with SC_ERR_CAPACITY at the step that is
                                actually TAKEN (a step that is rolled back or rewound never fails) and is reset */
} sc_stream_options;

typedef struct sc_stream_info_t {
  int32_t enc_frames, processed_block, process_idx, n_hyp, hyp_len, pcm_buffered, frontend_started;
  int64_t decode_steps;
} sc_stream_info_t;

typedef struct sc_engine sc_engine;
typedef struct sc_streams sc_streams;

/* weights already on the device, in the layout of speechcatcher_amd.weights.PackedWeights (Python host) */
int sc_engine_create(const sc_config *cfg, const sc_named_tensor *tensors, int n_tensors, int device, sc_engine **out);
/* ... or from a packed model file written by PackedWeights.save_packed (C / C++ hosts: no Python, no torch) */
int sc_engine_load(const char *packed_model_path, int device, sc_engine **out);
int sc_engine_config(const sc_engine *engine, sc_config *out);
void sc_engine_destroy(sc_engine *engine);

int sc_streams_create(sc_engine *engine, const sc_stream_options *options, sc_streams **out);
void sc_streams_destroy(sc_streams *streams);
/* One chunk step for n streams: stream_ids[i] (each stream at most once per call) gets n_samples[i] float samples
 * in +-1 from pcm[i] (HOST; NULL = already resident in the device PCM buffer, see sc_streams_pcm) with is_final[i],
 * at the stream's input rate (sc_stream_set_input_rate; 16 kHz unless set).
 * The host chunks are staged in pinned memory and reach the device with ONE copy.  Runs frontend -> encoder ->
 * every decode block that became ready (run to completion).  status[i] (HOST out, may be NULL): 1 output, 0 the
 * reference's early `return []`, SC_ERR_CAPACITY / SC_ERR_INPUT: this stream failed and was reset (message:
 * sc_stream_last_error), the others are unaffected. */
int sc_push(sc_streams *streams, const int *stream_ids, const float *const *pcm, const int *n_samples,
            const uint8_t *is_final, int n, int *status);
/* the same for 2-D (T, n_mels) already-normalised feature matrices (speech2text_streaming.py:438-449) */
int sc_push_features(sc_streams *streams, const int *stream_ids, const float *const *feats, const int *n_frames,
                     const uint8_t *is_final, int n, int *status);
/* Continuous batching - the reference server's concurrency unit is an independent stream that is called, answers,
 * and is called again (recognize_ws / process_audio_chunk, speechcatcher_server.py:205-296,359-397), not a batch in
 * lock-step.  sc_submit hands the engine ONE chunk for each listed stream (copied; a stream has at most one chunk
 * outstanding) and returns at once: the chunks are planned and their frontend + encoder stage is issued as one group
 * on the encoder HIP stream.  sc_poll runs the decode side - one beam-search step per tick for EVERY stream that is
 * inside a block, whichever call it belongs to - until at least min_done outstanding chunks are complete (or none is
 * outstanding) and reports up to max_done of them: done_ids[i] = stream, status[i] as in sc_push.  Returns the
 * number reported, < 0 on error.  A stream's reply is ready when ITS blocks are done; streams that finish early
 * get their next chunk while the stragglers of the previous one are still decoding.  Per stream the blocks, steps
 * and results are those of sc_push (the kernel form of a decode step follows the number of streams in it, and with it the
 * fp32 summation order: scores agree to ~1e-5, a beam cut closer than that can fall either way).  sc_push may be mixed in: it also advances the submitted streams. */
int sc_submit(sc_streams *streams, const int *stream_ids, const float *const *pcm, const int *n_samples,
              const uint8_t *is_final, int n);
int sc_poll(sc_streams *streams, int min_done, int max_done, int *done_ids /*HOST out*/, int *status /*HOST out, may be NULL*/);
int sc_streams_outstanding(const sc_streams *streams);
/* sc_submit policy: a chunk's own decode block only sees frames that were there before it (the block schedule runs one
 * hop behind the encoder, beam_search.py:590-634), so its frontend + encoder stage has a whole chunk period of slack:
 * the stages of successive admissions are merged and issued as ONE group when it holds min_streams streams (default:
 * half of the streams) or as soon as a queued decode block needs its frames.  1: every admission is issued at once.
 * Results do not depend on it in the fp32 form.  With split-precision projections ("split16") the group's row count
 * selects between the tiled GEMM (split operands) and the small-M kernels (fp32) for the subsampling / CTC / cross-K|V
 * projections: both are fp32-grade, results can differ in the last bits of fp32 between group sizes. */
int sc_streams_set_encoder_batch(sc_streams *streams, int min_streams);
/* Chunks a stream may have outstanding at a time (1..8; default 1 = the reference's call -> reply -> next call,
 * speechcatcher_server.py:359-397).  depth > 1: sc_submit accepts the next chunk(s) of a stream while an earlier one
 * is still being decoded, for hosts that already have the audio (a file: the reference CLI's chunk loop,
 * speechcatcher.py:574-592; a backlog): the frontend + encoder of chunk k+1 run beside the decoding of chunk k and the
 * stream does not idle between its reply and its next call.  Per stream the chunks are processed and reported in
 * order, at most one per sc_poll call, each with the results of the one-at-a-time protocol; the hypotheses of a
 * reported chunk are a copy taken when it completed, returned by sc_get_hyps / sc_get_hyps_batch until the NEXT
 * sc_poll call.  Nothing can be queued behind a final chunk; a chunk that fails (at admission or while decoding)
 * fails the chunks queued behind it as well - each is reported in its turn (also those submitted before the last of
 * them has been reported), the stream is reset once, when the chunk that failed is reported.  The depth can only be
 * changed while nothing is outstanding.  sc_push on such a handle works as always (it needs the stream idle). */
int sc_streams_set_queue_depth(sc_streams *streams, int depth);
/* message of the stream's last failure (status < 0 from sc_push / sc_poll); "" if it never failed */
const char *sc_stream_last_error(const sc_streams *streams, int stream);
/* live hypotheses, best first (BeamState.hypotheses: yseq, xpos, score, scores{decoder, ctc}; hypothesis.py).
 * Returns how many were written (<= nbest) or a negative code. */
int sc_get_hyps(sc_streams *streams, int stream, int nbest, int max_len, int32_t *ids, int32_t *xpos, int *lens,
                double *scores, double *score_dec, double *score_ctc);
/* ... of n streams at once - what a batch of Speech2TextStreaming.__call__s hands back (speech2text_streaming.py:
 * 466-539): ONE pack launch and ONE device-to-host copy into pinned memory.  ids / xpos [n][nbest][max_len],
 * lens / scores / score_dec / score_ctc [n][nbest], n_hyps [n]; any output but n_hyps may be NULL. */
int sc_get_hyps_batch(sc_streams *streams, const int *stream_ids, int n, int nbest, int max_len, int32_t *ids,
                      int32_t *xpos, int *lens, int *n_hyps, double *scores, double *score_dec, double *score_ctc);
/* What a caller that already holds the first from[i] tokens of stream i's best hypothesis still needs, and how much of
 * it is final (sc_hyp_commit above): for the hypotheses sc_get_hyps_batch would return (same rules: the
 * snapshot with a queue depth > 1, an error for a stream inside a decode block or listed twice) L[i], commit[i] - the
 * length of the prefix all live hypotheses share, which no later chunk changes -, n_hyps[i], and the tail of the best
 * one: ids / xpos / stability [n][max_tail], the first L[i] - from[i] of each row written, scores [n][3] (total,
 * decoder, ctc), status [n] (SC_COMMIT_*).  final[i] != 0 (final may be NULL): the chunk was the utterance's last, all
 * of the best hypothesis is committed.  A stream that has not started: n_hyps = L = commit = 0.  SC_ERR_ARG for
 * from[i] > L[i], L[i] - from[i] > max_tail, or more than SC_COMMIT_MAX_HYPS live hypotheses.  ONE job-table upload,
 * ONE launch and ONE copy back into pinned memory, on the read-back stream; the call keeps no state and changes none.
 * Any output may be NULL. */
int sc_get_hyps_delta(sc_streams *streams, const int *stream_ids, int n, const int *from, const int *final,
                      int max_tail, int32_t *L, int32_t *commit, int32_t *n_hyps, int32_t *ids, int32_t *xpos,
                      double *stability, double *scores, int32_t *status);
/* N-gram rescoring of the hypotheses sc_get_hyps_batch would return (sc_lm_rescore above; same rules: the
 * snapshot with a queue depth > 1, an error for a stream inside a decode block or listed twice): per stream its first
 * n_hyps[i] = min(nbest, live hypotheses) rows, labels without <sos> and without a trailing <eos>, from the model's
 * start_state; the </s> term (lm_eos >= 0: the id that stands for </s> in the model, -1: none) only where final[i] != 0
 * (final may be NULL).  order / fused / lm_sum / eos_lm / status [n][nbest] (any may be NULL; entries behind n_hyps[i] are
 * left as they are); order[i][r] indexes the rows of sc_get_hyps_batch.  lm: any sc_lm whose V is the model's vocabulary
 * size; it is not bound to the handle, and the call has synchronised before it returns.  nbest <= SC_RESCORE_MAX_HYPS.
 * The buffers are allocated by the first call; ONE job-table upload, ONE launch and ONE copy back into pinned memory,
 * all on the read-back stream.  Reads the engine's state, changes none, keeps none of its own. */
int sc_rescore_hyps(sc_streams *streams, const int *stream_ids, int n, int nbest, const sc_lm *lm, double alpha,
                    double beta, int lm_eos, const int *final, int32_t *order, double *fused, double *lm_sum,
                    double *eos_lm, int32_t *status, int *n_hyps);
/* The same launch for caller-given lists (all arrays HOST): list i has list_sizes[i] <= nbest rows, row r the LABELS
 * ids[i][r][0 .. lens[i][r]) - nothing skipped, nothing stripped - and the total scores[i][r]; state0[i] is the
 * automaton's state before the first label (-1, or state0 == NULL: the model's start_state).  Outputs [n][nbest] as above,
 * and end_state.  How the final of a decoder-free stream gets its </s> term (the ids and totals of sc_ctc_beam_hyps). */
int sc_lm_rescore_lists(sc_streams *streams, const sc_lm *lm, const int32_t *ids, const int32_t *lens,
                        const double *scores, const int *list_sizes, int n, int nbest, int max_len,
                        const int32_t *state0, double alpha, double beta, int lm_eos, int32_t *order, double *fused,
                        double *lm_sum, double *eos_lm, int32_t *status, int32_t *end_state);
/* Attention rescoring of n-best lists at finals (sc_dec_rescore above): ONE teacher-forced pass of the
 * attention decoder over the rows of the lists, against the listed streams' encoder rows enc[s][0 .. T_enc) - FULL and
 * decoder-free streams alike; a FULL stream's cross-attention cache is not reused, K|V are projected from the encoder rows
 * on one path.  fp32 weights only (SC_ERR_UNSUPPORTED when the handle does not hold them).  A listed stream must be idle -
 * no chunk outstanding, as for sc_reset -; its encoder group is waited for, as the beam's readers do.  Everything runs on
 * the read-back stream with one copy back; nothing of the engine is written, and a handle that never calls these
 * allocates nothing for them and issues the launches it issued before.  After sc_reset a stream has no frames: every
 * row SC_ATT_NO_FRAMES.  The workspace is allocated by the first call, as large as that call needs but never beyond the
 * limit (default SC_ATT_WS_DEFAULT_BYTES; sc_streams_set_attention_rescore_ws, at least 1 MiB); a call that needs more
 * is processed in slabs of whole streams, with the same bits; SC_ERR_CAPACITY when one stream's list alone does not fit.
 * sc_streams_attention_rescore_ws reports the limit and what is allocated.
 * sc_attention_rescore_beam: the first nbest <= SC_ATT_MAX_HYPS entries of the listed streams' REPORTED CTC beam states -
 * the entries sc_ctc_beam_hyps returns, packed on the device by sc_ctc_beam_pack -, their first-pass scores the entries'
 * totals lae(pb, pnb), with a language model attached the fused totals of sc_ctc_beam_hyps_lm; ctc_score [n][nbest]
 * receives them.  Outputs [n][nbest], n_hyps[i] entries each: order, fused, att, status as sc_dec_rescore defines them.
 * sc_attention_rescore_lists: the same for caller-given lists - list i has list_sizes[i] <= nbest rows, row r its
 * lens[i][r] labels ids[i][r][0 .. lens) and its total scores[i][r] - against the encoder rows of stream_ids[i] (a stream
 * may be listed more than once). */
#define SC_ATT_WS_DEFAULT_BYTES ((size_t)256 << 20)
int sc_attention_rescore_beam(sc_streams *streams, const int *stream_ids, int n, int nbest, double w_att, double w_ctc,
                              double beta, int32_t *order, double *fused, double *att, double *ctc_score, int32_t *status,
                              int *n_hyps);
int sc_attention_rescore_lists(sc_streams *streams, const int *stream_ids, int n, const int32_t *ids, const int32_t *lens,
                               const double *scores, const int *list_sizes, int nbest, int max_len, double w_att,
                               double w_ctc, double beta, int32_t *order, double *fused, double *att, int32_t *status);
int sc_streams_set_attention_rescore_ws(sc_streams *streams, size_t max_bytes);
int sc_streams_attention_rescore_ws(const sc_streams *streams, size_t *limit, size_t *allocated);
/* Consensus of n-best lists at finals (sc_mbr above): the minimum-Bayes-risk row and the slot statistics
 * of the pivot.  The scratch area of the read-back services holds the job table, the inputs and the outputs; ONE
 * upload, the launches of sc_mbr on the read-back stream, ONE copy back; nothing of the engine is written, and a handle
 * that never calls these allocates nothing for them and issues the launches it issued before.  The direction workspace
 * is an allocation of its own, made by the first call as large as that call needs, grow-only and never beyond the limit
 * (default SC_MBR_WS_DEFAULT_BYTES; sc_streams_set_mbr_ws, at least SC_MBR_WS_MIN_BYTES - what one list of
 * SC_MBR_MAX_LEN labels needs); a call that needs more runs in slabs of whole lists, with the same bits.
 * sc_streams_mbr_ws reports the limit and what is allocated.
 * sc_mbr_hyps: the hypotheses sc_get_hyps_batch would return (same rules: the snapshot with a queue depth > 1, an error
 * for a stream inside a decode block or listed twice), per stream its first n_hyps[i] = min(nbest, live hypotheses) rows,
 * labels without <sos> and without a trailing <eos>, scores the hypotheses' totals times `scale` (finite, >= 0).
 * pivot_best != 0 pins the pivot to row 0: the reported transcript stays the search's, only the slot statistics are
 * added.  nbest <= SC_MBR_MAX_HYPS; SC_ERR_ARG when a stream's rows have more than max_len labels (at most
 * SC_MBR_MAX_LEN are ever needed).
 * sc_mbr_lists: the same for caller-given lists (all arrays HOST): list i has list_sizes[i] <= nbest rows, row r the
 * LABELS ids[i][r][0 .. lens[i][r]) - nothing skipped, nothing stripped -, values[i][r] its total (are_weights == 0) or
 * its weight (are_weights != 0), pivot[i] the job's pivot (NULL: -1 everywhere); V is the handle's vocabulary size.
 * The way in for the n-best of decoder-free streams and for lists whose totals were fused by 8l or 8n.
 * Outputs (any may be NULL; what lies behind n_hyps[i] / list_sizes[i] entries, or behind m_P positions, is left as it
 * is): order / risk / weight / status [n][nbest], header [n][4], dist [n][16][16], conf / alt_tok / alt_mass [n][max_len],
 * gap_mass [n][max_len + 1]; a stream without hypotheses or an empty list gets header {-1, 0, 0, 0}. */
#define SC_MBR_WS_DEFAULT_BYTES ((size_t)256 << 20)
#define SC_MBR_WS_MIN_BYTES ((size_t)8 << 20)
int sc_mbr_hyps(sc_streams *streams, const int *stream_ids, int n, int nbest, double scale, int pivot_best, int max_len,
                int32_t *order, double *risk, double *weight, int32_t *status, int32_t *header, int32_t *dist,
                double *conf, int32_t *alt_tok, double *alt_mass, double *gap_mass, int *n_hyps);
int sc_mbr_lists(sc_streams *streams, const int32_t *ids, const int32_t *lens, const double *values, int are_weights,
                 const int *list_sizes, const int32_t *pivot, int n, int nbest, int max_len, double scale,
                 int32_t *order, double *risk, double *weight, int32_t *status, int32_t *header, int32_t *dist,
                 double *conf, int32_t *alt_tok, double *alt_mass, double *gap_mass);
int sc_streams_set_mbr_ws(sc_streams *streams, size_t max_bytes);
int sc_streams_mbr_ws(const sc_streams *streams, size_t *limit, size_t *allocated);

/* CTC forced alignment of the hypotheses sc_get_hyps_batch would return (same rules: the snapshot with a queue depth
 * > 1, an error for a stream inside a decode block), best first, against the stream's own CTC rows: the T frames of
 * the decode block the hypotheses come from.  Labels: yseq without <sos> and without a trailing <eos>.  Outputs
 * start / end / logp_mean [n][nbest][max_len], path_score / status [n][nbest] (SC_ALIGN_*), n_hyps [n]; any output
 * but n_hyps may be NULL.  Runs on the read-back stream; decoding is not affected.  The backpointer workspace is
 * allocated on the first call and grows with the requests. */
int sc_align_hyps(sc_streams *streams, const int *stream_ids, int n, int nbest, int max_len, int32_t *start,
                  int32_t *end, float *logp_mean, double *path_score, int *status, int *n_hyps);
/* sc_align_hyps and, for every token of every hypothesis, its alternates (sc_ctc_alternates above): the
 * alignment's launches, then ONE sc_ctc_alternates launch on the same read-back stream over the spans the alignment left
 * on the device, one copy back.  start ... status: exactly what sc_align_hyps gives, bit for bit.  alt_ids / alt_logp
 * [n][nbest][max_len][K], own_rank / span_status [n][nbest][max_len] (SC_ALT_*; SC_ALT_NO_SPAN for every token of a
 * hypothesis whose alignment failed); any output but n_hyps may be NULL.  1 <= K <= SC_ALT_MAX_K. */
int sc_alternates_hyps(sc_streams *streams, const int *stream_ids, int n, int nbest, int max_len, int K, int32_t *start,
                       int32_t *end, float *logp_mean, double *path_score, int *status, int32_t *alt_ids,
                       double *alt_logp, int32_t *own_rank, int32_t *span_status, int *n_hyps);
/* ... of a caller-given transcript ids[0..L) against the same frames of one stream */
int sc_align_tokens(sc_streams *streams, int stream, const int32_t *ids, int L, int32_t *start, int32_t *end,
                    float *logp_mean, double *path_score, int *status);
/* Speech2TextStreaming.reset (speech2text_streaming.py:252-263); not while the stream has a chunk outstanding.
 * The stream's input rate stays; its sample-rate converter starts over. */
int sc_reset(sc_streams *streams, int stream);
/* stream level: rate of the samples sc_push / sc_submit take for this stream.  Only on a stream that is idle and has
 * buffered nothing since its last reset; SC_ERR_ARG otherwise or for an unsupported rate.  Default 16000.
 * A stream at another rate is converted on the GPU in the admission's staging step (one launch per admission for all
 * such chunks; 16 kHz chunks of the same admission take the plain copy): the call then counts as one of n_out 16 kHz
 * samples, n_out from the integer formula above.  Both the call's n_samples and its n_out must be
 * <= max_chunk_samples + 16 hops (else SC_ERR_CAPACITY for that stream); pcm[i] == NULL (device-resident PCM) is
 * SC_ERR_ARG on such a stream.  A final call flushes the filter and ends the utterance: the next call starts a new
 * signal.  At most 8 distinct rates other than 16000 per sc_streams; the table of a rate is designed in float64 and
 * uploaded when the rate is first set. */
int sc_stream_set_input_rate(sc_streams *streams, int stream, int rate);
int sc_stream_input_rate(const sc_streams *streams, int stream);
/* stream level: wire format of the audio a stream takes (pcm.hip above) - format SC_PCM_*, channels 1..8
 * interleaved, channel in [0, channels) or SC_PCM_MIX, scale SC_PCM_SCALE_* (SC_PCM_SCALE_SERVER only with S16LE / MULAW /
 * ALAW).  The preconditions of sc_stream_set_input_rate: an idle stream that has buffered nothing since its last reset;
 * SC_ERR_ARG otherwise or for a value out of range.  Default (SC_PCM_F32, 1, 0, SC_PCM_SCALE_FULL): mono floats, today's
 * path.  The format survives sc_reset and composes with the input rate: the decoded samples are what a float chunk
 * would have been - scattered into the PCM ring at 16 kHz, the converter's input at another rate.  A stream with any
 * other format is CODED: it takes its audio through sc_push_raw / sc_submit_raw only (sc_push / sc_submit: SC_ERR_ARG),
 * host pointers only.  A coded chunk's bytes travel in a byte region of the admission's pinned staging slot (as large as
 * the slot's floats; pinned and device memory for it, the job tables and S level records are allocated when a format is
 * first set on the handle); ONE sc_pcm_decode launch per admission on the encoder stream writes the float spans reserved
 * for them before the admission's scatter / conversion launch reads those.  n_frames and the 16 kHz sample count obey
 * the limits of sc_stream_set_input_rate; a chunk whose bytes do not fit what is left of the byte region fails THAT stream
 * with SC_ERR_CAPACITY (a format of at most 4 bytes per frame always fits).  An admission without coded chunks launches
 * nothing new. */
int sc_stream_set_input_format(sc_streams *streams, int stream, int format, int channels, int channel, int scale);
int sc_stream_input_format(const sc_streams *streams, int stream, int *format, int *channels, int *channel, int *scale);
/* sc_push / sc_submit with audio[i] = the bytes of n_frames[i] sample FRAMES in stream_ids[i]'s format (HOST; floats for
 * a stream without a format: then these ARE sc_push / sc_submit) */
int sc_push_raw(sc_streams *streams, const int *stream_ids, const void *const *audio, const int *n_frames,
                const uint8_t *is_final, int n, int *status);
int sc_submit_raw(sc_streams *streams, const int *stream_ids, const void *const *audio, const int *n_frames,
                  const uint8_t *is_final, int n);
/* input level of a coded stream, cumulative over the utterance, up to and including the stream's last REPORTED chunk - the
 * chunk whose hypotheses sc_get_hyps returns - however many chunks are queued behind it; a stream's first chunk after
 * sc_reset or after a final chunk starts over.  All zero after sc_reset, for a stream without a format and for SC_PCM_F32
 * (then with full_scale = 0).  Waits for the staging step of that chunk if it is still in flight. */
int sc_stream_input_level(sc_streams *streams, int stream, sc_input_level_t *out /*HOST*/);
int sc_stream_info(const sc_streams *streams, int stream, sc_stream_info_t *out);
/* rows of the self-attention K|V pool per (stream, layer) this batch was created with (sc_stream_options.kv_pool_rows, or the
 * default: one row per (position, hypothesis) within min(a quarter of the free device memory, SC_KV_POOL_DEFAULT_MAX_GIB)) */
#define SC_KV_POOL_DEFAULT_MAX_GIB 24
int sc_streams_kv_rows(const sc_streams *streams);
int sc_streams_stats(const sc_streams *streams, long *enc_calls, long *dec_steps, long *dec_blocks);
/* measurement aid: encoder-layer hipGraphs captured so far (one per shape of an encoder group) and the host seconds
 * that took */
int sc_streams_capture_stats(const sc_streams *streams, long *n_captures, double *seconds);
/* measurement aids (bench.py): hipGraph replay on/off (off: launches can be bracketed by the sc_prof_* events);
 * encoder K|V rows the cross-attention has read since the last call (returned and cleared) */
int sc_streams_set_graphs(sc_streams *streams, int on);
/* measurement aid (tools/prof_bench.sh): an empty kernel named sc_marker_kernel<id> (id 0..3) on `stream` - brackets a window
 * of the run in a rocprofv3 trace / counter collection, so that the launches of THAT window can be told from the rest */
int sc_marker(int id, void *stream);
/* host seconds the decode step loop spent issuing a step (ctrl upload + graph launch) and waiting for its stop
 * flags, since the last call (returned and cleared) */
int sc_streams_host_times(sc_streams *streams, double *launch_s, double *wait_s);
/* ... and by compaction bucket: seconds[17], iterations[17] (index = bucket size in units of n_streams/16) */
int sc_streams_bucket_times(sc_streams *streams, double *seconds, long *iterations);
long sc_streams_take_xattn_rows(sc_streams *streams);
/* ... split by the kernel that read them (HOST [3]): rows[0] dec_attn_flash, rows[1] sc_dec_layer_cross, rows[2] sc_dec_layer_stream */
int sc_streams_take_xattn_rows_by_kernel(sc_streams *streams, long *rows);
/* all attention counters since the last call (returned and cleared), each summed over decode iterations, active streams
 * and decoder layers, by the form of the decoder layers that did the work - [0] stand-alone attention kernels (six launches per
 * layer) / [1] head-parallel layer kernels / [2] stream-resident layer kernel:
 *   out[0..2] encoder K|V rows the cross-attention read, out[3..5] token positions the self-attention covered (L per
 *   hypothesis: the algorithmic length), out[6..8] DISTINCT self-attention K|V rows read (device counter) */
int sc_streams_take_attn_counters(sc_streams *streams, long *out /*HOST [9]*/);
/* the batch's HIP stream and its device PCM ring [n_streams][capacity] (bench: inputs resident in HBM) */
void *sc_streams_hip_stream(sc_streams *streams);
float *sc_streams_pcm(sc_streams *streams, long *capacity);
/* host <-> device copies: write samples into a stream's device PCM ring; read back the samples buffered by the
 * frontend (frontend_states["waveform_buffer"], speech2text_streaming.py:300-338) and the encoder output so far
 * (beam_search.encoder_buffer).  The read functions return the number of samples / frames. */
int sc_streams_write_pcm(sc_streams *streams, int stream, long offset, const float *host, long n);
long sc_streams_read_pcm_buffer(sc_streams *streams, int stream, float *host, long max_n);
int sc_streams_read_enc(sc_streams *streams, int stream, float *host, int max_frames);
/* test aid: the CTC rows [0, min(T, max_rows)) of a stream's table as sc_align_hyps sees them (T: the frames of the
 * reported hypotheses' decode block) -> host [rows][vocab]; returns the number of rows */
int sc_streams_read_ctc(sc_streams *streams, int stream, float *host, int max_rows);
/* Acoustic activity per stream (off by default).  on != 0: every admission group issues ONE sc_ctc_activity
 * launch right behind its CTC projection, on the encoder stream, over the CTC rows [c0, t1) each of its chunks projects
 * (raw logits: the search's in-place log-softmax of a first block runs behind the group's event); frames are silence
 * iff bad or p_blank > blank_threshold (in (0, 1)).  The per-stream state and the S x max_frames track of doubles live
 * on the device and are allocated when the option is first switched on; switched off, no path does any new work.
 * SC_ERR_ARG while any chunk is outstanding.  Switching it on (again) restarts every stream's state.
 * strict_reference: after sc_reset the frames below the stale table's extent are not re-projected (scorers.py:342-350)
 * and therefore not scanned - n_frames counts the frames behind them, the track keeps the stale utterance's values
 * there. */
int sc_streams_set_activity(sc_streams *streams, int on, double blank_threshold);
/* state of the stream's last REPORTED chunk - the chunk whose hypotheses sc_get_hyps returns - over every frame the
 * encoder had emitted for the utterance when that chunk was admitted (a chunk that emits no frame carries its
 * predecessor's state), however many chunks are queued behind it; (0, 0, 0, -1, -1, 0) after sc_reset.  Waits for the
 * encoder group of that chunk if it is still in flight.  SC_ERR_ARG when the option is off. */
int sc_stream_activity(sc_streams *streams, int stream, sc_activity_t *out /*HOST*/);
/* the p_blank track of the frames that state covers -> host [min(frames, max_frames)] doubles (index = row of the CTC
 * table); returns the number written */
int sc_streams_read_activity(sc_streams *streams, int stream, double *host, int max_frames);
/* Phrase spotting per stream (off by default).  labels: host [n_phrases][SC_SPOT_MAX_LEN] (entries behind a
 * phrase's length are ignored), lens: host [n_phrases], min_scores: host [n_phrases] (each <= 0).  With a set in place
 * every admission group issues ONE sc_ctc_spot launch right behind its CTC projection, on the encoder stream, over the
 * CTC rows [c0, t1) each of its chunks projects (raw logits) - the search is not touched.  n_phrases == 0 switches the
 * option off: no path does any new work.  Everything is allocated when a set is first given.  SC_ERR_ARG while any chunk
 * is outstanding, for n_phrases outside [0, 64], a length outside [1, 32], a label outside the vocabulary or equal to
 * the blank, a min_score that is not <= 0.  A new set restarts every stream's state and enables every phrase for every
 * stream.  strict_reference: as for sc_streams_set_activity, frames that are not re-projected are not scanned. */
int sc_streams_set_phrases(sc_streams *streams, const int32_t *labels, const int32_t *lens, const double *min_scores,
                           int n_phrases);
/* bit p of mask: phrase p is enabled for the stream (default: all).  Takes effect with the next chunk admitted; a phrase
 * that is disabled keeps its states as they are.  SC_ERR_ARG when the option is off. */
int sc_stream_set_phrase_mask(sc_streams *streams, int stream, uint64_t mask);
/* counters of the stream's last REPORTED chunk - the chunk whose hypotheses sc_get_hyps returns - over every frame the
 * encoder had emitted for the utterance when that chunk was admitted; (0, 0) after sc_reset.  Waits for the encoder
 * group of that chunk if it is still in flight.  SC_ERR_ARG when the option is off. */
int sc_stream_spot(sc_streams *streams, int stream, sc_spot_t *out /*HOST*/);
/* the stored events that state covers, events [0, min(n_events, SC_SPOT_MAX_EVENTS, max)) of the utterance -> host;
 * returns the number written */
int sc_streams_read_spot_events(sc_streams *streams, int stream, sc_spot_event *host, int max);
/* test aid: the state block of a stream as the device holds it NOW (every group issued so far; waits for them) -> host
 * values [n_phrases][SC_SPOT_STATES], starts [n_phrases][SC_SPOT_STATES]; returns n_phrases */
int sc_streams_read_spot_state(sc_streams *streams, int stream, double *values, int32_t *starts);
/* Draft transcript per stream (off by default).  on != 0: every admission group issues ONE sc_ctc_draft
 * launch right behind its CTC projection (behind the activity and spotting launches where those are on), on the encoder
 * stream, over the CTC rows [c0, t1) each of its chunks projects (raw logits) - the search is not touched.  The state
 * (S x 32 bytes) and the token store (S x max_frames tokens: a frame opens at most one token, so it cannot overflow) are
 * allocated when the option is first switched on; off: no path does any new work.  SC_ERR_ARG while any chunk is
 * outstanding.  Switching it on restarts every stream's state.  sc_reset touches nothing on the device: the stream's next
 * span starts the utterance.  strict_reference: as for sc_streams_set_activity, frames that are not re-projected are not
 * scanned. */
int sc_streams_set_draft(sc_streams *streams, int on);
/* state of the stream's last REPORTED chunk - the chunk whose hypotheses sc_get_hyps returns - over every frame the
 * encoder had emitted for the utterance when that chunk was admitted; (0, 0, 0, -1, -1, -1, 0.0) after sc_reset.  Waits
 * for the encoder group of that chunk if it is still in flight.  SC_ERR_ARG when the option is off. */
int sc_stream_draft(sc_streams *streams, int stream, sc_draft_t *out /*HOST*/);
/* the draft of that state -> host: its stored tokens [0, min(n_closed, max)), then its open token, if any, where room
 * is left; returns the number written */
int sc_streams_read_draft(sc_streams *streams, int stream, sc_draft_token *host, int max);
/* CTC prefix beam search per stream (off by default).  beam >= 1: every admission group issues ONE
 * sc_ctc_beam launch with B = beam, C = candidates (both in [1, SC_BEAM_MAX]) right behind its CTC projection (behind the
 * activity, spotting and draft launches where those are on), on the encoder stream, over the CTC rows [c0, t1) each of its
 * chunks projects (raw logits) - the attention search is not touched.  The states (S x 528 bytes) and the node stores
 * (S x (1 + beam * max_frames) records: a frame adds at most `beam` nodes, so they cannot overflow) are allocated when the
 * option is first switched on, the stores again when `beam` grows; beam == 0 switches it off: no path does any new work.
 * SC_ERR_ARG while any chunk is outstanding.  Switching it on restarts every stream's state.  sc_reset touches nothing on
 * the device: the stream's next span starts the utterance.  strict_reference: as for sc_streams_set_activity, frames that
 * are not re-projected are not searched. */
int sc_streams_set_ctc_beam(sc_streams *streams, int beam, int candidates);
/* state of the stream's last REPORTED chunk over every frame the encoder had emitted for the utterance when that chunk
 * was admitted; the initial state after sc_reset.  Waits for the encoder group of that chunk if it is still in flight.
 * SC_ERR_ARG when the option is off. */
int sc_stream_ctc_beam(sc_streams *streams, int stream, sc_beam_t *out /*HOST*/);
/* the first nbest <= SC_BEAM_MAX entries of those states as token sequences, for n listed streams (each at most once) with
 * ONE sc_ctc_beam_pack launch and ONE copy back: header [n][nbest][4] (len, SC_BEAM_PACK_* status, node, last), ids /
 * frames [n][nbest][max_len] (the tokens and the frames of their first emission; only [0, min(len, max_len)) of a row is
 * written), scores [n][nbest][2] (pb, pnb).  ids, frames and scores may be NULL. */
int sc_ctc_beam_hyps(sc_streams *streams, const int *stream_ids, int n, int nbest, int max_len, int32_t *header /*HOST*/,
                     int32_t *ids /*HOST*/, int32_t *frames /*HOST*/, double *scores /*HOST*/);
/* An n-gram model fused into the beam of every stream (off by default).  Needs the beam option on.  With a
 * model attached the group launches sc_ctc_beam_lm in the place of sc_ctc_beam (the same launch slot, the same hand-over;
 * the state grows by a sc_beam_lm_t per stream, S x 192 bytes, allocated when a model is first attached); with lm == NULL
 * it launches sc_ctc_beam as before and nothing new.  One model serves all streams of the handle; the model's V must be the
 * batch's vocabulary size, alpha and beta finite.  SC_ERR_ARG while any chunk is outstanding; attaching, replacing or
 * detaching restarts every stream's beam (waiting for a group in flight first: the model may be destroyed once it is
 * detached, and switching the beam option off detaches it).  sc_reset and strict_reference: as sc_streams_set_ctc_beam.
 * Hypotheses of FULL streams do not depend on it.  SC_ERR_ARG while any stream has a grammar (sc_stream_set_grammar): grammar
 * and model together are not served.  Not in this revision: a model per stream, an end-of-sentence term at
 * finals, fusion into the blockwise search of FULL streams. */
int sc_streams_set_ctc_beam_lm(sc_streams *streams, const sc_lm *lm, double alpha, double beta);
/* beside sc_stream_ctc_beam: the model's side of the same state ((0.0, start_state) in entry 0 before the first frame).
 * SC_ERR_ARG when no model is attached. */
int sc_stream_ctc_beam_lm(sc_streams *streams, int stream, sc_beam_lm_t *out /*HOST*/);
/* beside sc_ctc_beam_hyps' scores: lm [n][nbest] and fused [n][nbest] = lae(pb, pnb) + (alpha * lm + beta * len) of the
 * same entries, NaN where a state has no such entry; computed on the host from the reported states, no launch.  Either
 * may be NULL.  SC_ERR_ARG when no model is attached. */
int sc_ctc_beam_hyps_lm(sc_streams *streams, const int *stream_ids, int n, int nbest, double *lm /*HOST*/,
                        double *fused /*HOST*/);
/* A grammar per stream (sc_ctc_beam_grammar above): the stream's beam answers only from the grammar.  Needs
 * the beam option on; NULL: none.  A menu belongs to a stream, not to the handle: streams of one handle may name different
 * grammars, the same one, or none.  A group lists the jobs of its streams without a grammar in its sc_ctc_beam launch, as
 * always, and those of its streams with one in ONE sc_ctc_beam_grammar launch behind it (the same hand-over; the state
 * grows by a sc_beam_gr_t per stream, S x 64 bytes, allocated when a grammar is first set on the handle); either launch is
 * skipped when its list is empty, and a handle on which no stream has a grammar issues the launches it always did.  The
 * rule of sc_stream_set_decoder: SC_ERR_ARG unless the stream is idle and has taken nothing of its utterance.  The setting
 * outlives sc_reset; switching the beam option off drops every stream's grammar.  The handle holds one use of the grammar
 * while a stream names it: sc_grammar_destroy returns SC_ERR_ARG meanwhile.  It works for SC_DECODER_FULL and
 * SC_DECODER_NONE streams alike; for a FULL stream the beam is a side result and its hypotheses do not depend on it.
 * Grammar and n-gram model together are not served in this revision: SC_ERR_ARG here while a model is attached to the
 * handle, and from sc_streams_set_ctc_beam_lm while any stream has a grammar.  The grammar's V and blank must be the
 * batch's. */
int sc_stream_set_grammar(sc_streams *streams, int stream, sc_grammar *grammar /*NULL: none*/);
/* beside sc_stream_ctc_beam: the grammar's side of the same state (start_state in entry 0 before the first frame), with
 * the same waiting rule.  SC_ERR_ARG when the stream has no grammar. */
int sc_stream_ctc_beam_grammar(sc_streams *streams, int stream, sc_beam_gr_t *out /*HOST*/);
/* beside sc_ctc_beam_hyps: g [n][nbest], the grammar's state after each of the same entries, and accept [n][nbest], its
 * accept flag (1: the entry is a complete phrase, or a sequence of them under a looped grammar); -1 where a state has no
 * such entry or the stream has no grammar.  Computed on the host from the reported states and the grammar's host copy, no
 * launch.  Either may be NULL. */
int sc_ctc_beam_hyps_grammar(sc_streams *streams, const int *stream_ids, int n, int nbest, int32_t *g /*HOST*/,
                             int32_t *accept /*HOST*/);
/* Decoder-free streams.  SC_DECODER_NONE: the stream is served from its CTC rows alone.  Admission queues
 * no decode block for it and lists no cross-attention K|V rows for its frames; the front end, the encoder, the CTC rows,
 * every side option and the reply status are those of any stream, a chunk is complete at once (the side-state readers
 * wait for its encoder group), sc_get_hyps returns the initial hypothesis and sc_stream_info.decode_steps stays 0.  The
 * other streams of the batch are not touched: the same launches for them, the same bits.  The mode outlives sc_reset.
 * SC_ERR_ARG unless the stream is idle and has taken nothing of its utterance (as for sc_stream_set_input_rate). */
#define SC_DECODER_FULL 0
#define SC_DECODER_NONE 1
int sc_stream_set_decoder(sc_streams *streams, int stream, int mode);
/* test aid: the CTC rows [0, min(rows projected, max_rows)) of the stream's utterance as the device holds them NOW (every
 * group issued so far; waits for them) -> host [.][vocab]; raw logits for a SC_DECODER_NONE stream, whose rows no decode
 * block touches.  Returns the number of rows. */
int sc_streams_read_ctc_projected(sc_streams *streams, int stream, float *host /*HOST*/, int max_rows);
/* the stream's decoder mode, SC_DECODER_*; SC_ERR_ARG for a null handle or a stream out of range */
int sc_stream_decoder(const sc_streams *streams, int stream);

#ifdef __cplusplus
}
#endif
#endif /* SCASR_H */
