/*
 * talkshow_hip.h — C ABI of the MI355X-native speech -> SMPL-X body-motion inference path.
 *
 * The reference (yhw-yhw/TalkSHOW) has no FFI: its boundary for this path is the Python surface of
 * package `nets`.  This header is what a host language binds underneath that surface;
 * our own `nets/` package (same names / signatures as the reference's) is the first client, through
 * ctypes (talkshow_amd/_lib.py).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; ts_last_error() gives the message
 *     (thread-local).  Nothing throws, nothing aborts.
 *   - "dev" pointers are HIP device pointers on the context's device; "host" pointers are CPU memory.
 *   - all activations are fp32, time-major / channel-last ("NLC"): x[b][t][c]; code indices are int64
 *     exactly as the reference's torch.int64 latents.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  Calls enqueue work
 *     and return; the caller synchronises (torch.cuda.synchronize() / hipStreamSynchronize).
 *   - weights are handed over ONCE as the reference's own state_dict (name, host pointer, shape); BatchNorm
 *     folding, mask-A zeroing, tap/segment packing and upload happen inside the library.
 *
 * Threads (the reference is single-threaded, default stream: SURVEY.md §8b)
 *   - ONE HOST THREAD PER STREAM AT A TIME.  Handles (ts_ctx, ts_convnet, ts_vqvae, ts_pixelcnn, ts_face, ts_mfcc, ts_smplx) hold
 *     read-only weights plus one scratch arena and one hipGraph cache PER STREAM; several host threads may call into the same
 *     handles concurrently as long as each thread uses its own stream (the per-stream maps are mutex-guarded; a stream's arena and
 *     graphs are only touched by the thread driving that stream).  Two threads on the same stream at the same time is a data race.
 *   - create / destroy / ts_face_set_arith / ts_prof_enable of a handle must not run concurrently with calls on that handle.
 *     ts_ctx_create and the create of ANY handle also belong ahead of the threads' first calls (or between them): they read weights back and
 *     probe the device with synchronous copies, which the HIP runtime refuses (hipErrorStreamCaptureImplicit) while any host thread
 *     captures a graph, whatever its capture mode, invalidating that capture.  Everything else — every pass, a session's open / step /
 *     push / flush / close, the first use of a resampling table — copies on a stream and waits for it, and may run beside captures.
 *   - ts_pixelcnn_stream and ts_body_stream sessions belong to the thread that steps them.  A session owns its state (row cache, sampler
 *     tables, graphs, tails and rings) and is bound to NO stream: every step / push / flush runs on the stream it is given, and independent
 *     sessions on different streams overlap like independent passes.  A session MAY CHANGE STREAMS between two calls once the caller has
 *     ordered them: everything the session queued on the earlier stream has completed (hipStreamSynchronize), or the later stream waits for
 *     it (hipStreamWaitEvent), before the first call on the later one.  Two calls of one session in flight on streams that are not ordered
 *     is a data race on the session's buffers; nothing detects it.  (The conv nets of a body session run on the per-stream arenas of the
 *     stream of each call; they keep nothing between calls.)
 *   - ts_last_error() is thread-local.  ts_stream_destroy(stream) drops that stream's arenas in every live handle: no call on the
 *     stream may be in progress.  A stream created afterwards may receive the same handle value; it starts from fresh arenas and graphs.
 *   - ts_pixelcnn_graph_stats is exact under concurrent callers: a capture counts what its own call issues (a thread-local tally), never
 *     the launches other threads make meanwhile.  The context-wide totals behind ts_prof_* count every thread's launches, as before.
 *   Exercised by tests/test_gpu_threads.py (three host threads, one stream each, bit-equal to the serial run) and tests/test_gpu_streams.py
 *   (every keyword of the mixed pass, sessions, growth beside replay, face / front end / SMPL-X / evaluation, one thread queueing on three
 *   streams, stream teardown, graph statistics: bit-equal to the serial run on the default stream, with evidence that the streams overlapped).
 */
#ifndef TALKSHOW_HIP_H
#define TALKSHOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ts_ctx ts_ctx;
typedef struct ts_convnet ts_convnet;     /* AudioEncoder            nets/spg/vqvae_1d.py:11-34          */
typedef struct ts_vqvae ts_vqvae;         /* VQVAE                   nets/spg/vqvae_1d.py:152-208        */
typedef struct ts_pixelcnn ts_pixelcnn;   /* GatedPixelCNN           nets/spg/gated_pixelcnn_v2.py:90-177 */
typedef struct ts_face ts_face;           /* s2g_face.Generator      nets/spg/s2g_face.py:142-224        */
typedef struct ts_mfcc ts_mfcc;
typedef struct ts_smplx ts_smplx;         /* smplx.SMPLX forward (third-party) scripts/demo.py:122-152, get_j.py */           /* get_mfcc_ta front-end   data_utils/utils.py:148-231         */

/* One entry of a reference state_dict: key name as the reference spells it (an optional "module." prefix is
 * accepted and stripped, nets/smplx_body_pixel.py:119-126), fp32 host data, shape.  int64 buffers
 * (num_batches_tracked) may be passed with data == NULL; they are ignored. */
typedef struct ts_tensor {
    const char *name;
    const float *data;
    int32_t ndim;
    int64_t shape[4];
} ts_tensor;

/* ---- context ------------------------------------------------------------------------------------------ */
int ts_ctx_create(int device, ts_ctx **out);
void ts_ctx_destroy(ts_ctx *ctx);
const char *ts_last_error(void);
/* library / build identification, e.g. "talkshow_hip 0.1 gfx950" */
const char *ts_version(void);
/* Non-blocking HIP streams for keeping several independent batches in flight on one GPU (the library keeps one
 * scratch arena per stream; weights are shared).  *out is a hipStream_t. */
int ts_stream_create(ts_ctx *ctx, void **out);
int ts_stream_destroy(ts_ctx *ctx, void *stream);

/* ---- AudioEncoder(in_dim=64, num_hiddens, num_residual_layers, ·)  — vqvae_1d.py:11-34 ------------------ */
int ts_audioenc_create(ts_ctx *ctx, const ts_tensor *sd, int n, int in_dim, int num_hiddens,
                       int num_residual_layers, ts_convnet **out);
void ts_convnet_destroy(ts_convnet *net);
/* AudioEncoder.forward (vqvae_1d.py:27-34): mfcc_dev (B,T,in_dim) -> feat_dev (B,H,num_hiddens), H = T//4
 * (two k4/s2/p1 convolutions: L -> floor(L/2)). */
int ts_audioenc_forward(ts_convnet *net, const float *mfcc_dev, int B, int T, float *feat_dev, void *stream);

/* ---- VQVAE(in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers, ·) — vqvae_1d.py:152 --
 * num_embeddings == 0 builds the quantiser-free auto-encoder `vqvae_1d.AE` (vqvae_1d.py:211-235), the FGD feature
 * extractor of nets/body_ae.py: same Encoder / Decoder, no vq_layer keys; its checkpoint's unused frame_enc / GRU
 * entries (Decoder(ae=True), never touched by forward) are accepted and ignored. */
int ts_vqvae_create(ts_ctx *ctx, const ts_tensor *sd, int n, int in_dim, int embedding_dim, int num_embeddings,
                    int num_hiddens, int num_residual_layers, ts_vqvae **out);
void ts_vqvae_destroy(ts_vqvae *vq);
/* VQVAE.encode (vqvae_1d.py:196-199) + VectorQuantizerEMA eval branch (vqvae_modules.py:274-286,311-323):
 * poses_dev (B,T,in_dim) -> z_dev (B,H,embedding_dim) [may be NULL], latents_dev (B,H) int64,
 * quantized_dev (B,H,embedding_dim) [may be NULL].  For an auto-encoder handle (num_embeddings == 0) this is
 * AE.encode (vqvae_1d.py:233-235): z_dev is required, the other two outputs must be NULL. */
int ts_vqvae_encode(ts_vqvae *vq, const float *poses_dev, int B, int T, float *z_dev, int64_t *latents_dev,
                    float *quantized_dev, void *stream);
/* VQVAE.decode(latents=...) (vqvae_1d.py:201-208): latents_dev (B,H) int64 -> recon written into
 * out_dev[b][t][out_col0 + c], c < in_dim, row stride out_ld floats (so body and hand decoders can write
 * the two halves of one (B,4H,129) buffer — the torch.cat of smplx_body_pixel.py:285). */
int ts_vqvae_decode(ts_vqvae *vq, const int64_t *latents_dev, int B, int H, float *out_dev, int out_ld,
                    int out_col0, void *stream);
/* Decoder.forward on CONTINUOUS latents (AE.forward eval branch, vqvae_1d.py:225-229; also VQVAE.decode(e=...)):
 * z_dev (B,H,embedding_dim) -> recon, same output addressing as ts_vqvae_decode. */
int ts_vqvae_decode_z(ts_vqvae *vq, const float *z_dev, int B, int H, float *out_dev, int out_ld, int out_col0,
                      void *stream);
/* body + hand decode in lockstep into one (B,4H,body_dim+hand_dim) buffer (the two decode calls + torch.cat of
 * smplx_body_pixel.py:282-285). */
int ts_vqvae_decode_pair(ts_vqvae *vq_body, ts_vqvae *vq_hand, const int64_t *lat_body_dev, const int64_t *lat_hand_dev,
                         int B, int H, float *out_dev, void *stream);
/* VQVAE.forward, eval branch (vqvae_1d.py:184-189): encode -> quantise -> decode in one call. */
int ts_vqvae_forward(ts_vqvae *vq, const float *poses_dev, int B, int T, int64_t *latents_dev, float *out_dev,
                     int out_ld, int out_col0, void *stream);

/* ---- GatedPixelCNN(input_dim, dim, n_layers, n_classes, audio=True, bh_model=True) ---------------------- */
int ts_pixelcnn_create(ts_ctx *ctx, const ts_tensor *sd, int n, int input_dim, int dim, int n_layers,
                       int n_classes, int aud_dim, ts_pixelcnn **out);
void ts_pixelcnn_destroy(ts_pixelcnn *pix);

#define TS_SAMPLE_GREEDY 0      /* argmax(logits), ties -> lowest index (the harness of SURVEY.md §0.3)           */
#define TS_SAMPLE_UNIFORMS 1    /* inverse-CDF draw from softmax(logits) with caller-supplied uniforms (B,H,2)    */
#define TS_SAMPLE_PHILOX 2      /* same draw, uniforms from Philox4x32-10(seed; clip index, position)             */
#define TS_TEACHER_FORCED 3     /* do not sample: positions are read from codes_dev (GatedPixelCNN.forward)       */

/* GatedPixelCNN.generate (gated_pixelcnn_v2.py:152-177), computed incrementally (row cache) instead of the
 * reference's full-grid recompute per position; same arithmetic per position.
 *   label_dev (B,) int64 speaker class; aud_dev (B,H,aud_dim) per-row audio features (the reference's
 *   (B,aud_dim,H,2) tensor is this repeated over the 2 columns, smplx_body_pixel.py:274);
 *   codes_dev (B,H,2) int64: output (input when mode == TS_TEACHER_FORCED);
 *   uniforms_dev (B,H,2) fp32 for TS_SAMPLE_UNIFORMS else NULL; seed / clip_index0 for TS_SAMPLE_PHILOX
 *   (clip b draws from subsequence clip_index0 + b, so results do not depend on how clips are sharded);
 *   logits_dev optional (B,H,2,input_dim) fp32: logits of every position as the reference's forward gives them.
 *   pre_codes_dev / pre_aud_dev / H0: optional continuity prefix (gated_pixelcnn_v2.py:158-165): H0 rows of
 *   already generated codes (B,H0,2) and their audio features (B,H0,aud_dim); pass NULL, NULL, 0 otherwise.
 *   Philox position rule (since round 3): the counter word of a code is its ABSOLUTE grid position (row * 2 + column) with
 *   the prefix rows counted — the first generated row of a call with H0 prefix rows draws at positions 2 H0, 2 H0 + 1 — so a
 *   clip generated as head + prefix-continued tail (or in ts_pixelcnn_stream_step chunks) draws exactly what one call over
 *   all its rows draws.  (Rounds 1-2 restarted at position 0 behind a prefix: sampled codes of H0 > 0 calls differ from those
 *   builds for the same seed.)  uniforms_dev always holds the H GENERATED rows only, (B,H,2). */
int ts_pixelcnn_generate(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, int B, int H, int mode,
                         const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                         float *logits_dev, const int64_t *pre_codes_dev, const float *pre_aud_dev, int H0,
                         void *stream);

/* hipGraph policy of ts_pixelcnn_generate / ts_body_pixel_infer (no counterpart in the reference, which launches eagerly): a one-shot
 * call (H0 == 0) replays graphs captured per (stream, B, H, mode).  A shape runs on small length-independent CHUNK graphs (8 code rows
 * each) until it is hot — its third sighting among the last 16 one-shot calls on the stream — and then gets one whole-call graph; at
 * most 24 unpinned graphs per stream are kept (8 whole-call + 16 chunk / streaming-step graphs), least recently used of its class out
 * first, destroyed behind an event (no host-side wait).  A serving host
 * that knows its pass shapes calls ts_pixelcnn_prepare once per (stream, shape): the whole-call graph is captured there (nothing
 * runs), pinned (never evicted; at most 12 per stream) and the first real call is already one replay.
 * Mixed passes (ts_body_pixel_infer_mixed) run on chunk graphs only, keyed by (active clips, rows, phase, mode, clips of the pass): at most
 * 12 distinct active clip counts per pass, more are rounded UP to multiples of 2, 4, 8, ... — the rule is stated at that entry. */
int ts_pixelcnn_prepare(ts_pixelcnn *pix, int B, int H, int mode, void *stream);
/* hipGraphs captured + instantiated on `stream` since the handle was created, or -1 (a serving loop checks that this stands still
 * once it is warm; bench.py asserts it over its timed regions). */
long ts_pixelcnn_graph_captures(ts_pixelcnn *pix, void *stream);

/* ---- per-clip sampling controls: temperature, top-k, top-p (nucleus) ------------------------------------------------------------------
 * No counterpart in the reference, which draws from the raw distribution (softmax + multinomial(1), gated_pixelcnn_v2.py:173-176).  One
 * record per clip; a draw is a pure, bit-reproducible function of the clip's logits row, the clip's record and the clip's uniform. */
typedef struct ts_sampling {
    float temperature;   /* finite, > 0, and 1.0f / temperature finite                                */
    float top_p;         /* 0 < top_p <= 1; 1 = off                                                    */
    int32_t top_k;       /* >= 0; 0 or any value >= V = off                                            */
    int32_t reserved;    /* 0                                                                          */
} ts_sampling;
/* neutral: {1.0f, 1.0f, 0, 0}.
 *
 * THE RULE, for a row l[0..V) with record (T, k, p) and uniform u (talkshow_amd/sampling.py restates it in numpy, operation for operation):
 *  1. Weights.  m = max l;  d_v = (l_v - m) * inv_T as TWO fp32 operations (subtract, then multiply; never fused), inv_T = 1.0f / T computed
 *     once on the host in fp32;  w_v = det_expf(d_v), the sampler's exponential (fp32 multiplies and adds only; 0 below -86).  At T = 1 the
 *     multiplication is exact and w_v has the bits of the sampler without controls.
 *  2. Rank.  Tokens are ranked by l_v descending (-0 equal to +0), ties by index ascending.  Exact; independent of T.
 *  3. Top-k.  If 1 <= k < V: keep ranks < k.
 *  4. Top-p, after top-k, on the mass top-k kept.  MASSES ARE INTEGERS: q_v = floor(w_v * 2^31) (exact product, truncating cast), summed as
 *     64-bit integers — an order-free accumulation, so no result depends on thread timing (no floating-point atomics exist in the library).
 *     Q = sum of q over the ranks top-k kept (all ranks when top-k is off);  M(i) = sum of q over ranks < i.  If p < 1: keep rank i iff
 *     i == 0 or M(i) < ceil(fl64((double)p * (double)Q)): both factors are exact in fp64, their product is ONE IEEE fp64 multiplication,
 *     rounded to nearest (p has 24 significant bits, Q up to 44: the exact product need not fit 53), then ceil; integers from there on.
 *     V <= 8191 keeps every sum below 2^44, the width the device gives a mass: a larger vocabulary is refused by every entry.
 *     Error of the quantisation against the real masses: < 2^-31 per token, < V * 2^-31 (9.6e-7 at V = 2048) of the largest weight (= 1).
 *  5. Draw.  The inverse CDF of the sampler without controls, in INDEX order with its summation structure, over w'_v = kept ? w_v : 0 in
 *     fp32: 256 contiguous chunks of ceil(V / 256) tokens summed left to right, the chunk sums prefix-summed left to right (pre[0] = 0),
 *     thr = u * total; the owning chunk t has pre[t] <= thr and (thr < pre[t+1] or t == 255); the draw is the first token of chunk t at
 *     which the running sum pre[t] + w'.. exceeds thr (a dropped token adds nothing and is never returned).  If no running sum of the
 *     chunk exceeds thr: the chunk's highest-index kept token when thr < pre[t+1]; otherwise (thr >= total: u = 1 - 2^-24) the row's
 *     highest-index kept token.  For a neutral record these are V - 1 and the chunk's last token: exactly what the sampler without
 *     controls returns.  u comes from uniforms_dev, or from Philox with the same key and counter as without controls: a clip's
 *     uniform does not depend on its record.
 * Consequences (tests/test_gpu_sampling_ops.py, test_gpu_sampling_pass.py): a neutral record draws bit for bit what the sampler without
 * controls draws; top_k = 1 is the argmax with lowest-index ties for every u; a clip's codes depend on its own record only.
 *
 * Graphs: the key of a captured graph has one "controls" field.  Passes without a table find and replay exactly the graphs they always did; a
 * pass with a table captures its own chunk (or whole-call) graphs once, and a repeated pass — with the same or another table: the table
 * travels to the stream's work buffers as kernel arguments ahead of the replay, no host memory is read after the call returns, nothing
 * synchronises, any number of calls may be queued — captures nothing.  BUDGET: a host that alternates passes with and without a table on
 * one stream shares the 16 chunk graphs (and the 8 whole-call graphs) kept per stream between the two kinds.
 * The streaming sessions take a table per step (ts_pixelcnn_stream_step_ctl, "streaming sessions" below: the records hold for that step
 * only).  Out of scope: ts_pixelcnn_v_*, the face generator.  (A STATIC per-clip bias on the codes,
 * allow-lists and bans included, is in scope: "code bias" below; so is a windowed penalty on the codes a clip has already produced:
 * "repetition penalty" below.)  Log-probabilities (below) share the scope: a session's step returns those of its own rows, ts_pixelcnn_v_* and the face
 * generator return none, a session does not SCORE given codes (its given rows apart), clips of different lengths are not SCORED in one pass, and scoring runs the rows one after the other as the decode does (given
 * the codes, teacher-forced rows do not depend on each other and could run as large GEMMs: other work, with other bits). */
/* Host only: the validation every _ctl entry applies before anything is launched.  n records for vocabulary V, 1 <= V <= 8191 (a larger V
 * is an error: see step 4); 0, or an error whose message names the clip: temperature not finite / <= 0 / with an infinite fp32 reciprocal, top_p outside (0, 1], top_k < 0, reserved != 0.
 * (The entries also refuse a table with TS_SAMPLE_GREEDY or TS_TEACHER_FORCED: per-clip greedy is top_k = 1.) */
int ts_sampling_check(const ts_sampling *ctl_host, int n, int V);
/* ts_pixelcnn_generate with a table: its arguments plus ctl_host (n_ctl records: 1 = one for all clips, or B); prefix and logits_dev as
 * there.  ctl_host == NULL: exactly ts_pixelcnn_generate. */
int ts_pixelcnn_generate_ctl(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, int B, int H, int mode,
                             const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev, float *logits_dev,
                             const int64_t *pre_codes_dev, const float *pre_aud_dev, int H0, const ts_sampling *ctl_host, int n_ctl,
                             void *stream);

/* ---- log-probabilities: how likely was that code? ---------------------------------------------------------------------------------------
 * The sampler launch already holds the row maximum, the 256 chunk sums, their total and the chosen index; the _lp entries also return
 *
 *     logprob = (float)( (double)d_c - log((double)S) )          one fp64 log per position, one rounding to fp32
 *
 * for the chosen (greedy, drawn) or given (teacher forced) code c, where
 *   m    the row maximum;
 *   d_c  the fp32 value the sampler feeds to det_expf for c: l_c - m without controls; (l_c - m) * inv_T, two fp32 operations, with a record;
 *   S    the fp32 total of the distribution the draw is made from, with the samplers' summation structure (256 contiguous chunks summed
 *        left to right, then the chunk sums added left to right); with a record, the total over the kept weights w' of step 5.
 * talkshow_amd/sampling.py::logprob restates it in numpy, operation for operation.  Consequences (tests/test_gpu_logprob_ops.py):
 *   - it is the log-probability under the distribution the draw was made from: with temperature and filtering when there is a record, the
 *     raw model distribution when there is no table, in greedy mode and in teacher-forced mode;
 *   - a neutral record gives the bits of the path without a table;
 *   - top_k = 1 gives exactly 0.0f (S = det_expf(0) = 1, d_c = 0; in a row whose maximum is attained by +0 and by -0 the zero may carry
 *     either sign: it is the sign of l_c - m);
 *   - a row whose other weights underflow gives 0.0f for the maximum and the finite d_c for any other code: d_c is used, never log(w_c);
 *   - there are no clamps;
 *   - the logit of c is picked up by the thread that owns index c; the code is never used as an address: a teacher-forced code outside
 *     [0, V) yields NaN for that position and reads nothing out of bounds.
 * It is a pure function of the clip's own logits row (and record): bit-identical alone or inside a mixed pass of any size, eager or replayed.
 * Accuracy.  (a) Device against the numpy restatement: S and d_c are bit-equal; the two fp64 logs may differ in the last place, so the
 * results are equal or adjacent fp32 values (the tests allow one fp32 spacing and no more).  (b) Restatement against an exact float64
 * log-softmax of the fp32 logits, without a record (sampling.py::logprob_error_bound, asserted by tests/test_logprob_host.py):
 *   |d_c| 2^-24 for the subtraction;  on S, relatively: (chunk - 1 + 255) 2^-24 for its fp32 additions (262 at V = 2048), det_expf's
 *   relative error — at most 8.11e-8 = 1.36 * 2^-24 against float64 exp on 2^26 + 1 evenly spaced arguments of [-86, 0] (the bit-exact numpy
 *   twin on a CPU; arguments in [-87, -86) give 0), bounded by 2^-23 in the tests — plus 86 * 2^-24 for the rounding of a weight's argument
 *   and V e^-86 for the dropped weights;  |logprob| 2^-24 for the final rounding.  At V = 2048: 2.1e-5 + (|d_c| + |logprob|) 6e-8.
 * Graphs: the sixth key field is a bit set, bit 0 = controls, bit 1 = log-probabilities.  Passes without either keep their keys, replay the
 * graphs they had and issue the launches they always did; a pass with log-probabilities captures its own graphs once (the samplers write
 * a staging buffer of the stream's work buffers, copied to logprob_dev behind the replay as the codes are) and a repeated one captures
 * nothing.  Teacher forced WITH a log-probability output runs the horizontal stack (eager launches, as teacher forced always does);
 * without one it stays the vertical-stack-only pass it was.
 *
 * ts_pixelcnn_generate_ctl's arguments plus logprob_dev (B,H,2) fp32: the prefix is allowed, the log-probabilities cover the H generated
 * (teacher forced: given) rows only.  ctl_host may be NULL (no table); a table with TS_TEACHER_FORCED or TS_SAMPLE_GREEDY stays refused.
 * logprob_dev == NULL: exactly ts_pixelcnn_generate_ctl. */
int ts_pixelcnn_generate_lp(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, int B, int H, int mode,
                            const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev, float *logits_dev,
                            const int64_t *pre_codes_dev, const float *pre_aud_dev, int H0, const ts_sampling *ctl_host, int n_ctl,
                            float *logprob_dev, void *stream);
/* Per-clip fixed-order float64 sums of a pass's log-probabilities: logprob_dev (B,H,2) -> sums_dev (B,3) = {body column, hand column,
 * body + hand}.  lens_dev: the table of the mixed pass that wrote them ((B,) int32 MFCC frames, H_b = lens[b] >> 2, capped at H), or NULL
 * for H rows per clip; rows at or beyond H_b do not enter.  Two stages: lane t of 256 adds rows t, t + 256, ... of a column in ascending
 * order, the 256 lane sums are added in ascending order; the third value is one addition of the first two.
 * talkshow_amd/sampling.py::logprob_sums equals it bit for bit. */
int ts_logprob_sums(ts_ctx *ctx, const float *logprob_dev, const int32_t *lens_dev, int B, int H, double *sums_dev, void *stream);

/* GatedPixelCNN(input_dim, dim, n_layers, n_classes, audio, bh_model=False) — the single-stack form (gated_pixelcnn_v2.py:37-42,
 * 80-85,147-150): vertical kernels one column wide, out_v = horiz_resid(gate(vert_stack(x_v) + class)) [+ x_v], logits from x_v; the
 * grid's W columns never mix, so the W codes of a row are drawn together.  Same state_dict keys as the reference module (the
 * vert_to_horiz / horiz_stack / fusion_h tensors it also holds are not read).  audio != 0: embedding_aud + fusion_v in front of
 * layer 1.  Not used by config/body_pixel.json; eager launches, no tuning. */
typedef struct ts_pixelcnn_v ts_pixelcnn_v;
int ts_pixelcnn_v_create(ts_ctx *ctx, const ts_tensor *sd, int n, int input_dim, int dim, int n_layers, int n_classes, int audio,
                         int aud_dim, ts_pixelcnn_v **out);
void ts_pixelcnn_v_destroy(ts_pixelcnn_v *pix);
/* generate / forward of that form: label_dev (B,), aud_dev (B,H,aud_dim) or NULL (audio == 0) — ONE audio row per code row: the
 * reference's (B, aud_dim, H, W) map with all W columns equal, as its caller builds it (smplx_body_pixel.py:274); a map whose columns
 * differ has no counterpart here (the Python layer raises NotImplementedError instead of dropping columns) —, grid (H, W) with W a power of two;
 * codes_dev (B,H,W) int64 out (in for TS_TEACHER_FORCED), logits_dev optional (B,H,W,input_dim), uniforms_dev (B,H,W) for
 * TS_SAMPLE_UNIFORMS; Philox position of (row, column) = (H0 + row) * W + column; prefix as in ts_pixelcnn_generate
 * (pre_codes_dev (B,H0,W), pre_aud_dev (B,H0,aud_dim)). */
int ts_pixelcnn_v_generate(ts_pixelcnn_v *pix, const int64_t *label_dev, const float *aud_dev, int B, int H, int W, int mode,
                           const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev, float *logits_dev,
                           const int64_t *pre_codes_dev, const float *pre_aud_dev, int H0, void *stream);

/* Launch count and algorithmic flops (2*M*N*K over every skinny_gemm launch) of the hipGraph captured for
 * (B, H, mode) on `stream` — what one replay executes; used by bench.py for the roofline line. */
int ts_pixelcnn_graph_stats(ts_pixelcnn *pix, void *stream, int B, int H, int mode, int64_t *launches, double *flops);

/* ---- s2g_face.Generator over the wav2vec2-base encoder (nets/spg/s2g_face.py:142-224, nets/spg/wav2vec.py:73-143) ---- */
/* state_dict of the reference Generator (keys "audio_encoder.*", "audio_feature_map.*", "audio_middle.*", "decoder.*",
 * "final_out.*"; the positional conv's weight norm is accepted under both the transformers>=4.3x names
 * "...conv.parametrizations.weight.original0/1" and the 4.22-era "...conv.weight_g/_v"). */
/* num_classes == 0 builds Generator(identity=False) (what smplx_face.py:37-45 constructs when convert_to_6d is set): no id_mlp keys,
 * first_net over the 256 audio channels alone, a 6-wide jaw head -> ts_face_generate writes (B,frames,106) and ignores id_dev. */
int ts_face_create(ts_ctx *ctx, const ts_tensor *sd, int n, int n_layers, int num_classes, ts_face **out);
void ts_face_destroy(ts_face *face);
/* Generator.forward, eval (s2g_face.py:196-224; TrainWrapper.generate / infer_on_audio, smplx_face.py:169-238):
 * wav_dev (B,N) fp32 16 kHz samples, id_dev (B,num_classes) fp32 one-hot or all-zero (smplx_face.py:205-208),
 * frames = N*30//16000 normally -> out_dev (B,frames,103) = [jaw(3) | expression(100)];
 * hidden_dev optional (B,frames,768): the wav2vec2 last_hidden_state (parity tests). */
int ts_face_generate(ts_face *face, const float *wav_dev, int B, int N, int frames, const float *id_dev, float *out_dev,
                     float *hidden_dev, void *stream);
/* ---- mixed face passes: clips of DIFFERENT lengths in one pass (no counterpart in the reference, which runs one recording at a time) ------
 * B clips, clip b with ns[b] 16 kHz samples and frames[b] output frames, stored padded to N_max samples and written padded to T_max frames;
 * the arithmetic of ts_face_generate on every clip.  Rows t < frames[b] of clip b are BIT-IDENTICAL whatever else is in the pass — the clip
 * alone in a mixed pass of one included — and bit-identical to ts_face_generate on the clip alone (B = 1, N = ns[b], frames = frames[b]) in a
 * process that runs without the stream-K band (TS_CONV_SK=0): no GEMM of a mixed pass takes the band, every kernel that looks across rows
 * (GroupNorm statistics, interpolation, positional and k = 3 convolutions, attention) stops at the clip's own length, and the rows beyond it
 * hold the zeros a clip run alone reads past its end.  This is the batch-invariant face entry: ts_face_generate's bits depend, by default,
 * on the batch a clip rides in (to rounding only).  Clips need no particular order.
 *   ns_host / ns_dev, frames_host / frames_dev (B,) int32: the same tables in host memory (checked and planned from without synchronising;
 *     not read after the call returns) and in device memory.  400 <= ns[b] <= N_max, 1 <= frames[b] <= T_max <= 65536 (frames[b] =
 *     ns[b] * 30 / 16000 normally); anything else, or a NULL table, is an error and nothing is written.
 *   wav_dev (B,N_max): samples at or beyond ns[b] are never read (they may hold anything, NaNs included).
 *   id_dev (B,num_classes) as for ts_face_generate.
 *   out_dev (B,T_max,103 | 106): rows t < frames[b] = the clip's output, rows t >= frames[b] are written as 0.
 *   hidden_dev optional (B,T_max,768): the same rule.  Every element of both outputs is written, nothing else is touched.
 * The opt-in split-bf16 plans (ts_face_set_arith 3 / 6) are not offered: an error.  The call allocates nothing beyond the growth of the stream's
 * work buffers and never synchronises; the attention work list and the row tables travel to the device in kernel arguments, in stream order.
 * Cost: every stage runs on B x longest rows, so clips of similar length make the cheaper pass.  TS_FACE_PACK=1 selects the packed plan, with
 * the same bits: the feature convolutions and the transformer layers (over nine tenths of the work) then run on the clips' OWN rows, packed back
 * to back — ts_face_mixed_rows gives both counts; the feature projection, the positional convolution and the heads stay on B x T_max rows. */
int ts_face_generate_mixed(ts_face *face, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_host,
                           const int32_t *frames_dev, int B, int N_max, int T_max, const float *id_dev, float *out_dev, float *hidden_dev,
                           void *stream);
/* Host only (no device, no handle): the rows a mixed pass of these clips computes, so that a host sizes its passes by real cost.  Same tables and
 * checks as ts_face_generate_mixed.  out4 = {feature rows padded = B ((N_max - 10) / 5 + 1), feature rows packed = sum over the clips of
 * (ns[b] - 10) / 5 + 1 rounded up to a multiple of 64, frames padded = B T_max, frames packed = sum of frames[b]}: the feature convolutions cost
 * in proportion to the second figure, the transformer layers to the fourth (attention: to the sum of frames[b]^2), the rest to the third. */
int ts_face_mixed_rows(const int32_t *ns_host, const int32_t *frames_host, int B, int N_max, int T_max, int64_t *out4);
/* OPT-IN arithmetic plan of the generator's GEMMs (no counterpart in the reference, which runs fp32 throughout): 0 = fp32 MFMA,
 * the default and the path every parity claim is made on; 3 / 6 = split-bf16: each fp32 operand becomes 2 / 3 bf16 terms and a
 * product 3 / 6 exact bf16 products accumulated in fp32 (csrc/conv_gemm_split.hip; measured error vs the reference golden in
 * DESIGN.md).  The first feature convolution, attention, LayerNorms and soft-max stay fp32.  Never applies to the body path.
 * The first selection of the 3-product plan also writes each layer's weights as bf16 plane images (one extra copy of the weights in HBM;
 * synchronises the device once). */
int ts_face_set_arith(ts_face *face, int bf16_products);

/* ---- audio front-end on the device: get_mfcc_ta (data_utils/utils.py:148-231) = torchaudio Resample(sr_in -> sr_out)
 * + MFCC(n_mfcc=64, n_fft=2048, n_mels=256, hop = 734 (fps 30) | 1467 (fps 15), mel_scale='htk').  torchaudio is
 * third-party and absent from the image: its published definitions are restated; parity against it is unpinned. ---- */
int ts_mfcc_create(ts_ctx *ctx, int sr_in, int sr_out, int fps, ts_mfcc **out);
void ts_mfcc_destroy(ts_mfcc *m);
/* frames for N input samples: floor(ceil(N * sr_out / sr_in) / hop) + 1 */
int ts_mfcc_num_frames(const ts_mfcc *m, long N);
/* wav_dev (B,N) mono fp32 at sr_in (multi-channel files: resample each channel, then average, as utils.py:150-154 —
 * resampling is linear, so averaging first is the same signal) -> feat_dev (B,T,64), T = ts_mfcc_num_frames(m, N). */
int ts_mfcc_forward(ts_mfcc *m, const float *wav_dev, int B, long N, float *feat_dev, void *stream);

/* ---- whole wrappers --------------------------------------------------------------------------------------- */
/* s2g_body_pixel.TrainWrapper.infer_on_audio after the MFCC front-end (smplx_body_pixel.py:272-285):
 * mfcc_dev (B,T,64), ids_dev (B,) int64 -> codes_dev (B,H,2) int64, poses_dev (B,4H,body_dim+hand_dim). */
int ts_body_pixel_infer(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand,
                        const float *mfcc_dev, const int64_t *ids_dev, int B, int T, int mode,
                        const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                        float *poses_dev, void *stream);
/* ---- mixed passes: clips of DIFFERENT lengths in one pass (no counterpart in the reference, whose loops run one clip at a time) ------
 * B clips, clip b with lens[b] MFCC rows, padded to T_max rows each; H_b = lens[b] / 4 code rows and 4 H_b pose frames, the arithmetic of
 * ts_body_pixel_infer.  A clip's codes and poses are BIT-IDENTICAL to what ts_body_pixel_infer gives for the clip alone (or in any other
 * pass): the conv stacks store zeros for every row beyond a clip's own length — the operand a clip run alone reads past its ends — and the
 * chain computes row r for the clips that have it.
 *   lens_host / lens_dev (B,) int32: the same table in host memory (planning never synchronises; not read after the call returns) and in
 *     device memory.  4 <= lens[b] <= T_max, NON-INCREASING (the active clips of a row are then a prefix of every buffer); anything else is
 *     an error.  The caller sorts (nets/smplx_body_pixel.py: generate_batches / generate_clips sort and un-sort).
 *   mfcc_dev (B,T_max,64): rows at or beyond lens[b] are never read (they may hold anything, NaNs included).
 *   uniforms_dev (B,H_max,2), H_max = T_max / 4, for TS_SAMPLE_UNIFORMS; rows at or beyond H_b are not read.
 *   clip_index_dev (B,) int64 or NULL: the Philox subsequence of every clip, in place of `clip_index0 + b` (sorting by length breaks
 *     that rule; with the table a clip's draws depend on its GLOBAL index only).  NULL: clip b draws from subsequence b.  Copied into
 *     the library's own buffer on the stream: graphs stay replayable and any number of calls may be queued.
 *   codes_dev (B,H_max,2): rows r < H_b = the clip's codes; rows r >= H_b are written as -1.
 *   poses_dev (B,4 H_max,body_dim+hand_dim): rows t < 4 H_b = the clip's poses; rows t >= 4 H_b are written as 0.
 *   Every element of both outputs is written, nothing else is touched.
 * Graph policy of a mixed pass: chunk graphs only (8 code rows each, as for first-time shapes of ts_pixelcnn_generate), keyed by (active
 * clips, rows, buffer phase, mode, clips of the pass).  A pass may use at most 12 DISTINCT active clip counts; one with more has every
 * count rounded UP to a multiple of 2, 4, 8, ... (the smallest power of two that fits; finished clips are carried along, which is always
 * correct), so that its graphs — one per count, one for the first chunk, one or two for a short last chunk — fit the 16 chunk graphs kept
 * per stream and a repeated pass captures nothing from its second run on (ts_pixelcnn_graph_captures stands still).  No whole-call graphs.
 * TS_TEACHER_FORCED and logits are not offered. */
int ts_body_pixel_infer_mixed(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                              const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                              const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                              float *poses_dev, void *stream);
/* The three stages of a mixed pass on their own (same table, same rules; lens are MFCC frame counts in all of them):
 * ts_audioenc_forward with length-masked layers: feat_dev (B,T_max/4,num_hiddens), rows at or beyond lens[b] / 4 written as 0; */
int ts_audioenc_forward_masked(ts_convnet *net, const float *mfcc_dev, const int32_t *lens_dev, int B, int T_max, float *feat_dev,
                               void *stream);
/* ts_pixelcnn_generate over a shrinking prefix of the clips: aud_dev (B,H_max,aud_dim), codes_dev (B,H_max,2) with -1 beyond lens[b] / 4; */
int ts_pixelcnn_generate_mixed(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                               const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                               const int64_t *clip_index_dev, int64_t *codes_dev, void *stream);
/* ts_body_pixel_infer_mixed / ts_pixelcnn_generate_mixed with per-clip sampling controls (ts_sampling above): their arguments plus ctl_host
 * (n_ctl records: 1 = one for all clips, or B, in the order of the submitted, SORTED clips — record b belongs to row b of every table of the
 * pass).  The records ride in the stream's work buffers, indexed by the clip's slot in the pass (the active clips are a prefix, so the slot
 * is the same in every chunk).  A clip's codes and poses are bit-identical to the clip run alone with its record.  ctl_host == NULL: exactly
 * the entry without the suffix.  A table needs TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX. */
int ts_body_pixel_infer_mixed_ctl(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                  const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                  const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                  float *poses_dev, const ts_sampling *ctl_host, int n_ctl, void *stream);
int ts_pixelcnn_generate_mixed_ctl(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                   const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                   const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl, void *stream);
/* The two entries above plus logprob_dev (B,H_max,2) fp32 ("log-probabilities" above; H_max = T_max / 4): a clip's values are bit-identical
 * to the clip run alone; rows at or beyond a clip's own H_b are written as 0.  ctl_host may be NULL.  The mixed entries stay sampling-only
 * (no teacher forcing).  logprob_dev == NULL: exactly the _ctl entry. */
int ts_body_pixel_infer_mixed_lp(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                 const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                 const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                 float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, void *stream);
int ts_pixelcnn_generate_mixed_lp(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                  const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                  const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                  float *logprob_dev, void *stream);
/* ---- given rows: continue each clip of a mixed pass from codes that already exist -------------------------------------------------------
 * The _lp entries plus, per clip, G_b GIVEN code rows, 0 <= G_b <= H_b = lens[b] / 4 (the reference's `infer(..., pre_latents, pre_audio)`
 * flow for a host that batches; keep a head and regenerate the tail; N tails for one head).  The audio is the clip's WHOLE audio, as in any
 * one-shot call.  Code rows r < G_b are TAKEN from the caller; rows G_b <= r < H_b are produced exactly as the pass produces them without
 * given rows (greedy, injected uniforms or Philox, with or without a sampling record).  codes_dev holds the given rows followed by the
 * produced rows, poses_dev the VQ decode of all H_b rows; rows at or beyond H_b are -1 / 0 as in every mixed pass.
 *   given_dev (B,H_max,2) int64: rows r < G_b of clip b are read, rows at or beyond G_b never are (they may hold anything);
 *   given_rows_host (B,) int32: G_b in the order of the submitted, SORTED clips like every other table of the pass.  It travels to the
 *     stream's work buffers as kernel arguments ahead of the first chunk: not read after the call returns, nothing synchronises, any number
 *     of calls — each with its own table and its own codes — may be queued.  G_b < 0 or G_b > lens[b] / 4 is an error, reported before
 *     anything is launched (ts_given_rows_check is that rule on its own);
 *   given_rows_dev (B,) int32 or NULL: the same table in device memory, for hosts that keep one beside lens_dev; the pass is planned and
 *     fed from the host copy and does not read it;
 *   uniforms_dev: the uniforms of rows below G_b are never read (they may hold anything, NaNs included).
 * THE RULE.  The sampler launch of position (r, j) — one workgroup per clip — is FORCED for clip slot b iff 2 r + j < 2 G_b, the position
 * being the Philox counter word of the launch.  A forced workgroup reads its code, writes it where a drawn code goes and draws nothing; an
 * unforced one runs the arithmetic of the sampler it stands in for.  Nothing else in the pass changes: a given row runs through the same
 * launches as a produced one (it costs what a produced row costs), so the row cache behind the prefix holds what a decode that DREW those
 * codes left there.  Consequences (tests/test_gpu_given_ops.py, test_gpu_given_pass.py):
 *   - values are pure: a clip's codes, poses and log-probabilities depend on the clip's own audio, id, given rows, record and random
 *     stream only — bit-identical alone or among any neighbours with other G, eager or replayed;
 *   - resume: given the first G_b rows of an earlier decode of the clip (same seed / clip index / record), the pass returns that decode bit
 *     for bit — a code's Philox position is its absolute (row, column), so the tail draws the numbers it drew then;
 *   - the produced rows equal what ts_pixelcnn_generate(..., pre_codes_dev, pre_aud_dev, H0 = G_b) returns for the clip alone on the same
 *     audio rows split at G_b.
 * Log-probabilities of given rows ("log-probabilities" above).  A given code c gets the log-probability of c under the distribution the row
 * would have been drawn from: (float)((double)d_c - log((double)S)) with the row's own m, d_c and S.  Without a record that is the value
 * teacher forcing (GatedPixelCNN.score) returns, bit for bit.  With a record, S is the total over the kept weights and a code the filters
 * REMOVED has weight w'_c = 0 in that distribution: its log-probability is log(0) = -inf (top_k = 1: 0.0f for the argmax, -inf for every
 * other code).  Kept codes get the bits a draw of them gets.  talkshow_amd/sampling.py::given_logprob restates it in numpy.
 * Bad codes.  A given code is compared, never used as an address.  One outside [0, V) inside a clip's prefix is copied to codes_dev as it
 * is, gets NaN as its log-probability, and enters the rows below it as a row of zeros in place of its embedding (its pose frames are the VQ
 * decoder's NaNs); nothing is addressed outside the buffers.  The Python layer refuses such a code on the host before anything is launched.
 * Graphs: bit 2 of the sixth key field.  In a pass with given rows EVERY chunk runs the given variants of the samplers, so its distinct keys
 * are what they are without given rows (at most 14 of the 16 chunk graphs); the given codes of a chunk travel into a staging block of the
 * work buffers ahead of its replay, for chunks with rows below max G_b only.  A repeated pass captures nothing, whatever its tables.
 * Passes without given rows find the keys, graphs and launches they found before.  given_dev == NULL: exactly the _lp entry.
 * Out of scope: rows inside every active clip's prefix still run the horizontal stack (the eager H0 path of ts_pixelcnn_generate skips
 * it); a streaming session takes given rows per step ("streaming sessions" below: the first g_b rows OF THE STEP); uniform lengths are the
 * special case of equal lens (no uniform entry). */
int ts_given_rows_check(const int32_t *given_rows_host, const int32_t *lens_host, int B);
int ts_body_pixel_infer_mixed_given(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                    const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                    const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                    float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                    const int32_t *given_rows_host, const int32_t *given_rows_dev, void *stream);
int ts_pixelcnn_generate_mixed_given(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                     const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                     const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                     float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                     const int32_t *given_rows_dev, void *stream);
/* ---- given poses: continue, resume and score from MOTION ---------------------------------------------------------------------------------
 * The entries of "given rows" start from codes; a host usually holds pose frames (the reference's `infer(..., pre_latents, pre_audio)` gets
 * pre_latents by encoding the poses of the previous window).  These entries encode the frames of many clips of DIFFERENT lengths in one pass
 * and hand the codes to the chain on the device: no synchronisation, no host copy of codes.
 *   poses_dev (B,P_max,ld) fp32, body columns [0, body_dim) and hand columns [body_dim, body_dim + hand_dim) of every row, as in
 *     ts_body_vq_infer; frames at or beyond a clip's own P_b are never read (they may hold anything, NaNs included);
 *   pose lens (B,) int32: P_b, the clip's own frame count, in ANY order (the encoders have no prefix structure).  The device table feeds the
 *     kernels; where a host table is taken too, it plans the pass and is not read after the call returns.
 * THE RULE.  Clip b has P_b / 4 code rows.  Every encoder layer is length-masked (ts_audioenc_forward_masked's scheme: whole-tile plans,
 * sk_ok = 0, no stream-K band), pre_vq_conv is masked at P_b / 4, and ONE kernel searches both codebooks: row h of clip b is valid iff
 * h < P_b / 4; a valid row gets exactly the index the uniform entries return for it (same arithmetic, operation for operation), an invalid
 * row gets -1 — the padding of every mixed pass — and its latent row is never read.  A clip's codes, latents and reconstruction are
 * bit-identical to ts_vqvae_encode / ts_body_vq_infer on the clip alone, whatever its neighbours and the padding hold.
 * ts_given_pose_rows_check is the host rule of a pass that CONTINUES from poses: P_b == 0 (nothing given), or P_b >= 4 with
 * P_b / 4 <= lens[b] / 4 (lens: the pass's MFCC frame counts); the clip then brings G_b = P_b / 4 given rows.  1 <= P_b <= 3 is an error (a
 * caller who hands over frames that cannot make one code row has miscounted), reported with the clip's index before anything is launched. */
/* VQVAE.encode of both parts, clips of different lengths: codes_dev (B,T_max/4,2) int64, -1 beyond a clip's rows; z_body_dev / z_hand_dev
 * (B,T_max/4,embedding_dim) or NULL: the encoders' outputs, 0 beyond a clip's rows.  T_max < 4 fails as the uniform encode does. */
int ts_vqvae_encode_pair_masked(ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *poses_dev, int poses_ld, const int32_t *lens_dev, int B,
                                int T_max, int64_t *codes_dev, float *z_body_dev, float *z_hand_dev, void *stream);
/* ts_body_vq_infer for clips of different lengths: poses_dev (B,T_max,body_dim+hand_dim) -> codes_dev (B,T_max/4,2) with -1 and recon_dev
 * (B,4 (T_max/4),body_dim+hand_dim) with 0 beyond a clip's rows (the encode above, then ts_vqvae_decode_pair_masked).  Either may be NULL. */
int ts_body_vq_infer_mixed(ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *poses_dev, const int32_t *lens_dev, int B, int T_max,
                           int64_t *codes_dev, float *recon_dev, void *stream);
int ts_given_pose_rows_check(const int32_t *pose_lens_host, const int32_t *lens_host, int B);
/* ts_body_pixel_infer_mixed_given whose given block is PRODUCED here: given_poses_dev (B,P_max,body_dim+hand_dim), pose_lens_host /
 * pose_lens_dev (B,) in the order of the submitted, sorted clips.  The encoders run in front of the pass as the audio encoder does, into a
 * code block of the stream's work buffers; G_b = P_b / 4 is set on the host; then exactly what the _given entry runs, with the same graphs.
 * P_max / 4 <= T_max / 4.  given_poses_dev == NULL, or every P_b == 0: exactly the _lp entry.  Passes that do not use this entry launch
 * what they launched before it existed. */
int ts_body_pixel_infer_mixed_poses(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                    const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                    const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                    float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                    const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                    void *stream);
/* ts_vqvae_decode_pair with length-masked layers: latents (B,H) each, rows at or beyond lens[b] / 4 are not read (gathered as zero rows;
 * an index outside the codebook INSIDE a clip still gives NaNs); out_dev (B,4H,body_dim+hand_dim), rows at or beyond 4 (lens[b] / 4) = 0. */
int ts_vqvae_decode_pair_masked(ts_vqvae *vq_body, ts_vqvae *vq_hand, const int64_t *lat_body_dev, const int64_t *lat_hand_dev,
                                const int32_t *lens_dev, int B, int H, float *out_dev, void *stream);
/* ---- kept positions: keep chosen positions of given codes, redraw the rest -----------------------------------------------------------------
 * "given rows" keeps a prefix in TIME.  The code grid has a second axis: column 0 is the BODY codebook, column 1 the HAND codebook, and the
 * chain predicts (r, 0) then (r, 1), each conditioned on the other part's past.  A pass with given rows may bring a mask `keep` beside the
 * given block, in the block's layout: (B,H_max,2) uint8, in slot order (the order of the submitted, sorted clips).
 * THE RULE.  The sampler launch of position (r, j) is FORCED for clip slot b iff 2 r + j < 2 G_b AND (keep == NULL or keep[b, r, j] != 0).
 * Everything else in "given rows" stays word for word: a forced workgroup reads its code, writes it where a drawn code goes and draws
 * nothing; an unforced one runs the arithmetic of the sampler it stands in for, operation for operation.  One rule therefore covers resume,
 * tail redraw, per-part redraw ("keep this body motion, draw new hands"; N hand takes for one body take; keep the hands, redraw the body)
 * and any mixture per clip, and the pass stays on its hipGraphs.  What follows from the rule:
 *   - unkept codes are never read: a position below G_b with keep == 0 is PRODUCED, and its entry of the given block may hold anything
 *     (values outside the vocabulary, -1);
 *   - unkept uniforms ARE read: the uniform of an unkept position below G_b is read (without a mask no uniform below G_b is); the uniform
 *     of a kept position still is not;
 *   - Philox is unchanged: a code's position is its absolute (row, column); kept positions consume nothing, their numbers are skipped, not
 *     shifted.  Handing back an earlier decode with ANY mask (same seed, clip index and record) therefore returns that decode bit for bit;
 *   - log-probabilities are unchanged in kind: a kept position gets the log-probability of its code under the distribution it would have
 *     been drawn from (talkshow_amd/sampling.py::given_logprob; -inf for a code the record removed), a produced position what a draw gets;
 *   - the mask is read for rows r < G_b only; rows beyond may hold anything.  A byte is 0 or not 0.
 * Forcing the HAND column while drawing the BODY column is a forced decode, not a posterior sample: the body draw at row r sees the hands
 * of rows < r only, never the hand code of its own row or of later rows; the result is NOT a sample of p(body | hands).
 * The entries: the _given / _poses entries with keep_dev appended before the stream.  keep_dev == NULL is exactly the existing entry (which
 * calls these with NULL); keep_dev without the given block it selects from is an error.  In the _poses_keep entry the mask applies to the
 * codes the encoders produce (rows r < P_b / 4).
 * Graphs: bit 3 (value 8) of the sixth key field for "mask present".  A masked pass runs the masked form in every chunk, so its number of
 * distinct keys is what a given pass has (at most 14 of the 16 chunk slots); a chunk's rows of the mask travel into a uint8 staging block of
 * the work buffers ahead of its replay, exactly as its given codes do (chunks with rows below max G_b only; eager runs read the caller's
 * mask).  A repeated masked pass captures nothing, whatever its mask; passes without a mask find the keys, graphs and launches they found
 * before.  talkshow_amd/sampling.py::keep_forced restates the rule in numpy.
 * Out of scope: the output head of a kept column still runs (a kept position costs what a produced one costs); poses remain the VQ decode
 * of the returned codes; the streaming sessions are untouched. */
int ts_pixelcnn_generate_mixed_keep(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                    const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                    const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                    const int32_t *given_rows_dev, const uint8_t *keep_dev, void *stream);
int ts_body_pixel_infer_mixed_keep(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                   const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                   const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                   float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                   const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev, void *stream);
int ts_body_pixel_infer_mixed_poses_keep(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                         const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                         const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                         float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                         const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                         const uint8_t *keep_dev, void *stream);
/* ---- speaker style: blended and time-varying speakers per clip ------------------------------------------------------------------------------
 * The speaker reaches the model in exactly one way: a vector h_l of 2D floats per layer, added pointwise to the pre-gate sums of every
 * position (gated_pixelcnn_v2.py:65, `h[:, :, None, None]`); with integer ids it is row label[b] of class_cond_embedding_l.  A pass may
 * bring float WEIGHTS in place of the ids.  A clip's style is a row of NC = n_classes float32 weights: one row for the whole clip, or one
 * row per CODE row (a code row is 4 pose frames).
 * THE RULE.  The class-conditioning vector of layer l at code row r of clip b, element k, with E_l the layer's (NC, 2D) table:
 *     acc = nothing
 *     for c = 0 .. NC-1 ascending:
 *         if w[b,r,c] != 0:  t = w[b,r,c] * E_l[c,k]            (rounded to fp32)
 *                            acc = t if acc is nothing else acc + t   (rounded to fp32)
 *     h_l[b,r,k] = acc, or +0.0 if every weight is 0
 * Product and sum are rounded separately (__fmul_rn / __fadd_rn: no FMA contraction).  A zero weight (+0.0 or -0.0) contributes nothing
 * and its table row is not read.  Weights are any FINITE floats: there is no non-negativity rule and no sum-to-one rule, because
 * extrapolation (1.5 and -0.5) is a use.  What follows from the rule:
 *   - a one-hot row gives E_l[c] bit for bit, a -0.0 entry included: a pass whose clips all bring one-hot rows returns what the integer
 *     ids return;
 *   - numpy.float32 arithmetic reproduces the rule exactly (talkshow_amd/sampling.py::style_rows);
 *   - a blend is an INTERPOLATION OF THE CONDITIONING VECTORS.  It is not a mixture of the speakers' distributions: 0.5 / 0.5 is a virtual
 *     fifth speaker whose vector lies between two trained ones, not a coin flip between two speakers.
 * The entries: the most general sibling of each family plus `const float *style_dev, int style_rows` ahead of the stream.  style_dev is
 * (B, style_rows, NC) float32 in slot order (the order of the submitted, sorted clips); style_rows is 1 (one row per clip) or H_max (one
 * row per code row; rows at or beyond a clip's own H_b are not used — a clip carried to a chunk's end runs under its last own row).  With
 * style_dev set, label_dev / ids_dev is not read and may be NULL.  style_dev == NULL: the sibling entry, launch for launch.  The weights
 * are NOT validated on the device (a NaN weight gives NaN logits); ts_style_check is the host-side rule.
 * style_rows == 1: the work buffer that held the gathered rows is filled by style_rows_kernel instead of the gather; keys, graphs and
 * chain launches are the same (the buffer's content is in no key), and a warm host captures nothing.
 * style_rows == H_max: the conditioning rows of ONE chunk (8 code rows) live in a staging buffer [NL][8][B][2D] fp32 of the work set
 * (allocated by the first such pass; 4 NL 8 B 2D bytes), filled by style_rows_kernel ahead of every chunk's replay — launched eagerly on
 * the stream like the staging of a chunk's uniforms and given codes; it is the only launch that reads the caller's block, so no caller
 * pointer enters a captured graph — and every gate launch of code row r reads row r's slab.  Graphs: bit 4 (value 16) of the sixth key
 * field.  Such a pass runs the staged form in every chunk, so its number of distinct keys is what the pass without tracks has (at most
 * 14 of the 16 chunk slots); a repeated tracked pass captures nothing, whatever its weights; passes without tracks find the keys, graphs
 * and launches they found before.
 * The style is orthogonal to sampling records, log-probabilities, given rows / poses, kept positions, clip indices and the draw modes.
 * Forced rows run under the style too (it shapes the row cache): handing back the head of an earlier decode WITH THE SAME STYLE returns
 * that decode bit for bit.
 * The streaming sessions take one weight row per clip per step, which holds until a later step brings another ("streaming sessions"
 * below).  Out of scope: per-row tracks inside a session's step, ts_body_pixel_infer, the face path, the single-stack form, weights per
 * layer. */
int ts_pixelcnn_generate_mixed_style(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                     const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                     const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                     float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                     const int32_t *given_rows_dev, const uint8_t *keep_dev, const float *style_dev, int style_rows,
                                     void *stream);
int ts_body_pixel_infer_mixed_style(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                    const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                    const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                    float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                    const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev,
                                    const float *style_dev, int style_rows, void *stream);
int ts_body_pixel_infer_mixed_poses_style(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                          const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                          const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                          float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                          const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                          const uint8_t *keep_dev, const float *style_dev, int style_rows, void *stream);
/* Host only: every one of the n weights of a style block (rows of NC) is finite; the error names the first bad index.  Python calls it
 * before anything is launched. */
int ts_style_check(const float *w_host, long n, int NC);
/* style_rows_kernel on its own (kernel-level tests): tables_dev (NL,NC,W) float32, weights_dev (M,NC) -> out_dev (NL,M,W), row m under
 * weight row m, by THE RULE above.  W is a positive multiple of 4; the three blocks are 16-byte aligned.  Synchronises. */
int ts_op_style_rows(ts_ctx *ctx, const float *tables_dev, int NL, int NC, int W, const float *weights_dev, int M, float *out_dev,
                     void *stream);

/* ---- code bias: per-clip bias and allow-lists on the codes ----------------------------------------------------------------------------------
 * No counterpart in the reference, which draws from the raw softmax.  A clip of a mixed pass may bring a TABLE b[2][V] of float32: row 0 is
 * added to the logits of the body column, row 1 to those of the hand column; the table is constant over the clip's code rows.  Every entry
 * is either -inf (the code is BANNED) or finite with |b_v| <= 1e30; NaN and +inf are refused; each of the two rows holds at least one entry
 * above -inf (ts_code_bias_check; V <= 8191 as for the controls).  An allow-list is a table of 0 and -inf.
 * THE RULE is a step 0 in front of steps 1-5 of ts_sampling, and one sentence added to the kept set:
 *  0. l'_v = l_v + b_v, ONE IEEE fp32 addition.  Steps 1-5 and the log-probability rule then run on l' unchanged, operation for operation:
 *     the maximum, d_v, det_expf, the ranking, top-k, the integer masses, top-p, the inverse CDF and d_c - log S.  The logits OUTPUT (the
 *     operator's row copy) stays the network's l.
 *  Kept set.  A token with l'_v = -inf is never kept, whatever top_k and top_p say and also under a neutral record.  (The sentence is
 *     needed: w_v = det_expf(-inf) = 0 already, key(-inf) ranks lowest and floor(0 * 2^31) = 0, so sums and masses do not move — but with
 *     such a token "kept" the two fallbacks of step 5, the chunk's and the row's highest kept token, can return it at u = 1 - 2^-24.  With
 *     banned tokens out of the kept set the draw never returns one.)
 *  Log-probabilities.  A drawn code gets d_c - log S under the biased, filtered distribution.
 *  Given codes.  A given or kept code that the bias bans is still TAKEN, as a code the filters remove is; its log-probability is -inf
 *     (d_c = -inf, and the code is not kept).
 *  Bit identity.  A clip without a table (index -1) executes the arithmetic of the sampler with controls as it was: nothing is added, its
 *     bits do not move.  An all-zero table gives the same CODES; its log-probabilities may differ in the sign of a zero only
 *     (-0 + 0 = +0: a logit -0 becomes +0, so a d_c or a result that was -0 may come out as +0).
 *  Scope.  The bias is a sampling control and shares the table's scope: TS_SAMPLE_UNIFORMS and TS_SAMPLE_PHILOX are accepted;
 *     TS_SAMPLE_GREEDY and TS_TEACHER_FORCED are refused with the table's message (per-clip greedy is top_k = 1).  A pass that brings a
 *     bias and no sampling table runs on neutral records, which compute the plain sampler's bits.  A uniform and a Philox number are
 *     consumed exactly as without a bias: a clip's random stream does not depend on its table.
 * talkshow_amd/sampling.py restates it (biased, keep_mask_bias, sample_bias).
 * The entries: the _style sibling of each family plus `const float *bias_dev, int n_bias, const int32_t *bias_index_host` ahead of the
 * stream.  bias_dev is (n_bias, 2, V) float32 on the device, 1 <= n_bias <= B (clips that share a table share one copy);
 * bias_index_host (B,) in slot order holds every clip's table, or -1 for a clip without one.  bias_dev == NULL: the _style entry, launch
 * for launch.  The tables' content is NOT validated on the device; ts_code_bias_check is the host-side rule.
 * Staging and graphs.  Tables and index are copied into the stream's work buffers in stream order ahead of the pass (one device-to-device
 * copy; the index travels as kernel arguments): captured samplers read work memory only, no host memory is read after the call returns,
 * nothing synchronises.  The samplers are kernels of their own (sample_ctl_bias_kernel / sample_ctl_bias_given_kernel) on graph keys of
 * their own: bit 5 (value 32) of the sixth key field.  Neither the tables' content nor n_bias is in the key: a repeated pass with other
 * tables captures nothing.  The table buffer is sized for one table per clip of the work set's clip CAPACITY (8 V bytes per clip), so it
 * NEVER MOVES between the passes of one capacity; the capacity grows only where every work buffer grows, and that drops all graphs of
 * the stream.  Passes without a bias launch the kernels and find the graphs they always did.
 * The streaming sessions take tables per step ("streaming sessions" below).
 * Out of scope: per-row bias tracks; ts_pixelcnn_v_*; the face generator; the scoring entries (score_clips / score_motion_clips take no
 * sampling table either). */
int ts_pixelcnn_generate_mixed_bias(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                    const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                    const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                    const int32_t *given_rows_dev, const uint8_t *keep_dev, const float *style_dev, int style_rows,
                                    const float *bias_dev, int n_bias, const int32_t *bias_index_host, void *stream);
int ts_body_pixel_infer_mixed_bias(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                   const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                   const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                   float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                   const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev,
                                   const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                   const int32_t *bias_index_host, void *stream);
int ts_body_pixel_infer_mixed_poses_bias(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                         const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                         const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                         float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                         const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                         const uint8_t *keep_dev, const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                         const int32_t *bias_index_host, void *stream);
/* Host only: the rule above on n_tables tables (n_tables, 2, V), 1 <= V <= 8191; 0, or an error that names the table, the column and the
 * code.  Python calls it before anything is launched. */
int ts_code_bias_check(const float *tables_host, int n_tables, int V);
/* Host only: 1 <= n_bias <= B and every index is -1 or in [0, n_bias); every entry that takes tables applies it before its first launch. */
int ts_code_bias_index_check(const int32_t *bias_index_host, int B, int n_bias);

/* ---- repetition penalty: a per-clip penalty over a window of earlier codes ------------------------------------------------------------------
 * No counterpart in the reference.  The one sampling control that reads what the clip has already produced: "not this code again within
 * the next W rows", or, with the opposite sign, "hold the pose".  One record per clip: */
#define TS_REPEAT_MAX_WINDOW 64
typedef struct ts_repeat {
    int32_t window;    /* W in [0, TS_REPEAT_MAX_WINDOW]; 0: off */
    float presence;    /* finite, |x| <= 1e30, any sign: subtracted once from a code the window has met */
    float frequency;   /* finite, |x| <= 1e30, any sign: subtracted once per time the window has met it */
    int32_t reserved;  /* 0 */
} ts_repeat;
/* A violation is refused, naming the clip, before anything is launched (ts_repeat_check).
 * THE RULE, for the sampler launch of absolute position (r, j) — code row r, column j — of a clip with W > 0:
 *  History.  c_v = the number of rows r' in [max(0, r - W), r) whose code in column j of THIS clip equals v.  Counted are the codes as the
 *     pass returns them: drawn, given and kept ones alike.  The two columns have separate histories (body and hand codebooks are different
 *     vocabularies), and no clip reads another's.
 *  0b. Behind step 0 (code bias) and ahead of step 1 (temperature): for c_v > 0, f = frequency * (float)c_v, g = presence + f,
 *     l''_v = l'_v - g — THREE IEEE fp32 operations, each rounded, never contracted into a fused multiply-add; for c_v == 0, l''_v is
 *     l'_v bit for bit.  Steps 1-5, the kept-set sentence of the code bias and the log-probability rule then run on l'' unchanged.  The
 *     logits OUTPUT (the row copy) stays the network's l.
 *  Finite by design.  |g| <= 1e30 + 64e30 < FLT_MAX, so a finite l' stays finite and -inf stays -inf: the penalty never empties a column
 *     and bans nothing, so no check depends on a draw.  presence = 1e30 is the practical "no repeat within W": such a code has weight
 *     det_expf(-1e30) = 0 and no crossing of step 5 lands on it.  It stays in the kept set, though (the penalty is no ban): where every
 *     code the filters keep has been met, it is what is drawn, and at u = 1 - 2^-24 the two fallbacks of step 5 may return it, as they
 *     may return any kept token of weight 0.  A host that needs a hard ban for the whole clip writes -inf into a code bias.
 *  Given and kept positions.  A forced position takes its code as before, and the code ENTERS THE HISTORY (a code outside [0, V) matches
 *     no token).  Its log-probability, when asked for, is that under the penalised, biased, filtered distribution; an unkept position is
 *     drawn under the penalty.
 *  Random numbers.  A uniform and a Philox number are consumed exactly as without the record.
 *  Bit identity.  A clip with window = 0 executes the arithmetic of the launch without the feature, operation for operation.  A clip with
 *     W > 0 and both penalties +0 returns the same codes AND the same log-probability bits: x - (+0) = x for every x, -0 included.
 *  Scope.  A sampling control with the table's scope: TS_SAMPLE_UNIFORMS and TS_SAMPLE_PHILOX; TS_SAMPLE_GREEDY and TS_TEACHER_FORCED are
 *     refused with the table's message (per-clip greedy is top_k = 1).  A pass without a sampling table runs on neutral records.
 * talkshow_amd/sampling.py restates it (repeat_counts, penalised, sample_repeat, decode_repeat).
 * Device state.  Every stream's work set holds history rings [clip slot][2][64] of int32: the code of row r, column j at index r & 63,
 * written by the thread that stores the code.  They are sized by the work set's clip CAPACITY like the bias tables, so they never move
 * between the passes of one capacity, and they need no clearing: a launch reads min(r, W) entries, all written earlier in the same pass by
 * the same slot (the active clips of a mixed pass are a prefix, so a clip's slot is the same in every chunk; clips carried past their end
 * write only their own ring).  r comes from the launch's absolute position — the kernel argument plus the dynamic base word under graph
 * replay, as for the given rows — so the eager route and the chunk graphs share one addressing.  A clip with window = 0 touches no ring.
 * Staging and graphs.  The records are copied into the stream's work buffers in stream order ahead of the pass (kernel arguments, like the
 * sampling table).  The samplers are kernels of their own (sample_ctl_rep_kernel / sample_ctl_rep_given_kernel: the code-bias kernels with
 * the penalty compiled in; a pass without tables runs them on a table index of -1) on graph keys of their own: bit 6 (value 64) of the
 * sixth key field.  Neither the records nor their number is in the key: a repeated pass with other records captures nothing.  Passes
 * without records launch the kernels and find the graphs they always did.
 * The entries: the _bias sibling of each family plus `const ts_repeat *rep_host, int n_rep` ahead of the stream: n_rep = 1 (one record
 * for all clips) or B records in slot order.  rep_host == NULL: the _bias entry, launch for launch.
 * Sessions.  The device record's fourth word is from_row, the first absolute row of the clip's current unbroken run of rows written under
 * window > 0: a launch at row r counts min(r - from_row, W) entries.  Every entry above leaves it 0 (a pass's history starts at row 0), so
 * their bits are those of min(r, W).  A streaming session (ts_pixelcnn_stream_step_ctl) keeps its rings between steps — a window reaches
 * back across step seams — and one from_row per clip on the host: set to the step's first row when the clip's window becomes positive
 * after being absent or 0, dropped when a step brings the clip no record or window = 0.  A penalty switched on mid-session therefore
 * starts from an EMPTY history at that row and never reads ring entries left by rows 64, 128, ... earlier.  ts_repeat and
 * ts_op_sample_repeat are unchanged: the word is not part of the public record.
 * Out of scope: ts_pixelcnn_v_*; the single-stack form; the scoring entries;
 * the face generator; windows beyond 64 rows; penalties that read the other column or other clips. */
int ts_pixelcnn_generate_mixed_repeat(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                      const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                      const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                      float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                      const int32_t *given_rows_dev, const uint8_t *keep_dev, const float *style_dev, int style_rows,
                                      const float *bias_dev, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                      void *stream);
int ts_body_pixel_infer_mixed_repeat(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                     const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                     const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                     float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                     const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev,
                                     const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                     const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, void *stream);
int ts_body_pixel_infer_mixed_poses_repeat(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                           const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                           const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                           float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                           const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                           const uint8_t *keep_dev, const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                           const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, void *stream);
/* Host only: the rule above on n records for vocabulary V, 1 <= V <= 8191; 0, or an error that names the clip.  The validation every
 * entry applies before its first launch. */
int ts_repeat_check(const ts_repeat *rep_host, int n, int V);

/* ---- guidance: a clip's logits pushed away from, or toward, those of a second conditioning ----------------------------------------------
 * No counterpart in the reference.  Every control above reshapes the distribution the model computes for ONE conditioning; guidance
 * compares two.  A pass has B clip slots.  A slot b may name one other slot g = guide[b] as its SHADOW, with a float scale[b]; guide[b] =
 * -1: none.  The shadow is an ordinary slot of the pass, of the same length as b, with its own audio rows and its own label or style
 * rows: the second conditioning q.  The shadow draws nothing.
 * THE RULE, for the sampler launch of every position (r, j): the workgroup of b reads both logits rows and forms, element by element,
 *     d = l_b - l_g;   t = scale * d;   l' = l_b + t
 * — THREE IEEE fp32 operations, each rounded, never contracted into a fused multiply-add (the convention of "speaker style").  The rule
 * runs AHEAD of step 0 (code bias), step 0b (repetition penalty) and steps 1-5: every later step, the log-probability included, runs on
 * l' exactly as it runs on l without the feature.  The logits OUTPUT (the row copy) stays the network's l, for both slots.
 *  Both slots, one history.  The workgroup of b writes what it chose or was given to BOTH slots: the token and the code of b and of g,
 *     the kept bytes and the log-probability to both where those outputs exist.  The workgroup of g returns without reading or writing
 *     anything.  l_g at the next position is therefore what q says about the codes b really produced.  A shadow's rows of every output
 *     are its primary's: codes, log-probabilities, and in the body wrapper its poses.
 *  scale > 0 pushes the draw away from q (classifier-free-guidance style: "more this audio than silence", "more speaker A, less speaker
 *     B"); scale = -0.5 draws from the geometric mean of the two distributions — the distribution-space blend "speaker style" is not;
 *     scale = -1 is q itself on b's history.
 *  Bit identity.  scale = 0 returns the codes of the pass without the table (t = +-0; a logit of -0 may become +0, so log-probabilities
 *     may differ in the sign of a zero).  A shadow with the primary's own conditioning gives d = 0 at every position: codes and
 *     log-probability bits equal the plain pass's for any finite scale.
 *  Random numbers.  A primary's uniform or Philox number is that of its own clip index and absolute position.  Shadows consume none and
 *     shift no other clip's index (a mixed pass names every slot's index in its clip table).
 *  Given, kept and forced positions are decided from the PRIMARY's row table and mask; a forced code is written to both slots.  The
 *     primary's repetition history is the only one read or written; a shadow's records, tables and given rows are never read.
 *  Independence.  A clip's result depends neither on which other clips of the pass are guided nor on where its shadow sits.
 *  Finite by design.  |scale| <= 1e4 keeps scale * d finite for any logits a trained network produces (|d| < 3e34).  Beyond that a
 *     non-finite l' — a NaN from inf - inf included — is the caller's affair: the samplers do not look for one.
 *  Scope.  A sampling control like the bias: TS_SAMPLE_UNIFORMS and TS_SAMPLE_PHILOX; greedy is top_k = 1.  A pass without a sampling
 *     table runs on neutral records.
 * ts_guide_check refuses, naming the slot, before anything is launched: an index outside [-1, B); a slot that names itself; a shadow named
 * twice; a shadow that is itself guided; unequal lengths in FRAMES (lens_host as the pass takes it, compared as it is — stricter than equal code rows; NULL: not checked); a NaN or an infinity; |scale| > 1e4.  In a pass it
 * comes LAST among the sampler checks.  talkshow_amd/sampling.py restates rule and check (guided, sample_guide, guide_roles).
 * Staging and graphs.  Roles (-1 plain, g >= 0 a primary, -2 a shadow) and scales are copied into the stream's work buffers in stream
 * order ahead of the pass (kernel arguments).  The samplers are kernels of their own (sample_ctl_guide_kernel /
 * sample_ctl_guide_given_kernel: the repetition kernels with the rule compiled in; a pass without records runs them on windows of 0, one
 * without tables on an index of -1) on graph keys of their own: bit 8 (value 256) of the sixth key field (bit 7 is a session's slot
 * restart).  Neither roles nor scales are in the key: a repeated guided pass captures nothing.  Passes without the table launch the
 * kernels and find the graphs they always did.  Chunking is unchanged: the chunks of a mixed pass are prefixes of the non-increasing length
 * table, so two slots of equal length are active together whatever lies between them.
 * The entries: ts_pixelcnn_generate_guided, ts_body_pixel_infer_guided and ts_body_pixel_infer_guided_poses are ts_pixelcnn_generate_mixed_repeat,
 * ts_body_pixel_infer_mixed_repeat and ts_body_pixel_infer_mixed_poses_repeat plus `const int32_t *guide_host, const float *guide_scale_host` ahead of the stream,
 * (B,) each in slot order.  guide_host == NULL: the _repeat entry, launch for launch.
 * The chain's streaming sessions take guidance at slot level ("session pairs" below), the seamless body sessions at clip level
 * (ts_body_stream_open_guided, "seamless sessions" below).
 * Out of scope: ts_pixelcnn_v_*; the single-stack form; the scoring entries (a pass whose rows are all given, with
 * a log-probability output, scores under guidance already); more than one shadow per clip. */
int ts_pixelcnn_generate_guided(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                     const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                     const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                     float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                     const int32_t *given_rows_dev, const uint8_t *keep_dev, const float *style_dev, int style_rows,
                                     const float *bias_dev, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                     const int32_t *guide_host, const float *guide_scale_host, void *stream);
int ts_body_pixel_infer_guided(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                    const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                    const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                    float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                    const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev,
                                    const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                    const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const int32_t *guide_host,
                                    const float *guide_scale_host, void *stream);
int ts_body_pixel_infer_guided_poses(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                          const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                          const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                          float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                          const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                          const uint8_t *keep_dev, const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                          const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const int32_t *guide_host,
                                          const float *guide_scale_host, void *stream);
/* Host only: the check above on a table of B slots; lens_host (B,) the slots' lengths in frames or NULL; 0, or an error that names the slot. */
int ts_guide_check(const int32_t *guide_host, const float *guide_scale_host, const int32_t *lens_host, int B);

/* ---- alternatives: entropy, rank and the n best codes of every position ------------------------------------------------------------------
 * No counterpart in the reference.  "log-probabilities" returns one number about a position's distribution, that of the code chosen.  A
 * pass that brings a ts_alt_out record also returns, from the same sampler launch, what else the model would have done and how sure it
 * was.  For a position of a clip let l'' be the row every later step runs on: the network's logits behind step 0 (code bias) and step 0b
 * (repetition penalty), and (T, k, p) the clip's record (neutral without a table).  The outputs describe the distribution THE FILTERS ARE
 * APPLIED TO — steps 1 and 2 of ts_sampling, ahead of top-k and top-p — so a top_k = 1 decode (the per-clip greedy) still reports
 * informative alternatives and entropy.
 * THE RULE.
 *  Quantities.  m = max l''; d_v = (l''_v - m) * inv_T, two fp32 operations, the argument of step 1; w_v = det_expf(d_v).  A token with
 *     l''_v = -inf (banned) has w_v = 0 and takes no part in any sum.
 *  S_all.  The fp32 total of w_v over all tokens with the samplers' summation structure: 256 contiguous chunks left to right, then the
 *     chunk sums left to right.  Where the record has neither top-k nor top-p in force, S_all is the S of "log-probabilities" bit for bit.
 *  Alternatives j = 0 .. n-1.  The tokens of rank j in step 2's ranking (l'' descending, -0 equal to +0, ties by index ascending), banned
 *     tokens excluded.  alt_code[j] is the index; alt_logprob[j] = (float)((double)d_j - log((double)S_all)) — d_j is used, never
 *     log w_j, as for "log-probabilities".  With fewer than n allowed tokens the remaining entries are code -1 and -inf.
 *  Entropy.  t_v = w_v * d_v, one fp32 product formed only where w_v > 0; E the fp32 total of t_v with the same summation structure
 *     (every addition rounded on its own: no fused multiply-add); entropy = (float)(log((double)S_all) - (double)E / (double)S_all).
 *     Both terms are non-negative (S_all >= 1, E <= 0): nothing cancels.
 *  Rank.  The number of tokens ahead of the position's code c — drawn, given or kept — in step 2's ranking over all V tokens: an exact
 *     integer, independent of T; -1 for a given code outside [0, V).
 *  Purity.  All four are pure functions of the clip's own row, record, bias row and history: bit-identical alone or inside a mixed pass of
 *     any size, eager or replayed, drawn or forced.  Nothing here feeds the draw: codes and log-probabilities of a pass with the record
 *     are those of the pass without it, bit for bit.
 *  Forced positions (given / kept) get all four, as they get their log-probability.
 *  Invalid rows of a mixed pass, at or beyond a clip's own H_b, hold -1, 0, 0, -1: codes, log-probabilities, entropy, rank.
 * talkshow_amd/sampling.py restates the rule (alternatives, alternatives_error_bound).
 * Kernels, staging and graphs.  The samplers are kernels of their own (sample_ctl_alt_kernel / sample_ctl_alt_given_kernel: the
 * repetition kernels with the log-probability and the rule compiled in; a pass without records runs them on windows of 0, one without
 * tables on an index of -1, one without a sampling table on neutral records — slots that execute the arithmetic of the smaller kernels
 * operation for operation).  No launch is added to the chain.  Under graph replay the four outputs go to a staging block of the stream's
 * work buffers and are copied out behind the replay, as logprob_dev is.  Graph keys of their own: bit 9 (value 512) of the sixth key
 * field, with n in the bits above it, so a repeated pass with the same n captures nothing.  Passes without the record launch the kernels
 * and find the graphs they always did.
 * The entries are the _repeat entry of each family (the session: the _ctl step) plus `const ts_alt_out *alt` ahead of the stream; NULL:
 * that entry, launch for launch.  They need logprob_dev (the kernels compute it either way) and a drawing mode; a guided pass and a session
 * with pairs are refused.  The new checks run behind every existing one.
 * Out of scope: guided passes and paired sessions; the seamless body sessions; the scoring entries; the single-stack form; the samplers
 * without controls' modes (greedy, teacher forced); the face generator. */
#define TS_ALT_MAX 8
typedef struct ts_alt_out {
    int32_t n;             /* 0 .. TS_ALT_MAX alternatives per position */
    int32_t reserved;      /* 0 */
    int32_t *codes_dev;    /* (B,H,2,n) int32; NULL for n = 0 */
    float *logprob_dev;    /* (B,H,2,n) fp32;  NULL for n = 0 */
    float *entropy_dev;    /* (B,H,2) fp32 */
    int32_t *rank_dev;     /* (B,H,2) int32 */
} ts_alt_out;
/* Host only: n outside [0, TS_ALT_MAX], reserved != 0, a missing pointer, a mode that is not TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (the
 * message says that per-clip greedy is top_k = 1 under a drawing mode); 0, or an error. */
int ts_alt_check(const ts_alt_out *alt, int mode);
int ts_pixelcnn_generate_alt(ts_pixelcnn *pix, const int64_t *label_dev, const float *aud_dev, const int32_t *lens_host,
                                   const int32_t *lens_dev, int B, int H_max, int mode, const float *uniforms_dev, uint64_t seed,
                                   const int64_t *clip_index_dev, int64_t *codes_dev, const ts_sampling *ctl_host, int n_ctl,
                                   float *logprob_dev, const int64_t *given_dev, const int32_t *given_rows_host,
                                   const int32_t *given_rows_dev, const uint8_t *keep_dev, const float *style_dev, int style_rows,
                                   const float *bias_dev, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                   const ts_alt_out *alt, void *stream);
int ts_body_pixel_infer_alt(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                  const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                  const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                  float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev, const int64_t *given_dev,
                                  const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep_dev,
                                  const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                  const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt, void *stream);
int ts_body_pixel_infer_alt_poses(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *mfcc_dev,
                                        const int64_t *ids_dev, const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode,
                                        const float *uniforms_dev, uint64_t seed, const int64_t *clip_index_dev, int64_t *codes_dev,
                                        float *poses_dev, const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                        const float *given_poses_dev, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                        const uint8_t *keep_dev, const float *style_dev, int style_rows, const float *bias_dev, int n_bias,
                                        const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt,
                                        void *stream);

/* s2g_body_vq.TrainWrapper.infer_on_audio(initial_pose=gt) core (smplx_body_vq.py:254-281):
 * poses_dev (B,T,body_dim+hand_dim) in c_index order -> recon_dev same shape, codes_dev (B,H,2) int64.
 * Either output may be NULL: recon_dev == NULL is the encode-only form (VQVAE.encode of both parts, the latents
 * `s2g_body_pixel.__call__` builds, smplx_body_pixel.py:193-203).  Body and hand networks run in lockstep
 * (same-shape layers go out as one grouped launch). */
int ts_body_vq_infer(ts_vqvae *vq_body, ts_vqvae *vq_hand, const float *poses_dev, int B, int T,
                     int64_t *codes_dev, float *recon_dev, void *stream);

/* ---- single operators (kernel-level parity tests call these; weights given in the reference's layouts) ------ */
/* nn.Conv1d / nn.ConvTranspose1d (+ optional fused activation: 0 none, 1 LeakyReLU(0.2), 2 ReLU) on NLC data:
 * x_dev (B,Lin,Cin); w_host (Cout,Cin,K) or, transposed, (Cin,Cout,K); bias_host (Cout) or NULL;
 * out_dev (B,Lout,Cout).  Supported: K in {1,3} stride 1 pad (K-1)/2; K=4 stride 2 pad 1 (both directions). */
int ts_op_conv1d(ts_ctx *ctx, const float *x_dev, int B, int Lin, int Cin, const float *w_host,
                 const float *bias_host, int Cout, int K, int stride, int pad, int transposed, int act,
                 float *out_dev, void *stream);
/* VectorQuantizerEMA.get_code_indices (vqvae_modules.py:311-319): x_dev (M,dim), codebook_dev (ncode,dim)
 * -> idx_dev (M) int64 = argmin_j (|x|^2 + |e_j|^2 - 2 x.e_j), ties -> lowest j. */
int ts_op_vq_argmin(ts_ctx *ctx, const float *x_dev, int M, const float *codebook_dev, int ncode, int dim,
                    int64_t *idx_dev, void *stream);
/* F.linear on few rows (the per-position GEMM of the PixelCNN chain): x_dev (M,K), w_host (N,K), bias_host (N)
 * -> out_dev (M,N); relu optional. */
int ts_op_linear(ts_ctx *ctx, const float *x_dev, int M, int K, const float *w_host, const float *bias_host,
                 int N, int relu, float *out_dev, void *stream);
/* the per-position sampler: logits_dev (B,V) -> idx_dev (B) int64; mode TS_SAMPLE_GREEDY or
 * TS_SAMPLE_UNIFORMS (uniforms_dev (B)). */
int ts_op_sample(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev,
                 int64_t *idx_dev, void *stream);
/* the same draw in TS_SAMPLE_PHILOX mode (softmax + multinomial(1) of gated_pixelcnn_v2.py:173-176 with the library's own
 * random stream): row b draws with u = Philox4x32-10(key = seed; counter = (position, clip_index0 + b, 0)) >> 8 * 2^-24,
 * exactly what ts_pixelcnn_generate uses for clip clip_index0 + b at grid position row * 2 + column. */
int ts_op_sample_philox(ts_ctx *ctx, const float *logits_dev, int B, int V, uint64_t seed, int64_t clip_index0,
                        uint32_t position, int64_t *idx_dev, void *stream);

/* ts_op_sample / ts_op_sample_philox with sampling controls (ts_sampling, steps 1-5): logits_dev (B,V), 1 <= V <= 8191; mode TS_SAMPLE_UNIFORMS
 * (uniforms_dev (B)) or TS_SAMPLE_PHILOX (seed, clip_index0, position as in ts_op_sample_philox); ctl_host: n_ctl = 1 (one record for all
 * rows) or B records -> idx_dev (B) int64 and, if not NULL, kept_dev (B,V) uint8: 1 for the tokens the filters kept. */
int ts_op_sample_ctl(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                     int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, uint8_t *kept_dev,
                     void *stream);
/* One sampler launch with the log-probability of every row's code: ts_op_sample_ctl's arguments plus logprob_dev (B) fp32.  ctl_host may be
 * NULL: then mode is any of the four (sample_lp_kernel), V is any size >= 1, kept_dev must be NULL, and for TS_TEACHER_FORCED idx_dev (B) is
 * the INPUT: the given codes (left as they are; one outside [0, V) gives NaN).  logprob_dev == NULL: ts_op_sample_ctl with a table, the
 * sampler of ts_op_sample / ts_op_sample_philox without. */
int ts_op_sample_lp(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                    int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, uint8_t *kept_dev,
                    float *logprob_dev, void *stream);

/* One launch of the samplers' given variants ("given rows" above) on given logits: ts_op_sample_lp's arguments without kept_dev, plus
 * forced_host (B) int32 — row b is forced iff forced_host[b] != 0 — and given_dev (B) int64, read for forced rows only.  mode greedy,
 * uniforms or Philox; ctl_host and logprob_dev may each be NULL.  idx_dev (B) receives the given code of a forced row and the sampler's
 * choice of every other row. */
int ts_op_sample_given(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                       int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                       const int32_t *forced_host, const int64_t *given_dev, void *stream);
/* The same launch with the DEVICE-side decision of "kept positions" exercised: ts_op_sample_lp's arguments without kept_dev, plus
 * given_rows_host (B) int32 (G of every row, >= 0), keep_dev (B) uint8 or NULL, given_dev (B) int64 and the launch's `position`: row b is
 * forced iff position < 2 given_rows_host[b] and (keep_dev == NULL or keep_dev[b] != 0).  given_dev is read for forced rows only, keep_dev
 * for rows with position < 2 G only, uniforms_dev for unforced rows only.  (ts_op_sample_given takes a host `forced` flag, turns it into a
 * row table and passes no mask: it does not reach the mask load.) */
int ts_op_sample_keep(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                      int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                      const int32_t *given_rows_host, const uint8_t *keep_dev, const int64_t *given_dev, void *stream);
/* One launch of the samplers under a "code bias": ts_op_sample_keep's arguments, then kept_dev (B,V) uint8 or NULL (1 for the tokens of
 * the kept set, banned tokens out) and logits_copy_dev (B,V) or NULL (the launch's row copy: the network's l, not l'), then bias_dev
 * (n_bias,2,V), n_bias, bias_index_host (B) (-1: the row has no table and computes ts_op_sample_ctl's bits) and column (0 body, 1 hand).
 * mode uniforms or Philox; ctl_host == NULL: neutral records.  given_rows_host == NULL (then keep_dev and given_dev are NULL too): the
 * launch without given rows, sample_ctl_bias_kernel; otherwise sample_ctl_bias_given_kernel.  The vector path is taken for V = 2048 on
 * 16-byte aligned logits and tables. */
int ts_op_sample_bias(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                      int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                      const int32_t *given_rows_host, const uint8_t *keep_dev, const int64_t *given_dev, uint8_t *kept_dev,
                      float *logits_copy_dev, const float *bias_dev, int n_bias, const int32_t *bias_index_host, int column, void *stream);
/* One launch of the samplers under a "repetition penalty": ts_op_sample_bias's arguments (bias_dev may be NULL here: no tables), then
 * rep_host, n_rep (1 or B records), then history_dev (B, R) int32, R = min(position >> 1, 64): the codes of rows (position >> 1) - R ...
 * (position >> 1) - 1 of the launch's column, oldest first (NULL for R = 0), then ring_out_dev (B, 64) int32 or NULL.  The entry fills
 * rings of -1, places the history in the ring slots where a pass would have left it, launches once (sample_ctl_rep_kernel, or
 * sample_ctl_rep_given_kernel with given rows) and copies each row's ring of that column to ring_out_dev.  rep_host == NULL:
 * ts_op_sample_bias. */
int ts_op_sample_repeat(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                        int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                        const int32_t *given_rows_host, const uint8_t *keep_dev, const int64_t *given_dev, uint8_t *kept_dev,
                        float *logits_copy_dev, const float *bias_dev, int n_bias, const int32_t *bias_index_host, int column,
                        const ts_repeat *rep_host, int n_rep, const int32_t *history_dev, int32_t *ring_out_dev, void *stream);
/* One launch of the samplers under "guidance": ts_op_sample_repeat's arguments (rep_host may be NULL here: no records; history_dev and
 * ring_out_dev are then optional), then guide_host (B) int32 — the shadow's ROW of every row or -1 — and guide_scale_host (B).  A primary
 * reads its shadow's logits row and writes idx_dev, kept_dev and logprob_dev of both rows; logits_copy_dev receives both rows as they
 * came; a shadow's ring stays as the entry filled it.  sample_ctl_guide_kernel, or sample_ctl_guide_given_kernel with given rows. */
int ts_op_sample_guide(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                       int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                       const int32_t *given_rows_host, const uint8_t *keep_dev, const int64_t *given_dev, uint8_t *kept_dev,
                       float *logits_copy_dev, const float *bias_dev, int n_bias, const int32_t *bias_index_host, int column,
                       const ts_repeat *rep_host, int n_rep, const int32_t *history_dev, int32_t *ring_out_dev, const int32_t *guide_host,
                       const float *guide_scale_host, void *stream);
/* One launch of the samplers with "alternatives": ts_op_sample_repeat's arguments (rep_host and bias_dev may both be NULL here), then the
 * record, whose arrays hold one position per row: codes_dev and logprob_dev (B,n), entropy_dev and rank_dev (B).  logprob_dev of the
 * launch is required.  sample_ctl_alt_kernel, or sample_ctl_alt_given_kernel with given rows; the vector path as for ts_op_sample_bias. */
int ts_op_sample_alt(ts_ctx *ctx, const float *logits_dev, int B, int V, int mode, const float *uniforms_dev, uint64_t seed,
                     int64_t clip_index0, uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx_dev, float *logprob_dev,
                     const int32_t *given_rows_host, const uint8_t *keep_dev, const int64_t *given_dev, uint8_t *kept_dev,
                     float *logits_copy_dev, const float *bias_dev, int n_bias, const int32_t *bias_index_host, int column,
                     const ts_repeat *rep_host, int n_rep, const int32_t *history_dev, int32_t *ring_out_dev, const ts_alt_out *alt,
                     void *stream);

/* Output assembly the callers do after both generators (scripts/demo.py:207-229 + data_utils/lower_body.py:68-87
 * `part2full`): body_dev (B,Tb,129) body+hand poses, face_dev (B,Tf,103) jaw(3)+expression(100) -> out_dev (B,Tf,265).
 * The body is aligned to the face length (last frame repeated, or trimmed); lower_pose33_host = the 33 fixed
 * lower-body values part2full inserts (`lower_pose`, or zeros with [6:9] = global orientation when stand=True). */
int ts_assemble_full(ts_ctx *ctx, const float *body_dev, int Tb, const float *face_dev, int Tf, int B,
                     const float *lower_pose33_host, float *out_dev, void *stream);

/* The same for clips of DIFFERENT lengths (after ts_body_pixel_infer_mixed and ts_face_generate_mixed): body_dev (B,Tb_max,129) with
 * tb[b] frames of clip b, face_dev (B,Tf_max,103) with tf[b] -> out_dev (B,Tf_max,265).  tb_dev / tf_dev (B,) int32 DEVICE tables,
 * 1 <= tb[b] <= Tb_max, 1 <= tf[b] <= Tf_max.  Row t < tf[b] is ts_assemble_full's row for the clip alone (Tb = tb[b], Tf = tf[b]): the body
 * frame is min(t, tb[b] - 1) — the last frame repeated, or trimmed.  Rows t >= tf[b] are written as 0.  Pure copies: bit-exact.  Every element
 * of out_dev is written, nothing else is touched; no synchronisation. */
int ts_assemble_full_mixed(ts_ctx *ctx, const float *body_dev, const int32_t *tb_dev, const float *face_dev, const int32_t *tf_dev, int B,
                           int Tb_max, int Tf_max, const float *lower_pose33_host, float *out_dev, void *stream);

/* ---- instrumentation ---------------------------------------------------------------------------------------- */
/* Per-kernel-family device time of the calls made on this context since the last reset, measured with HIP
 * events on the launch stream when enabled (adds synchronisation: benchmarking / profiling only).
 * families: 0 conv_gemm, 1 skinny_gemm (PixelCNN chain), 2 vq / sampling / glue.  ms_out[3], launches_out[3],
 * flops_out[3] (algorithmic 2*M*N*K of the GEMM launches; 0 for family 2). */
int ts_prof_enable(ts_ctx *ctx, int on);
int ts_prof_read(ts_ctx *ctx, double *ms_out, int64_t *launches_out, double *flops_out, int reset);
/* the same with n_families (1..4) entries per array; family 3 = the face generator's fused attention kernel (flops = 4 T^2 64 per
 * (clip, head) and layer), which ts_prof_read's three families leave out */
int ts_prof_read_n(ts_ctx *ctx, int n_families, double *ms_out, int64_t *launches_out, double *flops_out, int reset);

/* stage 1 of ts_mfcc_forward alone (get_mfcc_sepa, data_utils/utils.py:234-263, resamples the whole clip and then takes
 * the MFCC of two parts): wav_dev (B,N) at sr_in -> out_dev (B, ts_mfcc_resampled_len(m, N)) at sr_out. */
long ts_mfcc_resampled_len(const ts_mfcc *m, long n_samples);
int ts_mfcc_resample(ts_mfcc *m, const float *wav_dev, int B, long n_samples, float *out_dev, void *stream);
/* librosa.load(path, sr=16000) of the face front-end (data_utils/utils.py:194; librosa ~= 0.9.2 -> resampy 'kaiser_best'):
 * band-limited interpolation with a Kaiser-windowed sinc table (64 zero crossings, 512 samples per crossing, rolloff
 * 0.9475937167399596, beta 14.769656459379492), output length ceil(N * sr_out / sr_in) (librosa's fix_length).
 * wav_dev (B,N) mono -> out_dev (B, ts_resample_kaiser_len(N, sr_in, sr_out)).  Third-party arithmetic: PARITY UNPINNED. */
long ts_resample_kaiser_len(long n_samples, int sr_in, int sr_out);
int ts_resample_kaiser(ts_ctx *ctx, const float *wav_dev, int B, long n_samples, int sr_in, int sr_out, float *out_dev,
                       void *stream);

/* ---- mixed front-end passes: recordings of DIFFERENT lengths in one call (no counterpart in the reference, which reads one file at a time) ----
 * B recordings, recording b with ns[b] samples at the handle's input rate, stored padded to N_max samples.  The arithmetic of the uniform entries
 * on every recording: a recording's rows / samples are BIT-IDENTICAL whatever else is in the pass, and bit-identical to the uniform entry on the
 * recording alone (B = 1, N = ns[b]).  The kernels that look across a recording's samples or rows (polyphase and Kaiser resamplers, the STFT's
 * reflect padding, the per-clip top_db clamp) run as length variants that take from ns[b] what the uniform kernels take from N; the mel and DCT
 * GEMMs run over (B, T_max) rows with the length-masked epilogue and never take a stream-K band.  Recordings need no particular order.
 *   ns_host / ns_dev (B,) int32: the same table in host memory (checked and planned from without synchronising; not read after the call
 *     returns) and in device memory.  1 <= ns[b] <= N_max; anything else, a NULL table or B < 1 is an error and nothing is written.
 *   wav_dev (B,N_max): samples at or beyond ns[b] are never read (they may hold anything, NaNs included).
 * ONE HANDLE = ONE (sr_in, sr_out, fps): a host whose recordings come at several source rates groups them by rate, one handle and one
 * call per group.  The calls allocate nothing beyond the growth of the stream's work buffers and never synchronise.
 * ts_mfcc_forward_mixed: feat_dev (B,T_max,64), T_max = ts_mfcc_num_frames(m, N_max).  Rows t < T_b = ts_mfcc_num_frames(m, ns[b]) are the
 *   recording's MFCC rows, rows t >= T_b are written as 0; every element of feat_dev is written, nothing else is touched.  A recording whose
 *   resampled length is <= half an FFT window is an error (the rule of ts_mfcc_forward) and nothing is written. */
int ts_mfcc_forward_mixed(ts_mfcc *m, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max,
                          float *feat_dev, void *stream);
/* stage 1 alone: out_dev (B, ts_mfcc_resampled_len(m, N_max)); samples at or beyond ts_mfcc_resampled_len(m, ns[b]) are written as 0. */
int ts_mfcc_resample_mixed(ts_mfcc *m, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max,
                           float *out_dev, void *stream);
/* The per-recording maximum ts_mfcc_forward_mixed clamps at (its floor is this value - 80 dB): the same launches up to the mel projection, then
 * the maximum of 10 log10(max(x, 1e-10)) over the recording's own rows.  out_dev (B,) fp32.  Does not synchronise.  What a wav session
 * in TS_WAV_DB_PEAK mode is opened with when the recording is known beforehand. */
int ts_mfcc_peak_db_mixed(ts_mfcc *m, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max,
                          float *out_dev, void *stream);

/* ---- wav sessions: the front end fed SAMPLES in chunks (no counterpart in the reference, which reads whole files) ------------------------
 * A session of B slots that share one sample clock takes the recording's samples in pushes of any size 0 .. max_samples and returns, per
 * push, the MFCC rows that have become final; ts_mfcc_stream_flush ends the recording and returns the rest.  THE CONTRACT: the rows of a session
 * are the rows of ts_mfcc_forward on the whole recording, BIT FOR BIT, for any chunking — every stage is the one-shot kernel's arithmetic term
 * for term (the same taps in the same fmaf order; the same window, FFT passes and twiddle tables; the mel and DCT GEMMs on whole-tile plans,
 * where a row's bits do not depend on the rows it shares a launch with) — up to the one stage that looks across the recording, the clamp at
 * (maximum - 80 dB), which a session cannot know before the end.  db_mode fixes what stands in for it:
 *   TS_WAV_DB_PEAK     the floor of every row is peak_db_dev[b] - 80 (peak_db_dev: (B,) fp32 device table, copied at open).  With the
 *                      recording's own maximum (ts_mfcc_peak_db_mixed) the rows ARE the one-shot rows, bit for bit.
 *   TS_WAV_DB_RUNNING  the floor of row t is (the maximum over rows 0 .. t of the slot) - 80: a prefix maximum along time, carried across
 *                      pushes, so the rows do not depend on the chunking.  They equal the one-shot rows from the recording's loudest row on,
 *                      and before it wherever no value lies below the running floor.
 * When a row is final.  With norig, nnew, width, kw the handle's resampler constants (ts_mfcc_constants) and n samples received: resampled sample
 * j is final once its last tap (j / nnew) norig - width + kw - 1 < n; row t once t hop + 1023 < the count of final resampled samples (the left
 * reflection i < 0 -> -i reads nothing beyond that, except in row 0, whose sample -1024 reflects to 1024: row 0 waits for 1025 samples; the right
 * reflection and the rows up to T = N22 / hop + 1 come with the flush).
 * LATENCY: a row follows its centre sample by 1024 resampled samples plus the resampler's right wing of kw - width - 1 = width + norig - 1
 * input samples: 16 kHz -> 22 kHz (norig 8, width 7, kw 22): 46.5 ms + 14 samples = 47.4 ms; 44.1 kHz -> 22 kHz (norig 441, width 13, kw 467):
 * 46.5 ms + 453 samples = 56.8 ms; equal rates: 46.5 ms.
 * State, allocated at open and constant (ts_mfcc_stream_state_bytes): per slot fewer than kw input samples and at most 2048 resampled samples
 * kept between calls (each ahead of room for one call's own), one running maximum, and the call's work rows; the counters live on the host.
 * A session is bound to no stream (`stream` is per call) and takes ONE HOST THREAD AT A TIME.  ALL SLOTS SHARE THE SAMPLE CLOCK: there is no
 * slot restart, save, load or fork of a wav session (the body sessions fed from one refuse them too).
 * ts_mfcc_stream_push: wav_dev (B,n) contiguous, 0 <= n <= max_samples (n = 0: nothing is read) -> *frames rows in feat_dev (B,*frames,64)
 *   (room for ts_mfcc_stream_max_frames rows per slot always suffices; ts_mfcc_stream_plan names the count beforehand).  A refusal (after the
 *   flush, n out of range) moves no counter and launches nothing.
 * ts_mfcc_stream_flush: the remaining rows.  A recording whose resampled length is <= half an FFT window is refused with ts_mfcc_forward's
 *   message and no counter moves.  Afterwards only the counters and close are taken.
 * ts_mfcc_stream_plan: host arithmetic from the rates alone — the rows out after samples_before samples, and after n more (flush != 0: after
 *   the flush that follows them). */
typedef struct ts_mfcc_stream ts_mfcc_stream;
enum { TS_WAV_DB_RUNNING = 0, TS_WAV_DB_PEAK = 1 };
int ts_mfcc_stream_open(ts_mfcc *m, int B, long max_samples, int db_mode, const float *peak_db_dev, ts_mfcc_stream **out);
int ts_mfcc_stream_push(ts_mfcc_stream *h, const float *wav_dev, long n, float *feat_dev, int *frames, void *stream);
int ts_mfcc_stream_flush(ts_mfcc_stream *h, float *feat_dev, int *frames, void *stream);
long ts_mfcc_stream_samples_in(const ts_mfcc_stream *h);
long ts_mfcc_stream_frames_out(const ts_mfcc_stream *h);
long ts_mfcc_stream_state_bytes(const ts_mfcc_stream *h);
long ts_mfcc_stream_max_frames(const ts_mfcc_stream *h);
void ts_mfcc_stream_close(ts_mfcc_stream *h);
int ts_mfcc_stream_plan(int sr_in, int sr_out, int fps, long samples_before, long n, int flush, long *frames_before, long *frames_after);
/* out[5] = norig, nnew, width, kw, hop of the handle (equal rates: 1, 1, 0, 0, hop) */
void ts_mfcc_constants(const ts_mfcc *m, int32_t out[5]);

/* ts_resample_kaiser on recordings of different lengths: out_dev (B, ts_resample_kaiser_len(N_max, sr_in, sr_out)); row b holds the
 * ts_resample_kaiser_len(ns[b], ...) samples of the recording alone, zeros beyond.  A recording too short to give one output sample is an
 * error. */
int ts_resample_kaiser_mixed(ts_ctx *ctx, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max,
                             int sr_in, int sr_out, float *out_dev, void *stream);

/* ---- streaming generation -----------------------------------------------------------------------
 * Replaces the pre_latents / pre_audio prefix of GatedPixelCNN.generate (gated_pixelcnn_v2.py:158-165) and its caller
 * (smplx_body_pixel.py:260-269,291-304), which re-run the whole prefix for every chunk: a session keeps the row cache
 * (one previous row per layer, the layer-0 partial sums, the last code rows) on the device, so a step costs the same
 * whatever the history length and the state is O(1) (the receptive field is 17 code rows).  A clip generated in chunks
 * is bit-identical to the same clip generated by one ts_pixelcnn_generate call (greedy; and stochastic, since the
 * Philox position of a code is its absolute (row, column)).
 * label_dev (B,) int64 is fixed for the session; max_chunk_rows bounds Hc of every step (buffers are sized once). */
typedef struct ts_pixelcnn_stream ts_pixelcnn_stream;
int ts_pixelcnn_stream_open(ts_pixelcnn *pix, const int64_t *label_dev, int B, int max_chunk_rows, ts_pixelcnn_stream **out);
/* aud_dev (B,Hc,aud_dim): audio-encoder rows of the next Hc code rows -> codes_dev (B,Hc,2) int64.  mode: GREEDY,
 * UNIFORMS (uniforms_dev (B,Hc,2)) or PHILOX (seed, clip_index0 as in ts_pixelcnn_generate). */
int ts_pixelcnn_stream_step(ts_pixelcnn_stream *st, const float *aud_dev, int Hc, int mode, const float *uniforms_dev,
                            uint64_t seed, int64_t clip_index0, int64_t *codes_dev, void *stream);
/* code rows generated so far */
int64_t ts_pixelcnn_stream_rows(const ts_pixelcnn_stream *st);
/* Streaming sessions with per-clip sampling controls.  ts_pixelcnn_stream_step plus the optional pieces of a mixed pass, each under the
 * rule of the mixed entry of the same name and FOR THIS STEP ONLY; all NULL / 0: ts_pixelcnn_stream_step launch for launch, on its graph
 * keys (sixth field 0), with its bits.  Everything is checked on the host, the failing clip named, before anything is launched and before
 * the session's row counter moves.  Rows are absolute: Philox positions, given-row tests and the history ring of a step that starts at
 * row r0 are those of rows r0 .. r0 + Hc - 1 of a one-shot call, so a clip stepped under some pieces equals ts_pixelcnn_generate_mixed_*
 * under the same pieces bit for bit, codes and log-probabilities.
 *   ctl_host, n_ctl      "sampling controls": 1 record for all clips or B in slot order; UNIFORMS / PHILOX only.  A step without a table
 *                        runs the plain sampler.
 *   logprob_dev          (B,Hc,2) fp32, "log-probabilities" of this step's codes, written in the sampler launch; every mode.
 *   given_dev,           (B,Hc,2) int64 and (B,) with 0 <= g_b <= Hc: clip b's first g_b rows OF THIS STEP are taken, the rest produced
 *   given_rows_host      ("given rows"; the samplers' table holds r0 + g_b).  A taken code draws no number; with logprob_dev it scores under
 *                        the distribution it would have been drawn from; it enters the row cache and the history ring.
 *   style_dev            (B,NC) "speaker style" weights, one row per clip: the conditioning rows are rewritten ahead of this step and STAY
 *                        until a later step brings others (NULL: as they are; at row 0 the labels given at open).  A one-hot row is the
 *                        label bit for bit.
 *   bias_dev, n_bias,    "code bias": (n_bias,2,V) tables and (B,) table index or -1.  Without ctl_host the step runs on neutral records.
 *   bias_index_host      The session's table buffer is allocated at its first biased step, sized by its fixed clip count: it never moves.
 *   rep_host, n_rep      "repetition penalty" over the session's own rings (see "Sessions" there): 1 record or B.
 * Graphs: the sixth key field is the samplers' bit set as in a mixed pass; records, tables, given codes and style are in no key, so a
 * second step of the same (Hc, buffer phase) under other values captures nothing, and plain steps keep their graphs.
 * Not taken by a session: a mask of kept positions, given poses, style tracks inside a step, the scoring entries. */
int ts_pixelcnn_stream_step_ctl(ts_pixelcnn_stream *st, const float *aud_dev, int Hc, int mode, const float *uniforms_dev,
                                uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                                const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                const int64_t *given_dev, const int32_t *given_rows_host,
                                const float *style_dev,
                                const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                const ts_repeat *rep_host, int n_rep, void *stream);
/* The step plus "alternatives" for its Hc rows: the record's arrays are (B,Hc,2,n) and (B,Hc,2).  alt == NULL: the entry above, launch for
 * launch.  A session with pairs is refused. */
int ts_pixelcnn_stream_step_alt(ts_pixelcnn_stream *st, const float *aud_dev, int Hc, int mode, const float *uniforms_dev,
                                uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                                const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                const int64_t *given_dev, const int32_t *given_rows_host,
                                const float *style_dev,
                                const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt, void *stream);
int64_t ts_pixelcnn_stream_captures(const ts_pixelcnn_stream *st);   /* hipGraphs this session has captured so far */
void ts_pixelcnn_stream_close(ts_pixelcnn_stream *st);

/* ---- slot restart: the clips of a session come and go ("continuous batching") ---------------------------------------------
 * A SLOT of a running session ends its clip and begins a new one at any step, while its neighbours carry on.  After a restart of slot b
 * at session row R0 (the session's next row, ts_pixelcnn_stream_rows):
 *   - slot b's code row R0 + k is row k of a NEW clip with the given label (or style row) and Philox clip index;
 *   - its codes and log-probabilities from there on are those of ts_pixelcnn_generate* on that clip alone under the same mode, seed and
 *     pieces, bit for bit (PHILOX: clip_index0 = the given index; the Philox position of its code is (row - R0, column));
 *   - every other slot's bits are those of the session without the restart;
 *   - a slot may restart any number of times, at any session row, rows 0 to 2 included; several slots may restart in one call.
 * How: a step reads little of what earlier rows wrote — the token ring row above, the layer-0 look-ahead sums, one projected row per
 * layer, the conditioning rows, the Philox position and the history rings (DESIGN.md §5 has the list) — and every kernel of the chain
 * reads a negative code as the zero row.  The restart writes "nothing above this row" into the slot's rows of those buffers: -1 codes,
 * +0.0 sums, the bare bias where a projection would be.  A one-shot call's row 0 leaves those terms out; the restarted slot adds exact
 * zeros in their place, and x + (+0.0) is x.
 *   slots_host (n,)        distinct slots in [0, B)
 *   labels_host (n,)       class labels in [0, NC), or NULL                  } exactly one of the two; a one-hot style row is the label
 *   style_dev (n,NC)       "speaker style" weight rows on the device, or NULL } bit for bit
 *   clip_index_host (n,)   Philox clip index of each new clip, >= 0.  A restarted slot keeps its index whatever clip_index0 later steps
 *                          pass; a slot that has never restarted keeps clip_index0 + b of each step.
 * Session rows stay session rows everywhere else: given_rows_host of a step counts from the step's first row, the history rings are indexed
 * by the session row, and a restarted slot's repetition penalty starts from an empty history at R0 (as a clip's does at its row 0).  A
 * step's style_dev rewrites the conditioning rows of EVERY slot, a restarted one included.  A slot whose user has left needs no call: it
 * keeps stepping on whatever audio rows it is given and its output is ignored.
 * Everything is checked on the host, the failing slot named, before anything is launched or any table moves: a slot out of range or listed
 * twice, a label outside [0, NC), both a label and a style row or neither, a negative clip index.  Stream-ordered, no synchronisation; the
 * launches (one reset kernel; one more per style row) run ahead of the next step's replay and are in no graph.  A session that has
 * restarted a slot runs its steps with its origin table bound, on graph keys of their own (bit 7 of the sixth key field): captured once
 * per (Hc, buffer phase, kind of sampler), whichever slots restart later.  A session that never restarts launches, captures and returns
 * exactly what it did before this entry existed.
 * ts_body_stream_* (seamless sessions, below) has no such entry: its windows are cut on the session's row grid and all its clips have one
 * length. */
int ts_pixelcnn_stream_restart(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, const int64_t *labels_host,
                               const float *style_dev, const int64_t *clip_index_host, void *stream);
/* code rows of the slot's current clip (= ts_pixelcnn_stream_rows for a slot that has never restarted); -1 for a bad slot */
int64_t ts_pixelcnn_stream_slot_rows(const ts_pixelcnn_stream *st, int slot);

/* The session's cached graphs: their number, and the chain launches and flops recorded when they were captured, summed (any pointer may be
 * NULL).  A session that never restarts a slot shows the figures of the same steps before the restart entry existed. */
int ts_pixelcnn_stream_graph_stats(const ts_pixelcnn_stream *st, int64_t *graphs, int64_t *launches, double *flops);

/* ---- slot state: save a slot's state, load it into any slot (rewind, branch, hand a clip over, park a user) --------------------
 * What a slot carries from row to row is small and closed (the list under "slot restart"): three rows of the token ring,
 * Q1[r & 3], Q0[r & 3], Q0[(r + 1) & 3], P(l, r & 1) for l >= 1, CR[l], its row origin and Philox clip index, and its two 64-entry
 * repetition histories.  A restart writes "nothing above this row" there; a save reads those entries out and a load writes them back at
 * another slot, another session row and another buffer phase, one small launch each way.
 * THE RULE.  ts_pixelcnn_stream_save of slot b at session row r (the session's next row) gives a state S; the slot's clip then has
 * n = r - origin[b] rows.  Loading S into slot b' of a session T of a network with the same dimensions and weights, at T's next row r',
 * under Philox clip index k' (default: the index the source drew under) gives:
 *   - continuation: slot b' produces from row r' on the codes and log-probabilities slot b would have produced from row r on under the
 *     same later inputs (audio rows, mode, seed, the pieces of the steps);
 *   - one-shot equivalence: under index k' and any later inputs its rows equal rows n, n+1, ... of ts_pixelcnn_generate* over the clip's
 *     whole audio with the clip's first n code rows given and clip_index0 = k', under the same label or style and pieces, bit for bit.  A
 *     code's Philox position stays its (row, column) inside the clip;
 *   - neighbours: every other slot of T has the bits of T without the call;
 *   - save is read-only: the source session's later bits, launches and graph captures are those without the call; it runs in stream
 *     order behind the previous step and needs no synchronisation;
 *   - the state carries the slot's conditioning rows CR (a blend row in force stays in force until a step brings style rows), the label
 *     the slot stands for, both repetition histories with their length (a window carries across the move), the clip index and the
 *     clip's row count;
 *   - it does not carry sampling records, bias tables, session defaults or given rows: those belong to a step or to the target session
 *     and count in the TARGET session's rows, as after a restart;
 *   - fan-out: one state may be loaded into several slots in one call (state_index_host), each under its own clip index; a slot may be
 *     loaded any number of times;
 *   - portability: a state moves between sessions of different B and between two network handles with EQUAL WEIGHTS, and as bytes
 *     through the host and to another device.  ts_slot_info records D, NL, NC and V, which a load checks; that the weights are equal is
 *     the caller's business and is not checked.
 * The device state is one row of ts_pixelcnn_slot_state_words(pix) 32-bit words per slot (a function of D and NL alone; 16-byte aligned
 * blocks); the host record beside it is ts_slot_info.  A save at r < 3 is canonical: an entry the session's launches of rows r and r + 1
 * would not have read (they leave out terms in a session's first three rows) is saved as the value a restart writes there, so a state
 * is complete and phase-neutral whatever row it came from.  For the same reason a load at r' < min(n, 3) is REFUSED: the target's launches
 * of those rows would leave out terms the clip's state holds (n <= r' is always fine: the clip is younger than the session).  For
 * r' < n the slot's origin r' - n is negative; ts_pixelcnn_stream_slot_rows still gives n.
 * Everything is checked on the host, the slot named, before anything is launched or any table moves: a slot out of range, a slot listed
 * twice (load), a dimension or version mismatch, a state index outside the given states, r' < min(n, 3), a negative clip index.  The
 * first load of a session does what its first restart does (the origin table; steps on the restart graph keys from there on); a session
 * already on those keys captures nothing new, and neither call is in any graph.  A session that never saves or loads allocates,
 * launches, captures and returns exactly what it did before these entries existed.  ts_body_stream_* (seamless sessions) has no such
 * entries: its MFCC tail and code ring sit on the session's row grid. */
#define TS_SLOT_STATE_VERSION 1
typedef struct ts_slot_info {
    int32_t D, NL, NC, V;   /* the network the state is of */
    int32_t version;        /* TS_SLOT_STATE_VERSION */
    int32_t hist;           /* entries of the repetition histories that count (<= 64), or -1: no penalty was running */
    int64_t rows;           /* n: code rows of the clip */
    int64_t clip_index;     /* the Philox clip index the slot drew under, or -1 (a never-restarted slot of a session that has not stepped) */
    int64_t label;          /* the label the slot stands for where the library was told it (a restart or a load), or -1: the open label */
} ts_slot_info;
int64_t ts_pixelcnn_slot_state_words(const ts_pixelcnn *pix);   /* 32-bit words of one slot's state row; -1 for NULL */
/* slots_host (n,) in [0, B) -> state_dev (n, words) fp32-typed words (16-byte aligned), info_host (n,) */
int ts_pixelcnn_stream_save(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, float *state_dev, ts_slot_info *info_host, void *stream);
/* slot slots_host[i] takes state row state_index_host[i] of state_dev (n_states, words) / info_host (n_states,); state_index_host NULL: row i
 * (n_states == n) or row 0 (n_states == 1).  clip_index_host (n,) or NULL: each state's own index. */
int ts_pixelcnn_stream_load(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, const float *state_dev, int n_states,
                            const int32_t *state_index_host, const ts_slot_info *info_host, const int64_t *clip_index_host, void *stream);

/* ---- session pairs: "guidance" at slot level in a streaming session ----------------------------------------------------------------
 * A session of S slots may hold PAIRS (b, g): slot g is the SHADOW of slot b under the rule of "guidance" above.  g has its own audio rows
 * (aud_dev[g] of every step) and its own label or style row (from open, restart or load); it draws nothing and receives every token, code
 * and log-probability b writes.  A paired clip's codes and log-probabilities equal those of ts_pixelcnn_generate_guided on the two slots
 * alone, bit for bit, whatever the chunking, under every piece of ts_pixelcnn_stream_step_ctl; every other slot has the bits of the
 * session without the pair.  A primary draws under its own clip index and row origin; the shadow's are never read.
 * WHEN A PAIR MAY FORM.  The shadow's row cache must hold b's code history under q from the clip's row 0, so a pair is declared
 *   - at session row 0,
 *   - behind the call that restarts BOTH slots, or
 *   - behind the call that loads BOTH slots from states of equal clip rows,
 * and ahead of the next step.  Every other attempt is refused, naming the slots and the rows.  Restarting or loading one slot of a pair
 * without the other is refused ("slot 3 is paired with slot 7: list both"); a restart or a load that lists both DISSOLVES the pair unless a
 * ts_pixelcnn_stream_pair behind it declares it again.  There is no pairing and no un-pairing in the middle of a clip: scale 0 is the off
 * switch (the codes of the session without the pair).  A save reads a paired slot like any other; pairs are not part of a state: a guided
 * clip moves by saving both slots and loading both, then declaring the pair.
 * Roles and scales are kernel arguments, never in a graph key.  Each pair has a stored scale; ts_pixelcnn_stream_step_guided may bring
 * others for its step.  EVERY step entry of a session with pairs runs the guided sampler family (bit 8 of the sixth key field, with bit 7
 * once the session has restarted or loaded) on neutral records where it brought none, ts_guide_check last among its checks; greedy mode
 * is then refused as in a pass (top_k = 1 is the greedy guided decode).  One graph per (Hc, buffer phase, kind of sampler).  A shadow has
 * no repetition history of its own: the primary's ring is the only one read or written.  So a saved SHADOW's state records no history
 * (hist = -1): a load that swaps the roles — the old shadow's state into the new primary — starts that clip's penalty from an empty
 * history at the load, which is NOT what the one-shot pass under the same records gives.  Load the primary's state into the primary
 * where a repetition penalty runs.  A session without pairs issues exactly the
 * launches it did and finds the graphs it had.
 * ts_pixelcnn_stream_pair: n pairs (primary_host[i], shadow_host[i]) with stored scales scale_host[i]; host tables only, nothing is
 * launched; all or none.  ts_pixelcnn_stream_pairs: the session's table into guide_out (S,) as ts_guide_check takes it (the shadow's slot
 * of every primary, else -1); returns the number of pairs.  ts_pixelcnn_stream_step_guided: ts_pixelcnn_stream_step_ctl plus
 * guide_scale_host (S,), read at primaries only; NULL: the stored scales.  A NaN, an infinity or |scale| > 1e4 is refused naming the slot.
 * ts_pixelcnn_stream_pair_check, host only, holds the rule (the entries call it; talkshow_amd/streaming.py restates it as SlotPairs):
 * S slots at session row `rows`; guide_host (S,) the pair table; clip_rows_host (S,) the rows of every slot's current clip; fresh_host (S,)
 * per slot the serial (> 0) of the restart or load that listed it if no step was run since, else 0.  shadow_host != NULL: the declaration
 * of n pairs — refused for a slot out of range, a slot that names itself, a slot listed twice, a slot already paired, rows > 0 without one
 * call that listed both, unequal clip rows, a bad scale.  shadow_host == NULL: a restart or load listing the n slots of primary_host —
 * refused where it lists one slot of a pair without the other. */
int ts_pixelcnn_stream_pair(ts_pixelcnn_stream *st, const int32_t *primary_host, const int32_t *shadow_host, const float *scale_host, int n);
int ts_pixelcnn_stream_pairs(const ts_pixelcnn_stream *st, int32_t *guide_out);
int ts_pixelcnn_stream_step_guided(ts_pixelcnn_stream *st, const float *aud_dev, int Hc, int mode, const float *uniforms_dev,
                                   uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                                   const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                   const int64_t *given_dev, const int32_t *given_rows_host,
                                   const float *style_dev,
                                   const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                   const ts_repeat *rep_host, int n_rep, const float *guide_scale_host, void *stream);
int ts_pixelcnn_stream_pair_check(int S, int64_t rows, const int32_t *guide_host, const int64_t *clip_rows_host, const int32_t *fresh_host,
                                  const int32_t *primary_host, const int32_t *shadow_host, const float *scale_host, int n);

/* ---- seamless sessions ---------------------------------------------------------------------------------------------------
 * A body session fed MFCC chunks of ANY length that returns, over its pushes and one flush, the codes and poses ts_body_pixel_infer
 * returns for the concatenated audio, bit for bit (same mode, seed and clip_index0) — where a plain session (ts_audioenc_forward,
 * ts_pixelcnn_stream_step and ts_vqvae_decode_pair per chunk, as the reference does) pads every chunk border like a clip edge.  No
 * layer carries state: each call runs the audio encoder and both VQ decoders on a WINDOW through the existing entries and keeps the rows
 * whose bits the window's borders cannot reach: 7 code rows either side for the encoder (its receptive field), 13 for the decoders
 * (their receptive field of 6, and 7 more because the rounding of a Winograd-lowered layer reaches to the edge of its 4-row tile); every
 * window is cut at a multiple of 4 code rows so that those tiles sit where the one-shot call has them.  The price is a lag: a code row
 * is final 7 code rows (28 frames) after its audio arrived and its poses 13 rows after that — 20 code rows, 80 frames.  Where the audio
 * encoder itself is lowered (TS_CONV_WINO=1, or an encoder of 512 channels or more) its reach is 14 rows for the same reason, the session
 * takes that at open, and the lag is 27 code rows (ts_body_stream_lag_rows).
 * The session owns a ts_pixelcnn_stream, the last <= 71 MFCC frames (127 with a lowered encoder; double-buffered) and a ring of its last code rows; all buffers are
 * allocated at open and never grown, whatever the history.  max_chunk_frames bounds t of every push.  All clips of a session have one
 * length.  ids_dev (B,) int64 is fixed for the session.  A session belongs to the thread that drives it. */
typedef struct ts_body_stream ts_body_stream;
int ts_body_stream_open(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const int64_t *ids_dev, int B,
                        int max_chunk_frames, ts_body_stream **out);
/* Host only: what the next call — a push of t >= 1 frames (flush = 0) or the flush (flush != 0, t = 0) — will produce: *code_rows = n code
 * rows, *pose_frames = m pose frames (either may be 0), so that the host can size uniforms, given, logprob and the outputs. */
int ts_body_stream_plan(const ts_body_stream *st, int t, int flush, int64_t *code_rows, int64_t *pose_frames);
/* mfcc_dev (B,t,64), 16-byte aligned -> codes_dev (B,n,2) int64 (16-byte aligned): the n code rows this call finalises, and poses_dev
 * (B,m,body_dim+hand_dim): the next m pose frames, n and m as ts_body_stream_plan says; with n = 0 / m = 0 the pointer is not read.
 * mode, uniforms_dev (B,n,2), seed, clip_index0 and the optional pieces are those of ts_pixelcnn_stream_step_ctl FOR THE n ROWS THIS
 * CALL RUNS (logprob_dev, given_dev (B,n,2)); all NULL / 0: the plain step.  The session's own arguments are checked before the first
 * launch; the pieces are checked by the chain before its first launch and before any counter moves; what is launched ahead of that writes
 * scratch and the idle half of the double buffer only, so a REFUSED call leaves the session where it was.  A call that fails on the
 * device leaves the session broken: every later call is refused.  Stream-ordered; no
 * synchronisation, no host copy. */
int ts_body_stream_push(ts_body_stream *st, const float *mfcc_dev, int t, int mode, const float *uniforms_dev, uint64_t seed,
                        int64_t clip_index0, int64_t *codes_dev, float *poses_dev,
                        const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                        const int64_t *given_dev, const int32_t *given_rows_host,
                        const float *style_dev,
                        const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                        const ts_repeat *rep_host, int n_rep, void *stream);
/* The end of the clip: the rows and frames held back come out (the last window runs to the clip's true end, leftover frames_in % 4
 * included, as the one-shot call's does).  Over a session the pose frames sum to 4 (frames_in / 4).  Every later call is refused. */
int ts_body_stream_flush(ts_body_stream *st, int mode, const float *uniforms_dev, uint64_t seed, int64_t clip_index0, int64_t *codes_dev,
                         float *poses_dev,
                         const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                         const int64_t *given_dev, const int32_t *given_rows_host,
                         const float *style_dev,
                         const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                         const ts_repeat *rep_host, int n_rep, void *stream);
/* Guided sessions: "guidance" at clip level in a seamless session ("session pairs" above, "guidance").  The session's B clips may have
 * n_shadow SHADOWS, at most one per clip.  The chain session behind it has S = B + n_shadow slots: the clips in slots 0 .. B-1 (their
 * Philox clip indices stay clip_index0 + b), shadow k in slot B + k, paired with clip shadow_of[k] at row 0 under scale_host[k].  The audio
 * encoder runs on E = B + n_a MFCC streams, n_a the shadows with audio of their own (enc_of[k] = its stream, numbered B, B + 1, ... in
 * shadow order; -1: the shadow hears its clip's audio and gets the clip's ENCODED rows: nothing is encoded twice).  One small launch
 * (stream_spread_rows_kernel) writes the kept audio rows of stream map[s] to chain slot s.  MFCC tails, the encoder window and its
 * output are sized for E, the chain for S, the code ring, the latent columns and the decoders for B: ts_body_stream_state_bytes stays
 * constant.  Over its pushes and one flush the session returns, for the B clips, the codes, poses and log-probabilities of
 * ts_body_pixel_infer_guided on the whole audio, bit for bit.
 *   ids_dev (S,)                 labels of the chain's slots: the clips', then the shadows'
 *   shadow_of, enc_of (n_shadow,) host: strictly increasing clips; -1 or the next stream of its own
 *   shadow_style_dev             (n_shadow, NC) weight rows of the shadows on the device, or NULL (the labels).  Given: EVERY shadow takes
 *                                its row (a one-hot row is the label bit for bit), written as a restart at row 0 writes it, on `stream`
 *   scale_host (n_shadow,)       the pairs' stored scales
 * The session's calls are ts_body_stream_push_guided / _flush_guided: the existing entries with mfcc_dev (E, t, 64), with uniforms_dev,
 * codes_dev, logprob_dev, given_dev and every per-clip table for the S slots (the clips first: the clips' rows of the (S, n, 2) code
 * block are its first B * n entries, and only those reach the decoders), poses_dev (B, ., pose_dim), plus guide_scale_host (S,), read at
 * primaries only; NULL: the stored scales.  The plain entries are refused on a guided session and the guided ones on a plain session; a
 * refused call moves no counter; the broken-session rule is as above.  A session without shadows goes through the existing entries
 * unchanged.  No restart, save or load, as for every seamless session. */
int ts_body_stream_open_guided(ts_convnet *audioenc, ts_pixelcnn *pix, ts_vqvae *vq_body, ts_vqvae *vq_hand, const int64_t *ids_dev, int B,
                               int n_shadow, const int32_t *shadow_of, const int32_t *enc_of, const float *shadow_style_dev,
                               const float *scale_host, int max_chunk_frames, void *stream, ts_body_stream **out);
int ts_body_stream_push_guided(ts_body_stream *st, const float *mfcc_dev, int t, int mode, const float *uniforms_dev, uint64_t seed,
                               int64_t clip_index0, int64_t *codes_dev, float *poses_dev,
                               const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                               const int64_t *given_dev, const int32_t *given_rows_host,
                               const float *style_dev,
                               const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                               const ts_repeat *rep_host, int n_rep, const float *guide_scale_host, void *stream);
int ts_body_stream_flush_guided(ts_body_stream *st, int mode, const float *uniforms_dev, uint64_t seed, int64_t clip_index0,
                                int64_t *codes_dev, float *poses_dev,
                                const ts_sampling *ctl_host, int n_ctl, float *logprob_dev,
                                const int64_t *given_dev, const int32_t *given_rows_host,
                                const float *style_dev,
                                const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                const ts_repeat *rep_host, int n_rep, const float *guide_scale_host, void *stream);
int64_t ts_body_stream_frames_in(const ts_body_stream *st);     /* MFCC frames received */
int64_t ts_body_stream_code_rows(const ts_body_stream *st);     /* code rows finalised */
int64_t ts_body_stream_pose_frames(const ts_body_stream *st);   /* pose frames returned */
int64_t ts_body_stream_state_bytes(const ts_body_stream *st);   /* device bytes of the session's own buffers: constant from open to close */
int ts_body_stream_lag_rows(const ts_body_stream *st);          /* code rows between a row's audio and its poses: 20, or 27 with a lowered encoder */
int64_t ts_body_stream_captures(const ts_body_stream *st);      /* ts_pixelcnn_stream_captures of the chain session it owns */
void ts_body_stream_close(ts_body_stream *st);

/* ---- batched SMPL-X joints / vertices ----------------------------------------------------------------
 * Replaces the per-frame float64 CPU calls of smplx.SMPLX.forward in scripts/demo.py:122-152 (get_vertices) and
 * data_utils/get_j.py:20-50 (get_joints).  Third-party arithmetic (smplx ~= 0.1.28, requirements.txt:5; package and
 * licensed model file absent): PARITY UNPINNED — the published LBS algorithm restated; fp32 on the device.
 * Model arrays are HOST float32 / int32 in the package's layouts: v_template (V,3), shapedirs (V,3,n_betas+n_expr) =
 * cat(shapedirs, expr_dirs), posedirs ((J-1)*9, V*3), J_regressor (J,V), parents (J), lbs_weights (V,J), pose_mean (J*3)
 * in the package's joint order; pose_src_offset[j] = column of a pose row where joint j's axis-angle starts (TalkSHOW's
 * 265-d rows: global_orient 9, body 12.., jaw 0, eyes 3 / 6, hands 75.. / 120.., get_j.py:21-30); extra_idx = vertex ids
 * of vertex_joint_selector, lmk_faces (n_lmk,3) = faces_tensor[lmk_faces_idx], lmk_bary (n_lmk,3).
 * with_vertices != 0 also uploads the full-mesh blend-shape matrix (V*3 x 896 floats, 112 MB for the real model). */
int ts_smplx_create(ts_ctx *ctx, int V, int J, int n_betas, int n_expr, const float *v_template, const float *shapedirs,
                    const float *posedirs, const float *J_regressor, const int32_t *parents, const float *lbs_weights,
                    const float *pose_mean, const int32_t *pose_src_offset, int n_extra, const int32_t *extra_idx, int n_lmk,
                    const int32_t *lmk_faces, const float *lmk_bary, int with_vertices, ts_smplx **out);
void ts_smplx_destroy(ts_smplx *m);
/* J + n_extra + n_lmk (127 for the reference's model) */
int ts_smplx_num_joints(const ts_smplx *m);
/* rows_dev (N,row_ld): pose rows, expression coefficients at columns [expr_off, expr_off + n_expr); betas_dev (n_betas) shared
 * by all rows, or (N,n_betas) when betas_per_row != 0 -> joints_dev (N, num_joints, 3) and, if not NULL, verts_dev (N,V,3).
 * A row must hold every column the model reads: row_ld >= max(pose_src_offset) + 3, expr_off >= 0 and, for n_expr > 0,
 * expr_off + n_expr <= row_ld; anything else is an error and nothing is launched (ts_smplx_create refuses a negative pose_src_offset). */
int ts_smplx_forward(ts_smplx *m, const float *betas_dev, int betas_per_row, const float *rows_dev, int row_ld, int expr_off,
                     int64_t N, float *joints_dev, float *verts_dev, void *stream);

/* ---- evaluation on the device --------------------------------------------------------------------
 * The reference computes its metrics on the CPU after the hot path (scripts/test_body.py:113-194); these are the
 * reductions behind them, float64 accumulation, deterministic (fixed-order partial sums, no float atomics).
 * Outputs are device doubles. */
/* evaluation/FGD.py:131-146 (np.mean / np.cov inputs of the Frechet distance): feat_dev (n,D) float32, D in {32,64,128}
 * -> stats_dev[0..D) = sum over rows, stats_dev[D + i*D + j] = sum over rows of x_i x_j  (D + D*D doubles). */
int ts_eval_feat_stats(ts_ctx *ctx, const float *feat_dev, int64_t n, int D, double *stats_dev, void *stream);
/* evaluation/FGD.py:153-158 (feat_dist numerator): sum over all n elements of |a - b|. */
int ts_eval_l1_total(ts_ctx *ctx, const float *a_dev, const float *b_dev, int64_t n, double *out_dev, void *stream);
/* scripts/test_body.py:98-110 body_loss on joints: gt_dev (T,J,3), prs_dev (B,T,J,3) ->
 * out3_dev = { sum_t sum_b sum_{j<J_lvd} | |v_pr| - |v_gt| | over t < T_lvd-1   (LVD numerator, metrics.py:73-84),
 *              sum_{b,t,j} |gt - pr|_2                                           ("error" numerator),
 *              sum_{t,j} | var_b(pr) |_2  (unbiased variance over the B samples) ("diverse" numerator) }. */
int ts_eval_body_loss(ts_ctx *ctx, const float *gt_dev, const float *prs_dev, int B, int T, int J, int J_lvd, int T_lvd,
                      double *out3_dev, void *stream);
/* evaluation/metrics.py:96-109 diversity: kps_dev (bs, L) -> sum over pairs i<j of sum_k |kps_i[k] - kps_j[k]|. */
int ts_eval_diversity(ts_ctx *ctx, const float *kps_dev, int bs, int64_t L, double *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TALKSHOW_HIP_H */
