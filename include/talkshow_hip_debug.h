/*
 * talkshow_hip_debug.h — measurement, tuning and test aids of libtalkshow_hip.so.
 *
 * NOT part of the drop-in surface (include/talkshow_hip.h): nothing here has a counterpart in the reference, no product code under
 * nets/ or evaluation/ calls these, and they may change between rounds.  Clients: tools/ (profiling / A-B scripts) and tests/
 * (host-side layout and launch-plan checks, tile-shape agreement, the shader-clock sampler).  Same conventions as the main header
 * (0 on success unless stated, ts_last_error() for the message).
 */
#ifndef TALKSHOW_HIP_DEBUG_H
#define TALKSHOW_HIP_DEBUG_H

#include "talkshow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Like ts_stream_create, but kernels of this stream only run on compute units [cu_first, cu_first+cu_count) of the
 * device's CU-mask index space (hipExtStreamCreateWithCUMask).  No reference counterpart. */
int ts_stream_create_cus(ts_ctx *ctx, int cu_first, int cu_count, void **out_stream);
/* Tuning aid: with TS_SKINNY_TRACE=1 the chain kernel stamps the device wall clock (100 MHz) at five points; this reads
 * (and resets) the records, 6 uint64 each.  Returns the number of records or -1. */
int ts_debug_skinny_trace(unsigned long long *out, int max_records);
/* Measurement aid: launches a one-wave kernel on `stream` that, every window_us for n windows, writes three uint64 to dev_out
 * (device memory, 3 n values): wall-clock ticks (100 MHz) since its start, ticks of this window, shader-clock cycles of this
 * window — the clock the chip actually sustains while other streams load it (tools/conv_clock.py).  No reference counterpart. */
int ts_debug_clock_sample(unsigned long long *dev_out, int n, int window_us, void *stream);
/* Host-only helper (no GPU needed): how `conv_gemm_f32` launches an (M rows x N columns, `groups` problems) layer that takes 128 x 128
 * tiles — out4 = {row blocks tiled 128 x 128, row blocks tiled 64 x 128, workgroups of the first band, workgroups in all}.  Returns 1 if the
 * layer is launched in two bands (more than one round of 512 resident workgroups, not a whole number of rounds), 0 for a plain grid,
 * -1 on a bad argument.  No reference counterpart. */
int ts_debug_conv_bands(int M, int N, int groups, int *out4);
/* Host-only: the tile {row tile, column tile} workgroup `bid` of conv_gemm_split's XCD-aware 1-D grid works on (MT x NT tiles, column groups of
 * `gw`); 1 = out2 filled, 0 = that workgroup has no tile, -1 = bad argument. */
int ts_debug_split_tile(int bid, int MT, int NT, int gw, int *out2);
/* Host-only helper (no GPU needed): the TILED copy of a row-major weight matrix W[N][ldw] (K columns used) that the
 * PixelCNN chain kernel multiplies with — every 16-column x 16-k operand fragment one contiguous KB in lane order
 * (DESIGN.md §3/§4); epi 0 = linear column order, 1 = gate (8 tanh channels + their 8 sigmoid partners per tile,
 * gateD channels per half).  out holds ceil(N/16) * (K/16) * 256 floats.  K % 16 == 0.  No reference counterpart. */
int ts_debug_tile_weights(const float *W, int N, int K, long ldw, int epi, int gateD, float *out);

/* Tuning / roofline entry (not part of the drop-in surface): a stride-1 conv layer (K = 1 or 3, Cin % 32 == 0)
 * whose weights are ALREADY packed on the device as [round128(Cout)][K*Cin] (tap-major, k contiguous), launched
 * `iters` times between two HIP events recorded on `stream`.  tile: 0 = the production plan; otherwise one plan (engine names of
 * ts_debug_conv_plan): 1 .. 7 = Reg with 128x128, 64x64, 128x64, 64x128, 64x64 with 64-deep K chunks, 160x128, 96x128 tiles; 31 / 39 / 33 =
 * Ring with the 128x128 tile on 4 / 8 waves and its 96x128 tile, 35 / 36 = RingDealt with 39's / 33's tiles, 37 = RingBanded (128 x 128 +
 * 64 x 128 tiles), 38 = RingSK (deterministic; not bit-identical with the others) — 37 / 38 fall back to 35 where the layer has no such plan;
 * 22 / 23 = Split with 2 / 3 planes (3 / 6 bf16 products per fp32 product), 24 = 22 on plane images of the weights made by
 * launch_split_weight_planes (w_planes = 1: the face's x3 plan); the split kernel takes 128 x 128 tiles from 200 of them on, 64 x 64 below;
 * 48 = Taps48 (batched 48-channel taps only).  *ms_out = mean launch duration in milliseconds. */
int ts_op_conv1d_timed(ts_ctx *ctx, const float *x_dev, int B, int Lin, int Cin, const float *w_packed_dev,
                       const float *bias_dev, int Cout, int K, int tile, int iters, float *out_dev, float *ms_out,
                       void *stream);
/* The same for a strided convolution without padding + GELU — the shape of the wav2vec2 feature convolutions
 * (out[t] = sum_k W_k x[stride t + k], HF Wav2Vec2FeatureEncoder; K <= 4): out_dev is (B, (Lin - K) / stride + 1, Cout). */
int ts_op_conv1d_strided_timed(ts_ctx *ctx, const float *x_dev, int B, int Lin, int Cin, const float *w_packed_dev,
                               const float *bias_dev, int Cout, int K, int stride, int tile, int iters, float *out_dev,
                               float *ms_out, void *stream);

/* Tuning / test entry for conv_taps48.hip (the wav2vec2 positional convolution, HF Wav2Vec2PositionalConvEmbedding + the encoder's residual
 * add): grouped convolution with G groups of 48 channels in and out, `ntap` taps -ntap / 2 .. ntap - ntap / 2 - 1 with zero padding, out = GELU(conv +
 * bias) + res.  x_dev / res_dev (optional) / out_dev: (B, T, G * 48); w_dev: [G][48][ntap * 48] (tap-major, a tap's 48 input channels contiguous);
 * bias_dev: [G * 48].  `iters` launches between two HIP events; *ms_out = mean launch duration in milliseconds. */
int ts_op_conv_taps48_timed(ts_ctx *ctx, const float *x_dev, int B, int T, int G, int ntap, const float *w_dev, const float *bias_dev,
                            const float *res_dev, int iters, float *out_dev, float *ms_out, void *stream);

/* Host-only helper (no GPU needed, no HIP call): the plan launch_conv_gemm gives a layer (csrc/conv_gemm.hip::plan_conv) — `groups` problems of
 * M rows x N columns x Ktot, each with nseg (<= 4) segments of seg_len[i] channels (one tap each); groups > 4: that many batched problems of one
 * segment whose Ktot / seg_len[0] taps make up K (the positional convolution's layout).  sk_ok: the caller accepts the stream-K band (the face
 * generator sets it); the device is taken to pass the band's hardware check.  tile: 0 = the production choice, else a tile id of
 * ts_op_conv1d_timed.  knob_list: "NAME=VALUE,..." of the TS_* levers in place of the environment, null = the defaults.
 * Returns the engine — 0 Reg (conv_gemm.hip, register-staged), 1 RegBanded, 2 Ring (LDS-DMA ring engine, plain grid), 3 RingDealt (tiles dealt
 * to the XCDs), 4 RingBanded, 5 RingSK (stream-K band), 6 Taps48, 7 Split — with out4 = {tile rows, tile columns, waves, K chunk} (Reg / Ring /
 * RingDealt; the big tile of a banded or stream-K plan), or -1 on a bad argument or an unknown tile id.  No reference counterpart. */
int ts_debug_conv_plan(int M, int N, int Ktot, int groups, int sk_ok, const int *seg_len, int nseg, int tile, const char *knob_list, int *out4);
/* Host-only helper (no GPU needed, no HIP call): the plan launch_skinny_batch gives n (<= 6) chain problems of mnk[3 i .. 3 i + 2] = (M, N, K)
 * rows x columns x depth, laid out as the PixelCNN lays out its operands; a negative K is an epilogue-only block of zero rows of that depth.
 * knob_list as for ts_debug_conv_plan.  Returns the kernel — 0 wide (skinny_wide.hip), 1 fast (the descriptor kernel), 2 generic 16-column,
 * 3 generic 32-column — with out4 = {waves, row blocks of 16, column blocks of 16 (fast), workgroups}, or -1 on a bad argument. */
int ts_debug_skinny_plan(const int *mnk, int n, const char *knob_list, int *out4);
/* Test aid: one launch of up to 6 INDEPENDENT PixelCNN chain problems (csrc/kernels.h, SkinnySeg / SkinnyParams: the fields below mirror
 * them one for one; Ktot is the sum of the segment lengths; every pointer is a device pointer the caller owns) through the production
 * plan, descriptor packing and launch code (launch_skinny_batch) under knob_list ("NAME=VALUE,..." as for ts_debug_skinny_plan, null =
 * the defaults; TS_SKINNY_TRACE is refused).  Allocates and uploads nothing; does not synchronize `stream`.  Returns the kernel that
 * ran (0 wide, 1 fast, 2 generic 16-column, 3 generic 32-column: a wide or fast plan whose descriptors do not pack runs generic
 * 16-column) with out5 = {kernel, waves, row blocks of 16, column blocks of 16 (fast), workgroups (generic: the grid's, problems
 * included)}, or -1 with ts_last_error() set: a bad argument, problems that fit no kernel, tiled operands on a generic kernel. */
typedef struct ts_debug_skinny_seg {
    const float *base;   /* dense: row m at base + (m >> row_shift) * row_stride; null (without gidx) = zero rows */
    const int *gidx;     /* gather: row = base + gidx[m * gidx_stride] * row_stride; a negative index = a zero row */
    long row_stride, gidx_stride;
    int row_shift, len, tiled_w;
} ts_debug_skinny_seg;
typedef struct ts_debug_skinny_problem {
    int M, N, nseg;
    ts_debug_skinny_seg seg[3];
    const float *W;
    long ldw;
    const float *bias;
    const float *add1;
    long add1_stride;
    int add1_shift;
    const float *add2;
    long add2_stride;
    int add2_shift;
    const float *add3;
    long add3_stride;
    const float *clsrow;
    int cls_ld;
    int epi, relu, gateD;   /* epi 0 linear, 1 gate */
    float *out;
    long out_stride;
    float *pre;
    long pre_stride;
    int w_tiled, out_tiled_w, pre_tiled_w, add1_tiled_w;
} ts_debug_skinny_problem;
int ts_debug_skinny_run(ts_ctx *ctx, const ts_debug_skinny_problem *problems, int n, const char *knob_list, int *out5, void *stream);
/* Test aid: ONE launch of a conv_gemm_f32 problem given as plain structs (csrc/kernels.h, ConvSeg / ConvGroup / ConvParams: the fields below
 * mirror them one for one; every pointer is a device pointer the caller owns; what the launchers set themselves — zero, sk_ws, sk_flags,
 * xcd_tiles — is left out) through production's planning and launch code: plan_conv(p, tile, knob_list, the device's stream-K
 * check) and launch_conv_plan.  tile: 0 = the production plan, else a tile id of ts_op_conv1d_timed.  22 / 23 = Split with 2 / 3
 * planes on the fp32 weights as given; 24 = 22 with w_planes set, on plane images this entry makes of every group's whole weight image
 * (launch_split_weight_planes chunk by chunk, so ldw and the strides between batched problems carry over: multiples of 32 then).  48 = Taps48:
 * Ktot is a multiple of 48 there (any tap count), a multiple of 32 for every other tile.
 * knob_list: "NAME=VALUE,..." as for ts_debug_conv_plan, null = the defaults.  Allocates and uploads nothing beyond what the launchers do (the
 * stream-K band's per-stream scratch) and tile 24's plane images; does not synchronize `stream`, except for tile 24 (the images are freed on return).
 * dry != 0: host only, no HIP call (ctx and the pointers may be null; the device is taken to pass the stream-K check): stops after planning
 * and the launcher's layout checks, so the same return value and out8 say what a launch WOULD run.
 * Returns the engine that ran (numbering of ts_debug_conv_plan) with out8 = {engine, tile rows, tile columns, waves, K chunk, tiles of
 * the second band (the 64-row tiles of a banded plan, the tiles of the stream-K band; 0 if none), workgroups in all, masked (0 / 1: the length-masked kernels)}
 * (Split: engine 7 with the 128 x 128 or 64 x 64 tile its launcher takes by size, 4 waves),
 * or -1 with ts_last_error() set: a bad argument, an unknown tile id, a layout the plan's kernel does not implement (lens on a tile without a
 * masked kernel or with batched problems, more than 4 segments, Ktot over 60 000, a segment that is no multiple of the tile's K chunk; Split:
 * x, w, ldx, ldw, c0 or a batched stride off its 16-byte loads, plane images with 3 planes or a pitch that is no multiple of 32, ...).
 * Nothing is launched then. */
typedef struct ts_debug_conv_seg {
    int d, c0, len, ntap;
} ts_debug_conv_seg;
typedef struct ts_debug_conv_group {
    const float *x, *w, *bias, *res;
    float *out;
    int out_col0, nseg;
    ts_debug_conv_seg seg[4];
} ts_debug_conv_group;
typedef struct ts_debug_conv_problem {
    int M, Lout, Lin, stride;
    int ldx, ldo, ldr;
    int N, Ktot, act, ngroups;
    ts_debug_conv_group g[4];
    int res_after_act;
    long ldw;
    int w_rows;
    int zdiv;
    long x_zs0, x_zs1, w_zs0, w_zs1, o_zs0, o_zs1, b_zs1, r_zs0, r_zs1;
    int sk_ok;
    const int32_t *lens;
    int len_shr, len_shl;
    int w_planes;   /* tiles 22 / 23 only: every w IS a plane image already (ConvParams::w_planes); tile 24 makes the images itself */
} ts_debug_conv_problem;
int ts_debug_conv_run(ts_ctx *ctx, const ts_debug_conv_problem *problem, int tile, const char *knob_list, int dry, int *out8, void *stream);
/* Host-only helper (no GPU needed): the stream-K plan of the ring engine for `groups` problems of M rows x N columns x K (csrc/conv_gemm_ring.hip:
 * whole 128 x 128 tiles for the row tiles that fill whole units of 256 tiles, the rows after them as one list of (tile, 32-k stage) iterations
 * cut into equal runs).  1 = out6 = {row tiles kept whole, row tiles in the band, dealt ids of the whole-tile region, band workgroups,
 * stages per tile, the plan the layer gets by cost: 8 = this one, 9 / 3 / 7 = a whole-tile plan}; 0 = no stream-K plan for this shape
 * (whole units, under one unit, runs under 4 stages); -1 = bad argument.  No reference counterpart. */
int ts_debug_conv_sk_plan(int M, int N, int K, int groups, int *out6);
/* 1 if the current device passed the stream-K band's hardware check (workgroup ids of equal residue mod 8 share an XCD: probed once by
 * ts_ctx_create), 0 if not or if no context was created yet: then no layer gets a stream-K plan. */
int ts_debug_conv_sk_supported(void);
/* Host-only: the run of band workgroup q (0 <= q < band_workgroups, a multiple of 8) over a stream-K band of `band_tiles` tiles x `stages`
 * stages, in band-iteration units (tile * stages + stage): out4 = {first iteration, one past the last, the XCD (= q % 8) whose tiles
 * [xcd * band_tiles / 8, (xcd + 1) * band_tiles / 8) the run lies in, the run index the kernel's owner search finds for the first iteration
 * (= q / 8)}.  0 on success, -1 on a bad argument.  No reference counterpart. */
int ts_debug_conv_sk_run(int band_tiles, int stages, int band_workgroups, int q, int *out4);

/* Test aid: out[i] = the chain kernels' gate activation tanh(v[i]) * sigmoid(p[i]) as they compute it (v_exp_f32 / v_rcp_f32 form,
 * csrc/kernels.h::gate_act; reference: GatedActivation, gated_pixelcnn_v2.py:16-22) on n device floats. */
int ts_debug_gate_act(const float *v_dev, const float *p_dev, float *out_dev, long n, void *stream);
/* Test aid: out[i] = the face generator's GELU epilogue v / 2 (1 + erf(v / sqrt 2)) as the kernels compute it (csrc/kernels.h::gelu_fast,
 * branch-free erf_fast) on n device floats. */
int ts_debug_gelu(const float *v_dev, float *out_dev, long n, void *stream);

/* Test aids: the face generator's non-GEMM kernels (csrc/face.hip), one launch each on `stream` (device pointers throughout, fp32).
 * ts_debug_attention: qkv (B, T, 3 HID) rows [q | k | v] with heads of 64 channels (HID = 64 heads) -> out (B, T, HID) = per (clip, head)
 * softmax(q k^T * scale) v (attention_kernel: fused QK^T, online soft-max over key tiles of 64, PV). */
int ts_debug_attention(const float *qkv, int B, int T, int HID, int heads, float scale, float *out, void *stream);
/* Row-wise LayerNorm (eps 1e-5) over C = 64 / 256 / 512 / 768 channels of M rows of pitch ldx: out = LN(x) gamma + beta (+ post_res rows of
 * pitch ldr when given), then ReLU if relu != 0; out rows of pitch ldo. */
int ts_debug_layernorm_rows(const float *x, int ldx, long M, int C, const float *gamma, const float *beta, const float *post_res, int ldr,
                            int relu, float *out, int ldo, void *stream);
/* Linear interpolation over time (align_corners = False) of x (B, Lin, 512) to (B, T, 512), fused with LayerNorm(512). */
int ts_debug_lerp_ln(const float *x, int B, int Lin, int T, const float *gamma, const float *beta, float *out, void *stream);
/* wav2vec2 feature-extractor layer 0: wav (B, N) -> out (B, L0, 512), L0 = (N - 10) / 5 + 1, = GELU(GroupNorm(512, 512)(Conv1d(1, 512, 10,
 * stride 5, no bias))); w [512][10], gamma / beta [512].  form: 1 = statistics from the waveform's second moments, 0 = from a pass that
 * computes the convolution, -1 = what production picks (TS_W2V_MOMENTS).  Allocates its own scratch and synchronizes `stream`. */
int ts_debug_w2v_conv0(const float *wav, int B, int N, const float *w, const float *gamma, const float *beta, int form, float *out,
                       void *stream);
/* x[b][t][col0 + j] = bias[j] + sum_c w[j][c] id[b][c] for j < nj, c < nc, every t < T of clip b < B; x rows of pitch ld. */
int ts_debug_fill_id(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0, int B, int T,
                     void *stream);
/* Their length variants (mixed face passes, talkshow_hip.h: B clips padded to N samples / T frames; ns / frames / lens are DEVICE int32 tables
 * of the clips' own counts unless named _host).  Valid rows are the arithmetic of the entries above on the clip alone, bit for bit; rows at or
 * beyond a clip's length are written as zeros, samples / rows beyond it are not read.
 * ts_debug_attention_mixed: qkv (B, T_max, 3 HID), out (B, T_max, HID); keys and queries of clip b stop at frames[b]; out rows beyond are NOT
 * written.  Builds the work list from frames_host (ts_debug_face_mixed_grid) and synchronizes `stream`. */
int ts_debug_attention_mixed(const float *qkv, const int32_t *frames_host, const int32_t *frames_dev, int B, int T_max, int HID, int heads,
                             float scale, float *out, void *stream);
/* M = B T rows (b, t); rows t >= lens[b] are written as zeros, their input is not read. */
int ts_debug_layernorm_rows_lens(const float *x, int ldx, int B, int T, const int32_t *lens, int C, const float *gamma, const float *beta,
                                 const float *post_res, int ldr, int relu, float *out, int ldo, void *stream);
/* x (B, Lin, 512) -> out (B, T, 512): clip b interpolates its own feature rows (of ns[b] samples) to its own frames[b] frames. */
int ts_debug_lerp_ln_lens(const float *x, int B, int Lin, int T, const int32_t *ns, const int32_t *frames, const float *gamma,
                          const float *beta, float *out, void *stream);
/* wav (B, N) -> out (B, L0, 512), L0 = (N - 10) / 5 + 1; GroupNorm statistics over the clip's own (ns[b] - 10) / 5 + 1 rows.  form as above.
 * Allocates its own scratch and synchronizes `stream`. */
int ts_debug_w2v_conv0_lens(const float *wav, int B, int N, const int32_t *ns, const float *w, const float *gamma, const float *beta,
                            int form, float *out, void *stream);
int ts_debug_fill_id_lens(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0, int B, int T,
                          const int32_t *lens, void *stream);
/* Host-only (no GPU): the work list of a mixed pass's attention launch for the frame table frames_host (B,), 1 <= frames <= 65536.  Returns the
 * number n of workgroups (-1: bad table, or cap < n); out3 (n, 3) or NULL: workgroup i runs (clip, head, query tile of 64) or (-1, -1, -1).
 * Every tile with 64 tile < frames[clip] appears once; the tiles of one (clip, head) carry ids of equal residue mod 8 (one XCD); ids without a
 * tile pad the eight queues to equal length.  No reference counterpart. */
int ts_debug_face_mixed_grid(const int32_t *frames_host, int B, int heads, int32_t *out3, int cap);

/* ---- packed mixed face passes (csrc/face.cpp::face_packed_layout): the clips' own rows back to back ----
 * Host-only (no GPU): the row layout of a packed pass for ns_host / frames_host (B,).  feat_off (B + 1,): clip b's first row on the one time
 * axis of the feature convolutions at the conv0 rate (a multiple of 64; [B] = the total); row0 (B + 1,): its first transformer row ([B] = the
 * sum of frames); levels7: rows of level 0 .. 6 of the feature chain run as ONE problem (levels7[i] / levels7[i + 1] = Lin / Lout of
 * convolution i, k = 3 3 3 3 2 2, stride 2).  Any output may be NULL.  0, or -1: a bad table (ns < 400, frames < 1 or > 65536) or more rows
 * than the engines' int row indices hold. */
int ts_debug_face_packed_layout(const int32_t *ns_host, const int32_t *frames_host, int B, int64_t *feat_off, int64_t *row0, int64_t *levels7);
/* ts_face_generate_mixed with the row layout named: 0 = padded to the longest clip throughout, 1 = packed.  Same arguments, checks and outputs. */
int ts_debug_face_generate_mixed(ts_face *face, const float *wav_dev, const int32_t *ns_host, const int32_t *ns_dev,
                                 const int32_t *frames_host, const int32_t *frames_dev, int B, int N_max, int T_max, const float *id_dev,
                                 float *out_dev, float *hidden_dev, void *stream, int layout);
/* The packed pass's kernels (csrc/face.hip), one launch each; each builds its tables from the host tables and synchronizes `stream`.
 * ts_debug_attention_packed: qkv (sum frames, 3 HID), out (sum frames, HID), clip b in rows row0[b] .. row0[b] + frames[b]: the values of
 * ts_debug_attention_mixed on those rows. */
int ts_debug_attention_packed(const float *qkv, const int32_t *frames_host, const int32_t *frames_dev, int B, int HID, int heads, float scale,
                              float *out, void *stream);
/* dst (sum frames, C) row row0[b] + t = src (B, T_max, C) row (b, t), t < frames[b]; C % 4 == 0. */
int ts_debug_pack_rows(const float *src, const int32_t *frames_host, int B, int T_max, int C, float *dst, void *stream);
/* dst (B, T_max, C) row (b, t) = src row row0[b] + t for t < frames[b], +0.0 at and beyond: every element of dst is written. */
int ts_debug_unpack_rows(const float *src, const int32_t *frames_host, const int32_t *frames_dev, int B, int T_max, int C, float *dst,
                         void *stream);
/* ts_debug_w2v_conv0_lens writing out (feat_off[B], 512): clip b's rows from feat_off[b], zeros from its own count to feat_off[b + 1]. */
int ts_debug_w2v_conv0_packed(const float *wav, int B, int N, const int32_t *ns_host, const int32_t *ns_dev, const float *w,
                              const float *gamma, const float *beta, int form, float *out, void *stream);
/* ts_debug_lerp_ln_lens reading x (>= feat_off[B] / 64 rows, 512) with clip b's feature rows from feat_off[b] / 64; out (B, T, 512) padded. */
int ts_debug_lerp_ln_packed(const float *x, int B, int T, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_dev,
                            const float *gamma, const float *beta, float *out, void *stream);

/* Test aids: the stages of ts_mfcc_forward / ts_mfcc_forward_mixed after the resampler (csrc/mfcc.cpp, csrc/mfcc.hip), one production launch each
 * on `stream` with the handle's OWN tables (window, FFT twiddles, mel filterbank, DCT matrix; hop and rates as created).  Device pointers the
 * caller owns throughout; nothing is allocated or synchronized.  The resamplers have public entries (ts_mfcc_resample, ts_resample_kaiser and
 * their _mixed forms).  frames_dev: null = the uniform kernel; else the DEVICE table (B,) of the clips' own frame counts (the length variant:
 * rows at or beyond frames[b] are written as +0.0, the masked GEMMs may read but never use them, the dB kernel does not read them).  The table is
 * NOT checked: the caller keeps 1 <= frames[b] <= T (the kernels clamp a count to [0, T], so a bad table cannot take them outside the
 * buffers, but a clip of 0 rows has no maximum to clamp at).
 * ts_debug_mfcc_stft: x (B, N) at the OUTPUT rate -> power (B T, 1056), T = N / hop + 1: bins 0 .. 1024 of |STFT|^2 (center, reflect, periodic
 * Hann, n_fft 2048), then zeros.  N <= 1024 is refused like ts_mfcc_forward refuses it (reflect padding undefined). */
int ts_debug_mfcc_stft(ts_mfcc *m, const float *x, int B, long N, float *power, void *stream);
/* The length variant as production passes it: rows of N samples at the output rate, ns = the clips' sample counts at the INPUT rate (host and
 * device copies); clip b holds ts_mfcc_resampled_len of ns[b] samples (<= N, > 1024: checked on the host table) and that / hop + 1 frames. */
int ts_debug_mfcc_stft_lens(ts_mfcc *m, const float *x, const int32_t *ns_host, const int32_t *ns_dev, int B, long N, float *power,
                            void *stream);
/* frames_dev[b] = ts_mfcc_num_frames of ns_dev[b] (counts clamped to [0, N_max]): the row table of a mixed pass, made on the device. */
int ts_debug_mfcc_frames(ts_mfcc *m, const int32_t *ns_dev, int B, long N_max, int32_t *frames_dev, void *stream);
/* power (B T, 1056) -> mel (B T, 256): the HTK filterbank on conv_gemm_f32 (columns 1025 .. 1055 meet zero weights). */
int ts_debug_mfcc_mel(ts_mfcc *m, const float *power, const int32_t *frames_dev, int B, int T, float *mel, void *stream);
/* mel (B, T 256) in place: 10 log10(max(x, 1e-10)), clamped at the clip's own maximum - 80. */
int ts_debug_mfcc_db(ts_mfcc *m, float *mel, const int32_t *frames_dev, int B, int T, void *stream);
/* mel (B T, 256) -> feat (B T, 64): the orthonormal DCT-II on conv_gemm_f32. */
int ts_debug_mfcc_dct(ts_mfcc *m, const float *mel, const int32_t *frames_dev, int B, int T, float *feat, void *stream);
/* Wav sessions (talkshow_hip.h, "wav sessions"), stage by stage.  ts_debug_mfcc_stream_tap: every later call of the session also leaves its new
 * resampled samples in x22_dev (B rows of x22_ld, at their absolute index) and its new power rows in power_dev (B, power_rows, 1056) at their
 * frame index; a null pointer switches that tap off; a call that would write past a tap is refused.  ts_debug_mfcc_stream_tails: out[2] = the
 * input samples / resampled samples the session holds between calls.  ts_debug_mfcc_stream_db: the session's dB kernel on caller-owned
 * buffers, mel (B, F, 256) in place; peak (B,) = the peak mode, null = the running mode on run_max (B,), read and written. */
int ts_debug_mfcc_stream_tap(ts_mfcc_stream *h, float *x22_dev, long x22_ld, float *power_dev, long power_rows);
void ts_debug_mfcc_stream_tails(const ts_mfcc_stream *h, long out[2]);
int ts_debug_mfcc_stream_db(ts_mfcc *m, float *mel, int B, int F, const float *peak, float *run_max, void *stream);

/* Test aids: the stages of the SMPL-X forward pass of talkshow_hip.h (csrc/smplx.cpp, csrc/smplx.hip), one production launch each on `stream` with the handle's OWN
 * tables (pose offsets and mean, the three packed GEMM operands, parents, sparse skinning weights, selector and landmark maps).  Device pointers
 * the caller owns throughout; nothing is allocated or synchronized.  N <= 2^31 - 1 frames.
 * ts_debug_smplx_dims (host only): out5 = {Kpad = the GEMM depth (n_betas + n_expr + 9 (J - 1) rounded up to 32), U = needed vertices, KW = bones
 * kept per vertex, NJ = ts_smplx_num_joints, frames of one full-mesh chunk as ts_smplx_forward cuts them (for a call of more frames than that)}. */
int ts_debug_smplx_dims(const ts_smplx *m, int32_t *out5);
/* Host only: the U needed vertex ids in slot order (extra joints first, then landmark corners, each vertex once; {0} if the model has neither). */
int ts_debug_smplx_need(const ts_smplx *m, int32_t *verts_out);
/* rows (N, row_ld), betas (n_betas) or (N, n_betas) -> rot (N, J, 9) row-major rotation matrices, X (N, Kpad) = [betas | expression |
 * R_j - I for j >= 1 | +0.0].  row_ld and expr_off are checked as ts_smplx_forward checks them (talkshow_hip.h). */
int ts_debug_smplx_pose_prepare(ts_smplx *m, const float *betas, int betas_per_row, const float *rows, int row_ld, int expr_off, int64_t N,
                                float *rot_out, float *X_out, void *stream);
/* X (N, Kpad) -> which 0: the rest joints (N, 3 J) (the folded regressor); 1: the posed needed vertices (N, 3 U); 2: the posed mesh (N, 3 V)
 * (with_vertices models only).  The GEMM on conv_gemm_f32 as ts_smplx_forward issues it. */
int ts_debug_smplx_blend(ts_smplx *m, int which, const float *X, int64_t N, float *out, void *stream);
/* rot (N, J, 9), jrest (N, 3 J) -> G (N, J, 12) world transforms [R | t] by rows, A (N, J, 12) = [G.R | G.t - G.R J_j], joints (N, NJ, 3):
 * entries 0 .. J - 1 of every frame are written, the rest left alone. */
int ts_debug_smplx_rigid_chain(ts_smplx *m, const float *rot, const float *jrest, int64_t N, float *G_out, float *A_out, float *joints_out,
                               void *stream);
/* Linear blend skinning: vposed (N, 3 n), A (N, J, 12) -> out (N, 3 n); n = U with the needed vertices' weights (full == 0), V with the mesh's. */
int ts_debug_smplx_skin(ts_smplx *m, int full, const float *vposed, const float *A, int64_t N, float *out, void *stream);
/* vs (N, U, 3) skinned needed vertices -> entries J .. NJ - 1 of joints (N, NJ, 3): extra joints (copies), then landmarks (barycentric).
 * Launches nothing for a model without either. */
int ts_debug_smplx_joints_tail(ts_smplx *m, const float *vs, int64_t N, float *joints, void *stream);

/* Test aid: how many captured hipGraphs the PixelCNN keeps for `stream` right now (whole-call graphs of repeated shapes + the chunk
 * graphs that serve first-time shapes of any length; bounded, least recently used out first), or -1. */
int ts_debug_pixelcnn_graphs(ts_pixelcnn *pix, void *stream);

/* ---- code tables of the PixelCNN chain (csrc/code_tables.hip) ----
 * ts_debug_code_tables_plan (host only): the tables of a network of V codes and dim D under knob_list ("NAME=VALUE,...", null = defaults) and
 * the launches of code row r, column j of a pass of B clips that are lookups.  out12 = {tables fit (cap, kernels), the pass takes them, K-split
 * waves of slot V0, row sets per V0 table, bytes of the three V0 tables, waves of hg_0, bytes of the hg_0 table, slot V0 of row r is a lookup,
 * it writes the Q1 rider (row r+1 < last_row), it writes the Q0 rider (row r+2 < last_row), hg_0 of column j is a lookup, the cap in bytes}. */
int ts_debug_code_tables_plan(int V, int D, int B, int r, int j, int last_row, const char *knob_list, int64_t *out12);
/* TS_PIX_TABLES (-1 / 0 / 1) for one model object; builds the tables where wanted, drops the object's captured graphs.  mode -2 changes nothing.
 * Returns 1: tables exist, 0: not, -1: error. */
int ts_debug_pixelcnn_tables(ts_pixelcnn *pix, int mode);
/* A whole work buffer of `stream` (which = 0 HV, 1 OV0, 2 Q1, 3 Q0, 4 G; the per-pass audio terms 5 AE (B, H, D), 6 AEV (B, H, D), 7 AEH (B, H, D),
 * 8 AEH1 (B, H, 2D), 9 AV1C (B, H, 4D), 10 AV1P (B, H, 4D) of the latest pass of B clips and H rows, prefix included; 11 the token ring tok32
 * (B, R, 2) int32 words; 12 XV, 13 P, 14 V2H, 15 XH, 16 T0) copied to buf_dev (put = 0) or filled from it (put = 1); returns floats. */
int64_t ts_debug_pixelcnn_work(ts_pixelcnn *pix, void *stream, int which, float *buf_dev, int64_t cap_floats, int put);

/* ---- stage taps of the PixelCNN chain (csrc/pixelcnn.cpp: run_row / launch_row_slot; tests/test_gpu_pix_stages.py) ----
 * Test aid in the form of ts_debug_trunk_taps: makes the PRODUCTION pass copy out what every launch of a code row wrote; there is no second
 * code path.  The table is thread-local and one-shot: it applies to the next chain entry this thread makes — ts_pixelcnn_generate*,
 * ts_pixelcnn_generate_mixed*, ts_pixelcnn_stream_step*, called directly or from inside ts_body_pixel_infer* — and is dropped when that entry
 * returns, whether it succeeded or not.  taps == null drops a table that still waits.  Always returns 0.  With no table a pass issues
 * exactly what it issues without this entry.
 * GRAPHS: a tapped pass runs EAGERLY on the same run_row (the launches a TS_NO_GRAPH process issues).  It captures nothing, finds, adds
 * and evicts no graph of Work::graphs, and is no sighting for the hot-shape rule.  A one-shot call of more than CHUNK_ROWS rows without
 * a prefix runs in the whole call's configuration where its whole-call graph is cached, and as chunks otherwise.  That is NOT always the
 * untapped call's form: a pinned or hot shape whose graph is not cached (never captured yet, or just dropped) runs as a whole call
 * untapped, which captures, and as chunks tapped.  The bits of every stage are the same either way; the look-ahead sums differ: chunks
 * write P / Q1 / Q0 for rows past the end, a whole call does not.
 * Rows are ABSOLUTE code rows (a prefix counts, a session goes on counting).  row: the one row to tap, or -1: every row; only rows in
 * [row0, row0 + rows) are tapped.  slab_clips >= the clips of the pass (of a mixed pass: all of them); a pass of more clips fails.
 * stage[k]: DEVICE pointer or null.  Each holds `rows` records of units(k) slabs of S = round_up(slab_clips, 16) * width(k) floats:
 * unit u of row r at ((r - row0) * units(k) + u) * S.  A slab is the RAW copy of the launch's output block for its M rows of `stride`
 * floats: row-major M * stride floats, or, where the work buffer is tiled (tiled_width_of: networks with D % 128 == 0 unless
 * TS_SKINNY_TILED=0; tests decode with tiled_index of tests/test_gpu_chain_ops.py), the whole 16-row blocks of its tiled view of width tw
 * (element (m, n) = linear m * stride + n of that view).  Nothing else of a slab is written.  width = floats per clip of a slab.
 *   k  stage  units  width  M   stride  tw   unit u holds
 *   0  HV     NL     4D     B   4D      2D   layer u's pre-gate h_vert of row r, both columns [j][2D] (no class row), as vert_to_horiz reads it
 *   1  OV     NL     2D     B   2D      2D   layer u's gate output [j][D]: OV0, the XV_{u+1} slab, OVlast (u = NL - 1 >= 1: row-major)
 *   2  P      NL     4D     B   4D      0    u >= 1: Wprev_u . XV_u[r] + b, written FOR row r + 1 (none on a whole call's last row)
 *   3  Q1     1      4D     B   4D      0    W1 . E[r-1], written for row r + 1 (rows r >= 1 with r + 1 < last row)
 *   4  Q0     1      4D     B   4D      0    W0 . E[r-1], written for row r + 2 (rows r >= 1 with r + 2 < last row)
 *   5  V2H    NL     4D     2B  2D      0    vert_to_horiz of layer u, rows (clip, column) of 2D
 *   6  G      2 NL   D      B   D       D    u = 2 l + j: the horizontal gate output of layer l, column j
 *   7  XH     2 NL   D      B   D       D    u = 2 l + j, l >= 1: the horizontal input of layer l, column j (XH_1 folds fusion_h)
 *   8  T0     NL     2D     B   2D      0    u = l >= 1: Wh0_l . XH_l[0], column 0's launches only
 *   9  Y      2      HID    B   HID     HID  u = j: relu(output_conv.0)
 *  10  LG     2      V      B   V       0    u = j: the logits
 * Rows that run the vertical stack only (a prefix, teacher forcing without logits) leave stages 6 .. 10 alone. */
#define TS_DEBUG_PIX_TAP_STAGES 11
typedef struct ts_debug_pix_tap_table {
    int32_t row, row0, rows, slab_clips;
    float *stage[TS_DEBUG_PIX_TAP_STAGES];
} ts_debug_pix_tap_table;
int ts_debug_pixelcnn_taps(const ts_debug_pix_tap_table *taps);
/* One lookup launch on row-major caller buffers: which = 0 slot V0 (tok (B,2) int32; add1, add2 (B,4D) or null; cls (B,2D); pre (B,4D); out
 * (B,2D); q1, q0 (B,4D) or null), 1 hg_0 of column 1 (tok (B,2), column 0 read; add1 (B,2D) or null; cls (B,2D); out (B,D)). */
int ts_debug_code_table_stage(ts_pixelcnn *pix, int which, const int32_t *tok_dev, int B, const float *add1, const float *add2, const float *cls,
                              float *pre, float *out, float *q1, float *q0, void *stream);

/* Host-only (no GPU): the chunk plan of a mixed pass (talkshow_hip.h, "mixed passes").  hrows (B,) = code rows per clip, >= 1 and
 * non-increasing; max_counts = distinct active clip counts a pass may use (<= 0: the library's bound, 12).  active_out (ceil(hrows[0] / 8),)
 * or NULL: the clips chunk k = rows [8 k, 8 k + 8) runs with = #{b : hrows[b] > 8 k} rounded up to a multiple of the returned grid (capped
 * at B).  Returns the grid (1: nothing rounded; 2, 4, 8, ...: the smallest power of two that brings the distinct counts within the bound),
 * -1 on a bad table.  No reference counterpart. */
int ts_debug_mixed_plan(const int32_t *hrows, int B, int max_counts, int32_t *active_out);

/* Host-only (no GPU): the device records the library makes of n_rep (1 or B) public repetition records (talkshow_hip.h, "repetition
 * penalty"), four 32-bit words per clip slot into words_out (4 B,): window, presence, frequency (their bits) and from_row, which every
 * one-shot pass leaves 0 (only a streaming session sets it).  The rules of ts_repeat_check.  No reference counterpart. */
int ts_debug_rep_table(const ts_repeat *rep_host, int n_rep, int B, int V, int32_t *words_out);

/* Test aid: the paired, length-masked codebook search of a mixed pass on given latents (talkshow_hip.h, "given poses"; csrc/vq.hip:
 * vq_argmin_pair_lds_kernel).  z_body_dev (B H_max, dim_body), z_hand_dev (B H_max, dim_hand), lens_dev (B,) int32 POSE frame counts in any
 * order, codebooks (ncode, dim) in device memory -> codes_dev (B, H_max, 2) int64: column 0 / 1 = body / hand; row h of clip b holds what
 * ts_op_vq_argmin returns for that row of z if h < lens[b] / 4, else -1 (the row of z is then not read).  Networks with dim = 64 and one
 * ncode take the paired LDS kernel, every other pair two launches of the masked generic kernel. */
int ts_op_vq_argmin_pair_masked(ts_ctx *ctx, const float *z_body_dev, const float *z_hand_dev, const int32_t *lens_dev, int B, int H_max,
                                const float *codebook_body_dev, const float *codebook_hand_dev, int ncode_body, int ncode_hand, int dim_body,
                                int dim_hand, int64_t *codes_dev, void *stream);
/* The same with the launch form named — 0: the library's choice (TS_VQ_PAIR), 1: one paired launch, 2: one launch per network, 3: the masked
 * generic kernel — and `iters` >= 1 launches queued back to back ahead of the one synchronisation (tools/poses_pass.py times them). */
int ts_debug_vq_argmin_pair_masked(ts_ctx *ctx, const float *z_body_dev, const float *z_hand_dev, const int32_t *lens_dev, int B, int H_max,
                                   const float *codebook_body_dev, const float *codebook_hand_dev, int ncode_body, int ncode_hand,
                                   int dim_body, int dim_hand, int64_t *codes_dev, int form, int iters, void *stream);

/* ---- the Winograd F(4,3) lowering of wide stride-1 k = 3 C -> C layers (csrc/conv_wino.hip; knob TS_CONV_WINO) ----
 * Host-only (no GPU): is a conv layer of this geometry (padding k / 2) lowered under knob_list ("TS_CONV_WINO=1", null = the defaults), and
 * into what?  Returns 1 / 0 (lowered / direct), -1 on a bad argument; lowered: out5 = {GEMMs per network (6), their rows M = B ceil(L / 4),
 * columns N, depth K, rows of a tile (4)}.  The answer never depends on B or L (they only size M).  No reference counterpart. */
int ts_debug_wino_lowering(int cin, int cout, int k, int stride, const char *knob_list, int B, int L, int *out5);
/* Host-only: the six transformed matrices U_i = sum_k G[i][k] g_k of taps w (cout, cin, 3) (the reference's weight layout, BatchNorm
 * already folded), computed in double and rounded once to fp32, as the library packs them: out (6, round_up(cout, 128), cin), rows at or
 * beyond cout zero. */
int ts_debug_wino_weights(const float *w, int cout, int cin, float *out);
/* Test aid: ONE launch of a transform kernel on device buffers the caller owns.  which 0 wino_in: x (B, L, C) -> V (6, B J, C), J = ceil(L / 4);
 * 1 wino_out: O (6, B J, C), bias (C,), res (B, L, C) or null -> y (B, L, C) = act(At O + bias (+ res)), every row written; 2 wino_out_in: O,
 * bias -> V of the next layer, = 1 then 0 without storing y.  ptrs: 12 device pointers {x, V, O, bias, res, y} of network 0 then of network 1
 * (nnet = 1: the second six are not read).  lens_dev (B,) int32 or null: clip b has min(L, (lens[b] >> shr) << shl) rows; rows beyond read as
 * zeros and are stored as zeros.  act: 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 GELU.  Does not synchronize. */
int ts_debug_wino_transform(ts_ctx *ctx, int which, int nnet, int B, int L, int C, int act, const int32_t *lens_dev, int shr, int shl,
                            const void *const *ptrs, void *stream);
/* Test aid: the six GEMMs per network of a lowered layer, O_i = V_i U_i^T, as the library launches them (one batched conv_gemm_f32 launch).
 * V / O (6, M, C), U (6, round_up(C, 128), C) of ts_debug_wino_weights, device pointers; the *1 of nnet = 1 are not read.  Does not synchronize. */
int ts_debug_wino_gemm(ts_ctx *ctx, int nnet, const float *V0, const float *V1, const float *U0, const float *U1, float *O0, float *O1, int M,
                       int C, void *stream);
/* ---- the VQ decoders' first lowered layer from per-code tables (conv_wino.hip::wino_codes; knob TS_VQ_DEC_TABLES) ----
 * Test aid: ONE launch of wino_codes on device buffers the caller owns.  codes (B, L) int64, T (6, ncode, C), O (6, B J, C), J = ceil(L / 4):
 * O_i[b J + j] = sum_k Bt[i][k] T_i[codes[b][4j - 1 + k]] in wino_in's pinned order; a row outside [0, L_b) is the zero row and its code is
 * not read, a code outside [0, ncode) is the zero row.  lens_dev, shr, shl as for ts_debug_wino_transform.  Does not synchronize. */
int ts_debug_wino_codes(ts_ctx *ctx, int nnet, int B, int L, int C, const int32_t *lens_dev, int shr, int shl, const int64_t *codes0,
                        const int64_t *codes1, const float *T0, const float *T1, int ncode0, int ncode1, float *O0, float *O1, void *stream);
/* Test aid: 1 where the network decodes its first stack from tables, 0 where not (nothing is written), -1 on an error.  Copies to HOST
 * buffers, each optional: tables (6, ncode, hid), aft_table (ncode, hid) and u (6, round_up(hid, 128), hid), the first layer's Winograd
 * matrices the tables were multiplied by; *tables_dev = the tables' device address.  Synchronizes. */
int ts_debug_vqvae_dec_tables(ts_vqvae *vq, float *tables, float *aft_table, float *u, const float **tables_dev);

/* ---- stage taps of the conv trunks (csrc/models.cpp: run_trunk_n, vq_decode_n; tests/test_gpu_vq_stages.py) ----
 * Test aid: makes the PRODUCTION pass copy every stage's output to caller buffers; there is no second code path.  The table is thread-local
 * and one-shot: it applies to the next pass entry this thread makes — ts_audioenc_forward [_masked], ts_vqvae_encode / _decode / _decode_z /
 * _forward, ts_body_vq_infer [_mixed], ts_vqvae_decode_pair [_masked], ts_vqvae_encode_pair_masked, called directly or from inside another entry
 * (ts_body_pixel_infer runs three of them: set the table right ahead of the call it is meant for) — and is dropped when that entry returns,
 * whether it succeeded or not.  taps == null drops a table that still waits.  Always returns 0.
 * enc[i][k] / dec[i][k]: DEVICE pointers, each may be null; i = the network's index in a paired pass (0 body, 1 hand; a single network is
 * 0).  Stage k of the encoder trunk / of the decoder:
 *   0  project                       | the decoder's first layer (the aft_vq table gather, or aft_vq_conv on continuous latents)
 *   1  _enc_1    2  _down_1          | 1  _dec_1    2  _up_2
 *   3  _enc_2    4  _down_2          | 3  _dec_2    4  _up_3
 *   5  _enc_3                        | 5  _dec_3
 * (z and the decoder's project are outputs already.)  Each tap is one hipMemcpyAsync, device to device on the pass's stream right after the
 * stage's last launch, of the dense (B, L_stage, C_stage) block the stage left in the arena: encoder L = T, T, T/2, T/2, T/4, T/4 and
 * C = hid/4, hid/4, hid/2, hid/2, hid, hid; decoder L = H, H, 2H, 2H, 4H, 4H and C = hid, hid, hid/2, hid/2, hid/4, hid/4; a masked pass
 * copies the rows of T_max / H.  With no table a pass issues exactly what it issues without this entry. */
typedef struct ts_debug_trunk_tap_table {
    float *enc[2][6];
    float *dec[2][6];
} ts_debug_trunk_tap_table;
int ts_debug_trunk_taps(const ts_debug_trunk_tap_table *taps);

/* ---- seamless sessions (csrc/body_stream.cpp; talkshow_hip.h, "seamless sessions") ----
 * Host-only (no GPU): one call of the window plan on given counters.  state4 = {frames received F, code rows done A, code rows whose poses
 * are out D, flushed}; a push of t >= 1 frames (flush = 0) or the flush (flush != 0, t = 0); enc_lowered != 0: the plan of a session whose
 * audio encoder is Winograd-lowered (an encoder reach of 14 code rows in place of 7).  out14 = {F, A, D, flushed after the call;
 * encoder window frames [f0, f1) (empty: no call); code rows [A0, A1) the call finalises; decoder window code rows [v0, v1) (empty: no
 * call); code rows [D0, D1) whose poses come out; the first MFCC frame and the first code row a later call can still read}.  The
 * arithmetic talkshow_amd/streaming.py::SeamlessPlan restates.  No reference counterpart. */
int ts_debug_body_stream_plan(const int64_t *state4, int t, int flush, int enc_lowered, int64_t *out14);
/* Test aids: the three staging kernels of a session (csrc/body_stream.hip), ONE call of the launcher each on `stream`, device pointers the
 * caller owns throughout; nothing is allocated or synchronized.  Every shape outside the buffers is refused by the launcher (nonzero, nothing
 * launched); a call of zero elements returns 0 and launches nothing.
 * ts_debug_stream_stage_mfcc: per clip the concatenation [tail (B, cap, 64) rows [0, n_tail) | chunk (B, t, 64)]: frames [0, Tw) -> win
 * (B, Tw, 64), frames [next0, next0 + n_next) -> next (B, cap, 64) rows [0, n_next) (rows beyond are not written).  tail != next; n_tail,
 * n_next <= cap; Tw, next0 + n_next <= n_tail + t; every pointer 16-byte aligned. */
int ts_debug_stream_stage_mfcc(const float *tail, const float *chunk, float *win, float *next, int B, int n_tail, int t, int cap, int Tw,
                               int next0, int n_next, void *stream);
/* codes (B, n, 2) = code rows [A, A + n) -> ring (B, RC, 2), row r at slot r % RC (the other slots are left alone); rows [v0, v0 + Hw) -> column
 * 0 / 1 into lat_body / lat_hand (B, Hw), a row at or beyond A from `codes`, an earlier one from the ring.  v0 <= A, A + n - v0 <= RC,
 * v0 + Hw <= A + n; codes and ring 16-byte aligned. */
int ts_debug_stream_emit(const int64_t *codes, int64_t *ring, int64_t *lat_body, int64_t *lat_hand, int B, int n, int A, int RC, int v0, int Hw,
                         void *stream);
/* dst (B, n, W) = rows [r0, r0 + n) of every clip of src (B, R, W); r0 + n <= R.  16-byte copies where W % 4 == 0 and both pointers are 16-byte
 * aligned, word by word otherwise: the same bits either way. */
int ts_debug_stream_keep_rows(const float *src, float *dst, int B, int R, int r0, int n, int W, void *stream);
/* stream_spread_rows_kernel on its own: dst (S, n, W) = rows [r0, r0 + n) of stream map_host[s] of src (E, R, W); W a multiple of 4, both
 * blocks 16-byte aligned; map_host (S,) with values in [0, E), checked here.  Waits for the launch. */
int ts_debug_stream_spread_rows(const float *src, float *dst, const int32_t *map_host, int S, int E, int R, int r0, int n, int W, void *stream);

/* ---- the glue kernels of the VQ and PixelCNN passes (csrc/vq.hip) ----
 * Test aids: ONE call of the production launcher each on `stream`, device pointers the caller owns throughout; nothing is allocated or
 * synchronized.  A null pointer or a row count < 1 is refused here, everything else by the launcher (nonzero, nothing launched).
 * ts_debug_gather_rows: out[m][0 .. width) = table[idx[m idx_stride]][0 .. width) for m < M; table rows ld_table floats apart, out rows ldo (the
 * floats of a row at and beyond width are not written); an index outside [0, nrows) gives a row of NaN.  width, ld_table, ldo % 4 == 0.
 * lens == NULL and L == 0: the plain kernel.  Otherwise the masked one (lens a DEVICE table (M / L,), M % L == 0, len_shr >= 0): row m = b L + t
 * with t >= lens[b] >> len_shr is a row of +0.0 and its index is not read. */
int ts_debug_gather_rows(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M, int width, float *out,
                         int ldo, int L, const int32_t *lens, int len_shr, void *stream);
/* dst[m][0 .. cpad) = src[m][0 .. c) then +0.0, for the M = B L rows m = b L + t; src rows lds floats apart, dst rows ldd (floats at and beyond
 * cpad are not written); source columns >= c are not read.  lens (DEVICE (B,)) or NULL: rows t >= lens[b] are rows of +0.0, not read. */
int ts_debug_pad_rows(const float *src, int lds, int c, float *dst, int ldd, int cpad, int B, int L, const int32_t *lens, void *stream);
/* Rows r >= lens[b] >> 2 of codes (B, H, 2) int64 become -1 (launch_mask_codes), of logprob (B, H, 2) +0.0 (launch_mask_logprob); the rows
 * below are left alone.  Either block may be NULL, not both. */
int ts_debug_mask_rows(int64_t *codes, float *logprob, int B, int H, const int32_t *lens, void *stream);
/* dst[i] = first + i, i < n. */
int ts_debug_iota_i64(int64_t *dst, int n, int64_t first, void *stream);
/* dst[i] = (int32) src[i], i < n. */
int ts_debug_i64_to_i32(const int64_t *src, int32_t *dst, long n, void *stream);
/* dst[0 .. 2] = a, b, c, carried by the launch's own arguments. */
int ts_debug_set_words3(uint64_t *dst, uint64_t a, uint64_t b, uint64_t c, void *stream);
/* "slot state" (talkshow_hip.h): slot_save_kernel / slot_load_kernel alone on caller buffers in a session's shapes — tok32 (B, 4, 2) int32,
 * Q1 / Q0 (4, B, 4D), P (NL, 2, B, 4D), CR (NL, B, 2D), bv (NL, 4D), rep_ring (B, 2, 64) int32, tables (NL, NC, 2D), state rows of
 * 12 D + (NL - 1) 4 D + NL 2 D + 136 words.  slots / hist / index / origin are DEVICE tables (n,).  open_labels (B,) int64 with tables, or
 * both NULL.  A slot outside [0, B) or an index outside [0, n_states) writes nothing. */
int ts_debug_slot_save(const int32_t *slots, const int32_t *hist, int n, int B, int row, int D, int NL, int NC, const int32_t *tok32,
                       const float *Q1, const float *Q0, const float *P, const float *CR, const float *bv, const int32_t *rep_ring,
                       const int64_t *open_labels, const float *tables, float *state, void *stream);
int ts_debug_slot_load(const int32_t *slots, const int32_t *index, const int32_t *origin, int n, int n_states, int B, int row, int D, int NL,
                       int32_t *tok32, float *Q1, float *Q0, float *P, float *CR, int32_t *rep_ring, int32_t *row_origin, const float *state,
                       void *stream);
/* out[j] = sum over c ascending of e[j][c]^2 in fp32, e (n, dim) dense. */
int ts_debug_row_sqnorm(const float *e, int n, int dim, float *out, void *stream);

/* Tuning entry (not part of the drop-in surface): `iters` DEPENDENT skinny_gemm launches replayed from one hipGraph;
 * *us_out = microseconds per launch.  gate != 0: N = 2K with the tanh*sigmoid epilogue; debug: unused. */
int ts_debug_skinny_chain(ts_ctx *ctx, int M, int K, int gate, int iters, int debug, float *us_out);

#ifdef __cplusplus
}
#endif
#endif /* TALKSHOW_HIP_DEBUG_H */
