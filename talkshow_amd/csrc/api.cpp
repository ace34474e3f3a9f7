// Whole-wrapper entry points and the single-operator entry points used by the kernel-level parity tests.
#include <cstring>
#include <vector>
#include "host_common.h"
#include "conv_tile.h"
#include "skinny_desc.h"

using namespace ts;

namespace {
struct BodyWork {
    DevBuf feat;
    DevBuf lat[2];
    DevBuf given;   // ts_body_pixel_infer_mixed_poses: the code rows its encoders produce, (B, H_max, 2) int64 — the pass's given block
};
// scratch between the stages of ts_body_pixel_infer (audio feature map, split latents), one set per stream
BodyWork &body_work(hipStream_t s) {
    static StreamWorks<BodyWork> works;
    return works.get(s);
}
}  // namespace

namespace ts {
// the TS_* levers as `get` (NAME -> value text or null) reports them
template <class Get>
static Knobs read_knobs(Get get) {
    Knobs v;
    auto num = [&](const char *name, int dflt) { const char *e = get(name); return e && e[0] ? std::atoi(e) : dflt; };
    v.conv_bands = num("TS_CONV_BANDS", 1) != 0;
    v.conv_ring = num("TS_CONV_RING", 9);
    v.conv_deal = num("TS_CONV_DEAL", 1) != 0;
    v.conv_ring_paired = num("TS_CONV_RING_PAIRED", 1) != 0;
    v.conv_taps48 = num("TS_CONV_TAPS48", 1) != 0;
    v.face_pack = num("TS_FACE_PACK", 0) != 0;
    v.conv_sk = num("TS_CONV_SK", 1);
    v.conv_wino = num("TS_CONV_WINO", -1);
    v.vq_dec_tables = num("TS_VQ_DEC_TABLES", -1);
    v.wino_deal = num("TS_WINO_DEAL", 1) != 0;
    v.w2v_moments = num("TS_W2V_MOMENTS", 1) != 0;
    v.vq_lds = num("TS_VQ_LDS", 1) != 0;
    v.vq_pair = num("TS_VQ_PAIR", 1) != 0;
    v.split_xcd = num("TS_SPLIT_XCD", 8);
    v.prof_log = num("TS_PROF_LOG", 0) != 0;
    if (const char *e = get("TS_NO_GRAPH")) v.no_graph = e[0] && e[0] != '0';
    v.pix_defer_p = num("TS_PIX_DEFER_P", -1);
    v.pix_tables = num("TS_PIX_TABLES", -1);
    v.skinny_v = num("TS_SKINNY_V", 1);
    v.skinny_nt = num("TS_SKINNY_NT", 16);
    v.skinny_tiled = num("TS_SKINNY_TILED", 1) != 0;
    v.wide_min = num("TS_SKINNY_WIDE_MIN", 160);
    v.skinny_shape = num("TS_SKINNY_SHAPE", 0);
    v.skinny_trace = num("TS_SKINNY_TRACE", 0);
    v.wide_ablate = num("TS_SKINNY_WIDE_ABLATE", 0);
    v.wide_pair = num("TS_SKINNY_WIDE_PAIR", 1) != 0;
    return v;
}
const Knobs &knobs() {
    static const Knobs k = read_knobs([](const char *name) { return std::getenv(name); });
    return k;
}
// the plan debug entries: the levers of a "NAME=VALUE,NAME=VALUE" list (null: the defaults), read by the same table as the environment
static Knobs knobs_from_list(const char *list) {
    return read_knobs([list](const char *name) -> const char * {
        const size_t n = std::strlen(name);
        for (const char *q = list; q && (q = std::strstr(q, name)); q += n)
            if ((q == list || q[-1] == ',' || q[-1] == ' ') && q[n] == '=') return q + n + 1;
        return nullptr;
    });
}
}  // namespace ts

extern "C" {

// Streams for pipelining independent batches.  Created back to back so that ROCclr's round-robin hands consecutive
// streams distinct hardware queues (GPU_MAX_HW_QUEUES); hosts without a stream pool of their own use these.
int ts_stream_create(ts_ctx *ctx, void **out) {
    if (!ctx || !out) return fail("ts_stream_create: null argument");
    TS_HIP(hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    TS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return 0;
}
// A stream whose kernels only run on compute units [cu_first, cu_first + cu_count) of the device's CU-mask index space
// (consecutive mask bits are spread round-robin over the 8 XCDs).  Used to keep the latency-bound PixelCNN chain and the
// MFMA-bound conv stacks of different batches off each other's CUs.
int ts_stream_create_cus(ts_ctx *ctx, int cu_first, int cu_count, void **out) {
    if (!ctx || !out) return fail("ts_stream_create_cus: null argument");
    TS_HIP(hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    TS_HIP(hipGetDeviceProperties(&prop, ctx->device));
    const int ncu = prop.multiProcessorCount;
    if (cu_first < 0 || cu_count < 1 || cu_first + cu_count > ncu) return fail("ts_stream_create_cus: CU range outside the device");
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int i = cu_first; i < cu_first + cu_count; ++i) mask[i / 32] |= 1u << (i % 32);
    hipStream_t s = nullptr;
    TS_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    *out = s;
    return 0;
}
// Output assembly after both generators (scripts/demo.py:207-229, data_utils/lower_body.py:68-87)
int ts_assemble_full(ts_ctx *ctx, const float *body, int Tb, const float *face, int Tf, int B, const float *lower_pose33,
                     float *out, void *stream) {
    if (!ctx || !body || !face || !lower_pose33 || !out) return fail("ts_assemble_full: null argument");
    if (B < 1 || Tb < 1 || Tf < 1) return fail("ts_assemble_full: empty input");
    MiscScope ms(ctx, (hipStream_t)stream);
    TS_HIP(launch_assemble_full(body, face, lower_pose33, B, Tb, Tf, out, (hipStream_t)stream));
    return 0;
}

// The same for clips of different lengths (talkshow_hip.h): the tables are read on the device only
int ts_assemble_full_mixed(ts_ctx *ctx, const float *body, const int32_t *tb_dev, const float *face, const int32_t *tf_dev, int B, int Tb_max,
                           int Tf_max, const float *lower_pose33, float *out, void *stream) {
    if (!ctx || !body || !face || !lower_pose33 || !out) return fail("ts_assemble_full_mixed: null argument");
    if (!tb_dev || !tf_dev) return fail("ts_assemble_full_mixed: null length table");
    if (B < 1 || Tb_max < 1 || Tf_max < 1) return fail("ts_assemble_full_mixed: empty input");
    MiscScope ms(ctx, (hipStream_t)stream);
    TS_HIP(launch_assemble_full_lens(body, tb_dev, face, tf_dev, lower_pose33, B, Tb_max, Tf_max, out, (hipStream_t)stream));
    return 0;
}

// Host-only (no GPU): the code tables of a PixelCNN of V codes and dim D under knob_list, and which launches of code row r, column j of a
// pass of B clips are lookups.  out12 = {the tables fit, the pass takes them, K-split waves of V0, row sets per V0 table, bytes of the three
// V0 tables, waves of hg_0, bytes of the hg_0 table, slot V0 of row r is a lookup, it writes the Q1 rider, it writes the Q0 rider, hg_0 of
// column j is a lookup, the cap in bytes}
int ts_debug_code_tables_plan(int V, int D, int B, int r, int j, int last_row, const char *knob_list, int64_t *out12) {
    if (!out12 || B < 1 || r < 0 || j < 0 || j > 1) return fail("ts_debug_code_tables_plan: bad argument");
    const Knobs k = knob_list ? ts::knobs_from_list(knob_list) : Knobs();
    const ts::CodeTablePlan t = ts::code_table_plan(V, D, k);
    const bool takes = ts::code_table_pass(t.fits && k.pix_tables != 0, k.pix_tables, B);
    const bool v0 = takes && ts::code_table_v0_row(r);
    const int64_t o[12] = {t.fits, takes, t.waves_v0, t.sets_v0, (int64_t)t.bytes_v0, t.waves_hg, (int64_t)t.bytes_hg, v0,
                           v0 && ts::code_table_rider(r, 1, last_row), v0 && ts::code_table_rider(r, 0, last_row),
                           takes && ts::code_table_hg_col(j), (int64_t)ts::CODE_TABLE_CAP_BYTES};
    for (int i = 0; i < 12; ++i) out12[i] = o[i];
    return 0;
}

// tuning aid (TS_SKINNY_TRACE=1): in-kernel wall-clock stamps of the PixelCNN chain kernel, 6 u64 per record
int ts_debug_skinny_trace(unsigned long long *out, int max_records) {
    if (!out) return -1;
    return ts::skinny_trace_read(out, max_records);
}
// measurement aid: a one-wave kernel on `stream` that records the shader clock the chip runs at, every window_us, n times
int ts_debug_clock_sample(unsigned long long *dev_out, int n, int window_us, void *stream) {
    if (!dev_out || n < 1 || window_us < 1) return fail("ts_debug_clock_sample: bad argument");
    TS_HIP(ts::launch_clock_sample(dev_out, n, (unsigned long long)window_us * 100, (hipStream_t)stream));
    return 0;
}
// Host-only (no GPU): the launch plan of an (M x N, `groups` problems) conv layer — out4 = {row blocks of 128 x 128 tiles, row blocks of
// 64 x 128 tiles, workgroups of the first band, workgroups}; returns 1 if the layer is launched in two bands, 0 for a plain grid
int ts_debug_conv_bands(int M, int N, int groups, int *out4) {
    if (M < 1 || N < 1 || groups < 1 || groups > 4 || !out4) return fail("ts_debug_conv_bands: bad argument") ? -1 : -1;
    ts::ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M;
    p.N = N;
    p.ngroups = groups;
    const ts::ConvPlan pl = ts::plan_conv(p, 0, ts::knobs_from_list("TS_CONV_RING=0"), false);
    const ts::ConvBands &bd = pl.bands;
    out4[0] = bd.mt_big; out4[1] = bd.mt_small; out4[2] = bd.first_small; out4[3] = bd.total;
    return pl.engine == ts::ConvEngine::RegBanded ? 1 : 0;
}
// Host-only (no GPU): tile (out2 = {row tile, column tile}) that workgroup `bid` of conv_gemm_split's 1-D grid works on for an MT x NT
// tile grid and column groups of `gw` tiles; returns 1, 0 if that workgroup has no tile, -1 on a bad argument
int ts_debug_split_tile(int bid, int MT, int NT, int gw, int *out2) {
    if (bid < 0 || MT < 1 || NT < 1 || gw < 1 || !out2) return fail("ts_debug_split_tile: bad argument") ? -1 : -1;
    return ts::split_tile_of(bid, MT, NT, gw, out2[0], out2[1]) ? 1 : 0;
}
int ts_debug_tile_weights(const float *W, int N, int K, long ldw, int epi, int gateD, float *out) {
    if (!W || !out || N < 1 || K < 16 || K % 16 || ldw < K) return fail("ts_debug_tile_weights: bad argument");
    if (epi == ts::EPI_GATE && (gateD < 8 || gateD % 8 || N % (2 * gateD))) return fail("ts_debug_tile_weights: gate tiles need gateD % 8 == 0 and N % (2 gateD) == 0");
    ts::skinny_tile_weights(W, N, K, ldw, epi, gateD, out);
    return 0;
}
int ts_stream_destroy(ts_ctx *ctx, void *stream) {
    if (!ctx) return fail("ts_stream_destroy: null ctx");
    TS_HIP(hipStreamSynchronize((hipStream_t)stream));
    drop_stream_everywhere((hipStream_t)stream);   // scratch arenas and captured graphs keyed by this handle
    TS_HIP(hipStreamDestroy((hipStream_t)stream));
    return 0;
}

// s2g_body_pixel.TrainWrapper.infer_on_audio, device part (nets/smplx_body_pixel.py:272-285)
int ts_body_pixel_infer(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc,
                        const int64_t *ids, int B, int T, int mode, const float *uniforms, uint64_t seed, int64_t clip0,
                        int64_t *codes, float *poses, void *stream) {
    if (!ae || !pix || !vb || !vh || !mfcc || !ids || !codes || !poses) return fail("ts_body_pixel_infer: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int H = (T / 2) / 2;
    if (H < 1) return fail("ts_body_pixel_infer: clip too short");
    const int aud_dim = convnet_hidden(ae), body_dim = vqvae_in_dim(vb), hand_dim = vqvae_in_dim(vh);
    BodyWork &w = body_work(s);
    TS_TRY(w.feat.ensure((size_t)B * H * aud_dim * sizeof(float)));
    TS_TRY(ts_audioenc_forward(ae, mfcc, B, T, w.feat.f(), s));
    TS_TRY(ts_pixelcnn_generate(pix, ids, w.feat.f(), B, H, mode, uniforms, seed, clip0, codes, nullptr, nullptr, nullptr,
                                0, s));
    // body_latents = latents[..., 0]; hand_latents = latents[..., 1]  (:279-280)
    for (int k = 0; k < 2; ++k) {
        TS_TRY(w.lat[k].ensure((size_t)B * H * sizeof(int64_t)));
        TS_HIP(hipMemcpy2DAsync(w.lat[k].p, sizeof(int64_t), codes + k, 2 * sizeof(int64_t), sizeof(int64_t),
                                (size_t)B * H, hipMemcpyDeviceToDevice, s));
    }
    (void)body_dim;
    (void)hand_dim;
    return ts_vqvae_decode_pair(vb, vh, static_cast<int64_t *>(w.lat[0].p), static_cast<int64_t *>(w.lat[1].p), B, H, poses, s);
}

// the scope every sampling control shares (sampling records, code bias, repetition penalty); `who` names the entry in the message
static int ctl_mode_check(const std::string &who, int mode) {
    if (mode == TS_SAMPLE_UNIFORMS || mode == TS_SAMPLE_PHILOX) return 0;
    return fail(who + ": sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip greedy is top_k = 1)");
}

// What every mixed body entry refuses before its first launch: null arguments, the shape, the length table (within T_max, at least one code
// row, non-increasing) and the sampling records; `who` names the entry in the messages.  A pass under a "speaker style" does not read the
// speaker ids: the style block takes their place
static int body_mixed_check(const char *who, const void *ae, const void *pix, const void *vb, const void *vh, const float *mfcc, const MixedPass &a,
                            const float *poses, const MixedOpts &o) {
    const std::string w(who);
    const int B = a.B, T_max = a.rows;
    if (!ae || !pix || !vb || !vh || !mfcc || !(o.style ? static_cast<const void *>(o.style) : a.ids) || !a.lens_host || !a.lens_dev || !a.codes || !poses)
        return fail(w + ": null argument");
    if (B < 1) return fail(w + ": bad shape");
    if ((T_max / 2) / 2 < 1) return fail(w + ": T_max too short");
    for (int b = 0; b < B; ++b) {
        if (a.lens_host[b] > T_max) return fail(w + ": clip " + std::to_string(b) + " is longer than T_max");
        if (a.lens_host[b] < 4) return fail(w + ": clip " + std::to_string(b) + " is shorter than 4 frames (one code row)");
        if (b > 0 && a.lens_host[b] > a.lens_host[b - 1])
            return fail(w + ": lengths must be non-increasing (clip " + std::to_string(b) + " is longer than the one before it)");
    }
    if (o.ctl_host) {   // a bad record or mode is refused before the first launch of the pass
        TS_TRY(ctl_mode_check(w + "_ctl", a.mode));
        if (o.n_ctl != 1 && o.n_ctl != B) return fail(w + "_ctl: n_ctl must be 1 or B");
        if (ts_sampling_check(o.ctl_host, o.n_ctl, 1) != 0) return 1;   // the records; the vocabulary is checked by the PixelCNN's pass
    }
    return 0;
}

// What the body entries refuse of a "code bias" before their first launch: the mode (the bias shares the sampling table's scope) and the
// index table
static int body_bias_check(const char *who, int mode, int B, int n_bias, const int32_t *bias_index_host) {
    TS_TRY(ctl_mode_check(who, mode));
    if (!bias_index_host) return fail(std::string(who) + ": the tables need their index table");
    return ts_code_bias_index_check(bias_index_host, B, n_bias);
}

// What the body entries refuse of a "repetition penalty" before their first launch: the mode (a sampling control, like the bias), the
// number of records and the records themselves
static int body_repeat_check(const char *who, int mode, int B, int V, const ts_repeat *rep_host, int n_rep) {   // V = 1: the vocabulary is
                                                                                                                // checked by the pass itself
    TS_TRY(ctl_mode_check(who, mode));
    if (n_rep != 1 && n_rep != B)
        return fail(std::string(who) + ": a pass of " + std::to_string(B) + " clips brings 1 or " + std::to_string(B) + " repetition records, got " +
                    std::to_string(n_rep));
    return ts_repeat_check(rep_host, n_rep, V);
}

// What the body entries refuse of "guidance" before their first launch, the audio encoder's: the mode (a sampling control, like the bias) and
// the tables, by the one rule the pass behind them applies again (ts_guide_check: one source for every message)
static int body_guide_check(const char *who, int mode, int B, const MixedOpts &o, const int32_t *lens_host) {
    TS_TRY(ctl_mode_check(who, mode));
    return ts_guide_check(o.guide_host, o.guide_scale_host, lens_host, B);
}

// The body of every ts_body_pixel_infer_mixed* entry without given poses (a.rows = T_max): each entry fills `o` with its own arguments
static int body_mixed(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const MixedPass &a, float *poses,
                      const MixedOpts &o, hipStream_t s) {
    TS_TRY(body_mixed_check("ts_body_pixel_infer_mixed", ae, pix, vb, vh, mfcc, a, poses, o));
    const int B = a.B, H = (a.rows / 2) / 2;
    TS_TRY(mixed_style_rows_check("ts_body_pixel_infer_mixed", "T_max / 4", o, H));
    if (o.bias && body_bias_check("ts_body_pixel_infer_mixed_bias", a.mode, B, o.n_bias, o.bias_index_host) != 0) return 1;
    if (o.rep_host && body_repeat_check("ts_body_pixel_infer_mixed_repeat", a.mode, B, 1, o.rep_host, o.n_rep) != 0) return 1;
    TS_TRY(mixed_given_check("ts_body_pixel_infer_mixed_keep", "ts_body_pixel_infer_mixed_given", o, a.lens_host, B));   // a bad row table is refused before the first launch of the pass, too
    if (o.guide_host && body_guide_check("ts_body_pixel_infer_guided", a.mode, B, o, a.lens_host) != 0) return 1;
    if (o.alt) {   // last, and ahead of the audio encoder's launches
        if (ts_alt_check(o.alt, a.mode) != 0) return 1;
        if (!o.logprob) return fail("ts_body_pixel_infer_alt: the record needs logprob_dev beside it");
    }
    BodyWork &w = body_work(s);
    TS_TRY(w.feat.ensure((size_t)B * H * convnet_hidden(ae) * sizeof(float)));
    TS_TRY(ts_audioenc_forward_masked(ae, mfcc, a.lens_dev, B, a.rows, w.feat.f(), s));
    MixedPass rows = a;
    rows.rows = H;
    TS_TRY(pixelcnn_generate_mixed(pix, w.feat.f(), rows, o, s));
    for (int k = 0; k < 2; ++k) {
        TS_TRY(w.lat[k].ensure((size_t)B * H * sizeof(int64_t)));
        TS_HIP(hipMemcpy2DAsync(w.lat[k].p, sizeof(int64_t), a.codes + k, 2 * sizeof(int64_t), sizeof(int64_t),
                                (size_t)B * H, hipMemcpyDeviceToDevice, s));
    }
    return ts_vqvae_decode_pair_masked(vb, vh, static_cast<int64_t *>(w.lat[0].p), static_cast<int64_t *>(w.lat[1].p), a.lens_dev, B, H,
                                       poses, s);
}

// The same path for clips of different lengths in ONE pass (talkshow_hip.h: "mixed passes"): length-masked conv stacks, the chain over
// a shrinking prefix of the clips, documented padding in both outputs.
int ts_body_pixel_infer_mixed(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                              const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                              uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, void *stream) {
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, MixedOpts(), (hipStream_t)stream);
}

// the same pass with per-clip sampling controls (ctl_host == NULL: exactly the entry above)
int ts_body_pixel_infer_mixed_ctl(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                  const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                  uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                  void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass with a log-probability output (B, T_max / 4, 2); logprob == NULL: exactly the entry above
int ts_body_pixel_infer_mixed_lp(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                 const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                 uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                 float *logprob, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass in which clip b brings given_rows[b] code rows (given (B, T_max / 4, 2)); given == NULL: exactly the entry above
int ts_body_pixel_infer_mixed_given(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                    const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                    uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                    void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the given pass with a mask of kept positions (talkshow_hip.h, "kept positions"; keep (B, T_max / 4, 2) uint8); keep == NULL: exactly the
// entry above
int ts_body_pixel_infer_mixed_keep(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                   const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                   uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                   float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                   const uint8_t *keep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass under a "speaker style" (talkshow_hip.h): style (B, style_rows, NC) float weights in slot order in place of the ids, which
// are then not read and may be NULL; style_rows is 1 or T_max / 4.  style == NULL: exactly the entry above
int ts_body_pixel_infer_mixed_style(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                    const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                    uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                    const uint8_t *keep, const float *style, int style_rows, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass under a "code bias" (talkshow_hip.h): bias (n_bias, 2, V) device tables, bias_index_host (B,) the table of every clip in
// slot order or -1.  bias == NULL: exactly the entry above
int ts_body_pixel_infer_mixed_bias(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                   const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                   uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                   float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                   const uint8_t *keep, const float *style, int style_rows, const float *bias, int n_bias,
                                   const int32_t *bias_index_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass under a "repetition penalty" (talkshow_hip.h): rep_host n_rep (1 or B) records in slot order.  rep_host == NULL: exactly
// the entry above
int ts_body_pixel_infer_mixed_repeat(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                     const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                     uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                     float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                     const uint8_t *keep, const float *style, int style_rows, const float *bias, int n_bias,
                                     const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass with "alternatives" (talkshow_hip.h): the record of the four outputs over the pass's T_max / 4 code rows.  alt == NULL:
// exactly the entry above
int ts_body_pixel_infer_alt(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                  const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                  uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                  float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                  const uint8_t *keep, const float *style, int style_rows, const float *bias, int n_bias,
                                  const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.alt = alt;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same pass under "guidance" (talkshow_hip.h): guide_host (B,) the shadow's slot of every clip slot or -1, guide_scale_host (B,).  A
// shadow's rows of codes, log-probabilities and poses are its primary's.  guide_host == NULL: exactly the entry above
int ts_body_pixel_infer_guided(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                    const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                    uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob, const int64_t *given, const int32_t *given_rows_host, const int32_t *given_rows_dev,
                                    const uint8_t *keep, const float *style, int style_rows, const float *bias, int n_bias,
                                    const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const int32_t *guide_host,
                                    const float *guide_scale_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.guide_host = guide_host, o.guide_scale_host = guide_scale_host;
    return body_mixed(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// Host only: the rule every entry with given POSES applies to its frame table before anything is launched (talkshow_hip.h, "given poses")
int ts_given_pose_rows_check(const int32_t *pose_lens_host, const int32_t *lens_host, int B) {
    if (!pose_lens_host || !lens_host || B < 1) return fail("ts_given_pose_rows_check: bad argument");
    for (int b = 0; b < B; ++b) {
        const int P = pose_lens_host[b];
        if (P == 0) continue;
        if (P < 4)
            return fail("given poses of clip " + std::to_string(b) + ": P = " + std::to_string(P) + " frames; one code row needs 4 (or P = 0: none)");
        if (P / 4 > (lens_host[b] >> 2))
            return fail("given poses of clip " + std::to_string(b) + ": P = " + std::to_string(P) + " frames are " + std::to_string(P / 4) +
                        " code rows but the clip has " + std::to_string(lens_host[b] >> 2) + " of its own");
    }
    return 0;
}

// The body of every ts_body_pixel_infer_mixed_poses* entry: the given rows of body_mixed are ENCODED here from o.given_poses, on the device
// and in stream order, and the pass behind them is body_mixed's
static int body_mixed_poses(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const MixedPass &a, float *poses,
                            MixedOpts o, hipStream_t s) {
    if (o.keep && !o.given_poses)
        return fail("ts_body_pixel_infer_mixed_poses_keep: a mask of kept positions needs the given poses whose codes it selects from");
    std::vector<int32_t> G;   // the code rows the frames of every clip make: outlives the pass's host checks
    if (o.given_poses) {
        const char *who = "ts_body_pixel_infer_mixed_poses";
        const int B = a.B, H = (a.rows / 2) / 2;
        // everything the pass itself would refuse is refused here too, ahead of the encoders' launches
        if (!o.pose_lens_host || !o.pose_lens_dev) return fail(std::string(who) + ": given poses need their frame tables");
        TS_TRY(body_mixed_check("ts_body_pixel_infer_mixed", ae, pix, vb, vh, mfcc, a, poses, o));
        TS_TRY(mixed_style_rows_check("ts_body_pixel_infer_mixed", "T_max / 4", o, H));
        if (a.mode != TS_SAMPLE_GREEDY && a.mode != TS_SAMPLE_UNIFORMS && a.mode != TS_SAMPLE_PHILOX) return fail(std::string(who) + ": bad mode");
        if (a.mode == TS_SAMPLE_UNIFORMS && !a.uniforms) return fail(std::string(who) + ": TS_SAMPLE_UNIFORMS needs uniforms_dev");
        if (o.bias && body_bias_check("ts_body_pixel_infer_mixed_poses_bias", a.mode, B, o.n_bias, o.bias_index_host) != 0) return 1;
        if (o.rep_host && body_repeat_check("ts_body_pixel_infer_mixed_poses_repeat", a.mode, B, 1, o.rep_host, o.n_rep) != 0) return 1;
        if (ts_given_pose_rows_check(o.pose_lens_host, a.lens_host, B) != 0) return 1;
        if (o.guide_host && body_guide_check("ts_body_pixel_infer_guided_poses", a.mode, B, o, a.lens_host) != 0) return 1;
        int p_top = 0;
        G.resize(B);
        for (int b = 0; b < B; ++b) {
            G[b] = o.pose_lens_host[b] / 4;
            p_top = std::max(p_top, (int)o.pose_lens_host[b]);
        }
        if (p_top > o.P_max) return fail(std::string(who) + ": a clip brings more pose frames than P_max");
        if (p_top == 0) {   // nothing given anywhere: the pass without given rows
            o.keep = nullptr;
        } else {
            if (o.P_max / 4 > H) return fail(std::string(who) + ": P_max / 4 exceeds the pass's code rows T_max / 4");
            BodyWork &w = body_work(s);
            TS_TRY(w.given.ensure((size_t)B * H * 2 * sizeof(int64_t)));
            int64_t *given = static_cast<int64_t *>(w.given.p);
            // rows h < P_b / 4 of clip b: its codes; rows up to P_max / 4: -1; rows beyond stay as they are — the pass reads rows below G_b only
            TS_TRY(vq_encode_pair_masked(vb, vh, o.given_poses, vqvae_in_dim(vb) + vqvae_in_dim(vh), o.pose_lens_dev, B, o.P_max, given, H, nullptr, nullptr, 0, s));
            o.given = given, o.given_rows_host = G.data();
        }
    }
    return body_mixed(ae, pix, vb, vh, mfcc, a, poses, o, s);
}

// ts_body_pixel_infer_mixed_given whose given rows are ENCODED here from pose frames, on the device and in stream order (talkshow_hip.h,
// "given poses"); given_poses == NULL: exactly the _lp entry
int ts_body_pixel_infer_mixed_poses(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                    const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                    uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                    const int32_t *pose_lens_dev, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same with a mask of kept positions over the codes the encoders produce (keep (B, T_max / 4, 2) uint8, rows r < P_b / 4 read); keep ==
// NULL: exactly the entry above
int ts_body_pixel_infer_mixed_poses_keep(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                         const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                         uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host,
                                         int n_ctl, float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                         const int32_t *pose_lens_dev, const uint8_t *keep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same under a "speaker style" (style (B, style_rows, NC) in place of the ids; style == NULL: exactly the entry above).  The encoders
// never see a speaker: the style shapes the pass behind them only
int ts_body_pixel_infer_mixed_poses_style(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                          const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                          uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host,
                                          int n_ctl, float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                          const int32_t *pose_lens_dev, const uint8_t *keep, const float *style, int style_rows, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    o.style = style, o.style_rows = style_rows;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same under a "code bias" (bias (n_bias, 2, V), bias_index_host (B,) in slot order; bias == NULL: exactly the entry above).  The
// encoders never see the tables: given codes are taken whatever the tables say
int ts_body_pixel_infer_mixed_poses_bias(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                         const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                         uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host,
                                         int n_ctl, float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                         const int32_t *pose_lens_dev, const uint8_t *keep, const float *style, int style_rows, const float *bias,
                                         int n_bias, const int32_t *bias_index_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same under a "repetition penalty" (rep_host n_rep (1 or B) records in slot order; rep_host == NULL: exactly the entry above).  The
// encoders never see the records: the codes they find enter the histories as given codes do
int ts_body_pixel_infer_mixed_poses_repeat(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                           const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                           uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host,
                                           int n_ctl, float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                           const int32_t *pose_lens_dev, const uint8_t *keep, const float *style, int style_rows,
                                           const float *bias, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                           void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same with "alternatives" (alt == NULL: exactly the entry above).  The encoders never see the record: the codes they find are ranked
// and scored as given codes are
int ts_body_pixel_infer_alt_poses(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                        const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                        uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host,
                                        int n_ctl, float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host,
                                        const int32_t *pose_lens_dev, const uint8_t *keep, const float *style, int style_rows,
                                        const float *bias, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                        const ts_alt_out *alt, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.alt = alt;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

// the same under "guidance" (guide_host (B,), guide_scale_host (B,) in slot order; guide_host == NULL: exactly the entry above).  The encoders
// never see the tables: a shadow brings no poses of its own, the codes of its primary's are written to both slots
int ts_body_pixel_infer_guided_poses(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const float *mfcc, const int64_t *ids,
                                    const int32_t *lens_host, const int32_t *lens_dev, int B, int T_max, int mode, const float *uniforms,
                                    uint64_t seed, const int64_t *clip_index, int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl,
                                    float *logprob, const float *given_poses, int P_max, const int32_t *pose_lens_host, const int32_t *pose_lens_dev,
                                    const uint8_t *keep, const float *style, int style_rows, const float *bias, int n_bias,
                                    const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const int32_t *guide_host,
                                    const float *guide_scale_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given_poses = given_poses, o.P_max = P_max, o.pose_lens_host = pose_lens_host, o.pose_lens_dev = pose_lens_dev, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.guide_host = guide_host, o.guide_scale_host = guide_scale_host;
    return body_mixed_poses(ae, pix, vb, vh, mfcc, {ids, lens_host, lens_dev, B, T_max, mode, uniforms, seed, clip_index, codes}, poses, o, (hipStream_t)stream);
}

int ts_op_conv1d(ts_ctx *ctx, const float *x, int B, int Lin, int Cin, const float *w, const float *bias, int Cout,
                 int K, int stride, int pad, int transposed, int act, float *out, void *stream) {
    if (!ctx || !x || !w || !out) return fail("ts_op_conv1d: null argument");
    hipStream_t s = (hipStream_t)stream;
    int kind;
    if (!transposed && stride == 1 && (K == 1 || K == 3) && pad == (K - 1) / 2) kind = 0;
    else if (!transposed && stride == 2 && K == 4 && pad == 1) kind = 1;
    else if (transposed && stride == 2 && K == 4 && pad == 1) kind = 2;
    else return fail("ts_op_conv1d: unsupported geometry");
    std::vector<float> zb(Cout, 0.f);
    ts_tensor t[2];
    t[0].name = "op.weight";
    t[0].data = w;
    t[0].ndim = 3;
    t[0].shape[0] = transposed ? Cin : Cout;
    t[0].shape[1] = transposed ? Cout : Cin;
    t[0].shape[2] = K;
    t[1].name = "op.bias";
    t[1].data = bias ? bias : zb.data();
    t[1].ndim = 1;
    t[1].shape[0] = Cout;
    StateDict sd(t, 2);
    ConvLayer L;
    TS_TRY(pack_conv_layer(sd, "op", "", "", kind, K, Cin, Cout, act, &L));
    DevBuf xin;
    const float *xp = x;
    int ldx = Cin;
    if (Cin % 32 != 0) {
        TS_TRY(xin.ensure((size_t)B * Lin * L.cin_pad * sizeof(float)));
        TS_HIP(launch_pad_rows(x, Cin, Cin, xin.f(), L.cin_pad, L.cin_pad, (long)B * Lin, s));
        xp = xin.f();
        ldx = L.cin_pad;
    }
    ConvParams p;
    conv_layer_params(L, xp, ldx, B, Lin, nullptr, 0, out, Cout, 0, Cout, &p);
    TS_TRY(run_conv(ctx, p, 0, s));
    TS_HIP(hipStreamSynchronize(s));   // temporaries die with this frame
    return 0;
}

// one warm-up launch, then `iters` launches of the layer between two HIP events on `s`: *ms_out = mean launch duration (ms)
static int time_conv_launches(const ts::ConvParams &p, int tile, int iters, float *ms_out, hipStream_t s) {
    hipEvent_t a, b;
    TS_HIP(hipEventCreate(&a));
    TS_HIP(hipEventCreate(&b));
    TS_HIP(ts::launch_conv_gemm(p, tile, s));
    TS_HIP(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i) TS_HIP(ts::launch_conv_gemm(p, tile, s));
    TS_HIP(hipEventRecord(b, s));
    TS_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    TS_HIP(hipEventElapsedTime(&ms, a, b));
    if (ms_out) *ms_out = ms / (iters > 0 ? iters : 1);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return 0;
}

// Tuning / roofline entry (not part of the drop-in surface): a stride-1 conv layer (K = 1 or 3, Cin % 32 == 0) with
// weights ALREADY packed on the device as [round128(Cout)][K*Cin] (tap-major), launched `iters` times between two HIP
// events on `stream` with a chosen tile shape (0 = the heuristic used in production).  ms_out = mean launch duration.
int ts_op_conv1d_timed(ts_ctx *ctx, const float *x, int B, int Lin, int Cin, const float *w_packed_dev,
                       const float *bias_dev, int Cout, int K, int tile, int iters, float *out, float *ms_out,
                       void *stream) {
    if (!ctx || !x || !w_packed_dev || !out) return fail("ts_op_conv1d_timed: null argument");
    if (Cin % 32 || (K != 1 && K != 3)) return fail("ts_op_conv1d_timed: unsupported geometry");
    hipStream_t s = (hipStream_t)stream;
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = B * Lin;
    p.Lout = p.Lin = Lin;
    p.stride = 1;
    p.ldx = Cin;
    p.ldo = Cout;
    p.N = Cout;
    p.Ktot = K * Cin;
    p.act = 1;
    p.ngroups = 1;
    p.g[0].x = x;
    p.g[0].w = w_packed_dev;
    p.g[0].bias = bias_dev;
    p.g[0].out = out;
    p.g[0].nseg = K;
    for (int k = 0; k < K; ++k) p.g[0].seg[k] = ConvSeg{K == 1 ? 0 : k - 1, 0, Cin};
    if (tile == 24) {   // 2 planes from plane images of the packed weights (launch_split_weight_planes), as the face's x3 plan runs them
        DevBuf planes;
        const long rows = (Cout + 127) / 128 * 128;
        TS_TRY(planes.ensure((size_t)rows * p.Ktot * sizeof(float)));
        TS_HIP(launch_split_weight_planes(w_packed_dev, planes.f(), rows, p.Ktot, s));
        p.g[0].w = planes.f();
        p.w_planes = 1;
        const int rc = time_conv_launches(p, 22, iters, ms_out, s);
        TS_HIP(hipStreamSynchronize(s));   // the plane images die with this frame
        return rc;
    }
    return time_conv_launches(p, tile, iters, ms_out, s);
}

// the same for a strided convolution without padding (the wav2vec2 feature convolutions: out[t] = sum_k W_k x[stride t + k]);
// out: (B, (Lin - K) / stride + 1, Cout)
int ts_op_conv1d_strided_timed(ts_ctx *ctx, const float *x, int B, int Lin, int Cin, const float *w_packed_dev,
                               const float *bias_dev, int Cout, int K, int stride, int tile, int iters, float *out,
                               float *ms_out, void *stream) {
    if (!ctx || !x || !w_packed_dev || !out) return fail("ts_op_conv1d_strided_timed: null argument");
    if (Cin % 32 || K < 1 || K > 4 || stride < 1 || Lin < K) return fail("ts_op_conv1d_strided_timed: unsupported geometry");
    hipStream_t s = (hipStream_t)stream;
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.Lin = Lin;
    p.Lout = (Lin - K) / stride + 1;
    p.M = B * p.Lout;
    p.stride = stride;
    p.ldx = Cin;
    p.ldo = Cout;
    p.N = Cout;
    p.Ktot = K * Cin;
    p.act = 3;
    p.ngroups = 1;
    p.g[0].x = x;
    p.g[0].w = w_packed_dev;
    p.g[0].bias = bias_dev;
    p.g[0].out = out;
    p.g[0].nseg = K;
    for (int k = 0; k < K; ++k) p.g[0].seg[k] = ConvSeg{k, 0, Cin};
    return time_conv_launches(p, tile, iters, ms_out, s);
}

// grouped many-tap convolution, 48 channels per group in and out (conv_taps48.hip: the wav2vec2 positional conv): x, res, out
// (B, T, G * 48); w [G][48][ntap * 48] (tap-major, channels contiguous); bias [G * 48]; out = GELU(conv + bias) + res, taps
// -ntap / 2 .. ntap - ntap / 2 - 1, zero padding
int ts_op_conv_taps48_timed(ts_ctx *ctx, const float *x, int B, int T, int G, int ntap, const float *w, const float *bias,
                            const float *res, int iters, float *out, float *ms_out, void *stream) {
    if (!ctx || !x || !w || !out) return fail("ts_op_conv_taps48_timed: null argument");
    if (B < 1 || T < 1 || G < 1 || ntap < 1) return fail("ts_op_conv_taps48_timed: unsupported geometry");
    hipStream_t s = (hipStream_t)stream;
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = B * T;
    p.Lout = p.Lin = T;
    p.stride = 1;
    p.ldx = p.ldo = p.ldr = G * 48;
    p.N = 48;
    p.Ktot = ntap * 48;
    p.act = 3;
    p.res_after_act = 1;
    p.ngroups = p.zdiv = G;
    p.x_zs1 = p.o_zs1 = p.r_zs1 = p.b_zs1 = 48;
    p.w_zs1 = 48L * p.Ktot;
    p.g[0].x = x;
    p.g[0].w = w;
    p.g[0].bias = bias;
    p.g[0].res = res;
    p.g[0].out = out;
    p.g[0].nseg = 1;
    p.g[0].seg[0] = ConvSeg{-(ntap / 2), 0, 48, ntap};
    return time_conv_launches(p, 48, iters, ms_out, s);
}

int ts_debug_conv_plan(int M, int N, int Ktot, int groups, int sk_ok, const int *seg_len, int nseg, int tile, const char *knob_list, int *out4) {
    if (M < 1 || N < 1 || Ktot < 1 || groups < 1 || groups > 64 || nseg < 1 || nseg > 4 || !seg_len || !out4) return -1;
    if (groups > 4 && (nseg != 1 || seg_len[0] < 1 || Ktot % seg_len[0])) return -1;
    ts::ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M;
    p.Lout = p.Lin = M;
    p.stride = 1;
    p.N = N;
    p.Ktot = Ktot;
    p.ngroups = groups;
    p.zdiv = groups > 4 ? groups : 0;   // batched problems sharing g[0]'s geometry; the segment's taps make up Ktot
    p.sk_ok = sk_ok != 0;
    for (int z = 0; z < (groups > 4 ? 1 : groups); ++z) {
        p.g[z].nseg = nseg;
        for (int i = 0; i < nseg; ++i) p.g[z].seg[i] = ts::ConvSeg{0, 0, seg_len[i], groups > 4 ? Ktot / seg_len[0] : 1};
    }
    const ts::ConvPlan pl = ts::plan_conv(p, tile, ts::knobs_from_list(knob_list), true);
    if (pl.engine == ts::ConvEngine::Invalid) return -1;
    out4[0] = pl.bm;
    out4[1] = pl.bn;
    out4[2] = pl.wm > 0 ? (pl.bm / pl.wm) * (pl.bn / pl.wn) : 0;
    out4[3] = pl.bk;
    return (int)pl.engine;
}

int ts_debug_skinny_plan(const int *mnk, int n, const char *knob_list, int *out4) {
    if (!mnk || n < 1 || n > ts::SKINNY_MAX_PROBLEMS || !out4) return -1;
    const ts::Knobs k = ts::knobs_from_list(knob_list);
    const bool tiled = k.skinny_v != 0 && k.skinny_nt != 32 && k.skinny_tiled;   // the operands the PixelCNN lays out (skinny_descriptor_kernel_enabled)
    const float *fake = reinterpret_cast<const float *>(uintptr_t(4096));        // 16-byte aligned, never read: the plan looks at shapes only
    ts::SkinnyParams p[ts::SKINNY_MAX_PROBLEMS];
    const ts::SkinnyParams *ps[ts::SKINNY_MAX_PROBLEMS];
    for (int i = 0; i < n; ++i) {
        const int M = mnk[3 * i], N = mnk[3 * i + 1], K = mnk[3 * i + 2] < 0 ? -mnk[3 * i + 2] : mnk[3 * i + 2];
        if (M < 1 || N < 1 || K < 1) return -1;
        const bool zero_rows = mnk[3 * i + 2] < 0;
        std::memset(&p[i], 0, sizeof(p[i]));
        p[i].M = M;
        p[i].N = N;
        p[i].Ktot = K;
        p[i].nseg = 1;
        p[i].seg[0].base = zero_rows ? nullptr : fake;
        p[i].seg[0].row_stride = K;
        p[i].seg[0].len = K;
        p[i].seg[0].tiled_w = tiled && !zero_rows ? K : 0;
        p[i].W = fake;
        p[i].ldw = K;
        p[i].w_tiled = tiled && !zero_rows ? K / 16 : 0;
        p[i].out = const_cast<float *>(fake);
        p[i].out_stride = N;
        ps[i] = &p[i];
    }
    const ts::SkinnyPlan pl = ts::plan_skinny(ps, n, k);
    if (pl.kernel == ts::SkinnyKernel::Invalid) return -1;
    const bool grid1d = pl.kernel == ts::SkinnyKernel::Wide || pl.kernel == ts::SkinnyKernel::Fast;
    out4[0] = pl.W;
    out4[1] = pl.RB;
    out4[2] = pl.CB;
    out4[3] = grid1d ? pl.total : pl.gx * pl.gy * n;
    return (int)pl.kernel;
}

int ts_debug_skinny_run(ts_ctx *ctx, const ts_debug_skinny_problem *pr, int n, const char *knob_list, int *out5, void *stream) {
    if (!ctx || !pr || !out5 || n < 1 || n > ts::SKINNY_MAX_PROBLEMS) return fail("ts_debug_skinny_run: bad argument") ? -1 : -1;
    if (knob_list && std::strstr(knob_list, "TS_SKINNY_TRACE"))   // the record buffer only exists when the environment asked for it
        return fail("ts_debug_skinny_run: TS_SKINNY_TRACE is not a knob of this entry") ? -1 : -1;
    ts::SkinnyParams q[ts::SKINNY_MAX_PROBLEMS];
    const ts::SkinnyParams *ps[ts::SKINNY_MAX_PROBLEMS];
    for (int i = 0; i < n; ++i) {
        const ts_debug_skinny_problem &d = pr[i];
        if (d.M < 1 || d.N < 1 || d.nseg < 1 || d.nseg > ts::SKINNY_MAX_SEG || !d.W || !d.out) return fail("ts_debug_skinny_run: bad problem") ? -1 : -1;
        ts::SkinnyParams &p = q[i];
        std::memset(&p, 0, sizeof(p));
        p.M = d.M;
        p.N = d.N;
        p.nseg = d.nseg;
        for (int k = 0; k < d.nseg; ++k) {
            const ts_debug_skinny_seg &g = d.seg[k];
            if (g.len < 1) return fail("ts_debug_skinny_run: empty segment") ? -1 : -1;
            p.seg[k] = ts::SkinnySeg{g.base, g.gidx, g.row_stride, g.gidx_stride, g.row_shift, g.len, g.tiled_w};
            p.Ktot += g.len;
        }
        p.W = d.W;
        p.ldw = d.ldw;
        p.bias = d.bias;
        p.add1 = d.add1;
        p.add1_stride = d.add1_stride;
        p.add1_shift = d.add1_shift;
        p.add2 = d.add2;
        p.add2_stride = d.add2_stride;
        p.add2_shift = d.add2_shift;
        p.add3 = d.add3;
        p.add3_stride = d.add3_stride;
        p.clsrow = d.clsrow;
        p.cls_ld = d.cls_ld;
        p.epi = d.epi;
        p.relu = d.relu;
        p.gateD = d.gateD;
        p.out = d.out;
        p.out_stride = d.out_stride;
        p.pre = d.pre;
        p.pre_stride = d.pre_stride;
        p.w_tiled = d.w_tiled;
        p.out_tiled_w = d.out_tiled_w;
        p.pre_tiled_w = d.pre_tiled_w;
        p.add1_tiled_w = d.add1_tiled_w;
        ps[i] = &p;
    }
    ts::SkinnyPlan ran;
    const hipError_t e = ts::launch_skinny_batch(ps, n, (hipStream_t)stream, ts::knobs_from_list(knob_list), &ran);
    if (ran.kernel == ts::SkinnyKernel::Invalid) return fail("ts_debug_skinny_run: the problems fit no kernel") ? -1 : -1;
    if (e != hipSuccess) return fail(std::string("ts_debug_skinny_run: ") + hipGetErrorString(e)) ? -1 : -1;
    const bool grid1d = ran.kernel == ts::SkinnyKernel::Wide || ran.kernel == ts::SkinnyKernel::Fast;
    out5[0] = (int)ran.kernel;
    out5[1] = ran.W;
    out5[2] = ran.RB;
    out5[3] = ran.CB;
    out5[4] = grid1d ? ran.total : ran.gx * ran.gy * n;
    return (int)ran.kernel;
}

int ts_debug_conv_run(ts_ctx *ctx, const ts_debug_conv_problem *d, int tile, const char *knob_list, int dry, int *out8, void *stream) {
    auto bad = [](const std::string &m) { return fail("ts_debug_conv_run: " + m) ? -1 : -1; };
    if (!d || !out8 || (!dry && !ctx)) return bad("null argument");
    const int kq = tile == 48 ? 48 : 32;   // conv_taps48's K is 48 per tap, any tap count (conv_taps48_takes is the judge); everyone else walks chunks of 32
    if (d->M < 1 || d->N < 1 || d->Lout < 1 || d->Lin < 1 || d->stride < 1 || d->M % d->Lout || d->ldx < 1 || d->ldo < 1 || d->Ktot < kq || d->Ktot % kq ||
        d->act < 0 || d->act > 3 || d->ldw < 0 || d->w_rows < 0 || d->zdiv < 0)
        return bad("bad geometry");
    if (d->ngroups < 1 || (d->zdiv == 0 && d->ngroups > 4) || (d->zdiv > 0 && d->ngroups % d->zdiv)) return bad("1 to 4 groups, or a multiple of zdiv batched problems");
    ts::ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = d->M, p.Lout = d->Lout, p.Lin = d->Lin, p.stride = d->stride;
    p.ldx = d->ldx, p.ldo = d->ldo, p.ldr = d->ldr;
    p.N = d->N, p.Ktot = d->Ktot, p.act = d->act, p.ngroups = d->ngroups;
    p.res_after_act = d->res_after_act, p.ldw = d->ldw, p.w_rows = d->w_rows;
    p.zdiv = d->zdiv;
    p.x_zs0 = d->x_zs0, p.x_zs1 = d->x_zs1, p.w_zs0 = d->w_zs0, p.w_zs1 = d->w_zs1, p.o_zs0 = d->o_zs0, p.o_zs1 = d->o_zs1;
    p.b_zs1 = d->b_zs1, p.r_zs0 = d->r_zs0, p.r_zs1 = d->r_zs1;
    p.sk_ok = d->sk_ok;
    p.lens = d->lens, p.len_shr = d->len_shr, p.len_shl = d->len_shl;
    for (int z = 0; z < (d->zdiv > 0 ? 1 : d->ngroups); ++z) {
        const ts_debug_conv_group &s = d->g[z];
        ts::ConvGroup &g = p.g[z];
        if (!dry && (!s.x || !s.w || !s.out)) return bad("null operand");
        if (s.nseg < 1 || s.out_col0 < 0 || (s.res && d->ldr < 1)) return bad("bad group");
        g.x = s.x, g.w = s.w, g.bias = s.bias, g.res = s.res, g.out = s.out;
        g.out_col0 = s.out_col0, g.nseg = s.nseg;
        long k = 0;
        for (int i = 0; i < s.nseg && i < 4; ++i) {
            if (s.seg[i].len < 1 || s.seg[i].c0 < 0 || s.seg[i].ntap < 0) return bad("bad segment");
            g.seg[i] = ts::ConvSeg{s.seg[i].d, s.seg[i].c0, s.seg[i].len, s.seg[i].ntap};
            k += (long)s.seg[i].len * (s.seg[i].ntap > 1 ? s.seg[i].ntap : 1);
        }
        if (s.nseg <= 4 && k != d->Ktot) return bad("the segments do not add up to Ktot");
    }
    // 24 = 22 on plane images of the weights (w_planes), as ts_op_conv1d_timed and the face's x3 plan run it
    if (d->w_planes && tile != 22 && tile != 23) return bad("w_planes: weights given as plane images are for tiles 22 / 23 (24 makes the images itself)");
    p.w_planes = d->w_planes != 0 || tile == 24;
    const ts::ConvPlan pl = ts::plan_conv(p, tile == 24 ? 22 : tile, ts::knobs_from_list(knob_list), dry ? true : ts::conv_sk_supported());
    if (pl.engine == ts::ConvEngine::Invalid) return bad("unknown tile id");
    if (const char *why = ts::conv_plan_refusal(p, pl)) return bad(why);
    if (tile == 24 && (p.w_zs0 < 0 || p.w_zs1 < 0)) return bad("plane images of weights with a negative stride between batched problems");
    if (!dry) {
        // the plane images of every group's whole weight image: a chunk of 32 floats becomes a chunk of 32 dwords at the same offset, so the
        // row pitch (ldw) and the strides between batched problems carry over (conv_plan_refusal has made sure they are multiples of 32)
        DevBuf planes[4];
        for (int z = 0; tile == 24 && z < (p.zdiv > 0 ? 1 : p.ngroups); ++z) {
            const long rows = p.w_rows > 0 ? p.w_rows : (p.N + 127) / 128 * 128, ldw = p.ldw > 0 ? p.ldw : p.Ktot;
            const long extent = rows * ldw + (p.zdiv > 0 ? (p.ngroups / p.zdiv - 1) * p.w_zs0 + (p.zdiv - 1) * p.w_zs1 : 0);
            if (planes[z].ensure((size_t)extent * sizeof(float)) != 0) {   // (ensure has set the message)
                (void)hipStreamSynchronize((hipStream_t)stream);
                return -1;
            }
            const hipError_t es = ts::launch_split_weight_planes(p.g[z].w, planes[z].f(), extent / 32, 32, (hipStream_t)stream);
            if (es != hipSuccess) {
                (void)hipStreamSynchronize((hipStream_t)stream);
                return bad(hipGetErrorString(es));
            }
            p.g[z].w = planes[z].f();
        }
        hipError_t e = ts::launch_conv_plan(p, pl, (hipStream_t)stream);
        if (tile == 24) {   // the plane images die with this frame
            const hipError_t ew = hipStreamSynchronize((hipStream_t)stream);
            if (e == hipSuccess) e = ew;
        }
        if (e != hipSuccess) return bad(hipGetErrorString(e));
    }
    const int nt128 = (p.N + 127) / 128;
    int second = 0, wgs = 0;
    switch (pl.engine) {
        case ts::ConvEngine::Reg: wgs = ((p.M + pl.bm - 1) / pl.bm) * ((p.N + pl.bn - 1) / pl.bn) * p.ngroups; break;
        case ts::ConvEngine::RegBanded: second = pl.bands.total - pl.bands.first_small, wgs = pl.bands.total; break;
        case ts::ConvEngine::Ring: wgs = ((p.M + pl.bm - 1) / pl.bm) * nt128 * p.ngroups; break;
        case ts::ConvEngine::RingDealt: wgs = 8 * ((((p.M + pl.bm - 1) / pl.bm) * nt128 + 7) / 8) * p.ngroups; break;
        case ts::ConvEngine::RingBanded:
            second = pl.bands.mt_small * nt128 * p.ngroups;
            wgs = (8 * ((pl.bands.mt_big * nt128 + 7) / 8) + 8 * ((pl.bands.mt_small * nt128 + 7) / 8)) * p.ngroups;
            break;
        case ts::ConvEngine::RingSK: second = pl.sk.mt_sk * nt128 * p.ngroups, wgs = (pl.sk.dp8 + pl.sk.wsk) * p.ngroups; break;
        case ts::ConvEngine::Taps48: wgs = 8 * (int)((((long)(p.M + 127) / 128) * p.ngroups + 7) / 8); break;
        default: break;
    }
    int o[8] = {(int)pl.engine, pl.bm, pl.bn, pl.wm > 0 ? (pl.bm / pl.wm) * (pl.bn / pl.wn) : 0, pl.bk, second, wgs, p.lens ? 1 : 0};
    if (pl.engine == ts::ConvEngine::Split) {   // the variant its launcher takes by size: 128 x 128 or 64 x 64 tiles, 4 waves
        long n = 0;
        o[1] = o[2] = ts::conv_split_tile(p, &n);
        o[3] = 4, o[6] = (int)n;
    }
    std::memcpy(out8, o, sizeof(o));
    return (int)pl.engine;
}

int ts_debug_conv_sk_plan(int M, int N, int K, int groups, int *out6) {
    if (M < 1 || N < 1 || K < 32 || K % 32 || groups < 1 || groups > 4 || !out6) return -1;
    ts::ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.M = M;
    p.N = N;
    p.Ktot = K;
    p.ngroups = groups;
    for (int z = 0; z < groups; ++z) {
        p.g[z].nseg = 1;
        p.g[z].seg[0] = ts::ConvSeg{0, 0, K, 1};
    }
    ts::ConvSK sk{};
    if (!ts::conv_gemm_plan_sk_shape(p, sk)) return 0;
    ts::ConvBands bd{};
    const bool have = ts::conv_gemm_plan_bands(p, bd) && bd.mt_big >= 1;
    const ts::ConvPlan pick = ts::conv_gemm_ring_pick(p, have ? &bd : nullptr, &sk);
    // the plan by cost in this entry's documented numbers (tools/sk_layers.py reads them): 8 = the band, 9 / 3 / 7 = RingDealt 128 / 96, RingBanded
    const int code = pick.engine == ts::ConvEngine::RingSK ? 8 : pick.engine == ts::ConvEngine::RingBanded ? 7 : pick.bm == 96 ? 3 : 9;
    const int o[6] = {sk.mt_dp, sk.mt_sk, sk.dp8, sk.wsk, sk.stages, code};
    std::memcpy(out6, o, sizeof(o));
    return 1;
}

int ts_debug_conv_sk_supported(void) { return ts::conv_sk_supported() ? 1 : 0; }

int ts_debug_conv_sk_run(int band_tiles, int stages, int band_workgroups, int q, int *out4) {
    if (band_tiles < 8 || stages < 1 || band_workgroups < 8 || (band_workgroups & 7) || q < 0 || q >= band_workgroups || !out4) return -1;
    const ts::SkRuns R{band_tiles, stages, band_workgroups >> 3};
    const int c = q & 7, r = q >> 3;
    out4[0] = R.begin(c, r);
    out4[1] = R.begin(c, r + 1);
    out4[2] = c;
    out4[3] = R.run_of(c, out4[0] < out4[1] ? out4[0] : R.tlo(c) * stages);
    return 0;
}

int ts_debug_gate_act(const float *v_dev, const float *p_dev, float *out_dev, long n, void *stream) {
    if (!v_dev || !p_dev || !out_dev || n < 0) return fail("ts_debug_gate_act: bad argument");
    TS_HIP(ts::launch_gate_act(v_dev, p_dev, out_dev, n, (hipStream_t)stream));
    return 0;
}

int ts_debug_gelu(const float *v_dev, float *out_dev, long n, void *stream) {
    if (!v_dev || !out_dev || n < 0) return fail("ts_debug_gelu: bad argument");
    TS_HIP(ts::launch_gelu(v_dev, out_dev, n, (hipStream_t)stream));
    return 0;
}

// ---- the face generator's non-GEMM kernels (face.hip), one launch each on `stream` ----
int ts_debug_attention(const float *qkv, int B, int T, int HID, int heads, float scale, float *out, void *stream) {
    if (!qkv || !out || B < 1 || T < 1 || heads < 1 || HID != heads * 64) return fail("ts_debug_attention: bad argument");
    TS_HIP(ts::launch_attention(qkv, B, T, HID, heads, scale, out, (hipStream_t)stream));
    return 0;
}
int ts_debug_layernorm_rows(const float *x, int ldx, long M, int C, const float *gamma, const float *beta, const float *post_res,
                            int ldr, int relu, float *out, int ldo, void *stream) {
    if (!x || !gamma || !beta || !out || M < 1 || ldx < C || ldo < C || (post_res && ldr < C)) return fail("ts_debug_layernorm_rows: bad argument");
    if (C != 64 && C != 256 && C != 512 && C != 768) return fail("ts_debug_layernorm_rows: C must be 64, 256, 512 or 768");
    TS_HIP(ts::launch_layernorm_rows(x, ldx, M, C, gamma, beta, post_res, ldr, relu, out, ldo, (hipStream_t)stream));
    return 0;
}
int ts_debug_lerp_ln(const float *x, int B, int Lin, int T, const float *gamma, const float *beta, float *out, void *stream) {
    if (!x || !gamma || !beta || !out || B < 1 || Lin < 1 || T < 1) return fail("ts_debug_lerp_ln: bad argument");
    TS_HIP(ts::launch_lerp_ln(x, B, Lin, T, gamma, beta, out, (hipStream_t)stream));
    return 0;
}
int ts_debug_w2v_conv0(const float *wav, int B, int N, const float *w, const float *gamma, const float *beta, int form, float *out,
                       void *stream) {
    if (!wav || !w || !gamma || !beta || !out || B < 1 || N < 10 || form < -1 || form > 1) return fail("ts_debug_w2v_conv0: bad argument");
    constexpr int C = 512;
    const int L0 = (N - 10) / 5 + 1, ntb = (L0 + 127) / 128;
    hipStream_t s = (hipStream_t)stream;
    DevBuf part, stats;
    TS_TRY(part.ensure((size_t)B * ntb * C * sizeof(double2)));
    TS_TRY(stats.ensure((size_t)B * C * sizeof(float2)));
    const bool moments = form < 0 ? ts::knobs().w2v_moments : form == 1;
    TS_HIP(ts::launch_w2v_conv0(wav, B, N, L0, w, gamma, beta, static_cast<double2 *>(part.p), static_cast<float2 *>(stats.p), out, C,
                                moments, s));
    TS_HIP(hipStreamSynchronize(s));   // the scratch dies with this frame
    return 0;
}
int ts_debug_fill_id(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0, int B, int T,
                     void *stream) {
    if (!id || !w || !bias || !x || nc < 1 || nj < 1 || col0 < 0 || ld < col0 + nj || B < 1 || T < 1) return fail("ts_debug_fill_id: bad argument");
    TS_HIP(ts::launch_fill_id(id, nc, w, bias, nj, x, ld, col0, B, T, (hipStream_t)stream));
    return 0;
}

// ---- their length variants (mixed face passes), one launch each; the tables are device int32 unless named _host ----
int ts_debug_face_mixed_grid(const int32_t *frames_host, int B, int heads, int32_t *out3, int cap) {
    std::vector<int> work;
    const int n = ts::face_mixed_grid(frames_host, B, heads, work);
    if (n < 0) return -1;
    if (out3) {
        if (cap < n) return -1;
        for (int i = 0; i < n; ++i) {
            const int e = work[i], z = e >> 10;
            out3[3 * i] = e < 0 ? -1 : z / heads;
            out3[3 * i + 1] = e < 0 ? -1 : z % heads;
            out3[3 * i + 2] = e < 0 ? -1 : e & 1023;
        }
    }
    return n;
}
int ts_debug_attention_mixed(const float *qkv, const int32_t *frames_host, const int32_t *frames_dev, int B, int T_max, int HID, int heads,
                             float scale, float *out, void *stream) {
    if (!qkv || !out || !frames_host || !frames_dev || B < 1 || T_max < 1 || T_max > 65536 || heads < 1 || HID != heads * 64)
        return fail("ts_debug_attention_mixed: bad argument");
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 1 || frames_host[b] > T_max) return fail("ts_debug_attention_mixed: bad frame table");
    std::vector<int> work;
    const int n = ts::face_mixed_grid(frames_host, B, heads, work);
    if (n < 1) return fail("ts_debug_attention_mixed: bad frame table");
    hipStream_t s = (hipStream_t)stream;
    DevBuf wk;
    TS_TRY(wk.ensure((size_t)n * sizeof(int)));
    TS_HIP(ts::launch_put_words(wk.i(), work.data(), n, s));
    TS_HIP(ts::launch_attention_mixed(qkv, T_max, HID, heads, wk.i(), n, frames_dev, scale, out, s));
    TS_HIP(hipStreamSynchronize(s));   // the work list dies with this frame
    return 0;
}
int ts_debug_layernorm_rows_lens(const float *x, int ldx, int B, int T, const int32_t *lens, int C, const float *gamma, const float *beta,
                                 const float *post_res, int ldr, int relu, float *out, int ldo, void *stream) {
    if (!x || !gamma || !beta || !out || !lens || B < 1 || T < 1 || ldx < C || ldo < C || (post_res && ldr < C))
        return fail("ts_debug_layernorm_rows_lens: bad argument");
    if (C != 64 && C != 256 && C != 512 && C != 768) return fail("ts_debug_layernorm_rows_lens: C must be 64, 256, 512 or 768");
    TS_HIP(ts::launch_layernorm_rows_lens(x, ldx, B, T, lens, C, gamma, beta, post_res, ldr, relu, out, ldo, (hipStream_t)stream));
    return 0;
}
int ts_debug_lerp_ln_lens(const float *x, int B, int Lin, int T, const int32_t *ns, const int32_t *frames, const float *gamma,
                          const float *beta, float *out, void *stream) {
    if (!x || !ns || !frames || !gamma || !beta || !out || B < 1 || Lin < 1 || T < 1) return fail("ts_debug_lerp_ln_lens: bad argument");
    TS_HIP(ts::launch_lerp_ln_lens(x, B, Lin, T, ns, frames, gamma, beta, out, (hipStream_t)stream));
    return 0;
}
int ts_debug_w2v_conv0_lens(const float *wav, int B, int N, const int32_t *ns, const float *w, const float *gamma, const float *beta,
                            int form, float *out, void *stream) {
    if (!wav || !ns || !w || !gamma || !beta || !out || B < 1 || N < 10 || form < -1 || form > 1)
        return fail("ts_debug_w2v_conv0_lens: bad argument");
    constexpr int C = 512;
    const int L0 = (N - 10) / 5 + 1, ntb = (L0 + 127) / 128;
    hipStream_t s = (hipStream_t)stream;
    DevBuf part, stats;
    TS_TRY(part.ensure((size_t)B * ntb * C * sizeof(double2)));
    TS_TRY(stats.ensure((size_t)B * C * sizeof(float2)));
    const bool moments = form < 0 ? ts::knobs().w2v_moments : form == 1;
    TS_HIP(ts::launch_w2v_conv0_lens(wav, B, N, ns, w, gamma, beta, static_cast<double2 *>(part.p), static_cast<float2 *>(stats.p), out, C,
                                     moments, s));
    TS_HIP(hipStreamSynchronize(s));   // the scratch dies with this frame
    return 0;
}
int ts_debug_fill_id_lens(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0, int B, int T,
                          const int32_t *lens, void *stream) {
    if (!id || !w || !bias || !x || !lens || nc < 1 || nj < 1 || col0 < 0 || ld < col0 + nj || B < 1 || T < 1)
        return fail("ts_debug_fill_id_lens: bad argument");
    TS_HIP(ts::launch_fill_id_lens(id, nc, w, bias, nj, x, ld, col0, B, T, lens, (hipStream_t)stream));
    return 0;
}

// ---- the packed mixed pass's layout and kernels (face.cpp::face_packed_layout, face.hip); tables built here from the host tables ----
namespace {
// feat_off[0 .. B] and row0[0 .. B] of `lay` on the device, in stream order
int put_layout(const ts::FacePacked &lay, DevBuf &tab, hipStream_t s) {
    std::vector<int> t(lay.feat_off);
    t.insert(t.end(), lay.row0.begin(), lay.row0.end());
    TS_TRY(tab.ensure(t.size() * sizeof(int)));
    TS_HIP(ts::launch_put_words(tab.i(), t.data(), (long)t.size(), s));
    return 0;
}
}  // namespace
int ts_debug_face_packed_layout(const int32_t *ns_host, const int32_t *frames_host, int B, int64_t *feat_off, int64_t *row0, int64_t *levels7) {
    ts::FacePacked lay;
    if (ts::face_packed_layout(ns_host, frames_host, B, &lay)) return -1;
    for (int b = 0; b <= B; ++b) {
        if (feat_off) feat_off[b] = lay.feat_off[b];
        if (row0) row0[b] = lay.row0[b];
    }
    for (int i = 0; i < 7 && levels7; ++i) levels7[i] = lay.len[i];
    return 0;
}
int ts_debug_attention_packed(const float *qkv, const int32_t *frames_host, const int32_t *frames_dev, int B, int HID, int heads, float scale,
                              float *out, void *stream) {
    if (!qkv || !out || !frames_host || !frames_dev || B < 1 || heads < 1 || HID != heads * 64) return fail("ts_debug_attention_packed: bad argument");
    std::vector<int> work, ns(B, 400);
    const int n = ts::face_mixed_grid(frames_host, B, heads, work);
    ts::FacePacked lay;
    if (n < 1 || ts::face_packed_layout(ns.data(), frames_host, B, &lay)) return fail("ts_debug_attention_packed: bad frame table");
    hipStream_t s = (hipStream_t)stream;
    DevBuf wk, tab;
    TS_TRY(wk.ensure((size_t)n * sizeof(int)));
    TS_HIP(ts::launch_put_words(wk.i(), work.data(), n, s));
    TS_TRY(put_layout(lay, tab, s));
    TS_HIP(ts::launch_attention_packed(qkv, HID, heads, wk.i(), n, frames_dev, tab.i() + B + 1, scale, out, s));
    TS_HIP(hipStreamSynchronize(s));   // the tables die with this frame
    return 0;
}
int ts_debug_pack_rows(const float *src, const int32_t *frames_host, int B, int T_max, int C, float *dst, void *stream) {
    if (!src || !dst || !frames_host || B < 1 || T_max < 1 || C < 4 || C % 4) return fail("ts_debug_pack_rows: bad argument");
    std::vector<int> ns(B, 400);
    ts::FacePacked lay;
    if (ts::face_packed_layout(ns.data(), frames_host, B, &lay)) return fail("ts_debug_pack_rows: bad frame table");
    for (int b = 0; b < B; ++b)
        if (frames_host[b] > T_max) return fail("ts_debug_pack_rows: bad frame table");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tab;
    TS_TRY(put_layout(lay, tab, s));
    TS_HIP(ts::launch_pack_rows(src, B, T_max, C, tab.i() + B + 1, (int)lay.rows, dst, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}
int ts_debug_unpack_rows(const float *src, const int32_t *frames_host, const int32_t *frames_dev, int B, int T_max, int C, float *dst,
                         void *stream) {
    if (!src || !dst || !frames_host || !frames_dev || B < 1 || T_max < 1 || C < 4 || C % 4) return fail("ts_debug_unpack_rows: bad argument");
    std::vector<int> ns(B, 400);
    ts::FacePacked lay;
    if (ts::face_packed_layout(ns.data(), frames_host, B, &lay)) return fail("ts_debug_unpack_rows: bad frame table");
    for (int b = 0; b < B; ++b)
        if (frames_host[b] > T_max) return fail("ts_debug_unpack_rows: bad frame table");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tab;
    TS_TRY(put_layout(lay, tab, s));
    TS_HIP(ts::launch_unpack_rows(src, tab.i() + B + 1, frames_dev, B, T_max, C, dst, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}
int ts_debug_w2v_conv0_packed(const float *wav, int B, int N, const int32_t *ns_host, const int32_t *ns_dev, const float *w,
                              const float *gamma, const float *beta, int form, float *out, void *stream) {
    if (!wav || !ns_host || !ns_dev || !w || !gamma || !beta || !out || B < 1 || N < 400 || form < -1 || form > 1)
        return fail("ts_debug_w2v_conv0_packed: bad argument");
    std::vector<int> fr(B, 1);
    ts::FacePacked lay;
    if (ts::face_packed_layout(ns_host, fr.data(), B, &lay)) return fail("ts_debug_w2v_conv0_packed: bad sample table");
    for (int b = 0; b < B; ++b)
        if (ns_host[b] > N) return fail("ts_debug_w2v_conv0_packed: bad sample table");
    constexpr int C = 512;
    const int L0 = (N - 10) / 5 + 1, ntb = (L0 + 127) / 128;
    hipStream_t s = (hipStream_t)stream;
    DevBuf part, stats, tab;
    TS_TRY(part.ensure((size_t)B * ntb * C * sizeof(double2)));
    TS_TRY(stats.ensure((size_t)B * C * sizeof(float2)));
    TS_TRY(put_layout(lay, tab, s));
    const bool moments = form < 0 ? ts::knobs().w2v_moments : form == 1;
    TS_HIP(ts::launch_w2v_conv0_packed(wav, B, N, ns_dev, tab.i(), lay.len[0], w, gamma, beta, static_cast<double2 *>(part.p),
                                       static_cast<float2 *>(stats.p), out, C, moments, s));
    TS_HIP(hipStreamSynchronize(s));   // the scratch dies with this frame
    return 0;
}
int ts_debug_lerp_ln_packed(const float *x, int B, int T, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_dev,
                            const float *gamma, const float *beta, float *out, void *stream) {
    if (!x || !ns_host || !ns_dev || !frames_dev || !gamma || !beta || !out || B < 1 || T < 1) return fail("ts_debug_lerp_ln_packed: bad argument");
    std::vector<int> fr(B, 1);
    ts::FacePacked lay;
    if (ts::face_packed_layout(ns_host, fr.data(), B, &lay)) return fail("ts_debug_lerp_ln_packed: bad sample table");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tab;
    TS_TRY(put_layout(lay, tab, s));
    TS_HIP(ts::launch_lerp_ln_packed(x, B, T, ns_dev, frames_dev, tab.i(), gamma, beta, out, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

int ts_op_vq_argmin(ts_ctx *ctx, const float *x, int M, const float *cb, int ncode, int dim, int64_t *idx, void *stream) {
    if (!ctx || !x || !cb || !idx) return fail("ts_op_vq_argmin: null argument");
    hipStream_t s = (hipStream_t)stream;
    DevBuf sq;
    TS_TRY(sq.ensure((size_t)ncode * sizeof(float)));
    TS_HIP(launch_row_sqnorm(cb, ncode, dim, sq.f(), s));
    TS_HIP(launch_vq_argmin(x, dim, M, cb, sq.f(), ncode, dim, idx, 1, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

// the paired, length-masked codebook search on given latents (kernel-level tests): form 0 = the library's choice, 1 paired, 2 two launches,
// 3 the generic fallback; `iters` launches back to back (tools time them), one synchronisation
int ts_debug_vq_argmin_pair_masked(ts_ctx *ctx, const float *z_body, const float *z_hand, const int32_t *lens, int B, int H, const float *cb_body,
                                   const float *cb_hand, int ncode_body, int ncode_hand, int dim_body, int dim_hand, int64_t *codes, int form,
                                   int iters, void *stream) {
    if (!ctx || !z_body || !z_hand || !lens || !cb_body || !cb_hand || !codes) return fail("ts_op_vq_argmin_pair_masked: null argument");
    if (B < 1 || H < 1 || ncode_body < 1 || ncode_hand < 1 || dim_body < 4 || dim_hand < 4 || dim_body % 4 || dim_hand % 4 || form < 0 || form > 3 ||
        iters < 1)
        return fail("ts_op_vq_argmin_pair_masked: bad shape");
    hipStream_t s = (hipStream_t)stream;
    DevBuf sq[2];
    TS_TRY(sq[0].ensure((size_t)ncode_body * sizeof(float)));
    TS_TRY(sq[1].ensure((size_t)ncode_hand * sizeof(float)));
    TS_HIP(launch_row_sqnorm(cb_body, ncode_body, dim_body, sq[0].f(), s));
    TS_HIP(launch_row_sqnorm(cb_hand, ncode_hand, dim_hand, sq[1].f(), s));
    VqPairParams p;
    p.z[0] = z_body; p.z[1] = z_hand;
    p.cb[0] = cb_body; p.cb[1] = cb_hand;
    p.csq[0] = sq[0].f(); p.csq[1] = sq[1].f();
    p.ncode[0] = ncode_body; p.ncode[1] = ncode_hand;
    p.dim[0] = dim_body; p.dim[1] = dim_hand;
    p.B = B; p.H = H; p.Hout = H; p.lens = lens; p.codes = codes;
    for (int i = 0; i < iters; ++i) TS_HIP(launch_vq_argmin_pair_masked(p, form, s));
    TS_HIP(hipStreamSynchronize(s));   // the scratch dies with this frame
    return 0;
}
int ts_op_vq_argmin_pair_masked(ts_ctx *ctx, const float *z_body, const float *z_hand, const int32_t *lens, int B, int H, const float *cb_body,
                                const float *cb_hand, int ncode_body, int ncode_hand, int dim_body, int dim_hand, int64_t *codes, void *stream) {
    return ts_debug_vq_argmin_pair_masked(ctx, z_body, z_hand, lens, B, H, cb_body, cb_hand, ncode_body, ncode_hand, dim_body, dim_hand, codes, 0, 1,
                                          stream);
}

int ts_op_linear(ts_ctx *ctx, const float *x, int M, int K, const float *w, const float *bias, int N, int relu,
                 float *out, void *stream) {
    if (!ctx || !x || !w || !out) return fail("ts_op_linear: null argument");
    if (K % 8 != 0) return fail("ts_op_linear: K must be a multiple of 8");
    hipStream_t s = (hipStream_t)stream;
    DevBuf wd, bd;
    TS_TRY(wd.upload(w, (size_t)N * K * sizeof(float)));
    if (bias) TS_TRY(bd.upload(bias, (size_t)N * sizeof(float)));
    SkinnyParams q;
    std::memset(&q, 0, sizeof(q));
    q.M = M;
    q.N = N;
    q.nseg = 1;
    q.Ktot = K;
    q.seg[0].base = x;
    q.seg[0].row_stride = K;
    q.seg[0].len = K;
    q.W = wd.f();
    q.ldw = K;
    q.bias = bias ? bd.f() : nullptr;
    q.epi = EPI_LINEAR;
    q.relu = relu;
    q.out = out;
    q.out_stride = N;
    TS_TRY(run_skinny(ctx, q, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

// Tuning entry (not part of the drop-in surface): `iters` DEPENDENT skinny_gemm launches (stage i reads stage i-1's
// output) captured in one hipGraph and replayed; *us_out = microseconds per launch.  M x K activations, N = K outputs
// (linear) or 2K (gate epilogue, so the chain closes on itself); `debug` is unused (kept for ABI stability).
int ts_debug_skinny_chain(ts_ctx *ctx, int M, int K, int gate, int iters, int debug, float *us_out) {
    if (!ctx || !us_out) return fail("ts_debug_skinny_chain: null argument");
    const int N = gate ? 2 * K : K;
    DevBuf w, bias, x0, x1, lab, cls;
    std::vector<float> hw((size_t)N * K), hb(N, 0.01f), hx((size_t)M * K, 0.5f), hc((size_t)M * N, 0.01f);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = ((int)(i * 2654435761u >> 16) % 2001 - 1000) * (1.0f / (1000.f * K));
    std::vector<int> hl(M, 1);
    TS_TRY(w.upload(hw.data(), hw.size() * 4));
    TS_TRY(bias.upload(hb.data(), hb.size() * 4));
    TS_TRY(x0.upload(hx.data(), hx.size() * 4));
    TS_TRY(x1.upload(hx.data(), hx.size() * 4));
    TS_TRY(lab.upload(hl.data(), hl.size() * 4));
    TS_TRY(cls.upload(hc.data(), hc.size() * 4));
    hipStream_t s;
    TS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipGraph_t g;
    hipGraphExec_t ex;
    TS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < iters; ++i) {
        SkinnyParams q;
        std::memset(&q, 0, sizeof(q));
        q.M = M;
        q.N = N;
        q.nseg = 1;
        q.Ktot = K;
        q.seg[0].base = (i & 1) ? x1.f() : x0.f();
        q.seg[0].row_stride = K;
        q.seg[0].len = K;
        q.W = w.f();
        q.ldw = K;
        q.bias = bias.f();
        q.epi = gate ? EPI_GATE : EPI_LINEAR;
        q.gateD = K;
        q.clsrow = gate ? cls.f() : nullptr;
        q.cls_ld = N;
        q.out = (i & 1) ? x0.f() : x1.f();
        q.out_stride = K;
        TS_HIP(launch_skinny_gemm(q, s));
    }
    TS_HIP(hipStreamEndCapture(s, &g));
    TS_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    hipEvent_t a, b;
    TS_HIP(hipEventCreate(&a));
    TS_HIP(hipEventCreate(&b));
    TS_HIP(hipGraphLaunch(ex, s));
    TS_HIP(hipEventRecord(a, s));
    TS_HIP(hipGraphLaunch(ex, s));
    TS_HIP(hipEventRecord(b, s));
    TS_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    TS_HIP(hipEventElapsedTime(&ms, a, b));
    *us_out = ms * 1e3f / iters;
    (void)hipGraphExecDestroy(ex);
    (void)hipGraphDestroy(g);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    (void)hipStreamDestroy(s);
    return 0;
}

int ts_op_sample(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, int64_t *idx,
                 void *stream) {
    if (!ctx || !logits || !idx) return fail("ts_op_sample: null argument");
    if (mode != TS_SAMPLE_GREEDY && mode != TS_SAMPLE_UNIFORMS) return fail("ts_op_sample: bad mode");
    if (mode == TS_SAMPLE_UNIFORMS && !uniforms) return fail("ts_op_sample: uniforms required");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tok;
    TS_TRY(tok.ensure((size_t)B * sizeof(int)));
    SampleParams sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.logits = logits;
    sp.B = B;
    sp.V = V;
    sp.mode = mode;
    sp.uniforms = uniforms;
    sp.u_stride = 1;
    sp.tok32 = tok.i();
    sp.tok_stride = 1;
    sp.codes = idx;
    sp.code_stride = 1;
    TS_HIP(launch_sample(sp, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

int ts_op_sample_philox(ts_ctx *ctx, const float *logits, int B, int V, uint64_t seed, int64_t clip_index0, uint32_t position,
                        int64_t *idx, void *stream) {
    if (!ctx || !logits || !idx) return fail("ts_op_sample_philox: null argument");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tok;
    TS_TRY(tok.ensure((size_t)B * sizeof(int)));
    SampleParams sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.logits = logits;
    sp.B = B;
    sp.V = V;
    sp.mode = TS_SAMPLE_PHILOX;
    sp.seed = seed;
    sp.clip_index0 = clip_index0;
    sp.position = position;
    sp.tok32 = tok.i();
    sp.tok_stride = 1;
    sp.codes = idx;
    sp.code_stride = 1;
    TS_HIP(launch_sample(sp, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- Winograd lowering: host answers and single launches for tests/test_wino_host.py, tests/test_gpu_wino.py ----
int ts_debug_wino_lowering(int cin, int cout, int k, int stride, const char *knob_list, int B, int L, int *out5) {
    if (cin < 1 || cout < 1 || k < 1 || stride < 1 || B < 1 || L < 1 || !out5) return -1;
    const ts::Knobs kn = ts::knobs_from_list(knob_list);
    if (stride != 1 || !ts::wino_lowered(0, k, cin, cout, kn.conv_wino)) return 0;
    const int o[5] = {6, B * ((L + 3) / 4), cout, cin, 4};
    std::memcpy(out5, o, sizeof(o));
    return 1;
}

int ts_debug_wino_weights(const float *w, int cout, int cin, float *out) {
    if (!w || !out || cout < 1 || cin < 1) return fail("ts_debug_wino_weights: bad argument");
    ts::wino_transform_weights(w, cout, cin, round_up(cout, 128), out);
    return 0;
}

int ts_debug_wino_transform(ts_ctx *ctx, int which, int nnet, int B, int L, int C, int act, const int32_t *lens_dev, int shr, int shl,
                            const void *const *ptrs, void *stream) {
    if (!ctx || !ptrs || nnet < 1 || nnet > 2) return fail("ts_debug_wino_transform: bad argument");
    ts::WinoParams w;
    std::memset(&w, 0, sizeof(w));
    w.nnet = nnet;
    w.B = B, w.L = L, w.J = (L + 3) / 4, w.C = C, w.act = act;
    w.lens = lens_dev, w.len_shr = shr, w.len_shl = shl;
    for (int i = 0; i < nnet; ++i) {
        const void *const *q = ptrs + 6 * i;
        w.x[i] = (const float *)q[0], w.V[i] = (float *)q[1], w.O[i] = (const float *)q[2], w.bias[i] = (const float *)q[3];
        w.res[i] = (const float *)q[4], w.y[i] = (float *)q[5];
    }
    MiscScope ms(ctx, (hipStream_t)stream);
    TS_HIP(ts::launch_wino(which, w, (hipStream_t)stream));
    return 0;
}

int ts_debug_wino_gemm(ts_ctx *ctx, int nnet, const float *V0, const float *V1, const float *U0, const float *U1, float *O0, float *O1, int M,
                       int C, void *stream) {
    if (!ctx || nnet < 1 || nnet > 2 || !V0 || !U0 || !O0 || (nnet == 2 && (!V1 || !U1 || !O1)) || M < 1 || C < 32 || C % 32)
        return fail("ts_debug_wino_gemm: bad argument");
    const float *V[2] = {V0, V1}, *U[2] = {U0, U1};
    float *O[2] = {O0, O1};
    return ts::run_wino_gemm(ctx, nnet, V, U, O, M, C, round_up(C, 128), (hipStream_t)stream);
}

int ts_debug_wino_codes(ts_ctx *ctx, int nnet, int B, int L, int C, const int32_t *lens_dev, int shr, int shl, const int64_t *codes0,
                        const int64_t *codes1, const float *T0, const float *T1, int ncode0, int ncode1, float *O0, float *O1, void *stream) {
    if (!ctx || nnet < 1 || nnet > 2) return fail("ts_debug_wino_codes: bad argument");
    ts::WinoParams w;
    std::memset(&w, 0, sizeof(w));
    w.nnet = nnet;
    w.B = B, w.L = L, w.J = (L + 3) / 4, w.C = C;
    w.lens = lens_dev, w.len_shr = shr, w.len_shl = shl;
    w.codes[0] = codes0, w.codes[1] = codes1, w.T[0] = T0, w.T[1] = T1, w.ncode[0] = ncode0, w.ncode[1] = ncode1, w.Ow[0] = O0, w.Ow[1] = O1;
    MiscScope ms(ctx, (hipStream_t)stream);
    TS_HIP(ts::launch_wino(3, w, (hipStream_t)stream));
    return 0;
}

// ---- the glue kernels of vq.hip, one launch each on `stream` (talkshow_hip_debug.h): the launcher's own refusals come back through TS_HIP ----
int ts_debug_gather_rows(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M, int width, float *out,
                         int ldo, int L, const int32_t *lens, int len_shr, void *stream) {
    if (!table || !idx || !out || M < 1 || width < 1) return fail("ts_debug_gather_rows: bad argument");
    if (!lens && L == 0) TS_HIP(ts::launch_gather_rows(table, ld_table, nrows, idx, idx_stride, M, width, out, ldo, (hipStream_t)stream));
    else TS_HIP(ts::launch_gather_rows_masked(table, ld_table, nrows, idx, idx_stride, M, width, out, ldo, L, lens, len_shr, (hipStream_t)stream));
    return 0;
}
int ts_debug_pad_rows(const float *src, int lds, int c, float *dst, int ldd, int cpad, int B, int L, const int32_t *lens, void *stream) {
    if (!src || !dst || B < 1 || L < 1 || cpad < 1) return fail("ts_debug_pad_rows: bad argument");
    if (!lens) TS_HIP(ts::launch_pad_rows(src, lds, c, dst, ldd, cpad, (long)B * L, (hipStream_t)stream));
    else TS_HIP(ts::launch_pad_rows_masked(src, lds, c, dst, ldd, cpad, B, L, lens, (hipStream_t)stream));
    return 0;
}
int ts_debug_mask_rows(int64_t *codes, float *logprob, int B, int H, const int32_t *lens, void *stream) {
    if ((!codes && !logprob) || !lens || B < 1 || H < 1) return fail("ts_debug_mask_rows: bad argument");
    if (codes) TS_HIP(ts::launch_mask_codes(codes, B, H, lens, (hipStream_t)stream));
    if (logprob) TS_HIP(ts::launch_mask_logprob(logprob, B, H, lens, (hipStream_t)stream));
    return 0;
}
int ts_debug_iota_i64(int64_t *dst, int n, int64_t first, void *stream) {
    if (!dst || n < 1) return fail("ts_debug_iota_i64: bad argument");
    TS_HIP(ts::launch_iota_i64(dst, n, first, (hipStream_t)stream));
    return 0;
}
int ts_debug_i64_to_i32(const int64_t *src, int32_t *dst, long n, void *stream) {
    if (!src || !dst || n < 1) return fail("ts_debug_i64_to_i32: bad argument");
    TS_HIP(ts::launch_i64_to_i32(src, dst, n, (hipStream_t)stream));
    return 0;
}
int ts_debug_set_words3(uint64_t *dst, uint64_t a, uint64_t b, uint64_t c, void *stream) {
    if (!dst) return fail("ts_debug_set_words3: bad argument");
    TS_HIP(ts::launch_set_words3(dst, a, b, c, (hipStream_t)stream));
    return 0;
}
int ts_debug_slot_save(const int32_t *slots, const int32_t *hist, int n, int B, int row, int D, int NL, int NC, const int32_t *tok32,
                       const float *Q1, const float *Q0, const float *P, const float *CR, const float *bv, const int32_t *rep_ring,
                       const int64_t *open_labels, const float *tables, float *state, void *stream) {
    ts::SlotSaveParams q;
    std::memset(&q, 0, sizeof(q));
    q.slots = slots, q.hist = hist, q.n = n, q.B = B, q.row = row, q.D = D, q.NL = NL, q.NC = NC, q.R = 4;
    q.tok32 = tok32, q.Q1 = Q1, q.Q0 = Q0, q.P = P, q.CR = CR, q.bv = bv, q.rep_ring = rep_ring;
    q.open_labels = open_labels, q.tables = tables, q.state = state;
    TS_HIP(ts::launch_slot_save(q, (hipStream_t)stream));
    return 0;
}
int ts_debug_slot_load(const int32_t *slots, const int32_t *index, const int32_t *origin, int n, int n_states, int B, int row, int D, int NL,
                       int32_t *tok32, float *Q1, float *Q0, float *P, float *CR, int32_t *rep_ring, int32_t *row_origin, const float *state,
                       void *stream) {
    ts::SlotLoadParams q;
    std::memset(&q, 0, sizeof(q));
    q.slots = slots, q.index = index, q.origin = origin, q.n = n, q.n_states = n_states, q.B = B, q.row = row, q.D = D, q.NL = NL, q.R = 4;
    q.tok32 = tok32, q.Q1 = Q1, q.Q0 = Q0, q.P = P, q.CR = CR, q.rep_ring = rep_ring, q.row_origin = row_origin, q.state = state;
    TS_HIP(ts::launch_slot_load(q, (hipStream_t)stream));
    return 0;
}
int ts_debug_row_sqnorm(const float *e, int n, int dim, float *out, void *stream) {
    if (!e || !out || n < 1 || dim < 1) return fail("ts_debug_row_sqnorm: bad argument");
    TS_HIP(ts::launch_row_sqnorm(e, n, dim, out, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
