// Face generator: s2g_face.Generator.forward (nets/spg/s2g_face.py:196-224) over the wav2vec2-base encoder as the
// reference subclasses it (nets/spg/wav2vec.py:76-143), as a launch plan on conv_gemm_f32 + the kernels of face.hip.
//
//   wav (B,N) --conv0+GroupNorm+GELU--> (B,L0,512) --6 strided convs (GELU)--> (B,L6,512)
//     --lerp to `frames` + LayerNorm--> Linear 512->768 --(+ GELU(grouped k128 conv)) LayerNorm-->
//     12 x { QKV GEMM, QK^T (batched GEMM), softmax, P.V (batched GEMM), out-proj (+res), LN, FFN1 GELU, FFN2 (+res), LN }
//     --Linear 768->256 | id_mlp(id) concat--> 3 x {conv k3, LN, +res, ReLU} --> two heads of 3 x {conv k3, LN, ReLU}
//     --1x1 convs--> (B,frames,3+100)
#include <algorithm>

#include "host_common.h"

using namespace ts;

namespace {

struct LNp {
    DevBuf g, b;
};

struct EncLayer {
    ConvLayer qkv, outp, ff1, ff2;
    LNp ln1, ln2;
};

int up(DevBuf &d, const float *p, size_t n) { return d.upload(p, n * sizeof(float)); }

int load_ln(const StateDict &sd, const std::string &k, int c, LNp *o) {
    const float *g = sd.get(k + ".weight", {c}), *b = sd.get(k + ".bias", {c});
    if (!g || !b) return 1;
    TS_TRY(up(o->g, g, c));
    return up(o->b, b, c);
}

int load_linear(const StateDict &sd, const std::string &k, int n, int kk, int act, ConvLayer *L) {
    const float *w = sd.get(k + ".weight", {n, kk}), *b = sd.get(k + ".bias", {n});
    if (!w || !b) return 1;
    TS_TRY(pack_linear_layer(w, kk, b, n, kk, L));
    L->act = act;
    return 0;
}

int load_conv3(const StateDict &sd, const std::string &k, int cout, int cin, int K, ConvLayer *L) {
    const float *w = sd.get(k + ".weight", {cout, cin, K}), *b = sd.get(k + ".bias", {cout});
    if (!w || !b) return 1;
    const int taps3[3] = {-1, 0, 1}, taps1[1] = {0};
    return pack_conv_raw(w, b, cout, cin, K, K == 3 ? taps3 : taps1, 0, L);
}

// generic ConvParams for a packed layer: rows (b, t) with t < Lout, input row t*stride + d
void params_for(const ConvLayer &L, const float *x, int ldx, int B, int Lin, int Lout, int stride, const float *res, int ldr,
                float *out, int ldo, int col0, int nstore, int act, ConvParams *p, bool planes_ok = false) {
    std::memset(p, 0, sizeof(*p));
    p->M = B * Lout;
    p->Lout = Lout;
    p->Lin = Lin;
    p->stride = stride;
    p->ldx = ldx;
    p->ldo = ldo;
    p->ldr = ldr;
    p->N = nstore;
    p->Ktot = L.ktot;
    p->act = act;
    p->ngroups = 1;
    ConvGroup &G = p->g[0];
    G.x = x;
    G.w = L.w.f();
    if (planes_ok && L.wp.p) {   // x3 plan: the layer's weights as plane images (ts_face_set_arith)
        G.w = L.wp.f();
        p->w_planes = 1;
    }
    G.bias = L.bias.f();
    G.res = res;
    G.out = out;
    G.out_col0 = col0;
    G.nseg = L.nseg;
    for (int s = 0; s < L.nseg; ++s) G.seg[s] = L.segs[0][s];
}

}  // namespace

struct ts_face {
    ts_ctx *ctx = nullptr;
    int NL = 12, HID = 768, HEADS = 12, FFN = 3072, C0 = 512, NCLS = 4, POSK = 128, POSG = 16;
    int JAW = 3, CIN = 320;   // identity=False (num_classes 0, the reference's convert_to_6d form): no id channels (CIN 256), 6 jaw values
    DevBuf c0_w, c0_g, c0_b;
    ConvLayer fc[6];
    LNp fp_ln;
    ConvLayer fp_proj;
    DevBuf pos_w, pos_b, pos_wp;
    DevBuf pos_wd;   // the same weights unpadded, [group][48][taps * 48] (conv_taps48.hip); empty unless the group width is 48
    int pos_npad = 128, pos_ktot = 0;
    LNp enc_ln;
    std::vector<std::unique_ptr<EncLayer>> layers;
    ConvLayer afm;
    DevBuf id_w, id_b;
    ConvLayer fn[3], fn0res, dec[2][3], fin[2];
    LNp fn_ln[3], dec_ln[2][3];

    int split_planes = 0;   // 0: fp32 MFMA (default, the parity path); 2 / 3: opt-in split-bf16 GEMMs (ts_face_set_arith)

    struct Work {
        DevBuf A, Bf, part, stats, X512, H, H2, TMP, QKV, ATT, FF, X320, Y1, Y2, R, D1, D2;
        DevBuf att_work;   // mixed passes: the attention work list (face_mixed_grid), written on the stream by every call
        DevBuf pack_tab;   // packed mixed passes: feat_off[0 .. B], row0[0 .. B] (face_packed_layout), written on the stream by every call
    };
    StreamWorks<Work> works;
    Work &work(hipStream_t s) { return works.get(s); }
};

namespace ts {
int face_hidden(const ts_face *f) { return f->HID; }

// Work list of the mixed attention launch (face.hip::attention_mixed_kernel), host arithmetic only: one entry per workgroup id,
// (clip * heads + head) << 10 | query tile for every tile with 64 tile < frames[clip], -1 for an id without a tile.  Workgroup ids go to the
// XCDs round-robin, so lane x = id % 8 of the list is XCD x's queue: every (clip, head) is dealt WHOLE to one lane — its tiles run on one XCD
// back to back and find K / V in that L2, as in the uniform kernel — longest first (stable: clip-major, head-minor among equals), each to the
// lane that is shortest so far (ties: the lowest lane), and the lanes are padded to the longest with -1.  Equal frame counts give the uniform
// kernel's order.
int face_mixed_grid(const int32_t *frames, int B, int heads, std::vector<int> &work) {
    work.clear();
    if (!frames || B < 1 || heads < 1 || (long)B * heads >= (1l << 21)) return -1;
    std::vector<int> clips(B);
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1 || frames[b] > 65536) return -1;
        clips[b] = b;
    }
    std::stable_sort(clips.begin(), clips.end(), [&](int a, int b) { return (frames[a] + 63) / 64 > (frames[b] + 63) / 64; });
    std::vector<int> lane[8];
    for (int b : clips) {
        const int nq = (frames[b] + 63) / 64;
        for (int h = 0; h < heads; ++h) {
            int x = 0;
            for (int c = 1; c < 8; ++c)
                if (lane[c].size() < lane[x].size()) x = c;
            for (int q = 0; q < nq; ++q) lane[x].push_back(((b * heads + h) << 10) | q);
        }
    }
    size_t slots = 0;
    for (auto &l : lane) slots = std::max(slots, l.size());
    work.assign(slots * 8, -1);
    for (int x = 0; x < 8; ++x)
        for (size_t i = 0; i < lane[x].size(); ++i) work[i * 8 + x] = lane[x][i];
    return (int)work.size();
}

// Row layout of a packed mixed pass, host arithmetic only (no HIP call, no order among the clips needed).
//   Feature rows: the six stride-2 convolutions read no padding, so the clips lie back to back on ONE time axis and run as a single problem
//   (B = 1): clip b owns S_b = roundup64(L0(ns[b])) rows at the conv0 rate from feat_off[b] = sum of the segments before it.  Both are
//   multiples of 64 = 2^6, so at level i (0 .. 6) the clip starts at feat_off[b] >> i exactly, and output row (feat_off[b] >> (i + 1)) + t of
//   level i + 1 reads input rows (feat_off[b] >> i) + 2 t + d: for t below the clip's own count these are the clip's own valid rows.  Rows near
//   a seam are computed from a neighbour's data and read by nothing valid.  len[i] = rows of level i of that one problem (len[0] = feat_rows,
//   len[i + 1] = (len[i] - k_i) / 2 + 1: Lin / Lout of convolution i).
//   Transformer rows: clip b owns rows [row0[b], row0[b] + frames[b]), no rounding.
// Refused (-1): a null or bad table (ns < 400, frames < 1 or > 65536), or a row count beyond what the engines index with — rows are `int` in
// conv_tile.h and the ring engine, and a tile forms row indices up to one tile past the last row before it clamps them (element offsets are
// `long`: rows x pitch cannot leave them).  The packed totals exceed the padded pass's by at most 63 rows per clip.
int face_packed_layout(const int32_t *ns, const int32_t *frames, int B, FacePacked *o) {
    if (!ns || !frames || !o || B < 1) return -1;
    constexpr long ROW_MAX = 2147483647l - 4096;
    o->feat_off.assign(B + 1, 0);
    o->row0.assign(B + 1, 0);
    long foff = 0, roff = 0;
    for (int b = 0; b < B; ++b) {
        if (ns[b] < 400 || frames[b] < 1 || frames[b] > 65536) return -1;
        o->feat_off[b] = (int)foff;
        o->row0[b] = (int)roff;
        foff += ((long)((ns[b] - 10) / 5 + 1) + 63) / 64 * 64;
        roff += frames[b];
        if (foff > ROW_MAX || roff > ROW_MAX) return -1;
    }
    o->feat_off[B] = (int)foff;
    o->row0[B] = (int)roff;
    o->feat_rows = foff;
    o->rows = roff;
    o->len[0] = (int)foff;
    for (int i = 0; i < 6; ++i) o->len[i + 1] = (o->len[i] - FACE_FC_K[i]) / 2 + 1;
    return 0;
}
}  // namespace ts

namespace {
// a mixed pass (ts_face_generate_mixed): the clips' own sample and frame counts; the uniform entry passes none
struct FaceLens {
    const int32_t *ns_host, *ns_dev, *frames_host, *frames_dev;
    const char *who;   // the entry's name, for messages
    bool pack;   // the packed plan (face_packed_layout) for the feature convolutions and the transformer; false: padded throughout
};
int face_generate_mixed(ts_face *f, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_host,
                        const int32_t *frames_dev, int B, int N_max, int T_max, const float *id, float *out, float *hidden_out, void *stream,
                        bool pack, const char *who);
int face_run(ts_face *f, const float *wav, int B, int N, int frames, const float *id, float *out, float *hidden_out, hipStream_t s,
             const FaceLens *mx);
int check_mixed_tables(const int32_t *ns_host, const int32_t *frames_host, int B, int N_max, int T_max, const char *who);
}  // namespace

extern "C" {

int ts_face_create(ts_ctx *ctx, const ts_tensor *sd_, int n, int n_layers, int num_classes, ts_face **out) {
    if (!ctx || !sd_ || !out) return fail("ts_face_create: null argument");
    TS_HIP(hipSetDevice(ctx->device));
    StateDict sd(sd_, n);
    std::unique_ptr<ts_face> f(new ts_face());
    f->ctx = ctx;
    f->NL = n_layers;
    if (num_classes < 0) return fail("ts_face_create: num_classes < 0");
    f->NCLS = num_classes;
    // Generator(identity=False) (s2g_face.py:142-171, built by smplx_face.py:37-45 when convert_to_6d is set): AudioEncoder without
    // id_mlp (first_net takes the 256 audio channels alone), jaw head each_dim[0] = 6 wide (one joint in the 6-D rotation form)
    f->JAW = num_classes > 0 ? 3 : 6;
    f->CIN = num_classes > 0 ? 320 : 256;
    const int C0 = f->C0, HID = f->HID, FFN = f->FFN;
    const std::string p = "audio_encoder.";
    // ---- feature extractor ----
    const float *w0 = sd.get(p + "feature_extractor.conv_layers.0.conv.weight", {C0, 1, 10});
    const float *g0 = sd.get(p + "feature_extractor.conv_layers.0.layer_norm.weight", {C0});
    const float *b0 = sd.get(p + "feature_extractor.conv_layers.0.layer_norm.bias", {C0});
    if (!w0 || !g0 || !b0) return 1;
    TS_TRY(up(f->c0_w, w0, (size_t)C0 * 10));
    TS_TRY(up(f->c0_g, g0, C0));
    TS_TRY(up(f->c0_b, b0, C0));
    for (int i = 0; i < 6; ++i) {
        const int K = FACE_FC_K[i];
        const float *w = sd.get(p + "feature_extractor.conv_layers." + std::to_string(i + 1) + ".conv.weight", {C0, C0, K});
        if (!w) return 1;
        const int taps[3] = {0, 1, 2};   // stride 2, no padding: out[t] = sum_k W_k x[2t + k]
        TS_TRY(pack_conv_raw(w, nullptr, C0, C0, K, taps, 3, &f->fc[i]));
    }
    TS_TRY(load_ln(sd, p + "feature_projection.layer_norm", C0, &f->fp_ln));
    TS_TRY(load_linear(sd, p + "feature_projection.projection", HID, C0, 0, &f->fp_proj));
    // ---- positional conv: weight_norm(dim=2) folded; grouped weights padded 48 -> 64 channels per tap ----
    {
        const int G = f->POSG, K = f->POSK, cg = HID / G;
        const std::string q = p + "encoder.pos_conv_embed.conv";
        const float *g = nullptr, *v = nullptr;
        if (sd.m.count(q + ".parametrizations.weight.original0")) {
            g = sd.get(q + ".parametrizations.weight.original0", {1, 1, K});
            v = sd.get(q + ".parametrizations.weight.original1", {HID, cg, K});
        } else {   // transformers 4.22-era checkpoints (the reference's pin), SURVEY.md §0.9
            g = sd.get(q + ".weight_g", {1, 1, K});
            v = sd.get(q + ".weight_v", {HID, cg, K});
        }
        const float *b = sd.get(q + ".bias", {HID});
        if (!g || !v || !b) return 1;
        std::vector<double> nrm(K, 0.0);
        for (size_t i = 0; i < (size_t)HID * cg; ++i)
            for (int k = 0; k < K; ++k) nrm[k] += (double)v[i * K + k] * v[i * K + k];
        for (int k = 0; k < K; ++k) nrm[k] = std::sqrt(nrm[k]);
        const int cpad = 64, npad = f->pos_npad;
        if (cg > cpad || cg % 4) return fail("pos_conv: unsupported group width");
        f->pos_ktot = K * cpad;
        std::vector<float> wp((size_t)G * npad * f->pos_ktot, 0.f), bp((size_t)G * npad, 0.f);
        for (int gi = 0; gi < G; ++gi)
            for (int o = 0; o < cg; ++o) {
                const int oc = gi * cg + o;
                bp[(size_t)gi * npad + o] = b[oc];
                for (int k = 0; k < K; ++k)
                    for (int c = 0; c < cg; ++c)
                        wp[((size_t)gi * npad + o) * f->pos_ktot + (size_t)k * cpad + c] =
                            (float)(g[k] * (v[((size_t)oc * cg + c) * K + k] / nrm[k]));
            }
        TS_TRY(up(f->pos_w, wp.data(), wp.size()));
        TS_TRY(up(f->pos_b, bp.data(), bp.size()));
        if (cg == 48) {
            std::vector<float> wd((size_t)G * cg * K * cg);
            for (int gi = 0; gi < G; ++gi)
                for (int o = 0; o < cg; ++o)
                    for (int k = 0; k < K; ++k)
                        for (int c = 0; c < cg; ++c)
                            wd[(((size_t)gi * cg + o) * K + k) * cg + c] = wp[((size_t)gi * npad + o) * f->pos_ktot + (size_t)k * cpad + c];
            TS_TRY(up(f->pos_wd, wd.data(), wd.size()));
        }
    }
    TS_TRY(load_ln(sd, p + "encoder.layer_norm", HID, &f->enc_ln));
    for (int l = 0; l < n_layers; ++l) {
        const std::string q = p + "encoder.layers." + std::to_string(l) + ".";
        std::unique_ptr<EncLayer> L(new EncLayer());
        const float *wq = sd.get(q + "attention.q_proj.weight", {HID, HID}), *bq = sd.get(q + "attention.q_proj.bias", {HID});
        const float *wk = sd.get(q + "attention.k_proj.weight", {HID, HID}), *bk = sd.get(q + "attention.k_proj.bias", {HID});
        const float *wv = sd.get(q + "attention.v_proj.weight", {HID, HID}), *bv = sd.get(q + "attention.v_proj.bias", {HID});
        if (!wq || !bq || !wk || !bk || !wv || !bv) return 1;
        std::vector<float> w3((size_t)3 * HID * HID), b3((size_t)3 * HID);
        std::memcpy(w3.data(), wq, (size_t)HID * HID * 4);
        std::memcpy(w3.data() + (size_t)HID * HID, wk, (size_t)HID * HID * 4);
        std::memcpy(w3.data() + (size_t)2 * HID * HID, wv, (size_t)HID * HID * 4);
        std::memcpy(b3.data(), bq, HID * 4);
        std::memcpy(b3.data() + HID, bk, HID * 4);
        std::memcpy(b3.data() + 2 * HID, bv, HID * 4);
        TS_TRY(pack_linear_layer(w3.data(), HID, b3.data(), 3 * HID, HID, &L->qkv));
        TS_TRY(load_linear(sd, q + "attention.out_proj", HID, HID, 0, &L->outp));
        TS_TRY(load_ln(sd, q + "layer_norm", HID, &L->ln1));
        TS_TRY(load_linear(sd, q + "feed_forward.intermediate_dense", FFN, HID, 3, &L->ff1));
        TS_TRY(load_linear(sd, q + "feed_forward.output_dense", HID, FFN, 0, &L->ff2));
        TS_TRY(load_ln(sd, q + "final_layer_norm", HID, &L->ln2));
        f->layers.push_back(std::move(L));
    }
    // ---- heads ----
    TS_TRY(load_linear(sd, "audio_feature_map", 256, HID, 0, &f->afm));
    if (num_classes > 0) {
        const float *iw = sd.get("audio_middle.id_mlp.weight", {64, num_classes, 1}), *ib = sd.get("audio_middle.id_mlp.bias", {64});
        if (!iw || !ib) return 1;
        TS_TRY(up(f->id_w, iw, (size_t)64 * num_classes));
        TS_TRY(up(f->id_b, ib, 64));
    }
    const std::string fn = "audio_middle.first_net.conv_layers.";
    // 320 -> 256 channels: the residual branch is a conv; 256 -> 256 (identity=False): nn.Identity, no keys (layers.py:95-96)
    if (f->CIN != 256) TS_TRY(load_conv3(sd, fn + "0.residual_layer.0", 256, f->CIN, 3, &f->fn0res));
    TS_TRY(load_conv3(sd, fn + "0.conv", 256, f->CIN, 3, &f->fn[0]));
    TS_TRY(load_conv3(sd, fn + "1.conv", 256, 256, 3, &f->fn[1]));
    TS_TRY(load_conv3(sd, fn + "2.conv", 256, 256, 3, &f->fn[2]));
    for (int i = 0; i < 3; ++i) TS_TRY(load_ln(sd, fn + std::to_string(i) + ".norm", 256, &f->fn_ln[i]));
    for (int d = 0; d < 2; ++d) {
        const int c = d == 0 ? 64 : 256;
        for (int i = 0; i < 3; ++i) {
            const std::string k = "decoder." + std::to_string(d) + "." + std::to_string(i);
            TS_TRY(load_conv3(sd, k + ".conv", c, i == 0 ? 256 : c, 3, &f->dec[d][i]));
            TS_TRY(load_ln(sd, k + ".norm", c, &f->dec_ln[d][i]));
        }
        TS_TRY(load_conv3(sd, "final_out." + std::to_string(d), d == 0 ? f->JAW : 100, c, 1, &f->fin[d]));
    }
    *out = f.release();
    return 0;
}

void ts_face_destroy(ts_face *f) { delete f; }

// Arithmetic plan of the generator's GEMMs (feature convolutions 1..6, projections, positional conv, transformer-block GEMMs,
// LN-conv heads): 0 = fp32 MFMA (default: what every parity claim is made on), 3 / 6 = split-bf16 with three / six bf16 products
// per fp32 product (conv_gemm_split.hip).  Layer 0 of the feature extractor (K = 10, VALU), the attention products, LayerNorms
// and soft-max stay fp32 in every plan.
int ts_face_set_arith(ts_face *f, int bf16_products) {
    if (!f) return fail("ts_face_set_arith: null argument");
    if (bf16_products != 0 && bf16_products != 3 && bf16_products != 6) return fail("ts_face_set_arith: 0 (fp32), 3 or 6 bf16 products");
    const int planes = bf16_products == 0 ? 0 : (bf16_products == 3 ? 2 : 3);
    // (the plan is published LAST, after the weight plane images exist and the device has finished writing them: a generate call that
    // starts after this function returns sees a complete plan.  Like every entry of a handle, set_arith must not run concurrently
    // with ts_face_generate on the same handle — talkshow_hip.h, thread contract.)
    if (planes == 2 && !f->pos_wp.p) {
        // weights are constants: their two bf16 planes are made once, here, in the layout conv_gemm_split copies into LDS, and only the
        // activations are split per call (the plane images have the size and pitch of the fp32 matrices: + 1 x the weights of HBM)
        TS_HIP(hipSetDevice(f->ctx->device));
        std::vector<ConvLayer *> all;
        for (auto &c : f->fc) all.push_back(&c);
        all.push_back(&f->fp_proj);
        for (auto &L : f->layers)
            for (ConvLayer *c : {&L->qkv, &L->outp, &L->ff1, &L->ff2}) all.push_back(c);
        all.push_back(&f->afm);
        for (auto &c : f->fn) all.push_back(&c);
        if (f->CIN != 256) all.push_back(&f->fn0res);
        for (auto &d : f->dec)
            for (auto &c : d) all.push_back(&c);
        for (auto &c : f->fin) all.push_back(&c);
        for (ConvLayer *c : all) {
            if (!c->w.p || c->ktot % 32) continue;
            TS_TRY(c->wp.ensure(c->w.bytes));
            TS_HIP(launch_split_weight_planes(c->w.f(), c->wp.f(), (long)(c->w.bytes / sizeof(float) / c->ktot), c->ktot, nullptr));
        }
        TS_TRY(f->pos_wp.ensure(f->pos_w.bytes));
        TS_HIP(launch_split_weight_planes(f->pos_w.f(), f->pos_wp.f(), (long)(f->pos_w.bytes / sizeof(float) / f->pos_ktot), f->pos_ktot, nullptr));
        TS_HIP(hipDeviceSynchronize());   // the fills ran on the null stream; generate streams are non-blocking: order by completion
    }
    f->split_planes = planes;
    return 0;
}

// s2g_face.Generator.forward, eval (s2g_face.py:196-224): wav (B,N) fp32, id (B,num_classes) fp32 (one-hot or zeros,
// smplx_face.py:205-208) -> out (B,frames,103); hidden_out optional (B,frames,768) = wav2vec2 last_hidden_state.
// A handle created with num_classes = 0 is Generator(identity=False): id is ignored (may be NULL), out is (B,frames,106).
int ts_face_generate(ts_face *f, const float *wav, int B, int N, int frames, const float *id, float *out, float *hidden_out,
                     void *stream) {
    if (!f || !wav || !out || (!id && f->NCLS > 0)) return fail("ts_face_generate: null argument");
    if (B < 1 || frames < 1) return fail("ts_face_generate: bad shape");
    return face_run(f, wav, B, N, frames, id, out, hidden_out, (hipStream_t)stream, nullptr);
}

// Clips of different lengths in one pass (talkshow_hip.h): the launch plan of ts_face_generate with the length variants of the kernels wherever
// a clip's end matters and no stream-K band, padded to the longest clip throughout; with TS_FACE_PACK=1 the feature convolutions and the
// transformer run on the clips' own rows, packed back to back (face_packed_layout), with the same bits.
int ts_face_generate_mixed(ts_face *f, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_host,
                           const int32_t *frames_dev, int B, int N_max, int T_max, const float *id, float *out, float *hidden_out,
                           void *stream) {
    return face_generate_mixed(f, wav, ns_host, ns_dev, frames_host, frames_dev, B, N_max, T_max, id, out, hidden_out, stream,
                               ts::knobs().face_pack, "ts_face_generate_mixed");
}
// the same with the row layout named: 0 = padded, 1 = packed (both in one process: tests, A/B)
int ts_debug_face_generate_mixed(ts_face *f, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_host,
                                 const int32_t *frames_dev, int B, int N_max, int T_max, const float *id, float *out, float *hidden_out,
                                 void *stream, int layout) {
    if (layout != 0 && layout != 1) return fail("ts_debug_face_generate_mixed: layout is 0 (padded) or 1 (packed)");
    return face_generate_mixed(f, wav, ns_host, ns_dev, frames_host, frames_dev, B, N_max, T_max, id, out, hidden_out, stream, layout == 1,
                               "ts_debug_face_generate_mixed");
}

// Host only: what a mixed pass of these clips costs in rows — out4 = {feature rows (conv0 rate) padded = B L0(N_max), packed = sum of the clips'
// own rounded up to 64 each, frames padded = B T_max, packed = sum of frames[b]}.  The tables are checked as ts_face_generate_mixed checks them.
int ts_face_mixed_rows(const int32_t *ns_host, const int32_t *frames_host, int B, int N_max, int T_max, int64_t *out4) {
    if (!ns_host || !frames_host || !out4) return fail("ts_face_mixed_rows: null argument");
    TS_TRY(check_mixed_tables(ns_host, frames_host, B, N_max, T_max, "ts_face_mixed_rows"));
    FacePacked lay;
    if (face_packed_layout(ns_host, frames_host, B, &lay)) return fail("ts_face_mixed_rows: the pass has more rows than the kernels index");
    out4[0] = (int64_t)B * ((N_max - 10) / 5 + 1);
    out4[1] = lay.feat_rows;
    out4[2] = (int64_t)B * T_max;
    out4[3] = lay.rows;
    return 0;
}

}  // extern "C"

namespace {
int check_mixed_tables(const int32_t *ns_host, const int32_t *frames_host, int B, int N_max, int T_max, const char *who_) {
    const std::string who = who_;
    if (B < 1 || N_max < 1 || T_max < 1 || T_max > 65536) return fail(who + ": bad shape");
    for (int b = 0; b < B; ++b) {
        const std::string clip = who + ": clip " + std::to_string(b);
        if (ns_host[b] < 400) return fail(clip + " is shorter than 400 samples");
        if (ns_host[b] > N_max) return fail(clip + " is longer than N_max");
        if (frames_host[b] < 1) return fail(clip + " has no frames");
        if (frames_host[b] > T_max) return fail(clip + " has more frames than T_max");
    }
    return 0;
}
int face_generate_mixed(ts_face *f, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, const int32_t *frames_host,
                        const int32_t *frames_dev, int B, int N_max, int T_max, const float *id, float *out, float *hidden_out, void *stream,
                        bool pack, const char *who_) {
    const std::string who = who_;
    if (!f || !wav || !out || (!id && f->NCLS > 0)) return fail(who + ": null argument");
    if (!ns_host || !ns_dev || !frames_host || !frames_dev) return fail(who + ": null length table");
    if (f->split_planes) return fail(who + ": the split-bf16 plans (ts_face_set_arith 3 / 6) are not offered in a mixed pass");
    TS_TRY(check_mixed_tables(ns_host, frames_host, B, N_max, T_max, who_));
    const FaceLens mx{ns_host, ns_dev, frames_host, frames_dev, who_, pack};
    return face_run(f, wav, B, N_max, T_max, id, out, hidden_out, (hipStream_t)stream, &mx);
}
// mx == nullptr: B clips of N samples and `frames` frames each.  mx: B clips padded to N samples and `frames` frames (the tables are checked)
int face_run(ts_face *f, const float *wav, int B, int N, int frames, const float *id, float *out, float *hidden_out, hipStream_t s,
             const FaceLens *mx) {
    ts_ctx *ctx = f->ctx;
    const int C0 = f->C0, HID = f->HID, FFN = f->FFN, HEADS = f->HEADS, T = frames;
    int L[7];
    L[0] = (N - 10) / 5 + 1;
    if (N < 10 || L[0] < 1) return fail("ts_face_generate: audio too short");
    for (int i = 0; i < 6; ++i) {
        L[i + 1] = (L[i] - FACE_FC_K[i]) / 2 + 1;
        if (L[i] < FACE_FC_K[i]) return fail("ts_face_generate: audio too short (needs >= 400 samples)");
    }
    const long M = (long)B * T;
    // packed mixed pass: the feature convolutions as ONE problem over the clips' segments, the transformer over the clips' own frames
    const bool pk = mx && mx->pack;
    FacePacked lay;
    if (pk && face_packed_layout(mx->ns_host, mx->frames_host, B, &lay))
        return fail(std::string(mx->who) + ": the pass has more rows than the kernels index");
    const long R = pk ? lay.rows : M;   // rows of the transformer block
    ts_face::Work &w = f->work(s);
    const size_t F = sizeof(float);
    const int ntb = (L[0] + 127) / 128;
    TS_TRY(w.A.ensure((size_t)(pk ? lay.len[0] : (long)B * L[0]) * C0 * F));
    TS_TRY(w.Bf.ensure((size_t)(pk ? lay.len[1] : (long)B * L[1]) * C0 * F));
    TS_TRY(w.part.ensure((size_t)B * ntb * C0 * sizeof(double2)));
    TS_TRY(w.stats.ensure((size_t)B * C0 * sizeof(float2)));
    TS_TRY(w.X512.ensure(M * C0 * F));
    TS_TRY(w.H.ensure((M * HID + 64) * F));
    TS_TRY(w.H2.ensure(R * HID * F));
    TS_TRY(w.TMP.ensure(M * HID * F));
    TS_TRY(w.QKV.ensure(R * 3 * HID * F));
    TS_TRY(w.ATT.ensure(R * HID * F));
    TS_TRY(w.FF.ensure(R * FFN * F));
    TS_TRY(w.X320.ensure(M * 320 * F));
    const int CIN = f->CIN, JAW = f->JAW, OUTW = f->JAW + 100;
    TS_TRY(w.Y1.ensure(M * 256 * F));
    TS_TRY(w.Y2.ensure(M * 256 * F));
    TS_TRY(w.R.ensure(M * 256 * F));
    TS_TRY(w.D1.ensure(M * 64 * F));
    TS_TRY(w.D2.ensure(M * 64 * F));
    const int32_t *lens = mx ? mx->frames_dev : nullptr;   // frames per clip: the length table of every masked layer
    int n_work = 0;
    if (mx) {   // the attention work list of this pass, from the host table; it reaches the stream's buffer in stream order
        std::vector<int> work;
        n_work = face_mixed_grid(mx->frames_host, B, HEADS, work);
        if (n_work < 1) return fail("ts_face_generate_mixed: bad frame table");
        TS_TRY(w.att_work.ensure((size_t)n_work * sizeof(int)));
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(w.att_work.i(), work.data(), n_work, s));
    }
    const int *feat_off = nullptr, *row0 = nullptr;   // device tables of the packed layout, B + 1 words each
    if (pk) {
        std::vector<int> tab(lay.feat_off);
        tab.insert(tab.end(), lay.row0.begin(), lay.row0.end());
        TS_TRY(w.pack_tab.ensure(tab.size() * sizeof(int)));
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(w.pack_tab.i(), tab.data(), (long)tab.size(), s));
        feat_off = w.pack_tab.i();
        row0 = feat_off + B + 1;
    }

    ConvParams p;
    auto conv = [&](const ConvLayer &Ly, const float *x, int ldx, int Bc, int Lin, int Lout, int stride, const float *res,
                    int ldr, float *o, int ldo, int col0, int nstore, int act) -> int {
        params_for(Ly, x, ldx, Bc, Lin, Lout, stride, res, ldr, o, ldo, col0, nstore, act, &p, f->split_planes == 2);
        // tolerance-only GEMMs (<= 1e-4 vs the reference; measured 2e-6): the ring engine may split the last unit's tiles in K.  Not in a mixed
        // pass: without the band a row's bits do not depend on the rows it shares a launch with
        p.sk_ok = mx ? 0 : 1;
        return run_conv(ctx, p, f->split_planes ? 20 + f->split_planes : 0, s);
    };
    // a pointwise layer over all M rows.  Mixed passes: in the (B, T) row form with the masked epilogue — rows at or beyond frames[b] are stored
    // as zeros (same plan: it depends on M, N and K only)
    auto linear_masked = [&](const ConvLayer &Ly, const float *x, int ldx, float *o, int ldo, int col0, int nstore) -> int {
        if (!mx) return conv(Ly, x, ldx, 1, (int)M, (int)M, 1, nullptr, 0, o, ldo, col0, nstore, 0);
        params_for(Ly, x, ldx, B, T, T, 1, nullptr, 0, o, ldo, col0, nstore, 0, &p);
        p.lens = lens;
        return run_conv(ctx, p, 0, s);
    };
    auto ln = [&](const float *x, int C, const LNp &q, const float *post, int relu, float *o) -> int {
        MiscScope ms(ctx, s);
        // mixed passes: zeros at or beyond frames[b] — what the k = 3 layers read past a clip's end, and the padding of `hidden`
        if (mx) TS_HIP(launch_layernorm_rows_lens(x, C, B, T, lens, C, q.g.f(), q.b.f(), post, C, relu, o, C, s));
        else TS_HIP(launch_layernorm_rows(x, C, M, C, q.g.f(), q.b.f(), post, C, relu, o, C, s));
        return 0;
    };

    // ---- wav2vec2 feature extractor ----
    {
        MiscScope ms(ctx, s);
        if (pk)   // the same statistics; the apply pass writes each clip's segment of the one time axis
            TS_HIP(launch_w2v_conv0_packed(wav, B, N, mx->ns_dev, feat_off, lay.len[0], f->c0_w.f(), f->c0_g.f(), f->c0_b.f(),
                                           static_cast<double2 *>(w.part.p), static_cast<float2 *>(w.stats.p), w.A.f(), C0,
                                           ts::knobs().w2v_moments, s));
        else if (mx)   // statistics over each clip's own rows; samples at or beyond ns[b] are not read
            TS_HIP(launch_w2v_conv0_lens(wav, B, N, mx->ns_dev, f->c0_w.f(), f->c0_g.f(), f->c0_b.f(), static_cast<double2 *>(w.part.p),
                                         static_cast<float2 *>(w.stats.p), w.A.f(), C0, ts::knobs().w2v_moments, s));
        else
            TS_HIP(launch_w2v_conv0(wav, B, N, L[0], f->c0_w.f(), f->c0_g.f(), f->c0_b.f(), static_cast<double2 *>(w.part.p),
                                    static_cast<float2 *>(w.stats.p), w.A.f(), C0, ts::knobs().w2v_moments, s));
    }
    // (stride 2, no padding: a valid output row reads valid input rows only — in a padded mixed pass the rows beyond a clip's own are dead
    // weight; a packed pass runs the clips' segments as one clip, face_packed_layout)
    float *cur = w.A.f(), *nxt = w.Bf.f();
    for (int i = 0; i < 6; ++i) {
        if (pk) TS_TRY(conv(f->fc[i], cur, C0, 1, lay.len[i], lay.len[i + 1], 2, nullptr, 0, nxt, C0, 0, C0, 3));
        else TS_TRY(conv(f->fc[i], cur, C0, B, L[i], L[i + 1], 2, nullptr, 0, nxt, C0, 0, C0, 3));
        std::swap(cur, nxt);
    }
    {
        MiscScope ms(ctx, s);
        if (pk) TS_HIP(launch_lerp_ln_packed(cur, B, T, mx->ns_dev, lens, feat_off, f->fp_ln.g.f(), f->fp_ln.b.f(), w.X512.f(), s));
        else if (mx) TS_HIP(launch_lerp_ln_lens(cur, B, L[6], T, mx->ns_dev, lens, f->fp_ln.g.f(), f->fp_ln.b.f(), w.X512.f(), s));
        else TS_HIP(launch_lerp_ln(cur, B, L[6], T, f->fp_ln.g.f(), f->fp_ln.b.f(), w.X512.f(), s));
    }
    // the grouped positional conv reads 64-channel windows every 48 channels: the last group's window runs 16 floats past
    // the row (zero weights there) — keep the slack after the final row finite
    TS_HIP(hipMemsetAsync(w.H.f() + M * HID, 0, 64 * F, s));
    // (masked in a mixed pass: the positional conv reads 64 rows either side of a frame and finds zeros beyond the clip's end, as it finds its own
    // padding when the clip runs alone)
    TS_TRY(linear_masked(f->fp_proj, w.X512.f(), C0, w.H.f(), HID, 0, HID));
    // ---- positional conv embedding (16 groups as batched problems) + residual + LayerNorm ----
    {
        std::memset(&p, 0, sizeof(p));
        const int cg = HID / f->POSG;
        p.M = (int)M;
        p.Lout = p.Lin = T;
        p.stride = 1;
        p.ldx = HID;
        p.ldo = HID;
        p.ldr = HID;
        p.N = cg;
        p.Ktot = f->pos_ktot;
        p.act = 3;
        p.res_after_act = 1;
        p.ngroups = f->POSG;
        p.zdiv = f->POSG;
        p.x_zs1 = cg;
        p.w_zs1 = (long)f->pos_npad * f->pos_ktot;
        p.o_zs1 = cg;
        p.b_zs1 = f->pos_npad;
        p.r_zs1 = cg;
        ConvGroup &G = p.g[0];
        G.x = w.H.f();
        G.w = f->pos_w.f();
        if (f->split_planes == 2 && f->pos_wp.p) {
            G.w = f->pos_wp.f();
            p.w_planes = 1;
        }
        G.bias = f->pos_b.f();
        G.res = w.H.f();
        G.out = w.TMP.f();
        G.nseg = 1;
        G.seg[0] = ConvSeg{-(f->POSK / 2), 0, 64, f->POSK};
        int pos_tile = f->split_planes ? 20 + f->split_planes : 0;
        if (!f->split_planes && f->pos_wd.p && ts::knobs().conv_taps48) {   // unpadded: 48-channel taps, 48 weight rows per group (conv_taps48.hip)
            ConvParams q = p;
            q.Ktot = f->POSK * cg;
            q.w_zs1 = (long)cg * q.Ktot;
            q.g[0].w = f->pos_wd.f();
            q.g[0].seg[0].len = cg;
            // the unpadded weights are ONLY laid out for conv_taps48: take them when that kernel takes the layer (alignment, lengths) and
            // name it explicitly (tile 48 fails loudly on a mismatch); otherwise the padded 64-row weights + the generic engine stay (ADVICE r5:
            // a fall-through to 64 x 64 tiles over 48-row weights would read 16 rows past the last group)
            if (conv_taps48_takes(q)) {
                p = q;
                pos_tile = 48;
            }
        }
        TS_TRY(run_conv(ctx, p, pos_tile, s));
    }
    TS_TRY(ln(w.TMP.f(), HID, f->enc_ln, nullptr, 0, w.H.f()));
    // ---- transformer layers (post-LN) ----
    double att_tt = (double)B * T * T;   // sum over the clips of frames^2
    if (mx) {
        att_tt = 0;
        for (int b = 0; b < B; ++b) att_tt += (double)mx->frames_host[b] * mx->frames_host[b];
    }
    // packed: the clips' own rows of the padded block back to back (every row real: uniform LayerNorms, no masks), the padded block again after
    // the last layer with zeros at and beyond frames[b]
    float *h = w.H.f(), *tmp = w.TMP.f();
    if (pk) {
        MiscScope ms(ctx, s);
        TS_HIP(launch_pack_rows(w.H.f(), B, T, HID, row0, (int)R, w.TMP.f(), s));
        std::swap(h, tmp);
    }
    auto ln_t = [&](const float *x, const LNp &q, float *o) -> int {
        if (!pk) return ln(x, HID, q, nullptr, 0, o);
        MiscScope ms(ctx, s);
        TS_HIP(launch_layernorm_rows(x, HID, R, HID, q.g.f(), q.b.f(), nullptr, HID, 0, o, HID, s));
        return 0;
    };
    for (auto &Lp : f->layers) {
        EncLayer &E = *Lp;
        TS_TRY(conv(E.qkv, h, HID, 1, (int)R, (int)R, 1, nullptr, 0, w.QKV.f(), 3 * HID, 0, 3 * HID, 0));
        // softmax(Q K^T / 8) V per (clip, head), fused: the scores stay in registers (face.hip::attention_kernel)
        {
            MiscScope ms(ctx, s, FAM_ATTN, 4.0 * HEADS * att_tt * 64);   // Q K^T and P V: 2 x (2 T^2 d) per (clip, head)
            if (pk) TS_HIP(launch_attention_packed(w.QKV.f(), HID, HEADS, w.att_work.i(), n_work, lens, row0, 0.125f, w.ATT.f(), s));
            else if (mx) TS_HIP(launch_attention_mixed(w.QKV.f(), T, HID, HEADS, w.att_work.i(), n_work, lens, 0.125f, w.ATT.f(), s));
            else TS_HIP(launch_attention(w.QKV.f(), B, T, HID, HEADS, 0.125f, w.ATT.f(), s));
        }
        TS_TRY(conv(E.outp, w.ATT.f(), HID, 1, (int)R, (int)R, 1, h, HID, tmp, HID, 0, HID, 0));
        TS_TRY(ln_t(tmp, E.ln1, w.H2.f()));
        TS_TRY(conv(E.ff1, w.H2.f(), HID, 1, (int)R, (int)R, 1, nullptr, 0, w.FF.f(), FFN, 0, FFN, 3));
        TS_TRY(conv(E.ff2, w.FF.f(), FFN, 1, (int)R, (int)R, 1, w.H2.f(), HID, tmp, HID, 0, HID, 0));
        TS_TRY(ln_t(tmp, E.ln2, h));
    }
    if (pk) {
        MiscScope ms(ctx, s);
        TS_HIP(launch_unpack_rows(h, row0, lens, B, T, HID, w.H.f(), s));
    }
    if (hidden_out) TS_HIP(hipMemcpyAsync(hidden_out, w.H.f(), M * HID * F, hipMemcpyDeviceToDevice, s));
    // ---- audio_feature_map | id channels ----
    TS_TRY(linear_masked(f->afm, w.H.f(), HID, w.X320.f(), CIN, 0, 256));
    if (f->NCLS > 0) {
        MiscScope ms(ctx, s);
        if (mx) TS_HIP(launch_fill_id_lens(id, f->NCLS, f->id_w.f(), f->id_b.f(), 64, w.X320.f(), 320, 256, B, T, lens, s));
        else TS_HIP(launch_fill_id(id, f->NCLS, f->id_w.f(), f->id_b.f(), 64, w.X320.f(), 320, 256, B, T, s));
    }
    // ---- SeqTranslator1D: 3 x {conv, LN, + residual, ReLU} ----
    TS_TRY(conv(f->fn[0], w.X320.f(), CIN, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    if (CIN != 256) TS_TRY(conv(f->fn0res, w.X320.f(), CIN, B, T, T, 1, nullptr, 0, w.R.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->fn_ln[0], CIN != 256 ? w.R.f() : w.X320.f(), 1, w.Y2.f()));
    TS_TRY(conv(f->fn[1], w.Y2.f(), 256, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->fn_ln[1], w.Y2.f(), 1, w.R.f()));
    TS_TRY(conv(f->fn[2], w.R.f(), 256, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->fn_ln[2], w.R.f(), 1, w.Y2.f()));     // feature = Y2
    // ---- jaw head (64 ch) ----
    TS_TRY(conv(f->dec[0][0], w.Y2.f(), 256, B, T, T, 1, nullptr, 0, w.D1.f(), 64, 0, 64, 0));
    TS_TRY(ln(w.D1.f(), 64, f->dec_ln[0][0], nullptr, 1, w.D2.f()));
    TS_TRY(conv(f->dec[0][1], w.D2.f(), 64, B, T, T, 1, nullptr, 0, w.D1.f(), 64, 0, 64, 0));
    TS_TRY(ln(w.D1.f(), 64, f->dec_ln[0][1], nullptr, 1, w.D2.f()));
    TS_TRY(conv(f->dec[0][2], w.D2.f(), 64, B, T, T, 1, nullptr, 0, w.D1.f(), 64, 0, 64, 0));
    TS_TRY(ln(w.D1.f(), 64, f->dec_ln[0][2], nullptr, 1, w.D2.f()));
    TS_TRY(linear_masked(f->fin[0], w.D2.f(), 64, out, OUTW, 0, JAW));
    // ---- expression head (256 ch) ----
    TS_TRY(conv(f->dec[1][0], w.Y2.f(), 256, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->dec_ln[1][0], nullptr, 1, w.R.f()));
    TS_TRY(conv(f->dec[1][1], w.R.f(), 256, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->dec_ln[1][1], nullptr, 1, w.R.f()));
    TS_TRY(conv(f->dec[1][2], w.R.f(), 256, B, T, T, 1, nullptr, 0, w.Y1.f(), 256, 0, 256, 0));
    TS_TRY(ln(w.Y1.f(), 256, f->dec_ln[1][2], nullptr, 1, w.R.f()));
    TS_TRY(linear_masked(f->fin[1], w.R.f(), 256, out, OUTW, JAW, 100));
    return 0;
}
}  // namespace
