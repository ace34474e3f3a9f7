// Host-side helpers shared by models.cpp / pixelcnn.cpp / sampler_host.cpp / api.cpp: error channel, device buffers, the
// reference-state_dict view, the launch wrappers that feed the per-family profiler.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/talkshow_hip.h"
#include "../../include/talkshow_hip_debug.h"
#include "kernels.h"

namespace ts {

void set_error(const std::string &m);
inline int fail(const std::string &m) {
    set_error(m);
    return 1;
}

#define TS_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) return ::ts::fail(std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define TS_TRY(expr)              \
    do {                          \
        int r__ = (expr);         \
        if (r__ != 0) return r__; \
    } while (0)

// The synchronous hipMemcpy is refused by the runtime (hipErrorStreamCaptureImplicit) while ANY host thread captures a graph, in every capture
// mode, and the refusal invalidates that thread's capture.  The asynchronous copy on the same (legacy) stream and a wait for that stream are
// not refused, and order and complete the same way: what every copy that can run beside another thread's call goes through.
inline hipError_t copy_and_wait(void *dst, const void *src, size_t n, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, nullptr);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int ensure(size_t n) {   // grow-only; contents are NOT preserved
        if (n <= bytes) return 0;
        release();
        TS_HIP(hipMalloc(&p, n));
        bytes = n;
        return 0;
    }
    int upload(const void *host, size_t n) {
        TS_TRY(ensure(n));
        TS_HIP(copy_and_wait(p, host, n, hipMemcpyHostToDevice));
        return 0;
    }
    float *f() const { return static_cast<float *>(p); }
    int *i() const { return static_cast<int *>(p); }
};

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- per-stream scratch --------------------------------------------------------------------------------------
// Every model object keeps one Work (activation arena, captured graphs) per HIP stream, created on the stream's first
// call, so independent batches can be in flight on different streams against one weight copy.  Lookups are serialised:
// two host threads may make their first call on two new streams at the same time.  A Work itself is only ever touched
// by the thread driving its stream (contract in talkshow_hip.h: one host thread per stream at a time).
// ts_stream_destroy() evicts the Work of the dying stream from every live object (a later stream could reuse the handle
// value and would otherwise inherit graphs captured for the old one).
struct StreamScoped {
    StreamScoped();
    virtual ~StreamScoped();
    virtual void drop_stream(hipStream_t s) = 0;
    StreamScoped(const StreamScoped &) = delete;
    StreamScoped &operator=(const StreamScoped &) = delete;
};
void drop_stream_everywhere(hipStream_t s);

template <class W>
struct StreamWorks : StreamScoped {
    std::mutex mu;
    std::map<hipStream_t, std::unique_ptr<W>> m;
    W &get(hipStream_t s) {
        std::lock_guard<std::mutex> g(mu);
        auto &w = m[s];
        if (!w) w.reset(new W());
        return *w;
    }
    W *find(hipStream_t s) {
        std::lock_guard<std::mutex> g(mu);
        auto it = m.find(s);
        return it == m.end() ? nullptr : it->second.get();
    }
    void drop_stream(hipStream_t s) override {
        std::lock_guard<std::mutex> g(mu);
        m.erase(s);
    }
};

// relaxed atomic accumulate for the always-on diagnostic counters (several host threads may launch concurrently)
inline void atomic_add(std::atomic<double> &a, double v) {
    double cur = a.load(std::memory_order_relaxed);
    while (!a.compare_exchange_weak(cur, cur + v, std::memory_order_relaxed)) {
    }
}

// view of a reference state_dict, "module." prefixes stripped (nets/smplx_body_pixel.py:119-126)
struct StateDict {
    std::map<std::string, const ts_tensor *> m;
    StateDict(const ts_tensor *t, int n) {
        for (int i = 0; i < n; ++i) {
            std::string k = t[i].name ? t[i].name : "";
            size_t pos;
            while ((pos = k.find("module.")) != std::string::npos) k.erase(pos, 7);
            m[k] = &t[i];
        }
    }
    // returns nullptr (and sets the error) if missing or shape mismatch
    const float *get(const std::string &key, std::initializer_list<int64_t> shape) const {
        auto it = m.find(key);
        if (it == m.end() || !it->second->data) {
            set_error("state_dict: missing key '" + key + "'");
            return nullptr;
        }
        const ts_tensor *t = it->second;
        bool ok = t->ndim == (int)shape.size();
        int i = 0;
        for (int64_t s : shape) {
            if (ok && t->shape[i] != s) ok = false;
            ++i;
        }
        if (!ok) {
            std::string got = "(", want = "(";
            for (int j = 0; j < t->ndim; ++j) got += std::to_string(t->shape[j]) + ",";
            for (int64_t s : shape) want += std::to_string(s) + ",";
            set_error("state_dict: shape mismatch for '" + key + "': got " + got + ") want " + want + ")");
            return nullptr;
        }
        return t->data;
    }
};

// ---- per-family device-time profiler (ts_prof_*) ------------------------------------------------------------
enum { FAM_CONV = 0, FAM_SKINNY = 1, FAM_MISC = 2, FAM_ATTN = 3, FAM_COUNT = 4 };

struct Profiler {
    bool on = false;
    struct Rec {
        hipEvent_t a, b;
        int fam;
        double flops = 0;
        std::string tag;   // TS_PROF_LOG=1: per-launch line printed by collect()
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double ms[FAM_COUNT] = {};
    double flops[FAM_COUNT] = {};
    long launches[FAM_COUNT] = {};
    hipEvent_t get_event();
    void begin(int fam, hipStream_t s);
    void end(hipStream_t s);
    int collect();   // synchronises the recorded events and folds them into ms[]
    void reset();
    ~Profiler();
};

}  // namespace ts

struct ts_ctx {
    int device = 0;
    ts::Profiler prof;
    // always-on launch / algorithmic-flop counters per kernel family (cheap host-side bookkeeping)
    std::atomic<long> n_launch[ts::FAM_COUNT] = {};
    std::atomic<double> n_flops[ts::FAM_COUNT] = {};
    ts::DevBuf neg1;   // a single int32 -1 (gather index meaning "zero row")
};

namespace ts {

int run_conv(ts_ctx *ctx, const ConvParams &p, int tile, hipStream_t s);
int run_skinny(ts_ctx *ctx, const SkinnyParams &p, hipStream_t s);
int run_skinny_batch(ts_ctx *ctx, const SkinnyParams *const *ps, int n, hipStream_t s);
// What run_skinny / run_skinny_batch issue on THIS host thread while a tally is installed: the capturing call of pixelcnn.cpp counts its
// own graph with it (the context-wide counters above also move with every other thread inside the library).  Thread-local, never nested.
struct SkinnyTally {
    long launches = 0;
    double flops = 0;
    SkinnyTally();
    ~SkinnyTally();
    SkinnyTally(const SkinnyTally &) = delete;
    SkinnyTally &operator=(const SkinnyTally &) = delete;
};
// misc launches are wrapped with this scope guard so they show up under FAM_MISC
struct MiscScope {
    ts_ctx *ctx;
    hipStream_t s;
    MiscScope(ts_ctx *c, hipStream_t st, int fam = FAM_MISC, double flops = 0.0) : ctx(c), s(st) {
        if (ctx->prof.on) {
            ctx->prof.begin(fam, s);
            ctx->prof.flops[fam] += flops;
        }
    }
    ~MiscScope() {
        if (ctx->prof.on) ctx->prof.end(s);
    }
};

// ---- a folded + packed convolution layer -------------------------------------------------------------------
struct ConvLayer {
    int kind = 0;   // 0: stride-1 (k1 / k3), 1: down (k4 s2 p1), 2: up (ConvTranspose k4 s2 p1)
    int cin = 0, cin_pad = 0, cout = 0, cout_pad = 0, npad = 0, ktot = 0;
    int act = 0;
    int ngroups = 1, nseg = 0;
    ConvSeg segs[2][4];
    DevBuf w, bias;   // [ngroups][npad][ktot], [ngroups][npad]
    DevBuf wp;        // face generator, x3 plan only: w as bf16 plane images (launch_split_weight_planes)
    DevBuf wino;      // lowered layers only (kernels.h::wino_lowered): the six Winograd matrices [6][npad][cin]; w stays packed for TS_CONV_WINO=0
    std::string name;
};

// Packs one reference layer: conv `conv_key` (+ BatchNorm `norm_key` folded, + parallel residual conv
// `res_key` folded) into `out`.  kind as above; k = kernel size for kind 0 (1 or 3).
int pack_conv_layer(const StateDict &sd, const std::string &conv_key, const std::string &norm_key,
                    const std::string &res_key, int kind, int k, int cin, int cout, int act, ConvLayer *out);
// generic: pack an (N,K) row-major matrix (+bias) as a k1 ConvLayer (used for the PixelCNN audio precompute)
int pack_linear_layer(const float *w, long ldw, const float *bias, int N, int K, ConvLayer *out);

// raw form: w (cout, cin, K) reference layout, optional bias; taps[k] = input row shift of kernel index k
int pack_conv_raw(const float *w, const float *bias, int cout, int cin, int K, const int *taps, int act, ConvLayer *out);

// Fills ConvParams for `layer` applied to x (B, Lin, ldx) -> out; returns Lout (rows per clip of the output buffer).
// For kind 2 the output buffer has 2*Lin rows of cout_pad (or ldo) floats.
int conv_layer_params(const ConvLayer &layer, const float *x, int ldx, int B, int Lin, const float *res, int ldr,
                      float *out, int ldo, int out_col0, int n_store, ConvParams *p);

// models.cpp: the six GEMMs per network of a Winograd-lowered layer (V, U, O of n = 1 or 2 networks; U rows npad apart) as one batched launch
// (one_v: all six multiply the one (M, C) matrix V[i] points to)
int run_wino_gemm(ts_ctx *ctx, int n, const float *const *V, const float *const *U, float *const *O, int M, int c, int npad, hipStream_t s,
                  bool one_v = false);

// accessors so that api.cpp needs no knowledge of the model structs
int convnet_hidden(const ts_convnet *n);
// face.cpp, host arithmetic only: the work list of a mixed pass's attention launch (one word per workgroup id; see there).  Returns the number
// of workgroups, -1 on a bad table
int face_mixed_grid(const int32_t *frames, int B, int heads, std::vector<int> &work);
// face.cpp, host arithmetic only: the row layout of a packed mixed pass (see there).  feat_off / row0 hold B + 1 entries (the last = the total);
// len[i] = rows of level i of the feature chain run as one problem.  0, or -1 on a bad table or a row count the engines cannot index
struct FacePacked {
    std::vector<int> feat_off, row0;
    long feat_rows = 0, rows = 0;
    int len[7] = {};
};
constexpr int FACE_FC_K[6] = {3, 3, 3, 3, 2, 2};   // kernel sizes of the six stride-2 feature convolutions (wav2vec2 base)
int face_packed_layout(const int32_t *ns, const int32_t *frames, int B, FacePacked *out);
int vqvae_in_dim(const ts_vqvae *v);
// models.cpp: both VQ encoders over clips of different lengths, codes into a (B, codes_H, 2) block (codes_H >= T_max / 4); form: launch_vq_argmin_pair_masked
int vq_encode_pair_masked(ts_vqvae *vb, ts_vqvae *vh, const float *poses, int poses_ld, const int32_t *lens_dev, int B, int T_max, int64_t *codes,
                          int codes_H, float *z_body, float *z_hand, int form, hipStream_t s);

// ---- mixed passes: the arguments behind the exported ts_*_mixed* ladders (talkshow_hip.h has every contract) -----------------
// What every mixed entry takes, in the entries' own order: `rows` is H_max for the PixelCNN, T_max for the body wrapper
struct MixedPass {
    const int64_t *ids;
    const int32_t *lens_host, *lens_dev;
    int B, rows, mode;
    const float *uniforms;
    uint64_t seed;
    const int64_t *clip_index;
    int64_t *codes;
};
// What a mixed entry MAY take: a suffixed entry sets the fields its parameters name; null / 0 is the entry without that keyword
struct MixedOpts {
    const ts_sampling *ctl_host = nullptr;   // sampling controls
    int n_ctl = 0;
    float *logprob = nullptr;                // log-probabilities
    const int64_t *given = nullptr;          // given rows
    const int32_t *given_rows_host = nullptr;
    const uint8_t *keep = nullptr;           // kept positions
    const float *style = nullptr;            // speaker style
    int style_rows = 0;
    const float *bias = nullptr;             // code bias
    int n_bias = 0;
    const int32_t *bias_index_host = nullptr;
    const ts_repeat *rep_host = nullptr;     // repetition penalty
    int n_rep = 0;
    const int32_t *guide_host = nullptr;     // guidance: (B,) the shadow's slot of every clip slot or -1, and (B,) the scales
    const float *guide_scale_host = nullptr;
    const ts_alt_out *alt = nullptr;         // alternatives: the record of the four outputs
    // the body wrapper only: given poses
    const float *given_poses = nullptr;
    int P_max = 0;
    const int32_t *pose_lens_host = nullptr, *pose_lens_dev = nullptr;
};
// pixelcnn.cpp: the one body behind ts_pixelcnn_generate_mixed and its suffixed siblings (a.ids the labels, a.rows = H_max)
int pixelcnn_generate_mixed(ts_pixelcnn *p, const float *aud, const MixedPass &a, const MixedOpts &o, hipStream_t s);
// the checks both levels make with one text: `who` the entry family the messages name, `rows_name` what it calls its H code rows
inline int mixed_style_rows_check(const char *who, const char *rows_name, const MixedOpts &o, int H) {
    if (!o.style || o.style_rows == 1 || o.style_rows == H) return 0;
    return fail(std::string(who) + "_style: style_rows is 1 or " + rows_name + " = " + std::to_string(H) + ", got " + std::to_string(o.style_rows));
}
// who_keep / who_given: the entries the two messages name
inline int mixed_given_check(const char *who_keep, const char *who_given, const MixedOpts &o, const int32_t *lens_host, int B) {
    if (o.keep && !o.given) return fail(std::string(who_keep) + ": a mask of kept positions needs the given codes it selects from");
    if (!o.given) return 0;
    if (!o.given_rows_host) return fail(std::string(who_given) + ": given codes need their row table");
    return ts_given_rows_check(o.given_rows_host, lens_host, B);
}

// ---- a pass's sampler tables (sampler_host.cpp) -----------------------------------------------------------------------------
// The host side of the per-clip sampling pieces of ONE pass (a mixed pass, a session step, a one-shot call with a table), in three steps:
// build() checks what `o` brought, in one order for every caller, and leaves the device records here; the pass's owner then stages them
// into its Work in stream order and binds its run configuration to the Work's buffers (pixelcnn.cpp: stage_sampler_tables,
// bind_sampler_tables).  What differs between callers happens between the steps, on the vectors (a session makes from_row and the given
// bounds absolute), never inside them.
// The entries the messages of build() name: a table's faults, neutral records under a bias / under repetition records, a mask, given codes
struct SamplerNames {
    const char *ctl, *bias, *rep, *keep, *given;
    const char *guide = "ts_guide_check";   // neutral records under a guide table
    const char *alt = "alternatives";       // the refusals of a pass that brings a ts_alt_out record
};
inline SamplerNames sampler_names(const char *who) { return {who, who, who, who, who, who, who}; }   // an entry that names itself throughout
struct SamplerTables {
    int B = 0;
    std::vector<SampleCtl> ctl;        // B records where a table, a bias or repetition records came (neutral ones without a table), else empty
    std::vector<SampleRep> rep;        // B records where repetition records came
    std::vector<int32_t> no_bias;      // B times -1 where repetition records came without bias tables: the index the samplers want
    std::vector<int32_t> given_rows;   // a copy of o.given_rows_host where given codes came
    // guidance: B roles (-1 plain, g >= 0 the shadow's slot, -2 a shadow) and B scales where a guide table came, else empty.  A guided pass
    // runs the BIAS and REP arithmetic: ctl, rep (window 0) and no_bias are then filled with neutral values where their pieces did not come
    std::vector<int32_t> guide_role;
    std::vector<float> guide_scale;
    // alternatives: the record came (checked).  ctl, rep (window 0) and no_bias are then filled with neutral values where their pieces did
    // not come, as under guidance: the pass runs on the most general unguided samplers
    bool alt = false;
    // Launches nothing.  lens_host: the frames a clip's given rows must fit (>> 2), read only where given codes came
    int build(const MixedOpts &o, int B, int V, int mode, const int32_t *lens_host, const SamplerNames &who);
};

}  // namespace ts
