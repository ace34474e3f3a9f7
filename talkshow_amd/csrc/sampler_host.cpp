// The host rules of the per-clip sampling pieces (talkshow_hip.h: sampling controls, given rows, kept positions, speaker style, code bias,
// repetition penalty), none of which knows a network: the exported ts_*_check rules, the device records a pass makes of the public ones
// (SamplerTables::build, host_common.h), and the kernel-level test entries ts_op_sample_* / ts_op_style_rows.  pixelcnn.cpp stages and
// binds what build() leaves.
#include <algorithm>

#include "host_common.h"

using namespace ts;

namespace {

// ---- sampling controls (talkshow_hip.h: ts_sampling) ------------------------------------------------------------------------------------
// the rules of ts_sampling_check on one record; 0 or the message's tail
const char *ctl_fault(const ts_sampling &r) {
    if (!(r.temperature > 0.0f) || !std::isfinite(r.temperature)) return "temperature must be finite and > 0";
    if (!std::isfinite(1.0f / r.temperature)) return "1 / temperature overflows fp32";
    if (!(r.top_p > 0.0f) || !(r.top_p <= 1.0f)) return "top_p must be in (0, 1]";
    if (r.top_k < 0) return "top_k must be >= 0 (0 or >= V: off)";
    if (r.reserved != 0) return "reserved must be 0";
    return nullptr;
}
int ctl_check(const ts_sampling *ctl, int n, int V, const char *who) {
    if (!ctl || n < 1 || V < 1) return fail(std::string(who) + ": bad argument");
    if (V > SAMPLE_CTL_MAX_V)
        return fail(std::string(who) + ": sampling controls support vocabularies of at most " + std::to_string(SAMPLE_CTL_MAX_V) + " classes, got V = " + std::to_string(V));
    for (int b = 0; b < n; ++b)
        if (const char *m = ctl_fault(ctl[b])) return fail(std::string(who) + ": sampling record of clip " + std::to_string(b) + ": " + m);
    return 0;
}
// validated host table -> the B device records of a pass (n_ctl = 1: one record for all clips); 1 / temperature is computed HERE, once, in fp32
int ctl_table(const ts_sampling *ctl, int n_ctl, int B, int V, int mode, const char *who, std::vector<SampleCtl> &tab) {
    if (mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX)
        return fail(std::string(who) + ": sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip greedy is top_k = 1)");
    if (n_ctl != 1 && n_ctl != B) return fail(std::string(who) + ": n_ctl must be 1 or B");
    TS_TRY(ctl_check(ctl, n_ctl, V, who));
    tab.resize(B);
    for (int b = 0; b < B; ++b) {
        const ts_sampling &r = ctl[n_ctl == 1 ? 0 : b];
        tab[b] = SampleCtl{1.0f / r.temperature, r.top_p, r.top_k, 0};
    }
    return 0;
}

// n_rep (1 or B) checked records -> one device record per clip slot
int rep_table(const ts_repeat *rep_host, int n_rep, int B, int V, const char *who, std::vector<SampleRep> &tab) {
    if (n_rep != 1 && n_rep != B)
        return fail(std::string(who) + ": a pass of " + std::to_string(B) + " clips brings 1 or " + std::to_string(B) + " repetition records, got " +
                    std::to_string(n_rep));
    TS_TRY(ts_repeat_check(rep_host, n_rep, V));
    tab.resize(B);
    for (int b = 0; b < B; ++b) {
        const ts_repeat &r = rep_host[n_rep == 1 ? 0 : b];
        tab[b] = SampleRep{r.window, r.presence, r.frequency, 0};
    }
    return 0;
}

}  // namespace

extern "C" {

int ts_sampling_check(const ts_sampling *ctl_host, int n, int V) { return ctl_check(ctl_host, n, V, "ts_sampling_check"); }

// Host only ("code bias"): tables (n_tables,2,V) — every entry -inf or finite with |b| <= 1e30 (no NaN, no +inf), every row with at least
// one entry above -inf, V within the controls' limit; the message names the table, the column and the code
int ts_code_bias_check(const float *tables_host, int n_tables, int V) {
    if (!tables_host || n_tables < 1 || V < 1) return fail("ts_code_bias_check: bad argument");
    if (V > SAMPLE_CTL_MAX_V)
        return fail("ts_code_bias_check: a code bias supports vocabularies of at most " + std::to_string(SAMPLE_CTL_MAX_V) + " classes, got V = " +
                    std::to_string(V));
    static const char *const col[2] = {"body", "hand"};
    for (int t = 0; t < n_tables; ++t)
        for (int j = 0; j < 2; ++j) {
            const float *row = tables_host + ((size_t)t * 2 + j) * V;
            const std::string where = "ts_code_bias_check: table " + std::to_string(t) + ", " + col[j] + " column";
            bool any = false;
            for (int v = 0; v < V; ++v) {
                const float x = row[v];
                if (std::isnan(x)) return fail(where + ": the bias of code " + std::to_string(v) + " is NaN");
                if (std::isinf(x)) {
                    if (x > 0) return fail(where + ": the bias of code " + std::to_string(v) + " is +inf (only -inf, a ban, is allowed)");
                    continue;
                }
                if (std::fabs(x) > 1e30f) return fail(where + ": the bias of code " + std::to_string(v) + " exceeds 1e30 in magnitude");
                any = true;
            }
            if (!any) return fail(where + ": every code is banned (-inf); a column needs at least one code it may use");
        }
    return 0;
}

// Host only ("code bias"): what every entry that takes tables checks of their number and of the index table before anything is launched
int ts_code_bias_index_check(const int32_t *bias_index_host, int B, int n_bias) {
    if (!bias_index_host || B < 1) return fail("ts_code_bias_index_check: bad argument");
    if (n_bias < 1 || n_bias > B)
        return fail("code bias: a pass of " + std::to_string(B) + " clips brings 1 to " + std::to_string(B) + " tables (shared tables travel once), got " +
                    std::to_string(n_bias));
    for (int b = 0; b < B; ++b)
        if (bias_index_host[b] < -1 || bias_index_host[b] >= n_bias)
            return fail("code bias: the table index of clip " + std::to_string(b) + " is " + std::to_string(bias_index_host[b]) + ", not -1 (none) or in [0, " +
                        std::to_string(n_bias) + ")");
    return 0;
}

// Host only ("repetition penalty"): n records — window in [0, 64], presence and frequency finite with |x| <= 1e30, reserved 0 — for a
// vocabulary within the controls' limit; the message names the clip
int ts_repeat_check(const ts_repeat *rep_host, int n, int V) {
    if (!rep_host || n < 1 || V < 1) return fail("ts_repeat_check: bad argument");
    if (V > SAMPLE_CTL_MAX_V)
        return fail("ts_repeat_check: a repetition penalty supports vocabularies of at most " + std::to_string(SAMPLE_CTL_MAX_V) +
                    " classes, got V = " + std::to_string(V));
    for (int b = 0; b < n; ++b) {
        const ts_repeat &r = rep_host[b];
        const std::string where = "ts_repeat_check: clip " + std::to_string(b);
        if (r.window < 0 || r.window > TS_REPEAT_MAX_WINDOW)
            return fail(where + ": window " + std::to_string(r.window) + " is outside [0, " + std::to_string(TS_REPEAT_MAX_WINDOW) + "]");
        const float v[2] = {r.presence, r.frequency};
        static const char *const name[2] = {"presence", "frequency"};
        for (int k = 0; k < 2; ++k) {
            if (std::isnan(v[k])) return fail(where + ": " + name[k] + " is NaN");
            if (std::isinf(v[k])) return fail(where + ": " + name[k] + " is infinite");
            if (std::fabs(v[k]) > 1e30f) return fail(where + ": " + name[k] + " exceeds 1e30 in magnitude");
        }
        if (r.reserved != 0) return fail(where + ": the reserved word is " + std::to_string(r.reserved) + ", not 0");
    }
    return 0;
}

// Host only ("guidance"): guide (B,) the shadow's slot of every clip slot or -1, scale (B,) floats (read where guide[b] >= 0), lens (B,)
// the slots' lengths IN FRAMES as the pass entries take them, compared as they are (NULL: a launch whose rows have no lengths).  Refuses, naming the slot: an index outside [-1, B), a slot that names
// itself, a shadow named twice, a shadow that is itself guided, unequal lengths, a NaN or an infinity, |scale| > 1e4
int ts_guide_check(const int32_t *guide_host, const float *scale_host, const int32_t *lens_host, int B) {
    if (!guide_host || !scale_host || B < 1) return fail("ts_guide_check: bad argument");
    std::vector<int> named(B, -1);   // the primary that names a slot as its shadow
    for (int b = 0; b < B; ++b) {
        const int g = guide_host[b];
        const std::string where = "ts_guide_check: clip " + std::to_string(b);
        if (g < -1 || g >= B) return fail(where + ": the shadow index is " + std::to_string(g) + ", not -1 (none) or in [0, " + std::to_string(B) + ")");
        if (g < 0) continue;
        if (g == b) return fail(where + " names itself as its shadow");
        if (named[g] >= 0) return fail(where + ": its shadow, slot " + std::to_string(g) + ", is already the shadow of clip " + std::to_string(named[g]));
        named[g] = b;
    }
    for (int b = 0; b < B; ++b) {
        const int g = guide_host[b];
        if (g < 0) continue;
        const std::string where = "ts_guide_check: clip " + std::to_string(b);
        if (guide_host[g] >= 0) return fail(where + ": its shadow, slot " + std::to_string(g) + ", is itself guided (a shadow draws nothing)");
        if (named[b] >= 0) return fail(where + " is guided and is the shadow of clip " + std::to_string(named[b]) + " (a shadow draws nothing)");
        if (lens_host && lens_host[g] != lens_host[b])
            return fail(where + ": its length of " + std::to_string(lens_host[b]) + " frames differs from the " + std::to_string(lens_host[g]) + " frames of its shadow, slot " +
                        std::to_string(g));
        const float sc = scale_host[b];
        if (std::isnan(sc)) return fail(where + ": the scale is NaN");
        if (std::isinf(sc)) return fail(where + ": the scale is infinite");
        if (std::fabs(sc) > 1e4f) return fail(where + ": the scale exceeds 1e4 in magnitude");
    }
    return 0;
}

// Host only ("alternatives"): the record of a pass and the mode it runs in
int ts_alt_check(const ts_alt_out *alt, int mode) {
    if (!alt) return fail("ts_alt_check: bad argument");
    if (alt->n < 0 || alt->n > TS_ALT_MAX)
        return fail("ts_alt_check: n = " + std::to_string(alt->n) + " is outside [0, " + std::to_string(TS_ALT_MAX) + "]");
    if (alt->reserved != 0) return fail("ts_alt_check: the reserved word is " + std::to_string(alt->reserved) + ", not 0");
    if (!alt->entropy_dev || !alt->rank_dev) return fail("ts_alt_check: entropy_dev and rank_dev are required");
    if (alt->n > 0 && (!alt->codes_dev || !alt->logprob_dev)) return fail("ts_alt_check: n > 0 needs codes_dev and logprob_dev");
    if (mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX)
        return fail("ts_alt_check: alternatives need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip greedy is top_k = 1 under a drawing mode)");
    return 0;
}

// Host only: the rule every _given entry applies to its row table before anything is launched
int ts_given_rows_check(const int32_t *given_rows_host, const int32_t *lens_host, int B) {
    if (!given_rows_host || !lens_host || B < 1) return fail("ts_given_rows_check: bad argument");
    for (int b = 0; b < B; ++b)
        if (given_rows_host[b] < 0 || given_rows_host[b] > (lens_host[b] >> 2))
            return fail("given rows of clip " + std::to_string(b) + ": G = " + std::to_string(given_rows_host[b]) + " must be in [0, " +
                        std::to_string(lens_host[b] >> 2) + "], the clip's own code rows");
    return 0;
}

// Host only (tests): the device records rep_table makes of n_rep (1 or B) public records, four 32-bit words per clip slot into words_out
int ts_debug_rep_table(const ts_repeat *rep_host, int n_rep, int B, int V, int32_t *words_out) {
    if (!rep_host || !words_out || B < 1) return fail("ts_debug_rep_table: bad argument");
    std::vector<SampleRep> tab;
    TS_TRY(rep_table(rep_host, n_rep, B, V, "ts_debug_rep_table", tab));
    std::memcpy(words_out, tab.data(), (size_t)B * sizeof(SampleRep));
    return 0;
}

}  // extern "C"

int ts::SamplerTables::build(const MixedOpts &o, int B_, int V, int mode, const int32_t *lens_host, const SamplerNames &who) {
    B = B_;
    if (o.ctl_host) TS_TRY(ctl_table(o.ctl_host, o.n_ctl, B, V, mode, who.ctl, ctl));   // before anything is launched
    if (o.bias || o.rep_host) {   // sampling controls with the table's scope; without a table the pass runs on neutral records (the plain sampler's bits)
        if (!o.ctl_host) {
            const ts_sampling neutral = {1.0f, 1.0f, 0, 0};
            TS_TRY(ctl_table(&neutral, 1, B, V, mode, o.rep_host ? who.rep : who.bias, ctl));   // refuses greedy and teacher forced
        }
        if (o.bias) TS_TRY(ts_code_bias_index_check(o.bias_index_host, B, o.n_bias));
    }
    if (o.rep_host) {
        TS_TRY(rep_table(o.rep_host, o.n_rep, B, V, who.rep, rep));
        if (!o.bias) no_bias.assign(B, -1);   // a pass without tables brings the index the BIAS path wants
    }
    TS_TRY(mixed_given_check(who.keep, who.given, o, lens_host, B));
    if (o.given) given_rows.assign(o.given_rows_host, o.given_rows_host + B);
    if (o.guide_host) {   // last: the refusals above keep their order and text
        if (ctl.empty()) {   // a sampling control like the bias: neutral records, which refuse greedy and teacher forced
            const ts_sampling neutral = {1.0f, 1.0f, 0, 0};
            TS_TRY(ctl_table(&neutral, 1, B, V, mode, who.guide, ctl));
        }
        TS_TRY(ts_guide_check(o.guide_host, o.guide_scale_host, lens_host, B));
        guide_role.assign(o.guide_host, o.guide_host + B);
        guide_scale.assign(B, 0.0f);
        for (int b = 0; b < B; ++b)
            if (o.guide_host[b] >= 0) {
                guide_role[o.guide_host[b]] = -2;
                guide_scale[b] = o.guide_scale_host[b];
            }
        // the guided samplers run the BIAS and REP paths: an index of -1 and records of window 0 are "same arithmetic" there
        if (!o.bias && no_bias.empty()) no_bias.assign(B, -1);
        if (rep.empty()) rep.assign(B, SampleRep{0, 0.0f, 0.0f, 0});
    }
    if (o.alt) {   // behind every check there was: the refusals above keep their order and text
        TS_TRY(ts_alt_check(o.alt, mode));
        if (o.guide_host) return fail(std::string(who.alt) + ": a guided pass (a session with pairs) returns no alternatives");
        if (!o.logprob) return fail(std::string(who.alt) + ": the record needs logprob_dev beside it");
        if (ctl.empty()) {
            const ts_sampling neutral = {1.0f, 1.0f, 0, 0};
            TS_TRY(ctl_table(&neutral, 1, B, V, mode, who.alt, ctl));
        }
        // the samplers run the BIAS and REP paths: an index of -1 and records of window 0 are "same arithmetic" there
        if (!o.bias && no_bias.empty()) no_bias.assign(B, -1);
        if (rep.empty()) rep.assign(B, SampleRep{0, 0.0f, 0.0f, 0});
        alt = true;
    }
    return 0;
}

namespace {

// What a ts_op_sample_* entry brought: each copies its own parameters, so a piece the entry does not have is null here and the body's
// rules for it never fire.  `missing`: one of the entry's own required pointers is null; `modes`: the entry takes modes 0 .. modes - 1
// (0: the mode is left to ctl_table)
struct OpSample {
    const char *who;
    bool missing;
    int modes;
    ts_ctx *ctx;
    const float *logits;
    int B, V, mode;
    const float *uniforms;
    uint64_t seed;
    int64_t clip_index0;
    uint32_t position;
    int64_t *idx;
    void *stream;
    uint8_t *kept = nullptr;
    float *logprob = nullptr;
    const int32_t *forced_host = nullptr, *given_rows_host = nullptr;
    const uint8_t *keep = nullptr;
    const int64_t *given = nullptr;
    float *logits_copy = nullptr;
    MixedOpts o;   // the sampling table, the bias, the repetition records and the guide table, as a pass takes them
    int column = 0;
    const int32_t *history = nullptr;
    int32_t *ring_out = nullptr;
};

// The one body of the six entries: the checks in the entries' common order, the uploads, one fill of SampleParams, one launch
int op_sample(const OpSample &a) {
    const std::string who = a.who;
    const MixedOpts &o = a.o;
    const int B = a.B, V = a.V;
    if (!a.ctx || !a.logits || !a.idx || a.missing) return fail(who + ": null argument");
    const int hist_rows = (int)std::min<uint32_t>(a.position >> 1, (uint32_t)SAMPLE_REP_RING);
    if (o.rep_host && hist_rows > 0 && !a.history) return fail(who + ": rows behind row 0 need their history");
    if (!o.rep_host && !o.guide_host && (a.history || a.ring_out)) return fail(who + ": a history and a ring output need records");
    if (B < 1 || V < 1) return fail(who + ": bad shape");
    if (a.column != 0 && a.column != 1) return fail(who + ": column is 0 (body) or 1 (hand)");
    if (a.modes && (a.mode < 0 || a.mode >= a.modes)) return fail(who + ": bad mode");
    if (a.mode == TS_SAMPLE_UNIFORMS && !a.uniforms) return fail(who + ": uniforms required");
    const bool pieces = o.bias || o.rep_host || o.guide_host || o.alt;   // they run on neutral records where no table came
    if (a.kept && !o.ctl_host && !pieces) return fail(who + ": kept_dev needs a table");
    const bool given_rows = a.forced_host || a.given_rows_host;
    if (given_rows) {
        if (!a.given) return fail(who + ": given rows need their codes");
        if (a.position > 0x7ffffff0u) return fail(who + ": position too large for a row table");
        for (int b = 0; a.given_rows_host && b < B; ++b)
            if (a.given_rows_host[b] < 0) return fail(who + ": given rows of row " + std::to_string(b) + " are negative");
    } else if (a.keep || a.given) {
        return fail(who + ": given codes and their mask need the row table");
    }
    SamplerTables t;
    TS_TRY(t.build(o, B, V, a.mode, nullptr, sampler_names(a.who)));
    // the kernels force a workgroup whose position is below 2 G: G = position / 2 + 1 forces row b at this position, G = 0 never does
    std::vector<int> rows(a.forced_host ? B : 0);
    for (size_t b = 0; b < rows.size(); ++b) rows[b] = a.forced_host[b] ? (int)(a.position / 2) + 1 : 0;

    hipStream_t s = (hipStream_t)a.stream;
    DevBuf tok, dtab, drows, dbi, drep, dring, drole, dscale;
    TS_TRY(tok.ensure((size_t)B * sizeof(int)));
    SampleGivenParams gp;
    std::memset(&gp, 0, sizeof(gp));
    SampleParams &sp = gp.c.s;
    sp.logits = a.logits;
    sp.B = B;
    sp.V = V;
    sp.mode = a.mode;
    sp.uniforms = a.uniforms;
    sp.u_stride = 1;
    sp.seed = a.seed;
    sp.clip_index0 = a.clip_index0;
    sp.position = a.position;
    sp.tok32 = tok.i();
    sp.tok_stride = 1;
    sp.codes = a.idx;
    sp.code_stride = 1;
    sp.logits_copy = a.logits_copy;
    sp.copy_stride = V;
    gp.c.kept = a.kept;
    gp.c.logprob = a.logprob;
    gp.c.lp_stride = 1;
    if (!t.ctl.empty()) {
        TS_TRY(dtab.ensure((size_t)B * sizeof(SampleCtl)));
        TS_HIP(launch_put_words(dtab.i(), reinterpret_cast<const int *>(t.ctl.data()), (long)B * 4, s));
        gp.c.ctl = static_cast<const SampleCtl *>(dtab.p);
    }
    if (pieces) {   // o.bias == NULL: no tables (an index of -1 everywhere)
        TS_TRY(dbi.ensure((size_t)B * sizeof(int32_t)));
        TS_HIP(launch_put_words(dbi.i(), o.bias ? o.bias_index_host : t.no_bias.data(), B, s));
        gp.c.bias = o.bias;
        gp.c.bias_index = static_cast<const int32_t *>(dbi.p);
        gp.c.bias_col = a.column;
    }
    const size_t ring_pitch = (size_t)2 * SAMPLE_REP_RING * sizeof(int32_t);   // one clip's two rings
    if (!t.guide_role.empty()) {
        TS_TRY(drole.ensure((size_t)B * sizeof(int32_t)));
        TS_TRY(dscale.ensure((size_t)B * sizeof(float)));
        TS_HIP(launch_put_words(drole.i(), t.guide_role.data(), B, s));
        TS_HIP(launch_put_words(dscale.i(), reinterpret_cast<const int *>(t.guide_scale.data()), B, s));
        gp.c.guide_role = static_cast<const int32_t *>(drole.p);
        gp.c.guide_scale = dscale.f();
    }
    if (!t.rep.empty()) {
        TS_TRY(drep.ensure((size_t)B * sizeof(SampleRep)));
        TS_TRY(dring.ensure((size_t)B * ring_pitch));
        TS_HIP(launch_put_words(drep.i(), reinterpret_cast<const int *>(t.rep.data()), (long)B * 4, s));
        TS_HIP(hipMemsetAsync(dring.p, 0xff, (size_t)B * ring_pitch, s));
        // rows r - R .. r - 1 are consecutive ring slots modulo 64: one or two strided copies
        const uint32_t first = (a.position >> 1) - (uint32_t)hist_rows;
        for (int done = 0; a.history && done < hist_rows;) {   // (a guided launch without records brings none: its windows are 0)
            const int slot = (int)((first + (uint32_t)done) & (uint32_t)(SAMPLE_REP_RING - 1));
            const int n = std::min(hist_rows - done, SAMPLE_REP_RING - slot);
            TS_HIP(hipMemcpy2DAsync(dring.i() + (size_t)a.column * SAMPLE_REP_RING + slot, ring_pitch, a.history + done,
                                    (size_t)hist_rows * sizeof(int32_t), (size_t)n * sizeof(int32_t), B, hipMemcpyDeviceToDevice, s));
            done += n;
        }
        gp.c.rep = static_cast<const SampleRep *>(drep.p);
        gp.c.rep_ring = dring.i();
    }
    if (given_rows) {
        TS_TRY(drows.ensure((size_t)B * sizeof(int)));
        TS_HIP(launch_put_words(drows.i(), a.forced_host ? rows.data() : a.given_rows_host, B, s));
        gp.rows = drows.i();
        gp.given = a.given;
        gp.given_stride = 1;
        gp.keep = a.keep;
        gp.keep_stride = 1;
    }
    if (t.alt) {   // one position per row
        TS_HIP(launch_sample_alt(SampleAltParams{gp, o.alt->n, o.alt->codes_dev, o.alt->logprob_dev, o.alt->entropy_dev, o.alt->rank_dev, 1}, s));
    } else if (given_rows) {
        TS_HIP(launch_sample_given(gp, s));
    } else if (gp.c.ctl) {
        TS_HIP(launch_sample_ctl(gp.c, s));
    } else if (a.logprob) {
        TS_HIP(launch_sample_lp(SampleLpParams{sp, a.logprob, 1}, s));
    } else {
        TS_HIP(launch_sample(sp, s));
    }
    if (!t.rep.empty() && a.ring_out)
        TS_HIP(hipMemcpy2DAsync(a.ring_out, (size_t)SAMPLE_REP_RING * sizeof(int32_t), dring.i() + (size_t)a.column * SAMPLE_REP_RING, ring_pitch,
                                (size_t)SAMPLE_REP_RING * sizeof(int32_t), B, hipMemcpyDeviceToDevice, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace

extern "C" {

// the sampler with controls on given logits (ts_op_sample / ts_op_sample_philox with a table; kernel-level tests call it)
int ts_op_sample_ctl(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                     uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, uint8_t *kept, void *stream) {
    if (!ctl_host) return fail("ts_op_sample_ctl: a table is required (ts_op_sample / ts_op_sample_philox are the entries without one)");
    return ts_op_sample_lp(ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, ctl_host, n_ctl, idx, kept, nullptr, stream);
}

// one sampler launch on given logits, with the log-probability of every row's code (kernel-level tests call it).  Without a table: any of
// the four modes through sample_lp_kernel (sample_kernel when logprob is NULL); teacher forced reads idx.  With one: ts_op_sample_ctl's launch.
int ts_op_sample_lp(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                    uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, uint8_t *kept, float *logprob, void *stream) {
    OpSample a{logprob ? "ts_op_sample_lp" : "ts_op_sample_ctl", false, 4, ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl, a.kept = kept, a.logprob = logprob;
    return op_sample(a);
}

// one launch of the samplers' given variants on given logits (kernel-level tests call it): row b is forced iff forced_host[b] != 0
int ts_op_sample_given(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                       uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *forced_host,
                       const int64_t *given, void *stream) {
    OpSample a{"ts_op_sample_given", !forced_host || !given, 3, ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl, a.logprob = logprob, a.forced_host = forced_host, a.given = given;
    return op_sample(a);
}

// one launch of the samplers' given variants on given logits with the DEVICE-side decision exercised (kernel-level tests call it): row b is
// forced iff position < 2 given_rows_host[b] and (keep == NULL or keep[b] != 0)
int ts_op_sample_keep(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                      uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *given_rows_host,
                      const uint8_t *keep, const int64_t *given, void *stream) {
    OpSample a{"ts_op_sample_keep", !given_rows_host || !given, 3, ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl, a.logprob = logprob, a.given_rows_host = given_rows_host, a.keep = keep, a.given = given;
    return op_sample(a);
}

// ts_op_sample_keep's launch under a "code bias" (kernel-level tests call it): bias (n_bias,2,V) device tables, bias_index_host (B,) the
// table of every row or -1, column 0 / 1.  Without a sampling table the rows run on neutral records.  given_rows_host == NULL: no given
// rows (sample_ctl_bias_kernel; given, keep unused); otherwise the given variant.  kept (optional, (B,V)): the kept bytes
int ts_op_sample_bias(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                      uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *given_rows_host,
                      const uint8_t *keep, const int64_t *given, uint8_t *kept, float *logits_copy, const float *bias, int n_bias,
                      const int32_t *bias_index_host, int column, void *stream) {
    if (!bias || !bias_index_host) return fail("ts_op_sample_bias: null argument");
    return ts_op_sample_repeat(ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, ctl_host, n_ctl, idx, logprob, given_rows_host, keep,
                               given, kept, logits_copy, bias, n_bias, bias_index_host, column, nullptr, 0, nullptr, nullptr, stream);
}

// The same launch under a "repetition penalty" (kernel-level tests call it): rep_host n_rep (1 or B) records; history (B,R) int32 on the
// device, R = min(position >> 1, 64), the codes of rows (position >> 1) - R .. (position >> 1) - 1 of this column, oldest first; ring_out
// (B,64) int32 or NULL.  The entry fills rings of -1, places the history where a pass would have left it (row r at r & 63), launches once
// and copies every row's ring of this column out.  bias == NULL: no tables (an index of -1 everywhere).  rep_host == NULL: ts_op_sample_bias
int ts_op_sample_repeat(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                        uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *given_rows_host,
                        const uint8_t *keep, const int64_t *given, uint8_t *kept, float *logits_copy, const float *bias, int n_bias,
                        const int32_t *bias_index_host, int column, const ts_repeat *rep_host, int n_rep, const int32_t *history,
                        int32_t *ring_out, void *stream) {
    OpSample a{rep_host ? "ts_op_sample_repeat" : "ts_op_sample_bias", (bias && !bias_index_host) || (!bias && !rep_host), 0, ctx, logits, B, V,
               mode, uniforms, seed, clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl;
    a.kept = kept, a.logprob = logprob, a.given_rows_host = given_rows_host, a.keep = keep, a.given = given, a.logits_copy = logits_copy;
    a.o.bias = bias, a.o.n_bias = n_bias, a.o.bias_index_host = bias_index_host, a.o.rep_host = rep_host, a.o.n_rep = n_rep;
    a.column = column, a.history = history, a.ring_out = ring_out;
    return op_sample(a);
}

// The same launch under "guidance" (kernel-level tests call it): guide_host (B,) the shadow's row of every row or -1, scale_host (B,).  A
// primary reads its shadow's logits row and writes idx, kept and logprob for both rows; a shadow's ring is not touched.  Every other
// argument as for ts_op_sample_repeat (rep_host == NULL: no records; bias == NULL: no tables).  guide_host == NULL is refused
int ts_op_sample_guide(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                       uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *given_rows_host,
                       const uint8_t *keep, const int64_t *given, uint8_t *kept, float *logits_copy, const float *bias, int n_bias,
                       const int32_t *bias_index_host, int column, const ts_repeat *rep_host, int n_rep, const int32_t *history,
                       int32_t *ring_out, const int32_t *guide_host, const float *scale_host, void *stream) {
    OpSample a{"ts_op_sample_guide", !guide_host || !scale_host || (bias && !bias_index_host), 0, ctx, logits, B, V, mode, uniforms, seed,
               clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl;
    a.kept = kept, a.logprob = logprob, a.given_rows_host = given_rows_host, a.keep = keep, a.given = given, a.logits_copy = logits_copy;
    a.o.bias = bias, a.o.n_bias = n_bias, a.o.bias_index_host = bias_index_host, a.o.rep_host = rep_host, a.o.n_rep = n_rep;
    a.o.guide_host = guide_host, a.o.guide_scale_host = scale_host;
    a.column = column, a.history = history, a.ring_out = ring_out;
    return op_sample(a);
}

// The same launch with "alternatives" (kernel-level tests call it): ts_op_sample_repeat's arguments, where rep_host and bias may both be NULL
// (records of window 0, an index of -1), then the record: codes / logprob (B,n), entropy / rank (B).  alt == NULL is refused
int ts_op_sample_alt(ts_ctx *ctx, const float *logits, int B, int V, int mode, const float *uniforms, uint64_t seed, int64_t clip_index0,
                     uint32_t position, const ts_sampling *ctl_host, int n_ctl, int64_t *idx, float *logprob, const int32_t *given_rows_host,
                     const uint8_t *keep, const int64_t *given, uint8_t *kept, float *logits_copy, const float *bias, int n_bias,
                     const int32_t *bias_index_host, int column, const ts_repeat *rep_host, int n_rep, const int32_t *history,
                     int32_t *ring_out, const ts_alt_out *alt, void *stream) {
    OpSample a{"ts_op_sample_alt", !alt || (bias && !bias_index_host), 0, ctx, logits, B, V, mode, uniforms, seed, clip_index0, position, idx, stream};
    a.o.ctl_host = ctl_host, a.o.n_ctl = n_ctl;
    a.kept = kept, a.logprob = logprob, a.given_rows_host = given_rows_host, a.keep = keep, a.given = given, a.logits_copy = logits_copy;
    a.o.bias = bias, a.o.n_bias = n_bias, a.o.bias_index_host = bias_index_host, a.o.rep_host = rep_host, a.o.n_rep = n_rep;
    a.o.alt = alt, a.o.logprob = logprob;
    a.column = column, a.history = history, a.ring_out = ring_out;
    return op_sample(a);
}

// Host only ("speaker style"): every weight of a style block is finite; the first bad index is named
int ts_style_check(const float *w_host, long n, int NC) {
    if (!w_host || n < 0 || NC < 1) return fail("ts_style_check: bad argument");
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(w_host[i]))
            return fail("ts_style_check: weight " + std::to_string(i) + " (row " + std::to_string(i / NC) + ", speaker " + std::to_string(i % NC) +
                        ") is not finite");
    return 0;
}

// style_rows_kernel on its own (kernel-level tests call it): tables (NL,NC,W), weights (M,NC) -> out (NL,M,W), row m from weight row m.
// Run as ONE clip slot with a track of M rows, so the kernel's row indexing is what is exercised
int ts_op_style_rows(ts_ctx *ctx, const float *tables, int NL, int NC, int W, const float *weights, int M, float *out, void *stream) {
    if (!ctx || !tables || !weights || !out) return fail("ts_op_style_rows: null argument");
    if (NL < 1 || NC < 1 || M < 1 || W < 4 || W % 4) return fail("ts_op_style_rows: bad shape (W is a positive multiple of 4)");
    hipStream_t s = (hipStream_t)stream;
    StyleRowsParams q;
    std::memset(&q, 0, sizeof(q));
    q.tables = tables;
    q.weights = weights;
    q.w_ld = NC;
    q.S = M, q.NC = NC, q.W = W, q.NL = NL;
    q.r0 = 0, q.n = M, q.slots = 1;
    q.out = out;
    q.out_l_stride = (long)M * W;
    q.out_r_stride = W;
    TS_HIP(launch_style_rows(q, s));
    TS_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
