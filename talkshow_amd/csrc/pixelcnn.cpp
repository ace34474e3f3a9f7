// GatedPixelCNN (nets/spg/gated_pixelcnn_v2.py) as an INCREMENTAL, row-cached launch plan.
//
// The reference's generate() (:152-177) re-runs the whole 15-layer network over the whole H x 2 grid for each of
// the 2H positions.  Causality (:57-87: layer 0 is mask 'A'; vertical kernels look up, horizontal kernels look left)
// means position (r, j) only needs
//   * the vertical stack at row r: layer 0 sees code rows r-3..r-1, layer l>=1 sees its own input at rows r-1, r;
//   * the horizontal stack at columns <= j of row r.
// So per row we run the vertical stack once for both columns, then the horizontal chain for column 0 (body code),
// sample, then column 1 (hand code), sample: 216x fewer FLOPs, every conv tap multiplied exactly once in fp32.
//
// Row-shifted partial sums (keeps every stage's K at <= 2*dim, i.e. its weight slice small and its MFMA burst short):
//   h_vert_l(r) = Wcur_l . XV_l[r] + ( Wprev_l . XV_l[r-1] + b )         the bracket is computed one row EARLIER, in the
//   h_vert_0(r) = W2 . E[r-1] + ( W1 . E[r-2] ) + ( W0 . E[r-3] ) + b     same launch that first sees XV_l[r-1] / E[..]
//
// Launch plan of row r (every entry is ONE skinny_gemm launch over all clips of the pass; "|" separates independent
// problems that share a launch):
//   V0        v0.gate | v0.Q1 | v0.Q0                     gate: OV0 = gate(W2.E[r-1] + Q1[r] + Q0[r] + b + c0)
//                                                         (rows r >= 1 of a pass that takes the code tables: ONE lookup launch, no GEMM;
//                                                         so is hg_0 of column 1 — see ts_pixelcnn::CodeTables)
//   V1        v1.gate | v1.P | v2h_0                      layer 1 reads OV0 directly: fusion_v[:, :D] (gated_pixelcnn_v2.py:137-144)
//                                                         is composed into its two tap matrices on the host, the audio half
//                                                         of the fusion becomes two per-row additive terms precomputed for
//                                                         all rows (XV_1 is never materialised)
//   V_l       v_l.gate | v_l.P | v2h_{l-1}                l = 2..NL-1
//   V_NL      v2h_{NL-1}
//   column j: hg_0, S_1 .. S_{NL-1}, head1', head2, sample
//
// Horizontal chain, one launch per layer.  In the reference a layer is gate(horiz_stack(x_h) + ...) followed by
// horiz_resid (+ x_h), i.e. two dependent linear maps per layer; consecutive linear maps are composed on the host
// (products in fp64, rounded once to fp32 — the same kind of fold as BatchNorm into a conv):
//   S_l   A: XH_l[j]  = Rw_l . G_{l-1} + rb_l + XH_{l-1}[j]                               (Rw_l = horiz_resid_{l-1};
//         B: G_l      = gate( (Wh1_l.Rw_l) . G_{l-1} + Wh1_l . XH_{l-1}[j] + bm_l          l = 1 also folds fusion_h)
//                             + V2H_l[j] + c_l  [+ Wh0_l . XH_l[0] for j = 1, precomputed while column 0 ran] )
//   head1'   relu( (W1.Wr_{NL-1}) . G_{NL-1} + W1 . XH_{NL-1}[j] + b )
// A and B only need (G_{l-1}, XH_{l-1}) so they share a launch: NL + 2 dependent launches per column instead of 2*NL + 3.
// The vertical stack of a row and the column-0 chain of the same row are independent except for V2H_l (ready after
// V_{l+1}); V_k rides in the launch of the column-0 stage that runs one step behind it: V0, V1, then (hg_0 | V2),
// (S_1 | V3), ... = 2 + (NL + 2) + (NL + 2) = 36 skinny launches per row for NL = 15, plus the 2 sampler launches
// (a per-op port would need 2 + 17 + 66).
//
// Rows are absolute indices: a one-shot call runs rows 0..H-1 (after an optional known prefix), a streaming session
// (ts_pixelcnn_stream_*) continues at the row where its previous step stopped, on a row cache that persists in its Work.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <deque>
#include <set>
#include <tuple>

#include "host_common.h"
#include "skinny_desc.h"

using namespace ts;

struct ts_pixelcnn {
    ts_ctx *ctx = nullptr;
    int V = 0, D = 0, NL = 0, NC = 0, AD = 0, HID = 512;
    DevBuf emb;                                              // [V][D]
    std::vector<std::vector<std::unique_ptr<DevBuf>>> wvt;   // vertical taps: layer 0 {W0,W1,W2}, l>=1 {Wprev,Wcur}; each [4D][2D]
    std::vector<std::unique_ptr<DevBuf>> bv;                 // [2*2D] (duplicated per column)
    std::vector<std::unique_ptr<DevBuf>> wv2h, bv2h, wh, bh, cls, wr, br;
    DevBuf fha;                                              // fusion_h[:, :D]  [D][D] (fusion_v's half lives composed in wv1c / wv1p)
    DevBuf wv1c, wv1p;                                       // layer 1 vertical taps with fusion_v[:, :D] composed in  [4D][2D]
    ConvLayer aud_v1c, aud_v1p;                              // the same taps applied to the audio half of the fusion   [4D][D]
    ConvLayer aud_embed, aud_fv, aud_fh;                     // embedding_aud ; fusion_{v,h}[:, D:] (+ fusion bias)
    DevBuf w1, b1, w2, b2;                                   // output_conv
    // composed horizontal maps (see the header): per layer l >= 1
    std::vector<std::unique_ptr<DevBuf>> rw, rb;             // A: Rw_l [D][D], rb_l [D]        (index l, entry 0 unused)
    std::vector<std::unique_ptr<DevBuf>> wB, bm;             // B: [2D][D or 2D], bm_l [2D]
    DevBuf w1m, b1m;                                         // head1': [HID][D or 2D], [HID]
    ConvLayer aud_h1;                                        // Wh1_1 applied to AEH for every row (l = 1 has AEH in place of XH_0)
    DevBuf cls_all;                                          // the NL class tables again, contiguous [NL][NC][2D]: what style_rows_kernel reads
    DevBuf bv_all;                                           // the NL vertical biases again, contiguous [NL][2*2D]: what slot_reset_kernel reads
    // Code tables (code_tables.hip).  Two launches of a code row multiply nothing but embeddings of codes that are already known: slot
    // V0 (W2 . E[r-1] and its riders W1 . E[r-1], W0 . E[r-1]) and hg_0 of column 1 (wh[0] . emb[code(r, 0)]).  The tables hold, per code,
    // the slice sums the chain kernels would form (same MFMA, same k order, same K split), so a lookup launch that adds them in the
    // kernels' order gives the kernels' bits without MFMAs, weight streams or whole-CU workgroups.  Built once per model from the weights
    // alone, shared by every stream.  V0: per matrix 1 + W / 2 row sets of [V][4D] (the prefix of column 0's slices; column 1's slices one
    // by one); hg_0: one row set of [V][2D].
    struct CodeTables {
        DevBuf v0[3];      // wvt[0][2] (the gate), wvt[0][1] (rider Q1), wvt[0][0] (rider Q0)
        DevBuf hg;
        int sets = 0;      // row sets of a V0 table
        bool built = false;
    } tables;
    int tables_mode = -1;  // TS_PIX_TABLES: -1 auto (see use_tables), 0 the GEMM launches, 1 every pass
    bool use_graph = true;
    int defer_p = -1;     // the next-row projections P_l of the vertical stack ride with column 1's launches: -1 auto, 0 never, 1 always
    // tiled operand layouts (kernels.h, SkinnyParams::w_tiled): every weight matrix of the chain gets a tiled twin, and
    // the activation buffers that feed the next stage's GEMM (OV0, XV, HV, G, XH, Y) are written / read tiled
    bool tiled = false;
    struct TiledW {
        DevBuf buf;
        int K = 0, epi = 0;
    };
    std::map<const float *, std::unique_ptr<TiledW>> wtiled;
    // Work set: every buffer the row loop touches + the hipGraph replays of it.  One per stream, so that independent
    // batches can be in flight on different streams against the single weight copy above.
    struct Work {
        int capB = 0, capH = 0;
        DevBuf aud_all, AE, AEV, AEH, AEH1, AV1C, AV1P, tok32, CR, XV, OV0, OVlast, HV, V2H, P, Q1, Q0, XH, G, T0, Y, LG, tfcodes;
        // every pointer inside the captured kernels is one of the buffers above or the staging buffers below, so a graph
        // is valid for any caller pointers; key = (B, H, H0, mode)
        DevBuf codes_int, unif_int, dyn;   // dyn: {seed, clip0, position base} of the call being replayed, written by a kernel ahead of it
        DevBuf cAEH, cAEH1, cAV1C, cAV1P;  // the audio terms of ONE chunk of rows, compact (chunked one-shot calls: see run_chunked)
        DevBuf clip_tab;                   // mixed passes: the Philox subsequence of every clip (int64), read by the captured samplers
        DevBuf ctl_tab;                    // passes with sampling controls: one SampleCtl per clip SLOT of the pass, written in stream order ahead of it
        DevBuf lp_int;                     // runs with a log-probability output: what the captured samplers write, (B,rows,2) fp32 beside codes_int
        DevBuf given_tab, given_int;       // passes with given rows: G of every clip SLOT (int32, written in stream order ahead of the pass); the given codes of
                                           // ONE chunk, (B,rows,2) int64 beside codes_int (what the captured samplers read); a session's holds max_chunk_rows rows
        DevBuf keep_int;                   // passes with a mask of kept positions: the mask bytes of ONE chunk, (B,rows,2) uint8 beside given_int
        DevBuf style_int;                  // passes with per-row speaker style: the class-conditioning rows of ONE chunk, [NL][CHUNK_ROWS][Bs][2D] fp32 (slabs Bs
                                           // clips apart, like CR); allocated by the first such pass, filled ahead of every chunk by style_rows_kernel
        DevBuf bias_tab, bias_idx;         // passes with a code bias: the tables (NB,2,V) fp32 and the table index of every clip SLOT (int32, -1: none), both
                                           // written in stream order ahead of the pass (what the captured samplers read).  bias_tab holds capB tables — a pass
                                           // brings at most one per clip — so it moves only when ensure_work has dropped the graphs that read it
        DevBuf rep_tab, rep_ring;          // passes with a repetition penalty: one SampleRep per clip SLOT, written in stream order ahead of the pass, and the
                                           // history rings [slot][2][64] int32 (the code of row r, column j at index r & 63) the sample_ctl_rep kernels read and
                                           // write.  Both are sized by capB in ensure_work, so they never move under a graph; the rings need no clearing: a launch
                                           // reads min(r, W) entries, all written earlier in the same pass by the same slot
        DevBuf guide_tab, guide_scl;       // passes with guidance: the role of every clip SLOT (int32: -1 plain, g >= 0 the shadow's slot, -2 a shadow) and
                                           // the scale of every primary (fp32), written in stream order ahead of the pass; sized by capB in ensure_work
        DevBuf alt_int;                    // passes with alternatives: what the captured samplers write, four blocks of capB * capH * 2 positions each —
                                           // codes [.][8] int32, log-probabilities [.][8] fp32, entropy fp32, rank int32 — laid out (B,rows,2,n) / (B,rows,2)
                                           // from the block's start; allocated by the first such pass, sized by the Work's capacity alone, so it moves only
                                           // when ensure_work has dropped the graphs that write it
        hipStream_t cap_stream = nullptr;
        // Captured graphs, least recently used out first: at most GRAPH_CAP per Work.  Keys: (B, H, H0, mode, 0) = a whole one-shot call;
        // (B, Hc, -(1 + phase), mode, 0) = Hc rows of a chunked one-shot call; (B, Hc, 1000 + phase, mode, 0) = a streaming step (in a session's own Work);
        // (Br, Hc, -(1 + phase), mode, Bs) = Hc rows of a MIXED pass of Bs clips for its first Br clips: the per-clip slabs of the work
        // buffers are Bs clips apart whatever Br is, so the stride is part of what a captured graph is valid for (0: the slabs are B apart).
        // The sixth field is a bit set: bit 0 for a run whose samplers read ctl_tab (sample_ctl_kernel), bit 1 for a run whose samplers write
        // log-probabilities into lp_int, bit 2 for a pass with given rows (EVERY chunk of such a pass runs the given variants of the samplers,
        // which read given_tab and given_int), bit 3 for a given pass that brings a mask of kept positions (every chunk's samplers then also
        // read keep_int; without the bit their mask pointer is null), bit 4 for a pass with per-row speaker style (the gate launches of every chunk
        // read their conditioning rows from style_int in place of CR), bit 5 for a pass with a code bias (its samplers are the sample_ctl_bias
        // kernels, which read bias_tab and bias_idx; neither the tables' content nor their number is part of the key), bit 6 for a pass with a repetition penalty (its samplers are the
        // sample_ctl_rep kernels, which read rep_tab and bias_idx and read and write rep_ring; the records are not part of the key), bit 7 for the steps of a
        // session that has restarted a slot (their samplers read the session's row_origin and the clip table; which slots restarted, and where, is not part of the key), bit 8 for a pass
        // with guidance (its samplers are the sample_ctl_guide kernels, which read guide_tab and guide_scl beside what the sample_ctl_rep kernels read; roles and scales are not part of the key), bit 9 for a pass with alternatives (its samplers are the sample_ctl_alt kernels, which write alt_int; n sits in the bits above, value n << 10); 0 otherwise: runs with none find exactly the graphs they found before the field existed; the
        // tables' CONTENT is not part of the key (a replay reads what the call wrote).
        // At most GRAPH_CAP unpinned graphs + PIN_CAP pinned ones per Work.
        typedef std::tuple<int, int, int, int, int, int> Key;
        struct Entry {
            hipGraphExec_t exec;
            uint64_t used;
        };
        static constexpr size_t GRAPH_CAP = 24;
        static constexpr size_t PIN_CAP = 12;                 // shapes a host may pin with ts_pixelcnn_prepare (they are never evicted)
        static constexpr size_t RECENT = 16;                  // window of one-shot calls a shape must recur in to count as hot
        std::map<Key, Entry> graphs;
        std::map<Key, std::pair<long, double>> graph_stats;   // skinny launches, flops
        std::set<Key> pinned;
        std::deque<Key> recent;                               // the last RECENT one-shot (H0 = 0) shapes that found no whole-call graph
        // graphs taken out of the cache while a replay of them may still be queued on the stream: destroyed once the event recorded
        // behind them has completed (no host-side wait on the serving stream)
        struct Retired {
            hipGraphExec_t exec;
            hipEvent_t done;
        };
        std::vector<Retired> retired;
        uint64_t tick = 0;
        long captures = 0;                                    // graphs captured + instantiated on this stream so far
        // A one-shot shape gets its own whole-call graph (~36 H nodes: tens of milliseconds to capture and instantiate) only when it is
        // HOT: pinned by the host, or met for the third time within the last RECENT one-shot calls on this stream.  A pass over a
        // dataset of many distinct lengths (scripts/test_body.py:113-194), however often it is repeated, never qualifies and keeps running
        // on the length-independent chunk graphs; a serving loop on one or a few shapes qualifies on its third call.
        bool hot(const Key &k) {
            if (pinned.count(k)) return true;
            int n = 0;
            for (const Key &r : recent) n += r == k;
            recent.push_back(k);
            if (recent.size() > RECENT) recent.pop_front();
            return n >= 2;
        }
        void reap(bool wait) {
            size_t keep = 0;
            for (size_t i = 0; i < retired.size(); ++i) {
                Retired &r = retired[i];
                if (wait) (void)hipEventSynchronize(r.done);
                if (wait || hipEventQuery(r.done) == hipSuccess) {
                    (void)hipGraphExecDestroy(r.exec);
                    (void)hipEventDestroy(r.done);
                } else {
                    retired[keep++] = r;
                }
            }
            retired.resize(keep);
        }
        void drop_graphs() {
            reap(true);
            for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second.exec);
            graphs.clear();
            graph_stats.clear();            // `pinned` stays: a pinned shape whose graph went with a buffer growth is re-captured by its next call
        }
        // Two classes share the cache: whole-call graphs of hot one-shot shapes (key field 2 = H0 in [0, 1000): at most WHOLE_CAP
        // unpinned ones) and the length-independent chunk / streaming-step graphs (at most GRAPH_CAP - WHOLE_CAP) — a burst of hot
        // shapes never pushes out the chunk graphs every other call falls back on.  Room for one more graph of `key`'s class: the least
        // recently used unpinned graph of that class leaves the cache; it is destroyed behind an event on `s`.
        static constexpr size_t WHOLE_CAP = 8;
        static bool whole(const Key &k) { return std::get<2>(k) >= 0 && std::get<2>(k) < 1000; }
        int make_room(hipStream_t s, const Key &key) {
            reap(false);
            const bool cls = whole(key);
            const size_t cap = cls ? WHOLE_CAP : GRAPH_CAP - WHOLE_CAP;
            for (;;) {
                size_t n = 0;
                auto lru = graphs.end();
                for (auto it = graphs.begin(); it != graphs.end(); ++it) {
                    if (whole(it->first) != cls || pinned.count(it->first)) continue;
                    ++n;
                    if (lru == graphs.end() || it->second.used < lru->second.used) lru = it;
                }
                if (n < cap) break;
                Retired r{lru->second.exec, nullptr};
                TS_HIP(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
                TS_HIP(hipEventRecord(r.done, s));
                retired.push_back(r);
                graph_stats.erase(lru->first);
                graphs.erase(lru);
            }
            if (retired.size() > 2 * GRAPH_CAP) reap(true);   // a host that never lets the stream drain: bounded all the same
            return 0;
        }
        ~Work() {
            drop_graphs();
            if (cap_stream) (void)hipStreamDestroy(cap_stream);
        }
    };
    StreamWorks<Work> works;
    Work &work(hipStream_t s) { return works.get(s); }
};

// f3: a generation session whose row cache (one previous row per layer + the layer-0 partial sums + the last code rows)
// persists across calls — O(1) state for any history length (the receptive field is 17 code rows)
struct ts_pixelcnn_stream {
    ts_pixelcnn *p = nullptr;
    int B = 0;
    long rows = 0;              // code rows generated so far = absolute index of the next row
    int max_rows = 0;           // largest chunk a step may bring (buffers are sized once, at open)
    ts_pixelcnn::Work w;
    DevBuf label;
    // "repetition penalty" on a session: per clip, the first row of its current unbroken run of rows written under window > 0 (what
    // SampleRep::from_row carries to the samplers), REP_NONE while the clip has no such run (a value no row takes: a loaded slot's run may
    // have begun below the session's row 0, "slot state")
    static constexpr int32_t REP_NONE = INT32_MIN;
    std::vector<int32_t> rep_from;
    int64_t last_clip0 = -1;           // clip_index0 of the latest step (-1: none yet): what a never-restarted slot b drew under, less b
    // "slot restart" (talkshow_hip.h): nothing below exists, on the host or the device, until the session's first restart
    bool restarted = false;            // steps bind row_origin and the clip table (sampler bit 7: graph keys of their own)
    bool cr_ready = false;             // CR was written from the labels ahead of a restart at row 0: the first step leaves it alone
    std::vector<int32_t> origin;       // per slot: the session row at which its current clip began
    std::vector<int64_t> clip_index;   // per slot: the Philox clip index given at its restart, -1 while it has never restarted
    DevBuf row_origin, restart_tab;    // (B,) int32 the samplers read; {slots (B,), labels (B,)} of the restart being queued
    // "slot state" (talkshow_hip.h): nothing below exists until the session's first save or load
    DevBuf state_tab;                  // three (B,) int32 tables of the save / load being queued (kernel arguments, in stream order)
    std::vector<int64_t> slot_label;   // per slot: the label a restart or a load brought, -1: the one given at open (the caller holds it)
    // "session pairs" (talkshow_hip.h): nothing below exists until the session's first pair, restart or load
    std::vector<int32_t> pair_of;      // per slot: its shadow's slot where it is a primary, else -1 (the table ts_guide_check takes)
    std::vector<float> pair_scale;     // per slot: the stored scale of a primary
    int n_pairs = 0;
    std::vector<int32_t> fresh;        // per slot: the serial of the restart or load that listed it at session row fresh_at, else 0
    long fresh_at = -1;
    int32_t serial = 0;
};

namespace {

int upload_vec(std::vector<std::unique_ptr<DevBuf>> &dst, const std::vector<float> &v) {
    dst.emplace_back(new DevBuf());
    return dst.back()->upload(v.data(), v.size() * sizeof(float));
}

// rows per graph of a chunked one-shot call: a multiple of 4 (the period of the row rings), so that every chunk after the first
// starts in the same buffer phase
constexpr int CHUNK_ROWS = 8;

int ensure_work(ts_pixelcnn *p, ts_pixelcnn::Work *w, int B, int Htot) {
    if (B <= w->capB && Htot <= w->capH) return 0;
    const int cb = std::max(B, w->capB), ch = std::max(Htot, w->capH);
    const size_t D = p->D, NL = p->NL, f = sizeof(float);
    const size_t cb16 = round_up(cb, 16);   // tiled buffers hold whole 16-row blocks
    TS_TRY(w->aud_all.ensure((size_t)cb * ch * p->AD * f));
    TS_TRY(w->AE.ensure((size_t)cb * ch * D * f));
    TS_TRY(w->AEV.ensure((size_t)cb * ch * D * f));
    TS_TRY(w->AEH.ensure((size_t)cb * ch * D * f));
    TS_TRY(w->tok32.ensure((size_t)cb * ch * 2 * sizeof(int)));
    TS_TRY(w->CR.ensure(NL * cb * 2 * D * f));
    TS_TRY(w->XV.ensure(NL * 2 * cb16 * 2 * D * f));
    TS_TRY(w->OV0.ensure(cb16 * 2 * D * f));
    TS_TRY(w->OVlast.ensure((size_t)cb * 2 * D * f));
    TS_TRY(w->HV.ensure(NL * cb16 * 4 * D * f));
    TS_TRY(w->V2H.ensure(NL * cb * 4 * D * f));
    TS_TRY(w->P.ensure(NL * 2 * cb * 4 * D * f));
    TS_TRY(w->Q1.ensure((size_t)4 * cb * 4 * D * f));
    TS_TRY(w->Q0.ensure((size_t)4 * cb * 4 * D * f));
    TS_TRY(w->XH.ensure((NL + 1) * 2 * cb16 * D * f));
    TS_TRY(w->G.ensure((size_t)2 * cb16 * D * f));
    TS_TRY(w->T0.ensure(NL * cb * 2 * D * f));
    TS_TRY(w->AEH1.ensure((size_t)cb * ch * 2 * D * f));
    TS_TRY(w->AV1C.ensure((size_t)cb * ch * 4 * D * f));
    TS_TRY(w->AV1P.ensure((size_t)cb * ch * 4 * D * f));
    TS_TRY(w->Y.ensure(cb16 * p->HID * f));
    TS_TRY(w->LG.ensure((size_t)cb * p->V * f));
    TS_TRY(w->tfcodes.ensure((size_t)cb * ch * 2 * sizeof(int64_t)));
    TS_TRY(w->codes_int.ensure((size_t)cb * ch * 2 * sizeof(int64_t)));
    TS_TRY(w->unif_int.ensure((size_t)cb * ch * 2 * sizeof(float)));
    TS_TRY(w->dyn.ensure(3 * sizeof(uint64_t)));
    TS_TRY(w->clip_tab.ensure((size_t)cb * sizeof(int64_t)));
    TS_TRY(w->ctl_tab.ensure((size_t)cb * sizeof(SampleCtl)));
    TS_TRY(w->lp_int.ensure((size_t)cb * ch * 2 * sizeof(float)));
    TS_TRY(w->given_tab.ensure((size_t)cb * sizeof(int)));
    TS_TRY(w->given_int.ensure((size_t)cb * CHUNK_ROWS * 2 * sizeof(int64_t)));
    TS_TRY(w->keep_int.ensure((size_t)cb * CHUNK_ROWS * 2));
    TS_TRY(w->bias_idx.ensure((size_t)cb * sizeof(int32_t)));
    TS_TRY(w->rep_tab.ensure((size_t)cb * sizeof(SampleRep)));
    TS_TRY(w->rep_ring.ensure((size_t)cb * 2 * SAMPLE_REP_RING * sizeof(int32_t)));
    TS_TRY(w->guide_tab.ensure((size_t)cb * sizeof(int32_t)));
    TS_TRY(w->guide_scl.ensure((size_t)cb * sizeof(float)));
    TS_TRY(w->cAEH.ensure((size_t)cb * CHUNK_ROWS * D * f));
    TS_TRY(w->cAEH1.ensure((size_t)cb * CHUNK_ROWS * 2 * D * f));
    TS_TRY(w->cAV1C.ensure((size_t)cb * CHUNK_ROWS * 4 * D * f));
    TS_TRY(w->cAV1P.ensure((size_t)cb * CHUNK_ROWS * 4 * D * f));
    w->drop_graphs();   // buffers moved: captured pointers are stale
    w->capB = cb;
    w->capH = ch;
    return 0;
}

// Rows are ABSOLUTE indices of the session / call.  One-shot call: rows 0..Htot-1, the first H0 of them a known prefix.
// Streaming step: rows r0..r0+Hc-1 behind a row cache left by the previous steps.
struct RunCfg {
    int B, H, H0, Htot, mode;
    const float *uniforms;
    uint64_t seed;
    int64_t clip0;
    int64_t *codes;        // (B,H,2)
    float *logits;         // (B,H,2,V) or null
    const uint64_t *dyn;   // device {seed, clip0} (graph replay) or null
    ts_pixelcnn::Work *w;
    int R;                 // rows of the token ring tok32[B][R][2]: row rr lives at rr % R (one-shot: R = Htot, no wrap)
    int aud_r0, aud_rows;  // the audio-term buffers AEV / AEH / AEH1 hold rows [aud_r0, aud_r0 + aud_rows)
    int out_r0;            // first row written to `codes` / `logits` / read from `uniforms` (those arrays hold H rows)
    int pos_r0;            // Philox position of row r, column j = pos_base + (r - pos_r0) * 2 + j
    long pos_base;         // (added on the device from a dynamic word when a captured graph is replayed)
    int last_row;          // rows >= last_row are never generated: look-ahead partial sums for them are skipped
    // where the audio terms of rows [aud_r0, aud_r0 + aud_rows) live (the Work's whole-call buffers unless a chunk brings its own)
    const float *aeh = nullptr, *aeh1 = nullptr, *av1c = nullptr, *av1p = nullptr;
    // the caller's codes / uniforms arrays hold out_H rows per clip, of which this run fills rows out_row0 .. out_row0 + H - 1
    int out_H = 0, out_row0 = 0;
    // mixed passes (run_mixed): B is the ACTIVE prefix of a pass of Bs clips.  Every per-clip slab of the work buffers is addressed with
    // Bs, so "the first B clips" is the same memory in every chunk of the pass (0: a uniform call, the slabs are B apart)
    int Bs = 0;
    const int64_t *clip_table = nullptr;   // device (Bs,) Philox subsequence per clip, in place of clip0 + b
    const SampleCtl *ctl = nullptr;        // device (slabB(),) sampling controls per clip slot (the Work's ctl_tab), or null: the sampler without controls
    float *logprob = nullptr;              // set by run_rows: (B,io_H,2) log-probabilities beside `codes` (staging or the caller's), or null
    int io_H = 0, io_row0 = 0;             // set by run_rows: row count / first row of the arrays the samplers address (staging or the caller's)
    // passes with given rows (run_mixed): the samplers are the given variants.  given_rows: device (slabB(),) G per clip slot (the Work's
    // given_tab); given_src: the caller's (B,out_H,2) block; given_stage: this run has rows below max G, so its rows of the block are staged
    // ahead of a replay; given: set by run_rows, laid out like `codes` (staging or the caller's)
    const int *given_rows = nullptr;
    const int64_t *given_src = nullptr, *given = nullptr;
    bool given_stage = false;
    // "kept positions": keep_src the caller's (B,out_H,2) uint8 mask beside given_src or null (every given position kept); staged with the
    // given codes; keep: set by run_rows, laid out like `given`
    const unsigned char *keep_src = nullptr, *keep = nullptr;
    // "speaker style" with per-row tracks: the Work's style_int, which holds the conditioning rows of code rows [style_r0, style_r0 +
    // CHUNK_ROWS) as [NL][CHUNK_ROWS][slabB()][2D]; null: one conditioning row per clip for the whole call (the Work's CR)
    const float *style = nullptr;
    int style_r0 = 0;
    // "code bias": the Work's bias_tab (NB,2,V) and bias_idx (slabB(),), or null: the samplers without tables.  With tables c.ctl is set too
    // (neutral records when the call brought none)
    const float *bias = nullptr;
    const int32_t *bias_index = nullptr;
    // "repetition penalty": the Work's rep_tab (slabB(),) and rep_ring [slabB()][2][64], or null: the samplers without records.  With
    // records c.ctl and c.bias_index are set too (neutral records / an index of -1 when the call brought none)
    const SampleRep *rep = nullptr;
    int32_t *rep_ring = nullptr;
    // "guidance": the Work's guide_tab and guide_scl (slabB(),), or null: the samplers without a role table.  With them c.ctl, c.bias_index,
    // c.rep and c.rep_ring are set too (neutral records, an index of -1, records of window 0 when the call brought none)
    const int32_t *guide_role = nullptr;
    const float *guide_scale = nullptr;
    // "alternatives": the caller's record, or null: the samplers without them.  With it c.ctl, c.bias_index, c.rep and c.rep_ring are set too
    // (neutral records, an index of -1, records of window 0 when the call brought none).  alt: set by run_rows, the arrays the samplers
    // address, laid out like `codes` (staging or the caller's)
    const ts_alt_out *alt_src = nullptr;
    ts_alt_out alt = {};
    // "slot restart": the session's (slabB(),) table of the row at which every slot's current clip began, or null (a session that never
    // restarted a slot, and every one-shot call).  With it c.clip_table is set too
    const int32_t *row_origin = nullptr;
    // the class-conditioning rows of layer l for the gate launches of code row r (every such launch belongs to one row)
    const float *cls_rows(int l, int r, size_t D2) const {
        if (!style) return w->CR.f() + (size_t)l * slabB() * D2;
        return style + ((size_t)l * CHUNK_ROWS + (size_t)(r - style_r0)) * slabB() * D2;
    }
    int slabB() const { return Bs > 0 ? Bs : B; }
    void audio_from(ts_pixelcnn::Work *wk) { aeh = wk->AEH.f(), aeh1 = wk->AEH1.f(), av1c = wk->AV1C.f(), av1p = wk->AV1P.f(); }
};
inline RunCfg one_shot_cfg(int B, int H, int H0, int mode, const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes,
                           float *logits, ts_pixelcnn::Work *w) {
    const int Htot = H0 + H;
    // Philox position of code (r, j) = 2 r + j with r counted from the first PREFIX row: a call that continues another one
    // behind its codes (`infer(chunk1, pre_latents=chunk0 codes)`) draws the next numbers of the stream, not chunk 0's again
    RunCfg c{B, H, H0, Htot, mode, uniforms, seed, clip0, codes, logits, nullptr, w, Htot, 0, Htot, H0, 0, 0, Htot};
    c.audio_from(w);
    return c;
}

SkinnyParams base_params(int M, int N, int epi) {
    SkinnyParams q;
    std::memset(&q, 0, sizeof(q));
    q.M = M;
    q.N = N;
    q.epi = epi;
    return q;
}
void add_dense(SkinnyParams &q, const float *base, long stride, int shift, int len) {
    SkinnySeg &s = q.seg[q.nseg++];
    s.base = base;
    s.gidx = nullptr;
    s.row_stride = stride;
    s.gidx_stride = 0;
    s.row_shift = shift;
    s.len = len;
    q.Ktot += len;
}
void add_gather(SkinnyParams &q, const float *table, long stride, const int *gidx, long gstride, int len) {
    SkinnySeg &s = q.seg[q.nseg++];
    s.base = table;
    s.gidx = gidx;
    s.row_stride = stride;
    s.gidx_stride = gstride;
    s.row_shift = 0;
    s.len = len;
    q.Ktot += len;
}

// Stage tags (talkshow_hip_debug.h, ts_debug_pixelcnn_taps): what a problem's `out` is, as (stage, unit of the stage).  A gate's `pre` is
// HV of the same unit.  Only a tapped pass reads them.
enum PixStage { PS_HV, PS_OV, PS_P, PS_Q1, PS_Q0, PS_V2H, PS_G, PS_XH, PS_T0, PS_Y, PS_LG, PS_N };
static_assert(PS_N == TS_DEBUG_PIX_TAP_STAGES, "the stage list of talkshow_hip_debug.h");
inline int ptag(int stage, int unit) { return ((stage + 1) << 8) | unit; }

struct Slot {   // one launch: up to SKINNY_MAX_PROBLEMS independent problems
    SkinnyParams p[SKINNY_MAX_PROBLEMS];
    int tag[SKINNY_MAX_PROBLEMS];   // ptag of every problem, 0: not a tapped stage
    int n = 0;
    void add(const SkinnyParams &q, int t = 0) { tag[n] = t, p[n++] = q; }
    bool table = false;   // the slot is a code-table lookup (ts_pixelcnn::CodeTables): `ts` is launched, there are no problems
    CodeTableStage ts;
    int ttag = 0;         // ptag of the lookup's `out` (its `pre` is HV of the same unit, its riders are Q1 / Q0)
};

// Stage taps: a table this thread set waits (`pending`) for the next chain entry; that entry's PixTapScope makes it `active` for its own
// duration and drops it on the way out.  A pass without a table pays one thread-local load per launch and issues nothing.
struct PixTapState {
    ts_debug_pix_tap_table t;
    bool pending = false, active = false;
    int depth = 0;
};
thread_local PixTapState g_ptaps;
struct PixTapScope {
    PixTapScope() {
        if (g_ptaps.depth++ == 0 && g_ptaps.pending) g_ptaps.active = true, g_ptaps.pending = false;
    }
    ~PixTapScope() {
        if (--g_ptaps.depth == 0) g_ptaps.active = false;
    }
};
inline bool tapping() { return g_ptaps.active; }

// ---- code tables (the host arithmetic is in kernels.h: code_table_plan and the rules beside it) ----
bool use_tables(const ts_pixelcnn *p, int B) { return code_table_pass(p->tables.built, p->tables_mode, B); }

int build_code_tables(ts_pixelcnn *p) {
    if (p->tables.built) return 0;
    const CodeTablePlan t = code_table_plan(p->V, p->D, ts::knobs());
    if (!t.fits) return 0;
    const int V = p->V, D = p->D;
    const size_t set = (size_t)V * 4 * D;
    for (int m = 0; m < 3; ++m) {
        TS_TRY(p->tables.v0[m].ensure(t.sets_v0 * set * sizeof(float)));
        for (int st = 0; st < t.sets_v0; ++st) {   // set 0: column 0's slices summed; set 1 + i: slice W / 2 + i of column 1 alone
            CodeTableBuild b;
            b.W = p->wvt[0][2 - m]->f();
            b.ldw = 2 * D;
            b.N = 4 * D, b.K = 2 * D, b.waves = t.waves_v0;
            b.s0 = st == 0 ? 0 : t.waves_v0 / 2 + st - 1;
            b.s1 = st == 0 ? t.waves_v0 / 2 : b.s0 + 1;
            b.emb = p->emb.f();
            b.D = D, b.V = V, b.kcol = st == 0 ? 0 : D;
            b.out = p->tables.v0[m].f() + st * set;
            TS_HIP(launch_code_table_build(b, nullptr));
        }
    }
    TS_TRY(p->tables.hg.ensure(t.bytes_hg));
    CodeTableBuild b;
    b.W = p->wh[0]->f();      // tap 0 block: the first D columns of [2D][2D]
    b.ldw = 2 * D;
    b.N = 2 * D, b.K = D, b.waves = t.waves_hg, b.s0 = 0, b.s1 = t.waves_hg;
    b.emb = p->emb.f();
    b.D = D, b.V = V, b.kcol = 0;
    b.out = p->tables.hg.f();
    TS_HIP(launch_code_table_build(b, nullptr));
    TS_HIP(hipStreamSynchronize(nullptr));   // the chain's streams do not wait for the null stream
    p->tables.sets = t.sets_v0;
    p->tables.built = true;
    return 0;
}
inline int tiled_log2(int w) {
    int l = 0;
    while ((1 << l) < w) ++l;
    return w > 0 ? l : 0;
}

// the tiled view width of the work buffer that holds `ptr`, or 0 (row-major buffers / foreign pointers)
int tiled_width_of(const ts_pixelcnn *p, const ts_pixelcnn::Work *w, const void *ptr) {
    if (!p->tiled || !ptr) return 0;
    auto in = [&](const DevBuf &b) { return ptr >= b.p && ptr < static_cast<const char *>(b.p) + b.bytes; };
    if (in(w->OV0) || in(w->XV) || in(w->HV)) return 2 * p->D;     // HV is [B][4D], read by v2h as [2B][2D]
    if (in(w->G) || in(w->XH)) return p->D;
    if (in(w->Y)) return p->HID;
    return 0;
}

int launch_slot(ts_pixelcnn *p, ts_pixelcnn::Work *w, const Slot &a, const Slot *b, hipStream_t s) {
    // workgroups are dispatched in problem order: the rider (vertical stack: the big K = 512 problems) goes first, so that
    // whatever does not fit the first round of workgroups is the cheap end of the launch
    SkinnyParams q[SKINNY_MAX_PROBLEMS];
    const SkinnyParams *ps[SKINNY_MAX_PROBLEMS];
    int n = 0;
    if (a.table) {   // a lookup launch: no GEMM, so not a skinny launch of the statistics; a rider (none today) would follow as its own launch
        MiscScope ms(p->ctx, s);
        TS_HIP(launch_code_table_stage(a.ts, s));
        if (!b || b->n == 0) return 0;
    }
    if (b)
        for (int i = 0; i < b->n; ++i) q[n++] = b->p[i];
    for (int i = a.n - 1; i >= 0; --i) q[n++] = a.p[i];
    for (int i = 0; i < n; ++i) {
        if (p->tiled) {   // operands by identity: tiled weight twin, tiled activation buffers (see ts_pixelcnn::tiled)
            auto it = p->wtiled.find(q[i].W);
            if (it != p->wtiled.end() && it->second->K == q[i].Ktot && it->second->epi == q[i].epi) {
                q[i].W = it->second->buf.f();
                q[i].w_tiled = q[i].Ktot / 16;
            }
            for (int k = 0; k < q[i].nseg; ++k)
                if (!q[i].seg[k].gidx) q[i].seg[k].tiled_w = tiled_width_of(p, w, q[i].seg[k].base);
            q[i].out_tiled_w = tiled_width_of(p, w, q[i].out);
            q[i].pre_tiled_w = tiled_width_of(p, w, q[i].pre);
            q[i].add1_tiled_w = tiled_width_of(p, w, q[i].add1);
        }
        ps[i] = &q[i];
    }
    // A launch splits K over ONE wave count for all its problems, taken from its largest K (skinny_waves16, the 16-column plans' rule),
    // and a problem's bits depend on that split.  Which problems share a launch depends on how the pass is run (a deferred P_l rides with
    // column 1 or not, the last row has no P_l, a prefix row has no horizontal slot), so a problem must get the split of its OWN K
    // whatever rides along — the split the code tables were built with, too.  Networks with D < 128 (every K < 256 but head2's) and
    // D >= 256 (every K >= 256) never mix; in between (K = D < 256 <= 2D) a mixed launch goes out as two.  Zero-row segments multiply
    // nothing: a problem made of them alone has the same bits under any split and stays where it is.  This holds for the 16-column plans
    // (wide, fast, generic 16-column); a launch that falls to the generic 32-column kernel (shapes of odd models) splits by another rule
    // (plan_skinny) and is outside the bit contract, as it always was.
    auto waves_of = [](const SkinnyParams &x) {
        int k = 0;
        for (int i = 0; i < x.nseg; ++i)
            if (x.seg[i].base || x.seg[i].gidx) k += x.seg[i].len;
        return k == 0 ? 0 : skinny_waves16(k);
    };
    int n4 = 0, n8 = 0;
    for (int i = 0; i < n; ++i) n4 += waves_of(q[i]) == 4, n8 += waves_of(q[i]) == 8;
    if (n4 == 0 || n8 == 0) return run_skinny_batch(p->ctx, ps, n, s);
    const SkinnyParams *part[SKINNY_MAX_PROBLEMS];
    for (int pass = 0; pass < 2; ++pass) {
        int m = 0;
        for (int i = 0; i < n; ++i)
            if ((waves_of(q[i]) == 4) == (pass == 1)) part[m++] = &q[i];
        TS_TRY(run_skinny_batch(p->ctx, part, m, s));
    }
    return 0;
}

// one raw slab of a tapped stage -> its place in the caller's buffer (layout: talkshow_hip_debug.h)
int tap_copy(ts_pixelcnn *p, ts_pixelcnn::Work *w, int r, int tag, const float *src, long M, long stride, hipStream_t s) {
    const ts_debug_pix_tap_table &t = g_ptaps.t;
    const int stage = (tag >> 8) - 1, unit = tag & 255;
    if (tag <= 0 || stage >= PS_N || !src || !t.stage[stage]) return 0;
    const int D = p->D, NL = p->NL;
    const int units[PS_N] = {NL, NL, NL, 1, 1, NL, 2 * NL, 2 * NL, NL, 2, 2};
    const int width[PS_N] = {4 * D, 2 * D, 4 * D, 4 * D, 4 * D, 4 * D, D, D, 2 * D, p->HID, p->V};
    const size_t slab = (size_t)round_up(t.slab_clips, 16) * width[stage];
    const int tw = tiled_width_of(p, w, src);
    const size_t n = tw ? (size_t)round_up((int)((M * stride + tw - 1) / tw), 16) * tw : (size_t)(M * stride);
    if (unit >= units[stage] || n > slab) return fail("pixelcnn taps: a stage does not fit the slab the table names");
    float *dst = t.stage[stage] + ((size_t)(r - t.row0) * units[stage] + unit) * slab;
    MiscScope ms(p->ctx, s);
    TS_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
int tap_slot(ts_pixelcnn *p, ts_pixelcnn::Work *w, int r, const Slot &a, hipStream_t s) {
    if (a.table) {
        const int unit = a.ttag & 255;
        TS_TRY(tap_copy(p, w, r, a.ttag, a.ts.out, a.ts.M, a.ts.out_stride, s));
        TS_TRY(tap_copy(p, w, r, ptag(PS_HV, unit), a.ts.pre, a.ts.M, a.ts.pre_stride, s));
        TS_TRY(tap_copy(p, w, r, ptag(PS_Q1, 0), a.ts.rider[0], a.ts.M, a.ts.rider_stride, s));
        TS_TRY(tap_copy(p, w, r, ptag(PS_Q0, 0), a.ts.rider[1], a.ts.M, a.ts.rider_stride, s));
    }
    for (int i = 0; i < a.n; ++i) {
        TS_TRY(tap_copy(p, w, r, a.tag[i], a.p[i].out, a.p[i].M, a.p[i].out_stride, s));
        if (a.p[i].epi == EPI_GATE) TS_TRY(tap_copy(p, w, r, ptag(PS_HV, a.tag[i] & 255), a.p[i].pre, a.p[i].M, a.p[i].pre_stride, s));
    }
    return 0;
}
// launch_slot of code row r; a tapped pass copies out what the launch wrote, on the same stream right behind it
int launch_row_slot(ts_pixelcnn *p, const RunCfg &c, int r, const Slot &a, const Slot *b, hipStream_t s) {
    TS_TRY(launch_slot(p, c.w, a, b, s));
    if (!tapping()) return 0;
    const ts_debug_pix_tap_table &t = g_ptaps.t;
    if ((t.row >= 0 && t.row != r) || r < t.row0 || r >= t.row0 + t.rows) return 0;
    if (c.B > t.slab_clips) return fail("pixelcnn taps: the pass has more clips than the table's slab_clips");
    TS_TRY(tap_slot(p, c.w, r, a, s));
    if (b) TS_TRY(tap_slot(p, c.w, r, *b, s));
    return 0;
}

// vertical stack + v->h projections of row r as NL+2 launch slots
// `deferred` (optional): the P_l problems (only read by row r+1) are handed back instead of riding in slot V_l
void build_vertical(ts_pixelcnn *p, const RunCfg &c, int r, std::vector<Slot> &out, std::vector<SkinnyParams> *deferred = nullptr) {
    const int B = c.B, D = p->D, NL = p->NL, R = c.R;
    const size_t Bs = c.slabB();         // clips between the per-layer / per-row slabs of a buffer (>= B: see RunCfg::Bs)
    ts_pixelcnn::Work *w = c.w;
    const int *tok = w->tok32.i();
    const size_t Bp = round_up((int)Bs, 16);   // slices of the tiled buffers are whole 16-row blocks apart
    auto XV = [&](int l, int par) { return w->XV.f() + ((size_t)(l * 2 + par) * Bp) * 2 * D; };
    auto HV = [&](int l) { return w->HV.f() + (size_t)l * Bp * 4 * D; };
    auto V2H = [&](int l) { return w->V2H.f() + (size_t)l * Bs * 4 * D; };
    auto P = [&](int l, int par) { return w->P.f() + ((size_t)(l * 2 + par) * Bs) * 4 * D; };
    auto Q = [&](DevBuf &q, int row) { return q.f() + (size_t)(row & 3) * Bs * 4 * D; };
    auto CR = [&](int l) { return c.cls_rows(l, r, 2 * (size_t)D); };

    auto gate_common = [&](SkinnyParams &q, int l) {
        q.ldw = 2 * D;
        q.clsrow = CR(l);
        q.cls_ld = 2 * D;
        q.gateD = D;
        q.out = l == 0 ? w->OV0.f() : (l + 1 < NL ? XV(l + 1, r & 1) : w->OVlast.f());
        q.out_stride = 2 * D;
        q.pre = HV(l);
        q.pre_stride = 4 * D;
    };
    auto emb_row = [&](SkinnyParams &q, int rr) {   // embeddings of both codes of row rr >= 0
        for (int col = 0; col < 2; ++col) add_gather(q, p->emb.f(), D, tok + (size_t)(rr % R) * 2 + col, (long)R * 2, D);
    };
    auto make_v2h = [&](int l) {   // vert_to_horiz on the pre-gate activations, both columns
        SkinnyParams v = base_params(2 * B, 2 * D, EPI_LINEAR);
        add_dense(v, HV(l), 2 * D, 0, 2 * D);
        v.W = p->wv2h[l]->f();
        v.ldw = 2 * D;
        v.bias = p->bv2h[l]->f();
        v.out = V2H(l);
        v.out_stride = 2 * D;
        return v;
    };
    auto add_v2h = [&](Slot &s, int l) { s.add(make_v2h(l), ptag(PS_V2H, l)); };

    out.clear();
    {   // V0: layer 0 (mask 'A', kernel rows 0..2 <-> code rows r-3..r-1): newest row here, older rows via Q1 / Q0.
        // Rows above the grid contribute nothing: their terms are simply left out (no zero-filled buffers to rely on).
        Slot s;
        SkinnyParams g = base_params(B, 4 * D, EPI_GATE);
        if (r >= 1) emb_row(g, r - 1);
        else add_dense(g, nullptr, 0, 0, std::min(128, 2 * D));   // top row: bias + conditioning only (a zero segment keeps it on the descriptor kernel)
        g.W = p->wvt[0][2]->f();
        g.bias = p->bv[0]->f();
        if (r >= 2) {
            g.add1 = Q(w->Q1, r);      // W1 . E[r-2], computed by the launch of row r-1
            g.add1_stride = 4 * D;
        }
        if (r >= 3) {
            g.add2 = Q(w->Q0, r);      // W0 . E[r-3], computed by the launch of row r-2
            g.add2_stride = 4 * D;
        }
        gate_common(g, 0);
        if (code_table_v0_row(r) && use_tables(p, B)) {   // the same sums from the code tables: one lookup launch for the gate and both riders
            CodeTableStage &ts = s.ts;
            std::memset(&ts, 0, sizeof(ts));
            for (int m = 0; m < 3; ++m) ts.tab[m] = p->tables.v0[m].f();
            ts.set_stride = (long)p->V * 4 * D;
            ts.nsets = p->tables.sets;
            ts.M = B, ts.N = 4 * D, ts.gateD = D;
            ts.tok0 = tok + (size_t)((r - 1) % R) * 2;   // exactly where emb_row's gather reads the two codes of row r-1
            ts.tok1 = ts.tok0 + 1;
            ts.tok_stride = (long)R * 2;
            ts.bias = g.bias;
            ts.add1 = g.add1, ts.add1_stride = g.add1_stride;
            ts.add2 = g.add2, ts.add2_stride = g.add2_stride;
            ts.cls = g.clsrow, ts.cls_ld = g.cls_ld;
            ts.pre = g.pre, ts.pre_stride = g.pre_stride, ts.pre_tw = tiled_log2(tiled_width_of(p, w, g.pre));
            ts.out = g.out, ts.out_stride = g.out_stride, ts.out_tw = tiled_log2(tiled_width_of(p, w, g.out));
            for (int t = 1; t >= 0; --t)
                if (code_table_rider(r, t, c.last_row)) ts.rider[1 - t] = Q(t == 1 ? w->Q1 : w->Q0, r + (2 - t));
            ts.rider_stride = 4 * D;
            s.table = true;
            s.ttag = ptag(PS_OV, 0);
        } else {
            s.add(g, ptag(PS_OV, 0));
        }
        for (int t = 1; t >= 0 && r >= 1 && !s.table; --t) {   // row r-1's codes as seen from row r+1 (kernel row 1) and r+2 (kernel row 0)
            const int target = r + (2 - t);
            if (target >= c.last_row) continue;
            SkinnyParams q = base_params(B, 4 * D, EPI_LINEAR);
            emb_row(q, r - 1);
            q.W = p->wvt[0][t]->f();
            q.ldw = 2 * D;
            q.out = Q(t == 1 ? w->Q1 : w->Q0, target);
            q.out_stride = 4 * D;
            s.add(q, ptag(t == 1 ? PS_Q1 : PS_Q0, 0));
        }
        out.push_back(s);
    }
    if (NL == 1) {
        Slot s;
        add_v2h(s, 0);
        out.push_back(s);
        return;
    }
    for (int l = 1; l < NL; ++l) {   // V_l: v_l.gate | v_l.P | v2h_{l-1}
        Slot s;
        // layer 1 reads the gate output of layer 0 through the composed taps (audio fusion folded in), l >= 2 its own input row
        const float *xin = l == 1 ? w->OV0.f() : XV(l, r & 1);
        const size_t arow = (size_t)(r - c.aud_r0) * 4 * D;
        const long astride = (long)c.aud_rows * 4 * D;
        SkinnyParams g = base_params(B, 4 * D, EPI_GATE);
        add_dense(g, xin, 2 * D, 0, 2 * D);
        g.W = l == 1 ? p->wv1c.f() : p->wvt[l][1]->f();
        if (r > 0) {
            g.add1 = P(l, r & 1);          // Wprev . XV_l[r-1] + bias, computed while row r-1 ran
            g.add1_stride = 4 * D;
        } else {
            g.bias = p->bv[l]->f();        // nothing above the first row
        }
        if (l == 1) {
            g.add2 = c.av1c + arow;        // Wcur_1 . [AEV[r] | AEV[r]]
            g.add2_stride = astride;
        }
        gate_common(g, l);
        s.add(g, ptag(PS_OV, l));
        if (r + 1 < c.last_row) {
            SkinnyParams q = base_params(B, 4 * D, EPI_LINEAR);
            add_dense(q, xin, 2 * D, 0, 2 * D);
            q.W = l == 1 ? p->wv1p.f() : p->wvt[l][0]->f();
            q.ldw = 2 * D;
            q.bias = p->bv[l]->f();
            if (l == 1) {
                q.add1 = c.av1p + arow;        // Wprev_1 . [AEV[r] | AEV[r]]
                q.add1_stride = astride;
            }
            q.out = P(l, (r + 1) & 1);
            q.out_stride = 4 * D;
            if (deferred) deferred->push_back(q);   // (run_row tags them: entry i is P of layer i + 1)
            else s.add(q, ptag(PS_P, l));
        }
        add_v2h(s, l - 1);
        out.push_back(s);
    }
    {
        Slot s;
        add_v2h(s, NL - 1);
        out.push_back(s);
    }
}

// horizontal chain + head of position (r, j): NL + 2 launch slots (the sampler launch follows separately)
void build_horizontal(ts_pixelcnn *p, const RunCfg &c, int r, int j, std::vector<Slot> &out) {
    const int B = c.B, D = p->D, NL = p->NL, R = c.R;
    const size_t Bs = c.slabB();
    ts_pixelcnn::Work *w = c.w;
    const int *tok = w->tok32.i();
    auto V2H = [&](int l) { return w->V2H.f() + (size_t)l * Bs * 4 * D + (size_t)j * 2 * D; };
    const size_t Bp = round_up((int)Bs, 16);
    auto XH = [&](int l, int col) { return w->XH.f() + ((size_t)(l * 2 + col) * Bp) * D; };
    auto CR = [&](int l) { return c.cls_rows(l, r, 2 * (size_t)D); };
    auto G = [&](int l) { return w->G.f() + (size_t)(l & 1) * Bp * D; };
    auto T0 = [&](int l) { return w->T0.f() + (size_t)l * Bs * 2 * D; };
    auto make_t0 = [&](int l) {   // column 0 only: Wh0_l . XH_l[0], consumed by column 1's S_l
        SkinnyParams t = base_params(B, 2 * D, EPI_LINEAR);
        add_dense(t, XH(l, 0), D, 0, D);
        t.W = p->wh[l]->f();      // tap 0 block
        t.ldw = 2 * D;
        t.out = T0(l);
        t.out_stride = 2 * D;
        return t;
    };
    out.clear();
    {   // hg_0 — mask 'A': only the column to the left, i.e. the embedding of the code just sampled
        Slot s;
        SkinnyParams q = base_params(B, 2 * D, EPI_GATE);
        if (j == 1) add_gather(q, p->emb.f(), D, tok + (size_t)(r % R) * 2 + 0, (long)R * 2, D);
        else add_dense(q, nullptr, 0, 0, std::min(128, 2 * D));   // column 0 has nothing to its left: a block of zero rows keeps the launch on
                                                 // the descriptor kernel (K = 0 would drop the whole launch to the generic one)
        q.W = p->wh[0]->f();
        q.ldw = 2 * D;
        q.bias = p->bh[0]->f();
        q.add1 = V2H(0);
        q.add1_stride = 4 * D;
        q.clsrow = CR(0);
        q.cls_ld = 2 * D;
        q.gateD = D;
        q.out = G(0);
        q.out_stride = D;
        if (code_table_hg_col(j) && use_tables(p, B)) {   // the code just sampled: its row of the hg_0 table in place of the GEMM
            CodeTableStage &ts = s.ts;
            std::memset(&ts, 0, sizeof(ts));
            ts.tab[0] = p->tables.hg.f();
            ts.set_stride = (long)p->V * 2 * D;
            ts.nsets = 1;
            ts.M = B, ts.N = 2 * D, ts.gateD = D;
            ts.tok0 = tok + (size_t)(r % R) * 2 + 0;
            ts.tok_stride = (long)R * 2;
            ts.bias = q.bias;
            ts.add1 = q.add1, ts.add1_stride = q.add1_stride;
            ts.cls = q.clsrow, ts.cls_ld = q.cls_ld;
            ts.out = q.out, ts.out_stride = q.out_stride, ts.out_tw = tiled_log2(tiled_width_of(p, w, q.out));
            s.table = true;
            s.ttag = ptag(PS_G, j);
        } else {
            s.add(q, ptag(PS_G, j));
        }
        out.push_back(s);
    }
    for (int l = 1; l < NL; ++l) {   // S_l
        Slot s;
        SkinnyParams a = base_params(B, D, EPI_LINEAR);
        add_dense(a, G(l - 1), D, 0, D);
        a.W = p->rw[l]->f();
        a.ldw = D;
        a.bias = p->rb[l]->f();
        if (l == 1) {
            a.add1 = c.aeh + (size_t)(r - c.aud_r0) * D;
            a.add1_stride = (long)c.aud_rows * D;
        } else {
            a.add1 = XH(l - 1, j);
            a.add1_stride = D;
        }
        a.out = XH(l, j);
        a.out_stride = D;
        s.add(a, ptag(PS_XH, 2 * l + j));

        SkinnyParams g = base_params(B, 2 * D, EPI_GATE);
        add_dense(g, G(l - 1), D, 0, D);
        if (l >= 2) add_dense(g, XH(l - 1, j), D, 0, D);
        g.W = p->wB[l]->f();
        g.ldw = g.Ktot;
        g.bias = p->bm[l]->f();
        g.add1 = V2H(l);
        g.add1_stride = 4 * D;
        if (l == 1) {
            g.add2 = c.aeh1 + (size_t)(r - c.aud_r0) * 2 * D;
            g.add2_stride = (long)c.aud_rows * 2 * D;
        }
        if (j == 1) {
            g.add3 = T0(l);
            g.add3_stride = 2 * D;
        }
        g.clsrow = CR(l);
        g.cls_ld = 2 * D;
        g.gateD = D;
        g.out = G(l);
        g.out_stride = D;
        s.add(g, ptag(PS_G, 2 * l + j));
        if (j == 0 && l >= 2) s.add(make_t0(l - 1), ptag(PS_T0, l - 1));
        out.push_back(s);
    }
    {   // head1' = relu(output_conv.0(XH_NL)) with XH_NL = horiz_resid_{NL-1}(G_{NL-1}) + XH_{NL-1} composed in
        Slot s;
        SkinnyParams h1 = base_params(B, p->HID, EPI_LINEAR);
        add_dense(h1, G(NL - 1), D, 0, D);
        if (NL >= 2) add_dense(h1, XH(NL - 1, j), D, 0, D);
        h1.W = p->w1m.f();
        h1.ldw = h1.Ktot;
        h1.bias = p->b1m.f();
        h1.relu = 1;
        h1.out = w->Y.f();
        h1.out_stride = p->HID;
        s.add(h1, ptag(PS_Y, j));
        if (j == 0 && NL >= 2) s.add(make_t0(NL - 1), ptag(PS_T0, NL - 1));
        out.push_back(s);
    }
    {
        Slot s;
        SkinnyParams h2 = base_params(B, p->V, EPI_LINEAR);
        add_dense(h2, w->Y.f(), p->HID, 0, p->HID);
        h2.W = p->w2.f();
        h2.ldw = p->HID;
        h2.bias = p->b2.f();
        h2.out = w->LG.f();
        h2.out_stride = p->V;
        s.add(h2, ptag(PS_LG, j));
        out.push_back(s);
    }
}

int launch_sampler(ts_pixelcnn *p, const RunCfg &c, int r, int j, hipStream_t s) {
    ts_pixelcnn::Work *w = c.w;
    SampleParams sp;
    std::memset(&sp, 0, sizeof(sp));
    const int ro = r - c.out_r0 + c.io_row0;     // row in the (B,sH,2) arrays the samplers address
    const int sH = c.io_H > 0 ? c.io_H : c.H;
    sp.logits = w->LG.f();
    sp.B = c.B;
    sp.V = p->V;
    sp.mode = c.mode;
    sp.uniforms = c.uniforms ? c.uniforms + (size_t)ro * 2 + j : nullptr;
    sp.u_stride = (long)sH * 2;
    sp.seed = c.seed;
    sp.clip_index0 = c.clip0;
    sp.clip_table = c.clip_table;
    sp.row_origin = c.row_origin;
    sp.dyn = c.dyn;
    sp.position = (uint32_t)((r - c.pos_r0) * 2 + j + (c.dyn ? 0 : c.pos_base));
    sp.tok32 = w->tok32.i() + (size_t)(r % c.R) * 2 + j;
    sp.tok_stride = (long)c.R * 2;
    sp.codes = c.codes + (size_t)ro * 2 + j;
    sp.code_stride = (long)sH * 2;
    if (c.logits) {
        sp.logits_copy = c.logits + ((size_t)ro * 2 + j) * p->V;
        sp.copy_stride = (long)sH * 2 * p->V;
    }
    MiscScope ms(p->ctx, s);
    float *lp = c.logprob ? c.logprob + (size_t)ro * 2 + j : nullptr;
    SampleCtlParams cp;   // read by the given and the controlled samplers only
    cp.s = sp, cp.ctl = c.ctl, cp.kept = nullptr;
    cp.logprob = lp, cp.lp_stride = (long)sH * 2;
    cp.bias = c.bias, cp.bias_index = c.bias_index, cp.bias_col = j;
    cp.rep = c.rep, cp.rep_ring = c.rep_ring;
    cp.guide_role = c.guide_role, cp.guide_scale = c.guide_scale;
    if (c.alt_src) {   // the given variants where the pass brought given rows
        SampleAltParams ap;
        std::memset(&ap, 0, sizeof(ap));
        ap.g.c = cp;
        if (c.given_rows) {
            ap.g.rows = c.given_rows;
            ap.g.given = c.given + (size_t)ro * 2 + j;
            ap.g.given_stride = (long)sH * 2;
            ap.g.keep = c.keep ? c.keep + (size_t)ro * 2 + j : nullptr;
            ap.g.keep_stride = (long)sH * 2;
        }
        const size_t pos = (size_t)ro * 2 + j;
        ap.n = c.alt.n;
        ap.codes = c.alt.n ? c.alt.codes_dev + pos * c.alt.n : nullptr;
        ap.logprob = c.alt.n ? c.alt.logprob_dev + pos * c.alt.n : nullptr;
        ap.entropy = c.alt.entropy_dev + pos;
        ap.rank = c.alt.rank_dev + pos;
        ap.stride = (long)sH * 2;
        TS_HIP(launch_sample_alt(ap, s));
    } else if (c.given_rows) {
        SampleGivenParams gp;
        gp.c = cp;
        gp.rows = c.given_rows;
        gp.given = c.given + (size_t)ro * 2 + j;
        gp.given_stride = (long)sH * 2;
        gp.keep = c.keep ? c.keep + (size_t)ro * 2 + j : nullptr;
        gp.keep_stride = (long)sH * 2;
        TS_HIP(launch_sample_given(gp, s));
    } else if (c.ctl) {
        TS_HIP(launch_sample_ctl(cp, s));
    } else if (lp) {
        SampleLpParams q;
        q.s = sp;
        q.logprob = lp;
        q.lp_stride = (long)sH * 2;
        TS_HIP(launch_sample_lp(q, s));
    } else {
        TS_HIP(launch_sample(sp, s));
    }
    return 0;
}

int run_row(ts_pixelcnn *p, const RunCfg &c, int r, bool need_h, hipStream_t s) {
    std::vector<Slot> V, H;
    // Slot V0 from row 1 on and hg_0 of column 1 are lookups in the code tables (ts_pixelcnn::CodeTables) where the pass takes them:
    // TS_PIX_TABLES = 1 every pass, 0 none, -1 (default) passes of at least CODE_TABLE_MIN_CLIPS = 64 clips — the passes whose V0 is a wide
    // launch (one 128 KB workgroup per CU, which chains on other streams cannot share).  Below that V0 and hg_0 are `fast` launches of
    // about the cost of the lookup launch, and hg_0 carries a deferred P_l besides.  Bits are equal either way.
    // Up to 128 clips the column-0 launches (vertical slot riding with the horizontal one) come to 272 workgroups at every
    // tile shape — 16 more than CUs, and the 16 doubled-up CUs set the launch time (5.9 vs 3.6 us at 32 clips).  The P_l
    // projections are only read by the next row: there they ride with column 1's launches (96 -> 160 workgroups).
    std::vector<SkinnyParams> Pd;
    const bool defer = need_h && (p->defer_p < 0 ? c.B <= 128 : p->defer_p > 0);
    build_vertical(p, c, r, V, defer ? &Pd : nullptr);
    if (!need_h) {
        for (auto &sl : V) TS_TRY(launch_row_slot(p, c, r, sl, nullptr, s));
        return 0;
    }
    build_horizontal(p, c, r, 0, H);
    size_t vi = 0;
    // hg_0 needs V2H_0 (V1); S_k needs V2H_k (V_{k+1}): V0, V1, H0 + V2, H1 + V3, ...
    for (; vi < 2 && vi < V.size(); ++vi) TS_TRY(launch_row_slot(p, c, r, V[vi], nullptr, s));
    for (size_t k = 0; k < H.size(); ++k) {
        const Slot *ride = nullptr;
        if (vi < V.size() && V[vi].n + H[k].n <= SKINNY_MAX_PROBLEMS) ride = &V[vi++];
        TS_TRY(launch_row_slot(p, c, r, H[k], ride, s));
    }
    for (; vi < V.size(); ++vi) TS_TRY(launch_row_slot(p, c, r, V[vi], nullptr, s));   // only if the stack outlasts the chain
    TS_TRY(launch_sampler(p, c, r, 0, s));
    build_horizontal(p, c, r, 1, H);
    size_t pi = 0;
    for (size_t k = 0; k < H.size(); ++k) {
        Slot ride;
        // the last horizontal slots take what is left, so that every P_l has run before the row ends
        while (!H[k].table && pi < Pd.size() && H[k].n + ride.n < SKINNY_MAX_PROBLEMS && (ride.n == 0 || Pd.size() - pi > H.size() - 1 - k)) {
            ride.add(Pd[pi], ptag(PS_P, (int)pi + 1));
            ++pi;
        }
        TS_TRY(launch_row_slot(p, c, r, H[k], ride.n ? &ride : nullptr, s));
    }
    if (pi < Pd.size()) return fail("pixelcnn: deferred projections left over");
    return launch_sampler(p, c, r, 1, s);
}

}  // namespace

extern "C" {

int ts_pixelcnn_create(ts_ctx *ctx, const ts_tensor *sd_, int n, int V, int D, int NL, int NC, int AD, ts_pixelcnn **out) {
    if (!ctx || !sd_ || !out) return fail("ts_pixelcnn_create: null argument");
    if (D % 32 != 0 || AD % 32 != 0) return fail("PixelCNN dim and audio dim must be multiples of 32");
    if (NL < 1) return fail("n_layers must be >= 1");
    TS_HIP(hipSetDevice(ctx->device));
    StateDict sd(sd_, n);
    std::unique_ptr<ts_pixelcnn> p(new ts_pixelcnn());
    p->ctx = ctx;
    p->V = V;
    p->D = D;
    p->NL = NL;
    p->NC = NC;
    p->AD = AD;
    const int D2 = 2 * D;

    const float *emb = sd.get("embedding.weight", {V, D});
    if (!emb) return 1;
    TS_TRY(p->emb.upload(emb, (size_t)V * D * sizeof(float)));

    p->wvt.resize(NL);
    std::vector<float> cls_all, bv_all;
    for (int l = 0; l < NL; ++l) {
        const std::string q = "layers." + std::to_string(l);
        const int kh = l == 0 ? 4 : 2;       // kernel // 2 + 1 rows, kernel = 7 / 3 (gated_pixelcnn_v2.py:34,112-113)
        const int rows = l == 0 ? 3 : 2;     // mask 'A' zeroes the last row of layer 0 (:57-58)
        const float *wv = sd.get(q + ".vert_stack.weight", {D2, D, kh, 3});
        const float *bv = sd.get(q + ".vert_stack.bias", {D2});
        const float *wvh = sd.get(q + ".vert_to_horiz.weight", {D2, D2, 1, 1});
        const float *bvh = sd.get(q + ".vert_to_horiz.bias", {D2});
        const float *wh = sd.get(q + ".horiz_stack.weight", {D2, D, 1, 2});
        const float *bh = sd.get(q + ".horiz_stack.bias", {D2});
        const float *cl = sd.get(q + ".class_cond_embedding.weight", {NC, D2});
        const float *wr = sd.get(q + ".horiz_resid.weight", {D, D, 1, 1});
        const float *br = sd.get(q + ".horiz_resid.bias", {D});
        if (!wv || !bv || !wvh || !bvh || !wh || !bh || !cl || !wr || !br) return 1;
        // one matrix per kernel row t: output n = (col j, channel co); k = (input col c)*D + ci; kernel column c - j + 1
        std::vector<float> pb((size_t)2 * D2);
        for (int j = 0; j < 2; ++j)
            for (int co = 0; co < D2; ++co) pb[(size_t)j * D2 + co] = bv[co];
        for (int t = 0; t < rows; ++t) {
            std::vector<float> pv((size_t)2 * D2 * 2 * D);
            for (int j = 0; j < 2; ++j)
                for (int co = 0; co < D2; ++co)
                    for (int cc = 0; cc < 2; ++cc)
                        for (int ci = 0; ci < D; ++ci)
                            pv[((size_t)j * D2 + co) * 2 * D + (size_t)cc * D + ci] =
                                wv[(((size_t)co * D + ci) * kh + t) * 3 + (cc - j + 1)];
            TS_TRY(upload_vec(p->wvt[l], pv));
        }
        TS_TRY(upload_vec(p->bv, pb));
        bv_all.insert(bv_all.end(), pb.begin(), pb.end());
        TS_TRY(upload_vec(p->wv2h, std::vector<float>(wvh, wvh + (size_t)D2 * D2)));
        TS_TRY(upload_vec(p->bv2h, std::vector<float>(bvh, bvh + D2)));
        // horizontal: row co, k = tap*D + ci ; tap 0 <-> column j-1, tap 1 <-> column j (kernel (1,2), padding (0,1))
        std::vector<float> ph((size_t)D2 * 2 * D);
        for (int co = 0; co < D2; ++co)
            for (int tap = 0; tap < 2; ++tap)
                for (int ci = 0; ci < D; ++ci)
                    ph[(size_t)co * 2 * D + (size_t)tap * D + ci] =
                        (l == 0 && tap == 1) ? 0.f : wh[((size_t)co * D + ci) * 2 + tap];   // mask 'A' (:59)
        TS_TRY(upload_vec(p->wh, ph));
        TS_TRY(upload_vec(p->bh, std::vector<float>(bh, bh + D2)));
        TS_TRY(upload_vec(p->cls, std::vector<float>(cl, cl + (size_t)NC * D2)));
        cls_all.insert(cls_all.end(), cl, cl + (size_t)NC * D2);
        TS_TRY(upload_vec(p->wr, std::vector<float>(wr, wr + (size_t)D * D)));
        TS_TRY(upload_vec(p->br, std::vector<float>(br, br + D)));
    }
    TS_TRY(p->cls_all.upload(cls_all.data(), cls_all.size() * sizeof(float)));
    TS_TRY(p->bv_all.upload(bv_all.data(), bv_all.size() * sizeof(float)));
    // audio conditioning
    const float *wa = sd.get("embedding_aud.weight", {D, AD, 1, 1}), *ba = sd.get("embedding_aud.bias", {D});
    const float *wfv = sd.get("fusion_v.weight", {D, D2, 1, 1}), *bfv = sd.get("fusion_v.bias", {D});
    const float *wfh = sd.get("fusion_h.weight", {D, D2, 1, 1}), *bfh = sd.get("fusion_h.bias", {D});
    if (!wa || !ba || !wfv || !bfv || !wfh || !bfh) return 1;
    TS_TRY(pack_linear_layer(wa, AD, ba, D, AD, &p->aud_embed));
    TS_TRY(pack_linear_layer(wfv + D, D2, bfv, D, D, &p->aud_fv));
    TS_TRY(pack_linear_layer(wfh + D, D2, bfh, D, D, &p->aud_fh));
    std::vector<float> fa((size_t)D * D), fb((size_t)D * D);
    for (int o = 0; o < D; ++o)
        for (int i = 0; i < D; ++i) {
            fa[(size_t)o * D + i] = wfv[(size_t)o * D2 + i];
            fb[(size_t)o * D + i] = wfh[(size_t)o * D2 + i];
        }
    TS_TRY(p->fha.upload(fb.data(), fb.size() * sizeof(float)));
    if (NL > 1) {
        // layer 1's vertical taps see XV_1 = fusion_v[:, :D] . OV0 + (fusion_v[:, D:] . AE + b) per column.  Compose (fp64,
        // rounded once): W' = W . blockdiag(F, F) acting on OV0, and Ws = W[:, :D] + W[:, D:] acting on the audio term,
        // which is the same for both columns (the audio map is repeated over the 2 columns, smplx_body_pixel.py:274).
        const float *wv1 = sd.get("layers.1.vert_stack.weight", {D2, D, 2, 3});
        if (!wv1) return 1;
        for (int t = 0; t < 2; ++t) {   // t = 0: row above (Wprev), t = 1: the row itself (Wcur)
            std::vector<double> Wt((size_t)2 * D2 * 2 * D);
            for (int j = 0; j < 2; ++j)
                for (int co = 0; co < D2; ++co)
                    for (int cc = 0; cc < 2; ++cc)
                        for (int ci = 0; ci < D; ++ci)
                            Wt[((size_t)j * D2 + co) * 2 * D + (size_t)cc * D + ci] =
                                wv1[(((size_t)co * D + ci) * 2 + t) * 3 + (cc - j + 1)];
            std::vector<float> Wc((size_t)2 * D2 * 2 * D), Ws((size_t)2 * D2 * D);
            for (int n = 0; n < 2 * D2; ++n)
                for (int cc = 0; cc < 2; ++cc)
                    for (int i = 0; i < D; ++i) {
                        double a = 0.0;
                        for (int m = 0; m < D; ++m) a += Wt[(size_t)n * 2 * D + (size_t)cc * D + m] * (double)fa[(size_t)m * D + i];
                        Wc[(size_t)n * 2 * D + (size_t)cc * D + i] = (float)a;
                    }
            for (int n = 0; n < 2 * D2; ++n)
                for (int i = 0; i < D; ++i)
                    Ws[(size_t)n * D + i] = (float)(Wt[(size_t)n * 2 * D + i] + Wt[(size_t)n * 2 * D + D + i]);
            TS_TRY((t == 1 ? p->wv1c : p->wv1p).upload(Wc.data(), Wc.size() * sizeof(float)));
            TS_TRY(pack_linear_layer(Ws.data(), D, nullptr, 2 * D2, D, t == 1 ? &p->aud_v1c : &p->aud_v1p));
        }
    }
    // head
    const float *w1 = sd.get("output_conv.0.weight", {p->HID, D, 1, 1}), *b1 = sd.get("output_conv.0.bias", {p->HID});
    const float *w2 = sd.get("output_conv.2.weight", {V, p->HID, 1, 1}), *b2 = sd.get("output_conv.2.bias", {V});
    if (!w1 || !b1 || !w2 || !b2) return 1;
    TS_TRY(p->w1.upload(w1, (size_t)p->HID * D * sizeof(float)));
    TS_TRY(p->b1.upload(b1, (size_t)p->HID * sizeof(float)));
    TS_TRY(p->w2.upload(w2, (size_t)V * p->HID * sizeof(float)));
    TS_TRY(p->b2.upload(b2, (size_t)V * sizeof(float)));
    // ---- composed horizontal maps (products in double, rounded once) ----
    {
        auto mat = [&](const std::string &k, int rows_, int cols_, int stride_, int off_) {   // rows_ x cols_ view of a conv weight
            const float *src = sd.m.at(k)->data;
            std::vector<double> m((size_t)rows_ * cols_);
            for (int i = 0; i < rows_; ++i)
                for (int jx = 0; jx < cols_; ++jx) m[(size_t)i * cols_ + jx] = src[((size_t)i * cols_ + jx) * stride_ + off_];
            return m;
        };
        auto vec = [&](const std::string &k, int n_) {
            const float *src = sd.m.at(k)->data;
            return std::vector<double>(src, src + n_);
        };
        auto mm = [](const std::vector<double> &A, const std::vector<double> &Bm, int m_, int k_, int n_) {   // (m x k)(k x n)
            std::vector<double> Cm((size_t)m_ * n_, 0.0);
            for (int i = 0; i < m_; ++i)
                for (int kk = 0; kk < k_; ++kk) {
                    const double a = A[(size_t)i * k_ + kk];
                    const double *brow = &Bm[(size_t)kk * n_];
                    double *crow = &Cm[(size_t)i * n_];
                    for (int jx = 0; jx < n_; ++jx) crow[jx] += a * brow[jx];
                }
            return Cm;
        };
        auto mv = [](const std::vector<double> &A, const std::vector<double> &x, int m_, int k_) {
            std::vector<double> y(m_, 0.0);
            for (int i = 0; i < m_; ++i)
                for (int kk = 0; kk < k_; ++kk) y[i] += A[(size_t)i * k_ + kk] * x[kk];
            return y;
        };
        auto upf = [&](std::vector<std::unique_ptr<DevBuf>> &dst, const std::vector<double> &v) {
            return upload_vec(dst, std::vector<float>(v.begin(), v.end()));
        };
        // entry 0 of the per-layer vectors is a placeholder (layer 0 has no composed stage)
        TS_TRY(upload_vec(p->rw, std::vector<float>(1, 0.f)));
        TS_TRY(upload_vec(p->rb, std::vector<float>(1, 0.f)));
        TS_TRY(upload_vec(p->wB, std::vector<float>(1, 0.f)));
        TS_TRY(upload_vec(p->bm, std::vector<float>(1, 0.f)));
        const std::vector<double> Fha = [&] {   // fusion_h[:, :D]
            const float *src = sd.m.at("fusion_h.weight")->data;
            std::vector<double> m((size_t)D * D);
            for (int i = 0; i < D; ++i)
                for (int jx = 0; jx < D; ++jx) m[(size_t)i * D + jx] = src[(size_t)i * D2 + jx];
            return m;
        }();
        for (int l = 1; l < NL; ++l) {
            const std::string q = "layers." + std::to_string(l), qp = "layers." + std::to_string(l - 1);
            std::vector<double> Rw = mat(qp + ".horiz_resid.weight", D, D, 1, 0), rbv = vec(qp + ".horiz_resid.bias", D);
            if (l == 1) {   // XH_1 = fusion_h[:, :D] . (horiz_resid_0 . G_0 + b) + AEH
                rbv = mv(Fha, rbv, D, D);
                Rw = mm(Fha, Rw, D, D, D);
            }
            const std::vector<double> Wh1 = mat(q + ".horiz_stack.weight", D2, D, 2, 1);   // tap 1: the column itself
            const std::vector<double> Wm = mm(Wh1, Rw, D2, D, D);
            std::vector<double> bmv = mv(Wh1, rbv, D2, D);
            const std::vector<double> bhv = vec(q + ".horiz_stack.bias", D2);
            for (int i = 0; i < D2; ++i) bmv[i] += bhv[i];
            const int KB = l == 1 ? D : 2 * D;
            std::vector<double> WB((size_t)D2 * KB);
            for (int i = 0; i < D2; ++i) {
                for (int jx = 0; jx < D; ++jx) WB[(size_t)i * KB + jx] = Wm[(size_t)i * D + jx];
                if (l >= 2)
                    for (int jx = 0; jx < D; ++jx) WB[(size_t)i * KB + D + jx] = Wh1[(size_t)i * D + jx];
            }
            TS_TRY(upf(p->rw, Rw));
            TS_TRY(upf(p->rb, rbv));
            TS_TRY(upf(p->wB, WB));
            TS_TRY(upf(p->bm, bmv));
            if (l == 1) {
                std::vector<float> wh1f(Wh1.begin(), Wh1.end());
                TS_TRY(pack_linear_layer(wh1f.data(), D, nullptr, D2, D, &p->aud_h1));
            }
        }
        {   // head1' = relu(W1 . (horiz_resid_{NL-1} . G + b + XH_{NL-1}) + b1)
            const std::string ql = "layers." + std::to_string(NL - 1);
            const std::vector<double> W1 = mat("output_conv.0.weight", p->HID, D, 1, 0);
            const std::vector<double> Wr = mat(ql + ".horiz_resid.weight", D, D, 1, 0);
            const std::vector<double> W1r = mm(W1, Wr, p->HID, D, D);
            std::vector<double> bb = mv(W1, vec(ql + ".horiz_resid.bias", D), p->HID, D);
            const std::vector<double> b1v = vec("output_conv.0.bias", p->HID);
            for (int i = 0; i < p->HID; ++i) bb[i] += b1v[i];
            const int K1 = NL >= 2 ? 2 * D : D;
            std::vector<float> wm((size_t)p->HID * K1), bf(bb.begin(), bb.end());
            for (int i = 0; i < p->HID; ++i) {
                for (int jx = 0; jx < D; ++jx) wm[(size_t)i * K1 + jx] = (float)W1r[(size_t)i * D + jx];
                if (NL >= 2)
                    for (int jx = 0; jx < D; ++jx) wm[(size_t)i * K1 + D + jx] = (float)W1[(size_t)i * D + jx];
            }
            TS_TRY(p->w1m.upload(wm.data(), wm.size() * sizeof(float)));
            TS_TRY(p->b1m.upload(bf.data(), bf.size() * sizeof(float)));
        }
    }
    // ---- tiled twins of every weight matrix the chain multiplies with (see ts_pixelcnn::tiled) ----
    p->tiled = skinny_descriptor_kernel_enabled() && D % 128 == 0 && p->HID % 128 == 0 && V % 16 == 0;
    if (p->tiled) {
        auto tile = [&](const DevBuf &rm, int N, int K, long ldw, int epi, int gateD) -> int {
            std::vector<float> host((size_t)N * ldw);
            TS_HIP(hipMemcpy(host.data(), rm.p, host.size() * sizeof(float), hipMemcpyDeviceToHost));
            std::vector<float> t((size_t)((N + 15) / 16) * (K / 16) * 256);
            skinny_tile_weights(host.data(), N, K, ldw, epi, gateD, t.data());
            std::unique_ptr<ts_pixelcnn::TiledW> tw(new ts_pixelcnn::TiledW());
            tw->K = K;
            tw->epi = epi;
            TS_TRY(tw->buf.upload(t.data(), t.size() * sizeof(float)));
            p->wtiled[rm.f()] = std::move(tw);
            return 0;
        };
        const int D4 = 4 * D;
        TS_TRY(tile(*p->wvt[0][2], D4, D2, D2, EPI_GATE, D));                              // V0 gate (the two code rows gathered: K = 2D)
        TS_TRY(tile(*p->wvt[0][0], D4, D2, D2, EPI_LINEAR, 0));                            // Q0 / Q1
        TS_TRY(tile(*p->wvt[0][1], D4, D2, D2, EPI_LINEAR, 0));
        for (int l = 1; l < NL; ++l) {
            if (l >= 2) {
                TS_TRY(tile(*p->wvt[l][1], D4, D2, D2, EPI_GATE, D));
                TS_TRY(tile(*p->wvt[l][0], D4, D2, D2, EPI_LINEAR, 0));
            }
            TS_TRY(tile(*p->wh[l], D2, D, D2, EPI_LINEAR, 0));                             // t0: tap-0 block of horiz_stack
            TS_TRY(tile(*p->rw[l], D, D, D, EPI_LINEAR, 0));
            TS_TRY(tile(*p->wB[l], D2, l == 1 ? D : D2, l == 1 ? D : D2, EPI_GATE, D));
        }
        for (int l = 0; l < NL; ++l) TS_TRY(tile(*p->wv2h[l], D2, D2, D2, EPI_LINEAR, 0));
        TS_TRY(tile(*p->wh[0], D2, D, D2, EPI_GATE, D));                                   // hg_0 of column 1 (K = D gather)
        if (NL > 1) {
            TS_TRY(tile(p->wv1c, D4, D2, D2, EPI_GATE, D));
            TS_TRY(tile(p->wv1p, D4, D2, D2, EPI_LINEAR, 0));
        }
        TS_TRY(tile(p->w1m, p->HID, NL >= 2 ? D2 : D, NL >= 2 ? D2 : D, EPI_LINEAR, 0));
        TS_TRY(tile(p->w2, V, p->HID, p->HID, EPI_LINEAR, 0));
    }
    if (ts::knobs().no_graph) p->use_graph = false;
    if (ts::knobs().pix_defer_p >= 0) p->defer_p = ts::knobs().pix_defer_p;
    p->tables_mode = ts::knobs().pix_tables;
    if (p->tables_mode != 0) TS_TRY(build_code_tables(p.get()));   // where they do not fit (code_table_plan) the GEMM launches stay
    *out = p.release();
    return 0;
}
void ts_pixelcnn_destroy(ts_pixelcnn *p) { delete p; }

long ts_pixelcnn_graph_captures(ts_pixelcnn *p, void *stream) {
    if (!p) return -1;
    ts_pixelcnn::Work *w = p->works.find((hipStream_t)stream);
    return w ? w->captures : 0;
}

int ts_debug_pixelcnn_graphs(ts_pixelcnn *p, void *stream) {
    if (!p) return -1;
    ts_pixelcnn::Work *w = p->works.find((hipStream_t)stream);
    return w ? (int)w->graphs.size() : 0;
}

int ts_pixelcnn_graph_stats(ts_pixelcnn *p, void *stream, int B, int H, int mode, int64_t *launches, double *flops) {
    if (!p) return fail("ts_pixelcnn_graph_stats: null argument");
    ts_pixelcnn::Work *w = p->works.find((hipStream_t)stream);
    if (!w) return fail("ts_pixelcnn_graph_stats: nothing was run on this stream");
    auto jt = w->graph_stats.find(std::make_tuple(B, H, 0, mode, 0, 0));
    if (jt == w->graph_stats.end()) return fail("ts_pixelcnn_graph_stats: no captured graph for this shape");
    if (launches) *launches = jt->second.first;
    if (flops) *flops = jt->second.second;
    return 0;
}

// Stage taps (talkshow_hip_debug.h): the table waits for the next chain entry of this thread
int ts_debug_pixelcnn_taps(const ts_debug_pix_tap_table *taps) {
    g_ptaps.pending = taps != nullptr;
    if (taps) g_ptaps.t = *taps;
    return 0;
}

// ---- code tables: test entries (talkshow_hip_debug.h) ----
// TS_PIX_TABLES for one model object: mode -1 / 0 / 1 as the variable (-2: change nothing, only answer); builds the tables if they are
// wanted and fit.  Every captured graph of the object's per-stream Works is dropped (their launches belong to the old setting); streaming
// sessions opened earlier keep theirs.
// Returns 1 if the tables exist, 0 if not (mode 0 before any build, or they do not fit), -1 on error
int ts_debug_pixelcnn_tables(ts_pixelcnn *p, int mode) {
    if (!p || mode < -2 || mode > 1) return fail("ts_debug_pixelcnn_tables: bad argument") ? -1 : -1;
    if (mode == -2) return p->tables.built ? 1 : 0;   // a question only
    if (hipSetDevice(p->ctx->device) != hipSuccess) return fail("ts_debug_pixelcnn_tables: hipSetDevice") ? -1 : -1;
    if (mode != 0 && build_code_tables(p) != 0) return -1;
    p->tables_mode = mode;
    {
        std::lock_guard<std::mutex> g(p->works.mu);
        for (auto &kv : p->works.m) kv.second->drop_graphs();
    }
    return p->tables.built ? 1 : 0;
}

// A work buffer of `stream`'s Work, whole: which = 0 HV, 1 OV0, 2 Q1, 3 Q0, 4 G, 5 AE, 6 AEV, 7 AEH, 8 AEH1, 9 AV1C, 10 AV1P, 11 tok32 (int32 words),
// 12 XV, 13 P, 14 V2H, 15 XH, 16 T0.  put = 0: copied to buf_dev, put = 1: filled from buf_dev
// (tests poison the buffers ahead of a run).  Copies min(buffer, cap_floats) floats behind the stream's work and waits; returns the count, -1 on error
int64_t ts_debug_pixelcnn_work(ts_pixelcnn *p, void *stream, int which, float *buf_dev, int64_t cap_floats, int put) {
    if (!p || !buf_dev || cap_floats < 0 || which < 0 || which > 16) return fail("ts_debug_pixelcnn_work: bad argument") ? -1 : -1;
    ts_pixelcnn::Work *w = p->works.find((hipStream_t)stream);
    if (!w) return fail("ts_debug_pixelcnn_work: nothing was run on this stream") ? -1 : -1;
    DevBuf *bufs[17] = {&w->HV,   &w->OV0,  &w->Q1,   &w->Q0,    &w->G, &w->AE,  &w->AEV, &w->AEH, &w->AEH1,
                        &w->AV1C, &w->AV1P, &w->tok32, &w->XV,   &w->P, &w->V2H, &w->XH,  &w->T0};
    const size_t n = std::min((size_t)cap_floats, bufs[which]->bytes / sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(put ? bufs[which]->p : (void *)buf_dev, put ? (const void *)buf_dev : bufs[which]->p, n * sizeof(float), hipMemcpyDeviceToDevice, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail("ts_debug_pixelcnn_work: copy failed") ? -1 : -1;
    return (int64_t)n;
}

// One lookup launch on the caller's row-major buffers (the red-zone tests): which = 0 slot V0 — tok (B,2) int32 codes of the row above,
// add1 / add2 (B,4D) or null, cls (B,2D), pre (B,4D), out (B,2D), q1 / q0 (B,4D) rider outputs or null; which = 1 hg_0 of column 1 — tok
// (B,2) of which column 0 is read, add1 (B,2D) or null, cls (B,2D), out (B,D); the rest null.  Needs the tables (ts_debug_pixelcnn_tables)
int ts_debug_code_table_stage(ts_pixelcnn *p, int which, const int32_t *tok, int B, const float *add1, const float *add2, const float *cls,
                              float *pre, float *out, float *q1, float *q0, void *stream) {
    if (!p || !tok || !cls || !out || B < 1 || which < 0 || which > 1) return fail("ts_debug_code_table_stage: bad argument");
    if (!p->tables.built) return fail("ts_debug_code_table_stage: this model has no code tables");
    const int D = p->D;
    CodeTableStage ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.M = B, ts.gateD = D;
    ts.tok0 = tok, ts.tok1 = tok + 1, ts.tok_stride = 2;
    ts.cls = cls, ts.cls_ld = 2 * D;
    ts.out = out;
    if (which == 0) {
        for (int m = 0; m < 3; ++m) ts.tab[m] = p->tables.v0[m].f();
        ts.set_stride = (long)p->V * 4 * D;
        ts.nsets = p->tables.sets;
        ts.N = 4 * D;
        ts.bias = p->bv[0]->f();
        ts.add1 = add1, ts.add2 = add2, ts.add1_stride = ts.add2_stride = 4 * D;
        ts.pre = pre, ts.pre_stride = 4 * D;
        ts.out_stride = 2 * D;
        ts.rider[0] = q1, ts.rider[1] = q0, ts.rider_stride = 4 * D;
    } else {
        ts.tab[0] = p->tables.hg.f();
        ts.set_stride = (long)p->V * 2 * D;
        ts.nsets = 1;
        ts.N = 2 * D;
        ts.bias = p->bh[0]->f();
        ts.add1 = add1, ts.add1_stride = 2 * D;
        ts.out_stride = D;
    }
    MiscScope ms(p->ctx, (hipStream_t)stream);
    TS_HIP(launch_code_table_stage(ts, (hipStream_t)stream));
    return 0;
}

}  // extern "C"

namespace {
// ---- a pass's sampler tables (host_common.h: SamplerTables) behind their check: into the Work, then into the run configuration -------
// the sixth field of a graph key: which sampler the run's launches are (Work::Key)
inline int sampler_bits(const RunCfg &c, const float *logprob) {
    const bool given = c.given_rows;
    return (c.ctl ? 1 : 0) | (logprob ? 2 : 0) | (given ? 4 : 0) | (given && c.keep_src ? 8 : 0) | (c.style ? 16 : 0) | (c.bias ? 32 : 0) | (c.rep ? 64 : 0) |
           (c.row_origin ? 128 : 0) | (c.guide_role ? 256 : 0) | (c.alt_src ? 512 | (c.alt_src->n << 10) : 0);
}
// The tables reach the Work in stream order as kernel ARGUMENTS (launch_put_words): nothing on the host has to outlive the call, nothing
// synchronises, and any number of calls — each with its own tables — may be queued behind each other.
int stage_sampler_tables(ts_pixelcnn *p, ts_pixelcnn::Work *w, const SamplerTables &t, const MixedOpts &o, hipStream_t s) {
    static_assert(sizeof(SampleCtl) == 4 * sizeof(int) && sizeof(SampleRep) == 4 * sizeof(int), "SampleCtl and SampleRep are four words");
    ts_ctx *ctx = p->ctx;
    const int B = t.B;
    if (!t.ctl.empty()) {
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(w->ctl_tab.i(), reinterpret_cast<const int *>(t.ctl.data()), (long)B * 4, s));
    }
    if (o.bias) {   // n_bias <= B <= capB tables: the buffer follows capB alone (see Work::bias_tab), so it moves only when ensure_work has
                    // dropped the graphs that read it (a session's capacity is fixed); the index travels as kernel arguments
        TS_TRY(w->bias_tab.ensure((size_t)w->capB * 2 * p->V * sizeof(float)));
        MiscScope ms(ctx, s);
        TS_HIP(hipMemcpyAsync(w->bias_tab.p, o.bias, (size_t)o.n_bias * 2 * p->V * sizeof(float), hipMemcpyDeviceToDevice, s));
        TS_HIP(launch_put_words(static_cast<int *>(w->bias_idx.p), o.bias_index_host, B, s));
    }
    if (o.rep_host) {   // the records as kernel arguments, like the sampling table; a pass without tables brings the index the BIAS path wants
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(static_cast<int *>(w->rep_tab.p), reinterpret_cast<const int *>(t.rep.data()), (long)B * 4, s));
        if (!o.bias) TS_HIP(launch_put_words(static_cast<int *>(w->bias_idx.p), t.no_bias.data(), B, s));
    }
    if (o.given) {   // stream-ordered, as kernel arguments: the host table is free when the call returns
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(w->given_tab.i(), t.given_rows.data(), B, s));
    }
    if (o.guide_host) {   // roles and scales as kernel arguments, and what the REP path reads where the pass brought no records / no tables
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(w->guide_tab.i(), t.guide_role.data(), B, s));
        TS_HIP(launch_put_words(w->guide_scl.i(), reinterpret_cast<const int *>(t.guide_scale.data()), B, s));
        if (!o.rep_host) {
            TS_HIP(launch_put_words(static_cast<int *>(w->rep_tab.p), reinterpret_cast<const int *>(t.rep.data()), (long)B * 4, s));
            if (!o.bias) TS_HIP(launch_put_words(static_cast<int *>(w->bias_idx.p), t.no_bias.data(), B, s));
        }
    }
    if (t.alt) {   // what the REP path reads where the pass brought no records / no tables, and the staging block of the four outputs
        MiscScope ms(ctx, s);
        if (!o.rep_host) {
            TS_HIP(launch_put_words(static_cast<int *>(w->rep_tab.p), reinterpret_cast<const int *>(t.rep.data()), (long)B * 4, s));
            if (!o.bias) TS_HIP(launch_put_words(static_cast<int *>(w->bias_idx.p), t.no_bias.data(), B, s));
        }
        TS_TRY(w->alt_int.ensure((size_t)w->capB * w->capH * 2 * (2 * SAMPLE_ALT_MAX + 2) * sizeof(float)));
    }
    return 0;
}
// Every table is indexed by the clip's slot in the pass (in a mixed pass the active clips are a prefix, so the slot is the same in every
// chunk).  The given variants run in every chunk of a pass that brought given codes (one set of graph keys); which chunks stage codes, and
// under which mask, is the caller's (given_stage, keep_src)
void bind_sampler_tables(RunCfg &c, ts_pixelcnn::Work *w, const MixedOpts &o) {
    if (o.ctl_host || o.bias || o.rep_host) c.ctl = static_cast<const SampleCtl *>(w->ctl_tab.p);
    if (o.bias) c.bias = w->bias_tab.f(), c.bias_index = static_cast<const int32_t *>(w->bias_idx.p);
    if (o.rep_host) {   // records and rings; without tables the staged index is -1 everywhere and c.bias stays null
        c.rep = static_cast<const SampleRep *>(w->rep_tab.p);
        c.rep_ring = static_cast<int32_t *>(w->rep_ring.p);
        c.bias_index = static_cast<const int32_t *>(w->bias_idx.p);
    }
    if (o.given) c.given_rows = w->given_tab.i(), c.given_src = o.given;
    if (o.guide_host) {   // the guided samplers read everything the sample_ctl_rep kernels read
        c.ctl = static_cast<const SampleCtl *>(w->ctl_tab.p);
        c.rep = static_cast<const SampleRep *>(w->rep_tab.p);
        c.rep_ring = static_cast<int32_t *>(w->rep_ring.p);
        c.bias_index = static_cast<const int32_t *>(w->bias_idx.p);
        c.guide_role = w->guide_tab.i();
        c.guide_scale = w->guide_scl.f();
    }
    if (o.alt) {   // the alternatives samplers read everything the sample_ctl_rep kernels read
        c.ctl = static_cast<const SampleCtl *>(w->ctl_tab.p);
        c.rep = static_cast<const SampleRep *>(w->rep_tab.p);
        c.rep_ring = static_cast<int32_t *>(w->rep_ring.p);
        c.bias_index = static_cast<const int32_t *>(w->bias_idx.p);
        c.alt_src = o.alt;
    }
}

// audio conditioning of `rows` code rows per clip: AE = embedding_aud(aud); AEV / AEH = fusion_{v,h}[:, D:] . AE + bias;
// AEH1 = layer 1's horiz_stack applied to AEH (gated_pixelcnn_v2.py:137-144) — four conv_gemm launches for all rows at once
int audio_terms(ts_pixelcnn *p, ts_pixelcnn::Work *w, const float *aud, int B, int rows, hipStream_t s) {
    ts_ctx *ctx = p->ctx;
    const int D = p->D, AD = p->AD;
    ConvParams q;
    conv_layer_params(p->aud_embed, aud, AD, 1, B * rows, nullptr, 0, w->AE.f(), D, 0, D, &q);
    TS_TRY(run_conv(ctx, q, 0, s));
    conv_layer_params(p->aud_fv, w->AE.f(), D, 1, B * rows, nullptr, 0, w->AEV.f(), D, 0, D, &q);
    TS_TRY(run_conv(ctx, q, 0, s));
    conv_layer_params(p->aud_fh, w->AE.f(), D, 1, B * rows, nullptr, 0, w->AEH.f(), D, 0, D, &q);
    TS_TRY(run_conv(ctx, q, 0, s));
    if (p->NL > 1) {
        conv_layer_params(p->aud_h1, w->AEH.f(), D, 1, B * rows, nullptr, 0, w->AEH1.f(), 2 * D, 0, 2 * D, &q);
        TS_TRY(run_conv(ctx, q, 0, s));
        conv_layer_params(p->aud_v1c, w->AEV.f(), D, 1, B * rows, nullptr, 0, w->AV1C.f(), 4 * D, 0, 4 * D, &q);
        TS_TRY(run_conv(ctx, q, 0, s));
        conv_layer_params(p->aud_v1p, w->AEV.f(), D, 1, B * rows, nullptr, 0, w->AV1P.f(), 4 * D, 0, 4 * D, &q);
        TS_TRY(run_conv(ctx, q, 0, s));
    }
    return 0;
}

// class conditioning rows: CR[l][b] = class_cond_embedding_l[label[b]]  (h of gated_pixelcnn_v2.py:65)
int class_rows(ts_pixelcnn *p, ts_pixelcnn::Work *w, const int64_t *label, int B, hipStream_t s) {
    const int D = p->D;
    MiscScope ms(p->ctx, s);
    for (int l = 0; l < p->NL; ++l)
        TS_HIP(launch_gather_rows(p->cls[l]->f(), 2 * D, p->NC, label, 1, B, 2 * D, w->CR.f() + (size_t)l * B * 2 * D, 2 * D, s));
    return 0;
}

// "speaker style" (talkshow_hip.h): the same rows from float weights, one row of NC weights per clip slot (style (B,NC)), through
// style_rows_kernel in place of the gather.  CR's content is in no graph key: the pass behind it is the pass behind the labels
int class_rows_style(ts_pixelcnn *p, ts_pixelcnn::Work *w, const float *style, int B, hipStream_t s) {
    MiscScope ms(p->ctx, s);
    StyleRowsParams q;
    std::memset(&q, 0, sizeof(q));
    q.tables = p->cls_all.f();
    q.weights = style;
    q.w_ld = p->NC;
    q.S = 1, q.NC = p->NC, q.W = 2 * p->D, q.NL = p->NL;
    q.r0 = 0, q.n = 1, q.slots = B;
    q.out = w->CR.f();
    q.out_l_stride = (long)B * 2 * p->D;
    q.out_r_stride = 0;
    TS_HIP(launch_style_rows(q, s));
    return 0;
}

// Runs rows [r_begin, r_end) of `c`: eagerly, or as a replay of the hipGraph captured for `key` (host launch cost would
// otherwise dominate: ~37 dependent tiny launches per row).  On the graph path the kernels write codes into the Work's
// staging buffer (every pointer inside a captured kernel is a Work buffer, so a graph is valid for any caller pointers);
// the caller's arrays hold c.out_H rows per clip, of which this run covers rows c.out_row0 .. c.out_row0 + c.H - 1.
int run_rows(ts_pixelcnn *p, RunCfg c, int r_begin, int r_end, bool graph, const ts_pixelcnn::Work::Key &key,
             const float *uniforms, int64_t *codes, float *logprob, hipStream_t s, bool capture_only = false) {
    ts_pixelcnn::Work *w = c.w;
    const int out_H = c.out_H > 0 ? c.out_H : c.H;
    auto row_loop = [&](hipStream_t st) -> int {
        for (int r = r_begin; r < r_end; ++r) {
            // prefix rows only feed the row cache; so do teacher-forced rows that return neither logits nor log-probabilities
            const bool need_h = r >= c.out_r0 && !(c.mode == TS_TEACHER_FORCED && !c.logits && !logprob);
            TS_TRY(run_row(p, c, r, need_h, st));
        }
        return 0;
    };
    if (tapping() && !capture_only) graph = false;   // a tapped pass runs eagerly: no graph ever holds a tap copy, the cache is not touched
    if (!graph) {   // the samplers address the caller's arrays directly: rows out_row0 .. of out_H per clip
        if (out_H != c.H && c.logits) return fail("pixelcnn: eager rows with logits write the caller's arrays whole");
        c.codes = codes;
        c.logprob = logprob;
        if (c.alt_src) c.alt = *c.alt_src;
        c.uniforms = uniforms;
        c.given = c.given_src;
        c.keep = c.keep_src;
        c.io_H = out_H;
        c.io_row0 = c.out_row0;
        return row_loop(s);
    }
    c.given = static_cast<const int64_t *>(w->given_int.p);
    if (c.given_rows && c.given_stage && !capture_only)   // the chunk's rows of the given block, the way the uniforms travel
        TS_HIP(hipMemcpy2DAsync(w->given_int.p, (size_t)c.H * 2 * sizeof(int64_t), c.given_src + (size_t)c.out_row0 * 2,
                                (size_t)out_H * 2 * sizeof(int64_t), (size_t)c.H * 2 * sizeof(int64_t), c.B, hipMemcpyDeviceToDevice, s));
    c.keep = c.keep_src ? static_cast<const unsigned char *>(w->keep_int.p) : nullptr;
    if (c.given_rows && c.keep_src && c.given_stage && !capture_only)   // and the same rows of the mask
        TS_HIP(hipMemcpy2DAsync(w->keep_int.p, (size_t)c.H * 2, c.keep_src + (size_t)c.out_row0 * 2, (size_t)out_H * 2, (size_t)c.H * 2, c.B,
                                hipMemcpyDeviceToDevice, s));
    c.codes = static_cast<int64_t *>(w->codes_int.p);
    c.logprob = logprob ? w->lp_int.f() : nullptr;
    if (c.alt_src) {   // the four blocks of alt_int
        const size_t cap = (size_t)w->capB * w->capH * 2;
        c.alt = *c.alt_src;
        c.alt.codes_dev = static_cast<int32_t *>(w->alt_int.p);
        c.alt.logprob_dev = w->alt_int.f() + cap * SAMPLE_ALT_MAX;
        c.alt.entropy_dev = w->alt_int.f() + cap * 2 * SAMPLE_ALT_MAX;
        c.alt.rank_dev = static_cast<int32_t *>(w->alt_int.p) + cap * (2 * SAMPLE_ALT_MAX + 1);
    }
    c.uniforms = c.mode == TS_SAMPLE_UNIFORMS ? w->unif_int.f() : nullptr;
    c.dyn = static_cast<const uint64_t *>(w->dyn.p);
    if (c.mode == TS_SAMPLE_UNIFORMS && !capture_only)
        TS_HIP(hipMemcpy2DAsync(w->unif_int.p, (size_t)c.H * 2 * sizeof(float), uniforms + (size_t)c.out_row0 * 2,
                                (size_t)out_H * 2 * sizeof(float), (size_t)c.H * 2 * sizeof(float), c.B, hipMemcpyDeviceToDevice, s));
    // the call's sampler words travel as the ARGUMENTS of a one-thread launch (copied when the launch is queued): no host buffer
    // has to stay intact behind the call, so any number of calls may be queued on the stream without a synchronisation
    if (!capture_only) TS_HIP(launch_set_words3(static_cast<uint64_t *>(w->dyn.p), c.seed, (uint64_t)c.clip0, (uint64_t)c.pos_base, s));
    auto it = w->graphs.find(key);
    if (it == w->graphs.end()) {
        TS_TRY(w->make_room(s, key));
        if (!w->cap_stream) TS_HIP(hipStreamCreateWithFlags(&w->cap_stream, hipStreamNonBlocking));
        hipGraph_t g = nullptr;
        TS_HIP(hipStreamBeginCapture(w->cap_stream, hipStreamCaptureModeThreadLocal));
        int rc;
        {   // this thread's launches only: the context-wide counters move with every other thread inside the library
            SkinnyTally tally;
            rc = row_loop(w->cap_stream);
            w->graph_stats[key] = {tally.launches, tally.flops};
        }
        const hipError_t ec = hipStreamEndCapture(w->cap_stream, &g);
        if (rc != 0) {
            if (g) (void)hipGraphDestroy(g);
            return rc;
        }
        if (ec != hipSuccess) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
        hipGraphExec_t ex = nullptr;
        const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess) return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
        ++w->captures;
        it = w->graphs.emplace(key, ts_pixelcnn::Work::Entry{ex, 0}).first;
    }
    if (capture_only) return 0;
    it->second.used = ++w->tick;
    TS_HIP(hipGraphLaunch(it->second.exec, s));
    TS_HIP(hipMemcpy2DAsync(codes + (size_t)c.out_row0 * 2, (size_t)out_H * 2 * sizeof(int64_t), w->codes_int.p,
                            (size_t)c.H * 2 * sizeof(int64_t), (size_t)c.H * 2 * sizeof(int64_t), c.B, hipMemcpyDeviceToDevice, s));
    if (logprob)   // the same rows of the caller's log-probability array, the way the codes travel
        TS_HIP(hipMemcpy2DAsync(logprob + (size_t)c.out_row0 * 2, (size_t)out_H * 2 * sizeof(float), w->lp_int.p,
                                (size_t)c.H * 2 * sizeof(float), (size_t)c.H * 2 * sizeof(float), c.B, hipMemcpyDeviceToDevice, s));
    if (c.alt_src) {   // and of the four alternatives arrays: n words per position, then one
        const ts_alt_out &d = *c.alt_src;
        const size_t e = sizeof(float), n = (size_t)d.n;
        struct { void *dst; const void *src; size_t words; } blocks[4] = {{d.codes_dev, c.alt.codes_dev, n}, {d.logprob_dev, c.alt.logprob_dev, n},
                                                                          {d.entropy_dev, c.alt.entropy_dev, 1}, {d.rank_dev, c.alt.rank_dev, 1}};
        for (auto &m : blocks)
            if (m.words)
                TS_HIP(hipMemcpy2DAsync(static_cast<char *>(m.dst) + (size_t)c.out_row0 * 2 * m.words * e, (size_t)out_H * 2 * m.words * e, m.src,
                                        (size_t)c.H * 2 * m.words * e, (size_t)c.H * 2 * m.words * e, c.B, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// A one-shot call (no prefix) as a sequence of CHUNK_ROWS-row graphs: the reference's own evaluation loop
// (scripts/test_body.py:113-194) feeds clips of arbitrary lengths, and a whole-call graph per length would cost a capture +
// instantiate of ~36 H nodes for every new H and keep them all.  A chunk's graph depends on (B, rows in the chunk, buffer
// phase of its first row, mode) only — the streaming sessions' construction (ts_pixelcnn_stream_step): a 4-row token ring, rows
// indexed absolutely, the Philox position base a device word — so two graphs (first chunk, later chunks) plus one or two for the
// short last chunk serve every clip length.  The audio terms were computed for the whole call; a chunk's rows are copied into the
// compact chunk buffers its graph reads.  Bit-identical to the whole-call graph (same launches, same order, same rings: only the
// look-ahead partial sums of rows past the end are computed and never read).

// Rows [r0, r0 + Hc) behind a row cache, indexed absolutely: what a chunk of a one-shot call and a session step share.  The token ring
// keeps 4 rows: layer 0 looks three code rows up; 4 also is the period of the Q ring.  The audio pointers are the caller's
RunCfg ring_cfg(ts_pixelcnn::Work *w, int B, int r0, int Hc, int mode, uint64_t seed, int64_t clip0) {
    return RunCfg{B, Hc, 0, r0 + Hc, mode, nullptr, seed, clip0, nullptr, nullptr, nullptr, w,
                  /* ring */ 4, r0, Hc, r0, r0, 2l * r0, 0x7fffffff};
}
// a captured chunk is valid for every start row with the same buffer phases (parity of the per-layer row cache, slot in the 4-row
// rings) and the same set of existing rows above (rows 0..2 have fewer): graphs are keyed on that, not on r0
inline int ring_phase(int r0) { return r0 < 3 ? r0 : 3 + (r0 % 4); }
// rows [r0, r0 + Hc) of a call of out_H rows as one chunk: the Work's compact chunk buffers for the audio terms
RunCfg chunk_cfg(ts_pixelcnn::Work *w, int B, int r0, int Hc, int out_H, int mode, uint64_t seed, int64_t clip0) {
    RunCfg c = ring_cfg(w, B, r0, Hc, mode, seed, clip0);
    c.aeh = w->cAEH.f(), c.aeh1 = w->cAEH1.f(), c.av1c = w->cAV1C.f(), c.av1p = w->cAV1P.f();
    c.out_H = out_H;
    c.out_row0 = r0;
    return c;
}
// the graph key of chunk `c` in a pass of Bs clip slots (0: a uniform call): its rows, the buffer phase of its first row, its samplers
ts_pixelcnn::Work::Key chunk_key(const RunCfg &c, int Bs, const float *logprob) {
    return std::make_tuple(c.B, c.H, -(1 + ring_phase(c.out_row0)), c.mode, Bs, sampler_bits(c, logprob));
}
// the chunk's rows of the whole call's audio terms (H rows per clip), for the first B clips, into the chunk buffers
int stage_chunk_audio(ts_pixelcnn *p, ts_pixelcnn::Work *w, int B, int r0, int Hc, int H, hipStream_t s) {
    const size_t D = p->D, f = sizeof(float);
    struct { const DevBuf *src; DevBuf *dst; size_t width; } rows[4] = {
        {&w->AEH, &w->cAEH, D}, {&w->AEH1, &w->cAEH1, 2 * D}, {&w->AV1C, &w->cAV1C, 4 * D}, {&w->AV1P, &w->cAV1P, 4 * D}};
    for (auto &m : rows)
        if (p->NL > 1 || m.src == &w->AEH)
            TS_HIP(hipMemcpy2DAsync(m.dst->p, (size_t)Hc * m.width * f, m.src->f() + (size_t)r0 * m.width, (size_t)H * m.width * f,
                                    (size_t)Hc * m.width * f, B, hipMemcpyDeviceToDevice, s));
    return 0;
}

int run_chunked(ts_pixelcnn *p, ts_pixelcnn::Work *w, int B, int H, int mode, const float *uniforms, uint64_t seed, int64_t clip0,
                int64_t *codes, const SampleCtl *ctl, float *logprob, hipStream_t s) {
    for (int r0 = 0; r0 < H; r0 += CHUNK_ROWS) {
        const int Hc = std::min(CHUNK_ROWS, H - r0);
        RunCfg c = chunk_cfg(w, B, r0, Hc, H, mode, seed, clip0);
        c.ctl = ctl;
        TS_TRY(stage_chunk_audio(p, w, B, r0, Hc, H, s));
        TS_TRY(run_rows(p, c, r0, r0 + Hc, true, chunk_key(c, 0, logprob), uniforms, codes, logprob, s));
    }
    return 0;
}

// ---- mixed passes: clips of different lengths in one pass (talkshow_hip.h has the contract) ------------------------------------------
// The network is causal in the row direction and no clip reads another, so code row r only has to be computed for the clips that have
// more than r rows.  With the clips ordered by non-increasing length those are a PREFIX of every per-clip buffer: chunk [r0, r0 + 8) runs
// with B = #{b : H_b > r0} on the chunk graphs of run_chunked.  A clip that ends inside a chunk is carried to the chunk's end; its surplus
// rows are computed and discarded (harmless by causality, like the look-ahead sums past the end of a uniform call).
//
// Pure host arithmetic (ts_debug_mixed_plan, tests/test_mixed_pass_host.py): active[k] = clips of chunk k.  A pass may use at most
// `max_counts` DISTINCT active counts; beyond that every count is rounded UP to a multiple of grid = 2, 4, 8, ... (capped at B) — finished
// clips are carried along, which is always correct — until the distinct counts fit.  Returns the grid.
int mixed_plan(const int *hrows, int B, int max_counts, std::vector<int> &active) {
    const int nchunks = (hrows[0] + CHUNK_ROWS - 1) / CHUNK_ROWS;
    std::vector<int> raw(nchunks);
    for (int k = 0; k < nchunks; ++k) {
        int n = 0;
        while (n < B && hrows[n] > k * CHUNK_ROWS) ++n;   // non-increasing lengths: the active clips are the first n
        raw[k] = n;
    }
    for (int grid = 1;; grid *= 2) {
        active.resize(nchunks);
        std::set<int> distinct;
        for (int k = 0; k < nchunks; ++k) {
            active[k] = std::min(B, round_up(raw[k], grid));
            distinct.insert(active[k]);
        }
        if ((int)distinct.size() <= max_counts) return grid;
    }
}

// graph keys of one mixed pass: one for the first chunk (buffer phase 0), one per distinct active count for the chunks behind it, one or
// two for a short last chunk — MIXED_MAX_COUNTS + 3 <= the 16 chunk-class slots of Work::make_room, so that a repeated pass finds every
// graph it needs and captures nothing from its second run on
constexpr int MIXED_MAX_COUNTS = 12;

// the chunks of one validated pass whose tables are staged in the Work: a.rows = H_max, hrows the clips' own code rows
int run_mixed(ts_pixelcnn *p, ts_pixelcnn::Work *w, const MixedPass &a, const MixedOpts &o, const std::vector<int> &hrows, bool graph, hipStream_t s) {
    const int B = a.B, H_max = a.rows;
    const size_t D = p->D;
    const bool tracked = o.style && o.style_rows > 1;
    int given_max = 0;
    if (o.given)
        for (int b = 0; b < B; ++b) given_max = std::max(given_max, (int)o.given_rows_host[b]);
    std::vector<int> active;
    (void)mixed_plan(hrows.data(), B, MIXED_MAX_COUNTS, active);
    for (int k = 0; k < (int)active.size(); ++k) {
        const int r0 = k * CHUNK_ROWS, Hc = std::min(CHUNK_ROWS, hrows[0] - r0), Ba = active[k];
        RunCfg c = chunk_cfg(w, Ba, r0, Hc, H_max, a.mode, a.seed, 0);
        c.Bs = B;
        c.clip_table = static_cast<const int64_t *>(w->clip_tab.p);
        bind_sampler_tables(c, w, o);
        if (o.given) {   // only chunks with rows below max G stage codes; a masked pass runs the masked form in every chunk
            c.keep_src = o.keep;
            c.given_stage = r0 < given_max;
        }
        if (tracked) {   // the chunk's conditioning rows, staged eagerly ahead of the replay like its uniforms and given codes: the only
                         // launch that reads the caller's weight block, so no caller pointer enters a captured graph
            MiscScope ms(p->ctx, s);
            StyleRowsParams q;
            std::memset(&q, 0, sizeof(q));
            q.tables = p->cls_all.f();
            q.weights = o.style;
            q.w_ld = p->NC;
            q.S = H_max, q.NC = p->NC, q.W = (int)(2 * D), q.NL = p->NL;
            q.r0 = r0, q.n = Hc, q.slots = Ba;
            q.lens = a.lens_dev, q.len_shr = 2;
            q.out = w->style_int.f();
            q.out_l_stride = (long)CHUNK_ROWS * B * 2 * D;
            q.out_r_stride = (long)B * 2 * D;
            TS_HIP(launch_style_rows(q, s));
            c.style = w->style_int.f();
            c.style_r0 = r0;
        }
        TS_TRY(stage_chunk_audio(p, w, Ba, r0, Hc, H_max, s));
        TS_TRY(run_rows(p, c, r0, r0 + Hc, graph, chunk_key(c, B, o.logprob), a.uniforms, a.codes, o.logprob, s));
    }
    return 0;
}

}  // namespace

extern "C" {

// Host only (no GPU): the chunk plan of a mixed pass.  hrows (B,) code rows per clip, non-increasing, >= 1; max_counts <= 0 = the
// library's bound.  active_out (ceil(hrows[0] / 8),) clips of every 8-row chunk (may be NULL); returns the rounding grid (1 = no rounding), -1 on a bad table.
int ts_debug_mixed_plan(const int32_t *hrows, int B, int max_counts, int32_t *active_out) {
    if (!hrows || B < 1) return fail("ts_debug_mixed_plan: bad argument") ? -1 : -1;
    for (int b = 0; b < B; ++b)
        if (hrows[b] < 1 || (b > 0 && hrows[b] > hrows[b - 1])) return fail("ts_debug_mixed_plan: lengths must be >= 1 and non-increasing") ? -1 : -1;
    std::vector<int> active;
    const int grid = mixed_plan(hrows, B, max_counts > 0 ? max_counts : MIXED_MAX_COUNTS, active);
    if (active_out)
        for (size_t k = 0; k < active.size(); ++k) active_out[k] = active[k];
    return grid;
}

int ts_pixelcnn_generate_mixed_ctl(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                   int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                   int64_t *codes, const ts_sampling *ctl_host, int n_ctl, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

// the mixed pass with a log-probability output (B,H_max,2): rows at or beyond a clip's own H_b are 0 (logprob == NULL: the entry above)
int ts_pixelcnn_generate_mixed_lp(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                  int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                  int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}
// the mixed pass in which clip b brings given_rows[b] code rows that are taken, not drawn (talkshow_hip.h, "given rows"); given == NULL: the
// _lp entry, launch for launch
int ts_pixelcnn_generate_mixed_given(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                     int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                     int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                     const int32_t *given_rows_host, const int32_t *given_rows_dev, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

int ts_pixelcnn_generate_mixed_keep(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                    int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                    int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                    const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

// the given pass with a mask of kept positions beside the given block (talkshow_hip.h, "kept positions"): position (r, j) of clip b is taken
// iff r < G_b and keep[b, r, j] != 0, every other position is produced.  keep == NULL: the _given entry, launch for launch.
// With "speaker style" (talkshow_hip.h): style (B, style_rows, NC) float weights in slot order take the place of the labels — style_rows == 1
// fills CR through style_rows_kernel and changes nothing else; style_rows == H_max stages every chunk's conditioning rows into style_int and
// runs on graph keys of its own (bit 4).  style == NULL: the _keep entry, launch for launch
int ts_pixelcnn_generate_mixed_style(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                     int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                     int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                     const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, const float *style,
                                     int style_rows, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}
// the same pass under a "code bias" (talkshow_hip.h): bias_dev (n_bias,2,V) fp32 tables on the device, bias_index_host (B,) the table of every
// clip in slot order or -1.  Tables and index are copied into the Work in stream order ahead of the pass; the samplers are the
// sample_ctl_bias kernels on graph keys of their own (bit 5); a call without a sampling table runs on neutral records.  bias_dev == NULL:
// the _style entry, launch for launch
int ts_pixelcnn_generate_mixed_bias(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                    int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                    int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                    const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, const float *style,
                                    int style_rows, const float *bias_dev, int n_bias, const int32_t *bias_index_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}
// the same pass under a "repetition penalty" (talkshow_hip.h): rep_host n_rep (1 or B) records in slot order.  The records are copied into the
// Work in stream order ahead of the pass (kernel arguments, like the sampling table); the samplers are the sample_ctl_rep kernels on graph
// keys of their own (bit 6), which keep every slot's history in Work::rep_ring; a call without a sampling table runs on neutral records, a
// call without tables on an index of -1.  rep_host == NULL: the _bias entry, launch for launch
int ts_pixelcnn_generate_mixed_repeat(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                      int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                      int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                      const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, const float *style,
                                      int style_rows, const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                      const ts_repeat *rep_host, int n_rep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

// the same pass with "alternatives" (talkshow_hip.h): the record of the four outputs, (B,H_max,2,n) and (B,H_max,2).  The samplers are the
// sample_ctl_alt kernels on graph keys of their own (bit 9, n above it); a call without a table runs on neutral records, one without records
// on windows of 0, one without tables on an index of -1.  alt == NULL: the _repeat entry, launch for launch
int ts_pixelcnn_generate_alt(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                   int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                   int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                   const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, const float *style,
                                   int style_rows, const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                   const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.alt = alt;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

// the same pass under "guidance" (talkshow_hip.h): guide_host (B,) the shadow's slot of every clip slot or -1, guide_scale_host (B,).  Roles
// and scales are copied into the Work in stream order ahead of the pass (kernel arguments); the samplers are the sample_ctl_guide kernels
// on graph keys of their own (bit 8); a call without a sampling table runs on neutral records.  guide_host == NULL: the _repeat entry,
// launch for launch
int ts_pixelcnn_generate_guided(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                                     int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                                     int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                                     const int32_t *given_rows_host, const int32_t *given_rows_dev, const uint8_t *keep, const float *style,
                                     int style_rows, const float *bias_dev, int n_bias, const int32_t *bias_index_host,
                                     const ts_repeat *rep_host, int n_rep, const int32_t *guide_host, const float *guide_scale_host,
                                     void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host, o.keep = keep;
    o.style = style, o.style_rows = style_rows, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.guide_host = guide_host, o.guide_scale_host = guide_scale_host;
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, o, (hipStream_t)stream);
}

}  // extern "C"

// The body of every ts_pixelcnn_generate_mixed* entry: each fills `o` with its own arguments, so an absent keyword is null here and costs no
// launch, no buffer and no bit of a graph key.  (given_rows_dev is not passed on: the table travels as kernel arguments from the host copy.)
int ts::pixelcnn_generate_mixed(ts_pixelcnn *p, const float *aud, const MixedPass &a, const MixedOpts &o, hipStream_t s) {
    PixTapScope taps;
    const int B = a.B, H_max = a.rows, mode = a.mode;
    if (!p || (!a.ids && !o.style) || !aud || !a.lens_host || !a.lens_dev || !a.codes) return fail("ts_pixelcnn_generate_mixed: null argument");
    if (B < 1 || H_max < 1) return fail("ts_pixelcnn_generate_mixed: bad shape");
    TS_TRY(mixed_style_rows_check("ts_pixelcnn_generate_mixed", "H_max", o, H_max));
    const bool tracked = o.style && o.style_rows > 1;   // H_max == 1: one row per clip either way
    if (mode != TS_SAMPLE_GREEDY && mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX) return fail("ts_pixelcnn_generate_mixed: bad mode");
    if (mode == TS_SAMPLE_UNIFORMS && !a.uniforms) return fail("ts_pixelcnn_generate_mixed: uniforms required");
    std::vector<int> hrows(B);
    for (int b = 0; b < B; ++b) {
        if (a.lens_host[b] < 4) return fail("ts_pixelcnn_generate_mixed: clip " + std::to_string(b) + " is shorter than 4 frames (one code row)");
        if (b > 0 && a.lens_host[b] > a.lens_host[b - 1])
            return fail("ts_pixelcnn_generate_mixed: lengths must be non-increasing (clip " + std::to_string(b) + " is longer than the one before it)");
        hrows[b] = a.lens_host[b] >> 2;
        if (hrows[b] > H_max) return fail("ts_pixelcnn_generate_mixed: clip " + std::to_string(b) + " has more code rows than H_max");
    }
    SamplerTables t;
    TS_TRY(t.build(o, B, p->V, mode, a.lens_host,
                   {"ts_pixelcnn_generate_mixed_ctl", "ts_pixelcnn_generate_mixed_bias", "ts_pixelcnn_generate_mixed_repeat",
                    "ts_pixelcnn_generate_mixed_keep", "ts_pixelcnn_generate_mixed_given", "ts_pixelcnn_generate_guided",
                    "ts_pixelcnn_generate_alt"}));
    ts_ctx *ctx = p->ctx;
    ts_pixelcnn::Work *w = &p->work(s);
    TS_TRY(ensure_work(p, w, B, H_max));
    TS_TRY(stage_sampler_tables(p, w, t, o, s));
    TS_TRY(audio_terms(p, w, aud, B, H_max, s));
    if (tracked) {   // sized with the Work's clip capacity, so it moves only when ensure_work has dropped the graphs that read it
                     // (its size follows capB alone, and no graph reads it before its first allocation)
        TS_TRY(w->style_int.ensure((size_t)p->NL * CHUNK_ROWS * w->capB * 2 * p->D * sizeof(float)));
    } else if (o.style) {
        TS_TRY(class_rows_style(p, w, o.style, B, s));
    } else {
        TS_TRY(class_rows(p, w, a.ids, B, s));
    }
    {   // the clips' Philox subsequences, in a Work buffer (what the captured samplers read): the caller's table, or 0 .. B-1
        MiscScope ms(ctx, s);
        if (a.clip_index) TS_HIP(hipMemcpyAsync(w->clip_tab.p, a.clip_index, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        else TS_HIP(launch_iota_i64(static_cast<int64_t *>(w->clip_tab.p), B, 0, s));
    }
    TS_TRY(run_mixed(p, w, a, o, hrows, p->use_graph && !ctx->prof.on, s));
    MiscScope ms(ctx, s);
    TS_HIP(launch_mask_codes(a.codes, B, H_max, a.lens_dev, s));   // rows at or beyond a clip's own H_b (surplus rows, rows never run): -1
    if (o.logprob) TS_HIP(launch_mask_logprob(o.logprob, B, H_max, a.lens_dev, s));   // and their log-probabilities: 0
    if (o.alt)   // and their alternatives: -1, 0, 0, -1
        TS_HIP(launch_mask_alt(o.alt->codes_dev, o.alt->logprob_dev, o.alt->entropy_dev, o.alt->rank_dev, o.alt->n, B, H_max, a.lens_dev, s));
    return 0;
}

extern "C" {

int ts_pixelcnn_generate_mixed(ts_pixelcnn *p, const int64_t *label, const float *aud, const int32_t *lens_host, const int32_t *lens_dev,
                               int B, int H_max, int mode, const float *uniforms, uint64_t seed, const int64_t *clip_index,
                               int64_t *codes, void *stream) {
    return pixelcnn_generate_mixed(p, aud, {label, lens_host, lens_dev, B, H_max, mode, uniforms, seed, clip_index, codes}, MixedOpts(), (hipStream_t)stream);
}

int ts_pixelcnn_generate_ctl(ts_pixelcnn *p, const int64_t *label, const float *aud, int B, int H, int mode,
                             const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes, float *logits,
                             const int64_t *pre_codes, const float *pre_aud, int H0, const ts_sampling *ctl_host, int n_ctl, void *stream) {
    return ts_pixelcnn_generate_lp(p, label, aud, B, H, mode, uniforms, seed, clip0, codes, logits, pre_codes, pre_aud, H0, ctl_host, n_ctl,
                                   nullptr, stream);
}

// ts_pixelcnn_generate_ctl with a log-probability output (B,H,2) over the generated (teacher forced: the given) rows; NULL: that entry
int ts_pixelcnn_generate_lp(ts_pixelcnn *p, const int64_t *label, const float *aud, int B, int H, int mode,
                            const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes, float *logits,
                            const int64_t *pre_codes, const float *pre_aud, int H0, const ts_sampling *ctl_host, int n_ctl, float *logprob,
                            void *stream) {
    PixTapScope taps;
    if (!p || !label || !aud || !codes) return fail("ts_pixelcnn_generate: null argument");
    if (B < 1 || H < 1 || H0 < 0) return fail("ts_pixelcnn_generate: bad shape");
    if (mode < 0 || mode > TS_TEACHER_FORCED) return fail("ts_pixelcnn_generate: bad mode");
    if (mode == TS_SAMPLE_UNIFORMS && !uniforms) return fail("ts_pixelcnn_generate: uniforms required");
    if (H0 > 0 && (!pre_codes || !pre_aud)) return fail("ts_pixelcnn_generate: prefix pointers required");
    const char *who = "ts_pixelcnn_generate_ctl";
    MixedOpts o;   // a one-shot call takes the table alone
    o.ctl_host = ctl_host, o.n_ctl = n_ctl;
    SamplerTables t;
    TS_TRY(t.build(o, B, p->V, mode, nullptr, sampler_names(who)));
    hipStream_t s = (hipStream_t)stream;
    ts_ctx *ctx = p->ctx;
    const int Htot = H0 + H, AD = p->AD;
    ts_pixelcnn::Work *w = &p->work(s);
    TS_TRY(ensure_work(p, w, B, Htot));
    TS_TRY(stage_sampler_tables(p, w, t, o, s));

    // eager launches remain for the instrumented / logits-returning / teacher-forced paths (teacher forced with log-probabilities too: it
    // runs the horizontal stack, see need_h in run_rows, as eager launches)
    const bool graph = p->use_graph && !ctx->prof.on && !logits && mode != TS_TEACHER_FORCED;
    RunCfg c = one_shot_cfg(B, H, H0, mode, uniforms, seed, clip0, codes, logits, w);
    bind_sampler_tables(c, w, o);

    const float *aud_all = aud;
    if (H0 > 0) {
        const size_t f = sizeof(float);
        TS_HIP(hipMemcpy2DAsync(w->aud_all.f(), (size_t)Htot * AD * f, pre_aud, (size_t)H0 * AD * f, (size_t)H0 * AD * f,
                                B, hipMemcpyDeviceToDevice, s));
        TS_HIP(hipMemcpy2DAsync(w->aud_all.f() + (size_t)H0 * AD, (size_t)Htot * AD * f, aud, (size_t)H * AD * f,
                                (size_t)H * AD * f, B, hipMemcpyDeviceToDevice, s));
        aud_all = w->aud_all.f();
    }
    TS_TRY(audio_terms(p, w, aud_all, B, Htot, s));
    TS_TRY(class_rows(p, w, label, B, s));
    // known codes: the continuity prefix, and every position when teacher forced
    if (H0 > 0 || mode == TS_TEACHER_FORCED) {
        MiscScope ms(ctx, s);
        int64_t *tf = static_cast<int64_t *>(w->tfcodes.p);
        const size_t e = sizeof(int64_t);
        if (H0 > 0)
            TS_HIP(hipMemcpy2DAsync(tf, (size_t)Htot * 2 * e, pre_codes, (size_t)H0 * 2 * e, (size_t)H0 * 2 * e, B,
                                    hipMemcpyDeviceToDevice, s));
        if (mode == TS_TEACHER_FORCED)
            TS_HIP(hipMemcpy2DAsync(tf + (size_t)H0 * 2, (size_t)Htot * 2 * e, codes, (size_t)H * 2 * e,
                                    (size_t)H * 2 * e, B, hipMemcpyDeviceToDevice, s));
        TS_HIP(launch_i64_to_i32(tf, w->tok32.i(), (long)B * Htot * 2, s));
    }
    const ts_pixelcnn::Work::Key key = std::make_tuple(B, H, H0, mode, 0, sampler_bits(c, logprob));
    // A shape without a whole-call graph runs as chunk graphs (two or three small captures that serve every clip length) until it is
    // hot (Work::hot: pinned by ts_pixelcnn_prepare, or its third sighting among the last 16 one-shot calls of this stream); then it gets
    // its own whole-call graph (one replay per call: the serving loops, bench.py).  The cache is bounded either way.
    if (graph && H0 == 0 && H > CHUNK_ROWS && !w->graphs.count(key) && (tapping() || !w->hot(key)))   // (a tapped pass is no sighting)
        return run_chunked(p, w, B, H, mode, uniforms, seed, clip0, codes, c.ctl, logprob, s);
    return run_rows(p, c, 0, Htot, graph, key, uniforms, codes, logprob, s);
}

int ts_pixelcnn_generate(ts_pixelcnn *p, const int64_t *label, const float *aud, int B, int H, int mode,
                         const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes, float *logits,
                         const int64_t *pre_codes, const float *pre_aud, int H0, void *stream) {
    return ts_pixelcnn_generate_ctl(p, label, aud, B, H, mode, uniforms, seed, clip0, codes, logits, pre_codes, pre_aud, H0, nullptr, 0, stream);
}

// Captures (without running anything) the whole-call graph of a one-shot shape on `stream` and pins it: the first real call of that
// shape is already a single replay, and the graph is never evicted.  Serving hosts call this for their pass shapes at start-up
// (bench.py's warm()); nothing in the reference corresponds (it has no graphs).
int ts_pixelcnn_prepare(ts_pixelcnn *p, int B, int H, int mode, void *stream) {
    if (!p) return fail("ts_pixelcnn_prepare: null argument");
    if (B < 1 || H < 1) return fail("ts_pixelcnn_prepare: bad shape");
    if (mode != TS_SAMPLE_GREEDY && mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX) return fail("ts_pixelcnn_prepare: bad mode");
    TS_HIP(hipSetDevice(p->ctx->device));
    if (!p->use_graph) return 0;                                   // TS_NO_GRAPH: eager launches, nothing to prepare
    hipStream_t s = (hipStream_t)stream;
    ts_pixelcnn::Work *w = &p->work(s);
    TS_TRY(ensure_work(p, w, B, H));
    const ts_pixelcnn::Work::Key key = std::make_tuple(B, H, 0, mode, 0, 0);
    if (!w->pinned.count(key) && w->pinned.size() >= ts_pixelcnn::Work::PIN_CAP) return fail("ts_pixelcnn_prepare: too many pinned shapes on this stream");
    RunCfg c = one_shot_cfg(B, H, 0, mode, nullptr, 0, 0, nullptr, nullptr, w);
    TS_TRY(run_rows(p, c, 0, H, true, key, nullptr, nullptr, nullptr, s, /*capture_only=*/true));
    w->pinned.insert(key);
    return 0;
}

// ---- streaming generation (reference: the pre_latents / pre_audio prefix of gated_pixelcnn_v2.py:158-165
// and its caller smplx_body_pixel.py:260-269,291-304, which recompute the whole prefix for every chunk) --------------------
int ts_pixelcnn_stream_open(ts_pixelcnn *p, const int64_t *label, int B, int max_chunk_rows, ts_pixelcnn_stream **out) {
    if (!p || !label || !out) return fail("ts_pixelcnn_stream_open: null argument");
    if (B < 1 || max_chunk_rows < 1) return fail("ts_pixelcnn_stream_open: bad shape");
    TS_HIP(hipSetDevice(p->ctx->device));
    std::unique_ptr<ts_pixelcnn_stream> st(new ts_pixelcnn_stream());
    st->p = p;
    st->B = B;
    st->max_rows = max_chunk_rows;
    // everything is allocated here, once: growing a buffer later would drop the row cache it holds
    TS_TRY(ensure_work(p, &st->w, B, std::max(max_chunk_rows, 4)));
    // a step's given block is staged whole ((B,Hc,2) with Hc up to max_chunk_rows), where a one-shot pass stages CHUNK_ROWS rows at a time
    TS_TRY(st->w.given_int.ensure((size_t)B * std::max(max_chunk_rows, CHUNK_ROWS) * 2 * sizeof(int64_t)));
    st->rep_from.assign(B, ts_pixelcnn_stream::REP_NONE);
    TS_TRY(st->label.ensure((size_t)B * sizeof(int64_t)));
    // (not hipMemcpy: another thread may be capturing a graph while this one opens a session)
    TS_HIP(copy_and_wait(st->label.p, label, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice));
    *out = st.release();
    return 0;
}

void ts_pixelcnn_stream_close(ts_pixelcnn_stream *st) { delete st; }

int64_t ts_pixelcnn_stream_rows(const ts_pixelcnn_stream *st) { return st ? st->rows : -1; }

}  // extern "C"

namespace {
// ---- "session pairs" (talkshow_hip.h): the session's side of ts_pixelcnn_stream_pair_check ---------------------------------------------
int64_t stream_slot_rows(const ts_pixelcnn_stream *st, int b) { return st->rows - (st->restarted ? st->origin[b] : 0); }
// the serials as the rule reads them: a step since the call that set them makes every slot stale
std::vector<int32_t> stream_fresh(const ts_pixelcnn_stream *st) {
    if (st->fresh.empty() || st->fresh_at != st->rows) return std::vector<int32_t>(st->B, 0);
    return st->fresh;
}
// what a restart or a load of `slots` checks of the pairs before anything is launched: 0, or the one-sided refusal
int stream_touch_check(const ts_pixelcnn_stream *st, const int32_t *slots, int n) {
    if (st->n_pairs == 0) return 0;
    std::vector<int64_t> rows(st->B);
    for (int b = 0; b < st->B; ++b) rows[b] = stream_slot_rows(st, b);
    return ts_pixelcnn_stream_pair_check(st->B, st->rows, st->pair_of.data(), rows.data(), stream_fresh(st).data(), slots, nullptr, nullptr, n);
}
// behind a restart or a load that was queued: the listed slots' pairs are dissolved (both slots were listed), their serial is the call's
void stream_touched(ts_pixelcnn_stream *st, const int32_t *slots, int n) {
    if (st->fresh.empty() || st->fresh_at != st->rows) st->fresh.assign(st->B, 0);
    st->fresh_at = st->rows;
    ++st->serial;
    for (int i = 0; i < n; ++i) {
        const int b = slots[i];
        st->fresh[b] = st->serial;
        if (st->n_pairs > 0 && st->pair_of[b] >= 0) st->pair_of[b] = -1, st->pair_scale[b] = 0.0f, --st->n_pairs;
    }
}

// The body of the step entries: `o_in` holds what ts_pixelcnn_stream_step_ctl brought (the fields of a mixed pass that a session takes: no
// mask of kept positions, no style track, no poses), so an absent piece is null here and costs no launch, no buffer and no bit of the
// graph key; a session with pairs adds its guide table and the step's scales (scale_host (B,), read at primaries; NULL: the stored ones).
// Everything is checked before anything is launched and before st->rows moves.
int stream_step(ts_pixelcnn_stream *st, const float *aud, int Hc, int mode, const float *uniforms, uint64_t seed, int64_t clip0,
                int64_t *codes, const MixedOpts &o_in, hipStream_t s, const float *scale_host = nullptr) {
    PixTapScope taps;
    if (!st || !aud || !codes) return fail("ts_pixelcnn_stream_step: null argument");
    if (Hc < 1) return fail("ts_pixelcnn_stream_step: empty chunk");
    if (Hc > st->max_rows) return fail("ts_pixelcnn_stream_step: chunk longer than max_chunk_rows given to ts_pixelcnn_stream_open");
    if (mode != TS_SAMPLE_GREEDY && mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX)
        return fail("ts_pixelcnn_stream_step: bad mode");
    if (mode == TS_SAMPLE_UNIFORMS && !uniforms) return fail("ts_pixelcnn_stream_step: uniforms required");
    if (st->rows + Hc > (1l << 30)) return fail("ts_pixelcnn_stream_step: row counter overflow");
    ts_pixelcnn *p = st->p;
    ts_ctx *ctx = p->ctx;
    ts_pixelcnn::Work *w = &st->w;
    const int B = st->B, r0 = (int)st->rows;
    const char *who = "ts_pixelcnn_stream_step_ctl";
    const std::vector<int32_t> lens(B, 4 * Hc);   // the rules of the mixed entry, on a pass of B clips of Hc rows
    MixedOpts o = o_in;
    std::vector<float> scales;
    if (st->n_pairs > 0) {   // "session pairs": roles and scales are kernel arguments of the guided samplers, checked last as in a pass
        scales = st->pair_scale;
        for (int b = 0; scale_host && b < B; ++b)
            if (st->pair_of[b] >= 0) scales[b] = scale_host[b];
        o.guide_host = st->pair_of.data(), o.guide_scale_host = scales.data();
    }
    SamplerTables t;
    TS_TRY(t.build(o, B, p->V, mode, lens.data(), sampler_names(who)));
    constexpr int32_t REP_NONE = ts_pixelcnn_stream::REP_NONE;
    std::vector<int32_t> rep_from(B, REP_NONE);   // the session's table behind this step, kept only if the step is queued
    for (size_t b = 0; b < t.rep.size(); ++b)
        if (t.rep[b].window > 0) t.rep[b].from_row = rep_from[b] = st->rep_from[b] != REP_NONE ? st->rep_from[b] : r0;
    for (int b = 0; o.guide_host && b < B; ++b)   // a shadow's ring is never written: it has no run of penalised rows
        if (o.guide_host[b] >= 0) rep_from[o.guide_host[b]] = REP_NONE;
    for (int32_t &g : t.given_rows) g += r0;   // the table the samplers read holds absolute bounds: clip b is forced at positions below 2 (r0 + g_b)
    if (r0 == 0 && !o.style && !st->cr_ready) TS_TRY(class_rows(p, w, static_cast<const int64_t *>(st->label.p), B, s));
    if (o.style) TS_TRY(class_rows_style(p, w, o.style, B, s));   // CR stays as written until a later step brings other rows
    RunCfg c = ring_cfg(w, B, r0, Hc, mode, seed, clip0);
    c.audio_from(w);   // a step's audio terms are the Work's whole buffers
    TS_TRY(stage_sampler_tables(p, w, t, o, s));
    bind_sampler_tables(c, w, o);
    c.given_stage = true;   // a step's given block is staged whole
    if (st->restarted) {   // "slot restart": the origins, and every slot's Philox clip index as this step sees it (kernel arguments)
        std::vector<int64_t> clips(B);
        for (int b = 0; b < B; ++b) clips[b] = st->clip_index[b] >= 0 ? st->clip_index[b] : clip0 + b;
        MiscScope ms(ctx, s);
        TS_HIP(launch_put_words(static_cast<int *>(w->clip_tab.p), reinterpret_cast<const int *>(clips.data()), 2l * B, s));
        c.clip_table = static_cast<const int64_t *>(w->clip_tab.p);
        c.row_origin = static_cast<const int32_t *>(st->row_origin.p);
    }
    TS_TRY(audio_terms(p, w, aud, B, Hc, s));
    const bool graph = p->use_graph && !ctx->prof.on;
    TS_TRY(run_rows(p, c, r0, r0 + Hc, graph, std::make_tuple(B, Hc, 1000 + ring_phase(r0), mode, 0, sampler_bits(c, o.logprob)), uniforms, codes,
                    o.logprob, s));
    st->rep_from.swap(rep_from);
    st->last_clip0 = clip0;
    st->rows += Hc;
    return 0;
}
}  // namespace

extern "C" {

int ts_pixelcnn_stream_step(ts_pixelcnn_stream *st, const float *aud, int Hc, int mode, const float *uniforms, uint64_t seed,
                            int64_t clip0, int64_t *codes, void *stream) {
    return stream_step(st, aud, Hc, mode, uniforms, seed, clip0, codes, MixedOpts(), (hipStream_t)stream);
}

// ts_pixelcnn_stream_step under the per-clip sampling pieces of a mixed pass (talkshow_hip.h, "streaming sessions"); every optional
// argument NULL / 0: that entry, launch for launch and on its graph keys
int ts_pixelcnn_stream_step_ctl(ts_pixelcnn_stream *st, const float *aud, int Hc, int mode, const float *uniforms, uint64_t seed,
                                int64_t clip0, int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob,
                                const int64_t *given, const int32_t *given_rows_host, const float *style, const float *bias_dev,
                                int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host;
    o.style = style, o.style_rows = 1, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    return stream_step(st, aud, Hc, mode, uniforms, seed, clip0, codes, o, (hipStream_t)stream);
}

// ts_pixelcnn_stream_step_ctl plus "alternatives" for the step's rows (talkshow_hip.h); alt == NULL: that entry, exactly
int ts_pixelcnn_stream_step_alt(ts_pixelcnn_stream *st, const float *aud, int Hc, int mode, const float *uniforms, uint64_t seed,
                                int64_t clip0, int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob,
                                const int64_t *given, const int32_t *given_rows_host, const float *style, const float *bias_dev,
                                int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const ts_alt_out *alt,
                                void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host;
    o.style = style, o.style_rows = 1, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    o.alt = alt;
    return stream_step(st, aud, Hc, mode, uniforms, seed, clip0, codes, o, (hipStream_t)stream);
}

// ts_pixelcnn_stream_step_ctl plus the step's scales (talkshow_hip.h, "session pairs"): guide_scale_host (B,), read at primaries only;
// NULL: the stored scales — ts_pixelcnn_stream_step_ctl, exactly
int ts_pixelcnn_stream_step_guided(ts_pixelcnn_stream *st, const float *aud, int Hc, int mode, const float *uniforms, uint64_t seed,
                                   int64_t clip0, int64_t *codes, const ts_sampling *ctl_host, int n_ctl, float *logprob,
                                   const int64_t *given, const int32_t *given_rows_host, const float *style, const float *bias_dev,
                                   int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                                   const float *guide_scale_host, void *stream) {
    MixedOpts o;
    o.ctl_host = ctl_host, o.n_ctl = n_ctl, o.logprob = logprob;
    o.given = given, o.given_rows_host = given_rows_host;
    o.style = style, o.style_rows = 1, o.bias = bias_dev, o.n_bias = n_bias, o.bias_index_host = bias_index_host;
    o.rep_host = rep_host, o.n_rep = n_rep;
    return stream_step(st, aud, Hc, mode, uniforms, seed, clip0, codes, o, (hipStream_t)stream, guide_scale_host);
}

// Host only ("session pairs"): the rule on host tables.  guide (S,) the session's pair table, clip_rows (S,) the rows of every slot's
// current clip, fresh (S,) the serial of the restart or load that listed the slot with no step since, else 0.  shadow != NULL: the
// declaration of n pairs (primary[i], shadow[i], scale[i]).  shadow == NULL: a restart or a load that lists the n slots of `primary`.
int ts_pixelcnn_stream_pair_check(int S, int64_t rows, const int32_t *guide_host, const int64_t *clip_rows_host, const int32_t *fresh_host,
                                  const int32_t *primary, const int32_t *shadow, const float *scale, int n) {
    const std::string who = "session pairs: ";
    if (S < 1 || rows < 0 || !guide_host || !clip_rows_host || !fresh_host || !primary || (shadow && !scale)) return fail(who + "bad argument");
    if (n < 1) return fail(who + "no slot given");
    std::vector<int> mate(S, -1);   // the other slot of every paired slot
    for (int b = 0; b < S; ++b) {
        const int g = guide_host[b];
        if (g < -1 || g >= S || g == b) return fail(who + "bad argument");
        if (g >= 0) mate[b] = g, mate[g] = b;
    }
    auto in_range = [&](int i, int x) -> int {
        if (x >= 0 && x < S) return 0;
        return fail(who + "entry " + std::to_string(i) + ": slot " + std::to_string(x) + " is outside [0, S = " + std::to_string(S) + ")");
    };
    std::vector<char> listed(S, 0);
    if (!shadow) {   // a restart or a load: both slots of a pair, or neither
        for (int i = 0; i < n; ++i) {
            TS_TRY(in_range(i, primary[i]));
            listed[primary[i]] = 1;
        }
        for (int i = 0; i < n; ++i) {
            const int b = primary[i];
            if (mate[b] >= 0 && !listed[mate[b]])
                return fail(who + "slot " + std::to_string(b) + " is paired with slot " + std::to_string(mate[b]) + ": list both");
        }
        return 0;
    }
    for (int i = 0; i < n; ++i) {
        const int b = primary[i], g = shadow[i];
        TS_TRY(in_range(i, b));
        TS_TRY(in_range(i, g));
        const std::string sb = "slot " + std::to_string(b), sg = "slot " + std::to_string(g);
        if (b == g) return fail(who + sb + " names itself as its shadow");
        for (int x : {b, g}) {
            if (listed[x]) return fail(who + "slot " + std::to_string(x) + " is listed twice");
            if (mate[x] >= 0)
                return fail(who + "slot " + std::to_string(x) + " is paired with slot " + std::to_string(mate[x]) +
                            ": restart or load both to dissolve the pair");
        }
        listed[b] = listed[g] = 1;
        if (rows > 0 && (fresh_host[b] == 0 || fresh_host[b] != fresh_host[g]))
            return fail(who + sb + " and " + sg + " cannot pair at session row " + std::to_string(rows) +
                        ": a pair forms at session row 0 or behind the call that restarts or loads both slots, ahead of the next step");
        if (clip_rows_host[b] != clip_rows_host[g])
            return fail(who + sb + " holds a clip of " + std::to_string(clip_rows_host[b]) + " rows, " + sg + " one of " +
                        std::to_string(clip_rows_host[g]) + ": a shadow carries its primary's history from the clip's row 0");
        if (std::isnan(scale[i])) return fail(who + sb + ": the scale is NaN");
        if (std::isinf(scale[i])) return fail(who + sb + ": the scale is infinite");
        if (std::fabs(scale[i]) > 1e4f) return fail(who + sb + ": the scale exceeds 1e4 in magnitude");
    }
    return 0;
}

// "session pairs": n pairs declared behind an open, a restart or a load and ahead of the next step.  Host tables only: nothing is launched
int ts_pixelcnn_stream_pair(ts_pixelcnn_stream *st, const int32_t *primary, const int32_t *shadow, const float *scale, int n) {
    if (!st || !primary || !shadow || !scale) return fail("ts_pixelcnn_stream_pair: null argument");
    const int B = st->B;
    std::vector<int64_t> rows(B);
    for (int b = 0; b < B; ++b) rows[b] = stream_slot_rows(st, b);
    const std::vector<int32_t> none(B, -1);
    TS_TRY(ts_pixelcnn_stream_pair_check(B, st->rows, st->pair_of.empty() ? none.data() : st->pair_of.data(), rows.data(),
                                         stream_fresh(st).data(), primary, shadow, scale, n));
    if (st->pair_of.empty()) st->pair_of.assign(B, -1), st->pair_scale.assign(B, 0.0f);
    for (int i = 0; i < n; ++i) st->pair_of[primary[i]] = shadow[i], st->pair_scale[primary[i]] = scale[i];
    st->n_pairs += n;
    return 0;
}

// "session pairs": the session's table, (S,) as ts_guide_check takes it; returns the number of pairs, -1 on a null argument
int ts_pixelcnn_stream_pairs(const ts_pixelcnn_stream *st, int32_t *guide_out) {
    if (!st || !guide_out) return fail("ts_pixelcnn_stream_pairs: null argument") ? -1 : -1;
    for (int b = 0; b < st->B; ++b) guide_out[b] = st->pair_of.empty() ? -1 : st->pair_of[b];
    return st->n_pairs;
}

int64_t ts_pixelcnn_stream_captures(const ts_pixelcnn_stream *st) { return st ? st->w.captures : -1; }

// "slot restart" (talkshow_hip.h).  Everything is checked before anything is launched or any table moves.  The launches: the tables of
// the call as kernel arguments, slot_reset_kernel, and one style_rows launch per slot that brings a weight row — all ahead of the next
// step's replay and in no graph
int ts_pixelcnn_stream_restart(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, const int64_t *labels_host, const float *style_dev,
                               const int64_t *clip_index_host, void *stream) {
    const std::string who = "ts_pixelcnn_stream_restart: ";
    if (!st || !slots_host || !clip_index_host) return fail(who + "null argument");
    const int B = st->B;
    if (n < 1 || n > B) return fail(who + "n must be in [1, B = " + std::to_string(B) + "], got " + std::to_string(n));
    for (int i = 0; i < n; ++i)
        if (slots_host[i] < 0 || slots_host[i] >= B)
            return fail(who + "entry " + std::to_string(i) + ": slot " + std::to_string(slots_host[i]) + " is outside [0, B = " + std::to_string(B) + ")");
    if (!labels_host == !style_dev)
        return fail(who + "slot " + std::to_string(slots_host[0]) + ": " + (labels_host ? "both a label and a style row" : "neither a label nor a style row") +
                    " (a restarted clip takes exactly one of them)");
    ts_pixelcnn *p = st->p;
    std::vector<char> seen(B, 0);
    for (int i = 0; i < n; ++i) {
        const std::string slot = "slot " + std::to_string(slots_host[i]);
        if (seen[slots_host[i]]++) return fail(who + slot + " is listed twice");
        if (labels_host && (labels_host[i] < 0 || labels_host[i] >= p->NC))
            return fail(who + slot + ": label " + std::to_string(labels_host[i]) + " is outside [0, NC = " + std::to_string(p->NC) + ")");
        if (clip_index_host[i] < 0) return fail(who + slot + ": clip index " + std::to_string(clip_index_host[i]) + " is negative");
    }
    TS_TRY(stream_touch_check(st, slots_host, n));   // "session pairs": both slots of a pair, or neither
    TS_HIP(hipSetDevice(p->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    ts_pixelcnn::Work *w = &st->w;
    if (st->rows == 0 && !st->cr_ready)   // the labels given at open, as the first step would write them: the restarted slots' rows then replace theirs
        TS_TRY(class_rows(p, w, static_cast<const int64_t *>(st->label.p), B, s));
    MiscScope ms(p->ctx, s);
    if (!st->restarted) {   // the session's first restart: the tables exist from here on, every origin 0 in stream order
        TS_TRY(st->row_origin.ensure((size_t)B * sizeof(int32_t)));
        TS_TRY(st->restart_tab.ensure((size_t)2 * B * sizeof(int32_t)));
        const std::vector<int32_t> zeros(B, 0);
        TS_HIP(launch_put_words(static_cast<int *>(st->row_origin.p), zeros.data(), B, s));
    }
    std::vector<int32_t> tab(2 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) tab[i] = slots_host[i], tab[n + i] = labels_host ? (int32_t)labels_host[i] : 0;
    int32_t *tab_dev = static_cast<int32_t *>(st->restart_tab.p);
    TS_HIP(launch_put_words(tab_dev, tab.data(), 2l * n, s));
    SlotResetParams q;
    std::memset(&q, 0, sizeof(q));
    q.slots = tab_dev, q.labels = labels_host ? tab_dev + n : nullptr;
    q.n = n, q.B = B, q.row = (int)st->rows;
    q.D = p->D, q.NL = p->NL, q.NC = p->NC, q.R = 4;   // the ring of ring_cfg
    q.tok32 = w->tok32.i(), q.Q1 = w->Q1.f(), q.Q0 = w->Q0.f(), q.P = w->P.f(), q.CR = w->CR.f();
    q.bv = p->bv_all.f(), q.tables = p->cls_all.f();
    q.row_origin = static_cast<int32_t *>(st->row_origin.p);
    TS_HIP(launch_slot_reset(q, s));
    for (int i = 0; style_dev && i < n; ++i) {   // the "speaker style" rule in its order, on the slot's own rows of CR
        StyleRowsParams y;
        std::memset(&y, 0, sizeof(y));
        y.tables = p->cls_all.f();
        y.weights = style_dev + (size_t)i * p->NC;
        y.w_ld = p->NC;
        y.S = 1, y.NC = p->NC, y.W = 2 * p->D, y.NL = p->NL;
        y.r0 = 0, y.n = 1, y.slots = 1;
        y.out = w->CR.f() + (size_t)slots_host[i] * 2 * p->D;
        y.out_l_stride = (long)B * 2 * p->D;
        y.out_r_stride = 0;
        TS_HIP(launch_style_rows(y, s));
    }
    if (!st->restarted) st->origin.assign(B, 0), st->clip_index.assign(B, -1);
    if (st->slot_label.empty()) st->slot_label.assign(B, -1);
    st->restarted = st->cr_ready = true;
    for (int i = 0; i < n; ++i) {
        const int b = slots_host[i];
        st->origin[b] = (int32_t)st->rows;
        st->clip_index[b] = clip_index_host[i];
        if (labels_host) st->slot_label[b] = labels_host[i];   // ("slot state": the label the slot stands for; a weight row keeps the old one)
        st->rep_from[b] = ts_pixelcnn_stream::REP_NONE;   // a penalty starts from an empty history, as a one-shot clip's does
    }
    stream_touched(st, slots_host, n);
    return 0;
}

// ---- "slot state" (talkshow_hip.h): save a slot's state, load it into any slot -------------------------------------------------------------
int64_t ts_pixelcnn_slot_state_words(const ts_pixelcnn *p) { return p ? (int64_t)slot_state_layout(p->D, p->NL).words : -1; }

// Read-only on the session: the tables of the call as kernel arguments and slot_save_kernel, in stream order behind the previous step and
// in no graph.  Everything is checked before anything is launched.
int ts_pixelcnn_stream_save(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, float *state_dev, ts_slot_info *info_host, void *stream) {
    const std::string who = "ts_pixelcnn_stream_save: ";
    if (!st || !slots_host || !state_dev || !info_host) return fail(who + "null argument");
    const int B = st->B;
    if (n < 1 || n > B) return fail(who + "n must be in [1, B = " + std::to_string(B) + "], got " + std::to_string(n));
    for (int i = 0; i < n; ++i)
        if (slots_host[i] < 0 || slots_host[i] >= B)
            return fail(who + "entry " + std::to_string(i) + ": slot " + std::to_string(slots_host[i]) + " is outside [0, B = " + std::to_string(B) + ")");
    if (reinterpret_cast<uintptr_t>(state_dev) & 15) return fail(who + "the state block must be 16-byte aligned");
    ts_pixelcnn *p = st->p;
    TS_HIP(hipSetDevice(p->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    ts_pixelcnn::Work *w = &st->w;
    TS_TRY(st->state_tab.ensure((size_t)3 * B * sizeof(int32_t)));
    const int r = (int)st->rows;
    std::vector<int32_t> tab(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const int b = slots_host[i];
        const int32_t from = st->rep_from[b];
        const int hist = from == ts_pixelcnn_stream::REP_NONE ? -1 : std::min(r - from, SAMPLE_REP_RING);
        tab[i] = b, tab[n + i] = hist;
        ts_slot_info &o = info_host[i];
        o.D = p->D, o.NL = p->NL, o.NC = p->NC, o.V = p->V, o.version = TS_SLOT_STATE_VERSION, o.hist = hist;
        o.rows = st->rows - (st->restarted ? st->origin[b] : 0);
        o.clip_index = st->restarted && st->clip_index[b] >= 0 ? st->clip_index[b] : (st->last_clip0 >= 0 ? st->last_clip0 + b : -1);
        o.label = st->slot_label.empty() ? -1 : st->slot_label[b];
    }
    MiscScope ms(p->ctx, s);
    int32_t *tab_dev = static_cast<int32_t *>(st->state_tab.p);
    TS_HIP(launch_put_words(tab_dev, tab.data(), 2l * n, s));
    SlotSaveParams q;
    std::memset(&q, 0, sizeof(q));
    q.slots = tab_dev, q.hist = tab_dev + n;
    q.n = n, q.B = B, q.row = r;
    q.D = p->D, q.NL = p->NL, q.NC = p->NC, q.R = 4;
    q.tok32 = w->tok32.i(), q.Q1 = w->Q1.f(), q.Q0 = w->Q0.f(), q.P = w->P.f(), q.CR = w->CR.f(), q.bv = p->bv_all.f();
    q.rep_ring = static_cast<const int32_t *>(w->rep_ring.p);
    if (st->rows == 0 && !st->cr_ready)   // CR is the first step's to write: the rows it will hold are the open labels'
        q.open_labels = static_cast<const int64_t *>(st->label.p), q.tables = p->cls_all.f();
    q.state = state_dev;
    TS_HIP(launch_slot_save(q, s));
    return 0;
}

// Everything is checked before anything is launched or any table moves.  The launches: what a session's first restart does (the origin
// table), the tables of the call as kernel arguments, slot_load_kernel — ahead of the next step's replay and in no graph.
int ts_pixelcnn_stream_load(ts_pixelcnn_stream *st, const int32_t *slots_host, int n, const float *state_dev, int n_states,
                            const int32_t *state_index_host, const ts_slot_info *info_host, const int64_t *clip_index_host, void *stream) {
    const std::string who = "ts_pixelcnn_stream_load: ";
    if (!st || !slots_host || !state_dev || !info_host) return fail(who + "null argument");
    const int B = st->B;
    if (n < 1 || n > B) return fail(who + "n must be in [1, B = " + std::to_string(B) + "], got " + std::to_string(n));
    if (n_states < 1) return fail(who + "no state given");
    if (!state_index_host && n_states != 1 && n_states != n)
        return fail(who + std::to_string(n) + " slots but " + std::to_string(n_states) + " states (one for all listed slots, one each, or an index)");
    if (reinterpret_cast<uintptr_t>(state_dev) & 15) return fail(who + "the state block must be 16-byte aligned");
    for (int i = 0; i < n; ++i)
        if (slots_host[i] < 0 || slots_host[i] >= B)
            return fail(who + "entry " + std::to_string(i) + ": slot " + std::to_string(slots_host[i]) + " is outside [0, B = " + std::to_string(B) + ")");
    ts_pixelcnn *p = st->p;
    const long r = st->rows;
    std::vector<char> seen(B, 0);
    std::vector<int32_t> tab(3 * (size_t)n);
    std::vector<int64_t> clips(n);
    for (int i = 0; i < n; ++i) {
        const int b = slots_host[i];
        const std::string slot = "slot " + std::to_string(b);
        if (seen[b]++) return fail(who + slot + " is listed twice");
        const int k = state_index_host ? state_index_host[i] : (n_states == 1 ? 0 : i);
        if (k < 0 || k >= n_states) return fail(who + slot + ": state index " + std::to_string(k) + " is outside the " + std::to_string(n_states) + " states given");
        const ts_slot_info &o = info_host[k];
        if (o.version != TS_SLOT_STATE_VERSION)
            return fail(who + slot + ": the state has layout version " + std::to_string(o.version) + ", this library reads " + std::to_string(TS_SLOT_STATE_VERSION));
        if (o.D != p->D || o.NL != p->NL || o.NC != p->NC || o.V != p->V)
            return fail(who + slot + ": the state is of a network with (D, NL, NC, V) = (" + std::to_string(o.D) + ", " + std::to_string(o.NL) + ", " +
                        std::to_string(o.NC) + ", " + std::to_string(o.V) + "), this session's has (" + std::to_string(p->D) + ", " + std::to_string(p->NL) +
                        ", " + std::to_string(p->NC) + ", " + std::to_string(p->V) + ")");
        if (o.rows < 0 || o.rows > (1l << 30) || o.hist < -1 || o.hist > SAMPLE_REP_RING || o.hist > o.rows || o.label < -1 || o.label >= p->NC)
            return fail(who + slot + ": the state's record is damaged (rows " + std::to_string(o.rows) + ", history " + std::to_string(o.hist) + ", label " +
                        std::to_string(o.label) + ")");
        if (r < std::min<long>(o.rows, 3))
            return fail(who + slot + ": a clip of " + std::to_string(o.rows) + " rows cannot be loaded at session row " + std::to_string(r) +
                        " (the session's rows 0 to 2 leave out terms the clip's state holds: load at row min(rows, 3) or later)");
        clips[i] = clip_index_host ? clip_index_host[i] : o.clip_index;
        if (clips[i] < 0)
            return fail(who + slot + ": clip index " + std::to_string(clips[i]) + " is negative" + (clip_index_host ? "" : " (the state records none: give one)"));
        tab[i] = b, tab[n + i] = k, tab[2 * n + i] = (int32_t)(r - o.rows);
    }
    TS_TRY(stream_touch_check(st, slots_host, n));   // "session pairs": both slots of a pair, or neither
    TS_HIP(hipSetDevice(p->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    ts_pixelcnn::Work *w = &st->w;
    if (st->rows == 0 && !st->cr_ready)   // as a restart at row 0: the open labels' rows first, the loaded slots' rows then replace theirs
        TS_TRY(class_rows(p, w, static_cast<const int64_t *>(st->label.p), B, s));
    MiscScope ms(p->ctx, s);
    TS_TRY(st->state_tab.ensure((size_t)3 * B * sizeof(int32_t)));
    if (!st->restarted) {   // what the session's first restart does: the tables exist from here on, every origin 0 in stream order
        TS_TRY(st->row_origin.ensure((size_t)B * sizeof(int32_t)));
        TS_TRY(st->restart_tab.ensure((size_t)2 * B * sizeof(int32_t)));
        const std::vector<int32_t> zeros(B, 0);
        TS_HIP(launch_put_words(static_cast<int *>(st->row_origin.p), zeros.data(), B, s));
    }
    int32_t *tab_dev = static_cast<int32_t *>(st->state_tab.p);
    TS_HIP(launch_put_words(tab_dev, tab.data(), 3l * n, s));
    SlotLoadParams q;
    std::memset(&q, 0, sizeof(q));
    q.slots = tab_dev, q.index = tab_dev + n, q.origin = tab_dev + 2 * n;
    q.n = n, q.n_states = n_states, q.B = B, q.row = (int)r;
    q.D = p->D, q.NL = p->NL, q.R = 4;
    q.tok32 = w->tok32.i(), q.Q1 = w->Q1.f(), q.Q0 = w->Q0.f(), q.P = w->P.f(), q.CR = w->CR.f();
    q.rep_ring = static_cast<int32_t *>(w->rep_ring.p);
    q.row_origin = static_cast<int32_t *>(st->row_origin.p);
    q.state = state_dev;
    TS_HIP(launch_slot_load(q, s));
    if (!st->restarted) st->origin.assign(B, 0), st->clip_index.assign(B, -1);
    if (st->slot_label.empty()) st->slot_label.assign(B, -1);
    st->restarted = st->cr_ready = true;
    for (int i = 0; i < n; ++i) {
        const int b = slots_host[i];
        const ts_slot_info &o = info_host[tab[n + i]];
        st->origin[b] = tab[2 * n + i];
        st->clip_index[b] = clips[i];
        st->rep_from[b] = o.hist < 0 ? ts_pixelcnn_stream::REP_NONE : (int32_t)(r - o.hist);
        st->slot_label[b] = o.label;
    }
    stream_touched(st, slots_host, n);
    return 0;
}

// what the session's cached graphs hold: their number, and the skinny launches and flops recorded at their capture, summed
int ts_pixelcnn_stream_graph_stats(const ts_pixelcnn_stream *st, int64_t *graphs, int64_t *launches, double *flops) {
    if (!st) return fail("ts_pixelcnn_stream_graph_stats: null argument");
    long n = 0;
    double f = 0.0;
    for (const auto &kv : st->w.graph_stats) n += kv.second.first, f += kv.second.second;
    if (graphs) *graphs = (int64_t)st->w.graphs.size();
    if (launches) *launches = n;
    if (flops) *flops = f;
    return 0;
}

int64_t ts_pixelcnn_stream_slot_rows(const ts_pixelcnn_stream *st, int slot) {
    if (!st || slot < 0 || slot >= st->B) return -1;
    return st->rows - (st->restarted ? st->origin[slot] : 0);
}
}  // extern "C"
