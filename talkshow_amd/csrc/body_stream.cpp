// Seamless body sessions (talkshow_hip.h, "seamless sessions"): MFCC chunks of any length in, the poses of the one-shot call out, bit
// for bit.  No layer keeps state between pushes and no engine is touched: every window goes through ts_audioenc_forward and
// ts_vqvae_decode_pair as any clip does, and seamlessness comes from where the windows are cut —
//   * a row is kept only if its whole receptive field lies inside the window or beyond the clip's own edge (ENC_MARGIN_ROWS = 7 code
//     rows for the audio encoder, DEC_MARGIN_ROWS = 6 for the VQ decoders), so the zero padding at a window border never reaches it;
//   * a window starts at a multiple of 4 code rows, so the 4-row tiles of the Winograd-lowered stacks (conv_wino.hip), counted from a
//     window's row 0 at 75, 150 and 300 Hz, lie where the one-shot call has them;
//   * equal VALUES are not yet equal BITS under the lowering: an output row of an F(4,3) tile is summed from products that hold the
//     tile's other input rows (y0 from d0..d4, y1 and y2 from d1..d4, y3 from d1..d5; the terms beyond the three taps cancel exactly in
//     real numbers, not in fp32), so a lowered layer's rounding reaches to its tile's edge.  Through three lowered layers per stack at
//     75, 150 and 300 Hz that widens a pose frame's reach from 6 to at most 13 code rows either side: DEC_TILE_SLACK_ROWS = 7 more.
//     The audio encoder (256 channels) is direct under the default lowering rule (kernels.h::WINO_MIN_C) and needs none.  Where it IS
//     lowered (the test knob TS_CONV_WINO=1, or an encoder of WINO_MIN_C channels) the same walk through its three stacks widens an audio
//     row's reach from 4i-25 .. 4i+28 to 4i-53 .. 4i+56 frames, 14 code rows either side: ENC_TILE_SLACK_ROWS = 7 more, taken by a
//     session when kernels.h::wino_lowered says so for the encoder's width at open.
// The same arithmetic is restated in talkshow_amd/streaming.py (SeamlessPlan); tests/test_seamless_plan.py holds the two against each other
// through ts_debug_body_stream_plan.  The host keeps four counters; everything else is stream-ordered on the device.
#include <algorithm>

#include "host_common.h"

using namespace ts;

namespace {

constexpr int ENC_MARGIN_ROWS = 7, ENC_TILE_SLACK_ROWS = 7, DEC_MARGIN_ROWS = 6, DEC_TILE_SLACK_ROWS = 7, ALIGN_ROWS = 4;
constexpr int DEC_REACH_ROWS = DEC_MARGIN_ROWS + DEC_TILE_SLACK_ROWS;   // code rows either side a kept pose row needs inside its window
// frames a session can hold back between calls, at an encoder reach of `me` code rows: F - 4 w0 with 4 w0 >= 4 (A - me - 3) and
// 4 A >= 4 (F / 4 - me) >= F - 3 - 4 me, so at most 8 me + 15 (71 frames at 7 rows, 127 at 14)
constexpr int tail_cap_frames(int me) { return 8 * me + 16; }
// code rows a session can hold back between calls: A - v0 with v0 >= D - 13 - 3 and D >= A - 13
constexpr int RING_KEEP_ROWS = 32;

struct Counters {
    int64_t F = 0, A = 0, D = 0;
    bool flushed = false;
};

// The work of one call.  Frames and rows are absolute (counted from the clip's start)
struct CallPlan {
    Counters after;
    int64_t w0 = 0, enc_f0 = 0, enc_f1 = 0;   // encoder window: frames [enc_f0, enc_f1), enc_f0 = 4 w0; empty if no call is made
    int64_t A0 = 0, A1 = 0;                    // audio / code rows this call finalises
    int64_t v0 = 0, v1 = 0;                    // decoder window: code rows [v0, v1); empty if no call is made
    int64_t D0 = 0, D1 = 0;                    // code rows whose poses come out
    int64_t keep_frame0 = 0, keep_row0 = 0;    // what the next call can still read: frames from 4 w0_next, code rows from v0_next
};

inline int64_t align_down(int64_t x) { return x / ALIGN_ROWS * ALIGN_ROWS; }

// me: the encoder's reach in code rows, ENC_MARGIN_ROWS (+ ENC_TILE_SLACK_ROWS where the encoder is lowered)
CallPlan plan_call(const Counters &c, int t, bool flush, int me) {
    CallPlan p;
    const int64_t F = c.F + t, A = c.A, D = c.D;
    p.A0 = A;
    p.A1 = flush ? F / 4 : std::max(A, F / 4 - me);
    p.w0 = align_down(std::max<int64_t>(0, A - me));
    if (p.A1 > A) {
        p.enc_f0 = 4 * p.w0;
        p.enc_f1 = flush ? F : std::min(F, 4 * (p.A1 + me));
    }
    p.D0 = D;
    p.D1 = flush ? p.A1 : std::max(D, p.A1 - DEC_REACH_ROWS);
    if (p.D1 > D) {
        p.v0 = align_down(std::max<int64_t>(0, D - DEC_REACH_ROWS));
        p.v1 = std::min(p.A1, p.D1 + DEC_REACH_ROWS);
    }
    p.after.F = F, p.after.A = p.A1, p.after.D = p.D1, p.after.flushed = flush;
    p.keep_frame0 = 4 * align_down(std::max<int64_t>(0, p.A1 - me));
    p.keep_row0 = align_down(std::max<int64_t>(0, p.D1 - DEC_REACH_ROWS));
    return p;
}

}  // namespace

struct ts_body_stream {
    ts_convnet *ae = nullptr;
    ts_vqvae *vb = nullptr, *vh = nullptr;
    ts_pixelcnn_stream *pix = nullptr;
    int B = 0, max_frames = 0, max_rows = 0, aud_dim = 0, pose_dim = 0;
    // "guided sessions" (talkshow_hip.h): the chain runs S = B + n_shadow slots (the clips, then the shadows), the audio encoder E = B + n_a
    // MFCC streams (n_a: the shadows with audio of their own); slot_map (S,) int32 on the device: the encoder stream slot s hears.
    // A plain session has S = E = B and no map
    int S = 0, E = 0;
    bool guided = false;
    DevBuf slot_map;
    int enc_reach = ENC_MARGIN_ROWS, tail_cap = 0;   // code rows either side a kept audio row needs inside its window; frames of a tail half
    int win_cap = 0, ring_cap = 0;   // frames of the largest encoder window; code rows of the ring = of the largest decoder window
    Counters c;
    int64_t tail0 = 0;               // absolute frame of the tail's first row: 4 w0 of the next call
    int half = 0;                    // which half of the double buffer holds the tail
    bool broken = false;             // a device call failed after the chain had advanced: the counters no longer describe the device
    DevBuf tail[2], ring, win, feat, aud, lat[2], dec;
    ~ts_body_stream() {
        if (pix) ts_pixelcnn_stream_close(pix);
    }
    size_t bytes() const {
        return tail[0].bytes + tail[1].bytes + ring.bytes + win.bytes + feat.bytes + aud.bytes + lat[0].bytes + lat[1].bytes + dec.bytes +
               slot_map.bytes;
    }
};

namespace {

struct StepPieces {
    const ts_sampling *ctl_host;
    int n_ctl;
    float *logprob;
    const int64_t *given;
    const int32_t *given_rows_host;
    const float *style, *bias;
    int n_bias;
    const int32_t *bias_index_host;
    const ts_repeat *rep_host;
    int n_rep;
    bool guided = false;                  // the call came through a _guided entry: mfcc holds E streams, the pieces S slots
    const float *guide_scale = nullptr;   // (S,) host, read at primaries; NULL: the stored scales
};

int stream_launches(ts_body_stream *st, const CallPlan &p, const float *mfcc, int t, bool flush, int mode, const float *uniforms, uint64_t seed,
                    int64_t clip0, int64_t *codes_out, float *poses_out, const StepPieces &o, hipStream_t s);

// The body of push (mfcc, t >= 1) and flush (mfcc null, t = 0)
int stream_call(ts_body_stream *st, const char *who, const float *mfcc, int t, bool flush, int mode, const float *uniforms, uint64_t seed,
                int64_t clip0, int64_t *codes_out, float *poses_out, const StepPieces &o, hipStream_t s) {
    const std::string w(who);
    if (!st) return fail(w + ": null session");
    if (st->broken) return fail(w + ": an earlier call of this session failed on the device; close it");
    if (st->c.flushed) return fail(w + ": the session has been flushed (the clip has ended); open another");
    if (o.guided != st->guided)
        return fail(w + (st->guided ? ": the session was opened with shadows (ts_body_stream_open_guided): its calls are the _guided entries, which "
                                      "bring the MFCC block of its E streams"
                                    : ": the session was opened without shadows: its calls are ts_body_stream_push / _flush"));
    if (!flush) {
        if (!mfcc) return fail(w + ": null argument");
        if (t < 1) return fail(w + ": a push holds at least one MFCC frame, got " + std::to_string(t));
        if (t > st->max_frames)
            return fail(w + ": " + std::to_string(t) + " frames, more than max_chunk_frames = " + std::to_string(st->max_frames) +
                        " given to ts_body_stream_open");
        if (reinterpret_cast<uintptr_t>(mfcc) & 15) return fail(w + ": mfcc_dev must be 16-byte aligned");
        if (st->c.F + t > (1ll << 32)) return fail(w + ": frame counter overflow");
    }
    if (mode != TS_SAMPLE_GREEDY && mode != TS_SAMPLE_UNIFORMS && mode != TS_SAMPLE_PHILOX) return fail(w + ": bad mode");
    const CallPlan p = plan_call(st->c, t, flush, st->enc_reach);
    const int n = (int)(p.A1 - p.A0), n_pose = (int)(4 * (p.D1 - p.D0));
    if (n > 0 && !codes_out) return fail(w + ": the call runs " + std::to_string(n) + " code rows and codes_dev is null");
    if (n > 0 && (reinterpret_cast<uintptr_t>(codes_out) & 15)) return fail(w + ": codes_dev must be 16-byte aligned");
    if (n_pose > 0 && !poses_out) return fail(w + ": the call returns " + std::to_string(n_pose) + " pose frames and poses_dev is null");
    if (n > 0 && mode == TS_SAMPLE_UNIFORMS && !uniforms) return fail(w + ": uniforms required ((B, " + std::to_string(n) + ", 2))");
    // the sizes every launch below relies on; they follow from the plan's arithmetic for any history (tests/test_seamless_plan.py)
    const int n_tail = (int)(st->c.F - st->tail0), n_cat = n_tail + t;
    const int Tw = (int)(p.enc_f1 - p.enc_f0), Hw = (int)(p.v1 - p.v0);
    const int next0 = (int)(p.keep_frame0 - st->tail0), n_next = flush ? 0 : (int)(p.after.F - p.keep_frame0);
    const int64_t ring0 = Hw > 0 ? p.v0 : p.A0;   // the oldest ring row this call reads
    if (n > st->max_rows || n_tail < 0 || n_tail > st->tail_cap || n_next > st->tail_cap || Tw > st->win_cap || Tw > n_cat ||
        (Tw > 0 && p.enc_f0 != st->tail0) || next0 < 0 || Hw > st->ring_cap || p.A1 - ring0 > st->ring_cap || ring0 < p.A0 - RING_KEEP_ROWS)
        return fail(w + ": internal: the window plan left the session's buffers");

    // From here a failure may leave the device behind or ahead of the counters: the session is marked broken until the call has either
    // gone through or been REFUSED — it returned an error, the chain's row counter stands where the session's does and the runtime
    // reports no error, which is what a bad optional piece looks like (the chain checks them before its first launch)
    st->broken = true;
    const int rc = stream_launches(st, p, mfcc, t, flush, mode, uniforms, seed, clip0, codes_out, poses_out, o, s);
    if (rc != 0) {
        if (ts_pixelcnn_stream_rows(st->pix) == st->c.A && hipPeekAtLastError() == hipSuccess) st->broken = false;
        return rc;
    }
    st->broken = false;
    st->c = p.after;
    st->tail0 = p.keep_frame0;
    st->half ^= 1;
    return 0;
}

// The device part of a call whose plan `p` has been checked against the session's buffers
int stream_launches(ts_body_stream *st, const CallPlan &p, const float *mfcc, int t, bool flush, int mode, const float *uniforms, uint64_t seed,
                    int64_t clip0, int64_t *codes_out, float *poses_out, const StepPieces &o, hipStream_t s) {
    const int B = st->B, E = st->E, n = (int)(p.A1 - p.A0), n_pose = (int)(4 * (p.D1 - p.D0));
    const int n_tail = (int)(st->c.F - st->tail0), Tw = (int)(p.enc_f1 - p.enc_f0), Hw = (int)(p.v1 - p.v0);
    const int next0 = (int)(p.keep_frame0 - st->tail0), n_next = flush ? 0 : (int)(p.after.F - p.keep_frame0);
    const int64_t ring0 = Hw > 0 ? p.v0 : p.A0;
    // 1. [tail | chunk] -> the encoder window, and the next tail into the other half (the live half is not written: a call that fails below
    //    leaves the session where it was)
    TS_HIP(launch_stream_stage_mfcc(st->tail[st->half].f(), mfcc, st->win.f(), st->tail[st->half ^ 1].f(), E, n_tail, t, st->tail_cap, Tw,
                                    next0, n_next, s));
    // 2. the window through the audio encoder, its kept rows through the chain.  The chain checks the optional pieces before its own first
    //    launch and before its row counter moves
    if (n > 0 && st->guided) {   // E streams encoded once each, their kept rows spread to the S slots; the step runs under the session's pairs
        TS_TRY(ts_audioenc_forward(st->ae, st->win.f(), E, Tw, st->feat.f(), s));
        TS_HIP(launch_stream_spread_rows(st->feat.f(), st->aud.f(), static_cast<const int32_t *>(st->slot_map.p), st->S, E, Tw / 4,
                                         (int)(p.A0 - p.w0), n, st->aud_dim, s));
        TS_TRY(ts_pixelcnn_stream_step_guided(st->pix, st->aud.f(), n, mode, uniforms, seed, clip0, codes_out, o.ctl_host, o.n_ctl, o.logprob,
                                              o.given, o.given_rows_host, o.style, o.bias, o.n_bias, o.bias_index_host, o.rep_host, o.n_rep,
                                              o.guide_scale, s));
    } else if (n > 0) {
        TS_TRY(ts_audioenc_forward(st->ae, st->win.f(), B, Tw, st->feat.f(), s));
        TS_HIP(launch_stream_keep_rows(st->feat.f(), st->aud.f(), B, Tw / 4, (int)(p.A0 - p.w0), n, st->aud_dim, s));
        TS_TRY(ts_pixelcnn_stream_step_ctl(st->pix, st->aud.f(), n, mode, uniforms, seed, clip0, codes_out, o.ctl_host, o.n_ctl, o.logprob, o.given,
                                           o.given_rows_host, o.style, o.bias, o.n_bias, o.bias_index_host, o.rep_host, o.n_rep, s));
    }
    // 3. the codes into the ring; the decoder window out of ring + step, through both decoders; the kept frames to the caller.  A guided
    //    call's code block is (S, n, 2), clip-major with stride n: its first B * n entries are the clips', and only those are emitted
    if (n > 0 || Hw > 0)
        TS_HIP(launch_stream_emit(codes_out, static_cast<int64_t *>(st->ring.p), static_cast<int64_t *>(st->lat[0].p),
                                  static_cast<int64_t *>(st->lat[1].p), B, n, (int)p.A0, st->ring_cap, (int)ring0, Hw, s));
    if (Hw > 0) {
        TS_TRY(ts_vqvae_decode_pair(st->vb, st->vh, static_cast<int64_t *>(st->lat[0].p), static_cast<int64_t *>(st->lat[1].p), B, Hw,
                                    st->dec.f(), s));
        TS_HIP(launch_stream_keep_rows(st->dec.f(), poses_out, B, 4 * Hw, (int)(4 * (p.D0 - p.v0)), n_pose, st->pose_dim, s));
    }
    return 0;
}

}  // namespace

extern "C" {

}  // extern "C"

namespace {
// The body of both open entries: ids (S,) the labels of the chain's slots; MFCC tails, the encoder window and feat are sized for the E
// encoder streams, the chain session and its audio rows for S, the code ring, the latent columns and the decoders for the B clips
int stream_open(const char *who, ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const int64_t *ids, int B, int S, int E,
                int max_chunk_frames, ts_body_stream **out) {
    if (!ae || !pix || !vb || !vh || !ids || !out) return fail(std::string(who) + ": null argument");
    if (B < 1 || max_chunk_frames < 1 || max_chunk_frames > (1 << 20)) return fail(std::string(who) + ": bad shape");
    std::unique_ptr<ts_body_stream> st(new ts_body_stream());
    st->ae = ae, st->vb = vb, st->vh = vh;
    st->B = B, st->S = S, st->E = E, st->max_frames = max_chunk_frames;
    st->aud_dim = convnet_hidden(ae), st->pose_dim = vqvae_in_dim(vb) + vqvae_in_dim(vh);
    // a lowered encoder's rounding reaches further (see the head of this file); the rule networks are created under
    if (wino_lowered(0, 3, st->aud_dim, st->aud_dim, knobs().conv_wino)) st->enc_reach += ENC_TILE_SLACK_ROWS;
    // the most code rows one call can run: a push of t frames finalises at most t / 4 + 1 rows, a flush the enc_reach rows held back.
    // The chain session is opened for that count, so no call is split
    st->max_rows = std::max(st->enc_reach, max_chunk_frames / 4 + 1);
    st->tail_cap = tail_cap_frames(st->enc_reach);
    st->win_cap = st->tail_cap + max_chunk_frames;
    st->ring_cap = RING_KEEP_ROWS + st->max_rows;
    TS_TRY(ts_pixelcnn_stream_open(pix, ids, S, st->max_rows, &st->pix));   // selects the device
    // everything is allocated here, once: no call grows a buffer
    const size_t b = (size_t)B, e = (size_t)E;
    for (auto &h : st->tail) TS_TRY(h.ensure(e * st->tail_cap * 64 * sizeof(float)));
    TS_TRY(st->ring.ensure(b * st->ring_cap * 2 * sizeof(int64_t)));
    TS_TRY(st->win.ensure(e * st->win_cap * 64 * sizeof(float)));
    TS_TRY(st->feat.ensure(e * (st->win_cap / 4) * st->aud_dim * sizeof(float)));
    TS_TRY(st->aud.ensure((size_t)S * st->max_rows * st->aud_dim * sizeof(float)));
    for (auto &l : st->lat) TS_TRY(l.ensure(b * st->ring_cap * sizeof(int64_t)));
    TS_TRY(st->dec.ensure(b * 4 * st->ring_cap * st->pose_dim * sizeof(float)));
    *out = st.release();
    return 0;
}
}  // namespace

extern "C" {

int ts_body_stream_open(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const int64_t *ids, int B, int max_chunk_frames,
                        ts_body_stream **out) {
    return stream_open("ts_body_stream_open", ae, pix, vb, vh, ids, B, B, B, max_chunk_frames, out);
}

// "guided sessions" (talkshow_hip.h).  Everything is checked on the host before the session exists.  The launches: the slot map as kernel
// arguments and, where the shadows bring weight rows, the chain's restart of the shadow slots at row 0 — on `stream`, in no graph
int ts_body_stream_open_guided(ts_convnet *ae, ts_pixelcnn *pix, ts_vqvae *vb, ts_vqvae *vh, const int64_t *ids, int B, int n_shadow,
                               const int32_t *shadow_of, const int32_t *enc_of, const float *shadow_style, const float *scale_host,
                               int max_chunk_frames, void *stream, ts_body_stream **out) {
    const std::string who = "ts_body_stream_open_guided: ";
    if (!shadow_of || !enc_of || !scale_host) return fail(who + "null argument");
    if (B < 1 || n_shadow < 1 || n_shadow > B)
        return fail(who + "a session of " + std::to_string(B) + " clips holds 1 to " + std::to_string(B) + " shadows, got " + std::to_string(n_shadow));
    const int S = B + n_shadow;
    int E = B;
    std::vector<int32_t> map(S), prim(n_shadow), shad(n_shadow);
    for (int b = 0; b < B; ++b) map[b] = b;
    for (int k = 0; k < n_shadow; ++k) {
        const std::string sh = "shadow " + std::to_string(k);
        if (shadow_of[k] < 0 || shadow_of[k] >= B) return fail(who + sh + ": clip " + std::to_string(shadow_of[k]) + " is outside [0, B = " + std::to_string(B) + ")");
        if (k > 0 && shadow_of[k] <= shadow_of[k - 1])
            return fail(who + sh + ": the shadows stand in clip order, one per clip (clip " + std::to_string(shadow_of[k]) + " behind clip " +
                        std::to_string(shadow_of[k - 1]) + ")");
        if (enc_of[k] != -1 && enc_of[k] != E)
            return fail(who + sh + ": its encoder stream is -1 (the clip's) or the next stream of its own, " + std::to_string(E) + ", got " +
                        std::to_string(enc_of[k]));
        map[B + k] = enc_of[k] < 0 ? shadow_of[k] : E++;
        prim[k] = shadow_of[k], shad[k] = B + k;
    }
    ts_body_stream *st = nullptr;
    TS_TRY(stream_open("ts_body_stream_open_guided", ae, pix, vb, vh, ids, B, S, E, max_chunk_frames, &st));
    std::unique_ptr<ts_body_stream> hold(st);
    st->guided = true;
    hipStream_t s = (hipStream_t)stream;
    TS_TRY(st->slot_map.ensure((size_t)S * sizeof(int32_t)));
    TS_HIP(launch_put_words(static_cast<int *>(st->slot_map.p), map.data(), S, s));
    if (shadow_style) {   // a shadow's weight row, written as a restart at row 0 writes it (a one-hot row is the label bit for bit)
        std::vector<int64_t> clips(shad.begin(), shad.end());
        TS_TRY(ts_pixelcnn_stream_restart(st->pix, shad.data(), n_shadow, nullptr, shadow_style, clips.data(), stream));
    }
    TS_TRY(ts_pixelcnn_stream_pair(st->pix, prim.data(), shad.data(), scale_host, n_shadow));
    *out = hold.release();
    return 0;
}

void ts_body_stream_close(ts_body_stream *st) { delete st; }

int ts_body_stream_plan(const ts_body_stream *st, int t, int flush, int64_t *code_rows, int64_t *pose_frames) {
    if (!st || !code_rows || !pose_frames) return fail("ts_body_stream_plan: null argument");
    if (st->c.flushed) return fail("ts_body_stream_plan: the session has been flushed (the clip has ended)");
    if (flush ? t != 0 : (t < 1 || t > st->max_frames))
        return fail("ts_body_stream_plan: a push holds 1 .. max_chunk_frames = " + std::to_string(st->max_frames) + " frames and a flush 0, got " +
                    std::to_string(t));
    const CallPlan p = plan_call(st->c, t, flush != 0, st->enc_reach);
    *code_rows = p.A1 - p.A0;
    *pose_frames = 4 * (p.D1 - p.D0);
    return 0;
}

int ts_body_stream_push(ts_body_stream *st, const float *mfcc, int t, int mode, const float *uniforms, uint64_t seed, int64_t clip0,
                        int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                        const int32_t *given_rows_host, const float *style, const float *bias, int n_bias, const int32_t *bias_index_host,
                        const ts_repeat *rep_host, int n_rep, void *stream) {
    const StepPieces o{ctl_host, n_ctl, logprob, given, given_rows_host, style, bias, n_bias, bias_index_host, rep_host, n_rep};
    return stream_call(st, "ts_body_stream_push", mfcc, t, false, mode, uniforms, seed, clip0, codes, poses, o, (hipStream_t)stream);
}

int ts_body_stream_flush(ts_body_stream *st, int mode, const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes, float *poses,
                         const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given, const int32_t *given_rows_host,
                         const float *style, const float *bias, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep,
                         void *stream) {
    const StepPieces o{ctl_host, n_ctl, logprob, given, given_rows_host, style, bias, n_bias, bias_index_host, rep_host, n_rep};
    return stream_call(st, "ts_body_stream_flush", nullptr, 0, true, mode, uniforms, seed, clip0, codes, poses, o, (hipStream_t)stream);
}

// The existing entries on a session with shadows: mfcc (E, t, 64); uniforms, codes, logprob, given and every per-clip table for the S slots
// of the chain (the clips first); poses (B, ., pose_dim); guide_scale_host (S,) read at primaries, NULL: the stored scales
int ts_body_stream_push_guided(ts_body_stream *st, const float *mfcc, int t, int mode, const float *uniforms, uint64_t seed, int64_t clip0,
                               int64_t *codes, float *poses, const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given,
                               const int32_t *given_rows_host, const float *style, const float *bias, int n_bias,
                               const int32_t *bias_index_host, const ts_repeat *rep_host, int n_rep, const float *guide_scale_host, void *stream) {
    const StepPieces o{ctl_host, n_ctl, logprob, given, given_rows_host, style, bias, n_bias, bias_index_host, rep_host, n_rep, true, guide_scale_host};
    return stream_call(st, "ts_body_stream_push_guided", mfcc, t, false, mode, uniforms, seed, clip0, codes, poses, o, (hipStream_t)stream);
}

int ts_body_stream_flush_guided(ts_body_stream *st, int mode, const float *uniforms, uint64_t seed, int64_t clip0, int64_t *codes, float *poses,
                                const ts_sampling *ctl_host, int n_ctl, float *logprob, const int64_t *given, const int32_t *given_rows_host,
                                const float *style, const float *bias, int n_bias, const int32_t *bias_index_host, const ts_repeat *rep_host,
                                int n_rep, const float *guide_scale_host, void *stream) {
    const StepPieces o{ctl_host, n_ctl, logprob, given, given_rows_host, style, bias, n_bias, bias_index_host, rep_host, n_rep, true, guide_scale_host};
    return stream_call(st, "ts_body_stream_flush_guided", nullptr, 0, true, mode, uniforms, seed, clip0, codes, poses, o, (hipStream_t)stream);
}

int64_t ts_body_stream_frames_in(const ts_body_stream *st) { return st ? st->c.F : -1; }
int64_t ts_body_stream_code_rows(const ts_body_stream *st) { return st ? st->c.A : -1; }
int64_t ts_body_stream_pose_frames(const ts_body_stream *st) { return st ? 4 * st->c.D : -1; }
int64_t ts_body_stream_state_bytes(const ts_body_stream *st) { return st ? (int64_t)st->bytes() : -1; }
int64_t ts_body_stream_captures(const ts_body_stream *st) { return st ? ts_pixelcnn_stream_captures(st->pix) : -1; }
int ts_body_stream_lag_rows(const ts_body_stream *st) { return st ? st->enc_reach + DEC_REACH_ROWS : -1; }

// Host only (talkshow_hip_debug.h): one call of the plan on given counters
int ts_debug_body_stream_plan(const int64_t *state4, int t, int flush, int enc_lowered, int64_t *out14) {
    if (!state4 || !out14) return fail("ts_debug_body_stream_plan: null argument");
    Counters c;
    c.F = state4[0], c.A = state4[1], c.D = state4[2], c.flushed = state4[3] != 0;
    if (c.flushed) return fail("ts_debug_body_stream_plan: the session has been flushed");
    if (c.F < 0 || c.A < 0 || c.D < 0 || c.D > c.A || 4 * c.A > c.F || (flush ? t != 0 : t < 1))
        return fail("ts_debug_body_stream_plan: bad argument");
    const CallPlan p = plan_call(c, t, flush != 0, ENC_MARGIN_ROWS + (enc_lowered ? ENC_TILE_SLACK_ROWS : 0));
    const int64_t o[14] = {p.after.F, p.after.A, p.after.D, p.after.flushed, p.enc_f0, p.enc_f1, p.A0, p.A1, p.v0, p.v1, p.D0, p.D1,
                           p.keep_frame0, p.keep_row0};
    std::copy(o, o + 14, out14);
    return 0;
}

// Test aids (talkshow_hip_debug.h): the three staging kernels, one launcher call each on `stream`; the launchers own every shape check
int ts_debug_stream_stage_mfcc(const float *tail, const float *chunk, float *win, float *next, int B, int n_tail, int t, int cap, int Tw,
                               int next0, int n_next, void *stream) {
    if ((n_tail > 0 && !tail) || (Tw > 0 && !win) || (n_next > 0 && !next)) return fail("ts_debug_stream_stage_mfcc: null argument");
    TS_HIP(launch_stream_stage_mfcc(tail, chunk, win, next, B, n_tail, t, cap, Tw, next0, n_next, (hipStream_t)stream));
    return 0;
}
int ts_debug_stream_emit(const int64_t *codes, int64_t *ring, int64_t *lat_body, int64_t *lat_hand, int B, int n, int A, int RC, int v0, int Hw,
                         void *stream) {
    TS_HIP(launch_stream_emit(codes, ring, lat_body, lat_hand, B, n, A, RC, v0, Hw, (hipStream_t)stream));
    return 0;
}
// map_host (S,): the source stream of every slot, each in [0, E) (checked here: the kernel trusts its map); waits for the launch
int ts_debug_stream_spread_rows(const float *src, float *dst, const int32_t *map_host, int S, int E, int R, int r0, int n, int W, void *stream) {
    if (!map_host || S < 1) return fail("ts_debug_stream_spread_rows: bad argument");
    for (int i = 0; i < S; ++i)
        if (map_host[i] < 0 || map_host[i] >= E) return fail("ts_debug_stream_spread_rows: slot " + std::to_string(i) + " names stream " + std::to_string(map_host[i]));
    DevBuf map;
    TS_TRY(map.ensure((size_t)S * sizeof(int32_t)));
    TS_HIP(launch_put_words(static_cast<int *>(map.p), map_host, S, (hipStream_t)stream));
    TS_HIP(launch_stream_spread_rows(src, dst, static_cast<const int32_t *>(map.p), S, E, R, r0, n, W, (hipStream_t)stream));
    TS_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
int ts_debug_stream_keep_rows(const float *src, float *dst, int B, int R, int r0, int n, int W, void *stream) {
    TS_HIP(launch_stream_keep_rows(src, dst, B, R, r0, n, W, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
