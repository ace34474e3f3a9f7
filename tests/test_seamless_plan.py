"""The window plan of the seamless body sessions (`talkshow_amd/streaming.py::SeamlessPlan`), without a GPU.

Cover:  over random schedules every audio row and every pose frame is produced exactly once and in order, every window starts at a
        multiple of 4 code rows and holds the margins, the outputs sum to 4 * (T // 4), and what a session retains is bounded.
Reach:  the receptive fields the two margins stand for, measured on the oracle's networks (one NaN in, which outputs turn NaN): exactly
        4i-25 .. 4i+28 MFCC frames per audio row and t//4-6 .. t//4+6 code rows per pose frame — the constants are neither short nor
        padded, and a plan with either margin one lower keeps an output that reads beyond its window.  The decoders' third constant,
        DEC_TILE_SLACK_ROWS, is how much further the ROUNDING of their Winograd-lowered stacks reaches (to the tile edges): the walk
        `dec_rounding_cone`, which gives the measured cone for direct layers, gives 13 rows for lowered ones.
Values: the plan's windows through the oracle's networks against the one call, atol 5e-6 (CPU convolutions of different lengths differ
        by rounding: 8.9e-7 measured with the right margin at output scale 1.7, 3.2e-5 with the encoder margin one short; the decoder is
        exact with the right margin, 7.8e-4 one short).
Two restatements: the C++ plan behind the native session (`ts_debug_body_stream_plan`) equals `SeamlessPlan` call for call.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from talkshow_amd import streaming as S
from talkshow_amd import synth

ENC_CONE = (-25, 28)      # MFCC frames audio row i reads, relative to 4 i (measured below)
DEC_CONE = (-6, 6)        # code rows pose frame t reads, relative to t // 4 (measured below)


def dec_rounding_cone(t):
    """Code rows [lo, hi] whose VALUES can reach the BITS of pose frame t when every k = 3 stack of a decoder is Winograd-lowered
    (csrc/conv_wino.hip: F(4,3), tiles of 4 rows counted from row 0; y0 is summed from products holding d0..d4, y1 and y2 d1..d4, y3
    d1..d5, with d_k = x[4q - 1 + k]): the receptive field of `oracle.torch_port.vqvae_decode` walked backwards with every lowered layer
    reaching to its tile's edge.  With direct layers (tile = None) the walk gives DEC_CONE, which the NaN test below measures."""
    def layer(a, b, tiled):
        if not tiled:
            return a - 1, b + 1
        return (a - 1 if a % 4 == 0 else a - a % 4), (b + 1 if b % 4 == 3 else b - b % 4 + 3)

    def up(a, b):          # ConvTranspose1d(k = 4, stride 2, padding 1): out[o] reads in[ceil((o - 2) / 2) .. floor((o + 1) / 2)]
        return -((2 - a) // 2), (b + 1) // 2

    def walk(tiled):
        a = b = t
        for stage in range(3):                     # _dec_3 at 300 Hz, _up_3, _dec_2 at 150 Hz, _up_2, _dec_1 at 75 Hz
            for _ in range(3):
                a, b = layer(a, b, tiled)
            if stage < 2:
                a, b = up(a, b)
        return a, b
    return walk(False), walk(True)


def enc_rounding_cone(i):
    """MFCC frames [lo, hi] audio row i reads: `oracle.torch_port.audio_encoder` walked backwards (_enc_3 at 75 Hz, _down_2, _enc_2 at
    150 Hz, _down_1, _enc_1 at 300 Hz, project), with direct layers and with every stack Winograd-lowered (`dec_rounding_cone`)."""
    def layer(a, b, tiled):
        if not tiled:
            return a - 1, b + 1
        return (a - 1 if a % 4 == 0 else a - a % 4), (b + 1 if b % 4 == 3 else b - b % 4 + 3)

    def walk(tiled):
        a = b = i
        for stage in range(3):
            for _ in range(3):
                a, b = layer(a, b, tiled)
            if stage < 2:
                a, b = 2 * a - 1, 2 * b + 2          # Conv1d(k = 4, stride 2, padding 1): out[o] reads in[2 o - 1 .. 2 o + 2]
        return a - 1, b + 1                          # project: k = 3, 64 -> 256 channels, never lowered
    return walk(False), walk(True)


ENC_CONE_LOWERED = (-53, 56)      # the widest of the lowered walk over the four phases of i % 4 (checked below)


def schedules(n=200, seed=11):
    """(T, pushes) with sum(pushes) = T: T from 1 to 400, pushes from 1 to 97 frames, every fifth schedule of 1-frame pushes only."""
    rng = np.random.default_rng(seed)
    out = [(1, (1,)), (3, (3,)), (3, (1, 1, 1)), (4, (4,)), (400, (97,) * 4 + (12,)), (403, (403,))]
    while len(out) < n:
        T = int(rng.integers(1, 401))
        if len(out) % 5 == 0:
            out.append((T, (1,) * T))
            continue
        cuts, left = [], T
        while left:
            cuts.append(int(min(left, rng.integers(1, 98))))
            left -= cuts[-1]
        out.append((T, tuple(cuts)))
    return out


def run_plan(pushes, **margins):
    """The calls of a session fed `pushes` then flushed: [(Call, F after it, (frames, rows) retained after it)]."""
    p, calls = S.SeamlessPlan(**margins), []
    for t in pushes:
        c = p.push(t)
        calls.append((c, p.F, p.retained(c)))
    c = p.flush()
    calls.append((c, p.F, p.retained(c)))
    return calls, p


def cone_violations(calls, T, tiles=True, enc_cone=ENC_CONE):
    """Kept outputs whose receptive field, cut to the clip [0, T) / [0, T // 4), leaves their window.  The audio encoder: the measured
    cone.  The decoders: the measured cone (tiles=False), or the reach of their rounding under the lowering (tiles=True)."""
    bad, H = [], T // 4
    reach = [(min(dec_rounding_cone(4 * r + f)[tiles][0] for f in range(4)) - r,
              max(dec_rounding_cone(4 * r + f)[tiles][1] for f in range(4)) - r) for r in range(400, 404)]      # periodic in r % 4
    for c, _, _ in calls:
        if c.enc is not None:
            f0, f1 = c.enc
            for i in range(*c.rows):
                lo, hi = max(0, 4 * i + enc_cone[0]), min(T - 1, 4 * i + enc_cone[1])
                if lo < f0 or hi >= f1:
                    bad.append(("audio row", i, (lo, hi), c.enc))
        if c.dec is not None:
            v0, v1 = c.dec
            for r in range(*c.poses):
                lo, hi = max(0, r + reach[r % 4][0]), min(H - 1, r + reach[r % 4][1])
                if lo < v0 or hi >= v1:
                    bad.append(("pose row", r, (lo, hi), c.dec))
    return bad


def test_cover_random_schedules():
    for T, pushes in schedules():
        calls, p = run_plan(pushes)
        biggest_push = max(pushes)
        H = T // 4
        rows_at = frames_at = 0
        for k, (c, F, (keep_f, keep_r)) in enumerate(calls):
            last = k == len(calls) - 1
            assert c.rows[0] == rows_at and c.poses[0] == frames_at, (T, pushes, k)      # exactly once, in order
            rows_at, frames_at = c.rows[1], c.poses[1]
            assert c.rows[1] >= c.rows[0] and c.poses[1] >= c.poses[0] and c.poses[1] <= c.rows[1]
            assert (c.enc is None) == (c.rows[1] == c.rows[0]) and (c.dec is None) == (c.poses[1] == c.poses[0])
            if c.enc is not None:
                f0, f1 = c.enc
                assert f0 % 16 == 0 and 0 <= f0 < f1 <= F, (T, pushes, k)                # a multiple of 4 code rows; inside what has arrived
                assert last or (f1 - f0) % 4 == 0                                        # only the clip's own end brings leftover frames
                assert f0 // 4 <= c.rows[0] and c.rows[1] <= (f1 - f0) // 4 + f0 // 4    # the kept rows exist in the window's output
                assert last or f1 - f0 <= S.TAIL_CAP_FRAMES + biggest_push
            if c.dec is not None:
                v0, v1 = c.dec
                assert v0 % 4 == 0 and 0 <= v0 <= c.poses[0] and c.poses[1] <= v1 <= c.rows[1], (T, pushes, k)
                assert v1 - v0 <= S.RING_KEEP_ROWS + S.chain_rows(biggest_push)
            assert c.rows[1] - c.rows[0] <= S.chain_rows(biggest_push)                   # the chain session is never asked for more
            if not last:                                                                 # bounded state, for any history
                assert 0 <= keep_f <= S.TAIL_CAP_FRAMES - 1 and 0 <= keep_r <= S.RING_KEEP_ROWS - 1, (T, pushes, k, keep_f, keep_r)
                nxt = calls[k + 1][0]                                                    # ... and enough of it for the next call
                assert nxt.enc is None or nxt.enc[0] == c.keep_frame0
                assert nxt.dec is None or nxt.dec[0] >= c.keep_row0
        assert rows_at == H and frames_at == H and p.F == T and p.flushed
        assert sum(4 * (c.poses[1] - c.poses[0]) for c, _, _ in calls) == 4 * (T // 4)
        assert cone_violations(calls, T) == [], (T, pushes)                              # every window holds the margins
        if T < 4:
            assert all(c.enc is None and c.dec is None for c, _, _ in calls)             # nothing produced, no call made
    p = S.SeamlessPlan()
    p.push(5)
    p.flush()
    for bad in (lambda: p.push(4), lambda: p.flush(), lambda: S.SeamlessPlan().push(0), lambda: S.SeamlessPlan().peek(3, flush=True)):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def nets():
    from oracle import torch_port as P
    sd_a = P._t(synth.audioencoder_state_dict(seed=3))
    sd_v = P._t(synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=256, num_hiddens=128))
    return P, sd_a, sd_v


def test_reach_is_exactly_the_two_margins(nets):
    P, sd_a, sd_v = nets
    torch.manual_seed(0)
    with torch.no_grad():
        T = 200
        x = torch.randn(1, 64, T) * 20
        for f in (0, 1, 2, 3, 97, 100, 198, 199):
            y = x.clone()
            y[0, :, f] = float("nan")
            hit = torch.isnan(P.audio_encoder(y, sd_a)[0]).any(0).numpy()               # which audio rows read frame f
            want = np.array([4 * i + ENC_CONE[0] <= f <= 4 * i + ENC_CONE[1] for i in range(T // 4)])
            assert np.array_equal(hit, want), f
        H = 40
        lat = torch.randint(0, 255, (1, H))
        sd = dict(sd_v)
        emb = sd["vq_layer.embeddings"].clone()
        emb[255] = float("nan")                                                         # code 255 stands nowhere else
        sd["vq_layer.embeddings"] = emb
        for r in (0, 1, 19, 20, 39):
            z = lat.clone()
            z[0, r] = 255
            hit = torch.isnan(P.vqvae_decode(z, sd)[0]).any(0).numpy()                  # which pose frames read code row r
            want = np.array([t // 4 + DEC_CONE[0] <= r <= t // 4 + DEC_CONE[1] for t in range(4 * H)])
            assert np.array_equal(hit, want), r
    assert S.ENC_MARGIN_ROWS == -(ENC_CONE[0] // 4) == -(-ENC_CONE[1] // 4) == 7        # 25 and 28 frames: 7 code rows, not 6
    assert S.DEC_MARGIN_ROWS == -DEC_CONE[0] == DEC_CONE[1] == 6
    # the walk that stands for the lowered decoders gives the measured cone when no layer is tiled ...
    walks = [dec_rounding_cone(t) for t in range(1600, 1664)]
    assert all((m[0] - t // 4, m[1] - t // 4) == DEC_CONE for t, (m, _) in zip(range(1600, 1664), walks))
    # ... and 13 code rows at the most when every stack is: the slack is neither short nor padded
    far = max(max(t // 4 - w[0], w[1] - t // 4) for t, (_, w) in zip(range(1600, 1664), walks))
    assert far == S.DEC_MARGIN_ROWS + S.DEC_TILE_SLACK_ROWS == 13
    # the audio encoder, where it is lowered too: the direct walk is the measured cone, the lowered one reaches 4i-53 .. 4i+56 — 14 code rows
    ewalks = [enc_rounding_cone(i) for i in range(400, 416)]
    assert all((m[0] - 4 * i, m[1] - 4 * i) == ENC_CONE for i, (m, _) in zip(range(400, 416), ewalks))
    lowered = (min(w[0] - 4 * i for i, (_, w) in zip(range(400, 416), ewalks)), max(w[1] - 4 * i for i, (_, w) in zip(range(400, 416), ewalks)))
    assert lowered == ENC_CONE_LOWERED
    assert -(lowered[0] // 4) == -(-lowered[1] // 4) == S.ENC_MARGIN_ROWS + S.ENC_TILE_SLACK_ROWS == 14


def test_plan_of_a_lowered_encoder():
    """enc_slack=ENC_TILE_SLACK_ROWS, the plan a session takes where the audio encoder is lowered: covers the lowered cone, one row less does
    not, and the state stays bounded (8 x 14 + 15 = 127 frames)."""
    caught = 0
    for T, pushes in schedules(80):
        calls, p = run_plan(pushes, enc_slack=S.ENC_TILE_SLACK_ROWS)
        assert cone_violations(calls, T, enc_cone=ENC_CONE_LOWERED) == [], (T, pushes)
        assert p.A == p.D == T // 4 and all(c.enc is None or c.enc[0] % 16 == 0 for c, _, _ in calls)
        assert all(keep[0] <= 127 and keep[1] <= S.RING_KEEP_ROWS - 1 for _, _, keep in calls[:-1])
        assert all(c.rows[1] - c.rows[0] <= S.chain_rows(max(pushes), 14) for c, _, _ in calls)
        caught += bool(cone_violations(run_plan(pushes, enc_slack=S.ENC_TILE_SLACK_ROWS - 1)[0], T, enc_cone=ENC_CONE_LOWERED))
    assert caught > 0


@pytest.mark.parametrize("margins,tiles", [(dict(enc_margin=6), True), (dict(dec_margin=5, dec_slack=0), False), (dict(dec_slack=6), True)],
                         ids=["encoder 6", "decoder 5 of direct layers", "slack 6 of lowered layers"])
def test_a_margin_one_lower_is_caught(margins, tiles):
    caught = 0
    for T, pushes in schedules(60):
        calls, _ = run_plan(pushes, **margins)
        assert cone_violations(run_plan(pushes, dec_slack=0)[0], T, tiles=False) == []      # direct layers need no slack
        caught += bool(cone_violations(calls, T, tiles))
    assert caught > 0      # some kept output reads beyond its window (the last row of reach matters at one phase of the tiles only)


VALUE_SCHEDULES = [(403,), (64, 86, 120, 133), (10,) * 40 + (3,)]


@pytest.fixture(scope="module")
def full_call(nets):
    """The one call on a 403-frame clip, computed once: audio rows (256, 100), poses (39, 400), the codes behind them."""
    P, sd_a, sd_v = nets
    torch.manual_seed(1)
    with torch.no_grad():
        x = torch.randn(1, 64, 403) * 20
        lat = torch.randint(0, 256, (1, 100))
        return x, lat, P.audio_encoder(x, sd_a)[0].numpy(), P.vqvae_decode(lat, sd_v)[0].numpy()


def stitched(nets, full_call, pushes, **margins):
    P, sd_a, sd_v = nets
    x, lat, _, _ = full_call
    calls, _ = run_plan(pushes, **margins)
    aud, pose = [], []
    with torch.no_grad():
        for c, _, _ in calls:
            if c.enc is not None:
                f0, f1 = c.enc
                y = P.audio_encoder(x[:, :, f0:f1], sd_a)[0].numpy()
                aud.append(y[:, c.rows[0] - f0 // 4:c.rows[1] - f0 // 4])
            if c.dec is not None:
                v0, v1 = c.dec
                y = P.vqvae_decode(lat[:, v0:v1], sd_v)[0].numpy()
                pose.append(y[:, 4 * (c.poses[0] - v0):4 * (c.poses[1] - v0)])
    return np.concatenate(aud, 1), np.concatenate(pose, 1)


@pytest.mark.parametrize("pushes", VALUE_SCHEDULES, ids=["one push", "four pushes", "10-frame pushes"])
def test_values_of_the_windows_equal_the_one_call(nets, full_call, pushes):
    _, _, aud_ref, pose_ref = full_call
    aud, pose = stitched(nets, full_call, pushes)
    assert aud.shape == aud_ref.shape and pose.shape == pose_ref.shape
    ea, ep = float(np.abs(aud - aud_ref).max()), float(np.abs(pose - pose_ref).max())
    print(f"\n[measured] windows vs one call, {len(pushes)} pushes: audio rows {ea:.2e}, poses {ep:.2e} (bound 5e-6)")
    assert ea <= 5e-6 and ep <= 5e-6


def test_values_tell_a_short_margin(nets, full_call):
    """The bound above is not loose: one row short on either side fails it."""
    _, _, aud_ref, pose_ref = full_call
    aud, _ = stitched(nets, full_call, VALUE_SCHEDULES[1], enc_margin=6)
    _, pose = stitched(nets, full_call, VALUE_SCHEDULES[1], dec_margin=5, dec_slack=0)
    assert float(np.abs(aud - aud_ref).max()) > 5e-6 and float(np.abs(pose - pose_ref).max()) > 5e-6


def test_the_two_restatements_agree():
    from talkshow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    i64p = C.POINTER(C.c_int64)
    for k, (T, pushes) in enumerate(schedules(120)):
        low = k % 2                                   # every other schedule on the plan of a lowered encoder
        p = S.SeamlessPlan(enc_slack=S.ENC_TILE_SLACK_ROWS if low else 0)
        for t in pushes + (0,):
            flush = t == 0
            state = np.asarray(p.state, np.int64)
            out = np.full(14, -7, np.int64)
            assert lib.ts_debug_body_stream_plan(state.ctypes.data_as(i64p), t, int(flush), low, out.ctypes.data_as(i64p)) == 0, lib.ts_last_error()
            c = p.flush() if flush else p.push(t)
            enc, dec = c.enc or (0, 0), c.dec or (0, 0)
            want = list(p.state) + [enc[0], enc[1], c.rows[0], c.rows[1], dec[0], dec[1], c.poses[0], c.poses[1], c.keep_frame0, c.keep_row0]
            assert out.tolist() == want, (T, pushes, t)
        state = np.asarray(p.state, np.int64)
        assert lib.ts_debug_body_stream_plan(state.ctypes.data_as(i64p), 4, 0, low, out.ctypes.data_as(i64p)) != 0      # after the flush
    fresh = np.zeros(4, np.int64)
    assert lib.ts_debug_body_stream_plan(fresh.ctypes.data_as(i64p), 0, 0, 0, out.ctypes.data_as(i64p)) != 0       # t = 0
    assert S.chain_rows(1) == 7 and S.chain_rows(240) == 61 and S.chain_rows(1, 14) == 14
