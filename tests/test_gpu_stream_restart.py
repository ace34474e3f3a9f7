"""Slot restart on the streaming sessions (`ts_pixelcnn_stream_restart`, `PixelCNNStream.restart`, `BodyStream.restart`;
include/talkshow_hip.h, "slot restart"): a slot of a running session ends its clip and begins a new one while its neighbours carry on.

The yardstick throughout is the one-shot `GatedPixelCNN.run` on the clip ALONE (B = 1, same seed, clip_index0 = the slot's clip index, the
slot's own keywords): every comparison is EQUALITY of codes and of log-probability bits.  A slot that is never restarted is held against
ONE one-shot call over all of its rows, computed once per (case, draw mode) and shared (a shorter session is a prefix of it: the network is
causal in the row direction).

Shapes, as in test_gpu_stream_ctl.py: (S) the `pix_small` golden's network (V = 128: the generic sampler path) at B = 3; (F) the full-size
synthetic network (V = 2048: the register path) at B = 2; (W) (S)'s network at B = 33 (across the 16- and 32-row slab edges).  Every test
fails on a build without the feature: the session has no such method and the library no such symbol.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from talkshow_amd.streaming import SlotClock

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, CLIP0 = 77, 5
RECS = [(0.8, 0.9, 0), (1.3, 1.0, 5), None]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Case:
    def __init__(self, m, label, aud, seed):
        self.m, self.label = m, np.asarray(label, np.int64)
        self.aud = torch.as_tensor(aud, dtype=torch.float32).cuda()
        self.B, self.H = int(self.aud.shape[0]), int(self.aud.shape[1])
        self.V, self.NC = m.input_dim, m.n_classes
        rng = np.random.default_rng(seed)
        B, V = self.B, self.V
        t0 = np.zeros((2, V), F32)
        t0[:, rng.choice(V, V // 2, replace=False)] = -np.inf
        t1 = rng.standard_normal((2, V)).astype(F32)
        t1[0, rng.choice(V, V // 4, replace=False)] = -np.inf
        self.sampling = [RECS[b % 3] for b in range(B)]
        self.bias = [(t1, t0, None)[b % 3] for b in range(B)]                # slot 1 (the restarted one) draws under t0's bans
        self.u = (0.999 * rng.random((B, self.H, 2))).astype(F32)
        self.blend = rng.random(self.NC).astype(F32)

    def draw(self, how, b=None, s=0, e=None, clip=None):
        """The drawing arguments of a session step over rows [s, e) (b None), or of the one-shot call on slot b's clip that holds them."""
        from talkshow_amd import _lib
        if how == "greedy":
            return dict(mode=_lib.TS_SAMPLE_GREEDY)
        if how == "uniforms":
            return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(self.u[:, s:e] if b is None else self.u[b:b + 1, s:e]))
        return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0 if b is None else (CLIP0 + b if clip is None else clip))

    def alone(self, how, b, s, e, seg, kw=None, lp=False, given=None):
        """(codes (e-s,2), log-probability bits or None) of the clip that slot b held over session rows [s, e), run alone."""
        k1 = {k: [v[b]] for k, v in (kw or {}).items()}
        if seg["style"] is not None:
            k1["style"] = [seg["style"]]
        if given and b in given and given[b][0] == s:
            k1["given"] = [given[b][1]]
        out = self.m.run(np.array([seg["label"]], np.int64), self.aud[b:b + 1, s:e], **self.draw(how, b, s, e, seg["clip"]), logprobs=lp, **k1)
        return _np(out[0])[0], (_bits(out[2])[0] if lp else None)

    def play(self, how, events, kw=None, lp=False, given=None, max_rows=8):
        """A session through `events`: ("step", Hc) or ("restart", slots, labels or None, clip indices, style rows or None).  kw: per-slot
        keyword lists of every step; given: {slot: (session row of its clip's first row, (g,2) block)}: the clip's first g rows are taken.
        Returns codes (B,H,2), log-probability bits (or None) and, per slot, the clips it held: dict(start, label, style, clip)."""
        st = self.m.open_stream(self.label, self.B, max_rows)
        clock = SlotClock(self.B)
        segs = [[dict(start=0, label=int(self.label[b]), style=None, clip=None)] for b in range(self.B)]
        codes, lps = [], []
        for ev in events:
            if ev[0] == "restart":
                slots, labels, clips, styles = ev[1], ev[2], ev[3], ev[4] if len(ev) > 4 else None
                st.restart(slots, labels, style=styles, clip_indices=clips)
                clock.restart(slots, clips)
                for i, b in enumerate(slots):
                    old = segs[b][-1]
                    seg = dict(start=clock.row, label=old["label"] if labels is None or labels[i] is None else int(labels[i]),
                               style=None if styles is None else styles[i], clip=clips[i])
                    if old["start"] == clock.row:
                        segs[b][-1] = seg
                    else:
                        segs[b].append(seg)
                continue
            hc, at = ev[1], clock.row
            k = dict(kw or {})
            if given:
                g = [None] * self.B
                for b, (s0, block) in given.items():
                    if s0 <= at < s0 + len(block):
                        g[b] = block[at - s0:at - s0 + hc]
                if any(x is not None for x in g):
                    k["given"] = g
            out = st.step(self.aud[:, at:at + hc], **self.draw(how, None, at, at + hc), logprobs=lp, **k)
            if lp:
                codes.append(_np(out[0])), lps.append(_bits(out[1]))
            else:
                codes.append(_np(out))
            clock.advance(hc)
            assert st.rows == clock.row and list(st.slot_rows) == clock.slot_rows
        st.close()
        return np.concatenate(codes, 1), (np.concatenate(lps, 1) if lp else None), segs

    def check(self, how, codes, lps, segs, kw=None, lp=False, given=None, slots=None, tag=""):
        """Every clip every listed slot held equals its one-shot call."""
        H = codes.shape[1]
        for b in range(self.B) if slots is None else slots:
            for i, seg in enumerate(segs[b]):
                s, e = seg["start"], segs[b][i + 1]["start"] if i + 1 < len(segs[b]) else H
                if e == s:
                    continue
                want = self.alone(how, b, s, e, seg, kw, lp, given)
                bad = np.flatnonzero((codes[b, s:e] != want[0]).any(1))[:1]
                assert bad.size == 0, f"{tag} {how}: slot {b}, clip from session row {s}: first differing clip row {bad}"
                if lp:
                    assert np.array_equal(lps[b, s:e], want[1]), f"{tag} {how}: slot {b}, clip from session row {s}: log-probability bits differ"


@pytest.fixture(scope="module")
def cases(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    assert m.input_dim == 128
    full = GatedPixelCNN(2048, 256, 15, 4, True, True).cuda()
    full.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=7)))
    rng = np.random.default_rng(61)
    return {"S": Case(m, np.asarray(g["label"])[:3], rng.standard_normal((3, 14, 256)).astype(F32), 1),
            "F": Case(full, synth.speaker_ids(2), rng.standard_normal((2, 14, 256)).astype(F32), 2),
            "W": Case(m, np.arange(33) % m.n_classes, rng.standard_normal((33, 8, 256)).astype(F32), 3)}


_WHOLE = {}


def _whole(c, name, how, b):
    """Slot b's uninterrupted one-shot call over all H rows of the case, once per (case, draw mode, slot); nobody changes it."""
    if (name, how, b) not in _WHOLE:
        _WHOLE[(name, how, b)] = c.alone(how, b, 0, c.H, dict(label=int(c.label[b]), style=None, clip=None))[0]
    return _WHOLE[(name, how, b)]


# ---- 1. a restart at every row: all seven buffer phases, and the rows where Q / P terms are absent ---------------------------------------------
@pytest.mark.parametrize("k", range(9))
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
@pytest.mark.parametrize("name", [pytest.param("S", id="small"), pytest.param("F", id="full")])
def test_restart_at_every_row(cases, name, how, k):
    c = cases[name]
    new_label = (int(c.label[1]) + 1) % c.NC
    events = ([("step", k)] if k else []) + [("restart", [1], [new_label], [40 + k]), ("step", 1), ("step", 2), ("step", 3)]
    codes, _, segs = c.play(how, events)
    assert codes.shape[1] == k + 6 and segs[1][-1]["start"] == k
    c.check(how, codes, None, segs, slots=[1], tag=f"{name} k={k}")           # the old clip's k rows and the new clip's 6
    for b in range(c.B):
        if b != 1:
            assert np.array_equal(codes[b], _whole(c, name, how, b)[:k + 6]), f"{name} {how} k={k}: neighbour slot {b} changed"
    if how == "philox":                                                          # the new clip is not the old one carried on
        assert not np.array_equal(codes[1], _whole(c, name, how, 1)[:k + 6])


# ---- 2. several slots at once, at different rows, the same slot twice ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
def test_several_slots_and_the_same_slot_twice(cases, how):
    c = cases["S"]
    events = [("step", 2), ("restart", [0, 2], [3, 1], [50, 51]), ("step", 3), ("restart", [2], [0], [52]), ("step", 1),
              ("restart", [1, 0], [2, 2], [53, 50]), ("restart", [1], [0], [54]), ("step", 4)]
    codes, lps, segs = c.play(how, events, lp=True)
    assert [len(s) for s in segs] == [3, 2, 3] and segs[1][-1] == dict(start=6, label=0, style=None, clip=54)
    c.check(how, codes, lps, segs, lp=True, tag="S")


@pytest.mark.parametrize("how", ["greedy", "philox"])
def test_slots_across_the_slab_edges(cases, how):
    c = cases["W"]
    events = [("step", 2), ("restart", [0, 16, 32], [1, 2, 3], [100, 116, 132]), ("step", 3), ("restart", [32, 15, 31], [0, 0, 1], [232, 215, 231]),
              ("step", 3)]
    codes, _, segs = c.play(how, events)
    c.check(how, codes, None, segs, tag="W")                                    # all 33 slots: the five restarted ones and every neighbour


# ---- 3. under keywords, the restarted clip and its neighbours together --------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["philox", "uniforms"])
@pytest.mark.parametrize("key", ["sampling", "code_bias", "repeat3", "repeat5", "style", "given", "logprobs", "every"])
def test_keywords(cases, key, how):
    c = cases["S"]
    rep = {"repeat3": [(5, 1.0, 0.5), (3, 1e30, 0.0), (0, 1.0, 1.0)], "repeat5": [(3, 0.7, 0.3), (5, 1e30, 0.0), (64, 0.5, 0.1)]}
    kw, style, given = {}, None, None
    if key in ("sampling", "every"):
        kw["sampling"] = c.sampling
    if key in ("code_bias", "every"):
        kw["code_bias"] = c.bias
    if key in rep or key == "every":
        kw["repeat"] = rep.get(key, rep["repeat5"])
    if key in ("style", "every"):
        style = [c.blend]
    if key in ("given", "every"):
        given = {1: (4, np.random.default_rng(9).integers(0, c.V // 2, (2, 2)))}
    events = [("step", 4), ("restart", [1], None if style else [2], [41], style), ("step", 1), ("step", 2), ("step", 3)]
    codes, lps, segs = c.play(how, events, kw=kw, lp=True, given=given)
    c.check(how, codes, lps, segs, kw=kw, lp=True, given=given, tag=key)
    if given:
        assert np.array_equal(codes[1, 4:6], given[1][1])
    drawn = range(6 if given else 4, 10)                                         # the new clip's rows that were not taken
    if "code_bias" in kw:                                                        # the slot's table held: no banned code was drawn
        for j in range(2):
            assert np.all(np.isfinite(c.bias[1][j][codes[1, drawn, j]]))
    if "repeat" in kw:                                                           # a presence of 1e30 bans the codes of the window — counted
        W = kw["repeat"][1][0]                                                   # from the restart: the old clip's rows are not in it
        for j in range(2):
            for r in drawn:
                assert codes[1, r, j] not in codes[1, max(4, r - W):r, j], f"row {r} column {j} repeats a code of the last {W} rows"


# ---- 4. graphs -----------------------------------------------------------------------------------------------------------------------------------
def _stats(st):
    from talkshow_amd import _lib
    g, n, f = C.c_int64(), C.c_int64(), C.c_double()
    _lib.check(_lib.load().ts_pixelcnn_stream_graph_stats(st._h, C.byref(g), C.byref(n), C.byref(f)))
    return g.value, n.value, f.value


def test_warm_session_captures_nothing_on_later_restarts(cases):
    c = cases["S"]
    d = c.draw("philox")
    st = c.m.open_stream(c.label, c.B, 3)
    st.restart([1], [2], clip_indices=[9])
    for at in range(0, 15, 3):                                                   # the warm round: buffer phases 0, 3 + 3, 3 + 2, 3 + 1, 3 + 0
        st.step(c.aud[:, at % 12:at % 12 + 3], **d)
    caps = st.graph_captures()
    assert caps == 5
    for slots in ([0], [2, 1], [], [0, 1, 2]):                                   # rows 15, 18, 21, 24: the same four phases again
        if slots:
            st.restart(slots, [1] * len(slots), clip_indices=[60 + b for b in slots])
        st.step(c.aud[:, 0:3], **d)
    assert st.graph_captures() == caps, "a restart of other slots at other rows captured a graph"
    assert list(st.slot_rows) == [3, 3, 3] and st.rows == 27
    st.close()


def test_session_that_never_restarts_is_the_session_there_was(cases):
    """Capture count, graph count and the chain launches recorded at capture: two sessions that never restart agree with each other and
    with the counts of test_gpu_stream_ctl.py::test_defaults_and_graphs (2 graphs for steps of 4 rows: buffer phases 0 and 3 + 0); a
    session that does restart runs the SAME number of chain launches per step — its graphs differ by the samplers' arguments alone."""
    c = cases["S"]
    d = c.draw("philox")
    out = {}
    for tag in ("a", "restarted", "b"):
        st = c.m.open_stream(c.label, c.B, 4)
        codes = [st.step(c.aud[:, 0:4], **d)]
        if tag == "restarted":
            st.restart([1], [2], clip_indices=[9])
        codes += [st.step(c.aud[:, 4:8], **d), st.step(c.aud[:, 8:12], **d)]
        out[tag] = (st.graph_captures(), _stats(st), _np(torch.cat(codes, 1)))
        st.close()
    assert out["a"][0] == out["b"][0] == 2 and out["a"][1] == out["b"][1] and out["a"][1][0] == 2
    assert np.array_equal(out["a"][2], out["b"][2])
    for b in range(c.B):
        assert np.array_equal(out["a"][2][b], _whole(c, "S", "philox", b)[:12])
    assert out["restarted"][0] == 2 and out["restarted"][1] == out["a"][1]       # phase 0 plain, phase 3 + 0 under the origin table
    assert np.array_equal(out["restarted"][2][[0, 2]], out["a"][2][[0, 2]]) and not np.array_equal(out["restarted"][2][1], out["a"][2][1])


def test_graphs_off_same_bits():
    """The eager launches (TS_NO_GRAPH=1; the levers are read once per process -> child process): test 1 on (S) and test 2."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                        "(test_restart_at_every_row and small) or test_several_slots"], env=dict(os.environ, TS_NO_GRAPH="1"),
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "30 passed" in r.stdout, r.stdout[-500:]


# ---- 5. BodyStream.restart -----------------------------------------------------------------------------------------------------------------------
def test_body_stream_restart(cases):
    import bench
    from talkshow_amd import _lib
    c = cases["S"]
    w = bench.build_models(0, seed=7)[0]
    w.generator = c.m
    sched, at_push = (3, 1, 4, 2), 2
    mf = torch.from_numpy(synth.mfcc_features(501, c.B, 4 * sum(sched))).cuda()
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED)
    ids = torch.from_numpy(c.label)
    sessions = {"restarted": w.open_stream(ids, c.B, 4 * max(sched)), "plain": w.open_stream(ids, c.B, 4 * max(sched)),
                "fresh": None}
    poses = {k: [] for k in sessions}
    at = 0
    for i, hc in enumerate(sched):
        chunk = mf[:, 4 * at:4 * (at + hc)]
        if i == at_push:
            sessions["restarted"].restart([1], [2], clip_indices=[44])
            sessions["fresh"] = w.open_stream(torch.tensor([2]), 1, 4 * max(sched))
            assert list(sessions["restarted"].slot_rows) == [at, 0, at]
        poses["restarted"].append(sessions["restarted"].push(chunk, clip_index0=CLIP0, **kw))
        poses["plain"].append(sessions["plain"].push(chunk, clip_index0=CLIP0, **kw))
        if sessions["fresh"] is not None:
            poses["fresh"].append(sessions["fresh"].push(chunk[1:2], clip_index0=44, **kw))
        at += hc
    got, plain, fresh = (torch.cat(poses[k], 1) for k in ("restarted", "plain", "fresh"))
    t0 = 4 * sum(sched[:at_push])
    assert got.shape == (c.B, 4 * at, 129) and fresh.shape == (1, 4 * at - t0, 129)
    assert torch.equal(got[1, t0:], fresh[0]), "the restarted slot's poses differ from a fresh session's"
    assert torch.equal(got[[0, 2]], plain[[0, 2]]) and torch.equal(got[1, :t0], plain[1, :t0]), "a neighbour's poses changed"
    assert not torch.equal(got[1, t0:], plain[1, t0:])
    for s in sessions.values():
        s.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_where_it_was(cases):
    from talkshow_amd import _lib
    c = cases["S"]
    d = c.draw("philox")
    st = c.m.open_stream(c.label, c.B, 4)
    first = st.step(c.aud[:, 0:4], **d)
    nan_row = np.full(c.NC, np.nan, F32)
    bad = [("slot 3", dict(slots=[0, 3], label=[0, 0])), ("slot -1", dict(slots=[-1], label=[0])), ("slot 1 is listed twice", dict(slots=[1, 2, 1], label=0)),
           (f"slot 2: label {c.NC}", dict(slots=[1, 2], label=[0, c.NC])), ("slot 0: label -1", dict(slots=0, label=-1)),
           ("slot 1 brings both", dict(slots=[1], label=[0], style=[c.blend])), ("slot 2 brings neither", dict(slots=[1, 2], label=[0, None])),
           ("slot 0: clip index -2", dict(slots=[0], label=[1], clip_indices=[-2])), ("slot 1: a style row holds", dict(slots=[1], style=[np.ones(c.NC + 1, F32)])),
           ("slot 1: a style weight is not finite", dict(slots=[1], style=[nan_row]))]
    for names, kw in bad:
        with pytest.raises(ValueError, match=names):
            st.restart(**kw)
        assert st.rows == 4 and list(st.slot_rows) == [4, 4, 4], names
    lib, h = _lib.load(), st._h                                                  # the C entry's own checks: the failing slot is named
    i32, i64 = C.c_int32 * 2, C.c_int64 * 2
    style = torch.ones((2, c.NC), dtype=torch.float32, device="cuda")
    for names, args in [("slot 3 is outside", (i32(0, 3), 2, i64(0, 0), None, i64(1, 2))), ("slot 1 is listed twice", (i32(1, 1), 2, i64(0, 0), None, i64(1, 2))),
                        (f"slot 2: label {c.NC}", (i32(0, 2), 2, i64(0, c.NC), None, i64(1, 2))), ("slot 2: clip index -1", (i32(0, 2), 2, i64(0, 0), None, i64(1, -1))),
                        ("both a label and a style row", (i32(0, 2), 2, i64(0, 0), _lib.dptr(style), i64(1, 2))),
                        ("neither a label nor a style row", (i32(0, 2), 2, None, None, i64(1, 2)))]:
        with pytest.raises(RuntimeError, match=names):
            _lib.check(lib.ts_pixelcnn_stream_restart(h, *args, _lib.stream_ptr()))
        assert st.rows == 4 and list(st.slot_rows) == [4, 4, 4], names
    assert lib.ts_pixelcnn_stream_slot_rows(h, 3) == -1
    rest = st.step(c.aud[:, 4:8], **d)                                           # the session continues to the right bits
    assert st.graph_captures() == 2                                              # on the plain keys: no refused call bound the origin table
    st.close()
    codes = _np(torch.cat([first, rest], 1))
    for b in range(c.B):
        assert np.array_equal(codes[b], _whole(c, "S", "philox", b)[:8])


def test_seamless_session_restarts_no_slot(cases):
    import bench
    w = bench.build_models(0, seed=7)[0]
    st = w.open_stream([0, 1], 2, 48, seamless=True)
    with pytest.raises(NotImplementedError, match="seamless"):
        st.restart([0], 1)
    st.close()
