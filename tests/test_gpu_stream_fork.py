"""Slot state on the streaming sessions (`ts_pixelcnn_stream_save` / `_load`, `PixelCNNStream.save` / `load` / `fork`, `BodyStream`;
include/talkshow_hip.h, "slot state"): a slot's clip is saved and carried on in any slot of any session of the same network.

The yardstick throughout is the one-shot `GatedPixelCNN.run` over the clip's WHOLE audio (the source slot's rows up to the save, then the
target slot's rows from the load on) with `given=` the clip's first n code rows and clip_index0 = the index it was loaded under: the loaded
slot's rows equal rows n, n+1, ... of it.  Every comparison is EQUALITY of codes and of log-probability bits.  A slot that is not loaded is
held against a twin session that never saved or loaded.

Shapes, as in test_gpu_stream_restart.py: (S) the `pix_small` golden's network (V = 128) with a source session of B = 3 and target sessions
of B = 2 and 4; (F) the full-size synthetic network (V = 2048) with B = 2 and a dozen rows; (W) (S)'s network at B = 33.  Every test fails
on a build without the feature: the sessions have no such methods and the library no such symbols.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from talkshow_amd.streaming import SlotClock, SlotState

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, CLIP0 = 77, 5
HOWS = ["greedy", "uniforms", "philox"]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Net:
    def __init__(self, m, labels, seed):
        self.m, self.labels = m, np.asarray(labels, np.int64)
        self.V, self.NC = m.input_dim, m.n_classes
        rng = np.random.default_rng(seed)
        self.B, self.H = len(self.labels), 24
        self.aud = torch.from_numpy(rng.standard_normal((2, self.B, self.H, 256)).astype(F32)).cuda()   # [0]: source sessions, [1]: targets
        self.u = (0.999 * rng.random((2, self.B, self.H, 2))).astype(F32)
        self.blend = rng.random(self.NC).astype(F32)
        V = self.V
        self.table = np.zeros((2, V), F32)
        self.table[:, rng.choice(V, V // 2, replace=False)] = -np.inf


class Sess:
    """A session over rows of side `side` of the net's audio and uniforms, slots [0, B); collects what its steps return."""

    def __init__(self, net, side, B, how, lp=False, max_rows=8, m=None, labels=None):
        self.net, self.side, self.B, self.how, self.lp = net, side, B, how, lp
        self.st = (m or net.m).open_stream(net.labels[:B] if labels is None else labels, B, max_rows)
        self.codes, self.lps, self.at = [], [], 0
        self.shift = np.zeros(B, np.int64)       # audio / uniform row of slot b at session row r: r + shift[b] (a rewound slot hears rows again)

    def draw(self, s, e):
        from talkshow_amd import _lib
        if self.how == "greedy":
            return dict(mode=_lib.TS_SAMPLE_GREEDY)
        if self.how == "uniforms":
            u = np.stack([self.net.u[self.side, b, self.rows_of(b, s, e)] for b in range(self.B)])
            return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(u))
        return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0)

    def rows_of(self, b, s, e):
        return (np.arange(s, e) + int(self.shift[b])) % self.net.H   # (a long session hears the rows again: only its graph counts are read)

    def audio(self, s, e):
        return torch.stack([self.net.aud[self.side, b, self.rows_of(b, s, e)] for b in range(self.B)])

    def step(self, hc, **kw):
        s, e = self.at, self.at + hc
        out = self.st.step(self.audio(s, e), **self.draw(s, e), logprobs=self.lp, **kw)
        if self.lp:
            self.codes.append(_np(out[0])), self.lps.append(_bits(out[1]))
        else:
            self.codes.append(_np(out))
        self.at = e
        assert self.st.rows == e
        return self

    def to(self, r, **kw):
        while self.at < r:
            self.step(min(3, r - self.at), **kw)
        return self

    def out(self):
        c = np.concatenate(self.codes, 1) if self.codes else np.zeros((self.B, 0, 2), np.int64)
        return c, (np.concatenate(self.lps, 1) if self.lps else None)

    def close(self):
        self.st.close()


def oracle(net, how, label, aud, u, head, clip, lp=False, m=None, **kw):
    """rows n .. of the one-shot call over the clip's whole audio (rows, 256) with its first n = len(head) code rows given."""
    from talkshow_amd import _lib
    n = 0 if head is None else len(head)
    if how == "greedy":
        d = dict(mode=_lib.TS_SAMPLE_GREEDY)
    elif how == "uniforms":
        d = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(u[None]))
    else:
        d = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=clip)
    if n:
        kw = dict(kw, given=[np.concatenate([head, kw.pop("given")[0]]) if "given" in kw else head])
    out = (m or net.m).run(np.array([label], np.int64), aud[None], **d, logprobs=lp, **kw)
    return _np(out[0])[0, n:], (_bits(out[2])[0, n:] if lp else None)


def clip_of(net, b_src, r, b_dst, r2, m_rows):
    """The audio and uniforms of the clip that ran rows [0, r) in source slot b_src and runs rows [r2, r2 + m_rows) in target slot b_dst."""
    aud = torch.cat([net.aud[0, b_src, :r], net.aud[1, b_dst, r2:r2 + m_rows]])
    return aud, np.concatenate([net.u[0, b_src, :r], net.u[1, b_dst, r2:r2 + m_rows]])


@pytest.fixture(scope="module")
def nets(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    sd = synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls))
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(sd)
    m2 = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()     # a second handle of equal weights
    m2.load_state_dict(sd)
    full = GatedPixelCNN(2048, 256, 15, 4, True, True).cuda()
    full.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=7)))
    S = Net(m, np.arange(4) % n_cls, 1)
    S.m2 = m2
    return {"S": S, "F": Net(full, synth.speaker_ids(2), 2), "W": Net(m, np.arange(33) % n_cls, 3)}


_SRC = {}


def source(net, name, how, rows=9, B=3):
    """The source session of (net, draw mode), stepped row by row with slot 1 saved AT EVERY ROW 0 .. rows-1 — and, beside it, a twin that
    never saved: the same codes, captures and graph figures (a save is read-only).  Once per (net, mode); nobody changes it."""
    if (name, how) not in _SRC:
        B = min(B, net.B)
        s, twin = Sess(net, 0, B, how), Sess(net, 0, B, how)
        states = []
        for r in range(rows):
            caps = s.st.graph_captures()
            states.append(s.st.save([1]))
            assert s.st.graph_captures() == caps and s.st.rows == r
            s.step(1), twin.step(1)
        codes, tcodes = s.out()[0], twin.out()[0]
        assert np.array_equal(codes, tcodes), "a session that saved differs from its twin"
        assert s.st.graph_captures() == twin.st.graph_captures() and _stats(s.st) == _stats(twin.st)
        for r, stt in enumerate(states):
            o = stt.infos[0]
            assert (o["rows"], o["label"], o["hist"], o["version"]) == (r, int(net.labels[1]), -1, 1)
            assert o["clip_index"] == (-1 if r == 0 else (CLIP0 if how == "philox" else 0) + 1) and (o["V"], o["NC"]) == (net.V, net.NC)
        s.close(), twin.close()
        _SRC[(name, how)] = (states, codes)
    return _SRC[(name, how)]


_TWIN = {}


def target_twin(net, name, how, B, rows):
    """The target session that never loads, once per (net, mode, B)."""
    if (name, how, B) not in _TWIN:
        t = Sess(net, 1, B, how).to(rows)
        _TWIN[(name, how, B)] = t.out()[0]
        t.close()
    return _TWIN[(name, how, B)]


def _stats(st):
    from talkshow_amd import _lib
    g, n, f = C.c_int64(), C.c_int64(), C.c_double()
    _lib.check(_lib.load().ts_pixelcnn_stream_graph_stats(st._h, C.byref(g), C.byref(n), C.byref(f)))
    return g.value, n.value, f.value


def continuation(net, name, how, rs, r2, via_c=False):
    states, src = source(net, name, how)
    twin = target_twin(net, name, how, 2, 12)
    for r in rs:
        k2 = 40 + r
        t = Sess(net, 1, 2, how).to(r2)
        if via_c:
            _c_load(t.st, [0], states[r], [0], [k2])
        else:
            t.st.load([0], states[r], clip_indices=[k2])
        assert list(t.st.slot_rows) == [r, r2] and t.st.rows == r2
        t.step(1).step(2).step(3)
        got = t.out()[0]
        t.close()
        aud, u = clip_of(net, 1, r, 0, r2, 6)
        want = oracle(net, how, int(net.labels[1]), aud, u, src[1, :r], k2)[0]
        bad = np.flatnonzero((got[0, r2:] != want).any(1))[:1]
        assert bad.size == 0, f"{name} {how} r={r} r'={r2}: the loaded slot differs from the one-shot call from its row {bad} on"
        assert np.array_equal(got[0, :r2], twin[0, :r2]) and np.array_equal(got[1], twin[1, :r2 + 6]), f"{name} {how} r={r} r'={r2}: slot 1 changed"


# ---- 1. continuation against the one-shot oracle: every save row, every load phase ---------------------------------------------------------------
@pytest.mark.parametrize("r2", range(3, 7))
@pytest.mark.parametrize("how", HOWS)
def test_continuation_small(nets, how, r2):
    continuation(nets["S"], "S", how, range(9), r2)


@pytest.mark.parametrize("r2", [3, 4])
@pytest.mark.parametrize("how", HOWS)
def test_continuation_full_size(nets, how, r2):
    continuation(nets["F"], "F", how, (0, 2, 5), r2)


def _c_save(st, slots):
    from talkshow_amd import _lib
    lib, n = _lib.load(), len(slots)
    W = int(lib.ts_pixelcnn_slot_state_words(st.net.handle()))
    words = torch.empty((n, W), dtype=torch.int32, device="cuda")
    info = (_lib.TsSlotInfo * n)()
    _lib.check(lib.ts_pixelcnn_stream_save(st._h, (C.c_int32 * n)(*slots), n, _lib.dptr(words), info, _lib.stream_ptr()))
    return words, info


def _c_info(state):
    from talkshow_amd import _lib
    info = (_lib.TsSlotInfo * len(state))()
    for o, d in zip(info, state.infos):
        for k, _ in _lib.TsSlotInfo._fields_:
            setattr(o, k, int(d[k]))
    return info


def _c_load(st, slots, state, index, clips):
    from talkshow_amd import _lib
    n = len(slots)
    words = state.words.cuda().contiguous()
    _lib.check(_lib.load().ts_pixelcnn_stream_load(st._h, (C.c_int32 * n)(*slots), n, _lib.dptr(words), len(state), (C.c_int32 * n)(*index) if index else None,
                                                  _c_info(state), (C.c_int64 * n)(*clips) if clips else None, _lib.stream_ptr()))


def test_continuation_through_the_c_entries(nets):
    """Once through ts_pixelcnn_stream_save / _load themselves: the words the C save writes are the words of `PixelCNNStream.save`, and a C load
    carries the clip on."""
    net = nets["S"]
    s = Sess(net, 0, 3, "philox").to(5)
    words, info = _c_save(s.st, [1, 2])
    py = s.st.save([1, 2])
    assert torch.equal(words, py.words) and [int(o.rows) for o in info] == [5, 5] and [int(o.clip_index) for o in info] == [CLIP0 + 1, CLIP0 + 2]
    assert int(info[0].label) == -1 and int(info[0].hist) == -1 and int(info[0].D) == net.m.dim     # the library was never told the label
    s.close()
    continuation(net, "S", "philox", (0, 2, 7), 4, via_c=True)


# ---- 2. rewind --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_rewind(nets, how):
    net = nets["S"]
    s = Sess(net, 0, 3, how).to(6)
    state = s.st.save(1)
    s.to(11)
    s.st.load([1], state)                                    # the same slot, the index it drew under: the take is played again
    s.shift[1] = -5
    assert list(s.st.slot_rows) == [11, 6, 11]
    s.to(16)
    codes = s.out()[0]
    assert np.array_equal(codes[1, 11:16], codes[1, 6:11]), f"{how}: the rewound slot does not repeat its rows"
    twin = Sess(net, 0, 3, how).to(16)
    assert np.array_equal(codes[[0, 2]], twin.out()[0][[0, 2]])
    twin.close()
    s.st.load([1], state, clip_indices=[91])                 # and under another index: another take of the same rows
    s.shift[1] = -10
    s.to(21)
    codes = s.out()[0]
    s.close()
    want = oracle(net, how, int(net.labels[1]), net.aud[0, 1, :11], net.u[0, 1, :11], codes[1, :6], 91)[0]
    assert np.array_equal(codes[1, 16:21], want)
    if how == "philox":
        assert not np.array_equal(codes[1, 16:21], codes[1, 6:11])


# ---- 3. fan-out ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_fan_out_and_the_same_slot_twice(nets, how):
    net = nets["S"]
    states, src = source(net, "S", how)
    r, r2 = 5, 4
    t = Sess(net, 1, 4, how, lp=True).to(r2)
    t.st.load([0, 2, 3], states[r], clip_indices=[60, 61, 62])
    t.st.load([0], states[r], clip_indices=[70])
    t.st.load([0], states[r], clip_indices=[71])
    assert list(t.st.slot_rows) == [r, r2, r, r]
    t.to(r2 + 6)
    got, lps = t.out()
    t.close()
    twin = target_twin(net, "S", how, 4, 12)
    assert np.array_equal(got[1], twin[1, :r2 + 6])
    for b, k in ((0, 71), (2, 61), (3, 62)):
        aud, u = clip_of(net, 1, r, b, r2, 6)
        want = oracle(net, how, int(net.labels[1]), aud, u, src[1, :r], k, lp=True)
        assert np.array_equal(got[b, r2:], want[0]) and np.array_equal(lps[b, r2:], want[1]), f"{how}: slot {b} under index {k}"


# ---- 4. slots of wide sessions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "philox"])
def test_slots_across_the_slab_edges(nets, how):
    net = nets["W"]
    src_slots, dst_slots, r, r2 = [0, 15, 16, 31, 32], [32, 31, 16, 15, 0], 4, 3
    s = Sess(net, 0, 33, how).to(r)
    state = s.st.save(src_slots)
    src = s.out()[0]
    s.close()
    t = Sess(net, 1, 33, how).to(r2)
    t.st.load(dst_slots, state, clip_indices=[100 + b for b in dst_slots])
    t.to(r2 + 4)
    got = t.out()[0]
    t.close()
    twin = Sess(net, 1, 33, how).to(r2 + 4)
    tw = twin.out()[0]
    twin.close()
    for b in range(33):
        if b not in dst_slots:
            assert np.array_equal(got[b], tw[b]), f"{how}: neighbour slot {b} changed"
    for a, b in zip(src_slots, dst_slots):
        aud, u = clip_of(net, a, r, b, r2, 4)
        want = oracle(net, how, int(net.labels[a]), aud, u, src[a, :r], 100 + b)[0]
        assert np.array_equal(got[b, r2:], want), f"{how}: slot {a} -> slot {b}"


# ---- 5. under controls ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["philox", "uniforms"])
@pytest.mark.parametrize("key", ["sampling", "code_bias", "repeat3", "repeat5", "style", "given", "every"])
def test_under_controls(nets, key, how):
    """The source runs 6 rows under the control and saves slot 1; the target is at row 3 (a history of 6 rows is longer than r' = 3) and
    steps the loaded slot 0 under the same control: records, tables and given rows are the TARGET's steps', the history and the blend row
    came with the state."""
    net = nets["S"]
    rec = {"repeat3": (3, 1e30, 0.0), "repeat5": (5, 0.7, 0.3)}
    off = (0, 1.0, 1.0)
    r, r2, k2 = 6, 3, 33
    one, skw, tkw = {}, {}, {}                               # the clip's own keyword values; the source's and the target's step keywords
    if key in ("sampling", "every"):
        one["sampling"] = (0.8, 0.9, 0)
        skw["sampling"], tkw["sampling"] = [None, one["sampling"], None], [one["sampling"], None]
    if key in ("code_bias", "every"):
        one["code_bias"] = net.table
        skw["code_bias"], tkw["code_bias"] = [None, net.table, None], [net.table, None]
    if key in rec or key == "every":
        one["repeat"] = rec.get(key, rec["repeat5"])
        skw["repeat"], tkw["repeat"] = [off, one["repeat"], off], [one["repeat"], off]
    s = Sess(net, 0, 3, how, lp=True)
    if key in ("style", "every"):
        s.step(2, style=[None, net.blend, None], **skw)      # in force from the clip's row 0, and until a step brings other rows: none does
    s.to(r, **skw)
    state = s.st.save([1])
    assert state.infos[0]["hist"] == (r if "repeat" in one else -1)
    src = s.out()[0]
    s.close()
    t = Sess(net, 1, 2, how, lp=True).to(r2)
    t.st.load([0], state, clip_indices=[k2])
    given = None
    if key in ("given", "every"):
        given = np.random.default_rng(9).integers(0, net.V // 2, (2, 2))
        t.step(3, given=[given, None], **tkw)
    t.to(r2 + 6, **tkw)                                      # style=None: the loaded blend row stays in force
    got, lps = t.out()
    t.close()
    aud, u = clip_of(net, 1, r, 0, r2, 6)
    okw = {k: [v] for k, v in one.items()}
    if given is not None:
        okw["given"] = [given]
    head = src[1, :r]
    if key in ("style", "every"):
        okw["style"] = [net.blend]
    want = oracle(net, how, int(net.labels[1]), aud, u, head, k2, lp=True, **okw)
    assert np.array_equal(got[0, r2:], want[0]), f"{key} {how}: codes"
    assert np.array_equal(lps[0, r2:], want[1]), f"{key} {how}: log-probability bits"
    if given is not None:
        assert np.array_equal(got[0, r2:r2 + 2], given)
    if key == "repeat3":                                     # a presence of 1e30 bans the window's codes — the source's rows among them
        clip = np.concatenate([head, got[0, r2:]])
        for j in range(2):
            for x in range(r, r + 6):
                assert clip[x, j] not in clip[x - 3:x, j]


# ---- 6. portability -----------------------------------------------------------------------------------------------------------------------------------
def test_portability(nets):
    """Another handle of equal weights, another batch size, and the state as bytes through the host."""
    net = nets["S"]
    states, src = source(net, "S", "philox")
    r, r2, k2 = 7, 5, 88
    data = states[r].cpu().tobytes()
    back = SlotState.frombytes(data)
    assert back.device.type == "cpu" and back.infos == states[r].infos and torch.equal(back.words, states[r].words.cpu())
    outs = []
    for m, state in ((net.m2, back.to("cuda")), (net.m, states[r])):
        t = Sess(net, 1, 2, "philox", m=m).to(r2)
        t.st.load([0], state, clip_indices=[k2])
        t.to(r2 + 6)
        outs.append(t.out()[0])
        t.close()
    aud, u = clip_of(net, 1, r, 0, r2, 6)
    want = oracle(net, "philox", int(net.labels[1]), aud, u, src[1, :r], k2)[0]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0][0, r2:], want)


# ---- 7. graphs ------------------------------------------------------------------------------------------------------------------------------------------
def test_graphs(nets):
    net = nets["S"]
    states, _ = source(net, "S", "philox")                   # (the source's saves captured nothing and left its figures its twin's)
    warm = Sess(net, 1, 2, "philox", max_rows=3)
    warm.st.restart([1], [2], clip_indices=[9])
    for _ in range(5):                                       # buffer phases 0, 3 + 3, 3 + 2, 3 + 1, 3 + 0 on the restart keys
        warm.step(3)
    caps = warm.st.graph_captures()
    assert caps == 5
    for slots in ([0], [1, 0]):
        warm.st.load(slots, states[4], clip_indices=[60 + b for b in slots])
        warm.step(3).step(3)
    assert warm.st.graph_captures() == caps, "a load into a session on the restart keys captured a graph"
    warm.close()
    cold = Sess(net, 1, 2, "philox", max_rows=3)
    for _ in range(5):
        cold.step(3)
    assert cold.st.graph_captures() == 5
    cold.st.load([0], states[4], clip_indices=[60])          # the session's first load: the restart keys from here on
    for _ in range(4):
        cold.step(3)
    assert cold.st.graph_captures() == 9, "one capture per (Hc, buffer phase) of the four phases of rows >= 3"
    cold.st.load([1], states[8])
    for _ in range(4):
        cold.step(3)
    assert cold.st.graph_captures() == 9
    cold.close()


def test_graphs_off_same_bits():
    """The eager launches (TS_NO_GRAPH=1; the levers are read once per process -> child process)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                        "(test_continuation_small and philox) or test_rewind or test_fan_out"], env=dict(os.environ, TS_NO_GRAPH="1"),
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "10 passed" in r.stdout, r.stdout[-500:]


# ---- 8. BodyStream ------------------------------------------------------------------------------------------------------------------------------------
def test_body_stream_fork(nets):
    import bench
    from talkshow_amd import _lib
    net = nets["S"]
    w = bench.build_models(0, seed=7)[0]
    w.generator = net.m
    B, sched = 3, (3, 2, 4, 2)
    mf = torch.from_numpy(synth.mfcc_features(501, B, 4 * sum(sched))).cuda()
    mf[2] = mf[1]                                            # slot 2 will hear what slot 1 hears
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0)
    st = w.open_stream(torch.from_numpy(net.labels[:B]), B, 4 * max(sched))
    poses, codes, at = [], [], 0
    for i, hc in enumerate(sched):
        if i == 2:
            st.fork(1, [2])                                  # under the source's clip index: a twin
            assert list(st.slot_rows) == [at, at, at]
        if i == 3:
            st.fork(1, [0], clip_indices=[55])
        rows = w.audioencoder.forward_nlc(mf[:, 4 * at:4 * (at + hc)])
        poses.append(st.push(mf[:, 4 * at:4 * (at + hc)], **kw))
        codes.append(rows)
        at += hc
    got = torch.cat(poses, 1)
    t0 = 4 * sum(sched[:2])
    assert got.shape == (B, 4 * at, 129)
    assert torch.equal(got[2, t0:], got[1, t0:]), "the forked slot's poses differ from its source's over the next two pushes"
    assert not torch.equal(got[2, :t0], got[1, :t0])
    st.close()
    # its codes under another index: the chain session below it against the oracle
    n = sum(sched[:3])
    pix = net.m.open_stream(net.labels[:B], B, max(sched))
    rows = torch.cat(codes, 1)
    out = []
    for i, hc in enumerate(sched):
        s = sum(sched[:i])
        if i == 3:
            pix.fork(1, [0], clip_indices=[55])
        out.append(_np(pix.step(rows[:, s:s + hc], **kw)))
    pix.close()
    out = np.concatenate(out, 1)
    aud = torch.cat([rows[1, :n], rows[0, n:]])
    want = oracle(net, "philox", int(net.labels[1]), aud, None, out[1, :n], 55)[0]
    assert np.array_equal(out[0, n:], want)


# ---- 9. red zones round the state block ---------------------------------------------------------------------------------------------------------------
def test_save_writes_exactly_its_rows(nets):
    from talkshow_amd import _lib
    net = nets["S"]
    lib = _lib.load()
    s = Sess(net, 0, 3, "greedy").to(4)
    W = int(lib.ts_pixelcnn_slot_state_words(net.m.handle()))
    assert W == SlotClock.state_words(net.m.dim, net.m.n_layers) and lib.ts_pixelcnn_slot_state_words(None) == -1
    RZ, n, SENT = 1024, 2, 0x5A5A5A5A
    buf = torch.full((2 * RZ + n * W,), SENT, dtype=torch.int32, device="cuda")
    info = (_lib.TsSlotInfo * n)()
    _lib.check(lib.ts_pixelcnn_stream_save(s.st._h, (C.c_int32 * n)(2, 0), n, buf.data_ptr() + 4 * RZ, info, _lib.stream_ptr()))
    ref = s.st.save([2, 0])
    s.close()
    img = _np(buf)
    assert np.all(img[:RZ] == SENT) and np.all(img[RZ + n * W:] == SENT), "a red zone was written"
    assert np.array_equal(img[RZ:RZ + n * W].reshape(n, W), _np(ref.words))
    L = SlotClock.state_layout(net.m.dim, net.m.n_layers)
    assert np.all(_np(ref.words)[:, L["tok"] + 6:L["tok"] + 8] == 0) and np.all(_np(ref.words)[:, L["rep"]:] == -1)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_where_it_was(nets):
    from talkshow_amd import _lib
    net = nets["S"]
    states, _ = source(net, "S", "philox")
    full = Sess(nets["F"], 0, 2, "philox").to(3)
    other = full.st.save([0])                                # a state of another (D, NL, NC, V)
    full.close()
    t = Sess(net, 1, 3, "philox").to(2)
    st = t.st
    old = SlotState(states[5].words, [dict(states[5].infos[0], version=2)])
    both = SlotState(torch.cat([states[4].words, states[5].words]), states[4].infos + states[5].infos)
    bad = [("slot 3 is outside", dict(slots=[0, 3], state=states[1])), ("slot -1 is outside", dict(slots=[-1], state=states[1])),
           ("slot 1 is listed twice", dict(slots=[1, 2, 1], state=states[1])), ("3 slots but 2 states", dict(slots=[0, 1, 2], state=both)),
           ("slot 0: the state is of a network", dict(slots=[0], state=other)), ("slot 2: the state has layout version 2", dict(slots=[2], state=old)),
           ("slot 1: a clip of 3 rows cannot be loaded at session row 2", dict(slots=[0, 1], state=SlotState(both.words, [states[2].infos[0], states[3].infos[0]]))),
           ("slot 0: a clip of 8 rows cannot be loaded at session row 2", dict(slots=[0], state=states[8])),
           ("slot 2: clip index -4 is negative", dict(slots=[2], state=states[1], clip_indices=[-4])),
           ("slot 0: clip index -1 is negative", dict(slots=[0], state=states[0]))]
    for names, kw in bad:
        with pytest.raises(ValueError, match=names):
            st.load(**kw)
        assert st.rows == 2 and list(st.slot_rows) == [2, 2, 2], names
    with pytest.raises(ValueError, match="slot 3 is outside"):
        st.save([0, 3])
    with pytest.raises(ValueError, match="slot 1: clip index -2"):
        st.fork(0, [1], clip_indices=[-2])
    lib, h = _lib.load(), st._h                              # the C entries' own checks: the failing slot is named
    i32, i64 = C.c_int32 * 2, C.c_int64 * 2
    w45, inf = both.words, _c_info(both)
    low = SlotState(torch.cat([states[1].words, states[2].words]), states[1].infos + states[2].infos)     # clips the session's row 2 admits
    w12, inf12 = low.words, _c_info(low)

    def cload(slots, words, n_states, index, info, clips):
        return lib.ts_pixelcnn_stream_load(h, slots, 2, _lib.dptr(words), n_states, index, info, clips, _lib.stream_ptr())
    for names, call in [("slot 3 is outside", lambda: cload(i32(0, 3), w12, 2, None, inf12, i64(1, 2))),
                        ("slot 1 is listed twice", lambda: cload(i32(1, 1), w12, 2, None, inf12, i64(1, 2))),
                        ("slot 2: state index 2 is outside the 2 states", lambda: cload(i32(0, 2), w12, 2, i32(0, 2), inf12, i64(1, 2))),
                        ("2 slots but 3 states", lambda: cload(i32(0, 2), w12, 3, None, inf12, i64(1, 2))),
                        ("slot 0: the state is of a network", lambda: cload(i32(0, 2), other.words, 1, None, _c_info(other), i64(1, 2))),
                        ("slot 0: the state has layout version 2", lambda: cload(i32(0, 2), old.words, 1, None, _c_info(old), i64(1, 2))),
                        ("slot 0: a clip of 4 rows cannot be loaded at session row 2", lambda: cload(i32(0, 2), w45, 2, None, inf, i64(1, 2))),
                        ("slot 2: clip index -1 is negative", lambda: cload(i32(0, 2), states[1].words, 1, None, _c_info(states[1]), i64(1, -1))),
                        ("slot 0: clip index -1 is negative .the state records none", lambda: cload(i32(0, 2), states[0].words, 1, None, _c_info(states[0]), None)),
                        ("slot 5 is outside", lambda: lib.ts_pixelcnn_stream_save(h, i32(0, 5), 2, _lib.dptr(w45), inf, _lib.stream_ptr())),
                        ("null argument", lambda: lib.ts_pixelcnn_stream_save(h, i32(0, 1), 2, None, inf, _lib.stream_ptr()))]:
        with pytest.raises(RuntimeError, match=names):
            _lib.check(call())
        assert st.rows == 2 and list(st.slot_rows) == [2, 2, 2], names
    assert st.graph_captures() == 1
    st.load([0, 1], SlotState(both.words, [states[2].infos[0], states[1].infos[0]]), clip_indices=[5, 6])     # n = 2 at r' = 2 is accepted (this one
    assert list(st.slot_rows) == [2, 1, 2]                                                                   # only to show the rule's edge: the words are other rows')
    t.close()
    t = Sess(net, 1, 3, "philox").to(2)                      # and no refused call moved a bit: the session goes on as its twin
    for names, kw in bad[:3]:
        with pytest.raises(ValueError):
            t.st.load(**kw)
    t.to(8)
    assert np.array_equal(t.out()[0], target_twin(net, "S", "philox", 3, 12)[:, :8]) and t.st.graph_captures() == 3
    t.close()


def test_accepted_neighbour_of_the_row_rule(nets):
    """n = 2 at r' = 2 is accepted and right: the clip is as old as the session."""
    net = nets["S"]
    states, src = source(net, "S", "philox")
    for r, r2 in ((2, 2), (1, 1), (0, 0), (1, 2)):
        t = Sess(net, 1, 2, "philox").to(r2)
        t.st.load([0], states[r], clip_indices=[21])
        t.to(r2 + 5)
        got = t.out()[0]
        t.close()
        aud, u = clip_of(net, 1, r, 0, r2, 5)
        assert np.array_equal(got[0, r2:], oracle(net, "philox", int(net.labels[1]), aud, u, src[1, :r], 21)[0]), (r, r2)
        assert np.array_equal(got[1], target_twin(net, "S", "philox", 2, 12)[1, :r2 + 5])


def test_seamless_session_takes_no_state(nets):
    import bench
    w = bench.build_models(0, seed=7)[0]
    st = w.open_stream([0, 1], 2, 48, seamless=True)
    for call in (lambda: st.save([0]), lambda: st.load([0], None), lambda: st.fork(0, [1])):
        with pytest.raises(NotImplementedError, match="seamless"):
            call()
    st.close()
