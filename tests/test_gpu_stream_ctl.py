"""Per-clip sampling controls on the streaming sessions (`ts_pixelcnn_stream_step_ctl`; the keywords of `PixelCNNStream.step` and
`BodyStream.push`; include/talkshow_hip.h, "streaming sessions").

The yardstick throughout is the one-shot `GatedPixelCNN.run(..., sampling=, logprobs=, given=, given_keep=, style=, code_bias=, repeat=)`
with the same seed and clip_index0: both routes launch the same sampler kernels on the same logits at the same absolute positions, so
every comparison is EQUALITY of codes and of log-probability bits.  The one exception is `from_row` (test 6): no one-shot call has an
empty history mid-clip, so the yardstick there is the numpy restatement `sampling.sample_repeat` on the network's own teacher-forced
logits — codes equal, log-probabilities equal or adjacent float32 (the accuracy `sampling.logprob` states).

Shapes: (S) the `pix_small` golden's network (V = 128: the generic sampler path) at B = 3, H = 10; (F) the full-size synthetic network
(V = 2048: the register path) at B = 2, H = 9; (W) (S)'s network at B = 33, H = 6 on random audio rows (across the 16- and 32-row slab
edges).  Every test fails on a build without the feature: `step()` has no such keywords and the library no such symbol.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
RECS = [(0.8, 0.9, 0), (1.3, 1.0, 5), None]
REPS = [(3, 0.7, 0.3), (5, 1.0, 0.5), (0, 1.0, 1.0)]
SCHEDULES = {"ragged": (3, 1, 4, 2), "rows": None, "whole": "H"}


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _fit(sched, H):
    """`sched` cut to H rows in all (a schedule written for H = 10 serves the shorter cases)."""
    if sched is None:
        return (1,) * H
    if sched == "H":
        return (H,)
    out, at = [], 0
    for hc in sched:
        if at >= H:
            break
        out.append(min(hc, H - at))
        at += out[-1]
    if at < H:
        out.append(H - at)
    return tuple(out)


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
        self.tables = (t0, t1)
        self.sampling = [RECS[b % 3] for b in range(B)]
        self.bias = [(t0, t1, None)[b % 3] for b in range(B)]                # shared objects: two tables travel
        self.repeat = [REPS[b % 3] for b in range(B)]
        self.style = [rng.random(self.NC).astype(F32) for _ in range(B)]     # a blend per clip
        self.u = (0.999 * rng.random((B, self.H, 2))).astype(F32)

    def every(self):
        return dict(sampling=self.sampling, code_bias=self.bias, repeat=self.repeat, style=self.style)

    def draw(self, how):
        from talkshow_amd import _lib
        if how == "uniforms":
            return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=self.u)
        return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=5)

    def one_shot(self, how, aud=None, **kw):
        """(codes, logprobs) of the one call, or codes alone without `logprobs`."""
        out = self.m.run(self.label, self.aud if aud is None else aud, **self.draw(how), **kw)
        return (_np(out[0]), _bits(out[2])) if len(out) == 3 else _np(out[0])

    def stepped(self, how, sched, per_step=None, aud=None, open_kw=None, **kw):
        """The same rows through a session in the chunks of `sched`; per_step: step index -> keywords of that step in place of `kw`."""
        aud = self.aud if aud is None else aud
        d = self.draw(how)
        st = self.m.open_stream(self.label, self.B, max(sched), **(open_kw or {}))
        codes, lps, at = [], [], 0
        for k, hc in enumerate(sched):
            dk = dict(d)
            if "uniforms" in dk:
                dk["uniforms"] = np.ascontiguousarray(dk["uniforms"][:, at:at + hc])
            kk = kw if per_step is None or k not in per_step else per_step[k]
            out = st.step(aud[:, at:at + hc], **dk, **kk)
            if isinstance(out, tuple):
                codes.append(_np(out[0])), lps.append(_bits(out[1]))
            else:
                codes.append(_np(out))
            at += hc
        assert st.rows == at
        st.close()
        codes = np.concatenate(codes, 1)
        return (codes, np.concatenate(lps, 1)) if lps else codes


@pytest.fixture(scope="module")
def small_net(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    return m, g


@pytest.fixture(scope="module")
def cases(small_net):
    from talkshow_amd.modules import GatedPixelCNN
    m, g = small_net
    assert m.input_dim == 128 and g["aud"].shape[:2] == (3, 10)
    full = GatedPixelCNN(2048, 256, 15, 4, True, True).cuda()
    full.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=7)))
    rng = np.random.default_rng(60)
    return {"S": Case(m, g["label"], g["aud"], 1),
            "F": Case(full, synth.speaker_ids(2), rng.standard_normal((2, 9, 256)).astype(F32), 2),
            "W": Case(m, np.arange(33) % m.n_classes, rng.standard_normal((33, 6, 256)).astype(F32), 3)}


_REF = {}


def _reference(c, name, how):
    """The one-shot call with every keyword on, once per (case, draw mode); nobody changes it."""
    if (name, how) not in _REF:
        _REF[(name, how)] = c.one_shot(how, logprobs=True, **c.every())
    return _REF[(name, how)]


# ---- 1. chunked equals one-shot, every keyword on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("how", ["philox", "uniforms"])
@pytest.mark.parametrize("name", ["S", "F", "W"])
def test_chunked_equals_one_shot_every_keyword_on(cases, name, how, sched):
    c = cases[name]
    want = _reference(c, name, how)
    plain = c.one_shot(how)
    assert not np.array_equal(plain, want[0]), "the keywords change nothing here: the comparison would show nothing"
    got = c.stepped(how, _fit(SCHEDULES[sched], c.H), logprobs=True, **c.every())
    assert np.array_equal(got[0], want[0]), f"{name} {how} {sched}: first differing row {np.flatnonzero((got[0] != want[0]).any((0, 2)))[:1]}"
    assert np.array_equal(got[1], want[1]), f"{name} {how} {sched}: log-probability bits differ"
    for b in range(c.B):                                                   # the tables held: no banned code was drawn
        if c.bias[b] is not None:
            for j in range(2):
                assert np.all(np.isfinite(c.bias[b][j][got[0][b, :, j]]))


# ---- 2. keywords one at a time ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["sampling", "logprobs", "given", "style", "code_bias", "repeat"])
def test_keywords_one_at_a_time(cases, key):
    c = cases["S"]
    sched = (3, 1, 4, 2)
    if key == "logprobs":
        want, got = c.one_shot("philox", logprobs=True), c.stepped("philox", sched, logprobs=True)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
        assert np.array_equal(want[0], c.one_shot("philox"))
        return
    if key == "given":                                                     # rows of the first step: a one-shot call gives a clip's HEAD
        rng = np.random.default_rng(8)
        given = [None, rng.integers(0, c.V, (2, 2)), rng.integers(0, c.V, (3, 2))]
        want = c.one_shot("philox", given=given, logprobs=True)
        got = c.stepped("philox", sched, per_step={0: dict(given=given, logprobs=True)}, logprobs=True)
        assert np.array_equal(got[0][1, :2], given[1]) and np.array_equal(got[0][2, :3], given[2])
    else:
        kw = {key: c.every()[key]}
        want, got = c.one_shot("philox", logprobs=True, **kw), c.stepped("philox", sched, logprobs=True, **kw)
        assert not np.array_equal(want[0], c.one_shot("philox")), f"{key} alone changes nothing here"
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), key


# ---- 3. records that change between steps -----------------------------------------------------------------------------------------------------
def test_records_change_between_steps(cases):
    """Step 1 (rows [0, 4)) under set 1, step 2 under set 2 == run(given = step 1's codes, set 2) from row 4 on: given rows enter the row
    cache and the history and draw nothing.  Every window is positive in both sets (a clip without a record in step 1 would start step 2
    from an empty history: test 6)."""
    c = cases["S"]
    a, H = 4, c.H
    set1 = dict(sampling=[(1.3, 1.0, 5), None, (0.8, 0.9, 0)], repeat=[(5, 1.0, 0.5), (2, 0.3, 0.0), (64, 0.5, 0.1)])
    set2 = dict(sampling=c.sampling, repeat=[(3, 0.7, 0.3), (5, 1.0, 0.5), (1, 2.0, 0.0)])
    for how in ("philox", "uniforms"):
        got = c.stepped(how, (a, H - a), per_step={0: dict(logprobs=True, **set1), 1: dict(logprobs=True, **set2)})
        want = c.one_shot(how, given=got[0][:, :a], logprobs=True, **set2)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1][:, a:], got[1][:, a:]), how
        same = c.stepped(how, (a, H - a), logprobs=True, **set2)
        assert not np.array_equal(same[0][:, :a], got[0][:, :a]), "set 1 draws what set 2 draws: the comparison would show nothing"


def test_bias_tables_change_between_steps(cases):
    c = cases["S"]
    a, H = 4, c.H
    t0, t1 = c.tables
    set1, set2 = dict(code_bias=[t1, None, t0]), dict(code_bias=[t0, t1, None])
    got = c.stepped("philox", (a, H - a), per_step={0: dict(logprobs=True, **set1), 1: dict(logprobs=True, **set2)})
    want = c.one_shot("philox", given=got[0][:, :a], logprobs=True, **set2)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1][:, a:], got[1][:, a:])
    assert np.all(np.isfinite(t1[0][got[0][0, :a, 0]])) and np.all(np.isfinite(t0[0][got[0][0, a:, 0]]))


def test_style_handed_over_between_steps(cases):
    """Style rows of step 1 stay through step 2 (no style keyword) and change at step 3; the one-shot call takes per-row tracks that are
    constant over each step's rows.  A one-hot row is the label."""
    c = cases["S"]
    sched = (3, 4, 3)
    rng = np.random.default_rng(4)
    s1 = [rng.random(c.NC).astype(F32) for _ in range(c.B)]
    s3 = [rng.random(c.NC).astype(F32) for _ in range(c.B)]
    tracks = [np.stack([s1[b]] * 7 + [s3[b]] * 3) for b in range(c.B)]
    got = c.stepped("philox", sched, per_step={0: dict(style=s1, logprobs=True), 1: dict(logprobs=True), 2: dict(style=s3, logprobs=True)})
    want = c.one_shot("philox", style=tracks, logprobs=True)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    assert not np.array_equal(got[0], c.one_shot("philox"))
    hot = list(np.eye(c.NC, dtype=F32)[c.label])
    assert np.array_equal(c.stepped("philox", sched, style=hot), c.one_shot("philox"))


# ---- 4. given rows in the middle --------------------------------------------------------------------------------------------------------------
def test_given_rows_in_the_middle(cases):
    c = cases["S"]
    sched, g = (3, 4, 3), [0, 2, 4]
    rng = np.random.default_rng(12)
    block = rng.integers(0, c.V, (c.B, 4, 2))
    full = np.full((c.B, c.H, 2), c.V + 7, np.int64)                       # unkept entries: outside the vocabulary, never read
    keep = np.zeros((c.B, c.H, 2), np.uint8)
    for b in range(c.B):
        full[b, 3:3 + g[b]] = block[b, :g[b]]
        keep[b, 3:3 + g[b]] = 1
    given = [None if g[b] == 0 else block[b, :g[b]] for b in range(c.B)]
    for extra in (dict(), dict(sampling=c.sampling, repeat=(5, 1.0, 0.5))):
        for how in ("philox", "uniforms"):
            got = c.stepped(how, sched, per_step={1: dict(given=given, logprobs=True, **extra)}, logprobs=True, **extra)
            want = c.one_shot(how, given=full, given_keep=keep, logprobs=True, **extra)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), (how, sorted(extra))
            for b in range(c.B):
                assert np.array_equal(got[0][b, 3:3 + g[b]], block[b, :g[b]])


# ---- 5. the history across seams and around the ring ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [(64, 0.7, 0.2), (16, 1e30, 0.0)])
def test_history_across_seams_and_around_the_ring(cases, rep):
    c = cases["S"]
    B, H = 2, 70
    aud = torch.from_numpy(np.random.default_rng(70).standard_normal((B, H, 256)).astype(F32)).cuda()
    c2 = Case(c.m, c.label[:B], aud, 5)
    want = c2.one_shot("philox", repeat=rep, logprobs=True)
    got = c2.stepped("philox", (7,) * 10, repeat=rep, logprobs=True)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    assert not np.array_equal(got[0], c2.one_shot("philox"))
    if rep[0] == 16:
        for b in range(B):
            for j in range(2):
                col = got[0][b, :, j]
                for r in range(H):
                    assert col[r] not in col[max(0, r - 16):r], f"clip {b} column {j}: row {r} repeats a code of the last 16 rows"


# ---- 6. from_row ----------------------------------------------------------------------------------------------------------------------------------
def _replay(c, aud, u, codes, lp, rep, from_row, rows):
    """Rows `rows` of a session's codes through `sampling.sample_repeat` on the network's teacher-forced logits, the history cut at from_row."""
    from talkshow_amd import _lib
    _, logits = c.m.run(c.label, aud, mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)
    logits = _np(logits)
    for b in range(codes.shape[0]):
        for r in rows:
            R = min(r, 64)
            for j in range(2):
                hist = codes[b, r - R:r, j].copy()
                hist[:max(0, from_row - (r - R))] = -1                          # entries of rows before from_row: never counted
                i, _, l, _ = S.sample_repeat(logits[b, r, j][None], [u[b, r, j]], None, rep, hist[None], 2 * r + j, column=j)
                assert i[0] == codes[b, r, j], f"clip {b} row {r} column {j}: the session drew {codes[b, r, j]}, the restatement {i[0]}"
                want = np.asarray(l[0], F32)
                assert abs(float(lp[b, r, j]) - float(want)) <= np.spacing(np.abs(want)), (b, r, j)


def test_penalty_switched_on_mid_session_starts_from_an_empty_history(cases):
    from talkshow_amd import _lib
    c = cases["S"]
    B, H, rep = 2, 20, (8, 1.0, 0.5)
    rng = np.random.default_rng(90)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    c2 = Case(c.m, c.label[:B], aud, 6)
    on = dict(repeat=rep, logprobs=True)
    codes, lpb = c2.stepped("uniforms", (5,) * 4, per_step={0: dict(logprobs=True), 1: dict(logprobs=True), 2: on, 3: on})
    plain = c2.one_shot("uniforms")
    assert np.array_equal(codes[:, :10], plain[:, :10]) and not np.array_equal(codes[:, 10:], plain[:, 10:])
    _replay(c2, aud, c2.u, codes, lpb.view(F32), rep, 10, range(10, 20))
    whole = c2.one_shot("uniforms", given=codes[:, :10], repeat=rep)          # a history that starts at row 0 draws something else
    assert not np.array_equal(whole[:, 10:], codes[:, 10:]), "the rows before from_row do not matter here: pick another seed"


def test_penalty_dropped_and_brought_back_counts_nothing_from_before_the_gap(cases):
    c = cases["S"]
    B, rep = 2, (8, 1.0, 0.5)
    sched = (5,) + (7,) * 10 + (5,)
    H = sum(sched)
    rng = np.random.default_rng(91)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    c2 = Case(c.m, c.label[:B], aud, 7)
    on = dict(repeat=rep, logprobs=True)
    codes, lpb = c2.stepped("uniforms", sched, per_step={0: on, len(sched) - 1: on}, logprobs=True)
    head = c2.one_shot("uniforms", repeat=rep)
    assert np.array_equal(codes[:, :5], head[:, :5])
    _replay(c2, aud, c2.u, codes, lpb.view(F32), rep, 75, range(75, 80))


# ---- 7. defaults and graphs -----------------------------------------------------------------------------------------------------------------------
def test_defaults_and_graphs(cases):
    from talkshow_amd import _lib
    c = cases["S"]
    B, H = c.B, 20
    aud = torch.from_numpy(np.random.default_rng(20).standard_normal((B, H, 256)).astype(F32)).cuda()
    c2 = Case(c.m, c.label, aud, 8)
    assert np.array_equal(c2.stepped("philox", (4,) * 5), c2.one_shot("philox"))       # no keyword: the step there always was
    d = c2.draw("philox")
    st = c.m.open_stream(c.label, B, 4)
    assert st.graph_captures() == 0
    plain = [st.step(aud[:, 0:4], **d), st.step(aud[:, 4:8], **d)]
    caps = st.graph_captures()
    assert caps == 2                                                                   # buffer phases 0 and 3 + 0
    t0, t1 = c.tables
    st.step(aud[:, 8:12], **d, sampling=c.sampling, code_bias=[t0, t1, None], repeat=c.repeat, style=c.style, logprobs=True)
    assert st.graph_captures() == caps + 1, "a controlled step runs on a graph of its own"
    st.step(aud[:, 12:16], **d, sampling=(0.5, 0.7, 9), code_bias=[None, t0, t0], repeat=(9, 0.1, 0.1), style=c.style[::-1], logprobs=True)
    assert st.graph_captures() == caps + 1, "other records, tables and style: the same graph"
    st.step(aud[:, 16:20], **d)
    assert st.graph_captures() == caps + 1, "the plain step's graph stayed in place"
    st.close()
    assert np.array_equal(_np(torch.cat(plain, 1)), c2.one_shot("philox")[:, :8])
    # session defaults: a step without the keyword runs under them, a step with the keyword under its own value
    kw = dict(sampling=c.sampling, repeat=c.repeat)
    want = c2.one_shot("philox", logprobs=True, **kw)
    got = c2.stepped("philox", (4,) * 5, open_kw=kw, logprobs=True)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    got = c2.stepped("philox", (4,) * 5, open_kw=dict(sampling=(0.1, 0.2, 3), repeat=(64, 9.0, 9.0)), logprobs=True, **kw)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


# ---- 8. BodyStream.push ---------------------------------------------------------------------------------------------------------------------------
def test_body_stream_push_with_all_keywords(cases):
    """`push` under every keyword returns `_decode_pair` of the codes the one-shot call gives on the same audio rows (the yardstick of test
    1), chunk by chunk, bit for bit, and the log-probabilities."""
    import bench
    c = cases["S"]
    w = bench.build_models(0, seed=7)[0]
    w.generator = c.m
    sched = (3, 1, 4, 2)
    mf = torch.from_numpy(synth.mfcc_features(500, c.B, 4 * c.H)).cuda()
    rows = torch.cat([w.audioencoder.forward_nlc(mf[:, 4 * a:4 * (a + hc)]) for a, hc in zip(np.cumsum((0,) + sched[:-1]), sched)], 1)
    want = c.one_shot("philox", aud=rows, logprobs=True, **c.every())
    d = c.draw("philox")
    session = w.open_stream(torch.from_numpy(c.label), c.B, 4 * max(sched))
    at = 0
    for hc in sched:
        poses, lp = session.push(mf[:, 4 * at:4 * (at + hc)], **d, logprobs=True, **c.every())
        codes = torch.from_numpy(want[0][:, at:at + hc]).cuda()
        assert poses.shape == (c.B, 4 * hc, 129) and torch.equal(poses, w._decode_pair(codes)), f"rows {at} .. {at + hc}"
        assert np.array_equal(_bits(lp), want[1][:, at:at + hc])
        at += hc
    assert session.frames == 4 * c.H
    session.close()
