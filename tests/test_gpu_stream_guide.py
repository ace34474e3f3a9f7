"""Session pairs on the chain's streaming session (`ts_pixelcnn_stream_pair`, `ts_pixelcnn_stream_step_guided`; `PixelCNNStream` with
`pairs=` and `step(guide=)`; include/talkshow_hip.h, "session pairs"): guidance at slot level inside a running session.

The yardstick is the one-shot `GatedPixelCNN.run(..., guide=)` on the pair alone: a primary's codes and log-probability bits equal it for
every chunking, in both drawing modes, alone and under every other piece of a step.  Every comparison is EQUALITY.  A session of S = 5
slots over 19 rows: pairs (0, 1) and (3, 4), slot 2 plain.  (S) the `pix_small` golden's network (V = 128: the samplers' general path);
(F) the full-size synthetic network (V = 2048: their vector path).  Every test fails on a build without the feature: the keywords and the
entries do not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, CLIP0 = 91, 3
S, H = 5, 19
PAIRS = {0: 1, 3: 4}
CHUNKS = [(19,), (1, 3, 15), (7, 12)]
HOWS = ["uniforms", "philox"]
PIECES = ["sampling", "code_bias", "repeat", "given", "style", "all"]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Net:
    def __init__(self, m, seed):
        self.m, self.V, self.NC = m, m.input_dim, m.n_classes
        rng = np.random.default_rng(seed)
        self.labels = (np.arange(S) * 3 + 1) % self.NC             # a shadow's label differs from its primary's
        assert self.labels[0] != self.labels[1] and self.labels[3] != self.labels[4]
        self.aud = rng.standard_normal((S, H, 256)).astype(F32)
        self.u = (0.999 * rng.random((S, H, 2))).astype(F32)
        V = self.V
        self.tables = []
        for _ in range(S):
            t = np.zeros((2, V), F32)
            t[:, rng.choice(V, V // 2, replace=False)] = -np.inf
            self.tables.append(t)
        self.sampling = [(0.8 + 0.1 * b, 0.9, V // 4 + b) for b in range(S)]
        self.repeat = [(16 - b, 0.5 + b, 0.25) for b in range(S)]
        self.given = [rng.integers(0, V, (g, 2)).astype(np.int64) for g in (5, 2, 9, 8, 0)]      # the clips' first rows
        self.style = [rng.random(self.NC).astype(F32) for _ in range(S)]

    def pieces(self, piece):
        """The per-slot values of the pieces a case runs under (a shadow's are never read, its style row apart)."""
        names = PIECES[:-1] if piece == "all" else [] if piece is None else [piece]
        return {k: getattr(self, "tables" if k == "code_bias" else k) for k in names}


def draw(net, how, slots, s, e, clip0=CLIP0):
    if how == "uniforms":
        return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(net.u[slots, s:e]))
    return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=clip0)


def step_kw(kw, s, e):
    """The pieces of the step over rows [s, e): `given` holds each clip's first rows, a step takes what falls inside it."""
    out = dict(kw)
    if "given" in kw:
        out["given"] = [g[s:min(e, len(g))] if len(g) > s else None for g in kw["given"]]
        if all(g is None for g in out["given"]):
            del out["given"]
    return out


def session(net, chunks, how, pairs=PAIRS, kw=None, scales=None, aud=None, labels=None, st=None):
    """The session over the chunking -> (codes (S, H, 2), log-probability bits, the handle).  scales: `guide=` of every step."""
    aud = net.aud if aud is None else aud
    st = st or net.m.open_stream(net.labels if labels is None else labels, S, max(chunks), pairs=pairs)
    codes, lps, at = [], [], 0
    for i, hc in enumerate(chunks):
        out = st.step(torch.from_numpy(aud[:, at:at + hc]).cuda(), **draw(net, how, slice(None), at, at + hc), logprobs=True,
                      guide=None if scales is None else scales[i], **step_kw(kw or {}, at, at + hc))
        codes.append(_np(out[0])), lps.append(_bits(out[1]))
        at += hc
        assert st.rows == at
    return np.concatenate(codes, 1), np.concatenate(lps, 1), st


def one_shot(net, how, b, g=None, scale=2.0, kw=None, aud=None, labels=None, head=None):
    """`run` on clip b alone (guided by slot g's conditioning) -> (codes (H, 2), log-probability bits); head: given rows ahead of kw's."""
    aud = net.aud if aud is None else aud
    labels = net.labels if labels is None else labels
    kw = {k: [v[b]] for k, v in (kw or {}).items()}
    guide = None
    if g is not None:
        guide = [{"scale": scale, "aud_rows": aud[g], "id": int(labels[g])}]
        if "style" in kw:
            guide[0]["style"] = net.style[g]
    if head is not None:
        kw["given"] = [head]
    d = draw(net, how, slice(b, b + 1), 0, H, clip0=CLIP0 + b)
    out = net.m.run(labels[b:b + 1], torch.from_numpy(aud[b:b + 1]).cuda(), **d, logprobs=True, guide=guide, **kw)
    return _np(out[0])[0], _bits(out[2])[0]


@pytest.fixture(scope="module")
def nets(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    full = GatedPixelCNN(2048, 256, 15, 4, True, True).cuda()
    full.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=7)))
    return {"S": Net(m, 11), "F": Net(full, 12)}


@pytest.fixture(scope="module")
def plain(nets):
    """The sessions without pairs, computed once: (net, how, piece) -> (codes, log-probability bits)."""
    memo = {}

    def get(name, how, piece=None):
        if (name, how, piece) not in memo:
            c, lp, st = session(nets[name], (7, 12), how, pairs=None, kw=nets[name].pieces(piece))
            st.close()
            memo[(name, how, piece)] = (c, lp)
        return memo[(name, how, piece)]
    return get


def check_session(net, c, lp, how, kw, plain_c, plain_lp, scale=2.0):
    for b, g in PAIRS.items():
        rc, rlp = one_shot(net, how, b, g, scale, kw)
        assert np.array_equal(c[b], rc), f"codes of primary {b}"
        assert np.array_equal(lp[b], rlp), f"log-probability bits of primary {b}"
        assert np.array_equal(c[g], c[b]) and np.array_equal(lp[g], lp[b]), f"shadow {g} holds its primary's rows"
        free = slice(len(kw["given"][b]) if "given" in kw else 0, None)
        assert (c[b, free] != plain_c[b, free]).any(), f"guidance moved no code of clip {b}: the equality would be vacuous"
    rc, rlp = one_shot(net, how, 2, None, kw=kw)
    assert np.array_equal(c[2], rc) and np.array_equal(lp[2], rlp), "the plain slot against the one-shot call"
    assert np.array_equal(c[2], plain_c[2]) and np.array_equal(lp[2], plain_lp[2]), "the plain slot against the session without pairs"


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "-".join(map(str, c)))
def test_a_paired_clip_equals_the_one_shot_guided_run(nets, plain, chunks, how):
    net = nets["S"]
    c, lp, st = session(net, chunks, how)
    assert st.pairs == {0: (1, 1.0), 3: (4, 1.0)}
    st.close()
    c, lp, st = session(net, chunks, how, pairs={0: (1, 2.0), 3: (4, 2.0)})
    st.close()
    check_session(net, c, lp, how, {}, *plain("S", how))


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("piece", PIECES)
def test_composed_with_every_piece_of_a_step(nets, plain, piece, chunks, how):
    net = nets["S"]
    kw = net.pieces(piece)
    c, lp, st = session(net, chunks, how, pairs={0: (1, 2.0), 3: (4, 2.0)}, kw=kw)
    st.close()
    check_session(net, c, lp, how, kw, *plain("S", how, piece))


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("piece", [None, "all"])
def test_the_vector_path_of_the_samplers(nets, plain, piece, how):
    net = nets["F"]
    kw = net.pieces(piece)
    c, lp, st = session(net, (7, 12), how, pairs={0: (1, 2.0), 3: (4, 2.0)}, kw=kw)
    st.close()
    check_session(net, c, lp, how, kw, *plain("F", how, piece))


@pytest.mark.parametrize("how", HOWS)
def test_scale_zero_returns_the_codes_of_the_session_without_pairs(nets, plain, how):
    net = nets["S"]
    c, _, st = session(net, (1, 3, 15), how, pairs={0: (1, 0.0), 3: (4, 2.0)}, scales=[None, {3: 0.0}, {3: 0}])
    st.close()
    pc, _ = plain("S", how)
    assert np.array_equal(c[0], pc[0]) and np.array_equal(c[1], pc[0])
    assert np.array_equal(c[3, 1:], one_shot(net, how, 3, 4, 0.0, head=c[3, :1])[0][1:])      # scale 2 for one row, then off
    assert np.array_equal(c[2], pc[2])


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("scale", [2.0, -0.5])
def test_a_shadow_with_its_primarys_conditioning_changes_no_bit(nets, plain, scale, how):
    net = nets["S"]
    aud, labels = net.aud.copy(), net.labels.copy()
    aud[1], labels[1], aud[4], labels[4] = aud[0], labels[0], aud[3], labels[3]
    c, lp, st = session(net, (7, 12), how, pairs={0: (1, scale), 3: (4, scale)}, aud=aud, labels=labels)
    st.close()
    pc, plp = plain("S", how)
    for b in (0, 2, 3):
        assert np.array_equal(c[b], pc[b]) and np.array_equal(lp[b], plp[b]), b


@pytest.mark.parametrize("how", HOWS)
def test_a_steps_scale_equals_the_one_shot_with_the_scale_changed_at_that_row(nets, how):
    net = nets["S"]
    c, lp, st = session(net, (7, 12), how, pairs={0: (1, 2.0), 3: (4, 2.0)}, scales=[None, {0: -0.5}])
    assert st.pairs == {0: (1, 2.0), 3: (4, 2.0)}            # a step's scale is not stored
    st.close()
    first, _ = one_shot(net, how, 0, 1, 2.0)
    assert np.array_equal(c[0, :7], first[:7])
    rc, rlp = one_shot(net, how, 0, 1, -0.5, head=first[:7])
    assert np.array_equal(c[0, 7:], rc[7:]) and np.array_equal(lp[0, 7:], rlp[7:])
    assert (rc[7:] != first[7:]).any()
    rc, rlp = one_shot(net, how, 3, 4, 2.0)                  # the other pair kept its stored scale
    assert np.array_equal(c[3], rc) and np.array_equal(lp[3], rlp)


def test_graph_captures_stand_still(nets):
    net = nets["S"]
    st = net.m.open_stream(net.labels, S, 4, pairs={0: (1, 2.0), 3: (4, 2.0)})
    twin = net.m.open_stream(net.labels, S, 4)
    seen, at = [], 0
    for i in range(4):
        a = torch.from_numpy(net.aud[:, at:at + 4]).cuda()
        st.step(a, **draw(net, "philox", slice(None), at, at + 4), guide=None if i % 2 else float(i))
        twin.step(a, **draw(net, "philox", slice(None), at, at + 4))
        seen.append((st.graph_captures(), twin.graph_captures()))
        at += 4
    assert seen[1] == seen[2] == seen[3], seen                # one graph per (rows, buffer phase, kind of sampler): roles and scales are in no key
    assert seen[3][0] == seen[3][1], seen                     # as many as the session without pairs captures
    st.close(), twin.close()


def test_refusals_launch_nothing_and_move_no_row(nets):
    net = nets["S"]
    st = net.m.open_stream(net.labels, S, 12, pairs={0: (1, 2.0), 3: (4, 2.0)})
    a7 = torch.from_numpy(net.aud[:, :7]).cuda()
    with pytest.raises(RuntimeError, match="per-clip greedy is top_k = 1"):
        st.step(a7, mode=_lib.TS_SAMPLE_GREEDY)
    for bad, text in [({1: 2.0}, "slot 1 is no primary"), ({0: float("nan")}, "slot 0: the scale is NaN"),
                      ([None, None, None, 1e5, None], "slot 3: the scale exceeds 1e4"), (float("inf"), "slot 0: the scale is infinite")]:
        with pytest.raises(ValueError, match=text):
            st.step(a7, **draw(net, "philox", slice(None), 0, 7), guide=bad)
    with pytest.raises(ValueError, match="slot 0 is paired with slot 1"):
        st._declare([0], [2], [1.0])                           # the library's own check, behind the wrapper's
    with pytest.raises(ValueError, match="slot 2 names itself"):
        st._declare([2], [2], [1.0])
    assert st.rows == 0 and st.graph_captures() == 0 and st.pairs == {0: (1, 2.0), 3: (4, 2.0)}
    c, lp, st = session(net, (7, 12), "philox", st=st)         # and the session is where it was
    st.close()
    rc, rlp = one_shot(net, "philox", 0, 1, 2.0)
    assert np.array_equal(c[0], rc) and np.array_equal(lp[0], rlp)
    for bad in ({0: 0}, {0: 7}, {0: (1, float("nan"))}, {0: 1, 2: 1}, {0: 1, 1: 2}):
        with pytest.raises(ValueError, match="session pairs: "):
            net.m.open_stream(net.labels, S, 4, pairs=bad)
    st = net.m.open_stream(net.labels, S, 4)
    with pytest.raises(ValueError, match="the session holds no pair"):
        st.step(torch.from_numpy(net.aud[:, :4]).cuda(), guide=2.0)
    st.step(torch.from_numpy(net.aud[:, :4]).cuda())
    with pytest.raises(ValueError, match="cannot pair at session row 4"):
        st._declare([0], [1], [1.0])                           # no pairing in the middle of a clip
    assert st.pairs == {}
    st.close()
