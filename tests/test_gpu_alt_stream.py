"""Alternatives on a streaming session (`ts_pixelcnn_stream_step_alt`; `alternatives=` on `PixelCNNStream.step` and as an `open_stream`
default): 3 slots, 9 code rows stepped 4 + 1 + 4 under sampling records, a bias table and repetition records equal the one-shot
`GatedPixelCNN.run` bit for bit — codes, log-probabilities and all four outputs of the keyword; the session captures nothing after its
first round; a step without the keyword is the step it was.  The small network of the quick tests.  Every test fails on a build without
the feature: the keyword and the entry do not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = dict(input_dim=256, dim=64, n_layers=3)
V, NC, B, H, N = DIMS["input_dim"], 4, 3, 9, 3
SCHED = [4, 1, 4]


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_alt(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _cat(alts):
    return S.Alternatives(*(torch.cat([getattr(a, f) for a in alts], 1) for f in S.Alternatives._fields))


@pytest.fixture(scope="module")
def net():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=11, **DIMS)))
    return m


@pytest.fixture(scope="module")
def case(net):
    rng = np.random.default_rng(77)
    aud = torch.from_numpy(rng.standard_normal((B, H, net.aud_dim)).astype(F32)).cuda()
    label = np.array([0, 2, 3], np.int64)
    allow = S.allow_bias((rng.choice(V, 30, replace=False), rng.choice(V, 2, replace=False)), V)
    kw = dict(sampling=[(0.8, 0.9, 0), (1.0, 1.0, 1), (1.7, 1.0, 12)], code_bias=[None, allow, None], repeat=[(3, 0.7, 0.3), (64, 0.5, 0.0), None])
    return aud, label, kw, rng.random((B, H, 2)).astype(F32)


def _steps(st, aud, draw, u=None, **kw):
    outs, at = [], 0
    for hc in SCHED:
        d = dict(draw)
        if u is not None:
            d["uniforms"] = torch.from_numpy(np.ascontiguousarray(u[:, at:at + hc])).cuda()
        outs.append(st.step(aud[:, at:at + hc], **d, **kw))
        at += hc
    return outs


@pytest.mark.parametrize("how", ["philox", "uniforms"])
def test_stepped_equals_one_shot(net, case, how):
    from talkshow_amd import _lib
    aud, label, kw, u = case
    if how == "philox":
        draw, ukw, u_steps = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=31, clip_index0=9), {}, None
    else:
        draw, ukw, u_steps = dict(mode=_lib.TS_SAMPLE_UNIFORMS), dict(uniforms=torch.from_numpy(u).cuda()), u
    codes, _, lp, alt = net.run(label, aud, logprobs=True, alternatives=N, **draw, **ukw, **kw)
    plain = net.run(label, aud, logprobs=True, **draw, **ukw, **kw)
    assert _same(codes, plain[0]) and _same(lp, plain[2])
    st = net.open_stream(label, B, max(SCHED))
    outs = _steps(st, aud, draw, u_steps, logprobs=True, alternatives=N, **kw)
    assert all(len(o) == 3 for o in outs)
    assert _same(torch.cat([o[0] for o in outs], 1), codes) and _same(torch.cat([o[1] for o in outs], 1), lp)
    assert _same_alt(_cat([o[2] for o in outs]), alt), f"{how}: the stepped alternatives differ from the one-shot call's"
    st.close()


def test_graphs_stand_still_and_the_plain_step_is_the_step_it_was(net, case):
    from talkshow_amd import _lib
    aud, label, kw, _ = case
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=5, clip_index0=0)
    ref = net.open_stream(label, B, 4)
    want = [ref.step(aud[:, 0:4], **draw), ref.step(aud[:, 4:8], **draw)]
    ref.close()
    st = net.open_stream(label, B, 4, alternatives=N)                    # the session default
    a0 = st.step(aud[:, 0:4], **draw)
    a1 = st.step(aud[:, 4:8], **draw)
    assert len(a0) == 2 and isinstance(a0[1], S.Alternatives) and tuple(a0[1].codes.shape) == (B, 4, 2, N)
    assert _same(a0[0], want[0]) and _same(a1[0], want[1]), "neutral records with alternatives: the plain step's codes"
    st.step(aud[:, 0:4], **draw, **kw)                                   # rows 8 .. 11 (the buffer phase of rows 4 .. 7) under tables and records
    caps = st.graph_captures()
    st.step(aud[:, 4:8], **draw, sampling=(0.5, 0.7, 9), code_bias=kw["code_bias"][::-1], repeat=(9, 0.1, 0.1))      # other values, the same kinds
    st.step(aud[:, 0:4], **draw)
    assert st.graph_captures() == caps, "a step with alternatives captured a graph after the first round"
    st.close()
    st = net.open_stream(label, B, 4)
    got = [st.step(aud[:, 0:4], **draw, alternatives=None), st.step(aud[:, 4:8], **draw)]
    assert torch.is_tensor(got[0]) and _same(got[0], want[0]) and _same(got[1], want[1])
    with pytest.raises(ValueError):
        st.step(aud[:, 0:4], mode=_lib.TS_SAMPLE_GREEDY, alternatives=N)
    with pytest.raises(ValueError):
        st.step(aud[:, 0:4], **draw, alternatives=9)
    assert st.rows == 8
    st.close()
    with pytest.raises(NotImplementedError):
        net.open_stream(label, B, 4, pairs={0: 1}, alternatives=N)
    paired = net.open_stream(label, B, 4, pairs={0: 1})
    with pytest.raises(NotImplementedError):
        paired.step(aud[:, 0:4], **draw, alternatives=N)
    assert paired.rows == 0
    paired.close()
