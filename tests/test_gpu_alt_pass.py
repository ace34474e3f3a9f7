"""Alternatives through the body decode (`ts_body_pixel_infer_alt`, `ts_pixelcnn_generate_alt`; `alternatives=` on
`GatedPixelCNN.run` and `TrainWrapper.generate_clips / generate_batch / generate_clips_from_wav`).

The rule (include/talkshow_hip.h, "alternatives"): the n best allowed codes with their log-probabilities, the entropy and the rank of
every position's code, under the distribution the filters are applied to, from the sampler launch itself.  Every check is EQUALITY, or
the restatement's one fp32 spacing for the two values behind an fp64 log.  The PixelCNN is the small network of the quick tests
(input_dim 256, dim 64, n_layers 3) inside the shipped wrapper; clips of 17, 9 and 3 code rows, submitted shuffled: the borders of the
8-row chunks are crossed and one clip is shorter than a chunk.  One pass runs on the full-size network (V = 2048: the vector path of the
kernels inside a pass).  Every test fails on a build without the feature: the keyword and the entries do not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = dict(input_dim=256, dim=64, n_layers=3)
V, NC = DIMS["input_dim"], 4
ROWS = [17, 9, 3]
RECS = [(0.8, 0.9, 0), (1.7, 1.0, 12), (1.0, 1.0, 1)]
REPS = [(5, 0.7, 0.3), None, (64, 0.5, 0.25)]
N = 3


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """Two results of one clip: tensors, with a `sampling.Alternatives` compared field by field."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, S.Alternatives):
            if not (isinstance(y, S.Alternatives) and same(tuple(x), tuple(y))):
                return False
        elif not np.array_equal(_bits(x), _bits(y)):
            return False
    return True


def one_spacing(got, want):
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    inf = np.isinf(want)
    ok = np.abs(got[~inf].astype(np.float64) - want[~inf].astype(np.float64)) <= np.spacing(np.abs(want[~inf])).astype(np.float64)
    return bool((got[inf] == want[inf]).all() and ok.all())


@pytest.fixture(scope="module")
def pix():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=11, **DIMS)))
    return m


@pytest.fixture(scope="module")
def wrappers(pix):
    """(the shipped wrapper around the small code predictor, the full-size code predictor it shipped with)."""
    import bench
    wr = bench.build_models(0, seed=7)[0]
    full = wr.generator
    wr.generator = pix
    return wr, full


@pytest.fixture(scope="module")
def w(wrappers):
    return wrappers[0]


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(23)
    order = rng.permutation(len(ROWS))               # submitted shuffled: the Python layer sorts and un-sorts
    rows = [ROWS[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(3100 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    allow = S.allow_bias((rng.choice(V, 40, replace=False), rng.choice(V, 2, replace=False)), V)      # the hand column keeps 2 codes: padding for n = 3
    return rows, mf, ids, [RECS[i] for i in order], [REPS[i] for i in order], [[None, allow, None][i] for i in order]


def _pieces(_lib, clips, how):
    rows, mf, ids, recs, reps, bias = clips
    kw = dict(sampling=recs, repeat=reps, code_bias=bias)
    if how == "uniforms":
        rng = np.random.default_rng(31)
        kw.update(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=[rng.random((h, 2)).astype(F32) for h in rows])
    else:
        kw.update(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50)
    return kw


@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_keyword_moves_no_bit_and_a_clip_is_the_clip_alone(w, pix, clips, how):
    from talkshow_amd import _lib
    rows, mf, ids, recs, reps, bias = clips
    kw = _pieces(_lib, clips, how)
    first = w.generate_clips(mf, ids, logprobs=True, **kw)
    long_clip = int(np.argmax(rows))
    given = [None] * len(rows)
    given[long_clip] = _np(first[long_clip][0])[:11]                      # eleven rows back: across the first chunk border
    keep = [None] * len(rows)
    keep[long_clip] = "body"
    kw.update(given=given, given_keep=keep)
    plain = w.generate_clips(mf, ids, logprobs=True, **kw)
    caps = pix.graph_captures()
    assert all(same(a, b) for a, b in zip(w.generate_clips(mf, ids, logprobs=True, alternatives=None, **kw), plain))
    assert pix.graph_captures() == caps, "alternatives=None captured a graph"
    got = w.generate_clips(mf, ids, logprobs=True, alternatives=N, **kw)
    for b in range(len(rows)):
        assert len(got[b]) == 4 and same(got[b][:3], plain[b]), f"{how}: clip {b}: codes, poses or log-probabilities moved"
        alt = got[b][3]
        assert tuple(alt.codes.shape) == (rows[b], 2, N) and tuple(alt.logprobs.shape) == (rows[b], 2, N)
        assert tuple(alt.entropy.shape) == (rows[b], 2) and tuple(alt.rank.shape) == (rows[b], 2)
        assert alt.codes.dtype == torch.int64 and alt.rank.dtype == torch.int64
    caps = pix.graph_captures()
    again = w.generate_clips(mf, ids, logprobs=True, alternatives=N, **kw)
    assert pix.graph_captures() == caps, "a repeated pass with alternatives captured a graph"
    assert all(same(a, b) for a, b in zip(again, got))
    without_lp = w.generate_clips(mf, ids, alternatives=N, **kw)
    assert all(len(o) == 3 and same(o[:2], p[:2]) and same(o[2:], g[3:]) for o, p, g in zip(without_lp, plain, got))
    for b in range(len(rows)):                                            # every clip alone: the same bits
        one = {k: ([v[b]] if isinstance(v, list) else v) for k, v in kw.items()}
        if how == "philox":
            one.pop("clip_index0")
            one["clip_indices"] = [50 + b]
        alone = w.generate_clips([mf[b]], ids[b:b + 1], logprobs=True, alternatives=N, **one)[0]
        assert same(alone, got[b]), f"{how}: clip {b} alone differs from the clip inside the pass"
    hand = [i for i, t in enumerate(bias) if t is not None][0]            # two allowed hand codes: the third alternative is padding
    alt = got[hand][3]
    assert (_np(alt.codes)[:, 1, 2] == -1).all() and np.isneginf(_np(alt.logprobs)[:, 1, 2]).all()
    assert (_np(alt.codes)[:, 0, :] >= 0).all()
    # the plain pass afterwards finds its own graphs and returns its old bits
    caps = pix.graph_captures()
    assert all(same(a, b) for a, b in zip(w.generate_clips(mf, ids, logprobs=True, **kw), plain)) and pix.graph_captures() == caps


def test_padding_beyond_a_clips_own_rows(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs, reps, bias = clips
    kw = _pieces(_lib, clips, "philox")
    codes, poses, lp, alt = w.generate_clips(mf, ids, logprobs=True, alternatives=N, _stacked=True, **kw)
    assert tuple(alt.codes.shape) == (len(rows), max(rows), 2, N)
    for b, h in enumerate(rows):
        assert (_np(alt.codes)[b, h:] == -1).all() and (_np(alt.logprobs)[b, h:] == 0).all()
        assert (_np(alt.entropy)[b, h:] == 0).all() and (_np(alt.rank)[b, h:] == -1).all()
        assert (_np(alt.rank)[b, :h] >= 0).all() and (_np(alt.entropy)[b, :h] >= 0).all()


def _against_restatement(net, B, H, n, seed):
    """A uniform batch on `net` under records, one bias table and one repetition record: the four outputs equal the restatement applied
    to the network's logits (teacher forced on the codes the decode produced: they do not depend on the controls once the codes agree)."""
    from talkshow_amd import _lib
    Vn = net.input_dim
    rng = np.random.default_rng(seed)
    aud = torch.from_numpy(rng.standard_normal((B, H, net.aud_dim)).astype(F32)).cuda()
    label = np.arange(B) % NC
    u = rng.random((B, H, 2)).astype(F32)
    recs = [(0.8, 0.9, 0), (1.0, 1.0, 1)][:B]
    reps = [(2, 1.5, 0.5), None][:B]
    ban = S.ban_bias((rng.choice(Vn, Vn // 3, replace=False), rng.choice(Vn, 5, replace=False)), Vn)
    bias = [None, ban][:B]
    codes, _, lp, alt = net.run(label, aud, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs, repeat=reps, code_bias=bias,
                                logprobs=True, alternatives=n)
    _, logits = net.run(label, aud, mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)
    codes, logits = _np(codes), _np(logits)
    for b in range(B):
        for r in range(H):
            for j in range(2):
                counts = None if reps[b] is None else S.repeat_counts(codes[b, :r, j], Vn, reps[b][0])
                want = S.alternatives(logits[b, r, j], recs[b], n, bias=None if bias[b] is None else bias[b][j], counts=counts, rep=reps[b],
                                      code=int(codes[b, r, j]))
                msg = f"clip {b} row {r} column {j}"
                assert np.array_equal(_np(alt.codes)[b, r, j], want.codes), msg
                assert int(_np(alt.rank)[b, r, j]) == want.rank, msg
                assert one_spacing(_np(alt.logprobs)[b, r, j], want.logprobs), msg
                assert one_spacing(_np(alt.entropy)[b, r, j], want.entropy), msg
                if recs[b][2] == 1:
                    assert int(_np(alt.codes)[b, r, j, 0]) == int(codes[b, r, j]), msg


def test_outputs_are_the_restatement_on_the_networks_logits(pix):
    _against_restatement(pix, 2, 10, 8, 41)


def test_full_size_network_runs_the_vector_path(wrappers):
    _against_restatement(wrappers[1], 2, 3, 8, 43)


def test_uncertain_keep_redraws_only_the_uncertain_positions(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs, reps, bias = clips
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=5, clip_index0=7)
    first = w.generate_clips(mf, ids, alternatives=0, **kw)
    masks = [S.uncertain_keep(o[2].entropy, float(np.median(_np(o[2].entropy)))) for o in first]
    assert all(m.any() and not m.all() for m in masks[:2]), "a mask keeps everything or nothing: pick another threshold"
    again = w.generate_clips(mf, ids, given=[_np(o[0]) for o in first], given_keep=masks, seed=99, clip_index0=7, mode=_lib.TS_SAMPLE_PHILOX)
    for o, a, m in zip(first, again, masks):
        assert np.array_equal(_np(o[0])[m], _np(a[0])[m]), "a kept position changed its code"
    assert any(not np.array_equal(_np(o[0]), _np(a[0])) for o, a in zip(first, again)), "nothing was redrawn"


def test_generate_batch_and_recordings(w):
    """`generate_batch` and `generate_clips_from_wav` return what `generate_clips` returns on the same clips."""
    from talkshow_amd import _lib
    from talkshow_amd.frontend import device_mfcc
    B = 3
    mf = synth.mfcc_features(500, B, 43)
    ids = np.array([1, 0, 2], np.int64)
    bkw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=9, sampling=[(0.8, 0.9, 0), None, (1.0, 1.0, 1)])
    c, p, lp, alt = w.generate_batch(mf, ids, logprobs=True, alternatives=N, **bkw)
    c2, p2, alt2 = w.generate_batch(mf, ids, alternatives=N, **bkw)
    want = w.generate_clips([torch.from_numpy(m) for m in mf], ids, logprobs=True, alternatives=N, **bkw)
    assert tuple(alt.codes.shape) == (B, 10, 2, N) and same((c, p, alt), (c2, p2, alt2))
    for b in range(B):
        assert same((c[b], p[b], lp[b], S.Alternatives(*(x[b] for x in alt))), want[b]), f"generate_batch(alternatives=): clip {b}"
    ns = [5872, 16000]
    wavs = [synth.wav16(11000 + k, 1, int(x))[0] for k, x in enumerate(ns)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100, repeat=[(6, 2.0, 0.0), (64, 0.3, 0.3)])
    mfw = [device_mfcc(16000)(x)[0] for x in wavs]
    want = w.generate_clips(mfw, ids[:2], alternatives=N, **kw)
    got = w.generate_clips_from_wav(wavs, 16000, ids[:2], alternatives=N, **kw)
    plain = w.generate_clips_from_wav(wavs, 16000, ids[:2], **kw)
    for b in range(len(ns)):
        assert same(got[b], want[b]), f"generate_clips_from_wav(alternatives=): recording {b}"
        assert len(plain[b]) == 2 and same(got[b][:2], plain[b])
    with pytest.raises(ValueError):
        w.generate_clips_from_wav(wavs, 16000, ids[:2], mode=_lib.TS_SAMPLE_GREEDY, alternatives=N)
    with pytest.raises(NotImplementedError):
        w.generate_clips_from_wav(wavs, 16000, ids[:2], alternatives=N, guide={"scale": 1.0, "id": 1})


def test_refusals_move_nothing(w, pix, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs, reps, bias = clips
    caps = pix.graph_captures()
    with pytest.raises(ValueError, match=r"sampling=\(1, 1, 1\)"):
        w.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_GREEDY, alternatives=3)
    with pytest.raises(ValueError):
        w.generate_clips(mf, ids, alternatives=9)
    with pytest.raises(ValueError):
        w.generate_clips(mf, ids, alternatives=-1)
    with pytest.raises(NotImplementedError):
        w.generate_clips(mf, ids, alternatives=3, guide={"scale": 1.0, "id": 1})
    aud = torch.zeros((2, 3, pix.aud_dim), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        pix.run([0, 1], aud, mode=_lib.TS_SAMPLE_GREEDY, alternatives=3)
    with pytest.raises(ValueError):
        pix.run([0, 1], aud, alternatives=3, want_logits=True)
    with pytest.raises(NotImplementedError):
        pix.run([0, 1], aud, alternatives=3, guide={"scale": 1.0, "id": 1})
    assert pix.graph_captures() == caps
