"""Code bias through the body decode (`ts_body_pixel_infer_mixed_bias`, `ts_pixelcnn_generate_mixed_bias`,
`ts_body_pixel_infer_mixed_poses_bias`; `code_bias=` on `GatedPixelCNN.run`, `TrainWrapper.generate_batch / generate_clips /
generate_clips_from_wav`, `parallel.whole_body_clips`; `TrainWrapper.code_bias_from_motion`).

The rule (include/talkshow_hip.h, "code bias"): l' = l + b ahead of the sampling rule, one fp32 addition; a token with l' = -inf is never
kept.  Every check but one is EQUALITY or membership; the one against the reference arithmetic carries `sampling.logprob_error_bound`.
The PixelCNN is the small network of the quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped wrapper; six clips of
20, 17, 17, 9, 8 and 3 code rows, submitted shuffled.  Every test fails on a build without the feature: the keyword and the entries do not
exist there.
"""
import os

import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(input_dim=256, dim=64, n_layers=3)
V, NC = DIMS["input_dim"], 4
ROWS = [20, 17, 17, 9, 8, 3]                       # code rows of the six clips: two chunks and a half, ties, a clip shorter than a chunk
RECS = [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.7, 1.0, 12), (0.5, 0.5, 40), (1.0, 1.0, 0), (4.0, 0.95, 64)]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def same_all(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def _pix(sd):
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, True, True).cuda()
    m.load_state_dict(synth.to_torch(sd))
    return m


@pytest.fixture(scope="module")
def sd():
    return synth.pixelcnn_state_dict(seed=11, **DIMS)


@pytest.fixture(scope="module")
def pix(sd):
    return _pix(sd)


@pytest.fixture(scope="module")
def w(pix):
    """The shipped wrapper (audio encoder, VQ decoders) around the small code predictor."""
    import bench
    wr = bench.build_models(0, seed=7)[0]
    wr.generator = pix
    return wr


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(21)
    order = rng.permutation(len(ROWS))               # submitted shuffled: the Python layer sorts and un-sorts
    rows = [ROWS[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(3000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    recs = [RECS[i] for i in order]
    return rows, mf, ids, recs


def _tables(seed):
    """Six entries in submission order: an allow-list of 40 / 25 codes, None, a finite random table, a ban of half the codes, the FIRST
    entry's object again, a dict with a hand row only."""
    rng = np.random.default_rng(seed)
    allow = S.allow_bias((rng.choice(V, 40, replace=False), rng.choice(V, 25, replace=False)), V)
    rnd = (2.0 * rng.standard_normal((2, V))).astype(F32)
    ban = S.ban_bias((rng.choice(V, V // 2, replace=False), np.arange(V // 2, V)), V)
    hand = np.where(rng.random(V) < 0.8, -np.inf, rng.standard_normal(V)).astype(F32)
    hand[7] = 0.5
    return [allow, None, rnd, ban, allow, {"hand": hand}]


def _table_of(entry):
    if entry is None:
        return None
    if isinstance(entry, dict):
        t = np.zeros((2, V), F32)
        for j, k in enumerate(("body", "hand")):
            if k in entry:
                t[j] = entry[k]
        return t
    return entry


def assert_allowed(out, tables, what=""):
    for b, (o, e) in enumerate(zip(out, tables)):
        t = _table_of(e)
        if t is None:
            continue
        codes = _np(o[0])
        for j in range(2):
            bad = np.flatnonzero(t[j][codes[:, j]] == -np.inf)
            assert bad.size == 0, f"{what}clip {b} column {j}: banned codes at rows {bad[:8]}"


def _modes(_lib, rows, rng):
    u = [rng.random((h, 2)).astype(F32) for h in rows]
    return {"uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u), "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50)}


# ---- 1. allowed codes; None and a zero table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_codes_are_allowed_and_none_is_the_plain_pass(w, clips, how):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    assert min(rows) < 8 < max(rows)
    kw = _modes(_lib, rows, np.random.default_rng(31))[how]
    tabs = _tables(41)
    for extra in (dict(), dict(sampling=recs)):
        plain = w.generate_clips(mf, ids, logprobs=True, **kw, **extra)
        got = w.generate_clips(mf, ids, logprobs=True, code_bias=tabs, **kw, **extra)
        assert_allowed(got, tabs, f"{how}: ")
        assert same(got[1], plain[1]), f"{how}: the clip with None differs from the pass without the keyword"
        assert not same_all(got, plain)
        for b in range(len(rows)):
            assert np.isfinite(_np(got[b][2])).all() and (_np(got[b][2]) <= 0).all()
        nones = w.generate_clips(mf, ids, logprobs=True, code_bias=[None] * len(rows), **kw, **extra)
        assert same_all(nones, plain)
        zero = w.generate_clips(mf, ids, logprobs=True, code_bias=np.zeros((2, V), F32), **kw, **extra)
        for b in range(len(rows)):
            assert np.array_equal(_np(zero[b][0]), _np(plain[b][0])), f"{how}: clip {b}: a zero table changes the codes"
            assert np.array_equal(_np(zero[b][2]), _np(plain[b][2]))      # == : the sign of a zero apart


# ---- 2. neighbours ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_a_clip_does_not_depend_on_its_neighbours(w, clips, how):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    B = len(rows)
    tabs = _tables(43)
    modes = _modes(_lib, rows, np.random.default_rng(33))[how]
    kw = dict(modes, logprobs=True)
    kw.pop("clip_index0", None)
    together = w.generate_clips(mf, ids, code_bias=tabs, sampling=recs, clip_indices=[70 + b for b in range(B)], **kw)
    for b in range(B):
        one = dict(kw)
        if "uniforms" in one:
            one["uniforms"] = [kw["uniforms"][b]]
        alone = w.generate_clips([mf[b]], [ids[b]], code_bias=[tabs[b]], sampling=[recs[b]], clip_indices=[70 + b], **one)[0]
        assert same(alone, together[b]), f"{how}: clip {b} ({rows[b]} rows) alone differs from the clip inside the six-clip pass"
    b = max((k for k in range(B) if tabs[k] is not None), key=lambda k: rows[k])      # the longest clip that brings a table
    other = _tables(44)
    mixed = [tabs[k] if k == b else (other[k].copy() if isinstance(other[k], np.ndarray) else other[k]) for k in range(B)]     # copies: another NB
    out = w.generate_clips(mf, ids, code_bias=mixed, sampling=recs, clip_indices=[70 + k for k in range(B)], **kw)
    assert same(out[b], together[b]), f"{how}: clip {b} changes with its neighbours' tables"
    lone = [tabs[k] if k == b else None for k in range(B)]                # NB = 1
    out = w.generate_clips(mf, ids, code_bias=lone, sampling=recs, clip_indices=[70 + k for k in range(B)], **kw)
    assert same(out[b], together[b]), f"{how}: clip {b} changes with NB"


# ---- 3. against the reference arithmetic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_against_the_reference_arithmetic(pix, how):
    """B = 3, H = 10 (the chunk boundary is crossed).  The biased pass draws codes and returns their log-probabilities; the network's
    teacher-forced logits of those codes, plus b, through a float64 log-softmax are the reference.  Bound: `S.logprob_error_bound`, the
    derived bound of the restatement against an exact log-softmax of its fp32 input (d_c and the total from the biased row)."""
    from talkshow_amd import _lib
    B, H = 3, 10
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(np.array([0, 3, 1], np.int64)).cuda()
    tabs = _tables(51)
    bias = [tabs[0], tabs[2], tabs[3]]
    kw = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=rng.random((B, H, 2)).astype(F32)) if how == "uniforms" else dict(mode=_lib.TS_SAMPLE_PHILOX, seed=5)
    codes, _, lp = pix.run(label, aud, code_bias=bias, logprobs=True, **kw)
    codes, lp = _np(codes), _np(lp)
    _, logits = pix.run(label, aud, mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)
    logits = _np(logits)                                                   # (B, H, 2, V): the network's l, no bias
    worst = 0.0
    for b in range(B):
        for r in range(H):
            for j in range(2):
                c = int(codes[b, r, j])
                assert bias[b][j, c] != -np.inf
                x = logits[b, r, j].astype(np.float64) + bias[b][j].astype(np.float64)
                with np.errstate(divide="ignore"):
                    ref = x[c] - x.max() - np.log(np.exp(x - x.max()).sum())
                lb = S.biased(logits[b, r, j], bias[b][j])
                bound = S.logprob_error_bound(V, lb[c] - lb.max(), lp[b, r, j])
                err = abs(float(lp[b, r, j]) - ref)
                worst = max(worst, err / bound)
                assert err <= bound, f"{how}: clip {b} row {r} column {j}: |{lp[b, r, j]} - {ref}| = {err:.3e} > {bound:.3e}"
    print(f"\n{how}: worst error / bound = {worst:.3f}")


# ---- 4. composition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", [True, False])
def test_composition(w, clips, records):
    """One pass with (records: sampling records,) a speaker style, a code bias, then given rows on half the clips with given_keep="body" on
    some: handing back the head of the biased decode with the same bias returns that decode bit for bit."""
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    B = len(rows)
    tabs = _tables(47)
    rng = np.random.default_rng(48)
    style = [None if b % 3 == 0 else rng.standard_normal(NC).astype(F32) for b in range(B)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=19, clip_index0=200, logprobs=True, style=style, code_bias=tabs)
    if records:
        kw["sampling"] = recs
    D = w.generate_clips(mf, ids, **kw)
    assert_allowed(D, tabs)
    G = [rows[b] if b == 0 else (rows[b] + 1) // 2 for b in range(B)]
    given = [_np(D[b][0])[:G[b]] if b % 2 == 0 else None for b in range(B)]
    keep = ["body" if (b % 4 == 0) else None for b in range(B)]
    back = w.generate_clips(mf, ids, given=given, given_keep=keep, **kw)
    for b in range(B):
        assert same(back[b], D[b]), f"clip {b}: handing back the head of a biased decode with the same bias does not return that decode"
    plain = w.generate_clips(mf, ids, **{**kw, "code_bias": None})
    assert not same_all(D, plain)
    if records:      # (a given code the FILTERS remove scores -inf too: the check below wants the bias alone)
        return
    # a given code the bias bans is still taken, and scores -inf
    b = 0
    t = _table_of(tabs[b])
    forced = _np(D[b][0]).copy()
    forced[0, 0] = int(np.flatnonzero(t[0] == -np.inf)[0])
    out = w.generate_clips(mf, ids, given=[forced if k == b else None for k in range(B)], **kw)
    assert np.array_equal(_np(out[b][0]), forced) and _np(out[b][2])[0, 0] == -np.inf and np.isfinite(_np(out[b][2])[1:]).all()


# ---- 5. graphs ----------------------------------------------------------------------------------------------------------------------------------
def test_graphs(w, pix, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    # five of the six clips: a pass shape no other test of this module runs, so what is captured below is captured HERE
    rows, mf, ids = rows[:5], mf[:5], ids[:5]
    B = len(rows)
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3, logprobs=True)
    caps0 = pix.graph_captures()
    plain = w.generate_clips(mf, ids, **kw)
    caps_plain = pix.graph_captures()
    assert caps_plain > caps0
    assert same_all(plain, w.generate_clips(mf, ids, code_bias=None, **kw)) and pix.graph_captures() == caps_plain
    t = _tables(52)[:5]
    one = [t[0] if k in (0, 4) else None for k in range(B)]                 # NB = 1
    r1 = w.generate_clips(mf, ids, code_bias=one, **kw)
    caps_b = pix.graph_captures()
    assert caps_b > caps_plain and caps_b - caps_plain <= 14 and caps_b - caps_plain == caps_plain - caps0     # keys of its own (bit 5)
    assert same_all(r1, w.generate_clips(mf, ids, code_bias=one, **kw)) and pix.graph_captures() == caps_b      # repeated: nothing captured
    distinct = [S.allow_bias((np.arange(10 * k, 10 * k + 30), np.arange(5 * k, 5 * k + 9)), V) for k in range(B)]   # NB = B
    r2 = w.generate_clips(mf, ids, code_bias=distinct, **kw)
    assert pix.graph_captures() == caps_b, "another table content or another NB captured a graph"
    assert_allowed(r2, distinct)
    for k in range(B):                                                     # correct, not merely allowed: each clip alone
        alone = w.generate_clips([mf[k]], [ids[k]], code_bias=[distinct[k]], mode=kw["mode"], seed=9, clip_indices=[3 + k], logprobs=True)[0]
        assert same(alone, r2[k]), f"NB = B: clip {k}"
    caps_c = pix.graph_captures()                                          # the single-clip shapes captured theirs
    r1b = w.generate_clips(mf, ids, code_bias=one, **kw)                   # NB = 1 again, behind NB = B
    assert same_all(r1, r1b) and pix.graph_captures() == caps_c
    assert_allowed(r1b, one)
    other = w.generate_clips(mf, ids, code_bias=[t[3] if k in (0, 4) else None for k in range(B)], **kw)
    assert pix.graph_captures() == caps_c and not same_all(other, r1)
    # the plain pass afterwards finds its own graphs and returns its old bits
    assert same_all(plain, w.generate_clips(mf, ids, **kw)) and pix.graph_captures() == caps_c


# ---- 6. entry points ----------------------------------------------------------------------------------------------------------------------------
def test_run_and_generate_batch(w, pix):
    from talkshow_amd import _lib
    B, H = 3, 10
    rng = np.random.default_rng(8)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(np.array([0, 3, 1], np.int64)).cuda()
    tabs = _tables(61)
    bias = [tabs[0], None, tabs[3]]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=31, clip_index0=4)
    plain = pix.run(label, aud, logprobs=True, **kw)
    got = pix.run(label, aud, logprobs=True, code_bias=bias, **kw)
    codes = _np(got[0])
    for b in (0, 2):
        for j in range(2):
            assert np.all(bias[b][j][codes[b, :, j]] != -np.inf)
    assert np.array_equal(codes[1], _np(plain[0])[1]) and np.array_equal(_bits(got[2])[1], _bits(plain[2])[1])
    assert len(pix.run(label, aud, code_bias=bias, **kw)) == 2 and np.array_equal(_np(pix.run(label, aud, code_bias=bias, **kw)[0]), codes)
    one = pix.run(label, aud, code_bias=tabs[0], sampling=(0.8, 0.9, 0), **kw)[0]       # one table for all, with a record
    assert all(np.all(tabs[0][j][_np(one)[:, :, j]] != -np.inf) for j in range(2))
    mf = synth.mfcc_features(500, B, 43)
    ids = np.array([1, 0, 2], np.int64)
    bkw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=9)
    c, p = w.generate_batch(mf, ids, code_bias=bias, **bkw)
    want = w.generate_clips([torch.from_numpy(m) for m in mf], ids, code_bias=bias, **bkw)
    c0, p0 = w.generate_batch(mf, ids, **bkw)
    for b in range(B):
        assert np.array_equal(_np(c[b]), _np(want[b][0])) and np.array_equal(_bits(p[b]), _bits(want[b][1]))
    assert np.array_equal(_np(c[1]), _np(c0[1])) and not np.array_equal(_np(c), _np(c0))


def test_code_bias_from_motion():
    """The vocabulary of example motion (full-size networks: the VQ codebooks and the predictor share V = 2 048): the allow-list of the
    codes two pose clips encode to, then a decode that stays inside it."""
    import bench
    from talkshow_amd import _lib
    from talkshow_amd.modules import encode_pair_masked, pad_pose_clips, upload
    wf = bench.build_models(0, seed=7)[0]
    Vf = wf.generator.input_dim
    motion = [synth.gt_poses(60 + k, 1, n)[0] for k, n in enumerate((37, 64))]
    vocab = wf.code_bias_from_motion(motion)
    block, lens = pad_pose_clips(motion, wf.generator._dev(), "test", 129)
    enc = _np(encode_pair_masked(wf.g_body, wf.g_hand, block, upload(lens, wf.generator._dev())))
    enc = np.concatenate([enc[b, :int(t) // 4] for b, t in enumerate(lens)])
    assert enc.shape == (9 + 16, 2) and (enc >= 0).all()
    assert vocab.shape == (2, Vf) and vocab.dtype == F32 and np.array_equal(vocab, S.allow_bias(enc, Vf))
    for j in range(2):
        assert sorted(np.flatnonzero(vocab[j] == 0)) == sorted(set(enc[:, j].tolist())) and (vocab[j][vocab[j] != 0] == -np.inf).all()
    mf = [synth.mfcc_features(3100 + k, 1, t)[0] for k, t in enumerate((50, 23))]
    out = wf.generate_clips(mf, [1, 2], mode=_lib.TS_SAMPLE_PHILOX, seed=3, code_bias=vocab, sampling=(1.3, 0.98, 0))
    for b, (codes, poses) in enumerate(out):
        codes = _np(codes)
        assert codes.shape == (mf[b].shape[0] // 4, 2) and np.isfinite(_np(poses)).all()
        for j in range(2):
            assert set(codes[:, j].tolist()) <= set(enc[:, j].tolist()), f"clip {b} column {j} left the vocabulary of the motion"


def test_recordings_and_whole_body(w):
    import argparse
    import json

    import nets
    from talkshow_amd import _lib, parallel
    from talkshow_amd.config import Object
    from talkshow_amd.frontend import device_mfcc
    from talkshow_amd.pose_index import assemble_full
    ns = [5872, 16000]
    wavs = [synth.wav16(11000 + k, 1, int(x))[0] for k, x in enumerate(ns)]
    ids = np.array([2, 1], np.int64)
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100)
    bias = [_tables(71)[0], {"body": S.ban_bias((np.arange(0, V, 2), []), V)[0]}]
    mf = [device_mfcc(16000)(x)[0] for x in wavs]
    want = w.generate_clips(mf, ids, code_bias=bias, **kw)
    assert_allowed(want, bias)
    wav = w.generate_clips_from_wav(wavs, 16000, ids, code_bias=bias, **kw)
    plain = w.generate_clips_from_wav(wavs, 16000, ids, **kw)
    for b in range(len(ns)):
        assert same(wav[b], want[b]), f"generate_clips_from_wav(code_bias=): recording {b}"
    assert not same_all(wav, plain)
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    fid = np.zeros((1, 4), np.float32)
    out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100, code_bias=bias)
    for b in range(len(ns)):
        f = face.generator.run_clips([wavs[b]], fid)[0]                  # the face half has no codes
        ref = _np(assemble_full(wav[b][1][None], f[None]))[0]
        assert np.array_equal(_np(out[b]), ref), f"whole_body_clips(code_bias=): recording {b}"


# ---- 7. what is refused, before any launch ------------------------------------------------------------------------------------------------------
def test_refusals(w, pix, clips):
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    rows, mf, ids, recs = clips
    B, H = 3, 10
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(np.array([0, 3, 1], np.int64)).cuda()
    codes = rng.integers(0, V, (B, H, 2))
    caps = pix.graph_captures()
    ok = np.zeros((2, V), F32)

    def bad(j, v, x):
        t = ok.copy()
        t[j, v] = x
        return t
    allb = ok.copy()
    allb[0] = -np.inf
    for table, pat in ((np.zeros((2, V + 1), F32), r"generate_clips: code_bias of clip 2 must be a \(2, 256\)"), (bad(0, 3, np.nan), r"clip 2: body column.*NaN"),
                       (bad(1, 3, np.inf), r"clip 2: hand column.*\+inf"), (bad(1, 9, 3e30), r"clip 2: hand column.*1e30"),
                       (allb, r"clip 2: body column: every code is banned")):
        with pytest.raises(ValueError, match=pat):
            w.generate_clips(mf, ids, code_bias=[ok, None, table, None, None, None])
    with pytest.raises(ValueError, match="top_k = 1"):
        w.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_GREEDY, code_bias=ok)
    with pytest.raises(ValueError, match="top_k = 1"):
        pix.run(label, aud, mode=_lib.TS_SAMPLE_GREEDY, code_bias=ok)
    with pytest.raises(ValueError, match="top_k = 1"):
        pix.run(label, aud, mode=_lib.TS_TEACHER_FORCED, codes=codes, code_bias=ok)
    with pytest.raises(ValueError, match="logits output"):
        pix.run(label, aud, want_logits=True, code_bias=ok)
    with pytest.raises(ValueError, match=r"run: code_bias of clip 1"):
        pix.run(label, aud, code_bias=[None, np.zeros((2, V - 1), F32), None])
    assert pix.graph_captures() == caps
    single = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, False, False)
    with pytest.raises(NotImplementedError, match="single-stack form"):
        single.run(label, aud, code_bias=ok)
    # the C entries refuse the modes and a bad index table themselves, before their first launch
    lib = _lib.load()
    I32P = _lib.C.POINTER(_lib.C.c_int32)
    lens = np.full(B, 4 * H, np.int32)
    lens_dev, out = torch.from_numpy(lens).cuda(), torch.full((B, H, 2), -7, dtype=torch.int64, device="cuda")
    td = torch.zeros((2, 2, V), dtype=torch.float32, device="cuda")

    def call(mode, index, n_bias=2):
        index = np.ascontiguousarray(index, np.int32)
        return lib.ts_pixelcnn_generate_mixed_bias(pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H,
                                                   mode, None, 0, None, _lib.dptr(out), None, 0, None, None, None, None, None, None, 0, _lib.dptr(td),
                                                   n_bias, index.ctypes.data_as(I32P), _lib.stream_ptr())
    assert call(_lib.TS_SAMPLE_GREEDY, [0, 1, -1]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_PHILOX, [0, 2, -1]) != 0 and "clip 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_PHILOX, [0, 0, 0], n_bias=4) != 0
    torch.cuda.synchronize()
    assert (_np(out) == -7).all() and pix.graph_captures() == caps
    assert call(_lib.TS_SAMPLE_PHILOX, [0, 1, -1]) == 0
    torch.cuda.synchronize()
    assert ((_np(out) >= 0) & (_np(out) < V)).all()
