"""Guidance through the body decode (`ts_body_pixel_infer_guided`, `ts_pixelcnn_generate_guided`,
`ts_body_pixel_infer_guided_poses`; `guide=` on `GatedPixelCNN.run`, `TrainWrapper.generate_batch / generate_clips /
generate_clips_from_wav`, `parallel.whole_body_clips`).

The rule (include/talkshow_hip.h, "guidance"): a guided clip's logits become l' = l + scale * (l - l_q), l_q the logits a shadow slot
computes for the same code history under a second conditioning, ahead of every other control.  Every check is EQUALITY of bits: against the
plain pass, against the clip alone, against `sampling.sample_guide` on teacher-forced logits.  The PixelCNN is the small network of the
quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped wrapper; five clips of 19, 19, 9, 9 and 2 code rows (two chunks and a
short third one), submitted shuffled.  Every test fails on a build without the feature: the keyword and the entries do not exist there.
"""
import os

import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(input_dim=256, dim=64, n_layers=3)
V, NC = DIMS["input_dim"], 4
ROWS = [19, 19, 9, 9, 2]
RECS = [(0.8, 0.9, 0), (1.0, 1.0, 0), (1.7, 1.0, 12), (0.5, 0.5, 40), (4.0, 0.95, 64)]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def same_all(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def pix():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=11, **DIMS)))
    return m


@pytest.fixture(scope="module")
def w(pix):
    """The shipped wrapper (audio encoder, VQ decoders) around the small code predictor."""
    import bench
    wr = bench.build_models(0, seed=7)[0]
    wr.generator = pix
    return wr


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(23)
    order = rng.permutation(len(ROWS))               # submitted shuffled: the Python layer sorts and un-sorts
    rows = [ROWS[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(4000 + k, 1, t)[0] for k, t in enumerate(lens)]
    other = [synth.mfcc_features(5000 + k, 1, t)[0] for k, t in enumerate(lens)]      # the second conditioning's audio, clip by clip
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    recs = [RECS[i] for i in order]
    return rows, mf, other, ids, recs


def _guides(other, ids, scale=2.0):
    """Five entries in submission order: other audio; another speaker; None; other audio AND another speaker, toward q; a style row."""
    return [{"scale": scale, "mfcc": other[0]}, {"scale": 1.5 * scale, "id": int((ids[1] + 1) % NC)}, None,
            {"scale": -0.5, "mfcc": other[3], "id": int((ids[3] + 2) % NC)}, {"scale": scale, "style": np.asarray([0.5, 0.5, 0, 0], F32)}]


def _modes(_lib, rows, rng):
    u = [rng.random((h, 2)).astype(F32) for h in rows]
    return {"uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u), "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50)}


# ---- consequences 1 and 2: scale 0, and a shadow with the clip's own conditioning -------------------------------------------------------
@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_scale_zero_and_own_conditioning_are_the_plain_pass(w, clips, how):
    from talkshow_amd import _lib
    rows, mf, other, ids, recs = clips
    assert min(rows) < 8 < max(rows) and max(rows) % 8 != 0
    kw = _modes(_lib, rows, np.random.default_rng(31))[how]
    for extra in (dict(), dict(sampling=recs)):
        plain = w.generate_clips(mf, ids, logprobs=True, **kw, **extra)
        zero = w.generate_clips(mf, ids, logprobs=True, guide=_guides(other, ids, 0.0)[:3] + [None, None], **kw, **extra)
        for b in range(len(rows)):
            assert np.array_equal(_np(zero[b][0]), _np(plain[b][0])), f"{how}: clip {b}: scale 0 changes the codes"
            assert np.array_equal(_np(zero[b][2]), _np(plain[b][2])) and np.array_equal(_bits(zero[b][1]), _bits(plain[b][1]))      # == : the sign of a zero apart
        for scale in (3.0, -0.5, 1e4):
            own = w.generate_clips(mf, ids, logprobs=True, guide=[{"scale": scale}, None, {"scale": -scale}, {"scale": scale}, {"scale": scale}], **kw, **extra)
            assert same_all(own, plain), f"{how}: a shadow with the clip's own conditioning moves bits at scale {scale}"
        moved = w.generate_clips(mf, ids, logprobs=True, guide=_guides(other, ids), **kw, **extra)
        assert same(moved[2], plain[2]), f"{how}: the clip with None differs from the pass without the keyword"
        assert sum(not np.array_equal(_np(moved[b][0]), _np(plain[b][0])) for b in (0, 1, 3)) >= 2, "guidance moves no codes"
        assert same_all(w.generate_clips(mf, ids, logprobs=True, guide=None, **kw, **extra), plain)
        assert same_all(w.generate_clips(mf, ids, logprobs=True, guide=[None] * len(rows), **kw, **extra), plain)


# ---- consequence 3: a primary draws the numbers of its own clip index and position -------------------------------------------------------
def test_philox_numbers_are_the_primaries_own(w, clips):
    from talkshow_amd import _lib
    rows, mf, other, ids, recs = clips
    seed, clip0 = 991, 40
    g = _guides(other, ids)
    ph = w.generate_clips(mf, ids, logprobs=True, guide=g, sampling=recs, mode=_lib.TS_SAMPLE_PHILOX, seed=seed, clip_index0=clip0)
    u = [np.asarray([[O.philox_uniform(seed, clip0 + b, 2 * r + j) for j in range(2)] for r in range(h)], F32) for b, h in enumerate(rows)]
    un = w.generate_clips(mf, ids, logprobs=True, guide=g, sampling=recs, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u)
    assert same_all(ph, un), "a guided pass draws other Philox numbers than (seed, the clip's own index, its absolute position)"
    named = w.generate_clips(mf, ids, logprobs=True, guide=g, sampling=recs, mode=_lib.TS_SAMPLE_PHILOX, seed=seed, clip_indices=[clip0 + b for b in range(len(rows))])
    assert same_all(ph, named)


# ---- consequence 5: neighbours, and where the shadow sits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["uniforms", "philox"])
def test_a_clip_does_not_depend_on_its_neighbours(w, clips, how):
    from talkshow_amd import _lib
    rows, mf, other, ids, recs = clips
    B = len(rows)
    g = _guides(other, ids)
    kw = dict(_modes(_lib, rows, np.random.default_rng(33))[how], logprobs=True)
    kw.pop("clip_index0", None)
    idx = [70 + b for b in range(B)]
    together = w.generate_clips(mf, ids, guide=g, sampling=recs, clip_indices=idx, **kw)
    for b in range(B):
        one = dict(kw)
        if "uniforms" in one:
            one["uniforms"] = [kw["uniforms"][b]]
        alone = w.generate_clips([mf[b]], [ids[b]], guide=[g[b]], sampling=[recs[b]], clip_indices=[idx[b]], **one)[0]
        assert same(alone, together[b]), f"{how}: clip {b} ({rows[b]} rows) alone differs from the clip inside the guided pass"
        lone = w.generate_clips(mf, ids, guide=[g[k] if k == b else None for k in range(B)], sampling=recs, clip_indices=idx, **kw)
        assert same(lone[b], together[b]), f"{how}: clip {b} changes with which of its neighbours are guided"


def test_where_the_shadow_sits(pix):
    """The C entry takes a shadow in any slot of the primary's length: [p, s, x, y] and [s, x, y, p] return p's bits, and s's rows are p's."""
    from talkshow_amd import _lib
    from talkshow_amd.modules import upload
    B, H = 4, 10
    rng = np.random.default_rng(9)
    aud = rng.standard_normal((B, H, 256)).astype(F32)
    label = np.array([0, 3, 1, 2], np.int64)
    i32p = _lib.C.POINTER(_lib.C.c_int32)
    lens = np.full(B, 4 * H, np.int32)

    def call(perm, guide, scale):
        a, l, ci = torch.from_numpy(aud[perm]).cuda(), torch.from_numpy(label[perm]).cuda(), torch.from_numpy(np.asarray(perm, np.int64) + 20).cuda()
        codes = torch.full((B, H, 2), -7, dtype=torch.int64, device="cuda")
        lp = torch.full((B, H, 2), 7.0, dtype=torch.float32, device="cuda")
        g, s = np.asarray(guide, np.int32), np.asarray(scale, F32)
        fixed = (pix.handle(), _lib.dptr(l), _lib.dptr(a), lens.ctypes.data_as(i32p), _lib.dptr(upload(lens, a.device)), B, H, _lib.TS_SAMPLE_PHILOX,
                 None, 5, _lib.dptr(ci), _lib.dptr(codes))
        _lib.pixelcnn_mixed_call(fixed, logprob=_lib.dptr(lp), guide=g.ctypes.data_as(i32p), guide_scale=_lib.fptr(s))
        return _np(codes), _np(lp)
    c1, l1 = call([0, 1, 2, 3], [1, -1, -1, -1], [2.5, 0, 0, 0])
    c2, l2 = call([1, 2, 3, 0], [-1, -1, -1, 0], [0, 0, 0, 2.5])
    assert np.array_equal(c1[0], c2[3]) and np.array_equal(_bits(l1[0]), _bits(l2[3]))
    assert np.array_equal(c1[1], c1[0]) and np.array_equal(c2[0], c2[3]) and np.array_equal(_bits(l1[1]), _bits(l1[0]))      # the shadow's rows are its primary's
    assert np.array_equal(c1[2:], c2[1:3]) and np.array_equal(_bits(l1[2:]), _bits(l2[1:3]))                                   # the plain slots
    plain = pix.run(torch.from_numpy(label).cuda(), torch.from_numpy(aud).cuda(), seed=5, clip_index0=20, logprobs=True)
    assert np.array_equal(c1[2:], _np(plain[0])[2:]) and not np.array_equal(c1[0], _np(plain[0])[0])


# ---- the reference arithmetic -----------------------------------------------------------------------------------------------------------
def test_against_the_reference_arithmetic(pix):
    """B = 3, H = 10 (the chunk boundary is crossed): clip 0 guided against another speaker, clip 1 against other audio toward q, clip 2
    plain.  The network's teacher-forced logits of the returned codes under each conditioning and the uniforms, through
    `sampling.sample_guide`, reproduce every code and every log-probability bit."""
    from talkshow_amd import _lib
    B, H = 3, 10
    rng = np.random.default_rng(6)
    aud = rng.standard_normal((B, H, 256)).astype(F32)
    aud_q = aud.copy()
    aud_q[1] = rng.standard_normal((H, 256)).astype(F32)
    label, label_q = np.array([0, 3, 1], np.int64), np.array([2, 3, 1], np.int64)
    recs = [(0.8, 0.9, 0), (1.3, 1.0, 20), (1.0, 1.0, 0)]
    guide = [{"scale": 2.0, "id": 2}, {"scale": -0.5, "aud_rows": aud_q[1]}, None]
    u = rng.random((B, H, 2)).astype(F32)
    dev = lambda x: torch.from_numpy(x).cuda()
    codes, _, lp = pix.run(dev(label), dev(aud), mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs, guide=guide, logprobs=True)
    plain = pix.run(dev(label), dev(aud), mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs, logprobs=True)
    codes, lp = _np(codes), _np(lp)
    assert codes.shape == (B, H, 2) and np.array_equal(codes[2], _np(plain[0])[2]) and not np.array_equal(codes[:2], _np(plain[0])[:2])
    lp_ = _np(pix.run(dev(label), dev(aud), mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)[1])
    lq_ = _np(pix.run(dev(label_q), dev(aud_q), mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)[1])
    moved = 0
    for b in (0, 1):
        for r in range(H):
            for j in range(2):
                rows = np.stack([lp_[b, r, j], lq_[b, r, j]])
                ti, _, tl, _ = S.sample_guide(rows, [u[b, r, j], 0.0], [recs[b]] * 2, [1, -1], [guide[b]["scale"], 0.0])
                assert ti[0] == codes[b, r, j], f"clip {b} row {r} column {j}: code {codes[b, r, j]}, the rule gives {ti[0]}"
                assert _bits(tl[0]) == _bits(lp[b, r, j]), f"clip {b} row {r} column {j}: logprob {lp[b, r, j]}, the rule gives {tl[0]}"
                moved += int(S.sample_ctl(rows[:1], [u[b, r, j]], recs[b])[0][0] != ti[0])
    assert moved >= 10, f"guidance moved {moved} of 40 draws"


# ---- composition, and handing a decode back -----------------------------------------------------------------------------------------------
def test_composition_and_handing_back(w, clips):
    """sampling, code_bias, repeat, style and guide in one pass; then given rows on some clips and given_keep="body" on one: handing back
    the head of the guided decode under the same keywords returns that decode; the poses are the VQ decode of the returned codes; then
    given rows, given_keep="body" AND given poses (on other clips) beside all of these in ONE guided pass."""
    from talkshow_amd import _lib
    rows, mf, other, ids, recs = clips
    B = len(rows)
    rng = np.random.default_rng(48)
    style = [None if b % 2 == 0 else rng.standard_normal(NC).astype(F32) for b in range(B)]
    bias = [None if b == 2 else (0.5 * rng.standard_normal((2, V))).astype(F32) for b in range(B)]
    rep = [(16, 1.0, 0.5)] * B
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=19, clip_index0=200, logprobs=True, style=style, code_bias=bias, repeat=rep, sampling=recs,
              guide=_guides(other, ids))
    D = w.generate_clips(mf, ids, **kw)
    assert not same_all(D, w.generate_clips(mf, ids, **{**kw, "guide": None}))
    G = [rows[b] if b == 0 else (rows[b] + 1) // 2 for b in range(B)]
    given = [_np(D[b][0])[:G[b]] if b in (0, 1, 3) else None for b in range(B)]
    keep = ["body" if b == 1 else None for b in range(B)]
    back = w.generate_clips(mf, ids, given=given, given_keep=keep, **kw)
    for b in range(B):
        assert same(back[b], D[b]), f"clip {b}: handing back the head of a guided decode does not return that decode"
    # every row given: the poses are the decode of those codes, with or without guidance (the plain pass decodes the same codes)
    allg = [_np(D[b][0]) for b in range(B)]
    taken = w.generate_clips(mf, ids, given=allg, **{**kw, "guide": None, "logprobs": False})
    for b in range(B):
        assert np.array_equal(_np(taken[b][0]), allg[b]) and np.array_equal(_bits(taken[b][1]), _bits(D[b][1])), f"clip {b}: poses are not the decode of the codes"
    # ONE pass with everything: sampling, code_bias, repeat, style and guide on all clips, given rows on clips 1 and 3 (given_keep="body" on
    # clip 1), given POSES on clips 0 and 4 — the pass that stages both kinds into one given block with the shadows' table entries 0.
    # Handing back: clips 1, 2 and 3 are the decode D (a clip does not depend on what its neighbours bring); every clip is the clip alone
    poses = [synth.gt_poses(80 + b, 1, 4 * ((rows[b] + 1) // 2))[0] if b in (0, 4) else None for b in range(B)]
    both = dict(kw, given=[given[b] if b in (1, 3) else None for b in range(B)], given_keep=keep, given_poses=poses)
    P = w.generate_clips(mf, ids, **both)
    for b in (1, 2, 3):
        assert same(P[b], D[b]), f"clip {b}: handing back the head of a guided decode beside clips that bring poses does not return that decode"
    assert not same(P[0], D[0]) or not same(P[4], D[4]), "the given poses changed nothing"
    for b in range(B):
        one = {**both, "given": [both["given"][b]], "given_keep": [keep[b]], "given_poses": [poses[b]], "clip_indices": [200 + b], "style": [style[b]],
               "code_bias": [bias[b]], "repeat": [rep[b]], "sampling": [recs[b]], "guide": [kw["guide"][b]]}
        one.pop("clip_index0")
        if one["given"][0] is None:
            one["given"] = one["given_keep"] = None
        if one["given_poses"][0] is None:
            one["given_poses"] = None
        alone = w.generate_clips([mf[b]], [ids[b]], **one)[0]
        assert same(alone, P[b]), f"clip {b}: the clip alone differs from the clip in the pass that holds given rows, kept positions and given poses"


# ---- graphs -------------------------------------------------------------------------------------------------------------------------------
def test_graphs(w, pix, clips):
    from talkshow_amd import _lib
    rows, mf, other, ids, recs = clips
    rows, mf, other, ids = rows[:4], mf[:4], other[:4], ids[:4]      # a pass shape no other test of this module runs
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3, logprobs=True)
    caps0 = pix.graph_captures()
    plain = w.generate_clips(mf, ids, **kw)
    caps_plain = pix.graph_captures()
    assert caps_plain > caps0
    assert same_all(plain, w.generate_clips(mf, ids, guide=None, **kw)) and pix.graph_captures() == caps_plain      # guide=None: no graph key
    g = _guides(other, ids)[:4]
    r1 = w.generate_clips(mf, ids, guide=g, **kw)
    caps_g = pix.graph_captures()
    assert caps_g > caps_plain, "a guided pass has graph keys of its own"
    assert same_all(r1, w.generate_clips(mf, ids, guide=g, **kw)) and pix.graph_captures() == caps_g               # repeated: nothing captured
    g2 = [dict(e, scale=-e["scale"]) if e is not None else None for e in g]
    r2 = w.generate_clips(mf, ids, guide=g2, **kw)
    assert pix.graph_captures() == caps_g and not same_all(r1, r2), "other scales captured a graph"
    assert same_all(plain, w.generate_clips(mf, ids, **kw)) and pix.graph_captures() == caps_g


# ---- entry points -------------------------------------------------------------------------------------------------------------------------
def test_run_and_generate_batch(w, pix):
    from talkshow_amd import _lib
    B, T = 3, 43
    mf = synth.mfcc_features(500, B, T)
    oth = synth.mfcc_features(600, B, T)
    ids = np.array([1, 0, 2], np.int64)
    g = [{"scale": 2.0, "mfcc": oth[0]}, None, {"scale": -0.5, "id": 3}]
    bkw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=9)
    c, p = w.generate_batch(mf, ids, guide=g, **bkw)
    want = w.generate_clips([torch.from_numpy(m) for m in mf], ids, guide=g, **bkw)
    c0, p0 = w.generate_batch(mf, ids, **bkw)
    assert tuple(c.shape) == (B, T // 4, 2)
    for b in range(B):
        assert np.array_equal(_np(c[b]), _np(want[b][0])) and np.array_equal(_bits(p[b]), _bits(want[b][1]))
    assert np.array_equal(_np(c[1]), _np(c0[1])) and not np.array_equal(_np(c), _np(c0))
    # run: the audio encoder's rows of both conditionings, guide audio as "aud_rows"
    rows_p = w.audioencoder.forward_nlc(torch.from_numpy(mf).cuda())
    rows_q = w.audioencoder.forward_nlc(torch.from_numpy(oth).cuda())
    gr = [{"scale": 2.0, "aud_rows": rows_q[0]}, None, {"scale": -0.5, "id": 3}]
    out = pix.run(torch.from_numpy(ids).cuda(), rows_p, guide=gr, logprobs=True, **bkw)
    lp = w.generate_batch(mf, ids, guide=g, logprobs=True, **bkw)[2]
    assert len(out) == 3 and np.array_equal(_np(out[0]), _np(c)) and np.array_equal(_bits(out[2]), _bits(lp))
    nothing = pix.run(torch.from_numpy(ids).cuda(), rows_p, guide=[None] * B, want_logits=True, **bkw)      # a list of None is no guidance: the logits output stays
    assert nothing[1] is not None and np.array_equal(_np(nothing[0]), _np(pix.run(torch.from_numpy(ids).cuda(), rows_p, **bkw)[0]))
    mine = torch.full((B, T // 4, 2), 7.0, dtype=torch.float32, device="cuda")
    out2 = pix.run(torch.from_numpy(ids).cuda(), rows_p, guide=gr, logprobs=mine, **bkw)
    assert out2[2] is mine and np.array_equal(_bits(mine), _bits(lp)) and len(pix.run(torch.from_numpy(ids).cuda(), rows_p, guide=gr, **bkw)) == 2


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
    oth = [synth.wav16(12000 + k, 1, int(x))[0] for k, x in enumerate(ns)]
    ids = np.array([2, 1], np.int64)
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100)
    mfcc = device_mfcc(16000)
    mf, mq = [mfcc(x)[0] for x in wavs], [mfcc(x)[0] for x in oth]
    want = w.generate_clips(mf, ids, guide=[{"scale": 1.5, "mfcc": mq[0], "id": 0}, {"scale": -0.5, "mfcc": mq[1]}], **kw)
    gw = [{"scale": 1.5, "wav": oth[0], "id": 0}, {"scale": -0.5, "wav": oth[1]}]
    wav = w.generate_clips_from_wav(wavs, 16000, ids, guide=gw, **kw)
    plain = w.generate_clips_from_wav(wavs, 16000, ids, **kw)
    for b in range(len(ns)):
        assert same(wav[b], want[b]), f"generate_clips_from_wav(guide=): recording {b}"
    assert not same_all(wav, plain)
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    fid = np.zeros((1, 4), np.float32)
    out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100, guide=gw)
    assert len(out) == len(ns)
    for b in range(len(ns)):
        f = face.generator.run_clips([wavs[b]], fid)[0]                  # the face half runs on the recordings themselves
        ref = _np(assemble_full(wav[b][1][None], f[None]))[0]
        assert np.array_equal(_np(out[b]), ref), f"whole_body_clips(guide=): recording {b}"


# ---- what is refused, before any launch -----------------------------------------------------------------------------------------------------
def test_refusals(w, pix, clips):
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    rows, mf, other, ids, recs = clips
    B, H = 3, 10
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(np.array([0, 3, 1], np.int64)).cuda()
    caps = pix.graph_captures()
    ok = {"scale": 1.0}
    for entry, pat in (({"scale": 1.0, "wav": other[2]}, r"generate_clips: guide of clip 2: unknown keys"), ({"id": 1}, r"clip 2 needs a scale"),
                       ({"scale": float("nan")}, r"clip 2: the scale is NaN"), ({"scale": float("inf")}, r"clip 2: the scale is infinite"),
                       ({"scale": 2e4}, r"clip 2: the scale exceeds 1e4"), ({"scale": 1.0, "mfcc": other[2][:-1]}, r"clip 2: mfcc must have the clip's own shape"),
                       ({"scale": 1.0, "id": NC}, r"clip 2: the id 4 is outside"), ({"scale": 1.0, "style": np.zeros(NC + 1, F32)}, r"clip 2: the style must have shape"),
                       ({"scale": 1.0, "style": np.asarray([0, np.nan, 0, 0], F32)}, r"clip 2: style"), (7, r"clip 2 must be None or a dict")):
        with pytest.raises(ValueError, match=pat):
            w.generate_clips(mf, ids, guide=[ok, None, entry, None, None])
    with pytest.raises(ValueError, match="one dict for all clips or a list"):
        w.generate_clips(mf, ids, guide=[ok, None])
    with pytest.raises(ValueError, match="top_k = 1"):
        w.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_GREEDY, guide=ok)
    with pytest.raises(ValueError, match="top_k = 1"):
        pix.run(label, aud, mode=_lib.TS_SAMPLE_GREEDY, guide=ok)
    with pytest.raises(ValueError, match="logits output"):
        pix.run(label, aud, want_logits=True, guide=ok)
    with pytest.raises(ValueError, match=r"run: guide of clip 1: aud_rows must have the clip's own shape"):
        pix.run(label, aud, guide=[None, {"scale": 1.0, "aud_rows": aud[1, :-1]}, None])
    with pytest.raises(ValueError, match=r"generate_clips_from_wav: guide of clip 0: wav must have"):
        w.generate_clips_from_wav([synth.wav16(1, 1, 6000)[0]], 16000, [0], guide={"scale": 1.0, "wav": np.zeros(5999, F32)})
    assert pix.graph_captures() == caps
    single = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, False, False)
    with pytest.raises(NotImplementedError, match="single-stack form"):
        single.run(label, aud, guide=ok)
    # the C entries refuse the mode and a bad table themselves, before their first launch
    lib = _lib.load()
    I32P = _lib.C.POINTER(_lib.C.c_int32)
    lens = np.asarray([4 * H, 4 * H, 4 * H - 4], np.int32)
    lens_dev, out = torch.from_numpy(lens).cuda(), torch.full((B, H, 2), -7, dtype=torch.int64, device="cuda")

    def call(mode, guide, scale):
        g, s = np.ascontiguousarray(guide, np.int32), np.ascontiguousarray(scale, F32)
        fixed = (pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H, mode, None, 0, None, _lib.dptr(out))
        name, args = _lib.pixelcnn_mixed_args(fixed, guide=g.ctypes.data_as(I32P), guide_scale=_lib.fptr(s), stream=_lib.stream_ptr())
        assert name == "ts_pixelcnn_generate_guided"
        return getattr(lib, name)(*args)
    assert call(_lib.TS_SAMPLE_GREEDY, [1, -1, -1], [1, 0, 0]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_PHILOX, [3, -1, -1], [1, 0, 0]) != 0 and "clip 0" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_PHILOX, [-1, 2, -1], [0, 1, 0]) != 0 and "length" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_PHILOX, [1, 0, -1], [1, 1, 0]) != 0 and "itself guided" in lib.ts_last_error().decode()
    torch.cuda.synchronize()
    assert (_np(out) == -7).all() and pix.graph_captures() == caps
    assert call(_lib.TS_SAMPLE_PHILOX, [1, -1, -1], [1, 0, 0]) == 0
    torch.cuda.synchronize()
    o = _np(out)
    assert ((o[:2] >= 0) & (o[:2] < V)).all() and np.array_equal(o[0], o[1]) and (o[2, :H - 1] >= 0).all() and (o[2, H - 1] == -1).all()
