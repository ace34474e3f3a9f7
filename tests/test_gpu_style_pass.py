"""Speaker style through the body decode (`ts_body_pixel_infer_mixed_style`, `ts_pixelcnn_generate_mixed_style`,
`ts_body_pixel_infer_mixed_poses_style`; `style=` on `GatedPixelCNN.run`, `TrainWrapper.generate_batch / generate_clips /
generate_clips_from_wav / score_clips / score_motion_clips`, `parallel.whole_body_clips`).

The rule (include/talkshow_hip.h, "speaker style"): the class-conditioning vector of layer l at code row r of clip b is the ascending sum
of w[b, r, c] * E_l[c] over the non-zero weights, product and sum rounded to fp32 separately.  Every check but one is EQUALITY; the one
against the reference arithmetic (test 5) carries a bound measured inside the test, as the comparison's own docstring explains.  The
PixelCNN is the small network of the quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped wrapper.  Every test fails on a
build without the feature: the keyword and the entries do not exist there.
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
EYE = np.eye(NC, dtype=F32)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


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


@pytest.fixture(scope="module")
def grid():
    """B = 3, H = 10 (the 8-row chunk boundary is crossed): audio rows, labels, a fixed random code grid."""
    B, H = 3, 10
    rng = np.random.default_rng(6)
    aud = rng.standard_normal((B, H, 256)).astype(F32)
    label = np.array([0, 3, 1], np.int64)
    codes = rng.integers(0, V, (B, H, 2))
    return B, H, aud, label, codes


def _modes(_lib, rows, rng):
    u = [rng.random((h, 2)).astype(F32) for h in rows]
    return {"greedy": dict(mode=_lib.TS_SAMPLE_GREEDY), "uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u),
            "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50)}


def _blends(rows, seed):
    """One non-trivial weight row per clip: exact zeros, a negative weight, a weight above 1."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(len(rows)):
        x = rng.standard_normal(NC).astype(F32)
        x[b % NC] = 0.0
        x[(b + 1) % NC] = 1.5
        x[(b + 2) % NC] = -0.5
        out.append(x)
    return out


def _tracks(rows, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((h, NC)) * (rng.random((h, NC)) < 0.7)).astype(F32) for h in rows]


# ---- 1. one-hot is the id -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
def test_one_hot_is_the_id(w, clips, how):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    assert min(rows) < 8 < max(rows)
    kw = _modes(_lib, rows, np.random.default_rng(31))[how]
    want = w.generate_clips(mf, ids, logprobs=True, **kw)
    per_clip = w.generate_clips(mf, ids, logprobs=True, style=[EYE[i] for i in ids], **kw)
    track = w.generate_clips(mf, ids, logprobs=True, style=[np.tile(EYE[i], (h, 1)) for i, h in zip(ids, rows)], **kw)
    nones = w.generate_clips(mf, ids, logprobs=True, style=[None] * len(rows), **kw)
    some = w.generate_clips(mf, ids, logprobs=True, style=[None if b % 2 else np.tile(EYE[ids[b]], (rows[b], 1)) for b in range(len(rows))], **kw)
    for b in range(len(rows)):
        assert same(per_clip[b], want[b]), f"{how}: clip {b} ({rows[b]} rows) under its one-hot row differs from its integer id"
        assert same(track[b], want[b]), f"{how}: clip {b} ({rows[b]} rows) under a one-hot track differs from its integer id"
        assert same(nones[b], want[b]) and same(some[b], want[b]), f"{how}: clip {b}: style entries of None are the clip's id"


# ---- 2. a constant track is the per-clip blend ------------------------------------------------------------------------------------------------
def test_constant_track_is_the_blend(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=5, clip_index0=9, sampling=recs, logprobs=True)
    bl = _blends(rows, 41)
    per_clip = w.generate_clips(mf, ids, style=bl, **kw)
    track = w.generate_clips(mf, ids, style=[np.tile(x, (h, 1)) for x, h in zip(bl, rows)], **kw)
    plain = w.generate_clips(mf, ids, **kw)
    for b in range(len(rows)):
        assert same(per_clip[b], track[b]), f"clip {b}: a track of equal rows differs from the per-clip blend"
    assert not all(same(a, b) for a, b in zip(per_clip, plain))       # the blend does something


# ---- 3. a blend is a virtual speaker ------------------------------------------------------------------------------------------------------------
def test_blend_is_a_virtual_speaker(w, pix, sd, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    wv = np.array([0.7, 0.0, 0.3, -0.25], F32)
    sd2 = dict(sd)
    for l in range(DIMS["n_layers"]):
        key = f"layers.{l}.class_cond_embedding.weight"
        t = np.array(sd[key], F32, copy=True)
        t[0] = S.style_rows(wv, t)
        sd2[key] = t
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=3, logprobs=True)
    got = w.generate_clips(mf, ids, style=wv, **kw)
    w.generator = _pix(sd2)
    try:
        want = w.generate_clips(mf, [0], **kw)
    finally:
        w.generator = pix
    for b in range(len(rows)):
        assert same(got[b], want[b]), f"clip {b}: style=w differs from integer id 0 on the model whose row 0 is style_rows(w, table)"


# ---- 4. causality of a track ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 9])
@pytest.mark.parametrize("how", ["greedy", "philox"])
def test_track_is_causal(w, clips, how, R):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    kw = _modes(_lib, rows, np.random.default_rng(33))[how]
    id0 = w.generate_clips(mf, [0], logprobs=True, **kw)
    switch = [np.concatenate([np.tile(EYE[0], (min(R, h), 1)), np.tile(EYE[1], (max(h - R, 0), 1))]) for h in rows]
    got = w.generate_clips(mf, ids, logprobs=True, style=switch, **kw)
    changed = False
    for b, h in enumerate(rows):
        n = min(R, h)
        assert np.array_equal(_np(got[b][0])[:n], _np(id0[b][0])[:n]), f"{how}, R = {R}: clip {b}: codes of rows below R differ from the id-0 decode"
        assert np.array_equal(_bits(got[b][2])[:n], _bits(id0[b][2])[:n]), f"{how}, R = {R}: clip {b}: log-probabilities of rows below R differ"
        if h > R:
            changed |= not np.array_equal(_bits(got[b][2])[R:], _bits(id0[b][2])[R:])
    assert changed                                                      # the switch does something from row R on


# ---- 5. against the reference arithmetic ------------------------------------------------------------------------------------------------------
def _oracle_logprobs(monkeypatch, sd, aud, label, codes, patched):
    """float64 log_softmax of the torch oracle's teacher-forced logits at `codes`; label (B,) int64, or, with the patched layer, (B,H,NC)."""
    import torch.nn.functional as F

    from oracle import torch_port as TP

    def layer(x_v, x_h, lab, sdl, p, kernel, residual):
        """oracle.torch_port._gated_layer with `label` a (B, H, NC) float tensor: h is (B, 2D, H, 1), one vector per code row."""
        h = torch.matmul(lab, sdl[p + ".class_cond_embedding.weight"]).permute(0, 2, 1)[:, :, :, None]
        h_vert = F.conv2d(x_v, sdl[p + ".vert_stack.weight"], sdl[p + ".vert_stack.bias"], 1, (kernel // 2, 1))
        h_vert = h_vert[:, :, :x_v.size(-2), :]
        out_v = TP._gate(h_vert + h)
        h_horiz = F.conv2d(x_h, sdl[p + ".horiz_stack.weight"], sdl[p + ".horiz_stack.bias"], 1, (0, 1))
        h_horiz = h_horiz[:, :, :, :x_h.size(-1)]
        v2h = F.conv2d(h_vert, sdl[p + ".vert_to_horiz.weight"], sdl[p + ".vert_to_horiz.bias"])
        out = TP._gate(v2h + h_horiz + h)
        out_h = F.conv2d(out, sdl[p + ".horiz_resid.weight"], sdl[p + ".horiz_resid.bias"])
        if residual:
            out_h = out_h + x_h
        return out_v, out_h
    if patched:
        monkeypatch.setattr(TP, "_gated_layer", layer)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items() if isinstance(v, np.ndarray)}
    v = t["layers.0.vert_stack.weight"].clone(); v[:, :, -1] = 0                   # make_causal, as oracle.torch_port.pixelcnn_generate does
    hz = t["layers.0.horiz_stack.weight"].clone(); hz[:, :, :, -1] = 0
    t["layers.0.vert_stack.weight"], t["layers.0.horiz_stack.weight"] = v, hz
    a = torch.from_numpy(aud).double().permute(0, 2, 1).unsqueeze(-1).repeat(1, 1, 1, 2)
    with torch.no_grad():
        lg = TP.pixelcnn_forward(torch.from_numpy(codes), label, a, t, DIMS["n_layers"])      # (B, V, H, 2)
        lp = torch.log_softmax(lg.double(), 1)
        return torch.gather(lp, 1, torch.from_numpy(codes)[:, None]).squeeze(1).numpy()


def test_against_the_reference_arithmetic(pix, sd, grid, monkeypatch):
    """The log-probabilities of a fixed random code grid, teacher forced (every row given), under a switching track and under a
    two-speaker blend, against float64 log_softmax of the torch oracle's logits with its gated layer patched to take (B, H, NC) weights.
    tests/test_gpu_logprob_pass.py holds no comparison of the integer-id pass with the oracle, so the bound is measured here: e0 = the
    largest error of the integer-id pass against the UNPATCHED oracle (evaluated in float64) on the same grid, and a style may err by
    4 e0 — blends of up to NC terms add roundings to h.  The figures of a run are printed; DESIGN.md section 5 ("Speaker style")
    records them."""
    from talkshow_amd import _lib
    B, H, aud, label, codes = grid
    audd = torch.from_numpy(aud).cuda()
    label_dev = torch.from_numpy(label).cuda()

    def device(style):
        out = pix.run(label_dev, audd, mode=_lib.TS_SAMPLE_GREEDY, given=codes, logprobs=True, style=style)
        assert np.array_equal(_np(out[0]), codes)
        return _np(out[2]).astype(np.float64)
    e0 = float(np.abs(device(None) - _oracle_logprobs(monkeypatch, sd, aud, torch.from_numpy(label), codes, False)).max())
    print(f"integer ids against the unpatched oracle: max |error| = {e0:.3e}")
    assert 0 < e0 < 1e-3
    switch = [np.concatenate([np.tile(EYE[label[b]], (4 + b, 1)), np.tile(EYE[(label[b] + 1) % NC], (H - 4 - b, 1))]) for b in range(B)]
    blend = np.array([[0.6, 0.0, 0.4, 0.0], [0.0, 1.5, 0.0, -0.5], [0.3, 0.0, 0.0, 0.7]], F32)
    for name, style, lab in (("switching track", switch, np.stack(switch)), ("two-speaker blend", blend, np.tile(blend[:, None], (1, H, 1)))):
        ref = _oracle_logprobs(monkeypatch, sd, aud, torch.from_numpy(lab.astype(np.float64)), codes, True)
        err = float(np.abs(device(style) - ref).max())
        print(f"{name} against the patched oracle: max |error| = {err:.3e} (allowed {4 * e0:.3e})")
        assert err <= 4 * e0, f"{name}: {err:.3e} > 4 x {e0:.3e}"


# ---- 6. neighbours ------------------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_neighbours(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    tr = _tracks(rows, 43)
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=11, logprobs=True)
    B = len(rows)
    together = w.generate_clips(mf, ids, style=tr, clip_indices=[70 + b for b in range(B)], **kw)
    other = [t[::-1].copy() for t in tr]
    for b in range(B):
        alone = w.generate_clips([mf[b]], [ids[b]], style=[tr[b]], clip_indices=[70 + b], **kw)[0]
        assert same(alone, together[b]), f"clip {b} ({rows[b]} rows) alone differs from the clip inside a pass of tracks"
    b = int(np.argmax(rows))
    mixed = w.generate_clips(mf, ids, style=[tr[k] if k == b else other[k] for k in range(B)], clip_indices=[70 + k for k in range(B)], **kw)
    assert same(mixed[b], together[b])                                   # other neighbours' tracks, the same clip


# ---- 7. composition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", [True, False])
def test_composition(w, clips, records):
    """One pass with (records: sampling records,) given rows on half the clips, given_keep="body" on some of them, and tracks: handing
    back its own head returns it bit for bit.  `score_clips` scores under the model's own distribution (it takes no sampling records), so
    its equality with the pass's log-probabilities is checked on the pass WITHOUT records."""
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    B = len(rows)
    tr = _tracks(rows, 47)
    tr[1] = _blends(rows, 48)[1]                                         # a per-clip row and an id among the tracks
    tr[4] = None
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=19, clip_index0=200, logprobs=True, style=tr)
    if records:
        kw["sampling"] = recs
    D = w.generate_clips(mf, ids, **kw)
    G = [rows[b] if b == 0 else (rows[b] + 1) // 2 for b in range(B)]
    given = [_np(D[b][0])[:G[b]] if b % 2 == 0 else None for b in range(B)]
    keep = ["body" if (b % 4 == 0) else None for b in range(B)]
    back = w.generate_clips(mf, ids, given=given, given_keep=keep, **kw)
    for b in range(B):
        assert same(back[b], D[b]), f"clip {b}: handing back the head of a decode with the same style does not return that decode"
    plain = w.generate_clips(mf, ids, **{**kw, "style": None})
    assert not all(same(a, b) for a, b in zip(D, plain))
    if not records:
        sc = w.score_clips(mf, ids, [_np(d[0]) for d in D], style=tr)
        for b in range(B):
            assert np.array_equal(_bits(sc[b][0]), _bits(D[b][2])), f"clip {b}: score_clips(style=) differs from the decode's log-probabilities"
        sc0 = w.score_clips(mf, ids, [_np(d[0]) for d in D])
        assert not all(np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(sc, sc0))


# ---- 8. graphs ----------------------------------------------------------------------------------------------------------------------------------
def test_graphs(w, pix, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    # five of the six clips: a pass shape no other test of this module runs, so what is captured below is captured HERE
    rows, mf, ids = rows[:5], mf[:5], ids[:5]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3, logprobs=True)
    caps0 = pix.graph_captures()
    plain = w.generate_clips(mf, ids, **kw)
    caps_plain = pix.graph_captures()
    assert caps_plain > caps0
    assert same_all(plain, w.generate_clips(mf, ids, **kw)) and pix.graph_captures() == caps_plain        # warm
    # style=None: the returns and the graphs of the call without the keyword
    assert same_all(plain, w.generate_clips(mf, ids, style=None, **kw)) and pix.graph_captures() == caps_plain
    # per-clip rows: the plain pass's keys and graphs (the conditioning rows' content is in no key)
    bl = w.generate_clips(mf, ids, style=_blends(rows, 51), **kw)
    assert pix.graph_captures() == caps_plain and not same_all(bl, plain)
    # a tracked pass has keys of its own (bit 4): as many as the plain pass has, at most 14 of the 16 chunk slots
    t1 = w.generate_clips(mf, ids, style=_tracks(rows, 52), **kw)
    caps_t = pix.graph_captures()
    assert caps_t > caps_plain and caps_t - caps_plain <= 14 and caps_t - caps_plain == caps_plain - caps0
    t2 = w.generate_clips(mf, ids, style=_tracks(rows, 53), **kw)
    t1b = w.generate_clips(mf, ids, style=_tracks(rows, 52), **kw)
    assert pix.graph_captures() == caps_t                          # a repeated tracked pass captures nothing, whatever its weights
    assert same_all(t1, t1b) and not same_all(t1, t2)
    # the plain pass afterwards finds its own graphs and returns what it returned
    assert same_all(plain, w.generate_clips(mf, ids, **kw)) and pix.graph_captures() == caps_t
    assert same_all(bl, w.generate_clips(mf, ids, style=_blends(rows, 51), **kw)) and pix.graph_captures() == caps_t


def same_all(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


# ---- 9. whole_body_clips and the entries that start from recordings -------------------------------------------------------------------------------
def test_whole_body_clips_and_recordings(w):
    import argparse
    import json

    import nets
    from talkshow_amd import _lib, parallel
    from talkshow_amd.config import Object
    from talkshow_amd.frontend import device_mfcc, mixed_tables
    from talkshow_amd.pose_index import assemble_full
    ns = [5872, 16000]
    wavs = [synth.wav16(11000 + k, 1, int(x))[0] for k, x in enumerate(ns)]
    ids = np.array([2, 1], np.int64)
    rows = [int(r) for r in mixed_tables(ns, 16000)["code_rows"]]
    style = [_tracks(rows, 61)[0], np.array([0.5, 0.0, 0.0, 0.5], F32)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100)
    mf = [device_mfcc(16000)(x)[0] for x in wavs]
    want = w.generate_clips(mf, ids, style=style, **kw)
    wav = w.generate_clips_from_wav(wavs, 16000, ids, style=style, **kw)
    plain = w.generate_clips_from_wav(wavs, 16000, ids, **kw)
    for b in range(len(ns)):
        assert same(wav[b], want[b]), f"generate_clips_from_wav(style=): recording {b}"
    assert not same_all(wav, plain)
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    fid = np.zeros((1, 4), np.float32)
    out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100, style=style)
    out0 = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100)
    for b in range(len(ns)):
        f = face.generator.run_clips([wavs[b]], fid)[0]                  # the face half, which never sees the style
        ref = _np(assemble_full(wav[b][1][None], f[None]))[0]
        ref0 = _np(assemble_full(plain[b][1][None], f[None]))[0]
        assert np.array_equal(_np(out[b]), ref), f"whole_body_clips(style=): recording {b}: body columns / face columns"
        assert np.array_equal(_np(out0[b]), ref0) and not np.array_equal(ref, ref0)


# ---- 10. what the Python layer refuses -------------------------------------------------------------------------------------------------------------
def test_refusals(w, pix, clips, grid):
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    rows, mf, ids, recs = clips
    B, H, aud, label, codes = grid
    audd = torch.from_numpy(aud).cuda()
    label_dev = torch.from_numpy(label).cuda()
    caps = pix.graph_captures()
    ok = [EYE[0]] * len(rows)
    for bad, pat in (([*ok[:2], np.ones((rows[2] + 1, NC), F32), *ok[3:]], r"generate_clips: style of clip 2 must have shape"),
                     ([*ok[:4], np.ones(NC + 1, F32), *ok[5:]], r"generate_clips: style of clip 4 has 5 weights per row"),
                     ([*ok[:5], np.array([0, np.nan, 0, 1], F32)], r"generate_clips: style of clip 5: .*not finite")):
        with pytest.raises(ValueError, match=pat):
            w.generate_clips(mf, ids, style=bad)
    with pytest.raises(ValueError, match=r"score_clips: style of clip 1 has 3 weights"):
        w.score_clips(mf, ids, [np.zeros((h, 2), np.int64) for h in rows], style=[ok[0], np.ones(3, F32), *ok[2:]])
    with pytest.raises(ValueError, match=r"run: style of clip 1 must have shape"):
        pix.run(label_dev, audd, style=[None, np.ones((H + 1, NC), F32), None])
    with pytest.raises(ValueError, match="teacher forcing"):
        pix.run(label_dev, audd, mode=_lib.TS_TEACHER_FORCED, codes=codes, style=EYE[0])
    assert pix.graph_captures() == caps
    single = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], NC, False, False)
    with pytest.raises(NotImplementedError, match="single-stack form"):
        single.run(label_dev, audd, style=EYE[0])
    # the C entries: style_rows is 1 or H_max; a style without labels is a pass
    lib = _lib.load()
    I32P = _lib.C.POINTER(_lib.C.c_int32)
    lens = np.full(B, 4 * H, np.int32)
    lens_dev, out = torch.from_numpy(lens).cuda(), torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")
    st = torch.from_numpy(np.tile(EYE[label][:, None], (1, H, 1))).cuda()
    args = (pix.handle(), None, _lib.dptr(audd), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H, _lib.TS_SAMPLE_GREEDY, None, 0, None,
            _lib.dptr(out), None, 0, None, None, None, None, None)
    assert lib.ts_pixelcnn_generate_mixed_style(*args, _lib.dptr(st), H - 1, _lib.stream_ptr()) != 0
    assert "style_rows is 1 or H_max" in lib.ts_last_error().decode()
    assert lib.ts_pixelcnn_generate_mixed_style(*args, None, 0, _lib.stream_ptr()) != 0            # neither labels nor a style
    _lib.check(lib.ts_pixelcnn_generate_mixed_style(*args, _lib.dptr(st), H, _lib.stream_ptr()))   # label_dev == NULL with a style
    want = pix.run(label_dev, audd, mode=_lib.TS_SAMPLE_GREEDY)[0]
    assert np.array_equal(_np(out), _np(want))
