"""Kept positions through the body decode (`ts_body_pixel_infer_mixed_keep`, `ts_pixelcnn_generate_mixed_keep`,
`ts_body_pixel_infer_mixed_poses_keep`; `given_keep=` on `GatedPixelCNN.run`, `TrainWrapper.generate_batch / generate_clips /
generate_clips_from_wav`, `parallel.whole_body_clips`).

The rule (include/talkshow_hip.h, "kept positions"): position (r, j) of clip b is TAKEN iff 2 r + j < 2 G_b and (no mask or
keep[b, r, j] != 0); every other position is produced as without given rows, from the Philox number / uniform of its absolute position.
Every check is EQUALITY.  The PixelCNN is the small network of the quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped
wrapper.  Every test fails on a build without the feature: the keyword and the entries do not exist there.
"""
import ctypes as C
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
V = DIMS["input_dim"]
ROWS = [20, 17, 17, 9, 8, 3]                       # code rows of the six clips: two chunks and a half, ties, a clip shorter than a chunk
GIVEN = [9, 17, 0, 8, 1, 3]                        # across the chunk boundary, a whole clip, none, exactly one chunk, one row, a whole short clip
RECS = [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.7, 1.0, 12), (0.5, 0.5, 40), (1.0, 1.0, 0), (4.0, 0.95, 64)]
I32P = C.POINTER(C.c_int32)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def pix():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], 4, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=11, **DIMS)))
    return m


@pytest.fixture(scope="module")
def w(pix):
    """The shipped wrapper (audio encoder, VQ decoders) around the small code predictor; its own predictor is kept as `full_generator`."""
    import bench
    wr = bench.build_models(0, seed=7)[0]
    wr.full_generator = wr.generator
    wr.generator = pix
    return wr


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(21)
    order = rng.permutation(len(ROWS))               # submitted shuffled: the Python layer sorts and un-sorts
    rows = [ROWS[i] for i in order]
    G = [GIVEN[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(3000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    recs = [RECS[i] for i in order]
    return rows, G, mf, ids, recs


@pytest.fixture(scope="module")
def decode(w, clips):
    """D: the plain Philox decode of the six clips with per-clip records, computed once."""
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50, sampling=recs)
    return kw, [tuple(_np(t) for t in r) for r in w.generate_clips(mf, ids, logprobs=True, **kw)]


@pytest.fixture(scope="module")
def grid():
    """B = 4, H = 10 (the 8-row chunk boundary is crossed): audio rows, labels, uniforms."""
    B, H = 4, 10
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(synth.speaker_ids(B)).cuda()
    u = rng.random((B, H, 2)).astype(F32)
    return B, H, aud, label, u


def _modes(_lib, rows, recs, rng):
    """greedy, injected uniforms and Philox for `generate_clips`; the drawing modes with per-clip records."""
    u = [rng.random((h, 2)).astype(F32) for h in rows]
    return {"greedy": dict(mode=_lib.TS_SAMPLE_GREEDY), "uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs),
            "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50, sampling=recs)}


def _c_pass(pix, label, aud, lens, mode, u, seed, table, block, keep, codes, lp):
    """`ts_pixelcnn_generate_mixed_keep` itself, on caller-owned device blocks."""
    from talkshow_amd import _lib
    B, H = aud.shape[0], aud.shape[1]
    lens_dev = torch.from_numpy(lens).cuda()
    ci = torch.arange(B, dtype=torch.int64, device="cuda") + 7
    _lib.check(_lib.load().ts_pixelcnn_generate_mixed_keep(
        pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H, mode, _lib.dptr(u), seed,
        _lib.dptr(ci), _lib.dptr(codes), None, 0, _lib.dptr(lp), _lib.dptr(block), table.ctypes.data_as(I32P), None, _lib.dptr(keep),
        _lib.stream_ptr()))


# ---- 1. an all-ones mask is given= ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
def test_all_ones_is_given(w, clips, how):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    rng = np.random.default_rng(31)
    kw = _modes(_lib, rows, recs, rng)[how]
    given = [rng.integers(0, V, (g, 2)) for g in G]
    want = w.generate_clips(mf, ids, logprobs=True, given=given, **kw)
    ones = [np.ones((g, 2), np.uint8) for g in G]
    got = w.generate_clips(mf, ids, logprobs=True, given=given, given_keep=ones, **kw)
    for b in range(len(rows)):
        assert same(got[b], want[b]), f"{how}: clip {b} ({rows[b]} rows, G = {G[b]}) under an all-ones mask differs from given="
        assert np.array_equal(_np(got[b][0])[:G[b]], given[b])


# ---- 2. an all-zero mask is the pass without given rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
def test_all_zero_is_the_plain_pass(w, pix, clips, grid, how):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    rng = np.random.default_rng(32)
    kw = _modes(_lib, rows, recs, rng)[how]
    plain = w.generate_clips(mf, ids, logprobs=True, **kw)
    poison = [np.where(rng.random((h, 2)) < 0.5, -7, 2 ** 40) for h in rows]                      # G_b = H_b, never read
    got = w.generate_clips(mf, ids, logprobs=True, given=poison, given_keep=[np.zeros((h, 2), bool) for h in rows], **kw)
    for b in range(len(rows)):
        assert same(got[b], plain[b]), f"{how}: clip {b} ({rows[b]} rows) under an all-zero mask differs from the plain pass"
    # the C entry with the poison ON THE DEVICE (the Python helper blanks unkept entries of its block)
    B, H, aud, label, u = grid
    gkw = {"greedy": dict(mode=_lib.TS_SAMPLE_GREEDY), "uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u),
           "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=41)}[how]
    c0, _, lp0 = pix.run(label, aud, clip_index0=7, logprobs=True, **gkw)
    block = torch.from_numpy(np.where(rng.random((B, H, 2)) < 0.5, -7, 2 ** 40)).cuda()
    keep = torch.zeros((B, H, 2), dtype=torch.uint8, device="cuda")
    codes = torch.full((B, H, 2), -5, dtype=torch.int64, device="cuda")
    lp = torch.full((B, H, 2), 3.0, dtype=torch.float32, device="cuda")
    _c_pass(pix, label, aud, np.full(B, 4 * H, np.int32), gkw["mode"], torch.from_numpy(u).cuda() if how == "uniforms" else None, gkw.get("seed", 0),
            np.full(B, H, np.int32), block, keep, codes, lp)
    assert np.array_equal(_np(codes), _np(c0)) and np.array_equal(_bits(lp), _bits(lp0))


# ---- 3. a prefix-shaped mask is given= with G_b = g ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms", "philox"])
def test_prefix_mask_is_a_shorter_prefix(pix, grid, how):
    from talkshow_amd import _lib
    B, H, aud, label, u = grid
    g = [0, 3, 8, 9]
    rng = np.random.default_rng(33)
    full = rng.integers(0, V, (B, H, 2))
    mask = np.zeros((B, H, 2), np.uint8)
    for b in range(B):
        mask[b, :g[b]] = 1
    recs = [(0.7, 0.9, 0), (1.0, 1.0, 1), (2.5, 0.6, 30), (1.0, 0.999, 5)]
    kw = {"greedy": dict(mode=_lib.TS_SAMPLE_GREEDY), "uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs),
          "philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=31, sampling=recs)}[how]
    want = pix.run(label, aud, clip_index0=4, logprobs=True, given=[full[b, :g[b]] for b in range(B)], **kw)
    dirty = np.where(mask != 0, full, -7)
    got = pix.run(label, aud, clip_index0=4, logprobs=True, given=dirty, given_keep=mask, **kw)
    assert got[1] is None and np.array_equal(_np(got[0]), _np(want[0])) and np.array_equal(_bits(got[2]), _bits(want[2]))
    for b in range(B):
        assert np.array_equal(_np(got[0])[b, :g[b]], full[b, :g[b]])


# ---- 4. redraw identity -------------------------------------------------------------------------------------------------------------------
def test_redraw_identity(w, clips, decode):
    rows, G, mf, ids, recs = clips
    kw, D = decode
    n = len(rows)
    given = [D[b][0].copy() for b in range(n)]
    rng = np.random.default_rng(34)
    random_mask = [rng.integers(0, 2, (h, 2)).astype(bool) for h in rows]
    for name, keep in (("body", "body"), ("hand", "hand"), ("random", random_mask), ("per clip", ["body", None, "hand", random_mask[3], "body", "hand"])):
        res = w.generate_clips(mf, ids, logprobs=True, given=given, given_keep=keep, **kw)
        for b in range(n):
            assert same(res[b], D[b]), f"given_keep={name}: clip {b} is not the decode it was given"
    other = dict(kw, seed=kw["seed"] + 1)
    res = [tuple(_np(t) for t in r) for r in w.generate_clips(mf, ids, logprobs=True, given=given, given_keep="body", **other)]
    assert all(np.array_equal(res[b][0][:, 0], D[b][0][:, 0]) for b in range(n)), "the kept body column"
    assert any(not np.array_equal(res[b][0][:, 1], D[b][0][:, 1]) for b in range(n)), "another seed never drew another hand code"
    res = [tuple(_np(t) for t in r) for r in w.generate_clips(mf, ids, logprobs=True, given=given, given_keep="hand", **other)]
    assert all(np.array_equal(res[b][0][:, 1], D[b][0][:, 1]) for b in range(n)), "the kept hand column"
    assert any(not np.array_equal(res[b][0][:, 0], D[b][0][:, 0]) for b in range(n))


# ---- 5. self-consistency against the teacher-forced logits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["greedy", "uniforms"])
def test_self_consistency(pix, grid, how):
    from talkshow_amd import _lib
    B, H, aud, label, u = grid
    rng = np.random.default_rng(35)
    G = [10, 3, 8, 9]
    given = rng.integers(0, V, (B, H, 2))
    mask = rng.integers(0, 2, (B, H, 2)).astype(np.uint8)
    recs = [(0.7, 0.9, 0), (1.0, 1.0, 1), (2.5, 0.6, 30), (1.0, 0.999, 5)] if how == "uniforms" else None
    kw = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs) if how == "uniforms" else dict(mode=_lib.TS_SAMPLE_GREEDY)
    X, none, lp = pix.run(label, aud, logprobs=True, given=[given[b, :G[b]] for b in range(B)], given_keep=[mask[b, :G[b]] for b in range(B)], **kw)
    X, lp = _np(X), _np(lp)
    _, L = pix.run(label, aud, mode=_lib.TS_TEACHER_FORCED, codes=torch.from_numpy(X).cuda(), want_logits=True)
    L = _np(L)
    kept_any = produced_below = 0
    for r in range(H):
        for j in range(2):
            forced = S.keep_forced(G, mask, r, j)
            idx, wlp = S.sample_given(L[:, r, j], u[:, r, j], forced, given[:, r, j], recs, greedy=how == "greedy")
            print(how, r, j, "forced", forced, "X", X[:, r, j], "want", idx, "lp", lp[:, r, j], wlp)
            assert np.array_equal(X[:, r, j], idx), f"{how}: position ({r}, {j})"
            assert np.array_equal(X[forced, r, j], given[forced, r, j])
            if how == "greedy":
                assert np.array_equal(X[~forced, r, j], np.argmax(L[~forced, r, j], axis=-1))
            assert np.array_equal(lp[:, r, j].view(np.uint32), wlp.view(np.uint32)), f"{how}: log-probabilities at ({r}, {j})"
            kept_any += int(forced.sum())
            produced_below += int((~forced & (np.asarray(G) > r)).sum())
    assert kept_any > 10 and produced_below > 10


# ---- 6. neighbours -----------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_neighbours(w, clips):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    n = len(rows)
    rng = np.random.default_rng(36)
    given = [rng.integers(0, V, (G[b], 2)) for b in range(n)]
    keep = [rng.integers(0, 2, (G[b], 2)).astype(np.uint8) for b in range(n)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123)
    res = w.generate_clips(mf, ids, sampling=recs, clip_index0=50, logprobs=True, given=given, given_keep=keep, **kw)
    for b in range(n):
        alone = w.generate_clips([mf[b]], ids[b:b + 1], sampling=[recs[b]], clip_indices=[50 + b], logprobs=True, given=[given[b]], given_keep=[keep[b]], **kw)[0]
        assert same(res[b], alone), f"clip {b} ({rows[b]} rows, G = {G[b]}) differs from the clip alone"
        c = _np(res[b][0])[:G[b]]
        assert np.array_equal(c[keep[b] != 0], given[b][keep[b] != 0])
    # one clip changes its mask: the five others keep their bits
    k = rows.index(20)
    k2 = list(keep)
    k2[k] = 1 - keep[k]
    res2 = w.generate_clips(mf, ids, sampling=recs, clip_index0=50, logprobs=True, given=given, given_keep=k2, **kw)
    for b in range(n):
        if b != k:
            assert same(res[b], res2[b]), f"clip {b} changed when clip {k} changed its mask"
    assert not np.array_equal(_np(res2[k][0]), _np(res[k][0]))


# ---- 7. graphs ---------------------------------------------------------------------------------------------------------------------------
def test_graphs(w, pix, clips, grid):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    # five of the six clips: a pass shape no other test of this module runs, so what is captured below is captured HERE
    rows, G, mf, ids, recs = rows[:5], G[:5], mf[:5], ids[:5], recs[:5]
    lib = _lib.load()
    B, H, aud, label, _ = grid
    rng = np.random.default_rng(37)
    given = [rng.integers(0, V, (g, 2)) for g in G]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3, sampling=recs, logprobs=True)

    def stats():
        nl, fl = C.c_int64(0), C.c_double(0)
        _lib.check(lib.ts_pixelcnn_graph_stats(pix.handle(), _lib.stream_ptr(), B, H, _lib.TS_SAMPLE_PHILOX, C.byref(nl), C.byref(fl)))
        return nl.value, fl.value
    for _ in range(4):                                          # the uniform call's whole-call graph: what the statistics speak of
        pix.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=5)
    before = stats()
    plain = w.generate_clips(mf, ids, **kw)
    caps_plain = pix.graph_captures()
    giv = w.generate_clips(mf, ids, given=given, **kw)
    caps = pix.graph_captures()
    assert all(same(a, b) for a, b in zip(giv, w.generate_clips(mf, ids, given=given, **kw))) and pix.graph_captures() == caps      # both warm
    # given_keep=None: the returns and the graphs of the call without the keyword
    none = w.generate_clips(mf, ids, given=given, given_keep=None, **kw)
    assert all(same(a, b) for a, b in zip(giv, none)) and pix.graph_captures() == caps
    keep = [rng.integers(0, 2, (g, 2)).astype(bool) for g in G]
    first = w.generate_clips(mf, ids, given=given, given_keep=keep, **kw)
    caps_masked = pix.graph_captures()
    assert caps_masked > caps                                   # the masked form has keys of its own (bit 3) ...
    assert caps_masked - caps <= 14 and caps_masked - caps == caps - caps_plain      # ... as many as the given pass has (at most 14 of the 16 chunk slots)
    second = w.generate_clips(mf, ids, given=given, given_keep=keep, **kw)
    other = w.generate_clips(mf, ids, given=given, given_keep=[~k for k in keep], **kw)
    w.generate_clips(mf, ids, given=given, given_keep="hand", **kw)
    assert pix.graph_captures() == caps_masked                  # a repeated masked pass captures nothing, whatever its mask
    assert all(same(a, b) for a, b in zip(first, second)) and not all(same(a, b) for a, b in zip(first, other))
    # the plain pass and the given pass that were warm before capture nothing after it, and return what they returned
    plain2 = w.generate_clips(mf, ids, **kw)
    giv2 = w.generate_clips(mf, ids, given=given, **kw)
    assert pix.graph_captures() == caps_masked
    assert all(same(a, b) for a, b in zip(plain, plain2)) and all(same(a, b) for a, b in zip(giv, giv2))
    caps2 = pix.graph_captures()
    pix.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=5)
    assert pix.graph_captures() == caps2 and stats() == before  # the launch counts there were


# ---- 8. from poses, and the entries that start from recordings --------------------------------------------------------------------------------
def test_from_poses_and_recordings(w):
    import argparse
    import json

    import nets
    from nets.init_model import init_model
    from talkshow_amd import _lib, parallel
    from talkshow_amd.config import Object, load_JsonConfig
    from talkshow_amd.frontend import device_mfcc, mixed_tables
    from talkshow_amd.pose_index import assemble_full
    vw = init_model("s2g_body_vq", argparse.Namespace(gpu=0, infer=True), load_JsonConfig(os.path.join(REPO, "config", "body_vq.json")))
    vw.g_body, vw.g_hand = w.g_body, w.g_hand
    small, w.generator = w.generator, w.full_generator        # the encoders' codes need the full vocabulary
    try:
        ns = [5872, 16000, 1602, 8001]
        wavs = [synth.wav16(11000 + k, 1, int(x))[0] for k, x in enumerate(ns)]
        ids = (np.arange(len(ns)) % 4).astype(np.int64)
        rows = [int(r) for r in mixed_tables(ns, 16000)["code_rows"]]
        frames = [4 * min(3, rows[0]) + 2, 0, 4 * rows[2], 4]
        gp = [None if f == 0 else synth.gt_poses(600 + b, 1, f)[0] for b, f in enumerate(frames)]
        enc = iter(vw.encode_clips([g for g in gp if g is not None]))
        given = [None if g is None else _np(next(enc)) for g in gp]
        kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100)
        mf = [device_mfcc(16000)(x)[0] for x in wavs]
        want = w.generate_clips(mf, ids, given=given, given_keep="body", **kw)
        got = w.generate_clips(mf, ids, given_poses=gp, given_keep="body", **kw)
        all_kept = w.generate_clips(mf, ids, given=given, **kw)
        for b in range(len(ns)):
            assert same(got[b], want[b]), f"clip {b}: given_poses + given_keep='body' differs from given=encode_clips(...) + given_keep='body'"
            g = 0 if given[b] is None else len(given[b])
            assert np.array_equal(_np(got[b][0])[:g, 0], given[b][:, 0] if g else np.zeros(0, np.int64))
        assert not all(same(a, b) for a, b in zip(want, all_kept))             # the hands were redrawn somewhere
        # both kinds in one pass, per-clip entries
        mixed = w.generate_clips(mf, ids, given=[given[0], None, None, None], given_poses=[None, None, gp[2], gp[3]],
                                 given_keep=["body", None, "body", "body"], **kw)
        assert all(same(a, b) for a, b in zip(mixed, want))
        # the entries that start from recordings carry the keyword
        wav = w.generate_clips_from_wav(wavs, 16000, ids, given_poses=gp, given_keep="body", **kw)
        for b in range(len(ns)):
            assert same(wav[b], want[b]), f"generate_clips_from_wav: clip {b}"
        cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
        face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
        face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
        out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100, given=given, given_keep="body")
        fid = np.zeros((1, 4), np.float32)
        for b in range(len(ns)):
            f = face.generator.run_clips([wavs[b]], fid)[0]
            ref = _np(assemble_full(want[b][1][None], f[None]))[0]
            assert np.array_equal(_np(out[b]), ref), f"whole_body_clips: recording {b}"
    finally:
        w.generator = small


# ---- 9. what the Python layer refuses ------------------------------------------------------------------------------------------------------
def test_refusals(w, pix, clips, grid):
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    rows, G, mf, ids, recs = clips
    n = len(rows)
    B, H, aud, label, _ = grid
    given = [np.zeros((g, 2), np.int64) for g in G]
    caps = pix.graph_captures()
    k = G.index(9)
    with pytest.raises(ValueError, match=rf"clip {k} must have shape \(9, 2\)"):
        w.generate_clips(mf, ids, given=given, given_keep=[None] * k + [np.ones((8, 2), bool)] + [None] * (n - k - 1))
    with pytest.raises(ValueError, match="'legs'"):
        w.generate_clips(mf, ids, given=given, given_keep="legs")
    with pytest.raises(ValueError, match="brings none"):
        w.generate_clips(mf, ids, given_keep="body")
    z = G.index(0)
    g2 = list(given)
    g2[z] = None
    with pytest.raises(ValueError, match=rf"clip {z} selects from given rows, but the clip brings none"):
        w.generate_clips(mf, ids, given=g2, given_keep=[None] * z + ["hand"] + [None] * (n - z - 1))
    bad = [g.copy() for g in given]
    bad[k][4, 1] = V
    w.generate_clips(mf, ids, given=bad, given_keep="body", mode=_lib.TS_SAMPLE_GREEDY)          # unkept: never read, accepted
    with pytest.raises(ValueError, match=rf"clip {k} hold the code {V}"):
        w.generate_clips(mf, ids, given=bad, given_keep="hand", mode=_lib.TS_SAMPLE_GREEDY)
    with pytest.raises(ValueError, match="brings none"):
        pix.run(label, aud, given_keep="body")
    single = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], 4, True, False)
    with pytest.raises(NotImplementedError):
        single.run(label, aud, given_keep="body")
    # the C entries refuse a mask without the block it selects from, before anything is launched
    codes = torch.full((B, H, 2), -5, dtype=torch.int64, device="cuda")
    keep = torch.ones((B, H, 2), dtype=torch.uint8, device="cuda")
    lens = np.full(B, 4 * H, np.int32)
    lens_dev = torch.from_numpy(lens).cuda()
    rc = _lib.load().ts_pixelcnn_generate_mixed_keep(pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H,
                                                     _lib.TS_SAMPLE_GREEDY, None, 0, None, _lib.dptr(codes), None, 0, None, None, None, None,
                                                     _lib.dptr(keep), _lib.stream_ptr())
    assert rc != 0 and "needs the given codes" in _lib.load().ts_last_error().decode()
    torch.cuda.synchronize()
    assert (_np(codes) == -5).all()
