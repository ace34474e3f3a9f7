"""Given rows through the body decode (`ts_body_pixel_infer_mixed_given`, `ts_pixelcnn_generate_mixed_given`; `given=` on
`GatedPixelCNN.run`, `TrainWrapper.generate_batch / generate_clips / generate_clips_from_wav`, `parallel.whole_body_clips`).

The contract (include/talkshow_hip.h, "given rows"): clip b's first G_b code rows are TAKEN, the rest produced as without them; a clip's
codes, poses and log-probabilities are a pure function of the clip's own inputs — alone or among neighbours with other G, eager or
replayed; given the head of an earlier decode the pass returns that decode; the produced rows are those of the existing prefix path.
Every check is EQUALITY.  The PixelCNN is the small network of the quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped
wrapper.  Every test fails on a build without the feature: the keyword and the entries do not exist there.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

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


def same(a, b):
    return all(np.array_equal(_np(x), _np(y)) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def pix():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], 4, True, True).cuda()
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
def decodes(w, clips):
    """The existing path's decodes D of the six clips, computed once: Philox with per-clip records, and greedy."""
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    kws = {"philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50, sampling=recs), "greedy": dict(mode=_lib.TS_SAMPLE_GREEDY)}
    return {k: (kw, [tuple(_np(t) for t in r) for r in w.generate_clips(mf, ids, logprobs=True, **kw)]) for k, kw in kws.items()}


@pytest.fixture(scope="module")
def grid():
    """B = 4, H = 10 (the 8-row chunk boundary is crossed): audio rows, labels, uniforms."""
    B, H = 4, 10
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(synth.speaker_ids(B)).cuda()
    u = rng.random((B, H, 2)).astype(F32)
    return B, H, aud, label, u


# ---- 1. resume ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["philox", "greedy"])
def test_resume_returns_the_decode(w, clips, decodes, how):
    rows, G, mf, ids, recs = clips
    kw, D = decodes[how]
    given = [D[b][0][:G[b]].copy() for b in range(len(rows))]
    res = w.generate_clips(mf, ids, logprobs=True, given=given, **kw)
    for b in range(len(rows)):
        c, p, lp = (_np(t) for t in res[b])
        assert c.shape == (rows[b], 2) and lp.shape == (rows[b], 2)
        assert np.array_equal(c, D[b][0]), f"{how}: codes of clip {b} (G = {G[b]} of {rows[b]} rows)"
        assert np.array_equal(p, D[b][1]), f"{how}: poses of clip {b} (G = {G[b]} of {rows[b]} rows)"
        assert np.array_equal(lp.view(np.uint32), D[b][2].view(np.uint32)), f"{how}: log-probabilities of clip {b} (G = {G[b]} of {rows[b]} rows)"
    # the stacked form and generate_batch's block form: padding as in every mixed pass
    codes, poses, lp = w.generate_clips(mf, ids, logprobs=True, given=given, _stacked=True, **kw)
    for b in range(len(rows)):
        assert np.all(_np(codes)[b, rows[b]:] == -1) and np.all(_np(lp)[b, rows[b]:] == 0.0) and np.all(_np(poses)[b, 4 * rows[b]:] == 0.0)
        assert np.array_equal(_np(codes)[b, :rows[b]], D[b][0])


# ---- 2. against the existing prefix path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["philox", "uniforms", "greedy"])
def test_produced_rows_equal_the_prefix_path(pix, grid, how):
    from talkshow_amd import _lib
    B, H, aud, label, u = grid
    G = [0, 3, 8, 9]
    rng = np.random.default_rng(77)
    given = [rng.integers(0, V, (g, 2)) for g in G]            # random codes, not the decode's own
    kw = {"philox": dict(mode=_lib.TS_SAMPLE_PHILOX, seed=31), "uniforms": dict(mode=_lib.TS_SAMPLE_UNIFORMS), "greedy": dict(mode=_lib.TS_SAMPLE_GREEDY)}[how]
    codes, none, lp = pix.run(label, aud, clip_index0=4, given=given, logprobs=True, uniforms=u if how == "uniforms" else None, **kw)
    assert none is None
    codes, lp = _np(codes), _np(lp)
    for b in range(B):
        g = G[b]
        assert np.array_equal(codes[b, :g], given[b])
        ub = None if how != "uniforms" else np.ascontiguousarray(u[b:b + 1, g:])
        pre = dict(pre_codes=torch.from_numpy(given[b][None]).cuda(), pre_aud=aud[b:b + 1, :g].contiguous()) if g else {}
        c1, _, lp1 = pix.run(label[b:b + 1], aud[b:b + 1, g:].contiguous(), clip_index0=4 + b, uniforms=ub, logprobs=True, **pre, **kw)
        assert np.array_equal(codes[b, g:], _np(c1)[0]), f"{how}: produced rows of clip {b} behind {g} given rows differ from the prefix path"
        assert np.array_equal(lp[b, g:].view(np.uint32), _np(lp1)[0].view(np.uint32)), f"{how}: log-probabilities of the produced rows of clip {b}"
    slp, _ = pix.score(label, aud, torch.from_numpy(codes).cuda())
    slp = _np(slp)
    for b in range(B):                                          # a given row: the teacher-forced value of its code, bit for bit
        assert np.array_equal(lp[b, :G[b]].view(np.uint32), slp[b, :G[b]].view(np.uint32)), f"{how}: given rows of clip {b}"


# ---- 3. neighbours ----------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_neighbours(w, clips):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    n = len(rows)
    rng = np.random.default_rng(5)
    given = [rng.integers(0, V, (G[b], 2)) for b in range(n)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123)
    res = w.generate_clips(mf, ids, sampling=recs, clip_index0=50, logprobs=True, given=given, **kw)
    for b in range(n):
        alone = w.generate_clips([mf[b]], ids[b:b + 1], sampling=[recs[b]], clip_indices=[50 + b], logprobs=True, given=[given[b]], **kw)[0]
        assert same(res[b], alone), f"clip {b} ({rows[b]} rows, G = {G[b]}) differs from the clip alone"
        assert np.array_equal(_np(res[b][0])[:G[b]], given[b])
    # one clip changes its G and its codes: the five others keep their bits
    k = rows.index(20)
    g2 = list(given)
    g2[k] = rng.integers(0, V, (13, 2))
    res2 = w.generate_clips(mf, ids, sampling=recs, clip_index0=50, logprobs=True, given=g2, **kw)
    for b in range(n):
        if b != k:
            assert same(res[b], res2[b]), f"clip {b} changed when clip {k} changed its given rows"
    assert np.array_equal(_np(res2[k][0])[:13], g2[k]) and not np.array_equal(_np(res2[k][0]), _np(res[k][0]))
    # a removed code under top_k = 1 is -inf, a kept one 0
    t = recs.index((1.0, 1.0, 1))
    lp_t = _np(res[t][2])
    assert np.all((lp_t == 0.0) | np.isneginf(lp_t)) and np.isneginf(lp_t[:G[t]]).any() and np.all(lp_t[G[t]:] == 0.0)


# ---- 4. G = 0 and given=None ---------------------------------------------------------------------------------------------------------------
def test_no_given_rows_is_the_plain_pass(w, pix, clips):
    from talkshow_amd import _lib
    rows, G, mf, ids, recs = clips
    n = len(rows)
    for kw in (dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3), dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, sampling=recs, logprobs=True),
               dict(mode=_lib.TS_SAMPLE_GREEDY, logprobs=True)):
        plain = w.generate_clips(mf, ids, **kw)
        caps = pix.graph_captures()
        again = w.generate_clips(mf, ids, **kw)
        assert pix.graph_captures() == caps                    # the plain pass is warm
        none = w.generate_clips(mf, ids, given=None, **kw)
        assert pix.graph_captures() == caps                    # given=None captures nothing the plain pass had not
        zero = w.generate_clips(mf, ids, given=[None] * n, **kw)
        empty = w.generate_clips(mf, ids, given=[np.zeros((0, 2), np.int64)] * n, **kw)
        for b in range(n):
            assert same(plain[b], again[b]) and same(plain[b], none[b]) and same(plain[b], zero[b]) and same(plain[b], empty[b])
    caps = pix.graph_captures()
    w.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_GREEDY, logprobs=True)
    assert pix.graph_captures() == caps                        # and the plain pass still finds its own


# ---- 5. repeats and queueing ---------------------------------------------------------------------------------------------------------------
def _c_pass(pix, label, aud, lens, mode, u, seed, table, block, codes, lp):
    """`ts_pixelcnn_generate_mixed_given` itself, on caller-owned host tables."""
    from talkshow_amd import _lib
    B, H = aud.shape[0], aud.shape[1]
    lens_dev = torch.from_numpy(lens).cuda()
    ci = torch.arange(B, dtype=torch.int64, device="cuda") + 7
    _lib.check(_lib.load().ts_pixelcnn_generate_mixed_given(
        pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, H, mode, _lib.dptr(u), seed,
        _lib.dptr(ci), _lib.dptr(codes), None, 0, _lib.dptr(lp), _lib.dptr(block), table.ctypes.data_as(I32P), None, _lib.stream_ptr()))


def test_repeated_and_queued_passes(pix, grid):
    from talkshow_amd import _lib
    B, H, aud, label, _ = grid
    rng = np.random.default_rng(12)
    tables = [[0, 3, 8, 9], [10, 0, 1, 5], [2, 2, 2, 2]]
    blocks = [torch.from_numpy(rng.integers(0, V, (B, H, 2))).cuda() for _ in tables]
    lens = np.full(B, 4 * H, np.int32)
    mode = _lib.TS_SAMPLE_PHILOX
    alone = []
    for t, blk in zip(tables, blocks):
        codes = torch.full((B, H, 2), -5, dtype=torch.int64, device="cuda")
        lp = torch.full((B, H, 2), 3.0, dtype=torch.float32, device="cuda")
        _c_pass(pix, label, aud, lens.copy(), mode, None, 41, np.asarray(t, np.int32), blk, codes, lp)
        torch.cuda.synchronize()
        alone.append((_np(codes), _np(lp)))
        if len(alone) == 1:
            caps = pix.graph_captures()                        # the first pass captured what the shape needs
    assert pix.graph_captures() == caps                        # repeated passes with other tables capture nothing
    for (c, _), t, blk in zip(alone, tables, blocks):
        for b in range(B):
            assert np.array_equal(c[b, :t[b]], _np(blk)[b, :t[b]])
    assert not np.array_equal(alone[0][0], alone[1][0])
    # three calls queued back to back, the host tables overwritten as soon as each call returns
    table, lens_q = np.zeros(B, np.int32), lens.copy()
    outs = []
    for t, blk in zip(tables, blocks):
        codes = torch.full((B, H, 2), -5, dtype=torch.int64, device="cuda")
        lp = torch.full((B, H, 2), 3.0, dtype=torch.float32, device="cuda")
        table[:] = t
        lens_q[:] = lens
        _c_pass(pix, label, aud, lens_q, mode, None, 41, table, blk, codes, lp)
        table[:] = 2 ** 30
        lens_q[:] = -1
        outs.append((codes, lp))
    torch.cuda.synchronize()
    assert pix.graph_captures() == caps
    for (c, lp), (ac, alp) in zip(outs, alone):
        assert np.array_equal(_np(c), ac) and np.array_equal(_np(lp).view(np.uint32), alp.view(np.uint32))


# ---- 6. what is not read, what is written ---------------------------------------------------------------------------------------------------
def test_unread_inputs_and_red_zones(pix, grid):
    from talkshow_amd import _lib
    B, H, aud, label, u = grid
    hrows, G = [10, 9, 5, 2], [3, 9, 0, 2]
    lens = np.asarray([4 * h + 1 for h in hrows], np.int32)
    rng = np.random.default_rng(8)
    clean = rng.integers(0, V, (B, H, 2))
    dirty = clean.copy()
    u_dirty = u.copy()
    for b in range(B):
        clean[b, G[b]:] = 0
        dirty[b, G[b]::2], dirty[b, G[b] + 1::2] = 2 ** 40, -7
        u_dirty[b, :G[b]] = np.nan
    table = np.asarray(G, np.int32)
    ZC, ZF = 4096 // 8, 4096 // 4                              # 4 KiB of sentinel on either side of each output
    n = B * H * 2

    def run(block, uu):
        cbuf = torch.full((n + 2 * ZC,), -12345, dtype=torch.int64, device="cuda")
        fbuf = torch.full((n + 2 * ZF,), 777.0, dtype=torch.float32, device="cuda")
        codes, lp = cbuf[ZC:ZC + n].view(B, H, 2), fbuf[ZF:ZF + n].view(B, H, 2)
        _c_pass(pix, label, aud, lens, _lib.TS_SAMPLE_UNIFORMS, torch.from_numpy(np.ascontiguousarray(uu)).cuda(), 0, table,
                torch.from_numpy(block).cuda(), codes, lp)
        torch.cuda.synchronize()
        ch, fh = _np(cbuf), _np(fbuf)
        assert (ch[:ZC] == -12345).all() and (ch[ZC + n:] == -12345).all() and (fh[:ZF] == 777.0).all() and (fh[ZF + n:] == 777.0).all()
        c, f = ch[ZC:ZC + n].reshape(B, H, 2), fh[ZF:ZF + n].reshape(B, H, 2)
        assert (c != -12345).all() and (f != 777.0).all()      # every documented element is written
        for b in range(B):
            assert (c[b, hrows[b]:] == -1).all() and (f[b, hrows[b]:] == 0.0).all() and (c[b, :hrows[b]] >= 0).all()
            assert np.array_equal(c[b, :G[b]], block[b, :G[b]]) and np.isfinite(f[b, :hrows[b]]).all()
        return c, f
    c0, f0 = run(clean, u)
    c1, f1 = run(dirty, u_dirty)
    assert np.array_equal(c0, c1) and np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    # a bad table is refused before anything is launched: nothing is written
    codes = torch.full((B, H, 2), -5, dtype=torch.int64, device="cuda")
    lp = torch.full((B, H, 2), 3.0, dtype=torch.float32, device="cuda")
    caps = pix.graph_captures()
    for bad, who in (([3, 10, 0, 2], "clip 1"), ([3, 9, -1, 2], "clip 2")):
        with pytest.raises(RuntimeError, match=who):
            _c_pass(pix, label, aud, lens, _lib.TS_SAMPLE_GREEDY, None, 0, np.asarray(bad, np.int32), torch.from_numpy(clean).cuda(), codes, lp)
    torch.cuda.synchronize()
    assert (_np(codes) == -5).all() and (_np(lp) == 3.0).all() and pix.graph_captures() == caps
    # and the Python layer refuses a bad code, a bad shape and too many rows on the host, naming the clip
    with pytest.raises(ValueError, match="clip 2 hold the code 256"):
        pix.run(label, aud, given=[None, None, np.asarray([[0, 256]]), None])
    with pytest.raises(ValueError, match="clip 1 brings 11 given rows"):
        pix.run(label, aud, given=[None, np.zeros((11, 2), np.int64), None, None])
    with pytest.raises(ValueError, match="no logits output"):
        pix.run(label, aud, given=[None] * 4, want_logits=True)


# ---- 7. the entries that start from recordings --------------------------------------------------------------------------------------------
def test_wav_entries(w):
    import argparse
    import json

    import nets
    from talkshow_amd import _lib, parallel
    from talkshow_amd.config import Object
    from talkshow_amd.frontend import device_mfcc, mixed_tables
    from talkshow_amd.modules import resample_kaiser_device  # noqa: F401  (the 16 kHz route needs none)
    from talkshow_amd.pose_index import assemble_full
    ns = [5872, 16000, 1602, 8001]
    wavs = [synth.wav16(11000 + k, 1, int(n))[0] for k, n in enumerate(ns)]
    ids = (np.arange(len(ns)) % 4).astype(np.int64)
    rows = [int(r) for r in mixed_tables(ns, 16000)["code_rows"]]
    rng = np.random.default_rng(2)
    G = [min(3, rows[0]), 0, rows[2], 1]
    given = [rng.integers(0, V, (g, 2)) if g else None for g in G]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=100)
    mf = [device_mfcc(16000)(x)[0] for x in wavs]
    want = w.generate_clips(mf, ids, given=given, **kw)
    got = w.generate_clips_from_wav(wavs, 16000, ids, given=given, **kw)
    for b in range(len(ns)):
        assert same(got[b], want[b]), f"generate_clips_from_wav: clip {b} ({ns[b]} samples, G = {G[b]})"
        assert np.array_equal(_np(got[b][0])[:G[b]], given[b] if G[b] else np.zeros((0, 2), np.int64))
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=77, clip_index0=100, given=given)
    fid = np.zeros((1, 4), np.float32)
    for b in range(len(ns)):
        f = face.generator.run_clips([wavs[b]], fid)[0]
        ref = _np(assemble_full(want[b][1][None], f[None]))[0]
        assert np.array_equal(_np(out[b]), ref), f"whole_body_clips: recording {b} ({ns[b]} samples, G = {G[b]})"
