"""Mixed passes: clips of DIFFERENT lengths in one body pass (`ts_body_pixel_infer_mixed`, `TrainWrapper.generate_clips`,
`generate_batches` with unequal T).

The contract under test is the project's central one extended to the length mix: a clip's bits do not depend on what it shares a
pass with.  So the bar of every comparison with the clip run alone is EQUALITY (codes `array_equal`, poses `array_equal`), and the
bar against the reference's goldens is the suite's existing one (all greedy codes equal, poses within 1e-4) — nothing here
introduces a tolerance.  Every test fails on a build without the feature: the entry points do not exist there and
`generate_batches` raises on unequal T.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from talkshow_amd import synth
from test_gpu_canary import F32, I64, run_both

pytestmark = pytest.mark.gpu

# 42 clips: T % 4 in {0, 1, 2, 3}; clips shorter than one 8-row chunk (T < 32); clips that end inside a chunk; 30 distinct lengths; the three
# recordings' lengths (75 / 96 / 72 code rows are 300 / 384 / 288 MFCC rows: here their quarter-size cousins keep the solo runs short)
LENS = [131, 130, 129, 128, 96, 96, 75, 75, 75, 72, 72, 61, 50, 50, 47, 47, 46, 45, 44, 33, 33, 33, 31, 30, 29, 28, 27, 26, 21, 17, 16, 15,
        13, 12, 9, 8, 7, 6, 5, 4, 128, 75]
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def w():
    import bench
    return bench.build_models(0, seed=7)[0]          # the weights every reference golden was made with


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _clips(seed, lens):
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(lens))               # submission order is NOT sorted: the Python layer sorts and un-sorts
    lens = [int(lens[i]) for i in order]
    clips = [synth.mfcc_features(seed * 1000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(lens)) % 4).astype(np.int64)
    return lens, clips, ids


def _sorted_pass(lens, clips, ids, fill=0.0):
    """The C entry's inputs: clips by non-increasing length, padded to the longest with `fill`."""
    from nets.smplx_body_pixel import mixed_pass_order
    order, _ = mixed_pass_order(lens)
    T_max = lens[order[0]]
    mf = np.full((len(lens), T_max, 64), fill, np.float32)
    for k, i in enumerate(order):
        mf[k, :lens[i]] = clips[i]
    return order, mf, np.asarray([lens[i] for i in order], np.int32), ids[order]


def test_reference_parity_on_recordings_in_one_pass(golden, w):
    """The three recordings x four speaker ids = 12 clips of three lengths in ONE mixed pass: greedy codes equal to the reference
    golden 1 944 / 1 944, poses within the suite's 1e-4 of the golden."""
    from talkshow_amd import _lib
    g = golden("real_audio_body")
    tags = ("style", "1st_page", "french")
    clips, ids, who = [], [], []
    for spk in range(4):                             # interleaved: no two neighbours have one length
        for t in tags:
            clips.append(g[t + "_rows"])
            ids.append(spk)
            who.append((t, spk))
    assert len({c.shape[0] for c in clips}) == 3
    res = w.generate_clips(clips, np.asarray(ids, np.int64), mode=_lib.TS_SAMPLE_GREEDY)
    equal = total = 0
    for (t, spk), (codes, poses) in zip(who, res):
        ref = g[t + "_codes"].astype(np.int64)[spk]
        assert codes.shape == ref.shape
        equal += int((codes.cpu().numpy() == ref).sum())
        total += ref.size
        if spk == int(g[t + "_pose_id"]):
            assert_close_measured(f"mixed_pass.{t}.poses", poses.cpu().numpy(), g[t + "_poses"], 1e-4)
    print(f"\nmixed pass on the recordings: greedy codes equal to the reference {equal} / {total}")
    assert total == 1944 and equal == total


@pytest.mark.parametrize("mode_name", ["greedy", "uniforms", "philox"])
def test_bit_identity_with_the_clip_alone(w, mode_name):
    """42 clips of 30 lengths in one pass against each clip through `generate_batch` at B = 1: codes equal, poses array_equal."""
    from talkshow_amd import _lib
    mode = {"greedy": _lib.TS_SAMPLE_GREEDY, "uniforms": _lib.TS_SAMPLE_UNIFORMS, "philox": _lib.TS_SAMPLE_PHILOX}[mode_name]
    lens, clips, ids = _clips(11, LENS)
    assert len(lens) >= 40 and len(set(lens)) >= 6 and {t % 4 for t in lens} == {0, 1, 2, 3} and min(lens) // 4 < 8
    rng = np.random.default_rng(5)
    u = [rng.random((t // 4, 2)).astype(np.float32) for t in lens] if mode == _lib.TS_SAMPLE_UNIFORMS else None
    res = w.generate_clips(clips, ids, mode=mode, uniforms=u, seed=1234, clip_index0=100)
    for b, (codes, poses) in enumerate(res):
        sc, sp = w.generate_batch(clips[b][None], ids[b:b + 1], mode=mode, uniforms=None if u is None else u[b][None], seed=1234,
                                  clip_index0=100 + b)
        assert codes.shape == (lens[b] // 4, 2) and poses.shape == (4 * (lens[b] // 4), 129)
        assert np.array_equal(codes.cpu().numpy(), sc.cpu().numpy()[0]), f"{mode_name}: codes of clip {b} (T = {lens[b]}) differ from the clip alone"
        assert np.array_equal(poses.cpu().numpy(), sp.cpu().numpy()[0]), f"{mode_name}: poses of clip {b} (T = {lens[b]}) differ from the clip alone"
    if mode != _lib.TS_SAMPLE_GREEDY:                # they are draws
        gr = w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_GREEDY)
        assert any(not np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) for a, b in zip(res, gr))


def test_large_pass_production_plans(w):
    """256 clips of the recordings' lengths and a spread around them in one pass — the shape at which the conv stacks run their production
    plans (the ring engine's dealt and banded launches, paired body + hand layers) and the chain its wide kernel: sampled clips equal the
    clip alone, in greedy and in Philox mode."""
    from talkshow_amd import _lib
    rng = np.random.default_rng(8)
    base = [300, 384, 288, 301, 302, 303, 150, 97, 45, 18]
    lens, clips, ids = _clips(51, [base[i] for i in rng.integers(0, len(base), 256)])
    for mode in (_lib.TS_SAMPLE_GREEDY, _lib.TS_SAMPLE_PHILOX):
        res = w.generate_clips(clips, ids, mode=mode, seed=31, clip_index0=7)
        picked = {}
        for b, t in enumerate(lens):                 # the first and the last clip of every length
            picked.setdefault(t, [b, b])[1] = b
        for b in sorted({x for pair in picked.values() for x in pair}):
            sc, sp = w.generate_batch(clips[b][None], ids[b:b + 1], mode=mode, seed=31, clip_index0=7 + b)
            assert np.array_equal(res[b][0].cpu().numpy(), sc.cpu().numpy()[0]), f"codes of clip {b} (T = {lens[b]})"
            assert np.array_equal(res[b][1].cpu().numpy(), sp.cpu().numpy()[0]), f"poses of clip {b} (T = {lens[b]})"


@pytest.mark.parametrize("knob", ["TS_CONV_RING=0", "TS_CONV_DEAL=0", "TS_CONV_BANDS=0", "TS_CONV_RING_PAIRED=0", "TS_NO_GRAPH=1"])
def test_alternate_engines(knob):
    """The same comparison with the conv layers on the other engines a lever can put them on (conv_gemm.hip's plain and banded grids, the
    ring engine's plain grid) and with eager chain launches; the levers are read once per process -> child process."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, v = knob.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                        "test_large_pass_production_plans or test_padding_contract"], env=dict(os.environ, **{k: v}),
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_stage_entries_bit_identity(hip, w):
    """The length-table forms of the audio encoder and of the paired decoders alone: valid rows equal to the clip alone, rows beyond a
    clip written as zeros; code indices beyond a clip are never read (they hold an index no table has)."""
    _lib, lib, ctx = hip
    lens, clips, ids = _clips(3, [131, 96, 75, 75, 72, 50, 47, 33, 30, 21, 9, 6, 5, 4])
    order, mf, slens, _ = _sorted_pass(lens, clips, ids, fill=np.nan)
    B, T_max = mf.shape[0], mf.shape[1]
    H = T_max // 4
    mfd, ld = torch.from_numpy(mf).cuda(), torch.from_numpy(slens).cuda()
    feat = torch.full((B, H, 256), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.ts_audioenc_forward_masked(w.audioencoder.handle(), _lib.dptr(mfd), _lib.dptr(ld), B, T_max, _lib.dptr(feat), _lib.stream_ptr()))
    rng = np.random.default_rng(9)
    lat = rng.integers(0, 2048, (B, H, 2)).astype(np.int64)
    for k in range(B):
        lat[k, slens[k] // 4:] = 0x7EADBEEF7EADBEEF
    latd = torch.from_numpy(lat).cuda()
    lb, lh = latd[..., 0].contiguous(), latd[..., 1].contiguous()
    out = torch.full((B, 4 * H, 129), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.ts_vqvae_decode_pair_masked(w.g_body.handle(), w.g_hand.handle(), _lib.dptr(lb), _lib.dptr(lh), _lib.dptr(ld), B, H,
                                               _lib.dptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, i in enumerate(order):
        h = lens[i] // 4
        solo = w.audioencoder.forward_nlc(torch.from_numpy(clips[i][None]).cuda())
        assert np.array_equal(feat[k, :h].cpu().numpy(), solo[0].cpu().numpy()), f"audio encoder: clip of T = {lens[i]}"
        assert not feat[k, h:].any()
        dec = w._decode_pair(latd[k:k + 1, :h].contiguous())
        assert np.array_equal(out[k, :4 * h].cpu().numpy(), dec[0].cpu().numpy()), f"decoders: clip of {h} code rows"
        assert not out[k, 4 * h:].any()


def test_order_independence(w):
    """The same clips submitted in two orders, global indices following the clips: the same per-clip results (Philox)."""
    from talkshow_amd import _lib
    lens, clips, ids = _clips(21, [96, 75, 75, 72, 61, 50, 33, 31, 17, 9, 8, 5])
    gidx = [1000 + 7 * b for b in range(len(lens))]
    a = w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_indices=gidx)
    perm = np.random.default_rng(2).permutation(len(lens))
    b = w.generate_clips([clips[i] for i in perm], ids[perm], mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_indices=[gidx[i] for i in perm])
    for k, i in enumerate(perm):
        assert np.array_equal(a[i][0].cpu().numpy(), b[k][0].cpu().numpy()) and np.array_equal(a[i][1].cpu().numpy(), b[k][1].cpu().numpy())
    c = w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_indices=[x + 1 for x in gidx])   # other subsequences: other draws
    assert any(not np.array_equal(x[0].cpu().numpy(), y[0].cpu().numpy()) for x, y in zip(a, c))


@pytest.mark.parametrize("mode_name", ["greedy", "uniforms"])
def test_padding_contract_under_canaries(hip, w, mode_name):
    """Red zones around every buffer, NaN in the input padding beyond T_b: zones intact, every output element written, code rows beyond
    H_b = -1, pose rows beyond 4 H_b = 0, valid rows what the wrapper gives on clean inputs."""
    _lib, lib, ctx = hip
    mode = _lib.TS_SAMPLE_GREEDY if mode_name == "greedy" else _lib.TS_SAMPLE_UNIFORMS
    lens, clips, ids = _clips(31, [78, 75, 72, 50, 47, 33, 31, 30, 9, 7, 4])
    order, mf, slens, sids = _sorted_pass(lens, clips, ids, fill=np.nan)
    B, T_max = mf.shape[0], mf.shape[1]
    H = T_max // 4
    rng = np.random.default_rng(1)
    u = np.full((B, H, 2), np.nan, np.float32)
    ul = [rng.random((t // 4, 2)).astype(np.float32) for t in lens]
    for k, i in enumerate(order):
        u[k, :lens[i] // 4] = ul[i]
    ins = {"mfcc": (mf, F32), "ids": (sids, I64)}
    if mode == _lib.TS_SAMPLE_UNIFORMS:
        ins["u"] = (u, F32)
    ldev = torch.from_numpy(slens).cuda()            # (the int32 table itself: run_both guards float32 / int64 buffers)
    r = run_both(lambda p: _lib.check(lib.ts_body_pixel_infer_mixed(
        w.audioencoder.handle(), w.generator.handle(), w.g_body.handle(), w.g_hand.handle(), p["mfcc"], p["ids"],
        slens.ctypes.data_as(I32P), _lib.dptr(ldev), B, T_max, mode, p.get("u"), 0, None, p["codes"], p["poses"], _lib.stream_ptr())),
        ins, {"codes": ((B, H, 2), I64), "poses": ((B, 4 * H, 129), F32)})
    codes, poses = r["codes"].cpu().numpy(), r["poses"].cpu().numpy()
    clean = w.generate_clips(clips, ids, mode=mode, uniforms=ul if mode == _lib.TS_SAMPLE_UNIFORMS else None)
    for k, i in enumerate(order):
        h = lens[i] // 4
        assert (codes[k, h:] == -1).all() and not poses[k, 4 * h:].any()
        assert ((codes[k, :h] >= 0) & (codes[k, :h] < 2048)).all() and np.isfinite(poses[k, :4 * h]).all()
        assert np.array_equal(codes[k, :h], clean[i][0].cpu().numpy()) and np.array_equal(poses[k, :4 * h], clean[i][1].cpu().numpy())


def _chain_launches(hip, fn):
    _lib, lib, ctx = hip
    ms, n, fl = (C.c_double * 3)(), (C.c_int64 * 3)(), (C.c_double * 3)()
    _lib.check(lib.ts_prof_enable(ctx, 1))
    try:
        _lib.check(lib.ts_prof_read(ctx, ms, n, fl, 1))
        fn()
        torch.cuda.synchronize()
        _lib.check(lib.ts_prof_read(ctx, ms, n, fl, 1))
    finally:
        _lib.check(lib.ts_prof_enable(ctx, 0))
    return int(n[1])


def test_launch_plan(hip, w):
    """Chain launches of a mixed pass = those of a uniform pass of H_max rows (the chunk rounding carries a clip to the end of its
    8-row chunk: more rows per launch, never more launches); a repeated pass captures nothing; more distinct lengths than the bound run
    correctly with active counts rounded up, inside the graph budget."""
    _lib, lib, ctx = hip
    lens, clips, ids = _clips(41, [131, 96, 75, 75, 72, 50, 33, 21, 9, 4])
    H_max = max(lens) // 4
    mixed = _chain_launches(hip, lambda: w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_GREEDY))
    uniform = _chain_launches(hip, lambda: w.generate_batch(synth.mfcc_features(1, len(lens), max(lens)), ids, mode=_lib.TS_SAMPLE_GREEDY))
    per_length = sum(_chain_launches(hip, lambda t=t: w.generate_batch(synth.mfcc_features(1, 1, t), ids[:1], mode=_lib.TS_SAMPLE_GREEDY))
                     for t in sorted(set(lens)))
    print(f"\nchain launches: mixed pass {mixed}, uniform pass of {H_max} rows {uniform}, one pass per distinct length {per_length}")
    assert mixed == uniform and mixed < per_length
    s = _lib.stream_ptr()
    first = [(c.cpu().numpy(), p.cpu().numpy()) for c, p in w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=5)]
    cap = lib.ts_pixelcnn_graph_captures(w.generator.handle(), s)
    for _ in range(2):
        again = w.generate_clips(clips, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=5)
        torch.cuda.synchronize()
        assert lib.ts_pixelcnn_graph_captures(w.generator.handle(), s) == cap
        assert all(np.array_equal(a[0], b[0].cpu().numpy()) and np.array_equal(a[1], b[1].cpu().numpy()) for a, b in zip(first, again))
    # 20 clips, each one chunk longer than the next: 20 distinct active counts > the documented 12 -> rounded up to multiples of 2
    many = [4 * (8 * k + 1) for k in range(20)]
    hrows = np.asarray(sorted((t // 4 for t in many), reverse=True), np.int32)
    active = np.zeros((int(hrows[0]) + 7) // 8, np.int32)
    assert lib.ts_debug_mixed_plan(hrows.ctypes.data_as(I32P), len(many), 0, active.ctypes.data_as(I32P)) == 2
    assert len(set(active.tolist())) <= 12
    lens2, clips2, ids2 = _clips(43, many)
    res = w.generate_clips(clips2, ids2, mode=_lib.TS_SAMPLE_GREEDY)
    cap = lib.ts_pixelcnn_graph_captures(w.generator.handle(), s)
    res2 = w.generate_clips(clips2, ids2, mode=_lib.TS_SAMPLE_GREEDY)
    torch.cuda.synchronize()
    assert lib.ts_pixelcnn_graph_captures(w.generator.handle(), s) == cap          # the whole pass fits the chunk-graph budget
    assert lib.ts_debug_pixelcnn_graphs(w.generator.handle(), s) <= 24
    for b in (0, 5, 11, 19):
        sc, sp = w.generate_batch(clips2[b][None], ids2[b:b + 1], mode=_lib.TS_SAMPLE_GREEDY)
        for r in (res, res2):
            assert np.array_equal(r[b][0].cpu().numpy(), sc.cpu().numpy()[0]) and np.array_equal(r[b][1].cpu().numpy(), sp.cpu().numpy()[0])


def test_uniform_path_untouched_and_unequal_batches(w):
    """`generate_batches` with equal T = `generate_batch` on the stacked tensor (the existing guarantee); with unequal T every batch gets
    the bits and the Philox subsequences it gets alone at its place in the list."""
    from talkshow_amd import _lib
    a, b = synth.mfcc_features(1, 3, 60), synth.mfcc_features(2, 2, 60)
    ia, ib = np.asarray([0, 1, 2], np.int64), np.asarray([3, 0], np.int64)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = w.generate_batches([da, db], [ia, ib], mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=40)
    c, p = w.generate_batch(np.concatenate([a, b]), np.concatenate([ia, ib]), mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=40)
    assert np.array_equal(torch.cat([g[0] for g in got]).cpu().numpy(), c.cpu().numpy())
    assert np.array_equal(torch.cat([g[1] for g in got]).cpu().numpy(), p.cpu().numpy())
    b2 = synth.mfcc_features(3, 2, 83)
    got = w.generate_batches([da, torch.from_numpy(b2).cuda()], [ia, ib], mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=40)
    ca, pa = w.generate_batch(a, ia, mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=40)
    cb, pb = w.generate_batch(b2, ib, mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=43)
    assert got[0][0].shape == (3, 15, 2) and got[1][0].shape == (2, 20, 2) and got[1][1].shape == (2, 80, 129)
    assert np.array_equal(got[0][0].cpu().numpy(), ca.cpu().numpy()) and np.array_equal(got[0][1].cpu().numpy(), pa.cpu().numpy())
    assert np.array_equal(got[1][0].cpu().numpy(), cb.cpu().numpy()) and np.array_equal(got[1][1].cpu().numpy(), pb.cpu().numpy())


def test_errors(hip, w):
    """An unsorted table, a length above T_max and T_b < 4 at the C entry: the library's error code and a message; Python: ValueError."""
    _lib, lib, ctx = hip
    B, T_max = 3, 40
    H = T_max // 4
    mf = torch.zeros((B, T_max, 64), dtype=torch.float32, device="cuda")
    ids = torch.zeros((B,), dtype=torch.int64, device="cuda")
    codes = torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")
    poses = torch.zeros((B, 4 * H, 129), dtype=torch.float32, device="cuda")
    for bad, word in (([30, 40, 20], "non-increasing"), ([44, 40, 20], "T_max"), ([40, 20, 3], "shorter")):
        lens = np.asarray(bad, np.int32)
        ld = torch.from_numpy(lens).cuda()
        rc = lib.ts_body_pixel_infer_mixed(w.audioencoder.handle(), w.generator.handle(), w.g_body.handle(), w.g_hand.handle(),
                                           _lib.dptr(mf), _lib.dptr(ids), lens.ctypes.data_as(I32P), _lib.dptr(ld), B, T_max,
                                           _lib.TS_SAMPLE_GREEDY, None, 0, None, _lib.dptr(codes), _lib.dptr(poses), _lib.stream_ptr())
        assert rc != 0 and word in lib.ts_last_error().decode(), (bad, lib.ts_last_error().decode())
    torch.cuda.synchronize()
    assert not codes.any() and not poses.any()       # a rejected call launches nothing
    with pytest.raises(ValueError):
        w.generate_clips([np.zeros((3, 64), np.float32), np.zeros((40, 64), np.float32)], np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        w.generate_clips([np.zeros((40, 32), np.float32)], np.zeros(1, np.int64))
    with pytest.raises(ValueError):
        w.generate_clips([], np.zeros(0, np.int64))
    with pytest.raises(ValueError):
        w.generate_batches([torch.zeros((1, 3, 64), device="cuda"), torch.zeros((1, 40, 64), device="cuda")],
                           [np.zeros(1, np.int64), np.ones(1, np.int64)])
