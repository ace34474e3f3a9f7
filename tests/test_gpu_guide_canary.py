"""Memory-safety witnesses for the three pass entries of "guidance" (include/talkshow_hip.h), in the style of tests/test_gpu_bias_canary.py:
every input sits between red zones of NaN, every OUTPUT between red zones pre-filled (zones and body) with a sentinel; after the call the
zones are intact, the inputs are unmodified, every documented element has lost the sentinel — the shadows' rows included, which their
primaries' workgroups write — and the outputs equal the same call on plain, tightly allocated tensors bit for bit.  Shapes: 2 slots (one
pair) and 33 slots with ragged lengths: pairs next to each other, one with a slot of the same length between, one with the shadow BELOW
its primary, one of the shortest clips.  T_max in {31, 78} (odd).  Small networks (hid 128, 256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import _ragged, nets, run_both  # noqa: F401  (nets: the module-scoped fixture of the small networks)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
FP = C.POINTER(C.c_float)
V = 256


def _case(B, T_max, seed):
    """Lengths longest first with the pairs' lengths made equal; the guide table and its scales; uniforms."""
    rng = np.random.default_rng(seed)
    lens = np.sort(_ragged(B, T_max, seed))[::-1].copy()
    guide, scale = np.full(B, -1, np.int32), np.zeros(B, np.float32)
    pairs = [(0, 1)] if B == 2 else [(0, 1), (5, 7), (21, 20), (10, 11), (32, 31)]
    for k, (p, g) in enumerate(pairs):
        lo, hi = min(p, g), max(p, g)
        lens[lo:hi + 1] = lens[lo]                     # non-increasing stays non-increasing
        guide[p], scale[p] = g, (2.0, -0.5, 7.5, -1.0, 1e4)[k]
    assert np.all(np.diff(lens) <= 0)
    u = rng.random((B, T_max // 4, 2)).astype(np.float32)
    return lens, guide, scale, u, pairs


def _check(r, lens, pairs, B, H):
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h = lens[b] // 4
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V)), f"slot {b}"
        assert np.all(lp[b, h:] == 0) and np.isfinite(lp[b, :h]).all(), f"slot {b}"
    for p, g in pairs:
        assert np.array_equal(codes[g], codes[p]) and np.array_equal(r["lp"].reshape(B, H, 2)[g], r["lp"].reshape(B, H, 2)[p]), f"shadow {g} of {p}"
    if "poses" in r:
        pb = r["poses"].reshape(B, 4 * H, 129)
        poses = r["poses"].view(np.float32).reshape(B, 4 * H, 129)
        for b in range(B):
            assert np.all(poses[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(poses[b, :4 * (lens[b] // 4)]).all()
        for p, g in pairs:
            assert np.array_equal(pb[g], pb[p]), f"poses of shadow {g} are not its primary's"


@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_chain_and_body_entries(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, guide, scale, u, pairs = _case(B, T_max, 5 * B + T_max)
    aud = np.random.default_rng(B + T_max).standard_normal((B, H, 256)).astype(np.float32)
    ids = (np.arange(B) % 4).astype(np.int64)
    common = {"lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "ids": (ids, torch.int64), "u": (u, torch.float32)}
    tail = (guide.ctypes.data_as(I32P), scale.ctypes.data_as(FP))

    def chain(p):
        _lib.check(lib.ts_pixelcnn_generate_guided(px.handle(), p["ids"], p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H,
                                                        _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], None, None, None,
                                                        None, None, 0, None, 0, None, None, 0, *tail, _lib.stream_ptr()))
    r = run_both(chain, dict(common, aud=(aud, torch.float32)), {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32)})
    _check(r, lens, pairs, B, H)

    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan

    def body(p):
        _lib.check(lib.ts_body_pixel_infer_guided(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"], lens.ctypes.data_as(I32P),
                                                       p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], p["poses"], None,
                                                       0, p["lp"], None, None, None, None, None, 0, None, 0, None, None, 0, *tail, _lib.stream_ptr()))
    r2 = run_both(body, dict(common, mfcc=(mf, torch.float32)),
                  {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r2, lens, pairs, B, H)


@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    """Given poses on primaries, plain slots and (never read) on shadows: a shadow's rows are its primary's, the encoders' rows included."""
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, guide, scale, u, pairs = _case(B, T_max, 9 * B + T_max)
    rng = np.random.default_rng(B * T_max)
    G = np.asarray([int(rng.choice([0, 1, (h + 1) // 2])) for h in lens // 4], np.int32)
    plens = np.asarray([0 if g == 0 else 4 * g + (b % 4) for b, g in enumerate(G)], np.int32)
    plens[0] = 4 * ((lens[0] // 4 + 1) // 2)
    P_max = int(plens.max())
    gp = synth.gt_poses(60 + B, B, P_max)
    for b in range(B):
        gp[b, plens[b]:] = np.nan
    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan
    ids = (np.arange(B) % 4).astype(np.int64)
    ins = {"mfcc": (mf, torch.float32), "lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "ids": (ids, torch.int64),
           "gp": (gp, torch.float32), "plens": (plens, torch.int32), "u": (u, torch.float32)}

    def run(p):
        _lib.check(lib.ts_body_pixel_infer_guided_poses(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"],
                                                             lens.ctypes.data_as(I32P), p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"],
                                                             p["codes"], p["poses"], None, 0, p["lp"], p["gp"], P_max, plens.ctypes.data_as(I32P),
                                                             p["plens"], None, None, 0, None, 0, None, None, 0, guide.ctypes.data_as(I32P),
                                                             scale.ctypes.data_as(FP), _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h = lens[b] // 4
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V)) and np.all(lp[b, h:] == 0)
        assert not np.isnan(lp[b, :h]).any()
    for p, g in pairs:
        assert np.array_equal(codes[g], codes[p]) and np.array_equal(r["lp"].reshape(B, H, 2)[g], r["lp"].reshape(B, H, 2)[p])
        assert np.array_equal(r["poses"].reshape(B, 4 * H, 129)[g], r["poses"].reshape(B, 4 * H, 129)[p])
