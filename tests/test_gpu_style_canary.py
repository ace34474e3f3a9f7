"""Memory-safety witnesses for the three pass entries of "speaker style" (include/talkshow_hip.h), in the style of
tests/test_gpu_keep_canary.py: the style block and every other input sit between red zones, every OUTPUT sits between red zones
pre-filled (zones and body) with a sentinel; after the call the zones are intact, the inputs are unmodified, every documented element has
lost the sentinel, and the outputs equal the same call on plain, tightly allocated tensors bit for bit.  What the rule says is never read
holds poison: weight rows at or beyond a clip's own code rows (NaN), and the ids, which are NULL.  Both forms (style_rows = 1 and
style_rows = H_max); shapes: B in {1, 33}, T_max in {31, 78}, ragged lengths.  Small networks (hid 128, 256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import _ragged, nets, run_both  # noqa: F401  (nets: the module-scoped fixture of the small networks)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
V, NC = 256, 4


def _case(B, T_max, S, seed):
    """Lengths longest first, a weight block (B, S, NC) with exact zeros, negatives and values above 1, NaN beyond a clip's own rows."""
    rng = np.random.default_rng(seed)
    lens = np.sort(_ragged(B, T_max, seed))[::-1].copy()
    H = T_max // 4
    style = (rng.standard_normal((B, S, NC)) * (rng.random((B, S, NC)) < 0.7)).astype(np.float32)
    style[0, 0] = [0, 0, 1, 0]
    if S > 1:
        for b in range(B):
            style[b, lens[b] // 4:] = np.nan
    u = rng.random((B, H, 2)).astype(np.float32)
    return lens, style, u


def _check(r, lens, B, H):
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h = lens[b] // 4
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V))
        assert np.all(lp[b, h:] == 0) and np.isfinite(lp[b, :h]).all()
    if "poses" in r:
        poses = r["poses"].view(np.float32).reshape(B, 4 * H, 129)
        for b in range(B):
            assert np.all(poses[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(poses[b, :4 * (lens[b] // 4)]).all()


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_chain_and_body_entries(nets, B, T_max, tracked):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    S = H if tracked else 1
    lens, style, u = _case(B, T_max, S, 5 * B + T_max + S)
    aud = np.random.default_rng(B + T_max).standard_normal((B, H, 256)).astype(np.float32)
    common = {"lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "style": (style, torch.float32),
              "u": (u, torch.float32)}

    def chain(p):
        _lib.check(lib.ts_pixelcnn_generate_mixed_style(px.handle(), None, p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H,
                                                        _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], None, None, None,
                                                        None, p["style"], S, _lib.stream_ptr()))
    r = run_both(chain, dict(common, aud=(aud, torch.float32)), {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32)})
    _check(r, lens, B, H)

    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan

    def body(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_style(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], None, lens.ctypes.data_as(I32P),
                                                       p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], p["poses"], None,
                                                       0, p["lp"], None, None, None, None, p["style"], S, _lib.stream_ptr()))
    r2 = run_both(body, dict(common, mfcc=(mf, torch.float32)),
                  {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r2, lens, B, H)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, style, u = _case(B, T_max, H, 9 * B + T_max)
    rng = np.random.default_rng(B * T_max)
    G = np.asarray([int(rng.choice([0, 1, (h + 1) // 2, h])) for h in lens // 4], np.int32)
    plens = np.asarray([0 if g == 0 else 4 * g + (b % 4) for b, g in enumerate(G)], np.int32)
    plens[0] = 4 * (lens[0] // 4)
    P_max = int(plens.max())
    gp = synth.gt_poses(60 + B, B, P_max)
    for b in range(B):
        gp[b, plens[b]:] = np.nan
    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan
    ins = {"mfcc": (mf, torch.float32), "lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64),
           "gp": (gp, torch.float32), "plens": (plens, torch.int32), "style": (style, torch.float32), "u": (u, torch.float32)}

    def run(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_poses_style(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], None,
                                                             lens.ctypes.data_as(I32P), p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"],
                                                             p["codes"], p["poses"], None, 0, p["lp"], p["gp"], P_max, plens.ctypes.data_as(I32P),
                                                             p["plens"], None, p["style"], H, _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r, lens, B, H)
