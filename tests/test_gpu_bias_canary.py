"""Memory-safety witnesses for the entries of "code bias" (include/talkshow_hip.h), in the style of tests/test_gpu_style_canary.py: the
bias block sits between red zones of NaN and every other input between zones too, every OUTPUT sits between red zones pre-filled (zones
and body) with a sentinel; after the call the zones are intact, the inputs are unmodified, every documented element has lost the sentinel,
and the outputs equal the same call on plain, tightly allocated tensors bit for bit.  The index table holds -1 and the LAST valid table;
the column of a table that is all the rule allows is a ban of most codes, so a read of the wrong row shows in the codes.  Shapes: B in
{1, 33}, T_max in {31, 78} (odd), ragged lengths.  Small networks (hid 128, 256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import _ragged, nets, run_both  # noqa: F401  (nets: the module-scoped fixture of the small networks)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
V = 256


def _case(B, T_max, seed):
    """Lengths longest first; NB = min(B, 3) tables — finite random, an allow-list of 9 codes per column, a ban of the upper half — and an
    index that holds -1 and NB - 1; uniforms."""
    rng = np.random.default_rng(seed)
    lens = np.sort(_ragged(B, T_max, seed))[::-1].copy()
    H = T_max // 4
    NB = min(B, 3)
    tabs = np.zeros((NB, 2, V), np.float32)
    tabs[0] = rng.standard_normal((2, V))
    if NB > 1:
        tabs[1] = -np.inf
        for j in range(2):
            tabs[1, j, rng.choice(V, 9, replace=False)] = 0.0
    tabs[NB - 1, :, V // 2:] = -np.inf
    index = rng.integers(-1, NB, B).astype(np.int32)
    index[0] = NB - 1
    if B > 1:
        index[1], index[B - 1] = -1, NB - 1
    u = rng.random((B, H, 2)).astype(np.float32)
    return lens, tabs, index, u


def _check(r, lens, tabs, index, B, H):
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h = lens[b] // 4
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V))
        assert np.all(lp[b, h:] == 0) and np.isfinite(lp[b, :h]).all()
        if index[b] >= 0:
            for j in range(2):
                assert np.all(tabs[index[b], j][codes[b, :h, j]] != -np.inf), f"clip {b} column {j}: a banned code was drawn"
    if "poses" in r:
        poses = r["poses"].view(np.float32).reshape(B, 4 * H, 129)
        for b in range(B):
            assert np.all(poses[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(poses[b, :4 * (lens[b] // 4)]).all()


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_chain_and_body_entries(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, tabs, index, u = _case(B, T_max, 5 * B + T_max)
    NB = tabs.shape[0]
    aud = np.random.default_rng(B + T_max).standard_normal((B, H, 256)).astype(np.float32)
    ids = (np.arange(B) % 4).astype(np.int64)
    common = {"lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "ids": (ids, torch.int64),
              "bias": (tabs, torch.float32), "u": (u, torch.float32)}

    def chain(p):
        _lib.check(lib.ts_pixelcnn_generate_mixed_bias(px.handle(), p["ids"], p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H,
                                                       _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], None, None, None,
                                                       None, None, 0, p["bias"], NB, index.ctypes.data_as(I32P), _lib.stream_ptr()))
    r = run_both(chain, dict(common, aud=(aud, torch.float32)), {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32)})
    _check(r, lens, tabs, index, B, H)

    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan

    def body(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_bias(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"], lens.ctypes.data_as(I32P),
                                                      p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], p["poses"], None,
                                                      0, p["lp"], None, None, None, None, None, 0, p["bias"], NB, index.ctypes.data_as(I32P),
                                                      _lib.stream_ptr()))
    r2 = run_both(body, dict(common, mfcc=(mf, torch.float32)),
                  {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r2, lens, tabs, index, B, H)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, tabs, index, u = _case(B, T_max, 9 * B + T_max)
    NB = tabs.shape[0]
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
           "gp": (gp, torch.float32), "plens": (plens, torch.int32), "bias": (tabs, torch.float32), "u": (u, torch.float32)}

    def run(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_poses_bias(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"],
                                                            lens.ctypes.data_as(I32P), p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"],
                                                            p["codes"], p["poses"], None, 0, p["lp"], p["gp"], P_max, plens.ctypes.data_as(I32P),
                                                            p["plens"], None, None, 0, p["bias"], NB, index.ctypes.data_as(I32P), _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    # given rows are taken whatever the tables say (a banned one gets -inf): check the produced rows only
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h, g = lens[b] // 4, plens[b] // 4
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V)) and np.all(lp[b, h:] == 0)
        assert not np.isnan(lp[b, :h]).any() and np.isfinite(lp[b, g:h]).all()
        if index[b] >= 0:
            for j in range(2):
                assert np.all(tabs[index[b], j][codes[b, g:h, j]] != -np.inf), f"clip {b} column {j}: a banned code was drawn"


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("Vop", [2048, 300])
def test_operator(B, Vop):
    """`ts_op_sample_bias` between red zones: the vector path and the generic one, every optional output."""
    from talkshow_amd import _lib
    lib, ctx = _lib.load(), _lib.context(0)
    rng = np.random.default_rng(B + Vop)
    NB = min(B, 2)
    logits = rng.standard_normal((B, Vop)).astype(np.float32)
    tabs = rng.standard_normal((NB, 2, Vop)).astype(np.float32)
    tabs[NB - 1, :, Vop // 3:] = -np.inf
    index = rng.integers(-1, NB, B).astype(np.int32)
    index[B - 1] = NB - 1
    if B > 1:
        index[0] = -1
    u = rng.random(B).astype(np.float32)
    ins = {"logits": (logits, torch.float32), "bias": (tabs, torch.float32), "u": (u, torch.float32)}

    def run(p):
        _lib.check(lib.ts_op_sample_bias(ctx, p["logits"], B, Vop, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, 0, 0, None, 0, p["idx"], p["lp"], None, None, None,
                                         None, p["copy"], p["bias"], NB, index.ctypes.data_as(I32P), 1, None))
    r = run_both(run, ins, {"idx": ((B,), torch.int64), "lp": ((B,), torch.float32), "copy": ((B, Vop), torch.float32)})
    assert np.array_equal(r["copy"].view(np.float32).reshape(B, Vop).view(np.uint32), logits.view(np.uint32))
    for b in range(B):
        assert 0 <= r["idx"][b] < Vop and (index[b] < 0 or tabs[index[b], 1, r["idx"][b]] != -np.inf)
