"""Memory-safety witnesses for the entries of "repetition penalty" (include/talkshow_hip.h), in the style of tests/test_gpu_bias_canary.py:
every device input sits between red zones, every OUTPUT — `ring_out_dev` of the operator included — between red zones pre-filled (zones
and body) with a sentinel; after the call the zones are intact, the inputs are unmodified, every documented element has lost the sentinel,
and the outputs equal the same call on plain, tightly allocated tensors bit for bit.  The records (host memory) hold window 0, small
windows and the full 64 rows; the passes run with and without bias tables.  Shapes: B in {1, 33}, T_max in {31, 78} (odd), ragged
lengths.  Small networks (hid 128, 256 codes).
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
KINDS = [(0, 9.0, 9.0), (64, 1e30, 0.0), (3, 0.7, 0.3), (64, -0.5, 0.1), (1, 2.0, 0.0)]


def _records(_lib, B, seed):
    rng = np.random.default_rng(seed)
    recs = [KINDS[int(k)] for k in rng.integers(0, len(KINDS), B)]
    recs[0] = KINDS[1]
    if B > 1:
        recs[1], recs[B - 1] = KINDS[0], KINDS[3]
    arr = (_lib.TsRepeat * B)()
    for b, (w, p, f) in enumerate(recs):
        arr[b].window, arr[b].presence, arr[b].frequency, arr[b].reserved = w, p, f, 0
    return recs, arr


def _case(B, T_max, seed):
    rng = np.random.default_rng(seed)
    lens = np.sort(_ragged(B, T_max, seed))[::-1].copy()
    H = T_max // 4
    NB = min(B, 2)
    tabs = rng.standard_normal((NB, 2, V)).astype(np.float32)
    tabs[NB - 1, :, V // 2:] = -np.inf
    index = rng.integers(-1, NB, B).astype(np.int32)
    index[0] = NB - 1
    u = rng.random((B, H, 2)).astype(np.float32)
    return lens, tabs, index, u


def _check(r, lens, recs, B, H, first=None):
    codes = r["codes"].reshape(B, H, 2)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        h = lens[b] // 4
        g = 0 if first is None else int(first[b])
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V))
        assert np.all(lp[b, h:] == 0) and np.isfinite(lp[b, g:h]).all()
        if recs[b] == KINDS[1]:                       # "no repeat within 64 rows" among the produced rows (u < 1 - 2^-24 here)
            for j in range(2):
                col = codes[b, g:h, j].tolist()
                assert len(set(col)) == len(col), f"clip {b} column {j} repeats a code under presence = 1e30"
    if "poses" in r:
        poses = r["poses"].view(np.float32).reshape(B, 4 * H, 129)
        for b in range(B):
            assert np.all(poses[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(poses[b, :4 * (lens[b] // 4)]).all()


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_chain_and_body_entries(nets, B, T_max, tables):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, tabs, index, u = _case(B, T_max, 5 * B + T_max)
    NB = tabs.shape[0]
    recs, arr = _records(_lib, B, B + T_max)
    aud = np.random.default_rng(B + T_max).standard_normal((B, H, 256)).astype(np.float32)
    ids = (np.arange(B) % 4).astype(np.int64)
    common = {"lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "ids": (ids, torch.int64), "u": (u, torch.float32)}
    if tables:
        common["bias"] = (tabs, torch.float32)

    def bias_args(p):
        return (p["bias"], NB, index.ctypes.data_as(I32P)) if tables else (None, 0, None)

    def chain(p):
        _lib.check(lib.ts_pixelcnn_generate_mixed_repeat(px.handle(), p["ids"], p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H,
                                                         _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], None, None, None,
                                                         None, None, 0, *bias_args(p), arr, B, _lib.stream_ptr()))
    r = run_both(chain, dict(common, aud=(aud, torch.float32)), {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32)})
    _check(r, lens, recs, B, H)

    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan

    def body(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_repeat(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"], lens.ctypes.data_as(I32P),
                                                        p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], p["poses"], None,
                                                        0, p["lp"], None, None, None, None, None, 0, *bias_args(p), arr, B, _lib.stream_ptr()))
    r2 = run_both(body, dict(common, mfcc=(mf, torch.float32)),
                  {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r2, lens, recs, B, H)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    H = T_max // 4
    lens, tabs, index, u = _case(B, T_max, 9 * B + T_max)
    recs, arr = _records(_lib, B, 3 * B + T_max)
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
        _lib.check(lib.ts_body_pixel_infer_mixed_poses_repeat(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"],
                                                              lens.ctypes.data_as(I32P), p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0,
                                                              p["clip"], p["codes"], p["poses"], None, 0, p["lp"], p["gp"], P_max,
                                                              plens.ctypes.data_as(I32P), p["plens"], None, None, 0, None, 0, None, arr, B,
                                                              _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    # given rows are taken whatever the records say: the property of the produced rows only
    _check(r, lens, recs, B, H, first=plens // 4)


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("Vop", [2048, 300])
def test_operator(B, Vop, given):
    """`ts_op_sample_repeat` between red zones: the vector path and the generic one, every optional output, the history and the ring
    output; row 70 of column 1 (a wrapped ring)."""
    from talkshow_amd import _lib
    from talkshow_amd import sampling as S
    lib, ctx = _lib.load(), _lib.context(0)
    rng = np.random.default_rng(B + Vop)
    r, column = 70, 1
    logits = rng.standard_normal((B, Vop)).astype(np.float32)
    hist = rng.integers(0, Vop, (B, 64)).astype(np.int32)
    hist[:, ::5] = np.argmax(logits, 1)[:, None]
    recs, arr = _records(_lib, B, B + Vop)
    u = (0.999 * rng.random(B)).astype(np.float32)
    ins = {"logits": (logits, torch.float32), "hist": (hist, torch.int32), "u": (u, torch.float32)}
    G = np.asarray([71 if b % 2 == 0 else 0 for b in range(B)], np.int32)
    codes_in = rng.integers(0, Vop, B).astype(np.int64)
    if given:
        ins["given"] = (codes_in, torch.int64)

    def run(p):
        _lib.check(lib.ts_op_sample_repeat(ctx, p["logits"], B, Vop, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, 0, 2 * r + column, None, 0, p["idx"], p["lp"],
                                           G.ctypes.data_as(I32P) if given else None, None, p["given"] if given else None, None, p["copy"], None, 0,
                                           None, column, arr, B, p["hist"], p["ring"], None))
    out = run_both(run, ins, {"idx": ((B,), torch.int64), "lp": ((B,), torch.float32), "copy": ((B, Vop), torch.float32),
                              "ring": ((B, 64), torch.int32)})
    assert np.array_equal(out["copy"].view(np.float32).reshape(B, Vop).view(np.uint32), logits.view(np.uint32))
    forced = [bool(given and G[b] > 0) for b in range(B)]
    ti, _, _, tring = S.sample_repeat(logits, u, None, recs, hist, 2 * r + column, column=column, given=codes_in, forced=forced)
    assert np.array_equal(out["idx"], ti) and np.array_equal(out["ring"].reshape(B, 64), tring)
