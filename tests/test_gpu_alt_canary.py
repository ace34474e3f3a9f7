"""Memory-safety witness for `ts_pixelcnn_generate_alt` (include/talkshow_hip.h, "alternatives"), in the style of
tests/test_gpu_poses_canary.py: every device input sits between red zones, every OUTPUT — the four arrays of the record included —
between 4 KiB red zones pre-filled (zones and body) with a sentinel; after the call the zones are intact, the inputs are unmodified, every
documented element has lost the sentinel, and the outputs equal the same call on plain, tightly allocated tensors bit for bit.
B = 33 clips of 3, 2 and 1 code rows, n = 3.  Small networks (256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_poses_canary import nets, run_both  # noqa: F401  (nets: the module-scoped fixture of the small networks)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
V, B, H, N = 256, 33, 3, 3


@pytest.mark.parametrize("given", [False, True])
def test_chain_entry_between_red_zones(nets, given):
    from talkshow_amd import _lib
    lib = _lib.load()
    _, px, _, _ = nets
    rng = np.random.default_rng(33)
    rows = np.array([3] * 11 + [2] * 11 + [1] * 11, np.int32)
    lens = (4 * rows + rng.integers(0, 4, B)).astype(np.int32)
    lens = np.sort(lens)[::-1].copy()
    rows = lens // 4
    aud = rng.standard_normal((B, H, 256)).astype(np.float32)
    ids = (np.arange(B) % 4).astype(np.int64)
    u = rng.random((B, H, 2)).astype(np.float32)
    tabs = rng.standard_normal((1, 2, V)).astype(np.float32)
    tabs[0, 1, 2:] = -np.inf                                  # the hand column of a clip with the table keeps 2 codes: padding for n = 3
    index = np.where(np.arange(B) % 3 == 0, 0, -1).astype(np.int32)
    G = np.where(np.arange(B) % 2 == 0, np.minimum(rows, 1), 0).astype(np.int32)
    gcodes = rng.integers(0, V, (B, H, 2)).astype(np.int64)
    gcodes[0, 0, 0] = V + 5                                   # a given code outside the vocabulary: rank -1, a NaN log-probability
    ins = {"lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64), "ids": (ids, torch.int64), "u": (u, torch.float32),
           "aud": (aud, torch.float32), "bias": (tabs, torch.float32)}
    if given:
        ins["given"] = (gcodes, torch.int64)

    def chain(p):
        rec = _lib.TsAltOut(N, 0, p["acodes"].value, p["alp"].value, p["ent"].value, p["rank"].value)
        _lib.check(lib.ts_pixelcnn_generate_alt(px.handle(), p["ids"], p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H, _lib.TS_SAMPLE_UNIFORMS,
                                                      p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], p["given"] if given else None,
                                                      G.ctypes.data_as(I32P) if given else None, None, None, None, 0, p["bias"], 1,
                                                      index.ctypes.data_as(I32P), None, 0, C.byref(rec), _lib.stream_ptr()))
    r = run_both(chain, ins, {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32), "acodes": ((B, H, 2, N), torch.int32),
                              "alp": ((B, H, 2, N), torch.float32), "ent": ((B, H, 2), torch.float32), "rank": ((B, H, 2), torch.int32)})
    codes = r["codes"].reshape(B, H, 2)
    acodes, alp = r["acodes"].reshape(B, H, 2, N), r["alp"].view(np.float32).reshape(B, H, 2, N)
    ent, rank = r["ent"].view(np.float32).reshape(B, H, 2), r["rank"].reshape(B, H, 2)
    for b in range(B):
        h = int(rows[b])
        assert np.all(acodes[b, h:] == -1) and np.all(alp[b, h:] == 0) and np.all(ent[b, h:] == 0) and np.all(rank[b, h:] == -1)
        assert np.all(codes[b, h:] == -1)
        assert np.all((acodes[b, :h, 0] >= 0) & (acodes[b, :h, 0] < V)) and np.isfinite(alp[b, :h, 0]).all() and np.all(ent[b, :h] >= 0)
        if index[b] == 0:
            assert np.all(acodes[b, :h, 1, 2] == -1) and np.isneginf(alp[b, :h, 1, 2]).all() and set(acodes[b, :h, 1, :2].reshape(-1)) <= {0, 1}
        else:
            assert np.all(acodes[b, :h] >= 0)
        outside = given and b == 0
        assert np.all(rank[b, :h].reshape(-1)[1 if outside else 0:] >= 0)
        if outside:
            assert rank[0, 0, 0] == -1
