"""The length variants of the face generator's non-GEMM kernels (csrc/face.hip), one by one through their debug entries
(include/talkshow_hip_debug.h), against the EXISTING kernel on the clip alone.

The bar is `array_equal`: a mixed pass promises the bits of the clip alone, so each variant must reproduce the uniform kernel exactly —
its float64 accuracy is then the one tests/test_gpu_face_ops.py pins for the uniform kernels.  Rows at or beyond a clip's length must be
zeros (attention: untouched), and inputs there hold NaNs: a read beyond a clip's end shows in its valid rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_face_ops import ATT_CFG, ATT_T, F32, _run, dev, hip, nans, qkv_case  # noqa: F401  (hip: fixture)

pytestmark = pytest.mark.gpu

I32P = C.POINTER(C.c_int32)


def i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(I32P), dev(a)


def feature_rows(n):
    L = (n - 10) // 5 + 1
    for k in (3, 3, 3, 3, 2, 2):
        L = (L - k) // 2 + 1
    return L


@pytest.mark.parametrize("heads,B", ATT_CFG)
def test_attention_mixed(hip, heads, B):
    """Frame counts drawn from ATT_T mixed in one launch (several launches cover the whole table), NaN in the K / V rows beyond each clip's
    length: every clip's rows equal `ts_debug_attention` on the clip alone; rows beyond are not written."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(100 * heads + B)
    table = [t for t in ATT_T if t <= 300]
    HID = heads * 64
    for rep in range(len(table) // B + 2):
        frames = [table[(rep * B + b) % len(table)] for b in range(B)] if rep else [table[i] for i in rng.permutation(len(table))[:B]]
        if rep == 1 and B == 1:
            frames = [1800]
        T_max = max(frames)
        qkv = np.full((B, T_max, 3 * HID), np.nan, F32)
        for b, t in enumerate(frames):
            qkv[b, :t] = qkv_case("synthetic", 1, t, heads, rng)[0]
            qkv[b, t:, :HID] = 0.0                                  # (queries beyond a clip are rows nobody computes; keep them finite anyway)
        fh, fp, fd = i32(frames)
        out, qd = nans(B, T_max, HID), dev(qkv)
        _run(_lib, lib.ts_debug_attention_mixed(_lib.dptr(qd), fp, _lib.dptr(fd), B, T_max, HID, heads, 0.125, _lib.dptr(out), None))
        out = out.cpu().numpy()
        for b, t in enumerate(frames):
            alone, qa = nans(1, t, HID), dev(qkv[b:b + 1, :t])
            _run(_lib, lib.ts_debug_attention(_lib.dptr(qa), 1, t, HID, heads, 0.125, _lib.dptr(alone), None))
            assert np.array_equal(out[b, :t], alone.cpu().numpy()[0]), f"clip {b} of frames {frames}"
            assert np.isnan(out[b, t:]).all(), f"clip {b} of frames {frames}: rows beyond the clip were written"


@pytest.mark.parametrize("C_", (64, 256, 512, 768))
def test_layernorm_rows_lens(hip, C_):
    _lib, lib, _ = hip
    rng = np.random.default_rng(C_)
    lens = [1, 63, 64, 65, 129, 300, 7]
    B, T = len(lens), max(lens)
    for post, relu in ((False, 0), (True, 1)):
        x = np.full((B, T, C_), np.nan, F32)
        res = np.full((B, T, C_), np.nan, F32)
        for b, t in enumerate(lens):
            x[b, :t] = rng.standard_normal((t, C_)) * 3 + 1
            res[b, :t] = rng.standard_normal((t, C_))
        g, be = dev(rng.standard_normal(C_).astype(F32)), dev(rng.standard_normal(C_).astype(F32))
        xd, rd = dev(x), dev(res)
        _, _, ld = i32(lens)
        out = nans(B, T, C_)
        _run(_lib, lib.ts_debug_layernorm_rows_lens(_lib.dptr(xd), C_, B, T, _lib.dptr(ld), C_, _lib.dptr(g), _lib.dptr(be),
                                                    _lib.dptr(rd) if post else None, C_, relu, _lib.dptr(out), C_, None))
        out = out.cpu().numpy()
        for b, t in enumerate(lens):
            alone = nans(t, C_)
            xa, ra = dev(x[b, :t]), dev(res[b, :t])
            _run(_lib, lib.ts_debug_layernorm_rows(_lib.dptr(xa), C_, t, C_, _lib.dptr(g), _lib.dptr(be), _lib.dptr(ra) if post else None, C_,
                                                   relu, _lib.dptr(alone), C_, None))
            assert np.array_equal(out[b, :t], alone.cpu().numpy()), f"clip {b} ({t} rows)"
            assert not out[b, t:].any(), f"clip {b}: rows beyond its {t} are not 0"


def test_lerp_ln_lens(hip):
    _lib, lib, _ = hip
    rng = np.random.default_rng(5)
    ns = [160000, 204800, 153600, 400, 16001, 23456, 8533, 33613, 50000]
    frames = [300, 384, 288, 1, 29, 50, 17, 64, 90]
    B, Lin, T = len(ns), feature_rows(max(ns)), max(frames)
    x = np.full((B, Lin, 512), np.nan, F32)
    for b, n in enumerate(ns):
        x[b, :feature_rows(n)] = rng.standard_normal((feature_rows(n), 512))
    g, be = dev(rng.standard_normal(512).astype(F32)), dev(rng.standard_normal(512).astype(F32))
    _, _, nd = i32(ns)
    _, _, fd = i32(frames)
    out, xd = nans(B, T, 512), dev(x)
    _run(_lib, lib.ts_debug_lerp_ln_lens(_lib.dptr(xd), B, Lin, T, _lib.dptr(nd), _lib.dptr(fd), _lib.dptr(g), _lib.dptr(be), _lib.dptr(out), None))
    out = out.cpu().numpy()
    for b, (n, t) in enumerate(zip(ns, frames)):
        Lb = feature_rows(n)
        alone, xa = nans(1, t, 512), dev(x[b:b + 1, :Lb])
        _run(_lib, lib.ts_debug_lerp_ln(_lib.dptr(xa), 1, Lb, t, _lib.dptr(g), _lib.dptr(be), _lib.dptr(alone), None))
        assert np.array_equal(out[b, :t], alone.cpu().numpy()[0]), f"clip {b} ({Lb} -> {t})"
        assert not out[b, t:].any(), f"clip {b}: frames beyond its {t} are not 0"


@pytest.mark.parametrize("form", (1, 0), ids=("moments", "convolution_pass"))
def test_w2v_conv0_lens(hip, form):
    """Both statistics forms; sample counts below one time block of either form, across several blocks, odd; NaN beyond each clip."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(11 + form)
    ns = [400, 645, 5131, 5135, 6007, 12345, 33613, 52001]
    B, N = len(ns), max(ns)
    L0 = (N - 10) // 5 + 1
    wav = np.full((B, N), np.nan, F32)
    for b, n in enumerate(ns):
        wav[b, :n] = (rng.standard_normal(n) * 0.1 + 0.01 * b).astype(F32)
    w = dev((rng.standard_normal((512, 10)) * 0.3).astype(F32))
    g, be = dev(rng.standard_normal(512).astype(F32)), dev(rng.standard_normal(512).astype(F32))
    _, _, nd = i32(ns)
    out, wd = nans(B, L0, 512), dev(wav)
    _run(_lib, lib.ts_debug_w2v_conv0_lens(_lib.dptr(wd), B, N, _lib.dptr(nd), _lib.dptr(w), _lib.dptr(g), _lib.dptr(be), form, _lib.dptr(out), None))
    out = out.cpu().numpy()
    for b, n in enumerate(ns):
        Lb = (n - 10) // 5 + 1
        alone, wa = nans(1, Lb, 512), dev(wav[b:b + 1, :n])
        _run(_lib, lib.ts_debug_w2v_conv0(_lib.dptr(wa), 1, n, _lib.dptr(w), _lib.dptr(g), _lib.dptr(be), form, _lib.dptr(alone), None))
        assert np.array_equal(out[b, :Lb], alone.cpu().numpy()[0]), f"clip {b} ({n} samples)"
        assert not out[b, Lb:].any(), f"clip {b}: rows beyond its {Lb} are not 0"


def test_fill_id_lens(hip):
    _lib, lib, _ = hip
    rng = np.random.default_rng(2)
    lens = [7, 1, 301, 64, 300]
    B, T, nc, nj, ld, col0 = len(lens), max(lens), 4, 64, 320, 256
    idv = dev(np.eye(4, dtype=F32)[np.arange(B) % 4])
    w, bias = dev(rng.standard_normal((nj, nc)).astype(F32)), dev(rng.standard_normal(nj).astype(F32))
    _, _, ldv = i32(lens)
    x = nans(B, T, ld)
    _run(_lib, lib.ts_debug_fill_id_lens(_lib.dptr(idv), nc, _lib.dptr(w), _lib.dptr(bias), nj, _lib.dptr(x), ld, col0, B, T, _lib.dptr(ldv), None))
    x = x.cpu().numpy()
    assert np.isnan(x[:, :, :col0]).all()                           # only the id columns are written
    for b, t in enumerate(lens):
        alone, ia = nans(1, t, ld), idv[b:b + 1].contiguous()
        _run(_lib, lib.ts_debug_fill_id(_lib.dptr(ia), nc, _lib.dptr(w), _lib.dptr(bias), nj, _lib.dptr(alone), ld, col0, 1, t, None))
        assert np.array_equal(x[b, :t, col0:], alone.cpu().numpy()[0, :, col0:]), f"clip {b}"
        assert not x[b, t:, col0:].any(), f"clip {b}: rows beyond its {t} are not 0"
