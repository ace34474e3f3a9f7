"""The kernels of the packed mixed face pass (csrc/face.hip), one by one through their debug entries (include/talkshow_hip_debug.h).

A packed pass promises the bits of the padded pass, so each kernel is held to `array_equal` against the length variant it replaces
(tests/test_gpu_face_mixed_ops.py holds those to the uniform kernels, tests/test_gpu_face_ops.py holds the uniform kernels to float64);
attention is also checked against float64 directly, at the uniform kernel's bound.  Rows that belong to no clip hold NaN on the way in
and must be untouched on the way out.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_face_mixed_ops import feature_rows, i32
from test_gpu_face_ops import ATT_BOUND, F32, _run, _scaled_close, att_ref, dev, hip, nans, qkv_case  # noqa: F401  (hip: fixture)

pytestmark = pytest.mark.gpu

ATT_FRAMES = (1, 63, 64, 65, 128, 129)


def _l0(n):
    return (n - 10) // 5 + 1


def _offsets(counts, mult=1):
    seg = [-(-c // mult) * mult for c in counts]
    return np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)


@pytest.mark.parametrize("heads,order", [(12, (0, 1, 2, 3, 4, 5)), (12, (5, 0, 3, 2, 4, 1)), (1, (2, 5, 1, 0, 4, 3))])
def test_attention_packed(hip, heads, order):
    """Frame counts 1, 63, 64, 65, 128 and 129 in ONE launch, packed back to back: every clip's rows within the uniform kernel's bound of
    float64 softmax(q k^T / 8) v, and equal to `attention_mixed` on the padded batch bit for bit.  The padded batch holds NaN in every row
    that belongs to no clip; the packed rows have no such row — the rows around them (one clip's worth before and after) hold NaN and
    stay untouched."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(heads + 10 * order[0])
    frames = [ATT_FRAMES[i] for i in order]
    B, T_max, HID, R = len(frames), max(frames), heads * 64, sum(frames)
    row0 = _offsets(frames)
    clips = [qkv_case("synthetic", 1, t, heads, rng)[0] for t in frames]
    guard = 129
    packed = np.full((guard + R + guard, 3 * HID), np.nan, F32)
    padded = np.full((B, T_max, 3 * HID), np.nan, F32)
    for b, c in enumerate(clips):
        packed[guard + row0[b]:guard + row0[b + 1]] = c
        padded[b, :frames[b]] = c
    fh, fp, fd = i32(frames)
    out_all, qd = nans(guard + R + guard, HID), dev(packed)
    _run(_lib, lib.ts_debug_attention_packed(C.c_void_p(qd.data_ptr() + guard * 3 * HID * 4), fp, _lib.dptr(fd), B, HID, heads, 0.125,
                                             C.c_void_p(out_all.data_ptr() + guard * HID * 4), None))
    out_all = out_all.cpu().numpy()
    assert np.isnan(out_all[:guard]).all() and np.isnan(out_all[guard + R:]).all(), "rows outside the packed block were written"
    out = out_all[guard:guard + R]
    assert np.isfinite(out).all()
    mixed, pd = nans(B, T_max, HID), dev(padded)
    _run(_lib, lib.ts_debug_attention_mixed(_lib.dptr(pd), fp, _lib.dptr(fd), B, T_max, HID, heads, 0.125, _lib.dptr(mixed), None))
    mixed = mixed.cpu().numpy()
    for b, t in enumerate(frames):
        got = out[row0[b]:row0[b + 1]]
        assert np.array_equal(got, mixed[b, :t]), f"clip {b} ({t} frames): differs from attention_mixed"
        ref = att_ref(clips[b][None], heads, np.arange(t))[0]
        scale = float(np.abs(clips[b].reshape(t, 3, HID)[:, 2]).max())
        _scaled_close(f"attention_packed.T{t}.h{heads}", got, ref, scale, ATT_BOUND["synthetic"])


@pytest.mark.parametrize("C_", (768, 4, 100))
def test_pack_unpack_rows(hip, C_):
    """pack: exact copies of each clip's rows, nothing outside the packed block written, rows beyond a clip's frames (NaN) not read into
    it.  unpack: exact copies, +0.0 (sign bit clear) at and beyond frames[b], every element of the padded block written, its NaN-filled
    surroundings untouched."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(C_)
    frames = [1, 63, 64, 65, 129, 7, 300]
    B, T, R = len(frames), max(frames), sum(frames)
    row0 = _offsets(frames)
    fh, fp, fd = i32(frames)
    src = np.full((B, T, C_), np.nan, F32)
    for b, t in enumerate(frames):
        src[b, :t] = rng.standard_normal((t, C_))
    guard = 8
    dst, sd = nans(guard + R + guard, C_), dev(src)
    _run(_lib, lib.ts_debug_pack_rows(_lib.dptr(sd), fp, B, T, C_, C.c_void_p(dst.data_ptr() + guard * C_ * 4), None))
    dst = dst.cpu().numpy()
    assert np.isnan(dst[:guard]).all() and np.isnan(dst[guard + R:]).all(), "pack_rows wrote outside its block"
    packed = dst[guard:guard + R]
    for b, t in enumerate(frames):
        assert np.array_equal(packed[row0[b]:row0[b + 1]], src[b, :t]), f"pack_rows, clip {b}"
    back, pk = nans(guard + B * T + guard, C_), dev(np.concatenate([np.full((guard, C_), np.nan, F32), packed, np.full((guard, C_), np.nan, F32)]))
    _run(_lib, lib.ts_debug_unpack_rows(C.c_void_p(pk.data_ptr() + guard * C_ * 4), fp, _lib.dptr(fd), B, T, C_,
                                        C.c_void_p(back.data_ptr() + guard * C_ * 4), None))
    back = back.cpu().numpy()
    assert np.isnan(back[:guard]).all() and np.isnan(back[guard + B * T:]).all(), "unpack_rows wrote outside its block"
    body = back[guard:guard + B * T].reshape(B, T, C_)
    for b, t in enumerate(frames):
        assert np.array_equal(body[b, :t], src[b, :t]), f"unpack_rows, clip {b}"
        assert not body[b, t:].view(np.uint32).any(), f"unpack_rows, clip {b}: rows beyond its {t} frames are not +0.0"


@pytest.mark.parametrize("form", (1, 0), ids=("moments", "convolution_pass"))
def test_w2v_conv0_packed(hip, form):
    """The packed apply pass against `w2v_conv0_lens` on the rows both write (the clip's own rows and the zeros up to the end of its
    segment); both statistics forms; sample counts whose row counts are 1, 63, 0 and 15 off a multiple of 64, below one block, across
    several; NaN beyond each clip's samples; nothing outside the (feat_rows, 512) block written."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(21 + form)
    ns = [400, 645, 650, 640, 5131, 5135, 12345, 33613, 400]
    assert {_l0(n) % 64 for n in ns} >= {0, 1, 63, 15}
    B, N = len(ns), max(ns)
    L0 = _l0(N)
    off = _offsets([_l0(n) for n in ns], 64)
    wav = np.full((B, N), np.nan, F32)
    for b, n in enumerate(ns):
        wav[b, :n] = (rng.standard_normal(n) * 0.1 + 0.01 * b).astype(F32)
    w = dev((rng.standard_normal((512, 10)) * 0.3).astype(F32))
    g, be = dev(rng.standard_normal(512).astype(F32)), dev(rng.standard_normal(512).astype(F32))
    nh, np_, nd = i32(ns)
    wd = dev(wav)
    lens_out = nans(B, L0, 512)
    _run(_lib, lib.ts_debug_w2v_conv0_lens(_lib.dptr(wd), B, N, _lib.dptr(nd), _lib.dptr(w), _lib.dptr(g), _lib.dptr(be), form, _lib.dptr(lens_out), None))
    lens_out = lens_out.cpu().numpy()
    guard, rows = 4, int(off[-1])
    out = nans(guard + rows + guard, 512)
    _run(_lib, lib.ts_debug_w2v_conv0_packed(_lib.dptr(wd), B, N, np_, _lib.dptr(nd), _lib.dptr(w), _lib.dptr(g), _lib.dptr(be), form,
                                             C.c_void_p(out.data_ptr() + guard * 512 * 4), None))
    out = out.cpu().numpy()
    assert np.isnan(out[:guard]).all() and np.isnan(out[guard + rows:]).all(), "rows outside the packed block were written"
    body = out[guard:guard + rows]
    for b, n in enumerate(ns):
        seg = body[off[b]:off[b + 1]]
        both = min(seg.shape[0], L0)                                      # the rows both kernels write for this clip
        assert both >= _l0(n)
        assert np.array_equal(seg[:both], lens_out[b, :both]), f"clip {b} ({n} samples)"
        assert not seg[_l0(n):].any(), f"clip {b}: rows between its {_l0(n)} and the end of its segment are not 0"


def test_lerp_ln_packed(hip):
    """Level-6 rows at feat_off[b] / 64 of one axis against `lerp_ln_lens` on the padded (B, Lin, 512) block: the whole padded output equal,
    zeros included; the rows between the clips' own hold NaN."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(6)
    ns = [160000, 204800, 153600, 400, 16001, 23456, 8533, 33613, 50000]
    frames = [300, 384, 288, 1, 29, 50, 17, 64, 90]
    B, Lin, T = len(ns), feature_rows(max(ns)), max(frames)
    off = _offsets([_l0(n) for n in ns], 64)
    padded = np.full((B, Lin, 512), np.nan, F32)
    packed = np.full((int(off[-1]) // 64, 512), np.nan, F32)
    for b, n in enumerate(ns):
        x = rng.standard_normal((feature_rows(n), 512)).astype(F32)
        padded[b, :x.shape[0]] = x
        packed[off[b] // 64:off[b] // 64 + x.shape[0]] = x
        assert off[b] // 64 + x.shape[0] <= off[b + 1] // 64
    g, be = dev(rng.standard_normal(512).astype(F32)), dev(rng.standard_normal(512).astype(F32))
    nh, np_, nd = i32(ns)
    _, _, fd = i32(frames)
    want, xd = nans(B, T, 512), dev(padded)
    _run(_lib, lib.ts_debug_lerp_ln_lens(_lib.dptr(xd), B, Lin, T, _lib.dptr(nd), _lib.dptr(fd), _lib.dptr(g), _lib.dptr(be), _lib.dptr(want), None))
    guard = 4
    got, pd = nans(guard + B * T + guard, 512), dev(packed)
    _run(_lib, lib.ts_debug_lerp_ln_packed(_lib.dptr(pd), B, T, np_, _lib.dptr(nd), _lib.dptr(fd), _lib.dptr(g), _lib.dptr(be),
                                           C.c_void_p(got.data_ptr() + guard * 512 * 4), None))
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.isnan(got[:guard]).all() and np.isnan(got[guard + B * T:]).all(), "rows outside the padded block were written"
    body = got[guard:guard + B * T].reshape(B, T, 512)
    for b, t in enumerate(frames):
        assert np.isfinite(body[b, :t]).all() and np.array_equal(body[b, :t], want[b, :t]), f"clip {b} ({feature_rows(ns[b])} -> {t})"
        assert not body[b, t:].any(), f"clip {b}: frames beyond its {t} are not 0"
