"""Speaker style, host side (no GPU): the numpy restatement of the rule (`sampling.style_rows`; include/talkshow_hip.h, "speaker style"),
`_lib.style_block` — the weight block a pass with `style=` hands to the `_style` entries — through the length sort, every refusal with
the clip it names, and `ts_style_check`.  Every test fails on a build without the feature: the helper, the restatement and the entries
do not exist there.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NC = 4
NEW = ["ts_pixelcnn_generate_mixed_style", "ts_body_pixel_infer_mixed_style", "ts_body_pixel_infer_mixed_poses_style", "ts_style_check",
       "ts_op_style_rows"]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _table(seed, nc=NC, w=24):
    t = np.random.default_rng(seed).standard_normal((nc, w)).astype(F32)
    t[min(1, nc - 1), 3] = -0.0
    t[min(2, nc - 1), 5] = 0.0
    return t


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_rule_against_float64():
    """|fp32 result - exact| <= the roundings the rule makes: one per product and one per sum, each at most half an ulp of a magnitude
    bounded by sum |w_c E_c|: NC products + (NC - 1) sums, so (2 NC - 1) * 2^-24 * sum |w_c E_c| (first order, rounded up to 2 NC)."""
    rng = np.random.default_rng(1)
    for nc in (1, 4, 7):
        t = _table(10 + nc, nc)
        w = rng.standard_normal((50, nc)).astype(F32) * 2
        w[rng.random(w.shape) < 0.3] = 0
        got = S.style_rows(w, t)
        assert got.dtype == F32 and got.shape == (50, t.shape[1])
        exact = w.astype(np.float64) @ t.astype(np.float64)
        bound = 2 * nc * 2.0 ** -24 * (np.abs(w).astype(np.float64) @ np.abs(t).astype(np.float64))
        assert (np.abs(got.astype(np.float64) - exact) <= bound).all()


def test_one_hot_is_the_table_row_bit_for_bit():
    t = _table(2)
    assert np.signbit(t[1, 3]) and t[1, 3] == 0                    # the -0.0 entry is there
    got = S.style_rows(np.eye(NC, dtype=F32), t)
    assert np.array_equal(_bits(got), _bits(t))
    # leading axes are kept: a (B, H, NC) block of one-hot rows
    lab = np.array([[0, 1, 1], [3, 2, 1]])
    got = S.style_rows(np.eye(NC, dtype=F32)[lab], t)
    assert got.shape == (2, 3, t.shape[1]) and np.array_equal(_bits(got), _bits(t[lab]))


def test_zero_weights():
    t = _table(3)
    z = S.style_rows(np.zeros((2, NC), F32), t)
    assert np.array_equal(_bits(z), np.zeros_like(_bits(z)))        # +0.0, not -0.0
    z = S.style_rows(np.full((1, NC), -0.0, F32), t)
    assert np.array_equal(_bits(z), np.zeros_like(_bits(z)))        # a -0.0 weight is a zero weight
    # a zero weight's table row is not read into the sum: NaN there does not reach the output
    t2 = t.copy()
    t2[2] = np.nan
    w = np.array([[0.7, 0.3, 0.0, -0.5]], F32)
    got = S.style_rows(w, t2)
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(S.style_rows(w, t)))
    # product and sum are rounded separately, in ascending order
    a = (F32(0.7) * t[0]).astype(F32)
    a = (a + (F32(0.3) * t[1]).astype(F32)).astype(F32)
    a = (a + (F32(-0.5) * t[3]).astype(F32)).astype(F32)
    assert np.array_equal(_bits(got[0]), _bits(a))
    with pytest.raises(ValueError):
        S.style_rows(np.zeros((2, NC + 1), F32), t)


# ---- the block ---------------------------------------------------------------------------------------------------------------------------
def _clips():
    rows = [8, 20, 3, 17, 9, 17]
    order = sorted(range(len(rows)), key=lambda b: (-rows[b], b))
    ids = np.array([0, 1, 2, 3, 0, 1])
    return rows, order, ids


def test_block_per_clip_rows_follow_the_sort():
    rows, order, ids = _clips()
    rng = np.random.default_rng(5)
    style = [None, rng.standard_normal(NC), None, [0.7, 0, 0.3, 0], rng.standard_normal(NC).astype(F32), None]
    blk = _lib.style_block(style, rows, NC, order, ids=ids)
    assert blk.shape == (6, 1, NC) and blk.dtype == F32            # no track anywhere: the S = 1 form
    for k, i in enumerate(order):
        want = np.eye(NC, dtype=F32)[ids[i]] if style[i] is None else np.asarray(style[i], F32)
        assert np.array_equal(_bits(blk[k, 0]), _bits(want)), f"slot {k} = clip {i}"
    # without an order: the submitted one
    b2 = _lib.style_block(style, rows, NC, ids=ids)
    for i in range(6):
        assert np.array_equal(b2[i], blk[order.index(i)])
    assert _lib.style_block(None, rows, NC, order, ids=ids) is None
    # one id for all clips
    b3 = _lib.style_block([None] * 6, rows, NC, order, ids=[2])
    assert np.array_equal(b3, np.tile(np.eye(NC, dtype=F32)[2], (6, 1, 1)))


def test_block_with_tracks():
    rows, order, ids = _clips()
    rng = np.random.default_rng(6)
    style = [None, rng.standard_normal((20, NC)), [0, 0, 1.5, -0.5], None, rng.standard_normal((9, NC)), rng.standard_normal(NC)]
    blk = _lib.style_block(style, rows, NC, order, ids=ids)
    assert blk.shape == (6, 20, NC) and blk.dtype == F32           # one track anywhere: every clip gets one
    for k, i in enumerate(order):
        e = np.eye(NC, dtype=F32)[ids[i]] if style[i] is None else np.asarray(style[i], F32)
        if e.ndim == 1:
            assert np.array_equal(blk[k], np.tile(e, (20, 1))), f"slot {k} = clip {i}: a per-clip row is repeated into a track"
        else:
            assert np.array_equal(blk[k, :rows[i]], e) and np.array_equal(blk[k, rows[i]:], np.tile(e[-1], (20 - rows[i], 1)))
    assert np.isfinite(blk).all()


def test_block_one_array_for_all():
    rows, order, ids = _clips()
    one = np.array([0.25, 0.25, 0.5, 0], F32)
    blk = _lib.style_block(one, rows, NC, order)
    assert blk.shape == (6, 1, NC) and np.array_equal(blk[:, 0], np.tile(one, (6, 1)))
    assert np.array_equal(_lib.style_block([0.25, 0.25, 0.5, 0], rows, NC, order), blk)          # a plain list of numbers is one row
    per = np.random.default_rng(7).standard_normal((6, NC)).astype(F32)
    blk = _lib.style_block(per, rows, NC, order)
    for k, i in enumerate(order):
        assert np.array_equal(blk[k, 0], per[i])
    import torch
    assert np.array_equal(_lib.style_block(torch.from_numpy(per), rows, NC, order), blk)


def test_refusals_name_the_clip():
    rows, order, ids = _clips()
    ok = np.ones(NC, F32)

    def bad(style, pattern, **kw):
        with pytest.raises(ValueError, match=pattern):
            _lib.style_block(style, rows, NC, order, who="generate_clips", **{"ids": ids, **kw})
    bad([ok, ok, np.ones((4, NC)), ok, ok, ok], r"generate_clips: style of clip 2 must have shape \(4,\) or \(3, 4\)")       # a track of the wrong length
    bad([ok, ok, ok, np.ones((17, NC, 1)), ok, ok], r"style of clip 3 must have shape")
    bad([ok, np.ones(NC + 1), ok, ok, ok, ok], r"style of clip 1 has 5 weights per row, the model has NC = 4")
    bad([ok, ok, ok, ok, np.ones((9, 3)), ok], r"style of clip 4 has 3 weights per row")
    bad([ok, ok, ok, ok, ok, np.array([1, np.nan, 0, 0])], r"style of clip 5: ts_style_check: weight 1 \(row 0, speaker 1\) is not finite")
    tr = np.ones((20, NC))
    tr[7, 2] = np.inf
    bad([ok, tr, ok, ok, ok, ok], r"style of clip 1: ts_style_check: weight 30 \(row 7, speaker 2\) is not finite")
    bad([ok, ok, ok, np.array(["a"] * NC), ok, ok], r"style of clip 3 must be numbers")
    bad([None, ok, ok, ok, ok, ok], r"style of clip 0 is None", ids=None)
    bad([ok, ok, ok, ok, ok, None], r"style of clip 5 is None", ids=[0, 1, 2, 3, 0, 9])
    bad([ok] * 5, r"one entry per clip \(6\)")
    bad(np.ones((5, NC), F32), r"one style array for all clips must have shape \(NC=4,\) or \(B=6, NC=4\)")
    bad(np.ones((6, 20, NC), F32), r"one style array for all clips")
    bad(np.ones(NC + 2, F32), r"style of clip 0 has 6 weights per row")
    bad("speaker", r"one entry per clip")


# ---- the C side ----------------------------------------------------------------------------------------------------------------------------
def test_style_check():
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    w = np.random.default_rng(8).standard_normal((5, NC)).astype(F32) * 1e30
    w[0, 0], w[1, 1] = -0.0, -3.0                                   # any finite float: no sign rule, no sum rule
    assert lib.ts_style_check(w.ctypes.data_as(fp), w.size, NC) == 0
    for val in (np.nan, np.inf, -np.inf):
        x = w.copy()
        x[3, 2] = val
        x[4, 0] = np.nan                                            # the FIRST bad index is named
        assert lib.ts_style_check(x.ctypes.data_as(fp), x.size, NC) != 0
        assert "weight 14 (row 3, speaker 2) is not finite" in lib.ts_last_error().decode()
    assert lib.ts_style_check(w.ctypes.data_as(fp), 0, NC) == 0
    assert lib.ts_style_check(None, 4, NC) != 0 and lib.ts_style_check(w.ctypes.data_as(fp), 4, 0) != 0


def test_prototypes_and_header():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "talkshow_hip.h")).read()
    assert "speaker style" in hdr
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in talkshow_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: the ctypes prototype and the header disagree"
    for name in NEW[:3]:
        assert re.search(name + r"\s*\([^;]*const float \*style_dev, int style_rows,\s*void \*stream\);", hdr), name


def test_keyword_exists_where_documented():
    import inspect

    from nets.smplx_body_pixel import TrainWrapper
    from talkshow_amd import parallel
    from talkshow_amd.modules import GatedPixelCNN
    for fn in (TrainWrapper.generate_clips, TrainWrapper.generate_batch, TrainWrapper.generate_clips_from_wav, TrainWrapper.score_clips,
               TrainWrapper.score_motion_clips, parallel.whole_body_clips, GatedPixelCNN.run):
        p = inspect.signature(fn).parameters
        assert "style" in p and p["style"].default is None, fn.__qualname__
