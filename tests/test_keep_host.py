"""Kept positions, host side (no GPU): `_lib.given_keep_block` — the mask a pass with `given_keep=` hands to the `_keep` entries beside its
given block (include/talkshow_hip.h, "kept positions") —, the vocabulary rule of `_lib.given_block` under a mask, the numpy restatement of
the rule (`sampling.keep_forced`) and the new entries' prototypes and host-side refusals.  Every test fails on a build without the
feature: the helper, the restatement and the entries do not exist there.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 256
NEW = ["ts_pixelcnn_generate_mixed_keep", "ts_body_pixel_infer_mixed_keep", "ts_body_pixel_infer_mixed_poses_keep", "ts_op_sample_keep"]


def _clips():
    """Six clips submitted shuffled: code rows, given rows (none, G = 0, G = H_b among them), per-clip masks and the order of a length sort."""
    rows = [8, 20, 3, 17, 9, 17]
    rng = np.random.default_rng(4)
    G = [8, 9, 0, None, 1, 17]
    counts = list(G)
    keep = ["body", rng.integers(0, 2, (9, 2)).astype(bool), np.zeros((0, 2), np.uint8), None, "hand", None]
    order = sorted(range(len(rows)), key=lambda b: (-rows[b], b))
    return rows, G, counts, keep, order


def _want(G, k):
    """What a clip's rows of the mask must hold."""
    out = np.zeros((G, 2), np.uint8)
    if k is None:
        out[:] = 1
    elif isinstance(k, str):
        out[:, {"body": 0, "hand": 1}[k]] = 1
    else:
        out[:] = np.asarray(k) != 0
    return out


def test_mask_follows_the_sort():
    rows, G, counts, keep, order = _clips()
    mask = _lib.given_keep_block(keep, counts, rows, order)
    assert mask.shape == (6, 20, 2) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    for k, i in enumerate(order):
        g = 0 if G[i] is None else G[i]
        np.testing.assert_array_equal(mask[k, :g], _want(g, keep[i]), err_msg=f"slot {k} = clip {i}")
        assert (mask[k, g:] == 0).all()
    # without an order: the submitted one
    m2 = _lib.given_keep_block(keep, counts, rows)
    for i in range(6):
        np.testing.assert_array_equal(m2[i], mask[order.index(i)])
    # None: no mask at all (every given position kept, the entries without the keyword)
    assert _lib.given_keep_block(None, counts, rows, order) is None
    # one string for all: the clips that bring rows get it, a clip that brings none stays empty
    for part, col in (("body", 0), ("hand", 1)):
        m3 = _lib.given_keep_block(part, counts, rows, order)
        for k, i in enumerate(order):
            g = 0 if G[i] is None else G[i]
            assert (m3[k, :g, col] == 1).all() and (m3[k, :g, 1 - col] == 0).all() and (m3[k, g:] == 0).all()
    # one (B, G, 2) block for all clips, as 0 / 1 integers of any width and as bool
    blk = np.random.default_rng(1).integers(0, 2, (2, 3, 2))
    for dt in (np.int64, np.uint8, bool):
        m4 = _lib.given_keep_block(blk.astype(dt), [3, 3], [5, 4])
        assert m4.shape == (2, 5, 2) and np.array_equal(m4[:, :3], blk) and (m4[:, 3:] == 0).all()
    # the result owns its memory
    arr = keep[1].copy()
    keep[1][...] = True
    np.testing.assert_array_equal(mask[order.index(1), :9], arr)


def test_counts_from_the_keywords():
    g = [np.zeros((3, 2), np.int64), None, np.zeros((0, 2), np.int64), None]
    p = [None, np.zeros((9, 129), np.float32), None, None]
    assert _lib.given_counts(g, p, 4) == [3, 2, 0, None]
    assert _lib.given_counts(np.zeros((4, 5, 2), np.int64), None, 4) == [5] * 4
    assert _lib.given_counts(None, np.zeros((4, 11, 129), np.float32), 4) == [2] * 4
    assert _lib.given_counts(None, None, 3) == [None] * 3


def test_errors_name_the_submitted_clip():
    rows, G, counts, keep, order = _clips()

    def bad(i, k, match):
        kv = list(keep)
        kv[i] = k
        with pytest.raises(ValueError, match=match):
            _lib.given_keep_block(kv, counts, rows, order)
    bad(1, np.zeros((8, 2), bool), r"clip 1 must have shape \(9, 2\)")              # not the clip's given rows
    bad(0, np.zeros((8,), bool), r"clip 0 must have shape \(8, 2\)")
    bad(5, np.zeros((17, 3), np.uint8), r"clip 5 must have shape \(17, 2\)")
    bad(4, np.full((1, 2), 2), r"clip 4 must be bool or 0 / 1 integers.*value 2")
    bad(4, np.full((1, 2), -1), r"clip 4 must be bool or 0 / 1 integers.*value -1")
    bad(0, np.zeros((8, 2), np.float32), r"clip 0 must be bool or 0 / 1 integers, got float32")
    bad(5, "hands", r"clip 5 is None, 'body', 'hand' or a \(G, 2\) mask, got 'hands'")
    bad(3, "body", r"clip 3 selects from given rows, but the clip brings none")
    bad(3, np.zeros((0, 2), bool), r"clip 3 selects from given rows, but the clip brings none")
    with pytest.raises(ValueError, match="'torso'"):
        _lib.given_keep_block("torso", counts, rows, order)
    with pytest.raises(ValueError, match="brings none"):
        _lib.given_keep_block("body", [None] * 6, rows, order)
    with pytest.raises(ValueError, match="one entry per clip"):
        _lib.given_keep_block(keep[:-1], counts, rows, order)
    with pytest.raises(ValueError, match=r"\(B=6, G, 2\)"):
        _lib.given_keep_block(np.zeros((5, 2, 2), bool), counts, rows, order)
    with pytest.raises(ValueError, match="permutation"):
        _lib.given_keep_block(keep, counts, rows, [0, 0, 1, 2, 3, 4])


def test_vocabulary_rule_covers_kept_positions_only():
    rows, G, counts, keep, order = _clips()
    rng = np.random.default_rng(8)
    given = [None if g is None else rng.integers(0, V, (g, 2)) for g in G]
    mask = _lib.given_keep_block(keep, counts, rows, order)
    poisoned = [None if g is None else g.copy() for g in given]
    for i, g in enumerate(poisoned):
        if g is not None and g.size:
            unkept = _want(len(g), keep[i]) == 0
            g[unkept] = np.where(np.arange(int(unkept.sum())) % 2 == 0, 2 ** 40, -7)
    assert any((g is not None and ((g < 0) | (g >= V)).any()) for g in poisoned)
    block, table = _lib.given_block(poisoned, rows, V, order, keep=mask)                # accepted: the pass never reads them
    clean, table0 = _lib.given_block(given, rows, V, order, keep=mask)
    assert np.array_equal(table, table0) and np.array_equal(block, clean)
    for k, i in enumerate(order):
        g = 0 if G[i] is None else G[i]
        kept = mask[k, :g] != 0
        assert np.array_equal(block[k, :g][kept], given[i][kept] if g else np.zeros(0, np.int64)) and (block[k, :g][~kept] == 0).all()
    with pytest.raises(ValueError, match="outside"):                                    # without the mask the same block is refused
        _lib.given_block(poisoned, rows, V, order)
    # a bad code at a KEPT position is refused, naming the clip
    for i, (r, j) in ((0, (3, 0)), (4, (0, 1)), (5, (16, 1))):
        gv = [None if g is None else g.copy() for g in given]
        gv[i][r, j] = V
        with pytest.raises(ValueError, match=rf"clip {i} hold the code {V}, outside"):
            _lib.given_block(gv, rows, V, order, keep=mask)
    # keep=None is the rule there was
    b0, t0 = _lib.given_block(given, rows, V, order, keep=None)
    b1, t1 = _lib.given_block(given, rows, V, order)
    assert np.array_equal(b0, b1) and np.array_equal(t0, t1)


def test_keep_forced_against_a_loop():
    rng = np.random.default_rng(2)
    B, H = 7, 6
    G = rng.integers(0, H + 1, B)
    G[0], G[1] = 0, H
    keep = rng.integers(0, 2, (B, H, 2)).astype(np.uint8)
    keep[2] = 255 * keep[2]                                   # a byte is 0 or not 0
    for r in range(H):
        for j in range(2):
            got = S.keep_forced(G, keep, r, j)
            none = S.keep_forced(G, None, r, j)
            assert got.dtype == bool and got.shape == (B,)
            for b in range(B):
                below = 2 * r + j < 2 * G[b]
                assert none[b] == below
                assert got[b] == (below and keep[b, r, j] != 0)
    # the mask is read below G_b only: rows at or beyond may be missing altogether
    ragged = [np.ones((int(g), 2), np.uint8) for g in G]
    for r in range(H):
        for j in range(2):
            assert np.array_equal(S.keep_forced(G, ragged, r, j), S.keep_forced(G, None, r, j))


def test_entries_are_declared_and_refuse_on_the_host():
    header = open(os.path.join(REPO, "include", "talkshow_hip.h")).read()
    declared = set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/talkshow_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "kept positions" in header and header.index("kept positions") > header.index("given poses")
    # each sibling takes its parent's arguments with keep_dev ahead of the stream
    for kid, parent in (("ts_pixelcnn_generate_mixed_keep", "ts_pixelcnn_generate_mixed_given"),
                        ("ts_body_pixel_infer_mixed_keep", "ts_body_pixel_infer_mixed_given"),
                        ("ts_body_pixel_infer_mixed_poses_keep", "ts_body_pixel_infer_mixed_poses")):
        pa, ka = _lib.SIGNATURES[parent][1], _lib.SIGNATURES[kid][1]
        assert ka == pa[:-1] + [C.c_void_p, pa[-1]], kid
    ga, ka = _lib.SIGNATURES["ts_op_sample_given"][1], _lib.SIGNATURES["ts_op_sample_keep"][1]
    assert ka == ga[:-2] + [C.c_void_p] + ga[-2:]             # given_rows_host where forced_host was, then keep_dev, given_dev, stream
    # refused before anything touches a device: null arguments (this runs without a GPU)
    i32p = C.POINTER(C.c_int32)
    t = np.zeros(2, np.int32)
    assert lib.ts_op_sample_keep(None, None, 2, 8, _lib.TS_SAMPLE_GREEDY, None, 0, 0, 0, None, 0, None, None, t.ctypes.data_as(i32p), None, None, None) != 0
    assert "ts_op_sample_keep" in lib.ts_last_error().decode()
    assert lib.ts_pixelcnn_generate_mixed_keep(None, None, None, t.ctypes.data_as(i32p), None, 2, 4, _lib.TS_SAMPLE_GREEDY, None, 0, None, None, None, 0,
                                               None, None, None, None, None, None) != 0
    assert "null argument" in lib.ts_last_error().decode()
    assert lib.ts_body_pixel_infer_mixed_keep(None, None, None, None, None, None, t.ctypes.data_as(i32p), None, 2, 16, _lib.TS_SAMPLE_GREEDY, None, 0,
                                              None, None, None, None, 0, None, None, None, None, None, None) != 0
    assert "null argument" in lib.ts_last_error().decode()
    assert lib.ts_body_pixel_infer_mixed_poses_keep(None, None, None, None, None, None, t.ctypes.data_as(i32p), None, 2, 16, _lib.TS_SAMPLE_GREEDY, None,
                                                    0, None, None, None, None, 0, None, None, 0, None, None, t.ctypes.data_as(C.c_void_p), None) != 0
    assert "needs the given poses" in lib.ts_last_error().decode()
