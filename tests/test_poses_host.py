"""Given poses, host side (no GPU): `sampling.given_pose_rows` — the numpy restatement of the frame rule — and `_lib.given_pose_block`, the
padded block and the frame table a pass with `given_poses=` hands to `ts_body_pixel_infer_mixed_poses` (include/talkshow_hip.h, "given
poses").  Every ValueError is raised with the library never loaded.  Every test fails on a build without the feature: the names do not
exist there.
"""
import ctypes as C

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

F32 = np.float32
W = 129


@pytest.fixture()
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded by host-only code")
    monkeypatch.setattr(_lib, "load", boom)


def _order(rows):
    from nets.smplx_body_pixel import mixed_pass_order
    return mixed_pass_order([4 * h + 1 for h in rows])[0]


def test_rule_table(no_library):
    """P in {None, 0, 4, 5, 7, 8, 31} of a clip with T = 31 MFCC rows (7 code rows) and of one with T = 4 (one row)."""
    assert [S.given_pose_rows(P, 31) for P in (None, 0, 4, 5, 7, 8, 31)] == [0, 0, 1, 1, 1, 2, 7]
    assert [S.given_pose_rows(P, 4) for P in (None, 0, 4, 5, 7)] == [0, 0, 1, 1, 1]
    for P in (1, 2, 3):
        with pytest.raises(ValueError, match=rf"P = {P} frames; one code row needs 4"):
            S.given_pose_rows(P, 31)
    with pytest.raises(ValueError, match=r"P = 8 frames are 2 code rows but the clip has 1"):
        S.given_pose_rows(8, 7)
    with pytest.raises(ValueError, match=r"P = 32 frames are 8 code rows but the clip has 7"):
        S.given_pose_rows(32, 31)
    with pytest.raises(ValueError):
        S.given_pose_rows(-4, 31)


def _clips():
    rows = [7, 20, 1, 17, 7, 2, 9]
    P = [None, 0, 4, 5, 7, 8, 31]                                # the table of the issue, one per clip
    rng = np.random.default_rng(5)
    given = [None if p is None else rng.standard_normal((p, W)).astype(F32) for p in P]
    return rows, P, given, _order(rows)


def test_block_and_table_follow_the_sort(no_library):
    rows, P, given, order = _clips()
    assert order != list(range(len(rows)))
    block, table = _lib.given_pose_block(given, rows, order)
    assert isinstance(block, np.ndarray) and block.shape == (7, 31, W) and block.dtype == F32
    assert table.shape == (7,) and table.dtype == np.int32
    for k, i in enumerate(order):
        p = 0 if P[i] is None else P[i]
        assert table[k] == p and table[k] // 4 == S.given_pose_rows(P[i], 4 * rows[i])
        assert np.array_equal(block[k, :p], given[i][:p] if p else block[k, :0])
        assert (block[k, p:] == 0).all()
    # without an order: the submitted one; one (B, P, 129) block is B entries of P frames
    block2, table2 = _lib.given_pose_block(given, rows)
    for i in range(7):
        assert np.array_equal(block2[i], block[order.index(i)]) and table2[i] == table[order.index(i)]
    one = np.arange(2 * 8 * W, dtype=F32).reshape(2, 8, W)
    b3, t3 = _lib.given_pose_block(one, [5, 2])
    assert b3.shape == (2, 8, W) and list(t3) == [8, 8] and np.array_equal(b3, one)
    # nothing given anywhere: an empty block and a table of zeros
    b4, t4 = _lib.given_pose_block([None, None], [5, 2])
    assert b4.shape == (2, 0, W) and list(t4) == [0, 0]
    # the results own their memory
    keep = [None if g is None else g.copy() for g in given]
    for g in given:
        if g is not None:
            g[...] = -5
    for k, i in enumerate(order):
        if keep[i] is not None:
            assert np.array_equal(block[k, :len(keep[i])], keep[i])


def test_errors_name_the_submitted_clip(no_library):
    rows, P, given, order = _clips()

    def bad(i, g, match):
        gv = list(given)
        gv[i] = g
        with pytest.raises(ValueError, match=match):
            _lib.given_pose_block(gv, rows, order, who="t")
    for p in (1, 2, 3):
        bad(3, np.zeros((p, W), F32), rf"clip 3 brings {p} given pose frames; one code row needs 4")
    bad(2, np.zeros((8, W), F32), r"clip 2 brings 8 given pose frames = 2 code rows but has 1 code rows")
    bad(5, np.zeros((12, W), F32), r"clip 5 brings 12 given pose frames = 3 code rows but has 2 code rows")
    bad(0, np.zeros((8, 128), F32), r"clip 0 must have shape \(P, 129\)")
    bad(6, np.zeros(W, F32), r"clip 6 must have shape \(P, 129\)")
    bad(1, np.zeros((8, W), np.int64), r"clip 1 must be floats")
    with pytest.raises(ValueError, match="one entry per clip"):
        _lib.given_pose_block(given[:-1], rows, order)
    with pytest.raises(ValueError, match=r"\(B=7, P, 129\)"):
        _lib.given_pose_block(np.zeros((6, 8, W), F32), rows, order)
    with pytest.raises(ValueError, match="permutation"):
        _lib.given_pose_block(given, rows, [0, 0, 1, 2, 3, 4, 5])
    # a clip brings one kind
    codes = [None] * 7
    codes[4] = np.zeros((1, 2), np.int64)
    with pytest.raises(ValueError, match=r"clip 4 brings both"):
        _lib.given_kinds_check(codes, given, 7, "t")
    codes[4], codes[0] = None, np.zeros((1, 2), np.int64)          # clip 0 brings no poses: fine
    _lib.given_kinds_check(codes, given, 7, "t")
    with pytest.raises(ValueError, match=r"clip 1 brings both"):    # one block counts for every clip
        _lib.given_kinds_check(np.zeros((7, 1, 2), np.int64), given, 7, "t")


def test_the_c_table_rule():
    """`ts_given_pose_rows_check`: host only, the rule of `given_pose_rows` on a table, naming the clip."""
    lib = _lib.load()
    i32p = C.POINTER(C.c_int32)
    lens = np.asarray([83, 70, 16, 7], np.int32)          # 20, 17, 4, 1 code rows

    def rc(tab):
        t = np.asarray(tab, np.int32)
        return lib.ts_given_pose_rows_check(t.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), len(tab))
    assert rc([83, 0, 19, 7]) == 0 and rc([0, 0, 0, 0]) == 0 and rc([80, 71, 16, 4]) == 0
    for p in (1, 2, 3):
        assert rc([0, p, 0, 0]) != 0 and "clip 1" in lib.ts_last_error().decode()
    assert rc([84, 0, 0, 0]) != 0 and "clip 0" in lib.ts_last_error().decode()
    assert rc([0, 0, 0, 8]) != 0 and "clip 3" in lib.ts_last_error().decode()
    assert rc([0, 0, -4, 0]) != 0 and "clip 2" in lib.ts_last_error().decode()
    for tab in ([83, 0, 19, 7], [0, 72, 0, 0], [0, 0, 0, 8], [0, 2, 0, 0]):
        def ok():
            for P, T in zip(tab, lens):
                S.given_pose_rows(P, T)
        if rc(tab) == 0:
            ok()
        else:
            with pytest.raises(ValueError):
                ok()
