"""Given rows, host side (no GPU): `_lib.given_block` — the padded block and the row table a pass with `given=` hands to
`ts_body_pixel_infer_mixed_given` — and the numpy restatement of the rule (`sampling.given_logprob`, `sampling.sample_given`;
include/talkshow_hip.h, "given rows").  Every test fails on a build without the feature: the helper and the restatement do not exist there.
"""
import ctypes as C

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

F32 = np.float32
V = 256


def _clips():
    """Six clips submitted shuffled: code rows, given rows (None, G = 0, G = H_b among them) and the order of a length sort."""
    rows = [8, 20, 3, 17, 9, 17]
    rng = np.random.default_rng(3)
    G = [8, 9, 0, None, 1, 17]                       # G = H_b, a prefix, an empty array, None, one row, G = H_b again
    given = [None if g is None else rng.integers(0, V, (g, 2)) for g in G]
    order = sorted(range(len(rows)), key=lambda b: (-rows[b], b))
    return rows, G, given, order


def test_block_and_table_follow_the_sort():
    rows, G, given, order = _clips()
    block, table = _lib.given_block(given, rows, V, order)
    assert block.shape == (6, 20, 2) and block.dtype == np.int64 and table.shape == (6,) and table.dtype == np.int32
    for k, i in enumerate(order):
        g = 0 if G[i] is None else G[i]
        assert table[k] == g
        if g:
            np.testing.assert_array_equal(block[k, :g], given[i])
        assert (block[k, g:] == 0).all()
    # without an order: the submitted one; one (B, G, 2) block is B entries of G rows
    block2, table2 = _lib.given_block(given, rows, V)
    for i in range(6):
        np.testing.assert_array_equal(block2[i], block[order.index(i)])
        assert table2[i] == table[order.index(i)]
    one = np.arange(2 * 3 * 2).reshape(2, 3, 2)
    b3, t3 = _lib.given_block(one, [5, 4], V)
    assert b3.shape == (2, 5, 2) and list(t3) == [3, 3] and np.array_equal(b3[:, :3], one) and (b3[:, 3:] == 0).all()
    # the inputs are left as they were, and the results own their memory (a caller may overwrite its arrays right away)
    keep = [None if g is None else g.copy() for g in given]
    for g in given:
        if g is not None:
            g[...] = -5
    for k, i in enumerate(order):
        if keep[i] is not None:
            np.testing.assert_array_equal(block[k, :len(keep[i])], keep[i])


def test_errors_name_the_submitted_clip():
    rows, G, given, order = _clips()

    def bad(i, g, match):
        gv = list(given)
        gv[i] = g
        with pytest.raises(ValueError, match=match):
            _lib.given_block(gv, rows, V, order)
    bad(4, np.zeros((2, 3), np.int64), r"clip 4 must have shape \(G, 2\)")
    bad(1, np.zeros(4, np.int64), r"clip 1 must have shape \(G, 2\)")
    bad(2, np.zeros((4, 2), np.int64), r"clip 2 brings 4 given rows but has 3 code rows")
    bad(5, np.asarray([[0, 1], [V, 2]]), rf"clip 5 hold the code {V}, outside \[0, {V}\)")
    bad(0, np.asarray([[0, -1]]), r"clip 0 hold the code -1, outside")
    bad(3, np.asarray([[0, 2 ** 40]]), r"clip 3 hold the code 1099511627776, outside")
    bad(3, np.zeros((2, 2), np.float32), r"clip 3 must be integers")
    with pytest.raises(ValueError, match="one entry per clip"):
        _lib.given_block(given[:-1], rows, V, order)
    with pytest.raises(ValueError, match=r"\(B=6, G, 2\)"):
        _lib.given_block(np.zeros((5, 2, 2), np.int64), rows, V, order)
    with pytest.raises(ValueError, match="permutation"):
        _lib.given_block(given, rows, V, [0, 0, 1, 2, 3, 4])


def test_the_c_table_rule():
    """`ts_given_rows_check`: G_b < 0 or G_b > lens[b] / 4 is an error that names the clip; host only."""
    lib = _lib.load()
    i32p = C.POINTER(C.c_int32)
    lens = np.asarray([83, 70, 16, 7], np.int32)          # 20, 17, 4, 1 code rows

    def rc(tab):
        t = np.asarray(tab, np.int32)
        return lib.ts_given_rows_check(t.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), len(tab))
    assert rc([20, 0, 4, 1]) == 0 and rc([0, 0, 0, 0]) == 0
    assert rc([20, 18, 0, 0]) != 0 and "clip 1" in lib.ts_last_error().decode()
    assert rc([0, 0, 0, -1]) != 0 and "clip 3" in lib.ts_last_error().decode()
    assert rc([21, 0, 0, 0]) != 0 and "clip 0" in lib.ts_last_error().decode()


def test_restatement_forced_rows():
    rng = np.random.default_rng(9)
    B = 5
    logits = (rng.standard_normal((B, V)) * 3).astype(F32)
    u = rng.random(B).astype(F32)
    forced = [1, 0, 1, 0, 0]
    recs = [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.0, 1.0, 1), (1.7, 0.3, 12), (1.0, 1.0, 0)]
    top = np.argsort(-logits, axis=1)
    given = np.asarray([top[0, 0], 2 ** 40, top[2, 1], -7, 0], np.int64)          # row 2: top_k = 1 and NOT the argmax
    # without a record
    idx, lp = S.sample_given(logits, u, forced, given)
    ref = [S.draw(logits[b], u[b], 1.0, np.ones(V, bool)) for b in range(B)]
    for b in range(B):
        if forced[b]:
            assert idx[b] == given[b] and lp[b] == S.logprob(logits[b], given[b]) and np.isfinite(lp[b])
        else:
            assert idx[b] == ref[b] and lp[b] == S.logprob(logits[b], ref[b])
    gidx, glp = S.sample_given(logits, u, forced, given, greedy=True)
    assert [gidx[b] for b in (1, 3, 4)] == [top[b, 0] for b in (1, 3, 4)] and gidx[0] == given[0] and glp[0] == lp[0]
    # with records: a kept code gets the bits a draw of it gets, a removed one -inf
    idx, lp = S.sample_given(logits, u, forced, given, recs)
    want_idx, kept = S.sample_ctl(logits, u, recs)
    assert kept[0, given[0]] and lp[0] == S.logprob(logits[0], given[0], recs[0]) and idx[0] == given[0]
    assert not kept[2, given[2]] and lp[2] == -np.inf and idx[2] == given[2]
    for b in (1, 3, 4):
        assert idx[b] == want_idx[b] and lp[b] == S.logprob(logits[b], want_idx[b], recs[b])
    assert lp[1] == 0.0                                   # top_k = 1, drawn
    assert S.given_logprob(logits[2], top[2, 0], recs[2]) == 0.0          # top_k = 1, given the argmax: 0; anything else: -inf
    assert all(S.given_logprob(logits[2], c, recs[2]) == -np.inf for c in top[2, 1:6])
    assert np.isnan(S.given_logprob(logits[0], V)) and np.isnan(S.given_logprob(logits[0], -1, recs[0]))
    # a neutral record keeps everything: the value without a table
    for c in (0, 17, V - 1):
        assert S.given_logprob(logits[4], c, (1.0, 1.0, 0)) == S.logprob(logits[4], c)
