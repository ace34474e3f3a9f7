"""Repetition penalty, host side (no GPU): what `ts_repeat_check` and `_lib.repeat_table` refuse, and the numpy twin of the rule
(`sampling.repeat_counts`, `sampling.penalised`; include/talkshow_hip.h, "repetition penalty").  The twin is what the GPU tests compare the
device with, so its own arithmetic is pinned here by hand-made cases."""
import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

F32 = np.float32
V = 300


def _check(records, n=None, v=V):
    arr = (_lib.TsRepeat * len(records))()
    for b, r in enumerate(records):
        arr[b].window, arr[b].presence, arr[b].frequency, arr[b].reserved = r
    rc = _lib.load().ts_repeat_check(arr, len(records) if n is None else n, v)
    return rc, _lib.load().ts_last_error().decode()


GOOD = (5, 0.5, 0.25, 0)
BAD = [((-1, 0.0, 0.0, 0), "window"), ((65, 0.0, 0.0, 0), "window"), ((3, float("nan"), 0.0, 0), "presence"),
       ((3, 0.0, float("nan"), 0), "frequency"), ((3, float("inf"), 0.0, 0), "presence"), ((3, 0.0, float("-inf"), 0), "frequency"),
       ((3, 1.5e30, 0.0, 0), "presence"), ((3, 0.0, -1.5e30, 0), "frequency"), ((3, 0.0, 0.0, 1), "reserved")]


def test_check_accepts_the_documented_range():
    ok = [(0, 0.0, 0.0, 0), (64, 1e30, -1e30, 0), (1, -1e30, 1e30, 0), (0, 7.0, -3.0, 0), GOOD]
    rc, msg = _check(ok)
    assert rc == 0, msg


@pytest.mark.parametrize("bad, word", BAD)
def test_check_refuses_and_names_the_clip(bad, word):
    for where in (0, 2):
        recs = [GOOD] * 3
        recs[where] = bad
        rc, msg = _check(recs)
        assert rc != 0 and f"clip {where}" in msg and word in msg, msg


def test_check_refuses_bad_arguments():
    assert _check([GOOD], n=0)[0] != 0
    assert _check([GOOD], v=0)[0] != 0
    assert _check([GOOD], v=8192)[0] != 0
    assert _lib.load().ts_repeat_check(None, 1, V) != 0


@pytest.mark.parametrize("bad, word", [b for b in BAD if b[0][3] == 0])
def test_normaliser_refuses_and_names_the_submitted_clip(bad, word):
    order = [2, 0, 1]                                                      # slot k holds submitted clip order[k]
    recs = [GOOD[:3], GOOD[:3], bad[:3]]
    with pytest.raises(ValueError, match="clip 2") as e:
        _lib.repeat_table(recs, 3, V, order, who="t")
    assert word in str(e.value)
    with pytest.raises(ValueError, match="clip 0"):
        _lib.repeat_table(bad[:3], 3, V, order, who="t")                   # one record for all: the first clip is named


def test_normaliser_shapes():
    with pytest.raises(ValueError, match="one per clip"):
        _lib.repeat_table([GOOD[:3]] * 2, 3, V)                            # a list of the wrong length
    with pytest.raises(ValueError, match="tuple"):
        _lib.repeat_table([5, 0.5, 0.25], 3, V)                            # a single record is never a list
    with pytest.raises(ValueError):
        _lib.repeat_table("often", 3, V)
    with pytest.raises(ValueError, match="clip 1"):
        _lib.repeat_table([None, {"windows": 3}, None], 3, V)
    for window in (2.5, float("inf"), float("nan"), "16", None, True):       # every one a ValueError that names the clip
        with pytest.raises(ValueError, match="clip 1.*whole number"):
            _lib.repeat_table([None, (window, 0.0, 0.0), None], 3, V)
    with pytest.raises(ValueError, match="clip 1.*numbers"):
        _lib.repeat_table([None, (3, "much", 0.0), None], 3, V)
    for mode in (_lib.TS_SAMPLE_GREEDY, _lib.TS_TEACHER_FORCED):           # a record together with a mode that draws nothing
        with pytest.raises(ValueError, match="TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX"):
            _lib.repeat_table(GOOD[:3], 3, V, mode=mode)
    assert _lib.repeat_table(None, 3, V, mode=_lib.TS_SAMPLE_GREEDY) == (None, 0)
    arr, n = _lib.repeat_table([None, {"window": 7, "presence": 2.0}, (64, -0.5, 0.125)], 3, V, [2, 0, 1], mode=_lib.TS_SAMPLE_PHILOX)
    assert n == 3
    got = [(arr[k].window, arr[k].presence, arr[k].frequency, arr[k].reserved) for k in range(3)]
    assert got == [(64, -0.5, 0.125, 0), (0, 0.0, 0.0, 0), (7, 2.0, 0.0, 0)]           # slot order
    arr, n = _lib.repeat_table((16, 1.0, 0.0), 2, V)
    assert n == 2 and all((arr[k].window, arr[k].presence, arr[k].frequency) == (16, 1.0, 0.0) for k in range(2))


def test_header_and_python_agree_on_the_window():
    assert _lib.TS_REPEAT_MAX_WINDOW == S.REPEAT_MAX_WINDOW == 64
    import ctypes as C
    assert C.sizeof(_lib.TsRepeat) == 16


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------

def test_repeat_counts_by_hand():
    hist = [4, 9, 4, 4, 299, 0, 9]                                         # rows 0 .. 6 of one column: r = 7
    c = S.repeat_counts(hist, V, 10)                                       # r < W: the whole history
    assert c.dtype == np.int32 and c.shape == (V,)
    assert (c[4], c[9], c[299], c[0]) == (3, 2, 1, 1) and c.sum() == 7
    c = S.repeat_counts(hist, V, 7)                                        # r = W
    assert (c[4], c[9], c[299], c[0]) == (3, 2, 1, 1) and c.sum() == 7
    c = S.repeat_counts(hist, V, 4)                                        # r > W: rows 3 .. 6
    assert (c[4], c[9], c[299], c[0]) == (1, 1, 1, 1) and c.sum() == 4
    c = S.repeat_counts(hist, V, 1)                                        # a window of 1: the row before
    assert c[9] == 1 and c.sum() == 1
    assert S.repeat_counts(hist, V, 0).sum() == 0                          # off
    assert S.repeat_counts([], V, 64).sum() == 0                           # row 0: an empty history
    c = S.repeat_counts([17] * 64, V, 64)                                  # one code seen 64 times
    assert c[17] == 64 and c.sum() == 64
    c = S.repeat_counts([3] + [17] * 64, V, 64)                            # the entry 65 rows back is outside every window
    assert c[17] == 64 and c[3] == 0
    c = S.repeat_counts([-1, V, 5, 10 ** 6], V, 64)                        # a given code outside [0, V) matches no token
    assert c[5] == 1 and c.sum() == 1
    for w in (-1, 65):
        with pytest.raises(ValueError):
            S.repeat_counts(hist, V, w)


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_penalised_leaves_unmet_tokens_and_minus_infinity_alone():
    rng = np.random.default_rng(5)
    row = rng.standard_normal(V).astype(F32)
    row[3], row[8], row[11] = F32(-0.0), F32(-np.inf), F32(-np.inf)
    counts = np.zeros(V, np.int32)
    counts[[8, 20, 21]] = [2, 1, 64]
    out = S.penalised(row, counts, (64, 1e30, 1e30))
    assert out.dtype == F32
    unmet = counts == 0
    assert np.array_equal(_bits(out)[unmet], _bits(row)[unmet])            # bit for bit, the -0 and the unmet -inf included
    assert out[8] == -np.inf                                               # a met -inf stays -inf
    assert np.isfinite(out[[20, 21]]).all() and out[21] == F32(F32(row[21]) - F32(F32(1e30) + F32(F32(1e30) * F32(64.0))))
    out = S.penalised(row, counts, (64, -1e30, -1e30))                     # the other sign: finite, too
    assert np.isfinite(out[[20, 21]]).all() and out[8] == -np.inf


def test_penalised_is_three_separately_rounded_operations():
    l, p, f, c = F32(0.16746475), F32(0.64132816), F32(0.8526328), 29
    three = F32(l - F32(p + F32(f * F32(c))))
    got = S.penalised(np.array([l, l], F32), np.array([c, 0]), (5, p, f))
    assert _bits(got)[0] == _bits(three) and _bits(got)[1] == _bits(l)
    exact = F32(np.float64(l) - (np.float64(p) + np.float64(f) * c))       # one rounding at the end
    fma = F32(np.float64(l) - np.float64(F32(np.float64(p) + np.float64(f) * c)))      # product and sum contracted into one fma
    assert _bits(exact) != _bits(three) and _bits(fma) != _bits(three)     # the case tells the three forms apart


def test_zero_penalties_return_the_input_bits():
    rng = np.random.default_rng(6)
    row = rng.standard_normal(V).astype(F32)
    row[::7] = F32(-0.0)
    row[5] = F32(-np.inf)
    row[6] = F32(0.0)
    counts = rng.integers(0, 65, V).astype(np.int32)
    counts[0], counts[5], counts[6] = 64, 3, 1                             # row[0] is a -0 that the window met
    out = S.penalised(row, counts, (64, 0.0, 0.0))
    assert np.array_equal(_bits(out), _bits(row))                          # x - (+0) = x for every x, -0 included


def test_sample_repeat_ring_and_window_zero():
    """The ring bookkeeping of one launch, and a window-0 row against `sample_bias`'s."""
    rng = np.random.default_rng(7)
    B, r = 3, 70
    logits = rng.standard_normal((B, V)).astype(F32)
    u = rng.random(B).astype(F32)
    hist = rng.integers(0, V, (B, 64))
    recs = [(0, 5.0, 5.0), (64, 1e30, 0.0), (3, 0.5, 0.5)]
    idx, kept, lp, ring = S.sample_repeat(logits, u, None, recs, hist, 2 * r + 1, column=1)
    i0, k0, l0 = S.sample_bias(logits, u, None, None, [-1] * B, 1)
    assert idx[0] == i0[0] and np.array_equal(kept[0], k0[0]) and _bits(lp)[0] == _bits(l0)[0]
    for b in range(B):
        want = np.empty(64, np.int64)
        for i in range(64):
            want[(r - 64 + i) & 63] = hist[b, i]
        if recs[b][0] > 0:
            want[r & 63] = idx[b]
        assert np.array_equal(ring[b], want)
    assert idx[1] not in set(hist[1].tolist())                             # "no repeat within 64 rows"
    idx2, _, lp2, ring2 = S.sample_repeat(logits, u, None, recs, hist, 2 * r + 1, column=1, given=[7, V + 3, 9], forced=[True, True, False])
    assert idx2.tolist()[:2] == [7, V + 3] and idx2[2] == idx[2] and np.isnan(lp2[1])
    assert ring2[1, r & 63] == -1 and ring2[0, r & 63] == hist[0, 0]    # an outside code: -1; window 0: row r - 64 stays
