"""Code bias on the host (include/talkshow_hip.h, "code bias"): `_lib.code_bias_block` and its refusals, `ts_code_bias_check`, the numpy
twin of step 0 and of the kept-set sentence (`sampling.biased`, `keep_mask_bias`, `sample_bias`), `allow_bias` / `ban_bias`.  No GPU.
The grid of `test_twin_never_returns_a_banned_token` is also run through the UNMODIFIED `sampling.draw` with every token kept: that
must return a banned token at least once, which is what makes the kept-set sentence necessary."""
import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

F32 = np.float32
U_LAST = F32(1.0 - 2.0 ** -24)
NEUTRAL = (1.0, 1.0, 0)
VS = [2048, 300]


def regime_rows(golden, V):
    """The five rows of tests/test_gpu_sampling_ops.py::regime_rows, rebuilt here: the peaked real row, a flat row, an all-equal row,
    blocks of ties, a row with -inf entries."""
    rng = np.random.default_rng(100 + V)
    real = golden("pix_full")["step_logits"][1, 7, 1][:V]
    flat = (0.01 * rng.standard_normal(V)).astype(F32)
    ties = rng.integers(0, 5, V).astype(F32)
    minf = rng.standard_normal(V).astype(F32)
    minf[rng.random(V) < 0.3] = -np.inf
    minf[V // 2] = 1.5
    return np.ascontiguousarray(np.stack([real, flat, np.zeros(V, F32), ties, minf]), F32)


def ban_patterns(V):
    """Two ban rows: 60 % of the tokens and the last five indices; the last token of every thread's chunk and the last two chunks whole.
    Index V // 2 stays allowed (the -inf regime row has its one sure finite logit there)."""
    rng = np.random.default_rng(7 + V)
    chunk = (V + 255) // 256
    a = np.zeros(V, F32)
    a[rng.random(V) < 0.6] = -np.inf
    a[-5:] = -np.inf
    b = np.zeros(V, F32)
    b[chunk - 1::chunk] = -np.inf
    b[-2 * chunk:] = -np.inf
    for t in (a, b):
        t[V // 2] = 0.0
        t[1] = F32(0.75)                 # and one finite, non-zero bias
    return [a, b]


def grid(V):
    return [NEUTRAL, (0.5, 1.0, 0), (1.7, 0.9, 0), (1.0, 1.0, 7), (4.0, 0.999, 64), (1.0, 0.3, V - 1)]


def test_twin_never_returns_a_banned_token(golden):
    """360 draws: 2 vocabularies x 2 ban rows x 5 row regimes x 6 records x u in {0, 1 - 2^-24, random}."""
    banned_by_plain_draw = n = 0
    for V in VS:
        rows = regime_rows(golden, V)
        rng = np.random.default_rng(V)
        for bias in ban_patterns(V):
            for b in range(rows.shape[0]):
                lb = S.biased(rows[b], bias)
                allowed = lb != F32(-np.inf)
                assert allowed.any()
                for rec in grid(V):
                    kept = S.keep_mask_bias(rows[b], rec, bias)
                    assert kept.any() and not kept[~allowed].any()
                    assert np.array_equal(kept, S.keep_mask(lb, rec) & allowed)
                    for u in (F32(0.0), U_LAST, F32(rng.random())):
                        c = S.draw(lb, u, rec[0], kept)
                        assert allowed[c] and kept[c], f"V {V} row {b} record {rec} u {u}: drew banned token {c}"
                        n += 1
                        # the same draw through the unmodified `draw` with every token "kept"
                        banned_by_plain_draw += int(not allowed[S.draw(lb, u, rec[0], np.ones(V, bool))])
    assert n == 360
    print(f"\nthe unmodified draw with everything kept returned a banned token in {banned_by_plain_draw} of {n} draws")
    assert banned_by_plain_draw >= 1, "the kept-set sentence would do nothing"


@pytest.mark.parametrize("V", VS)
def test_logprob_against_float64(golden, V):
    rows = regime_rows(golden, V)
    rng = np.random.default_rng(V + 3)
    worst = 0.0
    for bias in ban_patterns(V) + [rng.standard_normal(V).astype(F32)]:
        for b in range(rows.shape[0]):
            lb = S.biased(rows[b], bias)
            u = rng.random(3).astype(F32)
            idx, kept, lp = S.sample_bias(np.tile(rows[b], (3, 1)), u, None, bias[None, None, :].repeat(2, 1), [0, 0, 0], 1)
            x = rows[b].astype(np.float64) + bias.astype(np.float64)      # l + b exactly; step 0's one rounding is part of what is bounded
            with np.errstate(divide="ignore"):
                ref = x - x.max() - np.log(np.exp(x - x.max()).sum())
            for i in range(3):
                c = int(idx[i])
                err = abs(float(lp[i]) - ref[c])
                bound = S.logprob_error_bound(V, lb[c] - lb.max(), lp[i])
                worst = max(worst, err / bound)
                assert err <= bound, f"V {V} row {b} code {c}: |{lp[i]} - {ref[c]}| = {err} > {bound}"
                assert lp[i] == S.logprob(lb, c, NEUTRAL)
    print(f"\nV {V}: worst error / bound = {worst:.3f}")


def test_no_table_and_zero_table():
    rng = np.random.default_rng(5)
    row = rng.standard_normal(300).astype(F32)
    row[3] = F32(-0.0)
    assert S.biased(row, None) is not None and np.array_equal(S.biased(row, None).view(np.uint32), row.view(np.uint32))
    z = S.biased(row, np.zeros(300, F32))
    assert np.array_equal(z, row) and not np.signbit(z[3])               # -0 + 0 = +0: equal, the sign of a zero apart
    for rec in (NEUTRAL, (0.7, 0.9, 5)):
        assert np.array_equal(S.keep_mask_bias(row, rec, None), S.keep_mask(row, rec))
        assert np.array_equal(S.keep_mask_bias(row, rec, np.zeros(300, F32)), S.keep_mask(row, rec))
    u = rng.random(4).astype(F32)
    rows = np.tile(row, (4, 1))
    a = S.sample_bias(rows, u, (0.7, 0.9, 5), np.zeros((1, 2, 300), F32), [-1, 0, -1, 0], 0)
    b = S.sample_ctl(rows, u, (0.7, 0.9, 5))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_given_code_under_a_ban():
    row = np.linspace(-1, 1, 100).astype(F32)
    bias = np.zeros(100, F32)
    bias[40] = -np.inf
    assert S.given_logprob_bias(row, 40, None, bias) == -np.inf
    assert S.given_logprob_bias(row, 40, (1.0, 0.9, 0), bias) == -np.inf
    assert S.given_logprob_bias(row, 41, None, bias) == S.logprob(S.biased(row, bias), 41, NEUTRAL)
    assert np.isnan(S.given_logprob_bias(row, 100, None, bias))
    assert S.given_logprob_bias(row, 40, None, None) == S.given_logprob(row, 40, None)
    one = np.full(100, -np.inf, F32)
    one[17] = 3.0
    assert S.given_logprob_bias(row, 17, None, one) == 0.0              # an allow-list of one token: probability 1


def test_allow_and_ban_round_trips():
    V = 64
    codes = np.array([[3, 9], [3, 10], [5, 9], [-1, -1]])
    a, b = S.allow_bias(codes, V), S.ban_bias(codes, V)
    assert a.shape == b.shape == (2, V) and a.dtype == b.dtype == F32
    assert sorted(np.flatnonzero(a[0] == 0)) == [3, 5] and sorted(np.flatnonzero(a[1] == 0)) == [9, 10]
    assert np.array_equal(np.isinf(a), ~np.isinf(b)) and (a[np.isfinite(a)] == 0).all() and (b[np.isfinite(b)] == 0).all()
    assert (a[np.isinf(a)] < 0).all() and (b[np.isinf(b)] < 0).all()
    a2 = S.allow_bias(([3, 5], [9, 10]), V)
    assert np.array_equal(a, a2)
    back = np.stack(np.meshgrid(np.flatnonzero(a[0] == 0), np.flatnonzero(a[1] == 0)), -1).reshape(-1, 2)
    assert np.array_equal(S.allow_bias(back, V), a)                      # table -> codes -> table
    assert np.array_equal(S.ban_bias(([], []), V), np.zeros((2, V), F32))
    with pytest.raises(ValueError):
        S.allow_bias(([3], []), V)
    with pytest.raises(ValueError):
        S.allow_bias(np.array([[3, V]]), V)
    with pytest.raises(ValueError):
        S.ban_bias((list(range(V)), [1]), V)
    with pytest.raises(ValueError):
        S.allow_bias(np.zeros((3, 2), F32), V)


def test_block_layout_and_sharing():
    V = 32
    t = S.allow_bias(([1, 2], [3]), V)
    u = S.ban_bias(([1], [3]), V)
    assert _lib.code_bias_block(None, 3, V) == (None, None)
    assert _lib.code_bias_block([None, None, None], 3, V) == (None, None)
    tab, idx = _lib.code_bias_block(t, 3, V)                               # one table for all: NB = 1
    assert tab.shape == (1, 2, V) and tab.dtype == F32 and idx.dtype == np.int32 and list(idx) == [0, 0, 0]
    tab, idx = _lib.code_bias_block([t, None, t, u], 4, V)                 # shared by identity
    assert tab.shape == (2, 2, V) and list(idx) == [0, -1, 0, 1]
    assert np.array_equal(tab[0], t) and np.array_equal(tab[1], u)
    tab, idx = _lib.code_bias_block([t, None, t.copy(), u], 4, V)          # an equal COPY is another table
    assert tab.shape == (3, 2, V) and list(idx) == [0, -1, 1, 2]
    tab, idx = _lib.code_bias_block([t, None, t, u], 4, V, order=[3, 1, 0, 2])      # slot k holds submitted clip order[k]
    assert list(idx) == [1, -1, 0, 0] and np.array_equal(tab[0], t)
    body = np.linspace(-2, 2, V).astype(F32)
    tab, idx = _lib.code_bias_block([{"body": body}, {"hand": body, "body": None}], 2, V)
    assert np.array_equal(tab[0, 0], body) and (tab[0, 1] == 0).all() and (tab[1, 0] == 0).all() and np.array_equal(tab[1, 1], body)
    lib = _lib.load()
    assert lib.ts_code_bias_index_check(idx.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 2, 2) == 0
    bad = np.array([0, 2], np.int32)
    assert lib.ts_code_bias_index_check(bad.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 2, 2) != 0 and "clip 1" in lib.ts_last_error().decode()
    assert lib.ts_code_bias_index_check(idx.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 2, 3) != 0      # more tables than clips


def _bad_tables(V):
    good = np.zeros((2, V), F32)

    def with_(j, v, x):
        t = good.copy()
        t[j, v] = x
        return t
    allb = good.copy()
    allb[1] = -np.inf
    return {
        "shape": (np.zeros((2, V + 1), F32), "(2, "),
        "one_row": (np.zeros(V, F32), "(2, "),
        "strings": (np.full((2, V), "x"), "numbers"),
        "nan": (with_(0, 5, np.nan), "NaN"),
        "plus_inf": (with_(1, 7, np.inf), "+inf"),
        "too_large": (with_(0, 2, 2e30), "1e30"),
        "too_small": (with_(1, 2, -2e30), "1e30"),
        "all_banned": (allb, "hand column"),
        "dict_key": ({"legs": np.zeros(V, F32)}, "keys"),
        "dict_row": ({"hand": np.zeros(V - 1, F32)}, "'hand' row"),
        "dict_nan": ({"body": with_(0, 5, np.nan)[0]}, "body column"),
    }


@pytest.mark.parametrize("case", sorted(_bad_tables(8)))
def test_block_refusals_name_the_clip(case):
    V = 48
    bad, word = _bad_tables(V)[case]
    good = np.zeros((2, V), F32)
    with pytest.raises(ValueError) as e:
        _lib.code_bias_block([good, None, bad], 3, V, order=[2, 0, 1], who="generate_clips")
    assert "clip 2" in str(e.value) and word in str(e.value) and "generate_clips" in str(e.value), str(e.value)


def test_block_refusals_of_the_call():
    V = 16
    good = np.zeros((2, V), F32)
    with pytest.raises(ValueError):
        _lib.code_bias_block([good, good], 3, V)                           # one entry per clip
    with pytest.raises(ValueError):
        _lib.code_bias_block("body", 3, V)
    with pytest.raises(ValueError):
        _lib.code_bias_block([good] * 3, 3, V, order=[0, 0, 1])
    for mode in (_lib.TS_SAMPLE_GREEDY, _lib.TS_TEACHER_FORCED):
        with pytest.raises(ValueError) as e:
            _lib.code_bias_block(good, 3, V, mode=mode)
        assert "top_k = 1" in str(e.value)
    for mode in (_lib.TS_SAMPLE_UNIFORMS, _lib.TS_SAMPLE_PHILOX):
        assert _lib.code_bias_block(good, 3, V, mode=mode)[0].shape == (1, 2, V)
    with pytest.raises(ValueError):
        _lib.code_bias_block(np.zeros((2, 8192), F32), 1, 8192)            # the controls' vocabulary limit
    assert _lib.code_bias_block(np.zeros((2, 8191), F32), 1, 8191)[0].shape == (1, 2, 8191)


def test_check_names_table_and_column():
    lib, V = _lib.load(), 20
    t = np.zeros((3, 2, V), F32)
    t[1, 0, 4] = -np.inf
    t[2, 1, :] = -np.inf
    t[2, 1, 3] = 1e30
    fp = _lib.C.POINTER(_lib.C.c_float)
    assert lib.ts_code_bias_check(t.ctypes.data_as(fp), 3, V) == 0
    t[2, 1, 3] = -np.inf
    assert lib.ts_code_bias_check(t.ctypes.data_as(fp), 3, V) != 0
    msg = lib.ts_last_error().decode()
    assert "table 2" in msg and "hand" in msg, msg
    assert lib.ts_code_bias_check(t.ctypes.data_as(fp), 2, V) == 0
    t[1, 0, 9] = np.nan
    assert lib.ts_code_bias_check(t.ctypes.data_as(fp), 3, V) != 0
    msg = lib.ts_last_error().decode()
    assert "table 1" in msg and "body" in msg and "code 9" in msg, msg
