"""Per-clip sampling controls, host side (no GPU): `ts_sampling_check`, the numpy twin `talkshow_amd/sampling.py` against the oracle's
sampler and against an independent float64 definition of the kept set, and the records' way through the length sort.

The float64 comparison of the top-p boundary is made where it can be decided: `p` is constructed per row as the midpoint between two
consecutive float64 cumulative masses at a rank whose own probability is at least 1e-3, so the boundary lies at least 5e-4 of the mass
away from `p` — above the error of the twin's masses (fp32 weights: at most about 2e-5 relative each from the scaled exponent; their
integer quantisation floor(w 2^31): < 2048 * 2^-31 = 9.6e-7 in total, far inside the 2048 * 2^-24 = 1.2e-4 an fp32 accumulation would
be allowed).  The distance is asserted first, on the float64 side alone; no row is left out.  Top-k is compared on every row, ties
included: the ranking is exact.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S

F32 = np.float32
U_LAST = F32(1.0) - F32(2.0 ** -24)


@pytest.fixture(scope="module")
def lib():
    from talkshow_amd import _lib
    return _lib, _lib.load()


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, r in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = r
    return arr


# ---- 1. validation -----------------------------------------------------------------------------------------------------------------
BAD = [((0.0, 1.0, 0, 0), "temperature"), ((-1.0, 1.0, 0, 0), "temperature"), ((float("nan"), 1.0, 0, 0), "temperature"),
       ((float("inf"), 1.0, 0, 0), "temperature"), ((1e-39, 1.0, 0, 0), "temperature"),          # a subnormal T: 1 / T overflows fp32
       ((1.0, 0.0, 0, 0), "top_p"), ((1.0, -0.5, 0, 0), "top_p"), ((1.0, 1.0000001, 0, 0), "top_p"), ((1.0, float("nan"), 0, 0), "top_p"),
       ((1.0, 1.0, -1, 0), "top_k"), ((1.0, 1.0, 0, 1), "reserved")]


@pytest.mark.parametrize("rec,word", BAD, ids=[f"{w}{i}" for i, (_, w) in enumerate(BAD)])
def test_check_rejects_and_names_the_clip(lib, rec, word):
    _lib, L = lib
    neutral = (1.0, 1.0, 0, 0)
    for slot in (0, 3):
        recs = [neutral] * 5
        recs[slot] = rec
        assert L.ts_sampling_check(_table(_lib, recs), 5, 2048) != 0
        msg = L.ts_last_error().decode()
        assert f"clip {slot}" in msg and word in msg, msg


def test_check_accepts(lib):
    _lib, L = lib
    ok = [(1.0, 1.0, 0, 0), (1.0, 1.0, 2048, 0), (1.0, 1.0, 5000, 0), (0.5, 1e-6, 1, 0), (4.0, 0.999, 64, 0), (1e-38, 1.0, 0, 0)]
    assert L.ts_sampling_check(_table(_lib, ok), len(ok), 2048) == 0, L.ts_last_error().decode()
    assert L.ts_sampling_check(None, 1, 2048) != 0


def test_python_table_helper(lib):
    _lib, _ = lib
    assert _lib.sampling_records(None, 3) == [(1.0, 1.0, 0)] * 3
    assert _lib.sampling_records({"temperature": 0.8}, 2) == [(0.8, 1.0, 0)] * 2
    assert _lib.sampling_records((0.9, 0.95, 64), 2) == [(0.9, 0.95, 64)] * 2
    assert _lib.sampling_records([None, {"top_k": 1}, (2.0, 0.5, 0)], 3) == [(1.0, 1.0, 0), (1.0, 1.0, 1), (2.0, 0.5, 0)]
    arr, n = _lib.sampling_table([None, {"top_p": 0.5, "top_k": 7}], 2)
    assert n == 2 and (arr[1].temperature, arr[1].top_p, arr[1].top_k, arr[1].reserved) == (1.0, 0.5, 7, 0)
    with pytest.raises(ValueError, match="clip 1"):
        _lib.sampling_table([None, {"temperature": -1.0}, None], 3)
    with pytest.raises(ValueError, match="one per clip"):
        _lib.sampling_table([None, None], 3)
    with pytest.raises(ValueError, match="unknown keys"):
        _lib.sampling_table({"temp": 1.0}, 1)
    with pytest.raises(ValueError, match="top_k = 1"):
        _lib.sampling_table(None, 2, mode=_lib.TS_SAMPLE_GREEDY)


def test_single_record_is_a_tuple_not_a_list(lib):
    _lib, _ = lib
    for n in (3, 5):                                            # [T, p, k] is not one record, whatever the clip count
        with pytest.raises(ValueError, match="one record per clip; write one record for all clips as a tuple"):
            _lib.sampling_records([0.9, 0.95, 64], n)
    with pytest.raises(ValueError, match="a tuple"):
        _lib.sampling_record([0.9, 0.95, 64])
    with pytest.raises(ValueError):
        _lib.sampling_records("0.9", 1)


def test_vocabulary_limit(lib):
    """The device holds a row's integer mass in 44 bits: V * 2^31 < 2^44, so V <= 8191; beyond it every entry refuses, on the host."""
    _lib, L = lib
    ok = _table(_lib, [(1.0, 1.0, 0, 0)])
    assert L.ts_sampling_check(ok, 1, 8191) == 0
    for V in (8192, 65536, 1 << 20):
        assert L.ts_sampling_check(ok, 1, V) != 0
        assert "8191" in L.ts_last_error().decode()
    with pytest.raises(ValueError, match="8191"):
        _lib.sampling_table(None, 2, V=8192)


def test_infer_on_audio_refuses_controls_it_cannot_honour():
    """`infer_on_audio(temperature=, top_k=, top_p=)`: with continuity=True (the streaming session takes no controls yet), with greedy=True,
    and with a bad record, a ValueError before the audio is read (the file named here does not exist) and before any device is touched."""
    import argparse
    import types
    from nets.smplx_body_pixel import TrainWrapper
    me = types.SimpleNamespace(args=argparse.Namespace(infer=True), generator=types.SimpleNamespace(input_dim=2048))
    with pytest.raises(ValueError, match="streaming session"):
        TrainWrapper.infer_on_audio(me, "no_such_file.wav", continuity=True, temperature=0.8)
    with pytest.raises(ValueError, match="streaming session"):
        TrainWrapper.infer_on_audio(me, "no_such_file.wav", continuity=True, top_k=5)
    with pytest.raises(ValueError, match="greedy"):
        TrainWrapper.infer_on_audio(me, "no_such_file.wav", greedy=True, top_p=0.9)
    with pytest.raises(ValueError, match="clip 0"):
        TrainWrapper.infer_on_audio(me, "no_such_file.wav", temperature=-1.0)


# ---- 2. the twin's exponential and its neutral draw ---------------------------------------------------------------------------------
def test_det_expf_copy_equals_the_oracles():
    x = np.concatenate([np.linspace(-100.0, 0.0, 100000 - 3), [-86.0, -86.00001, -0.0]]).astype(F32)
    assert x.size == 100000
    a, b = S.det_expf(x), O.det_expf(x)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("V", [2048, 300, 100])
def test_neutral_twin_equals_the_oracle_sampler(golden, V):
    rng = np.random.default_rng(V)
    real = golden("pix_full")["step_logits"][1, 7, 1][:V]
    rows = np.stack([real, rng.standard_normal(V).astype(F32), (5 * rng.standard_normal(V)).astype(F32), np.zeros(V, F32)])
    us = np.asarray([0.0, U_LAST, 0.5, 0.999999], F32)
    for u in us:
        uu = np.full(len(rows), u, F32)
        idx, kept = S.sample_ctl(rows, uu, (1.0, 1.0, 0))
        assert kept.all()
        np.testing.assert_array_equal(idx, O.sample_inverse_cdf(rows, uu))
    uu = rng.random(len(rows)).astype(F32)
    np.testing.assert_array_equal(S.sample_ctl(rows, uu, [(1.0, 1.0, V + 5)] * len(rows))[0], O.sample_inverse_cdf(rows, uu))


# ---- 3. the kept set against a float64 definition -----------------------------------------------------------------------------------
def ranks64(row):
    l = np.asarray(row, np.float64)
    return np.lexsort((np.arange(l.size), -l))


def probs64(row, T):
    z = np.asarray(row, np.float64) / float(T)
    p = np.exp(z - z.max())
    return p / p.sum()


def keep64(row, T, k, p):
    """The rule in float64: z = l / T, softmax, the same ranking; top-k, then top-p on the mass top-k kept."""
    V = len(row)
    order = ranks64(row)
    pr = probs64(row, T)[order]
    n_k = k if 1 <= k < V else V
    keep = np.arange(V) < n_k
    if p < 1:
        M = np.concatenate([[0.0], np.cumsum(pr)[:-1]])
        keep &= (np.arange(V) == 0) | (M < float(p) * pr[:n_k].sum())
    out = np.zeros(V, bool)
    out[order[keep]] = True
    return out


def boundary_p(row, T, k):
    """p as fp32, halfway between two consecutive float64 cumulative masses (of the mass top-k kept) at the LAST rank whose own share is
    at least 1e-3 (1.001e-3, so that rounding p to fp32 cannot bring the distance under 5e-4) -> (p, distance to the nearer boundary)."""
    V = len(row)
    pr = probs64(row, T)[ranks64(row)]
    n_k = k if 1 <= k < V else V
    share = pr[:n_k] / pr[:n_k].sum()
    c = np.concatenate([[0.0], np.cumsum(share)])
    cand = np.flatnonzero(share >= 1.001e-3)
    assert cand.size, "no rank of this row carries 1e-3 of the mass"
    r = int(cand[-1])
    p = F32(0.5 * (c[r] + c[r + 1]))
    return p, float(min(float(p) - c[r], c[r + 1] - float(p))), r


def float64_cases(golden):
    """(name, row, (T, p, k)) for the float64 comparison: the real peaked row at three temperatures, seeded normal rows of width 1 and 5;
    top-k off and on.  tests/test_gpu_sampling_ops.py imports this constructor and compares the DEVICE's kept set on the same cases."""
    real = np.ascontiguousarray(golden("pix_full")["step_logits"][1, 7, 1])
    rng = np.random.default_rng(2048)
    rows = [("real/T0.5", real, 0.5), ("real/T1", real, 1.0), ("real/T4", real, 4.0),
            ("normal1", rng.standard_normal(2048).astype(F32), 1.0), ("normal5", (5 * rng.standard_normal(2048)).astype(F32), 1.0)]
    out = []
    for name, row, T in rows:
        for k in (0, 200):
            p, dist, r = boundary_p(row, T, k)
            out.append((f"{name}/k{k}", row, (float(T), float(p), k), dist, r))
    return out


def test_kept_set_against_float64(golden):
    cases = float64_cases(golden)
    assert len(cases) == 10
    for name, row, rec, dist, r in cases:
        assert dist >= 5e-4, f"{name}: p lies {dist:.2e} of the mass from the boundary"          # first, on the float64 side alone
    for name, row, rec, dist, r in cases:
        T, p, k = rec
        want = keep64(row, T, k, p)
        got = S.keep_mask(row, rec)
        assert want.sum() == r + 1
        assert np.array_equal(got, want), f"{name}: kept sets differ at {np.flatnonzero(got != want)[:8]}"


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
def test_top_k_against_float64_ties_included(golden, T):
    rng = np.random.default_rng(7)
    real = np.ascontiguousarray(golden("pix_full")["step_logits"][1, 7, 1])
    tied = rng.integers(0, 6, 2048).astype(F32)              # blocks of equal logits straddle every k
    small = rng.integers(0, 3, 100).astype(F32)
    for row in (real, tied, small, np.zeros(300, F32), rng.standard_normal(5).astype(F32), np.asarray([2.0], F32)):
        V = row.size
        for k in (0, 1, 2, 5, 7, 64, V - 1, V, V + 5):
            got = S.keep_mask(row, (T, 1.0, k))
            assert np.array_equal(got, keep64(row, T, k, 1.0)), (V, k)
            assert got.sum() == (k if 1 <= k < V else V)
    assert np.array_equal(np.flatnonzero(S.keep_mask(np.zeros(300, F32), (T, 1.0, 5))), np.arange(5))     # all equal: the lowest indices


def test_extremes_on_the_twin(golden):
    real = np.ascontiguousarray(golden("pix_full")["step_logits"][1, 7, 1])
    tied = np.zeros(300, F32)
    tied[[40, 7, 200]] = 3.0
    for row in (real, tied):
        for rec in ((1.0, 1.0, 1), (1.7, 1e-6, 0), (0.5, 1e-6, 1)):
            for u in (0.0, 0.3, U_LAST):
                idx, kept = S.sample_ctl(row[None], np.asarray([u], F32), rec)
                assert idx[0] == int(np.argmax(row)) and kept.sum() == 1 and kept[0, idx[0]]
    row = np.asarray([1.0, -np.inf, 0.5, -np.inf, -0.0, 0.0], F32)                                            # -inf: never drawn, kept only if k reaches it
    assert np.array_equal(S.keep_mask(row, (1.0, 1.0, 3)), [True, False, True, False, True, False])           # -0 ties with +0: index order
    assert np.array_equal(S.keep_mask(row, (1.0, 1.0, 5)), [True, True, True, False, True, True])
    for u in (0.0, 0.5, U_LAST):
        assert S.sample_ctl(row[None], np.asarray([u], F32), (1.0, 1.0, 0))[0][0] in (0, 2, 4, 5)


# ---- 4. the records follow the clips through the sort --------------------------------------------------------------------------------
def test_records_follow_the_sort_and_back(lib):
    _lib, _ = lib
    from nets.smplx_body_pixel import mixed_pass_order
    lens = [12, 80, 33, 80, 70, 12]
    recs = _lib.sampling_records([None, (0.5, 1.0, 0), {"top_k": 1}, (2.0, 0.9, 0), {"top_p": 0.3}, (1.0, 1.0, 7)], 6)
    order, inverse = mixed_pass_order(lens)
    assert order == [1, 3, 4, 2, 0, 5]
    srt = [recs[i] for i in order]                            # what generate_clips hands to the C entry: slot k = submitted clip order[k]
    assert srt == [(0.5, 1.0, 0), (2.0, 0.9, 0), (1.0, 0.3, 0), (1.0, 1.0, 1), (1.0, 1.0, 0), (1.0, 1.0, 7)]
    assert [srt[inverse[b]] for b in range(6)] == recs        # and back
    arr, n = _lib.sampling_table(srt, 6)
    assert [(round(a.temperature, 6), round(a.top_p, 6), a.top_k) for a in arr] == [(round(F32(t).item(), 6), round(F32(p).item(), 6), k)
                                                                                      for t, p, k in srt]
