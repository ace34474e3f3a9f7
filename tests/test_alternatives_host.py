"""The rule of "alternatives" (include/talkshow_hip.h) on the host: the numpy restatement (`talkshow_amd/sampling.py::alternatives`)
against its DEFINITION — sort the row, float64 softmax — within `alternatives_error_bound`, its edge cases, `uncertain_keep`, and every
argument check the Python surface makes before any device work.  No GPU; the library is loaded for its host-only rules.
"""
import numpy as np
import pytest

from talkshow_amd import sampling as S

F32 = np.float32
VS = [2048, 2047, 300, 5, 1]
SCALES = [0.01, 1.0, 20.0, 200.0]
TEMPS = [0.5, 1.0, 1.7, 4.0]


def exact(row, T):
    """The definition in float64: (ranking, log-softmax, entropy) of the fp32 row at temperature T (as the fp32 value it is passed as)."""
    z = (row.astype(np.float64) - np.float64(row.max())) / np.float64(F32(T))
    lse = np.log(np.exp(z).sum())
    lp = z - lse
    p = np.exp(lp)
    order = np.lexsort((np.arange(row.size), -(row + F32(0.0)).astype(np.float64)))
    return order, z, lp, float(-(p[p > 0] * lp[p > 0]).sum())


@pytest.mark.parametrize("V", VS)
def test_restatement_from_definition(V):
    rng = np.random.default_rng(40 + V)
    worst = 0.0
    for scale in SCALES:
        for T in TEMPS:
            row = (rng.standard_normal(V) * scale).astype(F32)
            code = int(rng.integers(V))
            got = S.alternatives(row, (T, 0.5, 3), 8, code=code)         # top_p / top_k are not part of the rule
            order, z, lp, H = exact(row, T)
            k = min(8, V)
            assert np.array_equal(got.codes[:k], order[:k]) and (got.codes[k:] == -1).all()
            assert got.rank == int(np.flatnonzero(order == code)[0])
            assert np.isneginf(got.logprobs[k:]).all()
            for j in range(k):
                lb, hb = S.alternatives_error_bound(V, z[order[j]], lp[order[j]], H)
                assert abs(float(got.logprobs[j]) - lp[order[j]]) <= lb, (V, scale, T, j)
            assert abs(float(got.entropy) - H) <= hb, (V, scale, T, float(got.entropy), H, hb)
            worst = max(worst, abs(float(got.entropy) - H))
    print(f"V {V}: worst |entropy - float64| = {worst:.3g}")


@pytest.mark.parametrize("V", [2048, 300, 5])
def test_flat_row(V):
    """Every logit equal: the entropy is log V rounded, the ranking is index order."""
    row = np.full(V, -3.5, F32)
    got = S.alternatives(row, None, 8, code=V - 1)
    assert got.entropy == F32(np.log(np.float64(V)))
    assert np.array_equal(got.codes[:min(8, V)], np.arange(min(8, V))) and got.rank == V - 1
    assert (got.logprobs[:min(8, V)] == F32(-np.log(np.float64(V)))).all()
    assert S.alternatives(row, None, 0, code=3).rank == 3


def test_one_hot_row():
    """One logit at 0 and the rest at -200: every other weight is dropped, S_all = 1, E = 0 and the entropy is exactly 0.0; the
    alternatives behind the first have finite d_j and therefore finite log-probabilities."""
    row = np.full(300, -200.0, F32)
    row[123] = 0.0
    got = S.alternatives(row, None, 3, code=0)
    assert got.entropy == F32(0.0) and not np.signbit(got.entropy)
    assert list(got.codes) == [123, 0, 1] and got.rank == 1
    assert got.logprobs[0] == F32(0.0) and got.logprobs[1] == F32(-200.0) and np.isfinite(got.logprobs).all()


def test_banned_token_takes_no_part():
    rng = np.random.default_rng(3)
    row = rng.standard_normal(300).astype(F32)
    top = int(np.argmax(row))
    bias = np.zeros(300, F32)
    bias[top] = -np.inf
    got = S.alternatives(row, None, 8, bias=bias, code=top)
    assert top not in got.codes
    assert got.rank == 299                                    # -inf ranks behind every allowed token
    other = row.copy()
    other[top] = 1000.0                                       # whatever the network said of a banned token: not a bit of any output moves
    again = S.alternatives(other, None, 8, bias=bias, code=top)
    assert np.array_equal(got.codes, again.codes) and np.array_equal(got.logprobs.view(np.uint32), again.logprobs.view(np.uint32))
    assert got.entropy.view(np.uint32) == again.entropy.view(np.uint32) and again.rank == 299
    z = np.delete(row, top).astype(np.float64)                # and the sums are those over the 299 allowed tokens
    z = z - z.max()
    lp = z - np.log(np.exp(z).sum())
    assert abs(float(got.entropy) + float((np.exp(lp) * lp).sum())) <= S.alternatives_error_bound(300, 0, 0, got.entropy)[1]


def test_fewer_allowed_than_n():
    row = np.array([0.5, -1.0, 2.0, 0.0, 1.0], F32)
    bias = np.array([-np.inf, 0.0, -np.inf, -np.inf, 0.25], F32)
    got = S.alternatives(row, (0.7, 1.0, 0), 8, bias=bias, code=2)
    assert list(got.codes) == [4, 1, -1, -1, -1, -1, -1, -1]
    assert np.isfinite(got.logprobs[:2]).all() and np.isneginf(got.logprobs[2:]).all()
    assert got.rank == 3            # the banned tokens 0, 2, 3 tie at -inf behind the two allowed ones, in index order: 4, 1, 0, 2, 3


@pytest.mark.parametrize("V", [2048, 300, 5, 1])
def test_prefix_and_independence_of_n(V):
    rng = np.random.default_rng(8 + V)
    row = (3.0 * rng.standard_normal(V)).astype(F32)
    rec = (1.7, 1.0, 0)
    a8 = S.alternatives(row, rec, 8, code=V // 2)
    for n in (0, 1, 3):
        a = S.alternatives(row, rec, n, code=V // 2)
        assert np.array_equal(a.codes, a8.codes[:n]) and np.array_equal(a.logprobs.view(np.uint32), a8.logprobs[:n].view(np.uint32))
        assert a.entropy.view(np.uint32) == a8.entropy.view(np.uint32) and a.rank == a8.rank
    finite = a8.logprobs[np.isfinite(a8.logprobs)]
    assert (np.diff(finite) <= 0).all()
    for T in (0.5, 4.0):                                      # the rank does not depend on the temperature
        assert S.alternatives(row, (T, 1.0, 0), 1, code=V // 2).rank == a8.rank


def test_neutral_total_is_the_logprob_total():
    """Without top-k / top-p, alt_logprob[rank] has the bits of `sampling.logprob` of the same code."""
    rng = np.random.default_rng(12)
    row = (2.0 * rng.standard_normal(2048)).astype(F32)
    got = S.alternatives(row, (0.8, 1.0, 0), 8)
    for j in range(8):
        assert got.logprobs[j].view(np.uint32) == S.logprob(row, got.codes[j], (0.8, 1.0, 0)).view(np.uint32)


def test_repetition_history_enters():
    rng = np.random.default_rng(13)
    row = rng.standard_normal(300).astype(F32)
    top = int(np.argmax(row))
    counts = S.repeat_counts([top, top, 5], 300, 5)
    got = S.alternatives(row, None, 2, counts=counts, rep=(5, 50.0, 0.0), code=top)
    assert top not in got.codes and got.rank > 1
    off = S.alternatives(row, None, 2, counts=counts, rep=(0, 50.0, 0.0), code=top)
    assert off.codes[0] == top and off.rank == 0


def test_uncertain_keep():
    e = np.array([[0.1, 2.0], [1.0, 0.0]], F32)
    assert np.array_equal(S.uncertain_keep(e, 1.0), [[True, False], [True, True]])
    assert S.uncertain_keep(e, 1.0).dtype == bool
    with pytest.raises(ValueError):
        S.uncertain_keep(np.zeros((3,), F32), 1.0)
    with pytest.raises(ValueError):
        S.uncertain_keep(e, float("nan"))


def test_argument_checks():
    from talkshow_amd import _lib
    for bad in (-1, 9, 1.5, True, "3"):
        with pytest.raises(ValueError):
            S.alt_count(bad)
        with pytest.raises(ValueError):
            S.alternatives(np.zeros(5, F32), None, bad)
    assert [S.alt_count(n) for n in (0, 8, np.int64(3))] == [0, 8, 3]
    assert _lib.alt_request(None, _lib.TS_SAMPLE_GREEDY, "run") is None           # the keyword is off: nothing is checked
    assert _lib.alt_request(3, _lib.TS_SAMPLE_PHILOX, "run") == 3 and _lib.alt_request(0, _lib.TS_SAMPLE_UNIFORMS, "run") == 0
    for mode in (_lib.TS_SAMPLE_GREEDY, _lib.TS_TEACHER_FORCED):
        with pytest.raises(ValueError, match=r"sampling=\(1, 1, 1\)"):
            _lib.alt_request(3, mode, "run")
    with pytest.raises(NotImplementedError):
        _lib.alt_request(3, _lib.TS_SAMPLE_PHILOX, "run", guide=True)
    with pytest.raises(ValueError):                                              # n is checked ahead of the mode and of guidance
        _lib.alt_request(9, _lib.TS_SAMPLE_GREEDY, "run", guide=True)


def test_entries_are_named_only_with_the_keyword():
    """The ctypes ladder: `_alt` is the `_repeat` entry plus one record pointer ahead of the stream, and is chosen only by a call that
    brings the record."""
    from talkshow_amd import _lib
    for plain, alt in _lib.ALT_ENTRY.items():
        assert _lib.SIGNATURES[alt][1] == _lib.SIGNATURES[plain][1][:-1] + _lib.MIXED_PIECES["alt"] + [_lib.SIGNATURES[plain][1][-1]]
    fixed12, fixed16 = tuple(range(12)), tuple(range(16))
    name, args = _lib.pixelcnn_mixed_args(fixed12, stream="s")
    assert name == "ts_pixelcnn_generate_mixed_repeat" and len(args) == len(_lib.SIGNATURES[name][1])
    name, args = _lib.pixelcnn_mixed_args(fixed12, alt="rec", stream="s")
    assert name == "ts_pixelcnn_generate_alt" and args[-2:] == ("rec", "s") and len(args) == len(_lib.SIGNATURES[name][1])
    name, args = _lib.body_mixed_args(fixed16, alt="rec", stream="s")
    assert name == "ts_body_pixel_infer_alt" and len(args) == len(_lib.SIGNATURES[name][1])
    name, args = _lib.body_mixed_args(fixed16, poses=(1, 2, 3, 4), alt="rec", stream="s")
    assert name == "ts_body_pixel_infer_alt_poses" and len(args) == len(_lib.SIGNATURES[name][1])
    with pytest.raises(NotImplementedError):
        _lib.pixelcnn_mixed_args(fixed12, guide="g", guide_scale="s", alt="rec", stream="s")
    step, alt = _lib.SIGNATURES["ts_pixelcnn_stream_step_ctl"][1], _lib.SIGNATURES["ts_pixelcnn_stream_step_alt"][1]
    assert alt == step[:-1] + _lib.MIXED_PIECES["alt"] + [step[-1]]
    rep, op = _lib.SIGNATURES["ts_op_sample_repeat"][1], _lib.SIGNATURES["ts_op_sample_alt"][1]
    assert op == rep[:-1] + _lib.MIXED_PIECES["alt"] + [rep[-1]]
