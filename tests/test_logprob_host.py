"""Log-probabilities of the body decode, host side (no GPU): the numpy restatement `talkshow_amd/sampling.py::logprob` of the rule in
`include/talkshow_hip.h` ("log-probabilities") against an exact float64 log-softmax of the fp32 logits, the per-clip sums against
`math.fsum`, and the Python layer's argument errors.

The bound of the float64 comparison is DERIVED (`sampling.logprob_error_bound`): |d_c| 2^-24 for the subtraction; on S, relatively,
(chunk - 1 + 255) 2^-24 for its fp32 additions, det_expf's relative error (bounded by 2^-23: checked here against float64 exp on 2^20 + 1
points of [-86, 0]; 8.11e-8 was the worst of 2^26 + 1 points), 86 * 2^-24 for the rounding of a weight's argument and V e^-86 for the dropped
weights; |logprob| 2^-24 for the final rounding.  At V = 2048 that is 2.1e-5 + (|d_c| + |logprob|) 6e-8.  No figure of it comes from a device.
"""
import math

import numpy as np
import pytest

from talkshow_amd import sampling as S

F32 = np.float32
VS = (2048, 1000, 256, 7)


def special_rows(V, seed=0):
    """name -> (V,) fp32 row: random rows of three scales, an all-equal row, a row with one dominant logit whose other weights underflow
    (l - max < -86), rows with ties (also at the maximum) and with +0 / -0."""
    rng = np.random.default_rng(1000 + V + seed)
    rows = {}
    for k, scale in enumerate((1.0, 4.0, 12.0)):
        rows[f"random{k}"] = (rng.standard_normal(V) * scale).astype(F32)
    rows["equal"] = np.full(V, F32(-3.25))
    dom = (rng.standard_normal(V) - 200.0).astype(F32)
    dom[V // 3] = F32(5.0)
    rows["dominant"] = dom
    ties = rng.integers(-3, 3, V).astype(F32)                # few distinct values: ties everywhere, the maximum included
    rows["ties"] = ties
    z = np.where(rng.random(V) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    z[rng.integers(0, V, max(1, V // 8))] = F32(-1.5)
    rows["zeros"] = z
    return rows


def exact_log_softmax(row):
    x = np.asarray(row, F32).astype(np.float64)
    d = x - x.max()
    return d - math.log(math.fsum(np.exp(d)))


def test_det_expf_error_is_inside_the_bound_the_derivation_uses():
    x = np.linspace(-86.0, 0.0, (1 << 20) + 1).astype(F32)
    e = np.exp(x.astype(np.float64))
    rel = np.abs(S.det_expf(x).astype(np.float64) - e) / e
    print(f"det_expf worst relative error on 2^20 + 1 points of [-86, 0]: {rel.max():.3e} at {x[rel.argmax()]}")
    assert rel.max() <= S.DET_EXPF_REL_ERR
    below = np.linspace(-87.0, -86.0, 1001).astype(F32)
    assert np.all(S.det_expf(below[below < F32(-86.0)]) == 0.0)


@pytest.mark.parametrize("V", VS)
def test_restatement_against_exact_float64(V):
    worst = 0.0
    for name, row in special_rows(V).items():
        ex = exact_log_softmax(row)
        m = row.max()
        codes = sorted({0, V - 1, int(row.argmax()), int(row.argmin()), *np.random.default_rng(V).integers(0, V, 12).tolist()})
        for c in codes:
            lp = S.logprob(row, c)
            assert lp.dtype == np.float32 and np.isfinite(lp)
            bound = S.logprob_error_bound(V, np.float64(row[c]) - np.float64(m), ex[c])
            err = abs(float(lp) - ex[c])
            worst = max(worst, err / bound)
            assert err <= bound, f"V={V} row {name} code {c}: |{float(lp)!r} - {ex[c]!r}| = {err:.3e} > {bound:.3e}"
    print(f"V={V}: worst error / derived bound = {worst:.3f}")


@pytest.mark.parametrize("V", VS)
def test_stated_consequences(V):
    for name, row in special_rows(V).items():
        top = int(np.flatnonzero(row == row.max())[0])
        for c in (0, V - 1, top):
            a, b = S.logprob(row, c), S.logprob(row, c, (1.0, 1.0, 0))
            assert a.view(np.uint32) == b.view(np.uint32), f"neutral record, row {name}"   # the bits of the path without a record
        for T in (1.0, 0.7, 2.5):
            z = S.logprob(row, top, (T, 1.0, 1))
            assert z == 0.0, f"top_k = 1, row {name}"           # exactly zero (its sign is that of l_c - max: -0 where both zeros tie)
    dom = special_rows(V)["dominant"]
    top = int(dom.argmax())
    assert S.logprob(dom, top) == 0.0
    other = (top + 1) % V
    d = F32(dom[other] - dom[top])
    assert d < -86 and S.logprob(dom, other) == d                # the finite d_c, never log(w_c) = -inf
    assert np.isnan(S.logprob(dom, V)) and np.isnan(S.logprob(dom, -1))
    eq = special_rows(V)["equal"]
    assert abs(float(S.logprob(eq, V // 2)) + math.log(V)) <= S.logprob_error_bound(V, 0.0, math.log(V))


def test_record_renormalises_over_the_kept_set():
    """With a record the value is the log-probability under the distribution the draw is made from: exp over the kept tokens sums to 1."""
    row = special_rows(256)["random1"]
    for rec in ((0.7, 0.9, 0), (2.5, 0.6, 30), (1.0, 1.0, 5)):
        kept = np.flatnonzero(S.keep_mask(row, rec))
        total = math.fsum(math.exp(float(S.logprob(row, int(c), rec))) for c in kept)
        assert abs(total - 1.0) < 1e-4, (rec, total)


def test_logprob_sums_against_fsum():
    rng = np.random.default_rng(5)
    for B, H in ((1, 1), (5, 9), (2, 300), (3, 700)):          # 300, 700: more rows than lanes, a second and third round per lane
        lp = (-8.0 * rng.random((B, H, 2))).astype(F32)
        rows = [H] + [int(rng.integers(0, H + 1)) for _ in range(B - 1)]
        for table in (None, rows):
            got = S.logprob_sums(lp, table)
            assert got.dtype == np.float64 and got.shape == (B, 3)
            for b in range(B):
                hb = H if table is None else table[b]
                ref = [math.fsum(lp[b, :hb, 0].astype(np.float64)), math.fsum(lp[b, :hb, 1].astype(np.float64))]
                ref.append(math.fsum(lp[b, :hb].astype(np.float64).reshape(-1)))
                mag = float(np.abs(lp[b, :hb]).astype(np.float64).sum())
                for k in range(3):                               # fewer than 2 hb + 256 fp64 additions of terms of one sign
                    assert abs(got[b, k] - ref[k]) <= (2 * hb + 258) * 2.0 ** -53 * mag
    lp = np.zeros((2, 4, 2), F32)
    lp[1, 3] = np.nan                                            # beyond the clip's rows: does not enter
    assert np.array_equal(S.logprob_sums(lp, [4, 3]), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        S.logprob_sums(np.zeros((2, 4, 3), F32))


def test_argument_errors_are_raised_before_the_library_is_loaded(monkeypatch):
    import torch
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    assert _lib.logprob_request(False, (2, 4, 2)) is None and _lib.logprob_request(None, (2, 4, 2)) is None
    assert _lib.logprob_request(True, (2, 4, 2)) == "new"
    ok = torch.zeros((2, 4, 2), dtype=torch.float32)
    assert _lib.logprob_request(ok, (2, 4, 2)) is ok
    with pytest.raises(ValueError, match="float32"):
        _lib.logprob_request(torch.zeros((2, 4, 2), dtype=torch.float64), (2, 4, 2))
    with pytest.raises(ValueError, match="shape"):
        _lib.logprob_request(torch.zeros((2, 4), dtype=torch.float32), (2, 4, 2))
    with pytest.raises(ValueError, match="contiguous"):
        _lib.logprob_request(torch.zeros((2, 2, 4), dtype=torch.float32).transpose(1, 2), (2, 4, 2))
    with pytest.raises(ValueError, match="cuda"):
        _lib.logprob_request(ok, (2, 4, 2), device="cuda:0")
    with pytest.raises(ValueError, match="True, False"):
        _lib.logprob_request("yes", (2, 4, 2))
    with pytest.raises(ValueError, match=r"\(2, 4, 2\)"):
        _lib.score_codes_shape((2, 4), 2, 4)
    with pytest.raises(ValueError, match=r"\(2, 4, 2\)"):
        _lib.score_codes_shape((2, 5, 2), 2, 4)
    _lib.score_codes_shape((2, 4, 2), 2, 4)
    v = GatedPixelCNN(256, 64, 3, 4, True, False)                # the single-stack form returns none
    aud = torch.zeros((2, 4, 256))
    with pytest.raises(NotImplementedError, match="log-probabilities"):
        v.run(np.zeros(2, np.int64), aud, logprobs=True)
    with pytest.raises(NotImplementedError, match="log-probabilities"):
        v.score(np.zeros(2, np.int64), aud, np.zeros((2, 4, 2), np.int64))
    px = GatedPixelCNN(256, 64, 3, 4, True, True)
    with pytest.raises(ValueError, match=r"\(2, 4, 2\)"):
        px.score(np.zeros(2, np.int64), aud, np.zeros((2, 4), np.int64))
