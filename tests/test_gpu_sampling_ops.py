"""The sampler with per-clip controls as an operator (`ts_op_sample_ctl`; `csrc/vq.hip`: `sample_ctl_kernel`, an entry of
`sample_ctl_body`) against the sampler without controls (`sample_kernel`, an entry of `sample_plain_body`), the numpy twin
(`talkshow_amd/sampling.py`), the float64 definition of tests/test_sampling_host.py and the float64 truncated distribution.
Every comparison with the twin or the plain sampler is EQUALITY: a draw is a pure function of (logits row, record, uniform).  Operator
launches carry B = 5 rows (the chi-square draws 4 096 per call, as `test_op_sample_philox_chi_square` does).
Every test fails on a build without the feature: `ts_op_sample_ctl` does not exist there.
"""
import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S
from test_sampling_host import U_LAST, float64_cases, keep64, probs64

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [2048, 256, 300, 100]
NEUTRAL = (1.0, 1.0, 0)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, (t, p, k) in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    return arr


def op_ctl(hip, logits, recs, u=None, philox=None, want_kept=True):
    """logits (B,V) numpy or device tensor, recs = list of 1 or B records -> (idx (B,), kept (B,V) bool or None)."""
    _lib, lib, ctx = hip
    ld = logits if torch.is_tensor(logits) else torch.from_numpy(np.ascontiguousarray(logits, F32)).cuda()
    B, V = ld.shape
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((B, V), 9, dtype=torch.uint8, device="cuda") if want_kept else None
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    seed, clip0, pos = philox if philox is not None else (0, 0, 0)
    mode = _lib.TS_SAMPLE_UNIFORMS if u is not None else _lib.TS_SAMPLE_PHILOX
    _lib.check(lib.ts_op_sample_ctl(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, _table(_lib, recs), len(recs),
                                    _lib.dptr(idx), _lib.dptr(kept), None))
    return idx.cpu().numpy(), (kept.cpu().numpy().astype(bool) if want_kept else None)


def regime_rows(golden, V):
    """Five rows: the peaked real row, a flat row, an all-equal row, blocks of ties (they straddle every rank k), a row with -inf entries."""
    rng = np.random.default_rng(100 + V)
    real = golden("pix_full")["step_logits"][1, 7, 1][:V]
    flat = (0.01 * rng.standard_normal(V)).astype(F32)
    ties = rng.integers(0, 5, V).astype(F32)
    minf = rng.standard_normal(V).astype(F32)
    minf[rng.random(V) < 0.3] = -np.inf
    minf[V // 2] = 1.5
    return np.ascontiguousarray(np.stack([real, flat, np.zeros(V, F32), ties, minf]), F32)


@pytest.mark.parametrize("V", VS)
def test_neutral_records_equal_the_plain_sampler(hip, golden, V):
    _lib, lib, ctx = hip
    rng = np.random.default_rng(V)
    rows = regime_rows(golden, V)
    rows[2] = rng.standard_normal(V).astype(F32)
    ld = torch.from_numpy(rows).cuda()
    B = rows.shape[0]
    plain = torch.empty(B, dtype=torch.int64, device="cuda")
    for u in ([0.0] * B, [float(U_LAST)] * B, list(rng.random(B)), list(rng.random(B)), [0.0, float(U_LAST), 0.5, float(U_LAST), 0.0]):
        u = np.asarray(u, F32)
        ud = torch.from_numpy(u).cuda()
        _lib.check(lib.ts_op_sample(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_UNIFORMS, _lib.dptr(ud), _lib.dptr(plain), None))
        for recs in ([NEUTRAL], [NEUTRAL] * B, [(1.0, 1.0, V), (1.0, 1.0, V + 5), NEUTRAL, NEUTRAL, (1.0, 1.0, V)]):
            idx, kept = op_ctl(hip, ld, recs, u=u)
            np.testing.assert_array_equal(idx, plain.cpu().numpy())
            assert kept.all()
    for seed, clip0, pos in ((99, 0, 15), (2 ** 40 + 3, 2 ** 33, 149)):
        _lib.check(lib.ts_op_sample_philox(ctx, _lib.dptr(ld), B, V, seed, clip0, pos, _lib.dptr(plain), None))
        idx, _ = op_ctl(hip, ld, [NEUTRAL], philox=(seed, clip0, pos))
        np.testing.assert_array_equal(idx, plain.cpu().numpy())


@pytest.mark.parametrize("V", VS)
def test_twin_grid(hip, golden, V):
    """T x k x p = 160 records on each of the five row regimes: idx and kept equal the twin's.  Every launch carries five DIFFERENT records
    (n_ctl = B); a last round carries one record for all rows (n_ctl = 1)."""
    rows = regime_rows(golden, V)
    B = rows.shape[0]
    ld = torch.from_numpy(rows).cuda()
    grid = [(T, p, k) for T in (0.5, 1.0, 1.7, 4.0) for k in (0, 1, 2, 7, 64, V - 1, V, V + 5) for p in (1e-6, 0.3, 0.9, 0.999, 1.0)]
    assert len(grid) == 160
    rng = np.random.default_rng(V + 1)
    special = [0.0, float(U_LAST), 0.5]
    cache = {}                                         # the twin's kept set of (row, record): computed once, shared by the draws

    def twin(b, rec, u):
        if (b, rec) not in cache:
            cache[(b, rec)] = S.keep_mask(rows[b], rec)
        return S.draw(rows[b], u, rec[0], cache[(b, rec)]), cache[(b, rec)]
    for c in range(len(grid)):
        recs = [grid[(c + 31 * b) % len(grid)] for b in range(B)]          # over the 160 launches every row meets every record
        u = np.asarray([special[(c + b) % 3] if (c + b) % 4 == 0 else rng.random() for b in range(B)], F32)
        idx, kept = op_ctl(hip, ld, recs, u=u)
        for b in range(B):
            ti, tk = twin(b, recs[b], u[b])
            assert np.array_equal(kept[b], tk), f"V {V} row {b} record {recs[b]}: kept differs at {np.flatnonzero(kept[b] != tk)[:8]}"
            assert idx[b] == ti, f"V {V} row {b} record {recs[b]} u {u[b]}: device {idx[b]} twin {ti}"
            assert kept[b, idx[b]]
    for rec in (grid[7], grid[58], grid[133]):                              # n_ctl = 1
        u = rng.random(B).astype(F32)
        idx, kept = op_ctl(hip, ld, [rec], u=u)
        for b in range(B):
            ti, tk = twin(b, rec, u[b])
            assert np.array_equal(kept[b], tk) and idx[b] == ti
    k5 = op_ctl(hip, ld, [(1.0, 1.0, 5)], u=np.zeros(B, F32))[1]
    assert np.array_equal(np.flatnonzero(k5[2]), np.arange(5))              # the all-equal row: k = 5 keeps indices 0 .. 4
    finite = np.isfinite(rows[4])
    kk = op_ctl(hip, ld, [(1.0, 1.0, int(finite.sum()))], u=np.zeros(B, F32))[1]
    assert not kk[4][~finite].any()                                         # -inf entries: not kept until k reaches them
    if finite.sum() + 3 < V:
        kk = op_ctl(hip, ld, [(1.0, 1.0, int(finite.sum()) + 3)], u=rng.random(B).astype(F32))
        assert kk[1][4][~finite].sum() == 3 and finite[kk[0][4]]            # kept when k reaches them; their weight is 0: no running sum crosses at one


@pytest.mark.parametrize("V", VS)
def test_extremes_give_the_argmax(hip, golden, V):
    rows = regime_rows(golden, V)
    B = rows.shape[0]
    am = np.asarray([int(np.argmax(r)) for r in rows])                      # numpy's argmax: the first maximum
    rng = np.random.default_rng(3)
    for u in (np.zeros(B, F32), np.full(B, U_LAST, F32), rng.random(B).astype(F32)):
        for recs in ([(1.0, 1.0, 1)], [(4.0, 1e-6, 0)], [(0.5, 1.0, 1), (1.0, 1e-6, 0), (1.7, 1e-6, 1), (4.0, 1.0, 1), (1.0, 1e-6, 2)]):
            idx, kept = op_ctl(hip, rows, recs, u=u)
            np.testing.assert_array_equal(idx, am)
            assert (kept.sum(1) == 1).all()


def test_kept_set_against_float64(hip, golden):
    cases = float64_cases(golden)
    for i in range(0, len(cases), 5):
        batch = cases[i:i + 5]
        for name, row, rec, dist, r in batch:
            assert dist >= 5e-4, name
        rows = np.stack([c[1] for c in batch])
        recs = [(c[2][0], c[2][1], c[2][2]) for c in batch]
        _, kept = op_ctl(hip, rows, recs, u=np.full(len(batch), 0.5, F32))
        for b, (name, row, rec, dist, r) in enumerate(batch):
            want = keep64(row, rec[0], rec[2], rec[1])
            assert np.array_equal(kept[b], want), f"{name}: kept sets differ at {np.flatnonzero(kept[b] != want)[:8]}"


@pytest.mark.parametrize("rec", [(1.0, 0.9, 0), (4.0, 1.0, 50), (0.7, 0.95, 0)], ids=["T1_p0.9", "T4_k50", "T0.7_p0.95"])
def test_chi_square_against_the_truncated_distribution(hip, golden, rec):
    """204 800 Philox draws (4 096 rows x 50 calls, subsequences 0 .. 204 799 at one grid position) from the real row under one record:
    Pearson chi-square against the float64 truncated, renormalised distribution over the classes with expected count >= 5 (the rest
    pooled), p > 1e-3 — the bar of `test_op_sample_philox_chi_square`; not one draw outside the kept set."""
    from scipy import stats
    row = np.ascontiguousarray(golden("pix_full")["step_logits"][1, 7, 1])
    V = row.size
    nb, calls, pos, seed = 4096, 50, 15, 99
    ld = torch.from_numpy(np.tile(row, (nb, 1))).cuda()
    draws = np.concatenate([op_ctl(hip, ld, [rec], philox=(seed, c * nb, pos), want_kept=False)[0] for c in range(calls)])
    u = np.asarray([O.philox_uniform(seed, b, pos) for b in range(64)], F32)         # the uniforms are the plain sampler's
    np.testing.assert_array_equal(draws[:64], S.sample_ctl(np.tile(row, (64, 1)), u, rec)[0])
    T, p, k = rec
    kept = keep64(row, T, k, p)
    assert np.array_equal(kept, S.keep_mask(row, rec))
    outside = int((~kept[draws]).sum())
    assert outside == 0, f"{outside} draws outside the kept set"
    pr = np.where(kept, probs64(row, T), 0.0)
    pr /= pr.sum()
    n = draws.size
    counts = np.bincount(draws, minlength=V).astype(np.float64)
    big = pr * n >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(pr[big] * n, pr[~big].sum() * n)
    ok = exp > 0
    chi2, pval = stats.chisquare(obs[ok], exp[ok] * obs[ok].sum() / exp[ok].sum())
    print(f"\nrecord {rec}: {kept.sum()} kept, chi-square over {big.sum()} classes + pooled rest, {n} draws: {chi2:.1f}, p = {pval:.3f}")
    assert big.sum() >= 2 and pval > 1e-3


def test_errors_before_any_launch(hip):
    _lib, lib, ctx = hip
    ld = torch.zeros((5, 64), dtype=torch.float32, device="cuda")
    idx = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    u = torch.zeros(5, dtype=torch.float32, device="cuda")

    def call(recs, mode, n=None):
        return lib.ts_op_sample_ctl(ctx, _lib.dptr(ld), 5, 64, mode, _lib.dptr(u), 0, 0, 0, _table(_lib, recs), len(recs) if n is None else n,
                                    _lib.dptr(idx), None, None)
    assert call([NEUTRAL] * 4 + [(0.0, 1.0, 0)], _lib.TS_SAMPLE_UNIFORMS) != 0 and "clip 4" in lib.ts_last_error().decode()
    assert call([NEUTRAL], _lib.TS_SAMPLE_GREEDY) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call([NEUTRAL] * 3, _lib.TS_SAMPLE_UNIFORMS) != 0 and "n_ctl" in lib.ts_last_error().decode()
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()
