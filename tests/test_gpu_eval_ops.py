"""Op-level tests of the evaluation reductions (`csrc/eval.hip`, `csrc/eval.cpp`) through the C ABI (`ts_eval_feat_stats`, `ts_eval_l1_total`,
`ts_eval_body_loss`, `ts_eval_diversity`: each one kernel of per-workgroup partials plus `sum_partials`), against sums written from the
definitions the sources cite (np.mean / np.cov moments, feat_dist's L1, body_loss's LVD / L2 error / variance, the pairwise diversity).

Guards.  Inputs and outputs sit in the allocations of tests/test_gpu_canary.py (`Guarded`, `run_both`: NaN red zones round the inputs, a
sentinel in and round the outputs, the guarded call bit-equal to the plain one, every output element written).

Exact cases, no tolerance.  Operands are small integers stored as fp32, |x| <= 512: every product and every partial sum is an integer below
2^53, exact in double in any order, so the outputs must EQUAL numpy's sums (a float64 BLAS product is exact here too).  They cover every
instantiation (D = 32, 64, 128), the block edges, and the second grid-stride trip of feat_stats (past 1024 x 128 rows) and of l1 (past
1024 x 4096 elements); for the diversity a wrong unranking of the pair index counts some pair twice and changes the sum.

Random fp32 cases against a correctly rounded reference (`math.fsum` of the float64 terms, `np.longdouble` for the moments).  Unit: sum |term|.
Products and differences of two fp32 values are exact in double, so only additions and the square roots round; the ceiling is
(longest addition chain + 8) 2^-53, the chain read from the code's loop structure:
  feat_stats  a workgroup adds its rows one by one (128 per grid-stride trip), sum_partials adds the workgroups' partials one by one:
              128 ceil(ceil(n / 128) / nwg) + nwg, nwg = min(1024, ceil(n / 128))
  l1          a thread adds ceil(n / (256 nwg)) elements, the block tree adds 8 levels, then nwg partials: that + 8 + nwg, nwg = min(1024, ceil(n / 4096))
  diversity   ceil(L / 256) + 8 + pairs
  body_loss   error and LVD: ceil(B J / 256) + 8 + T; the + 8 of the ceiling covers the squares, their sum and the square root of a term (unit
              of the LVD: sum |v_p| + |v_g|, what the difference of the two magnitudes is made of).  The variance subtracts the mean from
              every sample: the cancellation has no bound in units of the result, so NO ceiling is asserted for it; its unit is
              sum_j |var_j|_1 and the bound is the measured one alone.
Each asserted bound is 2x the largest error that the first MI355X run of this file recorded (TS_MEASURED_LOG;
profiles/smplx_eval_ops_measured.jsonl: that run asserted the ceilings, or nothing where there is none), with one exception: both l1
cases came out equal to the correctly rounded sum, and the bound is one unit in the last place of a double.  `test_bounds_catch_defects` (CPU)
applies each defect of DEFECTS to the reference and shows that the bound named there misses it by at least 10x.
"""
import math

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from test_gpu_canary import F32, F64 as T64, run_both

F64 = np.float64
EPS = 2.0 ** -53
# 2x the largest error in the first MI355X run's records (profiles/smplx_eval_ops_measured.jsonl; that run had no bounds yet and asserted the
# ceilings, its variance lines carry an infinite bound), in units of sum |term|.  Every case passed on that run.
FEAT_BOUND = 3.7e-15         # 1.850e-15: D = 128, n = 129
# l1: both cases came out equal to the correctly rounded sum (0.0), and 2 x 0 is no bound: one unit in the last place of a double, the
# smallest amount by which a result can differ from it, is asserted instead
L1_BOUND = 2.0 ** -52
DIV_BOUND = 3.5e-16          # 1.718e-16: bs = 37, L = 901
BODY_SUM_BOUND = 5.4e-16     # LVD and L2 error; 2.666e-16: B = 1
BODY_VAR_BOUND = 4.0e-16     # 1.987e-16: B = 5


def ceiling(chain):
    return (chain + 8) * EPS


def feat_chain(n):
    wg = min(1024, -(-n // 128))
    return 128 * -(-(-(-n // 128)) // wg) + wg


def l1_chain(n):
    wg = min(1024, max(1, -(-n // 4096)))
    return -(-n // (256 * wg)) + 8 + wg


def div_chain(bs, L):
    return -(-L // 256) + 8 + bs * (bs - 1) // 2


def body_chain(B, T, Jn):
    return -(-B * Jn // 256) + 8 + T


def measured(stage, case, err, bound, ceil=None):
    """Records err (TS_MEASURED_LOG) and asserts it under the stage's bound; the bound itself under the case's ceiling.  Until the first
    run's records exist a bound is infinite: then the ceiling is asserted, or nothing where there is none."""
    if math.isinf(bound) and ceil is not None:
        bound = ceil
    assert ceil is None or bound <= ceil, f"{stage}.{case}: bound {bound:.2e} over the ceiling {ceil:.2e}"
    assert_close_measured(f"eval.{stage}.{case}", np.array([err]), np.array([0.0]), bound)


def in_units(err, unit):
    err, unit = np.asarray(err, F64), np.asarray(unit, F64)
    assert (err[unit == 0] == 0).all(), "a sum that nothing contributes to is not exactly zero"
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def ints(rng, shape, hi=512):
    return rng.integers(-hi, hi + 1, shape).astype(np.float32)


# ----------------------------------------------------------------------------------------------- references
def feat_ref(x, defect=None, dtype=np.longdouble):
    """x (n, D) fp32 -> (sum x (D,), sum x x^T (D, D)) and their units, accumulated in `dtype`."""
    x = np.asarray(x, F64)
    if defect == "row_dropped":
        x = x[:-1]
    if defect == "fp32_accumulation":
        x32 = x.astype(np.float32)
        return np.cumsum(x32, axis=0, dtype=np.float32)[-1].astype(F64), np.einsum("ni,nj->ij", x32, x32).astype(F64)
    xl = x.astype(dtype)
    return xl.sum(0), xl.T @ xl


def feat_units(x):
    a = np.abs(np.asarray(x, F64))
    return a.sum(0), a.T @ a


def l1_ref(a, b):
    t = np.abs(np.asarray(a, F64).reshape(-1) - np.asarray(b, F64).reshape(-1))
    return math.fsum(t), math.fsum(t)


def div_ref(k, defect=None):
    """k (bs, L) fp32 -> sum over pairs i < j of sum |k_i - k_j|, and the same (all terms are magnitudes)."""
    k = np.asarray(k, F64)
    bs = k.shape[0]
    pairs = [(i, j) for i in range(bs) for j in range(i + 1, bs)]
    if defect == "pair_counted_twice":
        pairs[-1] = pairs[0]
    t = np.concatenate([np.abs(k[i] - k[j]) for i, j in pairs])
    return math.fsum(t), math.fsum(t)


def body_ref(gt, prs, Jl, Tl, defect=None):
    """gt (T, J, 3), prs (B, T, J, 3) fp32 -> the three raw sums {LVD over t < Tl - 1 and j < Jl, sum |g - p|_2, sum_t sum_j |var_b p|_2}
    and their units."""
    g, p = np.asarray(gt, F64), np.asarray(prs, F64)
    B = p.shape[0]
    steps = Tl if defect == "lvd_over_T_lvd_steps" else Tl - 1
    pv = np.linalg.norm(p[:, 1:steps + 1, :Jl] - p[:, :steps, :Jl], axis=-1)
    gv = np.linalg.norm(g[1:steps + 1, :Jl] - g[:steps, :Jl], axis=-1)
    err = np.linalg.norm(g[None] - p, axis=-1)
    with np.errstate(all="ignore"):
        var = p.var(axis=0, ddof=0 if defect == "biased_variance" else 1)
    out = [math.fsum(np.abs(pv - gv[None]).reshape(-1)), math.fsum(err.reshape(-1)), math.fsum(np.linalg.norm(var, axis=-1).reshape(-1))]
    unit = [math.fsum((pv + gv[None]).reshape(-1)), out[1], math.fsum(np.abs(var).sum(-1).reshape(-1)) if B > 1 else math.nan]
    return out, unit


# ----------------------------------------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load(), _lib.context(0)


def run_feat(hip, x):
    _lib, lib, ctx = hip
    n, D = x.shape
    r = run_both(lambda p: _lib.check(lib.ts_eval_feat_stats(ctx, p["x"], n, D, p["out"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"out": ((D + D * D,), T64)})
    o = r["out"].cpu().numpy()
    return o[:D], o[D:].reshape(D, D)


def run_l1(hip, a, b):
    _lib, lib, ctx = hip
    r = run_both(lambda p: _lib.check(lib.ts_eval_l1_total(ctx, p["a"], p["b"], a.size, p["out"], _lib.stream_ptr())),
                 {"a": (a, F32), "b": (b, F32)}, {"out": ((1,), T64)})
    return float(r["out"].cpu().numpy()[0])


def run_div(hip, k):
    _lib, lib, ctx = hip
    bs, L = k.shape
    r = run_both(lambda p: _lib.check(lib.ts_eval_diversity(ctx, p["k"], bs, L, p["out"], _lib.stream_ptr())),
                 {"k": (k, F32)}, {"out": ((1,), T64)})
    return float(r["out"].cpu().numpy()[0])


def run_body(hip, gt, prs, Jl, Tl):
    _lib, lib, ctx = hip
    B, T, Jn, _ = prs.shape
    r = run_both(lambda p: _lib.check(lib.ts_eval_body_loss(ctx, p["gt"], p["prs"], B, T, Jn, Jl, Tl, p["out"], _lib.stream_ptr())),
                 {"gt": (gt, F32), "prs": (prs, F32)}, {"out": ((3,), T64)})
    return r["out"].cpu().numpy()


# ----------------------------------------------------------------------------------------------- exact cases
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1024 * 128 + 129])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_feat_stats_exact(hip, D, n):
    """Every instantiation at one row, one short of a staged block of 128, a block, one over, and the second grid-stride trip; all D + D^2
    outputs.  D = 128 declares 66 048 bytes of static LDS: the launch itself is part of what is tested."""
    x = ints(np.random.default_rng(D + n), (n, D))
    s, o = run_feat(hip, x)
    x64 = x.astype(F64)
    assert np.array_equal(s, x64.sum(0)), "sum x differs from the exact sum"
    assert np.array_equal(o, x64.T @ x64), "sum x x^T differs from the exact sum"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 1024 * 4096 + 4097])
def test_l1_total_exact(hip, n):
    rng = np.random.default_rng(n)
    a, b = ints(rng, n), ints(rng, n)
    assert run_l1(hip, a, b) == float(np.abs(a.astype(F64) - b.astype(F64)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 255, 257, 901])
@pytest.mark.parametrize("bs", [2, 3, 37])
def test_diversity_exact(hip, bs, L):
    """Sequences whose pairwise distances all differ (a common offset per sequence that grows quadratically): a pair counted twice in
    place of another changes the sum."""
    rng = np.random.default_rng(bs * 1000 + L)
    k = np.clip(ints(rng, (bs, L), 100) + ((np.arange(bs) ** 2) % 401)[:, None], -512, 512).astype(np.float32)
    k64 = k.astype(F64)
    ref = sum(float(np.abs(k64[i] - k64[j]).sum()) for i in range(bs) for j in range(i + 1, bs))
    assert run_div(hip, k) == ref


# ----------------------------------------------------------------------------------------------- random fp32 cases
@pytest.mark.gpu
@pytest.mark.parametrize("D,n,kind", [(D, n, "unit") for D in (32, 64, 128) for n in (129, 3001)] + [(64, 3001, "offset")])
def test_feat_stats_random(hip, D, n, kind):
    """Per-column scales over a decade and a mean; "offset": mean 1000, sigma 1 — fp32 accumulation would lose the variance at once."""
    rng = np.random.default_rng(D * n)
    if kind == "offset":
        x = (1000.0 + rng.standard_normal((n, D))).astype(np.float32)
    else:
        x = (rng.standard_normal((n, D)) * rng.uniform(0.1, 3.0, D) + rng.standard_normal(D)).astype(np.float32)
    s, o = run_feat(hip, x)
    rs, ro = feat_ref(x)
    us, uo = feat_units(x)
    e = max(in_units(np.abs(s - rs).astype(F64), us), in_units(np.abs(o - ro).astype(F64), uo))
    measured("feat_stats", f"{kind}.d{D}.n{n}", e, FEAT_BOUND, ceiling(feat_chain(n)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 100003])
def test_l1_total_random(hip, n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), (3.0 * rng.standard_normal(n)).astype(np.float32)
    ref, unit = l1_ref(a, b)
    measured("l1", f"n{n}", abs(run_l1(hip, a, b) - ref) / unit, L1_BOUND, ceiling(l1_chain(n)))


@pytest.mark.gpu
@pytest.mark.parametrize("bs,L", [(2, 257), (37, 901), (5, 20000)])
def test_diversity_random(hip, bs, L):
    k = np.random.default_rng(bs + L).standard_normal((bs, L)).astype(np.float32)
    ref, unit = div_ref(k)
    measured("diversity", f"bs{bs}.l{L}", abs(run_div(hip, k) - ref) / unit, DIV_BOUND, ceiling(div_chain(bs, L)))


# ----------------------------------------------------------------------------------------------- body_loss
def body_inputs(rng, B, T, Jn):
    gt = rng.standard_normal((T, Jn, 3)).astype(np.float32)
    prs = (gt[None] + 0.3 * rng.standard_normal((B, T, Jn, 3))).astype(np.float32)
    return gt, prs


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 5])
def test_body_loss(hip, B):
    """T in {2, 3, 33} x J in {1, 55, 127, 300} (over 256: the variance loop's second trip) x J_lvd in {0, 22, J} x T_lvd in {2, T - 1, T}
    (T_lvd < T: what no Python caller passes).  The three raw sums, not the divisions.  B = 1: the variance of one sample is NaN, the other
    two sums are finite and right.  prs = gt broadcast: all three exactly 0."""
    rng = np.random.default_rng(B)
    worst_sum = worst_var = 0.0
    chain = 0
    for T in (2, 3, 33):
        for Jn in (1, 55, 127, 300):
            gt, prs = body_inputs(rng, B, T, Jn)
            for Jl in sorted({0, min(22, Jn), Jn}):
                for Tl in sorted({2, max(2, T - 1), T}):
                    got = run_body(hip, gt, prs, Jl, Tl)
                    ref, unit = body_ref(gt, prs, Jl, Tl)
                    what = f"B {B} T {T} J {Jn} J_lvd {Jl} T_lvd {Tl}"
                    if Jl == 0:
                        assert got[0] == 0.0, f"{what}: the LVD over no joints is not 0"
                    worst_sum = max(worst_sum, in_units(np.abs(got[:2] - ref[:2]), unit[:2]))
                    if B == 1:
                        assert math.isnan(got[2]) and np.isfinite(got[:2]).all(), f"{what}: one sample must give a NaN variance and finite sums"
                    else:
                        worst_var = max(worst_var, in_units(abs(got[2] - ref[2]), unit[2]))
                    chain = max(chain, body_chain(B, T, Jn))
            same = run_body(hip, gt, np.ascontiguousarray(np.broadcast_to(gt[None], (B,) + gt.shape)), min(22, Jn), T)
            assert (same[:2] == 0).all() and (math.isnan(same[2]) if B == 1 else same[2] == 0), f"B {B} T {T} J {Jn}: prs = gt is not exactly 0"
    measured("body_sums", f"b{B}", worst_sum, BODY_SUM_BOUND, ceiling(chain))
    if B > 1:
        measured("body_var", f"b{B}", worst_var, BODY_VAR_BOUND)


@pytest.mark.gpu
def test_body_loss_rejects_bad_shapes(hip):
    """A rejected shape returns non-zero and launches nothing: the output keeps its fill."""
    _lib, lib, ctx = hip
    gt, prs = torch.zeros(4, 5, 3, device="cuda"), torch.zeros(2, 4, 5, 3, device="cuda")
    out = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    for B, T, Jn, Jl, Tl in ((0, 4, 5, 5, 4), (2, 1, 5, 5, 1), (2, 4, 0, 0, 4), (2, 4, 5, 6, 4), (2, 4, 5, -1, 4), (2, 4, 5, 5, 5), (2, 4, 5, 5, 1)):
        assert lib.ts_eval_body_loss(ctx, _lib.dptr(gt), _lib.dptr(prs), B, T, Jn, Jl, Tl, _lib.dptr(out), _lib.stream_ptr()) != 0
        assert b"ts_eval_body_loss: bad shape" in lib.ts_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ----------------------------------------------------------------------------------------------- the Python layer
@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 128])
def test_feature_stats_other_widths(hip, D):
    """FeatureStats(32) and (128) over ragged pushes == numpy float64 mean / cov of all rows together (tests/test_gpu_parity.py does 64)."""
    from talkshow_amd import evaluation as E
    rng = np.random.default_rng(D)
    st, rows = E.FeatureStats(D), []
    for n in (1, 127, 128, 129, 5000, 33):
        x = (rng.standard_normal((n, D)) * rng.uniform(0.1, 3.0, D) + rng.standard_normal(D)).astype(np.float32)
        st.push(x)
        rows.append(x)
    allr = np.vstack(rows).astype(F64)
    mu, sig = st.mean_cov()
    np.testing.assert_allclose(mu, allr.mean(0), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(sig, np.cov(allr, rowvar=False), rtol=1e-8, atol=1e-10)


# ----------------------------------------------------------------------------------------------- CPU: the bounds
# defect -> the bound that catches it
DEFECTS = {"row_dropped": "feat_stats", "fp32_accumulation": "feat_stats", "pair_counted_twice": "diversity", "biased_variance": "body_var",
           "lvd_over_T_lvd_steps": "body_sums"}


def test_bounds_catch_defects():
    """Each defect, applied to the reference on inputs of the GPU tests, moves the result by at least 10x the bound named for it."""
    rng = np.random.default_rng(0)
    moved = {}
    x = (rng.standard_normal((3001, 32)) * rng.uniform(0.1, 3.0, 32) + rng.standard_normal(32)).astype(np.float32)
    rs, ro = feat_ref(x)
    us, uo = feat_units(x)
    for d in ("row_dropped", "fp32_accumulation"):
        s, o = feat_ref(x, d)
        moved[d] = max(in_units(np.abs(s - rs).astype(F64), us), in_units(np.abs(o - ro).astype(F64), uo))
    k = rng.standard_normal((37, 901)).astype(np.float32)
    ref, unit = div_ref(k)
    moved["pair_counted_twice"] = abs(div_ref(k, "pair_counted_twice")[0] - ref) / unit
    gt, prs = body_inputs(rng, 5, 33, 55)
    ref, unit = body_ref(gt, prs, 22, 32)
    moved["biased_variance"] = abs(body_ref(gt, prs, 22, 32, "biased_variance")[0][2] - ref[2]) / unit[2]
    moved["lvd_over_T_lvd_steps"] = abs(body_ref(gt, prs, 22, 32, "lvd_over_T_lvd_steps")[0][0] - ref[0]) / unit[0]
    bounds = {"feat_stats": FEAT_BOUND, "diversity": DIV_BOUND, "body_var": BODY_VAR_BOUND, "body_sums": BODY_SUM_BOUND}
    assert set(moved) == set(DEFECTS)
    for d, e in moved.items():
        b = bounds[DEFECTS[d]]
        assert math.isfinite(b), f"the {DEFECTS[d]} bound is not set"
        print(f"\n[defect] {d}: {e:.3e} = {e / b:.0f} x the {DEFECTS[d]} bound {b:.1e}")
        assert e >= 10 * b, f"{d} moves the result by {e:.2e} only, under 10x the {DEFECTS[d]} bound {b:.1e}"


def test_references_and_chains():
    """The references against numpy on integers (exact) and the chain lengths at the shapes the GPU tests use."""
    rng = np.random.default_rng(1)
    x = ints(rng, (300, 32))
    s, o = feat_ref(x)
    assert np.array_equal(s.astype(F64), x.astype(F64).sum(0)) and np.array_equal(o.astype(F64), x.astype(F64).T @ x.astype(F64))
    gt, prs = ints(rng, (4, 6, 3), 8).astype(F64), ints(rng, (3, 4, 6, 3), 8).astype(F64)
    out, _ = body_ref(gt, prs, 6, 4)
    lvd = sum(abs(np.linalg.norm(prs[b, t + 1, j] - prs[b, t, j]) - np.linalg.norm(gt[t + 1, j] - gt[t, j]))
              for b in range(3) for t in range(3) for j in range(6))
    assert abs(out[0] - lvd) <= 1e-12 * lvd
    assert abs(out[2] - np.linalg.norm(prs.astype(F64).var(0, ddof=1), axis=-1).sum()) <= 1e-12 * out[2]
    assert feat_chain(1) == 129 and feat_chain(3001) == 128 + 24 and feat_chain(1024 * 128 + 129) == 256 + 1024
    assert l1_chain(257) == 2 + 8 + 1 and l1_chain(1024 * 4096 + 4097) == 17 + 8 + 1024
    assert div_chain(37, 901) == 4 + 8 + 666
