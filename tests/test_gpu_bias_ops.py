"""The samplers under a code bias as an operator (`ts_op_sample_bias`; `csrc/vq.hip`: `sample_ctl_bias_kernel` and
`sample_ctl_bias_given_kernel`, the BIAS = true entries of `sample_ctl_body`) against the numpy twin (`talkshow_amd/sampling.py`:
`biased`, `keep_mask_bias`, `sample_bias`) and against `ts_op_sample_ctl` / `ts_op_sample_lp` for rows without a table.  Indices and kept
bytes are compared for EQUALITY; a log-probability may differ from the twin's by one fp32 spacing (the two fp64 logs) and no more.
Launches carry B = 5 rows at V = 2048 (the vector path), 256, 300 and 100 (the generic path; 300 is no multiple of 256).  The column of
a table that a launch must not read is filled with NaN.  Every test fails on a build without the feature: the entry does not exist there.
"""
import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [2048, 256, 300, 100]
NEUTRAL = (1.0, 1.0, 0)
U_LAST = F32(1.0 - 2.0 ** -24)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, (t, p, k) in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    return arr


def regime_rows(golden, V):
    """tests/test_gpu_sampling_ops.py::regime_rows: the peaked real row, a flat row, an all-equal row, blocks of ties, a row with -inf."""
    rng = np.random.default_rng(100 + V)
    real = golden("pix_full")["step_logits"][1, 7, 1][:V]
    flat = (0.01 * rng.standard_normal(V)).astype(F32)
    ties = rng.integers(0, 5, V).astype(F32)
    minf = rng.standard_normal(V).astype(F32)
    minf[rng.random(V) < 0.3] = -np.inf
    minf[V // 2] = 1.5
    return np.ascontiguousarray(np.stack([real, flat, np.zeros(V, F32), ties, minf]), F32)


def op_bias(hip, logits, tables, index, column, recs=None, u=None, philox=None, given_rows=None, keep=None, given=None, want_copy=False):
    """One launch: logits (B,V), tables (NB,2,V), index (B,), column -> dict(idx, kept (B,V) bool, lp (B,), copy (B,V) or None)."""
    _lib, lib, ctx = hip
    ld = logits if torch.is_tensor(logits) else torch.from_numpy(np.ascontiguousarray(logits, F32)).cuda()
    B, V = ld.shape
    td = torch.from_numpy(np.ascontiguousarray(tables, F32)).cuda()
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((B, V), 9, dtype=torch.uint8, device="cuda")
    lp = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    copy = torch.full((B, V), 3.0, dtype=torch.float32, device="cuda") if want_copy else None
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    seed, clip0, pos = philox if philox is not None else (0, 0, 0)
    mode = _lib.TS_SAMPLE_UNIFORMS if u is not None else _lib.TS_SAMPLE_PHILOX
    i32p = _lib.C.POINTER(_lib.C.c_int32)
    index = np.ascontiguousarray(index, np.int32)
    gr = None if given_rows is None else np.ascontiguousarray(given_rows, np.int32)
    kd = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda()
    gd = None if given is None else torch.from_numpy(np.ascontiguousarray(given, np.int64)).cuda()
    _lib.check(lib.ts_op_sample_bias(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, None if recs is None else _table(_lib, recs),
                                     0 if recs is None else len(recs), _lib.dptr(idx), _lib.dptr(lp), None if gr is None else gr.ctypes.data_as(i32p),
                                     _lib.dptr(kd), _lib.dptr(gd), _lib.dptr(kept), _lib.dptr(copy), _lib.dptr(td), int(td.shape[0]),
                                     index.ctypes.data_as(i32p), int(column), None))
    return dict(idx=idx.cpu().numpy(), kept=kept.cpu().numpy().astype(bool), lp=lp.cpu().numpy(),
                copy=None if copy is None else copy.cpu().numpy())


def op_ctl_lp(hip, logits, recs, u):
    """`ts_op_sample_lp` with a table: what rows without a bias must equal bit for bit."""
    _lib, lib, ctx = hip
    ld = torch.from_numpy(np.ascontiguousarray(logits, F32)).cuda()
    B, V = ld.shape
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((B, V), 9, dtype=torch.uint8, device="cuda")
    lp = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ud = torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    _lib.check(lib.ts_op_sample_lp(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_UNIFORMS, _lib.dptr(ud), 0, 0, 0, _table(_lib, recs), len(recs),
                                   _lib.dptr(idx), _lib.dptr(kept), _lib.dptr(lp), None))
    return idx.cpu().numpy(), kept.cpu().numpy().astype(bool), lp.cpu().numpy()


def within_one_spacing(got, want):
    if np.isinf(want) or np.isnan(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.abs(F32(want))))


def bias_kinds(V):
    """name -> (V,) bias row, or None for 'the row has no table' (index -1).  V // 2 stays allowed everywhere: the -inf regime row has its
    one sure finite logit there."""
    rng = np.random.default_rng(11 + V)
    chunk = (V + 255) // 256

    def allow(n):
        t = np.full(V, -np.inf, F32)
        t[rng.choice(V, n, replace=False)] = 0.0
        t[V // 2] = 0.0
        return t
    one = np.full(V, -np.inf, F32)
    one[V // 2] = 0.0
    last = np.zeros(V, F32)
    last[-(2 * chunk + 3):] = -np.inf                 # the row's last tokens: the last two chunks and three more
    last[chunk - 1:V // 2:chunk] = -np.inf            # and the last token of every chunk of the lower half
    return {"none": None, "zeros": np.zeros(V, F32), "random": (2.0 * rng.standard_normal(V)).astype(F32), "allow1": one, "allow7": allow(6),
            "allow_half": allow(V // 2), "ban_last": last}


def grid(V):
    return [NEUTRAL, (0.5, 1.0, 0), (1.7, 0.9, 0), (1.0, 1.0, 7), (4.0, 0.999, 64), (1.0, 0.3, V - 1), (1.0, 1.0, 1), (0.7, 1e-6, 0)]


@pytest.mark.parametrize("V", VS)
def test_twin_grid(hip, golden, V):
    """8 records x 7 bias kinds x both columns on the five row regimes; u rotates through 0, 1 - 2^-24 and random: index, kept bytes and
    log-probability against the twin.  Every launch carries five different records."""
    rows = regime_rows(golden, V)
    B = rows.shape[0]
    ld = torch.from_numpy(rows).cuda()
    recs_all = grid(V)
    rng = np.random.default_rng(V + 1)
    special = [0.0, float(U_LAST), 0.5]
    for name, bias in bias_kinds(V).items():
        cache = {}
        for column in (0, 1):
            tables = np.full((1, 2, V), np.nan, F32)                     # the other column is never read
            if bias is not None:
                tables[0, column] = bias
            index = [-1 if bias is None else 0] * B
            for c in range(len(recs_all)):
                recs = [recs_all[(c + 3 * b) % len(recs_all)] for b in range(B)]
                u = np.asarray([special[(c + b) % 3] if (c + b + column) % 2 == 0 else rng.random() for b in range(B)], F32)
                got = op_bias(hip, ld, tables, index, column, recs, u=u)
                for b in range(B):
                    if (b, recs[b]) not in cache:
                        cache[(b, recs[b])] = S.keep_mask_bias(rows[b], recs[b], bias)
                    tk = cache[(b, recs[b])]
                    lb = S.biased(rows[b], bias)
                    ti = S.draw(lb, u[b], recs[b][0], tk)
                    what = f"V {V} bias {name} column {column} row {b} record {recs[b]} u {u[b]}"
                    assert np.array_equal(got["kept"][b], tk), f"{what}: kept differs at {np.flatnonzero(got['kept'][b] != tk)[:8]}"
                    assert got["idx"][b] == ti, f"{what}: device {got['idx'][b]} twin {ti}"
                    assert lb[ti] != -np.inf and tk[ti]
                    want = S.logprob(lb, ti, recs[b])
                    assert within_one_spacing(got["lp"][b], want), f"{what}: logprob {got['lp'][b]} twin {want}"


@pytest.mark.parametrize("V", VS)
def test_mixed_launch(hip, golden, V):
    """Rows 0 and 4 without a table, rows 1 and 2 sharing table 0, row 3 with table 1, in one launch: rows without a table equal
    `ts_op_sample_lp` with the same records BIT FOR BIT (index, kept bytes, log-probability bits); the others equal the twin.  The logits
    copy is the network's row, bias or not."""
    rows = regime_rows(golden, V)
    rows[2] = np.random.default_rng(V).standard_normal(V).astype(F32)
    rows[2, 5] = F32(-0.0)
    kinds = bias_kinds(V)
    tables = np.stack([np.stack([kinds["random"], kinds["ban_last"]]), np.stack([kinds["allow_half"], kinds["random"]])])
    index = [-1, 0, 0, 1, -1]
    recs = [(0.7, 0.9, 0), NEUTRAL, (1.7, 1.0, 40), (1.0, 0.95, 0), NEUTRAL]
    rng = np.random.default_rng(V + 9)
    for column in (0, 1):
        for u in (np.zeros(5, F32), np.full(5, U_LAST, F32), rng.random(5).astype(F32)):
            got = op_bias(hip, rows, tables, index, column, recs, u=u, want_copy=True)
            pi, pk, pl = op_ctl_lp(hip, rows, recs, u)
            assert np.array_equal(got["copy"].view(np.uint32), rows.view(np.uint32)), "the logits copy is the network's row"
            for b in range(5):
                if index[b] < 0:
                    assert got["idx"][b] == pi[b] and np.array_equal(got["kept"][b], pk[b])
                    assert got["lp"][b:b + 1].view(np.uint32)[0] == pl[b:b + 1].view(np.uint32)[0], f"row {b}: {got['lp'][b]} vs {pl[b]}"
                else:
                    bias = tables[index[b], column]
                    tk = S.keep_mask_bias(rows[b], recs[b], bias)
                    ti = S.draw(S.biased(rows[b], bias), u[b], recs[b][0], tk)
                    assert np.array_equal(got["kept"][b], tk) and got["idx"][b] == ti
                    assert within_one_spacing(got["lp"][b], S.logprob(S.biased(rows[b], bias), ti, recs[b]))
    # no sampling table at all: neutral records
    u = rng.random(5).astype(F32)
    got = op_bias(hip, rows, tables, index, 1, None, u=u)
    ti, tk, tl = S.sample_bias(rows, u, None, tables, index, 1)
    assert np.array_equal(got["idx"], ti) and np.array_equal(got["kept"], tk)
    assert all(within_one_spacing(got["lp"][b], tl[b]) for b in range(5))


@pytest.mark.parametrize("V", VS)
def test_given_codes_under_a_ban(hip, golden, V):
    """The given variant: a forced row takes its code whatever the table says — a banned code gets -inf and is still written; an allowed one
    gets the twin's value; a row whose mask byte is 0 or whose position is not below 2 G draws from the biased distribution."""
    rows = regime_rows(golden, V)
    kinds = bias_kinds(V)
    tables = np.stack([np.stack([kinds["ban_last"], kinds["allow7"]])])
    index = [0, 0, -1, 0, 0]
    banned0 = int(np.flatnonzero(kinds["ban_last"] == -np.inf)[-1])
    allowed0 = int(np.flatnonzero(kinds["ban_last"] == 0)[3])
    given = np.asarray([banned0, allowed0, banned0, banned0, 2 ** 40], np.int64)
    rng = np.random.default_rng(V + 2)
    u = rng.random(5).astype(F32)
    # the operator's position is 0 here: G >= 1 puts it below 2 G; row 3's mask byte is 0 and row 4 has G = 0: both unforced
    for recs in (None, [(0.8, 0.9, 0)] * 5):
        rec = NEUTRAL if recs is None else recs[0]
        got = op_bias(hip, rows, tables, index, 0, recs, u=u, given_rows=[1, 1, 1, 1, 0], keep=[1, 1, 1, 0, 1], given=given)
        assert got["idx"][0] == banned0 and got["lp"][0] == -np.inf                      # banned, still taken
        assert got["idx"][1] == allowed0
        assert within_one_spacing(got["lp"][1], S.given_logprob_bias(rows[1], allowed0, rec, tables[0, 0]))
        assert got["idx"][2] == banned0                                                  # no table: the code is not banned for this row
        assert within_one_spacing(got["lp"][2], S.given_logprob(rows[2], banned0, rec))
        for b in (3, 4):                                                                 # unforced: the biased draw
            tk = S.keep_mask_bias(rows[b], rec, tables[0, 0])
            ti = S.draw(S.biased(rows[b], tables[0, 0]), u[b], rec[0], tk)
            assert got["idx"][b] == ti and np.array_equal(got["kept"][b], tk)
            assert within_one_spacing(got["lp"][b], S.logprob(S.biased(rows[b], tables[0, 0]), ti, rec))


@pytest.mark.parametrize("V", VS)
def test_top_k_1_and_single_token(hip, golden, V):
    rows = regime_rows(golden, V)
    kinds = bias_kinds(V)
    rng = np.random.default_rng(V + 4)
    for name in ("allow7", "allow_half", "ban_last", "random"):
        bias = kinds[name]
        want = np.asarray([int(np.argmax(S.biased(r, bias))) for r in rows])             # the first maximum of the allowed tokens
        assert all(bias[w] != -np.inf for w in want)
        for u in (np.zeros(5, F32), np.full(5, U_LAST, F32), rng.random(5).astype(F32)):
            got = op_bias(hip, rows, np.stack([bias, bias])[None], [0] * 5, 1, [(1.0, 1.0, 1)], u=u)
            np.testing.assert_array_equal(got["idx"], want)
            assert (got["kept"].sum(1) == 1).all() and (got["lp"] == 0).all()
    one = kinds["allow1"]
    for recs in (None, [(1.7, 0.5, 3)]):
        for u in (np.zeros(5, F32), np.full(5, U_LAST, F32), rng.random(5).astype(F32)):
            got = op_bias(hip, rows, np.stack([one, one])[None], [0] * 5, 0, recs, u=u)
            assert (got["idx"] == V // 2).all() and (got["lp"] == 0).all() and (got["kept"].sum(1) == 1).all()


def test_chi_square_under_an_allow_list(hip, golden):
    """4 096 Philox draws from the real row under an allow-list of 40 codes (its 8 likeliest among them): Pearson chi-square over the
    allowed classes with expected count >= 5 (the rest pooled) against the renormalised float64 distribution, p > 1e-3 — the statistic and
    the bar of `test_op_sample_philox_chi_square`; 0 draws of banned tokens; and the draws are the twin's on the oracle's Philox uniforms."""
    from scipy import stats
    row = np.ascontiguousarray(golden("pix_full")["step_logits"][1, 7, 1])
    V = row.size
    rng = np.random.default_rng(21)
    allowed = np.zeros(V, bool)
    allowed[np.argsort(-row)[:8]] = True
    allowed[rng.choice(V, 32, replace=False)] = True
    bias = np.where(allowed, F32(0.0), F32(-np.inf)).astype(F32)
    nb, pos, seed = 4096, 15, 99
    ld = torch.from_numpy(np.tile(row, (nb, 1))).cuda()
    draws = op_bias(hip, ld, np.stack([bias, np.full(V, np.nan, F32)])[None], [0] * nb, 0, None, philox=(seed, 0, pos))["idx"]
    banned = int((~allowed[draws]).sum())
    assert banned == 0, f"{banned} draws of banned tokens"
    u = np.asarray([O.philox_uniform(seed, b, pos) for b in range(64)], F32)
    np.testing.assert_array_equal(draws[:64], S.sample_bias(np.tile(row, (64, 1)), u, None, np.stack([bias, bias])[None], [0] * 64, 0)[0])
    p = np.where(allowed, np.exp(row.astype(np.float64) - row.max()), 0.0)
    p /= p.sum()
    n = draws.size
    counts = np.bincount(draws, minlength=V).astype(np.float64)
    big = p * n >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(p[big] * n, p[~big].sum() * n)
    ok = exp > 0
    chi2, pval = stats.chisquare(obs[ok], exp[ok] * obs[ok].sum() / exp[ok].sum())
    print(f"\nallow-list of {allowed.sum()}: chi-square over {big.sum()} classes + pooled rest, {n} draws: {chi2:.1f}, p = {pval:.3f}")
    assert big.sum() >= 2 and pval > 1e-3


def test_errors_before_any_launch(hip):
    _lib, lib, ctx = hip
    V = 64
    ld = torch.zeros((5, V), dtype=torch.float32, device="cuda")
    idx = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    u = torch.zeros(5, dtype=torch.float32, device="cuda")
    td = torch.zeros((2, 2, V), dtype=torch.float32, device="cuda")
    i32p = _lib.C.POINTER(_lib.C.c_int32)

    def call(mode, index, n_bias=2, column=0):
        index = np.ascontiguousarray(index, np.int32)
        return lib.ts_op_sample_bias(ctx, _lib.dptr(ld), 5, V, mode, _lib.dptr(u), 0, 0, 0, None, 0, _lib.dptr(idx), None, None, None, None, None,
                                     None, _lib.dptr(td), n_bias, index.ctypes.data_as(i32p), column, None)
    assert call(_lib.TS_SAMPLE_GREEDY, [0] * 5) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_TEACHER_FORCED, [0] * 5) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [0, 1, 2, 0, 0]) != 0 and "clip 2" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [0, 1, -2, 0, 0]) != 0 and "clip 2" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [0] * 5, n_bias=6) != 0
    assert call(_lib.TS_SAMPLE_UNIFORMS, [0] * 5, column=2) != 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [0, 1, -1, 0, 0]) == 0
