"""The samplers under a repetition penalty as an operator (`ts_op_sample_repeat`; `csrc/vq.hip`: `sample_ctl_rep_kernel` and
`sample_ctl_rep_given_kernel`, the REP = true entries of `sample_ctl_body`) against the numpy twin (`talkshow_amd/sampling.py`:
`repeat_counts`, `penalised`, `sample_repeat`).  Codes, kept bytes and rings are compared for EQUALITY.  A log-probability is compared
twice: with the twin's (whose d_c and total are the device's bits; the two fp64 logs may differ in the last place: one fp32 spacing), and,
for rows under a neutral sampling record, with the float64 log-softmax of the penalised fp32 row within `sampling.logprob_error_bound`.
V = 2048 on aligned rows is the vector path, V = 300 the generic one (no multiple of 256).  Launches carry the five row regimes with five
different penalty records.  Every test fails on a build without the feature: the entry does not exist there.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [2048, 300]
NEUTRAL = (1.0, 1.0, 0)
U_LAST = F32(1.0 - 2.0 ** -24)
REPS = [(0, 3.0, 2.0), (1, 1e30, 0.0), (5, 0.7, 0.3), (64, -0.5, 0.1), (64, 0.0, 0.0)]
SAMPLING = [NEUTRAL, (0.7, 0.9, 0), (1.5, 1.0, 12)]
ROWS_R = [0, 1, 4, 63, 64, 65, 130]          # an empty history, partial ones, exactly full, wrapped, wrapped twice


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, (t, p, k) in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    return arr


def _rtable(_lib, reps):
    arr = (_lib.TsRepeat * len(reps))()
    for b, (w, p, f) in enumerate(reps):
        arr[b].window, arr[b].presence, arr[b].frequency, arr[b].reserved = w, p, f, 0
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


def ban_table(V):
    """(1, 2, V): a table that bans codes (a third of them, and the last three of the vocabulary in column 1) and moves the others."""
    rng = np.random.default_rng(7 + V)
    t = rng.standard_normal((1, 2, V)).astype(F32)
    t[0][rng.random((2, V)) < 0.33] = -np.inf
    t[0, 1, -3:] = -np.inf
    t[0, :, V // 2] = 0.25                            # the -inf regime row keeps its one sure finite logit
    return t


def histories(rows, V, r, rng):
    """(B, R) int32, R = min(r, 64), oldest first.  Row 0: codes in the first and the last token of a thread's chunk, its argmax among them;
    row 1: the last code of the vocabulary, the code before it and random ones; row 2: ONE code R times; row 3: the row's own likeliest
    codes; row 4: random codes and the row's one sure finite logit.  All in [0, V)."""
    B = rows.shape[0]
    R = min(r, 64)
    chunk = (V + 255) // 256
    h = np.zeros((B, R), np.int32)
    if R == 0:
        return h
    firsts = rng.integers(0, V // chunk, R) * chunk
    h[0] = np.where(np.arange(R) % 2 == 0, firsts, np.minimum(firsts + chunk - 1, V - 1))
    h[0, R // 2] = int(np.argmax(rows[0]))
    h[1] = rng.integers(0, V, R)
    h[1, ::3] = V - 1
    h[1, -1] = V - 2
    h[2] = int(np.argmax(rows[2]) + 5) % V
    top = np.argsort(-rows[3], kind="stable")[:6]
    h[3] = top[rng.integers(0, 6, R)]
    h[4] = rng.integers(0, V, R)
    h[4, 0] = V // 2
    return h


def op_repeat(hip, logits, reps, hist, position, column, recs=None, u=None, philox=None, tables=None, index=None, given_rows=None, keep=None,
              given=None, want_lp=True, want_copy=False, entry="repeat"):
    """One launch -> dict(idx, kept (B,V) uint8, lp (B,) or None, ring (B,64), copy).  entry="bias": `ts_op_sample_bias` on the same arguments."""
    _lib, lib, ctx = hip
    ld = logits if torch.is_tensor(logits) else torch.from_numpy(np.ascontiguousarray(logits, F32)).cuda()
    B, V = ld.shape
    td = None if tables is None else torch.from_numpy(np.ascontiguousarray(tables, F32)).cuda()
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((B, V), 9, dtype=torch.uint8, device="cuda")
    lp = torch.full((B,), 7.0, dtype=torch.float32, device="cuda") if want_lp else None
    copy = torch.full((B, V), 3.0, dtype=torch.float32, device="cuda") if want_copy else None
    ring = torch.full((B, 64), -9, dtype=torch.int32, device="cuda")
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    seed, clip0 = philox if philox is not None else (0, 0)
    mode = _lib.TS_SAMPLE_UNIFORMS if u is not None else _lib.TS_SAMPLE_PHILOX
    i32p = _lib.C.POINTER(_lib.C.c_int32)
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    gr = None if given_rows is None else np.ascontiguousarray(given_rows, np.int32)
    kd = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda()
    gd = None if given is None else torch.from_numpy(np.ascontiguousarray(given, np.int64)).cuda()
    hd = None if hist is None or hist.shape[1] == 0 else torch.from_numpy(np.ascontiguousarray(hist, np.int32)).cuda()
    head = (ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, int(position), None if recs is None else _table(_lib, recs),
            0 if recs is None else len(recs), _lib.dptr(idx), _lib.dptr(lp), None if gr is None else gr.ctypes.data_as(i32p), _lib.dptr(kd),
            _lib.dptr(gd), _lib.dptr(kept), _lib.dptr(copy), _lib.dptr(td), 0 if td is None else int(td.shape[0]),
            None if index is None else index.ctypes.data_as(i32p), int(column))
    if entry == "bias":
        _lib.check(lib.ts_op_sample_bias(*head, None))
    else:
        _lib.check(lib.ts_op_sample_repeat(*head, _rtable(_lib, reps), len(reps), _lib.dptr(hd), _lib.dptr(ring), None))
    return dict(idx=idx.cpu().numpy(), kept=kept.cpu().numpy(), lp=None if lp is None else lp.cpu().numpy(), ring=ring.cpu().numpy(),
                copy=None if copy is None else copy.cpu().numpy())


def within_one_spacing(got, want):
    if np.isinf(want) or np.isnan(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.abs(F32(want))))


def penalised_row(row, bias, rep, hist):
    lb = S.biased(row, bias)
    return S.penalised(lb, S.repeat_counts(hist, row.size, rep[0]), rep) if rep[0] > 0 else lb


def check_against_exact(V, lpen, code, got_lp, what):
    """A neutral sampling record: the float64 log-softmax of the penalised fp32 row, within the derived bound."""
    x = lpen.astype(np.float64)
    with np.errstate(divide="ignore"):
        ref = x[code] - x.max() - np.log(np.exp(x - x.max()).sum())
    bound = S.logprob_error_bound(V, lpen[code] - lpen.max(), ref)
    assert abs(float(got_lp) - ref) <= bound, f"{what}: |{got_lp} - {ref}| > {bound:.3e}"


@pytest.mark.parametrize("V", VS)
def test_twin_grid(hip, golden, V):
    """The full cross: 7 rows r x 3 sampling records x with / without a table that bans codes x the 5 rotations of the five penalty
    records over the five row regimes, so every regime meets every (penalty record, sampling record, table or none) at every r; the
    columns alternate; u rotates through 0, 1 - 2^-24 and random."""
    rows = regime_rows(golden, V)
    B = rows.shape[0]
    ld = torch.from_numpy(rows).cuda()
    tables = ban_table(V)
    rng = np.random.default_rng(V + 1)
    special = [0.0, float(U_LAST), 0.5]
    n = 0
    moved = 0
    for r in ROWS_R:
        hist = histories(rows, V, r, rng)
        for rec, with_bias, rot in itertools.product(SAMPLING, (False, True), range(len(REPS))):
            column = n % 2
            reps = [REPS[(rot + b) % len(REPS)] for b in range(B)]
            recs = [rec] * B
            u = np.asarray([special[(n + b) % 3] if (n + b) % 2 == 0 else rng.random() for b in range(B)], F32)
            got = op_repeat(hip, ld, reps, hist, 2 * r + column, column, recs, u=u, tables=tables if with_bias else None,
                            index=[0] * B if with_bias else None, want_copy=(n % 11 == 0))
            ti, tk, tl, tring = S.sample_repeat(rows, u, recs, reps, hist, 2 * r + column, tables if with_bias else None,
                                                [0] * B if with_bias else None, column)
            what = f"V {V} r {r} column {column} record {rec} bias {with_bias} launch {n}"
            np.testing.assert_array_equal(got["idx"], ti, err_msg=what)
            np.testing.assert_array_equal(got["ring"], tring, err_msg=what)
            np.testing.assert_array_equal(got["kept"].astype(bool), tk, err_msg=what)
            if got["copy"] is not None:
                assert np.array_equal(got["copy"].view(np.uint32), rows.view(np.uint32)), f"{what}: the logits copy is the network's row"
            for b in range(B):
                bias = tables[0, column] if with_bias else None
                lpen = penalised_row(rows[b], bias, reps[b], hist[b])
                kept_def = S.keep_mask_bias(lpen, rec, None) & ((lpen != -np.inf) if with_bias else True)      # keep_mask_bias on l''
                assert np.array_equal(tk[b], kept_def)
                assert tk[b][ti[b]] and lpen[ti[b]] != -np.inf
                assert within_one_spacing(got["lp"][b], tl[b]), f"{what} row {b}: logprob {got['lp'][b]} twin {tl[b]}"
                if rec == NEUTRAL:
                    check_against_exact(V, lpen, int(ti[b]), got["lp"][b], f"{what} row {b}")
                plain = S.draw(S.biased(rows[b], bias), u[b], rec[0], S.keep_mask_bias(rows[b], rec, bias))
                moved += int(plain != ti[b])
            n += 1
    assert moved > 50, f"the penalty changed only {moved} draws of the grid: the histories do not bite"


@pytest.mark.parametrize("V", VS)
def test_no_repeat_and_hold(hip, golden, V):
    """presence = 1e30 over a full window: the draw is none of the 64 codes of the history (their weight is 0, and a crossing is a token of
    positive weight; u = 1 - 2^-24, where the fallbacks of step 5 may return a kept token of weight 0, is the header's stated exception and
    is left to the twin grid); the opposite sign on a flat row returns a code of the history."""
    rows = regime_rows(golden, V)
    rng = np.random.default_rng(V + 3)
    r = 64
    hist = np.stack([rng.choice(V, 64, replace=False) for _ in range(5)]).astype(np.int32)
    hist[4, 0] = V // 2                                                   # the -inf row: even its surest code is avoided
    for u in (np.zeros(5, F32), np.full(5, 0.999, F32), rng.random(5).astype(F32)):
        got = op_repeat(hip, rows, [(64, 1e30, 0.0)], hist, 2 * r, 0, None, u=u)
        for b in range(5):
            assert got["idx"][b] not in set(hist[b].tolist()), f"row {b}: code {got['idx'][b]} is in the window"
            assert np.isfinite(got["lp"][b])
        got = op_repeat(hip, rows[1:3], [(64, -1e30, 0.0)], hist[1:3], 2 * r, 0, None, u=u[1:3])
        for b in range(2):
            assert got["idx"][b] in set(hist[1 + b].tolist())


@pytest.mark.parametrize("V", VS)
def test_window_zero_is_the_bias_launch(hip, golden, V):
    """A launch whose records all have window 0 returns `ts_op_sample_bias`'s bits — index, kept bytes, log-probability bits — and leaves
    the rings as the history left them; a launch of (64, +0, +0) returns the same index and log-probability bits too."""
    rows = regime_rows(golden, V)
    rows[2] = np.random.default_rng(V).standard_normal(V).astype(F32)
    rows[2, 5] = F32(-0.0)
    tables = ban_table(V)
    rng = np.random.default_rng(V + 5)
    r = 70
    hist = histories(rows, V, r, rng)
    hist[2, -3:] = 5                                                       # the -0 logit is met by the window
    recs = [(0.7, 0.9, 0), NEUTRAL, (1.7, 1.0, 40), (1.0, 0.95, 0), NEUTRAL]
    for index in ([0] * 5, [-1, 0, -1, 0, -1]):
        for u in (np.zeros(5, F32), np.full(5, U_LAST, F32), rng.random(5).astype(F32)):
            want = op_repeat(hip, rows, None, None, 2 * r + 1, 1, recs, u=u, tables=tables, index=index, entry="bias")
            got = op_repeat(hip, rows, [(0, 1e30, 1e30)], hist, 2 * r + 1, 1, recs, u=u, tables=tables, index=index)
            assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["kept"], want["kept"])
            assert np.array_equal(got["lp"].view(np.uint32), want["lp"].view(np.uint32))
            ring = np.empty((5, 64), np.int32)
            for i in range(64):
                ring[:, (r - 64 + i) & 63] = hist[:, i]
            assert np.array_equal(got["ring"], ring), "a window of 0 writes no ring entry"
            zero = op_repeat(hip, rows, [(64, 0.0, 0.0)], hist, 2 * r + 1, 1, recs, u=u, tables=tables, index=index)
            assert np.array_equal(zero["idx"], want["idx"]) and np.array_equal(zero["lp"].view(np.uint32), want["lp"].view(np.uint32))
            ring[:, r & 63] = want["idx"]
            assert np.array_equal(zero["ring"], ring)


@pytest.mark.parametrize("V", VS)
def test_philox(hip, golden, V):
    """Philox once: the launch draws the twin's codes on the oracle's uniforms of (seed, clip, position): the random stream does not
    depend on the record."""
    rows = regime_rows(golden, V)
    rng = np.random.default_rng(V + 6)
    r, column, seed, clip0 = 65, 1, 99, 40
    hist = histories(rows, V, r, rng)
    reps = REPS
    got = op_repeat(hip, rows, reps, hist, 2 * r + column, column, [(0.9, 0.95, 0)] * 5, philox=(seed, clip0))
    u = np.asarray([O.philox_uniform(seed, clip0 + b, 2 * r + column) for b in range(5)], F32)
    ti, tk, tl, tring = S.sample_repeat(rows, u, [(0.9, 0.95, 0)] * 5, reps, hist, 2 * r + column, column=column)
    np.testing.assert_array_equal(got["idx"], ti)
    np.testing.assert_array_equal(got["ring"], tring)
    np.testing.assert_array_equal(got["kept"].astype(bool), tk)


@pytest.mark.parametrize("want_lp", [True, False])
@pytest.mark.parametrize("V", VS)
def test_given_variants(hip, golden, V, want_lp):
    """The given variant at r = 65 (position 131, column 1).  Row 0: forced (G = 70), a code of its history; row 1: forced, a code outside
    the vocabulary (the ring receives -1, the log-probability NaN); row 2: forced on paper, mask byte 0: drawn under the penalty; row 3:
    G = 65, the position is not below 2 G: drawn; row 4: forced, a code the table bans: taken, -inf.  With and without a log-probability
    output (without it a forced workgroup returns ahead of everything and still writes its ring entry)."""
    rows = regime_rows(golden, V)
    tables = ban_table(V)
    rng = np.random.default_rng(V + 8)
    r, column = 65, 1
    hist = histories(rows, V, r, rng)
    banned = int(np.flatnonzero(tables[0, column] == -np.inf)[0])
    given = np.asarray([int(hist[0, -1]), 2 ** 40, 11, 12, banned], np.int64)
    G = [70, 66, 70, 65, 66]
    keep = [1, 1, 0, 1, 1]
    forced = [True, True, False, False, True]
    reps = [(5, 0.7, 0.3), (64, 1.0, 0.0), (5, 0.7, 0.3), (64, -0.5, 0.1), (3, 0.5, 0.5)]
    u = rng.random(5).astype(F32)
    for recs in (None, [(0.8, 0.9, 0)] * 5):
        got = op_repeat(hip, rows, reps, hist, 2 * r + column, column, recs, u=u, tables=tables, index=[0] * 5, given_rows=G, keep=keep,
                        given=given, want_lp=want_lp)
        ti, tk, tl, tring = S.sample_repeat(rows, u, recs, reps, hist, 2 * r + column, tables, [0] * 5, column, given=given, forced=forced)
        np.testing.assert_array_equal(got["idx"], ti)
        np.testing.assert_array_equal(got["ring"], tring)
        assert got["idx"][0] == given[0] and got["idx"][1] == 2 ** 40 and got["idx"][4] == banned
        assert tring[1, r & 63] == -1 and tring[0, r & 63] == given[0]
        for b in range(5):
            if want_lp or not forced[b]:
                assert np.array_equal(got["kept"][b].astype(bool), tk[b]), f"row {b}"
        if want_lp:
            assert np.isnan(got["lp"][1]) and got["lp"][4] == -np.inf
            for b in (0, 2, 3):
                assert within_one_spacing(got["lp"][b], tl[b]), f"row {b}: {got['lp'][b]} twin {tl[b]}"
            # the forced code of row 0 is in its window: it is scored under the PENALISED distribution
            rec = NEUTRAL if recs is None else recs[0]
            unpen = S.given_logprob_bias(rows[0], int(given[0]), rec, tables[0, column])
            if np.isfinite(tl[0]) and np.isfinite(unpen):
                assert tl[0] != unpen


def test_errors_before_any_launch(hip):
    _lib, lib, ctx = hip
    V = 64
    ld = torch.zeros((5, V), dtype=torch.float32, device="cuda")
    idx = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    u = torch.zeros(5, dtype=torch.float32, device="cuda")
    hd = torch.zeros((5, 64), dtype=torch.int32, device="cuda")

    def call(mode, reps, n=None, position=200, hist=hd):
        arr = _rtable(_lib, reps)
        return lib.ts_op_sample_repeat(ctx, _lib.dptr(ld), 5, V, mode, _lib.dptr(u), 0, 0, position, None, 0, _lib.dptr(idx), None, None, None, None,
                                       None, None, None, 0, None, 0, arr, len(reps) if n is None else n, _lib.dptr(hist), None, None)
    ok = (5, 1.0, 0.0)
    assert call(_lib.TS_SAMPLE_GREEDY, [ok]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_TEACHER_FORCED, [ok]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok, ok, (65, 0.0, 0.0), ok, ok]) != 0 and "clip 2" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok, ok, ok, (3, float("nan"), 0.0), ok]) != 0 and "clip 3" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok, ok]) != 0                    # 1 or B records
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok], hist=None) != 0             # rows behind row 0 need their history
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok]) == 0
    assert call(_lib.TS_SAMPLE_UNIFORMS, [ok], position=1, hist=None) == 0
