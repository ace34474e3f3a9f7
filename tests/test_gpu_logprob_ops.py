"""The samplers' log-probability output as an operator (`ts_op_sample_lp`; `csrc/vq.hip`: `sample_lp_kernel` without a table, the `LP`
instantiation of `sample_plain_body`; `sample_ctl_kernel<., true>` with one, the `LP` instantiations of `sample_ctl_body`) and
`ts_logprob_sums`, against the existing entries and the numpy restatement
(`talkshow_amd/sampling.py::logprob`, `logprob_sums`).

Codes equal the existing entries' codes EXACTLY.  A log-probability may differ from the restatement by one fp32 spacing and no more: S and
d_c are bit-equal, the two fp64 logs may differ in their last place.  Where the rule says equal — a neutral record against no record,
top_k = 1 — the comparison is equality.  Shapes: V = 2048 (the 16-byte loads), 1000 (chunks of 4, the last threads own nothing), 256 (chunks
of 1), 7 (fewer tokens than threads); B = 1 and 5.  The output sits between two 4 KiB zones of sentinels, which stay intact.
Every test fails on a build without the feature: the entries do not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from test_logprob_host import special_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [2048, 1000, 256, 7]
NEUTRAL = (1.0, 1.0, 0)
RECORDS = [None, NEUTRAL, (0.7, 0.9, 0), (1.0, 1.0, 1), (2.5, 0.6, 30)]
U_LAST = F32(1.0) - F32(2.0 ** -24)
ZONE = 1024                                           # floats: 4 KiB on either side of the output
SENTINEL = F32(-1.2345678e30)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, (t, p, k) in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    return arr


def op_lp(hip, ld, mode, rec=None, u=None, philox=(0, 0, 0), codes=None, want_lp=True):
    """One `ts_op_sample_lp` launch on ld (B,V) device logits: -> (idx (B,) int64, logprob (B,) float32).  rec: None = no table, one record
    for all rows, or a list of B.  The output's sentinel zones are checked here."""
    _lib, lib, ctx = hip
    B, V = ld.shape
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda") if codes is None else torch.from_numpy(np.asarray(codes, np.int64)).cuda()
    buf = torch.full((2 * ZONE + B,), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = buf[ZONE:ZONE + B]
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    tab, n = (None, 0)
    if rec is not None:
        recs = rec if isinstance(rec, list) else [rec]
        tab, n = _table(_lib, recs), len(recs)
    _lib.check(lib.ts_op_sample_lp(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), philox[0], philox[1], philox[2], tab, n, _lib.dptr(idx), None,
                                   _lib.dptr(out) if want_lp else None, None))
    host = buf.cpu().numpy()
    assert np.all(host[:ZONE] == SENTINEL) and np.all(host[ZONE + B:] == SENTINEL), "a sentinel zone around the output was written"
    return idx.cpu().numpy(), host[ZONE:ZONE + B].copy()


def assert_within_one_spacing(got, want, msg):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), msg
    ok = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64)) <= np.spacing(np.abs(want[~nan])).astype(np.float64)
    assert ok.all(), f"{msg}: device {got[~nan][~ok][:4]} restatement {want[~nan][~ok][:4]}"


def batch(V, B):
    rows = special_rows(V)
    names = ["random1", "dominant", "ties", "zeros", "equal"][:B]
    return np.ascontiguousarray(np.stack([rows[n] for n in names]), F32)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", VS)
def test_modes_without_a_table(hip, V, B):
    """Greedy, injected uniforms and Philox: the codes of ts_op_sample / ts_op_sample_philox, the restatement's log-probability of them."""
    _lib, lib, ctx = hip
    rows = batch(V, B)
    ld = torch.from_numpy(rows).cuda()
    plain = torch.empty(B, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(V + B)

    def check(idx, lp, what):
        np.testing.assert_array_equal(idx, plain.cpu().numpy(), err_msg=what)
        assert_within_one_spacing(lp, [S.logprob(rows[b], idx[b]) for b in range(B)], f"V {V} B {B} {what}")
    _lib.check(lib.ts_op_sample(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_GREEDY, None, _lib.dptr(plain), None))
    check(*op_lp(hip, ld, _lib.TS_SAMPLE_GREEDY), "greedy")
    for u in (np.zeros(B, F32), np.full(B, U_LAST, F32), rng.random(B).astype(F32)):
        ud = torch.from_numpy(u).cuda()
        _lib.check(lib.ts_op_sample(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_UNIFORMS, _lib.dptr(ud), _lib.dptr(plain), None))
        check(*op_lp(hip, ld, _lib.TS_SAMPLE_UNIFORMS, u=u), f"uniforms {u[:2]}")
    for philox in ((99, 0, 15), (2 ** 40 + 3, 2 ** 33, 149)):
        _lib.check(lib.ts_op_sample_philox(ctx, _lib.dptr(ld), B, V, *philox, _lib.dptr(plain), None))
        check(*op_lp(hip, ld, _lib.TS_SAMPLE_PHILOX, philox=philox), f"philox {philox}")
    # a NULL output: the sampler of the entry it extends
    _lib.check(lib.ts_op_sample_philox(ctx, _lib.dptr(ld), B, V, 99, 0, 15, _lib.dptr(plain), None))
    idx, lp = op_lp(hip, ld, _lib.TS_SAMPLE_PHILOX, philox=(99, 0, 15), want_lp=False)
    np.testing.assert_array_equal(idx, plain.cpu().numpy())
    assert np.all(lp == SENTINEL)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", VS)
def test_teacher_forced(hip, V, B):
    """Given codes, among them index 0, V - 1 and one outside [0, V): NaN at that position, every other element the restatement's; the
    codes are left as they are."""
    _lib, lib, ctx = hip
    rows = batch(V, B)
    ld = torch.from_numpy(rows).cuda()
    rng = np.random.default_rng(7 * V + B)
    for oob in (V, -1, 2 ** 40 + 3, -2 ** 33):      # just past the end, negative, and values whose low 32 bits are valid indices
        if B == 5:
            cases = [np.asarray([0, V - 1, oob, int(rng.integers(0, V)), int(rows[4].argmax())], np.int64)]
        else:
            cases = [np.asarray([c], np.int64) for c in (0, V - 1, oob)]
        for codes in cases:
            idx, lp = op_lp(hip, ld, _lib.TS_TEACHER_FORCED, codes=codes)
            np.testing.assert_array_equal(idx, codes)
            want = [S.logprob(rows[b], codes[b]) for b in range(B)]
            assert_within_one_spacing(lp, want, f"V {V} B {B} codes {codes}")
            assert np.isnan(lp).sum() == sum(not 0 <= int(c) < V for c in codes)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", VS)
def test_records_on_the_special_rows(hip, V, B):
    """No record, neutral, (0.7, 0.9, 0), (1, 1, 1), (2.5, 0.6, 30) on the special rows, u = 0, 1 - 2^-24 and a random one, and Philox."""
    _lib, lib, ctx = hip
    rows = batch(V, B)
    ld = torch.from_numpy(rows).cuda()
    rng = np.random.default_rng(3 * V + B)
    base = {}
    for u in (np.zeros(B, F32), np.full(B, U_LAST, F32), rng.random(B).astype(F32), None):
        philox = (1234, 5, 17)
        mode = _lib.TS_SAMPLE_PHILOX if u is None else _lib.TS_SAMPLE_UNIFORMS
        for rec in RECORDS:
            idx, lp = op_lp(hip, ld, mode, rec=rec, u=u, philox=philox)
            if rec is not None:                      # the codes of the existing entry
                ref = torch.empty(B, dtype=torch.int64, device="cuda")
                ud = None if u is None else torch.from_numpy(u).cuda()
                _lib.check(lib.ts_op_sample_ctl(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), *philox, _table(_lib, [rec]), 1, _lib.dptr(ref),
                                                None, None))
                np.testing.assert_array_equal(idx, ref.cpu().numpy())
            want = [S.logprob(rows[b], idx[b], rec) for b in range(B)]
            assert_within_one_spacing(lp, want, f"V {V} B {B} record {rec} u {None if u is None else u[:2]}")
            if rec is None:
                base = dict(idx=idx, lp=lp)
            elif rec == NEUTRAL:                     # equal to the path without a record, codes and log-probabilities
                np.testing.assert_array_equal(idx, base["idx"])
                assert np.array_equal(lp, base["lp"]), f"neutral record: {lp} against {base['lp']}"
            elif rec[2] == 1:                        # top_k = 1: the argmax, log-probability exactly 0
                np.testing.assert_array_equal(idx, [int(np.flatnonzero(r == r.max())[0]) for r in rows])
                assert np.all(lp == 0.0)
    # one record per row in one launch
    if B == 5:
        recs = [NEUTRAL, (0.7, 0.9, 0), (1.0, 1.0, 1), (2.5, 0.6, 30), (0.5, 0.5, 3)]
        u = rng.random(B).astype(F32)
        idx, lp = op_lp(hip, ld, _lib.TS_SAMPLE_UNIFORMS, rec=recs, u=u)
        assert_within_one_spacing(lp, [S.logprob(rows[b], idx[b], recs[b]) for b in range(B)], f"V {V} per-row records")


def test_underflow_row_gives_the_finite_argument(hip):
    """A row whose other weights underflow: 0.0 for the maximum and the finite d_c for any other code; d_c is used, never log(w_c)."""
    _lib, lib, ctx = hip
    V = 2048
    row = special_rows(V)["dominant"]
    ld = torch.from_numpy(np.ascontiguousarray(row[None])).cuda()
    top = int(row.argmax())
    for c in (top, 0, V - 1, top + 1):
        _, lp = op_lp(hip, ld, _lib.TS_TEACHER_FORCED, codes=np.asarray([c]))
        assert lp[0] == F32(row[c] - row[top]) and np.isfinite(lp[0])
    _, lp = op_lp(hip, ld, _lib.TS_SAMPLE_GREEDY)
    assert lp[0] == 0.0


def test_refusals(hip):
    _lib, lib, ctx = hip
    ld = torch.zeros((2, 16), dtype=torch.float32, device="cuda")
    idx = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((2,), 5.0, dtype=torch.float32, device="cuda")
    tab = _table(_lib, [NEUTRAL])
    for mode in (_lib.TS_TEACHER_FORCED, _lib.TS_SAMPLE_GREEDY):      # a table needs a mode that draws
        assert lib.ts_op_sample_lp(ctx, _lib.dptr(ld), 2, 16, mode, None, 0, 0, 0, tab, 1, _lib.dptr(idx), None, _lib.dptr(lp), None) != 0
        assert "top_k = 1" in lib.ts_last_error().decode()
    assert lib.ts_op_sample_lp(ctx, _lib.dptr(ld), 2, 16, _lib.TS_SAMPLE_UNIFORMS, None, 0, 0, 0, None, 0, _lib.dptr(idx), None, _lib.dptr(lp), None) != 0
    assert lib.ts_op_sample_lp(ctx, _lib.dptr(ld), 2, 16, 9, None, 0, 0, 0, None, 0, _lib.dptr(idx), None, _lib.dptr(lp), None) != 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all() and (lp.cpu().numpy() == 5.0).all()


@pytest.mark.parametrize("H", [1, 9])
@pytest.mark.parametrize("B", [1, 5])
def test_logprob_sums_equal_the_restatement(hip, B, H):
    _lib, lib, ctx = hip
    rng = np.random.default_rng(10 * B + H)
    lp = (-9.0 * rng.random((B, H, 2))).astype(F32)
    rows = [H] + [int(rng.integers(0, H + 1)) for _ in range(B - 1)]      # a table that ends clips early (0 rows included)
    if B == 5:
        rows[1], rows[2] = 0, max(H - 1, 0)
        lp[2, rows[2]:] = np.nan                                         # beyond the clip's rows: must not enter
    ld = torch.from_numpy(lp).cuda()
    for table in (None, rows):
        if table is None and B == 5:
            ld2 = torch.from_numpy(np.nan_to_num(lp, nan=-1.0)).cuda()
            src, ref = ld2, S.logprob_sums(np.nan_to_num(lp, nan=-1.0))
        else:
            src, ref = ld, S.logprob_sums(lp, table)
        lens = None if table is None else torch.from_numpy(np.asarray(table, np.int32) * 4 + 3).cuda()   # MFCC frames: H_b = lens >> 2
        buf = torch.full((B * 3 + 1024,), 7.5, dtype=torch.float64, device="cuda")
        out = buf[512:512 + 3 * B]
        _lib.check(lib.ts_logprob_sums(ctx, _lib.dptr(src), _lib.dptr(lens), B, H, _lib.dptr(out), None))
        host = buf.cpu().numpy()
        assert np.all(host[:512] == 7.5) and np.all(host[512 + 3 * B:] == 7.5)
        got = host[512:512 + 3 * B].reshape(B, 3)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"B {B} H {H} table {table}: {got} against {ref}"


def test_logprob_sums_more_rows_than_lanes(hip):
    """H = 600: every lane adds two or three rows before the lane sums are added."""
    _lib, lib, ctx = hip
    rng = np.random.default_rng(3)
    lp = (-9.0 * rng.random((2, 600, 2))).astype(F32)
    ld = torch.from_numpy(lp).cuda()
    rows = [600, 257]
    lens = torch.from_numpy(np.asarray(rows, np.int32) * 4).cuda()
    out = torch.empty((2, 3), dtype=torch.float64, device="cuda")
    _lib.check(lib.ts_logprob_sums(ctx, _lib.dptr(ld), _lib.dptr(lens), 2, 600, _lib.dptr(out), None))
    assert np.array_equal(out.cpu().numpy().view(np.uint64), S.logprob_sums(lp, rows).view(np.uint64))
