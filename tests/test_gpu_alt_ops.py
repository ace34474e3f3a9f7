"""The samplers with alternatives as an operator (`ts_op_sample_alt`; `csrc/vq.hip`: `sample_ctl_alt_kernel` and
`sample_ctl_alt_given_kernel`, the ALT = true entries of `sample_ctl_body`) against the numpy restatement
(`talkshow_amd/sampling.py::alternatives`).  Alternative codes and ranks are compared for EQUALITY.  S_all, E and every d_j are the
device's bits by construction, so a log-probability and the entropy are the restatement's value or an adjacent float32: one fp32 spacing
and no more (the two fp64 logs may differ in the last place; the allowance and the reason of tests/test_gpu_logprob_ops.py).  With no
tolerance at all: idx and logprob are `ts_op_sample_repeat`'s on the same arguments; where no filter is in force and rank < n,
alt_logprob[rank] has the bits of logprob; under top_k = 1, alt_code[0] is idx.  All four outputs sit between 4 KiB red zones.
V = 2048 on aligned rows is the vector path; 2047, 256, 5 and 1 the generic one.  Every test fails on a build without the feature: the
entry does not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [2048, 2047, 256, 5, 1]
NS = [0, 1, 3, 8]
B = 5
NEUTRAL = (1.0, 1.0, 0)
RECORDS = [NEUTRAL, (0.5, 1.0, 0), (1.0, 1.0, 1), (0.8, 0.9, 12)]
ZONE = 1024            # 4 KiB of 32-bit words on either side of every output


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


def gaussian_rows(V):
    rng = np.random.default_rng(900 + V)
    return np.ascontiguousarray(rng.standard_normal((B, V)) * np.array([[0.01], [1.0], [3.0], [20.0], [200.0]]), F32)


def special_rows(V):
    """All equal; ties across thread-chunk borders (equal values at indices 7, 8 and V - 1, above everything else); mixed +0 / -0; an
    underflowing row (most weights below e^-86); a Gaussian."""
    rng = np.random.default_rng(901 + V)
    rows = np.zeros((B, V), F32)
    rows[0] = 1.25
    rows[1] = rng.standard_normal(V).astype(F32)
    for i in (7, 8, V - 1):
        rows[1, min(i, V - 1)] = 6.5
    rows[2] = np.where(rng.random(V) < 0.5, F32(0.0), F32(-0.0))
    rows[3] = (-100.0 * rng.random(V) - 90.0).astype(F32)
    rows[3, V // 2] = 0.0
    rows[3, V // 3] = -1.0
    rows[4] = rng.standard_normal(V).astype(F32)
    return rows


class Zoned:
    """A device array between two red zones of ZONE words."""

    def __init__(self, count, dtype, fill):
        self.count, self.fill = count, fill
        self.full = torch.full((count + 2 * ZONE,), fill, dtype=dtype, device="cuda")

    def ptr(self):
        return self.full.data_ptr() + 4 * ZONE

    def get(self, shape):
        got = self.full.cpu().numpy()
        assert (got[:ZONE] == self.fill).all() and (got[ZONE + self.count:] == self.fill).all(), "a red zone was written"
        return got[ZONE:ZONE + self.count].reshape(shape)


def op_alt(hip, logits, n, recs, reps, hist, position, u, column=0, tables=None, index=None, given_rows=None, given=None, entry="alt"):
    """One launch of `ts_op_sample_alt` (entry="repeat": `ts_op_sample_repeat` on the same arguments) -> dict of numpy arrays."""
    _lib, lib, ctx = hip
    C = _lib.C
    ld = torch.from_numpy(np.ascontiguousarray(logits, F32)).cuda()
    nb, V = ld.shape
    td = None if tables is None else torch.from_numpy(np.ascontiguousarray(tables, F32)).cuda()
    idx = torch.full((nb,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((nb,), 7.0, dtype=torch.float32, device="cuda")
    ring = torch.full((nb, 64), -9, dtype=torch.int32, device="cuda")
    ud = torch.from_numpy(np.ascontiguousarray(u, F32)).cuda()
    i32p = C.POINTER(C.c_int32)
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    gr = None if given_rows is None else np.ascontiguousarray(given_rows, np.int32)
    gd = None if given is None else torch.from_numpy(np.ascontiguousarray(given, np.int64)).cuda()
    hd = None if hist is None or hist.shape[1] == 0 else torch.from_numpy(np.ascontiguousarray(hist, np.int32)).cuda()
    head = (ctx, _lib.dptr(ld), nb, V, _lib.TS_SAMPLE_UNIFORMS, _lib.dptr(ud), 0, 0, int(position), _table(_lib, recs), len(recs), _lib.dptr(idx),
            _lib.dptr(lp), None if gr is None else gr.ctypes.data_as(i32p), None, _lib.dptr(gd), None, None, _lib.dptr(td),
            0 if td is None else int(td.shape[0]), None if index is None else index.ctypes.data_as(i32p), int(column), _rtable(_lib, reps), len(reps),
            _lib.dptr(hd), _lib.dptr(ring))
    out = {}
    if entry == "repeat":
        _lib.check(lib.ts_op_sample_repeat(*head, None))
    else:
        zc, zl = Zoned(nb * n, torch.int32, -77), Zoned(nb * n, torch.float32, 77.0)
        ze, zr = Zoned(nb, torch.float32, 77.0), Zoned(nb, torch.int32, -77)
        rec = _lib.TsAltOut(n, 0, zc.ptr() if n else None, zl.ptr() if n else None, ze.ptr(), zr.ptr())
        _lib.check(lib.ts_op_sample_alt(*head, C.byref(rec), None))
        out.update(codes=zc.get((nb, n)), alt_lp=zl.get((nb, n)), entropy=ze.get((nb,)), rank=zr.get((nb,)))
    out.update(idx=idx.cpu().numpy(), lp=lp.cpu().numpy(), ring=ring.cpu().numpy())
    return out


def one_spacing(got, want):
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    inf = np.isinf(want)
    ok = np.abs(got[~inf].astype(np.float64) - want[~inf].astype(np.float64)) <= np.spacing(np.abs(want[~inf])).astype(np.float64)
    return (got[inf] == want[inf]).all() and ok.all()


def check_launch(hip, rows, n, recs, reps, hist, position, column=0, tables=None, index=None, given_rows=None, given=None, forced=None, what=""):
    V = rows.shape[1]
    u = np.random.default_rng(17).random(rows.shape[0]).astype(F32)
    args = dict(column=column, tables=tables, index=index, given_rows=given_rows, given=given)
    got = op_alt(hip, rows, n, recs, reps, hist, position, u, **args)
    ref = op_alt(hip, rows, n, recs, reps, hist, position, u, entry="repeat", **args)
    assert np.array_equal(got["idx"], ref["idx"]), what
    assert np.array_equal(got["lp"].view(np.uint32), ref["lp"].view(np.uint32)), what
    assert np.array_equal(got["ring"], ref["ring"]), what
    for b in range(rows.shape[0]):
        t = -1 if index is None else int(index[b])
        bias = None if t < 0 else np.asarray(tables, F32)[t, column]
        counts = None if hist is None else S.repeat_counts(hist[b], V, reps[b][0])
        want = S.alternatives(rows[b], recs[b], n, bias=bias, counts=counts, rep=reps[b], code=int(got["idx"][b]))
        msg = f"{what} V {V} n {n} row {b} record {recs[b]}"
        assert np.array_equal(got["codes"][b], want.codes), msg
        assert int(got["rank"][b]) == want.rank, msg
        assert one_spacing(got["alt_lp"][b], want.logprobs), (msg, got["alt_lp"][b], want.logprobs)
        assert one_spacing(got["entropy"][b], want.entropy), (msg, got["entropy"][b], want.entropy)
        is_forced = forced is not None and forced[b]
        if is_forced:
            assert int(got["idx"][b]) == int(given[b]), msg
        _, top_p, top_k = recs[b]
        filtered = (1 <= top_k < V) or top_p < 1.0
        r = int(got["rank"][b])
        if not filtered and 0 <= r < n:      # no filter in force: the S of "log-probabilities" is S_all, bit for bit
            assert got["alt_lp"][b, r].view(np.uint32) == got["lp"][b].view(np.uint32), msg
        if top_k == 1 and n > 0 and not is_forced:
            assert int(got["codes"][b, 0]) == int(got["idx"][b]), msg
    return got


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", VS)
def test_rows_and_records(hip, V, n):
    """Gaussian and special rows under every record, no table, no history."""
    reps = [(0, 0.0, 0.0)] * B
    for rows, name in ((gaussian_rows(V), "gaussian"), (special_rows(V), "special")):
        for rec in RECORDS:
            check_launch(hip, rows, n, [rec] * B, reps, None, 0, what=f"{name} rows")
    check_launch(hip, gaussian_rows(V), n, [RECORDS[b % 4] for b in range(B)], reps, None, 0, what="per-row records")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", VS)
def test_bias_leaves_two_tokens(hip, V, n):
    """A table that leaves 2 allowed tokens (1 for V = 1): never a banned code among the alternatives, padding behind the allowed ones,
    the sums over the allowed tokens only.  Row 4 has no table."""
    rows = gaussian_rows(V)
    t = np.full((1, 2, V), -np.inf, F32)
    allowed = sorted({V // 3, V - 1})
    t[0, :, allowed] = [[0.0, 0.0], [0.5, 0.5]][:len(allowed)]
    index = [0, 0, 0, 0, -1]
    for column in (0, 1):
        got = check_launch(hip, rows, n, [NEUTRAL] * B, [(0, 0.0, 0.0)] * B, None, column, column=column, tables=t, index=index, what="two allowed")
        for b in range(4):
            assert set(got["codes"][b][got["codes"][b] >= 0]) <= set(allowed)
            assert (got["codes"][b][len(allowed):] == -1).all() and np.isneginf(got["alt_lp"][b][len(allowed):]).all()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", VS)
def test_history_of_five_rows(hip, V, n):
    """A repetition history of 5 rows (position 10 and 11): the alternatives, the entropy and the rank are those of the penalised row."""
    rows = gaussian_rows(V)
    rng = np.random.default_rng(5 + V)
    hist = rng.integers(0, V, (B, 5)).astype(np.int32)
    hist[:, 0] = np.argmax(rows, axis=1)                 # the likeliest code was met: the ranking changes
    hist[1, 1:] = hist[1, 0]
    reps = [(5, 3.0, 2.0), (5, 0.7, 0.3), (3, 1e30, 0.0), (0, 9.0, 9.0), (5, -0.5, 0.1)]
    for column in (0, 1):
        check_launch(hip, rows, n, [RECORDS[3]] * B, reps, hist, 10 + column, column=column, what="history")
        check_launch(hip, rows, n, [NEUTRAL] * B, reps, hist, 10 + column, column=column, what="history, neutral")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", VS)
def test_forced_rows(hip, V, n):
    """Forced rows (the given variant of the kernel), one given code outside [0, V): all four outputs as for a drawn row; rank -1 and a NaN
    log-probability for the code outside; an unforced row of the same launch draws."""
    rows = special_rows(V)
    rows[0] = gaussian_rows(V)[2]
    given = np.array([V // 2, V, min(8, V - 1), V - 1, 0], np.int64)      # row 1: outside
    given_rows = np.array([1, 1, 1, 1, 0], np.int32)                       # position 0 < 2 G: rows 0-3 forced, row 4 drawn
    forced = [True, True, True, True, False]
    for rec in RECORDS:
        got = check_launch(hip, rows, n, [rec] * B, [(0, 0.0, 0.0)] * B, None, 0, given_rows=given_rows, given=given, forced=forced, what="forced")
        assert got["rank"][1] == -1 and np.isnan(got["lp"][1])


def test_refusals(hip):
    """`ts_alt_check` and the entry's own refusals, each before anything is launched."""
    _lib, lib, ctx = hip
    ok = torch.zeros(64, dtype=torch.float32, device="cuda")

    def rec(n=3, reserved=0, codes=True, lp=True, ent=True, rank=True):
        p = ok.data_ptr()
        return _lib.TsAltOut(n, reserved, p if codes else None, p if lp else None, p if ent else None, p if rank else None)

    for bad, text in ((rec(n=9), "outside [0, 8]"), (rec(n=-1), "outside [0, 8]"), (rec(reserved=1), "reserved"), (rec(ent=False), "required"),
                      (rec(rank=False), "required"), (rec(codes=False), "needs codes_dev"), (rec(lp=False), "needs codes_dev")):
        assert lib.ts_alt_check(_lib.C.byref(bad), _lib.TS_SAMPLE_PHILOX) != 0
        assert text in lib.ts_last_error().decode()
    assert lib.ts_alt_check(_lib.C.byref(rec(n=0, codes=False, lp=False)), _lib.TS_SAMPLE_UNIFORMS) == 0
    for mode in (_lib.TS_SAMPLE_GREEDY, _lib.TS_TEACHER_FORCED):
        assert lib.ts_alt_check(_lib.C.byref(rec()), mode) != 0
        assert "top_k = 1" in lib.ts_last_error().decode()
    assert lib.ts_alt_check(None, _lib.TS_SAMPLE_PHILOX) != 0
