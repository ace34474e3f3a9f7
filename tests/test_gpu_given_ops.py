"""The samplers' given variants as an operator (`ts_op_sample_given`; `csrc/vq.hip`: sample_given_kernel, sample_lp_given_kernel,
sample_ctl_given_kernel — the `GIVEN` instantiations of `sample_plain_body` and `sample_ctl_body`) against their
siblings (`ts_op_sample_lp`) and the numpy restatement (`sampling.given_logprob`).

One launch of B = 5 rows, forced in the pattern [1, 0, 1, 0, 0]: an unforced row returns its sibling's index and log-probability BIT FOR
BIT; a forced row returns its given code, the teacher-forced log-probability without a record and, with one, the restatement's value to
one fp32 spacing (the two fp64 logs) or exactly -inf for a code the filters removed.  The given codes of unforced rows hold 2**40 and -7,
the outputs sit between sentinel zones.  Every test fails on a build without the feature: the entry does not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from test_gpu_sampling_ops import VS, _table, regime_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
FORCED = [1, 0, 1, 0, 0]
ZONE = 512                                           # elements of sentinel on either side of an output
NEUTRAL = (1.0, 1.0, 0)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _mode_args(_lib, mode, u, philox):
    ud = torch.from_numpy(np.ascontiguousarray(u, F32)).cuda() if mode == _lib.TS_SAMPLE_UNIFORMS else None
    seed, clip0, pos = philox if mode == _lib.TS_SAMPLE_PHILOX else (0, 0, philox[2])
    return ud, seed, clip0, pos


def op_sibling(hip, ld, mode, u, philox, recs, idx_in=None):
    """`ts_op_sample_lp`: (idx, logprob) of the sampler the given variant stands in for (teacher forced: idx_in is scored)."""
    _lib, lib, ctx = hip
    B, V = ld.shape
    idx = torch.full((B,), -3, dtype=torch.int64, device="cuda") if idx_in is None else torch.from_numpy(np.asarray(idx_in, np.int64)).cuda()
    lp = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ud, seed, clip0, pos = _mode_args(_lib, mode if mode != _lib.TS_TEACHER_FORCED else _lib.TS_SAMPLE_GREEDY, u, philox)
    tab, n = (_table(_lib, recs), len(recs)) if recs else (None, 0)
    _lib.check(lib.ts_op_sample_lp(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, tab, n, _lib.dptr(idx), None, _lib.dptr(lp), None))
    return idx.cpu().numpy(), lp.cpu().numpy()


def op_given(hip, ld, mode, u, philox, recs, given, want_lp):
    """`ts_op_sample_given` with both outputs inside sentinel zones (checked here) -> (idx, logprob or None)."""
    _lib, lib, ctx = hip
    B, V = ld.shape
    ibuf = torch.full((B + 2 * ZONE,), -12345, dtype=torch.int64, device="cuda")
    fbuf = torch.full((B + 2 * ZONE,), 777.0, dtype=torch.float32, device="cuda")
    idx, lp = ibuf[ZONE:ZONE + B], (fbuf[ZONE:ZONE + B] if want_lp else None)
    ud, seed, clip0, pos = _mode_args(_lib, mode, u, philox)
    tab, n = (_table(_lib, recs), len(recs)) if recs else (None, 0)
    forced = np.asarray(FORCED, np.int32)
    gd = torch.from_numpy(np.asarray(given, np.int64)).cuda()
    _lib.check(lib.ts_op_sample_given(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, tab, n, _lib.dptr(idx), _lib.dptr(lp),
                                      forced.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(gd), None))
    ih, fh = ibuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (ih[:ZONE] == -12345).all() and (ih[ZONE + B:] == -12345).all(), "index output: a sentinel zone was written"
    assert (fh[:ZONE] == 777.0).all() and (fh[ZONE + B:] == 777.0).all(), "log-probability output: a sentinel zone was written"
    if not want_lp:
        assert (fh == 777.0).all()
    return ih[ZONE:ZONE + B].copy(), (fh[ZONE:ZONE + B].copy() if want_lp else None)


def within_one_spacing(got, want):
    got, want = np.float64(got), np.float64(want)
    return abs(got - want) <= np.float64(np.spacing(np.abs(F32(want))))


def _cases(rows):
    """(records or None, given codes): forced rows 0 and 2 get in-range codes, the others 2**40 and -7 (never read)."""
    V = rows.shape[1]
    top0 = np.argsort(-rows[0].astype(np.float64), kind="stable")
    g_kept = [int(top0[0]), 2 ** 40, 7 % V, -7, 2 ** 40]
    g_removed = [int(top0[5]), -7, 1, 2 ** 40, -7]
    return [
        (None, g_kept),
        (None, g_removed),
        # rank 0 of a peaked row under a mild record; row 2 is all-equal: top_k = 1 keeps index 0 only, the given index 1 is removed
        ([(0.8, 0.9, 0), (1.0, 1.0, 1), (1.0, 1.0, 1), (1.7, 0.3, 12), NEUTRAL], [int(top0[0]), 2 ** 40, 1, -7, 2 ** 40]),
        # a tight top_p keeps rank 0 alone: rank 5 is removed; index 7 of the all-equal row is inside top_k = 30 and the 0.6 nucleus
        ([(1.0, 1e-6, 0), NEUTRAL, (2.5, 0.6, 30), (0.5, 0.5, 40), (4.0, 0.95, 64)], g_removed[:2] + [7 % V] + g_removed[3:]),
        ([(1.0, 1e-6, 0), (1.0, 1.0, 1), (1.0, 1.0, 1), NEUTRAL, (1.0, 0.999, 5)], [int(top0[0]), -7, 0, 2 ** 40, -7]),
    ]


@pytest.mark.parametrize("V", VS)
def test_given_variants_against_their_siblings(hip, golden, V):
    _lib, lib, ctx = hip
    rows = regime_rows(golden, V)
    B = rows.shape[0]
    ld = torch.from_numpy(rows).cuda()
    rng = np.random.default_rng(5 * V)
    u = rng.random(B).astype(F32)
    u[0], u[2] = np.nan, np.nan                        # the uniforms of forced rows are never read
    u_sib = np.where(np.isnan(u), F32(0.5), u).astype(F32)
    philox = (2 ** 40 + 3, 2 ** 33, 149)
    saw_minus_inf = saw_finite_with_record = False
    for recs, given in _cases(rows):
        modes = [_lib.TS_SAMPLE_UNIFORMS, _lib.TS_SAMPLE_PHILOX] + ([_lib.TS_SAMPLE_GREEDY] if recs is None else [])
        for mode in modes:
            sib_idx, sib_lp = op_sibling(hip, ld, mode, u_sib, philox, recs)
            for want_lp in (True, False):
                idx, lp = op_given(hip, ld, mode, u, philox, recs, given, want_lp)
                for b in range(B):
                    if not FORCED[b]:
                        assert idx[b] == sib_idx[b], f"V {V} mode {mode} records {recs}: row {b} drew {idx[b]}, its sibling {sib_idx[b]}"
                        if want_lp:
                            assert lp[b].view(np.uint32) == sib_lp[b].view(np.uint32), f"V {V} mode {mode} records {recs}: row {b}"
                    else:
                        assert idx[b] == given[b]
                if not want_lp:
                    continue
                if recs is None:                      # the teacher-forced launch of the sibling on the same codes, bit for bit
                    codes = [given[b] if FORCED[b] else 0 for b in range(B)]
                    _, tf = op_sibling(hip, ld, _lib.TS_TEACHER_FORCED, u_sib, philox, None, idx_in=codes)
                    for b in (0, 2):
                        assert lp[b].view(np.uint32) == tf[b].view(np.uint32)
                        assert within_one_spacing(lp[b], S.given_logprob(rows[b], given[b]))
                else:
                    for b in (0, 2):
                        want = S.given_logprob(rows[b], given[b], recs[b])
                        if np.isneginf(want):
                            assert np.isneginf(lp[b]), f"V {V} records {recs[b]} row {b}: a removed code must give -inf, got {lp[b]}"
                            saw_minus_inf = True
                        else:
                            assert np.isfinite(lp[b]) and within_one_spacing(lp[b], want), f"V {V} record {recs[b]} row {b}: {lp[b]} vs {want}"
                            saw_finite_with_record = True
                        if recs[b][2] == 1:
                            assert lp[b] == 0.0 or np.isneginf(lp[b])            # top_k = 1: 0 or -inf
    assert saw_minus_inf and saw_finite_with_record


def test_a_table_with_greedy_stays_refused(hip, golden):
    _lib, lib, ctx = hip
    rows = regime_rows(golden, 256)
    ld = torch.from_numpy(rows).cuda()
    idx = torch.full((5,), -3, dtype=torch.int64, device="cuda")
    gd = torch.zeros(5, dtype=torch.int64, device="cuda")
    forced = np.asarray(FORCED, np.int32)
    rc = lib.ts_op_sample_given(ctx, _lib.dptr(ld), 5, 256, _lib.TS_SAMPLE_GREEDY, None, 0, 0, 0, _table(_lib, [NEUTRAL]), 1, _lib.dptr(idx), None,
                                forced.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(gd), None)
    assert rc != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert (idx.cpu().numpy() == -3).all()
