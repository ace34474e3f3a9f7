"""One launch of the samplers' given variants with the DEVICE-side decision of "kept positions" exercised (`ts_op_sample_keep`;
`csrc/vq.hip`: `given_forced` with its mask byte, behind every `GIVEN` instantiation of `sample_plain_body` and `sample_ctl_body`) against
the numpy restatement (`sampling.keep_forced`, `sampling.sample_given`, `sampling.given_logprob`) and against `ts_op_sample_given`.

B = 5 rows whose given-row counts put the launch's position on both sides of 2 G_b (position == 2 G_b - 1 and == 2 G_b among them), a
mask that mixes 0 and 1 (and a byte of 255: not 0), poisoned given codes (-7, 2**40) on every row that is not forced and NaN uniforms on
every row that is.  Every check is equality.  Every test fails on a build without the feature: the entry does not exist there.
"""
import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S
from test_gpu_sampling_ops import _table, regime_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
ZONE = 512
NEUTRAL = (1.0, 1.0, 0)
POSITION = 13                                        # row 6, column 1
ROWS = [7, 6, 7, 0, 9]                               # 2 G = 14 (position == 2 G - 1), 12 (below), 14, 0, 18
KEEP = [1, 1, 0, 1, 255]                             # -> forced: yes, no (position >= 2 G), no (masked out), no (G = 0), yes
PHILOX = (2 ** 40 + 3, 2 ** 33)                      # seed, clip_index0
RECS = [None,
        [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.0, 1.0, 1), (1.7, 0.3, 12), NEUTRAL],
        [(1.0, 1e-6, 0), NEUTRAL, (2.5, 0.6, 30), (0.5, 0.5, 40), (4.0, 0.95, 64)]]


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _logits(golden, V):
    """(device tensor (5, V), numpy rows): V = 2048 on a 16-byte aligned row is the vector path of every kernel."""
    rows = regime_rows(golden, V)
    ld = torch.from_numpy(rows).cuda()
    assert V != 2048 or ld.data_ptr() % 16 == 0
    return ld, rows


def op_keep(hip, ld, mode, u, position, recs, grows, keep, given, want_lp):
    """`ts_op_sample_keep` with both outputs inside sentinel zones (checked here) -> (idx, logprob or None)."""
    _lib, lib, ctx = hip
    B, V = ld.shape
    ibuf = torch.full((B + 2 * ZONE,), -12345, dtype=torch.int64, device="cuda")
    fbuf = torch.full((B + 2 * ZONE,), 777.0, dtype=torch.float32, device="cuda")
    idx, lp = ibuf[ZONE:ZONE + B], (fbuf[ZONE:ZONE + B] if want_lp else None)
    ud = torch.from_numpy(np.ascontiguousarray(u, F32)).cuda() if mode == _lib.TS_SAMPLE_UNIFORMS else None
    seed, clip0 = PHILOX if mode == _lib.TS_SAMPLE_PHILOX else (0, 0)
    tab, n = (_table(_lib, recs), len(recs)) if recs else (None, 0)
    g = np.asarray(grows, np.int32)
    kd = None if keep is None else torch.from_numpy(np.asarray(keep, np.uint8)).cuda()
    gd = torch.from_numpy(np.asarray(given, np.int64)).cuda()
    _lib.check(lib.ts_op_sample_keep(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, position, tab, n, _lib.dptr(idx), _lib.dptr(lp),
                                     g.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(kd), _lib.dptr(gd), None))
    ih, fh = ibuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (ih[:ZONE] == -12345).all() and (ih[ZONE + B:] == -12345).all(), "index output: a sentinel zone was written"
    assert (fh[:ZONE] == 777.0).all() and (fh[ZONE + B:] == 777.0).all(), "log-probability output: a sentinel zone was written"
    if not want_lp:
        assert (fh == 777.0).all()
    return ih[ZONE:ZONE + B].copy(), (fh[ZONE:ZONE + B].copy() if want_lp else None)


def op_given(hip, ld, mode, u, position, recs, forced, given, want_lp):
    """`ts_op_sample_given`: the launch with the HOST's forced flags (no mask load)."""
    _lib, lib, ctx = hip
    B, V = ld.shape
    idx = torch.full((B,), -3, dtype=torch.int64, device="cuda")
    lp = torch.full((B,), 7.0, dtype=torch.float32, device="cuda") if want_lp else None
    ud = torch.from_numpy(np.ascontiguousarray(u, F32)).cuda() if mode == _lib.TS_SAMPLE_UNIFORMS else None
    seed, clip0 = PHILOX if mode == _lib.TS_SAMPLE_PHILOX else (0, 0)
    tab, n = (_table(_lib, recs), len(recs)) if recs else (None, 0)
    f = np.asarray(forced, np.int32)
    gd = torch.from_numpy(np.asarray(given, np.int64)).cuda()
    _lib.check(lib.ts_op_sample_given(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, position, tab, n, _lib.dptr(idx), _lib.dptr(lp),
                                      f.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(gd), None))
    return idx.cpu().numpy(), (lp.cpu().numpy() if want_lp else None)


def _inputs(rows, forced, seed):
    """Given codes (in range where forced: rank 5 — which a tight record removes —, then rank 0; poison elsewhere) and uniforms (NaN where forced)."""
    B, V = rows.shape
    rng = np.random.default_rng(seed)
    top = np.argsort(-rows.astype(np.float64), axis=1, kind="stable")
    given = np.asarray([[-7, 2 ** 40][b % 2] for b in range(B)], np.int64)
    for n, b in enumerate(np.flatnonzero(forced)):
        given[b] = top[b, min(5, V - 1)] if n % 2 == 0 else top[b, 0]
    u = rng.random(B).astype(F32)
    u[np.asarray(forced, bool)] = np.nan
    return given, u


def test_the_cases_fall_on_both_sides():
    assert POSITION == 2 * ROWS[0] - 1 and POSITION >= 2 * ROWS[1] and POSITION + 1 == 2 * ROWS[2] and ROWS[3] == 0
    assert list(S.keep_forced(ROWS, np.asarray(KEEP).reshape(5, 1, 1).repeat(7, 1).repeat(2, 2), POSITION // 2, POSITION % 2)) == [True, False, False, False, True]


@pytest.mark.parametrize("V", [2048, 256, 37])
@pytest.mark.parametrize("position,grows", [(POSITION, ROWS), (2 * 6, [6, 7, 7, 7, 0])])      # and position == 2 G on row 0
def test_keep_against_the_restatement(hip, golden, V, position, grows):
    _lib, lib, ctx = hip
    ld, rows = _logits(golden, V)
    B = rows.shape[0]
    below = np.asarray([position < 2 * g for g in grows])
    forced = below & (np.asarray(KEEP) != 0)
    assert forced.any() and (below & ~forced).any() and (~below).any()
    given, u = _inputs(rows, forced, 3 * V + position)
    u_np = np.where(np.isnan(u), F32(0.5), u).astype(F32)
    u_px = np.asarray([O.philox_uniform(PHILOX[0], PHILOX[1] + b, position) for b in range(B)], F32)
    saw_inf = False
    for recs in RECS:
        modes = [_lib.TS_SAMPLE_UNIFORMS, _lib.TS_SAMPLE_PHILOX] + ([_lib.TS_SAMPLE_GREEDY] if recs is None else [])
        for mode in modes:
            uu = u_px if mode == _lib.TS_SAMPLE_PHILOX else u_np
            want_idx, want_lp = S.sample_given(rows, uu, forced, given, recs, greedy=mode == _lib.TS_SAMPLE_GREEDY)
            for want in (True, False):
                idx, lp = op_keep(hip, ld, mode, u, position, recs, grows, KEEP, given, want)
                what = f"V {V} position {position} mode {mode} records {recs}"
                print(what, "idx", idx, want_idx, "lp", lp, want_lp)
                assert np.array_equal(idx, want_idx), what
                assert np.array_equal(idx[forced], given[forced])
                # the same launch with the host's flags, bit for bit
                sidx, slp = op_given(hip, ld, mode, u, position, recs, forced.astype(np.int32), given, want)
                assert np.array_equal(idx, sidx), what
                if want:
                    assert np.array_equal(lp.view(np.uint32), slp.view(np.uint32)), what
                    assert np.array_equal(lp.view(np.uint32), want_lp.view(np.uint32)), what
                    saw_inf = saw_inf or bool(np.isneginf(lp[forced]).any())
    assert saw_inf                                   # a kept code that a record removed scored log(0)


@pytest.mark.parametrize("V", [2048, 256, 37])
def test_no_mask_is_the_given_launch(hip, golden, V):
    """keep_dev = NULL equals `ts_op_sample_given` with forced = (position < 2 G), bit for bit; so does an all-ones mask."""
    _lib, lib, ctx = hip
    ld, rows = _logits(golden, V)
    forced = np.asarray([POSITION < 2 * g for g in ROWS])
    given, u = _inputs(rows, forced, 11 * V)
    for recs in RECS:
        modes = [_lib.TS_SAMPLE_UNIFORMS, _lib.TS_SAMPLE_PHILOX] + ([_lib.TS_SAMPLE_GREEDY] if recs is None else [])
        for mode in modes:
            for want in (True, False):
                sidx, slp = op_given(hip, ld, mode, u, POSITION, recs, forced.astype(np.int32), given, want)
                for keep in (None, [1] * 5, [7, 1, 255, 1, 128]):
                    idx, lp = op_keep(hip, ld, mode, u, POSITION, recs, ROWS, keep, given, want)
                    assert np.array_equal(idx, sidx) and np.array_equal(idx[forced], given[forced])
                    assert not want or np.array_equal(lp.view(np.uint32), slp.view(np.uint32))


def test_refusals(hip, golden):
    _lib, lib, ctx = hip
    ld, rows = _logits(golden, 256)
    idx = torch.full((5,), -3, dtype=torch.int64, device="cuda")
    gd = torch.zeros(5, dtype=torch.int64, device="cuda")
    i32p = _lib.C.POINTER(_lib.C.c_int32)

    def rc(grows, mode=_lib.TS_SAMPLE_GREEDY, tab=None, n=0):
        g = np.asarray(grows, np.int32)
        return lib.ts_op_sample_keep(ctx, _lib.dptr(ld), 5, 256, mode, None, 0, 0, 3, tab, n, _lib.dptr(idx), None, g.ctypes.data_as(i32p), None,
                                     _lib.dptr(gd), None)
    assert rc([1, 1, -1, 1, 1]) != 0 and "row 2" in lib.ts_last_error().decode()
    assert rc(ROWS, tab=_table(_lib, [NEUTRAL]), n=1) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert rc(ROWS, mode=_lib.TS_SAMPLE_UNIFORMS) != 0 and "uniforms required" in lib.ts_last_error().decode()
    assert (idx.cpu().numpy() == -3).all()
