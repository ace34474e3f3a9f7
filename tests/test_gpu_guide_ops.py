"""The samplers under guidance as an operator (`ts_op_sample_guide`; `csrc/vq.hip`: `sample_ctl_guide_kernel` and
`sample_ctl_guide_given_kernel`, the GUIDE = true entries of `sample_ctl_body`) against the numpy twin (`talkshow_amd/sampling.py`:
`guided`, `guide_roles`, `sample_guide`).  Tokens, kept bytes, rings and log-probability BITS of primaries and shadows are compared for
equality with the twin; the plain rows of the same launch with `ts_op_sample_repeat` on the same arguments; a primary also with
`ts_op_sample_repeat` on the row l' the twin forms (device against device).  V = 2048 on aligned rows is the vector path; 5, 255, 257 and
2049 the generic one around a thread's chunk of 1, 1, 2 and 9 tokens.  Rows of 2 (a pair), 3 (a pair whose shadow sits BELOW its primary,
a plain row between them) and 33.  The two rows of a pair rank the codes differently, and a CPU assert shows that the rule moves at
least half the draws: a kernel that ignored the second row could not pass.  Every test fails on a build without the feature: the entry
does not exist there.
"""
import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import sampling as S

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = [5, 255, 257, 2048, 2049]
NEUTRAL = (1.0, 1.0, 0)
U_LAST = F32(1.0 - 2.0 ** -24)
RECS = [(0.7, 0.9, 0), (1.5, 1.0, 12), NEUTRAL]
REPS = [(5, 0.7, 0.3), (64, -0.5, 0.1), (0, 3.0, 2.0), (64, 1e30, 0.0)]
SCALES = [2.0, -0.5, 7.5, -1.0]
R = 70                                               # the launch's code row: a wrapped ring


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


def guide_tables(B):
    """(guide, scale): 2 rows a pair; 3 rows: primary 2, shadow 0, row 1 plain; 33 rows: pairs next to each other, far apart and with
    the shadow below, plain rows between and behind them."""
    pairs = {2: [(0, 1)], 3: [(2, 0)], 33: [(0, 1), (5, 2), (10, 30), (32, 31), (7, 20), (12, 13)]}[B]
    guide, scale = np.full(B, -1, np.int32), np.zeros(B, F32)
    for k, (p, g) in enumerate(pairs):
        guide[p], scale[p] = g, SCALES[k % len(SCALES)]
    return guide, scale


def launch(hip, entry, rows, position, column, u=None, philox=None, recs=None, tables=None, index=None, reps=None, hist=None, given_rows=None,
           keep=None, given=None, want_lp=True, want_copy=False, guide=None, scale=None):
    """One launch of `ts_op_sample_guide` (entry="guide") or `ts_op_sample_repeat` -> dict(idx, kept, lp, ring, copy) as numpy."""
    _lib, lib, ctx = hip
    ld = torch.from_numpy(np.ascontiguousarray(rows, F32)).cuda()
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
    hd = None if hist is None else torch.from_numpy(np.ascontiguousarray(hist, np.int32)).cuda()
    with_ring = reps is not None
    args = [ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, int(position), None if recs is None else _table(_lib, recs),
            0 if recs is None else len(recs), _lib.dptr(idx), _lib.dptr(lp), None if gr is None else gr.ctypes.data_as(i32p), _lib.dptr(kd),
            _lib.dptr(gd), _lib.dptr(kept), _lib.dptr(copy), _lib.dptr(td), 0 if td is None else int(td.shape[0]),
            None if index is None else index.ctypes.data_as(i32p), int(column), None if reps is None else _rtable(_lib, reps),
            0 if reps is None else len(reps), _lib.dptr(hd), _lib.dptr(ring) if with_ring else None]
    if entry == "guide":
        g, s = np.ascontiguousarray(guide, np.int32), np.ascontiguousarray(scale, F32)
        _lib.check(lib.ts_op_sample_guide(*args, g.ctypes.data_as(i32p), _lib.fptr(s), None))
    else:
        _lib.check(lib.ts_op_sample_repeat(*args, None))
    return dict(idx=idx.cpu().numpy(), kept=kept.cpu().numpy(), lp=None if lp is None else lp.cpu().numpy(),
                ring=ring.cpu().numpy() if with_ring else None, copy=None if copy is None else copy.cpu().numpy())


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


# what a launch brings: table, bias, ring, given, mask, logprob
COMBOS = [
    dict(), dict(lp=True), dict(table=True), dict(bias=True, lp=True), dict(ring=True), dict(given=True), dict(given=True, mask=True, lp=True),
    dict(ring=True, given=True), dict(table=True, bias=True, ring=True, lp=True), dict(table=True, bias=True, ring=True, given=True, mask=True),
    dict(table=True, bias=True, ring=True, given=True, mask=True, lp=True),
]


@pytest.mark.parametrize("B", [2, 3, 33])
@pytest.mark.parametrize("V", VS)
def test_twin_grid(hip, V, B):
    rng = np.random.default_rng(1000 * V + B)
    guide, scale = guide_tables(B)
    roles = S.guide_roles(guide, B, scale)
    prim, shad, plain = np.flatnonzero(roles >= 0), np.flatnonzero(roles == -2), np.flatnonzero(roles == -1)
    rows = (3.0 * rng.standard_normal((B, V))).astype(F32)
    for p in prim:      # a pair ranks the codes differently, and in the direction in which its scale bites: the shadow's row is the primary's
        # plus noise, with the primary's two likeliest codes moved 8 apart the other way — l' then prefers the second where l prefers the first
        g, sign = int(roles[p]), F32(np.sign(scale[p]))
        first, second = np.argsort(-rows[p], kind="stable")[:2]
        rows[g] = rows[p] + (0.5 * rng.standard_normal(V)).astype(F32)
        rows[g, first] += F32(8.0) * sign
        rows[g, second] -= F32(8.0) * sign
        assert not np.array_equal(np.argsort(-rows[p], kind="stable"), np.argsort(-rows[g], kind="stable"))
    tables = rng.standard_normal((2, 2, V)).astype(F32)
    tables[rng.random((2, 2, V)) < 0.3] = -np.inf
    tables[:, :, V // 2] = 0.25
    index = np.asarray([(b % 3) - 1 for b in range(B)], np.int32)      # -1, 0, 1, ...
    index[shad] = 1                                                      # a shadow's table is never read
    hist = rng.integers(0, V, (B, 64)).astype(np.int32)
    hist[:, ::7] = hist[:, :1]                                           # codes met more than once
    G = np.asarray([R + 1 if b % 3 == 0 else R if b % 3 == 1 else R + 5 for b in range(B)], np.int32)
    keep = np.asarray([0 if b % 3 == 2 else 1 for b in range(B)], np.uint8)
    G[shad], keep[shad] = R + 5, 1                                       # a shadow would be forced if it decided anything
    given = rng.integers(0, V, B).astype(np.int64)
    given[prim[0]] = 2 ** 40 if B == 3 else given[prim[0]]               # a given code outside the vocabulary, written to both rows
    moved = drawn = 0
    n = 0
    for mode in ("uniforms", "philox"):
        for combo in COMBOS:
            column = n % 2
            position = 2 * R + column
            recs = [RECS[(n + b) % 3] for b in range(B)] if combo.get("table") else None
            reps = [REPS[(n + b) % 4] for b in range(B)] if combo.get("ring") else None
            with_bias, with_given, with_mask, want_lp = (bool(combo.get(k)) for k in ("bias", "given", "mask", "lp"))
            if mode == "uniforms":
                u = np.zeros(B, F32) if n == 0 else np.full(B, U_LAST, F32) if n == 1 else rng.random(B).astype(F32)
                src = dict(u=u)
            else:
                seed, clip0 = 77 + n, 1000 + 3 * n
                u = np.asarray([O.philox_uniform(seed, clip0 + b, position) for b in range(B)], F32)      # a row's own index and position
                src = dict(philox=(seed, clip0))
            kw = dict(recs=recs, tables=tables if with_bias else None, index=index if with_bias else None, reps=reps,
                      hist=hist if reps is not None else None, given_rows=G if with_given else None, keep=keep if with_mask else None,
                      given=given if with_given else None, want_lp=want_lp)
            got = launch(hip, "guide", rows, position, column, want_copy=(n % 4 == 0), guide=guide, scale=scale, **src, **kw)
            forced = np.zeros(B, bool)
            if with_given:
                forced = np.asarray([position < 2 * int(G[b]) and (not with_mask or keep[b] != 0) for b in range(B)])
            ti, tk, tl, tring = S.sample_guide(rows, u, recs, guide, scale, reps, hist if reps is not None else None, position,
                                               tables if with_bias else None, index if with_bias else None, column,
                                               given if with_given else None, forced if with_given else None)
            what = f"V {V} B {B} {mode} launch {n} {combo}"
            np.testing.assert_array_equal(got["idx"], ti, err_msg=what)
            for p in prim:
                g = int(roles[p])
                assert got["idx"][g] == got["idx"][p], f"{what}: the shadow of row {p} holds another code"
            written = np.asarray([want_lp or not forced[b] for b in range(B)])      # a forced row without the output leaves ahead of the kept bytes
            for p in prim:
                written[roles[p]] = written[p]
            for b in range(B):
                if written[b]:
                    assert np.array_equal(got["kept"][b].astype(bool), tk[b]), f"{what} row {b}: kept bytes"
                else:
                    assert (got["kept"][b] == 9).all(), f"{what} row {b}: kept bytes written by a row that leaves early"
            if want_lp:
                assert np.array_equal(bits(got["lp"]), bits(tl)), f"{what}: logprob {got['lp']} twin {tl}"
            if reps is not None:
                np.testing.assert_array_equal(got["ring"], tring, err_msg=what)
                ring0 = np.empty((B, 64), np.int32)
                for i in range(64):
                    ring0[:, (R - 64 + i) & 63] = hist[:, i]
                assert np.array_equal(got["ring"][shad], ring0[shad]), f"{what}: a shadow's ring was touched"
            if got["copy"] is not None:
                assert np.array_equal(bits(got["copy"]), bits(rows)), f"{what}: the logits copies are the network's rows, the shadows' included"
            # the plain rows are the rows of the launch without the table; a primary is that launch's row on l'
            eff = rows.copy()
            for p in prim:
                eff[p] = S.guided(rows[p], rows[roles[p]], scale[p])
            ref = launch(hip, "repeat", eff, position, column, **src, **dict(kw, reps=reps if reps is not None else [(0, 0.0, 0.0)],
                                                                              hist=hist))
            for b in np.concatenate([plain, prim]):
                assert got["idx"][b] == ref["idx"][b], f"{what} row {b}"
                assert np.array_equal(got["kept"][b], ref["kept"][b]), f"{what} row {b}"
                if want_lp:
                    assert bits(got["lp"])[b] == bits(ref["lp"])[b], f"{what} row {b}"
                if reps is not None:
                    assert np.array_equal(got["ring"][b], ref["ring"][b]), f"{what} row {b}"
            # the CPU rule with and without guidance, on the rows that draw
            for p in prim:
                if forced[p]:
                    continue
                wi, _, _, _ = S.sample_repeat(rows[p][None], [u[p]], None if recs is None else [recs[p]], [(0, 0.0, 0.0)] if reps is None else [reps[p]],
                                              hist[p][None], position, tables if with_bias else None, [index[p]] if with_bias else None, column)
                drawn += 1
                moved += int(wi[0] != ti[p])
            n += 1
    assert 2 * moved >= drawn > 0, f"guidance moved {moved} of {drawn} draws: the second row does not bite"


def test_scale_zero_and_own_row(hip):
    """scale = 0: the codes of the launch without the table; a shadow that carries the primary's own row: codes, kept bytes and
    log-probability bits of that launch for any scale (both paths)."""
    for V in (2048, 300):
        rng = np.random.default_rng(V)
        rows = (2.0 * rng.standard_normal((4, V))).astype(F32)
        u = rng.random(4).astype(F32)
        recs = [(0.8, 0.95, 0), NEUTRAL, (1.3, 1.0, 30), NEUTRAL]
        ref = launch(hip, "repeat", rows, 1, 1, u=u, recs=recs, reps=[(0, 0.0, 0.0)])
        got = launch(hip, "guide", rows, 1, 1, u=u, recs=recs, guide=[1, -1, 3, -1], scale=[0.0, 0, 0.0, 0])
        assert got["idx"][0] == ref["idx"][0] and got["idx"][2] == ref["idx"][2]
        assert np.array_equal(got["kept"][0], ref["kept"][0]) and got["idx"][1] == got["idx"][0]
        own = rows.copy()
        own[1], own[3] = own[0], own[2]
        for scale in (3.0, -0.5, 1e4):
            got = launch(hip, "guide", own, 1, 1, u=u, recs=recs, guide=[1, -1, 3, -1], scale=[scale, 0, -scale, 0])
            for p, g in ((0, 1), (2, 3)):
                assert got["idx"][p] == ref["idx"][p] and np.array_equal(got["kept"][p], ref["kept"][p])
                assert bits(got["lp"])[p] == bits(ref["lp"])[p] and bits(got["lp"])[g] == bits(got["lp"])[p]


def test_errors_before_any_launch(hip):
    _lib, lib, ctx = hip
    V, B = 64, 4
    ld = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    u = torch.zeros(B, dtype=torch.float32, device="cuda")
    i32p = _lib.C.POINTER(_lib.C.c_int32)

    def call(mode, guide, scale):
        g = None if guide is None else np.ascontiguousarray(guide, np.int32)
        s = np.ascontiguousarray(scale, F32)
        return lib.ts_op_sample_guide(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(u), 0, 0, 4, None, 0, _lib.dptr(idx), None, None, None, None, None,
                                      None, None, 0, None, 0, None, 0, None, None, None if g is None else g.ctypes.data_as(i32p), _lib.fptr(s), None)
    ok = [1, -1, -1, -1]
    assert call(_lib.TS_SAMPLE_GREEDY, ok, [1, 0, 0, 0]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_TEACHER_FORCED, ok, [1, 0, 0, 0]) != 0 and "top_k = 1" in lib.ts_last_error().decode()
    assert call(_lib.TS_SAMPLE_UNIFORMS, None, [1, 0, 0, 0]) != 0
    for guide, scale, word in (([4, -1, -1, -1], [1, 0, 0, 0], "clip 0"), ([-1, 1, -1, -1], [0, 1, 0, 0], "names itself"),
                               ([2, -1, -1, 2], [1, 0, 0, 1], "already the shadow"), ([1, 2, -1, -1], [1, 1, 0, 0], "itself guided"),
                               ([-1, -1, 3, -1], [0, 0, float("nan"), 0], "clip 2"), ([1, -1, -1, -1], [2e4, 0, 0, 0], "1e4")):
        assert call(_lib.TS_SAMPLE_UNIFORMS, guide, scale) != 0 and word in lib.ts_last_error().decode(), (guide, lib.ts_last_error().decode())
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all()
    assert call(_lib.TS_SAMPLE_UNIFORMS, ok, [1, 0, 0, 0]) == 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy()[2:] != -7).all() and idx.cpu().numpy()[1] == idx.cpu().numpy()[0]
