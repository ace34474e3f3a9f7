"""Every sampler entry (`ts_op_sample`, `ts_op_sample_philox`, `ts_op_sample_lp`, `ts_op_sample_ctl`, `ts_op_sample_given`: the twelve
sampler kernels of `csrc/vq.hip`) replayed over recorded inputs, against the BITS the build before the fold into `sample_plain_body` /
`sample_ctl_body` returned: `tests/golden/sampler_bits.npz`.

The other sampler tests hold indices exactly but log-probabilities to one fp32 spacing of the numpy restatement; here the int64 codes and
the log-probabilities viewed as uint32 are compared with `array_equal`.  The fixture holds the inputs too: B = 5 rows (random, a peaked
row whose other weights underflow, an all-equal row, ties, random), forced pattern [1, 0, 1, 0, 0] for the given entry; V = 2048 (vector
loads), 1000 (chunks of 4, the last threads own nothing), 256 (chunks of 1), 5 (fewer tokens than threads), and V = 2048 once more on rows
that start 4 bytes off a 16-byte boundary, which is what sends a controls launch to its FAST = false instantiation (the operator entries
take no row stride; only the entries with a table run on those rows).  `launches` below is the one enumeration of the launches: the
recording was made by calling it on the earlier build, the test calls it on this one.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ["2048", "1000", "256", "5", "2048_off4"]
FORCED = [1, 0, 1, 0, 0]
NEUTRAL = (1.0, 1.0, 0)
RECORDS = [[NEUTRAL], [(0.8, 0.9, 0)], [(1.0, 1.0, 1)], [(2.5, 0.6, 30)],
           [(0.8, 0.9, 0), NEUTRAL, (2.5, 0.6, 30), (1.0, 1.0, 1), (1.7, 0.3, 12)]]
LP_UNTOUCHED = F32(777.0)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_bits.npz")


def _table(_lib, recs):
    arr = (_lib.TsSampling * len(recs))()
    for b, (t, p, k) in enumerate(recs):
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    return arr


def device_rows(rows, key):
    """(B,V) host rows -> a contiguous device view of them; for the `_off4` key the view starts one float into its allocation."""
    B, V = rows.shape
    off = 1 if key.endswith("_off4") else 0
    buf = torch.zeros(B * V + 4, dtype=torch.float32, device="cuda")
    ld = buf[off:off + B * V].view(B, V)
    ld.copy_(torch.from_numpy(np.ascontiguousarray(rows, F32)))
    assert (ld.data_ptr() & 15) == 4 * off
    return ld


def launches(hip, fx, key):
    """Yields (name, idx (5,) int64, logprob (5,) float32) of every launch of one key, in a fixed order.  fx: the fixture's input arrays."""
    _lib, lib, ctx = hip
    rows = fx["logits_" + key.split("_")[0]]
    B, V = rows.shape
    ld = device_rows(rows, key)
    plain_entries = not key.endswith("_off4")
    seed, clip0, pos = (int(v) for v in fx["philox"])
    forced = np.asarray(FORCED, np.int32)
    forced_p = forced.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
    uds = [torch.from_numpy(np.ascontiguousarray(u, F32)).cuda() for u in fx["uniforms"]]
    draws = [("u%d" % i, _lib.TS_SAMPLE_UNIFORMS, ud) for i, ud in enumerate(uds)] + [("philox", _lib.TS_SAMPLE_PHILOX, None)]

    def outputs(codes=None):
        idx = torch.full((B,), -3, dtype=torch.int64, device="cuda") if codes is None else torch.from_numpy(np.asarray(codes, np.int64)).cuda()
        return idx, torch.full((B,), float(LP_UNTOUCHED), dtype=torch.float32, device="cuda")

    def result(name, idx, lp):
        return name, idx.cpu().numpy(), lp.cpu().numpy()

    if plain_entries:
        idx, lp = outputs()
        _lib.check(lib.ts_op_sample(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_GREEDY, None, _lib.dptr(idx), None))
        yield result("sample greedy", idx, lp)
        for un, ud in zip(("u0", "u1"), uds):
            idx, lp = outputs()
            _lib.check(lib.ts_op_sample(ctx, _lib.dptr(ld), B, V, _lib.TS_SAMPLE_UNIFORMS, _lib.dptr(ud), _lib.dptr(idx), None))
            yield result("sample " + un, idx, lp)
        idx, lp = outputs()
        _lib.check(lib.ts_op_sample_philox(ctx, _lib.dptr(ld), B, V, seed, clip0, pos, _lib.dptr(idx), None))
        yield result("sample philox", idx, lp)
        for mn, mode, ud in [("greedy", _lib.TS_SAMPLE_GREEDY, None)] + draws + [("teacher", _lib.TS_TEACHER_FORCED, None)]:
            idx, lp = outputs(fx["teacher_" + key] if mode == _lib.TS_TEACHER_FORCED else None)
            _lib.check(lib.ts_op_sample_lp(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, None, 0, _lib.dptr(idx), None,
                                           _lib.dptr(lp), None))
            yield result("lp " + mn, idx, lp)
    for r, recs in enumerate(RECORDS):
        for mn, mode, ud in draws:
            for want_lp in (False, True):
                idx, lp = outputs()
                args = (ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, _table(_lib, recs), len(recs), _lib.dptr(idx), None)
                _lib.check(lib.ts_op_sample_lp(*args, _lib.dptr(lp), None) if want_lp else lib.ts_op_sample_ctl(*args, None))
                yield result("ctl%s records %d %s" % (" lp" if want_lp else "", r, mn), idx, lp)
    for g, given in enumerate(fx["given_" + key]):
        gd = torch.from_numpy(np.ascontiguousarray(given, np.int64)).cuda()
        tables = ([("none", None)] if plain_entries else []) + [(str(r), recs) for r, recs in enumerate(RECORDS)]
        for tn, recs in tables:
            modes = draws + ([("greedy", _lib.TS_SAMPLE_GREEDY, None)] if recs is None else [])
            for mn, mode, ud in modes:
                for want_lp in (False, True):
                    idx, lp = outputs()
                    tab, n = (_table(_lib, recs), len(recs)) if recs else (None, 0)
                    _lib.check(lib.ts_op_sample_given(ctx, _lib.dptr(ld), B, V, mode, _lib.dptr(ud), seed, clip0, pos, tab, n, _lib.dptr(idx),
                                                      _lib.dptr(lp) if want_lp else None, forced_p, _lib.dptr(gd), None))
                    yield result("given %d%s table %s %s" % (g, " lp" if want_lp else "", tn, mn), idx, lp)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


@pytest.mark.parametrize("key", KEYS)
def test_every_sampler_entry_returns_the_recorded_bits(hip, key):
    fx = dict(np.load(FIXTURE))
    names = [str(n) for n in fx["names_" + key]]
    want_idx, want_lp = fx["codes_" + key], fx["logprob_bits_" + key]
    assert want_idx.dtype == np.int64 and want_lp.dtype == np.uint32 and len(names) >= 40
    n = 0
    for name, idx, lp in launches(hip, fx, key):
        assert name == names[n], f"launch {n}: the enumeration gives {name!r}, the recording {names[n]!r}"
        assert np.array_equal(idx, want_idx[n]), f"V {key} {name}: codes {idx}, recorded {want_idx[n]}"
        assert np.array_equal(lp.view(np.uint32), want_lp[n]), f"V {key} {name}: log-probability bits {lp}, recorded {want_lp[n].view(F32)}"
        n += 1
    assert n == len(names)
