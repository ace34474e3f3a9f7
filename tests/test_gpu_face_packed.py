"""The PACKED plan of mixed face passes (`ts_face_generate_mixed` under `TS_FACE_PACK=1`, csrc/face.cpp::face_packed_layout): the six stride-2 feature convolutions
and the 12 transformer layers run on the clips' OWN rows, back to back, instead of on B x longest.

The bar is EQUALITY with the padded plan in the same process (`ts_debug_face_generate_mixed`, layout 0 against 1): packing changes which rows
are computed, never a row's bits — no GEMM of a mixed pass takes the stream-K band, so a row's bits depend neither on the rows it shares a
launch with nor on the tile its launch gets.  Every test fails on a build without the feature: the entries do not exist there.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_canary import F32, run_both
from test_gpu_face_mixed import SPEC, _frames

pytestmark = pytest.mark.gpu

I32P = C.POINTER(C.c_int32)
FC_K = (3, 3, 3, 3, 2, 2)
FIVE = [(400, 1), (16001, 29), (33613, 64), (34700, 65), (68300, 127)]


@pytest.fixture(scope="module")
def m():
    from talkshow_amd.modules import FaceGenerator
    g = FaceGenerator().cuda()                                            # the full-size network: 12 layers
    g.load_state_dict(synth.to_torch(synth.face_state_dict(seed=7)))
    return g


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _table(spec, seed):
    """Shuffled clips of `spec` as one padded batch with NaN in every sample at or beyond ns[b]."""
    order = np.random.default_rng(seed).permutation(len(spec))
    spec = [spec[i] for i in order]
    ns = np.asarray([n for n, _ in spec], np.int32)
    frames = np.asarray([_frames(n, f) for n, f in spec], np.int32)
    wav = np.full((len(spec), int(ns.max())), np.nan, np.float32)
    for b, n in enumerate(ns):
        wav[b, :n] = synth.wav16(seed * 1000 + b, 1, int(n))[0]
    ids = np.eye(4, dtype=np.float32)[np.arange(len(spec)) % 4]
    ids[::5] = 0.0
    return wav, ns, frames, ids


def _call(hip, m, ns, frames, layout, nd=None, fd=None):
    _lib, lib, _ = hip
    nd = torch.from_numpy(ns).cuda() if nd is None else nd
    fd = torch.from_numpy(frames).cuda() if fd is None else fd
    B, N_max, T_max = len(ns), int(ns.max()), int(frames.max())
    return lambda p: _lib.check(lib.ts_debug_face_generate_mixed(
        m.handle(), p["wav"], ns.ctypes.data_as(I32P), _lib.dptr(nd), frames.ctypes.data_as(I32P), _lib.dptr(fd), B, N_max, T_max, p["ids"],
        p["out"], p["hid"], _lib.stream_ptr(), layout))


def _padded(hip, m, wav, ns, frames, ids):
    _lib = hip[0]
    B, T_max = len(ns), int(frames.max())
    t = {"wav": torch.from_numpy(wav).cuda(), "ids": torch.from_numpy(ids).cuda(),
         "out": torch.full((B, T_max, 103), float("nan"), device="cuda"), "hid": torch.full((B, T_max, 768), float("nan"), device="cuda")}
    _call(hip, m, ns, frames, 0)({k: _lib.dptr(v) for k, v in t.items()})
    torch.cuda.synchronize()
    return t["out"].cpu().numpy(), t["hid"].cpu().numpy()


@pytest.mark.parametrize("spec,seed", [(FIVE, 1), (SPEC, 3)], ids=["five_clips", "24_clips_shuffled"])
def test_packed_equals_padded(hip, m, spec, seed):
    """`out` and `hidden` of the packed plan against the padded plan, one process: equal in every element (valid rows AND the zeros beyond
    a clip's frames).  Padded samples are NaN; the packed call's outputs sit between red zones and every element of them is written."""
    wav, ns, frames, ids = _table(spec, seed)
    B, T_max = len(ns), int(frames.max())
    want_out, want_hid = _padded(hip, m, wav, ns, frames, ids)
    assert all(np.isfinite(want_out[b, :t]).all() for b, t in enumerate(frames))
    r = run_both(_call(hip, m, ns, frames, 1), {"wav": (wav, F32), "ids": (ids, F32)},
                 {"out": ((B, T_max, 103), F32), "hid": ((B, T_max, 768), F32)})
    out, hid = r["out"].cpu().numpy(), r["hid"].cpu().numpy()
    for b, t in enumerate(frames):
        assert np.array_equal(out[b, :t], want_out[b, :t]), f"clip {b} ({ns[b]} samples, {t} frames): out differs from the padded plan"
        assert np.array_equal(hid[b, :t], want_hid[b, :t]), f"clip {b} ({ns[b]} samples, {t} frames): hidden differs from the padded plan"
        assert not out[b, t:].any() and not hid[b, t:].any(), f"clip {b}: rows beyond its {t} frames are not 0"
    assert np.array_equal(out, want_out) and np.array_equal(hid, want_hid)
    # `run_clips` reaches the public entry (layout=None) and passes a named layout through; which plan the public entry takes:
    # test_public_entry_takes_the_knobs_plan
    clips = [wav[b, :n] for b, n in enumerate(ns)]
    for layout in (None, 0, 1):
        got = m.run_clips(clips[:3], ids[:3], frames[:3], layout=layout)
        for b in range(3):
            assert np.array_equal(got[b].cpu().numpy(), want_out[b, :frames[b]]), f"run_clips(layout={layout}), clip {b}"


def test_no_stale_state(hip, m):
    """Small pass -> large pass -> the same small pass on one handle and stream: the buffers and tables the large pass grew and wrote leave
    nothing behind that the small pass reads."""
    small = _table(FIVE[:3], 5)
    large = _table(SPEC, 6)

    def run(t):
        wav, ns, frames, ids = t
        clips = [wav[b, :n] for b, n in enumerate(ns)]
        o, h = m.run_clips(clips, ids, frames, want_hidden=True, layout=1)
        return [x.cpu().numpy() for x in o], [x.cpu().numpy() for x in h]

    o1, h1 = run(small)
    run(large)
    o2, h2 = run(small)
    for b in range(3):
        assert np.array_equal(o1[b], o2[b]) and np.array_equal(h1[b], h2[b]), f"clip {b}: the second small pass differs from the first"


def _levels(n_rows):
    L = [int(n_rows)]
    for k in FC_K:
        L.append((L[-1] - k) // 2 + 1)
    return L


def gemm_flops(feature_rows, R, M):
    """2 M N K over every GEMM launch of one face pass (csrc/face.cpp::face_run; K as the layers are packed: a k = 3 layer is 3 taps of its
    input channels): feature_rows[i] = output rows of feature convolution i, R = transformer rows, M = B T_max rows of everything else."""
    f = sum(2 * feature_rows[i] * 512 * (k * 512) for i, k in enumerate(FC_K))
    f += 2 * M * 768 * 512                                                # feature projection
    f += 2 * M * 48 * (128 * 48) * 16                                     # positional convolution: 16 groups of 48 channels, 128 taps
    f += 12 * 2 * R * (768 * 2304 + 768 * 768 + 768 * 3072 + 3072 * 768)  # QKV, out-proj, FFN1, FFN2
    f += 2 * M * 256 * 768                                                # audio_feature_map
    f += 2 * (2 * M * 256 * 3 * 320) + 2 * (2 * M * 256 * 3 * 256)        # SeqTranslator1D: layer 0 and its residual conv, layers 1 and 2
    f += 2 * M * 64 * 3 * 256 + 2 * (2 * M * 64 * 3 * 64) + 2 * M * 3 * 64          # jaw head
    f += 3 * (2 * M * 256 * 3 * 256) + 2 * M * 100 * 256                  # expression head
    return float(f)


def test_prof_counters(hip, m):
    """One pass of the 24-clip table under `ts_prof`: the GEMM family's flops are the closed form of the layout — the feature convolutions
    over the one packed axis, the transformer over sum(frames) rows — and below the padded plan's; attention still launches once per layer."""
    _lib, lib, ctx = hip
    wav, ns, frames, ids = _table(SPEC, 3)
    B, N_max, T_max = len(ns), int(ns.max()), int(frames.max())
    t = {"wav": torch.from_numpy(wav).cuda(), "ids": torch.from_numpy(ids).cuda(),
         "out": torch.empty((B, T_max, 103), device="cuda"), "hid": torch.empty((B, T_max, 768), device="cuda")}
    ptrs = {k: _lib.dptr(v) for k, v in t.items()}
    nd, fd = torch.from_numpy(ns).cuda(), torch.from_numpy(frames).cuda()
    ms, n, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
    got = {}
    for layout in (0, 1):
        _call(hip, m, ns, frames, layout, nd, fd)(ptrs)                   # buffers grown outside the count
        _lib.check(lib.ts_prof_enable(ctx, 1))
        try:
            _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
            _call(hip, m, ns, frames, layout, nd, fd)(ptrs)
            torch.cuda.synchronize()
            _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
        finally:
            _lib.check(lib.ts_prof_enable(ctx, 0))
        got[layout] = (list(n), list(fl))
        print(f"\nlayout {layout}: launches per family {list(n)}, flops per family {[f'{v:.6e}' for v in fl]}")
    off = np.zeros(B + 1, np.int64)
    lv = np.zeros(7, np.int64)
    assert lib.ts_debug_face_packed_layout(ns.ctypes.data_as(I32P), frames.ctypes.data_as(I32P), B, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                           None, lv.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    M, R = B * T_max, int(frames.sum())
    padded_levels = _levels((N_max - 10) // 5 + 1)
    want_padded = gemm_flops([B * v for v in padded_levels[1:]], M, M)
    want_packed = gemm_flops(lv[1:].tolist(), R, M)
    print(f"closed forms: padded {want_padded:.6e}, packed {want_packed:.6e} ({want_packed / want_padded:.3f} of padded)")
    assert got[0][1][0] == want_padded, "the closed form does not describe the padded plan"
    assert got[1][1][0] == want_packed
    assert got[1][1][0] < got[0][1][0]
    assert got[1][0][3] == 12 and got[0][0][3] == 12                      # attention: one launch per layer
    assert got[1][0][0] == got[0][0][0]                                   # the same GEMM launches, on fewer rows
    assert got[1][1][3] == got[0][1][3]                                   # attention flops: sum of frames^2 in both plans


def test_public_entry_takes_the_knobs_plan(hip, m):
    """`ts_face_generate_mixed` itself (no layout named) under `ts_prof`: its GEMM flops are the closed form of the plan `TS_FACE_PACK` names
    (unset or 0: padded, the default; 1: packed) on the 5-clip set, where the two differ — the bits cannot tell the plans apart, the counters do."""
    _lib, lib, ctx = hip
    wav, ns, frames, ids = _table(FIVE, 1)
    B, N_max, T_max = len(ns), int(ns.max()), int(frames.max())
    t = {"wav": torch.from_numpy(wav).cuda(), "ids": torch.from_numpy(ids).cuda(), "out": torch.empty((B, T_max, 103), device="cuda")}
    nd, fd = torch.from_numpy(ns).cuda(), torch.from_numpy(frames).cuda()

    def call():
        _lib.check(lib.ts_face_generate_mixed(m.handle(), _lib.dptr(t["wav"]), ns.ctypes.data_as(I32P), _lib.dptr(nd), frames.ctypes.data_as(I32P),
                                              _lib.dptr(fd), B, N_max, T_max, _lib.dptr(t["ids"]), _lib.dptr(t["out"]), None, _lib.stream_ptr()))

    ms, n, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
    call()                                                                # buffers grown outside the count
    _lib.check(lib.ts_prof_enable(ctx, 1))
    try:
        _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
        call()
        torch.cuda.synchronize()
        _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
    finally:
        _lib.check(lib.ts_prof_enable(ctx, 0))
    lv = np.zeros(7, np.int64)
    assert lib.ts_debug_face_packed_layout(ns.ctypes.data_as(I32P), frames.ctypes.data_as(I32P), B, None, None,
                                           lv.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    M, R = B * T_max, int(frames.sum())
    want_packed = gemm_flops(lv[1:].tolist(), R, M)
    want_padded = gemm_flops([B * v for v in _levels((N_max - 10) // 5 + 1)[1:]], M, M)
    print(f"\npublic entry: GEMM flops {fl[0]:.6e}; closed forms: packed {want_packed:.6e}, padded {want_padded:.6e}")
    assert want_packed < want_padded
    assert fl[0] == (want_packed if os.environ.get("TS_FACE_PACK", "0") not in ("", "0") else want_padded)
