"""Recordings of DIFFERENT lengths, one pass from samples to 265-d rows: the mixed front-end (`ts_mfcc_forward_mixed`,
`ts_mfcc_resample_mixed`, `ts_resample_kaiser_mixed`), the mixed assembly (`ts_assemble_full_mixed`) and the Python entries over them
(`MFCC.run_clips`, `TrainWrapper.generate_clips_from_wav`, `parallel.whole_body_clips`).

The contract under test (include/talkshow_hip.h): a recording's rows do not depend on what it shares the call with and equal the
uniform entry on the recording alone.  Every comparison is `np.array_equal`; every padded input element beyond a recording's own
length is NaN; every output of a C entry sits between red zones, pre-filled with the sentinel.  Every test fails on a build without
the feature: the symbols and attributes do not exist there.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from talkshow_amd.frontend import mixed_tables
from test_gpu_canary import F32, Guarded, run_both

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)
# 16 kHz sample counts, unsorted, 0.05 - 1 s: the shortest clip the STFT takes (746 -> 1026 > 1024 resampled samples), the pair that straddles a
# frame boundary (5872 -> 12 rows, 5871 -> 11), counts either side of a resampler block of 256 outputs, two equal
NS = [16000, 746, 5872, 5871, 1602, 8001, 8000, 12345, 16000, 2935]
BODY_NS = [5872, 16000, 1602, 8001, 5872, 12345]          # six clips, two equal, every one with at least one code row


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


@pytest.fixture(scope="module")
def w():
    import bench
    return bench.build_models(0, seed=7)[0]


@pytest.fixture(scope="module")
def face():
    import argparse
    import json

    import nets
    from talkshow_amd.config import Object
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    f = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    f.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    return f


def _wavs(seed, ns):
    return [synth.wav16(seed * 1000 + k, 1, int(n))[0] for k, n in enumerate(ns)]


def _nan_block(wavs, N_max=None):
    ns = np.asarray([len(x) for x in wavs], np.int32)
    blk = np.full((len(wavs), int(ns.max()) if N_max is None else N_max), np.nan, np.float32)
    for b, x in enumerate(wavs):
        blk[b, :len(x)] = x
    return blk, ns


def _np(t):
    return t.cpu().numpy()


# ---- 1. the front-end, stage by stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out,fps,ns", [(16000, 22000, 30, NS), (44100, 22000, 30, [2300, 9000, 4567, 6001]),
                                                 (22000, 22000, 30, [22000, 1025, 8074, 3000]), (16000, 22000, 15, NS[:6])],
                         ids=["16k_lds", "44k1_plain", "no_resampling", "fps15"])
def test_front_end_stage_by_stage(hip, sr_in, sr_out, fps, ns):
    _lib, lib, ctx = hip
    from talkshow_amd.modules import MFCC
    m = MFCC(sr_in, sr_out, fps)
    wavs = _wavs(sr_in // 100 + fps, ns)
    blk, ns32 = _nan_block(wavs)
    B, N_max = blk.shape
    tab = mixed_tables(ns, sr_in, sr_out, fps)
    N22_max, T_max = int(lib.ts_mfcc_resampled_len(m._h, N_max)), int(lib.ts_mfcc_num_frames(m._h, N_max))
    assert N22_max == tab["n_resampled"].max() and T_max == tab["mfcc_rows"].max()
    nd = torch.from_numpy(ns32).cuda()
    r = run_both(lambda p: _lib.check(lib.ts_mfcc_resample_mixed(m._h, p["wav"], ns32.ctypes.data_as(I32P), _lib.dptr(nd), B, N_max, p["x22"],
                                                                 _lib.stream_ptr())), {"wav": (blk, F32)}, {"x22": ((B, N22_max), F32)})
    x22 = _np(r["x22"])
    r = run_both(lambda p: _lib.check(lib.ts_mfcc_forward_mixed(m._h, p["wav"], ns32.ctypes.data_as(I32P), _lib.dptr(nd), B, N_max, p["feat"],
                                                                _lib.stream_ptr())), {"wav": (blk, F32)}, {"feat": ((B, T_max, 64), F32)})
    feat = _np(r["feat"])
    assert not np.isnan(x22).any() and not np.isnan(feat).any()
    for b, x in enumerate(wavs):
        n22, T = int(tab["n_resampled"][b]), int(tab["mfcc_rows"][b])
        assert T == lib.ts_mfcc_num_frames(m._h, len(x)) and n22 == lib.ts_mfcc_resampled_len(m._h, len(x))
        assert np.array_equal(x22[b, :n22], _np(m.resample(x))[0]), f"clip {b} ({len(x)} samples): resampled samples differ from the clip alone"
        assert not x22[b, n22:].any()
        assert np.array_equal(feat[b, :T], _np(m(x))[0]), f"clip {b} ({len(x)} samples): MFCC rows differ from the clip alone"
        assert not feat[b, T:].any() and not np.signbit(feat[b, T:]).any()


def test_rows_do_not_depend_on_the_company():
    from talkshow_amd.modules import MFCC
    m = MFCC(16000)
    wavs = _wavs(5, NS)
    a = [_np(t) for t in m.run_clips(wavs)]
    assert [t.shape for t in a] == [(int(T), 64) for T in mixed_tables(NS, 16000)["mfcc_rows"]]
    pick = [7, 2, 1, 3]                                                # another order, another longest clip, fewer clips
    b = [_np(t) for t in m.run_clips([wavs[i] for i in pick] + [synth.wav16(99, 1, 20011)[0]])]
    for k, i in enumerate(pick):
        assert np.array_equal(a[i], b[k]), f"clip {i}: rows depend on the pass it rides in"
    for i in (1, 2, 8):                                                # alone in a mixed pass of one
        assert np.array_equal(a[i], _np(m.run_clips([wavs[i]])[0]))
    r = m.resample_clips([torch.from_numpy(x).cuda() for x in wavs[:4]])          # recordings that already live on the device
    for i in range(4):
        assert np.array_equal(_np(r[i]), _np(m.resample(wavs[i]))[0])


@pytest.mark.parametrize("sr_in", [22050, 44100])
def test_kaiser_resampler(hip, sr_in):
    _lib, lib, ctx = hip
    from talkshow_amd.modules import resample_kaiser_clips, resample_kaiser_device
    ns = [9001, 2300, 22050, 4567]
    wavs = _wavs(sr_in // 50, ns)
    blk, ns32 = _nan_block(wavs)
    B, N_max = blk.shape
    W = int(lib.ts_resample_kaiser_len(N_max, sr_in, 16000))
    nd = torch.from_numpy(ns32).cuda()
    r = run_both(lambda p: _lib.check(lib.ts_resample_kaiser_mixed(ctx, p["wav"], ns32.ctypes.data_as(I32P), _lib.dptr(nd), B, N_max, sr_in, 16000,
                                                                   p["out"], _lib.stream_ptr())), {"wav": (blk, F32)}, {"out": ((B, W), F32)})
    out = _np(r["out"])
    assert not np.isnan(out).any()
    clips = resample_kaiser_clips(wavs, sr_in, 16000)
    for b, x in enumerate(wavs):
        alone = _np(resample_kaiser_device(x[None], sr_in, 16000))[0]
        assert alone.shape == (int(mixed_tables([len(x)], sr_in)["n16"][0]),)
        assert np.array_equal(out[b, :len(alone)], alone), f"clip {b} ({len(x)} samples at {sr_in})"
        assert not out[b, len(alone):].any()
        assert np.array_equal(_np(clips[b]), alone)


# ---- 2. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(hip):
    _lib, lib, ctx = hip
    from talkshow_amd.modules import MFCC
    m = MFCC(16000)
    B, N_max = 3, 8000
    wav = torch.from_numpy(synth.wav16(1, B, N_max)).cuda()
    T_max, N22 = int(lib.ts_mfcc_num_frames(m._h, N_max)), int(lib.ts_mfcc_resampled_len(m._h, N_max))
    K16 = int(lib.ts_resample_kaiser_len(N_max, 44100, 16000))
    outs = {"feat": Guarded((B, T_max, 64), F32), "x22": Guarded((B, N22), F32), "w16": Guarded((B, N_max), F32), "k16": Guarded((B, K16), F32)}
    before = {k: g.bits() for k, g in outs.items()}

    def call(ns, null=None, B_=B, which=(0, 1, 2, 3)):
        ns = np.asarray(ns, np.int32)
        nd = torch.from_numpy(ns).cuda()
        tabs = [ns.ctypes.data_as(I32P), _lib.dptr(nd)]
        if null is not None:
            tabs[null] = None
        entries = [lambda: lib.ts_mfcc_forward_mixed(m._h, _lib.dptr(wav), *tabs, B_, N_max, outs["feat"].ptr(), _lib.stream_ptr()),
                   lambda: lib.ts_mfcc_resample_mixed(m._h, _lib.dptr(wav), *tabs, B_, N_max, outs["x22"].ptr(), _lib.stream_ptr()),
                   lambda: lib.ts_resample_kaiser_mixed(ctx, _lib.dptr(wav), *tabs, B_, N_max, 16000, 16000, outs["w16"].ptr(), _lib.stream_ptr()),
                   lambda: lib.ts_resample_kaiser_mixed(ctx, _lib.dptr(wav), *tabs, B_, N_max, 44100, 16000, outs["k16"].ptr(), _lib.stream_ptr())]
        rcs = [entries[k]() for k in which]
        torch.cuda.synchronize()
        return rcs

    assert mixed_tables([744], 16000)["n_resampled"][0] == 1023       # <= half an FFT window: the uniform entry's rule
    assert call([8000, 744, 4000], which=(0,))[0] != 0 and "half an FFT window" in lib.ts_last_error().decode()
    # two samples at 44.1 kHz give int(2 * 16000 / 44100) = 0 samples at 16 kHz: the rule of the uniform Kaiser entry
    assert call([8000, 2, 4000], which=(3,))[0] != 0 and "too short for this rate change" in lib.ts_last_error().decode()
    for ns, null, B_ in [([8001, 4000, 2000], None, B), ([8000, 4000, 2000], 0, B), ([8000, 4000, 2000], 1, B), ([8000, 4000, 2000], None, 0),
                         ([8000, 0, 2000], None, B)]:
        assert all(rc != 0 for rc in call(ns, null, B_)), (ns, null, B_)
    for k, g in outs.items():
        assert g.zones_intact() and np.array_equal(g.bits(), before[k]), f"a rejected call wrote to {k}"
    assert all(rc == 0 for rc in call([8000, 4000, 2000]))
    assert all(g.zones_intact() and not (g.bits() == g.sent).any() for g in outs.values())


# ---- 3. assembly -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stand", [False, True])
def test_assemble_full_mixed(hip, stand):
    _lib, lib, ctx = hip
    from talkshow_amd.pose_index import assemble_full, lower_pose_block
    pairs = [(8, 12), (12, 12), (16, 9), (4, 1), (4, 30)]
    B, Tb, Tf = len(pairs), 16, 30
    rng = np.random.default_rng(2)
    body = np.full((B, Tb, 129), np.nan, np.float32)
    fc = np.full((B, Tf, 103), np.nan, np.float32)
    for b, (tb, tf) in enumerate(pairs):
        body[b, :tb] = rng.standard_normal((tb, 129))
        fc[b, :tf] = rng.standard_normal((tf, 103))
    tbd = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    tfd = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    lp = lower_pose_block(stand)
    r = run_both(lambda p: _lib.check(lib.ts_assemble_full_mixed(ctx, p["body"], _lib.dptr(tbd), p["face"], _lib.dptr(tfd), B, Tb, Tf,
                                                                 _lib.fptr(lp), p["out"], _lib.stream_ptr())),
                 {"body": (body, F32), "face": (fc, F32)}, {"out": ((B, Tf, 265), F32)})
    out = _np(r["out"])
    for b, (tb, tf) in enumerate(pairs):
        alone = _np(assemble_full(body[b:b + 1, :tb], fc[b:b + 1, :tf], stand=stand))[0]
        assert np.array_equal(out[b, :tf], alone), f"clip {b} (tb {tb}, tf {tf})"
        assert not out[b, tf:].any() and not np.signbit(out[b, tf:]).any()                   # +0.0
    assert lib.ts_assemble_full_mixed(ctx, _lib.dptr(tbd), None, _lib.dptr(tbd), _lib.dptr(tfd), B, Tb, Tf, _lib.fptr(lp), _lib.dptr(tbd), None) != 0


# ---- 4. the body from recordings --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body_clips():
    from talkshow_amd.modules import MFCC
    wavs = _wavs(11, BODY_NS)
    m = MFCC(16000)
    return wavs, [m(x) for x in wavs], (np.arange(len(wavs)) % 4).astype(np.int64)


@pytest.mark.parametrize("how", ["greedy", "philox", "clip_indices"])
def test_body_from_recordings(w, body_clips, how):
    from talkshow_amd import _lib
    wavs, mfccs, ids = body_clips
    mode = _lib.TS_SAMPLE_GREEDY if how == "greedy" else _lib.TS_SAMPLE_PHILOX
    gidx = [40 + 3 * b for b in range(len(wavs))] if how == "clip_indices" else [100 + b for b in range(len(wavs))]
    res = w.generate_clips_from_wav(wavs, 16000, ids, mode=mode, seed=77, clip_index0=100, clip_indices=gidx if how == "clip_indices" else None)
    rows = mixed_tables(BODY_NS, 16000)
    for b, (codes, poses) in enumerate(res):
        assert codes.shape == (rows["code_rows"][b], 2) and poses.shape == (rows["pose_frames"][b], 129)
        sc, sp = w.generate_batch(mfccs[b], ids[b:b + 1], mode=mode, seed=77, clip_index0=gidx[b])
        assert np.array_equal(_np(codes), _np(sc)[0]), f"{how}: codes of clip {b} ({BODY_NS[b]} samples) differ from the clip alone"
        assert np.array_equal(_np(poses), _np(sp)[0]), f"{how}: poses of clip {b} ({BODY_NS[b]} samples) differ from the clip alone"


# ---- 5. the whole body ------------------------------------------------------------------------------------------------------------
def _alone(w, face, wav, sr, bid, fid, clip_index, seed, stand=False):
    """The route of existing entries on one recording."""
    from talkshow_amd import _lib
    from talkshow_amd.frontend import device_mfcc
    from talkshow_amd.modules import resample_kaiser_device
    from talkshow_amd.pose_index import assemble_full
    poses = w.generate_batch(device_mfcc(sr)(wav), np.asarray([bid], np.int64), mode=_lib.TS_SAMPLE_PHILOX, seed=seed, clip_index0=clip_index)[1]
    wav16 = wav if sr == 16000 else _np(resample_kaiser_device(wav[None], sr, 16000))[0]
    f = face.generator.run_clips([wav16], fid[None])[0]
    return _np(assemble_full(poses, f[None], stand=stand))[0]


@pytest.mark.parametrize("sr,ns", [(16000, BODY_NS), (22050, [2300, 22050, 11025])], ids=["16k", "22k05"])
def test_whole_body_clips(w, face, sr, ns):
    from talkshow_amd import parallel
    wavs = _wavs(sr // 10, ns)
    ids = (np.arange(len(ns)) % 4).astype(np.int64)
    fids = np.eye(4, dtype=np.float32)[(np.arange(len(ns)) + 1) % 4]
    fids[0] = 0.0
    out = parallel.whole_body_clips(w, face, wavs, sr, ids, fids, seed=9, clip_index0=20)
    frames = mixed_tables(ns, sr)["face_frames"]
    assert [tuple(o.shape) for o in out] == [(int(f), 265) for f in frames]
    out = [_np(o) for o in out]
    for b in range(len(ns)):
        assert np.array_equal(out[b], _alone(w, face, wavs[b], sr, ids[b], fids[b], 20 + b, 9)), f"clip {b} ({ns[b]} samples at {sr})"
    plain = parallel.whole_body_clips(w, face, wavs, sr, ids, fids, seed=9, clip_index0=20, overlap=False)
    assert all(np.array_equal(a, _np(b)) for a, b in zip(out, plain))
    stand = parallel.whole_body_clips(w, face, wavs[:2], sr, ids[:2], fids[:2], seed=9, clip_index0=20, stand=True)
    assert np.array_equal(_np(stand[1]), _alone(w, face, wavs[1], sr, ids[1], fids[1], 21, 9, stand=True))


# ---- 6. no synchronisation, no capture churn ---------------------------------------------------------------------------------------
def test_queued_calls_and_graph_captures(hip, w, face):
    _lib, lib, ctx = hip
    from talkshow_amd import parallel
    wavs = _wavs(21, BODY_NS)
    ids = (np.arange(len(wavs)) % 4).astype(np.int64)
    single = [_np(o) for o in parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=3)]
    torch.cuda.synchronize()
    streams = [_lib.stream_ptr(), C.c_void_p(parallel._side_stream(torch.device("cuda", 0)).cuda_stream)]
    cap = [lib.ts_pixelcnn_graph_captures(w.generator.handle(), s) for s in streams]
    again = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=3)
    torch.cuda.synchronize()
    assert [lib.ts_pixelcnn_graph_captures(w.generator.handle(), s) for s in streams] == cap, "a repeated pass captured a hipGraph"
    assert all(np.array_equal(a, _np(b)) for a, b in zip(single, again))
    # three calls queued back to back with no host synchronise between them, then one synchronise
    q = [parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=3) for _ in range(3)]
    torch.cuda.synchronize()
    for k in range(3):
        assert all(np.array_equal(a, _np(b)) for a, b in zip(single, q[k])), f"queued call {k} differs from the single call"
    # ... and with other recordings of other lengths between them: a host table read after its call returned would be the wrong table
    other = [x[:max(1602, len(x) - 37 * (k + 1))][::-1].copy() for k, x in enumerate(wavs[::-1])]
    q = [parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=3), parallel.whole_body_clips(w, face, other, 16000, ids, None, seed=3),
         parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=3)]
    torch.cuda.synchronize()
    for k in (0, 2):
        assert all(np.array_equal(a, _np(b)) for a, b in zip(single, q[k])), f"interleaved call {k} differs from the single call"
    ref = [_np(o) for o in parallel.whole_body_clips(w, face, other, 16000, ids, None, seed=3)]
    assert all(np.array_equal(a, _np(b)) for a, b in zip(ref, q[1]))
