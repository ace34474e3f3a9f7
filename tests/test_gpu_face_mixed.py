"""Mixed face passes: clips of DIFFERENT lengths in one pass of the face generator (`ts_face_generate_mixed`,
`FaceGenerator.run_clips`, `TrainWrapper.generate_clips`).

The contract under test (include/talkshow_hip.h): a clip's rows do not depend on what it shares the pass with, and equal
`ts_face_generate` on the clip alone in a process without the stream-K band.  So the bar of every comparison with the clip alone is
EQUALITY (`array_equal`), and the bar against the reference's goldens is the suite's existing 1e-4 — nothing here introduces a
tolerance.  Every test fails on a build without the feature: the entry point and `run_clips` do not exist there.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from talkshow_amd import synth
from test_gpu_canary import F32, run_both

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)

# (samples, frames or None = samples * 30 // 16000): 24 clips, 22 distinct sample counts; frame counts that straddle the attention tile of 64
# (63, 64, 65, 127, 128, 129), the minimum clip (400 samples, one frame), explicit frame counts below and above the default
SPEC = [(33613, None), (34200, None), (34700, None), (68300, None), (68900, None), (400, 1), (401, 1), (16000, None), (16001, 29),
        (23456, 50), (8000, None), (8533, 17), (12345, None), (45001, None), (50000, 90), (33613, 64), (5000, None), (640, None),
        (1200, 2), (20011, None), (27000, None), (30001, 60), (9999, None), (68300, 127)]


def _frames(n, f):
    return n * 30 // 16000 if f is None else f


@pytest.fixture(scope="module")
def m():
    from talkshow_amd.modules import FaceGenerator
    g = FaceGenerator().cuda()
    g.load_state_dict(synth.to_torch(synth.face_state_dict(seed=7)))      # the weights every reference golden was made with
    return g


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    return _lib, _lib.load(), _lib.context(0)


def _clips(seed, spec):
    order = np.random.default_rng(seed).permutation(len(spec))
    spec = [spec[i] for i in order]
    wavs = [synth.wav16(seed * 1000 + k, 1, n)[0] for k, (n, _) in enumerate(spec)]
    frames = np.asarray([_frames(n, f) for n, f in spec], np.int32)
    ids = np.eye(4, dtype=np.float32)[np.arange(len(spec)) % 4]
    ids[::5] = 0.0                                                        # some clips under the all-zero identity row
    return wavs, frames, ids


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _recording(name, g):
    """The golden's input samples; what the uniform test skips on (a host resampler that does not reproduce them) is a failure here."""
    from test_gpu_real_audio import _wav16
    try:
        return _wav16(name, g)
    except pytest.skip.Exception as e:
        pytest.fail(f"{name}: {e}")


def test_reference_parity_on_recordings_in_one_pass(golden, m):
    """The three recordings (300 / 384 / 288 frames), each under the zero id row and under its one-hot row: six clips of three lengths,
    interleaved, in ONE pass with hidden states, against the reference's outputs at the suite's 1e-4."""
    from test_gpu_real_audio import RECS, _tag
    g = golden("real_audio_face")
    wavs, ids, frames, who = [], [], [], []
    for hot in (False, True):
        for name in RECS:
            t = _tag(name)
            N, frame, spk = (int(v) for v in g[t + "_n"])
            wav = _recording(name, g)
            assert wav.shape == (N,)
            wavs.append(wav)
            frames.append(frame)
            ids.append(np.eye(4, dtype=np.float32)[spk] if hot else np.zeros(4, np.float32))
            who.append((t, hot))
    assert len(wavs) == 6 and sorted(set(frames)) == [288, 300, 384]
    outs, hids = m.run_clips(wavs, np.stack(ids), frames, want_hidden=True)
    for (t, hot), o, h in zip(who, _np(outs), _np(hids)):
        assert_close_measured(f"face_mixed.{t}.{'one_hot' if hot else 'zero_id'}", o, g[t + ("_out_one_hot" if hot else "_out_zero_id")], 1e-4)
        assert_close_measured(f"face_mixed.{t}.hidden.{'one_hot' if hot else 'zero_id'}", h[::6], g[t + "_hidden_6"], 1e-4)


def test_bit_identity_regardless_of_company(m):
    """24 clips of 22 sample counts in one pass: every clip's rows equal the clip through `run_clips` alone, and the same clip in a second
    pass of another composition and order."""
    wavs, frames, ids = _clips(3, SPEC)
    assert len(wavs) >= 24 and len({w.shape[0] for w in wavs}) >= 12 and {1, 63, 64, 65, 128, 129} <= set(frames.tolist())
    assert any(f != w.shape[0] * 30 // 16000 for w, f in zip(wavs, frames))
    outs, hids = m.run_clips(wavs, ids, frames, want_hidden=True)
    outs, hids = _np(outs), _np(hids)
    for b in range(len(wavs)):
        assert outs[b].shape == (frames[b], 103) and hids[b].shape == (frames[b], 768)
        o, h = m.run_clips([wavs[b]], ids[b:b + 1], frames[b:b + 1], want_hidden=True)
        assert np.array_equal(outs[b], o[0].cpu().numpy()), f"clip {b} ({wavs[b].shape[0]} samples, {frames[b]} frames): out differs from the clip alone"
        assert np.array_equal(hids[b], h[0].cpu().numpy()), f"clip {b} ({wavs[b].shape[0]} samples, {frames[b]} frames): hidden differs from the clip alone"
    perm = np.random.default_rng(9).permutation(len(wavs))[:15]           # fewer clips, another order, another longest clip
    extra = synth.wav16(77, 1, 51234)[0]
    outs2 = _np(m.run_clips([extra] + [wavs[i] for i in perm], np.concatenate([ids[:1], ids[perm]]),
                            np.concatenate([[96], frames[perm]]).astype(np.int32)))
    for k, i in enumerate(perm):
        assert np.array_equal(outs[i], outs2[1 + k]), f"clip {i}: rows depend on the pass it rides in"
    # the default frame counts are samples * 30 // 16000
    d = m.run_clips(wavs[:3], ids[:3])
    assert [x.shape[0] for x in d] == [w.shape[0] * 30 // 16000 for w in wavs[:3]]


def test_rows_equal_uniform_entry(m):
    """Mixed rows against `FaceGenerator.run(wav[None], id, frames)` on the clip alone (equal wherever the uniform entry takes no stream-K
    band; the spawning test below runs this under TS_CONV_SK=0, with both conv0 statistics forms)."""
    wavs, frames, ids = _clips(3, SPEC)
    outs, hids = m.run_clips(wavs, ids, frames, want_hidden=True)
    for b in range(len(wavs)):
        o, h = m.run(wavs[b][None], ids[b:b + 1], int(frames[b]), want_hidden=True)
        assert np.array_equal(outs[b].cpu().numpy(), o[0].cpu().numpy()), f"clip {b} ({wavs[b].shape[0]} samples, {frames[b]} frames): out"
        assert np.array_equal(hids[b].cpu().numpy(), h[0].cpu().numpy()), f"clip {b} ({wavs[b].shape[0]} samples, {frames[b]} frames): hidden"


# launches per family (conv, skinny, misc, attention) of ts_face_generate with the identity channels, any batch, as counted on the parent
# commit ae74f73: 69 GEMM launches; conv0, lerp_ln, 34 LayerNorms and fill_id; 12 attention launches
UNIFORM_LAUNCHES = [69, 0, 37, 12]


def test_uniform_entry_untouched(hip, m):
    """`ts_face_generate` at batch 4 issues the launches it issued before the mixed entry existed, and (without the stream-K band) equals
    a mixed pass of four equal-length clips bit for bit."""
    _lib, lib, ctx = hip
    N, frame = 40000, 75
    wav = synth.wav16(5, 4, N)
    ids = np.eye(4, dtype=np.float32)
    ms, n, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
    m.run(wav, ids, frame)                                                # buffers grown outside the count
    _lib.check(lib.ts_prof_enable(ctx, 1))
    try:
        _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
        out = m.run(wav, ids, frame)
        torch.cuda.synchronize()
        _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
    finally:
        _lib.check(lib.ts_prof_enable(ctx, 0))
    print(f"\nts_face_generate launches per family at batch 4: {list(n)}")
    assert list(n) == UNIFORM_LAUNCHES
    mixed = m.run_clips([w for w in wav], ids, [frame] * 4)
    for b in range(4):
        assert np.array_equal(out[b].cpu().numpy(), mixed[b].cpu().numpy()), f"clip {b}"


@pytest.mark.parametrize("env", [{"TS_CONV_SK": "0"}, {"TS_CONV_SK": "0", "TS_W2V_MOMENTS": "0"}], ids=["sk0", "sk0_direct_stats"])
def test_uniform_entry_identity_without_band(env):
    """The two comparisons with the uniform entry in a process that runs without the stream-K band (the levers are read once per process
    -> child process), with conv0's statistics from the second moments and from the convolution pass."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
                        "test_rows_equal_uniform_entry or test_uniform_entry_untouched"], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout


def test_production_shape(golden, m):
    """64 clips of the recordings' sample counts and a spread around them: the first and the last clip of each length against the clip
    alone in a mixed pass of one, and style.wav inside that pass against its golden."""
    g = golden("real_audio_face")
    style = _recording("style.wav", g)
    N, frame, spk = (int(v) for v in g["style_n"])
    rng = np.random.default_rng(4)
    base = [160000, 204800, 153600, 160533, 161111, 80000, 52001, 24000]
    ns = [base[i] for i in rng.integers(0, len(base), 64)]
    ns[11] = N
    wavs = [synth.wav16(900 + k, 1, n)[0] for k, n in enumerate(ns)]
    wavs[11] = style
    ids = np.eye(4, dtype=np.float32)[np.arange(64) % 4]
    ids[11] = np.eye(4, dtype=np.float32)[spk]
    outs = _np(m.run_clips(wavs, ids))
    assert_close_measured("face_mixed.style.one_hot_in_pass_of_64", outs[11], g["style_out_one_hot"], 1e-4)
    picked = {}
    for b, n in enumerate(ns):
        picked.setdefault(n, [b, b])[1] = b
    for b in sorted({x for pair in picked.values() for x in pair}):
        alone = m.run_clips([wavs[b]], ids[b:b + 1])[0].cpu().numpy()
        assert np.array_equal(outs[b], alone), f"clip {b} ({ns[b]} samples)"


@pytest.mark.parametrize("B", [1, 3, 33])
def test_memory_contract_under_canaries(hip, m, B):
    """Inputs between NaN zones with NaN in every sample at or beyond ns[b]; out and hidden between red zones, pre-filled with the sentinel:
    zones intact, every element written, rows at or beyond frames[b] exactly 0, bit-equal to the plain call and to `run_clips`."""
    _lib, lib, ctx = hip
    rng = np.random.default_rng(B)
    ns = (2 * rng.integers(200, 9000, B) + 1).astype(np.int32)           # odd sample counts
    ns[0] = 17999
    frames = (ns.astype(np.int64) * 30 // 16000).astype(np.int32)
    frames[frames < 1] = 1
    N_max, T_max = int(ns.max()), int(frames.max())
    clips = [synth.wav16(300 + b, 1, int(n))[0] for b, n in enumerate(ns)]
    wav = np.full((B, N_max), np.nan, np.float32)
    for b, c in enumerate(clips):
        wav[b, :ns[b]] = c
    ids = np.eye(4, dtype=np.float32)[np.arange(B) % 4]
    nd, fd = torch.from_numpy(ns).cuda(), torch.from_numpy(frames).cuda()
    r = run_both(lambda p: _lib.check(lib.ts_face_generate_mixed(
        m.handle(), p["wav"], ns.ctypes.data_as(I32P), _lib.dptr(nd), frames.ctypes.data_as(I32P), _lib.dptr(fd), B, N_max, T_max, p["ids"],
        p["out"], p["hid"], _lib.stream_ptr())),
        {"wav": (wav, F32), "ids": (ids, F32)}, {"out": ((B, T_max, 103), F32), "hid": ((B, T_max, 768), F32)})
    out, hid = r["out"].cpu().numpy(), r["hid"].cpu().numpy()
    clean, clean_h = m.run_clips(clips, ids, want_hidden=True)
    for b in range(B):
        t = int(frames[b])
        assert not out[b, t:].any() and not hid[b, t:].any(), f"clip {b}: rows beyond its {t} frames are not 0"
        assert np.isfinite(out[b, :t]).all() and np.isfinite(hid[b, :t]).all()
        assert np.array_equal(out[b, :t], clean[b].cpu().numpy()) and np.array_equal(hid[b, :t], clean_h[b].cpu().numpy())


def test_errors(hip, m):
    """Every rejected input of the contract returns non-zero with its message, and nothing is written to `out`."""
    _lib, lib, ctx = hip
    B, N_max, T_max = 3, 8000, 15
    wav = torch.from_numpy(synth.wav16(1, B, N_max)).cuda()
    ids = torch.zeros((B, 4), dtype=torch.float32, device="cuda")
    out = torch.full((B, T_max, 103), 7.0, dtype=torch.float32, device="cuda")

    def call(ns, frames, null=None):
        ns, frames = np.asarray(ns, np.int32), np.asarray(frames, np.int32)
        nd, fd = torch.from_numpy(ns).cuda(), torch.from_numpy(frames).cuda()
        args = [ns.ctypes.data_as(I32P), _lib.dptr(nd), frames.ctypes.data_as(I32P), _lib.dptr(fd)]
        if null is not None:
            args[null] = None
        rc = lib.ts_face_generate_mixed(m.handle(), _lib.dptr(wav), *args, B, N_max, T_max, _lib.dptr(ids), _lib.dptr(out), None,
                                        _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, lib.ts_last_error().decode()

    good_n, good_f = [8000, 4000, 400], [15, 7, 1]
    assert call(good_n, good_f)[0] == 0
    out.fill_(7.0)
    for ns, fr, null, msg in [([8000, 399, 400], good_f, None, "shorter than 400 samples"), (good_n, [15, 0, 1], None, "has no frames"),
                              ([8001, 4000, 400], good_f, None, "longer than N_max"), (good_n, [16, 7, 1], None, "more frames than T_max"),
                              (good_n, good_f, 0, "null length table"), (good_n, good_f, 1, "null length table"),
                              (good_n, good_f, 2, "null length table"), (good_n, good_f, 3, "null length table")]:
        rc, err = call(ns, fr, null)
        assert rc != 0 and msg in err, (rc, err)
    m.set_arith(3)
    try:
        rc, err = call(good_n, good_f)
        assert rc != 0 and "not offered in a mixed pass" in err, (rc, err)
    finally:
        m.set_arith(0)
    assert bool((out == 7.0).all()), "a rejected call wrote to out"


def test_wrapper_generate_clips(golden):
    """`TrainWrapper.generate_clips` on the three recordings as .wav paths beside sample arrays: list of float32 numpy (frames, 103), the
    recordings within 1e-4 of the reference (zero id and one class index per clip)."""
    import argparse
    import json

    import nets
    from talkshow_amd.config import Object
    from test_gpu_real_audio import RECS, _need_recording, _tag
    g = golden("real_audio_face")
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    w = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    clips = [_need_recording(n) for n in RECS] + [synth.wav16(2, 1, 12345)[0]]
    outs = w.generate_clips(clips)
    assert len(outs) == 4 and outs[3].shape == (12345 * 30 // 16000, 103) and all(o.dtype == np.float32 for o in outs)
    spk = [int(g[_tag(n) + "_n"][2]) for n in RECS]
    hot = w.generate_clips(clips, ids=spk + [0])
    for k, name in enumerate(RECS):
        t = _tag(name)
        assert_close_measured(f"face_mixed.{t}.wav_in_zero_id", outs[k], g[t + "_out_zero_id"], 1e-4)
        assert_close_measured(f"face_mixed.{t}.wav_in_one_hot", hot[k], g[t + "_out_one_hot"], 1e-4)
