"""Wav sessions end to end (`MFCC.open_stream`, `TrainWrapper.open_stream(..., wav_sr=...)`; talkshow_hip.h, "wav sessions").

The yardsticks are the project's own one-shot entries — `MFCC(sr)(wav)` for the front end, `generate_batch(MFCC(sr)(wav), ...)` for the
seamless body session, `BodyStream.push` of the same frame blocks for the plain one — and every comparison is EQUALITY: codes as integers,
rows, poses and log-probabilities as uint32 bits.  No tolerance anywhere.

Front end: a tracked recording (its first 3 s; at 44100 Hz, which no tracked file has, the first 132 300 samples of the 22 kHz style.wav read as
           44.1 kHz audio: a signal of 3 s, not speech at its true pitch) beside synthetic noise, B = 2, at 16000 / 24000 / 44100 Hz, four chunkings each (one push;
           pushes of 1 sample, of 0 and of odd sizes; equal pushes; max_samples pushes).  Peak mode under `MFCC.peak_db` = the one-shot rows;
           running mode: the same rows for every chunking, the one-shot rows from the loudest row on, and everywhere where row 0 is loudest.
Body:      full-size synthetic networks (those of tests/test_gpu_seamless.py), B = 2, 65 000 samples at 16 kHz = 122 MFCC rows = 30 code rows,
           ten past the 20-row lag; greedy and Philox; codes, poses and log-probabilities; one chunking holds a push that yields no row.
Counters, refusals (each before any device work, no counter moves) and canaries (ragged B and n between poisoned zones; NaN beyond n).
"""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from talkshow_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(U32) if a.dtype == np.float32 else a


def recording(name, seconds=3, rate=None):
    """the first `seconds` of channel 0 at the file's own rate, or read as audio at `rate`"""
    from talkshow_amd.frontend import load_wav
    x, sr = load_wav(os.path.join(REPO, "tests", "golden", "audio", name))
    n = seconds * (sr if rate is None else rate)
    assert x.shape[1] >= n
    return np.ascontiguousarray(x[0, :n]), sr


def noise(seed, n, shape="swell"):
    rng = np.random.default_rng(seed)
    env = {"swell": np.sin(np.linspace(0.02, np.pi, n)) ** 2 + 1e-3, "decay": np.exp(-np.linspace(0.0, 14.0, n))}[shape]
    return (0.3 * rng.standard_normal(n) * env).astype(F32)


def chunkings(n, cap):
    odd = [1, 0, 1, 333, cap, 2, 0, 777]
    odd += [cap] * ((n - sum(odd)) // cap)
    odd += [n - sum(odd)]
    return {"one": [n], "odd": odd, "equal": [n // 7] * 7 + [n % 7], "cap": [cap] * (n // cap) + [n % cap]}


def stream_rows(m, wav, sizes, cap, db):
    st = m.open_stream(wav.shape[0], cap, db=db)
    bytes0, out, at = st.state_bytes, [], 0
    for n in sizes:
        f = st.plan(n)
        out.append(st.push(wav[:, at:at + n]))
        at += n
        assert tuple(out[-1].shape) == (wav.shape[0], f, 64) and st.samples_in == at and st.frames_out == sum(int(o.shape[1]) for o in out)
    f = st.plan(0, flush=True)
    out.append(st.flush())
    assert int(out[-1].shape[1]) == f and st.state_bytes == bytes0
    with pytest.raises(ValueError):
        st.push(wav[:, :1])
    st.close()
    return bits(torch.cat(out, dim=1))


@pytest.fixture(scope="module", params=[16000, 24000, 44100])
def clips(request):
    """(MFCC handle, wav (2, N) on the device, one-shot row bits, peak): row 0 a recording, row 1 noise that swells and fades"""
    from talkshow_amd.modules import MFCC
    sr = request.param
    rec, _ = recording({16000: "1st-page.wav", 24000: "french.wav", 44100: "style.wav"}[sr], 3, rate=sr)
    assert rec.shape[0] == 3 * sr
    wav = torch.from_numpy(np.stack([rec, noise(sr, rec.shape[0])])).cuda()
    m = MFCC(sr, 22000, 30)
    return m, wav, bits(m(wav)), m.peak_db(wav)


def test_peak_mode_equals_the_one_shot_rows(clips):
    m, wav, want, peak = clips
    N = int(wav.shape[1])
    cap = N // 3 + 1
    assert torch.equal(peak, m.peak_db([wav[0], wav[1]]))
    for name, sizes in chunkings(N, cap).items():
        assert sum(sizes) == N and max(sizes) <= N
        got = stream_rows(m, wav, sizes, max(cap, max(sizes)), peak)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), f"{name}: rows {sorted(set(np.argwhere(got != want)[:, 1].tolist()))[:10]} differ"


def test_running_mode_chunkings_agree_and_meet_the_one_shot(clips):
    m, wav, want, _ = clips
    N = int(wav.shape[1])
    cap = N // 3 + 1
    runs = {name: stream_rows(m, wav, sizes, max(cap, max(sizes)), "running") for name, sizes in chunkings(N, cap).items()}
    for name, got in runs.items():
        assert np.array_equal(got, runs["one"]), f"{name}: the running rows depend on the chunking"
    # from the loudest row on the running maximum IS the recording's maximum
    x = m.resample(wav)
    from talkshow_amd import _lib
    L, B, T = _lib.load(), 2, want.shape[1]
    power = torch.empty((B, T, 1056), dtype=torch.float32, device="cuda")
    mel = torch.empty((B, T, 256), dtype=torch.float32, device="cuda")
    _lib.check(L.ts_debug_mfcc_stft(m._h, _lib.dptr(x), B, int(x.shape[1]), _lib.dptr(power), _lib.stream_ptr()))
    _lib.check(L.ts_debug_mfcc_mel(m._h, _lib.dptr(power), None, B, T, _lib.dptr(mel), _lib.stream_ptr()))
    loudest = mel.amax(dim=2).argmax(dim=1).cpu().numpy()
    for b in range(B):
        t = int(loudest[b])
        assert np.array_equal(runs["one"][b, t:], want[b, t:]), f"clip {b}: rows from the loudest ({t}) on"
    assert int(loudest[1]) > 10, "the noise swells: its early rows are clamped lower than the one-shot clamps them"


def test_running_mode_equals_the_one_shot_when_row_0_is_loudest():
    from talkshow_amd.modules import MFCC
    m = MFCC(16000, 22000, 30)
    wav = torch.from_numpy(np.stack([noise(5, 20000, "decay"), noise(6, 20000, "decay")])).cuda()
    want = bits(m(wav))
    for sizes in ([20000], [1, 4999, 0, 7000, 8000]):
        assert np.array_equal(stream_rows(m, wav, sizes, 20000, "running"), want)


# ---- body sessions fed samples ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(tmp_path_factory):
    """The wrapper of tests/test_gpu_seamless.py (full-size synthetic networks), 2 clips of 65 000 samples at 16 kHz, their one-shot MFCC rows"""
    from nets.init_model import init_model
    from talkshow_amd.config import Object
    from talkshow_amd.modules import MFCC
    vq_path = str(tmp_path_factory.mktemp("wavstream") / "vq.pth")
    torch.save({"generator": {"g_body": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=39)),
                              "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))}}, vq_path)
    cfg = json.load(open(os.path.join(REPO, "config", "body_pixel.json")))
    cfg["Model"]["vq_path"] = vq_path
    w = init_model("s2g_body_pixel", argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                       "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))})
    N = 65000
    rec, sr = recording("1st-page.wav", 5)
    assert sr == 16000
    wav = torch.from_numpy(np.stack([rec[8000:8000 + N], noise(77, N)])).cuda()
    m = MFCC(16000, 22000, 30)
    mf = m(wav)
    assert mf.shape[1] == 122
    return dict(w=w, wav=wav, N=N, m=m, mf=mf, peak=m.peak_db(wav), ids=synth.speaker_ids(2), ref={})


def draw(mode):
    from talkshow_amd import _lib
    return dict(mode=_lib.TS_SAMPLE_GREEDY) if mode == "greedy" else dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=5)


BODY_SCHEDULES = {"three": [30000, 20000, 15000], "with-empty": [400, 0, 21000, 1, 9599, 16000, 18000]}


@pytest.mark.parametrize("mode", ["greedy", "philox"])
@pytest.mark.parametrize("sched", list(BODY_SCHEDULES))
def test_seamless_from_samples_returns_the_one_shot_bits(full, sched, mode):
    w, wav, sizes = full["w"], full["wav"], BODY_SCHEDULES[sched]
    assert sum(sizes) == full["N"]
    if mode not in full["ref"]:
        full["ref"][mode] = tuple(bits(o).copy() for o in w.generate_batch(full["mf"], full["ids"], logprobs=True, **draw(mode)))
    ref_codes, ref_poses, ref_lp = full["ref"][mode]
    assert ref_codes.shape == (2, 30, 2) and ref_poses.shape == (2, 120, 129)
    st = w.open_stream(full["ids"], 2, 48, seamless=True, wav_sr=16000, wav_db=full["peak"], max_samples=max(sizes))
    bytes0, parts, at, empty = st.state_bytes, [], 0, 0
    for n in sizes + [None]:
        f, rows, frames = st.plan_wav(0 if n is None else n, flush=n is None)
        out = (st.flush(return_codes=True, logprobs=True, **draw(mode)) if n is None else
               st.push_wav(wav[:, at:at + n], return_codes=True, logprobs=True, **draw(mode)))
        at += n or 0
        assert tuple(out[0].shape) == (2, frames, 129) and tuple(out[1].shape) == (2, rows, 2) and tuple(out[2].shape) == (2, rows, 2)
        empty += f == 0
        parts.append([bits(o) for o in out])
        assert st.samples_in == at and st.frames == sum(p[0].shape[1] for p in parts) and st.state_bytes == bytes0
    assert empty >= (2 if sched == "with-empty" else 0), "a push that yields no MFCC row is part of the case"
    assert st.frames_in == 122
    st.close()
    poses, codes, lp = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
    assert np.array_equal(codes, ref_codes), f"codes differ first at row {int(np.argwhere(codes != ref_codes)[:, 1].min())}"
    assert np.array_equal(poses, ref_poses), f"pose frames {sorted(set(np.argwhere(poses != ref_poses)[:, 1].tolist()))[:10]} differ"
    assert np.array_equal(lp, ref_lp)


def test_plain_session_from_samples_equals_the_same_frame_blocks(full):
    w, wav = full["w"], full["wav"]
    sizes = [20000, 3000, 22000, 20000]
    st = w.open_stream(full["ids"], 2, 48, wav_sr=16000, wav_db=full["peak"], max_samples=max(sizes))
    ref = w.open_stream(full["ids"], 2, st.max_frames)             # the plain session inside, opened again
    mf, at, t_at, carried = full["mf"], 0, 0, 0
    for n in sizes + [None]:
        f, rows, frames = st.plan_wav(0 if n is None else n, flush=n is None)
        got = st.flush(**draw("philox")) if n is None else st.push_wav(wav[:, at:at + n], **draw("philox"))
        at += n or 0
        t = (carried + f) // 4 * 4
        assert (rows, frames) == (t // 4, t) and tuple(got.shape) == (2, t, 129)
        if t:
            want = ref.push(mf[:, t_at:t_at + t].contiguous(), **draw("philox"))
            assert np.array_equal(bits(got), bits(want)), f"after {at} samples"
        t_at, carried = t_at + t, carried + f - t
    assert t_at == 120 and st.frames == ref.frames == 120
    st.close(), ref.close()


def test_refusals_come_before_any_device_work(full):
    from talkshow_amd import _lib
    w, wav, m = full["w"], full["wav"], full["m"]
    with pytest.raises(ValueError, match="not finite"):
        m.open_stream(2, 1000, db=np.array([1.0, np.nan], F32))
    with pytest.raises(ValueError, match="not finite"):
        w.open_stream(full["ids"], 2, 48, seamless=True, wav_sr=16000, wav_db=torch.tensor([np.inf, 0.0]))
    with pytest.raises(ValueError):
        m.open_stream(2, 1000, db=np.zeros(3, F32))
    st = w.open_stream(full["ids"], 2, 48, seamless=True, wav_sr=16000, wav_db=full["peak"], max_samples=4000)
    st.push_wav(wav[:, :4000])

    def state():
        return st.samples_in, st.frames_in, st.frames, st.body.frames_in, st.body.code_rows

    s0 = state()
    for bad in (wav[:1, :100], wav[0, :100], torch.zeros((2, 3, 4)), wav[:, :4001]):
        with pytest.raises(ValueError):
            st.push_wav(bad)
        assert state() == s0
    short = w.open_stream(full["ids"], 2, 48, seamless=True, wav_sr=16000, max_samples=700)
    short.push_wav(wav[:, :700])                                                        # 700 samples at 16 kHz: 963 resampled, not above 1024
    with pytest.raises(ValueError, match="shorter than half an FFT window"):
        short.flush()
    assert (short.samples_in, short.frames_in, short.frames) == (700, 0, 0)
    short.close()
    f, rows, _ = st.plan_wav(4000)
    for _ in range(8):                                              # up to a call that runs code rows
        if rows:
            break
        st.push_wav(wav[:, :4000])
        f, rows, _ = st.plan_wav(4000)
    assert rows > 0
    s0 = state()
    with pytest.raises(ValueError, match=f"runs {rows} code rows"):
        st.push_wav(wav[:, :4000], mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.zeros((2, rows + 1, 2), F32))
    assert state() == s0
    for name in ("restart", "save", "load", "fork"):
        with pytest.raises(NotImplementedError, match="sample clock"):
            getattr(st, name)([0])
    assert state() == s0
    st.flush()
    s1 = state()
    for call in (lambda: st.push_wav(wav[:, :10]), st.flush, lambda: st.plan_wav(10)):
        with pytest.raises(ValueError, match="flushed"):
            call()
    assert state() == s1
    st.close()


def test_ragged_shapes_between_poisoned_zones_and_nan_beyond_n():
    """B = 3 and odd n through the C entries: the samples sit in a NaN-poisoned buffer that holds (B, n) and nothing else for the library to read
    — poison right behind every call's samples leaves the bits unchanged — and the rows land between intact sentinel zones"""
    from talkshow_amd import _lib
    from talkshow_amd.modules import MFCC
    L = _lib.load()
    m, B, N, RZ = MFCC(16000, 22000, 30), 3, 7001, 1024
    rng = np.random.default_rng(8)
    wav = (0.2 * rng.standard_normal((B, N))).astype(F32)
    want = bits(m(torch.from_numpy(wav).cuda()))
    peak = m.peak_db(torch.from_numpy(wav).cuda())
    h = C.c_void_p()
    torch.cuda.synchronize()
    _lib.check(L.ts_mfcc_stream_open(m._h, B, 2500, 1, _lib.dptr(peak), C.byref(h)))
    cap = int(L.ts_mfcc_stream_max_frames(h))
    rows, at = [], 0
    for n in (1, 2499, 0, 2500, 1237, 764, None):
        SENT = np.float32(-7.25)
        out = torch.full((2 * RZ + B * cap * 64,), float(SENT), dtype=torch.float32, device="cuda")
        f = C.c_int(-1)
        if n is None:
            _lib.check(L.ts_mfcc_stream_flush(h, C.c_void_p(out.data_ptr() + 4 * RZ), C.byref(f), _lib.stream_ptr()))
        else:
            src = torch.full((2 * RZ + B * n,), float("nan"), dtype=torch.float32, device="cuda")
            src[RZ:RZ + B * n] = torch.from_numpy(np.ascontiguousarray(wav[:, at:at + n]).reshape(-1)).cuda()
            _lib.check(L.ts_mfcc_stream_push(h, C.c_void_p(src.data_ptr() + 4 * RZ), n, C.c_void_p(out.data_ptr() + 4 * RZ), C.byref(f),
                                             _lib.stream_ptr()))
            at += n
        img = out.cpu().numpy()
        used = B * f.value * 64
        assert np.all(img[:RZ] == SENT) and np.all(img[RZ + used:] == SENT), "rows were written outside (B, f, 64)"
        rows.append(img[RZ:RZ + used].reshape(B, f.value, 64).copy())
    torch.cuda.synchronize()
    L.ts_mfcc_stream_close(h)
    got = np.concatenate(rows, axis=1).view(U32)
    assert at == N and got.shape == want.shape and np.array_equal(got, want)


def bad_keywords(rows):
    """keyword sets the BODY session refuses (its own checks and `step_pieces`), for a call that runs `rows` > 0 code rows"""
    from talkshow_amd import _lib
    return [dict(mode=_lib.TS_SAMPLE_UNIFORMS),                                             # no uniforms
            dict(mode=_lib.TS_SAMPLE_PHILOX, sampling={"bogus": 1.0}),                      # an unknown key in a record
            dict(mode=_lib.TS_SAMPLE_GREEDY, sampling=(0.7, 0.9, 0)),                       # controls under the greedy mode
            dict(mode=_lib.TS_SAMPLE_PHILOX, style=np.ones(3, F32)),                        # a style row of the wrong width
            dict(mode=_lib.TS_SAMPLE_PHILOX, given=[np.zeros((1, 2), np.int64)]),           # a list with one entry for two clips
            dict(mode=_lib.TS_SAMPLE_PHILOX, given=np.full((2, 1, 2), 1 << 20, np.int64)),  # a code outside the codebook
            dict(mode=_lib.TS_SAMPLE_PHILOX, logprobs=torch.empty((2, rows, 2)))]           # an output tensor: a wav call returns its own


@pytest.mark.parametrize("seamless", [True, False], ids=["seamless", "plain"])
def test_a_refused_keyword_moves_no_counter_and_loses_no_row(full, seamless):
    """Every keyword the body session would refuse is refused BEFORE the front end is given a sample: the five counters stand still at every
    push and at the flush (where the front end still holds rows), and the session, carried on, returns what a session never refused returns."""
    w, wav, sizes = full["w"], full["wav"], [30000, 20000, 15000]
    common = dict(wav_sr=16000, wav_db=full["peak"], max_samples=max(sizes))
    st = w.open_stream(full["ids"], 2, 48, seamless=seamless, **common)
    twin = w.open_stream(full["ids"], 2, 48, seamless=seamless, **common)

    def state():
        chain = (st.body.frames_in, st.body.code_rows) if seamless else (st.body.pix.rows, st.body.frames)
        return (st.samples_in, st.frames_in, st.frames) + chain

    tried, at = 0, 0
    for n in sizes + [None]:
        flush = n is None
        chunk = None if flush else wav[:, at:at + n]
        _, rows, _ = st.plan_wav(0 if flush else n, flush=flush)
        s0 = state()
        if rows:
            for kw in bad_keywords(rows):
                with pytest.raises(ValueError):
                    st.flush(**kw) if flush else st.push_wav(chunk, **kw)
                assert state() == s0, kw
                tried += 1
            with pytest.raises(TypeError):
                st.flush(tempo=2) if flush else st.push_wav(chunk, tempo=2)
            assert state() == s0
        got = st.flush(**draw("philox")) if flush else st.push_wav(chunk, **draw("philox"))
        want = twin.flush(**draw("philox")) if flush else twin.push_wav(chunk, **draw("philox"))
        assert np.array_equal(bits(got), bits(want)), f"after {at} samples"
        at += n or 0
    assert tried >= 14 and st.frames == twin.frames == 120
    st.close(), twin.close()


def test_given_rows_at_a_flush_whose_push_runs_no_code_row(full):
    """65 000 samples: 121 MFCC rows are out before the flush, whose front end adds one.  The flush's body push then runs NO code row (the
    encoder holds 7 back) and its body flush runs the last 7: a valid `given` block goes to that call alone, and the result equals a
    seamless session fed the one-shot MFCC rows in the same blocks with the same `given` at its flush."""
    w, wav, mf = full["w"], full["wav"], full["mf"]
    st = w.open_stream(full["ids"], 2, 48, seamless=True, wav_sr=16000, wav_db=full["peak"], max_samples=40000)
    twin = w.open_stream(full["ids"], 2, 128, seamless=True)
    a = st.push_wav(wav[:, :40000], return_codes=True, **draw("philox"))
    b = st.push_wav(wav[:, 40000:], return_codes=True, **draw("philox"))
    assert st.frames_in == 121 and st.body.plan_calls(1, flush=True)[0][0] == 0
    f, rows, frames = st.plan_wav(0, flush=True)
    assert (f, rows) == (1, 7)
    given = torch.from_numpy(np.random.default_rng(4).integers(0, 2048, (2, 3, 2))).cuda()
    got = st.flush(return_codes=True, given=given, **draw("philox"))
    assert tuple(got[0].shape) == (2, frames, 129) and torch.equal(got[1][:, :3], given) and st.frames == 120
    t0 = int(a[0].shape[1]) + int(b[0].shape[1])
    ta = twin.push(mf[:, :121].contiguous(), return_codes=True, **draw("philox"))
    tb = twin.push(mf[:, 121:].contiguous(), return_codes=True, **draw("philox"))
    tc = twin.flush(return_codes=True, given=given, **draw("philox"))
    assert int(ta[0].shape[1]) + int(tb[0].shape[1]) == t0 and tuple(tb[1].shape) == (2, 0, 2)
    assert np.array_equal(bits(got[0]), bits(torch.cat([tb[0], tc[0]], dim=1))) and torch.equal(got[1], tc[1])
    st.close(), twin.close()
