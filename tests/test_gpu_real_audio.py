"""Parity on REAL audio: the reference's own demo recordings (demo_audio/{style,1st-page,french}.wav, the inputs of
`/root/reference/scripts/demo.py:158-247`) against values the REFERENCE's modules produced on them.

Every other reference-made golden uses iid N(0, 20^2) feature rows / 0.1 N(0,1) white noise.  On speech the MFCC rows reach
470 .. 660 and are strongly correlated in time, the waveform is far from white (the face's conv0 GroupNorm statistics come from
its second moments, csrc/face.hip), and greedy near-ties are not governed by the synthetic margin statistics.  The goldens
(tests/golden/make_golden.py `real_audio_body` / `real_audio_face`):

* body — INPUT: the float64 twin's MFCC rows of each recording (the third-party front-end's pin stays separate), OUTPUT of the
  reference `AudioEncoder` -> greedy harness around `GatedPixelCNN.forward` -> both `VQVAE.decode`
  (`nets/smplx_body_pixel.py:272-285`, `nets/spg/gated_pixelcnn_v2.py:130-150`) under all four speaker ids: 1 944 decisions;
* face — INPUT: the 16 kHz samples (native for 1st-page.wav: no third-party step at all; the host kaiser_best twin for the other
  two), OUTPUT of the reference wrapper's `generate` (zero id) / `generator(...)` (one-hot id) and the wav2vec2 hidden state
  (`nets/smplx_face.py:221-238`, `nets/spg/wav2vec.py:76-143`).

Asserted: codes EQUAL, poses / face rows / hidden state within 1e-4, audio-encoder output within 2x its measured error; the same
from the .wav files through the device front-end; the face with `TS_W2V_MOMENTS=1` (default) and `=0` (child process).
`__graft_entry__.smoke()` prints the same counts into the driver's record.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from talkshow_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO = os.path.join(REPO, "tests", "golden", "audio")
RECS = ("style.wav", "1st-page.wav", "french.wav")
NEAR_TIE_LOGIT = 1e-3


def _tag(name):
    return name[:-4].replace("-", "_")


def _need_recording(name):
    p = os.path.join(AUDIO, name)
    assert os.path.exists(p), f"{p}: the committed recording is missing"
    return p


def _body_wrapper(tmp_path):
    from nets.init_model import init_model
    from talkshow_amd.config import Object
    vq_path = str(tmp_path / "vq.pth")
    torch.save({"generator": {"g_body": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=39)),
                              "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))}}, vq_path)
    cfg = json.load(open(os.path.join(REPO, "config", "body_pixel.json")))
    cfg["Model"]["vq_path"] = vq_path
    w = init_model("s2g_body_pixel", argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                       "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))})
    return w


def count_equal(got, ref, margin):
    """Autoregressive counting rule of tests/test_gpu_operating_points.py: a clip counts up to its first difference."""
    equal, report = 0, []
    for b in range(ref.shape[0]):
        d = np.flatnonzero((got[b] != ref[b]).reshape(-1))
        if d.size == 0:
            equal += ref[b].size
            continue
        equal += int(d[0])
        m = float(margin[b].reshape(-1)[d[0]])
        report.append(f"clip {b}: first difference at position {int(d[0])}, reference top-2 margin {m:.2e}"
                      f" ({'near-tie' if m < NEAR_TIE_LOGIT else 'NOT a near-tie'})")
    return equal, report


@pytest.mark.parametrize("name", RECS)
def test_body_on_recordings_from_stored_rows(golden, tmp_path, name):
    """Stored twin-MFCC rows -> device audio encoder -> greedy chain -> VQ decoders, against the reference's values on the same
    rows: under all four speaker ids (B = 4) and as clips 100..103 of a 256-clip pass (the wide kernel) beside synthetic clips."""
    from talkshow_amd import _lib
    g, t = golden("real_audio_body"), _tag(name)
    rows, ref, margin = g[t + "_rows"], g[t + "_codes"].astype(np.int64), g[t + "_margin"]
    T, spk = rows.shape[0], int(g[t + "_pose_id"])
    w = _body_wrapper(tmp_path)
    feat = w.audioencoder.forward_nlc(torch.from_numpy(rows[None]).cuda()).cpu().numpy()[0]
    # measured 4.1e-6 / 4.6e-6 / 5.4e-6 (profiles/r06_notes/real_audio_measured.jsonl; |out| up to 6, rows up to 663): bound = 2x the largest
    assert_close_measured(f"real_audio.{t}.aud_feat", feat, g[t + "_aud_feat"], 1.1e-5)
    mf, ids = np.repeat(rows[None], 4, 0), np.arange(4, dtype=np.int64)
    c4, p4 = w.generate_batch(mf, ids, mode=_lib.TS_SAMPLE_GREEDY)
    c4, p4 = c4.cpu().numpy(), p4.cpu().numpy()
    equal, report = count_equal(c4, ref, margin)
    print(f"\nreal_audio_body {name}: greedy codes equal to the reference {equal} / {ref.size} "
          f"(reference margins: min {margin.min():.2e}, {int((margin < NEAR_TIE_LOGIT).sum())} under {NEAR_TIE_LOGIT})")
    assert equal == ref.size, f"{name}: greedy codes equal to the reference {equal} / {ref.size}: " + "; ".join(report)
    assert_close_measured(f"real_audio.{t}.poses", p4[spk], g[t + "_poses"], 1e-4)
    big, big_ids = synth.mfcc_features(3000 + T, 256, T), synth.speaker_ids(256)
    big[100:104], big_ids[100:104] = mf, ids
    c256, p256 = w.generate_batch(big, big_ids, mode=_lib.TS_SAMPLE_GREEDY)
    np.testing.assert_array_equal(c256.cpu().numpy()[100:104], c4)        # == the reference, inside the bench's pass shape
    np.testing.assert_array_equal(p256.cpu().numpy()[100:104], p4)


@pytest.mark.parametrize("name", RECS)
def test_body_on_recordings_wav_in(golden, tmp_path, name):
    """The .wav file through the DEVICE front-end (stereo -> mono, 22 k / 16 k / 24 k -> 22 kHz, fp32 FFT MFCC) and the wrapper's
    `infer_on_audio`, against the reference's values on the float64 twin's rows: 0 codes differ, poses within 1e-4."""
    from talkshow_amd import _lib
    from talkshow_amd import frontend as fe
    p = _need_recording(name)
    g, t = golden("real_audio_body"), _tag(name)
    ref, margin, spk = g[t + "_codes"].astype(np.int64), g[t + "_margin"], int(g[t + "_pose_id"])
    w = _body_wrapper(tmp_path)
    dev_rows = fe.get_mfcc_ta(p, sr=22000, fps=30, smlpx=True, type="mfcc")
    assert dev_rows.shape == g[t + "_rows"].shape
    err = float(np.abs(dev_rows - g[t + "_rows"]).max())
    print(f"\n{name}: device MFCC rows vs the stored float64-twin rows: max |err| {err:.2e} (coefficients up to {np.abs(dev_rows).max():.0f})")
    assert err <= 2e-3
    c4, _ = w.generate_batch(np.repeat(dev_rows[None], 4, 0), np.arange(4, dtype=np.int64), mode=_lib.TS_SAMPLE_GREEDY)
    equal, report = count_equal(c4.cpu().numpy(), ref, margin)
    print(f"real_audio_body {name} wav-in: greedy codes equal to the reference {equal} / {ref.size}")
    assert equal == ref.size, f"{name} wav-in: {equal} / {ref.size}: " + "; ".join(report)
    poses = w.infer_on_audio(p, id=torch.tensor([spk]).cuda(), fps=30, greedy=True)       # the call demo.py makes (+ greedy)
    assert poses.shape == (1,) + g[t + "_poses"].shape
    assert_close_measured(f"real_audio.{t}.poses_wav_in", poses[0], g[t + "_poses"], 1e-4)


def test_body_on_a_recording_second_weight_set(golden, tmp_path):
    """french.wav's stored rows under a SECOND set of synthetic weights (seed 11: other logits, other near-ties) and all four speaker ids,
    against what the reference's modules produced with those weights (`real_audio_body_w11`): 576 / 576 codes equal, poses within 1e-4."""
    from nets.init_model import init_model
    from talkshow_amd import _lib
    from talkshow_amd.config import Object
    g, gw = golden("real_audio_body"), golden("real_audio_body_w11")
    seed = int(gw["weight_seed"])
    vq_path = str(tmp_path / "vq.pth")
    torch.save({"generator": {"g_body": synth.to_torch(synth.vqvae_state_dict(seed=seed, in_dim=39)),
                              "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=seed, in_dim=90, salt=1))}}, vq_path)
    cfg = json.load(open(os.path.join(REPO, "config", "body_pixel.json")))
    cfg["Model"]["vq_path"] = vq_path
    w = init_model("s2g_body_pixel", argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=seed)),
                       "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=seed))})
    rows, ref, margin = g["french_rows"], gw["codes"].astype(np.int64), gw["margin"]
    c4, p4 = w.generate_batch(np.repeat(rows[None], 4, 0), np.arange(4, dtype=np.int64), mode=_lib.TS_SAMPLE_GREEDY)
    equal, report = count_equal(c4.cpu().numpy(), ref, margin)
    print(f"\nreal_audio_body_w11 french.wav (weights seed {seed}): greedy codes equal to the reference {equal} / {ref.size} "
          f"(reference margins: min {margin.min():.2e}, {int((margin < NEAR_TIE_LOGIT).sum())} under {NEAR_TIE_LOGIT})")
    assert equal == ref.size, f"{equal} / {ref.size}: " + "; ".join(report)
    assert_close_measured("real_audio.french.poses_w11", p4.cpu().numpy()[1], gw["poses_id1"], 1e-4)


def test_stochastic_decode_on_a_recording_vs_oracle(golden):
    """configs[3] on real speech: the reference's audio-encoder output for french.wav (golden) -> device PixelCNN decode with INJECTED
    uniforms and with the device Philox stream, against the oracle's full-grid `pixelcnn_generate(uniforms=...)` (the reference's
    `generate`, `gated_pixelcnn_v2.py:152-177`, with an inverse-CDF draw): all 144 draws equal, and they are draws (they differ from greedy)."""
    from oracle import talkshow_oracle as O
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("real_audio_body")
    aud = g["french_aud_feat"][None]                                              # (1, 72, 256): reference AudioEncoder on the recording's rows
    H = aud.shape[1]
    sd = synth.pixelcnn_state_dict(seed=7)
    m = GatedPixelCNN(2048, 256, 15, 4, True, True).cuda()
    m.load_state_dict(synth.to_torch(sd))
    label = np.asarray([3], np.int64)
    u = O.philox_uniforms(2024, 7, 1, H)
    got_u, _ = m.run(label, aud, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u)
    got_p, _ = m.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=2024, clip_index0=7)
    np.testing.assert_array_equal(got_p.cpu().numpy(), got_u.cpu().numpy())       # device Philox == oracle Philox
    ref = O.pixelcnn_generate(label, np.repeat(aud.transpose(0, 2, 1)[:, :, :, None], 2, axis=3), sd, 15, H, uniforms=u)
    diff = int((got_u.cpu().numpy() != ref).sum())
    print(f"\nstochastic decode on french.wav: draws equal to the oracle {ref.size - diff} / {ref.size}")
    assert diff == 0
    assert not np.array_equal(ref[0], g["french_codes"][3].astype(np.int64))


def _wav16(name, g):
    """The face golden's input: the 16 kHz samples whose sha256 the golden stores.  A side file written by
    tests/golden/audio/fetch_reference_audio.py where present, else regenerated here by the host twin from the committed recording;
    anything that does not hash to the golden's input is not used."""
    t = _tag(name)
    want = str(g[t + "_wav16_sha256"])
    side = os.path.join(AUDIO, name + ".wav16.npy")
    if os.path.exists(side):
        wav = np.load(side)
        if hashlib.sha256(wav.tobytes()).hexdigest() == want:
            return wav
    from talkshow_amd import frontend as fe
    wav = fe.get_wav16(_need_recording(name), host=True)[:, 0]
    if hashlib.sha256(wav.tobytes()).hexdigest() != want:
        pytest.skip(f"{name}: the host resampler on this machine does not reproduce the golden's input bit for bit and "
                    f"{side} is absent")
    return wav


@pytest.mark.parametrize("name", RECS)
def test_face_on_recordings(golden, name):
    """16 kHz samples of the recording -> device wav2vec2 + heads (`ts_face_generate`) against the reference wrapper's output on
    the same samples: zero id (`generate`), one-hot id, the hidden state at every 6th frame; alone, and as clip 5 of a batch of 8
    beside white-noise clips (the GroupNorm moments are per clip)."""
    from talkshow_amd.modules import FaceGenerator
    g, t = golden("real_audio_face"), _tag(name)
    wav = _wav16(name, g)
    N, frame, spk = (int(v) for v in g[t + "_n"])
    assert wav.shape == (N,)
    m = FaceGenerator().cuda()
    m.load_state_dict(synth.to_torch(synth.face_state_dict(seed=7)))
    zero, hot = np.zeros((1, 4), np.float32), np.eye(4, dtype=np.float32)[[spk]]
    out0, hid = m.run(wav[None], zero, frame, want_hidden=True)
    assert_close_measured(f"real_audio.{t}.face_hidden", hid.cpu().numpy()[0, ::6], g[t + "_hidden_6"], 1e-4)
    assert_close_measured(f"real_audio.{t}.face_zero_id", out0.cpu().numpy()[0], g[t + "_out_zero_id"], 1e-4)
    assert_close_measured(f"real_audio.{t}.face_one_hot", m.run(wav[None], hot, frame).cpu().numpy()[0], g[t + "_out_one_hot"], 1e-4)
    batch = synth.wav16(4000 + N, 8, N)
    batch[5] = wav
    ids = np.zeros((8, 4), np.float32)
    ids[5] = hot[0]
    assert_close_measured(f"real_audio.{t}.face_in_batch", m.run(batch, ids, frame).cpu().numpy()[5], g[t + "_out_one_hot"], 1e-4)


def test_face_recording_inside_batch_64(golden):
    """style.wav (exactly 10 s: 160 000 samples at 16 kHz) as clips 7 and 40 of a BASELINE configs[2] batch of 64 beside white-noise
    clips — the shape at which the transformer GEMMs run their production plans (M = 19 200 rows: the ring engine's stream-K band on
    FFN2, bands on FFN1, ...) — against the reference's output on the recording: zero id and one-hot id, 1e-4."""
    from talkshow_amd.modules import FaceGenerator
    g = golden("real_audio_face")
    wav = _wav16("style.wav", g)
    N, frame, spk = (int(v) for v in g["style_n"])
    assert N == 160000 and frame == 300
    m = FaceGenerator().cuda()
    m.load_state_dict(synth.to_torch(synth.face_state_dict(seed=7)))
    batch = synth.wav16(4100, 64, N)
    ids = np.eye(4, dtype=np.float32)[np.arange(64) % 4]
    batch[7], batch[40] = wav, wav
    ids[7] = 0.0
    ids[40] = np.eye(4, dtype=np.float32)[spk]
    out = m.run(batch, ids, frame).cpu().numpy()
    assert_close_measured("real_audio.style.face_zero_id_in_batch_64", out[7], g["style_out_zero_id"], 1e-4)
    assert_close_measured("real_audio.style.face_one_hot_in_batch_64", out[40], g["style_out_one_hot"], 1e-4)


def test_face_on_recordings_conv0_convolution_pass():
    """The same test with conv0's GroupNorm statistics taken from a convolution pass instead of the waveform's second moments
    (`TS_W2V_MOMENTS=0`; knobs are read once per process -> child process)."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_face_on_recordings and not conv0"],
                       env=dict(os.environ, TS_W2V_MOMENTS="0"), capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("name", RECS)
def test_face_on_recordings_wav_in(golden, name):
    """The .wav file through the face wrapper's `infer_on_audio` (device kaiser_best resampler where the file is not 16 kHz) against
    the reference's output on the host twin's samples.  1st-page.wav is native 16 kHz: nothing but `int16 / 32768` sits between the
    file and the generator on either side, and the bar is the contract's 1e-4.  For the other two the device resampler (fp32) differs
    from the host twin (float64 accumulation) in the last bits of the samples; the bar stays 1e-4 on the output."""
    import nets
    from talkshow_amd.config import Object
    p = _need_recording(name)
    g, t = golden("real_audio_face"), _tag(name)
    N, frame, spk = (int(v) for v in g[t + "_n"])
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    w = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    out = w.infer_on_audio(p)                                                  # id=None -> the all-zero identity vector
    assert out.shape == (1, frame, 103)
    assert_close_measured(f"real_audio.{t}.face_wav_in_zero_id", out[0], g[t + "_out_zero_id"], 1e-4)
    hot = w.infer_on_audio(p, id=torch.tensor([spk]))
    assert_close_measured(f"real_audio.{t}.face_wav_in_one_hot", hot[0], g[t + "_out_one_hot"], 1e-4)
