"""Host front-end (numpy restatement of torchaudio Resample + MFCC).  torchaudio itself is not installed anywhere we can
run, so the restatement is pinned stage by stage against the INSTALLED third-party implementations of the same
definitions: the STFT / power stage against `torch.stft` (the function torchaudio.transforms.Spectrogram calls), the
HTK mel filterbank and the dB / top_db stage against `transformers.audio_utils` (HF's port of the torchaudio / librosa
definitions), the DCT-II table against `scipy.fft.dct`, and the whole MFCC against a pipeline assembled from those
pieces.  The two resamplers have no installed counterpart (UNPINNED against torchaudio / resampy themselves): their
indexing, phases, padding and length rules are checked against the continuous-time formulas they implement, evaluated
directly in float64, and on closed-form signals."""
import math
import os

import numpy as np
import pytest

from talkshow_amd import frontend as fe

REF_AUDIO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio")   # the reference's demo recordings


def _mfcc_f64(wave, sr, n_fft=2048, hop=734, n_mels=256, n_mfcc=64):
    x = np.pad(wave.astype(np.float64), (n_fft // 2, n_fft // 2), mode="reflect")
    T = 1 + (len(x) - n_fft) // hop
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]
    E = np.exp(-2j * np.pi * k / n_fft)                                   # explicit DFT matrix (no FFT library)
    P = np.stack([np.abs(E @ (x[t * hop:t * hop + n_fft] * w)) ** 2 for t in range(T)])
    fb = fe.melscale_fbanks(n_fft // 2 + 1, 0.0, sr // 2, n_mels, sr).astype(np.float64)
    db = 10 * np.log10(np.maximum(P @ fb, 1e-10))
    db = np.maximum(db, db.max() - 80.0)
    return (db @ fe.create_dct(n_mfcc, n_mels).astype(np.float64)).T


def test_mfcc_against_float64_dft():
    rng = np.random.default_rng(0)
    sr = 22000
    t = np.arange(6000) / sr
    wave = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
    got = fe.mfcc(wave, sr)
    ref = _mfcc_f64(wave, sr)
    assert got.shape == ref.shape == (64, 6000 // 734 + 1)
    np.testing.assert_allclose(got, ref, atol=2e-2, rtol=1e-4)          # coefficients are O(100); fp32 pipeline


def test_dct_and_filterbank_properties():
    d = fe.create_dct(64, 256).astype(np.float64)
    np.testing.assert_allclose(d.T @ d, np.eye(64), atol=1e-6)           # orthonormal DCT-II rows
    fb = fe.melscale_fbanks(1025, 0.0, 11000.0, 256, 22000)
    assert fb.shape == (1025, 256) and fb.min() >= 0 and fb.max() <= 1.0 + 1e-6
    peaks = fb.argmax(0)
    assert np.all(np.diff(peaks) >= 0)                                   # centre frequencies increase


def test_resample_preserves_a_tone_and_length():
    sr0, sr1 = 16000, 22000
    t = np.arange(16000) / sr0
    x = np.sin(2 * np.pi * 1000 * t).astype(np.float32)[None]
    y = fe.resample_sinc_hann(x, sr0, sr1)
    assert y.shape == (1, math.ceil(22000 * 16000 / 16000))
    t1 = np.arange(y.shape[1]) / sr1
    ref = np.sin(2 * np.pi * 1000 * t1)
    np.testing.assert_allclose(y[0, 200:-200], ref[200:-200], atol=2e-3)  # band-limited interpolation of an in-band tone
    assert fe.resample_sinc_hann(x, 16000, 16000) is x


def test_length_rule_matches_survey():
    # T = floor(N_22k / 734) + 1
    for n in (734 * 3, 220000, 12345):
        assert fe.mfcc(np.zeros(n, np.float32) + 1e-3, 22000).shape[1] == n // 734 + 1


def test_reference_demo_wavs_give_the_documented_frame_counts():
    # style.wav is 22 kHz stereo, exactly 10.0 s -> 300 frames (+1); 1st-page.wav 16 kHz, 12.816 s -> 385
    f = fe.get_mfcc_ta(os.path.join(REF_AUDIO, "style.wav"), sr=22000, fps=30)
    assert f.shape == (301, 64) or f.shape == (300, 64)
    f2 = fe.get_mfcc_ta(os.path.join(REF_AUDIO, "1st-page.wav"), sr=22000, fps=30)
    assert f2.shape[1] == 64 and abs(f2.shape[0] - 385) <= 1
    feat, gap = fe.get_mfcc_sepa(os.path.join(REF_AUDIO, "style.wav"), sr=22000, fps=30)
    assert gap == 44000 // 734 + 1 and feat.shape[1] == 64
    w = fe.get_wav16(os.path.join(REF_AUDIO, "1st-page.wav"))
    assert w.ndim == 2 and w.shape[1] == 1 and np.abs(w).max() <= 1.0


# ---- pins against installed third-party implementations -----------------------------------------------------------------
def _wave(n=22000 * 3, sr=22000, seed=1):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return (0.25 * np.sin(2 * np.pi * 330 * t) * (1 + 0.4 * np.sin(2 * np.pi * 2 * t)) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def _torch_stft_power(x, n_fft=2048, hop=734):
    import torch
    spec = torch.stft(torch.from_numpy(x), n_fft=n_fft, hop_length=hop, win_length=n_fft,
                      window=torch.hann_window(n_fft, periodic=True), center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)                      # torchaudio.functional.spectrogram's call
    return spec.abs().pow(2.0).T.numpy()                                        # (T, n_fft//2+1)


@pytest.mark.parametrize("hop", [734, 1467])
def test_stft_power_stage_pinned_to_torch_stft(hop):
    x = _wave()
    got = fe.power_spectrogram(x, 2048, hop)
    ref = _torch_stft_power(x, 2048, hop)
    assert got.shape == ref.shape == (len(x) // hop + 1, 1025)
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4 * float(ref.max()) * 1e-3)


def test_mel_db_dct_tables_pinned_to_transformers_and_scipy():
    from scipy.fft import dct
    from transformers import audio_utils as au
    fb = fe.melscale_fbanks(1025, 0.0, 11000.0, 256, 22000)
    hf = au.mel_filter_bank(num_frequency_bins=1025, num_mel_filters=256, min_frequency=0.0, max_frequency=11000.0,
                            sampling_rate=22000, norm=None, mel_scale="htk")
    np.testing.assert_allclose(fb, hf, atol=1e-6, rtol=0)
    d = fe.create_dct(64, 256)
    np.testing.assert_allclose(d, dct(np.eye(256), type=2, norm="ortho", axis=0)[:64].T, atol=1e-6, rtol=0)


def test_whole_mfcc_against_third_party_pipeline():
    """torch.stft -> HF mel_filter_bank -> HF power_to_db(db_range=80) -> scipy DCT-II ortho, vs frontend.mfcc."""
    from scipy.fft import dct
    from transformers import audio_utils as au
    x = _wave(22000 * 4, seed=2)
    power = _torch_stft_power(x).astype(np.float64)
    mel = power @ au.mel_filter_bank(1025, 256, 0.0, 11000.0, 22000, None, "htk")
    db = au.power_to_db(mel, reference=1.0, min_value=1e-10, db_range=80.0)
    ref = dct(db, type=2, norm="ortho", axis=1)[:, :64].T
    got = fe.mfcc(x, 22000)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, atol=2e-2, rtol=1e-4)               # O(10..1000) coefficients, fp32 pipeline


def test_mel_and_mel_mul_feature_types_pinned(tmp_path):
    """`get_mfcc_ta(type='mel' | 'mel_mul')` (`data_utils/utils.py:178-191`: torchaudio MelSpectrogram; per-frame 1 s chunks, a 50 ms
    window inside 2048-point frames, 10 ms hop, log) against the same pipelines assembled from installed third-party pieces:
    torch.stft (what torchaudio's Spectrogram calls, incl. its centred short window) and transformers' HTK mel filter bank; the
    chunking against the reference's own slicing rule written out."""
    import torch
    from scipy.io import wavfile
    from transformers import audio_utils as au
    sr = 22000
    x = _wave(sr * 2 + 311, sr, seed=4)
    path = str(tmp_path / "clip.wav")
    wavfile.write(path, sr, x)
    fb = au.mel_filter_bank(1025, 256, 0.0, float(sr // 2), sr, None, "htk")
    mel = fe.get_mfcc_ta(path, sr=sr, fps=30, type="mel")
    ref = _torch_stft_power(x, 2048, 734).astype(np.float64) @ fb
    assert mel.shape == ref.shape == (len(x) // 734 + 1, 256)
    np.testing.assert_allclose(mel, ref, rtol=2e-4, atol=2e-7 * float(ref.max()))
    mm = fe.get_mfcc_ta(path, sr=sr, fps=30, type="mel_mul")
    y = torch.from_numpy(np.float32(0.01) * x / np.mean(np.abs(x), dtype=np.float32))
    spf, pad = sr // 30, (sr - sr // 30) // 2
    yp = torch.nn.functional.pad(y[None], (pad, pad))[0]
    chunks = torch.stack([yp[i - sr // 2:i + sr // 2] for i in range(sr // 2, yp.shape[0] - sr // 2, spf)])
    spec = torch.stft(chunks, n_fft=2048, hop_length=sr // 100, win_length=sr // 20, window=torch.hann_window(sr // 20, periodic=True),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    refm = np.log(np.maximum(np.einsum("cft,fm->cmt", spec.abs().pow(2.0).numpy().astype(np.float64), fb), 1e-10))
    assert mm.shape == refm.shape == (chunks.shape[0], 256, sr // (sr // 100) + 1)
    big = refm > np.log(1e-9)                                  # away from the clamp, where a log amplifies fp32 noise without bound
    np.testing.assert_allclose(mm[big], refm[big], atol=5e-3, rtol=0)
    with pytest.raises(NotImplementedError, match="unknown feature type"):
        fe.get_mfcc_ta(path, sr=sr, fps=30, type="chroma")


# ---- librosa.load(sr=16000)'s resampler for the face path (resampy 'kaiser_best'; UNPINNED: librosa is not installed) ------
def test_kaiser_best_table_against_closed_form():
    """The 32769-entry table == rolloff * sinc(rolloff t) * I0(beta sqrt(1 - (t/64)^2)) / I0(beta) evaluated directly."""
    from scipy.special import i0
    win, delta, num_table = fe.kaiser_best_table()
    assert win.shape == (64 * 512 + 1,) and num_table == 512
    t = np.arange(win.shape[0]) / 512.0
    rolloff, beta = 0.9475937167399596, 14.769656459379492
    ref = rolloff * np.sinc(rolloff * t) * i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / 64.0) ** 2))) / i0(beta)
    np.testing.assert_allclose(win, ref, atol=2e-7)
    np.testing.assert_allclose(delta[:-1], np.diff(win), atol=0)
    assert delta[-1] == 0 and abs(win[0] - rolloff) < 1e-7


def test_kaiser_best_resampling_properties():
    x = np.sin(2 * np.pi * 1000 * np.arange(8000) / 8000.0).astype(np.float32)
    y = fe.resample_kaiser_best(x, 8000, 16000)                       # interpolation: unit-gain filter, exact to ~1e-7
    assert y.shape == (16000,) and y.dtype == np.float32
    np.testing.assert_allclose(y[300:-300], np.sin(2 * np.pi * 1000 * np.arange(16000) / 16000.0)[300:-300], atol=1e-6)
    assert fe.resample_kaiser_best(x, 16000, 16000) is not None and np.array_equal(fe.resample_kaiser_best(x, 16000, 16000), x)
    # decimation 22.05 kHz -> 16 kHz: length rule ceil(N * ratio) with the last sample zero-filled by fix_length, in-band
    # tone preserved up to the algorithm's own gain error (index_step = int(scale * 512) truncates: 371 instead of 371.5)
    n = 22050 + 7
    z = fe.resample_kaiser_best(np.sin(2 * np.pi * 440 * np.arange(n) / 22050.0).astype(np.float32), 22050, 16000)
    assert z.shape == (int(np.ceil(n * 16000 / 22050)),)
    ref = np.sin(2 * np.pi * 440 * np.arange(z.shape[0]) / 16000.0)
    assert np.abs(z[400:-400] - ref[400:-400]).max() < 3e-3
    # an out-of-band tone (9 kHz > 8 kHz Nyquist of the target) is removed
    hi = fe.resample_kaiser_best(np.sin(2 * np.pi * 9000 * np.arange(22050) / 22050.0).astype(np.float32), 22050, 16000)
    assert np.abs(hi[400:-400]).max() < 2e-2


def test_get_wav16_resamples_other_rates(tmp_path):
    from scipy.io import wavfile
    sr = 22050
    t = np.arange(sr) / sr
    stereo = np.stack([np.sin(2 * np.pi * 300 * t), 0.5 * np.sin(2 * np.pi * 300 * t)], 1)
    p = str(tmp_path / "a.wav")
    wavfile.write(p, sr, (stereo * 20000).astype(np.int16))
    w = fe.get_wav16(p, host=True)
    assert w.shape == (16000, 1) and w.dtype == np.float32
    ref = 0.75 * (20000 / 32768.0) * np.sin(2 * np.pi * 300 * np.arange(16000) / 16000.0)
    assert np.abs(w[400:-400, 0] - ref[400:-400]).max() < 2e-3


def test_get_mfcc_ta_encoder_choice_switch(tmp_path):
    """`get_mfcc_ta(am=<processor>, encoder_choice=...)` (`data_utils/utils.py:193-202`): 'faceformer' -> the raw 16 kHz samples
    (N, 1), 'meshtalk' -> samples scaled to mean |x| = 0.01, 'onset' -> onset times (K, 1), any other
    value -> the MFCC features exactly as without `am`; without `am` the argument has no effect, as in the reference."""
    from scipy.io import wavfile
    x = (0.2 * np.sin(2 * np.pi * 250 * np.arange(16000) / 16000.0)).astype(np.float32)
    p = str(tmp_path / "b.wav")
    wavfile.write(p, 16000, x)
    am = object()
    w = fe.get_mfcc_ta(p, sr=16000, fps=30, am=am, encoder_choice='faceformer', host=True)
    assert w.shape == (16000, 1) and np.array_equal(w[:, 0], x)
    m = fe.get_mfcc_ta(p, sr=16000, fps=30, am=am, encoder_choice='meshtalk', host=True)
    assert m.shape == (16000,) and abs(float(np.mean(np.abs(m))) - 0.01) < 1e-6
    on = fe.get_mfcc_ta(p, sr=16000, fps=30, am=am, encoder_choice='onset', host=True)
    assert on.ndim == 2 and on.shape[1] == 1                                          # onset times (s); test_onset_times_restatement
    base = fe.get_mfcc_ta(p, sr=22000, fps=30, host=True)
    assert base.shape[1] == 64
    for kw in (dict(am=am), dict(am=am, encoder_choice='mfcc'), dict(encoder_choice='faceformer')):
        assert np.array_equal(fe.get_mfcc_ta(p, sr=22000, fps=30, host=True, **kw), base)


@pytest.mark.parametrize("orig,new,n", [(16000, 22000, 1601), (22000, 16000, 2203), (48000, 16000, 4000), (8000, 22050, 333)])
def test_sinc_hann_resampler_against_its_continuous_definition(orig, new, n):
    """The polyphase / strided-window implementation (what torchaudio does, and what the device kernel mirrors) against the
    formula it implements, evaluated directly in float64 with no phases, padding or windows of samples:
        y[j] = sum_n x[n] * (f/orig) * sinc(t) * cos^2(pi t / (2 L)),  t = (n/orig - j/new) * f,  |t| < L = 6,
        f = 0.99 * min(orig, new)   (rates reduced by their gcd first).
    Pins the indexing (phase offsets, left padding, output length); the formula itself is the restated third-party part."""
    rng = np.random.default_rng(orig + new)
    x = rng.standard_normal(n).astype(np.float32)
    y = fe.resample_sinc_hann(x[None], orig, new)[0]
    g = math.gcd(orig, new)
    o, w, L = orig // g, new // g, 6
    f = min(o, w) * 0.99
    assert y.shape[0] == math.ceil(w * n / o)
    j = np.arange(y.shape[0], dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    t = (k / o - j / w) * f
    kern = np.where(np.abs(t) < L, np.sinc(t) * np.cos(np.pi * t / (2 * L)) ** 2, 0.0) * (f / o)
    want = kern @ x.astype(np.float64)
    np.testing.assert_allclose(y, want, atol=2e-5, rtol=0)


@pytest.mark.parametrize("orig,n", [(8000, 1500), (11025, 1700), (12000, 999)])
def test_kaiser_best_interpolation_against_its_continuous_definition(orig, n):
    """Up-sampling to 16 kHz (unit filter scale: no index_step truncation) against the band-limited interpolation formula
    evaluated directly in float64 from the CLOSED-FORM window, y[j] = sum_n x[n] h(|j/ratio - n|), |.| < 64 zero crossings:
    pins the table lookup, the linear interpolation between table entries, both wings and the edge limits."""
    from scipy.special import i0
    rng = np.random.default_rng(orig)
    x = rng.standard_normal(n).astype(np.float32)
    y = fe.resample_kaiser_best(x, orig, 16000)
    ratio = 16000.0 / orig
    n_out = int(n * ratio)
    rolloff, beta = 0.9475937167399596, 14.769656459379492
    t = np.abs(np.arange(n_out, dtype=np.float64)[:, None] / ratio - np.arange(n, dtype=np.float64)[None, :])
    h = np.where(t < 64.0, rolloff * np.sinc(rolloff * t) * i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / 64.0) ** 2))) / i0(beta), 0.0)
    want = h @ x.astype(np.float64)
    np.testing.assert_allclose(y[:n_out], want, atol=3e-5, rtol=0)
    assert y.shape[0] == math.ceil(n * ratio) and np.all(y[n_out:] == 0)       # librosa's fix_length zero-fills the tail


def test_onset_times_restatement(tmp_path):
    """`get_mfcc_ta(..., am=<processor>, encoder_choice='onset')` (`utils.py:200-201`, read by scripts/test_body.py:173): onset times in
    seconds, (K, 1).  librosa is absent here, so this runs the restatement of its published algorithm (PARITY UNPINNED, see the
    docstring of `frontend.onset_times`); what can be checked without the package: the Slaney filters integrate to one, the onset
    envelope is zero for a constant signal, every tone burst of a synthetic clip is found within two frames, silence gives no onset."""
    from scipy.io import wavfile
    from transformers import audio_utils as au
    w = fe.slaney_mel_filters(16000, 2048)
    assert w.shape == (128, 1025) and np.allclose(w.sum(1) * (16000 / 2048), 1.0, atol=2e-2) and (w >= 0).all()
    hf = au.mel_filter_bank(1025, 128, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney")      # HF's port of librosa.filters.mel: this stage IS pinned
    np.testing.assert_allclose(w.T, hf, atol=1e-7, rtol=0)
    assert fe.onset_times(np.zeros(16000, np.float32)).shape == (0,)
    rng = np.random.default_rng(3)
    beats = np.asarray([0.5, 1.2, 2.0, 2.9, 3.7, 4.4])
    tt = np.arange(4000) / 16000.0
    x = 0.001 * rng.standard_normal(5 * 16000)
    for j, b0 in enumerate(beats):
        x[int(b0 * 16000):int(b0 * 16000) + 4000] += 0.5 * np.sin(2 * np.pi * (300 + 60 * j) * tt) * np.exp(-12 * tt)
    p = str(tmp_path / "bursts.wav")
    wavfile.write(p, 16000, x.astype(np.float32))
    on = fe.get_mfcc_ta(p, fps=30, sr=16000, am="processor", encoder_choice="onset", host=True)
    assert on.ndim == 2 and on.shape[1] == 1 and on.dtype == np.float64
    assert np.abs(on[:, 0][None, :] - beats[:, None]).min(axis=1).max() < 0.08      # every burst, within two frames + a hop (32 ms each)
    assert (np.diff(on[:, 0]) > 0).all() and on.min() >= 0 and on.max() < 5.0
    env = fe.onset_strength(x.astype(np.float32), 16000)
    assert env.shape == (x.size // 512 + 1,) and (env >= 0).all() and env[:3].max() == 0.0
