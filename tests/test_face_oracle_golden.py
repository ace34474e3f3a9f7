"""Pin the face oracle (oracle/face_oracle.py) to goldens produced by the reference `s2g_face` wrapper running over the
installed transformers wav2vec2 module (tests/golden/make_golden.py, case `face_full`).  CPU only."""
import numpy as np

from oracle import face_oracle as FO
from talkshow_amd import synth


def test_face_generator_matches_reference(golden):
    g = golden("face_full")
    sd = synth.face_state_dict(seed=7)
    frame = g["out"].shape[1]
    hs, inter = FO.wav2vec2_forward(g["wav"], sd, frame, return_intermediates=True)
    np.testing.assert_allclose(hs, g["hidden"], atol=5e-5, rtol=0)
    out = FO.face_generator(g["wav"], g["ids"], sd, frame)
    assert out.shape == g["out"].shape == (2, 60, 103)
    np.testing.assert_allclose(out, g["out"], atol=1e-4, rtol=0)
    # smplx_face.TrainWrapper.generate uses the all-zero id vector (smplx_face.py:232-233)
    out0 = FO.face_generator(g["wav"], np.zeros_like(g["ids"]), sd, frame)
    np.testing.assert_allclose(out0, g["generate_zero_id"], atol=1e-4, rtol=0)
    assert np.abs(out0[1] - out[1]).max() > 1e-3          # the one-hot id of clip 1 matters


def test_legacy_weight_norm_keys_are_equivalent():
    a = synth.face_state_dict(seed=3, n_layers=1)
    b = synth.face_state_dict(seed=3, n_layers=1, legacy_weight_norm_keys=True)
    p = "audio_encoder.encoder.pos_conv_embed.conv"
    np.testing.assert_array_equal(FO.pos_conv_weight(a, p), FO.pos_conv_weight(b, p))


def test_linear_interpolation_endpoints():
    x = np.arange(499, dtype=np.float32)[None, :, None]
    y = FO.linear_interpolation(x, 300)[0, :, 0]
    assert y.shape == (300,) and abs(y[0] - 0.3316667) < 1e-4 and y[-1] <= 498 and np.all(np.diff(y) > 0)


def test_face_generator_on_a_recording(golden):
    """Real speech (tests/golden/real_audio_face.npz: the reference wrapper on its own demo recordings): french.wav, 9.6 s at
    16 kHz as the host kaiser_best twin produces it from the committed recording (tests/golden/audio/french.wav); the samples
    must hash to the golden's input."""
    import hashlib
    import os
    from talkshow_amd import frontend as fe
    g = golden("real_audio_face")
    wav = fe.get_wav16(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio", "french.wav"), host=True)[:, 0]
    assert hashlib.sha256(wav.tobytes()).hexdigest() == str(g["french_wav16_sha256"]), "the host twin's samples are not the golden's input"
    N, frame, spk = (int(v) for v in g["french_n"])
    sd = synth.face_state_dict(seed=7)
    hs = FO.wav2vec2_forward(wav[None], sd, frame)
    np.testing.assert_allclose(hs[0, ::6], g["french_hidden_6"], atol=5e-5, rtol=0)
    ids = np.zeros((1, 4), np.float32)
    np.testing.assert_allclose(FO.face_generator(wav[None], ids, sd, frame)[0], g["french_out_zero_id"], atol=1e-4, rtol=0)
    ids[0, spk] = 1.0
    np.testing.assert_allclose(FO.face_generator(wav[None], ids, sd, frame)[0], g["french_out_one_hot"], atol=1e-4, rtol=0)


def test_lerp_source_index_matches_aten():
    """FO.source_index against this host's own F.interpolate(mode='linear', align_corners=False), read back from an input whose frame i
    holds i: ATen's AVX2 / AVX512 kernels round scale * (j + 0.5) - 0.5 once (fused=True: what made the reference's goldens, and what the
    HIP kernel computes), its scalar kernel rounds the product first (fused=False: the oracle's linear_interpolation).  At the frames where
    the two forms differ (they do for every length below), torch must sit on its form's side."""
    import torch
    import torch.nn.functional as F
    cap = torch.backends.cpu.get_cpu_capability()
    want = {"AVX2": True, "AVX512": True, "DEFAULT": False}.get(cap)
    for L, T in ((499, 300), (49, 30), (2999, 1800), (1499, 900)):
        got = F.interpolate(torch.arange(L, dtype=torch.float32).view(1, 1, L), size=T, mode="linear", align_corners=False)[0, 0]
        got = got.double().numpy()
        form = {}
        for fused in (False, True):
            i0, i1, l0, l1 = FO.source_index(L, T, fused)
            form[fused] = i0 * l0.astype(np.float64) + i1 * l1.astype(np.float64)
        diff = np.abs(form[True] - form[False])
        d = diff > 0
        assert d.any(), f"{L} -> {T}: the two index forms agree everywhere"
        near = {f: bool((np.abs(got[d] - form[f][d]) < diff[d] / 4).all()) for f in (False, True)}
        assert near[True] or near[False], f"{L} -> {T}: torch ({cap}) matches neither index form"
        if want is not None:
            assert near[want], f"{L} -> {T}: torch ({cap}) does not round the source index {'once' if want else 'twice'}"
        np.testing.assert_allclose(got[~d], form[True][~d], atol=1e-3, rtol=0)
    # the oracle's interpolation is the two-rounding form
    x = np.random.default_rng(0).standard_normal((1, 1499, 4)).astype(np.float32)
    i0, i1, l0, l1 = FO.source_index(1499, 900)
    assert np.array_equal(FO.linear_interpolation(x, 900), (x[:, i0] * l0[None, :, None] + x[:, i1] * l1[None, :, None]).astype(np.float32))
