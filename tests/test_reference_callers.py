"""The reference's own CALLER code driven against this repository's drop-in packages.

`oracle/build_ref_callers.py` compiles `init_model` / `infer` of the reference's `scripts/demo.py`, `init_model` / `body_loss` /
`test` of `scripts/test_body.py` and the two helper modules they import (`data_utils/lower_body.py`, `data_utils/get_j.py`) into
code objects under `oracle/_ref/` (git-ignored, built where /root/reference exists, travels to the GPU box like a built
`.so`; one raw-marshal `.code` file per unit + a JSON manifest of sha256 hashes that `load()` verifies before unmarshalling).  Here those code objects run unchanged with THIS repo's `nets` / `evaluation` / SMPL-X layer bound to the names the
scripts import — `demo.py --infer --num_sample 2` and `test_body.py`'s test loop — and their results are checked against
reference goldens and the oracles.  Stubbed, as they are outside the path: the phoneme `Wav2Vec2Processor` download, the
renderer, `np.save`'s target file and the dataset loader (the onset times come from the package's own `get_mfcc_ta(encoder_choice='onset')`:
librosa when installed, else its restatement in `talkshow_amd/frontend.py`).
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from talkshow_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import build_ref_callers as BRC  # noqa: E402
from oracle import talkshow_oracle as O      # noqa: E402


def _units():
    got = BRC.load()
    if got is None:
        pytest.skip("oracle/_ref/reference_callers.json is absent (python oracle/build_ref_callers.py where /root/reference exists; "
                    "__graft_entry__.build() does it)")
    return got


def test_reference_callers_build_here():
    """Where the reference tree exists (the build container) the lift must succeed and be current; elsewhere: skipped."""
    if not os.path.isdir(BRC.REF):
        pytest.skip("no reference tree on this machine")
    import hashlib
    BRC.build()
    units, meta = BRC.load()
    assert set(units) == {"demo", "test_body", "test_face", "test_vq", "continuity", "diversity", "lower_body", "get_j", "spg_gated_pixelcnn_v2", "spg_vqvae_modules",
                          "spg_wav2vec", "spg_vqvae_1d"}
    for unit, ent in meta["units"].items():
        assert hashlib.sha256(open(os.path.join(BRC.REF, ent["file"]), "rb").read()).hexdigest() == ent["source_sha256"]
        assert hashlib.sha256(open(os.path.join(BRC.OUT_DIR, unit + ".code"), "rb").read()).hexdigest() == ent["code_sha256"]
    ns = {}
    exec(units["lower_body"], ns)
    assert callable(ns["part2full"]) and callable(ns["poses2pred"])
    # product code never touches the reference callers
    for root in ("talkshow_amd", "nets", "evaluation"):
        for dp, _, fs in os.walk(os.path.join(REPO, root)):
            for f in fs:
                if f.endswith(".py"):
                    assert "build_ref_callers" not in open(os.path.join(dp, f)).read()


def test_reference_callers_integrity_is_checked(tmp_path):
    """a built unit that does not hash to its manifest entry is refused before it is unmarshalled, a manifest that names
    other units / files than `UNITS` is refused, and nothing in the load path unpickles anything."""
    import marshal
    src = open(BRC.__file__).read()
    assert "pickle" not in src.replace("no pickle", "").replace("The pickle of earlier rounds".lower(), "").replace("# the pickle of earlier rounds", "")
    code = compile("x = 1", "<t>", "exec")
    blob = marshal.dumps(code)
    man = {"python": list(sys.version_info[:2]), "units": {}}
    for unit, (rel, names) in BRC.UNITS.items():
        (tmp_path / (unit + ".code")).write_bytes(blob)
        man["units"][unit] = {"file": rel, "names": names, "source_sha256": "0" * 64, "code_sha256": BRC._sha(blob), "code_bytes": len(blob)}
    keep_ref, BRC.REF = BRC.REF, str(tmp_path / "no_reference_here")
    try:
        (tmp_path / "reference_callers.json").write_text(json.dumps(man))
        units, _ = BRC.load(str(tmp_path))
        assert set(units) == set(BRC.UNITS)
        (tmp_path / "demo.code").write_bytes(blob + b"\x00")                          # tampered: one byte more
        with pytest.raises(BRC.RefCallersError, match="does not hash"):
            BRC.load(str(tmp_path))
        (tmp_path / "demo.code").write_bytes(blob)
        man["units"]["demo"]["file"] = "scripts/other.py"                              # a manifest that redirects a unit
        (tmp_path / "reference_callers.json").write_text(json.dumps(man))
        with pytest.raises(BRC.RefCallersError, match="does not match"):
            BRC.load(str(tmp_path))
        man["python"] = [2, 7]
        (tmp_path / "reference_callers.json").write_text(json.dumps(man))
        assert BRC.load(str(tmp_path)) is None                                         # another interpreter's code objects: not loaded
        assert BRC.load(str(tmp_path / "empty")) is None
    finally:
        BRC.REF = keep_ref


class _SaveRecorder:
    """numpy with `save` captured (demo.py writes visualise/video/<name>/<clip>.npy)."""

    def __init__(self):
        self.saved = []

    def __getattr__(self, k):
        return getattr(np, k)

    def save(self, name, arr):
        self.saved.append((name, np.asarray(arr)))


class _Greedy:
    """The reference has no greedy decode (it always samples): the wrapper's `greedy=True` extension is switched on from the
    outside so that the caller code, which knows nothing of it, yields a deterministic result.  Everything else passes through."""

    def __init__(self, w):
        self._w = w

    def __getattr__(self, k):
        return getattr(self._w, k)

    def infer_on_audio(self, *a, **kw):
        return self._w.infer_on_audio(*a, greedy=True, **kw)


def _config(tmp_path):
    from talkshow_amd.config import Object
    vq_path = str(tmp_path / "vq.pth")
    torch.save({"generator": {"g_body": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=39)),
                              "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))}}, vq_path)
    cfg = json.load(open(os.path.join(REPO, "config", "body_pixel.json")))
    cfg["Model"]["vq_path"] = vq_path
    return Object(cfg)


def _golden(name):
    return dict(np.load(os.path.join(REPO, "tests", "golden", name + ".npz")))


@pytest.mark.gpu
@pytest.mark.parametrize("stand", [False, True])
def test_demo_py_infer_against_the_drop_in(tmp_path, monkeypatch, stand):
    """scripts/demo.py: init_model(body) + init_model(face) from checkpoint FILES, infer(..., num_sample=2): the (2 T, 265) array
    it saves must be the reference-golden body poses and face parameters assembled by the oracle's part2full restatement."""
    import nets
    import nets.smplx_body_pixel as bp
    from scipy.io import wavfile
    from talkshow_amd.pose_index import lower_pose_block
    units, _ = _units()
    gb, gf = _golden("body_e2e_full"), _golden("face_10s")
    k = 1                                                             # golden clip 1: speaker id 1 (body), zero identity (face)
    seed, B, N = (int(v) for v in gf["wav_seed"])
    wav = synth.wav16(seed, B, N)[k]
    wav_path = str(tmp_path / "clip.wav")
    wavfile.write(wav_path, 16000, wav.astype(np.float32))            # float wav: read back bit for bit
    # checkpoints on disk in the reference's layout (demo.py:54-62 reads ckpt['generator'])
    body_ckpt, face_ckpt = str(tmp_path / "body.pth"), str(tmp_path / "face.pth")
    torch.save({"generator": {"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                              "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))}}, body_ckpt)
    torch.save({"generator": {"generator": synth.to_torch(synth.face_state_dict(seed=7))}}, face_ckpt)
    # torchaudio is absent when the goldens are made: the reference golden is defined on given MFCC rows (SURVEY.md Appendix C
    # item 6); the same substitution here.  The face path reads the wav file for real.
    monkeypatch.setattr(bp, "get_mfcc_ta", lambda *a, **kw: gb["mfcc"][k].copy())
    lb = {}
    exec(units["lower_body"], lb)
    rec = _SaveRecorder()
    rendered = []
    ns = dict(torch=torch, np=rec, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel,
              LS3DCG=nets.LS3DCG, part2full=lb["part2full"],
              Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              get_vertices=lambda *a, **kw: (["verts"], None),
              matrix_to_axis_angle=None, rotation_6d_to_matrix=None)
    exec(units["demo"], ns)
    args = argparse.Namespace(gpu=0, infer=True, num_sample=2, audio_file=wav_path, id=int(gb["ids"][k]), only_face=False,
                              stand=stand, whole_body=False)
    config = _config(tmp_path)
    g_body = ns["init_model"]("s2g_body_pixel", body_ckpt, args, config)
    g_face = ns["init_model"]("s2g_face", face_ckpt, args, config)
    assert type(g_body).__module__.startswith("nets.") and type(g_face).__module__.startswith("nets.")
    render = types.SimpleNamespace(_render_sequences=lambda *a, **kw: rendered.append((a, kw)))
    ns["infer"](_Greedy(g_body), g_face, None, render, config, args)
    assert len(rec.saved) == 1 and len(rendered) == 1
    name, arr = rec.saved[0]
    assert name.endswith("clip") and arr.shape == (2 * 300, 265)
    want = O.assemble_full(gb["poses"][k][None], gf["out"][k][None], lower_pose_block(stand))[0]     # (300, 265)
    np.testing.assert_allclose(arr[:300], want, atol=1e-4, rtol=0)
    np.testing.assert_array_equal(arr[300:], arr[:300])               # greedy: both samples are the same sequence
    # the body block is the golden poses exactly where part2full copies them (columns outside the lower-body insert)
    assert np.abs(arr[:300] - want).max() < 1e-4


AUDIO = os.path.join(REPO, "tests", "golden", "audio")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["style.wav", "1st-page.wav", "french.wav"])
def test_demo_py_on_the_reference_recordings(tmp_path, name):
    """BASELINE configs[0] where the product runs: `scripts/demo.py::infer` (lifted, unchanged) on the reference's own demo recordings
    (committed fixtures under tests/golden/audio/: 22 kHz stereo int16 / 16 kHz / 24 kHz mono) with NOTHING patched in the
    audio path — wav file in, (T, 265) rows out: device resampler + MFCC -> audio encoder -> PixelCNN -> VQ decoders, device kaiser
    resampler -> wav2vec2 face generator, `part2full`.  Checked: the frame counts the reference ships for these files
    (`demo/style/*.npy` 300, `demo/1st-page/*.npy` 384, `demo/french/french.npy` 288 rows), the layout invariants of those shipped arrays
    (columns 3:9 zero, 9:12 = the fixed global orientation, the lower-body joints = `lower_pose`), equality with the
    oracle's assembly of the wrappers' own outputs, and the device MFCC rows against the float64 twin on real speech."""
    import nets
    from talkshow_amd import frontend as fe
    from talkshow_amd.pose_index import lower_pose_block
    units, _ = _units()
    man = json.load(open(os.path.join(AUDIO, "audio_manifest.json")))[name]
    wav_path = os.path.join(AUDIO, name)
    T = man["frames_30fps"]
    body_ckpt, face_ckpt = str(tmp_path / "body.pth"), str(tmp_path / "face.pth")
    torch.save({"generator": {"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                              "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))}}, body_ckpt)
    torch.save({"generator": {"generator": synth.to_torch(synth.face_state_dict(seed=7))}}, face_ckpt)
    lb = {}
    exec(units["lower_body"], lb)
    rec = _SaveRecorder()
    rendered = []
    ns = dict(torch=torch, np=rec, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel,
              LS3DCG=nets.LS3DCG, part2full=lb["part2full"],
              Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              get_vertices=lambda *a, **kw: (["verts"], None), matrix_to_axis_angle=None, rotation_6d_to_matrix=None)
    exec(units["demo"], ns)
    args = argparse.Namespace(gpu=0, infer=True, num_sample=1, audio_file=wav_path, id=2, only_face=False, stand=False, whole_body=False)
    config = _config(tmp_path)
    g_body = ns["init_model"]("s2g_body_pixel", body_ckpt, args, config)
    g_face = ns["init_model"]("s2g_face", face_ckpt, args, config)
    ns["infer"](_Greedy(g_body), g_face, None, types.SimpleNamespace(_render_sequences=lambda *a, **kw: rendered.append(a)), config, args)
    assert len(rec.saved) == 1 and len(rendered) == 1
    arr = rec.saved[0][1]
    assert arr.shape == (T, 265) and arr.dtype == np.float32 and np.isfinite(arr).all()
    # the wrappers alone: frame counts, and the saved rows are their outputs through the oracle's part2full restatement
    poses = g_body.infer_on_audio(wav_path, id=torch.tensor([2]).cuda(), fps=30, greedy=True)
    face = g_face.infer_on_audio(wav_path)
    assert poses.shape == (1, T, 129) and face.shape == (1, T, 103)
    want = O.assemble_full(poses, face, lower_pose_block(False))[0]
    np.testing.assert_allclose(arr, want, atol=1e-6, rtol=0)
    # layout invariants of the arrays the reference ships (demo/style/*.npy)
    assert not arr[:, 3:9].any()                                                          # eye poses: never generated
    np.testing.assert_allclose(arr[:, 9:12], np.tile(np.float32([3.0747, -0.0158, -0.0152]), (T, 1)), atol=1e-6, rtol=0)
    lower = np.asarray(lower_pose_block(False), np.float32).reshape(-1)                   # `lower_pose` (lower_body.py:4-8), 33 values
    cols = np.r_[3:18, 21:27, 30:36, 39:45]                                               # where part2full puts them (lower_body.py:77-86)
    np.testing.assert_array_equal(arr[:, cols], np.tile(lower, (T, 1)))
    assert arr[:, 165:].std() > 0 and arr[:, 0:3].std() > 0                               # expression / jaw do move
    # the device front-end on real speech (stereo int16 -> mono, 22 k / 16 k / 24 k -> 22 k): MFCC rows vs the float64 twin
    dev_rows = fe.get_mfcc_ta(wav_path, sr=22000, fps=30, smlpx=True, type="mfcc")
    wave = fe._load_mono_resampled(wav_path, 22000)
    twin = fe.mfcc_float64(wave, 22000, hop_length=734).T
    assert dev_rows.shape == twin.shape and abs(dev_rows.shape[0] - (T + 1)) <= 1
    err = float(np.abs(dev_rows - twin).max())
    print(f"\n{name}: device MFCC vs float64 twin max |err| = {err:.2e} over coefficients up to {np.abs(twin).max():.0f}")
    assert err <= 2e-3                                              # measured 3.7e-4 .. 8.4e-4 (fp32 FFT in LDS, coefficients up to 470 .. 660)
    # ... and that arithmetic changes none of the greedy codes: device rows and the float64 twin's rows decode to the same grid
    from talkshow_amd import _lib
    idt = torch.tensor([2]).cuda()
    c_dev, _ = g_body.generate_batch(torch.from_numpy(dev_rows[None]).cuda(), idt, mode=_lib.TS_SAMPLE_GREEDY)
    c_twin, _ = g_body.generate_batch(torch.from_numpy(twin.astype(np.float32)[None]).cuda(), idt, mode=_lib.TS_SAMPLE_GREEDY)
    changed = int((c_dev != c_twin).sum())
    print(f"{name}: greedy codes that differ between device MFCC rows and the float64 twin's: {changed} / {c_dev.numel()}")
    assert changed == 0


class _SMPLXStandIn:
    """`smplx.create(...)` stand-in with the call shape `data_utils/get_j.py` uses: keyword groups in, {'joints': (N, J, 3)} out,
    on this repo's device SMPL-X layer over synthetic model parameters (the licensed model file is absent: SURVEY.md §8f-2)."""

    def __init__(self, layer):
        self.layer, self.batch_size = layer, 0

    def __call__(self, betas, expression, jaw_pose, leye_pose, reye_pose, global_orient, body_pose, left_hand_pose,
                 right_hand_pose, return_verts=True):
        rows = torch.cat([jaw_pose, leye_pose, reye_pose, global_orient, body_pose, left_hand_pose, right_hand_pose, expression],
                         dim=-1).to(torch.float32)
        assert rows.shape[1] == 265 and betas.shape[0] == rows.shape[0]
        return {"joints": self.layer.joints(betas.to(torch.float32), rows)}


@pytest.mark.gpu
def test_test_body_py_loop_against_the_drop_in(tmp_path, monkeypatch):
    """scripts/test_body.py: init_model + the test() loop (infer_on_audio with B=2, FGD feature pushes, part2full, joints,
    body_loss, get_scores / get_BCscore) over two synthetic 'dataset' batches.  Checked: it runs to the end on this repo's
    `nets`, `evaluation` and SMPL-X layer (including the `.item()` calls on every metric), and its numbers equal the same
    quantities computed by the oracles from the reference-golden poses."""
    import nets
    import nets.smplx_body_pixel as bp
    import evaluation.FGD as FGD
    import evaluation.metrics as metrics
    from oracle import eval_oracle as EO
    from oracle import smplx_oracle as SO
    from talkshow_amd import smplx_lbs
    units, _ = _units()
    gb = _golden("body_e2e_full")
    T = 300
    cur = {"k": 0}
    monkeypatch.setattr(bp, "get_mfcc_ta", lambda *a, **kw: gb["mfcc"][cur["k"]].copy())
    lb, gj = {}, {}
    exec(units["lower_body"], lb)
    exec(units["get_j"], gj)
    model = SO.synthetic_model(seed=3)
    layer = smplx_lbs.SMPLXLayer(model)
    smplx_model = _SMPLXStandIn(layer)
    config = _config(tmp_path)
    args = argparse.Namespace(gpu=0, infer=True)
    body_ckpt, ae_ckpt = str(tmp_path / "body.pth"), str(tmp_path / "ae.pth")
    torch.save({"generator": {"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                              "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))}}, body_ckpt)
    torch.save({"generator": {"g": synth.to_torch(synth.ae_state_dict(seed=7))}}, ae_ckpt)
    printed = []
    from scipy.io import wavfile
    from talkshow_amd import frontend
    beats = np.asarray([0.35, 1.1, 2.4, 3.3, 5.05, 6.6, 8.2, 9.4])                                # tone bursts at these times (s)
    tt = np.arange(4000) / 16000.0
    for k in range(2):
        wv = 0.001 * np.random.default_rng(30 + k).standard_normal(160000)
        for j, b0 in enumerate(beats + 0.05 * k):
            wv[int(b0 * 16000):int(b0 * 16000) + 4000] += 0.5 * np.sin(2 * np.pi * (300 + 40 * j) * tt) * np.exp(-12 * tt)
        wavfile.write(str(tmp_path / f"clip{k}.wav"), 16000, wv.astype(np.float32))
    seen_onsets = []

    def fake_get_mfcc_ta(path, **kw):                                # the package's own front-end on the clip's wav file
        assert kw.get("encoder_choice") == "onset" and kw.get("am") is not None   # test_body.py:173
        on = frontend.get_mfcc_ta(path, **kw)
        assert on.ndim == 2 and on.shape[1] == 1 and on.shape[0] >= len(beats)
        seen_onsets.append(on)
        return on

    ns = dict(torch=torch, np=np, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel,
              s2g_body_ae=nets.s2g_body_ae, LVD=metrics.LVD, part2full=lb["part2full"], poses2pred=lb["poses2pred"],
              to3d=gj["to3d"], get_joints=gj["get_joints"], get_mfcc_ta=fake_get_mfcc_ta, tqdm=lambda it, **kw: it,
              Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              print=lambda *a: printed.append(" ".join(str(x) for x in a)))
    exec(units["test_body"], ns)
    generator = ns["init_model"]("s2g_body_pixel", body_ckpt, args, config)
    ae = ns["init_model"]("s2g_body_ae", ae_ckpt, args, config)
    handler = FGD.EmbeddingSpaceEvaluator(ae, None, "cuda")
    # two 'dataset' items in the loader's format (data_utils/dataloader_torch.py): 165-wide axis-angle poses + 100 expression
    rng = np.random.default_rng(11)
    loader, gts = [], []
    for k in range(2):
        p165 = (0.2 * rng.standard_normal((1, 165, T))).astype(np.float32)
        exp = (0.5 * rng.standard_normal((1, 100, T))).astype(np.float32)
        gts.append((p165, exp))
        loader.append({"aud_feat": torch.zeros(1, 64, T), "poses": torch.from_numpy(p165), "expression": torch.from_numpy(exp),
                       "speaker": torch.tensor([20 + int(gb["ids"][k])]), "betas": torch.zeros(1, 1, 300, dtype=torch.float64),
                       "aud_file": [str(tmp_path / f"clip{k}.wav")]})

    class Loader(list):
        def __iter__(self):
            for i, b in enumerate(list.__iter__(self)):
                cur["k"] = i
                yield b

    ns["test"](Loader(loader), _Greedy(generator), handler, smplx_model, config)
    got = {ln.split("=")[0].strip(): float(ln.split("=")[1]) for ln in printed if "=" in ln and "score" not in ln}
    bc = [ln for ln in printed if ln.startswith("Beat consistency score=")]
    assert set(got) >= {"LVD", "error", "diverse", "fgd_dist", "feat_dist"} and len(bc) == 1
    assert len(seen_onsets) == 2 and all(np.abs(on[:, 0][None, :] - (beats + 0.05 * k)[:, None]).min(axis=1).max() < 0.08
                                         for k, on in enumerate(seen_onsets))            # every burst found within two frames + a hop
    # ---- the same quantities from the oracles over the golden poses ----
    LD, JD = [], []
    for k in range(2):
        pred129 = np.repeat(gb["poses"][k][None], 2, 0)                                           # B = 2 copies (greedy)
        zf = np.zeros((2, T, 103), np.float32)
        full = np.stack([lb["part2full"](torch.from_numpy(np.concatenate([zf[j, :, :3], pred129[j], zf[j, :, 3:]], -1))).numpy()
                         for j in range(2)])
        pj = np.stack([SO.smplx_forward(model, np.zeros(300), full[j])[0] for j in range(2)])               # (2, T, J, 3)
        p165, exp = gts[k]
        rows = np.concatenate([p165[0], exp[0]], 0).T                                             # (T, 265)
        g265 = lb["poses2pred"](torch.from_numpy(rows)).numpy()
        g265 = np.concatenate([np.zeros((T, 3), np.float32), g265[:, 3:165], np.zeros((T, 100), np.float32)], -1)
        gjn = SO.smplx_forward(model, np.zeros(300), g265)[0]
        LD.append(EO.body_loss(gjn, pj))
        JD.append((pj, gjn))
    for key, name in (("LVD", "LVD"), ("error", "error"), ("diverse", "diverse")):
        want = np.mean([d[name] for d in LD])
        assert abs(got[key] - want) <= 2e-4 * max(1.0, abs(want)), (key, got[key], want)
    assert np.isfinite(got["fgd_dist"]) and got["fgd_dist"] >= -1e-6 and np.isfinite(got["feat_dist"]) and got["feat_dist"] > 0


@pytest.mark.gpu
def test_test_face_py_loop_against_the_drop_in(tmp_path):
    """scripts/test_face.py (VERDICT r5 missing #6): its `init_model` from a checkpoint FILE and its `test()` loop — `infer_on_audio(wav file,
    id=speaker - 20, frame=T, am=..., am_sr=16000)`, the 265-d row it builds around the 103 face parameters, `get_joints` for both rows,
    its own `face_loss` (jaw / landmark distances, LVD) with the `.item()` prints — lifted unchanged and run on this repo's `nets`,
    `evaluation.metrics.LVD` and SMPL-X layer.  Expected values: the reference's `face_loss` (the lifted function itself) applied to what
    the float64 SMPL-X oracle makes of the REFERENCE-GOLDEN face output (`face_10s`, clip 0: one-hot class 1)."""
    import nets
    import evaluation.metrics as metrics
    from oracle import smplx_oracle as SO
    from scipy.io import wavfile
    from talkshow_amd import smplx_lbs
    units, _ = _units()
    gf = _golden("face_10s")
    seed, B, N = (int(v) for v in gf["wav_seed"])
    k, T = 0, 300
    spk = int(np.argmax(gf["ids"][k]))
    assert gf["ids"][k].sum() == 1.0
    wav_path = str(tmp_path / "clip.wav")
    wavfile.write(wav_path, 16000, synth.wav16(seed, B, N)[k].astype(np.float32))
    face_ckpt = str(tmp_path / "face.pth")
    torch.save({"generator": {"generator": synth.to_torch(synth.face_state_dict(seed=7))}}, face_ckpt)
    gj = {}
    exec(units["get_j"], gj)
    model = SO.synthetic_model(seed=3)
    smplx_model = _SMPLXStandIn(smplx_lbs.SMPLXLayer(model))
    printed = []
    ns = dict(torch=torch, np=np, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel, LVD=metrics.LVD,
              get_joints=gj["get_joints"], tqdm=lambda it, **kw: it,
              Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              print=lambda *a: printed.append(" ".join(str(x) for x in a)))
    exec(units["test_face"], ns)
    config = _config(tmp_path)
    args = argparse.Namespace(gpu=0, infer=True)
    generator = ns["init_model"]("s2g_face", face_ckpt, args, config)
    assert type(generator).__module__.startswith("nets.")
    rng = np.random.default_rng(13)
    p165 = (0.2 * rng.standard_normal((1, 165, T))).astype(np.float32)
    exp = (0.5 * rng.standard_normal((1, 100, T))).astype(np.float32)
    loader = [{"aud_feat": torch.zeros(1, 64, T), "poses": torch.from_numpy(p165), "expression": torch.from_numpy(exp),
               "speaker": torch.tensor([20 + spk]), "betas": torch.zeros(1, 1, 300, dtype=torch.float64), "aud_file": [wav_path]}]
    ns["test"](loader, generator, smplx_model, args, config)
    got = {ln.split("=")[0].strip(): float(ln.split("=")[1]) for ln in printed if "=" in ln}
    assert set(got) >= {"jaw_l1", "landmark_l1", "LVD"}
    # the same quantities from the reference-golden face rows through the float64 SMPL-X oracle and the reference's own face_loss
    face = gf["out"][k]                                                                 # (300, 103)
    full = np.concatenate([face[:, :3], np.zeros((T, 162), np.float32), face[:, 3:]], -1)
    poses = np.concatenate([p165[0], exp[0]], 0).T.copy()                               # (T, 265)
    poses[:, 3:165] = full[:, 3:165]
    gtj = SO.smplx_forward(model, np.zeros(300), poses)[0]
    prj = SO.smplx_forward(model, np.zeros(300), full)[0]
    want = ns["face_loss"](torch.from_numpy(gtj).float(), torch.from_numpy(poses), torch.from_numpy(prj).float(), torch.from_numpy(full))
    for key in ("jaw_l1", "landmark_l1", "LVD"):
        w_ = float(want[key])
        assert abs(got[key] - w_) <= 2e-4 * max(1.0, abs(w_)), (key, got[key], w_)


@pytest.mark.gpu
def test_test_vq_py_loop_against_the_drop_in(tmp_path):
    """scripts/test_vq.py::test (VERDICT r5 missing #6): `s2g_body_vq.infer_on_audio(wav, initial_pose=(1, 265, T), id, fps=30, B=1)` and
    its 'capacity' metric (L1 between the c_index rows of the ground truth and the VQ-VAE round trip), lifted unchanged.  Expected: the same
    metric from the REFERENCE-GOLDEN round trip (`body_vq_e2e_full`, made by the reference wrapper on the same poses)."""
    import nets
    units, _ = _units()
    g = _golden("body_vq_e2e_full")
    T = 300
    lb, gj = {}, {}
    exec(units["lower_body"], lb)
    exec(units["get_j"], gj)
    cfg = json.load(open(os.path.join(REPO, "config", "body_vq.json")))
    from talkshow_amd.config import Object
    config = Object(cfg)
    w = nets.s2g_body_vq(argparse.Namespace(gpu=0, infer=True), config)
    w.load_state_dict({"g_body": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=39)),
                       "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))})
    printed = []
    ns = dict(torch=torch, np=np, to3d=gj["to3d"], c_index_3d=lb["c_index_3d"], tqdm=lambda it, **kw: it,
              print=lambda *a: printed.append(" ".join(str(x) for x in a)))
    exec(units["test_vq"], ns)
    loader, want = [], []
    c_index = np.asarray(g["c_index"])
    for k in range(2):
        p165 = np.zeros((1, 165, T), np.float32)
        p165[0, c_index, :] = g["poses129"][k].T
        loader.append({"aud_feat": torch.zeros(1, 64, T), "poses": torch.from_numpy(p165), "expression": torch.zeros(1, 100, T),
                       "speaker": torch.tensor([20]), "betas": torch.zeros(1, 1, 300, dtype=torch.float64), "aud_file": ["unused.wav"]})
        ref = g["out"][:, k * 129:(k + 1) * 129]                                         # the reference wrapper's round trip of clip k
        want.append(np.abs(g["poses129"][k][:ref.shape[0]] - ref).sum(-1).mean())
    ns["test"](loader, w, config)
    got = {ln.split("=")[0].strip(): float(ln.split("=")[1]) for ln in printed if "=" in ln}
    assert "capacity" in got
    assert abs(got["capacity"] - float(np.mean(want))) <= 2e-4 * max(1.0, float(np.mean(want))), (got, np.mean(want))


@pytest.mark.gpu
def test_continuity_py_infer_against_the_drop_in(tmp_path):
    """scripts/continuity.py::infer (VERDICT r5 missing #6), lifted unchanged: the loop over 300-frame dataset items that calls
    `g_body.infer_on_audio(wav, initial_pose=..., norm_stats=..., txgfile=None, id=id, var=var, fps=30, continuity=True, smooth=False)` —
    the two-part generation behind `get_mfcc_sepa` —, pads / trims to the (zero) face length, `part2full`, `get_vertices`, `np.save`, the
    renderer's `_render_continuity`.  Wav file in (device resampler + MFCC of the first 2 s and of the rest), (300, 265) rows out.
    Expected: the oracle's restatement of the reference's two-chunk procedure on the float64-grade host twin of the same front-end, through
    the oracle's part2full."""
    import nets
    from scipy.io import wavfile
    from talkshow_amd import frontend as fe
    from talkshow_amd.pose_index import lower_pose_block
    units, _ = _units()
    lb = {}
    exec(units["lower_body"], lb)
    wav_path = str(tmp_path / "clip.wav")
    wavfile.write(wav_path, 16000, synth.wav16(77, 1, 160000)[0].astype(np.float32))
    body_ckpt = str(tmp_path / "body.pth")
    sd_p, sd_a = synth.pixelcnn_state_dict(seed=7), synth.audioencoder_state_dict(seed=7)
    torch.save({"generator": {"generator": synth.to_torch(sd_p), "audioencoder": synth.to_torch(sd_a)}}, body_ckpt)
    config = _config(tmp_path)
    args = argparse.Namespace(gpu=0, infer=True)
    demo = {}
    exec(units["demo"], dict(torch=torch, np=np, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel,
                             LS3DCG=nets.LS3DCG), demo)
    g_body = demo["init_model"]("s2g_body_pixel", body_ckpt, args, config)     # continuity.py imports diversity.py's init_model: the same function
    rec, rendered = _SaveRecorder(), []
    ns = dict(torch=torch, np=rec, part2full=lb["part2full"], Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              get_vertices=lambda *a, **kw: (["gt-verts", "pred-verts"], None), matrix_to_axis_angle=None, rotation_6d_to_matrix=None,
              denormalize=None)
    exec(units["continuity"], ns)
    T = 300
    rng = np.random.default_rng(5)
    loader = [{"poses": torch.from_numpy((0.2 * rng.standard_normal((1, 165, T))).astype(np.float32)),
               "expression": torch.from_numpy((0.5 * rng.standard_normal((1, 100, T))).astype(np.float32)),
               "speaker": torch.tensor([22]), "betas": torch.zeros(1, 1, 300, dtype=torch.float64), "aud_file": [wav_path]},
              {"poses": torch.zeros(1, 165, 120), "expression": torch.zeros(1, 100, 120), "speaker": torch.tensor([20]),
               "betas": torch.zeros(1, 1, 300, dtype=torch.float64), "aud_file": ["skipped: not 300 frames long"]}]
    render = types.SimpleNamespace(_render_continuity=lambda *a, **kw: rendered.append((a, kw)))
    ns["infer"](None, _Greedy(g_body), None, None, "exp", loader, None, torch.device("cuda", 0), None, True, None, render, args, config, (None, None))
    assert len(rec.saved) == 1 and len(rendered) == 1 and rendered[0][0][1] == "pred-verts" and rendered[0][1] == {"frame": 60}
    arr = rec.saved[0][1]
    assert arr.shape == (T, 265) and arr.dtype == np.float32
    # the reference's two-chunk procedure, restated by the oracle, on the host twin of get_mfcc_sepa
    feat, gap = fe.get_mfcc_sepa(wav_path, fps=30, sr=22000, host=True)
    assert gap == 1 + 44000 // 734 and feat.shape[1] == 64
    ref, _ = O.body_pixel_infer_continuity(feat[None], gap, np.asarray([2]), sd_a, sd_p, synth.vqvae_state_dict(seed=7, in_dim=39),
                                           synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))
    n = ref.shape[1]
    body = np.concatenate([ref[0], np.repeat(ref[0, -1:], T - n, 0)], 0) if n < T else ref[0, :T]      # continuity.py: pad with the last frame / trim
    want = O.assemble_full(body[None], np.zeros((1, T, 103), np.float32), lower_pose_block(False))[0]
    np.testing.assert_allclose(arr, want, atol=1e-4, rtol=0)


class _SMPLXVerticesStandIn(_SMPLXStandIn):
    """The per-frame call shape of `scripts/diversity.py::get_vertices` / `scripts/demo.py::get_vertices`: one row in, an object with
    `.vertices (1, V, 3)` and `.body_pose (1, 63)` out, on this repo's device SMPL-X layer (built with_vertices=True)."""

    def __call__(self, betas, expression, jaw_pose, leye_pose, reye_pose, global_orient, body_pose, left_hand_pose, right_hand_pose,
                 return_verts=True):
        rows = torch.cat([jaw_pose, leye_pose, reye_pose, global_orient, body_pose, left_hand_pose, right_hand_pose, expression],
                         dim=-1).to(torch.float32)
        joints, verts = self.layer.vertices(betas.to(torch.float32), rows)
        return types.SimpleNamespace(vertices=verts, joints=joints, body_pose=body_pose)


@pytest.mark.gpu
def test_diversity_py_infer_against_the_drop_in(tmp_path, monkeypatch):
    """scripts/diversity.py (VERDICT r5 missing #6), lifted unchanged: `init_model` from checkpoint files, `infer` — the loop over 300-frame
    dataset items with `g_face.infer_on_audio(wav, initial_pose=..., norm_stats=None, w_pre=False, frame=None, am=..., am_sr=...)` and
    `g_body.infer_on_audio(wav, initial_pose=..., norm_stats=..., txgfile=None, id=id, fps=30, w_pre=False)`, `part2full` / `poses2pred`,
    `np.save`, the renderer — and its own `get_vertices` (one SMPL-X call per frame) on this repo's SMPL-X layer.  The saved (300, 265)
    rows must be the reference-golden body poses + face parameters through the oracle's part2full; the vertices the per-frame loop
    returns must be the float64 oracle's."""
    import nets
    import nets.smplx_body_pixel as bp
    from oracle import smplx_oracle as SO
    from scipy.io import wavfile
    from talkshow_amd import smplx_lbs
    from talkshow_amd.pose_index import lower_pose_block
    units, _ = _units()
    gb, gf = _golden("body_e2e_full"), _golden("face_10s")
    k, T = 1, 300                                                     # golden clip 1: speaker id 1 (body), zero identity (face)
    seed, B, N = (int(v) for v in gf["wav_seed"])
    wav_path = str(tmp_path / "clip.wav")
    wavfile.write(wav_path, 16000, synth.wav16(seed, B, N)[k].astype(np.float32))
    body_ckpt, face_ckpt = str(tmp_path / "body.pth"), str(tmp_path / "face.pth")
    torch.save({"generator": {"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                              "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))}}, body_ckpt)
    torch.save({"generator": {"generator": synth.to_torch(synth.face_state_dict(seed=7))}}, face_ckpt)
    monkeypatch.setattr(bp, "get_mfcc_ta", lambda *a, **kw: gb["mfcc"][k].copy())     # as in the demo test: the golden is defined on given rows
    lb = {}
    exec(units["lower_body"], lb)
    rec, rendered = _SaveRecorder(), []
    ns = dict(torch=torch, np=rec, s2g_face=nets.s2g_face, s2g_body_vq=nets.s2g_body_vq, s2g_body_pixel=nets.s2g_body_pixel, LS3DCG=nets.LS3DCG,
              part2full=lb["part2full"], poses2pred=lb["poses2pred"], Wav2Vec2Processor=types.SimpleNamespace(from_pretrained=lambda *a, **kw: "am-stub"),
              matrix_to_axis_angle=None, rotation_6d_to_matrix=None, denormalize=None)
    exec(units["diversity"], ns)
    config = _config(tmp_path)
    args = argparse.Namespace(gpu=0, infer=True)
    g_body = ns["init_model"]("s2g_body_pixel", body_ckpt, args, config)
    g_face = ns["init_model"]("s2g_face", face_ckpt, args, config)
    model = SO.synthetic_model(seed=3)
    smplx_model = _SMPLXVerticesStandIn(smplx_lbs.SMPLXLayer(model, with_vertices=True))
    rng = np.random.default_rng(21)
    p165 = (0.2 * rng.standard_normal((1, 165, T))).astype(np.float32)
    exp = (0.5 * rng.standard_normal((1, 100, T))).astype(np.float32)
    loader = [{"poses": torch.from_numpy(p165), "expression": torch.from_numpy(exp), "speaker": torch.tensor([20 + int(gb["ids"][k])]),
               "betas": torch.zeros(1, 1, 300, dtype=torch.float64), "aud_file": [wav_path]}]
    render = types.SimpleNamespace(_render_sequences=lambda *a, **kw: rendered.append((a, kw)))
    ns["infer"](None, _Greedy(g_body), g_face, None, "exp", loader, None, torch.device("cuda", 0), None, True, smplx_model, render, args, config)
    assert len(rec.saved) == 1 and len(rendered) == 1
    arr = rec.saved[0][1]
    want = O.assemble_full(gb["poses"][k][None], gf["out"][k][None], lower_pose_block(False))[0]
    assert arr.shape == (T, 265)
    np.testing.assert_allclose(arr, want, atol=1e-4, rtol=0)
    # what get_vertices handed the renderer: [prediction] vertices, one SMPL-X call per frame; against the float64 oracle on the expected rows
    verts = rendered[0][0][1]
    assert len(verts) == 1 and verts[0].shape[0] == T
    ref_v = SO.smplx_forward(model, np.zeros(300), want[:8])[1]
    np.testing.assert_allclose(verts[0][:8], ref_v, atol=2e-4, rtol=0)
