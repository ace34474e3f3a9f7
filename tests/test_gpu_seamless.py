"""Seamless body streaming (`TrainWrapper.open_stream(..., seamless=True)`, `generate_long`, the C ABI `ts_body_stream_*`;
include/talkshow_hip.h, "seamless sessions").

The yardstick is always `generate_batch` on the concatenated audio with the same mode, seed and clip_index0, and every comparison is
EQUALITY: codes as integers, poses and log-probabilities as uint32 bits.  A window call goes through the entries a clip goes through, an
engine is never chosen by B or T, and every window starts at a multiple of 4 code rows (the Winograd tiles of the lowered stacks), so
nothing but equality is the claim.

Shapes: (F) full-size synthetic networks (PixelCNN 2048 / 256 / 15, VQ num_hiddens = 1024: both lowered conv stacks live) at B = 2,
T = 150 — 37 code rows, T % 4 = 2, rows that are interior on both sides of every seam; (S) the `pix_small` golden's PixelCNN with VQ nets
of 128 hidden channels at B = 33 (across the 16- and 32-row slab edges), T = 64, and the clips too short to leave anything interior
(T = 7: everything at the flush; T = 3: nothing at all).  Every test but the labelled control fails on a build without the feature: there
is no `seamless` keyword, no `generate_long` and no `ts_body_stream_*` symbol.
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
F32 = np.float32
SCHEDULES = [(150,), (64, 86), (10,) * 15, (37, 3, 110), (1,) * 40 + (110,)]
MODES = ["greedy", "philox", "uniforms"]


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    """The wrapper at full size on synthetic weights, B = 2 clips of 150 MFCC frames, and the one-shot results per mode (made once)."""
    from nets.init_model import init_model
    from talkshow_amd.config import Object
    vq_path = str(tmp_path_factory.mktemp("seamless") / "vq.pth")
    torch.save({"generator": {"g_body": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=39)),
                              "g_hand": synth.to_torch(synth.vqvae_state_dict(seed=7, in_dim=90, salt=1))}}, vq_path)
    cfg = json.load(open(os.path.join(REPO, "config", "body_pixel.json")))
    cfg["Model"]["vq_path"] = vq_path
    w = init_model("s2g_body_pixel", argparse.Namespace(gpu=0, infer=True), Object(cfg))
    w.load_state_dict({"generator": synth.to_torch(synth.pixelcnn_state_dict(seed=7)),
                       "audioencoder": synth.to_torch(synth.audioencoder_state_dict(seed=7))})
    B, T = 2, 150
    case = dict(w=w, B=B, T=T, mf=torch.from_numpy(synth.mfcc_features(31, B, T)).cuda(), ids=synth.speaker_ids(B),
                u=(0.999 * np.random.default_rng(5).random((B, T // 4, 2))).astype(F32), ref={})
    return case


@pytest.fixture(scope="module")
def small(golden):
    """The `pix_small` PixelCNN between an audio encoder and two VQ nets of 128 hidden channels, as a wrapper without a config file."""
    from nets.smplx_body_pixel import TrainWrapper
    from talkshow_amd.modules import AudioEncoder, GatedPixelCNN, VQVAE
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    w = object.__new__(TrainWrapper)
    w.generator = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    w.generator.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers,
                                                                         n_classes=n_cls)))
    w.audioencoder = AudioEncoder(64, 256, 2).cuda()
    w.audioencoder.load_state_dict(synth.to_torch(synth.audioencoder_state_dict(seed=3)))
    w.g_body, w.g_hand = VQVAE(39, 64, input_dim, 128, 2).cuda(), VQVAE(90, 64, input_dim, 128, 2).cuda()
    w.g_body.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=input_dim, num_hiddens=128)))
    w.g_hand.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=90, num_embeddings=input_dim, num_hiddens=128, salt=1)))
    w.each_dim, w.num_classes = [0, 39, 90], n_cls
    return w


def draw(mode, u=None):
    from talkshow_amd import _lib
    if mode == "greedy":
        return dict(mode=_lib.TS_SAMPLE_GREEDY)
    if mode == "uniforms":
        return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u)
    return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=5)


def one_shot(case, mode, **kw):
    key = (mode, tuple(sorted(kw)))
    if key not in case["ref"]:
        out = case["w"].generate_batch(case["mf"], case["ids"], **draw(mode, case["u"]), **kw)
        case["ref"][key] = tuple(_bits(o).copy() for o in out)
    return case["ref"][key]


def streamed(w, mf, ids, sched, mode, u=None, open_kw=None, logprobs=False):
    """The clip through a seamless session in the pushes of `sched`, then the flush -> (codes, pose bits[, logprob bits]), numpy."""
    B = int(mf.shape[0])
    st = w.open_stream(ids, B, max(sched), seamless=True, **(open_kw or {}))
    codes, poses, lps, at = [], [], [], 0
    for t in tuple(sched) + (None,):
        n, m = st.plan(0 if t is None else t, flush=t is None)
        d = draw(mode, None if u is None else np.ascontiguousarray(u[:, st.code_rows:st.code_rows + n]))
        out = (st.flush(**d, return_codes=True, logprobs=logprobs) if t is None else
               st.push(mf[:, at:at + t], **d, return_codes=True, logprobs=logprobs))
        assert tuple(out[0].shape) == (B, m, 129) and tuple(out[1].shape) == (B, n, 2)
        poses.append(_bits(out[0])), codes.append(_bits(out[1]))
        if logprobs:
            lps.append(_bits(out[2]))
        at += t or 0
        assert st.frames_in == at and st.code_rows == sum(c.shape[1] for c in codes) and st.frames == sum(p.shape[1] for p in poses)
    with pytest.raises(ValueError):
        st.push(mf[:, :4], **draw("greedy"))                      # the clip has ended
    st.close()
    res = (np.concatenate(codes, 1), np.concatenate(poses, 1))
    return res + ((np.concatenate(lps, 1),) if logprobs else ())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sched", SCHEDULES, ids=["whole", "64+86", "15x10", "37+3+110", "40x1+110"])
def test_any_chunking_returns_the_one_shot_bits_full_size(full, sched, mode):
    assert sum(sched) == full["T"]
    ref_codes, ref_poses = one_shot(full, mode)
    codes, poses = streamed(full["w"], full["mf"], full["ids"], sched, mode, full["u"])
    assert codes.shape == ref_codes.shape == (2, 37, 2) and poses.shape == ref_poses.shape == (2, 148, 129)
    assert np.array_equal(codes, ref_codes), f"codes differ first at row {int(np.argwhere(codes != ref_codes)[:, 1].min())}"
    bad = np.argwhere(poses != ref_poses)
    assert bad.size == 0, f"{len(bad)} pose words differ, frames {sorted(set(bad[:, 1].tolist()))[:12]} ..."


@pytest.mark.parametrize("T,sched", [(64, (20, 20, 24)), (7, (3, 4)), (3, (2, 1))], ids=["T=64", "T=7", "T=3"])
def test_small_networks_slab_edges_and_short_clips(small, T, sched):
    from talkshow_amd import _lib
    B = 33
    mf = torch.from_numpy(synth.mfcc_features(40 + T, B, T)).cuda()
    ids = np.arange(B) % small.num_classes
    codes, poses = streamed(small, mf, ids, sched, "philox")
    assert codes.shape == (B, T // 4, 2) and poses.shape == (B, 4 * (T // 4), 129)
    if T < 4:
        return                                                   # empty results, and no call was made
    ref_codes, ref_poses = small.generate_batch(mf, ids, **draw("philox"))
    assert np.array_equal(codes, _bits(ref_codes)) and np.array_equal(poses, _bits(ref_poses))
    if T == 7:                                                   # everything came out at the flush
        st = small.open_stream(ids, B, 7, seamless=True)
        assert st.plan(7) == (0, 0)
        assert tuple(st.push(mf, mode=_lib.TS_SAMPLE_GREEDY).shape) == (B, 0, 129) and st.plan(0, flush=True) == (1, 4)
        st.close()


def test_controls_as_session_defaults(full):
    rng = np.random.default_rng(9)
    V, NC = 2048, 4
    t0 = np.zeros((2, V), F32)
    t0[:, rng.choice(V, V // 2, replace=False)] = -np.inf
    kw = dict(sampling=[(0.8, 0.9, 0), (1.3, 1.0, 5)], style=[rng.random(NC).astype(F32) for _ in range(2)], code_bias=[t0, None],
              repeat=[(3, 0.7, 0.3), (5, 1.0, 0.5)])
    ref_codes, ref_poses, ref_lp = one_shot(full, "philox", logprobs=True, **kw)
    codes, poses, lp = streamed(full["w"], full["mf"], full["ids"], (37, 3, 110), "philox", open_kw=kw, logprobs=True)
    assert np.array_equal(codes, ref_codes) and np.array_equal(lp, ref_lp) and np.array_equal(poses, ref_poses)
    assert not np.array_equal(codes, one_shot(full, "philox")[0])          # the controls did something


def test_generate_long_equals_generate_batch(full):
    for mode in ("philox", "uniforms"):
        ref_codes, ref_poses = one_shot(full, mode)
        codes, poses = full["w"].generate_long(full["mf"], full["ids"], chunk_frames=48, **draw(mode, full["u"]))
        assert np.array_equal(_bits(codes), ref_codes) and np.array_equal(_bits(poses), ref_poses)


@pytest.mark.parametrize("mode", ["greedy", "philox"])
@pytest.mark.parametrize("t", [16, 40])
def test_long_clip_full_size_every_window_interior_and_the_ring_wraps(full, t, mode):
    """Where a long session spends its life: T = 602 (150 code rows, T % 4 = 2) in pushes of 16 and of 40 frames on the full-size
    networks.  The decoder windows of the steady state start well after the clip's start and end well before its end (interior on both
    sides, v0 up to 132), and 150 rows go round the code ring of 32 + 7 = 39 (t = 16) or 32 + 11 = 43 (t = 40) slots more than three times."""
    from talkshow_amd import streaming as S
    B, T = 2, 602
    key = ("long", mode)
    mf = full.setdefault("long_mf", torch.from_numpy(synth.mfcc_features(32, B, T)).cuda())
    if key not in full["ref"]:
        out = full["w"].generate_batch(mf, full["ids"], **draw(mode))
        full["ref"][key] = tuple(_bits(o).copy() for o in out)
    ref_codes, ref_poses = full["ref"][key]
    sched = (t,) * (T // t) + ((T % t,) if T % t else ())
    plan, two_sided = S.SeamlessPlan(), 0
    for c in [plan.push(x) for x in sched] + [plan.flush()]:
        two_sided += c.dec is not None and c.dec[0] >= 16 and c.dec[1] <= T // 4 - 16
    assert two_sided >= 5 and T // 4 > 3 * (S.RING_KEEP_ROWS + S.chain_rows(t))
    codes, poses = streamed(full["w"], mf, full["ids"], sched, mode)
    assert codes.shape == ref_codes.shape == (B, 150, 2) and poses.shape == ref_poses.shape == (B, 600, 129)
    assert np.array_equal(codes, ref_codes), f"codes differ first at row {int(np.argwhere(codes != ref_codes)[:, 1].min())}"
    bad = np.argwhere(poses != ref_poses)
    assert bad.size == 0, f"{len(bad)} pose words differ, frames {sorted(set(bad[:, 1].tolist()))[:12]} ..."


def test_state_is_bounded_for_any_history(small):
    from talkshow_amd import _lib
    B, t = 2, 16
    whole = torch.from_numpy(synth.mfcc_features(3, B, 60 * t)).cuda()
    st = small.open_stream([0, 1], B, t, seamless=True)
    lag = st.lag_rows
    assert lag in (20, 27)                      # 7 + 13 code rows; 14 + 13 where the audio encoder is lowered too (TS_CONV_WINO=1)
    seen, parts = {}, []
    for k in range(1, 61):
        p = st.push(whole[:, (k - 1) * t:k * t], mode=_lib.TS_SAMPLE_GREEDY)
        parts.append(p)
        if 4 * (k - 1) >= lag:
            assert tuple(p.shape) == (B, 16, 129)                # steady state: 4 code rows in, 16 frames out
        if k in (5, 20, 60):
            seen[k] = (st.state_bytes, st.graph_captures())
    assert seen[5][0] == seen[60][0] > 0
    assert seen[20][1] == seen[60][1] > 0, "the chain session went on capturing graphs after the warm-up pushes"
    assert st.frames_in == 960 and st.code_rows == 240 - (lag - 13) and st.frames == 4 * (240 - lag)
    parts.append(st.flush(mode=_lib.TS_SAMPLE_GREEDY))
    st.close()
    _, ref_poses = small.generate_batch(whole, [0, 1], mode=_lib.TS_SAMPLE_GREEDY)     # 240 rows round a ring of 39 slots
    assert np.array_equal(_bits(torch.cat(parts, 1)), _bits(ref_poses))


class Guarded:
    """An output of `shape` between two 4 KiB red zones, zones and body pre-filled with a sentinel (the manner of tests/test_gpu_canary.py)."""
    PAD = {torch.float32: 1024, torch.int64: 512}
    SENT = {torch.float32: 0x7FC0BEEF, torch.int64: 0x7EADBEEF7EADBEEF}

    def __init__(self, shape, dtype):
        self.n, self.pad, self.sent = int(np.prod(shape)), self.PAD[dtype], self.SENT[dtype]
        self.raw = torch.full((2 * self.pad + self.n,), self.sent, dtype=torch.int32 if dtype == torch.float32 else torch.int64, device="cuda")
        self.body = self.raw[self.pad:self.pad + self.n].view(dtype).view(shape)

    def check(self, what):
        assert bool((self.raw[:self.pad] == self.sent).all()) and bool((self.raw[self.pad + self.n:] == self.sent).all()), \
            f"{what}: a store landed outside the output"
        left = int((self.raw[self.pad:self.pad + self.n] == self.sent).sum())
        assert left == 0, f"{what}: {left} of {self.n} documented elements were never written"


def test_c_abi_writes_its_outputs_and_nothing_else(small):
    from talkshow_amd import _lib
    from talkshow_amd.modules import _index_tensor
    lib, B, T = _lib.load(), 3, 91
    mf = torch.from_numpy(synth.mfcc_features(8, B, T)).cuda()
    ids = _index_tensor([0, 1, 2], small.num_classes, "speaker id", torch.device("cuda"))
    h = C.c_void_p()
    _lib.check(lib.ts_body_stream_open(small.audioencoder.handle(), small.generator.handle(), small.g_body.handle(), small.g_hand.handle(),
                                       _lib.dptr(ids), B, 48, C.byref(h)))
    pieces = (None, 0, None, None, None, None, None, 0, None, None, 0)
    codes, poses, at = [], [], 0
    try:
        for t in (48, 43, None):
            n, m = C.c_int64(), C.c_int64()
            _lib.check(lib.ts_body_stream_plan(h, t or 0, int(t is None), C.byref(n), C.byref(m)))
            gc, gp = Guarded((B, n.value, 2), torch.int64), Guarded((B, m.value, 129), torch.float32)
            out = (_lib.TS_SAMPLE_GREEDY, None, 0, 0, C.c_void_p(gc.body.data_ptr()), C.c_void_p(gp.body.data_ptr())) + pieces
            if t is None:
                _lib.check(lib.ts_body_stream_flush(h, *out, _lib.stream_ptr()))
            else:
                chunk = mf[:, at:at + t].contiguous()
                _lib.check(lib.ts_body_stream_push(h, _lib.dptr(chunk), t, *out, _lib.stream_ptr()))
                at += t
            torch.cuda.synchronize()
            gc.check(f"codes of call {len(codes)}"), gp.check(f"poses of call {len(codes)}")
            codes.append(gc.body.clone()), poses.append(gp.body.clone())
        assert (lib.ts_body_stream_frames_in(h), lib.ts_body_stream_code_rows(h), lib.ts_body_stream_pose_frames(h)) == (T, T // 4, 4 * (T // 4))
        assert lib.ts_body_stream_push(h, _lib.dptr(mf), 4, *out, _lib.stream_ptr()) != 0 and b"flushed" in lib.ts_last_error()
    finally:
        torch.cuda.synchronize()
        lib.ts_body_stream_close(h)
    ref_codes, ref_poses = small.generate_batch(mf, ids, mode=_lib.TS_SAMPLE_GREEDY)
    assert np.array_equal(_bits(torch.cat(codes, 1)), _bits(ref_codes)) and np.array_equal(_bits(torch.cat(poses, 1)), _bits(ref_poses))


def test_refusals_move_no_counter(small):
    from talkshow_amd import _lib
    B = 2
    mf = torch.from_numpy(synth.mfcc_features(4, B, 48)).cuda()
    st = small.open_stream([0, 1], B, 48, seamless=True)
    st.push(mf, mode=_lib.TS_SAMPLE_GREEDY)
    before = (st.frames_in, st.code_rows, st.frames)
    enc = st.lag_rows - 13                      # 7; 14 where the audio encoder is lowered too (TS_CONV_WINO=1)
    n = 24 - enc - max(0, 12 - enc)             # the code rows a second push of 48 frames runs: 12
    assert before == (48, max(0, 12 - enc), 0) and st.plan(48) == (n, 4 * max(0, 24 - enc - 13)) and (enc, n) in ((7, 12), (14, 10))
    with pytest.raises(ValueError, match=rf"\(B=2, {n}, 2\)"):
        st.push(mf, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.zeros((B, 11, 2), F32))          # a wrong uniforms row count
    with pytest.raises(ValueError, match=rf"\(B=2, {n}, 2\)"):
        st.push(mf, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=[[[0.5, 0.5]] * 11] * B)            # ... as a list
    with pytest.raises(ValueError):
        st.push(mf[:, :0], mode=_lib.TS_SAMPLE_GREEDY)                                         # t = 0
    with pytest.raises(ValueError):
        st.push(torch.cat([mf, mf], 1), mode=_lib.TS_SAMPLE_GREEDY)                            # longer than max_frames
    with pytest.raises(ValueError, match="clip 1"):
        st.push(mf, given=[None, np.zeros((13, 2), np.int64)])                                 # more given rows than the call runs
    assert (st.frames_in, st.code_rows, st.frames) == before
    st.flush(mode=_lib.TS_SAMPLE_GREEDY)
    after = (st.frames_in, st.code_rows, st.frames)
    assert after == (48, 12, 48)
    for call in (lambda: st.push(mf, mode=_lib.TS_SAMPLE_GREEDY), lambda: st.flush(mode=_lib.TS_SAMPLE_GREEDY), lambda: st.plan(4)):
        with pytest.raises(ValueError):
            call()                                                                             # after the flush
    assert (st.frames_in, st.code_rows, st.frames) == after
    st.close()


def test_control_the_plain_session_has_a_seam_here(full):
    """CONTROL (passes without the feature): at (F) with chunks (64, 86) the plain session's poses differ from the one-shot call within 6
    code rows of the seam at code row 16 — the shapes above can tell a seam."""
    from talkshow_amd import _lib
    _, ref_poses = one_shot(full, "greedy")
    st = full["w"].open_stream(full["ids"], 2, 88)
    parts = [st.push(full["mf"][:, a:b].contiguous(), mode=_lib.TS_SAMPLE_GREEDY) for a, b in ((0, 64), (64, 150))]
    st.close()
    plain = _bits(torch.cat(parts, 1))
    assert plain.shape == ref_poses.shape
    assert (plain[:, 4 * 10:4 * 22] != ref_poses[:, 4 * 10:4 * 22]).any()
