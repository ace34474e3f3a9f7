"""Guidance at clip level in a plain body session (`TrainWrapper.open_stream(..., guide=)`, `BodyStream`; DESIGN.md §5, "session pairs").

B = 3: clip 0 guided against a second recording under another id, clip 1 guided by id only, clip 2 plain.  The chain session behind it
has S = 5 slots (the clips, then the two shadows) and the audio encoder runs on E = 4 streams.  Yardsticks: a twin built by hand from
`PixelCNNStream` with pairs; the one-shot `GatedPixelCNN.run(..., guide=)` on the rows the session encoded, for the log-probability bits; a
fresh one-clip session for a restarted clip.  EQUALITY throughout.  Every test fails on a build without the feature.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import _lib, synth

pytestmark = pytest.mark.gpu
SEED, CLIP0 = 23, 6
SCHED = (3, 1, 4, 2)                      # code rows per push
IDS = [1, 0, 3]
GUIDE = [{"scale": 2.0, "id": 2, "audio": True}, {"scale": 2.0, "id": 3}, None]
KW = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def w(golden):
    import bench
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    w = bench.build_models(0, seed=7)[0]
    w.generator = m
    T = 4 * sum(SCHED)
    w.mf = torch.from_numpy(synth.mfcc_features(601, 3, T)).cuda()
    w.ms = torch.from_numpy(synth.mfcc_features(602, 1, T)[0]).cuda()       # what clip 0's shadow hears
    return w


def chunks():
    at = 0
    for hc in SCHED:
        yield 4 * at, 4 * (at + hc)
        at += hc


def push_guide(i, f0, f1, ms):
    """The `guide=` of push i: the shadow's chunk every time; the third push brings other scales."""
    if i == 2:
        return [{"scale": -0.5, "mfcc": ms[f0:f1]}, 0.0, None]
    return [{"mfcc": ms[f0:f1]}, None, None]


def test_a_guided_session_equals_its_twin_built_from_the_chain_session(w):
    cap = 4 * max(SCHED)
    s = w.open_stream(torch.tensor(IDS), 3, cap, guide=GUIDE)
    plain = w.open_stream(torch.tensor(IDS), 3, cap)
    assert (s.g.S, s.g.E, s.g.spread()) == (5, 4, [0, 1, 2, 3, 1]) and s.pix.pairs == {0: (3, 2.0), 1: (4, 2.0)}
    twin = w.generator.open_stream(np.array(IDS + [2, 3], np.int64), 5, max(SCHED), pairs={0: (3, 2.0), 1: (4, 2.0)})
    idx = torch.tensor([0, 1, 2, 3, 1], device="cuda")
    got, ref, base, rows_all = [], [], [], []
    for i, (f0, f1) in enumerate(chunks()):
        got.append(s.push(w.mf[:, f0:f1], logprobs=True, guide=push_guide(i, f0, f1, w.ms), **KW))
        base.append(plain.push(w.mf[:, f0:f1], logprobs=True, **KW))
        rows = w.audioencoder.forward_nlc(torch.cat([w.mf[:, f0:f1], w.ms[None, f0:f1]])).index_select(0, idx)
        rows_all.append(rows)
        c, lp = twin.step(rows, logprobs=True, guide={0: -0.5, 1: 0.0} if i == 2 else None, **KW)
        ref.append((w._decode_pair(c[:3].contiguous()), lp[:3]))
    assert s.frames == 4 * sum(SCHED) and list(s.slot_rows) == [sum(SCHED)] * 3
    for k in (0, 1):
        a, b, p = (torch.cat([x[k] for x in v], 1) for v in (got, ref, base))
        assert a.shape[0] == 3 and torch.equal(a, b)
        assert torch.equal(a[2], p[2]), "the plain clip has the bits of the session without guidance"
        assert not torch.equal(a[0], p[0]) and not torch.equal(a[1], p[1]), "guidance moved nothing: the equality would be vacuous"
    # the log-probability bits of clip 1 up to the push that changes its scale, against the one-shot guided run on the rows the session encoded
    rows = torch.cat(rows_all, 1)
    n = SCHED[0] + SCHED[1]
    out = w.generator.run(np.array([IDS[1]], np.int64), rows[1:2, :n], mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0 + 1, logprobs=True,
                          guide=[{"scale": 2.0, "id": 3}])
    assert np.array_equal(_bits(torch.cat([x[1] for x in got], 1)[1, :n]), _bits(out[2])[0])
    out = w.generator.run(np.array([IDS[0]], np.int64), rows[0:1, :n], mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0, logprobs=True,
                          guide=[{"scale": 2.0, "id": 2, "aud_rows": rows[3, :n].cpu().numpy()}])
    assert np.array_equal(_bits(torch.cat([x[1] for x in got], 1)[0, :n]), _bits(out[2])[0])
    for x in (s, plain, twin):
        x.close()


def test_restart_with_a_guide_entry_equals_a_fresh_one_clip_guided_session(w):
    cap = 4 * max(SCHED)
    s = w.open_stream(torch.tensor(IDS), 3, cap, guide=GUIDE)
    still = w.open_stream(torch.tensor(IDS), 3, cap, guide=GUIDE)
    fresh1 = fresh0 = None
    got, keep, f1p, f0p = [], [], [], []
    for i, (f0, f1) in enumerate(chunks()):
        g = [{"mfcc": w.ms[f0:f1]}, None, None]
        if i == 2:
            s.restart([1, 0], [2, 1], clip_indices=[44, 45], guide=[{"scale": 1.5, "id": 0}, None])
            assert s.pix.pairs == {0: (3, 0.0), 1: (4, 1.5)} and list(s.slot_rows) == [0, 0, 4]
            fresh1 = w.open_stream(torch.tensor([2]), 1, cap, guide=[{"scale": 1.5, "id": 0}])
            fresh0 = w.open_stream(torch.tensor([1]), 1, cap)              # a shadow restarted without an entry is switched off
        got.append(s.push(w.mf[:, f0:f1], guide=g, **KW))
        keep.append(still.push(w.mf[:, f0:f1], guide=g, **KW))
        if fresh1 is not None:
            f1p.append(fresh1.push(w.mf[1:2, f0:f1], **dict(KW, clip_index0=44)))
            f0p.append(fresh0.push(w.mf[0:1, f0:f1], **dict(KW, clip_index0=45)))
    got, keep, f1p, f0p = (torch.cat(v, 1) for v in (got, keep, f1p, f0p))
    t0 = 4 * (SCHED[0] + SCHED[1])
    assert torch.equal(got[1, t0:], f1p[0]), "the restarted guided clip against a fresh one-clip guided session"
    assert torch.equal(got[0, t0:], f0p[0]), "the clip whose shadow restarted at scale 0 against a fresh plain session"
    assert torch.equal(got[2], keep[2]) and torch.equal(got[:2, :t0], keep[:2, :t0]), "a neighbour's poses changed"
    assert not torch.equal(got[1, t0:], keep[1, t0:])
    for x in (s, still, fresh1, fresh0):
        x.close()


def test_refusals_name_the_clip_and_move_nothing(w):
    cap = 4 * max(SCHED)
    s = w.open_stream(torch.tensor(IDS), 3, cap, guide=GUIDE)
    mf, ms = w.mf[:, :12], w.ms[:12]
    bad = [
        (None, "guide of clip 0: the shadow was opened with audio of its own"),
        (2.0, "guide of clip 0: the shadow was opened with audio of its own"),
        ([{"mfcc": ms[:8]}, None, None], r"guide of clip 0: .*\"mfcc\" of shape \(12, 64\) is required, got \(8, 64\)"),
        ([{"mfcc": ms}, {"mfcc": ms}, None], "guide of clip 1: the shadow was opened without audio of its own"),
        ([{"mfcc": ms}, None, 1.0], "guide of clip 2: the clip was opened without a shadow"),
        ([{"mfcc": ms, "scal": 1.0}, None, None], "guide of clip 0: unknown keys"),
        ([{"mfcc": ms}, float("nan"), None], "guide of clip 1: the scale is NaN"),
        ([{"mfcc": ms, "scale": 1e5}, None, None], "guide of clip 0: the scale exceeds 1e4"),
        ([{"mfcc": ms}, None], "one entry per clip"),
    ]
    for g, text in bad:
        with pytest.raises(ValueError, match=text):
            s.push(mf, guide=g, **KW)
    for call, text in [(lambda: s.save([1]), "save: clip 1 is guided"), (lambda: s.fork(2, [0]), "fork: clip 0 is guided"),
                       (lambda: s.fork(1, [2]), "fork: clip 1 is guided"), (lambda: s.load([0], s.save([2])), "load: clip 0 is guided"),
                       (lambda: s.restart([2], [1], guide=[{"scale": 1.0}]), "guide of clip 2: the clip was opened without a shadow"),
                       (lambda: s.restart([0], [1], guide=[{"scale": 1.0, "audio": False}]), "guide of clip 0: \"audio\" stays")]:
        with pytest.raises(ValueError, match=text):
            call()
    assert s.frames == 0 and s.pix.graph_captures() == 0 and s.pix.pairs == {0: (3, 2.0), 1: (4, 2.0)}
    p = s.push(mf, guide=[{"mfcc": ms}, None, None], **KW)
    assert p.shape == (3, 12, 129) and s.frames == 12
    s.close()
    plain = w.open_stream(torch.tensor(IDS), 3, cap)
    with pytest.raises(ValueError, match="opened without a shadow"):
        plain.push(mf, guide=2.0, **KW)
    with pytest.raises(ValueError, match="opened without a shadow"):
        plain.restart([0], [1], guide=[{"scale": 1.0}])
    assert plain.frames == 0
    plain.close()
    for g, text in [([{"scale": 2.0, "idd": 1}, None, None], "guide of clip 0: unknown keys"), ([None, {"id": 1}, None], "guide of clip 1: \"scale\" is required"),
                    ([None, None, {"scale": 1.0, "id": 9}], "guide of clip 2: id 9 is outside"), ([None, None], "one entry per clip")]:
        with pytest.raises(ValueError, match=text):
            w.open_stream(torch.tensor(IDS), 3, cap, guide=g)


def test_style_rows_in_open_and_restart_entries_against_the_one_shot_run(w):
    """A shadow's weight row from an open entry (written as a restart at row 0 writes it) and from a restart entry, and a shadow that
    takes its clip's own weight row: log-probability bits against `run(..., style=, guide=[{"style": ...}])` on the rows the session
    encoded."""
    rng = np.random.default_rng(9)
    row_a, row_b, crow0, crow1 = (rng.random(4).astype(np.float32) for _ in range(4))
    cap = 4 * max(SCHED)
    s = w.open_stream(torch.tensor([1, 0]), 2, cap, guide=[{"scale": 2.0, "style": row_a}, {"scale": 2.0, "id": 3}])
    assert s.pix.pairs == {0: (2, 2.0), 1: (3, 2.0)}
    lps, rows = [], []
    for i, (f0, f1) in enumerate(chunks()):
        if i == 2:
            s.restart([0, 1], style=[crow0, crow1], clip_indices=[50, 51], guide=[{"scale": 1.5, "style": row_b}, {"scale": 1.0}])
            assert s.pix.pairs == {0: (2, 1.5), 1: (3, 1.0)} and list(s.slot_rows) == [0, 0]
        lps.append(s.push(w.mf[:2, f0:f1], logprobs=True, **KW)[1])
        rows.append(w.audioencoder.forward_nlc(w.mf[:2, f0:f1]))
    s.close()
    lp, rows, n = _bits(torch.cat(lps, 1)), torch.cat(rows, 1), SCHED[0] + SCHED[1]
    run = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, logprobs=True)
    out = w.generator.run(np.array([1], np.int64), rows[0:1, :n], clip_index0=CLIP0, guide=[{"scale": 2.0, "style": row_a}], **run)
    assert np.array_equal(lp[0, :n], _bits(out[2])[0]), "a shadow's style row from the open entry"
    plain = w.generator.run(np.array([1], np.int64), rows[0:1, :n], clip_index0=CLIP0, **run)
    assert not np.array_equal(_bits(plain[2]), _bits(out[2]))
    out = w.generator.run(np.array([1], np.int64), rows[0:1, n:], clip_index0=50, style=[crow0], guide=[{"scale": 1.5, "style": row_b}], **run)
    assert np.array_equal(lp[0, n:], _bits(out[2])[0]), "a shadow's style row from the restart entry"
    out = w.generator.run(np.array([0], np.int64), rows[1:2, n:], clip_index0=51, style=[crow1], **run)
    assert np.array_equal(lp[1, n:], _bits(out[2])[0]), "a shadow that took its clip's own weight row changes no bit"
    with pytest.raises(ValueError, match="guide of clip 0: the clip was opened without a shadow"):
        w.open_stream(torch.tensor([1]), 1, cap).restart(0, 1, guide=2.0)


# ---- seamless, wav-fed and long sessions: `generate_batch(..., guide=)` on the whole audio is the yardstick ----------------------------------
import os            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

T_S = 120
GB_IDS = np.array(IDS, np.int64)
SEAMLESS_SCHEDULES = {"16s": (16,) * 7 + (8,), "40s": (40, 40, 40), "with-7": (33, 7, 40, 40)}


def _ubits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def sw(golden):
    """The `pix_small` PixelCNN between an audio encoder and two VQ nets of 128 hidden channels (tests/test_gpu_seamless.py, `small`), 3
    clips of 120 frames, the recording clip 0's shadow hears, and the one-shot guided results per drawing mode."""
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
    w.mf = torch.from_numpy(synth.mfcc_features(611, 3, 160)).cuda()
    w.ms = torch.from_numpy(synth.mfcc_features(612, 1, 160)[0]).cuda()
    w.u = (0.999 * np.random.default_rng(6).random((3, 40, 2))).astype(np.float32)
    w.ref = {}
    return w


def sdraw(mode, u=None):
    if mode == "uniforms":
        return dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u)
    return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=5)


def whole(w, mode, T=T_S):
    """`generate_batch(..., guide=)` on the first T frames -> (codes, pose bits, log-probability bits), made once."""
    if (mode, T) not in w.ref:
        guide = [{"scale": 2.0, "id": 2, "mfcc": w.ms[:T]}, {"scale": 2.0, "id": 3}, None]
        out = w.generate_batch(w.mf[:, :T], GB_IDS, logprobs=True, guide=guide, **sdraw(mode, w.u[:, :T // 4]))
        plain = w.generate_batch(w.mf[:, :T], GB_IDS, **sdraw(mode, w.u[:, :T // 4]))
        assert (_ubits(out[0])[0] != _ubits(plain[0])[0]).any() and (_ubits(out[0])[1] != _ubits(plain[0])[1]).any(), "guidance moved nothing"
        assert np.array_equal(_ubits(out[0])[2], _ubits(plain[0])[2])
        w.ref[(mode, T)] = tuple(_ubits(o).copy() for o in out)
    return w.ref[(mode, T)]


def seamless(w, sched, mode, T=T_S):
    """The clips through a guided seamless session in the pushes of `sched`, then the flush -> (codes, poses, log-probabilities, the
    session's state bytes and graph counts after every call)."""
    st = w.open_stream(GB_IDS, 3, max(sched), seamless=True, guide=GUIDE)
    parts, at, track = [], 0, []
    for t in tuple(sched) + (None,):
        n, m = st.plan(0 if t is None else t, flush=t is None)
        d = sdraw(mode, np.ascontiguousarray(w.u[:, st.code_rows:st.code_rows + n]))
        out = (st.flush(**d, return_codes=True, logprobs=True) if t is None else
               st.push(w.mf[:, at:at + t], **d, return_codes=True, logprobs=True, guide=[{"mfcc": w.ms[at:at + t]}, None, None]))
        assert tuple(out[0].shape) == (3, m, 129) and tuple(out[1].shape) == (3, n, 2) and tuple(out[2].shape) == (3, n, 2)
        parts.append([_ubits(o) for o in out])
        at += t or 0
        track.append((st.state_bytes, st.graph_captures()))
    assert st.frames_in == T and st.code_rows == T // 4 and st.frames == 4 * (T // 4)
    st.close()
    poses, codes, lp = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
    return codes, poses, lp, track


@pytest.mark.parametrize("mode", ["philox", "uniforms"])
@pytest.mark.parametrize("sched", list(SEAMLESS_SCHEDULES))
def test_a_guided_seamless_session_returns_the_one_shot_guided_bits(sw, sched, mode):
    codes, poses, lp, track = seamless(sw, SEAMLESS_SCHEDULES[sched], mode)
    ref = whole(sw, mode)
    assert np.array_equal(codes, ref[0]), f"codes differ first at row {int(np.argwhere(codes != ref[0])[:, 1].min())}"
    assert np.array_equal(poses, ref[1]) and np.array_equal(lp, ref[2])
    assert len({b for b, _ in track}) == 1, "state_bytes moved"


def test_the_same_with_every_conv_stack_lowered():
    """TS_CONV_WINO=1 (read once per process -> a child process): the audio encoder's reach is 14 rows there."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "test_a_guided_seamless_session_returns_the_one_shot_guided_bits"], env=dict(os.environ, TS_CONV_WINO="1"),
                       capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout, r.stdout[-500:]


def test_state_bytes_and_graph_count_stand_still_over_20_pushes(sw):
    codes, poses, lp, track = seamless(sw, (8,) * 20, "philox", T=160)
    ref = whole(sw, "philox", T=160)
    assert np.array_equal(codes, ref[0]) and np.array_equal(poses, ref[1]) and np.array_equal(lp, ref[2])
    assert len({b for b, _ in track}) == 1, track
    assert track[11][1] == track[19][1] > 0, [c for _, c in track]      # pushes 12 .. 20 capture nothing (the flush runs another row count)


def test_generate_long_passes_guide_through(sw):
    guide = [{"scale": 2.0, "id": 2, "mfcc": sw.ms[:T_S]}, {"scale": 2.0, "id": 3}, None]
    codes, poses = sw.generate_long(sw.mf[:, :T_S], GB_IDS, chunk_frames=36, guide=guide, **sdraw("philox"))
    ref = whole(sw, "philox")
    assert np.array_equal(_ubits(codes), ref[0]) and np.array_equal(_ubits(poses), ref[1])
    with pytest.raises(ValueError, match="guide of clip 0: mfcc must have the clip's own shape"):
        sw.generate_long(sw.mf[:, :T_S], GB_IDS, guide=[{"scale": 1.0, "mfcc": sw.ms[:50]}, None, None])


def test_a_wav_fed_session_takes_id_guidance(sw):
    from talkshow_amd.modules import MFCC
    N = 65000
    wav = (0.1 * torch.randn((2, N), generator=torch.Generator().manual_seed(4))).cuda()
    m = MFCC(16000, 22000, 30)
    mf, ids, guide = m(wav), np.array([1, 0], np.int64), [{"scale": 2.0, "id": 2}, None]
    ref = tuple(_ubits(o) for o in sw.generate_batch(mf, ids, logprobs=True, guide=guide, **sdraw("philox")))
    plain = sw.generate_batch(mf, ids, **sdraw("philox"))
    assert (ref[0][0] != _ubits(plain[0])[0]).any()
    st = sw.open_stream(ids, 2, 48, seamless=True, wav_sr=16000, wav_db=m.peak_db(wav), max_samples=30000, guide=guide)
    parts, at = [], 0
    for n in [30000, 20000, 15000, None]:
        out = (st.flush(return_codes=True, logprobs=True, **sdraw("philox")) if n is None else
               st.push_wav(wav[:, at:at + n], return_codes=True, logprobs=True, guide=[2.0, None] if at else None, **sdraw("philox")))
        at += n or 0
        parts.append([_ubits(o) for o in out])
    st.close()
    poses, codes, lp = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
    assert np.array_equal(codes, ref[0]) and np.array_equal(poses, ref[1]) and np.array_equal(lp, ref[2])
    with pytest.raises(NotImplementedError, match="guide of clip 0: a wav-fed session takes shadows WITHOUT audio of their own"):
        sw.open_stream(ids, 2, 48, seamless=True, wav_sr=16000, guide=[{"scale": 2.0, "audio": True}, None])
