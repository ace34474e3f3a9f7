"""Per-clip sampling controls through the body decode (`ts_pixelcnn_generate_ctl`, `ts_body_pixel_infer_mixed_ctl`; `GatedPixelCNN.run`,
`TrainWrapper.generate_clips`, `generate_clips_from_wav`, `parallel.whole_body_clips` with `sampling=`).

The contract: a draw is a pure function of the clip's logits row, the clip's record and the clip's uniform — so every comparison is
EQUALITY (codes and poses `array_equal`), and a clip's result does not depend on the records its neighbours carry.  The PixelCNN is the
small network of the quick tests (input_dim 256, dim 64, n_layers 3) inside the shipped wrapper.  Every test that passes `sampling=` fails
on a build without the feature (the keyword and the entries do not exist there).
"""
import os

import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S
from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(input_dim=256, dim=64, n_layers=3)
ROWS = [20, 17, 17, 9, 8, 3]                       # code rows of the six clips: two chunks and a half, ties, a clip shorter than a chunk
RECS = [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.7, 1.0, 12), (0.5, 0.5, 40), (1.0, 1.0, 0), (4.0, 0.95, 64)]
NEUTRAL = (1.0, 1.0, 0)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def pix():
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], 4, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=11, **DIMS)))
    return m


@pytest.fixture(scope="module")
def w(pix):
    """The shipped wrapper (audio encoder, VQ decoders) around the small code predictor."""
    import bench
    wr = bench.build_models(0, seed=7)[0]
    wr.generator = pix
    return wr


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(21)
    order = rng.permutation(len(ROWS))               # submitted shuffled: the Python layer sorts and un-sorts
    rows = [ROWS[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(3000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    recs = [RECS[i] for i in order]
    return rows, mf, ids, recs


def _same(a, b):
    return all(np.array_equal(_np(x[0]), _np(y[0])) and np.array_equal(_np(x[1]), _np(y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("mode_name", ["philox", "uniforms"])
def test_neutral_records_change_nothing(w, clips, mode_name):
    from talkshow_amd import _lib
    rows, mf, ids, _ = clips
    mode = _lib.TS_SAMPLE_PHILOX if mode_name == "philox" else _lib.TS_SAMPLE_UNIFORMS
    rng = np.random.default_rng(4)
    u = [rng.random((h, 2)).astype(F32) for h in rows] if mode == _lib.TS_SAMPLE_UNIFORMS else None
    kw = dict(mode=mode, uniforms=u, seed=77, clip_index0=30)
    plain = w.generate_clips(mf, ids, **kw)
    for sampling in (NEUTRAL, [NEUTRAL] * len(rows), [None, {"temperature": 1.0}, (1.0, 1.0, 256), (1.0, 1.0, 9999), {}, NEUTRAL]):
        assert _same(plain, w.generate_clips(mf, ids, sampling=sampling, **kw))
    hot = w.generate_clips(mf, ids, sampling=(0.5, 0.9, 0), **kw)
    assert not _same(plain, hot)                     # and a record that is not neutral does change the draws


def test_plain_pass_keeps_its_graphs(w):
    """A pass without controls replays the graphs it had: same launches per replay, no capture on its next run, whatever ran in between."""
    import ctypes as C
    from talkshow_amd import _lib
    lib = _lib.load()
    B, T = 4, 48
    mf = torch.from_numpy(synth.mfcc_features(9, B, T)).cuda()
    ids = np.arange(B, dtype=np.int64) % 4
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=5)
    for _ in range(3):                               # the third sighting makes the shape hot: a whole-call graph
        plain = w.generate_batch(mf, ids, **kw)

    def stats():
        n, f = C.c_int64(), C.c_double()
        _lib.check(lib.ts_pixelcnn_graph_stats(w.generator.handle(), _lib.stream_ptr(), B, T // 4, _lib.TS_SAMPLE_PHILOX, C.byref(n), C.byref(f)))
        return n.value, f.value
    before = stats()
    again = w.generate_batch(mf, ids, **kw)
    caps = w.generator.graph_captures()
    ctl = w.generate_batch(mf, ids, sampling=NEUTRAL, **kw)          # the mixed entry with equal lengths: its own (controls) graphs
    assert w.generator.graph_captures() > caps
    assert np.array_equal(_np(ctl[0]), _np(plain[0])) and np.array_equal(_np(ctl[1]), _np(plain[1]))
    caps = w.generator.graph_captures()
    last = w.generate_batch(mf, ids, **kw)
    assert w.generator.graph_captures() == caps and stats() == before
    assert np.array_equal(_np(last[0]), _np(again[0])) and np.array_equal(_np(last[0]), _np(plain[0]))


def test_every_draw_rederived_from_the_step_logits(pix):
    """B = 4, H = 10 (the 8-row chunk boundary is crossed), four different records, injected uniforms: every code equals the twin's draw
    from the device's own step logits; the graph path (no logits) gives the same codes."""
    from talkshow_amd import _lib
    B, H, V = 4, 10, DIMS["input_dim"]
    rng = np.random.default_rng(6)
    aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(synth.speaker_ids(B)).cuda()
    u = rng.random((B, H, 2)).astype(F32)
    u[0, 0, 0], u[1, 3, 1], u[2, 9, 0] = 0.0, 1.0 - 2.0 ** -24, 0.0
    recs = [(0.7, 0.9, 0), (1.0, 1.0, 1), (2.5, 0.6, 30), (1.0, 0.999, 5)]
    codes, lg = pix.run(label, aud, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs, want_logits=True)
    codes, lg = _np(codes), _np(lg)
    for b in range(B):
        idx, kept = S.sample_ctl(lg[b].reshape(-1, V), u[b].reshape(-1), [recs[b]] * (2 * H))
        np.testing.assert_array_equal(codes[b].reshape(-1), idx, err_msg=f"clip {b}, record {recs[b]}")
    np.testing.assert_array_equal(codes[1], _np(pix.run(label, aud, mode=_lib.TS_SAMPLE_GREEDY)[0])[1])      # top_k = 1: the greedy codes
    for _ in range(3):                               # chunk graphs, then (third sighting) the whole-call graph
        np.testing.assert_array_equal(_np(pix.run(label, aud, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs)[0]), codes)
    one = _np(pix.run(label, aud, mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u, sampling=recs[2])[0])               # one record for all clips
    np.testing.assert_array_equal(one[2], codes[2])
    assert not np.array_equal(one[0], codes[0])


def test_mixed_pass_each_clip_equals_the_clip_alone(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    n = len(rows)
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123)
    res = w.generate_clips(mf, ids, sampling=recs, clip_index0=50, **kw)
    for b in range(n):
        alone = w.generate_clips([mf[b]], ids[b:b + 1], sampling=[recs[b]], clip_indices=[50 + b], **kw)[0]
        assert res[b][0].shape == (rows[b], 2)
        assert np.array_equal(_np(res[b][0]), _np(alone[0])), f"codes of clip {b} ({rows[b]} rows, record {recs[b]})"
        assert np.array_equal(_np(res[b][1]), _np(alone[1])), f"poses of clip {b} ({rows[b]} rows, record {recs[b]})"
    g = recs.index((1.0, 1.0, 1))                    # top_k = 1: the clip's greedy codes
    greedy = w.generate_batch(mf[g][None], ids[g:g + 1], mode=_lib.TS_SAMPLE_GREEDY)[0]
    assert np.array_equal(_np(res[g][0]), _np(greedy)[0])
    a, b = 2, 3                                      # swapping two neighbours' records changes those two clips only
    swapped = list(recs)
    swapped[a], swapped[b] = recs[b], recs[a]
    res2 = w.generate_clips(mf, ids, sampling=swapped, clip_index0=50, **kw)
    for c in range(n):
        same = np.array_equal(_np(res[c][0]), _np(res2[c][0])) and np.array_equal(_np(res[c][1]), _np(res2[c][1]))
        assert same == (c not in (a, b)), f"clip {c} after swapping the records of clips {a} and {b}"


def test_batches_generate_and_infer_on_audio_carry_the_records(w, pix):
    """The other entries that take records: `generate_batches(..., sampling=)` (two batches of equal and of different lengths) against
    `generate_clips` on the same clips, `GatedPixelCNN.generate(..., sampling=)` against `run`, and `infer_on_audio(temperature=, top_k=,
    top_p=)` against `generate_batch(..., sampling=)`."""
    from talkshow_amd import _lib
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=41, clip_index0=7)
    for T0, T1 in ((48, 48), (48, 36)):
        m0, m1 = torch.from_numpy(synth.mfcc_features(70, 2, T0)).cuda(), torch.from_numpy(synth.mfcc_features(71, 3, T1)).cuda()
        ids0, ids1 = np.asarray([0, 1], np.int64), np.asarray([2, 3, 0], np.int64)
        recs = [(0.8, 0.9, 0), (1.0, 1.0, 1), None, (2.0, 1.0, 10), (0.6, 0.7, 30)]
        got = w.generate_batches([m0, m1], [ids0, ids1], sampling=recs, **kw)
        ref = w.generate_clips(list(m0.unbind(0)) + list(m1.unbind(0)), np.concatenate([ids0, ids1]), sampling=recs, **kw)
        flat = [(c[i], p[i]) for c, p in got for i in range(c.shape[0])]
        assert [tuple(c.shape) for c, _ in got] == [(2, T0 // 4, 2), (3, T1 // 4, 2)]
        assert all(np.array_equal(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1])) for a, b in zip(flat, ref))
        plain = w.generate_batches([m0, m1], [ids0, ids1], **kw)
        assert np.array_equal(_np(plain[1][0][0]), _np(got[1][0][0]))          # the clip with the neutral record
        assert not np.array_equal(_np(plain[0][0]), _np(got[0][0]))
    B, H = 3, 9
    rng = np.random.default_rng(12)
    rows = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(F32)).cuda()
    label = torch.from_numpy(synth.speaker_ids(B)).cuda()
    recs = [(0.7, 0.9, 0), (1.0, 1.0, 1), (3.0, 1.0, 20)]
    amap = rows.transpose(1, 2).unsqueeze(-1).expand(B, 256, H, 2)
    a = pix.generate(label, shape=(H, 2), batch_size=B, aud_feat=amap, seed=5, sampling=recs)
    b = pix.run(label, rows, mode=_lib.TS_SAMPLE_PHILOX, seed=5, sampling=recs)[0]
    assert np.array_equal(_np(a), _np(b)) and not np.array_equal(_np(a), _np(pix.generate(label, shape=(H, 2), batch_size=B, aud_feat=amap, seed=5)))
    mf = synth.mfcc_features(90, 1, 60)[0]                                      # (T, 64) rows, as tests/test_gpu_parity.py hands them over
    out = w.infer_on_audio(mf, id=torch.tensor([1]).cuda(), fps=30, B=2, seed=3, temperature=0.8, top_k=40, top_p=0.9)
    ref = w.generate_batch(np.repeat(mf[None], 2, 0), np.asarray([1, 1], np.int64), mode=_lib.TS_SAMPLE_PHILOX, seed=3,
                           sampling={"temperature": 0.8, "top_k": 40, "top_p": 0.9})[1]
    assert np.array_equal(out, _np(ref))
    assert not np.array_equal(out, w.infer_on_audio(mf, id=torch.tensor([1]).cuda(), fps=30, B=2, seed=3))


def test_queued_passes_keep_their_tables_and_capture_nothing(w, clips):
    """Three passes with three tables queued on one stream without a synchronisation in between: each equals the same pass run alone (the
    table rides the stream, not a host buffer).  A repeated pass captures nothing; another table on the same shapes captures nothing."""
    from talkshow_amd import _lib
    rows, mf, ids, recs = clips
    tables = [recs, recs[1:] + recs[:1], [(1.3, 0.8, 20)] * len(rows)]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3)
    alone = []
    for t in tables:
        alone.append([(_np(c), _np(p)) for c, p in w.generate_clips(mf, ids, sampling=t, **kw)])
        torch.cuda.synchronize()
    caps = w.generator.graph_captures()
    queued = [w.generate_clips(mf, ids, sampling=t, **kw) for t in tables]
    torch.cuda.synchronize()
    assert w.generator.graph_captures() == caps
    for q, a in zip(queued, alone):
        assert all(np.array_equal(_np(x[0]), y[0]) and np.array_equal(_np(x[1]), y[1]) for x, y in zip(q, a))
    assert any(not np.array_equal(alone[0][b][0], alone[1][b][0]) for b in range(len(rows)))
    w.generate_clips(mf, ids, sampling=[(2.0, 0.7, 3)] * len(rows), **kw)
    w.generate_clips(mf, ids, sampling=recs, **kw)
    assert w.generator.graph_captures() == caps


def test_recordings_carry_their_records(w):
    """`parallel.whole_body_clips(..., sampling=[...])` on four short recordings of different lengths: the body columns of a recording's
    265-d rows are the poses of `generate_clips_from_wav` on the recording alone with its record."""
    import argparse
    import json

    import nets
    from talkshow_amd import parallel
    from talkshow_amd.config import Object
    cfg = json.load(open(os.path.join(REPO, "config", "face.json")))
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    ns = [5872, 16000, 1602, 8001]
    wavs = [synth.wav16(11000 + k, 1, n)[0] for k, n in enumerate(ns)]
    ids = (np.arange(len(ns)) % 4).astype(np.int64)
    recs = [(0.8, 0.9, 0), None, {"top_k": 1}, (2.0, 0.95, 50)]
    out = parallel.whole_body_clips(w, face, wavs, 16000, ids, None, seed=9, clip_index0=20, sampling=recs)
    body_cols = np.r_[18:21, 27:30, 36:39, 45:165]               # where the 129 body + hand values sit in a 265-d row
    changed = 0
    for b in range(len(ns)):
        codes, poses = w.generate_clips_from_wav([wavs[b]], 16000, ids[b:b + 1], seed=9, clip_indices=[20 + b], sampling=recs[b])[0]
        poses, got = _np(poses), _np(out[b])[:, body_cols]
        t = np.minimum(np.arange(got.shape[0]), poses.shape[0] - 1)     # aligned to the face length: last frame repeated, or trimmed
        assert np.array_equal(got, poses[t]), f"recording {b} ({ns[b]} samples, record {recs[b]})"
        plain = w.generate_clips_from_wav([wavs[b]], 16000, ids[b:b + 1], seed=9, clip_indices=[20 + b])[0]
        changed += not np.array_equal(_np(plain[0]), _np(codes))
    assert changed >= 2                                           # the records reached the sampler


def test_errors_before_any_launch(w, pix, clips):
    from talkshow_amd import _lib
    from talkshow_amd.modules import GatedPixelCNN
    rows, mf, ids, recs = clips
    caps = w.generator.graph_captures()
    bad = list(recs)
    bad[4] = (0.0, 1.0, 0)
    with pytest.raises(ValueError, match="clip"):
        w.generate_clips(mf, ids, sampling=bad)
    srt = sorted(range(len(rows)), key=lambda b: (-mf[b].shape[0], b)).index(4)      # the C entry names the clip's slot in the sorted pass
    with pytest.raises(ValueError, match=f"clip {srt}"):
        w.generate_clips(mf, ids, sampling=bad)
    with pytest.raises(ValueError, match="top_k = 1"):
        w.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_GREEDY, sampling=recs)
    with pytest.raises(ValueError, match="one per clip"):
        w.generate_clips(mf, ids, sampling=recs[:3])
    aud = torch.zeros((2, 4, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="clip 1"):
        pix.run(np.zeros(2, np.int64), aud, sampling=[NEUTRAL, (1.0, 2.0, 0)])
    with pytest.raises(ValueError, match="top_k = 1"):
        pix.run(np.zeros(2, np.int64), aud, mode=_lib.TS_TEACHER_FORCED, codes=np.zeros((2, 4, 2), np.int64), sampling=NEUTRAL)
    v = GatedPixelCNN(DIMS["input_dim"], DIMS["dim"], DIMS["n_layers"], 4, True, False)
    with pytest.raises(NotImplementedError):
        v.run(np.zeros(2, np.int64), aud, sampling=NEUTRAL)
    # the C entries themselves refuse, too (a host that binds the ABI directly)
    lib = _lib.load()
    arr = (_lib.TsSampling * 2)()
    arr[0].temperature = arr[0].top_p = arr[1].top_p = 1.0
    arr[1].temperature = float("nan")
    label = torch.zeros(2, dtype=torch.int64, device="cuda")
    codes = torch.full((2, 4, 2), -7, dtype=torch.int64, device="cuda")
    args = (pix.handle(), _lib.dptr(label), _lib.dptr(aud), 2, 4)
    tail = (None, 0, 0, _lib.dptr(codes), None, None, None, 0)
    assert lib.ts_pixelcnn_generate_ctl(*args, _lib.TS_SAMPLE_PHILOX, *tail, arr, 2, _lib.stream_ptr()) != 0
    assert "clip 1" in lib.ts_last_error().decode()
    arr[1].temperature = 1.0
    assert lib.ts_pixelcnn_generate_ctl(*args, _lib.TS_SAMPLE_GREEDY, *tail, arr, 2, _lib.stream_ptr()) != 0
    assert "top_k = 1" in lib.ts_last_error().decode()
    torch.cuda.synchronize()
    assert (_np(codes) == -7).all() and w.generator.graph_captures() == caps
