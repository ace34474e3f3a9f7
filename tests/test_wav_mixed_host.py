"""Host-side logic of the pass from recordings to 265-d rows (no GPU): the table arithmetic that plans a mixed pass without reading
anything back from the device, the sort and its inverse, the mixed assembly stated in numpy against the oracle, and the argument
checks of the Python entries, which all run before the first device call.
"""
import math

import numpy as np
import pytest
import torch

from oracle import talkshow_oracle as O
from talkshow_amd import frontend
from talkshow_amd.pose_index import lower_pose_block

# 16 kHz sample counts: the pair that straddles a frame boundary (5872 -> 8074 = 11 * 734 resampled samples -> 12 rows; 5871 -> 11 rows),
# the shortest clip the STFT takes (746 -> 1026 > 1024), one second, odd counts, two equal
NS = [16000, 746, 5872, 5871, 1602, 8001, 8000, 12345, 16000, 2935]


def test_tables_closed_forms():
    t = frontend.mixed_tables(NS, 16000)
    for k, n in enumerate(NS):
        n22 = math.ceil(n * 11 / 8)
        assert t["n_resampled"][k] == n22
        assert t["mfcc_rows"][k] == n22 // 734 + 1
        assert t["code_rows"][k] == (n22 // 734 + 1) // 4
        assert t["pose_frames"][k] == 4 * ((n22 // 734 + 1) // 4)
        assert t["n16"][k] == n
        assert t["face_frames"][k] == n * 30 // 16000
    assert t["n_resampled"][2] == 8074 == 11 * 734 and t["mfcc_rows"][2] == 12 and t["mfcc_rows"][3] == 11
    t15 = frontend.mixed_tables(NS, 16000, fps=15)
    assert t15["mfcc_rows"].tolist() == [math.ceil(n * 11 / 8) // 1467 + 1 for n in NS]
    t44 = frontend.mixed_tables([2300, 9000, 44100], 44100)
    assert t44["n_resampled"].tolist() == [math.ceil(n * 220 / 441) for n in (2300, 9000, 44100)]
    assert t44["n16"].tolist() == [math.ceil(n * 16000 / 44100) for n in (2300, 9000, 44100)]
    assert t44["face_frames"].tolist() == [math.ceil(n * 16000 / 44100) * 30 // 16000 for n in (2300, 9000, 44100)]
    same = frontend.mixed_tables(NS, 22000)
    assert same["n_resampled"].tolist() == NS
    assert all(v.dtype == np.int64 and v.shape == (len(NS),) for v in t.values())
    with pytest.raises(ValueError):
        frontend.mixed_tables([100, -1], 16000)
    with pytest.raises(ValueError):
        frontend.mixed_tables(NS, 16000, fps=25)


@pytest.mark.parametrize("sr_in", [16000, 22050, 22000])
def test_tables_against_the_numpy_twins(sr_in):
    """The shapes `resample_sinc_hann` and `mfcc` produce on the same lengths."""
    ns = [5872, 5871, 746, 2935, 8001] if sr_in == 16000 else [3000, 4567, 9001]
    t = frontend.mixed_tables(ns, sr_in)
    rng = np.random.default_rng(0)
    for k, n in enumerate(ns):
        x = frontend.resample_sinc_hann(rng.standard_normal((1, n)).astype(np.float32), sr_in, 22000)
        assert x.shape == (1, t["n_resampled"][k])
        assert frontend.mfcc(x[0], 22000).shape == (64, t["mfcc_rows"][k])
        if sr_in != 16000:
            assert frontend.resample_kaiser_best(np.zeros(n, np.float32), sr_in, 16000).shape == (t["n16"][k],)


def test_sort_gives_the_body_pass_its_order_and_unsorts():
    rng = np.random.default_rng(3)
    ns = rng.integers(746, 40000, 50).tolist() + NS
    from nets.smplx_body_pixel import mixed_pass_order
    order, inverse = mixed_pass_order(ns)
    assert sorted(order) == list(range(len(ns)))
    s = [ns[i] for i in order]
    assert all(a >= b for a, b in zip(s, s[1:]))
    assert all(i < j for i, j, a, b in zip(order, order[1:], s, s[1:]) if a == b)            # stable: ties in submission order
    for sr in (16000, 22050, 44100):
        for fps in (15, 30):
            rows = frontend.mixed_tables(s, sr, fps=fps)["mfcc_rows"]
            assert (np.diff(rows) <= 0).all()                                                # non-increasing T_b: what the body pass demands
    assert [order[inverse[b]] for b in range(len(ns))] == list(range(len(ns)))
    assert [s[inverse[b]] for b in range(len(ns))] == ns                                     # the un-sort


def _assemble_mixed(body, tb, face, tf, lp):
    """The mixed assembly as the header states it: row t < tf[b] takes body frame min(t, tb[b] - 1); rows beyond are 0."""
    B, Tf = face.shape[0], face.shape[1]
    out = np.zeros((B, Tf, 265), np.float32)
    for b in range(B):
        t = np.arange(tf[b])
        bt = np.minimum(t, tb[b] - 1)
        p = np.concatenate([face[b, t, :3], body[b, bt], face[b, t, 3:]], axis=-1)
        l = np.broadcast_to(lp, (tf[b], 33))
        out[b, :tf[b]] = np.concatenate([p[:, :3], l[:, :15], p[:, 3:6], l[:, 15:21], p[:, 6:9], l[:, 21:27], p[:, 9:12], l[:, 27:], p[:, 12:]], -1)
    return out


@pytest.mark.parametrize("stand", [False, True])
def test_mixed_assembly_statement_against_the_oracle(stand):
    pairs = [(8, 12), (12, 12), (16, 9), (4, 1), (4, 30), (1, 5)]                            # tb < tf, tb = tf, tb > tf
    rng = np.random.default_rng(1)
    Tb, Tf = max(p[0] for p in pairs), max(p[1] for p in pairs)
    body = rng.standard_normal((len(pairs), Tb, 129)).astype(np.float32)
    face = rng.standard_normal((len(pairs), Tf, 103)).astype(np.float32)
    for b, (tb, tf) in enumerate(pairs):                                                     # what lies beyond a clip must not matter
        body[b, tb:] = np.nan
        face[b, tf:] = np.nan
    lp = lower_pose_block(stand)
    got = _assemble_mixed(body, [p[0] for p in pairs], face, [p[1] for p in pairs], lp)
    for b, (tb, tf) in enumerate(pairs):
        want = O.assemble_full(body[b:b + 1, :tb], face[b:b + 1, :tf], lp)[0]
        assert np.array_equal(got[b, :tf], want)
        assert not got[b, tf:].any()


def test_argument_errors_need_no_device():
    """Everything the list entries refuse is refused before their first device call."""
    from nets.smplx_body_pixel import TrainWrapper
    from talkshow_amd import parallel
    from talkshow_amd.modules import MFCC, resample_kaiser_clips
    ok = [np.zeros(16000, np.float32), torch.zeros(8000)]
    assert frontend.check_recordings(ok, "t").tolist() == [16000, 8000]
    for wavs in ([], np.zeros((2, 16000), np.float32), [np.zeros((1, 16000), np.float32)], [ok[0], np.zeros((2, 3))], [np.zeros(0)], "a.wav"):
        with pytest.raises(ValueError):
            MFCC.run_clips(None, wavs)
        with pytest.raises(ValueError):
            MFCC.resample_clips(None, wavs)
        with pytest.raises(ValueError):
            resample_kaiser_clips(wavs, 22050, 16000)
        with pytest.raises(ValueError):
            TrainWrapper.generate_clips_from_wav(None, wavs, 16000, [0])
        with pytest.raises(ValueError):
            parallel.whole_body_clips(None, None, wavs, 16000, [0], None)
    for ids in ([0, 1, 2], [], np.zeros(3, np.int64)):                                       # wrong number of ids
        with pytest.raises(ValueError):
            TrainWrapper.generate_clips_from_wav(None, ok, 16000, ids)
        with pytest.raises(ValueError):
            parallel.whole_body_clips(None, None, ok, 16000, ids, None)
    with pytest.raises(ValueError):
        TrainWrapper.generate_clips_from_wav(None, ok, 16000, [0, 1], clip_indices=[5])
