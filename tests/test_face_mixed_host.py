"""Host-side logic of the mixed face pass (no GPU): the attention work list, the masking argument, argument checking.

The library loads without a device; `ts_debug_face_mixed_grid` is host arithmetic only.  The masking argument is the reason a padded,
length-limited batch can equal the clip alone at all: stated here in torch on the CPU, on the operations whose reach crosses a clip's end.
"""
import ctypes as C

import numpy as np
import pytest
import torch

I32P = C.POINTER(C.c_int32)


def grid(frames, heads):
    from talkshow_amd import _lib
    lib = _lib.load()
    fr = np.ascontiguousarray(frames, np.int32)
    n = lib.ts_debug_face_mixed_grid(fr.ctypes.data_as(I32P), len(fr), heads, None, 0)
    assert n > 0
    out = np.full((n, 3), 7, np.int32)
    assert lib.ts_debug_face_mixed_grid(fr.ctypes.data_as(I32P), len(fr), heads, out.ctypes.data_as(I32P), n) == n
    return out


@pytest.mark.parametrize("frames,heads", [([1], 1), ([63, 64, 65], 12), ([1, 63, 64, 65, 300], 3), ([300, 384, 288] * 4, 12),
                                          ([65] * 5, 1), ([129, 1, 1, 1, 1, 1, 1, 1, 1, 64], 1)])
def test_attention_work_list(frames, heads):
    g = grid(frames, heads)
    live = g[g[:, 0] >= 0]
    assert (g[g[:, 0] < 0] == -1).all()
    want = {(b, h, q) for b, t in enumerate(frames) for h in range(heads) for q in range((t + 63) // 64)}
    got = [tuple(r) for r in live.tolist()]
    assert len(got) == len(set(got)) and set(got) == want             # every tile with 64 q < frames[b] exactly once, no other
    assert all(64 * q < frames[b] for b, h, q in got)
    lane = {}
    for i, (b, h, q) in enumerate(g.tolist()):
        if b >= 0:
            lane.setdefault((b, h), set()).add(i % 8)
    assert all(len(v) == 1 for v in lane.values())                    # one (clip, head) = one residue mod 8 = one XCD
    total = heads * sum((t + 63) // 64 for t in frames)
    assert len(live) == total and len(g) % 8 == 0
    # padding: only what dealing whole (clip, head) queues to 8 lanes needs — the longest lane is the greedy (longest first) bound
    longest = max((t + 63) // 64 for t in frames)
    assert len(g) // 8 <= max(longest, -(-total // 8) + longest - 1)


def test_attention_work_list_hand_checked():
    # 5 clips x 3 heads = 15 (clip, head) queues, not a multiple of 8; tiles 1, 1, 1, 2, 5 per head: 30 tiles; the three 5-tile queues
    # set the lane length: 40 ids
    g = grid([1, 63, 64, 65, 300], 3)
    assert len(g) == 40
    assert [tuple(r) for r in g[:3].tolist()] == [(4, 0, 0), (4, 1, 0), (4, 2, 0)]          # longest first, one lane each
    assert [tuple(r) for r in g[8:11].tolist()] == [(4, 0, 1), (4, 1, 1), (4, 2, 1)]        # ... back to back in their lanes
    # equal lengths: the uniform kernel's order (queue z on lane z % 8, tiles back to back)
    u = grid([130] * 2, 12)
    for i, (b, h, q) in enumerate(u.tolist()):
        slot, x = divmod(i, 8)
        assert (b * 12 + h, q) == ((slot // 3) * 8 + x, slot % 3)


def test_attention_work_list_rejects_bad_tables():
    from talkshow_amd import _lib
    lib = _lib.load()
    for fr in ([0], [5, -1], [65537]):
        a = np.asarray(fr, np.int32)
        assert lib.ts_debug_face_mixed_grid(a.ctypes.data_as(I32P), len(a), 12, None, 0) == -1
    a = np.asarray([100], np.int32)
    out = np.zeros((4, 3), np.int32)
    assert lib.ts_debug_face_mixed_grid(a.ctypes.data_as(I32P), 1, 12, out.ctypes.data_as(I32P), 4) == -1   # 24 entries do not fit 4


def test_masking_argument():
    """Zero rows beyond a clip's end + keys limited to the clip = the clip alone, for the operations that look across rows: the k = 3 convs
    of the heads, the k = 128 grouped positional conv (padding 64), and soft-max attention."""
    torch.manual_seed(0)
    lens, T, Cc = [5, 70, 131], 131, 32
    x = torch.zeros(len(lens), Cc, T, dtype=torch.float64)
    for b, t in enumerate(lens):
        x[b, :, :t] = torch.randn(Cc, t, dtype=torch.float64)
    w3, w128 = torch.randn(Cc, Cc, 3, dtype=torch.float64), torch.randn(Cc, Cc // 4, 128, dtype=torch.float64)
    y3 = torch.nn.functional.conv1d(x, w3, padding=1)
    y128 = torch.nn.functional.conv1d(x, w128, padding=64, groups=4)[:, :, :T]
    q, k, v = (torch.randn(len(lens), T, 16, dtype=torch.float64) for _ in range(3))
    for b, t in enumerate(lens):
        a3 = torch.nn.functional.conv1d(x[b:b + 1, :, :t], w3, padding=1)
        a128 = torch.nn.functional.conv1d(x[b:b + 1, :, :t], w128, padding=64, groups=4)[:, :, :t]
        assert torch.equal(y3[b, :, :t], a3[0]) and torch.equal(y128[b, :, :t], a128[0])
        s = (q[b, :t] @ k[b, :t].T) * 0.25                          # keys limited to the clip: the scores of the clip alone
        alone = torch.softmax(s, -1) @ v[b, :t]
        full = (q[b] @ k[b].T) * 0.25
        full[:, t:] = float("-inf")                                  # the same limit stated as a mask on the padded batch
        assert torch.allclose((torch.softmax(full, -1) @ v[b])[:t], alone, rtol=0, atol=1e-14)


def _gen():
    from talkshow_amd.modules import FaceGenerator
    return FaceGenerator(n_layers=1)


def test_run_clips_argument_checking():
    """`_check_clips` is everything `run_clips` does before its first device call."""
    g = _gen()
    ok = [np.zeros(16000, np.float32), torch.zeros(8000), np.zeros(534, np.float64)]
    clips, ns, fr, ids = g._check_clips(ok, None, None)
    assert ns.tolist() == [16000, 8000, 534] and fr.tolist() == [30, 15, 1] and ns.dtype == fr.dtype == np.int32
    assert g._check_clips(ok[:2], None, None)[2].tolist() == [30, 15]
    assert ids.shape == (3, 4) and not ids.any() and all(c.dtype == np.float32 for c in clips)
    assert g._check_clips(ok, np.eye(4)[[1]], [7, 7, 1])[3].tolist() == [[0, 1, 0, 0]] * 3
    for wavs, idv, frames in [([], None, None), (np.zeros((2, 16000), np.float32), None, None), ([np.zeros((1, 16000))], None, None),
                              ([np.zeros(399)], None, None), (ok, None, [30, 15]), (ok, None, [30, 15, 0]), (ok, None, [30.0, 15.0, 1.0]),
                              (ok, np.zeros((2, 4)), None), (ok, np.zeros((3, 5)), None), (ok, np.zeros(4), None),
                              ([np.zeros(533)], None, None)]:                     # 533 samples: no output frame by default
        with pytest.raises(ValueError):
            g.run_clips(wavs, idv, frames)                           # raises before any device call: this machine may have no device


def test_generate_clips_argument_checking():
    import argparse
    import json
    import os

    import nets
    from talkshow_amd.config import Object
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(repo, "config", "face.json")))
    w = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(cfg))
    ok = [np.zeros(16000, np.float32), np.zeros(8000, np.float32)]
    for clips, ids, frames in [([], None, None), (ok[0], None, None), ("a.wav", None, None), (ok, [0], None), (ok, [0, 4], None),
                               (ok, [0.0, 1.0], None), (ok, None, [30]), ([np.zeros((2, 8000))], None, None)]:
        with pytest.raises(ValueError):
            w.generate_clips(clips, ids=ids, frames=frames)
