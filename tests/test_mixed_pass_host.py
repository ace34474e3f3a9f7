"""Host side of mixed passes (clips of different lengths in one body pass): the pass planner on hand-checked tables, and the masking
argument the length-masked conv kernels rest on, stated in torch on the CPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

I32P = C.POINTER(C.c_int32)


def _plan(hrows, max_counts=0):
    from talkshow_amd import _lib
    lib = _lib.load()
    h = np.asarray(hrows, np.int32)
    active = np.zeros((int(h[0]) + 7) // 8, np.int32)
    grid = lib.ts_debug_mixed_plan(h.ctypes.data_as(I32P), len(h), max_counts, active.ctypes.data_as(I32P))
    return grid, active.tolist()


def test_sort_permutation_and_inverse():
    from nets.smplx_body_pixel import mixed_pass_order
    lens = [300, 384, 288, 384, 16, 300]
    order, inverse = mixed_pass_order(lens)
    assert order == [1, 3, 0, 5, 2, 4]                        # longest first, ties in submission order
    assert inverse == [2, 0, 4, 1, 5, 3]
    assert [lens[i] for i in order] == [384, 384, 300, 300, 288, 16]
    assert all(order[inverse[b]] == b for b in range(len(lens)))
    assert mixed_pass_order([7]) == ([0], [0])
    assert mixed_pass_order([5, 5, 5]) == ([0, 1, 2], [0, 1, 2])


def test_active_counts_per_chunk():
    # code rows 24, 24, 18, 18, 9, 3: rows [0, 8) all six; [8, 16) the five with more than 8 rows; [16, 24) the four with more than 16
    assert _plan([24, 24, 18, 18, 9, 3]) == (1, [6, 5, 4])
    # the recordings x four ids: 96, 75 and 72 code rows -> 9 chunks of twelve clips (rows 0 .. 71), one of eight (rows 72 .. 79: the 75s
    # and the 96s), two of four (rows 80 .. 95)
    assert _plan([96] * 4 + [75] * 4 + [72] * 4) == (1, [12] * 9 + [8] + [4] * 2)
    assert _plan([5]) == (1, [1])                             # shorter than one chunk
    assert _plan([8, 8]) == (1, [2])                          # exactly one chunk: no empty second one
    assert _plan([9, 8]) == (1, [2, 1])


def test_rounding_at_the_graph_bound():
    # 20 clips of 8 k + 1 rows: chunk k runs 20 - k clips, 20 distinct counts.  Bound 12 -> multiples of 2 (10 distinct), every count
    # rounded UP and never beyond the pass; bound 4 -> multiples of 8, capped at 20
    hrows = [8 * k + 1 for k in range(19, -1, -1)]
    raw = list(range(20, 0, -1))
    assert _plan(hrows, 20) == (1, raw)
    grid, active = _plan(hrows)                               # the library's own bound: 12
    assert grid == 2 and active == [min(20, (n + 1) // 2 * 2) for n in raw] and len(set(active)) == 10
    grid, active = _plan(hrows, 4)
    assert grid == 8 and active == [min(20, (n + 7) // 8 * 8) for n in raw] and len(set(active)) == 3
    assert all(a >= n for a, n in zip(active, raw))
    assert _plan(hrows, 1) == (32, [20] * 20)                 # one count: every chunk carries the whole pass


def test_bad_tables_are_rejected():
    assert _plan([8, 9])[0] == -1                             # not sorted
    assert _plan([8, 0])[0] == -1                             # an empty clip


# ---- the masking argument ------------------------------------------------------------------------------------------------------------
def _stack(seed, c=8):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(k3=(r(c, c, 3), r(c)), down=(r(c, c, 4), r(c)), mid=(r(c, c, 3), r(c)), up=(r(c, c, 4), r(c)), out=(r(c, c, 3), r(c)))


def _run(p, x, lens=None):
    """k3 -> k4 s2 (down) -> k3 -> transposed k4 s2 (up) -> k3, all with bias, ReLU between; x (B, C, T).  lens: zero every row at or beyond
    the clip's valid length after EVERY layer — valid lengths T_b, T_b >> 1, T_b >> 1, (T_b >> 1) << 1, (T_b >> 1) << 1."""
    def mask(y, shr, shl):
        if lens is None:
            return y
        y = y.clone()
        for b, t in enumerate(lens):
            y[b, :, (t >> shr) << shl:] = 0
        return y
    y = mask(F.relu(F.conv1d(x, *p["k3"], padding=1)), 0, 0)
    y = mask(F.relu(F.conv1d(y, *p["down"], stride=2, padding=1)), 1, 0)
    y = mask(F.relu(F.conv1d(y, *p["mid"], padding=1)), 1, 0)
    y = mask(F.relu(F.conv_transpose1d(y, *p["up"], stride=2, padding=1)), 1, 1)
    return mask(F.conv1d(y, *p["out"], padding=1), 1, 1)


@pytest.mark.parametrize("lens", [[23, 17, 16, 9, 4], [20, 19, 18, 17], [31, 5, 4]])
def test_masking_reproduces_the_clip_alone(lens):
    """Float64 on the CPU, where a sum's bits do not depend on the batch: a padded batch whose rows at or beyond each clip's valid length are
    zeroed after every layer gives, row for row, EXACTLY what each clip gives alone (odd and even T_b, >> 1 and << 1) — and without the
    mask it does not (bias and halo products leak from the padding into a clip's last rows)."""
    p = _stack(7)
    g = torch.Generator().manual_seed(1)
    clips = [torch.randn(8, t, generator=g, dtype=torch.float64) for t in lens]
    T_max = max(lens)
    x = torch.full((len(lens), 8, T_max), 1e3, dtype=torch.float64)       # loud padding
    for b, c in enumerate(clips):
        x[b, :, :lens[b]] = c
    xm = x.clone()
    for b, t in enumerate(lens):
        xm[b, :, t:] = 0                                                  # the input is masked too (the padding is never read)
    masked, leaky = _run(p, xm, lens), _run(p, xm)
    leaks = 0
    for b, c in enumerate(clips):
        solo = _run(p, c[None])[0]
        n = (lens[b] >> 1) << 1
        assert solo.shape[1] == n
        assert torch.equal(masked[b, :, :n], solo), f"clip of T = {lens[b]}"
        assert not masked[b, :, n:].any()
        leaks += int(not torch.equal(leaky[b, :, :n], solo))
    assert leaks > 0
