"""Host-side logic of the PACKED mixed face pass (no GPU): the row layout (`ts_debug_face_packed_layout`), the argument that lets clips lie
back to back on one time axis through the six stride-2 feature convolutions, and `ts_face_mixed_rows`.

The library loads without a device; both entries are host arithmetic only.  Every test fails on a build without the feature: the entries
do not exist there.
"""
import ctypes as C

import numpy as np
import pytest

from talkshow_amd import frontend

I32P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
FC_K = (3, 3, 3, 3, 2, 2)


def levels(n_rows):
    """Rows of level 0 .. 6 of the stride-2, no-padding chain from n_rows rows at the conv0 rate."""
    L = [int(n_rows)]
    for k in FC_K:
        L.append((L[-1] - k) // 2 + 1)
    return L


def l0(n):
    return (int(n) - 10) // 5 + 1


def layout(ns, frames):
    from talkshow_amd import _lib
    lib = _lib.load()
    ns, frames = np.ascontiguousarray(ns, np.int32), np.ascontiguousarray(frames, np.int32)
    B = len(ns)
    off, row0, lv = np.full(B + 1, -7, np.int64), np.full(B + 1, -7, np.int64), np.full(7, -7, np.int64)
    rc = lib.ts_debug_face_packed_layout(ns.ctypes.data_as(I32P), frames.ctypes.data_as(I32P), B, off.ctypes.data_as(I64P),
                                         row0.ctypes.data_as(I64P), lv.ctypes.data_as(I64P))
    return rc, off, row0, lv


def _tables():
    from test_gpu_face_mixed import SPEC, _frames
    rng = np.random.default_rng(0)
    spec = [(n, _frames(n, f)) for n, f in SPEC]
    assert (400, 1) in spec
    out = []
    for pos in (0, 7, len(spec) - 1):                                     # the 400-sample clip first, inside, last
        rest = [s for s in spec if s != (400, 1)]
        out.append(rest[:pos] + [(400, 1)] + rest[pos:])
    for _ in range(20):
        B = int(rng.integers(1, 40))
        ns = rng.integers(400, 330000, B)
        ns[int(rng.integers(0, B))] = 400                                 # one 400-sample clip anywhere in the list
        fr = np.maximum(1, ns * 30 // 16000 + rng.integers(-2, 3, B))
        out.append(list(zip(ns.tolist(), fr.tolist())))
    return out


@pytest.mark.parametrize("k", range(23))
def test_layout_properties(k):
    table = _tables()[k]
    ns, fr = [n for n, _ in table], [f for _, f in table]
    B = len(ns)
    rc, off, row0, lv = layout(ns, fr)
    assert rc == 0
    seg = [-(-l0(n) // 64) * 64 for n in ns]
    assert (off % 64 == 0).all() and off[0] == 0 and row0[0] == 0
    # disjoint, in submission order, each holding the clip's own rows; the totals are the sums
    assert np.array_equal(np.diff(off), seg) and all(s >= l0(n) for s, n in zip(seg, ns))
    assert np.array_equal(np.diff(row0), fr)
    assert off[B] == sum(seg) and row0[B] == sum(fr)
    assert off[B] <= sum(l0(n) for n in ns) + 63 * B                      # at most 63 rows of rounding per clip
    # the per-level lengths of the chain run as ONE problem follow the recurrence
    assert lv.tolist() == levels(off[B])
    # every valid output row of every clip, at every level, reads the clip's own valid rows of the level below — and those rows exist
    for b, n in enumerate(ns):
        own = levels(l0(n))
        assert own[6] >= 1
        for i, kk in enumerate(FC_K):
            first_in, first_out = int(off[b]) >> i, int(off[b]) >> (i + 1)
            assert first_in << i == off[b] and first_out << (i + 1) == off[b]          # exact: no rounding of the clip's start at any level
            t = np.arange(own[i + 1])
            reads = first_in + 2 * t[:, None] + np.arange(kk)[None]       # output row first_out + t reads input rows first_in + 2 t + d
            assert reads.min() >= first_in and reads.max() < first_in + own[i]
            assert first_out + own[i + 1] <= lv[i + 1] and reads.max() < lv[i]
            if b + 1 < B:                                                 # ... and stay inside the clip's segment at both levels
                assert first_in + own[i] <= int(off[b + 1]) >> i and first_out + own[i + 1] <= int(off[b + 1]) >> (i + 1)


def test_layout_rejects_bad_tables():
    assert layout([399], [1])[0] == -1
    assert layout([16000, 8000], [30, 0])[0] == -1
    assert layout([16000], [65537])[0] == -1
    assert layout([16000], [65536])[0] == 0
    # row counts beyond the engines' int row indices: a clip of 2^31 - 1 samples has 429 496 728 rows at the conv0 rate, five pass 2^31
    big = [2 ** 31 - 1] * 4
    assert layout(big, [1] * 4)[0] == 0
    assert layout(big + [2 ** 31 - 1], [1] * 5)[0] == -1
    assert layout([400] * 40000, [65536] * 40000)[0] == -1                # 2.6e9 transformer rows
    from talkshow_amd import _lib
    assert _lib.load().ts_debug_face_packed_layout(None, None, 1, None, None, None) == -1


def _chain(x, ws):
    """float64 stride-2, no-padding conv chain on x (rows, C): out[t] = sum_d x[2 t + d] @ w[d]."""
    for w in ws:
        k = w.shape[0]
        n = (x.shape[0] - k) // 2 + 1
        x = sum(x[d:d + 2 * n:2][:n] @ w[d] for d in range(k))
    return x


def test_seam_argument():
    """The chain on the concatenated axis, as one problem, equals the chain on every clip alone on every valid row — small integers in
    float64: exact.  Clips whose conv0 row counts are 1, 63, 64, 65 and 129 rows off a multiple of 64, in two orders; the zeros between a
    clip's own rows and the next segment are replaced by large values: no valid row may read them."""
    rng = np.random.default_rng(1)
    Cc = 4
    ws = [rng.integers(-2, 3, (k, Cc, Cc)).astype(np.float64) for k in FC_K]
    rows = [640 + 1, 448 + 63, 512 + 64, 704 + 65, 384 + 129, 79]         # 79 rows: the 400-sample clip, one row at level 6
    assert levels(79)[6] == 1
    for order in (range(len(rows)), rng.permutation(len(rows))):
        clips = [rng.integers(-3, 4, (rows[i], Cc)).astype(np.float64) for i in order]
        # the layout's offsets for sample counts with exactly these conv0 row counts
        ns = [5 * (c.shape[0] - 1) + 10 for c in clips]
        assert [l0(n) for n in ns] == [c.shape[0] for c in clips]
        rc, off, _, lv = layout(ns, [1] * len(ns))
        assert rc == 0
        axis = np.full((int(off[-1]), Cc), 1e6)
        for b, c in enumerate(clips):
            axis[off[b]:off[b] + c.shape[0]] = c
        x = axis
        for i, w in enumerate(ws):
            x = _chain(x, [w])
            assert x.shape[0] == lv[i + 1]
            for b, c in enumerate(clips):
                alone = _chain(c, ws[:i + 1])
                first = int(off[b]) >> (i + 1)
                assert np.array_equal(x[first:first + alone.shape[0]], alone), f"level {i + 1}, clip {b} ({c.shape[0]} rows)"
        assert np.abs(x).max() > 1e5                                      # the seam rows DO hold a neighbour's data: nothing valid read them


def _rows(ns, frames, N_max=None, T_max=None):
    from talkshow_amd import _lib
    lib = _lib.load()
    ns, frames = np.ascontiguousarray(ns, np.int32), np.ascontiguousarray(frames, np.int32)
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.ts_face_mixed_rows(ns.ctypes.data_as(I32P), frames.ctypes.data_as(I32P), len(ns), int(ns.max()) if N_max is None else N_max,
                                int(frames.max()) if T_max is None else T_max, out)
    return rc, list(out), lib.ts_last_error().decode()


def test_mixed_rows_closed_forms():
    """Recordings at 44.1 kHz: `frontend.mixed_tables` gives each one's 16 kHz sample count and face frames; the four row counts follow."""
    rng = np.random.default_rng(2)
    t = frontend.mixed_tables(rng.integers(3 * 44100, 20 * 44100, 64), 44100)
    ns, fr = t["n16"], t["face_frames"]
    B = len(ns)
    rc, got, _ = _rows(ns, fr)
    assert rc == 0
    want = [B * l0(ns.max()), sum(-(-l0(n) // 64) * 64 for n in ns), B * int(fr.max()), int(fr.sum())]
    assert got == want
    assert got[1] < got[0] and got[3] < got[2]                            # a spread of lengths: the packed pass has fewer rows
    rc, eq, _ = _rows([160000] * 64, [300] * 64)
    assert rc == 0 and eq == [64 * 31999, 64 * 32000, 64 * 300, 64 * 300]   # equal clips: 1 row of rounding each, no fewer frames
    from talkshow_amd.modules import FaceGenerator
    d = FaceGenerator.mixed_rows([int(n) for n in ns])
    assert [d["feature_rows_padded"], d["feature_rows_packed"], d["frames_padded"], d["frames_packed"]] == want
    assert FaceGenerator.mixed_rows([np.zeros(16000, np.float32), np.zeros(8000, np.float32)], [30, 15])["frames_packed"] == 45
    with pytest.raises(ValueError):
        FaceGenerator.mixed_rows([399])
    with pytest.raises(ValueError):
        FaceGenerator.mixed_rows([16000, 8000], [30])


def test_mixed_rows_rejects_bad_tables():
    good_n, good_f = [8000, 4000, 400], [15, 7, 1]
    assert _rows(good_n, good_f)[0] == 0
    for ns, fr, N_max, T_max, msg in [([8000, 399, 400], good_f, None, None, "shorter than 400 samples"),
                                      (good_n, [15, 0, 1], None, None, "has no frames"),
                                      (good_n, good_f, 7999, None, "longer than N_max"),
                                      (good_n, good_f, None, 14, "more frames than T_max"),
                                      (good_n, good_f, None, 65537, "bad shape")]:
        rc, out, err = _rows(ns, fr, N_max, T_max)
        assert rc != 0 and msg in err and out == [-1] * 4, (rc, err, out)
    from talkshow_amd import _lib
    lib = _lib.load()
    a = np.asarray(good_n, np.int32)
    assert lib.ts_face_mixed_rows(a.ctypes.data_as(I32P), None, 3, 8000, 15, (C.c_int64 * 4)()) != 0
    assert lib.ts_face_mixed_rows(a.ctypes.data_as(I32P), a.ctypes.data_as(I32P), 3, 8000, 15, None) != 0
