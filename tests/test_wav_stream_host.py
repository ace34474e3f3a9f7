"""The host arithmetic of the wav sessions (`talkshow_amd/frontend.py::WavStreamPlan`, `ts_mfcc_stream_plan`; talkshow_hip.h, "wav
sessions") and the numpy twin `frontend.mfcc_stream`, without a GPU.

Plan:   rates 16000 / 24000 / 44100 / 22000 -> 22000 at 30 and 15 fps, over random push schedules that hold pushes of 0 and of 1 sample:
        the Python plan equals the library's call for call; every row 0 .. N22 // hop leaves exactly once and in order; no row leaves before
        a brute-force walk over its samples' taps says that every one has been received; the tails the session keeps stay below kw input
        samples and at most 2048 resampled samples; a flush of a recording of 1024 resampled samples or fewer is refused by both.
Twin:   `mfcc_stream` in peak mode equals `frontend.mfcc` exactly, whatever the chunking; in running mode its row t equals row t of
        `frontend.mfcc_from_power` on the first t + 1 frames.  Equality of bits throughout: nothing here has a tolerance.
        The twin is exact for recordings of 4 rows or more only: it pads every matrix product to 4 rows, because the BLAS behind numpy
        rounds a product of fewer rows differently.  `test_blas_rows_do_not_depend_on_the_row_count_from_4_rows_up` states that property
        of the BLAS on its own, so that another build fails THERE with its name, and the clips here have 7 and 13 rows.  In running mode
        the prefixes of rows 0 .. 2 are themselves shorter than 4 rows: there the twin takes the prefix's own small products, so for
        those three rows the comparison holds the twin's restatement of the clamp against `mfcc_from_power`'s, not two roundings."""
import ctypes as C
import math

import numpy as np
import pytest

from talkshow_amd import frontend as F

RATES = (16000, 24000, 44100, 22000)
FPS = (30, 15)


@pytest.fixture(scope="module")
def lib():
    from talkshow_amd import _lib
    return _lib, _lib.load()


def schedule(rng, total, biggest):
    """push sizes that sum to `total`: zeros, ones and sizes up to `biggest`"""
    out, left = [0, 1, 1], total - 2
    while left > 0:
        n = int(rng.choice([0, 1, int(rng.integers(2, biggest + 1))], p=[0.1, 0.15, 0.75]))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def lib_plan(lib, sr, fps, before, n, flush):
    _lib, L = lib
    a, b = C.c_long(), C.c_long()
    _lib.check(L.ts_mfcc_stream_plan(sr, 22000, fps, before, n, int(flush), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def last_tap(p, j):
    """the last input sample resampled output j reads (the one-shot kernel's loop: base + kw - 1); equal rates: the sample itself"""
    return j if p.sr_in == p.sr_out else (j // p.nnew) * p.norig - p.width + p.kw - 1


def last_sample(p, t):
    """the last resampled sample row t reads before the flush: its window t hop - 1024 .. t hop + 1023 with i < 0 reflected to -i"""
    return max(abs(t * p.hop + k - 1024) for k in (0, 2047))


@pytest.mark.parametrize("fps", FPS)
@pytest.mark.parametrize("sr", RATES)
def test_plan_against_library_and_walk(lib, sr, fps):
    rng = np.random.default_rng(sr + fps)
    for trial in range(3):
        p = F.WavStreamPlan(sr, 22000, fps)
        total = int(rng.integers(4 * sr // 10, sr))                   # 0.4 .. 1 s: 12 .. 30 rows at 30 fps
        emitted = []
        for n in schedule(rng, total, sr // 8):
            before = p.samples_in
            t0 = p.frames_out
            f = p.push(n)
            fb, fa = lib_plan(lib, sr, fps, before, n, False)
            assert (fb, fa) == (t0, t0 + f), (sr, fps, before, n)
            emitted += list(range(t0, t0 + f))
            # never early: every sample of every emitted row has all its taps in (walked from the definition, not from the closed form)
            for t in range(t0, t0 + f):
                assert last_tap(p, last_sample(p, t)) < p.samples_in, t
            # never late: the next row is still short of a tap
            assert last_tap(p, last_sample(p, p.frames_out)) >= p.samples_in
            tail_in, tail22 = p.retained
            assert 0 <= tail_in < max(p.kw, 1) and 0 <= tail22 <= 2048, (tail_in, tail22)
        N22 = math.ceil(total * p.nnew / p.norig) if sr != 22000 else total
        assert p.total22(total) == N22
        t0 = p.frames_out
        f = p.flush()
        assert lib_plan(lib, sr, fps, total, 0, True) == (t0, t0 + f)
        emitted += list(range(t0, t0 + f))
        assert emitted == list(range(N22 // p.hop + 1))
        with pytest.raises(ValueError):
            p.push(1)


@pytest.mark.parametrize("sr", RATES)
def test_short_flush_refused(lib, sr):
    _lib, L = lib
    p = F.WavStreamPlan(sr, 22000, 30)
    n = 1024 * p.norig // p.nnew                                       # the most samples that still give N22 <= 1024
    assert p.total22(n) <= 1024 < p.total22(n + 1)
    p.push(n)
    with pytest.raises(ValueError, match="shorter than half an FFT window"):
        p.flush()
    assert (p.samples_in, p.frames_out, p.flushed) == (n, 0, False)
    a, b = C.c_long(), C.c_long()
    assert L.ts_mfcc_stream_plan(sr, 22000, 30, n, 0, 1, C.byref(a), C.byref(b)) != 0
    assert "shorter than half an FFT window" in L.ts_last_error().decode()
    p.push(p.norig)                                                    # one resampled sample more, at least: now a recording
    assert p.frames_out + p.flush() == p.total22(n + p.norig) // p.hop + 1


def test_latency_figures():
    """the figures talkshow_hip.h quotes: the resampler's right wing is kw - width - 1 = width + norig - 1 input samples"""
    for sr, (norig, width, kw) in {16000: (8, 7, 22), 44100: (441, 13, 467)}.items():
        p = F.WavStreamPlan(sr)
        assert (p.norig, p.width, p.kw) == (norig, width, kw)
        assert p.latency_samples == (1024, kw - width - 1)
    assert F.WavStreamPlan(22000).latency_samples == (1024, 0)


@pytest.fixture(scope="module")
def clip():
    rng = np.random.default_rng(11)
    n = 9000
    return (rng.standard_normal(n) * np.concatenate([np.linspace(0.001, 1.0, n // 2), np.linspace(1.0, 0.01, n - n // 2)])).astype(np.float32)


def cut(w, sizes):
    out, o = [], 0
    for s in sizes:
        out.append(w[o:o + s])
        o += s
    assert o == w.shape[0]
    return out


CHUNKINGS = ([9000], [1, 0, 1500, 733, 3000, 3766], [500] * 18, [1] * 40 + [8960])


def test_blas_rows_do_not_depend_on_the_row_count_from_4_rows_up():
    """What `frontend._rows_matmul` leans on (measured with OpenBLAS 0.3.29): row i of a float32 product of M >= 4 rows has the same bits for
    every M and every place i, in both shapes the front end multiplies.  A BLAS without the property cannot hold the twin tests below."""
    rng = np.random.default_rng(2)
    for K, N in ((1025, 256), (256, 64)):
        a, b = (rng.standard_normal((13, K)) ** 2).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
        full = a @ b
        for M in range(4, 13):
            assert np.array_equal(a[:M] @ b, full[:M]) and np.array_equal(a[13 - M:] @ b, full[13 - M:]), (K, N, M)
        assert np.array_equal(F._rows_matmul(a[:1], b), full[:1]) and np.array_equal(F._rows_matmul(a[5:8], b), full[5:8])


@pytest.mark.parametrize("hop", (734, 1467))
def test_twin_peak_mode_equals_one_shot(clip, hop):
    ref = F.mfcc(clip, 22000, hop_length=hop).T
    assert ref.shape[0] >= 4
    pk = F.peak_db(clip, 22000, hop_length=hop)
    for sizes in CHUNKINGS:
        blocks = F.mfcc_stream(cut(clip, sizes), 22000, hop_length=hop, db=pk)
        assert len(blocks) == len(sizes) + 1
        assert np.array_equal(np.concatenate(blocks), ref), sizes


@pytest.mark.parametrize("hop", (734, 1467))
def test_twin_running_mode_is_the_prefix_clamp(clip, hop):
    power = F.power_spectrogram(clip, 2048, hop)
    want = np.stack([F.mfcc_from_power(power[:t + 1], 22000)[:, t] for t in range(power.shape[0])])
    for sizes in CHUNKINGS:
        got = np.concatenate(F.mfcc_stream(cut(clip, sizes), 22000, hop_length=hop))
        assert np.array_equal(got, want), sizes
    # the clip grows louder up to its middle: the running floor really differs from the one-shot's in the early rows
    assert not np.array_equal(want, F.mfcc(clip, 22000, hop_length=hop).T)
