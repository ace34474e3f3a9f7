"""The stages of a wav session (`ts_mfcc_stream_*`, csrc/mfcc.{hip,cpp}; talkshow_hip.h, "wav sessions") on the GPU, one by one, against the
project's own one-shot entries.  Every comparison is EQUALITY OF BITS; nothing here has a tolerance.

A session's stages are reached through its taps (`ts_debug_mfcc_stream_tap`: every call also leaves its new resampled samples and its new
power rows in caller-owned buffers, at their absolute index) and its dB kernel through `ts_debug_mfcc_stream_db`.  Every buffer the library
writes for a test lies between two 4 KiB zones of sentinel words and starts out sentinel-filled (the discipline of tests/test_gpu_glue_ops.py):
after the session the zones are intact and the WHOLE buffer equals the one-shot entry's result, so every element was written and none beyond.

    stage       yardstick                         cases
    resampler   MFCC.resample on the whole clip   16000 (LDS-staged kernel), 44100 (plain kernel), 22000 (copy) x B = 1, 3; pushes of 1, norig - 1,
                                                  norig, norig + 1, 255, 257 and max_samples samples in one schedule
    STFT        ts_debug_mfcc_stft                N22 = 1025 (the shortest recording), 1467, 1468, 2 hop - 1 at both hops; single-sample pushes over
                                                  the first and the last 64 samples, pushes of 300 between
    dB          ts_debug_mfcc_db                  peak mode under the one-shot's maximum; running mode: row t = row t of the aid on frames 0 .. t,
                                                  T = 1, 2, 7 split over 1, 2 and T calls
    GEMM rows   MFCC.__call__                     B = 1, pushes of one hop: calls that emit ONE row (M = 1) return the bits the row has in the whole call
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, U32, I32 = np.float32, np.uint32, np.int32
SENTINEL = 0x7FC5A5A5                        # a NaN: a float left unwritten never compares equal by accident as a value either
RZ = 1024                                    # words per red zone: 4 KiB


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load()


class Zoned:
    """A float32 device buffer of `shape` between two sentinel zones, sentinel-filled (or holding `a`)."""

    def __init__(self, shape, a=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        img = np.full(2 * RZ + self.n, SENTINEL, U32)
        if a is not None:
            img[RZ:RZ + self.n] = np.ascontiguousarray(a, dtype=F32).reshape(-1).view(U32)
        self.t = torch.from_numpy(img.view(I32)).cuda()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * RZ)

    def read(self, name):
        img = self.t.cpu().numpy().view(U32)
        assert np.all(img[:RZ] == SENTINEL) and np.all(img[RZ + self.n:] == SENTINEL), f"{name}: a red zone was written"
        return img[RZ:RZ + self.n].copy().reshape(self.shape)


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def noise(seed, B, N):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, N)) * np.linspace(0.05, 1.0, N)[None, :]).astype(F32)


class RawSession:
    """`ts_mfcc_stream_*` through ctypes with both taps and the feature rows in zoned buffers."""

    def __init__(self, hip, mfcc, B, max_samples, n22, rows):
        self._lib, self.L = hip
        self.B, self.mfcc = B, mfcc
        self.h = C.c_void_p()
        self._lib.check(self.L.ts_mfcc_stream_open(mfcc._h, B, max_samples, 0, None, C.byref(self.h)))
        self.x22, self.pw = Zoned((B, n22)), Zoned((B, rows, 1056))
        self._lib.check(self.L.ts_debug_mfcc_stream_tap(self.h, self.x22.ptr(), n22, self.pw.ptr(), rows))
        self.cap = int(self.L.ts_mfcc_stream_max_frames(self.h))
        self.feat = Zoned((B, self.cap, 64))
        self.state_bytes = int(self.L.ts_mfcc_stream_state_bytes(self.h))

    def push(self, wav, a, b):
        chunk = torch.from_numpy(np.ascontiguousarray(wav[:, a:b])).cuda() if b > a else None
        f = C.c_int(-1)
        self._lib.check(self.L.ts_mfcc_stream_push(self.h, self._lib.dptr(chunk), b - a, self.feat.ptr(), C.byref(f), self._lib.stream_ptr()))
        return f.value

    def flush(self):
        f = C.c_int(-1)
        self._lib.check(self.L.ts_mfcc_stream_flush(self.h, self.feat.ptr(), C.byref(f), self._lib.stream_ptr()))
        return f.value

    def tails(self):
        out = (C.c_long * 2)()
        self.L.ts_debug_mfcc_stream_tails(self.h, out)
        return int(out[0]), int(out[1])

    def close(self):
        torch.cuda.synchronize()
        assert int(self.L.ts_mfcc_stream_state_bytes(self.h)) == self.state_bytes
        self.L.ts_mfcc_stream_close(self.h)


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("sr", (16000, 44100, 22000))
def test_resampler_any_chunking_equals_the_whole(hip, sr, B):
    from talkshow_amd.frontend import WavStreamPlan
    from talkshow_amd.modules import MFCC
    m = MFCC(sr, 22000, 30)
    k = m.constants
    assert (k["kw"] > 0) == (sr != 22000)
    lds_bytes = 4 * (k["nnew"] * k["kw"] + (255 // k["nnew"] + 1) * k["norig"] + k["kw"])
    assert (lds_bytes <= 48 * 1024) == (sr != 44100), "16000 takes the LDS-staged kernel, 44100 the plain one"
    cap, norig = 600, k["norig"]
    sizes = [1, norig - 1, norig, norig + 1, 255, 257, cap]
    N = sum(sizes) + cap + 64
    sizes += [cap, 64]
    wav = noise(sr + B, B, N)
    want = bits(m.resample(wav))
    n22 = want.shape[1]
    plan = WavStreamPlan(sr, 22000, 30)
    st = RawSession(hip, m, B, cap, n22, n22 // 734 + 1)
    at = 0
    for n in sizes:
        assert st.push(wav, at, at + n) == plan.push(n)
        at += n
        assert st.tails() == plan.retained and st.tails()[0] < max(k["kw"], 1) and st.tails()[1] <= 2048
    assert st.flush() == plan.flush()
    st.close()
    got = st.x22.read("resampled tap")
    assert np.array_equal(got, want), f"{int((got != want).sum())} resampled words differ, first at {np.argwhere(got != want)[0].tolist()}"
    st.pw.read("power tap"), st.feat.read("features")


@pytest.mark.parametrize("fps,N", [(30, 1025), (30, 1467), (30, 1468), (15, 2933), (15, 1467), (15, 1468)])
def test_stft_rows_equal_the_whole_clip(hip, fps, N):
    """equal rates: the samples ARE the resampled samples, so N22 = N exactly"""
    from talkshow_amd.modules import MFCC
    _lib, L = hip
    m = MFCC(22000, 22000, fps)
    B, hop = 2, m.constants["hop"]
    T = N // hop + 1
    wav = noise(N + fps, B, N)
    want = Zoned((B, T, 1056))
    x = torch.from_numpy(wav).cuda()
    _lib.check(L.ts_debug_mfcc_stft(m._h, _lib.dptr(x), B, N, want.ptr(), _lib.stream_ptr()))
    st = RawSession(hip, m, B, 300, N, T)
    sizes, mid = [1] * 64, N - 128
    sizes += [300] * (mid // 300) + ([mid % 300] if mid % 300 else []) + [1] * 64
    assert sum(sizes) == N
    at = rows = 0
    for n in sizes:
        rows += st.push(wav, at, at + n)
        at += n
    assert rows == (N - 1024) // hop + 1                          # N >= 1025: row 0 needs sample 1024, its own reflection
    rows += st.flush()
    assert rows == T
    st.close()
    got, ref = st.pw.read("power tap"), want.read("one-shot power")
    assert np.array_equal(got, ref), f"power rows {sorted(set(np.argwhere(got != ref)[:, 1].tolist()))} differ"
    assert np.array_equal(st.x22.read("resampled tap"), bits(wav))


def mel_block(seed, B, T):
    """mel energies over 14 decades with exact zeros, quiet early rows and a loud late one: both clamps bite, and the running floor moves"""
    rng = np.random.default_rng(seed)
    mel = (10.0 ** rng.uniform(-12, 2, (B, T, 256))).astype(F32)
    mel *= np.linspace(1e-3, 1.0, T, dtype=F32)[None, :, None]
    mel[:, :, 5] = 0.0
    if T > 2:
        mel[:, T - 2, 17] = 3e4
    return mel


def one_shot_db(hip, m, mel):
    _lib, L = hip
    B, T = mel.shape[:2]
    z = Zoned(mel.shape, mel)
    _lib.check(L.ts_debug_mfcc_db(m._h, z.ptr(), None, B, T, _lib.stream_ptr()))
    return z.read("one-shot dB").view(F32)


@pytest.mark.parametrize("T", (1, 2, 7, 70))
def test_db_peak_mode_equals_the_one_shot_clamp(hip, T):
    """T = 70: more rows than the 64 workgroups per slot the launch takes: some workgroup takes a second row"""
    from talkshow_amd.modules import MFCC
    _lib, L = hip
    m, B = MFCC(22000, 22000, 30), 3
    mel = mel_block(T, B, T)
    want = one_shot_db(hip, m, mel)
    peak = Zoned((B,), want.reshape(B, -1).max(axis=1))          # clamping from below leaves the maximum: the one-shot's own
    run = Zoned((B,), np.full(B, -np.inf, F32))
    z = Zoned(mel.shape, mel)
    _lib.check(L.ts_debug_mfcc_stream_db(m._h, z.ptr(), B, T, peak.ptr(), run.ptr(), _lib.stream_ptr()))
    assert np.array_equal(z.read("session dB"), want.view(U32))
    assert np.all(run.read("running maximum").view(F32) == -np.inf), "the peak mode leaves the running maximum alone"
    peak.read("peak")


@pytest.mark.parametrize("T", (1, 2, 7))
def test_db_running_mode_is_the_prefix_maximum(hip, T):
    from talkshow_amd.modules import MFCC
    _lib, L = hip
    m, B = MFCC(22000, 22000, 30), 2
    mel = mel_block(10 + T, B, T)
    want = np.stack([one_shot_db(hip, m, np.ascontiguousarray(mel[:, :t + 1]))[:, t] for t in range(T)], axis=1)
    if T == 7:
        assert not np.array_equal(want, one_shot_db(hip, m, mel)), "the case must tell the running floor from the one-shot's"
    for calls in sorted({1, min(2, T), T}):
        edges = np.linspace(0, T, calls + 1).astype(int)
        run = Zoned((B,), np.full(B, -np.inf, F32))
        got = np.empty((B, T, 256), U32)
        for a, b in zip(edges[:-1], edges[1:]):
            z = Zoned((B, b - a, 256), mel[:, a:b])
            _lib.check(L.ts_debug_mfcc_stream_db(m._h, z.ptr(), B, int(b - a), None, run.ptr(), _lib.stream_ptr()))
            got[:, a:b] = z.read("session dB")
        assert np.array_equal(got, want.view(U32)), (T, calls)
        assert np.array_equal(run.read("running maximum").view(F32), want.reshape(B, -1).max(axis=1))


def test_gemm_rows_of_single_row_calls(hip):
    """B = 1 and pushes of one hop: most calls emit exactly one row, so both GEMMs run with M = 1"""
    from talkshow_amd.modules import MFCC
    m = MFCC(22000, 22000, 30)
    wav = torch.from_numpy(noise(3, 1, 9 * 734 + 100)).cuda()
    want = bits(m(wav))
    st = m.open_stream(1, 734, db=m.peak_db(wav))
    blocks = [st.push(wav[:, a:a + 734]) for a in range(0, wav.shape[1], 734)]
    counts = [int(b.shape[1]) for b in blocks]
    blocks.append(st.flush())
    st.close()
    assert counts.count(1) >= 6 and counts[0] == 0, counts
    got = bits(torch.cat(blocks, dim=1))
    assert got.shape == want.shape and np.array_equal(got, want), f"rows {sorted(set(np.argwhere(got != want)[:, 1].tolist()))} differ"
