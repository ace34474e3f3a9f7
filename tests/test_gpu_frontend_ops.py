"""Op-level tests of the audio front end (`csrc/mfcc.hip`, `csrc/mfcc.cpp`), stage by stage against float64: the two resamplers through their
public entries (`ts_mfcc_resample`, `ts_resample_kaiser`, the `_mixed` forms) and the four stages behind them through the test aids of
`include/talkshow_hip_debug.h` (`ts_debug_mfcc_stft / _mel / _db / _dct`, `frames_dev` or `_lens` = the length variant), each one production
launch on the handle's own tables: what is tested is the device's window, twiddles, filterbank, DCT matrix, polyphase and Kaiser tables.

References.  Float64 restatements of the published definitions the sources cite, written here: torchaudio's sinc-Hann polyphase kernel
(`poly_kernel`, `poly_ref`), resampy's kaiser_best interpolation (`kaiser_filter`, `kaiser_ref`), torch.stft with center / reflect and a
periodic Hann window on `np.fft.rfft` (`stft_ref`), the HTK filterbank (`mel_fbanks`), 10 log10(clamp 1e-10) with the per-clip clamp
(`db_ref`), the orthonormal DCT-II (`dct_matrix`).  None restates a kernel's order of operations, none uses the fp32 twins of
talkshow_amd/frontend.py; `test_references_against_third_party` holds them to torch.stft, transformers' filterbank and scipy's DCT.

Guards.  Inputs and outputs sit in the allocations of tests/test_gpu_canary.py (`Guarded`, `run_both`: NaN red zones round the inputs, a
sentinel in and round the outputs, the guarded call bit-equal to the plain one, every output element written).  In length-variant cases every
padded input element beyond a clip's own length holds NaN and every output element beyond it must be +0.0.

Error units and bounds (measured, not guessed: the protocol of tests/test_gpu_conv_ops.py).
  stft      per bin (|X_k| + A) A with A = sum |x_n w_n| over the frame: first-order propagation of |X|^2 with |dX_k| proportional to A
  db        max(|v|, 1) of the float64 value v
  mel, dct  sum |x w| (as test_gpu_conv_ops.py); ceiling (Ktot + 4) 2^-24, Ktot = 1056 / 256
  tables    read back through the GEMMs by one-hot rows (the product is 1 w plus zeros, exact): |got - ref| <= 2^-24 |ref| + 1e-11, one fp32
            rounding of the float64 value plus the cancellation at the triangles' corners (the corner frequencies carry ~1e-12 Hz of libm
            difference, a triangle is >= 7 Hz wide: `test_table_tolerance_derivation` measures 80-bit against 64-bit).  Derived, not measured.
  poly      sum |k| |x|; ceiling (kw + 2) 2^-24: an fma chain of kw terms plus one table entry rounded differently by another libm.  The
            Hann window's outermost taps (t clamped to +-6: ~1e-49) lie below fp32's range and round absolutely, not relatively: 2^-126 |x|
            per tap (the smallest normal number: covers a flush to zero) is taken off the error first.  An impulse reads exactly these.
  kaiser    scale sum |w| |x|, |w| = the interpolation (1 - eta) |win_k| + eta |win_k+1| of the table's magnitudes (the first-order weight of
            the table's own fp32 rounding: where the interpolated weight crosses zero between two entries its own magnitude says nothing);
            ceiling 4 2^-24: the kernel accumulates in double, only the final rounding and the table's own fp32 rounding remain
Each asserted bound is 2x the largest error of its stage that the first MI355X run of this file recorded against the float64 reference
(TS_MEASURED_LOG; profiles/frontend_ops_measured.jsonl): fixed sums are bit-reproducible, the margin covers a compiler or libm revision that
reassociates or rounds once more.  Where a ceiling is given, the bound is asserted to lie under the ceiling of every case.  For the FFT and
the dB stage NO ceiling is asserted: no documented bound of the device's log10f or of the FFT's error constant was at hand, so for these two
the bound is the measured one alone.  `test_bounds_catch_defects` (CPU) applies each defect of DEFECTS to the float64 reference and shows that
the bound of the stage named there misses it by at least 10x.

Bit-identity.  The valid rows / samples of every length variant equal the uniform kernel on the clip alone; the stages run one after the
other through the entries give the bits of ts_mfcc_forward / ts_mfcc_forward_mixed.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from test_gpu_canary import F32, Guarded, run_both

F64 = np.float64
U = 2.0 ** -24
NFFT, NBINS, NPAD, NMELS, NMFCC = 2048, 1025, 1056, 256, 64
HOPS = {30: 734, 15: 1467}
# 2x the largest error of the stage in the first MI355X run's records (profiles/frontend_ops_measured.jsonl; that run had no bounds yet and
# asserted the ceilings, its stft and db lines carry an infinite bound), in the units of the docstring.  Every case passed on that run.
STFT_BOUND = 5.4e-7      # 2.686e-7: impulse, hop 734, N = 1467
DB_BOUND = 5.9e-7        # 2.916e-7: the length variant (T = 7: 2.911e-7)
MEL_BOUND = 6.4e-7       # 3.194e-7: noise, 22000 (5.4 x 2^-24 over Ktot = 1056)
DCT_BOUND = 3.6e-7       # 1.774e-7: noise, 22000
POLY_BOUND = 5.4e-7      # 2.698e-7: 8000 -> 22000
KAISER_BOUND = 2.0e-7    # 9.569e-8: 22050 -> 16000, N = 20000
TABLE_REL, TABLE_ABS = U, 1e-11
F32_TINY = 2.0 ** -126
KAISER_CEILING = 4 * U


def gemm_ceiling(Ktot):
    return (Ktot + 4) * U


def poly_ceiling(kw):
    return (kw + 2) * U


def measured(stage, case, err, bound, ceiling=None):
    """Records err (TS_MEASURED_LOG) and asserts it under the stage's bound; the bound itself under the case's ceiling."""
    assert ceiling is None or bound <= ceiling, f"{stage}.{case}: bound {bound:.2e} over the ceiling {ceiling:.2e}"
    assert_close_measured(f"frontend.{stage}.{case}", np.array([err]), np.array([0.0]), bound)


def in_units(err, unit):
    """max err / unit; where the unit is 0 (nothing contributes) the error must be 0."""
    err, unit = np.asarray(err, F64), np.asarray(unit, F64)
    assert (err[unit == 0] == 0).all(), "a value that nothing contributes to is not exactly zero"
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


# ----------------------------------------------------------------------------------------------- float64 references
def hann(n=NFFT, periodic=True):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n if periodic else n - 1))


def rfft_last_pass(fr, defect=False):
    """rfft of rows of 2048 reals written as a 1024-point complex transform of z = even + i odd whose last radix-4 step is spelled out
    (Z[k + 256 q] = sum_r W^(r k) (-i)^(r q) Y_r[k], Y_r = the 256-point transform of z[r::4], W = exp(-2 pi i / 1024)) and the even / odd
    split.  defect: the twiddle of (r, k) = (1, 37) takes index r k + 1."""
    z = fr[:, 0::2] + 1j * fr[:, 1::2]
    k = np.arange(256)
    Z = np.zeros((fr.shape[0], 1024), complex)
    Y = [np.fft.fft(z[:, r::4], axis=1) for r in range(4)]
    for r in range(4):
        idx = (r * k).astype(F64)
        if defect and r == 1:
            idx[37] += 1
        tw = np.exp(-2j * np.pi * idx / 1024.0)
        for q in range(4):
            Z[:, k + 256 * q] += tw * (-1j) ** (r * q) * Y[r]
    kk = np.arange(1025)
    Zk, Zn = Z[:, kk % 1024], np.conj(Z[:, (1024 - kk) % 1024])
    return 0.5 * (Zk + Zn) - 0.5j * np.exp(-2j * np.pi * kk / 2048.0) * (Zk - Zn)


def stft_ref(x, hop, defect=None):
    """x (N,) -> power (T, 1025), |X| (T, 1025), A (T,): torch.stft(center=True, pad_mode='reflect', periodic Hann, n_fft 2048), T = N // hop + 1."""
    x = np.asarray(x, F64)
    T = x.size // hop + 1
    pad = np.pad(x, NFFT // 2, mode="symmetric" if defect == "reflect_repeats_edge" else "reflect")
    if defect == "hop_733":
        hop = 733
    w = hann(periodic=defect != "hann_symmetric")
    fr = np.stack([pad[t * hop:t * hop + NFFT] for t in range(T)]) * w
    X = rfft_last_pass(fr, True) if defect == "twiddle_index" else np.fft.rfft(fr, axis=1)
    if defect == "bin_1024_from_bin_0":
        X[:, 1024] = X[:, 0]
    return np.abs(X) ** 2, np.abs(X), np.abs(fr).sum(1)


def stft_error(got, x, hop):
    """got (T, 1025) against the reference of x (N,), in the units (|X_k| + A) A."""
    P, aX, A = stft_ref(x, hop)
    return in_units(np.abs(np.asarray(got, F64) - P), (aX + A[:, None]) * A[:, None])


def mel_points(n_mels, f_max, scale="htk"):
    if scale == "htk":
        m = np.linspace(0.0, 2595.0 * np.log10(1.0 + f_max / 700.0), n_mels + 2)
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0          # Slaney (the defect): linear below 1 kHz, logarithmic above
    to_mel = lambda f: np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)
    m = np.linspace(0.0, float(to_mel(np.asarray(f_max))), n_mels + 2)
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def mel_fbanks(sr, scale="htk", dtype=F64):
    """torchaudio.functional.melscale_fbanks(1025, 0, sr // 2, 256, sr, norm=None, mel_scale) -> (1025, 256)."""
    f_max = dtype(sr // 2)
    freqs = np.linspace(dtype(0), f_max, NBINS, dtype=dtype)
    if dtype is F64:
        pts = mel_points(NMELS, f_max, scale)
    else:
        m = np.linspace(dtype(0), dtype(2595) * np.log10(dtype(1) + f_max / dtype(700)), NMELS + 2, dtype=dtype)
        pts = dtype(700) * (dtype(10) ** (m / dtype(2595)) - dtype(1))
    diff = pts[1:] - pts[:-1]
    slopes = pts[None, :] - freqs[:, None]
    return np.maximum(0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]))


def dct_matrix(defect=None, dtype=F64):
    """torchaudio.functional.create_dct(64, 256, 'ortho') -> (256, 64): column k = cos(pi / 256 (n + 1/2) k) sqrt(2 / 256), k = 0 over sqrt 2."""
    n, k = np.arange(NMELS, dtype=dtype)[:, None], np.arange(NMFCC, dtype=dtype)[None, :]
    d = np.cos(dtype(np.pi if dtype is F64 else np.arctan(dtype(1)) * 4) / dtype(NMELS) * (n + dtype(0.5)) * k)
    if defect != "dct_row0_unscaled":
        d[:, 0] /= np.sqrt(dtype(2))
    return d * np.sqrt(dtype(2) / dtype(NMELS))


def db_ref(p, frames=None, defect=None):
    """p (B, T, 256) -> 10 log10(max(p, 1e-10)) clamped at the clip's own maximum - 80 (over its first frames[b] rows; the rows beyond: 0)."""
    p = np.asarray(p, F64)
    B, T = p.shape[:2]
    frames = [T] * B if frames is None else frames
    out = np.zeros_like(p)
    v = [10.0 * np.log10(np.maximum(p[b, :frames[b]], 1e-9 if defect == "floor_1e-9" else 1e-10)) for b in range(B)]
    for b in range(B):
        mx = max(vv.max() for vv in v) if defect == "max_over_block" else v[b].max()
        out[b, :frames[b]] = np.maximum(v[b], mx - 80.0)
    return out


def poly_params(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    orig, new = sr_in // g, sr_out // g
    base = min(orig, new) * 0.99
    width = int(math.ceil(6.0 * orig / base))
    return orig, new, base, width, 2 * width + orig


def poly_kernel(sr_in, sr_out):
    """torchaudio _get_sinc_resample_kernel (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) -> (new, kw) float64."""
    orig, new, base, width, kw = poly_params(sr_in, sr_out)
    idx = np.arange(-width, width + orig, dtype=F64) / orig
    t = (np.arange(0, -new, -1, dtype=F64)[:, None] / new + idx[None, :]) * base
    t = np.clip(t, -6.0, 6.0)
    window = np.cos(t * np.pi / 6.0 / 2.0) ** 2
    t = t * np.pi
    return np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)


def poly_ref(x, sr_in, sr_out, defect=None):
    """torchaudio _apply_sinc_resample_kernel on x (N,): pad (width, width + orig), convolve with stride orig, keep ceil(new N / orig)
    -> (values, units sum |k| |x|)."""
    x = np.asarray(x, F64)
    orig, new, _, width, kw = poly_params(sr_in, sr_out)
    kern = poly_kernel(sr_in, sr_out)
    n_out = -(-new * x.size // orig)
    j = np.arange(n_out)
    idx = (j // new)[:, None] * orig - width + np.arange(kw)[None, :] + (1 if defect == "width_shift" else 0)
    ok = (idx >= 0) & (idx < x.size)
    terms = kern[j % new] * np.where(ok, x[np.clip(idx, 0, x.size - 1)], 0.0)
    return terms.sum(1), np.abs(terms).sum(1)


def kaiser_filter():
    """resampy's published kaiser_best design: the right half of a Kaiser-windowed sinc, 64 zero crossings, 512 samples per crossing."""
    from scipy.signal.windows import kaiser
    num_zeros, num_bits = 64, 512
    n = num_bits * num_zeros
    rolloff, beta = 0.9475937167399596, 14.769656459379492
    win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, n + 1)) * kaiser(2 * n + 1, beta)[n:]
    return win, np.append(np.diff(win), 0.0), num_bits


_KAISER = []


def kaiser_ref(x, sr_in, sr_out, defect=None):
    """resampy.resample(x, sr_in, sr_out, filter='kaiser_best') (resample_f) followed by librosa's fix_length to ceil(N ratio)
    -> (values, units): output t at input time t / ratio sums win[offset + i step] + eta delta[...] over both wings."""
    if not _KAISER:
        _KAISER.append(kaiser_filter())
    win, delta, num_table = _KAISER[0]
    x = np.asarray(x, F64)
    N, ratio = x.size, sr_out / sr_in
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    n_res, n_fix = int(N * ratio), int(math.ceil(N * ratio))
    tr = np.arange(n_res) / ratio
    n = tr.astype(np.int64)
    y, unit = np.zeros(n_fix), np.zeros(n_fix)
    awin = np.abs(win)
    adelta = np.append(awin[1:] - awin[:-1], 0.0)
    for wing in (0, 1):
        frac = scale * (tr - n) if wing == 0 else scale - scale * (tr - n)
        index_frac = frac * num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        reach = (win.size - offset) // step
        if wing == 0:
            count = np.minimum(n + 1, reach)
        else:
            count = np.minimum(N - n - 1, reach) - (1 if defect == "k_max_short" else 0) * (N - n - 1 <= reach)
        i = np.arange(int(max(count.max(), 0)))[None, :]
        live = i < count[:, None]
        k = np.where(live, offset[:, None] + i * step, 0)
        src = np.where(live, n[:, None] - i if wing == 0 else n[:, None] + i + 1, 0)
        xs = np.where(live, x[src], 0.0)
        y[:n_res] += ((win[k] + eta[:, None] * delta[k]) * xs).sum(1)
        unit[:n_res] += ((awin[k] + eta[:, None] * adelta[k]) * np.abs(xs)).sum(1)
    return y * scale, unit * scale


# ----------------------------------------------------------------------------------------------- inputs
def stft_inputs(kind, N, seed):
    """(3, N) float32, another content in every clip."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    if kind == "noise":
        x = rng.standard_normal((3, N)) * np.array([1.0, 0.3, 3.0])[:, None]
    elif kind == "impulse":
        x = np.zeros((3, N))
        x[0, 0], x[1, N - 1], x[2, (N // 2) | 1] = 1.0, -0.75, 1.5
    elif kind in ("cos_low", "cos_high"):
        bins = (0, 1, 511) if kind == "cos_low" else (512, 1023, 1024)
        x = np.stack([np.cos(2.0 * np.pi * k * n / NFFT) for k in bins])
    else:                                                    # a strong tone and noise 100 dB below it
        x = np.stack([np.cos(2.0 * np.pi * f * n / NFFT) for f in (100.3, 700.5, 1000.25)]) + 1e-5 * rng.standard_normal((3, N))
    return x.astype(np.float32)


def db_inputs(T, where, seed):
    """(3, T, 256) float32 powers: clip maxima 1e13, 1e3 and 1e-6 (130, 30 and -60 dB: more than 80 dB from each other), each clip spanning
    140 dB below its maximum, with exact zeros, values under 1e-10 and a subnormal; the maximum sits at flat index `where` (negative: from the
    end) of every clip."""
    rng = np.random.default_rng(seed)
    n = T * NMELS
    p = np.empty((3, n), F64)
    for b, top in enumerate((1e13, 1e3, 1e-6)):
        p[b] = top * 10.0 ** (-14.0 * rng.random(n)) * 0.99
        sp = rng.permutation(n)[:12]
        p[b, sp[:4]], p[b, sp[4:8]], p[b, sp[8:12]] = 0.0, 3e-12, 1e-40
        p[b, where] = top
    return p.reshape(3, T, NMELS).astype(np.float32)


# ----------------------------------------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    lib, ctx = _lib.load(), _lib.context(0)
    handles = {}

    def handle(sr_in, sr_out, fps=30):
        if (sr_in, sr_out, fps) not in handles:
            h = C.c_void_p()
            _lib.check(lib.ts_mfcc_create(ctx, sr_in, sr_out, fps, C.byref(h)))
            handles[(sr_in, sr_out, fps)] = h
        return handles[(sr_in, sr_out, fps)]

    yield _lib, lib, ctx, handle
    torch.cuda.synchronize()
    for h in handles.values():
        lib.ts_mfcc_destroy(h)


def i32(v):
    a = np.ascontiguousarray(v, np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32)), torch.from_numpy(a).cuda()


def run_inplace(call, data):
    """run_both for an entry that works in place on one float32 buffer: the plain run and the run between sentinel red zones give the same bits,
    the zones stay intact.  -> the guarded body (device tensor)."""
    plain = torch.from_numpy(np.ascontiguousarray(data, np.float32)).cuda()
    call(C.c_void_p(plain.data_ptr()))
    torch.cuda.synchronize()
    g = Guarded(data.shape, F32, data)
    call(g.ptr())
    torch.cuda.synchronize()
    assert g.zones_intact(), "a store landed outside the buffer"
    assert np.array_equal(g.bits(), plain.view(torch.int32).cpu().numpy().reshape(-1)), "the guarded run differs from the plain run"
    return g.body


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def stft_run(hip, h, hop, x):
    _lib, lib, _, _ = hip
    B, N = x.shape
    T = N // hop + 1
    r = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_stft(h, p["x"], B, N, p["pw"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"pw": ((B * T, NPAD), F32)})
    return r["pw"].cpu().numpy().reshape(B, T, NPAD)


# ----------------------------------------------------------------------------------------------- STFT power
STFT_KINDS = ["noise", "impulse", "cos_low", "cos_high", "tone"]
STFT_LENGTHS = [(30, 1025), (30, 1467), (30, 1468), (30, 5000), (15, 1467), (15, 2934)]


@pytest.mark.gpu
@pytest.mark.parametrize("fps,N", STFT_LENGTHS)
@pytest.mark.parametrize("kind", STFT_KINDS)
def test_stft_power(hip, fps, N, kind):
    """N = 1025: the minimum, both frames reflect at both ends; 1468 = 2 hop: the last frame is centred on sample N; 5000: interior frames and
    one that reflects on the right only.  Impulses: the power of a frame that holds the impulse once is (x w[n])^2 on every bin, which any
    permutation inside a Stockham pass or a wrong even / odd split breaks; cosines on bins 0, 1, 511, 512, 1023, 1024."""
    hop = HOPS[fps]
    x = stft_inputs(kind, N, N + fps)
    pw = stft_run(hip, hip[3](22000, 22000, fps), hop, x)
    T = N // hop + 1
    assert pw.shape == (3, T, NPAD)
    assert (bits(pw[:, :, NBINS:]) == 0).all(), "columns 1025 .. 1055 are not +0.0"
    worst = 0.0
    for b in range(3):
        worst = max(worst, stft_error(pw[b, :, :NBINS], x[b], hop))
        if kind == "impulse":
            pad = np.pad(x[b].astype(F64), NFFT // 2, mode="reflect")
            for t in range(T):
                fr = pad[t * hop:t * hop + NFFT] * hann()
                if np.count_nonzero(fr) == 1:
                    flat = fr[np.flatnonzero(fr)[0]] ** 2
                    assert np.abs(pw[b, t, :NBINS] - flat).max() <= STFT_BOUND * 2 * flat, f"clip {b} frame {t}: not (x w[n])^2"
    measured("stft", f"{kind}.hop{hop}.n{N}", worst, STFT_BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize("sr_in,ns", [(22000, (1467, 1468, 1025)), (24000, (1600, 1601, 1118))])
def test_stft_power_lens(hip, sr_in, ns):
    """Resampled lengths 1467 and 1468 (two and three frames: the boundary) and the minimum 1025 in one block, ns at the input rate as
    production passes it; NaN beyond every clip's own samples.  Valid rows = the uniform kernel on the clip alone, the rows beyond = +0.0."""
    _lib, lib, _, handle = hip
    h = handle(sr_in, 22000, 30)
    lens = [int(lib.ts_mfcc_resampled_len(h, n)) for n in ns]
    assert lens == [1467, 1468, 1025]
    N, hop = max(lens), 734
    T = N // hop + 1
    x = stft_inputs("noise", N, 5)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    nh, nhp, nd = i32(ns)
    r = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_stft_lens(h, p["x"], nhp, _lib.dptr(nd), 3, N, p["pw"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"pw": ((3 * T, NPAD), F32)})
    pw = r["pw"].cpu().numpy().reshape(3, T, NPAD)
    worst = 0.0
    for b, n in enumerate(lens):
        Tb = n // hop + 1
        alone = stft_run(hip, h, hop, np.ascontiguousarray(x[b:b + 1, :n]))[0]
        assert np.array_equal(bits(pw[b, :Tb]), bits(alone)), f"clip {b}: its rows differ from the uniform kernel on the clip alone"
        assert (bits(pw[b, Tb:]) == 0).all(), f"clip {b}: a row beyond its {Tb} frames is not +0.0"
        worst = max(worst, stft_error(pw[b, :Tb, :NBINS], x[b, :n], hop))
    measured("stft", f"lens.{sr_in}", worst, STFT_BOUND)


@pytest.mark.gpu
def test_stft_refuses_short_clips(hip):
    _lib, lib, _, handle = hip
    x, pw = torch.zeros(1, 1024, device="cuda"), torch.zeros(2, NPAD, device="cuda")
    assert lib.ts_debug_mfcc_stft(handle(22000, 22000, 30), _lib.dptr(x), 1, 1024, _lib.dptr(pw), _lib.stream_ptr()) != 0
    assert b"clip shorter than half an FFT window (reflect padding undefined)" in lib.ts_last_error()
    nh, nhp, nd = i32([1024])
    assert lib.ts_debug_mfcc_stft_lens(handle(22000, 22000, 30), _lib.dptr(x), nhp, _lib.dptr(nd), 1, 1024, _lib.dptr(pw), _lib.stream_ptr()) != 0
    assert b"clip shorter than half an FFT window (reflect padding undefined)" in lib.ts_last_error()


# ----------------------------------------------------------------------------------------------- dB / top_db
def db_run(hip, p, frames=None):
    _lib, lib, _, handle = hip
    B, T = p.shape[:2]
    fd = i32(frames)[2] if frames is not None else None
    return run_inplace(lambda ptr: _lib.check(lib.ts_debug_mfcc_db(handle(22000, 22000, 30), ptr, _lib.dptr(fd), B, T, _lib.stream_ptr())),
                       p).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 7])
def test_db_topdb(hip, T):
    """Three clips whose maxima lie more than 80 dB apart (a maximum taken across clips clamps a whole clip flat), the maximum in each of the
    four waves' share and in the last element; T = 1: one element per thread."""
    worst = 0.0
    for where in (5, 64 + 17, 128 + 63, 192 + 1, -1):
        p = db_inputs(T, where, 10 * T + where % 7)
        got = db_run(hip, p)
        ref = db_ref(p)
        worst = max(worst, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        quiet = p.copy()                                  # the same clips with nothing to clamp: every element under the floor raised to the top
        for b in range(3):
            g, r = got[b].reshape(-1), ref[b].reshape(-1)
            assert int(g.argmax()) == where % g.size, f"T {T} where {where} clip {b}: the maximum moved"
            lo = np.float32(g.max() - np.float32(80.0))
            raw = 10.0 * np.log10(np.maximum(p[b].reshape(-1).astype(F64), 1e-10))
            under = raw < raw.max() - 80.0 - 1e-3         # clamped for certain (clip 2, whose maximum is -60 dB, has none: -100 dB is its lowest)
            assert under.any() == (b < 2)
            if under.any():
                assert g.min() == lo, f"T {T} where {where} clip {b}: the floor is not fl32(max - 80) of the clip's own maximum"
                assert (g[under] == lo).all()
            else:
                assert g.min() > lo
            quiet[b].reshape(-1)[g <= lo] = p[b].max()
        free = db_run(hip, quiet)
        keep = got > (got.reshape(3, -1).max(1) - np.float32(80.0))[:, None, None]
        assert np.array_equal(bits(got[keep]), bits(free[keep])), f"T {T} where {where}: the clamp pass touched an element above the floor"
    measured("db", f"T{T}", worst, DB_BOUND)


@pytest.mark.gpu
def test_db_topdb_lens(hip):
    """Rows beyond frames[b] hold NaN: they must not move the maximum and come out +0.0; the valid rows are the uniform kernel on the clip alone."""
    T, frames = 7, [7, 1, 4]
    p = db_inputs(T, 77, 3)
    for b, f in enumerate(frames):
        p[b, f:] = np.nan
        p[b, 0, 77] = p[b, :f].max() * 2
    got = db_run(hip, p, frames)
    ref = db_ref(np.nan_to_num(p), frames)
    worst = 0.0
    for b, f in enumerate(frames):
        alone = db_run(hip, np.ascontiguousarray(p[b:b + 1, :f]))
        assert np.array_equal(bits(got[b, :f]), bits(alone[0])), f"clip {b}: its rows differ from the uniform kernel on the clip alone"
        assert (bits(got[b, f:]) == 0).all(), f"clip {b}: a row beyond its {f} frames is not +0.0"
        worst = max(worst, float((np.abs(got[b, :f] - ref[b, :f]) / np.maximum(np.abs(ref[b, :f]), 1.0)).max()))
    measured("db", "lens", worst, DB_BOUND)


# ----------------------------------------------------------------------------------------------- mel and DCT: the tables, the GEMMs
def gemm_run(hip, which, h, x, B, T, frames=None):
    _lib, lib, _, _ = hip
    fn, n = (lib.ts_debug_mfcc_mel, NMELS) if which == "mel" else (lib.ts_debug_mfcc_dct, NMFCC)
    fd = i32(frames)[2] if frames is not None else None
    r = run_both(lambda p: _lib.check(fn(h, p["x"], _lib.dptr(fd), B, T, p["out"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"out": ((B * T, n), F32)})
    return r["out"].cpu().numpy()


def table_close(got, ref):
    return np.abs(np.asarray(got, F64) - ref) <= TABLE_REL * np.abs(ref) + TABLE_ABS


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [22000, 16000])
def test_device_tables(hip, sr):
    """One-hot power rows return the columns of the device's filterbank, one-hot mel rows the DCT matrix: exactly (1 w plus zeros)."""
    h = hip[3](sr, sr, 30)
    onehot = np.zeros((NBINS, NPAD), np.float32)
    onehot[np.arange(NBINS), np.arange(NBINS)] = 1.0
    fb = gemm_run(hip, "mel", h, onehot, 1, NBINS)
    ref = mel_fbanks(sr)
    bad = ~table_close(fb, ref)
    assert not bad.any(), f"filterbank: {int(bad.sum())} entries off, the worst by {np.abs(fb - ref).max():.3e} at {np.argwhere(bad)[:4].tolist()}"
    assert (fb >= 0).all()
    d = gemm_run(hip, "dct", h, np.eye(NMELS, dtype=np.float32), 1, NMELS)
    ref = dct_matrix()
    bad = ~table_close(d, ref)
    assert not bad.any(), f"DCT: {int(bad.sum())} entries off, the worst by {np.abs(d - ref).max():.3e} at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [22000, 16000])
def test_mel_and_dct_gemm(hip, sr):
    """A noise block through both GEMMs against float64 tables, in units of sum |x w|; the masked form on a frame table with NaN rows."""
    h = hip[3](sr, sr, 30)
    rng = np.random.default_rng(sr)
    B, T, frames = 3, 13, [13, 1, 6]
    for which, K, W, bound in (("mel", NPAD, mel_fbanks(sr), MEL_BOUND), ("dct", NMELS, dct_matrix(), DCT_BOUND)):
        if which == "mel":
            x = np.zeros((B * T, NPAD), np.float32)
            x[:, :NBINS] = rng.standard_normal((B * T, NBINS)) ** 2 * 10.0 ** rng.uniform(-3, 3, (B * T, 1))
        else:
            x = (30.0 * rng.standard_normal((B * T, NMELS))).astype(np.float32)
        kx = x[:, :W.shape[0]].astype(F64)
        got = gemm_run(hip, which, h, x, B, T)
        e = in_units(np.abs(got - kx @ W), np.abs(kx) @ np.abs(W))
        measured(which, f"noise.{sr}", e, bound, gemm_ceiling(K))
        xm = x.reshape(B, T, -1).copy()
        for b, f in enumerate(frames):
            xm[b, f:] = np.nan
        gm = gemm_run(hip, which, h, xm.reshape(B * T, -1), B, T, frames).reshape(B, T, -1)
        for b, f in enumerate(frames):
            assert np.array_equal(bits(gm[b, :f]), bits(got.reshape(B, T, -1)[b, :f])), f"{which} clip {b}: masked rows differ from the unmasked launch"
            assert (bits(gm[b, f:]) == 0).all(), f"{which} clip {b}: a row beyond its {f} frames is not +0.0"


# ----------------------------------------------------------------------------------------------- polyphase resampler
def poly_lengths(sr_in):
    """N = 1, N under `width`, the N that give 256 outputs and 257 (where no N gives 257: the fewest over 256) — one and two blocks —, N ~ 3000."""
    orig, new, _, width, _ = poly_params(sr_in, 22000)
    n_out = lambda n: -(-new * n // orig)
    n256 = next(n for n in range(1, 4000) if n_out(n) == 256)
    n257 = next(n for n in range(1, 4000) if n_out(n) > 256)
    return [1, width - 2, n256, n257, 3001]


@pytest.mark.gpu
@pytest.mark.parametrize("sr_in", [16000, 24000, 8000, 44100])
def test_resample_polyphase(hip, sr_in):
    """16 k and 24 k: the LDS kernel; 8 k: up-sampling; 44.1 k: the plain kernel (220 x 467 taps).  Noise, and unit impulses at samples 0 and
    N - 1 that read the table's edge taps back."""
    _lib, lib, _, handle = hip
    h = handle(sr_in, 22000, 30)
    orig, new, _, width, kw = poly_params(sr_in, 22000)
    assert (kw, new) == {16000: (22, 11), 24000: (26, 11), 8000: (18, 11), 44100: (467, 220)}[sr_in]
    rng = np.random.default_rng(sr_in)
    worst = 0.0
    for N in poly_lengths(sr_in):
        n_out = int(lib.ts_mfcc_resampled_len(h, N))
        assert n_out == -(-new * N // orig)
        imp = np.zeros((2, N), np.float32)
        imp[0, 0], imp[1, N - 1] = 1.0, 1.0
        for x in (rng.standard_normal((2, N)).astype(np.float32) * np.float32(0.3), imp):
            r = run_both(lambda p: _lib.check(lib.ts_mfcc_resample(h, p["x"], 2, N, p["out"], _lib.stream_ptr())),
                         {"x": (x, F32)}, {"out": ((2, n_out), F32)})
            got = r["out"].cpu().numpy()
            for b in range(2):
                ref, unit = poly_ref(x[b], sr_in, 22000)
                err = np.maximum(np.abs(got[b] - ref) - kw * F32_TINY * np.abs(x[b]).max(), 0.0)
                worst = max(worst, in_units(err, unit))
    measured("poly", str(sr_in), worst, POLY_BOUND, poly_ceiling(kw))


@pytest.mark.gpu
@pytest.mark.parametrize("sr_in", [16000, 44100])
def test_resample_polyphase_mixed(hip, sr_in):
    """The length variants (LDS and plain) with NaN beyond each clip: the clip's samples = the uniform kernel on the clip alone, +0.0 beyond."""
    _lib, lib, _, handle = hip
    h = handle(sr_in, 22000, 30)
    ns = [700, 1, 187, 333]
    N = max(ns)
    n_out = int(lib.ts_mfcc_resampled_len(h, N))
    x = np.random.default_rng(1).standard_normal((4, N)).astype(np.float32)
    for b, n in enumerate(ns):
        x[b, n:] = np.nan
    nh, nhp, nd = i32(ns)
    r = run_both(lambda p: _lib.check(lib.ts_mfcc_resample_mixed(h, p["x"], nhp, _lib.dptr(nd), 4, N, p["out"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"out": ((4, n_out), F32)})
    got = r["out"].cpu().numpy()
    for b, n in enumerate(ns):
        nb = int(lib.ts_mfcc_resampled_len(h, n))
        xb = np.ascontiguousarray(x[b:b + 1, :n])
        a = run_both(lambda p: _lib.check(lib.ts_mfcc_resample(h, p["x"], 1, n, p["out"], _lib.stream_ptr())), {"x": (xb, F32)}, {"out": ((1, nb), F32)})
        assert np.array_equal(bits(got[b, :nb]), bits(a["out"].cpu().numpy()[0])), f"clip {b}: differs from the uniform kernel on the clip alone"
        assert (bits(got[b, nb:]) == 0).all(), f"clip {b}: a sample beyond its {nb} is not +0.0"


# ----------------------------------------------------------------------------------------------- Kaiser resampler
KAISER_CASES = [(22050, 200), (22050, 20000), (44100, 3), (44100, 441), (44100, 200), (44100, 20000), (48000, 200), (48000, 20000),
                (8000, 200), (8000, 20000)]


@pytest.mark.gpu
@pytest.mark.parametrize("sr_in,N", KAISER_CASES)
def test_resample_kaiser(hip, sr_in, N):
    """N = 3 at 44.1 k: one output sample; 441: exactly 160, no fix_length sample; 200: both wings of every output cut by the clip's ends;
    20000: interior outputs with full wings.  Noise, and impulses at 0 and N - 1."""
    _lib, lib, ctx, _ = hip
    n_fix, n_res = int(lib.ts_resample_kaiser_len(N, sr_in, 16000)), int(N * (16000 / sr_in))
    assert n_fix == math.ceil(N * 16000 / sr_in) and n_fix - n_res in (0, 1)
    if (sr_in, N) == (44100, 3):
        assert (n_res, n_fix) == (1, 2)
    if (sr_in, N) == (44100, 441):
        assert n_res == n_fix == 160
    rng = np.random.default_rng(sr_in + N)
    imp = np.zeros((2, N), np.float32)
    imp[0, 0], imp[1, N - 1] = 1.0, 1.0
    worst = 0.0
    for x in (rng.standard_normal((2, N)).astype(np.float32) * np.float32(0.3), imp):
        r = run_both(lambda p: _lib.check(lib.ts_resample_kaiser(ctx, p["x"], 2, N, sr_in, 16000, p["out"], _lib.stream_ptr())),
                     {"x": (x, F32)}, {"out": ((2, n_fix), F32)})
        got = r["out"].cpu().numpy()
        assert (bits(got[:, n_res:]) == 0).all(), "the fix_length sample is not +0.0"
        for b in range(2):
            ref, unit = kaiser_ref(x[b], sr_in, 16000)
            worst = max(worst, in_units(np.abs(got[b] - ref), unit))
    measured("kaiser", f"{sr_in}.n{N}", worst, KAISER_BOUND, KAISER_CEILING)


@pytest.mark.gpu
def test_resample_kaiser_mixed(hip):
    _lib, lib, ctx, _ = hip
    ns, sr_in = [700, 3, 441, 200], 44100
    N = max(ns)
    n_fix = int(lib.ts_resample_kaiser_len(N, sr_in, 16000))
    x = np.random.default_rng(2).standard_normal((4, N)).astype(np.float32)
    for b, n in enumerate(ns):
        x[b, n:] = np.nan
    nh, nhp, nd = i32(ns)
    r = run_both(lambda p: _lib.check(lib.ts_resample_kaiser_mixed(ctx, p["x"], nhp, _lib.dptr(nd), 4, N, sr_in, 16000, p["out"], _lib.stream_ptr())),
                 {"x": (x, F32)}, {"out": ((4, n_fix), F32)})
    got = r["out"].cpu().numpy()
    for b, n in enumerate(ns):
        nb, nr = int(lib.ts_resample_kaiser_len(n, sr_in, 16000)), int(n * (16000 / sr_in))
        xb = np.ascontiguousarray(x[b:b + 1, :n])
        a = run_both(lambda p: _lib.check(lib.ts_resample_kaiser(ctx, p["x"], 1, n, sr_in, 16000, p["out"], _lib.stream_ptr())),
                     {"x": (xb, F32)}, {"out": ((1, nb), F32)})
        assert np.array_equal(bits(got[b, :nb]), bits(a["out"].cpu().numpy()[0])), f"clip {b}: differs from the uniform kernel on the clip alone"
        assert (bits(got[b, nr:]) == 0).all(), f"clip {b}: a sample beyond its {nr} is not +0.0"


# ----------------------------------------------------------------------------------------------- the stages chained = production
@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True])
def test_stages_chained_equal_production(hip, mixed):
    """B = 2 at 16 kHz, 0.3 s: resampler, STFT, mel, dB, DCT one after the other through the entries = the bits of ts_mfcc_forward; with lengths
    4800 and 3000 the length variants = the bits of ts_mfcc_forward_mixed."""
    _lib, lib, _, handle = hip
    h = handle(16000, 22000, 30)
    B, N = 2, 4800
    ns = [4800, 3000] if mixed else [N, N]
    wav = (0.3 * np.random.default_rng(8).standard_normal((B, N))).astype(np.float32)
    for b, n in enumerate(ns):
        wav[b, n:] = np.nan
    N22, T = int(lib.ts_mfcc_resampled_len(h, N)), int(lib.ts_mfcc_num_frames(h, N))
    nh, nhp, nd = i32(ns)
    s = _lib.stream_ptr()
    if mixed:
        prod = run_both(lambda p: _lib.check(lib.ts_mfcc_forward_mixed(h, p["wav"], nhp, _lib.dptr(nd), B, N, p["feat"], s)),
                        {"wav": (wav, F32)}, {"feat": ((B, T, NMFCC), F32)})["feat"].cpu().numpy()
        fd = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.ts_debug_mfcc_frames(h, _lib.dptr(nd), B, N, _lib.dptr(fd), s))
        frames = fd.cpu().numpy()
        assert frames.tolist() == [int(lib.ts_mfcc_num_frames(h, n)) for n in ns]
        fdp = _lib.dptr(fd)
        x22 = run_both(lambda p: _lib.check(lib.ts_mfcc_resample_mixed(h, p["wav"], nhp, _lib.dptr(nd), B, N, p["out"], s)),
                       {"wav": (wav, F32)}, {"out": ((B, N22), F32)})["out"].cpu().numpy()
        pw = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_stft_lens(h, p["x"], nhp, _lib.dptr(nd), B, N22, p["pw"], s)),
                      {"x": (x22, F32)}, {"pw": ((B * T, NPAD), F32)})["pw"].cpu().numpy()
    else:
        fdp = None
        prod = run_both(lambda p: _lib.check(lib.ts_mfcc_forward(h, p["wav"], B, N, p["feat"], s)),
                        {"wav": (wav, F32)}, {"feat": ((B, T, NMFCC), F32)})["feat"].cpu().numpy()
        x22 = run_both(lambda p: _lib.check(lib.ts_mfcc_resample(h, p["wav"], B, N, p["out"], s)),
                       {"wav": (wav, F32)}, {"out": ((B, N22), F32)})["out"].cpu().numpy()
        pw = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_stft(h, p["x"], B, N22, p["pw"], s)),
                      {"x": (x22, F32)}, {"pw": ((B * T, NPAD), F32)})["pw"].cpu().numpy()
    mel = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_mel(h, p["x"], fdp, B, T, p["out"], s)),
                   {"x": (pw, F32)}, {"out": ((B * T, NMELS), F32)})["out"].cpu().numpy()
    db = run_inplace(lambda ptr: _lib.check(lib.ts_debug_mfcc_db(h, ptr, fdp, B, T, s)), mel.reshape(B, T, NMELS)).cpu().numpy()
    feat = run_both(lambda p: _lib.check(lib.ts_debug_mfcc_dct(h, p["x"], fdp, B, T, p["out"], s)),
                    {"x": (db.reshape(B * T, NMELS), F32)}, {"out": ((B * T, NMFCC), F32)})["out"].cpu().numpy()
    assert np.isfinite(prod).all()
    assert np.array_equal(bits(feat.reshape(B, T, NMFCC)), bits(prod)), "the stages chained differ from the production entry"


# ----------------------------------------------------------------------------------------------- CPU: the references, the bounds
def test_references_against_third_party():
    """The float64 references against installed third-party implementations of the same definitions (none is torchaudio or resampy, which
    are absent): torch.stft in float64, transformers' mel_filter_bank, scipy's DCT; the resamplers' references by their unit DC gain and an impulse read back."""
    from scipy.fft import dct
    from transformers import audio_utils as au
    x = np.random.default_rng(0).standard_normal(5000)
    for hop in (734, 1467):
        spec = torch.stft(torch.from_numpy(x), n_fft=NFFT, hop_length=hop, win_length=NFFT, window=torch.hann_window(NFFT, periodic=True, dtype=torch.float64),
                          center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        P, aX, _ = stft_ref(x, hop)
        assert P.shape == (5000 // hop + 1, NBINS) and np.abs(P - spec.abs().pow(2).T.numpy()).max() <= 1e-9 * P.max()
    fr = np.random.default_rng(1).standard_normal((3, NFFT))
    assert np.abs(rfft_last_pass(fr) - np.fft.rfft(fr, axis=1)).max() <= 1e-10
    for sr in (22000, 16000):
        assert np.abs(mel_fbanks(sr) - au.mel_filter_bank(NBINS, NMELS, 0.0, float(sr // 2), sr, None, "htk")).max() <= 1e-9
    v = np.random.default_rng(2).standard_normal((5, NMELS))
    assert np.abs(v @ dct_matrix() - dct(v, type=2, norm="ortho", axis=1)[:, :NMFCC]).max() <= 1e-12
    # the polyphase kernel: unit DC gain (every phase sums to ~1 after the 0.99 roll-off) and the impulse response read back
    for sr_in in (16000, 44100, 8000):
        k = poly_kernel(sr_in, 22000)
        assert np.abs(k.sum(1) - 1.0).max() < 2e-2
        orig, new, _, width, kw = poly_params(sr_in, 22000)
        imp = np.zeros(64)
        imp[10] = 1.0
        y, _ = poly_ref(imp, sr_in, 22000)
        j = np.arange(y.size)
        tap = 10 + width - (j // new) * orig
        ok = (tap >= 0) & (tap < kw)
        assert np.array_equal(y[ok], k[j[ok] % new, tap[ok]]) and (y[~ok] == 0).all()
    # the Kaiser interpolation: unit DC gain away from the ends, for both directions
    for sr_in in (44100, 8000):
        y, _ = kaiser_ref(np.ones(4000), sr_in, 16000)
        mid = y[y.size // 3:2 * y.size // 3]
        assert np.abs(mid - 1.0).max() < 1e-2


def test_table_tolerance_derivation():
    """The two terms of the table tolerance.  (a) Rounding a float64 table to fp32 moves an entry by at most 2^-24 |ref|.  (b) Another libm
    moves the float64 value itself by far less than 1e-11: the same formulas in 80-bit arithmetic differ from the float64 ones by < 1e-12,
    largest at the triangles' corners, where (f - f_j) / (f_j+1 - f_j) cancels."""
    for sr in (22000, 16000):
        fb = mel_fbanks(sr)
        assert (np.abs(fb.astype(np.float32).astype(F64) - fb) <= TABLE_REL * np.abs(fb)).all()
        if np.finfo(np.longdouble).eps < 1e-18:
            d = float(np.abs(mel_fbanks(sr, dtype=np.longdouble) - fb).max())
            print(f"\n[tables] filterbank {sr}: 80-bit against 64-bit {d:.2e}")
            assert d <= TABLE_ABS / 10
    d64 = dct_matrix()
    assert (np.abs(d64.astype(np.float32).astype(F64) - d64) <= TABLE_REL * np.abs(d64)).all()
    if np.finfo(np.longdouble).eps < 1e-18:
        assert float(np.abs(dct_matrix(dtype=np.longdouble) - d64).max()) <= TABLE_ABS / 10


# defect -> the stage whose bound catches it
DEFECTS = {"hann_symmetric": "stft", "reflect_repeats_edge": "stft", "bin_1024_from_bin_0": "stft", "twiddle_index": "stft", "hop_733": "stft",
           "max_over_block": "db", "floor_1e-9": "db", "width_shift": "poly", "k_max_short": "kaiser", "dct_row0_unscaled": "tables",
           "slaney_mel_points": "tables"}


def test_bounds_catch_defects():
    """Each defect, applied to the float64 reference on inputs of the GPU tests, moves the result by at least 10x the bound of its stage."""
    moved = {}
    clips = [x for kind in STFT_KINDS for x in stft_inputs(kind, 5000, 1)]          # what test_stft_power runs at N = 5000
    for d in ("hann_symmetric", "reflect_repeats_edge", "hop_733", "twiddle_index", "bin_1024_from_bin_0"):
        moved[d] = max(stft_error(stft_ref(x, 734, d)[0], x, 734) for x in clips)
    p = db_inputs(2, 5, 1)
    for d in ("max_over_block", "floor_1e-9"):
        ref = db_ref(p)
        moved[d] = float((np.abs(db_ref(p, defect=d) - ref) / np.maximum(np.abs(ref), 1.0)).max())
    xn = np.random.default_rng(3).standard_normal(300)
    ref, unit = poly_ref(xn, 16000, 22000)
    moved["width_shift"] = in_units(np.abs(poly_ref(xn, 16000, 22000, "width_shift")[0] - ref), unit)
    ref, unit = kaiser_ref(xn[:200], 44100, 16000)
    moved["k_max_short"] = in_units(np.abs(kaiser_ref(xn[:200], 44100, 16000, "k_max_short")[0] - ref), unit)
    bounds = {"stft": STFT_BOUND, "db": DB_BOUND, "poly": POLY_BOUND, "kaiser": KAISER_BOUND}
    assert set(moved) | {"dct_row0_unscaled", "slaney_mel_points"} == set(DEFECTS)
    for d, e in moved.items():
        b = bounds[DEFECTS[d]]
        print(f"\n[defect] {d}: {e:.3e} = {e / b:.0f} x the {DEFECTS[d]} bound {b:.1e}")
        assert e >= 10 * b, f"{d} moves the result by {e:.2e} only, under 10x the {DEFECTS[d]} bound {b:.1e}"
    # the tables: the defect against the table tolerance at the entry it moves most
    for d, good, bad in (("dct_row0_unscaled", dct_matrix(), dct_matrix("dct_row0_unscaled")),
                         ("slaney_mel_points", mel_fbanks(22000), mel_fbanks(22000, "slaney"))):
        ratio = float((np.abs(bad - good) / (TABLE_REL * np.abs(good) + TABLE_ABS)).max())
        print(f"\n[defect] {d}: {ratio:.2e} x the table tolerance")
        assert ratio >= 10


def test_bounds_under_every_ceiling():
    for b, c in ((MEL_BOUND, gemm_ceiling(NPAD)), (DCT_BOUND, gemm_ceiling(NMELS)), (KAISER_BOUND, KAISER_CEILING)):
        assert b <= c
    for sr_in in (16000, 24000, 8000, 44100):
        assert POLY_BOUND <= poly_ceiling(poly_params(sr_in, 22000)[4])
