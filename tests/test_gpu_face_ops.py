"""Op-level tests of the face generator's kernels, one by one, against float64 restatements of the same operation on the same fp32
inputs: the non-GEMM kernels of `csrc/face.hip` (fused attention, row LayerNorm, 50 -> 30 fps interpolation + LayerNorm, conv0 +
GroupNorm + GELU in both statistics forms, the id channels), the GELU epilogue (`csrc/kernels.h::gelu_fast`) and the opt-in split-bf16
GEMM (`csrc/conv_gemm_split.hip`), through the test entry points of `include/talkshow_hip_debug.h`.

Every float bound has two parts.  The CEILING comes from fp32 error analysis, is written in the test's docstring and is scaled to the
regime (the comparisons divide the error by that scale: |mean| * rstd for the normalisations, max |v| for attention, sum |x||w| for the
GEMM).  The asserted BOUND is at most 2x the largest error measured on the MI355X (TS_MEASURED_LOG), as everywhere in this suite, and
sits under the ceiling.  Every bound is also shown to catch a plausible defect: the defect is applied to the float64 reference on the
CPU and must miss the bound by at least 10x (`_catches`).
"""
import math
import os

import numpy as np
import pytest
import torch
from scipy.special import erf

from conftest import assert_close_measured
from oracle import face_oracle as FO

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    lib = _lib.load()
    ctx = _lib.context(0)
    return _lib, lib, ctx


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _run(_lib, rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def _scaled_close(name, got, ref, scale, bound):
    """assert_close_measured on the error divided by the regime's scale (the ceiling's unit)."""
    got64 = np.asarray(got, F64)
    assert np.isfinite(got64).all(), f"{name}: non-finite output"
    assert_close_measured(name, got64 / scale, np.asarray(ref, F64) / scale, bound)


def _catches(name, defect, ref, scale, bound):
    """A plausible defect, applied to the float64 reference, must move it by at least 10x the bound (in the same units)."""
    err = float(np.max(np.abs(np.asarray(defect, F64) - np.asarray(ref, F64)) / scale))
    print(f"\n[defect] {name}: {err:.3e} = {err / bound:.0f} x the bound {bound:.1e}")
    assert err >= 10 * bound, f"{name}: the defect moves the result by {err:.2e} only, under 10x the bound {bound:.1e}"


def gelu64(v):
    return 0.5 * v * (1.0 + erf(v / math.sqrt(2.0)))


# ----------------------------------------------------------------------------------------------- attention
# (heads, B): B * heads = 8 and 24 (multiples of the 8 XCDs the kernel's grid deals (clip, head) pairs to) and 3, 12 (not)
ATT_CFG = ((1, 8), (1, 3), (12, 2), (12, 1))
ATT_T = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 128, 129, 300, 1800)
# bounds on max |err| / max |v|, 2x the largest error measured on the MI355X over each regime's cases: synthetic 7.3e-7 (T = 1 800, 12 heads),
# equal scores 2.8e-8, late peak 2.2e-10, underflow 5.4e-7, V offset 2.95e-6 (T = 1 800)
ATT_BOUND = {"synthetic": 1.4e-6, "equal_scores": 5e-8, "late_peak": 4e-10, "underflow": 1e-6, "v_offset": 5.8e-6}


def _att_rows(T, rng):
    """Query rows restated in float64: all of them up to T = 300, else the first and last 64 and 128 in between."""
    if T <= 300:
        return np.arange(T)
    return np.unique(np.concatenate([np.arange(64), np.arange(T - 64, T), rng.integers(0, T, 128)]))


def att_ref(qkv, heads, rows, scale=0.125, defect=None):
    """float64 softmax(q k^T scale) v per (clip, head) of qkv (B, T, 3 HID) for the query `rows` -> (B, len(rows), HID).
    defect: 'padding_key' (the tile's zero padding keys join the soft-max: score 0, value 0), 'temperature' (scores x log2 e),
    'last_key' (the last key dropped)."""
    B, T, _ = qkv.shape
    x = qkv.astype(F64).reshape(B, T, 3, heads, 64).transpose(2, 0, 3, 1, 4)     # (3, B, heads, T, 64)
    q, k, v = x[0][:, :, rows], x[1], x[2]
    s = q @ k.transpose(0, 1, 3, 2) * scale
    if defect == "temperature":
        s = s * math.log2(math.e)
    elif defect == "last_key":
        s, v = s[..., :-1], v[:, :, :-1]
    elif defect == "padding_key":
        npad = (-T) % 64
        s = np.concatenate([s, np.zeros(s.shape[:-1] + (npad,))], -1)
        v = np.concatenate([v, np.zeros(v.shape[:2] + (npad, 64))], 2)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    o = p @ v                                                                       # (B, heads, rows, 64)
    return o.transpose(0, 2, 1, 3).reshape(B, len(rows), heads * 64)


def att_run(hip, qkv, heads):
    _lib, lib, _ = hip
    B, T, _ = qkv.shape
    qd = dev(qkv)
    out = nans(B, T, heads * 64)
    _run(_lib, lib.ts_debug_attention(_lib.dptr(qd), B, T, heads * 64, heads, 0.125, _lib.dptr(out), None))
    return out


def qkv_case(regime, B, T, heads, rng):
    """(B, T, 3 HID) fp32 inputs of one score regime."""
    x = rng.standard_normal((B, T, 3, heads, 64))
    if regime in ("synthetic", "v_offset"):
        x[:, :, :2] *= math.sqrt(2.0)              # scores q.k / 8 of std 2, like the synthetic weights' (q / k gain 1.3 after LN)
        if regime == "v_offset":
            x[:, :, 2] += 1000.0                    # a normaliser error e shows as 1000 e
    elif regime == "equal_scores":
        x[:, :, 1] = x[:, :1, 1]                    # one key row for every key: every score of a query is the same
    elif regime == "late_peak":
        # query i has ONE dominant key (score ~30 above the rest) in the last key tile: the running max jumps there, the rescale
        # factor exp(m_old - m_new) is ~1e-13
        x[:, :, :2] *= 0.3
        nlast = T - 64 * ((T - 1) // 64)
        ndir = min(16, nlast)
        a = math.sqrt(30.0 / 0.125)
        for i in range(T):
            x[:, i, 0, :, i % ndir] = a
        for m in range(ndir):
            x[:, T - 1 - m, 1, :, m] = a
    elif regime == "underflow":
        # every key after tile 0 scores >= 100 below tile 0's (exp(-120): 0 in fp32); key 5 dominates tile 0
        x[:, :, :2] *= 0.5
        x[:, :, 0, :, 0] = 40.0
        x[:, :64, 1, :, 0] = 0.0
        x[:, 64:, 1, :, 0] = -24.0
        x[:, :, 0, :, 1] = 4.0
        x[:, 5, 1, :, 1] = 8.0
    return x.reshape(B, T, 3 * heads * 64).astype(F32)


def _att_check(hip, regime, T, heads, B, rng, defects=()):
    qkv = qkv_case(regime, B, T, heads, rng)
    out = att_run(hip, qkv, heads)
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), f"attention {regime} T={T}: non-finite output"
    v = qkv.reshape(B, T, 3, heads * 64)[:, :, 2]
    if T == 1:                                      # one key: p = 1, l = 1 -> the output IS v, bit for bit
        assert np.array_equal(got, v), f"attention T=1 ({regime}): output differs from V"
    rows = _att_rows(T, rng)
    ref = att_ref(qkv, heads, rows)
    scale = float(np.abs(v).max())
    bound = ATT_BOUND[regime]
    _scaled_close(f"attention.{regime}.T{T}.h{heads}.B{B}", got[:, rows], ref, scale, bound)
    for d in defects:
        if T == 1 or d == "padding_key" and T % 64 == 0:     # one key: every defect gives the same output
            continue
        _catches(f"attention.{regime}.T{T}.{d}", att_ref(qkv, heads, rows, defect=d), ref, scale, bound)
    return qkv, out


@pytest.mark.parametrize("T", ATT_T)
def test_attention_synthetic_scores(hip, T):
    """attention_kernel (fused QK^T -> online soft-max over key tiles of 64 -> PV, fp32 MFMA) against float64 softmax(q k^T / 8) v at every
    key-tile variant (T = 1 .. 129 around the 16-key blocks and 64-key tiles, 300 and 1 800 frames), 1 and 12 heads, B * heads a multiple of
    8 and not; scores of std 2 (the synthetic weights').  Also: a clip's rows are bit-identical alone and inside the batch, two runs give the
    same bits, nothing is non-finite, T = 1 returns V exactly.
    CEILING (error / max |v|): a score carries <= 64 * 2^-24 * sum_d |q_d k_d| / 8 of MFMA rounding, which exp2 turns into the same relative
    error of p; P V and the normaliser add <= (T + 64) 2^-24 -> 2^-17 * max_ij sum_d |q_d k_d| / 8 + (T + 64) 2^-23: ~1.4e-4 at T = 1 800
    here.  Defects: an unmasked padding key, a soft-max temperature off by log2 e, the last key dropped."""
    rng = np.random.default_rng(1000 + T)
    for heads, B in ATT_CFG:
        qkv, out = _att_check(hip, "synthetic", T, heads, B, rng, defects=("padding_key", "temperature", "last_key") if B == 3 or B == 1 else ())
        again = att_run(hip, qkv, heads)
        assert torch.equal(out, again), f"attention T={T} h={heads} B={B}: bits changed between two runs"
        if B > 1:
            for b in (0, B - 1):
                alone = att_run(hip, qkv[b:b + 1], heads)
                assert torch.equal(alone[0], out[b]), f"attention T={T} h={heads}: clip {b} alone differs from clip {b} of a batch of {B}"


@pytest.mark.parametrize("regime,Ts", [("equal_scores", (1, 17, 64, 65, 129, 300)), ("late_peak", (65, 128, 129, 300, 1800)),
                                       ("underflow", (65, 129, 300, 1800)), ("v_offset", (1, 17, 64, 65, 300, 1800))])
def test_attention_score_regimes(hip, regime, Ts):
    """The online soft-max where it can go wrong, against float64: every score of a row equal (output = the mean of V); one dominant key per
    query in the LAST key tile (the running max jumps late: rescale factor ~1e-13); the dominant key in tile 0 with every later key >= 100
    below (their probabilities underflow to exactly 0); V = 1000 + noise (a normaliser error e shows as 1000 e, i.e. as e after the
    scaling by max |v|).  Same ceiling as test_attention_synthetic_scores, with max |score| ~30 / 40 here."""
    rng = np.random.default_rng({"equal_scores": 1, "late_peak": 2, "underflow": 3, "v_offset": 4}[regime])
    for T in Ts:
        for heads, B in ((1, 3), (12, 2)):
            # the defects each regime can see: a soft-max ~30 above the rest hides a padding key or a temperature error (< e^-30), equal
            # scores hide the temperature, keys ~100 below the max hide the last one; under a common offset of 1 000 one key of 1 800 moves
            # the output by ~5e-5 of max |v| (the synthetic regime pins that defect)
            defects = {"equal_scores": ("padding_key", "last_key"), "late_peak": ("last_key",), "underflow": ("padding_key", "temperature"),
                       "v_offset": ("padding_key", "temperature")}[regime] if heads == 1 else ()
            _att_check(hip, regime, T, heads, B, rng, defects=defects)
    if regime == "equal_scores":                    # the restatement itself: equal scores average V
        qkv = qkv_case(regime, 1, 65, 1, rng)
        v = qkv.reshape(1, 65, 3, 64)[:, :, 2].astype(F64)
        assert np.allclose(att_ref(qkv, 1, np.arange(65)), v.mean(1, keepdims=True), atol=1e-12)


# ----------------------------------------------------------------------------------------------- LayerNorm rows
LN_BOUND = 1.7e-6        # on |err| / (1 + |mean| * rstd + |res|); measured 8.8e-7 (C = 512, 19 201 rows, residual + ReLU)
# constant rows: |out - (beta (+ res))| in units of ulp(mean) rstd |gamma| + ulp(out), per C; measured 0.46 / 0.49 / 2.02 / 3.17 (19 201 rows)
LN_CONST_BOUND = {64: 0.9, 256: 0.95, 512: 4.0, 768: 6.3}
ROW_KINDS = ("unit", "small", "offset", "constant")


def ln_rows(rng, M, C):
    """Rows cycling through: unit variance, std 1e-3 (eps = 1e-5 matters), mean 100 x std, constant (output = beta (+ res))."""
    x = np.empty((M, C), F64)
    for m in range(M):
        kind = ROW_KINDS[m % 4]
        r = rng.standard_normal(C)
        x[m] = {"unit": r, "small": 1e-3 * r + 0.01, "offset": 100.0 + r, "constant": np.full(C, rng.uniform(-3, 3))}[kind]
    return x.astype(F32)


def ln_ref(x, g, b, res=None, relu=False, eps=1e-5, ddof=0):
    x64 = x.astype(F64)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).sum(1, keepdims=True) / (x.shape[1] - ddof)
    rstd = 1.0 / np.sqrt(var + eps)
    y = (x64 - mean) * rstd * g + b
    if res is not None:
        y = y + res
    if relu:
        y = np.maximum(y, 0.0)
    scale = 1.0 + np.abs(mean) * rstd + (np.abs(res) if res is not None else 0.0)
    return y, scale


@pytest.mark.parametrize("C", (64, 256, 512, 768))
@pytest.mark.parametrize("M", (1, 3, 4, 5, 19201))
def test_layernorm_rows(hip, C, M):
    """layernorm_rows_kernel (one wavefront per row, fp32 sums over lanes) against float64 nn.LayerNorm (eps 1e-5, biased variance) at every
    channel count, 1 .. 5 rows (the 4-row workgroup's edges) and 19 201, with and without the post-norm residual and ReLU; x, residual and
    output rows pitched wider than C (the pitch's tail must stay untouched).
    CEILING (error / (1 + |mean| rstd + |res|)): the mean's fp32 sum carries <= (C / 64 + 6) 2^-24 |mean| (lane sums, then a 6-level tree),
    which the normalisation multiplies by rstd; the centred values, the variance and the affine step add a few ulp: 32 * 2^-24 = 1.9e-6.
    Constant rows must give beta (+ res): the only error is the fp32 mean's, <= (C / 64 + 7) ulp(mean), times rstd = 1 / sqrt(eps) and
    |gamma|, plus the affine step's rounding: CEILING C / 64 + 9 in units of ulp(mean) rstd |gamma| + ulp(out) (21 at C = 768).
    Defects: eps 1e-6, the unbiased variance; on the constant rows, the residual added before the norm."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(C * 7 + M)
    x = ln_rows(rng, M, C)
    g = (1.0 + 0.1 * rng.standard_normal(C)).astype(F32)
    b = (0.1 * rng.standard_normal(C)).astype(F32)
    res = rng.standard_normal((M, C)).astype(F32)
    ldx, ldr, ldo = C + 4, C + 12, C + 7
    xp = np.full((M, ldx), np.nan, F32)
    xp[:, :C] = x
    rp = np.full((M, ldr), np.nan, F32)
    rp[:, :C] = res
    xd, rd, gd, bd = dev(xp), dev(rp), dev(g), dev(b)
    for post, relu in ((False, 0), (False, 1), (True, 0), (True, 1)):
        out = nans(M, ldo)
        _run(_lib, lib.ts_debug_layernorm_rows(_lib.dptr(xd), ldx, M, C, _lib.dptr(gd), _lib.dptr(bd), _lib.dptr(rd) if post else None,
                                               ldr, relu, _lib.dptr(out), ldo, None))
        got = out.cpu().numpy()
        assert np.isnan(got[:, C:]).all(), "a store landed in the output pitch's tail"
        ref, scale = ln_ref(x, g, b, res if post else None, bool(relu))
        _scaled_close(f"layernorm.C{C}.M{M}.res{int(post)}.relu{relu}", got[:, :C], ref, scale, LN_BOUND)
        if M >= 4:                                  # constant rows give beta (+ res), to a few ulp of the mean times rstd = 316
            const = np.arange(M) % 4 == 3
            ulps = (np.spacing(np.abs(x[const, :1])).astype(F64) / math.sqrt(1e-5) * np.abs(g)
                    + np.spacing(np.abs(ref[const]).astype(F32)).astype(F64))
            assert_close_measured(f"layernorm.C{C}.M{M}.res{int(post)}.relu{relu}.constant_rows_in_ulps", got[const, :C] / ulps,
                                  ref[const] / ulps, LN_CONST_BOUND[C])
            if post:                                # the residual added before the norm (pre-LN) instead of after it
                pre = ln_ref(x.astype(F64) + res, g, b, relu=bool(relu))[0]
                _catches(f"layernorm.C{C}.M{M}.relu{relu}.constant_rows.residual_before_norm", pre[const], ref[const], ulps, LN_CONST_BOUND[C])
        if M >= 4 and not post and not relu:
            _catches(f"layernorm.C{C}.eps_1e-6", ln_ref(x, g, b, eps=1e-6)[0], ref, scale, LN_BOUND)
            _catches(f"layernorm.C{C}.unbiased_variance", ln_ref(x, g, b, ddof=1)[0], ref, scale, LN_BOUND)


# ----------------------------------------------------------------------------------------------- interpolation + LayerNorm(512)
LERP_BOUND = 1.5e-6      # on |err| / (1 + |mean| * rstd); measured 7.9e-7 (2 999 -> 1 800)
LERP_SHAPES = ((499, 300), (49, 30), (2999, 1800), (1, 1), (1, 5), (2, 1), (100, 100), (150, 300), (300, 100), (1499, 900))


def lerp_index(Lin, T, align_corners=False):
    """F.interpolate(mode='linear') source indices and weights.  align_corners=False: ATen's fp32 source index as its AVX2 / AVX512 CPU
    kernels round it (once: oracle/face_oracle.py::source_index(fused=True); tests/test_face_oracle_golden.py pins that to the installed
    torch) — the arithmetic of the reference's face goldens."""
    if not align_corners:
        i0, i1, l0, l1 = FO.source_index(Lin, T, fused=True)
        return i0, i1, l0.astype(F64), l1.astype(F64)
    src = (np.arange(T, dtype=F64) * ((Lin - 1) / (T - 1) if T > 1 else 0.0)).astype(F32)
    i0 = np.floor(src).astype(np.int64)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, np.minimum(i0 + 1, Lin - 1), (F32(1) - l1).astype(F64), l1.astype(F64)


def lerp_ln_ref(x, T, g, b, **kw):
    i0, i1, l0, l1 = lerp_index(x.shape[1], T, **kw)
    v = x[:, i0].astype(F64) * l0[None, :, None] + x[:, i1].astype(F64) * l1[None, :, None]
    B = x.shape[0]
    y, scale = ln_ref(v.reshape(B * T, -1), g, b)
    return y.reshape(B, T, -1), scale.reshape(B, T, 1)


@pytest.mark.parametrize("Lin,T", LERP_SHAPES)
def test_lerp_ln(hip, Lin, T):
    """lerp_ln_kernel (linear_interpolation over time, align_corners = False, fused with LayerNorm(512)) against float64 interpolation with
    ATen's fp32 source indices (as its vectorized CPU kernels round them, which made the reference's goldens) + float64 LayerNorm: 50 -> 30 fps at
    10 s / 1 s / 60 s / 30 s, single frames in and out, equal lengths, upsampling, and 300 -> 100 (source indices land on integers).
    CEILING (error / (1 + |mean| rstd)): the two-term blend rounds once (2^-24 |x| rstd), then LayerNorm(512)'s 14 * 2^-24: 32 * 2^-24 =
    1.9e-6.  Defect: align_corners = True."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(Lin * 3 + T)
    B = 2
    x = (rng.standard_normal((B, Lin, 512)) + rng.standard_normal((B, Lin, 1))).astype(F32)
    g = (1.0 + 0.1 * rng.standard_normal(512)).astype(F32)
    b = (0.1 * rng.standard_normal(512)).astype(F32)
    xd, gd, bd = dev(x), dev(g), dev(b)            # named: a temporary's memory could be reused before the kernel reads it
    out = nans(B, T, 512)
    _run(_lib, lib.ts_debug_lerp_ln(_lib.dptr(xd), B, Lin, T, _lib.dptr(gd), _lib.dptr(bd), _lib.dptr(out), None))
    ref, scale = lerp_ln_ref(x, T, g, b)
    _scaled_close(f"lerp_ln.{Lin}to{T}", out.cpu().numpy(), ref, scale, LERP_BOUND)
    if Lin > 1 and T > 1 and Lin != T:
        _catches(f"lerp_ln.{Lin}to{T}.align_corners", lerp_ln_ref(x, T, g, b, align_corners=True)[0], ref, scale, LERP_BOUND)
    i0, i1, _, _ = lerp_index(Lin, T)
    assert i0.min() >= 0 and i1.max() <= Lin - 1


# ----------------------------------------------------------------------------------------------- conv0 + GroupNorm + GELU
C0_BOUND = 4.3e-7        # on |err| / (1 + |gamma| rstd sum_k |w_k| max |x|); measured 2.15e-7 (both forms, L0 = 79, square wave)
C0_FORMS_BOUND = 3.7e-7  # the two forms against each other, same units; measured 1.88e-7 (L0 = 31 999, square wave)
C0_L0 = (1, 2, 79, 1024, 1025, 31999)
SIGNALS = ("noise", "dc_tone", "silence", "near_silence", "square", "recording")


def _recording_slice(N):
    """A 10 s slice of a committed recording, 16 kHz samples as the real-audio tests derive them (1st-page.wav is native 16 kHz)."""
    from talkshow_amd import frontend as fe
    p = os.path.join(REPO, "tests", "golden", "audio", "1st-page.wav")
    assert os.path.exists(p), f"{p}: the committed recording is missing"
    wav = fe.get_wav16(p, host=True)[:, 0]
    assert wav.shape[0] >= N + 16000
    return np.ascontiguousarray(wav[16000:16000 + N], dtype=F32)


def signal(kind, N, rng):
    t = np.arange(N)
    if kind == "noise":
        return (0.1 * rng.standard_normal(N)).astype(F32)
    if kind == "dc_tone":
        return (0.3 + 0.2 * np.sin(2 * np.pi * 220.0 * t / 16000.0)).astype(F32)
    if kind == "silence":
        return np.zeros(N, F32)
    if kind == "near_silence":
        return (1e-5 * rng.standard_normal(N)).astype(F32)
    if kind == "square":
        return np.where((t // 37) % 2 == 0, 1.0, -1.0).astype(F32)
    if kind == "noise_0.05":
        return (0.05 * rng.standard_normal(N)).astype(F32)
    return _recording_slice(N)


def conv0_ref(x, w, g, b, frames, eps_outside=False):
    """float64 Conv1d(1, 512, 10, stride 5, no bias) -> GroupNorm(512, 512) (eps 1e-5, biased variance over time) -> exact GELU of one clip
    at the given output frames -> (out (len(frames), 512), scale (1, 512))."""
    L0 = (x.shape[0] - 10) // 5 + 1
    win = np.lib.stride_tricks.sliding_window_view(x.astype(F64), 10)[::5][:L0]
    y = win @ w.astype(F64).T
    mean = y.mean(0, keepdims=True)
    var = ((y - mean) ** 2).mean(0, keepdims=True)
    rstd = 1.0 / (np.sqrt(var) + 1e-5) if eps_outside else 1.0 / np.sqrt(var + 1e-5)
    z = (y[frames] - mean) * rstd * g + b
    scale = 1.0 + np.abs(g) * (1.0 / np.sqrt(var + 1e-5)) * np.abs(w.astype(F64)).sum(1) * float(np.abs(x).max())
    return gelu64(z), scale


@pytest.mark.parametrize("L0", C0_L0)
def test_w2v_conv0_groupnorm_gelu(hip, L0):
    """conv0 + GroupNorm(512, 512) + GELU (face.hip: the statistics from the waveform's second moments (form 1, production's default) and
    from a pass that computes the convolution (form 0)) against float64, at L0 = 1, 2, 79, 1 024 / 1 025 (the moments kernel's 1 024-frame
    block edge) and 31 999 (10 s), batches of 1 and 3: white noise, DC offset + tone, silence (output = GELU(beta)), near-silence (1e-5),
    a full-scale +-1 square wave and a 10 s slice of a committed recording.  The two forms agree with each other; a clip gives the same bits
    alone and inside the batch.
    CEILING (error / (1 + |gamma| rstd sum_k |w_k| max |x|)): the statistics are double sums (exact to ~1e-8 relative); the apply pass's
    10 fp32 fmas carry <= 10 * 2^-24 sum_k |w_k x_k|, which the normalisation multiplies by |gamma| rstd, and the GELU adds <= 2^-22:
    16 * 2^-24 = 9.5e-7 + GELU.  Defect: eps outside the square root."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(L0)
    N = 5 * (L0 - 1) + 10 + L0 % 4                  # 0 .. 3 samples that no frame reaches
    w = (0.3 * rng.standard_normal((512, 10))).astype(F32)
    g = (1.0 + 0.1 * rng.standard_normal(512)).astype(F32)
    b = (0.1 * rng.standard_normal(512)).astype(F32)
    wd, gd, bd = dev(w), dev(g), dev(b)
    frames = np.arange(L0) if L0 < 31999 else np.unique(np.concatenate([np.arange(256), np.arange(L0 - 256, L0), np.arange(0, L0, 61)]))
    for batch in (("noise", "dc_tone", "silence"), ("near_silence", "square", "recording" if N >= 160000 else "noise_0.05")):
        wav = np.stack([signal(k, N, rng) for k in batch])
        wavd = dev(wav)
        outs = {}
        for form in (1, 0):
            out = nans(3, L0, 512)
            _run(_lib, lib.ts_debug_w2v_conv0(_lib.dptr(wavd), 3, N, _lib.dptr(wd), _lib.dptr(gd), _lib.dptr(bd), form, _lib.dptr(out), None))
            outs[form] = out
            alone, wav1 = nans(1, L0, 512), dev(wav[1:2])
            _run(_lib, lib.ts_debug_w2v_conv0(_lib.dptr(wav1), 1, N, _lib.dptr(wd), _lib.dptr(gd), _lib.dptr(bd), form, _lib.dptr(alone), None))
            assert torch.equal(alone[0], out[1]), f"conv0 form {form}, L0 {L0}: clip 1 alone differs from clip 1 of a batch of 3"
        for c, kind in enumerate(batch):
            ref, scale = conv0_ref(wav[c], w, g, b, frames)
            for form in (1, 0):
                _scaled_close(f"w2v_conv0.L0_{L0}.{kind}.form{form}", outs[form][c].cpu().numpy()[frames], ref, scale, C0_BOUND)
            _scaled_close(f"w2v_conv0.L0_{L0}.{kind}.moments_vs_direct", outs[1][c].cpu().numpy()[frames], outs[0][c].cpu().numpy()[frames],
                          scale, C0_FORMS_BOUND)
            if kind == "silence":                   # y = 0, var = 0: both forms give GELU(beta) with the same statistics
                assert np.array_equal(outs[1][c].cpu().numpy(), outs[0][c].cpu().numpy())
            if kind in ("noise", "near_silence") and L0 > 1:
                _catches(f"w2v_conv0.L0_{L0}.{kind}.eps_outside_sqrt", conv0_ref(wav[c], w, g, b, frames, eps_outside=True)[0], ref, scale,
                         C0_BOUND)


# ----------------------------------------------------------------------------------------------- id channels
@pytest.mark.parametrize("B,T,nc,nj,ld,col0", [(1, 1, 4, 64, 320, 256), (3, 7, 4, 64, 320, 256), (5, 301, 4, 64, 320, 256),
                                               (64, 1, 4, 64, 320, 256), (2, 1800, 4, 64, 320, 256), (3, 45, 7, 33, 50, 9)])
def test_fill_id(hip, B, T, nc, nj, ld, col0):
    """fill_id_kernel (id_mlp of the one-hot id broadcast over time into columns [col0, col0 + nj) of rows of pitch ld) against float64 at
    ragged B and T; one-hot, zero and dense ids; every frame of a clip bit-identical; the other columns untouched.
    CEILING: nc fp32 fmas: (nc + 1) 2^-24 (|bias| + sum |w id|) <= 3e-6 with these magnitudes.  Bound: 2x the measured 6.55e-7."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(B * 100 + T)
    ids = rng.standard_normal((B, nc)).astype(F32)
    ids[0] = 0.0
    if B > 1:
        ids[1] = np.eye(nc, dtype=F32)[1 % nc]
    w = rng.standard_normal((nj, nc)).astype(F32)
    bias = rng.standard_normal(nj).astype(F32)
    idd, wd, bd = dev(ids), dev(w), dev(bias)
    x = nans(B, T, ld)
    _run(_lib, lib.ts_debug_fill_id(_lib.dptr(idd), nc, _lib.dptr(wd), _lib.dptr(bd), nj, _lib.dptr(x), ld, col0, B, T, None))
    got = x.cpu().numpy()
    assert np.isnan(got[..., :col0]).all() and np.isnan(got[..., col0 + nj:]).all(), "a store landed outside the id columns"
    blk = got[..., col0:col0 + nj]
    assert (blk == blk[:, :1]).all(), "the frames of a clip differ"
    ref = bias.astype(F64) + ids.astype(F64) @ w.astype(F64).T
    assert_close_measured(f"fill_id.B{B}.T{T}.nc{nc}", blk[:, 0], ref, 1.3e-6)
    assert np.array_equal(blk[0, 0], bias), "a zero id gives the bias exactly"


# ----------------------------------------------------------------------------------------------- GELU epilogue
GELU_BOUND = 2.2e-7      # on |err| / max(|v|, 1); measured 1.14e-7
GELU_REL_BOUND = 2.3e-7  # relative error for 1e-30 <= |v| <= 1e-2; measured 1.17e-7


def test_gelu_fast_accuracy(hip):
    """kernels.h::gelu_fast (libm's two-piece erf run branch-free with one v_exp_f32) against float64 GELU: every float32 in windows of
    2^18 around the erf piece boundary |v| = sqrt 2 (both signs), around 0 (zero, the denormals) and around the smallest normal; a
    log-uniform sweep over +-[1e-30, 1e4]; +-0, denormals; NaN propagates.
    CEILING (error / max(|v|, 1)): erf_fast <= 9e-8 of float64 erf (its claim over [-6, 6]), halved by 0.5 v, plus the rounding of
    v / sqrt 2, 1 + erf and the two products (<= 4 ulp of GELU): 9e-8 / 2 + 4 * 2^-24 = 2.8e-7; relative, for |v| <= 1e-2, 4 ulp = 2.4e-7 +
    the polynomial's.  Defect: the tanh approximation."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(9)
    sq2 = int(np.array(math.sqrt(2.0), F32).view(np.int32))
    tiny = int(np.array(np.finfo(F32).tiny, F32).view(np.int32))
    wins = [np.arange(c - 2 ** 17, c + 2 ** 17, dtype=np.int64) for c in (sq2, tiny)] + [np.arange(0, 2 ** 18, dtype=np.int64)]
    pos = np.concatenate(wins).astype(np.int32).view(F32)
    sweep = 10.0 ** rng.uniform(-30, 4, 1 << 20)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 6.0, -6.0, 1e4, -1e4], F64)
    v = np.concatenate([pos, -pos, sweep, -sweep, special]).astype(F32)
    v = np.concatenate([v, np.array([np.nan], F32)])
    vd = dev(v)
    out = torch.empty_like(vd)
    _run(_lib, lib.ts_debug_gelu(_lib.dptr(vd), _lib.dptr(out), v.size, None))
    got = out.cpu().numpy().astype(F64)
    assert np.isnan(got[-1]), "NaN must propagate"
    got, v64 = got[:-1], v[:-1].astype(F64)
    ref = gelu64(v64)
    scale = np.maximum(np.abs(v64), 1.0)
    _scaled_close("gelu_fast.abs_over_max_v_1", got, ref, scale, GELU_BOUND)
    small = (np.abs(v64) >= 1e-30) & (np.abs(v64) <= 1e-2)
    rel = np.abs(got[small] - ref[small]) / np.abs(ref[small])
    assert_close_measured("gelu_fast.rel_small_v", rel, np.zeros_like(rel), GELU_REL_BOUND)
    z = np.where(v64 == 0)[0]
    assert (got[z] == 0).all() and (np.signbit(got[z]) == np.signbit(v64[z])).all(), "GELU(+-0) = +-0"
    near = (np.abs(v64) > 1.3) & (np.abs(v64) < 1.5)
    assert near.sum() >= 2 ** 18, "the window around the erf piece boundary is covered"
    tanh_gelu = 0.5 * v64 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v64 + 0.044715 * v64 ** 3)))
    _catches("gelu_fast.tanh_approximation", tanh_gelu, ref, scale, GELU_BOUND)


# ----------------------------------------------------------------------------------------------- split-bf16 GEMM
# on |err| / (1 + sum_k |x_k w_k|), 2x the largest measured over the shapes: against the float64 emulation of the split arithmetic 1.69e-7
# (2 planes) / 2.23e-7 (3 planes), both on the FFN1 shape (K = 768); against exact float64 3.78e-6 (2 planes, K = 32) / 2.23e-7 (3 planes)
SPLIT_BOUND_EMU = {22: 3.3e-7, 23: 4.4e-7, 24: 3.3e-7}
SPLIT_BOUND_EXACT = {22: 7.5e-6, 23: 4.4e-7, 24: 7.5e-6}
SPLIT_SHAPES = {   # (B, L, Cin, Cout, taps)
    "ragged_225x200": (3, 75, 64, 200, 3),
    "ragged_19227x500": (3, 6409, 64, 500, 3),
    "n39_3taps": (2, 300, 256, 39, 3),
    "k32": (2, 100, 32, 128, 1),
    "tiles199": (1, 199 * 128, 64, 128, 1),
    "tiles200": (1, 200 * 128, 64, 128, 1),
    "face_ffn1": (64, 300, 768, 3072, 1),
}


def bf16_rne(x):
    """fp32 -> the bf16 value (as fp32) nearest, ties to even: v_cvt_pk_bf16_f32."""
    u = x.astype(F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split_planes(x, n):
    """x = x0 + x1 (+ x2): x0 = bf16(x), x1 = bf16 of the exact fp32 remainder, ..."""
    out, r = [], x.astype(F32)
    for _ in range(n):
        h = bf16_rne(r)
        out.append(h)
        r = (r - h).astype(F32)
    return out


def split_emulate(A, W, planes, drop=()):
    """float64 sum of exactly the products the kernel forms: x_i y_j for i + j < planes (`drop`: (i, j) pairs left out)."""
    Ap, Wp = split_planes(A, planes), split_planes(W, planes)
    acc = np.zeros((A.shape[0], W.shape[0]))
    for i in range(planes):
        for j in range(planes - i):
            if (i, j) not in drop:
                acc += Ap[i].astype(F64) @ Wp[j].astype(F64).T
    return acc


def leaky(v):
    return np.where(v >= 0, v, 0.2 * v)


@pytest.mark.parametrize("shape", list(SPLIT_SHAPES), ids=list(SPLIT_SHAPES))
def test_split_bf16_gemm(hip, shape):
    """conv_gemm_split (tile ids 22 / 23: 2 / 3 bf16 planes, 3 / 6 products; 24: 2 planes with the weights as plane images made by
    launch_split_weight_planes, the face's x3 plan) at ragged M and N, N = 39 with 3 taps, K = 32, 199 / 200 tiles of 128 x 128 (either side
    of the 64 x 64 / 128 x 128 variant switch) and the face FFN1 shape, + bias + LeakyReLU (ts_op_conv1d_timed's epilogue), on a sample of
    rows (the first and last 64 and 128 in between):
      * against a float64 EMULATION of the split arithmetic (bf16 round-to-nearest-even planes of the exact remainders, exactly the
        products the kernel forms): only the kernel's fp32 accumulation differs.  CEILING (error / (1 + sum_k |x_k w_k|)): NP products per
        k summed in fp32: 6 K 2^-24 (3.5e-5 at K = 96, 2.7e-4 at K = 768; the sums are not worst-case);
      * against exact float64: CEILING 3 * 2^-16 = 4.6e-5 more for 3 products (each drops terms <= 2^-16 |x w|), fp32 grade for 6;
      * tile 24 bit-identical to tile 22; every tile the same bits in two runs.
    Defect: the x0 y1 product dropped."""
    _lib, lib, ctx = hip
    B, L, Cin, Cout, taps = SPLIT_SHAPES[shape]
    rng = np.random.default_rng(sum(SPLIT_SHAPES[shape]))
    Kt = taps * Cin
    npad = (Cout + 127) // 128 * 128
    x = rng.standard_normal((B, L, Cin)).astype(F32)
    w = np.zeros((npad, Kt), F32)
    w[:Cout] = (rng.standard_normal((Cout, Kt)) / np.sqrt(Kt)).astype(F32)
    bias = np.zeros(npad, F32)
    bias[:Cout] = rng.standard_normal(Cout).astype(F32)
    M = B * L
    rows = np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), rng.integers(0, M, 128)]))
    bi, ti = np.divmod(rows, L)
    A = np.zeros((rows.size, Kt), F32)
    for k in range(taps):
        t = ti + k - taps // 2
        ok = (t >= 0) & (t < L)
        A[ok, k * Cin:(k + 1) * Cin] = x[bi[ok], t[ok]]
    Wc = w[:Cout]
    exact = A.astype(F64) @ Wc.astype(F64).T + bias[:Cout]
    scale = 1.0 + np.abs(A).astype(F64) @ np.abs(Wc).astype(F64).T + np.abs(bias[:Cout])
    xd, wd, bd = dev(x), dev(w), dev(bias)
    outs = {}
    for tile in (22, 23, 24):
        runs = []
        for _ in range(2):
            out = nans(B, L, Cout)
            _run(_lib, lib.ts_op_conv1d_timed(ctx, _lib.dptr(xd), B, L, Cin, _lib.dptr(wd), _lib.dptr(bd), Cout, taps, tile, 0,
                                              _lib.dptr(out), None, None))
            runs.append(out)
        assert torch.equal(runs[0], runs[1]), f"split tile {tile} ({shape}): bits changed between two runs"
        outs[tile] = runs[0]
        planes = 3 if tile == 23 else 2
        got = runs[0].reshape(M, Cout)[torch.from_numpy(rows).cuda()].cpu().numpy()
        emu = split_emulate(A, Wc, planes) + bias[:Cout]
        _scaled_close(f"split_bf16.{shape}.tile{tile}.vs_emulation", got, leaky(emu), scale, SPLIT_BOUND_EMU[tile])
        _scaled_close(f"split_bf16.{shape}.tile{tile}.vs_float64", got, leaky(exact), scale, SPLIT_BOUND_EXACT[tile])
        if tile == 22:
            dropped = split_emulate(A, Wc, 2, drop=((0, 1),)) + bias[:Cout]
            _catches(f"split_bf16.{shape}.x0y1_dropped", leaky(dropped), leaky(emu), scale, SPLIT_BOUND_EMU[tile])
            _catches(f"split_bf16.{shape}.x0y1_dropped.vs_float64", leaky(dropped), leaky(exact), scale, SPLIT_BOUND_EXACT[tile])
    assert torch.equal(outs[24], outs[22]), f"{shape}: the plane-image weights (tile 24) differ from the in-kernel split (tile 22)"


def test_split_bf16_gemm_plain_tile_order(hip):
    """The split kernel with TS_SPLIT_XCD=0 (a plain 2-D tile grid instead of the XCD-aware 1-D order; the knob is read once per process):
    the shapes above that take either variant re-run in a child process, against the same emulation and bounds."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q",
                        "-k", "test_split_bf16_gemm and (ragged_225x200 or ragged_19227x500 or n39_3taps or tiles199 or tiles200)"],
                       env=dict(os.environ, TS_SPLIT_XCD="0"), capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "5 passed" in r.stdout, r.stdout[-2000:]
