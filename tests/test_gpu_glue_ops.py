"""The glue kernels of csrc/vq.hip and the session staging kernels of csrc/body_stream.hip on the GPU, each launched ALONE through its debug
entry (include/talkshow_hip_debug.h) and compared with the restatements of tests/test_glue_host.py.  All comparisons are equality of bits;
row_sqnorm alone has a float bound.

Buffers (the discipline of tests/test_gpu_wino.py::Zoned): every input and every output lies between two 4 KiB zones of sentinel words,
every output starts out sentinel-filled (the code ring starts out as a session's ring), and after the call the zones are intact, the inputs
unchanged and the WHOLE output buffer equals the restatement's image of it — so exactly the elements the contract names have changed.
Floats that are only moved are random uint32 words with NaN payloads, a signalling NaN, denormals and -0.0 among them.  Every case runs
eagerly and once more from a replayed torch.cuda.graph that holds the test's calls as one linear chain (run_both).

    kernel                         test                                    edges
    gather_rows_kernel             test_gather_rows[width]                 1 / 64 / 65 / 256 float4 per row (lane loop: one lane, full, second round by one,
                                                                           4 rounds); M = 1, 3, 4, 5, 9 (last workgroup of 4 waves partial); idx_stride 1, 2
                                                                           (the slots between hold 2^41 + 5); ld_table, ldo > width (gap keeps the sentinel);
                                                                           nrows 1, 70; indices -1, nrows, 2^40 -> a row of NaN
    gather_rows_masked_kernel      test_gather_rows_masked                 L = 9, lens (36, 21, 0, 7) >> 2 and (9, 5, 0) >> 0; rows beyond = +0.0 with 2^40 / -1
                                                                           in their index slots (never read: no NaN); a bad index inside a clip = NaN
    both launchers' refusals       test_gather_rows_refusals               width, ld_table, ldo % 4; M % L; len_shr < 0; NULL lens; NULL pointers, M < 1
    pad_rows_kernel                test_pad_rows                           the four (c, lds, cpad, ldd); 1 and 257 rows (cpad = 4 crosses a block); NaN beside
                                                                           the c channels; dst columns [cpad, ldd) keep the sentinel
    pad_rows_masked_kernel         test_pad_rows                           L = 9, lens (9, 5, 0, 12): full, part, none, lens > L; NaN rows beyond a clip -> +0.0
    mask_codes_kernel              test_mask_rows[B-H]                     B H = 1, 27, 515; H_b = lens >> 2 in {0, 1, H - 1, H, H + 3} with lens % 4 != 0
    mask_logprob_kernel            test_mask_rows[B-H]                     the same tables; either block alone
    iota_i64_kernel                test_small_kernels                      n = 1, 256, 257; first = 0, 2^33
    i64_to_i32_kernel              test_small_kernels                      n = 1, 257; -1, 2047, the int32 extremes
    set_words3_kernel              test_small_kernels                      three launches back to back, no synchronisation; 2^63 + 1, 2^64 - 1
    row_sqnorm_kernel              test_row_sqnorm                         (1, 4), (257, 64), (70, 32): exact on multiples of 1/64, dim 2^-24 sum on normals
    stream_stage_mfcc_kernel       test_stream_stage_mfcc                  window in the tail / in the chunk / across the seam; empty window; empty next; both
                                                                           empty (no launch); rows >= n_next of next keep the sentinel; second grid-stride round
                                   test_stream_stage_mfcc_refusals         every clause of the launcher's check, tail == next and four misaligned pointers included
    stream_emit_kernel             test_stream_emit                        wrap inside the append; ring exactly full; v0 == A; n == 0; Hw == 0; row A - 1 from the
                                                                           ring beside row A from codes; untouched slots unchanged; second grid-stride round
                                   test_stream_emit_refusals               every clause of the launcher's check
    stream_keep_rows_kernel<float4> test_stream_keep_rows                  W = 256, 4 aligned; r0 = 0, r0 > 0, n = 0; second grid-stride round
    stream_keep_rows_kernel<float> test_stream_keep_rows                   W = 129; W = 256 with dst (and with src) 4 bytes off 16-byte alignment: the same bits;
                                                                           second grid-stride round
                                   test_stream_keep_rows_refusals          every clause of the launcher's check

Grid-stride: a staging launch has at most 2048 workgroups of 256 threads = 524 288 threads, so a launch of more elements sends some thread
round its loop again.  stage: (8 x 4090 + 8 x 10) frames x 16 float4 = 524 800.  emit: 64 x 8192 + 64 x 16 = 525 312.  keep_rows, words:
2 x 2050 x 129 = 528 900.  keep_rows, float4: 4 x 2050 x 256 / 4 = 524 800.  (tests/test_glue_host.py asserts the same arithmetic.)

row_sqnorm bound: the kernel adds dim non-negative products one after the other in fp32, so |got - sum| <= dim 2^-24 sum to first order
(one rounding of a product and at most dim - 1 of partial sums, each relative 2^-24, all terms of one sign); measured far below, see the
[measured] lines."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from test_glue_host import (EMIT_BIG, EMIT_CASES, EMIT_RC, F32, F64, GATHER_BAD, GATHER_MASKED, GATHER_MS, GATHER_NROWS, GATHER_STRIDES,
                            GATHER_WIDTHS, I32, I32_NS, I64, IOTA_CASES, KEEP_BIG_SCALAR, KEEP_BIG_VEC, KEEP_CASES, MASK_SHAPES, PAD_MASKED,
                            PAD_ROWS, PAD_SHAPES, SENTINEL, SQNORM_SHAPES, STAGE_BIG, STAGE_CAP, STAGE_CASES, U32, emit_data, gather_data,
                            iota_ref, keep_data, mask_lens_tables, mask_ref, pad_data, payload, sentinel, sqnorm_ref, stage_data)

pytestmark = pytest.mark.gpu

RZ = 1024                                   # words per red zone: 4 KiB


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load(), _lib.context(0)


class Zoned:
    """A host array on the device between two sentinel zones; off: that many sentinel words more ahead of the body (a body 4 off bytes past
    16-byte alignment)."""

    def __init__(self, a, off=0):
        self.dtype, self.shape, self.off = a.dtype, a.shape, off
        words = np.ascontiguousarray(a).reshape(-1).view(U32)
        self.n = words.size
        img = np.full(2 * RZ + off + self.n, SENTINEL, U32)
        img[RZ + off:RZ + off + self.n] = words
        self.t = torch.from_numpy(img.view(I32)).cuda()

    def ptr(self):
        return self.t.data_ptr() + 4 * (RZ + self.off)

    def read(self, name):
        """zones intact -> the body as a host array"""
        img = self.t.cpu().numpy().view(U32)
        lo = RZ + self.off
        assert np.all(img[:lo] == SENTINEL) and np.all(img[lo + self.n:] == SENTINEL), f"{name}: a red zone was written"
        return img[lo:lo + self.n].copy().view(self.dtype).reshape(self.shape)


def same(name, got, want, nan=None):
    """got == want bit for bit; where `nan` is set, any NaN but the sentinel will do (the element was written, with a NaN)"""
    g, w = got.reshape(-1), want.reshape(-1)
    if nan is not None and nan.any():
        m = nan.reshape(-1)
        assert np.all(np.isnan(g[m].view(F32))) and not np.any(g[m] == SENTINEL), f"{name}: a row of a bad index is not a row of NaN"
        g, w = g[~m], w[~m]
    ne = np.flatnonzero(g != w)
    assert ne.size == 0, f"{name}: {ne.size} of {g.size} elements differ, the first at {int(ne[0])}: got {g[ne[0]]!r}, want {w[ne[0]]!r}"


class Case:
    """data: dict(ins, before, want[, nan]) of tests/test_glue_host.py; call(lib, p, stream) -> rc with p name -> device address;
    offs: name -> words off alignment; check(name, got) replaces the bit comparison of the outputs."""

    def __init__(self, name, data, call, offs=None, check=None):
        self.name, self.d, self.call, self.offs, self.check = name, data, call, offs or {}, check

    def alloc(self):
        self.z = {k: Zoned(a, self.offs.get(k, 0)) for k, a in {**self.d["ins"], **self.d["before"]}.items()}

    def launch(self, hip):
        _lib, lib, _ = hip
        rc = self.call(lib, {k: z.ptr() for k, z in self.z.items()}, _lib.stream_ptr())
        assert rc == 0, f"{self.name}: refused: {lib.ts_last_error().decode()}"

    def verify(self, how):
        for k, a in self.d["ins"].items():
            same(f"{self.name} ({how}): input {k}", self.z[k].read(f"{self.name} ({how}): input {k}"), a)
        got = {k: self.z[k].read(f"{self.name} ({how}): {k}") for k in self.d["before"]}
        if self.check:
            return self.check(f"{self.name} ({how})", got)
        for k, w in self.d["want"].items():
            same(f"{self.name} ({how}): {k}", got[k], w, self.d.get("nan", {}).get(k))


def run_both(hip, cases):
    """every case eagerly, then every case again on fresh buffers from ONE replayed graph: the calls captured one after the other on the
    capture stream, a linear chain"""
    for how in ("eager", "graph"):
        for c in cases:
            c.alloc()
        torch.cuda.synchronize()
        if how == "eager":
            for c in cases:
                c.launch(hip)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for c in cases:
                    c.launch(hip)
            g.replay()
        torch.cuda.synchronize()
        for c in cases:
            c.verify(how)


def refused(hip, name, data, call):
    """call(lib, p, stream) must return nonzero with a message and leave every buffer as it was"""
    _lib, lib, _ = hip
    z = {k: Zoned(a) for k, a in {**data["ins"], **data["before"]}.items()}
    rc = call(lib, {k: b.ptr() for k, b in z.items()}, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and lib.ts_last_error(), f"{name}: accepted"
    for k, a in {**data["ins"], **data["before"]}.items():
        same(f"{name}: {k} after a refused call", z[k].read(f"{name}: {k}"), a)


# ----------------------------------------------------------------------------------------------- gather_rows, plain and masked
def gather_call(a, **over):
    a = dict(a, **over)

    def call(lib, p, s):
        p = dict(p, **{k[2:]: v for k, v in over.items() if k.startswith("p_")})
        return lib.ts_debug_gather_rows(p["table"], a["ld_table"], a["nrows"], p["idx"], a["idx_stride"], a["M"], a["width"], p["out"], a["ldo"],
                                        a["L"], p.get("lens"), a["len_shr"], s)
    return call


def bad_value(i, nrows):
    v = GATHER_BAD[i % 3]
    return nrows if v is None else v


@pytest.mark.parametrize("width", GATHER_WIDTHS)
def test_gather_rows(hip, width):
    rng = np.random.default_rng(width)
    cases, k = [], 0
    for M in GATHER_MS:
        for stride in GATHER_STRIDES:
            for nrows in GATHER_NROWS:
                for roomy in (False, True):
                    bad = {}
                    for m in range(min(3, M // 2)):          # the first rows; the rest hold good indices
                        bad[m], k = bad_value(k, nrows), k + 1
                    d = gather_data(rng, width, M, stride, nrows, roomy, bad)
                    cases.append(Case(f"gather w={width} M={M} stride={stride} nrows={nrows} roomy={roomy}", d, gather_call(d["args"])))
    for i in range(3):                                       # one row, a bad index: the whole output is one row of NaN
        d = gather_data(rng, width, 1, 1, 70, True, {0: bad_value(i, 70)})
        cases.append(Case(f"gather w={width} M=1 bad={bad_value(i, 70)}", d, gather_call(d["args"])))
    assert any(c.d["nan"]["out"].any() for c in cases) and any(not c.d["nan"]["out"].any() for c in cases)
    run_both(hip, cases)


def test_gather_rows_masked(hip):
    rng = np.random.default_rng(11)
    cases = []
    for L, lens, shr in GATHER_MASKED:
        M = L * len(lens)
        inside = next(m for m in range(M) if m % L < (lens[m // L] >> shr)) + 1          # the second own row of the first clip
        for width in GATHER_WIDTHS:
            for stride in GATHER_STRIDES:
                for roomy in (False, True):
                    d = gather_data(rng, width, M, stride, 70, roomy, {inside: 70}, (L, lens, shr))
                    out, nan = d["want"]["out"], d["nan"]["out"]
                    assert nan[inside, :width].all() and nan.sum() == width                  # the one NaN row is the bad index inside a clip
                    assert (out[:, :width] == 0).all(axis=1).sum() == sum(L - min(L, n >> shr) for n in lens)
                    cases.append(Case(f"gather masked lens={lens} w={width} stride={stride} roomy={roomy}", d, gather_call(d["args"])))
    run_both(hip, cases)


def test_gather_rows_refusals(hip):
    rng = np.random.default_rng(12)
    plain = gather_data(rng, 8, 4, 1, 70, True)
    masked = gather_data(rng, 8, 18, 1, 70, True, masked=(9, (9, 5), 0))
    run_both(hip, [Case("gather base", plain, gather_call(plain["args"])), Case("gather masked base", masked, gather_call(masked["args"]))])
    for d, over in ((plain, dict(width=6)), (plain, dict(ld_table=14)), (plain, dict(ldo=10)), (masked, dict(width=6)), (masked, dict(ld_table=14)),
                    (masked, dict(ldo=10)), (masked, dict(M=17)), (masked, dict(len_shr=-1)), (masked, dict(p_lens=None)), (masked, dict(L=0)),
                    (plain, dict(p_table=None)), (plain, dict(p_idx=None)), (plain, dict(p_out=None)), (plain, dict(M=0)), (masked, dict(M=0))):
        refused(hip, f"gather {over}", d, gather_call(d["args"], **over))


# ----------------------------------------------------------------------------------------------- pad_rows, plain and masked
def pad_call(a, **over):
    a = dict(a, **over)

    def call(lib, p, s):
        p = dict(p, **{k[2:]: v for k, v in over.items() if k.startswith("p_")})
        return lib.ts_debug_pad_rows(p["src"], a["lds"], a["c"], p["dst"], a["ldd"], a["cpad"], a["B"], a["L"], p.get("lens"), s)
    return call


def test_pad_rows(hip):
    rng = np.random.default_rng(13)
    cases = []
    L, lens = PAD_MASKED
    for c, lds, cpad, ldd in PAD_SHAPES:
        for rows in PAD_ROWS:
            d = pad_data(rng, c, lds, cpad, ldd, 1, rows)
            cases.append(Case(f"pad {(c, lds, cpad, ldd)} rows={rows}", d, pad_call(d["args"])))
        d = pad_data(rng, c, lds, cpad, ldd, len(lens), L, lens)
        assert (d["want"]["dst"][:, :cpad] == 0).all(axis=1).sum() >= sum(L - min(L, n) for n in lens)
        cases.append(Case(f"pad masked {(c, lds, cpad, ldd)}", d, pad_call(d["args"])))
    d = pad_data(rng, 4, 4, 4, 8, 257, 1)                    # the same 257 rows as 257 clips of one row
    cases.append(Case("pad B=257 L=1", d, pad_call(d["args"])))
    run_both(hip, cases)
    d = pad_data(rng, 3, 5, 4, 8, 2, 3, (3, 1))
    for over in (dict(p_src=None), dict(p_dst=None), dict(B=0), dict(L=0), dict(cpad=0)):
        refused(hip, f"pad {over}", d, pad_call(d["args"], **over))


# ----------------------------------------------------------------------------------------------- mask_codes / mask_logprob
@pytest.mark.parametrize("B,H", MASK_SHAPES)
def test_mask_rows(hip, B, H):
    rng = np.random.default_rng(100 * B + H)
    cases = []
    for j, lens in enumerate(mask_lens_tables(B, H)):
        for which in (("codes", "logprob"), ("codes",), ("logprob",)) if j == 0 else (("codes", "logprob"),):
            codes = rng.integers(0, 2048, (B, H, 2)).astype(I64)
            codes.reshape(-1)[0] = 2 ** 63 - 1
            lp = payload(rng, (B, H, 2))
            want = dict(codes=mask_ref(codes, lens, -1) if "codes" in which else codes, logprob=mask_ref(lp, lens, 0) if "logprob" in which else lp)
            d = dict(ins=dict(lens=lens), before=dict(codes=codes, logprob=lp), want=want)
            cases.append(Case(f"mask {which} B={B} H={H} lens={lens.tolist()}", d,
                              lambda lib, p, s, which=which: lib.ts_debug_mask_rows(p["codes"] if "codes" in which else None,
                                                                                    p["logprob"] if "logprob" in which else None, B, H, p["lens"], s)))
    run_both(hip, cases)
    if B == 1:
        d = cases[0].d
        for name, call in (("no block", lambda lib, p, s: lib.ts_debug_mask_rows(None, None, B, H, p["lens"], s)),
                           ("no lens", lambda lib, p, s: lib.ts_debug_mask_rows(p["codes"], p["logprob"], B, H, None, s)),
                           ("B = 0", lambda lib, p, s: lib.ts_debug_mask_rows(p["codes"], p["logprob"], 0, H, p["lens"], s)),
                           ("H = 0", lambda lib, p, s: lib.ts_debug_mask_rows(p["codes"], p["logprob"], B, 0, p["lens"], s))):
            refused(hip, f"mask {name}", d, call)


# ----------------------------------------------------------------------------------------------- iota, i64 -> i32, set_words3, row_sqnorm
def test_small_kernels(hip):
    rng = np.random.default_rng(14)
    cases = []
    for n, first in IOTA_CASES:
        d = dict(ins={}, before=dict(dst=sentinel((n,), I64)), want=dict(dst=iota_ref(n, first)))
        cases.append(Case(f"iota n={n} first={first}", d, lambda lib, p, s, n=n, first=first: lib.ts_debug_iota_i64(p["dst"], n, first, s)))
    for n in I32_NS:
        src = rng.integers(0, 2048, n).astype(I64)
        src[:min(n, 4)] = (-1, 2047, 2 ** 31 - 1, -2 ** 31)[:min(n, 4)]
        d = dict(ins=dict(src=src), before=dict(dst=sentinel((n,), I32)), want=dict(dst=src.astype(I32)))
        cases.append(Case(f"i64_to_i32 n={n}", d, lambda lib, p, s, n=n: lib.ts_debug_i64_to_i32(p["src"], p["dst"], n, s)))
    words = {"d0": (1, 2, 3), "d1": (2 ** 63 + 1, 0, 2 ** 64 - 1), "d2": (0x0123456789ABCDEF, 2 ** 63 + 1, 7)}
    d = dict(ins={}, before={k: sentinel((3,), np.uint64) for k in words}, want={k: np.array(v, np.uint64) for k, v in words.items()})

    def three(lib, p, s):                                    # three launches queued back to back: each carries its words in its own arguments
        return max(lib.ts_debug_set_words3(p[k], *words[k], s) for k in ("d0", "d1", "d2"))
    cases.append(Case("set_words3 x 3", d, three))
    run_both(hip, cases)
    _lib, lib, _ = hip
    z = Zoned(sentinel((4,), I64))
    for rc in (lib.ts_debug_iota_i64(None, 4, 0, None), lib.ts_debug_iota_i64(z.ptr(), 0, 0, None), lib.ts_debug_i64_to_i32(None, z.ptr(), 4, None),
               lib.ts_debug_i64_to_i32(z.ptr(), None, 4, None), lib.ts_debug_i64_to_i32(z.ptr(), z.ptr(), 0, None),
               lib.ts_debug_set_words3(None, 1, 2, 3, None), lib.ts_debug_row_sqnorm(None, 1, 4, z.ptr(), None),
               lib.ts_debug_row_sqnorm(z.ptr(), 1, 4, None, None), lib.ts_debug_row_sqnorm(z.ptr(), 0, 4, z.ptr(), None)):
        assert rc != 0
    torch.cuda.synchronize()
    assert np.all(z.read("refused small calls").view(U32) == SENTINEL)


@pytest.mark.parametrize("n,dim", SQNORM_SHAPES)
def test_row_sqnorm(hip, n, dim):
    rng = np.random.default_rng(n + dim)
    exact = (rng.integers(-256, 257, (n, dim)) / 64.0).astype(F32)          # squares are multiples of 2^-12 <= 16, sums < 2^24 of them: exact in fp32
    exact[0, :2] = (4.0, -4.0)
    normal = rng.standard_normal((n, dim)).astype(F32)
    ref_e, ref_n = sqnorm_ref(exact), sqnorm_ref(normal)
    assert np.array_equal(ref_e.astype(F32).astype(F64), ref_e)
    scale = dim * 2.0 ** -24 * ref_n

    def check_exact(name, got):
        same(name, got["out"].view(U32), ref_e.astype(F32).view(U32))

    def check_bound(name, got):
        assert not np.any(got["out"].view(U32) == SENTINEL), f"{name}: rows not written"
        assert_close_measured(f"{name} n={n} dim={dim}: |err| / (dim 2^-24 sum)", got["out"].astype(F64) / scale, ref_n / scale, 1.0)

    def call(lib, p, s):
        return lib.ts_debug_row_sqnorm(p["e"], n, dim, p["out"], s)
    run_both(hip, [Case("row_sqnorm exact", dict(ins=dict(e=exact), before=dict(out=sentinel((n,), F32))), call, check=check_exact),
                   Case("row_sqnorm normal", dict(ins=dict(e=normal), before=dict(out=sentinel((n,), F32))), call, check=check_bound)])


# ----------------------------------------------------------------------------------------------- stream_stage_mfcc
def stage_call(a, **over):
    a = dict(a, **over)

    def call(lib, p, s):
        p = dict(p)
        for k, v in over.items():
            if k.startswith("p_"):
                p[k[2:]] = v(p) if callable(v) else v
        return lib.ts_debug_stream_stage_mfcc(p["tail"], p["chunk"], p["win"], p["next"], a["B"], a["n_tail"], a["t"], a["cap"], a["Tw"], a["next0"],
                                              a["n_next"], s)
    return call


def test_stream_stage_mfcc(hip):
    rng = np.random.default_rng(15)
    cases = []
    for B in (1, 3):
        for n_tail, t, Tw, next0, n_next in STAGE_CASES:
            d = stage_data(rng, B, STAGE_CAP, n_tail, t, Tw, next0, n_next)
            assert np.all(d["want"]["next"][:, n_next:] == SENTINEL)
            cases.append(Case(f"stage B={B} {(n_tail, t, Tw, next0, n_next)}", d, stage_call(d["args"])))
    d = stage_data(rng, **STAGE_BIG)
    cases.append(Case("stage grid-stride", d, stage_call(d["args"])))
    run_both(hip, cases)


def test_stream_stage_mfcc_refusals(hip):
    d = stage_data(np.random.default_rng(16), 2, STAGE_CAP, 5, 7, 12, 3, 9)
    run_both(hip, [Case("stage base", d, stage_call(d["args"]))])
    overs = [dict(B=0), dict(n_tail=-1), dict(t=-1), dict(Tw=-1), dict(n_next=-1), dict(next0=-1), dict(n_tail=13), dict(n_next=13, next0=0), dict(Tw=13),
             dict(next0=4), dict(p_chunk=None), dict(p_next=lambda p: p["tail"]), dict(p_tail=None), dict(p_win=None), dict(p_next=None)]
    overs += [{"p_" + k: (lambda p, k=k: p[k] + 4)} for k in ("tail", "chunk", "win", "next")]
    for over in overs:
        refused(hip, f"stage {sorted(over)} {[v for v in over.values() if not callable(v)]}", d, stage_call(d["args"], **over))


# ----------------------------------------------------------------------------------------------- stream_emit
def emit_call(a, **over):
    a = dict(a, **over)

    def call(lib, p, s):
        p = dict(p)
        for k, v in over.items():
            if k.startswith("p_"):
                p[k[2:]] = v(p) if callable(v) else v
        return lib.ts_debug_stream_emit(p["codes"], p["ring"], p["lat_body"], p["lat_hand"], a["B"], a["n"], a["A"], a["RC"], a["v0"], a["Hw"], s)
    return call


def test_stream_emit(hip):
    rng = np.random.default_rng(17)
    cases = []
    for B in (1, 3):
        for n, A, v0, Hw in EMIT_CASES:
            d = emit_data(rng, B, EMIT_RC, n, A, v0, Hw)
            cases.append(Case(f"emit B={B} {(n, A, v0, Hw)}", d, emit_call(d["args"])))
    d = emit_data(rng, **EMIT_BIG)
    cases.append(Case("emit grid-stride", d, emit_call(d["args"])))
    run_both(hip, cases)


def test_stream_emit_refusals(hip):
    d = emit_data(np.random.default_rng(18), 2, EMIT_RC, 4, 6, 4, 6)
    run_both(hip, [Case("emit base", d, emit_call(d["args"]))])
    overs = [dict(B=0), dict(n=-1), dict(Hw=-1), dict(A=-1, v0=-1), dict(v0=-1), dict(RC=0), dict(v0=7), dict(RC=5), dict(Hw=7), dict(p_codes=None),
             dict(p_lat_body=None), dict(p_lat_hand=None), dict(p_ring=None), dict(p_codes=lambda p: p["codes"] + 8), dict(p_ring=lambda p: p["ring"] + 8)]
    for over in overs:
        refused(hip, f"emit {sorted(over)} {[v for v in over.values() if not callable(v)]}", d, emit_call(d["args"], **over))


# ----------------------------------------------------------------------------------------------- stream_keep_rows
def keep_call(a, **over):
    a = dict(a, **over)

    def call(lib, p, s):
        p = dict(p, **{k[2:]: v for k, v in over.items() if k.startswith("p_")})
        return lib.ts_debug_stream_keep_rows(p["src"], p["dst"], a["B"], a["R"], a["r0"], a["n"], a["W"], s)
    return call


def test_stream_keep_rows(hip):
    rng = np.random.default_rng(19)
    cases = []
    for B in (1, 3):
        for R, r0, n, W in KEEP_CASES:
            d = keep_data(rng, B, R, r0, n, W)
            cases.append(Case(f"keep B={B} {(R, r0, n, W)}", d, keep_call(d["args"])))
        d = keep_data(rng, B, 5, 1, 3, 256)
        cases.append(Case(f"keep B={B} W=256, dst 4 bytes off", d, keep_call(d["args"]), offs=dict(dst=1)))
        d = keep_data(rng, B, 5, 1, 3, 256)
        cases.append(Case(f"keep B={B} W=256, src 4 bytes off", d, keep_call(d["args"]), offs=dict(src=1)))
    for big in (KEEP_BIG_SCALAR, KEEP_BIG_VEC):
        d = keep_data(rng, **big)
        cases.append(Case(f"keep grid-stride {big}", d, keep_call(d["args"])))
    run_both(hip, cases)


def test_stream_keep_rows_refusals(hip):
    d = keep_data(np.random.default_rng(20), 2, 5, 1, 3, 4)
    run_both(hip, [Case("keep base", d, keep_call(d["args"]))])
    for over in (dict(B=0), dict(R=0), dict(W=0), dict(r0=-1), dict(n=-1), dict(r0=3), dict(p_src=None), dict(p_dst=None)):
        refused(hip, f"keep {over}", d, keep_call(d["args"], **over))
