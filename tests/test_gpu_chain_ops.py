"""Op-level tests of the PixelCNN chain GEMM kernels, one by one, against a float64 restatement of one chain problem: the wide kernel
(`csrc/skinny_wide.hip::skinny16_wide_kernel`), the descriptor kernel at every tile shape (`skinny16_fast_kernel<W, RB, CB>`) and the two
generic kernels (`skinny16_kernel<W>`, `skinny_gemm_kernel<W>`), each forced through `ts_debug_skinny_run` with a knob list: the
production plan, descriptor packing and launch code, one process, the kernel that ran reported back (`out5`).

The reference restates the documented semantics of `csrc/kernels.h` (SkinnySeg / SkinnyParams, the tiled index formula, the weight tile
order), not any kernel's code.  Every operand sits in its own NaN-filled allocation with NaN red zones; rows past M of an input (up to
its 16-row padding), columns past a segment inside its row stride and every output element a problem must not write are NaN too.  A read
past the documented extent then shows as a non-finite output, a stray store as a changed NaN pattern.

Bounds.  The error of an output is measured in units of its own scale: S = sum_k |a_mk w_nk| + sum |epilogue terms| for the linear form
and `pre`; for the gate, (S_v + S_p / 4) after gate_act's own absolute error GATE_ABS = 3e-7 (test_gate_activation_accuracy) is taken off
(d tanh(v) sigmoid(p) / dv <= 1, d / dp <= 1 / 4).  CEILING from fp32 error analysis: a wave's share is a chain of K / W fused
multiply-adds, W partial sums meet in a fixed order, then up to 5 epilogue additions: (K / W + W + 6) 2^-24 in those units.  The
asserted BOUND (LIN_BOUND, GATE_BOUND) is 2x the largest error measured on the MI355X (TS_MEASURED_LOG: the first MI355X run of this
file measured them, nobody had before) and sits under every case's ceiling.  Each bound misses each defect of DEFECTS, applied to the float64 reference on the
CPU, by at least 10x (`test_bounds_catch_defects`).

Bit-identity (the contract at `skinny_gemm.hip:13`), pinned by test_kernels_bit_identical: for a problem at a given W (plan_skinny takes
W = 8 from K >= 256, else 4), the wide kernel, the fast kernel at every tile shape (11 / 21 / 22 / 42) and skinny16_kernel<W> give the
same bits, row-major or tiled operands alike.  skinny_gemm_kernel (32 columns, 8-k steps on the 32 x 32 x 2 MFMA) is NOT in that set at
any W: measured at W = 4 (K = 128), 8 (K = 256, 384: the 16-column kernels' W too) and 16 (K = 512, 1024), its results differ in the last
bits every time.  It is pinned against the reference only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_close_measured

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GATE_ABS = 3e-7                     # |gate_act - tanh * sigmoid|, tests/test_gpu_parity.py::test_gate_activation_accuracy
# 2x the largest error measured on the MI355X over every case of this file (in the units above): linear / pre 1.12e-7 (1.9 x 2^-24, the
# epilogue-only problem of multi6: three additions), gate 3.1e-8 beyond GATE_ABS (wide, a 256-clip vertical gate)
LIN_BOUND = 2.2e-7
GATE_BOUND = 6.2e-8
KERNELS = ("wide", "fast", "generic16", "generic32")
RZ = 64                             # red zone (floats) on each side of every allocation: 256 B keeps 16-byte alignment
NANBITS = 0x7FE5A5A5                # the fill: a quiet NaN with a payload no arithmetic produces
FORCE = {"generic16": "TS_SKINNY_V=0", "generic32": "TS_SKINNY_NT=32", "fast": "TS_SKINNY_WIDE_MIN=0",
         "wide": "TS_SKINNY_WIDE_MIN=1"}


# ----------------------------------------------------------------------------------------------- layouts (numpy, from kernels.h)
def tiled_index(m, k, W):
    """kernels.h, SkinnyParams: float index of element (m, k) of a [rows][W] array stored as 16 x 16 fragments in lane order."""
    m, k = np.asarray(m, np.int64), np.asarray(k, np.int64)
    return (((m >> 4) * (W >> 4) + (k >> 4)) << 8) + (((m & 15) + 16 * ((k & 15) >> 2)) << 2) + (k & 3)


def tiled_decode(i, W):
    """The inverse of tiled_index: (m, k) of float index i."""
    i = np.asarray(i, np.int64)
    frag, r = i >> 8, i & 255
    lane, e = r >> 2, r & 3
    m = (frag // (W >> 4)) * 16 + (lane & 15)
    k = (frag % (W >> 4)) * 16 + 4 * (lane >> 4) + e
    return m, k


def tiled_lin(lin, tw):
    """Float index of element `lin` = row * stride + col of a buffer written in the tiled view of width tw (out_tiled_w and kin)."""
    lin = np.asarray(lin, np.int64)
    return tiled_index(lin // tw, lin % tw, tw)


def weight_column(t, li, N, epi, gateD):
    """Weight row (output column n) at position li of 16-column weight tile t: linear t * 16 + li; gate tiles are 8 'tanh' channels
    followed by their 8 'sigmoid' partners (columns c and c + gateD of a 2 gateD group)."""
    if epi == 0:
        return t * 16 + li
    tpg = gateD // 8
    group, ch0 = t // tpg, (t % tpg) * 8
    return group * 2 * gateD + (li >> 3) * gateD + ch0 + (li & 7)


def tile_weights(W, epi, gateD=0):
    """The tiled weight copy: tile t, q-step q at (t * K / 16 + q) * 256 in lane order = the tiled view of the [16 ceil(N / 16)][K] matrix
    whose row 16 t + li is weight row weight_column(t, li); rows past N are zeros."""
    N, K = W.shape
    nt = (N + 15) // 16
    rows = np.zeros((nt * 16, K), F32)
    for t in range(nt):
        for li in range(16):
            n = weight_column(t, li, N, epi, gateD)
            if n < N:
                rows[t * 16 + li] = W[n]
    out = np.empty(nt * 16 * K, F32)
    m, k = np.meshgrid(np.arange(nt * 16), np.arange(K), indexing="ij")
    out[tiled_index(m, k, K)] = rows
    return out


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def gate64(v, gateD, partner_shift=0):
    """Output channel g * gateD + c = tanh(v[g * 2 gateD + c]) * sigmoid(v[g * 2 gateD + gateD + c]); -> (out, tanh cols, sigmoid cols)."""
    G = v.shape[1] // (2 * gateD)
    c = np.arange(gateD)
    t = np.concatenate([g * 2 * gateD + c for g in range(G)])
    s = np.concatenate([g * 2 * gateD + gateD + (c + partner_shift) % gateD for g in range(G)])
    return np.tanh(v[:, t]) * sigmoid64(v[:, s]), t, s


# ----------------------------------------------------------------------------------------------- problems
class Buf:
    """One allocation: n floats at offset RZ + off of a NaN-filled host image (red zones both sides), uploaded as is."""

    def __init__(self, n, off=0, out=False):
        self.n, self.off, self.out = n, off, out
        self.h = np.full(RZ + off + n + RZ, NANBITS, np.uint32).view(F32)
        self.d = None

    def body(self):
        return self.h[RZ + self.off:RZ + self.off + self.n]

    def ptr(self):
        return self.d.data_ptr() + 4 * (RZ + self.off)

    def upload(self):
        if self.d is None:
            self.d = torch.from_numpy(self.h.copy()).cuda()
        else:
            self.d.copy_(torch.from_numpy(self.h))


def seg(kind, n, **kw):
    """A segment of A: 'dense' (shift, extra stride columns, tiled), 'gather' (gstride, neg: some ids -1) or 'null' (zero rows)."""
    return dict(kind=kind, len=n, **kw)


def prob(M, N, segs, epi=0, **kw):
    """One chain problem: segs of A; epi 0 linear (relu) / 1 gate (gateD, cls = cls_ld, pre = dict(extra, tw)); bias; add1 / add2 =
    dict(shift, extra, tiled, off); add3 = dict(extra); out = dict(extra, tw); w_tiled; ldw_extra."""
    if isinstance(segs, int):
        segs = [seg("dense", segs)]
    return dict(M=M, N=N, segs=segs, epi=epi, **kw)


def round16(x):
    return (x + 15) // 16 * 16


def build(spec, rng):
    """Host images of every operand of `spec` and the float64 pieces the reference needs.  Nothing touches the GPU."""
    M, N, epi = spec["M"], spec["N"], spec["epi"]
    K = sum(s["len"] for s in spec["segs"])
    gateD = spec.get("gateD", N // 2) if epi == 1 else 0
    b = dict(spec=spec, M=M, N=N, K=K, epi=epi, gateD=gateD, bufs=[], ints=[])
    pr = _lib().SkinnyProblem()
    pr.M, pr.N, pr.nseg, pr.epi, pr.relu, pr.gateD = M, N, len(spec["segs"]), epi, spec.get("relu", 0), gateD
    fill = []            # (Buf, struct setter) resolved at upload time
    A = []
    for i, s in enumerate(spec["segs"]):
        L = s["len"]
        sg = pr.seg[i]
        sg.len = L
        if s["kind"] == "null":
            A.append(np.zeros((M, L)))
            continue
        if s["kind"] == "gather":
            rows = 37
            stride = L + s.get("extra", 4)
            tab = Buf(rows * stride)
            t = rng.standard_normal((rows, L)).astype(F32)
            tab.body().reshape(rows, stride)[:, :L] = t
            gs = s.get("gstride", 1)
            ids = rng.integers(0, rows, M).astype(np.int32)
            if s.get("neg"):
                ids[::5] = -1
                ids[M - 1] = -3
            gi = np.full(M * gs + 3, -1, np.int32)
            gi[np.arange(M) * gs] = ids
            b["ints"].append(gi)
            A.append(np.where(ids[:, None] >= 0, t[np.maximum(ids, 0)].astype(F64), 0.0))
            sg.row_stride, sg.gidx_stride = stride, gs
            fill.append((tab, lambda p, sg=sg: setattr(sg, "base", p)))
            b.setdefault("gidx", []).append((sg, len(b["ints"]) - 1))
            b["bufs"].append(tab)
            continue
        shift = s.get("shift", 0)
        rows = ((M - 1) >> shift) + 1
        x = rng.standard_normal((rows, L)).astype(F32)
        if s.get("tiled"):
            buf = Buf(round16(rows) * L)
            m, k = np.meshgrid(np.arange(rows), np.arange(L), indexing="ij")
            buf.body()[tiled_index(m, k, L)] = x
            sg.tiled_w, sg.row_stride = L, L
        else:
            stride = L + s.get("extra", 4)
            buf = Buf(round16(rows) * stride)
            buf.body().reshape(-1, stride)[:rows, :L] = x
            sg.row_stride = stride
        sg.row_shift = shift
        A.append(x.astype(F64)[np.arange(M) >> shift])
        fill.append((buf, lambda p, sg=sg: setattr(sg, "base", p)))
        b["bufs"].append(buf)
    b["A"] = np.concatenate(A, 1)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
    b["W"] = W.astype(F64)
    if spec.get("w_tiled"):
        wb = Buf((N + 15) // 16 * 16 * K)
        wb.body()[:] = tile_weights(W, epi, gateD)
        pr.w_tiled, pr.ldw = K // 16, K
    else:
        ldw = K + spec.get("ldw_extra", 4)
        wb = Buf(N * ldw)
        wb.body().reshape(N, ldw)[:, :K] = W
        pr.ldw = ldw
    fill.append((wb, lambda p: setattr(pr, "W", p)))
    b["bufs"].append(wb)
    terms = {}
    if spec.get("bias", True):
        v = rng.standard_normal(N).astype(F32)
        bb = Buf(N)
        bb.body()[:] = v
        terms["bias"] = v.astype(F64)
        fill.append((bb, lambda p: setattr(pr, "bias", p)))
        b["bufs"].append(bb)
    for name in ("add1", "add2", "add3"):
        o = spec.get(name)
        if o is None:
            continue
        o = dict(o)
        shift = o.get("shift", 0) if name != "add3" else 0
        rows = ((M - 1) >> shift) + 1
        v = rng.standard_normal((rows, N)).astype(F32)
        if o.get("tiled"):
            stride = o["tiled"]["stride"]
            tw = o["tiled"]["tw"]
            ab = Buf(round16((rows * stride + tw - 1) // tw) * tw)
            lin = np.arange(rows)[:, None] * stride + np.arange(N)[None, :]
            ab.body()[tiled_lin(lin, tw)] = v
            pr.add1_tiled_w = tw
        else:
            stride = N + o.get("extra", 4)
            ab = Buf(rows * stride, off=o.get("off", 0))
            ab.body().reshape(rows, stride)[:, :N] = v
        setattr(pr, name + "_stride", stride)
        if name != "add3":
            setattr(pr, name + "_shift", shift)
        terms[name] = (v.astype(F64), shift)
        fill.append((ab, lambda p, name=name: setattr(pr, name, p)))
        b["bufs"].append(ab)
    if epi == 1 and spec.get("cls"):
        ld = spec["cls"]
        v = rng.standard_normal((M, ld)).astype(F32)
        cb = Buf(M * ld)
        cb.body()[:] = v.reshape(-1)
        pr.cls_ld = ld
        b["cls"] = v.astype(F64)
        fill.append((cb, lambda p: setattr(pr, "clsrow", p)))
        b["bufs"].append(cb)
    b["terms"] = terms
    # outputs: NaN everywhere; out has Nout written columns of its row stride, `pre` N
    Nout = N // 2 if epi == 1 else N
    b["outs"] = {}
    for name, cols, o in (("out", Nout, spec.get("out", {})), ("pre", N, spec.get("pre"))):
        if o is None:
            continue
        tw = o.get("tw", 0)
        stride = o.get("stride", cols + o.get("extra", 4))
        if tw:
            ob = Buf(round16((M * stride + tw - 1) // tw) * tw, out=True)
        else:
            ob = Buf(M * stride, off=o.get("off", 0), out=True)
        setattr(pr, name + "_stride", stride)
        if tw:
            setattr(pr, name + "_tiled_w", tw)
        lin = np.arange(M)[:, None] * stride + np.arange(cols)[None, :]
        b["outs"][name] = (ob, tiled_lin(lin, tw) if tw else lin)
        fill.append((ob, lambda p, name=name: setattr(pr, name, p)))
        b["bufs"].append(ob)
    b["pr"], b["fill"] = pr, fill
    return b


def reference(b, defect=None):
    """float64 outputs of built problem b -> {'out': (value, scale), 'pre': (value, scale)}; `defect` (DEFECTS) alters the arithmetic."""
    M, N, K = b["M"], b["N"], b["K"]
    A, W = b["A"], b["W"]
    if defect == "drop_k_step":                   # the last 16-k step of K skipped
        A = A.copy()
        A[:, K - 16:] = 0.0
    acc = A @ W.T
    scale = np.abs(A) @ np.abs(W).T
    rows = np.arange(M)
    v = acc
    for name, t in b["terms"].items():
        if name == "bias":
            term = t[(np.arange(N) + 1) % N] if defect == "bias_next_column" else t
            term = np.broadcast_to(term, (M, N))
        else:
            if name == "add2" and defect == "no_add2":
                continue
            x, shift = t
            r = rows >> shift
            if name == "add1" and defect == "add1_unshifted":
                r = np.minimum(rows, x.shape[0] - 1)
            term = x[r]
        v = v + term
        scale = scale + np.abs(term)
    if b["epi"] == 0:
        if b["spec"].get("relu"):
            v = np.maximum(v, 0.0)
        return {"out": (v, scale)}
    res = {}
    cls = b.get("cls")
    if cls is not None:
        ld = cls.shape[1]
        c = cls[:, np.arange(N) % ld]
        pre = v + c if defect == "cls_before_pre" else v
        v, vscale = v + c, scale + np.abs(c)
    else:
        pre, vscale = v, scale
    res["pre"] = (pre, scale)
    g, t, s = gate64(v, b["gateD"], 1 if defect == "partner_off_by_one" else 0)
    res["out"] = (g, vscale[:, t] + vscale[:, s] / 4)
    return res


DEFECTS = ("drop_k_step", "no_add2", "add1_unshifted", "cls_before_pre", "partner_off_by_one", "bias_next_column")


def normalized_error(name, b, got, ref):
    """max error in the units of the module docstring: |err| / S (linear, pre); (|err| - GATE_ABS)+ / (S_v + S_p / 4) (gate)."""
    val, scale = ref
    err = np.abs(np.asarray(got, F64) - val)
    if name == "out" and b["epi"] == 1:
        err = np.maximum(err - GATE_ABS, 0.0)
    return float((err / np.maximum(scale, 1e-30)).max())


def bound_of(name, b):
    return GATE_BOUND if name == "out" and b["epi"] == 1 else LIN_BOUND


# ----------------------------------------------------------------------------------------------- GPU plumbing
_LIB = []


def _lib():
    if not _LIB:
        from talkshow_amd import _lib as L
        _LIB.append(L)
    return _LIB[0]


@pytest.fixture(scope="module")
def hip():
    L = _lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return L, L.load(), L.context(0)


def upload(b):
    for buf in b["bufs"]:
        buf.upload()
    for setter in b["fill"]:
        setter[1](setter[0].ptr())
    b["int_d"] = [torch.from_numpy(gi).cuda() for gi in b["ints"]]
    for sg, j in b.get("gidx", []):
        sg.gidx = b["int_d"][j].data_ptr()


def reset_outputs(bs):
    for b in bs:
        for ob, _ in b["outs"].values():
            ob.upload()


def launch(hip, bs, knobs):
    """One ts_debug_skinny_run of problems bs -> (return code, out5, ts_last_error)."""
    L, lib, ctx = hip
    arr = (L.SkinnyProblem * len(bs))(*[b["pr"] for b in bs])
    out5 = (C.c_int * 5)()
    rc = lib.ts_debug_skinny_run(ctx, arr, len(bs), knobs.encode() if knobs else None, out5, None)
    torch.cuda.synchronize()
    return rc, tuple(out5), (lib.ts_last_error().decode() if rc < 0 else "")


def outputs(b):
    """{name: (logical [M][cols] float32 values, whole device image as uint32)} of b's outputs after a run."""
    res = {}
    for name, (ob, idx) in b["outs"].items():
        img = ob.d.cpu().numpy()
        res[name] = (img[RZ + ob.off + idx], img.view(np.uint32))
    return res


def check_untouched(tag, b, got):
    """Inputs unchanged bit for bit; every output element the problem must not write still holds the NaN fill."""
    for buf in b["bufs"]:
        img = buf.d.cpu().numpy().view(np.uint32)
        want = buf.h.view(np.uint32)
        if not buf.out:
            assert np.array_equal(img, want), f"{tag}: an input buffer changed"
    for name, (ob, idx) in b["outs"].items():
        img = got[name][1].copy()
        img[RZ + ob.off + idx.reshape(-1)] = NANBITS
        bad = np.flatnonzero(img != NANBITS)
        assert bad.size == 0, f"{tag}: {name} written outside its rows / columns at float {bad[:8] - RZ - ob.off}"


def run_case(hip, tag, bs, knobs, kernel, rb_cb=None, measured=True):
    """Launch problems bs under knobs; assert the kernel that ran, the reference bounds, the untouched NaNs, a repeat's bits.
    -> ([per problem: {name: logical output}], out5)."""
    reset_outputs(bs)
    rc, o5, err = launch(hip, bs, knobs)
    assert rc >= 0, f"{tag}: {err}"
    assert KERNELS[o5[0]] == kernel, f"{tag}: ran {KERNELS[o5[0]]} {o5}, meant {kernel}"
    if rb_cb is not None:
        assert (o5[2], o5[3]) == rb_cb, f"{tag}: tile {o5[2:4]}, meant {rb_cb}"
    print(f"\n[ran] {tag}: {KERNELS[o5[0]]} W={o5[1]} RB={o5[2]} CB={o5[3]} workgroups={o5[4]}")
    res = []
    for i, b in enumerate(bs):
        got = outputs(b)
        ref = reference(b)
        ceiling = (b["K"] / o5[1] + o5[1] + 6) * U
        for name, (val, _) in got.items():
            assert np.isfinite(val).all(), f"{tag} p{i} {name}: non-finite output (a read past an operand's extent?)"
            bound = bound_of(name, b)
            assert bound <= ceiling, f"{tag}: bound {bound:.1e} over the ceiling {ceiling:.1e}"
            e = normalized_error(name, b, val, ref[name])
            if measured:
                assert_close_measured(f"chain.{KERNELS[o5[0]]}.{'gate' if name == 'out' and b['epi'] else 'lin'}.{tag}.p{i}.{name}",
                                      np.array([e]), np.array([0.0]), bound)
            else:
                assert e <= bound, f"{tag} p{i} {name}: error {e:.3e} over the bound {bound:.1e}"
        check_untouched(f"{tag} p{i}", b, got)
        res.append({k: v[0].copy() for k, v in got.items()})
    reset_outputs(bs)
    rc2, o52, _ = launch(hip, bs, knobs)
    assert rc2 == rc and o52 == o5
    for i, b in enumerate(bs):
        again = outputs(b)
        for name in again:
            assert np.array_equal(again[name][0].view(np.uint32), res[i][name].view(np.uint32)), f"{tag} p{i} {name}: bits changed"
    return res, o5


def same_bits(x, y):
    return all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in x)


# ----------------------------------------------------------------------------------------------- production launches
def _production_specs(problems, rows2b):
    """The chain problems of one production launch kind (tests/test_host_logic.py, (M, N, K) with K < 0 = epilogue-only) with the operand
    kinds pixelcnn.cpp gives them (D = 256: vertical problems N = 4D, horizontal 2D / D, heads HID = 512 / V = 2048):
      K < 0, N = 4D: V0 at the top row — a zero-row segment, gate, class rows of 2D, `pre` [B][4D] in the tiled view of width 2D, out tiled;
      K < 0, N = 2D: hg_0 at column 0 — zero rows, gate, add1 = v2h (stride 4D), class rows of 2D, out tiled;
      M = 2B: vert_to_horiz — the tiled `pre` read as [2B][2D], bias, row-major out;
      N = 4D: the first is the gate of V_l (tiled input, add1 = P, add2 = audio term, `pre`, class rows), the second P (bias, add1), the
              third the Q projection of V0 (two gathered embedding segments of D);
      N = 2D, K = 2D: S_l's gate (G and XH tiled, add1 = v2h, add3 = T0, class rows) beside S_l's linear problem, else head1 (ReLU, out tiled);
      N = 2D, K = D: T0 beside head1 (tiled input, row-major out), S_1's gate beside S_1's linear problem (tiled G, add1 = v2h, add2 =
              audio term), else hg_0 at column 1 (one gathered embedding segment, gate);
      N = D: S_l's linear problem (tiled input, add1 = XH tiled, out tiled);  N = V: head2 (tiled input, bias)."""
    D = 256
    Ns = [(N, K) for M, N, K in problems]
    specs, n4 = [], 0
    for M, N, K in problems:
        gate_common = dict(epi=1, gateD=D, cls=2 * D)
        if K < 0 and N == 4 * D:
            s = prob(M, N, [seg("null", -K)], pre=dict(stride=4 * D, tw=2 * D), out=dict(stride=2 * D, tw=2 * D), **gate_common)
        elif K < 0:
            s = prob(M, N, [seg("null", -K)], add1=dict(extra=4 * D - N), out=dict(stride=D, tw=D), **gate_common)
        elif M == rows2b:
            s = prob(M, N, [seg("dense", K, tiled=True)], out=dict(extra=0))
        elif N == 4 * D:
            if n4 == 0:
                s = prob(M, N, [seg("dense", K, tiled=True)], bias=False, add1=dict(extra=0), add2=dict(extra=4 * D),
                         pre=dict(stride=4 * D, tw=2 * D), out=dict(stride=2 * D, tw=2 * D), **gate_common)
            elif n4 == 1:
                s = prob(M, N, [seg("dense", K, tiled=True)], add1=dict(extra=4 * D), out=dict(extra=0))
            else:
                s = prob(M, N, [seg("gather", K // 2, gstride=4), seg("gather", K // 2, gstride=4)], bias=False, out=dict(extra=0))
            n4 += 1
        elif N == 2 * D and K == 2 * D:
            if (D, D) in Ns:
                s = prob(M, N, [seg("dense", D, tiled=True), seg("dense", D, tiled=True)], add1=dict(extra=4 * D - N),
                         add3=dict(extra=0), out=dict(stride=D, tw=D), **gate_common)
            else:
                s = prob(M, N, [seg("dense", D, tiled=True), seg("dense", D, tiled=True)], relu=1, out=dict(stride=N, tw=N))
        elif N == 2 * D:
            if (2 * D, 2 * D) in Ns and (D, D) not in Ns:
                s = prob(M, N, [seg("dense", K, tiled=True)], bias=False, out=dict(extra=0))
            elif (D, D) in Ns:
                s = prob(M, N, [seg("dense", K, tiled=True)], add1=dict(extra=4 * D - N), add2=dict(extra=4 * D), out=dict(stride=D, tw=D),
                         **gate_common)
            else:
                s = prob(M, N, [seg("gather", K, gstride=4)], add1=dict(extra=4 * D - N), out=dict(stride=D, tw=D), **gate_common)
        elif N == D:
            s = prob(M, N, [seg("dense", K, tiled=True)], add1=dict(tiled=dict(stride=D, tw=D)), out=dict(stride=D, tw=D))
        else:
            s = prob(M, N, [seg("dense", K, tiled=True)], out=dict(extra=0))
        s["w_tiled"] = K > 0
        specs.append(s)
    return specs


def _chain_tables():
    import test_host_logic as H
    return [("b32", i, p, w) for i, (n, p, w) in enumerate(H.CHAIN32)] + [("b256", i, p, w) for i, (n, p, w) in enumerate(H.CHAIN256)]


@pytest.mark.gpu
@pytest.mark.parametrize("table,idx", [(t, i) for t, i, _, _ in _chain_tables()])
def test_production_launches(hip, table, idx):
    """Every launch kind of a code row at 32 clips and in a 256-clip pass (tests/test_host_logic.py CHAIN32 / CHAIN256, imported), built with
    pixelcnn.cpp's operand kinds (_production_specs), under the production knobs: the planned kernel runs (out5 = the table's plan) and every
    problem is within the bound of the float64 reference, writes nothing outside its rows and columns and gives the same bits launched
    alone (a launch of one problem may get another kernel or tile shape: the contract makes that invisible)."""
    (_, _, problems, want), = [c for c in _chain_tables() if c[0] == table and c[1] == idx]
    rng = np.random.default_rng(idx + (1000 if table == "b256" else 0))
    rows2b = 64 if table == "b32" else 512
    bs = [build(s, rng) for s in _production_specs(problems, rows2b)]
    for b in bs:
        upload(b)
    tag = f"{table}.launch{idx}"
    res, o5 = run_case(hip, tag, bs, None, want[0], rb_cb=(want[2], want[3]) if want[0] == "fast" else None)
    assert (o5[1], o5[4]) == (want[1], want[4]), f"{tag}: W / workgroups {o5[1]} / {o5[4]}, planned {want}"
    for i, b in enumerate(bs):
        reset_outputs([b])
        rc, o5, err = launch(hip, [b], None)
        assert rc >= 0, err
        alone = {k: v[0] for k, v in outputs(b).items()}
        assert same_bits(alone, res[i]), f"{tag} p{i}: differs from the same problem launched alone ({KERNELS[o5[0]]})"


# ----------------------------------------------------------------------------------------------- forced kernels at their W
def _mixed(M, K, N=96, gateD=24):
    """A linear problem (bias, add1, add2 with shift 1, add3, ReLU) and a gate problem (bias, add1 shift 1, add2, class rows of a
    non-power-of-two width, pre) of depth K, row-major: the operands every kernel reads."""
    lin = prob(M, N, K, relu=1, add1=dict(), add2=dict(shift=1), add3=dict(extra=8), out=dict(extra=12))
    gate = prob(M, 2 * gateD * 2, K, epi=1, gateD=gateD, cls=3 * gateD, add1=dict(shift=1), add2=dict(extra=0),
                pre=dict(extra=8), out=dict(extra=4))
    return [lin, gate]


# (kernel, K, W, knobs): generic16 at W = 4 / 8, generic32 at W = 4 / 8 / 16 (K = 8 x odd: only generic32 takes it), fast at W = 4 / 8
MATRIX = [("generic16", 128, 4, ""), ("generic16", 256, 8, ""), ("generic16", 512, 8, ""),
          ("generic32", 200, 4, ""), ("generic32", 136, 4, ""), ("generic32", 264, 8, ""), ("generic32", 520, 16, ""),
          ("generic32", 512, 16, ""), ("generic32", 256, 8, "")]
for _shape in (11, 21, 22, 42):
    MATRIX += [("fast", 128, 4, f"TS_SKINNY_SHAPE={_shape}"), ("fast", 512, 8, f"TS_SKINNY_SHAPE={_shape}")]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,K,W,knobs", MATRIX)
@pytest.mark.parametrize("M", [1, 17, 63, 100])
def test_forced_kernel(hip, kernel, K, W, knobs, M):
    """Each kernel forced by its knob at each wave count it can take (W follows from K), on a linear and a gate problem of the edges:
    M ragged against 16 / 32 / 64-row tiles, N not a multiple of 32 (linear), gate tiles per group = 3 (sdiv's division branch), class
    rows of width 3 gateD (not a power of two, not 2 gateD), add1 / add2 with shift 1, add3, ReLU, strides wider than the columns."""
    rng = np.random.default_rng(M * 1000 + K)
    gateD = 32 if kernel == "generic32" else 24                 # the 32-column kernel's gate tiles are 16 + 16 channels
    bs = [build(s, rng) for s in _mixed(M, K, gateD=gateD)]
    for b in bs:
        upload(b)
    full = ",".join(k for k in (FORCE[kernel], knobs) if k)
    rb_cb = None
    if kernel == "fast":
        s = int(knobs.split("=")[1])
        rb_cb = (s // 10, s % 10) if K // (16 * W) <= 4 else (min(s // 10, 2), 1)
    tag = f"{kernel}.W{W}.K{K}.M{M}" + (f".{knobs}" if knobs else "")
    _, o5 = run_case(hip, tag, bs, full, kernel, rb_cb=rb_cb)
    assert o5[1] == W, f"{tag}: W = {o5[1]}"


# ----------------------------------------------------------------------------------------------- the wide kernel
@pytest.mark.gpu
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("M,K", [(64, 256), (65, 512), (193, 256), (255, 512), (256, 128), (256, 512), (257, 256)])
def test_wide_kernel(hip, M, K, pair):
    """skinny16_wide_kernel under TS_SKINNY_WIDE_MIN=1, with the (clip-block pair, column tile) order (only where a problem has exactly 4
    row tiles: M = 193 .. 256) and column-major: K = 128 (the rolled stage loop, 2 q-steps per slice), 256 (4 stages of 2 + 2), 512
    (8 stages of 4); clamped last row blocks (M = 65, 193, 255, 257); a gate problem (gateD 40: 5 tiles per group, class rows of 2 gateD,
    pre tiled like HV) beside a linear one whose A is a tiled segment + a gather (negative ids) + a dense row-major segment."""
    rng = np.random.default_rng(M * 7 + K + pair)
    lin = prob(M, 192, [seg("dense", K // 2, tiled=True), seg("gather", K // 4, neg=True, gstride=2), seg("dense", K // 4, extra=8)],
               w_tiled=True, add1=dict(extra=64), add3=dict(extra=4), out=dict(stride=256, tw=256))
    gate = prob(M, 320, [seg("dense", K, tiled=True)], epi=1, gateD=40, cls=80, w_tiled=True, add1=dict(shift=1, extra=0),
                add2=dict(extra=16), pre=dict(stride=320, tw=64), out=dict(extra=12))
    if K // 4 % 64:
        lin["segs"] = [seg("dense", K // 2, tiled=True), seg("gather", K // 2, neg=True, gstride=2)]
    bs = [build(s, rng) for s in (lin, gate)]
    for b in bs:
        upload(b)
    run_case(hip, f"wide.pair{pair}.M{M}.K{K}", bs, f"TS_SKINNY_WIDE_MIN=1,TS_SKINNY_WIDE_PAIR={pair}", "wide")


# ----------------------------------------------------------------------------------------------- named edges
def _edge_cases():
    """(name, problem specs, knobs, kernel, (RB, CB) or None)."""
    c = []
    w1 = "TS_SKINNY_WIDE_MIN=1"
    # M ragged against the tiles, on the fast kernel at 16 / 32 / 64-row tiles and the generic ones
    for M in (1, 15, 17, 31, 33, 63, 65, 100, 193, 255, 257):
        c.append((f"ragged_fast42_M{M}", [prob(M, 128, 256, w_tiled=True, out=dict(extra=4))], "TS_SKINNY_WIDE_MIN=0,TS_SKINNY_SHAPE=42",
                  "fast", (4, 2)))
        c.append((f"ragged_fast11_M{M}", [prob(M, 80, [seg("dense", 256, tiled=True)], out=dict(tw=128, stride=128))],
                  "TS_SKINNY_SHAPE=11", "fast", (1, 1)))
        c.append((f"ragged_generic16_M{M}", [prob(M, 80, 256, add1=dict(shift=1))], FORCE["generic16"], "generic16", None))
    # M at the fast kernel's limit
    c.append(("fast_M4096", [prob(4096, 32, 128, out=dict(extra=0))], "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
    c.append(("rowmajor_M4097_generic", [prob(4097, 32, 128, out=dict(extra=0))], "TS_SKINNY_SHAPE=21", "generic16", None))
    # K shares per wave: cnt 1, 2, 3, 4, 8 on the fast kernel (W = 4: K = 64 / 128 / 192; W = 8: 384 / 512 / 1024)
    for K in (64, 128, 192, 384, 512, 1024):
        c.append((f"fast_K{K}", [prob(40, 64, [seg("dense", K, tiled=True)], w_tiled=True)], "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
    # segment boundaries: on wave shares (fast), between them (generic16 only), on wide stages, between them (fast under WIDE_MIN=1)
    c.append(("segs_on_shares_fast", [prob(48, 96, [seg("dense", 128), seg("gather", 256, gstride=3), seg("dense", 128, tiled=True)])],
              "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
    c.append(("segs_between_shares_generic16", [prob(48, 96, [seg("dense", 32), seg("gather", 448, neg=True), seg("dense", 32)])],
              "TS_SKINNY_SHAPE=21", "generic16", None))
    c.append(("segs_on_stages_wide", [prob(128, 128, [seg("dense", 64, tiled=True), seg("gather", 128, neg=True), seg("dense", 64)],
                                           w_tiled=True)], w1, "wide", None))
    c.append(("segs_between_stages_fast", [prob(128, 128, [seg("dense", 32), seg("dense", 224)], w_tiled=True)],
              w1, "fast", None))
    c.append(("null_segment_in_problem_fast", [prob(40, 64, [seg("null", 128), seg("dense", 128)])], "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
    # gate widths and class-row widths
    for gD, ld, kern in ((8, 16, "fast"), (8, 16, "generic16"), (24, 48, "fast"), (40, 160, "fast"), (40, 120, "generic16"),
                         (256, 512, "fast"), (256, 1024, "fast"), (16, 96, "generic32")):
        G = 3 if gD == 256 else 2
        c.append((f"gate_D{gD}_cls{ld}_{kern}", [prob(50, 2 * gD * G, 256, epi=1, gateD=gD, cls=ld, pre=dict(extra=4),
                                                       w_tiled=kern == "fast", out=dict(extra=4))],
                  FORCE[kern] + ",TS_SKINNY_SHAPE=21", kern, (2, 1) if kern == "fast" else None))
    c.append(("gate_D256_wide", [prob(256, 1024, [seg("dense", 512, tiled=True)], epi=1, gateD=256, cls=1024, pre=dict(stride=1024, tw=512),
                                      w_tiled=True, out=dict(stride=512, tw=512))], w1, "wide", None))
    # column tails
    c.append(("linear_N40_generic16", [prob(33, 40, 256)], FORCE["generic16"], "generic16", None))
    c.append(("linear_N40_fast", [prob(33, 40, 256, w_tiled=True)], "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
    c.append(("linear_N96_not_wide", [prob(128, 96, [seg("dense", 256, tiled=True)], w_tiled=True)], w1, "fast", None))
    # unaligned operands keep the plan off the wide kernel
    c.append(("odd_out_stride_not_wide", [prob(128, 128, [seg("dense", 256, tiled=True)], w_tiled=True, out=dict(stride=131))], w1, "fast", None))
    c.append(("add1_misaligned_not_wide", [prob(128, 128, [seg("dense", 256, tiled=True)], w_tiled=True, add1=dict(off=1, extra=4))],
              w1, "fast", None))
    # shifts
    c.append(("row_shift_generic16", [prob(40, 64, [seg("dense", 128, shift=1), seg("dense", 128)], add1=dict(shift=1), add2=dict(shift=1))],
              "", "generic16", None))
    c.append(("row_shift_generic32", [prob(40, 64, [seg("dense", 128, shift=1)], add2=dict(shift=1))], FORCE["generic32"], "generic32", None))
    # several problems: different M, K, epilogues; start[] and the problem search
    many = [prob(33, 96, 256, add1=dict()), prob(100, 64, [seg("dense", 512, tiled=True)], w_tiled=True, relu=1),
            prob(17, 64, 256, epi=1, gateD=16, cls=24, pre=dict()), prob(64, 128, [seg("null", 128)], add1=dict(), add2=dict(shift=1)),
            prob(1, 32, [seg("gather", 384, neg=True, gstride=2)]), prob(65, 48, 256, epi=1, gateD=8, cls=16, add3=dict())]
    for n in (2, 3, 6):
        c.append((f"multi{n}_fast", many[:n], "TS_SKINNY_SHAPE=21", "fast", (2, 1)))
        c.append((f"multi{n}_generic16", [dict(p, w_tiled=False, segs=[dict(s, tiled=False) for s in p["segs"]]) for p in many[:n]],
                  FORCE["generic16"], "generic16", None))
    # equal-work wide launches: the half-K problems get 2 tiles per workgroup (SD_ITEMS), an epilogue-only problem counts as 4 q-steps
    eq = [prob(256, 2048, [seg("dense", 512, tiled=True)], w_tiled=True), prob(256, 1024, [seg("dense", 256, tiled=True)], w_tiled=True),
          prob(512, 512, [seg("dense", 512, tiled=True)], w_tiled=True),
          prob(200, 1024, [seg("null", 128)], epi=1, gateD=256, cls=512, add1=dict(), out=dict(stride=512, tw=512))]
    c.append(("wide_equal_work", eq, "", "wide", None))
    c.append(("wide_equal_work_colmajor", eq, "TS_SKINNY_WIDE_PAIR=0", "wide", None))
    return c


EDGES = _edge_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [e[0] for e in EDGES])
def test_edge_case(hip, name):
    """The named edges of the chain kernels (_edge_cases): ragged M on every tile height, M at the fast kernel's 4096-row limit and one
    past it (row-major: generic16, right), cnt = 1 / 2 / 3 / 4 / 8, segment boundaries on and between wave shares and wide stages, mixed
    segment kinds, gate widths 8 / 16 / 24 / 40 / 256 and class rows of N, 2 gateD and other widths, column tails, unaligned operands,
    shifts, multi-problem launches (each problem then bit-identical to itself launched alone under the same knobs)."""
    (_, specs, knobs, kernel, rb_cb), = [e for e in EDGES if e[0] == name]
    rng = np.random.default_rng(sum(map(ord, name)))
    bs = [build(s, rng) for s in specs]
    for b in bs:
        upload(b)
    res, o5 = run_case(hip, name, bs, knobs, kernel, rb_cb=rb_cb)
    if name.startswith("wide_equal_work"):
        assert o5[4] == 240, f"{name}: {o5[4]} workgroups"       # items 1 / 2 / 1 / 4: 128 + 32 + 64 + 16
    if len(bs) > 1:
        for i, b in enumerate(bs):
            reset_outputs([b])
            rc, o5, err = launch(hip, [b], knobs)
            assert rc >= 0, err
            assert same_bits({k: v[0] for k, v in outputs(b).items()}, res[i]), f"{name} p{i}: differs launched alone ({KERNELS[o5[0]]})"


@pytest.mark.gpu
def test_refusals(hip):
    """What no kernel may compute: tiled operands past the fast kernel's 4096 rows (the generic kernels read row-major only), tiled
    operands forced onto a generic kernel, gate widths the forced kernel cannot tile, the trace knob.  Each returns -1 with a message and
    writes nothing."""
    rng = np.random.default_rng(9)
    cases = [("tiled_M4097", prob(4097, 32, [seg("dense", 128, tiled=True)], w_tiled=True), "", "generic16"),
             ("tiled_on_generic16", prob(40, 64, [seg("dense", 128, tiled=True)]), FORCE["generic16"], None),
             ("gate_D24_on_generic32", prob(40, 96, 128, epi=1, gateD=24), FORCE["generic32"], None),
             ("trace_knob", prob(40, 64, 128), "TS_SKINNY_TRACE=1", None)]
    for name, spec, knobs, _ in cases:
        b = build(spec, rng)
        upload(b)
        rc, o5, err = launch(hip, [b], knobs)
        assert rc == -1 and err, f"{name}: rc {rc}"
        print(f"\n[refused] {name}: {err}")
        check_untouched(name, b, outputs(b))
        assert (outputs(b)["out"][1] == NANBITS).all(), f"{name}: wrote output"


# ----------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(17, 128), (64, 256), (200, 512), (256, 256), (100, 384), (40, 1024)])
def test_kernels_bit_identical(hip, M, K):
    """The contract of skinny_gemm.hip: at the W plan_skinny takes from K, skinny16_kernel<W>, the fast kernel at every tile shape and the
    wide kernel (where the shape allows it: K = 128 / 256 / 512, M >= 64) give the same bits, on the same problem laid out row-major
    (generic) or tiled (fast, wide).  skinny_gemm_kernel<W> is outside that set (within the bound of the reference, not bit-identical)."""
    rng = np.random.default_rng(M + K)
    specs = [prob(M, 128, K, add1=dict(), add2=dict(shift=1), add3=dict()),
             prob(M, 256, K, epi=1, gateD=64, cls=128, pre=dict(extra=4))]
    tiled = [dict(s, w_tiled=True, segs=[dict(x, tiled=True) for x in s["segs"]]) for s in specs]
    results = {}
    W, W32 = (8 if K >= 256 else 4), (16 if K >= 512 else (8 if K >= 256 else 4))
    for layout, ss in (("rowmajor", specs), ("tiled", tiled)):
        bs = [build(s, np.random.default_rng(M + K)) for s in ss]
        for b in bs:
            upload(b)
        runs = [("generic16", FORCE["generic16"], "rowmajor"), ("generic32", FORCE["generic32"], "rowmajor")]
        runs += [(f"fast{s}", f"TS_SKINNY_WIDE_MIN=0,TS_SKINNY_SHAPE={s}", None) for s in (11, 21, 22, 42)]
        wide_ok = K in (128, 256, 512) and M >= 64
        if wide_ok:
            runs += [("wide", "TS_SKINNY_WIDE_MIN=1", "tiled")]
        for label, knobs, only in runs:
            if only and only != layout:
                continue
            want = label.rstrip("0123456789") if not label.startswith("generic") else label
            res, o5 = run_case(hip, f"ident.M{M}.K{K}.{label}.{layout}", bs, knobs, want, measured=False)
            results[(label, layout)] = res
            assert o5[1] == (W32 if label == "generic32" else W), f"{label}: W = {o5[1]}"
    base = results[("generic16", "rowmajor")]
    same = sorted(k for k, r in results.items() if all(same_bits(x, y) for x, y in zip(r, base)))
    differ = sorted(k for k in results if k not in same)
    print(f"\n[bit-identity] M={M} K={K} W={W} (generic32: W={W32}): same as generic16 {same}; differ {differ}")
    assert differ == [("generic32", "rowmajor")], f"bit-identity sets changed: {differ} differ from skinny16_kernel<{W}>"


# ----------------------------------------------------------------------------------------------- CPU: the reference's own pieces
@pytest.mark.parametrize("epi,N,K,gateD", [(0, 40, 64, 0), (0, 512, 256, 0), (0, 33, 16, 0), (1, 16, 32, 8), (1, 96, 48, 24),
                                           (1, 1024, 64, 256), (1, 48, 32, 8)])
def test_tile_weights_matches_library(epi, N, K, gateD):
    """The test's numpy weight tiling equals the library's (ts_debug_tile_weights, host-only) for linear and gate tile orders, N not a
    multiple of 16, gateD = 8 / 24 / 256."""
    L = _lib()
    lib = L.load()
    W = np.random.default_rng(N + K).standard_normal((N, K + 4)).astype(F32)
    out = np.full((N + 15) // 16 * K * 16, np.nan, F32)
    L.check(lib.ts_debug_tile_weights(W.ctypes.data_as(C.c_void_p), N, K, K + 4, epi, gateD, out.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(out, tile_weights(np.ascontiguousarray(W[:, :K]), epi, gateD))


def test_tiled_index_decode_and_hand_worked():
    """tiled_decode inverts tiled_index over whole buffers, and both agree with kernels.h's formula on elements worked by hand."""
    for W in (16, 64, 512):
        i = np.arange(48 * W)
        m, k = tiled_decode(i, W)
        assert np.array_equal(tiled_index(m, k, W), i)
        assert m.max() == 47 and k.max() == W - 1
    # (m, k, W) -> index: fragment ((m >> 4) * (W >> 4) + (k >> 4)) of 256 floats, lane (m & 15) + 16 ((k & 15) >> 2), element k & 3
    for (m, k, W), want in (((0, 0, 16), 0), ((1, 0, 16), 4), ((0, 1, 16), 1), ((0, 4, 16), 64), ((0, 16, 32), 256),
                            ((16, 0, 32), 512), ((17, 21, 32), 768 + 4 * (1 + 16) + 1), ((15, 15, 16), 4 * (15 + 48) + 3)):
        assert int(tiled_index(m, k, W)) == want, (m, k, W)
    # tiled views: element lin = row * stride + col of a [rows][stride] buffer written in a view of width tw (HV: stride 4D, view 2D)
    assert int(tiled_lin(1 * 128 + 70, 64)) == int(tiled_index(3, 6, 64))


def test_gate_reference_matches_oracle():
    """With one gate group (gateD = N / 2) the reference's gate on given pre-activations is oracle.talkshow_oracle.gated_activation (the
    channel split of GatedActivation); with several groups its tanh / sigmoid pairing is the one the weight tiles lay out (channel c of
    group g and its partner c + gateD sit in the same tile, 8 lanes apart)."""
    from oracle import talkshow_oracle as O
    rng = np.random.default_rng(4)
    v = rng.standard_normal((7, 48)) * 3
    g, t, s = gate64(v, 24)
    np.testing.assert_allclose(g.astype(F32), O.gated_activation(v), rtol=0, atol=2e-7)
    gD, G = 24, 3
    g, t, s = gate64(np.zeros((1, 2 * gD * G)), gD)
    for tile in range(2 * gD * G // 16):
        for li in range(8):
            ch = weight_column(tile, li, 2 * gD * G, 1, gD)
            partner = weight_column(tile, li + 8, 2 * gD * G, 1, gD)
            j = int(np.flatnonzero(t == ch)[0])
            assert s[j] == partner, (tile, li)


def test_bounds_catch_defects():
    """Each bound misses each defect, applied to the float64 reference of a problem that has every operand (gate: bias, add1 shift 1,
    add2, class rows, pre; linear: bias, add1 shift 1, add2, add3), by at least 10x: one 16-k step dropped, add2 ignored, add1 read at row m
    instead of m >> shift, the class row added before `pre` is stored, the sigmoid partner one channel off, the bias of column n + 1."""
    rng = np.random.default_rng(12)
    cases = {"gate": build(prob(64, 256, 512, epi=1, gateD=64, cls=128, add1=dict(shift=1), add2=dict(), pre=dict()), rng),
             "linear": build(prob(64, 128, 512, add1=dict(shift=1), add2=dict(), add3=dict()), rng)}
    for kind, b in cases.items():
        ref = reference(b)
        for d in DEFECTS:
            bad = reference(b, d)
            for name in ref:
                if d == "cls_before_pre" and name == "out" or d == "partner_off_by_one" and name == "pre":
                    continue          # a defect of the other output
                if kind == "linear" and d in ("cls_before_pre", "partner_off_by_one"):
                    continue
                e = normalized_error(name, b, bad[name][0], ref[name])
                bound = bound_of(name, b)
                print(f"\n[defect] {kind}.{name}.{d}: {e:.3e} = {e / bound:.0f} x the bound {bound:.1e}")
                assert e >= 10 * bound, f"{kind}.{name}: {d} moves the result by {e:.2e} only, under 10x the bound {bound:.1e}"
