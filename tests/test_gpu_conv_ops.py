"""Op-level tests of conv_gemm_f32, engine by engine and tile by tile, against a float64 restatement of one launch: the register-staged
engine (`csrc/conv_gemm.hip`: tiles 1 - 7, the banded launch), the LDS-DMA ring engine (`csrc/conv_gemm_ring.hip`: tiles 31 / 39 / 33, dealt
35 / 36, banded 37, the stream-K band 38) and their length-masked twins, the split-bf16 engine (`csrc/conv_gemm_split.hip`: tiles 22 / 23 /
24, both tile variants) and the 48-channel tap engine (`csrc/conv_taps48.hip`: tile 48), each forced through `ts_debug_conv_run` with a tile
id or a knob list: production's planning and launch code (plan_conv, launch_conv_plan), one process, the engine that ran reported back (`out8`).

The reference (`reference`) restates the documented semantics at the top of `csrc/kernels.h` (ConvSeg / ConvGroup / ConvParams) and reads
the very images that are uploaded through the documented index formulas; it restates no kernel's code.  Every operand sits in its own
NaN-filled allocation with NaN red zones.  NaN too: the channels of an x row outside every segment's window, weight rows from w_rows on
(without w_rows: zeros up to the 128-row padding, as production packs them), weight floats between Ktot and ldw, and every output element
a launch must not write (columns outside [out_col0, out_col0 + N), rows >= M).  A stray read shows as a non-finite output, a stray store as
a changed NaN pattern (checked bit for bit).  x rows at or beyond a clip's length in masked cases hold zeros: the kernels read them (the
contract in kernels.h: "the operand the gather parks").

Which plan runs which problem is decided by the planning code; it is written down in TABLE (one line per problem, one character per plan
of PLANS: the engine's number, `-` = refused), checked on the CPU through the dry form of the entry (`test_plan_table`) and asserted
against `out8` on the GPU: a fallback cannot silently turn a case into a test of another kernel.  Where 37 / 38 fall back to the dealt
128 x 128 tile (the table says 3) the run would repeat tile 35's and is left out.

Bounds.  The error of an element is measured in units of its own scale S = sum |x w| + |bias| + |res|.  For GELU the absolute error that
tests/test_gpu_face_ops.py::test_gelu_fast_accuracy pins (GELU_ABS = 2.2e-7 max(|v|, 1)) is taken off first and S is multiplied by 1.13
(max |GELU'|).  CEILING from fp32 error analysis of a sequential accumulation over Ktot plus the epilogue additions: (Ktot + 4) 2^-24 in
those units.  The asserted bounds are two, WHOLE_BOUND (whole-tile plans) and SK_BOUND (stream-K: a split tile is P0 + P1 (+ P2)): 2x the
largest error the first MI355X run of this file recorded (TS_MEASURED_LOG; profiles/conv_ops_measured.jsonl), each under the ceiling of
every case (asserted).  Each bound misses each defect of DEFECTS, applied to the float64 reference on the CPU, by at least 10x
(`test_bounds_catch_defects`).

Bit-identity (the contract tests/test_gpu_parity.py::test_conv_tile_shapes_agree states on one shape), here on every case: all whole-tile
plans of both engines give the same bits on the same problem, masked or not.  RingSK is outside that set: within SK_BOUND and the same bits
over three launches with another input launched in between.  The valid rows of a masked run have the bits of the same clip run alone
through the unmasked kernel of the same tile (Lin = the clip's own length).

Taps48 and Split are outside the bit-identical set too (their own k order; bf16 products), each checked like RingSK: against the reference,
the NaN pattern, the same bits over three launches with another input in between.  Taps48: T48_BOUND in the units above.  Split: two
references, as tests/test_gpu_face_ops.py::test_split_bf16_gemm has them: `reference(P, planes=...)`, the float64 emulation of the split
arithmetic (that file's split_emulate: only the kernel's fp32 accumulation differs; ceiling (Ktot + 4) 2^-24), and exact float64 (3 * 2^-16 more
with 2 planes); the bounds are that file's SPLIT_BOUND_EMU / SPLIT_BOUND_EXACT, here in units of S (that file divides by 1 + S: this asks
more), with a GELU allowance of its own (SPLIT_GELU_CEIL: the engine has its own erf, pinned by test_split_erff_accuracy).  Tile 24 (plane
images of the weights) has the bits of tile 22, and every single-group case runs again on the plain tile order (TS_SPLIT_XCD=0, a child process).
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import assert_close_measured

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GELU_ABS = 2.2e-7                   # |gelu_fast - GELU| / max(|v|, 1): GELU_BOUND of tests/test_gpu_face_ops.py::test_gelu_fast_accuracy
GELU_SLOPE = 1.13                   # max |GELU'(v)| = 1.129
# 2x the largest error the first MI355X run of this file recorded over every case, in the units above (profiles/conv_ops_measured.jsonl):
# whole tiles 3.24e-7 (5.4 x 2^-24; bands_paired, Ktot = 32, LeakyReLU), stream-K 2.38e-7 (stream_k_paired, Ktot = 256, beyond GELU_ABS).
# (That run's records were asserted against the ceilings; the record of column_window_258 is from the second run, which repeated every
# other figure to the last digit.)  None = not measured: the ceiling of the case is the bound.
WHOLE_BOUND = 6.5e-7
SK_BOUND = 4.8e-7
# conv_taps48.hip over every t48_* case, and the split engine where a case of this file exceeds the bounds of tests/test_gpu_face_ops.py
# (SPLIT_BOUND_EMU / SPLIT_BOUND_EXACT, measured there on dense K and in units of 1 + S; here they hold in units of S, which asks more).
# 2x the largest error the first MI355X run of these cases recorded (profiles/conv_ops_measured.jsonl, the records conv.t48.* / conv.split.*):
# Taps48 1.994e-7 (t48_acts_0_none: 4 taps, no activation, a null bias).  Split: two cases exceeded a starting bound, both against exact
# float64 with 2 planes: bands 7.95e-6 and bands_paired 8.74e-6 (Ktot = 32: no averaging over k, the maximum over 8.5 million elements, units of
# S; against the emulation the same runs are within 1.73e-7, so it is the arithmetic's own error, 0.19 of its 3 * 2^-16).  Everything else
# stayed inside: 2.35e-7 at most with 3 planes (bands), 2.35e-7 against the emulation.  None = not measured: the ceiling of the case is the bound.
T48_BOUND = 4.0e-7
SPLIT_EMU_OVER = {}                 # tile id -> bound against the float64 emulation of the split arithmetic, where a case here exceeded the starting bound
SPLIT_EXACT_OVER = {22: 1.75e-5, 24: 1.75e-5}   # ... against exact float64 (24 has 22's bits)
# split_erff (conv_gemm_split.hip's GELU): |err| / max(|v|, 1).  CEILING: its erf within 5e-7 relative of float64 erf (the claim in its comment),
# halved by 0.5 v, plus the fp32 roundings of v / sqrt 2, 1 + erf and the two products (<= 4 ulp of GELU): 2.5e-7 + 4 * 2^-24.  The ceiling is
# also what a Split run with GELU is allowed ahead of its accumulation error (as GELU_ABS is for gelu_fast).
SPLIT_GELU_CEIL = 2.5e-7 + 4 * U
SPLIT_ERFF_BOUND = 4.2e-7           # 2x the 2.053e-7 the first MI355X run recorded (conv.split_erff.abs_over_max_v_1); None = not measured: the ceiling
RZ = 256                           # red zone (floats) on each side of every allocation: 1 KB keeps 16-byte alignment
NANBITS = 0x7FE5A5A5                # the fill: a quiet NaN with a payload no arithmetic produces
ENGINES = ("Reg", "RegBanded", "Ring", "RingDealt", "RingBanded", "RingSK", "Taps48", "Split")
# (label, tile id, knob list): every plan a case is offered to
PLANS = [("reg1", 1, None), ("reg2", 2, None), ("reg3", 3, None), ("reg4", 4, None), ("reg5", 5, None), ("reg6", 6, None),
         ("reg7", 7, None), ("ring31", 31, None), ("ring39", 39, None), ("ring33", 33, None), ("dealt35", 35, None),
         ("dealt36", 36, None), ("banded37", 37, None), ("sk38", 38, None), ("prod", 0, None), ("prod_nodeal", 0, "TS_CONV_DEAL=0"),
         ("prod_nobands", 0, "TS_CONV_BANDS=0"), ("prod_noring", 0, "TS_CONV_RING=0"), ("prod_nopaired", 0, "TS_CONV_RING_PAIRED=0"),
         ("split22", 22, None), ("split23", 23, None), ("split24", 24, None), ("taps48", 48, None)]
SPLIT_PLANES = {22: 2, 23: 3, 24: 2}
OWN_BITS = ("RingSK", "Taps48", "Split")        # engines whose k order or arithmetic is their own: outside the "same bits as every whole-tile plan" set


def ceiling(Ktot):
    return (Ktot + 4) * U


def split_ceiling(Ktot, planes, exact):
    """Split against the emulation of its arithmetic: the fp32 accumulation, as every engine; against exact float64 with 2 planes 3 * 2^-16 more
    (each of the three products kept drops terms <= 2^-16 |x w|)."""
    return ceiling(Ktot) + (3 * 2.0 ** -16 if exact and planes == 2 else 0.0)


def bound_for(engine, Ktot):
    b = SK_BOUND if engine == "RingSK" else T48_BOUND if engine == "Taps48" else WHOLE_BOUND
    return ceiling(Ktot) if b is None else b


def split_bound(tile, Ktot, exact):
    """The bound of tests/test_gpu_face_ops.py for this tile id, or the one measured here where a case of this file exceeded it."""
    from test_gpu_face_ops import SPLIT_BOUND_EMU, SPLIT_BOUND_EXACT
    b = (SPLIT_EXACT_OVER if exact else SPLIT_EMU_OVER).get(tile, (SPLIT_BOUND_EXACT if exact else SPLIT_BOUND_EMU)[tile])
    return split_ceiling(Ktot, SPLIT_PLANES[tile], exact) if b is None else b


# ----------------------------------------------------------------------------------------------- problems
class Buf:
    """One allocation: n floats at offset RZ + off of a NaN-filled host image (red zones both sides), uploaded as is."""

    def __init__(self, n, off=0, out=False):
        self.n, self.off, self.out = n, off, out
        self.h = np.full(RZ + off + n + RZ, NANBITS, np.uint32).view(F32)
        self.d = self.d0 = None

    def body(self):
        return self.h[RZ + self.off:RZ + self.off + self.n]

    def ptr(self, floats=0):
        return self.d.data_ptr() + 4 * (RZ + self.off + floats)

    def upload(self):
        self.d0 = torch.from_numpy(self.h).cuda()      # the pristine image, for resets and for the untouched check
        self.d = self.d0.clone()

    def reset(self):
        self.d.copy_(self.d0)


def grp(segs, col0=0, net=0):
    """One ConvGroup: segs = [(d, c0, len, ntap)], its out_col0, and the network (own x / res / out buffers) it belongs to."""
    return dict(segs=[tuple(s) + (0,) * (4 - len(s)) for s in segs], col0=col0, net=net)


def taps(ds, C, c0=0):
    return [(d, c0, C) for d in ds]


def prob(B, Lin, N, groups, Lout=None, stride=1, act=2, res=None, ldx=None, ldo=None, ldr=None, off=0, ldw_extra=0, w_rows=0,
         zdiv=0, zs=0, lens=None, shr=0, shl=0, sk_ok=0, wpad_nan=0, res_is_x=0, no_bias=0):
    """One launch.  res: None / 'before' / 'after' the activation.  off: out, res and bias pointers that many floats off 16-byte alignment.
    zdiv: that many batched problems of groups[0]'s geometry, every x / o / r / b stride = zs.  lens: the clips' base lengths (masked).
    wpad_nan: the weight rows from N up to the 128-row padding hold NaN, not zeros (a kernel that reads N rows only).  res_is_x: the residual
    IS the x buffer (ldr = ldx; the output elsewhere).  no_bias: a null bias pointer."""
    Lout = Lin if Lout is None else Lout
    ldx = ldx or max(s[1] + s[2] for g in groups for s in g["segs"]) + (zdiv - 1) * zs * (zdiv > 0)
    ldo = ldo or (N if not zdiv else zdiv * zs)
    ldr = ldx if res_is_x else ldr or ldo
    return dict(B=B, Lin=Lin, Lout=Lout, stride=stride, N=N, groups=groups, act=act, res=res, ldx=ldx, ldo=ldo, ldr=ldr, off=off,
                ldw_extra=ldw_extra, w_rows=w_rows, zdiv=zdiv, zs=zs, lens=lens, shr=shr, shl=shl, sk_ok=sk_ok, wpad_nan=wpad_nan,
                res_is_x=res_is_x, no_bias=no_bias)


def ktot_of(g):
    return sum(s[2] * max(s[3], 1) for s in g["segs"])


def valid_rows(spec):
    """GEMM rows of each clip that a masked launch computes: (lens[b] >> len_shr) << len_shl (kernels.h)."""
    return [(int(n) >> spec["shr"]) << spec["shl"] for n in spec["lens"]]


def build(spec, rng):
    """Host images of every operand of `spec`.  Nothing touches the GPU."""
    B, Lin, Lout, N, ldx, ldo, ldr = (spec[k] for k in ("B", "Lin", "Lout", "N", "ldx", "ldo", "ldr"))
    M, Z, zs = B * Lout, max(spec["zdiv"], 1), spec["zs"]
    Ktot = ktot_of(spec["groups"][0])
    assert all(ktot_of(g) == Ktot for g in spec["groups"])
    ldw = Ktot + spec["ldw_extra"]
    wrows = (N + 127) // 128 * 128
    P = dict(spec=spec, M=M, Ktot=Ktot, ldw=ldw, wrows=wrows, Z=Z, nets=[], groups=[], bufs=[])
    for n in range(1 + max(g["net"] for g in spec["groups"])):
        x = Buf(B * Lin * ldx)
        img = x.body().reshape(B, Lin, ldx)
        for g in spec["groups"]:
            if g["net"] == n:
                for z in range(Z):
                    for d, c0, ln, nt in g["segs"]:
                        img[:, :, z * zs + c0:z * zs + c0 + ln] = 0.0       # channels some segment reads
        vals = rng.standard_normal((B, Lin, ldx)).astype(F32)
        np.copyto(img, vals, where=img == 0.0)
        if spec["lens"] is not None:                                         # rows at or beyond a clip's length: zeros where read
            for b, v in enumerate(valid_rows(spec)):
                tail = img[b, v * spec["stride"]:]
                tail[np.isfinite(tail)] = 0.0
        # (a column window that runs past the pitch spills into the next row's first columns: out[m ldo + out_col0 + n] as documented)
        spill = max(0, max(g["col0"] for g in spec["groups"]) + (Z - 1) * zs + N - ldo)
        net = dict(x=x, out=Buf(M * ldo + spill, off=spec["off"], out=True), out2=Buf(M * ldo + spill, off=spec["off"], out=True), res=None)
        if spec["res"] and spec["res_is_x"]:
            net["res"] = x                                                   # the same allocation, read through both pointers
        elif spec["res"]:
            net["res"] = Buf(M * ldr, off=spec["off"])
            r = net["res"].body().reshape(M, ldr)
            for g in spec["groups"]:
                if g["net"] == n:
                    for z in range(Z):
                        r[:, z * zs:z * zs + N] = rng.standard_normal((M, N)).astype(F32)
        P["nets"].append(net)
        P["bufs"] += [b for b in (x, net["out"], net["out2"], net["res"]) if b is not None and not any(b is o for o in P["bufs"])]
    for g in spec["groups"]:
        w = Buf(Z * wrows * ldw)
        wi = w.body().reshape(Z, wrows, ldw)
        wi[:, :N, :Ktot] = (rng.standard_normal((Z, N, Ktot)) / np.sqrt(Ktot)).astype(F32)
        if spec["w_rows"]:
            wi[:, :spec["w_rows"], :Ktot][:, N:] = 0.0
        elif not spec["wpad_nan"]:
            wi[:, N:, :Ktot] = 0.0                                           # the 128-row padding production packs
        bias = Buf(Z * max(zs, N), off=spec["off"])
        for z in range(Z):
            bias.body()[z * zs:z * zs + N] = rng.standard_normal(N).astype(F32)
        P["groups"].append(dict(g, w=w, bias=bias))
        P["bufs"] += [w, bias]
    return P


def struct(P, dry=False, alone=None):
    """The ts_debug_conv_problem of P.  alone = (clip b, its valid GEMM rows v): the same layer on that clip alone, unmasked, Lin = the
    clip's own length, written to the nets' second output buffers."""
    s = P["spec"]
    pr = _lib().ConvProblem()
    pr.M, pr.Lout, pr.Lin, pr.stride = P["M"], s["Lout"], s["Lin"], s["stride"]
    pr.ldx, pr.ldo, pr.ldr, pr.N, pr.Ktot, pr.act = s["ldx"], s["ldo"], s["ldr"], s["N"], P["Ktot"], s["act"]
    pr.ngroups = P["Z"] if s["zdiv"] else len(P["groups"])
    pr.res_after_act = 1 if s["res"] == "after" else 0
    pr.ldw = P["ldw"] if s["ldw_extra"] else 0
    pr.w_rows, pr.zdiv, pr.sk_ok = s["w_rows"], s["zdiv"], s["sk_ok"]
    if s["zdiv"]:
        pr.x_zs1 = pr.o_zs1 = pr.r_zs1 = pr.b_zs1 = s["zs"]
        pr.w_zs1 = P["wrows"] * P["ldw"]
    xrow = orow = 0
    if alone is not None:
        b, v = alone
        pr.M, pr.Lout, pr.Lin = v, v, v * s["stride"]
        xrow, orow = b * s["Lin"], b * s["Lout"]
    elif s["lens"] is not None:
        pr.len_shr, pr.len_shl = s["shr"], s["shl"]
        pr.lens = 4096 if dry else P["lens_d"].data_ptr()
    for i, g in enumerate(P["groups"]):
        net = P["nets"][g["net"]]
        G = pr.g[i]
        G.out_col0, G.nseg = g["col0"], len(g["segs"])
        for j, sg in enumerate(g["segs"]):
            G.seg[j].d, G.seg[j].c0, G.seg[j].len, G.seg[j].ntap = sg
        if not dry:
            G.x, G.w, G.bias = net["x"].ptr(xrow * s["ldx"]), g["w"].ptr(), None if s["no_bias"] else g["bias"].ptr()
            G.out = net["out2" if alone is not None else "out"].ptr(orow * s["ldo"])
            G.res = net["res"].ptr(orow * s["ldr"]) if net["res"] is not None else None
    return pr


def act64(v, act):
    if act == 1:
        return np.where(v >= 0, v, 0.2 * v)
    if act == 2:
        return np.maximum(v, 0.0)
    if act == 3:
        from scipy.special import erf
        return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))
    return v


DEFECTS = ("tap_shifted_one_row", "halo_reads_neighbour_clip", "last_stage_dropped", "c0_ignored", "residual_wrong_side",
           "bias_next_column", "stride_ignored", "phases_swapped", "mask_edge_one_row_late")
# conv_taps48's LDS rotation off by one (the 16-byte pieces of a tap's activation row against the weights'); the split engine's x0 y1 product
# left out (tests/test_gpu_face_ops.py::test_split_bf16_gemm's defect; planes = 2)
T48_DEFECTS = ("segments_rotated_one",)
SPLIT_DEFECTS = ("x0y1_dropped",)


def reference(P, defect=None, planes=0):
    """float64 outputs of P as kernels.h documents a launch -> per network a list of (first column, value [M][N], scale [M][N], pre).
    For group g (batched: problem z1 with every pointer advanced by z1 * its stride, conv_tile_ptrs) and row m = b Lout + t:
      pre[n] = bias[n] + sum_s sum_tap sum_c x[b Lin + t stride + d_s + tap][c0_s + c] w[n][off_s + tap len_s + c]
    with input rows outside [0, Lin) and weight rows from w_rows on as zero, weight row pitch ldw; the residual before or after the
    activation; with lens, rows t >= (lens[b] >> shr) << shl are +0.0.  `defect` (DEFECTS) alters the arithmetic.
    planes = 2 / 3: the float64 EMULATION of the split engine's arithmetic in place of the exact products (split_emulate of
    tests/test_gpu_face_ops.py: bf16 round-to-nearest-even planes of x and w, the products x_i w_j with i + j < planes, summed in float64)."""
    if planes:
        from test_gpu_face_ops import split_emulate
        drop = ((0, 1),) if defect == "x0y1_dropped" else ()
    s = P["spec"]
    B, Lin, Lout, N, ldx, ldo, ldr, zs = (s[k] for k in ("B", "Lin", "Lout", "N", "ldx", "ldo", "ldr", "zs"))
    M, Ktot, ldw = P["M"], P["Ktot"], P["ldw"]
    stride = 1 if defect == "stride_ignored" else s["stride"]
    t = np.arange(Lout)
    n = np.arange(N)
    res = [[] for _ in P["nets"]]
    for gi, g in enumerate(P["groups"]):
        net = P["nets"][g["net"]]
        xb, wb, bb = net["x"].body(), g["w"].body(), g["bias"].body()
        for z in range(P["Z"]):
            bias = bb[z * zs + ((n + 1) % N if defect == "bias_next_column" else n)].astype(F64) * (0.0 if s["no_bias"] else 1.0)
            pre = np.broadcast_to(bias, (M, N)).copy()
            scale = np.abs(pre)
            off = 0
            for si, (d, c0, ln, nt) in enumerate(g["segs"]):
                for tap in range(max(nt, 1)):
                    r = t * stride + d + tap + (1 if defect == "tap_shifted_one_row" and si == 0 else 0)
                    row = (np.arange(B)[:, None] * Lin + r[None, :]).reshape(-1)            # b Lin + input row, per GEMM row m
                    ok = np.tile((r >= 0) & (r < Lin), B)
                    if defect == "halo_reads_neighbour_clip":
                        ok = (row >= 0) & (row < B * Lin)
                    cc = z * zs + (0 if defect == "c0_ignored" else c0) + np.arange(ln)
                    if defect == "segments_rotated_one":
                        cc = cc[(np.arange(ln) + 4) % ln]
                    X = np.zeros((M, ln))
                    X[ok] = xb[row[ok][:, None] * ldx + cc[None, :]]
                    k = off + np.arange(ln)
                    if defect == "last_stage_dropped":
                        k = k[k < Ktot - 32]
                    W = wb[z * P["wrows"] * ldw + n[:, None] * ldw + k[None, :]].astype(F64)
                    if s["w_rows"]:
                        W[n >= s["w_rows"]] = 0.0
                    pre += split_emulate(X[:, :k.size], W, planes, drop) if planes else X[:, :k.size] @ W.T
                    scale += np.abs(X[:, :k.size]) @ np.abs(W).T
                    off += ln
            v = pre
            after = (s["res"] == "after") != (defect == "residual_wrong_side")
            if net["res"] is not None:
                rr = net["res"].body()[np.arange(M)[:, None] * ldr + z * zs + n[None, :]].astype(F64)
                scale = scale + np.abs(rr)
                v = act64(pre, s["act"]) + rr if after else act64(pre + rr, s["act"])
                pre = pre if after else pre + rr
            else:
                v = act64(pre, s["act"])
            if s["lens"] is not None:
                late = 1 if defect == "mask_edge_one_row_late" else 0
                live = np.concatenate([t < vr + late for vr in valid_rows(s)])
                v = np.where(live[:, None], v, 0.0)
            col0 = g["col0"] + z * zs
            if defect == "phases_swapped" and len(P["groups"]) > 1:
                col0 = P["groups"][gi ^ 1]["col0"]
            res[g["net"]].append((col0, v, scale, pre))
    return res


def normalized_error(P, got, ref, gelu_abs=GELU_ABS):
    """max error of got [M][N] against ref = (col0, value, scale, pre) in the units of the module docstring.  gelu_abs: the allowance of the
    engine's GELU (gelu_fast; the split engine has its own: SPLIT_GELU_CEIL)."""
    _, val, scale, pre = ref
    err = np.abs(np.asarray(got, F64) - val)
    if P["spec"]["act"] == 3:
        err = np.maximum(err - gelu_abs * np.maximum(np.abs(pre), 1.0), 0.0)
        scale = scale * GELU_SLOPE
    return float((err / np.maximum(scale, 1e-30)).max())


# ----------------------------------------------------------------------------------------------- the cases
def _stack(B=3, L=75, C=64, nets=1, **kw):
    return prob(B, L, C, [grp(taps((-1, 0, 1), C), net=i) for i in range(nets)], res="before", act=2, **kw)


def _down(B, Lin, C=64, **kw):
    return prob(B, Lin, C, [grp(taps((-1, 0, 1, 2), C))], Lout=Lin // 2, stride=2, act=1, **kw)


def _up(B, Lin, C=64, nets=1, **kw):
    """The two output phases of a transposed convolution (models.cpp::conv_layer_params): out[2 j] and out[2 j + 1] interleave into a
    (B, 2 Lin, C) buffer = rows of pitch 2 C, group g at out_col0 = g C."""
    gs = []
    for i in range(nets):
        gs += [grp(taps((-1, 0), C), col0=0, net=i), grp(taps((0, 1), C), col0=C, net=i)]
    return prob(B, Lin, C, gs, ldo=2 * C, act=1, **kw)


def _t48(B, T, G, ntap, d=None, zs=48, c0=0, col0=0, act=3, res="after", **kw):
    """A layer of conv_taps48.hip: G batched problems (zdiv = G, every stride zs >= 48) of one segment of `ntap` taps of 48 channels from
    row shift d (default: centred, -(ntap / 2), as the positional convolution), 48 columns."""
    return prob(B, T, 48, [grp([(-(ntap // 2) if d is None else d, c0, 48, ntap)], col0=col0)], act=act, res=res, zdiv=G, zs=zs, wpad_nan=1, **kw)


T48_DEAL = {1: (40, 1), 6: (130, 3), 9: (300, 3), 20: (520, 4)}     # (group, row tile) items -> (M, G): items = ceil(M / 128) G
MASK_LENS = (0, 1, 32, 64, 96, 100)    # valid GEMM rows of the six clips of `masked`: on a 32-row block edge, on every tile's edge, inside a block
SK_M1, SK_M2 = 12161, 6017              # the smallest M at N <= 512, Ktot <= 256 with a stream-K plan (ts_debug_conv_sk_plan): one / two groups
BAND_M, BAND_M_REG = 16549, 22529       # 130 x 4 tiles: a band plan (tile 37); the smallest M at which production's cost model takes 128 x 128
                                        # tiles at N = 512 and bands them on conv_gemm.hip (ts_debug_conv_bands): 177 x 4 tiles
BAND_CLIPS = 13
_SK_SEGS = [(-1, 0, 64), (0, 64, 128), (1, 0, 64)]


def _band_lens(L):
    return [L, L - 1, L - 31, L - 32, 1024, 1000, 640, 129, 128, 64, 1, 0, L]


def _cases():
    c = {}
    c["stack_tail"] = _stack()
    c["single_frame"] = prob(2, 1, 32, [grp(taps((-1, 0, 1), 32))], act=2)
    c["down_150"] = _down(3, 150)
    c["down_66"] = _down(3, 66)
    c["up"] = _up(3, 37)
    c["paired_stack"] = _stack(nets=2)
    c["paired_up"] = _up(3, 37, nets=2)
    for N in (39, 129):
        c[f"pose_rows_{N}"] = prob(3, 75, N, [grp(taps((-1, 0, 1), 64))], act=0, res="before", off=1)
    c["column_window_256"] = prob(3, 75, 64, [grp(taps((-1, 0, 1), 64), col0=256)], ldo=320, ldr=64, res="before")
    # 258 + 64 = 322 > 320: the last two columns of a row land in the first two of the next (the documented flat store), on the scalar path
    c["column_window_258"] = prob(3, 75, 64, [grp(taps((-1, 0, 1), 64), col0=258)], ldo=320, ldr=64, res="before")
    c["windows"] = prob(2, 50, 96, [grp([(-1, 32, 32), (0, 0, 96), (2, 128, 64)])], ldx=224, act=1)
    c["ntap_batched"] = prob(2, 40, 64, [grp([(-3, 0, 64, 7)])], act=3, res="after", zdiv=3, zs=64)
    c["strided_weights"] = prob(3, 75, 200, [grp(taps((-1, 0, 1), 64))], ldw_extra=32, w_rows=200, act=1)
    for a in range(4):
        for side in ("before", "after"):
            c[f"acts_{a}_{side}"] = prob(2, 45, 64, [grp(taps((-1, 0, 1), 64))], act=a, res=side)
    c["masked"] = _stack(B=6, L=100, lens=list(MASK_LENS))
    c["masked_down"] = _down(6, 200, lens=[2 * v for v in MASK_LENS], shr=1)
    c["masked_up"] = _up(6, 100, lens=[4 * (v // 2) for v in MASK_LENS], shr=2, shl=1)
    c["masked_paired"] = _stack(B=6, L=100, nets=2, lens=list(MASK_LENS))
    for tag, M in (("bands", BAND_M), ("bands_reg", BAND_M_REG)):
        L = M // BAND_CLIPS
        c[tag] = prob(1, M, 512, [grp(taps((0,), 32))], act=1)
        c[tag + "_paired"] = prob(1, M, 256, [grp(taps((0,), 32), net=0), grp(taps((0,), 32), net=1)], act=1)
        c[tag + "_masked"] = prob(BAND_CLIPS, L, 512, [grp(taps((0,), 32))], act=1, lens=_band_lens(L))
    c["stream_k"] = prob(1, SK_M1, 512, [grp(_SK_SEGS)], ldx=192, act=3, res="before", sk_ok=1)
    c["stream_k_paired"] = prob(1, SK_M2, 512, [grp(_SK_SEGS, net=0), grp(_SK_SEGS, net=1)], ldx=192, act=3, res="before", sk_ok=1)
    # ---- conv_taps48.hip: G batched problems of `ntap` 48-channel taps, 48 columns; weight rows 48 .. 127 of each problem hold NaN ----
    c["t48_short_clip"] = _t48(1, 5, 1, 128)           # every tap partly in the zero padding; M under one wave's 16 rows
    for T in (127, 128, 129):                          # the m < M guards of loader and epilogue either side of one 128-row tile
        c[f"t48_tile_edge_{T}"] = _t48(1, T, 2, 4)
    # (group, row tile) items dealt to the 8 XCDs in runs of per = (items + 7) >> 3: one item, fewer than XCDs, a remainder (9 = 4 x 2 + 1),
    # groups that start inside an XCD's run (5 row tiles per group, runs of 3)
    for items, (M, G) in T48_DEAL.items():
        c[f"t48_deal_{items}"] = _t48(1, M, G, 2)
    c["t48_clips"] = _t48(3, 75, 2, 16)                # halo rows must read zeros, not the neighbouring clip
    c["t48_odd_taps"] = _t48(2, 45, 2, 7)              # the ring's prologue and last stage on an odd count; one tap: no ring at all
    c["t48_one_tap"] = _t48(2, 45, 2, 1)
    c["t48_causal_back"] = _t48(2, 45, 2, 6, d=-5)     # one-sided windows
    c["t48_causal_fwd"] = _t48(2, 45, 2, 6, d=0)
    # independent pitches: 64-channel slots of which the first 16 are never read (NaN), the output 8 columns in, ldo != ldr != ldx
    c["t48_layout"] = _t48(2, 45, 2, 4, zs=64, c0=16, ldx=2 * 64 + 16, ldo=2 * 64 + 8, ldr=2 * 64, col0=8)
    for a in (0, 3):
        for side in (None, "before", "after"):
            c[f"t48_acts_{a}_{side or 'none'}"] = _t48(2, 45, 1, 4, act=a, res=side, no_bias=int(a == 0 and side is None))
    c["t48_inplace_res"] = _t48(2, 45, 2, 4, res_is_x=1)   # the face generator passes its hidden state as x and as the residual
    # ---- conv_gemm_split.hip: what the cases above do not reach ----
    # the positional convolution's layout in small: 48-channel groups read as 64-channel windows every 48 channels, 6 taps, GELU + residual after
    c["split_pos_conv"] = prob(2, 40, 48, [grp([(-3, 0, 64, 6)])], act=3, res="after", zdiv=3, zs=48)
    # 200 tiles of 128 x 128: the big variant (every small case takes 64 x 64), three taps, a residual of its own pitch, a column window
    c["split_big_layout"] = prob(8, 3200, 64, [grp(taps((-1, 0, 1), 64), col0=64)], ldo=192, ldr=64, res="before", act=1)
    return c


CASES = _cases()
# One line per problem, one character per plan of PLANS (in that order): the number of the engine that runs it (ENGINES), - = refused.
# Decided by plan_conv / conv_plan_refusal; regenerate with `python tests/test_gpu_conv_ops.py` and READ the difference.
TABLE = {
    # plan:                  1234567 (31 39 33) (35 36) 37 38, tile 0: default, DEAL=0, BANDS=0, RING=0, RING_PAIRED=0, (22 23 24) 48
    "stack_tail": "0000000222333300000777-",
    "single_frame": "0000-00222333300000777-",
    "down_150": "0000000222333300000777-",
    "down_66": "0000000222333300000777-",
    "up": "0000000222333300000777-",
    "paired_stack": "0000000222333300000777-",
    "paired_up": "0000000222333300000777-",
    "pose_rows_39": "0000000222333300000777-",
    "pose_rows_129": "0000000222333300000777-",
    "column_window_256": "0000000222333300000777-",
    "column_window_258": "0000000222333300000777-",
    "windows": "0000-00222333300000777-",
    "ntap_batched": "0000000222333300000777-",
    "strided_weights": "0000000222333300000777-",
    "acts_0_before": "0000000222333300000777-",
    "acts_0_after": "0000000222333300000777-",
    "acts_1_before": "0000000222333300000777-",
    "acts_1_after": "0000000222333300000777-",
    "acts_2_before": "0000000222333300000777-",
    "acts_2_after": "0000000222333300000777-",
    "acts_3_before": "0000000222333300000777-",
    "acts_3_after": "0000000222333300000777-",
    "masked": "0000---222333300000----",
    "masked_down": "0000---222333300000----",
    "masked_up": "0000---222333300000----",
    "masked_paired": "0000---222333300000----",
    "bands": "0000-00222334300000777-",
    "bands_paired": "0000-00222334300000777-",
    "bands_masked": "0000---222334300000----",
    "bands_reg": "0000-00222334332313777-",
    "bands_reg_paired": "0000-00222334332311777-",
    "bands_reg_masked": "0000---222334332313----",
    "stream_k": "0000000222333500000777-",
    "stream_k_paired": "0000000222333500000777-",
    "t48_short_clip": "--------------66666---6",
    "t48_tile_edge_127": "--------------66666---6",
    "t48_tile_edge_128": "--------------66666---6",
    "t48_tile_edge_129": "--------------66666---6",
    "t48_deal_1": "--------------66666---6",
    "t48_deal_6": "--------------66666---6",
    "t48_deal_9": "--------------66666---6",
    "t48_deal_20": "--------------66666---6",
    "t48_clips": "--------------66666---6",
    "t48_odd_taps": "----------------------6",
    "t48_one_tap": "----------------------6",
    "t48_causal_back": "--------------66666---6",
    "t48_causal_fwd": "--------------66666---6",
    "t48_layout": "--------------66666---6",
    "t48_acts_0_none": "--------------66666---6",
    "t48_acts_0_before": "--------------66666---6",
    "t48_acts_0_after": "--------------66666---6",
    "t48_acts_3_none": "--------------66666---6",
    "t48_acts_3_before": "--------------66666---6",
    "t48_acts_3_after": "--------------66666---6",
    "t48_inplace_res": "--------------66666---6",
    "split_pos_conv": "0000000222333300000777-",
    "split_big_layout": "0000000222333300000777-",
}


def plan_row(name):
    return TABLE[name]


def dry_row(spec):
    L = _lib()
    lib = L.load()
    P = dict(spec=spec, M=spec["B"] * spec["Lout"], Ktot=ktot_of(spec["groups"][0]), Z=max(spec["zdiv"], 1), wrows=(spec["N"] + 127) // 128 * 128,
             groups=spec["groups"], nets=[None] * 4)
    P["ldw"] = P["Ktot"] + spec["ldw_extra"]
    pr = struct(P, dry=True)
    o8 = (C.c_int * 8)()
    row = ""
    for _, tile, knobs in PLANS:
        rc = lib.ts_debug_conv_run(None, C.byref(pr), tile, knobs.encode() if knobs else None, 1, o8, None)
        row += "-" if rc < 0 else str(rc)
    return row


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


def upload(P):
    for b in P["bufs"]:
        b.upload()
    if P["spec"]["lens"] is not None:
        P["lens_d"] = torch.tensor(P["spec"]["lens"], dtype=torch.int32).cuda()


def launch(hip, pr, tile, knobs):
    """One ts_debug_conv_run -> (return code, out8, ts_last_error)."""
    L, lib, ctx = hip
    o8 = (C.c_int * 8)()
    rc = lib.ts_debug_conv_run(ctx, C.byref(pr), tile, knobs.encode() if knobs else None, 0, o8, None)
    torch.cuda.synchronize()
    return rc, tuple(o8), (lib.ts_last_error().decode() if rc < 0 else "")


def bits(t):
    return t.view(torch.int32)


def check_against_reference(tag, P, ref, engine, gelu_abs=GELU_ABS, more=()):
    """a, b, c of the module docstring on the nets' `out` buffers; -> the largest normalized error.  more: further references of the same
    outputs (the split engine has two) -> (the error against ref, the errors against each of `more`)."""
    s = P["spec"]
    M, N, ldo = P["M"], s["N"], s["ldo"]
    if engine != "Split":
        bound = bound_for(engine, P["Ktot"])
        assert bound <= ceiling(P["Ktot"]), f"{tag}: bound {bound:.1e} over the ceiling {ceiling(P['Ktot']):.1e}"
    others = [0.0] * len(more)
    worst = 0.0
    for ni, net in enumerate(P["nets"]):
        ob = net["out"]
        img = ob.d.cpu().numpy()
        body = img[RZ + ob.off:RZ + ob.off + ob.n]
        expect = ob.h.view(np.uint32).copy()
        eb = expect[RZ + ob.off:RZ + ob.off + ob.n]
        for ri, (col0, val, scale, pre) in enumerate(ref[ni]):
            idx = np.arange(M)[:, None] * ldo + col0 + np.arange(N)[None, :]       # out[m ldo + out_col0 + n]
            got = body[idx]
            assert np.isfinite(got).all(), f"{tag} net{ni} col {col0}: non-finite output (a read past an operand's extent?)"
            worst = max(worst, normalized_error(P, got, (col0, val, scale, pre), gelu_abs))
            for k, r2 in enumerate(more):
                others[k] = max(others[k], normalized_error(P, got, r2[ni][ri], gelu_abs))
            if s["lens"] is not None:
                dead = np.concatenate([np.arange(s["Lout"]) >= v for v in valid_rows(s)])
                assert (got[dead].view(np.uint32) == 0).all(), f"{tag} net{ni}: a masked row is not +0.0"
            eb[idx] = got.view(np.uint32)
        bad = np.flatnonzero(img.view(np.uint32) != expect)
        assert bad.size == 0, f"{tag} net{ni}: written outside its rows / columns at float {bad[:8] - RZ - ob.off} (pitch {ldo})"
    for b in P["bufs"]:
        if not b.out:
            assert torch.equal(bits(b.d), bits(b.d0)), f"{tag}: an input buffer changed"
    return (worst, others) if more else worst


def split_variant(tag, P, o8):
    """out8 of a Split run: 128 x 128 tiles from 200 of them on, 64 x 64 below (include/talkshow_hip_debug.h), 4 waves; a single group's
    tiles on the XCD-aware 1-D grid of 8 ceil(tiles / 8) workgroups unless TS_SPLIT_XCD=0 (read once per process)."""
    s = P["spec"]
    ng = P["Z"] if s["zdiv"] else len(P["groups"])
    t = 128 if -(-P["M"] // 128) * -(-s["N"] // 128) * ng >= 200 else 64
    tiles = -(-P["M"] // t) * -(-s["N"] // t)
    xcd = int(os.environ.get("TS_SPLIT_XCD", "8")) > 0 and ng == 1 and not s["zdiv"]
    want = (7, t, t, 4, 32, 0, 8 * -(-tiles // 8) if xcd else tiles * ng, 0)
    assert tuple(o8) == want, f"{tag}: out8 {tuple(o8)}, the shape asks for {want}"


def reset(P, which="out"):
    for net in P["nets"]:
        net[which].reset()


def run_problem(hip, name, P, only=None, other=None):
    """Problem P on every plan TABLE accepts (only: a filter on the plan's label).  Asserts the engine out8 reports, a - c against the
    reference on the first whole-tile plan and on stream-K, d (the bits of every other whole-tile plan equal the first's: then a - c hold
    for them too), e for masked problems, and that a refused plan writes nothing.  other: a second problem of the same shape (or a function
    that builds and uploads one when it is first needed), launched between the repeats of a run of an engine of OWN_BITS.  Those engines:
    a - c on every run (Split: against the float64 emulation of its arithmetic and against exact float64, each with its own bound; the
    variant out8 reports is the one the size asks for), the same bits over three launches, tile 24 the bits of tile 22."""
    s = P["spec"]
    ref = reference(P)
    row = plan_row(name)
    first = None
    ran = []
    emu, own = {}, {}
    for (label, tile, knobs), ch in zip(PLANS, row):
        if only and not only(label, ch):
            continue
        if label in ("banded37", "sk38") and ch == "3":
            continue                                   # the fallback to tile 35: that run exists
        tag = f"{name}.{label}"
        reset(P)
        rc, o8, err = launch(hip, struct(P), tile, knobs)
        if ch == "-":
            assert rc == -1 and err, f"{tag}: rc {rc}, the table says refused"
            for net in P["nets"]:
                assert torch.equal(bits(net["out"].d), bits(net["out"].d0)), f"{tag}: a refused launch wrote output"
            continue
        assert rc >= 0, f"{tag}: {err}"
        engine = ENGINES[o8[0]]
        assert str(o8[0]) == ch, f"{tag}: ran {engine} {o8}, the table says {ENGINES[int(ch)]}"
        assert o8[7] == (1 if s["lens"] is not None else 0), f"{tag}: masked flag {o8[7]}"
        print(f"\n[ran] {tag}: {engine} {o8[1]}x{o8[2]} waves={o8[3]} bk={o8[4]} second band={o8[5]} workgroups={o8[6]} masked={o8[7]}")
        ran.append(label)
        if engine in OWN_BITS:
            planes = SPLIT_PLANES[tile] if engine == "Split" else 0
            if engine == "Split":
                split_variant(tag, P, o8)
                if planes not in emu:
                    emu[planes] = reference(P, planes=planes)
                e_emu, (e_exact,) = check_against_reference(tag, P, emu[planes], engine, SPLIT_GELU_CEIL, more=(ref,))
                for kind, e, exact in (("emu", e_emu, False), ("exact", e_exact, True)):
                    bound = split_bound(tile, P["Ktot"], exact)
                    assert bound <= split_ceiling(P["Ktot"], planes, exact), f"{tag}: {kind} bound {bound:.1e} over the ceiling"
                    assert_close_measured(f"conv.split.{kind}.{tag}", np.array([e]), np.array([0.0]), bound)
            else:
                e = check_against_reference(tag, P, ref, engine)
                assert_close_measured(f"conv.{'sk' if engine == 'RingSK' else 't48'}.{tag}", np.array([e]), np.array([0.0]), bound_for(engine, P["Ktot"]))
            keep = [net["out"].d.clone() for net in P["nets"]]
            if callable(other):
                other = other()
            for rep in range(2):                       # deterministic: the same bits again, another input's launch in between
                if other is not None:
                    rc2, _, err2 = launch(hip, struct(other), tile, knobs)
                    assert rc2 == rc, err2
                reset(P)
                rc2, o82, _ = launch(hip, struct(P), tile, knobs)
                assert (rc2, o82) == (rc, o8)
                for net, k in zip(P["nets"], keep):
                    assert torch.equal(bits(net["out"].d), bits(k)), f"{tag}: {engine} bits changed on repeat {rep + 1}"
            # the same kernel on the same operands: tile 24 (plane images of the weights) = tile 22; every Taps48 run = the first
            was = own.setdefault((engine, planes, label if engine == "RingSK" else ""), (label, keep))
            for net, k in zip(P["nets"], was[1]):
                assert torch.equal(bits(net["out"].d), bits(k)), f"{tag}: bits differ from {was[0]}"
            continue
        if first is None:
            e = check_against_reference(tag, P, ref, engine)
            assert_close_measured(f"conv.whole.{tag}", np.array([e]), np.array([0.0]), bound_for(engine, P["Ktot"]))
            first = (label, [net["out"].d.clone() for net in P["nets"]])
        else:
            for ni, (net, k) in enumerate(zip(P["nets"], first[1])):
                if not torch.equal(bits(net["out"].d), bits(k)):
                    e = check_against_reference(tag, P, ref, engine)     # says where, if it is outside the contract
                    raise AssertionError(f"{tag} net{ni}: bits differ from {first[0]} (error against the reference {e:.3e})")
        if s["lens"] is not None:
            # e: each clip alone through the unmasked kernel of the same tile (37 -> its dealt tile; tile 0: the plan the clip alone gets)
            for b, v in enumerate(valid_rows(s)):
                if v == 0:
                    continue
                reset(P, "out2")
                rc2, o82, err2 = launch(hip, struct(P, alone=(b, v)), 35 if tile == 37 else tile, knobs)
                assert rc2 >= 0 and o82[7] == 0, f"{tag} clip {b} alone: {err2} {o82}"
                for ni, net in enumerate(P["nets"]):
                    lo, hi = (RZ + net["out"].off + (b * s["Lout"] + k) * s["ldo"] for k in (0, v))
                    assert torch.equal(bits(net["out"].d[lo:hi]), bits(net["out2"].d[lo:hi])), \
                        f"{tag} net{ni} clip {b}: its {v} valid rows differ from the clip run alone ({ENGINES[o82[0]]} {o82[1]}x{o82[2]})"
    return ran


# ----------------------------------------------------------------------------------------------- GPU tests
PLAN_FILTER = os.environ.get("TS_CONV_OPS_PLANS")     # only the plans whose label starts so (test_split_plain_tile_order's child process)


def _only_for(name):
    if PLAN_FILTER:
        return lambda label, ch: label.startswith(PLAN_FILTER)
    if name.startswith("bands_reg"):                   # the larger band shape exists for conv_gemm.hip's banded launch: that and a baseline
        return lambda label, ch: ch == "1" or label == "reg2"
    if name == "split_big_layout":                     # exists for the split engine's 128 x 128 variant: that, and one baseline each of the others
        return lambda label, ch: label.startswith("split") or label in ("reg1", "dealt35", "prod")
    return None


def _other_of(name, seed):
    """A second problem of the same shape, built and uploaded when an engine of OWN_BITS first asks for it."""
    def make():
        other = build(CASES[name], np.random.default_rng(seed))
        upload(other)
        return other
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("stream_k")])
def test_case(hip, name):
    """Every case of _cases (the smallest shapes at which each ConvParams feature can go wrong) on every plan that accepts it."""
    P = build(CASES[name], np.random.default_rng(sum(map(ord, name))))
    upload(P)
    ran = run_problem(hip, name, P, only=_only_for(name), other=_other_of(name, 1 + sum(map(ord, name))))
    assert ran, f"{name}: no plan ran"
    only = _only_for(name)
    for (label, _, _), ch in zip(PLANS, plan_row(name)):
        if ch in "67" and (only is None or only(label, ch)):
            assert label in ran, f"{name}: {label} (Taps48 / Split) did not run ({ran})"
    if PLAN_FILTER:
        return
    want = {"bands": "banded37", "bands_paired": "banded37", "bands_masked": "banded37"}.get(name)
    assert want is None or want in ran, f"{name}: {want} did not run"
    if name.startswith("bands_reg"):
        assert len(ran) >= 2, f"{name}: the banded launch of conv_gemm.hip did not run ({ran})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stream_k", "stream_k_paired"])
def test_stream_k(hip, name):
    """The smallest layers with a stream-K plan, three segments, residual and GELU, one and two groups: the band (tile 38) within SK_BOUND
    and deterministic, every whole-tile plan within WHOLE_BOUND and bit-identical."""
    L, lib, _ = hip
    assert lib.ts_debug_conv_sk_supported() == 1, "this device does not pass the stream-K band's hardware check"
    P = build(CASES[name], np.random.default_rng(5))
    other = build(CASES[name], np.random.default_rng(6))
    upload(P)
    upload(other)
    ran = run_problem(hip, name, P, other=other)
    assert "sk38" in ran, f"{name}: the stream-K band did not run ({ran})"


SPLIT_PLAIN_CASES = [n for n, c in CASES.items() if len(c["groups"]) == 1 and not c["zdiv"] and c["lens"] is None and not n.startswith(("t48", "stream_k", "bands_reg"))]


@pytest.mark.gpu
def test_split_plain_tile_order():
    """The split kernel with TS_SPLIT_XCD=0 (a plain 2-D tile grid instead of the XCD-aware 1-D order; the knob is read once per process,
    as tests/test_gpu_face_ops.py::test_split_bf16_gemm_plain_tile_order says): every single-group case of this file again in a child
    process, the three Split plans only, against the same references and bounds (split_variant asserts the plain grid's workgroup count)."""
    import subprocess
    import sys
    assert len(SPLIT_PLAIN_CASES) >= 20
    expr = "test_case and (" + " or ".join(f"[{n}]" for n in SPLIT_PLAIN_CASES) + ")"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k", expr],
                       env=dict({k: v for k, v in os.environ.items() if k != "TS_MEASURED_LOG"}, TS_SPLIT_XCD="0", TS_CONV_OPS_PLANS="split"),
                       capture_output=True, text=True, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(SPLIT_PLAIN_CASES)} passed" in r.stdout, r.stdout[-2000:]
    assert r.stdout.count("[ran] ") == 3 * len(SPLIT_PLAIN_CASES), "each case on split22, split23 and split24"


@pytest.mark.gpu
def test_split_erff_accuracy(hip):
    """conv_gemm_split.hip::split_erff (the rational erf of the split engine's GELU epilogue; gelu_fast is another function) against float64
    GELU.  A K = 32 GEMM on tile 22 with the identity as weights and no bias, on inputs of at most 16 significant bits: x0 = bf16(x) and
    x1 = x - x0 are both exact, the weight planes are 1 and 0, so the accumulator is x1 + x0 = the input (checked: with act 0 the output
    has the input's bits) and the output is the kernel's GELU of it.  v: every bf16 value with 2^-126 <= |v| <= 32 (the normal range from
    the smallest normal up: the clamp of the erf argument at +-4 is |v| = 5.66, +-30 is inside), +-0, and a grid of 2^16 values of 16
    significant bits over [-6, 6].  Bound: SPLIT_ERFF_BOUND (2x measured), under the ceiling SPLIT_GELU_CEIL derived beside it.  Defect: the
    tanh approximation."""
    from test_gpu_face_ops import gelu64
    hi = np.arange(0x0080, 0x4201, dtype=np.uint32)                  # bf16 bit patterns of 2^-126 .. 32
    pos = (hi << 16).view(F32)
    grid = np.linspace(-6.0, 6.0, 1 << 16).astype(F32)
    grid = ((grid.view(np.uint32) + 0x80) & 0xFFFFFF00).view(F32)    # 16 significant bits
    v = np.concatenate([pos, -pos, grid, np.array([0.0, -0.0, 4.0, -4.0, 30.0, -30.0], F32)])
    v = np.concatenate([v, np.zeros(-v.size % 32, F32)])
    M = v.size // 32
    outs = {}
    for act in (0, 3):
        P = build(prob(1, M, 32, [grp([(0, 0, 32)])], act=act, no_bias=1), np.random.default_rng(0))
        P["nets"][0]["x"].body()[:] = v
        w = P["groups"][0]["w"].body().reshape(P["wrows"], 32)
        w[:] = 0.0
        w[np.arange(32), np.arange(32)] = 1.0
        upload(P)
        rc, o8, err = launch(hip, struct(P), 22, None)
        assert rc == 7, err
        ob = P["nets"][0]["out"]
        outs[act] = ob.d.cpu().numpy()[RZ + ob.off:RZ + ob.off + ob.n]
    same = outs[0].view(np.uint32) == v.view(np.uint32)
    assert (same | (v == 0)).all() and (outs[0][v == 0] == 0).all(), "the identity GEMM does not return its input: the test's premise"
    v64 = v.astype(F64)
    ref = gelu64(v64)
    scale = np.maximum(np.abs(v64), 1.0)
    bound = SPLIT_GELU_CEIL if SPLIT_ERFF_BOUND is None else SPLIT_ERFF_BOUND
    assert bound <= SPLIT_GELU_CEIL
    assert np.isfinite(outs[3]).all()
    tanh_gelu = 0.5 * v64 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v64 + 0.044715 * v64 ** 3)))
    e = float((np.abs(tanh_gelu - ref) / scale).max())
    print(f"\n[defect] split_erff.tanh_approximation: {e:.3e} = {e / bound:.0f} x the bound {bound:.1e}")
    assert e >= 10 * bound
    assert (outs[3][v == 0] == 0).all(), "GELU(0) = 0"
    assert_close_measured("conv.split_erff.abs_over_max_v_1", outs[3].astype(F64) / scale, ref / scale, bound)


def _refusals():
    """(name, case, tile, what to change in the struct)."""
    def nseg5(pr):
        pr.g[0].nseg = 5                      # (the struct has room for four: the fifth is never read)
        pr.g[0].seg[3].len = 64

    def deep(pr):
        pr.Ktot, pr.ldx, pr.g[0].nseg = 60032, 60032, 1
        pr.g[0].seg[0].len = 60032

    def field(name, value, group=False, seg=False):
        def change(pr):
            setattr(pr.g[0].seg[0] if seg else pr.g[0] if group else pr, name, value(pr) if callable(value) else value)
        return change

    r = [(f"lens_tile{t}", "masked", t, None) for t in (5, 6, 7, 48, 22, 23, 24)] + [("lens_tile38", "stream_k_lens", 38, None)]
    r += [("lens_zdiv", "ntap_batched", 2, "lens"), ("nseg5", "stack_tail", 2, nseg5), ("ktot_60032", "stack_tail", 2, deep),
          ("windows_tile5", "windows", 5, None), ("unknown_tile", "stack_tail", 99, None)]
    r += [(f"ring{t}_len48", "len48", t, None) for t in (31, 39, 33, 35, 36, 37, 38)]
    # the split engine: chunks of 32 k; 16-byte loads of x and w rows (c0, ldx, ldw, the pointers, the strides between batched problems);
    # plane images of the weights: two planes only, every row and problem on a chunk of 32; tile 24 makes its images itself
    r += [(f"split{t}_len48", "len48", t, None) for t in (22, 23, 24)]
    for t in (22, 23, 24):
        r += [(f"split{t}_c0_2", "stack_tail", t, field("c0", 2, seg=True)), (f"split{t}_ldx_66", "stack_tail", t, field("ldx", 66)),
              (f"split{t}_x_4_bytes_off", "stack_tail", t, field("x", lambda pr: pr.g[0].x + 4, group=True)),
              (f"split{t}_w_4_bytes_off", "stack_tail", t, field("w", lambda pr: pr.g[0].w + 4, group=True)),
              (f"split{t}_x_zs1_66", "ntap_batched", t, field("x_zs1", 66)), (f"split{t}_x_zs0_2", "ntap_batched", t, field("x_zs0", 2)),
              (f"split{t}_ldw_194", "stack_tail", t, field("ldw", 194)), (f"split{t}_w_zs1_off_2", "ntap_batched", t, field("w_zs1", lambda pr: pr.w_zs1 + 2))]
    r += [("split23_plane_images", "stack_tail", 23, field("w_planes", 1)), ("split24_given_images", "stack_tail", 24, field("w_planes", 1)),
          ("reg2_plane_images", "stack_tail", 2, field("w_planes", 1)),
          ("split24_ldw_196", "stack_tail", 24, field("ldw", 196)), ("split22_images_ldw_196", "stack_tail", 22, lambda pr: (field("ldw", 196)(pr), field("w_planes", 1)(pr))),
          ("split24_w_zs1_off_4", "ntap_batched", 24, field("w_zs1", lambda pr: pr.w_zs1 + 4))]
    return r


@pytest.mark.gpu
def test_refusals(hip):
    """What no kernel may compute: lens on a tile without a masked kernel (5 / 6 / 7 / 38 / 48) or with batched problems, more than 4
    segments, Ktot over 60 000, a ring tile with a segment that is no multiple of 32, the 64-deep tile 5 on segments of 32 and 96, an
    unknown tile id; on the Split tiles lens, a segment of 48, and whatever breaks the kernel's 16-byte loads or its plane images (the
    list in _refusals).  Each returns -1 with a message before anything is launched (the checks are the host's: no kernel is handed a
    layout it would misread) and leaves the output's NaN fill intact."""
    specs = dict(CASES, len48=prob(2, 40, 64, [grp([(-1, 0, 48), (0, 0, 48)])]), stream_k_lens=dict(CASES["stream_k"], lens=[SK_M1 - 5]))
    built = {}
    for name, case, tile, change in _refusals():
        if case not in built:
            built[case] = build(specs[case], np.random.default_rng(3))
            upload(built[case])
        P = built[case]
        if change == "lens":
            P = dict(P, spec=dict(P["spec"], lens=[40, 7]), lens_d=torch.tensor([40, 7], dtype=torch.int32).cuda())
        pr = struct(P)
        if callable(change):
            change(pr)
        rc, o8, err = launch(hip, pr, tile, None)
        assert rc == -1 and err, f"{name}: rc {rc}"
        print(f"\n[refused] {name}: {err}")
        for net in P["nets"]:
            assert torch.equal(bits(net["out"].d), bits(net["out"].d0)), f"{name}: wrote output"


# ----------------------------------------------------------------------------------------------- CPU: the reference, the bounds, the table
def _torch_weights(P, tap_tables, transposed):
    """The packed weights of P turned back into torch's layout by models.cpp::pack_conv_layer's tap tables: tap_tables[g][s] = kernel index of
    segment s of group g.  -> weight (Cout, Cin, K) (transposed: (Cin, Cout, K)), bias (Cout,)."""
    s = P["spec"]
    N, Cin = s["N"], s["groups"][0]["segs"][0][2]
    K = max(max(t) for t in tap_tables) + 1
    w = np.zeros((N, Cin, K))
    for g, tt in zip(P["groups"], tap_tables):
        wi = g["w"].body().reshape(P["wrows"], P["ldw"])[:N].astype(F64)
        for si, kk in enumerate(tt):
            w[:, :, kk] = wi[:, si * Cin:(si + 1) * Cin]
    bias = P["groups"][0]["bias"].body()[:N].astype(F64)
    return torch.from_numpy(w.transpose(1, 0, 2).copy() if transposed else w), torch.from_numpy(bias)


def test_reference_matches_torch():
    """The float64 reference on stack_tail / single_frame (Conv1d k3 p1), down (Conv1d k4 s2 p1) and up (ConvTranspose1d k4 s2 p1) equals
    torch.nn.functional in float64 to 1e-12: an implementation it shares no code with."""
    import torch.nn.functional as Fn
    for name, tt, kw in (("stack_tail", [[0, 1, 2]], dict(padding=1)), ("single_frame", [[0, 1, 2]], dict(padding=1)),
                         ("down_150", [[0, 1, 2, 3]], dict(stride=2, padding=1)), ("down_66", [[0, 1, 2, 3]], dict(stride=2, padding=1)),
                         ("up", [[3, 1], [2, 0]], dict(stride=2, padding=1))):
        spec = copy.deepcopy(CASES[name])
        P = build(spec, np.random.default_rng(1))
        s = P["spec"]
        C0 = s["groups"][0]["segs"][0][2]
        x = torch.from_numpy(P["nets"][0]["x"].body().reshape(s["B"], s["Lin"], s["ldx"])[:, :, :C0].astype(F64)).permute(0, 2, 1)
        up = name == "up"
        w, b = _torch_weights(P, tt, up)
        if up:
            for g in P["groups"][1:]:                     # one ConvTranspose1d has one bias: both phases carry it
                g["bias"].body()[:] = P["groups"][0]["bias"].body()
        y = (Fn.conv_transpose1d if up else Fn.conv1d)(x, w, b, **kw).permute(0, 2, 1).numpy()       # (B, Lout', N)
        ref = reference(P)[0]
        if up:
            got = np.empty((P["M"], 2, s["N"]))
            for col0, val, _, pre in ref:
                got[:, col0 // s["N"]] = pre
            got = got.reshape(s["B"], 2 * s["Lin"], s["N"])
        else:
            pre = ref[0][3]
            if s["res"]:
                pre = pre - P["nets"][0]["res"].body().reshape(P["M"], s["ldr"])[:, :s["N"]].astype(F64)
            got = pre.reshape(s["B"], s["Lout"], s["N"])
        err = float(np.abs(got - y).max())
        print(f"\n[reference vs torch] {name}: {err:.2e}")
        assert got.shape == y.shape and err <= 1e-12, f"{name}: {err}"


def test_bounds_catch_defects():
    """Each bound (the ceiling, while nothing is measured) misses each defect of DEFECTS by at least 10x, each applied to the float64
    reference of a problem that has every operand: a strided, masked layer with three windows that cover the row, bias and a residual
    before LeakyReLU; the two phases of `up` for the swap."""
    rng = np.random.default_rng(12)
    full = build(prob(4, 40, 64, [grp([(-1, 32, 32), (0, 0, 64), (1, 32, 32), (2, 0, 32)])], Lout=20, stride=2, act=1, res="before",
                      lens=[40, 38, 20, 14], shr=1), rng)
    up = build(CASES["up"], rng)
    for d in DEFECTS:
        P = up if d == "phases_swapped" else full
        ref, bad = reference(P), reference(P, d)
        N = P["spec"]["N"]
        want = {col0: (col0, v, sc, pre) for col0, v, sc, pre in ref[0]}
        e = max(normalized_error(P, v, want[col0]) for col0, v, _, _ in bad[0])
        for engine in ("Reg", "RingSK"):
            bound = bound_for(engine, P["Ktot"])
            print(f"\n[defect] {d}: {e:.3e} = {e / bound:.0f} x the {engine} bound {bound:.1e}")
            assert e >= 10 * bound, f"{d} moves the result by {e:.2e} only, under 10x the bound {bound:.1e}"
        assert N == 64


def _defect_error(P, d, planes=0, against=None):
    """How far defect d moves the float64 reference of P (planes: the emulation of the split arithmetic), in the file's units."""
    ref = reference(P, planes=planes) if against is None else against
    bad = reference(P, d, planes=planes)
    want = {col0: r for col0, *r in ref[0]}
    moved = {col0: v for col0, v, _, _ in bad[0]}
    if not all(np.isfinite(v).all() for v in moved.values()):
        return float("inf")                            # the defect reads the NaN fill (c0_ignored on a window that starts 16 channels in): non-finite output
    if d == "phases_swapped":
        return max(normalized_error(P, v, (c,) + tuple(want[c]), SPLIT_GELU_CEIL) for c, v in moved.items())
    return max(normalized_error(P, bad[0][i][1], ref[0][i], SPLIT_GELU_CEIL) for i in range(len(ref[0])))


def test_new_bounds_catch_defects():
    """The Taps48 and Split bounds (the ceilings, while nothing is measured) miss by at least 10x every defect of DEFECTS that applies to
    their cases, each applied to the float64 reference: Taps48 on t48_layout (two clips, two groups, c0 = 16, bias, a residual) with the
    LDS rotation off by one piece of 16 bytes in addition; Split on split_pos_conv, on a strided layer with three windows, bias and a
    residual, and on the two phases of `up`, with the x0 y1 product dropped in addition (against the emulation and against exact float64,
    as tests/test_gpu_face_ops.py::test_split_bf16_gemm does)."""
    rng = np.random.default_rng(13)
    t48 = build(CASES["t48_layout"], rng)
    for d in ("tap_shifted_one_row", "halo_reads_neighbour_clip", "last_stage_dropped", "c0_ignored", "residual_wrong_side", "bias_next_column") + T48_DEFECTS:
        e, bound = _defect_error(t48, d), bound_for("Taps48", t48["Ktot"])
        print(f"\n[defect] taps48 {d}: {e:.3e} = {e / bound:.0f} x the bound {bound:.1e}")
        assert e >= 10 * bound, f"{d} moves the result by {e:.2e} only, under 10x the bound {bound:.1e}"
    pos = build(CASES["split_pos_conv"], rng)
    full = build(prob(4, 40, 64, [grp([(-1, 32, 32), (0, 0, 64), (1, 32, 32), (2, 0, 32)])], Lout=20, stride=2, act=1, res="before"), rng)
    up = build(CASES["up"], rng)
    applies = {"tap_shifted_one_row": (pos, full), "halo_reads_neighbour_clip": (pos, full), "last_stage_dropped": (pos, full), "c0_ignored": (full,),
               "residual_wrong_side": (pos, full), "bias_next_column": (pos, full), "stride_ignored": (full,), "phases_swapped": (up,)}
    for d, Ps in applies.items():
        for P in Ps:
            e = _defect_error(P, d)
            for tile in (22, 23, 24):
                bound = max(split_bound(tile, P["Ktot"], False), split_bound(tile, P["Ktot"], True))
                print(f"\n[defect] split{tile} {d}: {e:.3e} = {e / bound:.0f} x the bound {bound:.1e}")
                assert e >= 10 * bound, f"{d} moves the result by {e:.2e} only, under 10x the tile {tile} bound {bound:.1e}"
    for P in (pos, full):
        for tile in (22, 24):
            for exact in (False, True):
                e = _defect_error(P, "x0y1_dropped", planes=2, against=reference(P) if exact else None)
                bound = split_bound(tile, P["Ktot"], exact)
                print(f"\n[defect] split{tile} x0y1_dropped vs {'float64' if exact else 'emulation'}: {e:.3e} = {e / bound:.0f} x the bound {bound:.1e}")
                assert e >= 10 * bound, f"x0y1_dropped moves the result by {e:.2e} only, under 10x the bound {bound:.1e}"


def test_split_emulation_self_check():
    """The emulation of the split arithmetic that `reference` takes from tests/test_gpu_face_ops.py, on a case of this file: with 3 planes
    it is the exact reference to fp32 grade (<= 3 dropped terms of 2^-24 per product), with 2 planes within 3 * 2^-16 and not closer than
    2^-20 (the planes really are bf16), and the planes of a bf16-exact operand are the operand and zero."""
    from test_gpu_face_ops import split_planes
    P = build(CASES["split_pos_conv"], np.random.default_rng(2))
    exact = reference(P)
    for planes, lo, hi in ((3, 0.0, 3 * U), (2, 2.0 ** -20, 3 * 2.0 ** -16)):
        emu = reference(P, planes=planes)
        e = max(float((np.abs(a[3] - b[3]) / b[2]).max()) for a, b in zip(emu[0], exact[0]))
        print(f"\n[emulation] {planes} planes: pre-activation within {e:.3e} of float64")
        assert lo <= e <= hi, f"{planes} planes: {e:.3e}"
    v = np.array([1.5, -3.0, 0.0078125, 6.0], F32)
    p0, p1 = split_planes(v, 2)
    assert np.array_equal(p0, v) and not p1.any()


def test_bounds_under_every_ceiling():
    for name, spec in CASES.items():
        K = ktot_of(spec["groups"][0])
        for engine in ("Reg", "RingSK", "Taps48"):
            assert bound_for(engine, K) <= ceiling(K), f"{name}: the {engine} bound is over the ceiling {ceiling(K):.2e}"
        for tile, planes in SPLIT_PLANES.items():
            for exact in (False, True):
                assert split_bound(tile, K, exact) <= split_ceiling(K, planes, exact), f"{name}: the tile {tile} bound is over the ceiling"


def test_plan_table():
    """TABLE is what the planning code decides (the dry form of ts_debug_conv_run: plan_conv + conv_plan_refusal, no device), every plan
    of the issue's list runs somewhere, and the shapes found on the CPU are the smallest: SK_M1 / SK_M2 (ts_debug_conv_sk_plan), BAND_M_REG
    (ts_debug_conv_bands)."""
    lib = _lib().load()
    assert set(TABLE) == set(CASES)
    for name, spec in CASES.items():
        assert dry_row(spec) == TABLE[name], f"{name}: the planning code says {dry_row(spec)}"
    for i, (label, _, _) in enumerate(PLANS):
        assert any(row[i] != "-" for row in TABLE.values()), f"{label} accepts no case"
    for e in range(8):
        assert any(str(e) in row for row in TABLE.values()), f"no case runs {ENGINES[e]}"
    for name, row in TABLE.items():
        t48 = name.startswith("t48")
        assert (row[22] == "6") == t48, f"{name}: conv_taps48 takes the t48 cases and no other"
        want = "---" if t48 or CASES[name]["lens"] is not None else "777"
        assert row[19:22] == want, f"{name}: the Split tiles take every unmasked case with segments that are multiples of 32"
    for name in CASES:
        if "masked" in name:
            assert [TABLE[name][i] for i in (4, 5, 6)] == ["-"] * 3, f"{name}: tiles 5 / 6 / 7 have no masked kernel"
            assert TABLE[name][13] in "-3", f"{name}: the stream-K band has no masked kernel"
    assert TABLE["windows"][4] == "-" and TABLE["bands"][12] == "4" and TABLE["stream_k"][13] == "5"
    o6, o4 = (C.c_int * 6)(), (C.c_int * 4)()
    for groups, M in ((1, SK_M1), (2, SK_M2)):
        assert lib.ts_debug_conv_sk_plan(M, 512, 256, groups, o6) == 1
        assert all(lib.ts_debug_conv_sk_plan(m, n, k, groups, o6) != 1 for n in (128, 256, 384, 512) for k in range(32, 257, 32)
                   for m in range(1, M))
    assert lib.ts_debug_conv_bands(BAND_M_REG, 512, 1, o4) == 1 and lib.ts_debug_conv_bands(BAND_M_REG - 1, 512, 1, o4) == 0


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("#" + " " * 21 + "  " + " ".join(f"{t}" for _, t, _ in PLANS))
    for name, spec in CASES.items():
        print(f'    "{name}": "{dry_row(spec)}",')
