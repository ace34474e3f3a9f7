"""Op-level tests of conv_gemm_f32, engine by engine and tile by tile, against a float64 restatement of one launch: the register-staged
engine (`csrc/conv_gemm.hip`: tiles 1 - 7, the banded launch), the LDS-DMA ring engine (`csrc/conv_gemm_ring.hip`: tiles 31 / 39 / 33, dealt
35 / 36, banded 37, the stream-K band 38) and their length-masked twins, each forced through `ts_debug_conv_run` with a tile id or a knob
list: production's planning and launch code (plan_conv, launch_conv_plan), one process, the engine that ran reported back (`out8`).

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
"""
import copy
import ctypes as C

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
RZ = 256                            # red zone (floats) on each side of every allocation: 1 KB keeps 16-byte alignment
NANBITS = 0x7FE5A5A5                # the fill: a quiet NaN with a payload no arithmetic produces
ENGINES = ("Reg", "RegBanded", "Ring", "RingDealt", "RingBanded", "RingSK", "Taps48", "Split")
# (label, tile id, knob list): every plan a case is offered to
PLANS = [("reg1", 1, None), ("reg2", 2, None), ("reg3", 3, None), ("reg4", 4, None), ("reg5", 5, None), ("reg6", 6, None),
         ("reg7", 7, None), ("ring31", 31, None), ("ring39", 39, None), ("ring33", 33, None), ("dealt35", 35, None),
         ("dealt36", 36, None), ("banded37", 37, None), ("sk38", 38, None), ("prod", 0, None), ("prod_nodeal", 0, "TS_CONV_DEAL=0"),
         ("prod_nobands", 0, "TS_CONV_BANDS=0"), ("prod_noring", 0, "TS_CONV_RING=0"), ("prod_nopaired", 0, "TS_CONV_RING_PAIRED=0")]


def ceiling(Ktot):
    return (Ktot + 4) * U


def bound_for(engine, Ktot):
    b = SK_BOUND if engine == "RingSK" else WHOLE_BOUND
    return ceiling(Ktot) if b is None else b


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
         zdiv=0, zs=0, lens=None, shr=0, shl=0, sk_ok=0):
    """One launch.  res: None / 'before' / 'after' the activation.  off: out, res and bias pointers that many floats off 16-byte alignment.
    zdiv: that many batched problems of groups[0]'s geometry, every x / o / r / b stride = zs.  lens: the clips' base lengths (masked)."""
    Lout = Lin if Lout is None else Lout
    ldx = ldx or max(s[1] + s[2] for g in groups for s in g["segs"]) + (zdiv - 1) * zs * (zdiv > 0)
    ldo = ldo or (N if not zdiv else zdiv * zs)
    return dict(B=B, Lin=Lin, Lout=Lout, stride=stride, N=N, groups=groups, act=act, res=res, ldx=ldx, ldo=ldo, ldr=ldr or ldo, off=off,
                ldw_extra=ldw_extra, w_rows=w_rows, zdiv=zdiv, zs=zs, lens=lens, shr=shr, shl=shl, sk_ok=sk_ok)


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
        if spec["res"]:
            net["res"] = Buf(M * ldr, off=spec["off"])
            r = net["res"].body().reshape(M, ldr)
            for g in spec["groups"]:
                if g["net"] == n:
                    for z in range(Z):
                        r[:, z * zs:z * zs + N] = rng.standard_normal((M, N)).astype(F32)
        P["nets"].append(net)
        P["bufs"] += [b for b in (x, net["out"], net["out2"], net["res"]) if b is not None]
    for g in spec["groups"]:
        w = Buf(Z * wrows * ldw)
        wi = w.body().reshape(Z, wrows, ldw)
        wi[:, :N, :Ktot] = (rng.standard_normal((Z, N, Ktot)) / np.sqrt(Ktot)).astype(F32)
        if spec["w_rows"]:
            wi[:, :spec["w_rows"], :Ktot][:, N:] = 0.0
        else:
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
            G.x, G.w, G.bias = net["x"].ptr(xrow * s["ldx"]), g["w"].ptr(), g["bias"].ptr()
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


def reference(P, defect=None):
    """float64 outputs of P as kernels.h documents a launch -> per network a list of (first column, value [M][N], scale [M][N], pre).
    For group g (batched: problem z1 with every pointer advanced by z1 * its stride, conv_tile_ptrs) and row m = b Lout + t:
      pre[n] = bias[n] + sum_s sum_tap sum_c x[b Lin + t stride + d_s + tap][c0_s + c] w[n][off_s + tap len_s + c]
    with input rows outside [0, Lin) and weight rows from w_rows on as zero, weight row pitch ldw; the residual before or after the
    activation; with lens, rows t >= (lens[b] >> shr) << shl are +0.0.  `defect` (DEFECTS) alters the arithmetic."""
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
            bias = bb[z * zs + ((n + 1) % N if defect == "bias_next_column" else n)].astype(F64)
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
                    X = np.zeros((M, ln))
                    X[ok] = xb[row[ok][:, None] * ldx + cc[None, :]]
                    k = off + np.arange(ln)
                    if defect == "last_stage_dropped":
                        k = k[k < Ktot - 32]
                    W = wb[z * P["wrows"] * ldw + n[:, None] * ldw + k[None, :]].astype(F64)
                    if s["w_rows"]:
                        W[n >= s["w_rows"]] = 0.0
                    pre += X[:, :k.size] @ W.T
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


def normalized_error(P, got, ref):
    """max error of got [M][N] against ref = (col0, value, scale, pre) in the units of the module docstring."""
    _, val, scale, pre = ref
    err = np.abs(np.asarray(got, F64) - val)
    if P["spec"]["act"] == 3:
        err = np.maximum(err - GELU_ABS * np.maximum(np.abs(pre), 1.0), 0.0)
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


MASK_LENS = (0, 1, 32, 64, 96, 100)     # valid GEMM rows of the six clips of `masked`: on a 32-row block edge, on every tile's edge, inside a block
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
    return c


CASES = _cases()
# One line per problem, one character per plan of PLANS (in that order): the number of the engine that runs it (ENGINES), - = refused.
# Decided by plan_conv / conv_plan_refusal; regenerate with `python tests/test_gpu_conv_ops.py` and READ the difference.
TABLE = {
    # plan:                  1234567 (31 39 33) (35 36) 37 38, tile 0: default, DEAL=0, BANDS=0, RING=0, RING_PAIRED=0
    "stack_tail": "0000000222333300000",
    "single_frame": "0000-00222333300000",
    "down_150": "0000000222333300000",
    "down_66": "0000000222333300000",
    "up": "0000000222333300000",
    "paired_stack": "0000000222333300000",
    "paired_up": "0000000222333300000",
    "pose_rows_39": "0000000222333300000",
    "pose_rows_129": "0000000222333300000",
    "column_window_256": "0000000222333300000",
    "column_window_258": "0000000222333300000",
    "windows": "0000-00222333300000",
    "ntap_batched": "0000000222333300000",
    "strided_weights": "0000000222333300000",
    "acts_0_before": "0000000222333300000",
    "acts_0_after": "0000000222333300000",
    "acts_1_before": "0000000222333300000",
    "acts_1_after": "0000000222333300000",
    "acts_2_before": "0000000222333300000",
    "acts_2_after": "0000000222333300000",
    "acts_3_before": "0000000222333300000",
    "acts_3_after": "0000000222333300000",
    "masked": "0000---222333300000",
    "masked_down": "0000---222333300000",
    "masked_up": "0000---222333300000",
    "masked_paired": "0000---222333300000",
    "bands": "0000-00222334300000",
    "bands_paired": "0000-00222334300000",
    "bands_masked": "0000---222334300000",
    "bands_reg": "0000-00222334332313",
    "bands_reg_paired": "0000-00222334332311",
    "bands_reg_masked": "0000---222334332313",
    "stream_k": "0000000222333500000",
    "stream_k_paired": "0000000222333500000",
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


def check_against_reference(tag, P, ref, engine):
    """a, b, c of the module docstring on the nets' `out` buffers; -> the largest normalized error."""
    s = P["spec"]
    M, N, ldo = P["M"], s["N"], s["ldo"]
    bound = bound_for(engine, P["Ktot"])
    assert bound <= ceiling(P["Ktot"]), f"{tag}: bound {bound:.1e} over the ceiling {ceiling(P['Ktot']):.1e}"
    worst = 0.0
    for ni, net in enumerate(P["nets"]):
        ob = net["out"]
        img = ob.d.cpu().numpy()
        body = img[RZ + ob.off:RZ + ob.off + ob.n]
        expect = ob.h.view(np.uint32).copy()
        eb = expect[RZ + ob.off:RZ + ob.off + ob.n]
        for col0, val, scale, pre in ref[ni]:
            idx = np.arange(M)[:, None] * ldo + col0 + np.arange(N)[None, :]       # out[m ldo + out_col0 + n]
            got = body[idx]
            assert np.isfinite(got).all(), f"{tag} net{ni} col {col0}: non-finite output (a read past an operand's extent?)"
            worst = max(worst, normalized_error(P, got, (col0, val, scale, pre)))
            if s["lens"] is not None:
                dead = np.concatenate([np.arange(s["Lout"]) >= v for v in valid_rows(s)])
                assert (got[dead].view(np.uint32) == 0).all(), f"{tag} net{ni}: a masked row is not +0.0"
            eb[idx] = got.view(np.uint32)
        bad = np.flatnonzero(img.view(np.uint32) != expect)
        assert bad.size == 0, f"{tag} net{ni}: written outside its rows / columns at float {bad[:8] - RZ - ob.off} (pitch {ldo})"
    for b in P["bufs"]:
        if not b.out:
            assert torch.equal(bits(b.d), bits(b.d0)), f"{tag}: an input buffer changed"
    return worst


def reset(P, which="out"):
    for net in P["nets"]:
        net[which].reset()


def run_problem(hip, name, P, only=None, other=None):
    """Problem P on every plan TABLE accepts (only: a filter on the plan's label).  Asserts the engine out8 reports, a - c against the
    reference on the first whole-tile plan and on stream-K, d (the bits of every other whole-tile plan equal the first's: then a - c hold
    for them too), e for masked problems, and that a refused plan writes nothing.  other: a second problem of the same shape, launched
    between the repeats of a stream-K run."""
    s = P["spec"]
    ref = reference(P)
    row = plan_row(name)
    first = None
    ran = []
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
        if engine == "RingSK":
            e = check_against_reference(tag, P, ref, engine)
            assert_close_measured(f"conv.sk.{tag}", np.array([e]), np.array([0.0]), bound_for(engine, P["Ktot"]))
            keep = [net["out"].d.clone() for net in P["nets"]]
            for rep in range(2):                       # deterministic: the same bits again, another input's launch in between
                if other is not None:
                    rc2, _, err2 = launch(hip, struct(other), tile, knobs)
                    assert rc2 == rc, err2
                reset(P)
                rc2, o82, _ = launch(hip, struct(P), tile, knobs)
                assert (rc2, o82) == (rc, o8)
                for net, k in zip(P["nets"], keep):
                    assert torch.equal(bits(net["out"].d), bits(k)), f"{tag}: stream-K bits changed on repeat {rep + 1}"
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
def _only_for(name):
    if name.startswith("bands_reg"):                   # the larger band shape exists for conv_gemm.hip's banded launch: that and a baseline
        return lambda label, ch: ch == "1" or label == "reg2"
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("stream_k")])
def test_case(hip, name):
    """Every case of _cases (the smallest shapes at which each ConvParams feature can go wrong) on every plan that accepts it."""
    P = build(CASES[name], np.random.default_rng(sum(map(ord, name))))
    upload(P)
    ran = run_problem(hip, name, P, only=_only_for(name))
    assert ran, f"{name}: no plan ran"
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


def _refusals():
    """(name, case, tile, what to change in the struct)."""
    def nseg5(pr):
        pr.g[0].nseg = 5                      # (the struct has room for four: the fifth is never read)
        pr.g[0].seg[3].len = 64

    def deep(pr):
        pr.Ktot, pr.ldx, pr.g[0].nseg = 60032, 60032, 1
        pr.g[0].seg[0].len = 60032

    r = [(f"lens_tile{t}", "masked", t, None) for t in (5, 6, 7, 48)] + [("lens_tile38", "stream_k_lens", 38, None)]
    r += [("lens_zdiv", "ntap_batched", 2, "lens"), ("nseg5", "stack_tail", 2, nseg5), ("ktot_60032", "stack_tail", 2, deep),
          ("windows_tile5", "windows", 5, None), ("unknown_tile", "stack_tail", 99, None), ("split_tile", "stack_tail", 22, None)]
    r += [(f"ring{t}_len48", "len48", t, None) for t in (31, 39, 33, 35, 36, 37, 38)]
    return r


@pytest.mark.gpu
def test_refusals(hip):
    """What no kernel may compute: lens on a tile without a masked kernel (5 / 6 / 7 / 38 / 48) or with batched problems, more than 4
    segments, Ktot over 60 000, a ring tile with a segment that is no multiple of 32, the 64-deep tile 5 on segments of 32 and 96, an
    unknown tile id, the Split ids.  Each returns -1 with a message and leaves the output's NaN fill intact."""
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


def test_bounds_under_every_ceiling():
    for name, spec in CASES.items():
        K = ktot_of(spec["groups"][0])
        for engine in ("Reg", "RingSK"):
            assert bound_for(engine, K) <= ceiling(K), f"{name}: the {engine} bound is over the ceiling {ceiling(K):.2e}"


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
    for e in range(6):
        assert any(str(e) in row for row in TABLE.values()), f"no case runs {ENGINES[e]}"
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
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("#" + " " * 21 + "  " + " ".join(f"{t}" for _, t, _ in PLANS))
    for name, spec in CASES.items():
        print(f'    "{name}": "{dry_row(spec)}",')
