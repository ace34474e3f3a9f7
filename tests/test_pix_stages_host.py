"""The PixelCNN chain of csrc/pixelcnn.cpp stage by stage: the float64 references, scales, ceilings, networks and weight regimes that
tests/test_gpu_pix_stages.py runs on the GPU, and their own checks on the CPU.  No GPU here.

References.  Every stage is the reference module's own definition on the RAW state dict (GatedMaskedConv2d.forward, the two fusions and
output_conv, gated_pixelcnn_v2.py:61-87,130-150), in float64 and channels-last, with NOTHING folded: the fusions are not composed into
taps, horiz_resid is not composed into horiz_stack, mask 'A' is the zeroed kernel row / column of the full kernel.  Each stage is computed
from given inputs of THAT stage, so the GPU test feeds it the GPU's own taps of the stages before it (earlier rows included).  A value
travels with its scale as a pair (v, s): s = the sum of absolute values of the unfolded float64 expression, e.g. for a horizontal gate
|Wh1| (|Wr| |G| + |br| + |XH|) + |Wh0| |XH[0]| + |bh| + |V2H| + |cls|.  The row-shifted partial sums P_l, Q1, Q0 are the brackets the
header of pixelcnn.cpp defines, from the same raw weights.

Units.  As tests/test_gpu_chain_ops.py: the error of an element over its own scale S; for a gate GATE_ABS is taken off and the scale is
(S_v + S_p / 4).

Ceilings.  The chain-ops GEMM ceiling (K / W + W + 6) 2^-24 (W = 8 from K >= 256, else 4), plus the fold's roundings counted from
ts_pixelcnn_create:
  FOLD_ROUNDINGS = 1.  A composed matrix (Wh1 . Rw, W1 . Wr, Fh . Rw_0, Wt . blockdiag(Fv, Fv)) is a float64 product of fp32 matrices
  rounded ONCE to fp32: each entry moves by 2^-24 of its own magnitude, which is at most the matching entry of the product of the absolute
  matrices, i.e. 2^-24 of that term's share of S.  A composed bias (Wh1 . rb + bh, W1 . br + b1, Fh . br_0) is likewise one float64
  expression rounded once, 2^-24 of its share.  The shares are disjoint parts of S, so all of them together cost 1 x 2^-24 in units of S.
  (The float64 sums themselves err by K 2^-53: nothing.)
  AUDIO_ROUNDINGS(D) = 2 (D + 4) + 1.  The audio half of a fusion reaches the chain as a per-row term made by fp32 conv GEMMs of depth D
  from AE: AEV / AEH = F[:, D:] . AE + b, then AV1C / AV1P / AEH1 = (a weight sum or Wh1, rounded once: the + 1) . that.  Each GEMM is
  (Ktot + 4) 2^-24 of its own scale (tests/test_gpu_conv_ops.py::ceiling), the first one's error passes through the second's |W|, and
  both scales are shares of S.
Parts of one stage that different launches computed (P_l and the row's own tap, Q1 / Q0, T0) are disjoint shares of S: the stage's error
is at most the LARGEST part's ceiling times S, plus one rounding per joining addition (counted in the + 6).

Bounds.  Stages whose weights are used as loaded (HV_0, Q1, Q0, every OV, HV_l and P_l for l >= 2, V2H, G_0, T0, LG) are asserted under
LIN_BOUND / GATE_BOUND of tests/test_gpu_chain_ops.py.  Folded stages (HV_1, P_1, XH_1, G_l for l >= 1, Y) have FOLD_LIN_BOUND /
FOLD_GATE_BOUND: 2 x the largest record of the folded stages themselves on the MI355X (profiles/pix_stages_measured.jsonl, one family per
folded stage kind), quoted beside the constants.

XH_l for l >= 2 is used as loaded too (rw_l / rb_l are horiz_resid_{l-1} itself; only rw_1 / rb_1 compose fusion_h), but under
residual_cancel it is a DOMINATED sum: one product (-3 G_c) carries the element, so from that k on every step of the wave's chain rounds
a partial sum of the size of S itself, where the well-scaled sums LIN_BOUND was measured on round partial sums that random-walk far below
S.  In units of S the MI355X records 4.06e-7 = 6.8 x 2^-24 there (d128l3/residual_cancel/B3/forced, XH_2 of column 1 on row 5; d64l3
3.0e-7; synth 1.07e-7, fold_extreme 1.53e-7), over LIN_BOUND and well under the ceiling (K / W + W + 6) 2^-24 = 42 x 2^-24.  That excess
is the format's, not a defect's: an fp32 restatement of the kernels' documented order (Ref.resid_chain, fp32 = True: K cut into W slices,
one fmaf chain per slice with the MFMA's k order, the slices added in order, then tot + (bias + add1)) gives the GPU's XH_l bit for bit,
every element of every row, and tests/test_gpu_pix_stages.py asserts exactly that wherever K < 256.  The stage is therefore measured
against the scale its roundings are relative to, the partial-sum scale P = the sum of the absolute values of every intermediate result of
that chain in float64: each operation rounds its own result, so the error is at most 1 x 2^-24 P to first order, whatever dominates.
Asserted: 2^-24 P (a bound from the format alone; the records, family resid, carry the figure in units of S beside it).

Every bound sits under every case's ceiling (test_bounds_under_every_ceiling) and misses each defect of DEFECTS by 10 x on
the stage the defect lives in, which is also the first stage that fails (test_bounds_catch_defects)."""
import numpy as np
import pytest

from test_gpu_chain_ops import GATE_ABS, GATE_BOUND, LIN_BOUND, U

F32, F64 = np.float32, np.float64
FOLD_ROUNDINGS = 1
HID = 512
# 2 x the largest record of the folded stages' OWN records on the MI355X (profiles/pix_stages_measured.jsonl, families fold_HV1, fold_P1,
# fold_XH1, fold_Y, fold_gate; None = not measured, the ceiling stands in).  Folded linear stages: 1.17e-7 = 2.0 x 2^-24,
# d32l2/fold_extreme/B3/greedy, XH_1 of column 0 on row 6 (HV_1 8.0e-8, P_1 9.7e-8, Y 1.05e-7; the unfolded linear stages of the same run
# 1.26e-7 against LIN_BOUND 2.2e-7).  Folded gates: 2.57e-8 beyond GATE_ABS, d128l3/fold_extreme/B3/greedy, G_2 of column 1 on row 1 (the
# unfolded gates 3.27e-8 against GATE_BOUND 6.2e-8).
FOLD_LIN_BOUND = 2.34e-7
FOLD_GATE_BOUND = 5.2e-8
# (D, layers, V): what each exercises is in tests/test_gpu_pix_stages.py
NETWORKS = {"d32l1": (32, 1, 64), "d32l2": (32, 2, 64), "d64l3": (64, 3, 64), "d128l3": (128, 3, 64), "shipped": (256, 15, 2048)}
REGIMES = ("synth", "fold_extreme", "residual_cancel")
NC, AD = 4, 64
DEFECTS = ("h0_mask_B", "v0_sees_row_r", "residual_in_layer0", "rb_dropped", "fusion_bias_twice", "class_row_of_layer_below",
           "P_other_parity", "Q1_Q0_swapped", "T0_from_column_1", "T0_of_layer_below", "audio_row_above", "V2H_of_column_0",
           "head_without_XH")


def audio_roundings(D):
    return 2 * (D + 4) + 1


def gemm_ceiling(K):
    W = 8 if K >= 256 else 4
    return (K / W + W + 6) * U


def state_dict(name, regime="synth", seed=11):
    """The raw fp32 state dict of network `name` under a weight regime."""
    from talkshow_amd import synth
    D, NL, V = NETWORKS[name]
    sd = {k: np.array(v, F32) for k, v in synth.pixelcnn_state_dict(seed, V, D, NL, NC, AD).items()}
    rng = np.random.default_rng(seed + 1)
    if regime == "fold_extreme":          # four orders across channels, fusion biases that dominate: the composition's one rounding shows
        ramp = (10.0 ** rng.uniform(-2, 2, D)).astype(F32)
        for l in range(NL):
            sd[f"layers.{l}.horiz_resid.weight"] *= ramp[None, :, None, None] / np.sqrt(np.mean(ramp ** 2))
            sd[f"layers.{l}.horiz_resid.bias"] *= F32(8.0)
        for f in ("fusion_v", "fusion_h"):
            sd[f + ".weight"] *= np.concatenate([ramp, ramp[::-1]])[None, :, None, None] / np.sqrt(np.mean(ramp ** 2))
            sd[f + ".bias"] = (rng.standard_normal(D) * 3.0).astype(F32)
    elif regime == "residual_cancel":     # horiz_resid(G) ~ -XH: G in (-1, 1) cannot cancel XH exactly; a large negative-definite map comes closest
        for l in range(1, NL):
            w = sd[f"layers.{l}.horiz_resid.weight"]
            w[:, :, 0, 0] = w[:, :, 0, 0] * F32(0.05) - F32(3.0) * np.eye(D, dtype=F32)
            sd[f"layers.{l}.horiz_stack.weight"][:, :, 0, 1] += F32(0.5) * np.concatenate([np.eye(D), np.eye(D)]).astype(F32)
    elif regime != "synth":
        raise ValueError(regime)
    return sd


# ----------------------------------------------------------------------------------------------- (value, scale) arithmetic
def const(x):
    x = np.asarray(x, F64)
    return x, np.abs(x)


def lin(W, x):
    """x (.., K) pair through W (N, K) -> (.., N) pair."""
    return x[0] @ W.T, x[1] @ np.abs(W).T


def add(*xs):
    xs = [x for x in xs if x is not None]
    return sum(x[0] for x in xs), sum(x[1] for x in xs)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gate(pre, D):
    """GatedActivation over the last axis (.., 2D) -> (.., D): tanh(first half) * sigmoid(second half); scale S_v + S_p / 4."""
    v, s = pre
    return np.tanh(v[..., :D]) * sigmoid(v[..., D:]), s[..., :D] + s[..., D:] / 4


class Ref:
    """Float64 stage references of one network on its raw state dict.  Activations are channels-last: code rows E (B, 2, D) [column],
    vertical rows (B, 2, C), horizontal (B, C) per column.  `defect`: one of DEFECTS, altering the stage it names."""

    def __init__(self, sd, NL, defect=None):
        self.sd = {k: np.asarray(v, F64) for k, v in sd.items()}
        self.NL, self.defect = NL, defect
        self.V, self.D = self.sd["embedding.weight"].shape
        v = self.sd["layers.0.vert_stack.weight"].copy()       # make_causal, mask 'A': the zeroed kernel row and column of the full kernel
        h = self.sd["layers.0.horiz_stack.weight"].copy()
        if defect != "v0_sees_row_r":
            v[:, :, -1] = 0
        if defect != "h0_mask_B":
            h[:, :, :, -1] = 0
        self.sd["layers.0.vert_stack.weight"], self.sd["layers.0.horiz_stack.weight"] = v, h

    def w(self, l, name):
        return self.sd[f"layers.{l}.{name}"]

    def emb(self, codes):
        return self.sd["embedding.weight"][codes]

    def cls(self, l, label):
        if self.defect == "class_row_of_layer_below" and l >= 1:
            l -= 1
        return const(self.w(l, "class_cond_embedding.weight")[label])

    def audio(self, aud_row):
        """embedding_aud on one audio row (B, AD) -> AE (B, D)."""
        return lin(self.sd["embedding_aud.weight"][:, :, 0, 0], const(aud_row))[0] + self.sd["embedding_aud.bias"]

    # ---- vertical stack
    def vrow(self, Wt, x):
        """One kernel row Wt (2D, D, 3) on a row x (B, 2, D) pair, padding 1 over the two columns -> (B, 2, 2D) pair."""
        out = []
        for j in range(2):
            out.append(add(*[lin(Wt[:, :, c - j + 1], (x[0][:, c], x[1][:, c])) for c in range(2)]))
        return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1)

    def rider(self, t, E):
        """W_t . E of layer 0: t = 2 the newest row's share of HV_0, 1 = Q1 (read one row later), 0 = Q0 (two rows later)."""
        if self.defect == "Q1_Q0_swapped" and t < 2:
            t = 1 - t
        return self.vrow(self.w(0, "vert_stack.weight")[:, :, t], const(E))

    def hv0(self, E1, E2, E3, E0=None):
        """h_vert of layer 0 at row r from E[r-1], E[r-2], E[r-3] (None above the grid); E0 = E[r] is read only by a defect."""
        parts = [const(np.broadcast_to(self.w(0, "vert_stack.bias"), (E0.shape[0], 2, 2 * self.D)))]
        for t, E in ((2, E1), (1, E2), (0, E3)):
            if E is not None:
                parts.append(self.rider(t, E))
        parts.append(self.vrow(self.w(0, "vert_stack.weight")[:, :, 3], const(E0)))
        return add(*parts)

    def xv1(self, ov0, ae):
        """fusion_v on [OV0 | AE] per column: ov0 (B, 2, D) pair, ae (B, D)."""
        F, b = self.sd["fusion_v.weight"][:, :, 0, 0], self.sd["fusion_v.bias"]
        D = self.D
        a = lin(F[:, D:], const(ae))
        bias = const(np.broadcast_to(b * (2.0 if self.defect == "fusion_bias_twice" else 1.0), a[0].shape))
        ab = add(a, bias)
        return add(lin(F[:, :D], ov0), (ab[0][:, None], ab[1][:, None]))

    def p(self, l, xv):
        """The bracket of layer l >= 1 computed one row early: Wprev . XV_l[r] + b, read at row r + 1."""
        W = self.w(l, "vert_stack.weight")
        return add(self.vrow(W[:, :, 0], xv), const(np.broadcast_to(self.w(l, "vert_stack.bias"), xv[0].shape[:2] + (2 * self.D,))))

    def hv(self, l, xv_r, xv_above):
        """h_vert of layer l >= 1 at row r from its input rows r and r - 1 (None at the top row)."""
        W = self.w(l, "vert_stack.weight")
        cur = self.vrow(W[:, :, 1], xv_r)
        if xv_above is None:
            return add(cur, const(np.broadcast_to(self.w(l, "vert_stack.bias"), cur[0].shape)))
        return add(cur, self.p(l, xv_above))

    def ov(self, l, hv, label):
        c = self.cls(l, label)
        return gate(add(hv, (c[0][:, None], c[1][:, None])), self.D)

    def v2h(self, l, hv):
        return add(lin(self.w(l, "vert_to_horiz.weight")[:, :, 0, 0], hv), const(np.broadcast_to(self.w(l, "vert_to_horiz.bias"), hv[0].shape)))

    # ---- horizontal stack, column j
    def g0(self, j, v2h_j, E_row, label):
        """Layer 0's horizontal gate: mask 'A' sees the column to the left only.  v2h_j (B, 2D) pair, E_row (B, 2, D)."""
        Wh = self.w(0, "horiz_stack.weight")[:, :, 0]
        parts = [v2h_j, self.cls(0, label), const(np.broadcast_to(self.w(0, "horiz_stack.bias"), v2h_j[0].shape))]
        if j == 1:
            parts.append(lin(Wh[:, :, 0], const(E_row[:, 0])))
        parts.append(lin(Wh[:, :, 1], const(E_row[:, j])))         # the masked tap: zero weights unless a defect left them
        return gate(add(*parts), self.D)

    def xh_next(self, l, G, xh, ae=None, E_col=None, drop_xh=False):
        """The horizontal input of layer l + 1 from layer l's gate output G (B, D) pair: horiz_resid_l (+ XH_l for l >= 1), and behind
        layer 0 of a network with more layers fusion_h on [. | AE]."""
        parts = [lin(self.w(l, "horiz_resid.weight")[:, :, 0, 0], G)]
        if self.defect != "rb_dropped" or l == 0:
            parts.append(const(np.broadcast_to(self.w(l, "horiz_resid.bias"), G[0].shape)))
        if l >= 1 and not drop_xh:
            parts.append(xh)
        if l == 0 and self.defect == "residual_in_layer0":
            parts.append(const(E_col))
        out = add(*parts)
        if l == 0 and self.NL > 1:
            F, b = self.sd["fusion_h.weight"][:, :, 0, 0], self.sd["fusion_h.bias"]
            out = add(lin(F[:, :self.D], out), lin(F[:, self.D:], const(ae)), const(np.broadcast_to(b, G[0].shape)))
        return out

    def resid_chain(self, l, G, xh, fp32=False):
        """XH_{l+1} = horiz_resid_l . G + (b + XH_l), l >= 1, in the chain kernels' own order (csrc/kernels.h, skinny_gemm.hip): K is cut
        into W slices of whole 16-k steps (W = 8 from K >= 256, else 4), each slice is one fused-multiply-add chain from zero, within a
        16-k step in the order k = e + 4 g for e = 0 .. 3, g = 0 .. 3 (the lane groups of the 16 x 16 x 4 MFMA); the slices are added as
        ((s0 + s1) + s2) + .., then tot + (bias + add1).  fp32 = False: float64 throughout -> (value, P), P = the sum of the absolute
        values of every intermediate result, the scale the roundings of such a chain are relative to (each rounds its own result: the
        error is at most 2^-24 P to first order).  fp32 = True: every operation rounded to fp32 -> the kernel's value."""
        Wr = self.w(l, "horiz_resid.weight")[:, :, 0, 0]
        b = self.w(l, "horiz_resid.bias")
        T = F32 if fp32 else F64
        rnd = (lambda v: v.astype(F32)) if fp32 else (lambda v: v)
        A, X, Wr, b = np.asarray(G, F64), np.asarray(xh, F64), Wr.astype(T).astype(F64), b.astype(T).astype(F64)
        K = A.shape[1]
        W, Q = (8 if K >= 256 else 4), K // 16
        P = np.zeros((A.shape[0], Wr.shape[0]))
        tot = None
        for w in range(W):
            acc = np.zeros_like(P)
            for q in range(Q * w // W, Q * (w + 1) // W):
                for k in (16 * q + e + 4 * g for e in range(4) for g in range(4)):
                    acc = rnd(A[:, k:k + 1] * Wr[None, :, k] + acc).astype(F64)
                    P += np.abs(acc)
            if tot is None:
                tot = acc
            else:
                tot = rnd(tot + acc).astype(F64)
                P += np.abs(tot)
        e = rnd(b + X).astype(F64)
        out = rnd(tot + e).astype(F64)
        return (out.astype(F32) if fp32 else out), P + np.abs(e) + np.abs(out)

    def t0(self, l, xh0):
        return lin(self.w(l, "horiz_stack.weight")[:, :, 0, 0], xh0)

    def g(self, l, j, xh_j, xh_0, v2h_j, label):
        """Layer l >= 1's horizontal gate from its own input XH_l[j] (and XH_l[0] for column 1)."""
        Wh = self.w(l, "horiz_stack.weight")[:, :, 0]
        parts = [lin(Wh[:, :, 1], xh_j), v2h_j, self.cls(l, label), const(np.broadcast_to(self.w(l, "horiz_stack.bias"), v2h_j[0].shape))]
        if j == 1:
            parts.append(self.t0(l, xh_0))
        return gate(add(*parts), self.D)

    def y(self, xh_last):
        v, s = add(lin(self.sd["output_conv.0.weight"][:, :, 0, 0], xh_last), const(np.broadcast_to(self.sd["output_conv.0.bias"], xh_last[0].shape[:1] + (HID,))))
        return np.maximum(v, 0.0), s

    def lg(self, y):
        return add(lin(self.sd["output_conv.2.weight"][:, :, 0, 0], y), const(np.broadcast_to(self.sd["output_conv.2.bias"], y[0].shape[:1] + (self.V,))))


def run_row(ref, r, codes, label, aud, earlier, given=None, last_row=None):
    """Every stage of code row r, in the order the stages depend on each other, as {key: (value, scale)}.  A stage's inputs are the
    GPU's taps `given[row][key]` (arrays) where given, else the float64 values of this row computed so far and of `earlier[row]` (the
    dicts earlier calls returned).  Keys: ("HV", l) ("OV", l) ("P", l) ("Q1",) ("Q0",) ("V2H", l): (B, 2, .); ("G", l, j) ("XH", l, j)
    ("T0", l) ("Y", j) ("LG", j): (B, .).  aud (B, H, AD) raw audio rows, or, with `given`, given[row]["AE"] the device's AE rows.
    The defects that exchange slabs are applied here, where the slabs are chosen."""
    NL = ref.NL
    H = codes.shape[1] if last_row is None else last_row
    d = ref.defect
    out = {}

    def inp(row, key):
        if given is not None:
            return const(given[row][key])
        return const((out if row == r else earlier[row])[key][0])

    def ae(rr):
        return np.asarray(given[rr]["AE"], F64) if given is not None and "AE" in given[rr] else ref.audio(aud[:, rr])

    E = lambda rr: ref.emb(codes[:, rr]) if rr >= 0 else None
    ae_row = r - 1 if d == "audio_row_above" and r >= 1 else r
    out["HV", 0] = ref.hv0(E(r - 1), E(r - 2), E(r - 3), E(r))
    if r >= 1 and r + 1 < H:
        out["Q1", ] = ref.rider(1, E(r - 1))
    if r >= 1 and r + 2 < H:
        out["Q0", ] = ref.rider(0, E(r - 1))
    for l in range(NL):
        if l >= 1:
            ra = r - 2 if d == "P_other_parity" and r >= 2 else r - 1
            if l == 1:
                xv = ref.xv1(inp(r, ("OV", 0)), ae(ae_row))
                above = ref.xv1(inp(ra, ("OV", 0)), ae(ra)) if r >= 1 else None
            else:
                xv = inp(r, ("OV", l - 1))
                above = inp(ra, ("OV", l - 1)) if r >= 1 else None
            out["HV", l] = ref.hv(l, xv, above)
            if r + 1 < H:
                out["P", l] = ref.p(l, xv)
        out["OV", l] = ref.ov(l, inp(r, ("HV", l)), label)
        out["V2H", l] = ref.v2h(l, inp(r, ("HV", l)))
    for j in range(2):
        v2h = lambda l: tuple(x[:, 0 if d == "V2H_of_column_0" else j] for x in inp(r, ("V2H", l)))
        out["G", 0, j] = ref.g0(j, v2h(0), E(r), label)
        for l in range(1, NL):
            xh_prev = inp(r, ("XH", l - 1, j)) if l >= 2 else None
            out["XH", l, j] = ref.xh_next(l - 1, inp(r, ("G", l - 1, j)), xh_prev, ae(ae_row) if l == 1 else None, E(r)[:, j])
            if l >= 2:       # as loaded: measured against the partial-sum scale of the kernel's own chain (the third entry)
                out["XH", l, j] += (ref.resid_chain(l - 1, inp(r, ("G", l - 1, j))[0], xh_prev[0])[1],)
            if j == 0:
                out["T0", l] = ref.t0(l, inp(r, ("XH", l, 0)))
            x0 = None
            if j == 1:
                x0 = inp(r, ("XH", l, 1 if d == "T0_from_column_1" else 0))
                if d == "T0_of_layer_below" and l >= 2:
                    x0 = inp(r, ("XH", l - 1, 0))
            out["G", l, j] = ref.g(l, j, out["XH", l, j], x0, v2h(l), label)
        xh_prev = inp(r, ("XH", NL - 1, j)) if NL >= 2 else None
        out["Y", j] = ref.y(ref.xh_next(NL - 1, inp(r, ("G", NL - 1, j)), xh_prev, None, E(r)[:, j], drop_xh=d == "head_without_XH"))
        out["LG", j] = ref.lg(inp(r, ("Y", j)))
    return out


def chain(ref, codes, label, aud):
    """All rows in float64, every stage from the float64 values of the stages before it -> [row] {key: (value, scale)}."""
    rows = []
    for r in range(codes.shape[1]):
        rows.append(run_row(ref, r, codes, label, aud, rows))
    return rows


# ----------------------------------------------------------------------------------------------- units, ceilings, bounds
def stage_info(key, D, NL):
    """(gate?, folded?, reads an audio term?, K of the largest GEMM part) of a stage."""
    s, l = key[0], (key[1] if len(key) > 1 else 0)
    if s == "OV":
        return True, False, False, 0
    if s in ("HV", "P"):
        return False, l == 1, l == 1, 2 * D
    if s in ("Q1", "Q0", "V2H"):
        return False, False, False, 2 * D
    if s == "G":
        return True, l >= 1, l == 1, D if l <= 1 else 2 * D
    if s == "XH":                       # rw_1 / rb_1 compose fusion_h; rw_l / rb_l for l >= 2 are horiz_resid_{l-1} as loaded
        return False, l == 1, l == 1, D
    if s == "T0":
        return False, False, False, D
    if s == "Y":
        return False, True, False, 2 * D if NL >= 2 else D
    if s == "LG":
        return False, False, False, HID
    raise KeyError(key)


def ceiling(key, D, NL):
    gate_, folded, audio, K = stage_info(key, D, NL)
    if key[0] == "XH" and not folded:
        return U                        # in units of the partial-sum scale every rounding is counted where it happens: 1 x 2^-24
    return gemm_ceiling(K) + (FOLD_ROUNDINGS + (audio_roundings(D) if audio else 0)) * U * folded


def bound(key, D, NL):
    """The asserted bound of a stage; a folded family without a measured constant yet is held to its ceiling."""
    gate_, folded, audio, K = stage_info(key, D, NL)
    if not folded:
        return GATE_BOUND if gate_ else (U if key[0] == "XH" else LIN_BOUND)
    b = FOLD_GATE_BOUND if gate_ else FOLD_LIN_BOUND
    return ceiling(key, D, NL) if b is None else b


def family(key, D, NL):
    """The family a stage's record goes under: the unfolded stages together (XH_l for l >= 2 on its own line, resid), every folded
    stage kind by itself, so that the folded bounds come from folded stages' own records."""
    gate_, folded, audio, K = stage_info(key, D, NL)
    if not folded:
        return "gate" if gate_ else ("resid" if key[0] == "XH" else "lin")
    return "fold_gate" if gate_ else "fold_" + key[0] + ("1" if key[0] != "Y" else "")


def units(key, got, ref_pair, D, NL):
    """The largest error of `got` against (value, scale) in units of the element's own scale."""
    v, s = ref_pair[0], ref_pair[-1]    # (value, S) or, for XH_l with l >= 2, (value, S, P): measured against P
    e = np.abs(np.asarray(got, F64) - v)
    if stage_info(key, D, NL)[0]:
        e = np.maximum(e - GATE_ABS, 0.0)
    assert np.all((s > 0) | (e == 0)), f"{key}: a nonzero error on an element of zero scale"
    return float(np.max(np.where(s > 0, e / np.where(s > 0, s, 1.0), 0.0)))


def clip_inputs(name, B, H, seed=5):
    D, NL, V = NETWORKS[name]
    rng = np.random.default_rng(seed)
    return (rng.integers(0, V, (B, H, 2)), rng.integers(0, NC, B), rng.standard_normal((B, H, AD)).astype(F32))


# ----------------------------------------------------------------------------------------------- CPU checks
@pytest.mark.parametrize("name,regime", [("d32l1", "synth"), ("d32l2", "synth"), ("d64l3", "synth"), ("d64l3", "fold_extreme"),
                                         ("d64l3", "residual_cancel"), ("d128l3", "synth")])
def test_chained_references_reproduce_the_oracle(name, regime, monkeypatch):
    """The stage references, chained in float64, give oracle.pixelcnn_forward's logits (the oracle's own arithmetic switched to float64)."""
    from oracle import talkshow_oracle as O
    monkeypatch.setattr(O, "F32", F64)
    D, NL, V = NETWORKS[name]
    sd = state_dict(name, regime)
    codes, label, aud = clip_inputs(name, 2, 5)
    rows = chain(Ref(sd, NL), codes, label, aud)
    got = np.stack([np.stack([rows[r]["LG", j][0] for j in range(2)], 1) for r in range(5)], 1)       # (B, H, 2, V)
    sd64 = O.causal_weights({k: v.astype(F64) for k, v in sd.items()}, NL)
    amap = np.repeat(aud.astype(F64).transpose(0, 2, 1)[..., None], 2, 3)                             # (B, AD, H, 2)
    want = O.pixelcnn_forward(codes, label, amap, sd64, NL).transpose(0, 2, 3, 1)
    assert want.dtype == F64
    scale = np.stack([np.stack([rows[r]["LG", j][1] for j in range(2)], 1) for r in range(5)], 1)
    assert np.max(np.abs(got - want) / scale) < 1e-12


def test_partial_sums_are_the_brackets():
    """P_l, Q1 and Q0 of a row are what the rows after it add: HV_l(r + 1) = Wcur . XV_l[r + 1] + P_l(r), and HV_0 splits into its riders."""
    name = "d64l3"
    D, NL, V = NETWORKS[name]
    ref = Ref(state_dict(name), NL)
    codes, label, aud = clip_inputs(name, 2, 6)
    rows = chain(ref, codes, label, aud)
    for r in range(1, 5):
        for l in range(2, NL):
            cur = ref.vrow(ref.w(l, "vert_stack.weight")[:, :, 1], const(rows[r + 1]["OV", l - 1][0]))[0]
            np.testing.assert_allclose(rows[r + 1]["HV", l][0], cur + rows[r]["P", l][0], rtol=0, atol=1e-12)
    r = 3
    E = ref.emb(codes[:, r])
    top = ref.vrow(ref.w(0, "vert_stack.weight")[:, :, 2], const(E))[0] + ref.w(0, "vert_stack.bias")
    np.testing.assert_allclose(rows[r + 1]["HV", 0][0], top + rows[r]["Q1", ][0] + rows[r - 1]["Q0", ][0], rtol=0, atol=1e-12)


def all_keys(NL, r, H):
    ks = [("HV", l) for l in range(NL)] + [("OV", l) for l in range(NL)] + [("V2H", l) for l in range(NL)]
    if r + 1 < H:
        ks += [("P", l) for l in range(1, NL)]
    if r >= 1 and r + 1 < H:
        ks.append(("Q1",))
    if r >= 1 and r + 2 < H:
        ks.append(("Q0",))
    ks += [("T0", l) for l in range(1, NL)]
    for j in range(2):
        ks += [("G", l, j) for l in range(NL)] + [("XH", l, j) for l in range(1, NL)] + [("Y", j), ("LG", j)]
    return ks


def test_bounds_under_every_ceiling():
    for name, (D, NL, V) in NETWORKS.items():
        for key in all_keys(NL, 3, 10):
            assert bound(key, D, NL) <= ceiling(key, D, NL), (name, key, bound(key, D, NL), ceiling(key, D, NL))
            assert ceiling(key, D, NL) < 1e-4


# the stage each defect lives in = the first that must fail, in run_row's order, on row 5 of the three-layer network
EXPECT = {"h0_mask_B": ("G", 0, 0), "v0_sees_row_r": ("HV", 0), "residual_in_layer0": ("XH", 1, 0), "rb_dropped": ("XH", 2, 0),
          "fusion_bias_twice": ("HV", 1), "class_row_of_layer_below": ("OV", 1), "P_other_parity": ("HV", 1), "Q1_Q0_swapped": ("HV", 0),
          "T0_from_column_1": ("G", 1, 1), "T0_of_layer_below": ("G", 2, 1), "audio_row_above": ("HV", 1), "V2H_of_column_0": ("G", 0, 1),
          "head_without_XH": ("Y", 0)}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("defect", DEFECTS)
def test_bounds_catch_defects(defect, regime):
    """Each defect, applied to the float64 reference, misses every asserted bound by at least 10 x on the stage it lives in, and that stage
    is the first to fail.  Every stage is computed from the GOOD values of the stages before it, as the GPU test computes it from taps."""
    name, r, H = "d64l3", 5, 10
    D, NL, V = NETWORKS[name]
    sd = state_dict(name, regime)
    codes, label, aud = clip_inputs(name, 3, H)
    good = chain(Ref(sd, NL), codes, label, aud)
    taps = [{k: v[0] for k, v in row.items()} for row in good]
    bad = run_row(Ref(sd, NL, defect), r, codes, label, aud, None, given=taps)
    biggest = max(LIN_BOUND, GATE_BOUND, *(bound(k, D, NL) for k in bad))
    failed = [k for k in bad if units(k, bad[k][0], good[r][k], D, NL) > bound(k, D, NL)]
    assert failed and failed[0] == EXPECT[defect], (defect, failed[:3])
    assert units(EXPECT[defect], bad[EXPECT[defect]][0], good[r][EXPECT[defect]], D, NL) >= 10 * biggest
    clean = run_row(Ref(sd, NL), r, codes, label, aud, None, given=taps)
    assert max(units(k, clean[k][0], good[r][k], D, NL) for k in clean) < 1e-12


