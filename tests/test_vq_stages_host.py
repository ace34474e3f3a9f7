"""The conv trunks of csrc/models.cpp (run_trunk_n, vq_decode_n, run_stack_n, run_stack_wino, pack_conv_layer) stage by stage: the float64
references, scales, networks, weight regimes and input regimes that tests/test_gpu_vq_stages.py runs on the GPU, and their own checks on
the CPU.  No GPU here.

References.  Every stage is the reference module's definition on the raw state dict, in float64 and channels-last (B, L, C), nothing folded:
ConvNormRelu = conv, BatchNorm1d(eval, eps 1e-5) (+ residual_layer(x) for down / up), LeakyReLU(0.2) (vqvae_modules.py:87-172);
Res_CNR_Stack = the layers, conv + BN, relu(h + x) (vqvae_modules.py:175-212); Conv1d k4 s2 p1, ConvTranspose1d k4 s2 p1 (written as the
scatter of its definition, not as two phases), k1 for pre_vq_conv / aft_vq_conv / project.  Neither pack_conv_layer's fold nor the fp32
oracle is used; the references are checked against float64 torch.nn modules and, chained, against oracle/talkshow_oracle.py.

Scales.  An element's error is measured in units of its own scale S, as tests/test_gpu_conv_ops.py does.  A direct layer:
S = |c| + sum (|w a| + |w_res|) |x| in float64, a = gamma / sqrt(var + eps), c = (b - mean) a + beta + b_res.  A stack of layers (only
its output is tapped) takes the running bound S_1 = |W_1| |x| + |c_1|, S_2 = |W_2| S_1 + |c_2|, ..., the tail adding |x| for the residual:
an error of e S_k in layer k's output moves layer k + 1's by at most e |W_{k+1}| S_k <= e S_{k+1} (LeakyReLU and ReLU do not expand), so the
errors of the layers add in these units.  A LOWERED stack (Winograd F(4,3)) takes the tile form of the same bound: T(v)[t] = the per-channel
maximum of v over the six input rows 4j - 1 .. 4j + 4 of row t's tile, S_1 = |W_1| T(|x|) + |c_1| (all three taps on the tile's maximum),
S_2 = |W_2| T(S_1) + |c_2|, ...: a tile's output rows are sums of products of the tile's other rows, so its rounding error is
relative to the tile, not to the row.

Ceilings (direct).  (Ktot + 4) 2^-24 of tests/test_gpu_conv_ops.py for the GEMM and its epilogue, plus the roundings of pack_conv_layer's
fold, FOLD_ROUNDINGS = 8, counted from its code: a = g / sqrt(var + 1e-5f) is three roundings and the fp32 constant a fourth (1e-5f is
1e-5 (1 - 2.6e-8): under half a rounding of var + eps, counted whole); the weight w a + w_res two more, each relative to |w a| + |w_res| at
most; the bias (b - mean) a + beta + b_res four of its own on top of a's, of which the weight's count covers all but two.  A stack's ceiling
is the sum of its layers' (the argument above).  The asserted bound is WHOLE_BOUND of tests/test_gpu_conv_ops.py, far below every ceiling
(test_bounds_under_every_ceiling), for single layers AND for stacks, whose running scale makes the same figure a stricter demand."""
import numpy as np
import pytest

from test_gpu_conv_ops import U, WHOLE_BOUND, ceiling

F32, F64 = np.float32, np.float64
EPS = 1e-5
FOLD_ROUNDINGS = 8
NRES = 2
# (state-dict name under the trunk's prefix, kind) of tap 0 .. 5 (include/talkshow_hip_debug.h, ts_debug_trunk_taps)
ENC_STAGES = (("project", "cnr"), ("_enc_1", "stack"), ("_down_1", "down"), ("_enc_2", "stack"), ("_down_2", "down"), ("_enc_3", "stack"))
DEC_STAGES = (("aft_vq_conv", "k1"), ("_dec_1", "stack"), ("_up_2", "up"), ("_dec_2", "stack"), ("_up_3", "up"), ("_dec_3", "stack"))
DEFECTS = ("eps_outside_sqrt", "residual_after_act", "phases_swapped", "w0_w3_swapped", "odd_last_tap_zero", "stack_residual_omitted",
           "slope_0.01", "fold_without_mean", "tile_shifted_one_row")


# ----------------------------------------------------------------------------------------------- float64 references, channels-last
def conv_same(x, w, b=None):
    """Conv1d(k, stride 1, padding k // 2), k = 1 or 3: x (B, L, Cin), w (Cout, Cin, k) -> (B, L, Cout)."""
    B, L, _ = x.shape
    K = w.shape[2]
    xp = np.zeros((B, L + K - 1, x.shape[2]), F64)
    xp[:, K // 2:K // 2 + L] = x
    y = sum(xp[:, k:k + L] @ w[:, :, k].T for k in range(K))
    return y if b is None else y + b


def conv_down(x, w, b=None, rows=None):
    """Conv1d(k 4, stride 2, padding 1): out[t] = sum_k W_k x[2t + k - 1], (L + 2 - 4) // 2 + 1 rows.  rows: the input rows the layer
    believes it has (a defect), the output count unchanged."""
    B, L, _ = x.shape
    Lout = (L - 2) // 2 + 1
    xp = np.zeros((B, L + 3, x.shape[2]), F64)
    xp[:, 1:1 + (L if rows is None else rows)] = x[:, :rows]
    y = sum(xp[:, k:k + 2 * Lout:2] @ w[:, :, k].T for k in range(4))
    return y if b is None else y + b


def conv_up(x, w, b=None):
    """ConvTranspose1d(k 4, stride 2, padding 1), w (Cin, Cout, 4): input row j adds x[j] W_k to row 2j + k of a buffer of 2L + 2 rows, whose
    first and last row are cut off: 2L rows."""
    B, L, _ = x.shape
    full = np.zeros((B, 2 * L + 2, w.shape[1]), F64)
    for k in range(4):
        full[:, k:k + 2 * L:2] += x @ w[:, :, k]
    y = full[:, 1:-1]
    return y if b is None else y + b


def batchnorm(v, sd, p, defect=None):
    g, be, mu, var = (sd[f"{p}.{k}"].astype(F64) for k in ("weight", "bias", "running_mean", "running_var"))
    den = np.sqrt(var) + EPS if defect == "eps_outside_sqrt" else np.sqrt(var + EPS)
    if defect == "fold_without_mean":
        mu = 0.0
    return (v - mu) / den * g + be


def leaky(v, defect=None):
    return np.where(v >= 0, v, (0.01 if defect == "slope_0.01" else 0.2) * v)


def conv_norm_relu(sd, p, x, sample="none", defect=None):
    w, b = sd[p + ".conv.weight"].astype(F64), sd[p + ".conv.bias"].astype(F64)
    residual = p + ".residual_layer.weight" in sd
    if residual:
        wr, br = sd[p + ".residual_layer.weight"].astype(F64), sd[p + ".residual_layer.bias"].astype(F64)
    if defect == "w0_w3_swapped" and sample != "none":
        w, wr = w[:, :, [3, 1, 2, 0]], wr[:, :, [3, 1, 2, 0]]
    rows = 2 * ((x.shape[1] - 2) // 2 + 1) if defect == "odd_last_tap_zero" else None
    conv = {"none": conv_same, "down": lambda *a: conv_down(*a, rows=rows), "up": conv_up}[sample]
    out = batchnorm(conv(x, w, b), sd, p + ".norm", defect)
    if residual and defect != "residual_after_act":
        out = out + conv(x, wr, br)
    out = leaky(out, defect)
    if residual and defect == "residual_after_act":
        out = out + conv(x, wr, br)
    if defect == "phases_swapped" and sample == "up":
        B, L2, Cc = out.shape
        out = out.reshape(B, L2 // 2, 2, Cc)[:, :, ::-1].reshape(B, L2, Cc)
    return out


def res_cnr_stack(sd, p, x, defect=None):
    h = x
    for i in range(NRES):
        h = conv_norm_relu(sd, f"{p}._layers.{i}", h, defect=defect)
    h = batchnorm(conv_same(h, sd[p + ".conv.weight"].astype(F64), sd[p + ".conv.bias"].astype(F64)), sd, p + ".norm", defect)
    y = np.maximum(h if defect == "stack_residual_omitted" else h + x, 0.0)
    if defect == "tile_shifted_one_row":                         # every row holds its successor's value
        y = np.concatenate([y[:, 1:], y[:, -1:]], 1)
    return y


def conv_k1(sd, p, x):
    return conv_same(x, sd[p + ".weight"].astype(F64), sd[p + ".bias"].astype(F64))


def stage_ref(sd, p, kind, x, defect=None):
    """The float64 output of stage `p` (a full state-dict prefix) on the float64 input x (B, L, Cin)."""
    x = np.asarray(x, F64)
    if kind == "stack":
        return res_cnr_stack(sd, p, x, defect)
    if kind == "k1":
        return conv_k1(sd, p, x)
    return conv_norm_relu(sd, p, x, {"cnr": "none", "down": "down", "up": "up"}[kind], defect)


# ----------------------------------------------------------------------------------------------- scales
def folded_abs(sd, p, transposed=False):
    """|w a| + |w_res| in the layer's own weight layout and |c| of one conv (+ BN (+ residual conv)) of the dict, float64."""
    q = p + ".conv" if p + ".conv.weight" in sd else p
    w, b = sd[q + ".weight"].astype(F64), sd[q + ".bias"].astype(F64)
    a, c = np.ones_like(b), b
    if p + ".norm.weight" in sd:
        g, be, mu, var = (sd[f"{p}.norm.{k}"].astype(F64) for k in ("weight", "bias", "running_mean", "running_var"))
        a = g / np.sqrt(var + EPS)
        c = (b - mu) * a + be
    A = a[None, :, None] if transposed else a[:, None, None]
    W = np.abs(w * A)
    if p + ".residual_layer.weight" in sd:
        W = W + np.abs(sd[p + ".residual_layer.weight"].astype(F64))
        c = c + sd[p + ".residual_layer.bias"].astype(F64)
    return W, np.abs(c)


def tile_max(v):
    """T(v): v (B, L, C) >= 0 -> per row t the per-channel maximum over rows 4j - 1 .. 4j + 4 (those inside the clip) of its tile j = t // 4."""
    B, L, Cc = v.shape
    J = (L + 3) // 4
    vp = np.zeros((B, 4 * J + 2, Cc), F64)
    vp[:, 1:1 + L] = v
    m = np.max(np.stack([vp[:, k:k + 4 * J:4] for k in range(6)]), 0)
    return np.repeat(m, 4, axis=1)[:, :L]


def stage_scale(sd, p, kind, x, tile=False):
    """S of stage p's output elements on input x (the docstring of this file); tile: the lowered form (stacks only)."""
    ax = np.abs(np.asarray(x, F64))
    if kind == "stack":
        s = ax
        for q in [f"{p}._layers.{i}" for i in range(NRES)] + [p]:
            W, c = folded_abs(sd, q)
            s = (tile_max(s) @ W.sum(2).T if tile else conv_same(s, W)) + c
        return s + ax
    W, c = folded_abs(sd, p, transposed=kind == "up")
    return {"cnr": conv_same, "k1": conv_same, "down": conv_down, "up": conv_up}[kind](ax, W) + c


def stage_ceiling(sd, p, kind):
    """The direct path's ceiling for stage p in units of stage_scale (the docstring of this file)."""
    def one(q, taps, norm):
        w = sd[q + ".conv.weight"] if q + ".conv.weight" in sd else sd[q + ".weight"]
        cin = w.shape[0] if kind == "up" else w.shape[1]
        return ceiling(taps * ((cin + 31) // 32 * 32)) + (FOLD_ROUNDINGS * U if norm else 0.0)
    if kind == "stack":
        return sum(one(q, 3, True) for q in [f"{p}._layers.{i}" for i in range(NRES)] + [p])
    return one(p, {"cnr": 3, "k1": 1, "down": 4, "up": 2}[kind], kind != "k1")       # up: two taps per output phase


# ----------------------------------------------------------------------------------------------- networks, weight regimes, input regimes
def network(name):
    """name -> (state dict, dict(kind, in_dim, ncode, hid, emb)); kind 'vq' / 'ae' / 'audio'."""
    from talkshow_amd import synth
    if name == "A256":
        return synth.audioencoder_state_dict(seed=11), dict(kind="audio", in_dim=64, ncode=0, hid=256, emb=0)
    if name == "AE256":
        return synth.ae_state_dict(seed=11, in_dim=129, num_hiddens=256), dict(kind="ae", in_dim=129, ncode=0, hid=256, emb=64)
    in_dim, ncode, hid, salt = {"V256/39": (39, 128, 256, 0), "V256/90": (90, 70, 256, 1), "V512/90": (90, 96, 512, 1),
                                "V1024/39": (39, 2048, 1024, 0)}[name]
    sd = synth.vqvae_state_dict(seed=11, in_dim=in_dim, num_embeddings=ncode, num_hiddens=hid, salt=salt)
    return sd, dict(kind="vq", in_dim=in_dim, ncode=ncode, hid=hid, emb=64)


REGIMES = ("synth", "bn_extreme", "residual_cancel")


def apply_regime(sd, regime):
    """A copy of the dict with its BatchNorm and residual tensors changed.  bn_extreme: per channel running_var cycles through {1e-6, 1e-3,
    1, 50}, gamma through {1, -1, 0, 3} (four channels each, so that every pair occurs), running_mean = +-5 (sixteen channels each).
    residual_cancel: residual_layer.weight = -a conv.weight (1 - 2^-10): the folded weight is the small difference of two large terms."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    if regime == "bn_extreme":
        for k in [k for k in sd if k.endswith(".running_var")]:
            p, ch = k[:-len(".running_var")], np.arange(sd[k].shape[0])
            sd[k] = np.array([1e-6, 1e-3, 1.0, 50.0], F32)[ch % 4]
            sd[p + ".weight"] = np.array([1.0, -1.0, 0.0, 3.0], F32)[(ch // 4) % 4]
            sd[p + ".running_mean"] = np.where((ch // 16) % 2 == 0, 5.0, -5.0).astype(F32)
    elif regime == "residual_cancel":
        for k in [k for k in sd if k.endswith(".residual_layer.weight")]:
            p = k[:-len(".residual_layer.weight")]
            a = sd[p + ".norm.weight"].astype(F64) / np.sqrt(sd[p + ".norm.running_var"].astype(F64) + EPS)
            w = sd[p + ".conv.weight"].astype(F64)
            A = a[None, :, None] if "_up_" in p else a[:, None, None]      # ConvTranspose1d weights are (cin, cout, k)
            sd[k] = (-A * w * (1.0 - 2.0 ** -10)).astype(F32)
    else:
        assert regime == "synth"
    return sd


INPUTS = ("unit", "onset", "spike", "offset")


def encoder_input(regime, seed, B, T, dim, scale):
    """unit: poses of the synthetic generator's scale; onset: a still clip that starts moving mid-tile (rows < 10 scaled 1e-3); spike: one
    frame times 100; offset: every frame moved by a constant 30 scales."""
    from talkshow_amd import synth
    x = (synth.gt_poses(seed, B, T, dim=dim, scale=scale)).astype(F32)
    if regime == "onset":
        x[:, :10] *= F32(1e-3)
    elif regime == "spike":
        x[:, min(T - 1, 13)] *= F32(100.0)
    elif regime == "offset":
        x += F32(30.0 * scale)
    else:
        assert regime == "unit"
    return x


def chain(sd, prefix, stages, x, defect=None):
    """Every stage's float64 output, each from the one before."""
    outs = []
    for name, kind in stages:
        x = stage_ref(sd, prefix + name, kind, x, defect)
        outs.append(x)
    return outs


# ----------------------------------------------------------------------------------------------- tests
def _t64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F64))


def test_references_against_torch_modules():
    """Every stage reference against float64 torch.nn modules (Conv1d, ConvTranspose1d, BatchNorm1d in eval mode) loaded from the same dict,
    on every weight regime and at odd lengths."""
    import torch
    from torch import nn

    def conv_mod(sd, p, kind):
        w = sd[p + ".weight"]
        if kind == "up":
            m = nn.ConvTranspose1d(w.shape[0], w.shape[1], 4, 2, 1)
        else:
            m = nn.Conv1d(w.shape[1], w.shape[0], w.shape[2], 2 if kind == "down" else 1, 1 if kind == "down" else w.shape[2] // 2)
        m = m.double()
        m.load_state_dict({"weight": _t64(sd[p + ".weight"]), "bias": _t64(sd[p + ".bias"])})
        return m.eval()

    def bn_mod(sd, p):
        m = nn.BatchNorm1d(sd[p + ".weight"].shape[0], eps=1e-5).double()
        m.load_state_dict({k: _t64(sd[f"{p}.{k}"]) for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
        return m.eval()

    def cnr_t(sd, p, kind, x):
        out = bn_mod(sd, p + ".norm")(conv_mod(sd, p + ".conv", kind)(x))
        if p + ".residual_layer.weight" in sd:
            out = out + conv_mod(sd, p + ".residual_layer", kind)(x)
        return nn.functional.leaky_relu(out, 0.2)

    def stage_t(sd, p, kind, x):
        if kind == "k1":
            return conv_mod(sd, p, "k1")(x)
        if kind != "stack":
            return cnr_t(sd, p, kind, x)
        h = x
        for i in range(NRES):
            h = cnr_t(sd, f"{p}._layers.{i}", "cnr", h)
        return torch.relu(bn_mod(sd, p + ".norm")(conv_mod(sd, p + ".conv", "cnr")(h)) + x)

    rng = np.random.default_rng(0)
    sd0, info = network("V256/39")
    for regime in REGIMES:
        sd = apply_regime(sd0, regime)
        for prefix, stages, cin in (("encoder.", ENC_STAGES, 39), ("decoder.", DEC_STAGES, 64)):
            for L in (5, 7, 12):
                x = rng.standard_normal((2, L, cin))
                for name, kind in stages:
                    with torch.no_grad():
                        want = stage_t(sd, prefix + name, kind, _t64(x.transpose(0, 2, 1))).numpy().transpose(0, 2, 1)
                    got = stage_ref(sd, prefix + name, kind, x)
                    assert got.shape == want.shape, (regime, name, L)
                    err = float((np.abs(got - want) / stage_scale(sd, prefix + name, kind, x)).max())
                    assert err <= 1e-13, (regime, name, L, err)
                    x = got / max(1.0, float(np.abs(got).max()))            # the next stage's input, kept at unit size


def test_chained_references_reproduce_the_oracle():
    """The stage references chained are the fp32 oracle's networks (oracle/talkshow_oracle.py) on the synthetic dict, to that oracle's own
    rounding: each stage within its direct ceiling, summed over the stages so far, in units of the stage's scale."""
    from oracle import talkshow_oracle as O
    sd, info = network("V256/39")
    x = encoder_input("unit", 3, 2, 31, 39, 0.3)
    xc = np.ascontiguousarray(x.transpose(0, 2, 1))
    outs = chain(sd, "encoder.", ENC_STAGES, x)
    z = conv_k1(sd, "encoder.pre_vq_conv", outs[-1])
    zo = O.vq_encoder(xc, sd).transpose(0, 2, 1)
    budget = sum(stage_ceiling(sd, "encoder." + n, k) for n, k in ENC_STAGES) + stage_ceiling(sd, "encoder.pre_vq_conv", "k1")
    e = float((np.abs(zo - z) / stage_scale(sd, "encoder.pre_vq_conv", "k1", outs[-1])).max())
    print(f"\n[oracle] z: {e:.3e} of the scale (budget {budget:.2e}), max |diff| {float(np.abs(zo - z).max()):.2e}")
    assert e <= budget and float(np.abs(zo - z).max()) <= 2e-5
    lat = np.random.default_rng(1).integers(0, info["ncode"], (2, 7))
    d = chain(sd, "decoder.", DEC_STAGES, sd["vq_layer.embeddings"][lat])
    y = conv_k1(sd, "decoder.project", d[-1])
    yo = O.vqvae_decode(lat, sd).transpose(0, 2, 1)
    print(f"[oracle] poses: max |diff| {float(np.abs(yo - y).max()):.2e}")
    assert float(np.abs(yo - y).max()) <= 1e-4
    sa, _ = network("A256")
    m = encoder_input("unit", 4, 1, 12, 64, 20.0)
    fo = O.audio_encoder(np.ascontiguousarray(m.transpose(0, 2, 1)), sa).transpose(0, 2, 1)
    assert float(np.abs(fo - chain(sa, "", ENC_STAGES, m)[-1]).max()) <= 2e-5


def lowered_bound():
    """The asserted bound of the lowered stacks (tests/test_gpu_vq_stages.py::LOWERED_BOUND), or None while nothing is measured."""
    from test_gpu_vq_stages import LOWERED_BOUND
    return LOWERED_BOUND


def defect_errors(defect):
    """How far `defect` moves each stage's float64 reference, per (regime, stage): in units of the direct scale and of the tile scale."""
    out = []
    sd0, _ = network("V256/39")
    for regime in REGIMES:
        sd = apply_regime(sd0, regime)
        for prefix, stages, x in (("encoder.", ENC_STAGES, encoder_input("unit", 5, 3, 31, 39, 0.3)),
                                  ("decoder.", DEC_STAGES, sd["vq_layer.embeddings"][np.random.default_rng(2).integers(0, 128, (3, 5))])):
            good = chain(sd, prefix, stages, x)
            for k, (name, kind) in enumerate(stages):
                xin = x if k == 0 else good[k - 1]
                bad = stage_ref(sd, prefix + name, kind, xin, defect)
                diff = np.abs(bad - good[k])
                own = float((diff / stage_scale(sd, prefix + name, kind, xin)).max())
                tile = float((diff / stage_scale(sd, prefix + name, kind, xin, tile=True)).max()) if kind == "stack" else 0.0
                out.append((regime, prefix + name, own, tile))
    return out


@pytest.mark.parametrize("defect", DEFECTS)
def test_bounds_catch_defects(defect):
    """Each defect, applied to the float64 reference of the stage it belongs to, moves some case of the GPU test (V256, the three weight
    regimes, an odd length) by at least 10x the bound that case is asserted under: WHOLE_BOUND in own-scale units for the direct plan and,
    where a bound of the lowered stacks is measured, that bound in tile-scale units for a lowered stack."""
    errs = defect_errors(defect)
    own = max(errs, key=lambda r: r[2])
    print(f"\n[defect] {defect}: direct {own[2]:.3e} = {own[2] / WHOLE_BOUND:.0f} x WHOLE_BOUND ({own[0]}, {own[1]})")
    if defect != "tile_shifted_one_row":
        assert own[2] >= 10 * WHOLE_BOUND, f"{defect} moves no stage by 10x the bound: {own[2]:.2e}"
    lb = lowered_bound()
    stack_defects = ("eps_outside_sqrt", "stack_residual_omitted", "slope_0.01", "fold_without_mean", "tile_shifted_one_row")
    if defect in stack_defects:
        tile = max(errs, key=lambda r: r[3])
        print(f"[defect] {defect}: lowered {tile[3]:.3e} ({tile[0]}, {tile[1]}), bound {lb}")
        if lb is not None:
            assert tile[3] >= 10 * lb, f"{defect} moves no lowered stack by 10x the bound: {tile[3]:.2e}"
        else:
            assert tile[3] > 0


def test_bounds_under_every_ceiling():
    for name in ("V256/39", "V256/90", "V512/90", "V1024/39", "AE256", "A256"):
        sd, info = network(name)
        enc, stages = ("" if info["kind"] == "audio" else "encoder."), []
        stages += [(enc + n, k) for n, k in ENC_STAGES]
        if info["kind"] != "audio":
            stages += [("decoder." + n, k) for n, k in DEC_STAGES] + [("encoder.pre_vq_conv", "k1"), ("decoder.project", "k1")]
        for p, kind in stages:
            assert WHOLE_BOUND <= stage_ceiling(sd, p, kind), (name, p)
