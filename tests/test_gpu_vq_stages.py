"""The conv trunks of csrc/models.cpp on the GPU, stage by stage against float64: the encoder and decoder of the VQ-VAEs, the auto-encoder
flavour and the audio encoder, through the PRODUCT entries with the stage taps of ts_debug_trunk_taps (include/talkshow_hip_debug.h), which
make the production pass copy every stage's output out of its arena.

The reference of stage k is computed from the GPU's own tap of stage k - 1 (tests/test_vq_stages_host.py: float64, the reference module's
definition on the raw state dict, nothing folded), so nothing compounds: a stage that is wrong is named.  z and the decoder's project are
checked from tap 5 the same way, the code indices as tests/test_gpu_parity.py::test_op_vq_argmin (b) does: the argmin of the distances
recomputed in the kernel's order from the GPU's z, no exceptions.

Units and bounds (the docstring of tests/test_vq_stages_host.py).  Direct stages: own-scale units, asserted under WHOLE_BOUND of
tests/test_gpu_conv_ops.py, DIRECT_OVER naming any fold regime that exceeds it (with its record, under its ceiling).  Lowered stacks
(Winograd F(4,3): by default the 512- and 1024-wide ones, under TS_CONV_WINO=1 every one, in a child process): tile-scale units.  There is
no derived constant for them: LOWERED_BOUND is 2x the largest figure the first MI355X run of this file recorded over all cases (through
TS_MEASURED_LOG into profiles/vq_stages_measured.jsonl), None = not measured (the stages are recorded, not asserted); the stacks are held
to 2x their own records per weight regime besides (LOWERED_STACK_BOUND), two orders of magnitude below it.  Beside each lowered
record stand the same stage's error in own-scale units and, from the parent process, the direct plan's error on the same case (reported, not
asserted).  Under each weight regime no input regime may exceed 4x the unit input's record: the tile scale would not describe the kernel.
(Across WEIGHT regimes the figures are not comparable, in either plan: the running scale takes |W| where the values add up like a random
walk, so its slack depends on the weights.  The first run recorded 1.2e-9 under synth and 5.9e-8 under bn_extreme for the lowered stacks,
and 3.8e-9 against the very same 5.9e-8 for the direct ones: bn_extreme's record is the rounding of pack_conv_layer's c = (b - mean) a +
beta on a channel that c dominates, the same number in both plans.  Each record carries its ratio to (synth, unit) for the reader.)

Weight regimes (V256, both plans): synth, bn_extreme, residual_cancel.  Shapes: B in {1, 3}, T in {4, 5, 6, 7, 31, 78} (H = 1, every T mod
4, an odd length into each stride-2 layer, B ceil(L / 4) never a multiple of a GEMM tile), decoder H in {1, 2, 3, 5, 19} with random, constant
and alternating codes; input regimes unit / onset / spike / offset."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_vq_stages_host as H
from test_gpu_conv_ops import WHOLE_BOUND

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = 0x7FE5A5A5                       # a quiet NaN with a payload no arithmetic produces
# 2x the largest error of the lowering, in tile-scale units, that the first MI355X run of this file and of
# tests/test_gpu_wino.py::test_lowered_layer_regimes recorded over every case (profiles/vq_stages_measured.jsonl): 3.540e-7, the record
# wino.layer_regimes.C512.L24.unit (one layer, C = 512, unit inputs).  The stacks stay far below it, their running scale being looser than a
# single layer's: 5.93e-8 at most (vq_stages.V256/39.bn_extreme.dec.B3.H1.random.decoder._dec_1.lowered; the direct plan records the same
# figure to the last digit on that case: it is the fold's rounding of c, not the lowering), 1.6e-9 under synth and residual_cancel.
# None = not measured: recorded, not asserted.
LOWERED_BOUND = 7.1e-7
# The stacks on top of it, per weight regime (a stack's running scale has the regime's slack, see the docstring): 2x the largest record of
# a lowered stack over every network and shape of that run — synth 1.184e-9 (vq_stages.V256/39.wino_all.lowered_regime.synth.unit; the
# 512- and 1024-wide stacks of the default plan stay at 1.6e-10), bn_extreme 5.929e-8, residual_cancel 1.620e-9 (their .unit records).
# Without this a lowered stack could lose two orders of magnitude unnoticed under the one-layer figure above.
LOWERED_STACK_BOUND = {"synth": 2.4e-9, "bn_extreme": 1.2e-7, "residual_cancel": 3.3e-9}
LOWERED_REGIME_RATIO = 4.0                  # no input regime's record over this many times the unit input's of the same weight regime
# (network, weight regime, stage) -> bound, for a direct stage of a fold regime that exceeded WHOLE_BOUND on the first run, with its record;
# each under the stage's ceiling (asserted)
DIRECT_OVER = {}
KNOB = ("TS_CONV_WINO=" + os.environ["TS_CONV_WINO"]) if os.environ.get("TS_CONV_WINO") else None
PLAN = "wino_all" if KNOB == "TS_CONV_WINO=1" else "default"
T_LIST, B_LIST, H_LIST = (4, 5, 6, 7, 31, 78), (1, 3), (1, 2, 3, 5, 19)


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load(), _lib.context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def record(name, **kv):
    print(f"\n[measured] {name}: " + ", ".join(f"{k} = {v:.3e}" if isinstance(v, float) else f"{k} = {v}" for k, v in kv.items()))
    log = os.environ.get("TS_MEASURED_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(name=name, plan=PLAN, **kv)) + "\n")


def in_units(diff, S):
    """max of diff / S; an element of scale 0 must be exact."""
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(S > 0, diff / S, np.where(diff > 0, np.inf, 0.0))
    return float(e.max())


# ----------------------------------------------------------------------------------------------- networks and tapped passes
class Net:
    def __init__(self, hip, name, regime="synth"):
        from talkshow_amd import modules, synth
        self._lib, self.lib, self.ctx = hip
        self.name, self.regime = name, regime
        sd0, self.info = H.network(name)
        self.sd = H.apply_regime(sd0, regime)
        i = self.info
        self.kind, self.hid, self.in_dim, self.ncode = i["kind"], i["hid"], i["in_dim"], i["ncode"]
        if self.kind == "audio":
            self.m = modules.AudioEncoder(64, self.hid, 2)
        elif self.kind == "ae":
            self.m = modules.AE(self.in_dim, 64, 0, self.hid, 2)
        else:
            self.m = modules.VQVAE(self.in_dim, 64, self.ncode, self.hid, 2)
        self.m.cuda().load_state_dict(synth.to_torch(self.sd))
        self.enc_prefix = "" if self.kind == "audio" else "encoder."
        self.in_scale = 20.0 if self.kind == "audio" else 0.3

    def lowered(self, c):
        out = (C.c_int * 5)()
        return self.lib.ts_debug_wino_lowering(c, c, 3, 1, KNOB.encode() if KNOB else None, 1, 4, out) == 1

    def enc_shapes(self, B, T):
        h = self.hid
        return [(B, T, h // 4), (B, T, h // 4), (B, T // 2, h // 2), (B, T // 2, h // 2), (B, T // 2 // 2, h), (B, T // 2 // 2, h)]

    def dec_shapes(self, B, Hh):
        h = self.hid
        return [(B, Hh, h), (B, Hh, h), (B, 2 * Hh, h // 2), (B, 2 * Hh, h // 2), (B, 4 * Hh, h // 4), (B, 4 * Hh, h // 4)]


def tap_buffers(shapes):
    return [torch.from_numpy(np.full(s, SENTINEL, np.uint32).view(F32)).cuda() for s in shapes]


def set_taps(hip, enc=(), dec=()):
    """enc / dec: per network a list of six device tensors (or None)."""
    _lib, lib, ctx = hip
    t = _lib.TrunkTaps()
    for i, bufs in enumerate(enc):
        for k, b in enumerate(bufs or ()):
            t.enc[i][k] = b.data_ptr() if b is not None else None
    for i, bufs in enumerate(dec):
        for k, b in enumerate(bufs or ()):
            t.dec[i][k] = b.data_ptr() if b is not None else None
    _lib.check(lib.ts_debug_trunk_taps(C.byref(t)))


def host(bufs, what):
    out = [b.cpu().numpy() for b in bufs]
    for k, a in enumerate(out):
        assert not np.any(bits(a) == SENTINEL), f"{what}: tap {k} was not written everywhere"
    return out


def encode(hip, net, x, tap=True):
    """x (B, T, in_dim) host -> (taps [6] host or None, z or feat host, codes host or None) through the product entry."""
    _lib, lib, ctx = hip
    B, T, _ = x.shape
    xd = dev(x)
    Hh = T // 2 // 2
    bufs = tap_buffers(net.enc_shapes(B, T)) if tap else None
    if tap:
        set_taps(hip, enc=[bufs])
    lat = None
    if net.kind == "audio":
        z = torch.empty((B, Hh, net.hid), dtype=torch.float32, device="cuda")
        _lib.check(lib.ts_audioenc_forward(net.m.handle(), _lib.dptr(xd), B, T, _lib.dptr(z), _lib.stream_ptr()))
    else:
        z = torch.empty((B, Hh, 64), dtype=torch.float32, device="cuda")
        lat = torch.empty((B, Hh), dtype=torch.int64, device="cuda") if net.ncode else None
        _lib.check(lib.ts_vqvae_encode(net.m.handle(), _lib.dptr(xd), B, T, _lib.dptr(z), _lib.dptr(lat), None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return (host(bufs, "encode") if tap else None), z.cpu().numpy(), (lat.cpu().numpy() if lat is not None else None)


def decode(hip, net, lat=None, z=None, tap=True):
    """codes (B, H) or continuous latents z (B, H, 64) host -> (taps, poses (B, 4H, in_dim)) through the product entry."""
    _lib, lib, ctx = hip
    B, Hh = (lat if lat is not None else z).shape[:2]
    bufs = tap_buffers(net.dec_shapes(B, Hh)) if tap else None
    out = torch.from_numpy(np.full((B, 4 * Hh, net.in_dim), SENTINEL, np.uint32).view(F32)).cuda()
    if tap:
        set_taps(hip, dec=[bufs])
    if lat is not None:
        ld = dev(lat.astype(np.int64))
        _lib.check(lib.ts_vqvae_decode(net.m.handle(), _lib.dptr(ld), B, Hh, _lib.dptr(out), net.in_dim, 0, _lib.stream_ptr()))
    else:
        zd = dev(z.astype(F32))
        _lib.check(lib.ts_vqvae_decode_z(net.m.handle(), _lib.dptr(zd), B, Hh, _lib.dptr(out), net.in_dim, 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return (host(bufs, "decode") if tap else None), host([out], "decode out")[0]


# ----------------------------------------------------------------------------------------------- the comparison
class Tally:
    """The largest lowered error per (weight regime, input regime), in tile units."""

    def __init__(self):
        self.worst = {}

    def add(self, key, e):
        self.worst[key] = max(self.worst.get(key, 0.0), e)

    def check(self, what):
        for key, e in self.worst.items():
            base = self.worst[(key[0], "unit")]
            record(f"vq_stages.{what}.lowered_regime.{key[0]}.{key[1]}", tile_units=e, over_unit=e / base,
                   over_synth_unit=e / self.worst.get(("synth", "unit"), float("nan")))
            assert e <= LOWERED_REGIME_RATIO * base, f"{what} {key}: {e:.3e} is {e / base:.1f} x the unit input's record {base:.3e}"


def check_stages(net, label, prefix, stages, x_in, taps, tally=None, key=None):
    """Every tap against the float64 reference computed from the tap before it (tap 0: from x_in, float64)."""
    for k, (name, kind) in enumerate(stages):
        p = prefix + name
        xin = np.asarray(x_in, F64) if k == 0 else taps[k - 1].astype(F64)
        got = taps[k]
        assert np.isfinite(got).all(), f"{label} {p}: a non-finite element"
        ref = H.stage_ref(net.sd, p, kind, xin)
        assert ref.shape == got.shape, (label, p, ref.shape, got.shape)
        diff = np.abs(got.astype(F64) - ref)
        own = in_units(diff, H.stage_scale(net.sd, p, kind, xin))
        if kind == "stack" and net.lowered(got.shape[-1]):
            tile = in_units(diff, H.stage_scale(net.sd, p, kind, xin, tile=True))
            record(f"vq_stages.{label}.{p}.lowered", tile_units=tile, own_units=own, bound=LOWERED_BOUND)
            if tally is not None:
                tally.add(key, tile)
            if LOWERED_BOUND is not None:
                bound = min(LOWERED_BOUND, LOWERED_STACK_BOUND[net.regime])
                assert tile <= bound, f"{label} {p}: {tile:.3e} of the tile scale > {bound:.1e}"
        else:
            bound = DIRECT_OVER.get((net.name, net.regime, name), WHOLE_BOUND)
            ceil = H.stage_ceiling(net.sd, p, kind)
            record(f"vq_stages.{label}.{p}.direct", own_units=own, bound=bound, ceiling=ceil)
            assert bound <= ceil
            assert own <= bound, f"{label} {p}: {own:.3e} of its scale > {bound:.1e}"


def check_k1(net, label, p, x_tap, got):
    xin = x_tap.astype(F64)
    ref = H.conv_k1(net.sd, p, xin)
    own = in_units(np.abs(got.astype(F64) - ref), H.stage_scale(net.sd, p, "k1", xin))
    record(f"vq_stages.{label}.{p}.direct", own_units=own, bound=WHOLE_BOUND, ceiling=H.stage_ceiling(net.sd, p, "k1"))
    assert own <= WHOLE_BOUND, f"{label} {p}: {own:.3e} of its scale > {WHOLE_BOUND:.1e}"


def fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def check_codes(net, label, z, lat):
    """The indices are the argmin of the distances recomputed in the kernel's order from the GPU's z (test_op_vq_argmin (b)); rows whose
    squared norm overflows fp32 (bn_extreme drives z to 1e30) have no finite distance to order and are left out."""
    cb = net.sd["vq_layer.embeddings"].astype(F32)
    x = z.reshape(-1, z.shape[-1])
    xsq, csq = np.zeros(x.shape[0], F32), np.zeros(cb.shape[0], F32)
    dot = np.zeros((x.shape[0], cb.shape[0]), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(x.shape[1]):
            xsq, csq = fma32(x[:, c], x[:, c], xsq), fma32(cb[:, c], cb[:, c], csq)
            dot = fma32(x[:, c:c + 1], cb[None, :, c], dot)
        d = (xsq[:, None] + csq[None, :]) - F32(2.0) * dot
    ok = np.isfinite(d).all(1)
    assert net.regime == "bn_extreme" or ok.all(), label
    np.testing.assert_array_equal(lat.reshape(-1)[ok], d.argmin(1)[ok], err_msg=label)


def run_network(hip, name, regimes, full):
    """The shapes of the docstring on `name` under each weight regime.  full: all T x B and H x B x codes under synth; else, and under the
    other weight regimes, the shapes that take each path once (every T mod 4 and odd length still enters, at one batch size each)."""
    tally = Tally()
    for regime in regimes:
        net = Net(hip, name, regime)
        rng = np.random.default_rng(7)
        full = full and regime == "synth"
        shapes = [(B, T, "unit") for T in T_LIST for B in B_LIST] if full else [(3, 4, "unit"), (3, 5, "unit"), (1, 6, "unit"), (1, 7, "unit"), (3, 31, "unit")]
        shapes += [(3, T, r) for T in ((31, 78) if full else (31,)) for r in H.INPUTS[1:]]
        for B, T, inp in shapes:
            x = H.encoder_input(inp, 100 + T, B, T, net.in_dim, net.in_scale)
            label = f"{name}.{regime}.enc.B{B}.T{T}.{inp}"
            taps, z, lat = encode(hip, net, x)
            check_stages(net, label, net.enc_prefix, H.ENC_STAGES, x, taps, tally, (regime, inp))
            if net.kind == "audio":
                assert np.array_equal(bits(z), bits(taps[5])), label
                continue
            check_k1(net, label, "encoder.pre_vq_conv", taps[5], z)
            if net.ncode:
                check_codes(net, label, z, lat)
        if net.kind == "audio":
            continue
        cases = ([(B, Hh, "random") for Hh in H_LIST for B in B_LIST] + [(3, Hh, c) for Hh in (3, 19) for c in ("equal", "alternating")]) if full \
            else [(3, 1, "random"), (1, 5, "random"), (3, 19, "random"), (3, 5, "equal"), (3, 5, "alternating")]
        for B, Hh, how in cases:
            label = f"{name}.{regime}.dec.B{B}.H{Hh}.{how}"
            if net.ncode:
                lat = rng.integers(0, net.ncode, (B, Hh))
                if how == "equal":
                    lat[:] = 5
                elif how == "alternating":
                    lat[:] = np.where(np.arange(Hh) % 2 == 0, 3, net.ncode - 1)[None]
                taps, out = decode(hip, net, lat=lat)
                x0 = net.sd["vq_layer.embeddings"][lat]
            else:
                x0 = rng.standard_normal((B, Hh, 64)).astype(F32)
                if how == "equal":
                    x0[:] = x0[:1, :1]
                elif how == "alternating":
                    x0[:] = np.where((np.arange(Hh) % 2 == 0)[None, :, None], x0[:1, :1], -x0[:1, :1])
                taps, out = decode(hip, net, z=x0)
            check_stages(net, label, "decoder.", H.DEC_STAGES, x0, taps, tally, (regime, "unit"))
            check_k1(net, label, "decoder.project", taps[5], out)
    tally.check(f"{name}.{PLAN}")


# ----------------------------------------------------------------------------------------------- 1. stage by stage
@pytest.mark.parametrize("name", ["V256/39", "V256/90"])
def test_stages_v256(hip, name):
    """The narrow VQ-VAEs, every shape; V256/39 under the three weight regimes.  All direct by default; all lowered in the child below."""
    run_network(hip, name, H.REGIMES if name == "V256/39" else ("synth",), full=True)


def test_stages_v256_lowered_at_every_width(hip):
    """TS_CONV_WINO=1 lowers the 64-, 128- and 256-wide stacks; the knob is read once per process, so test_stages_v256 runs again in a
    child process (the pattern of tests/test_gpu_wino.py)."""
    env = dict(os.environ, TS_CONV_WINO="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k", "test_stages_v256 and not lowered"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout
    assert ".lowered" in r.stdout and PLAN == "default"


@pytest.mark.parametrize("name", ["V512/90", "AE256", "A256", "V1024/39"])
def test_stages_other_networks(hip, name):
    """V512/90 under the defaults (_enc_3 and _dec_1 lowered, the decoder from its code tables), the auto-encoder flavour (stage 0 of the
    decoder is aft_vq_conv on continuous latents), the audio encoder, and the shipped body network 39 / 64 / 2048 / 1024 at B = 1, T = 12."""
    if name != "V1024/39":
        return run_network(hip, name, ("synth",), full=name == "A256")
    net = Net(hip, name)
    x = H.encoder_input("unit", 112, 1, 12, 39, 0.3)
    taps, z, lat = encode(hip, net, x)
    check_stages(net, f"{name}.synth.enc.B1.T12.unit", "encoder.", H.ENC_STAGES, x, taps)
    check_k1(net, f"{name}.synth.enc.B1.T12.unit", "encoder.pre_vq_conv", taps[5], z)
    check_codes(net, name, z, lat)
    dtaps, out = decode(hip, net, lat=lat)
    check_stages(net, f"{name}.synth.dec.B1.H3", "decoder.", H.DEC_STAGES, net.sd["vq_layer.embeddings"][lat], dtaps)
    check_k1(net, f"{name}.synth.dec.B1.H3", "decoder.project", dtaps[5], out)


# ----------------------------------------------------------------------------------------------- 2. the taps themselves
def family_launches(hip, fn):
    _lib, lib, ctx = hip
    n = (C.c_int64 * 4)()
    _lib.check(lib.ts_prof_read_n(ctx, 4, None, n, None, 1))
    _lib.check(lib.ts_prof_enable(ctx, 1))
    try:
        r = fn()
        torch.cuda.synchronize()
        _lib.check(lib.ts_prof_read_n(ctx, 4, None, n, None, 1))
    finally:
        _lib.check(lib.ts_prof_enable(ctx, 0))
    return r, [int(v) for v in n]


@pytest.mark.parametrize("name", ["V256/39", "V512/90"])
def test_taps_cost_nothing_and_are_one_shot(hip, name):
    """A tapped and an untapped call launch the same kernels (the ts_prof_read_n family counts) and return the same bits; the table serves
    one call: the call after it writes no tap; and the last tap chained through the final layer (ts_op_conv1d, the same packing and
    planning code) has the product output's bits."""
    _lib, lib, ctx = hip
    net = Net(hip, name)
    x = H.encoder_input("unit", 9, 3, 31, net.in_dim, 0.3)
    net.m.handle()                                                     # built ahead of the counts: ts_vqvae_create launches the decoder's code tables
    (t1, z1, l1), n1 = family_launches(hip, lambda: encode(hip, net, x, tap=True))
    (_, z0, l0), n0 = family_launches(hip, lambda: encode(hip, net, x, tap=False))
    assert n1 == n0 and sum(n0) > 0, (n1, n0)
    assert np.array_equal(bits(z1), bits(z0)) and np.array_equal(l1, l0)
    (d1, o1), m1 = family_launches(hip, lambda: decode(hip, net, lat=l1, tap=True))
    (_, o0), m0 = family_launches(hip, lambda: decode(hip, net, lat=l1, tap=False))
    assert m1 == m0 and sum(m0) > 0, (m1, m0)
    assert np.array_equal(bits(o1), bits(o0))
    # one-shot: the table is gone after the call it served, also after a call that failed
    bufs = tap_buffers(net.enc_shapes(3, 31))
    set_taps(hip, enc=[bufs])
    xd = dev(x)
    assert lib.ts_vqvae_encode(net.m.handle(), _lib.dptr(xd), 3, 31, None, None, None, _lib.stream_ptr()) != 0       # refused: no latents
    encode(hip, net, x, tap=False)
    torch.cuda.synchronize()
    assert all(np.all(bits(b.cpu().numpy()) == SENTINEL) for b in bufs)
    # a null table drops one that waits
    set_taps(hip, enc=[bufs])
    _lib.check(lib.ts_debug_trunk_taps(None))
    encode(hip, net, x, tap=False)
    assert all(np.all(bits(b.cpu().numpy()) == SENTINEL) for b in bufs)
    # consistency: the final layers on the last taps
    fp = C.POINTER(C.c_float)
    for tap, w, b, got in ((t1[5], "encoder.pre_vq_conv", 64, z1), (d1[5], "decoder.project", net.in_dim, o1)):
        td = dev(tap)
        B, L, Cin = tap.shape
        out = torch.empty((B, L, b), dtype=torch.float32, device="cuda")
        wt, bs = np.ascontiguousarray(net.sd[w + ".weight"], F32), np.ascontiguousarray(net.sd[w + ".bias"], F32)
        _lib.check(lib.ts_op_conv1d(ctx, _lib.dptr(td), B, L, Cin, wt.ctypes.data_as(fp), bs.ctypes.data_as(fp), b, 1, 1, 0, 0, 0,
                                    _lib.dptr(out), _lib.stream_ptr()))
        assert np.array_equal(bits(out.cpu().numpy()), bits(got)), w


def pair(hip):
    return Net(hip, "V256/39"), Net(hip, "V256/90")


def test_paired_taps_equal_each_network_alone(hip):
    """Body + hand in lockstep (ts_body_vq_infer, ts_vqvae_decode_pair): every tap of either network bit-equal to the network alone."""
    _lib, lib, ctx = hip
    vb, vh = pair(hip)
    for B, T in ((3, 31), (1, 6)):
        Hh = T // 4
        poses = H.encoder_input("unit", 21, B, T, 129, 0.3)
        eb, eh = tap_buffers(vb.enc_shapes(B, T)), tap_buffers(vh.enc_shapes(B, T))
        db, dh = tap_buffers(vb.dec_shapes(B, Hh)), tap_buffers(vh.dec_shapes(B, Hh))
        pd = dev(poses)
        codes = torch.empty((B, Hh, 2), dtype=torch.int64, device="cuda")
        recon = torch.empty((B, 4 * Hh, 129), dtype=torch.float32, device="cuda")
        set_taps(hip, enc=[eb, eh], dec=[db, dh])
        _lib.check(lib.ts_body_vq_infer(vb.m.handle(), vh.m.handle(), _lib.dptr(pd), B, T, _lib.dptr(codes), _lib.dptr(recon), _lib.stream_ptr()))
        torch.cuda.synchronize()
        codes, recon = codes.cpu().numpy(), recon.cpu().numpy()
        for net, e, d, col, sl in ((vb, host(eb, "pair enc"), host(db, "pair dec"), 0, slice(0, 39)),
                                   (vh, host(eh, "pair enc"), host(dh, "pair dec"), 1, slice(39, 129))):
            t1, z1, l1 = encode(hip, net, np.ascontiguousarray(poses[..., sl]))
            assert np.array_equal(l1, codes[..., col])
            d1, o1 = decode(hip, net, lat=l1)
            for k in range(6):
                assert np.array_equal(bits(t1[k]), bits(e[k])), ("enc", net.name, k, B, T)
                assert np.array_equal(bits(d1[k]), bits(d[k])), ("dec", net.name, k, B, T)
            assert np.array_equal(bits(o1), bits(recon[:, :, sl]))
        # ts_vqvae_decode_pair on other codes
        rng = np.random.default_rng(B)
        lb, lh = rng.integers(0, vb.ncode, (B, 5)), rng.integers(0, vh.ncode, (B, 5))
        db, dh = tap_buffers(vb.dec_shapes(B, 5)), tap_buffers(vh.dec_shapes(B, 5))
        out = torch.empty((B, 20, 129), dtype=torch.float32, device="cuda")
        lbd, lhd = dev(lb), dev(lh)
        set_taps(hip, dec=[db, dh])
        _lib.check(lib.ts_vqvae_decode_pair(vb.m.handle(), vh.m.handle(), _lib.dptr(lbd), _lib.dptr(lhd), B, 5, _lib.dptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        for net, d, lat, sl in ((vb, db, lb, slice(0, 39)), (vh, dh, lh, slice(39, 129))):
            d1, o1 = decode(hip, net, lat=lat)
            assert all(np.array_equal(bits(d1[k]), bits(host(d, "pair dec")[k])) for k in range(6)), net.name
            assert np.array_equal(bits(o1), bits(out.cpu().numpy()[:, :, sl]))


@pytest.mark.parametrize("T_max", [31, 78])
def test_masked_pair_taps(hip, T_max):
    """ts_vqvae_encode_pair_masked / ts_vqvae_decode_pair_masked with clips of lens (T_max, a middle value that is no multiple of 4, the
    entries' minimum 4), the caller's rows beyond a clip's length NaN-filled: every tap's valid rows bit-equal to the clip run alone, rows at
    or beyond the stage's own length ((lens >> shr) << shl, as LenMask has it) exactly +0.0."""
    from talkshow_amd.modules import encode_pair_masked
    _lib, lib, ctx = hip
    vb, vh = pair(hip)
    lens_h = np.array([T_max, {31: 13, 78: 41}[T_max], 4], np.int32)
    B, Hm = 3, T_max // 4
    poses = H.encoder_input("unit", 33, B, T_max, 129, 0.3)
    block = poses.copy()
    for b in range(B):
        block[b, lens_h[b]:] = np.nan
    lens = dev(lens_h)
    eb, eh = tap_buffers(vb.enc_shapes(B, T_max)), tap_buffers(vh.enc_shapes(B, T_max))
    set_taps(hip, enc=[eb, eh])
    codes, zb, zh = encode_pair_masked(vb.m, vh.m, dev(block), lens, want_z=True)
    torch.cuda.synchronize()
    codes = codes.cpu().numpy()
    eb, eh = host(eb, "masked enc"), host(eh, "masked enc")
    lat = np.random.default_rng(3).integers(0, 70, (2, B, Hm))
    for b in range(B):
        lat[:, b, lens_h[b] >> 2:] = -7                                 # whatever the caller left there: not read
    db, dh = tap_buffers(vb.dec_shapes(B, Hm)), tap_buffers(vh.dec_shapes(B, Hm))
    out = torch.from_numpy(np.full((B, 4 * Hm, 129), SENTINEL, np.uint32).view(F32)).cuda()
    lbd, lhd = dev(lat[0].astype(np.int64)), dev(lat[1].astype(np.int64))
    set_taps(hip, dec=[db, dh])
    _lib.check(lib.ts_vqvae_decode_pair_masked(vb.m.handle(), vh.m.handle(), _lib.dptr(lbd), _lib.dptr(lhd), _lib.dptr(lens), B, Hm, _lib.dptr(out),
                                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    db, dh, out = host(db, "masked dec"), host(dh, "masked dec"), out.cpu().numpy()
    for b in range(B):
        n, h = int(lens_h[b]), int(lens_h[b]) >> 2
        for net, e, d, col, sl, z in ((vb, eb, db, 0, slice(0, 39), zb), (vh, eh, dh, 1, slice(39, 129), zh)):
            t1, z1, l1 = encode(hip, net, np.ascontiguousarray(poses[b:b + 1, :n, sl]))
            d1, o1 = decode(hip, net, lat=lat[col][b:b + 1, :h])
            for k in range(6):
                le, ld = n >> (k // 2), h << (k // 2)
                assert t1[k].shape[1] == le and d1[k].shape[1] == ld
                assert np.array_equal(bits(t1[k][0]), bits(e[k][b, :le])), ("enc", b, net.name, k)
                assert np.all(bits(e[k][b, le:]) == 0), ("enc beyond", b, net.name, k)
                assert np.array_equal(bits(d1[k][0]), bits(d[k][b, :ld])), ("dec", b, net.name, k)
                assert np.all(bits(d[k][b, ld:]) == 0), ("dec beyond", b, net.name, k)
            assert np.array_equal(bits(z1[0]), bits(z.cpu().numpy()[b, :h])) and np.all(bits(z.cpu().numpy()[b, h:]) == 0)
            assert np.array_equal(l1[0], codes[b, :h, col]) and np.all(codes[b, h:, col] == -1)
            assert np.array_equal(bits(o1[0]), bits(out[b, :4 * h, sl])) and np.all(bits(out[b, 4 * h:, sl]) == 0)


@pytest.mark.parametrize("name", ["V256/39", "V512/90", "A256"])
def test_arena_hygiene(hip, name):
    """A small pass, then on the same handles and stream larger passes on inputs of magnitude 1e20 and 3e38 (the second overflows to inf
    and NaN inside the arenas; neither faults anything), then the small pass again: every tap and output of the last call bit-equal to the
    first."""
    net = Net(hip, name)
    x = H.encoder_input("unit", 41, 1, 7, net.in_dim, net.in_scale)
    big = H.encoder_input("unit", 42, 3, 31, net.in_dim, 1.0)
    first = encode(hip, net, x)
    encode(hip, net, (big * F32(1e20)).astype(F32))
    with np.errstate(over="ignore"):
        bt, bz, _ = encode(hip, net, (big * F32(3e38)).astype(F32))
    # it did overflow: inf and NaN in the taps behind a LeakyReLU (a stack's closing ReLU is v > 0 ? v : 0, which turns a NaN into 0)
    assert not np.isfinite(bt[0]).all()
    third = encode(hip, net, x)
    for a, b in zip(first[0] + [first[1]], third[0] + [third[1]]):
        assert np.array_equal(bits(a), bits(b))
    assert first[2] is None or np.array_equal(first[2], third[2])
    if net.kind == "audio":
        return
    lat = np.random.default_rng(5).integers(0, net.ncode, (1, 2))
    d1, o1 = decode(hip, net, lat=lat)
    zbig = np.random.default_rng(6).standard_normal((3, 8, 64)).astype(F32)
    decode(hip, net, z=zbig * F32(1e20))
    with np.errstate(over="ignore"):
        dt, _ = decode(hip, net, z=zbig * F32(3e38))
    assert not np.isfinite(dt[0]).all()
    d3, o3 = decode(hip, net, lat=lat)
    for a, b in zip(d1 + [o1], d3 + [o3]):
        assert np.array_equal(bits(a), bits(b))
