"""The PixelCNN chain (csrc/pixelcnn.cpp) stage by stage on the GPU, through the stage taps of include/talkshow_hip_debug.h
(ts_debug_pixelcnn_taps): the PRODUCTION pass copies out what every launch of a code row wrote; tests/test_pix_stages_host.py holds the
float64 references, scales, ceilings and bounds.  All passes go through modules.GatedPixelCNN.run / open_stream or, for clips of different
lengths, the C entry ts_pixelcnn_generate_mixed.

Tap buffers are filled with the NaN sentinel 0x7FE5A5A5 ahead of every pass and have red zones on each side: `Taps.collect` decodes every
slab a pass must write (a surviving NaN = a missing write) and then demands the sentinel in every float outside the copied extents (a
changed pattern = a stage, unit or row the pass must not write, or a copy past its slab).

(a) test_stages_against_float64: every stage of every row against float64, each from the GPU's own taps of the stages before it (earlier
    rows included) and the device's AE rows (ts_debug_pixelcnn_work), no element skipped.  Units, ceilings and bounds: the host file.
    XH_l for l >= 2 (horiz_resid as loaded, a dominated sum under residual_cancel) is held to the partial-sum scale of its own chain and,
    where K < 256, to the bits of an fp32 restatement of the kernels' documented order (the host file says why).
    Every case records its largest error per stage family through TS_MEASURED_LOG (profiles/pix_stages_measured.jsonl).
(b) test_bits_across_forms / test_bits_across_knobs: for the same clip, labels, audio and (greedy, hence equal) codes, every stage of
    every row has equal bits under the chunked one-shot path, the whole-call graph's configuration, a mixed pass with a longer and a
    shorter neighbour, a session fed 1, 3 and 8 rows, a pass behind a pre_codes prefix (whose prefix rows run the vertical stack only),
    TS_PIX_TABLES 0 / 1, and in child processes TS_NO_GRAPH=1, TS_PIX_DEFER_P=0 / 1 and TS_SKINNY_TILED=0 (after decoding).  A form that
    looks ahead past the clip's end (chunks, sessions) writes P / Q1 / Q0 on rows where the whole call does not: the forms are compared
    on the stages both have, and each form's own set is pinned by the sentinel check.
(c) test_tap_changes_nothing: codes and logits of a tapped pass equal the untapped pass's bits; ts_debug_pixelcnn_graphs and
    graph_captures do not move; an untapped pass right after leaves the sentinel-filled buffers untouched; a one-row table writes one row.

Networks (V = 64 unless said): D 32 / 1 layer (the NL == 1 branch), 32 / 2 (no l >= 2 segment, no T0), 64 / 3 (K < 256, W = 4), 128 / 3
(2D = 256, W = 8, tiled operands), 256 / 15 / V 2048 (the shipped size, H = 4, B = 32 and 65).  H = 10: rows 0 .. 3 differ in which of E, Q1,
Q0 exist, row 4 wraps the rings, rows 7 -> 8 cross CHUNK_ROWS, the last row has no P and no riders.  B in {1, 3, 17, 65}: 17 is no multiple
of the 16-row padding, 65 takes the code tables by the automatic rule and the wide kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_pix_stages_host as HS
from test_gpu_chain_ops import NANBITS, RZ, round16, tiled_lin

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
H_ROWS = 10
I32P = C.POINTER(C.c_int32)
HERE = os.path.abspath(__file__)
STAGES = ("HV", "OV", "P", "Q1", "Q0", "V2H", "G", "XH", "T0", "Y", "LG")
CHUNKED = os.environ.get("TS_NO_GRAPH", "0") in ("", "0")     # a first-time one-shot shape of more than 8 rows runs as chunks, unless eager


def record(name, **kv):
    print(f"\n[measured] {name}: " + ", ".join(f"{k} = {v:.3e}" if isinstance(v, float) else f"{k} = {v}" for k, v in kv.items()))
    log = os.environ.get("TS_MEASURED_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(name=name, **kv)) + "\n")


def is_tiled(D):
    return D % 128 == 0 and os.environ.get("TS_SKINNY_TILED", "1") != "0"


_NETS = {}


def network(name, regime="synth"):
    """(module on the GPU, raw state dict) of a network of HS.NETWORKS under a weight regime, made once."""
    if (name, regime) not in _NETS:
        from talkshow_amd import synth
        from talkshow_amd.modules import GatedPixelCNN
        assert torch.cuda.is_available(), "gpu tests need a HIP device"
        D, NL, V = HS.NETWORKS[name]
        sd = HS.state_dict(name, regime)
        net = GatedPixelCNN(V, D, NL, HS.NC, True, True, aud_dim=HS.AD).cuda()
        net.load_state_dict(synth.to_torch(sd))
        _NETS[name, regime] = (net, sd)
    return _NETS[name, regime]


def keys_of_row(NL, r, need_h, last_row, first_row=0):
    """The stages a pass writes on code row r: (stage, unit) in tap terms -> the host file's key.  last_row: rows at or beyond it are never
    generated (a one-shot call: its row count; chunks and sessions look ahead without end: None)."""
    far = last_row is None
    ks = {}
    for l in range(NL):
        ks["HV", l] = ("HV", l)
        ks["OV", l] = ("OV", l)
        ks["V2H", l] = ("V2H", l)
        if l >= 1 and (far or r + 1 < last_row):
            ks["P", l] = ("P", l)
    if r >= 1 and (far or r + 1 < last_row):
        ks["Q1", 0] = ("Q1",)
    if r >= 1 and (far or r + 2 < last_row):
        ks["Q0", 0] = ("Q0",)
    if need_h:
        for j in range(2):
            for l in range(NL):
                ks["G", 2 * l + j] = ("G", l, j)
                if l >= 1:
                    ks["XH", 2 * l + j] = ("XH", l, j)
            ks["Y", j] = ("Y", j)
            ks["LG", j] = ("LG", j)
        for l in range(1, NL):
            ks["T0", l] = ("T0", l)
    return ks


class Taps:
    """The tap buffers of one network for rows [0, rows): sentinel fill, red zones, the table, decoding."""

    def __init__(self, name, rows, clips):
        D, NL, V = HS.NETWORKS[name]
        self.D, self.NL, self.V, self.rows, self.clips = D, NL, V, rows, clips
        self.tiled = is_tiled(D)
        self.units = dict(HV=NL, OV=NL, P=NL, Q1=1, Q0=1, V2H=NL, G=2 * NL, XH=2 * NL, T0=NL, Y=2, LG=2)
        self.width = dict(HV=4 * D, OV=2 * D, P=4 * D, Q1=4 * D, Q0=4 * D, V2H=4 * D, G=D, XH=D, T0=2 * D, Y=HS.HID, LG=V)
        self.slab = {k: round16(clips) * w for k, w in self.width.items()}
        self.buf = {k: torch.empty(2 * RZ + rows * self.units[k] * self.slab[k], dtype=torch.int32, device="cuda") for k in STAGES}
        self.fill()

    def fill(self):
        for b in self.buf.values():
            b.fill_(NANBITS)

    def arm(self, row=-1):
        from talkshow_amd import _lib
        t = _lib.PixTaps()
        t.row, t.row0, t.rows, t.slab_clips = row, 0, self.rows, self.clips
        for i, k in enumerate(STAGES):
            t.stage[i] = self.buf[k].data_ptr() + 4 * RZ
        assert tuple(_lib.PIX_TAP_STAGES) == STAGES
        _lib.load().ts_debug_pixelcnn_taps(C.byref(t))

    def layout(self, stage, unit, B):
        """(rows M, row stride, written columns, tiled view width or 0) of a stage's launch output."""
        D, tw = self.D, self.tiled
        if stage == "HV":
            return B, 4 * D, 4 * D, 2 * D * tw
        if stage == "OV":
            last = unit == self.NL - 1 and unit != 0
            return B, 2 * D, 2 * D, 0 if last else 2 * D * tw
        if stage == "V2H":
            return 2 * B, 2 * D, 2 * D, 0
        if stage in ("G", "XH"):
            return B, D, D, D * tw
        if stage == "Y":
            return B, HS.HID, HS.HID, HS.HID * tw
        return B, self.width[stage], self.width[stage], 0

    def collect(self, B, plan, clips=None):
        """plan: {row: {(stage, unit): key}} = exactly what the pass must have written.  Returns {row: {key: float32 array}} with the host
        file's shapes for clips [0, clips); asserts no NaN in them and the sentinel in every float outside the copied extents."""
        torch.cuda.synchronize()
        out = {}
        for stage in STAGES:
            raw = self.buf[stage].cpu().numpy().view(np.uint32)
            body = raw[RZ:-RZ]
            seen = np.zeros(body.size, bool)
            for r, ks in plan.items():
                for (st, unit), key in ks.items():
                    if st != stage:
                        continue
                    Br = B[r] if isinstance(B, dict) else B
                    M, stride, cols, tw = self.layout(stage, unit, Br)
                    base = (r * self.units[stage] + unit) * self.slab[stage]
                    n = round16(-(-M * stride // tw)) * tw if tw else M * stride
                    assert n <= self.slab[stage]
                    seen[base:base + n] = True
                    lin = np.arange(M)[:, None] * stride + np.arange(cols)[None, :]
                    v = body[base:base + n][tiled_lin(lin, tw) if tw else lin].view(F32)
                    assert np.isfinite(v).all(), f"row {r} {key}: {int((~np.isfinite(v)).sum())} elements were not written"
                    v = v.reshape(Br, -1)
                    if stage in ("HV", "OV", "P", "Q1", "Q0", "V2H"):
                        v = v.reshape(Br, 2, -1)
                    out.setdefault(r, {})[key] = v[:clips] if clips else v
            assert (raw[:RZ] == NANBITS).all() and (raw[-RZ:] == NANBITS).all(), f"{stage}: a red zone of the tap buffer changed"
            stray = np.flatnonzero(~seen & (body != NANBITS))
            assert stray.size == 0, f"{stage}: {stray.size} floats written outside the stages of the pass, first at row " \
                                    f"{stray[0] // (self.units[stage] * self.slab[stage])} unit {stray[0] // self.slab[stage] % self.units[stage]}"
        return out


def work_buffer(net, which, n):
    from talkshow_amd import _lib
    buf = torch.empty(n, dtype=torch.float32, device="cuda")
    got = _lib.load().ts_debug_pixelcnn_work(net.handle(), _lib.stream_ptr(), which, _lib.dptr(buf), n, 0)
    assert got >= n, (got, n)
    return buf.cpu().numpy()


def device_ae(net, sd, aud, B, H, D, NL):
    """The device's AE rows (B, H, D) of the latest pass, checked against float64 (a conv GEMM: WHOLE_BOUND) before they feed the references."""
    from test_gpu_conv_ops import WHOLE_BOUND
    ae = work_buffer(net, 5, B * H * D).reshape(B, H, D)
    want = HS.Ref(sd, NL).audio(aud.astype(F64))
    s_ae = np.abs(aud.astype(F64)) @ np.abs(sd["embedding_aud.weight"][:, :, 0, 0].astype(F64)).T + np.abs(sd["embedding_aud.bias"].astype(F64))
    assert np.max(np.abs(ae - want) / s_ae) <= WHOLE_BOUND
    return ae


def inputs(name, B, H, seed=5):
    codes, label, aud = HS.clip_inputs(name, B, H, seed)
    return codes, label, aud, torch.from_numpy(label).cuda(), torch.from_numpy(aud).cuda()


def check_rows(name, regime, sd, taps, codes, label, ae, rows, horizontal_from, last_row, case):
    """(a): every stage of `rows` against float64 from the taps; returns nothing, asserts and records per family."""
    D, NL, V = HS.NETWORKS[name]
    ref = HS.Ref(sd, NL)
    given = {r: dict(taps[r], AE=ae[:, r]) for r in taps}
    worst = {}
    fails = []
    for r in rows:
        want = HS.run_row(ref, r, codes, label, None, None, given=given, last_row=1 << 30 if last_row is None else last_row)
        for key, got in taps[r].items():
            u = HS.units(key, got, want[key], D, NL)
            fam = HS.family(key, D, NL)
            extra = {}
            if fam == "resid":       # XH_l, l >= 2: in units of the partial-sum scale; the figure in units of S travels with the record
                extra = dict(units_of_S=HS.units(key, got, want[key][:2], D, NL))
                if D < 256:          # and, where W = 4, the fp32 restatement of the kernels' documented order: the same bits
                    l, j = key[1], key[2]
                    mine = ref.resid_chain(l - 1, taps[r]["G", l - 1, j], taps[r]["XH", l - 1, j], fp32=True)[0]
                    nbad = int((mine.view(np.uint32) != got.view(np.uint32)).sum())
                    assert nbad == 0, f"{case}: row {r} {key}: {nbad} elements differ from the fp32 restatement of the documented order"
            if u > worst.get(fam, (-1.0,))[0]:
                worst[fam] = (u, key, r, extra)
            if u > HS.bound(key, D, NL):
                fails.append((r, key, u, HS.bound(key, D, NL)))
        missing = [k for k in want if k not in taps[r] and (r >= horizontal_from or k[0] in ("HV", "OV", "P", "Q1", "Q0", "V2H"))]
        assert not missing, f"row {r}: stages without a tap: {missing}"
    for fam, (u, key, r, extra) in sorted(worst.items()):
        record(f"{case}/{fam}", units=u, stage="_".join(str(x) for x in key), row=r, bound=HS.bound(key, D, NL), ceiling=HS.ceiling(key, D, NL),
               **extra)
    assert not fails, f"{case}: {len(fails)} stages over their bound, first (row, stage, units, bound): {fails[:4]}"


CASES_F = [("d32l1", "synth", 3), ("d32l2", "synth", 17), ("d64l3", "synth", 1), ("d64l3", "synth", 3), ("d64l3", "synth", 17),
           ("d64l3", "synth", 65), ("d64l3", "fold_extreme", 17), ("d64l3", "residual_cancel", 17), ("d128l3", "synth", 3),
           ("d128l3", "synth", 17), ("d128l3", "synth", 65), ("d128l3", "fold_extreme", 3), ("d128l3", "residual_cancel", 3),
           ("d32l2", "fold_extreme", 3), ("d32l2", "residual_cancel", 17), ("d32l1", "synth", 17)]
# the greedy form runs where it adds a path: small and wide passes, every regime
CASES_A = [c + ("forced",) for c in CASES_F] + [c + ("greedy",) for c in CASES_F if c[2] in (3, 65) or c[1] != "synth"]


@pytest.mark.parametrize("name,regime,B,mode", CASES_A)
def test_stages_against_float64(name, regime, B, mode):
    """(a) on H = 10 rows: teacher-forced with logits (the eager whole call), and greedy (the chunked path of a first-time shape)."""
    from talkshow_amd import _lib
    D, NL, V = HS.NETWORKS[name]
    net, sd = network(name, regime)
    codes, label, aud, label_d, aud_d = inputs(name, B, H_ROWS)
    taps = Taps(name, H_ROWS, B)
    _lib.load().ts_debug_pixelcnn_tables(net.handle(), -1)       # the automatic rule; drops the graphs an earlier test left
    taps.arm()
    if mode == "forced":
        out_codes, logits = net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=torch.from_numpy(codes).cuda(), want_logits=True)
        last = H_ROWS
    else:
        out_codes, logits = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
        codes = out_codes.cpu().numpy()
        last = None if CHUNKED else H_ROWS             # chunks look ahead past the end
    got = taps.collect(B, {r: keys_of_row(NL, r, True, last) for r in range(H_ROWS)})
    ae = device_ae(net, sd, aud, B, H_ROWS, D, NL)
    if logits is not None:                              # the logits the call returned are the LG taps, bit for bit
        for r in range(H_ROWS):
            for j in range(2):
                assert np.array_equal(logits[:, r, j].cpu().numpy().view(np.uint32), got[r]["LG", j].view(np.uint32))
    check_rows(name, regime, sd, got, codes, label, ae, range(H_ROWS), 0, last, f"{name}/{regime}/B{B}/{mode}")


@pytest.mark.parametrize("B", [32, 65])
def test_stages_shipped_size(B):
    """(a) at the shipped size 256 / 15 layers / 2048 codes, H = 4, teacher forced with logits."""
    from talkshow_amd import _lib
    name, H = "shipped", 4
    D, NL, V = HS.NETWORKS[name]
    net, sd = network(name)
    codes, label, aud, label_d, aud_d = inputs(name, B, H)
    taps = Taps(name, H, B)
    _lib.load().ts_debug_pixelcnn_tables(net.handle(), -1)       # the automatic rule: B = 65 takes the tables, B = 32 the GEMMs
    taps.arm()
    net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=torch.from_numpy(codes).cuda(), want_logits=True)
    got = taps.collect(B, {r: keys_of_row(NL, r, True, H) for r in range(H)})
    ae = device_ae(net, sd, aud, B, H, D, NL)
    check_rows(name, "synth", sd, got, codes, label, ae, range(H), 0, H, f"{name}/synth/B{B}/forced")


# ----------------------------------------------------------------------------------------------- (b) bits across pass forms
def base_form(name, regime, B, H=H_ROWS):
    """The greedy one-shot pass of a first-time shape (chunked), tapped -> (codes, taps by row, the inputs)."""
    from talkshow_amd import _lib
    D, NL, V = HS.NETWORKS[name]
    net, sd = network(name, regime)
    codes, label, aud, label_d, aud_d = inputs(name, B, H)
    taps = Taps(name, H, B)
    _lib.load().ts_debug_pixelcnn_tables(net.handle(), -1)       # the automatic rule; without graphs the shape chunks
    taps.arm()
    out, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    got = taps.collect(B, {r: keys_of_row(NL, r, True, None if CHUNKED else H) for r in range(H)})
    return out.cpu().numpy(), got


def same_bits(a, b, what, clip=slice(None), rows=None, vertical_only_below=0):
    """Every stage both forms have, bit for bit, on the clips `clip` of a (b holds those clips alone or all of them alike)."""
    n = 0
    for r in (rows if rows is not None else sorted(set(a) & set(b))):
        for key in a[r]:
            if key not in b[r]:
                continue
            x, y = a[r][key][clip], b[r][key]
            assert x.shape == y.shape, (what, r, key, x.shape, y.shape)
            bad = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).reshape(-1))
            assert bad.size == 0, f"{what}: row {r} stage {key}: {bad.size} of {x.size} elements differ in bits"
            n += 1
    assert n > 0
    return n


@pytest.mark.parametrize("name,regime,B", [("d64l3", "synth", 3), ("d128l3", "fold_extreme", 3), ("d32l2", "synth", 17), ("d32l1", "synth", 3)])
def test_bits_across_forms(name, regime, B):
    from talkshow_amd import _lib
    lib = _lib.load()
    D, NL, V = HS.NETWORKS[name]
    H = H_ROWS
    net, sd = network(name, regime)
    lib.ts_debug_pixelcnn_tables(net.handle(), -1)       # the automatic rule, no graph of an earlier test
    codes, label, aud, label_d, aud_d = inputs(name, B, H)
    plan_far = {r: keys_of_row(NL, r, True, None) for r in range(H)}
    plan_call = {r: keys_of_row(NL, r, True, H) for r in range(H)}
    taps = Taps(name, H, B)
    # the chunked one-shot path: a first-time shape of more than CHUNK_ROWS rows
    assert lib.ts_debug_pixelcnn_graphs(net.handle(), _lib.stream_ptr()) == 0
    taps.arm()
    out, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    base = taps.collect(B, plan_far)
    gcodes = out.cpu().numpy()
    # the whole-call graph's configuration: the shape pinned, so the call no longer chunks
    net.prepare(B, H)
    untapped, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    assert np.array_equal(untapped.cpu().numpy(), gcodes)
    taps.fill()
    taps.arm()
    out, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    assert np.array_equal(out.cpu().numpy(), gcodes)
    whole = taps.collect(B, plan_call)
    same_bits(base, whole, "whole call vs chunks")
    # teacher forced with logits on the greedy codes (the eager whole call)
    taps.fill()
    taps.arm()
    net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=torch.from_numpy(gcodes).cuda(), want_logits=True)
    same_bits(base, taps.collect(B, plan_call), "teacher forced vs greedy")
    # TS_PIX_TABLES 0 / 1
    for m in (1, 0):
        assert lib.ts_debug_pixelcnn_tables(net.handle(), m) in (0, 1)
        taps.fill()
        taps.arm()
        out, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
        assert np.array_equal(out.cpu().numpy(), gcodes)
        same_bits(base, taps.collect(B, plan_far), f"TS_PIX_TABLES={m}")
    lib.ts_debug_pixelcnn_tables(net.handle(), -1)
    # behind a pre_codes prefix of 4 rows: rows 0 .. 3 run the vertical stack only
    taps.fill()
    taps.arm()
    out, _ = net.run(label_d, aud_d[:, 4:].contiguous(), mode=_lib.TS_SAMPLE_GREEDY, pre_codes=torch.from_numpy(gcodes[:, :4]).cuda(),
                     pre_aud=aud_d[:, :4].contiguous())
    assert np.array_equal(out.cpu().numpy(), gcodes[:, 4:])
    pre = taps.collect(B, {r: keys_of_row(NL, r, r >= 4, H) for r in range(H)})
    n_v = same_bits(base, pre, "prefix: vertical rows", rows=range(4))
    assert n_v == sum(len(pre[r]) for r in range(4)) and all(k[0] not in ("G", "XH", "T0", "Y", "LG") for r in range(4) for k in pre[r])
    same_bits(base, pre, "prefix: generated rows", rows=range(4, H))
    # a session fed 1, 3 and 8 rows (12 rows of audio: the clip's 10 and two more)
    aud12 = torch.cat([aud_d, aud_d[:, :2]], 1).contiguous()
    st = net.open_stream(label_d, B, 8)
    t12 = Taps(name, 12, B)
    r0 = 0
    sess = []
    for n in (1, 3, 8):
        t12.arm()
        sess.append(st.step(aud12[:, r0:r0 + n].contiguous(), mode=_lib.TS_SAMPLE_GREEDY).cpu().numpy())
        r0 += n
    st.close()
    assert np.array_equal(np.concatenate(sess, 1)[:, :H], gcodes)
    stream = t12.collect(B, {r: keys_of_row(NL, r, True, None) for r in range(12)})
    same_bits(base, stream, "session 1 + 3 + 8", rows=range(H))
    # a mixed pass: the clips of the base pass as the MIDDLE clips, a 12-row clip ahead and a 6-row clip behind
    Bm = B + 2
    lens = np.array([12 * 4] + [H * 4] * B + [6 * 4], np.int32)
    audm = torch.zeros((Bm, 12, HS.AD), dtype=torch.float32, device="cuda")
    audm[0] = aud12[0]
    audm[1:1 + B, :H] = aud_d
    audm[1 + B, :6] = aud_d[0, :6]
    labm = torch.cat([label_d[:1], label_d, label_d[:1]]).contiguous()
    cm = torch.zeros((Bm, 12, 2), dtype=torch.int64, device="cuda")
    lens_d = torch.from_numpy(lens).cuda()
    tm = Taps(name, 12, Bm)
    tm.arm()
    _lib.pixelcnn_mixed_call((net.handle(), _lib.dptr(labm), _lib.dptr(audm), lens.ctypes.data_as(I32P), _lib.dptr(lens_d), Bm, 12,
                              _lib.TS_SAMPLE_GREEDY, None, 0, None, _lib.dptr(cm)))
    assert np.array_equal(cm.cpu().numpy()[1:1 + B, :H], gcodes)
    active = {r: Bm if r < 8 else Bm - 1 for r in range(12)}          # chunk [8, 12) runs without the 6-row clip
    mixed = tm.collect(active, {r: keys_of_row(NL, r, True, None) for r in range(12)})
    same_bits({r: {k: v[1:1 + B] for k, v in mixed[r].items()} for r in range(H)}, base, "mixed pass", rows=range(H))


KNOBS = [("TS_NO_GRAPH", "1"), ("TS_PIX_DEFER_P", "0"), ("TS_PIX_DEFER_P", "1"), ("TS_SKINNY_TILED", "0")]


@pytest.mark.parametrize("knob,value", KNOBS)
def test_bits_across_knobs(knob, value, tmp_path):
    """The knobs a process reads once, in a child process: the tapped greedy pass of d128l3 (tiled operands, W = 8) and d64l3 there equals
    this process's, stage by stage, after decoding."""
    env = dict(os.environ, **{knob: value})
    env.pop("TS_MEASURED_LOG", None)
    r = subprocess.run([sys.executable, HERE, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(HERE)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name, regime, B in CHILD_CASES:
        codes, mine = base_form(name, regime, B)
        z = np.load(tmp_path / f"{name}.npz")
        assert np.array_equal(z["codes"], codes)
        theirs = {}
        for k in z.files:
            if k != "codes":
                rr, *key = k.split("|")
                theirs.setdefault(int(rr), {})[tuple(int(x) if x.isdigit() else x for x in key)] = z[k]
        if knob == "TS_NO_GRAPH":     # the whole eager call there, the chunks here: the look-ahead sums past the end exist here only
            assert ("P", 1) not in theirs[H_ROWS - 1] and ("P", 1) in mine[H_ROWS - 1]
        same_bits(mine, theirs, f"{knob}={value} {name}")


CHILD_CASES = [("d128l3", "synth", 17), ("d64l3", "residual_cancel", 3)]


def child_main(out_dir):
    for name, regime, B in CHILD_CASES:
        codes, got = base_form(name, regime, B)
        flat = {"|".join([str(r)] + [str(x) for x in key]): v for r in got for key, v in got[r].items()}
        np.savez(os.path.join(out_dir, f"{name}.npz"), codes=codes, **flat)


# ----------------------------------------------------------------------------------------------- (c) the tap changes nothing
@pytest.mark.parametrize("name,B", [("d64l3", 3), ("d128l3", 17)])
def test_tap_changes_nothing(name, B):
    from talkshow_amd import _lib
    lib = _lib.load()
    D, NL, V = HS.NETWORKS[name]
    H = H_ROWS
    net, sd = network(name)
    lib.ts_debug_pixelcnn_tables(net.handle(), -1)
    codes, label, aud, label_d, aud_d = inputs(name, B, H, seed=9)
    codes_d = torch.from_numpy(codes).cuda()
    taps = Taps(name, H, B)
    for _ in range(3):                                   # the third sighting makes the shape hot: it gets its whole-call graph
        plain, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    _, plain_logits = net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=codes_d, want_logits=True)
    torch.cuda.synchronize()
    graphs, captures = lib.ts_debug_pixelcnn_graphs(net.handle(), _lib.stream_ptr()), net.graph_captures()
    assert graphs >= 1
    taps.arm()
    tapped, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    got = taps.collect(B, {r: keys_of_row(NL, r, True, H) for r in range(H)})
    assert np.array_equal(tapped.cpu().numpy(), plain.cpu().numpy())
    assert (lib.ts_debug_pixelcnn_graphs(net.handle(), _lib.stream_ptr()), net.graph_captures()) == (graphs, captures)
    taps.fill()
    taps.arm()
    _, tapped_logits = net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=codes_d, want_logits=True)
    taps.collect(B, {r: keys_of_row(NL, r, True, H) for r in range(H)})
    assert np.array_equal(tapped_logits.cpu().numpy().view(np.uint32), plain_logits.cpu().numpy().view(np.uint32))
    # the table was one-shot: the same passes right after write nothing
    taps.fill()
    again, _ = net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    net.run(label_d, aud_d, mode=_lib.TS_TEACHER_FORCED, codes=codes_d, want_logits=True)
    taps.collect(B, {})
    assert np.array_equal(again.cpu().numpy(), plain.cpu().numpy())
    assert (lib.ts_debug_pixelcnn_graphs(net.handle(), _lib.stream_ptr()), net.graph_captures()) == (graphs, captures)
    # a table that waits is dropped by null; a one-row table taps that row alone, with the same bits
    taps.arm()
    lib.ts_debug_pixelcnn_taps(None)
    net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    taps.collect(B, {})
    taps.arm(row=5)
    net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    one = taps.collect(B, {5: keys_of_row(NL, 5, True, H)})
    same_bits(got, one, "one-row table", rows=[5])
    # an entry that fails drops the table too
    taps.fill()
    taps.arm()
    assert lib.ts_pixelcnn_generate(net.handle(), None, None, B, H, _lib.TS_SAMPLE_GREEDY, None, 0, 0, None, None, None, None, 0, None) != 0
    net.run(label_d, aud_d, mode=_lib.TS_SAMPLE_GREEDY)
    taps.collect(B, {})


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    child_main(sys.argv[1])
