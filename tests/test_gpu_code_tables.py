"""The PixelCNN chain's code tables (csrc/code_tables.hip) against the GEMM launches they replace: slot V0 of rows r >= 1 and
hg_0 of column 1 as lookups of slice sums.  The contract is BIT identity, so every comparison is equality of bits, never a tolerance.

`ts_debug_pixelcnn_tables(pix, mode)` sets TS_PIX_TABLES for one model object (1: every pass takes the tables, 0: today's GEMM launches) and
drops its graphs, so one process runs both sides; one test runs the knob-off side in a child process under the environment variable itself.
The work buffers the lookups write — HV(0) (the pre-gate values), OV0, the Q1 / Q0 riders, G(0) — are read back whole through
`ts_debug_pixelcnn_work`; ahead of every run they are filled with a NaN sentinel, so an element one side writes and the other does not shows.

Small networks (D = 32 / 64, V = 64, 2 / 3 layers, 5 rows) keep the tables tiny; their K has 4 slices.  The shipped size (D = 256, V = 2048)
runs the real slice bookkeeping (8 slices, tiled operands) at B = 32 (split-K kernels) and B = 65 (the wide kernel), 3 rows.

A clip without a single code row cannot enter a pass (the entries refuse clips shorter than 4 frames, tables or not): the mixed pass here
runs three lengths down to the shortest a pass takes, ONE code row, and checks that the refusal of a shorter one is the same on both sides.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from talkshow_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
I32P = C.POINTER(C.c_int32)
V = 64
SMALL = {"d32": dict(input_dim=V, dim=32, n_layers=2), "d64": dict(input_dim=V, dim=64, n_layers=3)}
SENT = 0x7FC0BEEF
WORK = {"HV": 0, "OV0": 1, "Q1": 2, "Q0": 3, "G": 4}
H = 5


def _np(t):
    return t.cpu().numpy()


def _make(dims, seed):
    from talkshow_amd.modules import GatedPixelCNN
    m = GatedPixelCNN(dims["input_dim"], dims["dim"], dims["n_layers"], 4, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, **dims)))
    return m


@pytest.fixture(scope="module")
def nets():
    return {k: _make(d, 11) for k, d in SMALL.items()}


@pytest.fixture(scope="module")
def shipped():
    return _make(dict(input_dim=2048, dim=256, n_layers=15), 7)


def tables(pix, mode):
    from talkshow_amd import _lib
    got = _lib.load().ts_debug_pixelcnn_tables(pix.handle(), mode)
    assert got >= 0, _lib.load().ts_last_error()
    if mode != 0:
        assert got == 1, "the model built no code tables"


class WorkBuffers:
    """The five work buffers of the current stream's Work: poison() fills them with the sentinel, bits() reads them back whole."""

    def __init__(self, pix):
        from talkshow_amd import _lib
        self.lib, self.pix, self.s = _lib.load(), pix, _lib.stream_ptr()
        self.tmp = torch.full((1 << 24,), SENT, dtype=torch.int32, device="cuda")      # 64 MB: larger than any buffer of these runs

    def poison(self):
        self.tmp.fill_(SENT)
        for w in WORK.values():
            n = self.lib.ts_debug_pixelcnn_work(self.pix.handle(), self.s, w, C.c_void_p(self.tmp.data_ptr()), self.tmp.numel(), 1)
            assert 0 < n < self.tmp.numel()

    def bits(self):
        out = {}
        for k, w in WORK.items():
            n = self.lib.ts_debug_pixelcnn_work(self.pix.handle(), self.s, w, C.c_void_p(self.tmp.data_ptr()), self.tmp.numel(), 0)
            assert 0 < n < self.tmp.numel()
            out[k] = self.tmp[:n].cpu().numpy().copy()
        return out


def both_sides(pix, run, buffers=True):
    """run() -> tuple of tensors, under TS_PIX_TABLES = 0 and = 1 on the same Work; returns (off, on) as (outputs, work buffer bits)."""
    res = []
    wb = WorkBuffers(pix) if buffers else None
    for mode in (0, 1):
        tables(pix, mode)
        if buffers:
            run()                      # the Work exists and has its final size: what is poisoned next is what the run writes
            wb.poison()
        out = tuple(_np(t) for t in run())
        res.append((out, wb.bits() if buffers else None))
    tables(pix, -1)
    return res


def assert_same(off, on, what):
    for i, (a, b) in enumerate(zip(off[0], on[0])):
        va, vb = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
        assert np.array_equal(va, vb), f"{what}: output {i} differs with the tables on"
    if off[1] is not None:
        for k in WORK:
            assert off[1][k].shape == on[1][k].shape
            diff = int((off[1][k] != on[1][k]).sum())
            assert diff == 0, f"{what}: work buffer {k} differs in {diff} of {off[1][k].size} words with the tables on"
        assert int((on[1]["OV0"] != SENT).sum()) > 0 and int((on[1]["Q1"] != SENT).sum()) > 0     # the runs did write them


def _inputs(B, rows, seed):
    rng = np.random.default_rng(seed)
    aud = torch.from_numpy(rng.standard_normal((B, rows, 256)).astype(F32)).cuda()
    label = torch.from_numpy(synth.speaker_ids(B)).cuda()
    return aud, label


@pytest.mark.parametrize("net", ["d32", "d64"])
@pytest.mark.parametrize("B", [1, 33, 64, 65])
@pytest.mark.parametrize("how", ["greedy", "philox"])
def test_full_decode(nets, net, B, how):
    """Codes, log-probabilities and the work buffers of a whole decode: 16-row tiles (1), ragged 32-row tiles (33), the coalesced engines' sizes
    (64, 65)."""
    from talkshow_amd import _lib
    pix = nets[net]
    aud, label = _inputs(B, H, 100 + B)
    kw = dict(mode=_lib.TS_SAMPLE_GREEDY) if how == "greedy" else dict(mode=_lib.TS_SAMPLE_PHILOX, seed=77, clip_index0=3)

    def run():
        codes, _, lp = pix.run(label, aud, logprobs=True, **kw)
        return codes, lp
    off, on = both_sides(pix, run)
    assert_same(off, on, f"{net} B={B} {how}")
    assert ((off[0][0] >= 0) & (off[0][0] < V)).all()


@pytest.mark.parametrize("net", ["d32", "d64"])
def test_mixed_lengths(nets, net):
    """Three lengths in one pass: 20 rows (two chunks and a half), 9 (one row into the second chunk), 1 (the shortest clip a pass takes)."""
    from talkshow_amd import _lib
    lib = _lib.load()
    pix = nets[net]
    rows = [20, 20, 9, 9, 9, 1, 1]
    B, Hm = len(rows), max(rows)
    lens = np.asarray([4 * h + (i % 4) for i, h in enumerate(rows)], np.int32)
    lens[::-1].sort()
    aud, label = _inputs(B, Hm, 5)
    lens_dev = torch.from_numpy(lens).cuda()

    def run(lens_host=lens):
        codes = torch.zeros((B, Hm, 2), dtype=torch.int64, device="cuda")
        lp = torch.empty((B, Hm, 2), dtype=torch.float32, device="cuda")
        rc = lib.ts_pixelcnn_generate_mixed_lp(pix.handle(), _lib.dptr(label), _lib.dptr(aud), lens_host.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, Hm,
                                               _lib.TS_SAMPLE_PHILOX, None, 19, None, _lib.dptr(codes), None, 0, _lib.dptr(lp), _lib.stream_ptr())
        assert rc == 0, lib.ts_last_error()
        return codes, lp
    off, on = both_sides(pix, run)
    assert_same(off, on, f"{net} mixed lengths")
    for b, h in enumerate(sorted(rows, reverse=True)):
        assert (on[0][0][b, h:] == -1).all() and (on[0][0][b, :h] >= 0).all()
    short = lens.copy()
    short[-1] = 3                                         # no code row at all: refused on both sides, before anything runs
    for mode in (0, 1):
        tables(pix, mode)
        codes = torch.zeros((B, Hm, 2), dtype=torch.int64, device="cuda")
        rc = lib.ts_pixelcnn_generate_mixed_lp(pix.handle(), _lib.dptr(label), _lib.dptr(aud), short.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, Hm,
                                               _lib.TS_SAMPLE_PHILOX, None, 19, None, _lib.dptr(codes), None, 0, None, _lib.stream_ptr())
        assert rc != 0 and b"shorter than 4 frames" in lib.ts_last_error()
    tables(pix, -1)


@pytest.mark.parametrize("net", ["d32", "d64"])
def test_continue_from_given_codes(nets, net):
    """A pass whose clips bring 0, 1, 3 and all 5 of their rows: the lookups read the given codes where the gather read them."""
    from talkshow_amd import _lib
    pix = nets[net]
    B = 4
    aud, label = _inputs(B, H, 9)
    rng = np.random.default_rng(3)
    given = [rng.integers(0, V, (g, 2)) for g in (0, 1, 3, 5)]

    def run():
        codes, _, lp = pix.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=5, given=given, logprobs=True)
        return codes, lp
    off, on = both_sides(pix, run)
    assert_same(off, on, f"{net} given codes")
    for b, g in enumerate(given):
        assert np.array_equal(on[0][0][b, :len(g)], g)


@pytest.mark.parametrize("net", ["d32", "d64"])
def test_two_chunk_streaming(nets, net):
    """A session of two steps (3 + 4 rows): rows 0 .. 2 of the first step have fewer rows above them, the second starts in a later ring phase;
    equal to the knob-off session and to the one-shot call."""
    from talkshow_amd import _lib
    pix = nets[net]
    B, h1, h2 = 3, 3, 4
    aud, label = _inputs(B, h1 + h2, 13)

    def run():
        st = pix.open_stream(label, B, 4)
        c0 = st.step(aud[:, :h1].contiguous(), mode=_lib.TS_SAMPLE_PHILOX, seed=8)
        c1 = st.step(aud[:, h1:].contiguous(), mode=_lib.TS_SAMPLE_PHILOX, seed=8)
        torch.cuda.synchronize()
        st.close()
        return c0, c1
    off, on = both_sides(pix, run, buffers=False)          # a session's Work is its own: the codes are what is compared
    assert_same(off, on, f"{net} streaming")
    tables(pix, 1)
    whole, _ = pix.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=8)
    tables(pix, -1)
    assert np.array_equal(np.concatenate(on[0], 1), _np(whole))


@pytest.mark.parametrize("B", [32, 65])
def test_shipped_size(shipped, B):
    """D = 256, V = 2048, 15 layers: K = 512 in 8 slices of 64 (V0), K = 256 in 8 slices of 32 (hg_0), tiled work buffers; 3 rows, so that
    row 2 reads a Q1 rider and writes both."""
    from talkshow_amd import _lib
    aud, label = _inputs(B, 3, 40 + B)

    def run():
        codes, _, lp = shipped.run(label, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=4, logprobs=True)
        return codes, lp
    off, on = both_sides(shipped, run)
    assert_same(off, on, f"shipped size B={B}")


def test_environment_knob(nets, tmp_path):
    """TS_PIX_TABLES=0 itself, read by a fresh process: the codes of the in-process decode with the tables on."""
    from talkshow_amd import _lib
    pix = nets["d64"]
    B = 33
    aud, label = _inputs(B, H, 100 + B)
    tables(pix, 1)
    codes, _ = pix.run(label, aud, mode=_lib.TS_SAMPLE_GREEDY)
    tables(pix, -1)
    script = tmp_path / "child.py"
    script.write_text(f"""
import sys, numpy as np, torch
sys.path.insert(0, {REPO!r}); sys.path.insert(0, {os.path.join(REPO, 'tests')!r})
import test_gpu_code_tables as T
from talkshow_amd import _lib
lib = _lib.load()
pix = T._make(T.SMALL["d64"], 11)
assert lib.ts_debug_pixelcnn_tables(pix.handle(), -2) == 0, "TS_PIX_TABLES=0 still built tables"
aud, label = T._inputs({B}, T.H, {100 + B})
codes, _ = pix.run(label, aud, mode=_lib.TS_SAMPLE_GREEDY)
np.save({str(tmp_path / 'codes.npy')!r}, codes.cpu().numpy())
""")
    env = dict(os.environ, TS_PIX_TABLES="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(tmp_path / "codes.npy"), _np(codes))


@pytest.mark.parametrize("net", ["d32", "d64"])
def test_lookup_launches_between_red_zones(nets, net):
    """Every buffer a lookup launch writes — pre-gate values, gated values, both riders (slot V0); gated values (hg_0) — between red zones at
    B = 33: zones intact, every element written, equal to the launch on tight allocations.  Codes include -1 (the zero row) and V - 1."""
    from test_gpu_poses_canary import run_both
    from talkshow_amd import _lib
    lib = _lib.load()
    pix = nets[net]
    tables(pix, 1)
    B, D = 33, SMALL[net]["dim"]
    rng = np.random.default_rng(B + D)
    tok = rng.integers(0, V, (B, 2)).astype(np.int32)
    tok[0], tok[1], tok[2], tok[B - 1] = (-1, 5), (7, -1), (-1, -1), (V - 1, V - 1)
    f = lambda *s: rng.standard_normal(s).astype(F32)
    ins = {"tok": (tok, torch.int32), "a1": (f(B, 4 * D), torch.float32), "a2": (f(B, 4 * D), torch.float32), "cls": (f(B, 2 * D), torch.float32)}
    f32 = torch.float32

    def v0(p, riders=True, terms=True):
        _lib.check(lib.ts_debug_code_table_stage(pix.handle(), 0, p["tok"], B, p["a1"] if terms else None, p["a2"] if terms else None, p["cls"],
                                                 p["pre"], p["out"], p["q1"] if riders else None, p["q0"] if riders else None, _lib.stream_ptr()))
    outs = {"pre": ((B, 4 * D), f32), "out": ((B, 2 * D), f32), "q1": ((B, 4 * D), f32), "q0": ((B, 4 * D), f32)}
    r = run_both(v0, ins, outs)
    assert np.isfinite(r["out"].view(F32)).all() and np.abs(r["out"].view(F32)).max() <= 1.0
    # a negative code is the zero row: with both codes negative a rider is +0.0 everywhere
    assert not r["q1"].reshape(B, 4 * D)[2].any() and not r["q0"].reshape(B, 4 * D)[2].any()
    # the last row of the grid writes no rider, the first rows read no Q terms
    r2 = run_both(lambda p: v0(p, riders=False, terms=False), ins, {k: outs[k] for k in ("pre", "out")})
    assert not np.array_equal(r2["pre"], r["pre"])

    ins_h = {"tok": (tok, torch.int32), "a1": (f(B, 2 * D), torch.float32), "cls": (f(B, 2 * D), torch.float32)}
    run_both(lambda p: _lib.check(lib.ts_debug_code_table_stage(pix.handle(), 1, p["tok"], B, p["a1"], None, p["cls"], None, p["out"], None, None,
                                                                _lib.stream_ptr())),
             ins_h, {"out": ((B, D), f32)})
    tables(pix, -1)
