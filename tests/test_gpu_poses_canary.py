"""Memory-safety witnesses for the entries of "given poses" (include/talkshow_hip.h), in the style of tests/test_gpu_canary.py: every
OUTPUT sits between 4 KiB red zones pre-filled (zones and body) with a sentinel, every INPUT between zones of NaN / an impossible length;
after the call the zones are intact, every documented element has lost the sentinel, and the outputs equal the same call on plain,
tightly allocated tensors bit for bit.  Shapes: B in {1, 33}, T_max in {31, 78}, ragged P_b.  Small networks (hid 128, 256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth

pytestmark = pytest.mark.gpu
PAD = 1024
F_SENT, I_SENT, L_SENT = 0x7FC0BEEF, 0x7EADBEEF7EADBEEF, 0x7EADBEEF
ITYPE = {torch.float32: torch.int32, torch.int64: torch.int64, torch.int32: torch.int32}
SENT = {torch.float32: F_SENT, torch.int64: I_SENT, torch.int32: L_SENT}


class Guarded:
    def __init__(self, shape, dtype, data=None):
        self.shape, self.dtype, self.n = tuple(shape), dtype, int(np.prod(shape))
        self.sent = SENT[dtype]
        self.raw = torch.full((2 * PAD + self.n,), self.sent, dtype=ITYPE[dtype], device="cuda")
        self.body = self.raw[PAD:PAD + self.n].view(dtype).view(self.shape)
        if data is not None:
            self.body.copy_(torch.as_tensor(np.ascontiguousarray(data)).to(dtype).reshape(self.shape))

    def ptr(self):
        return C.c_void_p(self.body.data_ptr())

    def zones_intact(self):
        return bool((self.raw[:PAD] == self.sent).all()) and bool((self.raw[PAD + self.n:] == self.sent).all())

    def bits(self):
        return self.raw[PAD:PAD + self.n].cpu().numpy().copy()


def run_both(call, ins, outs):
    """call(ptrs) enqueues the entry; ins: name -> (numpy, dtype); outs: name -> (shape, dtype).  Plain run, guarded run, the checks above."""
    res = []
    for guarded in (False, True):
        gi = {k: Guarded(a.shape, dt, a) for k, (a, dt) in ins.items()}
        go = {k: Guarded(s, dt) for k, (s, dt) in outs.items()}
        if not guarded:      # tight allocations: clones of the bodies
            tight = {k: g.body.clone() for k, g in {**gi, **go}.items()}
            ptrs = {k: C.c_void_p(t.data_ptr()) for k, t in tight.items()}
        else:
            ptrs = {k: g.ptr() for k, g in {**gi, **go}.items()}
        call(ptrs)
        torch.cuda.synchronize()
        if guarded:
            for k, g in {**gi, **go}.items():
                assert g.zones_intact(), f"{k}: a store landed in a red zone"
            for k, g in gi.items():
                assert np.array_equal(g.bits(), Guarded(g.shape, g.dtype, ins[k][0]).bits()), f"input {k} was modified"
            res.append({k: g.bits() for k, g in go.items()})
        else:
            res.append({k: tight[k].view(ITYPE[outs[k][1]]).reshape(-1).cpu().numpy() for k in outs})
    for k, (shape, dt) in outs.items():
        assert np.array_equal(res[0][k], res[1][k]), f"output {k}: the call between red zones differs from the plain call"
        left = int((res[1][k] == np.asarray(SENT[dt]).astype(res[1][k].dtype)).sum())
        assert left == 0, f"output {k}: {left} elements were never written"
    return res[1]


@pytest.fixture(scope="module")
def nets():
    from talkshow_amd.modules import AudioEncoder, GatedPixelCNN, VQVAE
    dims = dict(input_dim=256, dim=64, n_layers=3)
    vb, vh = VQVAE(39, 64, 256, 128, 2).cuda(), VQVAE(90, 64, 256, 128, 2).cuda()
    vb.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=256, num_hiddens=128)))
    vh.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=90, num_embeddings=256, num_hiddens=128, salt=1)))
    ae = AudioEncoder(64, 256, 2).cuda()
    ae.load_state_dict(synth.to_torch(synth.audioencoder_state_dict(seed=3)))
    px = GatedPixelCNN(dims["input_dim"], dims["dim"], dims["n_layers"], 4, True, True).cuda()
    px.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=3, **dims)))
    return ae, px, vb, vh


def _ragged(B, T_max, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(4, T_max + 1, B).astype(np.int32)
    lens[0] = T_max
    if B > 2:
        lens[1], lens[2] = 4, 7
    return lens


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_mixed_encode_and_reconstruction(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    _, _, vb, vh = nets
    lens = _ragged(B, T_max, B + T_max)
    poses = synth.gt_poses(40 + B, B, T_max)
    for b in range(B):
        poses[b, lens[b]:] = np.nan                 # never read
    H = T_max // 4
    ins = {"poses": (poses, torch.float32), "lens": (lens, torch.int32)}

    def enc(p):
        _lib.check(lib.ts_vqvae_encode_pair_masked(vb.handle(), vh.handle(), p["poses"], 129, p["lens"], B, T_max, p["codes"], p["zb"], p["zh"],
                                                   _lib.stream_ptr()))
    r = run_both(enc, ins, {"codes": ((B, H, 2), torch.int64), "zb": ((B, H, 64), torch.float32), "zh": ((B, H, 64), torch.float32)})
    codes = r["codes"].reshape(B, H, 2)
    for b in range(B):
        assert np.all(codes[b, lens[b] // 4:] == -1) and np.all((codes[b, :lens[b] // 4] >= 0) & (codes[b, :lens[b] // 4] < 256))
        assert np.all(r["zb"].reshape(B, H, 64)[b, lens[b] // 4:] == 0) and np.all(r["zh"].reshape(B, H, 64)[b, lens[b] // 4:] == 0)

    def rec(p):
        _lib.check(lib.ts_body_vq_infer_mixed(vb.handle(), vh.handle(), p["poses"], p["lens"], B, T_max, p["codes"], p["recon"], _lib.stream_ptr()))
    r2 = run_both(rec, ins, {"codes": ((B, H, 2), torch.int64), "recon": ((B, 4 * H, 129), torch.float32)})
    assert np.array_equal(r2["codes"], r["codes"])
    recon = r2["recon"].view(np.float32).reshape(B, 4 * H, 129)
    for b in range(B):
        assert np.all(recon[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(recon[b, :4 * (lens[b] // 4)]).all()


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    lens = np.sort(_ragged(B, T_max, 7 * B + T_max))[::-1].copy()                  # the pass wants its clips longest first
    rng = np.random.default_rng(B * T_max)
    plens = np.asarray([int(rng.choice([0, 4, 4 * (t // 4) // 2 + 1, 4 * (t // 4) + 3])) for t in lens], np.int32)
    plens[0] = 4 * (T_max // 4)                                                    # every row of the longest clip given
    plens = np.where(plens // 4 > lens // 4, 4 * (lens // 4), plens).astype(np.int32)
    plens[(plens > 0) & (plens < 4)] = 4
    P_max = int(plens.max())
    gp = synth.gt_poses(60 + B, B, P_max)
    for b in range(B):
        gp[b, plens[b]:] = np.nan
    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan
    ids = (np.arange(B) % 4).astype(np.int64)
    H = T_max // 4
    i32p = C.POINTER(C.c_int32)
    ins = {"mfcc": (mf, torch.float32), "ids": (ids, torch.int64), "lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64),
           "gp": (gp, torch.float32), "plens": (plens, torch.int32)}

    def run(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_poses(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"], lens.ctypes.data_as(i32p),
                                                       p["lens"], B, T_max, _lib.TS_SAMPLE_PHILOX, None, 5, p["clip"], p["codes"], p["poses"], None, 0,
                                                       p["lp"], p["gp"], P_max, plens.ctypes.data_as(i32p), p["plens"], _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    codes = r["codes"].reshape(B, H, 2)
    # the given rows are the mixed encode's codes of the same frames
    enc = torch.empty((B, P_max // 4, 2), dtype=torch.int64, device="cuda")
    gpd, pld = torch.from_numpy(np.nan_to_num(gp)).cuda(), torch.from_numpy(plens).cuda()
    _lib.check(lib.ts_vqvae_encode_pair_masked(vb.handle(), vh.handle(), _lib.dptr(gpd), 129, _lib.dptr(pld), B, P_max, _lib.dptr(enc), None, None,
                                               _lib.stream_ptr()))
    enc = enc.cpu().numpy()
    for b in range(B):
        g, h = plens[b] // 4, lens[b] // 4
        assert np.array_equal(codes[b, :g], enc[b, :g]) and np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < 256))
