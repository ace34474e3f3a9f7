"""Memory-safety witnesses for the three pass entries of "kept positions" (include/talkshow_hip.h), in the style of
tests/test_gpu_poses_canary.py: the mask, the given block and the uniforms sit between red zones, every OUTPUT sits between red zones
pre-filled (zones and body) with a sentinel; after the call the zones are intact, the inputs are unmodified, every documented element has
lost the sentinel, and the outputs equal the same call on plain, tightly allocated tensors bit for bit.  What the rule says is never read
holds poison: given codes of unkept positions and of rows at or beyond G_b (-7, 2**40), uniforms of kept positions (NaN), mask bytes at or
beyond G_b (0xA5).  Shapes: B in {1, 33}, T_max in {31, 78}, ragged lengths.  Small networks (hid 128, 256 codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import ITYPE, SENT, _ragged, run_both

pytestmark = pytest.mark.gpu
ITYPE.setdefault(torch.uint8, torch.uint8)
SENT.setdefault(torch.uint8, 0xA5)
I32P = C.POINTER(C.c_int32)
V = 256


@pytest.fixture(scope="module")
def nets():
    from talkshow_amd.modules import AudioEncoder, GatedPixelCNN, VQVAE
    dims = dict(input_dim=V, dim=64, n_layers=3)
    vb, vh = VQVAE(39, 64, 256, 128, 2).cuda(), VQVAE(90, 64, 256, 128, 2).cuda()
    vb.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=256, num_hiddens=128)))
    vh.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=90, num_embeddings=256, num_hiddens=128, salt=1)))
    ae = AudioEncoder(64, 256, 2).cuda()
    ae.load_state_dict(synth.to_torch(synth.audioencoder_state_dict(seed=3)))
    px = GatedPixelCNN(dims["input_dim"], dims["dim"], dims["n_layers"], 4, True, True).cuda()
    px.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=3, **dims)))
    return ae, px, vb, vh


def _case(B, T_max, seed):
    """Lengths longest first, G_b (0, H_b and values between), a random mask, and the poisoned block / uniforms / mask of the rule."""
    rng = np.random.default_rng(seed)
    lens = np.sort(_ragged(B, T_max, seed))[::-1].copy()
    H = T_max // 4
    rows = lens // 4
    G = np.asarray([int(rng.choice([0, 1, (h + 1) // 2, h])) for h in rows], np.int32)
    G[0] = rows[0]
    keep = rng.integers(0, 2, (B, H, 2)).astype(np.uint8)
    given = rng.integers(0, V, (B, H, 2)).astype(np.int64)
    u = rng.random((B, H, 2)).astype(np.float32)
    poison = np.where(rng.random((B, H, 2)) < 0.5, -7, 2 ** 40)
    for b in range(B):
        kept = np.zeros((H, 2), bool)
        kept[:G[b]] = keep[b, :G[b]] != 0
        given[b][~kept] = poison[b][~kept]
        u[b][kept] = np.nan
        keep[b, G[b]:] = 0xA5
    return lens, G, keep, given, u


def _check(codes, lens, G, keep, given, B):
    for b in range(B):
        h, g = lens[b] // 4, G[b]
        assert np.all(codes[b, h:] == -1) and np.all((codes[b, :h] >= 0) & (codes[b, :h] < V))
        kept = keep[b, :g] != 0
        assert np.array_equal(codes[b, :g][kept], given[b, :g][kept])


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_chain_and_body_entries(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    lens, G, keep, given, u = _case(B, T_max, 5 * B + T_max)
    H = T_max // 4
    aud = np.random.default_rng(B + T_max).standard_normal((B, H, 256)).astype(np.float32)
    ids = (np.arange(B) % 4).astype(np.int64)
    common = {"ids": (ids, torch.int64), "lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64),
              "given": (given, torch.int64), "keep": (keep, torch.uint8), "u": (u, torch.float32)}

    def chain(p):
        _lib.check(lib.ts_pixelcnn_generate_mixed_keep(px.handle(), p["ids"], p["aud"], lens.ctypes.data_as(I32P), p["lens"], B, H,
                                                       _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], None, 0, p["lp"], p["given"],
                                                       G.ctypes.data_as(I32P), None, p["keep"], _lib.stream_ptr()))
    r = run_both(chain, dict(common, aud=(aud, torch.float32)), {"codes": ((B, H, 2), torch.int64), "lp": ((B, H, 2), torch.float32)})
    _check(r["codes"].reshape(B, H, 2), lens, G, keep, given, B)
    lp = r["lp"].view(np.float32).reshape(B, H, 2)
    for b in range(B):
        assert np.all(lp[b, lens[b] // 4:] == 0) and np.isfinite(lp[b, :lens[b] // 4]).all()

    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan

    def body(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_keep(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"], lens.ctypes.data_as(I32P),
                                                      p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"], p["codes"], p["poses"], None, 0,
                                                      p["lp"], p["given"], G.ctypes.data_as(I32P), None, p["keep"], _lib.stream_ptr()))
    r2 = run_both(body, dict(common, mfcc=(mf, torch.float32)),
                  {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    _check(r2["codes"].reshape(B, H, 2), lens, G, keep, given, B)
    poses = r2["poses"].view(np.float32).reshape(B, 4 * H, 129)
    for b in range(B):
        assert np.all(poses[b, 4 * (lens[b] // 4):] == 0) and np.isfinite(poses[b, :4 * (lens[b] // 4)]).all()


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("T_max", [31, 78])
def test_pass_from_poses(nets, B, T_max):
    from talkshow_amd import _lib
    lib = _lib.load()
    ae, px, vb, vh = nets
    lens, G, keep, _, u = _case(B, T_max, 9 * B + T_max)
    H = T_max // 4
    plens = np.asarray([0 if g == 0 else 4 * g + (b % 4) for b, g in enumerate(G)], np.int32)      # G_b = P_b / 4
    P_max = int(plens.max())
    gp = synth.gt_poses(60 + B, B, P_max)
    for b in range(B):
        gp[b, plens[b]:] = np.nan
    mf = synth.mfcc_features(80 + B, B, T_max)
    for b in range(B):
        mf[b, lens[b]:] = np.nan
    ids = (np.arange(B) % 4).astype(np.int64)
    ins = {"mfcc": (mf, torch.float32), "ids": (ids, torch.int64), "lens": (lens, torch.int32), "clip": (np.arange(B, dtype=np.int64), torch.int64),
           "gp": (gp, torch.float32), "plens": (plens, torch.int32), "keep": (keep, torch.uint8), "u": (u, torch.float32)}

    def run(p):
        _lib.check(lib.ts_body_pixel_infer_mixed_poses_keep(ae.handle(), px.handle(), vb.handle(), vh.handle(), p["mfcc"], p["ids"],
                                                            lens.ctypes.data_as(I32P), p["lens"], B, T_max, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, p["clip"],
                                                            p["codes"], p["poses"], None, 0, p["lp"], p["gp"], P_max, plens.ctypes.data_as(I32P),
                                                            p["plens"], p["keep"], _lib.stream_ptr()))
    r = run_both(run, ins, {"codes": ((B, H, 2), torch.int64), "poses": ((B, 4 * H, 129), torch.float32), "lp": ((B, H, 2), torch.float32)})
    codes = r["codes"].reshape(B, H, 2)
    enc = torch.empty((B, P_max // 4, 2), dtype=torch.int64, device="cuda")
    gpd, pld = torch.from_numpy(np.nan_to_num(gp)).cuda(), torch.from_numpy(plens).cuda()
    _lib.check(lib.ts_vqvae_encode_pair_masked(vb.handle(), vh.handle(), _lib.dptr(gpd), 129, _lib.dptr(pld), B, P_max, _lib.dptr(enc), None, None,
                                               _lib.stream_ptr()))
    enc = np.concatenate([enc.cpu().numpy(), np.zeros((B, H - P_max // 4, 2), np.int64)], 1)
    _check(codes, lens, G, keep, enc, B)
