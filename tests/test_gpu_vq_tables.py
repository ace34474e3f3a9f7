"""The VQ decoders' first Winograd-lowered layer from per-code tables (csrc/conv_wino.hip::wino_codes, models.cpp::ts_vqvae_create and
run_stack_wino; knob TS_VQ_DEC_TABLES).  _dec_1's first layer multiplies nothing but rows of the 'aft_vq' table, so its six GEMMs are done
once per network over all codes (T_i = aft_table U_i^T) and a decode from codes reads T_i rows where it ran wino_in and the GEMMs.

1. the kernel against a numpy restatement of its pinned order on the network's own tables, bit for bit: 1, 3, 4, 5, 8, 13 code rows (less
   than a tile, every length mod 4, tiles with both neighbours), a negative code, a code past the table, a masked pass (a clip with all its
   rows, a part, none), both networks in one launch; the O buffer between sentinel zones and sentinel-filled (tests/test_gpu_wino.py::Zoned)
2. the table entries against float64 aft_table U_i^T
3. a decode with the tables against the knob off (child process: the knob is read once per process) and both against float64
4. a seamless session against the one-shot call with the tables on, bit for bit
5. the transform kernels on the plain grid (TS_WINO_DEAL=0) against the same restatements
Mixed against alone and paired against single decodes of this width run in tests/test_gpu_wino.py with the tables on (the default).

Networks: hid = 512 (the narrowest width lowered by default), 256 codes, 2 residual layers, B <= 5."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

F32, F64 = np.float32, np.float64
HID, NCODE = 512, 256
LENGTHS = (1, 3, 4, 5, 8, 13)
pytestmark = pytest.mark.gpu


def make_pair():
    from talkshow_amd import synth
    from talkshow_amd.modules import VQVAE
    sds = [synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=NCODE, num_hiddens=HID),
           synth.vqvae_state_dict(seed=3, in_dim=90, num_embeddings=NCODE, num_hiddens=HID, salt=1)]
    nets = [VQVAE(39, 64, NCODE, HID, 2).cuda(), VQVAE(90, 64, NCODE, HID, 2).cuda()]
    for n, sd in zip(nets, sds):
        n.load_state_dict(synth.to_torch(sd))
    return nets, sds


def decode_inputs():
    rng = np.random.default_rng(17)
    return rng.integers(0, NCODE, (2, 5, 13)).astype(np.int64)


def decode_pair(nets):
    """the two decodes of test 3 -> (5, 52, 129)"""
    lat = decode_inputs()
    return np.concatenate([n.decode_nlc(torch.from_numpy(lat[i]).cuda()).cpu().numpy() for i, n in enumerate(nets)], -1)


if __name__ == "__main__":                                  # the child of test 3: the same decodes under this process's knobs
    np.save(sys.argv[1], decode_pair(make_pair()[0]))
    sys.exit(0)


from test_gpu_wino import Zoned, dev  # noqa: E402
from test_wino_host import bt_rows  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load(), _lib.context(0)


@pytest.fixture(scope="module")
def pair(hip):
    """the two networks and, per network, the tables, the aft_vq table and the first layer's Winograd matrices as the device holds them"""
    _lib, lib, ctx = hip
    nets, sds = make_pair()
    tabs = []
    for n in nets:
        T, aft, U = np.empty((6, NCODE, HID), F32), np.empty((NCODE, HID), F32), np.empty((6, HID, HID), F32)
        p = C.c_void_p()
        assert lib.ts_debug_vqvae_dec_tables(n.handle(), T.ctypes.data, aft.ctypes.data, U.ctypes.data, C.byref(p)) == 1, "tables are on by default"
        tabs.append(dict(T=T, aft=aft, U=U, dev=p.value))
    return nets, sds, tabs


def codes_o_np(codes, T, Lb):
    """codes (B, L) -> O (6, B J, C): O_i = row i of Bt over the rows T_i[code], conv_wino.hip's order; zero rows outside [0, L_b) and for a
    code outside the table"""
    B, L = codes.shape
    ncode, Cc = T.shape[1:]
    J = (L + 3) // 4
    cp = np.full((B, 4 * J + 2), ncode, np.int64)                                   # row t of the clip at index t + 1; ncode = the zero row
    for b in range(B):
        c = codes[b, :Lb[b]]
        cp[b, 1:1 + Lb[b]] = np.where((c >= 0) & (c < ncode), c, ncode)
    out = []
    for i in range(6):
        Ti = np.concatenate([T[i], np.zeros((1, Cc), F32)])
        out.append(bt_rows([Ti[cp[:, k:k + 4 * J:4]] for k in range(6)])[i].reshape(B * J, Cc))
    return np.stack(out).astype(F32)


def run_codes(hip, codes, tabs, lens=None, shr=0, shl=0):
    """one launch over len(tabs) networks; codes (nnet, B, L) -> the O of each network, zones checked"""
    _lib, lib, ctx = hip
    nnet, B, L = codes.shape
    J = (L + 3) // 4
    cd = [dev(codes[i]) for i in range(nnet)]
    Os = [Zoned(6 * B * J * HID) for _ in range(nnet)]
    two = nnet == 2
    _lib.check(lib.ts_debug_wino_codes(ctx, nnet, B, L, HID, _lib.dptr(lens), shr, shl, cd[0].data_ptr(), cd[1].data_ptr() if two else None,
                                       tabs[0]["dev"], tabs[1]["dev"] if two else None, NCODE, NCODE if two else 0,
                                       Os[0].ptr(), Os[1].ptr() if two else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return [o.check("O").reshape(6, B * J, HID) for o in Os]


def test_table_kernel_equals_the_restatement_bit_for_bit(hip, pair):
    _, _, tabs = pair
    rng = np.random.default_rng(1)
    B = 3
    for L in LENGTHS:
        codes = rng.integers(0, NCODE, (1, B, L)).astype(np.int64)
        codes[0, 1, L // 2] = -1                                                    # a negative code: the zero row
        codes[0, 2, L - 1] = NCODE                                                  # past the table: the zero row, nothing read
        (O,) = run_codes(hip, codes, tabs[:1])
        assert np.array_equal(O.view(np.uint32), codes_o_np(codes[0], tabs[0]["T"], [L] * B).view(np.uint32)), L
    # a masked pass, as the decoder masks its first stack (lens >> 2 code rows): all of a clip's rows, a part, none; the rows beyond a
    # clip's own hold what no table has and are not read
    for L in (5, 13):
        lens_h = np.array([4 * L + 3, 4 * (L // 2) + 1, 2], np.int32)
        Lb = [min(L, int(n) >> 2) for n in lens_h]
        codes = rng.integers(0, NCODE, (1, B, L)).astype(np.int64)
        for b in range(B):
            codes[0, b, Lb[b]:] = 1 << 40
        (O,) = run_codes(hip, codes, tabs[:1], lens=dev(lens_h), shr=2)
        assert np.array_equal(O.view(np.uint32), codes_o_np(codes[0], tabs[0]["T"], Lb).view(np.uint32)), ("masked", L)
        J = (L + 3) // 4
        assert np.all(O.reshape(6, B, J, HID)[:, 2] == 0)
    # both networks in one launch = each alone.  The launch deals its 2 x (B J 128 / 256) workgroups to the 8 XCDs in contiguous runs
    # (wino_item): 20 workgroups (a remainder of 4, the second network starting inside a run), 6 (fewer than XCDs), 16 (no remainder)
    for Bp, L, total in ((5, 13, 20), (3, 5, 6), (4, 16, 16)):
        assert 2 * ((Bp * ((L + 3) // 4) * (HID // 4) + 255) // 256) == total
        codes = rng.integers(0, NCODE, (2, Bp, L)).astype(np.int64)
        for i, O in enumerate(run_codes(hip, codes, tabs)):
            assert np.array_equal(O.view(np.uint32), codes_o_np(codes[i], tabs[i]["T"], [L] * Bp).view(np.uint32)), ("pair", i, Bp, L)


def test_table_entries_against_float64(pair):
    """T_i[code] = aft_table[code] . U_i rows, an fp32 dot product of K = 512 terms in an order of the engine's choosing: whatever the order,
    |error| <= gamma_K sum_k |a_k u_k| with gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability, 3.1).  The error the
    tables were measured at is printed beside it."""
    _, _, tabs = pair
    u = 2.0 ** -24
    gamma = HID * u / (1 - HID * u)
    for i, t in enumerate(tabs):
        a, U = t["aft"].astype(F64), t["U"].astype(F64)
        ref = np.einsum("nk,iok->ino", a, U)
        bound = gamma * np.einsum("nk,iok->ino", np.abs(a), np.abs(U))
        err = np.abs(t["T"].astype(F64) - ref)
        print(f"\n[measured] dec tables net {i}: max |err| = {err.max():.3e}, max |T| = {np.abs(ref).max():.3e}, max err / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound)


def test_decode_with_tables_against_knob_off_and_float64(pair, tmp_path):
    """The tables round otherwise than wino_in and the GEMMs: the decode moves within fp32 rounding.  Both paths against the float64 network
    (oracle/torch_port.py) on the same codes, inside the 2e-5 of DESIGN.md 4 (the synthetic networks' poses are of unit scale: asserted);
    the difference between the two paths is printed."""
    from oracle import torch_port as tp
    nets, sds, _ = pair
    lat = decode_inputs()
    on = decode_pair(nets)
    out = str(tmp_path / "off.npy")
    env = dict(os.environ, TS_VQ_DEC_TABLES="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    off = np.load(out)
    ref = []
    with torch.no_grad():
        for i, sd in enumerate(sds):
            sd64 = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items() if isinstance(v, np.ndarray)}
            ref.append(tp.vqvae_decode(torch.from_numpy(lat[i]), sd64).transpose(1, 2).numpy())
    ref = np.concatenate(ref, -1)
    e_on, e_off = float(np.abs(on - ref).max()), float(np.abs(off - ref).max())
    print(f"\n[measured] decode hid {HID}: tables {e_on:.3e}, knob off {e_off:.3e} against float64 (max |pose| {np.abs(ref).max():.3f}); "
          f"tables against knob off {float(np.abs(on.astype(F64) - off).max()):.3e}, {int((on != off).sum())} of {on.size} words differ")
    assert on.shape == off.shape == ref.shape == (5, 52, 129)
    assert 0.1 <= float(np.abs(ref).max()) <= 1.0
    assert e_on <= 2e-5 and e_off <= 2e-5
    assert np.any(on != off), "the knob changed nothing: the child did not run the GEMM path"


def test_seamless_session_equals_one_shot_with_tables(hip, pair):
    """A seamless session in chunks against generate_batch on the whole audio, VQ decoders of 512 hidden channels with their tables:
    codes equal, poses equal as bits (a tile of the table kernel reads the codes wino_in's tile read rows of)."""
    from nets.smplx_body_pixel import TrainWrapper
    from talkshow_amd import synth
    from talkshow_amd.modules import AudioEncoder, GatedPixelCNN
    from test_gpu_seamless import _bits, draw, streamed
    nets, _, _ = pair
    input_dim, dim, n_layers, n_cls, seed = NCODE, 64, 4, 4, 7                     # the pix_small golden's PixelCNN, 256 codes wide
    w = object.__new__(TrainWrapper)
    w.generator = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    w.generator.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    w.audioencoder = AudioEncoder(64, 256, 2).cuda()
    w.audioencoder.load_state_dict(synth.to_torch(synth.audioencoder_state_dict(seed=3)))
    w.g_body, w.g_hand = nets
    w.each_dim, w.num_classes = [0, 39, 90], n_cls
    B, T = 3, 150
    mf = torch.from_numpy(synth.mfcc_features(41, B, T)).cuda()
    ids = np.arange(B) % n_cls
    ref_codes, ref_poses = w.generate_batch(mf, ids, **draw("philox"))
    for sched in ((64, 86), (37, 3, 110)):
        codes, poses = streamed(w, mf, ids, sched, "philox")
        assert np.array_equal(codes, _bits(ref_codes)) and np.array_equal(poses, _bits(ref_poses)), sched


def test_transform_kernels_on_the_plain_grid():
    """The four transform kernels deal their workgroups to the XCDs in contiguous runs where the device passed ts_ctx_create's probe (the
    default, which every other test runs) and take a plain (blocks, networks) grid otherwise or under TS_WINO_DEAL=0: the same bits.  The
    knob is read once per process, so the bit-for-bit tests of the kernels run again in a child process."""
    here = os.path.abspath(__file__)
    env = dict(os.environ, TS_WINO_DEAL="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(os.path.dirname(here), "test_gpu_wino.py") + "::test_transforms_equal_the_restatement_bit_for_bit",
                        here + "::test_table_kernel_equals_the_restatement_bit_for_bit", "-m", "gpu", "-x", "-q"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
