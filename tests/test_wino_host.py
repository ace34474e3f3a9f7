"""Host-side checks of the Winograd F(4,3) lowering of the wide stride-1 k = 3 C -> C layers (csrc/conv_wino.hip, csrc/models.cpp): which
layers are lowered, the transformed weights, the algebra of the committed matrices, and the numerics of lowered VQ-VAEs on the CPU port.
No GPU: the GPU side is tests/test_gpu_wino.py, which imports the restatements below."""
import ctypes as C

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
# the standard F(4,3) matrices, interpolation points 0, +-1, +-2, inf (csrc/conv_wino.hip)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], F64)
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], F64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], F64)


# ----------------------------------------------------------------------------------------------- restatements (fp32, the kernels' order)
def bt_rows(d):
    """Bt d with the summation order written down in csrc/conv_wino.hip: d = six fp32 arrays -> six fp32 arrays, one rounding per operation."""
    f = F32
    d0, d1, d2, d3, d4, d5 = d
    return [(f(4) * d0 - f(5) * d2) + d4,
            ((d3 - f(4) * d1) - f(4) * d2) + d4,
            ((f(4) * d1 - f(4) * d2) - d3) + d4,
            ((f(2) * d3 - f(2) * d1) - d2) + d4,
            ((f(2) * d1 - d2) - f(2) * d3) + d4,
            (f(4) * d1 - f(5) * d3) + d5]


def at_rows(m):
    f = F32
    m0, m1, m2, m3, m4, m5 = m
    return [(((m0 + m1) + m2) + m3) + m4,
            ((m1 - m2) + f(2) * m3) - f(2) * m4,
            ((m1 + m2) + f(4) * m3) + f(4) * m4,
            (((m1 - m2) + f(8) * m3) - f(8) * m4) + m5]


def act32(v, act):
    if act == 1:
        return np.where(v >= 0, v, v * F32(0.2)).astype(F32)
    if act == 2:
        return np.where(v > 0, v, F32(0)).astype(F32)
    assert act == 0
    return v


def clip_rows(L, lens, shr, shl):
    return None if lens is None else [min(L, (int(n) >> shr) << shl) for n in lens]


def wino_in_np(x, lens=None, shr=0, shl=0):
    """x (B, L, C) fp32 -> V (6, B J, C): rows outside [0, L_b) of a clip read as zeros."""
    B, L, Cc = x.shape
    J = (L + 3) // 4
    Lb = clip_rows(L, lens, shr, shl) or [L] * B
    xp = np.zeros((B, 4 * J + 2, Cc), F32)                  # row t of the clip at index t + 1
    for b in range(B):
        xp[b, 1:1 + Lb[b]] = x[b, :Lb[b]]
    d = [xp[:, k:k + 4 * J:4] for k in range(6)]            # d_k[b][j] = x[b][4j - 1 + k]
    return np.stack([v.reshape(B * J, Cc) for v in bt_rows(d)]).astype(F32)


def wino_y_np(O, bias, B, L, act, res=None, lens=None, shr=0, shl=0):
    """O (6, B J, C) -> y (B, L, C) = act(At O + bias (+ res)), rows in [L_b, L) zero."""
    J = (L + 3) // 4
    Cc = O.shape[-1]
    rows = at_rows([O[i].reshape(B, J, Cc) for i in range(6)])
    y = np.stack(rows, 2).reshape(B, 4 * J, Cc)[:, :L]
    v = y + bias.astype(F32)
    if res is not None:
        v = v + res
    v = act32(v.astype(F32), act)
    Lb = clip_rows(L, lens, shr, shl)
    if Lb is not None:
        for b in range(B):
            v[b, Lb[b]:] = 0
    return np.ascontiguousarray(v, F32)


def wino_weights64(w):
    """U (6, cout, cin) float64 of taps w (cout, cin, 3)."""
    return np.einsum("ik,ock->ioc", G, w.astype(F64))


def conv64(x, w, bias):
    """float64 direct convolution, stride 1, padding 1: x (B, L, C), w (cout, cin, 3) -> (B, L, cout)."""
    B, L, _ = x.shape
    xp = np.zeros((B, L + 2, x.shape[2]), F64)
    xp[:, 1:-1] = x
    return sum(xp[:, k:k + L] @ w[:, :, k].astype(F64).T for k in range(3)) + bias.astype(F64)


# ----------------------------------------------------------------------------------------------- tests
def _lowering(lib, cin, cout, k, stride, knobs):
    out = (C.c_int * 5)()
    r = lib.ts_debug_wino_lowering(cin, cout, k, stride, knobs.encode() if knobs else None, 256, 75, out)
    return r, list(out)


def network_layers(in_dim, hid, decoder, emb=64, nres=2):
    """(name, cin, cout, k, stride) of every conv layer of an encoder trunk [+ the VQ-VAE's own layers] (vqvae_1d.py)."""
    ls = [("project", in_dim, hid // 4, 3, 1)]
    for name, c in (("_enc_1", hid // 4), ("_enc_2", hid // 2), ("_enc_3", hid)):
        ls += [(f"{name}.{i}", c, c, 3, 1) for i in range(nres + 1)]
        if c < hid:
            ls.append((f"_down after {name}", c, 2 * c, 4, 2))
    if decoder:
        ls += [("pre_vq_conv", hid, emb, 1, 1), ("aft_vq_conv", emb, hid, 1, 1)]
        for name, c in (("_dec_1", hid), ("_dec_2", hid // 2), ("_dec_3", hid // 4)):
            ls += [(f"{name}.{i}", c, c, 3, 1) for i in range(nres + 1)]
            if c > hid // 4:
                ls.append((f"_up after {name}", c, c // 2, 4, 2))
        ls.append(("decoder.project", hid // 4, in_dim, 1, 1))
    return ls


def test_eligibility_of_every_layer():
    """Lowered by the layer's own geometry only: k = 3, stride 1, Cin = Cout, no channel padding, and at least 512 wide by default."""
    from talkshow_amd import _lib
    lib = _lib.load()
    nets = {"body": network_layers(39, 1024, True), "hand": network_layers(90, 1024, True), "audio": network_layers(64, 256, False)}
    for net, layers in nets.items():
        for name, cin, cout, k, stride in layers:
            geom = k == 3 and stride == 1 and cin == cout and cin % 32 == 0
            for knobs, want in ((None, geom and cout >= 512), ("TS_CONV_WINO=-1", geom and cout >= 512), ("TS_CONV_WINO=0", False),
                                ("TS_CONV_WINO=1", geom)):
                r, out = _lowering(lib, cin, cout, k, stride, knobs)
                assert r == int(want), (net, name, knobs, r)
                if want:
                    assert out == [6, 256 * 19, cout, cin, 4], (net, name, out)
    # the default set is exactly _enc_2, _enc_3, _dec_1, _dec_2 of the VQ-VAEs; nothing of the audio encoder
    on = [n for n, cin, cout, k, s in nets["body"] if _lowering(lib, cin, cout, k, s, None)[0] == 1]
    assert on == [f"{st}.{i}" for st in ("_enc_2", "_enc_3", "_dec_1", "_dec_2") for i in range(3)]
    assert not [n for n, cin, cout, k, s in nets["audio"] if _lowering(lib, cin, cout, k, s, None)[0] == 1]
    # the answer does not depend on the batch or the length
    out = (C.c_int * 5)()
    assert {lib.ts_debug_wino_lowering(512, 512, 3, 1, None, B, L, out) for B in (1, 3, 256) for L in (1, 5, 75, 300)} == {1}
    assert lib.ts_debug_wino_lowering(512, 512, 3, 1, None, 3, 5, out) == 1 and list(out) == [6, 6, 512, 512, 4]


def test_transformed_weights_against_float64():
    from talkshow_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for cout, cin in ((64, 64), (160, 96)):
        w = rng.standard_normal((cout, cin, 3)).astype(F32)
        npad = (cout + 127) // 128 * 128
        out = np.full((6, npad, cin), np.nan, F32)
        assert lib.ts_debug_wino_weights(w.ctypes.data, cout, cin, out.ctypes.data) == 0
        ref = wino_weights64(w)
        # computed in double and rounded once: within half an fp32 ulp of the float64 value (the double sums may differ in their last bits)
        half_ulp = 0.5 * np.spacing(np.abs(ref).astype(F32)).astype(F64)
        assert np.all(np.abs(out[:, :cout].astype(F64) - ref) <= half_ulp * (1 + 1e-6))
        assert np.all(out[:, cout:] == 0)


def test_matrices_compute_the_convolution():
    """At [(G g) . (Bt d)] = the four outputs of the 3-tap correlation of d with g, in float64, for the committed matrices."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        g, d = rng.standard_normal(3), rng.standard_normal(6)
        y = AT @ ((G @ g) * (BT @ d))
        ref = np.array([d[r] * g[0] + d[r + 1] * g[1] + d[r + 2] * g[2] for r in range(4)])
        np.testing.assert_allclose(y, ref, rtol=0, atol=1e-13)
    # and the restatements the GPU tests use are these matrices
    d = [rng.standard_normal(7).astype(F32) for _ in range(6)]
    np.testing.assert_allclose(np.stack(bt_rows(d)), BT @ np.stack(d).astype(F64), rtol=0, atol=2e-5)
    np.testing.assert_allclose(np.stack(at_rows(d)), AT @ np.stack(d).astype(F64), rtol=0, atol=2e-5)
    # wino_in / wino_y restatements on whole clips, through exact float64 products: the convolution, for every L mod 4 and L < 4
    for L in (1, 2, 3, 4, 5, 6, 7, 19):
        x = rng.standard_normal((2, L, 8)).astype(F32)
        w = rng.standard_normal((8, 8, 3)).astype(F32)
        V = wino_in_np(x).astype(F64)
        O = np.einsum("imc,ioc->imo", V, wino_weights64(w))
        y = wino_y_np(O.astype(F32), np.zeros(8, F32), 2, L, 0)
        np.testing.assert_allclose(y, conv64(x, w, np.zeros(8)), rtol=0, atol=5e-5)


class _WinoF:
    """torch.nn.functional with conv1d replaced, for eligible layers, by the fp32 F(4,3) form (weights transformed in float64, rounded once)."""

    def __init__(self, min_c=512):
        self.min_c, self.lowered = min_c, 0

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def conv1d(self, x, w, b=None, stride=1, padding=0, *a, **kw):
        if not (w.shape[2] == 3 and stride == 1 and padding == 1 and w.shape[0] == w.shape[1] >= self.min_c and x.dtype == torch.float32):
            return torch.nn.functional.conv1d(x, w, b, stride, padding, *a, **kw)
        self.lowered += 1
        B, Cc, L = x.shape
        J = (L + 3) // 4
        U = torch.from_numpy(wino_weights64(w.numpy()).astype(F32))                   # (6, cout, cin)
        xp = torch.zeros((B, Cc, 4 * J + 2), dtype=torch.float32)
        xp[:, :, 1:1 + L] = x
        d = torch.stack([xp[:, :, k:k + 4 * J:4] for k in range(6)])                   # (6, B, C, J)
        V = torch.einsum("ik,kbcj->ibcj", torch.from_numpy(BT.astype(F32)), d)
        O = torch.einsum("ioc,ibcj->iboj", U, V)
        y = torch.einsum("ri,iboj->bojr", torch.from_numpy(AT.astype(F32)), O).reshape(B, Cc, 4 * J)[:, :, :L]
        return y + b[None, :, None]


@pytest.mark.slow
@pytest.mark.parametrize("seed", [0, 7])
def test_lowered_vqvae_on_the_cpu_port(seed, monkeypatch):
    """The CPU experiment behind the lowering as a test: every eligible layer of oracle/torch_port.py's VQ encode and decode in the fp32
    Winograd form against the float64 direct networks, body and hand, 8 clips of 300 frames: z within the 2e-5 of test_vqvae_golden, not
    one code index changed, reconstructions within 1e-4."""
    from oracle import torch_port as tp
    from talkshow_amd import synth
    poses = synth.gt_poses(11 + seed, 8, 300)
    for in_dim, salt, sl in ((39, 0, slice(0, 39)), (90, 1, slice(39, 129))):
        sd = synth.vqvae_state_dict(seed=seed, in_dim=in_dim, salt=salt)
        x = np.ascontiguousarray(poses[..., sl])
        sd64 = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items() if isinstance(v, np.ndarray)}
        with torch.no_grad():
            z64, _, idx64 = tp.vqvae_encode(torch.from_numpy(x).double(), sd64)
            r64 = tp.vqvae_decode(idx64, sd64)
            wf = _WinoF()
            monkeypatch.setattr(tp, "F", wf)
            z, _, idx = tp.vqvae_encode(torch.from_numpy(x), tp._t(sd))
            r = tp.vqvae_decode(idx, tp._t(sd))
            monkeypatch.undo()
        assert wf.lowered == 12, wf.lowered                      # _enc_2, _enc_3, _dec_1, _dec_2: three layers each
        zerr = float((z.double() - z64).abs().max())
        rerr = float((r.double() - r64).abs().max())
        print(f"\n[measured] wino cpu port seed {seed} in_dim {in_dim}: z {zerr:.3e} recon {rerr:.3e}")
        assert zerr <= 2e-5 and rerr <= 1e-4
        assert torch.equal(idx, idx64)
