"""The paired, length-masked codebook search of a mixed pass, alone (`ts_op_vq_argmin_pair_masked`; csrc/vq.hip: vq_argmin_pair_lds_kernel
and its generic fallback) on random latents.

The contract (include/talkshow_hip.h, "given poses"): row h of clip b is valid iff h < lens[b] / 4; a valid row holds EXACTLY the index
`ts_op_vq_argmin` returns for that row — the arithmetic is the same operation for operation, so there is no tolerance — and an invalid row
holds -1 and is never read.  The output sits between 4 KiB red zones.  Every test fails on a build without the feature: the entry does not
exist there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 512                                   # int64 elements of red zone on each side: 4 KiB
SENT = 0x7EADBEEF7EADBEEF


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib, _lib.load(), _lib.context(0)


def reference(hip, z, cb):
    """`ts_op_vq_argmin` on all rows of one network: (M,) int64."""
    _lib, lib, ctx = hip
    M, dim = z.shape
    idx = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.ts_op_vq_argmin(ctx, _lib.dptr(z), M, _lib.dptr(cb), cb.shape[0], dim, _lib.dptr(idx), _lib.stream_ptr()))
    return idx.cpu().numpy()


def paired(hip, zb, zh, rows, B, H, cbb, cbh, form=None):
    """The entry under test with the output between red zones -> (B, H, 2) numpy.  rows: code rows per clip; the table handed over holds
    POSE frames, 4 rows + a remainder."""
    _lib, lib, ctx = hip
    lens = torch.as_tensor([4 * r + (k % 4) for k, r in enumerate(rows)], dtype=torch.int32, device="cuda")
    raw = torch.full((2 * PAD + B * H * 2,), SENT, dtype=torch.int64, device="cuda")
    body = raw[PAD:PAD + B * H * 2]
    args = (ctx, _lib.dptr(zb), _lib.dptr(zh), _lib.dptr(lens), B, H, _lib.dptr(cbb), _lib.dptr(cbh), cbb.shape[0], cbh.shape[0], zb.shape[1],
            zh.shape[1], C.c_void_p(body.data_ptr()))
    if form is None:
        _lib.check(lib.ts_op_vq_argmin_pair_masked(*args, _lib.stream_ptr()))
    else:
        _lib.check(lib.ts_debug_vq_argmin_pair_masked(*args, form, 1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((raw[:PAD] == SENT).all()) and bool((raw[PAD + B * H * 2:] == SENT).all()), "a store landed outside the code block"
    return body.cpu().numpy().reshape(B, H, 2)


def check(hip, B, H, rows, ncode, dim=64, seed=0, dup=False, nan_invalid=False, forms=(None,), ncode_hand=None):
    rng = np.random.default_rng(seed)
    nh = ncode if ncode_hand is None else ncode_hand
    cbs = [rng.standard_normal((n, dim)).astype(F32) for n in (ncode, nh)]
    if dup:                                   # duplicated code rows: the lowest index wins
        for cb in cbs:
            for j in range(1, cb.shape[0], 3):
                cb[j] = cb[j - 1]
    z = [rng.standard_normal((B * H, dim)).astype(F32) for _ in range(2)]
    if dup:                                   # and queries that sit ON duplicated codes: exact ties at the minimum
        for k in range(2):
            n = min(B * H, cbs[k].shape[0])
            z[k][:n:2] = cbs[k][:n:2]
    valid = np.zeros((B, H), bool)
    for b, r in enumerate(rows):
        valid[b, :r] = True
    zd = [torch.from_numpy(a).cuda() for a in z]
    cbd = [torch.from_numpy(a).cuda() for a in cbs]
    want = np.stack([reference(hip, zd[k], cbd[k]).reshape(B, H) for k in range(2)], -1)
    if nan_invalid:
        for k in range(2):
            a = z[k].reshape(B, H, dim).copy()
            a[~valid] = np.nan
            zd[k] = torch.from_numpy(a.reshape(B * H, dim)).cuda()
    for form in forms:
        got = paired(hip, zd[0], zd[1], rows, B, H, cbd[0], cbd[1], form)
        assert np.all(got[~valid] == -1), f"form {form}: invalid rows must hold -1"
        bad = int((got[valid] != want[valid]).sum())
        assert bad == 0, f"form {form}: {bad} of {int(valid.sum()) * 2} valid rows differ from ts_op_vq_argmin"
    return want, valid


@pytest.mark.parametrize("ncode", [1, 70, 2048])
@pytest.mark.parametrize("B,H,rows", [(1, 1, [1]), (1, 1, [0]), (3, 9, [9, 5, 1]), (3, 9, [9, 0, 3])])
def test_valid_rows_equal_the_uniform_search(hip, B, H, rows, ncode):
    """A workgroup (8 rows) straddles a clip's end, a clip has no rows, a workgroup is wholly invalid ((3, 9) with rows {9, 0, 3}: rows 8-15
    hold one valid row, rows 9-17 none); 70 codes leave a partial codebook tile.  Paired launch, one launch per network and the generic
    fallback are all held to the same indices."""
    want, valid = check(hip, B, H, rows, ncode, seed=ncode + B, forms=(None, 1, 2, 3))
    if ncode == 1:
        assert np.all(want == 0)


def test_rw8_instantiation(hip):
    """B H_max = 64 x 256 >= 32 x 512 rows: the 32-rows-per-workgroup instantiation; lengths from 0 to H_max, shuffled."""
    B, H = 64, 256
    rng = np.random.default_rng(3)
    rows = [int(r) for r in rng.integers(0, H + 1, B)]
    rows[0], rows[1], rows[2], rows[3] = H, 0, 1, H - 1
    check(hip, B, H, rows, 2048, seed=8)


def test_fallback_dim_32_and_unequal_codebooks(hip):
    """dim = 32 has no LDS form; codebooks of different sizes do not pair: both take the masked generic kernel."""
    check(hip, 3, 9, [9, 5, 1], 70, dim=32, seed=4)
    check(hip, 3, 9, [9, 0, 3], 70, dim=64, seed=5, ncode_hand=33)


@pytest.mark.parametrize("dim", [64, 32])
def test_duplicated_codes_lowest_index_wins(hip, dim):
    check(hip, 3, 9, [9, 5, 1], 70, dim=dim, seed=6, dup=True, forms=(None, 2))
    # queries placed on a duplicated pair must return the LOWER index of the pair
    rng = np.random.default_rng(6)
    cb = rng.standard_normal((70, dim)).astype(F32)
    cb[1], cb[69] = cb[0], cb[68]
    z = np.stack([cb[1], cb[69], cb[0]]).astype(F32)
    zd, cbd = torch.from_numpy(z).cuda(), torch.from_numpy(cb).cuda()
    got = paired(hip, zd, zd, [3], 1, 3, cbd, cbd)
    assert got[:, :, 0].tolist() == [[0, 68, 0]] and got[:, :, 1].tolist() == [[0, 68, 0]]


@pytest.mark.parametrize("dim", [64, 32])
def test_nan_in_invalid_rows_changes_nothing(hip, dim):
    check(hip, 3, 9, [9, 0, 3], 70, dim=dim, seed=7, nan_invalid=True, forms=(None, 2))
    check(hip, 3, 9, [9, 5, 1], 2048 if dim == 64 else 70, dim=dim, seed=9, nan_invalid=True)
