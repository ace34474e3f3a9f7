"""`style_rows_kernel` on its own (`ts_op_style_rows`) against the numpy restatement of the rule (`sampling.style_rows`;
include/talkshow_hip.h, "speaker style"), BIT FOR BIT: M in {1, 3, 257} weight rows, NC in {1, 4, 7} speakers, W in {64, 2 * dim of the
quick tests' network} and NL in {1, 3} tables.  The weights hold exact zeros (+0.0 and -0.0), negatives, values above 1 and one all-zero
row; one table row per layer is NaN under a zero weight wherever that speaker's weight is zero, and must not reach the output.  Fails on a
build without the feature: the entry does not exist there.
"""
import numpy as np
import pytest
import torch

from talkshow_amd import sampling as S

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = dict(input_dim=256, dim=64, n_layers=3)


def _case(M, NC, W, NL, seed):
    rng = np.random.default_rng(seed)
    tables = rng.standard_normal((NL, NC, W)).astype(F32)
    tables[:, 0, 1] = -0.0
    w = (rng.standard_normal((M, NC)) * 1.5).astype(F32)          # negatives and values above 1
    w[rng.random((M, NC)) < 0.35] = 0.0
    w[rng.random((M, NC)) < 0.05] = -0.0
    w[M // 2] = 0.0                                               # one all-zero row
    if M > 1:
        w[0] = 0.0
        w[0, NC - 1] = 1.0                                        # a one-hot row
    if NC > 1:                                                    # speaker `dead` is NaN in every table and has weight zero everywhere
        dead = NC // 2
        w[:, dead] = 0.0
        if M > 1 and dead == NC - 1:
            w[0, 0] = 1.0
        tables[:, dead] = np.nan
    return tables, w


@pytest.mark.parametrize("NL", [1, 3])
@pytest.mark.parametrize("W", [64, 2 * DIMS["dim"]])
@pytest.mark.parametrize("NC", [1, 4, 7])
@pytest.mark.parametrize("M", [1, 3, 257])
def test_kernel_is_the_rule(M, NC, W, NL):
    from talkshow_amd import _lib
    lib = _lib.load()
    tables, w = _case(M, NC, W, NL, 1000 * M + 100 * NC + W + NL)
    td, wd = torch.from_numpy(tables).cuda(), torch.from_numpy(w).cuda()
    out = torch.full((NL, M, W), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.ts_op_style_rows(_lib.context(), _lib.dptr(td), NL, NC, W, _lib.dptr(wd), M, _lib.dptr(out), _lib.stream_ptr()))
    got = out.cpu().numpy()
    want = np.stack([S.style_rows(w, tables[l]) for l in range(NL)])
    if NC > 1:
        assert np.isfinite(got).all(), "a table row under a zero weight reached the output"
    else:
        assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} elements differ from sampling.style_rows"
    zero = got[:, M // 2].view(np.uint32)
    assert not zero.any(), "an all-zero weight row gives +0.0"
    if M > 1 and NC > 1:                                          # the one-hot row is its table row, the -0.0 entry included
        c = int(np.flatnonzero(w[0])[0])
        assert np.array_equal(got[:, 0].view(np.uint32), tables[:, c].view(np.uint32))


def test_refusals():
    from talkshow_amd import _lib
    lib = _lib.load()
    t = torch.zeros((1, 4, 64), device="cuda")
    w = torch.zeros((2, 4), device="cuda")
    o = torch.zeros((1, 2, 64), device="cuda")
    ctx, s = _lib.context(), _lib.stream_ptr()
    assert lib.ts_op_style_rows(ctx, _lib.dptr(t), 1, 4, 62, _lib.dptr(w), 2, _lib.dptr(o), s) != 0      # W is a multiple of 4
    assert lib.ts_op_style_rows(ctx, None, 1, 4, 64, _lib.dptr(w), 2, _lib.dptr(o), s) != 0
    assert lib.ts_op_style_rows(ctx, _lib.dptr(t), 1, 4, 64, _lib.dptr(w), 0, _lib.dptr(o), s) != 0
    assert lib.ts_op_style_rows(ctx, _lib.dptr(t), 0, 4, 64, _lib.dptr(w), 2, _lib.dptr(o), s) != 0
