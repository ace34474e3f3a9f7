"""The promise the Python call sites rest on (include/talkshow_hip.h: "X == NULL: exactly the entry above, launch for launch"): every
mixed entry, called with its own arguments, and the most general entry of its family, called with the same arguments and NULL / 0 for the
rest, give bit-equal codes, poses and log-probabilities, and the second call finds every graph it needs captured by the first.

One small pass: 3 clips of 36, 8 and 4 MFCC rows = 9, 2 and 1 code rows — two chunks, the active prefix shrinks from 3 clips to 1 and the
last chunk is short —, Philox draws, given rows G = (2, 1, 0) (codes, or 8, 4 and 0 pose frames), a random mask, a one-row style blend, one
shared bias table, one repetition record of window 4.  Networks and weights of tests/test_gpu_keep_canary.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import _lib, synth
from test_gpu_keep_canary import V, nets  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
LENS = np.asarray([36, 8, 4], np.int32)
B, T_MAX, H = 3, 36, 9
G = np.asarray([2, 1, 0], np.int32)
PLENS = (4 * G).astype(np.int32)
SEED = 0x5EED
SUFFIXES = ("ctl", "lp", "given", "keep", "style", "bias", "repeat")
POSES_SUFFIXES = ("poses", "poses_keep", "poses_style", "poses_bias", "poses_repeat")
ENTRIES = (["ts_pixelcnn_generate_mixed"] + [f"ts_pixelcnn_generate_mixed_{s}" for s in SUFFIXES] + ["ts_body_pixel_infer_mixed"] +
           [f"ts_body_pixel_infer_mixed_{s}" for s in SUFFIXES + POSES_SUFFIXES])


@pytest.fixture(scope="module")
def pieces():
    """Every optional piece of the pass as the keywords of `_lib.body_mixed_args`, by the suffix that brings it; the tensors behind the
    pointers are kept alive beside them."""
    rng = np.random.default_rng(11)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    ctl = (_lib.TsSampling * B)()
    for b, (t, p, k) in enumerate([(0.7, 0.9, 0), (1.3, 1.0, 40), (1.0, 0.5, 0)]):
        ctl[b].temperature, ctl[b].top_p, ctl[b].top_k, ctl[b].reserved = t, p, k, 0
    rep = (_lib.TsRepeat * 1)()
    rep[0].window, rep[0].presence, rep[0].frequency, rep[0].reserved = 4, 1.5, 0.5, 0
    style = rng.random((B, 1, 4)).astype(np.float32)
    style /= style.sum(-1, keepdims=True)
    bidx = np.zeros(B, np.int32)
    alive = dict(given=dev(rng.integers(0, V, (B, H, 2)).astype(np.int64)), keep=dev(rng.integers(0, 2, (B, H, 2)).astype(np.uint8)),
                 style=dev(style), bias=dev(rng.standard_normal((1, 2, V)).astype(np.float32)),
                 gp=dev(synth.gt_poses(61, B, int(PLENS.max()))), plens=dev(PLENS), bidx=bidx, ctl=ctl, rep=rep)
    kw = {"ctl": dict(ctl=ctl, n_ctl=B),
          "given": dict(given=_lib.dptr(alive["given"]), given_rows=G.ctypes.data_as(I32P)),
          "poses": dict(poses=(_lib.dptr(alive["gp"]), int(PLENS.max()), PLENS.ctypes.data_as(I32P), _lib.dptr(alive["plens"]))),
          "keep": dict(keep=_lib.dptr(alive["keep"])),
          "style": dict(style=_lib.dptr(alive["style"]), style_rows=1),
          "bias": dict(bias=_lib.dptr(alive["bias"]), n_bias=1, bias_index=bidx.ctypes.data_as(I32P)),
          "repeat": dict(rep=rep, n_rep=1)}
    return kw, alive


def _own_pieces(name):
    """The pieces an entry's parameter list holds, in order: its suffix's and those of the siblings above it."""
    suffix = name.split("_mixed", 1)[1].lstrip("_")
    if not suffix:
        return ()
    if suffix.startswith("poses"):
        return ("ctl", "lp", "poses") + tuple(s.split("_")[1] for s in POSES_SUFFIXES[1:POSES_SUFFIXES.index(suffix) + 1])
    return SUFFIXES[:SUFFIXES.index(suffix) + 1]


def _own_args(fixed, own, kw, lp):
    """The entry's own argument tuple: the fixed arguments, every piece it has (a third, NULL, device table behind the given rows), the stream."""
    args = list(fixed)
    for piece in own:
        if piece == "lp":
            args.append(_lib.dptr(lp))
        elif piece == "poses":
            args += kw["poses"]["poses"]
        else:
            args += list(kw[piece].values()) + ([None] if piece == "given" else [])
    return args + [_lib.stream_ptr()]


@pytest.mark.parametrize("name", ENTRIES)
def test_an_entry_is_the_most_general_one_with_null_for_the_rest(nets, pieces, name):  # noqa: F811
    lib = _lib.load()
    ae, px, vb, vh = nets
    kw, _ = pieces
    body = name.startswith("ts_body")
    own = _own_pieces(name)
    lens_dev = torch.from_numpy(LENS).cuda()
    clip = torch.tensor([5, 9, 2], dtype=torch.int64, device="cuda")
    ids = torch.tensor([1, 3, 0], dtype=torch.int64, device="cuda")
    src = torch.from_numpy(synth.mfcc_features(83, B, T_MAX) if body else
                           np.random.default_rng(7).standard_normal((B, H, 256)).astype(np.float32)).cuda()
    nets_args = (ae.handle(), px.handle(), vb.handle(), vh.handle()) if body else (px.handle(),)

    def outputs():
        codes = torch.full((B, H, 2), -9, dtype=torch.int64, device="cuda")
        poses = torch.full((B, 4 * H, 129), -9.0, dtype=torch.float32, device="cuda") if body else None
        lp = torch.full((B, H, 2), -9.0, dtype=torch.float32, device="cuda") if "lp" in own else None
        return codes, poses, lp

    def fixed(codes, poses):
        head = (_lib.dptr(src), _lib.dptr(ids)) if body else (_lib.dptr(ids), _lib.dptr(src))
        return (*nets_args, *head, LENS.ctypes.data_as(I32P), _lib.dptr(lens_dev), B, T_MAX if body else H, _lib.TS_SAMPLE_PHILOX, None, SEED,
                _lib.dptr(clip), _lib.dptr(codes), *((_lib.dptr(poses),) if body else ()))

    first = outputs()
    own_args = _own_args(fixed(*first[:2]), own, kw, first[2])
    assert len(own_args) == len(_lib.SIGNATURES[name][1])
    _lib.check(getattr(lib, name)(*own_args))
    torch.cuda.synchronize()
    captures = lib.ts_pixelcnn_graph_captures(px.handle(), _lib.stream_ptr())

    second = outputs()
    general = {k: v for piece in own if piece != "lp" for k, v in kw[piece].items()}
    helper = _lib.body_mixed_args if body else _lib.pixelcnn_mixed_args
    top, args = helper(fixed(*second[:2]), logprob=_lib.dptr(second[2]), stream=_lib.stream_ptr(), **general)
    assert top == ("ts_body_pixel_infer_mixed_poses_repeat" if "poses" in own else
                   "ts_body_pixel_infer_mixed_repeat" if body else "ts_pixelcnn_generate_mixed_repeat")
    _lib.check(getattr(lib, top)(*args))
    torch.cuda.synchronize()
    assert lib.ts_pixelcnn_graph_captures(px.handle(), _lib.stream_ptr()) == captures   # NULL adds no graph key: nothing is captured

    for a, b in zip(first, second):
        if a is not None:
            bits = torch.int64 if a.dtype == torch.int64 else torch.int32   # floats compared as their bit patterns
            assert torch.equal(a.view(bits), b.view(bits))
    codes = first[0].cpu().numpy()
    for b in range(B):   # the pass ran: every own row holds a code, every row beyond them the documented -1
        assert np.all((codes[b, :LENS[b] // 4] >= 0) & (codes[b, :LENS[b] // 4] < V)) and np.all(codes[b, LENS[b] // 4:] == -1)
