"""The argument helpers of the mixed passes, host side (no GPU, the library is not loaded): `_lib.body_mixed_args` and
`_lib.pixelcnn_mixed_args` put every optional piece of a pass — sampling controls, log-probabilities, given codes or given poses, kept
positions, speaker style, code bias, repetition records — at its own position of the most general entry of its family and every absent
piece there as None / 0; and the signatures `_lib` composes from named pieces are the argument lists the suffixed entries had when they
were spelled out one by one.
"""
import ctypes as C
import itertools

import pytest

from talkshow_amd import _lib
from talkshow_amd._lib import _i, _rp, _sp, _u64, _vp

_p32 = C.POINTER(C.c_int32)

# the argument lists of the suffixed mixed entries as the declarations in include/talkshow_hip.h have them, spelled out once
LITERAL = {
    "ts_body_pixel_infer_mixed_ctl": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp],
    "ts_pixelcnn_generate_mixed_ctl": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp],
    "ts_body_pixel_infer_mixed_lp": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp],
    "ts_pixelcnn_generate_mixed_lp": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp],
    "ts_body_pixel_infer_mixed_given": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp],
    "ts_pixelcnn_generate_mixed_given": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp],
    "ts_body_pixel_infer_mixed_poses": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _i, _p32, _vp, _vp],
    "ts_pixelcnn_generate_mixed_keep": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp],
    "ts_body_pixel_infer_mixed_keep": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp],
    "ts_body_pixel_infer_mixed_poses_keep": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _i, _p32, _vp, _vp, _vp],
    "ts_pixelcnn_generate_mixed_style": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp],
    "ts_body_pixel_infer_mixed_style": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp],
    "ts_body_pixel_infer_mixed_poses_style": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _i, _p32, _vp, _vp, _vp, _i, _vp],
    "ts_pixelcnn_generate_mixed_bias": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _vp],
    "ts_body_pixel_infer_mixed_bias": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _vp],
    "ts_body_pixel_infer_mixed_poses_bias": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _i, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _vp],
    "ts_pixelcnn_generate_mixed_repeat": [_vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _rp, _i, _vp],
    "ts_body_pixel_infer_mixed_repeat": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _rp, _i, _vp],
    "ts_body_pixel_infer_mixed_poses_repeat": [_vp, _vp, _vp, _vp, _vp, _vp, _p32, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _sp, _i, _vp, _vp, _i, _p32, _vp, _vp, _vp, _i, _vp, _i, _p32, _rp, _i, _vp],
}

BODY_FIXED = tuple(f"fixed{k}" for k in range(16))
PIX_FIXED = tuple(f"fixed{k}" for k in range(12))
# every optional piece as distinct stand-ins for the converted values: keyword -> value, in the order of the entries' parameters
PIECES = {
    "ctl": dict(ctl="CTL", n_ctl=3),
    "logprob": dict(logprob="LP"),
    "given": dict(given="GIVEN", given_rows="GROWS"),
    "poses": dict(poses=("POSES", 12, "PLENS", "PLENS_DEV")),
    "keep": dict(keep="KEEP"),
    "style": dict(style="STYLE", style_rows=9),
    "bias": dict(bias="BIAS", n_bias=2, bias_index="BIDX"),
    "repeat": dict(rep="REP", n_rep=3),
}
ABSENT = {"ctl": (None, 0), "logprob": (None,), "given": (None, None, None), "keep": (None,), "style": (None, 0), "bias": (None, 0, None),
          "repeat": (None, 0)}
PRESENT = {"ctl": ("CTL", 3), "logprob": ("LP",), "given": ("GIVEN", "GROWS", None), "poses": ("POSES", 12, "PLENS", "PLENS_DEV"),
           "keep": ("KEEP",), "style": ("STYLE", 9), "bias": ("BIAS", 2, "BIDX"), "repeat": ("REP", 3)}


def _combinations(middles):
    """Every presence combination of {ctl, logprob, one of `middles`, keep, style, bias, repeat}."""
    flags = ("ctl", "logprob", "keep", "style", "bias", "repeat")
    for middle in middles:
        for on in itertools.product((False, True), repeat=len(flags)):
            yield middle, {k for k, v in zip(flags, on) if v}


def _expected(fixed, middle, on):
    """The tuple the helper must return: the pieces in signature order, the family's middle piece (given or poses) behind logprob."""
    out = list(fixed)
    for k in ("ctl", "logprob"):
        out += PRESENT[k] if k in on else ABSENT[k]
    out += PRESENT[middle] if middle in ("given", "poses") else ABSENT["given"]
    for k in ("keep", "style", "bias", "repeat"):
        out += PRESENT[k] if k in on else ABSENT[k]
    return tuple(out) + ("STREAM",)


def _kwargs(middle, on):
    kw = dict(stream="STREAM")
    for k in on | ({middle} if middle else set()):
        kw.update(PIECES[k])
    return kw


def test_body_args_place_every_piece_in_every_presence_combination():
    seen = 0
    for middle, on in _combinations((None, "given", "poses")):
        name, args = _lib.body_mixed_args(BODY_FIXED, **_kwargs(middle, on))
        assert name in ("ts_body_pixel_infer_mixed_repeat", "ts_body_pixel_infer_mixed_poses_repeat")
        assert (name == "ts_body_pixel_infer_mixed_poses_repeat") == (middle == "poses"), (middle, on)
        assert len(args) == len(_lib.SIGNATURES[name][1]), (middle, on)
        assert args == _expected(BODY_FIXED, middle, on), (middle, on)
        seen += 1
    assert seen == 3 * 64


def test_pixelcnn_args_place_every_piece_in_every_presence_combination():
    seen = 0
    for middle, on in _combinations((None, "given")):
        name, args = _lib.pixelcnn_mixed_args(PIX_FIXED, **_kwargs(middle, on))
        assert name == "ts_pixelcnn_generate_mixed_repeat"
        assert len(args) == len(_lib.SIGNATURES[name][1]), (middle, on)
        assert args == _expected(PIX_FIXED, middle, on), (middle, on)
        seen += 1
    assert seen == 2 * 64


def test_a_count_without_its_piece_travels_as_zero():
    """n_ctl, style_rows, n_bias, n_rep and the tables that go with an absent pointer do not leak into the call."""
    _, args = _lib.body_mixed_args(BODY_FIXED, n_ctl=4, given_rows="GROWS", style_rows=7, n_bias=2, bias_index="BIDX", n_rep=5, stream="STREAM")
    assert args == _expected(BODY_FIXED, None, set())
    _, args = _lib.pixelcnn_mixed_args(PIX_FIXED, n_ctl=4, given_rows="GROWS", style_rows=7, n_bias=2, bias_index="BIDX", n_rep=5, stream="STREAM")
    assert args == _expected(PIX_FIXED, None, set())


def test_given_codes_and_given_poses_do_not_share_a_call():
    with pytest.raises(ValueError, match="given codes or given poses"):
        _lib.body_mixed_args(BODY_FIXED, given="GIVEN", given_rows="GROWS", poses=("POSES", 12, "PLENS", "PLENS_DEV"))


@pytest.mark.parametrize("name", sorted(LITERAL))
def test_composed_signature_equals_the_literal_list(name):
    res, args = _lib.SIGNATURES[name]
    assert res is _i
    assert args == LITERAL[name]


def test_the_literal_lists_cover_every_suffixed_mixed_entry():
    suffixed = {n for n in _lib.SIGNATURES if n.startswith(("ts_body_pixel_infer_mixed_", "ts_pixelcnn_generate_mixed_"))}
    assert suffixed == set(LITERAL) and len(LITERAL) == 19
    for stem in _lib.MIXED_CORE:   # a sibling is its parent plus arguments ahead of the stream: the plain entries are the cores
        assert _lib.SIGNATURES[stem][1] == _lib.MIXED_CORE[stem] + [_vp]
