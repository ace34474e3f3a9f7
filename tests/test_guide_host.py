"""Guidance, host side (include/talkshow_hip.h, "guidance"): the host check `ts_guide_check` against its numpy restatement
`sampling.guide_roles` (every refusal with the same text, 200 random valid tables), the three separate roundings of `sampling.guided`,
the identities of `sampling.sample_guide`, the `_lib` argument builders with and without the piece, and the keyword's own parser.
No GPU: the library's host-only entries run on any machine.
"""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd import sampling as S

F32 = np.float32
i32p = C.POINTER(C.c_int32)


def c_check(guide, scale, lens=None):
    """ts_guide_check -> None, or the message without its prefix."""
    g = np.ascontiguousarray(guide, np.int32)
    s = np.ascontiguousarray(scale, np.float32)
    le = None if lens is None else np.ascontiguousarray(lens, np.int32)
    rc = _lib.load().ts_guide_check(g.ctypes.data_as(i32p), s.ctypes.data_as(_lib._fp), None if le is None else le.ctypes.data_as(i32p), g.size)
    if rc == 0:
        return None
    msg = _lib.load().ts_last_error().decode()
    assert msg.startswith("ts_guide_check: ")
    return msg[len("ts_guide_check: "):]


def twin_check(guide, scale, lens=None):
    try:
        S.guide_roles(guide, len(guide), scale, lens)
    except ValueError as e:
        return str(e)
    return None


REFUSALS = [
    # (guide, scale, lens, words the message must hold)
    ([-2, -1, -1], [0, 0, 0], None, ("clip 0", "shadow index is -2")),
    ([-1, 3, -1], [0, 1, 0], None, ("clip 1", "shadow index is 3")),
    ([-1, 1, -1], [0, 1, 0], None, ("clip 1", "names itself")),
    ([2, -1, -1, 2], [1, 0, 0, 1], None, ("clip 3", "slot 2", "already the shadow of clip 0")),
    ([1, 2, -1], [1, 1, 0], None, ("clip 0", "slot 1", "itself guided")),
    ([-1, 2, 1], [0, 1, 1], None, ("clip 1", "itself guided")),
    ([1, -1, -1], [1, 0, 0], [12, 8, 8], ("clip 0", "12 frames", "8 frames", "slot 1")),
    ([-1, -1, 0], [0, 0, float("nan")], None, ("clip 2", "NaN")),
    ([-1, 0], [0, float("inf")], None, ("clip 1", "infinite")),
    ([-1, 0], [0, float("-inf")], None, ("clip 1", "infinite")),
    ([1, -1], [10000.5, 0], None, ("clip 0", "1e4")),
    ([1, -1], [-1.0001e4, 0], None, ("clip 0", "1e4")),
]


@pytest.mark.parametrize("guide,scale,lens,words", REFUSALS)
def test_refusals_agree(guide, scale, lens, words):
    got = c_check(guide, scale, lens)
    assert got is not None, "the library accepted the table"
    for w in words:
        assert w in got, got
    assert twin_check(guide, scale, lens) == got


def test_the_bound_itself_and_unread_scales_pass():
    assert c_check([1, -1], [1e4, float("nan")]) is None          # |scale| = 1e4 is allowed; a plain slot's scale is not read
    assert c_check([1, -1], [-1e4, 0]) is None
    assert twin_check([1, -1], [1e4, float("nan")]) is None
    assert c_check([1, -1], [1, 0], [8, 8]) is None
    assert _lib.load().ts_guide_check(None, None, None, 2) != 0


def test_random_valid_tables():
    rng = np.random.default_rng(11)
    for trial in range(200):
        B = int(rng.integers(1, 40))
        slots = rng.permutation(B)
        n_pairs = int(rng.integers(0, B // 2 + 1))
        guide = np.full(B, -1, np.int32)
        scale = rng.standard_normal(B).astype(F32) * F32(100.0)
        lens = (4 * rng.integers(1, 20, B)).astype(np.int32)
        want = np.full(B, -1, np.int32)
        for k in range(n_pairs):
            p, g = int(slots[2 * k]), int(slots[2 * k + 1])
            guide[p] = g
            lens[g] = lens[p]
            want[p], want[g] = g, -2
        assert c_check(guide, scale, lens) is None, (trial, guide)
        np.testing.assert_array_equal(S.guide_roles(guide, B, scale, lens), want)


def test_guided_rounds_three_times():
    """p = 0.5 + 2^-24, q = p - (1 + 2^-12), scale = 1 + 2^-12: d is exact; scale * d = 1 + 2^-11 + 2^-24 rounds (a tie, to even) to
    1 + 2^-11; p + that is a tie again and rounds to 1.5 + 2^-11.  A fused multiply-add adds the exact product and gives
    1.5 + 2^-11 + 2^-23, the next float."""
    p = F32(0.5) + F32(2.0 ** -24)
    d = F32(1.0) + F32(2.0 ** -12)
    q = F32(p - d)
    scale = F32(1.0) + F32(2.0 ** -12)
    assert Fraction(float(p)) - Fraction(float(q)) == Fraction(float(d))
    got = S.guided([p], [q], scale)[0]
    assert got.dtype == F32 and float(got) == 1.5 + 2.0 ** -11
    exact = Fraction(float(p)) + Fraction(float(scale)) * Fraction(float(d))
    fused = F32(float(exact))                                             # exact is a double here: one rounding
    assert Fraction(float(np.float64(float(exact)))) == exact
    assert float(fused) == 1.5 + 2.0 ** -11 + 2.0 ** -23 and fused != got


def test_scale_zero_and_equal_rows_are_the_plain_draw():
    rng = np.random.default_rng(5)
    V = 300
    rows = rng.standard_normal((3, V)).astype(F32)
    rows[1] = rows[0]                                                     # the shadow carries the primary's own row
    u = rng.random(3).astype(F32)
    recs = [(0.8, 0.9, 20)] * 3
    pi, pk, pl, _ = S.sample_repeat(rows, u, recs, (0, 0.0, 0.0), np.zeros((3, 0)), 0)
    for scale in (3.5, -0.5, 1e4):
        gi, gk, gl, _ = S.sample_guide(rows, u, recs, [1, -1, -1], [scale, 0, 0])
        assert gi[0] == pi[0] and np.array_equal(gk[0], pk[0]) and gl[0].view(np.uint32) == pl[0].view(np.uint32)
        assert gi[1] == gi[0] and gl[1].view(np.uint32) == gl[0].view(np.uint32)      # the shadow's entries are the primary's
        assert gi[2] == pi[2]
    rows[1] = rng.standard_normal(V).astype(F32)
    gi, gk, gl, _ = S.sample_guide(rows, u, recs, [1, -1, -1], [0.0, 0, 0])
    assert gi[0] == pi[0] and np.array_equal(gk[0], pk[0])
    assert np.array_equal(S.guided(rows[0], rows[1], 0.0), rows[0]) and S.guided(rows[0], rows[0], 7.0).tolist() == rows[0].tolist()


def test_sample_guide_composes_with_bias_and_repeat():
    rng = np.random.default_rng(6)
    V, r = 64, 9
    rows = rng.standard_normal((2, V)).astype(F32)
    u = rng.random(2).astype(F32)
    bias = rng.standard_normal((1, 2, V)).astype(F32)
    hist = rng.integers(0, V, (2, r))
    gi, gk, gl, ring = S.sample_guide(rows, u, None, [1, -1], [2.0, 0], (5, 1.0, 0.5), hist, 2 * r + 1, bias, [0, -1], 1)
    eff = np.stack([S.guided(rows[0], rows[1], 2.0), rows[1]])
    wi, wk, wl, wring = S.sample_repeat(eff, u, None, [(5, 1.0, 0.5), (0, 0.0, 0.0)], hist, 2 * r + 1, bias, [0, -1], 1)
    assert gi[0] == wi[0] and gi[1] == wi[0] and gl[1].view(np.uint32) == wl[0].view(np.uint32)
    np.testing.assert_array_equal(ring, wring)
    assert ring[1, r & 63] == -1 and ring[0, r & 63] == gi[0]             # the shadow's ring holds its history and nothing else


# ---- the argument builders -------------------------------------------------------------------------------------------------------------

PIECES = dict(ctl="CTL", n_ctl=3, logprob="LP", keep="KEEP", style="STYLE", style_rows=5, bias="BIAS", n_bias=2, bias_index="BIDX", rep="REP", n_rep=3)


@pytest.mark.parametrize("middle", ["none", "given", "poses"])
def test_builders_place_the_piece(middle):
    fixed_b, fixed_p = tuple(f"b{i}" for i in range(16)), tuple(f"p{i}" for i in range(12))
    mid = {"none": {}, "given": dict(given="G", given_rows="GR"), "poses": dict(poses=("P", 40, "PL", "PLD"))}[middle]
    groups = [("ctl", "n_ctl"), ("logprob",), ("keep",), ("style", "style_rows"), ("bias", "n_bias", "bias_index"), ("rep", "n_rep")]
    for present in itertools.product((False, True), repeat=len(groups)):
        kw = {k: PIECES[k] for g, on in zip(groups, present) if on for k in g}
        name0, args0 = _lib.body_mixed_args(fixed_b, stream="S", **mid, **kw)
        name1, args1 = _lib.body_mixed_args(fixed_b, stream="S", guide="GUIDE", guide_scale="SCALE", **mid, **kw)
        want0 = "ts_body_pixel_infer_mixed_poses_repeat" if middle == "poses" else "ts_body_pixel_infer_mixed_repeat"
        want1 = "ts_body_pixel_infer_guided_poses" if middle == "poses" else "ts_body_pixel_infer_guided"
        assert name0 == want0 and name1 == want1
        assert args1 == args0[:-1] + ("GUIDE", "SCALE", "S") and args0[-1] == "S"
        assert len(args0) == len(_lib.SIGNATURES[name0][1]) and len(args1) == len(_lib.SIGNATURES[name1][1])
        assert _lib.body_mixed_args(fixed_b, stream="S", guide=None, guide_scale=None, **mid, **kw) == (name0, args0)
        if middle != "poses":
            n0, a0 = _lib.pixelcnn_mixed_args(fixed_p, stream="S", **mid, **kw)
            n1, a1 = _lib.pixelcnn_mixed_args(fixed_p, stream="S", guide="GUIDE", guide_scale="SCALE", **mid, **kw)
            assert (n0, n1) == ("ts_pixelcnn_generate_mixed_repeat", "ts_pixelcnn_generate_guided")
            assert a1 == a0[:-1] + ("GUIDE", "SCALE", "S")
            assert len(a0) == len(_lib.SIGNATURES[n0][1]) and len(a1) == len(_lib.SIGNATURES[n1][1])
    with pytest.raises(ValueError):
        _lib.body_mixed_args(fixed_b, stream="S", guide="GUIDE")


def test_prototypes():
    lib = _lib.load()
    assert sorted(_lib.GUIDED_ENTRY.values()) == ["ts_body_pixel_infer_guided", "ts_body_pixel_infer_guided_poses", "ts_pixelcnn_generate_guided"]
    for plain, guided in _lib.GUIDED_ENTRY.items():
        rep, gui = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[guided][1]
        assert plain.endswith("_repeat") and gui == rep[:-1] + [i32p, _lib._fp, C.c_void_p]
        assert hasattr(lib, guided)
    rep, gui = _lib.SIGNATURES["ts_op_sample_repeat"][1], _lib.SIGNATURES["ts_op_sample_guide"][1]
    assert gui == rep[:-1] + [i32p, _lib._fp, C.c_void_p] and hasattr(lib, "ts_op_sample_guide") and hasattr(lib, "ts_guide_check")


# ---- the keyword's parser ----------------------------------------------------------------------------------------------------------------

def test_guide_entries():
    assert _lib.guide_entries(None, 3) is None and _lib.guide_entries([None, None], 2) is None
    e = _lib.guide_entries({"scale": 2}, 2)
    assert e == [{"scale": 2.0, "audio": None, "id": None, "style": None}] * 2
    a = np.zeros((8, 64), F32)
    e = _lib.guide_entries([None, {"scale": -0.5, "mfcc": a, "id": 1}], 2, n_classes=4)
    assert e[0] is None and e[1]["audio"] is a and e[1]["id"] == 1 and e[1]["scale"] == -0.5
    bad = [([{"scale": 1, "wav": a}, None], "clip 0", "unknown keys"), ([None, {"id": 1}], "clip 1", "needs a scale"),
           ([None, {"scale": "x"}], "clip 1", "number"), ([{"scale": float("nan")}, None], "clip 0", "NaN"),
           ([{"scale": float("inf")}, None], "clip 0", "infinite"), ([None, {"scale": 1e5}], "clip 1", "1e4"),
           ([None, {"scale": 1, "id": 1.5}], "clip 1", "whole number"), ([None, {"scale": 1, "id": 4}], "clip 1", "outside [0, 4)"),
           ([None, 3], "clip 1", "dict"), ([None], "guide takes", "list")]
    for g, *words in bad:
        with pytest.raises(ValueError) as err:
            _lib.guide_entries(g, 2, who="t", n_classes=4)
        for w in words:
            assert w in str(err.value), str(err.value)
    with pytest.raises(ValueError) as err:
        _lib.guide_entries({"scale": 1}, 2, mode=_lib.TS_SAMPLE_GREEDY)
    assert "top_k = 1" in str(err.value)
    assert _lib.guide_entries([None, None], 2, mode=_lib.TS_SAMPLE_GREEDY) is None      # nothing guided: nothing to refuse


def test_guide_layout_and_expand():
    order = [2, 0, 1]                                                     # slot k holds submitted clip order[k]
    ent = _lib.guide_entries([{"scale": 1.5}, None, {"scale": -1}], 3)
    src, shadow, guide, scale = _lib.guide_layout(order, ent)
    assert src == [0, 0, 1, 1, 2] and shadow == [False, True, False, True, False]
    assert guide.tolist() == [1, -1, 3, -1, -1] and scale.tolist() == [-1.0, 0.0, 1.5, 0.0, 0.0] and guide.dtype == np.int32 and scale.dtype == F32
    assert c_check(guide, scale, np.asarray([12, 12, 8, 8, 8], np.int32)) is None
    assert S.guide_roles(guide, 5, scale).tolist() == [1, -2, 3, -2, -1]
    tab, n = _lib.sampling_table([(1.0, 1.0, 0), (0.5, 0.9, 3), (2.0, 1.0, 7)], 3, 64, _lib.TS_SAMPLE_PHILOX)
    gblock, gtable = np.arange(3 * 2 * 2).reshape(3, 2, 2), np.asarray([1, 2, 0], np.int32)
    bidx = np.asarray([0, -1, 0], np.int32)
    (ctl, n_ctl), (gb, gt), poses, keep, (bt, bi), (rep, n_rep) = _lib.guide_expand(src, shadow, (tab, n), (gblock, gtable), bias=("T", bidx))
    assert n_ctl == 5 and [ctl[s].top_k for s in range(5)] == [0, 0, 3, 3, 7]
    assert gt.tolist() == [1, 0, 2, 0, 0] and np.array_equal(gb[1], gblock[0]) and bi.tolist() == [0, -1, -1, -1, 0]
    assert poses == (None, None) and keep is None and rep is None and n_rep == 0
    one, n1 = _lib.expand_records(tab, 1, src)
    assert one is tab and n1 == 1
