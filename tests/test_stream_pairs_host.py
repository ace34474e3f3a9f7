"""Session pairs on the host (include/talkshow_hip.h, "session pairs"): `streaming.SlotPairs` against `ts_pixelcnn_stream_pair_check` — the
same text for every refusal, agreement over random sequences of open, restart, load, step and pair calls — the `guide=` parser of a
session step, the body-level slot layout and `guide=` parsers of `streaming.BodyGuide`, and the ctypes prototypes of the new entries.
No GPU: the C rule is host arithmetic on host tables.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from talkshow_amd import _lib
from talkshow_amd.streaming import SlotPairs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ts_pixelcnn_stream_pair", "ts_pixelcnn_stream_pairs", "ts_pixelcnn_stream_step_guided", "ts_pixelcnn_stream_pair_check",
       "ts_body_stream_open_guided", "ts_body_stream_push_guided", "ts_body_stream_flush_guided"]


def c_check(S, rows, guide, clip_rows, fresh, primary, shadow=None, scale=None):
    """`ts_pixelcnn_stream_pair_check` -> None, or the library's message."""
    lib = _lib.load()
    i32, n = C.c_int32, len(primary)
    rc = lib.ts_pixelcnn_stream_pair_check(
        S, rows, (i32 * S)(*guide), (C.c_int64 * S)(*clip_rows), (i32 * S)(*fresh), (i32 * n)(*primary),
        None if shadow is None else (i32 * n)(*shadow), None if shadow is None else (C.c_float * n)(*scale), n)
    return None if rc == 0 else lib.ts_last_error().decode()


def py_check(*a):
    try:
        SlotPairs.check(*a)
    except ValueError as e:
        return str(e)
    return None


def test_every_new_entry_is_declared_exported_and_has_a_prototype():
    text = open(os.path.join(REPO, "include", "talkshow_hip.h")).read()
    declared = set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    step, guided = _lib.SIGNATURES["ts_pixelcnn_stream_step_ctl"], _lib.SIGNATURES["ts_pixelcnn_stream_step_guided"]
    assert guided[1] == step[1][:-1] + [C.POINTER(C.c_float)] + step[1][-1:]      # the scales sit ahead of the stream
    for plain in ("push", "flush"):
        a, b = _lib.SIGNATURES[f"ts_body_stream_{plain}"], _lib.SIGNATURES[f"ts_body_stream_{plain}_guided"]
        assert b[1] == a[1][:-1] + [C.POINTER(C.c_float)] + a[1][-1:]
    assert "ts_debug_stream_spread_rows" in _lib.SIGNATURES and hasattr(lib, "ts_debug_stream_spread_rows")
    assert not [n for n in NEW if "_mixed_" in n]


NONE5, ZERO5 = [-1] * 5, [0] * 5
# (what is refused, the arguments, the text)
REFUSALS = [
    ("a primary out of range", (5, 0, NONE5, ZERO5, ZERO5, [5], [1], [1.0]), "session pairs: entry 0: slot 5 is outside [0, S = 5)"),
    ("a shadow out of range", (5, 0, NONE5, ZERO5, ZERO5, [0, 2], [1, -1], [1.0, 1.0]), "session pairs: entry 1: slot -1 is outside [0, S = 5)"),
    ("a slot that names itself", (5, 0, NONE5, ZERO5, ZERO5, [2], [2], [1.0]), "session pairs: slot 2 names itself as its shadow"),
    ("a shadow named twice", (5, 0, NONE5, ZERO5, ZERO5, [0, 2], [1, 1], [1.0, 1.0]), "session pairs: slot 1 is listed twice"),
    ("a shadow that is a primary of the call", (5, 0, NONE5, ZERO5, ZERO5, [0, 1], [1, 2], [1.0, 1.0]), "session pairs: slot 1 is listed twice"),
    ("a primary already paired", (5, 0, [1, -1, -1, -1, -1], ZERO5, ZERO5, [0], [2], [1.0]),
     "session pairs: slot 0 is paired with slot 1: restart or load both to dissolve the pair"),
    ("a shadow already a shadow", (5, 0, [1, -1, -1, -1, -1], ZERO5, ZERO5, [2], [1], [1.0]),
     "session pairs: slot 1 is paired with slot 0: restart or load both to dissolve the pair"),
    ("pairing in the middle of a clip", (5, 7, NONE5, [7] * 5, ZERO5, [3], [4], [1.0]),
     "session pairs: slot 3 and slot 4 cannot pair at session row 7: a pair forms at session row 0 or behind the call that restarts or loads "
     "both slots, ahead of the next step"),
    ("only one of the two was restarted", (5, 7, NONE5, [0, 7, 7, 7, 7], [1, 0, 0, 0, 0], [0], [1], [1.0]),
     "session pairs: slot 0 and slot 1 cannot pair at session row 7: a pair forms at session row 0 or behind the call that restarts or loads "
     "both slots, ahead of the next step"),
    ("the two were listed by different calls", (5, 7, NONE5, [0, 0, 7, 7, 7], [1, 2, 0, 0, 0], [0], [1], [1.0]),
     "session pairs: slot 0 and slot 1 cannot pair at session row 7: a pair forms at session row 0 or behind the call that restarts or loads "
     "both slots, ahead of the next step"),
    ("loaded states of unequal clip rows", (5, 7, NONE5, [5, 6, 7, 7, 7], [3, 3, 0, 0, 0], [0], [1], [1.0]),
     "session pairs: slot 0 holds a clip of 5 rows, slot 1 one of 6: a shadow carries its primary's history from the clip's row 0"),
    ("a NaN", (5, 0, NONE5, ZERO5, ZERO5, [0], [1], [float("nan")]), "session pairs: slot 0: the scale is NaN"),
    ("an infinity", (5, 0, NONE5, ZERO5, ZERO5, [0, 3], [1, 4], [1.0, float("-inf")]), "session pairs: slot 3: the scale is infinite"),
    ("a scale beyond 1e4", (5, 0, NONE5, ZERO5, ZERO5, [0], [1], [-10001.0]), "session pairs: slot 0: the scale exceeds 1e4 in magnitude"),
    ("restarting a primary alone", (8, 9, [-1, -1, -1, 7, -1, -1, -1, -1], [9] * 8, [0] * 8, [3], None, None),
     "session pairs: slot 3 is paired with slot 7: list both"),
    ("loading a shadow alone", (8, 9, [-1, -1, -1, 7, -1, -1, -1, -1], [9] * 8, [0] * 8, [0, 7], None, None),
     "session pairs: slot 7 is paired with slot 3: list both"),
    ("a listed slot out of range", (8, 9, [-1, -1, -1, 7, -1, -1, -1, -1], [9] * 8, [0] * 8, [8], None, None),
     "session pairs: entry 0: slot 8 is outside [0, S = 8)"),
]


@pytest.mark.parametrize("what,args,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_has_one_text_in_c_and_python(what, args, text):
    assert c_check(*args) == text
    assert py_check(*args) == text


def test_what_the_rule_accepts():
    ok = [
        (5, 0, NONE5, ZERO5, ZERO5, [0, 3], [1, 4], [2.0, -0.5]),                      # at session row 0
        (5, 0, NONE5, ZERO5, ZERO5, [4], [0], [1e4]),                                  # the shadow may sit ahead of its primary
        (5, 7, NONE5, [0, 0, 7, 7, 7], [4, 4, 0, 0, 0], [1], [0], [0.0]),              # behind the restart of both
        (5, 7, NONE5, [5, 5, 7, 7, 7], [4, 4, 0, 0, 0], [0], [1], [1.0]),              # behind the load of both, equal clip rows
        (5, 7, [1, -1, -1, -1, -1], [7] * 5, ZERO5, [0, 1], None, None),               # a restart that lists both slots of a pair
        (5, 7, [1, -1, -1, -1, -1], [7] * 5, ZERO5, [2, 3], None, None),               # ... or neither
    ]
    for a in ok:
        assert c_check(*a) is None, a
        assert py_check(*a) is None, a


class Model:
    """A session as both sides see it: session row, per-slot clip origin, and a SlotPairs; every call is put to C and Python alike."""

    def __init__(self, S):
        self.S, self.row, self.origin, self.p = S, 0, [0] * S, SlotPairs(S)

    def clip_rows(self):
        return [self.row - o for o in self.origin]

    def both(self, *a):
        c, p = c_check(*a), py_check(*a)
        assert c == p, (a, c, p)
        return c

    def touch(self, slots, rows):
        """a restart (rows 0) or a load (the states' rows) of `slots`"""
        err = self.both(self.S, self.row, self.p.guide, self.clip_rows(), self.p.fresh_now(self.row), slots)
        try:
            self.p.check_touch(self.row, slots)
            assert err is None
        except ValueError as e:
            assert str(e) == err
            return err
        self.p.touched(self.row, slots)
        for b, n in zip(slots, rows):
            self.origin[b] = self.row - n
        return None

    def pair(self, prim, shad, scale):
        err = self.both(self.S, self.row, self.p.guide, self.clip_rows(), self.p.fresh_now(self.row), prim, shad, scale)
        before = (list(self.p.guide), list(self.p.scale))
        try:
            self.p.pair(self.row, self.clip_rows(), prim, shad, scale)
            assert err is None
        except ValueError as e:
            assert str(e) == err
            assert before == (self.p.guide, self.p.scale)      # all or none
        return err


def test_c_and_python_agree_on_200_random_sequences():
    rng = np.random.default_rng(2024)
    accepted = refused = dissolved = 0
    for _ in range(200):
        S = int(rng.integers(2, 10))
        m = Model(S)
        for _ in range(12):
            op = rng.choice(["step", "restart", "load", "pair", "pair_fresh"])
            if op == "step":
                m.row += int(rng.integers(1, 5))
                continue
            k = int(rng.integers(1, min(S, 4) + 1))
            slots = [int(v) for v in rng.choice(S, k, replace=False)]
            if op in ("restart", "load"):
                rows = [0] * k if op == "restart" else [int(v) for v in rng.integers(0, m.row + 1, k)]
                if op == "load" and rng.random() < 0.6:
                    rows = [rows[0]] * k
                had = sum(g >= 0 for g in m.p.guide)
                if m.touch(slots, rows) is None:
                    dissolved += had - sum(g >= 0 for g in m.p.guide)
                if op == "restart" or rng.random() < 0.5:
                    continue
                op = "pair_fresh"
            n = int(rng.integers(1, 3))
            if op == "pair_fresh" and len(slots) >= 2:          # among the slots the latest call listed, where that has a chance
                prim, shad = slots[0:1], slots[1:2]
            else:
                prim = [int(v) for v in rng.integers(-1, S + 1, n)]
                shad = [int(v) for v in rng.integers(-1, S + 1, n)]
            scale = [float(rng.choice([0.0, 2.0, -0.5, 1e4, 10001.0, float("nan"), float("inf")], p=[.2, .3, .2, .1, .1, .05, .05]))
                     for _ in prim]
            if m.pair(prim, shad, scale) is None:
                accepted += 1
            else:
                refused += 1
        g = m.p.guide                                           # the table stays one ts_guide_check accepts
        _lib.guide_check(g, m.p.scale) if any(v >= 0 for v in g) else None
    assert accepted > 100 and refused > 100 and dissolved > 10, (accepted, refused, dissolved)


def test_pairs_keyword_forms():
    assert SlotPairs.parse({0: 1, 3: (4, 2.5)}) == ([0, 3], [1, 4], [SlotPairs.DEFAULT_SCALE, 2.5])
    for bad in ([(0, 1)], {0: (1, 2, 3)}, {0: {1: 2}}, "0:1"):
        with pytest.raises(ValueError, match="pairs"):
            SlotPairs.parse(bad)


def test_step_guide_parser_every_form_and_every_refusal():
    p = SlotPairs(5)
    p.pair(0, [0] * 5, [0, 3], [1, 4], [2.0, -0.5])
    assert p.pairs == {0: (1, 2.0), 3: (4, -0.5)}
    assert p.step_scales(None) is None
    assert p.step_scales(1.5) == [1.5, 0.0, 0.0, 1.5, 0.0]
    assert p.step_scales(0) == [0.0] * 5
    assert p.step_scales({3: 7.0}) == [2.0, 0.0, 0.0, 7.0, 0.0]                 # a primary left out keeps its stored scale
    assert p.step_scales([None, None, None, 0.25, None]) == [2.0, 0.0, 0.0, 0.25, 0.0]
    assert p.step_scales([1e4, None, None, -1e4, None]) == [1e4, 0.0, 0.0, -1e4, 0.0]
    assert p.step_scales({0: 0.1})[0] == float(np.float32(0.1))                # the fp32 value the library receives
    assert p.scale == [2.0, 0.0, 0.0, -0.5, 0.0]                                # a step's scales are not stored
    refusals = [
        ({1: 2.0}, "step: guide: slot 1 is no primary of a pair"),
        ({2: 2.0}, "step: guide: slot 2 is no primary of a pair"),
        ([None, None, 1.0, None, None], "step: guide: slot 2 is no primary of a pair"),
        ({5: 2.0}, "step: guide: slot 5 is outside [0, S = 5)"),
        ({0: float("nan")}, "step: guide: slot 0: the scale is NaN"),
        ({3: float("inf")}, "step: guide: slot 3: the scale is infinite"),
        ([1.0, None, None, -10000.5 * 2, None], "step: guide: slot 3: the scale exceeds 1e4 in magnitude"),
        (float("nan"), "step: guide: slot 0: the scale is NaN"),
        ({0: "2"}, "step: guide: slot 0: the scale is not a number"),
        ([1.0, None, None], "step: guide holds one entry per slot (S = 5), got 3"),
        ("2", "step: guide is None, a float, a {primary: scale} dict or an (S,) list, got str"),
    ]
    for g, text in refusals:
        with pytest.raises(ValueError) as e:
            p.step_scales(g)
        assert str(e.value) == text, g
    with pytest.raises(ValueError, match="the session holds no pair"):
        SlotPairs(3).step_scales(2.0)
    with pytest.raises(ValueError, match="slot 0 is no primary of a pair"):
        SlotPairs(3).step_scales({0: 2.0})


def test_a_restart_that_lists_both_dissolves_and_may_declare_again():
    p = SlotPairs(5)
    p.pair(0, [0] * 5, [0, 3], [1, 4], [2.0, -0.5])
    with pytest.raises(ValueError, match="slot 3 is paired with slot 4: list both"):
        p.check_touch(6, [2, 3])
    p.check_touch(6, [4, 3])
    p.touched(6, [4, 3])
    assert p.pairs == {0: (1, 2.0)}
    p.pair(6, [6, 6, 6, 0, 0], [4], [3], [1.0])                 # the roles may swap in the new clip
    assert p.pairs == {0: (1, 2.0), 4: (3, 1.0)}
    p.touched(6, [0, 1])
    with pytest.raises(ValueError, match="cannot pair at session row 9"):
        p.copy().pair(9, [3, 3, 9, 3, 3], [0], [1], [1.0])      # a step has been run since
    p.pair(6, [0, 0, 6, 0, 0], [1], [0], [1.0])
    assert p.pairs == {1: (0, 1.0), 4: (3, 1.0)}


# ---- the body level: `BodyGuide` (clips first, shadows behind, the encoder map) ---------------------------------------------------------
def test_body_slot_layout_for_every_presence_pattern():
    import itertools
    from talkshow_amd.streaming import BodyGuide
    n = 0
    for B in range(1, 5):
        for kinds in itertools.product((None, "shared", "own"), repeat=B):      # per clip: no shadow, one on the clip's audio, one on its own
            guide = [None if k is None else {"scale": 1.0 + b, "audio": k == "own"} for b, k in enumerate(kinds)]
            g = BodyGuide(guide, B, 4)
            n_g, n_a = sum(k is not None for k in kinds), sum(k == "own" for k in kinds)
            assert (g.S, g.E) == (B + n_g, B + n_a)
            assert g.shadow_of == [b for b, k in enumerate(kinds) if k is not None]          # the shadows behind the clips, in clip order
            own = iter(range(B, B + n_a))
            assert g.enc_of == [next(own) if kinds[b] == "own" else -1 for b in g.shadow_of]
            spread = g.spread()
            assert spread[:B] == list(range(B)) and len(spread) == g.S and max(spread) == g.E - 1
            for k, b in enumerate(g.shadow_of):
                assert spread[B + k] == (g.enc_of[k] if kinds[b] == "own" else b)
                assert g.pairs()[b] == (B + k, 1.0 + b)
            if n_g:
                _lib.guide_check([g.pairs().get(b, (-1, 0))[0] for b in range(g.S)], [1.0] * g.S)   # a table ts_guide_check accepts
            n += 1
    assert n == 3 + 9 + 27 + 81


def test_body_open_and_push_guide_parsers():
    from talkshow_amd.streaming import BodyGuide
    one = BodyGuide({"scale": 2, "id": 1}, 2, 4)                                   # one dict serves all clips
    assert one.entries == [{"scale": 2.0, "id": 1, "style": None, "audio": False}] * 2 and (one.S, one.E) == (4, 2)
    assert BodyGuide(None, 3, 4).S == 3 and BodyGuide([None] * 3, 3, 4).shadow_of == []
    row = [0.5, 0.5, 0.0, 0.0]
    g = BodyGuide([{"scale": 2.0, "style": np.array(row, np.float32), "audio": True}, {"scale": -0.5, "id": 3}, None], 3, 4)
    assert g.entries[0]["style"] == row and g.entries[1]["id"] == 3
    for bad, text in [([{"scale": 1.0, "mfcc": 0}, None, None], "guide of clip 0: unknown keys"),
                      ([None, {"id": 2}, None], "guide of clip 1: \"scale\" is required"),
                      ([None, None, {"scale": "2"}], "guide of clip 2: the scale is not a number"),
                      ([{"scale": float("inf")}, None, None], "guide of clip 0: the scale is infinite"),
                      ([{"scale": 1.0, "id": 4}, None, None], "guide of clip 0: id 4 is outside"),
                      ([{"scale": 1.0, "style": [1.0, 0.0]}, None, None], "guide of clip 0: a style row holds n_classes = 4"),
                      ([{"scale": 1.0, "style": [1.0, 0.0, float("nan"), 0.0]}, None, None], "guide of clip 0: a style weight is not finite"),
                      ([{"scale": 1.0, "audio": 1}, None, None], "guide of clip 0: \"audio\" is True"),
                      ([2.0, None, None], "guide of clip 0: an entry is None or a dict"),
                      ([None], "one entry per clip")]:
        with pytest.raises(ValueError, match=text):
            BodyGuide(bad, 3, 4)

    class M:                                                                        # stands in for an MFCC chunk: only its shape is read
        def __init__(self, *shape):
            self.shape = shape
    m = M(12, 64)
    assert g.push([{"mfcc": m}, None, None], 12) == (None, [m])
    assert g.push([{"scale": 0.25, "mfcc": m}, 3, None], 12) == ({0: 0.25, 1: 3.0}, [m])
    own = BodyGuide([None, {"scale": 1.0}, {"scale": 1.0}], 3, 4)                   # no shadow hears audio of its own
    assert own.push(None, 8) == (None, []) and own.push(0.5, 8) == ({1: 0.5, 2: 0.5}, [])
    assert own.push([None, {"scale": 2.0}, {}], 8) == ({1: 2.0}, [])
    for bad, text in [(None, "guide of clip 0: the shadow was opened with audio of its own"),
                      (1.0, "guide of clip 0: the shadow was opened with audio of its own"),
                      ([{"mfcc": M(8, 64)}, None, None], r"guide of clip 0: .*\(12, 64\) is required, got \(8, 64\)"),
                      ([{"mfcc": m}, {"mfcc": m}, None], "guide of clip 1: the shadow was opened without audio of its own"),
                      ([{"mfcc": m}, None, 0.0], "guide of clip 2: the clip was opened without a shadow"),
                      ([{"mfcc": m, "wav": 1}, None, None], "guide of clip 0: unknown keys"),
                      ([{"mfcc": m}, float("nan"), None], "guide of clip 1: the scale is NaN"),
                      ([{"mfcc": m}, -20000.0, None], "guide of clip 1: the scale exceeds 1e4"),
                      ([{"mfcc": m}, "x", None], "guide of clip 1: the scale is not a number"),
                      ([{"mfcc": m}], "one entry per clip"), ("2", "one entry per clip")]:
        with pytest.raises(ValueError, match=text):
            g.push(bad, 12)
    with pytest.raises(ValueError, match="opened without a shadow"):
        BodyGuide(None, 2, 4).push(1.0, 8)
