"""Slot state, the host arithmetic (`talkshow_amd/streaming.py::SlotClock`, `SlotState`; include/talkshow_hip.h, "slot state"): the layout of
a state row, what a save at r < 3 writes as a restart's values, where a load puts a state, and the refusals — without a GPU.  Every test
fails on a tree without the feature: the names do not exist."""
import types

import numpy as np
import pytest
import torch

from talkshow_amd import _lib
from talkshow_amd.modules import PixelCNNStream
from talkshow_amd.streaming import SeamlessBodyStream, SlotClock, SlotState


# ---- 1. the layout against a brute-force restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, NL", [(32, 2), (64, 3), (256, 15)])
def test_layout_against_brute_force(D, NL):
    blocks = [("q1", 4 * D), ("q0a", 4 * D), ("q0b", 4 * D)] + [(("p", l), 4 * D) for l in range(1, NL)] + [(("cr", l), 2 * D) for l in range(NL)]
    blocks += [("tok", 6), ("pad", 2), ("rep", 128)]
    at, where = 0, {}
    for name, n in blocks:                                   # one block after the other, nothing between them
        where[name] = at
        at += n
    L = SlotClock.state_layout(D, NL)
    assert (L["q1"], L["q0a"], L["q0b"]) == (where["q1"], where["q0a"], where["q0b"])
    assert L["p"] == where.get(("p", 1), where[("cr", 0)]) and L["cr"] == where[("cr", 0)]
    assert L["tok"] == where["tok"] and L["rep"] == where["rep"] and L["words"] == at == SlotClock.state_words(D, NL)
    for l in range(1, NL):
        assert L["p"] + (l - 1) * 4 * D == where[("p", l)]
    floats = [L["q1"], L["q0a"], L["q0b"]] + [where[("p", l)] for l in range(1, NL)] + [where[("cr", l)] for l in range(NL)]
    assert all(o % 4 == 0 for o in floats) and L["tok"] % 4 == 0 and L["rep"] % 4 == 0 and (L["words"] - L["tok"]) % 4 == 0
    if (D, NL) == (256, 15):
        assert 4 * L["words"] == 100896                      # "about 100 KB per slot on the full-size network"


def test_the_info_record_is_48_bytes():
    import ctypes as C
    assert C.sizeof(_lib.TsSlotInfo) == 48 and _lib.TS_SLOT_STATE_VERSION == SlotClock.STATE_VERSION


# ---- 2. the canonical entries at r = 0, 1, 2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", range(7))
def test_canonical_entries_against_the_launches(r):
    """The launches of a session's first rows: row x reads the token row x - 1 if it exists, Q1[x & 3] from row 2 on, Q0[x & 3]
    from row 3 on, P(l, x & 1) from row 1 on.  A saved entry is canonical exactly when the row that would read it does not: the token rows
    below 0, Q1 (read by row r), Q0a (read by row r), Q0b (read by row r + 1), P (read by row r).  Its canonical value is the restart's."""
    c = SlotClock.canonical(r)
    assert c["tok"] == [k for k in range(3) if r - 1 - k < 0]
    assert c["q1"] == (not r >= 2) and c["q0a"] == (not r >= 3) and c["q0b"] == (not r + 1 >= 3) and c["p"] == (not r >= 1)
    w = SlotClock.rewrites(r)                                # the entries a restart at row r writes are the entries a state holds
    plan = SlotClock.load_plan(r, r)
    assert [i for i in plan["tok"] if i is not None] == w["tok"] and [plan["q1"]] == w["q1"] and plan["q0"] == w["q0"] and plan["p"] == w["p"]
    assert len(c["tok"]) == 3 - len(w["tok"])                # the ring rows a restart cannot write are the ones a save makes -1
    if r >= 3:
        assert c == {"tok": [], "q1": False, "q0a": False, "q0b": False, "p": False}


# ---- 3. a load against a brute-force replay -------------------------------------------------------------------------------------------------------
def test_load_against_a_replay_of_random_triples():
    """A source runs rows 0 .. r-1 of a clip that began at row o and writes code x of its row into ring[x & 63] under a penalty switched on
    h rows ago; the state stores the history by age; the target puts it at r'.  What the samplers of the target's row r' + j then read
    (ring[(row - 1 - t) & 63] for t < min(row - from_row, window)) must be the clip's own last codes, and the Philox position the clip's."""
    rng = np.random.default_rng(5)
    seen_negative = seen_short = 0
    for _ in range(200):
        o = int(rng.integers(0, 50))
        n = int(rng.integers(0, 200))
        r = o + n
        h = int(rng.integers(-1, n + 1))                     # -1: no penalty running
        r2 = int(rng.integers(min(n, 3), 260))
        code = lambda clip_row: 1000 + clip_row              # noqa: E731  the code of a clip row (one column)
        ring = np.full(64, -7, np.int64)
        for x in range(o, r):
            ring[x & 63] = code(x - o)
        hist = -1 if h < 0 else min(h, 64)                   # what the state records
        by_age = [int(ring[(r - 1 - k) & 63]) if k < hist else -1 for k in range(64)]
        plan = SlotClock.load_plan(r2, n, hist)
        assert plan["origin"] == r2 - n
        seen_negative += plan["origin"] < 0
        seen_short += hist > r2
        target = np.full(64, -9, np.int64)
        for k in range(64):
            target[plan["ring"][k]] = by_age[k]
        clock = SlotClock(2).advance(r2).load([1], [n], [9])
        assert clock.slot_rows == [r2, n] and clock.origin(1) == r2 - n and clock.clip(1, 100) == 9 and clock.clip(0, 100) == 100
        assert clock.position(1, r2, 1) == 2 * n + 1         # the next code's Philox position: its row and column inside the clip
        if hist < 0:
            assert plan["rep_from"] is None
            continue
        assert plan["rep_from"] == r2 - hist
        for window in (1, 3, 64):
            cnt = min(r2 - plan["rep_from"], window)
            got = [int(target[(r2 - 1 - t) & 63]) for t in range(cnt)]
            assert got == [code(n - 1 - t) for t in range(min(h, window))]
        for k, i in enumerate(plan["tok"]):                  # the token rows: at their ring index, or below the session's row 0
            assert i == ((r2 - 1 - k) % 4 if r2 - 1 - k >= 0 else None)
        assert plan["q1"] == r2 % 4 and plan["q0"] == [r2 % 4, (r2 + 1) % 4] and plan["p"] == r2 % 2
    assert seen_negative > 20 and seen_short > 3


# ---- 4. the refusals, before the library is touched ----------------------------------------------------------------------------------------------
B, DIMS = 3, (32, 3, 4, 128)


def _info(rows=5, clip=7, **kw):
    o = dict(D=DIMS[0], NL=DIMS[1], NC=DIMS[2], V=DIMS[3], version=SlotClock.STATE_VERSION, hist=-1, rows=rows, clip_index=clip, label=1)
    o.update(kw)
    return o


def _state(*infos):
    return SlotState(torch.zeros((len(infos), SlotClock.state_words(DIMS[0], DIMS[1])), dtype=torch.int32), infos)


class _Rows:
    """A library that answers the row counter and nothing else."""

    def __init__(self, rows):
        self.rows = rows

    def __getattr__(self, name):
        if name == "ts_pixelcnn_stream_rows":
            return lambda h: self.rows
        raise AssertionError(f"the library was called ({name}) before the refusal")


@pytest.fixture
def session(monkeypatch):
    def make(rows=None):
        def load():
            if rows is None:
                raise AssertionError("the library was touched before the refusal")
            return _Rows(rows)
        monkeypatch.setattr(_lib, "load", load)
        st = object.__new__(PixelCNNStream)
        st.net = types.SimpleNamespace(dim=DIMS[0], n_layers=DIMS[1], n_classes=DIMS[2], input_dim=DIMS[3], _dev=lambda: torch.device("cpu"))
        st.B, st.max_rows, st._h = B, 4, None
        st._labels = np.array([0, 1, 2], np.int64)
        return st
    return make


LOAD_REFUSALS = [
    ("slot 3 is outside", dict(slots=[0, 3], state=_state(_info()))),
    ("slot -1 is outside", dict(slots=-1, state=_state(_info()))),
    ("slot 1 is listed twice", dict(slots=[1, 2, 1], state=_state(_info()))),
    ("3 slots but 2 states", dict(slots=[0, 1, 2], state=_state(_info(), _info()))),
    ("2 slots but 3 clip index", dict(slots=[0, 1], state=_state(_info()), clip_indices=[1, 2, 3])),
    ("slot 2: the state is of a network", dict(slots=[1, 2], state=_state(_info(), _info(D=64)))),
    ("slot 0: the state is of a network", dict(slots=[0], state=_state(_info(V=2048)))),
    ("slot 0: the state is of a network", dict(slots=[0], state=_state(_info(NL=4)))),
    ("slot 0: the state is of a network", dict(slots=[0], state=_state(_info(NC=5)))),
    ("slot 1: the state has layout version 2", dict(slots=[1], state=_state(_info(version=2)))),
    ("slot 2: clip index -4 is negative", dict(slots=[0, 2], state=_state(_info()), clip_indices=[1, -4])),
    ("slot 0: clip index -1 is negative .the state records none", dict(slots=[0], state=_state(_info(clip=-1)))),
    ("no slot given", dict(slots=[], state=_state(_info()))),
    ("must be a SlotState", dict(slots=[0], state=np.zeros(4))),
]


@pytest.mark.parametrize("names, kw", LOAD_REFUSALS, ids=[r[0] for r in LOAD_REFUSALS])
def test_load_refuses_and_names_the_slot(session, names, kw):
    st = session()
    with pytest.raises(ValueError, match=names):
        st.load(**kw)
    assert list(st._labels) == [0, 1, 2]


@pytest.mark.parametrize("rows, n, ok", [(0, 1, False), (1, 2, False), (2, 3, False), (2, 50, False), (2, 2, True), (1, 1, True), (0, 0, True),
                                         (3, 50, True), (3, 3, True)])
def test_the_row_rule(session, rows, n, ok):
    """r' < min(n, 3) is refused, naming the slot and both numbers, with only the row counter read; n = 2 at r' = 2 is accepted."""
    if ok:
        assert SlotClock.check_load(B, DIMS, rows, [1], [_info(rows=n)]) == ([1], [0], [7])
        return
    with pytest.raises(ValueError, match=f"slot 1: a clip of {n} rows cannot be loaded at session row {rows} "):
        session(rows).load([1], _state(_info(rows=n)))


@pytest.mark.parametrize("names, kw", [("slot 3 is outside", dict(slots=[3])), ("no slot given", dict(slots=[]))])
def test_save_refuses(session, names, kw):
    with pytest.raises(ValueError, match=names):
        session().save(**kw)


@pytest.mark.parametrize("names, kw", [("slot 5 is outside", dict(src=5, dst_slots=[0])), ("one source slot", dict(src=[0, 1], dst_slots=[2])),
                                       ("slot 2 is listed twice", dict(src=0, dst_slots=[2, 2])),
                                       ("slot 1: clip index -3", dict(src=0, dst_slots=[2, 1], clip_indices=[4, -3])),
                                       ("2 slots but 1 clip index", dict(src=0, dst_slots=[2, 1], clip_indices=[4]))])
def test_fork_refuses(session, names, kw):
    with pytest.raises(ValueError, match=names):
        session().fork(**kw)


def test_seamless_session_takes_no_state():
    s = object.__new__(SeamlessBodyStream)
    s._h = None
    for call in (lambda: s.save([0]), lambda: s.load([0], None), lambda: s.fork(0, [1])):
        with pytest.raises(NotImplementedError, match="seamless"):
            call()


# ---- 5. SlotState: indexing and bytes -------------------------------------------------------------------------------------------------------------
def test_slot_state_indexing_and_bytes():
    W = SlotClock.state_words(DIMS[0], DIMS[1])
    rng = np.random.default_rng(3)
    words = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (3, W), dtype=np.int64).astype(np.int32))   # NaN patterns and -0.0 among them
    s = SlotState(words, [_info(rows=k, clip=10 + k, hist=min(k, 64), label=k % 4) for k in (4, 70, 0)])
    assert len(s) == 3 and s.rows == [4, 70, 0] and s.device.type == "cpu"
    one, two = s[1], s[[2, 0]]
    assert len(one) == 1 and one.infos[0]["rows"] == 70 and torch.equal(one.words[0], words[1])
    assert two.rows == [0, 4] and torch.equal(two.words, words[[2, 0]]) and len(s[1:]) == 2 and s[-1].rows == [0]
    back = SlotState.frombytes(s.tobytes())
    assert back.infos == s.infos and torch.equal(back.words, words) and back.words.dtype == torch.int32
    assert len(s.tobytes()) == 8 + 16 + 3 * 48 + 3 * W * 4
    for bad in (b"", s.tobytes()[:-1], b"X" + s.tobytes()[1:]):
        with pytest.raises(ValueError, match="frombytes"):
            SlotState.frombytes(bad)
    with pytest.raises(ValueError, match="3 rows of words but 1 records"):
        SlotState(words, [_info()])
