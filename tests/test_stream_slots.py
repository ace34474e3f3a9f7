"""Slot restart, host side (no GPU): `talkshow_amd.streaming.SlotClock` against a brute-force restatement — positions, origins, clip rows
and clip indices over random restart schedules, and what a restart at row r must rewrite in a slot's slabs — and the argument rules of
`PixelCNNStream.restart`, which raise ValueError naming the slot before the library is called."""
import types

import numpy as np
import pytest
import torch

from talkshow_amd import _lib
from talkshow_amd.modules import PixelCNNStream
from talkshow_amd.streaming import SlotClock

B, NC = 3, 4


def _brute(B, events):
    """Row by row: per slot the rows since its last restart.  Returns, per slot, {session row: row inside its clip}, and the counters."""
    k, clip, row, table = [0] * B, [None] * B, 0, [dict() for _ in range(B)]
    for ev in events:
        if ev[0] == "restart":
            for b, c in zip(ev[1], ev[2]):
                k[b], clip[b] = 0, c
            continue
        for _ in range(ev[1]):
            for b in range(B):
                table[b][row] = k[b]
                k[b] += 1
            row += 1
    return table, k, clip, row


@pytest.mark.parametrize("seed", range(8))
def test_clock_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(1, 7))
    events = []
    for _ in range(30):
        if rng.random() < 0.45:
            slots = [int(b) for b in rng.choice(nb, int(rng.integers(1, nb + 1)), replace=False)]
            events.append(("restart", slots, [int(c) for c in rng.integers(0, 1000, len(slots))]))
        else:
            events.append(("step", int(rng.integers(1, 6))))
    clock = SlotClock(nb)
    for ev in events:
        if ev[0] == "restart":
            clock.restart(ev[1], ev[2])
        else:
            clock.advance(ev[1])
    table, k, clip, row = _brute(nb, events)
    assert clock.row == row and clock.slot_rows == k
    for b in range(nb):
        assert clock.clip(b, 17) == (17 + b if clip[b] is None else clip[b])
        assert clock.origin(b) == row - k[b]
        for r, kr in table[b].items():
            assert clock.origin(b, r) == r - kr
            assert [clock.position(b, r, j) for j in (0, 1)] == [2 * kr, 2 * kr + 1]


@pytest.mark.parametrize("r", range(12))
def test_rewrites_against_the_producers(r):
    """Who wrote what: row x puts its codes at ring index x % 4, Q1 for row x + 1 at (x + 1) % 4, Q0 for row x + 2 at (x + 2) % 4 and P for
    row x + 1 at parity (x + 1) & 1.  A restart at row r must rewrite every entry a row >= r reads and a row < r wrote."""
    stale = {"tok": set(), "q1": set(), "q0": set(), "p": set()}
    for x in range(r):
        if x >= r - 3:
            stale["tok"].add(x % 4)                  # layer 0 of rows r .. r + 2 looks up to three rows up
        if x + 1 >= r:
            stale["q1"].add((x + 1) % 4)
            stale["p"].add((x + 1) & 1)
        if x + 2 >= r:
            stale["q0"].add((x + 2) % 4)
    w = SlotClock.rewrites(r)
    assert stale["tok"] == set(w["tok"]) and len(w["tok"]) == min(r, 3)
    assert stale["q1"] <= set(w["q1"]) and stale["q0"] <= set(w["q0"]) and stale["p"] <= {w["p"]}
    if r >= 2:
        assert stale["q1"] == set(w["q1"]) and stale["q0"] == set(w["q0"]) and stale["p"] == {w["p"]}


class _Spy:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name == "ts_pixelcnn_stream_restart":
            return lambda h, slots, n, labels, style, clips, s: self.calls.append(
                (list(slots[:n]), None if labels is None else list(labels[:n]), list(clips[:n]))) or 0
        return getattr(self._lib, name)


@pytest.fixture
def session(monkeypatch):
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    st = object.__new__(PixelCNNStream)
    st.net = types.SimpleNamespace(input_dim=128, n_classes=NC, _dev=lambda: torch.device("cpu"))
    st.B, st.max_rows, st._h = B, 4, None
    st._labels = np.array([0, 1, 2], np.int64)
    return st, spy


REFUSALS = [
    ("slot 3", dict(slots=[0, 3], label=[0, 0])),
    ("slot -1", dict(slots=-1, label=0)),
    ("slot 1 is listed twice", dict(slots=[1, 2, 1], label=0)),
    (f"slot 2: label {NC}", dict(slots=[1, 2], label=[0, NC])),
    ("slot 1 brings both", dict(slots=[1], label=[0], style=[np.ones(NC, np.float32)])),
    ("slot 2 brings neither", dict(slots=[1, 2], label=[0, None])),
    ("slot 0 brings neither", dict(slots=[0])),
    ("slot 0: clip index -2", dict(slots=[0], label=[1], clip_indices=[-2])),
    ("slot 1: a style row holds", dict(slots=[1], style=[np.ones(NC + 1, np.float32)])),
    ("slot 1: a style row holds", dict(slots=[1], style=[np.ones((2, NC), np.float32)])),
    ("slot 2: a style weight is not finite", dict(slots=[2], style=[np.full(NC, np.inf, np.float32)])),
    ("2 slots but 3 label entries", dict(slots=[0, 1], label=[0, 1, 2])),
    ("no slot given", dict(slots=[], label=0)),
]


@pytest.mark.parametrize("names, kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_restart_refuses_and_names_the_slot(session, names, kw):
    st, spy = session
    with pytest.raises(ValueError, match=names):
        st.restart(**kw)
    assert spy.calls == [] and list(st._labels) == [0, 1, 2]


def test_restart_passes_its_tables_and_the_labels_follow(session):
    st, spy = session
    st.restart([2, 0], 3)                                     # one label for all listed slots; clip indices default to the slot numbers
    st.restart(1, 0, clip_indices=99)
    assert spy.calls == [([2, 0], [3, 3], [2, 0]), ([1], [0], [99])]
    assert list(st._labels) == [3, 0, 3]


def test_seamless_session_has_no_restart():
    from talkshow_amd.streaming import SeamlessBodyStream
    with pytest.raises(NotImplementedError, match="seamless"):
        SeamlessBodyStream.restart(object.__new__(SeamlessBodyStream), [0], 1)
