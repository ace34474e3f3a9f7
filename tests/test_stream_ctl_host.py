"""Sampling controls on the streaming sessions, host side (no GPU): the prototypes of the two new entries, what `PixelCNNStream.step`
refuses before any device work (the session's row counter stands still and no step entry is called), the `from_row` word that
`rep_table` leaves 0 for every one-shot pass, and the session defaults of `open_stream`.  The session here is a stand-in without a device
handle: everything `step` checks is host code, so a refusal has to come before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from talkshow_amd import _lib
from talkshow_amd.modules import PixelCNNStream

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, NC, HC = 3, 128, 4, 4


def test_header_and_prototype_argument_counts_agree():
    text = open(os.path.join(REPO, "include", "talkshow_hip.h")).read()
    for name, n in (("ts_pixelcnn_stream_step_ctl", 20), ("ts_pixelcnn_stream_captures", 1)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in talkshow_hip.h"
        assert len(m.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    step = _lib.SIGNATURES["ts_pixelcnn_stream_step"][1]
    ctl = _lib.SIGNATURES["ts_pixelcnn_stream_step_ctl"][1]
    assert ctl[:len(step) - 1] == step[:-1] and ctl[-1] == step[-1]        # the step's arguments, the pieces, the stream
    assert _lib.SIGNATURES["ts_pixelcnn_stream_captures"][0] is C.c_int64
    lib = _lib.load()
    assert hasattr(lib, "ts_pixelcnn_stream_step_ctl") and hasattr(lib, "ts_pixelcnn_stream_captures")
    assert lib.ts_pixelcnn_stream_captures(None) == -1


class _Spy:
    """The library, with the session entries replaced: the row counter of the stand-in session, and a record of step calls."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name == "ts_pixelcnn_stream_rows":
            return lambda h: 17
        if name in ("ts_pixelcnn_stream_step", "ts_pixelcnn_stream_step_ctl"):
            return lambda *a: self.calls.append(name) or 0
        return getattr(self._lib, name)


@pytest.fixture
def session(monkeypatch):
    import types
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    st = object.__new__(PixelCNNStream)
    st.net = types.SimpleNamespace(input_dim=V, n_classes=NC, _dev=lambda: torch.device("cpu"))
    st.B, st.max_rows, st._h = B, HC, None
    st.defaults = {"sampling": None, "style": None, "code_bias": None, "repeat": None}
    st._labels = np.array([0, 1, 2], np.int64)
    return st, spy


def _ban_all():
    t = np.zeros((2, V), np.float32)
    t[1] = -np.inf
    return t


REFUSALS = [
    ("g_b > Hc", dict(given=[None, np.zeros((HC + 1, 2), np.int64), None]), "clip 1"),
    ("a code outside the vocabulary", dict(given=[None, None, np.array([[0, V]])]), "clip 2"),
    ("a style track", dict(style=[None, np.ones((HC, NC), np.float32), None]), "clip 1"),
    ("a window of 65", dict(repeat=[(3, 0.0, 0.0), (3, 0.0, 0.0), (65, 0.0, 0.0)]), "clip 2"),
    ("a bias column without an allowed code", dict(code_bias=[None, _ban_all(), None]), "clip 1"),
    ("a bad sampling record", dict(sampling=[None, None, (0.0, 1.0, 0)]), "clip 2"),
]


@pytest.mark.parametrize("what, kw, names", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_step_refuses_and_names_the_clip(session, what, kw, names):
    st, spy = session
    aud = torch.zeros((B, HC, 256))
    rows = st.rows
    with pytest.raises(ValueError, match=names):
        st.step(aud, mode=_lib.TS_SAMPLE_PHILOX, **kw)
    assert st.rows == rows and spy.calls == [], what


def test_greedy_step_with_a_table_is_refused_with_the_tables_message(session):
    """The table's own message (`_lib.sampling_table`, `ctl_table`): it concerns the step's mode, so it names no clip."""
    st, spy = session
    aud = torch.zeros((B, HC, 256))
    for kw in (dict(sampling=(0.8, 1.0, 0)), dict(code_bias=np.zeros((2, V), np.float32)), dict(repeat=(3, 1.0, 0.0))):
        with pytest.raises(ValueError, match="TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX"):
            st.step(aud, mode=_lib.TS_SAMPLE_GREEDY, **kw)
    with pytest.raises(ValueError, match="opened for B=3"):
        st.step(torch.zeros((B + 1, HC, 256)))
    assert st.rows == 17 and spy.calls == []


def test_rep_table_leaves_from_row_at_zero():
    lib = _lib.load()
    recs = [(5, 0.5, 0.25), (0, 1.0, 1.0), (64, -0.5, 0.125)]
    arr = (_lib.TsRepeat * 3)()
    for b, (w, p, f) in enumerate(recs):
        arr[b].window, arr[b].presence, arr[b].frequency, arr[b].reserved = w, p, f, 0
    for n, Bs in ((3, 3), (1, 4)):
        words = np.full(4 * Bs, 99, np.int32)
        assert lib.ts_debug_rep_table(arr, n, Bs, V, words.ctypes.data_as(C.POINTER(C.c_int32))) == 0, lib.ts_last_error().decode()
        words = words.reshape(Bs, 4)
        assert np.all(words[:, 3] == 0), "one-shot passes count min(r - 0, W) entries: the word stays 0"
        for b in range(Bs):
            w, p, f = recs[b if n == 3 else 0]
            assert words[b, 0] == w and np.array_equal(words[b, 1:3].view(np.float32), np.array([p, f], np.float32))
    arr[2].reserved = 4                                                        # the public record cannot carry the word
    assert lib.ts_debug_rep_table(arr, 3, 3, V, words.ctypes.data_as(C.POINTER(C.c_int32))) != 0
    assert "clip 2" in lib.ts_last_error().decode() and "reserved" in lib.ts_last_error().decode()
    assert lib.ts_debug_rep_table(arr, 2, 3, V, words.ctypes.data_as(C.POINTER(C.c_int32))) != 0


def test_open_stream_defaults_are_overridden_by_step_keywords(session):
    st, _ = session
    dev = torch.device("cpu")
    t0, t1 = np.zeros((2, V), np.float32), np.ones((2, V), np.float32)
    st.defaults = {"sampling": (0.5, 0.9, 7), "style": np.array([0, 0, 1, 0], np.float32), "code_bias": t0, "repeat": (16, 1.0, 0.0)}
    mode = _lib.TS_SAMPLE_PHILOX
    lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows = st._pieces(HC, mode, dev, None, False, None, None, None, None)
    assert lp is None and block is None and table is None
    assert n_ctl == B and all((ctl[b].temperature, ctl[b].top_k) == (0.5, 7) for b in range(B))
    assert np.array_equal(btab, t0[None]) and bidx.tolist() == [0, 0, 0]
    assert n_rep == B and all((rtab[b].window, rtab[b].presence) == (16, 1.0) for b in range(B))
    assert srows.shape == (B, NC) and np.array_equal(srows, np.tile([0, 0, 1, 0], (B, 1)))
    out = st._pieces(HC, mode, dev, [None, (2.0, 1.0, 0), None], True, [None, np.ones((2, 2), np.int64), None], [None, np.full(NC, 0.25), None],
                     [None, t1, None], [(0, 0.0, 0.0), None, (3, 0.5, 0.5)])
    lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows = out
    assert lp == "new" and [ctl[b].temperature for b in range(B)] == [1.0, 2.0, 1.0]
    assert np.array_equal(btab, t1[None]) and bidx.tolist() == [-1, 0, -1]
    assert [rtab[b].window for b in range(B)] == [0, 0, 3]
    assert block.shape == (B, HC, 2) and table.tolist() == [0, 2, 0]
    assert np.array_equal(srows, np.array([[1, 0, 0, 0], [.25, .25, .25, .25], [0, 0, 1, 0]], np.float32))   # None: the clip's own label
    st.defaults = {"sampling": None, "style": None, "code_bias": None, "repeat": None}
    assert st._pieces(HC, mode, dev, None, False, None, None, None, None) == (None, None, 0, None, None, None, 0, None, None, None)
