"""Session pairs when the clips of a session come and go (include/talkshow_hip.h, "session pairs"): a pair restarts together, is
dissolved by a restart that lists both slots, moves between sessions as two saved states, and is never touched on one side only.

Yardsticks: the one-shot `GatedPixelCNN.run(..., guide=)` on the new clip alone (with `given=` its first rows where the clip was carried
over), and a twin session that never made the call for every slot the call does not list.  EQUALITY of codes and log-probability bits.
The `pix_small` golden's network, S = 5 slots over 19 session rows.  Every test fails on a build without the feature.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, CLIP0 = 57, 2
S, H = 5, 19
HOWS = ["uniforms", "philox"]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def net(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    rng = np.random.default_rng(5)
    m.labels = (np.arange(S) * 3 + 1) % n_cls
    m.aud = rng.standard_normal((S, H, 256)).astype(F32)
    m.u = (0.999 * rng.random((S, H, 2))).astype(F32)
    return m


class Sess:
    """A session whose slot b hears aud[src[b], r + shift[b]] at session row r; collects what its steps return."""

    def __init__(self, m, how, n_slots=S, pairs=None, labels=None, src=None):
        self.m, self.how, self.n = m, how, n_slots
        self.st = m.open_stream(m.labels[:n_slots] if labels is None else labels, n_slots, 8, pairs=pairs)
        self.src, self.shift = list(range(n_slots)) if src is None else list(src), [0] * n_slots
        self.codes, self.lps, self.at = [], [], 0

    def rows(self, s, e):
        return [(self.src[b], slice(s + self.shift[b], e + self.shift[b])) for b in range(self.n)]

    def step(self, hc, **kw):
        s, e = self.at, self.at + hc
        aud = torch.from_numpy(np.stack([self.m.aud[b, r] for b, r in self.rows(s, e)])).cuda()
        if self.how == "uniforms":
            d = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.stack([self.m.u[b, r] for b, r in self.rows(s, e)]))
        else:
            d = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=CLIP0)
        c, lp = self.st.step(aud, **d, logprobs=True, **kw)
        self.codes.append(_np(c)), self.lps.append(_bits(lp))
        self.at = e
        return self

    def to(self, r):
        while self.at < r:
            self.step(min(4, r - self.at))
        return self

    def out(self):
        return np.concatenate(self.codes, 1), np.concatenate(self.lps, 1)


def one_shot(m, how, label, b, rows, clip, guide=None, head=None):
    """`run` on one clip alone: label, the audio / uniforms aud[b, rows]; guide: (scale, shadow label, shadow's b, shadow's rows)."""
    if how == "uniforms":
        d = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(m.u[b, rows][None]))
    else:
        d = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=SEED, clip_index0=clip)
    g = None if guide is None else [{"scale": guide[0], "id": int(guide[1]), "aud_rows": m.aud[guide[2], guide[3]]}]
    out = m.run(np.array([label], np.int64), torch.from_numpy(m.aud[b, rows][None]).cuda(), **d, logprobs=True, guide=g,
                given=None if head is None else [head])
    return _np(out[0])[0], _bits(out[2])[0]


@pytest.mark.parametrize("how", HOWS)
def test_a_pair_restarts_together_and_the_others_keep_their_bits(net, how):
    m = net
    a = Sess(m, how, pairs={0: (1, 2.0)})
    twin = Sess(m, how, pairs={0: (1, 2.0)}).to(H)
    a.to(5)
    a.st.restart([3, 4], label=[0, 2], clip_indices=[20, 21], pairs={3: (4, 2.0)})
    assert a.st.pairs == {0: (1, 2.0), 3: (4, 2.0)} and list(a.st.slot_rows) == [5, 5, 5, 0, 0]
    a.to(11)
    a.st.restart([4, 3], label=[1, 3], clip_indices=[31, 30], pairs={4: (3, -0.5)})      # the roles swap in the next clip
    assert a.st.pairs == {0: (1, 2.0), 4: (3, -0.5)}
    a.to(H)
    c, lp = a.out()
    tc, tlp = twin.out()
    for b in (0, 1, 2):
        assert np.array_equal(c[b], tc[b]) and np.array_equal(lp[b], tlp[b]), b
    for b in (3, 4):
        assert np.array_equal(c[b, :5], tc[b, :5]) and np.array_equal(lp[b, :5], tlp[b, :5]), b
    rc, rlp = one_shot(m, how, 0, 3, slice(5, 11), 20, guide=(2.0, 2, 4, slice(5, 11)))
    assert np.array_equal(c[3, 5:11], rc) and np.array_equal(lp[3, 5:11], rlp)
    assert np.array_equal(c[4, 5:11], rc) and np.array_equal(lp[4, 5:11], rlp)
    pc, _ = one_shot(m, how, 0, 3, slice(5, 11), 20)
    assert (pc != rc).any(), "guidance moved no code: the equality would be vacuous"
    rc, rlp = one_shot(m, how, 1, 4, slice(11, H), 31, guide=(-0.5, 3, 3, slice(11, H)))
    assert np.array_equal(c[4, 11:], rc) and np.array_equal(lp[4, 11:], rlp)
    assert np.array_equal(c[3, 11:], rc) and np.array_equal(lp[3, 11:], rlp)
    pc, _ = one_shot(m, how, 1, 4, slice(11, H), 31)
    assert (pc != rc).any()
    rc, rlp = one_shot(m, how, m.labels[0], 0, slice(0, H), CLIP0, guide=(2.0, m.labels[1], 1, slice(0, H)))
    assert np.array_equal(c[0], rc) and np.array_equal(lp[0], rlp)      # the standing pair, on the restart graph keys from row 5 on


@pytest.mark.parametrize("how", HOWS)
def test_a_restart_that_lists_both_without_pairs_dissolves_the_pair(net, how):
    m = net
    a = Sess(m, how, pairs={0: (1, 2.0), 3: (4, 2.0)}).to(5)
    a.st.restart([1, 0], label=[2, 3], clip_indices=[11, 10])
    assert a.st.pairs == {3: (4, 2.0)}
    a.to(H)
    c, lp = a.out()
    for b, label, clip in ((0, 3, 10), (1, 2, 11)):                     # two plain clips from row 5 on
        rc, rlp = one_shot(m, how, label, b, slice(5, H), clip)
        assert np.array_equal(c[b, 5:], rc) and np.array_equal(lp[b, 5:], rlp), b
    assert (c[0, 5:] != c[1, 5:]).any()
    rc, rlp = one_shot(m, how, m.labels[3], 3, slice(0, H), CLIP0 + 3, guide=(2.0, m.labels[4], 4, slice(0, H)))
    assert np.array_equal(c[3], rc) and np.array_equal(lp[3], rlp)


def test_one_side_of_a_pair_is_never_restarted_or_loaded_alone(net):
    m, lib = net, _lib.load()
    a = Sess(m, "philox", pairs={3: (4, 2.0)}).to(7)
    twin = Sess(m, "philox", pairs={3: (4, 2.0)}).to(H)
    state = a.st.save([0])
    before = (a.st.rows, list(a.st.slot_rows), a.st.pairs, a.st.graph_captures())
    with pytest.raises(ValueError, match="session pairs: slot 3 is paired with slot 4: list both"):
        a.st.restart([3], label=1)
    with pytest.raises(ValueError, match="session pairs: slot 4 is paired with slot 3: list both"):
        a.st.restart([0, 4], label=1)
    with pytest.raises(ValueError, match="session pairs: slot 4 is paired with slot 3: list both"):
        a.st.load([4], state)
    with pytest.raises(ValueError, match="session pairs: slot 3 is paired with slot 4: list both"):
        a.st.fork(0, [2, 3])
    with pytest.raises(ValueError, match="cannot pair at session row 7"):
        a.st.restart([0, 1], label=1, pairs={0: 2})                     # slot 2 is not restarted: nothing of the call is done
    with pytest.raises(ValueError, match="slot 1 and slot 0 cannot pair at session row 7"):
        a.st.restart([1], label=1, pairs={1: 0})                        # slot 0 is in the middle of its clip
    # the library's own refusal, behind the wrapper's
    i32, i64 = C.c_int32 * 1, C.c_int64 * 1
    assert lib.ts_pixelcnn_stream_restart(a.st._h, i32(3), 1, i64(1), None, i64(9), _lib.stream_ptr()) != 0
    assert lib.ts_last_error().decode() == "session pairs: slot 3 is paired with slot 4: list both"
    words = state.words.contiguous()
    info = (_lib.TsSlotInfo * 1)()
    for k, _ in _lib.TsSlotInfo._fields_:
        setattr(info[0], k, int(state.infos[0][k]))
    assert lib.ts_pixelcnn_stream_load(a.st._h, i32(4), 1, _lib.dptr(words), 1, None, info, None, _lib.stream_ptr()) != 0
    assert lib.ts_last_error().decode() == "session pairs: slot 4 is paired with slot 3: list both"
    assert (a.st.rows, list(a.st.slot_rows), a.st.pairs, a.st.graph_captures()) == before
    a.to(H)
    for x, y in zip(a.out(), twin.out()):
        assert np.array_equal(x, y)                                      # no refusal left a trace


@pytest.mark.parametrize("how", HOWS)
def test_a_guided_clip_moves_to_another_session_as_two_states(net, how):
    m = net
    a = Sess(m, how, pairs={0: (1, 2.0)}).to(7)
    state = a.st.save([0, 1])
    head = a.out()[0][0]
    assert len(head) == 7 and np.array_equal(a.out()[0][1], head)
    # a session of 3 slots, 4 rows old: slot 2 carries clip 0 on, slot 0 its shadow; slot 1 stays plain
    t = Sess(m, how, n_slots=3, labels=m.labels[[4, 2, 3]], src=[4, 2, 3]).to(4)
    twin = Sess(m, how, n_slots=3, labels=m.labels[[4, 2, 3]], src=[4, 2, 3]).to(16)
    t.st.load([2, 0], state, clip_indices=[40, 41], pairs={2: (0, 2.0)})
    assert t.st.pairs == {2: (0, 2.0)} and list(t.st.slot_rows) == [7, 4, 7]
    t.src[2], t.shift[2], t.src[0], t.shift[0] = 0, 3, 1, 3               # session row 4 is the clips' row 7
    t.to(16)
    c, lp = t.out()
    rc, rlp = one_shot(m, how, m.labels[0], 0, slice(0, H), 40, guide=(2.0, m.labels[1], 1, slice(0, H)), head=head)
    assert np.array_equal(c[2, 4:], rc[7:]) and np.array_equal(lp[2, 4:], rlp[7:])
    assert np.array_equal(c[0, 4:], rc[7:]) and np.array_equal(lp[0, 4:], rlp[7:])
    pc, _ = one_shot(m, how, m.labels[0], 0, slice(0, H), 40, head=head)
    assert (pc[7:] != rc[7:]).any(), "guidance moved no code: the equality would be vacuous"
    tc, tlp = twin.out()
    assert np.array_equal(c[1], tc[1]) and np.array_equal(lp[1], tlp[1])
    # loaded without `pairs`, the two states are two plain clips
    u = Sess(m, how, n_slots=3, labels=m.labels[[4, 2, 3]], src=[4, 2, 3]).to(4)
    u.st.load([2, 0], state, clip_indices=[40, 41])
    assert u.st.pairs == {}
    u.src[2], u.shift[2], u.src[0], u.shift[0] = 0, 3, 1, 3
    u.to(16)
    assert np.array_equal(u.out()[0][2, 4:], pc[7:])


def test_a_load_of_unequal_clip_rows_forms_no_pair(net):
    m = net
    a = Sess(m, "philox").to(3)
    a.st.restart([2], label=1)
    a.to(7)
    state = a.st.save([0, 2])
    assert [o["rows"] for o in state.infos] == [7, 4]
    t = Sess(m, "philox", n_slots=3).to(4)
    before = (t.st.rows, list(t.st.slot_rows), t.st.pairs)
    with pytest.raises(ValueError, match="session pairs: slot 2 holds a clip of 7 rows, slot 0 one of 4: a shadow carries"):
        t.st.load([2, 0], state, pairs={2: 0})
    assert (t.st.rows, list(t.st.slot_rows), t.st.pairs) == before
    t.st.load([2, 0], state)                                             # the states themselves are fine
    with pytest.raises(ValueError, match="slot 2 holds a clip of 7 rows, slot 0 one of 4"):
        t.st._declare([2], [0], [1.0])                                   # the library's own check, behind the load
    assert t.st.pairs == {}
