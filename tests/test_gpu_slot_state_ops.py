"""slot_save_kernel and slot_load_kernel (csrc/vq.hip; include/talkshow_hip.h, "slot state") on the GPU, each launched ALONE through its debug
entry (ts_debug_slot_save, ts_debug_slot_load) and compared, bit for bit, with a numpy restatement written from
`SlotClock.state_layout` / `canonical` / `load_plan`.

The discipline of tests/test_gpu_glue_ops.py: every buffer lies between two 4 KiB zones of sentinel words, every output starts out
sentinel-filled (a load's outputs start out as a session's random buffers), and after the call the zones are intact, the inputs unchanged
and the WHOLE of every output equals the restatement's image of it — so exactly the words the layout names have changed.  Floats are random
uint32 words, NaN payloads and -0.0 among them.  Every case runs eagerly and once more from a replayed graph.

Shapes: B = 3, D = 32, NL = 3, NC = 4; save at r = 0 .. 5 (the canonical rows and every ring phase), load at r' = 3 .. 6 (all four ring
phases, both P parities) and at r' = 1 (token rows below the session's row 0 are not written); one slot, slots (2, 0), one state row
into three slots, a slot / a state index out of range (nothing written); D = 256, NL = 15 once (the second round of the float4 loop:
4D / 4 = 256 float4 is one round of 256 threads, so the CR rows of 2D / 4 = 128 take half a round and the Q / P rows a whole one; D = 512
sends every thread round again); every clause of both launchers' checks."""
import numpy as np
import pytest
import torch

from talkshow_amd.streaming import SlotClock
from test_glue_host import I32, I64, U32, payload, sentinel
from test_gpu_glue_ops import Case, hip, refused, run_both  # noqa: F401  (hip: the module's fixture)

pytestmark = pytest.mark.gpu


def buffers(rng, B, D, NL, NC):
    """A session's buffers as words: random everywhere, codes in the integer ones."""
    return dict(tok=rng.integers(0, 128, (B, 4, 2)).astype(I32), Q1=payload(rng, (4, B, 4 * D)), Q0=payload(rng, (4, B, 4 * D)),
                P=payload(rng, (NL, 2, B, 4 * D)), CR=payload(rng, (NL, B, 2 * D)), ring=rng.integers(0, 128, (B, 2, 64)).astype(I32))


def save_ref(buf, bv, r, slots, hist, B, D, NL, before, labels=None, tables=None):
    L, c = SlotClock.state_layout(D, NL), SlotClock.canonical(r)
    out = before.copy()
    for i, b in enumerate(slots):
        if not 0 <= b < B:
            continue
        row = out[i]
        row[L["q1"]:L["q1"] + 4 * D] = 0 if c["q1"] else buf["Q1"][r & 3, b]
        row[L["q0a"]:L["q0a"] + 4 * D] = 0 if c["q0a"] else buf["Q0"][r & 3, b]
        row[L["q0b"]:L["q0b"] + 4 * D] = 0 if c["q0b"] else buf["Q0"][(r + 1) & 3, b]
        for l in range(1, NL):
            o = L["p"] + (l - 1) * 4 * D
            row[o:o + 4 * D] = bv[l] if c["p"] else buf["P"][l, r & 1, b]
        for l in range(NL):
            o = L["cr"] + l * 2 * D
            row[o:o + 2 * D] = buf["CR"][l, b] if labels is None else tables[l, labels[b]]
        tok = np.zeros(8, I32)
        for k in range(3):
            tok[2 * k:2 * k + 2] = -1 if k in c["tok"] else buf["tok"][b, (r - 1 - k) % 4]
        row[L["tok"]:L["tok"] + 8] = tok.view(U32)
        rep = np.full((2, 64), -1, I32)
        for k in range(min(max(hist[i], 0), 64)):
            rep[:, k] = buf["ring"][b, :, (r - 1 - k) % 64]
        row[L["rep"]:L["rep"] + 128] = rep.reshape(-1).view(U32)
    return out


def load_ref(buf, origin0, state, r, slots, index, origin, B, D, NL):
    L = SlotClock.state_layout(D, NL)
    out = {k: v.copy() for k, v in buf.items()}
    out["origin"] = origin0.copy()
    for i, b in enumerate(slots):
        if not 0 <= b < B or not 0 <= index[i] < len(state):
            continue
        row, plan = state[index[i]], SlotClock.load_plan(r, r - origin[i])
        out["Q1"][plan["q1"], b] = row[L["q1"]:L["q1"] + 4 * D]
        out["Q0"][plan["q0"][0], b] = row[L["q0a"]:L["q0a"] + 4 * D]
        out["Q0"][plan["q0"][1], b] = row[L["q0b"]:L["q0b"] + 4 * D]
        for l in range(1, NL):
            o = L["p"] + (l - 1) * 4 * D
            out["P"][l, plan["p"], b] = row[o:o + 4 * D]
        for l in range(NL):
            o = L["cr"] + l * 2 * D
            out["CR"][l, b] = row[o:o + 2 * D]
        tok = row[L["tok"]:L["tok"] + 8].view(I32)
        for k, at in enumerate(plan["tok"]):
            if at is not None:
                out["tok"][b, at] = tok[2 * k:2 * k + 2]
        rep = row[L["rep"]:L["rep"] + 128].view(I32).reshape(2, 64)
        for k, at in enumerate(plan["ring"]):
            out["ring"][b, :, at] = rep[:, k]
        out["origin"][b] = origin[i]
    return out


def save_case(name, seed, r, slots, hist, B=3, D=32, NL=3, NC=4, open_labels=False):
    rng = np.random.default_rng(seed)
    buf, bv = buffers(rng, B, D, NL, NC), payload(rng, (NL, 4 * D))
    tables, labels = payload(rng, (NL, NC, 2 * D)), rng.integers(0, NC, B).astype(I64)
    n, W = len(slots), SlotClock.state_words(D, NL)
    before = sentinel((n, W))
    want = save_ref(buf, bv, r, slots, hist, B, D, NL, before, labels if open_labels else None, tables)
    ins = dict(buf, bv=bv, tables=tables, labels=labels, slots=np.asarray(slots, I32), hist=np.asarray(hist, I32))
    data = dict(ins=ins, before=dict(state=before), want=dict(state=want))

    def call(lib, p, s, **over):
        a = dict(n=n, B=B, row=r, D=D, NL=NL, NC=NC)
        a.update({k: v for k, v in over.items() if k in a})
        p = dict(p, **{k: v for k, v in over.items() if k not in a})
        return lib.ts_debug_slot_save(p["slots"], p["hist"], a["n"], a["B"], a["row"], a["D"], a["NL"], a["NC"], p["tok"], p["Q1"], p["Q0"], p["P"],
                                      p["CR"], p["bv"], p["ring"], p["labels"] if open_labels else None, p["tables"] if open_labels else None,
                                      p["state"], s)
    return Case(name, data, call), data, call


def load_case(name, seed, r, slots, index, rows, n_states, B=3, D=32, NL=3, NC=4):
    rng = np.random.default_rng(seed)
    buf = buffers(rng, B, D, NL, NC)
    W = SlotClock.state_words(D, NL)
    state = payload(rng, (n_states, W))
    origin0 = rng.integers(-50, 50, B).astype(I32)
    origin = [r - n for n in rows]
    want = load_ref(buf, origin0, state, r, slots, index, origin, B, D, NL)
    ins = dict(state=state, slots=np.asarray(slots, I32), index=np.asarray(index, I32), org=np.asarray(origin, I32))
    data = dict(ins=ins, before=dict(buf, origin=origin0), want=want)
    n = len(slots)

    def call(lib, p, s, **over):
        a = dict(n=n, n_states=n_states, B=B, row=r, D=D, NL=NL)
        a.update({k: v for k, v in over.items() if k in a})
        p = dict(p, **{k: v for k, v in over.items() if k not in a})
        return lib.ts_debug_slot_load(p["slots"], p["index"], p["org"], a["n"], a["n_states"], a["B"], a["row"], a["D"], a["NL"], p["tok"], p["Q1"],
                                      p["Q0"], p["P"], p["CR"], p["ring"], p["origin"], p["state"], s)
    return Case(name, data, call), data, call


def test_save(hip):
    cases = []
    for r in range(6):
        cases.append(save_case(f"save r={r} slot 1", 10 + r, r, [1], [min(r, 2)])[0])
        cases.append(save_case(f"save r={r} slots (2, 0)", 20 + r, r, [2, 0], [-1, r])[0])
    cases.append(save_case("save r=0 from the open labels", 31, 0, [2, 0], [0, -1], open_labels=True)[0])
    cases.append(save_case("save r=70: a full history, a ring that has wrapped", 32, 70, [1, 2], [64, 37])[0])
    cases.append(save_case("save: slots 3 and -1 of 3 write nothing", 33, 4, [3, 1, -1], [2, 2, 2])[0])
    run_both(hip, cases)


def test_load(hip):
    cases = []
    for r in range(3, 7):
        cases.append(load_case(f"load r'={r} slot 1", 40 + r, r, [1], [0], [r - 1], 1)[0])
        cases.append(load_case(f"load r'={r} slots (2, 0)", 50 + r, r, [2, 0], [0, 1], [2, 40], 2)[0])
        cases.append(load_case(f"load r'={r}: one state row into three slots", 60 + r, r, [0, 2, 1], [1, 1, 1], [9, 9, 9], 2)[0])
    cases.append(load_case("load r'=1: token rows below the session's row 0", 71, 1, [2], [0], [1], 1)[0])
    cases.append(load_case("load r'=0", 72, 0, [0], [0], [0], 1)[0])
    cases.append(load_case("load r'=130: the history ring wraps", 73, 130, [1], [0], [200], 1)[0])
    cases.append(load_case("load: a slot and a state index out of range write nothing", 74, 5, [3, 1, 0], [0, 2, -1], [5, 5, 5], 2)[0])
    run_both(hip, cases)


def test_full_size_rows(hip):
    """D = 256, NL = 15: the network's own rows; D = 512: every thread goes round the float4 loop again."""
    cases = [save_case("save D=256 NL=15", 80, 5, [1, 0], [64, 3], B=2, D=256, NL=15)[0],
             load_case("load D=256 NL=15", 81, 6, [0, 1], [0, 0], [11, 11], 1, B=2, D=256, NL=15)[0],
             save_case("save D=512 NL=2", 82, 1, [0], [1], B=2, D=512, NL=2)[0],
             load_case("load D=512 NL=2", 83, 3, [1], [0], [3], 1, B=2, D=512, NL=2)[0]]
    run_both(hip, cases)


def test_save_then_load_moves_a_slot(hip):
    """The two kernels against each other: slot 1 at row 5 saved, loaded into slot 2 of other buffers at row 10: the entries rows 10 and 11
    read of slot 2 are the entries rows 5 and 6 read of slot 1."""
    _lib, lib, _ = hip
    rng = np.random.default_rng(90)
    B, D, NL, NC = 3, 32, 3, 4
    c, data, call = save_case("save", 91, 5, [1], [4])
    c.alloc(), c.launch(hip)
    torch.cuda.synchronize()
    state = c.z["state"].read("state").reshape(1, -1)
    src = data["ins"]
    l, ldata, _ = load_case("load", 92, 10, [2], [0], [5], 1)
    ldata["ins"]["state"] = state
    l.alloc(), l.launch(hip)
    torch.cuda.synchronize()
    got = {k: l.z[k].read(k) for k in ldata["before"]}
    assert np.array_equal(got["Q1"][10 & 3, 2], src["Q1"][5 & 3, 1]) and np.array_equal(got["Q0"][10 & 3, 2], src["Q0"][5 & 3, 1])
    assert np.array_equal(got["Q0"][11 & 3, 2], src["Q0"][6 & 3, 1]) and np.array_equal(got["P"][1:, 0, 2], src["P"][1:, 1, 1])
    assert np.array_equal(got["CR"][:, 2], src["CR"][:, 1]) and got["origin"][2] == 5
    for k in range(3):
        assert np.array_equal(got["tok"][2, (9 - k) % 4], src["tok"][1, (4 - k) % 4])
    for k in range(4):
        assert np.array_equal(got["ring"][2, :, (9 - k) % 64], src["ring"][1, :, (4 - k) % 64])
    assert np.all(got["ring"][2, :, (9 - 4) % 64] == -1)
    assert rng is not None and (B, D, NL, NC) == (3, 32, 3, 4)


SAVE_BAD = [dict(n=0), dict(n=4), dict(row=-1), dict(D=30), dict(D=0), dict(NL=0), dict(B=0)] + [{k: None} for k in
            ("slots", "hist", "tok", "Q1", "Q0", "P", "CR", "bv", "ring", "state")] + [{k: "off"} for k in ("Q1", "Q0", "P", "CR", "bv", "state")]
LOAD_BAD = [dict(n=0), dict(n=4), dict(n_states=0), dict(row=-1), dict(D=30), dict(D=0), dict(NL=0), dict(B=0)] + [{k: None} for k in
            ("slots", "index", "org", "tok", "Q1", "Q0", "P", "CR", "ring", "origin", "state")] + [{k: "off"} for k in ("Q1", "Q0", "P", "CR", "state")]


def _refusals(hip, make, bads):
    for over in bads:
        _, data, call = make()

        def bad(lib, p, s, over=over):
            o = {k: (p[k] + 4 if v == "off" else v) for k, v in over.items()}      # "off": 4 bytes past 16-byte alignment
            return call(lib, p, s, **o)
        refused(hip, f"refusal {over}", data, bad)


def test_save_refusals(hip):
    _refusals(hip, lambda: save_case("save", 95, 4, [1, 2], [1, 1]), SAVE_BAD)
    _, data, call = save_case("save", 96, 0, [1], [0], open_labels=True)
    refused(hip, "open labels without tables", data, lambda lib, p, s: lib.ts_debug_slot_save(
        p["slots"], p["hist"], 1, 3, 0, 32, 3, 4, p["tok"], p["Q1"], p["Q0"], p["P"], p["CR"], p["bv"], p["ring"], p["labels"], None, p["state"], s))
    refused(hip, "open labels with NC = 0", data, lambda lib, p, s: call(lib, p, s, NC=0))
    refused(hip, "open labels with misaligned tables", data, lambda lib, p, s: call(lib, p, s, tables=p["tables"] + 4))


def test_load_refusals(hip):
    _refusals(hip, lambda: load_case("load", 97, 4, [1, 2], [0, 0], [4, 4], 1), LOAD_BAD)
