"""What the sampler set-up paths REFUSE, and with which words: the return code and the exact `ts_last_error()` text of every refusal site of
`ts_pixelcnn_generate_mixed*` (through `ts_pixelcnn_generate_mixed_repeat`), of a session step (`ts_pixelcnn_stream_step_ctl`), of
`ts_pixelcnn_generate_lp` and of the six kernel-level entries `ts_op_sample_ctl / _lp / _given / _keep / _bias / _repeat`.

tests/golden/sampler_refusals.json is the table: entry, the fault (a name of FAULTS below: which arguments of an otherwise valid call are
made faulty), whether the call brings a sampling table, the return code and the text.  The texts were recorded from the library BEFORE the
set-up paths were merged into one record and one `op_sample` body, so the table pins the messages, their `who` and the ORDER of the checks
(a fault is reached only if every check ahead of it passes).  Faults that depend on a combination of pieces — a bias or repetition records
without controls, records without tables, a mask without given codes — run once with a sampling table and once without: the second takes
the neutral-record path, which names another entry.

Every call is refused before anything is launched.  Not in the table: refusals only a failing allocation or a faulting kernel could reach,
and the row-counter overflow of a session (2^30 rows away).  Shapes: the 3-layer network of tests/test_gpu_keep_canary.py (V = 256), B = 3;
mixed pass of 9, 2 and 1 code rows (two 8-row chunks), one-shot call and session step of 8 rows.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from talkshow_amd import _lib
from test_gpu_keep_canary import V, nets  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
B, H, HC = 3, 9, 8
LENS = np.asarray([36, 8, 4], np.int32)
GREEDY, UNIFORMS, PHILOX, FORCED = _lib.TS_SAMPLE_GREEDY, _lib.TS_SAMPLE_UNIFORMS, _lib.TS_SAMPLE_PHILOX, _lib.TS_TEACHER_FORCED
with open(os.path.join(os.path.dirname(__file__), "golden", "sampler_refusals.json")) as _f:
    TABLE = json.load(_f)["rows"]

MIXED, STEP, ONE_SHOT = "ts_pixelcnn_generate_mixed_repeat", "ts_pixelcnn_stream_step_ctl", "ts_pixelcnn_generate_lp"
OPS = tuple(f"ts_op_sample_{s}" for s in ("ctl", "lp", "given", "keep", "bias", "repeat"))

# the parameters of every entry, in order (include/talkshow_hip.h, talkshow_hip_debug.h)
_OP_HEAD = ("ctx", "logits", "B", "V", "mode", "uniforms", "seed", "clip_index0", "position", "ctl_host", "n_ctl", "idx")
_OP_BIAS = ("logprob", "given_rows_host", "keep", "given", "kept", "logits_copy", "bias", "n_bias", "bias_index_host", "column")
PARAMS = {
    MIXED: ("p", "label", "aud", "lens_host", "lens_dev", "B", "H_max", "mode", "uniforms", "seed", "clip_index", "codes", "ctl_host", "n_ctl",
            "logprob", "given", "given_rows_host", "given_rows_dev", "keep", "style", "style_rows", "bias", "n_bias", "bias_index_host",
            "rep_host", "n_rep", "stream"),
    STEP: ("st", "aud", "Hc", "mode", "uniforms", "seed", "clip0", "codes", "ctl_host", "n_ctl", "logprob", "given", "given_rows_host", "style",
           "bias", "n_bias", "bias_index_host", "rep_host", "n_rep", "stream"),
    ONE_SHOT: ("p", "label", "aud", "B", "H", "mode", "uniforms", "seed", "clip0", "codes", "logits", "pre_codes", "pre_aud", "H0", "ctl_host",
               "n_ctl", "logprob", "stream"),
    OPS[0]: _OP_HEAD + ("kept", "stream"),
    OPS[1]: _OP_HEAD + ("kept", "logprob", "stream"),
    OPS[2]: _OP_HEAD + ("logprob", "forced_host", "given", "stream"),
    OPS[3]: _OP_HEAD + ("logprob", "given_rows_host", "keep", "given", "stream"),
    OPS[4]: _OP_HEAD + _OP_BIAS + ("stream",),
    OPS[5]: _OP_HEAD + _OP_BIAS + ("rep_host", "n_rep", "history", "ring_out", "stream"),
}

# faults of the sampling table, the same for every entry that builds one (ctl_table): they need a table, so they run with one only
_CTL = {"ctl_greedy": dict(mode=GREEDY), "ctl_n": dict(n_ctl=2), "ctl_record": dict(ctl_host="bad_ctl")}
# the pieces whose refusals depend on which other pieces came: with a sampling table and without
_BOTH = ("greedy", "greedy_bias_only", "greedy_rep_only", "keep_without_given", "given_without_rows", "given_rows_range", "bias_n", "bias_index",
         "bias_index_null", "rep_n", "rep_record", "rows_negative", "given_without_codes", "codes_without_rows", "mask_without_rows")
_PASS = {"greedy": dict(mode=GREEDY),
         "greedy_bias_only": dict(mode=GREEDY, rep_host=None, n_rep=0),
         "greedy_rep_only": dict(mode=GREEDY, bias=None, n_bias=0, bias_index_host=None),
         "bias_n": dict(n_bias=B + 1), "bias_n_zero": dict(n_bias=0), "bias_index": dict(bias_index_host="bad_index"),
         "bias_index_null": dict(bias_index_host=None),
         "rep_n": dict(n_rep=2), "rep_record": dict(rep_host="bad_rep"),
         "given_without_rows": dict(given_rows_host=None), "given_rows_range": dict(given_rows_host="long_rows")}
FAULTS = {
    MIXED: dict(_CTL, **_PASS, null_aud=dict(aud=None), null_label=dict(label=None, style=None, style_rows=0), shape_B=dict(B=0),
                shape_H=dict(H_max=0), style_rows=dict(style_rows=2), mode=dict(mode=FORCED), uniforms=dict(mode=UNIFORMS),
                short_clip=dict(lens_host="short_lens"), order=dict(lens_host="rising_lens"), rows=dict(H_max=8),
                keep_without_given=dict(given=None, given_rows_host=None)),
    STEP: dict(_CTL, **_PASS, null_aud=dict(aud=None), null_st=dict(st=None), empty=dict(Hc=0), long=dict(Hc=HC + 1), mode=dict(mode=FORCED),
               uniforms=dict(mode=UNIFORMS)),
    ONE_SHOT: dict(_CTL, ctl_forced=dict(mode=FORCED), null_aud=dict(aud=None), shape_B=dict(B=0), shape_H0=dict(H0=-1), mode=dict(mode=4),
                   uniforms=dict(mode=UNIFORMS, uniforms=None), prefix=dict(H0=2)),
}
_OP = dict(null_logits=dict(logits=None), shape_B=dict(B=0), shape_V=dict(V=0), uniforms=dict(uniforms=None))
FAULTS[OPS[0]] = dict(_CTL, **_OP, no_table=dict(ctl_host=None, n_ctl=0), mode=dict(mode=4))
FAULTS[OPS[1]] = dict(_CTL, **_OP, mode=dict(mode=4), kept_without_table=dict(ctl_host=None, n_ctl=0, kept="kept"),
                      kept_without_table_or_logprob=dict(ctl_host=None, n_ctl=0, kept="kept", logprob=None), null_logits_no_logprob=dict(logits=None, logprob=None))
FAULTS[OPS[2]] = dict(_CTL, **_OP, mode=dict(mode=FORCED), null_forced=dict(forced_host=None), position=dict(position=0x7ffffff1))
FAULTS[OPS[3]] = dict(_CTL, **_OP, mode=dict(mode=FORCED), null_given=dict(given=None), position=dict(position=0x7ffffff1),
                      rows_negative=dict(given_rows_host="negative_rows"))
_OP_PASS = dict(_CTL, **_OP, column=dict(column=2), position=dict(position=0x7ffffff1), rows_negative=dict(given_rows_host="negative_rows"),
                given_without_codes=dict(given=None), codes_without_rows=dict(given_rows_host=None, keep=None),
                mask_without_rows=dict(given_rows_host=None, given=None), greedy=dict(mode=GREEDY), bias_n=dict(n_bias=B + 1),
                bias_index=dict(bias_index_host="bad_index"))
FAULTS[OPS[4]] = dict(_OP_PASS, null_bias=dict(bias=None), bias_index_null=dict(bias_index_host=None))
FAULTS[OPS[5]] = dict(_OP_PASS, bias_index_null=dict(bias_index_host=None), rep_n=dict(n_rep=2), rep_record=dict(rep_host="bad_rep"),
                      history=dict(history=None), nothing=dict(bias=None, bias_index_host=None, rep_host=None, n_rep=0, history=None),
                      history_without_records=dict(rep_host=None, n_rep=0), ring_without_records=dict(rep_host=None, n_rep=0, history=None, ring_out="ring"),
                      greedy_rep_only=dict(mode=GREEDY, bias=None, n_bias=0, bias_index_host=None),
                      greedy_bias_only=dict(mode=GREEDY, rep_host=None, n_rep=0, history=None))


def variants(entry, fault):
    """Whether the call brings a sampling table: the table's own faults need one, the combinations run both ways, the rest bring one."""
    return (True, False) if fault in _BOTH else (True,)


CASES = [(e, f, t) for e in PARAMS for f in FAULTS[e] for t in variants(e, f)]


def make_world(px):
    """Every valid argument by name, the tensors and host tables behind the pointers kept alive beside them; one session that has made a
    valid 8-row step, so that a refused step has a row count and a capture count to leave alone."""
    rng = np.random.default_rng(5)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def i32(*v):
        return np.asarray(v, np.int32)

    ctl, bad_ctl = (_lib.TsSampling * B)(), (_lib.TsSampling * B)()
    for b, (t, p, k) in enumerate([(0.7, 0.9, 0), (1.3, 1.0, 40), (1.0, 0.5, 0)]):
        ctl[b].temperature, ctl[b].top_p, ctl[b].top_k, ctl[b].reserved = t, p, k, 0
        bad_ctl[b].temperature, bad_ctl[b].top_p, bad_ctl[b].top_k, bad_ctl[b].reserved = (0.0 if b == 1 else t), p, k, 0
    rep, bad_rep = (_lib.TsRepeat * 1)(), (_lib.TsRepeat * 1)()
    rep[0].window, rep[0].presence, rep[0].frequency, rep[0].reserved = 4, 1.5, 0.5, 0
    bad_rep[0].window, bad_rep[0].presence, bad_rep[0].frequency, bad_rep[0].reserved = 65, 1.5, 0.5, 0
    host = dict(lens=LENS, short_lens=i32(36, 8, 3), rising_lens=i32(36, 8, 12), rows=i32(2, 1, 0), long_rows=i32(2, 1, 9), negative_rows=i32(2, -1, 0),
                forced=i32(1, 0, 1), index=i32(0, -1, 0), bad_index=i32(0, 1, 0))
    t = dict(aud=dev(rng.standard_normal((B, H, 256)).astype(np.float32)), label=dev(np.asarray([1, 3, 0], np.int64)), lens_dev=dev(LENS),
             clip=dev(np.asarray([5, 9, 2], np.int64)), codes=dev(np.full((B, H, 2), -9, np.int64)), lp=dev(np.zeros((B, H, 2), np.float32)),
             given=dev(rng.integers(0, V, (B, H, 2)).astype(np.int64)), keep=dev(rng.integers(0, 2, (B, H, 2)).astype(np.uint8)),
             style=dev(np.full((B, 1, 4), 0.25, np.float32)), bias=dev(rng.standard_normal((1, 2, V)).astype(np.float32)),
             u=dev(np.full((B, H, 2), 0.5, np.float32)), logits=dev(rng.standard_normal((B, V)).astype(np.float32)),
             idx=dev(np.full(B, -7, np.int64)), kept=dev(np.zeros((B, V), np.uint8)), history=dev(np.zeros((B, 2), np.int32)),
             ring=dev(np.zeros((B, 64), np.int32)))
    st = px.open_stream(np.asarray([1, 3, 0], np.int64), B, HC)
    st.step(t["aud"][:, :HC].contiguous(), mode=PHILOX, seed=3)
    torch.cuda.synchronize()
    hp = {k: v.ctypes.data_as(I32P) for k, v in host.items()}
    dp = {k: _lib.dptr(v) for k, v in t.items()}
    named = dict(bad_ctl=bad_ctl, bad_rep=bad_rep, bad_index=hp["bad_index"], short_lens=hp["short_lens"], rising_lens=hp["rising_lens"],
                 long_rows=hp["long_rows"], negative_rows=hp["negative_rows"], kept=dp["kept"], ring=dp["ring"])
    pieces = dict(logprob=dp["lp"], given=dp["given"], given_rows_host=hp["rows"], bias=dp["bias"], n_bias=1, bias_index_host=hp["index"],
                  rep_host=rep, n_rep=1)
    op = dict(ctx=_lib.context(0), logits=dp["logits"], B=B, V=V, mode=UNIFORMS, uniforms=dp["u"], seed=0, clip_index0=0, position=4, idx=dp["idx"],
              kept=None, logits_copy=None, column=0, history=dp["history"], ring_out=None, forced_host=hp["forced"], keep=dp["keep"], stream=None,
              **pieces)
    base = {MIXED: dict(p=px.handle(), label=dp["label"], aud=dp["aud"], lens_host=hp["lens"], lens_dev=dp["lens_dev"], B=B, H_max=H, mode=PHILOX,
                        uniforms=None, seed=7, clip_index=dp["clip"], codes=dp["codes"], given_rows_dev=None, keep=dp["keep"], style=dp["style"],
                        style_rows=1, stream=None, **pieces),
            STEP: dict(st=st._h, aud=dp["aud"], Hc=HC, mode=PHILOX, uniforms=None, seed=7, clip0=0, codes=dp["codes"], style=dp["style"], stream=None,
                       **pieces),
            ONE_SHOT: dict(p=px.handle(), label=dp["label"], aud=dp["aud"], B=B, H=HC, mode=PHILOX, uniforms=dp["u"], seed=7, clip0=0, codes=dp["codes"],
                           logits=None, pre_codes=None, pre_aud=None, H0=0, logprob=dp["lp"], stream=None)}
    for e in OPS:
        base[e] = op
    return dict(base=base, named=named, ctl=ctl, st=st, alive=(host, t, rep))


@pytest.fixture(scope="module")
def world(nets):  # noqa: F811
    w = make_world(nets[1])
    yield w
    w["st"].close()


def refuse(world, entry, fault, table):
    """The entry's valid call with the fault's arguments in place -> (return code, ts_last_error text)."""
    a = dict(world["base"][entry], ctl_host=world["ctl"] if table else None, n_ctl=B if table else 0)
    for k, v in FAULTS[entry][fault].items():
        a[k] = world["named"][v] if isinstance(v, str) else v
    lib = _lib.load()
    rc = getattr(lib, entry)(*(a[k] for k in PARAMS[entry]))
    return int(rc), lib.ts_last_error().decode()


def test_the_table_holds_every_fault_once():
    assert sorted((r["entry"], r["fault"], r["table"]) for r in TABLE) == sorted(CASES)
    for e in PARAMS:
        assert len(PARAMS[e]) == len(_lib.SIGNATURES[e][1])


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r['entry']}-{r['fault']}-{'table' if r['table'] else 'no_table'}")
def test_refusal_code_and_text(world, row):
    lib, st = _lib.load(), world["st"]._h
    rows, captures = lib.ts_pixelcnn_stream_rows(st), lib.ts_pixelcnn_stream_captures(st)
    assert rows == HC
    rc, text = refuse(world, row["entry"], row["fault"], row["table"])
    assert rc != 0, "the call was not refused"
    assert (rc, text) == (row["rc"], row["error"])
    # nothing moved: a refused session step leaves the session where it was (and so does every other refusal)
    assert lib.ts_pixelcnn_stream_rows(st) == rows and lib.ts_pixelcnn_stream_captures(st) == captures
