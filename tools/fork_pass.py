"""What saving and loading slot state costs on a streaming session: same process, interleaved, against the plain session and against what
a host had to do before a slot's state could move (replay the clip's history through `given=`).

Full-size code predictor (2 048 classes, dim 256, 15 layers); one region = the next --rows code rows of the leg in steps of --step rows
(32 slots, 75 rows, 15-row steps: five 2 s chunks), Philox:
  (A)  the plain session                             one session of --clips slots, `ts_pixelcnn_stream_step`
  (A') the same on a session of its own              the run-to-run spread of (A) inside this process
  (B)  (A) with --forks slots saved and loaded       `ts_pixelcnn_stream_save` of --forks slots and `ts_pixelcnn_stream_load` of their states
       into --forks others ahead of every step       into other slots (other slots every step, new clip indices), then the step on the graphs
                                                     of a restarted session: two small launches and four argument-carrying ones per step over (A)
  (C)  what a host does today, per clip              a session of ONE clip stepped through the clip's history as `given=` rows before it can
                                                     continue: --rows rows (C75) and 6 x --rows rows (C450).  The session is opened and its
                                                     graphs captured BEFORE the timed regions and its slot restarted ahead of each replay, so
                                                     the figure is the replay alone: a host that opens a session for the purpose pays the
                                                     opening and the captures on top
Timed regions alternate A A' B C75 C450 ... after a warm-up of four regions per leg (every buffer phase met, every graph captured: the
captures inside the timed regions are reported and should be 0); HIP events on the stream; the figure is the median region.  Nothing is
asserted.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/fork_pass.py --regions 5 --out profiles/fork_pass.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--rows", type=int, default=75)
    ap.add_argument("--step", type=int, default=15)
    ap.add_argument("--forks", type=int, default=4)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    pix = w.generator
    NC, V = pix.n_classes, pix.input_dim
    B, H, HC, NF = a.clips, a.rows, a.step, a.forks
    mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
    aud = w.audioencoder.forward_nlc(mfcc)
    chunks = [aud[:, r:r + HC].contiguous() for r in range(0, H, HC)]
    solo = [ch[0:1].contiguous() for ch in chunks]
    history = np.random.default_rng(1).integers(0, V, (1, HC, 2))          # one step's given rows (any codes cost the same)
    ids = (np.arange(B) % NC).astype(np.int64)
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1)
    sessions = {k: pix.open_stream(ids, B, HC) for k in ("a", "a2", "b")}
    single = pix.open_stream(ids[:1], 1, HC)
    turn = [0]

    def leg(name, fork):
        st = sessions[name]

        def run():
            out = None
            for ch in chunks:
                if fork:
                    src = [(turn[0] * 2 * NF + i) % B for i in range(NF)]
                    dst = [(turn[0] * 2 * NF + NF + i) % B for i in range(NF)]
                    turn[0] += 1
                    st.load(dst, st.save(src), clip_indices=[1000 * turn[0] + s for s in dst])
                out = st.step(ch, **draw)
            return out
        return run

    def leg_c(regions):
        def run():
            single.restart([0], [0], clip_indices=[0])
            out = None
            for _ in range(regions):
                for ch in solo:
                    out = single.step(ch, given=history, **draw)
            return out
        return run
    legs = (leg("a", False), leg("a2", False), leg("b", True), leg_c(1), leg_c(6))
    for _ in range(4):                                       # warm-up: 75 rows = phases 0, then 3 + (r0 % 4) for r0 = 15 .. 285: all four met
        for fn in legs:
            fn()
    torch.cuda.synchronize()
    caps = lambda: dict({k: s.graph_captures() for k, s in sessions.items()}, c=single.graph_captures())   # noqa: E731
    cap0 = caps()
    acc = [[] for _ in legs]
    for _ in range(a.regions):
        for fn, t in zip(legs, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    cap1 = caps()
    rows_done = {k: s.rows for k, s in sessions.items()}
    slot_rows_b = [int(v) for v in sessions["b"].slot_rows]
    words = int(_lib.load().ts_pixelcnn_slot_state_words(pix.handle()))
    for s in list(sessions.values()) + [single]:
        s.close()
    ta, ta2, tb, tc, tc6 = acc
    med = statistics.median
    r3 = lambda xs: [round(x, 3) for x in xs]                # noqa: E731
    steps = len(chunks)
    doc = dict(
        tool="fork_pass", device=torch.cuda.get_device_name(0), slots=B, code_rows=H, step_rows=HC, steps_per_region=steps,
        forks_per_step=NF, regions=a.regions, state_bytes_per_slot=4 * words,
        a_plain_ms=r3(ta), a2_plain_again_ms=r3(ta2), b_forking_ms=r3(tb), c_replay_1x_ms=r3(tc), c_replay_6x_ms=r3(tc6),
        a_plain_ms_median=round(med(ta), 3), a2_plain_again_ms_median=round(med(ta2), 3), b_forking_ms_median=round(med(tb), 3),
        c_replay_1x_ms_median=round(med(tc), 3), c_replay_6x_ms_median=round(med(tc6), 3), c_replay_1x_rows=H, c_replay_6x_rows=6 * H,
        a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4),
        spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
        b_minus_a_per_step_us=round(1000 * (med(tb) - med(ta)) / steps, 3),
        c_replay_ms_per_row=round(med(tc6) / (6 * H), 4),
        graph_captures_before_timed_regions=cap0, graph_captures_in_timed_regions={k: int(cap1[k] - cap0[k]) for k in cap0},
        session_rows_at_close=rows_done, slot_rows_b_at_close=slot_rows_b)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
