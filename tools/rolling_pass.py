"""What clips that come and go cost on a streaming session: same process, interleaved, against the plain session and against what a host
had to do before slots could restart.

Full-size code predictor (2 048 classes, dim 256, 15 layers); one region = the next --rows code rows of the leg in steps of --step rows
(32 slots, 75 rows, 15-row steps: five 2 s chunks), Philox:
  (A)  the plain session                             one session of --clips slots, `ts_pixelcnn_stream_step`
  (A') the same on a session of its own              the run-to-run spread of (A) inside this process
  (B)  (A) with --restarts slots restarted ahead     `ts_pixelcnn_stream_restart` (other slots every step, new label and clip index), then the
       of every step                                 step on the graphs of a restarted session: one reset launch and the staging of two
                                                     small tables per step over (A)
  (C)  what a host does without restarts             --clips sessions of ONE clip, stepped in turn: a user who arrives late gets a session
                                                     of their own
Timed regions alternate A A' B C A A' B C ... after a warm-up of four regions per leg (every buffer phase met, every graph captured: the
captures inside the timed regions are reported and should be 0); HIP events on the stream; the figure is the median region.  Nothing is
asserted about the ratios.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/rolling_pass.py --regions 5 --out profiles/rolling_pass.json
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
    ap.add_argument("--restarts", type=int, default=4)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    pix = w.generator
    NC = pix.n_classes
    B, H, HC, NR = a.clips, a.rows, a.step, a.restarts
    mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
    aud = w.audioencoder.forward_nlc(mfcc)
    chunks = [aud[:, r:r + HC].contiguous() for r in range(0, H, HC)]
    solo = [[ch[b:b + 1].contiguous() for b in range(B)] for ch in chunks]
    ids = (np.arange(B) % NC).astype(np.int64)
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1)
    sessions = {k: pix.open_stream(ids, B, HC) for k in ("a", "a2", "b")}
    singles = [pix.open_stream(ids[b:b + 1], 1, HC) for b in range(B)]
    turn = [0]

    def leg(name, restart):
        st = sessions[name]

        def run():
            out = None
            for ch in chunks:
                if restart:
                    slots = [(turn[0] * NR + i) % B for i in range(NR)]
                    turn[0] += 1
                    st.restart(slots, [(turn[0] + s) % NC for s in slots], clip_indices=[1000 * turn[0] + s for s in slots])
                out = st.step(ch, **draw)
            return out
        return run

    def leg_c():
        out = None
        for k in range(len(chunks)):
            for b, st in enumerate(singles):
                out = st.step(solo[k][b], clip_index0=b, **draw)
        return out
    legs = (leg("a", False), leg("a2", False), leg("b", True), leg_c)
    for _ in range(4):                                       # warm-up: 75 rows = phases 0, then 3 + (r0 % 4) for r0 = 15 .. 285: all four met
        for fn in legs:
            fn()
    torch.cuda.synchronize()
    caps = lambda: dict({k: s.graph_captures() for k, s in sessions.items()}, c=sum(s.graph_captures() for s in singles))   # noqa: E731
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
    for s in list(sessions.values()) + singles:
        s.close()
    ta, ta2, tb, tc = acc
    med = statistics.median
    r3 = lambda xs: [round(x, 3) for x in xs]                # noqa: E731
    steps = len(chunks)
    doc = dict(
        tool="rolling_pass", device=torch.cuda.get_device_name(0), slots=B, code_rows=H, step_rows=HC, steps_per_region=steps,
        restarts_per_step=NR, regions=a.regions,
        a_plain_ms=r3(ta), a2_plain_again_ms=r3(ta2), b_restarting_ms=r3(tb), c_one_session_per_clip_ms=r3(tc),
        a_plain_ms_median=round(med(ta), 3), a2_plain_again_ms_median=round(med(ta2), 3), b_restarting_ms_median=round(med(tb), 3),
        c_one_session_per_clip_ms_median=round(med(tc), 3),
        a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
        spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
        b_minus_a_per_step_us=round(1000 * (med(tb) - med(ta)) / steps, 3),
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
