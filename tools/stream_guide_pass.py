"""What session pairs cost on a streaming session: same process, interleaved, against plain sessions of the same and of half the slots.

Full-size code predictor (2 048 classes, dim 256, 15 layers); four sessions, one per leg, opened once; one region = the next --rows code
rows of the leg's session in steps of --step rows (32 clips, 75 rows, 15-row steps: five 2 s chunks), Philox; EVERY leg under a neutral
sampling table, one all-zero shared bias table and repeat = (16, 0, 0), so that all four run the BIAS and REP arithmetic the guided
samplers imply:
  (A)  a plain session of 2 x --clips slots          clip and second conditioning as clips of their own: the chain work of (B)
  (A') the same on a session of its own              the run-to-run spread of (A) inside this process
  (B)  --clips clips, each guided at scale 2         2 x --clips slots, --clips pairs (clip b in slot b, its shadow in slot --clips + b):
                                                     `ts_pixelcnn_stream_step_guided`, sample_ctl_guide_kernel, two more small tables staged per step
  (C)  a plain session of --clips slots              the clips alone
A step costs the same at every row of a session, so the regions of a leg follow each other on its session.  Timed regions alternate
A A' B C A A' B C ... after a warm-up of four regions per leg (every buffer phase met, every graph captured: the captures inside the timed
regions are reported and should be 0); HIP events on the stream; the figure is the median region.  Nothing is asserted.
One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/stream_guide_pass.py --regions 5 --out profiles/stream_guide_pass.json
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
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    pix = w.generator
    NC, V = pix.n_classes, pix.input_dim
    B, H, HC = a.clips, a.rows, a.step
    mfcc = torch.from_numpy(synth.mfcc_features(B, 2 * B, 4 * H)).cuda()
    aud = w.audioencoder.forward_nlc(mfcc)                                   # slots 0 .. B-1 the clips, B .. 2B-1 the second conditionings
    chunks2 = [aud[:, r:r + HC].contiguous() for r in range(0, H, HC)]
    chunks1 = [c[:B].contiguous() for c in chunks2]
    ids = (np.arange(2 * B) % NC).astype(np.int64)
    ids[B:] = (ids[B:] + 1) % NC                                             # a shadow under another speaker, too
    kw = dict(sampling=(1.0, 1.0, 0), code_bias=np.zeros((2, V), np.float32), repeat=(16, 0.0, 0.0))
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1)
    sessions = {"a": pix.open_stream(ids, 2 * B, HC), "a2": pix.open_stream(ids, 2 * B, HC),
                "b": pix.open_stream(ids, 2 * B, HC, pairs={b: (B + b, a.scale) for b in range(B)}), "c": pix.open_stream(ids[:B], B, HC)}

    def leg(name, chunks):
        st = sessions[name]

        def run():
            out = None
            for ch in chunks:
                out = st.step(ch, **draw, **kw)
            return out
        return run
    legs = (leg("a", chunks2), leg("a2", chunks2), leg("b", chunks2), leg("c", chunks1))
    first = [fn() for fn in legs]                            # (the first of the four warm-up regions)
    moved = float((first[2][:B] != first[0][:B]).float().mean())
    shadows_follow = bool(torch.equal(first[2][:B], first[2][B:]))
    for _ in range(3):                                       # warm-up: 75 rows = phases 0, then 3 + (r0 % 4) for r0 = 15 .. 285: all four met
        for fn in legs:
            fn()
    torch.cuda.synchronize()
    cap0 = {k: s.graph_captures() for k, s in sessions.items()}
    acc = [[] for _ in legs]
    for _ in range(a.regions):
        for fn, t in zip(legs, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    cap1 = {k: s.graph_captures() for k, s in sessions.items()}
    rows_done = {k: s.rows for k, s in sessions.items()}
    for s in sessions.values():
        s.close()
    ta, ta2, tb, tc = acc
    med = statistics.median
    r3 = lambda xs: [round(x, 3) for x in xs]                # noqa: E731
    steps = len(chunks2)
    doc = dict(
        tool="stream_guide_pass", device=torch.cuda.get_device_name(0), clips=B, code_rows=H, step_rows=HC, steps_per_region=steps,
        regions=a.regions, scale=a.scale,
        a_plain_2b_ms=r3(ta), a2_plain_2b_again_ms=r3(ta2), b_guided_ms=r3(tb), c_plain_b_ms=r3(tc),
        a_plain_2b_ms_median=round(med(ta), 3), a2_plain_2b_again_ms_median=round(med(ta2), 3), b_guided_ms_median=round(med(tb), 3),
        c_plain_b_ms_median=round(med(tc), 3),
        spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
        b_minus_a_per_step_us=round(1000 * (med(tb) - med(ta)) / steps, 3), b_minus_c_ms=round(med(tb) - med(tc), 3),
        b_over_a=round(med(tb) / med(ta), 4), b_over_c=round(med(tb) / med(tc), 4),
        positions_moved_by_guidance_first_region=round(moved, 4), shadows_rows_equal_primaries=shadows_follow,
        graph_captures_before_timed_regions=cap0, graph_captures_in_timed_regions={k: int(cap1[k] - cap0[k]) for k in cap0},
        session_rows_at_close=rows_done)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
