"""What seamless streaming costs: same process, interleaved, against the plain body session.

Full-size networks (code predictor 2 048 / 256 / 15, VQ nets of 1 024 hidden channels); --clips clips; one region = --rows code rows of
audio (4 frames each) pushed --step code rows at a time (32 clips, 300 rows, 15-row pushes: twenty 2 s chunks of 60 MFCC frames), Philox:
  (A)  the plain session        `open_stream(...)`: every chunk alone through the audio encoder, the chain step and both VQ decoders
  (A') the same on a session of its own: the run-to-run spread of (A) inside this process
  (B)  the seamless session     `open_stream(..., seamless=True)` and its `flush()`: the same chain steps, the conv nets on windows —
                                the encoder on (n + 14 .. 17) / n times the rows of a push of n code rows, the decoders on (n + 26 .. 29) / n
A plain session goes on from region to region; a seamless one ends with its flush, so every region of (B) has a session of its own, opened
ahead of the timed regions.  Timed regions alternate A A' B A A' B ... after a warm-up of two regions per leg; HIP events on the stream;
the figure is the median region.  Nothing is asserted.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/seamless_pass.py --regions 5 --out profiles/seamless_pass.json
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
WARMUP = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--step", type=int, default=15)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    B, H, HC = a.clips, a.rows, a.step
    mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
    chunks = [mfcc[:, 4 * r:4 * (r + HC)].contiguous() for r in range(0, H, HC)]
    ids = (np.arange(B) % w.num_classes).astype(np.int64)
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1)
    plain = {k: w.open_stream(ids, B, 4 * HC) for k in ("a", "a2")}
    seamless = [w.open_stream(ids, B, 4 * HC, seamless=True) for _ in range(WARMUP + a.regions)]
    state_bytes = seamless[0].state_bytes
    frames = {"a": 0, "a2": 0, "b": 0}

    def plain_leg(name):
        def run():
            for ch in chunks:
                frames[name] += int(plain[name].push(ch, **draw).shape[1])
        return run

    def seamless_leg():
        st = seamless.pop()
        for ch in chunks:
            frames["b"] += int(st.push(ch, **draw).shape[1])
        frames["b"] += int(st.flush(**draw).shape[1])
        return st
    legs = (plain_leg("a"), plain_leg("a2"), seamless_leg)
    done = []
    for _ in range(WARMUP):
        for fn in legs:
            done.append(fn())
    torch.cuda.synchronize()
    acc = [[] for _ in legs]
    for _ in range(a.regions):
        for fn, t in zip(legs, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            done.append(fn())
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    captures = [s.graph_captures() for s in done if s is not None]
    for s in list(plain.values()) + [s for s in done if s is not None]:
        s.close()
    ta, ta2, tb = acc
    med = statistics.median
    r3 = lambda xs: [round(x, 3) for x in xs]                # noqa: E731
    n_regions = WARMUP + a.regions
    doc = dict(
        tool="seamless_pass", device=torch.cuda.get_device_name(0), clips=B, code_rows=H, step_rows=HC, pushes_per_region=len(chunks),
        regions=a.regions,
        a_plain_ms=r3(ta), a2_plain_again_ms=r3(ta2), b_seamless_ms=r3(tb),
        a_plain_ms_median=round(med(ta), 3), a2_plain_again_ms_median=round(med(ta2), 3), b_seamless_ms_median=round(med(tb), 3),
        a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4),
        spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
        b_minus_a_per_push_us=round(1000 * (med(tb) - med(ta)) / len(chunks), 3),
        conv_rows_factor_encoder_at_most=round((HC + 17) / HC, 3), conv_rows_factor_decoder_at_most=round((HC + 29) / HC, 3),
        pose_frames_per_region={k: v // n_regions for k, v in frames.items()}, seamless_state_bytes=state_bytes,
        seamless_graph_captures_per_session=captures)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
