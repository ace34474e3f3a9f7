"""Mixed pass against one pass per length, same process, interleaved.

N clips whose lengths come from a fixed, seeded list — the three demo recordings' lengths (300 / 384 / 288 MFCC rows) plus a spread of
3 .. 20 s (90 .. 600 rows at 30 fps) — are generated
  (A) as the library offered before mixed passes: clips grouped by length, one `generate_batch` per length;
  (B) as ONE mixed pass (`generate_clips`).
Timed regions alternate A B A B ... after a warm-up of both (graphs captured, clocks up); the figure is the median region.  Chain
launch counts come from `ts_prof_read` on one instrumented run of each.  One JSON line; `--out FILE` also writes it there.

    python tools/mixed_pass.py --clips 64 --regions 5
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def lengths(n, seed, distinct):
    rng = np.random.default_rng(seed)
    pool = [300, 384, 288] + sorted(int(t) for t in rng.integers(90, 601, max(0, distinct - 3)))
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8, help="distinct lengths in the pool (the recordings' three + a 3..20 s spread)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    lib, ctx = _lib.load(), _lib.context(0)
    lens = lengths(a.clips, a.seed, a.distinct)
    clips = [torch.from_numpy(synth.mfcc_features(100 + k, 1, t)[0]).cuda() for k, t in enumerate(lens)]
    ids = torch.from_numpy((np.arange(a.clips) % 4).astype(np.int64)).cuda()
    groups = {}
    for b, t in enumerate(lens):
        groups.setdefault(t, []).append(b)
    stacked = {t: (torch.stack([clips[b] for b in bs]), ids[bs]) for t, bs in groups.items()}
    mode = _lib.TS_SAMPLE_PHILOX

    def per_length():
        return [w.generate_batch(m, i, mode=mode, seed=1, clip_index0=0) for m, i in stacked.values()]

    def mixed():
        return w.generate_clips(clips, ids, mode=mode, seed=1)

    def launches(fn):
        ms, n, fl = (C.c_double * 3)(), (C.c_int64 * 3)(), (C.c_double * 3)()
        _lib.check(lib.ts_prof_enable(ctx, 1))
        _lib.check(lib.ts_prof_read(ctx, ms, n, fl, 1))
        fn()
        torch.cuda.synchronize()
        _lib.check(lib.ts_prof_read(ctx, ms, n, fl, 1))
        _lib.check(lib.ts_prof_enable(ctx, 0))
        return int(n[1])

    la, lb = launches(per_length), launches(mixed)
    for _ in range(3):                                   # warm-up: every graph either path needs is captured here
        per_length(), mixed()
    torch.cuda.synchronize()
    cap0 = lib.ts_pixelcnn_graph_captures(w.generator.handle(), _lib.stream_ptr())
    ta, tb = [], []
    for _ in range(a.regions):
        for fn, acc in ((per_length, ta), (mixed, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    cap1 = lib.ts_pixelcnn_graph_captures(w.generator.handle(), _lib.stream_ptr())
    frames = sum(4 * (t // 4) for t in lens)
    rec = dict(tool="mixed_pass", clips=a.clips, distinct_lengths=len(groups), lengths_min_max=[min(lens), max(lens)], seed=a.seed,
               regions=a.regions, per_length_ms=[round(x, 3) for x in ta], mixed_ms=[round(x, 3) for x in tb],
               per_length_ms_median=round(statistics.median(ta), 3), mixed_ms_median=round(statistics.median(tb), 3),
               speedup=round(statistics.median(ta) / statistics.median(tb), 3), chain_launches_per_length=la, chain_launches_mixed=lb,
               graph_captures_in_timed_regions=int(cap1 - cap0), pose_frames=frames, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
