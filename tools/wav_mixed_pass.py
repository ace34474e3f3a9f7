"""From recordings to 265-d rows: today's route against `parallel.whole_body_clips`, same process, interleaved.

Four rows, full-size networks, 16 kHz recordings held as host arrays (what a serving host has):
  recordings   12 = the three demo recordings' sample counts (160 000 / 204 800 / 153 600) x 4 ids, 3 lengths
  lengths8     64 recordings, 8 lengths (the three above + a seeded 2 .. 10 s spread)
  lengths64    64 recordings, every one its own length
  lengths16    256 recordings, 16 lengths
(A) the route of the entries that existed before the mixed front-end: one front-end call per recording (`frontend._mfcc_on_device`: a
synchronisation and a device -> host copy each), the MFCC rows padded on the host inside `generate_clips` (mixed body pass),
`FaceGenerator.run_clips` (mixed face pass), `assemble_full` clip by clip.  (B) ONE `whole_body_clips`.  Timed regions alternate A B A B
after a warm-up of both; events on the stream; the figure is the median of the regions.  One JSON line per row; `--out FILE` writes them
(with the commit id) as one JSON document.

    python tools/wav_mixed_pass.py --regions 5 --out profiles/wav_mixed_pass.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REC_NS = [160000, 204800, 153600]


def rows(seed):
    rng = np.random.default_rng(seed)
    pool8 = REC_NS + sorted(int(n) for n in rng.integers(2 * 16000, 10 * 16000 + 1, 5))
    pool16 = pool8 + sorted(int(n) for n in rng.integers(2 * 16000, 10 * 16000 + 1, 8))
    return {"recordings": [n for _ in range(4) for n in REC_NS],
            "lengths8": [pool8[i] for i in rng.integers(0, 8, 64)],
            "lengths64": [int(n) for n in rng.choice(np.arange(2 * 16000, 10 * 16000 + 1), 64, replace=False)],
            "lengths16": [pool16[i] for i in rng.integers(0, 16, 256)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", default="recordings,lengths8,lengths64,lengths16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit id to record (default: git rev-parse HEAD of this tree)")
    a = ap.parse_args()
    import bench
    import nets
    from talkshow_amd import _lib, frontend, parallel, synth
    from talkshow_amd.config import Object
    from talkshow_amd.pose_index import assemble_full
    body = bench.build_models(0, seed=7)[0]
    face = nets.s2g_face(argparse.Namespace(gpu=0, infer=True), Object(json.load(open(os.path.join(REPO, "config", "face.json")))))
    face.load_state_dict({"generator": synth.to_torch(synth.face_state_dict(seed=7))})
    results = []
    for name, ns in rows(a.seed).items():
        if name not in a.rows.split(","):
            continue
        B = len(ns)
        wavs = [synth.wav16(50 + b, 1, int(n))[0] for b, n in enumerate(ns)]
        ids = (np.arange(B) % 4).astype(np.int64)
        fids = np.eye(4, dtype=np.float32)[np.arange(B) % 4]

        def per_recording():
            mf = [frontend._mfcc_on_device(w, 16000, 22000, 30) for w in wavs]
            poses = [p for _, p in body.generate_clips(mf, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=1)]
            fc = face.generator.run_clips(wavs, fids)
            return [assemble_full(p[None], f[None])[0] for p, f in zip(poses, fc)]

        def one_pass():
            return parallel.whole_body_clips(body, face, wavs, 16000, ids, fids, seed=1)

        for _ in range(a.warmup):
            ra, rb = per_recording(), one_pass()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(ra, rb))
        ta, tb = [], []
        for _ in range(a.regions):
            for fn, acc in ((per_recording, ta), (one_pass, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        frames = frontend.mixed_tables(ns, 16000)["face_frames"]
        rec = dict(row=name, recordings=B, distinct_lengths=len(set(ns)), seconds_min_max=[round(min(ns) / 16000, 2), round(max(ns) / 16000, 2)],
                   per_recording_ms=[round(x, 3) for x in ta], one_pass_ms=[round(x, 3) for x in tb],
                   per_recording_ms_median=round(statistics.median(ta), 3), one_pass_ms_median=round(statistics.median(tb), 3),
                   a_over_b=round(statistics.median(ta) / statistics.median(tb), 3), frames_total=int(frames.sum()), rows_bit_equal=bool(same))
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        commit = a.commit
        if commit is None:
            try:
                commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
            except OSError:
                commit = None
        with open(a.out, "w") as f:
            json.dump(dict(tool="wav_mixed_pass", commit=commit, seed=a.seed, regions=a.regions, device=torch.cuda.get_device_name(0),
                           rows=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
