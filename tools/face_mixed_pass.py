"""Mixed face pass against one face pass per distinct length, same process, interleaved.

Four rows, full-size network (12 layers), inputs staged on the device before anything is timed:
  recordings   12 clips = the three demo recordings' sample counts (160 000 / 204 800 / 153 600) x 4 ids, 3 lengths
  lengths8     64 clips, 8 lengths (the three above + a seeded 3 .. 20 s spread)
  lengths64    64 clips, every clip its own length
  equal64      64 equal clips of 10 s (the bench's face shape): the cost of the contract — the mixed entry gives up the stream-K band and
               adds masked epilogues, against the uniform entry in the default process (band on)
(A) `FaceGenerator.run` once per distinct length, (B) ONE `ts_face_generate_mixed` over all clips.  Timed regions alternate A B A B after
a warm-up of both; events on the stream; the figure is the median of the regions.  Padding waste of B = sum(T_max - frames[b]) / (B T_max).
`--layout` names B's row layout: `default` = the public entry (padded unless TS_FACE_PACK=1), `padded` / `packed` = that plan through
`ts_debug_face_generate_mixed`, `both` = padded AND packed in the same loop (A B0 B1 A B0 B1): the two plans in one process, one session.
One JSON line per row; `--out FILE` writes them (with the commit id) as one JSON document.

    python tools/face_mixed_pass.py --regions 5 --layout both --out profiles/face_packed_pass.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
I32P = C.POINTER(C.c_int32)
REC_NS = [160000, 204800, 153600]


def rows(seed):
    rng = np.random.default_rng(seed)
    spread = sorted(int(n) for n in rng.integers(3 * 16000, 20 * 16000 + 1, 5))
    pool8 = REC_NS + spread
    return {"recordings": [n for _ in range(4) for n in REC_NS],
            "lengths8": [pool8[i] for i in rng.integers(0, 8, 64)],
            "lengths64": sorted(int(n) for n in rng.choice(np.arange(3 * 16000, 20 * 16000 + 1), 64, replace=False)),
            "equal64": [160000] * 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", default="recordings,lengths8,lengths64,equal64")
    ap.add_argument("--layout", default="default", choices=["default", "padded", "packed", "both"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit id to record (default: git rev-parse HEAD of this tree)")
    a = ap.parse_args()
    from talkshow_amd import _lib, synth
    from talkshow_amd.modules import FaceGenerator
    m = FaceGenerator().cuda()
    m.load_state_dict(synth.to_torch(synth.face_state_dict(seed=7)))
    lib = _lib.load()
    results = []
    for name, ns in rows(a.seed).items():
        if name not in a.rows.split(","):
            continue
        B = len(ns)
        ns = np.asarray(ns, np.int32)
        fr = (ns.astype(np.int64) * 30 // 16000).astype(np.int32)
        N_max, T_max = int(ns.max()), int(fr.max())
        ids = np.eye(4, dtype=np.float32)[np.arange(B) % 4]
        wav = np.zeros((B, N_max), np.float32)
        for b, n in enumerate(ns):
            wav[b, :n] = synth.wav16(50 + b, 1, int(n))[0]
        wav_d, ids_d = torch.from_numpy(wav).cuda(), torch.from_numpy(ids).cuda()
        ns_d, fr_d = torch.from_numpy(ns).cuda(), torch.from_numpy(fr).cuda()
        out = torch.empty((B, T_max, 103), dtype=torch.float32, device="cuda")
        groups = {}
        for b, n in enumerate(ns.tolist()):
            groups.setdefault(n, []).append(b)
        staged = [(wav_d[bs, :n].contiguous(), ids_d[bs].contiguous(), n * 30 // 16000) for n, bs in groups.items()]

        def per_length():
            return [m.run(w, i, f) for w, i, f in staged]

        def mixed(layout):
            args = [m.handle(), _lib.dptr(wav_d), ns.ctypes.data_as(I32P), _lib.dptr(ns_d), fr.ctypes.data_as(I32P), _lib.dptr(fr_d), B, N_max,
                    T_max, _lib.dptr(ids_d), _lib.dptr(out), None, _lib.stream_ptr()]
            if layout == "default":
                _lib.check(lib.ts_face_generate_mixed(*args))
            else:
                _lib.check(lib.ts_debug_face_generate_mixed(*args, 1 if layout == "packed" else 0))

        layouts = ["padded", "packed"] if a.layout == "both" else [a.layout]
        fns = [("per_length", per_length)] + [(lay, lambda lay=lay: mixed(lay)) for lay in layouts]
        for _ in range(a.warmup):
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k, _ in fns}
        for _ in range(a.regions):
            for k, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1))
        ta, tb = t["per_length"], t[layouts[-1]]                           # mixed_ms: the named layout (both: packed)
        rows4 = (C.c_int64 * 4)()
        _lib.check(lib.ts_face_mixed_rows(ns.ctypes.data_as(I32P), fr.ctypes.data_as(I32P), B, N_max, T_max, rows4))
        rec = dict(row=name, clips=B, distinct_lengths=len(groups), frames_min_max=[int(fr.min()), int(fr.max())], layout=a.layout,
                   per_length_ms=[round(x, 3) for x in ta], mixed_ms=[round(x, 3) for x in tb],
                   per_length_ms_median=round(statistics.median(ta), 3), mixed_ms_median=round(statistics.median(tb), 3),
                   a_over_b=round(statistics.median(ta) / statistics.median(tb), 3),
                   padding_waste=round(float((T_max - fr).sum()) / (B * T_max), 4), frames_total=int(fr.sum()),
                   rows=dict(zip(("feature_padded", "feature_packed", "frames_padded", "frames_packed"), (int(v) for v in rows4))))
        if a.layout == "both":
            tp = t["padded"]
            rec.update(padded_ms=[round(x, 3) for x in tp], padded_ms_median=round(statistics.median(tp), 3),
                       padded_ms_spread=round(max(tp) - min(tp), 3), packed_ms_spread=round(max(tb) - min(tb), 3),
                       a_over_padded=round(statistics.median(ta) / statistics.median(tp), 3),
                       padded_over_packed=round(statistics.median(tp) / statistics.median(tb), 3))
        print(json.dumps(rec))
        results.append(rec)
    if a.out:
        commit = a.commit
        if commit is None:
            try:
                commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
            except OSError:
                commit = None
        with open(a.out, "w") as f:
            json.dump(dict(tool="face_mixed_pass", commit=commit, seed=a.seed, regions=a.regions, device=torch.cuda.get_device_name(0),
                           rows=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
