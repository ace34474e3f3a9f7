#!/usr/bin/env python
"""Chain alone, one process per figure: `chain_ms_per_pass` of a greedy decode of --clips clips x 75 code rows, timed as bench.py's
chain_roofline times it (HIP events around one replay of the pass's whole-call graph; five replays, the median).  Used for the A/B of the
code tables (profiles/code_tables.json): the library comes from TS_LIB_PATH (unset: this tree's build), TS_PIX_TABLES from the environment.

    python tools/chain_tables_ab.py --clips 256 --tag new
    TS_LIB_PATH=tools/lib_parent.so python tools/chain_tables_ab.py --clips 256 --tag parent

Prints one JSON line: {"tag", "clips", "chain_ms_per_pass", "launches_per_pass", "lib", "TS_PIX_TABLES"}.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from talkshow_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    lib = _lib.load()
    w, _ = bench.build_models(0)
    T = bench.FRAMES_PER_CLIP
    mfcc = torch.from_numpy(synth.mfcc_features(4000, a.clips, T)).cuda()
    ids = torch.from_numpy(synth.speaker_ids(a.clips)).cuda()
    stream = torch.cuda.Stream()
    r = bench.chain_roofline(w, lib, _lib, stream, mfcc, ids, T // 4, f"skinny_gemm_f32_M{a.clips}")
    torch.cuda.synchronize()
    print(json.dumps({"tag": a.tag, "clips": a.clips, "chain_ms_per_pass": r["chain_ms_per_pass"], "launches_per_pass": r["launches_per_pass"],
                      "lib": os.environ.get("TS_LIB_PATH", "tree"), "TS_PIX_TABLES": os.environ.get("TS_PIX_TABLES", "")}))


if __name__ == "__main__":
    main()
