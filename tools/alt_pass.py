"""What alternatives cost in the body decode: same process, interleaved, against the mixed pass of the same sampler family.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips, Philox, integer ids:
  (A)  `run(logprobs=True)` under a neutral sampling table, one all-zero bias table and repeat = (16, 0, 0): the sample_ctl_rep kernels with
       log-probabilities — the family the alternatives kernels are made of, so the difference is the keyword's own reductions
  (A') the same call again                           the run-to-run spread of (A) inside this process
  (B)  (A) with alternatives=0                       S_all, E, the entropy and the rank: two more chunk sums, one count, two fp64 logs
  (C1) (A) with alternatives=1                       one selection round on top of (B)
  (C)  (A) with alternatives=8                       eight selection rounds
  (D)  what a host does without the keyword, on the same uniform batch: `run(want_logits=True)` (the decode off its graphs, B x H x 2 x V
       floats written) plus torch log_softmax / topk(8) / entropy / rank over them
(B), (C1) and (C) must return (A)'s codes and log-probabilities.  Timed regions alternate A A' B C1 C D A A' ... after a warm-up of all
(graphs captured); HIP events on the stream; the figure is the median region.  Nothing is asserted about the ratios.  One JSON document:
`--out FILE` writes it there (default: stdout only).

    python tools/alt_pass.py --clips 32 256 --regions 5 --out profiles/alt_pass.json
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


def timed(fns, regions):
    """fns = (fn_a, fn_b, ...) -> [[ms of a], [ms of b], ...] over `regions` alternating regions."""
    acc = [[] for _ in fns]
    for _ in range(regions):
        for fn, t in zip(fns, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--rows", type=int, default=75)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    pix = w.generator
    NC, V = pix.n_classes, pix.input_dim
    shapes = []
    for B in a.clips:
        H = a.rows
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids = (np.arange(B) % NC).astype(np.int64)
        aud = w.audioencoder.forward_nlc(mfcc)
        kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1, sampling=(1.0, 1.0, 0), code_bias=np.zeros((2, V), np.float32), repeat=(16, 0.0, 0.0),
                  logprobs=True)

        def leg(n):
            return lambda: pix.run(ids, aud, alternatives=n, **kw)

        def leg_d():
            codes, logits = pix.run(ids, aud, mode=_lib.TS_SAMPLE_PHILOX, seed=1, want_logits=True)
            lsm = torch.log_softmax(logits, -1)
            top = lsm.topk(8, -1)
            ent = -(lsm.exp() * lsm).sum(-1)
            own = lsm.gather(-1, codes.unsqueeze(-1))
            rank = (lsm > own).sum(-1)
            return codes, top, ent, rank

        legs = (leg(None), leg(None), leg(0), leg(1), leg(8), leg_d)
        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            for f in legs:
                f()
        torch.cuda.synchronize()
        want = legs[0]()
        same = [bool(torch.equal(want[0], f()[0]) and torch.equal(want[2].view(torch.int32), f()[2].view(torch.int32))) for f in legs[2:5]]
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc1, tc, td = timed(legs, a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows=H, sampler_launches=2 * H, regions=a.regions,
            a_logprobs_ms=r3(ta), a2_logprobs_again_ms=r3(ta2), b_alternatives_0_ms=r3(tb), c1_alternatives_1_ms=r3(tc1), c_alternatives_8_ms=r3(tc),
            d_logits_and_torch_ms=r3(td),
            a_ms_median=round(med(ta), 3), a2_ms_median=round(med(ta2), 3), b_ms_median=round(med(tb), 3), c1_ms_median=round(med(tc1), 3),
            c_ms_median=round(med(tc), 3), d_ms_median=round(med(td), 3),
            spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3), c1_minus_a_ms=round(med(tc1) - med(ta), 3),
            c_minus_a_ms=round(med(tc) - med(ta), 3), d_minus_a_ms=round(med(td) - med(ta), 3),
            b_over_a=round(med(tb) / med(ta), 4), c1_over_a=round(med(tc1) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
            d_over_a=round(med(td) / med(ta), 4), c_minus_a_per_sampler_launch_us=round(1000 * (med(tc) - med(ta)) / (2 * H), 3),
            selection_share_of_c=round((med(tc) - med(tb)) / max(med(tc) - med(ta), 1e-9), 3),
            logits_bytes=B * H * 2 * V * 4, alternatives_8_bytes=B * H * 2 * (8 * 8 + 8), graph_captures_in_timed_regions=int(cap1 - cap0),
            codes_and_logprobs_equal_a=same))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="alt_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
