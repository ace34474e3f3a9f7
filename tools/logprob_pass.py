"""What the log-probability output costs, and what scoring through it saves: same process, interleaved.

Full-size code predictor (2 048 classes, dim 256, 15 layers) inside the shipped wrapper, B x 75 code rows for every B of --clips:
  decode   (A) `GatedPixelCNN.run(..., mode=PHILOX)`                    sample_kernel, whole-call graph
           (B) `GatedPixelCNN.run(..., mode=PHILOX, logprobs=True)`     sample_lp_kernel, its own whole-call graph
  scoring  (A) `TrainWrapper.score_batch(mfcc, ids, codes)`             teacher forced, log-probabilities and sums from the sampler launch
           (B) the route it replaces: the audio encoder, `run(..., TEACHER_FORCED, want_logits=True)` — (B,75,2,2048) fp32 — and torch
               `log_softmax` + `gather` + per-clip sums
Timed regions alternate A B A B ... after a warm-up of both (graphs captured); HIP events on the stream; the figure is the median region.
One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/logprob_pass.py --clips 32 256 --regions 5 --out profiles/logprob_pass.json
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


def timed(pairs, regions):
    """pairs = ((fn_a, fn_b)); -> ([ms of a], [ms of b]) over `regions` alternating regions."""
    ta, tb = [], []
    for _ in range(regions):
        for fn, acc in zip(pairs, (ta, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return ta, tb


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
    mode = _lib.TS_SAMPLE_PHILOX
    shapes = []
    for B in a.clips:
        H = a.rows
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids = torch.from_numpy((np.arange(B) % 4).astype(np.int64)).cuda()
        aud = w.audioencoder.forward_nlc(mfcc)

        def plain():
            return pix.run(ids, aud, mode=mode, seed=1)

        def with_lp():
            return pix.run(ids, aud, mode=mode, seed=1, logprobs=True)

        for _ in range(4):                                   # warm-up: the third sighting captures each side's whole-call graph
            plain(), with_lp()
        torch.cuda.synchronize()
        codes = plain()[0]

        def score():
            return w.score_batch(mfcc, ids, codes)

        def score_logits():
            rows = w.audioencoder.forward_nlc(mfcc)
            _, lg = pix.run(ids, rows, mode=_lib.TS_TEACHER_FORCED, codes=codes, want_logits=True)
            lp = torch.log_softmax(lg, -1).gather(-1, codes.unsqueeze(-1)).squeeze(-1)
            s = lp.double().sum(1)
            return lp, torch.cat([s, s.sum(1, keepdim=True)], 1)

        for _ in range(2):
            score(), score_logits()
        torch.cuda.synchronize()
        cap0 = pix.graph_captures()
        da, db = timed((plain, with_lp), a.regions)
        cap1 = pix.graph_captures()
        sa, sb = timed((score, score_logits), a.regions)
        same_codes = bool(np.array_equal(plain()[0].cpu().numpy(), with_lp()[0].cpu().numpy()))
        lp_dec = with_lp()[2].cpu().numpy()
        lp_sc, sums = score()
        lp_ref, sums_ref = score_logits()
        med = statistics.median
        shapes.append(dict(
            clips=B, code_rows=H, regions=a.regions,
            decode_ms=[round(x, 3) for x in da], decode_logprobs_ms=[round(x, 3) for x in db],
            decode_ms_median=round(med(da), 3), decode_logprobs_ms_median=round(med(db), 3), decode_ratio=round(med(db) / med(da), 4),
            logprobs_cost_per_pass_ms=round(med(db) - med(da), 3), sampler_launches_per_pass=2 * H,
            graph_captures_in_timed_decode_regions=int(cap1 - cap0), codes_equal=same_codes,
            score_ms=[round(x, 3) for x in sa], score_via_logits_ms=[round(x, 3) for x in sb],
            score_ms_median=round(med(sa), 3), score_via_logits_ms_median=round(med(sb), 3), score_ratio=round(med(sa) / med(sb), 4),
            logits_bytes_not_written=int(B) * H * 2 * pix.input_dim * 4,
            score_equals_decode_logprobs=bool(np.array_equal(lp_sc.cpu().numpy(), lp_dec)),
            score_max_abs_diff_to_torch_log_softmax=float((lp_sc - lp_ref).abs().max()),
            sums_max_abs_diff_to_torch=float((sums - sums_ref).abs().max())))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="logprob_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
