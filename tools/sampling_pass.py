"""What the sampling controls cost: a Philox decode without controls against the same decode with (T 0.9, k 64, p 0.95) on every clip,
same process, interleaved.

Full-size code predictor (2 048 classes, dim 256, 15 layers), `GatedPixelCNN.run` on audio-encoder rows, so that both sides replay a
whole-call graph of the same chain and differ in the 2 sampler launches per code row only:
  (A) `run(..., mode=PHILOX)`                     sample_kernel
  (B) `run(..., mode=PHILOX, sampling=record)`    sample_ctl_kernel
at B x 75 code rows for every B of --clips.  Timed regions alternate A B A B ... after a warm-up of both (graphs captured); HIP events on
the stream; the figure is the median region.  The samplers' OWN per-launch times come from instrumented (eager) runs through
`ts_prof_read_n`: family 2 holds the 2 sampler launches per code row plus glue launches whose number does not depend on the row count, so
(family time at `--rows` rows - family time at `--rows` / 3 rows) / (the difference in sampler launches) is the time of one sampler
launch with the glue cancelled — computed for sample_kernel and for sample_ctl_kernel, each the smaller of two runs.  One JSON line per
shape; `--out FILE` also appends them there.

    python tools/sampling_pass.py --clips 32 256 --regions 5
"""
import argparse
import ctypes as C
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
    ap.add_argument("--clips", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--rows", type=int, default=75)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--record", type=float, nargs=3, default=[0.9, 0.95, 64], metavar=("T", "P", "K"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib
    w, _ = bench.build_models(0)
    pix = w.generator
    lib, ctx = _lib.load(), _lib.context(0)
    rec = (a.record[0], a.record[1], int(a.record[2]))
    mode = _lib.TS_SAMPLE_PHILOX
    for B in a.clips:
        H = a.rows
        rng = np.random.default_rng(B)
        aud = torch.from_numpy(rng.standard_normal((B, H, 256)).astype(np.float32)).cuda()
        label = torch.from_numpy((np.arange(B) % 4).astype(np.int64)).cuda()

        def plain():
            return pix.run(label, aud, mode=mode, seed=1)

        def ctl():
            return pix.run(label, aud, mode=mode, seed=1, sampling=rec)

        def family2(fn):
            ms, n, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
            _lib.check(lib.ts_prof_enable(ctx, 1))
            _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
            fn()
            torch.cuda.synchronize()
            _lib.check(lib.ts_prof_read_n(ctx, 4, ms, n, fl, 1))
            _lib.check(lib.ts_prof_enable(ctx, 0))
            return float(ms[2]), int(n[2])

        for _ in range(4):                                   # warm-up: the third sighting captures each side's whole-call graph
            plain(), ctl()
        torch.cuda.synchronize()
        Hs = max(1, H // 3)                                  # the same decode over fewer rows: the glue launches stay, the sampler launches go
        aud_s = aud[:, :Hs].contiguous()

        def per_launch(sampling):
            long_ = min(family2(lambda: pix.run(label, aud, mode=mode, seed=1, sampling=sampling))[0] for _ in range(2))
            short = min(family2(lambda: pix.run(label, aud_s, mode=mode, seed=1, sampling=sampling))[0] for _ in range(2))
            return 1e3 * (long_ - short) / (2 * (H - Hs))
        us_plain, us_ctl = per_launch(None), per_launch(rec)
        plain(), ctl()
        torch.cuda.synchronize()
        cap0 = pix.graph_captures()
        ta, tb = [], []
        for _ in range(a.regions):
            for fn, acc in ((plain, ta), (ctl, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        cap1 = pix.graph_captures()
        same = bool(np.array_equal(plain()[0].cpu().numpy(), pix.run(label, aud, mode=mode, seed=1, sampling=(1.0, 1.0, 0))[0].cpu().numpy()))
        ma, mb = statistics.median(ta), statistics.median(tb)
        out = dict(tool="sampling_pass", clips=B, code_rows=H, record=list(rec), regions=a.regions, plain_ms=[round(x, 3) for x in ta],
                   ctl_ms=[round(x, 3) for x in tb], plain_ms_median=round(ma, 3), ctl_ms_median=round(mb, 3), ratio=round(mb / ma, 4),
                   controls_cost_per_pass_ms=round(mb - ma, 3), sampler_launches_per_pass=2 * H,
                   sample_kernel_us_per_launch=round(us_plain, 3), sample_ctl_kernel_us_per_launch=round(us_ctl, 3),
                   graph_captures_in_timed_regions=int(cap1 - cap0), neutral_record_equals_plain=same, device=torch.cuda.get_device_name(0))
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
