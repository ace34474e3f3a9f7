"""What a mask of kept positions costs in the body decode: same process, interleaved, against the given pass it extends.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips (the shape of tools/given_pass.py),
Philox, no table, no log-probabilities, every row given (G_b = H_b) from the pass's own plain decode:
  (A)  the given pass                           `ts_pixelcnn_generate_mixed_given`: the code path there was before the mask — the yardstick
  (A') the same call again                      the run-to-run spread of (A) inside this process
  (B)  the same pass with an all-ones mask      `ts_pixelcnn_generate_mixed_keep`: the mask staged per chunk, one more byte load per sampler
                                                workgroup, nothing drawn (the codes must equal (A)'s)
  (C)  the same pass with given_keep="body"     column 0 kept, every hand code drawn (the body column must equal (A)'s)
Timed regions alternate A A' B C A A' B C ... after a warm-up of all (graphs captured); HIP events on the stream; the figure is the median
region.  Nothing is asserted about the ratios.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/keep_pass.py --clips 32 256 --regions 5 --out profiles/keep_pass.json
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
    lib = _lib.load()
    mode = _lib.TS_SAMPLE_PHILOX
    i32p = C.POINTER(C.c_int32)
    shapes = []
    for B in a.clips:
        H = a.rows
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids = torch.from_numpy((np.arange(B) % 4).astype(np.int64)).cuda()
        aud = w.audioencoder.forward_nlc(mfcc)
        lens = np.full(B, 4 * H, np.int32)
        lens_dev = torch.from_numpy(lens).cuda()
        clip_index = torch.arange(B, dtype=torch.int64, device="cuda")
        codes = torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")
        full = np.full(B, H, np.int32)
        args = lambda block, table: (  # noqa: E731
            pix.handle(), _lib.dptr(ids), _lib.dptr(aud), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode, None, 1,
            _lib.dptr(clip_index), _lib.dptr(codes), None, 0, None, _lib.dptr(block), None if table is None else table.ctypes.data_as(i32p), None)

        def given_pass(block, table):
            _lib.check(lib.ts_pixelcnn_generate_mixed_given(*args(block, table), _lib.stream_ptr()))
            return codes

        def keep_pass(block, table, keep):
            _lib.check(lib.ts_pixelcnn_generate_mixed_keep(*args(block, table), _lib.dptr(keep), _lib.stream_ptr()))
            return codes

        head = given_pass(None, None).clone()                 # the plain decode: what every leg is given
        ones = torch.ones((B, H, 2), dtype=torch.uint8, device="cuda")
        body = ones.clone()
        body[:, :, 1] = 0

        def leg_a():
            return given_pass(head, full)

        def leg_b():
            return keep_pass(head, full, ones)

        def leg_c():
            return keep_pass(head, full, body)

        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        want = head.cpu().numpy()
        eq_a = bool(np.array_equal(leg_a().cpu().numpy(), want))
        eq_b = bool(np.array_equal(leg_b().cpu().numpy(), want))
        got_c = leg_c().cpu().numpy()
        eq_c_body, eq_c_all = bool(np.array_equal(got_c[:, :, 0], want[:, :, 0])), bool(np.array_equal(got_c, want))
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc = timed((leg_a, leg_a, leg_b, leg_c), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows=H, given_rows=H, regions=a.regions,
            a_given_ms=r3(ta), a2_given_again_ms=r3(ta2), b_all_ones_mask_ms=r3(tb), c_keep_body_ms=r3(tc),
            a_given_ms_median=round(med(ta), 3), a2_given_again_ms_median=round(med(ta2), 3), b_all_ones_mask_ms_median=round(med(tb), 3),
            c_keep_body_ms_median=round(med(tc), 3),
            a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
            spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3), c_minus_a_ms=round(med(tc) - med(ta), 3),
            sampler_launches_per_pass=2 * H, graph_captures_in_timed_regions=int(cap1 - cap0),
            a_codes_equal_given=eq_a, b_codes_equal_given=eq_b, c_body_column_equals_given=eq_c_body, c_codes_equal_given=eq_c_all))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="keep_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
