"""What a repetition penalty costs in the body decode: same process, interleaved, against the mixed pass of the bias family.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips (the shape of tools/bias_pass.py),
Philox, a neutral sampling table, no log-probabilities, nothing given, integer ids:
  (A)  one all-zero bias table shared by all clips   `ts_pixelcnn_generate_mixed_repeat` with rep_host == NULL: sample_ctl_bias_kernel —
                                                     the yardstick: the bias family is the nearest existing sampler
  (A') the same call again                           the run-to-run spread of (A) inside this process
  (B)  (A) with repeat = (16, 1.0, 0.0) for all      sample_ctl_rep_kernel: 16 ring entries read, counted and one written per launch
  (C)  (A) with (W_b, 0.5, 0.25), W_b = 64 - b % 33  a different window per clip, 32 to 64 entries
(64, 0, 0) in the place of (B) must return (A)'s codes.  Timed regions alternate A A' B C A A' B C ... after a warm-up of all (graphs
captured); HIP events on the stream; the figure is the median region.  Nothing is asserted about the ratios.  One JSON document:
`--out FILE` writes it there (default: stdout only).

    python tools/repeat_pass.py --clips 32 256 --regions 5 --out profiles/repeat_pass.json
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


def share_repeating_within_16(codes):
    """(B,H,2) codes -> the share of positions whose code occurred in the 16 rows before it in the same clip and column."""
    B, H, _ = codes.shape
    hit = 0
    for r in range(1, H):
        prev = codes[:, max(0, r - 16):r]
        hit += int((prev == codes[:, r:r + 1]).any(1).sum())
    return hit / float(B * (H - 1) * 2)


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
    lib = _lib.load()
    mode = _lib.TS_SAMPLE_PHILOX
    i32p = C.POINTER(C.c_int32)
    neutral = (_lib.TsSampling * 1)()
    neutral[0].temperature, neutral[0].top_p, neutral[0].top_k, neutral[0].reserved = 1.0, 1.0, 0, 0
    shapes = []
    for B in a.clips:
        H = a.rows
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids = torch.from_numpy((np.arange(B) % NC).astype(np.int64)).cuda()
        aud = w.audioencoder.forward_nlc(mfcc)
        lens = np.full(B, 4 * H, np.int32)
        lens_dev = torch.from_numpy(lens).cuda()
        clip_index = torch.arange(B, dtype=torch.int64, device="cuda")
        codes = torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")
        zero = torch.zeros((1, 2, V), device="cuda")
        index = np.zeros(B, np.int32)

        def records(fn):
            arr = (_lib.TsRepeat * B)()
            for b in range(B):
                arr[b].window, arr[b].presence, arr[b].frequency, arr[b].reserved = (*fn(b), 0)
            return arr
        rec_b = records(lambda b: (16, 1.0, 0.0))
        rec_c = records(lambda b: (64 - b % 33, 0.5, 0.25))
        rec_0 = records(lambda b: (64, 0.0, 0.0))

        def run(rep):
            _lib.check(lib.ts_pixelcnn_generate_mixed_repeat(
                pix.handle(), _lib.dptr(ids), _lib.dptr(aud), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode, None, 1,
                _lib.dptr(clip_index), _lib.dptr(codes), neutral, 1, None, None, None, None, None, None, 0, _lib.dptr(zero), 1,
                index.ctypes.data_as(i32p), rep, 0 if rep is None else B, _lib.stream_ptr()))
            return codes

        def leg_a():
            return run(None)

        def leg_b():
            return run(rec_b)

        def leg_c():
            return run(rec_c)

        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        want = leg_a().cpu().numpy().copy()
        eq_0 = bool(np.array_equal(run(rec_0).cpu().numpy(), want))
        cb, cc = leg_b().cpu().numpy().copy(), leg_c().cpu().numpy().copy()
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc = timed((leg_a, leg_a, leg_b, leg_c), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows=H, sampler_launches=2 * H, regions=a.regions,
            a_zero_bias_table_ms=r3(ta), a2_zero_bias_table_again_ms=r3(ta2), b_window_16_ms=r3(tb), c_window_per_clip_ms=r3(tc),
            a_zero_bias_table_ms_median=round(med(ta), 3), a2_zero_bias_table_again_ms_median=round(med(ta2), 3),
            b_window_16_ms_median=round(med(tb), 3), c_window_per_clip_ms_median=round(med(tc), 3),
            a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
            spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3), c_minus_a_ms=round(med(tc) - med(ta), 3),
            c_minus_a_per_sampler_launch_us=round(1000 * (med(tc) - med(ta)) / (2 * H), 3),
            ring_bytes_per_clip=2 * 64 * 4, record_bytes_per_clip=16, graph_captures_in_timed_regions=int(cap1 - cap0),
            zero_penalties_codes_equal_a=eq_0, a_share_repeating_within_16=round(share_repeating_within_16(want), 4),
            b_share_repeating_within_16=round(share_repeating_within_16(cb), 4), c_share_repeating_within_16=round(share_repeating_within_16(cc), 4)))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="repeat_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
