"""What a code bias costs in the body decode: same process, interleaved, against the mixed pass with a neutral sampling table.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips (the shape of tools/style_pass.py),
Philox, no log-probabilities, nothing given, integer ids:
  (A)  a neutral sampling table, no bias        `ts_pixelcnn_generate_mixed_bias` with bias_dev == NULL: sample_ctl_kernel — the yardstick,
                                                because the same sampler family runs
  (A') the same call again                      the run-to-run spread of (A) inside this process
  (B)  one table shared by all clips            NB = 1: sample_ctl_bias_kernel, every workgroup reads the same 8 KB row
  (C)  one distinct table per clip              NB = B: 8 KB of table per clip and launch, 16 B KB staged per pass
The tables are finite random biases with a quarter of the codes banned.  A zero table in (B) and (C) must return (A)'s codes.  Timed
regions alternate A A' B C A A' B C ... after a warm-up of all (graphs captured); HIP events on the stream; the figure is the median
region.  Nothing is asserted about the ratios.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/bias_pass.py --clips 32 256 --regions 5 --out profiles/bias_pass.json
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

        def run(tables, index):
            _lib.check(lib.ts_pixelcnn_generate_mixed_bias(
                pix.handle(), _lib.dptr(ids), _lib.dptr(aud), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode, None, 1,
                _lib.dptr(clip_index), _lib.dptr(codes), neutral, 1, None, None, None, None, None, None, 0, _lib.dptr(tables),
                0 if tables is None else int(tables.shape[0]), None if index is None else index.ctypes.data_as(i32p), _lib.stream_ptr()))
            return codes

        rng = np.random.default_rng(B)

        def make(n):
            t = rng.standard_normal((n, 2, V)).astype(np.float32)
            t[rng.random((n, 2, V)) < 0.25] = -np.inf
            t[:, :, 0] = 0.0
            return torch.from_numpy(t).cuda()
        shared, own = make(1), make(B)
        idx_shared, idx_own = np.zeros(B, np.int32), np.arange(B, dtype=np.int32)
        zero1, zeroB = torch.zeros((1, 2, V), device="cuda"), torch.zeros((B, 2, V), device="cuda")

        def leg_a():
            return run(None, None)

        def leg_b():
            return run(shared, idx_shared)

        def leg_c():
            return run(own, idx_own)

        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        want = leg_a().cpu().numpy()
        eq_b = bool(np.array_equal(run(zero1, idx_shared).cpu().numpy(), want))
        eq_c = bool(np.array_equal(run(zeroB, idx_own).cpu().numpy(), want))
        cb, cc = leg_b().cpu().numpy().copy(), leg_c().cpu().numpy().copy()
        sh, ow = shared.cpu().numpy(), own.cpu().numpy()
        banned_b = int(sum((sh[0, j][cb[:, :, j]] == -np.inf).sum() for j in range(2)))
        banned_c = int(sum((ow[b, j][cc[b, :, j]] == -np.inf).sum() for b in range(B) for j in range(2)))
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc = timed((leg_a, leg_a, leg_b, leg_c), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows=H, sampler_launches=2 * H, regions=a.regions,
            a_neutral_table_ms=r3(ta), a2_neutral_table_again_ms=r3(ta2), b_shared_table_ms=r3(tb), c_table_per_clip_ms=r3(tc),
            a_neutral_table_ms_median=round(med(ta), 3), a2_neutral_table_again_ms_median=round(med(ta2), 3),
            b_shared_table_ms_median=round(med(tb), 3), c_table_per_clip_ms_median=round(med(tc), 3),
            a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
            spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3), c_minus_a_ms=round(med(tc) - med(ta), 3),
            c_minus_a_per_sampler_launch_us=round(1000 * (med(tc) - med(ta)) / (2 * H), 3),
            table_bytes_per_clip=int(8 * V), staged_bytes_c=int(8 * V * B), graph_captures_in_timed_regions=int(cap1 - cap0),
            b_zero_table_codes_equal_a=eq_b, c_zero_table_codes_equal_a=eq_c, b_banned_codes_drawn=banned_b, c_banned_codes_drawn=banned_c))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="bias_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
