"""What a speaker style costs in the body decode: same process, interleaved, against the plain mixed pass.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips (the shape of tools/keep_pass.py),
Philox, no table, no log-probabilities, nothing given:
  (A)  the plain mixed pass                     `ts_pixelcnn_generate_mixed_style` with style_dev == NULL: integer ids, the gather — the yardstick
  (A') the same call again                      the run-to-run spread of (A) inside this process
  (B)  per-clip blends (style_rows = 1)         the conditioning rows filled by style_rows_kernel in place of the gather, once per pass;
                                                the plain pass's graphs
  (C)  per-row tracks (style_rows = H_max)      every chunk's conditioning rows staged by style_rows_kernel ahead of its replay; graph keys
                                                of its own (bit 4), the gate launches read the row's slab
A one-hot block in (B) and (C) must return (A)'s codes.  Timed regions alternate A A' B C A A' B C ... after a warm-up of all (graphs
captured); HIP events on the stream; the figure is the median region.  Nothing is asserted about the ratios.  One JSON document:
`--out FILE` writes it there (default: stdout only).

    python tools/style_pass.py --clips 32 256 --regions 5 --out profiles/style_pass.json
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
    NC = pix.n_classes
    lib = _lib.load()
    mode = _lib.TS_SAMPLE_PHILOX
    i32p = C.POINTER(C.c_int32)
    shapes = []
    for B in a.clips:
        H = a.rows
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids_host = (np.arange(B) % NC).astype(np.int64)
        ids = torch.from_numpy(ids_host).cuda()
        aud = w.audioencoder.forward_nlc(mfcc)
        lens = np.full(B, 4 * H, np.int32)
        lens_dev = torch.from_numpy(lens).cuda()
        clip_index = torch.arange(B, dtype=torch.int64, device="cuda")
        codes = torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")

        def run(style, S):
            _lib.check(lib.ts_pixelcnn_generate_mixed_style(
                pix.handle(), _lib.dptr(ids), _lib.dptr(aud), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode, None, 1,
                _lib.dptr(clip_index), _lib.dptr(codes), None, 0, None, None, None, None, None, _lib.dptr(style), S, _lib.stream_ptr()))
            return codes

        rng = np.random.default_rng(B)
        eye = np.eye(NC, dtype=np.float32)[ids_host]
        hot1 = torch.from_numpy(eye[:, None].copy()).cuda()                                    # (B, 1, NC) one-hot: must equal (A)
        hotH = torch.from_numpy(np.tile(eye[:, None], (1, H, 1))).cuda()                       # (B, H, NC)
        blend = torch.from_numpy(rng.dirichlet(np.ones(NC), (B, 1)).astype(np.float32)).cuda()   # every speaker's row is read
        track = torch.from_numpy(rng.dirichlet(np.ones(NC), (B, H)).astype(np.float32)).cuda()

        def leg_a():
            return run(None, 0)

        def leg_b():
            return run(blend, 1)

        def leg_c():
            return run(track, H)

        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        want = leg_a().cpu().numpy()
        eq_b = bool(np.array_equal(run(hot1, 1).cpu().numpy(), want))
        eq_c = bool(np.array_equal(run(hotH, H).cpu().numpy(), want))
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc = timed((leg_a, leg_a, leg_b, leg_c), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        chunks = (H + 7) // 8
        shapes.append(dict(
            clips=B, code_rows=H, chunks=chunks, regions=a.regions,
            a_plain_ms=r3(ta), a2_plain_again_ms=r3(ta2), b_per_clip_blend_ms=r3(tb), c_per_row_track_ms=r3(tc),
            a_plain_ms_median=round(med(ta), 3), a2_plain_again_ms_median=round(med(ta2), 3), b_per_clip_blend_ms_median=round(med(tb), 3),
            c_per_row_track_ms_median=round(med(tc), 3),
            a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4), c_over_a=round(med(tc) / med(ta), 4),
            spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3), c_minus_a_ms=round(med(tc) - med(ta), 3),
            c_minus_a_per_chunk_us=round(1000 * (med(tc) - med(ta)) / chunks, 2),
            style_int_bytes=int(4 * pix.n_layers * 8 * B * 2 * pix.dim), graph_captures_in_timed_regions=int(cap1 - cap0),
            b_one_hot_codes_equal_plain=eq_b, c_one_hot_codes_equal_plain=eq_c))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="style_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
