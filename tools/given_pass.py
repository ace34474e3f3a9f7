"""What given rows cost in the body decode, and what the route they replace costs: same process, interleaved.

Full-size code predictor (2 048 classes, dim 256, 15 layers), B x 75 code rows for every B of --clips, Philox, no table, no log-probabilities:
  (A) the plain mixed pass                     `ts_pixelcnn_generate_mixed_given` with given_dev = NULL: sample_kernel on the chunk graphs
  (B) the same pass with a table of G = 0      the given variants of the samplers with nothing forced: what the variant launch costs
  (C) the same pass with G_b = H_b / 2         the first half of (A)'s own decode handed back (resume: the codes must equal (A)'s)
  (D) today's route for (C)                    one `GatedPixelCNN.run(pre_codes=, pre_aud=)` per distinct (H0, H): the prefix rows run the
                                               vertical stack only, the rest as eager launches or its own whole-call graph
Timed regions alternate A B C D A B C D ... after a warm-up of all four (graphs captured); HIP events on the stream; the figure is the
median region.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/given_pass.py --clips 32 256 --regions 5 --out profiles/given_pass.json
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
        G = H // 2
        mfcc = torch.from_numpy(synth.mfcc_features(B, B, 4 * H)).cuda()
        ids = torch.from_numpy((np.arange(B) % 4).astype(np.int64)).cuda()
        aud = w.audioencoder.forward_nlc(mfcc)
        lens = np.full(B, 4 * H, np.int32)
        lens_dev = torch.from_numpy(lens).cuda()
        clip_index = torch.arange(B, dtype=torch.int64, device="cuda")
        codes = torch.zeros((B, H, 2), dtype=torch.int64, device="cuda")

        def mixed(block, table):
            _lib.check(lib.ts_pixelcnn_generate_mixed_given(
                pix.handle(), _lib.dptr(ids), _lib.dptr(aud), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode, None, 1,
                _lib.dptr(clip_index), _lib.dptr(codes), None, 0, None, _lib.dptr(block), None if table is None else table.ctypes.data_as(i32p),
                None, _lib.stream_ptr()))
            return codes

        def plain():
            return mixed(None, None)

        head = plain().clone()
        zeros, half = np.zeros(B, np.int32), np.full(B, G, np.int32)
        pre_codes, pre_aud, tail_aud = head[:, :G].contiguous(), aud[:, :G].contiguous(), aud[:, G:].contiguous()

        def variant():
            return mixed(head, zeros)

        def given():
            return mixed(head, half)

        def prefix_route():
            return pix.run(ids, tail_aud, mode=mode, seed=1, pre_codes=pre_codes, pre_aud=pre_aud)[0]

        for _ in range(4):                                   # warm-up: every side's graphs are captured (the prefix route: its third sighting)
            plain(), variant(), given(), prefix_route()
        torch.cuda.synchronize()
        want = head.cpu().numpy()
        eq_variant = bool(np.array_equal(variant().cpu().numpy(), want))
        eq_given = bool(np.array_equal(given().cpu().numpy(), want))
        eq_prefix = bool(np.array_equal(prefix_route().cpu().numpy(), want[:, G:]))
        cap0 = pix.graph_captures()
        ta, tb, tc, td = timed((plain, variant, given, prefix_route), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows=H, given_rows=G, regions=a.regions,
            plain_ms=r3(ta), variant_g0_ms=r3(tb), given_half_ms=r3(tc), prefix_route_ms=r3(td),
            plain_ms_median=round(med(ta), 3), variant_g0_ms_median=round(med(tb), 3), given_half_ms_median=round(med(tc), 3),
            prefix_route_ms_median=round(med(td), 3),
            variant_cost_per_pass_ms=round(med(tb) - med(ta), 3), variant_ratio=round(med(tb) / med(ta), 4),
            given_half_ratio_to_plain=round(med(tc) / med(ta), 4), given_half_ratio_to_prefix_route=round(med(tc) / med(td), 4),
            sampler_launches_per_pass=2 * H, graph_captures_in_timed_regions=int(cap1 - cap0),
            variant_codes_equal_plain=eq_variant, given_codes_equal_plain=eq_given, prefix_route_codes_equal_plain_tail=eq_prefix))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="given_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
