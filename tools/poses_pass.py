"""What continuing from MOTION costs in the body decode, against continuing from codes and against the route it replaces: same process,
interleaved.

Full-size networks, B clips of mixed lengths (code rows spread over [rows / 3, rows], sorted longest first), Philox, G_b = H_b / 2.  Every
input of the pass — MFCC block, tables, ids — is staged on the device once, outside the timed regions; the regions call the C entries:
  (A) the mixed pass from device-resident given CODES    `ts_body_pixel_infer_mixed_given` on a (B, H_max, 2) device block
  (B) the same pass from device-resident POSES           `ts_body_pixel_infer_mixed_poses` on a (B, P_max, 129) device block: the encode inside
  (C) today's route for (B)                              one `encode_nlc` per network per distinct length, the codes copied to the host,
                                                         `given_block` + upload, then (A)'s call
Timed regions alternate A B C A B C ... after a warm-up of all three; HIP events on the stream around the whole call; the figure is the
median region.  The codes of B and C must equal A's.  Beside them, the codebook search alone on the pass's own shape: one paired launch
(form 1) against one launch per network (form 2), `--search-iters` launches each.
One JSON document, written to `--out` (default profiles/poses_pass.json).

    python tools/poses_pass.py --clips 32 256 --regions 5
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
    ap.add_argument("--search-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "poses_pass.json"))
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib, synth
    w, _ = bench.build_models(0)
    lib, ctx = _lib.load(), _lib.context(0)
    from talkshow_amd.modules import upload
    i32p = C.POINTER(C.c_int32)
    shapes = []
    for B in a.clips:
        rng = np.random.default_rng(B)
        rows = sorted((int(h) for h in rng.integers(max(2, a.rows // 3), a.rows + 1, B)), reverse=True)
        rows[0] = a.rows
        H, T = a.rows, 4 * a.rows
        lens = np.asarray([4 * h for h in rows], np.int32)
        mf = torch.zeros((B, T, 64), device="cuda")
        for b, h in enumerate(rows):
            mf[b, :4 * h] = torch.from_numpy(synth.mfcc_features(10 + b, 1, 4 * h)[0]).cuda()
        ids = torch.from_numpy((np.arange(B) % 4).astype(np.int64)).cuda()
        lens_dev = torch.from_numpy(lens).cuda()
        clip_index = torch.arange(B, dtype=torch.int64, device="cuda")
        G = np.asarray([h // 2 for h in rows], np.int32)
        plens = (4 * G).astype(np.int32)
        plens_dev = torch.from_numpy(plens).cuda()
        P_max = int(plens.max())
        motion = torch.zeros((B, P_max, 129), device="cuda")
        for b in range(B):
            motion[b, :plens[b]] = torch.from_numpy(synth.gt_poses(500 + b, 1, int(plens[b]))[0]).cuda()
        codes = torch.empty((B, H, 2), dtype=torch.int64, device="cuda")
        poses = torch.empty((B, 4 * H, 129), device="cuda")
        args = (w.audioencoder.handle(), w.generator.handle(), w.g_body.handle(), w.g_hand.handle(), _lib.dptr(mf), _lib.dptr(ids),
                lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, T, _lib.TS_SAMPLE_PHILOX, None, 1, _lib.dptr(clip_index), _lib.dptr(codes),
                _lib.dptr(poses), None, 0, None)

        def encode_by_length():
            """today's route: one uniform encode per network per distinct length, the codes copied to the host"""
            out = [None] * B
            for P in sorted({int(p) for p in plens}):
                idx = [b for b in range(B) if int(plens[b]) == P]
                x = motion[idx, :P]
                lb = w.g_body.encode_nlc(x[..., :39].contiguous(), want_quantized=False)[2]
                lh = w.g_hand.encode_nlc(x[..., 39:].contiguous(), want_quantized=False)[2]
                c = torch.stack([lb, lh], -1).cpu().numpy()
                for k, b in enumerate(idx):
                    out[b] = c[k]
            return out

        block_dev = upload(_lib.given_block(encode_by_length(), rows, 2048)[0], "cuda")

        def from_codes(block=None):
            _lib.check(lib.ts_body_pixel_infer_mixed_given(*args, _lib.dptr(block_dev if block is None else block), G.ctypes.data_as(i32p), None,
                                                           _lib.stream_ptr()))
            return codes

        def from_poses():
            _lib.check(lib.ts_body_pixel_infer_mixed_poses(*args, _lib.dptr(motion), P_max, plens.ctypes.data_as(i32p), _lib.dptr(plens_dev),
                                                           _lib.stream_ptr()))
            return codes

        def todays_route():
            return from_codes(upload(_lib.given_block(encode_by_length(), rows, 2048)[0], "cuda"))

        for _ in range(3):
            from_codes(), from_poses(), todays_route()
        torch.cuda.synchronize()
        want = from_codes().cpu().numpy()
        eq_b = bool(np.array_equal(from_poses().cpu().numpy(), want))
        eq_c = bool(np.array_equal(todays_route().cpu().numpy(), want))
        cap0 = w.generator.graph_captures()
        ta, tb, tc = timed((from_codes, from_poses, todays_route), a.regions)
        cap1 = w.generator.graph_captures()

        # the codebook search alone, on the shape the pass gives it: B x max G rows per network, 2 048 codes of 64
        Hs = int(G.max())
        z = [torch.randn((B * Hs, 64), device="cuda") for _ in range(2)]
        cb = [torch.randn((2048, 64), device="cuda") for _ in range(2)]
        slens = plens_dev
        out = torch.empty((B, Hs, 2), dtype=torch.int64, device="cuda")

        def search(form):
            def run():
                _lib.check(lib.ts_debug_vq_argmin_pair_masked(ctx, _lib.dptr(z[0]), _lib.dptr(z[1]), _lib.dptr(slens), B, Hs, _lib.dptr(cb[0]),
                                                              _lib.dptr(cb[1]), 2048, 2048, 64, 64, _lib.dptr(out), form, a.search_iters,
                                                              _lib.stream_ptr()))
            return run
        search(1)(), search(2)()
        s1, s2 = timed((search(1), search(2)), a.regions)
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, code_rows_max=a.rows, code_rows_total=int(sum(rows)), given_rows_total=int(G.sum()), distinct_pose_lengths=len({int(p) for p in plens}),
            regions=a.regions, from_codes_ms=r3(ta), from_poses_ms=r3(tb), todays_route_ms=r3(tc),
            from_codes_ms_median=round(med(ta), 3), from_poses_ms_median=round(med(tb), 3), todays_route_ms_median=round(med(tc), 3),
            encode_inside_cost_ms=round(med(tb) - med(ta), 3), todays_route_ratio_to_from_poses=round(med(tc) / med(tb), 4),
            graph_captures_in_timed_regions=int(cap1 - cap0), from_poses_codes_equal=eq_b, todays_route_codes_equal=eq_c,
            search_rows_per_network=B * Hs, search_iters=a.search_iters,
            search_paired_us_per_launch=round(1e3 * med(s1) / a.search_iters, 2),
            search_two_launches_us_per_pair=round(1e3 * med(s2) / a.search_iters, 2)))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="poses_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
