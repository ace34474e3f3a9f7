"""What guidance costs in the body decode: same process, interleaved, against the plain passes on either side of it.

Full-size code predictor (2 048 classes, dim 256, 15 layers), 75 code rows per clip for every B of --clips, Philox, no log-probabilities,
nothing given, integer ids.  Every leg runs under a neutral sampling table, one all-zero shared bias table and `repeat = (16, 0, 0)`: the
repetition family is the guided samplers' neighbour (the guided kernels are its kernels with the rule compiled in), so the same chain work
and the same sampler arithmetic run on both sides:
  (A)  2 B plain slots                          `ts_pixelcnn_generate_mixed_repeat`: slot 2 k holds clip k, slot 2 k + 1 the second
                                                conditioning of clip k (other audio, another speaker) as a clip of its own — the chain
                                                work of (B), no guidance
  (A') the same call again                      the run-to-run spread of (A) inside this process
  (B)  B clips, each guided against a shadow    `ts_pixelcnn_generate_guided` on the same 2 B slots: slot 2 k + 1 is the shadow of slot
                                                2 k, scale 2; half the sampler workgroups return at once, the other half read two rows
  (C)  B plain slots                            the clips alone: what guidance costs a host in slots is (B) - (C)
Scale 0 in (B) must return (A)'s codes of the even slots; a shadow's rows must be its primary's.  Timed regions alternate A A' B C
A A' B C ... after a warm-up of all (graphs captured); HIP events on the stream; the figure is the median region.  Nothing is asserted.
One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/guide_pass.py --clips 32 256 --regions 5 --out profiles/guide_pass.json
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
    ap.add_argument("--scale", type=float, default=2.0)
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
    rep = (_lib.TsRepeat * 1)()
    rep[0].window, rep[0].presence, rep[0].frequency, rep[0].reserved = 16, 0.0, 0.0, 0
    shapes = []
    for B in a.clips:
        H, B2 = a.rows, 2 * B
        mfcc = torch.from_numpy(synth.mfcc_features(B, B2, 4 * H)).cuda()      # slot 2 k: clip k; slot 2 k + 1: its second conditioning
        ids2 = torch.from_numpy((np.arange(B2) % NC).astype(np.int64)).cuda()
        aud2 = w.audioencoder.forward_nlc(mfcc)
        aud1, ids1 = aud2[0::2].contiguous(), ids2[0::2].contiguous()
        zero = torch.zeros((1, 2, V), device="cuda")

        def slots(n, aud, ids, index):
            lens = np.full(n, 4 * H, np.int32)
            return dict(n=n, aud=aud, ids=ids, lens=lens, lens_dev=torch.from_numpy(lens).cuda(), clip=torch.from_numpy(index).cuda(),
                        codes=torch.zeros((n, H, 2), dtype=torch.int64, device="cuda"), bidx=np.zeros(n, np.int32))
        two = slots(B2, aud2, ids2, np.arange(B2, dtype=np.int64))
        one = slots(B, aud1, ids1, np.arange(0, B2, 2, dtype=np.int64))         # the clips keep the Philox subsequences of the even slots
        guide = np.full(B2, -1, np.int32)
        guide[0::2] = np.arange(1, B2, 2)
        scales = {s: np.where(guide >= 0, np.float32(s), np.float32(0)).astype(np.float32) for s in (a.scale, 0.0)}

        def run(s, scale=None):
            fixed = (pix.handle(), _lib.dptr(s["ids"]), _lib.dptr(s["aud"]), s["lens"].ctypes.data_as(i32p), _lib.dptr(s["lens_dev"]), s["n"], H, mode,
                     None, 1, _lib.dptr(s["clip"]), _lib.dptr(s["codes"]))
            pieces = dict(ctl=neutral, n_ctl=1, bias=_lib.dptr(zero), n_bias=1, bias_index=s["bidx"].ctypes.data_as(i32p), rep=rep, n_rep=1)
            if scale is not None:
                pieces.update(guide=guide.ctypes.data_as(i32p), guide_scale=_lib.fptr(scales[scale]))
            _lib.pixelcnn_mixed_call(fixed, **pieces)
            return s["codes"]

        def leg_a():
            return run(two)

        def leg_b():
            return run(two, a.scale)

        def leg_c():
            return run(one)

        for _ in range(4):                                   # warm-up: every leg's graphs are captured
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        want = leg_a().cpu().numpy().copy()
        zero_b = run(two, 0.0).cpu().numpy().copy()
        got_b = leg_b().cpu().numpy().copy()
        got_c = leg_c().cpu().numpy().copy()
        cap0 = pix.graph_captures()
        ta, ta2, tb, tc = timed((leg_a, leg_a, leg_b, leg_c), a.regions)
        cap1 = pix.graph_captures()
        med = statistics.median
        r3 = lambda xs: [round(x, 3) for x in xs]            # noqa: E731
        shapes.append(dict(
            clips=B, slots_a=B2, slots_b=B2, slots_c=B, code_rows=H, sampler_launches=2 * H, regions=a.regions, scale=a.scale,
            a_plain_2b_ms=r3(ta), a2_plain_2b_again_ms=r3(ta2), b_guided_ms=r3(tb), c_plain_b_ms=r3(tc),
            a_plain_2b_ms_median=round(med(ta), 3), a2_plain_2b_again_ms_median=round(med(ta2), 3), b_guided_ms_median=round(med(tb), 3),
            c_plain_b_ms_median=round(med(tc), 3), spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
            b_over_a=round(med(tb) / med(ta), 4), b_minus_c_ms=round(med(tb) - med(tc), 3), b_over_c=round(med(tb) / med(tc), 4),
            b_minus_a_per_sampler_launch_us=round(1000 * (med(tb) - med(ta)) / (2 * H), 3), graph_captures_in_timed_regions=int(cap1 - cap0),
            b_scale_zero_codes_equal_a_even_slots=bool(np.array_equal(zero_b[0::2], want[0::2])),
            b_shadow_rows_equal_primaries=bool(np.array_equal(got_b[1::2], got_b[0::2])),
            c_codes_equal_a_even_slots=bool(np.array_equal(got_c, want[0::2])),
            b_share_of_positions_moved=round(float((got_b[0::2] != want[0::2]).mean()), 4)))
        print(json.dumps(shapes[-1]))
    doc = dict(tool="guide_pass", device=torch.cuda.get_device_name(0), shapes=shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
