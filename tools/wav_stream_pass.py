"""What feeding a seamless session SAMPLES costs, and how far the running clamp is from the one-shot's on real speech.

Full-size networks (code predictor 2 048 / 256 / 15, VQ nets of 1 024 hidden channels); --clips clips of 16 kHz noise whose one-shot front
end gives 4 x --rows MFCC rows; one region = the whole clip through a seamless session in --rows / --step pushes and its flush, Philox:
  (A)  the seamless session fed the precomputed MFCC rows, 4 x --step a push        `open_stream(..., seamless=True)`
  (A') the same again: the run-to-run spread of (A) inside this process
  (B)  the session fed the samples of those pushes through `push_wav`               `open_stream(..., seamless=True, wav_sr=16000, wav_db=peak)`
       (peak mode under `MFCC.peak_db`, so the body does the work of (A) on the same bits; its pushes are cut by samples, not by rows)
A seamless session ends with its flush, so every region has a session of its own, opened ahead of the timed regions.  Timed regions
alternate A A' B after a warm-up of two regions per leg; HIP events on the stream; the figure is the median region.

The open question (talkshow_hip.h, "wav sessions"): a live host does not know its recording's maximum, so it runs the clamp in "running" mode.
On the three tracked recordings (tests/golden/audio/) the tool reports the share of MFCC rows whose bits differ between "running" and "peak"
(peak = `MFCC.peak_db`, which gives the one-shot rows), the largest difference, and the share of greedy codes that change.

Nothing is asserted.  One JSON document: `--out FILE` writes it there (default: stdout only).

    python tools/wav_stream_pass.py --regions 5 --out profiles/wav_stream_pass.json
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
WARMUP = 2
RECORDINGS = ("style.wav", "1st-page.wav", "french.wav")


def running_against_peak(w, name):
    """One tracked recording through the front-end session in both dB modes, and both row sets through the greedy body pass."""
    from talkshow_amd import _lib
    from talkshow_amd.frontend import load_wav
    from talkshow_amd.modules import MFCC
    x, sr = load_wav(os.path.join(REPO, "tests", "golden", "audio", name))
    wav = torch.from_numpy(x.mean(axis=0, dtype=np.float32)[None]).cuda()
    m = MFCC(sr, 22000, 30)
    one_shot, peak = m(wav), m.peak_db(wav)
    rows = {}
    for mode, db in (("peak", peak), ("running", "running")):
        st = m.open_stream(1, int(wav.shape[1]), db=db)
        rows[mode] = torch.cat([st.push(wav), st.flush()], dim=1)
        st.close()
    differ = (rows["running"].view(torch.int32) != rows["peak"].view(torch.int32)).any(dim=2)[0]
    ids = np.zeros(1, np.int64)
    codes = {k: w.generate_batch(v, ids, mode=_lib.TS_SAMPLE_GREEDY)[0] for k, v in rows.items()}
    last = int(differ.nonzero().max().item()) if bool(differ.any()) else -1
    return dict(recording=name, sample_rate=sr, samples=int(wav.shape[1]), mfcc_rows=int(differ.numel()),
                peak_db=round(float(peak[0]), 4), peak_rows_equal_one_shot=bool(torch.equal(rows["peak"], one_shot)),
                rows_differing=int(differ.sum()), rows_differing_share=round(float(differ.float().mean()), 4), last_differing_row=last,
                max_abs_difference=round(float((rows["running"] - rows["peak"]).abs().max()), 4),
                greedy_codes=int(codes["peak"].numel()), greedy_codes_changed=int((codes["running"] != codes["peak"]).sum()),
                greedy_codes_changed_share=round(float((codes["running"] != codes["peak"]).float().mean()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--step", type=int, default=15)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from talkshow_amd import _lib
    from talkshow_amd.frontend import WavStreamPlan
    from talkshow_amd.modules import MFCC
    w, _ = bench.build_models(0)
    B, H, HC = a.clips, a.rows, a.step
    clock = WavStreamPlan(16000, 22000, 30)
    T = 4 * H
    N = -((-(T - 1) * clock.hop - 72) * clock.norig // clock.nnew)          # N22 = ceil(N nnew / norig) just above (T - 1) hop: T rows
    assert clock.total22(N) // clock.hop + 1 == T
    rng = np.random.default_rng(B)
    wav = torch.from_numpy((0.3 * rng.standard_normal((B, N)) * np.abs(np.sin(np.linspace(0.1, 40.0, N)))[None]).astype(np.float32)).cuda()
    m = MFCC(16000, 22000, 30)
    mfcc, peak = m(wav), m.peak_db(wav)
    pushes = H // HC
    chunks = [mfcc[:, 4 * r:4 * (r + HC)].contiguous() for r in range(0, H, HC)]
    per = -(-N // pushes)
    wav_chunks = [wav[:, k:k + per].contiguous() for k in range(0, N, per)]
    ids = (np.arange(B) % w.num_classes).astype(np.int64)
    draw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=1)
    n_each = WARMUP + a.regions
    fed_rows = [w.open_stream(ids, B, 4 * HC, seamless=True) for _ in range(2 * n_each)]
    fed_wav = [w.open_stream(ids, B, 4 * HC, seamless=True, wav_sr=16000, wav_db=peak, max_samples=per) for _ in range(n_each)]
    state = dict(seamless_state_bytes=fed_rows[0].state_bytes, front_end_state_bytes=fed_wav[0].front.state_bytes)
    frames = {"a": 0, "a2": 0, "b": 0}

    def rows_leg(name):
        def run():
            st = fed_rows.pop()
            for ch in chunks:
                frames[name] += int(st.push(ch, **draw).shape[1])
            frames[name] += int(st.flush(**draw).shape[1])
            return st
        return run

    def wav_leg():
        st = fed_wav.pop()
        for ch in wav_chunks:
            frames["b"] += int(st.push_wav(ch, **draw).shape[1])
        frames["b"] += int(st.flush(**draw).shape[1])
        return st
    legs = (rows_leg("a"), rows_leg("a2"), wav_leg)
    done = []
    for _ in range(WARMUP):
        for fn in legs:
            done.append(fn())
    torch.cuda.synchronize()
    acc = [[] for _ in legs]
    for _ in range(a.regions):
        for fn, t in zip(legs, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            done.append(fn())
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    for s in done:
        s.close()
    ta, ta2, tb = acc
    med = statistics.median
    r3 = lambda xs: [round(x, 3) for x in xs]                # noqa: E731
    k = m.constants
    doc = dict(
        tool="wav_stream_pass", device=torch.cuda.get_device_name(0), clips=B, code_rows=H, step_rows=HC, pushes_per_region=pushes,
        regions=a.regions, sample_rate=16000, samples_per_clip=N, samples_per_push=per, mfcc_rows=T,
        a_rows_ms=r3(ta), a2_rows_again_ms=r3(ta2), b_wav_ms=r3(tb),
        a_rows_ms_median=round(med(ta), 3), a2_rows_again_ms_median=round(med(ta2), 3), b_wav_ms_median=round(med(tb), 3),
        a2_over_a=round(med(ta2) / med(ta), 4), b_over_a=round(med(tb) / med(ta), 4),
        spread_a_ms=round(abs(med(ta2) - med(ta)), 3), b_minus_a_ms=round(med(tb) - med(ta), 3),
        b_minus_a_per_push_us=round(1000 * (med(tb) - med(ta)) / pushes, 3),
        pose_frames_per_region={key: v // n_each for key, v in frames.items()},
        latency_ms=round(1000 * (1024 / 22000 + (k["kw"] - k["width"] - 1) / 16000), 3), resampler=k, **state,
        running_against_peak=[running_against_peak(w, name) for name in RECORDINGS])
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
