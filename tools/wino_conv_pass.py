"""The VQ conv stacks of one pass, conv family and misc family apart (ts_prof: HIP event pairs around every launch): both encoders and both
decoders of B clips of 300 frames in lockstep (ts_body_vq_infer with a reconstruction) — every layer the Winograd lowering touches, and
nothing of the PixelCNN chain.  TS_B = clips (default 256), TS_CONV_WINO as for the library; TS_PROF_LOG=1 adds one stderr line per conv
launch.  Prints one JSON line: milliseconds and launches per pass of each family, medians over TS_ITERS passes (default 5)."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from talkshow_amd import _lib, synth  # noqa: E402

lib = _lib.load()
w, _ = bench.build_models(0)
B, T, iters = int(os.environ.get("TS_B", "256")), 300, int(os.environ.get("TS_ITERS", "5"))
gt = torch.from_numpy(synth.gt_poses(2000, B, T)).cuda()
codes = torch.empty((B, T // 4, 2), dtype=torch.int64, device="cuda")
recon = torch.empty((B, T, 129), dtype=torch.float32, device="cuda")


def step():
    _lib.check(lib.ts_body_vq_infer(w.g_body.handle(), w.g_hand.handle(), _lib.dptr(gt), B, T, _lib.dptr(codes), _lib.dptr(recon), _lib.stream_ptr()))


step()
torch.cuda.synchronize()
ctx = _lib.context(0)
conv, misc, n = [], [], None
for _ in range(iters):
    _lib.check(lib.ts_prof_enable(ctx, 1))
    step()
    torch.cuda.synchronize()
    ms, nl, fl = (C.c_double * 3)(), (C.c_int64 * 3)(), (C.c_double * 3)()
    _lib.check(lib.ts_prof_read(ctx, ms, nl, fl, 1))
    _lib.check(lib.ts_prof_enable(ctx, 0))
    conv.append(ms[0]), misc.append(ms[2])
    n = (int(nl[0]), int(nl[2]))
print(json.dumps({"clips": B, "conv_ms": statistics.median(conv), "misc_ms": statistics.median(misc), "conv_plus_misc_ms": statistics.median(c + m for c, m in zip(conv, misc)),
                  "conv_launches": n[0], "misc_launches": n[1], "conv_ms_all": conv, "misc_ms_all": misc}))
