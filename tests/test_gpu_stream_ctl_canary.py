"""Memory-safety witness for `ts_pixelcnn_stream_step_ctl` (include/talkshow_hip.h, "streaming sessions"), in the manner of
tests/test_gpu_repeat_canary.py, through the C ABI: the second step (Hc = 3) of a session of 33 clips — across the 16- and 32-row slab
edges — under a sampling table, given rows, style rows, two bias tables and repetition records.  `codes_dev` and `logprob_dev` sit between
red zones pre-filled (zones and body) with a sentinel, every device input (`given_dev` and `bias_dev` among them) between poisoned zones;
after the call the zones are intact, the inputs unmodified, every documented element has lost the sentinel, and the outputs equal the
same step made through `PixelCNNStream.step` bit for bit.  A second test: what the entry refuses on a live session, with the row counter
unmoved.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import run_both

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
B, HC, NC = 33, 3, 4
RECS = [(0.8, 0.9, 0), (1.3, 1.0, 5), (1.0, 1.0, 0)]
REPS = [(3, 0.7, 0.3), (64, 1.0, 0.5), (0, 1.0, 1.0)]


@pytest.fixture(scope="module")
def net(golden):
    from talkshow_amd.modules import GatedPixelCNN
    g = golden("pix_small")
    input_dim, dim, n_layers, n_cls, seed = [int(v) for v in g["cfg"]]
    m = GatedPixelCNN(input_dim, dim, n_layers, n_cls, True, True).cuda()
    m.load_state_dict(synth.to_torch(synth.pixelcnn_state_dict(seed=seed, input_dim=input_dim, dim=dim, n_layers=n_layers, n_classes=n_cls)))
    assert n_cls == NC
    return m


def _inputs(V):
    rng = np.random.default_rng(33)
    aud = rng.standard_normal((B, 2 * HC, 256)).astype(np.float32)
    u = (0.999 * rng.random((B, 2 * HC, 2))).astype(np.float32)
    tabs = rng.standard_normal((2, 2, V)).astype(np.float32)
    tabs[1, :, V // 2:] = -np.inf
    index = (np.arange(B) % 3 - 1).astype(np.int32)                       # -1, 0, 1, ...
    grows = (np.arange(B) % (HC + 1)).astype(np.int32)                    # 0 .. Hc
    given = rng.integers(0, V, (B, HC, 2)).astype(np.int64)
    style = rng.random((B, NC)).astype(np.float32)
    return aud, u, tabs, index, grows, given, style


def test_second_step_between_red_zones(net):
    from talkshow_amd import _lib
    lib = _lib.load()
    V = net.input_dim
    aud, u, tabs, index, grows, given, style = _inputs(V)
    label = np.arange(B) % NC
    ctl = (_lib.TsSampling * B)()
    rep = (_lib.TsRepeat * B)()
    for b in range(B):
        ctl[b].temperature, ctl[b].top_p, ctl[b].top_k, ctl[b].reserved = *RECS[b % 3], 0
        rep[b].window, rep[b].presence, rep[b].frequency, rep[b].reserved = *REPS[b % 3], 0
    first = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u[:, :HC], repeat=[REPS[b % 3] for b in range(B)])

    def call(p):
        st = net.open_stream(label, B, HC)
        st.step(aud[:, :HC], **first)
        _lib.check(lib.ts_pixelcnn_stream_step_ctl(st._h, p["aud"], HC, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, 0, p["codes"], ctl, B, p["lp"],
                                                   p["given"], grows.ctypes.data_as(I32P), p["style"], p["bias"], 2,
                                                   index.ctypes.data_as(I32P), rep, B, _lib.stream_ptr()))
        assert st.rows == 2 * HC
        st.close()
    ins = {"aud": (np.ascontiguousarray(aud[:, HC:]), torch.float32), "u": (np.ascontiguousarray(u[:, HC:]), torch.float32),
           "given": (given, torch.int64), "style": (style, torch.float32), "bias": (tabs, torch.float32)}
    r = run_both(call, ins, {"codes": ((B, HC, 2), torch.int64), "lp": ((B, HC, 2), torch.float32)})
    codes, lp = r["codes"].reshape(B, HC, 2), r["lp"].view(np.float32).reshape(B, HC, 2)
    assert np.all((codes >= 0) & (codes < V)) and not np.isnan(lp).any()
    for b in range(B):                                                    # a taken code may lie outside its clip's kept set: -inf, never NaN
        assert np.isfinite(lp[b, grows[b]:]).all()
        assert np.array_equal(codes[b, :grows[b]], given[b, :grows[b]])
        if index[b] == 1:
            assert np.all(codes[b, grows[b]:] < V // 2), f"clip {b} drew a banned code"
    st = net.open_stream(label, B, HC)
    st.step(aud[:, :HC], **first)
    pc, pl = st.step(aud[:, HC:], mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(u[:, HC:]), sampling=[RECS[b % 3] for b in range(B)],
                     logprobs=True, given=[given[b, :grows[b]] if grows[b] else None for b in range(B)], style=list(style),
                     code_bias=[None if index[b] < 0 else tabs[index[b]] for b in range(B)], repeat=[REPS[b % 3] for b in range(B)])
    st.close()
    assert np.array_equal(pc.cpu().numpy(), codes) and np.array_equal(pl.cpu().numpy().view(np.uint32), lp.view(np.uint32))


def test_refusals_leave_the_row_counter_alone(net):
    from talkshow_amd import _lib
    lib = _lib.load()
    V = net.input_dim
    aud, u, tabs, index, grows, given, style = _inputs(V)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in
         dict(aud=aud[:, HC:], u=u[:, HC:], given=given, bias=tabs).items()}
    codes = torch.full((B, HC, 2), -7, dtype=torch.int64, device=dev)
    st = net.open_stream(np.arange(B) % NC, B, HC)
    st.step(aud[:, :HC], mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u[:, :HC])
    ctl = (_lib.TsSampling * 1)()
    ctl[0].temperature, ctl[0].top_p, ctl[0].top_k = 0.8, 1.0, 0
    rep = (_lib.TsRepeat * B)()
    for b in range(B):
        rep[b].window = 3
    rep[20].window = 65
    big = grows.copy()
    big[7] = HC + 1
    bad_index = index.copy()
    bad_index[30] = 2
    P = _lib.dptr

    def step(mode=_lib.TS_SAMPLE_UNIFORMS, ctl_=None, n_ctl=0, given_=None, grows_=None, bias_=None, n_bias=0, index_=None, rep_=None, n_rep=0):
        return lib.ts_pixelcnn_stream_step_ctl(st._h, P(t["aud"]), HC, mode, P(t["u"]), 0, 0, P(codes), ctl_, n_ctl, None, given_,
                                               None if grows_ is None else grows_.ctypes.data_as(I32P), None, bias_, n_bias,
                                               None if index_ is None else index_.ctypes.data_as(I32P), rep_, n_rep, _lib.stream_ptr())
    for what, kw, word in [("greedy with a table", dict(mode=_lib.TS_SAMPLE_GREEDY, ctl_=ctl, n_ctl=1), "TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX"),
                           ("greedy with a penalty", dict(mode=_lib.TS_SAMPLE_GREEDY, rep_=rep, n_rep=B), "TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX"),
                           ("g_b > Hc", dict(given_=P(t["given"]), grows_=big), "clip 7"),
                           ("given without its table", dict(given_=P(t["given"])), "row table"),
                           ("a window of 65", dict(rep_=rep, n_rep=B), "clip 20"),
                           ("a table index out of range", dict(bias_=P(t["bias"]), n_bias=2, index_=bad_index), "clip 30"),
                           ("two records for 33 clips", dict(ctl_=ctl, n_ctl=2), "n_ctl")]:
        assert step(**kw) != 0, what
        assert word in lib.ts_last_error().decode(), (what, lib.ts_last_error().decode())
        assert st.rows == HC, what
    torch.cuda.synchronize()
    assert bool((codes == -7).all()), "a refused step wrote codes"
    assert step(ctl_=ctl, n_ctl=1) == 0 and st.rows == 2 * HC                 # the session is still good
    torch.cuda.synchronize()
    assert bool(((codes >= 0) & (codes < V)).all())
    st.close()
