"""Memory-safety witness for `ts_pixelcnn_stream_step_guided` (include/talkshow_hip.h, "session pairs"), in the manner of
tests/test_gpu_stream_ctl_canary.py, through the C ABI: the second step (Hc = 3) of a session of S = 2 slots (one pair) and of S = 33
slots (sixteen pairs across the 16- and 32-row slab edges, shadows next to, apart from and below their primaries, slot 32 plain) under a
sampling table, given rows, style rows, two bias tables, repetition records and the step's own scales.  `codes_dev` and `logprob_dev`
sit between red zones pre-filled (zones and body) with a sentinel, every device input between poisoned zones; after the call the zones
are intact, the inputs unmodified, every documented element has lost the sentinel — a shadow's rows are written by its primary's
workgroup through the slot strides —, and the outputs equal the same step made through `PixelCNNStream.step` bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_poses_canary import run_both

pytestmark = pytest.mark.gpu
I32P = C.POINTER(C.c_int32)
HC, NC = 3, 4
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


def pairs_of(S):
    """S = 2: (1, 0), the shadow below its primary.  S = 33: shadows next to (2k, 2k + 1 for the first eight slots), apart from (8 + k,
    20 + k) and below (31, 30) their primaries; slot 32 and a few more stay plain."""
    if S == 2:
        return {1: (0, 2.0)}
    p = {2 * k: (2 * k + 1, 2.0) for k in range(4)}
    p.update({8 + k: (20 + k, -0.5) for k in range(8)})
    p[31] = (30, 1.5)
    return p


@pytest.mark.parametrize("S", [2, 33])
def test_second_guided_step_between_red_zones(net, S):
    from talkshow_amd import _lib
    lib = _lib.load()
    V = net.input_dim
    rng = np.random.default_rng(S)
    aud = rng.standard_normal((S, 2 * HC, 256)).astype(np.float32)
    u = (0.999 * rng.random((S, 2 * HC, 2))).astype(np.float32)
    tabs = rng.standard_normal((2, 2, V)).astype(np.float32)
    tabs[1, :, V // 2:] = -np.inf
    index = (np.arange(S) % 3 - 1).astype(np.int32)
    grows = (np.arange(S) % (HC + 1)).astype(np.int32)
    given = rng.integers(0, V, (S, HC, 2)).astype(np.int64)
    style = rng.random((S, NC)).astype(np.float32)
    label = np.arange(S) % NC
    pairs = pairs_of(S)
    shadow_of = {g: b for b, (g, _) in pairs.items()}
    scales = np.zeros(S, np.float32)
    for b in pairs:
        scales[b] = 0.75 + 0.25 * (b % 3)                                  # the step's own scales, read at primaries only
    scales[[g for g in shadow_of]] = np.nan                               # ... so a shadow's entry may hold anything
    ctl = (_lib.TsSampling * S)()
    rep = (_lib.TsRepeat * S)()
    for b in range(S):
        ctl[b].temperature, ctl[b].top_p, ctl[b].top_k, ctl[b].reserved = *RECS[b % 3], 0
        rep[b].window, rep[b].presence, rep[b].frequency, rep[b].reserved = *REPS[b % 3], 0
    first = dict(mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=u[:, :HC], repeat=[REPS[b % 3] for b in range(S)])

    def call(p):
        st = net.open_stream(label, S, HC, pairs=pairs)
        st.step(aud[:, :HC], **first)
        _lib.check(lib.ts_pixelcnn_stream_step_guided(st._h, p["aud"], HC, _lib.TS_SAMPLE_UNIFORMS, p["u"], 0, 0, p["codes"], ctl, S, p["lp"],
                                                      p["given"], grows.ctypes.data_as(I32P), p["style"], p["bias"], 2,
                                                      index.ctypes.data_as(I32P), rep, S, scales.ctypes.data_as(C.POINTER(C.c_float)),
                                                      _lib.stream_ptr()))
        assert st.rows == 2 * HC
        st.close()
    ins = {"aud": (np.ascontiguousarray(aud[:, HC:]), torch.float32), "u": (np.ascontiguousarray(u[:, HC:]), torch.float32),
           "given": (given, torch.int64), "style": (style, torch.float32), "bias": (tabs, torch.float32)}
    r = run_both(call, ins, {"codes": ((S, HC, 2), torch.int64), "lp": ((S, HC, 2), torch.float32)})
    codes, lp = r["codes"].reshape(S, HC, 2), r["lp"].view(np.float32).reshape(S, HC, 2)
    assert np.all((codes >= 0) & (codes < V)) and not np.isnan(lp).any()
    for g, b in shadow_of.items():
        assert np.array_equal(codes[g], codes[b]) and np.array_equal(lp[g].view(np.uint32), lp[b].view(np.uint32)), (b, g)
    for b in range(S):
        if b in shadow_of:
            continue
        assert np.isfinite(lp[b, grows[b]:]).all()
        assert np.array_equal(codes[b, :grows[b]], given[b, :grows[b]])
        if index[b] == 1:
            assert np.all(codes[b, grows[b]:] < V // 2), f"clip {b} drew a banned code"
    st = net.open_stream(label, S, HC, pairs=pairs)
    st.step(aud[:, :HC], **first)
    pc, pl = st.step(aud[:, HC:], mode=_lib.TS_SAMPLE_UNIFORMS, uniforms=np.ascontiguousarray(u[:, HC:]), sampling=[RECS[b % 3] for b in range(S)],
                     logprobs=True, given=[given[b, :grows[b]] if grows[b] else None for b in range(S)], style=list(style),
                     code_bias=[None if index[b] < 0 else tabs[index[b]] for b in range(S)], repeat=[REPS[b % 3] for b in range(S)],
                     guide={b: float(scales[b]) for b in pairs})
    st.close()
    assert np.array_equal(pc.cpu().numpy(), codes) and np.array_equal(pl.cpu().numpy().view(np.uint32), lp.view(np.uint32))


# ---- the guided seamless session and its row-spread kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E,R,r0,n", [(1, 1, 5, 0, 5), (3, 2, 9, 2, 4), (33, 7, 12, 3, 9)])
def test_the_row_spread_kernel_between_red_zones(S, E, R, r0, n):
    from talkshow_amd import _lib
    lib = _lib.load()
    W = 256
    rng = np.random.default_rng(S)
    src = rng.standard_normal((E, R, W)).astype(np.float32)
    smap = (np.arange(S) * 5 % E).astype(np.int32)                         # a map that repeats a source (S > E)
    assert S == 1 or len(set(smap.tolist())) < S

    def call(p):
        _lib.check(lib.ts_debug_stream_spread_rows(p["src"], p["dst"], smap.ctypes.data_as(I32P), S, E, R, r0, n, W, _lib.stream_ptr()))
    r = run_both(call, {"src": (src, torch.float32)}, {"dst": ((S, n, W), torch.float32)})
    assert np.array_equal(r["dst"].view(np.float32).reshape(S, n, W), src[smap, r0:r0 + n])
    bad = smap.copy()
    bad[-1] = E
    dst = torch.zeros((S, n, W), device="cuda")
    assert lib.ts_debug_stream_spread_rows(_lib.dptr(torch.from_numpy(src).cuda()), _lib.dptr(dst), bad.ctypes.data_as(I32P), S, E, R, r0, n, W,
                                           _lib.stream_ptr()) != 0
    assert "names stream" in lib.ts_last_error().decode()


@pytest.mark.parametrize("B,n_g", [(1, 1), (17, 16)], ids=["S=2", "S=33"])
def test_guided_push_and_flush_between_red_zones(net, B, n_g):
    """One push of 40 frames (3 code rows, no pose frame yet) and the flush (7 rows, 40 frames) of a guided session through the C ABI:
    every output between red zones, and equal to the same calls through `SeamlessBodyStream`."""
    from nets.smplx_body_pixel import TrainWrapper
    from talkshow_amd import _lib
    from talkshow_amd.modules import AudioEncoder, VQVAE
    lib = _lib.load()
    V = net.input_dim
    w = object.__new__(TrainWrapper)
    w.generator = net
    w.audioencoder = AudioEncoder(64, 256, 2).cuda()
    w.audioencoder.load_state_dict(synth.to_torch(synth.audioencoder_state_dict(seed=3)))
    w.g_body, w.g_hand = VQVAE(39, 64, V, 128, 2).cuda(), VQVAE(90, 64, V, 128, 2).cuda()
    w.g_body.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=39, num_embeddings=V, num_hiddens=128)))
    w.g_hand.load_state_dict(synth.to_torch(synth.vqvae_state_dict(seed=3, in_dim=90, num_embeddings=V, num_hiddens=128, salt=1)))
    w.each_dim, w.num_classes = [0, 39, 90], NC
    S, T = B + n_g, 40
    own = [k % 2 == 0 for k in range(n_g)]                                 # every other shadow hears audio of its own
    E = B + sum(own)
    shadow_of = np.arange(n_g, dtype=np.int32)
    enc_of, e = [], B
    for k in range(n_g):
        enc_of.append(e if own[k] else -1)
        e += own[k]
    enc_of = np.asarray(enc_of, np.int32)
    mf = synth.mfcc_features(70 + S, E, T)
    ids = (np.arange(S) * 3 + 1) % NC
    scales = np.full(n_g, 2.0, np.float32)
    ids_dev = torch.from_numpy(ids.astype(np.int64)).cuda()
    FP = C.POINTER(C.c_float)
    PH, sp = _lib.TS_SAMPLE_PHILOX, _lib.stream_ptr

    def call(p):
        h = C.c_void_p()
        _lib.check(lib.ts_body_stream_open_guided(w.audioencoder.handle(), net.handle(), w.g_body.handle(), w.g_hand.handle(), _lib.dptr(ids_dev),
                                                  B, n_g, shadow_of.ctypes.data_as(I32P), enc_of.ctypes.data_as(I32P), None,
                                                  scales.ctypes.data_as(FP), T, sp(), C.byref(h)))
        bytes0 = lib.ts_body_stream_state_bytes(h)
        # the plain entry is refused on a session with shadows, and moves no counter
        assert lib.ts_body_stream_push(h, p["mf"], T, PH, None, 9, 0, p["c1"], None, None, 0, None, None, None, None, None, 0, None, None, 0,
                                       sp()) != 0
        assert "opened with shadows" in lib.ts_last_error().decode() and lib.ts_body_stream_frames_in(h) == 0
        _lib.check(lib.ts_body_stream_push_guided(h, p["mf"], T, PH, None, 9, 0, p["c1"], None, None, 0, p["l1"], None, None, None, None, 0, None,
                                                  None, 0, None, sp()))
        _lib.check(lib.ts_body_stream_flush_guided(h, PH, None, 9, 0, p["c2"], p["poses"], None, 0, p["l2"], None, None, None, None, 0, None,
                                                   None, 0, None, sp()))
        assert lib.ts_body_stream_state_bytes(h) == bytes0 and lib.ts_body_stream_pose_frames(h) == T
        torch.cuda.synchronize()
        lib.ts_body_stream_close(h)
    outs = {"c1": ((S, 3, 2), torch.int64), "l1": ((S, 3, 2), torch.float32), "c2": ((S, 7, 2), torch.int64), "l2": ((S, 7, 2), torch.float32),
            "poses": ((B, T, 129), torch.float32)}
    r = run_both(call, {"mf": (mf, torch.float32)}, outs)
    guide = [{"scale": 2.0, "id": int(ids[B + k]), "audio": own[k]} for k in range(n_g)] + [None] * (B - n_g)
    st = w.open_stream(ids[:B].astype(np.int64), B, T, seamless=True, guide=guide)
    mfd = torch.from_numpy(mf).cuda()
    shadow_mf = iter(mfd[B:])
    o1 = st.push(mfd[:B], seed=9, return_codes=True, logprobs=True, guide=[{"mfcc": next(shadow_mf)} if k < n_g and own[k] else None for k in range(B)])
    o2 = st.flush(seed=9, return_codes=True, logprobs=True)
    st.close()
    assert np.array_equal(r["c1"].reshape(S, 3, 2)[:B], o1[1].cpu().numpy()) and np.array_equal(r["c2"].reshape(S, 7, 2)[:B], o2[1].cpu().numpy())
    assert np.array_equal(r["l2"].reshape(S, 7, 2)[:B], o2[2].cpu().numpy().view(np.int32))
    assert np.array_equal(r["poses"].reshape(B, T, 129), o2[0].cpu().numpy().view(np.int32))
    for k in range(n_g):                                                    # a shadow's rows are its primary's
        assert np.array_equal(r["c2"].reshape(S, 7, 2)[B + k], r["c2"].reshape(S, 7, 2)[k])
