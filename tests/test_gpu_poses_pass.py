"""Given poses through the wrappers (`ts_vqvae_encode_pair_masked`, `ts_body_vq_infer_mixed`, `ts_body_pixel_infer_mixed_poses`;
`encode_clips` / `reconstruct_clips` on the VQ wrapper, `given_poses=` / `score_clips` / `score_motion_clips` on the body wrapper).

The contract (include/talkshow_hip.h, "given poses"): a clip's codes, latents and reconstruction in a mixed encode are those of the clip
alone, whatever the padding holds; a pass that continues from poses equals the pass that continues from the codes of those poses; scoring
in one pass equals scoring clip by clip.  Every check is EQUALITY of bits.  The wrapper is the shipped one at full size: the code predictor's
vocabulary has to be the VQ-VAEs' codebook size (2 048) for encoded codes to be codes it knows; the clips are short instead.  Every test fails on a
build without the feature: the methods and the keyword do not exist there.
"""
import argparse
import os

import numpy as np
import pytest
import torch

from talkshow_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = [4, 5, 7, 8, 30, 31, 77, 300]                 # pose frames: one row, remainders 1 and 3, two rows, ..., a long clip


def _np(t):
    return t.cpu().numpy()


def bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def w():
    """The shipped body wrapper: audio encoder, code predictor and VQ-VAEs at full size."""
    import bench
    return bench.build_models(0, seed=7)[0]


@pytest.fixture(scope="module")
def vw(w):
    """The VQ wrapper on the SAME two networks."""
    from nets.init_model import init_model
    from talkshow_amd.config import load_JsonConfig
    v = init_model("s2g_body_vq", argparse.Namespace(gpu=0, infer=True), load_JsonConfig(os.path.join(REPO, "config", "body_vq.json")))
    v.g_body, v.g_hand = w.g_body, w.g_hand
    return v


@pytest.fixture(scope="module")
def alone(vw):
    """Every length of PS encoded and reconstructed ALONE by the uniform entries, once: P -> (pose clip, codes, z_body, z_hand, recon)."""
    out = {}
    for k, P in enumerate(PS):
        x = synth.gt_poses(900 + k, 1, P)
        zb, _, lb = vw.g_body.encode_nlc(x[..., :39].copy(), want_z=True, want_quantized=False)
        zh, _, lh = vw.g_hand.encode_nlc(x[..., 39:].copy(), want_z=True, want_quantized=False)
        codes, recon = vw.reconstruct_batch(x)
        assert np.array_equal(_np(codes)[0], np.stack([_np(lb)[0], _np(lh)[0]], -1))
        out[P] = (x[0], _np(codes)[0], _np(zb)[0], _np(zh)[0], _np(recon)[0])
    return out


# ---- 1. the mixed encode against the clip alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 8, 33])
def test_encode_equals_the_clip_alone(vw, alone, B):
    rng = np.random.default_rng(B)
    Ps = [PS[i % len(PS)] for i in rng.permutation(max(B, len(PS)))[:B]] if B > 1 else [77]
    clips = [alone[P][0] for P in Ps]
    enc = vw.encode_clips(clips, want_z=True)
    rec = vw.reconstruct_clips(clips)
    # the same clips in a block whose padding is NaN
    T_max = max(Ps)
    block = np.full((B, T_max, 129), np.nan, F32)
    for b, P in enumerate(Ps):
        block[b, :P] = clips[b]
    enc_nan = vw.encode_clips(block, want_z=True, lens=Ps)
    rec_nan = vw.reconstruct_clips(block, lens=Ps)
    for b, P in enumerate(Ps):
        _, codes, zb, zh, recon = alone[P]
        for tag, e, r in (("zero padding", enc[b], rec[b]), ("NaN padding", enc_nan[b], rec_nan[b])):
            assert np.array_equal(_np(e[0]), codes) and np.array_equal(_np(r[0]), codes), f"codes of clip {b} (P = {P}, {tag})"
            assert np.array_equal(bits(e[1]), bits(zb)) and np.array_equal(bits(e[2]), bits(zh)), f"z of clip {b} (P = {P}, {tag})"
            assert r[1].shape == (4 * (P // 4), 129) and np.array_equal(bits(r[1]), bits(recon)), f"reconstruction of clip {b} (P = {P}, {tag})"


# ---- 2. continuation ------------------------------------------------------------------------------------------------------------------------
ROWS = [20, 17, 17, 9, 8, 3]
RECS = [(0.8, 0.9, 0), (1.0, 1.0, 1), (1.7, 1.0, 12), (0.5, 0.5, 40), (1.0, 1.0, 0), (4.0, 0.95, 64)]


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(21)
    order = rng.permutation(len(ROWS))
    rows = [ROWS[i] for i in order]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(3000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(len(rows)) % 4).astype(np.int64)
    motion = [synth.gt_poses(700 + k, 1, 4 * h + 3)[0] for k, h in enumerate(rows)]          # 4 H_b + 3 frames of motion per clip
    return rows, mf, ids, [RECS[i] for i in order], motion


def _kw(how, recs):
    from talkshow_amd import _lib
    return dict(mode=_lib.TS_SAMPLE_PHILOX, seed=123, clip_index0=50, sampling=recs) if how == "philox" else dict(mode=_lib.TS_SAMPLE_GREEDY)


def _same(res_a, res_b, what):
    assert len(res_a) == len(res_b)
    for b, (x, y) in enumerate(zip(res_a, res_b)):
        for name, s, t in zip(("codes", "poses", "log-probabilities"), x, y):
            assert np.array_equal(bits(s), bits(t)), f"{what}: {name} of clip {b}"


@pytest.mark.parametrize("how", ["philox", "greedy"])
def test_given_poses_equal_given_codes(w, vw, clips, how):
    rows, mf, ids, recs, motion = clips
    kw = _kw(how, recs)
    # G_b in {0, 1, H_b / 2, H_b}, frames with remainders
    G = [0, 1, rows[2] // 2, rows[3], rows[4] // 2, rows[5]]
    frames = [0, 5, 4 * G[2] + 3, 4 * G[3], 4 * G[4] + 1, 4 * G[5] + 3]
    gp = [None if f == 0 else motion[b][:f] for b, f in enumerate(frames)]
    codes = vw.encode_clips([g for g in gp if g is not None])
    given, k = [], 0
    for g in gp:
        given.append(None if g is None else _np(codes[k]))
        k += g is not None
    assert [0 if g is None else len(g) for g in given] == G
    want = w.generate_clips(mf, ids, logprobs=True, given=given, **kw)
    got = w.generate_clips(mf, ids, logprobs=True, given_poses=gp, **kw)
    _same(got, want, f"{how}, given_poses")
    for b, g in enumerate(G):
        assert np.array_equal(_np(got[b][0])[:g], given[b] if g else _np(got[b][0])[:0])
    # a second call with the same shapes captures nothing
    after = w.generator.graph_captures()
    w.generate_clips(mf, ids, logprobs=True, given_poses=gp, **kw)
    assert w.generator.graph_captures() == after
    # one pass that mixes given codes, given poses and nothing
    mixed_g = [given[0], given[1], None, given[3], None, None]
    mixed_p = [None, None, gp[2], None, gp[4], None]
    ref = [given[0], given[1], given[2], given[3], given[4], None]
    _same(w.generate_clips(mf, ids, logprobs=True, given=mixed_g, given_poses=mixed_p, **kw),
          w.generate_clips(mf, ids, logprobs=True, given=ref, **kw), f"{how}, both kinds in one pass")
    # given_poses of Nones is the pass without the keyword
    _same(w.generate_clips(mf, ids, logprobs=True, given_poses=[None] * len(rows), **kw), w.generate_clips(mf, ids, logprobs=True, **kw), "all None")


def test_given_poses_from_recordings(w, vw):
    """`given_poses=` through `generate_clips_from_wav` (the recordings are sorted by sample count, the entries follow them): equal to
    `given=` on the encoded codes, poses alone and both kinds in one pass."""
    from talkshow_amd import _lib
    from talkshow_amd.frontend import mixed_tables
    rng = np.random.default_rng(4)
    ns = [9000, 30000, 14000, 22000]                                   # submitted out of order
    wavs = [(0.1 * rng.standard_normal(n)).astype(F32) for n in ns]
    rows = [int(t) // 4 for t in mixed_tables(ns, 16000, 22000, 30)["mfcc_rows"]]
    assert min(rows) >= 2
    frames = [4 * rows[0] + 2, 0, 4 * (rows[2] // 2) + 1, 4]
    gp = [None if f == 0 else synth.gt_poses(600 + b, 1, f)[0] for b, f in enumerate(frames)]
    enc = iter(vw.encode_clips([g for g in gp if g is not None]))
    given = [None if g is None else _np(next(enc)) for g in gp]
    kw = dict(mode=_lib.TS_SAMPLE_PHILOX, seed=9, clip_index0=3)
    want = w.generate_clips_from_wav(wavs, 16000, [0, 1, 2, 3], given=given, **kw)
    _same(w.generate_clips_from_wav(wavs, 16000, [0, 1, 2, 3], given_poses=gp, **kw), want, "from recordings, given_poses")
    _same(w.generate_clips_from_wav(wavs, 16000, [0, 1, 2, 3], given=[given[0], None, None, None], given_poses=[None, None, gp[2], gp[3]], **kw),
          want, "from recordings, both kinds")


def test_round_trip_through_decoded_poses(w, vw, clips):
    """Decode, hand back poses[:4 g]: the pass equals the `given=` pass on the RE-ENCODED codes (re-encoding decoded poses need not be the
    identity, so that is all that is asserted)."""
    rows, mf, ids, recs, motion = clips
    kw = _kw("philox", recs)
    D = w.generate_clips(mf, ids, **kw)
    g = [max(1, h // 2) for h in rows]
    gp = [_np(D[b][1])[:4 * g[b]] for b in range(len(rows))]
    re_codes = [_np(c) for c in vw.encode_clips(gp)]
    _same(w.generate_clips(mf, ids, logprobs=True, given_poses=gp, **kw), w.generate_clips(mf, ids, logprobs=True, given=re_codes, **kw), "round trip")


# ---- 3. scoring ---------------------------------------------------------------------------------------------------------------------------
def test_scoring_in_one_pass_equals_clip_by_clip(w, vw):
    rng = np.random.default_rng(33)
    rows = [int(h) for h in rng.integers(1, 21, 33)]
    lens = [4 * h + int(rng.integers(0, 4)) for h in rows]
    mf = [synth.mfcc_features(5000 + k, 1, t)[0] for k, t in enumerate(lens)]
    ids = (np.arange(33) % 4).astype(np.int64)
    motion = [synth.gt_poses(800 + k, 1, 4 * h)[0] for k, h in enumerate(rows)]
    codes = [_np(c) for c in vw.encode_clips(motion)]
    a = w.score_clips(mf, ids, codes)
    m = w.score_motion_clips(mf, ids, motion)
    for b in range(33):
        lp, sums = w.score_batch(mf[b][None], ids[b:b + 1], codes[b][None])
        for tag, r in (("score_clips", a[b]), ("score_motion_clips", m[b])):
            assert r[0].shape == (rows[b], 2) and r[1].shape == (3,)
            assert np.array_equal(bits(r[0]), bits(lp[0])), f"{tag}: log-probabilities of clip {b}"
            assert np.array_equal(_np(r[1]).view(np.uint64), _np(sums[0]).view(np.uint64)), f"{tag}: sums of clip {b}"
    with pytest.raises(ValueError, match="clip 2 has"):
        w.score_motion_clips(mf[:3], ids[:3], [motion[0], motion[1], motion[2][:-1]])
    with pytest.raises(ValueError, match="clip 1 must have shape"):
        w.score_clips(mf[:2], ids[:2], [codes[0], codes[1][:-1] if rows[1] > 1 else np.zeros((2, 2), np.int64)])


# ---- 4. against the reference's encode -----------------------------------------------------------------------------------------------
# The 32 clips of tests/golden/vq_encode_b32.npz (300 GT frames each, codebooks spread over the encoders' outputs), clip b truncated to
# PARITY_LENS[b % 8] frames: 544 nearest-neighbour decisions (272 per network) in one mixed pass.  The lengths were chosen on the CPU from the
# oracle's own float64 top-2 margins: smallest margin 1.85e-3 against bounds around 1.1e-3, 0 of 544 rows skipped.
PARITY_LENS = [4, 5, 7, 8, 30, 31, 77, 120]
Z_TOL = 2e-5            # the tolerance tests/test_gpu_parity.py::test_vqvae_golden pins z to, per component
SKIP_CAP = 0.01


def test_mixed_encode_against_the_reference():
    """Codes of the mixed pass == `oracle.torch_port.vq_encode_pair` (the reference's modules on the CPU) on every truncated clip ALONE, on
    every row whose decision a z error of Z_TOL cannot move.  d_j = |z - e_j|^2; an error dz with |dz_c| <= Z_TOL has |dz| <= sqrt(64) Z_TOL,
    and d_j moves by 2 (z - e_j).dz + |dz|^2, so |delta d| <= 2 sqrt(64) Z_TOL max_j |z - e_j| (the square term is 1e-8 of it).  A row is held
    to equality iff its float64 top-2 margin, from the oracle's z, exceeds that; at most 1 % of the rows may fall below."""
    from nets.init_model import init_model
    from oracle import talkshow_oracle as O
    from oracle import torch_port as TP
    from talkshow_amd.config import load_JsonConfig
    from talkshow_amd.modules import VQVAE
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "vq_encode_b32.npz")))
    seed, B, T = (int(v) for v in g["gt_seed"])
    sds = (synth.vqvae_state_dict(seed=7, in_dim=39, codebook=(g["mu_body"], g["sigma_body"])),
           synth.vqvae_state_dict(seed=7, in_dim=90, salt=1, codebook=(g["mu_hand"], g["sigma_hand"])))
    v = init_model("s2g_body_vq", argparse.Namespace(gpu=0, infer=True), load_JsonConfig(os.path.join(REPO, "config", "body_vq.json")))
    v.g_body, v.g_hand = VQVAE(39, 64, 2048, 1024, 2).cuda(), VQVAE(90, 64, 2048, 1024, 2).cuda()
    v.g_body.load_state_dict(synth.to_torch(sds[0]))
    v.g_hand.load_state_dict(synth.to_torch(sds[1]))
    poses = synth.gt_poses(seed, B, T)
    lens = [PARITY_LENS[b % len(PARITY_LENS)] for b in range(B)]
    clips = [poses[b, :lens[b]] for b in range(B)]
    got = [_np(c) for c in v.encode_clips(clips)]
    rows = skipped = wrong = 0
    smallest = np.inf
    for b in range(B):
        ref = TP.vq_encode_pair(clips[b][None], sds[0], sds[1])[0]                       # (H_b, 2), the clip alone
        assert got[b].shape == ref.shape == (lens[b] // 4, 2)
        for col, (sd, sl) in enumerate(zip(sds, (slice(0, 39), slice(39, 129)))):
            z = O.vq_encoder(np.ascontiguousarray(clips[b][None, :, sl].transpose(0, 2, 1)), sd)[0].T.astype(np.float64)      # (H_b, 64)
            d = ((z[:, None, :] - sd["vq_layer.embeddings"].astype(np.float64)[None]) ** 2).sum(-1)
            top2 = np.sort(d, 1)[:, :2]
            margin = top2[:, 1] - top2[:, 0]
            hold = margin > 2.0 * np.sqrt(64.0) * Z_TOL * np.sqrt(d.max(1))
            rows += len(margin)
            skipped += int((~hold).sum())
            smallest = min(smallest, float(margin.min()))
            wrong += int((got[b][hold, col] != ref[hold, col]).sum())
    print(f"\nmixed encode against the reference: {rows} rows, {skipped} below the margin bound, smallest margin {smallest:.3e}, {wrong} differ")
    assert skipped <= SKIP_CAP * rows, f"{skipped} of {rows} rows fall below the margin bound: more than 1 %"
    assert wrong == 0, f"{wrong} of {rows - skipped} decisions differ from the reference's VQVAE.encode on the clip alone"


# ---- 5. errors, before any launch -----------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(w, clips):
    from talkshow_amd import _lib
    rows, mf, ids, recs, motion = clips
    lib, ctx = _lib.load(), _lib.context(0)
    n = len(rows)

    def launches():
        import ctypes as C
        cnt = (C.c_int64 * 4)()
        _lib.check(lib.ts_prof_read_n(ctx, 4, None, cnt, None, 0))
        return list(cnt), w.generator.graph_captures()
    lib.ts_prof_enable(ctx, 1)
    try:
        before = launches()

        def bad(gp, match, given=None):
            with pytest.raises(ValueError, match=match):
                w.generate_clips(mf, ids, given_poses=gp, given=given, mode=_lib.TS_SAMPLE_GREEDY)
        for p in (1, 2, 3):
            bad([None] * 2 + [motion[2][:p]] + [None] * (n - 3), rf"clip 2 brings {p} given pose frames")
        bad([np.zeros((4 * rows[0] + 4, 129), F32)] + [None] * (n - 1), r"clip 0 brings .* code rows but has")
        bad([None, np.zeros((8, 128), F32)] + [None] * (n - 2), r"clip 1 must have shape \(P, 129\)")
        g = [None] * n
        g[3] = np.zeros((1, 2), np.int64)
        bad([None] * 3 + [motion[3][:4]] + [None] * (n - 4), r"clip 3 brings both", given=g)
        assert launches() == before, "a refused call launched something"
    finally:
        lib.ts_prof_enable(ctx, 0)
