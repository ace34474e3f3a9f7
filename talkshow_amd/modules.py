"""Module-shaped host objects over the C-ABI handles.

The reference's wrappers expose `nn.Module`s (`.generator`, `.g_body`, `.g_hand`, `.audioencoder`) on which callers
call `.eval()`, `.state_dict()`, `.load_state_dict()`, `.parameters()` and the model-specific entry points
(`VQVAE.encode/decode/__call__`, `GatedPixelCNN.generate`, `AudioEncoder.__call__`).  These classes keep that
surface — weights live in a CPU `OrderedDict` under the reference's key names — but every compute method goes to
libtalkshow_hip.so.  There is no torch implementation behind them.

Shape conventions of the methods follow the reference (channels-first tensors in, channels-first tensors out) so
that `nets/` reads like the reference wrappers; the transposes to the library's NLC layout happen here, on device.
"""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, synth


class NativeModule:
    """Weights in reference state_dict form + a lazily (re)built device handle."""

    _schema_cache = {}

    def __init__(self, schema_sd):
        self._sd = OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in schema_sd.items())
        self._handle = None
        self._device = torch.device("cpu")
        self.training = False

    # --- nn.Module-like surface -------------------------------------------------------------------
    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def load_state_dict(self, sd, strict=True):
        sd = OrderedDict((k.replace("module.", ""), v) for k, v in sd.items())
        missing = [k for k in self._sd if k not in sd]
        unexpected = [k for k in sd if k not in self._sd]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: "
                               f"missing keys {missing[:5]}{'...' if len(missing) > 5 else ''}, "
                               f"unexpected keys {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        for k, cur in self._sd.items():
            if k not in sd:
                continue
            v = sd[k]
            v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if tuple(v.shape) != tuple(cur.shape):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)}, "
                                   f"the shape in current model is {tuple(cur.shape)}")
            self._sd[k] = v.to(cur.dtype).contiguous().clone()
        self._after_load()
        self._release()
        return self

    def _after_load(self):
        pass

    _BUFFER_SUFFIXES = ("running_mean", "running_var", "num_batches_tracked", "vq_layer.embeddings", "ema_dw.hidden",
                        "ema_cluster_size.hidden")

    def parameters(self):
        # nn.Module.parameters() leaves buffers out (BatchNorm statistics, the EMA codebook of VectorQuantizerEMA)
        return (v for k, v in self._sd.items() if v.dtype == torch.float32 and not k.endswith(self._BUFFER_SUFFIXES))

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("talkshow_amd is an inference path; training is out of scope (DESIGN.md)")
        return self.eval()

    def to(self, device):
        self._device = torch.device(device)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else torch.cuda.current_device()))

    # --- native handle ---------------------------------------------------------------------------
    def _release(self):
        if self._handle is not None:
            self._destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _require_hip(self):
        if self._device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__}: device is '{self._device}' and torch.cuda.is_available() is "
                               f"{torch.cuda.is_available()}, but this implementation only runs on a HIP device "
                               "(torch device 'cuda:N' on ROCm, MI355X / gfx950). There is no CPU path.")
        return self._device.index if self._device.index is not None else torch.cuda.current_device()

    def _ctx(self):
        return _lib.context(self._require_hip())

    def handle(self):
        if self._handle is None:
            with torch.cuda.device(self._require_hip()):     # the caller's current device is left as it was
                self._handle = self._create(self._ctx())
        return self._handle

    def _dev(self):
        return torch.device("cuda", self._require_hip())


_range_seen = {}   # (id(owning tensor), view geometry, n) -> (weakref to the owner, _version): caller-owned device tensors already checked


def _check_index_range(x, n, what):
    """IndexError for indices outside [0, n) like nn.Embedding.  Host-origin indices (ints, lists, numpy, CPU tensors) are
    checked on the host before upload: no device sync.  A device tensor costs one device->host sync the first time this
    tensor OBJECT is seen at this version; the cache holds a weak reference to the object (never its address: tensors built
    inside a call get recycled addresses with _version 0, and a stale hit would skip the check)."""
    import weakref
    if isinstance(x, torch.Tensor) and x.is_cuda:
        owner = x._base if x._base is not None else x       # a view (ids[:n]) is a new object per call: key on the tensor it views
        key = (id(owner), x.storage_offset(), tuple(x.shape), tuple(x.stride()), n)
        ent = _range_seen.get(key)
        if ent is not None and ent[0]() is owner and ent[1] == x._version:
            return
        lo, hi = (int(x.min()), int(x.max())) if x.numel() else (0, 0)
        if lo >= 0 and hi < n:
            if len(_range_seen) > 256:
                _range_seen.clear()
            _range_seen[key] = (weakref.ref(owner), x._version)
    else:
        a = x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
    if lo < 0 or hi >= n:
        raise IndexError(f"{what} out of range: [{lo}, {hi}] not within [0, {n})")


def _index_tensor(x, n, what, device):
    """x (int / list / numpy / tensor anywhere) -> flat contiguous int64 tensor on `device`, range-checked (see above)."""
    _check_index_range(x, n, what)
    return torch.as_tensor(x, dtype=torch.int64, device=device).reshape(-1).contiguous()


def _dev_f32(x, device):
    return torch.as_tensor(x, dtype=torch.float32, device=device).contiguous()


class AudioEncoder(NativeModule):
    """`vqvae_1d.AudioEncoder(in_dim, num_hiddens, num_residual_layers, num_residual_hiddens)` (`vqvae_1d.py:11-34`)."""

    def __init__(self, in_dim, num_hiddens, num_residual_layers, num_residual_hiddens=None):
        self.in_dim, self.num_hiddens, self.nres = in_dim, num_hiddens, num_residual_layers
        super().__init__(synth.audioencoder_state_dict(0, in_dim, num_hiddens, num_residual_layers))

    def _create(self, ctx):
        arr, n, keep = _lib.pack_state_dict(self._sd)
        h = C.c_void_p()
        _lib.check(_lib.load().ts_audioenc_create(ctx, arr, n, self.in_dim, self.num_hiddens, self.nres, C.byref(h)))
        return h

    def _destroy(self, h):
        _lib.load().ts_convnet_destroy(h)

    def forward_nlc(self, mfcc):
        """mfcc (B,T,in_dim) device tensor -> (B,T//4,num_hiddens)."""
        mfcc = _dev_f32(mfcc, self._dev())
        B, T, _ = mfcc.shape
        if T < 4:
            raise RuntimeError(f"sequence too short: {T} frames (need >= 4 for one code row)")
        out = torch.empty((B, T // 2 // 2, self.num_hiddens), dtype=torch.float32, device=mfcc.device)
        _lib.check(_lib.load().ts_audioenc_forward(self.handle(), _lib.dptr(mfcc), B, T, _lib.dptr(out), _lib.stream_ptr()))
        return out

    def __call__(self, x, frame_num=0):
        """reference call shape: x (B,in_dim,T) -> (B,num_hiddens,T//4) (`vqvae_1d.py:27-34`)."""
        x = _dev_f32(x, self._dev())
        return self.forward_nlc(x.transpose(1, 2).contiguous()).transpose(1, 2)


class VQVAE(NativeModule):
    """`vqvae_1d.VQVAE(in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers, ·)` (`vqvae_1d.py:152-208`)."""

    def __init__(self, in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers, num_residual_hiddens=None,
                 commitment_cost=0.25, decay=0.99, share=False):
        self.in_dim, self.embedding_dim, self.num_embeddings = in_dim, embedding_dim, num_embeddings
        self.num_hiddens, self.nres = num_hiddens, num_residual_layers
        super().__init__(synth.vqvae_state_dict(0, in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers))

    def _create(self, ctx):
        arr, n, keep = _lib.pack_state_dict(self._sd)
        h = C.c_void_p()
        _lib.check(_lib.load().ts_vqvae_create(ctx, arr, n, self.in_dim, self.embedding_dim, self.num_embeddings,
                                               self.num_hiddens, self.nres, C.byref(h)))
        return h

    def _destroy(self, h):
        _lib.load().ts_vqvae_destroy(h)

    # --- NLC device entry points ---
    def encode_nlc(self, poses, want_z=False, want_quantized=True):
        poses = _dev_f32(poses, self._dev())
        B, T, _ = poses.shape
        if T < 4:
            raise RuntimeError(f"sequence too short: {T} frames (need >= 4 for one code row)")
        H = T // 2 // 2
        lat = torch.empty((B, H), dtype=torch.int64, device=poses.device)
        z = torch.empty((B, H, self.embedding_dim), dtype=torch.float32, device=poses.device) if want_z else None
        q = torch.empty((B, H, self.embedding_dim), dtype=torch.float32, device=poses.device) if want_quantized else None
        _lib.check(_lib.load().ts_vqvae_encode(self.handle(), _lib.dptr(poses), B, T, _lib.dptr(z), _lib.dptr(lat),
                                               _lib.dptr(q), _lib.stream_ptr()))
        return z, q, lat

    def decode_nlc(self, latents, out=None, col0=0):
        latents = torch.as_tensor(latents, dtype=torch.int64, device=self._dev()).contiguous()
        B, H = latents.shape
        if out is None:
            out = torch.empty((B, 4 * H, self.in_dim), dtype=torch.float32, device=latents.device)
        _lib.check(_lib.load().ts_vqvae_decode(self.handle(), _lib.dptr(latents), B, H, _lib.dptr(out), out.shape[-1], col0,
                                               _lib.stream_ptr()))
        return out

    def decode_z_nlc(self, z):
        """Decoder.forward on CONTINUOUS latents z (B,H,embedding_dim) -> (B,4H,in_dim) (`ts_vqvae_decode_z`)."""
        z = _dev_f32(z, self._dev())
        B, H, _ = z.shape
        out = torch.empty((B, 4 * H, self.in_dim), dtype=torch.float32, device=z.device)
        _lib.check(_lib.load().ts_vqvae_decode_z(self.handle(), _lib.dptr(z), B, H, _lib.dptr(out), self.in_dim, 0,
                                                 _lib.stream_ptr()))
        return out

    def forward_nlc(self, poses, out=None, col0=0):
        poses = _dev_f32(poses, self._dev())
        B, T, _ = poses.shape
        H = T // 2 // 2
        lat = torch.empty((B, H), dtype=torch.int64, device=poses.device)
        if out is None:
            out = torch.empty((B, 4 * H, self.in_dim), dtype=torch.float32, device=poses.device)
        _lib.check(_lib.load().ts_vqvae_forward(self.handle(), _lib.dptr(poses), B, T, _lib.dptr(lat), _lib.dptr(out),
                                                out.shape[-1], col0, _lib.stream_ptr()))
        return lat, out

    # --- reference call shapes ---
    def encode(self, gt_poses, id=None):
        """`VQVAE.encode` (`vqvae_1d.py:196-199`): gt_poses (B,T,in_dim) -> (e (B,emb,H), latents (B,H))."""
        _, q, lat = self.encode_nlc(gt_poses)
        return q.transpose(1, 2), lat

    def decode(self, b, w, e=None, latents=None, pre_state=None):
        """`VQVAE.decode` (`vqvae_1d.py:201-208`): returns the reference's tuple (recon (B,in_dim,4w), None)."""
        if e is not None:      # continuous latents (B, embedding_dim, w): Decoder.forward on them as they are (`vqvae_1d.py:202-203`)
            z = _dev_f32(e, self._dev()).transpose(1, 2).contiguous()
            return self.decode_z_nlc(z).transpose(1, 2), None
        return self.decode_nlc(latents.reshape(b, w)).transpose(1, 2), None

    def __call__(self, gt_poses, id=None, pre_state=None):
        """`VQVAE.forward`, eval branch (`vqvae_1d.py:184-189`): (e, x_recon (B,in_dim,T))."""
        _, q, lat = self.encode_nlc(gt_poses)
        return q.transpose(1, 2), self.decode_nlc(lat).transpose(1, 2)


class AE(VQVAE):
    """`vqvae_1d.AE(in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers, ·)` (`vqvae_1d.py:211-235`):
    Encoder + Decoder without a quantiser — the FGD feature extractor behind `nets.s2g_body_ae` (`body_ae.py:145-152`)."""

    def __init__(self, in_dim, embedding_dim, num_embeddings, num_hiddens, num_residual_layers, num_residual_hiddens=None):
        self.in_dim, self.embedding_dim, self.num_embeddings = in_dim, embedding_dim, 0
        self.num_hiddens, self.nres = num_hiddens, num_residual_layers
        NativeModule.__init__(self, synth.ae_state_dict(0, in_dim, embedding_dim, num_hiddens, num_residual_layers))

    def encode_nlc(self, poses):
        """poses (B,T,in_dim) -> z (B,T//4,embedding_dim), device tensor."""
        poses = _dev_f32(poses, self._dev())
        B, T, _ = poses.shape
        if T < 4:
            raise RuntimeError(f"sequence too short: {T} frames (need >= 4 for one latent row)")
        z = torch.empty((B, T // 2 // 2, self.embedding_dim), dtype=torch.float32, device=poses.device)
        _lib.check(_lib.load().ts_vqvae_encode(self.handle(), _lib.dptr(poses), B, T, _lib.dptr(z), None, None,
                                               _lib.stream_ptr()))
        return z

    # --- reference call shapes ---
    def encode(self, gt_poses, id=None):
        """`AE.encode` (`vqvae_1d.py:233-235`): gt_poses (B,T,in_dim) -> z (B,embedding_dim,T//4)."""
        return self.encode_nlc(gt_poses).transpose(1, 2)

    def decode(self, *a, **k):
        raise NotImplementedError("AE has no code-index decode; use __call__ (encode -> decode of continuous latents)")

    def __call__(self, gt_poses, id=None, pre_state=None):
        """`AE.forward`, eval branch (`vqvae_1d.py:225-229`): (z (B,emb,H), x_recon (B,in_dim,T)); Decoder ignores pre_state."""
        z = self.encode_nlc(gt_poses)
        return z.transpose(1, 2), self.decode_z_nlc(z).transpose(1, 2)


class GatedPixelCNN(NativeModule):
    """`gated_pixelcnn_v2.GatedPixelCNN(input_dim, dim, n_layers, n_classes, audio, bh_model)`.

    audio=True, bh_model=True (config/body_pixel.json) is the tuned incremental chain (`ts_pixelcnn_*`).  The other three
    constructor variants are supported as the reference supports them, untuned: audio=False with bh_model=True runs the same
    chain with an identity fusion and zero audio rows (bit-identical to having no fusion: 1.0 * x + 0 is exact); bh_model=False
    is the single vertical stack (`ts_pixelcnn_v_*`: columns never mix, grid width any power of two)."""

    def __init__(self, input_dim=256, dim=64, n_layers=15, n_classes=10, audio=False, bh_model=False, aud_dim=256):
        self.input_dim, self.dim, self.n_layers, self.n_classes, self.aud_dim = input_dim, dim, n_layers, n_classes, aud_dim
        self.audio, self.bh_model = bool(audio), bool(bh_model)
        super().__init__(synth.pixelcnn_state_dict(0, input_dim, dim, n_layers, n_classes, aud_dim, audio=self.audio,
                                                   bh_model=self.bh_model))

    def _after_load(self):
        # the reference zeroes these taps in place on every forward of layer 0 (make_causal, gated_pixelcnn_v2.py:57-63),
        # so its state_dict() returns them zeroed after the first call; mirror that.
        self._sd["layers.0.vert_stack.weight"][:, :, -1] = 0
        self._sd["layers.0.horiz_stack.weight"][:, :, :, -1] = 0

    def _create(self, ctx):
        h = C.c_void_p()
        if not self.bh_model:
            arr, n, keep = _lib.pack_state_dict(self._sd)
            _lib.check(_lib.load().ts_pixelcnn_v_create(ctx, arr, n, self.input_dim, self.dim, self.n_layers, self.n_classes,
                                                        int(self.audio), self.aud_dim, C.byref(h)))
            return h
        sd = self._sd
        if not self.audio:   # no audio branch: an identity fusion over zero audio rows is the same arithmetic, exactly
            D = self.dim
            eye = torch.cat([torch.eye(D), torch.zeros(D, D)], 1).reshape(D, 2 * D, 1, 1)
            sd = OrderedDict(sd)
            sd["embedding_aud.weight"], sd["embedding_aud.bias"] = torch.zeros(D, self.aud_dim, 1, 1), torch.zeros(D)
            sd["fusion_v.weight"], sd["fusion_v.bias"] = eye.clone(), torch.zeros(D)
            sd["fusion_h.weight"], sd["fusion_h.bias"] = eye.clone(), torch.zeros(D)
        arr, n, keep = _lib.pack_state_dict(sd)
        _lib.check(_lib.load().ts_pixelcnn_create(ctx, arr, n, self.input_dim, self.dim, self.n_layers, self.n_classes,
                                                  self.aud_dim, C.byref(h)))
        return h

    def _destroy(self, h):
        (_lib.load().ts_pixelcnn_destroy if self.bh_model else _lib.load().ts_pixelcnn_v_destroy)(h)

    def run(self, label, aud_rows, mode=_lib.TS_SAMPLE_PHILOX, codes=None, uniforms=None, seed=0, clip_index0=0,
            want_logits=False, pre_codes=None, pre_aud=None, shape=None, sampling=None, logprobs=False, given=None, given_keep=None,
            style=None, code_bias=None, repeat=None, guide=None, alternatives=None):
        """aud_rows (B,H,aud_dim) device (None for audio=False: pass shape=(B,H)); returns (codes (B,H,W) int64, logits
        (B,H,W,V) or None); W = 2 unless bh_model=False and shape=(B,H,W) says otherwise.  sampling: one sampling record
        (`_lib.sampling_record`: temperature, top_p, top_k) for all clips or one per clip (`ts_pixelcnn_generate_ctl`); the logits returned
        are the network's, before any control.  bh_model=False takes none.
        logprobs: True, or a float32 (B,H,2) device tensor to fill -> a THIRD return value, the log-probability of every code under the
        distribution it was drawn from (`ts_pixelcnn_generate_lp`; teacher forced: of the given codes under the model's); the decode
        stays on its graphs.  False (the default): two return values and the launches there always were.
        given: one (B,G,2) integer block, or a list of B entries (None or a (G_b,2) integer array): clip b's first G_b code rows are TAKEN
        from it and the rest produced as without it (`ts_pixelcnn_generate_mixed_given`, the mixed entry with equal lengths; aud_rows is the
        clip's whole audio).  The codes returned hold the given rows followed by the produced ones; with logprobs, a given row gets the
        log-probability of its code under the distribution it would have been drawn from (`sampling.given_logprob`).  A code outside
        [0, input_dim), a bad shape or G_b > H raises ValueError naming the clip before any device work.  Not with want_logits, pre_codes or
        TS_TEACHER_FORCED.  None (the default): no return value and no launch changes.
        given_keep: with `given`, WHICH of the given positions are taken (`_lib.given_keep_block`; talkshow_hip.h, "kept positions"): None
        (all: the behaviour without the keyword), "body" (column 0 kept, the hand column drawn), "hand" (column 1 kept, the body column
        drawn), a (G_b,2) bool / 0-1 array, one of these per clip in a list, or one (B,G,2) block.  An unkept position is produced as if
        nothing were given there — its given code is not read and may hold anything — and draws the number of its absolute (row, column), so
        handing back an earlier decode with any mask returns that decode.  Keeping hands while drawing the body is a forced decode, not a
        posterior sample (the body draw at row r sees hands of rows < r only).  ValueError naming the clip for a bad mask or a mask on a
        clip that brings nothing; `ts_pixelcnn_generate_mixed_keep`.
        style: float SPEAKER WEIGHTS in place of `label` (`_lib.style_block`; talkshow_hip.h, "speaker style"): a list with, per clip,
        None (the clip's label, that is, its one-hot row), an (n_classes,) row for the whole clip or an (H,n_classes) track with one row
        per code row; or one (n_classes,) or (B,n_classes) array for all clips.  The class-conditioning vector of a code row is the
        weighted sum of the classes' vectors (`sampling.style_rows`): a blend is an interpolation of the conditioning vectors, NOT a
        mixture of the classes' distributions; a one-hot row is the label bit for bit; weights are any finite floats.  Goes through the
        mixed entry with equal lengths (`ts_pixelcnn_generate_mixed_style`): not with want_logits, pre_codes or TS_TEACHER_FORCED.
        ValueError naming the clip for a wrong shape, a wrong n_classes or a non-finite weight, before any device work.  None (the
        default): no return value and no launch changes.
        code_bias: WHICH CODES a clip may use (`_lib.code_bias_block`; talkshow_hip.h, "code bias"): one (2, input_dim) float table for all
        clips, or a list with, per clip, None, a table or a {"body", "hand"} dict.  Row 0 is added to the logits of column 0 and row 1 to
        those of column 1 ahead of the sampling rule (`sampling.biased`); -inf bans a code.  TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only.
        Goes through the mixed entry with equal lengths (`ts_pixelcnn_generate_mixed_bias`): not with want_logits or pre_codes.
        ValueError naming the clip for a bad table, before any device work.  None (the default): no return value and no launch changes.
        repeat: a REPETITION PENALTY over a window of earlier codes (`_lib.repeat_table`; talkshow_hip.h, "repetition penalty"): one record
        (window, presence, frequency) or dict for all clips, or a list with one per clip.  A code the clip produced c > 0 times in the last
        `window` rows of the same column loses presence + frequency * c ahead of the sampling rule (`sampling.penalised`).
        TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only.  Goes through the mixed entry with equal lengths (`ts_pixelcnn_generate_mixed_repeat`):
        not with want_logits or pre_codes.  ValueError naming the clip for a bad record, before any device work.  None (the default): no
        return value and no launch changes.
        guide: GUIDANCE against a second conditioning (`_lib.guide_entries`; talkshow_hip.h, "guidance"): one dict for all clips or a list
        with, per clip, None or {"scale": s, "aud_rows": (H, aud_dim) array or None, "id": int or None, "style": row / track or None}; an
        absent audio, id or style is the clip's own.  The clip is decoded under its own conditioning p while a SHADOW slot behind it runs
        the same code history under the second conditioning q; at every position the logits become l' = l + scale * (l - l_q)
        (`sampling.guided`) ahead of every other control.  scale > 0 pushes away from q, -0.5 is the geometric mean of the two
        distributions, 0 the call without the keyword.  The shadows are dropped from what is returned.  TS_SAMPLE_UNIFORMS /
        TS_SAMPLE_PHILOX only.  Goes through the mixed entry with equal lengths (`ts_pixelcnn_generate_guided`): not with want_logits
        or pre_codes.  ValueError naming the clip for a wrong key, shape or scale, before any device work.  None (the default): no return
        value and no launch changes.
        alternatives: n in [0, 8] -> one more return value behind the log-probabilities (where those are asked for), a
        `sampling.Alternatives` (talkshow_hip.h, "alternatives"): codes int64 (B,H,2,n) and logprobs float32 (B,H,2,n) of the n likeliest
        allowed codes of every position, entropy float32 (B,H,2) and rank int64 (B,H,2) of the position's own code — drawn, given or kept —
        all under the distribution the filters are applied to (code bias, repetition penalty and temperature applied; top-k and top-p
        not), written by the sampler launch itself.  Codes and log-probabilities are those of the call without the keyword, bit for bit.
        TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only (ValueError: a greedy decode with alternatives is sampling=(1, 1, 1) under Philox); not
        with guide (NotImplementedError).  Goes through the mixed entry with equal lengths (`ts_pixelcnn_generate_alt`): not with
        want_logits or pre_codes.  None (the default): no return value and no launch changes."""
        guided = guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide))
        an = _lib.alt_request(alternatives, mode, "run", guide=guided)      # ValueError / NotImplementedError before any device work
        if an is not None:
            if not self.bh_model:
                raise NotImplementedError("alternatives exist for the bh_model=True chain (ts_pixelcnn_generate_alt), not for the single-stack form")
            if want_logits or pre_codes is not None:
                raise ValueError("run: alternatives go through the mixed entry, which takes no logits output and no pre_codes")
        if guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide)):      # a list of None only is no guidance
            if not self.bh_model:
                raise NotImplementedError("guidance exists for the bh_model=True chain (ts_pixelcnn_generate_guided), not for the single-stack form")
            if want_logits or pre_codes is not None:
                raise ValueError("run: guidance goes through the mixed entry, which takes no logits output and no pre_codes")
        if repeat is not None:
            if not self.bh_model:
                raise NotImplementedError("a repetition penalty exists for the bh_model=True chain (ts_pixelcnn_generate_mixed_repeat), not for the single-stack form")
            if want_logits or pre_codes is not None:
                raise ValueError("run: a repetition penalty goes through the mixed entry, which takes no logits output and no pre_codes")
        if code_bias is not None:
            if not self.bh_model:
                raise NotImplementedError("a code bias exists for the bh_model=True chain (ts_pixelcnn_generate_mixed_bias), not for the single-stack form")
            if want_logits or pre_codes is not None:
                raise ValueError("run: a code bias goes through the mixed entry, which takes no logits output and no pre_codes")
        if style is not None:
            if not self.bh_model:
                raise NotImplementedError("speaker style exists for the bh_model=True chain (ts_pixelcnn_generate_mixed_style), not for the single-stack form")
            if want_logits or pre_codes is not None or mode == _lib.TS_TEACHER_FORCED:
                raise ValueError("run: a speaker style goes through the mixed entry, which takes no logits output, no pre_codes and no teacher forcing")
        if given_keep is not None and not self.bh_model:
            raise NotImplementedError("kept positions exist for the bh_model=True chain (ts_pixelcnn_generate_mixed_keep), not for the single-stack form")
        if given is not None:
            if not self.bh_model:
                raise NotImplementedError("given rows exist for the bh_model=True chain (ts_pixelcnn_generate_mixed_given), not for the single-stack form")
            if want_logits or pre_codes is not None or mode == _lib.TS_TEACHER_FORCED:
                raise ValueError("run: given rows go through the mixed entry, which takes no logits output, no pre_codes and no teacher forcing")
        if sampling is not None and not self.bh_model:
            raise NotImplementedError("sampling controls exist for the bh_model=True chain (ts_pixelcnn_generate_ctl), not for the single-stack form")
        if logprobs is not None and logprobs is not False and not self.bh_model:
            raise NotImplementedError("log-probabilities exist for the bh_model=True chain (ts_pixelcnn_generate_lp), not for the single-stack form")
        dev = self._dev()
        W = 2
        if aud_rows is not None:
            aud_rows = _dev_f32(aud_rows, dev)
            B, H, _ = aud_rows.shape
            if shape is not None and len(shape) == 3:
                W = int(shape[2])
        else:
            if self.audio:
                raise ValueError("this network was built with audio=True: aud_rows is required")
            B, H = int(shape[0]), int(shape[1])
            W = int(shape[2]) if len(shape) == 3 else 2
        if self.bh_model and W != 2:
            raise NotImplementedError("bh_model grids have exactly 2 columns (body, hand)")
        lp = _lib.logprob_request(logprobs, (B, H, 2), dev)   # a wrong output tensor: ValueError before any device work
        ctl, n_ctl = None, 0
        if sampling is not None:   # validated (ValueError names the clip) before any device work
            ctl, n_ctl = _lib.sampling_table(sampling, B, self.input_dim, mode)
        btab, bidx = _lib.code_bias_block(code_bias, B, self.input_dim, who="run", mode=mode)   # ValueError before any device work
        rtab, n_rep = _lib.repeat_table(repeat, B, self.input_dim, who="run", mode=mode)       # too
        gent = _lib.guide_entries(guide, B, who="run", audio_key="aud_rows", mode=mode, n_classes=self.n_classes, rows=[H] * B)   # and the guide entries
        for b, e in enumerate(gent or ()):
            if e is not None and e["audio"] is not None:
                if aud_rows is None or tuple(np.shape(e["audio"])) != (H, aud_rows.shape[2]):
                    raise ValueError(f"run: guide of clip {b}: aud_rows must have the clip's own shape ({H}, {self.aud_dim}), got {tuple(np.shape(e['audio']))}")
        kblock = None
        if given_keep is not None:   # ValueError before any device work, too (without given rows there is nothing to select from)
            kblock = _lib.given_keep_block(given_keep, _lib.given_counts(given, None, B), [H] * B, who="run")
        if given is not None:
            block, table = _lib.given_block(given, [H] * B, self.input_dim, who="run", keep=kblock)   # ValueError before any device work
        if self.bh_model and aud_rows is None:
            aud_rows = torch.zeros((B, H, self.aud_dim), dtype=torch.float32, device=dev)
        label = _index_tensor(label, self.n_classes, "class label", dev)
        if label.numel() == 1 and B > 1:
            label = label.repeat(B)
        if label.numel() != B:
            raise ValueError(f"label must hold 1 or B={B} class indices, got {label.numel()}")
        sblock = _lib.style_block(style, [H] * B, self.n_classes, who="run", ids=label)   # ValueError before any device work
        if gent is not None:      # the slots of the guided pass: every shadow directly behind its primary
            src, shadow, gtab, gscale = _lib.guide_layout(range(B), gent)
            need_ids = sblock is None and any(e is not None and e["style"] is not None for e in gent)
            sblock = _lib.guide_style_block(sblock, src, shadow, gent, [H] * B, self.n_classes, label.cpu().numpy() if need_ids else None, who="run")
        if mode == _lib.TS_TEACHER_FORCED:
            codes = torch.as_tensor(codes, dtype=torch.int64, device=dev).contiguous()
            if lp is not None:
                _lib.score_codes_shape(codes.shape, B, H)
        else:
            codes = torch.zeros((B, H, W), dtype=torch.int64, device=dev)
        logits = torch.empty((B, H, W, self.input_dim), dtype=torch.float32, device=dev) if want_logits else None
        if uniforms is not None:
            uniforms = _dev_f32(uniforms, dev)
        H0 = 0
        if pre_codes is not None:
            pre_codes = torch.as_tensor(pre_codes, dtype=torch.int64, device=dev).contiguous()
            H0 = pre_codes.shape[1]
            if pre_aud is not None:
                pre_aud = _dev_f32(pre_aud, dev)
            elif self.bh_model:
                pre_aud = torch.zeros((B, H0, self.aud_dim), dtype=torch.float32, device=dev)
        if not self.bh_model:
            _lib.check(_lib.load().ts_pixelcnn_v_generate(
                self.handle(), _lib.dptr(label), _lib.dptr(aud_rows), B, H, W, mode, _lib.dptr(uniforms), int(seed) & (2 ** 64 - 1),
                int(clip_index0), _lib.dptr(codes), _lib.dptr(logits), _lib.dptr(pre_codes), _lib.dptr(pre_aud), H0, _lib.stream_ptr()))
            return codes, logits
        if gent is not None:
            return self._run_guided(label, aud_rows, mode, uniforms, seed, clip_index0, lp, ctl, n_ctl, block if given is not None else None,
                                    table if given is not None else None, kblock if given is not None else None, sblock, btab, bidx, rtab,
                                    n_rep, gent, src, shadow, gtab, gscale)
        if given is not None or sblock is not None or btab is not None or rtab is not None or an is not None:   # the mixed entry with equal lengths; clip b keeps Philox subsequence clip_index0 + b
            i32p = C.POINTER(C.c_int32)
            lens = np.full(B, 4 * H, np.int32)
            lens_dev = upload(lens, dev)
            clip_index = upload(np.arange(B, dtype=np.int64) + int(clip_index0), dev)
            if isinstance(lp, str):
                lp = torch.empty((B, H, 2), dtype=torch.float32, device=dev)
            areq = None if an is None else _lib.AltRequest(an, (B, H, 2), dev)
            lp_dev = lp if lp is not None or areq is None else torch.empty((B, H, 2), dtype=torch.float32, device=dev)   # the record needs one beside it
            fixed = (self.handle(), _lib.dptr(label), _lib.dptr(aud_rows), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H, mode,
                     _lib.dptr(uniforms), int(seed) & (2 ** 64 - 1), _lib.dptr(clip_index), _lib.dptr(codes))
            block_dev = upload(block, dev) if given is not None else None
            keep_dev = upload(kblock, dev) if kblock is not None and given is not None else None
            style_dev = upload(sblock, dev) if sblock is not None else None
            bias_dev = upload(btab, dev) if btab is not None else None
            _lib.pixelcnn_mixed_call(
                fixed, ctl=ctl, n_ctl=n_ctl, logprob=_lib.dptr(lp_dev), given=_lib.dptr(block_dev), given_rows=table.ctypes.data_as(i32p) if given is not None else None,
                keep=_lib.dptr(keep_dev), style=_lib.dptr(style_dev), style_rows=int(sblock.shape[1]) if sblock is not None else 0,
                bias=_lib.dptr(bias_dev), n_bias=int(btab.shape[0]) if btab is not None else 0, bias_index=bidx.ctypes.data_as(i32p) if btab is not None else None,
                rep=rtab, n_rep=n_rep, alt=None if areq is None else areq.ptr())
            out = (codes, None) if lp is None else (codes, None, lp)
            return out if areq is None else out + (areq.result(),)
        args = (self.handle(), _lib.dptr(label), _lib.dptr(aud_rows), B, H, mode, _lib.dptr(uniforms), int(seed) & (2 ** 64 - 1),
                int(clip_index0), _lib.dptr(codes), _lib.dptr(logits), _lib.dptr(pre_codes), _lib.dptr(pre_aud), H0)
        if lp is not None:
            if isinstance(lp, str):
                lp = torch.empty((B, H, 2), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().ts_pixelcnn_generate_lp(*args, ctl, n_ctl, _lib.dptr(lp), _lib.stream_ptr()))
            return codes, logits, lp
        if sampling is None:
            _lib.check(_lib.load().ts_pixelcnn_generate(*args, _lib.stream_ptr()))
        else:
            _lib.check(_lib.load().ts_pixelcnn_generate_ctl(*args, ctl, n_ctl, _lib.stream_ptr()))
        return codes, logits

    def _run_guided(self, label, aud_rows, mode, uniforms, seed, clip_index0, lp, ctl, n_ctl, block, table, kblock, sblock, btab, bidx, rtab,
                    n_rep, gent, src, shadow, gtab, gscale):
        """The guided branch of `run`: every validated per-clip block (slot order = submission order here) is re-indexed to the slots of
        the guided pass (`_lib.guide_layout`: slot s copies original slot src[s]; a shadow then takes its own audio and id, brings no
        given rows and no table), one call of `ts_pixelcnn_generate_guided`, and the primaries' rows are returned."""
        dev = aud_rows.device
        B, H, _ = aud_rows.shape
        i32p = C.POINTER(C.c_int32)
        Bx = len(src)
        sidx = np.asarray(src, np.int64)
        shadows = np.asarray(shadow, bool)
        sdev = upload(sidx, dev)
        aud_x = aud_rows.index_select(0, sdev).contiguous()
        label_x = label.index_select(0, sdev).contiguous()
        for s in np.flatnonzero(shadows):
            e = gent[src[s]]
            if e["audio"] is not None:
                aud_x[s] = _dev_f32(e["audio"], dev)
            if e["id"] is not None:
                label_x[s] = e["id"]
        lens = np.full(Bx, 4 * H, np.int32)
        lens_dev = upload(lens, dev)
        clip_index = upload(sidx + int(clip_index0), dev)      # a primary keeps Philox subsequence clip_index0 + b; shadows draw nothing
        u_x = None if uniforms is None else uniforms.index_select(0, sdev).contiguous()
        codes = torch.zeros((Bx, H, 2), dtype=torch.int64, device=dev)
        lp_x = None if lp is None else torch.empty((Bx, H, 2), dtype=torch.float32, device=dev)
        ctl, n_ctl = _lib.expand_records(ctl, n_ctl, src)
        rtab, n_rep = _lib.expand_records(rtab, n_rep, src)
        if block is not None:
            block, table = block[sidx], np.where(shadows, 0, table[sidx]).astype(np.int32)
            kblock = None if kblock is None else kblock[sidx]
        if btab is not None:
            bidx = np.where(shadows, -1, bidx[sidx]).astype(np.int32)
        fixed = (self.handle(), _lib.dptr(label_x), _lib.dptr(aud_x), lens.ctypes.data_as(i32p), _lib.dptr(lens_dev), Bx, H, mode,
                 _lib.dptr(u_x), int(seed) & (2 ** 64 - 1), _lib.dptr(clip_index), _lib.dptr(codes))
        block_dev = upload(block, dev) if block is not None else None
        keep_dev = upload(kblock, dev) if kblock is not None else None
        style_dev = upload(sblock, dev) if sblock is not None else None
        bias_dev = upload(btab, dev) if btab is not None else None
        _lib.pixelcnn_mixed_call(
            fixed, ctl=ctl, n_ctl=n_ctl, logprob=_lib.dptr(lp_x), given=_lib.dptr(block_dev), given_rows=table.ctypes.data_as(i32p) if block is not None else None,
            keep=_lib.dptr(keep_dev), style=_lib.dptr(style_dev), style_rows=int(sblock.shape[1]) if sblock is not None else 0,
            bias=_lib.dptr(bias_dev), n_bias=int(btab.shape[0]) if btab is not None else 0, bias_index=bidx.ctypes.data_as(i32p) if btab is not None else None,
            rep=rtab, n_rep=n_rep, guide=gtab.ctypes.data_as(i32p), guide_scale=_lib.fptr(gscale))
        prim = upload(np.flatnonzero(~shadows).astype(np.int64), dev)
        codes = codes.index_select(0, prim)
        if lp is None:
            return codes, None
        if isinstance(lp, str):
            return codes, None, lp_x.index_select(0, prim)
        lp.copy_(lp_x.index_select(0, prim))
        return codes, None, lp

    def score(self, label, aud_rows, codes, logprobs=True):
        """Teacher-forced scoring: the log-probability of every GIVEN code under the model, label / aud_rows (B,H,aud_dim) as for `run`,
        codes (B,H,2) int64 -> (logprobs (B,H,2) float32, sums (B,3) float64 = per clip {body column, hand column, both}:
        `ts_logprob_sums`, fixed-order fp64).  No logits leave the sampler launch; a code outside [0, input_dim) gives NaN at its position.
        Scoring the codes of a decode without a sampling table returns that decode's own log-probabilities, bit for bit."""
        if not self.bh_model:
            raise NotImplementedError("log-probabilities exist for the bh_model=True chain (ts_pixelcnn_generate_lp), not for the single-stack form")
        B, H = int(aud_rows.shape[0]), int(aud_rows.shape[1])
        _lib.score_codes_shape(tuple(getattr(codes, "shape", ())), B, H)
        _, _, lp = self.run(label, aud_rows, mode=_lib.TS_TEACHER_FORCED, codes=codes, logprobs=logprobs)
        return lp, self.logprob_sums(lp)

    def logprob_sums(self, lp, rows=None):
        """(B,H,2) log-probabilities -> (B,3) float64 per-clip sums {body, hand, both} (`ts_logprob_sums`; `sampling.logprob_sums` is its
        numpy restatement, equal bit for bit).  rows: (B,) every clip's own row count (None: H); rows beyond do not enter."""
        dev = self._dev()
        lp = _dev_f32(lp, dev)
        B, H = int(lp.shape[0]), int(lp.shape[1])
        lens = None
        if rows is not None:
            lens = upload(np.asarray(rows, np.int32) * 4, dev)           # the entry takes the mixed pass's table: MFCC frames, 4 per code row
        sums = torch.empty((B, 3), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().ts_logprob_sums(self._ctx(), _lib.dptr(lp), _lib.dptr(lens), B, H, _lib.dptr(sums), _lib.stream_ptr()))
        return sums

    def prepare(self, batch_size, rows, mode=_lib.TS_SAMPLE_GREEDY):
        """Serving aid (`ts_pixelcnn_prepare`): capture and pin the whole-call hipGraph of a (batch_size, rows, mode) decode on the current
        stream now, so that the first real call of that shape is already one replay.  Without it a shape runs on chunk graphs until its
        third sighting among the stream's last 16 calls.  No-op for the untuned bh_model=False form."""
        if self.bh_model:
            _lib.check(_lib.load().ts_pixelcnn_prepare(self.handle(), int(batch_size), int(rows), int(mode), _lib.stream_ptr()))
        return self

    def graph_captures(self):
        """hipGraphs captured so far on the current stream (a serving loop checks that this stands still once it is warm)."""
        return int(_lib.load().ts_pixelcnn_graph_captures(self.handle(), _lib.stream_ptr())) if self.bh_model else 0

    def open_stream(self, label, batch_size, max_chunk_rows, *, sampling=None, style=None, code_bias=None, repeat=None, pairs=None,
                    alternatives=None):
        """A generation session with a persistent row cache (`ts_pixelcnn_stream_*`): `.step(aud_rows)` continues the
        clip(s) where the previous step stopped, at a cost independent of the history length.  sampling / style / code_bias / repeat:
        session DEFAULTS in the forms `PixelCNNStream.step` takes; a step that passes no value for a keyword runs under the default, any
        value it does pass takes its place for that step.  pairs: GUIDANCE at slot level (talkshow_hip.h, "session pairs"):
        {primary: shadow} (stored scale 1) or {primary: (shadow, scale)} — slot `shadow` runs the primary's code history under its own label
        and audio rows and draws nothing; the primary is decoded as `run(..., guide=)` decodes it (`PixelCNNStream.step`).  alternatives: the
        session default of `step(alternatives=)`; not with pairs."""
        if not (self.audio and self.bh_model):
            raise NotImplementedError("streaming sessions exist for the shipped configuration (audio=True, bh_model=True)")
        return PixelCNNStream(self, label, batch_size, max_chunk_rows, sampling=sampling, style=style, code_bias=code_bias, repeat=repeat,
                              pairs=pairs, alternatives=alternatives)

    @staticmethod
    def _audio_rows(aud):
        """(B, aud_dim, H, W) audio map of the reference call shape -> the (B, H, aud_dim) rows the C entry takes (ONE audio row per
        code row).  The reference convolves the whole map; its only caller builds it by repeating one row over the columns
        (`smplx_body_pixel.py:274`), and that is the case implemented: a map whose columns differ is refused, not silently
        truncated to its first column."""
        if aud is None:
            return None
        # an expanded view (stride 0 over the columns: `unsqueeze(-1).expand`) or a single column cannot differ: no device work.  A
        # materialised map (`.repeat(1, 1, 1, 2)`, the reference caller's form) costs one device compare + a host read per call on
        # this reference-call-shape path (`generate_batch`, the serving entry, takes rows and never comes here); a host that has
        # validated its maps switches it off with TS_AUDIO_MAP_CHECK=0.  NaNs are reported as NaNs, not as differing columns.
        if aud.shape[-1] > 1 and aud.stride(-1) != 0 and os.environ.get("TS_AUDIO_MAP_CHECK", "1") != "0":
            same = (aud == aud[..., :1]) | (aud != aud)
            if not bool(same.all()):
                raise NotImplementedError("GatedPixelCNN: the audio map's columns differ; one audio row per code row is supported "
                                          "(the reference's caller repeats a row over the columns, smplx_body_pixel.py:274)")
        return aud[..., 0].transpose(1, 2)

    # --- reference call shapes ---
    def generate(self, label, shape=(8, 8), batch_size=64, aud_feat=None, pre_latents=None, pre_audio=None,
                 mode=None, seed=None, uniforms=None, sampling=None, logprobs=False, alternatives=None):
        """`GatedPixelCNN.generate` (`gated_pixelcnn_v2.py:152-177`): aud_feat (B,aud_dim,H,2) -> codes (B,H,2).

        Default is stochastic like the reference (softmax + one multinomial draw per position), with Philox uniforms
        seeded from torch's default generator; `mode=TS_SAMPLE_GREEDY` gives the argmax harness.  `sampling`: as for `run`.
        `logprobs=True` (or an output tensor): returns (codes, logprobs (B,H,2) float32) instead of codes.
        `alternatives=n`: as for `run`; a `sampling.Alternatives` is appended to what is returned.
        """
        rows = self._audio_rows(aud_feat)
        pre_rows = self._audio_rows(pre_audio)
        if mode is None:
            mode = _lib.TS_SAMPLE_PHILOX if uniforms is None else _lib.TS_SAMPLE_UNIFORMS
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if mode == _lib.TS_SAMPLE_PHILOX else 0
        out = self.run(label, rows, mode=mode, uniforms=uniforms, seed=seed, pre_codes=pre_latents, pre_aud=pre_rows,
                       shape=(batch_size, shape[0], shape[1]), sampling=sampling, logprobs=logprobs, alternatives=alternatives)
        if alternatives is not None:
            return (out[0],) + tuple(out[2:])
        return out[0] if len(out) == 2 else (out[0], out[2])

    def __call__(self, x, label, aud=None):
        """`GatedPixelCNN.forward` (`gated_pixelcnn_v2.py:130-150`): x (B,H,2) codes -> logits (B,input_dim,H,2)."""
        rows = self._audio_rows(aud)
        _, logits = self.run(label, rows, mode=_lib.TS_TEACHER_FORCED, codes=x, want_logits=True, shape=tuple(x.shape))
        return logits.permute(0, 3, 1, 2)


def step_style_rows(net, B, labels, style):
    """`style=` of a session step -> (B, n_classes) float32 numpy, one weight row per clip: the forms of `_lib.style_block` without tracks.
    labels: the session's (B,) class labels, what `style=[None, ...]` stands for."""
    if isinstance(style, (list, tuple)):
        for i, e in enumerate(style):
            if e is not None and np.ndim(e.detach().cpu().numpy() if hasattr(e, "detach") else e) >= 2:
                raise ValueError(f"step: style of clip {i} is a track of rows; a session takes ONE weight row per clip for a step "
                                 f"(it holds until a later step brings another)")
    return np.ascontiguousarray(_lib.style_block(style, [1] * B, net.n_classes, who="step", ids=labels)[:, 0])


def step_pieces(net, B, labels, defaults, Hc, mode, dev, sampling, logprobs, given, style, code_bias, repeat):
    """The keywords of one session step of Hc rows as the host-side pieces of the C call (`PixelCNNStream.step`, and the seamless body
    session's push): the session's `defaults` stand in for a keyword left at None, then every value is validated (ValueError naming the
    clip).  Pure host code: nothing is launched or uploaded."""
    sampling = defaults["sampling"] if sampling is None else sampling
    style = defaults["style"] if style is None else style
    code_bias = defaults["code_bias"] if code_bias is None else code_bias
    repeat = defaults["repeat"] if repeat is None else repeat
    V = net.input_dim
    lp = _lib.logprob_request(logprobs, (B, Hc, 2), dev)
    ctl, n_ctl = (None, 0) if sampling is None else _lib.sampling_table(sampling, B, V, mode)
    btab, bidx = _lib.code_bias_block(code_bias, B, V, who="step", mode=mode)
    rtab, n_rep = _lib.repeat_table(repeat, B, V, who="step", mode=mode)
    block = table = None
    if given is not None:
        block, table = _lib.given_block(given, [Hc] * B, V, who="step")
    srows = None if style is None else step_style_rows(net, B, labels, style)
    return lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows


class PixelCNNStream:
    """Host handle of `ts_pixelcnn_stream`: label (B,) or (1,) int64 fixed for the session."""

    def __init__(self, net, label, batch_size, max_chunk_rows, sampling=None, style=None, code_bias=None, repeat=None, pairs=None,
                 alternatives=None):
        from talkshow_amd.streaming import SlotPairs
        from talkshow_amd import sampling as _sampling
        if alternatives is not None:
            _sampling.alt_count(alternatives)      # ValueError before the session exists
            if pairs:
                raise NotImplementedError("open_stream: alternatives are not offered on a session with pairs")
        dev = net._dev()
        label = _index_tensor(label, net.n_classes, "class label", dev)
        if label.numel() == 1 and batch_size > 1:
            label = label.repeat(batch_size)
        if label.numel() != batch_size:
            raise ValueError(f"label must hold 1 or B={batch_size} class indices, got {label.numel()}")
        self.net, self.B, self.max_rows = net, int(batch_size), int(max_chunk_rows)
        self.defaults = {"sampling": sampling, "style": style, "code_bias": code_bias, "repeat": repeat, "alternatives": alternatives}
        self._labels = label.detach().cpu().numpy()      # what `style=[None, ...]` stands for: the clip's own label
        self._pairs = SlotPairs(self.B)
        declared = None
        if pairs:                                          # validated before the session exists (ValueError naming the slot)
            declared = SlotPairs.parse(pairs)
            self._pairs.pair(0, [0] * self.B, *declared)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ts_pixelcnn_stream_open(net.handle(), _lib.dptr(label), self.B, self.max_rows, C.byref(h)))
        self._h = h
        if declared:
            self._declare(*declared)

    def _pair_table(self, make=True):
        """This handle's `SlotPairs`.  `__init__` makes it; a handle put together without `__init__` (the host tests build one around a
        spy library) gets it on first use.  make=False: None while there is none."""
        if self.__dict__.get("_pairs") is None and make:
            from talkshow_amd.streaming import SlotPairs
            self._pairs = SlotPairs(self.B)
        return self.__dict__.get("_pairs")

    def _declare(self, primary, shadow, scale):
        """`ts_pixelcnn_stream_pair` on pairs the host rule (`streaming.SlotPairs`) has accepted: host tables, nothing is launched."""
        n = len(primary)
        _lib.check_value(_lib.load().ts_pixelcnn_stream_pair(self._h, (C.c_int32 * n)(*[int(b) for b in primary]),
                                                             (C.c_int32 * n)(*[int(g) for g in shadow]),
                                                             (C.c_float * n)(*[float(v) for v in scale]), n))

    @property
    def pairs(self):
        """{primary: (shadow, stored scale)} as the library holds them (`ts_pixelcnn_stream_pairs`; the scales are this handle's copy)."""
        tab = (C.c_int32 * self.B)()
        _lib.load().ts_pixelcnn_stream_pairs(self._h, tab)
        if list(tab) != self._pair_table().guide:
            raise RuntimeError(f"session pairs: the library holds {list(tab)}, this handle {self._pair_table().guide}")
        return self._pair_table().pairs

    @property
    def rows(self):
        return int(_lib.load().ts_pixelcnn_stream_rows(self._h))

    def graph_captures(self):
        """hipGraphs this session has captured so far (`ts_pixelcnn_stream_captures`): stands still once every (Hc, buffer phase, kind of
        sampler) the host steps with has been met — the records, tables, given codes and style of a step are in no graph key."""
        return int(_lib.load().ts_pixelcnn_stream_captures(self._h))

    def _style_rows(self, style):
        """`step_style_rows` on this session's network and labels."""
        return step_style_rows(self.net, self.B, self._labels, style)

    def _pieces(self, Hc, mode, dev, sampling, logprobs, given, style, code_bias, repeat):
        """`step_pieces` on this session's network, labels and defaults."""
        return step_pieces(self.net, self.B, self._labels, self.defaults, Hc, mode, dev, sampling, logprobs, given, style, code_bias, repeat)

    def step(self, aud_rows, mode=_lib.TS_SAMPLE_PHILOX, uniforms=None, seed=0, clip_index0=0, *, sampling=None, logprobs=False, given=None,
             style=None, code_bias=None, repeat=None, guide=None, alternatives=None):
        """aud_rows (B,Hc,aud_dim) device -> codes (B,Hc,2) int64 of the next Hc code rows.
        The keywords take the forms `GatedPixelCNN.run` takes and follow its rules FOR THIS STEP (`ts_pixelcnn_stream_step_ctl`;
        talkshow_hip.h, "streaming sessions"); sampling / style / code_bias / repeat left at None run under the session's default
        (`open_stream`).  sampling: one record or one per clip.  logprobs: True or a float32 (B,Hc,2) tensor -> returns (codes, logprobs).
        given: a list with None or a (g_b,2) array per clip, or one (B,g,2) block: clip b's first g_b rows OF THIS STEP are taken from it.
        style: one weight row per clip (no tracks); the rows stay in force until a later step brings others.  code_bias: tables for this
        step.  repeat: records over the session's own history, which persists across steps; a clip whose penalty is switched on (after no
        record, or window 0) starts from an empty history at this step's first row.  A bad value raises ValueError naming the clip before
        any device work; the session's row counter does not move.  With every keyword at its default and no session default the call is
        `ts_pixelcnn_stream_step`, exactly.
        guide: the scales of the session's PAIRS for this step (`ts_pixelcnn_stream_step_guided`; talkshow_hip.h, "session pairs"): None
        (the stored scales), a float for all pairs, a {primary: scale} dict, or an (S,) list with None at non-primaries.  A scale for a
        slot that is no primary, a NaN, an infinity or |scale| > 1e4 raises ValueError naming the slot.  A session with pairs runs every
        step under them: a primary's codes and log-probabilities are those of `run(..., guide=)` on the pair alone, a shadow's rows of
        what is returned are its primary's, and a shadow's entries of sampling / given / code_bias / repeat are never read.  Greedy mode
        is refused with pairs (`top_k = 1` is the greedy guided decode).  A session without pairs takes no `guide` and runs as ever.
        alternatives: n in [0, 8] (None: the session's default, `open_stream(alternatives=)`) -> a `sampling.Alternatives` over this step's
        (B,Hc,2) positions is appended to what is returned, as for `run` (`ts_pixelcnn_stream_step_alt`; talkshow_hip.h, "alternatives").
        Drawing modes only (ValueError); not on a session with pairs (NotImplementedError)."""
        B, Hc = int(aud_rows.shape[0]), int(aud_rows.shape[1])
        if B != self.B:
            raise ValueError(f"session was opened for B={self.B}, got {B}")
        dev = self.net._dev()
        if alternatives is None:
            alternatives = self.defaults.get("alternatives")
        ptab = self._pair_table(make=False)
        an = _lib.alt_request(alternatives, mode, "step", guide=guide is not None or (ptab is not None and any(g >= 0 for g in ptab.guide)))
        scales = None if guide is None else self._pair_table().step_scales(guide)      # None: the library runs the stored scales
        lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows = self._pieces(Hc, mode, dev, sampling, logprobs, given, style, code_bias,
                                                                                   repeat)
        if uniforms is not None and tuple(uniforms.shape) != (B, Hc, 2):   # the library strides them by the chunk's Hc * 2: a wrong shape would misalign clips b > 0
            raise ValueError(f"step(): uniforms must have shape (B={B}, Hc={Hc}, 2), got {tuple(uniforms.shape)}")
        aud_rows = _dev_f32(aud_rows, dev)
        codes = torch.empty((B, Hc, 2), dtype=torch.int64, device=dev)
        if uniforms is not None:
            uniforms = _dev_f32(uniforms, dev)
        args = (self._h, _lib.dptr(aud_rows), Hc, mode, _lib.dptr(uniforms), int(seed) & (2 ** 64 - 1), int(clip_index0), _lib.dptr(codes))
        if lp is None and ctl is None and btab is None and rtab is None and block is None and srows is None and scales is None and an is None:
            _lib.check(_lib.load().ts_pixelcnn_stream_step(*args, _lib.stream_ptr()))
            return codes
        if isinstance(lp, str):
            lp = torch.empty((B, Hc, 2), dtype=torch.float32, device=dev)
        i32p = C.POINTER(C.c_int32)
        block_dev = upload(block, dev) if block is not None else None
        style_dev = upload(srows, dev) if srows is not None else None
        bias_dev = upload(btab, dev) if btab is not None else None
        areq = None if an is None else _lib.AltRequest(an, (B, Hc, 2), dev)
        lp_dev = lp if lp is not None or areq is None else torch.empty((B, Hc, 2), dtype=torch.float32, device=dev)   # the record needs one beside it
        pieces = (ctl, n_ctl, _lib.dptr(lp_dev), _lib.dptr(block_dev), table.ctypes.data_as(i32p) if block is not None else None,
                  _lib.dptr(style_dev), _lib.dptr(bias_dev), int(btab.shape[0]) if btab is not None else 0,
                  bidx.ctypes.data_as(i32p) if btab is not None else None, rtab, n_rep)
        if areq is not None:      # the entry with the record is named only when the keyword is given
            _lib.check(_lib.load().ts_pixelcnn_stream_step_alt(*args, *pieces, areq.ptr(), _lib.stream_ptr()))
            return (codes, areq.result()) if lp is None else (codes, lp, areq.result())
        if scales is None:
            _lib.check(_lib.load().ts_pixelcnn_stream_step_ctl(*args, *pieces, _lib.stream_ptr()))
        else:
            _lib.check(_lib.load().ts_pixelcnn_stream_step_guided(*args, *pieces, (C.c_float * B)(*scales), _lib.stream_ptr()))
        return codes if lp is None else (codes, lp)

    @property
    def slot_rows(self):
        """(B,) int64 numpy: the code rows of every slot's CURRENT clip (`rows` for a slot that has never restarted)."""
        lib = _lib.load()
        return np.array([lib.ts_pixelcnn_stream_slot_rows(self._h, b) for b in range(self.B)], np.int64)

    def _touch(self, slots, clip_rows, pairs):
        """The pair table behind a restart or load of `slots` that (re-)declares `pairs`, validated as a whole before any device work:
        -> (the new table, the parsed declaration or None).  clip_rows: the rows the listed slots' clips will hold."""
        from talkshow_amd.streaming import SlotPairs
        held = self._pair_table(make=False)
        if not pairs and (held is None or not held.pairs):      # no pair is held and none is declared: nothing to check, nothing to keep
            return held, None
        rows = self.rows
        sim = self._pair_table().copy()
        sim.check_touch(rows, slots)
        sim.touched(rows, slots)
        declared = None
        if pairs:
            declared = SlotPairs.parse(pairs)
            held = [int(v) for v in self.slot_rows]
            for b, n in zip(slots, clip_rows):
                held[b] = int(n)
            sim.pair(rows, held, *declared)
        return sim, declared

    def restart(self, slots, label=None, *, style=None, clip_indices=None, pairs=None):
        """Slot restart (`ts_pixelcnn_stream_restart`; talkshow_hip.h, "slot restart"): each listed slot ends its clip and begins a NEW one at
        the session's next row, while the other slots carry on — continuous batching.  From there on the slot's codes and
        log-probabilities are those of `run` on the new clip alone (same mode, seed and keywords, clip_index0 = its clip index), bit for
        bit, and every other slot's bits are those of the session without the call.
        slots: one slot or a list of distinct slots.  label: the new clips' class labels (one for all listed slots, or one each), OR
        style: one (n_classes,) weight row for all, or a list / (n, n_classes) array with one row each (`None` entries take `label`'s
        entry).  clip_indices: the new clips' Philox clip indices (default: the slot numbers); a restarted slot keeps its index whatever
        `clip_index0` later steps pass.  Any number of times, at any row.  The session's labels follow, so a later `style=[None, ...]`
        means the NEW clip's own label; a weight row given here holds until a step brings style rows (a session default `style`
        does, at every step).  Keywords of later steps keep counting in session rows: `given` from the step's first row, and a restarted
        slot's `repeat` history is empty at its first row.  A slot whose user has left needs no call and no mask: it keeps stepping on
        whatever audio rows it is given and its output is ignored.  A bad value raises ValueError naming the slot before any device
        work; `rows` and `slot_rows` do not move.
        pairs: {primary: shadow} or {primary: (shadow, scale)} among the slots this call lists ("session pairs"): the two begin a guided
        clip together.  A slot of a pair restarts only with its other slot ("slot 3 is paired with slot 7: list both"); listing both
        dissolves the pair unless `pairs` declares it again."""
        from talkshow_amd.streaming import SlotClock
        NC = self.net.n_classes
        slots, labels, styles, clips = SlotClock.check(self.B, NC, slots, label, style, clip_indices)
        n = len(slots)
        sim, declared = self._touch(slots, [0] * n, pairs)
        rows = None
        if styles is not None:          # one entry of the C call's two tables is NULL: labels become their one-hot rows beside weight rows
            rows = np.zeros((n, NC), np.float32)
            for i in range(n):
                if styles[i] is None:
                    rows[i, int(labels[i])] = 1.0
                else:
                    e = styles[i]
                    rows[i] = np.asarray(e.detach().cpu().numpy() if hasattr(e, "detach") else e, np.float32)
        i32, i64 = C.c_int32 * n, C.c_int64 * n
        style_dev = upload(rows, self.net._dev()) if rows is not None else None
        _lib.check(_lib.load().ts_pixelcnn_stream_restart(
            self._h, i32(*slots), n, None if rows is not None else i64(*[int(v) for v in labels]), _lib.dptr(style_dev), i64(*clips),
            _lib.stream_ptr()))
        self._pairs = sim
        if declared:
            self._declare(*declared)
        for i, b in enumerate(slots):   # what `style=[None, ...]` stands for from here on; a blend keeps the slot's old label
            if labels is not None and labels[i] is not None:
                self._labels[b] = int(labels[i])
        return self

    # ---- slot state (talkshow_hip.h, "slot state"; the rule is restated at `streaming.SlotClock`) ----
    def _dims(self):
        net = self.net
        return (int(net.dim), int(net.n_layers), int(net.n_classes), int(net.input_dim))

    def save(self, slots):
        """Slot state (`ts_pixelcnn_stream_save`): the state of each listed slot at the session's next row -> `SlotState` on the session's
        device.  Read-only: the session's later bits, launches and graph captures are those without the call; stream-ordered, no
        synchronisation.  Loaded into any slot of any session of a network with the same dimensions and weights (`load`), the slot carries
        the clip on: its rows equal rows n, n+1, ... of `run` over the clip's whole audio with `given=` its first n code rows, bit for bit.
        The state carries the conditioning rows, the label the slot stands for, the repetition histories, the clip index and n — not the
        sampling records, bias tables, defaults or given rows of a step.  A bad slot raises ValueError before any device work."""
        from talkshow_amd.streaming import SlotClock, SlotState
        slots = SlotClock.check_slots(self.B, slots, "save")
        n, dev = len(slots), self.net._dev()
        lib = _lib.load()
        W = int(lib.ts_pixelcnn_slot_state_words(self.net.handle()))
        assert W == SlotClock.state_words(*self._dims()[:2])
        words = torch.empty((n, W), dtype=torch.int32, device=dev)
        info = (_lib.TsSlotInfo * n)()
        with torch.cuda.device(dev):
            _lib.check(lib.ts_pixelcnn_stream_save(self._h, (C.c_int32 * n)(*slots), n, _lib.dptr(words), info, _lib.stream_ptr()))
        infos = [{k: int(getattr(o, k)) for k, _ in _lib.TsSlotInfo._fields_} for o in info]
        for o, b in zip(infos, slots):      # the label the slot stands for: this handle has followed it through every restart and load
            o["label"] = int(self._labels[b])
        return SlotState(words, infos)

    def load(self, slots, state, *, clip_indices=None, pairs=None):
        """Slot state (`ts_pixelcnn_stream_load`): each listed slot takes a saved state — `state` holds one for all listed slots (fan-out) or
        one each — and carries that clip on from the session's next row under its clip index (clip_indices: one per slot; default: the
        index the source drew under).  The other slots keep their bits.  The state may come from another session, another batch size,
        another handle of a network with equal weights (not checked), another device, or `SlotState.frombytes`.  Refused with ValueError
        naming the slot, before any device work and with `rows` / `slot_rows` where they were: a slot out of range or listed twice, a count
        mismatch, a state of other (D, NL, NC, V) or version, session row < min(clip rows, 3), a negative clip index.  The session's first
        load does what its first restart does (steps on the restart graph keys from there on).
        pairs: as for `restart`, among the slots this call lists, whose states must hold clips of equal rows: a guided clip is saved as
        `save([b, g])` and carried on by `load([b2, g2], state, pairs={b2: g2})` (pairs are not part of a state)."""
        from talkshow_amd.streaming import SlotClock, SlotState
        if not isinstance(state, SlotState):
            raise ValueError(f"load: state must be a SlotState, got {type(state).__name__}")
        SlotClock.check_load(self.B, self._dims(), None, slots, state.infos, clip_indices)      # every rule the arguments alone decide,
        slots, index, clips = SlotClock.check_load(self.B, self._dims(), self.rows, slots, state.infos, clip_indices)   # then the row's
        sim, declared = self._touch(slots, [state.infos[k]["rows"] for k in index], pairs)
        n, m, dev = len(slots), len(state), self.net._dev()
        W = SlotClock.state_words(*self._dims()[:2])
        if tuple(state.words.shape) != (m, W):
            raise ValueError(f"load: the state's words have shape {tuple(state.words.shape)}, this network's states are ({m}, {W})")
        words = state.words.to(device=dev, dtype=torch.int32).contiguous()
        if words.data_ptr() % 16:
            words = words.clone()
        info = (_lib.TsSlotInfo * m)()
        for o, d in zip(info, state.infos):
            for k, _ in _lib.TsSlotInfo._fields_:
                setattr(o, k, int(d[k]))
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ts_pixelcnn_stream_load(self._h, (C.c_int32 * n)(*slots), n, _lib.dptr(words), m, (C.c_int32 * n)(*index), info,
                                                          (C.c_int64 * n)(*clips), _lib.stream_ptr()))
        self._pairs = sim
        if declared:
            self._declare(*declared)
        for b, k in zip(slots, index):      # what `style=[None, ...]` stands for from here on
            self._labels[b] = int(state.infos[k]["label"])
        return self

    def fork(self, src, dst_slots, *, clip_indices=None):
        """`save(src)` and `load(dst_slots, ...)` inside this session: every listed slot carries slot `src`'s clip on (N candidate
        continuations of a live clip: give each its own clip index).  Checked as a whole before anything is launched."""
        from talkshow_amd.streaming import SlotClock
        src = SlotClock.check_slots(self.B, src, "fork")
        if len(src) != 1:
            raise ValueError(f"fork: one source slot, got {len(src)}")
        dst = SlotClock.check_slots(self.B, dst_slots, "fork", distinct=True)
        if clip_indices is not None:
            clip_indices = [clip_indices] * len(dst) if isinstance(clip_indices, int) else list(clip_indices)
            if len(clip_indices) != len(dst):
                raise ValueError(f"fork: {len(dst)} slots but {len(clip_indices)} clip index entries")
            for b, c in zip(dst, clip_indices):
                if int(c) != c or int(c) < 0:
                    raise ValueError(f"fork: slot {b}: clip index {c} is negative")
        return self.load(dst, self.save(src), clip_indices=clip_indices)

    def close(self):
        if self._h is not None:
            torch.cuda.synchronize()
            _lib.load().ts_pixelcnn_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FaceGenerator(NativeModule):
    """`s2g_face.Generator(n_poses, each_dim, dim_list, training, device, identity, num_classes)` (`s2g_face.py:142-224`)."""

    def __init__(self, n_poses=88, each_dim=None, dim_list=None, training=False, device=None, identity=True,
                 num_classes=4, n_layers=12):
        # identity=False is what the reference wrapper builds when convert_to_6d is set (`smplx_face.py:37-45`): no id channels,
        # jaw head each_dim[0] wide (6)
        self.identity, self.num_classes, self.n_layers = bool(identity), num_classes, n_layers
        self.jaw_dim = int(each_dim[0]) if each_dim else (3 if identity else 6)
        if self.jaw_dim != (3 if identity else 6):
            raise NotImplementedError(f"jaw head of width {self.jaw_dim} with identity={identity}: the reference pairs 3 with True, 6 with False")
        self.out_dim = self.jaw_dim + 100
        self.device = device
        super().__init__(synth.face_state_dict(0, n_layers=n_layers, num_classes=num_classes, identity=self.identity, jaw_dim=self.jaw_dim))

    def load_state_dict(self, sd, strict=True):
        # checkpoints written with transformers 4.22 (the reference's pin) spell the weight-normed positional conv
        # `weight_g` / `weight_v`
        ren = {"audio_encoder.encoder.pos_conv_embed.conv.weight_g":
               "audio_encoder.encoder.pos_conv_embed.conv.parametrizations.weight.original0",
               "audio_encoder.encoder.pos_conv_embed.conv.weight_v":
               "audio_encoder.encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
        sd = OrderedDict((ren.get(k.replace("module.", ""), k.replace("module.", "")), v) for k, v in sd.items())
        return super().load_state_dict(sd, strict)

    def _create(self, ctx):
        arr, n, keep = _lib.pack_state_dict(self._sd)
        h = C.c_void_p()
        _lib.check(_lib.load().ts_face_create(ctx, arr, n, self.n_layers, self.num_classes if self.identity else 0, C.byref(h)))
        return h

    def _destroy(self, h):
        _lib.load().ts_face_destroy(h)

    def set_arith(self, bf16_products=0):
        """OPT-IN arithmetic plan of the generator's GEMMs (`ts_face_set_arith`): 0 = fp32 MFMA (default; the parity path),
        3 / 6 = split-bf16 with three / six exact bf16 products per fp32 product.  Returns self."""
        _lib.check(_lib.load().ts_face_set_arith(self.handle(), int(bf16_products)))
        return self

    def run(self, wav, id_vec, frames, want_hidden=False):
        """wav (B,N) device fp32, id_vec (B,num_classes) -> (B,frames,103) [, hidden (B,frames,768)]; (B,frames,106) for identity=False."""
        dev = self._dev()
        wav = _dev_f32(wav, dev)
        B, N = wav.shape
        if self.identity:
            id_vec = _dev_f32(id_vec, dev).reshape(-1, self.num_classes)
            if id_vec.shape[0] == 1 and B > 1:
                id_vec = id_vec.repeat(B, 1).contiguous()
        else:
            id_vec = None                                    # Generator(identity=False) never looks at it
        out = torch.empty((B, frames, self.out_dim), dtype=torch.float32, device=dev)
        hid = torch.empty((B, frames, 768), dtype=torch.float32, device=dev) if want_hidden else None
        _lib.check(_lib.load().ts_face_generate(self.handle(), _lib.dptr(wav), B, N, int(frames), _lib.dptr(id_vec),
                                                _lib.dptr(out), _lib.dptr(hid), _lib.stream_ptr()))
        return (out, hid) if want_hidden else out

    def _check_clips(self, wavs, id_vec, frames):
        """Host-side argument checking of `run_clips` (no device call): -> (list of 1-D float32 arrays, ns, frames, id rows or None)."""
        if isinstance(wavs, (np.ndarray, torch.Tensor)) or not hasattr(wavs, "__len__") or len(wavs) < 1:
            raise ValueError("run_clips: wavs must be a non-empty list of 1-D sample arrays")
        clips = []
        for b, w in enumerate(wavs):
            a = w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
            if a.ndim != 1:
                raise ValueError(f"run_clips: clip {b} has shape {tuple(a.shape)}; a 1-D array of 16 kHz samples is expected")
            if a.shape[0] < 400:
                raise ValueError(f"run_clips: clip {b} has {a.shape[0]} samples; the feature extractor needs at least 400")
            clips.append(np.ascontiguousarray(a, dtype=np.float32))
        B = len(clips)
        ns = np.array([c.shape[0] for c in clips], dtype=np.int32)
        if frames is None:
            fr = (ns.astype(np.int64) * 30 // 16000).astype(np.int32)        # 30 fps out of 16 kHz in
        else:
            fr = np.asarray(frames)
            if fr.ndim != 1 or fr.shape[0] != B or not np.issubdtype(fr.dtype, np.integer):
                raise ValueError(f"run_clips: frames must be {B} integers, one per clip")
            fr = fr.astype(np.int32)
        if (fr < 1).any():
            raise ValueError(f"run_clips: clip {int(np.argmax(fr < 1))} would have no output frame")
        ids = None
        if self.identity:
            if id_vec is None:
                ids = np.zeros((B, self.num_classes), dtype=np.float32)
            else:
                ids = (id_vec.detach().cpu().numpy() if torch.is_tensor(id_vec) else np.asarray(id_vec)).astype(np.float32)
                if ids.ndim != 2 or ids.shape[1] != self.num_classes or ids.shape[0] not in (1, B):
                    raise ValueError(f"run_clips: id_vec must be ({B}, {self.num_classes}) or (1, {self.num_classes}), got {tuple(ids.shape)}")
                if ids.shape[0] == 1 and B > 1:
                    ids = np.repeat(ids, B, axis=0)
            ids = np.ascontiguousarray(ids)
        return clips, ns, fr, ids

    @staticmethod
    def mixed_rows(wavs_or_counts, frames=None):
        """What a mixed pass of these clips computes, in rows (`ts_face_mixed_rows`; host arithmetic, no device): wavs_or_counts = the list
        `run_clips` takes, or the clips' sample counts; frames as for `run_clips` -> dict(feature_rows_padded, feature_rows_packed,
        frames_padded, frames_packed).  The feature convolutions cost in proportion to feature_rows_packed, the transformer layers to
        frames_packed, the feature projection, positional convolution and heads to frames_padded."""
        ns = np.asarray([int(w) if np.ndim(w) == 0 else int(w.shape[0]) for w in wavs_or_counts], dtype=np.int64)
        if ns.size < 1 or (ns < 400).any() or (ns >= 2 ** 31).any():
            raise ValueError("mixed_rows: a non-empty list of clips of at least 400 samples each is expected")
        ns = ns.astype(np.int32)
        fr = (ns.astype(np.int64) * 30 // 16000).astype(np.int32) if frames is None else np.asarray(frames)
        if fr.ndim != 1 or fr.shape[0] != ns.shape[0] or not np.issubdtype(fr.dtype, np.integer) or (fr < 1).any():
            raise ValueError(f"mixed_rows: frames must be {ns.shape[0]} positive integers, one per clip")
        fr = np.ascontiguousarray(fr, dtype=np.int32)
        out = (C.c_int64 * 4)()
        i32p = C.POINTER(C.c_int32)
        _lib.check(_lib.load().ts_face_mixed_rows(ns.ctypes.data_as(i32p), fr.ctypes.data_as(i32p), len(ns), int(ns.max()), int(fr.max()), out))
        return dict(zip(("feature_rows_padded", "feature_rows_packed", "frames_padded", "frames_packed"), (int(v) for v in out)))

    def run_clips(self, wavs, id_vec, frames=None, want_hidden=False, layout=None):
        """Clips of DIFFERENT lengths in one pass (`ts_face_generate_mixed`): wavs = list of 1-D arrays / tensors of 16 kHz samples (>= 400 each),
        id_vec (B,num_classes), (1,num_classes) or None (all-zero rows), frames = one frame count per clip (default len * 30 // 16000)
        -> list of (frames[b], 103 | 106) device tensors [, list of hidden states (frames[b], 768)].  A clip's rows are bit-identical whatever
        else is in the pass.  layout: None = the library's plan (padded to the longest clip unless TS_FACE_PACK=1); 0 / 1 name the padded plan / the
        packed plan (the clips' own rows back to back in the feature convolutions and the transformer; same bits).  Wrong argument shapes raise ValueError before any
        device call."""
        if layout not in (None, 0, 1):
            raise ValueError("run_clips: layout is None, 0 (padded) or 1 (packed)")
        clips, ns, fr, ids = self._check_clips(wavs, id_vec, frames)
        dev = self._dev()
        B, N_max, T_max = len(clips), int(ns.max()), int(fr.max())
        padded = np.zeros((B, N_max), dtype=np.float32)
        for b, c in enumerate(clips):
            padded[b, :c.shape[0]] = c
        wav = torch.from_numpy(padded).to(dev)
        ns_dev, fr_dev = torch.from_numpy(ns).to(dev), torch.from_numpy(fr).to(dev)
        id_dev = torch.from_numpy(ids).to(dev) if ids is not None else None
        out = torch.empty((B, T_max, self.out_dim), dtype=torch.float32, device=dev)
        hid = torch.empty((B, T_max, 768), dtype=torch.float32, device=dev) if want_hidden else None
        _lib.face_generate_mixed(self.handle(), wav, ns, ns_dev, fr, fr_dev, B, N_max, T_max, id_dev, out, hid, layout)
        outs = [out[b, :int(fr[b])] for b in range(B)]
        return (outs, [hid[b, :int(fr[b])] for b in range(B)]) if want_hidden else outs

    def __call__(self, in_spec, gt_poses=None, id=None, pre_state=None, time_steps=None):
        """reference call shape (`s2g_face.py:196`): in_spec (B,1,N) -> (out (B,time_steps,103), None)."""
        wav = _dev_f32(in_spec, self._dev())
        wav = wav.reshape(wav.shape[0], -1)
        return self.run(wav, id, time_steps), None


class MFCC:
    """Device front-end: `get_mfcc_ta` = torchaudio Resample(sr_in -> sr_out) + MFCC(64) (`data_utils/utils.py:148-231`)."""

    def __init__(self, sr_in, sr_out=22000, fps=30, device=None):
        self.sr_in, self.sr_out, self.fps = int(sr_in), int(sr_out), int(fps)
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        self._dev = torch.device("cuda", idx if idx is not None else torch.cuda.current_device())
        h = C.c_void_p()
        _lib.check(_lib.load().ts_mfcc_create(_lib.context(self._dev.index), self.sr_in, self.sr_out, self.fps, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            _lib.load().ts_mfcc_destroy(self._h)
        except Exception:
            pass

    def resample(self, wav):
        """stage 1 alone: wav (B,N) or (N,) at sr_in -> (B,N') at sr_out (torchaudio sinc-Hann polyphase), device tensor."""
        wav = _dev_f32(wav, self._dev)
        if wav.ndim == 1:
            wav = wav[None]
        B, N = wav.shape
        out = torch.empty((B, _lib.load().ts_mfcc_resampled_len(self._h, N)), dtype=torch.float32, device=self._dev)
        _lib.check(_lib.load().ts_mfcc_resample(self._h, _lib.dptr(wav), B, N, _lib.dptr(out), _lib.stream_ptr()))
        return out

    def __call__(self, wav):
        """wav (B,N) or (N,) mono samples at sr_in -> (B,T,64) device tensor."""
        wav = _dev_f32(wav, self._dev)
        if wav.ndim == 1:
            wav = wav[None]
        B, N = wav.shape
        T = _lib.load().ts_mfcc_num_frames(self._h, N)
        out = torch.empty((B, T, 64), dtype=torch.float32, device=self._dev)
        _lib.check(_lib.load().ts_mfcc_forward(self._h, _lib.dptr(wav), B, N, _lib.dptr(out), _lib.stream_ptr()))
        return out


    # --- recordings of different lengths in one call (`ts_mfcc_*_mixed`) ---
    def _tables(self, ns):
        from .frontend import mixed_tables
        return mixed_tables(ns, self.sr_in, self.sr_out, self.fps)

    def forward_padded(self, wav, ns_host, ns_dev):
        """wav (B,N_max) device block, ns_host (B,) int32 numpy and ns_dev its device copy -> (B,T_max,64), rows beyond a recording's own
        T_b = 0.  No host work beyond the check of ns_host, no synchronisation."""
        B, N_max = wav.shape
        T_max = int(self._tables([N_max])["mfcc_rows"][0])
        out = torch.empty((B, T_max, 64), dtype=torch.float32, device=self._dev)
        _lib.check(_lib.load().ts_mfcc_forward_mixed(self._h, _lib.dptr(wav), ns_host.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     _lib.dptr(ns_dev), B, N_max, _lib.dptr(out), _lib.stream_ptr()))
        return out

    def run_clips(self, wavs):
        """Recordings of DIFFERENT lengths in one call (`ts_mfcc_forward_mixed`): wavs = list of (N_b,) arrays / tensors at sr_in -> list of
        (T_b, 64) device views of one padded result.  A recording's rows are bit-identical whatever else is in the list, and equal
        `MFCC(...)(wav_b)`."""
        from .frontend import check_recordings
        ns = check_recordings(wavs, "MFCC.run_clips")
        wav, ns_host, ns_dev = pad_recordings(wavs, ns, range(len(ns)), self._dev)
        out = self.forward_padded(wav, ns_host, ns_dev)
        rows = self._tables(ns)["mfcc_rows"]
        return [out[b, :int(rows[b])] for b in range(len(ns))]

    def resample_clips(self, wavs):
        """Stage 1 alone on recordings of different lengths (`ts_mfcc_resample_mixed`) -> list of (N'_b,) device views at sr_out."""
        from .frontend import check_recordings
        ns = check_recordings(wavs, "MFCC.resample_clips")
        wav, ns_host, ns_dev = pad_recordings(wavs, ns, range(len(ns)), self._dev)
        B, N_max = wav.shape
        n_res = self._tables(ns)["n_resampled"]
        out = torch.empty((B, int(self._tables([N_max])["n_resampled"][0])), dtype=torch.float32, device=self._dev)
        _lib.check(_lib.load().ts_mfcc_resample_mixed(self._h, _lib.dptr(wav), ns_host.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      _lib.dptr(ns_dev), B, N_max, _lib.dptr(out), _lib.stream_ptr()))
        return [out[b, :int(n_res[b])] for b in range(B)]


    # --- samples in chunks (`ts_mfcc_stream_*`; talkshow_hip.h, "wav sessions") ---
    @property
    def constants(self):
        """The handle's resampler constants: dict of norig, nnew, width, kw (1, 1, 0, 0 at equal rates) and hop."""
        out = (C.c_int32 * 5)()
        _lib.load().ts_mfcc_constants(self._h, out)
        return dict(zip(("norig", "nnew", "width", "kw", "hop"), (int(v) for v in out)))

    def peak_db(self, wavs):
        """The maximum the one-shot call clamps each recording at (its floor is this - 80 dB): wavs (B,N) / (N,) samples at sr_in, or a list of
        (N_b,) recordings of different lengths -> (B,) float32 device tensor (`ts_mfcc_peak_db_mixed`).  Does not synchronise."""
        from .frontend import check_recordings
        if not isinstance(wavs, (list, tuple)):
            wavs = _dev_f32(wavs, self._dev)
            wavs = list(wavs[None] if wavs.ndim == 1 else wavs)
        ns = check_recordings(wavs, "MFCC.peak_db")
        wav, ns_host, ns_dev = pad_recordings(wavs, ns, range(len(ns)), self._dev)
        out = torch.empty((len(ns),), dtype=torch.float32, device=self._dev)
        _lib.check(_lib.load().ts_mfcc_peak_db_mixed(self._h, _lib.dptr(wav), ns_host.ctypes.data_as(C.POINTER(C.c_int32)), _lib.dptr(ns_dev),
                                                     len(ns), int(wav.shape[1]), _lib.dptr(out), _lib.stream_ptr()))
        return out

    def open_stream(self, B, max_samples, db="running"):
        """A session that takes the recording's samples in chunks: `MFCCStream`.  db="running": the floor of row t is the maximum over rows
        0 .. t, minus 80 dB; db = a (B,) tensor or array (or one number): the recordings' maxima in dB (`peak_db`), known beforehand — the
        rows then equal `self(wav)` bit for bit, whatever the chunking."""
        return MFCCStream(self, B, max_samples, db)


class MFCCStream:
    """`MFCC.open_stream`: B slots on one sample clock.  `push(wav (B,n))` -> the (B,f,64) rows that became final (f may be 0; a row follows its
    centre sample by 1024 resampled samples and the resampler's right wing), `flush()` -> the rest, ending the recording; `plan(n, flush)`
    names f beforehand.  Concatenated, the rows are those of `MFCC(...)(wav)` for any chunking, bit for bit up to the clamp (see
    `MFCC.open_stream`).  A bad argument raises ValueError before any device work, and no counter moves.  Slots share the clock: there is no
    restart, save, load or fork."""

    def __init__(self, mfcc, B, max_samples, db="running"):
        self.mfcc, self.B, self.max_samples = mfcc, int(B), int(max_samples)
        if self.B < 1 or self.max_samples < 1:
            raise ValueError(f"open_stream: B and max_samples are at least 1, got B={B}, max_samples={max_samples}")
        peak = None
        if isinstance(db, str):
            if db != "running":
                raise ValueError(f"open_stream: db is \"running\" or the (B,) maxima in dB, got {db!r}")
        else:
            peak = torch.as_tensor(db, dtype=torch.float32).reshape(-1)
            if peak.numel() == 1 and self.B > 1:
                peak = peak.repeat(self.B)
            if peak.numel() != self.B:
                raise ValueError(f"open_stream: the maxima must hold 1 or B={self.B} values, got {peak.numel()}")
            if not bool(torch.isfinite(peak).all()):
                raise ValueError("open_stream: a maximum is not finite")
            peak = peak.to(mfcc._dev).contiguous()
        self.db = "running" if peak is None else "peak"
        h = C.c_void_p()
        with torch.cuda.device(mfcc._dev):
            torch.cuda.current_stream().synchronize()      # the table is copied at open
            _lib.check(_lib.load().ts_mfcc_stream_open(mfcc._h, self.B, self.max_samples, 0 if peak is None else 1, _lib.dptr(peak), C.byref(h)))
        self._h = h
        self.max_frames = int(_lib.load().ts_mfcc_stream_max_frames(h))
        self._flushed = False

    def _get(self, name):
        if self._h is None:
            raise ValueError("the session is closed")
        return int(getattr(_lib.load(), name)(self._h))

    @property
    def samples_in(self):
        return self._get("ts_mfcc_stream_samples_in")

    @property
    def frames_out(self):
        return self._get("ts_mfcc_stream_frames_out")

    @property
    def state_bytes(self):
        """Device bytes of the session's buffers: constant from open to close."""
        return self._get("ts_mfcc_stream_state_bytes")

    def plan(self, n, flush=False):
        """Rows the next call returns: `push` of n samples, or (flush=True; n is not read) `flush()`.  ValueError where that call would."""
        if self._h is None:
            raise ValueError("the session is closed")
        if self._flushed:
            raise ValueError("the session has been flushed (the recording has ended): open another")
        n = 0 if flush else int(n)
        if n < 0 or n > self.max_samples:
            raise ValueError(f"a push holds 0 to max_samples = {self.max_samples} samples, got {n}")
        m, before, after = self.mfcc, C.c_long(), C.c_long()
        try:
            _lib.check(_lib.load().ts_mfcc_stream_plan(m.sr_in, m.sr_out, m.fps, self.samples_in, n, int(bool(flush)), C.byref(before), C.byref(after)))
        except RuntimeError as e:          # host arithmetic only: a refusal is about the arguments
            raise ValueError(str(e)) from None
        return int(after.value) - self.frames_out

    def push(self, wav):
        """wav (B,n) samples at sr_in, 0 <= n <= max_samples (a (n,) block where B = 1) -> (B,f,64) device tensor."""
        if not hasattr(wav, "shape") or len(wav.shape) not in (1, 2):
            raise ValueError(f"push: wav must have shape (B={self.B}, n), got {tuple(getattr(wav, 'shape', ()))}")
        shape = tuple(int(v) for v in wav.shape)
        if len(shape) == 1:
            shape = (1,) + shape
        if shape[0] != self.B:
            raise ValueError(f"push: wav must have shape (B={self.B}, n), got {tuple(wav.shape)}")
        n = shape[1]
        f = self.plan(n)
        dev = self.mfcc._dev
        out = torch.empty((self.B, f, 64), dtype=torch.float32, device=dev)
        w = _dev_f32(wav, dev).reshape(self.B, n) if n else None
        got = C.c_int()
        _lib.check(_lib.load().ts_mfcc_stream_push(self._h, _lib.dptr(w), n, _lib.dptr(out) if f else None, C.byref(got), _lib.stream_ptr()))
        assert got.value == f
        return out

    def flush(self):
        """The rows held back, ending the recording.  A recording of 1024 resampled samples or fewer is refused (ValueError), as by the one-shot
        call."""
        f = self.plan(0, flush=True)
        out = torch.empty((self.B, f, 64), dtype=torch.float32, device=self.mfcc._dev)
        got = C.c_int()
        _lib.check(_lib.load().ts_mfcc_stream_flush(self._h, _lib.dptr(out) if f else None, C.byref(got), _lib.stream_ptr()))
        assert got.value == f
        self._flushed = True
        return out

    def close(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize()
            _lib.load().ts_mfcc_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload(a, dev):
    """numpy array -> device tensor through pinned memory, without blocking the host (a pageable copy waits for the stream)."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def pad_pose_clips(poses_list, dev, who, width, lens=None):
    """Pose clips of different lengths -> (block (B, T_max, width) float32 device tensor, lens (B,) int32 numpy).  poses_list: a list of
    (P_b, width) arrays / tensors (padded here with zeros), or — with `lens` — one (B, T_max, width) block whose frames at or beyond lens[b]
    are never read.  ValueError naming the clip for a bad shape or a clip shorter than 4 frames (one code row).  Nothing waits for the device."""
    if lens is not None:
        block = _dev_f32(poses_list, dev)
        lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        if block.dim() != 3 or block.shape[0] != lens.size or block.shape[2] != width:
            raise ValueError(f"{who}: a padded block must have shape (B={lens.size}, T_max, {width}), got {tuple(block.shape)}")
        for b, t in enumerate(lens):
            if t < 4 or t > block.shape[1]:
                raise ValueError(f"{who}: clip {b} has {int(t)} frames; a clip holds 4 (one code row) to T_max = {int(block.shape[1])}")
        return block, lens
    if not isinstance(poses_list, (list, tuple)) or len(poses_list) < 1:
        raise ValueError(f"{who}: a non-empty list of (P, {width}) pose clips, got {type(poses_list).__name__}")
    for b, g in enumerate(poses_list):
        shape = tuple(getattr(g, "shape", ()))
        if len(shape) != 2 or shape[1] != width:
            raise ValueError(f"{who}: clip {b} must have shape (P, {width}), got {shape}")
        if shape[0] < 4:
            raise ValueError(f"{who}: clip {b} has {shape[0]} pose frames; one code row needs 4")
    lens = np.ascontiguousarray([int(g.shape[0]) for g in poses_list], dtype=np.int32)
    B, T_max = len(poses_list), int(lens.max())
    if all(torch.is_tensor(g) and g.is_cuda for g in poses_list):
        block = torch.zeros((B, T_max, width), dtype=torch.float32, device=dev)
        for b, g in enumerate(poses_list):
            block[b, :int(lens[b])] = g
    else:
        padded = np.zeros((B, T_max, width), dtype=np.float32)
        for b, g in enumerate(poses_list):
            padded[b, :int(lens[b])] = g.detach().cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        block = upload(padded, dev)
    return block, lens


def encode_pair_masked(g_body, g_hand, block, lens_dev, want_z=False):
    """`ts_vqvae_encode_pair_masked`: block (B, T_max, body + hand) device tensor, lens_dev (B,) int32 device table of the clips' own frame
    counts -> codes (B, T_max // 4, 2) int64 with -1 beyond a clip's rows [, z_body, z_hand (B, T_max // 4, embedding_dim), 0 beyond]."""
    B, T_max, ld = block.shape
    H = T_max // 4
    codes = torch.empty((B, H, 2), dtype=torch.int64, device=block.device)
    zb = torch.empty((B, H, g_body.embedding_dim), dtype=torch.float32, device=block.device) if want_z else None
    zh = torch.empty((B, H, g_hand.embedding_dim), dtype=torch.float32, device=block.device) if want_z else None
    _lib.check(_lib.load().ts_vqvae_encode_pair_masked(g_body.handle(), g_hand.handle(), _lib.dptr(block), int(ld), _lib.dptr(lens_dev), int(B),
                                                       int(T_max), _lib.dptr(codes), _lib.dptr(zb), _lib.dptr(zh), _lib.stream_ptr()))
    return (codes, zb, zh) if want_z else codes


def ids_in_row_order(ids, n_classes, order, dev, what='speaker id'):
    """Class indices of a pass whose rows are recordings order[0], order[1], ...: ids (B values or one for all; anything `_index_tensor`
    takes) -> (B,) int64 device tensor in row order, range-checked like nn.Embedding.  Host ids are checked, broadcast and reordered on the
    host and travel through pinned memory: nothing waits for the stream.  Ids that already live on the device are reordered there."""
    B = len(order)
    if torch.is_tensor(ids) and ids.is_cuda:
        ids = _index_tensor(ids, n_classes, what, dev)
        if ids.numel() == 1 and B > 1:
            ids = ids.repeat(B)
        if ids.numel() != B:
            raise ValueError(f"ids must hold 1 or B={B} indices, got {ids.numel()}")
        return ids.index_select(0, upload(np.asarray(order, np.int64), dev)).contiguous()
    _check_index_range(ids, n_classes, what)
    a = (ids.detach().numpy() if torch.is_tensor(ids) else np.asarray(ids)).astype(np.int64).reshape(-1)
    if a.size == 1 and B > 1:
        a = np.repeat(a, B)
    if a.size != B:
        raise ValueError(f"ids must hold 1 or B={B} indices, got {a.size}")
    return upload(a[np.asarray(order, np.int64)], dev)


def pad_recordings(wavs, ns, order, dev):
    """The padded block of a pass: recording order[k] in row k of a (B, N_max) float32 device tensor, zeros beyond it, + the sample counts
    of the rows as int32 on the host and on the device.  Host recordings are padded on the host and travel in ONE copy; recordings that
    already live on the device are copied there.  Nothing here waits for the device."""
    order = list(order)
    ns_host = np.ascontiguousarray([int(ns[i]) for i in order], dtype=np.int32)
    N_max = int(ns_host.max())
    if all(torch.is_tensor(w) and w.is_cuda for w in wavs):
        wav = torch.zeros((len(order), N_max), dtype=torch.float32, device=dev)
        for k, i in enumerate(order):
            wav[k, :int(ns[i])] = wavs[i]
    else:
        padded = np.zeros((len(order), N_max), dtype=np.float32)
        for k, i in enumerate(order):
            w = wavs[i]
            padded[k, :int(ns[i])] = w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
        wav = upload(padded, dev)
    return wav, ns_host, upload(ns_host, dev)


def resample_kaiser_padded(wav, ns_host, ns_dev, sr_in, sr_out):
    """`ts_resample_kaiser_mixed` on a padded device block (B,N_max) -> (B, ceil(N_max sr_out / sr_in)), zeros beyond a recording's own samples."""
    B, N_max = wav.shape
    lib = _lib.load()
    out = torch.empty((B, lib.ts_resample_kaiser_len(N_max, int(sr_in), int(sr_out))), dtype=torch.float32, device=wav.device)
    _lib.check(lib.ts_resample_kaiser_mixed(_lib.context(wav.device.index), _lib.dptr(wav), ns_host.ctypes.data_as(C.POINTER(C.c_int32)),
                                            _lib.dptr(ns_dev), B, N_max, int(sr_in), int(sr_out), _lib.dptr(out), _lib.stream_ptr()))
    return out


def resample_kaiser_clips(wavs, sr_in, sr_out, device=None):
    """`resample_kaiser_device` on recordings of DIFFERENT lengths in one call (`ts_resample_kaiser_mixed`): list of (N_b,) -> list of
    (ceil(N_b sr_out / sr_in),) device views, each equal to the recording resampled alone."""
    from .frontend import check_recordings
    ns = check_recordings(wavs, "resample_kaiser_clips")
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    dev = torch.device("cuda", idx if idx is not None else torch.cuda.current_device())
    wav, ns_host, ns_dev = pad_recordings(wavs, ns, range(len(ns)), dev)
    out = resample_kaiser_padded(wav, ns_host, ns_dev, sr_in, sr_out)
    lib = _lib.load()
    return [out[b, :lib.ts_resample_kaiser_len(int(n), int(sr_in), int(sr_out))] for b, n in enumerate(ns)]


def resample_kaiser_device(wav, sr_in, sr_out, device=None):
    """`librosa.resample(..., res_type='kaiser_best')` on the GPU (`ts_resample_kaiser`): wav (B,N) -> (B, ceil(N*sr_out/sr_in))."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    dev = torch.device("cuda", idx if idx is not None else torch.cuda.current_device())
    wav = _dev_f32(wav, dev)
    if wav.ndim == 1:
        wav = wav[None]
    B, N = wav.shape
    lib = _lib.load()
    out = torch.empty((B, lib.ts_resample_kaiser_len(N, int(sr_in), int(sr_out))), dtype=torch.float32, device=dev)
    _lib.check(lib.ts_resample_kaiser(_lib.context(dev.index), _lib.dptr(wav), B, N, int(sr_in), int(sr_out), _lib.dptr(out),
                                      _lib.stream_ptr()))
    return out
