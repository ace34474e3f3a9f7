"""Drop-in for `nets/smplx_body_pixel.py` of the reference (speech -> body/hand code indices -> SMPL-X poses).

Same constructor, attributes and method signatures as the reference `TrainWrapper` (`smplx_body_pixel.py:26-326`);
the audio encoder, the autoregressive PixelCNN and both VQ decoders run in libtalkshow_hip.so.  Inference only.
"""
import numpy as np
import torch

from nets.base import TrainWrapperBaseClass, resolve_device
from talkshow_amd import _lib
from talkshow_amd.frontend import get_mfcc_sepa, get_mfcc_ta
from talkshow_amd.modules import AudioEncoder, GatedPixelCNN as pixelcnn, VQVAE as s2g_body, _index_tensor
from talkshow_amd.pose_index import c_index_3d, c_index_6d


def _fresh_seed():
    """A Philox key drawn from torch's generator (so `torch.manual_seed` makes sampling reproducible, as in the reference)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def mixed_pass_order(lens):
    """Order of a mixed pass: the clips by NON-INCREASING length, ties in submission order (a stable sort, so the order — and with it the
    memory a clip's rows live in — is a function of the lengths alone).  Returns (order, inverse): sorted slot k holds submitted clip
    order[k]; submitted clip b sits in slot inverse[b].  Pure host code (tests/test_mixed_pass_host.py)."""
    order = sorted(range(len(lens)), key=lambda b: (-int(lens[b]), b))
    inverse = [0] * len(order)
    for k, b in enumerate(order):
        inverse[b] = k
    return order, inverse


class TrainWrapper(TrainWrapperBaseClass):
    '''
    a wrapper receiving audio features and generating motion (reference: a wrapper receving a batch from data_utils
    and calculate loss)
    '''

    def __init__(self, args, config):
        model_cfg, pose_cfg = config.Model, config.Data.pose
        self.args, self.config = args, config
        self.device = resolve_device(args.gpu)
        self.global_step = self.epoch = 0
        self.convert_to_6d, self.expression = pose_cfg.convert_to_6d, pose_cfg.expression
        self.init_params()
        self.num_classes = 4
        self.audio = True
        self.composition, self.bh_model = model_cfg.composition, model_cfg.bh_model

        # the four networks of `smplx_body_pixel.py:46-57`, same hyper-parameters
        self.audioencoder = AudioEncoder(in_dim=64, num_hiddens=256, num_residual_layers=2,
                                         num_residual_hiddens=256).to(self.device)
        # 6-D rotations double every pose width (39 / 90 -> 78 / 180 modelled dims) and the reference then trades depth for
        # width in the code predictor (`smplx_body_pixel.py:48-52`)
        dim, layer = (512, 10) if self.convert_to_6d else (256, 15)
        self.generator = pixelcnn(2048, dim, layer, self.num_classes, self.audio, self.bh_model).to(self.device)
        vq_kw = dict(embedding_dim=64, num_embeddings=model_cfg.code_num, num_hiddens=1024, num_residual_layers=2,
                     num_residual_hiddens=512)
        self.g_body = s2g_body(self.each_dim[1], **vq_kw).to(self.device)
        self.g_hand = s2g_body(self.each_dim[2], **vq_kw).to(self.device)
        # ... and, as in the reference (`:59-62`), the VQ-VAE weights come from `Model.vq_path` right here
        vq_ckpt = torch.load(model_cfg.vq_path, map_location='cpu')['generator']
        self.g_body.load_state_dict(vq_ckpt['g_body'])
        self.g_hand.load_state_dict(vq_ckpt['g_hand'])

        self.discriminator = None
        self.c_index = c_index_6d if self.convert_to_6d else c_index_3d
        super().__init__(args, config)

    def init_optimizer(self):
        self.generator_optimizer = self.audioencoder_optimizer = self.discriminator_optimizer = None

    def state_dict(self):
        # the six entries of a reference checkpoint (`smplx_body_pixel.py:104-113`); optimiser slots stay empty here
        out = dict.fromkeys(('generator', 'generator_optim', 'audioencoder', 'audioencoder_optim', 'discriminator',
                             'discriminator_optim'))
        out['generator'] = self.generator.state_dict()
        out['audioencoder'] = self.audioencoder.state_dict() if self.audio else None
        return out

    def load_state_dict(self, state_dict):
        """Accepts what the reference accepts (`:115-142`): a checkpoint dict with 'generator' (+ 'audioencoder', optimiser
        entries ignored) or a bare generator state_dict; DataParallel's `module.` prefixes are dropped."""
        def unprefixed(sd):
            return {(k.replace('module.', '') if isinstance(k, str) else k): v for k, v in sd.items()}
        nested = {k: unprefixed(v) for k, v in state_dict.items() if hasattr(v, 'items')}
        self.generator.load_state_dict(nested['generator'] if 'generator' in nested else unprefixed(state_dict))
        if 'audioencoder' in nested and self.audioencoder is not None:
            self.audioencoder.load_state_dict(nested['audioencoder'])

    # ---------------------------------------------------------------------------------------------------------
    def _decode_pair(self, latents):
        """g_body.decode / g_hand.decode + torch.cat (smplx_body_pixel.py:279-285), written into one NLC buffer."""
        B, H, _ = latents.shape
        out = torch.empty((B, 4 * H, self.each_dim[1] + self.each_dim[2]), dtype=torch.float32, device=latents.device)
        self.g_body.decode_nlc(latents[..., 0].contiguous(), out=out, col0=0)
        self.g_hand.decode_nlc(latents[..., 1].contiguous(), out=out, col0=self.each_dim[1])
        return out

    def generate_batch(self, mfcc, ids, mode=_lib.TS_SAMPLE_PHILOX, uniforms=None, seed=None, clip_index0=0, _ids_checked=False, sampling=None,
                       logprobs=False, given=None, given_poses=None, given_keep=None, style=None, code_bias=None, repeat=None, guide=None,
                       alternatives=None):
        """Batched device entry (one call into the C ABI): mfcc (B,T,64), ids (B,) -> codes (B,H,2), poses (B,4H,129).

        This is what `infer_on_audio` runs after the front-end, for B different clips; bench.py and the multi-GPU
        driver use it directly.

        sampling: one sampling record (`_lib.sampling_record`: temperature, top_p, top_k) for all clips, or one per clip.  WITH a record the
        batch goes through the mixed entry (`generate_clips`, `ts_body_pixel_infer_mixed_ctl`) with equal lengths — a clip's codes there
        equal this entry's, bit for bit, so a neutral record changes nothing but the route.  Without one: the uniform entry below, unchanged.
        logprobs=True: a third return value, (B,H,2) float32, the log-probability of every code under the distribution it was drawn from
        (`ts_body_pixel_infer_mixed_lp`: the route of `sampling`, with or without a record; codes and poses are those of the call without it).
        given: one (B,G,2) integer block or a list of B entries (None or (G_b,2)): the clips' first code rows, taken instead of drawn
        (`generate_clips`, `ts_body_pixel_infer_mixed_given`).  None: nothing changes.
        given_poses: one (B,P,129) block or a list of B entries (None or (P_b,129)): the clips' first pose frames, encoded on the device into
        their first P_b // 4 code rows (`generate_clips`, `ts_body_pixel_infer_mixed_poses`).  None: nothing changes.
        given_keep: which positions of the given rows are taken — None (all), "body", "hand", a (G_b,2) mask, a list of these or one (B,G,2)
        block (`generate_clips`, `ts_body_pixel_infer_mixed_keep`).  None: nothing changes.
        style: float speaker weights in place of the integer ids — per clip None, an (NC,) row or an (H,NC) track, or one (NC,) / (B,NC)
        array for all clips (`generate_clips`, `ts_body_pixel_infer_mixed_style`).  None: nothing changes.
        code_bias: a per-clip bias / allow-list on the codes — one (2, V) table for all clips, or per clip None, a (2, V) table or a
        {"body", "hand"} dict (`generate_clips`, `ts_body_pixel_infer_mixed_bias`).  None: nothing changes.
        repeat: a per-clip repetition penalty over a window of earlier codes — one (window, presence, frequency) record or dict for all
        clips, or a list with one per clip (`generate_clips`, `ts_body_pixel_infer_mixed_repeat`).  None: nothing changes.
        guide: per-clip guidance against a second conditioning — one dict for all clips or a list with, per clip, None or {"scale",
        "mfcc" (T,64), "id", "style"} (`generate_clips`, `ts_body_pixel_infer_guided`).  None: nothing changes.
        alternatives: n in [0, 8] -> one more return value, a `sampling.Alternatives` over the (B,H,2) positions: the n likeliest codes with
        their log-probabilities, the entropy and the rank of the position's code (`generate_clips`, `ts_body_pixel_infer_alt`).  None:
        nothing changes.
        """
        if not (logprobs is None or isinstance(logprobs, bool)):
            raise ValueError("generate_batch: logprobs is True or False (GatedPixelCNN.run takes an output tensor)")
        if (sampling is not None or logprobs or given is not None or given_poses is not None or given_keep is not None or style is not None
                or code_bias is not None or repeat is not None or guide is not None or alternatives is not None):
            dev = self.generator._dev()
            mfcc = torch.as_tensor(mfcc, dtype=torch.float32, device=dev)
            u = None if uniforms is None else list(torch.as_tensor(uniforms, dtype=torch.float32).unbind(0))
            return self.generate_clips(list(mfcc.unbind(0)), ids, mode=mode, uniforms=u, seed=seed, clip_index0=clip_index0,
                                       _ids_checked=_ids_checked, _stacked=True, sampling=sampling, logprobs=bool(logprobs), given=given,
                                       given_poses=given_poses, given_keep=given_keep, style=style, code_bias=code_bias, repeat=repeat,
                                       guide=guide, alternatives=alternatives)
        dev = self.generator._dev()
        mfcc = torch.as_tensor(mfcc, dtype=torch.float32, device=dev).contiguous()
        if _ids_checked:   # generate_batches range-checked every batch's ids before stacking them (no sync on the stacked tensor)
            ids = torch.as_tensor(ids, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        else:
            ids = _index_tensor(ids, self.num_classes, 'speaker id', dev)   # IndexError like nn.Embedding; host inputs are checked without a sync
        B, T, _ = mfcc.shape
        H = T // 2 // 2
        # nn.Embedding of a single label broadcasts over the batch in the reference (gated_pixelcnn_v2.py:65-66)
        if ids.numel() == 1 and B > 1:
            ids = ids.repeat(B)
        if ids.numel() != B:
            raise ValueError(f"ids must hold 1 or B={B} speaker indices, got {ids.numel()}")
        if seed is None:   # like the reference, which draws from torch's generator on every call: repeated calls differ
            seed = _fresh_seed() if mode == _lib.TS_SAMPLE_PHILOX else 0     # greedy / injected uniforms never read it
        codes = torch.zeros((B, H, 2), dtype=torch.int64, device=dev)
        poses = torch.empty((B, 4 * H, self.each_dim[1] + self.each_dim[2]), dtype=torch.float32, device=dev)
        if uniforms is not None:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32, device=dev).contiguous()
        _lib.check(_lib.load().ts_body_pixel_infer(
            self.audioencoder.handle(), self.generator.handle(), self.g_body.handle(), self.g_hand.handle(),
            _lib.dptr(mfcc), _lib.dptr(ids), B, T, mode, _lib.dptr(uniforms), int(seed) & (2 ** 64 - 1), int(clip_index0),
            _lib.dptr(codes), _lib.dptr(poses), _lib.stream_ptr()))
        return codes, poses

    def score_batch(self, mfcc, ids, codes):
        """Teacher-forced scoring of GIVEN codes: mfcc (B,T,64), ids (B,) or one for all, codes (B,T//4,2) int64 -> (logprobs (B,H,2)
        float32, sums (B,3) float64): log p(code | earlier codes, audio, speaker) at every position under the model's raw distribution,
        and per clip the fixed-order float64 sums {body column, hand column, both} — the negative of a clip's total is its NLL.  The
        audio encoder and `GatedPixelCNN.score` (`ts_pixelcnn_generate_lp`, `ts_logprob_sums`): no logits are written anywhere."""
        dev = self.generator._dev()
        mfcc = torch.as_tensor(mfcc, dtype=torch.float32, device=dev).contiguous()
        if mfcc.dim() != 3:
            raise ValueError(f"score_batch: mfcc must be (B, T, 64), got {tuple(mfcc.shape)}")
        B, T, _ = mfcc.shape
        _lib.score_codes_shape(tuple(getattr(codes, "shape", ())), B, T // 4)
        ids = _index_tensor(ids, self.num_classes, 'speaker id', dev)
        rows = self.audioencoder.forward_nlc(mfcc)
        return self.generator.score(ids, rows, codes)

    def generate_batches(self, mfccs, ids_list, mode=_lib.TS_SAMPLE_PHILOX, seed=None, clip_index0=0, sampling=None, logprobs=False):
        """Coalesced execution of several independent batches (the serving path): the batches' clips are stacked and
        the autoregressive chain runs ONCE over all of them, so a stage's weights are streamed once for all batches
        in flight instead of once per batch (a chain stage is latency-bound below ~64 clips).  Results are bit-identical
        to running each batch alone (tests/test_gpu_parity.py::test_golden_clips_inside_baseline_batches); global clip
        indices (the Philox subsequences) run on from `clip_index0` in list order.

        Batches whose T differ ride in ONE mixed pass (`generate_clips`: length-masked conv stacks, the chain over a shrinking prefix
        of the clips); each batch gets its results trimmed to its own H and 4 H, with the same bits and the same Philox subsequences.
        Batches of one T take the uniform path below, unchanged.  sampling: one sampling record for all clips or one per clip of the
        stacked batches, in list order; WITH a record the batches go through the mixed pass whatever their lengths (equal ones included):
        a clip's codes there equal the uniform entry's.  logprobs=True: every batch's tuple gains its (B_i,H_i,2) log-probabilities, and
        the batches take the mixed pass as with a record.

        mfccs: list of (B_i,T_i,64) device tensors, ids_list: list of (B_i,) -> list of (codes_i, poses_i) views."""
        dev = self.generator._dev()
        sizes = [int(m.shape[0]) for m in mfccs]
        if len({int(m.shape[1]) for m in mfccs}) > 1 or sampling is not None or logprobs:     # different lengths, controls or log-probabilities: one mixed pass
            return self._generate_batches_mixed(mfccs, ids_list, sizes, mode, seed, clip_index0, sampling, bool(logprobs))
        # nn.Embedding's IndexError per submitted batch, BEFORE stacking: host ids are checked on the host, a caller-owned device
        # tensor once per tensor version (modules._check_index_range) — the stacked tensor built below is new on every call, and
        # checking it would cost the serving path one blocking device -> host read per pass
        from talkshow_amd.modules import _check_index_range
        for i in ids_list:
            _check_index_range(i, self.num_classes, 'speaker id')
        mf = torch.cat([torch.as_tensor(m, dtype=torch.float32, device=dev) for m in mfccs], 0)
        ids = torch.cat([torch.as_tensor(i, dtype=torch.int64, device=dev).reshape(-1).expand(b) if
                         torch.as_tensor(i).numel() == 1 else torch.as_tensor(i, dtype=torch.int64, device=dev).reshape(-1)
                         for i, b in zip(ids_list, sizes)], 0)
        codes, poses = self.generate_batch(mf, ids, mode=mode, seed=seed, clip_index0=clip_index0, _ids_checked=True)
        return list(zip(codes.split(sizes, 0), poses.split(sizes, 0)))

    def _generate_batches_mixed(self, mfccs, ids_list, sizes, mode, seed, clip_index0, sampling=None, logprobs=False):
        from talkshow_amd.modules import _check_index_range
        dev = self.generator._dev()
        clips, ids = [], []
        for m, i, b in zip(mfccs, ids_list, sizes):
            _check_index_range(i, self.num_classes, 'speaker id')
            m = torch.as_tensor(m, dtype=torch.float32, device=dev)
            i = torch.as_tensor(i, dtype=torch.int64, device=dev).reshape(-1)
            if i.numel() == 1 and b > 1:
                i = i.expand(b)
            if i.numel() != b:
                raise ValueError(f"ids must hold 1 or B={b} speaker indices, got {i.numel()}")
            clips += list(m.unbind(0))
            ids.append(i)
        res = self.generate_clips(clips, torch.cat(ids, 0), mode=mode, seed=seed, clip_index0=clip_index0, _ids_checked=True,
                                  _stacked=True, sampling=sampling, logprobs=logprobs)
        codes, poses = res[0], res[1]
        out, k = [], 0
        for m, b in zip(mfccs, sizes):          # per submitted batch, trimmed to that batch's own H and 4 H
            H = int(m.shape[1]) // 4
            out.append((codes[k:k + b, :H], poses[k:k + b, :4 * H]) + ((res[2][k:k + b, :H],) if logprobs else ()))
            k += b
        return out

    def generate_clips(self, mfcc_list, ids, mode=_lib.TS_SAMPLE_PHILOX, uniforms=None, seed=None, clip_index0=0, clip_indices=None,
                       _ids_checked=False, _stacked=False, sampling=None, logprobs=False, given=None, given_poses=None, given_keep=None,
                       style=None, code_bias=None, repeat=None, guide=None, alternatives=None):
        """One MIXED pass over clips of different lengths (`ts_body_pixel_infer_mixed`): mfcc_list = list of (T_b,64) clips, ids (B,) or
        one id for all -> list of (codes_b (H_b,2), poses_b (4 H_b,129)) in submission order, H_b = T_b // 4.

        Every clip's result is bit-identical to `generate_batch` on the clip alone.  The library wants the clips ordered by length; they
        are sorted here (stable, longest first), padded to the longest, and the results are put back in submission order.  Clip b draws from
        Philox subsequence `clip_index0 + b` with b its position in the SUBMITTED list, whatever the sort does: the draws are what they
        would be had all clips had one length; `clip_indices` (B ints) names every clip's global index outright instead (a host that
        regroups clips between passes keeps each clip's random stream).  uniforms: list of (H_b,2) per clip for TS_SAMPLE_UNIFORMS.
        sampling: one sampling record (`_lib.sampling_record`: temperature, top_p, top_k) for all clips, or a list of one per clip in
        SUBMISSION order; the records are carried through the length sort exactly as `clip_indices` are, and a clip's codes depend on its
        own record only (`ts_body_pixel_infer_mixed_ctl`).  A bad record raises ValueError naming the clip, before anything is launched.
        logprobs=True: every clip's tuple gains logprobs_b (H_b,2) float32 (`ts_body_pixel_infer_mixed_lp`), bit-identical to the clip alone.
        given: a list in SUBMISSION order with None or a (G_b,2) integer array per clip (or one (B,G,2) block), 0 <= G_b <= H_b: the clip's
        first G_b code rows are TAKEN from it, the rest produced as without it (`ts_body_pixel_infer_mixed_given`; the MFCC rows are the
        clip's whole audio).  The entries are carried through the length sort exactly as the sampling records and `clip_indices` are.  Given
        the first rows of an earlier decode of the clip (same seed, index and record) the pass returns that decode bit for bit; a given
        row's log-probability is that of its code under the distribution it would have been drawn from (-inf for a code the record's
        filters remove).  A bad shape, G_b > H_b or a code outside [0, V) raises ValueError naming the clip before anything is launched.
        given_poses: the same from MOTION — a list in submission order with None or a (P_b,129) float array per clip (or one (B,P,129) block),
        P_b = 0 or 4 <= P_b with P_b // 4 <= H_b: the frames are encoded on the device (`ts_body_pixel_infer_mixed_poses`: both VQ encoders,
        length-masked, in front of the pass; no synchronisation, no host copy of codes) and the clip continues from its first P_b // 4 code
        rows, exactly as with `given=` set to `encode_clips`' codes of those frames.  The frames are in the wrapper's own pose layout: the
        129 c_index columns this method RETURNS (the VQ-VAEs' side; a caller who un-normalised or re-ordered its poses for display hands
        back the rows as they were before that).  A clip brings `given` or `given_poses`, never both (ValueError naming the clip); a pass may
        hold both kinds.  1 <= P_b <= 3, P_b // 4 > H_b or a wrong width raises ValueError naming the clip before anything is launched.
        given_keep: WHICH positions of a clip's given rows are taken (talkshow_hip.h, "kept positions"; `_lib.given_keep_block`) — a list in
        submission order with, per clip, None (all of them: the behaviour without the keyword), "body" (column 0, the body codebook, is
        kept and the hands are drawn), "hand" (column 1 kept, the body drawn) or a (G_b,2) bool / 0-1 array ((P_b // 4, 2) for a clip that
        brings poses: the mask applies to the codes the encoders produce); or one string or one (B,G,2) block for all clips.  Position
        (r, j) is taken iff r < G_b and its mask entry is 1; every other position is produced as if nothing were given there: its given code
        is never read (it may hold anything, so the vocabulary check covers kept positions only), it draws the Philox number of its absolute
        (row, column) — "keep this body take, draw N hand takes" is N entries with N clip indices — and its log-probability is a draw's.
        Handing back an earlier decode (same seed, index, record) with ANY mask returns that decode bit for bit.  Keeping the hands while
        drawing the body is a forced decode, not a posterior sample: the body draw at row r sees the hands of rows < r only.  Poses are the
        VQ decode of the returned codes.  A mask of the wrong shape, a non-0/1 array, an unknown string or an entry on a clip that brings
        nothing raises ValueError naming the clip before anything is launched (`ts_body_pixel_infer_mixed_keep` / `_poses_keep`).
        style: float SPEAKER WEIGHTS in place of the integer ids (talkshow_hip.h, "speaker style"; `_lib.style_block`) — a list in submission
        order with, per clip, None (the clip's id, that is, its one-hot row), an (NC,) row of weights for the whole clip (0.7 of speaker 0
        and 0.3 of speaker 2; 1.5 and -0.5 to exaggerate) or an (H_b,NC) track with one row per code row (4 pose frames: start as A, hand
        over to B across two seconds); or one (NC,) or (B,NC) array for all clips.  The class-conditioning vector of a code row is the
        weighted sum of the speakers' vectors (ascending, product and sum rounded to fp32 separately, zero weights skipped;
        `sampling.style_rows`): a blend is an INTERPOLATION OF THE CONDITIONING VECTORS — a virtual speaker between the trained ones — NOT
        a mixture of the speakers' distributions.  A one-hot row is the integer id bit for bit; weights are any finite floats.  Entries
        follow the clips through the length sort like the sampling records.  If no clip brings a track the pass is the pass of the ids with
        other conditioning rows (same graphs); otherwise per-clip rows are repeated into tracks and the pass stages every chunk's rows
        (graph keys of its own).  Orthogonal to every other keyword; given rows run under the style too, so handing back the head of an
        earlier decode WITH THE SAME STYLE returns that decode.  A wrong shape, a wrong NC or a non-finite weight raises ValueError naming
        the clip before anything is launched (`ts_body_pixel_infer_mixed_style` / `_poses_style`).  None: nothing changes.
        code_bias: WHICH CODES A CLIP MAY USE, and how likely (talkshow_hip.h, "code bias"; `_lib.code_bias_block`) — one (2, V) float
        table for all clips, or a list in submission order with, per clip, None (the clip's bits do not move), a (2, V) table or a dict
        {"body": (V,), "hand": (V,)} (a missing key: zeros).  Row 0 is added to the logits of the body column and row 1 to those of the
        hand column, ahead of temperature / top-k / top-p (one fp32 addition; `sampling.biased`); -inf BANS a code: it is never drawn.
        `sampling.allow_bias(codes, V)` makes the allow-list of the codes in an (n, 2) array — `code_bias_from_motion(poses)` that of
        example motion ("stay inside the vocabulary of this seated speaker") —, `sampling.ban_bias` its complement.  Entries that are the
        same object travel once.  Log-probabilities are those of the biased, filtered distribution.  Given rows are taken whatever the
        table says (a banned given code gets -inf).  TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only (per-clip greedy is top_k = 1); a clip's
        random numbers do not depend on its table.  Orthogonal to every other keyword.  A wrong shape, a NaN, a +inf, a value beyond
        1e30 or a column without an allowed code raises ValueError naming the clip before anything is launched
        (`ts_body_pixel_infer_mixed_bias` / `_poses_bias`).  None: nothing changes.
        repeat: NOT THIS CODE AGAIN SO SOON (talkshow_hip.h, "repetition penalty"; `_lib.repeat_table`) — one record (window, presence,
        frequency), a dict with those keys or None for all clips, or a list in submission order with one such entry per clip (a single
        record is never written as a list).  At code row r a code the clip produced c > 0 times in the last `window` <= 64 rows of the
        SAME column loses presence + frequency * c ahead of temperature / top-k / top-p (`sampling.penalised`); drawn, given and kept codes
        count alike; body and hand columns have separate histories.  presence = 1e30 is "no repeat within the window"; negative values
        favour what was just produced ("hold the pose").  window 0: the clip's bits do not move.  Log-probabilities are those of the
        penalised, biased, filtered distribution; given rows are taken as before and enter the history, so handing back the head of a
        decode WITH THE SAME RECORD returns that decode.  TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only; a clip's random numbers do not depend
        on its record.  Orthogonal to every other keyword.  A window outside [0, 64], a NaN, an infinity or a value beyond 1e30 raises
        ValueError naming the clip before anything is launched (`ts_body_pixel_infer_mixed_repeat` / `_poses_repeat`).  None: nothing
        changes.
        guide: MORE OF THIS, LESS OF THAT (talkshow_hip.h, "guidance"; `_lib.guide_entries`) — one dict for all clips, or a list in submission
        order with, per clip, None or a dict {"scale": s, "mfcc": (T_b, 64) array or None, "id": int or None, "style": row / track or
        None}; an absent audio, id or style is the clip's own.  The clip is decoded under its own conditioning p; a SHADOW slot placed
        directly behind it runs the same code history under the second conditioning q (other audio, another speaker), and at every
        position the clip's logits become l' = l + scale * (l - l_q) — difference, product and sum rounded to fp32 separately
        (`sampling.guided`) — AHEAD of code bias, repetition penalty, temperature, top-k and top-p; log-probabilities are those of the
        guided distribution.  scale > 0: more driven by this audio than by q's (silence, say), "more speaker A, less speaker B";
        scale = -0.5: the geometric mean of the two distributions — the MIXTURE OF DISTRIBUTIONS `style=` is not; scale = 0: the clip's
        bits do not move; a shadow with the clip's own conditioning changes nothing for any scale.  The shadow draws nothing, consumes no
        random number and shifts no clip's index; given, kept and forced positions are the clip's own and are written to both slots;
        every other keyword's entry follows the clip, shadows bring none.  A guided clip costs a second slot of the pass; the caller
        gets B results.  TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only.  A wrong key, shape, length or scale (NaN, infinite, beyond 1e4)
        raises ValueError naming the clip before anything is launched (`ts_body_pixel_infer_guided` / `ts_body_pixel_infer_guided_poses`).  None:
        nothing changes.
        alternatives: WHAT ELSE, AND HOW SURE (talkshow_hip.h, "alternatives") — n in [0, 8]: every clip's tuple gains, behind the
        log-probabilities where those are asked for, a `sampling.Alternatives` with codes int64 (H_b,2,n) and logprobs float32 (H_b,2,n) of
        the n likeliest allowed codes of every position, entropy float32 (H_b,2) and rank int64 (H_b,2) of the position's own code (drawn,
        given or kept; -1 for a given code outside the vocabulary) — all under the distribution the filters are applied to: code bias,
        repetition penalty and temperature applied, top-k and top-p not, so a top_k = 1 decode still reports them.  Written by the sampler
        launch itself; codes, poses and log-probabilities are those of the call without the keyword, bit for bit, and a clip's values are
        bit-identical to the clip alone.  `sampling.uncertain_keep(alt.entropy, threshold)` is a `given_keep=` mask: hand the codes back
        with it to keep what the model was sure of and redraw the rest.  TS_SAMPLE_UNIFORMS / TS_SAMPLE_PHILOX only (ValueError: a greedy
        decode with alternatives is sampling=(1, 1, 1) under Philox); not with guide (NotImplementedError); n outside [0, 8] raises
        ValueError — all before anything is launched (`ts_body_pixel_infer_alt` / `ts_body_pixel_infer_alt_poses`).  None:
        nothing changes."""
        if not (logprobs is None or isinstance(logprobs, bool)):
            raise ValueError("generate_clips: logprobs is True or False")
        guided = guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide))
        an = _lib.alt_request(alternatives, mode, "generate_clips", guide=guided)
        dev = self.generator._dev()
        B = len(mfcc_list)
        if B < 1:
            raise ValueError("generate_clips: no clips")
        clips = [torch.as_tensor(m, dtype=torch.float32, device=dev) for m in mfcc_list]
        lens = [int(m.shape[0]) for m in clips]
        for b, (m, t) in enumerate(zip(clips, lens)):
            if m.dim() != 2 or m.shape[1] != 64:
                raise ValueError(f"generate_clips: clip {b} must have shape (T, 64), got {tuple(m.shape)}")
            if t < 4:
                raise ValueError(f"generate_clips: clip {b} has {t} MFCC rows; one code row needs 4")
        if _ids_checked:
            ids = torch.as_tensor(ids, dtype=torch.int64, device=dev).reshape(-1)
        else:
            ids = _index_tensor(ids, self.num_classes, 'speaker id', dev)
        if ids.numel() == 1 and B > 1:
            ids = ids.repeat(B)
        if ids.numel() != B:
            raise ValueError(f"ids must hold 1 or B={B} speaker indices, got {ids.numel()}")
        order, inverse = mixed_pass_order(lens)
        ctl, n_ctl = None, 0
        if sampling is not None:   # sorted slot k holds the record of submitted clip order[k]
            recs = _lib.sampling_records(sampling, B)
            ctl, n_ctl = _lib.sampling_table([recs[i] for i in order], B, self.generator.input_dim, mode)
        gblock = gtable = kblock = None
        if given_keep is not None:   # the mask of kept positions, in slot order like the blocks it selects from
            kblock = _lib.given_keep_block(given_keep, _lib.given_counts(given, given_poses, B), [t // 4 for t in lens], order, who="generate_clips")
        if given is not None:      # sorted slot k holds the given rows of submitted clip order[k]; validated before anything is launched
            gblock, gtable = _lib.given_block(given, [t // 4 for t in lens], self.generator.input_dim, order, who="generate_clips", keep=kblock)
        pblock = ptable = None
        if given_poses is not None:
            _lib.given_kinds_check(given, given_poses, B, "generate_clips")
            pblock, ptable = _lib.given_pose_block(given_poses, [t // 4 for t in lens], order, who="generate_clips",
                                                   width=self.each_dim[1] + self.each_dim[2])
            if int(ptable.max()) == 0:      # nothing given anywhere: the pass without the keyword
                pblock = ptable = None
        if gblock is None and pblock is None:
            kblock = None
        sblock = _lib.style_block(style, [t // 4 for t in lens], self.num_classes, order, who="generate_clips", ids=ids)   # slot order, like the records
        btab, bidx = _lib.code_bias_block(code_bias, B, self.generator.input_dim, order, who="generate_clips", mode=mode)   # slot order, too
        rtab, n_rep = _lib.repeat_table(repeat, B, self.generator.input_dim, order, who="generate_clips", mode=mode)                # and the records
        gent = _lib.guide_entries(guide, B, who="generate_clips", audio_key="mfcc", mode=mode, n_classes=self.num_classes, rows=[t // 4 for t in lens])
        for b, e in enumerate(gent or ()):
            if e is not None and e["audio"] is not None and tuple(np.shape(e["audio"])) != (lens[b], 64):
                raise ValueError(f"generate_clips: guide of clip {b}: mfcc must have the clip's own shape ({lens[b]}, 64), got {tuple(np.shape(e['audio']))}")
        T_max = lens[order[0]]
        H_max = T_max // 4
        sorted_lens = [lens[i] for i in order]
        mf = torch.zeros((B, T_max, 64), dtype=torch.float32, device=dev)
        for k, i in enumerate(order):
            mf[k, :lens[i]] = clips[i]
        lens_host = np.asarray(sorted_lens, dtype=np.int32)
        lens_dev = torch.from_numpy(lens_host).to(dev)
        order_dev = torch.as_tensor(order, dtype=torch.int64, device=dev)
        ids_sorted = ids.index_select(0, order_dev).contiguous()
        if clip_indices is None:
            clip_index = (order_dev + int(clip_index0)).contiguous()      # global index of the clip in each sorted slot
        else:
            if len(clip_indices) != B:
                raise ValueError(f"generate_clips: clip_indices must name {B} clips, got {len(clip_indices)}")
            clip_index = torch.as_tensor([int(clip_indices[i]) for i in order], dtype=torch.int64, device=dev)
        u = None
        if mode == _lib.TS_SAMPLE_UNIFORMS:
            if uniforms is None or len(uniforms) != B:
                raise ValueError("generate_clips: TS_SAMPLE_UNIFORMS needs one (H_b, 2) array of uniforms per clip")
            u = torch.zeros((B, H_max, 2), dtype=torch.float32, device=dev)
            for k, i in enumerate(order):
                ui = torch.as_tensor(uniforms[i], dtype=torch.float32, device=dev)
                if tuple(ui.shape) != (lens[i] // 4, 2):
                    raise ValueError(f"generate_clips: uniforms of clip {i} must have shape ({lens[i] // 4}, 2), got {tuple(ui.shape)}")
                u[k, :lens[i] // 4] = ui
        if seed is None:
            seed = _fresh_seed() if mode == _lib.TS_SAMPLE_PHILOX else 0
        Bp, gpair, prim = B, (None, None), None      # the slots of the pass: B, or B plus one shadow behind every guided clip
        if gent is not None:
            # every validated block is in slot order: slot s of the guided pass copies original slot src[s]; a shadow then takes its own
            # audio, id and style and brings no given rows, no poses and no table
            src, shadow, gtab, gscale = _lib.guide_layout(order, gent)
            slot_ent = [gent[i] for i in order]
            Bp, sidx, shadows = len(src), np.asarray(src, np.int64), np.asarray(shadow, bool)
            sdev = torch.as_tensor(sidx, device=dev)
            mf, ids_sorted, clip_index = mf.index_select(0, sdev).contiguous(), ids_sorted.index_select(0, sdev).contiguous(), clip_index.index_select(0, sdev).contiguous()
            u = None if u is None else u.index_select(0, sdev).contiguous()
            for s in np.flatnonzero(shadows):
                e, t = slot_ent[src[s]], sorted_lens[src[s]]
                if e["audio"] is not None:
                    mf[s, :t] = torch.as_tensor(e["audio"], dtype=torch.float32, device=dev)
                if e["id"] is not None:
                    ids_sorted[s] = e["id"]
            need_ids = sblock is None and any(e is not None and e["style"] is not None for e in gent)
            sblock = _lib.guide_style_block(sblock, src, shadow, slot_ent, [t // 4 for t in sorted_lens], self.num_classes,
                                            ids.index_select(0, order_dev).cpu().numpy() if need_ids else None, who="generate_clips", names=order)
            lens_host = np.ascontiguousarray(lens_host[sidx])
            lens_dev = torch.from_numpy(lens_host).to(dev)
            (ctl, n_ctl), (gblock, gtable), (pblock, ptable), kblock, (btab, bidx), (rtab, n_rep) = _lib.guide_expand(
                src, shadow, (ctl, n_ctl), (gblock, gtable), (pblock, ptable), kblock, (btab, bidx), (rtab, n_rep))
            gpair = (gtab, gscale)
            prim = torch.as_tensor(np.flatnonzero(~shadows).astype(np.int64), device=dev)
        codes = torch.empty((Bp, H_max, 2), dtype=torch.int64, device=dev)
        poses = torch.empty((Bp, 4 * H_max, self.each_dim[1] + self.each_dim[2]), dtype=torch.float32, device=dev)
        args = (self.audioencoder.handle(), self.generator.handle(), self.g_body.handle(), self.g_hand.handle(),
                _lib.dptr(mf), _lib.dptr(ids_sorted), lens_host.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(lens_dev), Bp, T_max,
                mode, _lib.dptr(u), int(seed) & (2 ** 64 - 1), _lib.dptr(clip_index), _lib.dptr(codes), _lib.dptr(poses))
        lp = torch.empty((Bp, H_max, 2), dtype=torch.float32, device=dev) if logprobs or an is not None else None   # the record needs one beside it
        areq = None if an is None else _lib.AltRequest(an, (Bp, H_max, 2), dev)
        self._mixed_call(args, dev, ctl=(ctl, n_ctl), lp=lp, given=(gblock, gtable), poses=(pblock, ptable), keep=kblock, style=sblock,
                         bias=(btab, bidx), repeat=(rtab, n_rep), guide=gpair, alt=areq)      # the most general entry of the family; absent keywords travel as NULL
        if not logprobs:
            lp = None
        if prim is not None:      # the shadows' rows are their primaries': the caller sees B results
            codes, poses = codes.index_select(0, prim), poses.index_select(0, prim)
            lp = None if lp is None else lp.index_select(0, prim)
        inv_dev = torch.as_tensor(inverse, dtype=torch.int64, device=dev)
        codes, poses = codes.index_select(0, inv_dev), poses.index_select(0, inv_dev)     # back to submission order
        if areq is not None:      # the keyword's own return value, behind the log-probabilities; sliced per clip where the call returns per clip
            from talkshow_amd import sampling as S
            alt = areq.result(inv_dev)
            lp = None if lp is None else lp.index_select(0, inv_dev)
            if _stacked:
                return (codes, poses) + (() if lp is None else (lp,)) + (alt,)
            return [(codes[b, :lens[b] // 4], poses[b, :4 * (lens[b] // 4)]) + (() if lp is None else (lp[b, :lens[b] // 4],)) +
                    (S.Alternatives(*(x[b, :lens[b] // 4] for x in alt)),) for b in range(B)]
        if lp is not None:
            lp = lp.index_select(0, inv_dev)
            if _stacked:
                return codes, poses, lp
            return [(codes[b, :lens[b] // 4], poses[b, :4 * (lens[b] // 4)], lp[b, :lens[b] // 4]) for b in range(B)]
        if _stacked:
            return codes, poses
        return [(codes[b, :lens[b] // 4], poses[b, :4 * (lens[b] // 4)]) for b in range(B)]

    def _mixed_call(self, args, dev, ctl=(None, 0), lp=None, given=(None, None), poses=(None, None), keep=None, style=None, bias=(None, None),
                    repeat=(None, 0), guide=(None, None), alt=None):
        """Uploads the host blocks of a mixed pass, each once, and makes its one call (`_lib.body_mixed_call`): args the fixed arguments,
        the rest validated blocks (pairs: block and table) in slot order or None.  Given poses beside given codes are staged into one block."""
        from talkshow_amd.modules import upload
        i32p = _lib.C.POINTER(_lib.C.c_int32)
        (gblock, gtable), (pblock, ptable), (btab, bidx) = given, poses, bias
        gdev = pose_piece = None
        if gblock is not None and pblock is not None:    # both kinds in one pass: the pose clips' codes join the code clips' in one block, on the device
            gdev, gtable = self._stage_given(gblock, gtable, pblock, ptable, dev)
        elif gblock is not None:
            gdev = upload(gblock, dev)
        elif pblock is not None:
            pdev, tdev = (pblock if torch.is_tensor(pblock) else upload(pblock, dev)), upload(ptable, dev)   # both alive until the call is queued
            pose_piece = (_lib.dptr(pdev), int(pdev.shape[1]), ptable.ctypes.data_as(i32p), _lib.dptr(tdev))
        kdev, sdev, bdev = (None if block is None else upload(block, dev) for block in (keep, style, btab))
        _lib.body_mixed_call(
            args, ctl=ctl[0], n_ctl=ctl[1], logprob=_lib.dptr(lp), given=_lib.dptr(gdev), given_rows=None if gdev is None else gtable.ctypes.data_as(i32p),
            poses=pose_piece, keep=_lib.dptr(kdev), style=_lib.dptr(sdev), style_rows=0 if style is None else int(style.shape[1]),
            bias=_lib.dptr(bdev), n_bias=0 if btab is None else int(btab.shape[0]), bias_index=None if btab is None else bidx.ctypes.data_as(i32p),
            rep=repeat[0], n_rep=repeat[1], guide=None if guide[0] is None else guide[0].ctypes.data_as(i32p), guide_scale=_lib.fptr(guide[1]),
            alt=None if alt is None else alt.ptr())

    def _stage_given(self, gblock, gtable, pblock, ptable, dev):
        """One given block for a pass that holds code clips AND pose clips: gblock / gtable from `_lib.given_block`, pblock / ptable from
        `_lib.given_pose_block` (slot order; no clip is in both) -> ((B,H_max,2) int64 device block, (B,) int32 host table).  The pose
        clips are encoded on the device (`ts_vqvae_encode_pair_masked`, the kernels `ts_body_pixel_infer_mixed_poses` runs) and their rows
        selected into the uploaded code block there: nothing is read back."""
        from talkshow_amd.modules import encode_pair_masked, upload
        pdev = pblock if torch.is_tensor(pblock) else upload(pblock, dev)
        gdev = upload(gblock, dev)
        enc = encode_pair_masked(self.g_body, self.g_hand, pdev, upload(ptable, dev))          # (B, P_max // 4, 2), -1 beyond a clip's rows
        Hp = min(int(enc.shape[1]), int(gdev.shape[1]))
        from_poses = upload(np.ascontiguousarray(ptable > 0), dev)[:, None, None]
        gdev[:, :Hp] = torch.where(from_poses, enc[:, :Hp], gdev[:, :Hp])
        return gdev, np.ascontiguousarray(gtable + ptable // 4, dtype=np.int32)

    def _score_pass(self, mfcc_list, ids, who, make_given, style=None):
        """The shared body of `score_clips` / `score_motion_clips`: the masked audio encoder, `ts_pixelcnn_generate_mixed_given` with every
        row given (G_b = H_b: nothing is drawn) and the log-probability output, `ts_logprob_sums` with the length table."""
        from talkshow_amd.modules import upload
        dev = self.generator._dev()
        B = len(mfcc_list)
        if B < 1:
            raise ValueError(f"{who}: no clips")
        clips = [torch.as_tensor(m, dtype=torch.float32, device=dev) for m in mfcc_list]
        lens = [int(m.shape[0]) for m in clips]
        for b, (m, t) in enumerate(zip(clips, lens)):
            if m.dim() != 2 or m.shape[1] != 64:
                raise ValueError(f"{who}: clip {b} must have shape (T, 64), got {tuple(m.shape)}")
            if t < 4:
                raise ValueError(f"{who}: clip {b} has {t} MFCC rows; one code row needs 4")
        order, inverse = mixed_pass_order(lens)
        rows = [t // 4 for t in lens]
        given = make_given(rows, order, dev)               # validated on the host before anything is launched; (B,H_max,2) device block
        ids = _index_tensor(ids, self.num_classes, 'speaker id', dev)
        if ids.numel() == 1 and B > 1:
            ids = ids.repeat(B)
        if ids.numel() != B:
            raise ValueError(f"ids must hold 1 or B={B} speaker indices, got {ids.numel()}")
        sblock = _lib.style_block(style, rows, self.num_classes, order, who=who, ids=ids)   # before anything is launched, too
        T_max, H_max = lens[order[0]], lens[order[0]] // 4
        mf = torch.zeros((B, T_max, 64), dtype=torch.float32, device=dev)
        for k, i in enumerate(order):
            mf[k, :lens[i]] = clips[i]
        lens_host = np.asarray([lens[i] for i in order], dtype=np.int32)
        table = np.asarray([rows[i] for i in order], dtype=np.int32)
        lens_dev = upload(lens_host, dev)
        ids_sorted = ids.index_select(0, torch.as_tensor(order, dtype=torch.int64, device=dev)).contiguous()
        feat = torch.empty((B, H_max, self.audioencoder.num_hiddens), dtype=torch.float32, device=dev)
        codes = torch.empty((B, H_max, 2), dtype=torch.int64, device=dev)
        lp = torch.empty((B, H_max, 2), dtype=torch.float32, device=dev)
        sums = torch.empty((B, 3), dtype=torch.float64, device=dev)
        lib, i32p = _lib.load(), _lib.C.POINTER(_lib.C.c_int32)
        _lib.check(lib.ts_audioenc_forward_masked(self.audioencoder.handle(), _lib.dptr(mf), _lib.dptr(lens_dev), B, T_max, _lib.dptr(feat),
                                                  _lib.stream_ptr()))
        fixed = (self.generator.handle(), _lib.dptr(ids_sorted), _lib.dptr(feat), lens_host.ctypes.data_as(i32p), _lib.dptr(lens_dev), B, H_max,
                 _lib.TS_SAMPLE_GREEDY, None, 0, None, _lib.dptr(codes))
        sdev = upload(sblock, dev) if sblock is not None else None
        _lib.pixelcnn_mixed_call(fixed, logprob=_lib.dptr(lp), given=_lib.dptr(given), given_rows=table.ctypes.data_as(i32p),
                                 style=_lib.dptr(sdev), style_rows=0 if sblock is None else int(sblock.shape[1]))
        _lib.check(lib.ts_logprob_sums(self.generator._ctx(), _lib.dptr(lp), _lib.dptr(lens_dev), B, H_max, _lib.dptr(sums), _lib.stream_ptr()))
        return [(lp[inverse[b], :rows[b]], sums[inverse[b]]) for b in range(B)]

    def score_clips(self, mfcc_list, ids, codes_list, style=None):
        """`score_batch` for clips of DIFFERENT lengths in ONE pass: mfcc_list = list of (T_b,64), ids (B,) or one for all, codes_list = list
        of (T_b // 4, 2) integer arrays -> list of (logprobs_b (H_b,2) float32, sums_b (3,) float64 {body, hand, both}) in submission order,
        each bit-identical to `score_batch` on the clip alone.  A wrong shape or a code outside [0, V) raises ValueError naming the clip.
        style: the clips' speaker weights as for `generate_clips` (None, an (NC,) row or an (H_b,NC) track per clip, or one array for all):
        the codes are scored under that style — the log-probabilities a decode with the same style returned."""
        from talkshow_amd.modules import upload

        def make(rows, order, dev):
            if not isinstance(codes_list, (list, tuple)) or len(codes_list) != len(rows):
                raise ValueError(f"score_clips: one (H_b, 2) code array per clip ({len(rows)})")
            for b, c in enumerate(codes_list):
                if c is None or tuple(c.shape) != (rows[b], 2):
                    raise ValueError(f"score_clips: codes of clip {b} must have shape ({rows[b]}, 2), got {None if c is None else tuple(c.shape)}")
            block, _ = _lib.given_block(list(codes_list), rows, self.generator.input_dim, order, who="score_clips")
            return upload(block, dev)
        return self._score_pass(mfcc_list, ids, "score_clips", make, style=style)

    def score_motion_clips(self, mfcc_list, ids, poses_list, style=None):
        """How likely is this recorded MOTION under the model: `score_clips` on the codes the VQ encoders give the poses, encoded on the
        device in the same pass (`ts_vqvae_encode_pair_masked` in front of it; no host copy of codes).  poses_list = list of (P_b,129)
        arrays in the wrapper's own pose layout (see `generate_clips`) with P_b = 4 (T_b // 4) frames: ValueError naming the clip otherwise.
        style: as for `score_clips`; the encoders never see a speaker, the style shapes the scoring pass only."""
        from talkshow_amd.modules import encode_pair_masked, upload

        def make(rows, order, dev):
            if not isinstance(poses_list, (list, tuple)) or len(poses_list) != len(rows):
                raise ValueError(f"score_motion_clips: one (P_b, 129) pose array per clip ({len(rows)})")
            for b, g in enumerate(poses_list):
                P = None if g is None or len(getattr(g, "shape", ())) != 2 else int(g.shape[0])
                if P != 4 * rows[b]:
                    raise ValueError(f"score_motion_clips: clip {b} has {rows[b]} code rows and needs {4 * rows[b]} pose frames, got "
                                     f"{None if g is None else tuple(getattr(g, 'shape', ()))}")
            pblock, ptable = _lib.given_pose_block(list(poses_list), rows, order, who="score_motion_clips",
                                                   width=self.each_dim[1] + self.each_dim[2])
            pdev = pblock if torch.is_tensor(pblock) else upload(pblock, dev)
            return encode_pair_masked(self.g_body, self.g_hand, pdev, upload(ptable, dev))     # (B, H_max, 2): P_max = 4 H_max
        return self._score_pass(mfcc_list, ids, "score_motion_clips", make, style=style)

    def code_bias_from_motion(self, poses_list):
        """The ALLOW-LIST of example motion: poses_list = list of (P_b, 129) pose clips in the wrapper's own pose layout (see
        `generate_clips`; P_b >= 4) -> a (2, V) float32 table, 0 for every body / hand code the clips encode to and -inf for every other:
        `code_bias=` of the decode entries ("stay inside the vocabulary of this reference motion").  One `ts_vqvae_encode_pair_masked` pass
        on the device — the route `given_poses` takes — then `sampling.allow_bias` on the host (this call reads the codes back)."""
        from talkshow_amd import sampling as S
        from talkshow_amd.modules import encode_pair_masked, pad_pose_clips, upload
        dev = self.generator._dev()
        block, lens = pad_pose_clips(list(poses_list), dev, "code_bias_from_motion", self.each_dim[1] + self.each_dim[2])
        codes = encode_pair_masked(self.g_body, self.g_hand, block, upload(lens, dev)).cpu().numpy()      # -1 beyond a clip's own rows
        return S.allow_bias(codes.reshape(-1, 2), self.generator.input_dim)

    def infer_padded_wav(self, wav, ns_host, ns_dev, sr, ids, clip_index, mode, seed, fps=30, lens_dev=None, sampling_table=None, given=None,
                         given_poses=None, given_keep=None, style=None, code_bias=None, repeat=None, guide=None, alternatives=None):
        """The device part of a pass over recordings: wav (B,N_max) padded device block whose rows are ordered longest first, ns_host / ns_dev
        their sample counts (int32, host and device), ids / clip_index (B,) int64 device tensors in row order -> codes (B,H_max,2) with -1
        and poses (B,4 H_max,129) with 0 beyond a clip's own rows.  The mixed MFCC front-end feeds the mixed body pass on the device; the body
        pass's host table is `mixed_tables` arithmetic (lens_dev: its device copy, (B,) int32, if the caller has uploaded one).  No synchronisation.
        sampling_table: `_lib.sampling_table(...)` in ROW order (the caller sorted it with the rows), or None.
        given: `_lib.given_block(...)` in ROW order — (block, table), both numpy — or None.
        given_poses: `_lib.given_pose_block(...)` in ROW order — (block, table) — or None; with `given` too, no clip is in both.
        given_keep: `_lib.given_keep_block(...)` in ROW order — the (B, H_max, 2) uint8 mask of kept positions — or None.
        style: `_lib.style_block(...)` in ROW order — the (B, 1 or H_max, NC) float32 speaker weights that take the place of `ids` — or None.
        code_bias: `_lib.code_bias_block(...)` in ROW order — (tables (NB, 2, V) float32, index (B,) int32), both numpy — or None.
        repeat: `_lib.repeat_table(...)` in ROW order — (records, B) — or None.
        guide: (guide (B,) int32, scale (B,) float32) numpy tables in ROW order — the shadow's row of every row or -1, and the scales
        (talkshow_hip.h, "guidance") — or None.  A shadow is a row of `wav` like any other.
        alternatives: n in [0, 8] (talkshow_hip.h, "alternatives") -> a fourth return value, a `sampling.Alternatives` over the (B,H_max,2)
        positions in ROW order; a drawing mode only, not with guide.  None: three return values and the launches there always were."""
        from talkshow_amd.frontend import device_mfcc, mixed_tables
        an = _lib.alt_request(alternatives, mode, "infer_padded_wav", guide=guide is not None)      # before anything is launched
        from talkshow_amd.modules import upload
        dev = self.generator._dev()
        rows = mixed_tables(ns_host, sr, 22000, fps)["mfcc_rows"]
        if int(rows.min()) < 4:
            raise ValueError(f"clip of {int(ns_host[int(np.argmin(rows))])} samples gives {int(rows.min())} MFCC rows; one code row needs 4")
        lens_host = np.ascontiguousarray(rows, dtype=np.int32)
        if lens_dev is None:
            lens_dev = upload(lens_host, dev)
        if guide is not None:
            _lib.guide_check(guide[0], guide[1], lens_host)      # ValueError naming the row, before anything is launched
        mf = device_mfcc(sr, 22000, fps).forward_padded(wav, ns_host, ns_dev)
        B, T_max = mf.shape[0], mf.shape[1]
        H_max = T_max // 4
        codes = torch.empty((B, H_max, 2), dtype=torch.int64, device=dev)
        poses = torch.empty((B, 4 * H_max, self.each_dim[1] + self.each_dim[2]), dtype=torch.float32, device=dev)
        args = (self.audioencoder.handle(), self.generator.handle(), self.g_body.handle(), self.g_hand.handle(),
                _lib.dptr(mf), _lib.dptr(ids), lens_host.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), _lib.dptr(lens_dev), B, T_max,
                mode, None, int(seed) & (2 ** 64 - 1), _lib.dptr(clip_index), _lib.dptr(codes), _lib.dptr(poses))
        if given_poses is not None and int(given_poses[1].max()) == 0:
            given_poses = None
        if given is None and given_poses is None:
            given_keep = None
        if given_keep is not None and given_keep.shape != (B, H_max, 2):
            raise ValueError(f"infer_padded_wav: the mask of kept positions must be (B, H_max, 2) = ({B}, {H_max}, 2), got {given_keep.shape}")
        if style is not None:
            if style.ndim != 3 or style.shape[0] != B or style.shape[1] not in (1, H_max):
                raise ValueError(f"infer_padded_wav: the style block must be (B, 1 or H_max, NC) = ({B}, 1 or {H_max}, NC), got {style.shape}")
            style = np.ascontiguousarray(style, dtype=np.float32)
        btab, bidx = code_bias if code_bias is not None else (None, None)
        if btab is not None:
            V = self.generator.input_dim
            if btab.ndim != 3 or btab.shape[1:] != (2, V) or btab.dtype != np.float32 or bidx.shape != (B,) or bidx.dtype != np.int32:
                raise ValueError(f"infer_padded_wav: the code bias is (tables (NB, 2, {V}) float32, index ({B},) int32), got "
                                 f"{btab.dtype} {btab.shape} and {bidx.dtype} {bidx.shape}")
            bidx = np.ascontiguousarray(bidx)
        rtab, n_rep = repeat if repeat is not None and repeat[0] is not None else (None, 0)
        if rtab is not None and n_rep != B:
            raise ValueError(f"infer_padded_wav: the repetition records are one per row ({B}), got {n_rep}")
        gblock, gtable = given if given is not None else (None, None)
        if gblock is not None and gblock.shape != (B, H_max, 2):
            raise ValueError(f"infer_padded_wav: the given block must be (B, H_max, 2) = ({B}, {H_max}, 2), got {gblock.shape}")
        pblock, ptable = given_poses if given_poses is not None else (None, None)
        if pblock is not None and int(pblock.shape[1]) // 4 > H_max:
            raise ValueError(f"infer_padded_wav: the given poses hold {int(pblock.shape[1])} frames but the pass has {H_max} code rows")
        areq = None if an is None else _lib.AltRequest(an, (B, H_max, 2), dev)
        lp = None if areq is None else torch.empty((B, H_max, 2), dtype=torch.float32, device=dev)      # the record needs one beside it
        self._mixed_call(args, dev, ctl=sampling_table or (None, 0), lp=lp, given=(gblock, gtable), poses=(pblock, ptable), keep=given_keep, style=style,
                         bias=(btab, bidx), repeat=(rtab, int(n_rep)), guide=guide or (None, None), alt=areq)
        if areq is not None:
            return codes, poses, lens_host, areq.result()
        return codes, poses, lens_host

    def guide_wav_rows(self, gent, order, wav, ns_host, ids, clip_index, sr, fps, pieces, who):
        """The rows of a GUIDED pass over recordings: gent = `_lib.guide_entries(..., audio_key="wav")` in submission order, order the sort
        of the pass, wav / ns_host / ids / clip_index the padded block and its tables in ROW order, pieces = `infer_padded_wav`'s
        keywords (validated blocks in row order) -> (wav, ns_host, ns_dev, ids, clip_index, pieces, prim): every shadow is a row directly
        behind its primary, with its own samples, id and style and its primary's sample count; it brings no given rows, no poses and no
        table; pieces gains `guide`; prim (numpy) are the rows of the clips themselves, in their old order."""
        from talkshow_amd.frontend import mixed_tables
        from talkshow_amd.modules import upload
        dev = wav.device
        src, shadow, gtab, gscale = _lib.guide_layout(order, gent)
        slot_ent = [gent[i] for i in order]
        sidx, shadows = np.asarray(src, np.int64), np.asarray(shadow, bool)
        sdev = torch.as_tensor(sidx, device=dev)
        rows_slot = [int(t) // 4 for t in mixed_tables(ns_host, sr, 22000, fps)["mfcc_rows"]]
        style = pieces.get("style")
        need_ids = style is None and any(e is not None and e["style"] is not None for e in gent)
        style = _lib.guide_style_block(style, src, shadow, slot_ent, rows_slot, self.num_classes, ids.cpu().numpy() if need_ids else None,
                                       who=who, names=order)
        wav, ids, clip_index = wav.index_select(0, sdev).contiguous(), ids.index_select(0, sdev).contiguous(), clip_index.index_select(0, sdev).contiguous()
        for s in np.flatnonzero(shadows):
            e = slot_ent[src[s]]
            if e["audio"] is not None:
                wav[s, :int(ns_host[src[s]])] = torch.as_tensor(e["audio"], dtype=wav.dtype, device=dev)
            if e["id"] is not None:
                ids[s] = e["id"]
        ns_host = np.ascontiguousarray(ns_host[sidx])
        table, given, given_poses, keep, code_bias, repeat = _lib.guide_expand(
            src, shadow, pieces.get("sampling_table") or (None, 0), pieces.get("given") or (None, None), pieces.get("given_poses") or (None, None),
            pieces.get("given_keep"), pieces.get("code_bias") or (None, None), pieces.get("repeat") or (None, 0))
        out = dict(sampling_table=table if table[0] is not None else None, given=given if given[0] is not None else None,
                   given_poses=given_poses if given_poses[0] is not None else None, given_keep=keep, style=style,
                   code_bias=code_bias if code_bias[0] is not None else None, repeat=repeat if repeat[0] is not None else None,
                   guide=(gtab, gscale))
        return wav, ns_host, upload(ns_host, dev), ids, clip_index, out, np.flatnonzero(~shadows)

    def generate_clips_from_wav(self, wavs, sr, ids, mode=_lib.TS_SAMPLE_PHILOX, seed=None, clip_index0=0, clip_indices=None, fps=30,
                                sampling=None, given=None, given_poses=None, given_keep=None, style=None, code_bias=None, repeat=None, guide=None,
                                alternatives=None):
        """`generate_clips` from RECORDINGS: wavs = list of (N_b,) sample arrays / tensors at `sr`, ids (B,) or one id for all -> list of
        (codes_b (H_b,2), poses_b (4 H_b,129)) in submission order.  The mixed MFCC front-end and the mixed body pass run back to back on the
        device: the MFCC rows never leave it and nothing synchronises.  A clip's result is bit-identical to
        `generate_batch(MFCC(sr)(wav_b), id_b)` on the clip alone; clip b draws from Philox subsequence `clip_index0 + b`, b its position in
        the SUBMITTED list (or `clip_indices[b]`).  sampling: one sampling record for all recordings or one per recording in submission
        order; the records follow the recordings through the sort by sample count.  given: as for `generate_clips`, one entry per recording
        in submission order (a recording's code rows: `frontend.mixed_tables(ns, sr)["code_rows"]`).  given_poses: as for `generate_clips`,
        one entry per recording.  given_keep: as for `generate_clips` — which positions of a recording's given rows are taken (None, "body",
        "hand", a mask; one entry per recording, or one for all).  style: as for `generate_clips` — float speaker weights in place of the
        ids, per recording None, an (NC,) row or an (H_b,NC) track (H_b the recording's code rows), or one array for all.  code_bias: as for
        `generate_clips` — which codes a recording may use: one (2, V) table for all, or per recording None, a table or a dict.  repeat:
        as for `generate_clips` — a repetition penalty over a window of earlier codes: one record for all, or a list with one per recording.
        guide: as for `generate_clips` — guidance against a second conditioning, whose audio is given as "wav": (N_b,) samples at `sr`,
        the recording's own sample count (None: the recording's own audio); one dict for all, or a list with None or a dict per recording.
        alternatives: as for `generate_clips` — n in [0, 8]: every recording's tuple gains a `sampling.Alternatives` over its (H_b,2)
        positions; a drawing mode only, not with guide."""
        from talkshow_amd.frontend import check_recordings, mixed_tables
        guided = guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide))
        an = _lib.alt_request(alternatives, mode, "generate_clips_from_wav", guide=guided)      # before anything is launched
        from talkshow_amd.modules import ids_in_row_order, pad_recordings, upload
        ns = check_recordings(wavs, "generate_clips_from_wav")
        B = len(ns)
        n_ids = int(ids.numel()) if torch.is_tensor(ids) else int(np.asarray(ids).size)
        if n_ids not in (1, B):
            raise ValueError(f"ids must hold 1 or B={B} speaker indices, got {n_ids}")
        if clip_indices is not None and len(clip_indices) != B:
            raise ValueError(f"generate_clips_from_wav: clip_indices must name {B} clips, got {len(clip_indices)}")
        dev = self.generator._dev()
        order, inverse = mixed_pass_order(ns)
        table = None
        if sampling is not None:
            recs = _lib.sampling_records(sampling, B)
            table = _lib.sampling_table([recs[i] for i in order], B, self.generator.input_dim, mode)
        given_in = given
        if given_keep is not None:
            given_keep = _lib.given_keep_block(given_keep, _lib.given_counts(given, given_poses, B),
                                               [int(t) // 4 for t in mixed_tables(ns, sr, 22000, fps)["mfcc_rows"]], order, who="generate_clips_from_wav")
        if given is not None:
            given = _lib.given_block(given, [int(t) // 4 for t in mixed_tables(ns, sr, 22000, fps)["mfcc_rows"]], self.generator.input_dim, order,
                                     who="generate_clips_from_wav", keep=given_keep)
        if given_poses is not None:
            _lib.given_kinds_check(given_in, given_poses, B, "generate_clips_from_wav")
            given_poses = _lib.given_pose_block(given_poses, [int(t) // 4 for t in mixed_tables(ns, sr, 22000, fps)["mfcc_rows"]], order,
                                                who="generate_clips_from_wav", width=self.each_dim[1] + self.each_dim[2])
        if style is not None:
            style = _lib.style_block(style, [int(t) // 4 for t in mixed_tables(ns, sr, 22000, fps)["mfcc_rows"]], self.num_classes, order,
                                     who="generate_clips_from_wav", ids=ids)
        if code_bias is not None:
            code_bias = _lib.code_bias_block(code_bias, B, self.generator.input_dim, order, who="generate_clips_from_wav", mode=mode)
        if repeat is not None:
            repeat = _lib.repeat_table(repeat, B, self.generator.input_dim, order, who="generate_clips_from_wav", mode=mode)
        gent = _lib.guide_entries(guide, B, who="generate_clips_from_wav", audio_key="wav", mode=mode, n_classes=self.num_classes,
                                  rows=None if guide is None else [int(t) // 4 for t in mixed_tables(ns, sr, 22000, fps)["mfcc_rows"]])
        for b, e in enumerate(gent or ()):
            if e is not None and e["audio"] is not None and tuple(np.shape(e["audio"])) != (int(ns[b]),):
                raise ValueError(f"generate_clips_from_wav: guide of clip {b}: wav must have the recording's own sample count ({int(ns[b])},), got "
                                 f"{tuple(np.shape(e['audio']))}")
        ids = ids_in_row_order(ids, self.num_classes, order, dev)
        if clip_indices is None:
            clip_index = upload(np.asarray(order, np.int64) + int(clip_index0), dev)
        else:
            clip_index = upload(np.asarray([int(clip_indices[i]) for i in order], np.int64), dev)
        if seed is None:
            seed = _fresh_seed() if mode == _lib.TS_SAMPLE_PHILOX else 0
        wav, ns_host, ns_dev = pad_recordings(wavs, ns, order, dev)
        pieces = dict(sampling_table=table, given=given, given_poses=given_poses, given_keep=given_keep, style=style, code_bias=code_bias, repeat=repeat)
        prim = None
        if gent is not None:
            wav, ns_host, ns_dev, ids, clip_index, pieces, prim = self.guide_wav_rows(gent, order, wav, ns_host, ids, clip_index, sr, fps, pieces,
                                                                                       "generate_clips_from_wav")
        if an is not None:      # no guidance here (refused above): the rows are the recordings
            from talkshow_amd import sampling as S
            codes, poses, lens, alt = self.infer_padded_wav(wav, ns_host, ns_dev, sr, ids, clip_index, mode, seed, fps, alternatives=an, **pieces)
            return [(codes[inverse[b], :int(lens[inverse[b]]) // 4], poses[inverse[b], :4 * (int(lens[inverse[b]]) // 4)],
                     S.Alternatives(*(x[inverse[b], :int(lens[inverse[b]]) // 4] for x in alt))) for b in range(B)]
        codes, poses, lens = self.infer_padded_wav(wav, ns_host, ns_dev, sr, ids, clip_index, mode, seed, fps, **pieces)
        if prim is not None:      # the shadows' rows are their primaries': the caller sees B results
            pdev = torch.as_tensor(prim, dtype=torch.int64, device=dev)
            codes, poses, lens = codes.index_select(0, pdev), poses.index_select(0, pdev), lens[prim]
        return [(codes[inverse[b], :int(lens[inverse[b]]) // 4], poses[inverse[b], :4 * (int(lens[inverse[b]]) // 4)]) for b in range(B)]

    def infer_on_audio(self, aud_fn, initial_pose=None, norm_stats=None, exp=None, var=None, w_pre=False, rand=None,
                       continuity=False, id=None, fps=15, sr=22000, B=1, am=None, am_sr=None, frame=0, **kwargs):
        '''
        (aud_fn, txgfile) -> generated motion (B, T, C)      [smplx_body_pixel.py:232-289]

        Extra keyword arguments understood here (ignored by the reference through **kwargs):
        `greedy=True` (argmax decode), `seed=int`, `uniforms=(B,H,2)`, and the sampling controls `temperature=`, `top_k=`, `top_p=`
        (one record for all B samples; `generate_batch(..., sampling=)`), and `code_bias=` — ONE (2, V) table (or {"body", "hand"} dict) for
        all B samples: which codes the decode may use (`generate_clips`), and `repeat=` — ONE (window, presence, frequency) record or
        dict for all B samples: a repetition penalty over a window of earlier codes (`generate_clips`).  With `continuity=True` they raise ValueError: a host that wants
        controls on a streaming session opens one itself (`open_stream(..., sampling=, style=, code_bias=, repeat=)`, `BodyStream.push`).
        '''
        assert self.args.infer, "train mode"
        code_bias = kwargs.get('code_bias', None)
        if code_bias is not None:
            if continuity:
                raise ValueError("infer_on_audio: the streaming session behind continuity=True takes no code bias")
            if isinstance(code_bias, (list, tuple)):
                raise ValueError("infer_on_audio: code_bias is ONE (2, V) table or dict for all B samples (generate_clips takes one per clip)")
            mode_ = _lib.TS_SAMPLE_GREEDY if kwargs.get('greedy', False) else _lib.TS_SAMPLE_PHILOX
            _lib.code_bias_block(code_bias, 1, self.generator.input_dim, who="infer_on_audio", mode=mode_)   # raises before the audio is read
        repeat = kwargs.get('repeat', None)
        if repeat is not None:
            if continuity:
                raise ValueError("infer_on_audio: the streaming session behind continuity=True takes no repetition penalty")
            if isinstance(repeat, list):
                raise ValueError("infer_on_audio: repeat is ONE (window, presence, frequency) record or dict for all B samples (generate_clips takes one per clip)")
            mode_ = _lib.TS_SAMPLE_GREEDY if kwargs.get('greedy', False) else _lib.TS_SAMPLE_PHILOX
            _lib.repeat_table(repeat, 1, self.generator.input_dim, who="infer_on_audio", mode=mode_)   # raises before the audio is read
        sampling = None
        if any(kwargs.get(k) is not None for k in ('temperature', 'top_k', 'top_p')):
            if continuity:
                raise ValueError("infer_on_audio: the streaming session behind continuity=True takes no sampling controls yet "
                                 "(temperature / top_k / top_p)")
            if kwargs.get('greedy', False):
                raise ValueError("infer_on_audio: sampling controls with greedy=True (greedy through the controls is top_k=1)")
            sampling = {k: kwargs[k] for k in ('temperature', 'top_k', 'top_p') if kwargs.get(k) is not None}
            _lib.sampling_table(sampling, 1, self.generator.input_dim)      # a bad record raises before the audio is read
        self.generator.eval()
        self.g_body.eval()
        self.g_hand.eval()

        if continuity:
            aud_feat, gap = get_mfcc_sepa(aud_fn, sr=sr, fps=fps)
        else:
            aud_feat = get_mfcc_ta(aud_fn, sr=sr, fps=fps, smlpx=True, type='mfcc', am=am)
        aud_feat = aud_feat.transpose(1, 0)
        aud_feat = aud_feat[np.newaxis, ...].repeat(B, axis=0)
        aud_feat = torch.tensor(aud_feat, dtype=torch.float32).to(self.device)

        if id is None:
            id = torch.tensor([0]).to(self.device)
        else:
            lo, hi = int(id.min()), int(id.max())                 # nn.Embedding's IndexError, before anything is launched
            if lo < 0 or hi >= self.num_classes:
                raise IndexError(f"speaker id out of range: [{lo}, {hi}] not within [0, {self.num_classes})")
            id = id.repeat(B)

        mode = _lib.TS_SAMPLE_GREEDY if kwargs.get('greedy', False) else _lib.TS_SAMPLE_PHILOX
        uniforms = kwargs.get('uniforms', None)
        if uniforms is not None:
            mode = _lib.TS_SAMPLE_UNIFORMS
        seed = kwargs.get('seed', None)
        if seed is None:
            seed = _fresh_seed() if mode == _lib.TS_SAMPLE_PHILOX else 0

        with torch.no_grad():
            aud_feat = aud_feat.permute(0, 2, 1)                      # (B, T, 64)
            if continuity:
                # the reference generates the first 2 s, then the rest behind the first part's codes and audio rows as a
                # prefix it re-runs in full (`:260-269`); here the second part continues the first part's row cache
                self.audioencoder.eval()
                session = self.open_stream(id, B, max_frames=max(gap, aud_feat.shape[1] - gap))
                u0 = u1 = None
                if uniforms is not None:                                 # (B, H, 2) for the whole clip: split at the seam's code row
                    uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
                    h0, h1 = gap // 4, (aud_feat.shape[1] - gap) // 4    # code rows of the two parts (each loses its own remainder)
                    if tuple(uniforms.shape) != (B, h0 + h1, 2):
                        raise ValueError(f"continuity: uniforms must have shape (B={B}, {h0} + {h1} code rows, 2), got {tuple(uniforms.shape)}")
                    u0, u1 = uniforms[:, :h0].contiguous(), uniforms[:, h0:h0 + h1].contiguous()
                part0 = session.push(aud_feat[:, :gap], mode=mode, seed=seed, uniforms=u0)
                part1 = session.push(aud_feat[:, gap:], mode=mode, seed=seed, uniforms=u1)
                session.close()
                pred_poses = torch.cat([part0, part1], dim=1).cpu().numpy()
            else:
                self.audioencoder.eval()
                _, poses = self.generate_batch(aud_feat, id, mode=mode, uniforms=uniforms, seed=seed, sampling=sampling, code_bias=code_bias, repeat=repeat)
                pred_poses = poses.cpu().numpy()

        output = pred_poses
        return output

    def open_stream(self, id, B, max_frames, *, seamless=False, sampling=None, style=None, code_bias=None, repeat=None, wav_sr=None,
                    wav_db="running", max_samples=None, fps=30, guide=None):
        """Long-audio / continuity generation: a session that is fed MFCC chunks and returns the poses of
        each chunk, every chunk continuing the PixelCNN row cache of the ones before it (`ts_pixelcnn_stream_*`) — the
        reference's `infer(..., pre_latents, pre_audio)` chain (`:291-304`) for any number of chunks, at a cost per chunk
        that does not grow with the history.  sampling / style / code_bias / repeat: session defaults for the keywords of
        `push` (`GatedPixelCNN.open_stream`).

        seamless=False (the default): `BodyStream`.  As in the reference, each chunk goes through the audio encoder and the VQ
        decoders on its own (their receptive fields are not carried across chunks), so every chunk border is padded like a clip
        edge: audio rows within 7 code rows of a seam, the codes drawn from them, and pose frames within 6 code rows of it differ
        from one call over the whole audio.  `push(mfcc (B,T,64)) -> poses (B, 4*(T//4), 129)`; a chunk's T % 4 frames are lost.

        seamless=True: `talkshow_amd.streaming.SeamlessBodyStream` (`ts_body_stream_*`).  ANY chunking returns the
        bits of `generate_batch` on the concatenated audio (same mode, seed, clip_index0 and keywords): the conv nets run on
        windows cut so that every kept row has its whole receptive field, through the same entries a clip takes.
          push(mfcc (B,t,64), ...)   any t in 1 .. max_frames; leftover frames are carried.  Returns poses (B, n, 129), n = 4 x the code
                                     rows that became final — possibly 0 during the first ~80 frames: the poses of a code row follow its
                                     audio by 20 code rows (80 frames, 2.67 s at 30 fps).
          flush(...)                 the rest, ending the clip; a later push raises ValueError.  Over a session the returned frames sum to
                                     4 * (frames_in // 4).
          return_codes=True adds the call's codes (B,Hc,2), logprobs=True their log-probabilities.  The step keywords (sampling, style,
          code_bias, repeat, given, uniforms) apply to the Hc code rows THAT call runs: `session.plan(t, flush=False)` ->
          (code_rows, pose_frames) names the counts beforehand, and a wrong `uniforms` / `given` row count raises ValueError naming the
          expected one before any device work.  Properties: frames_in, code_rows, frames, state_bytes (constant for any history).
        Not taken by a seamless session: clips of different lengths, given poses, kept positions, style tracks inside a step.

        wav_sr=None (the default): the sessions above, fed MFCC frames.  wav_sr = a sample rate: `talkshow_amd.streaming.WavBodyStream`, the
        same session fed SAMPLES at that rate through a streaming front end (`MFCC.open_stream`; talkshow_hip.h, "wav sessions"):
          push_wav(wav (B,n), ...)   any n in 0 .. max_samples (default: the samples of max_frames frames); the keywords of `push`.  A call
                                     that yields no MFCC frame makes no body call and returns empty tensors.
          flush(...)                 flushes the front end, pushes the last frames and flushes a seamless session.
          plan_wav(n, flush=False)   -> (MFCC frames, code rows, pose frames) of that call.
        wav_db="running" clamps each MFCC row at (the maximum so far - 80 dB); wav_db = the recordings' maxima (`MFCC.peak_db(wav)`, (B,))
        makes the frames those of `MFCC(wav_sr)(wav)` bit for bit, and with seamless=True the poses those of `generate_batch` on them, for
        any chunking of the samples.  The slots of a wav-fed session share ONE SAMPLE CLOCK: `restart`, `save`, `load` and `fork` raise
        NotImplementedError.

        guide: GUIDANCE at clip level in a plain session (`BodyStream`; `talkshow_amd.streaming.BodyGuide`): per clip None or {"scale": s,
        "id": int or None, "style": row or None, "audio": bool}; one dict serves all clips.  An absent id or style is the clip's own;
        "audio": False (the default) means the shadow hears the clip's own audio (id or style guidance), True that every push brings the
        shadow's MFCC chunk (`push(..., guide=[{"scale": s, "mfcc": (t, 64)}, ...])`).  Plain and seamless sessions take both kinds
        (`ts_body_stream_open_guided`); a wav-fed session takes shadows WITHOUT audio of their own (the MFCC rows come from the B-slot
        front end; "audio": True raises NotImplementedError naming the reason)."""
        if wav_sr is not None:
            from talkshow_amd.streaming import WavBodyStream
            return WavBodyStream(self, id, B, max_frames, seamless, wav_sr, wav_db=wav_db, max_samples=max_samples, fps=fps, sampling=sampling,
                                 style=style, code_bias=code_bias, repeat=repeat, guide=guide)
        if seamless:
            from talkshow_amd.streaming import SeamlessBodyStream
            return SeamlessBodyStream(self, id, B, max_frames, sampling=sampling, style=style, code_bias=code_bias, repeat=repeat, guide=guide)
        return BodyStream(self, id, B, max_frames, sampling=sampling, style=style, code_bias=code_bias, repeat=repeat, guide=guide)

    def generate_long(self, mfcc, ids, chunk_frames=240, mode=_lib.TS_SAMPLE_PHILOX, uniforms=None, seed=None, clip_index0=0, sampling=None,
                      style=None, code_bias=None, repeat=None, guide=None):
        """`generate_batch` for audio of ANY length at memory bounded by the chunk: mfcc (B,T,64), ids (B,) or one for all -> codes
        (B,T//4,2), poses (B,4 (T//4),129), bit for bit what `generate_batch(mfcc, ids, mode=, uniforms=, seed=, clip_index0=, ...)` returns,
        through one seamless session (`open_stream(..., seamless=True)`) pushed chunk_frames at a time.  Only the results are as long as the
        audio (mfcc may live on the host: a chunk is uploaded when it is pushed).  uniforms: (B,T//4,2) for TS_SAMPLE_UNIFORMS.  sampling /
        style (one weight row per clip) / code_bias / repeat: the keywords of `generate_batch` a session takes, for the whole clip.
        guide: the keyword of `generate_batch` — one dict for all clips or per clip None or {"scale": s, "mfcc": (T, 64) or None, "id": ..,
        "style": one weight row} — passed through to the session: a shadow's "mfcc" is whole-length audio, cut per chunk."""
        if len(mfcc.shape) != 3 or int(mfcc.shape[2]) != 64:
            raise ValueError(f"generate_long: mfcc must be (B, T, 64), got {tuple(mfcc.shape)}")
        B, T = int(mfcc.shape[0]), int(mfcc.shape[1])
        chunk_frames = int(chunk_frames)
        if chunk_frames < 1:
            raise ValueError(f"generate_long: chunk_frames is at least 1, got {chunk_frames}")
        if uniforms is not None:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
            if tuple(uniforms.shape) != (B, T // 4, 2):
                raise ValueError(f"generate_long: uniforms must have shape (B={B}, {T // 4}, 2), got {tuple(uniforms.shape)}")
            mode = _lib.TS_SAMPLE_UNIFORMS
        if seed is None:
            seed = _fresh_seed() if mode == _lib.TS_SAMPLE_PHILOX else 0
        opened = shadow_mfcc = None
        if guide is not None:                      # the entries a session is opened with, and the whole-length audio of the shadows that bring one
            per = [guide] * B if isinstance(guide, dict) else list(guide)
            if len(per) != B:
                raise ValueError(f"generate_long: guide is one dict for all clips or a list with one entry per clip (B = {B})")
            opened, shadow_mfcc = [], {}
            for b, e in enumerate(per):
                if isinstance(e, dict) and e.get("mfcc") is not None:
                    if tuple(e["mfcc"].shape) != (T, 64):
                        raise ValueError(f"generate_long: guide of clip {b}: mfcc must have the clip's own shape ({T}, 64), got {tuple(e['mfcc'].shape)}")
                    shadow_mfcc[b] = e["mfcc"]
                opened.append(dict({k: v for k, v in e.items() if k != "mfcc"}, audio=b in shadow_mfcc) if isinstance(e, dict) else e)
        session = self.open_stream(ids, B, chunk_frames, seamless=True, sampling=sampling, style=style, code_bias=code_bias, repeat=repeat,
                                   guide=opened)
        codes, poses = [], []
        try:
            for f0 in list(range(0, T, chunk_frames)) + [None]:
                t = 0 if f0 is None else min(chunk_frames, T - f0)
                r0 = session.code_rows
                n, _ = session.plan(t, flush=f0 is None)
                kw = dict(mode=mode, seed=seed, clip_index0=clip_index0, uniforms=None if uniforms is None else uniforms[:, r0:r0 + n],
                          return_codes=True)
                if shadow_mfcc and f0 is not None:
                    kw["guide"] = [{"mfcc": shadow_mfcc[b][f0:f0 + t]} if b in shadow_mfcc else None for b in range(B)]
                p, c = session.flush(**kw) if f0 is None else session.push(mfcc[:, f0:f0 + t], **kw)
                codes.append(c)
                poses.append(p)
        finally:
            session.close()
        return torch.cat(codes, 1), torch.cat(poses, 1)

    def infer(self, aud_feat, frame, id, B, pre_latents=None, pre_audio=None, pre_pose=None, mode=None, seed=None):
        """smplx_body_pixel.py:291-304 (continuity helper, reference call shape): returns latents, audio (B,256,H,2),
        body, hand (B,C,T); `pre_latents` / `pre_audio` are re-run as a prefix exactly like the reference does."""
        if mode is None:
            mode = _lib.TS_SAMPLE_PHILOX
        if seed is None:
            seed = _fresh_seed()
        rows = self.audioencoder.forward_nlc(aud_feat)                                    # (B,H,256)
        audio = rows.transpose(1, 2).unsqueeze(dim=-1).repeat(1, 1, 1, 2)
        pre_rows = pre_audio[..., 0].transpose(1, 2).contiguous() if pre_audio is not None else None
        latents, _ = self.generator.run(id, rows, mode=mode, seed=seed, pre_codes=pre_latents, pre_aud=pre_rows)
        out = self._decode_pair(latents)                                                   # Decoder ignores pre_state
        body = out[..., :self.each_dim[1]].transpose(1, 2)
        hand = out[..., self.each_dim[1]:].transpose(1, 2)
        return latents, audio, body, hand

    def generate(self, aud, id, frame_num=0):
        """smplx_body_pixel.py:306-325: aud (B,64,T), id (B,) -> (B,T,129).  (The reference version raises a
        TypeError because `decode` returns tuples; this one returns the tensor it meant to.)"""
        _, poses = self.generate_batch(torch.as_tensor(aud).permute(0, 2, 1), id)
        return poses


class BodyStream:
    """See `TrainWrapper.open_stream`.  `push(mfcc_chunk (B,T,64)) -> poses (B, 4*(T//4), 129)` device tensor.

    guide (talkshow_amd.streaming.BodyGuide; DESIGN.md §5, "session pairs"): per clip None or {"scale": s, "id": int or None, "style": row or
    None, "audio": bool} — guidance at clip level.  The chain session then has S = B + n_g slots, the clips first and their shadows behind
    them, paired (`PixelCNNStream`, `pairs=`); the audio encoder runs on the clips' chunks and on the chunks of the shadows that hear audio
    of their own, the encoded rows are spread to the S slots by index, ONE step runs under the pairs and only the clips' rows are decoded.
    A clip opened without a shadow cannot take one later: open a shadow (scale 0 is the off switch) wherever guidance may be wanted."""

    def __init__(self, wrapper, id, B, max_frames, sampling=None, style=None, code_bias=None, repeat=None, guide=None):
        from talkshow_amd.streaming import BodyGuide
        self.w, self.B = wrapper, int(B)
        if id is None:
            id = torch.tensor([0])
        gen = wrapper.generator
        self.g = g = BodyGuide(guide, self.B, gen.n_classes)
        rows = max(1, int(max_frames) // 4)
        self.seed = _fresh_seed()          # one stream of random numbers per session unless push() is given a seed
        if not g.shadow_of:
            self.pix = gen.open_stream(id, self.B, rows, sampling=sampling, style=style, code_bias=code_bias, repeat=repeat)
            return
        ids = _index_tensor(id, gen.n_classes, "speaker id", gen._dev()).cpu().numpy().reshape(-1)
        if ids.size == 1 and self.B > 1:
            ids = np.repeat(ids, self.B)
        if ids.size != self.B:
            raise ValueError(f"open_stream: id must hold 1 or B={self.B} speaker ids, got {ids.size}")
        self.shadow_style = {}             # clip -> its shadow's weight row, where the entry brought one
        labels = list(ids) + [ids[b] if g.entries[b]["id"] is None else g.entries[b]["id"] for b in g.shadow_of]
        defaults = {k: self._spread(k, v) for k, v in (("sampling", sampling), ("style", None), ("code_bias", code_bias), ("repeat", repeat))}
        self._style_default = style        # spread at every push: a shadow keeps its own conditioning under a session default
        styled = [b for b in g.shadow_of if g.entries[b]["style"] is not None]
        self.pix = gen.open_stream(np.asarray(labels, np.int64), g.S, rows, sampling=defaults["sampling"], code_bias=defaults["code_bias"],
                                   repeat=defaults["repeat"], pairs=None if styled else g.pairs())
        if styled:                         # a shadow's weight row is written as a restart at row 0 writes it; the pairs form behind it
            for b in styled:
                self.shadow_style[b] = np.asarray(g.entries[b]["style"], np.float32)
            self.pix.restart([g.slot_of[b] for b in styled], style=[self.shadow_style[b] for b in styled], pairs=g.pairs())

    def _spread(self, name, v):
        """`BodyGuide.spread_kw`: a per-clip keyword of B entries as the S entries of the chain session."""
        return self.g.spread_kw(name, v, self.shadow_style)

    @property
    def frames(self):
        return 4 * self.pix.rows

    def push(self, mfcc, mode=_lib.TS_SAMPLE_PHILOX, seed=None, clip_index0=0, uniforms=None, *, sampling=None, logprobs=False, given=None,
             style=None, code_bias=None, repeat=None, guide=None):
        """The keywords are `PixelCNNStream.step`'s, for this chunk's code rows; with `logprobs` the return value is (poses, logprobs
        (B, T//4, 2)).  guide: None, a float for all guided clips, or a list with, per clip, None, a float or {"scale": s, "mfcc": (t, 64)}
        (`BodyGuide.push`): the step's scales, and the MFCC chunk of every shadow opened with "audio": True.  A wrong key or shape, or an
        entry on a clip opened without a shadow, raises ValueError naming the clip before any device work."""
        g = self.g
        if not g.shadow_of:
            if guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide)):
                g.push(guide, int(mfcc.shape[1]))      # raises: names the clip that was opened without a shadow
            rows = self.w.audioencoder.forward_nlc(mfcc)                      # (B, T//4, 256), this chunk alone
            out = self.pix.step(rows, mode=mode, uniforms=uniforms, seed=self.seed if seed is None else seed, clip_index0=clip_index0,
                                sampling=sampling, logprobs=logprobs, given=given, style=style, code_bias=code_bias, repeat=repeat)
            if isinstance(out, tuple):
                return self.w._decode_pair(out[0]), out[1]
            return self.w._decode_pair(out)
        if int(mfcc.shape[0]) != self.B:
            raise ValueError(f"session was opened for B={self.B}, got {int(mfcc.shape[0])}")
        scales, chunks = g.push(guide, int(mfcc.shape[1]))
        if scales is not None:
            self.pix._pairs.step_scales(scales, who="push")
        style = self._style_default if style is None else style
        kw = {k: self._spread(k, v) for k, v in (("sampling", sampling), ("given", given), ("style", style), ("code_bias", code_bias),
                                                 ("repeat", repeat), ("uniforms", uniforms))}
        dev = self.w.generator._dev()
        mfcc = torch.as_tensor(mfcc, dtype=torch.float32, device=dev)
        if chunks:                                                            # the E streams: the clips, then the shadows that hear their own
            mfcc = torch.cat([mfcc, torch.stack([torch.as_tensor(m, dtype=torch.float32, device=dev) for m in chunks])])
        rows = self.w.audioencoder.forward_nlc(mfcc)                          # (E, T//4, 256)
        rows = rows.index_select(0, torch.as_tensor(g.spread(), dtype=torch.int64, device=rows.device))      # (S, T//4, 256): plumbing
        want_lp = logprobs is not None and logprobs is not False
        out = self.pix.step(rows, mode=mode, seed=self.seed if seed is None else seed, clip_index0=clip_index0, logprobs=bool(want_lp),
                            guide=scales, **kw)
        codes = out[0] if want_lp else out
        poses = self.w._decode_pair(codes[:self.B].contiguous())              # the clips' rows are the block's first B
        if not want_lp:
            return poses
        lp = out[1][:self.B]
        if torch.is_tensor(logprobs):
            logprobs.copy_(lp)
            lp = logprobs
        return poses, lp

    @property
    def slot_rows(self):
        """`PixelCNNStream.slot_rows`: the code rows of every slot's current clip."""
        return self.pix.slot_rows[:self.B]

    def _unguided(self, slots, what):
        for b in ([slots] if isinstance(slots, int) else list(slots)):
            if self.g.entries[b] is not None if 0 <= b < self.B else False:
                raise ValueError(f"{what}: clip {b} is guided: its state is two slots of the chain session (`session.pix.save([b, g])`, "
                                 f"`load([b2, g2], state, pairs={{b2: g2}})`)")

    def restart(self, slots, id=None, *, style=None, clip_indices=None, guide=None):
        """`PixelCNNStream.restart`: the listed slots begin new clips (speaker `id`, or a `style` row) with the next push.  A plain session
        runs the audio encoder and the VQ decoders on each chunk per clip, so nothing else carries over: a restarted slot's poses equal
        those of a fresh `open_stream(id, 1, ...)` pushed the same chunks (same seed, clip_index0 = its clip index).  A slot whose user
        has left needs no call: push any audio rows for it and ignore its poses.
        guide: one entry per listed slot (the forms of `open_stream`): a guided clip restarts together with its shadow under the new
        entry's id or style, and the pair is declared again under its scale.  A clip opened without a shadow cannot take one; a clip with
        a shadow that restarts without an entry gets scale 0; "audio" stays as the clip was opened."""
        g = self.g
        if not g.shadow_of:
            if guide is not None and not (isinstance(guide, (list, tuple)) and all(e is None for e in guide)):
                b = ([slots] if isinstance(slots, int) else list(slots) or [0])[0]
                if isinstance(guide, (list, tuple)) and len(guide) == len([slots] if isinstance(slots, int) else list(slots)):
                    b = [c for c, e in zip([slots] if isinstance(slots, int) else list(slots), guide) if e is not None][0]
                raise ValueError(f"restart: guide of clip {b}: the clip was opened without a shadow (open one wherever guidance may be wanted)")
            self.pix.restart(slots, id, style=style, clip_indices=clip_indices)
            return self
        from talkshow_amd.streaming import BodyGuide, SlotClock
        NC = self.w.generator.n_classes
        slots, labels, styles, clips = SlotClock.check(self.B, NC, slots, id, style, clip_indices)
        n = len(slots)
        entries = BodyGuide.parse(guide, n, NC, who="restart")
        new, pairs = {}, {}
        all_slots, all_labels, all_styles, all_clips = list(slots), list(labels or [None] * n), list(styles or [None] * n), list(clips)
        for i, b in enumerate(slots):
            opened, e = g.entries[b], entries[i]
            if opened is None:
                if e is not None:
                    raise ValueError(f"restart: guide of clip {b}: the clip was opened without a shadow (open one wherever guidance may be wanted)")
                continue
            if e is None:                  # the shadow restarts as the clip's twin, switched off
                e = {"scale": 0.0, "id": None, "style": None, "audio": opened["audio"]}
            elif e["audio"] != opened["audio"]:
                raise ValueError(f"restart: guide of clip {b}: \"audio\" stays as the clip was opened ({opened['audio']})")
            new[b] = e
            all_slots.append(g.slot_of[b]), all_clips.append(g.slot_of[b])
            if e["style"] is not None:
                all_labels.append(None), all_styles.append(np.asarray(e["style"], np.float32))
            elif e["id"] is not None:
                all_labels.append(e["id"]), all_styles.append(None)
            else:                          # the clip's own conditioning
                all_labels.append(all_labels[i]), all_styles.append(all_styles[i])
            pairs[b] = (g.slot_of[b], e["scale"])
        has_style = any(v is not None for v in all_styles)
        self.pix.restart(all_slots, all_labels if any(v is not None for v in all_labels) else None, style=all_styles if has_style else None,
                         clip_indices=all_clips, pairs=pairs or None)
        for b, e in new.items():
            g.entries[b] = e
            self.shadow_style.pop(b, None)
            if e["style"] is not None:
                self.shadow_style[b] = np.asarray(e["style"], np.float32)
            elif e["id"] is None and styles is not None and styles[slots.index(b)] is not None:
                self.shadow_style[b] = np.asarray(torch.as_tensor(styles[slots.index(b)]).cpu().numpy(), np.float32)
        return self

    def save(self, slots):
        """`PixelCNNStream.save`: the state of the listed slots' clips.  A plain session runs the audio encoder and the VQ decoders on each
        chunk per clip, so the chain's slot state is all a clip carries between pushes.  A guided clip is refused, naming it."""
        self._unguided(slots, "save")
        return self.pix.save(slots)

    def load(self, slots, state, *, clip_indices=None):
        """`PixelCNNStream.load`: the listed slots carry the saved clips on with the next push.  A guided clip is refused, naming it."""
        self._unguided(slots, "load")
        self.pix.load(slots, state, clip_indices=clip_indices)
        return self

    def fork(self, src, dst_slots, *, clip_indices=None):
        """`PixelCNNStream.fork`: the listed slots carry slot `src`'s clip on, each under its own clip index (default: the source's, which
        makes them its twins: the same poses for the same audio).  A guided clip is refused, naming it."""
        self._unguided(src, "fork")
        self._unguided(dst_slots, "fork")
        self.pix.fork(src, dst_slots, clip_indices=clip_indices)
        return self

    def close(self):
        self.pix.close()
