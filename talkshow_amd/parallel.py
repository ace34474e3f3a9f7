"""Multi-GPU driver pieces: one process per GPU, clips sharded by contiguous blocks, ONE exchange at the end.

The reference has no distributed code.  Clips are independent (no cross-sample op anywhere,
BatchNorm is in eval mode), so ranks never talk during generation; `gather_sequences` is the single RCCL all-gather
(backend "nccl" == RCCL over xGMI on ROCm; "gloo" in the CPU tests) of the generated pose sequences.
Determinism contract: the result for global clip k does not depend on the world size — greedy decode is a pure
function of the clip, and the stochastic sampler's Philox subsequence is the global clip index (clip_index0).
"""
import torch
import torch.distributed as dist


def shard_range(n_clips, rank, world):
    """Contiguous block of ceil(n/world) clips for `rank` (last ranks may get fewer / none): (start, stop)."""
    per = (n_clips + world - 1) // world
    start = min(rank * per, n_clips)
    return start, min(start + per, n_clips)


def gather_sequences(local, n_total=None):
    """all-gather of (n_local, T, C) sequences -> (n_total, T, C) on every rank, in global clip order.

    Ranks may hold different n_local (ragged tail): shards are padded to the largest block for the collective and
    trimmed afterwards.  Without an initialised process group this is the identity.
    """
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local
    world = dist.get_world_size()
    n_local = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
    counts = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(counts, n_local)
    counts = [int(c.item()) for c in counts]
    nmax = max(counts)
    if local.shape[0] < nmax:
        pad = torch.zeros((nmax - local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        local = torch.cat([local, pad], 0)
    out = torch.empty((world * nmax,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous())
    parts = [out[r * nmax:r * nmax + counts[r]] for r in range(world)]
    res = torch.cat(parts, 0)
    if n_total is not None:
        assert res.shape[0] == n_total, (res.shape, n_total)
    return res


def generate_sharded(generate_fn, mfcc, ids, batch=32):
    """Run `generate_fn(mfcc_block, ids_block, clip_index0)` over THIS rank's shard in batches; no collective here.

    mfcc (N,T,64) / ids (N,) are the GLOBAL inputs (every rank holds them, or at least its own block).
    generate_fn returns (codes, poses (n,T',C)) for a block.  Returns (local poses (n_local,T',C), (start, stop)); hand
    `local` to `gather_sequences` for the one exchange.  A rank whose shard is empty (fewer clips than ranks, or a
    ragged tail) returns a (0,T',C) tensor with the right trailing shape, dtype and device for the collective:
    generate_fn is asked for them with a zero-clip block (`mfcc[0:0]`), which the HIP wrapper answers without a launch
    (`output_shape`), a stand-in by returning an empty result.
    """
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    n = mfcc.shape[0]
    a, b = shard_range(n, rank, world)
    outs = []
    for s in range(a, b, batch):
        e = min(s + batch, b)
        _, poses = generate_fn(mfcc[s:e], ids[s:e], s)
        outs.append(poses)
    if outs:
        local = torch.cat(outs, 0)
    else:
        local = _empty_like_output(generate_fn, mfcc, ids)
    return local, (a, b)


def _empty_like_output(generate_fn, mfcc, ids):
    """(0,T',C) tensor on the device / in the dtype generate_fn produces, for a rank with no clips."""
    shape_fn = getattr(generate_fn, "output_shape", None)
    if shape_fn is not None:
        tail, dtype, device = shape_fn(mfcc)
        return torch.zeros((0,) + tuple(tail), dtype=dtype, device=device)
    _, probe = generate_fn(mfcc[0:0], ids[0:0], 0)
    if probe.ndim < 2 or probe.shape[0] != 0:
        raise RuntimeError("generate_fn must answer a zero-clip block with a (0,T',C) tensor (or expose output_shape)")
    return probe


_side_streams = {}


def _side_stream(device, k=0):
    """library-created side stream k of the device (each its own hardware queue and scratch arena)"""
    from . import _lib
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if (idx, k) not in _side_streams:
        _side_streams[(idx, k)] = _lib.create_streams(1, idx)[0]
    return _side_streams[(idx, k)]


def whole_body_local(body, face, mfcc, ids, wav, face_ids, mode=None, seed=0, clip_index0=0, batch_body=32, batch_face=64,
                     stand=False, overlap=True):
    """Whole-body generation of THIS rank's clips (no collective): body path in batches of `batch_body`, face path in
    batches of `batch_face`, (n, Tf, 265) rows assembled on the GPU (`pose_index.assemble_full` = demo.py:207-229 +
    part2full).  mfcc (n,T,64), ids (n,), wav (n,S) 16 kHz samples, face_ids (n,4); `clip_index0` = global index of
    the first clip (Philox subsequences).  n = 0 gives a (0, Tf, 265) tensor on the current device."""
    from . import _lib
    from .pose_index import assemble_full
    n = mfcc.shape[0]
    frames = wav.shape[1] * 30 // 16000                       # smplx_face.py:203
    mode = _lib.TS_SAMPLE_PHILOX if mode is None else mode
    if n == 0:
        return torch.zeros((0, frames, 265), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    poses, faces = [], []
    # the two generators are independent until the assembly: the body path (its autoregressive chain is latency-bound and leaves most
    # of the matrix pipe idle) goes to a side stream and runs under the face generator's GEMMs; both join before the assembly
    cur = torch.cuda.current_stream()
    side = _side_stream(cur.device) if overlap else cur
    if overlap:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        for s in range(0, n, batch_body):
            e = min(s + batch_body, n)
            poses.append(body.generate_batch(mfcc[s:e], ids[s:e], mode=mode, seed=seed, clip_index0=clip_index0 + s)[1])
    # face batches alternate between the current stream and a second side stream: a GEMM's partly filled last round and the gap
    # between one batch's dependent launches are filled by the other batch's workgroups (tools/face_streams.py: 59.4 -> 56.6 ms per
    # batch of 64 with two in flight); the generator keeps its scratch per stream, a batch's rows do not depend on the stream it ran on
    face_streams = [cur, _side_stream(cur.device, 1)] if overlap and n > batch_face else [cur]
    for st in face_streams[1:]:
        st.wait_stream(cur)
    for i, s in enumerate(range(0, n, batch_face)):
        e = min(s + batch_face, n)
        with torch.cuda.stream(face_streams[i % len(face_streams)]):
            faces.append(face.generator.run(wav[s:e], face_ids[s:e], frames))
    for st in face_streams[1:]:
        cur.wait_stream(st)
    for i, t in enumerate(faces):
        if face_streams[i % len(face_streams)] is not cur:
            t.record_stream(cur)
    if overlap:
        cur.wait_stream(side)
        for t in poses:
            t.record_stream(cur)
    return assemble_full(torch.cat(poses, 0), torch.cat(faces, 0), stand=stand)


def whole_body_clips(body, face, wavs, sr, ids, face_ids, mode=None, seed=0, clip_index0=0, stand=False, overlap=True, sampling=None,
                     given=None, given_poses=None, given_keep=None, style=None, code_bias=None, repeat=None, guide=None):
    """Whole-body generation from RECORDINGS of different lengths, in one pass: wavs = list of (N_b,) sample arrays / tensors at ONE source
    rate `sr` (a host with several rates groups by rate), ids = one body speaker index per recording (or one for all), face_ids
    (B, 4) / (1, 4) one-hot or zero rows or None -> list of (frames_b, 265) device tensors in submission order, frames_b =
    `frontend.mixed_tables(ns, sr)["face_frames"]`.

    The recordings are sorted once by sample count (longest first, stable: the order the body pass asks for; the face pass does not care)
    into one padded block.  Body branch: mixed MFCC front-end -> `ts_body_pixel_infer_mixed`; face branch: the same samples at 16 kHz,
    otherwise through `ts_resample_kaiser_mixed`, -> `ts_face_generate_mixed`; the branches run on the side-stream arrangement of
    `whole_body_local`, then `ts_assemble_full_mixed`.  Every table is host arithmetic and every host array travels through pinned memory
    (`modules.upload`): nothing between taking the list and returning it synchronises or leaves the device (speaker ids handed over as a
    DEVICE tensor are range-checked once per tensor version, which reads them back; host ids are checked on the host).  A recording's rows are bit-identical to the route of uniform entries on the recording alone
    (`MFCC` -> `generate_batch`, `FaceGenerator.run_clips`, `assemble_full`), its Philox subsequence is `clip_index0` + its position in
    the submitted list.  sampling: one sampling record (`_lib.sampling_record`) for all recordings or one per recording in submission order —
    they follow the recordings through the sort (the body branch then runs `ts_body_pixel_infer_mixed_ctl`; the face generator takes none).
    given: one entry per recording in submission order, None or the (G_b, 2) code rows the body decode of that recording starts from
    (`TrainWrapper.generate_clips`; the body branch then runs `ts_body_pixel_infer_mixed_given`); they follow the recordings through the sort.
    given_poses: the same from motion — None or the (P_b, 129) pose frames of that recording's head, encoded on the device
    (`TrainWrapper.generate_clips`; `ts_body_pixel_infer_mixed_poses`).  A recording brings one kind.
    given_keep: which positions of a recording's given rows are taken — None (all), "body" (keep the body column, draw new hands), "hand",
    or a (G_b, 2) mask, per recording or one for all (`TrainWrapper.generate_clips`; `ts_body_pixel_infer_mixed_keep`).
    style: float speaker weights for the BODY half in place of `ids` — per recording None (its id), an (NC,) row or an (H_b, NC) track with
    one row per code row, or one (NC,) / (B, NC) array for all (`TrainWrapper.generate_clips`; `ts_body_pixel_infer_mixed_style`; a blend
    interpolates the conditioning vectors, it is not a mixture of the speakers' distributions).  The face half keeps `face_ids`.
    code_bias: which codes the BODY half of a recording may use — one (2, V) table for all, or per recording None, a (2, V) table or a
    {"body", "hand"} dict; -inf bans a code (`TrainWrapper.generate_clips`; `ts_body_pixel_infer_mixed_bias`).  The face half has no codes.
    repeat: a repetition penalty over a window of earlier codes for the BODY half — one (window, presence, frequency) record or dict for
    all, or a list with one per recording (`TrainWrapper.generate_clips`; `ts_body_pixel_infer_mixed_repeat`).
    guide: guidance of the BODY half against a second conditioning — one dict for all or per recording None or {"scale", "wav" (N_b,)
    samples at `sr`, "id", "style"} (`TrainWrapper.generate_clips_from_wav`; `ts_body_pixel_infer_guided`).  The shadows are rows of
    the body pass only: the face half runs on the recordings themselves."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from nets.smplx_body_pixel import mixed_pass_order

    from .frontend import check_recordings, mixed_tables
    from .modules import ids_in_row_order, pad_recordings, resample_kaiser_padded, upload
    from .pose_index import lower_pose_block
    ns = check_recordings(wavs, "whole_body_clips")
    B = len(ns)
    n_ids = int(ids.numel()) if torch.is_tensor(ids) else int(np.asarray(ids).size)
    if n_ids not in (1, B):
        raise ValueError(f"whole_body_clips: ids must hold 1 or B={B} speaker indices, got {n_ids}")
    gen = face.generator
    if gen.out_dim != 103:
        raise ValueError("whole_body_clips: the 265-d assembly takes the 103-wide face output (jaw 3 + expression 100)")
    fid = None
    if gen.identity:
        fid = np.zeros((B, gen.num_classes), np.float32) if face_ids is None else \
            (face_ids.detach().cpu().numpy() if torch.is_tensor(face_ids) else np.asarray(face_ids)).astype(np.float32)
        if fid.ndim != 2 or fid.shape[1] != gen.num_classes or fid.shape[0] not in (1, B):
            raise ValueError(f"whole_body_clips: face_ids must be ({B}, {gen.num_classes}) or (1, {gen.num_classes}), got {tuple(fid.shape)}")
        if fid.shape[0] == 1 and B > 1:
            fid = np.repeat(fid, B, axis=0)
    order, inverse = mixed_pass_order(ns)
    tab = mixed_tables([ns[i] for i in order], sr)
    if int(tab["mfcc_rows"].min()) < 4 or int(tab["n16"].min()) < 400 or int(tab["face_frames"].min()) < 1:
        raise ValueError("whole_body_clips: a recording is too short (4 MFCC rows, 400 samples at 16 kHz and one face frame are needed)")
    mode = _lib.TS_SAMPLE_PHILOX if mode is None else mode
    if sampling is not None:   # validated before the first launch; sorted slot k holds the record of submitted recording order[k]
        recs = _lib.sampling_records(sampling, B)
        sampling = _lib.sampling_table([recs[i] for i in order], B, body.generator.input_dim, mode)
    if given_keep is not None or given is not None or given_poses is not None:      # validated before the first launch, too: rows_sub[i] = code rows of submitted recording i
        rows_sub = [0] * B
        for k, i in enumerate(order):
            rows_sub[i] = int(tab["mfcc_rows"][k]) // 4
        _lib.given_kinds_check(given, given_poses, B, "whole_body_clips")
        if given_keep is not None:
            given_keep = _lib.given_keep_block(given_keep, _lib.given_counts(given, given_poses, B), rows_sub, order, who="whole_body_clips")
        if given is not None:
            given = _lib.given_block(given, rows_sub, body.generator.input_dim, order, who="whole_body_clips", keep=given_keep)
        if given_poses is not None:
            given_poses = _lib.given_pose_block(given_poses, rows_sub, order, who="whole_body_clips", width=body.each_dim[1] + body.each_dim[2])
    if style is not None:      # validated before the first launch, too; the body half only
        rows_sub = [0] * B
        for k, i in enumerate(order):
            rows_sub[i] = int(tab["mfcc_rows"][k]) // 4
        style = _lib.style_block(style, rows_sub, body.num_classes, order, who="whole_body_clips", ids=ids)
    if code_bias is not None:      # validated before the first launch, too; the body half only
        code_bias = _lib.code_bias_block(code_bias, B, body.generator.input_dim, order, who="whole_body_clips", mode=mode)
    if repeat is not None:         # and the records
        repeat = _lib.repeat_table(repeat, B, body.generator.input_dim, order, who="whole_body_clips", mode=mode)
    grows = None
    if guide is not None:      # rows of submitted recording i, for the entries' style tracks
        grows = [0] * B
        for k, i in enumerate(order):
            grows[i] = int(tab["mfcc_rows"][k]) // 4
    gent = _lib.guide_entries(guide, B, who="whole_body_clips", audio_key="wav", mode=mode, n_classes=body.num_classes, rows=grows)      # and the guide entries
    for b, e in enumerate(gent or ()):
        if e is not None and e["audio"] is not None and tuple(np.shape(e["audio"])) != (int(ns[b]),):
            raise ValueError(f"whole_body_clips: guide of clip {b}: wav must have the recording's own sample count ({int(ns[b])},), got "
                             f"{tuple(np.shape(e['audio']))}")
    dev = body.generator._dev()
    # every host table of the pass, before the first launch: sample counts and the padded block, 16 kHz counts, face and body frame counts
    wav, ns_host, ns_dev = pad_recordings(wavs, ns, order, dev)
    small = np.ascontiguousarray(np.stack([tab["n16"], tab["face_frames"], tab["pose_frames"], tab["mfcc_rows"]]), dtype=np.int32)
    small_dev = upload(small, dev)
    n16_dev, tf_dev, tb_dev, rows_dev = small_dev[0], small_dev[1], small_dev[2], small_dev[3]
    ids_sorted = ids_in_row_order(ids, body.num_classes, order, dev)
    clip_index = upload(np.asarray(order, np.int64) + int(clip_index0), dev)
    fid_dev = upload(fid[order], dev) if fid is not None else None
    Tf_max = int(small[1].max())
    cur = torch.cuda.current_stream()
    side = _side_stream(cur.device) if overlap else cur
    if overlap:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        pieces = dict(sampling_table=sampling, given=given, given_poses=given_poses, given_keep=given_keep, style=style, code_bias=code_bias, repeat=repeat)
        if gent is None:
            _, poses, _ = body.infer_padded_wav(wav, ns_host, ns_dev, sr, ids_sorted, clip_index, mode, seed, lens_dev=rows_dev, **pieces)
        else:      # the body half alone runs the shadows' rows; its poses come back as the recordings' own B rows
            bwav, bns, bns_dev, bids, bclip, pieces, prim = body.guide_wav_rows(gent, order, wav, ns_host, ids_sorted, clip_index, sr, 30, pieces,
                                                                                  "whole_body_clips")
            _, poses, _ = body.infer_padded_wav(bwav, bns, bns_dev, sr, bids, bclip, mode, seed, **pieces)
            poses = poses.index_select(0, upload(prim.astype(np.int64), dev))
    i32p = C.POINTER(C.c_int32)
    if int(sr) == 16000:
        wav16 = wav
    else:
        wav16 = resample_kaiser_padded(wav, ns_host, ns_dev, sr, 16000)
    T16_max = int(wav16.shape[1])                                    # the block's own width; every n16[b] must fit it
    if int(small[0].max()) > T16_max:
        raise RuntimeError(f"whole_body_clips: a recording has {int(small[0].max())} samples at 16 kHz, the resampled block is {T16_max} wide")
    fout = torch.empty((B, Tf_max, gen.out_dim), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ts_face_generate_mixed(gen.handle(), _lib.dptr(wav16), small[0].ctypes.data_as(i32p), _lib.dptr(n16_dev),
                                                  small[1].ctypes.data_as(i32p), _lib.dptr(tf_dev), B, T16_max, Tf_max, _lib.dptr(fid_dev),
                                                  _lib.dptr(fout), None, _lib.stream_ptr()))
    if overlap:
        cur.wait_stream(side)
        poses.record_stream(cur)
    out = torch.empty((B, Tf_max, 265), dtype=torch.float32, device=dev)
    lp = lower_pose_block(stand)
    _lib.check(_lib.load().ts_assemble_full_mixed(_lib.context(dev.index), _lib.dptr(poses), _lib.dptr(tb_dev), _lib.dptr(fout),
                                                  _lib.dptr(tf_dev), B, poses.shape[1], Tf_max, _lib.fptr(lp), _lib.dptr(out),
                                                  _lib.stream_ptr()))
    return [out[inverse[b], :int(small[1][inverse[b]])] for b in range(B)]


def whole_body_sharded(body, face, mfcc, ids, wav, face_ids, mode=None, seed=0, batch_body=32, batch_face=64, stand=False):
    """BASELINE configs[4]: whole-body generation of N clips sharded over the ranks, one all-gather at the end.

    body / face: the `nets.s2g_body_pixel` / `nets.s2g_face` wrappers of this rank (full weight replicas).
    mfcc (N,T,64), ids (N,) int64 speaker indices, wav (N,S) 16 kHz samples, face_ids (N,4) one-hot / zero float vectors:
    the GLOBAL inputs (a rank only touches its own block).  Returns (all_rows (N,Tf,265) on every rank, (start, stop) of
    this rank's block); a rank with an empty block contributes a (0,Tf,265) shard.
    """
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    n = mfcc.shape[0]
    a, b = shard_range(n, rank, world)
    local = whole_body_local(body, face, mfcc[a:b], ids[a:b], wav[a:b], face_ids[a:b], mode=mode, seed=seed,
                             clip_index0=a, batch_body=batch_body, batch_face=batch_face, stand=stand)
    return gather_sequences(local, n), (a, b)
