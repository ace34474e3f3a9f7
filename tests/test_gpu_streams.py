"""Every pass family OVERLAPPED: the thread contract of include/talkshow_hip.h ("one host thread per stream at a time"; handles hold read-only
weights plus one scratch arena and one graph cache PER STREAM) for what tests/test_gpu_threads.py does not reach — the mixed pass under every
keyword, the per-clip sampler tables, sessions with controls, seamless sessions, the Winograd arenas of the VQ stacks, the face generator's
mixed and packed pass, the mixed audio front end, SMPL-X, the evaluation entries, stream teardown and `ts_pixelcnn_graph_stats`.

EVERY comparison is bit equality with the same call made serially on the default stream; besides equality the module asserts capture
counts and, where threads are meant to overlap, that they did: each thread records an event on its stream before and after each round, and
at least half of the rounds must show two streams' intervals intersecting (a concurrency test that ran serially proves nothing; the counts
are printed).  No tolerance and no timing anywhere.

Models: the shipped wrapper (`bench.build_models(0, seed=7)`: full-size audio encoder and VQ decoders, whose k = 3 stacks of 512+ channels
run on the Winograd arenas) around the small code predictor of the pass tests (input_dim 256, dim 64, n_layers 3), and `bench.build_face(0)`.
Clips are the pass tests' 20, 17, 17, 9, 8 and 3 code rows and subsets: two chunks and a half, ties, a clip shorter than a chunk.  At most
three library streams exist at a time, beside the default stream.

Every barrier wait and every join carries a timeout; a thread that raises aborts the barrier; a thread still alive after its join fails the
test; nothing is retried.
"""
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from talkshow_amd import synth
from test_gpu_bias_pass import DIMS, NC, RECS, ROWS, V, _pix, _tables
from test_gpu_eval_ops import body_inputs
from test_gpu_seamless import draw as session_draw
from test_gpu_smplx_ops import forward_inputs, model_by_name
from test_gpu_stream_ctl import REPS, Case

pytestmark = pytest.mark.gpu
F32 = np.float32
BARRIER_S, JOIN_S = 120, 600
KINDS = ("records", "given", "motion", "plain")          # between them: every keyword of the mixed pass, and the pass without any
CLIPS = {6: ROWS, 4: [20, 17, 9, 3], 5: [17, 17, 9, 8, 3], 2: [17, 8], 9: ROWS + [17, 9, 3]}


@pytest.fixture(scope="module")
def env():
    import bench
    from talkshow_amd import _lib
    pix = _pix(synth.pixelcnn_state_dict(seed=11, **DIMS))
    w = bench.build_models(0, seed=7)[0]
    w.generator = pix
    e = SimpleNamespace(_lib=_lib, lib=_lib.load(), w=w, pix=pix, face=bench.build_face(0), clips={})
    for n, rows in CLIPS.items():
        lens = [4 * h + (k + n) % 4 for k, h in enumerate(rows)]
        e.clips[n] = SimpleNamespace(rows=rows, mf=[synth.mfcc_features(4000 + 10 * n + k, 1, t)[0] for k, t in enumerate(lens)],
                                     ids=((np.arange(len(rows)) + n) % NC).astype(np.int64))
    yield e
    torch.cuda.synchronize()


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _host(x):
    """Device tensors anywhere inside lists, tuples and dicts -> numpy (the copy waits for the current stream)."""
    if torch.is_tensor(x):
        return x.cpu().numpy()
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    return x


def _where(a, b, at="result"):
    """None if a and b hold the same BITS throughout, else the path of the first difference."""
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return at
        return next((d for d in (_where(x, y, f"{at}[{i}]") for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, dict):
        if not isinstance(b, dict) or sorted(a) != sorted(b):
            return at
        return next((d for d in (_where(a[k], b[k], f"{at}[{k!r}]") for k in sorted(a)) if d), None)
    a, b = np.asarray(a), np.asarray(b)
    return None if a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() else at


def opts(e, kind, rows, seed):
    """The keywords of one mixed pass over clips of `rows` code rows, as fresh host arrays: `kind` picks the set, `seed` the content."""
    rng = np.random.default_rng(seed)
    B = len(rows)
    kw = dict(mode=e._lib.TS_SAMPLE_PHILOX, seed=1000 + seed, clip_index0=7 * seed)
    if kind == "records":            # sampling records, log-probabilities, repetition penalty
        kw.update(sampling=[RECS[(b + seed) % len(RECS)] for b in range(B)], logprobs=True, repeat=[REPS[(b + seed) % len(REPS)] for b in range(B)])
    elif kind == "given":            # given codes under masks of kept positions, code bias, log-probabilities
        tabs = _tables(seed)
        kw.update(given=[rng.integers(0, V, ((h + 1) // 2, 2)) if b % 2 == 0 else None for b, h in enumerate(rows)],
                  given_keep=[("body", None, "hand", None)[b % 4] for b in range(B)], code_bias=[tabs[(b + seed) % len(tabs)] for b in range(B)],
                  logprobs=True)
    elif kind == "motion":           # given poses; style as the id, as a per-clip row and as a per-row track
        kw.update(given_poses=[synth.gt_poses(50 * seed + b, 1, 4 * ((h + 1) // 2) + 1)[0] if b % 2 == 1 else None for b, h in enumerate(rows)],
                  style=[(None, rng.random(NC).astype(F32), rng.random((h, NC)).astype(F32))[b % 3] for b, h in enumerate(rows)])
    elif kind == "tracks":           # a style track on every clip and a table on every clip: bias_tab and style_int follow the Work's capacity
        tabs = [t for t in _tables(seed) if t is not None]
        kw.update(style=[rng.random((h, NC)).astype(F32) for h in rows], code_bias=[tabs[(b + seed) % len(tabs)] for b in range(B)], logprobs=True)
    else:
        assert kind == "plain"
    return kw


def scribble(x):
    """Overwrites every host array inside x in place: whatever reads it after this reads something else."""
    if isinstance(x, np.ndarray):
        x.fill(V + 7 if x.dtype.kind in "iu" else 1e30)
    elif isinstance(x, dict):
        [scribble(v) for v in x.values()]
    elif isinstance(x, (list, tuple)):
        [scribble(v) for v in x]


def mixed(e, n, kind, seed):
    c = e.clips[n]
    return e.w.generate_clips(c.mf, c.ids, **opts(e, kind, c.rows, seed))


def overlapped_rounds(base, marks):
    """marks[t][r] = (event before, event after) of thread t's round r, or None -> the rounds in which two streams' intervals intersect."""
    n = 0
    for r in range(len(marks[0])):
        iv = [(base.elapsed_time(m[r][0]), base.elapsed_time(m[r][1])) for m in marks if m[r] is not None]
        n += any(max(a[0], b[0]) < min(a[1], b[1]) for i, a in enumerate(iv) for b in iv[i + 1:])
    return n


def crew(streams, rounds, work, main=None):
    """One host thread per stream; every round starts behind a barrier; work(t, r) runs on the calling thread's current stream and returns
    device tensors (nested).  main(threads) runs on the calling thread meanwhile.  -> (got[t][r] as numpy, overlapped rounds, main's result)."""
    n = len(streams)
    gate = threading.Barrier(n)
    got, marks, errors = [[None] * rounds for _ in range(n)], [[None] * rounds for _ in range(n)], []
    torch.cuda.synchronize()
    base = torch.cuda.Event(enable_timing=True)
    base.record()

    def body(t):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    gate.wait(timeout=BARRIER_S)                     # all enter the library together, every round
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out = work(t, r)
                    b.record()
                    streams[t].synchronize()
                    got[t][r], marks[t][r] = _host(out), (a, b)
        except Exception as ex:                                      # noqa: BLE001
            errors.append((t, repr(ex)))
            gate.abort()

    th = [threading.Thread(target=body, args=(t,)) for t in range(n)]
    for x in th:
        x.start()
    extra = None
    try:
        if main is not None:
            extra = main(th)
    finally:
        for x in th:
            x.join(timeout=JOIN_S)
    alive = [t for t, x in enumerate(th) if x.is_alive()]
    assert not alive, f"threads {alive} are still running {JOIN_S} s after the others ended"
    assert not errors, errors
    torch.cuda.synchronize()
    return got, overlapped_rounds(base, marks), extra


def serial(n, rounds, work):
    """The same rounds, one after the other, on the default stream."""
    want = [[_host(work(t, r)) for r in range(rounds)] for t in range(n)]
    torch.cuda.synchronize()
    return want


def assert_same(got, want, what):
    for t, (g, w) in enumerate(zip(got, want)):
        for r, (a, b) in enumerate(zip(g, w)):
            d = _where(a, b)
            assert d is None, f"{what}: thread {t} round {r}: {d} differs from the serial run on the default stream"


def destroy(e, streams):
    for s in streams:
        e._lib.check(e.lib.ts_stream_destroy(e._lib.context(0), s.cuda_stream))


def assert_overlap(what, seen, rounds):
    print(f"\n[overlap] {what}: {seen} of {rounds} rounds had two streams busy at once")
    assert 2 * seen >= rounds, f"{what}: only {seen} of {rounds} rounds overlapped on the device: the test ran serially and shows nothing"


# ---- 1. every keyword of the mixed pass, one thread per stream -----------------------------------------------------------------------------
def test_every_keyword_of_the_mixed_pass_one_thread_per_stream(env):
    """Threads of 6, 4 and 5 clips (other Work capacities, other strides, other graph keys), four rounds, the option set rotating from round
    to round: a stream's Work meets tables of other content and other sampler bits on graphs that are warm or evicted.  Codes, poses and
    log-probabilities equal the serial run; per stream and round, `graph_captures` equals the count of the same sequence run alone on a
    fresh stream (so rounds 2 to 4 capture nothing a serial run does not)."""
    e, sizes, ROUNDS = env, (6, 4, 5), 4

    def work(t, r):
        out = mixed(e, sizes[t], KINDS[(t + r) % len(KINDS)], 10 * t + r)
        return out, e.pix.graph_captures()

    want = serial(3, ROUNDS, work)
    assert _where(want[0][0][0], want[0][1][0]) is not None                    # the rounds differ: the options reached the pass
    streams = e._lib.create_streams(3, 0)
    alone = []
    for t, s in enumerate(streams):                                            # the same sequences, one after the other, on fresh streams
        with torch.cuda.stream(s):
            alone.append([_host(work(t, r)) for r in range(ROUNDS)])
            s.synchronize()
    destroy(e, streams)
    streams = e._lib.create_streams(3, 0)
    try:
        got, seen, _ = crew(streams, ROUNDS, work)
    finally:
        destroy(e, streams)
    for t in range(3):
        for r in range(ROUNDS):
            assert _where(alone[t][r][0], want[t][r][0]) is None, f"thread {t}'s pass of round {r} ALONE on a library stream differs from the default stream"
            d = _where(got[t][r][0], want[t][r][0])
            assert d is None, f"thread {t} round {r} ({KINDS[(t + r) % len(KINDS)]}, {sizes[t]} clips): {d} differs from the serial run"
        assert [g[1] for g in got[t]] == [a[1] for a in alone[t]], \
            f"stream {t}: captures per round {[g[1] for g in got[t]]} under threads, {[a[1] for a in alone[t]]} for the same sequence alone"
        assert got[t][0][1] > 0
    assert_overlap("mixed pass, three threads", seen, ROUNDS)


# ---- 2. one host thread, three streams, nothing synchronised in between ----------------------------------------------------------------------
def test_one_thread_queues_nine_passes_on_three_streams(env):
    """The benchmark's headline shape.  Every pass brings its own clips and tables as host arrays that are overwritten and deleted as soon as
    the call returns: nothing on the host has to outlive the call, and the conv stacks, Winograd arenas and chains of different passes
    overlap on the device."""
    e, sizes = env, (6, 4, 5)
    passes = [(i % 3, KINDS[i % len(KINDS)], 100 + i) for i in range(9)]
    want = [_host(mixed(e, sizes[k], kind, seed)) for k, kind, seed in passes]
    torch.cuda.synchronize()
    streams = e._lib.create_streams(3, 0)
    try:
        outs = []
        for k, kind, seed in passes:
            c = e.clips[sizes[k]]
            with torch.cuda.stream(streams[k]):
                mf, ids, kw = [m.copy() for m in c.mf], c.ids.copy(), opts(e, kind, c.rows, seed)
                outs.append(e.w.generate_clips(mf, ids, **kw))
                scribble([mf, ids, kw])
                del mf, ids, kw
        torch.cuda.synchronize()                                               # once, at the end
        got = _host(outs)
    finally:
        destroy(e, streams)
    for i, (k, kind, seed) in enumerate(passes):
        d = _where(got[i], want[i])
        assert d is None, f"pass {i} ({kind}, {sizes[k]} clips, stream {k}): {d} differs from the serial run"


# ---- 3. sessions ---------------------------------------------------------------------------------------------------------------------------------
class Sessions:
    """Three sessions of five calls each and their one-shot yardsticks (tests/test_gpu_stream_ctl.py, tests/test_gpu_seamless.py)."""
    CALLS = 5

    def __init__(self, e):
        self.e = e
        rng = np.random.default_rng(77)
        B = 6
        self.case = Case(e.pix, np.arange(B) % NC, rng.standard_normal((B, 10, 256)).astype(F32), 9)
        self.ctl = dict(sampling=self.case.sampling, code_bias=self.case.bias, repeat=self.case.repeat, logprobs=True)
        self.ctl_sched = (3, 1, 2, 2, 2)
        self.sB, self.sT, self.s_sched = 2, 150, (64, 23, 41, 22)          # uneven pushes, then the flush
        self.s_mf = torch.from_numpy(synth.mfcc_features(31, self.sB, self.sT)).cuda()
        self.s_ids = synth.speaker_ids(self.sB)
        self.pB, self.p_sched = 3, (3, 4, 2, 4, 3)                          # code rows per push of the plain session
        self.p_mf = torch.from_numpy(synth.mfcc_features(500, self.pB, 4 * sum(self.p_sched))).cuda()
        self.p_ids = np.array([1, 0, 2], np.int64)
        self.live = {}

    def yardsticks(self):
        """The one-shot calls, on the default stream -> what call r of session t must return."""
        e, c, d = self.e, self.case, session_draw("philox")
        codes, lp = c.one_shot("philox", **self.ctl)
        assert not np.array_equal(codes, c.one_shot("philox")), "the controls change nothing here"
        at = np.cumsum((0,) + self.ctl_sched)
        ctl = [[codes[:, a:b], lp[:, a:b].view(F32)] for a, b in zip(at[:-1], at[1:])]
        sc, sp = (_host(x) for x in e.w.generate_batch(self.s_mf, self.s_ids, **d))
        at = np.cumsum((0,) + self.p_sched)
        rows = torch.cat([e.w.audioencoder.forward_nlc(self.p_mf[:, 4 * a:4 * b]) for a, b in zip(at[:-1], at[1:])], 1)
        pc = e.pix.run(self.p_ids, rows, **d)[0]
        plain = [_host(e.w._decode_pair(pc[:, a:b].contiguous())) for a, b in zip(at[:-1], at[1:])]
        torch.cuda.synchronize()
        return ctl, (sc, sp), plain

    def call(self, t, r, only=None):
        """Call r of session t on the current stream (opened at its first call, closed behind its last)."""
        e, d = self.e, session_draw("philox")
        if t == 0:                                                         # PixelCNNStream under sampling, code_bias, repeat, with logprobs
            if r == 0:
                self.live[t] = e.pix.open_stream(self.case.label, self.case.B, max(self.ctl_sched))
            a = sum(self.ctl_sched[:r])
            out = self.live[t].step(self.case.aud[:, a:a + self.ctl_sched[r]], **d, **self.ctl)
        elif t == 1:                                                       # seamless BodyStream: uneven pushes and the flush
            if r == 0:
                self.live[t] = e.w.open_stream(self.s_ids, self.sB, max(self.s_sched), seamless=True)
            if r < len(self.s_sched):
                a = sum(self.s_sched[:r])
                out = self.live[t].push(self.s_mf[:, a:a + self.s_sched[r]], **d, return_codes=True)
            else:
                out = self.live[t].flush(**d, return_codes=True)
        else:                                                              # the plain BodyStream
            if r == 0:
                self.live[t] = e.w.open_stream(self.p_ids, self.pB, 4 * max(self.p_sched))
            a = 4 * sum(self.p_sched[:r])
            out = self.live[t].push(self.p_mf[:, a:a + 4 * self.p_sched[r]], **d)
        out = _host(out)                                                   # (waits for the stream: close() below frees the session's buffers)
        if r == self.CALLS - 1:
            self.live.pop(t).close()
        return out

    def check(self, got, yard, what):
        ctl, (sc, sp), plain = yard
        for r in range(self.CALLS):
            d = _where(got[0][r], ctl[r])
            assert d is None, f"{what}: controlled session, step {r}: {d} differs from the one-shot call"
            d = _where(got[2][r], plain[r])
            assert d is None, f"{what}: plain body session, push {r}: poses differ from the decode of the one-shot call's codes"
        poses, codes = (np.concatenate([g[k] for g in got[1]], 1) for k in (0, 1))
        assert _where(codes, sc) is None and _where(poses, sp) is None, f"{what}: the seamless session differs from generate_batch"


@pytest.fixture(scope="module")
def sessions(env):
    s = Sessions(env)
    return s, s.yardsticks()


def test_three_sessions_in_lockstep_beside_one_shot_passes(env, sessions):
    """A controlled PixelCNNStream, a seamless BodyStream and a plain BodyStream, each on its own thread and stream, call by call behind a
    barrier, while the main thread runs one-shot mixed passes on the default stream against the same handles.  (Sessions are opened
    inside the threads, beside the other threads' first captures: with a synchronous `hipMemcpy` in `ts_pixelcnn_stream_open` the runtime
    refused the copy and invalidated a neighbour's capture — `copy_and_wait` in host_common.h.)"""
    e, (s, yard) = env, sessions
    ref = _host(mixed(e, 6, "records", 3))
    torch.cuda.synchronize()

    def main(threads):
        bad, n = [], 0
        while n == 0 or (n < 40 and any(x.is_alive() for x in threads)):
            d = _where(_host(mixed(e, 6, "records", 3)), ref)
            if d:
                bad.append((n, d))
            n += 1
        return bad, n

    streams = e._lib.create_streams(3, 0)
    try:
        got, seen, (bad, n) = crew(streams, s.CALLS, s.call, main)
    finally:
        s.live.clear()
        destroy(e, streams)
    s.check(got, yard, "three threads")
    assert not bad, f"one-shot passes on the default stream beside the sessions: (pass, first difference) {bad[:4]} of {n}"
    assert_overlap("three sessions in lockstep", seen, s.CALLS)


def test_a_session_moves_to_another_stream_once_the_streams_are_ordered(env, sessions):
    """The rule of include/talkshow_hip.h ("Threads"): a session owns its state and is bound to no stream; a call runs on the stream it is
    given, and a session may continue on another stream once everything it queued on the earlier one has completed.  Two calls on stream A,
    a stream synchronise, the rest on stream B: the one-shot call's bits."""
    e, (s, yard) = env, sessions
    streams = e._lib.create_streams(2, 0)
    try:
        got = [[None] * s.CALLS for _ in range(3)]
        for r in range(s.CALLS):
            with torch.cuda.stream(streams[0 if r < 2 else 1]):
                for t in range(3):
                    got[t][r] = s.call(t, r)
            if r == 1:
                streams[0].synchronize()                                   # the caller orders the two streams
    finally:
        s.live.clear()
        destroy(e, streams)
    s.check(got, yard, "streams A, A, B, B, B")


# ---- 4. growth beside replay ---------------------------------------------------------------------------------------------------------------------
def test_a_work_grows_on_one_stream_beside_replays_on_another(env):
    """Thread A replays one warm pass eight times; thread B runs passes of 2, 5 and 9 clips with style tracks and code bias, each of which
    grows B's Work: `ensure_work` drops B's graphs, bias_tab and style_int are freed and allocated again while A's replays are queued."""
    e, grow, reps = env, (2, 5, 9), (3, 3, 2)

    def b_pass(r):
        return mixed(e, grow[r], "tracks", 40 + r)

    want_a = _host(mixed(e, 6, "given", 5))
    want_b = [_host(b_pass(r)) for r in range(3)]
    torch.cuda.synchronize()
    streams = e._lib.create_streams(2, 0)
    try:
        with torch.cuda.stream(streams[0]):
            warm = _host(mixed(e, 6, "given", 5))
            caps = e.pix.graph_captures()

        def work(t, r):
            if t == 0:
                return [mixed(e, 6, "given", 5) for _ in range(reps[r])], e.pix.graph_captures()
            return b_pass(r), e.pix.graph_captures()

        got, seen, _ = crew(streams, 3, work)
    finally:
        destroy(e, streams)
    assert _where(warm, want_a) is None and caps > 0
    for r in range(3):
        for k, out in enumerate(got[0][r][0]):
            d = _where(out, want_a)
            assert d is None, f"replay {k} of round {r} beside a pass of {grow[r]} clips: {d} differs from the serial run"
        assert got[0][r][1] == caps, f"the replaying stream captured a graph in round {r}: {caps} -> {got[0][r][1]}"
        d = _where(got[1][r][0], want_b[r])
        assert d is None, f"the growing stream's pass of {grow[r]} clips: {d} differs from the serial run"
    assert got[1][0][1] < got[1][1][1] < got[1][2][1], "every growth drops the graphs: each pass captures its own"
    assert_overlap("growth beside replay", seen, 3)


# ---- 5. face, front end, SMPL-X and evaluation -----------------------------------------------------------------------------------------------------
def test_face_front_end_smplx_and_evaluation_on_two_streams(env):
    """Round 0: the face wrapper's `generate_clips` (the library's plan) and the packed plan on recordings of three lengths, beside
    `generate_clips_from_wav` from 44.1 kHz input on the other thread (this module's first use of that Kaiser table: the mutex-guarded
    map's first-use path runs while the other thread is inside the library, which is why the serial run comes AFTER the threads here).
    Round 1: both threads run the SMPL-X forward (joints and vertices, one shared handle) and the four evaluation entries."""
    from nets.smplx_face import TrainWrapper as FaceWrapper
    from talkshow_amd import evaluation as E
    from talkshow_amd.smplx_lbs import SMPLXLayer
    e = env
    fw = object.__new__(FaceWrapper)                                           # the wrapper's generate_clips around bench.build_face(0)
    fw.generator, fw.num_classes = e.face, 4
    fw.config = SimpleNamespace(Data=SimpleNamespace(pose=SimpleNamespace(normalization=False)))
    wav16 = [synth.wav16(7000 + k, 1, n)[0] for k, n in enumerate((5872, 16000, 9001))]
    fid = np.eye(4, dtype=F32)[[1, 0, 3]]
    wav44 = [synth.wav16(8000 + k, 1, n)[0] for k, n in enumerate((9000, 22050, 14001))]
    ids44 = np.array([2, 0, 1], np.int64)
    model = model_by_name("v700")
    layer = SMPLXLayer(model, with_vertices=True)
    inp = []
    for t, N in enumerate((5, 7)):
        rng = np.random.default_rng(900 + t)
        betas, rows = forward_inputs("v700", model, N)
        gt, prs = body_inputs(rng, 2 + t, 9 + t, 55)
        inp.append(dict(betas=betas, rows=rows, x=rng.standard_normal((129 + t, 64)).astype(F32), a=rng.standard_normal((37 + t, 64)).astype(F32),
                        b=rng.standard_normal((37 + t, 64)).astype(F32), k=rng.standard_normal((3 + t, 257, 5)).astype(F32), gt=gt, prs=prs))

    def work(t, r):
        if r == 0 and t == 0:
            return [fw.generate_clips(wav16, [1, 0, 3]), e.face.run_clips(wav16, fid, layout=1), e.face.run_clips(wav16, fid, layout=0)]
        if r == 0:
            return e.w.generate_clips_from_wav(wav44, 44100, ids44, mode=e._lib.TS_SAMPLE_PHILOX, seed=5, clip_index0=3)
        i = inp[t]
        stats = E.FeatureStats(64)
        stats.push(i["x"])
        return [layer.vertices(i["betas"], i["rows"]), stats.acc, E.l1_mean_per_row(i["a"], i["b"]), E.diversity(i["k"]), E.body_loss(i["gt"], i["prs"])]

    streams = e._lib.create_streams(2, 0)
    try:
        got, seen, _ = crew(streams, 2, work)
    finally:
        destroy(e, streams)
    print(f"\n[overlap] face / front end / SMPL-X / evaluation: {seen} of 2 rounds had two streams busy at once (not asserted)")
    want = serial(2, 2, work)
    assert_same(got, want, "face, front end, SMPL-X, evaluation")
    assert _where(got[0][0][0], got[0][0][1]) is None and _where(got[0][0][1], got[0][0][2]) is None    # wrapper, packed and padded plan: same bits
    assert all(np.isfinite(x).all() for x in got[0][1][0]) and all(np.isfinite(p).all() for _, p in got[1][0])


# ---- 6. stream teardown --------------------------------------------------------------------------------------------------------------------------
def test_a_stream_created_after_a_destroy_starts_from_a_fresh_work(env):
    e = env
    want = _host(mixed(e, 5, "records", 61))
    torch.cuda.synchronize()
    first = e._lib.create_streams(1, 0)
    with torch.cuda.stream(first[0]):
        a = _host(mixed(e, 5, "records", 61))
        caps_a = e.pix.graph_captures()
    handle = first[0].cuda_stream
    destroy(e, first)
    assert caps_a > 0 and e.lib.ts_pixelcnn_graph_captures(e.pix.handle(), C.c_void_p(handle)) == 0, "the destroyed stream's Work is still there"
    second = e._lib.create_streams(1, 0)                                       # may receive the same handle value
    try:
        with torch.cuda.stream(second[0]):
            assert e.pix.graph_captures() == 0, "a new stream inherited a Work"
            b = _host(mixed(e, 5, "records", 61))
            caps_b = e.pix.graph_captures()
    finally:
        destroy(e, second)
    print(f"\n[teardown] the second stream {'received' if second[0].cuda_stream == handle else 'did not receive'} the first one's handle value")
    assert caps_b == caps_a, f"the same pass on a fresh Work captures the same graphs: {caps_a} then {caps_b}"
    assert _where(a, want) is None and _where(b, want) is None


# ---- 7. graph statistics under threads -----------------------------------------------------------------------------------------------------------
def test_graph_stats_count_the_capturing_call_alone(env):
    """Two threads capture whole-call graphs (`prepare`) of different shapes behind the same barrier, four times; `ts_pixelcnn_graph_stats`
    of every shape equals what a serial capture of that shape reports.  Counted from context-wide totals, a capture also counts what the
    other thread launches meanwhile."""
    e, mode = env, env._lib.TS_SAMPLE_PHILOX
    shapes = [[(3, H) for H in (20, 19, 18, 17)], [(2, H) for H in (20, 19, 18, 17)]]      # descending: the Work grows once, stats are kept

    def stats(stream, B, H):
        n, f = C.c_int64(), C.c_double()
        e._lib.check(e.lib.ts_pixelcnn_graph_stats(e.pix.handle(), stream, B, H, mode, C.byref(n), C.byref(f)))
        return n.value, f.value

    want = []
    for t in range(2):
        for B, H in shapes[t]:
            e.pix.prepare(B, H, mode)
        want.append([stats(e._lib.stream_ptr(), B, H) for B, H in shapes[t]])
    assert all(n > 0 and f > 0 for row in want for n, f in row) and len({x for row in want for x in row}) == 8
    streams = e._lib.create_streams(2, 0)
    try:
        crew(streams, 4, lambda t, r: e.pix.prepare(*shapes[t][r], mode) and None)
        got = [[stats(C.c_void_p(streams[t].cuda_stream), B, H) for B, H in shapes[t]] for t in range(2)]
    finally:
        destroy(e, streams)
    print(f"\n[graph stats] serial {want}\n[graph stats] under two threads {got}")
    assert got == want, "a capture's statistics hold launches of another thread"
