"""Host side of the op-level tests of the VQ glue kernels (csrc/vq.hip: gather_rows, pad_rows, mask_codes / mask_logprob, iota_i64, i64_to_i32,
set_words3, row_sqnorm) and the session staging kernels (csrc/body_stream.hip: stream_stage_mfcc, stream_emit, stream_keep_rows).  No GPU: the
GPU side is tests/test_gpu_glue_ops.py, which imports the restatements, the payloads and the case tables below.

The restatements are numpy statements of the DOCUMENTED contracts (the comments of csrc/kernels.h, the header of csrc/body_stream.hip,
include/talkshow_hip_debug.h), written on whole arrays: none of them walks a flat thread index as the kernels do.  Each takes the image of an
output buffer BEFORE the call and returns its image AFTER it, so "what is written" and "what is left alone" are one comparison.  The tests
here hold every restatement against plain Python loops over (clip, row, column) on tiny shapes, so that a vectorisation slip in a
restatement cannot hide the same slip in a kernel, and check that the case tables reach the edges they are there for.

Floats that are only MOVED travel as uint32 bit patterns (payload): NaNs with payloads, a signalling NaN, denormals, -0.0, infinities among
random words.  A copy that went through arithmetic, or flushed a denormal, changes bits."""
import numpy as np
import pytest

U32, I32, I64, F32, F64 = np.uint32, np.int32, np.int64, np.float32, np.float64
SENTINEL = 0x7FE5A5A5                       # a quiet NaN with a payload no arithmetic produces (tests/test_gpu_wino.py)
QNAN = 0x7FC00000
SPECIALS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x007FFFFF], U32)
STAGE_ROUND = 2048 * 256                    # elements one round of the staging kernels' grid-stride loop covers (stage_blocks caps at 2048 x 256)


def payload(rng, shape):
    """random uint32 words with every SPECIALS pattern among them (where there is room), none equal to the sentinel"""
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(U32)
    flat = a.reshape(-1)
    if flat.size:
        pos = rng.choice(flat.size, size=min(flat.size, max(len(SPECIALS), flat.size // 16)), replace=False)
        flat[pos] = np.resize(SPECIALS, pos.size)
        flat[flat == SENTINEL] = 0x12345678
    return a


def sentinel(shape, dtype=U32):
    """a buffer of `shape` whose every 32-bit word is the sentinel"""
    words = np.dtype(dtype).itemsize // 4
    return np.full(int(np.prod(shape, dtype=np.int64)) * words, SENTINEL, U32).view(dtype).reshape(shape)


# ----------------------------------------------------------------------------------------------- restatements
def gather_ref(table, nrows, idx, idx_stride, width, out_before, L=0, lens=None, len_shr=0):
    """table (>= nrows, ld_table) words, idx flat int64, out_before (M, ldo) -> (out after, mask of the elements that are "some NaN").
    Row m takes table[idx[m idx_stride]][:width]; an index outside [0, nrows) makes the row NaN; with lens, row m = b L + t of a clip
    with t >= lens[b] >> len_shr is +0.0 whatever its index; out[:, width:] is left alone."""
    out = out_before.copy()
    M = out.shape[0]
    r = np.asarray(idx, I64)[::idx_stride][:M]
    bad = (r < 0) | (r >= nrows)
    out[:, :width] = table[np.where(bad, 0, r), :width]
    out[bad, :width] = QNAN
    nan = np.zeros(out.shape, bool)
    nan[bad, :width] = True
    if lens is not None:
        beyond = (np.arange(L)[None, :] >= (np.asarray(lens)[:, None] >> len_shr)).reshape(-1)
        out[beyond, :width] = 0
        nan[beyond] = False
    return out, nan


def pad_ref(src, c, cpad, out_before, L=0, lens=None):
    """src (M, lds) words, out_before (M, ldd) -> out after: columns [0, c) copied, [c, cpad) +0.0, [cpad, ldd) left alone; with lens, row
    m = b L + t with t >= lens[b] is +0.0 in [0, cpad)."""
    out = out_before.copy()
    out[:, :cpad] = 0
    out[:, :min(c, cpad)] = src[:, :min(c, cpad)]
    if lens is not None:
        beyond = (np.arange(L)[None, :] >= np.asarray(lens)[:, None]).reshape(-1)
        out[beyond, :cpad] = 0
    return out


def mask_ref(block, lens, fill):
    """block (B, H, 2): rows r >= lens[b] >> 2 become `fill`, the others stay"""
    B, H, _ = block.shape
    beyond = np.arange(H)[None, :] >= (np.asarray(lens)[:, None] >> 2)
    return np.where(beyond[:, :, None], np.asarray(fill, block.dtype), block)


def iota_ref(n, first):
    return I64(first) + np.arange(n, dtype=I64)


def sqnorm_ref(e):
    return (e.astype(F64) ** 2).sum(axis=1)


def stage_ref(tail, chunk, n_tail, Tw, next0, n_next, next_before):
    """tail (B, cap, 64), chunk (B, t, 64), next_before (B, cap, 64) -> (win (B, Tw, 64), next after): frames of [tail[:n_tail] | chunk]"""
    cat = np.concatenate([tail[:, :n_tail], chunk], axis=1)
    nxt = next_before.copy()
    nxt[:, :n_next] = cat[:, next0:next0 + n_next]
    return cat[:, :Tw].copy(), nxt


def emit_ref(hist, ring_before, A, n, v0, Hw):
    """hist (B, A + n, 2): the code pair of EVERY row of the clips so far (rows [A, A + n) are the call's `codes`); ring_before (B, RC, 2).
    -> (ring after, lat_body (B, Hw), lat_hand (B, Hw)): row r lives at slot r % RC, so after the call a slot holds the latest row <
    A + n of its residue if that row is new, and what it held otherwise; the latent columns are rows [v0, v0 + Hw) of the history."""
    RC = ring_before.shape[1]
    ring = ring_before.copy()
    slots = np.arange(RC)
    latest = (A + n - 1) - ((A + n - 1 - slots) % RC)          # the last row below A + n with row % RC == slot (may be < A, or < 0)
    new = latest >= A
    ring[:, new] = hist[:, latest[new]]
    win = hist[:, v0:v0 + Hw]
    return ring, win[:, :, 0].copy(), win[:, :, 1].copy()


def ring_holding(hist, junk, A):
    """the ring a session holds before a call at A rows: junk (B, RC, 2) with every row r in [max(0, A - RC), A) at slot r % RC"""
    ring = junk.copy()
    RC = ring.shape[1]
    for r in range(max(0, A - RC), A):
        ring[:, r % RC] = hist[:, r]
    return ring


def keep_ref(src, r0, n):
    return src[:, r0:r0 + n].copy()


# ----------------------------------------------------------------------------------------------- case tables (shared with the GPU file)
GATHER_WIDTHS = (4, 256, 260, 1024)          # float4 per row: 1 (one lane), 64 (every lane once), 65 (the lane loop's second round), 256 (4 rounds)
GATHER_MS = (1, 3, 4, 5, 9)                  # 4 rows per workgroup: partial, exact, one over, two and a quarter
GATHER_STRIDES = (1, 2)
GATHER_NROWS = (1, 70)
GATHER_BAD = (-1, None, 2 ** 40)             # None = nrows itself, the first index past the table
GATHER_MASKED = ((9, (36, 21, 0, 7), 2), (9, (9, 5, 0), 0))          # (L, lens, len_shr)
PAD_SHAPES = ((39, 129, 40, 40), (90, 129, 96, 96), (4, 4, 4, 8), (1, 3, 32, 32))          # (c, lds, cpad, ldd)
PAD_ROWS = (1, 257)                          # 257 rows of cpad = 4: 1028 elements, past one 256-thread block (and 4 of them)
PAD_MASKED = (9, (9, 5, 0, 12))              # (L, lens): lens > L is legal
MASK_SHAPES = ((1, 1), (3, 9), (5, 103))     # (B, H): B H = 1, 27, 515 (three blocks)
IOTA_CASES = tuple((n, first) for n in (1, 256, 257) for first in (0, 2 ** 33))
I32_NS = (1, 257)
SQNORM_SHAPES = ((1, 4), (257, 64), (70, 32))
# (n_tail, t, Tw, next0, n_next) at cap = 12: a window wholly in the chunk; windows straddling the seam; wholly in the tail; the zero-unit call;
# a window and no next; a seam inside both; and (added to the issue's six) no window and a next across the seam
STAGE_CASES = ((0, 8, 8, 4, 4), (5, 7, 12, 3, 9), (12, 0, 12, 0, 12), (3, 4, 0, 7, 0), (3, 4, 7, 0, 0), (4, 4, 5, 3, 5), (3, 4, 0, 2, 4))
STAGE_CAP = 12
STAGE_BIG = dict(B=8, n_tail=10, t=4096, Tw=4090, next0=4096, n_next=10, cap=16)
# (n, A, v0, Hw) at RC = 8
EMIT_CASES = ((4, 0, 0, 4), (4, 6, 4, 6), (8, 8, 8, 8), (3, 13, 8, 8), (0, 5, 2, 3), (4, 5, 5, 0), (1, 7, 0, 8))
EMIT_RC = 8
EMIT_BIG = dict(B=64, n=8192, A=8, v0=4, RC=8200, Hw=16)
# (R, r0, n, W)
KEEP_CASES = ((9, 0, 9, 129), (9, 8, 1, 129), (9, 2, 0, 129), (5, 1, 3, 256), (5, 1, 3, 4))
KEEP_BIG_SCALAR = dict(B=2, R=2100, r0=1, n=2050, W=129)
KEEP_BIG_VEC = dict(B=4, R=2051, r0=1, n=2050, W=256)


def mask_lens_tables(B, H):
    """int32 tables (B,) of pose-frame counts 4 r + (k % 4), k counting clips across the tables, whose r between them cover 0, 1, H - 1, H, H + 3"""
    rs = sorted({0, 1, H - 1, H, H + 3})
    tables = []
    for j in range(-(-len(rs) // B)):
        tables.append(np.array([4 * rs[(j * B + b) % len(rs)] + ((j * B + b) % 4) for b in range(B)], I32))
    return tables


def gather_data(rng, width, M, idx_stride, nrows, roomy, bad=(), masked=None):
    """One gather case.  roomy: ld_table = width + 8, ldo = width + 4 (else both = width).  bad: {row: index} planted out of range.
    masked (L, lens, len_shr): M = len(lens) L, the index slots of rows beyond a clip hold 2^40 and -1.
    -> dict(ins, before, want, nan, args)"""
    ld_table, ldo = (width + 8, width + 4) if roomy else (width, width)
    table = payload(rng, (nrows, ld_table))
    idx = np.full(M * idx_stride, 2 ** 41 + 5, I64)          # the slots between the strided ones: never to be used
    idx[::idx_stride] = rng.integers(0, nrows, M)
    for m, v in dict(bad).items():
        idx[m * idx_stride] = v
    L, lens, shr = masked if masked else (0, None, 0)
    if masked:
        assert M == len(lens) * L
        for m in range(M):
            if m % L >= (lens[m // L] >> shr):
                idx[m * idx_stride] = (2 ** 40, -1)[m % 2]
    before = sentinel((M, ldo))
    want, nan = gather_ref(table, nrows, idx, idx_stride, width, before, L, lens, shr)
    ins = dict(table=table, idx=idx)
    if masked:
        ins["lens"] = np.array(lens, I32)
    return dict(ins=ins, before=dict(out=before), want=dict(out=want), nan=dict(out=nan),
                args=dict(ld_table=ld_table, nrows=nrows, idx_stride=idx_stride, M=M, width=width, ldo=ldo, L=L, len_shr=shr))


def pad_data(rng, c, lds, cpad, ldd, B, L, lens=None):
    M = B * L
    src = payload(rng, (M, lds))
    src[:, c:] = QNAN                                         # what lies beside the c channels must not reach dst
    if lens is not None:
        for b in range(B):
            src[b * L + min(L, lens[b]):(b + 1) * L] = QNAN   # nor the rows beyond a clip
    before = sentinel((M, ldd))
    want = pad_ref(src, c, cpad, before, L, lens)
    ins = dict(src=src)
    if lens is not None:
        ins["lens"] = np.array(lens, I32)
    return dict(ins=ins, before=dict(dst=before), want=dict(dst=want), args=dict(lds=lds, c=c, ldd=ldd, cpad=cpad, B=B, L=L))


def stage_data(rng, B, cap, n_tail, t, Tw, next0, n_next):
    tail, chunk = payload(rng, (B, cap, 64)), payload(rng, (B, t, 64))
    before = sentinel((B, cap, 64))
    win, nxt = stage_ref(tail, chunk, n_tail, Tw, next0, n_next, before)
    return dict(ins=dict(tail=tail, chunk=chunk), before=dict(win=sentinel((B, Tw, 64)), next=before), want=dict(win=win, next=nxt),
                args=dict(B=B, n_tail=n_tail, t=t, cap=cap, Tw=Tw, next0=next0, n_next=n_next))


def emit_data(rng, B, RC, n, A, v0, Hw):
    """The history of the clips is random codes with the int64 extremes among them; the ring holds what a session's ring holds at A rows."""
    hist = rng.integers(0, 2048, (B, A + n, 2)).astype(I64)
    if hist.size >= 4:
        hist.reshape(-1)[rng.choice(hist.size, 4, replace=False)] = (-1, 2 ** 63 - 1, -2 ** 63, 2 ** 40 + 3)
    junk = rng.integers(-2 ** 62, -2 ** 61, (B, RC, 2)).astype(I64)          # no code of the history
    ring = ring_holding(hist, junk, A)
    ring_after, lb, lh = emit_ref(hist, ring, A, n, v0, Hw)
    return dict(ins=dict(codes=hist[:, A:A + n].copy()), before=dict(ring=ring, lat_body=sentinel((B, Hw), I64), lat_hand=sentinel((B, Hw), I64)),
                want=dict(ring=ring_after, lat_body=lb, lat_hand=lh), args=dict(B=B, n=n, A=A, RC=RC, v0=v0, Hw=Hw))


def keep_data(rng, B, R, r0, n, W):
    src = payload(rng, (B, R, W))
    return dict(ins=dict(src=src), before=dict(dst=sentinel((B, n, W))), want=dict(dst=keep_ref(src, r0, n)),
                args=dict(B=B, R=R, r0=r0, n=n, W=W))


def stage_units(B, Tw, n_next, **_):
    return (B * Tw + B * n_next) * 16


def emit_units(B, n, Hw, **_):
    return B * n + B * Hw


def keep_units(B, n, W, vec, **_):
    return B * n * W // (4 if vec else 1)


# ----------------------------------------------------------------------------------------------- the restatements against plain loops
def test_gather_ref_against_loops():
    rng = np.random.default_rng(1)
    for masked in (None, (3, (8, 5, 0), 2), (3, (3, 1, 0), 0)):
        for stride in (1, 2):
            M, width, nrows = (9 if masked else 7), 8, 5
            d = gather_data(rng, width, M, stride, nrows, True, bad={0: -1, 1: nrows, 3: 2 ** 40}, masked=masked)
            table, idx, a = d["ins"]["table"], d["ins"]["idx"], d["args"]
            out, nan = d["before"]["out"].copy(), np.zeros((M, a["ldo"]), bool)
            for m in range(M):
                if masked and m % masked[0] >= masked[1][m // masked[0]] >> masked[2]:
                    for k in range(width):
                        out[m, k] = 0
                    continue
                r = int(idx[m * stride])
                for k in range(width):
                    if 0 <= r < nrows:
                        out[m, k] = table[r, k]
                    else:
                        out[m, k], nan[m, k] = QNAN, True
            assert np.array_equal(out, d["want"]["out"]) and np.array_equal(nan, d["nan"]["out"])
            assert np.all(out[:, width:] == SENTINEL) and nan.any() and (not masked or (out[:, :width] == 0).all(axis=1).any())


def test_pad_ref_against_loops():
    rng = np.random.default_rng(2)
    for c, lds, cpad, ldd in ((3, 5, 4, 6), (4, 4, 4, 4), (1, 3, 8, 8)):
        for B, L, lens in ((1, 5, None), (3, 4, (4, 2, 0)), (2, 3, (7, 1))):
            d = pad_data(rng, c, lds, cpad, ldd, B, L, lens)
            src, out = d["ins"]["src"], d["before"]["dst"].copy()
            for b in range(B):
                for t in range(L):
                    for k in range(cpad):
                        live = k < c and (lens is None or t < lens[b])
                        out[b * L + t, k] = src[b * L + t, k] if live else 0
            assert np.array_equal(out, d["want"]["dst"])
            assert not np.any(out[:, :cpad] == QNAN) or c == 0      # the planted NaNs stayed outside


def test_mask_ref_against_loops():
    rng = np.random.default_rng(3)
    for B, H in MASK_SHAPES[:2]:
        for lens in mask_lens_tables(B, H):
            codes = rng.integers(0, 2048, (B, H, 2)).astype(I64)
            lp = payload(rng, (B, H, 2))
            wc, wl = codes.copy(), lp.copy()
            for b in range(B):
                for r in range(H):
                    if r >= lens[b] // 4:
                        wc[b, r, 0] = wc[b, r, 1] = -1
                        wl[b, r, 0] = wl[b, r, 1] = 0
            assert np.array_equal(mask_ref(codes, lens, -1), wc) and np.array_equal(mask_ref(lp, lens, 0), wl)


def test_mask_lens_tables_cover_the_edges():
    for B, H in MASK_SHAPES:
        tabs = mask_lens_tables(B, H)
        assert {int(v) >> 2 for t in tabs for v in t} == {0, 1, H - 1, H, H + 3}
        assert all(t.shape == (B,) for t in tabs)
        assert B == 1 or {int(v) & 3 for t in tabs for v in t} >= {1, 2}      # frame counts that are no multiple of 4


def test_small_refs_against_loops():
    assert iota_ref(3, 2 ** 33).tolist() == [2 ** 33, 2 ** 33 + 1, 2 ** 33 + 2] and iota_ref(1, 0).tolist() == [0]
    e = np.array([[1.5, -2.0, 0.25], [0.0, 4.0, -4.0]], F32)
    assert sqnorm_ref(e).tolist() == [sum(float(v) ** 2 for v in row) for row in e]
    assert sentinel((2, 3), I64).view(U32).tolist() == [[SENTINEL] * 6] * 2


def test_stage_ref_against_loops():
    rng = np.random.default_rng(4)
    for n_tail, t, Tw, next0, n_next in STAGE_CASES:
        d = stage_data(rng, 2, STAGE_CAP, n_tail, t, Tw, next0, n_next)
        tail, chunk = d["ins"]["tail"], d["ins"]["chunk"]
        win, nxt = d["before"]["win"].copy(), d["before"]["next"].copy()

        def frame(b, j):
            return tail[b, j] if j < n_tail else chunk[b, j - n_tail]
        for b in range(2):
            for j in range(Tw):
                for q in range(64):
                    win[b, j, q] = frame(b, j)[q]
            for j in range(n_next):
                for q in range(64):
                    nxt[b, j, q] = frame(b, next0 + j)[q]
        assert np.array_equal(win, d["want"]["win"]) and np.array_equal(nxt, d["want"]["next"])
        assert np.all(nxt[:, n_next:] == SENTINEL)


def test_emit_ref_against_a_dictionary():
    rng = np.random.default_rng(5)
    for n, A, v0, Hw in EMIT_CASES + ((2, 21, 17, 5),):
        B, RC = 2, EMIT_RC
        d = emit_data(rng, B, RC, n, A, v0, Hw)
        codes, ring0 = d["ins"]["codes"], d["before"]["ring"]
        for b in range(B):
            held = {}                                        # row -> code pair, as a reader of the ring and the step sees it
            slot = {s: tuple(ring0[b, s]) for s in range(RC)}
            for r in range(max(0, A - RC), A):
                held[r] = tuple(ring0[b, r % RC])
            for i in range(n):
                held[A + i] = tuple(codes[b, i])
                slot[(A + i) % RC] = tuple(codes[b, i])
            for s in range(RC):
                assert tuple(d["want"]["ring"][b, s]) == slot[s]
            for h in range(Hw):
                assert (d["want"]["lat_body"][b, h], d["want"]["lat_hand"][b, h]) == held[v0 + h]


def test_keep_ref_against_loops():
    rng = np.random.default_rng(6)
    for R, r0, n, W in ((4, 1, 2, 3), (3, 0, 3, 4), (3, 2, 0, 5)):
        d = keep_data(rng, 2, R, r0, n, W)
        out = d["before"]["dst"].copy()
        for b in range(2):
            for i in range(n):
                for k in range(W):
                    out[b, i, k] = d["ins"]["src"][b, r0 + i, k]
        assert np.array_equal(out, d["want"]["dst"])


# ----------------------------------------------------------------------------------------------- the tables reach what they are there for
def test_payload_holds_the_special_patterns():
    p = payload(np.random.default_rng(7), (40, 8))
    assert set(SPECIALS.tolist()) <= set(p.reshape(-1).tolist()) and not np.any(p == SENTINEL)
    f = p.view(F32)
    assert np.isnan(f).any() and np.any((f != 0) & (np.abs(f) < np.finfo(F32).tiny)) and np.any(p == 0x80000000)


def test_case_tables_obey_the_launchers_rules():
    """every staging case is a call the launchers accept (csrc/body_stream.hip), and the edges named in the GPU file's table are there"""
    for n_tail, t, Tw, next0, n_next in STAGE_CASES + (tuple(STAGE_BIG[k] for k in ("n_tail", "t", "Tw", "next0", "n_next")),):
        cap = STAGE_CAP if t < 100 else STAGE_BIG["cap"]
        assert 0 <= n_tail <= cap and 0 <= n_next <= cap and Tw <= n_tail + t and next0 + n_next <= n_tail + t
    assert any(Tw and Tw <= nt for nt, t, Tw, _, _ in STAGE_CASES) and any(nt == 0 and Tw for nt, t, Tw, _, _ in STAGE_CASES)
    assert any(0 < nt < Tw for nt, t, Tw, _, _ in STAGE_CASES) and any(Tw == 0 and nn == 0 for _, _, Tw, _, nn in STAGE_CASES)
    assert any(Tw == 0 and nn for _, _, Tw, _, nn in STAGE_CASES) and any(Tw and nn == 0 for _, _, Tw, _, nn in STAGE_CASES)
    for n, A, v0, Hw in EMIT_CASES + (tuple(EMIT_BIG[k] for k in ("n", "A", "v0", "Hw")),):
        RC = EMIT_RC if n < 100 else EMIT_BIG["RC"]
        assert v0 <= A and A + n - v0 <= RC and v0 + Hw <= A + n
    assert any(A % EMIT_RC + n > EMIT_RC for n, A, _, _ in EMIT_CASES)                    # a wrap inside the append
    assert sum(A + n - v0 == EMIT_RC for n, A, v0, _ in EMIT_CASES) >= 2                   # the ring exactly full
    assert any(v0 == A and Hw for n, A, v0, Hw in EMIT_CASES) and any(n == 0 and Hw for n, A, v0, Hw in EMIT_CASES)
    assert any(Hw == 0 and n for n, A, v0, Hw in EMIT_CASES) and any(v0 < A < v0 + Hw for n, A, v0, Hw in EMIT_CASES)
    for R, r0, n, W in KEEP_CASES:
        assert 0 <= r0 and r0 + n <= R


def test_grid_stride_cases_take_a_second_round():
    """a staging launch has at most 2048 blocks of 256 threads: more elements than that and some thread loops again"""
    assert stage_units(**STAGE_BIG) == (8 * 4090 + 8 * 10) * 16 == 524800 > STAGE_ROUND == 524288
    assert emit_units(**EMIT_BIG) == 64 * 8192 + 64 * 16 == 525312 > STAGE_ROUND
    assert keep_units(vec=False, **KEEP_BIG_SCALAR) == 2 * 2050 * 129 == 528900 > STAGE_ROUND
    assert keep_units(vec=True, **KEEP_BIG_VEC) == 4 * 2050 * 256 // 4 == 524800 > STAGE_ROUND
    assert max(stage_units(B=3, Tw=c[2], n_next=c[4]) for c in STAGE_CASES) < 256 * 256      # the small cases stay far below it
    assert KEEP_BIG_SCALAR["W"] % 4 and KEEP_BIG_VEC["W"] % 4 == 0


@pytest.mark.parametrize("width", GATHER_WIDTHS)
def test_gather_widths_are_lane_loop_edges(width):
    rounds = -(-(width // 4) // 64)
    assert width % 4 == 0 and rounds == {4: 1, 256: 1, 260: 2, 1024: 4}[width]
    assert (width // 4) % 64 == {4: 1, 256: 0, 260: 1, 1024: 0}[width]
