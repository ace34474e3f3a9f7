"""Numpy twin of the sampler with per-clip controls (`csrc/vq.hip::sample_ctl_kernel`; the rule: `include/talkshow_hip.h`, ts_sampling,
steps 1-5, "code bias": step 0 and the kept-set sentence, `biased` / `keep_mask_bias` / `sample_bias` below, and "repetition penalty":
step 0b, `repeat_counts` / `penalised` / `sample_repeat` / `decode_repeat` below, and "guidance": the rule ahead of step 0 and the host check,
`guided` / `guide_roles` / `sample_guide` below, and "alternatives": `alternatives` / `alternatives_error_bound` / `uncertain_keep`
below).  Pure host code, the device's arithmetic operation for operation: `keep_mask` and `sample_ctl` return what the device returns,
bit for bit, so tests compare indices and kept sets for equality.  A record is (temperature, top_p, top_k), `_lib.sampling_record`'s form.

The kept set is written here from its DEFINITION (sort the row, cumulative integer masses in rank order); the kernel finds the same set by
radix select.  Both use the same integers, and integer sums do not depend on the order they are taken in.
"""
import collections

import numpy as np

F32 = np.float32
NTHREADS = 256
Q_SCALE = 2.0 ** 31      # q_v = floor(w_v * 2^31): the weight as an integer mass


def det_expf(x):
    """exp(x) for x <= 0 as the samplers compute it (`csrc/kernels.h::det_expf`): fp32 multiplies and adds only, one IEEE rounding each,
    no fused multiply-add.  A copy of `oracle.talkshow_oracle.det_expf` (product code does not import the oracle);
    tests/test_sampling_host.py pins the two to each other."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = np.where(x < F32(-86.0), F32(0.0), x).astype(F32)            # the arguments that give 0 take no part below (-inf included)
        n = np.rint(xs * F32(1.44269504088896341)).astype(F32)
        r = (xs - n * F32(0.693145751953125)).astype(F32)
        r = (r - n * F32(1.42860682030941723212e-6)).astype(F32)
        q = np.full_like(r, F32(1.9875691500e-4))
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            q = (q * r + F32(c)).astype(F32)
        y = (q * (r * r) + r).astype(F32)
        y = (y + F32(1.0)).astype(F32)
        out = (y * np.ldexp(F32(1.0), np.maximum(n, -126).astype(np.int32)).astype(F32)).astype(F32)
    return np.where(x < F32(-86.0), F32(0.0), out).astype(F32)


def inv_temperature(temperature):
    """1.0f / T as the host computes it once per record (fp32 division)."""
    return F32(F32(1.0) / F32(temperature))


def weights(row, temperature):
    """Step 1: w_v = det_expf((l_v - max l) * inv_T), subtraction and multiplication as two fp32 operations."""
    row = np.asarray(row, F32)
    d = (row - row.max()).astype(F32)
    with np.errstate(invalid="ignore"):
        d = (d * inv_temperature(temperature)).astype(F32)
    return det_expf(d)


def ranking(row):
    """Step 2: token indices by logit descending (-0 equal to +0), ties by index ascending."""
    row = np.asarray(row, F32) + F32(0.0)
    return np.lexsort((np.arange(row.size), -row.astype(np.float64)))     # last key first: -l ascending, then index ascending


def keep_mask(logits, record):
    """Steps 1-4 for ONE row: (V,) bool, True for the tokens the record keeps."""
    temperature, top_p, top_k = record
    row = np.asarray(logits, F32).reshape(-1)
    V = row.size
    order = ranking(row)
    q = np.floor(weights(row, temperature).astype(np.float64) * Q_SCALE).astype(np.int64)[order]      # integer masses in rank order
    n_k = int(top_k) if 1 <= int(top_k) < V else V                        # step 3
    keep_rank = np.arange(V) < n_k
    if F32(top_p) < F32(1.0):                                             # step 4
        Q = int(q[:n_k].sum())
        thr = int(np.ceil(np.float64(F32(top_p)) * np.float64(Q)))        # one fp64 product; M < p Q <=> M < ceil(p Q) for an integer M
        M = np.concatenate([[0], np.cumsum(q)[:-1]])                      # mass of the ranks before each rank
        keep_rank &= (np.arange(V) == 0) | (M < thr)
    kept = np.zeros(V, bool)
    kept[order[keep_rank]] = True
    return kept


def draw(row, u, temperature, kept):
    """Step 5 for one row: the samplers' inverse CDF in index order over w' = kept ? w : 0 (256 contiguous chunks summed left to right,
    chunk sums prefix-summed left to right, a left-to-right walk in the owning chunk), all in fp32."""
    row = np.asarray(row, F32).reshape(-1)
    V = row.size
    chunk = (V + NTHREADS - 1) // NTHREADS
    w = np.where(kept, weights(row, temperature), F32(0.0)).astype(F32)
    pad = np.zeros(NTHREADS * chunk, F32)
    pad[:V] = w
    pad = pad.reshape(NTHREADS, chunk)
    s = np.zeros(NTHREADS, F32)
    for j in range(chunk):                                               # every chunk left to right (adding a zero changes no bit)
        s = (s + pad[:, j]).astype(F32)
    pre = np.concatenate([[F32(0.0)], np.add.accumulate(s, dtype=F32)]).astype(F32)
    thr = F32(F32(u) * pre[NTHREADS])
    owner = NTHREADS - 1
    for t in range(NTHREADS):
        if pre[t] <= thr and (thr < pre[t + 1] or t == NTHREADS - 1):
            owner = t
            break
    v0, v1 = owner * chunk, min((owner + 1) * chunk, V)
    kept_idx = np.flatnonzero(kept)
    c = pre[owner]
    for v in range(v0, v1):
        if kept[v]:
            c = F32(c + w[v])
            if c > thr:
                return int(v)
    own = kept_idx[(kept_idx >= v0) & (kept_idx < v1)]
    if thr < pre[owner + 1] and own.size:
        return int(own[-1])                                              # no crossing inside the owning chunk: its highest kept token
    return int(kept_idx[-1])                                             # no running sum above u * total: the row's highest kept token


def sample_ctl(logits, u, records):
    """Steps 1-5 for (B,V) rows: u (B,) uniforms, records = one record or B -> (idx (B,) int64, kept (B,V) bool)."""
    logits = np.asarray(logits, F32)
    B, V = logits.shape
    if isinstance(records, tuple) and len(records) == 3 and not isinstance(records[0], (tuple, list)):
        records = [records] * B
    idx = np.zeros(B, np.int64)
    kept = np.zeros((B, V), bool)
    for b in range(B):
        kept[b] = keep_mask(logits[b], records[b])
        idx[b] = draw(logits[b], u[b], records[b][0], kept[b])
    return idx, kept


# ---- log-probabilities (include/talkshow_hip.h, "log-probabilities"; csrc/vq.hip: sample_lp_kernel, sample_ctl_kernel<., true>) --------------

DET_EXPF_REL_ERR = 2.0 ** -23   # bound used for det_expf against exp on [-86, 0]; the worst error found on 2^26 + 1 points is 8.11e-8


def chunk_total(w):
    """The fp32 total S of a row of weights with the samplers' summation structure: 256 contiguous chunks of ceil(V / 256) summed left to
    right, then the 256 chunk sums added left to right."""
    w = np.asarray(w, F32).reshape(-1)
    chunk = (w.size + NTHREADS - 1) // NTHREADS
    pad = np.zeros(NTHREADS * chunk, F32)
    pad[:w.size] = w
    pad = pad.reshape(NTHREADS, chunk)
    s = np.zeros(NTHREADS, F32)
    for j in range(chunk):
        s = (s + pad[:, j]).astype(F32)
    return F32(np.add.accumulate(s, dtype=F32)[-1])


def logprob(row, code, record=None):
    """The log-probability the device returns for `code` on the logits `row` (V,): float32((double) d_c - log((double) S)), d_c the fp32
    argument of the code's exponential, S the fp32 total the draw is made from.  record None: the sampler without controls (greedy and
    teacher forced too), d_c = l_c - max, S over all weights.  With a record (temperature, top_p, top_k): d_c = (l_c - max) * inv_T as two
    fp32 operations, S over the weights the record keeps.  S and d_c equal the device's bit for bit; the fp64 log may differ from the
    device's in its last place, so the result is the device's or an adjacent float32.  A code outside [0, V) gives NaN.  (The device
    only ever returns values for kept tokens: a draw is one.)"""
    row = np.asarray(row, F32).reshape(-1)
    V = row.size
    code = int(code)
    if not 0 <= code < V:
        return F32(np.nan)
    d = (row - row.max()).astype(F32)
    if record is None:
        w = det_expf(d)
    else:
        temperature = record[0]
        with np.errstate(invalid="ignore"):
            d = (d * inv_temperature(temperature)).astype(F32)
        w = np.where(keep_mask(row, record), det_expf(d), F32(0.0)).astype(F32)
    S = chunk_total(w)
    return F32(np.float64(d[code]) - np.log(np.float64(S)))


def given_logprob(row, code, record=None):
    """The log-probability a GIVEN code gets on the logits `row` (include/talkshow_hip.h, "given rows"): that of `code` under the
    distribution the row would have been drawn from.  Without a record: `logprob(row, code)`, the teacher-forced value.  With one: the
    same expression over the kept weights when the record keeps `code` — the bits a draw of it gets — and log(0) = -inf when the filters
    removed it (its weight in that distribution is 0); top_k = 1 therefore gives 0 for the argmax and -inf for every other code.  NaN for a
    code outside [0, V)."""
    row = np.asarray(row, F32).reshape(-1)
    code = int(code)
    if not 0 <= code < row.size:
        return F32(np.nan)
    if record is not None and not keep_mask(row, record)[code]:
        with np.errstate(divide="ignore"):
            return F32(np.log(np.float64(0.0)))
    return logprob(row, code, record)


# ---- alternatives (include/talkshow_hip.h, "alternatives"; csrc/vq.hip: sample_ctl_body<..., ALT = true>) -----------------------------------

ALT_MAX = 8

Alternatives = collections.namedtuple("Alternatives", "codes logprobs entropy rank")
Alternatives.__doc__ = """What `alternatives=n` appends to a decode's return value: codes int64 (..., n) the n best allowed codes of every
position (-1 beyond the allowed ones), logprobs float32 (..., n) their log-probabilities (-inf there), entropy float32 (...) of the
position's distribution, rank int64 (...) of the position's own code (-1 for a given code outside the vocabulary) — all under the
distribution the filters are applied to (temperature applied, top-k and top-p not)."""


def alt_count(n):
    """The `alternatives=` keyword as an integer in [0, 8]; ValueError otherwise (a bool is no count)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"alternatives must be None or an integer in [0, {ALT_MAX}], got {n!r}")
    if not 0 <= int(n) <= ALT_MAX:
        raise ValueError(f"alternatives must be in [0, {ALT_MAX}], got {int(n)}")
    return int(n)


def alternatives(row, record, n, bias=None, counts=None, rep=None, code=None):
    """The rule of "alternatives" for ONE position, the device's arithmetic operation for operation: row (V,) the network's logits, record
    (temperature, top_p, top_k) or None (neutral; top_p and top_k are not used: the outputs describe the distribution ahead of the
    filters), n in [0, 8], bias the clip's (V,) row of this column or None (step 0), counts (V,) and rep = (window, presence, frequency)
    the history counts and record of step 0b (`repeat_counts`; None or window 0: no penalty), code the position's own code or None ->
    Alternatives(codes (n,) int64, logprobs (n,) float32, entropy float32, rank int: -1 for a code outside [0, V) and for code None).
    S_all, E and every d_j equal the device's bit for bit; the two fp64 logs may differ from the device's in their last place, so a
    log-probability and the entropy are the device's value or an adjacent float32."""
    n = alt_count(n)
    temperature = 1.0 if record is None else record[0]
    l = biased(row, bias)
    if counts is not None and rep is not None and int(rep[0]) > 0:
        l = penalised(l, counts, rep)
    V = l.size
    m = l[int(np.argmax(l))]                                              # the first maximum, as the workgroup arg-max returns it
    with np.errstate(invalid="ignore", over="ignore"):
        d = (l - m).astype(F32)
        d = (d * inv_temperature(temperature)).astype(F32)
        allowed = l != F32(-np.inf)
        w = np.where(allowed, det_expf(d), F32(0.0)).astype(F32)
        t = np.where(w > 0, (w * np.where(w > 0, d, F32(0.0))).astype(F32), F32(0.0)).astype(F32)    # one fp32 product where w > 0
    S_all = chunk_total(w)
    E = chunk_total(t)
    log_s = np.log(np.float64(S_all))
    order = ranking(l)
    best = order[allowed[order]][:n]
    codes = np.full(n, -1, np.int64)
    lps = np.full(n, -np.inf, F32)
    codes[:best.size] = best
    lps[:best.size] = (d[best].astype(np.float64) - log_s).astype(F32)
    entropy = F32(log_s - np.float64(E) / np.float64(S_all))
    rank = -1
    if code is not None and 0 <= int(code) < V:
        rank = int(np.flatnonzero(order == int(code))[0])
    return Alternatives(codes, lps, entropy, rank)


def alternatives_error_bound(V, d, lp, entropy):
    """Bounds on |alternatives(...) - exact| -> (bound for a log-probability with fp32 argument d and value lp, bound for the entropy),
    exact = the float64 log-softmax / entropy of z_v = (l''_v - m) / T over the allowed tokens, DERIVED from the rule in the manner of
    `logprob_error_bound`:
      d_v            a subtraction, 1 / T and a product, each one fp32 rounding: d_v = z_v (1 + e), |e| <= 3 * 2^-24 (1 + small)
      w_v            det_expf's relative error + that of its argument, |d_v| <= 86 for a non-zero weight: eps_w = DET_EXPF_REL_ERR + 86 * 3u;
                     weights below e^-86 are dropped: at most V * e^-86 of S_all >= 1
      S_all          at most chunk - 1 + 255 fp32 additions of non-negative terms, each relative 2^-24 of a partial sum <= S_all
      log-prob       |d| * 3u + eps_S / (1 - eps_S) + the fp64 log and subtraction 2^-50 (1 + |lp|) + the rounding to fp32 |lp| * 2^-24
      t_v            w_v * d_v: eps_w + 3u + one rounding; all terms are <= 0, so E carries eps_E = eps_w + 4u + (chunk - 1 + 255) u relative
                     to |E|; a dropped term is at most 87 e^-86 in magnitude (|z| e^z falls beyond 86)
      entropy        H = log S + A with A = -E / S >= 0, so A <= H: |dH| <= eps_S / (1 - eps_S) + H (eps_E + eps_S) + V * 87 e^-86 +
                     the fp64 operations 4 * 2^-50 (1 + H) + the rounding to fp32 H * 2^-24."""
    u = 2.0 ** -24
    chunk = (int(V) + NTHREADS - 1) // NTHREADS
    nadd = chunk - 1 + 255
    eps_w = DET_EXPF_REL_ERR + 86 * 3 * u
    eps_s = (nadd * u + eps_w) * 1.001 + V * np.exp(-86.0)
    eps_e = (eps_w + 4 * u + nadd * u) * 1.001
    lp_bound = abs(float(d)) * 3 * u * 1.001 + eps_s / (1 - eps_s) + 2.0 ** -50 * (1 + abs(float(lp))) + abs(float(lp)) * u
    H = abs(float(entropy))
    h_bound = eps_s / (1 - eps_s) + H * (eps_e + eps_s) * 1.001 + V * 87 * np.exp(-86.0) + 4 * 2.0 ** -50 * (1 + H) + H * u
    return lp_bound, h_bound


def uncertain_keep(entropy, threshold):
    """A mask for `given_keep=`: entropy (G, 2) of a decode's positions (`Alternatives.entropy` of one clip; a tensor is read back) ->
    (G, 2) bool, True where entropy <= threshold.  Handing the decode back through `given=` with this mask keeps what the model was sure
    of and redraws the rest."""
    e = np.asarray(entropy.detach().cpu().numpy() if hasattr(entropy, "detach") else entropy, np.float64)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"uncertain_keep: entropy must be (G, 2), got {tuple(e.shape)}")
    thr = float(threshold)
    if np.isnan(thr):
        raise ValueError("uncertain_keep: the threshold is NaN")
    return e <= thr


def style_rows(weights, table):
    """The rule of "speaker style" (include/talkshow_hip.h), restated: weights (..., NC) float, table (NC, W) float32 — one layer's
    class_cond_embedding — -> (..., W) float32, the class-conditioning vector of every weight row: over c ascending, every weight that is
    not 0 contributes t = w[c] * table[c], product and sum each rounded to float32 (numpy.float32 arithmetic: no fused multiply-add); the
    first contribution starts the sum; a zero weight contributes nothing and its table row is not read (it may hold NaN); +0.0 where every
    weight is 0.  A one-hot row therefore returns its table row bit for bit (-0.0 included).  style_rows_kernel computes exactly this."""
    w = np.asarray(weights, np.float32)
    table = np.asarray(table, np.float32)
    if w.ndim < 1 or table.ndim != 2 or w.shape[-1] != table.shape[0]:
        raise ValueError(f"style_rows: weights (..., NC) and table (NC, W) disagree: {w.shape} and {table.shape}")
    flat = w.reshape(-1, w.shape[-1])
    out = np.zeros((flat.shape[0], table.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for m in range(flat.shape[0]):
            acc = None
            for c in range(flat.shape[1]):
                if flat[m, c] != 0:
                    t = (flat[m, c] * table[c]).astype(np.float32)      # float32 * float32, rounded once
                    acc = t if acc is None else (acc + t).astype(np.float32)
            if acc is not None:
                out[m] = acc
    return out.reshape(w.shape[:-1] + (table.shape[1],))


# ---- code bias (include/talkshow_hip.h, "code bias"; csrc/vq.hip: sample_ctl_body<., ., ., BIAS = true>) -------------------------------------

def biased(row, bias=None):
    """Step 0: l' = l + b, one fp32 addition per token; bias None: the row itself (nothing is added, so a -0 stays -0)."""
    row = np.asarray(row, F32).reshape(-1)
    if bias is None:
        return row
    return (row + np.asarray(bias, F32).reshape(-1)).astype(F32)


def keep_mask_bias(logits, record, bias=None):
    """Steps 0-4 for ONE row: `keep_mask` of l' under the record, and — the kept-set sentence — never a token with l' = -inf.  bias None:
    `keep_mask(logits, record)`, nothing else."""
    if bias is None:
        return keep_mask(logits, record)
    lb = biased(logits, bias)
    return keep_mask(lb, record) & (lb != F32(-np.inf))


def sample_bias(logits, u, records, bias, index, column):
    """One launch of the samplers under a code bias, restated: logits (B,V), u (B,), records = None (neutral), one record or B, bias
    (NB,2,V) tables, index (B,) the table of every row or -1, column 0 (body) / 1 (hand) -> (idx (B,) int64, kept (B,V) bool, logprob (B,)
    float32).  A row with index -1 is `sample_ctl`'s row."""
    logits = np.asarray(logits, F32)
    B, V = logits.shape
    if records is None:
        records = (1.0, 1.0, 0)
    if isinstance(records, tuple) and len(records) == 3 and not isinstance(records[0], (tuple, list)):
        records = [records] * B
    idx = np.zeros(B, np.int64)
    kept = np.zeros((B, V), bool)
    lp = np.zeros(B, F32)
    for b in range(B):
        t = int(index[b])
        row_bias = None if t < 0 else np.asarray(bias, F32)[t, int(column)]
        lb = biased(logits[b], row_bias)
        kept[b] = keep_mask_bias(logits[b], records[b], row_bias)
        idx[b] = draw(lb, u[b], records[b][0], kept[b])
        lp[b] = logprob(lb, idx[b], records[b])
    return idx, kept, lp


def given_logprob_bias(row, code, record=None, bias=None):
    """`given_logprob` under a code bias: the given code is taken whatever the table says; its log-probability is that of the code under
    the biased, filtered distribution — -inf for a code the bias bans or the filters remove.  record None: a neutral record."""
    if bias is None:
        return given_logprob(row, code, record)
    record = (1.0, 1.0, 0) if record is None else record
    lb = biased(row, bias)
    code = int(code)
    if not 0 <= code < lb.size:
        return F32(np.nan)
    if not keep_mask_bias(row, record, bias)[code]:
        with np.errstate(divide="ignore"):
            return F32(np.log(np.float64(0.0)))
    return logprob(lb, code, record)


def _code_columns(codes, V):
    if isinstance(codes, (tuple, list)) and len(codes) == 2 and not (np.ndim(codes[0]) == 0 and np.ndim(codes[1]) == 0):
        cols = [np.asarray(codes[0], np.int64).reshape(-1), np.asarray(codes[1], np.int64).reshape(-1)]
    else:
        c = np.asarray(codes.detach().cpu().numpy() if hasattr(codes, "detach") else codes)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in "iu":
            raise ValueError(f"codes must be an (n, 2) integer array or a pair of index lists (body, hand), got {c.dtype} {tuple(c.shape)}")
        cols = [c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)]
    for j, c in enumerate(cols):
        c = c[c >= 0]                                                     # -1 marks rows beyond a clip's own (decode outputs): not a code
        if c.size and c.max() >= V:
            raise ValueError(f"column {j} holds code {int(c.max())}, outside [0, {V})")
        cols[j] = c
    return cols


def allow_bias(codes, V):
    """ALLOW-LIST: codes (n, 2) integers (column 0 body, column 1 hand; -1 entries are skipped) or a pair (body indices, hand indices) ->
    (2, V) float32 table, 0 for the codes that occur in a column and -inf for every other.  ValueError for a column without a code."""
    V = int(V)
    t = np.full((2, V), -np.inf, F32)
    for j, c in enumerate(_code_columns(codes, V)):
        if c.size == 0:
            raise ValueError(f"allow_bias: column {j} allows no code")
        t[j, c] = F32(0.0)
    return t


def ban_bias(codes, V):
    """BAN-LIST, `allow_bias`'s complement: -inf for the codes that occur in a column, 0 for every other.  ValueError if a column bans
    every code."""
    V = int(V)
    t = np.zeros((2, V), F32)
    for j, c in enumerate(_code_columns(codes, V)):
        t[j, c] = F32(-np.inf)
        if not np.isfinite(t[j]).any():
            raise ValueError(f"ban_bias: column {j} bans every code")
    return t


# ---- repetition penalty (include/talkshow_hip.h, "repetition penalty"; csrc/vq.hip: sample_ctl_body<., ., ., true, REP = true>) ---------------
# A record is (window, presence, frequency), `_lib.repeat_record`'s form.

REPEAT_MAX_WINDOW = 64      # the ring: the code of row r of a column lives at index r & 63


def repeat_counts(history, V, window):
    """History: c_v for every token.  history = the codes of rows 0 .. r - 1 of ONE clip and ONE column, oldest first (or any tail of them
    that holds the last min(r, window) rows) -> (V,) int32, how often each code occurs in the last `window` entries.  Codes outside [0, V)
    (a given code may be one) match no token.  window 0: zeros."""
    h = np.asarray(history, np.int64).reshape(-1)
    W = int(window)
    if not 0 <= W <= REPEAT_MAX_WINDOW:
        raise ValueError(f"repeat_counts: window {W} is outside [0, {REPEAT_MAX_WINDOW}]")
    h = h[h.size - min(h.size, W):]
    h = h[(h >= 0) & (h < int(V))]
    return np.bincount(h, minlength=int(V)).astype(np.int32)


def penalised(row, counts, record):
    """Step 0b: for c_v > 0, f = frequency * float(c_v), g = presence + f, l''_v = l'_v - g — three float32 operations, each rounded
    (numpy.float32 arithmetic: no fused multiply-add); for c_v == 0 the token's bits (a -0 stays -0)."""
    row = np.asarray(row, F32).reshape(-1)
    c = np.asarray(counts).reshape(-1)
    _, presence, frequency = record
    with np.errstate(over="ignore", invalid="ignore"):
        f = (F32(frequency) * c.astype(F32)).astype(F32)
        g = (F32(presence) + f).astype(F32)
        out = (row - g).astype(F32)
    return np.where(c > 0, out, row).astype(F32)


def _per_row(x, B, width):
    if isinstance(x, tuple) and len(x) == width and not isinstance(x[0], (tuple, list)):
        return [x] * B
    return list(x)


def sample_repeat(logits, u, records, repeat, history, position, bias=None, index=None, column=0, given=None, forced=None):
    """One launch of the samplers under a repetition penalty, restated, ring update included (`ts_op_sample_repeat`): logits (B,V), u
    (B,), records = None (neutral), one sampling record or B, repeat = one (window, presence, frequency) record or B, history (B,R) the
    codes of rows r - R .. r - 1 of this column, oldest first, R = min(r, 64), r = position >> 1; bias (NB,2,V) / index (B,) / column as
    for `sample_bias` (bias None: no tables); given (B,) codes and forced (B,) bool: the rows that TAKE their given code ->
    (idx (B,) int64, kept (B,V) bool, logprob (B,) float32, ring (B,64) int32).  The ring starts as -1 everywhere, holds the history where
    a pass would have left it (row r' at r' & 63) and, for a row with window > 0, the row's code at r & 63 (a given code outside [0, V):
    -1); a row with window 0 touches no ring and is `sample_bias`'s row."""
    logits = np.asarray(logits, F32)
    B, V = logits.shape
    r = int(position) >> 1
    R = min(r, REPEAT_MAX_WINDOW)
    history = np.zeros((B, 0), np.int64) if R == 0 else np.asarray(history, np.int64).reshape(B, R)
    records = _per_row((1.0, 1.0, 0) if records is None else records, B, 3)
    repeat = _per_row(repeat, B, 3)
    idx = np.zeros(B, np.int64)
    kept = np.zeros((B, V), bool)
    lp = np.zeros(B, F32)
    ring = np.full((B, REPEAT_MAX_WINDOW), -1, np.int32)
    for i in range(R):
        ring[:, (r - R + i) & (REPEAT_MAX_WINDOW - 1)] = history[:, i]
    for b in range(B):
        t = -1 if bias is None else int(index[b])
        row_bias = None if t < 0 else np.asarray(bias, F32)[t, int(column)]
        lb = biased(logits[b], row_bias)
        W = int(repeat[b][0])
        lpen = penalised(lb, repeat_counts(history[b], V, W), repeat[b]) if W > 0 else lb
        kept[b] = keep_mask(lpen, records[b])
        if row_bias is not None:
            kept[b] &= lpen != F32(-np.inf)
        if forced is not None and forced[b]:
            code = int(given[b])
            idx[b] = code
            if not 0 <= code < V:
                lp[b] = F32(np.nan)
            elif not kept[b, code]:
                with np.errstate(divide="ignore"):
                    lp[b] = F32(np.log(np.float64(0.0)))
            else:
                lp[b] = logprob(lpen, code, records[b])
            tok = code if 0 <= code < V else -1
        else:
            idx[b] = tok = draw(lpen, u[b], records[b][0], kept[b])
            lp[b] = logprob(lpen, idx[b], records[b])
        if W > 0:
            ring[b, r & (REPEAT_MAX_WINDOW - 1)] = tok
    return idx, kept, lp, ring


def decode_repeat(logits, u, record, repeat, bias=None, given=None, forced=None):
    """The row loop of ONE clip over logits a decode returned: logits (H,2,V) (the network's l of every position: the penalty does not
    change them as long as the codes agree), u (H,2) uniforms, record = a sampling record or None, repeat = the clip's (window, presence,
    frequency), bias = the clip's (2,V) table or None, given (H,2) codes and forced (H,2) bool or None -> (codes (H,2) int64, logprob
    (H,2) float32): position (r, j) is `sample_repeat` on the codes this loop produced in column j so far."""
    logits = np.asarray(logits, F32)
    H = logits.shape[0]
    codes = np.zeros((H, 2), np.int64)
    lps = np.zeros((H, 2), F32)
    tables = None if bias is None else np.asarray(bias, F32)[None]
    for r in range(H):
        R = min(r, REPEAT_MAX_WINDOW)
        for j in range(2):
            hist = np.where((codes[r - R:r, j] >= 0) & (codes[r - R:r, j] < logits.shape[2]), codes[r - R:r, j], -1)[None]
            f = None if forced is None else [bool(forced[r, j])]
            g = None if given is None else [int(given[r, j])]
            i, _, l, _ = sample_repeat(logits[r, j][None], [u[r, j]], record, repeat, hist, 2 * r + j, tables, [0], j, g, f)
            codes[r, j], lps[r, j] = i[0], l[0]
    return codes, lps


# ---- guidance (include/talkshow_hip.h, "guidance"; csrc/vq.hip: sample_ctl_body<., ., ., true, true, GUIDE = true>) ---------------------------

GUIDE_MAX_SCALE = 1e4


def guided(row_p, row_q, scale):
    """The rule: d = l_p - l_q, t = scale * d, l' = l_p + t — three float32 operations, each rounded (numpy.float32 arithmetic: no fused
    multiply-add).  scale = 0 and row_q equal to row_p return row_p's values (a -0 may become +0)."""
    p = np.asarray(row_p, F32).reshape(-1)
    q = np.asarray(row_q, F32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (p - q).astype(F32)
        t = (F32(scale) * d).astype(F32)
        return (p + t).astype(F32)


def guide_roles(guide, B, scale=None, lens=None):
    """`ts_guide_check` and the role table `SamplerTables::build` derives, restated: guide (B,) the shadow's slot of every slot or -1,
    scale (B,) (None: not checked), lens (B,) the slots' lengths in frames (None: not checked) -> (B,) int32 roles: -1 plain, g >= 0 a primary
    whose shadow is slot g, -2 a shadow.  ValueError with the library's text (without its "ts_guide_check: " prefix) for an index outside
    [-1, B), a slot that names itself, a shadow named twice, a shadow that is itself guided, unequal lengths, a NaN, an infinity or
    |scale| > 1e4 — found in the library's order."""
    B = int(B)
    guide = [int(g) for g in np.asarray(guide).reshape(-1)]
    if len(guide) != B or B < 1:
        raise ValueError("bad argument")
    named = [-1] * B
    for b, g in enumerate(guide):
        if g < -1 or g >= B:
            raise ValueError(f"clip {b}: the shadow index is {g}, not -1 (none) or in [0, {B})")
        if g < 0:
            continue
        if g == b:
            raise ValueError(f"clip {b} names itself as its shadow")
        if named[g] >= 0:
            raise ValueError(f"clip {b}: its shadow, slot {g}, is already the shadow of clip {named[g]}")
        named[g] = b
    roles = np.full(B, -1, np.int32)
    for b, g in enumerate(guide):
        if g < 0:
            continue
        if guide[g] >= 0:
            raise ValueError(f"clip {b}: its shadow, slot {g}, is itself guided (a shadow draws nothing)")
        if named[b] >= 0:
            raise ValueError(f"clip {b} is guided and is the shadow of clip {named[b]} (a shadow draws nothing)")
        if lens is not None and int(lens[g]) != int(lens[b]):
            raise ValueError(f"clip {b}: its length of {int(lens[b])} frames differs from the {int(lens[g])} frames of its shadow, slot {g}")
        if scale is not None:
            with np.errstate(over="ignore"):
                sc = F32(scale[b])
            if np.isnan(sc):
                raise ValueError(f"clip {b}: the scale is NaN")
            if np.isinf(sc):
                raise ValueError(f"clip {b}: the scale is infinite")
            if abs(sc) > F32(GUIDE_MAX_SCALE):
                raise ValueError(f"clip {b}: the scale exceeds 1e4 in magnitude")
        roles[b] = g
        roles[g] = -2
    return roles


def sample_guide(logits, u, records, guide, scale, repeat=None, history=None, position=0, bias=None, index=None, column=0, given=None,
                 forced=None):
    """One launch of the samplers under guidance, restated (`ts_op_sample_guide`): guide (B,) the shadow's row of every row or -1, scale
    (B,); everything else as `sample_repeat` takes it (repeat None: no records, history unused) -> (idx (B,) int64, kept (B,V) bool, logprob
    (B,) float32, ring (B,64) int32).  A primary runs `sample_repeat`'s row on l' = guided(l, l of its shadow, scale) under its own
    record, table, history and forced flag; its shadow's idx, kept and logprob are copies of the primary's and its ring holds its history
    and nothing else; a plain row is `sample_repeat`'s row."""
    logits = np.asarray(logits, F32)
    B, V = logits.shape
    roles = guide_roles(guide, B, scale)
    eff = logits.copy()
    rep = _per_row((0, 0.0, 0.0) if repeat is None else repeat, B, 3)
    rep = [tuple(r) for r in rep]
    f = None if forced is None else [bool(x) for x in forced]
    for b in range(B):
        if roles[b] >= 0:
            eff[b] = guided(logits[b], logits[roles[b]], scale[b])
        elif roles[b] == -2:      # draws nothing, takes nothing, writes no ring
            rep[b] = (0, 0.0, 0.0)
            if f is not None:
                f[b] = False
    r = int(position) >> 1
    if history is None:
        history = np.full((B, min(r, REPEAT_MAX_WINDOW)), -1, np.int64)
    idx, kept, lp, ring = sample_repeat(eff, u, records, rep, history, position, bias, index, column, given, f)
    for b in range(B):
        if roles[b] >= 0:
            g = int(roles[b])
            idx[g], kept[g], lp[g] = idx[b], kept[b], lp[b]
    return idx, kept, lp, ring


def keep_forced(G, keep, r, j):
    """The rule of "kept positions" (include/talkshow_hip.h) for one sampler launch: G (B,) given rows per clip slot, keep (B,H,2) mask of
    kept positions or None, (r, j) the launch's row and column -> (B,) bool: clip b is FORCED at (r, j) iff 2 r + j < 2 G_b and (keep is None
    or keep[b, r, j] != 0).  The mask is read below G_b only.  `sample_given` takes the result as its per-row `forced`."""
    G = np.asarray(G, np.int64).reshape(-1)
    pos = 2 * int(r) + int(j)
    out = np.zeros(G.size, bool)
    for b in range(G.size):
        if pos < 2 * int(G[b]):
            out[b] = True if keep is None else bool(keep[b][int(r)][int(j)] != 0)
    return out


def sample_given(logits, u, forced, given, records=None, greedy=False):
    """One launch of the samplers' given variants, restated: logits (B,V), u (B,) uniforms (those of forced rows are not read), forced (B,)
    flags, given (B,) codes (those of unforced rows are not read), records = None, one record or B -> (idx (B,) int64, logprob (B,)
    float32).  A forced row returns its given code and `given_logprob` of it; an unforced row what the sampler it stands in for returns:
    `sample_ctl` with records, the plain inverse CDF (a neutral record's draw) or, greedy, the first maximum."""
    logits = np.asarray(logits, F32)
    B, V = logits.shape
    if records is not None and isinstance(records, tuple) and len(records) == 3 and not isinstance(records[0], (tuple, list)):
        records = [records] * B
    idx = np.zeros(B, np.int64)
    lp = np.zeros(B, F32)
    for b in range(B):
        rec = None if records is None else records[b]
        if forced[b]:
            idx[b] = int(given[b])
            lp[b] = given_logprob(logits[b], idx[b], rec)
            continue
        if greedy:
            idx[b] = int(np.argmax(logits[b]))
        else:
            r = (1.0, 1.0, 0) if rec is None else rec
            idx[b] = draw(logits[b], u[b], r[0], keep_mask(logits[b], r))
        lp[b] = logprob(logits[b], idx[b], rec)
    return idx, lp


def given_pose_rows(P, T):
    """`ts_given_pose_rows_check` for one clip: P given pose frames (None: none) of a clip with T MFCC rows -> the given code rows G = P // 4.
    0 for None or P = 0.  ValueError for 1 <= P <= 3 (frames that cannot make one code row: the caller has miscounted), for P < 0, and for
    P // 4 > T // 4 (more rows than the clip has of its own).  A remainder P % 4 is dropped, as the VQ encoder drops it."""
    if P is None:
        return 0
    P, T = int(P), int(T)
    if P == 0:
        return 0
    if P < 4:
        raise ValueError(f"given poses: P = {P} frames; one code row needs 4 (or none: P = 0)")
    if P // 4 > T // 4:
        raise ValueError(f"given poses: P = {P} frames are {P // 4} code rows but the clip has {T // 4} of its own")
    return P // 4


LOGPROB_SUM_LANES = 256


def logprob_sums(lp, rows=None):
    """`ts_logprob_sums` addition for addition: lp (B,H,2) float32, rows (B,) = every clip's own row count H_b (None: H) -> (B,3) float64
    {body column, hand column, body + hand}.  Lane t adds rows t, t + 256, ... of a column in ascending order in fp64; the 256 lane sums
    are then added in ascending order; the third value is one fp64 addition of the first two.  Rows at or beyond H_b do not enter."""
    lp = np.asarray(lp, F32)
    B, H, W = lp.shape
    if W != 2:
        raise ValueError(f"logprob_sums: lp must be (B, H, 2), got {lp.shape}")
    out = np.zeros((B, 3), np.float64)
    for b in range(B):
        Hb = H if rows is None else min(H, max(int(rows[b]), 0))
        x = lp[b, :Hb].astype(np.float64)
        for k in range(2):
            lanes = np.zeros(LOGPROB_SUM_LANES, np.float64)
            for r0 in range(0, Hb, LOGPROB_SUM_LANES):                   # round j of every lane: row r0 + t
                seg = x[r0:r0 + LOGPROB_SUM_LANES, k]
                lanes[:seg.size] = lanes[:seg.size] + seg
            s = np.float64(0.0)
            for t in range(LOGPROB_SUM_LANES):
                s = s + lanes[t]
            out[b, k] = s
        out[b, 2] = out[b, 0] + out[b, 1]
    return out


def logprob_error_bound(V, d_c, lp):
    """Bound on |logprob(row, c) - exact| WITHOUT a record, exact = the float64 log-softmax of the fp32 logits at c, DERIVED from the rule:
      d_c            one fp32 subtraction: |d_c| * 2^-24
      every weight   det_expf's relative error (DET_EXPF_REL_ERR) + the rounding of its argument, |d_v| <= 86 for a non-zero weight:
                     exp(d (1 + e)), |e| <= 2^-24 -> relative 86 * 2^-24 (1 + small); weights below e^-86 are dropped: V * e^-86 of S >= 1
      S              at most chunk - 1 + 255 fp32 additions, each relative 2^-24 of a partial sum <= S (all terms are >= 0)
      log            |d log S| <= eps / (1 - eps);  the fp64 log and subtraction: 2^-50 (1 + |lp|)
      result         one rounding to fp32: |lp| * 2^-24."""
    u = 2.0 ** -24
    chunk = (int(V) + NTHREADS - 1) // NTHREADS
    eps = ((chunk - 1 + 255) * u + DET_EXPF_REL_ERR + 86 * u) * 1.001 + V * np.exp(-86.0)
    return abs(float(d_c)) * u + eps / (1 - eps) + 2.0 ** -50 * (1 + abs(float(lp))) + abs(float(lp)) * u
