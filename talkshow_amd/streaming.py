"""Seamless body streaming: where the windows of a chunked session are cut so that any chunking returns the one-shot call's bits.

`SeamlessPlan` is host arithmetic only (no GPU, no torch): the four counters of a session and, per call, the encoder window, the code
rows the chain runs, the decoder window and what is kept of each.  The native session (`csrc/body_stream.cpp`, `ts_body_stream_*`)
restates the same arithmetic in C++; `tests/test_seamless_plan.py` holds the two against each other through a host-only debug entry.
`SeamlessBodyStream` is the host handle of the native session (`TrainWrapper.open_stream(..., seamless=True)`).

Why these windows ("seamless sessions"): output row i of the audio encoder reads MFCC frames 4i-25 .. 4i+28, 7 code rows to
either side; pose frame t of a VQ decoder reads code rows t//4-6 .. t//4+6.  A row whose cone lies inside a window (or beyond the clip's own
edge, where window and clip pad alike) comes out of the window as out of the whole clip.  Windows start at a multiple of 4 code rows so
that the 4-row Winograd tiles of the lowered conv stacks, counted from a window's row 0, sit where the one-shot call has them.  Equal
values are not yet equal bits there: an output row of an F(4,3) tile is summed from products that hold the tile's other input rows (y0 from
d0..d4, y1 and y2 from d1..d4, y3 from d1..d5: csrc/conv_wino.hip), so a lowered layer's ROUNDING reaches to the edge of its tile.  Through
the three lowered layers of each decoder stack that widens a pose frame's reach from 6 to at most 13 code rows: DEC_TILE_SLACK_ROWS."""
from collections import namedtuple

ENC_MARGIN_ROWS = 7      # code rows of audio an encoder output row needs on either side
ENC_TILE_SLACK_ROWS = 7  # ... and how much further the rounding reaches where the audio encoder is Winograd-lowered (not by default)
DEC_MARGIN_ROWS = 6      # code rows a pose frame needs on either side
DEC_TILE_SLACK_ROWS = 7  # ... and how much further the rounding of the Winograd-lowered decoder stacks reaches (tile edges)
ALIGN_ROWS = 4           # every window starts at a multiple of this many code rows
TAIL_CAP_FRAMES = 72     # MFCC frames a session holds back between calls, at most 71 (see SeamlessPlan.retained; 8 m + 15 at m rows of reach)
RING_KEEP_ROWS = 32      # code rows a session holds back between calls, at most 29

# One call's work, in absolute frames / code rows of the clip.  enc = (f0, f1): the encoder window, frames [f0, f1), or None (no call);
# rows = (A0, A1): the audio / code rows the call finalises (rows [A0 - f0 // 4, A1 - f0 // 4) of the window's output, one chain step);
# dec = (v0, v1): the decoder window, code rows [v0, v1), or None; poses = (D0, D1): the code rows whose 4 pose frames each come out
# (frames [4 (D0 - v0), 4 (D1 - v0)) of the window's output); keep_frame0 / keep_row0: the first MFCC frame / code row a later call reads.
Call = namedtuple("Call", "enc rows dec poses keep_frame0 keep_row0")


def _align_down(x):
    return x // ALIGN_ROWS * ALIGN_ROWS


class SeamlessPlan:
    """F MFCC frames received, A audio / code rows done, D code rows whose poses are out, flushed.  `push(t)` / `flush()` move the counters
    and return the `Call`.  enc_margin / enc_slack / dec_margin / dec_slack: the named constants; a test lowers one to show that a shorter
    margin is caught (dec_slack=0: the plan for decoders without lowered stacks; enc_slack=ENC_TILE_SLACK_ROWS: the plan the native session
    takes where the audio encoder is lowered too, TS_CONV_WINO=1 or an encoder of 512 channels or more)."""

    def __init__(self, enc_margin=ENC_MARGIN_ROWS, dec_margin=DEC_MARGIN_ROWS, dec_slack=DEC_TILE_SLACK_ROWS, enc_slack=0):
        self.F = self.A = self.D = 0
        self.flushed = False
        self.enc_margin, self.dec_margin = int(enc_margin) + int(enc_slack), int(dec_margin) + int(dec_slack)

    def peek(self, t, flush=False):
        """The `Call` a push of t frames (or the flush, t = 0) would make; the counters stay."""
        if self.flushed:
            raise ValueError("the session has been flushed (the clip has ended): open another")
        t = int(t)
        if flush and t != 0:
            raise ValueError(f"a flush brings no frames, got t = {t}")
        if not flush and t < 1:
            raise ValueError(f"a push holds at least one MFCC frame, got t = {t}")
        F, A, D, me, md = self.F + t, self.A, self.D, self.enc_margin, self.dec_margin
        A1 = F // 4 if flush else max(A, F // 4 - me)
        enc = None
        if A1 > A:
            w0 = _align_down(max(0, A - me))
            enc = (4 * w0, F if flush else min(F, 4 * (A1 + me)))
        D1 = A1 if flush else max(D, A1 - md)
        dec = None
        if D1 > D:
            dec = (_align_down(max(0, D - md)), min(A1, D1 + md))
        return Call(enc, (A, A1), dec, (D, D1), 4 * _align_down(max(0, A1 - me)), _align_down(max(0, D1 - md)))

    def _commit(self, call, t, flush):
        self.F, self.A, self.D, self.flushed = self.F + t, call.rows[1], call.poses[1], flush
        return call

    def push(self, t):
        return self._commit(self.peek(t), int(t), False)

    def flush(self):
        return self._commit(self.peek(0, flush=True), 0, True)

    def retained(self, call):
        """(MFCC frames, code rows) the session holds after `call` (made last).  Frames: F - 4 w0_next with w0_next >= A - 7 - 3 and
        A >= F // 4 - 7, so at most 71; rows: A - v0_next with v0_next >= D - 13 - 3 and D >= A - 13, so at most 29 — for any history."""
        return self.F - call.keep_frame0, self.A - call.keep_row0

    @property
    def state(self):
        return self.F, self.A, self.D, int(self.flushed)


def chain_rows(max_chunk_frames, enc_reach=ENC_MARGIN_ROWS):
    """The most code rows one call of a session opened for pushes of up to max_chunk_frames can run: a push of t frames finalises at most
    t // 4 + 1 rows, the flush the enc_reach rows held back.  The native session opens its chain for this count, so no call is split."""
    return max(int(enc_reach), int(max_chunk_frames) // 4 + 1)


class SlotClock:
    """Slot restart (talkshow_hip.h, "slot restart"), restated on the host: the session row, per slot the row at which its
    current clip began (its origin) and the Philox clip index it was given, and from those the rows of each slot's clip and the Philox
    position of (slot, session row, column).  `rewrites(r)` names what a restart at row r writes on the device.  Pure Python: the wrapper
    validates a restart through `check`, the tests hold the native session against the rest."""

    RING_ROWS = 4     # rows of a session's token ring; also the period of the Q1 / Q0 rings

    def __init__(self, B):
        self.B = int(B)
        if self.B < 1:
            raise ValueError(f"a session has at least one slot, got B = {B}")
        self.row = 0
        self.origins = [[0] for _ in range(self.B)]      # per slot: the origin of every clip it has held, ascending
        self.clip_index = [None] * self.B                # per slot: the index given at its last restart; None: clip_index0 + slot of a step

    @staticmethod
    def check(B, n_classes, slots, labels=None, styles=None, clip_indices=None):
        """The argument rules of a restart -> (slots, labels or None, styles or None, clip indices) as lists of n entries.  ValueError naming
        the slot: a slot outside [0, B) or listed twice, a label outside [0, n_classes), both a label and a style row or neither, a style
        row of the wrong shape or with a non-finite weight, a negative clip index.  clip_indices None: every slot's own number."""
        B, NC = int(B), int(n_classes)
        slots = [slots] if isinstance(slots, int) else list(slots)
        n = len(slots)
        if n < 1:
            raise ValueError("restart: no slot given")

        def seq(v):
            try:
                return not isinstance(v, str) and len(v) >= 0
            except TypeError:
                return False

        def spread(x, what):   # one value for all listed slots, or one per slot (a style VALUE is itself a row of numbers)
            if x is None:
                return None
            if hasattr(x, "detach"):
                x = x.detach().cpu().numpy()
            one = seq(x) and len(x) > 0 and all(e is not None and not seq(e) for e in x) if what == "style" else not seq(x)
            x = [x] * n if one else list(x)
            if len(x) != n:
                raise ValueError(f"restart: {n} slots but {len(x)} {what} entries")
            return x
        labels, styles, clip_indices = spread(labels, "label"), spread(styles, "style"), spread(clip_indices, "clip index")
        seen = set()
        for i, b in enumerate(slots):
            if int(b) != b or not 0 <= int(b) < B:
                raise ValueError(f"restart: slot {b} is outside [0, B = {B})")
            b = slots[i] = int(b)
            if b in seen:
                raise ValueError(f"restart: slot {b} is listed twice")
            seen.add(b)
            has_label = labels is not None and labels[i] is not None
            has_style = styles is not None and styles[i] is not None
            if has_label == has_style:
                raise ValueError(f"restart: slot {b} brings {'both a label and a style row' if has_label else 'neither a label nor a style row'}: "
                                 f"a new clip takes exactly one")
            if has_label and (int(labels[i]) != labels[i] or not 0 <= int(labels[i]) < NC):
                raise ValueError(f"restart: slot {b}: label {labels[i]} is outside [0, n_classes = {NC})")
            if has_style:
                row = styles[i].detach().cpu().numpy() if hasattr(styles[i], "detach") else styles[i]
                row = list(row.tolist() if hasattr(row, "tolist") else row) if seq(row) else None
                row = None if row is None or any(seq(v) for v in row) else [float(v) for v in row]
                if row is None or len(row) != NC:
                    raise ValueError(f"restart: slot {b}: a style row holds n_classes = {NC} weights (a session takes no tracks)")
                if any(v != v or v in (float("inf"), float("-inf")) for v in row):
                    raise ValueError(f"restart: slot {b}: a style weight is not finite")
            if clip_indices is not None and (int(clip_indices[i]) != clip_indices[i] or int(clip_indices[i]) < 0):
                raise ValueError(f"restart: slot {b}: clip index {clip_indices[i]} is negative")
        return slots, labels, styles, [int(c) for c in clip_indices] if clip_indices is not None else list(slots)

    def restart(self, slots, clip_indices=None):
        """The listed slots begin new clips at the session's next row."""
        slots, _, _, clips = self.check(self.B, 1, slots, labels=0, clip_indices=clip_indices)
        for b, c in zip(slots, clips):
            if self.origins[b][-1] != self.row:
                self.origins[b].append(self.row)
            self.clip_index[b] = c
        return self

    def advance(self, rows):
        self.row += int(rows)
        return self

    def origin(self, slot, row=None):
        """The origin of the clip that slot `slot` held at session row `row` (None: holds now)."""
        if row is None:
            return self.origins[slot][-1]
        return max(o for o in self.origins[slot] if o <= row)

    @property
    def slot_rows(self):
        """Rows of every slot's current clip."""
        return [self.row - o[-1] for o in self.origins]

    def position(self, slot, row, col):
        """The Philox counter word of slot `slot`'s code at session row `row`, column `col`: its position inside the slot's clip."""
        return 2 * (row - self.origin(slot, row)) + col

    def clip(self, slot, clip_index0=0):
        """The Philox clip index slot `slot` draws under in a step that passes clip_index0."""
        return clip_index0 + slot if self.clip_index[slot] is None else self.clip_index[slot]

    @classmethod
    def rewrites(cls, r):
        """What a restart at session row r writes in a slot's slabs: the token ring rows (ring index of rows r-1, r-2, r-3 that exist), the
        Q1 ring row of row r, the Q0 ring rows of rows r and r + 1, the parity of P read by row r."""
        R = cls.RING_ROWS
        return {"tok": [(r - k) % R for k in (1, 2, 3) if r - k >= 0], "q1": [r % R], "q0": [r % R, (r + 1) % R], "p": r & 1}


    # ---- slot state (talkshow_hip.h, "slot state"): save a slot's state, load it into any slot ----------------------------------
    # The rule.  `save` of slot b at session row r (the session's next row) gives a state S of the slot's clip of n = r - origin[b] rows.
    # Loading S into slot b' of a session of a network with the same dimensions and weights at its next row r', under clip index k'
    # (default: the one the source drew under): the slot produces from r' on what slot b would have produced from r on under the same
    # later inputs, and its rows equal rows n, n+1, ... of the one-shot `run` over the clip's whole audio with `given=` the clip's first n
    # code rows and clip_index0 = k'; every other slot has its bits; the save changes nothing in its session.  The state carries the
    # conditioning rows, the label the slot stands for, both repetition histories with their length, the clip index and n; it does not
    # carry what belongs to a step or to the target session (sampling records, bias tables, defaults, given rows).  One state may be
    # loaded into several slots, each under its own index.  A save at r < 3 is canonical (`canonical`); a load at r' < min(n, 3) is refused.
    STATE_VERSION = 1
    TOK_WORDS = 8     # three ring rows of two codes, padded to a multiple of 4 words
    REP_RING = 64     # entries of one repetition history

    @classmethod
    def state_layout(cls, D, NL):
        """Word offsets of one slot's state row (32-bit words; a function of (D, NL) alone): q1, q0a, q0b (4D floats each: Q1[r & 3],
        Q0[r & 3], Q0[(r + 1) & 3]), p (NL - 1 rows of 4D: P(l, r & 1), l >= 1), cr (NL rows of 2D), tok (int32: word 2 k + c = the code of
        row r-1-k, column c, k < 3; two words of 0), rep (int32: word 64 c + k = column c's code of row r-1-k, -1 beyond the history), and
        `words`, the row's length.  Every float block starts at a multiple of 4 words."""
        D, NL = int(D), int(NL)
        if D < 4 or D % 4 or NL < 1:
            raise ValueError(f"state_layout: D is a positive multiple of 4 and NL at least 1, got D = {D}, NL = {NL}")
        L = {"q1": 0, "q0a": 4 * D, "q0b": 8 * D, "p": 12 * D}
        L["cr"] = L["p"] + (NL - 1) * 4 * D
        L["tok"] = L["cr"] + NL * 2 * D
        L["rep"] = L["tok"] + cls.TOK_WORDS
        L["words"] = L["rep"] + 2 * cls.REP_RING
        return L

    @classmethod
    def state_words(cls, D, NL):
        return cls.state_layout(D, NL)["words"]

    @staticmethod
    def canonical(r):
        """What a save at session row r writes as the value a RESTART writes there, because the session's launches of rows r and r + 1
        would not have read the entry (it may never have been written): `tok`: the ages k (row r-1-k) saved as -1; `q1`, `q0a`, `q0b`:
        saved as +0.0; `p`: saved as bv[l].  Nothing for r >= 3."""
        r = int(r)
        return {"tok": [k for k in range(3) if r - 1 - k < 0], "q1": r < 2, "q0a": r < 3, "q0b": r < 2, "p": r == 0}

    @classmethod
    def load_plan(cls, r_new, n, hist=-1):
        """Where a load at session row r_new puts the state of a clip of n rows whose histories hold `hist` entries (-1: no penalty was
        running): the slot's new origin (negative for r_new < n), its rep_from (None: no penalty running), the ring index of every
        saved token row (None: the row lies below the session's row 0 and is not written), the Q ring rows and the parity of P (the
        entries `rewrites(r_new)` names), and the history ring index of every age."""
        r, n, hist = int(r_new), int(n), int(hist)
        R = cls.RING_ROWS
        return {"origin": r - n, "rep_from": None if hist < 0 else r - hist,
                "tok": [(r - 1 - k) % R if r - 1 - k >= 0 else None for k in range(3)],
                "q1": r % R, "q0": [r % R, (r + 1) % R], "p": r & 1,
                "ring": [(r - 1 - k) % cls.REP_RING for k in range(cls.REP_RING)]}

    @staticmethod
    def check_slots(B, slots, who, distinct=False):
        slots = [slots] if isinstance(slots, int) else list(slots)
        if len(slots) < 1:
            raise ValueError(f"{who}: no slot given")
        seen = set()
        for i, b in enumerate(slots):
            if int(b) != b or not 0 <= int(b) < int(B):
                raise ValueError(f"{who}: slot {b} is outside [0, B = {int(B)})")
            slots[i] = int(b)
            if distinct and slots[i] in seen:
                raise ValueError(f"{who}: slot {b} is listed twice")
            seen.add(slots[i])
        return slots

    @classmethod
    def check_load(cls, B, dims, row, slots, infos, clip_indices=None, who="load"):
        """The argument rules of a load at session row `row` -> (slots, state index per slot, clip index per slot).  dims: the target
        network's (D, NL, NC, V); infos: the records of the given states (dicts with D, NL, NC, V, version, rows, clip_index, hist, label),
        one for all listed slots or one each; row None: every rule but the row's.  ValueError naming the slot: a slot outside [0, B) or listed twice, a count mismatch, a state
        of other dimensions or version, row < min(rows, 3), a negative clip index (or none given and none recorded)."""
        slots = cls.check_slots(B, slots, who, distinct=True)
        n, infos = len(slots), list(infos)
        if len(infos) not in (1, n):
            raise ValueError(f"{who}: {n} slots but {len(infos)} states (one for all listed slots, or one each)")
        index = [0] * n if len(infos) == 1 else list(range(n))
        if clip_indices is not None:
            clip_indices = [clip_indices] * n if isinstance(clip_indices, int) else list(clip_indices)
            if len(clip_indices) != n:
                raise ValueError(f"{who}: {n} slots but {len(clip_indices)} clip index entries")
        clips = []
        for i, b in enumerate(slots):
            o = infos[index[i]]
            if int(o["version"]) != cls.STATE_VERSION:
                raise ValueError(f"{who}: slot {b}: the state has layout version {o['version']}, this package reads {cls.STATE_VERSION}")
            got = tuple(int(o[k]) for k in ("D", "NL", "NC", "V"))
            if got != tuple(int(v) for v in dims):
                raise ValueError(f"{who}: slot {b}: the state is of a network with (D, NL, NC, V) = {got}, this session's has {tuple(dims)}")
            rows = int(o["rows"])
            if row is not None and int(row) < min(rows, 3):
                raise ValueError(f"{who}: slot {b}: a clip of {rows} rows cannot be loaded at session row {int(row)} (the session's rows 0 to 2 "
                                 f"leave out terms the clip's state holds: load at row min(rows, 3) or later)")
            c = o["clip_index"] if clip_indices is None else clip_indices[i]
            if c is None or int(c) != c or int(c) < 0:
                raise ValueError(f"{who}: slot {b}: clip index {c} is negative" + ("" if clip_indices is not None else " (the state records none: give one)"))
            clips.append(int(c))
        return slots, index, clips

    def load(self, slots, rows, clip_indices):
        """The listed slots continue clips of rows[i] rows under clip_indices[i] from the session's next row.  The clock forgets the clips a
        loaded slot held before: `origin(slot, row)` and `position` answer for rows from here on."""
        for b, n, c in zip(slots, rows, clip_indices):
            self.origins[b] = [self.row - int(n)]
            self.clip_index[b] = int(c)
        return self


def _f32(x):
    """x as the fp32 value the library receives (a finite double beyond fp32's range arrives as an infinity)."""
    import struct
    try:
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


class SlotPairs:
    """Session pairs (talkshow_hip.h, "session pairs"), restated on the host beside `SlotClock`: which slots of a session are
    primary and shadow of a guided clip, each pair's stored scale, and WHEN a pair may form.  The shadow's row cache must hold its primary's
    code history under the second conditioning from the clip's row 0, so a pair is declared at session row 0, or behind the call that
    restarts both slots, or behind the call that loads both from states of equal clip rows — and ahead of the next step.  Restarting or
    loading one slot of a pair without the other is refused; listing both dissolves the pair unless the call declares it again.  There is
    no pairing and no un-pairing in the middle of a clip: scale 0 is the off switch.  `check` is `ts_pixelcnn_stream_pair_check` with the
    C check's wording (tests/test_stream_pairs_host.py holds the two against each other); the instance is the table a session keeps.
    Pure Python."""

    WHO = "session pairs: "
    MAX_SCALE = 1e4
    DEFAULT_SCALE = 1.0     # `pairs={primary: shadow}` without a scale

    def __init__(self, S):
        self.S = int(S)
        if self.S < 1:
            raise ValueError(f"a session has at least one slot, got S = {S}")
        self.guide = [-1] * self.S        # the table ts_guide_check takes: a primary's shadow, else -1
        self.scale = [0.0] * self.S       # a primary's stored scale
        self.fresh = [0] * self.S         # the serial of the restart or load that listed the slot at session row fresh_at, else 0
        self.fresh_at = -1
        self.serial = 0

    @classmethod
    def scale_fault(cls, s):
        """The tail of the refusal of one scale, or None."""
        try:
            s = _f32(s)
        except (TypeError, ValueError):
            return "the scale is NaN"
        if s != s:
            return "the scale is NaN"
        if s in (float("inf"), float("-inf")):
            return "the scale is infinite"
        if abs(s) > cls.MAX_SCALE:
            return "the scale exceeds 1e4 in magnitude"
        return None

    @classmethod
    def check(cls, S, rows, guide, clip_rows, fresh, primary, shadow=None, scale=None):
        """`ts_pixelcnn_stream_pair_check`: S slots at session row `rows`; guide (S,) the pair table; clip_rows (S,) the rows of every slot's
        current clip; fresh (S,) per slot the serial of the restart or load that listed it if no step was run since, else 0.  shadow given:
        the declaration of the pairs (primary[i], shadow[i], scale[i]).  shadow None: a restart or load that lists the slots of `primary`.
        ValueError with the library's text."""
        who, S, rows = cls.WHO, int(S), int(rows)
        primary = list(primary)
        n = len(primary)
        if n < 1:
            raise ValueError(who + "no slot given")
        mate = [-1] * S
        for b, g in enumerate(guide):
            if g >= 0:
                mate[b], mate[g] = g, b

        def in_range(i, x):
            if int(x) != x or not 0 <= int(x) < S:
                raise ValueError(who + f"entry {i}: slot {x} is outside [0, S = {S})")
        listed = [False] * S
        if shadow is None:
            for i, b in enumerate(primary):
                in_range(i, b)
                listed[int(b)] = True
            for b in primary:
                if mate[int(b)] >= 0 and not listed[mate[int(b)]]:
                    raise ValueError(who + f"slot {int(b)} is paired with slot {mate[int(b)]}: list both")
            return
        shadow, scale = list(shadow), list(scale)
        for i in range(n):
            in_range(i, primary[i])
            in_range(i, shadow[i])
            b, g = int(primary[i]), int(shadow[i])
            if b == g:
                raise ValueError(who + f"slot {b} names itself as its shadow")
            for x in (b, g):
                if listed[x]:
                    raise ValueError(who + f"slot {x} is listed twice")
                if mate[x] >= 0:
                    raise ValueError(who + f"slot {x} is paired with slot {mate[x]}: restart or load both to dissolve the pair")
            listed[b] = listed[g] = True
            if rows > 0 and (fresh[b] == 0 or fresh[b] != fresh[g]):
                raise ValueError(who + f"slot {b} and slot {g} cannot pair at session row {rows}: a pair forms at session row 0 or behind "
                                       f"the call that restarts or loads both slots, ahead of the next step")
            if int(clip_rows[b]) != int(clip_rows[g]):
                raise ValueError(who + f"slot {b} holds a clip of {int(clip_rows[b])} rows, slot {g} one of {int(clip_rows[g])}: a shadow "
                                       f"carries its primary's history from the clip's row 0")
            fault = cls.scale_fault(scale[i])
            if fault:
                raise ValueError(who + f"slot {b}: {fault}")

    @classmethod
    def parse(cls, pairs):
        """`pairs=` of open_stream / restart / load -> ([primary], [shadow], [scale]): {primary: shadow} or {primary: (shadow, scale)}."""
        if not isinstance(pairs, dict):
            raise ValueError(f"pairs: a dict {{primary: shadow}} or {{primary: (shadow, scale)}}, got {type(pairs).__name__}")
        prim, shad, scal = [], [], []
        for b, v in pairs.items():
            g, s = (v[0], v[1]) if isinstance(v, (tuple, list)) and len(v) == 2 else (v, cls.DEFAULT_SCALE)
            if isinstance(g, (tuple, list, dict)) or isinstance(b, (tuple, list)):
                raise ValueError(f"pairs: the entry of slot {b} is a shadow slot or (shadow, scale), got {v!r}")
            prim.append(b), shad.append(g), scal.append(s)
        return prim, shad, scal

    def fresh_now(self, rows):
        """The serials as the rule reads them at session row `rows`: a step since the call that set them makes every slot stale."""
        return list(self.fresh) if self.fresh_at == int(rows) else [0] * self.S

    def check_touch(self, rows, slots):
        """What a restart or a load of `slots` checks of the pairs."""
        if any(g >= 0 for g in self.guide):
            self.check(self.S, rows, self.guide, [0] * self.S, self.fresh_now(rows), slots)

    def touched(self, rows, slots):
        """Behind a restart or a load of `slots` at session row `rows`: their pairs are dissolved, their serial is the call's."""
        self.fresh = self.fresh_now(rows)
        self.fresh_at = int(rows)
        self.serial += 1
        for b in slots:
            self.fresh[b] = self.serial
            if self.guide[b] >= 0:
                self.guide[b], self.scale[b] = -1, 0.0
        return self

    def copy(self):
        c = SlotPairs(self.S)
        c.guide, c.scale, c.fresh, c.fresh_at, c.serial = list(self.guide), list(self.scale), list(self.fresh), self.fresh_at, self.serial
        return c

    def pair(self, rows, clip_rows, primary, shadow, scale):
        """Declare the pairs at session row `rows` (all or none)."""
        self.check(self.S, rows, self.guide, clip_rows, self.fresh_now(rows), primary, shadow, scale)
        for b, g, s in zip(primary, shadow, scale):
            self.guide[int(b)], self.scale[int(b)] = int(g), _f32(s)
        return self

    @property
    def pairs(self):
        """{primary: (shadow, stored scale)}."""
        return {b: (g, self.scale[b]) for b, g in enumerate(self.guide) if g >= 0}

    def step_scales(self, guide, who="step"):
        """`guide=` of a step -> None (the stored scales) or the (S,) list of floats the step runs under (0.0 where no primary sits).
        A float applies to all pairs; a {primary: scale} dict or an (S,) list with None at non-primaries sets scales per pair (a primary
        left out keeps its stored scale).  ValueError naming the slot: a scale for a slot that is no primary, a NaN, an infinity,
        |scale| > 1e4."""
        if guide is None:
            return None
        out = list(self.scale)
        if isinstance(guide, dict):
            items = list(guide.items())
        elif isinstance(guide, (list, tuple)):
            if len(guide) != self.S:
                raise ValueError(f"{who}: guide holds one entry per slot (S = {self.S}), got {len(guide)}")
            items = [(b, s) for b, s in enumerate(guide) if s is not None]
        elif isinstance(guide, (int, float)) and not isinstance(guide, bool):
            items = [(b, guide) for b, g in enumerate(self.guide) if g >= 0]
            if not items:
                raise ValueError(f"{who}: guide: the session holds no pair")
        else:
            raise ValueError(f"{who}: guide is None, a float, a {{primary: scale}} dict or an (S,) list, got {type(guide).__name__}")
        for b, s in items:
            if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.S:
                raise ValueError(f"{who}: guide: slot {b} is outside [0, S = {self.S})")
            if self.guide[b] < 0:
                raise ValueError(f"{who}: guide: slot {b} is no primary of a pair")
            fault = self.scale_fault(s) if isinstance(s, (int, float)) and not isinstance(s, bool) else "the scale is not a number"
            if fault:
                raise ValueError(f"{who}: guide: slot {b}: {fault}")
            out[b] = _f32(s)
        return out


class BodyGuide:
    """Guidance at CLIP level in a body session (`TrainWrapper.open_stream(..., guide=)`; DESIGN.md §5, "session pairs"), on the host: the
    entries a session is opened with, the slot layout they give, and the `guide=` of a push.  The chain session behind a body session of
    B clips has S = B + n_g slots: the clips in slots 0 .. B-1 (so Philox clip indices stay clip_index0 + b without a table, and the
    clips' rows of a step's code block are its first B), the shadows behind them in clip order.  The audio encoder runs on E = B + n_a
    MFCC streams, n_a the shadows with audio of their own; a shadow that shares its clip's audio gets the clip's ENCODED rows.  Pure
    Python: nothing is launched."""

    KEYS = ("scale", "id", "style", "audio")

    def __init__(self, guide, B, n_classes, who="open_stream"):
        self.B, self.NC = int(B), int(n_classes)
        self.entries = self.parse(guide, self.B, self.NC, who)
        self.shadow_of, self.enc_of, self.S, self.E = self.layout([e is not None for e in self.entries],
                                                                  [bool(e and e["audio"]) for e in self.entries])
        self.slot_of = {b: self.B + k for k, b in enumerate(self.shadow_of)}      # clip -> its shadow's slot

    @classmethod
    def entry(cls, e, b, NC, who):
        """One entry -> None or {"scale", "id", "style", "audio"}; ValueError naming clip b."""
        if e is None:
            return None
        if not isinstance(e, dict):
            raise ValueError(f"{who}: guide of clip {b}: an entry is None or a dict with the keys {cls.KEYS}, got {type(e).__name__}")
        unknown = sorted(set(e) - set(cls.KEYS))
        if unknown:
            raise ValueError(f"{who}: guide of clip {b}: unknown keys {unknown} {cls.KEYS}")
        if "scale" not in e:
            raise ValueError(f"{who}: guide of clip {b}: \"scale\" is required")
        s = e["scale"]
        fault = SlotPairs.scale_fault(s) if isinstance(s, (int, float)) and not isinstance(s, bool) else "the scale is not a number"
        if fault:
            raise ValueError(f"{who}: guide of clip {b}: {fault}")
        i = e.get("id")
        if i is not None and (isinstance(i, bool) or int(i) != i or not 0 <= int(i) < NC):
            raise ValueError(f"{who}: guide of clip {b}: id {i} is outside [0, n_classes = {NC})")
        row = e.get("style")
        if row is not None:
            row = row.detach().cpu().numpy() if hasattr(row, "detach") else row
            row = list(row.tolist() if hasattr(row, "tolist") else row)
            if len(row) != NC or any(isinstance(v, (list, tuple)) for v in row):
                raise ValueError(f"{who}: guide of clip {b}: a style row holds n_classes = {NC} weights (a session takes no tracks)")
            row = [float(v) for v in row]
            if any(v != v or v in (float("inf"), float("-inf")) for v in row):
                raise ValueError(f"{who}: guide of clip {b}: a style weight is not finite")
        a = e.get("audio", False)
        if not isinstance(a, bool):
            raise ValueError(f"{who}: guide of clip {b}: \"audio\" is True (every push brings the shadow's MFCC chunk) or False")
        return {"scale": _f32(s), "id": None if i is None else int(i), "style": row, "audio": a}

    @classmethod
    def parse(cls, guide, B, NC, who="open_stream"):
        """`guide=` of open_stream -> B entries: None, one dict for all clips, or a list of B."""
        if guide is None:
            return [None] * B
        if isinstance(guide, dict):
            guide = [guide] * B
        if not isinstance(guide, (list, tuple)) or len(guide) != B:
            raise ValueError(f"{who}: guide is None, one dict for all clips or a list with one entry per clip (B = {B})")
        return [cls.entry(e, b, NC, who) for b, e in enumerate(guide)]

    @staticmethod
    def layout(present, audio):
        """present[b]: clip b has a shadow; audio[b]: the shadow hears audio of its own -> (shadow_of (n_g,) the clip of every shadow,
        enc_of (n_g,) its encoder stream or -1 = the clip's, S, E)."""
        B = len(present)
        shadow_of = [b for b in range(B) if present[b]]
        enc_of, E = [], B
        for b in shadow_of:
            if audio[b]:
                enc_of.append(E)
                E += 1
            else:
                enc_of.append(-1)
        return shadow_of, enc_of, B + len(shadow_of), E

    def spread(self):
        """(S,) the encoder stream whose rows chain slot s hears."""
        return list(range(self.B)) + [e if e >= 0 else b for b, e in zip(self.shadow_of, self.enc_of)]

    def pairs(self):
        """{clip: (shadow slot, stored scale)} for `PixelCNNStream`."""
        return {b: (self.slot_of[b], self.entries[b]["scale"]) for b in self.shadow_of}

    def spread_kw(self, name, v, shadow_style, who="push"):
        """A per-clip keyword of B entries as the S entries of the chain session: a shadow's entry of sampling / code_bias / repeat / given
        is never read (None), its `style` entry is its own conditioning (shadow_style[clip], else None: its id), its uniforms are zeros."""
        import torch
        B = self.B
        if v is None or not self.shadow_of:
            return v
        if name == "style":
            rows = torch.as_tensor(v).detach().cpu().numpy() if not isinstance(v, (list, tuple)) else None
            if rows is not None:
                v = [rows] * B if rows.ndim == 1 else list(rows)
            if len(v) != B:
                raise ValueError(f"{who}: style holds one row for all clips or one per clip (B = {B}), got {len(v)}")
            return list(v) + [shadow_style.get(b) for b in self.shadow_of]
        if name == "uniforms":
            u = torch.as_tensor(v, dtype=torch.float32)
            if u.dim() != 3 or int(u.shape[0]) != B:
                raise ValueError(f"{who}: uniforms must have shape (B={B}, Hc, 2), got {tuple(u.shape)}")
            return torch.cat([u, torch.zeros((self.S - B,) + tuple(u.shape[1:]), dtype=u.dtype, device=u.device)])
        if name == "given" and not isinstance(v, (list, tuple)):
            v = list(v)
        if isinstance(v, list):
            if len(v) != B:
                raise ValueError(f"{who}: {name} holds one entry per clip (B = {B}), got {len(v)}")
            return list(v) + [None] * (self.S - B)
        return v

    def push(self, guide, t, who="push", need_mfcc=True):
        """`guide=` of a push of t frames -> ({clip: scale} or None, [the MFCC chunk of every shadow with audio of its own, in encoder
        order]).  None, a float (all guided clips), or a list with, per clip, None, a float or {"scale": s, "mfcc": (t, 64)}.  A clip
        opened with "audio": True must bring "mfcc" of the chunk's own t, a clip opened without must not (need_mfcc=False: a flush, which
        brings no audio at all).  ValueError naming the clip."""
        B = self.B
        if guide is None or (isinstance(guide, (int, float)) and not isinstance(guide, bool)):
            if guide is not None and not self.shadow_of:
                raise ValueError(f"{who}: guide: the session was opened without a shadow")
            per = [guide if self.entries[b] is not None else None for b in range(B)]
        elif isinstance(guide, (list, tuple)) and len(guide) == B:
            per = list(guide)
        else:
            raise ValueError(f"{who}: guide is None, a float or a list with one entry per clip (B = {B})")
        scales, chunks = {}, []
        for b, e in enumerate(per):
            opened = self.entries[b]
            if opened is None:
                if e is not None:
                    raise ValueError(f"{who}: guide of clip {b}: the clip was opened without a shadow")
                continue
            m = None
            if isinstance(e, dict):
                unknown = sorted(set(e) - {"scale", "mfcc"})
                if unknown:
                    raise ValueError(f"{who}: guide of clip {b}: unknown keys {unknown} ('scale', 'mfcc')")
                m, e = e.get("mfcc"), e.get("scale")
            if e is not None:
                fault = SlotPairs.scale_fault(e) if isinstance(e, (int, float)) and not isinstance(e, bool) else "the scale is not a number"
                if fault:
                    raise ValueError(f"{who}: guide of clip {b}: {fault}")
                scales[b] = _f32(e)
            if opened["audio"] and need_mfcc:
                if m is None or tuple(getattr(m, "shape", ())) != (int(t), 64):
                    raise ValueError(f"{who}: guide of clip {b}: the shadow was opened with audio of its own: \"mfcc\" of shape ({int(t)}, 64) "
                                     f"is required, got {None if m is None else tuple(getattr(m, 'shape', ()))}")
                chunks.append(m)
            elif m is not None:
                raise ValueError(f"{who}: guide of clip {b}: the shadow was opened without audio of its own: it takes no \"mfcc\"")
        return (scales or None), chunks


class SlotState:
    """The saved state of one or more slots (`PixelCNNStream.save`; talkshow_hip.h, "slot state"): `words` (n, W) int32, one row per slot
    in `SlotClock.state_layout`, on any device, and `infos`, one dict per row (D, NL, NC, V, version, rows, clip_index, label, hist).
    Indexing gives the state of the chosen rows; `.to(device)` / `.cpu()` move the words; `tobytes()` / `frombytes()` make it portable."""
    _FIELDS = ("D", "NL", "NC", "V", "version", "hist", "rows", "clip_index", "label")
    _MAGIC = b"TSSLOT01"

    def __init__(self, words, infos):
        self.words, self.infos = words, [dict(o) for o in infos]
        if len(self.infos) != int(words.shape[0]):
            raise ValueError(f"SlotState: {int(words.shape[0])} rows of words but {len(self.infos)} records")

    def __len__(self):
        return len(self.infos)

    def __getitem__(self, i):
        idx = [i] if isinstance(i, int) else (list(range(len(self)))[i] if isinstance(i, slice) else [int(k) for k in i])
        idx = [k + len(self) if k < 0 else k for k in idx]
        return SlotState(self.words[idx].contiguous(), [self.infos[k] for k in idx])

    @property
    def device(self):
        return self.words.device

    @property
    def rows(self):
        return [int(o["rows"]) for o in self.infos]

    def to(self, device):
        return SlotState(self.words.to(device), self.infos)

    def cpu(self):
        return self.to("cpu")

    def tobytes(self):
        import struct
        w = self.words.detach().cpu().contiguous().numpy()
        head = self._MAGIC + struct.pack("<2q", w.shape[0], w.shape[1])
        recs = b"".join(struct.pack("<6i3q", *[int(o[k]) for k in self._FIELDS]) for o in self.infos)
        return head + recs + w.astype("<i4", copy=False).tobytes()

    @classmethod
    def frombytes(cls, data):
        import struct

        import numpy as np
        import torch
        data = bytes(data)
        m = len(cls._MAGIC)
        if len(data) < m + 16 or data[:m] != cls._MAGIC:
            raise ValueError("SlotState.frombytes: not a slot state")
        n, W = struct.unpack("<2q", data[m:m + 16])
        if n < 1 or W < 1 or len(data) != m + 16 + n * 48 + n * W * 4:
            raise ValueError(f"SlotState.frombytes: {len(data)} bytes do not hold {n} states of {W} words")
        infos = [dict(zip(cls._FIELDS, struct.unpack("<6i3q", data[m + 16 + 48 * i:m + 16 + 48 * (i + 1)]))) for i in range(n)]
        words = np.frombuffer(data, "<i4", n * W, m + 16 + 48 * n).reshape(n, W).astype(np.int32)
        return cls(torch.from_numpy(words), infos)


class SeamlessBodyStream:
    """See `TrainWrapper.open_stream(..., seamless=True)`: the host handle of `ts_body_stream` (talkshow_hip.h, "seamless sessions")."""

    def _no_state(self, *a, **k):
        """Not taken by a seamless session (talkshow_hip.h, "slot state")."""
        raise NotImplementedError("a seamless session saves and loads no slot state: its MFCC tail and its code ring sit on the SESSION's row "
                                  "grid; use a plain session (open_stream(..., seamless=False))")
    save = load = fork = _no_state

    def restart(self, *a, **k):
        """Not taken by a seamless session (talkshow_hip.h, "slot restart")."""
        raise NotImplementedError("a seamless session restarts no slot: its encoder and decoder windows are cut on the SESSION's row grid and "
                                  "all its clips have one length; use a plain session (open_stream(..., seamless=False)) or open another")

    def __init__(self, wrapper, id, B, max_frames, sampling=None, style=None, code_bias=None, repeat=None, seed=None, guide=None):
        import ctypes as C

        import numpy as np
        import torch

        from talkshow_amd import _lib
        from talkshow_amd.modules import _index_tensor
        gen = wrapper.generator
        if not (gen.audio and gen.bh_model):
            raise NotImplementedError("streaming sessions exist for the shipped configuration (audio=True, bh_model=True)")
        self.w, self.B, self.max_frames = wrapper, int(B), int(max_frames)
        if self.B < 1 or self.max_frames < 1:
            raise ValueError(f"open_stream: B and max_frames are at least 1, got B={B}, max_frames={max_frames}")
        dev = gen._dev()
        if id is None:
            id = torch.tensor([0])
        label = _index_tensor(id, gen.n_classes, "speaker id", dev)
        if label.numel() == 1 and self.B > 1:
            label = label.repeat(self.B)
        if label.numel() != self.B:
            raise ValueError(f"ids must hold 1 or B={self.B} speaker indices, got {label.numel()}")
        self.defaults = {"sampling": sampling, "style": style, "code_bias": code_bias, "repeat": repeat}
        self._labels = label.detach().cpu().numpy()      # what `style=[None, ...]` stands for: the clip's own label
        self.pose_dim = wrapper.each_dim[1] + wrapper.each_dim[2]
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)   # one random stream per session
        # guidance at clip level (talkshow_hip.h, "seamless sessions": guided sessions): the chain runs S = B + n_g slots, the encoder E streams
        self.g = g = BodyGuide(guide, self.B, gen.n_classes)
        self.S, self.shadow_style = g.S, {}
        h = C.c_void_p()
        if not g.shadow_of:
            with torch.cuda.device(dev):
                _lib.check(_lib.load().ts_body_stream_open(wrapper.audioencoder.handle(), gen.handle(), wrapper.g_body.handle(),
                                                           wrapper.g_hand.handle(), _lib.dptr(label), self.B, self.max_frames, C.byref(h)))
            self._h = h
            return
        ids = list(self._labels) + [self._labels[b] if g.entries[b]["id"] is None else g.entries[b]["id"] for b in g.shadow_of]
        self._labels = np.asarray(ids, np.int64)
        self.defaults = {k: g.spread_kw(k, v, self.shadow_style, who="open_stream") for k, v in self.defaults.items() if k != "style"}
        self.defaults["style"], self._style_default = None, style      # spread at every call: a shadow keeps its own conditioning
        rows = None
        if any(g.entries[b]["style"] is not None for b in g.shadow_of):     # every shadow then brings a row: its weights, or its id's one-hot
            rows = np.zeros((len(g.shadow_of), gen.n_classes), np.float32)
            for k, b in enumerate(g.shadow_of):
                if g.entries[b]["style"] is not None:
                    rows[k] = self.shadow_style[b] = np.asarray(g.entries[b]["style"], np.float32)
                else:
                    rows[k, int(ids[self.B + k])] = 1.0
        n_g = len(g.shadow_of)
        i32, label_s = C.c_int32 * n_g, torch.as_tensor(self._labels, device=dev)
        rows_dev = None if rows is None else torch.as_tensor(rows, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ts_body_stream_open_guided(
                wrapper.audioencoder.handle(), gen.handle(), wrapper.g_body.handle(), wrapper.g_hand.handle(), _lib.dptr(label_s), self.B, n_g,
                i32(*g.shadow_of), i32(*g.enc_of), _lib.dptr(rows_dev), (C.c_float * n_g)(*[g.entries[b]["scale"] for b in g.shadow_of]),
                self.max_frames, _lib.stream_ptr(), C.byref(h)))
            torch.cuda.current_stream().synchronize()                      # the weight rows were read from this call's own tensor
        self._h = h

    # ---- counters (host reads; nothing synchronises) ----
    def _get(self, name):
        from talkshow_amd import _lib
        if self._h is None:
            raise ValueError("the session is closed")
        return int(getattr(_lib.load(), name)(self._h))

    @property
    def frames_in(self):
        """MFCC frames received."""
        return self._get("ts_body_stream_frames_in")

    @property
    def code_rows(self):
        """Code rows finalised."""
        return self._get("ts_body_stream_code_rows")

    @property
    def frames(self):
        """Pose frames returned."""
        return self._get("ts_body_stream_pose_frames")

    @property
    def state_bytes(self):
        """Device bytes of the session's own buffers: constant from open to close, whatever the history."""
        return self._get("ts_body_stream_state_bytes")

    @property
    def lag_rows(self):
        """Code rows between a row's audio and its poses: 20 (7 + 13), or 27 where the audio encoder is Winograd-lowered too."""
        return self._get("ts_body_stream_lag_rows")

    def graph_captures(self):
        """`PixelCNNStream.graph_captures` of the chain session inside: stands still once the host's push sizes have been met."""
        return self._get("ts_body_stream_captures")

    def plan(self, t, flush=False):
        """(code_rows, pose_frames) the next call — `push` of t frames, or `flush()` with flush=True (t is then not read) — will run and
        return: the row count of that call's `uniforms` / `given`, and its output sizes.  ValueError after the flush, for t < 1 or for
        t > max_frames."""
        import ctypes as C

        from talkshow_amd import _lib
        if self._h is None:
            raise ValueError("the session is closed")
        n, m = C.c_int64(), C.c_int64()
        try:
            _lib.check(_lib.load().ts_body_stream_plan(self._h, 0 if flush else int(t), int(bool(flush)), C.byref(n), C.byref(m)))
        except RuntimeError as e:          # host arithmetic only: a refusal is about the arguments
            raise ValueError(str(e)) from None
        return int(n.value), int(m.value)

    def plan_calls(self, t, flush=False):
        """[(code_rows, pose_frames)] of `push` of t frames (left out for t = 0) and, with flush=True, of the `flush()` after it.  The push is
        `plan(t)`; the flush after it needs no margin: it finalises every code row and pose frame of the frames received that is not out
        yet, (frames_in + t) // 4 rows in all."""
        if not flush:
            return [self.plan(t)] if t else []
        if not t:
            return [self.plan(0, flush=True)]
        n, m = self.plan(t)
        total = (self.frames_in + int(t)) // 4
        return [(n, m), (total - self.code_rows - n, 4 * total - self.frames - m)]

    def _call(self, mfcc, flush, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes,
              guide=None):
        import ctypes as C

        import torch

        from talkshow_amd import _lib
        from talkshow_amd.modules import _dev_f32, step_pieces, upload
        who = "flush" if flush else "push"
        dev = self.w.generator._dev()
        B, t = self.B, 0
        if not flush:
            if not hasattr(mfcc, "shape") or len(mfcc.shape) != 3 or int(mfcc.shape[0]) != B or int(mfcc.shape[2]) != 64:
                raise ValueError(f"push: mfcc must have shape (B={B}, t, 64), got {tuple(getattr(mfcc, 'shape', ()))}")
            t = int(mfcc.shape[1])
        n, m = self.plan(t, flush)                     # ValueError: after the flush, t = 0, t > max_frames
        g, S = self.g, self.S
        scales = chunks = None
        if g.shadow_of or guide is not None:           # ValueError naming the clip; nothing is launched and no counter moves
            scales, chunks = g.push(guide, t, who=who, need_mfcc=not flush)
        if uniforms is not None:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32)          # lists and numpy arrays too
            if tuple(uniforms.shape) != (B, n, 2):
                raise ValueError(f"{who}: this call runs {n} code rows: uniforms must have shape (B={B}, {n}, 2), got {tuple(uniforms.shape)} "
                                 f"(session.plan(t) names the count)")
        if mode == _lib.TS_SAMPLE_UNIFORMS and uniforms is None and n > 0:
            raise ValueError(f"{who}: TS_SAMPLE_UNIFORMS needs uniforms of shape (B={B}, {n}, 2) for the {n} code rows this call runs")
        if given is not None and not isinstance(given, (list, tuple)) and len(getattr(given, "shape", ())) == 3 and int(given.shape[1]) > n:
            raise ValueError(f"{who}: this call runs {n} code rows: a given block holds at most {n} rows per clip, got {tuple(given.shape)}")
        lp = ctl = btab = bidx = rtab = block = table = srows = None
        n_ctl = n_rep = 0
        lp_out = None
        if g.shadow_of:                                # the pieces for the S slots of the chain: the clips', then what a shadow needs
            style = self._style_default if style is None else style
            sampling, given, style, code_bias, repeat, uniforms = (g.spread_kw(k, v, self.shadow_style, who=who) for k, v in (
                ("sampling", sampling), ("given", given), ("style", style), ("code_bias", code_bias), ("repeat", repeat), ("uniforms", uniforms)))
            if torch.is_tensor(logprobs):
                _lib.logprob_request(logprobs, (B, n, 2), dev)
                lp_out, logprobs = logprobs, True
        if n > 0:                                      # the keywords of the chain step this call makes, validated on the host
            lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows = step_pieces(
                self.w.generator, S, self._labels, self.defaults, n, mode, dev, sampling, logprobs, given, style, code_bias, repeat)
        if isinstance(lp, str) or (lp is None and logprobs):
            lp = torch.empty((S, n, 2), dtype=torch.float32, device=dev)
        codes = torch.empty((S, n, 2), dtype=torch.int64, device=dev)
        poses = torch.empty((B, m, self.pose_dim), dtype=torch.float32, device=dev)
        if uniforms is not None:
            uniforms = _dev_f32(uniforms, dev)
        i32p = C.POINTER(C.c_int32)
        block_dev = upload(block, dev) if block is not None else None
        style_dev = upload(srows, dev) if srows is not None else None
        bias_dev = upload(btab, dev) if btab is not None else None
        mid = (mode, _lib.dptr(uniforms) if n > 0 else None, (self.seed if seed is None else int(seed)) & (2 ** 64 - 1), int(clip_index0),
               _lib.dptr(codes) if n > 0 else None, _lib.dptr(poses) if m > 0 else None,
               ctl, n_ctl, _lib.dptr(lp) if n > 0 else None, _lib.dptr(block_dev), table.ctypes.data_as(i32p) if block is not None else None,
               _lib.dptr(style_dev), _lib.dptr(bias_dev), int(btab.shape[0]) if btab is not None else 0,
               bidx.ctypes.data_as(i32p) if btab is not None else None, rtab, n_rep, _lib.stream_ptr())
        lib = _lib.load()
        if g.shadow_of:                                # the guided entries: the MFCC block of the E streams, the step's scales ahead of the stream
            sc = None if scales is None else (C.c_float * S)(*self._scales(scales))
            mid = mid[:-1] + (sc, mid[-1])
            if flush:
                _lib.check(lib.ts_body_stream_flush_guided(self._h, *mid))
            else:
                mf = _dev_f32(mfcc, dev)
                if chunks:
                    mf = torch.cat([mf, torch.stack([_dev_f32(c, dev) for c in chunks])])
                mf = mf.contiguous()
                if mf.data_ptr() % 16:
                    mf = mf.clone()
                _lib.check(lib.ts_body_stream_push_guided(self._h, _lib.dptr(mf), t, *mid))
            codes = codes[:B]                          # the clips' rows are the block's first B
            if lp is not None:
                lp = lp[:B]
                if lp_out is not None:
                    lp_out.copy_(lp)
                    lp = lp_out
        elif flush:
            _lib.check(lib.ts_body_stream_flush(self._h, *mid))
        else:
            mf = _dev_f32(mfcc, dev)
            if mf.data_ptr() % 16:
                mf = mf.clone()
            _lib.check(lib.ts_body_stream_push(self._h, _lib.dptr(mf), t, *mid))
        out = (poses,) + ((codes,) if return_codes else ()) + ((lp,) if lp is not None else ())
        return out[0] if len(out) == 1 else out

    def _scales(self, scales):
        """{clip: scale} of a call -> the (S,) list the guided entries read at primaries: the stored scale where the call brings none."""
        out = [0.0] * self.S
        for b in self.g.shadow_of:
            out[b] = scales.get(b, self.g.entries[b]["scale"])
        return out

    def push(self, mfcc, mode=2, seed=None, clip_index0=0, uniforms=None, *, sampling=None, logprobs=False, given=None, style=None,
             code_bias=None, repeat=None, return_codes=False, guide=None):
        """mfcc (B, t, 64), any t in 1 .. max_frames -> poses (B, m, 129), the next m = 4 x (code rows whose poses became final) frames of
        the clip — possibly 0, as during a clip's first ~80 frames; leftover frames are carried.  The call runs n code rows (`plan(t)`
        names n and m beforehand): `uniforms` (B, n, 2), `given` and the keywords `sampling`, `style`, `code_bias`, `repeat` — the forms and
        rules of `PixelCNNStream.step`, the session's defaults standing in for None — apply to THOSE rows; with n = 0 they are not read.
        return_codes=True: (poses, codes (B, n, 2)); logprobs=True adds their log-probabilities (B, n, 2) last.  mode 2 is
        TS_SAMPLE_PHILOX.  A bad value raises ValueError before any device work, and no counter moves.
        guide (a session opened with `guide=`): None, a float for all guided clips, or per clip None, a float or {"scale": s, "mfcc":
        (t, 64)} (`BodyGuide.push`): the call's scales and the MFCC chunk of every shadow opened with "audio": True.  The caller gets the
        B clips' results."""
        return self._call(mfcc, False, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes,
                          guide)

    def flush(self, mode=2, seed=None, clip_index0=0, uniforms=None, *, sampling=None, logprobs=False, given=None, style=None, code_bias=None,
              repeat=None, return_codes=False, guide=None):
        """The end of the clip: the rows and frames held back (`plan(0, flush=True)`), in the form `push` returns them.  Over the session
        the returned frames sum to 4 * (frames_in // 4), and equal `generate_batch` on the concatenated audio bit for bit.  A later push
        raises ValueError."""
        return self._call(None, True, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes, guide)

    def close(self):
        if getattr(self, "_h", None) is not None:
            import torch

            from talkshow_amd import _lib
            torch.cuda.synchronize()
            _lib.load().ts_body_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WavBodyStream:
    """See `TrainWrapper.open_stream(..., wav_sr=...)`: a body session fed SAMPLES.  It owns an `MFCCStream` (talkshow_hip.h, "wav
    sessions") and the body session the frames go into; nothing leaves the device and nothing synchronises between the two.
      push_wav(wav (B,n), **push keywords)  -> poses [, codes][, log-probabilities] as `push` of the body session returns them; a call that
                                            yields no MFCC frame (or, in a plain session, fewer than 4 with the carried ones) makes no body
                                            call and returns empty tensors
      flush(**keywords)                     flushes the front end, pushes the last frames and (seamless) flushes the body session
      plan_wav(n, flush=False)              -> (MFCC frames, code rows, pose frames) of that call: the row count of its `uniforms` / `given`
    seamless=True: the frames go straight into the seamless session; with db = the recordings' maxima (`MFCC.peak_db`) every chunking of the
    samples returns the bits of `generate_batch(MFCC(...)(wav), ...)`.  seamless=False: the plain session drops T % 4 frames per chunk, so
    the wrapper forwards frames in multiples of 4 and carries the remainder: what comes back equals `BodyStream.push` of the same frame
    blocks.  ALL SLOTS SHARE ONE SAMPLE CLOCK: `restart`, `save`, `load` and `fork` raise NotImplementedError."""

    def _no_slots(self, *a, **k):
        """Not taken by a wav-fed session (talkshow_hip.h, "wav sessions")."""
        raise NotImplementedError("a wav-fed session restarts, saves, loads and forks no slot: its slots share one sample clock; feed MFCC "
                                  "frames to a plain session (open_stream(..., seamless=False)) for those")
    restart = save = load = fork = _no_slots

    def __init__(self, wrapper, id, B, max_frames, seamless, wav_sr, wav_db="running", max_samples=None, fps=30, **defaults):
        from talkshow_amd.frontend import WavStreamPlan
        from talkshow_amd.modules import MFCC
        self.w, self.B, self.seamless = wrapper, int(B), bool(seamless)
        for b, e in enumerate(BodyGuide.parse(defaults.get("guide"), self.B, wrapper.generator.n_classes)):
            if e is not None and e["audio"]:       # id or style guidance only: the MFCC rows come from the B-slot front end
                raise NotImplementedError(f"open_stream: guide of clip {b}: a wav-fed session takes shadows WITHOUT audio of their own (id or "
                                          f"style guidance): the front end would need slots for the shadows' samples; feed MFCC frames "
                                          f"(wav_sr=None) for \"audio\": True")
        clock = WavStreamPlan(wav_sr, 22000, fps)                # ValueError: rates, fps
        if max_samples is None:                                   # the samples of max_frames rows
            max_samples = max(1, int(max_frames) * clock.hop * clock.norig // clock.nnew)
        self.mfcc = MFCC(wav_sr, 22000, fps, device=wrapper.generator._dev())
        self.front = self.mfcc.open_stream(self.B, max_samples, db=wav_db)
        try:
            frames_cap = max(int(max_frames), self.front.max_frames + 3)       # one call's rows, and a plain session's carried ones
            self.max_frames = frames_cap
            if self.seamless:
                self.body = SeamlessBodyStream(wrapper, id, B, frames_cap, **defaults)
            else:
                from nets.smplx_body_pixel import BodyStream
                self.body = BodyStream(wrapper, id, B, frames_cap, **defaults)
                self._carry = None
        except Exception:
            self.front.close()
            raise
        self.pose_dim = wrapper.each_dim[1] + wrapper.each_dim[2]

    # ---- counters ----
    @property
    def samples_in(self):
        return self.front.samples_in

    @property
    def frames_in(self):
        """MFCC frames the front end has produced."""
        return self.front.frames_out

    @property
    def frames(self):
        """Pose frames returned."""
        return self.body.frames

    @property
    def state_bytes(self):
        """Device bytes of the front end's buffers (and of the seamless session's): constant from open to close."""
        return self.front.state_bytes + (self.body.state_bytes if self.seamless else 0)

    def _body_plan(self, f, flush):
        """[(code rows, pose frames)] of the body calls a wav call of f new frames makes, in order."""
        if not self.seamless:
            t = (f + (0 if self._carry is None else int(self._carry.shape[1]))) // 4 * 4
            return [(t // 4, t)] if t else []
        return self.body.plan_calls(f, flush)

    def plan_wav(self, n, flush=False):
        """(MFCC frames, code rows, pose frames) of the next call: `push_wav` of n samples, or `flush()` with flush=True (n is not read)."""
        f = self.front.plan(n, flush)
        calls = self._body_plan(f, flush)
        return f, sum(c[0] for c in calls), sum(c[1] for c in calls)

    def _empty(self, logprobs, return_codes):
        import torch
        dev = self.w.generator._dev()
        out = (torch.empty((self.B, 0, self.pose_dim), dtype=torch.float32, device=dev),)
        out += ((torch.empty((self.B, 0, 2), dtype=torch.int64, device=dev),) if return_codes else ())
        out += ((torch.empty((self.B, 0, 2), dtype=torch.float32, device=dev),) if logprobs else ())
        return out[0] if len(out) == 1 else out

    _KEYWORDS = ("mode", "seed", "clip_index0", "uniforms", "sampling", "logprobs", "given", "style", "code_bias", "repeat", "return_codes",
                 "guide")

    def _check(self, wav, flush, kw):
        """Everything a call can be refused for, on the host, before the front end is given a sample: the wav block's shape and size, the
        keywords' names, and for every body call this call will make the checks that body call makes itself (`step_pieces` with its
        planned row count).  -> (MFCC rows, the body calls' (code rows, pose frames), uniforms as a host tensor or None)"""
        import torch

        from talkshow_amd import _lib
        from talkshow_amd.modules import step_pieces
        who = "flush" if flush else "push_wav"
        n_samples = 0
        if not flush:
            shape = tuple(int(v) for v in getattr(wav, "shape", ()))
            if len(shape) == 1 and self.B == 1:
                shape = (1,) + shape
            if len(shape) != 2 or shape[0] != self.B:
                raise ValueError(f"push_wav: wav must have shape (B={self.B}, n), got {tuple(getattr(wav, 'shape', ()))}")
            n_samples = shape[1]
        for name in kw:
            if name not in self._KEYWORDS:
                raise TypeError(f"{who}: unknown keyword {name!r}")
        f = self.front.plan(n_samples, flush)                       # ValueError: after the flush, n out of range, a too-short recording
        calls = self._body_plan(f, flush)
        rows = sum(c[0] for c in calls)
        mode, uniforms, given = kw.get("mode", _lib.TS_SAMPLE_PHILOX), kw.get("uniforms"), kw.get("given")
        if not self.seamless and kw.get("return_codes"):
            raise ValueError(f"{who}: a plain session returns no codes (open the session with seamless=True)")
        if uniforms is not None:
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
            if tuple(uniforms.shape) != (self.B, rows, 2):
                raise ValueError(f"{who}: this call runs {rows} code rows: uniforms must have shape (B={self.B}, {rows}, 2), got "
                                 f"{tuple(uniforms.shape)} (session.plan_wav(n) names the count)")
        if mode == _lib.TS_SAMPLE_UNIFORMS and uniforms is None and rows > 0:
            raise ValueError(f"{who}: TS_SAMPLE_UNIFORMS needs uniforms of shape (B={self.B}, {rows}, 2) for the {rows} code rows this call runs")
        # `given` goes to the one body call that runs code rows (a flush makes two calls, and often one of them runs none)
        if given is not None and len([c for c in calls if c[0]]) > 1:
            raise ValueError("flush: the closing call makes two body calls that run code rows: give `given` rows to the pushes before it")
        if given is not None and not isinstance(given, (list, tuple)) and len(getattr(given, "shape", ())) == 3 and int(given.shape[1]) > rows:
            raise ValueError(f"{who}: this call runs {rows} code rows: a given block holds at most {rows} rows per clip, got {tuple(given.shape)}")
        if not any(kw.get("logprobs") is v for v in (None, False, True)):
            raise ValueError(f"{who}: logprobs is True or False (a wav call may make two body calls: it returns a tensor of its own)")
        chain = self.body if self.seamless else self.body.pix          # whose labels and defaults the step keywords meet
        gen = self.w.generator
        g = self.body.g
        if g.shadow_of or kw.get("guide") is not None:                 # the call's scales (no shadow of a wav session brings audio)
            g.push(kw.get("guide"), 0, who=who, need_mfcc=False)
        pieces = {k: kw.get(k) for k in ("sampling", "style", "code_bias", "repeat")}
        pieces["given"] = given
        if g.shadow_of:                                                # the S slots of the chain: the clips', then what a shadow needs
            if pieces["style"] is None:
                pieces["style"] = self.body._style_default
            pieces = {k: g.spread_kw(k, v, self.body.shadow_style, who=who) for k, v in pieces.items()}
        for nrows, _ in calls:
            if nrows > 0:                                              # ValueError naming the clip; nothing is launched or uploaded
                step_pieces(gen, g.S, chain._labels, chain.defaults, nrows, mode, gen._dev(), pieces["sampling"],
                            True if g.shadow_of and kw.get("logprobs") else kw.get("logprobs"), pieces["given"], pieces["style"],
                            pieces["code_bias"], pieces["repeat"])
        return f, calls, uniforms

    def _call(self, wav, flush, kw):
        import torch
        f, calls, uniforms = self._check(wav, flush, kw)
        feat = self.front.flush() if flush else self.front.push(wav)
        if not self.seamless:
            if self._carry is not None:
                feat = torch.cat([self._carry, feat], dim=1)
            t = int(feat.shape[1]) // 4 * 4
            self._carry = feat[:, t:].contiguous() if feat.shape[1] > t else None
            if t == 0:
                return self._empty(kw.get("logprobs"), False)
            return self.body.push(feat[:, :t].contiguous(), **{k: v for k, v in kw.items() if k != "return_codes"})
        outs, r0 = [], 0
        for i, (nrows, _) in enumerate(calls):
            k = dict(kw)
            if uniforms is not None:
                k["uniforms"] = uniforms[:, r0:r0 + nrows].contiguous()
            r0 += nrows
            if nrows == 0:                      # `given` rows are the rows of the one body call that runs code rows (_check)
                k.pop("given", None)
            last = flush and i == len(calls) - 1
            out = self.body.flush(**k) if last else self.body.push(feat, **k)
            outs.append(out if isinstance(out, tuple) else (out,))
        if not outs:
            return self._empty(kw.get("logprobs"), kw.get("return_codes"))
        out = tuple(torch.cat(parts, dim=1) for parts in zip(*outs)) if len(outs) > 1 else outs[0]
        return out[0] if len(out) == 1 else out

    def push_wav(self, wav, **kw):
        """wav (B,n) samples at wav_sr, 0 <= n <= max_samples; the keywords of the body session's `push` apply to the code rows this call
        runs (`plan_wav(n)` names them).  A bad value raises ValueError before any device work, and no counter moves."""
        return self._call(wav, False, kw)

    def flush(self, **kw):
        """The end of the recording: the front end's last frames go through the body session, and a seamless session is flushed.  `uniforms`
        holds the rows of both body calls, in order."""
        return self._call(None, True, kw)

    def close(self):
        try:
            self.front.close()
        finally:
            self.body.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
