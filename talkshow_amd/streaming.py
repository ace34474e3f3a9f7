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

    def __init__(self, wrapper, id, B, max_frames, sampling=None, style=None, code_bias=None, repeat=None, seed=None):
        import ctypes as C

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
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ts_body_stream_open(wrapper.audioencoder.handle(), gen.handle(), wrapper.g_body.handle(),
                                                       wrapper.g_hand.handle(), _lib.dptr(label), self.B, self.max_frames, C.byref(h)))
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

    def _call(self, mfcc, flush, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes):
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
        if n > 0:                                      # the keywords of the chain step this call makes, validated on the host
            lp, ctl, n_ctl, btab, bidx, rtab, n_rep, block, table, srows = step_pieces(
                self.w.generator, B, self._labels, self.defaults, n, mode, dev, sampling, logprobs, given, style, code_bias, repeat)
        if isinstance(lp, str) or (lp is None and logprobs):
            lp = torch.empty((B, n, 2), dtype=torch.float32, device=dev)
        codes = torch.empty((B, n, 2), dtype=torch.int64, device=dev)
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
        if flush:
            _lib.check(lib.ts_body_stream_flush(self._h, *mid))
        else:
            mf = _dev_f32(mfcc, dev)
            if mf.data_ptr() % 16:
                mf = mf.clone()
            _lib.check(lib.ts_body_stream_push(self._h, _lib.dptr(mf), t, *mid))
        out = (poses,) + ((codes,) if return_codes else ()) + ((lp,) if lp is not None else ())
        return out[0] if len(out) == 1 else out

    def push(self, mfcc, mode=2, seed=None, clip_index0=0, uniforms=None, *, sampling=None, logprobs=False, given=None, style=None,
             code_bias=None, repeat=None, return_codes=False):
        """mfcc (B, t, 64), any t in 1 .. max_frames -> poses (B, m, 129), the next m = 4 x (code rows whose poses became final) frames of
        the clip — possibly 0, as during a clip's first ~80 frames; leftover frames are carried.  The call runs n code rows (`plan(t)`
        names n and m beforehand): `uniforms` (B, n, 2), `given` and the keywords `sampling`, `style`, `code_bias`, `repeat` — the forms and
        rules of `PixelCNNStream.step`, the session's defaults standing in for None — apply to THOSE rows; with n = 0 they are not read.
        return_codes=True: (poses, codes (B, n, 2)); logprobs=True adds their log-probabilities (B, n, 2) last.  mode 2 is
        TS_SAMPLE_PHILOX.  A bad value raises ValueError before any device work, and no counter moves."""
        return self._call(mfcc, False, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes)

    def flush(self, mode=2, seed=None, clip_index0=0, uniforms=None, *, sampling=None, logprobs=False, given=None, style=None, code_bias=None,
              repeat=None, return_codes=False):
        """The end of the clip: the rows and frames held back (`plan(0, flush=True)`), in the form `push` returns them.  Over the session
        the returned frames sum to 4 * (frames_in // 4), and equal `generate_batch` on the concatenated audio bit for bit.  A later push
        raises ValueError."""
        return self._call(None, True, mode, seed, clip_index0, uniforms, sampling, logprobs, given, style, code_bias, repeat, return_codes)

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

    _KEYWORDS = ("mode", "seed", "clip_index0", "uniforms", "sampling", "logprobs", "given", "style", "code_bias", "repeat", "return_codes")

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
        for nrows, _ in calls:
            if nrows > 0:                                              # ValueError naming the clip; nothing is launched or uploaded
                step_pieces(gen, self.B, chain._labels, chain.defaults, nrows, mode, gen._dev(), kw.get("sampling"), kw.get("logprobs"),
                            given, kw.get("style"), kw.get("code_bias"), kw.get("repeat"))
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
