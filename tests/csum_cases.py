"""Constructed frames at the checksum's arithmetic edges, and an independent
reference for them (CPU only; tests/test_csum_cases.py holds this module to
its claims, tests/test_gpu_csum_edges.py runs the kernels over it).

The reference is RFC 1071 from its definition in Python integers: the frame as
big-endian 16-bit words, bytes 5-6 taken as zero for layout 7, an odd tail
zero-padded, ``S = sum(words)``, folded while it has a carry, complemented.
Nothing here calls ``oracle/`` or folds in numpy.

The classes are defined on S (``classify``):

  ZK     S > 0 and S = 0 (mod 0xFFFF): checksum 0x0000
  Z0     S = 0 (header and payload all zero): checksum 0xFFFF
  NEAR   S = 1 or S = 0xFFFE (mod 0xFFFF): checksum 0xFFFE or 0x0001
  FOLD2  (S & 0xFFFF) + (S >> 16) >= 0x10000: the second fold does work
  TOP    seq = ack = 0xFFFF, flags = 0xFF, payload all 0xFF
  PE/PO  payload 0xFF at the even / the odd payload indices only

A frame lands in a class by solving one whole header word (``ack``, or ``seq``
where a protocol rule pins ``ack``): both are 16-bit words of the sum, so
``S = S0 + value`` at every payload length and the payload stays what it was.
A twin (``ZK_T``, ``Z0_T``) is a ZK or Z0 frame that carries the other of
0x0000 / 0xFFFF (in-band for layout 7, in the sideband for layout 5): it
verifies under "sum everything, expect all ones" and is RUDP_OK_BAD_CSUM under
the contract of include/rudp.h.
"""
from __future__ import annotations

import functools
import struct
from typing import List, NamedTuple, Optional

import numpy as np

MOD = 0xFFFF
OK_BAD_CSUM, OK_GOOD, OK_SHORT, OK_UNVERIFIED = 0, 1, 2, 3

FIXED_LENGTHS = (0, 1, 2, 15, 16, 17, 48, 64, 1472, 4096)
MAX_LENGTHS = (65520, 65535)
TILE_ROWS = 16


# ------------------------------------------------------------------ reference
def ref_csum(frame: bytes, layout: int):
    """(checksum, S) of one frame: S is the plain sum of its big-endian words."""
    b = bytearray(frame)
    if layout == 7:
        for k in (5, 6):
            if k < len(b):
                b[k] = 0
    if len(b) % 2:
        b.append(0)
    S = sum(struct.unpack(">%dH" % (len(b) // 2), bytes(b)))
    s = S
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF, S


def ref_decode(frame: bytes, layout: int, sideband: Optional[int] = None):
    """(seq, ack, flags, ok, csum) as include/rudp.h defines them."""
    F = len(frame)
    b = list(frame[:7]) + [0] * 7
    if F < layout:  # the fields that are present, truncated like a short slice
        seq = (b[0] << 8 | b[1]) if F >= 2 else b[0]
        ack = (b[2] << 8 | b[3]) if F >= 4 else b[2]
        return seq, ack, b[4], OK_SHORT, 0
    csum, _ = ref_csum(frame, layout)
    if layout == 7:
        ok = OK_GOOD if csum == (b[5] << 8 | b[6]) else OK_BAD_CSUM
    elif sideband is not None:
        ok = OK_GOOD if csum == int(sideband) else OK_BAD_CSUM
    else:
        ok = OK_UNVERIFIED
    return b[0] << 8 | b[1], b[2] << 8 | b[3], b[4], ok, csum


def make_frame(seq: int, ack: int, flags: int, payload: bytes, layout: int, carried: Optional[int] = None) -> bytes:
    """The frame's bytes; layout 7 carries ``carried`` (default: the true checksum)."""
    head = struct.pack(">HHB", seq, ack, flags)
    if layout == 5:
        return head + bytes(payload)
    if carried is None:
        carried, _ = ref_csum(head + b"\0\0" + bytes(payload), 7)
    return head + struct.pack(">H", carried) + bytes(payload)


def twin_of(csum: int) -> int:
    """The other of 0x0000 / 0xFFFF."""
    assert csum in (0x0000, 0xFFFF)
    return csum ^ 0xFFFF


def classify(seq: int, ack: int, flags: int, payload: bytes, layout: int) -> set:
    """The classes a frame belongs to, from S and from its bytes."""
    _, S = ref_csum(make_frame(seq, ack, flags, payload, layout, 0), layout)
    p = bytes(payload)
    out = set()
    if S == 0:
        out.add("Z0")
    elif S % MOD == 0:
        out.add("ZK")
    if S % MOD in (1, 0xFFFE):
        out.add("NEAR")
    if (S & 0xFFFF) + (S >> 16) >= 0x10000:
        out.add("FOLD2")
    if seq == ack == 0xFFFF and flags == 0xFF and p == b"\xff" * len(p):
        out.add("TOP")
    if p[0::2] == b"\xff" * len(p[0::2]) and p[1::2] == b"\0" * len(p[1::2]):
        out.add("PE")
    if p[1::2] == b"\xff" * len(p[1::2]) and p[0::2] == b"\0" * len(p[0::2]):
        out.add("PO")
    return out


# ---------------------------------------------------------------- constructors
def solve(seq: int, ack: int, flags: int, payload: bytes, layout: int, residue: int, field: str = "ack") -> int:
    """The value of ``field`` ('ack' or 'seq') that makes S = residue (mod 0xFFFF),
    S > 0 (the given value of that field is ignored)."""
    if field == "ack":
        ack = 0
    else:
        seq = 0
    _, S0 = ref_csum(make_frame(seq, ack, flags, payload, layout, 0), layout)
    v = (residue - S0) % MOD
    if S0 + v == 0:  # an all-zero frame: the non-zero multiple is 0xFFFF itself
        v = MOD
    return v


def solve_fold2(flags: int, payload: bytes, layout: int, seq: int):
    """(seq, ack, flags) whose first fold lands on 0x10000 or above.  The low
    half of S is driven to the top through ``ack``; S must reach 0x10000 for the
    high half to count, so a short payload takes seq = 0xFFFF and flags = 0xFF."""
    for s, f in ((seq, flags), (0xFFFF, flags | 0x80), (0xFFFF, 0xFF)):
        _, S0 = ref_csum(make_frame(s, 0, f, payload, layout, 0), layout)
        for low in (0xFFFF, 0xFFFE, 0xFFF0, 0xFF00):
            a = (low - S0) & 0xFFFF
            S = S0 + a
            if (S & 0xFFFF) + (S >> 16) >= 0x10000:
                return s, a, f
    raise AssertionError("no FOLD2 frame found")


def _pattern(kind: str, L: int, rng) -> bytes:
    if kind == "rand":
        return rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    if kind == "ascii":
        return rng.integers(0x20, 0x7F, L, dtype=np.uint8).tobytes()
    if kind == "ff":
        return b"\xff" * L
    if kind == "zero":
        return b"\0" * L
    p = bytearray(L)
    p[(0 if kind == "even" else 1)::2] = b"\xff" * len(p[(0 if kind == "even" else 1)::2])
    return bytes(p)


def class_fields(name: str, L: int, layout: int, rng, payload_kind: Optional[str] = None):
    """(seq, ack, flags, payload) of one frame of class ``name`` (a twin's fields
    are those of its class; what it carries is the caller's business)."""
    base = name[:-2] if name.endswith("_T") else name
    seq, flags = int(rng.integers(0, 0x10000)), int(rng.integers(0, 0x100))
    ack = int(rng.integers(0, 0x10000))
    if base == "Z0":
        return 0, 0, 0, b"\0" * L
    if base == "TOP":
        return 0xFFFF, 0xFFFF, 0xFF, b"\xff" * L
    if base in ("PE", "PO"):
        return seq, ack, flags, _pattern("even" if base == "PE" else "odd", L, rng)
    pay = _pattern(payload_kind or "rand", L, rng)
    if base == "RAND":
        return seq, ack, flags, pay
    if base == "ZK":
        return seq, solve(seq, 0, flags, pay, layout, 0), flags, pay
    if base == "NEAR1":
        return seq, solve(seq, 0, flags, pay, layout, 1), flags, pay
    if base == "NEARM":
        return seq, solve(seq, 0, flags, pay, layout, 0xFFFE), flags, pay
    if base == "FOLD2":
        s, a, f = solve_fold2(flags, pay, layout, seq)
        return s, a, f, pay
    raise KeyError(name)


# what classify() must say of a frame built as class X
CLASS_OF = {"ZK": "ZK", "ZK_T": "ZK", "Z0": "Z0", "Z0_T": "Z0", "NEAR1": "NEAR", "NEARM": "NEAR", "FOLD2": "FOLD2",
            "TOP": "TOP", "PE": "PE", "PO": "PO"}
CLASSES = tuple(CLASS_OF)


class Frame(NamedTuple):
    label: str        # the class it was built as ('RAND': none; 'SHORT': shorter than the header)
    seq: int
    ack: int
    flags: int
    payload: bytes
    raw: Optional[bytes] = None   # SHORT only: the frame's bytes

    @property
    def twin(self) -> bool:
        return self.label.endswith("_T")


@functools.lru_cache(maxsize=4096)
def true_csum(fr: Frame, layout: int) -> int:
    """The frame's checksum by ref_csum (kept per frame: a batch asks for it several times)."""
    return ref_csum(make_frame(fr.seq, fr.ack, fr.flags, fr.payload, layout, 0), layout)[0]


def carried_csum(fr: Frame, layout: int) -> int:
    """The value the frame carries (in-band or sideband): the true checksum, or
    for a twin the other of 0x0000 / 0xFFFF."""
    c = true_csum(fr, layout)
    return twin_of(c) if fr.twin else c


def wire_bytes(fr: Frame, layout: int, twins: bool = True) -> bytes:
    """The frame as a decode sees it (``twins``: with the twin's carried value
    in-band) or, without, as the encode must write it."""
    if fr.label == "SHORT":
        return fr.raw
    return make_frame(fr.seq, fr.ack, fr.flags, fr.payload, layout,
                      carried_csum(fr, layout) if twins else true_csum(fr, layout))


def expected_decode(fr: Frame, layout: int, sideband: bool = True):
    """ref_decode of the frame as carried (layout 5: with or without the sideband)."""
    side = carried_csum(fr, layout) if (sideband and layout == 5 and fr.label != "SHORT") else None
    return ref_decode(wire_bytes(fr, layout), layout, side)


# ----------------------------------------------------------- fixed-length batch
# One cycle of rows; every ZK / Z0 row is followed by its twin (the same fields).
# Its length is odd, so over 16 * len(cycle) rows every entry meets every row
# index mod 16: both parities and both sides of every 16-row tile edge.
FIXED_CYCLE = ("ZK", "ZK_T", "Z0", "Z0_T", "NEAR1", "NEARM", "FOLD2", "TOP", "PE", "PO", "ZK:ff", "ZK_T", "RAND")
MAX_CYCLE = ("TOP", "ZK", "ZK_T", "FOLD2", "ZK:ff", "ZK_T", "FOLD2:ff")


class FixedBatch(NamedTuple):
    L: int
    layout: int
    frames: List[Frame]
    seq: np.ndarray       # u16 [n]
    ack: np.ndarray       # u16 [n]
    flags: np.ndarray     # u8 [n]
    payload: np.ndarray   # u8 [n, L]

    @property
    def n(self):
        return len(self.frames)

    @property
    def labels(self):
        return [f.label for f in self.frames]

    def carried(self):
        return np.array([carried_csum(f, self.layout) for f in self.frames], np.uint16)

    def true_csum(self):
        return np.array([true_csum(f, self.layout) for f in self.frames], np.uint16)

    def wire(self, twins=True):
        """u8 [n, L + layout]: the frames as encoded (``twins``: with the twins' carried values)."""
        rows = b"".join(wire_bytes(f, self.layout, twins) for f in self.frames)
        return np.frombuffer(rows, np.uint8).reshape(self.n, self.L + self.layout).copy()

    def expected(self, sideband=True):
        """seq, ack, flags, ok, csum arrays from ref_decode (twins substituted)."""
        cols = list(zip(*(expected_decode(f, self.layout, sideband) for f in self.frames)))
        return tuple(np.array(c, d) for c, d in zip(cols, (np.uint16, np.uint16, np.uint8, np.uint8, np.uint16)))


def _cycle_frames(cycle, n, rot, L, layout, rng):
    out: List[Frame] = []
    for r in range(n):
        entry = cycle[(r + rot) % len(cycle)]
        name, _, kind = entry.partition(":")
        if name.endswith("_T") and out and out[-1].label == name[:-2]:
            out.append(out[-1]._replace(label=name))  # the copy of the frame before it
        else:
            out.append(Frame(name, *class_fields(name, L, layout, rng, kind or None)))
    return out


def _as_fixed(frames, L, layout):
    return FixedBatch(L, layout, frames,
                      np.array([f.seq for f in frames], np.uint16), np.array([f.ack for f in frames], np.uint16),
                      np.array([f.flags for f in frames], np.uint8),
                      np.frombuffer(b"".join(f.payload for f in frames), np.uint8).reshape(len(frames), L).copy())


@functools.lru_cache(maxsize=32)
def fixed_batch(L: int, layout: int, rot: int = 0) -> FixedBatch:
    """The fixed-length corpus for one payload length.  ``rot`` rotates the cycle:
    entry ``rot`` of the cycle sits at row 0 and at the last row (only one frame
    can), so the rotations together put every class there; every rotation has
    every class at every row index mod 16."""
    rng = np.random.default_rng(0xC5C5 + 131 * L + 7 * layout + rot)
    if L in MAX_LENGTHS:
        cycle, n = MAX_CYCLE, 2 * len(MAX_CYCLE) + 1          # 15 rows
    else:
        cycle, n = FIXED_CYCLE, 2 * TILE_ROWS * len(FIXED_CYCLE) + 1   # 417 rows
    return _as_fixed(_cycle_frames(cycle, n, rot, L, layout, rng), L, layout)


# ------------------------------------------------------- packed variable-length
class PackedBatch(NamedTuple):
    layout: int
    frames: List[Frame]   # the decode's stream: SHORT frames included

    def encodable(self):
        """Indices (into ``frames``) of the frames an encode can make (not SHORT)."""
        return [i for i, f in enumerate(self.frames) if f.label != "SHORT"]

    def tables(self):
        """seq, ack, flags, packed payload, lengths of the encodable frames."""
        fr = [self.frames[i] for i in self.encodable()]
        return (np.array([f.seq for f in fr], np.uint16), np.array([f.ack for f in fr], np.uint16),
                np.array([f.flags for f in fr], np.uint8),
                np.frombuffer(b"".join(f.payload for f in fr), np.uint8).copy(),
                np.array([len(f.payload) for f in fr], np.int32))

    def encoded(self):
        """The encode's expected output: frames u8, frame_off i64 [n + 1], csum u16 [n]."""
        fr = [self.frames[i] for i in self.encodable()]
        parts = [wire_bytes(f, self.layout, False) for f in fr]
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        cs = np.array([true_csum(f, self.layout) for f in fr], np.uint16)
        return np.frombuffer(b"".join(parts), np.uint8).copy(), off, cs

    def wire(self):
        """The decode's input: frames u8 (twins substituted, SHORT frames in
        place), frame_off i64 [n + 1], sideband u16 [n] (0 for a SHORT frame)."""
        parts = [wire_bytes(f, self.layout) for f in self.frames]
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        side = np.array([0 if f.label == "SHORT" else carried_csum(f, self.layout) for f in self.frames], np.uint16)
        return np.frombuffer(b"".join(parts), np.uint8).copy(), off, side

    def expected(self, sideband=True):
        cols = list(zip(*(expected_decode(f, self.layout, sideband) for f in self.frames)))
        return tuple(np.array(c, d) for c, d in zip(cols, (np.uint16, np.uint16, np.uint8, np.uint8, np.uint16)))

    def valid_utf8(self):
        """u8 [n]: 1 where Python's strict decode accepts the payload (SHORT: empty, so 1)."""
        out = np.zeros(len(self.frames), np.uint8)
        for i, f in enumerate(self.frames):
            try:
                (b"" if f.label == "SHORT" else f.payload).decode()
                out[i] = 1
            except UnicodeDecodeError:
                pass
        return out


PACKED_SPRINKLE = (("ZK", 1472), ("FOLD2", 2944), ("NEAR1", 4000), ("ZK_T", 1472), ("PE", 2944), ("TOP", 65535),
                   ("NEARM", 1472), ("Z0", 4000), ("PO", 1472), ("Z0_T", 1472))
PACKED_COVER = 1900   # frames of the covering section
PACKED_ROT_COVER = 450    # ... of the shorter batches that only rotate the first and last frame's class


@functools.lru_cache(maxsize=32)
def packed_batch(layout: int, rot: int = 0, max_len: int = 40, sprinkle: bool = True,
                 cover: int = PACKED_COVER) -> PackedBatch:
    """About 2000 frames of 0-40 payload bytes with a few long ones (``sprinkle``).

    Frame 0 and the last frame are of class ``CLASSES[rot]``.  Then the covering
    section: at every step the frame offset's value mod 16 picks a class that
    has not started there yet (a filler otherwise), until every class has
    started at all 16 values, and on with the classes in turn.  It holds no
    SHORT frame, so its offsets are the same for the encode and the decode.
    Then every class between two frames shorter than the header (lengths 0 to
    layout - 1 in turn), which only the decode's stream has."""
    rng = np.random.default_rng(0xBA7C4 + 7 * layout + rot + 1000 * max_len)
    frames: List[Frame] = []
    off = 0

    def put(name, L, kind=None):
        nonlocal off
        frames.append(Frame(name, *class_fields(name, L, layout, rng, kind)))
        off += L + layout

    put(CLASSES[rot % len(CLASSES)], int(rng.integers(0, max_len + 1)))
    need = {c: set(range(16)) for c in CLASSES}
    long_at = {120 + 170 * k: s for k, s in enumerate(PACKED_SPRINKLE)} if sprinkle else {}
    turn = 0
    while len(frames) < cover:
        if len(frames) in long_at:
            name, L = long_at.pop(len(frames))
            need[name].discard(off % 16)
            put(name, L)
            continue
        r = off % 16
        wanting = [c for c in CLASSES if r in need[c]]
        if wanting:
            name = max(wanting, key=lambda c: len(need[c]))
            need[name].discard(r)
        elif any(need.values()):
            name = "RAND"
        else:
            name, turn = CLASSES[turn % len(CLASSES)], turn + 1
        kind = ("rand", "ascii", "ff", "zero")[int(rng.integers(0, 4))]
        put(name, int(rng.integers(0, max_len + 1)), kind)
    assert not any(need.values()), "the covering section is too short"
    k = 0
    for name in CLASSES:
        for _ in range(2):
            raw = rng.integers(0, 256, k % layout, dtype=np.uint8).tobytes()
            frames.append(Frame("SHORT", 0, 0, 0, b"", raw))
            k += 1
            if _ == 0:
                put(name, int(rng.integers(0, max_len + 1)))
    put(CLASSES[rot % len(CLASSES)], int(rng.integers(0, max_len + 1)))
    return PackedBatch(layout, frames)


def small_batch(layout: int) -> PackedBatch:
    """The packed corpus at the small-frame tiles' shape: payloads of 0-8 bytes, no long frame."""
    return packed_batch(layout, 0, 8, False, 700)


def fixed_as_packed(b: FixedBatch) -> PackedBatch:
    """A fixed-length batch as a packed one (the maximum lengths in the variable-length forms)."""
    return PackedBatch(b.layout, list(b.frames))


# ------------------------------------------------------------ protocol streams
SYN, ACK, FIN = 0x80, 0x40, 0x20


def zk_datagram(seq: int, flags: int, text: str, layout: int, field: str = "ack", other: int = 0) -> Frame:
    """A ZK frame of a protocol stream: ``field`` is solved, the other of seq /
    ack is ``other`` (the caller's ``seq`` is kept when ``field`` is 'ack')."""
    pay = text.encode()
    if field == "ack":
        return Frame("ZK", seq, solve(seq, 0, flags, pay, layout, 0, "ack"), flags, pay)
    return Frame("ZK", solve(0, other, flags, pay, layout, 0, "seq"), other, flags, pay)


def stream_wire(frames: List[Frame], layout: int):
    """frames u8, frame_off i64 [n + 1], sideband u16 [n] of a list of frames, twins substituted."""
    return PackedBatch(layout, list(frames)).wire()
