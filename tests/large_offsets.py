"""CPU helpers of tests/test_gpu_large_offsets.py (no GPU use; checked by
tests/test_large_offsets_ref.py).

Three things live here:

* *blocks*: a few thousand datagrams built on the CPU, with every answer the
  library owes for them computed from the plain restatements (oracle/codec_np,
  accept_ref, window_ref, ack_ref, dedup_ref);
* *placement*: the base at which a block is copied into a large buffer so that
  a byte line (2^31 or 2^32) falls inside one frame's payload, and the
  assertion that it does;
* *periodic batches*: a block repeated R times.  The expected output is the
  block's output repeated, offsets advanced by r * B; `compare_periodic` checks
  that in row chunks on whatever device the tensors live on and names the first
  differing byte and the line it lies beyond.  `segment_closed_form` gives the
  packets of a periodic message from its period alone.
"""
from __future__ import annotations

import random
from typing import NamedTuple, Optional

import numpy as np

from accept_ref import accept_ref, chars_ref
from accept_ref import scan_model as accept_scan_model
from ack_ref import CUMULATIVE, ack_ref, csum_of, fresh_state, header, info_ref
from ack_ref import scan_model as ack_scan_model
from dedup_ref import proxy_scan
from oracle import codec_np
from window_ref import NONE, ordered_ref, window_ref

SYN, ACK, FIN = 0x80, 0x40, 0x20
LINE31, LINE32 = 1 << 31, 1 << 32
LINES = (LINE31, LINE32)
BIG_BYTES = (1 << 32) + (1 << 21)   # the translated-input buffer
MARGIN = 16                         # bytes kept between a line and either end of its frame
OK_BAD_CSUM, OK_GOOD, OK_SHORT, OK_UNVERIFIED, OK_BAD_OFFSETS = 0, 1, 2, 3, 4
ST_PAYLOAD, ST_FRAMES_CAP, ST_OFFSETS = 2, 4, 8
DUP_BAD_OFFSETS = 2
WINDOW = 64          # dedup window of the blocks
WINDOW_CHARS = 8     # accept_window's window
ACK_ISN, ACK_CHUNK = 100, 8


def beyond(byte_off: int) -> str:
    """Which line a byte offset lies beyond, for messages."""
    if byte_off >= LINE32:
        return "beyond 2^32"
    if byte_off >= LINE31:
        return "beyond 2^31"
    return "below 2^31"


# ---------------------------------------------------------------- placement
def line_margin(off, H: int, i: int) -> int:
    """The margin a line inside frame i must keep: MARGIN when the frame is long
    enough to have such a byte, else 0 (a one-character datagram is 6 to 11
    bytes: the line then lies on a payload byte)."""
    return MARGIN if int(off[i + 1]) - int(off[i]) >= max(H, MARGIN) + MARGIN + 1 else 0


def assert_line_inside(off, H: int, base: int, line: int, need_margin: bool = True, in_payload: bool = True) -> int:
    """The line, seen from a block placed at `base`, falls strictly inside some
    frame's payload: not on a frame boundary, not in a header, and (frames long
    enough, `need_margin`) not within MARGIN bytes of either end of the frame.
    `in_payload` False asks only for mid-frame: never on a frame boundary.
    Returns the frame; raises AssertionError otherwise."""
    off = np.asarray(off, np.int64)
    p = line - base
    assert 0 <= p < int(off[-1]), f"line {line:#x} is outside the block placed at {base:#x}"
    i = int(np.searchsorted(off, p, side="right")) - 1
    a, b = int(off[i]), int(off[i + 1])
    assert a < p < b, f"line {line:#x} falls on the boundary of frame {i}"
    if not in_payload:
        return i
    assert p >= a + H, f"line {line:#x} falls in the header of frame {i}"
    m = line_margin(off, H, i)
    if need_margin:
        assert m == MARGIN, f"frame {i} ({b - a} B) is too short to keep {MARGIN} B around line {line:#x}"
    assert a + m <= p <= b - m, f"line {line:#x} is within {MARGIN} B of an end of frame {i}"
    return i


def straddle_base(off, H: int, line: int, *, anchor: Optional[int] = None, tail_room: int = 1 << 20,
                  want_unaligned: Optional[bool] = None, need_margin: bool = True) -> int:
    """A base for a block so that `line` falls inside the payload of a frame
    (`anchor`, or one near the middle that leaves at most `tail_room` bytes of
    the block after the line).  `want_unaligned`: base % 16 != 0 (True), == 0
    (False) or either (None)."""
    off = np.asarray(off, np.int64)
    n, B = len(off) - 1, int(off[-1])
    target = max(B // 2, B - tail_room)
    first = int(np.searchsorted(off, target, side="right")) - 1 if anchor is None else anchor
    for i in ([anchor] if anchor is not None else list(range(first, n))):
        a, b = int(off[i]), int(off[i + 1])
        m = line_margin(off, H, i)
        if need_margin and m != MARGIN:
            continue
        lo, hi = max(a + H, a + m, a + 1), min(b - m, b - 1)
        if lo > hi:
            continue
        for p in range((lo + hi) // 2, hi + 1):
            base = line - p
            if want_unaligned is None or (base % 16 != 0) == want_unaligned:
                assert_line_inside(off, H, base, line, need_margin)
                return base
    raise AssertionError("no frame of the block can hold the line")


def translate(off, base: int) -> np.ndarray:
    """The offsets of a block copied to [base, base + B) of a larger buffer."""
    return np.asarray(off, np.int64) + np.int64(base)


def placements(off, H: int, need_margin: bool = True, anchor: Optional[int] = None):
    """[(name, base)] for the control and the two straddling placements; the
    2^31 one unaligned, and both checked."""
    b31 = straddle_base(off, H, LINE31, anchor=anchor, want_unaligned=True, need_margin=need_margin)
    b32 = straddle_base(off, H, LINE32, anchor=anchor, need_margin=need_margin)
    assert b31 % 16 or b32 % 16
    assert b32 + int(off[-1]) <= BIG_BYTES, "the block does not fit behind the 2^32 line"
    return [("control", 0), ("2^31", b31), ("2^32", b32)]


# ------------------------------------------------------------------- blocks
TEXT = ("é中😀aßЖ€" * 800).encode()


def _body(rng, L: int, kind: float) -> bytes:
    """L payload bytes: valid multi-byte text, ASCII, or ASCII with a stray high byte."""
    if kind < 0.35:
        b = TEXT[:L]
        while True:
            try:
                b.decode()
                break
            except UnicodeDecodeError:
                b = b[:-1]
        return b + b"y" * (L - len(b))
    b = bytearray(rng.randbytes(L).translate(bytes(0x20 + (c % 0x5F) for c in range(256))))
    if L and kind > 0.9:
        b[rng.randrange(L)] = rng.randint(0x80, 0xFF)
    return bytes(b)


def block_payloads(kind: str, rng) -> list:
    """The payloads of block (a) 'chars', (b) 'ragged' or (c) 'long'."""
    if kind == "chars":
        chars = ("a", "é", "€", "😀")
        pays = [chars[rng.randrange(4)].encode() for _ in range(3000)]
        for i in range(50, 3000, 97):
            pays[i] = b""
        return pays
    if kind == "ragged":
        return [_body(rng, rng.randint(0, 2944), rng.random()) for _ in range(1200)]
    if kind == "long":
        pays = [_body(rng, rng.randint(0, 16), rng.random()) for _ in range(600)]
        pays[300] = "😀".encode() * 50_000   # 200 000 B and few enough characters to stay in one transfer
        return pays
    raise ValueError(kind)


class Block(NamedTuple):
    kind: str
    H: int
    frames: list            # bytes per datagram
    buf: np.ndarray         # u8 [B]
    off: np.ndarray         # i64 [n + 1]
    csum: np.ndarray        # u16 [n]: the rudp5 sideband (each frame's checksum before any damage)
    anchor: Optional[int]   # the frame a line must fall into (block 'long'), or None
    mean: int               # the true mean frame length, the product's len_hint

    @property
    def n(self):
        return len(self.frames)


def make_block(kind: str, H: int, seed: int = 0) -> Block:
    """A block whose headers are a receiver's and a sender's stream at once:
    seq_num and SYN/FIN follow a stop-and-wait transfer of the payloads'
    characters (restarted with a new SYN before seq_num would pass 65535),
    ack_num and the ACK flag a cumulative reply stream on a grid of ACK_CHUNK.
    Among them: byte-for-byte repeats of earlier frames inside and outside
    WINDOW, frames damaged after framing, and frames shorter than the header."""
    rng = random.Random(0xB10C + 131 * seed + H + sum(map(ord, kind)))
    pays = block_payloads(kind, rng)
    n = len(pays)

    def usable_text(p):
        try:
            return len(p.decode())
        except UnicodeDecodeError:
            return None
    damaged = {i for i in range(7, n, 41)}
    short = {i for i in range(23, n, 211)}
    repeat = {}
    for i in range(30, n, 29):
        d = rng.choice((1, 2, WINDOW - 1, WINDOW, WINDOW + 1, 3 * WINDOW))
        if i - d < 0 or i in damaged or i in short or (kind == "long" and 300 in (i, i - d)):
            continue
        repeat[i] = i - d
    assert any(i - j <= WINDOW for i, j in repeat.items()) and any(i - j > WINDOW for i, j in repeat.items())
    seq, ack, flags = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    isn, sent, fresh, k = rng.randint(1, 5000), 0, True, 0
    for i, p in enumerate(pays):
        if i in repeat:
            continue
        c = usable_text(p)
        if fresh or sent + (c or 0) > 60000:
            isn, sent = rng.randint(1, 5000), 0
            flags[i] |= SYN
        seq[i] = (isn + sent) & 0xFFFF
        k += 1
        ack[i] = ACK_ISN + k * ACK_CHUNK
        flags[i] |= ACK
        good = c is not None and i not in damaged and i not in short
        if good:
            sent, fresh = sent + c, False
        elif flags[i] & SYN:
            fresh = True  # the SYN was lost: the sender opens again
    assert ACK_ISN + k * ACK_CHUNK <= 65535
    last = max(i for i in range(n) if i not in repeat and i not in damaged and i not in short
               and usable_text(pays[i]) is not None)
    flags[last] |= FIN
    buf, off, cs = codec_np.encode_varlen(seq, ack, flags, pays, H)
    frames = [bytes(buf[off[i]:off[i + 1]]) for i in range(n)]
    for i in damaged:
        fr = bytearray(frames[i])
        fr[-1] ^= 0x80
        frames[i] = bytes(fr)
    for i in short:
        frames[i] = frames[i][:rng.randint(0, H - 1)]
    for i in sorted(repeat):
        frames[i], cs[i] = frames[repeat[i]], cs[repeat[i]]
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(f) for f in frames], out=off[1:])
    buf = np.frombuffer(b"".join(frames), np.uint8).copy()
    return Block(kind, H, frames, buf, off, cs, 300 if kind == "long" else None, int(off[-1]) // n)


# ------------------------------------------------- what the library owes for a block
def decode_expect(buf, off, H: int, csum_in=None, lim: Optional[int] = None) -> dict:
    """The decode's tables, frame by frame: a frame whose pair of offsets is
    decreasing or past `lim` is rejected unread, every other one is the
    oracle's (oracle/codec_np.decode_varlen, utf8_valid; accept_ref.chars_ref)."""
    buf, off = np.asarray(buf, np.uint8), np.asarray(off, np.int64)
    n = len(off) - 1
    lim = len(buf) if lim is None else lim
    good = (off[:-1] >= 0) & (off[:-1] <= off[1:]) & (off[1:] <= lim)
    w = dict(seq=np.zeros(n, np.uint16), ack=np.zeros(n, np.uint16), flags=np.zeros(n, np.uint8),
             ok=np.full(n, OK_BAD_OFFSETS, np.uint8), csum=np.zeros(n, np.uint16), valid=np.zeros(n, np.uint8),
             chars=np.zeros(n, np.uint32))
    idx = np.flatnonzero(good)
    if len(idx):
        parts = [bytes(buf[off[i]:off[i + 1]]) for i in idx]
        sbuf = np.frombuffer(b"".join(parts) + b"\0", np.uint8)[:-1]
        soff = np.zeros(len(idx) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=soff[1:])
        ci = None if csum_in is None else np.asarray(csum_in, np.uint16)[idx]
        s, a, f, o, c = codec_np.decode_varlen(sbuf, soff, H, ci)
        w["seq"][idx], w["ack"][idx], w["flags"][idx], w["ok"][idx], w["csum"][idx] = s, a, f, o, c
        w["valid"][idx] = codec_np.utf8_valid(sbuf, soff, H)
        w["chars"][idx] = chars_ref(sbuf, soff, H)
    w["good"] = good
    w["status"] = 0 if good.all() else ST_OFFSETS
    return w


def gather_expect(buf, off, H: int, keep, good=None):
    """(payload bytes, payload_off u64 [n + 1]) of rudp_gather_payloads."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    good = np.ones(n, bool) if good is None else good
    parts = [bytes(buf[off[i] + H:off[i + 1]]) if good[i] and keep[i] and off[i + 1] - off[i] > H else b""
             for i in range(n)]
    poff = np.zeros(n + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=poff[1:])
    return np.frombuffer(b"".join(parts) + b"\0", np.uint8)[:-1], poff


def reply_expect(reply, reply_ack, usable, seq, flags, last_isn, H: int):
    """(reply_frames, reply_csum, reply_index, reply_peer) of rudp_receive."""
    n = len(reply)
    idx, peer, last = [], [], n
    for i in range(n):
        if usable[i] and flags[i] & SYN and int(seq[i]) != last_isn:
            last = i
        if reply[i]:
            idx.append(i)
            peer.append(last)
    fr = b"".join(header(0, int(reply_ack[i]), ACK, H) for i in idx)
    cs = np.array([csum_of(0, int(reply_ack[i]), ACK) for i in idx], np.uint16)
    return np.frombuffer(fr + b"\0", np.uint8)[:-1], cs, np.array(idx, np.uint32), np.array(peer, np.uint64)


def block_expect(b: Block, sideband: bool) -> dict:
    """Everything the calls of construction 1 return for the block (at any base)."""
    H, n = b.H, b.n
    w = decode_expect(b.buf, b.off, H, b.csum if sideband else None)
    w["keep_mask"] = (np.arange(n) % 5 != 3).astype(np.uint8)
    w["gather"] = gather_expect(b.buf, b.off, H, w["keep_mask"])
    rng = random.Random(n)
    perm = list(range(n))
    rng.shuffle(perm)
    K = (2 * n) // 3
    rank = np.full(n, NONE, np.uint32)
    rank[perm[:K]] = np.arange(K, dtype=np.uint32)
    w["rank"], w["K"] = rank, K
    w["ordered"] = {skip: ordered_ref(b.buf, b.off, rank, K, skip) for skip in (0, H)}
    w["dup"] = np.array(proxy_scan(b.frames, WINDOW)[0], np.uint8)
    assert w["dup"].sum() >= 3, "the block holds no repeats inside the window"
    # the receiver: decode -> usable -> characters -> in-order acceptance -> gather (keep) -> replies
    usable = (np.isin(w["ok"], (OK_GOOD, OK_UNVERIFIED)) & (w["valid"] == 1)).astype(np.uint8)
    acc = accept_ref(w["seq"], w["flags"], w["chars"], usable, (0, 0, 0), None)
    first = accept_scan_model(w["seq"], w["flags"], w["chars"], usable, (0, 0, 0), None).first_anomaly
    pay, poff = gather_expect(b.buf, b.off, H, acc.keep)
    rf, rc, ri, rp = reply_expect(acc.reply, acc.reply_ack, usable, w["seq"], w["flags"], 0xFFFFFFFF, H)
    assert acc.count > n // 4, "the block's stream is not accepted: the receive path would gather nothing"
    w["receive"] = dict(usable=usable, accept=acc.accept, keep=acc.keep, reply=acc.reply, reply_ack=acc.reply_ack,
                        state_out=np.array([acc.state[0], acc.state[1], acc.state[2], 0], np.uint64),
                        payload=pay, payload_off=poff, reply_frames=rf, reply_csum=rc, reply_index=ri, reply_peer=rp,
                        info=np.array([acc.end, acc.count, acc.msg_start, acc.characters, first, len(ri), len(pay), 0],
                                      np.uint64))
    # the windowed receiver: accept_window, then gather_ordered of its ranks
    win = window_ref(w["seq"], w["flags"], w["chars"], usable, (0, 0, 0), None, window_chars=WINDOW_CHARS)
    w["window"] = dict(res=win, message=ordered_ref(b.buf, b.off, win.rank, win.info[1], H))
    # the sender: decode -> usable (no UTF-8 needed) -> the cumulative rule
    us_a = np.isin(w["ok"], (OK_GOOD, OK_UNVERIFIED)).astype(np.uint8)
    T = int(w["ack"].max()) - ACK_ISN
    kw = dict(isn=ACK_ISN, T=T, C=ACK_CHUNK, state=fresh_state(T, ACK_CHUNK), mode=CUMULATIVE, sent=T)
    r = ack_ref(w["seq"], w["ack"], w["flags"], us_a, **kw)
    first = ack_scan_model(w["ack"], w["flags"], us_a, **kw).first_anomaly
    assert r.count > n // 4, "the block's replies are not valid: the acknowledge path would judge nothing"
    w["acknowledge"] = dict(usable=us_a, valid=r.valid, pointer=r.pointer.astype(np.uint64),
                            state_out=np.array(r.state, np.uint64),
                            info=np.array(info_ref(r, n, ACK_CHUNK, first), np.uint64), T=T,
                            final_frame=np.frombuffer(header(*r.final, ACK, H), np.uint8) if r.final else None,
                            final_csum=csum_of(*r.final, ACK) if r.final else None)
    return w


# --------------------------------------------------------- periodic batches
def periodic_rows(B: int, reach: int = LINE32) -> int:
    """R, the repeats of a block of B bytes that carry it past 2^32: ceil((reach + 2B) / B)."""
    return -(-(reach + 2 * B) // B)


def assert_lines_mid_frame(off, H: int, R: int) -> None:
    """In a block of offsets `off` repeated R times, 2^31 and 2^32 both fall
    mid-frame, never on a frame boundary.  (Not always on a payload byte: in
    fixed 6-byte frames 2^31 and 2^32 are bytes 2 and 4 of a frame whatever the
    period, since 6 divides it.)"""
    B = int(off[-1])
    assert R * B > LINE32, "the batch does not reach 2^32"
    for line in LINES:
        assert_line_inside(off, H, (line // B) * B, line, need_margin=False, in_payload=False)


def tile_offsets(off, R: int) -> np.ndarray:
    """The n*R + 1 offsets of a block repeated R times (CPU restatement)."""
    off = np.asarray(off, np.int64)
    B = off[-1]
    body = (np.arange(R, dtype=np.int64)[:, None] * B + off[None, :-1]).reshape(-1)
    return np.concatenate([body, [R * B]])


def _signed(t):
    import torch
    return t.view({torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}.get(t.dtype, t.dtype))


def compare_periodic(got, block, R: int, *, what: str, advance: int = 0, byte_scale: Optional[int] = None,
                     chunk_bytes: int = 1 << 28) -> None:
    """got (1-D tensor of R * len(block) elements) is `block` repeated R times,
    row r advanced by r * advance (offset tables).  Compared in row chunks whose
    temporaries stay under chunk_bytes * 4; on a mismatch the AssertionError names
    the first differing element, its byte offset in the array the table indexes
    (`byte_scale` bytes per element, default the element size) and the line
    that offset lies beyond."""
    import torch
    got, block = _signed(got), _signed(block)
    L = block.numel()
    assert got.numel() == R * L, (what, got.numel(), R, L)
    width = 8 if advance else got.element_size()
    rows = max(1, chunk_bytes // max(1, L * width))
    for r0 in range(0, R, rows):
        r1 = min(R, r0 + rows)
        g = got[r0 * L:r1 * L].view(r1 - r0, L)
        want = block[None, :]
        if advance:
            want = want + (torch.arange(r0, r1, dtype=torch.int64, device=got.device) * advance)[:, None]
        ne = g != want
        if bool(ne.any()):
            at = r0 * L + int(torch.argmax(ne.reshape(-1).to(torch.uint8)))
            scale = got.element_size() if byte_scale is None else byte_scale
            byte = int(got[at]) if advance else at * scale
            raise AssertionError(f"{what}: first difference at element {at} (row {at // L}, column {at % L}), "
                                 f"byte offset {byte}, {beyond(byte)}: got {int(got[at])}, want "
                                 f"{int(block[at % L]) + (at // L) * advance}")
        del g, ne, want


def periodic_message(P: int = 1021):
    """One period of a message: ASCII with one 2-, one 3- and one 4-byte
    character, P bytes, starting on a lead byte.  Returns (bytes, starts): the
    byte at which each of its characters starts."""
    text = "".join(chr(0x41 + i % 26) for i in range(P))
    text = text[:200] + "é" + text[200:500] + "€" + text[500:800] + "😀" + text[800:]
    b = text.encode()
    while len(b) > P:
        text = text[:-1]
        b = text.encode()
    assert len(b) == P
    a =np.frombuffer(b, np.uint8)
    starts = np.flatnonzero((a & 0xC0) != 0x80).astype(np.int64)
    assert starts[0] == 0 and len(starts) == P - 6
    return b, starts


class ClosedForm(NamedTuple):
    packets: int
    characters: int
    seq: np.ndarray          # u16
    flags: np.ndarray        # u8
    len: np.ndarray          # u32
    payload_off: np.ndarray  # u64 [packets + 1]


def segment_closed_form(P: int, starts, R: int, chunk: int, isn: int) -> ClosedForm:
    """rudp_segment_utf8's tables for a period of P bytes (characters at
    `starts`) repeated R times: character q starts at byte (q // c) * P +
    starts[q % c], packet k at character k * chunk."""
    starts = np.asarray(starts, np.int64)
    c = len(starts)
    characters = R * c
    packets = max(1, -(-characters // chunk))
    q = np.arange(packets, dtype=np.int64) * chunk
    off = np.concatenate([(q // c) * P + starts[q % c], [R * P]]).astype(np.int64)
    flags = np.zeros(packets, np.uint8)
    flags[0] |= SYN
    flags[-1] |= FIN
    return ClosedForm(packets, characters, ((isn + q) & 0xFFFF).astype(np.uint16), flags,
                      np.diff(off).astype(np.uint32), off.astype(np.uint64))
