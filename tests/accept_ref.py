"""CPU references for rudp_payload_chars / rudp_accept_inorder.

``accept_ref``: the receiver's rule (include/rudp.h; receive_data and send_ack of
utils/reliableUDP.py:116-146) as a plain loop over the frames.
``chars_ref``: lead bytes per payload, in numpy.
``scan_model``: the device's one-scan form in numpy -- the state before every
frame guessed as a segmented prefix maximum -- with the index where it stops
being exact (``first_anomaly``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

SYN, ACK, FIN = 0x80, 0x40, 0x20
NO_ISN = 0xFFFFFFFF


class RefResult(NamedTuple):
    accept: np.ndarray      # u8 [n]
    keep: np.ndarray        # u8 [n]
    reply: np.ndarray       # u8 [n]
    reply_ack: np.ndarray   # u16 [n]
    state: tuple            # (expect, isn, live)
    end: int
    count: int
    msg_start: int
    characters: int


def accept_ref(seq, flags, chars, usable=None, state=(0, 0, 0), last_isn: Optional[int] = None) -> RefResult:
    n = len(seq)
    expect, isn, live = int(state[0]), int(state[1]), 1 if state[2] else 0
    last = NO_ISN if last_isn is None else int(last_isn)
    accept = np.zeros(n, np.uint8)
    reply = np.zeros(n, np.uint8)
    ack = np.zeros(n, np.uint16)
    end, msg_start = n, n
    for i in range(n):
        if usable is not None and not usable[i]:
            continue
        s, f, c = int(seq[i]), int(flags[i]), int(chars[i])
        if f & SYN:
            if s != last:
                isn, expect, live, msg_start = s, s + c, 1, i
                accept[i] = 1
        elif live and s == expect:
            expect += c
            accept[i] = 1
        if live:
            reply[i] = 1
            ack[i] = expect & 0xFFFF
        if accept[i] and f & FIN:
            end = i
            break
    idx = np.arange(n)
    keep = (accept.astype(bool) & ((idx >= msg_start) if msg_start < n else True) & (idx <= end)).astype(np.uint8)
    return RefResult(accept, keep, reply, ack, (expect, isn, live), end, int(accept.sum()), msg_start,
                     expect - isn if live else 0)


def chars_ref(frames: np.ndarray, frame_off, H: int) -> np.ndarray:
    """Lead bytes ((b & 0xC0) != 0x80) of frame i from byte H on; 0 for a frame
    whose offsets are decreasing or past the buffer."""
    frames = np.asarray(frames, np.uint8)
    lead = np.concatenate(([0], np.cumsum((frames & 0xC0) != 0x80, dtype=np.int64)))
    out = np.zeros(len(frame_off) - 1, np.uint32)
    for i in range(len(out)):
        a, b = int(frame_off[i]), int(frame_off[i + 1])
        if a <= b <= len(frames) and b - a > H:
            out[i] = lead[b] - lead[a + H]
    return out


class ScanResult(NamedTuple):
    accept: np.ndarray       # u8 [n]: accepted under the guess (exact before first_anomaly)
    guess: np.ndarray        # i64 [n]: the guessed expect before every frame
    live: np.ndarray         # bool [n]: live before every frame (exact everywhere)
    end_guess: int           # first accepted FIN under the guess, n if none
    first_anomaly: int       # n if the guess is exact up to end_guess


def scan_model(seq, flags, chars, usable=None, state=(0, 0, 0), last_isn: Optional[int] = None) -> ScanResult:
    n = len(seq)
    seq = np.asarray(seq, np.int64)
    flags = np.asarray(flags, np.int64)
    chars = np.asarray(chars, np.int64)
    us = np.ones(n, bool) if usable is None else np.asarray(usable).astype(bool)
    last = NO_ISN if last_isn is None else int(last_isn)
    syn = (flags & SYN) != 0
    reset = us & syn & (seq != last)
    data = us & ~syn
    idx = np.arange(n)
    value = seq + chars
    # the segmented exclusive prefix maximum, frame by frame (clarity over speed):
    # a reset restarts the segment with its own seq + c
    guess = np.zeros(n, np.int64)
    run = int(state[0])
    for i in range(n):
        guess[i] = run
        if reset[i]:
            run = int(value[i])
        elif data[i]:
            run = max(run, int(value[i]))
    seg_excl = np.cumsum(reset) - reset  # resets before frame i
    live = (seg_excl > 0) | bool(state[2])
    accept = reset | (data & live & (seq == guess))
    anomaly = data & live & (seq != guess) & (seq + chars > guess)
    fin = accept & ((flags & FIN) != 0)
    end_guess = int(idx[fin][0]) if fin.any() else n
    first = int(idx[anomaly][0]) if anomaly.any() else n
    if first > end_guess:
        first = n
    return ScanResult(accept.astype(np.uint8), guess, live, end_guess, first)


# ------------------------------------------------------------------ fixtures
def golden_cases():
    """tests/golden/accept.json (written by make_accept_golden.py from the reference)."""
    import json
    from pathlib import Path
    return json.loads((Path(__file__).resolve().parent / "golden" / "accept.json").read_text(encoding="utf-8"))["cases"]


def parse_rudp5(frames):
    """seq, flags (numpy) and the payload bytes of reference datagrams (5-byte header)."""
    seq = np.array([int.from_bytes(f[0:2], "big") for f in frames], np.uint16)
    flags = np.array([f[4] for f in frames], np.uint8)
    return seq, flags, [f[5:] for f in frames]


def pack_frames(frames):
    """Datagrams back to back: (u8 buffer, int64 [n + 1] offsets)."""
    off = np.zeros(len(frames) + 1, np.int64)
    np.cumsum([len(f) for f in frames], out=off[1:])
    return np.frombuffer(b"".join(frames), np.uint8).copy(), off


# ------------------------------------------------------------------- streams
def clean_stream(rng, n, *, resets=(), fin_at=None, max_chars=1, p_repeat=0.3, p_unusable=0.05, p_reset=0.002,
                 high_isn=0.05):
    """n frames a stop-and-wait sender (or several, one after another: a transfer
    abandoned for a new SYN) leaves at the receiver: every frame is the next
    in-order one or a retransmission of the one before, some copies unusable
    (damaged in flight), seq_num mod 2^16 as the sender's header keeps it.
    The sender goes on only after a usable copy of its frame has arrived.
    ``resets``: indices that start a new transfer (index 0 always does);
    ``fin_at``: the index of a usable frame with FIN (None: no FIN), a new
    in-order one unless the frame before it still waits for a usable copy.
    Returns seq (u16), flags (u8), chars (u32), usable (u8)."""
    seq = np.zeros(n, np.uint16)
    flags = np.zeros(n, np.uint8)
    chars = np.zeros(n, np.uint32)
    usable = np.ones(n, np.uint8)
    resets = set(resets) | {0}
    isn = sent = 0
    delivered = True  # a usable copy of the outstanding frame has arrived (its ACK lets the sender go on)
    for i in range(n):
        if i in resets or (i != fin_at and delivered and rng.random() < p_reset):
            isn = rng.randint(65000, 65535) if rng.random() < high_isn else rng.randint(1, 5000)
            c = rng.randint(1, max_chars)
            seq[i], flags[i], chars[i] = isn, SYN, c
            sent, delivered = c, False
        elif i and (not delivered or rng.random() < p_repeat) and (i != fin_at or not delivered):
            seq[i], flags[i], chars[i] = seq[i - 1], flags[i - 1] & (0xFF ^ FIN), chars[i - 1]
        else:
            c = rng.randint(1, max_chars)
            seq[i], flags[i], chars[i] = (isn + sent) & 0xFFFF, 0, c
            sent, delivered = sent + c, False
        if i == fin_at:
            flags[i] |= FIN
        elif rng.random() < p_unusable:
            usable[i] = 0
        delivered = delivered or bool(usable[i])
    return seq, flags, chars, usable


def adversarial_stream(rng, n, *, span=12, p_syn=0.08, p_fin=0.01, max_chars=3):
    """Random seq_num in a narrow band, random flags, characters 0..max_chars and
    usable bits: frames from the past and the future, repeated and competing SYNs."""
    base = rng.choice((0, 100, 65530))
    seq = np.array([(base + rng.randint(0, span)) & 0xFFFF for _ in range(n)], np.uint16)
    flags = np.array([(SYN if rng.random() < p_syn else 0) | (FIN if rng.random() < p_fin else 0)
                      | (ACK if rng.random() < 0.1 else 0) for _ in range(n)], np.uint8)
    chars = np.array([rng.randint(0, max_chars) for _ in range(n)], np.uint32)
    usable = np.array([rng.random() > 0.1 for _ in range(n)], np.uint8)
    return seq, flags, chars, usable
