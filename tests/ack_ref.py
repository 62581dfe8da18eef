"""CPU references for rudp_ack_progress / rudp_acknowledge.

``ack_ref``: the sender's rule (include/rudp.h; wait_ack, send_data and send_ack
of utils/reliableUDP.py:43-93) as a plain loop over the replies, in both modes.
``scan_model``: the device's one-scan form in numpy -- the characters
acknowledged before every reply guessed as a prefix maximum -- with the index
where it stops being exact (``first_anomaly``).
``clean_replies`` / ``adversarial_replies``: reply streams.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

SYN, ACK, FIN = 0x80, 0x40, 0x20
EXACT, CUMULATIVE = "exact", "cumulative"


def fresh_state(T: int, C: int):
    """(p, L, last, done) when send() starts."""
    L = min(C, T)
    return 0, L, int(L == T), 0


class RefResult(NamedTuple):
    valid: np.ndarray       # u8 [n]
    pointer: np.ndarray     # i64 [n]: p after reply i (0 past the end)
    state: tuple            # (p, L, last, done)
    end: int
    count: int
    newly: int
    done: int
    final: Optional[tuple]  # (seq, ack) of the closing datagram, or None


def is_valid(ack, usable, isn, T, C, p, L, mode=EXACT, sent=None):
    if not usable:
        return False
    expected = isn + p + L
    if mode == EXACT:
        return ack == expected
    sent = T if sent is None else sent
    d = ack - isn
    return expected <= ack <= isn + sent and (d % C == 0 or d == T)


def ack_ref(seq, ack, flags, usable=None, *, isn, T, C=1, state=None, mode=EXACT, sent=None) -> RefResult:
    n = len(ack)
    p, L, last, done = (int(v) for v in (fresh_state(T, C) if state is None else state))
    last, done = int(bool(last)), int(bool(done))
    p0 = p
    valid = np.zeros(n, np.uint8)
    pointer = np.zeros(n, np.int64)
    end, final = n, None
    if not done:
        for i in range(n):
            a, f = int(ack[i]), int(flags[i])
            if is_valid(a, True if usable is None else bool(usable[i]), isn, T, C, p, L, mode, sent):
                valid[i] = 1
                if f & ACK:
                    p = a - isn
                if f & FIN:
                    end, done = i, 1
                    final = ((isn + p) & 0xFFFF, (int(seq[i]) + 1) & 0xFFFF)
                elif last:
                    L = 0
                else:
                    L = min(C, T - p)
                    last = int(p + L == T)
            pointer[i] = p
            if done:
                break
    return RefResult(valid, pointer, (p, L, last, done), end, int(valid.sum()), p - p0, done, final)


def info_ref(r: RefResult, n: int, C: int, first_anomaly: int):
    """d_info as the device writes it."""
    p = r.state[0]
    return [r.end, r.count, r.newly % (1 << 64), p, first_anomaly, -(-p // C), r.done, 0]


def canonical(state, T, C):
    p, L, last, _ = state
    if p > T or (p % C and p != T):
        return False
    Lc = min(C, T - p)
    return L == Lc and int(bool(last)) == int(p + Lc == T)


class ScanResult(NamedTuple):
    valid: np.ndarray        # u8 [n]: valid under the guess (exact before first_anomaly)
    guess: np.ndarray        # i64 [n]: the guessed p before every reply
    end_guess: int           # first valid FIN under the guess, n if none
    first_anomaly: int       # n if the guess is exact up to end_guess


def scan_model(ack, flags, usable=None, *, isn, T, C=1, state=None, mode=EXACT, sent=None) -> ScanResult:
    n = len(ack)
    state = fresh_state(T, C) if state is None else tuple(int(v) for v in state)
    ack = np.asarray(ack, np.int64)
    flags = np.asarray(flags, np.int64)
    us = np.ones(n, bool) if usable is None else np.asarray(usable).astype(bool)
    sent = T if sent is None else sent
    d = ack - isn
    grid = (d % C == 0) | (d == T)
    lim = sent if mode == CUMULATIVE else T
    cand = us & ((flags & ACK) != 0) & (d >= 0) & (d <= lim) & grid
    value = np.where(cand, d, 0)
    guess = np.maximum(state[0], np.concatenate(([0], np.maximum.accumulate(value)[:-1]))) if n else value
    Lc = np.minimum(C, np.maximum(T - guess, 0))
    if mode == EXACT:
        valid = us & (d == guess + Lc)
        anomaly = (cand & (d > guess + Lc)) | (valid & ((flags & ACK) == 0))
    else:
        valid = us & (d >= guess + Lc) & (d <= sent) & grid
        anomaly = valid & ((flags & ACK) == 0)
    idx = np.arange(n)
    fin = valid & ((flags & FIN) != 0)
    end_guess = int(idx[fin][0]) if fin.any() else n
    first = int(idx[anomaly][0]) if anomaly.any() else n
    if not canonical(state, T, C):
        first = 0 if n else n
    elif first >= end_guess:
        first = n
    return ScanResult(valid.astype(np.uint8), guess, end_guess, first)


# ------------------------------------------------------------------ fixtures
def golden_cases():
    """tests/golden/ack.json (written by make_ack_golden.py from the reference)."""
    import json
    from pathlib import Path
    cases = json.loads((Path(__file__).resolve().parent / "golden" / "ack.json").read_text(encoding="utf-8"))["cases"]
    for c in cases:  # one hex string per reply, and (index, hex) per datagram sent
        c["replies"] = [c["replies"][k:k + 10] for k in range(0, len(c["replies"]), 10)]
        after = [first + k for first, count in c.pop("sent_after") for k in range(count)]
        assert len(after) == len(c["sent"])
        c["sent"] = [list(e) for e in zip(after, c["sent"])]
    return cases


def header(seq, ack, flags, H=5, payload=b""):
    """One datagram as Packet().to_byte() frames it; layout 7 with the RFC 1071
    checksum (the five header bytes and the payload as big-endian words, an odd
    tail padded) in-band."""
    h = bytes([seq >> 8, seq & 0xFF, ack >> 8, ack & 0xFF, flags])
    if H == 5:
        return h + payload
    return h + csum_of(seq, ack, flags, payload).to_bytes(2, "big") + payload


def csum_of(seq, ack, flags, payload=b""):
    body = bytes([seq >> 8, seq & 0xFF, ack >> 8, ack & 0xFF, flags]) + payload  # (the payload starts on an odd byte)
    body += b"\0" if len(body) & 1 else b""
    s = sum(int.from_bytes(body[i:i + 2], "big") for i in range(0, len(body), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def pack_frames(frames):
    """Datagrams back to back: (u8 buffer, int64 [n + 1] offsets)."""
    off = np.zeros(len(frames) + 1, np.int64)
    np.cumsum([len(f) for f in frames], out=off[1:])
    return np.frombuffer(b"".join(frames), np.uint8).copy(), off


def parse_rudp5(frames):
    seq = np.array([int.from_bytes(f[0:2], "big") for f in frames], np.uint16)
    ack = np.array([int.from_bytes(f[2:4], "big") for f in frames], np.uint16)
    flags = np.array([f[4] for f in frames], np.uint8)
    return seq, ack, flags


# ------------------------------------------------------------------- streams
def clean_replies(rng, n, *, isn, T, C=1, W=1, state=None, fin=True, p_repeat=0.3, p_unusable=0.05):
    """n replies a receiver of this protocol sends to a sender that keeps W frames
    in flight: one cumulative ack per datagram that arrives, so the ack of the
    next in-order frame, or a duplicate of the ack before it (a retransmitted
    frame is answered again: after a timeout up to W of them in a row), some
    copies unusable (damaged in flight); after the last frame the receiver's
    FIN|ACK (``fin``), repeated while it waits for the sender's closing ACK.
    The receiver goes on to the next frame only after a usable copy of its ack
    has left (the sender's retransmission brings the duplicate).  Returns seq
    (u16, 0 as the receiver sends it), ack (u16), flags (u8), usable (u8)."""
    got = int((fresh_state(T, C) if state is None else state)[0])  # characters the receiver holds
    seq = np.zeros(n, np.uint16)
    ack = np.zeros(n, np.uint16)
    flags = np.full(n, ACK, np.uint8)
    usable = np.ones(n, np.uint8)
    delivered, sent_fin, dups = True, False, 0
    for i in range(n):
        if i and dups == 0 and rng.random() < p_repeat:
            dups = rng.randint(1, W)
        if i and (not delivered or dups):
            ack[i], flags[i] = ack[i - 1], flags[i - 1]
            dups = max(dups - 1, 0)
        elif got < T:
            got = min(got + C, T)
            ack[i] = (isn + got) & 0xFFFF
            delivered = False
        else:
            ack[i] = (isn + got) & 0xFFFF
            if fin and (sent_fin or rng.random() < 0.5):
                flags[i] |= FIN
                sent_fin = True
        usable[i] = rng.random() >= p_unusable
        delivered = delivered or bool(usable[i])
    return seq, ack, flags, usable


def adversarial_replies(rng, n, *, isn, T, C=1, span=None):
    """Random ack_num in a band around the transfer, on and off the chunk grid,
    random flags and usable bits: acks from the past and the future, missing ACK
    flags, stray FINs."""
    span = span if span is not None else min(T + 2 * C, 6 * C + 3)
    lo = rng.choice((0, max(0, T - span)))
    seq = np.array([rng.choice((0, 7, 65535)) for _ in range(n)], np.uint16)
    ack = np.array([(isn + lo + rng.randint(0, span)) & 0xFFFF for _ in range(n)], np.uint16)
    flags = np.array([(ACK if rng.random() < 0.85 else 0) | (FIN if rng.random() < 0.03 else 0)
                      | (SYN if rng.random() < 0.02 else 0) for _ in range(n)], np.uint8)
    usable = np.array([rng.random() > 0.1 for _ in range(n)], np.uint8)
    return seq, ack, flags, usable
