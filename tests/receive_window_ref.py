"""CPU reference for rudp_receive_window: the call restated from the pieces the
other references already hold -- the per-source offset rule, the decode (the
oracle codec), ``chars_ref``, ``window_ref``, ``ordered_ref`` twice and the
reply datagrams of ``Packet(0, ack, ACK).to_byte()``.

Item i < n_carried is carried frame i, judged against the carried buffer's
size; the others are the new frames, judged against theirs.  A rejected item
is decoded as nothing: ok = 4, every other table 0.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from accept_ref import chars_ref
from oracle import codec_np
from window_ref import NO_ISN, NONE, ST_OFFSETS, ST_PAYLOAD_CAP, SYN, ordered_ref, window_ref

ST_CARRY_CAP = 128
OK_BAD_OFFSETS = 4


def _fold_csum(ack):
    s = ack.astype(np.uint32) + 0x4000
    return (~((s & 0xFFFF) + (s >> 16)) & 0xFFFF).astype(np.uint16)


def reply_frames_ref(acks, H):
    """The header-only frames of seq 0, ack, flags ACK, and their checksums."""
    acks = np.asarray(acks, np.uint16)
    lit = np.zeros((len(acks), H), np.uint8)
    lit[:, 2], lit[:, 3], lit[:, 4] = acks >> 8, acks & 0xFF, 0x40
    c = _fold_csum(acks)
    if H == 7:
        lit[:, 5], lit[:, 6] = c >> 8, c & 0xFF
    return lit.reshape(-1), c


def receive_window_ref(carried, carried_off, frames, frame_off, H, *, window_chars, carried_csum=None, csum=None,
                       state=(0, 0, 0), last_isn: Optional[int] = None, payload_cap=None, carry_cap=None,
                       rule=window_ref):
    """Every output of the call as numpy arrays / ints in a dict.  ``carried_off``
    None or of one entry: no carried frames.  ``rule``: ``window_ref`` or
    ``chunk_model`` (they differ in ``info[4]`` alone)."""
    srcs = (np.asarray(carried, np.uint8), np.asarray(frames, np.uint8))
    offs = (np.zeros(1, np.int64) if carried_off is None else np.asarray(carried_off).astype(np.uint64),
            np.asarray(frame_off).astype(np.uint64))
    nc, nn = len(offs[0]) - 1, len(offs[1]) - 1
    n = nc + nn
    side = csum is not None if nc == 0 else carried_csum is not None
    sums = (carried_csum, csum)
    # the per-source offset rule, and the good items' bytes back to back
    good = np.zeros(n, bool)
    parts, cs_in = [], np.zeros(n, np.uint16)
    for i in range(n):
        s, k = (0, i) if i < nc else (1, i - nc)
        a, b = int(offs[s][k]), int(offs[s][k + 1])
        good[i] = a <= b <= len(srcs[s])
        parts.append(srcs[s][a:b].tobytes() if good[i] else b"")
        if side:
            cs_in[i] = sums[s][k]
    joined = np.frombuffer(b"".join(parts), np.uint8)
    joff = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=joff[1:])
    seq, ack, flags, ok, cs = (a.copy() for a in codec_np.decode_varlen(joined, joff, H, cs_in if side else None))
    valid = codec_np.utf8_valid(joined, joff, H)
    chars = chars_ref(joined, joff, H)
    bad = ~good
    seq[bad], ack[bad], flags[bad], ok[bad], cs[bad], valid[bad], chars[bad] = 0, 0, 0, OK_BAD_OFFSETS, 0, 0, 0
    usable = (((ok == 1) | (ok == 3)) & (valid == 1)).astype(np.uint8)
    w = rule(seq, flags, chars, usable, state, last_isn, window_chars=window_chars, n_carried=nc)
    K, P = w.info[1], w.info[5]
    msg, moff, msrc, mst = ordered_ref(joined, joff, w.rank, K, H, payload_cap)
    car, coff, csrc, cst = ordered_ref(joined, joff, w.carry_rank, P, 0, carry_cap)
    last = NO_ISN if last_isn is None else int(last_isn)
    idx, peer, reset = [], [], n
    for i in range(nc, n):
        if usable[i] and flags[i] & SYN and int(seq[i]) != last:
            reset = i
        if w.reply[i]:
            idx.append(i)
            peer.append(reset)
    rframes, rcsum = reply_frames_ref(w.reply_ack[idx], H)
    status = (ST_OFFSETS if bad.any() else 0) | (mst & ST_PAYLOAD_CAP) | (ST_CARRY_CAP if cst & ST_PAYLOAD_CAP else 0)
    live = 1 if w.state[2] else 0
    return {
        "seq": seq, "ack": ack, "flags": flags, "ok": ok, "csum_out": cs, "valid": valid, "usable": usable,
        "chars": chars, "accept": w.accept, "rank": w.rank, "carry_rank": w.carry_rank, "reply": w.reply,
        "reply_ack": w.reply_ack, "state": [w.state[0], w.state[1], live, 0],
        "info": list(w.info) + [len(idx), int(moff[K]), int(coff[P]), 0],
        "payload": msg if not mst & ST_PAYLOAD_CAP else np.zeros(0, np.uint8), "payload_off": moff.astype(np.uint64),
        "payload_src": np.where(msrc < 0, NONE, msrc).astype(np.uint32),
        "carry_frames": car if not cst & ST_PAYLOAD_CAP else np.zeros(0, np.uint8), "carry_off": coff.astype(np.uint64),
        "carry_csum": cs_in[csrc] if side else None,
        "reply_frames": rframes, "reply_csum": rcsum, "reply_index": np.array(idx, np.uint32),
        "reply_peer": np.array(peer, np.uint64), "status": status, "K": K, "P": P, "R": len(idx),
    }
