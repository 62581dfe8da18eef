"""CPU reference for rudp_receive_flows, from the frames: the numpy codec's
decode and Python's strict UTF-8 (oracle/codec_np.py), the usable mask,
``chars_ref``, ``flows_ref`` (tests/flows_ref.py), the ordered gather as a loop
over the ranks, and the reply and closing datagrams through
``codec_np.encode_varlen`` (include/rudp.h states the contract).

``build_frames`` turns a ``flows_ref.make_batch`` mix into datagrams: datagram i
carries ``chars[i]`` characters of mixed widths, and ``usable[i] == 0`` becomes
damage on the wire."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from accept_ref import ACK, FIN, chars_ref
from flows_ref import FlowsRef, flows_ref, make_batch
from oracle import codec_np

OK_BAD_CSUM, OK_GOOD, OK_SHORT, OK_UNVERIFIED, OK_BAD_OFFSETS = 0, 1, 2, 3, 4
ST_OFFSETS, ST_PAYLOAD_CAP = 8, 16
FUSED_BYTES, FUSED_MEAN = 32768, 133  # the fused form's limits (csrc/receive_flows.hip)
N_FLOWS = 5000  # rows of the GPU tests' table

# One character of every UTF-8 width; a payload draws widths with mean 2.
ALPHABET = {1: "a", 2: "é", 3: "語", 4: "😀"}
WIDTHS = (1, 1, 1, 2, 3, 4)


class RecvFlowsRef(NamedTuple):
    seq: np.ndarray          # u16 [n]
    ack: np.ndarray          # u16 [n]
    flags: np.ndarray        # u8 [n]
    ok: np.ndarray           # u8 [n]
    csum: np.ndarray         # u16 [n]
    valid: np.ndarray        # u8 [n]
    usable: np.ndarray       # u8 [n]
    chars: np.ndarray        # u32 [n]
    flows: FlowsRef
    payload: bytes           # every active flow's piece, back to back (whatever payload_cap is)
    payload_off: np.ndarray  # u64 [K + 1]
    payload_src: np.ndarray  # u32 [K]
    reply_frames: bytes
    reply_csum: np.ndarray   # u16 [R]
    reply_index: np.ndarray  # u32 [R]
    fin_frames: bytes
    fin_csum: np.ndarray     # u16 [E]
    fin_flow: np.ndarray     # u32 [E]
    info: list               # [12]; [5] (a diagnostic) is None
    status: int


def decode_ref(frames, frame_off, H: int, csum_in=None):
    """(seq, ack, flags, ok, csum, valid, usable, chars) of packed frames, a
    frame whose offsets are decreasing or past the buffer rejected whole."""
    frames = np.asarray(frames, np.uint8)
    off = [int(v) for v in frame_off]
    n = len(off) - 1
    seq, ack, csum = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    flags, ok, valid = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        a, b = off[i], off[i + 1]
        if not 0 <= a <= b <= len(frames):
            ok[i] = OK_BAD_OFFSETS
            continue
        ci = None if csum_in is None else np.asarray(csum_in)[i:i + 1]
        s, k, f, o, c, _ = codec_np.decode(frames[a:b].reshape(1, -1), H, ci)
        seq[i], ack[i], flags[i], ok[i], csum[i] = s[0], k[0], f[0], o[0], c[0]
        try:
            bytes(frames[a + H:b] if b - a > H else b"").decode()
            valid[i] = 1
        except UnicodeDecodeError:
            valid[i] = 0
    usable = (((ok == OK_GOOD) | (ok == OK_UNVERIFIED)) & (valid == 1)).astype(np.uint8)
    safe = [o if 0 <= o <= len(frames) else len(frames) + 1 for o in off]  # (chars_ref takes non-negative offsets)
    return seq, ack, flags, ok, csum, valid, usable, chars_ref(frames, safe, H)


def header_frames(acks, flags: int, H: int):
    """Header-only frames (seq 0) back to back, and their checksums."""
    m = len(acks)
    fr, _, cs = codec_np.encode_varlen(np.zeros(m, np.uint16), np.asarray(acks, np.uint16),
                                       np.full(m, flags, np.uint8), [b""] * m, H)
    return fr.tobytes(), cs


def receive_flows_ref(frames, frame_off, flow, states, H: int, csum_in=None,
                      payload_cap: Optional[int] = None) -> RecvFlowsRef:
    frames = np.asarray(frames, np.uint8)
    off = [int(v) for v in frame_off]
    n = len(off) - 1
    seq, ack, flags, ok, csum, valid, usable, chars = decode_ref(frames, off, H, csum_in)
    f = flows_ref(seq, flags, chars, usable, flow, states)
    K = f.info[1]
    src = np.zeros(K, np.uint32)
    for i in np.flatnonzero(f.rank != 0xFFFFFFFF):
        src[f.rank[i]] = i
    pieces = [bytes(frames[off[i] + H:off[i + 1]]) for i in src.tolist()]
    poff = np.zeros(K + 1, np.uint64)
    np.cumsum([len(p) for p in pieces], out=poff[1:])
    idx = np.flatnonzero(f.reply).astype(np.uint32)
    reply_frames, reply_csum = header_frames(f.reply_ack[idx], ACK, H)
    ended = [a for a, row in enumerate(f.flow_info.tolist()) if row[1] < n]
    fin_frames, fin_csum = header_frames([(int(f.flow_info[a][5]) + int(f.flow_info[a][4])) & 0xFFFF for a in ended],
                                         FIN | ACK, H)
    total = int(poff[K])
    cap = len(frames) if payload_cap is None else payload_cap
    status = (ST_OFFSETS if (ok == OK_BAD_OFFSETS).any() else 0) | f.status | (ST_PAYLOAD_CAP if total > cap else 0)
    info = f.info + [None, 0, 0, total, 0, 0, 0]
    return RecvFlowsRef(seq, ack, flags, ok, csum, valid, usable, chars, f, b"".join(pieces), poff, src,
                        reply_frames, reply_csum, idx, fin_frames, fin_csum, np.array(ended, np.uint32), info, status)


def text_of(rng, chars: int) -> str:
    return "".join(ALPHABET[rng.choice(WIDTHS)] for _ in range(chars))


def build_frames(rng, seq, flags, chars, usable, H: int):
    """The datagrams of a ``make_batch`` mix: (frames u8, frame_off i64 [n + 1],
    csum_in u16 [n] or None for H == 7, texts).  Datagram i carries ``chars[i]``
    characters; ``usable[i] == 0`` is realised by damage, in rotation: a wrong
    checksum (in-band for H == 7, in the sideband for H == 5), a payload byte
    that is not UTF-8, a frame cut below the header.  ``texts[i]`` is the text
    of an undamaged datagram, else None.  The caller takes chars and usable
    from the bytes again (``decode_ref``)."""
    n = len(seq)
    out, off, side, texts, turn = bytearray(), [0], [], [], 0
    for i in range(n):
        text = text_of(rng, int(chars[i]))
        body = bytearray(text.encode())
        damage = None
        if not usable[i]:
            damage = turn % 3
            turn += 1
        if damage == 1:
            if body:
                body[0] = 0xFF
            else:
                body = bytearray(b"\xff")
        fr, _, cs = codec_np.encode_varlen(seq[i:i + 1], np.zeros(1, np.uint16), flags[i:i + 1], [bytes(body)], H)
        fr, c = bytearray(fr.tobytes()), int(cs[0])
        if damage == 0:
            if H == 7:
                fr[6] ^= 0x01
            else:
                c ^= 0x0100
        elif damage == 2:
            del fr[rng.randrange(H):]
        out += fr
        off.append(len(out))
        side.append(c)
        texts.append(text if damage is None else None)
    return (np.frombuffer(bytes(out), np.uint8).copy(), np.array(off, np.int64),
            np.array(side, np.uint16) if H == 5 else None, texts)


def mix_case(rng, n, n_active, H, n_flows=N_FLOWS):
    """The GPU tests' case: ``make_batch``'s mix as datagrams, and a table
    seeded as tests/test_gpu_flows.py seeds it.  Returns (frames, frame_off,
    csum_in or None, flow, table)."""
    from test_gpu_flows import seed_table
    seq, flags, chars, usable, flow = make_batch(rng, n, n_active, n_flows)
    frames, off, side, _ = build_frames(rng, seq, flags, chars, usable, H)
    table = np.zeros((n_flows, 4), np.uint64)
    seed_table(rng, table, flow, seq)
    return frames, off, side, flow, table


def fused_eligible(frames_bytes: int, n: int) -> bool:
    """Whether the library's default takes the one-launch form."""
    return n == 0 or (n <= 1024 and frames_bytes <= FUSED_BYTES and frames_bytes <= FUSED_MEAN * n)


__all__ = ["RecvFlowsRef", "build_frames", "decode_ref", "fused_eligible", "header_frames", "mix_case",
           "receive_flows_ref",
           "text_of", "FUSED_BYTES", "FUSED_MEAN", "N_FLOWS", "ST_OFFSETS", "ST_PAYLOAD_CAP"]
