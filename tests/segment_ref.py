"""numpy restatement of rudp_segment_utf8 (include/rudp.h): a cumulative sum of
the lead-byte mask and one searchsorted.  Shared by the CPU and GPU tests."""
import json
from typing import NamedTuple, Optional

import numpy as np

from conftest import GOLDEN

ST_LEN, ST_PACKETS_CAP = 1, 32
SYN, FIN = 0x80, 0x20


class Segments(NamedTuple):
    packets: int
    characters: int
    seq: np.ndarray          # u16 [packets]
    ack: np.ndarray          # u16 [packets]
    flags: np.ndarray        # u8 [packets]
    len: np.ndarray          # i64 [packets]
    payload_off: np.ndarray  # i64 [packets + 1]
    status: int


def segment_ref(msg, chunk: int, isn: int, max_packets: Optional[int] = None) -> Segments:
    b = np.frombuffer(bytes(msg), np.uint8) if not isinstance(msg, np.ndarray) else msg
    lead = (b & 0xC0) != 0x80
    upto = np.cumsum(lead, dtype=np.int64)      # lead bytes in b[:i + 1]
    characters = int(upto[-1]) if len(b) else 0
    packets = max(1, -(-characters // chunk))
    k = np.arange(packets, dtype=np.int64)
    # packet k >= 1 starts at the lead byte of character k * chunk: the first byte
    # through which k * chunk + 1 lead bytes were seen; packet 0 starts at byte 0
    starts = np.searchsorted(upto, k[1:] * chunk + 1, side="left")
    off = np.concatenate([[0], starts, [len(b)]]).astype(np.int64)
    lens = np.diff(off)
    flags = np.zeros(packets, np.uint8)
    flags[0] |= SYN
    flags[-1] |= FIN
    status = (ST_LEN if (lens > 65535).any() else 0) | \
        (ST_PACKETS_CAP if max_packets is not None and packets > max_packets else 0)
    return Segments(packets, characters, ((isn + k * chunk) & 0xFFFF).astype(np.uint16),
                    np.zeros(packets, np.uint16), flags, lens, off, status)


def frames_rudp5(msg: bytes, seg: Segments):
    """The 5-byte-header frames of the segments: seq, ack big-endian, the flags byte, the slice."""
    out = []
    for k in range(seg.packets):
        head = int(seg.seq[k]).to_bytes(2, "big") + int(seg.ack[k]).to_bytes(2, "big") + bytes([int(seg.flags[k])])
        out.append(head + msg[int(seg.payload_off[k]):int(seg.payload_off[k + 1])])
    return out


_cases = None


def golden_cases():
    """tests/golden/segment.json (frames built by the reference): dicts with
    message (str), isn, chunk, frames (list of bytes); loaded once."""
    global _cases
    if _cases is None:
        doc = json.loads((GOLDEN / "segment.json").read_text(encoding="utf-8"))
        _cases = [dict(message=doc["messages"][c["message"]], isn=c["isn"], chunk=c["chunk"],
                       frames=[bytes.fromhex(f) for f in c["frames"]]) for c in doc["cases"]]
    return _cases
