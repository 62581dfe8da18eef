"""Generate tests/golden/segment.json from the REFERENCE utils/packet.py.

Runs only in the build container, where /root/reference exists; the tests read
the fixture this writes, never the reference.  The reference module is imported
from its own path (nothing is copied), and every frame is built in the exact
call order of ``send_data`` (utils/reliableUDP.py:44-61): the message pointer
walks the text in slices of PAYLOAD_SIZE characters, seq_num = pointer + ISN,
ack_num 0, syn on the first slice, fin on the last, then set_payload, to_byte.
(utils/reliableUDP.py itself does not parse below Python 3.12, and its
PAYLOAD_SIZE is fixed at 1; the loop below is its send_data with the slice
size as a parameter.)

Each case records ``message`` (an index into the file's ``messages`` list:
every text serves twelve cases), ``isn``, ``chunk`` and ``frames`` (hex, one
string per datagram).

usage: python tests/golden/make_segment_golden.py
"""
from __future__ import annotations

import importlib.util
import json
import random
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_PACKET = Path("/root/reference/utils/packet.py")
REF_INPUT = Path("/root/reference/bin/input.txt")

CHUNKS = (1, 2, 3, 5, 16, 300)
ISNS = (3611, 65530)  # 65530: seq wraps past 2^16 inside the message
SEED = 0x5EED5E60
# make_golden.py's make_varlen alphabet: 1-4-byte characters, U+0000, U+FFFF
ALPHABET = "abcxyz019 \n\t~" + "éßñ" + "€中文字" + "😀🚀" + "\u0000\u007f\u0080\u07ff\u0800\uffff"


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_packet", REF_PACKET)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def send_frames(mod, message: str, isn: int, payload_size: int):
    """Every datagram send_data builds while the message pointer advances."""
    frames, pointer = [], 0
    while True:
        end = min(pointer + payload_size, len(message))
        is_first = pointer == 0
        is_last = end == len(message)
        packet = mod.Packet()
        packet.set_header_field("seq_num", str(pointer + isn), base=10)
        packet.set_header_field("ack_num", "0", base=10)
        if is_first:
            packet.set_header_field("syn", "1", base=2)
        if is_last:
            packet.set_header_field("fin", "1", base=2)
        packet.set_payload(message[pointer:end])
        frames.append(packet.to_byte())
        if is_last:
            return frames
        pointer = end


def messages():
    rng = random.Random(SEED)
    out = ["", "a", "é", "😀", REF_INPUT.read_text()]
    out += ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 200))) for _ in range(20)]
    return out


def main():
    mod = load_reference()
    cases, texts = [], messages()
    for index, message in enumerate(texts):
        for chunk in CHUNKS:
            for isn in ISNS:
                frames = send_frames(mod, message, isn, chunk)
                cases.append({"message": index, "isn": isn, "chunk": chunk, "frames": [f.hex() for f in frames]})
    path = HERE / "segment.json"
    path.write_text(json.dumps({"messages": texts, "cases": cases}, separators=(",", ":"), ensure_ascii=False) + "\n", encoding="utf-8")
    total = sum(len(f) // 2 for c in cases for f in c["frames"])
    print(f"{path}: {len(cases)} cases, {total} frame bytes, {path.stat().st_size} file bytes")


if __name__ == "__main__":
    main()
