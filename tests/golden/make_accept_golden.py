"""Generate tests/golden/accept.json from the REFERENCE utils/packet.py and recv().

Runs only in the build container, where /root/reference exists; the tests read
the fixture this writes, never the reference.  The reference modules are loaded
from their own path (nothing is copied).  Every stream is received by the
reference's own ``ReliableUDP.recv()`` (utils/reliableUDP.py:111-202, compiled
from its file with the one statement of ``send()`` that does not parse below
Python 3.12 blanked in memory) through a stub socket that hands out the
datagrams and keeps the replies; the datagrams and the replies are built and
parsed with the reference's ``Packet``.

Each case records ``frames`` (hex, one string per datagram, arrival order),
``last_isn`` (prev_random_number, null for None), ``state`` (expect, isn, live
before the first datagram; recv() starts every call at 0, 0, and live means
target_addr is set) and what the reference did: ``replied`` (one digit per
datagram: a reply was sent), ``ack`` (the reply's ack_num, 0 without a reply),
``end`` (the index of the datagram after which the receiver sent its FIN, the
datagram count when it never did; datagrams behind it are not received and
have zeros), ``message`` (what recv() returns, or the buffer it was waiting
with when the datagrams ran out) and ``state_after`` (expect, isn, live from
its attributes).  ``accepted`` (one digit per datagram) is the project's
restatement of the rule (tests/accept_ref.py): the reference does not show it
for a datagram that leaves its state as it was, and the generator fails unless
the restatement agrees with recv() on everything else above.  ``clean`` marks
streams a stop-and-wait sender alone produces (retransmissions included).

usage: python tests/golden/make_accept_golden.py
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
REF_RUDP = Path("/root/reference/utils/reliableUDP.py")
sys.path.insert(0, str(HERE.parent))
from accept_ref import accept_ref  # noqa: E402

CHUNKS = (1, 2, 3, 5, 16)
ISN = 3611
SEED = 0xACCE97


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_packet", REF_PACKET)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame(mod, seq: int, payload: str = "", syn=False, fin=False, ack=False, ack_num: int = 0) -> bytes:
    packet = mod.Packet()
    packet.set_header_field("seq_num", str(seq), base=10)
    packet.set_header_field("ack_num", str(ack_num), base=10)
    for name, on in (("syn", syn), ("ack", ack), ("fin", fin)):
        if on:
            packet.set_header_field(name, "1", base=2)
    packet.set_payload(payload)
    return packet.to_byte()


def send_frames(mod, message: str, isn: int, payload_size: int):
    """Every datagram send_data builds while the message pointer advances (:44-61)."""
    frames, pointer = [], 0
    while True:
        end = min(pointer + payload_size, len(message))
        frames.append(frame(mod, pointer + isn, message[pointer:end], syn=pointer == 0, fin=end == len(message)))
        if end == len(message):
            return frames
        pointer = end


class _Drained(Exception):
    """The stub socket has no datagram left: recv() is abandoned where it waits."""


class StubSocket:
    """The socket recv() talks to: hands out the stream's datagrams one by one,
    keeps what is sent and for which datagram, answers the receiver's FIN with
    the sender's last ACK (ack_num 1), and has nothing queued when flushed."""

    def __init__(self, mod, datagrams):
        self.mod, self.datagrams, self.taken = mod, datagrams, 0
        self.blocking, self.timeout, self.sent = True, None, []

    def setblocking(self, flag):
        self.blocking = flag

    def settimeout(self, timeout):
        self.timeout = timeout

    def recvfrom(self, size):
        if not self.blocking:
            raise BlockingIOError
        if self.timeout is not None:  # the wait for the final ACK
            return frame(self.mod, 0, ack=True, ack_num=1), "peer"
        if self.taken == len(self.datagrams):
            raise _Drained
        self.taken += 1
        return self.datagrams[self.taken - 1], "peer"

    def sendto(self, data, addr):
        self.sent.append((self.taken - 1, data))


def load_receiver(mod):
    """The reference's ReliableUDP class, compiled from its own file.  One
    statement of send() (a nested f-string, :50) does not parse below Python
    3.12; it is blanked in memory, recv() is untouched."""
    lines = REF_RUDP.read_text().splitlines()
    for i, line in enumerate(lines):
        if "Aborted after" in line:
            lines[i] = line[:len(line) - len(line.lstrip())] + "pass"
    sys.path.insert(0, str(REF_RUDP.parent.parent))
    try:
        space = {"__name__": "reference_reliable_udp"}
        exec(compile("\n".join(lines), str(REF_RUDP), "exec"), space)
    finally:
        sys.path.pop(0)
    return space["ReliableUDP"]


def receive(mod, receiver_cls, datagrams, last_isn, state):
    """The reference's own recv() over the datagrams, through a stub socket;
    what it did is read from the socket, its return value and its attributes.
    ``accepted`` is not observable there (a retransmitted SYN is accepted into
    the state it already has): it comes from the project's restatement of the
    rule, tests/accept_ref.py, which must agree with everything that is."""
    assert tuple(state[:2]) == (0, 0)  # recv() starts every call at pointer 0, random_number 0
    n = len(datagrams)
    rx = receiver_cls()
    rx.socket = sock = StubSocket(mod, datagrams)
    rx.prev_random_number = last_isn
    rx.target_addr = "peer" if state[2] else None
    end, message = n, None
    try:
        message = rx.recv()
    except _Drained as stop:
        tb = stop.__traceback__
        while tb is not None:  # the buffer receive_data was waiting with
            if tb.tb_frame.f_code.co_name == "receive_data":
                message = tb.tb_frame.f_locals["buffer"]
            tb = tb.tb_next
        after = [rx.random_number + len(message), rx.random_number, 1] if rx.target_addr else list(state)
    else:
        after = [rx.prev_random_number + len(message), rx.prev_random_number, 1]
    replied, acks = [0] * n, [0] * n
    for index, data in sock.sent:
        packet = mod.Packet(data)
        if packet.get_header_field("fin", base=2) == "1":
            end = min(end, index)  # the receiver's FIN|ACK: the transfer ended with this datagram
        else:
            assert not replied[index]
            replied[index], acks[index] = 1, int(packet.get_header_field("ack_num", base=10))
    if not rx.target_addr:
        message = ""  # nothing is kept while there is no peer
    # the restated rule on what Packet parses, checked against all of the above
    parsed = [mod.Packet(d) for d in datagrams]
    seq = [int(p.get_header_field("seq_num", base=10)) for p in parsed]
    flags = [int(p.get_header_field("syn", base=2) + p.get_header_field("ack", base=2)
                 + p.get_header_field("fin", base=2), 2) << 5 for p in parsed]
    chars = [len(p.get_payload() or "") for p in parsed]
    r = accept_ref(seq, flags, chars, None, tuple(state), last_isn)
    text = "".join(parsed[i].get_payload() or "" for i in range(n) if r.keep[i])
    assert (r.reply.tolist(), r.reply_ack.tolist(), r.end, text, list(r.state)) == (replied, acks, end, message, after), \
        "the restated rule and the reference's recv() disagree"
    return {"accepted": "".join(map(str, r.accept)), "replied": "".join(map(str, replied)), "ack": acks, "end": end,
            "message": message, "state_after": after}


def repeat(rng, frames, lo=1, hi=3):
    return [f for f in frames for _ in range(rng.randint(lo, hi))]


def main():
    mod = load_reference()
    receiver_cls = load_receiver(mod)
    rng = random.Random(SEED)
    texts = json.loads((HERE / "segment.json").read_text(encoding="utf-8"))["messages"]
    trace = json.loads((HERE / "wire_trace.json").read_text())
    cases = []

    def add(name, datagrams, last_isn=None, state=(0, 0, 0), clean=True):
        rec = receive(mod, receiver_cls, datagrams, last_isn, tuple(state))
        cases.append({"name": name, "clean": clean, "last_isn": last_isn, "state": list(state),
                      "frames": [d.hex() for d in datagrams], **rec})

    # the captured transfer (the sender's last datagram, its ACK of the FIN, lies behind the end)
    wire = [bytes.fromhex(h) for h in trace["client_to_server"]]
    add("wire_trace", wire)
    for k in range(3):
        add(f"wire_trace_repeated_{k}", repeat(rng, wire))
    # the segment.json texts, 1-4-byte characters, in datagrams of 1..16 characters
    for index, text in enumerate(texts):
        for chunk in CHUNKS:
            frames = send_frames(mod, text, ISN, chunk)
            add(f"text{index}_chunk{chunk}", frames if (index + chunk) % 2 else repeat(rng, frames),
                state=(0, 0, index % 2))
    # ISN 65530: the sender's seq_num wraps, the receiver's integer does not: the reference stalls
    stall = send_frames(mod, "wraps past the end", 65530, 1)
    add("isn_65530_stall", repeat(rng, stall, 1, 2))
    add("isn_65530_chunk5_stall", send_frames(mod, "wraps past the end", 65530, 5))
    # a repeated SYN of the previous transfer, without and with a peer, then a new transfer
    again = frame(mod, ISN, "t", syn=True)
    nxt = send_frames(mod, "next", 4000, 1)
    add("repeated_syn_no_peer", [again, again] + nxt, last_isn=ISN)
    add("repeated_syn_peer", [again] + nxt[:2] + [again] + nxt[2:], last_isn=ISN, state=(0, 0, 1))
    # a new SYN in the middle of a transfer
    first = send_frames(mod, "abandoned", 100, 1)
    second = send_frames(mod, "délivré", 2000, 2)
    add("new_syn_mid_transfer", first[:4] + second)
    add("new_syn_mid_transfer_repeated", repeat(rng, first[:6]) + repeat(rng, second))
    # the empty message
    add("empty_message", send_frames(mod, "", ISN, 1))
    add("empty_message_twice", send_frames(mod, "", ISN, 1) * 2)
    # a frame from the future in the middle of a transfer (no sender of this protocol sends one)
    hello = send_frames(mod, "hello world", 100, 1)
    add("future_frame", hello[:3] + [hello[8]] + hello[3:], clean=False)
    add("future_frame_first", [hello[0], hello[5]] + hello[1:], clean=False)
    add("future_frame_wide", hello[:2] + [frame(mod, 150, "zzzz")] + hello[2:], clean=False)
    # a data frame before any SYN: without a peer, and with one at expect 0, seq 0
    stray = frame(mod, 0, "x")
    add("stray_no_peer", [stray, frame(mod, 1, "y")] + nxt, clean=False)
    add("stray_peer", [stray, frame(mod, 1, "y")] + nxt, state=(0, 0, 1), clean=False)

    path = HERE / "accept.json"
    path.write_text(json.dumps({"cases": cases}, separators=(",", ":"), ensure_ascii=False) + "\n", encoding="utf-8")
    total = sum(len(c["frames"]) for c in cases)
    print(f"{path}: {len(cases)} cases, {total} datagrams, {path.stat().st_size} file bytes")


if __name__ == "__main__":
    main()
