"""Generate tests/golden/ack.json from the REFERENCE utils/packet.py and send().

Runs only where make_accept_golden.py runs (it loads the reference the same
way, from its own path; nothing is copied); the tests read the fixture this
writes, never the reference.  Every case is sent by the reference's own
``ReliableUDP.send()`` (utils/reliableUDP.py:38-108) through a stub socket that
hands out scripted reply datagrams and keeps what is sent; ``randint`` is
pinned to the case's ISN and PAYLOAD_SIZE set to its chunk.  send() is
abandoned where it waits once the replies run out (no timeout is played).

Each case records ``message``, ``chunk``, ``isn``, ``replies`` (the reply
datagrams in arrival order as one hex string: every reply is a 5-byte header),
``sent`` (hex, every datagram send() sent) with ``sent_after`` (for each, the
index of the reply after which it went out, -1: before any; written as runs
[first, count] of consecutive indices), ``done`` (1 when
the closing send_ack datagram went out) and ``pointer`` (its message_pointer at
the end).  The generator fails unless the project's
restatement of the rule (tests/ack_ref.py), stepped reply by reply with the
state carried, predicts every datagram, ``done`` and ``pointer``.

usage: python tests/golden/make_ack_golden.py
"""
from __future__ import annotations

import json
import random
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
from ack_ref import ACK, ack_ref, fresh_state, parse_rudp5  # noqa: E402
from make_accept_golden import frame, load_receiver, load_reference  # noqa: E402

CHUNKS = (1, 2, 3, 5, 16)
ISN = 3611
SEED = 0xAC4901


class _Drained(Exception):
    """The stub socket has no reply left: send() is abandoned where it waits."""


class StubSocket:
    def __init__(self, replies):
        self.replies, self.taken = replies, 0
        self.blocking, self.sent = True, []

    def setblocking(self, flag):
        self.blocking = flag

    def settimeout(self, timeout):
        pass

    def recvfrom(self, size):
        if not self.blocking:
            raise BlockingIOError
        if self.taken == len(self.replies):
            raise _Drained
        self.taken += 1
        return self.replies[self.taken - 1], "peer"

    def sendto(self, data, addr):
        self.sent.append((self.taken - 1, data))


def reference_send(sender_cls, message, chunk, isn, replies):
    sender_cls.PAYLOAD_SIZE = chunk
    sender_cls.send.__globals__["randint"] = lambda lo, hi: isn
    tx = sender_cls()
    tx.socket = sock = StubSocket(replies)
    try:
        tx.send(message, "127.0.0.1", 9)
    except _Drained:
        pass
    return sock.sent, tx.message_pointer


def restated_send(mod, message, chunk, isn, replies):
    """What ack_ref says the sender sends: the rule stepped one reply at a time."""
    T = len(message)

    def data(state):
        p, L, last, _ = state
        return frame(mod, isn + p, message[p:p + L], syn=p == 0, fin=bool(last))

    state = fresh_state(T, chunk)
    sent = [(-1, data(state))]
    seq, ack, flags = parse_rudp5(replies)
    for i in range(len(replies)):
        was_last = state[2]
        r = ack_ref(seq[i:i + 1], ack[i:i + 1], flags[i:i + 1], isn=isn, T=T, C=chunk, state=state)
        state = r.state
        if r.done:
            sent.append((i, frame(mod, r.final[0], ack=True, ack_num=r.final[1])))
            break
        if r.valid[0] and not was_last:
            sent.append((i, data(state)))
    whole = ack_ref(seq, ack, flags, isn=isn, T=T, C=chunk)
    assert whole.state == state, "one call and reply-by-reply calls disagree"
    return sent, state


def acks_for(mod, message, chunk, isn, fin_seq=0):
    """The replies a receiver sends for a clean transfer: one ACK per frame, then FIN|ACK."""
    T, out, p = len(message), [], 0
    while True:
        p = min(p + chunk, T)
        out.append(frame(mod, 0, ack=True, ack_num=isn + p))
        if p == T:
            break
    out.append(frame(mod, fin_seq, ack=True, fin=True, ack_num=isn + T))
    return out


def runs(indices):
    """[first, count] for every run of consecutive indices."""
    out = []
    for i in indices:
        if out and i == out[-1][0] + out[-1][1]:
            out[-1][1] += 1
        else:
            out.append([i, 1])
    return out


def main():
    mod = load_reference()
    sender_cls = load_receiver(mod)
    rng = random.Random(SEED)
    texts = json.loads((HERE / "segment.json").read_text(encoding="utf-8"))["messages"]
    trace = json.loads((HERE / "wire_trace.json").read_text())
    cases = []

    def add(name, message, chunk, isn, replies):
        sent, pointer = reference_send(sender_cls, message, chunk, isn, replies)
        want, state = restated_send(mod, message, chunk, isn, replies)
        assert sent == want, f"{name}: the restated rule and the reference's send() disagree on a datagram"
        assert (pointer, int(any(i >= 0 and d[4] == ACK and len(d) == 5 for i, d in sent))) == (state[0], state[3]), name
        assert all(len(r) == 5 for r in replies)
        cases.append({"name": name, "message": message, "chunk": chunk, "isn": isn,
                      "replies": b"".join(replies).hex(), "sent_after": runs([i for i, _ in sent]),
                      "sent": [d.hex() for _, d in sent], "done": state[3], "pointer": pointer})

    def dup(replies, lo=1, hi=3):
        return [r for r in replies for _ in range(rng.randint(lo, hi))]

    # the captured transfer
    wire = [bytes.fromhex(h) for h in trace["server_to_client"]]
    add("wire_trace", trace["message"], 1, trace["isn"], wire)
    add("wire_trace_duplicated", trace["message"], 1, trace["isn"], dup(wire))
    # the segment.json texts; one of the short ones with duplicated (then stale) replies at every chunk
    for index, text in enumerate(texts):
        for chunk in CHUNKS:
            add(f"text{index}_chunk{chunk}", text, chunk, ISN, acks_for(mod, text, chunk, ISN))
    for chunk in CHUNKS:
        add(f"duplicated_chunk{chunk}", texts[15], chunk, ISN, dup(acks_for(mod, texts[15], chunk, ISN)))
    hello = "hello world"
    clean = acks_for(mod, hello, 2, 100)
    # stale replies: acks of frames long acknowledged, in between
    add("stale", hello, 2, 100, clean[:3] + [clean[0], clean[1]] + clean[3:] + [clean[2]])
    # a reply from the future, then the transfer goes on
    add("future", hello, 2, 100, clean[:2] + [clean[4]] + clean[2:])
    # a missing ACK flag on a middle frame and on the last frame (then the stale ack is taken, and a FIN at it)
    mid = frame(mod, 0, ack_num=100 + 4)
    add("no_ack_flag_middle", hello, 2, 100, clean[:1] + [mid] + clean[1:])
    lastf = frame(mod, 0, ack_num=100 + 11)
    add("no_ack_flag_last", hello, 2, 100, clean[:5] + [lastf] + clean[5:])
    add("no_ack_flag_last_then_stale_fin", hello, 2, 100,
        clean[:5] + [lastf, clean[4], frame(mod, 9, ack=True, fin=True, ack_num=100 + 10)])
    # FIN without ACK: the transfer ends and the pointer stays
    add("fin_without_ack", hello, 2, 100, clean[:6] + [frame(mod, 5, fin=True, ack_num=100 + 11)])
    add("fin_without_ack_early", hello, 2, 100, clean[:2] + [frame(mod, 5, fin=True, ack_num=100 + 6)] + clean[2:])
    # a stray FIN with a wrong ack is ignored
    add("stray_fin_wrong_ack", hello, 2, 100, clean[:2] + [frame(mod, 5, ack=True, fin=True, ack_num=100 + 11)]
        + clean[2:])
    # the empty message
    add("empty_message", "", 1, ISN, acks_for(mod, "", 1, ISN))
    add("empty_message_fin_only", "", 3, ISN, [frame(mod, 0, ack=True, fin=True, ack_num=ISN)])
    # ISN 65530: expected passes 65535 and nothing matches any more: the sender stalls
    add("isn_65530_stall", "wraps past the end", 1, 65530, dup(acks_for(mod, "wraps past the end", 1, 65530), 1, 2))
    add("isn_65530_chunk5_stall", "wraps past the end", 5, 65530, acks_for(mod, "wraps past the end", 5, 65530))
    # seq 65535 on the FIN: the closing ack_num wraps to 0
    add("fin_seq_65535", "ab", 1, 7, acks_for(mod, "ab", 1, 7, fin_seq=65535))

    path = HERE / "ack.json"
    path.write_text(json.dumps({"cases": cases}, separators=(",", ":"), ensure_ascii=False) + "\n", encoding="utf-8")
    total = sum(len(c["replies"]) // 10 for c in cases)
    print(f"{path}: {len(cases)} cases, {total} replies, {path.stat().st_size} file bytes")
    assert path.stat().st_size <= (HERE / "accept.json").stat().st_size


if __name__ == "__main__":
    main()
