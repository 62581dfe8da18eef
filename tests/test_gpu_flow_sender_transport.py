"""flows.FlowSender over 127.0.0.1: one sender socket delivers three different
messages to three reference-style receivers at once.  Every recvmmsg batch,
whatever mix of the three transfers' replies it carries, is judged on the
device in one call (batch.acknowledge_flows), which also builds the closing
datagrams; one peer's loss never holds up another peer's transfer."""
import random
import socket
import threading

import pytest

from rudp import batch, flows
from rudp.relay import Relay
from rudp.transport import ACK, FIN, ReliableUDP, build, parse

pytestmark = pytest.mark.gpu

JOIN_S = 10  # a failure ends the test instead of hanging it
CHARS = ("a", "é", "€", "😀")  # 1, 2, 3 and 4 bytes
MIXED = "".join(random.Random(300).choice(CHARS) for _ in range(300))
ISNS = (4999, 65000, 17)


@pytest.fixture(autouse=True, scope="module")
def _warm_device(cuda):
    """The first device calls of a process take their time (runtime start, code
    object load): made here, not under the sender's retransmission timers."""
    import torch
    frame = torch.frombuffer(bytearray(build(0, 7, FIN | ACK, "")), dtype=torch.uint8).to(cuda)
    states = batch.ack_flow_states(4, cuda)
    batch.ack_flow_open(states, 2, 7, 0, 1)
    res = batch.acknowledge_flows(frame, torch.tensor([0, 5], dtype=torch.int64, device=cuda),
                                  torch.tensor([2], dtype=torch.int32, device=cuda), "rudp5", states=states)
    assert res.judged.check().ended == 1 and res.judged.finals() == [(0, build(7, 1, ACK, ""))]
    frames, off = ReliableUDP(codec_device="cuda:0")._gpu_frames("warm", 7)
    assert len(off) == 6 and len(frames) == off[-1] == 5 * 5 + 4


def _recv_in_thread(server, got):
    """server.recv() on a thread; returns it once recv() has flushed its socket
    (it does on entry), so nothing sent after this is lost."""
    flushed = threading.Event()
    flush = server.flush_recv_buffer

    def flush_and_tell():
        flush()
        flushed.set()

    server.flush_recv_buffer = flush_and_tell
    t = threading.Thread(target=lambda: got.append(server.recv()), daemon=True)
    t.start()
    assert flushed.wait(JOIN_S)
    server.flush_recv_buffer = flush
    return t


def _drop_once(direction, index):
    seen = set()

    def drop(d, i):
        if (d, i) == (direction, index) and (d, i) not in seen:
            seen.add((d, i))
            return True
        return False
    return drop


def deliver(messages, *, window, cumulative=False, drops=None, timeout=2.0):
    """One FlowSender, one receiver and one relay per message; returns the
    sender's results, what each receiver got, the relays and the sender."""
    drops = drops or [None] * len(messages)
    servers, relays, gots, threads = [], [], [], []
    for drop in drops:
        server = ReliableUDP().create()
        server.bind("127.0.0.1", 0)
        relay = Relay(server.socket.getsockname()[1], drop)
        relay.start()
        got = []
        threads.append(_recv_in_thread(server, got))
        servers.append(server), relays.append(relay), gots.append(got)
    sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    sock.bind(("127.0.0.1", 0))
    isns = iter(ISNS)
    tx = flows.FlowSender(sock, "cuda:0", max_flows=8, window=window, cumulative=cumulative, timeout=timeout,
                          isn_source=lambda: next(isns))
    for message, relay in zip(messages, relays):
        tx.submit(message, ("127.0.0.1", relay.port))
    results = tx.run(timeout=JOIN_S)
    for t in threads:
        t.join(JOIN_S)
    for relay in relays:
        relay.stop()
        assert not relay.errors
    for server in servers:
        server.close()
    sock.close()
    return results, gots, relays, tx


@pytest.mark.parametrize("cumulative", [False, True], ids=["exact", "cumulative"])
@pytest.mark.parametrize("window", [1, 8])
def test_three_messages_to_three_receivers(window, cumulative):
    messages = ["", "x", MIXED]
    results, gots, relays, tx = deliver(messages, window=window, cumulative=cumulative)
    assert gots == [[m] for m in messages]
    assert sorted(results) == sorted((("127.0.0.1", r.port), True) for r in relays)
    assert tx.resent == 0 and len(tx) == 0
    for message, relay, isn in zip(messages, relays, ISNS):
        sent = [parse(d) for d in relay.log["c2s"]]
        # no timeout ran: every character went out once, in order, then the closing ACK of the receiver's FIN
        assert [p.payload for p in sent[:-1]] == (list(message) or [""]) and len(sent) == max(len(message), 1) + 1
        assert sent[-1] == ((isn + len(message)) & 0xFFFF, 1, ACK, "")
        assert parse(relay.log["s2c"][-1]).flags == FIN | ACK


def test_one_peers_losses_do_not_touch_the_others():
    """Frame 5 of the first transfer and reply 5 of the second are lost once:
    the first goes back after its own timeout, the second takes the next reply
    (cumulative mode: with a window the exact rule cannot get past a lost
    reply, as for the single-peer windowed sender), and all three arrive; the
    third transfer completes without a resend."""
    messages = [MIXED[:40], MIXED[40:80], MIXED[80:120]]
    results, gots, relays, tx = deliver(messages, window=8, timeout=0.2, cumulative=True,
                                        drops=[_drop_once("c2s", 5), _drop_once("s2c", 5), None])
    assert gots == [[m] for m in messages]
    assert sorted(results) == sorted((("127.0.0.1", r.port), True) for r in relays)
    assert relays[0].stats["client_dropped"] == 1 and relays[1].stats["server_dropped"] == 1
    assert [parse(d).seq for d in relays[0].log["c2s"]].count(ISNS[0] + 5) >= 2  # lost, then resent
    assert tx.resent >= 1
    untouched = [parse(d) for d in relays[2].log["c2s"]]
    assert [p.payload for p in untouched[:-1]] == list(messages[2]) and len(untouched) == len(messages[2]) + 1


def test_constructor_and_submit_rules(cuda):
    sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    sock.bind(("127.0.0.1", 0))
    try:
        with pytest.raises(ValueError, match="rudp5"):
            flows.FlowSender(sock, "cuda:0", layout="rudp7")
        with pytest.raises(ValueError, match="window"):
            flows.FlowSender(sock, "cuda:0", window=0)
        tx = flows.FlowSender(sock, "cuda:0", max_flows=1, isn_source=lambda: 9)
        slot = tx.submit("ab", ("127.0.0.1", 9))
        assert slot == 0 and len(tx) == 1
        assert tx.states[0].tolist() == [0, 1, 0, 0, 9, 2, 1, 0]
        with pytest.raises(ValueError, match="still running"):
            tx.submit("cd", ("127.0.0.1", 9))
        with pytest.raises(RuntimeError, match="slots"):
            tx.submit("cd", ("127.0.0.1", 10))
    finally:
        sock.close()
