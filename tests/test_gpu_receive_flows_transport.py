"""flows.FlowReceiver(fused=True) over 127.0.0.1: every batch through the one
library call (batch.receive_flows_fused), the replies and the FIN|ACK datagrams
sent as the device built them.  Three plain per-datagram senders transfer at
the same time and every message arrives whole; and a peer whose FIN|ACK is
lost gets the device-built frame again without holding the slot for ever, as
tests/test_gpu_flows_transport.py has it for the default receiver."""
import socket
import threading

import pytest

from rudp import netio
from rudp.flows import FlowReceiver
from rudp.transport import ACK, FIN, SYN, ReliableUDP, build, parse

pytestmark = pytest.mark.gpu

JOIN_S = 10  # a failure ends the test instead of hanging it


def _receiver(max_flows=8):
    sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    sock.bind(("127.0.0.1", 0))
    rx = FlowReceiver(sock, "cuda:0", max_flows=max_flows, fused=True)
    assert rx.fused
    return rx, sock.getsockname()[1]


@pytest.fixture(autouse=True, scope="module")
def _warm_device(cuda):
    """The first device calls of a process take their time (runtime start, code
    object load): made here, not under a sender's retransmission timer."""
    rx, port = _receiver()
    peer = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    peer.settimeout(JOIN_S)
    peer.sendto(build(7, 0, SYN | FIN, "w"), ("127.0.0.1", port))
    assert [text for _, text in rx.serve(1, timeout=JOIN_S)] == ["w"]
    peer.close()
    rx.sock.close()


def test_three_concurrent_senders_fused():
    rx, port = _receiver()
    messages = ["x", "sept é€", "forty characters, some of them wide: 😀中ß"]
    assert [len(m) for m in messages] == [1, 7, 40]
    clients = [ReliableUDP(timeout=0.2, isn_source=lambda k=k: 1000 * (k + 1)).create() for k in range(3)]
    for c in clients:
        c.socket.bind(("127.0.0.1", 0))
    threads = [threading.Thread(target=c.send, args=(m, "127.0.0.1", port), daemon=True)
               for c, m in zip(clients, messages)]
    for t in threads:
        t.start()
    got = rx.serve(3, timeout=JOIN_S)
    assert sorted(got) == sorted((("127.0.0.1", c.socket.getsockname()[1]), m) for c, m in zip(clients, messages))
    deadline = 0
    while any(t.is_alive() for t in threads) and deadline < 50:  # the final ACKs come in; nothing else is due
        rx.poll(100)
        deadline += 1
    for t in threads:
        t.join(JOIN_S)
        assert not t.is_alive()
    while rx.closing and deadline < 100:
        rx.poll(100)
        deadline += 1
    assert not rx.closing and len(rx.table) == 0  # every handshake completed: every slot is free again
    assert not rx.states.any().item()
    for c in clients:
        c.close()
    rx.sock.close()


def test_lost_fin_ack_is_sent_again_and_the_slot_released_fused():
    rx, port = _receiver()
    peer = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    peer.bind(("127.0.0.1", 0))
    peer.settimeout(JOIN_S)
    key = netio.addr_key("127.0.0.1", peer.getsockname()[1])
    dest = ("127.0.0.1", port)

    peer.sendto(build(300, 0, SYN, "a"), dest)
    assert rx.poll(JOIN_S * 1000) == []
    reply = parse(peer.recvfrom(1024)[0])
    assert (reply.flags, reply.ack, reply.seq) == (ACK, 301, 0)
    slot = rx.table.slot_of(key)
    assert slot is not None and rx.states[slot].tolist() == [301, 300, 1, 0]

    fin = build(301, 0, FIN, "b")
    peer.sendto(fin, dest)
    assert rx.poll(JOIN_S * 1000) == [(("127.0.0.1", peer.getsockname()[1]), "ab")]
    replies = [parse(peer.recvfrom(1024)[0]) for _ in range(2)]
    assert [(r.flags, r.ack) for r in replies] == [(ACK, 302), (FIN | ACK, 302)]
    assert slot in rx.closing and rx.states[slot].tolist() == [0, 0, 0, 301]  # the flow turned over
    assert rx.closing[slot].frame == build(0, 302, FIN | ACK)  # the device's frame is kept for the resends

    peer.sendto(fin, dest)  # the FIN|ACK was lost: the sender's last frame again
    assert rx.poll(JOIN_S * 1000) == []
    again = parse(peer.recvfrom(1024)[0])
    assert (again.flags, again.ack) == (FIN | ACK, 302)
    assert rx.table.slot_of(key) == slot and rx.closing[slot].sends_left == 18

    peer.sendto(build(302, 1, ACK), dest)  # the final ACK
    assert rx.poll(JOIN_S * 1000) == []
    assert rx.table.slot_of(key) is None and len(rx.table) == 0 and not rx.closing
    assert rx.states[slot].tolist() == [0, 0, 0, 0]
    peer.close()
    rx.sock.close()
