"""ReliableUDP(batch_recv=True) over 127.0.0.1: recv() takes whole recvmmsg
batches, judges them on the device in one call (batch.receive) and answers
with one sendmmsg.  The sender is the existing per-datagram one; the text, the
replies it sees and the receiver's carried state must be what the
per-datagram receiver gives."""
import select
import socket
import threading

import pytest

from rudp.transport import ACK, FIN, SYN, ReliableUDP, build, parse

pytestmark = pytest.mark.gpu

JOIN_S = 10  # a failure ends the test instead of hanging it


@pytest.fixture(autouse=True, scope="module")
def _warm_device(cuda):
    """The first device call of a process takes its time (runtime start, code
    object load): made here, not under the sender's retransmission timer."""
    import torch
    from rudp import batch
    frame = torch.frombuffer(bytearray(build(7, 0, SYN | FIN, "")), dtype=torch.uint8).to(cuda)
    res = batch.receive(frame, torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5")
    assert res.reply_count == 1 and res.accepted.end == 0


def _server():
    server = ReliableUDP(codec_device="cuda:0", batch_recv=True).create()
    server.bind("127.0.0.1", 0)
    return server, server.socket.getsockname()[1]


def _recv_in_thread(server, got):
    """server.recv() on a thread; returns it once recv() has flushed its socket
    (it does on entry, utils/reliableUDP.py:112), so nothing sent after this is lost."""
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


class Doubler:
    """A forwarder between one client and the server that sends every datagram
    towards the server twice (no drops: the run is deterministic)."""

    def __init__(self, sport):
        self.front = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.front.bind(("127.0.0.1", 0))
        self.back = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.back.bind(("127.0.0.1", 0))
        self.port, self.sport = self.front.getsockname()[1], sport
        self.stop, self.wake = threading.Event(), socket.socketpair()
        self.to_server, self.to_client, self.client = [], [], None
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        while not self.stop.is_set():
            ready, _, _ = select.select([self.front, self.back, self.wake[0]], [], [])
            if self.front in ready:
                data, self.client = self.front.recvfrom(2048)
                self.to_server.append(data)
                for _ in range(2):
                    self.back.sendto(data, ("127.0.0.1", self.sport))
            if self.back in ready:
                data, _ = self.back.recvfrom(2048)
                self.to_client.append(data)
                if self.client is not None:
                    self.front.sendto(data, self.client)

    def close(self):
        self.stop.set()
        self.wake[1].send(b"x")
        self.thread.join(JOIN_S)
        for s in (self.front, self.back, *self.wake):
            s.close()


@pytest.mark.parametrize("message", ["plain ASCII text, one character per datagram", "aé€😀 ß中\n😀", ""],
                         ids=["ascii", "utf8_1_to_4_bytes", "empty"])
def test_batched_receiver_gets_the_text(message):
    server, sport = _server()
    got = []
    t = _recv_in_thread(server, got)
    client = ReliableUDP(timeout=2, isn_source=lambda: 4999).create()
    client.send(message, "127.0.0.1", sport)
    t.join(JOIN_S)
    assert got == [message]
    assert server._last_isn == 4999 and server._peer == ("127.0.0.1", client.socket.getsockname()[1])
    client.close()
    server.close()


def test_every_frame_twice():
    """Every data frame arrives twice (often in one batch): the copy is answered
    with the same ACK and not appended, as the per-datagram loop does."""
    message = "twice é€😀 over"
    server, sport = _server()
    got = []
    t = _recv_in_thread(server, got)
    relay = Doubler(sport)
    client = ReliableUDP(timeout=2, isn_source=lambda: 300).create()
    client.send(message, "127.0.0.1", relay.port)
    t.join(JOIN_S)
    relay.close()
    assert got == [message]
    # the sender never had to resend: one datagram per character, the FIN's ACK, nothing else
    sent = [parse(d) for d in relay.to_server]
    assert [p.payload for p in sent[:len(message)]] == list(message) and len(sent) == len(message) + 1
    # every data frame was answered twice with ACK(ISN + characters so far), in order
    acks = [parse(d) for d in relay.to_client]
    data_acks = [p.ack for p in acks if p.flags == ACK]
    # (the copy of the last frame comes behind the end of the transfer: it belongs to the FIN handshake)
    assert data_acks == [300 + k for k in range(1, len(message)) for _ in range(2)] + [300 + len(message)]
    assert acks[-1].flags == FIN | ACK and acks[-1].ack == 300 + len(message)
    client.close()
    server.close()


def test_two_transfers_and_the_repeated_syn():
    """Two transfers in a row on one receiver: the second recv() ignores a
    repeated SYN of the first transfer's ISN (but answers it, to the peer it
    carried over), then takes the next transfer from another sender."""
    server, sport = _server()
    got = []
    t = _recv_in_thread(server, got)
    client = ReliableUDP(timeout=2, isn_source=lambda: 100).create()
    client.send("hi", "127.0.0.1", sport)
    t.join(JOIN_S)
    assert got == ["hi"] and server._last_isn == 100
    t2 = _recv_in_thread(server, got)
    client.socket.settimeout(JOIN_S)
    for frame in (build(100, 0, SYN, "h"),        # the first transfer's SYN again: no new transfer
                  build(100 + 1, 0, FIN, "i")):   # and its last frame, resent late
        client.socket.sendto(frame, ("127.0.0.1", sport))
        reply = parse(client.socket.recvfrom(1024)[0])
        assert reply.flags == ACK and reply.ack == 0 and reply.seq == 0  # (ack = 0 + 0: no transfer yet)
    assert server._peer == ("127.0.0.1", client.socket.getsockname()[1]) and t2.is_alive()
    other = ReliableUDP(timeout=2, isn_source=lambda: 200).create()
    other.send("ok é", "127.0.0.1", sport)
    t2.join(JOIN_S)
    assert got == ["hi", "ok é"]
    assert server._last_isn == 200 and server._peer == ("127.0.0.1", other.socket.getsockname()[1])
    for s in (client, other, server):
        s.close()
