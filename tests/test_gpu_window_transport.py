"""The reordering receiver behind a windowed cumulative sender.

A scripted channel (no sockets, no timing): a sender model with 8 frames in
flight whose script loses the first copy of three frames and swaps two
adjacent pairs; batch.receive_window delivers the message with fewer
transmissions than the in-order batch.receive, and with exactly as many as the
plain-loop rule in its place.  Then 127.0.0.1: ReliableUDP(batch_recv=True,
reorder_window=8) receives from ReliableUDP(batch_send=True, window=8,
cumulative=True) through a forwarder that holds back every 7th datagram by one
position."""
import random
import select
import socket
import threading

import numpy as np
import pytest

from accept_ref import pack_frames, parse_rudp5
from rudp import batch
from rudp.transport import FIN, SYN, ReliableUDP, build
from window_ref import window_ref

pytestmark = pytest.mark.gpu

JOIN_S = 20  # a failure ends the test instead of hanging it
CHARS = ("a", "é", "€", "😀")  # 1, 2, 3 and 4 bytes
MESSAGE = "".join(random.Random(200).choice(CHARS) for _ in range(200))
ISN, W = 1000, 8
LOSE_FIRST_COPY = (3, 50, 51)
SWAP = (20, 120)  # frame k goes out behind frame k + 1


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)


def sender_model(receiver):
    """A windowed cumulative sender against `receiver` (flight of datagrams ->
    (ack numbers of its replies, transfer ended)).  Returns the data frames it
    transmitted."""
    T = len(MESSAGE)
    frames = [build(ISN + k, 0, (SYN if k == 0 else 0) | (FIN if k == T - 1 else 0), MESSAGE[k]) for k in range(T)]
    lost, base, nxt, sent = set(), 0, 0, 0
    for _ in range(10 * T):
        hi = min(base + W, T)
        if nxt >= hi:  # the window is out and unacknowledged: the timeout goes back to base
            nxt = base
        flight = list(range(nxt, hi))
        nxt = hi
        sent += len(flight)
        for k in LOSE_FIRST_COPY:
            if k in flight and k not in lost:
                lost.add(k)
                flight.remove(k)
        for k in SWAP:
            if k in flight and k + 1 in flight:
                i = flight.index(k)
                flight[i], flight[i + 1] = flight[i + 1], flight[i]
        acks, ended = receiver([frames[k] for k in flight])
        if ended:
            return sent
        if acks:
            base = max(base, max(acks) - ISN)
            nxt = max(nxt, base)
    raise AssertionError("the sender model never finished")


class DeviceWindow:
    def __init__(self, cuda):
        self.cuda, self.state, self.carried, self.parts = cuda, (0, 0, 0), None, []

    def __call__(self, flight):
        if not flight:
            return [], False
        buf, off = pack_frames(flight)
        res = batch.receive_window(_dev(self.cuda, buf), _dev(self.cuda, off), "rudp5", window_chars=W,
                                   carried=self.carried, state=self.state)
        self.state, self.carried = res.state, res.carried
        acc = res.accepted
        if acc.msg_start < len(acc):
            self.parts = []
        self.parts.append(bytes(res.message.check().payload.cpu().numpy()))
        return res.reply_ack.cpu().numpy().tolist(), acc.end < len(acc)


class DeviceInOrder(DeviceWindow):
    def __call__(self, flight):
        if not flight:
            return [], False
        buf, off = pack_frames(flight)
        res = batch.receive(_dev(self.cuda, buf), _dev(self.cuda, off), "rudp5", state=self.state)
        self.state = res.state
        acc = res.accepted
        self.parts.append(bytes(res.message.check().payload.cpu().numpy()))
        ack = acc.reply_ack.cpu().numpy()[acc.reply.cpu().numpy() == 1]
        return ack.tolist(), acc.end < len(acc)


class RuleWindow:
    """window_ref in the device's place, the pending frames carried by hand."""

    def __init__(self):
        self.state, self.pending, self.parts = (0, 0, 0), [], []

    def __call__(self, flight):
        if not flight:
            return [], False
        frames = self.pending + flight
        m = len(self.pending)
        seq, flags, payloads = parse_rudp5(frames)
        chars = np.array([len(p.decode()) for p in payloads], np.uint32)
        r = window_ref(seq, flags, chars, None, self.state, window_chars=W, n_carried=m)
        self.state = r.state
        self.pending = [frames[i] for i in np.flatnonzero(r.accept == 2)]
        ranked = np.flatnonzero(r.rank != 0xFFFFFFFF)
        self.parts.append(b"".join(payloads[i] for i in ranked[np.argsort(r.rank[ranked])]))
        return r.reply_ack[m:][r.reply[m:] == 1].tolist(), r.info[0] < len(frames)


def test_scripted_channel(cuda):
    window, inorder, rule = DeviceWindow(cuda), DeviceInOrder(cuda), RuleWindow()
    sent_window = sender_model(window)
    assert b"".join(window.parts).decode() == MESSAGE
    sent_inorder = sender_model(inorder)
    assert b"".join(inorder.parts).decode() == MESSAGE
    sent_rule = sender_model(rule)
    assert b"".join(rule.parts).decode() == MESSAGE
    assert len(MESSAGE) < sent_window < sent_inorder, (sent_window, sent_inorder)
    assert sent_window == sent_rule


# ------------------------------------------------------------------- loopback
class Forwarder:
    """client <-> server on 127.0.0.1; every 7th client datagram waits for the
    one behind it and goes out after it."""

    def __init__(self, server_port):
        self.sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.sock.bind(("127.0.0.1", 0))
        self.port = self.sock.getsockname()[1]
        self.server = ("127.0.0.1", server_port)
        self.client, self.held, self.count, self.swapped = None, None, 0, 0
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self.run, daemon=True)

    def run(self):
        while not self.stop.is_set():
            ready, _, _ = select.select([self.sock], [], [], 0.05)
            if not ready:
                if self.held is not None:  # nothing came behind it: on its way alone
                    self.sock.sendto(self.held, self.server)
                    self.held = None
                continue
            data, addr = self.sock.recvfrom(65535)
            if addr == self.server:
                if self.client is not None:
                    self.sock.sendto(data, self.client)
                continue
            self.client = addr
            self.count += 1
            if self.count % 7 == 0 and self.held is None:
                self.held = data
                continue
            self.sock.sendto(data, self.server)
            if self.held is not None:
                self.sock.sendto(self.held, self.server)
                self.held = None
                self.swapped += 1


@pytest.fixture(scope="module")
def warm(cuda):
    """The first device calls of a process take their time (runtime start, code
    object load): made here, not under the sender's retransmission timer."""
    import torch
    frame = torch.frombuffer(bytearray(build(0, 7, FIN | 0x40, "")), dtype=torch.uint8).to(cuda)
    assert batch.acknowledge(frame, torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5", isn=7,
                             total_chars=0).done
    rx = batch.receive_window(torch.frombuffer(bytearray(build(7, 0, SYN | FIN, "")), dtype=torch.uint8).to(cuda),
                              torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5", window_chars=W)
    assert rx.reply_count == 1 and rx.reply_frames("rudp5").numel() == 5 and rx.carried.count == 0
    ReliableUDP(codec_device="cuda:0")._gpu_frames("warm", 7)


@pytest.mark.parametrize("message", ["".join(random.Random(7).choice("abcdefgh ") for _ in range(120)),
                                     "😀𐍈" * 40], ids=["ascii", "four_byte_characters"])
def test_loopback_through_a_reordering_forwarder(warm, message):
    server = ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_window=W).create()
    server.bind("127.0.0.1", 0)
    fwd = Forwarder(server.socket.getsockname()[1])
    fwd.thread.start()
    got = []
    flushed = threading.Event()
    flush = server.flush_recv_buffer

    def flush_and_tell():
        flush()
        flushed.set()
    server.flush_recv_buffer = flush_and_tell
    receiver = threading.Thread(target=lambda: got.append(server.recv()), daemon=True)
    receiver.start()
    assert flushed.wait(JOIN_S)
    server.flush_recv_buffer = flush
    client = ReliableUDP(timeout=2.0, isn_source=lambda: 4999, codec_device="cuda:0", batch_send=True, window=W,
                         cumulative=True).create()
    sender = threading.Thread(target=lambda: client.send(message, "127.0.0.1", fwd.port), daemon=True)
    sender.start()
    sender.join(JOIN_S)
    receiver.join(JOIN_S)
    fwd.stop.set()
    fwd.thread.join(JOIN_S)
    alive = sender.is_alive() or receiver.is_alive() or fwd.thread.is_alive()
    client.close()
    server.close()
    fwd.sock.close()
    assert not alive
    assert got == [message]
    assert fwd.swapped >= 1
