"""ReliableUDP(batch_recv=True, reorder_window=8, reorder_fused=True): the
reordering receiver with each batch one library call (batch.receive_windowed),
behind ReliableUDP(batch_send=True, window=8, cumulative=True) on 127.0.0.1,
through a forwarder that holds back every 7th client datagram by one position
and loses the first copy of the 13th and the 40th.  Then the scripted channel
of test_gpu_window_transport.py: exactly as many transmissions as
batch.receive_window needs."""
import random
import select
import socket
import threading

import numpy as np
import pytest

from accept_ref import pack_frames
from rudp import batch
from rudp.transport import FIN, SYN, ReliableUDP, build
from test_gpu_window_transport import MESSAGE, DeviceWindow, W, sender_model

pytestmark = pytest.mark.gpu

JOIN_S = 20  # a failure ends the test instead of hanging it
DROP = (13, 40)  # client datagrams (counted from 1) whose first copy is lost


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)


class DeviceWindowed(DeviceWindow):
    def __call__(self, flight):
        if not flight:
            return [], False
        buf, off = pack_frames(flight)
        res = batch.receive_windowed(_dev(self.cuda, buf), _dev(self.cuda, off), "rudp5", window_chars=W,
                                     carried=self.carried, state=self.state)
        self.state, self.carried = res.state, res.carried
        acc = res.accepted
        if acc.msg_start < len(acc):
            self.parts = []
        self.parts.append(bytes(res.check().message.payload.cpu().numpy()))
        return res.reply_ack.cpu().numpy().tolist(), acc.end < len(acc)


def test_scripted_channel(cuda):
    fused, chain = DeviceWindowed(cuda), DeviceWindow(cuda)
    sent_fused = sender_model(fused)
    assert b"".join(fused.parts).decode() == MESSAGE
    assert sent_fused == sender_model(chain)
    assert b"".join(chain.parts).decode() == MESSAGE


class Forwarder:
    """client <-> server on 127.0.0.1; every 7th client datagram waits for the
    one behind it and goes out after it; the datagrams of DROP are lost."""

    def __init__(self, server_port):
        self.sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.sock.bind(("127.0.0.1", 0))
        self.port = self.sock.getsockname()[1]
        self.server = ("127.0.0.1", server_port)
        self.client, self.held, self.count, self.swapped, self.dropped = None, None, 0, 0, 0
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
            if self.count in DROP:
                self.dropped += 1
                continue
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
    rx = batch.receive_windowed(torch.frombuffer(bytearray(build(7, 0, SYN | FIN, "")), dtype=torch.uint8).to(cuda),
                                torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5", window_chars=W)
    assert rx.reply_count == 1 and rx.reply_frames.numel() == 5 and rx.carried.count == 0
    ReliableUDP(codec_device="cuda:0")._gpu_frames("warm", 7)


@pytest.mark.parametrize("message", ["".join(random.Random(7).choice("abcdefgh ") for _ in range(120)),
                                     "😀𐍈é€" * 25], ids=["ascii", "multi_byte_characters"])
def test_loopback_through_a_lossy_reordering_forwarder(warm, message):
    server = ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_window=W, reorder_fused=True).create()
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
    client = ReliableUDP(timeout=0.5, isn_source=lambda: 4999, codec_device="cuda:0", batch_send=True, window=W,
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
    assert fwd.swapped >= 1 and fwd.dropped == len(DROP)
