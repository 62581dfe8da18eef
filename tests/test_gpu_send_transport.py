"""ReliableUDP(batch_send=True) over 127.0.0.1: send() keeps a window of frames
in flight (sendmmsg), takes the replies in recvmmsg batches and judges each
batch on the device in one call (batch.acknowledge), which also builds the
closing datagram.  The receivers are the existing ones, per datagram and
batched; with window=1 the wire carries the reference's bytes both ways."""
import random
import threading

import pytest

from rudp.relay import Relay
from rudp.transport import ACK, FIN, SYN, ReliableUDP, build, parse

pytestmark = pytest.mark.gpu

JOIN_S = 10  # a failure ends the test instead of hanging it
CHARS = ("a", "é", "€", "😀")  # 1, 2, 3 and 4 bytes
MIXED = "".join(random.Random(300).choice(CHARS) for _ in range(300))


@pytest.fixture(autouse=True, scope="module")
def _warm_device(cuda):
    """The first device calls of a process take their time (runtime start, code
    object load): made here, not under the sender's retransmission timer."""
    import torch
    from rudp import batch
    frame = torch.frombuffer(bytearray(build(0, 7, FIN | ACK, "")), dtype=torch.uint8).to(cuda)
    res = batch.acknowledge(frame, torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5", isn=7,
                            total_chars=0)
    assert res.done and res.end == 0 and parse(bytes(res.final_frame.cpu().numpy())) == (7, 1, ACK, "")
    rx = batch.receive(torch.frombuffer(bytearray(build(7, 0, SYN | FIN, "")), dtype=torch.uint8).to(cuda),
                       torch.tensor([0, 5], dtype=torch.int64, device=cuda), "rudp5")
    assert rx.reply_count == 1
    frames, off = ReliableUDP(codec_device="cuda:0")._gpu_frames("warm", 7)
    assert len(off) == 6 and len(frames) == off[-1] == 5 * 5 + 4


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


def transfer(message, *, window, isn=4999, cumulative=False, batch_recv=False, drop=None, timeout=2.0):
    server = (ReliableUDP(codec_device="cuda:0", batch_recv=True) if batch_recv else ReliableUDP()).create()
    server.bind("127.0.0.1", 0)
    relay = Relay(server.socket.getsockname()[1], drop)
    relay.start()
    got = []
    t = _recv_in_thread(server, got)
    client = ReliableUDP(timeout=timeout, isn_source=lambda: isn, codec_device="cuda:0", batch_send=True,
                         window=window, cumulative=cumulative).create()
    client.send(message, "127.0.0.1", relay.port)
    t.join(JOIN_S)  # (the receiver returns on the closing datagram: the relay has logged everything by then)
    relay.stop()
    client.close()
    server.close()
    assert not relay.errors
    return got, relay


def test_window_1_puts_the_reference_bytes_on_the_wire(wire_trace):
    got, relay = transfer(wire_trace["message"], window=1, isn=wire_trace["isn"])
    assert got == [wire_trace["message"]]
    assert [d.hex() for d in relay.log["c2s"]] == wire_trace["client_to_server"]
    assert [d.hex() for d in relay.log["s2c"]] == wire_trace["server_to_client"]


@pytest.mark.parametrize("batch_recv", [False, True], ids=["per_datagram_receiver", "batched_receiver"])
@pytest.mark.parametrize("window", [8, 64])
@pytest.mark.parametrize("message", ["", "x", MIXED], ids=["empty", "one_character", "mixed_300"])
def test_windowed_sender_delivers(message, window, batch_recv):
    got, relay = transfer(message, window=window, batch_recv=batch_recv)
    assert got == [message]
    sent = [parse(d) for d in relay.log["c2s"]]
    # no timeout ran: every character went out once, in order, then the closing ACK of the receiver's FIN
    assert [p.payload for p in sent[:-1]] == (list(message) or [""]) and len(sent) == max(len(message), 1) + 1
    assert sent[0].flags & SYN and sent[-2].flags & FIN and sent[-1] == (4999 + len(message), 1, ACK, "")
    assert parse(relay.log["s2c"][-1]).flags == FIN | ACK


def _drop_once(direction, index):
    seen = set()

    def drop(d, i):
        if (d, i) == (direction, index) and (d, i) not in seen:
            seen.add((d, i))
            return True
        return False
    return drop


def test_a_lost_frame_is_resent_in_exact_mode():
    """Datagram 5 towards the receiver is lost: the acks behind it repeat ISN + 5,
    the exact rule ignores them, the timeout goes back to frame 5."""
    message = MIXED[:40]
    got, relay = transfer(message, window=8, drop=_drop_once("c2s", 5), timeout=0.2)
    assert got == [message]
    sent = [parse(d) for d in relay.log["c2s"]]
    assert [p.seq for p in sent].count(4999 + 5) >= 2 and relay.stats["client_dropped"] == 1  # (lost, then resent)


def test_a_lost_reply_does_not_stall_the_cumulative_sender():
    """Reply 5 towards the sender is lost: the next reply acknowledges past it and
    cumulative mode takes it, so nothing is sent twice."""
    message = MIXED[:40]
    got, relay = transfer(message, window=8, cumulative=True, drop=_drop_once("s2c", 5))
    assert got == [message]
    sent = [parse(d) for d in relay.log["c2s"]]
    assert len(sent) == len(message) + 1 and relay.stats["server_dropped"] == 1


def test_constructor_rules():
    with pytest.raises(ValueError, match="codec_device"):
        ReliableUDP(batch_send=True)
    with pytest.raises(ValueError, match="batch_send"):
        ReliableUDP(codec_device="cuda:0", window=8)
    with pytest.raises(ValueError, match="batch_send"):
        ReliableUDP(codec_device="cuda:0", cumulative=True)
    with pytest.raises(ValueError, match="window"):
        ReliableUDP(codec_device="cuda:0", batch_send=True, window=0)
