"""Stop-and-wait transfer of one message over UDP: the codec's caller (config 1).

The reference's only production caller of utils/packet.py is its
utils/reliableUDP.py (class ReliableUDP, :8-202), which does not parse below
Python 3.12 (PEP 701 f-string at :50).  This module is written from the
protocol it implements and the wire trace captured from it
(tests/golden/wire_trace.json): the same public surface, the same bytes on the
wire, organised as two loops, one per role.

Protocol (one character of payload per datagram, utils/reliableUDP.py:11):

* sender — draws an ISN in [1, 5000]; frame k carries message[k] with
  seq = ISN + k, ack 0, SYN on k = 0 and FIN on the last character (an empty
  message is one SYN|FIN frame).  It waits ``timeout`` seconds for a reply
  whose ack_num is ISN + k + len(payload); other replies are ignored, a
  timeout resends frame k.  Twenty sends without progress abort the transfer.
  An ACK moves k to ack_num - ISN.  After the last frame it keeps waiting for
  the receiver's FIN, answers it with ACK(seq = ISN + k, ack = peer seq + 1)
  and returns.
* receiver — answers the sender of the last SYN it accepted (kept across
  recv() calls, so a stray frame before the next SYN is ACKed there); accepts
  a SYN (unless it repeats the previous transfer's ISN) as
  a new transfer and then the frame whose seq - ISN equals the characters
  received so far; every datagram is answered with ACK(ack = ISN + characters
  received).  After accepting a FIN frame it sends FIN|ACK(ack = ISN + length)
  up to twenty times, half a second apart, until an ACK with ack_num 1 comes
  back, and returns the message.

``ReliableUDP(codec_device="cuda:0")`` frames the sender's data frames on the
GPU: every frame a transfer can send is known once the ISN is drawn, so one
pack_batch_varlen launch (rudp5, the reference's 5-byte layout) builds the
table and each send, retransmissions included, takes row k.  Same wire bytes.

``ReliableUDP(codec_device=..., batch_send=True, window=W)`` is a windowed
sender over the same table: up to W frames in flight (sendmmsg), the replies
taken in recvmmsg batches and each batch judged on the GPU in one call
(batch.acknowledge: wait_ack's rule for every reply, the new state, and the
closing datagram at the receiver's FIN).  With W = 1 the wire carries the same
bytes as the loop above.  ``cumulative=True`` lets a reply past the expected
one count, so a lost reply does not cost a timeout (the reference, with one
frame in flight, has no counterpart).
"""
from __future__ import annotations

import ipaddress
import random
from socket import AF_INET, SOCK_DGRAM, socket
from typing import Any, Callable, NamedTuple, Optional

from .batch import ACK, FIN, SYN
from .packet import Packet

MAX_DATAGRAM = 1024   # recvfrom size of the reference (utils/reliableUDP.py:9)
MAX_SENDS = 20        # sends without progress before giving up (:10)
CHUNK = 1             # characters per datagram (:11)
FIN_WAIT_S = 0.5      # receiver's wait for the final ACK (:166)
FLOW_LINGER_S = 1.0   # flows.FlowSender: an ended flow keeps its slot this long to repeat its closing ACK


class Reply(NamedTuple):
    seq: int
    ack: int
    flags: int
    payload: str


def build(seq: int, ack: int, flags: int, payload: str = "") -> bytes:
    """One frame through the drop-in codec (seq/ack taken mod 2^16 as
    set_header_field keeps the low 16 bits, utils/packet.py:56)."""
    p = Packet()
    p.set_header_field("seq_num", str(seq), base=10)
    p.set_header_field("ack_num", str(ack), base=10)
    for name, bit in (("syn", SYN), ("ack", ACK), ("fin", FIN)):
        if flags & bit:
            p.set_header_field(name, "1", base=2)
    p.set_payload(payload)
    return p.to_byte()


def parse(data: bytes) -> Reply:
    p = Packet(data)
    flags = sum(bit for name, bit in (("syn", SYN), ("ack", ACK), ("fin", FIN))
                if p.get_header_field(name, base=2) == "1")
    return Reply(int(p.get_header_field("seq_num", base=10)), int(p.get_header_field("ack_num", base=10)),
                 flags, p.get_payload() or "")


class ReliableUDP:
    BUFFER_SIZE = MAX_DATAGRAM
    RETRIES = MAX_SENDS
    PAYLOAD_SIZE = CHUNK

    def __init__(self, timeout=1, isn_source: Optional[Callable[[], int]] = None,
                 codec_device: Optional[str] = None, batch_recv: bool = False, batch_send: bool = False,
                 window: int = 1, cumulative: bool = False, reorder_window: Optional[int] = None,
                 reorder_fused: bool = False):
        self.socket: socket
        self.retransmission_timeout = timeout
        self._draw_isn = isn_source or (lambda: random.randint(1, 5000))
        self._codec_device = codec_device
        if batch_recv and not codec_device:
            raise ValueError("batch_recv=True judges the datagrams on the GPU: it needs codec_device")
        if batch_send and not codec_device:
            raise ValueError("batch_send=True judges the replies on the GPU: it needs codec_device")
        if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= 1024:
            raise ValueError(f"window must be an int in [1, 1024] frames in flight, got {window!r}")
        if (window != 1 or cumulative) and not batch_send:
            raise ValueError("window and cumulative belong to the windowed sender: they need batch_send=True")
        # send() keeps `window` frames in flight and judges the replies of each recvmmsg batch on the
        # device (_transmit_window); cumulative: a reply past the expected one counts (a lost reply does not stall)
        self._batch_send, self._window, self._cumulative = batch_send, window, cumulative
        self._batch_recv = batch_recv  # recv() over recvmmsg batches judged on the device (_recv_batches)
        if reorder_window is not None:
            if not batch_recv:
                raise ValueError("reorder_window belongs to the batched receiver: it needs batch_recv=True")
            if isinstance(reorder_window, bool) or not isinstance(reorder_window, int) \
                    or not 1 <= reorder_window <= 1024:
                raise ValueError(f"reorder_window must be an int in [1, 1024] characters, got {reorder_window!r}")
        # recv() keeps the frames that arrive ahead of the expected one inside this many characters and
        # answers with cumulative acks (_recv_batches_window); None: the reference's in-order receiver
        self._reorder_window = reorder_window
        if reorder_fused and reorder_window is None:
            raise ValueError("reorder_fused belongs to the reordering receiver: it needs reorder_window")
        # each batch judged, gathered and answered in one library call (batch.receive_windowed); False:
        # the chain of calls (batch.receive_window)
        self._reorder_fused = bool(reorder_fused)
        self._rx: Any = None           # its BatchReceiver, made on first use
        self._last_isn: Optional[int] = None  # the previous transfer's ISN (a repeated SYN is ignored)
        # the sender of the last SYN, kept across recv() calls as the reference
        # keeps self.target_addr (utils/reliableUDP.py:18, :131 only ever set it):
        # a stray non-SYN datagram at the start of a later recv() is answered there
        self._peer: Any = None

    # ------------------------------------------------------------ socket
    def create(self):
        self.socket = socket(AF_INET, SOCK_DGRAM)
        return self

    def bind(self, ip, port):
        self.socket.bind((str(ipaddress.ip_address(ip)), port))

    def close(self):
        self.socket.close()

    def flush_recv_buffer(self):
        """Drop whatever is queued on the socket (stale replies of an earlier transfer)."""
        self.socket.setblocking(False)
        try:
            while True:
                self.socket.recvfrom(65535)
        except BlockingIOError:
            pass
        finally:
            self.socket.setblocking(True)

    def _receive(self, timeout: Optional[float]):
        """(Reply, addr), or None when nothing arrived within `timeout` seconds."""
        self.socket.settimeout(timeout)
        try:
            data, addr = self.socket.recvfrom(MAX_DATAGRAM)
        except TimeoutError:
            return None
        return parse(data), addr

    # ------------------------------------------------------------ sender
    def send(self, message: str, ip, port) -> None:
        self.flush_recv_buffer()
        try:
            if self._batch_send:
                self._transmit_window(message, (str(ipaddress.ip_address(ip)), port))
            else:
                self._transmit(message, (str(ipaddress.ip_address(ip)), port))
        finally:
            self.flush_recv_buffer()

    def _transmit(self, message: str, dest) -> None:
        isn = self._draw_isn()
        table = self._gpu_frames(message, isn) if self._codec_device else None
        k, sends_left = 0, MAX_SENDS
        expect = None  # (ack_num that acknowledges the outstanding frame, it was the last one)
        while True:
            if expect is None:  # (re)send frame k
                n = CHUNK if k < len(message) else 0
                last = k + n >= len(message)
                if sends_left < 1:
                    if not last:
                        print(f"\033[91mAborted after {MAX_SENDS * self.retransmission_timeout} seconds "
                              f"({MAX_SENDS} sends of character {k} unacknowledged)\033[0m")
                    return
                if table is not None:
                    frame = table[0][table[1][k]:table[1][k + 1]]
                else:
                    flags = (SYN if k == 0 else 0) | (FIN if last else 0)
                    frame = build(isn + k, 0, flags, message[k:k + n])
                self.socket.sendto(frame, dest)
                sends_left -= 1
                expect = (isn + k + n, last)
            got = self._receive(self.retransmission_timeout)
            if got is None:
                expect = None  # timeout: resend
                continue
            reply = got[0]
            if reply.ack != expect[0]:
                continue  # not for the outstanding frame
            if reply.flags & ACK:
                k = reply.ack - isn
            if reply.flags & FIN:
                self.socket.sendto(build(isn + k, reply.seq + 1, ACK), dest)
                return
            if expect[1]:
                expect = (isn + k, True)  # everything is sent: wait for the FIN
            else:
                expect, sends_left = None, MAX_SENDS

    def _batch_receiver(self):
        """The socket's BatchReceiver (recvmmsg into pinned slots, H2D, one library call), made on first use."""
        import torch
        from . import netio
        if self._rx is None or self._rx.sock is not self.socket:
            self._rx = netio.BatchReceiver(self.socket, max_msgs=1024, slot_bytes=MAX_DATAGRAM, slots=2,
                                           device=torch.device(self._codec_device), with_sources=True)
        return self._rx

    def _transmit_window(self, message: str, dest) -> None:
        """_transmit with up to ``window`` frames in flight: the frames of
        _gpu_frames go out with sendmmsg, the replies come in recvmmsg batches,
        and each batch is judged on the device in one call (batch.acknowledge:
        wait_ack's rule for every reply, the new state, and the closing datagram
        at the receiver's FIN).  A timeout goes back to the frame at the
        acknowledged pointer, as send_data does, and MAX_SENDS timeouts without
        progress give up."""
        import numpy as np
        from . import netio
        isn = self._draw_isn()
        frames, off = self._gpu_frames(message, isn)
        frames, off = np.frombuffer(frames, np.uint8), np.asarray(off, np.int64)
        T, W = len(message), self._window
        rows = max(-(-T // CHUNK), 1)  # data rows; row `rows` (T > 0) is the header-only FIN frame of a late resend
        mode = "cumulative" if self._cumulative else "exact"
        rx = self._batch_receiver()
        self.socket.setblocking(True)

        def put(lo, hi):
            netio.send_batch(self.socket, frames[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], *dest)

        p, nxt, sends_left = 0, 0, MAX_SENDS  # characters acknowledged, next row to send, sends left for the frame at p
        state: Any = None                      # the device's (p, L, last, done); None: a fresh transfer
        while True:
            base = -(-p // CHUNK)
            hi = min(base + W, rows)
            if nxt < hi:
                put(nxt, hi)
                nxt = hi
            n = rx.recv(timeout_ms=max(int(self.retransmission_timeout * 1000), 1))
            if n == 0:  # timeout: back to the frame at p, L and last recomputed from p (SEND_DATA)
                L = min(CHUNK, T - p)
                sends_left -= 1
                if sends_left < 1:
                    if p + L < T:
                        print(f"\033[91mAborted after {MAX_SENDS * self.retransmission_timeout} seconds "
                              f"({MAX_SENDS} sends of character {p} unacknowledged)\033[0m")
                    return
                state, nxt = (p, L, int(p + L == T), 0), base
                if T and p == T:
                    put(rows, rows + 1)
                continue
            res, _, _ = rx.acknowledge("rudp5", isn=isn, total_chars=T, chunk=CHUNK, state=state, mode=mode,
                                       sent=min(nxt * CHUNK, T))
            state = res.state
            if res.done:  # (the one wait per batch; every host read below is behind it)
                self.socket.sendto(res.final_frame.cpu().numpy().tobytes(), dest)
                return
            if res.pointer_after != p:
                p, sends_left = res.pointer_after, MAX_SENDS

    def _gpu_frames(self, message: str, isn: int):
        """Frames for k = 0..len(message) in one GPU launch: (bytes, offsets)."""
        import numpy as np
        import torch
        from . import batch
        dev = torch.device(self._codec_device)
        # rows k < len(message) cut on the device (one character each, seq, SYN and FIN
        # as send_data sets them); an empty message is the one SYN|FIN row
        seg = batch.segment_message(message, isn, chunk=CHUNK, device=dev, check=False)
        tab = seg.table()
        seq, ack, flags, lens = tab.headers.seq, tab.headers.ack, tab.headers.flags, tab.lengths
        if message:  # k = len(message): the header-only FIN frame a late resend carries
            def append(col, value, dtype):  # (joined as bytes: every dtype concatenates that way)
                row = torch.from_numpy(np.array([value], dtype).view(np.uint8)).to(dev)
                return torch.cat((col.view(torch.uint8), row)).view(col.dtype)
            seq = append(seq, (isn + len(message)) & 0xFFFF, np.uint16)
            ack = append(ack, 0, np.uint16)
            flags = append(flags, FIN, np.uint8)
            lens = append(lens, 0, np.int32)
        res = batch.pack_batch_varlen((seq, ack, flags), seg.payload, lens, "rudp5", want_csum=False)
        return res.frames.cpu().numpy().tobytes(), res.frame_off.cpu().tolist()

    # ----------------------------------------------------------- receiver
    def _recv_batches(self):
        """The receive loop of recv() over whole recvmmsg batches: each batch is
        copied to the device and judged there in one call (batch.receive), its
        reply datagrams go out with one sendmmsg, and its part of the message
        joins the buffer.  Returns (isn, text, peer) as the loop below leaves them."""
        import numpy as np
        from . import netio
        rx = self._batch_receiver()
        self.socket.setblocking(True)
        peer = self._peer
        state = (0, 0, 1 if peer is not None else 0)  # no transfer yet; live: there is someone to answer
        parts = []
        while True:
            n = rx.recv(timeout_ms=-1)
            if n == 0:
                continue
            res, _, _ = rx.receive("rudp5", state=state, last_isn=self._last_isn)
            state = res.state
            R = res.reply_count  # (the one wait per batch; every host read below is behind it)
            acc = res.accepted
            if R:
                carried = netio.addr_key(*peer) if peer is not None else 0
                src = np.append(rx.sources, np.uint64(carried))  # index n: the peer carried from earlier batches
                dst = src[res.reply_peer[:R].cpu().numpy()]
                netio.send_batch_to(self.socket, res.reply_frames[:5 * R].cpu().numpy(),
                                    5 * np.arange(R + 1, dtype=np.int64), dst)
            if acc.msg_start < n:  # a new transfer started in this batch
                parts = []
                peer = netio.key_addr(int(rx.sources[acc.msg_start]))
                self._peer = peer
            if peer is None:  # nothing to answer yet: nothing is kept
                parts = []
            elif res.message_bytes:
                parts.append(res.message.payload.cpu().numpy().tobytes())
            if acc.end < n:
                break
        return int(state[1].item()), b"".join(parts).decode(), peer

    def _recv_batches_window(self):
        """_recv_batches for a windowed sender: each batch is judged behind the
        frames the batch before left pending (batch.receive_window: a frame
        ahead of the expected one inside reorder_window characters waits for
        the gap to fill), its part of the message arrives in delivery order
        and every reply is a cumulative acknowledgement.  With reorder_fused
        a batch is one library call (batch.receive_windowed) and one wait, at
        reply_count: the sizes of the pending frames come out of the same read."""
        import numpy as np
        from . import netio
        rx = self._batch_receiver()
        self.socket.setblocking(True)
        peer = self._peer
        state = (0, 0, 1 if peer is not None else 0)
        parts, carried = [], None
        while True:
            n = rx.recv(timeout_ms=-1)
            if n == 0:
                continue
            receive = rx.receive_windowed if self._reorder_fused else rx.receive_window
            res, _, _ = receive("rudp5", window_chars=self._reorder_window, carried=carried, state=state,
                                last_isn=self._last_isn)
            state, carried = res.state, res.carried
            acc, m = res.accepted, res.n_carried
            R = res.reply_count  # (every host read below is behind this wait)
            if R:
                held = netio.addr_key(*peer) if peer is not None else 0
                src = np.append(rx.sources, np.uint64(held))  # index n: the peer carried from earlier batches
                dst = src[res.reply_peer.cpu().numpy()]
                frames = res.reply_frames if self._reorder_fused else res.reply_frames("rudp5")
                netio.send_batch_to(self.socket, frames.cpu().numpy(), 5 * np.arange(R + 1, dtype=np.int64), dst)
            if m <= acc.msg_start < m + n:  # a new transfer started in this batch
                parts = []
                peer = netio.key_addr(int(rx.sources[acc.msg_start - m]))
                self._peer = peer
            if peer is None:  # nothing to answer yet: nothing is kept
                parts = []
            elif res.message.total[1]:
                parts.append(res.message.payload.cpu().numpy().tobytes())
            if acc.end < m + n:
                break
        return int(state[1].item()), b"".join(parts).decode(), peer

    def recv(self) -> str:
        self.flush_recv_buffer()
        if self._batch_recv:
            isn, text, peer = self._recv_batches_window() if self._reorder_window else self._recv_batches()
            return self._finish_recv(isn, text, peer)
        isn, text, peer = 0, "", self._peer
        received = 0  # characters accepted so far (the next in-order frame is isn + received)
        while True:
            reply, addr = self._receive(None)
            syn = bool(reply.flags & SYN)
            in_order = (received == 0 and syn) or reply.seq - isn == received
            repeated_syn = syn and reply.seq == self._last_isn
            finished = False
            if syn and not repeated_syn:  # a new transfer starts here
                isn, received, peer, text = reply.seq, 0, addr, ""
                self._peer = peer
            if (in_order or syn) and not repeated_syn:
                text += reply.payload
                received = len(text)
                finished = bool(reply.flags & FIN)
            if peer is None:  # nothing to answer yet
                text = ""
                continue
            self.socket.sendto(build(0, isn + len(text), ACK), peer)
            if finished:
                break
        return self._finish_recv(isn, text, peer)

    def _finish_recv(self, isn: int, text: str, peer) -> str:
        for _ in range(MAX_SENDS):
            self.socket.sendto(build(0, isn + len(text), FIN | ACK), peer)
            got = self._receive(FIN_WAIT_S)
            if got is not None and got[0].flags & ACK and got[0].ack == 1:
                break
        self._last_isn = isn
        self.flush_recv_buffer()
        return text
