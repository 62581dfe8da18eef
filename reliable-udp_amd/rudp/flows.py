"""Many peers on one socket: the host side of ``batch.receive_flows``.

``FlowTable`` maps a datagram's source (``netio.addr_key``) to the slot of its
peer's row in the device state table.  ``FlowReceiver`` is the small server
built on it: every recvmmsg batch, whatever mix of concurrent transfers it
carries, is judged on the device in one ``receive_flows`` call, the replies go
out with one sendmmsg, each to its own datagram's source, and every transfer
that ends is returned as ``(addr, text)`` and closed with the reference's
FIN|ACK handshake (``ReliableUDP._finish_recv``), kept per peer so that one
peer's lost FIN|ACK never holds up another peer's transfer.  ``FlowSender`` is
its counterpart on the send side: many messages to many peers at once, every
reply batch judged on the device in one ``acknowledge_flows`` call.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _native
from .batch import ACK, FIN, SYN, flow_states, layout_header_len
from .transport import CHUNK, FIN_WAIT_S, FLOW_LINGER_S, MAX_DATAGRAM, MAX_SENDS, build

FLOW_NONE = _native.FLOW_NONE


class FlowTable:
    """``addr_key`` -> slot, on the host.  A new peer gets the lowest free slot;
    with the table full an unknown peer gets ``FLOW_NONE`` (its datagrams are
    ignored) until a slot is released."""

    def __init__(self, capacity: int):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= 0xFFFFFFFE:
            raise ValueError(f"capacity must be an int in [1, 2^32 - 2], got {capacity!r}")
        self.capacity = capacity
        self._slot: Dict[int, int] = {}
        self._key: Dict[int, int] = {}
        self._next = 0               # slots at or above it were never handed out
        self._freed: List[int] = []  # released slots, kept sorted descending (pop gives the lowest)
        self.allocations = 0         # slots ever handed out

    def __len__(self) -> int:
        return len(self._slot)

    def slot_of(self, key: int) -> Optional[int]:
        return self._slot.get(int(key))

    def key_of(self, slot: int) -> Optional[int]:
        return self._key.get(int(slot))

    def _allocate(self, key: int) -> int:
        if self._freed:
            slot = self._freed.pop()
        elif self._next < self.capacity:
            slot, self._next = self._next, self._next + 1
        else:
            return FLOW_NONE
        self._slot[key], self._key[slot] = slot, key
        self.allocations += 1
        return slot

    def slots(self, sources) -> np.ndarray:
        """u32 [n]: the slot of every datagram's source, new peers allocated.
        One ``np.unique`` over the batch and one lookup per distinct peer."""
        keys, inverse = np.unique(np.asarray(sources, dtype=np.uint64), return_inverse=True)
        per = np.empty(keys.shape[0], np.uint32)
        for j, key in enumerate(keys.tolist()):
            slot = self._slot.get(key)
            per[j] = self._allocate(key) if slot is None else slot
        return per[inverse.reshape(-1)]

    def lookup(self, sources) -> np.ndarray:
        """As ``slots``, but an unknown peer gets ``FLOW_NONE`` and nothing is
        allocated: the sender's side, where a reply from a stranger has no flow."""
        keys, inverse = np.unique(np.asarray(sources, dtype=np.uint64), return_inverse=True)
        per = np.empty(keys.shape[0], np.uint32)
        for j, key in enumerate(keys.tolist()):
            slot = self._slot.get(key)
            per[j] = FLOW_NONE if slot is None else slot
        return per[inverse.reshape(-1)]

    def release(self, slot: int) -> None:
        key = self._key.pop(int(slot), None)
        if key is None:
            return
        del self._slot[key]
        self._freed.append(int(slot))
        self._freed.sort(reverse=True)


class _Closing:
    """A finished transfer whose FIN|ACK waits for the peer's final ACK."""
    __slots__ = ("frame", "isn", "sends_left", "deadline", "after")

    def __init__(self, frame: bytes, isn: int, deadline: float, after: int):
        self.frame, self.isn, self.sends_left, self.deadline, self.after = frame, isn, MAX_SENDS - 1, deadline, after


class FlowReceiver:
    """A multi-peer receiver on one bound UDP socket.

        rx = FlowReceiver(sock, "cuda:0")
        for addr, text in rx.serve(3): ...

    ``poll(timeout_ms)`` takes one recvmmsg batch (one wait for the device per
    batch) and returns the transfers it completed; ``serve(count)`` polls until
    ``count`` messages are in.  ``table`` (``FlowTable``) and ``states`` (the
    device table) are the per-peer state; ``closing`` the slots whose FIN|ACK
    still waits for the final ACK.  ``fused=True`` takes every batch through
    the one library call (``batch.receive_flows_fused``): the replies and the
    FIN|ACK datagrams come built from the device, one read per batch."""

    def __init__(self, sock, device, max_flows: int = 1024, layout="rudp5", fused: bool = False):
        import torch
        from . import netio
        self.sock, self.layout, self.H = sock, layout, layout_header_len(layout)
        self.device = torch.device(device)
        self.table = FlowTable(max_flows)
        self.states = flow_states(max_flows, self.device)
        self.rx = netio.BatchReceiver(sock, max_msgs=_native.FLOWS_MAX_BATCH, slot_bytes=MAX_DATAGRAM, slots=2,
                                      device=self.device, with_sources=True)
        self.closing: Dict[int, _Closing] = {}
        self._parts: Dict[int, List[bytes]] = {}
        self.fused = bool(fused)

    def _send_to(self, frame: bytes, key: int) -> None:
        from . import netio
        self.sock.sendto(frame, netio.key_addr(key))

    def _release(self, slot: int) -> None:
        self.closing.pop(slot, None)
        self._parts.pop(slot, None)
        self.table.release(slot)
        self.states[slot].zero_()  # a fresh flow for the slot's next peer (ordered before the next batch's call)

    def _resend(self, slot: int, c: _Closing, now: float) -> None:
        if c.sends_left > 0:
            self._send_to(c.frame, self.table.key_of(slot))
            c.sends_left -= 1
            c.deadline = now + FIN_WAIT_S
        else:
            self._release(slot)

    def _answer_closing(self, slots, seq, ack, flags, usable, now: float) -> None:
        """What the batch's datagrams mean for the slots whose FIN|ACK waits:
        the final ACK releases the slot; a datagram without ACK, or the closed
        transfer's SYN again, has the FIN|ACK sent again."""
        for slot, c in list(self.closing.items()):
            mine = np.flatnonzero((slots == slot) & usable)
            mine = mine[mine > c.after]
            c.after = -1
            resend = False
            for i in mine.tolist():
                f = int(flags[i])
                if f & ACK and not f & SYN and int(ack[i]) == 1:  # the handshake is complete
                    self._release(slot)
                    resend = False
                    break
                if not f & ACK or (f & SYN and int(seq[i]) == c.isn):
                    resend = True
            if resend:
                self._resend(slot, c, now)

    def _poll_fused(self, n: int, done) -> None:
        """One batch through ``batch.receive_flows_fused``: one read of the
        result; the replies and the closing datagrams go out as the device
        built them."""
        from . import netio
        sources = self.rx.sources.copy()
        slots = self.table.slots(sources)
        res, _, _ = self.rx.receive_flows_fused(slots, self.layout, states=self.states)
        rows, H = res.flows(), self.H  # (the one wait per batch; every host read below is of the same copy)
        R, E = res.replies, res.ended
        if R:
            netio.send_batch_to(self.sock, res.host("reply_frames")[:R * H], H * np.arange(R + 1, dtype=np.int64),
                                sources[res.host("reply_index")[:R]])
        fin = {int(a): res.host("fin_frames")[e * H:(e + 1) * H].tobytes()
               for e, a in enumerate(res.host("fin_flow")[:E].tolist())}
        now = time.monotonic()
        for a in range(rows.shape[0]):
            slot, end, _, msg_start, _, isn, kept, _ = (int(v) for v in rows[a])
            if msg_start < n:  # a new transfer of this peer started in the batch
                self._parts[slot] = []
                self.closing.pop(slot, None)
            if kept:
                self._parts.setdefault(slot, []).append(res.message(a))
            if end < n:
                text = b"".join(self._parts.pop(slot, [])).decode()
                key = self.table.key_of(slot)
                done.append((netio.key_addr(key), text))
                self._send_to(fin[a], key)
                self.closing[slot] = _Closing(fin[a], isn, now + FIN_WAIT_S, end)
        if self.closing:
            self._answer_closing(slots, res.host("seq"), res.host("ack"), res.host("flags"),
                                 res.host("usable") != 0, now)

    def poll(self, timeout_ms: int = -1) -> List[Tuple[Tuple[str, int], str]]:
        from . import netio
        import torch
        wait = timeout_ms
        if self.closing:
            due = max(0.0, min(c.deadline for c in self.closing.values()) - time.monotonic())
            due_ms = int(due * 1e3) + 1
            wait = due_ms if timeout_ms < 0 else min(timeout_ms, due_ms)
        self.sock.setblocking(True)
        n = self.rx.recv(timeout_ms=wait)
        done: List[Tuple[Tuple[str, int], str]] = []
        if n and self.fused:
            self._poll_fused(n, done)
        elif n:
            sources = self.rx.sources.copy()
            slots = self.table.slots(sources)
            res, _, _ = self.rx.receive_flows(slots, self.layout, states=self.states)
            rows = res.accepted.flows()  # (the one wait per batch; every host read below is behind it)
            idx = res.reply_index.cpu().numpy()
            if idx.shape[0]:
                netio.send_batch_to(self.sock, res.reply_frames(self.layout).cpu().numpy(),
                                    self.H * np.arange(idx.shape[0] + 1, dtype=np.int64), sources[idx])
            now = time.monotonic()
            for a in range(rows.shape[0]):
                slot, end, _, msg_start, characters, isn, kept, _ = (int(v) for v in rows[a])
                if msg_start < n:  # a new transfer of this peer started in the batch
                    self._parts[slot] = []
                    self.closing.pop(slot, None)
                if kept:
                    self._parts.setdefault(slot, []).append(res.message(a))
                if end < n:
                    text = b"".join(self._parts.pop(slot, [])).decode()
                    key = self.table.key_of(slot)
                    done.append((netio.key_addr(key), text))
                    fin = build(0, isn + characters, FIN | ACK)
                    self._send_to(fin, key)
                    self.closing[slot] = _Closing(fin, isn, now + FIN_WAIT_S, end)
            if self.closing:
                dec = res.decoded
                self._answer_closing(slots, dec.seq.view(torch.int16).cpu().numpy().view(np.uint16),
                                     dec.ack.view(torch.int16).cpu().numpy().view(np.uint16), dec.flags.cpu().numpy(),
                                     res.usable.cpu().numpy() != 0, now)
        now = time.monotonic()
        for slot, c in list(self.closing.items()):
            if now >= c.deadline:  # FIN_WAIT_S without the final ACK
                self._resend(slot, c, now)
        return done

    def serve(self, count: int, timeout: Optional[float] = None) -> List[Tuple[Tuple[str, int], str]]:
        """Poll until ``count`` messages are complete (or ``timeout`` seconds
        have passed) and return them as ``(addr, text)`` in completion order."""
        out: List[Tuple[Tuple[str, int], str]] = []
        stop = None if timeout is None else time.monotonic() + timeout
        while len(out) < count:
            left = -1 if stop is None else int(max(0.0, stop - time.monotonic()) * 1e3)
            if stop is not None and left == 0:
                break
            out.extend(self.poll(left))
        return out


class _Sending:
    """One submitted message: its frames (rows 0..rows-1 the data, row ``rows``
    the header-only FIN frame of a late resend when T > 0) and where it stands."""
    __slots__ = ("key", "slot", "frames", "off", "T", "rows", "p", "nxt", "sends_left", "deadline", "closing",
                 "linger")

    def __init__(self, key, slot, frames, off, T, deadline):
        self.key, self.slot, self.frames, self.off, self.T = key, slot, frames, off, T
        self.rows = max(-(-T // CHUNK), 1)
        self.p, self.nxt, self.sends_left, self.deadline = 0, 0, MAX_SENDS, deadline
        self.closing: Optional[bytes] = None  # the closing datagram, once the flow has ended
        self.linger = 0.0


class FlowSender:
    """A multi-peer sender on one UDP socket: ``ReliableUDP(batch_send=True,
    window=W)``'s transfer for many peers at once.

        tx = FlowSender(sock, "cuda:0", window=8)
        tx.submit("hello", ("127.0.0.1", 5000)); tx.submit("world", ("127.0.0.1", 5001))
        for addr, ok in tx.run(): ...

    ``submit`` frames a message on the device (``ReliableUDP._gpu_frames``) and
    opens its peer's row of the device table.  ``poll(timeout_ms)`` sends every
    flow's frames up to its window in one sendmmsg, takes one recvmmsg batch,
    has it judged for all flows in one ``acknowledge_flows`` call (one wait
    for the device per batch), advances every flow, sends the device-built
    closing datagram of each flow that ended and returns those as ``(addr,
    True)``; a flow whose ``timeout`` ran out goes back to the frame at its
    pointer as ``_transmit_window`` does, and after ``MAX_SENDS`` timeouts
    without progress is given up, ``(addr, False)``.  Every flow has its own
    timer, so one peer's loss never holds up another's transfer.  An ended
    flow keeps its slot for ``FLOW_LINGER_S``: a FIN from that peer in that
    time gets the closing datagram again."""

    def __init__(self, sock, device, max_flows: int = 1024, window: int = 8, cumulative: bool = False,
                 timeout: float = 1.0, layout="rudp5", isn_source=None):
        import random
        import torch
        from . import netio
        from .batch import ack_flow_states
        from .transport import ReliableUDP
        if layout_header_len(layout) != 5:
            raise ValueError("FlowSender speaks ReliableUDP's wire format: layout must be 'rudp5'")
        if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= 1024:
            raise ValueError(f"window must be an int in [1, 1024] frames in flight, got {window!r}")
        self.sock, self.layout, self.window, self.timeout = sock, layout, window, float(timeout)
        self.mode = "cumulative" if cumulative else "exact"
        self.device = torch.device(device)
        self.table = FlowTable(max_flows)
        self.states = ack_flow_states(max_flows, self.device)
        self.rx = netio.BatchReceiver(sock, max_msgs=_native.FLOWS_MAX_BATCH, slot_bytes=MAX_DATAGRAM, slots=2,
                                      device=self.device, with_sources=True)
        self._framer = ReliableUDP(codec_device=str(self.device))
        self._draw_isn = isn_source or (lambda: random.randint(1, 5000))
        self.flows: Dict[int, _Sending] = {}  # slot -> its message, ended ones until their linger is over
        self.resent = 0                       # timeouts that went back to a frame

    def __len__(self) -> int:
        """Messages neither done nor given up."""
        return sum(1 for f in self.flows.values() if f.closing is None)

    def submit(self, message: str, addr) -> int:
        """Queue ``message`` for ``addr`` (ip, port); returns its slot.  One
        transfer per peer at a time."""
        from . import netio
        from .batch import ack_flow_open
        key = netio.addr_key(*addr)
        slot = self.table.slot_of(key)
        if slot is not None:
            if self.flows[slot].closing is None:
                raise ValueError(f"a transfer to {addr} is still running")
            self._release(slot)
        slot = int(self.table.slots(np.array([key], np.uint64))[0])
        if slot == FLOW_NONE:
            raise RuntimeError(f"all {self.table.capacity} flow slots are taken")
        isn = self._draw_isn()
        frames, off = self._framer._gpu_frames(message, isn)
        ack_flow_open(self.states, slot, isn, len(message), CHUNK)
        self.flows[slot] = _Sending(key, slot, np.frombuffer(frames, np.uint8), np.asarray(off, np.int64),
                                    len(message), time.monotonic() + self.timeout)
        return slot

    def _release(self, slot: int) -> None:
        self.flows.pop(slot, None)
        self.table.release(slot)
        self.states[slot].zero_()  # an idle slot (ordered before the next batch's call)

    def _send_windows(self) -> None:
        """Every running flow's frames up to its window, in one sendmmsg; in
        cumulative mode the rows' ``sent`` first."""
        import torch
        from . import netio
        parts, lens, dst, sent = [], [], [], []
        for f in self.flows.values():
            if f.closing is not None:
                continue
            hi = min(-(-f.p // CHUNK) + self.window, f.rows)
            if f.nxt < hi:
                parts.append(f.frames[f.off[f.nxt]:f.off[hi]])
                lens.append(np.diff(f.off[f.nxt:hi + 1]))
                dst.append(np.full(hi - f.nxt, f.key, np.uint64))
                f.nxt = hi
                sent.append((f.slot, min(hi * CHUNK, f.T)))
        if not parts:
            return
        if self.mode == "cumulative":
            idx = torch.tensor([s for s, _ in sent], dtype=torch.int64).to(self.device, non_blocking=True)
            val = torch.tensor([v for _, v in sent], dtype=torch.int64).to(self.device, non_blocking=True)
            self.states[idx, 7] = val
        off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
        netio.send_batch_to(self.sock, np.concatenate(parts), off, np.concatenate(dst))

    def _timeouts(self, now: float, done) -> None:
        import torch
        from . import netio
        for f in list(self.flows.values()):
            if f.closing is not None:
                if now >= f.linger:
                    self._release(f.slot)
                continue
            if now < f.deadline:
                continue
            L = min(CHUNK, f.T - f.p)  # back to the frame at p, L and last recomputed from p (SEND_DATA)
            f.sends_left -= 1
            if f.sends_left < 1:
                done.append((netio.key_addr(f.key), False))
                self._release(f.slot)
                continue
            self.states[f.slot, :4] = torch.tensor([f.p, L, int(f.p + L == f.T), 0], dtype=torch.int64)
            f.nxt, f.deadline = -(-f.p // CHUNK), now + self.timeout
            self.resent += 1
            if f.T and f.p == f.T:  # everything is acknowledged but the FIN: the header-only FIN frame
                self.sock.sendto(f.frames[f.off[f.rows]:f.off[f.rows + 1]].tobytes(), netio.key_addr(f.key))

    def poll(self, timeout_ms: int = -1) -> List[Tuple[Tuple[str, int], bool]]:
        from . import netio
        done: List[Tuple[Tuple[str, int], bool]] = []
        self.sock.setblocking(True)
        self._send_windows()
        wait = timeout_ms
        if self.flows:
            due = min(f.deadline if f.closing is None else f.linger for f in self.flows.values())
            due_ms = int(max(0.0, due - time.monotonic()) * 1e3) + 1
            wait = due_ms if timeout_ms < 0 else min(timeout_ms, due_ms)
        n = self.rx.recv(timeout_ms=wait)
        if n:
            slots = self.table.lookup(self.rx.sources)
            lingering = [f for f in self.flows.values() if f.closing is not None]
            if lingering:  # a FIN from a peer whose flow has ended: the closing datagram again (read on the host)
                off, raw = self.rx.frame_off[:n + 1], self.rx.frames
                fin = np.array([off[i + 1] - off[i] >= 5 and bool(raw[off[i] + 4] & FIN) for i in range(n)])
                for f in lingering:
                    if (fin & (slots == f.slot)).any():
                        self.sock.sendto(f.closing, netio.key_addr(f.key))
            res, _, _ = self.rx.acknowledge_flows(slots, self.layout, states=self.states, mode=self.mode)
            rows = res.judged.flows()  # (the one wait per batch; the closing datagrams come with the same read)
            finals = dict(res.judged.finals())
            now = time.monotonic()
            for a in range(rows.shape[0]):
                slot, end, _, _, p, _, _, _ = (int(v) for v in rows[a])
                f = self.flows.get(slot)
                if f is None or f.closing is not None:
                    continue
                if p != f.p:
                    f.p, f.sends_left, f.deadline = p, MAX_SENDS, now + self.timeout
                if end < n:
                    f.closing, f.linger = finals[a], now + FLOW_LINGER_S
                    self.sock.sendto(f.closing, netio.key_addr(f.key))
                    done.append((netio.key_addr(f.key), True))
        self._timeouts(time.monotonic(), done)
        return done

    def run(self, timeout: Optional[float] = None) -> List[Tuple[Tuple[str, int], bool]]:
        """Poll until every submitted message is done or given up (or
        ``timeout`` seconds have passed); the ``(addr, ok)`` pairs in
        completion order."""
        out: List[Tuple[Tuple[str, int], bool]] = []
        stop = None if timeout is None else time.monotonic() + timeout
        while len(self):
            left = -1 if stop is None else int(max(0.0, stop - time.monotonic()) * 1e3)
            if stop is not None and left == 0:
                break
            out.extend(self.poll(left))
        return out
