"""A socket-free conversation between the protocol layer's sender and receivers.

The device calls are tested one by one elsewhere, each against inputs that a
generator describes.  Here the two halves meet: the frames the sender's calls
make are what a receiver judges, the replies the receiver's calls make are what
the sender judges, round after round until the transfer ends, with every
decision depending on what the other side said about the round before.

``Channel``   a pure function of (seed, scenario): what one side emitted in a
              round -> what the other side receives in it.  Loss, duplication,
              reordering inside the round, delay by one or two rounds, damage.
drivers       the host loops of rudp/transport.py and rudp/flows.py without
              sockets and timers (a round is a timer tick): ``Sender``,
              ``Receiver``, ``FlowSenders``, ``FlowReceivers``.  The same code
              for every backend.
backends      the judgement calls only.  ``RefBackend`` is the CPU references
              (segment_ref, decode_ref, accept_ref, receive_window_ref,
              receive_flows_ref, ack_ref, ack_flows_ref); ``DeviceBackend``
              ("chained" / "fused") is the library, its state kept on the
              device between rounds.
transcript    per round, every output of every call that the references
              define; ``compare`` names the first round, call and array at
              which two transcripts differ.
``SCENARIOS`` one table for the CPU and the GPU tests.

No torch at module level: the CPU tests import this file without a device.
"""
from __future__ import annotations

import random
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import ack_flows_ref
import receive_flows_ref
from accept_ref import ACK, FIN, SYN, accept_ref
from ack_ref import CUMULATIVE, EXACT, ack_ref, csum_of, header
from oracle import codec_np
from receive_window_ref import receive_window_ref
from segment_ref import segment_ref

C2S, S2C = "c2s", "s2c"           # sender -> receiver, receiver -> sender
SENDS = 3                         # timeouts without progress before the sender gives up (MAX_SENDS)
FIN_SENDS = 4                     # FIN|ACKs before the receiver stops waiting for the closing ACK (MAX_SENDS)
LINGER = 2                        # rounds an ended flow of FlowSenders keeps its slot (FLOW_LINGER_S)
MAX_BATCH = 1024                  # datagrams per call (a recvmmsg batch)
ALPHABET = "aé語😀"                # one character of every UTF-8 width


def text_of(seed, T: int) -> str:
    """T characters that mix the four UTF-8 widths."""
    rng = random.Random(f"text/{seed}/{T}")
    return "".join(rng.choice(ALPHABET) for _ in range(T))


def flags_of(d: bytes) -> int:
    return d[4] if len(d) >= 5 else 0


def parse_good(d: bytes, H: int) -> Optional[Tuple[int, int, int]]:
    """(seq, ack, flags) of a datagram the host loops read themselves (the
    closing handshake), None when it is short or, in rudp7, fails its checksum."""
    if len(d) < H:
        return None
    seq, ack, flags = int.from_bytes(d[0:2], "big"), int.from_bytes(d[2:4], "big"), d[4]
    if H == 7 and int.from_bytes(d[5:7], "big") != csum_of(seq, ack, flags, d[7:]):
        return None
    return seq, ack, flags


def pack(datagrams):
    off = np.zeros(len(datagrams) + 1, np.int64)
    np.cumsum([len(d) for d in datagrams], out=off[1:])
    return np.frombuffer(b"".join(datagrams), np.uint8).copy(), off


def split(buf, H: int, count: int) -> List[bytes]:
    raw = bytes(np.asarray(buf, np.uint8)[:H * count])
    return [raw[k * H:(k + 1) * H] for k in range(count)]


# ------------------------------------------------------------------- channel
class Channel:
    """What the wire does to one conversation.  ``carry(flow, direction, round,
    datagrams)`` returns what arrives in this round: the datagrams held back
    for it and those of the argument the channel lets through, ordered by a key
    that starts as the datagram's ordinal.

    Every decision is a function of (seed, flow, direction, the flow's datagram
    ordinal in that direction): a flow meets the same fate alone and among
    others.  ``rules[flow]`` is that flow's script, a list of (direction,
    match, action); a datagram no rule matches meets a random fault with
    probability ``p`` while the flow's ``budget`` lasts.  Once the rules and
    the budget are spent the channel is perfect.

    match   ("all",)             every datagram of the direction
            ("ord", k)           the k-th datagram of the direction
            ("round", r)         every datagram emitted in round r
            ("round_rest", r)    those but the first of them
            ("flag", mask, value, nth)  the nth (None: every) datagram whose
                                 flags & mask == value
    action  "lose", "dup" (a second copy right behind it), "swap" (it arrives
            a few places early), "reverse" (the later it left the earlier it
            arrives: a round of them arrives back to front), "delay1", "delay2", "dup_delay<n>" (a second
            copy n rounds later), and for rudp7 "flip" (one bit) and "cut"
            (below the header).

    A SYN-flagged datagram of the sender is never duplicated or delayed unless
    a rule says so: the reference's receive_data restarts on such a copy and
    the transfer cannot complete by design."""

    RANDOM5 = ("lose", "dup", "swap", "delay1", "delay2")
    RANDOM7 = RANDOM5 + ("flip", "cut")

    def __init__(self, seed, H: int, rules=None, p: float = 0.0, budget: int = 0):
        self.seed, self.H, self.p, self.budget0 = seed, H, p, budget
        self.rules = {f: list(r) for f, r in (rules or {}).items()}
        self.ordinal: Dict[tuple, int] = {}
        self.held: Dict[tuple, Dict[int, list]] = {}
        self.budget: Dict[int, int] = {}
        self.seen: Dict[tuple, int] = {}      # (flow, rule index) -> datagrams its flag matched so far
        self.faults = 0                       # faults applied (the round cap counts on them)

    def pending(self) -> bool:
        return any(v for h in self.held.values() for v in h.values())

    def _scripted(self, flow, direction, k, rnd, j, d):
        for at, (dirn, match, action) in enumerate(self.rules.get(flow, ())):
            if dirn != direction:
                continue
            kind = match[0]
            if kind == "all":
                hit = True
            elif kind == "ord":
                hit = k == match[1]
            elif kind == "round":
                hit = rnd == match[1]
            elif kind == "round_rest":
                hit = rnd == match[1] and j > 0
            else:
                hit = False
                if len(d) >= 5 and d[4] & match[1] == match[2]:
                    seen = self.seen.get((flow, at), 0)
                    self.seen[(flow, at)] = seen + 1
                    hit = match[3] is None or seen == match[3]
            if hit:
                return action
        return None

    def _decide(self, flow, direction, k, rnd, j, d):
        action = self._scripted(flow, direction, k, rnd, j, d)
        if action is not None:
            return action, random.Random(f"{self.seed}/{flow}/{direction}/{k}/scripted")
        left = self.budget.setdefault(flow, self.budget0)
        if self.p and left > 0:
            rng = random.Random(f"{self.seed}/{flow}/{direction}/{k}")
            if rng.random() < self.p:
                action = rng.choice(self.RANDOM7 if self.H == 7 else self.RANDOM5)
                if direction == C2S and flags_of(d) & SYN and action in ("dup", "swap", "delay1", "delay2"):
                    return None, rng
                self.budget[flow] = left - 1
                return action, rng
        return None, None

    def carry(self, flow, direction, rnd: int, datagrams) -> List[bytes]:
        key = (flow, direction)
        held = self.held.setdefault(key, {})
        out = held.pop(rnd, [])
        for j, d in enumerate(datagrams):
            k = self.ordinal.get(key, 0)
            self.ordinal[key] = k + 1
            action, rng = self._decide(flow, direction, k, rnd, j, d)
            if action is not None:
                self.faults += 1
            if action is None:
                out.append((float(k), d))
            elif action == "lose":
                pass
            elif action == "dup":
                out += [(float(k), d), (k + 0.5, d)]
            elif action == "swap":
                out.append((k - rng.uniform(1.25, 3.75), d))
            elif action == "reverse":
                out.append((float(-k), d))
            elif action in ("delay1", "delay2"):
                held.setdefault(rnd + int(action[-1]), []).append((float(k), d))
            elif action.startswith("dup_delay"):
                out.append((float(k), d))
                held.setdefault(rnd + int(action[9:]), []).append((float(k), d))
            elif action == "flip":
                bit = rng.randrange(8 * len(d))
                out.append((float(k), d[:bit // 8] + bytes([d[bit // 8] ^ (1 << bit % 8)]) + d[bit // 8 + 1:]))
            elif action == "cut":
                out.append((float(k), d[:rng.randrange(self.H)]))
            else:
                raise ValueError(action)
        out.sort(key=lambda t: t[0])
        return [d for _, d in out]

    def merge(self, direction, rnd: int, per_flow: Dict[int, List[bytes]]) -> List[Tuple[int, bytes]]:
        """One arrival order out of every flow's datagrams, each flow keeping its own."""
        pick = [f for f in sorted(per_flow) for _ in per_flow[f]]
        random.Random(f"{self.seed}/merge/{direction}/{rnd}").shuffle(pick)
        at = {f: 0 for f in per_flow}
        out = []
        for f in pick:
            out.append((f, per_flow[f][at[f]]))
            at[f] += 1
        return out


# ---------------------------------------------------------------- transcript
def norm(a) -> np.ndarray:
    """Any table as int64 [*] of its unsigned values (a device int32 that holds
    a u32 and the reference's u32 compare equal)."""
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), np.uint8)
    a = np.asarray(a)
    if a.dtype.kind == "i" and a.dtype.itemsize < 8:
        return a.astype(np.int64).ravel() & ((1 << 8 * a.dtype.itemsize) - 1)
    return a.astype(np.int64).ravel()


class Transcript:
    """rounds[r] is the list of (call, {array name: int64 array}) of round r."""

    def __init__(self):
        self.rounds: List[list] = []

    def begin(self):
        self.rounds.append([])

    def add(self, call: str, arrays: dict):
        self.rounds[-1].append((call, {k: norm(v) for k, v in arrays.items()}))

    def __len__(self):
        return len(self.rounds)


def compare(want: Transcript, got: Transcript, need=None) -> None:
    """Raise AssertionError naming the first round, call and array at which
    ``got`` differs from ``want``.  ``got`` may record fewer arrays of a call
    (a chained form returns fewer tables), but at least ``need[call]``."""
    for r, (w_calls, g_calls) in enumerate(zip(want.rounds, got.rounds)):
        names = ([c for c, _ in w_calls], [c for c, _ in g_calls])
        assert names[0] == names[1], f"round {r}: calls {names[1]} where the transcript has {names[0]}"
        for k, ((call, w), (_, g)) in enumerate(zip(w_calls, g_calls)):
            extra = set(g) - set(w)
            assert not extra, f"round {r}, call {k} ({call}): arrays {sorted(extra)} the transcript does not define"
            missing = set((need or {}).get(call, ())) - set(g)
            assert not missing, f"round {r}, call {k} ({call}): arrays {sorted(missing)} are not recorded"
            for name in g:
                if not np.array_equal(w[name], g[name]):
                    raise AssertionError(f"round {r}, call {k} ({call}), array {name}: got {g[name][:16].tolist()} "
                                         f"({len(g[name])} entries), the transcript has {w[name][:16].tolist()} "
                                         f"({len(w[name])})")
    assert len(got) == len(want), f"{len(got)} rounds where the transcript has {len(want)}"


# ------------------------------------------------------------- CPU backend
def _reply_peer(seq, flags, usable, reply, last_isn):
    n, idx, peer, reset = len(seq), [], [], len(seq)
    for i in range(n):
        if usable[i] and flags[i] & SYN and int(seq[i]) != (-1 if last_isn is None else last_isn):
            reset = i
        if reply[i]:
            idx.append(i)
            peer.append(reset)
    return idx, peer


class RefBackend:
    """The judgement calls on the CPU references.  ``accept``, ``ack`` and
    ``flows`` are the rules, replaceable (the wrong-backend tests)."""
    name = "ref"
    accept = staticmethod(accept_ref)
    ack = staticmethod(ack_ref)
    window_rule = None        # None: receive_window_ref's own (window_ref)

    # ---- sender: frames
    def frames(self, message: str, isn: int, C: int, H: int):
        """Rows 0..rows-1, and with T > 0 the header-only FIN row of a late resend."""
        raw = message.encode()
        seg = segment_ref(raw, C, isn)
        seq, ack, flags = seg.seq, seg.ack, seg.flags
        pay = [raw[int(seg.payload_off[k]):int(seg.payload_off[k + 1])] for k in range(seg.packets)]
        if message:
            seq = np.append(seq, np.uint16((isn + len(message)) & 0xFFFF))
            ack, flags, pay = np.append(ack, np.uint16(0)), np.append(flags, np.uint8(FIN)), pay + [b""]
        fr, off, _ = codec_np.encode_varlen(seq, ack, flags, pay, H)
        fr = fr.tobytes()
        return [fr[int(off[k]):int(off[k + 1])] for k in range(len(pay))], {"frames": fr, "frame_off": off}

    def header(self, seq: int, ack: int, flags: int, H: int) -> bytes:
        return header(seq & 0xFFFF, ack & 0xFFFF, flags, H)

    # ---- single peer, in-order receiver
    def rx_inorder(self, dgrams, state, last_isn, H):
        frames, off = pack(dgrams)
        n = len(dgrams)
        seq, ack, flags, ok, csum, valid, usable, chars = receive_flows_ref.decode_ref(frames, off, H)
        r = self.accept(seq, flags, chars, usable, state or (0, 0, 0), last_isn)
        idx, peer = _reply_peer(seq, flags, usable, r.reply, last_isn)
        rframes, rcsum = receive_flows_ref.header_frames(r.reply_ack[idx], ACK, H)
        piece = b"".join(dgrams[i][H:] for i in np.flatnonzero(r.keep))
        rec = dict(seq=seq, ack=ack, flags=flags, ok=ok, csum=csum, valid=valid, usable=usable, chars=chars,
                   accept=r.accept, keep=r.keep, reply=r.reply, reply_ack=r.reply_ack,
                   state=[r.state[0], r.state[1], 1 if r.state[2] else 0],
                   info=[r.end, r.count, r.msg_start, r.characters, len(idx), len(piece)], payload=piece,
                   reply_frames=rframes, reply_csum=rcsum, reply_index=idx, reply_peer=peer)
        return SimpleNamespace(rec=rec, state=r.state, carried=None, n=n, n_carried=0, end=r.end,
                               msg_start=r.msg_start, replies=split(np.frombuffer(rframes, np.uint8), H, len(idx)),
                               piece=piece, isn=lambda: r.state[1])

    # ---- single peer, reordering receiver
    def rx_window(self, dgrams, carried, state, last_isn, H, window_chars):
        frames, off = pack(dgrams)
        cfr, coff = carried if carried is not None else (np.zeros(0, np.uint8), None)
        kw = {} if self.window_rule is None else {"rule": self.window_rule}
        d = receive_window_ref(cfr, coff, frames, off, H, window_chars=window_chars, state=state or (0, 0, 0),
                               last_isn=last_isn, **kw)
        m = 0 if coff is None else len(coff) - 1
        info = d["info"]
        rec = {k: d[k] for k in ("seq", "ack", "flags", "ok", "valid", "usable", "chars", "accept", "rank",
                                 "carry_rank", "reply", "reply_ack", "payload", "payload_off", "payload_src",
                                 "carry_frames", "carry_off", "reply_frames", "reply_csum", "reply_index",
                                 "reply_peer")}
        rec.update(csum=d["csum_out"], state=d["state"][:3], status=[d["status"]],
                   info=info[:4] + info[5:7] + info[8:11])
        # (reply_index and reply_peer count in new-frame indices, as the wrappers return them)
        rec["reply_index"] = np.asarray(d["reply_index"], np.int64) - m
        peer = np.asarray(d["reply_peer"], np.int64)
        rec["reply_peer"] = np.where(peer >= m + len(dgrams), len(dgrams), peer - m)
        return SimpleNamespace(rec=rec, state=tuple(d["state"][:3]), n=m + len(dgrams), n_carried=m, end=info[0],
                               carried=(np.asarray(d["carry_frames"], np.uint8), np.asarray(d["carry_off"], np.int64)),
                               msg_start=info[2], replies=split(d["reply_frames"], H, d["R"]),
                               piece=bytes(np.asarray(d["payload"], np.uint8)), isn=lambda: d["state"][1])

    # ---- single peer, sender
    def tx_ack(self, dgrams, state, *, isn, T, C, mode, sent, H):
        frames, off = pack(dgrams)
        n = len(dgrams)
        seq, ack, flags, ok, csum, _, _, _ = receive_flows_ref.decode_ref(frames, off, H)
        usable = ((ok == 1) | (ok == 3)).astype(np.uint8)
        r = self.ack(seq, ack, flags, usable, isn=isn, T=T, C=C, state=state, mode=mode,
                     sent=sent if mode == CUMULATIVE else None)
        p = r.state[0]
        final = self.header(r.final[0], r.final[1], ACK, H) if r.final else b""
        rec = dict(seq=seq, ack=ack, flags=flags, ok=ok, csum=csum, usable=usable, valid=r.valid, pointer=r.pointer,
                   state=list(r.state), info=[r.end, r.count, r.newly, p, -(-p // C), r.done], final_frame=final)
        return SimpleNamespace(rec=rec, state=r.state, done=bool(r.done), pointer_after=p, final=final)

    # ---- many peers, receiver
    def rx_table(self, n_flows: int):
        return np.zeros((n_flows, 4), np.uint64)

    def rx_release(self, table, slot: int):
        table[slot] = 0

    def table_host(self, table):
        return np.asarray(table).copy()

    def flows(self, frames, off, flow, table, H):
        return receive_flows_ref.receive_flows_ref(frames, off, flow, table, H)

    def rx_flows(self, dgrams, slots, table, H):
        frames, off = pack(dgrams)
        r = self.flows(frames, off, np.asarray(slots, np.uint32), table, H)
        f = r.flows
        table[:] = f.states
        A, K, R, E = f.info[0], f.info[1], f.info[2], f.info[3]
        rec = dict(seq=r.seq, ack=r.ack, flags=r.flags, ok=r.ok, csum=r.csum, valid=r.valid, usable=r.usable,
                   chars=r.chars, accept=f.accept, keep=f.keep, reply=f.reply, reply_ack=f.reply_ack, rank=f.rank,
                   order=f.order, order_off=f.order_off, flow_info=f.flow_info, info=f.info[:5] + [r.info[8]],
                   status=[r.status], payload=r.payload, payload_off=r.payload_off, payload_src=r.payload_src,
                   reply_frames=r.reply_frames, reply_csum=r.reply_csum, reply_index=r.reply_index,
                   fin_frames=r.fin_frames, fin_csum=r.fin_csum, fin_flow=r.fin_flow, table=table)
        poff = [int(v) for v in r.payload_off]
        rows = np.asarray(f.flow_info, np.int64).reshape(A, 8)
        pieces = [r.payload[poff[int(row[7])]:poff[int(row[7]) + int(row[6])]] for row in rows]
        return SimpleNamespace(rec=rec, rows=rows, pieces=pieces, reply_index=[int(i) for i in r.reply_index],
                               replies=split(np.frombuffer(r.reply_frames, np.uint8), H, R),
                               fins=dict(zip([int(a) for a in r.fin_flow],
                                             split(np.frombuffer(r.fin_frames, np.uint8), H, E))),
                               seq=r.seq, ack=r.ack, flags=r.flags, usable=r.usable)

    # ---- many peers, sender
    def tx_table(self, n_flows: int):
        return np.zeros((n_flows, 8), np.uint64)

    def tx_open(self, table, slot, isn, T, C):
        table[slot] = ack_flows_ref.open_row(isn, T, C)

    def tx_sent(self, table, pairs):
        for slot, sent in pairs:
            table[slot, 7] = sent

    def tx_rewind(self, table, slot, state):
        table[slot, :4] = state

    def tx_release(self, table, slot):
        table[slot] = 0

    def tx_flows(self, dgrams, slots, table, mode, H):
        frames, off = pack(dgrams)
        seq, ack, flags, ok, csum, _, _, _ = receive_flows_ref.decode_ref(frames, off, H)
        usable = ((ok == 1) | (ok == 3)).astype(np.uint8)
        r = ack_flows_ref.ack_flows_ref(seq, ack, flags, usable, np.asarray(slots, np.uint32), table, mode)
        table[:] = r.states
        finals = {a: self.header(s, k, ACK, H) for a, s, k in r.finals}
        rec = dict(seq=seq, ack=ack, flags=flags, ok=ok, usable=usable, valid=r.valid, pointer=r.pointer, order=r.order,
                   order_off=r.order_off, flow_info=r.flow_info, info=r.info, status=[r.status],
                   final_frames=b"".join(finals[a] for a in sorted(finals)), final_flow=sorted(finals), table=table)
        return SimpleNamespace(rec=rec, rows=np.asarray(r.flow_info, np.int64).reshape(-1, 8), finals=finals)


# ------------------------------------------------------------ device backend
class DeviceBackend:
    """The judgement calls on the library.  ``form``: "chained" (receive_batch,
    receive_window, receive_flows, unpack_batch_varlen -> ack_progress) or
    "fused" (receive, receive_windowed, receive_flows_fused, acknowledge); the
    many-peer sender is acknowledge_flows in both.  The state a call returns is
    the tensor the next call takes, the carried frames stay on the device and
    the flow tables are updated in place; what is copied to the host here is
    what the transcript records and what the real loops read."""

    # what every form records at least (compare()'s ``need``)
    NEED = {
        "receive": ("accept", "keep", "reply", "reply_ack", "state", "info", "payload", "reply_frames"),
        "receive_window": ("accept", "rank", "carry_rank", "reply", "reply_ack", "state", "info", "payload",
                           "carry_frames", "carry_off", "reply_frames", "reply_index", "reply_peer"),
        "receive_flows": ("seq", "ack", "flags", "ok", "valid", "usable", "chars", "accept", "keep", "reply",
                          "reply_ack", "rank", "order", "order_off", "flow_info", "info", "payload", "reply_frames",
                          "reply_index", "fin_frames", "table"),
        "acknowledge": ("seq", "ack", "flags", "ok", "usable", "valid", "pointer", "state", "info", "final_frame"),
        "acknowledge_flows": ("seq", "ack", "flags", "ok", "usable", "valid", "pointer", "order", "order_off",
                              "flow_info", "info", "status", "final_frames", "final_flow", "table"),
        "frames": ("frames", "frame_off"),
    }

    PAD, SENT = 512, 0xA5     # sentinel bytes on either side of every output allocation

    def __init__(self, form: str, device, stream=None):
        assert form in ("chained", "fused")
        self.name, self.fused, self.dev, self.stream = form, form == "fused", device, stream
        self.guarded = 0      # library calls whose output allocations lay between sentinels

    def _on_stream(self):
        import contextlib
        import torch
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _between_sentinels(self, call: str, need: int):
        """While the context lasts, every device allocation the wrappers make
        for their outputs -- ``torch.empty(n, dtype=..., device=...)`` (the one
        buffer of a fused call, all its tables views of it; the accept and
        ack buffers and ``payload_chars``' table of the chains) and
        ``tensor.new_empty(n)`` (the chains' decode and gather outputs) -- is
        cut out of a larger one filled with sentinel bytes, and on leaving, the
        bytes on either side must be as they were.  PAD keeps the allocator's
        alignment.  The call must have made at least ``need`` such allocations
        of more than zero bytes (the number the wrapper makes today for a batch
        that is not empty): a wrapper that comes to allocate in a way these two
        patches do not see fails here instead of losing its guard unnoticed.

        Not guarded: the tables inside one allocation against each other (the
        per-call tests do that, through the C ABI with a buffer per table);
        what the wrappers make with ``torch.zeros`` / ``zeros_like`` /
        ``torch.full`` / ``torch.cat`` (reply header tables, the joined carried
        and new frames of ``receive_window``, an empty batch's buffer); the
        state tables the calls update in place; and everything this file
        allocates itself (the uploads, ``_headers``' frames)."""
        import contextlib
        import torch

        @contextlib.contextmanager
        def guard():
            real_empty, real_new, made, PAD, SENT = torch.empty, torch.Tensor.new_empty, [], self.PAD, self.SENT

            def cut(n, dtype, dev):
                nbytes = n * torch.empty(0, dtype=dtype).element_size()
                big = torch.full((nbytes + 2 * PAD,), SENT, dtype=torch.uint8, device=dev)
                made.append((big, nbytes))
                return big[PAD:PAD + nbytes].view(dtype)

            def size_of(size):
                if len(size) == 1 and isinstance(size[0], (tuple, list)):
                    size = tuple(size[0])
                return size[0] if len(size) == 1 and isinstance(size[0], int) and not isinstance(size[0], bool) else None

            def empty(*size, **kw):
                n, dev = size_of(size), kw.get("device")
                if n is not None and dev is not None and torch.device(dev).type == "cuda" and "dtype" in kw \
                        and set(kw) == {"dtype", "device"}:
                    return cut(n, kw["dtype"], dev)
                return real_empty(*size, **kw)

            def new_empty(t, *size, **kw):
                n = size_of(size)
                if n is not None and t.device.type == "cuda" and not kw:
                    return cut(n, t.dtype, t.device)
                return real_new(t, *size, **kw)
            torch.empty, torch.Tensor.new_empty = empty, new_empty
            try:
                yield
            finally:
                torch.empty, torch.Tensor.new_empty = real_empty, real_new
            for big, n in made:
                with self._on_stream():
                    edges = torch.cat((big[:PAD], big[PAD + n:])).cpu().numpy()
                assert (edges == SENT).all(), f"{call} wrote outside its {n}-byte output allocation"
            sizes = [n for _, n in made if n > 0]
            assert len(sizes) >= need, f"{call}: {len(sizes)} guarded output allocations {sizes}, {need} expected"
            self.guarded += 1
        return guard()

    def _up(self, dgrams):
        import torch
        frames, off = pack(dgrams)
        with self._on_stream():
            return (torch.from_numpy(frames).to(self.dev) if len(frames)
                    else torch.empty(0, dtype=torch.uint8, device=self.dev)), torch.from_numpy(off).to(self.dev)

    def _headers(self, seq, ack, flags: int, H: int):
        """Header-only frames of device u16 tables, framed by the library."""
        import torch
        from rudp import batch
        R = seq.shape[0]
        empty = torch.empty(0, dtype=torch.uint8, device=self.dev)
        if R == 0:
            return empty
        tab = (seq, ack, torch.full((R,), flags, dtype=torch.uint8, device=self.dev))
        return batch.pack_batch_varlen(tab, empty, torch.zeros(R, dtype=torch.int32, device=self.dev), H,
                                       want_csum=False, check=False).frames

    def header(self, seq: int, ack: int, flags: int, H: int) -> bytes:
        import torch
        with self._on_stream():
            t = torch.from_numpy(np.array([seq & 0xFFFF, ack & 0xFFFF], np.uint16)).to(self.dev)
            return self._headers(t[0:1], t[1:2], flags, H).cpu().numpy().tobytes()

    # ---- sender: frames (ReliableUDP._gpu_frames, for either layout)
    def frames(self, message: str, isn: int, C: int, H: int):
        import torch
        from rudp import batch
        with self._on_stream():
            seg = batch.segment_message(message, isn, chunk=C, device=self.dev, check=False)
            tab = seg.table()
            seq, ack, flags, lens = tab.headers.seq, tab.headers.ack, tab.headers.flags, tab.lengths
            if message:
                def append(col, value, dtype):
                    row = torch.from_numpy(np.array([value], dtype).view(np.uint8)).to(self.dev)
                    return torch.cat((col.view(torch.uint8), row)).view(col.dtype)
                seq = append(seq, (isn + len(message)) & 0xFFFF, np.uint16)
                ack = append(ack, 0, np.uint16)
                flags = append(flags, FIN, np.uint8)
                lens = append(lens, 0, np.int32)
            res = batch.pack_batch_varlen((seq, ack, flags), seg.payload, lens, H, want_csum=False)
            fr, off = res.frames.cpu().numpy().tobytes(), res.frame_off.cpu().numpy()
        return [fr[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)], {"frames": fr, "frame_off": off}

    # ---- single peer, in-order receiver
    def rx_inorder(self, dgrams, state, last_isn, H):
        import torch
        from rudp import batch
        frames, off = self._up(dgrams)
        n = len(dgrams)
        if self.fused:
            with self._between_sentinels("receive", 1):
                res = batch.receive(frames, off, H, state=state, last_isn=last_isn, stream=self.stream)
            acc, R, nbytes = res.accepted, res.reply_count, res.message_bytes
            with self._on_stream():
                piece = res.message.payload.cpu().numpy().tobytes() if nbytes else b""
                rframes = res.reply_frames[:H * R].cpu().numpy()
                rec = {k: getattr(res, k).cpu().numpy() for k in ("seq", "ack", "flags", "ok", "csum", "valid",
                                                                   "usable", "chars")}
                rec.update(reply_csum=res.reply_csum[:R].cpu().numpy(), reply_index=res.reply_index[:R].cpu().numpy(),
                           reply_peer=res.reply_peer[:R].cpu().numpy())
        else:
            with self._on_stream():
                with self._between_sentinels("receive_batch", 4):
                    res = batch.receive_batch(frames, off, H, state=state, last_isn=last_isn)
                acc = res.accepted
                idx = torch.nonzero(acc.reply).flatten()
                acks = acc.reply_ack.view(torch.int16)[idx].view(torch.uint16)
                R = int(idx.shape[0])
                rframes = self._headers(torch.zeros_like(acks), acks, ACK, H).cpu().numpy()
                piece = res.message.payload.cpu().numpy().tobytes()
                rec = dict(reply_index=idx.cpu().numpy())
        with self._on_stream():
            rec.update(accept=acc.accept.cpu().numpy(), keep=acc.keep.cpu().numpy(), reply=acc.reply.cpu().numpy(),
                       reply_ack=acc.reply_ack.cpu().numpy(), state=acc.state.cpu().numpy()[:3],
                       info=[acc.end, acc.count, acc.msg_start, acc.characters, R, len(piece)], payload=piece,
                       reply_frames=rframes)
        return SimpleNamespace(rec=rec, state=acc.state, carried=None, n=n, n_carried=0, end=acc.end,
                               msg_start=acc.msg_start, replies=split(rframes, H, R), piece=piece,
                               isn=lambda: int(acc.state[1].item()))

    # ---- single peer, reordering receiver
    def rx_window(self, dgrams, carried, state, last_isn, H, window_chars):
        from rudp import batch
        frames, off = self._up(dgrams)
        call = batch.receive_windowed if self.fused else batch.receive_window
        with self._between_sentinels(call.__name__, 1 if self.fused else 5):
            res = call(frames, off, H, window_chars=window_chars, carried=carried, state=state, last_isn=last_isn,
                       stream=self.stream)
        acc, m = res.accepted, res.n_carried
        R = res.reply_count
        with self._on_stream():
            K, nbytes = res.message.total
            car = res.carried
            P, cbytes = car.count, car.nbytes
            rframes = (res.reply_frames if self.fused else res.reply_frames(H)).cpu().numpy()
            piece = res.message.payload.cpu().numpy().tobytes()
            rec = dict(accept=acc.accept.cpu().numpy(), rank=acc.rank.cpu().numpy(),
                       carry_rank=acc.carry_rank.cpu().numpy(), reply=acc.reply.cpu().numpy(),
                       reply_ack=acc.reply_ack.cpu().numpy(), state=acc.state.cpu().numpy()[:3],
                       info=[acc.end, acc.count, acc.msg_start, acc.characters, acc.pending, acc.delivered, R, nbytes,
                             cbytes],
                       payload=piece, payload_off=res.message.out_off[:K + 1].cpu().numpy(),
                       payload_src=res.message.src[:K].cpu().numpy(), carry_frames=car.frames[:cbytes].cpu().numpy(),
                       carry_off=car.frame_off[:P + 1].cpu().numpy(), reply_frames=rframes,
                       reply_index=res.reply_index.cpu().numpy(), reply_peer=res.reply_peer.cpu().numpy())
            if self.fused:
                rec.update({k: getattr(res, k).cpu().numpy() for k in ("seq", "ack", "flags", "ok", "csum", "valid",
                                                                        "usable", "chars")})
                rec.update(reply_csum=res.reply_csum.cpu().numpy(), status=res.status.cpu().numpy())
        return SimpleNamespace(rec=rec, state=res.state, carried=car, n=m + len(dgrams), n_carried=m, end=acc.end,
                               msg_start=acc.msg_start, replies=split(rframes, H, R), piece=piece,
                               isn=lambda: int(res.state[1].item()))

    # ---- single peer, sender
    def tx_ack(self, dgrams, state, *, isn, T, C, mode, sent, H):
        import torch
        from rudp import _native, batch
        frames, off = self._up(dgrams)
        kw = dict(isn=isn, total_chars=T, chunk=C, state=state, mode=mode, sent=sent)
        if self.fused:
            with self._between_sentinels("acknowledge", 1):
                res = batch.acknowledge(frames, off, H, stream=self.stream, **kw)
            dec, usable = res, res.usable
        else:
            with self._between_sentinels("unpack_batch_varlen -> ack_progress", 2):
                with self._on_stream():
                    dec = batch.unpack_batch_varlen(frames, off, H, check=False)
                    usable = ((dec.ok == _native.OK_GOOD) | (dec.ok == _native.OK_UNVERIFIED)).to(torch.uint8)
                res = batch.ack_progress(dec.seq, dec.ack, dec.flags, usable=usable, stream=self.stream, **kw)
        done, p = res.done, res.pointer_after
        final = b""
        with self._on_stream():
            if done and self.fused:
                final = res.final_frame.cpu().numpy().tobytes()
            elif done:  # the chain has no call for the closing datagram: send_ack's, framed by the library
                seq16 = dec.seq.view(torch.int16)[res.end:res.end + 1].to(torch.int32)
                ack1 = ((seq16 + 1) & 0xFFFF).to(torch.int16).view(torch.uint16)
                mine = torch.from_numpy(np.array([(isn + p) & 0xFFFF], np.uint16)).to(self.dev)
                final = self._headers(mine, ack1, ACK, H).cpu().numpy().tobytes()
            rec = dict(seq=dec.seq.cpu().numpy(), ack=dec.ack.cpu().numpy(), flags=dec.flags.cpu().numpy(),
                       ok=dec.ok.cpu().numpy(), csum=dec.csum.cpu().numpy(), usable=usable.cpu().numpy(),
                       valid=res.valid.cpu().numpy(), pointer=res.pointer.cpu().numpy(), state=res.state.cpu().numpy(),
                       info=[res.end, res.count, res.newly_acknowledged, p, res.next_frame, int(done)],
                       final_frame=final)
        return SimpleNamespace(rec=rec, state=res.state, done=done, pointer_after=p, final=final)

    # ---- many peers, receiver
    def rx_table(self, n_flows: int):
        from rudp import batch
        with self._on_stream():
            return batch.flow_states(n_flows, self.dev)

    def rx_release(self, table, slot: int):
        with self._on_stream():
            table[slot].zero_()

    def table_host(self, table):
        with self._on_stream():
            return table.cpu().numpy().copy()

    def rx_flows(self, dgrams, slots, table, H):
        import torch
        from rudp import batch
        frames, off = self._up(dgrams)
        n = len(dgrams)
        with self._on_stream():
            flow = torch.from_numpy(np.asarray(slots, np.uint32).view(np.int32).copy()).to(self.dev)
        if self.fused:
            with self._between_sentinels("receive_flows_fused", 1):
                res = batch.receive_flows_fused(frames, off, flow, H, states=table, stream=self.stream)
            rows = res.flows().copy()
            A, K, R, E = res.active, res.kept, res.replies, res.ended
            h = res.host
            rec = {k: h(k) for k in ("seq", "ack", "flags", "ok", "csum", "valid", "usable", "chars", "accept", "keep",
                                     "reply", "reply_ack", "rank", "order")}
            nbytes = res.message_bytes
            rec.update(order_off=h("order_off")[:A + 1], flow_info=rows, info=h("info")[:5] + [nbytes],
                       status=h("status")[:1], payload=h("payload")[:nbytes], payload_off=h("payload_off")[:K + 1],
                       payload_src=h("payload_src")[:K], reply_frames=h("reply_frames")[:R * H],
                       reply_csum=h("reply_csum")[:R], reply_index=h("reply_index")[:R],
                       fin_frames=h("fin_frames")[:E * H], fin_csum=h("fin_csum")[:E], fin_flow=h("fin_flow")[:E])
            pieces = [res.message(a) for a in range(A)]
            fins = dict(zip(rec["fin_flow"].tolist(), split(rec["fin_frames"], H, E)))
            host = {k: rec[k] for k in ("seq", "ack", "flags", "usable")}
        else:
            with self._between_sentinels("receive_flows", 4):
                res = batch.receive_flows(frames, off, flow, H, states=table, stream=self.stream)
            acc, dec = res.accepted, res.decoded
            rows = acc.flows().copy()
            A, K = acc.active, acc.kept
            with self._on_stream():
                pieces = [res.message(a) for a in range(A)]
                rec = dict(seq=dec.seq.cpu().numpy(), ack=dec.ack.cpu().numpy(), flags=dec.flags.cpu().numpy(),
                           ok=dec.ok.cpu().numpy(), csum=dec.csum.cpu().numpy(), valid=dec.valid.cpu().numpy(),
                           usable=res.usable.cpu().numpy(), chars=res.chars.cpu().numpy(),
                           accept=acc.accept.cpu().numpy(), keep=acc.keep.cpu().numpy(), reply=acc.reply.cpu().numpy(),
                           reply_ack=acc.reply_ack.cpu().numpy(), rank=acc.rank.cpu().numpy(),
                           order=acc.order.cpu().numpy(), order_off=acc.order_off[:A + 1].cpu().numpy(), flow_info=rows,
                           status=acc.status.cpu().numpy(), payload=b"".join(pieces),
                           payload_off=res.pieces.out_off[:K + 1].cpu().numpy(),
                           payload_src=res.pieces.src[:K].cpu().numpy(),
                           reply_frames=res.reply_frames(H).cpu().numpy(), reply_index=res.reply_index.cpu().numpy())
                rec["info"] = [A, K, acc.replies, acc.ended, acc.flowless, len(rec["payload"])]
                # FlowReceiver builds the FIN|ACK of an ended flow on the host: isn + characters
                ended = [a for a in range(A) if int(rows[a][1]) < n]
                acks = np.array([(int(rows[a][5]) + int(rows[a][4])) & 0xFFFF for a in ended], np.uint16)
                ff = self._headers(torch.zeros(len(ended), dtype=torch.int16, device=self.dev).view(torch.uint16),
                                   torch.from_numpy(acks).to(self.dev), FIN | ACK, H).cpu().numpy()
                rec.update(fin_frames=ff, fin_flow=ended)
            fins = dict(zip(ended, split(ff, H, len(ended))))
            host = {k: rec[k] for k in ("seq", "ack", "flags", "usable")}
        R = len(rec["reply_index"])
        rec["table"] = self.table_host(table)
        return SimpleNamespace(rec=rec, rows=np.asarray(rows, np.int64), pieces=pieces,
                               reply_index=[int(i) for i in rec["reply_index"]],
                               replies=split(rec["reply_frames"], H, R), fins=fins, **host)

    # ---- many peers, sender
    def tx_table(self, n_flows: int):
        from rudp import batch
        with self._on_stream():
            return batch.ack_flow_states(n_flows, self.dev)

    def tx_open(self, table, slot, isn, T, C):
        from rudp import batch
        with self._on_stream():
            batch.ack_flow_open(table, slot, isn, T, C)

    def tx_sent(self, table, pairs):
        import torch
        with self._on_stream():
            idx = torch.tensor([s for s, _ in pairs], dtype=torch.int64).to(self.dev)
            table[idx, 7] = torch.tensor([v for _, v in pairs], dtype=torch.int64).to(self.dev)

    def tx_rewind(self, table, slot, state):
        import torch
        with self._on_stream():
            table[slot, :4] = torch.tensor([int(v) for v in state], dtype=torch.int64).to(self.dev)

    def tx_release(self, table, slot):
        with self._on_stream():
            table[slot].zero_()

    def tx_flows(self, dgrams, slots, table, mode, H):
        import torch
        from rudp import batch
        frames, off = self._up(dgrams)
        with self._on_stream():
            flow = torch.from_numpy(np.asarray(slots, np.uint32).view(np.int32).copy()).to(self.dev)
        with self._between_sentinels("acknowledge_flows", 2):
            res = batch.acknowledge_flows(frames, off, flow, H, states=table, mode=mode, stream=self.stream)
        j, dec = res.judged, res.decoded
        rows = j.flows().copy()
        finals = dict(j.finals())
        A = j.active
        with self._on_stream():
            rec = dict(seq=dec.seq.cpu().numpy(), ack=dec.ack.cpu().numpy(), flags=dec.flags.cpu().numpy(),
                       ok=dec.ok.cpu().numpy(), usable=res.usable.cpu().numpy(), valid=j.valid.cpu().numpy(),
                       pointer=j.pointer.cpu().numpy(), order=j.order.cpu().numpy(),
                       order_off=j.order_off[:A + 1].cpu().numpy(), flow_info=rows,
                       info=[A, j.count, j.ended, j.newly_acknowledged, j.flowless], status=j.status.cpu().numpy(),
                       final_frames=b"".join(finals[a] for a in sorted(finals)), final_flow=sorted(finals),
                       table=self.table_host(table))
        return SimpleNamespace(rec=rec, rows=np.asarray(rows, np.int64), finals=finals)


# ------------------------------------------------------------------- drivers
class Sender:
    """ReliableUDP._transmit_window without sockets: fill the window, judge the
    round's replies, an empty round is a timeout."""

    def __init__(self, be, message: str, isn: int, C: int, W: int, mode: str, H: int, log: Transcript):
        self.be, self.isn, self.C, self.W, self.mode, self.H, self.log = be, isn, C, W, mode, H, log
        self.T = len(message)
        self.rows = max(-(-self.T // C), 1)
        self.table, rec = be.frames(message, isn, C, H)
        self.frames_rec = rec
        self.p, self.nxt, self.sends_left, self.state = 0, 0, SENDS, None
        self.outbox: List[bytes] = []
        self.finished: Optional[str] = None   # "done" or "gave up"
        self.finished_round: Optional[int] = None
        self.pointers: List[int] = []         # p after every round

    def emit(self) -> List[bytes]:
        out, self.outbox = self.outbox, []
        if self.finished is None:
            hi = min(-(-self.p // self.C) + self.W, self.rows)
            if self.nxt < hi:
                out = out + self.table[self.nxt:hi]
                self.nxt = hi
        return out

    def judge(self, replies: List[bytes], rnd: int) -> None:
        if self.finished is None:
            self._judge(replies)
            if self.finished is not None:
                self.finished_round = rnd
        self.pointers.append(self.p)

    def _judge(self, replies):
        T, C, p = self.T, self.C, self.p
        if not replies:  # timeout: back to the frame at p, L and last recomputed from p (SEND_DATA)
            L = min(C, T - p)
            self.sends_left -= 1
            self.log.add("timeout", dict(p=[p], sends_left=[self.sends_left]))
            if self.sends_left < 1:
                self.finished = "gave up"
                return
            self.state, self.nxt = (p, L, int(p + L == T), 0), -(-p // C)
            if T and p == T:
                self.outbox.append(self.table[self.rows])
            return
        for at in range(0, len(replies), MAX_BATCH):
            res = self.be.tx_ack(replies[at:at + MAX_BATCH], self.state, isn=self.isn, T=T, C=C, mode=self.mode,
                                 sent=min(self.nxt * C, T), H=self.H)
            self.log.add("acknowledge", res.rec)
            self.state = res.state
            if res.done:
                self.outbox.append(res.final)
                self.closing = res.final
                self.p, self.finished = res.pointer_after, "done"
                return
            if res.pointer_after != self.p:
                self.p, self.sends_left = res.pointer_after, SENDS


class Receiver:
    """ReliableUDP._recv_batches / _recv_batches_window and _finish_recv without
    sockets.  ``window_chars`` None: the in-order receiver."""

    def __init__(self, be, H: int, log: Transcript, window_chars: Optional[int] = None):
        self.be, self.H, self.log, self.Wc = be, H, log, window_chars
        self.state, self.carried, self.last_isn = None, None, None
        self.parts: List[bytes] = []
        self.peer = False
        self.finack: Optional[bytes] = None   # set while the closing handshake runs
        self.fin_left = 0
        self.text: Optional[str] = None       # what recv() returned
        self.texts: List[str] = []            # ... and every recv() before it
        self.finished_round: Optional[int] = None
        self.restarts = 0                     # transfers begun (a SYN accepted as a new one)

    def _finish(self, rnd):
        self.last_isn, self.finack, self.finished_round = self.isn, None, rnd
        self.text = b"".join(self.parts).decode()
        self.texts.append(self.text)

    def again(self):
        """The next recv(): no transfer yet, the last one's peer to answer and
        its ISN to tell a repeated SYN by."""
        self.state, self.carried, self.parts, self.text = (0, 0, 1), None, [], None

    def step(self, dgrams: List[bytes], rnd: int) -> List[bytes]:
        if self.text is not None:
            return []
        if self.finack is not None:  # _finish_recv: an ACK with ack_num 1 ends the handshake
            for d in dgrams:
                got = parse_good(d, self.H)
                if got is not None and got[2] & ACK and got[1] == 1:
                    self._finish(rnd)
                    return []
            if self.fin_left < 1:
                self._finish(rnd)
                return []
            self.fin_left -= 1
            self.log.add("finack", dict(frame=self.finack))
            return [self.finack]
        if not dgrams:
            return []
        if self.Wc is None:
            res = self.be.rx_inorder(dgrams, self.state, self.last_isn, self.H)
            self.log.add("receive", res.rec)
        else:
            res = self.be.rx_window(dgrams, self.carried, self.state, self.last_isn, self.H, self.Wc)
            self.log.add("receive_window", res.rec)
        self.state, self.carried = res.state, res.carried
        out = list(res.replies)
        if res.n_carried <= res.msg_start < res.n:  # a new transfer started in this batch
            self.parts, self.peer = [], True
            self.restarts += 1
        if not self.peer:
            self.parts = []
        elif res.piece:
            self.parts.append(res.piece)
        if res.end < res.n:
            self.isn = res.isn()
            chars = len(b"".join(self.parts).decode())
            self.finack = self.be.header(0, self.isn + chars, FIN | ACK, self.H)
            self.fin_left = FIN_SENDS - 1
            self.log.add("finack", dict(frame=self.finack))
            out.append(self.finack)
        return out


class FlowReceivers:
    """FlowReceiver.poll without sockets: slots from a FlowTable keyed by the
    peer, one call per batch, a closing handshake per slot.

    Two departures from the real loop, both host logic only.  A slot that a
    stray datagram was given (a late copy after the release, frames ahead of a
    lost SYN) is released and zeroed again at once, where FlowReceiver keeps it
    until its peer's transfer ends: here "every slot is released" can then be
    asserted at the end of a conversation.  And a round is the timer's tick:
    every slot whose FIN|ACK waited through a round without the final ACK sends
    it again at the round's end, which takes in _answer_closing's immediate
    resend (on a datagram without ACK, or the closed transfer's SYN again) as
    well as the FIN_WAIT_S deadline; a slot never sends twice in a round."""

    def __init__(self, be, H: int, n_flows: int, log: Transcript):
        from rudp.flows import FlowTable
        self.be, self.H, self.log = be, H, log
        self.table = FlowTable(n_flows)
        self.states = be.rx_table(n_flows)
        self.closing: Dict[int, list] = {}    # slot -> [frame, isn, sends_left, after]
        self.parts: Dict[int, List[bytes]] = {}
        self.done: List[Tuple[int, str, int]] = []   # (peer, text, round)
        self.slot_history: List[Tuple[int, int]] = []  # (peer, slot) at every completion
        self.released = 0

    def _release(self, slot):
        self.closing.pop(slot, None)
        self.parts.pop(slot, None)
        self.table.release(slot)
        self.be.rx_release(self.states, slot)
        self.released += 1

    def step(self, arrivals: List[Tuple[int, bytes]], rnd: int) -> List[Tuple[int, bytes]]:
        out: List[Tuple[int, bytes]] = []
        waiting = set(self.closing)           # their FIN|ACK went out before this round
        for at in range(0, len(arrivals), MAX_BATCH):
            part = arrivals[at:at + MAX_BATCH]
            peers = np.array([f for f, _ in part], np.uint64)
            n = len(part)
            slots = self.table.slots(peers)
            res = self.be.rx_flows([d for _, d in part], slots, self.states, self.H)
            self.log.add("receive_flows", res.rec)
            out += [(int(peers[i]), fr) for i, fr in zip(res.reply_index, res.replies)]
            for a in range(res.rows.shape[0]):
                slot, end, _, msg_start, _, isn, kept, _ = (int(v) for v in res.rows[a])
                if msg_start < n:
                    self.parts[slot] = []
                    self.closing.pop(slot, None)
                    waiting.discard(slot)
                if kept:
                    self.parts.setdefault(slot, []).append(res.pieces[a])
                if end < n:
                    text = b"".join(self.parts.pop(slot, [])).decode()
                    peer = self.table.key_of(slot)
                    self.done.append((peer, text, rnd))
                    self.slot_history.append((peer, slot))
                    out.append((peer, res.fins[a]))
                    self.closing[slot] = [res.fins[a], isn, FIN_SENDS - 1, end]
                if slot not in self.parts and slot not in self.closing:
                    # a stray (a late copy after the release, frames ahead of a lost SYN) holds no row:
                    # the row it was given is as it was
                    self._release(slot)
            usable = np.asarray(res.usable) != 0
            for slot, c in list(self.closing.items()):  # _answer_closing: the final ACK releases the slot
                mine = np.flatnonzero((slots == slot) & usable)
                mine = mine[mine > c[3]]
                c[3] = -1
                for i in mine.tolist():
                    f = int(res.flags[i])
                    if f & ACK and not f & SYN and int(res.ack[i]) == 1:
                        self._release(slot)
                        waiting.discard(slot)
                        break
        for slot in sorted(waiting):            # a round without the final ACK: the FIN|ACK again
            c = self.closing.get(slot)
            if c is None:
                continue
            if c[2] > 0:
                c[2] -= 1
                out.append((self.table.key_of(slot), c[0]))
            else:
                self._release(slot)
        return out


class FlowSenders:
    """FlowSender.poll without sockets: a row per transfer, every flow's window
    in one batch, one call per reply batch, a timeout per flow (a round in
    which none of its replies arrived)."""

    def __init__(self, be, H: int, n_flows: int, W: int, mode: str, log: Transcript):
        from rudp.flows import FlowTable
        self.be, self.H, self.W, self.mode, self.log = be, H, W, mode, log
        self.table = FlowTable(n_flows)
        self.states = be.tx_table(n_flows)
        self.flows: Dict[int, SimpleNamespace] = {}   # slot -> its transfer
        self.outbox: List[Tuple[int, bytes]] = []
        self.done: Dict[int, Tuple[str, int]] = {}    # peer -> ("done" / "gave up", round)
        self.pointers: Dict[int, List[int]] = {}      # peer -> p after every round it ran
        self.slot_history: List[Tuple[int, int]] = []
        self.frames_rec: Dict[int, dict] = {}
        self.gen: Dict[int, int] = {}                 # peer -> transfers submitted for it so far
        # (peer, generation) -> (how it ended, round, p, closing datagram or None), kept past the release
        self.ended: Dict[Tuple[int, int], tuple] = {}

    def submit(self, peer: int, message: str, isn: int, C: int) -> int:
        slot = self.table.slot_of(peer)
        if slot is not None:
            assert self.flows[slot].closing is not None, "a transfer to this peer is still running"
            self._release(slot)
        slot = int(self.table.slots(np.array([peer], np.uint64))[0])
        frames, rec = self.be.frames(message, isn, C, self.H)
        self.frames_rec[peer] = rec
        self.be.tx_open(self.states, slot, isn, len(message), C)
        T = len(message)
        self.gen[peer] = self.gen.get(peer, -1) + 1
        self.flows[slot] = SimpleNamespace(peer=peer, slot=slot, frames=frames, T=T, C=C, rows=max(-(-T // C), 1), p=0,
                                           nxt=0, sends_left=SENDS, closing=None, linger=0, gen=self.gen[peer])
        self.slot_history.append((peer, slot))
        self.pointers[peer] = []
        return slot

    def running(self) -> int:
        return sum(1 for f in self.flows.values() if f.closing is None)

    def _release(self, slot):
        self.flows.pop(slot, None)
        self.table.release(slot)
        self.be.tx_release(self.states, slot)

    def emit(self) -> List[Tuple[int, bytes]]:
        out, self.outbox = self.outbox, []
        sent = []
        for f in self.flows.values():
            if f.closing is not None:
                continue
            hi = min(-(-f.p // f.C) + self.W, f.rows)
            if f.nxt < hi:
                out += [(f.peer, fr) for fr in f.frames[f.nxt:hi]]
                f.nxt = hi
                sent.append((f.slot, min(hi * f.C, f.T)))
        if sent and self.mode == CUMULATIVE:
            self.be.tx_sent(self.states, sent)
        return out

    def judge(self, arrivals: List[Tuple[int, bytes]], rnd: int) -> None:
        heard = {f for f, _ in arrivals}
        for at in range(0, len(arrivals), MAX_BATCH):
            part = arrivals[at:at + MAX_BATCH]
            n = len(part)
            slots = self.table.lookup(np.array([f for f, _ in part], np.uint64))
            for f in [f for f in self.flows.values() if f.closing is not None]:  # a FIN from an ended flow's peer
                if any(s == f.slot and flags_of(d) & FIN for s, (_, d) in zip(slots.tolist(), part)):
                    self.outbox.append((f.peer, f.closing))
            res = self.be.tx_flows([d for _, d in part], slots, self.states, self.mode, self.H)
            self.log.add("acknowledge_flows", res.rec)
            for a in range(res.rows.shape[0]):
                slot, end, _, _, p, _, _, _ = (int(v) for v in res.rows[a])
                f = self.flows.get(slot)
                if f is None or f.closing is not None:
                    continue
                if p != f.p:
                    f.p, f.sends_left = p, SENDS
                if end < n:
                    f.closing, f.linger = res.finals[a], rnd + LINGER
                    self.outbox.append((f.peer, f.closing))
                    self.done[f.peer] = ("done", rnd)
                    self.ended[(f.peer, f.gen)] = ("done", rnd, f.p, f.closing)
        for f in list(self.flows.values()):
            if f.closing is not None:
                if rnd >= f.linger:
                    self._release(f.slot)
                continue
            if f.peer not in heard:  # this flow's timeout
                L = min(f.C, f.T - f.p)
                f.sends_left -= 1
                self.log.add("timeout", dict(peer=[f.peer], p=[f.p], sends_left=[f.sends_left]))
                if f.sends_left < 1:
                    self.done[f.peer] = ("gave up", rnd)
                    self.ended[(f.peer, f.gen)] = ("gave up", rnd, f.p, None)
                    self.pointers[f.peer].append(f.p)
                    self._release(f.slot)
                    continue
                self.be.tx_rewind(self.states, f.slot, (f.p, L, int(f.p + L == f.T), 0))
                f.nxt = -(-f.p // f.C)
                if f.T and f.p == f.T:
                    self.outbox.append((f.peer, f.frames[f.rows]))
        for f in self.flows.values():
            if f.closing is None or self.done[f.peer][1] == rnd:
                self.pointers[f.peer].append(f.p)


# ----------------------------------------------------------------- scenarios
class Scenario(NamedTuple):
    name: str
    kind: str                 # "inorder", "window" or "flows"
    layout: int               # 5 or 7
    outcome: str              # "delivered" or "stalled"
    T: int = 0
    C: int = 1
    isn: int = 1
    W: int = 1
    mode: str = EXACT
    window_chars: Optional[int] = None
    rules: tuple = ()         # the single flow's script
    p: float = 0.0            # random faults
    budget: int = 0
    flows: tuple = ()         # kind "flows": (peer, T, C, isn, start round, rules) per transfer
    n_flows: int = 0          # rows of the tables
    again: Optional[Tuple[int, int]] = None   # single peer: (T, isn) of a second send() / recv() on the same pair


def cap(sc: Scenario) -> int:
    """The round a conversation must have ended by: the handshake (a round for
    the closing datagram and one for its receipt), the clean rounds (a window
    per round at the least: one frame per round in the worst case), and per
    budgeted fault the rounds a timeout chain can cost (SENDS of them, plus the
    two a delayed datagram may linger), and the receiver's FIN_SENDS rounds of
    waiting for a closing ACK that never comes.  A sender that gives up does so
    after SENDS empty rounds in a row, which the same terms cover.  A rule
    that meets every datagram may cost a chain per frame."""
    def one(T, C, rules, start=0):
        rows = max(-(-T // C), 1)
        def cost(rule):  # the timeout chains a rule can set off
            _, match, action = rule
            if match[0] == "all":
                return rows
            if action in ("swap", "dup"):
                return 0
            return 4 if match[0] in ("round", "round_rest") or match[-1] is None else 1
        faults = sc.budget + sum(cost(r) for r in rules)
        return start + rows + 2 + (SENDS + 2) * (faults + 1) + FIN_SENDS + LINGER
    if sc.kind == "flows":
        return max(one(T, C, rules, start) for _, T, C, _, start, rules in sc.flows)
    return one(sc.T, sc.C, sc.rules) + (one(sc.again[0], sc.C, ()) if sc.again else 0)


def _single():
    rows = []
    lose = lambda d, m: (d, m, "lose")  # noqa: E731
    scripted = {
        "syn_lost": (lose(C2S, ("ord", 0)),),
        "fin_lost": (lose(C2S, ("flag", FIN, FIN, 0)),),
        "replies_lost": (lose(S2C, ("round", 1)),),
        "finack_lost": (lose(S2C, ("flag", FIN, FIN, 0)),),
        "closing_ack_lost": (lose(C2S, ("flag", ACK, ACK, 0)),),
        # round 1's replies: the first comes a round late, the rest are lost, so the sender times out,
        # rewrites its state, and the stale reply arrives with the answers to the retransmission
        "stale_reply": ((S2C, ("round_rest", 1), "lose"), (S2C, ("round", 1), "delay1")),
    }
    # T in {0, 1, C, 2C + 1, 300} (and 20 or 40 characters where a scenario needs more than a window of
    # one-character frames), C in {1, 3, 16}, isn in {1, 4999, 65535 - T}
    shapes = [(0, 1, 1), (1, 1, 4999), (3, 3, 4999), (7, 3, 1), (33, 16, 65535 - 33), (300, 16, 4999),
              (40, 1, 65535 - 40)]
    for layout in (5, 7):
        for W, mode in ((1, EXACT), (8, CUMULATIVE)):
            tag = f"rudp{layout}_{mode}_W{W}"
            for T, C, isn in shapes:
                rows.append(Scenario(f"inorder_clean_{tag}_T{T}_C{C}", "inorder", layout, "delivered", T, C, isn, W,
                                     mode))
            for k, (T, C, isn) in enumerate(((40, 1, 4999), (33, 16, 65535 - 33), (7, 3, 1), (300, 16, 1))):
                rows.append(Scenario(f"inorder_random{k}_{tag}_T{T}_C{C}", "inorder", layout, "delivered", T, C, isn, W,
                                     mode, p=0.2, budget=6))
            for k, (what, rules) in enumerate(scripted.items()):
                # (shapes of three rounds at the least: a script on round 1 meets data frames and replies)
                T, C, isn = (((7, 3, 4999), (3, 1, 65535 - 3)) if W == 1 else
                             ((300, 16, 4999), (300, 3, 65535 - 300)))[(k + layout) % 2]
                rows.append(Scenario(f"inorder_{what}_{tag}_T{T}_C{C}", "inorder", layout, "delivered", T, C, isn,
                                     W, mode, rules=rules))
    # the reordering receiver behind a cumulative sender with 8 frames in flight
    win = {
        "reversed": ((C2S, ("all",), "reverse"),),
        # frame 2 comes two rounds late: what is behind it waits over two calls at least
        "gap": ((C2S, ("ord", 2), "delay2"),),
        "beyond": ((C2S, ("ord", 1), "lose"), (C2S, ("ord", 2), "lose")),
        # frame 1 comes two rounds late; of the frames that wait behind it, 3 has a copy in its own batch
        # and 4 and 5 have one in the next, when they are carried frames
        "carried_dups": ((C2S, ("ord", 1), "delay2"), (C2S, ("ord", 3), "dup"), (C2S, ("ord", 4), "dup_delay1"),
                         (C2S, ("ord", 5), "dup_delay1")),
    }
    for layout in (5, 7):
        for Wc in (1, 8, 64):
            tag = f"rudp{layout}_Wc{Wc}"
            for k, (what, rules) in enumerate(win.items()):
                # (a window of 8 characters holds a frame ahead only when frames are shorter than that)
                T, C, isn = ((300, 16, 4999), (20, 1, 65535 - 20))[1 if Wc == 8 else k % 2]
                if what == "beyond" and Wc == 8:
                    # (and holds none of the 8 in flight beyond it when they are one character each: with
                    # three, frames 1 and 2 lost leave 3 in the window and 4 to 7 beyond)
                    T, C, isn = 300, 3, 65535 - 300
                rows.append(Scenario(f"window_{what}_{tag}_T{T}_C{C}", "window", layout, "delivered", T, C, isn, 8,
                                     CUMULATIVE, Wc, rules=rules))
            for k, (T, C, isn) in enumerate(((40, 1, 1), (300, 16, 4999), (0, 1, 1), (1, 1, 65534))):
                # (a transfer of one frame is a handful of datagrams: faults are likelier there, so that it meets one)
                rows.append(Scenario(f"window_random{k}_{tag}_T{T}_C{C}", "window", layout, "delivered", T, C, isn, 8,
                                     CUMULATIVE, Wc, p=0.25 if T > 1 else 0.6, budget=8 if T > 1 else 2))
    # beyond the domain: isn + T > 65535.  Nothing matches once expect passes 65535: the transfer stalls
    # at the line and the sender gives up.
    for layout in (5, 7):
        rows.append(Scenario(f"inorder_beyond_domain_rudp{layout}", "inorder", layout, "stalled", 10, 1, 65530, 1,
                             EXACT))
        rows.append(Scenario(f"window_beyond_domain_rudp{layout}", "window", layout, "stalled", 20, 3, 65530, 8,
                             CUMULATIVE, 8))
    # exact mode with 8 frames in flight and one reply lost: the acks behind it are past the expected one,
    # and after the timeout the receiver answers every retransmission with its newest ack: no reply ever
    # matches again (what cumulative mode is for)
    for layout in (5, 7):
        rows.append(Scenario(f"inorder_exact_W8_reply_lost_rudp{layout}", "inorder", layout, "stalled", 20, 1, 4999, 8,
                             EXACT, rules=((S2C, ("ord", 1), "lose"),)))
    # two transfers on the same pair: a copy of the first SYN arrives during the second recv(), whose
    # last_isn tells it from a new transfer (it is answered, the old peer is still there, and changes
    # nothing)
    for layout in (5, 7):
        late = ((C2S, ("ord", 0), "dup_delay4"),)
        for W, mode in ((1, EXACT), (8, CUMULATIVE)):
            rows.append(Scenario(f"inorder_again_rudp{layout}_{mode}_W{W}", "inorder", layout, "delivered", 3, 1, 4999, W,
                                 mode, rules=late, again=(20, 65535 - 20)))
        rows.append(Scenario(f"window_again_rudp{layout}_Wc8", "window", layout, "delivered", 3, 1, 4999, 8,
                             CUMULATIVE, 8, rules=late, again=(20, 65535 - 20)))
    # a copy of the SYN two rounds late, behind later frames of its transfer: receive_data starts over at
    # ISN + C while the sender is further on, and no frame it still sends matches again (classified on the
    # CPU run of accept_ref / ack_ref)
    for layout in (5, 7):
        rows.append(Scenario(f"inorder_late_syn_copy_rudp{layout}", "inorder", layout, "stalled", 12, 1, 4999, 1, EXACT,
                             rules=((C2S, ("ord", 0), "dup_delay2"),)))
    return rows


def _flow_rules(k: int):
    """Flow k's own script."""
    menu = (
        (),
        ((C2S, ("ord", 0), "lose"),),
        ((C2S, ("flag", FIN, FIN, 0), "lose"),),
        ((S2C, ("round", 1), "lose"),),
        ((S2C, ("flag", FIN, FIN, 0), "lose"),),
        ((C2S, ("flag", ACK, ACK, 0), "lose"),),
        ((S2C, ("round_rest", 1), "lose"), (S2C, ("round", 1), "delay1")),
        ((C2S, ("ord", 2), "delay1"), (S2C, ("ord", 3), "dup")),
        ((C2S, ("ord", 1), "lose"), (S2C, ("ord", 1), "lose")),
    )
    return menu[k % len(menu)]


def _many():
    rows = []
    rng = random.Random("flows")
    for layout in (5, 7):
        for W, mode in ((1, EXACT), (8, CUMULATIVE)):
            flows = []
            for k in range(37):
                T = (0, 1, 3, 7, 60, 33, 16)[k % 7] if k < 14 else rng.randint(0, 60)
                C = (1, 3, 16)[k % 3]
                isn = (1, 4999, 65535 - T)[(k // 3) % 3]
                flows.append((k + 100, T, C, isn, 0, _flow_rules(k)))
            rows.append(Scenario(f"flows37_rudp{layout}_{mode}_W{W}", "flows", layout, "delivered", W=W, mode=mode,
                                 flows=tuple(flows), n_flows=37, p=0.1, budget=3))
        # 128 flows with 8 frames in flight each: the first round's batch is exactly 1024 datagrams
        # (the scripts lose a frame or a reply behind the first round, and never add a datagram)
        menu = (((C2S, ("ord", 9), "lose"),), ((S2C, ("ord", 2), "lose"),), (), ())
        flows = tuple((k + 1000, 8 + k % 5, 1, 1 + 37 * k, 0, menu[k % 4]) for k in range(128))
        rows.append(Scenario(f"flows128_rudp{layout}", "flows", layout, "delivered", W=8, mode=CUMULATIVE, flows=flows,
                             n_flows=128))
        # slot reuse: peer 7's transfer ends while its closing ACK is lost, so its slot (the table's last
        # row) still waits when a copy of its SYN arrives (seq == last_isn: ignored); then the slot is
        # released and a new transfer of the same peer opens it again with another ISN.  Peer 5 holds
        # the first row from start to end.
        flows = ((5, 60, 1, 1, 0, ()),
                 (7, 4, 3, 4999, 0, ((C2S, ("ord", 0), "dup_delay2"), (C2S, ("flag", ACK, ACK, 0), "lose"))),
                 (7, 9, 3, 65535 - 9, 5, ()))
        rows.append(Scenario(f"flows_slot_reuse_rudp{layout}", "flows", layout, "delivered", W=8, mode=CUMULATIVE,
                             flows=flows, n_flows=2))
    return rows


SCENARIOS: Dict[str, Scenario] = {s.name: s for s in _single() + _many()}


def message_of(sc: Scenario, peer=None, T=None) -> str:
    return text_of(f"{sc.name}/{peer}", sc.T if T is None else T)


# ---------------------------------------------------------------- conversations
class Result(NamedTuple):
    transcript: Transcript
    outcome: str                 # "delivered" or "stalled"
    rounds: int
    sender: object
    receiver: object
    channel: Channel


def converse(sc: Scenario, be, rounds: Optional[int] = None) -> Result:
    """Run scenario ``sc`` on backend ``be`` to its end (``rounds`` None; never
    past ``cap(sc)``) or for exactly ``rounds`` rounds."""
    return (_converse_flows if sc.kind == "flows" else _converse_single)(sc, be, rounds)


def _converse_single(sc, be, rounds, flow=0, message=None, rules=None):
    log = Transcript()
    H = sc.layout
    message = message_of(sc) if message is None else message
    ch = Channel(sc.name, H, {flow: sc.rules if rules is None else rules}, sc.p, sc.budget)
    log.begin()
    tx = Sender(be, message, sc.isn, sc.C, sc.W, sc.mode, H, log)
    log.add("frames", tx.frames_rec)
    rx = Receiver(be, H, log, sc.window_chars if sc.kind == "window" else None)
    limit = cap(sc) if rounds is None else rounds
    rnd, more = 0, [sc.again] if sc.again else []
    while rnd < limit:
        log.begin()
        rx_out = rx.step(ch.carry(flow, C2S, rnd, tx.emit()), rnd)
        tx.judge(ch.carry(flow, S2C, rnd, rx_out), rnd)
        rnd += 1
        if more and tx.finished == "done" and not tx.outbox and rx.text is not None:
            T, isn = more.pop(0)   # the next send() and recv() of the same pair
            tx = Sender(be, text_of(f"{sc.name}/again", T), isn, sc.C, sc.W, sc.mode, H, log)
            log.add("frames", tx.frames_rec)
            rx.again()
        elif rounds is None and tx.finished and not tx.outbox and not ch.pending() and \
                (rx.text is not None or rx.finack is None):
            break
    delivered = tx.finished == "done" and rx.text is not None and not more
    return Result(log, "delivered" if delivered else "stalled", rnd, tx, rx, ch)


def _converse_flows(sc, be, rounds):
    log = Transcript()
    H = sc.layout
    ch = Channel(sc.name, H, {}, sc.p, sc.budget)
    log.begin()
    tx = FlowSenders(be, H, sc.n_flows, sc.W, sc.mode, log)
    rx = FlowReceivers(be, H, sc.n_flows, log)
    todo = sorted(sc.flows, key=lambda f: f[4])
    limit = cap(sc) if rounds is None else rounds
    rnd, gen = 0, {}
    while rnd < limit:
        log.begin()
        while todo and todo[0][4] <= rnd:
            peer, T, C, isn, _, rules = todo.pop(0)
            gen[peer] = gen.get(peer, -1) + 1
            # (a peer's later transfer is another flow of the channel: its ordinals start over)
            ch.rules[(peer, gen[peer])] = list(rules)
            tx.submit(peer, text_of(f"{sc.name}/{peer}/{gen[peer]}", T), isn, C)
            log.add("frames", tx.frames_rec[peer])
        per: Dict[int, List[bytes]] = {}
        for peer, d in tx.emit():
            per.setdefault(peer, []).append(d)
        live = set(per) | {k[0][0] for k, h in ch.held.items() if k[1] == C2S and h.get(rnd)}
        arrived = {peer: ch.carry((peer, gen[peer]), C2S, rnd, per.get(peer, [])) for peer in sorted(live)}
        back: Dict[int, List[bytes]] = {}
        for peer, d in rx.step(ch.merge(C2S, rnd, arrived), rnd):
            back.setdefault(peer, []).append(d)
        live = set(back) | {k[0][0] for k, h in ch.held.items() if k[1] == S2C and h.get(rnd)}
        arrived = {peer: ch.carry((peer, gen[peer]), S2C, rnd, back.get(peer, [])) for peer in sorted(live)}
        tx.judge(ch.merge(S2C, rnd, arrived), rnd)
        rnd += 1
        if rounds is None and not todo and not tx.running() and not tx.outbox and not ch.pending() and \
                not rx.closing and not tx.flows:
            break
    texts = {}
    for peer, text, _ in rx.done:
        texts.setdefault(peer, []).append(text)
    want = {}
    for peer, T, _, _, _, _ in sorted(sc.flows, key=lambda f: f[4]):
        want.setdefault(peer, []).append(text_of(f"{sc.name}/{peer}/{len(want.get(peer, []))}", T))
    delivered = texts == want and all(v[0] == "done" for v in tx.done.values()) and len(tx.done) == len(want)
    return Result(log, "delivered" if delivered else "stalled", rnd, tx, rx, ch)


def solo(sc: Scenario, k: int, be) -> Result:
    """Flow k of a many-peer scenario alone, through the single-peer in-order
    conversation, under its own fault script (the same channel decisions: they
    are keyed by the flow, not by the batch)."""
    peer, T, C, isn, _, rules = sc.flows[k]
    one = sc._replace(kind="inorder", T=T, C=C, isn=isn)
    return _converse_single(one, be, None, flow=(peer, 0), message=text_of(f"{sc.name}/{peer}/0", T), rules=rules)


# -------------------------------------------------- checks shared by the CPU and the GPU tests
_ref_runs: Dict[str, Result] = {}


def ref_run(name: str) -> Result:
    """The CPU conversation of a scenario, run once."""
    if name not in _ref_runs:
        _ref_runs[name] = converse(SCENARIOS[name], RefBackend())
    return _ref_runs[name]


def closing(isn: int, T: int, H: int) -> bytes:
    """The sender's closing datagram, written out: seq (isn + T) mod 2^16,
    ack 1 (the receiver's FIN|ACK has seq 0), ACK."""
    seq = (isn + T) & 0xFFFF
    head = bytes([seq >> 8, seq & 0xFF, 0, 1, ACK])
    return head if H == 5 else head + csum_of(seq, 1, ACK).to_bytes(2, "big")


def check_end(sc: Scenario, res: Result) -> None:
    """The end-to-end assertions, independent of the per-round comparison: the
    text that comes out is the text that went in, exactly once and in order;
    every sender ends done with p == T and the closing datagram (isn + T) mod
    2^16, 1, ACK; every slot is released."""
    assert res.outcome == sc.outcome, (sc.name, res.outcome, res.rounds)
    tx, rx = res.sender, res.receiver
    if sc.kind == "flows":
        assert sc.outcome == "delivered"
        want, ends = {}, {}
        for peer, T, _, isn, _, _ in sorted(sc.flows, key=lambda f: f[4]):
            g = len(want.get(peer, []))
            want.setdefault(peer, []).append(text_of(f"{sc.name}/{peer}/{g}", T))
            ends[(peer, g)] = (T, closing(isn, T, sc.layout))
        got = {}
        for peer, text, _ in rx.done:
            got.setdefault(peer, []).append(text)
        assert got == want                                        # exactly once, in order
        assert set(tx.ended) == set(ends)                         # every transfer, slot-reuse generations included
        for key, (T, frame) in ends.items():
            how, _, p, sent = tx.ended[key]
            assert (how, p) == ("done", T), (sc.name, key, how, p, T)
            assert sent == frame, (sc.name, key, sent.hex(), frame.hex())
        assert not tx.flows and len(tx.table) == 0                # every sender row released ...
        assert not rx.closing and len(rx.table) == 0              # ... and every receiver row
        assert not norm(tx.be.table_host(tx.states)).any()        # both tables are all idle rows again
        assert not norm(rx.be.table_host(rx.states)).any()
        return
    msg = message_of(sc)
    if sc.outcome == "delivered" and sc.again:
        T, isn = sc.again
        assert rx.texts == [msg, text_of(f"{sc.name}/again", T)] and rx.restarts == 2
        assert tx.finished == "done" and tx.p == T and tx.closing == closing(isn, T, sc.layout)
        assert rx.last_isn == isn
    elif sc.outcome == "delivered":
        assert rx.texts == [msg] and rx.restarts >= 1             # exactly once
        assert tx.finished == "done" and tx.p == sc.T
        assert tx.closing == closing(sc.isn, sc.T, sc.layout)
        assert rx.last_isn == sc.isn
    else:
        assert tx.finished == "gave up" and tx.p < sc.T and rx.text is None


def check_wire_trace(be) -> None:
    """W = 1, C = 1, exact mode, a clean channel, on the message and ISN of
    tests/golden/wire_trace.json: the reference's own datagrams, both ways."""
    import json
    from conftest import GOLDEN
    trace = json.loads((GOLDEN / "wire_trace.json").read_text())
    sc = Scenario("wire_trace", "inorder", 5, "delivered", len(trace["message"]), 1, trace["isn"], 1, EXACT)
    log = Transcript()
    ch = Channel("wire_trace", 5)
    log.begin()
    tx = Sender(be, trace["message"], sc.isn, 1, 1, EXACT, 5, log)
    rx = Receiver(be, 5, log)
    c2s, s2c = [], []
    for rnd in range(cap(sc)):
        log.begin()
        out = tx.emit()
        c2s += out
        back = rx.step(ch.carry(0, C2S, rnd, out), rnd)
        s2c += back
        tx.judge(ch.carry(0, S2C, rnd, back), rnd)
        if tx.finished and not tx.outbox and rx.text is not None:
            break
    assert rx.text == trace["message"] and tx.finished == "done"
    assert [d.hex() for d in c2s] == trace["client_to_server"]
    assert [d.hex() for d in s2c] == trace["server_to_client"]
