"""CPU reference for rudp_accept_flows: ``accept_ref`` (tests/accept_ref.py)
applied to every flow's datagrams in arrival order with the flow's row as its
state, then the turn-over of the flows that ended, the flow-major ranks, the
order and the per-flow rows (include/rudp.h states the contract).

``interleave`` merges streams of ``clean_stream`` / ``adversarial_stream`` into
one arrival order, every stream keeping its own order; ``make_batch`` builds the
mix the GPU tests use."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from accept_ref import FIN, SYN, accept_ref, adversarial_stream, clean_stream, scan_model

FLOW_NONE = 0xFFFFFFFF
RANK_NONE = 0xFFFFFFFF
ST_FLOW = 256


class FlowsRef(NamedTuple):
    accept: np.ndarray      # u8 [n]
    keep: np.ndarray        # u8 [n]
    reply: np.ndarray       # u8 [n]
    reply_ack: np.ndarray   # u16 [n]
    rank: np.ndarray        # u32 [n]
    order: np.ndarray       # u32 [n]
    order_off: np.ndarray   # u32 [A + 1]
    flow_info: np.ndarray   # u64 [A, 8]
    info: list              # [A, K, R, ended, flowless]
    states: np.ndarray      # u64 [n_flows, 4]: the table after the call
    status: int
    anomalous: list         # per active flow: its scan_model has an anomaly before its end


def row_state(row):
    """(state, last_isn) of a table row as accept_ref takes them."""
    w3 = int(row[3])
    return (int(row[0]), int(row[1]), 1 if row[2] else 0), (w3 - 1 if 1 <= w3 <= 65536 else None)


def flows_ref(seq, flags, chars, usable, flow, states) -> FlowsRef:
    n = len(seq)
    states = np.array(states, np.uint64).reshape(-1, 4).copy()
    n_flows = states.shape[0]
    flow = np.asarray(flow, np.uint32)
    us = np.ones(n, bool) if usable is None else np.asarray(usable).astype(bool)
    valid = flow.astype(np.int64) < n_flows
    status = ST_FLOW if (~valid & (flow != FLOW_NONE)).any() else 0
    accept, keep, reply = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ack = np.zeros(n, np.uint16)
    rank = np.full(n, RANK_NONE, np.uint32)
    slots = sorted(set(flow[valid].tolist()))
    order, order_off, rows, anomalous = [], [], [], []
    K = ended = 0
    for slot in slots:
        idx = np.flatnonzero(valid & (flow == slot))
        order_off.append(len(order))
        order.extend(idx.tolist())
        state, last = row_state(states[slot])
        sub = (np.asarray(seq)[idx], np.asarray(flags)[idx], np.asarray(chars)[idx], us[idx])
        r = accept_ref(*sub, state, last)
        m = scan_model(*sub, state, last)
        anomalous.append(m.first_anomaly < len(idx))
        judged = np.arange(len(idx)) <= r.end
        accept[idx], keep[idx] = r.accept * judged, r.keep * judged
        reply[idx], ack[idx] = r.reply * judged, r.reply_ack * judged
        kept = idx[r.keep.astype(bool) & judged]
        rank[kept] = K + np.arange(len(kept))
        end = int(idx[r.end]) if r.end < len(idx) else n
        ms = int(idx[r.msg_start]) if r.msg_start < len(idx) else n
        expect, isn, live = r.state
        rows.append([slot, end, int((r.accept * judged).sum()), ms, r.characters, isn, len(kept), K])
        K += len(kept)
        if end < n:
            ended += 1
            states[slot] = (0, 0, 0, isn + 1)
        else:
            states[slot, :3] = (expect, isn, live)
    order_off.append(len(order))
    order.extend(np.flatnonzero(~valid).tolist())
    info = [len(slots), K, int(reply.sum()), ended, int((~valid).sum())]
    return FlowsRef(accept, keep, reply, ack, rank, np.array(order, np.uint32), np.array(order_off, np.uint32),
                    np.array(rows, np.uint64).reshape(len(slots), 8), info, states, status, anomalous)


def arrival_order(rng, lens):
    """The stream each datagram of a merged arrival order comes from: a random
    shuffle of every stream's index repeated by its length."""
    pick = [k for k, c in enumerate(lens) for _ in range(c)]
    rng.shuffle(pick)
    return pick


def interleave(rng, streams, slots, p_none=0.0):
    """One arrival order out of ``streams`` (tuples seq, flags, chars, usable),
    stream k on slot ``slots[k]``: the next datagram comes from a stream drawn
    in proportion to what it has left, so every stream keeps its own order.
    With probability ``p_none`` a datagram loses its flow (FLOW_NONE).
    Returns seq (u16), flags (u8), chars (u32), usable (u8), flow (u32)."""
    pick = arrival_order(rng, [len(s[0]) for s in streams])
    at = [0] * len(streams)
    n = len(pick)
    seq, flags = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    chars, usable, flow = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    for i, k in enumerate(pick):
        j = at[k]
        at[k] += 1
        seq[i], flags[i], chars[i], usable[i] = (streams[k][c][j] for c in range(4))
        flow[i] = FLOW_NONE if rng.random() < p_none else slots[k]
    return seq, flags, chars, usable, flow


def make_batch(rng, n, n_active, n_flows=5000, p_none=0.02, slots=None):
    """The GPU tests' mix: ``n`` datagrams of ``n_active`` flows (each at least
    one datagram), two thirds ``clean_stream`` (half of them with a FIN placed
    inside the batch), one third ``adversarial_stream``; slots drawn from
    [0, n_flows), the first and the last row among them when there are two or
    more flows.  Returns (seq, flags, chars, usable, flow)."""
    n_active = min(n_active, n)
    cuts = sorted(rng.sample(range(1, n), n_active - 1)) if n_active > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    if slots is None:
        if n_active >= 2:
            slots = [0, n_flows - 1] + rng.sample(range(1, n_flows - 1), n_active - 2)
            rng.shuffle(slots)
        else:
            slots = [rng.randrange(n_flows)]
    streams, clean = [], 0
    for k, m in enumerate(lens):
        if k % 3 == 2:
            streams.append(adversarial_stream(rng, m, p_fin=0.02))
        else:
            clean += 1
            fin_at = None
            if clean % 2 == 0:  # (inside the batch: datagrams follow the end where the flow has any left)
                fin_at = rng.randrange(m - 1) if m > 1 else 0
            streams.append(clean_stream(rng, m, fin_at=fin_at, max_chars=rng.choice((1, 1, 3, 16)), high_isn=0.2))
    return interleave(rng, streams, slots, p_none)


__all__ = ["FIN", "SYN", "FLOW_NONE", "RANK_NONE", "ST_FLOW", "FlowsRef", "flows_ref", "interleave", "make_batch",
           "row_state"]
