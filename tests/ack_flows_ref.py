"""CPU reference for rudp_ack_flows: ``ack_ref`` (tests/ack_ref.py) applied to
every flow's replies in arrival order with the flow's row as its state and
constants, then the idle, refused and done rows, the order, the per-flow rows
and the closing datagrams (include/rudp.h states the contract).

``make_reply_batch`` builds the mix the GPU tests use: per-flow streams of
``ack_ref.clean_replies`` / ``ack_ref.adversarial_replies`` merged into one
arrival order with ``flows_ref.arrival_order``."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ack_ref import (ACK, CUMULATIVE, EXACT, FIN, ack_ref, adversarial_replies, clean_replies, fresh_state,
                     scan_model)
from flows_ref import FLOW_NONE, ST_FLOW, arrival_order

ST_FLOW_ROW = 512


class AckFlowsRef(NamedTuple):
    valid: np.ndarray       # u8 [n]
    pointer: np.ndarray     # u64 [n]
    order: np.ndarray       # u32 [n]
    order_off: np.ndarray   # u32 [A + 1]
    flow_info: np.ndarray   # u64 [A, 8]
    info: list              # [A, valid, E, newly, outside]
    states: np.ndarray      # u64 [n_flows, 8]: the table after the call
    status: int
    finals: list            # per ended flow, ascending slot: (a, seq, ack) of its closing datagram
    anomalous: list         # per active flow: judged, and its scan_model has an anomaly before its end
    kinds: dict             # counts of the flow kinds of the batch (the GPU tests' input condition)


def open_row(isn, T, C, sent=0):
    """A fresh transfer's row."""
    p, L, last, done = fresh_state(T, C)
    return [p, L, last, done, isn, T, C, sent]


def row_kind(row, mode):
    """'idle', 'bad' or 'ok' for a table row."""
    isn, T, C, sent = (int(v) for v in row[4:8])
    if C == 0:
        return "idle"
    if isn > 65535 or C > 16383 or (mode == CUMULATIVE and sent > T):
        return "bad"
    return "ok"


def ack_flows_ref(seq, ack, flags, usable, flow, states, mode=EXACT) -> AckFlowsRef:
    n = len(ack)
    states = np.array(states, np.uint64).reshape(-1, 8).copy()
    n_flows = states.shape[0]
    flow = np.asarray(flow, np.uint32)
    seq, ack, flags = np.asarray(seq), np.asarray(ack), np.asarray(flags)
    us = np.ones(n, bool) if usable is None else np.asarray(usable).astype(bool)
    in_range = flow.astype(np.int64) < n_flows
    status = ST_FLOW if (~in_range & (flow != FLOW_NONE)).any() else 0
    kinds = {"idle": 0, "bad": 0, "done": 0, "anomalous": 0, "plain": 0, "ended_early": 0}
    judged = np.zeros(n, bool)
    slots = []
    for slot in sorted(set(flow[in_range].tolist())):
        kind = row_kind(states[slot], mode)
        if kind == "ok":
            slots.append(slot)
            judged |= flow == slot
        else:
            kinds[kind] += 1
            if kind == "bad":
                status |= ST_FLOW_ROW
    valid = np.zeros(n, np.uint8)
    pointer = np.zeros(n, np.uint64)
    order, order_off, rows, finals, anomalous = [], [], [], [], []
    count = ended = 0
    newly = 0
    for a, slot in enumerate(slots):
        idx = np.flatnonzero(flow == slot)
        order_off.append(len(order))
        order.extend(idx.tolist())
        row = [int(v) for v in states[slot]]
        state, (isn, T, C, sent) = tuple(row[:4]), row[4:8]
        sub = (seq[idx], ack[idx], flags[idx], us[idx])
        kw = dict(isn=isn, T=T, C=C, state=state, mode=mode, sent=sent if mode == CUMULATIVE else None)
        r = ack_ref(*sub, **kw)
        if state[3]:
            kinds["done"] += 1
            anomalous.append(False)
            rows.append([slot, n, 0, 0, state[0], -(-state[0] // C), 1, 0])
            continue
        m = scan_model(sub[1], sub[2], sub[3], **kw)
        anomalous.append(m.first_anomaly < len(idx))
        kinds["anomalous" if anomalous[-1] else "plain"] += 1
        inside = np.arange(len(idx)) <= r.end
        valid[idx] = r.valid * inside
        pointer[idx] = (r.pointer * inside).astype(np.uint64)
        end = int(idx[r.end]) if r.end < len(idx) else n
        closing = 0
        if end < n:
            ended += 1
            kinds["ended_early"] += r.end < len(idx) - 1
            finals.append((a, r.final[0], r.final[1]))
            closing = r.final[0] | r.final[1] << 16
        p = r.state[0]
        rows.append([slot, end, r.count, r.newly % (1 << 64), p, -(-p // C), r.done, closing])
        count += r.count
        newly = (newly + r.newly) % (1 << 64)
        states[slot, :4] = r.state
    order_off.append(len(order))
    order.extend(np.flatnonzero(~judged).tolist())
    info = [len(slots), count, ended, newly, int((~judged).sum())]
    return AckFlowsRef(valid, pointer, np.array(order, np.uint32), np.array(order_off, np.uint32),
                       np.array(rows, np.uint64).reshape(len(slots), 8), info, states, status, finals, anomalous, kinds)


def make_reply_batch(rng, n, n_active, mode=EXACT, n_flows=5000, p_none=0.02, slots=None, special=None,
                     adversarial=()):
    """The GPU tests' mix: ``n`` replies of ``n_active`` flows (each at least one
    reply), two thirds ``clean_replies``, one third ``adversarial_replies``
    (every third flow, and those named in ``adversarial``), with mixed isn
    (some near 65535), T (0 among them), C and W; slots drawn from [0,
    n_flows), the first and the last row among them when there are two or more
    flows.  ``special`` maps a flow's index to "done" (its row has done set on
    entry) or "idle" (its row is all zero); None: with four or more flows, flow
    3 is done and flow 1 idle.  Returns (seq, ack, flags, usable, flow, table)
    with the table's rows opened (in cumulative mode with ``sent`` = T: the
    sender has everything in flight)."""
    if special is None:
        special = {3: "done", 1: "idle"} if n_active >= 4 else {}
    n_active = min(n_active, n)
    cuts = sorted(rng.sample(range(1, n), n_active - 1)) if n_active > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    if slots is None:
        if n_active >= 2:
            slots = [0, n_flows - 1] + rng.sample(range(1, n_flows - 1), n_active - 2)
            rng.shuffle(slots)
        else:
            slots = [rng.randrange(n_flows)]
    table = np.zeros((n_flows, 8), np.uint64)
    streams = []
    for k, m in enumerate(lens):
        C = rng.choice((1, 1, 3, 16, 1000))
        T = rng.choice((0, 1, C, 5 * C, 7 * C + (1 if C > 1 else 0), 40 * C))
        isn = rng.choice((0, 7, 1000, 65535, max(0, 65535 - T // 2), 65530))
        W = rng.choice((1, 1, 4, 8))
        if k % 3 == 2 or k in adversarial:
            s = adversarial_replies(rng, m, isn=isn, T=T, C=C)
        else:
            s = clean_replies(rng, m, isn=isn, T=T, C=C, W=W)
        streams.append(s)
        table[slots[k]] = open_row(isn, T, C, T if mode == CUMULATIVE else 0)
        if special.get(k) == "done":
            table[slots[k], 3] = 1
        elif special.get(k) == "idle":
            table[slots[k]] = 0
    pick = arrival_order(rng, lens)
    at = [0] * len(streams)
    seq, ack = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    flags, usable, flow = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    for i, k in enumerate(pick):
        j = at[k]
        at[k] += 1
        seq[i], ack[i], flags[i], usable[i] = (streams[k][c][j] for c in range(4))
        flow[i] = FLOW_NONE if j and rng.random() < p_none else slots[k]  # (a flow keeps its first reply)
    return seq, ack, flags, usable, flow, table


__all__ = ["ACK", "FIN", "EXACT", "CUMULATIVE", "FLOW_NONE", "ST_FLOW", "ST_FLOW_ROW", "AckFlowsRef",
           "ack_flows_ref", "make_reply_batch", "open_row", "row_kind"]
