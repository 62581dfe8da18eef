"""rudp_accept_flows / batch.accept_flows / batch.receive_flows on the device:
every output bit for bit against the oracle (tests/flows_ref.py: accept_ref per
flow) for every batch size around the kernel's thread and tile edges and every
flow count from one flow to a flow per datagram, rows carried over three
batches, one flow against rudp_accept_inorder, the whole chain from frames to
message pieces and reply datagrams, and stream capture."""
import random

import numpy as np
import pytest

from accept_ref import ACK, FIN, SYN, adversarial_stream, chars_ref, clean_stream
from flows_ref import FLOW_NONE, RANK_NONE, ST_FLOW, arrival_order, flows_ref, interleave, make_batch
from rudp import _native, batch

pytestmark = pytest.mark.gpu

SENT8, SENT16, SENT32, SENT64 = 0xA5, 0xA5A5, 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
PAD = 8  # sentinel entries on either side of every output
N_FLOWS = 5000
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)


# ----------------------------------------------------------------- helpers
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _table(cuda, table):
    return _dev(cuda, np.asarray(table, np.uint64).view(np.int64))


class Got:
    pass


def flows_call(cuda, seq, flags, chars, usable, flow, d_table):
    """rudp_accept_flows with every output between sentinels; d_table (int64
    [n_flows, 4] on the device) is updated in place."""
    import torch
    n = len(seq)
    d_in = [_dev(cuda, seq), _dev(cuda, flags), _dev(cuda, np.asarray(chars, np.uint32).view(np.int32)),
            _dev(cuda, usable) if usable is not None else None, _dev(cuda, np.asarray(flow, np.uint32).view(np.int32))]
    u8 = [torch.full((n + 2 * PAD,), SENT8, dtype=torch.uint8, device=cuda) for _ in range(3)]
    ack = _dev(cuda, np.full(n + 2 * PAD, SENT16, np.uint16))
    u32 = [_dev(cuda, np.full(m + 2 * PAD, SENT32, np.uint32).view(np.int32)) for m in (n, n, n + 1)]
    rows = _dev(cuda, np.full(8 * (n + 2 * PAD), SENT64, np.uint64).view(np.int64))
    tail = _dev(cuda, np.full(8 + 2 * PAD, SENT64, np.uint64).view(np.int64))
    status = _dev(cuda, np.full(1 + 2 * PAD, SENT32, np.uint32).view(np.int32))

    def ptr(t, width):
        return t.data_ptr() + width * PAD if n else None

    rc = _native.lib().rudp_accept_flows(
        *(t.data_ptr() if t is not None and n else None for t in d_in), n, d_table.data_ptr(), d_table.shape[0],
        *(ptr(t, 1) for t in u8), ptr(ack, 2), *(ptr(t, 4) for t in u32), ptr(rows, 64),
        tail.data_ptr() + 8 * PAD, status.data_ptr() + 4 * PAD, 0, None)
    _native.check(rc)
    g = Got()
    for name, t in zip(("accept", "keep", "reply"), u8):
        a = t.cpu().numpy()
        assert (a[:PAD] == SENT8).all() and (a[PAD + n:] == SENT8).all(), name
        setattr(g, name, a[PAD:PAD + n])
    a = ack.cpu().numpy()
    assert (a[:PAD] == SENT16).all() and (a[PAD + n:] == SENT16).all()
    g.reply_ack = a[PAD:PAD + n]
    for name, t, m in zip(("rank", "order", "order_off"), u32, (n, n, n + 1)):
        a = t.cpu().numpy().view(np.uint32)
        assert (a[:PAD] == SENT32).all() and (a[PAD + m:] == SENT32).all(), name
        setattr(g, name, a[PAD:PAD + m])
    w = tail.cpu().numpy().view(np.uint64)
    assert (w[:PAD] == SENT64).all() and (w[PAD + 8:] == SENT64).all()
    g.info = w[PAD:PAD + 8].tolist()
    s = status.cpu().numpy().view(np.uint32)
    assert (s[:PAD] == SENT32).all() and (s[PAD + 1:] == SENT32).all()
    g.status = int(s[PAD])
    r = rows.cpu().numpy().view(np.uint64).reshape(-1, 8)
    A = g.info[0]
    assert A <= n and (r[:PAD] == SENT64).all() and (r[PAD + A:] == SENT64).all()  # nothing past row A - 1
    g.flow_info = r[PAD:PAD + A]
    assert (g.order_off[A + 1:] == SENT32).all()  # nothing past index A
    g.order_off = g.order_off[:A + 1]
    g.states = d_table.cpu().numpy().view(np.uint64)
    return g


def check_against_oracle(g, f, n):
    assert g.accept.tolist() == f.accept.tolist()
    assert g.keep.tolist() == f.keep.tolist()
    assert g.reply.tolist() == f.reply.tolist()
    assert g.reply_ack.tolist() == f.reply_ack.tolist()
    assert g.rank.tolist() == f.rank.tolist()
    assert g.info[:5] == f.info and g.info[6:] == [0, 0]
    if n:
        assert g.order.tolist() == f.order.tolist()
        assert g.order_off.tolist() == f.order_off.tolist()
        assert g.flow_info.tolist() == f.flow_info.tolist()
    assert g.status == f.status
    assert np.array_equal(g.states, f.states)  # the touched rows, and every other row unchanged


def seed_table(rng, table, flow, seq):
    """Rows of a quarter of the active slots start mid-transfer, closed, or with
    the flow's own first seq as the previous ISN (its SYN is then a repeated one)."""
    for slot in sorted(set(flow[flow != FLOW_NONE].tolist())):
        if slot < len(table) and rng.random() < 0.25:
            first = int(seq[np.flatnonzero(flow == slot)[0]])
            table[slot] = rng.choice(((0, 0, 1, 0), (105, 100, 1, 0), (65536, 65530, 1, 0), (0, 0, 0, first + 1),
                                      (0, 0, 0, 70000), (3, 2, 1, first + 1)))
    for slot in range(0, len(table), 97):  # rows no datagram names: they must come back unchanged
        if not (flow == slot).any():
            table[slot] = (slot + 1, slot, 1, slot + 2)


def mix_conditions(f, n, flow):
    """What a batch must contain so that no path can be skipped (from the oracle)."""
    rows = f.flow_info
    runs = {int(r[0]): np.flatnonzero(flow == int(r[0])) for r in rows}
    ended_with_tail = sum(1 for r in rows if r[1] < n and runs[int(r[0])][-1] > r[1])
    return dict(ended_with_tail=ended_with_tail, anomalous=sum(f.anomalous), exact=len(rows) - sum(f.anomalous),
                flowless=f.info[4], restarted=sum(1 for r in rows if r[3] < n), ended=f.info[3])


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", SIZES)
def test_every_flow_count_against_the_oracle(cuda, n):
    rng = random.Random(0xF10 + n)
    for n_active in (1, rng.choice((2, 3)), 37, 300, n):
        n_active = min(n_active, n)
        seq, flags, chars, usable, flow = make_batch(rng, n, n_active, N_FLOWS)
        table = np.zeros((N_FLOWS, 4), np.uint64)
        seed_table(rng, table, flow, seq)
        f = flows_ref(seq, flags, chars, usable, flow, table)
        if n == 1024 and n_active in (37, 300):  # asserted before the device runs
            c = mix_conditions(f, n, flow)
            assert c["ended_with_tail"] >= 1 and c["anomalous"] >= 1 and c["exact"] >= 1, c
            assert c["flowless"] >= 1 and c["restarted"] >= 1 and c["ended"] >= 3, c
            assert {0, N_FLOWS - 1} <= set(flow.tolist())
        g = flows_call(cuda, seq, flags, chars, usable, flow, _table(cuda, table))
        check_against_oracle(g, f, n)
        assert g.info[5] <= sum(f.anomalous)  # only a flow with an anomaly is ever walked


def test_empty_batch_touches_nothing(cuda):
    table = np.arange(40, dtype=np.uint64).reshape(10, 4)
    g = flows_call(cuda, np.zeros(0, np.uint16), np.zeros(0, np.uint8), np.zeros(0, np.uint32), None,
                   np.zeros(0, np.uint32), _table(cuda, table))
    assert g.info == [0] * 8 and g.status == 0 and np.array_equal(g.states, table)


def test_usable_null_and_every_datagram_flowless(cuda):
    rng = random.Random(77)
    seq, flags, chars, usable, flow = make_batch(rng, 130, 9, 64, p_none=0.0)
    table = np.zeros((64, 4), np.uint64)
    g = flows_call(cuda, seq, flags, chars, None, flow, _table(cuda, table))
    check_against_oracle(g, flows_ref(seq, flags, chars, None, flow, table), 130)
    none = np.full(130, FLOW_NONE, np.uint32)
    g = flows_call(cuda, seq, flags, chars, usable, none, _table(cuda, table))
    f = flows_ref(seq, flags, chars, usable, none, table)
    check_against_oracle(g, f, 130)
    assert g.info[:5] == [0, 0, 0, 0, 130] and g.order.tolist() == list(range(130)) and g.order_off.tolist() == [0]


def test_top_rows_of_a_large_table(cuda):
    """2^20 rows, slots only in the top 64: the row address is 64-bit arithmetic
    and the call does no work proportional to the table."""
    import torch
    rng = random.Random(0x100000)
    n_flows = 1 << 20
    slots = rng.sample(range(n_flows - 64, n_flows), 40)
    slots[0] = n_flows - 1
    seq, flags, chars, usable, flow = make_batch(rng, 300, 40, n_flows, slots=slots)
    assert min(flow.tolist()) >= n_flows - 64 and n_flows - 1 in flow.tolist()
    f = flows_ref(seq, flags, chars, usable, flow, np.zeros((n_flows, 4), np.uint64))
    g = flows_call(cuda, seq, flags, chars, usable, flow, torch.zeros((n_flows, 4), dtype=torch.int64, device=cuda))
    check_against_oracle(g, f, 300)
    assert not g.states[:n_flows - 64].any() and g.states[n_flows - 64:].any()


def test_out_of_range_slot_sets_the_status(cuda):
    rng = random.Random(0xBAD)
    seq, flags, chars, usable, flow = make_batch(rng, 257, 37, N_FLOWS)
    victim = int(np.flatnonzero(flow != FLOW_NONE)[11])
    for bad in (N_FLOWS, 0xFFFFFFFE):
        flow2 = flow.copy()
        flow2[victim] = bad
        table = np.zeros((N_FLOWS, 4), np.uint64)
        f = flows_ref(seq, flags, chars, usable, flow2, table)
        assert f.status == ST_FLOW
        g = flows_call(cuda, seq, flags, chars, usable, flow2, _table(cuda, table))
        check_against_oracle(g, f, 257)
        assert g.status == ST_FLOW and g.rank[victim] == RANK_NONE and not g.reply[victim]
    import torch
    d = lambda a: _dev(cuda, a)  # noqa: E731
    flow2[victim] = N_FLOWS
    res = batch.accept_flows(d(seq), d(flags), d(chars.view(np.int32)), d(flow2.view(np.int32)),
                             states=torch.zeros((N_FLOWS, 4), dtype=torch.int64, device=cuda), usable=d(usable))
    with pytest.raises(ValueError, match="flow slot"):
        res.check()


def test_python_refuses_what_the_call_refuses(cuda):
    import torch
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=cuda)  # noqa: E731
    states = batch.flow_states(4, cuda)
    with pytest.raises(ValueError, match="1024"):
        batch.accept_flows(z(1025, torch.uint16), z(1025, torch.uint8), z(1025, torch.int32), z(1025, torch.int32),
                           states=states)
    with pytest.raises(ValueError, match="flow must be"):
        batch.accept_flows(z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32), z(4, torch.int64), states=states)
    with pytest.raises(ValueError, match="states"):
        batch.accept_flows(z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32), z(4, torch.int32),
                           states=torch.zeros((4, 4), dtype=torch.int64))  # on the host
    with pytest.raises(ValueError, match="states"):
        batch.accept_flows(z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32), z(4, torch.int32),
                           states=z(16, torch.int64))
    assert not states.any().item()


# ------------------------------------------------------------ rows carried
def test_rows_carried_over_three_batches(cuda):
    rng = random.Random(0xCA221ED)
    F, n_flows = 12, 64
    slots = rng.sample(range(n_flows), F)
    long = {k: clean_stream(rng, 90, max_chars=3, p_reset=0.0) for k in range(0, F, 3)}  # one transfer, cut in three
    table = np.zeros((n_flows, 4), np.uint64)
    d_table = _table(cuda, table)
    closed = {}
    for b in range(3):
        streams = []
        for k in range(F):
            if k in long:
                streams.append(tuple(a[30 * b:30 * b + 30] for a in long[k]))
            elif b == 0:
                streams.append(clean_stream(rng, 20, fin_at=12 if k % 3 == 1 else None, max_chars=2))
            elif b == 1 and k % 3 == 1:  # the closed ISN's SYN again, then a new transfer
                again = (np.array([closed[k]], np.uint16), np.array([SYN], np.uint8), np.ones(1, np.uint32),
                         np.ones(1, np.uint8))
                new = clean_stream(rng, 19, fin_at=15, max_chars=2)
                streams.append(tuple(np.concatenate(p) for p in zip(again, new)))
            else:
                streams.append(adversarial_stream(rng, 20))
        seq, flags, chars, usable, flow = interleave(rng, streams, slots, p_none=0.0)
        f = flows_ref(seq, flags, chars, usable, flow, table)
        rows = {int(r[0]): r for r in f.flow_info}
        if b == 0:
            closed = {k: int(rows[slots[k]][5]) for k in range(F) if k % 3 == 1}
            assert all(rows[slots[k]][1] < len(seq) for k in closed)  # those flows ended
            assert all(f.states[slots[k]].tolist() == [0, 0, 0, closed[k] + 1] for k in closed)
        if b == 1:
            again = [k for k in closed if rows[slots[k]][3] < len(seq) and int(rows[slots[k]][5]) != closed[k]]
            assert len(again) >= 3  # started again with a new ISN, behind the repeated SYN
            for k in again:
                first = int(np.flatnonzero(flow == slots[k])[0]) if (flow == slots[k]).any() else None
                if first is not None and seq[first] == closed[k] and flags[first] & SYN and usable[first]:
                    assert not f.accept[first] and not f.reply[first]  # a closed flow answers nothing
        for k in long:  # the long transfers carry their state: never a reset after the first batch
            if b and slots[k] in rows:
                assert rows[slots[k]][3] == len(seq)
        g = flows_call(cuda, seq, flags, chars, usable, flow, d_table)
        check_against_oracle(g, f, len(seq))
        table = f.states
    assert all(int(table[slots[k]][2]) == 1 and int(table[slots[k]][0]) > int(table[slots[k]][1]) + 30 for k in long)


# ---------------------------------------------------------------- one flow
@pytest.mark.parametrize("n", (1, 64, 257, 1024))
def test_one_flow_is_accept_inorder(cuda, n):
    import torch
    rng = random.Random(0x1F + n)
    for kind in ("clean", "clean_fin", "adversarial"):
        if kind == "adversarial":
            seq, flags, chars, usable = adversarial_stream(rng, n, p_fin=0.004)
            state, last = rng.choice(((0, 0, 1), (105, 100, 1))), int(seq[0])
        else:
            seq, flags, chars, usable = clean_stream(rng, n, fin_at=n - 1 - n // 3 if kind == "clean_fin" else None,
                                                     max_chars=3)
            state, last = (0, 0, 0), None
        d = [_dev(cuda, seq), _dev(cuda, flags), _dev(cuda, chars.view(np.int32))]
        one = batch.accept_inorder(*d, usable=_dev(cuda, usable), state=state, last_isn=last)
        states = torch.zeros((9, 4), dtype=torch.int64, device=cuda)
        states[5] = torch.tensor([*state, 0 if last is None else last + 1], dtype=torch.int64)
        many = batch.accept_flows(*d, torch.full((n,), 5, dtype=torch.int32, device=cuda), states=states,
                                  usable=_dev(cuda, usable)).check()
        for name in ("accept", "keep", "reply"):
            assert torch.equal(getattr(one, name), getattr(many, name)), (kind, name)
        assert torch.equal(one.reply_ack.view(torch.int16), many.reply_ack.view(torch.int16)), kind
        row, st = states[5].tolist(), one.state.tolist()
        if one.end < n:  # identical up to the turn-over
            assert row == [0, 0, 0, st[1] + 1] and many.ended == 1
        else:
            assert row == st[:3] + [0 if last is None else last + 1] and many.ended == 0
        info = many.flows()
        assert info.shape == (1, 8)
        assert info[0].tolist() == [5, one.end, one.count, one.msg_start, one.characters, st[1],
                                    int(one.keep.sum().item()), 0]
        assert (many.active, many.kept, many.replies, many.flowless) == (1, info[0][6], int(one.reply.sum().item()), 0)
        assert not states[:5].any() and not states[6:].any()


# ------------------------------------------------------------ receive_flows
TEXTS = ("héllo wörld, ça va?", "日本語のテキストです", "plain ascii text here", "😀 emoji 😀 mix ñ", "x")


def _flow_frames(rng, text, isn, fin):
    """(seq, flags, payload bytes) of a stop-and-wait sender's datagrams for one
    text, 1-3 characters each, some sent twice."""
    out, k = [], 0
    while k < len(text) or not out:
        c = rng.randint(1, 3)
        piece = text[k:k + c]
        fl = (SYN if k == 0 else 0) | (FIN if fin and k + c >= len(text) else 0)
        out.append(((isn + k) & 0xFFFF, fl, piece.encode()))
        if rng.random() < 0.3:
            out.append(((isn + k) & 0xFFFF, fl & ~FIN & 0xFF, piece.encode()))
        k += c
    return out


def _receive_case(rng, n, slots):
    """n datagrams of len(slots) flows in one arrival order, as (seq, flags,
    payload, slot) rows, and the datagrams to damage: three checksums, one
    payload that is not UTF-8 and one without a flow, each a datagram whose
    sender sent it twice, so its flow goes on with the other copy."""
    per = []
    while sum(map(len, per)) != n:
        per = [_flow_frames(rng, TEXTS[k] * rng.randint(1, 2), rng.randint(1, 5000), fin=k % 2 == 0)
               for k in range(len(slots))]
    pick = arrival_order(rng, [len(p) for p in per])
    at, rows = [0] * len(slots), []
    for k in pick:
        rows.append((*per[k][at[k]], slots[k]))
        at[k] += 1
    twice = [i for i, r in enumerate(rows) if not r[1] & FIN
             and sum(1 for q in rows if (q[0], q[3]) == (r[0], r[3])) == 2]
    firsts = [i for i in twice if not any((rows[j][0], rows[j][3]) == (rows[i][0], rows[i][3]) for j in range(i))]
    chosen = rng.sample(firsts, 5)
    bad_utf8 = chosen[3]
    rows[bad_utf8] = (rows[bad_utf8][0], rows[bad_utf8][1], b"\xff\xfe", rows[bad_utf8][3])
    return rows, sorted(chosen[:3]), bad_utf8, chosen[4]


@pytest.mark.parametrize("layout", ("rudp5", "rudp7"))
def test_receive_flows_frames_to_messages_and_replies(cuda, layout):
    import torch
    from oracle import codec_np
    from rudp.transport import build
    H = 5 if layout == "rudp5" else 7
    rng = random.Random(0x2EC + H)
    n, slots = 65, [3, 0, 11, 7, 4]
    rows, bad_sum, bad_utf8, lost = _receive_case(rng, n, slots)
    seq = np.array([r[0] for r in rows], np.uint16)
    flags = np.array([r[1] for r in rows], np.uint8)
    flow = np.array([r[3] for r in rows], np.uint32)
    flow[lost] = FLOW_NONE
    payloads = [r[2] for r in rows]
    lens = np.array([len(p) for p in payloads], np.int32)
    packed = batch.pack_batch_varlen((_dev(cuda, seq), _dev(cuda, np.zeros(n, np.uint16)), _dev(cuda, flags)),
                                     _dev(cuda, np.frombuffer(b"".join(payloads), np.uint8).copy()), _dev(cuda, lens),
                                     layout, want_csum=H == 5)
    frames, off = packed.frames.clone(), packed.frame_off
    h_off = off.cpu().numpy()
    csum = None
    if H == 7:
        for i in bad_sum:  # a payload byte damaged in flight (still UTF-8: only the checksum objects)
            frames[int(h_off[i]) + H] ^= 0x01
    else:
        h_csum = packed.csum.cpu().numpy().copy()
        for i in bad_sum:
            h_csum[i] ^= 0x0100
        csum = _dev(cuda, h_csum)
    h_frames = frames.cpu().numpy()
    usable = np.ones(n, np.uint8)
    usable[bad_sum] = 0
    usable[bad_utf8] = 0
    chars = chars_ref(h_frames, h_off, H)
    table = np.zeros((12, 4), np.uint64)
    f = flows_ref(seq, flags, chars, usable, flow, table)
    assert f.info[3] >= 2 and f.info[4] == 1 and f.info[0] == 5
    states = batch.flow_states(12, cuda)
    res = batch.receive_flows(frames, off, _dev(cuda, flow.view(np.int32)), layout, states=states, csum=csum)
    res.accepted.check()
    res.pieces.check()
    assert res.usable.cpu().numpy().tolist() == usable.tolist()
    assert res.chars.cpu().numpy().view(np.uint32).tolist() == chars.tolist()
    acc = res.accepted
    assert acc.keep.cpu().numpy().tolist() == f.keep.tolist()
    assert acc.rank.cpu().numpy().view(np.uint32).tolist() == f.rank.tolist()
    assert np.array_equal(acc.flows().view(np.uint64), f.flow_info)
    assert np.array_equal(states.cpu().numpy().view(np.uint64), f.states)
    assert (acc.active, acc.kept, acc.replies, acc.ended, acc.flowless) == tuple(f.info)
    whole = b""
    for a, row in enumerate(f.flow_info.tolist()):
        want = b"".join(payloads[i] for i in np.flatnonzero(flow == row[0]) if f.keep[i])
        assert res.message(a) == want, a
        whole += want
        want.decode()  # every piece is whole characters
    assert res.pieces.payload.cpu().numpy().tobytes() == whole
    idx = np.flatnonzero(f.reply)
    assert res.reply_index.cpu().numpy().tolist() == idx.tolist() and res.reply_count == len(idx)
    R = len(idx)
    want_frames, _, _ = codec_np.encode_varlen(np.zeros(R, np.uint16), f.reply_ack[idx], np.full(R, ACK, np.uint8),
                                               [b""] * R, H)
    got = res.reply_frames(layout).cpu().numpy()
    assert got.tobytes() == want_frames.tobytes()
    if H == 5:
        assert got.tobytes() == b"".join(build(0, int(a), ACK) for a in f.reply_ack[idx])


# ------------------------------------------------------------------ capture
def test_accept_flows_under_stream_capture(cuda):
    import torch
    rng = random.Random(0xCA9)
    n = 257
    seq, flags, chars, usable, flow = make_batch(rng, n, 37, N_FLOWS)
    table = np.zeros((N_FLOWS, 4), np.uint64)
    f = flows_ref(seq, flags, chars, usable, flow, table)
    d = [_dev(cuda, seq), _dev(cuda, flags), _dev(cuda, chars.view(np.int32)), _dev(cuda, flow.view(np.int32))]
    d_us = _dev(cuda, usable)
    states = batch.flow_states(N_FLOWS, cuda)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            res = batch.accept_flows(*d, states=states, usable=d_us)
    torch.cuda.current_stream(cuda).wait_stream(side)
    for _ in range(2):  # replayed on a fresh table both times: the same outputs
        states.zero_()
        res._buf.fill_(0xEE)
        graph.replay()
        torch.cuda.synchronize(cuda)
        assert res.accept.cpu().numpy().tolist() == f.accept.tolist()
        assert res.keep.cpu().numpy().tolist() == f.keep.tolist()
        assert res.reply_ack.cpu().numpy().tolist() == f.reply_ack.tolist()
        assert res.rank.cpu().numpy().view(np.uint32).tolist() == f.rank.tolist()
        A = f.info[0]
        assert res.order.cpu().numpy().view(np.uint32).tolist() == f.order.tolist()
        assert res.order_off.cpu().numpy().view(np.uint32)[:A + 1].tolist() == f.order_off.tolist()
        assert np.array_equal(res.flow_info.cpu().numpy().view(np.uint64)[:A], f.flow_info)
        assert res.info.cpu().numpy().tolist()[:5] == f.info and int(res.status.item()) == 0
        assert np.array_equal(states.cpu().numpy().view(np.uint64), f.states)
