"""rudp_ack_flows / batch.ack_flows / batch.acknowledge_flows on the device:
every output bit for bit against the oracle (tests/ack_flows_ref.py: ack_ref per
flow) for every batch size around the kernel's thread and tile edges, flow
counts from one flow to a flow per reply and both modes, one flow against
rudp_ack_progress, rows carried over three batches with a host timeout in
between, the ends of a large table, refused rows and slots, the closing
datagrams in both layouts, the chain from reply datagrams, and stream capture."""
import random

import numpy as np
import pytest

from ack_flows_ref import (CUMULATIVE, EXACT, FLOW_NONE, ST_FLOW, ST_FLOW_ROW, ack_flows_ref, make_reply_batch,
                           open_row)
from ack_ref import ACK, FIN, adversarial_replies, clean_replies, fresh_state, header, csum_of, pack_frames
from flows_ref import arrival_order
from rudp import _native, batch

pytestmark = pytest.mark.gpu

SENT8, SENT16, SENT32, SENT64 = 0xA5, 0xA5A5, 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
PAD = 8  # sentinel entries on either side of every output
N_FLOWS = 5000
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
MODES = {EXACT: _native.ACK_EXACT, CUMULATIVE: _native.ACK_CUMULATIVE}


# ----------------------------------------------------------------- helpers
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _table(cuda, table):
    return _dev(cuda, np.asarray(table, np.uint64).view(np.int64))


class Got:
    pass


def flows_call(cuda, seq, ack, flags, usable, flow, d_table, mode=EXACT, H=0):
    """rudp_ack_flows with every output between sentinels; d_table (int64
    [n_flows, 8] on the device) is updated in place."""
    import torch
    n = len(ack)
    d_in = [_dev(cuda, seq), _dev(cuda, ack), _dev(cuda, flags), _dev(cuda, usable) if usable is not None else None,
            _dev(cuda, np.asarray(flow, np.uint32).view(np.int32))]
    valid = torch.full((n + 2 * PAD,), SENT8, dtype=torch.uint8, device=cuda)
    pointer = _dev(cuda, np.full(n + 2 * PAD, SENT64, np.uint64).view(np.int64))
    u32 = [_dev(cuda, np.full(m + 2 * PAD, SENT32, np.uint32).view(np.int32)) for m in (n, n + 1, n)]
    rows = _dev(cuda, np.full(8 * (n + 2 * PAD), SENT64, np.uint64).view(np.int64))
    tail = _dev(cuda, np.full(8 + 2 * PAD, SENT64, np.uint64).view(np.int64))
    status = _dev(cuda, np.full(1 + 2 * PAD, SENT32, np.uint32).view(np.int32))
    fin = torch.full((n * max(H, 1) + 2 * PAD,), SENT8, dtype=torch.uint8, device=cuda)
    fcs = _dev(cuda, np.full(n + 2 * PAD, SENT16, np.uint16))

    def ptr(t, width, on=True):
        return t.data_ptr() + width * PAD if n and on else None

    rc = _native.lib().rudp_ack_flows(
        *(t.data_ptr() if t is not None and n else None for t in d_in), n, MODES[mode], d_table.data_ptr(),
        d_table.shape[0], ptr(valid, 1), ptr(pointer, 8), ptr(u32[0], 4), ptr(u32[1], 4), ptr(rows, 64),
        tail.data_ptr() + 8 * PAD, status.data_ptr() + 4 * PAD, H, ptr(fin, 1, H), ptr(fcs, 2, H), ptr(u32[2], 4, H),
        0, None)
    _native.check(rc)
    g = Got()
    a = valid.cpu().numpy()
    assert (a[:PAD] == SENT8).all() and (a[PAD + n:] == SENT8).all()
    g.valid = a[PAD:PAD + n]
    a = pointer.cpu().numpy().view(np.uint64)
    assert (a[:PAD] == SENT64).all() and (a[PAD + n:] == SENT64).all()
    g.pointer = a[PAD:PAD + n]
    w = tail.cpu().numpy().view(np.uint64)
    assert (w[:PAD] == SENT64).all() and (w[PAD + 8:] == SENT64).all()
    g.info = w[PAD:PAD + 8].tolist()
    A, E = g.info[0], g.info[2]
    for name, t, m, used in zip(("order", "order_off", "final_flow"), u32, (n, n + 1, n),
                                (n, A + 1 if n else 0, E if H else 0)):
        a = t.cpu().numpy().view(np.uint32)
        assert (a[:PAD] == SENT32).all() and (a[PAD + used:] == SENT32).all(), name  # nothing past what is used
        setattr(g, name, a[PAD:PAD + used])
    s = status.cpu().numpy().view(np.uint32)
    assert (s[:PAD] == SENT32).all() and (s[PAD + 1:] == SENT32).all()
    g.status = int(s[PAD])
    r = rows.cpu().numpy().view(np.uint64).reshape(-1, 8)
    assert A <= n and (r[:PAD] == SENT64).all() and (r[PAD + A:] == SENT64).all()  # nothing past row A - 1
    g.flow_info = r[PAD:PAD + A]
    a = fin.cpu().numpy()
    used = E * H
    assert (a[:PAD] == SENT8).all() and (a[PAD + used:] == SENT8).all()  # nothing at or past E * layout
    g.final_frames = a[PAD:PAD + used].tobytes()
    a = fcs.cpu().numpy()
    assert (a[:PAD] == SENT16).all() and (a[PAD + (E if H else 0):] == SENT16).all()
    g.final_csum = a[PAD:PAD + (E if H else 0)]
    g.states = d_table.cpu().numpy().view(np.uint64)
    return g


def check_against_oracle(g, f, n, H=0):
    assert g.valid.tolist() == f.valid.tolist()
    assert g.pointer.tolist() == f.pointer.tolist()
    assert g.info[:5] == f.info and g.info[6:] == [0, 0]
    if n:
        assert g.order.tolist() == f.order.tolist()
        assert g.order_off.tolist() == f.order_off.tolist()
        assert g.flow_info.tolist() == f.flow_info.tolist()
    assert g.status == f.status
    assert np.array_equal(g.states, f.states)  # words 0 to 3 of the judged rows, and everything else unchanged
    assert g.info[5] == sum(f.anomalous)  # exactly the flows with an anomaly before their end are walked
    if H:
        assert g.final_flow.tolist() == [a for a, _, _ in f.finals]
        assert g.final_frames == b"".join(header(s, k, ACK, H) for _, s, k in f.finals)
        assert g.final_csum.tolist() == [csum_of(s, k, ACK) for _, s, k in f.finals]


def seed_table(rng, table, flow, mode):
    """Rows of a fifth of the judged slots start mid-transfer or from a state
    that is not canonical (L dropped to 0, last wrong or not 0 / 1, p off the
    grid), p + L never past T (beyond T the reference's L would be negative);
    rows no reply names must come back unchanged."""
    for slot in sorted(set(flow[flow != FLOW_NONE].tolist())):
        isn, T, C = (int(v) for v in table[slot][4:7])
        if C and not table[slot][3] and rng.random() < 0.2:
            p = min(T, C * rng.randint(0, 3))
            L = min(C, T - p)
            last = int(p + L == T)
            table[slot, :4] = rng.choice(((p, L, last, 0), (p, 0, 1, 0), (p, L, 7 * last, 0), (p, L, 1 - last, 0),
                                          (p - 1, 1, 0, 0) if p and C > 1 else (p, L, last, 0)))
    for slot in range(0, len(table), 97):
        if not (flow == slot).any():
            table[slot] = (slot + 1, slot, 1, 0, slot, 10 * slot, 7, 3)


KINDS = ("anomalous", "plain", "ended_early", "done", "idle")


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("mode", (EXACT, CUMULATIVE))
@pytest.mark.parametrize("n", SIZES)
def test_every_flow_count_against_the_oracle(cuda, n, mode):
    rng = random.Random(0xAF10 + n + (mode == CUMULATIVE))
    H = (0, 5, 7)[n % 3]
    few = {k: 0 for k in KINDS}
    plans = [(1, {}, ()), (1, {}, (0,)), (1, {}, (0,)), (1, {0: "done"}, ()), (1, {0: "idle"}, ()), (2, {}, (1,)),
             (2, {}, (0, 1)), (2, {0: "done", 1: "idle"}, ()), (37, None, ()), (n, None, ())]
    for n_active, special, adversarial in plans:
        n_active = min(n_active, n)
        seq, ack, flags, usable, flow, table = make_reply_batch(rng, n, n_active, mode, N_FLOWS, special=special,
                                                                adversarial=adversarial)
        if n_active > 2:
            seed_table(rng, table, flow, mode)
        f = ack_flows_ref(seq, ack, flags, usable, flow, table, mode)
        if n >= 255 and n_active > 2:  # asserted before the device runs
            # (with a flow per reply no reply follows a flow's end: that kind is the 37-flow mix's)
            assert all(f.kinds[k] >= 1 for k in KINDS if n_active == 37 or k != "ended_early"), f.kinds
            assert (n_active == n or (flow == FLOW_NONE).any()) and {0, N_FLOWS - 1} <= set(flow.tolist())
        elif n_active <= 2:
            for k in KINDS:
                few[k] += f.kinds[k]
        g = flows_call(cuda, seq, ack, flags, usable, flow, _table(cuda, table), mode, H)
        check_against_oracle(g, f, n, H)
    if n >= 255:  # at one and two flows the condition is split over the batches
        assert all(few[k] >= 1 for k in KINDS), few


def test_empty_batch_touches_nothing(cuda):
    table = np.arange(80, dtype=np.uint64).reshape(10, 8)
    for H in (0, 7):
        g = flows_call(cuda, np.zeros(0, np.uint16), np.zeros(0, np.uint16), np.zeros(0, np.uint8), None,
                       np.zeros(0, np.uint32), _table(cuda, table), EXACT, H)
        assert g.info == [0] * 8 and g.status == 0 and np.array_equal(g.states, table)


@pytest.mark.parametrize("mode", (EXACT, CUMULATIVE))
def test_usable_null_and_every_reply_flowless(cuda, mode):
    rng = random.Random(77)
    seq, ack, flags, usable, flow, table = make_reply_batch(rng, 130, 9, mode, 64, p_none=0.0)
    g = flows_call(cuda, seq, ack, flags, None, flow, _table(cuda, table), mode, 5)
    check_against_oracle(g, ack_flows_ref(seq, ack, flags, None, flow, table, mode), 130, 5)
    none = np.full(130, FLOW_NONE, np.uint32)
    g = flows_call(cuda, seq, ack, flags, usable, none, _table(cuda, table), mode, 5)
    f = ack_flows_ref(seq, ack, flags, usable, none, table, mode)
    check_against_oracle(g, f, 130, 5)
    assert g.info[:5] == [0, 0, 0, 0, 130] and g.order.tolist() == list(range(130)) and g.order_off.tolist() == [0]
    assert np.array_equal(g.states, table)


def test_first_and_last_row_of_a_5000_row_table(cuda):
    rng = random.Random(0x5000)
    for mode in (EXACT, CUMULATIVE):
        seq, ack, flags, usable, flow, table = make_reply_batch(rng, 200, 2, mode, N_FLOWS, special={},
                                                                slots=[N_FLOWS - 1, 0])
        assert set(flow.tolist()) - {FLOW_NONE} == {0, N_FLOWS - 1}
        f = ack_flows_ref(seq, ack, flags, usable, flow, table, mode)
        g = flows_call(cuda, seq, ack, flags, usable, flow, _table(cuda, table), mode, 7)
        check_against_oracle(g, f, 200, 7)
        assert g.flow_info[:, 0].tolist() == [0, N_FLOWS - 1] and not g.states[1:N_FLOWS - 1].any()


def test_out_of_range_slot_and_refused_rows(cuda):
    rng = random.Random(0xBAD)
    for mode in (EXACT, CUMULATIVE):
        seq, ack, flags, usable, flow, table = make_reply_batch(rng, 257, 37, mode, N_FLOWS)
        good = ack_flows_ref(seq, ack, flags, usable, flow, table, mode)
        victim = int(np.flatnonzero(flow != FLOW_NONE)[11])
        for bad in (N_FLOWS, 0xFFFFFFFE):
            flow2 = flow.copy()
            flow2[victim] = bad
            f = ack_flows_ref(seq, ack, flags, usable, flow2, table, mode)
            assert f.status == ST_FLOW
            g = flows_call(cuda, seq, ack, flags, usable, flow2, _table(cuda, table), mode, 5)
            check_against_oracle(g, f, 257, 5)
            assert g.status == ST_FLOW and not g.valid[victim] and not g.pointer[victim]
        slot = int(good.flow_info[4][0])
        ways = [(4, 65536), (6, 16384), (6, 1 << 40)] + ([(7, int(table[slot][5]) + 1)] if mode == CUMULATIVE else [])
        for word, value in ways:
            t2 = table.copy()
            t2[slot, word] = value
            f = ack_flows_ref(seq, ack, flags, usable, flow, t2, mode)
            assert f.status == ST_FLOW_ROW and slot not in f.flow_info[:, 0].tolist()
            g = flows_call(cuda, seq, ack, flags, usable, flow, _table(cuda, t2), mode, 7)
            check_against_oracle(g, f, 257, 7)
        t2 = table.copy()
        t2[slot, 4] = 70000
        flow2 = flow.copy()
        flow2[victim] = N_FLOWS  # both bits at once
        f = ack_flows_ref(seq, ack, flags, usable, flow2, t2, mode)
        assert f.status == ST_FLOW | ST_FLOW_ROW
        check_against_oracle(flows_call(cuda, seq, ack, flags, usable, flow2, _table(cuda, t2), mode), f, 257)
        if mode == EXACT:  # sent is not read
            t2 = table.copy()
            t2[slot, 7] = int(table[slot][5]) + 1
            f = ack_flows_ref(seq, ack, flags, usable, flow, t2, mode)
            assert f.status == 0
            check_against_oracle(flows_call(cuda, seq, ack, flags, usable, flow, _table(cuda, t2), mode), f, 257)
    d = lambda a: _dev(cuda, a)  # noqa: E731
    res = batch.ack_flows(d(seq), d(ack), d(flags), d(flow2.view(np.int32)), states=_table(cuda, table),
                          usable=d(usable), mode=mode)
    with pytest.raises(ValueError, match="flow slot"):
        res.check()


def test_python_refuses_what_the_call_refuses(cuda):
    import torch
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=cuda)  # noqa: E731
    states = batch.ack_flow_states(4, cuda)
    with pytest.raises(ValueError, match="1024"):
        batch.ack_flows(z(1025, torch.uint16), z(1025, torch.uint16), z(1025, torch.uint8), z(1025, torch.int32),
                        states=states)
    with pytest.raises(ValueError, match="flow must be"):
        batch.ack_flows(z(4, torch.uint16), z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int64), states=states)
    with pytest.raises(ValueError, match="states"):
        batch.ack_flows(z(4, torch.uint16), z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32),
                        states=batch.flow_states(4, cuda))  # the receiver's table
    with pytest.raises(ValueError, match="mode"):
        batch.ack_flows(z(4, torch.uint16), z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32), states=states,
                        mode="window")
    with pytest.raises(ValueError, match="layout"):
        batch.ack_flows(z(4, torch.uint16), z(4, torch.uint16), z(4, torch.uint8), z(4, torch.int32), states=states,
                        final_layout="rudp9")
    with pytest.raises(ValueError, match="1024"):
        batch.acknowledge_flows(z(8, torch.uint8), z(1026, torch.int64), z(1025, torch.int32), "rudp5", states=states)
    assert not states.any().item()
    batch.ack_flow_open(states, 2, 65535, 300, 16)
    assert states.cpu().tolist()[2] == open_row(65535, 300, 16) and not states[:2].any().item()


# ------------------------------------------------------------ rows carried
@pytest.mark.parametrize("mode", (EXACT, CUMULATIVE))
def test_rows_carried_over_three_batches_with_a_timeout_between(cuda, mode):
    """Transfers cut in three batches carry their rows on the device; between
    the second and the third the host's timeout rewrites words 0 to 3 of some
    rows to (p, L, last, 0), as the sender does when it goes back to p."""
    rng = random.Random(0xCA221ED + (mode == CUMULATIVE))
    F, n_flows = 12, 64
    slots = rng.sample(range(n_flows), F)
    table = np.zeros((n_flows, 8), np.uint64)
    streams = []
    for k in range(F):
        C = rng.choice((1, 3, 16))
        T, isn = 40 * C + (k % 2), rng.choice((5, 65000, 65535 - 20 * C))
        table[slots[k]] = open_row(isn, T, C, T if mode == CUMULATIVE else 0)
        streams.append(adversarial_replies(rng, 90, isn=isn, T=T, C=C) if k % 4 == 3
                       else clean_replies(rng, 90, isn=isn, T=T, C=C, W=4, fin=k % 3 == 0))
    d_table = _table(cuda, table)
    progressed = 0
    for b in range(3):
        lens = [30] * F
        pick = arrival_order(rng, lens)
        at = [30 * b] * F
        cols = [[], [], [], [], []]
        for k in pick:
            for c in range(4):
                cols[c].append(streams[k][c][at[k]])
            cols[4].append(slots[k])
            at[k] += 1
        seq, ack = np.array(cols[0], np.uint16), np.array(cols[1], np.uint16)
        flags, usable, flow = np.array(cols[2], np.uint8), np.array(cols[3], np.uint8), np.array(cols[4], np.uint32)
        if b == 2:  # the timeout: L and last recomputed from p, on the device table as on the oracle's
            import torch
            for k in range(0, F, 2):
                p, _, _, done, _, T, C, _ = (int(v) for v in table[slots[k]])
                if not done:
                    L = min(C, T - p) if p <= T else 0
                    table[slots[k], :4] = (p, L, int(p + L == T), 0)
                    d_table[slots[k], :4] = torch.tensor([p, L, int(p + L == T), 0], dtype=torch.int64)
        f = ack_flows_ref(seq, ack, flags, usable, flow, table, mode)
        g = flows_call(cuda, seq, ack, flags, usable, flow, d_table, mode, 5)
        check_against_oracle(g, f, len(ack), 5)
        progressed += sum(1 for r in f.flow_info if r[3] > 0 and b > 0)
        table = f.states
    assert progressed >= 6  # the carried rows went on from where the batch before left them


# ---------------------------------------------------------------- one flow
@pytest.mark.parametrize("mode", (EXACT, CUMULATIVE))
@pytest.mark.parametrize("n", (1, 64, 257, 1024))
def test_one_flow_is_ack_progress(cuda, n, mode):
    import torch
    rng = random.Random(0x1F + n)
    C, isn = 3, 65000
    T = 3 * n + 1
    for kind, state in (("clean", None), ("clean_mid", (6, 3, 0, 0)), ("adversarial", None),
                        ("off_grid", (4, 3, 0, 0)), ("no_length", (3, 0, 1, 0))):
        if kind.startswith("clean"):
            seq, ack, flags, usable = clean_replies(rng, n, isn=isn, T=T if n < 300 else 300, C=C, W=4, state=state)
            Tk = T if n < 300 else 300
        else:
            Tk = 30
            seq, ack, flags, usable = adversarial_replies(rng, n, isn=isn, T=Tk, C=C)
        st = fresh_state(Tk, C) if state is None else state
        d = [_dev(cuda, seq), _dev(cuda, ack), _dev(cuda, flags)]
        one = batch.ack_progress(*d, isn=isn, total_chars=Tk, chunk=C, usable=_dev(cuda, usable), state=st, mode=mode,
                                 sent=Tk)
        states = batch.ack_flow_states(9, cuda)
        states[5] = torch.tensor([*st, isn, Tk, C, Tk], dtype=torch.int64)
        many = batch.ack_flows(*d, torch.full((n,), 5, dtype=torch.int32, device=cuda), states=states,
                               usable=_dev(cuda, usable), mode=mode, final_layout="rudp7").check()
        assert torch.equal(one.valid, many.valid), kind
        assert torch.equal(one.pointer, many.pointer), kind
        assert states[5].tolist() == one.state.tolist() + [isn, Tk, C, Tk], kind
        info = many.flows()
        assert info.shape == (1, 8)
        assert info[0].tolist()[:7] == [5, one.end, one.count, one.newly_acknowledged, one.pointer_after,
                                        one.next_frame, int(one.done)], kind
        assert (many.active, many.count, many.ended, many.newly_acknowledged, many.flowless) == (
            1, one.count, int(one.end < n), one.newly_acknowledged, 0)
        assert int(many.info[5].item()) == int(not one.fast), kind  # walked exactly when ack_progress was
        if one.end < n:
            want = header((isn + one.pointer_after) & 0xFFFF, (int(seq[one.end]) + 1) & 0xFFFF, ACK, 7)
            assert many.finals() == [(0, want)], kind
        else:
            assert many.finals() == [] and info[0][7] == 0
        assert not states[:5].any() and not states[6:].any()


# ------------------------------------------------------- acknowledge_flows
@pytest.mark.parametrize("layout", ("rudp5", "rudp7"))
def test_acknowledge_flows_from_reply_datagrams(cuda, layout):
    import torch
    H = 5 if layout == "rudp5" else 7
    rng = random.Random(0xACF + H)
    seq, ack, flags, usable, flow, table = make_reply_batch(rng, 200, 12, EXACT, 40, p_none=0.05)
    frames = [header(int(s), int(a), int(f), H) for s, a, f in zip(seq, ack, flags)]
    short, wrong = [i for i in range(200) if not usable[i]][:2]
    frames[short] = frames[short][:H - 2]
    csum = None
    if H == 7:
        frames[wrong] = frames[wrong][:5] + bytes([frames[wrong][5] ^ 0x10, frames[wrong][6]])
    else:
        h_csum = np.array([csum_of(int(s), int(a), int(f)) for s, a, f in zip(seq, ack, flags)], np.uint16)
        h_csum[wrong] ^= 0x0100
        csum = _dev(cuda, h_csum)
    buf, off = pack_frames(frames)
    bad_off = int(np.flatnonzero(usable)[17])
    off = off.copy()
    # decreasing offsets: frame bad_off goes backwards (the frame before it takes one byte more and fails its checksum)
    off[bad_off] = off[bad_off + 1] + 1
    d_table = _table(cuda, table)
    res = batch.acknowledge_flows(_dev(cuda, buf), _dev(cuda, off), _dev(cuda, flow.view(np.int32)), layout,
                                  states=d_table, csum=csum)
    ok = res.decoded.ok.cpu().numpy()
    assert ok[short] == _native.OK_SHORT and ok[wrong] == _native.OK_BAD_CSUM
    assert ok[bad_off] == _native.OK_BAD_OFFSETS
    assert int(res.decoded.status.item()) == _native.ST_OFFSETS
    got_us = res.usable.cpu().numpy()
    assert got_us.tolist() == [int(o in (_native.OK_GOOD, _native.OK_UNVERIFIED)) for o in ok]
    assert not got_us[[short, wrong, bad_off]].any() and got_us.sum() >= 196
    # the rule's inputs are what the decode made of the datagrams
    d_seq = res.decoded.seq.view(torch.int16).cpu().numpy().view(np.uint16)
    d_ack = res.decoded.ack.view(torch.int16).cpu().numpy().view(np.uint16)
    d_fl = res.decoded.flags.cpu().numpy()
    good = np.flatnonzero(got_us)
    assert d_seq[good].tolist() == seq[good].tolist() and d_ack[good].tolist() == ack[good].tolist()
    assert d_fl[good].tolist() == flags[good].tolist()
    f = ack_flows_ref(d_seq, d_ack, d_fl, got_us, flow, table)
    j = res.judged.check()
    assert j.valid.cpu().numpy().tolist() == f.valid.tolist()
    assert j.pointer.cpu().numpy().view(np.uint64).tolist() == f.pointer.tolist()
    assert np.array_equal(j.flows().view(np.uint64), f.flow_info)
    assert (j.active, j.count, j.ended, j.newly_acknowledged, j.flowless) == tuple(f.info)
    assert j.ended >= 2
    assert j.finals() == [(a, header(s, k, ACK, H)) for a, s, k in f.finals]
    assert np.array_equal(d_table.cpu().numpy().view(np.uint64), f.states)


# ------------------------------------------------------------------ capture
def test_ack_flows_under_stream_capture(cuda):
    import torch
    rng = random.Random(0xCA9)
    n = 257
    seq, ack, flags, usable, flow, table = make_reply_batch(rng, n, 37, CUMULATIVE, N_FLOWS)
    f = ack_flows_ref(seq, ack, flags, usable, flow, table, CUMULATIVE)
    assert f.info[2] >= 2 and sum(f.anomalous) >= 1
    d = [_dev(cuda, seq), _dev(cuda, ack), _dev(cuda, flags), _dev(cuda, flow.view(np.int32))]
    d_us = _dev(cuda, usable)
    fresh = _table(cuda, table)
    states = fresh.clone()
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            res = batch.ack_flows(*d, states=states, usable=d_us, mode="cumulative", final_layout="rudp7")
    torch.cuda.current_stream(cuda).wait_stream(side)
    states.copy_(fresh)
    res._buf.fill_(0xEE)
    graph.replay()  # replayed once, on the fresh table
    torch.cuda.synchronize(cuda)
    A, E = f.info[0], f.info[2]
    assert res.valid.cpu().numpy().tolist() == f.valid.tolist()
    assert res.pointer.cpu().numpy().view(np.uint64).tolist() == f.pointer.tolist()
    assert res.order.cpu().numpy().view(np.uint32).tolist() == f.order.tolist()
    assert res.order_off.cpu().numpy().view(np.uint32)[:A + 1].tolist() == f.order_off.tolist()
    assert np.array_equal(res.flow_info.cpu().numpy().view(np.uint64)[:A], f.flow_info)
    assert res.info.cpu().numpy().tolist()[:5] == f.info and int(res.status.item()) == 0
    assert res.final_frames.cpu().numpy()[:E].tobytes() == b"".join(header(s, k, ACK, 7) for _, s, k in f.finals)
    assert res.final_flow.cpu().numpy()[:E].tolist() == [a for a, _, _ in f.finals]
    assert np.array_equal(states.cpu().numpy().view(np.uint64), f.states)
