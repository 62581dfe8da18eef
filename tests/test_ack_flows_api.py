"""rudp_ack_flows (added within ABI 8) at the boundary: the symbol and the
header's defines, the argument checks that run before any device call, the
Python validation, ``FlowTable.lookup``, and the oracle (tests/ack_flows_ref.py)
against the single-transfer rule and the reply streams the reference judged.
CPU-only."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from ack_flows_ref import (CUMULATIVE, EXACT, FLOW_NONE, ST_FLOW, ST_FLOW_ROW, ack_flows_ref, make_reply_batch,
                           open_row)
from ack_ref import ACK, adversarial_replies, ack_ref, clean_replies, fresh_state, golden_cases, parse_rudp5
from conftest import REPO
from flows_ref import arrival_order
from rudp import _native, batch, flows

NAME = "rudp_ack_flows"


def test_symbol_and_header():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    for define in (r"RUDP_HAS_ACK_FLOWS 1", r"RUDP_ABI_VERSION 8", r"RUDP_ST_FLOW_ROW 512u",
                   r"RUDP_FLOWS_MAX_BATCH 1024u"):
        assert re.search(rf"^#define {define}\b", text, flags=re.M), define
    assert hasattr(lib, NAME) and NAME in _native.EXPORTS
    assert re.search(rf"^RUDP_API int {NAME}\(", text, flags=re.M)
    assert _native.ST_FLOW_ROW == ST_FLOW_ROW == 512 and ST_FLOW == _native.ST_FLOW
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == NAME and ln.split()[1] == "T" for ln in out.splitlines()), path
    # the kernel holds exactly one batch, within the LDS a workgroup gets without asking
    hpp = (REPO / "reliable-udp_amd" / "csrc" / "ack_flows_device.hpp").read_text()
    assert "constexpr uint32_t kAfMax = kBlock * kAfFpt;" in hpp and "constexpr uint32_t kAfFpt = 4;" in hpp
    hip = (REPO / "reliable-udp_amd" / "csrc" / "ack_flows.hip").read_text()
    assert "static_assert(sizeof(AckFlowLds) <= 65536" in hip


NAMES = ("seq", "ack", "flags", "flow", "states", "valid", "pointer", "order", "order_off", "flow_info", "info",
         "status", "final_frames", "final_csum", "final_flow")


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    p = ctypes.cast(word, ctypes.c_void_p)

    def call(n=1, n_flows=4, mode=0, final_layout=5, **kw):
        a = {k: kw.get(k, p) for k in NAMES}
        return lib.rudp_ack_flows(a["seq"], a["ack"], a["flags"], None, a["flow"], n, mode, a["states"], n_flows,
                                  a["valid"], a["pointer"], a["order"], a["order_off"], a["flow_info"], a["info"],
                                  a["status"], final_layout, a["final_frames"], a["final_csum"], a["final_flow"],
                                  0, None)

    for kw in ("states", "info", "status"):
        for n in (0, 1):
            assert call(n=n, **{kw: None}) == _native.EINVAL
            assert f"d_{kw}".encode() in lib.rudp_last_error()
    for n_flows in (0, 0xFFFFFFFF, 1 << 40):
        for n in (0, 1):
            assert call(n=n, n_flows=n_flows) == _native.EINVAL and b"n_flows" in lib.rudp_last_error()
    for mode in (-1, 2, 7):
        assert call(mode=mode) == _native.EINVAL and b"mode" in lib.rudp_last_error()
        assert call(n=0, mode=mode) == _native.EINVAL
    for final_layout in (-1, 1, 6, 8):
        assert call(final_layout=final_layout) == _native.EINVAL and b"final_layout" in lib.rudp_last_error()
        assert call(n=0, final_layout=final_layout) == _native.EINVAL
    for final_layout in (5, 7):
        for kw in NAMES:
            if kw not in ("states", "info", "status", "final_csum"):
                assert call(final_layout=final_layout, **{kw: None}) == _native.EINVAL, kw
                assert f"d_{kw} ".encode() in lib.rudp_last_error()
    for kw in NAMES:  # without closing datagrams the final tables are not looked at
        if kw not in ("states", "info", "status", "final_csum", "final_frames", "final_flow"):
            assert call(final_layout=0, **{kw: None}) == _native.EINVAL, kw
            assert f"d_{kw} ".encode() in lib.rudp_last_error()
    for n in (1025, 4096, 1 << 33):
        assert call(n=n) == _native.ENOTSUP
        assert b"1024" in lib.rudp_last_error() and b"RUDP_FLOWS_MAX_BATCH" in lib.rudp_last_error()
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    seq = torch.zeros(4, dtype=torch.uint16)
    u8 = torch.zeros(4, dtype=torch.uint8)
    i32 = torch.zeros(4, dtype=torch.int32)
    st = torch.zeros((3, 8), dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):
        batch.ack_flows(seq, seq, u8, i32, states=st)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.ack_flows(np.zeros(4, np.uint16), seq, u8, i32, states=st)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.acknowledge_flows(np.zeros(4, np.uint8), torch.zeros(2, dtype=torch.int64), i32, "rudp5", states=st)
    with pytest.raises(ValueError, match="layout"):
        batch.acknowledge_flows(u8, torch.zeros(2, dtype=torch.int64), i32, "rudp6", states=st)
    with pytest.raises(ValueError, match="HIP device"):
        batch.acknowledge_flows(u8, torch.zeros(2, dtype=torch.int64), i32[:1], "rudp5", states=st)
    cpu = torch.device("cpu")
    assert batch._ack_flows_args(i32, st, "exact", None, cpu, 4) == (_native.ACK_EXACT, 0)
    assert batch._ack_flows_args(i32, st, "cumulative", "rudp7", cpu, 4) == (_native.ACK_CUMULATIVE, 7)
    for kw in ({"mode": "both"}, {"mode": None}, {"final_layout": "rudp6"}, {"final_layout": 0},
               {"states": torch.zeros((3, 4), dtype=torch.int64)}, {"states": torch.zeros(24, dtype=torch.int64)},
               {"states": st.to(torch.int32)}, {"flow": i32.to(torch.int64)}, {"flow": i32[:3]}):
        a = {"flow": i32, "states": st, "mode": "exact", "final_layout": None, **kw}
        with pytest.raises(ValueError):
            batch._ack_flows_args(a["flow"], a["states"], a["mode"], a["final_layout"], cpu, 4)
    for bad in (0, -1, True, 1.5, 0xFFFFFFFF):
        with pytest.raises(ValueError, match="n_flows"):
            batch.ack_flow_states(bad, "cpu")
    z = batch.ack_flow_states(7, "cpu")
    assert z.shape == (7, 8) and z.dtype == torch.int64 and not z.any()
    # a fresh row, as the header states it
    for isn, T, C in ((0, 0, 1), (65535, 300, 16), (7, 5, 16), (9, 32, 16), (1, 1 << 40, 16383)):
        batch.ack_flow_open(z, 2, isn, T, C)
        assert z[2].tolist() == open_row(isn, T, C) == [0, min(C, T), int(min(C, T) == T), 0, isn, T, C, 0]
    assert not z[:2].any() and not z[3:].any()
    for args in ((7, 0, 1, 1), (-1, 0, 1, 1), (True, 0, 1, 1), (0, 65536, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1),
                 (0, 0, 1, 0), (0, 0, 1, 16384), (0, 0, 1 << 63, 1)):
        with pytest.raises(ValueError):
            batch.ack_flow_open(z, *args)
    with pytest.raises(TypeError):
        batch.ack_flow_open(torch.zeros((7, 4), dtype=torch.int64), 0, 0, 1, 1)
    # the layout of the one result allocation: every array aligned to its element
    for n in (0, 1, 2, 3, 1023, 1024):
        for H in (0, 5, 7):
            lay = batch.AckFlows.layout(n, H)
            assert lay["pointer"] == 0 and lay["flow_info"] == 8 * n and lay["info"] == 72 * n
            assert lay["status"] == lay["info"] + 64 and lay["final_flow"] == lay["status"] + 8
            assert lay["final_csum"] % 2 == 0 and lay["final_frames"] == lay["final_csum"] + 2 * n
            assert lay["host_end"] == lay["final_frames"] + n * H
            assert lay["order"] % 4 == 0 and lay["order"] >= lay["host_end"]
            assert lay["order_off"] == lay["order"] + 4 * n and lay["valid"] == lay["order_off"] + 4 * (n + 1)
            assert lay["size"] == lay["valid"] + n
    assert any(bit == _native.ST_FLOW_ROW for bit, _ in batch._ST_ACK_FLOWS)
    with pytest.raises(ValueError, match="isn > 65535"):
        batch._raise_bits(_native.ST_FLOW_ROW, batch._ST_ACK_FLOWS)
    with pytest.raises(ValueError, match="flow slot"):
        batch._raise_bits(_native.ST_FLOW, batch._ST_ACK_FLOWS)
    batch._raise_bits(0, batch._ST_ACK_FLOWS)


def test_flow_table_lookup_allocates_nothing():
    t = flows.FlowTable(3)
    a, b, c = (0x7F000001 << 16 | port for port in (4000, 4001, 4002))
    assert t.lookup(np.array([a, b, a], np.uint64)).tolist() == [FLOW_NONE] * 3
    assert t.allocations == 0 and len(t) == 0
    s = t.slots(np.array([b, a], np.uint64))
    got = t.lookup(np.array([c, a, b, b, c], np.uint64))
    assert got.dtype == np.uint32 and got.tolist() == [FLOW_NONE, int(s[1]), int(s[0]), int(s[0]), FLOW_NONE]
    assert t.allocations == 2 and len(t) == 2 and t.slot_of(c) is None
    t.release(int(s[0]))
    assert t.lookup(np.array([b, a], np.uint64)).tolist() == [FLOW_NONE, int(s[1])]
    assert t.lookup(np.zeros(0, np.uint64)).shape == (0,)


def _single(seq, ack, flags, usable, isn, T, C, state, mode, sent, slot=3, n_flows=6):
    table = np.zeros((n_flows, 8), np.uint64)
    table[slot] = (*state, isn, T, C, sent if mode == CUMULATIVE else 0)
    table[slot ^ 1] = (11, 7, 1, 0, 9, 100, 7, 50)
    f = ack_flows_ref(seq, ack, flags, usable, np.full(len(ack), slot, np.uint32), table, mode)
    r = ack_ref(seq, ack, flags, usable, isn=isn, T=T, C=C, state=state, mode=mode, sent=sent)
    n = len(ack)
    assert f.valid.tolist() == r.valid.tolist() and f.pointer.tolist() == r.pointer.tolist()
    if n and not state[3]:
        assert f.states[slot].tolist() == list(r.state) + [int(v) for v in table[slot][4:]]
    else:
        assert f.states[slot].tolist() == table[slot].tolist()
    assert f.states[slot ^ 1].tolist() == table[slot ^ 1].tolist()
    assert not f.states[[k for k in range(n_flows) if k not in (slot, slot ^ 1)]].any()
    if n:
        p = r.state[0]
        closing = 0 if r.final is None else r.final[0] | r.final[1] << 16
        assert f.flow_info.tolist() == [[slot, r.end, r.count, r.newly, p, -(-p // C), r.done, closing]]
        assert f.order.tolist() == list(range(n)) and f.order_off.tolist() == [0, n]
        assert f.finals == ([] if r.final is None else [(0, *r.final)])
    assert f.info == [1 if n else 0, r.count, int(r.end < n), r.newly, 0] and f.status == 0
    return r


def test_oracle_single_flow_is_the_ack_rule():
    rng = random.Random(0xAC4F10)
    ended = 0
    for k in range(300):
        n = rng.randint(0, 120)
        C = rng.choice((1, 3, 16))
        T = rng.choice((0, 1, C, 5 * C + 1, 30 * C))
        isn = rng.choice((0, 7, 65535 - T // 2, 65530))
        mode = (EXACT, CUMULATIVE)[k & 1]
        if k % 4 >= 2:
            s = adversarial_replies(rng, n, isn=isn, T=T, C=C)
            state = rng.choice((fresh_state(T, C), (C, 0, 1, 0), (T, 0, 1, 0), (0, min(C, T), int(min(C, T) == T), 1)))
        else:
            s = clean_replies(rng, n, isn=isn, T=T, C=C, W=rng.choice((1, 4)))
            state = fresh_state(T, C)
        ended += _single(*s, isn, T, C, state, mode, T).end < n
    assert 30 < ended < 270


def test_oracle_reproduces_every_reference_stream_among_other_flows():
    """The reference's own reply streams, several of them interleaved in one
    batch with flowless replies in between: what the golden file records for
    each stream alone is what its flow gets."""
    rng = random.Random(0x60DAC)
    cases = golden_cases()
    assert len(cases) > 20
    for at in range(0, len(cases), 5):
        group = cases[at:at + 5]
        streams = [parse_rudp5([bytes.fromhex(h) for h in c["replies"]]) for c in group]
        slots = rng.sample(range(40), len(group))
        table = np.zeros((40, 8), np.uint64)
        for c, slot in zip(group, slots):
            table[slot] = open_row(c["isn"], len(c["message"]), c["chunk"])
        pick = arrival_order(rng, [len(s[0]) for s in streams])
        seq, ack, flags, flow = [], [], [], []
        cur = [0] * len(group)
        for k in pick:
            j = cur[k]
            cur[k] += 1
            seq.append(streams[k][0][j]), ack.append(streams[k][1][j]), flags.append(streams[k][2][j])
            flow.append(slots[k])
            if rng.random() < 0.1:  # a stranger's reply in between
                seq.append(0), ack.append(streams[k][1][j]), flags.append(ACK), flow.append(FLOW_NONE)
        n = len(ack)
        flow = np.array(flow, np.uint32)
        f = ack_flows_ref(np.array(seq, np.uint16), np.array(ack, np.uint16), np.array(flags, np.uint8), None, flow,
                          table)
        assert f.status == 0 and f.info[4] == int((flow == FLOW_NONE).sum())
        rows = {int(r[0]): r for r in f.flow_info.tolist()}
        for c, slot, s in zip(group, slots, streams):
            if not len(s[0]):
                assert slot not in rows
                continue
            row, mine = rows[slot], np.flatnonzero(flow == slot)
            assert (row[4], row[6]) == (c["pointer"], int(c["done"])), c["name"]
            assert (f.states[slot][0], f.states[slot][3]) == (c["pointer"], int(c["done"])), c["name"]
            last_index, last_sent = c["sent"][-1]
            if c["done"]:
                assert row[1] == int(mine[last_index]), c["name"]
                a = [r[0] for r in f.flow_info.tolist()].index(slot)
                fin = next(x for x in f.finals if x[0] == a)
                assert bytes.fromhex(last_sent) == bytes([fin[1] >> 8, fin[1] & 255, fin[2] >> 8, fin[2] & 255, ACK])
                assert row[7] == fin[1] | fin[2] << 16
            else:
                assert row[1] == n and row[7] == 0, c["name"]
            sent_after = {i for i, _ in c["sent"] if i >= 0}
            assert sent_after <= set(np.flatnonzero(f.valid[mine]).tolist()), c["name"]


def test_oracle_rows_status_and_mix_conditions():
    for mode in (EXACT, CUMULATIVE):
        rng = random.Random(0xA11 + (mode == CUMULATIVE))
        seq, ack, flags, usable, flow, table = make_reply_batch(rng, 257, 37, mode, n_flows=5000)
        assert {0, 4999} <= set(flow.tolist())
        good = ack_flows_ref(seq, ack, flags, usable, flow, table, mode)
        assert good.status == 0 and good.kinds["idle"] == 1 and good.kinds["done"] == 1
        assert good.info[0] == len(set(flow[flow != FLOW_NONE].tolist())) - 1
        assert good.order_off[-1] == 257 - good.info[4] and sorted(good.order.tolist()) == list(range(257))
        assert (good.states[:, 4:] == table[:, 4:]).all()
        # an out-of-range slot
        bad = flow.copy()
        victim = int(np.flatnonzero(flow != FLOW_NONE)[5])
        bad[victim] = 5000
        f = ack_flows_ref(seq, ack, flags, usable, bad, table, mode)
        assert f.status == ST_FLOW and not f.valid[victim] and not f.pointer[victim]
        assert f.order.tolist()[f.order_off[-1]:] == np.flatnonzero(~np.isin(bad, f.flow_info[:, 0])).tolist()
        # a refused row, in each of its ways: its flow is not listed and its row stays
        slot = int(good.flow_info[2][0])
        for word, value in ((4, 65536), (6, 16384)) + (((7, int(table[slot][5]) + 1),) if mode == CUMULATIVE else ()):
            t2 = table.copy()
            t2[slot, word] = value
            f = ack_flows_ref(seq, ack, flags, usable, flow, t2, mode)
            assert f.status == ST_FLOW_ROW and f.info[0] == good.info[0] - 1
            assert slot not in f.flow_info[:, 0].tolist() and (f.states[slot] == t2[slot]).all()
            assert not f.valid[flow == slot].any() and not f.pointer[flow == slot].any()
        if mode == EXACT:  # sent is not read
            t2 = table.copy()
            t2[slot, 7] = int(table[slot][5]) + 1
            f = ack_flows_ref(seq, ack, flags, usable, flow, t2, mode)
            assert f.status == 0 and f.flow_info.tolist() == good.flow_info.tolist()
