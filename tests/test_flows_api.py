"""rudp_accept_flows (added within ABI 8) at the boundary: the symbol and the
header's defines, the argument checks that run before any device call, the
Python validation, the host-side FlowTable, and the oracle (tests/flows_ref.py)
against the single-flow rule and the streams the reference judged.  CPU-only."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from accept_ref import accept_ref, adversarial_stream, chars_ref, clean_stream, golden_cases, pack_frames, parse_rudp5
from conftest import REPO
from flows_ref import FLOW_NONE, RANK_NONE, ST_FLOW, flows_ref, interleave, make_batch
from rudp import _native, batch, flows

NAME = "rudp_accept_flows"


def test_symbol_and_header():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    for define in (r"RUDP_HAS_ACCEPT_FLOWS 1", r"RUDP_ABI_VERSION 8", r"RUDP_FLOW_NONE 0xFFFFFFFFu",
                   r"RUDP_FLOWS_MAX_BATCH 1024u", r"RUDP_ST_FLOW 256u"):
        assert re.search(rf"^#define {define}\b", text, flags=re.M), define
    assert hasattr(lib, NAME) and NAME in _native.EXPORTS
    assert re.search(rf"^RUDP_API int {NAME}\(", text, flags=re.M)
    assert (_native.FLOW_NONE, _native.FLOWS_MAX_BATCH, _native.ST_FLOW) == (0xFFFFFFFF, 1024, 256)
    assert (FLOW_NONE, RANK_NONE, ST_FLOW) == (_native.FLOW_NONE, _native.RANK_NONE, _native.ST_FLOW)
    assert batch.FLOWS_MAX_BATCH == 1024 and batch.FLOW_NONE == flows.FLOW_NONE == 0xFFFFFFFF
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == NAME and ln.split()[1] == "T" for ln in out.splitlines()), path
    # the kernel holds exactly one batch
    hpp = (REPO / "reliable-udp_amd" / "csrc" / "flows_device.hpp").read_text()
    assert "constexpr uint32_t kFlowMax = kBlock * kFlowFpt;" in hpp and "constexpr uint32_t kFlowFpt = 4;" in hpp


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    p = ctypes.cast(word, ctypes.c_void_p)
    names = ("seq", "flags", "chars", "flow", "states", "accept", "keep", "reply", "reply_ack", "rank", "order",
             "order_off", "flow_info", "info", "status")

    def call(n=1, n_flows=4, **kw):
        a = {k: kw.get(k, p) for k in names}
        return lib.rudp_accept_flows(a["seq"], a["flags"], a["chars"], None, a["flow"], n, a["states"], n_flows,
                                     a["accept"], a["keep"], a["reply"], a["reply_ack"], a["rank"], a["order"],
                                     a["order_off"], a["flow_info"], a["info"], a["status"], 0, None)

    for kw in ("states", "info", "status"):
        for n in (0, 1):
            assert call(n=n, **{kw: None}) == _native.EINVAL
            assert f"d_{kw}".encode() in lib.rudp_last_error()
    for n_flows in (0, 0xFFFFFFFF, 1 << 40):
        assert call(n_flows=n_flows) == _native.EINVAL and b"n_flows" in lib.rudp_last_error()
    for kw in names:
        if kw not in ("states", "info", "status"):
            assert call(**{kw: None}) == _native.EINVAL
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
    st = torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):
        batch.accept_flows(seq, u8, i32, i32, states=st)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.accept_flows(np.zeros(4, np.uint16), u8, i32, i32, states=st)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive_flows(np.zeros(4, np.uint8), torch.zeros(2, dtype=torch.int64), i32, "rudp5", states=st)
    with pytest.raises(ValueError, match="layout"):
        batch.receive_flows(u8, torch.zeros(2, dtype=torch.int64), i32, "rudp6", states=st)
    with pytest.raises(ValueError, match="1024"):
        batch.receive_flows(u8, torch.zeros(1026, dtype=torch.int64), i32, "rudp5", states=st)
    for bad in (0, -1, True, 1.5, 0xFFFFFFFF):
        with pytest.raises(ValueError, match="n_flows"):
            batch.flow_states(bad, "cpu")
    z = batch.flow_states(7, "cpu")
    assert z.shape == (7, 4) and z.dtype == torch.int64 and not z.any()
    # the per-tensor check accept_flows applies: dtype, device, shape and size are ValueErrors
    cpu = torch.device("cpu")
    batch._flows_tensor(i32, "flow", cpu, (torch.int32,), 4)
    batch._flows_tensor(st, "states", cpu, (torch.int64,), ndim=2)
    for t, dtypes, kw in ((i32, (torch.int64,), {}), (i32, (torch.int32,), {"n": 5}), (st, (torch.int64,), {}),
                          (st.t(), (torch.int64,), {"ndim": 2}), (torch.zeros(12, dtype=torch.int64), (torch.int64,),
                                                                  {"ndim": 2})):
        with pytest.raises(ValueError):
            batch._flows_tensor(t, "x", cpu, dtypes, **kw)
    with pytest.raises(ValueError, match="expected"):
        batch._flows_tensor(i32, "x", torch.device("meta"), (torch.int32,))
    # the layout of the one result allocation: every array aligned to its element
    for n in (0, 1, 2, 3, 1023, 1024):
        lay = batch.FlowsAccepted.layout(n)
        assert lay["rank"] == 0 and lay["order"] == 4 * n and lay["order_off"] == 8 * n
        assert lay["reply_ack"] == 12 * n + 4 and lay["accept"] == 14 * n + 4
        assert lay["flow_info"] % 8 == 0 and lay["flow_info"] >= 17 * n + 4
        assert lay["info"] == lay["flow_info"] + 64 * n and lay["status"] == lay["info"] + 64
        assert lay["size"] >= lay["status"] + 4
    assert any(bit == _native.ST_FLOW for bit, _ in batch._ST_MESSAGES)


def test_flow_table():
    t = flows.FlowTable(3)
    a, b, c, d = (0x7F000001 << 16 | port for port in (4000, 4001, 4002, 4003))
    src = np.array([b, a, b, b, a], np.uint64)
    s = t.slots(src)
    assert s.dtype == np.uint32 and s.shape == (5,)
    assert s[0] == s[2] == s[3] and s[1] == s[4] and s[0] != s[1] and set(s.tolist()) == {0, 1}
    assert t.allocations == 2 and len(t) == 2  # one allocation per distinct peer
    assert t.slots(src).tolist() == s.tolist() and t.allocations == 2  # stable
    assert t.slot_of(a) == int(s[1]) and t.key_of(int(s[1])) == a
    s2 = t.slots(np.array([c, d, a], np.uint64))
    assert s2[0] == 2 and s2[1] == FLOW_NONE and s2[2] == s[1]  # full: an unknown peer has no flow
    assert t.allocations == 3 and t.slot_of(d) is None
    t.release(int(s[1]))  # a's slot
    assert t.slot_of(a) is None and len(t) == 2
    s3 = t.slots(np.array([d, d], np.uint64))
    assert s3.tolist() == [int(s[1])] * 2 and t.allocations == 4  # the released slot is reused
    t.release(17)  # unknown slots are ignored
    assert t.slots(np.zeros(0, np.uint64)).shape == (0,)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="capacity"):
            flows.FlowTable(bad)
    # never a loop over datagrams: 1024 datagrams of 3 peers cost 3 lookups
    class Counting(dict):
        gets = 0

        def get(self, *a):
            Counting.gets += 1
            return dict.get(self, *a)
    t2 = flows.FlowTable(8)
    t2._slot = Counting()
    t2.slots(np.array([a, b, c] * 341 + [a], np.uint64))
    assert Counting.gets == 3 and t2.allocations == 3


def _single(seq, flags, chars, usable, state, last_isn, slot=3, n_flows=6):
    table = np.zeros((n_flows, 4), np.uint64)
    table[slot] = (state[0], state[1], state[2], 0 if last_isn is None else last_isn + 1)
    table[slot ^ 1] = (11, 7, 1, 9)
    f = flows_ref(seq, flags, chars, usable, np.full(len(seq), slot, np.uint32), table)
    r = accept_ref(seq, flags, chars, usable, state, last_isn)
    n = len(seq)
    assert f.accept.tolist() == r.accept.tolist() and f.keep.tolist() == r.keep.tolist()
    assert f.reply.tolist() == r.reply.tolist() and f.reply_ack.tolist() == r.reply_ack.tolist()
    want = (0, 0, 0, r.state[1] + 1) if r.end < n else (*r.state, table[slot][3])
    assert f.states[slot].tolist() == list(want)
    assert f.states[slot ^ 1].tolist() == [11, 7, 1, 9] and not f.states[[k for k in range(n_flows)
                                                                           if k not in (slot, slot ^ 1)]].any()
    if n:
        assert f.flow_info.tolist() == [[slot, r.end, r.count, r.msg_start, r.characters, r.state[1],
                                         int(r.keep.sum()), 0]]
        assert f.rank[r.keep.astype(bool)].tolist() == list(range(int(r.keep.sum())))
        assert (f.rank[~r.keep.astype(bool)] == RANK_NONE).all()
        assert f.order.tolist() == list(range(n)) and f.order_off.tolist() == [0, n]
    assert f.info == [1 if n else 0, int(r.keep.sum()), int(r.reply.sum()), int(r.end < n), 0] and f.status == 0
    return r


def test_oracle_single_flow_is_the_inorder_rule():
    rng = random.Random(0xF10735)
    ended = 0
    for k in range(200):
        n = rng.randint(0, 150)
        if k % 2:
            seq, flags, chars, usable = adversarial_stream(rng, n, p_fin=rng.choice((0.0, 0.02)))
            state = rng.choice(((0, 0, 0), (0, 0, 1), (105, 100, 1), (65536, 65530, 1)))
            last = rng.choice((None, int(seq[0]) if n else 5, 3611))
        else:
            seq, flags, chars, usable = clean_stream(rng, n, fin_at=rng.choice((None, rng.randrange(n))) if n else None,
                                                     max_chars=rng.choice((1, 3, 16)))
            state, last = (0, 0, 0), rng.choice((None, 6000))
        ended += _single(seq, flags, chars, usable, state, last).end < n
    assert 20 < ended < 180


def test_oracle_reproduces_every_reference_stream_among_other_flows():
    """The reference's own streams, each played as one flow of a batch that also
    carries unrelated flows and flowless datagrams: what the reference did with
    the stream alone is what its flow gets."""
    rng = random.Random(0x60D)
    cases = golden_cases()
    assert len(cases) == 142
    for c in cases:
        frames = [bytes.fromhex(h) for h in c["frames"]]
        seq, flags, payloads = parse_rudp5(frames)
        buf, off = pack_frames(frames)
        chars = chars_ref(buf, off, 5)
        own = (seq, flags, chars, np.ones(len(seq), np.uint8))
        others = [adversarial_stream(rng, rng.randint(1, 30)), clean_stream(rng, rng.randint(1, 30), fin_at=0)]
        sq, fl, ch, us, flow = interleave(rng, [own] + others, [4, 0, 9], p_none=0.0)
        lost = np.array([rng.random() < 0.1 and f != 4 for f in flow.tolist()])
        flow[lost] = FLOW_NONE
        table = np.zeros((10, 4), np.uint64)
        table[4] = (*c["state"], 0 if c["last_isn"] is None or c["last_isn"] > 65535 else c["last_isn"] + 1)
        f = flows_ref(sq, fl, ch, us, flow, table)
        mine = np.flatnonzero(flow == 4)
        assert "".join(map(str, f.accept[mine])) == c["accepted"], c["name"]
        assert "".join(map(str, f.reply[mine])) == c["replied"], c["name"]
        assert f.reply_ack[mine].tolist() == c["ack"], c["name"]
        row = f.flow_info[[r[0] for r in f.flow_info.tolist()].index(4)].tolist()
        end = c["end"]
        assert row[1] == (int(mine[end]) if end < len(mine) else len(sq)), c["name"]
        kept = mine[f.keep[mine].astype(bool)]
        assert b"".join(frames[int(np.searchsorted(mine, i))][5:] for i in kept).decode() == c["message"], c["name"]
        assert f.rank[kept].tolist() == list(range(row[7], row[7] + row[6])), c["name"]
        after = c["state_after"]
        want = [0, 0, 0, after[1] + 1] if end < len(mine) else after + [int(table[4][3])]
        assert f.states[4].tolist() == want, c["name"]
        assert f.info[4] == int(lost.sum()) and f.status == 0


def test_oracle_out_of_range_slot_and_mix_conditions():
    rng = random.Random(0xA11)
    seq, flags, chars, usable, flow = make_batch(rng, 257, 37, n_flows=5000)
    assert {0, 4999} <= set(flow.tolist())
    table = np.zeros((5000, 4), np.uint64)
    good = flows_ref(seq, flags, chars, usable, flow, table)
    assert good.status == 0 and good.info[0] == len(set(flow[flow != FLOW_NONE].tolist()))
    assert good.order_off[-1] == 257 - good.info[4] and sorted(good.order.tolist()) == list(range(257))
    bad = flow.copy()
    victim = int(np.flatnonzero(flow != FLOW_NONE)[5])
    bad[victim] = 5000
    f = flows_ref(seq, flags, chars, usable, bad, table)
    assert f.status == ST_FLOW and f.info[4] == good.info[4] + 1
    assert not f.accept[victim] and not f.reply[victim] and f.rank[victim] == RANK_NONE
    assert f.order.tolist()[f.order_off[-1]:] == np.flatnonzero((bad == FLOW_NONE) | (bad == 5000)).tolist()
