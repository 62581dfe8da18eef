"""rudp_receive_flows / batch.receive_flows_fused on the device: every output
bit for bit against the oracle from frames (tests/receive_flows_ref.py), every
output between sentinels with nothing written past what the contract names,
both layouts, and every input the fused kernel takes run in both forms (knob 83
of the diagnostics build turns the fused kernel off)."""
import ctypes
import random

import numpy as np
import pytest

from accept_ref import ACK, FIN, SYN
from flows_ref import FLOW_NONE, ST_FLOW, arrival_order
from oracle import codec_np
from receive_flows_ref import (FUSED_BYTES, FUSED_MEAN, N_FLOWS, ST_OFFSETS, ST_PAYLOAD_CAP, build_frames,
                               fused_eligible, mix_case, receive_flows_ref)
from rudp import _native, batch
from test_gpu_flows import mix_conditions

pytestmark = pytest.mark.gpu

SENT = 0xA5
PADB = 64  # sentinel bytes on either side of every output
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
# name -> (bytes per entry, entries the caller provides for n datagrams)
OUTS = {"seq": (2, 0), "ack": (2, 0), "flags": (1, 0), "ok": (1, 0), "csum_out": (2, 0), "valid": (1, 0),
        "usable": (1, 0), "chars": (4, 0), "accept": (1, 0), "keep": (1, 0), "reply": (1, 0), "reply_ack": (2, 0),
        "rank": (4, 0), "order": (4, 0), "order_off": (4, 1), "flow_info": (64, 0), "payload_off": (8, 1),
        "payload_src": (4, 0), "reply_csum": (2, 0), "reply_index": (4, 0), "fin_csum": (2, 0), "fin_flow": (4, 0)}


# ----------------------------------------------------------------- helpers
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)  # (a copy: frombuffer arrays are read-only)


def _table(cuda, table):
    return _dev(cuda, np.asarray(table, np.uint64).view(np.int64))


def _forms(fn):
    """fn('default') with the product library (the fused kernel where the
    batch is eligible), then fn('chained') with knob 83 = 0 in the diagnostics
    build."""
    fn("default")
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(83, 0) == 1
        fn("chained")
    finally:
        tools.rudpx_tune(83, 1)
        _native.use_product()


def _past_the_mean(fn):
    """fn with the fused kernel taken whatever the mean frame length (knob 83 = 2)."""
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(83, 2) == 1
        fn("fused past the mean")
    finally:
        tools.rudpx_tune(83, 1)
        _native.use_product()


def rf_call(cuda, frames, off, side, flow, d_table, H, *, cap=None, fshift=0, pshift=0):
    """rudp_receive_flows with every output between sentinels; ``frames`` lies
    ``fshift`` bytes and ``payload`` ``pshift`` bytes past a 16-B boundary;
    d_table is updated in place.  Returns name -> the whole tensor's bytes."""
    import torch
    n = len(off) - 1
    nbytes = len(frames)
    cap = nbytes if cap is None else cap
    d_frames = torch.zeros(nbytes + 32, dtype=torch.uint8, device=cuda)
    assert d_frames.data_ptr() % 16 == 0
    d_frames[fshift:fshift + nbytes] = _dev(cuda, frames)
    d_off = _dev(cuda, np.asarray(off, np.int64))
    d_side = _dev(cuda, side) if side is not None else None
    d_flow = _dev(cuda, np.asarray(flow, np.uint32).view(np.int32))
    sizes = {k: w * (n + extra) for k, (w, extra) in OUTS.items()}
    sizes.update(reply_frames=n * H, fin_frames=n * H, payload=cap, info=96, status=4)
    bufs = {k: torch.full((2 * PADB + 16 + sz,), SENT, dtype=torch.uint8, device=cuda) for k, sz in sizes.items()}
    for t in bufs.values():
        assert t.data_ptr() % 16 == 0
    shift = {k: 0 for k in sizes}
    shift["payload"] = pshift
    out = _native.RudpReceivedFlows(payload_cap=cap)
    for k in sizes:
        setattr(out, k, bufs[k].data_ptr() + PADB + shift[k])
    rc = _native.lib().rudp_receive_flows(
        d_frames.data_ptr() + fshift, nbytes, d_off.data_ptr(), nbytes // n if n else 0, n,
        d_side.data_ptr() if d_side is not None else None, d_flow.data_ptr(), d_table.data_ptr(),
        d_table.shape[0], ctypes.byref(out), H, 0, None)
    _native.check(rc)
    torch.cuda.synchronize(cuda)
    got = {k: (t.cpu().numpy(), shift[k]) for k, t in bufs.items()}
    got["states"] = d_table.cpu().numpy().view(np.uint64)
    return got


def expected(r, n, H, cap):
    """name -> the bytes the contract says are written, from the oracle."""
    f = r.flows
    A, K = f.info[0], f.info[1]
    total = r.info[8]
    e = {"seq": r.seq, "ack": r.ack, "flags": r.flags, "ok": r.ok, "csum_out": r.csum, "valid": r.valid,
         "usable": r.usable, "chars": r.chars, "accept": f.accept, "keep": f.keep, "reply": f.reply,
         "reply_ack": f.reply_ack, "rank": f.rank}
    if n:
        e.update(order=f.order, order_off=f.order_off, flow_info=f.flow_info, payload_off=r.payload_off,
                 payload_src=r.payload_src, reply_csum=r.reply_csum.astype(np.uint16), reply_index=r.reply_index,
                 fin_csum=r.fin_csum.astype(np.uint16), fin_flow=r.fin_flow)
        assert len(f.order_off) == A + 1 and len(r.payload_off) == K + 1
    out = {k: np.ascontiguousarray(v).tobytes() for k, v in e.items()}
    if n:
        out.update(reply_frames=r.reply_frames, fin_frames=r.fin_frames, payload=r.payload if total <= cap else b"")
    return out


def check(got, r, n, H, cap, what=""):
    want = expected(r, n, H, cap)
    info = np.frombuffer(got["info"][0][PADB:PADB + 96].tobytes(), np.uint64).tolist()
    walked = info[5]
    assert walked <= sum(r.flows.anomalous), what  # (a diagnostic: only a flow with an anomaly is ever walked)
    want["info"] = np.array([walked if v is None else v for v in r.info], np.uint64).tobytes()
    want["status"] = np.array([r.status], np.uint32).tobytes()
    for k in got:
        if k == "states":
            continue
        a, sh = got[k]
        w = want.get(k, b"")
        lo = PADB + sh
        assert a[lo:lo + len(w)].tobytes() == w, (what, k)
        assert (a[:lo] == SENT).all() and (a[lo + len(w):] == SENT).all(), (what, k, "written outside the contract")
    assert np.array_equal(got["states"], r.flows.states), what


def run_both(cuda, frames, off, side, flow, table, H, *, fused=True, what="", r=None, **kw):
    """The oracle once (or the caller's), the device in both forms, each on a fresh table."""
    n = len(off) - 1
    cap = kw.get("cap")
    cap = len(frames) if cap is None else cap
    if r is None:
        r = receive_flows_ref(frames, off, flow, table, H, side, cap)
    assert fused_eligible(len(frames), n) == fused, (what, len(frames), n)  # before the device runs
    _forms(lambda form: check(rf_call(cuda, frames, off, side, flow, _table(cuda, table), H, **kw), r, n, H, cap,
                              (what, form)))
    return r


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("layout", (5, 7))
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_flow_count_against_the_oracle(cuda, n, layout):
    rng = random.Random(0x2F10 + 16 * n + layout)
    for n_active in (1, rng.choice((2, 3)), 37, 300, n):
        n_active = min(n_active, n)
        frames, off, side, flow, table = mix_case(rng, n, n_active, layout)
        assert len(frames) <= FUSED_BYTES and len(frames) <= FUSED_MEAN * n  # the fused form's, before the device runs
        r = receive_flows_ref(frames, off, flow, table, layout, side)
        if n == 1024 and n_active == 37:  # asserted before the device runs
            c = mix_conditions(r.flows, n, flow)
            assert c["ended_with_tail"] >= 1 and c["anomalous"] >= 1 and c["exact"] >= 1, c
            assert c["flowless"] >= 1 and c["restarted"] >= 1 and c["ended"] >= 3, c
            assert {0, N_FLOWS - 1} <= set(flow.tolist())
        run_both(cuda, frames, off, side, flow, table, layout, what=(n, n_active), r=r)


@pytest.mark.parametrize("layout", (5, 7))
def test_pointer_alignment(cuda, layout):
    """d_frames and payload at odd distances from a 16-B boundary: the image's
    first vector and the copy-out's head and tail chunks."""
    rng = random.Random(0xA119 + layout)
    frames, off, side, flow, table = mix_case(rng, 257, 37, layout)
    for fshift, pshift in ((1, 1), (7, 9), (15, 15), (0, 15), (15, 0)):
        run_both(cuda, frames, off, side, flow, table, layout, fshift=fshift, pshift=pshift, what=(fshift, pshift))


# ------------------------------------------------------------ fused limits
def padded_case(rng, n_mix, total_bytes, H):
    """A mix of n_mix datagrams and one more, on a slot of its own, whose ASCII
    payload pads the buffer to exactly total_bytes; it is accepted and kept."""
    frames, off, side, flow, table = mix_case(rng, n_mix, 9, H, n_flows=64)
    free = min(set(range(64)) - set(flow.tolist()))
    pad = total_bytes - len(frames) - H
    assert pad > 0
    body = bytes(rng.choice(b"abcdefghij") for _ in range(pad))
    fr, _, cs = codec_np.encode_varlen(np.array([100], np.uint16), np.zeros(1, np.uint16), np.array([SYN], np.uint8),
                                       [body], H)
    at = rng.randrange(n_mix)  # the long frame sits inside the batch
    cut = int(off[at])
    frames = np.concatenate([frames[:cut], fr, frames[cut:]])
    off = np.concatenate([off[:at + 1], off[at:] + len(fr)])
    flow = np.concatenate([flow[:at], [free], flow[at:]]).astype(np.uint32)
    if side is not None:
        side = np.concatenate([side[:at], cs, side[at:]]).astype(np.uint16)
    table[free] = 0
    assert len(frames) == total_bytes and len(off) == n_mix + 2
    return frames, off, side, flow, table


@pytest.mark.parametrize("layout", (5, 7))
def test_fused_byte_limit(cuda, layout):
    rng = random.Random(0xB17E + layout)
    for total in (FUSED_BYTES - 1, FUSED_BYTES, FUSED_BYTES + 1):
        frames, off, side, flow, table = padded_case(rng, 255, total, layout)
        r = run_both(cuda, frames, off, side, flow, table, layout, fused=total <= FUSED_BYTES, what=total)
        assert r.status == 0 and r.info[8] > total - 255 * 80  # the long payload is part of the message


@pytest.mark.parametrize("layout", (5, 7))
def test_fused_mean_limit_and_knob_2_past_it(cuda, layout):
    rng = random.Random(0x3EA2 + layout)
    n_mix = 63  # 64 datagrams with the long one
    for total in (FUSED_MEAN * 64, FUSED_MEAN * 64 + 1):
        frames, off, side, flow, table = padded_case(rng, n_mix, total, layout)
        fused = total <= FUSED_MEAN * 64
        r = run_both(cuda, frames, off, side, flow, table, layout, fused=fused, what=total)
        if not fused:
            _past_the_mean(lambda form: check(rf_call(cuda, frames, off, side, flow, _table(cuda, table), layout), r,
                                              64, layout, total, (total, form)))


# --------------------------------------------------------------- bad input
@pytest.mark.parametrize("layout", (5, 7))
def test_bad_offsets_and_bad_slots_in_one_batch(cuda, layout):
    rng = random.Random(0xBAD0 + layout)
    frames, off, side, flow, table = mix_case(rng, 257, 37, layout)
    off = off.copy()
    off[40] = off[41] + 3            # decreasing: frame 40 rejected (frame 39 runs on into its neighbours)
    off[120] = len(frames) + 100     # past the buffer: frames 119 and 120 rejected
    off[257] = len(frames) + 5       # the last frame ends past the buffer
    flow = flow.copy()
    valid = np.flatnonzero(flow != FLOW_NONE)
    flow[valid[11]] = N_FLOWS        # one past the table
    flow[valid[200]] = 0xFFFFFFFE
    assert (flow == FLOW_NONE).any()
    r = run_both(cuda, frames, off, side, flow, table, layout, what="bad input")
    assert r.status == ST_OFFSETS | ST_FLOW
    assert set(np.flatnonzero(r.ok == 4).tolist()) >= {40, 119, 120, 256}
    assert r.flows.info[1] > 10  # the flows go on


@pytest.mark.parametrize("layout", (5, 7))
def test_payload_cap(cuda, layout):
    rng = random.Random(0xCA9 + layout)
    frames, off, side, flow, table = mix_case(rng, 300, 20, layout)
    total = receive_flows_ref(frames, off, flow, table, layout, side).info[8]
    assert total > 16
    for cap, pshift in ((total, 0), (total, 9), (total - 1, 0), (0, 0)):
        r = run_both(cuda, frames, off, side, flow, table, layout, cap=cap, pshift=pshift, what=cap)
        assert r.status == (0 if cap >= total else ST_PAYLOAD_CAP) and int(r.payload_off[-1]) == total


def test_empty_batch_touches_nothing(cuda):
    table = np.arange(40, dtype=np.uint64).reshape(10, 4)
    for layout in (5, 7):
        r = run_both(cuda, np.zeros(0, np.uint8), np.zeros(1, np.int64), None, np.zeros(0, np.uint32), table, layout,
                     what="empty")
        assert r.info == [0, 0, 0, 0, 0, None, 0, 0, 0, 0, 0, 0] and r.status == 0


# ------------------------------------------------------------ rows carried
def _send(rng, text, isn, fin=True):
    rows, k = [], 0
    while k < len(text):
        c = min(rng.randint(1, 3), len(text) - k)
        fl = (SYN if k == 0 else 0) | (FIN if fin and k + c == len(text) else 0)
        rows.append(((isn + k) & 0xFFFF, fl, text[k:k + c].encode()))
        if rng.random() < 0.3:
            rows.append(((isn + k) & 0xFFFF, fl & ~FIN & 0xFF, text[k:k + c].encode()))
        k += c
    return rows


def _arrivals(rng, per, slots, H):
    """Streams of (seq, flags, payload) rows merged into one arrival order."""
    pick = arrival_order(rng, [len(p) for p in per])
    at, rows = [0] * len(per), []
    for k in pick:
        rows.append((*per[k][at[k]], slots[k]))
        at[k] += 1
    seq = np.array([r[0] for r in rows], np.uint16)
    flags = np.array([r[1] for r in rows], np.uint8)
    frames, off, cs = codec_np.encode_varlen(seq, np.zeros(len(rows), np.uint16), flags, [r[2] for r in rows], H)
    return frames, off, (cs if H == 5 else None), np.array([r[3] for r in rows], np.uint32), rows


@pytest.mark.parametrize("layout", (5, 7))
def test_rows_carried_over_three_batches(cuda, layout):
    """Long transfers cut in three, short ones that end in the first batch and
    are reopened in the second behind the closed ISN's SYN: the pieces join to
    the texts, and E, fin_flow and fin_frames are the turn-overs'."""
    from rudp.transport import build
    rng = random.Random(0xCA221ED + layout)
    H = layout
    slots = rng.sample(range(64), 6)
    long_text = {0: "héllo wörld, ça va? " * 4, 3: "日本語のテキストです" * 6}
    short_text = {1: "plain ascii", 2: "😀 emoji 😀", 4: "ñandú", 5: "x"}
    sent = {k: _send(rng, t, rng.randint(1, 5000)) for k, t in long_text.items()}
    first = {k: _send(rng, t, rng.randint(1, 5000)) for k, t in short_text.items()}
    second = {k: _send(rng, t[::-1], rng.randint(6000, 9000)) for k, t in short_text.items()}
    table = np.zeros((64, 4), np.uint64)
    tables = {form: None for form in ("default", "chained")}
    got = {k: b"" for k in range(6)}
    done = {k: [] for k in range(6)}
    for b in range(3):
        per = []
        for k in range(6):
            if k in sent:
                s = sent[k]
                per.append(s[b * len(s) // 3:(b + 1) * len(s) // 3])
            elif b == 0:
                per.append(first[k])
            elif b == 1:  # the closed ISN's SYN again (ignored), then a new transfer
                per.append([first[k][0]] + second[k])
            else:
                per.append([])
        frames, off, side, flow, rows = _arrivals(rng, per, slots, H)
        n = len(rows)
        r = receive_flows_ref(frames, off, flow, table, H, side)
        assert fused_eligible(len(frames), n)

        def go(form):
            import torch
            if tables[form] is None:
                tables[form] = torch.zeros((64, 4), dtype=torch.int64, device=cuda)
            check(rf_call(cuda, frames, off, side, flow, tables[form], H), r, n, H, len(frames), (b, form))
        _forms(go)
        table = r.flows.states
        info = r.flows.flow_info.tolist()
        for a, row in enumerate(info):
            k = slots.index(row[0])
            if row[3] < n:
                got[k] = b""
            got[k] += r.payload[int(r.payload_off[row[7]]):int(r.payload_off[row[7] + row[6]])]
        E = r.flows.info[3]
        assert len(r.fin_flow) == E == sum(1 for row in info if row[1] < n) and len(r.fin_frames) == E * H
        for e, a in enumerate(r.fin_flow.tolist()):
            k = slots.index(info[a][0])
            done[k].append(got[k].decode())
            assert r.fin_frames[e * H:e * H + 5] == build(0, info[a][5] + info[a][4], FIN | ACK)
        if b == 0:
            assert E == 4
        if b == 1:  # the repeated SYN of the closed ISN is neither accepted nor answered
            for k in short_text:
                i = next(i for i, row in enumerate(rows) if row[3] == slots[k])
                assert rows[i][0] == first[k][0][0] and not r.flows.accept[i] and not r.flows.reply[i]
            assert E == 4
    for k, t in long_text.items():
        assert done[k] == [t], k
    for k, t in short_text.items():
        assert done[k] == [t, t[::-1]], k


# ------------------------------------------------- against the existing calls
@pytest.mark.parametrize("layout", ("rudp5", "rudp7"))
def test_one_flow_is_rudp_receive(cuda, layout):
    import torch
    from accept_ref import clean_stream
    H = 5 if layout == "rudp5" else 7
    rng = random.Random(0x1F + H)
    for n, fin_at in ((64, None), (257, 200), (1024, None)):
        seq, flags, chars, usable = clean_stream(rng, n, fin_at=fin_at, max_chars=3)
        frames, off, side, _ = build_frames(rng, seq, flags, chars, usable, H)
        d = [_dev(cuda, frames), _dev(cuda, off)]
        csum = _dev(cuda, side) if side is not None else None
        one = batch.receive(*d, layout, csum=csum)

        def go(form):
            states = batch.flow_states(9, cuda)
            many = batch.receive_flows_fused(*d, torch.full((n,), 5, dtype=torch.int32, device=cuda), layout,
                                             states=states, csum=csum).check()
            for name in ("seq", "ack", "csum", "flags", "ok", "valid", "usable", "chars"):
                a, b = getattr(one, name), getattr(many, name)
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (form, name)
            for name in ("accept", "keep", "reply", "reply_ack"):
                a, b = getattr(one.accepted, name), getattr(many, name)
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (form, name)
            R = one.reply_count
            assert many.replies == R and many.message_bytes == one.message_bytes
            assert torch.equal(one.reply_frames[:R * H], many.reply_frames)
            assert torch.equal(one.reply_index[:R], many.reply_index)
            assert torch.equal(one.reply_csum[:R].view(torch.int16), many.reply_csum.view(torch.int16))
            assert many.message(0) == one.message.payload[:one.message_bytes].cpu().numpy().tobytes()
            row, st = states[5].tolist(), one.state.tolist()
            if one.accepted.end < n:  # identical up to the turn-over
                assert row == [0, 0, 0, st[1] + 1] and many.ended == 1 and many.fin_flow.tolist() == [0]
            else:
                assert row == st[:3] + [0] and many.ended == 0 and many.fin_frames.numel() == 0
        _forms(go)


@pytest.mark.parametrize("layout", ("rudp5", "rudp7"))
def test_equals_receive_flows_on_a_text_case(cuda, layout):
    import torch
    H = 5 if layout == "rudp5" else 7
    rng = random.Random(0x2EC + H)
    texts = ("héllo wörld, ça va?", "日本語のテキストです", "plain ascii text here",
             "😀 emoji 😀 mix ñ", "x")
    slots = [3, 0, 11, 7, 4]
    per = []
    while sum(map(len, per)) != 65:
        per = [_send(rng, texts[k] * rng.randint(1, 2), rng.randint(1, 5000), fin=k % 2 == 0) for k in range(5)]
    frames, off, side, flow, rows = _arrivals(rng, per, slots, H)
    frames = frames.copy()
    frames[int(off[7]) + H] ^= 0x01  # a payload byte damaged in flight
    flow[20] = FLOW_NONE
    d = [_dev(cuda, frames), _dev(cuda, off), _dev(cuda, flow.view(np.int32))]
    csum = _dev(cuda, side) if side is not None else None
    s_old = batch.flow_states(12, cuda)
    old = batch.receive_flows(*d, layout, states=s_old, csum=csum)

    def go(form):
        s_new = batch.flow_states(12, cuda)
        new = batch.receive_flows_fused(*d, layout, states=s_new, csum=csum).check()
        assert torch.equal(s_old, s_new), form
        for name in ("seq", "ack", "flags", "ok", "valid"):
            assert torch.equal(getattr(old.decoded, name).view(torch.uint8), getattr(new, name).view(torch.uint8)), name
        assert torch.equal(old.usable.view(torch.uint8), new.usable) and torch.equal(old.chars, new.chars)
        for name in ("accept", "keep", "reply", "reply_ack", "rank", "order"):
            a, b = getattr(old.accepted, name), getattr(new, name)
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
        assert np.array_equal(old.accepted.flows(), new.flows())
        A, K = new.active, new.kept
        assert (A, K, new.replies, new.ended, new.flowless) == (old.accepted.active, old.accepted.kept,
                                                              old.accepted.replies, old.accepted.ended, 1)
        assert torch.equal(old.accepted.order_off[:A + 1], new.order_off[:A + 1])
        assert torch.equal(old.pieces.out_off[:K + 1], new.payload_off[:K + 1])
        assert torch.equal(old.pieces.src[:K], new.payload_src[:K])
        assert torch.equal(old.pieces.payload, new.payload[:new.message_bytes])
        for a in range(A):
            assert old.message(a) == new.message(a)
        assert torch.equal(old.reply_index.int(), new.reply_index)
        assert torch.equal(old.reply_frames(layout), new.reply_frames)
    _forms(go)


# ------------------------------------------------------------------ capture
def test_both_forms_under_stream_capture(cuda):
    import torch
    rng = random.Random(0xCA97)
    n, H = 257, 7
    frames, off, side, flow, _ = mix_case(rng, n, 37, H)
    table = np.zeros((N_FLOWS, 4), np.uint64)
    r = receive_flows_ref(frames, off, flow, table, H, side)
    want = expected(r, n, H, len(frames))
    d = [_dev(cuda, frames), _dev(cuda, off), _dev(cuda, flow.view(np.int32))]

    def go(form):
        states = batch.flow_states(N_FLOWS, cuda)
        side_stream = torch.cuda.Stream(cuda)
        side_stream.wait_stream(torch.cuda.current_stream(cuda))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side_stream):
            with torch.cuda.graph(graph, stream=side_stream):
                res = batch.receive_flows_fused(*d, "rudp7", states=states)
        torch.cuda.current_stream(cuda).wait_stream(side_stream)
        for _ in range(2):  # replayed on a fresh table both times: the same outputs
            states.zero_()
            res._buf.fill_(0xEE)
            graph.replay()
            torch.cuda.synchronize(cuda)
            res._host = None
            for name in ("seq", "usable", "chars", "accept", "keep", "reply_ack", "rank", "order"):
                assert res.host(name).tobytes() == want[name], (form, name)
            assert res.flows().view(np.uint64).tobytes() == want["flow_info"], form
            K, R, E = r.flows.info[1], r.flows.info[2], r.flows.info[3]
            assert (res.kept, res.replies, res.ended, res.message_bytes) == (K, R, E, r.info[8]), form
            assert res.host("payload_off")[:K + 1].tobytes() == want["payload_off"], form
            assert res.host("payload")[:r.info[8]].tobytes() == r.payload, form
            assert res.host("reply_frames")[:R * H].tobytes() == r.reply_frames, form
            assert res.host("fin_frames")[:E * H].tobytes() == r.fin_frames, form
            assert res.host("fin_flow")[:E].tolist() == r.fin_flow.tolist(), form
            assert int(res.host("status")[0]) == 0, form
            assert np.array_equal(states.cpu().numpy().view(np.uint64), r.flows.states), form
    _forms(go)
