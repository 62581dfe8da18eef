"""rudp_segment_utf8 on the GPU: the reference's frames (tests/golden/segment.json),
the numpy restatement (tests/segment_ref.py) at vector and tile edges with
guarded outputs, the edge rules of include/rudp.h, and the callers built on it."""
import random
import re

import numpy as np
import pytest

from conftest import PKG
from rudp import _native, batch
from rudp.transport import ReliableUDP, build
from segment_ref import golden_cases, segment_ref

pytestmark = pytest.mark.gpu

TILE = int(re.search(r"kSegTileBytes = (\d+);", (PKG / "csrc" / "segment.hip").read_text()).group(1))
ROUND = int(re.search(r"kSegRoundBytes = (\d+);", (PKG / "csrc" / "segment.hip").read_text()).group(1))
GUARD = 64
ALPHABET = "abcxyz019 \n\t~" + "éßñ" + "€中文字" + "😀🚀" + "\u0000\u007f\u0080\u07ff\u0800\uffff"
_rng = random.Random(0x5E6)
TEXT = "".join(_rng.choice(ALPHABET) for _ in range(3 * TILE + 64)).encode()  # > 3 tiles + 5 bytes, mixed widths


def host(t):
    return t.cpu().numpy()


class Outputs:
    """Sentinel-filled output arrays of `cap` entries with GUARD entries behind each."""
    SENT = {"seq": 0xA5A5, "ack": 0xA5A5, "flags": 0xA5, "len": 0x5A5A5A5A, "off": 0x5A5A5A5A5A5A5A5A}

    def __init__(self, cuda, cap):
        import torch
        self.cap = cap
        dt = {"seq": torch.int16, "ack": torch.int16, "flags": torch.uint8, "len": torch.int32, "off": torch.int64}
        self.np_dt = {"seq": np.uint16, "ack": np.uint16, "flags": np.uint8, "len": np.uint32, "off": np.uint64}
        self.t = {k: torch.empty(cap + (1 if k == "off" else 0) + GUARD, dtype=d, device=cuda) for k, d in dt.items()}
        self.count = torch.empty(2 + GUARD, dtype=torch.int64, device=cuda)
        self.status = torch.empty(1 + GUARD, dtype=torch.int32, device=cuda)

    def fill(self):
        import torch
        for t in self.t.values():  # (every sentinel is one byte repeated)
            t.view(torch.uint8).fill_(0xA5 if t.element_size() < 4 else 0x5A)
        self.count.fill_(-7)
        self.status.fill_(-7)

    def read(self, name):
        return host(self.t[name]).view(self.np_dt[name])

    def guards_intact(self, with_off=True):
        for k in self.t:
            if k == "off" and not with_off:
                assert (self.read(k) == self.SENT[k]).all(), "NULL d_payload_off, yet the array was written"
                continue
            tail = self.read(k)[self.cap + (1 if k == "off" else 0):]
            assert len(tail) == GUARD and (tail == self.SENT[k]).all(), (k, tail[:4])
        assert (host(self.count)[2:] == -7).all() and (host(self.status)[1:] == -7).all()


def segment_raw(cuda, msg_t, nbytes, chunk, isn, out: Outputs, with_off=True, cap=None, null_tables=False):
    """One rudp_segment_utf8 call on msg_t[:nbytes] into `out`; returns (count, characters, status)."""
    out.fill()
    cap = out.cap if cap is None else cap
    p = (lambda k: None) if null_tables else (lambda k: out.t[k].data_ptr())
    rc = _native.lib().rudp_segment_utf8(
        msg_t.data_ptr() if nbytes else None, nbytes, chunk, isn, cap, p("seq"), p("ack"), p("flags"), p("len"),
        p("off") if with_off else None, out.count.data_ptr(), out.status.data_ptr(), cuda.index or 0, None)
    _native.check(rc)
    c = host(out.count)
    return int(c[0]), int(c[1]), int(host(out.status)[0])


def expect_equal(out: Outputs, want, with_off=True):
    n = want.packets
    assert np.array_equal(out.read("seq")[:n], want.seq)
    assert np.array_equal(out.read("ack")[:n], want.ack)
    assert np.array_equal(out.read("flags")[:n], want.flags)
    assert np.array_equal(out.read("len")[:n].astype(np.int64), want.len)
    if with_off:
        assert np.array_equal(out.read("off")[:n + 1].astype(np.int64), want.payload_off)


def upload(cuda, data: bytes, view=0):
    """A device view at byte offset `view` of a 16-B aligned allocation holding `data`."""
    import torch
    t = torch.zeros(view + len(data) + 1, dtype=torch.uint8, device=cuda)
    assert t.data_ptr() % 16 == 0
    if data:
        t[view:view + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    return t[view:view + len(data)]


# ------------------------------------------------------------ the reference's frames
def test_frame_message_equals_reference_frames(cuda):
    for c in golden_cases():
        res = batch.frame_message(c["message"], c["isn"], chunk=c["chunk"], layout="rudp5", device=cuda)
        off = np.concatenate([[0], np.cumsum([len(f) for f in c["frames"]])])
        assert np.array_equal(host(res.frame_off), off), (c["message"], c["chunk"])
        assert host(res.frames).tobytes() == b"".join(c["frames"]), (c["message"], c["chunk"], c["isn"])


def test_segment_message_on_device_tensor_equals_reference_fields(cuda):
    for c in golden_cases():
        msg = upload(cuda, c["message"].encode())
        seg = batch.segment_message(msg, c["isn"], chunk=c["chunk"])
        fr = c["frames"]
        assert seg.count == len(fr) and seg.characters == len(c["message"])
        tab = seg.table()
        assert host(tab.headers.seq).view(np.uint16).tolist() == [int.from_bytes(f[0:2], "big") for f in fr]
        assert host(tab.headers.ack).view(np.uint16).tolist() == [int.from_bytes(f[2:4], "big") for f in fr]
        assert host(tab.headers.flags).tolist() == [f[4] for f in fr]
        assert host(tab.lengths).tolist() == [len(f) - 5 for f in fr]
        assert host(tab.payload_off).tolist() == np.concatenate([[0], np.cumsum([len(f) - 5 for f in fr])]).tolist()


# ------------------------------------------------ the restatement, at vector and tile edges
SIZES = (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
PLACEMENTS = [(lead, 0) for lead in range(4)] + [(0, view) for view in (1, 7, 15)]  # (ASCII bytes prepended, view offset)


@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 64, 1472, 16383])
def test_against_restatement_at_edges(cuda, chunk):
    outs = {}
    for size in SIZES:
        for lead, view in PLACEMENTS:
            data = b"xyz"[:lead] + TEXT[:size]
            msg = upload(cuda, data, view)
            assert not data or msg.data_ptr() % 16 == view
            cap = max(1, -(-len(data) // chunk))
            out = outs[cap] if cap in outs else outs.setdefault(cap, Outputs(cuda, cap))
            for with_off in (True, False):
                want = segment_ref(data, chunk, 3611, cap)
                got = segment_raw(cuda, msg, len(data), chunk, 3611, out, with_off)
                assert got == (want.packets, want.characters, 0), (size, lead, view, with_off)
                expect_equal(out, want, with_off)
                out.guards_intact(with_off)


@pytest.mark.parametrize("rounds", [2, 4, 16])
def test_larger_tiles_of_long_messages(cuda, rounds):
    """Messages of more than 16384 tiles take tiles of 2 to 16 rounds; the diagnostics
    build takes the rounds from a knob, so those forms run here at small sizes."""
    tools = _native.tools_lib(activate=True)
    tile = rounds * ROUND
    big = TEXT * (1 + (3 * tile + 5) // len(TEXT))
    outs = {}
    try:
        assert tools.rudpx_tune(76, rounds) == 0
        for size in (tile - 1, tile, tile + 1, 3 * tile + 5):
            for lead, view in ((0, 0), (3, 0), (0, 7)):
                data = b"xyz"[:lead] + big[:size]
                msg = upload(cuda, data, view)
                for chunk in (1, 7, 1472):
                    cap = max(1, -(-len(data) // chunk))
                    out = outs[cap] if cap in outs else outs.setdefault(cap, Outputs(cuda, cap))
                    want = segment_ref(data, chunk, 65530, cap)
                    got = segment_raw(cuda, msg, len(data), chunk, 65530, out)
                    assert got == (want.packets, want.characters, 0), (size, lead, view, chunk)
                    expect_equal(out, want)
                    out.guards_intact()
    finally:
        tools.rudpx_tune(76, 0)
        _native.use_product()


@pytest.mark.parametrize("rounds", [1, 4])
@pytest.mark.parametrize("apron", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 16])
def test_both_forms_of_len(cuda, chunk, apron, rounds):
    """Chunks up to 16 characters have two forms of len[] (the diagnostics build's knob
    77: whole rows from the tile pass, or starts and differences): the same tables
    from both, also where a packet ends past the 64-byte apron."""
    tools = _native.tools_lib(activate=True)
    cont = bytes([0x80])
    odd = [b"a" + cont * 200 + b"bc", cont * 5 + b"abc" + cont * (ROUND + 70) + "é😀".encode() * 9,
           TEXT[:ROUND - 2] + cont * 3 * ROUND + TEXT[:50], b"ab" + cont * 70000 + b"cd", cont * 300]
    outs = {}
    try:
        assert tools.rudpx_tune(77, apron) in (0, 1) and tools.rudpx_tune(76, rounds) == 0
        cases = [(b"xyz"[:lead] + TEXT[:size], view) for size in SIZES for lead, view in PLACEMENTS]
        for data, view in cases + [(d, 0) for d in odd]:
            msg = upload(cuda, data, view)
            cap = max(1, -(-len(data) // chunk))
            out = outs[cap] if cap in outs else outs.setdefault(cap, Outputs(cuda, cap))
            for with_off in (True, False):
                want = segment_ref(data, chunk, 65530, cap)
                got = segment_raw(cuda, msg, len(data), chunk, 65530, out, with_off)
                assert got == (want.packets, want.characters, want.status), (len(data), view, with_off)
                if want.status == 0:
                    expect_equal(out, want, with_off)
                out.guards_intact(with_off)
    finally:
        tools.rudpx_tune(77, 1)
        tools.rudpx_tune(76, 0)
        _native.use_product()


def test_packet_spanning_many_tiles(cuda):
    data = ("😀" * (2 * 16383 + 10)).encode()  # 3 packets of 65532, 65532 and 40 bytes over 8 tiles
    assert len(data) > 7 * TILE
    msg = upload(cuda, data)
    out = Outputs(cuda, 5)
    want = segment_ref(data, 16383, 65530, 5)
    assert want.packets == 3 and want.len.tolist() == [65532, 65532, 40]
    assert segment_raw(cuda, msg, len(data), 16383, 65530, out) == (3, 2 * 16383 + 10, 0)
    expect_equal(out, want)
    out.guards_intact()


# ------------------------------------------------------------------ edge rules
def test_leading_continuation_bytes_belong_to_packet_0(cuda):
    data = bytes([0x80, 0x80, 0x61, 0x80, 0x62])
    out = Outputs(cuda, 5)
    assert segment_raw(cuda, upload(cuda, data), 5, 1, 9, out) == (2, 2, 0)
    assert out.read("off")[:3].tolist() == [0, 4, 5] and out.read("len")[:2].tolist() == [4, 1]
    assert out.read("flags")[:2].tolist() == [0x80, 0x20] and out.read("seq")[:2].tolist() == [9, 10]
    out.guards_intact()


def test_all_continuation_input_is_one_syn_fin_packet(cuda):
    data = bytes([0x80] * 37)
    out = Outputs(cuda, 4)
    for chunk in (1, 5):
        assert segment_raw(cuda, upload(cuda, data), 37, chunk, 9, out) == (1, 0, 0)
        assert out.read("flags")[0] == 0xA0 and out.read("len")[0] == 37 and out.read("off")[:2].tolist() == [0, 37]
        assert out.read("seq")[0] == 9 and out.read("ack")[0] == 0
    out.guards_intact()


def test_empty_message_is_one_syn_fin_packet(cuda):
    out = Outputs(cuda, 1)
    assert segment_raw(cuda, upload(cuda, b""), 0, 3, 65535, out) == (1, 0, 0)
    assert out.read("flags")[0] == 0xA0 and out.read("len")[0] == 0 and out.read("off")[:2].tolist() == [0, 0]
    assert out.read("seq")[0] == 65535
    out.guards_intact()


def test_packet_over_65535_bytes_sets_st_len(cuda):
    data = bytes([0x80] * 70000)
    out = Outputs(cuda, 8)
    assert segment_raw(cuda, upload(cuda, data), 70000, 1, 9, out) == (1, 0, _native.ST_LEN)
    out.guards_intact()
    with pytest.raises(ValueError, match="65535"):
        batch.segment_message(upload(cuda, data), 9)


def test_too_few_table_entries_sets_packets_cap(cuda):
    data = TEXT[:TILE + 100]
    want = segment_ref(data, 3, 9)
    out = Outputs(cuda, want.packets - 1)
    got = segment_raw(cuda, upload(cuda, data), len(data), 3, 9, out)
    assert got == (want.packets, want.characters, _native.ST_PACKETS_CAP)
    out.guards_intact()
    with pytest.raises(ValueError, match=f"{want.packets} packets are needed"):
        batch.segment_message(upload(cuda, data), 9, chunk=3, max_packets=want.packets - 1)
    seg = batch.segment_message(upload(cuda, data), 9, chunk=3, max_packets=want.packets)
    assert seg.count == want.packets and host(seg.table().lengths).tolist() == want.len.tolist()


def test_size_query_with_null_tables(cuda):
    data = TEXT[:1000]
    want = segment_ref(data, 2, 9)
    out = Outputs(cuda, 0)
    got = segment_raw(cuda, upload(cuda, data), len(data), 2, 9, out, cap=0, null_tables=True)
    assert got == (want.packets, want.characters, _native.ST_PACKETS_CAP)
    out.guards_intact()
    seg = batch.segment_message(upload(cuda, data), 9, chunk=2, max_packets=0, check=False)
    assert (seg.count, seg.characters) == (want.packets, want.characters)
    assert int(seg.status.item()) == _native.ST_PACKETS_CAP


@pytest.mark.parametrize("isn", [65530, 70000])
def test_isn_wraps_mod_2_16(cuda, isn):
    data = TEXT[:400]
    want = segment_ref(data, 2, isn)
    out = Outputs(cuda, want.packets)
    assert segment_raw(cuda, upload(cuda, data), len(data), 2, isn, out)[2] == 0
    expect_equal(out, want)
    assert out.read("seq")[0] == isn & 0xFFFF and (np.diff(out.read("seq")[:want.packets].astype(np.int64)) % 65536 == 2).all()


# ------------------------------------------------------------------ callers
def test_python_refuses_a_non_u8_device_tensor(cuda):
    import torch
    t = torch.zeros(8, dtype=torch.int32, device=cuda)
    for fn in (batch.segment_message, batch.frame_message):
        with pytest.raises(TypeError, match="uint8"):
            fn(t, 1)


@pytest.mark.parametrize("chunk", [1, 4, 1472])
def test_round_trip_through_decode_and_gather(cuda, chunk):
    message = TEXT[:TILE + 333].decode(errors="ignore")
    raw = message.encode()
    res = batch.frame_message(message, 4242, chunk=chunk, layout="rudp5", want_csum=True, device=cuda)
    dec = batch.unpack_batch_varlen(res.frames, res.frame_off, "rudp5", csum=res.csum, utf8=True)
    assert (host(dec.ok) == _native.OK_GOOD).all() and (host(dec.valid) == 1).all()
    got = batch.gather_payloads(res.frames, res.frame_off, "rudp5", keep=batch.keep_mask(dec))
    assert host(got.payload).tobytes() == raw
    seg = batch.segment_message(got.payload, 4242, chunk=chunk)
    assert seg.characters == len(message) and seg.count == max(1, -(-len(message) // chunk))
    again = batch.frame_message(got.payload, 4242, chunk=chunk, layout="rudp5")  # reads the count
    assert host(again.frames).tobytes() == host(res.frames).tobytes()
    given = batch.frame_message(got.payload, 4242, chunk=chunk, layout="rudp5", n=seg.count, check=False)
    assert host(given.frames).tobytes() == host(res.frames).tobytes()


@pytest.mark.parametrize("message", ["", "q", "ab✓𝄞é" + "z" * 50 + "😀"])
def test_transport_table_rows_equal_scalar_frames(cuda, message):
    isn = 65500
    r = ReliableUDP(isn_source=lambda: isn, codec_device="cuda:0")
    data, off = r._gpu_frames(message, isn)
    assert len(off) == len(message) + 2  # rows 0..len(message); the empty message is its one SYN|FIN row
    for ptr in range(len(off) - 1):
        flags = (batch.SYN if ptr == 0 else 0) | (batch.FIN if ptr >= len(message) - 1 else 0)
        assert data[off[ptr]:off[ptr + 1]] == build(isn + ptr, 0, flags, message[ptr:ptr + 1]), ptr
