"""rudp_receive_flows (added within ABI 8) at the boundary: the symbol and its
struct, the argument checks that run before any device call,
batch.receive_flows_fused's Python validation, the Python constants against
receive_flows.hip, and the CPU reference (tests/receive_flows_ref.py) held to
facts it does not compute itself.  CPU-only."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from accept_ref import ACK, FIN, SYN, accept_ref, clean_stream
from conftest import REPO
from flows_ref import FLOW_NONE, interleave, make_batch
from receive_flows_ref import FUSED_BYTES, FUSED_MEAN, build_frames, decode_ref, receive_flows_ref
from rudp import _native, batch
from rudp.transport import build

FIELDS = ("seq", "ack", "flags", "ok", "csum_out", "valid", "usable", "chars", "accept", "keep", "reply", "reply_ack",
          "rank", "order", "order_off", "flow_info", "payload", "payload_cap", "payload_off", "payload_src",
          "reply_frames", "reply_csum", "reply_index", "fin_frames", "fin_csum", "fin_flow", "info", "status")
OR_NULL = ("csum_out", "payload_src", "reply_csum", "fin_csum")


def test_symbol_header_and_struct():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^#define RUDP_HAS_RECEIVE_FLOWS 1\b", text, flags=re.M) and _native.HAS_RECEIVE_FLOWS
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    assert hasattr(lib, "rudp_receive_flows") and "rudp_receive_flows" in _native.EXPORTS
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == "rudp_receive_flows" and ln.split()[1] == "T" for ln in out.splitlines()), path
    body = re.search(r"typedef struct rudp_received_flows \{(.*?)\} rudp_received_flows;", text, flags=re.S).group(1)
    members = re.findall(r"(\w+);", body)
    assert [m for m in members if m.endswith("_or_null")] == [f + "_or_null" for f in OR_NULL]
    assert [m.replace("_or_null", "") for m in members] == list(FIELDS) == [
        f[0] for f in _native.RudpReceivedFlows._fields_]
    assert ctypes.sizeof(_native.RudpReceivedFlows) == 8 * len(FIELDS)
    for name in FIELDS:
        assert getattr(_native.RudpReceivedFlows, name).offset == 8 * FIELDS.index(name), name
    proto = re.search(r"RUDP_API int rudp_receive_flows\((.*?)\);", text, flags=re.S).group(1)
    names = [re.findall(r"\w+", a)[-1] for a in proto.split(",")]
    assert names == ["d_frames", "frames_bytes", "d_frame_off", "len_hint", "n", "d_csum_in_or_null", "d_flow",
                     "d_states", "n_flows", "out", "layout", "device", "hip_stream"]
    assert len(lib.rudp_receive_flows.argtypes) == len(names)


def _call(lib, word, *, frames="p", nbytes=8, off="p", n=1, csum=None, flow="p", states="p", n_flows=4, layout=5,
          out="o", cap=8, **null):
    p = ctypes.cast(word, ctypes.c_void_p)
    o = _native.RudpReceivedFlows(**{f: (cap if f == "payload_cap" else p.value) for f in FIELDS})
    for name in null:
        setattr(o, name, None)
    pick = lambda v: p if v == "p" else v  # noqa: E731
    return lib.rudp_receive_flows(pick(frames), nbytes, pick(off), 0, n, pick(csum), pick(flow), pick(states), n_flows,
                                  ctypes.byref(o) if out == "o" else None, layout, 0, None)


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    err = lib.rudp_last_error
    assert _call(lib, word, out=None) == _native.EINVAL and b"out is NULL" in err()
    for layout in (0, 6, 8):
        assert _call(lib, word, layout=layout) == _native.EINVAL and b"layout" in err()
    assert _call(lib, word, layout=7, csum="p") == _native.EINVAL and b"layout 7" in err()
    for n in (0, 1):  # required whatever the batch size
        assert _call(lib, word, n=n, states=None) == _native.EINVAL and b"d_states is NULL" in err()
        for field in ("info", "status"):
            assert _call(lib, word, n=n, **{field: None}) == _native.EINVAL
            assert b"rudp_receive_flows: " + field.encode() + b" is NULL" in err(), field
        for bad in (0, 0xFFFFFFFF, 1 << 40):
            assert _call(lib, word, n=n, n_flows=bad) == _native.EINVAL and b"n_flows" in err()
    for n in (1025, 1 << 33):
        assert _call(lib, word, n=n) == _native.ENOTSUP and b"RUDP_FLOWS_MAX_BATCH" in err()
    assert _call(lib, word, off=None) == _native.EINVAL and b"d_frame_off is NULL" in err()
    assert _call(lib, word, flow=None) == _native.EINVAL and b"d_flow is NULL" in err()
    assert _call(lib, word, frames=None) == _native.EINVAL and b"d_frames is NULL" in err()
    assert _call(lib, word, payload=None) == _native.EINVAL and b"payload is NULL" in err()
    for field in FIELDS:
        if field in OR_NULL + ("payload", "payload_cap", "info", "status"):
            continue
        assert _call(lib, word, **{field: None}) == _native.EINVAL, field
        assert b"rudp_receive_flows: " + field.encode() + b" is NULL" in err(), field
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    cpu8 = torch.zeros(4, dtype=torch.uint8)
    off = torch.zeros(2, dtype=torch.int64)
    flow = torch.zeros(1, dtype=torch.int32)
    states = torch.zeros((4, 4), dtype=torch.int64)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive_flows_fused(np.zeros(4, np.uint8), off, flow, "rudp5", states=states)
    with pytest.raises(ValueError, match="layout"):
        batch.receive_flows_fused(cpu8, off, flow, "rudp6", states=states)
    with pytest.raises(TypeError, match="out must be"):
        batch.receive_flows_fused(cpu8, off, flow, "rudp5", states=states, out=cpu8)
    with pytest.raises(ValueError, match="HIP device"):
        batch.receive_flows_fused(cpu8, off, flow, "rudp5", states=states)
    from rudp.flows import FlowReceiver
    import inspect
    assert inspect.signature(FlowReceiver.__init__).parameters["fused"].default is False
    sig = inspect.signature(batch.receive_flows_fused)
    assert list(sig.parameters) == ["frames", "frame_off", "flow", "layout", "states", "csum", "payload_cap", "out",
                                    "stream"]
    assert sig.parameters["layout"].default == "rudp7"
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[4:])


def test_result_layout():
    """Every array of the one allocation aligned to its element, none overlapping."""
    width = {"payload_off": 8, "flow_info": 8, "info": 8, "status": 4, "rank": 4, "order": 4, "order_off": 4,
             "chars": 4, "payload_src": 4, "reply_index": 4, "fin_flow": 4, "seq": 2, "ack": 2, "csum": 2,
             "reply_ack": 2, "reply_csum": 2, "fin_csum": 2, "flags": 1, "ok": 1, "valid": 1, "usable": 1, "accept": 1,
             "keep": 1, "reply": 1, "reply_frames": 1, "fin_frames": 1, "payload": 16}
    for n in (0, 1, 2, 3, 65, 1023, 1024):
        for H in (5, 7):
            cap = 6 * n + 1
            lay = batch.ReceivedFlowsFused.layout(n, H, cap)
            assert set(lay) == set(width) | {"size"}
            need = {"payload_off": 8 * (n + 1), "flow_info": 64 * n, "info": 96, "status": 4, "order_off": 4 * (n + 1),
                    "reply_frames": n * H, "fin_frames": n * H, "payload": cap}
            # (in layout order; empty arrays share an offset)
            at = [(lo, k) for lo, _, k in sorted((lay[k][0], lay[k][1], k) for k in width)]
            for (lo, k), (nxt, _) in zip(at, at[1:] + [(lay["size"], "")]):
                assert lo % width[k] == 0 and lay[k][1] >= need.get(k, width[k] * n), (n, H, k)
                assert lo + lay[k][1] <= nxt, (n, H, k)


def test_python_geometry_matches_the_kernel_source():
    csrc = REPO / "reliable-udp_amd" / "csrc"
    hip = (csrc / "receive_flows.hip").read_text()
    dev = (csrc / "flows_device.hpp").read_text()
    assert int(re.search(r"constexpr uint32_t kRfFusedBytes = (\d+);", hip).group(1)) == batch.FLOWS_FUSED_BYTES
    assert int(re.search(r"constexpr uint32_t kRfFusedMeanFrame = (\d+);", hip).group(1)) == batch.FLOWS_FUSED_MEAN
    assert (batch.FLOWS_FUSED_BYTES, batch.FLOWS_FUSED_MEAN) == (FUSED_BYTES, FUSED_MEAN)
    assert ("return knob && n <= kFlowMax && frames_bytes <= kRfFusedBytes &&\n"
            "         (knob == 2 || frames_bytes <= (uint64_t)kRfFusedMeanFrame * n);") in hip
    assert "static_assert(sizeof(RfLds) <= 160 * 1024" in hip
    # both kernels judge with the one device function
    assert dev.count("flows_judge_lds(") == 2 and "flows_judge_lds(a.f, L, N2, nullptr);" in hip
    assert "key == 83 ? &t.receive_flows_fused" in (csrc / "tuning.hip").read_text()
    assert "RUDP_KNOB(receive_flows_fused, 1)" in (csrc / "internal.hpp").read_text()
    from rudp import _build
    assert "receive_flows.hip" in _build.SOURCES


# ------------------------------------------------------------ the oracle
def _one_flow_frames(rng, n, H, fin_at):
    seq, flags, chars, usable = clean_stream(rng, n, fin_at=fin_at, max_chars=3)
    frames, off, side, texts = build_frames(rng, seq, flags, chars, usable, H)
    return frames, off, side, texts


@pytest.mark.parametrize("H", (5, 7))
def test_one_flow_is_the_single_peer_receiver(H):
    """One flow: accept_ref on the decoded tables and the join of the kept
    payloads, up to the turn-over of the row."""
    rng = random.Random(0x1F10 + H)
    for n, fin_at in ((1, None), (64, None), (257, 200), (300, 299)):
        frames, off, side, _ = _one_flow_frames(rng, n, H, fin_at)
        seq, _, flags, _, _, _, usable, chars = decode_ref(frames, off, H, side)
        one = accept_ref(seq, flags, chars, usable)
        table = np.zeros((9, 4), np.uint64)
        r = receive_flows_ref(frames, off, np.full(n, 5, np.uint32), table, H, side)
        f = r.flows
        assert f.accept.tolist() == one.accept.tolist() and f.keep.tolist() == one.keep.tolist()
        assert f.reply.tolist() == one.reply.tolist() and f.reply_ack.tolist() == one.reply_ack.tolist()
        want = b"".join(bytes(frames[off[i] + H:off[i + 1]]) for i in np.flatnonzero(one.keep))
        assert r.payload == want and r.info[8] == len(want) and int(r.payload_off[-1]) == len(want)
        assert r.payload_src.tolist() == np.flatnonzero(one.keep).tolist()
        if one.end < n:
            assert f.states[5].tolist() == [0, 0, 0, one.state[1] + 1] and r.fin_flow.tolist() == [0]
            assert len(r.fin_frames) == H and r.fin_frames[:5] == build(0, one.state[1] + one.characters, FIN | ACK)
        else:
            assert f.states[5].tolist() == [*one.state, 0] and len(r.fin_flow) == 0 and r.fin_frames == b""
        assert r.reply_index.tolist() == np.flatnonzero(one.reply).tolist()
        if H == 5:
            assert r.reply_frames == b"".join(build(0, int(a), ACK) for a in one.reply_ack[one.reply.astype(bool)])
        assert r.status == 0


def _send(rng, text, isn, fin):
    """A stop-and-wait sender's datagrams for ``text``: (seq, flags, chars) rows
    of 1-3 characters, some sent twice."""
    rows, k = [], 0
    while k < len(text):
        c = min(rng.randint(1, 3), len(text) - k)
        fl = (SYN if k == 0 else 0) | (FIN if fin and k + c == len(text) else 0)
        rows.append(((isn + k) & 0xFFFF, fl, text[k:k + c]))
        if rng.random() < 0.3:
            rows.append(((isn + k) & 0xFFFF, fl & ~FIN & 0xFF, text[k:k + c]))
        k += c
    return rows


@pytest.mark.parametrize("H", (5, 7))
def test_pieces_across_batches_join_to_the_text_and_closing_frames(H):
    """Every flow's pieces over three batches decode to the text its sender
    sent, and its closing frame is build(0, isn + characters, FIN | ACK), with
    an ISN within 3 of 65535 among them."""
    from oracle import codec_np
    rng = random.Random(0x7E87 + H)
    # (a seq_num past 65535 is never accepted, as in the reference: the two high ISNs send short texts whose
    # last datagram still starts at or below 65535, so only the closing ack wraps)
    texts = ["héllo", "日本語", "plain ascii text here " * 3, "😀 emoji 😀 mix ñ " * 3]
    isns = [65533, 65535, 1200, 7]
    slots = [3, 0, 11, 7]
    sent = [[(65533, SYN, "hé"), (65533, SYN, "hé"), (65535, FIN, "llo")], [(65535, SYN | FIN, "日本語")]]
    sent += [_send(rng, t, isn, fin=True) for t, isn in zip(texts[2:], isns[2:])]
    cut = [[0, len(s) // 3, 2 * len(s) // 3, len(s)] for s in sent]
    table = np.zeros((12, 4), np.uint64)
    got = {s: b"" for s in slots}
    closed = {}
    for b in range(3):
        streams = []
        for k, s in enumerate(sent):
            part = s[cut[k][b]:cut[k][b + 1]]
            streams.append((np.array([r[0] for r in part], np.uint16), np.array([r[1] for r in part], np.uint8),
                            np.arange(len(part), dtype=np.uint32), np.ones(len(part), np.uint8)))
        seq, flags, pick, _, flow = interleave(rng, streams, slots)  # (chars carries the row index through)
        payloads = []
        for i in range(len(seq)):
            k = slots.index(int(flow[i]))
            payloads.append(sent[k][cut[k][b] + int(pick[i])][2].encode())
        frames, off, cs = codec_np.encode_varlen(seq, np.zeros(len(seq), np.uint16), flags, payloads, H)
        r = receive_flows_ref(frames, off, flow, table, H, cs if H == 5 else None)
        assert r.status == 0 and r.usable.all()
        table = r.flows.states
        for a, row in enumerate(r.flows.flow_info.tolist()):
            base, kept = row[7], row[6]
            if row[3] < len(seq):  # a (repeated) SYN started the transfer again: what came before is dropped
                got[row[0]] = b""
            got[row[0]] += r.payload[int(r.payload_off[base]):int(r.payload_off[base + kept])]
        for e, a in enumerate(r.fin_flow.tolist()):
            row = r.flows.flow_info[a].tolist()
            closed[row[0]] = (r.fin_frames[e * H:(e + 1) * H], row[5], row[4], int(r.fin_csum[e]))
    assert set(closed) == set(slots)
    for k, s in enumerate(slots):
        assert got[s].decode() == texts[k], k
        frame, isn, characters, cs = closed[s]
        assert isn == isns[k] and characters == len(texts[k])
        want = build(0, isn + characters, FIN | ACK)  # (the rudp5 frame; build wraps the ack itself)
        assert frame[:5] == want and cs == codec_np.inet_checksum(want)
        if H == 7:
            assert frame[5:] == cs.to_bytes(2, "big")
    assert isns[0] + len(texts[0]) > 65535 and isns[1] + len(texts[1]) > 65535  # the ack wrapped


def test_builder_realises_unusable_by_damage_and_stays_small():
    """make_batch's mix through build_frames: usable from the bytes is the mix's
    usable, all three kinds of damage occur, chars of the usable datagrams are
    the mix's, and the n = 1024 batches stay inside the fused form's limits."""
    for n_active in (1, 37, 1024):
        for H in (5, 7):
            rng = random.Random(0xB111D + n_active + H)
            seq, flags, chars, usable, flow = make_batch(rng, 1024, n_active, 5000)
            frames, off, side, texts = build_frames(rng, seq, flags, chars, usable, H)
            d = decode_ref(frames, off, H, side)
            assert d[6].tolist() == usable.tolist()
            us = usable.astype(bool)
            assert d[7][us].tolist() == chars[us].tolist() and d[0][us].tolist() == seq[us].tolist()
            assert {0, 2} <= set(d[3][~us].tolist()) and (d[5][~us] == 0).any()  # bad checksum, short, not UTF-8
            assert len(frames) <= FUSED_BYTES and len(frames) <= FUSED_MEAN * 1024
            assert all((t is None) == (not u) for t, u in zip(texts, usable))
    assert FLOW_NONE == 0xFFFFFFFF


def test_mix_conditions_of_the_largest_gpu_batch():
    """The n = 1024 / 37-flow batches of tests/test_gpu_receive_flows.py (the
    same seeds, drawn in the same order) contain every path, by the oracle."""
    from receive_flows_ref import N_FLOWS, mix_case
    from test_gpu_flows import mix_conditions
    for layout in (5, 7):
        rng = random.Random(0x2F10 + 16 * 1024 + layout)
        for n_active in (1, rng.choice((2, 3)), 37):
            frames, off, side, flow, table = mix_case(rng, 1024, n_active, layout)
        r = receive_flows_ref(frames, off, flow, table, layout, side)
        c = mix_conditions(r.flows, 1024, flow)
        assert c["ended_with_tail"] >= 1 and c["anomalous"] >= 1 and c["exact"] >= 1, c
        assert c["flowless"] >= 1 and c["restarted"] >= 1 and c["ended"] >= 3, c
        assert {0, N_FLOWS - 1} <= set(flow.tolist())
        assert len(r.fin_flow) == c["ended"] and r.info[8] > 0 and r.info[2] > 0
        assert len(frames) <= FUSED_BYTES and len(frames) <= FUSED_MEAN * 1024
