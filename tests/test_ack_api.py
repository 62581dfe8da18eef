"""rudp_ack_progress / rudp_acknowledge (added within ABI 8) at the boundary: the
symbols and the struct, the argument checks that run before any device call,
the Python validation, the plain-loop rule against the transfers the reference
sent (tests/golden/ack.json), and the numpy model of the device's one-scan form
against the rule.  CPU-only."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from ack_ref import (ACK, CUMULATIVE, EXACT, FIN, ack_ref, adversarial_replies, canonical, clean_replies, fresh_state,
                     golden_cases, header, parse_rudp5, scan_model)
from conftest import REPO
from rudp import _native, batch

NAMES = ("rudp_ack_progress", "rudp_acknowledge")
FIELDS = ("seq", "ack", "flags", "ok", "csum_out", "usable", "valid", "pointer", "state_out", "info", "final_frame",
          "final_csum", "status")


def test_symbols_header_and_struct():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^#define RUDP_HAS_ACKNOWLEDGE 1\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ACK_EXACT 0\b", text, flags=re.M) and _native.ACK_EXACT == 0
    assert re.search(r"^#define RUDP_ACK_CUMULATIVE 1\b", text, flags=re.M) and _native.ACK_CUMULATIVE == 1
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    for name in NAMES:
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(rf"^RUDP_API int {name}\(", text, flags=re.M)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        for name in NAMES:
            assert any(ln.split()[-1] == name and ln.split()[1] == "T" for ln in out.splitlines()), (path, name)
    # struct rudp_acknowledged: the header's members in the binding's order, 8 bytes each
    body = re.search(r"typedef struct rudp_acknowledged \{(.*?)\} rudp_acknowledged;", text, flags=re.S).group(1)
    members = [m.replace("_or_null", "") for m in re.findall(r"(\w+);", body)]
    assert members == list(FIELDS) == [f[0] for f in _native.RudpAcknowledged._fields_]
    assert ctypes.sizeof(_native.RudpAcknowledged) == 8 * len(FIELDS)
    # the usable rule is stated where a C caller reads it
    assert "RUDP_OK_GOOD or RUDP_OK_UNVERIFIED" in text and "UTF-8\n *                 validity is not required" in text


def test_argument_errors_before_device():
    lib = _native.lib()
    err = lib.rudp_last_error
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    p = ctypes.cast(word, ctypes.c_void_p)

    def progress(seq=p, ack=p, flags=p, n=1, isn=100, T=10, C=2, mode=0, sent=10, st_in=p, valid=p, ptr=p, st_out=p,
                 info=p, device=0):
        return lib.rudp_ack_progress(seq, ack, flags, None, n, isn, T, C, mode, sent, st_in, valid, ptr, st_out, info,
                                     device, None)

    for kw, name in (("st_in", b"d_state_in"), ("st_out", b"d_state_out"), ("info", b"d_info")):
        for n in (0, 1):
            assert progress(**{kw: None, "n": n}) == _native.EINVAL and name + b" is NULL" in err()
    for kw, name in (("seq", b"d_seq"), ("ack", b"d_ack"), ("flags", b"d_flags"), ("valid", b"d_valid"),
                     ("ptr", b"d_pointer")):
        assert progress(**{kw: None}) == _native.EINVAL and name + b" is NULL" in err()
    for n in (0, 1):
        assert progress(n=n, isn=65536) == _native.EINVAL and b"isn" in err()
        for C in (0, 16384):
            assert progress(n=n, C=C) == _native.EINVAL and b"chunk_chars" in err()
        for mode in (-1, 2):
            assert progress(n=n, mode=mode) == _native.EINVAL and b"mode" in err()
        assert progress(n=n, sent=11) == _native.EINVAL and b"sent_chars" in err()
    # n == 0 needs no table: the checks let it through to the device choice (none is touched here)
    assert progress(seq=None, ack=None, flags=None, valid=None, ptr=None, n=0, device=-1) != 0
    assert b"NULL" not in err()

    def whole(frames=p, nbytes=8, off=p, n=1, csum=None, isn=100, T=10, C=2, mode=0, sent=10, st_in=p, layout=5,
              out="o", device=0, **null):
        o = _native.RudpAcknowledged(**{f: p.value for f in FIELDS})
        for name in null:
            setattr(o, name, None)
        return lib.rudp_acknowledge(frames, nbytes, off, 0, n, csum, isn, T, C, mode, sent, st_in,
                                    ctypes.byref(o) if out == "o" else None, layout, device, None)

    assert whole(out=None) == _native.EINVAL and b"out is NULL" in err()
    assert whole(layout=6) == _native.EINVAL and b"layout" in err()
    assert whole(layout=7, csum=p) == _native.EINVAL and b"d_csum_in" in err()
    for n in (0, 1):
        assert whole(n=n, st_in=None) == _native.EINVAL and b"d_state_in" in err()
        for field in ("state_out", "info", "status"):
            assert whole(n=n, **{field: None}) == _native.EINVAL and field.encode() + b" is NULL" in err(), field
        assert whole(n=n, isn=70000) == _native.EINVAL and b"isn" in err()
        assert whole(n=n, C=0) == _native.EINVAL and b"chunk_chars" in err()
        assert whole(n=n, mode=7) == _native.EINVAL and b"mode" in err()
        assert whole(n=n, sent=11) == _native.EINVAL and b"sent_chars" in err()
    assert whole(off=None) == _native.EINVAL and b"d_frame_off" in err()
    assert whole(frames=None) == _native.EINVAL and b"d_frames" in err()
    for field in ("seq", "ack", "flags", "ok", "usable", "valid", "pointer", "final_frame"):
        assert whole(**{field: None}) == _native.EINVAL
        assert b"rudp_acknowledge: " + field.encode() + b" is NULL" in err(), field
    none = {f: None for f in FIELDS if f not in ("state_out", "info", "status")}
    assert whole(frames=None, nbytes=0, off=None, n=0, device=-1, **none) != 0 and b"NULL" not in err()
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    cpu8 = torch.zeros(4, dtype=torch.uint8)
    cpu16 = torch.zeros(4, dtype=torch.uint16)
    off = torch.zeros(2, dtype=torch.int64)
    kw = dict(isn=100, total_chars=10, chunk=2)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.acknowledge(np.zeros(4, np.uint8), off, "rudp5", **kw)
    with pytest.raises(ValueError, match="layout"):
        batch.acknowledge(cpu8, off, "rudp6", **kw)
    with pytest.raises(ValueError, match="HIP device"):
        batch.acknowledge(cpu8, off, "rudp5", **kw)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.ack_progress(np.zeros(4, np.uint16), cpu16, cpu8, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        batch.ack_progress(cpu16, cpu16, cpu8, **kw)
    for bad in (dict(isn=65536), dict(isn=-1), dict(isn=True), dict(chunk=0), dict(chunk=16384), dict(total_chars=-1),
                dict(mode="greedy"), dict(sent=11), dict(sent=-1)):
        with pytest.raises(ValueError, match=next(iter(bad)).split("_")[0]):
            batch.acknowledge(cpu8, off, "rudp5", **{**kw, **bad})
    assert batch.fresh_ack_state(10, 3) == (0, 3, 0, 0) == fresh_state(10, 3)
    assert batch.fresh_ack_state(2, 3) == (0, 2, 1, 0) and batch.fresh_ack_state(0, 1) == (0, 0, 1, 0)
    # the layouts of the one result allocation: every array aligned to its element, none overlapping
    width = {"pointer": 8, "state": 8, "info": 8, "status": 4, "seq": 2, "ack": 2, "csum": 2, "final_csum": 2,
             "flags": 1, "ok": 1, "usable": 1, "valid": 1, "final_frame": 1}
    fixed = {"state": 32, "info": 64, "status": 4, "final_csum": 2, "final_frame": 7}
    for n in (0, 1, 2, 3, 1023, 1024, 1025):
        for lay in (batch.Acknowledged.layout(n, 7), batch.AckProgress.layout(n)):
            at = [(lay[k], k) for k in lay if k != "size"]  # (in layout order: empty arrays share an offset)
            assert at == sorted(at, key=lambda e: e[0]) and all(lo % width[k] == 0 for lo, k in at), n
            for (lo, k), (nxt, _) in zip(at, at[1:] + [(lay["size"], "")]):
                assert lo + fixed.get(k, width[k] * n) <= nxt, (n, k)


def _case_arrays(c):
    return parse_rudp5([bytes.fromhex(h) for h in c["replies"]])


def test_rule_reproduces_every_reference_transfer():
    """ack.json holds what the reference's send() sent after every reply; the
    rule, one call over all replies, ends where it did."""
    cases = golden_cases()
    names = {c["name"] for c in cases}
    assert {"wire_trace", "stale", "future", "no_ack_flag_middle", "no_ack_flag_last", "fin_without_ack",
            "stray_fin_wrong_ack", "empty_message", "isn_65530_stall", "fin_seq_65535", "duplicated_chunk1"} <= names
    assert sum(n.startswith("text") for n in names) == 125 and len(cases) == 145
    for c in cases:
        seq, ack, flags = _case_arrays(c)
        T, C, isn = len(c["message"]), c["chunk"], c["isn"]
        r = ack_ref(seq, ack, flags, isn=isn, T=T, C=C)
        assert (r.state[0], r.done) == (c["pointer"], c["done"]), c["name"]
        last_index, last_sent = c["sent"][-1]
        if r.done:
            assert last_index == r.end and bytes.fromhex(last_sent) == header(*r.final, ACK), c["name"]
        else:
            assert r.end == len(ack), c["name"]
        # every datagram went out after a valid reply, and no other valid reply but those for the last frame
        sent_after = {i for i, _ in c["sent"] if i >= 0}
        assert sent_after <= set(np.flatnonzero(r.valid).tolist()), c["name"]
    stall = next(c for c in cases if c["name"] == "isn_65530_stall")
    assert stall["pointer"] == 5 and not stall["done"]  # isn + 5 + 1 = 65536 never arrives
    wrap = next(c for c in cases if c["name"] == "fin_seq_65535")
    assert wrap["sent"][-1][1] == header(7 + 2, 0, ACK).hex()
    late = next(c for c in cases if c["name"] == "no_ack_flag_last_then_stale_fin")
    assert late["done"] and late["pointer"] == 10 < len(late["message"])  # the quirk: done before everything is acknowledged


def _model_matches_rule(seq, ack, flags, usable, **kw):
    r = ack_ref(seq, ack, flags, usable, **kw)
    m = scan_model(ack, flags, usable, **kw)
    n = len(ack)
    upto = min(m.first_anomaly + 1, m.end_guess + 1, n)  # the anomaly itself is still judged exactly
    if not canonical(kw["state"], kw["T"], kw["C"]):
        upto = 0  # a seed the guess does not cover: the walk starts at reply 0
    assert m.valid[:upto].tolist() == r.valid[:upto].tolist()
    before = min(m.first_anomaly, m.end_guess + 1, n)
    pointer_before = np.concatenate(([kw["state"][0] if kw.get("state") else 0], r.pointer[:-1]))[:before]
    assert m.guess[:before].tolist() == pointer_before.tolist()
    if m.first_anomaly == n:
        assert m.end_guess == r.end
    else:
        assert r.end > m.first_anomaly or (m.first_anomaly == 0 and not canonical(kw["state"], kw["T"], kw["C"]))
    return m


def _random_state(rng, T, C):
    k = rng.random()
    if k < 0.4:
        return fresh_state(T, C)
    p = min(rng.randrange(0, T // C + 2) * C, T)
    L = min(C, T - p)
    if k < 0.8:
        return p, L, int(p + L == T), 0
    return rng.choice(((p, 0, 1, 0), (p, L, 1 - int(p + L == T), 0), (min(p + 1, T), L, 0, 0), (p, L + 1, 0, 0)))


def test_scan_model_is_exact_before_its_first_anomaly():
    rng = random.Random(0xAC4901)
    anomalies = clean = 0
    for k in range(20000):
        n = rng.randint(1, 40)
        C = rng.choice((1, 1, 2, 3, 5, 16))
        T = rng.choice((0, 1, C, 3 * C, 3 * C + 1, 7 * C - 1, 40))
        isn = rng.choice((0, 100, 3611, 65530, 65535 - T))
        mode = rng.choice((EXACT, CUMULATIVE))
        sent = rng.randint(0, T) if mode == CUMULATIVE and rng.random() < 0.5 else None
        if rng.random() < 0.5:
            seq, ack, flags, usable = adversarial_replies(rng, n, isn=max(isn, 0), T=T, C=C)
        else:
            seq, ack, flags, usable = clean_replies(rng, n, isn=max(isn, 0), T=T, C=C, W=rng.choice((1, 8)))
            for _ in range(rng.randint(0, 2)):  # one or two replies of a clean stream disturbed
                j = rng.randrange(n)
                flags[j] = rng.choice((0, FIN, ACK | FIN, flags[j]))
                ack[j] = (int(ack[j]) + rng.choice((0, C, 2 * C, -C, 1))) & 0xFFFF
        m = _model_matches_rule(seq, ack, flags, usable, isn=max(isn, 0), T=T, C=C, state=_random_state(rng, T, C),
                                mode=mode, sent=sent)
        anomalies += m.first_anomaly < n
        clean += m.first_anomaly == n
    assert anomalies > 2000 and clean > 2000  # both kinds of stream were seen


def test_clean_streams_have_no_anomaly():
    """The condition the GPU tests' fast-path assertions rest on."""
    for c in golden_cases():
        seq, ack, flags = _case_arrays(c)
        if all(f == ACK or f == ACK | FIN for f in flags) and c["name"] != "future" and "stray" not in c["name"]:
            m = _model_matches_rule(seq, ack, flags, None, isn=c["isn"], T=len(c["message"]), C=c["chunk"],
                                    state=fresh_state(len(c["message"]), c["chunk"]))
            assert m.first_anomaly == len(ack), c["name"]
    rng = random.Random(0x5704)
    ended = 0
    for k in range(1000):
        n = rng.randint(1, 120)
        C = rng.choice((1, 1, 3, 16))
        T = rng.choice((0, 1, 5, 30, 200))
        isn = rng.choice((1, 3611, 65530))
        W = rng.choice((1, 8, 64))
        for mode in (EXACT, CUMULATIVE):
            seq, ack, flags, usable = clean_replies(rng, n, isn=isn, T=T, C=C, W=W)
            state = fresh_state(T, C)
            m = _model_matches_rule(seq, ack, flags, usable, isn=isn, T=T, C=C, state=state, mode=mode)
            assert m.first_anomaly == n, (k, mode)
            ended += m.end_guess < n
    assert ended > 200  # transfers that reached their FIN were among them


def test_python_geometry_matches_the_kernel_source():
    """batch.ACK_TILE / ACK_FUSED_BYTES / ACK_FUSED_MEAN restate acknowledge.hip's
    launch geometry (the GPU tests put their edge cases there)."""
    csrc = REPO / "reliable-udp_amd" / "csrc"
    hip = (csrc / "acknowledge.hip").read_text()
    block = int(re.search(r"constexpr int kBlock = (\d+);", (csrc / "codec_device.hpp").read_text()).group(1))
    fpt = int(re.search(r"constexpr uint32_t kAckFpt = (\d+);", hip).group(1))
    assert re.search(r"constexpr uint32_t kAckTile = kBlock \* kAckFpt;", hip)
    assert batch.ACK_TILE == block * fpt
    assert "if (a.n <= kAckTile) {" in hip  # the one-launch form covers exactly one tile
    assert int(re.search(r"constexpr uint32_t kAckFusedBytes = (\d+);", hip).group(1)) == batch.ACK_FUSED_BYTES
    assert int(re.search(r"constexpr uint32_t kAckFusedMeanFrame = (\d+);", hip).group(1)) == batch.ACK_FUSED_MEAN
    assert ("return knob && n <= kAckTile && frames_bytes <= kAckFusedBytes &&\n"
            "         (knob == 2 || frames_bytes <= (uint64_t)kAckFusedMeanFrame * n);") in hip
    # the fused form's LDS stays within what a workgroup gets without asking
    assert "uint32_t img[(kAckFusedBytes + 16u + 32u) / 4u];" in hip
    T = batch.ACK_TILE
    lds = (8 + 4 + 2 + 1 + 1 + 1) * T + 128 + 4 * (T + 1) + 2 * T + 16 + batch.ACK_FUSED_BYTES + 48
    assert lds <= 65536
    # knob 81 of the diagnostics build turns the fused form off
    assert "key == 81 ? &t.acknowledge_fused" in (csrc / "tuning.hip").read_text()
