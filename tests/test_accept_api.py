"""rudp_payload_chars / rudp_accept_inorder (added within ABI 8) at the boundary:
the symbols, the argument checks that run before any device call, the Python
validation, the plain-loop rule against the streams the reference judged
(tests/golden/accept.json), and the numpy model of the device's one-scan form
against the rule.  CPU-only."""
import ctypes
import random
import re
import subprocess

import numpy as np
import pytest

from accept_ref import (accept_ref, adversarial_stream, chars_ref, clean_stream, golden_cases, pack_frames,
                        parse_rudp5, scan_model)
from conftest import REPO
from rudp import _native, batch

NAMES = ("rudp_payload_chars", "rudp_accept_inorder")


def _case_arrays(c):
    frames = [bytes.fromhex(h) for h in c["frames"]]
    seq, flags, payloads = parse_rudp5(frames)
    buf, off = pack_frames(frames)
    chars = chars_ref(buf, off, 5)
    assert chars.tolist() == [len(p.decode()) for p in payloads]  # lead bytes are Python's len()
    return frames, seq, flags, chars


def test_symbols_and_header():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^#define RUDP_HAS_ACCEPT_INORDER 1\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    for name in NAMES:
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert re.search(rf"^RUDP_API int {name}\(", text, flags=re.M)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        for name in NAMES:
            assert any(ln.split()[-1] == name and ln.split()[1] == "T" for ln in out.splitlines()), (path, name)


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    p = ctypes.cast(word, ctypes.c_void_p)

    def chars(frames=p, nbytes=8, off=p, n=1, out=p, layout=5):
        return lib.rudp_payload_chars(frames, nbytes, off, 0, n, out, layout, 0, None)

    assert chars(layout=6) == _native.EINVAL and b"layout" in lib.rudp_last_error()
    assert chars(off=None) == _native.EINVAL and b"d_frame_off" in lib.rudp_last_error()
    assert chars(out=None) == _native.EINVAL and b"d_chars" in lib.rudp_last_error()
    assert chars(frames=None) == _native.EINVAL and b"d_frames" in lib.rudp_last_error()
    assert chars(frames=None, off=None, out=None, n=0) == 0  # an empty batch touches nothing

    def accept(seq=p, flags=p, ch=p, n=1, st_in=p, acc=p, keep=p, rep=p, ack=p, st_out=p, info=p):
        return lib.rudp_accept_inorder(seq, flags, ch, None, n, 0xFFFFFFFF, st_in, acc, keep, rep, ack, st_out, info,
                                       0, None)

    for kw, name in (("st_in", b"d_state_in"), ("st_out", b"d_state_out"), ("info", b"d_info")):
        for n in (0, 1):
            assert accept(**{kw: None, "n": n}) == _native.EINVAL
            assert name in lib.rudp_last_error()
    for kw, name in (("seq", b"d_seq"), ("flags", b"d_flags"), ("ch", b"d_chars"), ("acc", b"d_accept"),
                     ("keep", b"d_keep"), ("rep", b"d_reply"), ("ack", b"d_reply_ack")):
        assert accept(**{kw: None}) == _native.EINVAL
        assert name in lib.rudp_last_error()
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    cpu8 = torch.zeros(4, dtype=torch.uint8)
    off = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):
        batch.payload_chars(cpu8, off, "rudp5")
    with pytest.raises(ValueError, match="layout"):
        batch.payload_chars(cpu8, off, "rudp6")
    with pytest.raises(TypeError, match="torch tensors"):
        batch.payload_chars(np.zeros(4, np.uint8), off, "rudp5")
    seq = torch.zeros(4, dtype=torch.uint16)
    with pytest.raises(ValueError, match="HIP device"):
        batch.accept_inorder(seq, cpu8, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="torch tensors"):
        batch.accept_inorder(np.zeros(4, np.uint16), cpu8, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive_batch(np.zeros(4, np.uint8), off, "rudp5")
    with pytest.raises(ValueError, match="layout"):
        batch.receive_batch(cpu8, off, "rudp6")
    for bad in (-1, True, 1.5, "7"):
        with pytest.raises(ValueError, match="last_isn"):
            batch.receive_batch(cpu8, off, "rudp5", last_isn=bad)
    assert batch._check_last_isn(None) == batch.NO_ISN and batch._check_last_isn(3611) == 3611
    # the layout of the one result allocation: every array aligned to its element
    for n in (0, 1, 2, 3, 1023, 1024, 1025):
        lay = batch.Accepted.layout(n)
        assert lay[:3] == (0, n, 2 * n) and lay[3] >= 3 * n and lay[3] % 2 == 0
        assert lay[4] >= lay[3] + 2 * n and lay[4] % 8 == 0 and lay[5] == lay[4] + 32 and lay[6] == lay[5] + 48
    # the lanes the kernel picks for a typical frame length (geometry only)
    assert [batch.payload_chars_lanes(h, 5) for h in (0, 6, 68, 69, 133, 1479, 70000)] == [1, 1, 1, 2, 4, 32, 64]
    assert "usable" in batch.keep_mask.__doc__ and "would append" not in batch.keep_mask.__doc__


def test_rule_reproduces_every_reference_stream():
    cases = golden_cases()
    names = {c["name"] for c in cases}
    assert {"wire_trace", "isn_65530_stall", "repeated_syn_peer", "new_syn_mid_transfer", "empty_message",
            "future_frame", "stray_no_peer", "stray_peer"} <= names and len(cases) == 142
    assert sum(n.startswith("text") for n in names) == 125
    for c in cases:
        frames, seq, flags, chars = _case_arrays(c)
        r = accept_ref(seq, flags, chars, None, tuple(c["state"]), c["last_isn"])
        assert "".join(map(str, r.accept)) == c["accepted"], c["name"]
        assert "".join(map(str, r.reply)) == c["replied"], c["name"]
        assert r.reply_ack.tolist() == c["ack"], c["name"]
        assert r.end == c["end"] and list(r.state) == c["state_after"], c["name"]
        assert b"".join(frames[i][5:] for i in np.flatnonzero(r.keep)).decode() == c["message"], c["name"]
        assert r.characters == (len(c["message"]) if r.state[2] else 0), c["name"]
    stall = next(c for c in cases if c["name"] == "isn_65530_stall")
    assert stall["message"] == "wraps " and stall["end"] == len(stall["frames"]) and stall["state_after"][0] == 65536


def _model_matches_rule(seq, flags, chars, usable, state, last_isn):
    r = accept_ref(seq, flags, chars, usable, state, last_isn)
    m = scan_model(seq, flags, chars, usable, state, last_isn)
    upto = min(m.first_anomaly + 1, m.end_guess + 1, len(seq))  # the anomaly itself is still judged exactly
    assert m.accept[:upto].tolist() == r.accept[:upto].tolist()
    if m.first_anomaly == len(seq):
        assert m.end_guess == r.end
    else:
        assert r.end > m.first_anomaly
    return m


def test_scan_model_is_exact_before_its_first_anomaly():
    rng = random.Random(0xACCE97)
    anomalies = 0
    for k in range(300):
        n = rng.randint(1, 200)
        state = rng.choice(((0, 0, 0), (0, 0, 1), (105, 100, 1), (65536, 65530, 1)))
        seq, flags, chars, usable = adversarial_stream(rng, n, p_fin=rng.choice((0.0, 0.01, 0.05)))
        last = rng.choice((None, int(seq[0]), 3611))
        m = _model_matches_rule(seq, flags, chars, usable, state, last)
        anomalies += m.first_anomaly < n
    assert 50 < anomalies < 300  # both kinds of stream were seen


def test_clean_streams_have_no_anomaly():
    """The condition the GPU tests' fast-path assertions rest on."""
    for c in golden_cases():
        if c["clean"]:
            _, seq, flags, chars = _case_arrays(c)
            m = _model_matches_rule(seq, flags, chars, None, tuple(c["state"]), c["last_isn"])
            assert m.first_anomaly == len(seq), c["name"]
    rng = random.Random(0x5703)
    for k in range(1000):
        n = rng.randint(1, 120)
        fin_at = rng.choice((None, n - 1, rng.randrange(n)))
        seq, flags, chars, usable = clean_stream(rng, n, fin_at=fin_at, max_chars=rng.choice((1, 1, 3, 16)),
                                                 p_reset=0.03, high_isn=0.3,
                                                 resets=[rng.randrange(n) for _ in range(rng.randint(0, 2))])
        state = rng.choice(((0, 0, 0), (0, 0, 1)))
        m = _model_matches_rule(seq, flags, chars, usable, state, rng.choice((None, 77777, 6000)))
        assert m.first_anomaly == n, k


def test_python_geometry_matches_the_kernel_source():
    """batch.ACCEPT_TILE / ACCEPT_BASES / CHARS_BLOCK / payload_chars_lanes restate
    accept.hip's launch geometry (the GPU tests put their edge cases there)."""
    csrc = REPO / "reliable-udp_amd" / "csrc"
    hip = (csrc / "accept.hip").read_text() + (csrc / "accept_device.hpp").read_text()
    block = int(re.search(r"constexpr int kBlock = (\d+);", (csrc / "codec_device.hpp").read_text()).group(1))
    fpt = int(re.search(r"constexpr uint32_t kAccFpt = (\d+);", hip).group(1))
    assert re.search(r"constexpr uint32_t kAccTile = kBlock \* kAccFpt;", hip)
    assert batch.ACCEPT_TILE == block * fpt and batch.CHARS_BLOCK == block
    # the bases pass: one workgroup of kBlock threads, ceil(nt / kBlock) tiles per thread
    assert "hipLaunchKernelGGL(accept_bases_kernel, dim3(1), dim3(kBlock)" in hip
    assert "const uint64_t per = (nt + kBlock - 1u) / kBlock;" in hip
    assert batch.ACCEPT_BASES == block
    # the one-launch form covers exactly one tile
    assert "if (a.n <= kAccTile && tuning().accept_single)" in hip
    # lanes per frame: the launcher's rule, term by term
    assert "const uint64_t per = kBlock >> a.glog;" in hip
    rule = re.search(r"const uint32_t blocks = \(len_hint > H \? len_hint - H : 0u\) / (\d+)u \+ 1u;\s*"
                     r"uint32_t glog = 0;\s*while \(glog < (\d+)u && blocks > \((\d+)u << glog\)\) \+\+glog;", hip)
    assert rule, "payload_chars_glog changed: restate it in batch.payload_chars_lanes"
    vec, top, per_lane = map(int, rule.groups())
    for H in (5, 7):
        for hint in list(range(0, 300)) + [519, 1031, 1479, 4096, 5000, 70000, 0xFFFFFFFF]:
            blocks, glog = max(hint - H, 0) // vec + 1, 0
            while glog < top and blocks > (per_lane << glog):
                glog += 1
            assert batch.payload_chars_lanes(hint, H) == 1 << glog, (hint, H)


def test_keep_mask_usable_frames():
    """ok == 1, valid where judged, not a retransmission; rudp5 frames decoded
    without a checksum (ok == 3) only with unverified=True."""
    import torch
    from types import SimpleNamespace
    ok = torch.tensor([0, 1, 2, 3, 4, 1, 3, 3], dtype=torch.uint8)
    valid = torch.tensor([1, 1, 1, 1, 1, 0, 0, 1], dtype=torch.uint8)
    dup = torch.tensor([0, 0, 0, 0, 0, 0, 0, 1], dtype=torch.uint8)
    dec = SimpleNamespace(ok=ok, valid=valid)
    assert batch.keep_mask(dec).tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    assert batch.keep_mask(dec, unverified=True).tolist() == [0, 1, 0, 1, 0, 0, 0, 1]
    assert batch.keep_mask(dec, dup, unverified=True).tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert batch.keep_mask(SimpleNamespace(ok=ok, valid=None), unverified=True).tolist() == [0, 1, 0, 1, 0, 1, 1, 1]
    assert batch.keep_mask(SimpleNamespace(ok=ok, valid=None), dup).tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
    assert batch.keep_mask(dec).dtype == torch.uint8
