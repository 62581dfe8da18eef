"""rudp_segment_utf8 (added within ABI 8) at the boundary: the symbol, its
constants, the argument checks that run before any device call, the Python
validation, and the numpy restatement against the reference's frames.  CPU-only."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from rudp import _native, batch
from segment_ref import frames_rudp5, golden_cases, segment_ref


def test_symbol_and_constants():
    lib = _native.lib()
    assert lib.rudp_abi_version() == 8 == _native.ABI_VERSION
    assert hasattr(lib, "rudp_segment_utf8")
    assert "rudp_segment_utf8" in _native.EXPORTS
    assert _native.ST_PACKETS_CAP == 32
    assert any(bit == _native.ST_PACKETS_CAP for bit, _ in batch._ST_MESSAGES)


def test_header_and_libraries_agree_on_the_symbol():
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^RUDP_API int rudp_segment_utf8\(", text, flags=re.M)
    assert re.search(r"^#define RUDP_ST_PACKETS_CAP 32u", text, flags=re.M)
    assert re.search(r"^#define RUDP_HAS_SEGMENT_UTF8 1\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == "rudp_segment_utf8" and ln.split()[1] == "T" for ln in out.splitlines()), path


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 4)(*([0x5A5A5A5A5A5A5A5A] * 4))
    p = ctypes.cast(word, ctypes.c_void_p)

    def call(msg=p, nbytes=8, chunk=1, cap=1, seq=p, ack=p, flags=p, ln=p, off=p, count=p, status=p):
        return lib.rudp_segment_utf8(msg, nbytes, chunk, 0, cap, seq, ack, flags, ln, off, count, status, 0, None)

    for chunk in (0, 16384, 0xFFFFFFFF):
        assert call(chunk=chunk) == _native.EINVAL
        assert b"chunk_chars" in lib.rudp_last_error()
    for name in ("count", "status"):
        assert call(**{name: None}) == _native.EINVAL
        assert b"d_" + name.encode() in lib.rudp_last_error()
    assert call(msg=None) == _native.EINVAL
    assert b"d_msg" in lib.rudp_last_error()
    for kw, name in (("seq", b"d_seq"), ("ack", b"d_ack"), ("flags", b"d_flags"), ("ln", b"d_len")):
        assert call(**{kw: None}) == _native.EINVAL
        assert name in lib.rudp_last_error()
    # a bad chunk is reported whatever else is passed, the size query included
    assert call(chunk=0, cap=0, seq=None, ack=None, flags=None, ln=None, off=None) == _native.EINVAL
    assert b"chunk_chars" in lib.rudp_last_error()
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 4  # nothing was touched


def test_python_validation():
    import torch
    for chunk in (0, -1, 16384, 1.5, True, None):
        with pytest.raises(ValueError, match="chunk"):
            batch.segment_message("abc", 1, chunk=chunk)
        with pytest.raises(ValueError, match="chunk"):
            batch.frame_message("abc", 1, chunk=chunk)
    cpu = torch.zeros(4, dtype=torch.uint8)
    for fn in (batch.segment_message, batch.frame_message):
        with pytest.raises(ValueError, match="HIP device"):
            fn(cpu, 1)
        with pytest.raises(ValueError, match="HIP device"):
            fn("abc", 1, device="cpu")
        with pytest.raises(TypeError, match="str or a u8"):
            fn(np.zeros(4, np.uint8), 1)
        with pytest.raises(TypeError, match="str or a u8"):
            fn(b"abc", 1)
    with pytest.raises(ValueError, match="layout"):
        batch.frame_message("abc", 1, layout="rudp6")


def test_non_u8_tensor_is_refused():
    """Without a device here the tensor is a host one: either complaint refuses it
    (tests/test_gpu_segment.py has the device tensor, where the dtype is the reason)."""
    import torch
    for fn in (batch.segment_message, batch.frame_message):
        with pytest.raises((TypeError, ValueError), match="uint8|HIP device"):
            fn(torch.zeros(4, dtype=torch.int32), 1)


def test_reference_frames_are_reproduced_by_the_restatement():
    cases = golden_cases()
    assert len(cases) == 300
    assert {c["chunk"] for c in cases} == {1, 2, 3, 5, 16, 300} and {c["isn"] for c in cases} == {3611, 65530}
    texts = {c["message"] for c in cases}
    assert {"", "a", "é", "😀"} <= texts and len(texts) == 25
    for c in cases:
        raw = c["message"].encode()
        seg = segment_ref(raw, c["chunk"], c["isn"])
        assert seg.status == 0 and seg.characters == len(c["message"])
        assert seg.packets == len(c["frames"]) == max(1, -(-len(c["message"]) // c["chunk"]))
        assert frames_rudp5(raw, seg) == c["frames"], (c["message"], c["chunk"], c["isn"])


def test_restatement_edge_rules():
    s = segment_ref(bytes([0x80, 0x80, 0x61, 0x80, 0x62]), 1, 7)
    assert (s.packets, s.characters, s.payload_off.tolist()) == (2, 2, [0, 4, 5])
    s = segment_ref(bytes([0x80] * 5), 3, 7)
    assert (s.packets, s.characters, s.flags.tolist(), s.len.tolist()) == (1, 0, [0xA0], [5])
    s = segment_ref(bytes([0x80] * 70000), 1, 7)
    assert (s.packets, s.characters, s.status) == (1, 0, 1)
    s = segment_ref(b"abcde", 2, 70000, max_packets=2)
    assert s.status == 32 and s.seq.tolist() == [70000 & 0xFFFF, (70002) & 0xFFFF, 70004 & 0xFFFF]
