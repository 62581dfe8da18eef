"""rudp_receive (added within ABI 8) at the boundary: the symbol and its struct,
the argument checks that run before any device call, batch.receive's Python
validation, and the Python constants against receive.hip.  CPU-only."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from rudp import _native, batch

FIELDS = ("seq", "ack", "flags", "ok", "csum_out", "valid", "usable", "chars", "accept", "keep", "reply", "reply_ack",
          "state_out", "payload", "payload_cap", "payload_off", "reply_frames", "reply_csum", "reply_index",
          "reply_peer", "info", "status")


def test_symbol_header_and_struct():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^#define RUDP_HAS_RECEIVE 1\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    assert hasattr(lib, "rudp_receive") and "rudp_receive" in _native.EXPORTS
    assert re.search(r"^RUDP_API int rudp_receive\(", text, flags=re.M)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == "rudp_receive" and ln.split()[1] == "T" for ln in out.splitlines()), path
    # struct rudp_received: the header's members in the binding's order, 8 bytes each
    body = re.search(r"typedef struct rudp_received \{(.*?)\} rudp_received;", text, flags=re.S).group(1)
    members = [m.replace("_or_null", "") for m in re.findall(r"(\w+);", body)]
    assert members == list(FIELDS) == [f[0] for f in _native.RudpReceived._fields_]
    assert ctypes.sizeof(_native.RudpReceived) == 8 * len(FIELDS)
    assert _native.RudpReceived.payload_cap.offset == 8 * FIELDS.index("payload_cap")
    # the usable rule is stated where a C caller reads it
    assert "RUDP_OK_GOOD or RUDP_OK_UNVERIFIED" in text and "bad offsets" in text


def _call(lib, word, *, frames="p", nbytes=8, off="p", n=1, csum=None, st_in="p", layout=5, out="o", **null):
    p = ctypes.cast(word, ctypes.c_void_p)
    o = _native.RudpReceived(**{f: (8 if f == "payload_cap" else p.value) for f in FIELDS})
    for name in null:
        setattr(o, name, None)
    pick = lambda v: p if v == "p" else v
    return lib.rudp_receive(pick(frames), nbytes, pick(off), 0, n, pick(csum), 0xFFFFFFFF, pick(st_in),
                            ctypes.byref(o) if out == "o" else None, layout, 0, None)


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    err = lib.rudp_last_error
    assert _call(lib, word, out=None) == _native.EINVAL and b"out is NULL" in err()
    assert _call(lib, word, layout=6) == _native.EINVAL and b"layout" in err()
    assert _call(lib, word, layout=7, csum="p") == _native.EINVAL and b"d_csum_in" in err()
    for n in (0, 1):  # required whatever the batch size
        assert _call(lib, word, n=n, st_in=None) == _native.EINVAL and b"d_state_in" in err()
        for field in ("state_out", "info", "status"):
            assert _call(lib, word, n=n, **{field: None}) == _native.EINVAL
            assert field.encode() + b" is NULL" in err(), field
    assert _call(lib, word, n=1 << 32) == _native.EINVAL and b"2^32" in err()
    assert _call(lib, word, off=None) == _native.EINVAL and b"d_frame_off" in err()
    assert _call(lib, word, frames=None) == _native.EINVAL and b"d_frames" in err()
    for field in ("seq", "ack", "flags", "ok", "valid", "usable", "chars", "accept", "keep", "reply", "reply_ack",
                  "payload_off", "reply_frames", "reply_index", "reply_peer", "payload"):
        assert _call(lib, word, **{field: None}) == _native.EINVAL
        assert b"rudp_receive: " + field.encode() + b" is NULL" in err(), field
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    cpu8 = torch.zeros(4, dtype=torch.uint8)
    off = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive(np.zeros(4, np.uint8), off, "rudp5")
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive(cpu8, np.zeros(2, np.int64), "rudp5")
    with pytest.raises(ValueError, match="layout"):
        batch.receive(cpu8, off, "rudp6")
    with pytest.raises(ValueError, match="HIP device"):
        batch.receive(cpu8, off, "rudp5")
    for bad in (-1, True, 1.5, "7"):
        with pytest.raises(ValueError, match="last_isn"):
            batch.receive(cpu8, off, "rudp5", last_isn=bad)


def test_result_layout():
    """Every array of the one allocation aligned to its element, none overlapping."""
    width = {"payload_off": 8, "reply_peer": 8, "accepted": 8, "chars": 4, "reply_index": 4, "seq": 2, "ack": 2,
             "csum": 2, "reply_csum": 2, "flags": 1, "ok": 1, "valid": 1, "usable": 1, "reply_frames": 1,
             "payload": 16}
    for n in (0, 1, 2, 3, 1023, 1024, 1025):
        for H in (5, 7):
            lay = batch.Received.layout(n, H, 6 * n)
            assert set(lay) == set(width) | {"size"}
            at = [(lay[k], k) for k in lay if k != "size"]  # (in layout order: empty arrays share an offset)
            assert at == sorted(at, key=lambda e: e[0]) and all(lo % width[k] == 0 for lo, k in at), (n, H)
            size = {"payload_off": 8 * (n + 1) + 8, "reply_peer": 8 * n, "accepted": batch.Accepted.layout(n)[6] + 16,
                    "chars": 4 * n, "reply_index": 4 * n, "reply_frames": n * H, "payload": 6 * n}
            for (lo, k), (nxt, _) in zip(at, at[1:] + [(lay["size"], "")]):
                assert lo + size.get(k, width[k] * n) <= nxt, (n, H, k)


def test_python_geometry_matches_the_kernel_source():
    """batch.RECV_FUSED_BYTES / RECV_TILE restate receive.hip's choice of form (the
    GPU tests put their edge cases there)."""
    csrc = REPO / "reliable-udp_amd" / "csrc"
    hip = (csrc / "receive.hip").read_text()
    assert int(re.search(r"constexpr uint32_t kRecvFusedBytes = (\d+);", hip).group(1)) == batch.RECV_FUSED_BYTES
    assert int(re.search(r"constexpr uint32_t kRecvFusedMeanFrame = (\d+);", hip).group(1)) == batch.RECV_FUSED_MEAN
    assert ("return knob && n <= kAccTile && frames_bytes <= kRecvFusedBytes &&\n"
            "         (knob == 2 || frames_bytes <= (uint64_t)kRecvFusedMeanFrame * n);") in hip
    assert batch.RECV_TILE == batch.ACCEPT_TILE  # (test_accept_api.py holds that one to accept.hip's kAccTile)
    # the fused form's LDS stays within what a workgroup gets without asking
    acc = (csrc / "accept_device.hpp").read_text()
    assert "uint64_t pk[kAccTile];" in acc and "uint32_t img[(kRecvFusedBytes + 16u + 32u) / 4u];" in hip
    T = batch.RECV_TILE
    lds = (4 + 2 + 2 + 4 + 8) * T + 256 + 2 * 4 * (T + 1) + 64 + batch.RECV_FUSED_BYTES + 48
    assert lds <= 65536
    # knob 80 of the diagnostics build turns the fused form off
    tune = (csrc / "tuning.hip").read_text()
    assert "key == 80 ? &t.receive_fused" in tune
