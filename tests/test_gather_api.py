"""rudp_gather_payloads (ABI 8) at the boundary: the symbol, its constants and
the argument checks that run before any device call.  CPU-only."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from rudp import _native, batch


def test_abi_8_exports_the_gather():
    lib = _native.lib()
    assert lib.rudp_abi_version() == 8 == _native.ABI_VERSION
    assert hasattr(lib, "rudp_gather_payloads")
    assert "rudp_gather_payloads" in _native.EXPORTS
    assert _native.ST_PAYLOAD_CAP == 16
    assert any(bit == _native.ST_PAYLOAD_CAP for bit, _ in batch._ST_MESSAGES)


def test_header_binding_and_library_agree_on_the_symbol():
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^RUDP_API int rudp_gather_payloads\(", text, flags=re.M)
    assert re.search(r"#define RUDP_ST_PAYLOAD_CAP 16u", text)
    assert re.search(r"#define RUDP_ABI_VERSION 8\b", text)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == "rudp_gather_payloads" and ln.split()[1] == "T" for ln in out.splitlines()), path


def _call(lib, frames, frames_bytes, off, n, keep, out, cap, poff, status, layout):
    return lib.rudp_gather_payloads(frames, frames_bytes, off, 8, n, keep, out, cap, poff, status, layout, 0, None)


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 2)(0, 0)
    p = ctypes.cast(word, ctypes.c_void_p)
    # bad layout, whatever else is passed
    assert _call(lib, p, 8, p, 1, None, p, 8, p, p, 6) == _native.EINVAL
    assert b"layout" in lib.rudp_last_error()
    # the status word is required
    assert _call(lib, p, 8, p, 1, None, p, 8, p, None, 7) == _native.EINVAL
    assert b"d_status" in lib.rudp_last_error()
    # both offset arrays
    assert _call(lib, p, 8, None, 1, None, p, 8, p, p, 7) == _native.EINVAL
    assert b"d_frame_off" in lib.rudp_last_error()
    assert _call(lib, p, 8, p, 1, None, p, 8, None, p, 5) == _native.EINVAL
    assert b"d_payload_off" in lib.rudp_last_error()
    # frames missing for a non-empty buffer
    assert _call(lib, None, 8, p, 1, None, p, 8, p, p, 7) == _native.EINVAL
    assert b"d_frames" in lib.rudp_last_error()
    # an empty batch is a successful no-op: nothing is touched, no device needed
    word[0] = word[1] = 0x5A5A5A5A5A5A5A5A
    assert _call(lib, None, 0, None, 0, None, None, 0, None, None, 7) == 0
    assert _call(lib, p, 8, p, 0, None, p, 8, p, p, 5) == 0
    assert word[0] == word[1] == 0x5A5A5A5A5A5A5A5A
    # the zero-copy rule of the variable-length decode still holds
    off = (ctypes.c_uint64 * 1)(0)
    offp = ctypes.cast(off, ctypes.c_void_p)
    assert lib.rudp_decode(None, offp, 10, 1, None, None, None, None, None, None, offp, 7, 0,
                           None) == _native.ENOTSUP


def test_python_validation():
    frames = np.zeros(16, np.uint8)
    off = np.array([0, 8, 16], np.int64)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.gather_payloads(frames, off, "rudp7")
    with pytest.raises(ValueError, match="layout"):
        batch.gather_payloads(frames, off, "rudp6")
    import torch
    with pytest.raises(ValueError, match="HIP device"):
        batch.gather_payloads(torch.from_numpy(frames), torch.from_numpy(off), 5)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.gather_payloads(torch.from_numpy(frames), off, 5)
