"""rudp_receive_window (added within ABI 8) at the boundary: the symbol and its
struct, the argument checks that run before any device call,
batch.receive_windowed's Python validation, the Python constants against
receive_window.hip, and the CPU reference on the reference's own traces.
CPU-only."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from accept_ref import golden_cases, pack_frames
from conftest import REPO
from receive_window_ref import receive_window_ref, reply_frames_ref
from rudp import _native, batch
from window_ref import NONE, chunk_model

FIELDS = ("seq", "ack", "flags", "ok", "csum_out", "valid", "usable", "chars", "accept", "rank", "carry_rank", "reply",
          "reply_ack", "state_out", "payload", "payload_cap", "payload_off", "payload_src", "carry_frames", "carry_cap",
          "carry_off", "carry_csum", "reply_frames", "reply_csum", "reply_index", "reply_peer", "info", "status")
CAPS = ("payload_cap", "carry_cap")


def test_symbol_header_and_struct():
    lib = _native.lib()
    text = (REPO / "include" / "rudp.h").read_text()
    assert re.search(r"^#define RUDP_HAS_RECEIVE_WINDOW 1\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ABI_VERSION 8\b", text, flags=re.M)
    assert re.search(r"^#define RUDP_ST_CARRY_CAP 128u", text, flags=re.M) and _native.ST_CARRY_CAP == 128
    assert hasattr(lib, "rudp_receive_window") and "rudp_receive_window" in _native.EXPORTS
    assert re.search(r"^RUDP_API int rudp_receive_window\(", text, flags=re.M)
    for path in (_native.LIB_PATH, _native.TOOLS_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True,
                             check=True).stdout
        assert any(ln.split()[-1] == "rudp_receive_window" and ln.split()[1] == "T" for ln in out.splitlines()), path
    # struct rudp_received_window: the header's members in the binding's order, 8 bytes each
    body = re.search(r"typedef struct rudp_received_window \{(.*?)\} rudp_received_window;", text, flags=re.S).group(1)
    members = [m.replace("_or_null", "") for m in re.findall(r"(\w+);", body)]
    assert members == list(FIELDS) == [f[0] for f in _native.RudpReceivedWindow._fields_]
    assert ctypes.sizeof(_native.RudpReceivedWindow) == 8 * len(FIELDS)
    for name in FIELDS:
        assert getattr(_native.RudpReceivedWindow, name).offset == 8 * FIELDS.index(name), name
    # the prototype's arguments, in the binding's order
    proto = re.search(r"RUDP_API int rudp_receive_window\((.*?)\);", text, flags=re.S).group(1)
    names = [re.findall(r"\w+", a)[-1] for a in proto.split(",")]
    assert names == ["d_carried", "carried_bytes", "d_carried_off", "d_carried_csum_or_null", "n_carried", "d_frames",
                     "frames_bytes", "d_frame_off", "d_csum_in_or_null", "n_new", "len_hint", "last_isn",
                     "window_chars", "d_state_in", "out", "layout", "device", "hip_stream"]
    assert len(lib.rudp_receive_window.argtypes) == len(names)


def _call(lib, word, *, carried="p", cbytes=8, coff="p", ccsum=None, nc=1, frames="p", nbytes=8, off="p", csum=None,
          nn=1, wc=8, st_in="p", layout=5, out="o", **null):
    p = ctypes.cast(word, ctypes.c_void_p)
    o = _native.RudpReceivedWindow(**{f: (8 if f in CAPS else p.value) for f in FIELDS})
    for name in null:
        setattr(o, name, None)
    pick = lambda v: p if v == "p" else v
    return lib.rudp_receive_window(pick(carried), cbytes, pick(coff), pick(ccsum), nc, pick(frames), nbytes, pick(off),
                                   pick(csum), nn, 0, 0xFFFFFFFF, wc, pick(st_in),
                                   ctypes.byref(o) if out == "o" else None, layout, 0, None)


def test_argument_errors_before_device():
    lib = _native.lib()
    word = (ctypes.c_uint64 * 8)(*([0x5A5A5A5A5A5A5A5A] * 8))
    err = lib.rudp_last_error
    assert _call(lib, word, out=None) == _native.EINVAL and b"out is NULL" in err()
    assert _call(lib, word, layout=6) == _native.EINVAL and b"layout" in err()
    # the sidebands: none with layout 7, both or none with carried frames
    assert _call(lib, word, layout=7, csum="p", ccsum="p") == _native.EINVAL and b"layout 7" in err()
    assert _call(lib, word, layout=7, ccsum="p", nc=0) == _native.EINVAL and b"layout 7" in err()
    assert _call(lib, word, csum="p") == _native.EINVAL and b"both" in err()
    assert _call(lib, word, ccsum="p") == _native.EINVAL and b"both" in err()
    for wc in (0, 1025):
        assert _call(lib, word, wc=wc) == _native.EINVAL and b"window_chars" in err()
    assert _call(lib, word, nc=1024) == _native.EINVAL and b"n_carried" in err()
    assert _call(lib, word, nc=1023, nn=(1 << 32) - 1024) == _native.EINVAL and b"2^32" in err()
    for nc, nn in ((0, 0), (1, 1), (0, 1), (1, 0)):  # required whatever the batch size
        assert _call(lib, word, nc=nc, nn=nn, st_in=None) == _native.EINVAL and b"d_state_in" in err()
        for field in ("state_out", "info", "status"):
            assert _call(lib, word, nc=nc, nn=nn, **{field: None}) == _native.EINVAL
            assert field.encode() + b" is NULL" in err(), field
    for field in ("seq", "ack", "flags", "ok", "valid", "usable", "chars", "accept", "rank", "carry_rank", "reply",
                  "reply_ack", "payload_off", "carry_off", "reply_frames", "reply_index", "reply_peer", "payload",
                  "carry_frames"):
        for nc, nn in ((1, 1), (0, 1)) + (((1, 0),) if not field.startswith("reply_") or field == "reply_ack" else ()):
            assert _call(lib, word, nc=nc, nn=nn, **{field: None}) == _native.EINVAL, (field, nc, nn)
            assert b"rudp_receive_window: " + field.encode() + b" is NULL" in err(), field
    assert _call(lib, word, off=None) == _native.EINVAL and b"d_frame_off" in err()
    assert _call(lib, word, coff=None) == _native.EINVAL and b"d_carried_off" in err()
    assert _call(lib, word, frames=None) == _native.EINVAL and b"d_frames" in err()
    assert _call(lib, word, carried=None) == _native.EINVAL and b"d_carried is NULL" in err()
    assert list(word) == [0x5A5A5A5A5A5A5A5A] * 8  # nothing was touched


def test_python_validation():
    import torch
    from rudp.transport import ReliableUDP
    cpu8 = torch.zeros(4, dtype=torch.uint8)
    off = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="torch tensors"):
        batch.receive_windowed(np.zeros(4, np.uint8), off, "rudp5", window_chars=8)
    with pytest.raises(ValueError, match="layout"):
        batch.receive_windowed(cpu8, off, "rudp6", window_chars=8)
    for bad in (0, 1025, True, 2.0, None):
        with pytest.raises(ValueError, match="window_chars"):
            batch.receive_windowed(cpu8, off, "rudp5", window_chars=bad)
    for bad in (3, "carried", batch.CarriedFrames(None)):  # (receive_window's own carry is another type)
        with pytest.raises(TypeError, match="carried must be"):
            batch.receive_windowed(cpu8, off, "rudp5", window_chars=8, carried=bad)
    with pytest.raises(TypeError, match="out must be"):
        batch.receive_windowed(cpu8, off, "rudp5", window_chars=8, out=cpu8)
    with pytest.raises(ValueError, match="HIP device"):
        batch.receive_windowed(cpu8, off, "rudp5", window_chars=8)
    for bad in (-1, True, 1.5, "7"):
        with pytest.raises(ValueError, match="last_isn"):
            batch.receive_windowed(cpu8, off, "rudp5", window_chars=8, last_isn=bad)
    with pytest.raises(ValueError, match="reorder_fused.*reorder_window"):
        ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_fused=True)
    assert ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_window=8)._reorder_fused is False
    assert ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_window=8, reorder_fused=True)._reorder_fused


def test_result_layout():
    """Every array of the one allocation aligned to its element, none overlapping."""
    width = {"payload_off": 8, "carry_off": 8, "reply_peer": 8, "state": 8, "info": 8, "status": 4, "rank": 4,
             "carry_rank": 4, "chars": 4, "payload_src": 4, "reply_index": 4, "seq": 2, "ack": 2, "csum": 2,
             "reply_ack": 2, "reply_csum": 2, "carry_csum": 2, "flags": 1, "ok": 1, "valid": 1, "usable": 1,
             "accept": 1, "reply": 1, "reply_frames": 1, "payload": 16, "carry": 16}
    per_new = ("reply_peer", "reply_index", "reply_csum")
    for nc, nn in ((0, 0), (0, 1), (1, 0), (1, 2), (3, 4), (1023, 1024), (7, 1025)):
        for H in (5, 7):
            n, cap = nc + nn, 6 * (nc + nn) + 1
            lay = batch.ReceivedWindowed.layout(n, nn, H, cap, cap)
            assert set(lay) == set(width) | {"size"}
            at = [(lay[k], k) for k in lay if k != "size"]  # (in layout order: empty arrays share an offset)
            assert at == sorted(at, key=lambda e: e[0]) and all(lo % width[k] == 0 for lo, k in at), (nc, nn, H)
            size = {"payload_off": 8 * (n + 1), "carry_off": 8 * 1024, "state": 32, "info": 96, "status": 4,
                    "carry_csum": 2 * 1023, "reply_frames": nn * H, "payload": cap, "carry": cap}
            size.update({k: width[k] * nn for k in per_new})
            for (lo, k), (nxt, _) in zip(at, at[1:] + [(lay["size"], "")]):
                assert lo + size.get(k, width[k] * n) <= nxt, (nc, nn, H, k)


def test_python_geometry_matches_the_kernel_source():
    """batch.WINDOW_FUSED_BYTES / WINDOW_FUSED_MEAN restate receive_window.hip's
    choice of form (the GPU tests put their edge cases there)."""
    csrc = REPO / "reliable-udp_amd" / "csrc"
    hip = (csrc / "receive_window.hip").read_text()
    win = (csrc / "window.hip").read_text() + (csrc / "window_device.hpp").read_text()
    assert int(re.search(r"constexpr uint32_t kRwFusedBytes = (\d+);", hip).group(1)) == batch.WINDOW_FUSED_BYTES
    assert int(re.search(r"constexpr uint32_t kRwFusedMeanFrame = (\d+);", hip).group(1)) == batch.WINDOW_FUSED_MEAN
    assert int(re.search(r"constexpr uint32_t kWinNew = (\d+);", win).group(1)) == batch.WINDOW_CHUNK
    assert "constexpr uint32_t kRwCarryMax = kWinNew - 1u;" in hip and batch.WINDOW_CARRY_MAX == batch.WINDOW_CHUNK - 1
    assert ("return knob && n_new <= kWinNew && n_carried <= kRwCarryMax && total_bytes <= kRwFusedBytes &&\n"
            "         (knob == 2 || total_bytes <= (uint64_t)kRwFusedMeanFrame * n);") in hip
    # the fused form's LDS is held to a gfx950 workgroup's 160 KiB where it is declared
    assert "static_assert(sizeof(RwLds) <= 160 * 1024" in hip
    # both kernels judge a chunk with the one device function
    assert win.count("win_judge_chunk(") == 2 and "win_judge_chunk(a.w, S.win);" in hip
    # knob 82 of the diagnostics build chooses the form
    assert "key == 82 ? &t.receive_window_fused" in (csrc / "tuning.hip").read_text()
    assert "RUDP_KNOB(receive_window_fused, 1)" in (csrc / "internal.hpp").read_text()


def test_reference_on_the_golden_traces_at_a_window_of_one():
    """The reference's own traces: at window_chars = 1 the call is rudp_receive
    (accepted, replied, acks, end, message, state), by either statement of the rule."""
    for c in golden_cases():
        frames = [bytes.fromhex(h) for h in c["frames"]]
        buf, off = pack_frames(frames)
        for rule in (None, chunk_model):
            kw = {} if rule is None else {"rule": rule}
            r = receive_window_ref(np.zeros(0, np.uint8), None, buf, off, 5, window_chars=1, state=tuple(c["state"]),
                                   last_isn=c["last_isn"], **kw)
            name = c["name"]
            assert "".join(str(int(v == 1)) for v in r["accept"]) == c["accepted"], name
            ms = r["info"][2] if r["info"][2] < len(frames) else 0  # (frames before the last reset lose their rank)
            ranked = [int(v == "1" and i >= ms) for i, v in enumerate(c["accepted"])]
            assert [int(v != NONE) for v in r["rank"]] == ranked, name
            assert "".join(str(int(v)) for v in r["reply"]) == c["replied"], name
            assert r["reply_ack"].tolist() == c["ack"], name
            assert r["info"][0] == c["end"] and r["info"][5] == 0 and r["info"][10] == 0, name
            assert r["payload"].tobytes().decode() == c["message"] and r["info"][9] == len(r["payload"]), name
            assert r["state"] == c["state_after"] + [0], name
            assert r["status"] == 0 and r["R"] == c["replied"].count("1") == r["info"][8], name
            assert r["reply_index"].tolist() == [i for i, v in enumerate(c["replied"]) if v == "1"], name
            want, _ = reply_frames_ref(np.array([a for a, v in zip(c["ack"], c["replied"]) if v == "1"], np.uint16), 5)
            assert np.array_equal(r["reply_frames"], want), name


def test_reference_rejects_per_source():
    """An offset past its own buffer rejects the item even where the other
    buffer is long enough, at the seam between the sources included."""
    f = [bytes([0, 10 + k, 0, 0, 0x80 if k == 0 else 0]) + b"ab"[k % 2:k % 2 + 1] for k in range(4)]
    cbuf, coff = pack_frames(f[:2])
    nbuf, noff = pack_frames(f[2:])
    long_new = np.concatenate([nbuf, np.zeros(40, np.uint8)])
    for which, k in (("carried", 1), ("carried", 2), ("new", 0), ("new", 2)):
        co, no = coff.copy(), noff.copy()
        (co if which == "carried" else no)[k] += 20
        r = receive_window_ref(cbuf, co, long_new if which == "carried" else nbuf, no, 5, window_chars=8)
        base = 0 if which == "carried" else 2
        bad = sorted({base + j for j in (k - 1, k) if 0 <= j < 2})
        assert np.flatnonzero(r["ok"] == 4).tolist() == bad and r["status"] & 8, (which, k)
        assert not r["usable"][bad].any() and (r["rank"][bad] == NONE).all() and (r["carry_rank"][bad] == NONE).all()
