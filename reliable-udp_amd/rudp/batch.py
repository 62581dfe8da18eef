"""Batched encode / decode of Reliable-UDP frames on MI355X.

The reference frames one packet per Python call (utils/reliableUDP.py:53-61
encode, :118-123 decode, through utils/packet.py).  Here a whole batch is
framed, checksummed, parsed and verified by HIP kernels in librudp.so:

    frames, csum = pack_batch(headers, payloads, layout="rudp5")
    dec = unpack_batch(frames, layout="rudp5", csum=csum)

Inputs are either torch tensors on a HIP device (asynchronous, on the current
stream; the device-resident path the benchmark measures) or numpy arrays in
host memory (synchronous; staged through the GPU by rudp_encode_host /
rudp_decode_host, the model of the reference's socket-buffer boundary).
Nothing here computes on the CPU: without librudp.so or a HIP device the
calls raise.

Layouts:
  "rudp5"  the reference's 5-byte header (utils/packet.py:3-10) byte for
           byte; the RFC 1071 checksum comes back as a sideband u16 array.
  "rudp7"  {**custom_header, "checksum": 2}: the checksum in-band at bytes
           5-6, framed exactly as utils/packet.py frames that definition.
"""
from __future__ import annotations

import contextlib
import ctypes
import threading
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional, Tuple, Union

import numpy as np

from . import _native

LAYOUTS = {"rudp5": 5, "rudp7": 7, 5: 5, 7: 7}

# header byte 4 (utils/packet.py:6-9): SYN 0x80, ACK 0x40, FIN 0x20, offset 0x1F
SYN, ACK, FIN, OFFSET_MASK = 0x80, 0x40, 0x20, 0x1F


def layout_header_len(layout: Union[str, int]) -> int:
    try:
        return LAYOUTS[layout]
    except (KeyError, TypeError):
        raise ValueError(f"unknown layout {layout!r}: use 'rudp5' or 'rudp7'") from None


def make_flags(syn=0, ack=0, fin=0, offset=0):
    """Header byte 4 from the four custom_header bit fields (utils/packet.py:6-9)."""
    return (syn & 1) << 7 | (ack & 1) << 6 | (fin & 1) << 5 | (offset & OFFSET_MASK)


@dataclass
class HeaderTable:
    """SoA header table: seq_num u16[N], ack_num u16[N], flags u8[N]."""
    seq: Any
    ack: Any
    flags: Any

    def __len__(self) -> int:
        return len(self.seq)


class PayloadSpans:
    """Payload i of a packed batch is frames[start[i]:end[i]] (zero-copy).

    Behaves as the pair ``(start, end)`` of int64 [N] tensors; ``start``
    (= min(frame_off[i] + H, frame_off[i + 1]), two device ops) is computed on
    first use, so a decode whose caller reads only the header fields does
    not pay for it.
    """

    __slots__ = ("_frame_off", "_H", "_start")

    def __init__(self, frame_off, H: int):
        self._frame_off = frame_off
        self._H = H
        self._start = None

    @property
    def start(self):
        if self._start is None:
            if isinstance(self._frame_off, np.ndarray):  # a host-memory decode's offsets
                self._start = np.minimum(self._frame_off[:-1] + self._H, self._frame_off[1:])
            else:
                import torch
                self._start = torch.minimum(self._frame_off[:-1] + self._H, self._frame_off[1:])
        return self._start

    @property
    def end(self):
        return self._frame_off[1:]

    def __iter__(self):
        return iter((self.start, self.end))

    def __getitem__(self, i):
        return (self.start, self.end)[i]

    def __len__(self):
        return 2


_ST_MESSAGES = (
    (_native.ST_LEN, "lengths must lie in [0, 65535]"),
    (_native.ST_PAYLOAD, "packed payloads: sum(lengths) must equal payload.numel(); "
                         "gathered payloads: payload_off + lengths must stay inside payload"),
    (_native.ST_FRAMES_CAP, "out is too small for the frames (sum(lengths) + N * header bytes)"),
    (_native.ST_OFFSETS, "frame_off must be non-decreasing offsets inside frames"),
    (_native.ST_PAYLOAD_CAP, "out is too small for the kept payloads"),
    (_native.ST_PACKETS_CAP, "the message makes more packets than max_packets"),
    (_native.ST_FLOW, "a flow slot is neither below the states table's rows nor FLOW_NONE"),
)


def _raise_status(status) -> None:
    """Read a sync-free call's device status word (synchronizes) and raise
    ValueError with the reason when the device found the batch invalid."""
    if status is None:
        return
    bits = int(status.item())
    if bits:
        raise ValueError("; ".join(m for b, m in _ST_MESSAGES if bits & b) or f"status {bits:#x}")


class DecodedBatch(NamedTuple):
    seq: Any
    ack: Any
    flags: Any
    ok: Any          # 1 good, 0 bad checksum, 2 short frame, 3 unverified (rudp5, no csum)
    csum: Any        # recomputed checksum per packet
    payload: Any     # [N, L] view into frames (zero-copy) or a copy
    status: Any = None  # sync-free varlen decode: device u32[1], RUDP_ST_* (0 = valid)
    valid: Any = None   # utf8=True: u8 [N], 1 where get_payload() would return, 0 where it raises

    def check(self) -> "DecodedBatch":
        """Raise ValueError if the device rejected the batch (reads ``status``:
        one synchronization).  A no-op for calls that checked eagerly."""
        _raise_status(self.status)
        return self


def _is_torch(x) -> bool:
    try:
        import torch
    except ImportError:  # pragma: no cover
        return False
    return isinstance(x, torch.Tensor)


_PIN_DT = {np.uint8: "uint8", np.uint16: "uint16", np.int64: "int64"}


def _pinned_out(n: int, dtype) -> np.ndarray:
    """A per-packet output array of a *_host call: page-locked, from torch's
    caching host allocator (a repeated call of the same size reuses the block),
    so the pipeline's D2H lands at the link's rate instead of faulting fresh
    pageable pages in.  Only the small per-packet arrays come from here; frames
    and payloads are the caller's or plain numpy."""
    import torch
    return torch.empty((n,), dtype=getattr(torch, _PIN_DT[dtype]), pin_memory=True).numpy()


def _as_table(headers) -> HeaderTable:
    if isinstance(headers, HeaderTable):
        return headers
    if isinstance(headers, dict):
        return HeaderTable(headers["seq_num"], headers["ack_num"], headers["flags"])
    seq, ack, flags = headers
    return HeaderTable(seq, ack, flags)


# ---------------------------------------------------------------- device path
def _dev_check(t, name, dtype, ndim, device):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor on the same device")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _stream_ptr(stream, device) -> int:
    import torch
    if stream is not None:
        return int(stream.cuda_stream)
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # no Stream object per call
    if raw is not None:
        return int(raw(device.index if device.index is not None else torch.cuda.current_device()))
    return int(torch.cuda.current_stream(device).cuda_stream)


def _pack_device(tab: HeaderTable, payloads, H: int, out, csum_out, want_csum, stream):
    import torch
    dev = payloads.device
    if dev.type != "cuda":
        raise ValueError("device path needs tensors on a HIP device")
    _dev_check(payloads, "payloads", torch.uint8, 2, dev)
    n, L = payloads.shape
    for name, t, dt in (("seq", tab.seq, torch.uint16), ("ack", tab.ack, torch.uint16),
                        ("flags", tab.flags, torch.uint8)):
        _dev_check(t, name, dt, 1, dev)
        if t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} entries for {n} payloads")
    F = L + H
    if out is None:
        out = torch.empty((n, F), dtype=torch.uint8, device=dev)
    else:
        _dev_check(out, "out", torch.uint8, 2, dev)
        if tuple(out.shape) != (n, F):
            raise ValueError(f"out must have shape {(n, F)}, got {tuple(out.shape)}")
    if csum_out is None and want_csum:
        csum_out = torch.empty((n,), dtype=torch.uint16, device=dev)
    elif csum_out is not None:
        _dev_check(csum_out, "csum_out", torch.uint16, 1, dev)
    b = _native.RudpBatch(n=n, payload_len=L, reserved=0, seq=tab.seq.data_ptr(),
                          ack=tab.ack.data_ptr(), flags=tab.flags.data_ptr(),
                          payload=payloads.data_ptr() if n * L else None, len=None,
                          payload_off=None)
    _native.check(_native.lib().rudp_encode(
        ctypes.byref(b), out.data_ptr() if n else None,
        csum_out.data_ptr() if (csum_out is not None and n) else None,
        H, dev.index if dev.index is not None else torch.cuda.current_device(),
        _stream_ptr(stream, dev)))
    return out, csum_out


def _unpack_device(frames, H: int, csum, copy_payload: bool, stream, utf8: bool = False):
    import torch
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("device path needs tensors on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 2, dev)
    n, F = frames.shape
    L = max(F - H, 0)
    seq = torch.empty((n,), dtype=torch.uint16, device=dev)
    ack = torch.empty((n,), dtype=torch.uint16, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    cs = torch.empty((n,), dtype=torch.uint16, device=dev)
    if csum is not None:
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    pay = torch.empty((n, L), dtype=torch.uint8, device=dev) if copy_payload else None
    valid = torch.empty((n,), dtype=torch.uint8, device=dev) if utf8 else None
    if n:
        _native.check(_native.lib().rudp_decode_utf8(
            frames.data_ptr() if F else None, None, F, n, csum.data_ptr() if csum is not None else None,
            seq.data_ptr(), ack.data_ptr(), flags.data_ptr(), ok.data_ptr(), cs.data_ptr(),
            pay.data_ptr() if (pay is not None and L) else None,
            valid.data_ptr() if valid is not None else None, H,
            dev.index if dev.index is not None else torch.cuda.current_device(),
            _stream_ptr(stream, dev)))
    if pay is None:
        pay = frames[:, H:] if F >= H else frames[:, :0]
    return DecodedBatch(seq, ack, flags, ok, cs, pay, None, valid)


# ------------------------------------------------------------------ host path
def _host_arr(a, name, dtype, ndim):
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        raise TypeError(f"{name} must be {np.dtype(dtype)}, got {a.dtype}")
    if a.ndim != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {a.shape}")
    return a


def _ptr(a) -> Optional[int]:
    return a.ctypes.data if a.size else None


def _host_out(a, name, dtype, shape):
    if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape \
            or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
        raise ValueError(f"{name} must be a writeable C-contiguous {np.dtype(dtype)} array of shape {shape}")
    return a


def _pack_host(tab: HeaderTable, payloads, H, want_csum, device, out=None, csum_out=None):
    payloads = _host_arr(payloads, "payloads", np.uint8, 2)
    n, L = payloads.shape
    seq = _host_arr(tab.seq, "seq", np.uint16, 1)
    ack = _host_arr(tab.ack, "ack", np.uint16, 1)
    flags = _host_arr(tab.flags, "flags", np.uint8, 1)
    for name, a in (("seq", seq), ("ack", ack), ("flags", flags)):
        if a.shape[0] != n:
            raise ValueError(f"{name} has {a.shape[0]} entries for {n} payloads")
    frames = (_host_out(out, "out", np.uint8, (n, L + H)) if out is not None
              else np.empty((n, L + H), dtype=np.uint8))
    if csum_out is not None:
        csum = _host_out(csum_out, "csum_out", np.uint16, (n,))
    else:
        csum = _pinned_out(n, np.uint16) if want_csum else None
    b = _native.RudpBatch(n=n, payload_len=L, reserved=0, seq=_ptr(seq), ack=_ptr(ack),
                          flags=_ptr(flags), payload=_ptr(payloads), len=None, payload_off=None)
    _native.check(_native.lib().rudp_encode_host(
        ctypes.byref(b), _ptr(frames), _ptr(csum) if csum is not None else None, H, device))
    return frames, csum


def _unpack_host(frames, H, csum, copy_payload, device, utf8=False):
    frames = _host_arr(frames, "frames", np.uint8, 2)
    n, F = frames.shape
    L = max(F - H, 0)
    seq = _pinned_out(n, np.uint16)
    ack = _pinned_out(n, np.uint16)
    flags = _pinned_out(n, np.uint8)
    ok = _pinned_out(n, np.uint8)
    cs = _pinned_out(n, np.uint16)
    if csum is not None:
        csum = _host_arr(csum, "csum", np.uint16, 1)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    pay = np.empty((n, L), np.uint8) if copy_payload else None
    valid = _pinned_out(n, np.uint8) if utf8 else None
    if n:
        _native.check(_native.lib().rudp_decode_host(
            _ptr(frames), F, n, _ptr(csum) if csum is not None else None, _ptr(seq), _ptr(ack),
            _ptr(flags), _ptr(ok), _ptr(cs), _ptr(pay) if pay is not None else None,
            _ptr(valid) if valid is not None else None, H, device))
    if pay is None:
        pay = frames[:, H:] if F >= H else frames[:, :0]
    return DecodedBatch(seq, ack, flags, ok, cs, pay, None, valid)


# ------------------------------------------------------------------ public API
def pack_batch(headers, payloads, layout: Union[str, int] = "rudp7", *, out=None,
               csum_out=None, want_csum: Optional[bool] = None, stream=None, device: int = 0
               ) -> Tuple[Any, Any]:
    """Frame + checksum a batch.  Returns ``(frames, csum)``.

    ``headers``: HeaderTable, ``(seq, ack, flags)`` or a dict keyed like
    custom_header (``seq_num``, ``ack_num``) plus ``flags``.  ``payloads``:
    uint8 ``[N, L]``.  ``csum`` is the per-packet checksum (always for rudp5,
    on request for rudp7; else None).  Torch tensors on a HIP device run
    asynchronously on ``stream`` (default: current stream); numpy arrays run
    synchronously through ``device``.
    """
    H = layout_header_len(layout)
    tab = _as_table(headers)
    if want_csum is None:
        want_csum = H == 5
    if _is_torch(payloads):
        return _pack_device(tab, payloads, H, out, csum_out, want_csum, stream)
    return _pack_host(tab, payloads, H, want_csum, device, out, csum_out)


def unpack_batch(frames, layout: Union[str, int] = "rudp7", *, csum=None,
                 copy_payload: bool = False, stream=None, device: int = 0, utf8: bool = False) -> DecodedBatch:
    """Parse + verify a batch of fixed-length frames ``[N, F]``.

    ``csum`` (rudp5 only): sideband checksums to verify against.  The payload
    is returned as a zero-copy view ``frames[:, H:]`` unless ``copy_payload``.
    ``utf8``: also ``valid``, u8 [N], 1 where Packet(frame).get_payload()
    would return and 0 where its strict UTF-8 decode would raise
    (utils/packet.py:68-73), judged in the same pass over the frames
    (rudp_decode_utf8; numpy frames: rudp_decode_host, staged through the GPU).
    """
    H = layout_header_len(layout)
    if H == 7 and csum is not None:
        raise ValueError("rudp7 carries its checksum in-band; csum= is for rudp5")
    if _is_torch(frames):
        return _unpack_device(frames, H, csum, copy_payload, stream, utf8)
    return _unpack_host(frames, H, csum, copy_payload, device, utf8)


def synth_batch(n: int, payload_len: int, seed: int, *, first_index: int = 0, ascii: bool = True,
                device=None, stream=None) -> Tuple[HeaderTable, Any]:
    """Generate the deterministic synthetic batch on a HIP device (rudp_synth)."""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    seq = torch.empty((n,), dtype=torch.uint16, device=dev)
    ack = torch.empty((n,), dtype=torch.uint16, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    pay = torch.empty((n, payload_len), dtype=torch.uint8, device=dev)
    if n:
        _native.check(_native.lib().rudp_synth(
            seed & (2**64 - 1), first_index, n, payload_len, 1 if ascii else 0, seq.data_ptr(),
            ack.data_ptr(), flags.data_ptr(), pay.data_ptr() if payload_len else None,
            dev.index if dev.index is not None else 0, _stream_ptr(stream, dev)))
    return HeaderTable(seq, ack, flags), pay


# ------------------------------------------------------- variable-length batches
class VarlenFrames:
    """Result of ``pack_batch_varlen``: ``frames`` (u8, frames back to back, or
    the caller's ``out``), ``frame_off`` (int64 [N + 1]: frame i =
    frames[frame_off[i]:frame_off[i + 1]]), ``csum`` (u16 [N] or None) and
    ``status`` (device int32 [1], RUDP_ST_* of the call, 0 = valid).

    All of them live in one device allocation and are cut out of it on first
    access, so a sync-free caller that only keeps the result pays for one
    allocation and the launch.  Iterates as (frames, frame_off, csum, status).
    """

    __slots__ = ("_buf", "_n", "_cs_bytes", "_f_at", "_frames", "_frame_off", "_csum", "_status")

    # one allocation: frame_off (i64 [n + 1]) | status (i32) | pad | csum (u16 [n]) |
    # pad to 16 B | frames (unless the caller's)
    def __init__(self, buf, n: int, cs_bytes: int, f_at: int, frames=None):
        self._buf, self._n, self._cs_bytes, self._f_at = buf, n, cs_bytes, f_at
        self._frames, self._frame_off, self._csum, self._status = frames, None, None, None

    @staticmethod
    def layout(n: int, want_csum: bool):
        """(bytes before the frames, csum bytes): the allocation's head."""
        cs_bytes = 2 * n if want_csum else 0
        head = 8 * (n + 1) + 8 + cs_bytes
        return head + (-head % 16), cs_bytes

    @property
    def frames(self):
        if self._frames is None:
            self._frames = self._buf[self._f_at:]
        return self._frames

    @property
    def frame_off(self):
        if self._frame_off is None:
            import torch
            self._frame_off = self._buf[:8 * (self._n + 1)].view(torch.int64)
        return self._frame_off

    @property
    def status(self):
        if self._status is None:
            import torch
            at = 8 * (self._n + 1)
            self._status = self._buf[at:at + 4].view(torch.int32)
        return self._status

    @property
    def csum(self):
        if self._csum is None and self._cs_bytes:
            import torch
            at = 8 * (self._n + 1) + 8
            self._csum = self._buf[at:at + self._cs_bytes].view(torch.uint16)
        return self._csum

    def __iter__(self):
        return iter((self.frames, self.frame_off, self.csum, self.status))

    def __getitem__(self, i):
        return tuple(self)[i]

    def __len__(self):
        return 4

    def check(self) -> "VarlenFrames":
        """Raise ValueError if the device rejected the batch (one synchronization)."""
        _raise_status(self.status)
        return self


class VarlenDecoded:
    """Result of ``unpack_batch_varlen``, with the fields of ``DecodedBatch``:
    seq, ack (u16 [N]), flags, ok (u8 [N]), csum (u16 [N]), payload
    (``PayloadSpans``), status and valid (u8 [N] with ``utf8=True``, else
    None).  The output arrays share one device allocation and are cut out of
    it on first access.  Iterates as (seq, ack, flags, ok, csum, payload,
    status)."""

    __slots__ = ("_buf", "_n", "payload", "_v", "_utf8", "_stream")

    def __init__(self, buf, n: int, payload, utf8: bool = False, stream=None):
        self._buf, self._n, self.payload, self._v, self._utf8 = buf, n, payload, {}, utf8
        self._stream = stream  # the stream the decode was enqueued on (None: the current one)

    # one allocation: seq | ack | csum (u16 [n] each) | flags | ok | valid (u8 [n] each)
    def _cut(self, name, at, nbytes, dtype):
        v = self._v.get(name)
        if v is None:
            v = self._buf[at:at + nbytes]
            if dtype is not None:
                v = v.view(dtype)
            self._v[name] = v
        return v

    @property
    def seq(self):
        import torch
        return self._cut("seq", 0, 2 * self._n, torch.uint16)

    @property
    def ack(self):
        import torch
        return self._cut("ack", 2 * self._n, 2 * self._n, torch.uint16)

    @property
    def csum(self):
        import torch
        return self._cut("csum", 4 * self._n, 2 * self._n, torch.uint16)

    @property
    def flags(self):
        return self._cut("flags", 6 * self._n, self._n, None)

    @property
    def ok(self):
        return self._cut("ok", 7 * self._n, self._n, None)

    @property
    def valid(self):
        return self._cut("valid", 8 * self._n, self._n, None) if self._utf8 else None

    @property
    def status(self):
        """Device int32 [1]: RUDP_ST_OFFSETS when a frame was rejected for bad
        offsets (ok == RUDP_OK_BAD_OFFSETS), else 0, as ``VarlenFrames.status``.
        The decode keeps no status word of its own (a call is its one kernel,
        rudp_decode_varlen_checked with d_status NULL), so this is built from
        ``ok`` on first access: one device reduction, no synchronization, on
        the stream the decode ran on (so it reads ``ok`` after the decode wrote
        it), with the caller's current stream then made to wait for it."""
        v = self._v.get("status")
        if v is None:
            import torch
            if self._stream is None:
                v = ((self.ok == _native.OK_BAD_OFFSETS).any().to(torch.int32) * _native.ST_OFFSETS).reshape(1)
            else:
                cur = torch.cuda.current_stream(self._buf.device)
                with torch.cuda.stream(self._stream):
                    v = ((self.ok == _native.OK_BAD_OFFSETS).any().to(torch.int32) * _native.ST_OFFSETS).reshape(1)
                cur.wait_stream(self._stream)
                v.record_stream(cur)
            self._v["status"] = v
        return v

    def __iter__(self):
        return iter((self.seq, self.ack, self.flags, self.ok, self.csum, self.payload, self.status))

    def __getitem__(self, i):
        return tuple(self)[i]

    def __len__(self):
        return 7

    def check(self) -> "VarlenDecoded":
        """Raise ValueError if a frame was rejected for bad offsets (reads ok[]: one
        device reduction and one synchronization)."""
        _raise_status(self.status)
        return self


_tls = threading.local()


def _batch_struct() -> "_native.RudpBatch":
    """This thread's reusable struct rudp_batch (the C call only reads it during the call)."""
    b = getattr(_tls, "batch", None)
    if b is None:
        b = _tls.batch = _native.RudpBatch()
    return b


def _int_tensor(t, name, device, n=None, dtypes=None):
    import torch
    dtypes = dtypes or (torch.int32,)
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype not in dtypes \
            or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous 1-D {'/'.join(map(str, dtypes))} tensor on {device}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} has {t.shape[0]} entries, expected {n}")


class HostVarlenFrames(NamedTuple):
    """Result of ``pack_batch_varlen`` on numpy arrays (host memory, staged
    through the GPU by rudp_encode_varlen_host): frames (u8, back to back),
    frame_off (int64 [N + 1]), csum (u16 [N] or None), status (always 0: the
    batch was checked before any frame byte was written, and a bad one raised)."""
    frames: Any
    frame_off: Any
    csum: Any
    status: int = 0

    def check(self) -> "HostVarlenFrames":
        return self


def _pack_varlen_host(tab: HeaderTable, payload, lengths, H, payload_off, want_csum, out, device):
    if payload_off is not None:
        raise ValueError("host-memory varlen encode takes packed payloads (payload_off=None)")
    payload = _host_arr(payload, "payload", np.uint8, 1)
    lengths = np.ascontiguousarray(lengths)
    if lengths.dtype not in (np.int32, np.uint32) or lengths.ndim != 1:
        raise TypeError("lengths must be a 1-D int32/uint32 array")
    n = lengths.shape[0]
    seq = _host_arr(tab.seq, "seq", np.uint16, 1)
    ack = _host_arr(tab.ack, "ack", np.uint16, 1)
    flags = _host_arr(tab.flags, "flags", np.uint8, 1)
    for name, a in (("seq", seq), ("ack", ack), ("flags", flags)):
        if a.shape[0] != n:
            raise ValueError(f"{name} has {a.shape[0]} entries for {n} packets")
    # (the lengths, their sum against the payload and the capacity are checked by the
    # C entry before any frame byte is written: a bad batch raises ValueError)
    if out is not None:
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 \
                or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writeable C-contiguous 1-D uint8 array")
        frames = out
    else:
        frames = np.empty((payload.size + n * H,), np.uint8)
    off = _pinned_out(n + 1, np.int64)
    csum = _pinned_out(n, np.uint16) if want_csum else None
    b = _native.RudpBatch(n=n, payload_len=min(payload.size // n, 65535) if n else 0, reserved=0,
                          seq=_ptr(seq), ack=_ptr(ack), flags=_ptr(flags), payload=_ptr(payload),
                          len=_ptr(lengths.view(np.uint32)), payload_off=None)
    _native.check(_native.lib().rudp_encode_varlen_host(
        ctypes.byref(b), payload.size, _ptr(frames) if frames.size else 16, frames.size, off.ctypes.data,
        _ptr(csum) if csum is not None else None, H, device))
    return HostVarlenFrames(frames, off, csum, 0)


def pack_batch_varlen(headers, payload, lengths, layout: Union[str, int] = "rudp7", *,
                      payload_off=None, want_csum: Optional[bool] = None, stream=None, out=None,
                      check: bool = True, reuse: Optional[VarlenFrames] = None, device: int = 0) -> VarlenFrames:
    """Frame + checksum a variable-length batch on a HIP device.

    ``payload``: u8 1-D tensor holding the payload bytes; ``lengths``: int32
    [N] bytes per packet (<= 65535); ``payload_off``: int64 [N] start of each
    payload in ``payload``, or None when the payloads are packed back to back
    in packet order.  Returns frames packed back to back plus their offsets:
    frame i is byte-identical to Packet(...).to_byte() of that packet
    (utils/reliableUDP.py:53-61 builds one per character).

    The argument checks run on the device, inside the call (rudp_encode_varlen_checked):
    ``check=True`` waits for them and raises ValueError on a bad batch, as the
    reference's per-packet calls would fail; ``check=False`` never waits — the
    host does not touch the device — and the result's ``check()`` raises later.
    A rejected batch leaves ``frames`` unwritten.  ``out``: u8 1-D frame buffer
    of at least sum(lengths) + N * header bytes (its first frame_off[-1] bytes
    are the frames).  Without ``out`` the frame buffer is sized on the host for
    packed payloads (payload.numel() + N * header bytes) and, for gathered
    payloads, from one device read of the lengths' sum.  ``reuse``: an earlier
    result of this call for the same N and csum choice, whose buffers take this
    call's outputs (no allocation; the earlier result's contents are replaced).

    numpy arrays (packed payloads in host memory, a send buffer): staged
    through GPU ``device`` by rudp_encode_varlen_host, synchronously; the
    lengths are checked before any frame byte is written (ValueError) and the
    result is a ``HostVarlenFrames`` of numpy arrays.
    """
    H = layout_header_len(layout)
    tab = _as_table(headers)
    if want_csum is None:
        want_csum = H == 5
    if not _is_torch(payload):
        return _pack_varlen_host(tab, payload, lengths, H, payload_off, want_csum, out, device)
    import torch
    dev = payload.device
    if dev.type != "cuda":
        raise ValueError("varlen batches run on a HIP device")
    _dev_check(payload, "payload", torch.uint8, 1, dev)
    _int_tensor(lengths, "lengths", dev, dtypes=(torch.int32, torch.uint32))
    n = lengths.shape[0]
    for name, t, dt in (("seq", tab.seq, torch.uint16), ("ack", tab.ack, torch.uint16),
                        ("flags", tab.flags, torch.uint8)):
        _dev_check(t, name, dt, 1, dev)
        if t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} entries for {n} packets")
    if payload_off is not None:
        _int_tensor(payload_off, "payload_off", dev, n, dtypes=(torch.int64,))
    frames = None
    if out is not None:
        _dev_check(out, "out", torch.uint8, 1, dev)
        frames = out
    if payload_off is None:
        # exact for a valid packed batch (the device checks it); an oversized `out`
        # is only capacity and never inflates the hint that picks the kernel's tiles
        lsum = payload.numel()
    elif out is not None:
        # gathered into the caller's buffer: no device read, the hint is bounded by
        # both the payload buffer and the frame buffer
        lsum = min(payload.numel(), max(out.numel() - n * H, 0))
    else:
        # gathered payloads: the frame bytes are unknown until the lengths are summed
        # (rudp_varlen_bounds, one 40-byte device read); lengths are read as u32
        lmin = lmax = lsum = omin = oend = 0
        if n:
            bnd = (ctypes.c_int64 * 5)()
            _native.check(_native.lib().rudp_varlen_bounds(
                lengths.data_ptr(), payload_off.data_ptr(), n, bnd, dev.index or 0, _stream_ptr(stream, dev)))
            lmin, lmax, lsum, omin, oend = list(bnd)
        if lmin < 0 or lmax > 65535:
            raise ValueError("lengths must lie in [0, 65535]")
        if omin < 0 or oend > payload.numel():
            raise ValueError("payload_off + lengths must stay inside payload")
    f_at, cs_bytes = VarlenFrames.layout(n, want_csum)
    if reuse is not None:
        # the caller's earlier result of the same shape: its buffer takes this call's outputs
        need = f_at + (0 if frames is not None else lsum + n * H)
        if not isinstance(reuse, VarlenFrames) or reuse._n != n or reuse._cs_bytes != cs_bytes \
                or reuse._buf.device != dev or reuse._buf.numel() != need:
            raise ValueError("reuse= must be an earlier pack_batch_varlen result for the same N, "
                             "csum choice, device and frame bytes (and out= or not, as then)")
        buf = reuse._buf
    else:
        # (payload is u8 on dev: new_empty skips torch.empty's dtype/device parsing, ~0.5 us a call)
        buf = payload.new_empty(f_at + (0 if frames is not None else lsum + n * H))
    base = buf.data_ptr()
    f_ptr = frames.data_ptr() if frames is not None else base + f_at
    f_cap = frames.numel() if frames is not None else buf.numel() - f_at
    # payload_len carries the mean payload length: a hint that picks lanes per packet
    b = _batch_struct()
    b.n, b.payload_len = n, min(lsum // n, 65535) if n else 0
    b.seq, b.ack, b.flags = tab.seq.data_ptr(), tab.ack.data_ptr(), tab.flags.data_ptr()
    b.payload = payload.data_ptr() if payload.numel() else 16  # never read: all lengths 0
    b.len = lengths.data_ptr()
    b.payload_off = payload_off.data_ptr() if payload_off is not None else None
    _native.check(_native.lib().rudp_encode_varlen_checked(
        ctypes.byref(b), payload.numel(), f_ptr if f_cap else 16, f_cap,
        base, base + 8 * (n + 1) + 8 if cs_bytes else None, base + 8 * (n + 1), H,
        dev.index or 0, _stream_ptr(stream, dev)))
    res = VarlenFrames(buf, n, cs_bytes, f_at, frames)
    return res.check() if check else res


def _check_offsets(frames, frame_off, stream=None) -> int:
    """Validate offsets (one device->host read); returns the mean frame length."""
    n = frame_off.shape[0] - 1
    if n < 1:
        return 0
    out = (ctypes.c_int64 * 3)()  # min, max, decreasing pairs (rudp_frame_off_bounds)
    _native.check(_native.lib().rudp_frame_off_bounds(
        frame_off.data_ptr(), n, out, frame_off.device.index or 0, _stream_ptr(stream, frame_off.device)))
    first, last, nbad = list(out)
    if first < 0 or nbad or last > frames.numel():
        raise ValueError("frame_off must be non-decreasing offsets inside frames")
    return min((last - first) // n, 0xFFFFFFFF)


def _unpack_varlen_host(frames, frame_off, H, csum, check, utf8, device, len_hint=0, reuse=None):
    frames = _host_arr(frames, "frames", np.uint8, 1)
    frame_off = np.ascontiguousarray(frame_off)
    if frame_off.dtype not in (np.int64, np.uint64) or frame_off.ndim != 1:
        raise TypeError("frame_off must be a 1-D int64 array")
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if csum is not None:
        csum = _host_arr(csum, "csum", np.uint16, 1)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    if reuse is not None:
        # an earlier host result of the same N and utf8 choice: its arrays take this call's outputs
        if not isinstance(reuse, DecodedBatch) or not isinstance(reuse.seq, np.ndarray) or reuse.seq.shape != (n,) \
                or (reuse.valid is not None) != utf8:
            raise ValueError("reuse= must be an earlier host unpack_batch_varlen result for the same N and utf8 choice")
        seq, ack, cs, flags, ok, valid = reuse.seq, reuse.ack, reuse.csum, reuse.flags, reuse.ok, reuse.valid
        status = reuse.status
        status[0] = 0
    else:
        seq, ack, cs = (_pinned_out(n, np.uint16) for _ in range(3))
        flags, ok = _pinned_out(n, np.uint8), _pinned_out(n, np.uint8)
        valid = _pinned_out(n, np.uint8) if utf8 else None
        status = np.zeros((1,), np.uint32)
    if n:
        # (negative int64 offsets read as huge u64 ones: past the buffer, so rejected)
        _native.check(_native.lib().rudp_decode_varlen_host(
            _ptr(frames), frames.size, frame_off.ctypes.data, min(len_hint or frames.size // n, 0xFFFFFFFF), n,
            _ptr(csum) if csum is not None else None, _ptr(seq), _ptr(ack), _ptr(flags), _ptr(ok), _ptr(cs),
            _ptr(valid) if valid is not None else None, status.ctypes.data, H, device))
    # payload spans computed on first use (two passes over N offsets: ~1 ms per 1M frames)
    pay = PayloadSpans(frame_off.view(np.int64) if frame_off.dtype == np.uint64 else frame_off, H)
    res = DecodedBatch(seq, ack, flags, ok, cs, pay, status, valid)
    return res.check() if check else res


def unpack_batch_varlen(frames, frame_off, layout: Union[str, int] = "rudp7", *, csum=None,
                        stream=None, check: bool = True, reuse: Optional["VarlenDecoded"] = None,
                        utf8: bool = False, device: int = 0) -> "VarlenDecoded":
    """Parse + verify frames packed back to back (offsets as pack_batch_varlen returns).

    The payload is zero-copy: ``payload`` is the pair ``(start, end)`` of int64
    [N] tensors indexing ``frames`` (empty for frames shorter than the header),
    as a ``PayloadSpans`` that computes ``start`` on first use.  The offsets
    are checked on the device inside the call (rudp_decode_varlen_checked):
    every frame with bad offsets gets ok == RUDP_OK_BAD_OFFSETS, and
    ``check=True`` waits and raises ValueError when there is one;
    ``check=False`` never waits, and the result's ``check()`` raises later.
    ``reuse``: an earlier result for the same N whose output buffer takes this
    call's outputs (no allocation).  ``utf8``: also ``valid`` (u8 [N]: 1 where
    Packet(frame).get_payload() would return, 0 where its strict UTF-8 decode
    would raise, utils/packet.py:68-73; 0 for a rejected frame), judged by the
    decode kernel from the bytes it already holds (rudp_decode_varlen_utf8).

    numpy arrays (a receive buffer in host memory): staged through GPU
    ``device`` by rudp_decode_varlen_host, synchronously, with the same
    per-frame offset rule; the result is a ``DecodedBatch`` of numpy arrays
    (payload: ``PayloadSpans`` of int64 arrays, status u32 [1]); ``reuse``: an
    earlier such result whose arrays take this call's outputs (a receive loop
    keeps its buffers; pinned ones copy back at the link's rate).
    """
    H = layout_header_len(layout)
    if H == 7 and csum is not None:
        raise ValueError("rudp7 carries its checksum in-band; csum= is for rudp5")
    if not _is_torch(frames):
        return _unpack_varlen_host(frames, frame_off, H, csum, check, utf8, device, reuse=reuse)
    import torch
    dev = frames.device
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if csum is not None:
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    # one allocation for every output: seq | ack | csum (u16) | flags | ok (u8), cut
    # into views only when the caller reads them (per-view slicing was most of the
    # entry's host time at small batches)
    per = 9 if utf8 else 8
    if reuse is not None:
        if not isinstance(reuse, VarlenDecoded) or reuse._n != n or reuse._buf.device != dev \
                or reuse._utf8 != utf8:
            raise ValueError("reuse= must be an earlier unpack_batch_varlen result for the same N, device "
                             "and utf8 choice")
        buf = reuse._buf
    else:
        buf = frames.new_empty(per * n)  # (u8 on dev, checked above)
    base = buf.data_ptr()
    # mean frame length from the buffer size: a hint that picks lanes / tiles per frame
    hint = min(frames.numel() // n, 0xFFFFFFFF) if n else 0
    # no status word: a rejected frame is ok == RUDP_OK_BAD_OFFSETS (check() reads that)
    _native.check(_native.lib().rudp_decode_varlen_utf8(
        frames.data_ptr() if frames.numel() else 16, frames.numel(), frame_off.data_ptr(), hint, n,
        csum.data_ptr() if csum is not None else None, base, base + 2 * n, base + 6 * n, base + 7 * n,
        base + 4 * n, base + 8 * n if utf8 else None, None, H, dev.index or 0, _stream_ptr(stream, dev)))
    res = VarlenDecoded(buf, n, PayloadSpans(frame_off, H), utf8, stream)
    return res.check() if check else res


class GatheredPayloads:
    """Result of ``gather_payloads``: ``buffer`` (u8, the whole output buffer:
    the caller's ``out`` or the allocation; its first payload_off[-1] bytes are
    the kept payloads back to back), ``payload_off`` (int64 [N + 1]: payload i
    = buffer[payload_off[i]:payload_off[i + 1]], empty for a dropped, rejected
    or header-only frame), ``status`` (device int32 [1], RUDP_ST_* of the call,
    0 = valid), ``lengths`` (int32 [N], the differences of ``payload_off``,
    computed on first use) and ``payload`` (``buffer[:total]``: the message;
    one synchronization on first use, to read the total).  ``buffer`` and
    ``lengths`` are ``pack_batch_varlen``'s packed payload and lengths."""

    __slots__ = ("buffer", "_buf", "_n", "_payload_off", "_status", "_lengths", "_payload")

    # one allocation: payload_off (i64 [n + 1]) | status (i32) | pad
    def __init__(self, buffer, buf, n: int):
        self.buffer, self._buf, self._n = buffer, buf, n
        self._payload_off = self._status = self._lengths = self._payload = None

    @property
    def payload_off(self):
        if self._payload_off is None:
            import torch
            self._payload_off = self._buf[:8 * (self._n + 1)].view(torch.int64)
        return self._payload_off

    @property
    def status(self):
        if self._status is None:
            import torch
            at = 8 * (self._n + 1)
            self._status = self._buf[at:at + 4].view(torch.int32)
        return self._status

    @property
    def lengths(self):
        if self._lengths is None:
            import torch
            off = self.payload_off
            self._lengths = (off[1:] - off[:-1]).to(torch.int32)
        return self._lengths

    @property
    def payload(self):
        if self._payload is None:
            self._payload = self.buffer[:min(int(self.payload_off[-1].item()), self.buffer.numel())]
        return self._payload

    def check(self) -> "GatheredPayloads":
        """Raise ValueError if the device rejected a frame's offsets or found
        ``out`` too small (then with the byte count it needs); one synchronization."""
        bits = int(self.status.item())
        if bits:
            msgs = [m for b, m in _ST_MESSAGES if bits & b] or [f"status {bits:#x}"]
            if bits & _native.ST_PAYLOAD_CAP:
                msgs.append(f"{int(self.payload_off[-1].item())} bytes are needed, out has {self.buffer.numel()}")
            raise ValueError("; ".join(msgs))
        return self


def keep_mask(decoded, dup=None, *, unverified: bool = False):
    """u8 [N]: 1 for the usable frames of a decoded batch -- decoded
    ``ok == 1``, ``valid == 1`` where the decode judged UTF-8 (``utf8=True``),
    and, with ``dup`` (``detect_retransmissions``: the proxy's window rule), not
    a retransmission.  It knows nothing of sequence numbers: these are the
    frames a receiver can parse, not the ones it accepts (``accept_inorder``
    decides that, with this mask as ``usable``).  ``unverified``: rudp5 frames
    decoded without a sideband checksum (``ok == 3``) are usable too."""
    import torch
    m = decoded.ok == _native.OK_GOOD
    if unverified:
        m = m | (decoded.ok == _native.OK_UNVERIFIED)
    if decoded.valid is not None:
        m = m & (decoded.valid == 1)
    if dup is not None:
        m = m & (dup == 0)
    return m.to(torch.uint8)


def gather_payloads(frames, frame_off, layout: Union[str, int] = "rudp7", *, keep=None, out=None, stream=None,
                    check: bool = True) -> GatheredPayloads:
    """The payloads of the kept frames of a packed batch, back to back, with
    their offsets: the reference receiver's ``buffer + payload`` per accepted
    datagram (utils/reliableUDP.py:121, :135-136) for a whole batch, and the
    inverse of the packed ``pack_batch_varlen`` (rudp_gather_payloads).

    Device tensors only: ``frames`` u8 1-D, ``frame_off`` int64 [N + 1] as
    ``pack_batch_varlen`` returns them, ``keep`` a u8 or bool [N] tensor (0 =
    drop the frame; None keeps every frame; see ``keep_mask``).  A frame whose
    pair of offsets is decreasing or past ``frames`` contributes nothing and is
    never read, as in ``unpack_batch_varlen``.  ``out``: u8 1-D buffer for the
    payloads; None allocates frames.numel() bytes, an upper bound that needs
    no device read.  A caller's ``out`` may be smaller: when the kept payloads
    do not fit, nothing is written to it and the status says so.

    ``check=True`` waits and raises ValueError for rejected offsets or a too
    small ``out`` (with the byte count needed); ``check=False`` never waits,
    and the result's ``check()`` raises later.
    """
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("gather_payloads takes torch tensors on a HIP device (no host-memory form)")
    import torch
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("gather_payloads runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if keep is not None:
        _int_tensor(keep, "keep", dev, n, dtypes=(torch.uint8, torch.bool))
    if out is not None:
        _dev_check(out, "out", torch.uint8, 1, dev)
    buffer = out if out is not None else frames.new_empty(frames.numel())
    head = 8 * (n + 1) + 8
    buf = frames.new_empty(head)
    base = buf.data_ptr()
    if n:
        _native.check(_native.lib().rudp_gather_payloads(
            frames.data_ptr() if frames.numel() else None, frames.numel(), frame_off.data_ptr(),
            min(frames.numel() // n, 0xFFFFFFFF), n, keep.data_ptr() if keep is not None else None,
            buffer.data_ptr() if buffer.numel() else None, buffer.numel(), base, base + 8 * (n + 1), H,
            dev.index or 0, _stream_ptr(stream, dev)))
    else:
        buf.zero_()
    res = GatheredPayloads(buffer, buf, n)
    return res.check() if check else res


# ------------------------------------------------------------ in-order acceptance
# The launch geometry of csrc/accept.hip, for callers that size batches and for the
# tests' edge cases (tests/test_accept_api.py holds these to the kernel source).
ACCEPT_TILE = 1024      # frames per tile of rudp_accept_inorder; a batch up to one tile is one launch
ACCEPT_BASES = 256      # tiles up to which its bases pass takes one tile per thread
CHARS_BLOCK = 256       # threads per workgroup of rudp_payload_chars: 256 / lanes frames each
NO_ISN = 0xFFFFFFFF     # last_isn: no previous transfer


def payload_chars_lanes(len_hint: int, H: int) -> int:
    """Lanes per frame rudp_payload_chars picks for a typical frame length: the
    fewest, a power of two up to 64, that leave a lane at most four 16-byte
    blocks (the geometry only; never the result)."""
    blocks = max(len_hint - H, 0) // 16 + 1
    lanes = 1
    while lanes < 64 and blocks > 4 * lanes:
        lanes *= 2
    return lanes


def payload_chars(frames, frame_off, layout: Union[str, int] = "rudp7", *, stream=None):
    """int32 [N]: the characters of every frame's payload, counted as lead bytes
    ((b & 0xC0) != 0x80: Python's len() of the payload for valid UTF-8), for
    ``accept_inorder`` (rudp_payload_chars).  Device tensors as
    ``gather_payloads`` takes them; a frame shorter than the header, or one
    whose offsets are decreasing or past ``frames``, has 0.  Never waits."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("payload_chars takes torch tensors on a HIP device (no host-memory form)")
    import torch
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("payload_chars runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    chars = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _native.check(_native.lib().rudp_payload_chars(
            frames.data_ptr() if frames.numel() else None, frames.numel(), frame_off.data_ptr(),
            min(frames.numel() // n, 0xFFFFFFFF), n, chars.data_ptr(), H, dev.index or 0,
            _stream_ptr(stream, dev)))
    return chars


class Accepted:
    """Result of ``accept_inorder``: ``accept``, ``keep``, ``reply`` (u8 [N])
    and ``reply_ack`` (u16 [N]) as rudp_accept_inorder defines them, and
    ``state`` (int64 [4] on the device: expect, isn, live, 0 after the call;
    pass it as ``state=`` of the next call).  ``end`` (N when no accepted frame
    had FIN), ``count`` (accepted frames), ``msg_start`` (index of the last
    reset at or before ``end``, N when there is none), ``characters`` (of the
    message so far), ``first_anomaly`` and ``fast`` (the one-scan form was
    exact: ``first_anomaly == N``) are read from the device on first use, one
    synchronization for all of them; nothing else waits."""

    __slots__ = ("_buf", "_n", "_lay", "_views", "_info")

    def __init__(self, buf, n: int):
        self._buf, self._n, self._lay = buf, n, Accepted.layout(n)
        self._views, self._info = {}, None

    @staticmethod
    def layout(n: int):
        """Byte offsets in the one allocation: accept | keep | reply (u8 [n]) |
        reply_ack (u16 [n]) | state (u64 [4]) | info (u64 [6]); then the size."""
        ack = (3 * n + 1) & ~1
        state = (ack + 2 * n + 7) & ~7
        return 0, n, 2 * n, ack, state, state + 32, state + 80

    def _cut(self, name, lo, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    @property
    def accept(self):
        return self._cut("accept", self._lay[0], self._n, None)

    @property
    def keep(self):
        return self._cut("keep", self._lay[1], self._n, None)

    @property
    def reply(self):
        return self._cut("reply", self._lay[2], self._n, None)

    @property
    def reply_ack(self):
        import torch
        return self._cut("reply_ack", self._lay[3], 2 * self._n, torch.uint16)

    @property
    def state(self):
        import torch
        return self._cut("state", self._lay[4], 32, torch.int64)

    @property
    def info(self):
        """int64 [6] on the device: end, count, msg_start, characters, first_anomaly, 0."""
        import torch
        return self._cut("info", self._lay[5], 48, torch.int64)

    def _host_info(self):
        if self._info is None:
            self._info = [int(v) for v in self.info.tolist()]
        return self._info

    @property
    def end(self) -> int:
        return self._host_info()[0]

    @property
    def count(self) -> int:
        return self._host_info()[1]

    @property
    def msg_start(self) -> int:
        return self._host_info()[2]

    @property
    def characters(self) -> int:
        return self._host_info()[3]

    @property
    def first_anomaly(self) -> int:
        return self._host_info()[4]

    @property
    def fast(self) -> bool:
        return self._host_info()[4] == self._n

    def __len__(self) -> int:
        return self._n


_NO_STATE = {}  # device index -> the all-zero state (no transfer yet, no peer); only ever read


def _accept_state(state, dev):
    import torch
    if state is None:
        # One zero tensor per device, made outside any stream capture and complete
        # before it is first used (the one wait, once per device), so later calls
        # on any stream, captured ones included, may read it.  A first call inside
        # a capture gets a tensor of its own, which belongs to that graph.
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        zero = _NO_STATE.get(key)
        if zero is None:
            zero = torch.zeros(4, dtype=torch.int64, device=dev)
            if torch.cuda.is_current_stream_capturing():
                return zero
            torch.cuda.current_stream(dev).synchronize()
            _NO_STATE[key] = zero
        return zero
    if _is_torch(state):
        _int_tensor(state, "state", dev, 4, dtypes=(torch.int64,))
        return state
    try:
        expect, isn, live = (int(v) for v in state)
    except (TypeError, ValueError):
        raise TypeError("state must be None, (expect, isn, live) or an Accepted.state tensor") from None
    if expect < 0 or isn < 0:
        raise ValueError("state: expect and isn must not be negative")
    return torch.tensor([expect, isn, 1 if live else 0, 0], dtype=torch.int64).to(dev)


def _check_last_isn(last_isn) -> int:
    if last_isn is None:
        return NO_ISN
    if isinstance(last_isn, bool) or not isinstance(last_isn, int) or last_isn < 0:
        raise ValueError(f"last_isn must be None or a non-negative int, got {last_isn!r}")
    return min(last_isn, NO_ISN)


def accept_inorder(seq, flags, chars, *, usable=None, state=None, last_isn=None, stream=None) -> Accepted:
    """Which datagrams of a batch the reference's receiver accepts, in arrival
    order (``receive_data``, utils/reliableUDP.py:116-137: a SYN opens a
    transfer, then only the frame whose seq_num is ISN + characters received so
    far is accepted), and the ack_num of the reply it sends for each
    (``send_ack``, :139-146), on the device with no host wait
    (rudp_accept_inorder; include/rudp.h states the rule).

    ``seq`` (u16 [N]) and ``flags`` (u8 [N]) as the decode returns them,
    ``chars`` (int32 [N]) from ``payload_chars``, ``usable`` a u8 or bool [N]
    tensor (``keep_mask``; None: every frame).  ``state``: None (no transfer
    yet, no peer), ``(expect, isn, live)``, or the ``state`` of the previous
    call's result, which carries a transfer across batches without a host
    read.  (The first ``state=None`` call on a device waits once for its zero
    state to be written; no later call waits.)  ``last_isn``: the previous transfer's ISN, whose repeated SYN is
    ignored (None: there was none)."""
    if not _is_torch(seq) or not _is_torch(flags) or not _is_torch(chars):
        raise TypeError("accept_inorder takes torch tensors on a HIP device (no host-memory form)")
    import torch
    dev = seq.device
    if dev.type != "cuda":
        raise ValueError("accept_inorder runs on a HIP device")
    _dev_check(seq, "seq", torch.uint16, 1, dev)
    n = seq.shape[0]
    _int_tensor(flags, "flags", dev, n, dtypes=(torch.uint8,))
    _int_tensor(chars, "chars", dev, n, dtypes=(torch.int32,))
    if usable is not None:
        _int_tensor(usable, "usable", dev, n, dtypes=(torch.uint8, torch.bool))
    last = _check_last_isn(last_isn)
    st = _accept_state(state, dev)
    lay = Accepted.layout(n)
    buf = torch.empty(lay[6], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    tab = n > 0
    _native.check(_native.lib().rudp_accept_inorder(
        seq.data_ptr() if tab else None, flags.data_ptr() if tab else None, chars.data_ptr() if tab else None,
        usable.data_ptr() if usable is not None and tab else None, n, last, st.data_ptr(),
        base + lay[0] if tab else None, base + lay[1] if tab else None, base + lay[2] if tab else None,
        base + lay[3] if tab else None, base + lay[4], base + lay[5], dev.index or 0, _stream_ptr(stream, dev)))
    return Accepted(buf, n)


class ReceivedBatch(NamedTuple):
    """Result of ``receive_batch``: ``message`` (``GatheredPayloads``: its
    ``payload`` is this batch's part of the message, the bytes ``recv()``
    appends), ``accepted`` (``Accepted``) and ``replies`` (``HeaderTable`` of
    N rows for ``pack_batch``: seq 0, ack = reply_ack, flags ACK where a reply
    is sent and 0 where none is; select the rows with ``accepted.reply``)."""
    message: GatheredPayloads
    accepted: Accepted
    replies: HeaderTable


def receive_batch(frames, frame_off, layout: Union[str, int] = "rudp7", *, csum=None, state=None,
                  last_isn=None) -> ReceivedBatch:
    """A batch of datagrams (packed frames, as recvmmsg leaves them) turned into
    what the reference's ``recv()`` loop makes of them, with no host wait in
    between, on the current stream: ``unpack_batch_varlen(utf8=True)`` -> ``keep_mask`` (the usable
    frames; rudp5 without ``csum`` has no checksum to fail) -> ``payload_chars``
    -> ``accept_inorder`` -> ``gather_payloads(keep=accepted.keep)``.

    ``state`` and ``last_isn`` as ``accept_inorder`` takes them.  When
    ``accepted.msg_start`` is N the bytes continue the caller's buffer of the
    earlier batches, else they replace it; ``accepted.end < N`` ends the
    transfer, and the frames behind it belong to the next call."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("receive_batch takes torch tensors on a HIP device (no host-memory form)")
    last = _check_last_isn(last_isn)
    dec = unpack_batch_varlen(frames, frame_off, H, csum=csum, check=False, utf8=True)
    usable = keep_mask(dec, unverified=H == 5 and csum is None)
    chars = payload_chars(frames, frame_off, H)
    acc = accept_inorder(dec.seq, dec.flags, chars, usable=usable, state=state, last_isn=last)
    msg = gather_payloads(frames, frame_off, H, keep=acc.keep, check=False)
    import torch
    replies = HeaderTable(torch.zeros_like(acc.reply_ack), acc.reply_ack, acc.reply * ACK)
    return ReceivedBatch(msg, acc, replies)


# ------------------------------------------------------------ batch -> message and replies
# The geometry of csrc/receive.hip (tests/test_receive_api.py holds these to the source).
RECV_TILE = ACCEPT_TILE     # a batch of at most this many datagrams ...
RECV_FUSED_BYTES = 32768    # ... in at most this many bytes ...
RECV_FUSED_MEAN = 261       # ... and this many per datagram is one launch of one workgroup


class Received:
    """Result of ``receive``: one allocation, every member a view of it.

    ``seq``, ``ack``, ``csum`` (u16 [N]), ``flags``, ``ok``, ``valid`` (u8 [N])
    as ``unpack_batch_varlen(utf8=True)`` returns them; ``usable`` (u8 [N],
    ``keep_mask``'s answer) and ``chars`` (int32 [N], ``payload_chars``');
    ``accepted`` (an ``Accepted``: accept, keep, reply, reply_ack, state and
    the host reads end, count, msg_start, characters, first_anomaly);
    ``message`` (a ``GatheredPayloads``: payload, payload_off, lengths,
    check()); ``reply_frames`` (u8 [N * H]: the first ``reply_count * H`` bytes
    are the reply datagrams, header-only frames at stride H in arrival order),
    ``reply_csum`` (u16 [N]), ``reply_index`` (int32 [N]: the datagram each
    reply answers), ``reply_peer`` (int64 [N]: the datagram whose source the
    reply goes to, N = the peer carried from earlier batches), of which the
    first ``reply_count`` entries are written; ``state`` (int64 [4], for the
    next call's ``state=``), ``info`` (int64 [8]) and ``status`` (int32 [1],
    RUDP_ST_* of the call) on the device.  ``reply_count``, ``message_bytes``
    and the host reads of ``accepted`` synchronize once, on first use, and are
    cached; nothing else waits."""

    __slots__ = ("_buf", "_n", "_H", "_lay", "_views", "_info", "accepted", "message")

    def __init__(self, buf, n: int, H: int, cap: int):
        self._buf, self._n, self._H, self._lay = buf, n, H, Received.layout(n, H, cap)
        self._views, self._info = {}, None
        lay = self._lay
        self.accepted = Accepted(buf[lay["accepted"]:lay["chars"]], n)
        self.message = GatheredPayloads(buf[lay["payload"]:lay["payload"] + cap],
                                        buf[lay["payload_off"]:lay["reply_peer"]], n)

    @staticmethod
    def layout(n: int, H: int, cap: int):
        """Byte offsets in the one allocation, every array aligned to its
        element (the payload to 16 bytes); ``size`` is the allocation's."""
        lay, at = {}, 0
        for name, nbytes in (("payload_off", 8 * (n + 1) + 8),           # then status (i32) and a pad
                             ("reply_peer", 8 * n),
                             ("accepted", (Accepted.layout(n)[6] + 16 + 7) & ~7),  # its info has 8 words here
                             ("chars", 4 * n), ("reply_index", 4 * n),
                             ("seq", 2 * n), ("ack", 2 * n), ("csum", 2 * n), ("reply_csum", 2 * n),
                             ("flags", n), ("ok", n), ("valid", n), ("usable", n),
                             ("reply_frames", n * H)):
            lay[name] = at
            at += nbytes
        lay["payload"] = (at + 15) & ~15
        lay["size"] = lay["payload"] + cap
        return lay

    def _cut(self, name, nbytes, dtype, at=None):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name] if at is None else at
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    def _u16(self, name):
        import torch
        return self._cut(name, 2 * self._n, torch.uint16)

    seq = property(lambda self: self._u16("seq"))
    ack = property(lambda self: self._u16("ack"))
    csum = property(lambda self: self._u16("csum"))
    reply_csum = property(lambda self: self._u16("reply_csum"))
    flags = property(lambda self: self._cut("flags", self._n, None))
    ok = property(lambda self: self._cut("ok", self._n, None))
    valid = property(lambda self: self._cut("valid", self._n, None))
    usable = property(lambda self: self._cut("usable", self._n, None))
    reply_frames = property(lambda self: self._cut("reply_frames", self._n * self._H, None))

    @property
    def chars(self):
        import torch
        return self._cut("chars", 4 * self._n, torch.int32)

    @property
    def reply_index(self):
        import torch
        return self._cut("reply_index", 4 * self._n, torch.int32)

    @property
    def reply_peer(self):
        import torch
        return self._cut("reply_peer", 8 * self._n, torch.int64)

    @property
    def state(self):
        return self.accepted.state

    @property
    def info(self):
        """int64 [8] on the device: end, count, msg_start, characters,
        first_anomaly, reply_count, message_bytes, 0."""
        import torch
        return self._cut("info", 64, torch.int64, self._lay["accepted"] + Accepted.layout(self._n)[5])

    @property
    def status(self):
        return self.message.status

    def _host_info(self):
        if self._info is None:
            self._info = [int(v) for v in self.info.tolist()]
            self.accepted._info = self._info[:6]
        return self._info

    @property
    def reply_count(self) -> int:
        return self._host_info()[5]

    @property
    def message_bytes(self) -> int:
        return self._host_info()[6]

    def check(self) -> "Received":
        """Raise ValueError if the device rejected a frame's offsets or the
        message did not fit; one synchronization."""
        self.message.check()
        return self

    def __len__(self) -> int:
        return self._n


def receive(frames, frame_off, layout: Union[str, int] = "rudp7", *, csum=None, state=None, last_isn=None,
            stream=None) -> Received:
    """``receive_batch`` and the reply datagrams in one library call
    (rudp_receive): a batch of datagrams (packed frames, as recvmmsg leaves
    them) decoded, judged in order and gathered into this batch's part of the
    message, and the ``send_ack`` packets of utils/reliableUDP.py:139-146 built
    for ``sendmmsg``, with no host wait and no torch operation in between.  A
    batch of at most ``RECV_TILE`` datagrams in at most ``RECV_FUSED_BYTES``
    bytes (and ``RECV_FUSED_MEAN`` per datagram) is one kernel launch.

    ``frames`` (u8 1-D), ``frame_off`` (int64 [N + 1]) and ``csum`` (u16 [N],
    the rudp5 sideband; None: rudp5 frames are taken unverified) are device
    tensors; ``state`` and ``last_isn`` as ``accept_inorder`` takes them
    (``state`` may be the previous result's ``state``, which carries a
    transfer without a host read).  Every array equals what the calls of
    ``receive_batch`` return for the same input."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("receive takes torch tensors on a HIP device (no host-memory form)")
    import torch
    last = _check_last_isn(last_isn)
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("receive runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if csum is not None:
        if H == 7:
            raise ValueError("rudp7 carries its checksum in-band; csum is for rudp5")
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    st = _accept_state(state, dev)
    cap = frames.numel()
    lay = Received.layout(n, H, cap)
    if n:
        buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    else:  # payload_off[0], which an empty call does not write (a few bytes, on the call's stream)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            buf = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    alay = Accepted.layout(n)
    acc = base + lay["accepted"]

    def tab(at):
        return at if n else None

    out = _native.RudpReceived(
        seq=tab(base + lay["seq"]), ack=tab(base + lay["ack"]), flags=tab(base + lay["flags"]),
        ok=tab(base + lay["ok"]), csum_out=tab(base + lay["csum"]), valid=tab(base + lay["valid"]),
        usable=tab(base + lay["usable"]), chars=tab(base + lay["chars"]), accept=tab(acc + alay[0]),
        keep=tab(acc + alay[1]), reply=tab(acc + alay[2]), reply_ack=tab(acc + alay[3]), state_out=acc + alay[4],
        payload=base + lay["payload"] if cap else None, payload_cap=cap, payload_off=tab(base + lay["payload_off"]),
        reply_frames=tab(base + lay["reply_frames"]), reply_csum=tab(base + lay["reply_csum"]),
        reply_index=tab(base + lay["reply_index"]), reply_peer=tab(base + lay["reply_peer"]),
        info=acc + alay[5], status=base + lay["payload_off"] + 8 * (n + 1))
    _native.check(_native.lib().rudp_receive(
        frames.data_ptr() if cap else None, cap, frame_off.data_ptr(), min(cap // n, 0xFFFFFFFF) if n else 0, n,
        csum.data_ptr() if csum is not None and n else None, last, st.data_ptr(), ctypes.byref(out), H,
        dev.index or 0, _stream_ptr(stream, dev)))
    return Received(buf, n, H, cap)


# ------------------------------------------------------------ the reordering receiver
# The geometry of csrc/window.hip.
WINDOW_CHUNK = 1024         # new frames per launch of rudp_accept_window
WINDOW_MAX = 1024           # the largest window_chars; a call carries at most WINDOW_MAX - 1 frames
RANK_NONE = _native.RANK_NONE


class WindowAccepted:
    """Result of ``accept_window``: one device buffer with cut views.
    ``accept`` (u8 [N]: 1 delivered, 2 pending when the call ends), ``rank``
    and ``carry_rank`` (int32 [N] holding u32 values; -1 is RUDP_RANK_NONE),
    ``reply`` (u8 [N]), ``reply_ack`` (u16 [N]), ``state`` (int64 [4], for the
    next call's ``state=``) and ``info`` (int64 [8]: end, ranked, msg_start,
    characters, first_anomaly, pending, delivered, 0) as rudp_accept_window
    defines them.  ``end``, ``count`` (ranked frames), ``msg_start``,
    ``characters``, ``first_anomaly``, ``pending``, ``delivered`` and ``fast``
    are read from the device on first use, one synchronization for all."""

    __slots__ = ("_buf", "_n", "_lay", "_views", "_info")

    def __init__(self, buf, n: int):
        self._buf, self._n, self._lay = buf, n, WindowAccepted.layout(n)
        self._views, self._info = {}, None

    @staticmethod
    def layout(n: int):
        """Byte offsets in the one allocation: rank | carry_rank (u32 [n]) |
        reply_ack (u16 [n]) | accept | reply (u8 [n]) | state (u64 [4]) | info
        (u64 [8]); then the size."""
        lay, at = {}, 0
        for name, nbytes in (("rank", 4 * n), ("carry_rank", 4 * n), ("reply_ack", 2 * n), ("accept", n),
                             ("reply", n)):
            lay[name] = at
            at += nbytes
        lay["state"] = (at + 7) & ~7
        lay["info"] = lay["state"] + 32
        lay["size"] = lay["info"] + 64
        return lay

    def _cut(self, name, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    accept = property(lambda self: self._cut("accept", self._n, None))
    reply = property(lambda self: self._cut("reply", self._n, None))

    @property
    def rank(self):
        import torch
        return self._cut("rank", 4 * self._n, torch.int32)

    @property
    def carry_rank(self):
        import torch
        return self._cut("carry_rank", 4 * self._n, torch.int32)

    @property
    def reply_ack(self):
        import torch
        return self._cut("reply_ack", 2 * self._n, torch.uint16)

    @property
    def state(self):
        import torch
        return self._cut("state", 32, torch.int64)

    @property
    def info(self):
        import torch
        return self._cut("info", 64, torch.int64)

    def _host_info(self):
        if self._info is None:
            self._info = [int(v) for v in self.info.tolist()]
        return self._info

    end = property(lambda self: self._host_info()[0])
    count = property(lambda self: self._host_info()[1])
    msg_start = property(lambda self: self._host_info()[2])
    characters = property(lambda self: self._host_info()[3])
    first_anomaly = property(lambda self: self._host_info()[4])
    pending = property(lambda self: self._host_info()[5])
    delivered = property(lambda self: self._host_info()[6])
    fast = property(lambda self: self._host_info()[4] == self._n)

    def __len__(self) -> int:
        return self._n


def _check_window(window_chars) -> int:
    if isinstance(window_chars, bool) or not isinstance(window_chars, int) or not 1 <= window_chars <= WINDOW_MAX:
        raise ValueError(f"window_chars must be an int in [1, {WINDOW_MAX}], got {window_chars!r}")
    return window_chars


def accept_window(seq, flags, chars, *, window_chars, carried: int = 0, usable=None, state=None, last_isn=None,
                  stream=None) -> WindowAccepted:
    """``accept_inorder`` for a windowed sender (rudp_accept_window;
    include/rudp.h states the rule): a frame ahead of the expected one inside
    ``window_chars`` characters waits, is delivered when the gap before it
    fills, and every reply is a cumulative acknowledgement.  The first
    ``carried`` frames are the ones the previous call left pending (its
    ``accept == 2``), presented again in its order; they get no reply.  With
    ``window_chars=1`` the result is ``accept_inorder``'s.  The other arguments
    as ``accept_inorder`` takes them; never waits."""
    if not _is_torch(seq) or not _is_torch(flags) or not _is_torch(chars):
        raise TypeError("accept_window takes torch tensors on a HIP device (no host-memory form)")
    import torch
    dev = seq.device
    if dev.type != "cuda":
        raise ValueError("accept_window runs on a HIP device")
    Wc = _check_window(window_chars)
    _dev_check(seq, "seq", torch.uint16, 1, dev)
    n = seq.shape[0]
    if isinstance(carried, bool) or not isinstance(carried, int) or not 0 <= carried <= min(n, WINDOW_MAX - 1):
        raise ValueError(f"carried must be an int in [0, min(N, {WINDOW_MAX - 1})], got {carried!r}")
    _int_tensor(flags, "flags", dev, n, dtypes=(torch.uint8,))
    _int_tensor(chars, "chars", dev, n, dtypes=(torch.int32,))
    if usable is not None:
        _int_tensor(usable, "usable", dev, n, dtypes=(torch.uint8, torch.bool))
    last = _check_last_isn(last_isn)
    st = _accept_state(state, dev)
    lay = WindowAccepted.layout(n)
    buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(t):
        return t if n else None

    _native.check(_native.lib().rudp_accept_window(
        tab(seq.data_ptr()), tab(flags.data_ptr()), tab(chars.data_ptr()),
        usable.data_ptr() if usable is not None and n else None, n, last, Wc, carried, st.data_ptr(),
        tab(base + lay["accept"]), tab(base + lay["rank"]), tab(base + lay["carry_rank"]), tab(base + lay["reply"]),
        tab(base + lay["reply_ack"]), base + lay["state"], base + lay["info"], dev.index or 0,
        _stream_ptr(stream, dev)))
    return WindowAccepted(buf, n)


_ST_ORDERED = ((_native.ST_OFFSETS, "a ranked frame's offsets are decreasing or outside the frame buffer"),
               (_native.ST_RANK, "a rank at or above the count is not RANK_NONE"),
               (_native.ST_PAYLOAD_CAP, "the ranked frames do not fit the output buffer"))


class OrderedPayloads:
    """Result of ``gather_ordered``: ``buffer`` (u8, the caller's ``out`` or the
    allocation), ``out_off`` (int64 [N + 1], of which [0..K] are written),
    ``src`` (int32 [N], of which [0..K) are written: the frame of rank k),
    ``count`` (the int64 [1] device tensor K was read from) and ``status``
    (int32 [1], RUDP_ST_*).  ``total`` (K and the bytes, one synchronization
    on first use) and ``payload`` (``buffer[:bytes]``) wait; nothing else does."""

    __slots__ = ("buffer", "out_off", "src", "count", "status", "_total")

    def __init__(self, buffer, out_off, src, count, status):
        self.buffer, self.out_off, self.src, self.count, self.status = buffer, out_off, src, count, status
        self._total = None

    @property
    def total(self):
        """(K, bytes) on the host."""
        if self._total is None:
            import torch
            n = self.out_off.shape[0] - 1
            K = torch.clamp(self.count, 0, n)
            self._total = tuple(int(v) for v in torch.cat((K, self.out_off[K])).tolist())
        return self._total

    @property
    def payload(self):
        return self.buffer[:min(self.total[1], self.buffer.numel())]

    def check(self) -> "OrderedPayloads":
        bits = int(self.status.item())
        if bits:
            msgs = [m for b, m in _ST_ORDERED if bits & b] or [f"status {bits:#x}"]
            if bits & _native.ST_PAYLOAD_CAP:
                msgs.append(f"{self.total[1]} bytes are needed, out has {self.buffer.numel()}")
            raise ValueError("; ".join(msgs))
        return self


def gather_ordered(frames, frame_off, rank, count, *, skip: int, out=None, stream=None) -> OrderedPayloads:
    """``gather_payloads`` with a permutation (rudp_gather_ordered): frame i
    with ``rank[i]`` = r below K puts its bytes from ``skip`` (0, 5 or 7) on at
    position r of the output.  ``rank``: int32 [N] holding u32 values
    (``WindowAccepted.rank`` or ``.carry_rank``; -1 = none); ``count``: an
    int64 [1] device tensor holding K, read on the device
    (``WindowAccepted.info[1:2]`` or ``[5:6]``).  ``out``: u8 1-D buffer; None
    allocates frames.numel() bytes, which always suffice.  Never waits;
    ``check()`` on the result raises for a non-zero status."""
    if not _is_torch(frames) or not _is_torch(frame_off) or not _is_torch(rank) or not _is_torch(count):
        raise TypeError("gather_ordered takes torch tensors on a HIP device (no host-memory form)")
    import torch
    if skip not in (0, 5, 7):
        raise ValueError(f"skip must be 0, 5 or 7, got {skip!r}")
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("gather_ordered runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    _int_tensor(rank, "rank", dev, n, dtypes=(torch.int32,))
    _int_tensor(count, "count", dev, 1, dtypes=(torch.int64,))
    if out is not None:
        _dev_check(out, "out", torch.uint8, 1, dev)
    buffer = out if out is not None else frames.new_empty(frames.numel())
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        # out_off (i64 [n + 1]) | src (i32 [n]) | status (i32); an empty call writes nothing, so zeros
        buf = (torch.empty if n else torch.zeros)(8 * (n + 1) + 4 * n + 4, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    if n:
        _native.check(_native.lib().rudp_gather_ordered(
            frames.data_ptr() if frames.numel() else None, frames.numel(), frame_off.data_ptr(),
            min(frames.numel() // n, 0xFFFFFFFF), n, rank.data_ptr(), count.data_ptr(), skip,
            buffer.data_ptr() if buffer.numel() else None, buffer.numel(), base, base + 8 * (n + 1),
            base + 8 * (n + 1) + 4 * n, dev.index or 0, _stream_ptr(stream, dev)))
    return OrderedPayloads(buffer, buf[:8 * (n + 1)].view(torch.int64), buf[8 * (n + 1):8 * (n + 1) + 4 * n].view(
        torch.int32), count, buf[8 * (n + 1) + 4 * n:].view(torch.int32))


# ------------------------------------------------------------ many peers in one batch
FLOW_NONE = _native.FLOW_NONE             # a datagram without a flow (-1 in the int32 ``flow`` tensor)
FLOWS_MAX_BATCH = _native.FLOWS_MAX_BATCH   # datagrams per accept_flows call: one recvmmsg batch


def flow_states(n_flows: int, device):
    """The zero table of ``n_flows`` fresh flows for ``accept_flows``: int64
    [n_flows, 4] on ``device``, a row {expect, isn, live, last_isn + 1}."""
    import torch
    if isinstance(n_flows, bool) or not isinstance(n_flows, int) or not 1 <= n_flows <= 0xFFFFFFFE:
        raise ValueError(f"n_flows must be an int in [1, 2^32 - 2], got {n_flows!r}")
    return torch.zeros((n_flows, 4), dtype=torch.int64, device=device)


class FlowsAccepted:
    """Result of ``accept_flows``: one device buffer with cut views.
    ``accept``, ``keep``, ``reply`` (u8 [N]), ``reply_ack`` (u16 [N]), ``rank``
    (int32 [N] holding u32 values; -1 is RUDP_RANK_NONE), ``order`` (int32
    [N]), ``order_off`` (int32 [N + 1], of which [0..A] are written),
    ``flow_info`` (int64 [N, 8], A rows written), ``info`` (int64 [8]: A, K, R,
    ended flows, datagrams without a flow, flows walked, 0, 0), ``status``
    (int32 [1]) and ``states`` (the caller's table, updated in place) as
    rudp_accept_flows defines them.  ``active``, ``kept``, ``replies``,
    ``ended``, ``flowless`` and ``flows()`` are read from the device on first
    use, one synchronization for all; ``check()`` reads the status; nothing
    else waits."""

    __slots__ = ("_buf", "_n", "_lay", "_views", "_host", "states")

    def __init__(self, buf, n: int, states):
        self._buf, self._n, self._lay, self.states = buf, n, FlowsAccepted.layout(n), states
        self._views, self._host = {}, None

    @staticmethod
    def layout(n: int):
        """Byte offsets in the one allocation: rank | order (u32 [n]) | order_off
        (u32 [n + 1]) | reply_ack (u16 [n]) | accept | keep | reply (u8 [n]) |
        flow_info (u64 [n][8]) | info (u64 [8]) | status (u32); then the size."""
        lay, at = {}, 0
        for name, nbytes in (("rank", 4 * n), ("order", 4 * n), ("order_off", 4 * (n + 1)), ("reply_ack", 2 * n),
                             ("accept", n), ("keep", n), ("reply", n)):
            lay[name] = at
            at += nbytes
        lay["flow_info"] = (at + 7) & ~7
        lay["info"] = lay["flow_info"] + 64 * n
        lay["status"] = lay["info"] + 64
        lay["size"] = lay["status"] + 8
        return lay

    def _cut(self, name, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    accept = property(lambda self: self._cut("accept", self._n, None))
    keep = property(lambda self: self._cut("keep", self._n, None))
    reply = property(lambda self: self._cut("reply", self._n, None))

    @property
    def reply_ack(self):
        import torch
        return self._cut("reply_ack", 2 * self._n, torch.uint16)

    @property
    def rank(self):
        import torch
        return self._cut("rank", 4 * self._n, torch.int32)

    @property
    def order(self):
        import torch
        return self._cut("order", 4 * self._n, torch.int32)

    @property
    def order_off(self):
        import torch
        return self._cut("order_off", 4 * (self._n + 1), torch.int32)

    @property
    def flow_info(self):
        import torch
        return self._cut("flow_info", 64 * self._n, torch.int64).view(self._n, 8)

    @property
    def info(self):
        import torch
        return self._cut("info", 64, torch.int64)

    @property
    def status(self):
        import torch
        return self._cut("status", 4, torch.int32)

    def _read(self):
        if self._host is None:
            import torch
            lo = self._lay["flow_info"]  # flow_info | info: one copy
            words = self._buf[lo:self._lay["status"]].view(torch.int64).cpu().numpy()
            info = [int(v) for v in words[8 * self._n:]]
            self._host = (info, words[:8 * info[0]].reshape(info[0], 8).copy())
        return self._host

    active = property(lambda self: self._read()[0][0])
    kept = property(lambda self: self._read()[0][1])
    replies = property(lambda self: self._read()[0][2])
    ended = property(lambda self: self._read()[0][3])
    flowless = property(lambda self: self._read()[0][4])

    def flows(self):
        """int64 [A, 8] on the host, ascending by slot: slot, end, accepted,
        msg_start, characters, isn, kept, rank base of every active flow."""
        return self._read()[1]

    def check(self) -> "FlowsAccepted":
        _raise_status(self.status)
        return self

    def __len__(self) -> int:
        return self._n


def _flows_tensor(t, name, dev, dtypes, n=None, ndim=1):
    if not _is_torch(t):
        raise TypeError(f"{name} must be a torch tensor on a HIP device (no host-memory form)")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {'/'.join(map(str, dtypes))}, got {t.dtype}")
    if t.dim() != ndim or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {ndim}-D tensor, got shape {tuple(t.shape)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} has {t.shape[0]} entries, expected {n}")


def accept_flows(seq, flags, chars, flow, *, states, usable=None, stream=None) -> FlowsAccepted:
    """``accept_inorder`` for a batch that carries datagrams of many peers
    (rudp_accept_flows; include/rudp.h states the rule): ``flow`` (int32 [N]
    holding u32 values) names each datagram's row in ``states`` (int64
    [n_flows, 4] from ``flow_states``, updated in place), -1 (``FLOW_NONE``) a
    datagram to ignore.  Every flow is judged by the in-order rule on its own
    datagrams in arrival order, all flows in one launch; a flow whose transfer
    ends turns over to a closed row.  ``seq``, ``flags``, ``chars`` and
    ``usable`` as ``accept_inorder`` takes them; at most ``FLOWS_MAX_BATCH``
    datagrams.  Never waits; ``check()`` on the result raises when a slot was
    out of range."""
    for name, t in (("seq", seq), ("flags", flags), ("chars", chars), ("flow", flow), ("states", states)):
        if not _is_torch(t):
            raise TypeError(f"accept_flows takes torch tensors on a HIP device (no host-memory form): {name}")
    import torch
    dev = seq.device
    if dev.type != "cuda":
        raise ValueError("accept_flows runs on a HIP device")
    _flows_tensor(seq, "seq", dev, (torch.uint16,))
    n = seq.shape[0]
    if n > FLOWS_MAX_BATCH:
        raise ValueError(f"accept_flows takes at most {FLOWS_MAX_BATCH} datagrams (one recvmmsg batch), got {n}")
    _flows_tensor(flags, "flags", dev, (torch.uint8,), n)
    _flows_tensor(chars, "chars", dev, (torch.int32,), n)
    _flows_tensor(flow, "flow", dev, (torch.int32,), n)
    if usable is not None:
        _flows_tensor(usable, "usable", dev, (torch.uint8, torch.bool), n)
    _flows_tensor(states, "states", dev, (torch.int64,), ndim=2)
    if states.shape[1] != 4 or not 1 <= states.shape[0] <= 0xFFFFFFFE:
        raise ValueError(f"states must be int64 [n_flows, 4] with 1 <= n_flows <= 2^32 - 2, got {tuple(states.shape)}")
    lay = FlowsAccepted.layout(n)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(t):
        return t if n else None

    _native.check(_native.lib().rudp_accept_flows(
        tab(seq.data_ptr()), tab(flags.data_ptr()), tab(chars.data_ptr()),
        usable.data_ptr() if usable is not None and n else None, tab(flow.data_ptr()), n, states.data_ptr(),
        states.shape[0], tab(base + lay["accept"]), tab(base + lay["keep"]), tab(base + lay["reply"]),
        tab(base + lay["reply_ack"]), tab(base + lay["rank"]), tab(base + lay["order"]), tab(base + lay["order_off"]),
        tab(base + lay["flow_info"]), base + lay["info"], base + lay["status"], dev.index or 0,
        _stream_ptr(stream, dev)))
    return FlowsAccepted(buf, n, states)


class ReceivedFlows:
    """Result of ``receive_flows``.  ``decoded`` (``VarlenDecoded``: seq, ack,
    flags, ok, valid), ``usable`` (u8 [N]), ``chars`` (int32 [N]), ``accepted``
    (``FlowsAccepted``) and ``pieces`` (``OrderedPayloads``: every active flow's
    part of its message, back to back in flow order).  ``message(a)`` is the
    piece of active flow a (row a of ``accepted.flows()``), as bytes;
    ``reply_index`` (int64 [R]: the datagram each reply answers, and whose
    source it goes to), ``reply_ack`` (u16 [R]) and ``reply_frames(layout)``
    as ``ReceivedWindow`` has them.  The host reads wait once each, on first
    use."""

    __slots__ = ("decoded", "usable", "chars", "accepted", "pieces", "_bytes", "_reply")

    def __init__(self, decoded, usable, chars, accepted, pieces):
        self.decoded, self.usable, self.chars, self.accepted, self.pieces = decoded, usable, chars, accepted, pieces
        self._bytes, self._reply = None, None

    def message(self, a: int) -> bytes:
        rows = self.accepted.flows()
        if self._bytes is None:
            K = self.accepted.kept
            off = self.pieces.out_off[:K + 1].cpu().numpy()
            self._bytes = (off, self.pieces.buffer[:int(off[K])].cpu().numpy().tobytes() if K else b"")
        off, data = self._bytes
        base, kept = int(rows[a][7]), int(rows[a][6])
        return data[int(off[base]):int(off[base + kept])] if kept else b""

    def _replies(self):
        if self._reply is None:
            import torch
            idx = torch.nonzero(self.accepted.reply).flatten()
            self._reply = (idx, self.accepted.reply_ack.view(torch.int16)[idx].view(torch.uint16))
        return self._reply

    reply_index = property(lambda self: self._replies()[0])
    reply_ack = property(lambda self: self._replies()[1])
    reply_count = property(lambda self: int(self._replies()[0].shape[0]))

    def reply_frames(self, layout: Union[str, int] = "rudp7"):
        """u8 [R * H]: the reply datagrams, header-only frames at stride H in
        arrival order (seq 0, ack = reply_ack, flags ACK)."""
        import torch
        ack = self.reply_ack
        R = ack.shape[0]
        empty = torch.empty(0, dtype=torch.uint8, device=ack.device)
        if R == 0:
            return empty
        tab = (torch.zeros_like(ack), ack, torch.full((R,), ACK, dtype=torch.uint8, device=ack.device))
        return pack_batch_varlen(tab, empty, torch.zeros(R, dtype=torch.int32, device=ack.device), layout,
                                 want_csum=False, check=False).frames


def receive_flows(frames, frame_off, flow, layout: Union[str, int] = "rudp7", *, states, csum=None,
                  stream=None) -> ReceivedFlows:
    """``receive_batch`` for a batch that carries datagrams of many peers, with
    no host wait in between: ``unpack_batch_varlen(utf8=True)`` -> ``keep_mask``
    -> ``payload_chars`` -> ``accept_flows`` -> ``gather_ordered`` (rank, K,
    skip = the header), which leaves every active flow's message piece back to
    back.  ``flow`` and ``states`` as ``accept_flows`` takes them; ``csum``:
    the rudp5 sideband."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off) or not _is_torch(flow):
        raise TypeError("receive_flows takes torch tensors on a HIP device (no host-memory form)")
    import torch
    if frame_off.dim() != 1 or frame_off.shape[0] < 1:
        raise ValueError("frame_off needs N + 1 entries")
    if frame_off.shape[0] - 1 > FLOWS_MAX_BATCH:
        raise ValueError(f"receive_flows takes at most {FLOWS_MAX_BATCH} datagrams (one recvmmsg batch), "
                         f"got {frame_off.shape[0] - 1}")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        dec = unpack_batch_varlen(frames, frame_off, H, csum=csum, check=False, utf8=True)
        usable = keep_mask(dec, unverified=H == 5 and csum is None)
        chars = payload_chars(frames, frame_off, H)
        acc = accept_flows(dec.seq, dec.flags, chars, flow, states=states, usable=usable)
        pieces = gather_ordered(frames, frame_off, acc.rank, acc.info[1:2], skip=H)
    return ReceivedFlows(dec, usable, chars, acc, pieces)


# The geometry of csrc/receive_flows.hip (tests/test_receive_flows_api.py holds these to the source).
FLOWS_FUSED_BYTES = 32768   # rudp_receive_flows: a batch in at most this many bytes ...
FLOWS_FUSED_MEAN = 133      # ... and this many per datagram is one launch of one workgroup
_ST_FLOWS_FUSED = (_ST_ORDERED[0], _ST_MESSAGES[-1], _ST_ORDERED[2])  # offsets, flow slot, payload_cap


class ReceivedFlowsFused:
    """Result of ``receive_flows_fused``: one allocation, every member a view
    of it, on the device.

    Per datagram (N entries): ``seq``, ``ack``, ``csum``, ``reply_ack`` (u16),
    ``flags``, ``ok``, ``valid``, ``usable``, ``accept``, ``keep``, ``reply``
    (u8), ``chars`` (int32) and ``rank``, ``order`` (int32 holding u32 values)
    as ``receive_flows`` returns them; ``order_off`` (int32 [N + 1]),
    ``flow_info`` (int64 [N, 8]), ``payload`` (u8 [payload_cap]),
    ``payload_off`` (int64 [N + 1]), ``payload_src`` (int32 [N]), ``info``
    (int64 [12]: A, K, R, ended flows, datagrams without a flow, flows walked,
    0, 0, message bytes, 0, 0, 0), ``status`` (int32 [1]) and ``states`` (the
    caller's table, updated in place).  These never wait.

    ``reply_frames`` (u8 [R * H]), ``reply_csum`` (u16 [R]), ``reply_index``
    (int32 [R]: the datagram each reply answers, and whose source it goes to),
    ``fin_frames`` (u8 [E * H]: the closing FIN|ACK of every flow that ended),
    ``fin_csum`` (u16 [E]) and ``fin_flow`` (int32 [E]: its row of ``flows()``)
    are cut to their counts.  They, ``active``, ``kept``, ``replies``,
    ``ended``, ``flowless``, ``message_bytes``, ``flows()``, ``message(a)``,
    ``host(name)`` (any table as a numpy array) and ``check()`` read the
    device: one copy of the allocation, one synchronization, on first use."""

    __slots__ = ("_buf", "_n", "_H", "_cap", "_lay", "_views", "_host", "states")
    _TABLES = {  # name: (bytes per datagram, bytes on top, torch dtype name, numpy dtype)
        "payload_off": (8, 8, "int64", np.int64), "flow_info": (64, 0, "int64", np.int64),
        "info": (0, 96, "int64", np.int64), "status": (0, 8, "int32", np.int32),
        "rank": (4, 0, "int32", np.int32), "order": (4, 0, "int32", np.int32),
        "order_off": (4, 4, "int32", np.int32), "chars": (4, 0, "int32", np.int32),
        "payload_src": (4, 0, "int32", np.int32), "reply_index": (4, 0, "int32", np.int32),
        "fin_flow": (4, 0, "int32", np.int32),
        "seq": (2, 0, "uint16", np.uint16), "ack": (2, 0, "uint16", np.uint16), "csum": (2, 0, "uint16", np.uint16),
        "reply_ack": (2, 0, "uint16", np.uint16), "reply_csum": (2, 0, "uint16", np.uint16),
        "fin_csum": (2, 0, "uint16", np.uint16),
        "flags": (1, 0, "uint8", np.uint8), "ok": (1, 0, "uint8", np.uint8), "valid": (1, 0, "uint8", np.uint8),
        "usable": (1, 0, "uint8", np.uint8), "accept": (1, 0, "uint8", np.uint8), "keep": (1, 0, "uint8", np.uint8),
        "reply": (1, 0, "uint8", np.uint8),
    }

    def __init__(self, buf, n: int, H: int, cap: int, states):
        self._buf, self._n, self._H, self._cap, self.states = buf, n, H, cap, states
        self._lay = ReceivedFlowsFused.layout(n, H, cap)
        self._views, self._host = {}, None

    @staticmethod
    def layout(n: int, H: int, cap: int):
        """name -> (byte offset, bytes) in the one allocation, every array
        aligned to its element (the payload to 16 bytes); ``size`` is the
        allocation's."""
        lay, at = {}, 0
        for name, (per, top, _, _) in ReceivedFlowsFused._TABLES.items():
            lay[name] = (at, per * n + top)
            at += per * n + top
        for name in ("reply_frames", "fin_frames"):
            lay[name] = (at, n * H)
            at += n * H
        lay["payload"] = ((at + 15) & ~15, cap)
        lay["size"] = lay["payload"][0] + cap
        return lay

    def _cut(self, name):
        v = self._views.get(name)
        if v is None:
            import torch
            lo, nbytes = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            spec = ReceivedFlowsFused._TABLES.get(name)
            if spec is not None:
                v = v.view(getattr(torch, spec[2]))
            if name == "flow_info":
                v = v.view(self._n, 8)
            elif name == "status":
                v = v[:1]
            self._views[name] = v
        return v

    def __getattr__(self, name):
        if name in ReceivedFlowsFused._TABLES or name == "payload":
            return self._cut(name)
        raise AttributeError(name)

    def _read(self):
        if self._host is None:
            whole = self._buf.cpu().numpy()
            h = {}
            for name, span in self._lay.items():
                if name == "size":
                    continue
                lo, nbytes = span
                spec = ReceivedFlowsFused._TABLES.get(name)
                h[name] = whole[lo:lo + nbytes].view(spec[3] if spec else np.uint8)
            h["flow_info"] = h["flow_info"].reshape(self._n, 8)
            h["info"] = [int(v) for v in h["info"]]
            self._host = h
        return self._host

    def host(self, name: str):
        """Table ``name`` on the host (numpy, whole), from the one copy."""
        return self._read()[name]

    active = property(lambda self: self._read()["info"][0])
    kept = property(lambda self: self._read()["info"][1])
    replies = property(lambda self: self._read()["info"][2])
    ended = property(lambda self: self._read()["info"][3])
    flowless = property(lambda self: self._read()["info"][4])
    message_bytes = property(lambda self: self._read()["info"][8])
    reply_frames = property(lambda self: self._cut("reply_frames")[:self.replies * self._H])
    reply_csum = property(lambda self: self._cut("reply_csum")[:self.replies])
    reply_index = property(lambda self: self._cut("reply_index")[:self.replies])
    fin_frames = property(lambda self: self._cut("fin_frames")[:self.ended * self._H])
    fin_csum = property(lambda self: self._cut("fin_csum")[:self.ended])
    fin_flow = property(lambda self: self._cut("fin_flow")[:self.ended])

    def flows(self):
        """int64 [A, 8] on the host, ascending by slot: slot, end, accepted,
        msg_start, characters, isn, kept, rank base of every active flow."""
        return self._read()["flow_info"][:self.active]

    def message(self, a: int) -> bytes:
        """The message piece of active flow ``a`` (row a of ``flows()``)."""
        h = self._read()
        base, kept = int(h["flow_info"][a][7]), int(h["flow_info"][a][6])
        if not kept or self.message_bytes > self._cap:
            return b""
        off = h["payload_off"]
        return h["payload"][int(off[base]):int(off[base + kept])].tobytes()

    def check(self) -> "ReceivedFlowsFused":
        """Raise ValueError if the device rejected a frame's offsets or a flow
        slot, or the message did not fit."""
        bits = int(self._read()["status"][0]) if self._n else 0
        if bits:
            msgs = [m for b, m in _ST_FLOWS_FUSED if bits & b] or [f"status {bits:#x}"]
            if bits & _native.ST_PAYLOAD_CAP:
                msgs.append(f"{self.message_bytes} bytes are needed, payload has {self._cap}")
            raise ValueError("; ".join(msgs))
        return self

    def __len__(self) -> int:
        return self._n


def receive_flows_fused(frames, frame_off, flow, layout: Union[str, int] = "rudp7", *, states, csum=None,
                        payload_cap=None, out=None, stream=None) -> ReceivedFlowsFused:
    """``receive_flows``, the reply datagrams and the closing datagrams in one
    library call (rudp_receive_flows; include/rudp.h states the contract), with
    no torch operation in between.  A batch in at most ``FLOWS_FUSED_BYTES``
    bytes (and ``FLOWS_FUSED_MEAN`` per datagram) is one kernel launch.

    ``frames``, ``frame_off``, ``flow``, ``states`` and ``csum`` as
    ``receive_flows`` takes them.  ``payload_cap``: bytes for the message
    pieces (None: ``frames.numel()``, which always suffices).  ``out``: an
    earlier result whose allocation is taken over when it is large enough.
    Never waits; every table equals what ``receive_flows`` returns for the
    same input."""
    H = layout_header_len(layout)
    for name, t in (("frames", frames), ("frame_off", frame_off), ("flow", flow), ("states", states)):
        if not _is_torch(t):
            raise TypeError(f"receive_flows_fused takes torch tensors on a HIP device (no host-memory form): {name}")
    import torch
    if out is not None and not isinstance(out, ReceivedFlowsFused):
        raise TypeError("out must be an earlier receive_flows_fused result")
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("receive_flows_fused runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if n > FLOWS_MAX_BATCH:
        raise ValueError(f"receive_flows_fused takes at most {FLOWS_MAX_BATCH} datagrams (one recvmmsg batch), got {n}")
    _flows_tensor(flow, "flow", dev, (torch.int32,), n)
    _flows_tensor(states, "states", dev, (torch.int64,), ndim=2)
    if states.shape[1] != 4 or not 1 <= states.shape[0] <= 0xFFFFFFFE:
        raise ValueError(f"states must be int64 [n_flows, 4] with 1 <= n_flows <= 2^32 - 2, got {tuple(states.shape)}")
    if csum is not None:
        if H == 7:
            raise ValueError("rudp7 carries its checksum in-band; csum is for rudp5")
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    fbytes = frames.numel()
    cap = fbytes if payload_cap is None else payload_cap
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 0:
        raise ValueError(f"payload_cap must be a non-negative int, got {payload_cap!r}")
    lay = ReceivedFlowsFused.layout(n, H, cap)
    if out is not None and out._buf.numel() >= lay["size"] and out._buf.device == dev:
        buf = out._buf
    else:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            buf = (torch.empty if n else torch.zeros)(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(name, need=n):
        return base + lay[name][0] if need else None

    res = _native.RudpReceivedFlows(
        seq=tab("seq"), ack=tab("ack"), flags=tab("flags"), ok=tab("ok"), csum_out=tab("csum"), valid=tab("valid"),
        usable=tab("usable"), chars=tab("chars"), accept=tab("accept"), keep=tab("keep"), reply=tab("reply"),
        reply_ack=tab("reply_ack"), rank=tab("rank"), order=tab("order"), order_off=tab("order_off"),
        flow_info=tab("flow_info"), payload=tab("payload", cap), payload_cap=cap, payload_off=tab("payload_off"),
        payload_src=tab("payload_src"), reply_frames=tab("reply_frames"), reply_csum=tab("reply_csum"),
        reply_index=tab("reply_index"), fin_frames=tab("fin_frames"), fin_csum=tab("fin_csum"),
        fin_flow=tab("fin_flow"), info=base + lay["info"][0], status=base + lay["status"][0])
    _native.check(_native.lib().rudp_receive_flows(
        frames.data_ptr() if fbytes else None, fbytes, frame_off.data_ptr(), min(fbytes // n, 0xFFFFFFFF) if n else 0,
        n, csum.data_ptr() if csum is not None and n else None, flow.data_ptr() if n else None, states.data_ptr(),
        states.shape[0], ctypes.byref(res), H, dev.index or 0, _stream_ptr(stream, dev)))
    return ReceivedFlowsFused(buf, n, H, cap, states)


class CarriedFrames:
    """The frames a ``receive_window`` call left pending, whole, on the device:
    pass it as ``carried=`` of the next call.  ``frames`` (u8) and ``frame_off``
    (int64) are ``gather_ordered``'s output with ``skip=0``; ``csum`` the
    sideband checksums in the same order (None without one).  ``count`` and
    ``nbytes`` read the device once."""

    __slots__ = ("_ordered", "_csum_all")

    def __init__(self, ordered: OrderedPayloads, csum_all=None):
        self._ordered, self._csum_all = ordered, csum_all

    count = property(lambda self: self._ordered.total[0])
    nbytes = property(lambda self: self._ordered.total[1])

    @property
    def frames(self):
        return self._ordered.buffer[:self.nbytes]

    @property
    def frame_off(self):
        return self._ordered.out_off[:self.count + 1]

    @property
    def csum(self):
        if self._csum_all is None:
            return None
        import torch
        pick = self._ordered.src[:self.count].long()
        return self._csum_all.view(torch.int16)[pick].view(torch.uint16)  # (u16 is indexed through its i16 view)


class ReceivedWindow:
    """Result of ``receive_window``.  ``message`` (``OrderedPayloads``: its
    ``payload`` is this call's part of the message in delivery order),
    ``accepted`` (``WindowAccepted`` over carried ++ new frames), ``carried``
    (``CarriedFrames`` for the next call), ``state`` (for the next call's
    ``state=``), ``n_carried`` and ``n_new``.  Replies, counted in new-frame
    indices: ``replies`` (``HeaderTable`` of n_new rows for ``pack_batch``:
    seq 0, ack = reply_ack, flags ACK where a reply is sent), and on first use
    (one synchronization) ``reply_index`` (int64 [R]: the new frame each reply
    answers), ``reply_ack`` (u16 [R]) and ``reply_peer`` (int64 [R]: the new
    frame whose source the reply goes to, the last reset at or before it;
    n_new = the peer carried from earlier batches)."""

    __slots__ = ("message", "accepted", "carried", "replies", "n_carried", "n_new", "_reset", "_reply")

    def __init__(self, message, accepted, carried, replies, n_carried, n_new, reset):
        self.message, self.accepted, self.carried, self.replies = message, accepted, carried, replies
        self.n_carried, self.n_new, self._reset, self._reply = n_carried, n_new, reset, None

    state = property(lambda self: self.accepted.state)

    def _replies(self):
        if self._reply is None:
            import torch
            m, n = self.n_carried, self.n_new
            idx = torch.nonzero(self.accepted.reply[m:]).flatten()
            pos = torch.arange(n, device=idx.device)
            last = torch.cummax(torch.where(self._reset, pos, torch.full_like(pos, -1)), 0).values if n else pos
            peer = last[idx]
            ack = self.accepted.reply_ack[m:].view(torch.int16)[idx].view(torch.uint16)
            self._reply = (idx, ack, torch.where(peer < 0, torch.full_like(peer, n), peer))
        return self._reply

    def reply_frames(self, layout: Union[str, int] = "rudp7"):
        """u8 [R * H]: the reply datagrams, header-only frames at stride H in
        arrival order (``pack_batch_varlen`` of seq 0, ack = reply_ack, flags
        ACK with empty payloads)."""
        import torch
        ack = self.reply_ack
        R = ack.shape[0]
        tab = (torch.zeros_like(ack), ack, torch.full((R,), ACK, dtype=torch.uint8, device=ack.device))
        empty = torch.empty(0, dtype=torch.uint8, device=ack.device)
        if R == 0:
            return empty
        return pack_batch_varlen(tab, empty, torch.zeros(R, dtype=torch.int32, device=ack.device), layout,
                                 want_csum=False, check=False).frames

    reply_index = property(lambda self: self._replies()[0])
    reply_ack = property(lambda self: self._replies()[1])
    reply_peer = property(lambda self: self._replies()[2])
    reply_count = property(lambda self: int(self._replies()[0].shape[0]))


def receive_window(frames, frame_off, layout: Union[str, int] = "rudp7", *, window_chars, carried=None, csum=None,
                   state=None, last_isn=None, stream=None) -> ReceivedWindow:
    """``receive_batch`` for a windowed sender: the batch of new datagrams,
    behind the frames the previous call left pending (``carried``: that call's
    ``ReceivedWindow.carried``; None: none), decoded, judged by
    ``accept_window`` and gathered in delivery order, with the pending frames
    gathered whole for the next call: ``unpack_batch_varlen(utf8=True)`` over
    carried ++ new -> ``keep_mask`` -> ``payload_chars`` -> ``accept_window``
    -> ``gather_ordered`` (rank, skip = the header) -> ``gather_ordered``
    (carry_rank, skip 0).  Reading ``carried``'s size is the one wait before
    the call; none follows.  ``csum``: the rudp5 sideband of the new frames."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("receive_window takes torch tensors on a HIP device (no host-memory form)")
    import torch
    Wc = _check_window(window_chars)
    last = _check_last_isn(last_isn)
    if carried is not None and not isinstance(carried, CarriedFrames):
        raise TypeError("carried must be the `carried` of an earlier receive_window result")
    dev = frames.device
    n_new = frame_off.shape[0] - 1
    if n_new < 0:
        raise ValueError("frame_off needs N + 1 entries")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        m = carried.count if carried is not None else 0
        if m and (csum is None) != (carried.csum is None):
            raise ValueError("csum must be given in every call of a transfer or in none")
        if m:
            all_frames = torch.cat((carried.frames, frames))
            all_off = torch.cat((carried.frame_off, frame_off[1:] - frame_off[0] + carried.nbytes))
            all_csum = (torch.cat((carried.csum.view(torch.int16), csum.view(torch.int16))).view(torch.uint16)
                        if csum is not None else None)
        else:
            all_frames, all_off, all_csum = frames, frame_off, csum
        dec = unpack_batch_varlen(all_frames, all_off, H, csum=all_csum, check=False, utf8=True)
        usable = keep_mask(dec, unverified=H == 5 and csum is None)
        chars = payload_chars(all_frames, all_off, H)
        acc = accept_window(dec.seq, dec.flags, chars, window_chars=Wc, carried=m, usable=usable, state=state,
                            last_isn=last)
        msg = gather_ordered(all_frames, all_off, acc.rank, acc.info[1:2], skip=H)
        car = gather_ordered(all_frames, all_off, acc.carry_rank, acc.info[5:6], skip=0)
        ack = acc.reply_ack[m:]
        replies = HeaderTable(torch.zeros_like(ack), ack, acc.reply[m:] * ACK)
        seq64 = dec.seq.view(torch.int16)[m:].to(torch.int64) & 0xFFFF
        reset = (usable[m:] != 0) & ((dec.flags[m:] & SYN) != 0) & (seq64 != last)
    return ReceivedWindow(msg, acc, CarriedFrames(car, all_csum), replies, m, n_new, reset)


# The geometry of csrc/receive_window.hip (tests/test_receive_window_api.py holds these to the source).
WINDOW_FUSED_BYTES = 32768  # rudp_receive_window: at most WINDOW_CHUNK new datagrams, this many bytes in both buffers ...
WINDOW_FUSED_MEAN = 1005    # ... and this many per frame is one launch of one workgroup
WINDOW_CARRY_MAX = WINDOW_MAX - 1   # the most frames a call leaves pending

_ST_WINDOWED = ((_native.ST_OFFSETS, "a frame's offsets are decreasing or outside its buffer"),
                (_native.ST_PAYLOAD_CAP, "the message does not fit the payload buffer"),
                (_native.ST_CARRY_CAP, "the pending frames do not fit the carry buffer"))


class CarriedWindowed:
    """The frames a ``receive_windowed`` call left pending, whole, on the
    device: pass it as ``carried=`` of the next call.  ``frames`` (u8, the
    carry buffer), ``frame_off`` (int64 [1024]) and ``csum`` (u16 [1023], None
    without a sideband) are views of that call's allocation and go to the
    library as they are; ``count`` and ``nbytes`` come from the call's ``info``,
    read from the device once for the whole result, on first use."""

    __slots__ = ("_owner",)

    def __init__(self, owner):
        self._owner = owner

    count = property(lambda self: self._owner._host_info()[5])
    nbytes = property(lambda self: self._owner._host_info()[10])
    frames = property(lambda self: self._owner._cut("carry", self._owner._ccap, None))

    @property
    def frame_off(self):
        import torch
        return self._owner._cut("carry_off", 8 * WINDOW_MAX, torch.int64)

    @property
    def csum(self):
        import torch
        return self._owner._cut("carry_csum", 2 * WINDOW_CARRY_MAX, torch.uint16) if self._owner._side else None


class ReceivedWindowed:
    """Result of ``receive_windowed``: one allocation, every member a view of it.

    Over the N = n_carried + n_new items (the carried frames first): ``seq``,
    ``ack``, ``csum`` (u16 [N]), ``flags``, ``ok``, ``valid``, ``usable`` (u8
    [N]) and ``chars`` (int32 [N]) as ``receive`` returns them; ``accepted``
    (a ``WindowAccepted``: accept, rank, carry_rank, reply, reply_ack, state,
    info and its host reads); ``message`` (an ``OrderedPayloads``: this call's
    part of the message in delivery order); ``carried`` (for the next call's
    ``carried=``); ``state`` (for its ``state=``); ``info`` (int64 [12]) and
    ``status`` (int32 [1]) on the device.  Replies, with ``ReceivedWindow``'s
    meaning, counted in new-frame indices: ``reply_frames`` (u8 [R * H], the
    datagrams at stride H in arrival order), ``reply_csum`` (u16 [R]),
    ``reply_index`` (int64 [R]), ``reply_ack`` (u16 [R]) and ``reply_peer``
    (int64 [R]; n_new = the peer carried from earlier batches).
    ``reply_count``, ``message_bytes``, the host reads of ``accepted``,
    ``message.total`` and ``carried.count`` / ``.nbytes`` share one read of
    ``info``: one synchronization, on first use; nothing else waits."""

    __slots__ = ("_buf", "_lay", "_views", "_info", "_H", "_side", "_mcap", "_ccap", "n_carried", "n_new",
                 "accepted", "message", "carried")

    def __init__(self, buf, n_carried: int, n_new: int, H: int, mcap: int, ccap: int, side: bool):
        import torch
        n = n_carried + n_new
        self._buf, self._lay = buf, ReceivedWindowed.layout(n, n_new, H, mcap, ccap)
        self._views, self._info, self._H, self._side, self._mcap, self._ccap = {}, None, H, side, mcap, ccap
        self.n_carried, self.n_new = n_carried, n_new
        self.accepted = WindowAccepted(buf, n)
        self.accepted._lay = self._lay  # (the same names, this allocation's places)
        self.message = OrderedPayloads(self._cut("payload", mcap, None),
                                       self._cut("payload_off", 8 * (n + 1), torch.int64),
                                       self._cut("payload_src", 4 * n, torch.int32), self.info[1:2], self.status)
        self.carried = CarriedWindowed(self)

    @staticmethod
    def layout(n: int, n_new: int, H: int, mcap: int, ccap: int):
        """Byte offsets in the one allocation, every array aligned to its
        element (the two byte buffers to 16 bytes); ``size`` is the allocation's."""
        lay, at = {}, 0
        for name, nbytes in (("payload_off", 8 * (n + 1)), ("carry_off", 8 * WINDOW_MAX), ("reply_peer", 8 * n_new),
                             ("state", 32), ("info", 96), ("status", 8),
                             ("rank", 4 * n), ("carry_rank", 4 * n), ("chars", 4 * n), ("payload_src", 4 * n),
                             ("reply_index", 4 * n_new),
                             ("seq", 2 * n), ("ack", 2 * n), ("csum", 2 * n), ("reply_ack", 2 * n),
                             ("reply_csum", 2 * n_new), ("carry_csum", 2 * WINDOW_MAX),
                             ("flags", n), ("ok", n), ("valid", n), ("usable", n), ("accept", n), ("reply", n),
                             ("reply_frames", n_new * H)):
            lay[name] = at
            at += nbytes
        lay["payload"] = (at + 15) & ~15
        lay["carry"] = (lay["payload"] + mcap + 15) & ~15
        lay["size"] = lay["carry"] + ccap
        return lay

    def _cut(self, name, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    def _u16(self, name):
        import torch
        return self._cut(name, 2 * len(self), torch.uint16)

    seq = property(lambda self: self._u16("seq"))
    ack = property(lambda self: self._u16("ack"))
    csum = property(lambda self: self._u16("csum"))
    flags = property(lambda self: self._cut("flags", len(self), None))
    ok = property(lambda self: self._cut("ok", len(self), None))
    valid = property(lambda self: self._cut("valid", len(self), None))
    usable = property(lambda self: self._cut("usable", len(self), None))
    state = property(lambda self: self.accepted.state)

    @property
    def chars(self):
        import torch
        return self._cut("chars", 4 * len(self), torch.int32)

    @property
    def info(self):
        """int64 [12] on the device: [0..7] as ``WindowAccepted.info``, then
        reply_count, message_bytes, carried bytes, 0."""
        import torch
        return self._cut("info", 96, torch.int64)

    @property
    def status(self):
        import torch
        return self._cut("status", 4, torch.int32)

    def _host_info(self):
        if self._info is None:
            self._info = [int(v) for v in self.info.tolist()]
            self.accepted._info = self._info[:8]
            self.message._total = (self._info[1], self._info[9])
        return self._info

    reply_count = property(lambda self: self._host_info()[8])
    message_bytes = property(lambda self: self._host_info()[9])

    @property
    def reply_frames(self):
        return self._cut("reply_frames", self.n_new * self._H, None)[:self.reply_count * self._H]

    @property
    def reply_csum(self):
        import torch
        return self._cut("reply_csum", 2 * self.n_new, torch.uint16)[:self.reply_count]

    @property
    def reply_index(self):
        import torch
        return self._cut("reply_index", 4 * self.n_new, torch.int32)[:self.reply_count].long() - self.n_carried

    @property
    def reply_ack(self):
        import torch
        idx = self.reply_index + self.n_carried
        return self.accepted.reply_ack.view(torch.int16)[idx].view(torch.uint16)  # (u16 is indexed through its i16 view)

    @property
    def reply_peer(self):
        import torch
        peer = self._cut("reply_peer", 8 * self.n_new, torch.int64)[:self.reply_count]
        return torch.where(peer >= len(self), torch.full_like(peer, self.n_new), peer - self.n_carried)

    def check(self) -> "ReceivedWindowed":
        """Raise ValueError if the device rejected a frame's offsets, or the
        message or the pending frames did not fit; one synchronization."""
        bits = int(self.status.item())
        if bits:
            msgs = [m for b, m in _ST_WINDOWED if bits & b] or [f"status {bits:#x}"]
            raise ValueError("; ".join(msgs))
        return self

    def __len__(self) -> int:
        return self.n_carried + self.n_new


def receive_windowed(frames, frame_off, layout: Union[str, int] = "rudp7", *, window_chars, carried=None, csum=None,
                     state=None, last_isn=None, out=None, stream=None) -> ReceivedWindowed:
    """``receive_window`` and the reply datagrams in one library call
    (rudp_receive_window): the new datagrams judged behind the frames the
    previous call left pending, this call's part of the message gathered in
    delivery order, the frames still pending gathered whole for the next call,
    and the cumulative replies built for ``sendmmsg``, with no torch operation
    in between: the carried and the new frames go to the library as two
    buffers.  At most ``WINDOW_CHUNK`` new datagrams with at most
    ``WINDOW_FUSED_BYTES`` bytes in both buffers (and ``WINDOW_FUSED_MEAN``
    per frame) are one kernel launch.

    ``frames``, ``frame_off``, ``csum``, ``state`` and ``last_isn`` as
    ``receive`` takes them; ``window_chars`` as ``accept_window``; ``carried``:
    the previous result's ``carried`` (None: none), whose ``count`` and
    ``nbytes`` are that result's one host read.  ``out``: an earlier result
    whose allocation is taken over when it is large enough (not the one
    ``carried`` belongs to: callers ping-pong two).  Every array equals what
    ``receive_window`` returns for the same input."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("receive_windowed takes torch tensors on a HIP device (no host-memory form)")
    import torch
    Wc = _check_window(window_chars)
    last = _check_last_isn(last_isn)
    if carried is not None and not isinstance(carried, CarriedWindowed):
        raise TypeError("carried must be the `carried` of an earlier receive_windowed result")
    if out is not None and not isinstance(out, ReceivedWindowed):
        raise TypeError("out must be an earlier receive_windowed result")
    if out is not None and carried is not None and out is carried._owner:
        raise ValueError("out is the result `carried` belongs to: its frames would be overwritten")
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("receive_windowed runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n_new = frame_off.shape[0] - 1
    if n_new < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if csum is not None:
        if H == 7:
            raise ValueError("rudp7 carries its checksum in-band; csum is for rudp5")
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n_new:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n_new} frames")
    m = carried.count if carried is not None else 0
    cbytes = carried.nbytes if m else 0
    if m and (csum is None) != (carried.csum is None):
        raise ValueError("csum must be given in every call of a transfer or in none")
    st = _accept_state(state, dev)
    n, fbytes = m + n_new, frames.numel()
    cap = fbytes + cbytes  # the message and the pending frames each fit in what came in
    lay = ReceivedWindowed.layout(n, n_new, H, cap, cap)
    if out is not None and out._buf.numel() >= lay["size"] and out._buf.device == dev:
        buf = out._buf
    else:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            buf = (torch.empty if n else torch.zeros)(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(name, need=n):
        return base + lay[name] if need else None

    res = _native.RudpReceivedWindow(
        seq=tab("seq"), ack=tab("ack"), flags=tab("flags"), ok=tab("ok"), csum_out=tab("csum"), valid=tab("valid"),
        usable=tab("usable"), chars=tab("chars"), accept=tab("accept"), rank=tab("rank"),
        carry_rank=tab("carry_rank"), reply=tab("reply"), reply_ack=tab("reply_ack"), state_out=base + lay["state"],
        payload=tab("payload", cap), payload_cap=cap, payload_off=tab("payload_off"), payload_src=tab("payload_src"),
        carry_frames=tab("carry", cap), carry_cap=cap, carry_off=base + lay["carry_off"],
        carry_csum=tab("carry_csum", csum is not None), reply_frames=tab("reply_frames", n_new),
        reply_csum=tab("reply_csum", n_new), reply_index=tab("reply_index", n_new),
        reply_peer=tab("reply_peer", n_new), info=base + lay["info"], status=base + lay["status"])
    side = csum is not None
    _native.check(_native.lib().rudp_receive_window(
        carried.frames.data_ptr() if cbytes else None, cbytes, carried.frame_off.data_ptr() if m else None,
        carried.csum.data_ptr() if m and side else None, m,
        frames.data_ptr() if fbytes else None, fbytes, frame_off.data_ptr(),
        (csum.data_ptr() if n_new else carried.csum.data_ptr()) if side and n else None, n_new,
        min(cap // n, 0xFFFFFFFF) if n else 0, last, Wc, st.data_ptr(), ctypes.byref(res), H, dev.index or 0,
        _stream_ptr(stream, dev)))
    return ReceivedWindowed(buf, m, n_new, H, cap, cap, side)


# ------------------------------------------------------------ replies -> sender state
# The geometry of csrc/acknowledge.hip (tests/test_ack_api.py holds these to the source).
ACK_TILE = 1024            # replies per tile of rudp_ack_progress; a batch up to one tile is one launch
ACK_FUSED_BYTES = 32768    # rudp_acknowledge: a batch of at most ACK_TILE replies in at most this many bytes ...
ACK_FUSED_MEAN = 261       # ... and this many per reply is one launch of one workgroup
ACK_MODES = {"exact": _native.ACK_EXACT, "cumulative": _native.ACK_CUMULATIVE}


def fresh_ack_state(total_chars: int, chunk: int = 1):
    """(p, L, last, done) at the start of a ``send()``: nothing acknowledged, the
    first frame outstanding."""
    first = min(chunk, total_chars)
    return 0, first, int(first == total_chars), 0


class _AckResult:
    """What ``AckProgress`` and ``Acknowledged`` share: views of the one
    allocation by name, and the host reads of ``info`` (one synchronization on
    first use, cached)."""

    __slots__ = ("_buf", "_n", "_lay", "_views", "_info")

    def _cut(self, name, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    valid = property(lambda self: self._cut("valid", self._n, None))

    @property
    def pointer(self):
        import torch
        return self._cut("pointer", 8 * self._n, torch.int64)

    @property
    def state(self):
        """int64 [4] on the device: p, L, last, done after the call; pass it as
        ``state=`` of the next call."""
        import torch
        return self._cut("state", 32, torch.int64)

    @property
    def info(self):
        """int64 [8] on the device: end, valid replies, newly acknowledged
        characters, p after, first_anomaly, next frame, done, 0."""
        import torch
        return self._cut("info", 64, torch.int64)

    def _host_info(self):
        if self._info is None:
            self._info = [int(v) for v in self.info.tolist()]
        return self._info

    end = property(lambda self: self._host_info()[0])
    count = property(lambda self: self._host_info()[1])
    newly_acknowledged = property(lambda self: self._host_info()[2])
    pointer_after = property(lambda self: self._host_info()[3])
    first_anomaly = property(lambda self: self._host_info()[4])
    next_frame = property(lambda self: self._host_info()[5])
    done = property(lambda self: bool(self._host_info()[6]))
    fast = property(lambda self: self._host_info()[4] == self._n)

    def __len__(self) -> int:
        return self._n


class AckProgress(_AckResult):
    """Result of ``ack_progress``: ``valid`` (u8 [N]) and ``pointer`` (int64
    [N], the characters acknowledged after each reply) as rudp_ack_progress
    defines them, ``state`` (int64 [4] on the device, for the next call's
    ``state=``) and ``info``.  ``end`` (N when no valid reply had FIN),
    ``count`` (valid replies), ``newly_acknowledged``, ``pointer_after``,
    ``first_anomaly``, ``fast`` (the one-scan form was exact), ``next_frame``
    (the row of ``segment_message``'s table to send next) and ``done`` are read
    from the device on first use, one synchronization for all; nothing else
    waits."""

    __slots__ = ()

    def __init__(self, buf, n: int):
        self._buf, self._n, self._lay = buf, n, AckProgress.layout(n)
        self._views, self._info = {}, None

    @staticmethod
    def layout(n: int):
        """Byte offsets in the one allocation: pointer (u64 [n]) | state (u64
        [4]) | info (u64 [8]) | valid (u8 [n]); ``size`` is the allocation's."""
        return {"pointer": 0, "state": 8 * n, "info": 8 * n + 32, "valid": 8 * n + 96, "size": 9 * n + 96}


def _ack_scalars(isn, total_chars, chunk, mode, sent):
    for name, v in (("isn", isn), ("total_chars", total_chars), ("chunk", chunk)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    if isn > 0xFFFF:
        raise ValueError(f"isn must be at most 65535, got {isn}")
    chunk = _check_chunk(chunk)
    try:
        m = ACK_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"mode must be 'exact' or 'cumulative', got {mode!r}") from None
    if sent is None:
        sent = total_chars
    if isinstance(sent, bool) or not isinstance(sent, int) or not 0 <= sent <= total_chars:
        raise ValueError(f"sent must lie in [0, total_chars], got {sent!r}")
    return chunk, m, sent


_FRESH_ACK = {}  # (device index, L, last) -> the fresh state on the device; only ever read


def _ack_state(state, dev, total_chars, chunk):
    import torch
    if _is_torch(state):
        _int_tensor(state, "state", dev, 4, dtypes=(torch.int64,))
        return state
    if state is None:
        # One tensor per device and first frame, made outside any stream capture and
        # complete before it is first used (the one wait), as _accept_state keeps its
        # zero state: later calls on any stream, captured ones included, may read it.
        fresh = fresh_ack_state(total_chars, chunk)
        key = (dev.index if dev.index is not None else torch.cuda.current_device(),) + fresh[1:3]
        t = _FRESH_ACK.get(key)
        if t is None:
            t = torch.tensor(fresh, dtype=torch.int64).to(dev)
            if torch.cuda.is_current_stream_capturing():
                return t
            torch.cuda.current_stream(dev).synchronize()
            if len(_FRESH_ACK) < 64:
                _FRESH_ACK[key] = t
        return t
    try:
        p, L, last, done = (int(v) for v in state)
    except (TypeError, ValueError):
        raise TypeError("state must be None, (p, L, last, done) or the state tensor of a previous result") from None
    if p < 0 or L < 0:
        raise ValueError("state: p and L must not be negative")
    return torch.tensor([p, L, 1 if last else 0, 1 if done else 0], dtype=torch.int64).to(dev)


def ack_progress(seq, ack, flags, *, isn: int, total_chars: int, chunk: int = 1, usable=None, state=None,
                 mode: str = "exact", sent: Optional[int] = None, stream=None) -> AckProgress:
    """What the reference's sender makes of a batch of replies, in arrival order
    (``wait_ack``, utils/reliableUDP.py:64-85: a reply counts when its ack_num
    is ISN + characters acknowledged + characters outstanding), on the device
    with no host wait (rudp_ack_progress; include/rudp.h states the rule).

    ``seq``, ``ack`` (u16 [N]) and ``flags`` (u8 [N]) as the decode returns
    them, ``usable`` a u8 or bool [N] tensor (None: every reply).  ``isn``,
    ``total_chars`` and ``chunk`` are the constants of the ``send()``.
    ``state``: None (a fresh transfer), ``(p, L, last, done)``, or the
    ``state`` of the previous call's result.  (The first ``state=None`` call
    for a first frame's size on a device waits once for its fresh state to be
    written; no later call waits.)  ``mode="cumulative"`` takes any
    reply on the chunk grid between the expected one and ISN + ``sent``
    (default: ``total_chars``), for a sender with several frames in flight."""
    if not _is_torch(seq) or not _is_torch(ack) or not _is_torch(flags):
        raise TypeError("ack_progress takes torch tensors on a HIP device (no host-memory form)")
    chunk, m, sent = _ack_scalars(isn, total_chars, chunk, mode, sent)
    import torch
    dev = seq.device
    if dev.type != "cuda":
        raise ValueError("ack_progress runs on a HIP device")
    _dev_check(seq, "seq", torch.uint16, 1, dev)
    n = seq.shape[0]
    _int_tensor(ack, "ack", dev, n, dtypes=(torch.uint16,))
    _int_tensor(flags, "flags", dev, n, dtypes=(torch.uint8,))
    if usable is not None:
        _int_tensor(usable, "usable", dev, n, dtypes=(torch.uint8, torch.bool))
    st = _ack_state(state, dev, total_chars, chunk)
    lay = AckProgress.layout(n)
    buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    tab = n > 0
    _native.check(_native.lib().rudp_ack_progress(
        seq.data_ptr() if tab else None, ack.data_ptr() if tab else None, flags.data_ptr() if tab else None,
        usable.data_ptr() if usable is not None and tab else None, n, isn, total_chars, chunk, m, sent,
        st.data_ptr(), base + lay["valid"] if tab else None, base + lay["pointer"] if tab else None,
        base + lay["state"], base + lay["info"], dev.index or 0, _stream_ptr(stream, dev)))
    return AckProgress(buf, n)


class Acknowledged(_AckResult):
    """Result of ``acknowledge``: one allocation, every member a view of it.

    ``seq``, ``ack``, ``csum`` (u16 [N]), ``flags``, ``ok`` (u8 [N]) as
    ``unpack_batch_varlen`` returns them; ``usable`` (u8 [N]: the checksum and
    the frame's shape are good; UTF-8 is not looked at); ``valid``,
    ``pointer``, ``state``, ``info`` and the host reads as ``AckProgress``;
    ``final_frame`` (u8 [H]: the closing ``send_ack`` datagram, written when
    ``done`` became true in this batch, ``end < N``), ``final_csum`` (u16 [1])
    and ``status`` (int32 [1], RUDP_ST_* of the call) on the device."""

    __slots__ = ("_H",)

    def __init__(self, buf, n: int, H: int):
        self._buf, self._n, self._H, self._lay = buf, n, H, Acknowledged.layout(n, H)
        self._views, self._info = {}, None

    @staticmethod
    def layout(n: int, H: int):
        """Byte offsets in the one allocation, every array aligned to its
        element; ``size`` is the allocation's."""
        lay, at = {}, 0
        for name, nbytes in (("pointer", 8 * n), ("state", 32), ("info", 64), ("status", 8),
                             ("seq", 2 * n), ("ack", 2 * n), ("csum", 2 * n), ("final_csum", 2),
                             ("flags", n), ("ok", n), ("usable", n), ("valid", n), ("final_frame", 8)):
            lay[name] = at
            at += nbytes
        lay["size"] = at
        return lay

    def _u16(self, name):
        import torch
        return self._cut(name, 2 * self._n, torch.uint16)

    seq = property(lambda self: self._u16("seq"))
    ack = property(lambda self: self._u16("ack"))
    csum = property(lambda self: self._u16("csum"))
    flags = property(lambda self: self._cut("flags", self._n, None))
    ok = property(lambda self: self._cut("ok", self._n, None))
    usable = property(lambda self: self._cut("usable", self._n, None))
    final_frame = property(lambda self: self._cut("final_frame", self._H, None))

    @property
    def final_csum(self):
        import torch
        return self._cut("final_csum", 2, torch.uint16)

    @property
    def status(self):
        import torch
        return self._cut("status", 4, torch.int32)

    def check(self) -> "Acknowledged":
        """Raise ValueError if the device rejected a frame's offsets; one synchronization."""
        _raise_status(self.status)
        return self


def acknowledge(frames, frame_off, layout: Union[str, int] = "rudp7", *, isn: int, total_chars: int, chunk: int = 1,
                state=None, mode: str = "exact", sent: Optional[int] = None, csum=None, stream=None) -> Acknowledged:
    """A batch of reply datagrams (packed frames, as recvmmsg leaves them) turned
    into the sender's new state and, when the receiver's FIN is among them, the
    closing ``send_ack`` datagram of utils/reliableUDP.py:87-93, in one library
    call with no host wait (rudp_acknowledge).  A batch of at most ``ACK_TILE``
    replies in at most ``ACK_FUSED_BYTES`` bytes (and ``ACK_FUSED_MEAN`` per
    reply) is one kernel launch.

    ``frames`` (u8 1-D), ``frame_off`` (int64 [N + 1]) and ``csum`` (u16 [N],
    the rudp5 sideband; None: rudp5 frames are taken unverified) are device
    tensors; the rest as ``ack_progress`` takes them.  Every array equals what
    ``unpack_batch_varlen``, the usable rule and ``ack_progress`` return for the
    same input."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off):
        raise TypeError("acknowledge takes torch tensors on a HIP device (no host-memory form)")
    chunk, m, sent = _ack_scalars(isn, total_chars, chunk, mode, sent)
    import torch
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("acknowledge runs on a HIP device")
    _dev_check(frames, "frames", torch.uint8, 1, dev)
    _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
    n = frame_off.shape[0] - 1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if csum is not None:
        if H == 7:
            raise ValueError("rudp7 carries its checksum in-band; csum is for rudp5")
        _dev_check(csum, "csum", torch.uint16, 1, dev)
        if csum.shape[0] != n:
            raise ValueError(f"csum has {csum.shape[0]} entries for {n} frames")
    st = _ack_state(state, dev, total_chars, chunk)
    nbytes = frames.numel()
    lay = Acknowledged.layout(n, H)
    buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(name):
        return base + lay[name] if n else None

    out = _native.RudpAcknowledged(
        seq=tab("seq"), ack=tab("ack"), flags=tab("flags"), ok=tab("ok"), csum_out=tab("csum"),
        usable=tab("usable"), valid=tab("valid"), pointer=tab("pointer"), state_out=base + lay["state"],
        info=base + lay["info"], final_frame=base + lay["final_frame"], final_csum=base + lay["final_csum"],
        status=base + lay["status"])
    _native.check(_native.lib().rudp_acknowledge(
        frames.data_ptr() if nbytes else None, nbytes, frame_off.data_ptr(),
        min(nbytes // n, 0xFFFFFFFF) if n else 0, n, csum.data_ptr() if csum is not None and n else None,
        isn, total_chars, chunk, m, sent, st.data_ptr(), ctypes.byref(out), H, dev.index or 0,
        _stream_ptr(stream, dev)))
    return Acknowledged(buf, n, H)


# ------------------------------------------------------------ replies of many transfers
_ST_ACK_FLOWS = (_ST_MESSAGES[-1],  # a flow slot out of range
                 (_native.ST_FLOW_ROW, "a row of the states table has isn > 65535, chunk > 16383 or sent > total_chars"))


def _raise_bits(bits: int, messages) -> None:
    if bits:
        raise ValueError("; ".join(m for b, m in messages if bits & b) or f"status {bits:#x}")


def ack_flow_states(n_flows: int, device):
    """The zero table of ``n_flows`` idle slots for ``ack_flows``: int64
    [n_flows, 8] on ``device``, a row {p, L, last, done, isn, T, C, sent}."""
    import torch
    if isinstance(n_flows, bool) or not isinstance(n_flows, int) or not 1 <= n_flows <= 0xFFFFFFFE:
        raise ValueError(f"n_flows must be an int in [1, 2^32 - 2], got {n_flows!r}")
    return torch.zeros((n_flows, 8), dtype=torch.int64, device=device)


def ack_flow_open(states, slot: int, isn: int, total_chars: int, chunk: int = 1):
    """Open ``slot`` of an ``ack_flow_states`` table for a fresh transfer: the
    row {0, min(C, T), L == T, 0, isn, T, C, 0}, written in stream order."""
    import torch
    if not _is_torch(states) or states.dtype != torch.int64 or states.dim() != 2 or states.shape[1] != 8:
        raise TypeError("states must be the int64 [n_flows, 8] table of ack_flow_states")
    if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < states.shape[0]:
        raise ValueError(f"slot must be an int in [0, {states.shape[0]}), got {slot!r}")
    chunk, _, _ = _ack_scalars(isn, total_chars, chunk, "exact", None)
    if total_chars >= 1 << 63:
        raise ValueError(f"total_chars must be below 2^63, got {total_chars}")
    row = list(fresh_ack_state(total_chars, chunk)) + [isn, total_chars, chunk, 0]
    states[slot] = torch.tensor(row, dtype=torch.int64).to(states.device, non_blocking=True)
    return states


class AckFlows:
    """Result of ``ack_flows``: one device buffer with cut views.  ``valid``
    (u8 [N]), ``pointer`` (int64 [N]), ``order`` (int32 [N]), ``order_off``
    (int32 [N + 1], of which [0..A] are written), ``flow_info`` (int64 [N, 8],
    A rows written), ``info`` (int64 [8]: A, valid replies, ended flows,
    characters newly acknowledged, replies outside every run, flows walked, 0,
    0), ``status`` (int32 [1]), and with a ``final_layout`` ``final_frames``
    (u8 [N, H], E rows written), ``final_csum`` (u16 [N]) and ``final_flow``
    (int32 [N]) as rudp_ack_flows defines them; ``states`` is the caller's
    table, updated in place.  ``active``, ``count``, ``ended``,
    ``newly_acknowledged``, ``flowless``, ``flows()``, ``finals()`` and
    ``check()`` read the device once, one synchronization for all; nothing else
    waits."""

    __slots__ = ("_buf", "_n", "_H", "_lay", "_views", "_host", "states")

    def __init__(self, buf, n: int, H: int, states):
        self._buf, self._n, self._H, self._lay, self.states = buf, n, H, AckFlows.layout(n, H), states
        self._views, self._host = {}, None

    @staticmethod
    def layout(n: int, H: int):
        """Byte offsets in the one allocation: pointer (u64 [n]) | flow_info
        (u64 [n][8]) | info (u64 [8]) | status (u32, padded to 8) | final_flow
        (u32 [n]) | final_csum (u16 [n]) | final_frames (u8 [n * H]) | order
        (u32 [n]) | order_off (u32 [n + 1]) | valid (u8 [n]); then the size.
        flow_info to final_frames is what the host reads, in one copy."""
        lay, at = {}, 0
        for name, nbytes in (("pointer", 8 * n), ("flow_info", 64 * n), ("info", 64), ("status", 8),
                             ("final_flow", 4 * n), ("final_csum", 2 * n), ("final_frames", n * H)):
            lay[name] = at
            at += nbytes
        lay["host_end"] = at
        at = (at + 3) & ~3
        for name, nbytes in (("order", 4 * n), ("order_off", 4 * (n + 1)), ("valid", n)):
            lay[name] = at
            at += nbytes
        lay["size"] = at
        return lay

    def _cut(self, name, nbytes, dtype):
        v = self._views.get(name)
        if v is None:
            lo = self._lay[name]
            v = self._buf[lo:lo + nbytes]
            v = self._views[name] = v if dtype is None else v.view(dtype)
        return v

    valid = property(lambda self: self._cut("valid", self._n, None))

    @property
    def pointer(self):
        import torch
        return self._cut("pointer", 8 * self._n, torch.int64)

    @property
    def order(self):
        import torch
        return self._cut("order", 4 * self._n, torch.int32)

    @property
    def order_off(self):
        import torch
        return self._cut("order_off", 4 * (self._n + 1), torch.int32)

    @property
    def flow_info(self):
        import torch
        return self._cut("flow_info", 64 * self._n, torch.int64).view(self._n, 8)

    @property
    def info(self):
        import torch
        return self._cut("info", 64, torch.int64)

    @property
    def status(self):
        import torch
        return self._cut("status", 4, torch.int32)

    @property
    def final_frames(self):
        return self._cut("final_frames", self._n * self._H, None).view(self._n, self._H)

    @property
    def final_csum(self):
        import torch
        return self._cut("final_csum", 2 * self._n, torch.uint16)

    @property
    def final_flow(self):
        import torch
        return self._cut("final_flow", 4 * self._n, torch.int32)

    def _read(self):
        if self._host is None:
            lay, n, H = self._lay, self._n, self._H
            lo = lay["flow_info"]
            raw = self._buf[lo:lay["host_end"]].cpu().numpy()
            words = raw[:lay["status"] + 8 - lo].view(np.int64)
            info = [int(v) for v in words[8 * n:8 * n + 8]]
            A, E = info[0], info[2] if H else 0
            flows = words[:8 * A].reshape(A, 8).copy()
            fflow = raw[lay["final_flow"] - lo:lay["final_flow"] - lo + 4 * E].view(np.int32).copy()
            at = lay["final_frames"] - lo
            frames = [raw[at + H * e:at + H * (e + 1)].tobytes() for e in range(E)]
            self._host = (info, flows, int(words[8 * n + 8]) & 0xFFFFFFFF, fflow, frames)
        return self._host

    active = property(lambda self: self._read()[0][0])
    count = property(lambda self: self._read()[0][1])
    ended = property(lambda self: self._read()[0][2])
    newly_acknowledged = property(lambda self: self._read()[0][3])
    flowless = property(lambda self: self._read()[0][4])

    def flows(self):
        """int64 [A, 8] on the host, ascending by slot: slot, end, valid
        replies, characters newly acknowledged, p after, next frame, done,
        closing_seq | closing_ack << 16 of every active flow."""
        return self._read()[1]

    def finals(self):
        """[(a, datagram bytes)] of the flows that ended in this call, a the row
        of ``flows()``; empty without a ``final_layout``."""
        h = self._read()
        return list(zip(h[3].tolist(), h[4]))

    def check(self) -> "AckFlows":
        _raise_bits(self._read()[2], _ST_ACK_FLOWS)
        return self

    def __len__(self) -> int:
        return self._n


def _ack_flows_args(flow, states, mode, final_layout, dev, n):
    import torch
    _flows_tensor(flow, "flow", dev, (torch.int32,), n)
    _flows_tensor(states, "states", dev, (torch.int64,), ndim=2)
    if states.shape[1] != 8 or not 1 <= states.shape[0] <= 0xFFFFFFFE:
        raise ValueError(f"states must be int64 [n_flows, 8] with 1 <= n_flows <= 2^32 - 2, got {tuple(states.shape)}")
    try:
        m = ACK_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"mode must be 'exact' or 'cumulative', got {mode!r}") from None
    H = 0 if final_layout is None else layout_header_len(final_layout)
    return m, H


def ack_flows(seq, ack, flags, flow, *, states, usable=None, mode: str = "exact", final_layout=None,
              stream=None) -> AckFlows:
    """``ack_progress`` for a batch that carries the replies of many transfers
    (rudp_ack_flows; include/rudp.h states the rule): ``flow`` (int32 [N]
    holding u32 values) names each reply's row in ``states`` (int64 [n_flows,
    8] from ``ack_flow_states``, rows opened with ``ack_flow_open``; words 0 to
    3 are updated in place), -1 (``FLOW_NONE``) a reply to ignore.  Every flow
    is judged by the sender's rule on its own replies in arrival order, all
    flows in one launch.  ``final_layout`` ("rudp5" / "rudp7"): also build the
    closing datagram of every flow that ended.  At most ``FLOWS_MAX_BATCH``
    replies.  Never waits; ``check()`` on the result raises when a slot was out
    of range or a row refused."""
    for name, t in (("seq", seq), ("ack", ack), ("flags", flags), ("flow", flow), ("states", states)):
        if not _is_torch(t):
            raise TypeError(f"ack_flows takes torch tensors on a HIP device (no host-memory form): {name}")
    import torch
    dev = seq.device
    if dev.type != "cuda":
        raise ValueError("ack_flows runs on a HIP device")
    _flows_tensor(seq, "seq", dev, (torch.uint16,))
    n = seq.shape[0]
    if n > FLOWS_MAX_BATCH:
        raise ValueError(f"ack_flows takes at most {FLOWS_MAX_BATCH} replies (one recvmmsg batch), got {n}")
    _flows_tensor(ack, "ack", dev, (torch.uint16,), n)
    _flows_tensor(flags, "flags", dev, (torch.uint8,), n)
    if usable is not None:
        _flows_tensor(usable, "usable", dev, (torch.uint8, torch.bool), n)
    m, H = _ack_flows_args(flow, states, mode, final_layout, dev, n)
    lay = AckFlows.layout(n, H)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        buf = torch.empty(lay["size"], dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def tab(t):
        return t if n else None

    _native.check(_native.lib().rudp_ack_flows(
        tab(seq.data_ptr()), tab(ack.data_ptr()), tab(flags.data_ptr()),
        usable.data_ptr() if usable is not None and n else None, tab(flow.data_ptr()), n, m, states.data_ptr(),
        states.shape[0], tab(base + lay["valid"]), tab(base + lay["pointer"]), tab(base + lay["order"]),
        tab(base + lay["order_off"]), tab(base + lay["flow_info"]), base + lay["info"], base + lay["status"], H,
        tab(base + lay["final_frames"]) if H else None, tab(base + lay["final_csum"]) if H else None,
        tab(base + lay["final_flow"]) if H else None, dev.index or 0, _stream_ptr(stream, dev)))
    return AckFlows(buf, n, H, states)


class AcknowledgedFlows(NamedTuple):
    """Result of ``acknowledge_flows``: ``decoded`` (``VarlenDecoded``: seq, ack,
    flags, ok), ``usable`` (u8 [N]) and ``judged`` (``AckFlows``)."""
    decoded: Any
    usable: Any
    judged: AckFlows


def acknowledge_flows(frames, frame_off, flow, layout: Union[str, int] = "rudp7", *, states, csum=None,
                      mode: str = "exact", stream=None) -> AcknowledgedFlows:
    """Reply datagrams of many transfers (packed frames, as recvmmsg leaves
    them) to every sender's new state and the closing datagrams of the flows
    that ended: ``unpack_batch_varlen`` without a host check, ``acknowledge``'s
    usable rule (the checksum and the frame's shape are good) and ``ack_flows``
    with ``final_layout=layout``, chained on the stream with no host wait.  A
    frame with bad offsets is unusable and sets RUDP_ST_OFFSETS in
    ``decoded.status``."""
    H = layout_header_len(layout)
    if not _is_torch(frames) or not _is_torch(frame_off) or not _is_torch(flow) or not _is_torch(states):
        raise TypeError("acknowledge_flows takes torch tensors on a HIP device (no host-memory form)")
    import torch
    dev = frames.device
    if dev.type != "cuda":
        raise ValueError("acknowledge_flows runs on a HIP device")
    n = frame_off.shape[0] - 1 if frame_off.dim() == 1 else -1
    if n < 0:
        raise ValueError("frame_off needs N + 1 entries")
    if n > FLOWS_MAX_BATCH:
        raise ValueError(f"acknowledge_flows takes at most {FLOWS_MAX_BATCH} replies (one recvmmsg batch), got {n}")
    _ack_flows_args(flow, states, mode, layout, dev, n)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        dec = unpack_batch_varlen(frames, frame_off, H, csum=csum, check=False, stream=stream)
        usable = (dec.ok == _native.OK_GOOD) | (dec.ok == _native.OK_UNVERIFIED)
        usable = usable.to(torch.uint8)
    judged = ack_flows(dec.seq, dec.ack, dec.flags, flow, states=states, usable=usable, mode=mode,
                       final_layout=layout, stream=stream)
    return AcknowledgedFlows(dec, usable, judged)


# ------------------------------------------------------------ message -> datagrams
MAX_CHUNK = 16383  # characters per datagram: 4 * 16383 <= 65535 payload bytes


class SegmentTable(NamedTuple):
    """The first n packets of a ``SegmentedMessage``: ``pack_batch_varlen``'s
    ``headers`` and ``lengths``, and the n + 1 payload offsets."""
    headers: HeaderTable
    lengths: Any
    payload_off: Any


class SegmentedMessage:
    """Result of ``segment_message``: ``payload`` (u8, the message bytes on the
    device: the packed payload of every packet), ``headers`` (a ``HeaderTable``
    of the full-capacity seq / ack / flags arrays), ``lengths`` (int32
    [capacity]), ``payload_off`` (int64 [capacity + 1]) and ``status`` (device
    int32 [1], RUDP_ST_* of the call, 0 = valid).  Only the first ``count``
    entries are packets; ``count`` and ``characters`` are read from the device
    on first use (one synchronization for both), unless the call knew them on
    the host (a ``str`` message).  ``table(n)`` slices the arrays to n packets.

    All arrays live in one device allocation and are cut out of it on first use.
    """

    __slots__ = ("payload", "capacity", "_buf", "_known", "_views")

    # one allocation: payload_off (i64 [cap + 1]) | count (i64 [2]) | status (i32) | pad |
    # lengths (i32 [cap]) | seq (u16 [cap]) | ack (u16 [cap]) | flags (u8 [cap])
    def __init__(self, payload, buf, capacity: int, known=None):
        self.payload, self._buf, self.capacity = payload, buf, capacity
        self._known = known  # (count, characters) when the host knows them
        self._views = {}

    @staticmethod
    def layout(cap: int):
        """Byte offsets of (count, status, lengths, seq, ack, flags, end) in the allocation."""
        up = lambda x: x + (-x % 16)  # noqa: E731  (every array on a 16-B boundary)
        at_count = up(8 * (cap + 1))
        at_len = at_count + 32
        at_seq = up(at_len + 4 * cap)
        at_ack = up(at_seq + 2 * cap)
        at_flags = up(at_ack + 2 * cap)
        return at_count, at_count + 16, at_len, at_seq, at_ack, at_flags, at_flags + cap

    def _cut(self, name, lo, hi, dtype):
        v = self._views.get(name)
        if v is None:
            v = self._views[name] = self._buf[lo:hi].view(dtype)
        return v

    @property
    def payload_off(self):
        import torch
        return self._cut("payload_off", 0, 8 * (self.capacity + 1), torch.int64)

    @property
    def status(self):
        import torch
        at = self.layout(self.capacity)[1]
        return self._cut("status", at, at + 4, torch.int32)

    @property
    def lengths(self):
        import torch
        at = self.layout(self.capacity)[2]
        return self._cut("lengths", at, at + 4 * self.capacity, torch.int32)

    @property
    def headers(self) -> HeaderTable:
        import torch
        lay, cap = self.layout(self.capacity), self.capacity
        return HeaderTable(self._cut("seq", lay[3], lay[3] + 2 * cap, torch.uint16),
                           self._cut("ack", lay[4], lay[4] + 2 * cap, torch.uint16),
                           self._cut("flags", lay[5], lay[5] + cap, torch.uint8))

    def _counts(self):
        if self._known is None:
            import torch
            at = self.layout(self.capacity)[0]
            self._known = tuple(self._buf[at:at + 16].view(torch.int64).tolist())
        return self._known

    @property
    def count(self) -> int:
        """Packets the message makes (it may exceed ``capacity``: then the status says so)."""
        return self._counts()[0]

    @property
    def characters(self) -> int:
        """Lead bytes of the message: len(message) for valid UTF-8."""
        return self._counts()[1]

    def table(self, n: Optional[int] = None) -> SegmentTable:
        """The arrays sliced to ``n`` packets; None reads ``count``."""
        if n is None:
            n = min(self.count, self.capacity)
        if not 0 <= n <= self.capacity:
            raise ValueError(f"n = {n} is outside the table's {self.capacity} entries")
        h = self.headers
        return SegmentTable(HeaderTable(h.seq[:n], h.ack[:n], h.flags[:n]), self.lengths[:n], self.payload_off[:n + 1])

    def check(self) -> "SegmentedMessage":
        """Raise ValueError if the device rejected the call (one synchronization)."""
        bits = int(self.status.item())
        if bits:
            msgs = [m for b, m in _ST_MESSAGES if bits & b] or [f"status {bits:#x}"]
            if bits & _native.ST_PACKETS_CAP:
                msgs.append(f"{self.count} packets are needed, the table holds {self.capacity}")
            raise ValueError("; ".join(msgs))
        return self


def _check_chunk(chunk) -> int:
    if isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= MAX_CHUNK:
        raise ValueError(f"chunk must be an int in [1, {MAX_CHUNK}] characters per datagram, got {chunk!r}")
    return chunk


def segment_message(message, isn: int, *, chunk: int = 1, max_packets: Optional[int] = None, device=None,
                    stream=None, check: bool = True, reuse: Optional[SegmentedMessage] = None) -> SegmentedMessage:
    """Cut a message into datagrams of ``chunk`` characters on the device: the
    header table and lengths the reference's ``send_data`` derives per datagram
    (utils/reliableUDP.py:44-60: seq = ISN + character pointer, ack 0, SYN on
    the first and FIN on the last frame, an empty message one SYN|FIN frame),
    for the whole message in one call (rudp_segment_utf8).

    ``message``: a ``str``, encoded on the host and copied to ``device``
    (default "cuda"); its packet count max(1, ceil(len(message) / chunk)) is
    known on the host, so nothing waits.  Or a u8 1-D tensor of UTF-8 bytes on
    a HIP device: the table then holds ``max_packets`` entries, by default the
    bound max(1, ceil(numel / chunk)), which is exact for ASCII.  Characters
    are counted by lead bytes; validity is not judged (``validate_utf8``).

    ``check=True`` waits and raises ValueError when the message makes more
    packets than the table holds or a packet exceeds 65535 bytes (invalid
    UTF-8 only); ``check=False`` never waits.  ``reuse``: an earlier result of
    the same capacity, whose table takes this call's outputs (no allocation).
    """
    chunk = _check_chunk(chunk)
    import torch
    known = None
    if isinstance(message, str):
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise ValueError("segment_message runs on a HIP device")
        raw = message.encode()
        payload = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev) if raw else \
            torch.empty(0, dtype=torch.uint8, device=dev)
        known = (max(1, -(-len(message) // chunk)), len(message))
        if max_packets is None:
            max_packets = known[0]
    elif _is_torch(message):
        payload = message
        dev = payload.device
        if dev.type != "cuda":
            raise ValueError("segment_message runs on a HIP device")
        _dev_check(payload, "message", torch.uint8, 1, dev)
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError("segment_message runs on a HIP device")
        if max_packets is None:
            max_packets = max(1, -(-payload.numel() // chunk))
    else:
        raise TypeError("message must be a str or a u8 torch.Tensor on a HIP device")
    if isinstance(max_packets, bool) or not isinstance(max_packets, int) or max_packets < 0:
        raise ValueError(f"max_packets must be a non-negative int, got {max_packets!r}")
    cap = max_packets
    lay = SegmentedMessage.layout(cap)
    if reuse is not None:
        if not isinstance(reuse, SegmentedMessage) or reuse.capacity != cap or reuse._buf.device != dev:
            raise ValueError("reuse= must be an earlier segment_message result of the same capacity and device")
        buf = reuse._buf
    else:
        buf = payload.new_empty(lay[6])
    base = buf.data_ptr()
    tab = cap > 0
    _native.check(_native.lib().rudp_segment_utf8(
        payload.data_ptr() if payload.numel() else None, payload.numel(), chunk, int(isn) & 0xFFFFFFFF, cap,
        base + lay[3] if tab else None, base + lay[4] if tab else None, base + lay[5] if tab else None,
        base + lay[2] if tab else None, base if tab else None, base + lay[0], base + lay[1],
        dev.index if dev.index is not None else torch.cuda.current_device(), _stream_ptr(stream, dev)))
    res = SegmentedMessage(payload, buf, cap, known)
    return res.check() if check else res


def frame_message(message, isn: int, *, chunk: int = 1, layout: Union[str, int] = "rudp5",
                  want_csum: bool = False, n: Optional[int] = None, max_packets: Optional[int] = None, device=None,
                  stream=None, check: bool = True) -> VarlenFrames:
    """The datagrams of a message as the reference's ``send_data`` builds them
    (utils/reliableUDP.py:44-61), for the whole message: ``segment_message``,
    then ``pack_batch_varlen`` on its table.  Returns ``VarlenFrames``: frame k
    is byte-identical to the reference's packet for message pointer k * chunk.

    The frame batch needs the packet count on the host.  For a ``str`` it is
    known, and with ``n`` the caller gives it (the first ``n`` packets are
    framed): the call then never waits (with ``check=False``).  For a device
    tensor without ``n`` the count is read from the device: one
    synchronization.
    """
    H = layout_header_len(layout)
    seg = segment_message(message, isn, chunk=chunk, max_packets=max_packets, device=device, stream=stream,
                          check=check)
    tab = seg.table(n)  # (n None: the count, from the host for a str, else the one device read)
    return pack_batch_varlen(tab.headers, seg.payload, tab.lengths, H, want_csum=want_csum, stream=stream,
                             check=check)


def validate_utf8(frames, layout: Union[str, int] = "rudp7", *, frame_off=None, stream=None):
    """u8 [N]: 1 where Packet(frame).get_payload() would succeed (utils/packet.py:68-73),
    0 where it would raise UnicodeDecodeError.  ``frames``: [N, F] fixed-length,
    or 1-D with ``frame_off`` (N + 1 offsets)."""
    import torch
    H = layout_header_len(layout)
    dev = frames.device
    if frame_off is None:
        _dev_check(frames, "frames", torch.uint8, 2, dev)
        n, F = frames.shape
        off_ptr = None
    else:
        _dev_check(frames, "frames", torch.uint8, 1, dev)
        _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
        n = frame_off.shape[0] - 1
        F = _check_offsets(frames, frame_off, stream)  # mean frame length: a lanes-per-frame hint
        off_ptr = frame_off.data_ptr()
    valid = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n:
        _native.check(_native.lib().rudp_validate_utf8(
            frames.data_ptr() if frames.numel() else None, off_ptr, F, n, H, valid.data_ptr(),
            dev.index or 0, _stream_ptr(stream, dev)))
    return valid


PROXY_MAX_MEMORY = 500  # proxy.py:17


def detect_retransmissions(frames, *, frame_off=None, window: int = PROXY_MAX_MEMORY, stream=None,
                           check: bool = True):
    """u8 [N]: 1 where frame i equals one of the `window` frames before it.

    Batched form of the reference proxy's `packet in self.packets` check
    (proxy.py:90, with the 500-packet history of proxy.py:17, :92-94) and
    Packet.__eq__ semantics (utils/packet.py:83-86).  ``frames``: [N, F]
    fixed-length, or 1-D with ``frame_off`` (N + 1 offsets), checked on the
    device (rudp_dedup_window_checked): a frame whose offsets are decreasing or
    past ``frames`` gets 2 and is never read; ``check=True`` waits and raises
    ValueError when there is one, ``check=False`` never waits.
    """
    import torch
    dev = frames.device
    if frame_off is None:
        _dev_check(frames, "frames", torch.uint8, 2, dev)
        n, F = frames.shape
        off_ptr = None
    else:
        _dev_check(frames, "frames", torch.uint8, 1, dev)
        _int_tensor(frame_off, "frame_off", dev, dtypes=(torch.int64,))
        n = frame_off.shape[0] - 1
        if n < 0:
            raise ValueError("frame_off needs N + 1 entries")
        dup = torch.empty((n,), dtype=torch.uint8, device=dev)
        if n:
            # mean frame length from the buffer size: picks lanes per frame
            _native.check(_native.lib().rudp_dedup_window_checked(
                frames.data_ptr() if frames.numel() else 16, frames.numel(), frame_off.data_ptr(),
                min(frames.numel() // n, 0xFFFFFFFF), n, window, dup.data_ptr(), dev.index or 0,
                _stream_ptr(stream, dev)))
            if check and bool((dup == _native.DUP_BAD_OFFSETS).any()):
                raise ValueError("frame_off must be non-decreasing offsets inside frames")
        return dup
    dup = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n:
        _native.check(_native.lib().rudp_dedup_window(
            frames.data_ptr() if frames.numel() else None, off_ptr, F, n, window, dup.data_ptr(),
            dev.index or 0, _stream_ptr(stream, dev)))
    return dup
