"""Every form that computes the checksum, over the constructed corpus of
tests/csum_cases.py: one's-complement zero (0x0000 for a non-zero multiple of
0xFFFF, 0xFFFF for the all-zero frame only), its neighbours, the second fold,
the top of the 32-bit accumulator, parity patterns, and the 0x0000 / 0xFFFF
twins that must be RUDP_OK_BAD_CSUM.  Bit-exact against ``ref_csum`` /
``ref_decode`` (RFC 1071 in Python integers); no tolerance anywhere.

The forms are the tables below: what is called, under which knobs of the
diagnostics build (``rudpx_tune``; the numbers and values are those of the
tests named beside them), and for which shapes.  A form whose precondition
excludes a shape is not listed for it.
"""
import contextlib
import ctypes
import functools
import random

import numpy as np
import pytest

import csum_cases as cc
from accept_ref import FIN, SYN, accept_ref, chars_ref
from accept_ref import scan_model as accept_scan_model
from rudp import _native, batch

pytestmark = pytest.mark.gpu

LAYOUTS = (5, 7)


def _tile(L):
    """The fixed-length encode / decode tiles take payloads of whole 16-byte chunks up to 4096 bytes."""
    return L > 0 and L % 16 == 0 and L <= 4096


# ---- fixed-length encode: (name, knobs, applies to L) -------------------------
FIXED_ENCODE_FORMS = [("default", [], lambda L: True)]
# block size (10), packets per tile (2), tiles per CU (6): test_encode_tile_sizes_agree
FIXED_ENCODE_FORMS += [(f"block {b} tile {t} per-CU {pc}", [(10, b), (2, t), (6, pc)], _tile)
                       for b, t, pc in [(256, t, pc) for t in (4, 8, 16, 32, 256) for pc in (-1, 0, 5)]
                       + [(64, t, 0) for t in (4, 8, 16, 32)] + [(128, t, 16) for t in (8, 64)]]
# wave stores dealt from the first 64-B boundary (23): test_encode_align64_vs_oracle
FIXED_ENCODE_FORMS += [(f"align64 {a} tile {t}", [(23, a), (2, t)], _tile) for a in (1, 0) for t in (0, 4, 8, 32)]
# LDS-DMA phase 1 (25): test_dma_phase1_vs_oracle
FIXED_ENCODE_FORMS += [("DMA phase 1", [(25, 1)], _tile)]
# prebuilt header chunks (29) by tile (2), dealing (23), early table loads (30), LDS scratch (37):
# test_prebuilt_header_chunks_vs_oracle
FIXED_ENCODE_FORMS += [(f"prebuilt header chunks tile {t} align {a} early {e} scratch {s}",
                        [(29, 1), (2, t), (23, a), (30, e), (37, s)],
                        (lambda t: lambda L: _tile(L) and t * L <= 65536)(t))
                       for t in (0, 16, 32, 256)
                       for a, e, s in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, -1, 0), (0, 0, 1), (-1, -1, 1))]
# views shifted off the 16-byte grid: (payload bytes, frame bytes, table entries); tests/test_gpu_stride.py
ENCODE_VIEW_SHIFTS = ((1, 1, 0), (3, 3, 1))

# ---- fixed-length decode: verify tile (12), copy tile (11), 64-B dealing (23), staged outputs (34):
# test_decode_paths_agree; each with and without payload copy-out, through rudp_decode_utf8
FIXED_DECODE_FORMS = [("default", [], lambda L: True)]
FIXED_DECODE_FORMS += [(f"verify tile {v} copy tile {c} align {a} stage {s}", [(12, v), (11, c), (23, a), (34, s)],
                        lambda L: L > 0 and L % 16 == 0)
                       for v, c, a, s in ((1, 1, -1, 0), (1, 1, 1, 0), (0, 0, -1, 0), (1, 1, -1, 1), (1, 1, 1, 1))]
DECODE_VIEW_SHIFTS = (1, 3)

# ---- variable-length encode ---------------------------------------------------
# vector / per-packet (14) with the tile's header chunks (36): test_varlen_encode_kernels_vs_oracle;
# LDS tile on / off (16): test_varlen_encode_tile_kernel_vs_oracle
VARLEN_ENCODE_FORMS = [("default", [])]
VARLEN_ENCODE_FORMS += [(f"vector {v} header chunks {h}", [(14, v), (36, h)])
                        for v, h in ((1, 0), (1, 1), (1, 2), (0, 0))]
VARLEN_ENCODE_FORMS += [(f"tile {t} header chunks {h}", [(16, t), (36, h)])
                        for t, h in ((1, 0), (1, 1), (1, 2), (0, 0))]
VARLEN_ENCODE_HINTS = (0, 16, 1472, 65535)
# small-frame tiles: hint limit (46), frames per thread (47), own tile bases (50), length codes (74):
# test_small_frame_tiles_vs_oracle
SMALL_FRAME_FORMS = [(f"small {s} frames/thread {f} fused {u} codes {c}", [(46, s), (47, f), (50, u), (74, c)])
                     for f in (1, 2, 4, 8) for s, u, c in ((16, 1, 1), (16, 1, 0), (16, 0, 1), (0, 1, 1))]

# ---- variable-length decode ---------------------------------------------------
# vector (14) and tile (33) with the hint list of test_varlen_decode_kernels_vs_oracle
VARLEN_DECODE_FORMS = [(f"vector {v} tile {t}", [(14, v), (33, t)]) for v in (1, 0) for t in ((2, 0) if v else (1,))]
VARLEN_DECODE_HINTS = (0, 8, 64, 263, 519, 1031, 1472, 65535)
# the checked decode by byte spans (65) and not: tests/test_gpu_decode_span.py
SPAN_FORMS = [(f"span {s}", [(65, s)]) for s in (1, 0)]
SPAN_HINTS = (256, 1472)
# *_host varlen decode: per-frame outputs stored direct (1) or copied (0): knob 73
HOST_FORMS = [(f"host outputs direct {d}", [(73, d)]) for d in (1, 0)]


# ----------------------------------------------------------------- helpers
@contextlib.contextmanager
def knobs(settings):
    """The diagnostics build with the knobs set (none: the product library); every knob restored."""
    if not settings:
        _native.use_product()
        yield _native.lib()
        return
    lib = _native.tools_lib()
    lib.rudpx_tune.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.rudpx_tune.restype = ctypes.c_int
    old = []
    try:
        for k, v in settings:
            old.append((k, lib.rudpx_tune(k, v)))
        yield lib
    finally:
        for k, v in reversed(old):
            lib.rudpx_tune(k, v)
        _native.use_product()


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.cpu().numpy()


def _view(a, shift, cuda):
    """A device copy of ``a`` starting ``shift`` elements into a larger, 16-byte aligned allocation."""
    import torch
    a = np.ascontiguousarray(a)
    flat = a.reshape(-1)
    raw = torch.zeros(flat.size + shift + 16, dtype=getattr(torch, a.dtype.name), device=cuda)
    v = raw[shift:shift + flat.size]
    v.copy_(torch.from_numpy(flat).to(cuda))
    return v.view(*a.shape) if a.ndim > 1 else v


def same(got, want, what, where, labels, off=None):
    """array_equal, or an AssertionError that names the form, the frame and its class."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} for {want.shape} ({where})"
    if np.array_equal(got, want):
        return
    if off is None:
        i = int(np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[0])
        g, w = got[i], want[i]
    else:  # flat frame bytes: the frame that holds the first differing byte
        at = int(np.flatnonzero(got != want)[0])
        i = int(np.searchsorted(off, at, side="right") - 1)
        g, w = got[at], want[at]
    raise AssertionError(f"{what} differs: {where}, frame {i} of {len(labels)}, class {labels[i]}: "
                         f"got {g!r}, want {w!r}")


FIELDS = ("seq", "ack", "flags", "ok", "csum")


def _valid_of(frames):
    out = np.zeros(len(frames), np.uint8)
    for i, f in enumerate(frames):
        try:
            (b"" if f.label == "SHORT" else f.payload).decode()
            out[i] = 1
        except UnicodeDecodeError:
            pass
    return out


@functools.lru_cache(maxsize=8)
def fixed_want(L, layout, rot=0):
    b = cc.fixed_batch(L, layout, rot)
    w = {"batch": b, "labels": b.labels, "frames": b.wire(twins=False), "csum": b.true_csum(), "wire": b.wire(),
         "carried": b.carried(), "valid": _valid_of(b.frames)}
    w["side"] = dict(zip(FIELDS, b.expected(True)))
    w["noside"] = dict(zip(FIELDS, b.expected(False)))
    return w


@functools.lru_cache(maxsize=8)
def packed_want(layout, rot=0, kind="packed"):
    if kind == "small":
        b = cc.small_batch(layout)
    elif kind in cc.MAX_LENGTHS:
        b = cc.fixed_as_packed(cc.fixed_batch(kind, layout))
    else:
        b = cc.packed_batch(layout, rot) if rot == 0 else cc.packed_batch(layout, rot, cover=cc.PACKED_ROT_COVER)
    enc = b.encodable()
    fr, off, cs = b.encoded()
    wire, woff, carried = b.wire()
    w = {"batch": b, "labels": [f.label for f in b.frames], "enc_labels": [b.frames[i].label for i in enc],
         "tables": b.tables(), "frames": fr, "off": off, "csum": cs, "wire": wire, "woff": woff, "carried": carried,
         "valid": b.valid_utf8()}
    w["side"] = dict(zip(FIELDS, b.expected(True)))
    w["noside"] = dict(zip(FIELDS, b.expected(False)))
    return w


def _classes_met(labels, ok, csum):
    """The run saw what it is for: both zeros of the checksum, and twins judged bad."""
    lab = np.array(labels)
    assert (csum[lab == "ZK"] == 0x0000).all() and (lab == "ZK").any()
    assert (lab == "ZK_T").any() and (csum[lab == "ZK_T"] == 0x0000).all()
    assert (ok[lab == "ZK_T"] == cc.OK_BAD_CSUM).all()
    if (lab == "Z0").any():
        assert (csum[lab == "Z0"] == 0xFFFF).all()
        assert (csum[lab == "Z0_T"] == 0xFFFF).all() and (ok[lab == "Z0_T"] == cc.OK_BAD_CSUM).all()


# -------------------------------------------------------- fixed-length encode
def _fixed_inputs(w, cuda):
    import torch
    b = w["batch"]
    pay = dev(b.payload, cuda) if b.L else torch.zeros((b.n, 0), dtype=torch.uint8, device=cuda)
    return (dev(b.seq, cuda), dev(b.ack, cuda), dev(b.flags, cuda)), pay


def _check_fixed_encode(fr, cs, w, where):
    same(host(fr), w["frames"], "frames", where, w["labels"])
    same(host(cs), w["csum"], "csum", where, w["labels"])


def _fixed_encode_views(cuda, w, layout, where):
    """Payload, frames and header tables as views off the 16-byte grid (the stride forms)."""
    import torch
    b = w["batch"]
    F = b.L + layout
    for ps, fs, ts in ENCODE_VIEW_SHIFTS:
        tab = tuple(_view(x, ts, cuda) for x in (b.seq, b.ack, b.flags))
        pay = _view(b.payload, ps, cuda) if b.L else torch.zeros((b.n, 0), dtype=torch.uint8, device=cuda)
        raw = torch.full((b.n * F + fs + 32,), 0x5A, dtype=torch.uint8, device=cuda)
        out = raw[fs:fs + b.n * F].view(b.n, F)
        fr, cs = batch.pack_batch(tab, pay, layout, out=out, want_csum=True)
        _check_fixed_encode(fr, cs, w, f"{where}, views shifted {ps}/{fs}/{ts}")
        r = host(raw)
        assert (r[:fs] == 0x5A).all() and (r[fs + b.n * F:] == 0x5A).all(), where


@pytest.mark.parametrize("L", cc.FIXED_LENGTHS)
def test_fixed_encode_forms(cuda, L):
    for layout in LAYOUTS:
        for rot in range(1, len(cc.FIXED_CYCLE)):  # every class at row 0 and at the last row
            w = fixed_want(L, layout, rot)
            tab, pay = _fixed_inputs(w, cuda)
            fr, cs = batch.pack_batch(tab, pay, layout, want_csum=True)
            _check_fixed_encode(fr, cs, w, f"fixed encode, default, layout {layout}, L {L}, rotation {rot}")
        w = fixed_want(L, layout, 0)
        tab, pay = _fixed_inputs(w, cuda)
        for name, settings, applies in FIXED_ENCODE_FORMS:
            if not applies(L):
                continue
            with knobs(settings):
                fr, cs = batch.pack_batch(tab, pay, layout, want_csum=True)
            _check_fixed_encode(fr, cs, w, f"fixed encode, {name}, layout {layout}, L {L}")
        _fixed_encode_views(cuda, w, layout, f"fixed encode, layout {layout}, L {L}")
        lab = np.array(w["labels"])
        assert (w["csum"][lab == "ZK"] == 0x0000).all() and (w["csum"][lab == "Z0"] == 0xFFFF).all()


# -------------------------------------------------------- fixed-length decode
def _check_decoded(d, want, valid, where, labels, payload=None):
    for k in FIELDS:
        same(host(getattr(d, k)), want[k], k, where, labels)
    if valid is not None:
        same(host(d.valid), valid, "valid", where, labels)
    if payload is not None:
        same(host(d.payload), payload, "payload copy", where, labels)


def _fixed_decode_all(cuda, w, layout, L, settings, name):
    b = w["batch"]
    d_fr = dev(w["wire"], cuda)
    cases = [("in-band", None, "side")] if layout == 7 else \
        [("sideband", dev(w["carried"], cuda), "side"), ("no sideband", None, "noside")]
    for cname, d_cs, key in cases:
        for copy in (False, True):
            where = f"fixed decode, {name}, {cname}, copy-out {copy}, layout {layout}, L {L}"
            with knobs(settings):
                d = batch.unpack_batch(d_fr, layout, csum=d_cs, copy_payload=copy, utf8=True)
            _check_decoded(d, w[key], w["valid"], where, w["labels"], b.payload if copy else None)


@pytest.mark.parametrize("L", cc.FIXED_LENGTHS)
def test_fixed_decode_forms(cuda, L):
    for layout in LAYOUTS:
        for rot in range(1, len(cc.FIXED_CYCLE)):
            w = fixed_want(L, layout, rot)
            d = batch.unpack_batch(dev(w["wire"], cuda), layout, csum=dev(w["carried"], cuda) if layout == 5 else None,
                                   utf8=True)
            _check_decoded(d, w["side"], w["valid"], f"fixed decode, default, layout {layout}, L {L}, rotation {rot}",
                           w["labels"])
        w = fixed_want(L, layout, 0)
        for name, settings, applies in FIXED_DECODE_FORMS:
            if applies(L):
                _fixed_decode_all(cuda, w, layout, L, settings, name)
        for shift in DECODE_VIEW_SHIFTS:  # the frames as a view off the 16-byte grid
            fr = _view(w["wire"], shift, cuda)
            assert fr.data_ptr() % 16 == shift
            d = batch.unpack_batch(fr, layout, csum=dev(w["carried"], cuda) if layout == 5 else None, utf8=True)
            _check_decoded(d, w["side"], w["valid"], f"fixed decode, view shifted {shift}, layout {layout}, L {L}",
                           w["labels"])
        _classes_met(w["labels"], w["side"]["ok"], w["side"]["csum"])


# ------------------------------------------------------ variable-length encode
def _raw_encode_varlen(lib, cuda, tab, d_pay, d_lens, n, nbytes, hint, layout):
    import torch
    frames = torch.full((max(nbytes, 1),), 0xCD, dtype=torch.uint8, device=cuda)
    frame_off = torch.full((n + 1,), -1, dtype=torch.int64, device=cuda)
    csum = torch.zeros(n, dtype=torch.uint16, device=cuda)
    b = _native.RudpBatch(n=n, payload_len=hint, reserved=0, seq=tab[0].data_ptr(), ack=tab[1].data_ptr(),
                          flags=tab[2].data_ptr(), payload=d_pay.data_ptr() if d_pay.numel() else 16,
                          len=d_lens.data_ptr(), payload_off=None)
    _native.check(lib.rudp_encode_varlen(ctypes.byref(b), frames.data_ptr(), frame_off.data_ptr(), csum.data_ptr(),
                                         layout, 0, torch.cuda.current_stream().cuda_stream))
    return frames[:nbytes], frame_off, csum


def _check_varlen_encode(frames, frame_off, csum, w, where):
    same(host(frame_off), w["off"], "frame_off", where, w["enc_labels"] + ["end"])
    same(host(frames)[:len(w["frames"])], w["frames"], "frames", where, w["enc_labels"], off=w["off"])
    same(host(csum), w["csum"], "csum", where, w["enc_labels"])


def _varlen_encode_forms(cuda, w, layout, what, forms=VARLEN_ENCODE_FORMS, hints=VARLEN_ENCODE_HINTS, gathered=True):
    seq, ack, flags, pay, lens = w["tables"]
    n = len(lens)
    tab = (dev(seq, cuda), dev(ack, cuda), dev(flags, cuda))
    d_pay, d_lens = dev(pay, cuda), dev(lens, cuda)
    if gathered:  # the same payloads scattered through a bigger buffer, ragged alignment
        rng = np.random.default_rng(layout)
        gaps = rng.integers(0, 40, n)
        starts = (np.cumsum(gaps + lens) - lens).astype(np.int64)
        big = rng.integers(0, 256, int(starts[-1] + lens[-1]) + 64, dtype=np.uint8)
        at = np.concatenate([np.arange(s, s + k) for s, k in zip(starts, lens)])
        big[at] = pay
        d_big, d_starts = dev(big, cuda), dev(starts, cuda)
    for name, settings in forms:
        with knobs(settings) as lib:
            where = f"{what}, {name}, layout {layout}"
            r = batch.pack_batch_varlen(tab, d_pay, d_lens, layout, want_csum=True)
            _check_varlen_encode(r.frames, r.frame_off, r.csum, w, where + ", packed")
            if gathered:
                r = batch.pack_batch_varlen(tab, d_big, d_lens, layout, payload_off=d_starts, want_csum=True)
                _check_varlen_encode(r.frames, r.frame_off, r.csum, w, where + ", gathered")
            for hint in hints:
                out = _raw_encode_varlen(lib, cuda, tab, d_pay, d_lens, n, len(w["frames"]), hint, layout)
                _check_varlen_encode(*out, w, where + f", hint {hint}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_varlen_encode_forms(cuda, layout):
    for rot in range(1, len(cc.CLASSES)):  # every class as the first and as the last frame
        w = packed_want(layout, rot)
        _varlen_encode_forms(cuda, w, layout, f"varlen encode, rotation {rot}", forms=VARLEN_ENCODE_FORMS[:1], hints=(),
                             gathered=False)
    w = packed_want(layout, 0)
    _varlen_encode_forms(cuda, w, layout, "varlen encode")
    assert 65535 in w["tables"][4] and (w["csum"] == 0).any() and (w["csum"] == 0xFFFF).any()


# ------------------------------------------------------ variable-length decode
def _raw_decode_varlen(lib, cuda, d_buf, d_off, d_cs, n, hint, layout):
    import torch
    outs = [torch.full((n,), 0xAB, dtype=dt, device=cuda)
            for dt in (torch.uint16, torch.uint16, torch.uint8, torch.uint8, torch.uint16)]
    _native.check(lib.rudp_decode(d_buf.data_ptr(), d_off.data_ptr(), hint, n,
                                  d_cs.data_ptr() if d_cs is not None else None, *[o.data_ptr() for o in outs], None,
                                  layout, 0, torch.cuda.current_stream().cuda_stream))
    return dict(zip(FIELDS, (host(o) for o in outs)))


def _checked_decode_varlen(lib, cuda, d_buf, nbytes, d_off, d_cs, n, hint, layout):
    """rudp_decode_varlen_utf8 with its status word: the entry the span form serves."""
    import torch
    outs = [torch.full((n,), 0xAB, dtype=dt, device=cuda)
            for dt in (torch.uint16, torch.uint16, torch.uint8, torch.uint8, torch.uint16, torch.uint8)]
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _native.check(lib.rudp_decode_varlen_utf8(
        d_buf.data_ptr(), nbytes, d_off.data_ptr(), hint, n, d_cs.data_ptr() if d_cs is not None else None,
        *[o.data_ptr() for o in outs], status.data_ptr(), layout, 0, torch.cuda.current_stream().cuda_stream))
    assert int(status.item()) == 0
    return dict(zip(FIELDS + ("valid",), (host(o) for o in outs)))


def _check_fields(got, want, where, labels, valid=None):
    for k in FIELDS:
        same(got[k], want[k], k, where, labels)
    if valid is not None:
        same(got["valid"], valid, "valid", where, labels)


def _varlen_decode_forms(cuda, w, layout, what, full=True):
    n = len(w["labels"])
    d_buf, d_off = dev(w["wire"], cuda), dev(w["woff"], cuda)
    cases = [("in-band", None, "side")] if layout == 7 else \
        [("sideband", dev(w["carried"], cuda), "side"), ("no sideband", None, "noside")]
    for cname, d_cs, key in cases:
        where = f"{what}, {cname}, layout {layout}"
        d = batch.unpack_batch_varlen(d_buf, d_off, layout, csum=d_cs, utf8=True)
        _check_decoded(d, w[key], w["valid"], where + ", default", w["labels"])
        if not full:
            continue
        for name, settings in VARLEN_DECODE_FORMS:
            with knobs(settings) as lib:
                for hint in VARLEN_DECODE_HINTS:
                    got = _raw_decode_varlen(lib, cuda, d_buf, d_off, d_cs, n, hint, layout)
                    _check_fields(got, w[key], f"{where}, {name}, hint {hint}", w["labels"])
        for name, settings in SPAN_FORMS:
            with knobs(settings) as lib:
                for hint in SPAN_HINTS:
                    got = _checked_decode_varlen(lib, cuda, d_buf, len(w["wire"]), d_off, d_cs, n, hint, layout)
                    _check_fields(got, w[key], f"{where}, {name}, hint {hint}", w["labels"], w["valid"])
    if full:
        for shift in DECODE_VIEW_SHIFTS:  # the frames buffer as a view off the 16-byte grid
            fr = _view(w["wire"], shift, cuda)
            assert fr.data_ptr() % 16 == shift
            d = batch.unpack_batch_varlen(fr, d_off, layout, csum=cases[0][1], utf8=True)
            _check_decoded(d, w["side"], w["valid"], f"{what}, view shifted {shift}, layout {layout}", w["labels"])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_varlen_decode_forms(cuda, layout):
    for rot in range(1, len(cc.CLASSES)):
        _varlen_decode_forms(cuda, packed_want(layout, rot), layout, f"varlen decode, rotation {rot}", full=False)
    w = packed_want(layout, 0)
    _varlen_decode_forms(cuda, w, layout, "varlen decode")
    _classes_met(w["labels"], w["side"]["ok"], w["side"]["csum"])
    assert (w["side"]["ok"] == cc.OK_SHORT).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_frame_forms(cuda, layout):
    """The small-frame encode and decode tiles, on payloads of 0-8 bytes."""
    w = packed_want(layout, 0, "small")
    seq, ack, flags, pay, lens = w["tables"]
    assert pay.size // len(lens) < 16  # the hint that takes the small-frame tiles
    tab = (dev(seq, cuda), dev(ack, cuda), dev(flags, cuda))
    d_pay, d_lens = dev(pay, cuda), dev(lens, cuda)
    d_buf, d_off = dev(w["wire"], cuda), dev(w["woff"], cuda)
    d_cs = dev(w["carried"], cuda) if layout == 5 else None
    for name, settings in SMALL_FRAME_FORMS:
        where = f"small frames, {name}, layout {layout}"
        with knobs(settings):
            r = batch.pack_batch_varlen(tab, d_pay, d_lens, layout, want_csum=True, check=False).check()
            d = batch.unpack_batch_varlen(d_buf, d_off, layout, csum=d_cs, utf8=True, check=False).check()
        _check_varlen_encode(r.frames, r.frame_off, r.csum, w, where)
        _check_decoded(d, w["side"], w["valid"], where, w["labels"])
    _classes_met(w["labels"], w["side"]["ok"], w["side"]["csum"])


# --------------------------------------------------------------- maximum length
@pytest.mark.parametrize("L", cc.MAX_LENGTHS)
def test_maximum_length_forms(cuda, L):
    """TOP, ZK, FOLD2 and the ZK twins at payloads of 65520 and 65535 bytes, through
    the fixed-length entries (default forms and shifted views; the fixed tiles
    stop at 4096) and every variable-length form."""
    for layout in LAYOUTS:
        w = fixed_want(L, layout, 0)
        tab, pay = _fixed_inputs(w, cuda)
        fr, cs = batch.pack_batch(tab, pay, layout, want_csum=True)
        _check_fixed_encode(fr, cs, w, f"fixed encode, default, layout {layout}, L {L}")
        _fixed_encode_views(cuda, w, layout, f"fixed encode, layout {layout}, L {L}")
        _fixed_decode_all(cuda, w, layout, L, [], "default")
        _classes_met(w["labels"], w["side"]["ok"], w["side"]["csum"])
        pw = packed_want(layout, 0, L)
        _varlen_encode_forms(cuda, pw, layout, f"varlen encode, L {L}", gathered=False)
        _varlen_decode_forms(cuda, pw, layout, f"varlen decode, L {L}")


# ----------------------------------------------------------------- host entries
def _pinned(a):
    import torch
    t = torch.empty(a.shape, dtype=getattr(torch, a.dtype.name), pin_memory=True)
    out = t.numpy()
    out[...] = a
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_entries(cuda, layout):
    """rudp_encode_host, rudp_decode_host, rudp_encode_varlen_host and
    rudp_decode_varlen_host on one fixed and one packed batch, pageable and
    pinned memory, the varlen decode's outputs stored direct or copied."""
    for mem in (np.ascontiguousarray, _pinned):
        where = f"host, {'pinned' if mem is _pinned else 'pageable'}, layout {layout}"
        w = fixed_want(17, layout)
        b = w["batch"]
        fr, cs = batch.pack_batch(tuple(mem(x) for x in (b.seq, b.ack, b.flags)), mem(b.payload), layout,
                                  want_csum=True)
        same(fr, w["frames"], "frames", where + " fixed encode", w["labels"])
        same(cs, w["csum"], "csum", where + " fixed encode", w["labels"])
        d = batch.unpack_batch(mem(w["wire"]), layout, csum=mem(w["carried"]) if layout == 5 else None,
                               copy_payload=True, utf8=True)
        for k in FIELDS:
            same(getattr(d, k), w["side"][k], k, where + " fixed decode", w["labels"])
        same(d.valid, w["valid"], "valid", where + " fixed decode", w["labels"])
        same(d.payload, b.payload, "payload", where + " fixed decode", w["labels"])
        w = packed_want(layout, 0)
        seq, ack, flags, pay, lens = (mem(x) for x in w["tables"])
        for name, settings in [("default", [])] + HOST_FORMS:
            with knobs(settings) as lib:
                r = batch.pack_batch_varlen((seq, ack, flags), pay, lens, layout, want_csum=True)
                d = batch.unpack_batch_varlen(mem(w["wire"]), mem(w["woff"]), layout,
                                              csum=mem(w["carried"]) if layout == 5 else None, utf8=True)
                # pageable outputs through the raw entry (copied whatever the knob)
                n = len(w["labels"])
                pg = {k: np.full(n, 0xAB, dt) for k, dt in zip(FIELDS + ("valid",), (
                    np.uint16, np.uint16, np.uint8, np.uint8, np.uint16, np.uint8))}
                st = np.zeros(1, np.uint32)
                wire, woff = mem(w["wire"]), mem(w["woff"])
                side = mem(w["carried"]) if layout == 5 else None
                rc = lib.rudp_decode_varlen_host(wire.ctypes.data, wire.size, woff.ctypes.data, 0, n,
                                                 side.ctypes.data if side is not None else None,
                                                 *[pg[k].ctypes.data for k in ("seq", "ack", "flags", "ok", "csum",
                                                                               "valid")], st.ctypes.data, layout, 0)
                assert rc == 0 and st[0] == 0
            tag = f"{where}, {name}"
            same(r.frame_off, w["off"], "frame_off", tag, w["enc_labels"] + ["end"])
            same(r.frames, w["frames"], "frames", tag, w["enc_labels"], off=w["off"])
            same(r.csum, w["csum"], "csum", tag, w["enc_labels"])
            for k in FIELDS:
                same(getattr(d, k), w["side"][k], k, tag + " varlen decode", w["labels"])
                same(pg[k], w["side"][k], k, tag + " varlen decode, pageable outputs", w["labels"])
            same(d.valid, w["valid"], "valid", tag + " varlen decode", w["labels"])
            same(pg["valid"], w["valid"], "valid", tag + " varlen decode, pageable outputs", w["labels"])


# -------------------------------------------------------------- fused receivers
TEXTS = ("a", "é", "€")  # 1, 2 and 3 bytes


def zk_stream(layout, n=200, isn=1000, fin=True, twin_every=10, seed=0):
    """A clean in-order stream of one- to three-character datagrams, every frame
    ZK (solved through ack, which the receiver's rule never reads), a twin of
    every ``twin_every``-th frame directly before it.  Returns the frames and
    the index of every true frame."""
    rng = random.Random(seed + layout)
    frames, true_at, sent = [], [], 0
    for k in range(n):
        text = "".join(rng.choice(TEXTS) for _ in range(rng.randint(1, 3)))
        flags = (SYN if k == 0 else 0) | (FIN if fin and k == n - 1 else 0)
        fr = cc.zk_datagram((isn + sent) & 0xFFFF, flags, text, layout)
        if k % twin_every == 0:
            frames.append(fr._replace(label="ZK_T"))
        true_at.append(len(frames))
        frames.append(fr)
        sent += len(text)
    return frames, true_at


def _decode_columns(frames, H):
    cols = list(zip(*(cc.expected_decode(f, H, True) for f in frames)))
    return {k: np.array(c, d) for k, c, d in zip(FIELDS, cols, (np.uint16, np.uint16, np.uint8, np.uint8, np.uint16))}


def _reply_want(acks, H):
    """The reply datagrams (seq 0, ack, ACK, no payload) and their checksums, from ref_csum."""
    parts = [cc.make_frame(0, int(a), 0x40, b"", H) for a in acks]
    cs = np.array([cc.ref_csum(p, H)[0] for p in parts], np.uint16)
    return np.frombuffer(b"".join(parts), np.uint8), cs


def receive_want(frames, H, state=(0, 0, 0)):
    """Every output of rudp_receive for the stream, from ref_decode and accept_ref."""
    wire, off, _ = cc.stream_wire(frames, H)
    w = _decode_columns(frames, H)
    w["csum_out"] = w.pop("csum")
    n = len(frames)
    w["valid"] = _valid_of(frames)
    w["usable"] = (((w["ok"] == 1) | (w["ok"] == 3)) & (w["valid"] == 1)).astype(np.uint8)
    w["chars"] = chars_ref(wire, off, H)
    r = accept_ref(w["seq"], w["flags"], w["chars"], w["usable"], state)
    w.update(accept=r.accept, keep=r.keep, reply=r.reply, reply_ack=r.reply_ack)
    kept = [f.payload if r.keep[i] else b"" for i, f in enumerate(frames)]
    w["payload_off"] = np.concatenate([[0], np.cumsum([len(p) for p in kept])]).astype(np.uint64)
    w["payload"] = np.frombuffer(b"".join(kept), np.uint8)
    idx, peer, last = [], [], n
    for i in range(n):
        if w["usable"][i] and w["flags"][i] & SYN:
            last = i
        if r.reply[i]:
            idx.append(i)
            peer.append(last)
    w["reply_index"], w["reply_peer"] = np.array(idx, np.uint32), np.array(peer, np.uint64)
    w["reply_frames"], w["reply_csum"] = _reply_want(r.reply_ack[idx], H)
    first = accept_scan_model(w["seq"], w["flags"], w["chars"], w["usable"], state).first_anomaly
    w["state"] = [r.state[0], r.state[1], 1 if r.state[2] else 0, 0]
    w["info"] = [r.end, r.count, r.msg_start, r.characters, first, len(idx), len(w["payload"]), 0]
    return w


def _receive_both_forms(cuda, frames, H, state, where):
    import test_gpu_receive as rx
    wire, off, side = cc.stream_wire(frames, H)
    labels = [f.label for f in frames]
    case = rx.Case(cuda, wire, off, H, csum=side if H == 5 else None, state=state)
    assert case.n <= rx.T and case.nbytes <= rx.FB and case.nbytes <= rx.MEAN * case.n  # both forms take it
    want = receive_want(frames, H, state)

    def one(form):
        got = case.check(form)  # (equal to the chain of separate calls, nothing written outside)
        tag = f"{where}, {form}, layout {H}"
        for name, _ in rx.TABLES[:12]:
            same(got[name], want[name], name, tag, labels)
        same(got["payload_off"], want["payload_off"], "payload_off", tag, labels + ["end"])
        total, R = len(want["payload"]), len(want["reply_index"])
        assert np.array_equal(got["payload"][:total], want["payload"]), tag
        assert got["state_out"].tolist() == want["state"] and got["info"].tolist() == want["info"], tag
        assert int(got["status"][0]) == 0, tag
        rl = [labels[i] for i in want["reply_index"]]
        same(got["reply_index"][:R], want["reply_index"], "reply_index", tag, rl)
        same(got["reply_peer"][:R], want["reply_peer"], "reply_peer", tag, rl)
        same(got["reply_csum"][:R], want["reply_csum"], "reply_csum", tag, rl)
        same(got["reply_frames"][:R * H].reshape(R, H), want["reply_frames"].reshape(R, H), "reply_frames", tag, rl)
    rx._forms(one)
    return want, labels


@pytest.mark.parametrize("H", LAYOUTS)
def test_receive_zk_stream(cuda, H):
    """rudp_receive, fused and chained, on a stream whose every frame has the
    checksum 0x0000, with twins carrying 0xFFFF before every tenth frame."""
    frames, true_at = zk_stream(H)
    want, labels = _receive_both_forms(cuda, frames, H, (0, 0, 0), "receive")
    twins = np.array([lab == "ZK_T" for lab in labels])
    assert twins.sum() == 20 and (want["csum_out"] == 0).all()
    assert (want["ok"][twins] == cc.OK_BAD_CSUM).all() and (want["ok"][~twins] == cc.OK_GOOD).all()
    assert not want["usable"][twins].any() and not want["accept"][twins].any() and not want["reply"][twins].any()
    assert want["usable"][true_at].all() and want["accept"][true_at].all() and want["reply"][true_at].all()
    assert want["info"][0] == len(frames) - 1  # the FIN frame ends it


REPLY_STATE = (49149, 49000, 1)  # the next three characters draw the acks 49150, 49151 = 0xBFFF and 49152


def _reply_stream(H):
    return [cc.zk_datagram(49149 + k, 0, "a", H) for k in range(3)]


@pytest.mark.parametrize("H", LAYOUTS)
def test_receive_reply_with_checksum_zero(cuda, H):
    """The reply for ack_num 0xBFFF has S = 0xFFFF: its checksum is 0x0000 (in-band 00 00)."""
    want, _ = _receive_both_forms(cuda, _reply_stream(H), H, REPLY_STATE, "receive replies")
    assert want["reply_ack"].tolist() == [49150, 49151, 49152] and want["reply_csum"][1] == 0x0000
    assert cc.ref_csum(cc.make_frame(0, 0xBFFF, 0x40, b"", H), H) == (0x0000, 0xFFFF)
    if H == 7:
        assert bytes(want["reply_frames"][7:14]) == bytes.fromhex("0000bfff400000")


def _window_case(cuda, frames, H, Wc, state):
    import test_gpu_receive_window as rw
    wire, off, side = cc.stream_wire(frames, H)
    none = (np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint16))
    return rw, rw.Case(cuda, none, (wire, off, side), H, Wc, side=H == 5, state=state)


def _window_both_forms(cuda, frames, H, Wc, state, where):
    """rudp_receive_window in both forms against receive_window_ref (the existing
    restatement), whose decode columns are held to ref_decode here."""
    rw, case = _window_case(cuda, frames, H, Wc, state)
    labels = [f.label for f in frames]
    total = sum(case.nbytes)
    assert case.n <= 1024 and total <= rw.FB and total <= rw.MEAN * case.n  # both forms take it
    want = case.check_forms()
    tag = f"{where}, layout {H}, window {Wc}"
    for k, v in _decode_columns(frames, H).items():
        same(want["csum_out" if k == "csum" else k], v, k, tag + " (the restatement)", labels)
    R = want["R"]
    fr, cs = _reply_want(want["reply_ack"][want["reply_index"]], H)
    same(want["reply_csum"], cs, "reply_csum", tag + " (the restatement)", [labels[i] for i in want["reply_index"]])
    assert np.array_equal(want["reply_frames"], fr) and R == len(cs), tag
    return want, labels


@pytest.mark.parametrize("Wc", [1, 8])
@pytest.mark.parametrize("H", LAYOUTS)
def test_receive_window_zk_stream(cuda, H, Wc):
    frames, true_at = zk_stream(H, fin=False)
    # one frame ahead of a lost two-character datagram: pending inside a window of 8, refused by a window of 1
    sent = sum(len(frames[i].payload.decode()) for i in true_at)
    ahead = cc.zk_datagram((1000 + sent + 2) & 0xFFFF, 0, "é", H)
    frames.append(ahead)
    want, labels = _window_both_forms(cuda, frames, H, Wc, (0, 0, 0), "receive_window")
    twins = np.array([lab == "ZK_T" for lab in labels])
    assert twins.sum() == 20 and (want["csum_out"] == 0).all()
    assert (want["ok"][twins] == cc.OK_BAD_CSUM).all() and (want["ok"][~twins] == cc.OK_GOOD).all()
    assert not want["usable"][twins].any() and not want["accept"][twins].any() and not want["reply"][twins].any()
    assert (want["accept"][true_at] == 1).all() and want["reply"][true_at].all()
    if Wc == 8:
        assert want["accept"][-1] == 2 and want["P"] == 1
        assert bytes(want["carry_frames"]) == cc.wire_bytes(ahead, H)
        if H == 5:
            assert want["carry_csum"].tolist() == [0x0000]
    else:
        assert want["accept"][-1] == 0 and want["P"] == 0


@pytest.mark.parametrize("H", LAYOUTS)
def test_receive_window_reply_with_checksum_zero(cuda, H):
    want, _ = _window_both_forms(cuda, _reply_stream(H), H, 8, REPLY_STATE, "receive_window replies")
    assert want["reply_ack"].tolist() == [49150, 49151, 49152] and want["reply_csum"].tolist()[1] == 0x0000
    if H == 7:
        assert bytes(want["reply_frames"][7:14]) == bytes.fromhex("0000bfff400000")


# ------------------------------------------------------------------ acknowledge
def zk_replies(H, isn, T_, fin_seq):
    """The receiver's replies to a transfer of T_ one-character frames as
    header-only ZK frames solved through seq (ack is what the rule reads), a
    twin directly before every tenth, then its FIN|ACK with seq ``fin_seq``."""
    frames = []
    for k in range(T_):
        fr = cc.zk_datagram(0, 0x40, "", H, field="seq", other=(isn + k + 1) & 0xFFFF)
        if k % 10 == 0:
            frames.append(fr._replace(label="ZK_T"))
        frames.append(fr)
    frames.append(cc.Frame("FIN", fin_seq, (isn + T_) & 0xFFFF, 0x60, b""))
    return frames


def _acknowledge_both_forms(cuda, frames, H, isn, T_, where):
    """rudp_acknowledge, fused and chained, against ref_decode and the rule (ack_ref).
    Returns the decode columns, the usable column, the rule's result and its tables."""
    import test_gpu_acknowledge as ta
    from ack_ref import EXACT
    labels = [f.label for f in frames]
    wire, off, side = cc.stream_wire(frames, H)
    case = ta.Case(cuda, None, H, isn=isn, T_=T_, C=1, mode=EXACT, frames=(wire, off, side))
    assert case.n <= ta.T and case.nbytes <= ta.FB and case.nbytes <= ta.MEAN * case.n  # both forms take it
    cols = _decode_columns(frames, H)
    usable = ((cols["ok"] == 1) | (cols["ok"] == 3)).astype(np.uint8)
    r, rule = ta.expect(cols["seq"], cols["ack"], cols["flags"], usable, isn=isn, T_=T_, C=1,
                        state=case.kw["state"], mode=EXACT)
    final = cc.make_frame(*r.final, 0x40, b"", H) if r.final else None

    def one(form):
        got = case.check(form)  # (equal to the chain of separate calls and to the rule)
        tag = f"{where}, {form}, layout {H}"
        for k in FIELDS:
            same(got["csum_out" if k == "csum" else k], cols[k], k, tag, labels)
        same(got["usable"], usable, "usable", tag, labels)
        for k in ("valid", "pointer", "state_out", "info"):
            assert np.array_equal(got[k], rule[k]), (tag, k)
        if final is not None:
            assert bytes(got["final_frame"]) == final, (tag, bytes(got["final_frame"]).hex(), final.hex())
            assert int(got["final_csum"][0]) == cc.ref_csum(final, H)[0], tag
    ta._forms(one)
    return cols, usable, r, rule


@pytest.mark.parametrize("closing", ["zk", "wrap", "fold2"])
@pytest.mark.parametrize("H", LAYOUTS)
def test_acknowledge_zk_replies(cuda, H, closing):
    """rudp_acknowledge, fused and chained: replies with checksum 0x0000 and
    their twins, then the closing datagram (seq = isn + p, ack = the FIN
    reply's seq + 1, flags ACK) at three edges, set through the FIN reply's
    seq: its sum a multiple of 0xFFFF ('zk'); its ack_num wrapping to 0 behind
    a FIN reply of seq 0xFFFF ('wrap'); its sum 0xFFFF + 0xC000 + 0x4000 =
    0x1FFFF, the smallest that needs the second fold ('fold2')."""
    T_ = 40
    isn = 0xFFFF - T_ if closing == "fold2" else 3611
    closing_seq = (isn + T_) & 0xFFFF
    closing_ack = {"zk": cc.solve(closing_seq, 0, 0x40, b"", H, 0, "ack"), "wrap": 0, "fold2": 0xC000}[closing]
    frames = zk_replies(H, isn, T_, (closing_ack - 1) & 0xFFFF)
    labels = [f.label for f in frames]
    cols, usable, r, rule = _acknowledge_both_forms(cuda, frames, H, isn, T_, f"acknowledge, closing {closing}")
    assert r.final == (closing_seq, closing_ack) and r.done and r.end == len(frames) - 1
    final_csum, S = cc.ref_csum(cc.make_frame(closing_seq, closing_ack, 0x40, b"", H), H)
    if closing == "zk":
        assert final_csum == 0 and S > 0 and S % 0xFFFF == 0
    elif closing == "fold2":
        assert S == 0x1FFFF and final_csum == 0xFFFE
    twins = np.array([lab == "ZK_T" for lab in labels])
    assert twins.sum() == 4 and (cols["csum"][:-1] == 0).all()
    assert (cols["ok"][twins] == cc.OK_BAD_CSUM).all() and not rule["valid"][twins].any()
    assert rule["valid"][~twins].all()


@pytest.mark.parametrize("H", LAYOUTS)
def test_fused_receivers_decode_every_class(cuda, H):
    """The one-lane-per-frame decode of rudp_receive, rudp_receive_window and
    rudp_acknowledge (and their chained forms) over the small-frame corpus:
    every class, the twins and frames shorter than the header, whatever the
    protocol rules then make of their random sequence numbers and flags."""
    w = packed_want(H, 0, "small")
    frames = w["batch"].frames
    want, labels = _receive_both_forms(cuda, frames, H, (0, 0, 0), "receive, corpus")
    _classes_met(labels, want["ok"], want["csum_out"])
    same(want["ok"], w["side"]["ok"], "ok", "receive, corpus", labels)
    want, _ = _window_both_forms(cuda, frames, H, 8, (0, 0, 0), "receive_window, corpus")
    _classes_met(labels, want["ok"], want["csum_out"])
    cols, _, _, _ = _acknowledge_both_forms(cuda, frames, H, 3611, 40, "acknowledge, corpus")
    _classes_met(labels, cols["ok"], cols["csum"])
    assert (cols["ok"] == cc.OK_SHORT).any() and {"FOLD2", "NEAR1", "NEARM", "TOP", "PE", "PO"} <= set(labels)
