"""Every byte-offset path across the 2^31 and 2^32 byte lines.

include/rudp.h promises 64-bit offsets and sizes everywhere, and the kernels mix
uint64_t buffer offsets with uint32_t tile-relative ones on purpose; one
(uint32_t) in the wrong place would frame or parse the wrong bytes only for
buffers nobody else here allocates.  Three constructions (tests/large_offsets.py
holds their CPU side, tests/test_large_offsets_ref.py checks it):

1. *Translated input.*  A block of a few thousand datagrams whose answers come
   from the plain restatements is copied to [base, base + B) of one 4 GiB + 2 MiB
   buffer (never filled as a whole) so that 2^31, then 2^32, falls inside one
   frame's payload, and every call that reads packed frames gets frame_off +
   base and frames_bytes = the buffer's size.  Every output equals the CPU
   reference, which makes it bit for bit the base-0 control's.  The line keeps
   16 bytes from either end of its frame, except in the block of one-character
   datagrams (6 to 11 bytes each), where it lies on a payload byte.
2. *Translated source.*  The gathered encode with payload_off pointing into the
   same buffer at the two bases; and 66 000 packets of 65 535 B gathered from
   one 64 KiB pool, whose output crosses both lines.
3. *Dense periodic batches.*  An oracle-checked block repeated on the device
   until input, output and the scanned offsets pass 2^32; the expected output is
   the block's repeated, offsets advanced by r * B, compared on the device in
   row chunks.

Then offsets that only look valid in 32 bits, in tiny buffers: each is rejected
as the header says, and poisoning the aliased low bytes changes no output.

All calls go through the C ABI with an explicit len_hint, each case at the
block's true mean frame length (the product's geometry) and at 0.  Every
comparison is bit-exact.

Out of scope: single frames longer than 2^31 bytes (one frame is walked by one
lane group: minutes, not seconds); the *_host entry points (they would need
4 GiB of pinned host memory); n at or above 2^32.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

import large_offsets as lo
from large_offsets import BIG_BYTES, LINE32, compare_periodic
from oracle import codec_np
from rudp import _native

pytestmark = pytest.mark.gpu

PAD, SENT = 16, 0xA5
PEAK_LIMIT = 32 << 30
NO_ISN = 0xFFFFFFFF


# ----------------------------------------------------------------- fixtures
class Big:
    """The translated-input buffer; `t` is dropped at module teardown."""
    t = None


@pytest.fixture(scope="module")
def big(cuda):
    import torch
    b = Big()
    b.t = torch.empty(BIG_BYTES, dtype=torch.uint8, device=cuda)
    yield b
    b.t = None
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _memory(cuda):
    """Every test starts from a fresh peak counter, stays under 32 GiB and
    leaves nothing cached."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"peak device memory: {peak / 2**30:.2f} GiB")
    assert peak < PEAK_LIMIT, peak


# ------------------------------------------------------------------ helpers
def dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)


class Out:
    """An output array between sentinel guards."""

    def __init__(self, cuda, count, dtype):
        import torch
        self.dt = np.dtype(dtype)
        self.t = torch.full((2 * PAD + count * self.dt.itemsize,), SENT, dtype=torch.uint8, device=cuda)

    @property
    def ptr(self):
        return self.t.data_ptr() + PAD

    def get(self, name=""):
        a = self.t.cpu().numpy()
        assert (a[:PAD] == SENT).all() and (a[len(a) - PAD:] == SENT).all(), ("guard", name)
        return a[PAD:len(a) - PAD].view(self.dt)


def same(got, want, *tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, tag + (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), tag + (bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


def untouched(a):
    return bool((np.asarray(a).view(np.uint8) == SENT).all())


class Placed:
    """Packed frames on the device: in a buffer of their own (the control) or
    at `base` of the large one, offsets translated."""

    def __init__(self, cuda, big, buf, off, base, own, csum=None):
        self.cuda, self.n = cuda, len(off) - 1
        if own:
            self.hold = dev(cuda, buf)
            self.ptr, self.nbytes = self.hold.data_ptr(), len(buf)
        else:
            big.t[base:base + len(buf)].copy_(dev(cuda, buf))
            self.ptr, self.nbytes = big.t.data_ptr(), BIG_BYTES
        self.np_off = lo.translate(off, base)
        self.off = dev(cuda, self.np_off)
        self.csum = None if csum is None else dev(cuda, csum)


@functools.lru_cache(maxsize=None)
def block_and_answers(kind, H):
    b = lo.make_block(kind, H)
    return b, lo.block_expect(b, sideband=H == 5)


# ----------------------------------------------------- the calls, one by one
def call_decode(pl, hint, H, *, utf8, sideband, lim=None):
    cuda, n = pl.cuda, pl.n
    o = {k: Out(cuda, n, t) for k, t in (("seq", np.uint16), ("ack", np.uint16), ("flags", np.uint8),
                                         ("ok", np.uint8), ("csum", np.uint16), ("valid", np.uint8))}
    st = Out(cuda, 1, np.uint32)
    cs = pl.csum.data_ptr() if sideband else None
    lim = pl.nbytes if lim is None else lim
    lib = _native.lib()
    if utf8:
        _native.check(lib.rudp_decode_varlen_utf8(pl.ptr, lim, pl.off.data_ptr(), hint, n, cs, o["seq"].ptr,
                                                  o["ack"].ptr, o["flags"].ptr, o["ok"].ptr, o["csum"].ptr,
                                                  o["valid"].ptr, st.ptr, H, 0, None))
    else:
        _native.check(lib.rudp_decode_varlen_checked(pl.ptr, lim, pl.off.data_ptr(), hint, n, cs, o["seq"].ptr,
                                                     o["ack"].ptr, o["flags"].ptr, o["ok"].ptr, o["csum"].ptr,
                                                     st.ptr, H, 0, None))
    got = {k: v.get(k) for k, v in o.items()}
    if not utf8:
        assert untouched(got.pop("valid"))
    got["status"] = int(st.get()[0])
    return got


def call_validate(pl, hint, H):
    v = Out(pl.cuda, pl.n, np.uint8)
    _native.check(_native.lib().rudp_validate_utf8(pl.ptr, pl.off.data_ptr(), hint, pl.n, H, v.ptr, 0, None))
    return v.get("valid")


def call_chars(pl, hint, H, lim=None):
    c = Out(pl.cuda, pl.n, np.uint32)
    _native.check(_native.lib().rudp_payload_chars(pl.ptr, pl.nbytes if lim is None else lim, pl.off.data_ptr(), hint,
                                                   pl.n, c.ptr, H, 0, None))
    return c.get("chars")


def call_gather(pl, hint, H, keep, cap, lim=None):
    """(payload with its guard room, payload_off, status); cap bytes of room."""
    cuda = pl.cuda
    pay, poff, st = Out(cuda, cap, np.uint8), Out(cuda, pl.n + 1, np.uint64), Out(cuda, 1, np.uint32)
    k = None if keep is None else dev(cuda, keep)
    _native.check(_native.lib().rudp_gather_payloads(pl.ptr, pl.nbytes if lim is None else lim, pl.off.data_ptr(), hint,
                                                     pl.n, None if k is None else k.data_ptr(), pay.ptr, cap, poff.ptr,
                                                     st.ptr, H, 0, None))
    return pay.get("payload"), poff.get("payload_off"), int(st.get()[0])


def call_ordered(pl, hint, rank, K, skip, cap, lim=None, d_rank=None, d_count=None):
    cuda, n = pl.cuda, pl.n
    out, ooff, src, st = Out(cuda, cap, np.uint8), Out(cuda, n + 1, np.uint64), Out(cuda, n, np.uint32), \
        Out(cuda, 1, np.uint32)
    if d_rank is None:
        hold = (dev(cuda, np.asarray(rank, np.uint32).view(np.int32)), dev(cuda, np.array([K], np.int64)))
        d_rank, d_count = hold[0].data_ptr(), hold[1].data_ptr()
    _native.check(_native.lib().rudp_gather_ordered(pl.ptr, pl.nbytes if lim is None else lim, pl.off.data_ptr(), hint,
                                                    n, d_rank, d_count, skip, out.ptr, cap, ooff.ptr, src.ptr, st.ptr,
                                                    0, None))
    return out.get("out"), ooff.get("out_off"), src.get("src"), int(st.get()[0])


def check_ordered(got, want, n, *tag):
    out, ooff, src, st = got
    w_out, w_off, w_src, w_st = want
    K = len(w_src)
    assert st == w_st, tag + (st, w_st)
    same(ooff[:K + 1], w_off.astype(np.uint64), "out_off", *tag)
    assert untouched(ooff[K + 1:]) and untouched(src[K:]), tag
    same(src[:K], np.where(w_src < 0, lo.NONE, w_src).astype(np.uint32), "src", *tag)
    same(out[:len(w_out)], w_out, "out", *tag)
    assert untouched(out[len(w_out):]), tag  # nothing at or past the total


def call_dedup(pl, hint, window, checked, lim=None):
    d = Out(pl.cuda, pl.n, np.uint8)
    lib = _native.lib()
    if checked:
        _native.check(lib.rudp_dedup_window_checked(pl.ptr, pl.nbytes if lim is None else lim, pl.off.data_ptr(), hint,
                                                    pl.n, window, d.ptr, 0, None))
    else:
        _native.check(lib.rudp_dedup_window(pl.ptr, pl.off.data_ptr(), hint, pl.n, window, d.ptr, 0, None))
    return d.get("dup")


def call_off_check(pl, lim):
    st = Out(pl.cuda, 1, np.uint32)
    _native.check(_native.lib().rudp_frame_off_check(pl.off.data_ptr(), pl.n, lim, st.ptr, 0, None))
    return int(st.get()[0])


def call_off_bounds(pl):
    h = np.full(3, -1, np.int64)
    _native.check(_native.lib().rudp_frame_off_bounds(pl.off.data_ptr(), pl.n, h.ctypes.data, 0, None))
    return h.tolist()


RECV = dict(seq=np.uint16, ack=np.uint16, flags=np.uint8, ok=np.uint8, csum_out=np.uint16, valid=np.uint8,
            usable=np.uint8, chars=np.uint32, accept=np.uint8, keep=np.uint8, reply=np.uint8, reply_ack=np.uint16,
            reply_csum=np.uint16, reply_index=np.uint32, reply_peer=np.uint64)


def call_receive(pl, hint, H, sideband, cap):
    import torch
    cuda, n = pl.cuda, pl.n
    o = {k: Out(cuda, n, t) for k, t in RECV.items()}
    o.update(payload_off=Out(cuda, n + 1, np.uint64), state_out=Out(cuda, 4, np.uint64), info=Out(cuda, 8, np.uint64),
             status=Out(cuda, 1, np.uint32), payload=Out(cuda, cap, np.uint8), reply_frames=Out(cuda, n * H, np.uint8))
    st_in = torch.zeros(4, dtype=torch.int64, device=cuda)
    r = _native.RudpReceived(payload_cap=cap, **{k: v.ptr for k, v in o.items()})
    _native.check(_native.lib().rudp_receive(pl.ptr, pl.nbytes, pl.off.data_ptr(), hint, n,
                                             pl.csum.data_ptr() if sideband else None, NO_ISN, st_in.data_ptr(), r, H, 0,
                                             None))
    return {k: v.get(k) for k, v in o.items()}


def check_receive(got, w, n, *tag):
    r = w["receive"]
    for k in ("seq", "ack", "flags", "ok", "valid", "chars"):
        same(got[k], w[k], "receive", k, *tag)
    same(got["csum_out"], w["csum"], "receive", "csum_out", *tag)
    for k in ("usable", "accept", "keep", "reply", "reply_ack", "state_out", "info", "payload_off"):
        same(got[k], r[k], "receive", k, *tag)
    assert int(got["status"][0]) == 0, tag
    total, R = len(r["payload"]), len(r["reply_index"])
    same(got["payload"][:total], r["payload"], "receive", "payload", *tag)
    assert untouched(got["payload"][total:]), tag
    for k in ("reply_csum", "reply_index", "reply_peer"):
        same(got[k][:R], r[k], "receive", k, *tag)
        assert untouched(got[k][R:]), (k,) + tag
    H = len(got["reply_frames"]) // n
    same(got["reply_frames"][:R * H], r["reply_frames"], "receive", "reply_frames", *tag)
    assert untouched(got["reply_frames"][R * H:]), tag


ACKD = dict(seq=np.uint16, ack=np.uint16, flags=np.uint8, ok=np.uint8, csum_out=np.uint16, usable=np.uint8,
            valid=np.uint8, pointer=np.uint64)


def call_acknowledge(pl, hint, H, sideband, T):
    import torch
    cuda, n = pl.cuda, pl.n
    o = {k: Out(cuda, n, t) for k, t in ACKD.items()}
    o.update(state_out=Out(cuda, 4, np.uint64), info=Out(cuda, 8, np.uint64), final_frame=Out(cuda, H, np.uint8),
             final_csum=Out(cuda, 1, np.uint16), status=Out(cuda, 1, np.uint32))
    st_in = torch.tensor([int(v) for v in lo.fresh_state(T, lo.ACK_CHUNK)], dtype=torch.int64).to(cuda)
    a = _native.RudpAcknowledged(**{k: v.ptr for k, v in o.items()})
    _native.check(_native.lib().rudp_acknowledge(pl.ptr, pl.nbytes, pl.off.data_ptr(), hint, n,
                                                 pl.csum.data_ptr() if sideband else None, lo.ACK_ISN, T, lo.ACK_CHUNK,
                                                 _native.ACK_CUMULATIVE, T, st_in.data_ptr(), a, H, 0, None))
    return {k: v.get(k) for k, v in o.items()}


def check_acknowledge(got, w, *tag):
    a = w["acknowledge"]
    for k in ("seq", "ack", "flags", "ok"):
        same(got[k], w[k], "acknowledge", k, *tag)
    same(got["csum_out"], w["csum"], "acknowledge", "csum_out", *tag)
    for k in ("usable", "valid", "pointer", "state_out", "info"):
        same(got[k], a[k], "acknowledge", k, *tag)
    assert int(got["status"][0]) == 0, tag
    if a["final_frame"] is None:
        assert untouched(got["final_frame"]) and untouched(got["final_csum"]), tag
    else:
        same(got["final_frame"], a["final_frame"], "acknowledge", "final_frame", *tag)
        assert int(got["final_csum"][0]) == a["final_csum"], tag


def call_window(pl, hint, H, w, cap):
    """rudp_accept_window over the decode's tables, then rudp_gather_ordered of
    its ranks with the count read on the device: what receive_window chains."""
    import torch
    cuda, n = pl.cuda, pl.n
    d = [dev(cuda, w["seq"]), dev(cuda, w["flags"]), dev(cuda, w["chars"].view(np.int32)),
         dev(cuda, w["receive"]["usable"])]
    o = dict(accept=Out(cuda, n, np.uint8), rank=Out(cuda, n, np.uint32), carry_rank=Out(cuda, n, np.uint32),
             reply=Out(cuda, n, np.uint8), reply_ack=Out(cuda, n, np.uint16), state_out=Out(cuda, 4, np.uint64),
             info=Out(cuda, 8, np.uint64))
    st_in = torch.zeros(4, dtype=torch.int64, device=cuda)
    _native.check(_native.lib().rudp_accept_window(
        d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, NO_ISN, lo.WINDOW_CHARS, 0,
        st_in.data_ptr(), o["accept"].ptr, o["rank"].ptr, o["carry_rank"].ptr, o["reply"].ptr, o["reply_ack"].ptr,
        o["state_out"].ptr, o["info"].ptr, 0, None))
    msg = call_ordered(pl, hint, None, None, H, cap, d_rank=o["rank"].ptr, d_count=o["info"].ptr + 8)
    return {k: v.get(k) for k, v in o.items()}, msg


def check_window(got, msg, w, n, *tag):
    res = w["window"]["res"]
    for k in ("accept", "rank", "carry_rank", "reply", "reply_ack"):
        same(got[k], getattr(res, k), "window", k, *tag)
    same(got["state_out"], np.array([res.state[0], res.state[1], res.state[2], 0], np.uint64), "window", *tag)
    info = got["info"].tolist()
    assert info[:4] == res.info[:4] and info[5:] == res.info[5:] and info[4] <= n, tag + (info, res.info)
    check_ordered(msg, w["window"]["message"], n, "window", *tag)
    return info[4]


# -------------------------------------------- 1. translated input, every reader
@pytest.mark.parametrize("H", [5, 7])
@pytest.mark.parametrize("kind", ["chars", "ragged", "long"])
def test_translated_input(cuda, big, kind, H):
    """Blocks (a) one-character datagrams, (b) ragged 0-2944 B payloads, (c) one
    200 000 B frame among small ones, at base 0 of their own buffer and across
    2^31 and 2^32 of the large one: every reader of packed frames equals the
    CPU reference at both hints."""
    b, w = block_and_answers(kind, H)
    n, sideband = b.n, H == 5
    plain = lo.decode_expect(b.buf, b.off, H, None) if sideband else w
    places = lo.placements(b.off, H, need_margin=kind != "chars", anchor=b.anchor)
    anomaly = {}
    for name, base in places:
        if name != "control":
            line = lo.LINE31 if name == "2^31" else LINE32
            i = lo.assert_line_inside(b.off, H, base, line, need_margin=kind != "chars")
            assert b.anchor is None or i == b.anchor
        pl = Placed(cuda, big, b.buf, b.off, base, name == "control", b.csum)
        B = len(b.buf)
        assert call_off_bounds(pl) == [base, base + B, 0], name
        assert call_off_check(pl, pl.nbytes) == 0, name
        assert call_off_check(pl, base + B - 1) == lo.ST_OFFSETS, name   # one byte short, wherever the block lies
        for hint in (b.mean, 0):
            tag = (kind, H, name, hint)
            got = call_decode(pl, hint, H, utf8=False, sideband=sideband)
            for k in ("seq", "ack", "flags", "ok", "csum"):
                same(got[k], w[k], "decode_varlen_checked", k, *tag)
            assert got["status"] == 0, tag
            got = call_decode(pl, hint, H, utf8=True, sideband=sideband)
            for k in ("seq", "ack", "flags", "ok", "csum", "valid"):
                same(got[k], w[k], "decode_varlen_utf8", k, *tag)
            if sideband:  # and without the sideband checksum
                got = call_decode(pl, hint, H, utf8=True, sideband=False)
                for k in ("seq", "ack", "flags", "ok", "csum", "valid"):
                    same(got[k], plain[k], "decode_varlen_utf8 without sideband", k, *tag)
            same(call_validate(pl, hint, H), w["valid"], "validate_utf8", *tag)
            same(call_chars(pl, hint, H), w["chars"], "payload_chars", *tag)
            pay, poff = w["gather"]
            g_pay, g_off, g_st = call_gather(pl, hint, H, w["keep_mask"], len(pay) + 64)
            assert g_st == 0, tag
            same(g_off, poff, "gather_payloads", "payload_off", *tag)
            same(g_pay[:len(pay)], pay, "gather_payloads", "payload", *tag)
            assert untouched(g_pay[len(pay):]), tag
            for skip in (0, H):
                want = w["ordered"][skip]
                check_ordered(call_ordered(pl, hint, w["rank"], w["K"], skip, len(want[0]) + 64), want, n,
                              "gather_ordered", skip, *tag)
            same(call_dedup(pl, hint, lo.WINDOW, True), w["dup"], "dedup_window_checked", *tag)
            same(call_dedup(pl, hint, lo.WINDOW, False), w["dup"], "dedup_window", *tag)
            check_receive(call_receive(pl, hint, H, sideband, len(w["receive"]["payload"]) + 64), w, n, *tag)
            check_acknowledge(call_acknowledge(pl, hint, H, sideband, w["acknowledge"]["T"]), w, *tag)
            got, msg = call_window(pl, hint, H, w, len(w["window"]["message"][0]) + 64)
            anomaly[(name, hint)] = check_window(got, msg, w, n, *tag)
        del pl
    assert len(set(anomaly.values())) == 1, anomaly  # (the one word the rule does not fix: the control's everywhere)


# the diagnostics build's other kernel forms of the readers: (rudpx_tune key, value), one at a time
FORMS = ((65, 0), (65, 1), (33, 0), (33, 2), (14, 0), (41, 0), (32, 0), (62, 0), (63, 0), (69, 0), (49, 0))


@pytest.mark.parametrize("H", [5, 7])
@pytest.mark.parametrize("kind", ["chars", "ragged", "long"])
def test_translated_input_alternative_forms(cuda, big, kind, H):
    """The decode, UTF-8, character-count, dedup and gather kernels the product
    does not pick (span / tile / vector / byte decode, the two dedup and
    validation forms, XCD order off), across both lines."""
    b, w = block_and_answers(kind, H)
    sideband = H == 5
    tools = _native.tools_lib(activate=True)
    pay, poff = w["gather"]
    for name, base in lo.placements(b.off, H, need_margin=kind != "chars", anchor=b.anchor)[1:]:
        pl = Placed(cuda, big, b.buf, b.off, base, False, b.csum)
        for key, value in FORMS:
            old = tools.rudpx_tune(key, value)
            try:
                for hint in (b.mean, 0):
                    tag = (kind, H, name, hint, "knob", key, value)
                    got = call_decode(pl, hint, H, utf8=True, sideband=sideband)
                    for k in ("seq", "ack", "flags", "ok", "csum", "valid"):
                        same(got[k], w[k], "decode_varlen_utf8", k, *tag)
                    same(call_validate(pl, hint, H), w["valid"], "validate_utf8", *tag)
                    same(call_chars(pl, hint, H), w["chars"], "payload_chars", *tag)
                    same(call_dedup(pl, hint, lo.WINDOW, True), w["dup"], "dedup_window_checked", *tag)
                    g_pay, g_off, g_st = call_gather(pl, hint, H, w["keep_mask"], len(pay) + 64)
                    same(g_off, poff, "gather_payloads", "payload_off", *tag)
                    same(g_pay[:len(pay)], pay, "gather_payloads", "payload", *tag)
            finally:
                tools.rudpx_tune(key, old)


# ----------------------------------------- 2. translated source for the encode
def encode_varlen(cuda, n, hint, tabs, payload_ptr, payload_bytes, d_len, d_poff, frames_ptr, frames_cap, H):
    """rudp_encode_varlen_checked; returns (frame_off Out, csum Out, status)."""
    off, cs, st = Out(cuda, n + 1, np.uint64), Out(cuda, n, np.uint16), Out(cuda, 1, np.uint32)
    batch = _native.RudpBatch(n=n, payload_len=hint, reserved=0, seq=tabs[0].data_ptr(), ack=tabs[1].data_ptr(),
                              flags=tabs[2].data_ptr(), payload=payload_ptr, len=d_len.data_ptr(),
                              payload_off=None if d_poff is None else d_poff.data_ptr())
    _native.check(_native.lib().rudp_encode_varlen_checked(ctypes.byref(batch), payload_bytes, frames_ptr, frames_cap,
                                                           off.ptr, cs.ptr, st.ptr, H, 0, None))
    return off, cs, st


def random_headers(rng, n):
    return (rng.integers(0, 65536, n).astype(np.uint16), rng.integers(0, 65536, n).astype(np.uint16),
            rng.integers(0, 256, n).astype(np.uint8))


@pytest.mark.parametrize("H", [5, 7])
@pytest.mark.parametrize("kind", ["chars", "ragged", "long"])
def test_encode_gathered_from_translated_source(cuda, big, kind, H):
    """payload_off[i] into the large buffer across 2^31 and 2^32, the frames
    into a small buffer: frames, offsets and checksums are the oracle's."""
    rng = np.random.default_rng(0xE7C0 + H)
    pays = lo.block_payloads(kind, random.Random(0xE7C0 + H))
    if kind == "long":
        pays[300] = pays[300][:65535]    # the longest payload a datagram of this protocol carries
    n = len(pays)
    seq, ack, flags = random_headers(rng, n)
    want, want_off, want_cs = codec_np.encode_varlen(seq, ack, flags, pays, H)
    lens = np.array([len(p) for p in pays], np.int32)
    poff = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    paybuf = np.frombuffer(b"".join(pays), np.uint8)
    tabs = [dev(cuda, a) for a in (seq, ack, flags)]
    d_len = dev(cuda, lens)
    for name, base in lo.placements(poff, 0, need_margin=kind != "chars", anchor=300 if kind == "long" else None):
        src = Placed(cuda, big, paybuf, poff, base, name == "control")
        d_poff = dev(cuda, src.np_off[:-1].copy())
        for hint in (len(paybuf) // n, 0):
            fr = Out(cuda, len(want) + 64, np.uint8)
            off, cs, st = encode_varlen(cuda, n, hint, tabs, src.ptr, src.nbytes, d_len, d_poff, fr.ptr, len(want), H)
            tag = (kind, H, name, hint)
            assert int(st.get()[0]) == 0, tag
            same(off.get(), want_off.astype(np.uint64), "frame_off", *tag)
            same(cs.get(), want_cs, "csum", *tag)
            got = fr.get()
            same(got[:len(want)], want, "frames", *tag)
            assert untouched(got[len(want):]), tag


POOL_N, POOL_LEN = 66_000, 65_535


def pool_batch(cuda, H):
    """66 000 packets of 65 535 B gathered from one 64 KiB pool: six distinct
    rows (three headers x two pool offsets), each framed by the oracle."""
    import torch
    rng = np.random.default_rng(0x9001 + H)
    pool = rng.integers(0, 256, 65536, dtype=np.uint8)
    seq, ack, flags = random_headers(rng, 3)
    j = np.arange(6)
    rows, cs = codec_np.encode(seq[j % 3], ack[j % 3], flags[j % 3],
                               np.stack([pool[k % 2:k % 2 + POOL_LEN] for k in j]), H)
    tabs = [dev(cuda, np.tile(a, POOL_N // 3)) for a in (seq, ack, flags)]
    d_len = torch.full((POOL_N,), POOL_LEN, dtype=torch.int32, device=cuda)
    d_poff = dev(cuda, np.arange(POOL_N, dtype=np.int64) % 2)
    return dev(cuda, pool), tabs, d_len, d_poff, rows, cs


@pytest.mark.parametrize("H", [5, 7])
def test_encode_output_crosses_input_does_not(cuda, H):
    """The gathered encode's frames and scanned offsets cross 2^31 and 2^32 while
    its payloads stay inside 64 KiB."""
    import torch
    pool, tabs, d_len, d_poff, rows, cs = pool_batch(cuda, H)
    F = POOL_LEN + H
    total = POOL_N * F
    assert total > LINE32 and lo.LINE31 % F and LINE32 % F
    frames = torch.empty(total, dtype=torch.uint8, device=cuda)
    for hint in (POOL_LEN, 0):
        frames.fill_(SENT)
        off, csum, st = encode_varlen(cuda, POOL_N, hint, tabs, pool.data_ptr(), 65536, d_len, d_poff,
                                      frames.data_ptr(), total, H)
        assert int(st.get()[0]) == 0, hint
        same(off.get(), np.arange(POOL_N + 1, dtype=np.uint64) * np.uint64(F), "frame_off", hint)
        same(csum.get(), np.tile(cs, POOL_N // 6), "csum", hint)
        compare_periodic(frames, dev(cuda, rows.reshape(-1)), POOL_N // 6, what=f"frames (hint {hint})")
    del frames


# ------------------------------------------------ 3. dense periodic batches
def tile(cuda, block, R):
    """`block` (numpy, 1-D) repeated R times on the device."""
    import torch
    b = lo._signed(dev(cuda, block))
    t = torch.empty(R * b.numel(), dtype=b.dtype, device=cuda)
    t.view(R, b.numel()).copy_(b[None, :].expand(R, -1))
    return t


def sentinel(cuda, count, dtype):
    """`count` elements of numpy `dtype` as a u8 tensor filled with the sentinel byte."""
    import torch
    return torch.full((count * np.dtype(dtype).itemsize,), SENT, dtype=torch.uint8, device=cuda)


def typed(t, dtype):
    """A u8 tensor seen as elements of numpy `dtype` (signed of that width)."""
    import torch
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[np.dtype(dtype).itemsize])


def fixed_block(rng, m, L, H):
    """m fixed-length packets: ASCII, multi-byte text and stray high bytes."""
    seq, ack, flags = random_headers(rng, m)
    pay = rng.integers(0x20, 0x7F, (m, L)).astype(np.uint8)
    for i in range(m):
        if i % 4 == 1:
            pay[i, rng.integers(0, L)] = 0xFF               # invalid UTF-8
        elif i % 4 == 2 and L >= 3:
            pay[i, :3] = np.frombuffer("€".encode(), np.uint8)
    frames, cs = codec_np.encode(seq, ack, flags, pay, H)
    return seq, ack, flags, pay, frames, cs


def decode_fixed(cuda, frames, F, n, csum_in, H, copy_payload):
    """rudp_decode_utf8 of fixed-length frames; the outputs as device tensors."""
    o = {k: sentinel(cuda, n, t) for k, t in (("seq", np.uint16), ("ack", np.uint16), ("flags", np.uint8),
                                              ("ok", np.uint8), ("csum", np.uint16), ("valid", np.uint8))}
    if copy_payload:
        o["payload"] = sentinel(cuda, n * (F - H), np.uint8)
    _native.check(_native.lib().rudp_decode_utf8(
        frames.data_ptr(), None, F, n, None if csum_in is None else csum_in.data_ptr(), o["seq"].data_ptr(),
        o["ack"].data_ptr(), o["flags"].data_ptr(), o["ok"].data_ptr(), o["csum"].data_ptr(),
        o["payload"].data_ptr() if copy_payload else None, o["valid"].data_ptr(), H, 0, None))
    return o


def check_decode_fixed(cuda, o, blk, F, R, H, with_csum, tag):
    seq, ack, flags, pay, frames, cs = blk
    m = len(seq)
    off = np.arange(m + 1, dtype=np.int64) * F
    s, a, f, ok, c, _ = codec_np.decode(frames, H, cs if with_csum else None)
    valid = codec_np.utf8_valid(frames.reshape(-1), off, H)
    assert 0 < valid.sum() < m
    for k, want in (("seq", s), ("ack", a), ("flags", f), ("ok", ok), ("csum", c), ("valid", valid)):
        compare_periodic(typed(o[k], want.dtype), dev(cuda, want), R, what=f"decode {k} {tag}", byte_scale=F)
    if "payload" in o:
        compare_periodic(o["payload"], dev(cuda, frames[:, H:].reshape(-1)), R, what=f"decode payload {tag}")


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_fixed_decode_1472(cuda, H):
    """Fixed-length decode of 1472 B payloads with the payload copy-out and
    d_valid: frames in and payloads out both pass 2^32.  Two frames of the
    block are damaged after framing (a payload byte, a header byte)."""
    L, m = 1472, 33
    F = L + H
    blk = fixed_block(np.random.default_rng(0xF1D0 + H), m, L, H)
    blk[4][7, -1] ^= 0x10
    blk[4][20, 1] ^= 0x01
    assert 0 in codec_np.decode(blk[4], H, blk[5] if H == 5 else None)[3]
    R = -(-(LINE32 + 2 * m * F) // (m * L))          # the payloads out cross too
    assert (m * F) % 16 and R * m * L > LINE32
    lo.assert_lines_mid_frame(np.arange(m + 1, dtype=np.int64) * F, H, R)
    frames = tile(cuda, blk[4].reshape(-1), R)
    csum = tile(cuda, blk[5], R) if H == 5 else None
    o = decode_fixed(cuda, frames, F, R * m, csum, H, True)
    check_decode_fixed(cuda, o, blk, F, R, H, H == 5, (L, H))
    del o, frames, csum


@pytest.mark.parametrize("L,H", [(1, 5), (3, 7), (1471, 5), (1471, 7)])
def test_periodic_implicit_offsets_fixed(cuda, L, H):
    """The implicit-offset ("stride") forms: fixed-length encode, then decode of
    its frames, of shapes the fixed tile does not take.  About 7 * 10^8 packets
    of 1 B (4 * 10^8 of 3 B) run the small-frame tiles, their frames crossing
    2^32; at 1471 B the payloads in, the frames and the payloads out all do."""
    import torch
    m, F = 1001 if L < 16 else 33, L + H
    blk = fixed_block(np.random.default_rng(0x5A11 + L), m, L, H)
    seq, ack, flags, pay, want, cs = blk
    R = lo.periodic_rows(m * F)
    if L >= 16:
        R = max(R, -(-(LINE32 + 2 * m * F) // (m * L)))
        assert R * m * L > LINE32
    n = R * m
    assert (m * F) % 16 and n < LINE32
    lo.assert_lines_mid_frame(np.arange(m + 1, dtype=np.int64) * F, H, R)
    tabs = [tile(cuda, a, R) for a in (seq, ack, flags)]
    d_pay = tile(cuda, pay.reshape(-1), R)
    frames = torch.empty(n * F, dtype=torch.uint8, device=cuda)
    csum = sentinel(cuda, n, np.uint16)
    batch = _native.RudpBatch(n=n, payload_len=L, reserved=0, seq=tabs[0].data_ptr(), ack=tabs[1].data_ptr(),
                              flags=tabs[2].data_ptr(), payload=d_pay.data_ptr(), len=None, payload_off=None)
    # the library as it is; then, at 1471 B, the diagnostics build without the LDS tiles (vector kernels)
    # and without those too (byte kernels), which find each packet's payload on their own
    for form in (None,) + (((16, 0), (14, 0)) if L >= 16 else ()):
        frames.fill_(SENT)
        old = _native.tools_lib(activate=True).rudpx_tune(*form) if form else None
        try:
            _native.check(_native.lib().rudp_encode(ctypes.byref(batch), frames.data_ptr(), csum.data_ptr(), H, 0,
                                                    None))
            torch.cuda.synchronize()
        finally:
            if form:
                _native.tools_lib().rudpx_tune(form[0], old)
                _native.use_product()
        compare_periodic(frames, dev(cuda, want.reshape(-1)), R, what=f"encode frames {(L, H, form)}")
        compare_periodic(typed(csum, np.uint16), dev(cuda, cs), R, what=f"encode csum {(L, H, form)}", byte_scale=F)
    del tabs, d_pay, batch
    torch.cuda.empty_cache()
    o = decode_fixed(cuda, frames, F, n, typed(csum, np.uint16) if H == 5 else None, H, True)
    check_decode_fixed(cuda, o, blk, F, R, H, H == 5, (L, H))
    del o, frames, csum


def varlen_block(rng, lens, H):
    m = len(lens)
    seq, ack, flags = random_headers(rng, m)
    pays = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in lens]
    frames, off, cs = codec_np.encode_varlen(seq, ack, flags, pays, H)
    return seq, ack, flags, np.frombuffer(b"".join(pays), np.uint8), frames, off, cs


def run_periodic_varlen_encode(cuda, lens, H, hints, payload_crosses, forms=(None,)):
    """`forms`: None for the library as it is, else (rudpx_tune key, value)
    pairs of the diagnostics build, set one at a time around each call."""
    import torch
    lens = np.asarray(lens, np.int32)
    if (int(lens.sum()) + len(lens) * H) % 16 == 0:
        lens[0] += 1
    seq, ack, flags, pay, want, off, cs = varlen_block(np.random.default_rng(0x7A71 + H), lens, H)
    m, Bp, B = len(lens), len(pay), len(want)
    R = -(-(LINE32 + 2 * B) // Bp) if payload_crosses else lo.periodic_rows(B)
    n = R * m
    assert B % 16 and (R * Bp > LINE32 or not payload_crosses) and n < LINE32
    lo.assert_lines_mid_frame(off, H, R)
    tabs = [tile(cuda, a, R) for a in (seq, ack, flags)]
    d_pay, d_len = tile(cuda, pay, R), tile(cuda, lens, R)
    frames = torch.empty(R * B, dtype=torch.uint8, device=cuda)
    block_frames, block_cs, block_off = dev(cuda, want), dev(cuda, cs), dev(cuda, off[:-1].copy())
    for form, hint in ((f, h) for f in forms for h in hints):
        d_off, csum, st = sentinel(cuda, n + 1, np.uint64), sentinel(cuda, n, np.uint16), sentinel(cuda, 1, np.uint32)
        frames.fill_(SENT)
        batch = _native.RudpBatch(n=n, payload_len=hint, reserved=0, seq=tabs[0].data_ptr(), ack=tabs[1].data_ptr(),
                                  flags=tabs[2].data_ptr(), payload=d_pay.data_ptr(), len=d_len.data_ptr(),
                                  payload_off=None)
        old = _native.tools_lib(activate=True).rudpx_tune(*form) if form else None
        try:
            _native.check(_native.lib().rudp_encode_varlen_checked(
                ctypes.byref(batch), R * Bp, frames.data_ptr(), R * B, d_off.data_ptr(), csum.data_ptr(), st.data_ptr(),
                H, 0, None))
            torch.cuda.synchronize()
        finally:
            if form:
                _native.tools_lib().rudpx_tune(form[0], old)
        tag = (m, H, hint, form)
        assert int(typed(st, np.uint32).item()) == 0, tag
        offs = typed(d_off, np.uint64)
        assert int(offs[-1]) == R * B, tag
        compare_periodic(offs[:-1], block_off, R, what=f"frame_off {tag}", advance=B)
        del offs, d_off
        compare_periodic(typed(csum, np.uint16), block_cs, R, what=f"csum {tag}")
        compare_periodic(frames, block_frames, R, what=f"frames {tag}")
        del csum
        torch.cuda.empty_cache()
    del tabs, d_pay, d_len, frames


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_packed_encode_ragged(cuda, H):
    """Packed rudp_encode_varlen_checked with block (b)'s lengths: the payload,
    the frames and the scanned frame_off all cross 2^32."""
    lens = np.random.default_rng(0xBB + H).integers(0, 2945, 37)
    lens[5], lens[6] = 0, 2944
    run_periodic_varlen_encode(cuda, lens, H, (int(lens.mean()), 0), True)


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_packed_encode_small_frames(cuda, H):
    """Packed rudp_encode_varlen_checked with block (a)'s lengths, about 6 * 10^8
    packets of 0-4 B (some 19 GB of tables): the small-frame kernel with its
    length codes; the frames and the scanned frame_off cross 2^32."""
    lens = np.random.default_rng(0xAA).integers(1, 5, 1001)
    lens[::97] = 0
    run_periodic_varlen_encode(cuda, lens, H, (int(lens.mean()), 0), False)


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_packed_encode_small_frames_payload_crosses(cuda, H):
    """The same kernel at the longest payloads it is picked for (10-15 B, a hint
    below 16): about 3.5 * 10^8 packets, whose packed payload crosses 2^32 too
    (1-4 B payloads would need more than 2^32 / 4 packets for that)."""
    lens = np.random.default_rng(0xAB).integers(10, 16, 1001)
    lens[::97] = 0
    run_periodic_varlen_encode(cuda, lens, H, (int(lens.mean()), 0), True)


# the diagnostics build's other forms of the packed encode: (rudpx_tune key, value), one at a time
ENCODE_FORMS = ((16, 0), (14, 0), (51, 2), (51, 0), (52, 0), (24, 0), (43, 0), (36, 0), (67, 0))
SMALL_ENCODE_FORMS = ((46, 0), (50, 0), (74, 0), (47, 1), (47, 8), (24, 0))


def test_periodic_packed_encode_alternative_forms(cuda):
    """The packed encode's kernels the product does not pick (vector and byte
    kernels, byte tiles always and never, the library scan, the small-frame
    kernel off, its other packets per thread and base search), at the block's
    mean hint, across 2^32."""
    lens = np.random.default_rng(0xBB + 7).integers(0, 2945, 37)
    lens[5], lens[6] = 0, 2944
    run_periodic_varlen_encode(cuda, lens, 7, (int(lens.mean()),), True, ENCODE_FORMS)
    lens = np.random.default_rng(0xAA).integers(1, 5, 1001)
    lens[::97] = 0
    run_periodic_varlen_encode(cuda, lens, 5, (int(lens.mean()),), False, SMALL_ENCODE_FORMS)


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_gather_payloads(cuda, H):
    """rudp_gather_payloads at an MTU hint with a periodic keep mask: the frames
    in and the message out both cross 2^32."""
    import torch
    rng = np.random.default_rng(0x6A70 + H)
    m = 33
    lens = rng.integers(1300, 1473, m) + H
    lens[3], lens[4], lens[9] = H, 2, 0               # header only, shorter than the header, empty
    lens[0] += int(lens.sum()) % 16 == 0
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    B = int(off[-1])
    buf = rng.integers(0, 256, B, dtype=np.uint8)
    keep = (np.arange(m) % 4 != 1).astype(np.uint8)
    pay, poff = lo.gather_expect(buf, off, H, keep)
    Kp = len(pay)
    R = -(-(LINE32 + 2 * B) // Kp)
    n = R * m
    assert B % 16 and R * Kp > LINE32
    lo.assert_lines_mid_frame(off, H, R)
    frames = tile(cuda, buf, R)
    d_keep = tile(cuda, keep, R)
    d_off = torch.cat([(torch.arange(R, dtype=torch.int64, device=cuda)[:, None] * B
                        + dev(cuda, off[:-1].copy())[None, :]).reshape(-1),
                       torch.tensor([R * B], dtype=torch.int64, device=cuda)])
    block_pay, block_poff = dev(cuda, pay), dev(cuda, poff[:-1].astype(np.int64))
    out = torch.empty(R * Kp + 64, dtype=torch.uint8, device=cuda)
    for hint in (B // m, 0):
        out.fill_(SENT)
        d_poff, st = sentinel(cuda, n + 1, np.uint64), sentinel(cuda, 1, np.uint32)
        _native.check(_native.lib().rudp_gather_payloads(
            frames.data_ptr(), R * B, d_off.data_ptr(), hint, n, d_keep.data_ptr(), out.data_ptr(), R * Kp + 64,
            d_poff.data_ptr(), st.data_ptr(), H, 0, None))
        assert int(typed(st, np.uint32).item()) == 0, hint
        offs = typed(d_poff, np.uint64)
        assert int(offs[-1]) == R * Kp, hint
        compare_periodic(offs[:-1], block_poff, R, what=f"payload_off (hint {hint})", advance=Kp)
        compare_periodic(out[:R * Kp], block_pay, R, what=f"payload (hint {hint})")
        assert bool((out[R * Kp:] == SENT).all()), hint    # nothing at or past the total
        del offs, d_poff
    del frames, d_keep, d_off, out


@pytest.mark.parametrize("chunk", [16383, 1000])
def test_periodic_segment_utf8(cuda, chunk):
    """rudp_segment_utf8 of a periodic message whose bytes and whose characters
    both exceed 2^32, against the closed form; and the size query."""
    import torch
    P = 1021
    period, starts = lo.periodic_message(P)
    R = -(-(LINE32 + (1 << 26)) // P)
    isn = 4321
    want = lo.segment_closed_form(P, starts, R, chunk, isn)
    assert R * P > LINE32 and want.characters > LINE32 and P % 16
    msg = tile(cuda, np.frombuffer(period, np.uint8), R)
    count, st = Out(cuda, 2, np.uint64), Out(cuda, 1, np.uint32)
    _native.check(_native.lib().rudp_segment_utf8(msg.data_ptr(), R * P, chunk, isn, 0, None, None, None, None, None,
                                                  count.ptr, st.ptr, 0, None))
    assert count.get().tolist() == [want.packets, want.characters]
    assert int(st.get()[0]) == _native.ST_PACKETS_CAP
    K = want.packets
    o = dict(seq=Out(cuda, K, np.uint16), ack=Out(cuda, K, np.uint16), flags=Out(cuda, K, np.uint8),
             len=Out(cuda, K, np.uint32), payload_off=Out(cuda, K + 1, np.uint64))
    count, st = Out(cuda, 2, np.uint64), Out(cuda, 1, np.uint32)
    _native.check(_native.lib().rudp_segment_utf8(msg.data_ptr(), R * P, chunk, isn, K, o["seq"].ptr, o["ack"].ptr,
                                                  o["flags"].ptr, o["len"].ptr, o["payload_off"].ptr, count.ptr, st.ptr,
                                                  0, None))
    assert int(st.get()[0]) == 0
    assert count.get().tolist() == [want.packets, want.characters]
    same(o["payload_off"].get(), want.payload_off, "payload_off", chunk)
    same(o["len"].get(), want.len, "len", chunk)
    same(o["seq"].get(), want.seq, "seq", chunk)
    same(o["flags"].get(), want.flags, "flags", chunk)
    same(o["ack"].get(), np.zeros(K, np.uint16), "ack", chunk)
    del msg


# ------------------------------- offsets that only look valid in 32 bits
@pytest.mark.parametrize("H", [5, 7])
def test_readers_reject_offsets_valid_only_in_32_bits(cuda, H):
    """In a 1 MiB buffer: the pairs (100, 2^32 + 200), (2^32 + 200, 2^32 + 300)
    and (2^32 + 300, 400), whose low halves are all in bounds, between valid
    frames.  Each reader rejects them as include/rudp.h says, and the bytes at
    the aliased low offsets change nothing."""
    rng = np.random.default_rng(0xA11A + H)
    nbytes = 1 << 20
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    seq, ack, flags = random_headers(rng, 2)
    fr, foff, _ = codec_np.encode_varlen(seq, ack, flags, [b"x" * (40 - H), "é".encode() * ((60 - H) // 2)], H)
    buf[:len(fr)] = fr
    assert foff.tolist() == [0, 40, 99]
    off = np.array([0, 40, int(foff[2]), LINE32 + 200, LINE32 + 300, 400, 400 + int(foff[2]) - 40], np.int64)
    buf[400:int(off[6])] = fr[40:]                      # frame 5 repeats frame 1
    n = 6
    good = np.array([1, 1, 0, 0, 0, 1], bool)
    w = lo.decode_expect(buf, off, H, None, lim=nbytes)
    assert (w["good"] == good).all() and (w["ok"][~good] == lo.OK_BAD_OFFSETS).all() and w["status"] == lo.ST_OFFSETS
    frames = [bytes(buf[off[i]:off[i + 1]]) if good[i] else b"" for i in range(n)]
    dup = np.array(lo.proxy_scan(frames, 4, rejected={2, 3, 4})[0], np.uint8)
    assert dup.tolist() == [0, 0, 2, 2, 2, 1]
    pay, poff = lo.gather_expect(buf, off, H, np.ones(n, np.uint8), good)
    rank = np.arange(n, dtype=np.uint32)[::-1].copy()
    ordered = lo.ordered_ref(buf, off, rank, n, H)
    assert ordered[3] == lo.ST_OFFSETS
    for poisoned in (False, True):
        if poisoned:
            buf[int(off[2]):400] ^= 0x5A                # every aliased low byte
        pl = Placed(cuda, None, buf, off, 0, True)
        for hint in (int(off[6]) // n, 0):
            tag = (H, hint, poisoned)
            for utf8 in (False, True):
                got = call_decode(pl, hint, H, utf8=utf8, sideband=False)
                for k in ("seq", "ack", "flags", "ok", "csum") + (("valid",) if utf8 else ()):
                    same(got[k], w[k], "decode", k, *tag)
                assert got["status"] == lo.ST_OFFSETS, tag
            same(call_chars(pl, hint, H), w["chars"], "payload_chars", *tag)
            g_pay, g_off, g_st = call_gather(pl, hint, H, None, len(pay) + 64)
            assert g_st == lo.ST_OFFSETS, tag
            same(g_off, poff, "gather payload_off", *tag)
            same(g_pay[:len(pay)], pay, "gather payload", *tag)
            assert untouched(g_pay[len(pay):]), tag
            check_ordered(call_ordered(pl, hint, rank, n, H, len(ordered[0]) + 64), ordered, n, "gather_ordered", *tag)
            same(call_dedup(pl, hint, 4, True), dup, "dedup_window_checked", *tag)
            assert call_off_check(pl, nbytes) == lo.ST_OFFSETS, tag


@pytest.mark.parametrize("H", [5, 7])
def test_encode_rejects_payload_off_valid_only_in_32_bits(cuda, big, H):
    """Gathered encode: payload_off[i] = 2^32 + k with payload_bytes = 4096 is
    RUDP_ST_PAYLOAD, and no frame byte is written.  (The payload pointer is the
    large buffer, so that no offset leaves memory this module owns.)"""
    rng = np.random.default_rng(0xE4C + H)
    n = 8
    tabs = [dev(cuda, a) for a in random_headers(rng, n)]
    d_len = dev(cuda, np.full(n, 10, np.int32))
    for bad in ([3], [0, 7], list(range(n))):
        poff = np.arange(n, dtype=np.int64) * 16
        poff[bad] += LINE32
        for hint in (10, 0):
            fr = Out(cuda, n * (10 + H), np.uint8)
            off, cs, st = encode_varlen(cuda, n, hint, tabs, big.t.data_ptr(), 4096, d_len, dev(cuda, poff), fr.ptr,
                                        n * (10 + H), H)
            assert int(st.get()[0]) == lo.ST_PAYLOAD, (bad, hint)
            assert int(off.get()[n]) == n * (10 + H), (bad, hint)
            assert untouched(fr.get()) and untouched(cs.get()), (bad, hint)


def test_encode_rejects_sizes_valid_only_in_32_bits(cuda):
    """The 66 000 x 65 535 B batch, whose sizes pass 2^32.  Gathered with
    frames_cap = total - 2^32: RUDP_ST_FRAMES_CAP, frame_off[n] the true total
    and no frame byte written.  Packed with payload_bytes = sum(len) - 2^32:
    RUDP_ST_PAYLOAD.  (Both buffers have the true sizes, so that nothing a
    32-bit comparison would let through leaves memory this test owns.)"""
    import torch
    H = 5
    pool, tabs, d_len, d_poff, _, _ = pool_batch(cuda, H)
    total, payload = POOL_N * (POOL_LEN + H), POOL_N * POOL_LEN
    assert 0 < total - LINE32 < LINE32 and 0 < payload - LINE32
    frames = torch.full((total,), SENT, dtype=torch.uint8, device=cuda)

    def unwritten():
        step = 1 << 30
        return all(bool((frames[a:a + step] == SENT).all()) for a in range(0, total, step))
    for hint in (POOL_LEN, 0):
        off, cs, st = encode_varlen(cuda, POOL_N, hint, tabs, pool.data_ptr(), 65536, d_len, d_poff, frames.data_ptr(),
                                    total - LINE32, H)
        assert int(st.get()[0]) == lo.ST_FRAMES_CAP, hint
        assert int(off.get()[POOL_N]) == total, hint
        assert unwritten() and untouched(cs.get()), hint
    del pool
    packed = torch.empty(payload, dtype=torch.uint8, device=cuda)
    for hint in (POOL_LEN, 0):
        off, cs, st = encode_varlen(cuda, POOL_N, hint, tabs, packed.data_ptr(), payload - LINE32, d_len, None,
                                    frames.data_ptr(), total, H)
        assert int(st.get()[0]) == lo.ST_PAYLOAD, hint
        assert int(off.get()[POOL_N]) == total, hint
        assert unwritten() and untouched(cs.get()), hint
    del frames, packed
