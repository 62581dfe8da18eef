"""Packed payload copy-out of packed frames on the GPU (gather_payloads,
rudp_gather_payloads): the reference receiver's ``buffer + payload`` for every
accepted datagram (utils/reliableUDP.py:121, :135-136), byte for byte against
a numpy restatement (the concatenation of the kept frames' payload slices).
"""
import numpy as np
import pytest

from conftest import split_by_lengths
from oracle import synth
from rudp import _native, batch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(cuda)


def host(t):
    return t.cpu().numpy()


def ref_gather(frames, off, H, keep=None):
    """(payload bytes, payload_off, status): the kept slices frames[off[i] + H : off[i + 1]]."""
    n = len(off) - 1
    parts, lens, status = [], np.zeros(n, np.int64), 0
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if a > b or b > len(frames):
            status = _native.ST_OFFSETS
            continue
        if keep is not None and not keep[i]:
            continue
        if b - a > H:
            parts.append(frames[a + H:b])
            lens[i] = b - a - H
    pay = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return pay, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), status


def packed(rng, frame_lens):
    """Random full-range bytes cut into frames of the given lengths."""
    off = np.concatenate([[0], np.cumsum(frame_lens)]).astype(np.int64)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


def check_gather(cuda, frames, off, H, keep=None):
    """Gather into a sentinel-filled buffer of frames.size bytes with 64 guard
    bytes each side; everything outside [0, total) must stay sentinel."""
    import torch
    want, want_off, want_st = ref_gather(frames, off, H, keep)
    cap = len(frames)
    store = torch.full((cap + 128,), SENTINEL, dtype=torch.uint8, device=cuda)
    out = store[64:64 + cap]
    res = batch.gather_payloads(dev(frames, cuda), dev(off, cuda), H,
                                keep=None if keep is None else dev(keep, cuda), out=out, check=False)
    got_off = host(res.payload_off)
    assert int(host(res.status)[0]) == want_st
    assert np.array_equal(got_off, want_off)
    total = int(want_off[-1])
    s = host(store)
    assert np.array_equal(s[64:64 + total], want)
    assert (s[:64] == SENTINEL).all() and (s[64 + total:] == SENTINEL).all()
    assert np.array_equal(host(res.lengths), np.diff(want_off).astype(np.int32))
    assert res.lengths.dtype == torch.int32 and res.payload_off.dtype == torch.int64
    assert np.array_equal(host(res.payload), want)
    return res


# ---- 1. reference fixtures
@pytest.mark.parametrize("layout", [5, 7])
def test_fixture_frames_give_payload_and_lengths(cuda, golden_varlen, layout):
    g = golden_varlen
    fr = g[f"frames{layout}"]
    off = np.concatenate([[0], np.cumsum(g["lengths"] + layout)]).astype(np.int64)
    res = batch.gather_payloads(dev(fr, cuda), dev(off, cuda), layout)
    assert np.array_equal(host(res.payload), g["payload"])
    assert np.array_equal(host(res.lengths), g["lengths"])
    assert res.buffer.numel() == fr.size and int(host(res.status)[0]) == 0


def test_wire_trace_gives_the_message(cuda, wire_trace):
    datagrams = [bytes.fromhex(h) for h in wire_trace["client_to_server"]]
    off = np.concatenate([[0], np.cumsum([len(d) for d in datagrams])]).astype(np.int64)
    flat = np.frombuffer(b"".join(datagrams), np.uint8)
    res = batch.gather_payloads(dev(flat, cuda), dev(off, cuda), "rudp5")
    assert bytes(host(res.payload)) == wire_trace["message"].encode()


def test_dedup_fixture_drops_retransmissions(cuda, golden_dedup):
    g = golden_dedup
    frames, off = g["frames"], np.concatenate([[0], np.cumsum(g["lengths"])]).astype(np.int64)
    keep = (g["dup"] == 0).astype(np.uint8)
    assert 0 < keep.sum() < len(keep)
    datagrams, _ = split_by_lengths(frames, g["lengths"])
    want = b"".join(d[5:] for d, k in zip(datagrams, keep) if k)
    res = batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 5, keep=dev(keep, cuda))
    assert bytes(host(res.payload)) == want
    check_gather(cuda, frames, off, 5, keep)


# ---- 2. boundaries
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1025, 2047, 2048, 2049, 4097])
def test_frame_counts_at_tile_and_scan_block_edges(cuda, n):
    rng = np.random.default_rng(n)
    for H in (5, 7):
        frames, off = packed(rng, H + rng.integers(0, 5, n))
        check_gather(cuda, frames, off, H)
        check_gather(cuda, frames, off, H, rng.integers(0, 2, n).astype(np.uint8))


@pytest.mark.parametrize("layout", [5, 7])
def test_every_short_frame_length(cuda, layout):
    rng = np.random.default_rng(layout)
    lens = np.repeat(np.arange(0, layout + 18), 9)
    rng.shuffle(lens)
    check_gather(cuda, *packed(rng, lens), layout)
    check_gather(cuda, *packed(rng, np.sort(lens)), layout)


@pytest.mark.parametrize("layout", [5, 7])
def test_mtu_and_ragged_lengths(cuda, layout):
    rng = np.random.default_rng(40 + layout)
    check_gather(cuda, *packed(rng, np.full(300, 1472 + layout)), layout)
    check_gather(cuda, *packed(rng, rng.integers(0, 2945, 1000)), layout)


def test_long_frames_take_the_per_frame_path(cuda):
    rng = np.random.default_rng(77)
    # one 200 000-B frame between small ones (a small-frame tile that cannot stage it)
    lens = np.concatenate([7 + rng.integers(0, 5, 700), [200000], 7 + rng.integers(0, 5, 900)])
    frames, off = packed(rng, lens)
    check_gather(cuda, frames, off, 7)
    check_gather(cuda, frames, off, 5, rng.integers(0, 2, len(lens)).astype(np.uint8))
    # a run of 2944-B frames inside a batch whose mean is small: their tile overflows its LDS budget
    lens = np.concatenate([5 + rng.integers(0, 40, 2000), np.full(40, 2944), 5 + rng.integers(0, 40, 2000)])
    frames, off = packed(rng, lens)
    check_gather(cuda, frames, off, 5)
    # and single frames larger than any tile budget with an MTU-scale hint
    check_gather(cuda, *packed(rng, np.array([1400, 70000, 3, 0, 45000, 1500, 41000])), 7)


@pytest.mark.parametrize("hint", [0, 8, 64, 1479, 100000])
def test_len_hint_picks_geometry_never_the_result(cuda, hint):
    """The C call with every kind of hint on one mixed batch: tiny frames, a
    200 000-B frame and a run of 2944-B frames (small-frame tiles, MTU tiles
    and one-frame tiles each meet runs over and under their LDS budget)."""
    import torch
    rng = np.random.default_rng(123)
    lens = np.concatenate([rng.integers(0, 12, 1500), [200000], rng.integers(0, 12, 700), np.full(30, 2944),
                           rng.integers(0, 12, 1100)])
    frames, off = packed(rng, lens)
    n = len(lens)
    for H, keep in ((5, None), (7, rng.integers(0, 2, n).astype(np.uint8))):
        want, want_off, _ = ref_gather(frames, off, H, keep)
        d_frames, d_off = dev(frames, cuda), dev(off, cuda)
        d_keep = None if keep is None else dev(keep, cuda)
        store = torch.full((len(frames) + 128,), SENTINEL, dtype=torch.uint8, device=cuda)
        poff = torch.full((n + 1,), -1, dtype=torch.int64, device=cuda)
        status = torch.full((1,), -1, dtype=torch.int32, device=cuda)
        _native.check(_native.lib().rudp_gather_payloads(
            d_frames.data_ptr(), len(frames), d_off.data_ptr(), hint, n,
            d_keep.data_ptr() if d_keep is not None else None, store.data_ptr() + 64, len(frames),
            poff.data_ptr(), status.data_ptr(), H, 0, torch.cuda.current_stream(cuda).cuda_stream))
        torch.cuda.synchronize()
        s = host(store)
        assert int(host(status)[0]) == 0
        assert np.array_equal(host(poff), want_off)
        assert np.array_equal(s[64:64 + len(want)], want)
        assert (s[:64] == SENTINEL).all() and (s[64 + len(want):] == SENTINEL).all()


# ---- 3. keep masks
@pytest.mark.parametrize("shape", ["small", "mtu"])
def test_keep_masks(cuda, shape):
    import torch
    rng = np.random.default_rng(5)
    n = 3000 if shape == "small" else 150
    lens = 7 + (rng.integers(0, 5, n) if shape == "small" else rng.integers(0, 2945, n))
    frames, off = packed(rng, lens)
    check_gather(cuda, frames, off, 7, None)
    check_gather(cuda, frames, off, 7, np.ones(n, np.uint8))
    res = check_gather(cuda, frames, off, 7, np.zeros(n, np.uint8))  # total 0: output untouched
    assert res.payload.numel() == 0 and int(host(res.payload_off)[-1]) == 0
    check_gather(cuda, frames, off, 7, (np.arange(n) & 1).astype(np.uint8))
    check_gather(cuda, frames, off, 7, rng.integers(0, 2, n).astype(np.uint8))
    check_gather(cuda, frames, off, 7, rng.integers(0, 256, n).astype(np.uint8))  # any non-zero byte keeps
    # a kept frame directly after a long dropped run (and before one)
    keep = np.zeros(n, np.uint8)
    keep[[0, n // 2, n - 1]] = 1
    check_gather(cuda, frames, off, 7, keep)
    # a bool mask is taken as it is
    kb = rng.integers(0, 2, n).astype(bool)
    want, want_off, _ = ref_gather(frames, off, 7, kb)
    got = batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 7, keep=torch.from_numpy(kb).to(cuda))
    assert np.array_equal(host(got.payload), want) and np.array_equal(host(got.payload_off), want_off)


def test_keep_validation(cuda):
    import torch
    frames, off = packed(np.random.default_rng(1), np.full(4, 9))
    f, o = dev(frames, cuda), dev(off, cuda)
    with pytest.raises(ValueError, match="entries"):
        batch.gather_payloads(f, o, 7, keep=torch.ones(3, dtype=torch.uint8, device=cuda))
    with pytest.raises(TypeError, match="keep"):
        batch.gather_payloads(f, o, 7, keep=torch.ones(4, dtype=torch.int32, device=cuda))
    with pytest.raises(TypeError, match="keep"):
        batch.gather_payloads(f, o, 7, keep=np.ones(4, np.uint8))


# ---- 4. alignment and guards
@pytest.mark.parametrize("shape", ["small", "mtu"])
def test_unaligned_views_and_sentinels(cuda, shape):
    import torch
    rng = np.random.default_rng(9)
    n = 1500 if shape == "small" else 90
    lens = 5 + (rng.integers(0, 5, n) if shape == "small" else rng.integers(0, 2945, n))
    frames, off = packed(rng, lens)
    keep = (rng.integers(0, 4, n) > 0).astype(np.uint8)
    want, want_off, _ = ref_gather(frames, off, 5, keep)
    total, cap = len(want), len(want) + 40
    d_off, d_keep = dev(off, cuda), dev(keep, cuda)
    for k in range(1, 16):
        fstore = torch.full((len(frames) + 32,), SENTINEL, dtype=torch.uint8, device=cuda)
        fstore[k:k + len(frames)] = dev(frames, cuda)
        ko = (5 * k) % 16  # 1..15, each once
        store = torch.full((ko + 64 + cap + 64,), SENTINEL, dtype=torch.uint8, device=cuda)
        out = store[ko + 64:ko + 64 + cap]
        res = batch.gather_payloads(fstore[k:k + len(frames)], d_off, 5, keep=d_keep, out=out)
        s = host(store)
        assert np.array_equal(s[ko + 64:ko + 64 + total], want), k
        assert (s[:ko + 64] == SENTINEL).all() and (s[ko + 64 + total:] == SENTINEL).all(), k
        assert np.array_equal(host(res.payload_off), want_off), k


# ---- 5. rejection
def test_bad_offsets_are_rejected_frame_by_frame(cuda):
    rng = np.random.default_rng(21)
    n = 600
    frames, off = packed(rng, np.full(n, 20))
    off[100] = off[99] - 7                 # frame 99 decreasing; frame 100 = [off[99] - 7, off[101])
    off[400] = len(frames) + 1000          # frame 399 ends past the buffer; frame 400 decreasing
    want, want_off, st = ref_gather(frames, off, 7)
    assert st == _native.ST_OFFSETS
    lens = np.diff(want_off)
    assert lens[99] == 0 and lens[399] == 0 and lens[400] == 0 and lens[100] == 47 - 7
    res = check_gather(cuda, frames, off, 7)
    assert int(host(res.status)[0]) == _native.ST_OFFSETS
    with pytest.raises(ValueError, match="frame_off"):
        res.check()
    with pytest.raises(ValueError, match="frame_off"):
        batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 7)
    # judged whether or not the frame is kept
    keep = np.ones(n, np.uint8)
    keep[[99, 399, 400]] = 0
    res = check_gather(cuda, frames, off, 7, keep)
    assert int(host(res.status)[0]) == _native.ST_OFFSETS


@pytest.mark.parametrize("shape", ["small", "mtu"])
def test_out_one_byte_too_small(cuda, shape):
    import torch
    rng = np.random.default_rng(31)
    n = 2500 if shape == "small" else 120
    lens = 7 + (rng.integers(0, 5, n) if shape == "small" else rng.integers(0, 2945, n))
    frames, off = packed(rng, lens)
    want, want_off, _ = ref_gather(frames, off, 7)
    total = len(want)
    out = torch.full((total - 1,), SENTINEL, dtype=torch.uint8, device=cuda)
    res = batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 7, out=out, check=False)
    assert int(host(res.status)[0]) == _native.ST_PAYLOAD_CAP
    assert int(host(res.payload_off)[-1]) == total
    assert np.array_equal(host(res.payload_off), want_off)
    assert (host(out) == SENTINEL).all()
    with pytest.raises(ValueError, match=f"{total} bytes are needed"):
        res.check()
    with pytest.raises(ValueError, match="too small"):
        batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 7, out=out)
    # exactly enough is enough
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=cuda)
    res = batch.gather_payloads(dev(frames, cuda), dev(off, cuda), 7, out=out)
    assert np.array_equal(host(out), want)


# ---- 6. round trip
@pytest.mark.parametrize("layout", [5, 7])
def test_pack_gather_pack_round_trip(cuda, layout):
    rng = np.random.default_rng(layout)
    n = 3000
    lens = rng.integers(0, 60, n).astype(np.int32)
    pay = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    seq, ack, flags, _ = synth.synth(17, 0, n, 0)
    tab = (dev(seq, cuda), dev(ack, cuda), dev(flags, cuda))
    res = batch.pack_batch_varlen(tab, dev(pay, cuda), dev(lens, cuda), layout, want_csum=True)
    g = batch.gather_payloads(res.frames, res.frame_off, layout)
    assert np.array_equal(host(g.payload), pay) and np.array_equal(host(g.lengths), lens)
    # the relay's drop-and-reframe: the gather's buffer and lengths are the encode's packed payload
    again = batch.pack_batch_varlen(tab, g.payload, g.lengths, layout, want_csum=True)
    assert np.array_equal(host(again.frames), host(res.frames))
    assert np.array_equal(host(again.frame_off), host(res.frame_off))


def test_keep_mask_from_decode_keeps_only_clean_frames(cuda):
    rng = np.random.default_rng(3)
    n = 2000
    lens = rng.integers(1, 9, n).astype(np.int32)
    pay = rng.integers(0x20, 0x7F, int(lens.sum()), dtype=np.uint8)  # ASCII bodies
    poff = np.concatenate([[0], np.cumsum(lens)])
    bad_utf8 = rng.choice(n, 25, replace=False)
    pay[poff[bad_utf8]] = 0xFF  # never valid in UTF-8
    seq, ack, flags, _ = synth.synth(23, 0, n, 0)
    res = batch.pack_batch_varlen((dev(seq, cuda), dev(ack, cuda), dev(flags, cuda)), dev(pay, cuda),
                                  dev(lens, cuda), 7)
    frames = host(res.frames).copy()
    off = host(res.frame_off)
    bad_csum = np.setdiff1d(rng.choice(n, 40, replace=False), bad_utf8)
    frames[off[bad_csum] + 5] ^= 0x5A  # the in-band checksum's high byte
    d_frames = dev(frames, cuda)
    dec = batch.unpack_batch_varlen(d_frames, res.frame_off, 7, utf8=True)
    keep = batch.keep_mask(dec)
    clean = np.ones(n, np.uint8)
    clean[bad_utf8] = 0
    clean[bad_csum] = 0
    assert np.array_equal(host(keep), clean)
    g = batch.gather_payloads(d_frames, res.frame_off, 7, keep=keep)
    want, want_off, _ = ref_gather(frames, off, 7, clean)
    assert np.array_equal(host(g.payload), want) and np.array_equal(host(g.payload_off), want_off)
    # with retransmission flags: a frame flagged dup is dropped as well
    dup = np.zeros(n, np.uint8)
    dup[::7] = 1
    keep2 = batch.keep_mask(dec, dup=dev(dup, cuda))
    assert np.array_equal(host(keep2), clean & (dup == 0))


# ---- 7. side stream
def test_side_stream_after_an_encode_on_it(cuda):
    import torch
    rng = np.random.default_rng(8)
    n = 5000
    lens = rng.integers(0, 30, n).astype(np.int32)
    pay = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    seq, ack, flags, _ = synth.synth(29, 0, n, 0)
    tab = (dev(seq, cuda), dev(ack, cuda), dev(flags, cuda))
    d_pay, d_lens = dev(pay, cuda), dev(lens, cuda)
    keep = rng.integers(0, 2, n).astype(np.uint8)
    d_keep = dev(keep, cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        res = batch.pack_batch_varlen(tab, d_pay, d_lens, 5, stream=side, check=False)
        g = batch.gather_payloads(res.frames, res.frame_off, 5, keep=d_keep, stream=side, check=False)
    side.synchronize()
    poff = np.concatenate([[0], np.cumsum(lens)])
    want = np.concatenate([pay[poff[i]:poff[i + 1]] for i in range(n) if keep[i]] or [np.zeros(0, np.uint8)])
    assert int(host(g.status)[0]) == 0
    assert np.array_equal(host(g.payload), want)
    assert np.array_equal(host(g.lengths), lens * keep)
