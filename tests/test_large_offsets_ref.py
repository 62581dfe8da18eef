"""The CPU side of tests/test_gpu_large_offsets.py (tests/large_offsets.py),
checked before an MI355X sees it: the periodic expectations at R = 3 against
the oracle applied to the fully materialised batch (encode, decode, gather,
segment), the base translation, and the "line inside a payload" assertions on
blocks built to violate them."""
import numpy as np
import pytest
import torch

import large_offsets as lo
from oracle import codec_np
from segment_ref import segment_ref

R3 = 3


def _headers(rng, n):
    return (rng.integers(0, 65536, n).astype(np.uint16), rng.integers(0, 65536, n).astype(np.uint16),
            rng.integers(0, 256, n).astype(np.uint8))


def _t(a):
    return torch.from_numpy(np.array(a))


# ------------------------------------------------------------ periodic batches
@pytest.mark.parametrize("H", [5, 7])
def test_periodic_encode_is_the_oracle_on_the_tiled_batch(H):
    rng = np.random.default_rng(31 + H)
    lens = rng.integers(0, 300, 37)
    seq, ack, flags = _headers(rng, 37)
    pays = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in lens]
    frames, off, cs = codec_np.encode_varlen(seq, ack, flags, pays, H)
    full, full_off, full_cs = codec_np.encode_varlen(np.tile(seq, R3), np.tile(ack, R3), np.tile(flags, R3), pays * R3, H)
    B = len(frames)
    assert np.array_equal(lo.tile_offsets(off, R3), full_off)
    lo.compare_periodic(_t(full), _t(frames), R3, what="frames")
    lo.compare_periodic(_t(full_cs), _t(cs), R3, what="csum")
    lo.compare_periodic(_t(full_off[:-1]), _t(off[:-1]), R3, what="frame_off", advance=B)
    lo.compare_periodic(_t(full_off[:-1]), _t(off[:-1]), R3, what="frame_off", advance=B, chunk_bytes=64)  # row by row
    # a wrong byte, a wrong checksum and an offset that lost a carry are each named
    bad = full.copy()
    bad[B + 17] ^= 1
    with pytest.raises(AssertionError, match=f"element {B + 17} .*byte offset {B + 17}, below 2\\^31"):
        lo.compare_periodic(_t(bad), _t(frames), R3, what="frames", chunk_bytes=128)
    bad_off = full_off.copy()
    bad_off[2 * 37 + 5] -= B
    with pytest.raises(AssertionError, match=f"element {2 * 37 + 5} "):
        lo.compare_periodic(_t(bad_off[:-1]), _t(off[:-1]), R3, what="frame_off", advance=B)
    with pytest.raises(AssertionError):
        lo.compare_periodic(_t(full_cs[:-1]), _t(cs), R3, what="csum")


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_decode_is_the_oracle_on_the_tiled_batch(H):
    rng = np.random.default_rng(41 + H)
    m, L = 33, 48
    seq, ack, flags = _headers(rng, m)
    pay = rng.integers(0x20, 0x7F, (m, L)).astype(np.uint8)
    pay[1::4, 7] = 0xFF
    frames, cs = codec_np.encode(seq, ack, flags, pay, H)
    frames[5, -1] ^= 0x10                                  # one frame damaged in flight
    F = L + H
    off = np.arange(m + 1, dtype=np.int64) * F
    sideband = cs if H == 5 else None
    want = codec_np.decode(frames, H, sideband)[:5] + (codec_np.utf8_valid(frames.reshape(-1), off, H),)
    tiled = np.tile(frames, (R3, 1))
    full = codec_np.decode(tiled, H, None if sideband is None else np.tile(cs, R3))
    full_valid = codec_np.utf8_valid(tiled.reshape(-1), lo.tile_offsets(off, R3), H)
    for got, w in zip(full[:5] + (full_valid,), want):
        lo.compare_periodic(_t(got), _t(w), R3, what="decode")
    lo.compare_periodic(_t(full[5].reshape(-1)), _t(frames[:, H:].reshape(-1)), R3, what="payload")
    assert 0 in want[3] and 0 < want[5].sum() < m


@pytest.mark.parametrize("H", [5, 7])
def test_periodic_gather_is_the_restatement_on_the_tiled_batch(H):
    rng = np.random.default_rng(51 + H)
    m = 33
    lens = rng.integers(40, 90, m) + H
    lens[3], lens[4], lens[9] = H, 2, 0
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    keep = (np.arange(m) % 4 != 1).astype(np.uint8)
    pay, poff = lo.gather_expect(buf, off, H, keep)
    full_pay, full_poff = lo.gather_expect(np.tile(buf, R3), lo.tile_offsets(off, R3), H, np.tile(keep, R3))
    assert int(full_poff[-1]) == R3 * len(pay)
    lo.compare_periodic(_t(full_pay), _t(pay), R3, what="payload")
    lo.compare_periodic(_t(full_poff[:-1].astype(np.int64)), _t(poff[:-1].astype(np.int64)), R3, what="payload_off",
                        advance=len(pay))
    # the restatement is the gather's definition: kept frames' payloads back to back
    want = b"".join(bytes(buf[off[i] + H:off[i + 1]]) for i in range(m) if keep[i] and lens[i] > H)
    assert pay.tobytes() == want


@pytest.mark.parametrize("chunk", [1, 7, 1000, 1015, 16383])
def test_segment_closed_form_is_segment_ref_on_the_tiled_message(chunk):
    P = 1021
    period, starts = lo.periodic_message(P)
    assert len(period) == P and period.decode() and {1, 2, 3, 4} <= set(np.diff(np.append(starts, P)).tolist())
    for R in (1, R3, 17):
        got = lo.segment_closed_form(P, starts, R, chunk, 65000)
        ref = segment_ref(period * R, chunk, 65000)
        assert (got.packets, got.characters) == (ref.packets, ref.characters)
        assert np.array_equal(got.seq, ref.seq) and np.array_equal(got.flags, ref.flags)
        assert np.array_equal(got.len, ref.len) and np.array_equal(got.payload_off.astype(np.int64), ref.payload_off)
        assert ref.status == 0


# ---------------------------------------------------------------- placement
@pytest.mark.parametrize("H", [5, 7])
@pytest.mark.parametrize("kind", ["chars", "ragged", "long"])
def test_blocks_straddle_both_lines_and_translate(kind, H):
    b = lo.make_block(kind, H)
    assert b.n >= 600 and b.mean == len(b.buf) // b.n
    assert any(len(f) < H for f in b.frames) and any(len(f) == H for f in b.frames)
    places = lo.placements(b.off, H, need_margin=kind != "chars", anchor=b.anchor)
    assert [p[0] for p in places] == ["control", "2^31", "2^32"] and places[0][1] == 0
    assert any(base % 16 for _, base in places[1:])
    for (name, base), line in zip(places[1:], lo.LINES):
        i = lo.assert_line_inside(b.off, H, base, line, need_margin=kind != "chars")
        a, e = int(b.off[i]) + base, int(b.off[i + 1]) + base
        assert a + H <= line < e and (kind == "chars" or (a + 16 <= line <= e - 16))
        assert b.anchor in (None, i)
        assert base + len(b.buf) <= lo.BIG_BYTES
        t = lo.translate(b.off, base)
        assert t.dtype == np.int64 and np.array_equal(t - base, b.off) and t[0] == base
    if kind == "long":
        assert len(b.frames[b.anchor]) == 200_000 + H


def test_translated_block_has_the_controls_answers():
    """The expectation is a function of the frames, not of where they lie: the
    restatements applied to a block copied to a base of a larger buffer give
    the control's tables, and bytes outside the frames never reach them."""
    b = lo.make_block("long", 7)
    want = lo.decode_expect(b.buf, b.off, 7, None)
    rng = np.random.default_rng(5)
    for base in (1, 4099):
        room = rng.integers(0, 256, base + len(b.buf) + 33, dtype=np.uint8)
        room[base:base + len(b.buf)] = b.buf
        got = lo.decode_expect(room, lo.translate(b.off, base), 7, None)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        keep = np.ones(b.n, np.uint8)
        assert lo.gather_expect(room, lo.translate(b.off, base), 7, keep)[0].tobytes() == \
            lo.gather_expect(b.buf, b.off, 7, keep)[0].tobytes()
    w = lo.block_expect(b, sideband=False)
    assert w["status"] == 0 and w["receive"]["info"][6] > 200_000   # the long frame is part of the message
    assert {0, 1} <= set(w["dup"].tolist()) and 1 in w["acknowledge"]["valid"]


def test_rejected_pairs_read_nothing():
    buf = np.arange(4096, dtype=np.uint32).astype(np.uint8)
    off = np.array([0, 40, 99, lo.LINE32 + 200, lo.LINE32 + 300, 400, 459], np.int64)
    w = lo.decode_expect(buf, off, 5, None, lim=4096)
    assert w["good"].tolist() == [True, True, False, False, False, True] and w["status"] == lo.ST_OFFSETS
    assert w["ok"].tolist()[2:5] == [lo.OK_BAD_OFFSETS] * 3 and not w["chars"][2:5].any()
    buf2 = buf.copy()
    buf2[99:400] ^= 0x5A
    w2 = lo.decode_expect(buf2, off, 5, None, lim=4096)
    assert all(np.array_equal(w[k], w2[k]) for k in w)


def test_line_assertions_fire():
    off = np.array([0, 100, 200, 205, 300], np.int64)
    H = 5
    assert lo.assert_line_inside(off, H, lo.LINE31 - 150, lo.LINE31) == 1
    with pytest.raises(AssertionError, match="boundary"):
        lo.assert_line_inside(off, H, lo.LINE31 - 100, lo.LINE31)
    with pytest.raises(AssertionError, match="header"):
        lo.assert_line_inside(off, H, lo.LINE31 - 103, lo.LINE31)
    with pytest.raises(AssertionError, match="within 16 B"):
        lo.assert_line_inside(off, H, lo.LINE31 - 110, lo.LINE31)
    with pytest.raises(AssertionError, match="within 16 B"):
        lo.assert_line_inside(off, H, lo.LINE31 - 190, lo.LINE31)
    with pytest.raises(AssertionError, match="too short"):
        lo.assert_line_inside(np.array([0, 100, 109, 200], np.int64), H, lo.LINE31 - 106, lo.LINE31)
    assert lo.assert_line_inside(np.array([0, 100, 109, 200], np.int64), H, lo.LINE31 - 106, lo.LINE31,
                                 need_margin=False) == 1
    with pytest.raises(AssertionError, match="outside the block"):
        lo.assert_line_inside(off, H, lo.LINE31 - 300, lo.LINE31)
    with pytest.raises(AssertionError, match="outside the block"):
        lo.assert_line_inside(off, H, lo.LINE31 + 1, lo.LINE31)
    # a block of header-only frames cannot hold a line at all
    with pytest.raises(AssertionError, match="no frame"):
        lo.straddle_base(np.arange(0, 505, 5), H, lo.LINE32, need_margin=False)
    # a period that divides the lines puts them on frame boundaries
    with pytest.raises(AssertionError, match="boundary"):
        lo.assert_lines_mid_frame(np.array([0, 16, 32], np.int64), H, lo.periodic_rows(32))
    with pytest.raises(AssertionError, match="does not reach"):
        lo.assert_lines_mid_frame(np.array([0, 21, 42], np.int64), H, 1000)
    B = 33 * 1477
    lo.assert_lines_mid_frame(np.arange(34, dtype=np.int64) * 1477, H, lo.periodic_rows(B))
    assert lo.periodic_rows(B) * B >= lo.LINE32 + 2 * B > (lo.periodic_rows(B) - 1) * B


def test_beyond_names_the_line():
    assert lo.beyond(0) == lo.beyond(lo.LINE31 - 1) == "below 2^31"
    assert lo.beyond(lo.LINE31) == lo.beyond(lo.LINE32 - 1) == "beyond 2^31"
    assert lo.beyond(lo.LINE32) == "beyond 2^32"
