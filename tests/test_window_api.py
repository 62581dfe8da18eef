"""The reordering receiver's rule (tests/window_ref.py) on the CPU: its
reduction to the reference's in-order rule at a window of one character, the
cases written by hand, the model of the device form against the plain loop,
and the argument checks of rudp_accept_window / rudp_gather_ordered that run
before any HIP call."""
import ctypes
import random

import numpy as np
import pytest

from accept_ref import accept_ref, adversarial_stream, golden_cases, parse_rudp5
from rudp import _native, batch
from window_ref import (FIN, NONE, SYN, adversarial_window_stream, chunk_model, ordered_ref, window_ref,
                        window_stream)


def reduces(w, r):
    """window_ref's outputs at Wc = 1 against accept_ref's.  (info[1] counts the
    ranked frames, which is keep's sum; accept_inorder's count of every
    accepted frame is info[6] here.)"""
    assert w.accept.tolist() == r.accept.tolist()
    assert (w.rank != NONE).astype(np.uint8).tolist() == r.keep.tolist()
    assert w.reply.tolist() == r.reply.tolist() and w.reply_ack.tolist() == r.reply_ack.tolist()
    assert w.state == r.state
    assert [w.info[0], w.info[2], w.info[3]] == [r.end, r.msg_start, r.characters]
    assert w.info[1] == int(r.keep.sum()) and w.info[6] == r.count and w.info[5] == 0
    assert (w.carry_rank == NONE).all()
    order = np.argsort(w.rank[w.rank != NONE])
    assert np.flatnonzero(w.rank != NONE)[order].tolist() == np.flatnonzero(r.keep).tolist()  # arrival order


def test_window_of_one_is_the_reference_rule_on_its_own_traces():
    for c in golden_cases():
        seq, flags, payloads = parse_rudp5([bytes.fromhex(h) for h in c["frames"]])
        chars = np.array([len(p.decode()) for p in payloads], np.uint32)
        w = window_ref(seq, flags, chars, None, tuple(c["state"]), c["last_isn"], window_chars=1)
        reduces(w, accept_ref(seq, flags, chars, None, tuple(c["state"]), c["last_isn"]))
        assert w.accept.tolist() == [int(x) for x in c["accepted"]], c["name"]
        assert w.info[0] == c["end"] and list(w.state) == c["state_after"], c["name"]


def test_window_of_one_is_the_reference_rule_on_adversarial_streams():
    rng = random.Random(0x51DE)
    for _ in range(200):
        seq, flags, chars, usable = adversarial_stream(rng, rng.randint(0, 120))
        state = rng.choice(((0, 0, 0), (101, 100, 1), (3, 0, 1)))
        last = rng.choice((None, 100, 5))
        reduces(window_ref(seq, flags, chars, usable, state, last, window_chars=1),
                accept_ref(seq, flags, chars, usable, state, last))


def run(frames, Wc, state=(100, 100, 1), **kw):
    """frames: (seq, flags, chars) triples."""
    seq = np.array([f[0] for f in frames], np.uint16)
    flags = np.array([f[1] for f in frames], np.uint8)
    chars = np.array([f[2] for f in frames], np.uint32)
    return window_ref(seq, flags, chars, None, state, window_chars=Wc, **kw)


def test_gap_filled_by_a_later_frame():
    w = run([(101, 0, 1), (102, 0, 1), (100, 0, 1), (103, 0, 1)], 4)
    assert w.accept.tolist() == [1, 1, 1, 1] and w.rank.tolist() == [1, 2, 0, 3]
    assert w.reply_ack.tolist() == [100, 100, 103, 104] and w.state == (104, 100, 1)
    assert w.info == [4, 4, 4, 4, 4, 0, 4, 0]


def test_fin_delivered_from_pending_ends_at_the_filler():
    w = run([(101, FIN, 1), (100, 0, 1), (102, 0, 1)], 4)
    assert w.info[0] == 1 and w.accept.tolist() == [1, 1, 0] and w.rank.tolist() == [1, 0, NONE]
    assert w.reply.tolist() == [1, 1, 0] and w.reply_ack.tolist() == [100, 102, 0]
    # a pending frame's own FIN waits for its delivery
    w = run([(102, FIN, 1), (100, 0, 1)], 4)
    assert w.info[0] == 2 and w.accept.tolist() == [2, 1] and w.carry_rank.tolist() == [0, NONE]


def test_reset_clears_the_pending_set_and_the_ranks():
    w = run([(100, 0, 1), (102, 0, 1), (500, SYN, 2), (503, 0, 1), (502, 0, 1)], 4)
    assert w.accept.tolist() == [1, 0, 1, 1, 1] and w.rank.tolist() == [NONE, NONE, 0, 2, 1]
    assert w.info[:4] == [5, 3, 2, 4] and w.info[6] == 4 and w.state == (504, 500, 1)


def test_second_frame_for_a_pending_start_is_rejected():
    w = run([(102, 0, 1), (102, 0, 2), (100, 0, 2)], 4)
    assert w.accept.tolist() == [1, 0, 1] and w.rank.tolist() == [1, NONE, 0] and w.state == (103, 100, 1)


def test_window_edge():
    w = run([(100 + 4, 0, 1), (100 + 3, 0, 1), (102, 0, 0)], 4)
    assert w.accept.tolist() == [0, 2, 0] and w.carry_rank.tolist() == [NONE, 0, NONE] and w.info[5] == 1


def test_overlap_eviction():
    # the in-order frame covers the pending start 101: that frame leaves the set
    w = run([(101, 0, 1), (103, 0, 1), (100, 0, 3)], 8)
    assert w.accept.tolist() == [0, 1, 1] and w.rank.tolist() == [NONE, 1, 0] and w.state == (104, 100, 1)


def test_carried_frames_get_no_reply():
    w = run([(102, 0, 1), (103, 0, 1), (100, 0, 1), (101, 0, 1)], 8, n_carried=2)
    assert w.reply.tolist() == [0, 0, 1, 1] and w.reply_ack.tolist() == [0, 0, 101, 104]
    assert w.accept.tolist() == [1, 1, 1, 1] and w.rank.tolist() == [2, 3, 0, 1]


def test_device_form_model_equals_the_rule():
    """chunk_model (csrc/window.hip's steps) against the plain loop, and the
    streams of a windowed sender never reach its sequential walk."""
    import window_ref as wr
    rng = random.Random(0xC4A1)
    old, wr.CHUNK = wr.CHUNK, 16  # small chunks: many hand-overs
    try:
        for t in range(300):
            Wc = rng.choice((1, 2, 3, 8, 16))
            n = rng.randint(0, 70)
            seq, flags, chars, usable = adversarial_window_stream(rng, n, Wc, p_syn=rng.choice((0.0, 0.03, 0.1)))
            state = rng.choice(((0, 0, 0), (101, 100, 1)))
            nc = min(n, rng.choice((0, 1, Wc - 1)))
            a = window_ref(seq, flags, chars, usable, state, 100, window_chars=Wc, n_carried=nc)
            b = chunk_model(seq, flags, chars, usable, state, 100, window_chars=Wc, n_carried=nc)
            for name in ("accept", "rank", "carry_rank", "reply", "reply_ack"):
                assert getattr(a, name).tolist() == getattr(b, name).tolist(), (t, name)
            assert a.state == b.state and a.info[:4] + a.info[5:] == b.info[:4] + b.info[5:], t
        for t in range(200):
            W, C = rng.choice((1, 2, 8, 16)), rng.choice((1, 3))
            n = rng.randint(1, 100)
            seq, flags, chars, usable, state = window_stream(rng, n, W, C, total=rng.choice((None, 30)),
                                                             syn=rng.random() < 0.7, p_unusable=rng.choice((0, 0.05)))
            a = window_ref(seq, flags, chars, usable, state, window_chars=W * C)
            b = chunk_model(seq, flags, chars, usable, state, window_chars=W * C)
            assert a.accept.tolist() == b.accept.tolist() and a.rank.tolist() == b.rank.tolist(), t
            assert b.info[4] == n and a.info[:4] == b.info[:4], t
    finally:
        wr.CHUNK = old


def test_ordered_ref():
    frames = np.frombuffer(b"HHHHHabcHHHHHdeHHHHH", np.uint8)
    off = np.array([0, 8, 15, 20], np.int64)
    out, o, src, st = ordered_ref(frames, off, np.array([1, 0, NONE], np.uint32), 2, 5)
    assert bytes(out) == b"deabc" and o.tolist() == [0, 2, 5] and src.tolist() == [1, 0] and st == 0
    assert ordered_ref(frames, off, np.array([1, 0, 2], np.uint32), 2, 5)[3] == _native.ST_RANK


# ------------------------------------------------------------ argument checks
def test_header_names_the_new_calls():
    from conftest import REPO
    text = (REPO / "include" / "rudp.h").read_text()
    assert "#define RUDP_HAS_ACCEPT_WINDOW 1" in text and "#define RUDP_ABI_VERSION 8" in text
    assert "#define RUDP_ST_RANK 64u" in text and "#define RUDP_RANK_NONE 0xFFFFFFFFu" in text
    assert {"rudp_accept_window", "rudp_gather_ordered"} <= set(_native.EXPORTS)
    assert _native.ST_RANK == 64 and batch.RANK_NONE == NONE


def test_accept_window_argument_errors_before_device():
    lib = _native.lib()
    w = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(w, ctypes.c_void_p)

    def call(n=0, Wc=4, nc=0, st_in=p, st_out=p, info=p, tables=(None,) * 8):
        seq, fl, ch, acc, rank, carry, rep, ack = tables
        return lib.rudp_accept_window(seq, fl, ch, None, n, batch.NO_ISN, Wc, nc, st_in, acc, rank, carry, rep, ack,
                                      st_out, info, 0, None)
    assert call(st_in=None) == _native.EINVAL and b"d_state_in" in lib.rudp_last_error()
    assert call(st_out=None) == _native.EINVAL and b"d_state_out" in lib.rudp_last_error()
    assert call(info=None) == _native.EINVAL and b"d_info" in lib.rudp_last_error()
    for Wc in (0, 1025, 0xFFFFFFFF):
        assert call(Wc=Wc) == _native.EINVAL and b"window_chars" in lib.rudp_last_error()
    assert call(n=3, nc=4, tables=(p,) * 8) == _native.EINVAL and b"n_carried" in lib.rudp_last_error()
    assert call(n=5000, nc=1024, tables=(p,) * 8) == _native.EINVAL and b"n_carried" in lib.rudp_last_error()
    assert call(n=0xFFFFFFFF, tables=(p,) * 8) == _native.EINVAL
    names = ("d_seq", "d_flags", "d_chars", "d_accept", "d_rank", "d_carry_rank", "d_reply", "d_reply_ack")
    for k, name in enumerate(names):
        tables = tuple(None if j == k else p for j in range(8))
        assert call(n=1, tables=tables) == _native.EINVAL and name.encode() in lib.rudp_last_error()


def test_gather_ordered_argument_errors_before_device():
    lib = _native.lib()
    w = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(w, ctypes.c_void_p)

    def call(n=1, skip=5, frames=p, off=p, rank=p, count=p, out=p, out_off=p, status=p, fbytes=8, cap=8):
        return lib.rudp_gather_ordered(frames, fbytes, off, 0, n, rank, count, skip, out, cap, out_off, None, status,
                                       0, None)
    for skip in (1, 6, 8):
        assert call(skip=skip) == _native.EINVAL and b"skip" in lib.rudp_last_error()
    for name in ("status", "count", "off", "rank", "out_off", "frames", "out"):
        assert call(**{name: None}) == _native.EINVAL, name
    assert call(n=0xFFFFFFFF) == _native.EINVAL
    assert call(n=0, frames=None, off=None, rank=None, out=None, out_off=None) == 0  # nothing to do, nothing touched


def test_python_argument_checks():
    with pytest.raises(TypeError, match="torch"):
        batch.accept_window(np.zeros(1, np.uint16), np.zeros(1, np.uint8), np.zeros(1, np.int32), window_chars=4)
    with pytest.raises(TypeError, match="torch"):
        batch.gather_ordered(np.zeros(1, np.uint8), np.zeros(2, np.int64), np.zeros(1, np.int32),
                             np.zeros(1, np.int64), skip=5)
    with pytest.raises(TypeError, match="torch"):
        batch.receive_window(np.zeros(1, np.uint8), np.zeros(2, np.int64), "rudp5", window_chars=4)
    lay = batch.WindowAccepted.layout(7)
    assert lay["rank"] == 0 and lay["state"] % 8 == 0 and lay["size"] == lay["info"] + 64
    assert batch.WINDOW_CHUNK == 1024 and batch.WINDOW_MAX == 1024


def test_geometry_constants_restate_the_source():
    from conftest import PKG
    hip = (PKG / "csrc" / "window_device.hpp").read_text()
    assert f"kWinNew = {batch.WINDOW_CHUNK};" in hip and "uint16_t ring[1024];" in hip


def test_transport_option_checks():
    from rudp.transport import ReliableUDP
    with pytest.raises(ValueError, match="batch_recv"):
        ReliableUDP(reorder_window=8)
    for bad in (0, 1025, True, 2.0):
        with pytest.raises(ValueError, match="reorder_window"):
            ReliableUDP(codec_device="cuda:0", batch_recv=True, reorder_window=bad)
    assert ReliableUDP()._reorder_window is None
