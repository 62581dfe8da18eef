"""rudp_payload_chars / rudp_accept_inorder / batch.receive_batch on the device:
the streams the reference judged (tests/golden/accept.json) in one call and
split over two, characters per payload against numpy for every shape the
kernel's geometry distinguishes, the acceptance against the plain-loop rule on
clean streams (where the one-scan form must have been exact) and adversarial
ones (where the sequential form takes over), and stream capture."""
import random

import numpy as np
import pytest

from accept_ref import (FIN, accept_ref, adversarial_stream, chars_ref, clean_stream, golden_cases, pack_frames,
                        scan_model)
from rudp import _native, batch

pytestmark = pytest.mark.gpu

T = batch.ACCEPT_TILE
SENT8, SENT16, SENT32, SENT64 = 0xA5, 0xA5A5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 8  # sentinel entries on either side of every output


# ----------------------------------------------------------------- helpers
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def chars_call(cuda, frames_t, off_t, H, hint=None):
    """rudp_payload_chars into the middle of a sentinel-filled buffer."""
    import torch
    n = off_t.numel() - 1
    out = torch.full((n + 2 * PAD,), SENT32, dtype=torch.int32, device=cuda)
    hint = frames_t.numel() // max(n, 1) if hint is None else hint
    _native.check(_native.lib().rudp_payload_chars(
        frames_t.data_ptr() if frames_t.numel() else None, frames_t.numel(), off_t.data_ptr(), hint, n,
        out.data_ptr() + 4 * PAD, H, 0, None))
    got = out.cpu().numpy()
    assert (got[:PAD] == SENT32).all() and (got[PAD + n:] == SENT32).all()
    return got[PAD:PAD + n].astype(np.uint32)


class Got:
    pass


def accept_call(cuda, seq, flags, chars, usable=None, state=(0, 0, 0), last_isn=None, alias=False):
    """rudp_accept_inorder with every output between sentinels."""
    import torch
    n = len(seq)
    d_seq, d_fl, d_ch = _dev(cuda, seq), _dev(cuda, flags), _dev(cuda, np.asarray(chars, np.uint32).view(np.int32))
    d_us = _dev(cuda, usable) if usable is not None else None
    u8 = [torch.full((n + 2 * PAD,), SENT8, dtype=torch.uint8, device=cuda) for _ in range(3)]
    ack = torch.from_numpy(np.full(n + 2 * PAD, SENT16, np.uint16)).to(cuda)
    st_in = torch.tensor([state[0], state[1], 1 if state[2] else 0, 0], dtype=torch.int64).to(cuda)
    tail = torch.from_numpy(np.full(4 + 6 + 2 * PAD, SENT64, np.uint64).view(np.int64)).to(cuda)
    st_out = st_in.data_ptr() if alias else tail.data_ptr() + 8 * PAD
    _native.check(_native.lib().rudp_accept_inorder(
        d_seq.data_ptr() if n else None, d_fl.data_ptr() if n else None, d_ch.data_ptr() if n else None,
        d_us.data_ptr() if d_us is not None and n else None, n, batch.NO_ISN if last_isn is None else last_isn,
        st_in.data_ptr(), *(t.data_ptr() + PAD if n else None for t in u8), ack.data_ptr() + 2 * PAD if n else None,
        st_out, tail.data_ptr() + 8 * (PAD + 4), 0, None))
    g = Got()
    for name, t in zip(("accept", "keep", "reply"), u8):
        a = t.cpu().numpy()
        assert (a[:PAD] == SENT8).all() and (a[PAD + n:] == SENT8).all(), name
        setattr(g, name, a[PAD:PAD + n])
    a = ack.cpu().numpy()
    assert (a[:PAD] == SENT16).all() and (a[PAD + n:] == SENT16).all()
    g.reply_ack = a[PAD:PAD + n]
    w = tail.cpu().numpy().view(np.uint64)
    assert (w[:PAD] == SENT64).all() and (w[PAD + 10:] == SENT64).all()
    g.state = st_in.cpu().numpy().view(np.uint64)[:4].tolist() if alias else w[PAD:PAD + 4].tolist()
    if alias:
        assert (w[PAD:PAD + 4] == SENT64).all()
    g.info = w[PAD + 4:PAD + 10].tolist()
    return g


def check_against_rule(g, seq, flags, chars, usable, state, last_isn):
    """Every output equals the plain-loop rule; returns the reported first_anomaly."""
    n = len(seq)
    r = accept_ref(seq, flags, chars, usable, state, last_isn)
    m = scan_model(seq, flags, chars, usable, state, last_isn)
    assert g.accept.tolist() == r.accept.tolist()
    assert g.keep.tolist() == r.keep.tolist()
    assert g.reply.tolist() == r.reply.tolist()
    assert g.reply_ack.tolist() == r.reply_ack.tolist()
    assert g.state == [r.state[0], r.state[1], r.state[2], 0]
    assert g.info[:4] == [r.end, r.count, r.msg_start, r.characters] and g.info[5] == 0
    assert g.info[4] == m.first_anomaly
    if r.end < n:  # nothing behind the end is judged
        assert not g.accept[r.end + 1:].any() and not g.keep[r.end + 1:].any()
        assert not g.reply[r.end + 1:].any() and not g.reply_ack[r.end + 1:].any()
    return g.info[4]


# ------------------------------------------------------- the reference's streams
def _golden_groups():
    groups = {}
    for c in golden_cases():
        key = "scenarios"
        if c["name"].startswith("text"):  # text<index>_chunk<chunk>; the one-character streams are the longest
            index, key = c["name"][4:].split("_")
            key += f"_{int(index) % 3}" if key == "chunk1" else ""
        groups.setdefault(key, []).append(c)
    return groups


GROUPS = _golden_groups()


def _expected(c):
    n = len(c["frames"])
    acc = np.array([int(x) for x in c["accepted"]], np.uint8)
    rep = np.array([int(x) for x in c["replied"]], np.uint8)
    return n, acc, rep, np.array(c["ack"], np.uint16)


def test_golden_receive_batch(cuda):
    """Every stream through receive_batch in one call: the message recv()
    returns, the per-datagram decisions and replies, the end and the state."""
    fast = slow = 0
    for c in golden_cases():
        frames = [bytes.fromhex(h) for h in c["frames"]]
        n, acc, rep, ack = _expected(c)
        buf, off = pack_frames(frames)
        st = c["state"]
        res = batch.receive_batch(_dev(cuda, buf), _dev(cuda, off), "rudp5", state=tuple(st), last_isn=c["last_isn"])
        a = res.accepted
        name = c["name"]
        assert a.accept.cpu().numpy().tolist() == acc.tolist(), name
        assert a.reply.cpu().numpy().tolist() == rep.tolist(), name
        assert a.reply_ack.cpu().numpy().tolist() == ack.tolist(), name
        assert a.end == c["end"] and a.state.cpu().tolist() == c["state_after"] + [0], name
        assert bytes(res.message.check().payload.cpu().numpy()).decode() == c["message"], name
        assert a.characters == (len(c["message"]) if c["state_after"][2] else 0), name
        assert a.count == int(acc.sum()) and len(a) == n, name
        # the replies as a header table: ACK(seq 0, ack = ISN + characters) where one is sent
        assert res.replies.seq.cpu().numpy().tolist() == [0] * n
        assert res.replies.flags.cpu().numpy().tolist() == (rep * batch.ACK).tolist(), name
        assert res.replies.ack.cpu().numpy().tolist() == ack.tolist(), name
        if c["clean"]:
            assert a.fast and a.first_anomaly == n, name
        fast += a.fast
        slow += not a.fast
    assert fast >= 137 and slow == 3  # the three frames from the future took the sequential form


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_golden_two_calls(cuda, group):
    """Every stream cut at every datagram boundary into two calls that carry the
    state (on the device) and the buffer: the same decisions, end, state and
    message as the one call.  A first call that ends the transfer is the whole
    recv(): the datagrams behind it are the next call's."""
    import torch
    for c in GROUPS[group]:
        frames = [bytes.fromhex(h) for h in c["frames"]]
        n, acc, rep, ack = _expected(c)
        buf, off = pack_frames(frames)
        d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
        lens = np.array([len(f) - 5 for f in frames])
        resets = [i for i in range(n) if acc[i] and frames[i][4] & 0x80]
        sig = _dev(cuda, np.concatenate([acc, rep, ack.view(np.uint8)]))
        st_after = torch.tensor(c["state_after"] + [0], dtype=torch.int64, device=cuda)
        bad = torch.zeros((), dtype=torch.int64, device=cuda)

        def part_bytes(lo, hi):
            """The message bytes a call over datagrams [lo, hi) returns."""
            start = max([r for r in resets if lo <= r < hi], default=lo)
            return b"".join(frames[i][5:] for i in range(start, hi) if acc[i])

        def differs(res, lo, hi, want):
            a = res.accepted
            got = torch.cat([a.accept, a.reply, a.reply_ack.view(torch.uint8)])
            exp = torch.cat([sig[lo:hi], sig[n + lo:n + hi], sig[2 * n + 2 * lo:2 * n + 2 * hi]])
            d = (got != exp).sum() + (res.message.payload_off[-1] != len(want))
            if want:
                w = torch.frombuffer(bytearray(want), dtype=torch.uint8).to(cuda)
                d = d + (res.message.buffer[:len(want)] != w).sum()
            return d

        for k in range(1, n):
            one = batch.receive_batch(d_buf[:off[k]], d_off[:k + 1], "rudp5", state=tuple(c["state"]),
                                      last_isn=c["last_isn"])
            if c["end"] < k:
                bad += differs(one, 0, k, part_bytes(0, c["end"] + 1)) + (one.accepted.info[0] != c["end"])
                bad += (one.accepted.state != st_after).sum()
                continue
            two = batch.receive_batch(d_buf[off[k]:], d_off[k:] - int(off[k]), "rudp5", state=one.accepted.state,
                                      last_isn=c["last_isn"])
            hi = min(c["end"] + 1, n)
            bad += differs(one, 0, k, part_bytes(0, k)) + differs(two, k, n, part_bytes(k, hi))
            bad += (one.accepted.info[0] != k) + (two.accepted.info[0] != c["end"] - k)
            bad += (two.accepted.state != st_after).sum()
            # the buffer carries over unless the second call saw a reset
            carried = not any(k <= r < hi for r in resets)
            bad += two.accepted.info[2] != ((n - k) if carried else max(r for r in resets if r < hi) - k)
            whole = (part_bytes(0, k) if carried else b"") + part_bytes(k, hi)
            assert whole.decode() == c["message"], (c["name"], k)  # (the fixture's own consistency)
        assert int(bad.item()) == 0, c["name"]


# ------------------------------------------------------------ payload_chars
ALPHABET = "abcxyz019 \n~" + "éßñ" + "€中文字" + "😀🚀" + "\u0000\u007f\u0080߿ࠀ￿"


def _text_bytes(rng, nbytes):
    """UTF-8 of random 1-4-byte characters, cut to nbytes (so it may end inside a character)."""
    out = bytearray()
    while len(out) < nbytes:
        out += rng.choice(ALPHABET).encode()
    return bytes(out[:nbytes])


def _frames_of_lengths(rng, lengths, H):
    return [bytes(rng.randrange(256) for _ in range(H)) + _text_bytes(rng, L) for L in lengths]


@pytest.mark.parametrize("layout", [5, 7])
def test_payload_chars_lengths_and_alignments(cuda, layout):
    """Every payload length 0..70 and 1470..1480 (and frames shorter than the
    header), at every alignment 1..15 of the frame buffer, with the lanes per
    frame of both a small and an MTU-scale hint."""
    import torch
    rng = random.Random(layout)
    lengths = list(range(0, 71)) + list(range(1470, 1481))
    frames = _frames_of_lengths(rng, lengths, layout) + [b"", b"\x41", b"\x41" * (layout - 1), b"\x41" * layout]
    rng.shuffle(frames)
    buf, off = pack_frames(frames)
    want = chars_ref(buf, off, layout)
    assert want[[len(f) <= layout for f in frames]].sum() == 0 and want.sum() > 10000
    big = torch.zeros(buf.size + 64, dtype=torch.uint8, device=cuda)
    d_off = _dev(cuda, off)
    for mis in range(16):
        view = big[mis:mis + buf.size]
        view.copy_(_dev(cuda, buf))
        for hint in (None, 6, 1479 + layout, 70000):
            assert np.array_equal(chars_call(cuda, view, d_off, layout, hint), want), (mis, hint)
    view = big[3:3 + buf.size]
    view.copy_(_dev(cuda, buf))
    assert np.array_equal(batch.payload_chars(view, d_off, layout).cpu().numpy().view(np.uint32), want)


def test_payload_chars_long_frame_among_small(cuda):
    rng = random.Random(70000)
    frames = _frames_of_lengths(rng, [1] * 700 + [70000] + [1] * 700, 5)
    buf, off = pack_frames(frames)
    want = chars_ref(buf, off, 5)
    assert want[700] > 20000
    for hint in (None, 6, 70005):
        assert np.array_equal(chars_call(cuda, _dev(cuda, buf), _dev(cuda, off), 5, hint), want)


def test_payload_chars_rejected_offsets_read_nothing(cuda):
    """Decreasing and past-the-buffer offsets give 0, and a frame that ends at
    the buffer's last byte counts nothing of the poisoned bytes behind it."""
    import torch
    rng = random.Random(11)
    frames = _frames_of_lengths(rng, [3, 40, 0, 17, 9, 64, 33], 5)
    buf, off = pack_frames(frames)
    room = torch.full((buf.size + 256,), 0x41, dtype=torch.uint8, device=cuda)  # every byte a lead byte
    for mis in (0, 5, 15):
        view = room[mis:mis + buf.size]
        view.copy_(_dev(cuda, buf))
        bad = off.copy()
        bad[2] = off[3] + 1          # frame 1 runs past frame 2's start: frame 2 has decreasing offsets
        bad[7] = buf.size + 100      # the last frame runs past the buffer (into the poison)
        want = chars_ref(buf, bad, 5)
        assert want[2] == 0 and want[6] == 0 and want[1] > 0
        assert np.array_equal(chars_call(cuda, view, _dev(cuda, bad), 5), want), mis
        far = off.copy()
        far[4:] += 1 << 40           # offsets far outside any mapping
        assert np.array_equal(chars_call(cuda, view, _dev(cuda, far), 5), chars_ref(buf, far, 5)), mis
        assert np.array_equal(chars_call(cuda, view, _dev(cuda, off), 5), chars_ref(buf, off, 5)), mis


@pytest.mark.parametrize("layout,plen", [(5, 1), (7, 1), (5, 100), (5, 150), (7, 300), (5, 600), (7, 1472), (5, 5000)])
def test_payload_chars_frame_counts(cuda, layout, plen):
    """n = 1 and around every multiple of the frames a workgroup takes at the
    lanes the launcher picks for this frame length."""
    rng = random.Random(plen)
    lanes = batch.payload_chars_lanes(plen + layout, layout)
    per = batch.CHARS_BLOCK // lanes
    assert lanes == {1: 1, 100: 2, 150: 4, 300: 8, 600: 16, 1472: 32, 5000: 64}[plen]  # every lane count
    pool = _frames_of_lengths(rng, [plen] * 7, layout)
    for n in sorted({1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1} - {0}):
        frames = [pool[i % 7] for i in range(n)]
        buf, off = pack_frames(frames)
        got = chars_call(cuda, _dev(cuda, buf), _dev(cuda, off), layout)
        assert np.array_equal(got, chars_ref(buf, off, layout)), n


# ----------------------------------------------------------- accept_inorder
def test_accept_empty_batch(cuda):
    for state in ((0, 0, 0), (105, 100, 1)):
        for alias in (False, True):
            g = accept_call(cuda, np.zeros(0, np.uint16), np.zeros(0, np.uint8), np.zeros(0, np.uint32), state=state,
                            alias=alias)
            assert g.state == [state[0], state[1], state[2], 0]
            assert g.info == [0, 0, 0, state[0] - state[1] if state[2] else 0, 0, 0]


BASES = batch.ACCEPT_BASES * T  # frames up to which the bases pass has one tile per thread
CLEAN_N = [1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, BASES - 1, BASES, BASES + 1, 300000]


@pytest.mark.parametrize("n", CLEAN_N)
def test_accept_clean_streams(cuda, n):
    """Streams a stop-and-wait sender produces (retransmissions, unusable copies,
    transfers abandoned for a new SYN, resets and the FIN on the first and last
    frame of a tile): equal to the rule, and the one-scan form was exact."""
    rng = random.Random(n)
    edges = [e for e in (T - 1, T, 2 * T - 1, 2 * T) if e < n]
    fins = [None, n - 1] + ([((n - 1) // T) * T, ((n - 1) // T) * T - 1] if n > T else [])
    if n > 3 * T:
        fins = fins[1:3]  # the large sizes: only streams judged (nearly) to their end
    for fin_at in fins:
        # (a transfer stalled at the 2^16 wrap never accepts its FIN: those ISNs only where none is placed)
        seq, flags, chars, usable = clean_stream(rng, n, resets=edges, fin_at=fin_at,
                                                 max_chars=1 if n > 3 * T else rng.choice((1, 3)),
                                                 high_isn=0.05 if fin_at is None else 0.0)
        state = rng.choice(((0, 0, 0), (0, 0, 1)))
        g = accept_call(cuda, seq, flags, chars, usable, state, 6000, alias=fin_at is None)
        assert check_against_rule(g, seq, flags, chars, usable, state, 6000) == n, fin_at
        if fin_at is not None:
            assert g.info[0] == fin_at
    # the same without a usable mask, from a live state in the middle of a transfer:
    # the first frame is no SYN but the in-order frame the state expects
    seq, flags, chars, _ = clean_stream(rng, min(n, 3 * T), p_unusable=0.0)
    flags[0] = 0
    state = (int(seq[0]), max(int(seq[0]) - 10, 0), 1)
    g = accept_call(cuda, seq, flags, chars, None, state, None)
    assert check_against_rule(g, seq, flags, chars, None, state, None) == len(seq)


def _both_forms(cuda, fn):
    """fn() with batches up to one tile in one launch (the product's form), then
    in the five launches of larger batches (the diagnostics build's knob 79)."""
    fn()
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(79, 0) == 1
        fn()
    finally:
        tools.rudpx_tune(79, 1)
        _native.use_product()


def test_accept_adversarial_streams(cuda):
    """Random seq_num, flags and characters; both the exact one-scan results and
    the sequential continuation must have run, in both launch forms."""
    paths = {"fast": 0, "slow": 0}

    def run():
        rng = random.Random(0xADE5)
        for k in range(40):
            n = rng.choice((1, 2, 7, 64, 255, 257, 600, T, T + 1, 2 * T + 5, 3000))
            seq, flags, chars, usable = adversarial_stream(rng, n, p_fin=rng.choice((0.0, 0.002, 0.02)))
            state = rng.choice(((0, 0, 0), (0, 0, 1), (105, 100, 1), (65536, 65530, 1)))
            last = rng.choice((None, int(seq[0]), 3611))
            g = accept_call(cuda, seq, flags, chars, usable, state, last, alias=k % 2 == 0)
            first = check_against_rule(g, seq, flags, chars, usable, state, last)
            paths["fast" if first == n else "slow"] += 1

    _both_forms(cuda, run)
    assert paths["fast"] >= 4 and paths["slow"] >= 4, paths


def test_accept_placed_anomalies(cuda):
    """The anomaly at index 0, at a tile's last frame, in a later tile, and
    behind an accepted FIN (then it is not one: the frames there are not judged)."""
    def run():
        rng = random.Random(79)
        n = 3 * T + 100
        for at, fin_at, want in ((0, n - 1, 0), (T - 1, n - 1, T - 1), (2 * T + 17, None, 2 * T + 17),
                                 (600, 500, n), (T, T - 1, n), (5, 900, 5)):
            seq, flags, chars, usable = clean_stream(rng, n, fin_at=fin_at, p_reset=0.0, p_unusable=0.02, high_isn=0.0)
            state = (0, 0, 0)
            if at == 0:  # a live receiver whose first datagram comes from the future
                state, flags[0] = (int(seq[0]), int(seq[0]), 1), 0
                flags[1:] &= 0x7F
                seq[1:] = int(seq[0]) + 100  # (and nothing in order behind it)
            seq[at], flags[at], usable[at] = (int(seq[at]) + 50) & 0xFFFF, flags[at] & FIN, 1
            g = accept_call(cuda, seq, flags, chars, usable, state, None)
            assert check_against_rule(g, seq, flags, chars, usable, state, None) == want, (at, fin_at)
        # the sequential form over more than one of its LDS blocks, ended by a FIN it finds itself
        seq, flags, chars, usable = clean_stream(rng, n, fin_at=n - 7, p_reset=0.001, high_isn=0.0)
        # (a retransmission is replaced, so the transfer itself loses nothing and goes on to its FIN)
        at = next(i for i in range(3, n) if seq[i] == seq[i - 1] and usable[i - 1] and not flags[i] & 0x80)
        seq[at], flags[at], usable[at] = int(seq[at]) + 9, 0, 1
        g = accept_call(cuda, seq, flags, chars, usable, (0, 0, 0), None)
        assert check_against_rule(g, seq, flags, chars, usable, (0, 0, 0), None) == at
        assert g.info[0] == n - 7

    _both_forms(cuda, run)


def test_receive_batch_under_stream_capture(cuda):
    """A captured receive_batch replays to the eager result: no call of the
    chain waits for the device or allocates outside the graph."""
    import torch
    c = next(c for c in golden_cases() if c["name"] == "text5_chunk1")
    frames = [bytes.fromhex(h) for h in c["frames"]]
    buf, off = pack_frames(frames)
    d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
    state = torch.tensor(c["state"] + [0], dtype=torch.int64, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        eager = batch.receive_batch(d_buf, d_off, "rudp5", state=state, last_isn=c["last_isn"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap = batch.receive_batch(d_buf, d_off, "rudp5", state=state, last_isn=c["last_isn"])
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for name in ("accept", "keep", "reply"):
        assert torch.equal(getattr(cap.accepted, name), getattr(eager.accepted, name)), name
    assert torch.equal(cap.accepted.reply_ack.view(torch.uint8), eager.accepted.reply_ack.view(torch.uint8))
    assert torch.equal(cap.accepted.state, eager.accepted.state) and torch.equal(cap.accepted.info, eager.accepted.info)
    assert cap.accepted.end == c["end"] and cap.accepted.fast
    assert bytes(cap.message.payload.cpu().numpy()).decode() == c["message"]
