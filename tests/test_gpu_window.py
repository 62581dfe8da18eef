"""rudp_accept_window / rudp_gather_ordered / batch.receive_window on the
device: every output of the acceptance against the plain-loop rule
(tests/window_ref.py) for the sizes at which the chunked form takes another
path, the streams of a windowed sender judged without the sequential walk,
adversarial streams and placed anomalies; the reduction to rudp_accept_inorder
at a window of one character; the pending frames of one call carried into the
next; the ordered gather against numpy; and stream capture."""
import random

import numpy as np
import pytest

from accept_ref import adversarial_stream, clean_stream, golden_cases, pack_frames
from rudp import _native, batch
from window_ref import (FIN, NONE, ST_OFFSETS, ST_PAYLOAD_CAP, ST_RANK, SYN, adversarial_window_stream,
                        ordered_ref, window_ref, window_stream)

pytestmark = pytest.mark.gpu

T = batch.WINDOW_CHUNK
SENT8, SENT16, SENT32, SENT64 = 0xA5, 0xA5A5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 8  # sentinel entries on either side of every output


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class Got:
    pass


def window_call(cuda, seq, flags, chars, usable, state, last_isn, Wc, nc, alias=False):
    """rudp_accept_window with every output between sentinels."""
    import torch
    n = len(seq)
    d_seq, d_fl, d_ch = _dev(cuda, seq), _dev(cuda, flags), _dev(cuda, np.asarray(chars, np.uint32).view(np.int32))
    d_us = _dev(cuda, usable) if usable is not None else None
    u8 = [torch.full((n + 2 * PAD,), SENT8, dtype=torch.uint8, device=cuda) for _ in range(2)]
    u32 = [torch.full((n + 2 * PAD,), SENT32, dtype=torch.int32, device=cuda) for _ in range(2)]
    ack = torch.from_numpy(np.full(n + 2 * PAD, SENT16, np.uint16)).to(cuda)
    st_in = torch.tensor([state[0], state[1], 1 if state[2] else 0, 0], dtype=torch.int64).to(cuda)
    tail = torch.from_numpy(np.full(4 + 8 + 2 * PAD, SENT64, np.uint64).view(np.int64)).to(cuda)
    st_out = st_in.data_ptr() if alias else tail.data_ptr() + 8 * PAD

    def at(t, width):
        return t.data_ptr() + width * PAD if n else None
    _native.check(_native.lib().rudp_accept_window(
        d_seq.data_ptr() if n else None, d_fl.data_ptr() if n else None, d_ch.data_ptr() if n else None,
        d_us.data_ptr() if d_us is not None and n else None, n, batch.NO_ISN if last_isn is None else last_isn,
        Wc, nc, st_in.data_ptr(), at(u8[0], 1), at(u32[0], 4), at(u32[1], 4), at(u8[1], 1), at(ack, 2), st_out,
        tail.data_ptr() + 8 * (PAD + 4), 0, None))
    g = Got()
    for name, t, sent in (("accept", u8[0], SENT8), ("reply", u8[1], SENT8), ("rank", u32[0], SENT32),
                          ("carry_rank", u32[1], SENT32), ("reply_ack", ack, SENT16)):
        a = t.cpu().numpy()
        assert (a[:PAD] == sent).all() and (a[PAD + n:] == sent).all(), name
        a = a[PAD:PAD + n]
        setattr(g, name, a.view(np.uint32) if a.dtype == np.int32 else a)
    w = tail.cpu().numpy().view(np.uint64)
    assert (w[:PAD] == SENT64).all() and (w[PAD + 12:] == SENT64).all()
    g.state = st_in.cpu().numpy().view(np.uint64)[:4].tolist() if alias else w[PAD:PAD + 4].tolist()
    if alias:
        assert (w[PAD:PAD + 4] == SENT64).all()
    g.info = w[PAD + 4:PAD + 12].tolist()
    return g


def check_against_rule(cuda, seq, flags, chars, usable, state, last_isn, Wc, nc, alias=False):
    """Every output array and info word equals the plain-loop rule; returns the
    reported first_anomaly."""
    g = window_call(cuda, seq, flags, chars, usable, state, last_isn, Wc, nc, alias)
    r = window_ref(seq, flags, chars, usable, state, last_isn, window_chars=Wc, n_carried=nc)
    for name in ("accept", "rank", "carry_rank", "reply", "reply_ack"):
        got, want = getattr(g, name), getattr(r, name)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (name, len(seq), Wc, nc, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert g.state == [r.state[0], r.state[1], r.state[2], 0]
    assert g.info[:4] == r.info[:4] and g.info[5:] == r.info[5:], (g.info, r.info)
    assert g.info[4] <= len(seq)
    return g.info[4]


SIZES = (0, 1, 2, 7, 64, 255, 1023, 1024, 1025, 2049, 3000)
GEOMETRY = {1: (1, 1), 2: (2, 1), 8: (4, 2), 64: (64, 1), 1024: (128, 8)}  # Wc -> frames in flight, characters each


@pytest.mark.parametrize("Wc", sorted(GEOMETRY))
def test_windowed_sender_streams_never_walk(cuda, Wc):
    """What a windowed cumulative sender leaves under loss, duplication and
    swaps: equal to the rule and judged by the parallel form alone."""
    rng = random.Random(0xA110 + Wc)
    W, C = GEOMETRY[Wc]
    for n in SIZES:
        for nc in sorted({0, min(n, 1), min(n, Wc - 1)}):
            syn = rng.random() < 0.6
            seq, flags, chars, usable, state = window_stream(
                rng, n, W, C, syn=syn, total=rng.choice((None, None, max(n // 2, 2))),
                p_unusable=rng.choice((0.0, 0.03)))
            first = check_against_rule(cuda, seq, flags, chars, usable, state, None, Wc, nc, alias=bool(n & 1))
            assert first == n, (n, Wc, nc, first)


@pytest.mark.parametrize("Wc", sorted(GEOMETRY))
def test_adversarial_streams(cuda, Wc):
    """Frames from the past, ahead inside and beyond the window, repeated starts,
    empty payloads, competing SYNs, seq_num near 65535: the walk takes over."""
    rng = random.Random(0xADD0 + Wc)
    walked = 0
    for n in SIZES:
        for nc in sorted({0, min(n, 1), min(n, Wc - 1)}):
            seq, flags, chars, usable = adversarial_window_stream(rng, n, Wc, p_syn=rng.choice((0.0, 0.01, 0.08)))
            state = rng.choice(((0, 0, 0), (101, 100, 1), (int(seq[0]) if n else 0, 0, 1)))
            first = check_against_rule(cuda, seq, flags, chars, usable, state, rng.choice((None, 100)), Wc, nc)
            walked += first < n
    assert walked >= 5


def test_placed_anomalies(cuda):
    """One frame beyond the window placed into a windowed sender's stream: the
    chunk that holds it walks from there, the chunks after it do not."""
    rng = random.Random(0x91AC)
    n, Wc = 3 * T + 100, 8
    seq, flags, chars, usable, state = window_stream(rng, n, 4, 2, syn=False, p_unusable=0.0)
    for at in (0, T - 1, T, 2 * T + 3):
        far = (int(seq[at]) + 5 * Wc) & 0xFFFF
        s2 = np.insert(seq, at, far)[:n]
        f2 = np.insert(flags, at, 0)[:n]
        c2 = np.insert(chars, at, 2)[:n]
        u2 = np.insert(usable, at, 1)[:n]
        assert check_against_rule(cuda, s2, f2, c2, u2, state, None, Wc, 0) == at
    # an in-order frame without characters is the other anomaly
    r = window_ref(seq, flags, chars, usable, state, window_chars=Wc)
    at = T + 17
    expect_before = window_ref(seq[:at], flags[:at], chars[:at], usable[:at], state, window_chars=Wc).state[0]
    s2, f2 = np.insert(seq, at, expect_before & 0xFFFF)[:n], np.insert(flags, at, 0)[:n]
    c2, u2 = np.insert(chars, at, 0)[:n], np.insert(usable, at, 1)[:n]
    assert check_against_rule(cuda, s2, f2, c2, u2, state, None, Wc, 0) == at
    assert r.info[4] == n


# ------------------------------------------------------------------ reduction
def test_window_of_one_is_accept_inorder_bit_for_bit(cuda):
    import torch
    rng = random.Random(0x1DE1)
    streams = []
    for n in (0, 1, 7, 255, 1024, 1025, 3000):
        seq, flags, chars, usable = clean_stream(rng, n, fin_at=n - 1 if n & 1 else None, max_chars=3)
        streams.append((seq, flags, chars, usable, (0, 0, 0)))
        streams.append(adversarial_stream(rng, n) + (rng.choice(((0, 0, 0), (101, 100, 1))),))
    for seq, flags, chars, usable, state in streams:
        n = len(seq)
        d = [_dev(cuda, seq), _dev(cuda, flags), _dev(cuda, np.asarray(chars, np.uint32).view(np.int32))]
        us = _dev(cuda, usable)
        a = batch.accept_inorder(*d, usable=us, state=state, last_isn=100)
        w = batch.accept_window(*d, window_chars=1, usable=us, state=state, last_isn=100)
        assert torch.equal(w.accept, a.accept) and torch.equal((w.rank != -1).to(torch.uint8), a.keep)
        assert torch.equal(w.reply, a.reply)
        assert torch.equal(w.reply_ack.view(torch.uint8), a.reply_ack.view(torch.uint8))
        assert torch.equal(w.state, a.state)
        wi, ai = w.info.tolist(), a.info.tolist()
        # (info[1] counts the ranked frames, keep's sum; every accepted frame is info[6])
        assert [wi[0], wi[2], wi[3]] == [ai[0], ai[2], ai[3]] and wi[6] == ai[1], (n, wi, ai)
        assert wi[1] == int(a.keep.sum()) and wi[5] == 0


def test_golden_receive_window_of_one_is_receive(cuda):
    """The reference's own traces through receive_window at a window of one
    character: batch.receive's message, replies and state."""
    import torch
    for c in golden_cases():
        frames = [bytes.fromhex(h) for h in c["frames"]]
        buf, off = pack_frames(frames)
        d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
        want = batch.receive(d_buf, d_off, "rudp5", state=tuple(c["state"]), last_isn=c["last_isn"])
        got = batch.receive_window(d_buf, d_off, "rudp5", window_chars=1, state=tuple(c["state"]),
                                   last_isn=c["last_isn"])
        name = c["name"]
        assert bytes(got.message.check().payload.cpu().numpy()).decode() == c["message"], name
        assert torch.equal(got.message.payload, want.message.payload), name
        assert torch.equal(got.state, want.state) and got.state.tolist() == c["state_after"] + [0], name
        R = want.reply_count
        assert got.reply_count == R, name
        assert got.reply_index.tolist() == want.reply_index[:R].tolist(), name
        assert got.reply_peer.tolist() == want.reply_peer[:R].tolist(), name
        assert torch.equal(got.reply_frames("rudp5"), want.reply_frames[:5 * R]), name
        assert got.accepted.end == c["end"] and got.carried.count == 0, name


# ------------------------------------------------------------------ two calls
def make_frames(rng, seq, flags, chars):
    """rudp5 datagrams with payloads of chars[i] characters of 1 to 4 bytes."""
    alphabet = "az09 éß€世\U0001F600\U00010348"
    out = []
    for s, f, c in zip(seq.tolist(), flags.tolist(), chars.tolist()):
        text = "".join(rng.choice(alphabet) for _ in range(c))
        out.append(int(s).to_bytes(2, "big") + b"\x00\x00" + bytes([f]) + text.encode())
    return out


def message_of(frames, res):
    order = np.argsort(res.rank[res.rank != NONE])
    return b"".join(frames[i][5:] for i in np.flatnonzero(res.rank != NONE)[order])


def two_calls(cuda, frames, seq, flags, chars, state, Wc, k):
    """Datagrams [0, k) in one call, its pending frames and [k, n) in the next."""
    n = len(frames)
    whole = window_ref(seq, flags, chars, None, state, window_chars=Wc)
    buf, off = pack_frames(frames)
    d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
    one = batch.receive_window(d_buf[:off[k]], d_off[:k + 1], "rudp5", window_chars=Wc, state=state)
    r1 = window_ref(seq[:k], flags[:k], chars[:k], None, state, window_chars=Wc)
    assert bytes(one.message.check().payload.cpu().numpy()) == message_of(frames[:k], r1)
    if r1.info[0] < k:  # the transfer ended in the first call: the rest is the next recv()'s
        return
    pend = np.flatnonzero(r1.accept == 2)
    assert one.carried.count == len(pend)
    two = batch.receive_window(d_buf[off[k]:], d_off[k:] - int(off[k]), "rudp5", window_chars=Wc,
                               carried=one.carried, state=one.state)
    idx = np.concatenate([pend, np.arange(k, n)]).astype(np.int64)
    r2 = window_ref(seq[idx], flags[idx], chars[idx], None, r1.state, window_chars=Wc, n_carried=len(pend))
    m = len(pend)
    part2 = bytes(two.message.check().payload.cpu().numpy())
    assert part2 == message_of([frames[i] for i in idx], r2)
    joined = part2 if r2.info[2] < len(idx) else bytes(one.message.payload.cpu().numpy()) + part2
    assert joined == message_of(frames, whole), k
    assert two.state.tolist() == [whole.state[0], whole.state[1], whole.state[2], 0], k
    assert two.accepted.reply[m:].cpu().numpy().tolist() == r2.reply[m:].tolist(), k
    assert two.accepted.reply_ack[m:].cpu().numpy().tolist() == r2.reply_ack[m:].tolist(), k
    assert two.reply_index.tolist() == np.flatnonzero(r2.reply[m:]).tolist(), k
    assert two.carried.count == whole.info[5], k


def test_two_call_carry_at_every_cut(cuda):
    rng = random.Random(0xCA44)
    seq, flags, chars, usable, state = window_stream(rng, 40, 8, 1, p_loss=0.1, p_swap=0.2, total=30)
    frames = make_frames(rng, seq, flags, chars)
    for k in range(1, 40):
        two_calls(cuda, frames, seq, flags, chars, state, 8, k)


def test_two_call_carry_across_a_chunk(cuda):
    rng = random.Random(0xCA45)
    seq, flags, chars, usable, state = window_stream(rng, 1500, 16, 2, p_loss=0.1, p_swap=0.2)
    frames = make_frames(rng, seq, flags, chars)
    two_calls(cuda, frames, seq, flags, chars, state, 32, 1024)


# ------------------------------------------------------------ gather_ordered
def ordered_call(cuda, frames, off, rank, K, skip, *, cap=None, fmis=0, omis=0, want_src=True):
    """rudp_gather_ordered into a buffer with 64-byte sentinel guards around
    d_out, from a frames view `fmis` bytes into its allocation."""
    import torch
    n = len(off) - 1
    want, woff, wsrc, wst = ordered_ref(frames, off, rank, K, skip)
    cap = len(want) if cap is None else cap
    d_all = torch.cat([torch.zeros(fmis, dtype=torch.uint8), torch.from_numpy(np.array(frames, np.uint8))]).to(cuda)
    d_frames = d_all[fmis:]
    d_off = _dev(cuda, np.asarray(off, np.int64))
    d_rank = _dev(cuda, np.asarray(rank, np.uint32).view(np.int32))
    d_count = torch.tensor([K], dtype=torch.int64, device=cuda)
    out = torch.full((omis + 64 + cap + 64,), SENT8, dtype=torch.uint8, device=cuda)
    tab = torch.from_numpy(np.full(n + 1 + 2 * PAD, SENT64, np.uint64).view(np.int64)).to(cuda)
    src = torch.full((n + 2 * PAD,), SENT32, dtype=torch.int32, device=cuda)
    status = torch.full((1,), 0x7777, dtype=torch.int32, device=cuda)
    _native.check(_native.lib().rudp_gather_ordered(
        d_frames.data_ptr() if len(frames) else None, len(frames), d_off.data_ptr(), len(frames) // max(n, 1), n,
        d_rank.data_ptr(), d_count.data_ptr(), skip, out.data_ptr() + omis + 64, cap, tab.data_ptr() + 8 * PAD,
        src.data_ptr() + 4 * PAD if want_src else None, status.data_ptr(), 0, None))
    o = out.cpu().numpy()
    st = int(status.item())
    Kc = min(K, n)
    t = tab.cpu().numpy().view(np.uint64)
    assert (t[:PAD] == SENT64).all() and (t[PAD + Kc + 1:] == SENT64).all()  # nothing past index K
    assert t[PAD:PAD + Kc + 1].tolist() == woff.tolist()
    sr = src.cpu().numpy()
    if want_src:
        assert (sr[:PAD] == SENT32).all() and (sr[PAD + Kc:] == SENT32).all()
        assert sr[PAD:PAD + Kc].astype(np.int64).tolist() == wsrc.tolist()
    else:
        assert (sr == SENT32).all()
    assert (o[:omis + 64] == SENT8).all() and (o[omis + 64 + cap:] == SENT8).all()  # the guards
    if len(want) > cap:
        assert st == wst | ST_PAYLOAD_CAP and (o == SENT8).all()  # nothing written, the size reported
    else:
        assert st == wst
        assert o[omis + 64:omis + 64 + len(want)].tobytes() == want.tobytes()
        assert (o[omis + 64 + len(want):] == SENT8).all()  # nothing at or past the total
    return st


def ragged_frames(rng, n, H, shape):
    if shape == "ragged":
        lens = [rng.choice((0, 1, H - 1, H, H + 1, rng.randint(0, 5000))) for _ in range(n)]
    elif shape == "long_among_short":
        lens = [H + rng.randint(0, 3) for _ in range(n)]
        lens[rng.randrange(n)] = 5000
    else:
        lens = [H + rng.randint(1, 4) for _ in range(n)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    frames = np.frombuffer(random.Random(rng.random()).randbytes(int(off[-1])), np.uint8).copy()
    return frames, off


@pytest.mark.parametrize("skip", (0, 5, 7))
def test_gather_ordered_permutations(cuda, skip):
    rng = random.Random(0x0DE4 + skip)
    for n, shape in ((1, "ragged"), (7, "ragged"), (257, "ragged"), (300, "long_among_short"), (1500, "small")):
        frames, off = ragged_frames(rng, n, max(skip, 5), shape)
        for frac in (1.0, 0.5):
            K = int(n * frac)
            perm = list(range(n))
            rng.shuffle(perm)
            rank = np.full(n, NONE, np.uint32)
            rank[perm[:K]] = np.arange(K, dtype=np.uint32)
            st = ordered_call(cuda, frames, off, rank, K, skip, fmis=rng.choice((0, 1, 3, 9)),
                              omis=rng.choice((0, 1, 5)), want_src=bool(K & 1) or n < 8)
            assert st == 0


def test_gather_ordered_identity_is_gather_payloads(cuda):
    import torch
    rng = random.Random(0x1DE7)
    for H, layout in ((5, "rudp5"), (7, "rudp7")):
        frames, off = ragged_frames(rng, 700, H, "ragged")
        keep = np.array([rng.random() < 0.7 for _ in range(700)], np.uint8)
        rank = np.where(keep, np.cumsum(keep) - 1, NONE).astype(np.uint32)
        d_frames, d_off = _dev(cuda, frames), _dev(cuda, off)
        want = batch.gather_payloads(d_frames, d_off, layout, keep=_dev(cuda, keep))
        K = torch.tensor([int(keep.sum())], dtype=torch.int64, device=cuda)
        got = batch.gather_ordered(d_frames, d_off, _dev(cuda, rank.view(np.int32)), K, skip=H).check()
        assert torch.equal(got.payload, want.payload)
        assert got.total == (int(keep.sum()), int(want.payload_off[-1].item()))
        kept = torch.from_numpy(np.flatnonzero(keep)).to(cuda)
        assert torch.equal(got.out_off[:got.total[0]], want.payload_off[kept])
        assert torch.equal(got.src[:got.total[0]].long(), kept)


def test_gather_ordered_checked_behaviours(cuda):
    rng = random.Random(0xBE4A)
    frames, off = ragged_frames(rng, 40, 5, "ragged")
    rank = np.arange(40, dtype=np.uint32)[::-1].copy()
    total = len(ordered_ref(frames, off, rank, 40, 5)[0])
    assert total > 64
    # the output one byte too small: nothing written, the size in out_off[K]
    assert ordered_call(cuda, frames, off, rank, 40, 5, cap=total - 1) == ST_PAYLOAD_CAP
    # ranks at or above K that are not NONE are skipped
    assert ordered_call(cuda, frames, off, rank, 30, 5) == ST_RANK
    big = rank.copy()
    big[3] = 0xFFFFFFFE
    assert ordered_call(cuda, frames, off, big, 40, 5) == ST_RANK  # (its rank has no frame: an empty entry)
    # K above n counts as n
    assert ordered_call(cuda, frames, off, rank, 1000, 5) == 0
    # frames whose offsets are decreasing or past the buffer contribute nothing and are not read
    bad = off.copy()
    bad[10] = bad[11] + 7
    assert ordered_call(cuda, frames, bad, rank, 40, 5) == ST_OFFSETS
    past = off.copy()
    past[-1] = len(frames) + 4096
    assert ordered_call(cuda, frames, past, rank, 40, 5) == ST_OFFSETS
    assert ordered_call(cuda, frames, off, np.full(40, NONE, np.uint32), 0, 5) == 0  # K == 0: out_off[0] alone


# -------------------------------------------------------------- stream capture
def test_window_calls_under_stream_capture(cuda):
    """One call of each entry captured and replayed: nothing waits for the
    device or allocates outside the graph."""
    import torch
    rng = random.Random(0xCA97)
    seq, flags, chars, usable, state = window_stream(rng, 1500, 8, 1, total=1400)
    frames = make_frames(rng, seq, flags, chars)
    buf, off = pack_frames(frames)
    d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
    d = [_dev(cuda, seq), _dev(cuda, flags), _dev(cuda, chars.view(np.int32))]
    st = torch.tensor(list(state) + [0], dtype=torch.int64, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))

    def both():
        acc = batch.accept_window(*d, window_chars=8, state=st)
        return acc, batch.gather_ordered(d_buf, d_off, acc.rank, acc.info[1:2], skip=5)
    with torch.cuda.stream(s):
        eager_acc, eager_msg = both()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap_acc, cap_msg = both()
    g.replay()
    torch.cuda.synchronize()
    for name in ("accept", "rank", "carry_rank", "reply", "state", "info"):
        assert torch.equal(getattr(cap_acc, name), getattr(eager_acc, name)), name
    assert torch.equal(cap_acc.reply_ack.view(torch.uint8), eager_acc.reply_ack.view(torch.uint8))
    r = window_ref(seq, flags, chars, None, state, window_chars=8)
    assert cap_acc.info.tolist() == r.info and cap_acc.fast
    assert bytes(cap_msg.check().payload.cpu().numpy()) == message_of(frames, r)
    assert torch.equal(cap_msg.payload, eager_msg.payload)
