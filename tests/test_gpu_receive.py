"""rudp_receive / batch.receive on the device.  The oracle everywhere is the
existing chain (unpack_batch_varlen(utf8=True) -> keep_mask -> payload_chars ->
accept_inorder -> gather_payloads), itself pinned to the reference: every array
of the one call must equal the chain's byte for byte, the reply datagrams must
be pack_batch's frames of (0, reply_ack, ACK), and reply_index / reply_peer a
plain host loop's.  Every fused-eligible input runs in both forms (knob 80 of
the diagnostics build turns the fused kernel off)."""
import random

import numpy as np
import pytest

from accept_ref import FIN, SYN, adversarial_stream, clean_stream, golden_cases, pack_frames
from rudp import _native, batch

pytestmark = pytest.mark.gpu

T = batch.RECV_TILE
FB = batch.RECV_FUSED_BYTES
MEAN = batch.RECV_FUSED_MEAN
PAD = 16      # sentinel bytes on either side of every output
SENT = 0xA5
NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
TABLES = (("seq", "u16"), ("ack", "u16"), ("flags", "u8"), ("ok", "u8"), ("csum_out", "u16"), ("valid", "u8"),
          ("usable", "u8"), ("chars", "u32"), ("accept", "u8"), ("keep", "u8"), ("reply", "u8"), ("reply_ack", "u16"),
          ("reply_csum", "u16"), ("reply_index", "u32"), ("reply_peer", "u64"))


# ----------------------------------------------------------------- helpers
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _forms(fn):
    """fn('fused') with the product library, then fn('chained') with the fused
    form turned off in the diagnostics build."""
    fn("fused")
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(80, 0) == 1
        fn("chained")
    finally:
        tools.rudpx_tune(80, 1)
        _native.use_product()


def make_batch(cuda, seq, flags, payloads, H, ack=None):
    """Frames of the library's own encode: (u8 buffer, int64 offsets, u16 checksums) as numpy."""
    n = len(seq)
    body = np.frombuffer(b"".join(payloads), np.uint8).copy()
    lens = np.array([len(p) for p in payloads], np.int32)
    ack = np.zeros(n, np.uint16) if ack is None else ack
    fr = batch.pack_batch_varlen((_dev(cuda, np.asarray(seq, np.uint16)), _dev(cuda, ack),
                                  _dev(cuda, np.asarray(flags, np.uint8))), _dev(cuda, body), _dev(cuda, lens), H,
                                 want_csum=True)
    return fr.frames.cpu().numpy().copy(), fr.frame_off.cpu().numpy().copy(), fr.csum.cpu().numpy().copy()


CHARS = ("a", "é", "€", "😀")  # 1, 2, 3 and 4 bytes


def text_of(rng, chars, widths=(1,)):
    return "".join(CHARS[rng.choice(widths) - 1] for _ in range(chars)).encode()


def stream_batch(cuda, rng, stream, H, widths=(1,)):
    """A (seq, flags, chars, usable) stream as frames; an unusable frame gets a
    flipped payload bit (or, with no payload, a flipped seq bit), so its
    checksum fails.  Returns frames, offsets, checksums (numpy)."""
    seq, flags, chars, usable = stream
    buf, off, cs = make_batch(cuda, seq, flags, [text_of(rng, int(c), widths) for c in chars], H)
    for i in np.flatnonzero(np.asarray(usable) == 0):
        at = int(off[i + 1]) - 1 if off[i + 1] - off[i] > H else int(off[i])
        buf[at] ^= 0x01
    return buf, off, cs


class Case:
    """One input on the device and the chain's answer for it, computed once."""

    def __init__(self, cuda, buf, off, H, csum=None, state=(0, 0, 0), last_isn=None, mis=0, cap=None):
        import torch
        self.cuda, self.H, self.n, self.last_isn, self.state = cuda, H, len(off) - 1, last_isn, state
        self.nbytes = len(buf)
        self.room = torch.full((len(buf) + 64,), SENT, dtype=torch.uint8, device=cuda)  # guard bytes around the view
        self.frames = self.room[16 + mis:16 + mis + len(buf)]
        assert self.frames.data_ptr() % 16 == mis
        self.frames.copy_(_dev(cuda, np.asarray(buf, np.uint8)))
        self.off = _dev(cuda, np.asarray(off, np.int64))
        self.csum = None if csum is None else _dev(cuda, np.asarray(csum, np.uint16))
        self.cap = len(buf) if cap is None else cap
        self.want = self._chain()

    def _chain(self):
        import torch
        n, H, w = self.n, self.H, {}
        st = torch.tensor([self.state[0], self.state[1], 1 if self.state[2] else 0, 0], dtype=torch.int64).to(self.cuda)
        if n == 0:
            live = 1 if self.state[2] else 0
            w["state"] = [self.state[0], self.state[1], live, 0]
            w["info"] = [0, 0, 0, self.state[0] - self.state[1] if live else 0, 0, 0, 0, 0]
            w["status"], w["R"], w["total"] = 0, 0, 0
            return w
        dec = batch.unpack_batch_varlen(self.frames, self.off, H, csum=self.csum, check=False, utf8=True)
        usable = batch.keep_mask(dec, unverified=H == 5 and self.csum is None)
        chars = batch.payload_chars(self.frames, self.off, H)
        acc = batch.accept_inorder(dec.seq, dec.flags, chars, usable=usable, state=st, last_isn=self.last_isn)
        out = torch.full((self.cap,), SENT, dtype=torch.uint8, device=self.cuda)
        msg = batch.gather_payloads(self.frames, self.off, H, keep=acc.keep, out=out, check=False)
        for name, t in (("seq", dec.seq), ("ack", dec.ack), ("flags", dec.flags), ("ok", dec.ok), ("csum_out", dec.csum),
                        ("valid", dec.valid), ("usable", usable), ("chars", chars), ("accept", acc.accept),
                        ("keep", acc.keep), ("reply", acc.reply), ("reply_ack", acc.reply_ack),
                        ("payload_off", msg.payload_off)):
            w[name] = t.cpu().numpy().copy()
        w["chars"] = w["chars"].view(np.uint32)
        w["payload_off"] = w["payload_off"].view(np.uint64)
        w["state"] = acc.state.cpu().tolist()
        w["status"] = int(msg.status.item()) | (int(dec.status.item()) & _native.ST_OFFSETS)
        w["total"] = int(w["payload_off"][-1])
        w["payload"] = out.cpu().numpy().copy()  # sentinels from the total on, and everywhere on a capacity miss
        # the replies: a plain host loop over the chain's tables
        idx, peer, last = [], [], n
        for i in range(n):
            if w["usable"][i] and w["flags"][i] & SYN and int(w["seq"][i]) != (self.last_isn if self.last_isn is not None
                                                                                 else batch.NO_ISN):
                last = i
            if w["reply"][i]:
                idx.append(i)
                peer.append(last)
        w["R"], w["reply_index"], w["reply_peer"] = len(idx), np.array(idx, np.uint32), np.array(peer, np.uint64)
        acks = w["reply_ack"][idx].astype(np.uint16)
        R = len(idx)
        w["reply_frames"] = np.zeros(0, np.uint8)
        w["reply_csum"] = np.zeros(0, np.uint16)
        if R:
            fr, cs = batch.pack_batch(batch.HeaderTable(_dev(self.cuda, np.zeros(R, np.uint16)), _dev(self.cuda, acks),
                                                        _dev(self.cuda, np.full(R, batch.ACK, np.uint8))),
                                      torch.zeros((R, 0), dtype=torch.uint8, device=self.cuda), H, want_csum=True)
            w["reply_frames"] = fr.cpu().numpy().reshape(-1).copy()
            w["reply_csum"] = cs.cpu().numpy().copy()
            lit = np.zeros((R, H), np.uint8)  # Packet(seq 0, ack, ACK).to_byte(), byte by byte
            lit[:, 2], lit[:, 3], lit[:, 4] = acks >> 8, acks & 0xFF, 0x40
            s = acks.astype(np.uint32) + 0x4000
            c = (~((s & 0xFFFF) + (s >> 16)) & 0xFFFF).astype(np.uint16)
            if H == 7:
                lit[:, 5], lit[:, 6] = c >> 8, c & 0xFF
            assert np.array_equal(w["reply_frames"], lit.reshape(-1)) and np.array_equal(w["reply_csum"], c)
        w["info"] = acc.info.cpu().tolist()[:5] + [R, w["total"], 0]
        return w

    def call(self, alias=False, with_csum_out=True, with_reply_csum=True):
        """rudp_receive with every output between sentinels; returns the outputs as numpy."""
        import torch
        n, H, cuda = self.n, self.H, self.cuda
        size = dict((name, n) for name, _ in TABLES)
        kinds = dict(TABLES, payload_off="u64", state_out="u64", info="u64", status="u32", payload="u8",
                     reply_frames="u8")
        size.update(payload_off=n + 1, state_out=4, info=8, status=1, payload=self.cap, reply_frames=n * H)
        bufs = {name: torch.full((2 * PAD + size[name] * NP[kinds[name]]().itemsize,), SENT, dtype=torch.uint8,
                                 device=cuda) for name in kinds}
        st_in = torch.tensor([self.state[0], self.state[1], 1 if self.state[2] else 0, 0], dtype=torch.int64).to(cuda)
        ptr = {name: b.data_ptr() + PAD for name, b in bufs.items()}
        if alias:
            ptr["state_out"] = st_in.data_ptr()
        skip = set() if with_csum_out else {"csum_out"}
        skip |= set() if with_reply_csum else {"reply_csum"}
        o = _native.RudpReceived(payload_cap=self.cap, **{
            name: (ptr[name] if (n or name in ("state_out", "info", "status")) and name not in skip
                   and (name != "payload" or self.cap) else None) for name in kinds})
        _native.check(_native.lib().rudp_receive(
            self.frames.data_ptr() if self.nbytes else None, self.nbytes, self.off.data_ptr(),
            self.nbytes // n if n else 0, n, self.csum.data_ptr() if self.csum is not None and n else None,
            batch.NO_ISN if self.last_isn is None else self.last_isn, st_in.data_ptr(), o, H, 0, None))
        got = {}
        for name, b in bufs.items():
            a = b.cpu().numpy()
            assert (a[:PAD] == SENT).all() and (a[len(a) - PAD:] == SENT).all(), name
            got[name] = a[PAD:len(a) - PAD].view(NP[kinds[name]])
        if alias:
            assert (got["state_out"].view(np.uint8) == SENT).all()
            got["state_out"] = st_in.cpu().numpy().view(np.uint64)
        for name in skip:
            assert (got[name].view(np.uint8) == SENT).all(), name
        room = self.room.cpu().numpy()
        assert (room[:16 + self.frames.data_ptr() % 16] == SENT).all()
        assert (room[16 + self.frames.data_ptr() % 16 + self.nbytes:] == SENT).all()
        return got, skip

    def check(self, form="", **kw):
        """One call equals the chain, array by array, and writes nothing else."""
        got, skip = self.call(**kw)
        w, n, H = self.want, self.n, self.H
        tag = (form, n, H)
        sent = lambda a: (a.view(np.uint8) == SENT).all()
        assert got["state_out"].tolist() == w["state"], tag
        assert got["info"].tolist() == w["info"], tag
        assert int(got["status"][0]) == w["status"], tag
        if n == 0:
            assert all(sent(got[k]) for k in got if k not in ("state_out", "info", "status")), tag
            return got
        for name, _ in TABLES[:12]:
            if name not in skip:
                assert np.array_equal(got[name], w[name]), (name,) + tag
        assert np.array_equal(got["payload_off"], w["payload_off"]), tag
        assert np.array_equal(got["payload"], w["payload"]), tag  # the message, and nothing at or past the total
        R = w["R"]
        assert np.array_equal(got["reply_frames"][:R * H], w["reply_frames"]) and sent(got["reply_frames"][R * H:]), tag
        assert np.array_equal(got["reply_index"][:R], w["reply_index"]) and sent(got["reply_index"][R:]), tag
        assert np.array_equal(got["reply_peer"][:R], w["reply_peer"]) and sent(got["reply_peer"][R:]), tag
        if "reply_csum" not in skip:
            assert np.array_equal(got["reply_csum"][:R], w["reply_csum"]) and sent(got["reply_csum"][R:]), tag
        return got

    def check_forms(self, **kw):
        if self.n and self.n <= T and self.nbytes <= FB and self.nbytes <= MEAN * self.n:
            _forms(lambda form: self.check(form, **kw))
        elif self.n and self.n <= T and self.nbytes <= FB:
            # past the mean frame length the product chains; the fused kernel (knob 80 = 2) stays exact
            self.check("chained", **kw)
            tools = _native.tools_lib(activate=True)
            try:
                assert tools.rudpx_tune(80, 2) == 1
                self.check("fused past the mean", **kw)
            finally:
                tools.rudpx_tune(80, 1)
                _native.use_product()
        else:
            self.check("chained", **kw)


# ------------------------------------------------------- the reference's streams
def _expected(c):
    n = len(c["frames"])
    acc = np.array([int(x) for x in c["accepted"]], np.uint8)
    rep = np.array([int(x) for x in c["replied"]], np.uint8)
    return n, acc, rep, np.array(c["ack"], np.uint16)


def test_golden_one_call(cuda):
    """Every stream the reference judged through batch.receive: the message
    recv() returns, the decisions, the replies it put on the wire, the end and
    the state -- in both forms."""
    def run(form):
        for c in golden_cases():
            frames = [bytes.fromhex(h) for h in c["frames"]]
            n, acc, rep, ack = _expected(c)
            buf, off = pack_frames(frames)
            res = batch.receive(_dev(cuda, buf), _dev(cuda, off), "rudp5", state=tuple(c["state"]),
                                last_isn=c["last_isn"])
            a, name = res.accepted, (form, c["name"])
            assert a.accept.cpu().numpy().tolist() == acc.tolist(), name
            assert a.reply.cpu().numpy().tolist() == rep.tolist(), name
            assert a.reply_ack.cpu().numpy().tolist() == ack.tolist(), name
            assert a.end == c["end"] and res.state.cpu().tolist() == c["state_after"] + [0], name
            assert bytes(res.check().message.payload.cpu().numpy()).decode() == c["message"], name
            assert res.message_bytes == len(c["message"].encode()) and len(res) == n, name
            assert a.characters == (len(c["message"]) if c["state_after"][2] else 0), name
            assert a.count == int(acc.sum()) and int(res.status.item()) == 0, name
            # the datagrams send_ack put on the wire, in order
            R = res.reply_count
            sent = b"".join(bytes([0, 0, int(k) >> 8, int(k) & 0xFF, 0x40]) for k in ack[rep == 1])
            assert R == int(rep.sum()) and bytes(res.reply_frames[:5 * R].cpu().numpy()) == sent, name
            assert res.reply_index[:R].cpu().numpy().tolist() == np.flatnonzero(rep).tolist(), name
            if c["clean"]:
                assert a.fast and a.first_anomaly == n, name

    _forms(run)


def _golden_groups():
    groups = {}
    for c in golden_cases():
        key = "scenarios"
        if c["name"].startswith("text"):
            index, key = c["name"][4:].split("_")
            key += f"_{int(index) % 3}" if key == "chunk1" else ""
        groups.setdefault(key, []).append(c)
    return groups


GROUPS = _golden_groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_golden_two_calls(cuda, group):
    """Every stream cut at every datagram boundary into two calls, the state
    carried on the device: the same decisions, replies, end, state and message."""
    import torch

    def run(form):
        for c in GROUPS[group]:
            frames = [bytes.fromhex(h) for h in c["frames"]]
            n, acc, rep, ack = _expected(c)
            buf, off = pack_frames(frames)
            d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
            resets = [i for i in range(n) if acc[i] and frames[i][4] & 0x80]
            sig = _dev(cuda, np.concatenate([acc, rep, ack.view(np.uint8)]))
            st_after = torch.tensor(c["state_after"] + [0], dtype=torch.int64, device=cuda)
            bad = torch.zeros((), dtype=torch.int64, device=cuda)

            def part_bytes(lo, hi):
                start = max([r for r in resets if lo <= r < hi], default=lo)
                return b"".join(frames[i][5:] for i in range(start, hi) if acc[i])

            def differs(res, lo, hi, want):
                a = res.accepted
                got = torch.cat([a.accept, a.reply, a.reply_ack.view(torch.uint8)])
                exp = torch.cat([sig[lo:hi], sig[n + lo:n + hi], sig[2 * n + 2 * lo:2 * n + 2 * hi]])
                d = (got != exp).sum() + (res.info[6] != len(want)) + (res.message.payload_off[-1] != len(want))
                d = d + (res.info[5] != int(rep[lo:min(hi, c["end"] + 1)].sum())) + (res.status != 0).sum()
                if want:
                    w = torch.frombuffer(bytearray(want), dtype=torch.uint8).to(cuda)
                    d = d + (res.message.buffer[:len(want)] != w).sum()
                return d

            for k in range(1, n):
                one = batch.receive(d_buf[:off[k]], d_off[:k + 1], "rudp5", state=tuple(c["state"]),
                                    last_isn=c["last_isn"])
                if c["end"] < k:
                    bad += differs(one, 0, k, part_bytes(0, c["end"] + 1)) + (one.info[0] != c["end"])
                    bad += (one.state != st_after).sum()
                    continue
                two = batch.receive(d_buf[off[k]:], d_off[k:] - int(off[k]), "rudp5", state=one.state,
                                    last_isn=c["last_isn"])
                hi = min(c["end"] + 1, n)
                bad += differs(one, 0, k, part_bytes(0, k)) + differs(two, k, n, part_bytes(k, hi))
                bad += (one.info[0] != k) + (two.info[0] != c["end"] - k) + (two.state != st_after).sum()
                carried = not any(k <= r < hi for r in resets)
                bad += two.info[2] != ((n - k) if carried else max(r for r in resets if r < hi) - k)
            assert int(bad.item()) == 0, (form, c["name"])

    _forms(run)


# ------------------------------------------------------------------- sizes
def _clean_case(cuda, n, H, *, sideband=True, mis=0, widths=(1,), seed=0, state=(0, 0, 0), **kw):
    rng = random.Random(1000 * n + 10 * H + seed)
    buf, off, cs = stream_batch(cuda, rng, clean_stream(rng, n, **kw), H, widths) if n else (
        np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint16))
    return Case(cuda, buf, off, H, csum=cs if H == 5 and sideband else None, state=state, last_isn=6000, mis=mis)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, T - 1, T, T + 1, 3000])
def test_sizes(cuda, n):
    """One-character datagrams a stop-and-wait sender leaves, around every
    workgroup, tile and form boundary; T is the last fused size, T + 1 the first chained."""
    for H in (5, 7):
        for state in ((0, 0, 0), (105, 100, 1)):
            case = _clean_case(cuda, n, H, state=state, fin_at=n - 1 if n > 2 else None,
                               resets=[e for e in (T - 1, T) if e < n])
            if n:
                assert case.want["R"] > 0 or n < 3
            case.check_forms()
    if n == 0:  # the Python entry's empty batch
        import torch
        res = batch.receive(torch.zeros(0, dtype=torch.uint8, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda),
                            "rudp5", state=(105, 100, 1))
        assert res.reply_count == 0 and res.message_bytes == 0 and res.accepted.characters == 5
        assert res.state.cpu().tolist() == [105, 100, 1, 0] and res.message.payload.numel() == 0


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fused_byte_limit(cuda, delta):
    """One-character frames and one padded frame that lands frames_bytes on
    kRecvFusedBytes - 1, the limit itself (the last fused size) and one past it."""
    rng = random.Random(delta)
    n = 600
    seq, flags, chars, usable = clean_stream(rng, n, p_unusable=0.0)
    payloads = [text_of(rng, int(c)) for c in chars]
    pad = FB + delta - (sum(map(len, payloads)) + 5 * n)
    at = next(i for i in range(5, n) if not flags[i] & SYN and seq[i] != seq[i - 1])
    payloads[at] += b"x" * pad  # (its characters no longer match the stream: the frames behind it are refused)
    buf, off, cs = make_batch(cuda, seq, flags, payloads, 5)
    assert len(buf) == FB + delta
    Case(cuda, buf, off, 5, csum=cs).check_forms()


@pytest.mark.parametrize("delta", [0, 1])
def test_fused_mean_frame_limit(cuda, delta):
    """Frames of RECV_FUSED_MEAN bytes on average (the last fused batch) and one
    byte more (the first the product chains): long ASCII frames, each decoded
    and copied by one lane in the fused form, by many in the chained one."""
    rng = random.Random(261 + delta)
    n = 40
    lens = [MEAN - 5 + rng.choice((-100, 100)) for _ in range(n // 2)]
    lens += [2 * (MEAN - 5) - k for k in lens]
    lens[-1] += delta
    seq = (1000 + np.concatenate([[0], np.cumsum(lens[:-1])])).astype(np.uint16)  # one transfer, every frame in order
    flags = np.array([SYN] + [0] * (n - 2) + [FIN], np.uint8)
    payloads = [bytes(rng.randrange(0x20, 0x7F) for _ in range(k)) for k in lens]
    for H in (5, 7):
        buf, off, cs = make_batch(cuda, seq, flags, payloads, H)
        case = Case(cuda, buf, off, H, csum=cs if H == 5 else None, mis=7)
        assert len(buf) == (MEAN - 5 + H) * n + delta and case.want["total"] == sum(lens) and case.want["R"] == n
        case.check_forms()


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("H,sideband", [(7, False), (5, True), (5, False)])
def test_layouts_and_alignments(cuda, H, sideband):
    """rudp7, rudp5 with and without its sideband checksum, d_frames a view at
    byte offsets 1, 5 and 15 of a larger buffer whose guard bytes stay as they were;
    the optional outputs left out."""
    for mis in (0, 1, 5, 15):
        case = _clean_case(cuda, 300, H, sideband=sideband, mis=mis, widths=(1, 2, 3, 4), max_chars=3, seed=mis)
        if not sideband:
            assert set(case.want["ok"]) == ({3} if H == 5 else {0, 1})
        case.check_forms(with_csum_out=mis != 5, with_reply_csum=mis != 15)
        n = case.n
        res = batch.receive(case.frames, case.off, H, csum=case.csum, last_isn=6000)
        assert np.array_equal(res.csum.cpu().numpy(), case.want["csum_out"])
        assert np.array_equal(res.reply_peer[:res.reply_count].cpu().numpy().view(np.uint64), case.want["reply_peer"])
        assert np.array_equal(res.chars.cpu().numpy().view(np.uint32), case.want["chars"])
        assert np.array_equal(res.usable.cpu().numpy(), case.want["usable"]) and len(res) == n


# ------------------------------------------------------------- bad frames
def test_bad_frames_inside_a_fused_batch(cuda):
    """A corrupted checksum, invalid UTF-8 (overlong, surrogate, truncated at the
    frame end), a frame shorter than the header, an empty datagram, a decreasing
    offset pair and an offset past frames_bytes, among in-order frames: the
    call's answer is the chain's, and the rejected frames' bytes were not read
    (poisoning them changes nothing)."""
    for H, sideband in ((5, True), (7, False)):
        rng = random.Random(H)
        n = 64
        seq, flags, chars, usable = clean_stream(rng, n, p_unusable=0.0, p_reset=0.0, p_repeat=0.0)
        payloads = [text_of(rng, int(c), (1, 2, 3, 4)) for c in chars]
        payloads[10] = b"\xc0\xaf"           # overlong '/'
        payloads[11] = b"\xed\xa0\x80"       # a surrogate
        payloads[12] = "€".encode()[:2]      # truncated at the frame end
        buf, off, cs = make_batch(cuda, seq, flags, payloads, H)
        buf[off[20] + 1] ^= 0x40             # a header bit: the checksum no longer matches
        frames = [bytes(buf[off[i]:off[i + 1]]) for i in range(n)]
        frames[30] = frames[30][:3]          # shorter than the header
        frames[31] = b""                     # an empty datagram
        buf, off = pack_frames(frames)
        cs = cs.copy()
        case = Case(cuda, buf, off, H, csum=cs if sideband else None)
        assert case.want["ok"][20] == 0 and case.want["ok"][30] == 2 and case.want["ok"][31] == 2
        assert case.want["valid"][10:13].tolist() == [0, 0, 0] and case.want["status"] == 0
        case.check_forms()
        bad = off.copy()
        bad[41] = off[42] + 1                # frame 40 runs into 41, 41 has a decreasing pair
        bad[50] = len(buf) + 7               # frame 49 ends past the buffer, 50 starts there
        want = None
        for poison in (False, True):
            b2 = buf.copy()
            if poison:  # the bytes no valid frame covers: those of the rejected frames 49 and 50
                b2[off[49]:off[51]] ^= 0xFF
            case = Case(cuda, b2, bad, H, csum=cs if sideband else None)
            assert case.want["status"] == _native.ST_OFFSETS
            assert [int(case.want["ok"][i]) for i in (40, 41, 49, 50)].count(4) >= 3
            got = []
            _forms(lambda form: got.append(case.check(form)))
            for g in got:
                sig = {k: g[k].tobytes() for k in g if k != "payload"} | {"msg": g["payload"][:case.want["total"]].tobytes()}
                want = want or sig
                assert sig == want, poison


def test_mixed_lengths(cuda):
    """1-4-byte characters, several per datagram, and one 1000-byte frame among
    one-character frames (a payload copied by many lanes)."""
    rng = random.Random(4)
    n = 500
    seq, flags, chars, usable = clean_stream(rng, n, max_chars=5, p_reset=0.0, high_isn=0.0)
    payloads = [text_of(rng, int(c), (1, 2, 3, 4)) for c in chars]
    at = next(i for i in range(100, n) if not flags[i] & SYN and seq[i] != seq[i - 1] and usable[i] and usable[i - 1])
    payloads[at] = b"y" * 1000
    seq[at + 1:] += 1000 - int(chars[at])  # the stream goes on behind the long frame
    chars[at] = 1000
    for H in (5, 7):
        buf, off, cs = make_batch(cuda, seq, flags, payloads, H)
        for i in np.flatnonzero(usable == 0):
            buf[off[i + 1] - 1] ^= 0x01
        for mis in (0, 3):
            case = Case(cuda, buf, off, H, csum=cs if H == 5 else None, mis=mis)
            assert case.want["accept"][at] == 1 and case.want["keep"][at + 1:].any() and case.want["total"] > 1500
            case.check_forms()


# ------------------------------------------------------ adversarial streams
def test_adversarial_streams(cuda):
    """Random seq_num, flags and characters: the one-scan form and the
    sequential walk must both have run, and both forms stay exact."""
    paths = {"fast": 0, "slow": 0}
    rng = random.Random(0xADE5)
    for k in range(14):
        n = rng.choice((7, 64, 257, 600, T, T + 1, 2 * T + 5))
        stream = adversarial_stream(rng, n, p_fin=rng.choice((0.0, 0.002, 0.02)))
        buf, off, cs = stream_batch(cuda, rng, stream, 5)
        state = rng.choice(((0, 0, 0), (0, 0, 1), (105, 100, 1), (65536, 65530, 1)))
        case = Case(cuda, buf, off, 5, csum=cs, state=state, last_isn=rng.choice((None, int(stream[0][0]), 3611)))
        case.check_forms(alias=k % 2 == 0)
        paths["fast" if case.want["info"][4] == n else "slow"] += 1
    assert paths["slow"] >= 1, paths  # (the clean streams of the other tests take the one-scan form alone)


def _placed(cuda, rng, n, at, fin_at):
    seq, flags, chars, usable = clean_stream(rng, n, fin_at=fin_at, p_reset=0.0, p_unusable=0.02, high_isn=0.0)
    seq[at], flags[at], usable[at] = (int(seq[at]) + 50) & 0xFFFF, flags[at] & FIN, 1
    buf, off, cs = stream_batch(cuda, rng, (seq, flags, chars, usable), 5)
    return Case(cuda, buf, off, 5, csum=cs)


def _case(cuda, rng, stream, **kw):
    buf, off, cs = stream_batch(cuda, rng, stream, 5)
    return Case(cuda, buf, off, 5, csum=cs, **kw)


def test_placed_streams(cuda):
    """A frame from the future at index 0; an anomaly at a tile edge; two resets
    from different peers; a repeated SYN of last_isn; FIN in the middle; and a
    receiver without a peer before the first SYN."""
    rng = random.Random(80)
    # a live receiver whose first datagram comes from the future
    seq, flags, chars, usable = clean_stream(rng, 200, p_reset=0.0, high_isn=0.0)
    flags[:] &= 0x7F
    usable[0] = 1
    case = _case(cuda, rng, (seq + 40, flags, chars, usable), state=(int(seq[0]), int(seq[0]), 1))
    assert case.want["info"][4] == 0
    case.check_forms()
    # the anomaly on the last frame of a tile, the first of the next, and behind it
    for n, at in ((T, T - 1), (T + 1, T - 1), (T + 1, T), (2 * T + 30, T + 1)):
        case = _placed(cuda, rng, n, at, None)
        assert case.want["info"][4] == at, (n, at)
        case.check_forms()
    # two transfers from "different peers" in one batch: the replies name the reset they follow
    seq, flags, chars, usable = clean_stream(rng, 400, resets=[150], p_reset=0.0, p_unusable=0.0)
    case = _case(cuda, rng, (seq, flags, chars, usable), state=(77, 70, 1))
    assert set(case.want["reply_peer"].tolist()) == {0, 150}
    case.check_forms()
    # the same with the first SYN a repeat of the last transfer's: the live receiver answers it and
    # every frame behind it to its carried peer (n), until the second SYN
    case = _case(cuda, rng, (seq, flags, chars, usable), state=(77, 70, 1), last_isn=int(seq[0]))
    assert set(case.want["reply_peer"].tolist()) == {400, 150} and case.want["reply"][0] == 1
    case.check_forms()
    # FIN in the middle: nothing behind `end`, and no reply frame for it
    for n in (300, T + 200):
        seq, flags, chars, usable = clean_stream(rng, n, fin_at=120, p_reset=0.0)
        case = _case(cuda, rng, (seq, flags, chars, usable))
        assert case.want["info"][0] == 120 and case.want["R"] == int(case.want["reply"][:121].sum()) > 0
        assert not case.want["reply"][121:].any()
        case.check_forms()
    # no peer yet and no SYN: nothing accepted, nothing answered
    seq, flags, chars, usable = clean_stream(rng, 100, p_reset=0.0)
    flags[:] &= 0x7F
    case = _case(cuda, rng, (seq, flags, chars, usable))
    assert case.want["R"] == 0 and case.want["total"] == 0 and not case.want["accept"].any()
    case.check_forms()


# ------------------------------------------------- capacity, aliasing, bounds
@pytest.mark.parametrize("n", [400, T + 300])
def test_payload_capacity_and_aliasing(cuda, n):
    """payload_cap one byte short: the status bit, no payload byte written,
    payload_off[n] the size needed and everything else as ever; exactly enough:
    the message.  state_out aliasing state_in."""
    rng = random.Random(n)
    buf, off, cs = stream_batch(cuda, rng, clean_stream(rng, n, max_chars=3), 7, (1, 2, 3, 4))
    total = Case(cuda, buf, off, 7).want["total"]
    assert total > 300
    short = Case(cuda, buf, off, 7, cap=total - 1, state=(9, 2, 1))
    assert short.want["status"] == _native.ST_PAYLOAD_CAP and short.want["total"] == total
    assert (short.want["payload"] == SENT).all() and short.want["R"] > 0
    short.check_forms()
    exact = Case(cuda, buf, off, 7, cap=total, state=(9, 2, 1))
    assert exact.want["status"] == 0
    exact.check_forms(alias=True)


# ------------------------------------------------------------ stream capture
def _capture(cuda, n):
    import torch
    rng = random.Random(n)
    inputs = []
    for k in range(2):  # two inputs of one shape: one-character payloads, the same streams' lengths
        stream = clean_stream(random.Random(n), n, p_unusable=0.0)
        seq = ((stream[0].astype(np.uint32) + 11 * k) & 0xFFFF).astype(np.uint16)
        buf, off, cs = stream_batch(cuda, rng, (seq,) + stream[1:], 5)
        inputs.append((buf, off, cs, Case(cuda, buf, off, 5, csum=cs).want))
    assert inputs[0][0].shape == inputs[1][0].shape and not np.array_equal(inputs[0][0], inputs[1][0])
    d_buf, d_off, d_cs = (_dev(cuda, a) for a in inputs[0][:3])
    state = torch.zeros(4, dtype=torch.int64, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        batch.receive(d_buf, d_off, "rudp5", csum=d_cs, state=state)  # (warm: the stream's scratch set)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap = batch.receive(d_buf, d_off, "rudp5", csum=d_cs, state=state)
    for buf, off, cs, want in (inputs[1], inputs[0]):
        d_buf.copy_(_dev(cuda, buf))
        d_cs.copy_(_dev(cuda, cs))
        g.replay()
        torch.cuda.synchronize()
        R = want["R"]
        assert np.array_equal(cap.accepted.accept.cpu().numpy(), want["accept"])
        assert np.array_equal(cap.accepted.reply_ack.cpu().numpy(), want["reply_ack"])
        assert cap.info.cpu().tolist() == want["info"] and cap.state.cpu().tolist() == want["state"]
        assert np.array_equal(cap.reply_frames[:5 * R].cpu().numpy(), want["reply_frames"])
        assert np.array_equal(cap.message.buffer[:want["total"]].cpu().numpy(), want["payload"][:want["total"]])
        assert np.array_equal(cap.reply_peer[:R].cpu().numpy().view(np.uint64), want["reply_peer"])


def test_capture_fused(cuda):
    """One capture of the one-launch form (n = 300), replayed on changed input."""
    _capture(cuda, 300)


def test_capture_chained(cuda):
    """One capture of the chained form (n = 3000, three tiles), replayed on changed input."""
    _capture(cuda, 3000)
