"""rudp_receive_window / batch.receive_windowed on the device.  Every output of
the one call must equal, byte for byte, the CPU reference (receive_window_ref:
the per-source offset rule, the oracle decode, chars_ref, the window's rule as
window.hip states it, ordered_ref twice, the reply frames) and the existing
chain (batch.receive_window: the decode, accept_window and gather_ordered one
after another), and nothing else may be written: every output lies between
sentinels.  Every case runs in both forms (knob 82 of the diagnostics build
turns the fused kernel off)."""
import random

import numpy as np
import pytest

from accept_ref import golden_cases, pack_frames
from oracle import codec_np
from receive_window_ref import ST_CARRY_CAP, receive_window_ref
from rudp import _native, batch
from window_ref import (FIN, NONE, ST_OFFSETS, ST_PAYLOAD_CAP, SYN, adversarial_window_stream, chunk_model,
                        window_ref, window_stream)

pytestmark = pytest.mark.gpu

FB = batch.WINDOW_FUSED_BYTES
MEAN = batch.WINDOW_FUSED_MEAN
GEOMETRY = {1: (1, 1), 2: (2, 1), 8: (4, 2), 64: (64, 1), 1024: (128, 8)}  # tests/test_gpu_window.py's
PAD = 32      # sentinel bytes on either side of every output
SENT = 0xA5
NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
PER_ITEM = (("seq", "u16"), ("ack", "u16"), ("flags", "u8"), ("ok", "u8"), ("csum_out", "u16"), ("valid", "u8"),
            ("usable", "u8"), ("chars", "u32"), ("accept", "u8"), ("rank", "u32"), ("carry_rank", "u32"),
            ("reply", "u8"), ("reply_ack", "u16"))
CHARS = ("a", "é", "€", "😀")  # 1, 2, 3 and 4 bytes


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _forms(fn):
    """fn('fused') with the product library, then fn('chained') with the fused
    form turned off in the diagnostics build."""
    fn("fused")
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(82, 0) == 1
        fn("chained")
    finally:
        tools.rudpx_tune(82, 1)
        _native.use_product()


def _past_the_mean(fn):
    """fn with the fused kernel taken whatever the mean frame length (knob 82 = 2)."""
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(82, 2) == 1
        fn("fused past the mean")
    finally:
        tools.rudpx_tune(82, 1)
        _native.use_product()


def text_of(rng, chars, widths=(1,)):
    return "".join(CHARS[rng.choice(widths) - 1] for _ in range(chars)).encode()


def frames_of(rng, seq, flags, chars, usable, H, widths=(1,)):
    """The stream as frames of the oracle's encode: (u8 buffer, int64 offsets,
    u16 checksums); an unusable frame gets a flipped bit after its checksum was
    taken, so it fails to verify (layout 7, or layout 5 with its sideband)."""
    n = len(seq)
    buf, off, cs = codec_np.encode_varlen(seq, np.zeros(n, np.uint16), flags,
                                          [text_of(rng, int(c), widths) for c in chars], H)
    buf = buf.copy()
    for i in np.flatnonzero(np.asarray(usable) == 0):
        buf[int(off[i])] ^= 0x01  # (a seq bit: the characters stay what the stream says)
    return buf, off, cs


def split(buf, off, cs, k):
    """Frames [0, k) and [k, n) as two buffers with their own offsets."""
    a = int(off[k])
    return (buf[:a], off[:k + 1].copy(), cs[:k]), (buf[a:], off[k:] - a, cs[k:])


class Case:
    """One input on the device: the carried frames and the new ones, each a
    view `mis` bytes into an allocation with sentinels around it."""

    def __init__(self, cuda, carried, new, H, Wc, *, side=False, state=(0, 0, 0), last_isn=None, mis=(0, 0),
                 omis=(0, 0), caps=None):
        import torch
        self.cuda, self.H, self.Wc, self.side, self.state, self.last_isn = cuda, H, Wc, side, state, last_isn
        self.np = [tuple(np.asarray(x) for x in carried), tuple(np.asarray(x) for x in new)]
        self.count = [len(self.np[0][1]) - 1, len(self.np[1][1]) - 1]
        self.n = sum(self.count)
        self.nbytes = [len(self.np[0][0]), len(self.np[1][0])]
        self.mis, self.omis = mis, omis
        self.room, self.buf, self.off, self.cs = [], [], [], []
        for s in range(2):
            b, o, c = self.np[s]
            room = torch.full((len(b) + 64,), SENT, dtype=torch.uint8, device=cuda)
            view = room[16 + mis[s]:16 + mis[s] + len(b)]
            assert view.data_ptr() % 16 == mis[s]
            view.copy_(_dev(cuda, b.astype(np.uint8)))
            self.room.append(room)
            self.buf.append(view)
            self.off.append(_dev(cuda, o.astype(np.int64)))
            self.cs.append(_dev(cuda, c.astype(np.uint16)) if side else None)
        total = sum(self.nbytes)
        self.caps = (total, total) if caps is None else caps
        self._owner = None  # the carried frames as an earlier result's `carried` (windowed())

    def ref(self, rule=chunk_model):
        c, f = self.np
        return receive_window_ref(c[0], c[1], f[0], f[1], self.H, window_chars=self.Wc,
                                  carried_csum=c[2] if self.side else None, csum=f[2] if self.side else None,
                                  state=self.state, last_isn=self.last_isn, payload_cap=self.caps[0],
                                  carry_cap=self.caps[1], rule=rule)

    def call(self, alias=False, optional=True):
        """rudp_receive_window with every output between sentinels; the outputs as numpy."""
        import torch
        n, H, cuda = self.n, self.H, self.cuda
        nc, nn = self.count
        kinds = dict(PER_ITEM, payload_off="u64", payload_src="u32", carry_off="u64", carry_csum="u16",
                     reply_csum="u16", reply_index="u32", reply_peer="u64", state_out="u64", info="u64", status="u32",
                     payload="u8", carry_frames="u8", reply_frames="u8")
        size = dict((name, n) for name, _ in PER_ITEM)
        size.update(payload_off=n + 1, payload_src=n, carry_off=1024, carry_csum=1023, reply_csum=nn, reply_index=nn,
                    reply_peer=nn, state_out=4, info=12, status=1, payload=self.caps[0], carry_frames=self.caps[1],
                    reply_frames=nn * H)
        shift = {"payload": self.omis[0], "carry_frames": self.omis[1]}
        bufs = {name: torch.full((2 * PAD + size[name] * NP[kinds[name]]().itemsize + shift.get(name, 0),), SENT,
                                 dtype=torch.uint8, device=cuda) for name in kinds}
        st_in = torch.tensor([self.state[0], self.state[1], 1 if self.state[2] else 0, 0], dtype=torch.int64).to(cuda)
        ptr = {name: b.data_ptr() + PAD + shift.get(name, 0) for name, b in bufs.items()}
        assert all(ptr[k] % 16 == v for k, v in shift.items())
        if alias:
            ptr["state_out"] = st_in.data_ptr()
        skip = set() if optional else {"csum_out", "payload_src", "carry_csum", "reply_csum"}
        always = ("state_out", "info", "status", "carry_off")
        o = _native.RudpReceivedWindow(payload_cap=self.caps[0], carry_cap=self.caps[1], **{
            name: (ptr[name] if (n or name in always) and name not in skip
                   and (name != "payload" or self.caps[0]) and (name != "carry_frames" or self.caps[1]) else None)
            for name in kinds})
        side = self.side and n
        cs_new = self.cs[1] if nn else self.cs[0]  # (no new frames: any non-NULL pointer says "sidebands")
        total = sum(self.nbytes)
        _native.check(_native.lib().rudp_receive_window(
            self.buf[0].data_ptr() if self.nbytes[0] else None, self.nbytes[0], self.off[0].data_ptr() if nc else None,
            self.cs[0].data_ptr() if side and nc else None, nc,
            self.buf[1].data_ptr() if self.nbytes[1] else None, self.nbytes[1], self.off[1].data_ptr(),
            cs_new.data_ptr() if side else None, nn, total // n if n else 0,
            batch.NO_ISN if self.last_isn is None else self.last_isn, self.Wc, st_in.data_ptr(), o, H, 0, None))
        got = {}
        for name, b in bufs.items():
            a = b.cpu().numpy()
            lo = PAD + shift.get(name, 0)
            assert (a[:lo] == SENT).all() and (a[len(a) - PAD:] == SENT).all(), name
            got[name] = a[lo:len(a) - PAD].view(NP[kinds[name]])
        if alias:
            assert (got["state_out"].view(np.uint8) == SENT).all()
            got["state_out"] = st_in.cpu().numpy().view(np.uint64)
        for name in skip:
            assert (got[name].view(np.uint8) == SENT).all(), name
        for s in range(2):  # the inputs and their surroundings are as they were
            room = self.room[s].cpu().numpy()
            assert (room[:16 + self.mis[s]] == SENT).all() and (room[16 + self.mis[s] + self.nbytes[s]:] == SENT).all()
        return got, skip

    def check(self, form="", want=None, **kw):
        """One call equals the reference, array by array, and writes nothing else."""
        got, skip = self.call(**kw)
        w = self.ref() if want is None else want
        n, H = self.n, self.H
        tag = (form, self.count, H, self.Wc, self.side)
        sent = lambda a: (a.view(np.uint8) == SENT).all()

        def head(name, k, ref):  # the first k entries are the reference's, the rest untouched
            if name in skip:
                return
            assert np.array_equal(got[name][:k], ref), (name,) + tag
            assert sent(got[name][k:]), (name,) + tag
        assert got["state_out"].tolist() == w["state"], tag
        assert got["info"].tolist() == w["info"], tag
        assert int(got["status"][0]) == w["status"], tag
        if n == 0:
            assert got["carry_off"][0] == 0 and sent(got["carry_off"][1:]), tag
            assert all(sent(got[k]) for k in got if k not in ("state_out", "info", "status", "carry_off")), tag
            return got
        for name, _ in PER_ITEM:
            if name not in skip:
                assert np.array_equal(got[name], w[name]), (name,) + tag
        K, P, R = w["K"], w["P"], w["R"]
        head("payload_off", K + 1, w["payload_off"])
        head("payload_src", K, w["payload_src"])
        head("payload", len(w["payload"]), w["payload"])  # nothing on a capacity miss
        head("carry_off", P + 1, w["carry_off"])
        head("carry_frames", len(w["carry_frames"]), w["carry_frames"])
        if w["carry_csum"] is None:
            assert sent(got["carry_csum"]), tag
        else:
            head("carry_csum", P, w["carry_csum"])
        head("reply_frames", R * H, w["reply_frames"])
        head("reply_csum", R, w["reply_csum"])
        head("reply_index", R, w["reply_index"])
        head("reply_peer", R, w["reply_peer"])
        return got

    def check_forms(self, **kw):
        want = self.ref()
        _forms(lambda form: self.check(form, want, **kw))
        return want

    def check_chain(self):
        """batch.receive_windowed against batch.receive_window (valid offsets)."""
        import torch
        nc, nn = self.count
        car = None
        if nc:
            ordered = batch.OrderedPayloads(self.buf[0], self.off[0], torch.arange(nc, dtype=torch.int32,
                                                                                   device=self.cuda), None, None)
            ordered._total = (nc, self.nbytes[0])
            car = batch.CarriedFrames(ordered, self.cs[0])
        kw = dict(window_chars=self.Wc, csum=self.cs[1], state=self.state, last_isn=self.last_isn)
        want = batch.receive_window(self.buf[1], self.off[1], self.H, carried=car, **kw)

        def one(form):
            got = self.windowed(**kw)
            tag = (form, self.count, self.H, self.Wc)
            a, b = got.accepted, want.accepted
            for name in ("accept", "rank", "carry_rank", "reply", "state"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (name,) + tag
            assert torch.equal(a.reply_ack.view(torch.uint8), b.reply_ack.view(torch.uint8)), tag
            assert a.info.tolist() == b.info.tolist() == got.info.tolist()[:8], tag
            assert got.check().message.total == want.message.check().total, tag
            assert torch.equal(got.message.payload, want.message.payload), tag
            K = got.message.total[0]
            assert torch.equal(got.message.out_off[:K + 1], want.message.out_off[:K + 1]), tag
            assert (got.carried.count, got.carried.nbytes) == (want.carried.count, want.carried.nbytes), tag
            P, nb = got.carried.count, got.carried.nbytes
            assert torch.equal(got.carried.frames[:nb], want.carried.frames), tag
            assert torch.equal(got.carried.frame_off[:P + 1], want.carried.frame_off), tag
            if self.side and P:
                assert torch.equal(got.carried.csum[:P].view(torch.uint8), want.carried.csum.view(torch.uint8)), tag
            assert got.reply_count == want.reply_count, tag
            assert got.reply_index.tolist() == want.reply_index.tolist(), tag
            assert got.reply_peer.tolist() == want.reply_peer.tolist(), tag
            assert got.reply_ack.cpu().numpy().tolist() == want.reply_ack.cpu().numpy().tolist(), tag
            assert torch.equal(got.reply_frames, want.reply_frames(self.H)), tag
        _forms(one)

    def windowed(self, **kw):
        """batch.receive_windowed, the carried frames handed over as a result's ``carried``."""
        import torch
        nc = self.count[0]
        car = self._owner.carried if self._owner is not None else None
        if nc and car is None:
            lay = batch.ReceivedWindowed.layout(0, 0, self.H, 0, self.nbytes[0])
            owner = batch.ReceivedWindowed(torch.zeros(lay["size"], dtype=torch.uint8, device=self.cuda), 0, 0, self.H,
                                           0, self.nbytes[0], self.side)
            owner.carried.frames.copy_(self.buf[0])
            owner.carried.frame_off[:nc + 1].copy_(self.off[0])
            if self.side:
                owner._cut("carry_csum", 2 * 1023, torch.uint16)[:nc].view(torch.int16).copy_(
                    self.cs[0].view(torch.int16))
            owner._info = [0, 0, 0, 0, 0, nc, 0, 0, 0, 0, self.nbytes[0], 0]
            self._owner, car = owner, owner.carried
        return batch.receive_windowed(self.buf[1], self.off[1], self.H, carried=car, **kw)


def crafted(cuda, rng, nc, nn, Wc, H, side, **kw):
    """nc pending frames of one character at distinct starts inside the window
    behind a windowed sender's stream of nn frames of a live transfer."""
    W, C = GEOMETRY[Wc]
    isn = rng.randint(1, 3000)
    seq, flags, chars, usable, state = window_stream(rng, nn, W, C, syn=False, isn=isn, p_unusable=0.03)
    starts = rng.sample(range(1, Wc), nc) if nc else []
    cseq = np.array([(state[0] + s) & 0xFFFF for s in sorted(starts)], np.uint16)
    carried = frames_of(rng, cseq, np.zeros(nc, np.uint8), np.ones(nc, np.uint32), np.ones(nc, np.uint8), H)
    new = frames_of(rng, seq, flags, chars, usable, H)
    return Case(cuda, carried, new, H, Wc, side=side, state=state, **kw)


# ------------------------------------------------------------- sizes and shapes
VARIANTS = {"rudp7": (7, False), "rudp5_sideband": (5, True), "rudp5_unverified": (5, False)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("Wc", sorted(GEOMETRY))
def test_sizes_and_shapes(cuda, Wc, variant):
    H, side = VARIANTS[variant]
    rng = random.Random(0x5A5E + 7 * Wc + H + side)
    for nn in (0, 1, 2, 7, 64, 255, 1023, 1024, 1025):
        for nc in sorted({0, min(1, Wc - 1), Wc - 1}):
            case = crafted(cuda, rng, nc, nn, Wc, H, side)
            want = case.check_forms(alias=(nn + nc) % 2 == 1, optional=nn % 3 != 1)
            if nn == 0:  # the carried frames alone: all stay pending, no reply
                assert want["P"] == nc and want["R"] == 0 and want["K"] == 0
            if nn in (7, 1025):
                case.check_chain()


def test_empty_call(cuda):
    case = Case(cuda, (np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint16)),
                (np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint16)), 5, 8, state=(120, 100, 1))
    want = case.check_forms()
    assert want["info"] == [0, 0, 0, 20] + [0] * 8 and want["state"] == [120, 100, 1, 0]


# ----------------------------------------------------------------------- limits
def sized(cuda, rng, nc, nn, total, H=7, Wc=8):
    """A live transfer's frames, nc of them carried, in exactly `total` bytes."""
    n = nc + nn
    per, extra = divmod(total - n * H, n)
    chars = np.array([per + (1 if i < extra else 0) for i in range(n)], np.uint32)
    isn = 500
    seq = np.zeros(n, np.uint16)
    at = isn + 1
    order = list(range(nc, n)) + list(range(nc))  # the carried ones lie ahead of the new ones
    for i in order:
        seq[i] = at & 0xFFFF
        at += int(chars[i])
    buf, off, cs = frames_of(rng, seq, np.zeros(n, np.uint8), chars, np.ones(n, np.uint8), H)
    assert len(buf) == total
    carried, new = split(buf, off, cs, nc)
    return Case(cuda, carried, new, H, Wc, state=(isn + 1, isn, 1))


def test_the_byte_limit(cuda):
    rng = random.Random(0xB17E)
    for total in (FB - 1, FB, FB + 1):
        sized(cuda, rng, 3, 200, total).check_forms()


def test_the_mean_frame_limit(cuda):
    rng = random.Random(0x3EA4)
    for nc, nn in ((0, 20), (3, 17)):
        for total in (MEAN * 20 - 1, MEAN * 20, MEAN * 20 + 1):
            case = sized(cuda, rng, nc, nn, total)
            want = case.check_forms()
            _past_the_mean(lambda form: case.check(form, want))


# -------------------------------------------------------------------- alignment
def taken_and_left(rng, H, widths=(1, 2, 3, 4)):
    """A windowed sender's stream between the first and the last cut that leave
    frames pending: a call that takes carried frames and leaves some.  Returns
    the carried and the new frames, the state and the new frames' count."""
    W, C = GEOMETRY[8]
    seq, flags, chars, usable, state = window_stream(rng, 60, W, C, p_loss=0.1, p_swap=0.2)
    cuts = [k for k in range(10, 60)
            if (window_ref(seq[:k], flags[:k], chars[:k], usable[:k], state, window_chars=8).accept == 2).any()]
    k, e = cuts[0], cuts[-1]
    r1 = window_ref(seq[:k], flags[:k], chars[:k], usable[:k], state, window_chars=8)
    pend = np.flatnonzero(r1.accept == 2)
    idx = np.concatenate([pend, np.arange(k, e)])
    buf, off, cs = frames_of(rng, seq[idx], flags[idx], chars[idx], usable[idx], H, widths)
    carried, new = split(buf, off, cs, len(pend))
    return carried, new, (r1.state[0], r1.state[1], 1), e - k


def test_input_and_output_alignment(cuda):
    rng = random.Random(0xA119)
    carried, new, st, nn = taken_and_left(rng, 7)
    want = None
    for a in (0, 1, 7, 15):
        for b in (0, 1, 7, 15):
            for kw in ({"mis": (a, b)}, {"omis": (a, b)}):
                case = Case(cuda, carried, new, 7, 8, state=st, **kw)
                want = case.ref() if want is None else want
                _forms(lambda form: case.check(form, want))
    assert want["K"] >= 8 and want["P"] >= 1 and want["R"] == nn


# ---------------------------------------------------------------------- streams
def carried_case(cuda, rng, stream, state, k, Wc, H, side=False, widths=(1,), last_isn=None):
    """Frames [0, k) judged by the rule; what it leaves pending and frames [k, n)
    as the call's input.  Returns the case and the rule's state of call one."""
    seq, flags, chars, usable = stream
    r1 = window_ref(seq[:k], flags[:k], chars[:k], usable[:k], state, last_isn, window_chars=Wc)
    pend = np.flatnonzero(r1.accept == 2) if r1.info[0] == k else np.zeros(0, np.int64)
    idx = np.concatenate([pend, np.arange(k, len(seq))]).astype(np.int64)
    buf, off, cs = frames_of(rng, seq[idx], flags[idx], chars[idx], usable[idx], H, widths)
    carried, new = split(buf, off, cs, len(pend))
    return Case(cuda, carried, new, H, Wc, side=side, state=r1.state, last_isn=last_isn)


@pytest.mark.parametrize("Wc", sorted(GEOMETRY))
def test_windowed_sender_streams_never_walk(cuda, Wc):
    rng = random.Random(0x57E4 + Wc)
    W, C = GEOMETRY[Wc]
    for n, k in ((300, 100), (1500, 700), (2000, 990)):
        seq, flags, chars, usable, state = window_stream(rng, n, W, C, p_loss=0.08, p_swap=0.1, p_unusable=0.02)
        case = carried_case(cuda, rng, (seq, flags, chars, usable), state, k, Wc, 5, side=True)
        want = case.check_forms()
        assert want["info"][4] == case.n, (Wc, n)  # the parallel form alone
        assert want["info"] == case.ref(rule=window_ref)["info"]
    case.check_chain()


@pytest.mark.parametrize("Wc", sorted(GEOMETRY))
def test_adversarial_streams(cuda, Wc):
    rng = random.Random(0xAD7E + Wc)
    walked = 0
    for n, k in ((40, 20), (700, 300), (1400, 380)):
        seq, flags, chars, usable = adversarial_window_stream(rng, n, Wc)
        state = (int(seq[0]), max(int(seq[0]) - 3, 0), 1)
        case = carried_case(cuda, rng, (seq, flags, chars, usable), state, k, Wc, 7, widths=(1, 2, 3, 4), last_isn=100)
        want = case.check_forms()
        rule = case.ref(rule=window_ref)
        assert want["info"][:4] + want["info"][5:] == rule["info"][:4] + rule["info"][5:]
        walked += want["info"][4] < case.n
    assert walked
    case.check_chain()


def test_placed_events(cuda):
    """One frame beyond the window (the walk), a reset with frames pending, a
    FIN delivered from the pending set, characters of 1 to 4 bytes, invalid
    UTF-8, wrong checksums and short frames, each placed into a windowed
    sender's stream with frames carried."""
    rng = random.Random(0x91AC)
    Wc = 8
    W, C = GEOMETRY[Wc]
    for event in ("beyond", "reset", "fin_from_pending", "invalid_utf8", "wrong_checksum", "short"):
        for H, side in ((7, False), (5, True)):
            seq, flags, chars, usable, state = window_stream(rng, 120, W, C, p_loss=0.1, p_swap=0.2)
            seq, flags, chars, usable = seq.copy(), flags.copy(), chars.copy(), usable.copy()
            r1 = window_ref(seq[:50], flags[:50], chars[:50], usable[:50], state, window_chars=Wc)
            pend = np.flatnonzero(r1.accept == 2)
            E = r1.state[0]
            if event == "beyond":
                seq[70] = (int(seq[70]) + 5 * Wc) & 0xFFFF
            elif event == "reset":
                flags[60], seq[60] = SYN, 9000
                for j in range(61, 120):
                    seq[j] = (9000 + (int(seq[j]) - int(seq[61]) + C)) & 0xFFFF
            elif event == "fin_from_pending":
                # expect + C with FIN arrives first and waits (or is pending already); the frame at expect delivers both
                seq[50], seq[51], flags[51] = (E + C) & 0xFFFF, E & 0xFFFF, 0
                flags[seq == ((E + C) & 0xFFFF)] |= FIN
            idx = np.concatenate([pend, np.arange(50, 120)]).astype(np.int64)
            buf, off, cs = frames_of(rng, seq[idx], flags[idx], chars[idx], usable[idx], H, widths=(1, 2, 3, 4))
            buf, off = buf.copy(), off.copy()
            m = len(pend)
            if event == "invalid_utf8":
                for j in (m + 3, m + 30):
                    buf[int(off[j + 1]) - 1] = 0xC3  # a lead byte with nothing behind it
                    cs[j] = codec_np.decode_varlen(buf[off[j]:off[j + 1]], np.array([0, off[j + 1] - off[j]]), H)[4][0]
                    if H == 7:
                        buf[int(off[j]) + 5], buf[int(off[j]) + 6] = cs[j] >> 8, cs[j] & 0xFF
            elif event == "wrong_checksum":
                for j in ([0] if m else []) + [m + 4, m + 40]:
                    buf[int(off[j + 1]) - 1] ^= 0x20
            elif event == "short":
                cut = [m + 5, m + 6, m + 44]
                keep = np.ones(len(buf), bool)
                for j, left in zip(cut, (0, 3, H - 1)):
                    keep[int(off[j]) + left:int(off[j + 1])] = False
                lens = np.diff(off)
                for j, left in zip(cut, (0, 3, H - 1)):
                    lens[j] = left
                buf = buf[keep]
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            carried, new = split(buf, off, cs, m)
            case = Case(cuda, carried, new, H, Wc, side=side, state=r1.state)
            want = case.check_forms()
            if event == "beyond":
                assert want["info"][4] < case.n
            elif event == "reset":
                assert want["info"][2] == m + 10 and (want["reply_peer"][-1] == m + 10)
            elif event == "fin_from_pending":
                assert want["info"][0] == m + 1 and want["accept"][m + 1] == 1 and want["K"] >= 2
            elif event == "invalid_utf8":
                assert want["valid"][m + 3] == 0 and want["ok"][m + 3] == 1 and not want["usable"][m + 3]
            elif event == "wrong_checksum":
                assert want["ok"][m + 4] == 0 and want["ok"][m + 40] == 0
            elif event == "short":
                assert [want["ok"][j] for j in cut] == [2, 2, 2]


# ------------------------------------------------------------- rejected offsets
def test_rejected_offsets_at_each_placement(cuda):
    """A frame whose offsets fail its own source's rule, in the interior of the
    carried frames, as the last carried one, as the first and as the last new
    one: the frame past the buffer's end is not read (the allocation ends in
    sentinels the call leaves alone), every other frame is judged."""
    rng = random.Random(0x0FF5)
    W, C = GEOMETRY[8]
    seq, flags, chars, usable, state = window_stream(rng, 80, W, C, p_loss=0.2, p_swap=0.3)
    # the first cut that leaves three frames pending, and the twenty frames behind it
    k = next(k for k in range(10, 60)
             if (window_ref(seq[:k], flags[:k], chars[:k], usable[:k], state, window_chars=8).accept == 2).sum() >= 3)
    r1 = window_ref(seq[:k], flags[:k], chars[:k], usable[:k], state, window_chars=8)
    pend = np.flatnonzero(r1.accept == 2)
    idx = np.concatenate([pend, np.arange(k, k + 20)]).astype(np.int64)
    m = len(pend)
    for H, side in ((7, False), (5, True)):
        buf, off, cs = frames_of(rng, seq[idx], flags[idx], chars[idx], usable[idx], H)
        for which, j in (("carried", 1), ("carried", m - 1), ("new", 0), ("new", 19)):
            carried, new = split(buf, off, cs, m)
            o = (carried if which == "carried" else new)[1]
            nbytes = len((carried if which == "carried" else new)[0])
            if j + 1 == len(o) - 1:
                o[j + 1] = nbytes + 9          # the last frame ends past the buffer
                bad = [j]
            else:
                o[j + 1] = nbytes + 40         # an interior end past the buffer: the next frame starts there too
                bad = [j, j + 1]
            case = Case(cuda, carried, new, H, 8, side=side, state=r1.state)
            want = case.check_forms()
            base = 0 if which == "carried" else m
            assert np.flatnonzero(want["ok"] == 4).tolist() == [base + b for b in bad], (which, j)
            assert want["status"] & ST_OFFSETS and want["K"] > 0


# ------------------------------------------------------------ carry across calls
def message_of(frames, res):
    order = np.argsort(res.rank[res.rank != NONE])
    return b"".join(frames[i][5:] for i in np.flatnonzero(res.rank != NONE)[order])


def plain_frames(rng, seq, flags, chars):
    alphabet = "az09 éß€世\U0001F600\U00010348"
    return [int(s).to_bytes(2, "big") + b"\x00\x00" + bytes([f]) + "".join(rng.choice(alphabet) for _ in range(c)).encode()
            for s, f, c in zip(seq.tolist(), flags.tolist(), chars.tolist())]


def test_two_call_carry_at_every_cut(cuda):
    """Call two takes call one's carry buffers and info as they are."""
    rng = random.Random(0xCA44)
    seq, flags, chars, usable, state = window_stream(rng, 40, 8, 1, p_loss=0.1, p_swap=0.2, total=30)
    frames = plain_frames(rng, seq, flags, chars)
    whole = window_ref(seq, flags, chars, None, state, window_chars=8)
    buf, off = pack_frames(frames)
    d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
    n = len(frames)

    def cuts(form):
        for k in range(1, n):
            one = batch.receive_windowed(d_buf[:off[k]], d_off[:k + 1], "rudp5", window_chars=8, state=state)
            r1 = window_ref(seq[:k], flags[:k], chars[:k], None, state, window_chars=8)
            assert bytes(one.check().message.payload.cpu().numpy()) == message_of(frames[:k], r1), (form, k)
            if r1.info[0] < k:  # the transfer ended in the first call
                continue
            pend = np.flatnonzero(r1.accept == 2)
            assert one.carried.count == len(pend), (form, k)
            two = batch.receive_windowed(d_buf[off[k]:], d_off[k:] - int(off[k]), "rudp5", window_chars=8,
                                         carried=one.carried, state=one.state)
            idx = np.concatenate([pend, np.arange(k, n)]).astype(np.int64)
            r2 = window_ref(seq[idx], flags[idx], chars[idx], None, r1.state, window_chars=8, n_carried=len(pend))
            m = len(pend)
            part2 = bytes(two.check().message.payload.cpu().numpy())
            assert part2 == message_of([frames[i] for i in idx], r2), (form, k)
            joined = part2 if r2.info[2] < len(idx) else bytes(one.message.payload.cpu().numpy()) + part2
            assert joined == message_of(frames, whole), (form, k)
            assert two.state.tolist() == [whole.state[0], whole.state[1], whole.state[2], 0], (form, k)
            assert two.reply_index.tolist() == np.flatnonzero(r2.reply[m:]).tolist(), (form, k)
            assert two.reply_ack.cpu().numpy().tolist() == r2.reply_ack[m:][r2.reply[m:] == 1].tolist(), (form, k)
            assert two.carried.count == whole.info[5], (form, k)
    _forms(cuts)


def test_three_calls_ping_pong_two_buffer_sets(cuda):
    rng = random.Random(0xCA46)
    seq, flags, chars, usable, state = window_stream(rng, 90, 8, 1, p_loss=0.15, p_swap=0.3)
    frames = plain_frames(rng, seq, flags, chars)
    whole = window_ref(seq, flags, chars, None, state, window_chars=8)
    buf, off = pack_frames(frames)
    d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)

    def three(form):
        parts, st, car, sets = [], state, None, [None, None]
        for c, (a, b) in enumerate(((0, 30), (30, 60), (60, 90))):
            res = batch.receive_windowed(d_buf[off[a]:off[b]], d_off[a:b + 1] - int(off[a]), "rudp5", window_chars=8,
                                         carried=car, state=st, out=sets[c % 2])
            sets[c % 2] = res
            parts.append(bytes(res.check().message.payload.cpu().numpy()))  # (read before the set is written again)
            st, car = res.state, res.carried
        assert sets[0]._buf.data_ptr() != sets[1]._buf.data_ptr()
        assert b"".join(parts) == message_of(frames, whole), form
        assert res.carried.count == whole.info[5] and res.state.tolist()[:3] == list(whole.state), form
    _forms(three)


# ------------------------------------------------------- capacity and aliasing
def test_capacity_one_byte_short(cuda):
    rng = random.Random(0xCA9A)
    carried, new, st, _ = taken_and_left(rng, 7)
    full = Case(cuda, carried, new, 7, 8, state=st).ref()
    mbytes, cbytes = full["info"][9], full["info"][10]
    assert mbytes > 1 and cbytes > 1
    for caps, bits in (((mbytes - 1, cbytes), ST_PAYLOAD_CAP), ((mbytes, cbytes - 1), ST_CARRY_CAP),
                       ((mbytes - 1, cbytes - 1), ST_PAYLOAD_CAP | ST_CARRY_CAP), ((mbytes, cbytes), 0)):
        case = Case(cuda, carried, new, 7, 8, state=st, caps=caps)
        want = case.check_forms(alias=True)
        assert want["status"] == bits and want["info"][9:11] == [mbytes, cbytes]
        assert int(want["payload_off"][want["K"]]) == mbytes and int(want["carry_off"][want["P"]]) == cbytes
        assert len(want["payload"]) == (0 if bits & ST_PAYLOAD_CAP else mbytes)


# -------------------------------------------------------------- a window of one
def test_golden_window_of_one_is_receive(cuda):
    """The reference's own traces at a window of one character: rudp_receive's
    accept, keep (= ranked), reply, reply_ack, state, message and reply frames."""
    import torch
    for c in golden_cases():
        frames = [bytes.fromhex(h) for h in c["frames"]]
        buf, off = pack_frames(frames)
        d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
        want = batch.receive(d_buf, d_off, "rudp5", state=tuple(c["state"]), last_isn=c["last_isn"])

        def one(form):
            got = batch.receive_windowed(d_buf, d_off, "rudp5", window_chars=1, state=tuple(c["state"]),
                                         last_isn=c["last_isn"])
            name = (form, c["name"])
            a, b = got.accepted, want.accepted
            assert torch.equal(a.accept, b.accept) and torch.equal((a.rank != -1).to(torch.uint8), b.keep), name
            assert torch.equal(a.reply, b.reply), name
            assert torch.equal(a.reply_ack.view(torch.uint8), b.reply_ack.view(torch.uint8)), name
            assert bytes(got.check().message.payload.cpu().numpy()).decode() == c["message"], name
            assert torch.equal(got.message.payload, want.message.payload), name
            assert torch.equal(got.state, want.state) and got.state.tolist() == c["state_after"] + [0], name
            R = want.reply_count
            assert got.reply_count == R and got.message_bytes == want.message_bytes, name
            assert got.reply_index.tolist() == want.reply_index[:R].tolist(), name
            assert got.reply_peer.tolist() == want.reply_peer[:R].tolist(), name
            assert torch.equal(got.reply_frames, want.reply_frames[:5 * R]), name
            assert a.end == c["end"] and got.carried.count == 0 and got.carried.nbytes == 0, name
        _forms(one)


# -------------------------------------------------------------- stream capture
def test_both_forms_under_stream_capture(cuda):
    """One call captured on a side stream (a linear capture) and replayed:
    nothing waits for the device or allocates outside the graph."""
    import torch
    rng = random.Random(0xCA97)
    case = crafted(cuda, rng, 5, 300, 8, 5, True)
    want = case.ref()
    st = torch.tensor(list(case.state) + [0], dtype=torch.int64, device=cuda)
    case.windowed(window_chars=8, csum=case.cs[1], state=st)  # (the carried frames handed over outside the capture)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))

    def one(form):
        kw = dict(window_chars=8, csum=case.cs[1], state=st, stream=s)
        with torch.cuda.stream(s):
            eager = case.windowed(**kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap = case.windowed(**kw)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap._buf[:cap._lay["payload"]], eager._buf[:eager._lay["payload"]]), form
        assert cap.info.tolist() == want["info"] and int(cap.status.item()) == 0, form
        assert np.array_equal(cap.message.payload.cpu().numpy(), want["payload"]), form
        nb = cap.carried.nbytes
        assert np.array_equal(cap.carried.frames[:nb].cpu().numpy(), want["carry_frames"]), form
        assert np.array_equal(cap.reply_frames.cpu().numpy(), want["reply_frames"]), form
    _forms(one)
