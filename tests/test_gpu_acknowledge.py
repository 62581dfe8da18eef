"""rudp_ack_progress / rudp_acknowledge on the device.  Two oracles everywhere:
the plain-loop rule (tests/ack_ref.py, pinned to the reference's send() by
tests/golden/ack.json) and the chain of separate calls (unpack_batch_varlen ->
the usable rule -> ack_progress), every output compared bit for bit.  Every
fused-eligible input runs in both forms (knob 81 of the diagnostics build turns
the fused kernel off)."""
import random

import numpy as np
import pytest

from ack_ref import (ACK, CUMULATIVE, EXACT, FIN, ack_ref, adversarial_replies, canonical, clean_replies, csum_of,
                     fresh_state, golden_cases, header, info_ref, pack_frames, scan_model)
from rudp import _native, batch

pytestmark = pytest.mark.gpu

T = batch.ACK_TILE
FB = batch.ACK_FUSED_BYTES
MEAN = batch.ACK_FUSED_MEAN
PAD = 16      # sentinel bytes on either side of every output
SENT = 0xA5
NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
KINDS = dict(seq="u16", ack="u16", flags="u8", ok="u8", csum_out="u16", usable="u8", valid="u8", pointer="u64",
             state_out="u64", info="u64", final_frame="u8", final_csum="u16", status="u32")
MODE = {EXACT: _native.ACK_EXACT, CUMULATIVE: _native.ACK_CUMULATIVE}


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _forms(fn):
    """fn('fused') with the product library, then fn('chained') with the fused
    form turned off in the diagnostics build."""
    fn("fused")
    tools = _native.tools_lib(activate=True)
    try:
        assert tools.rudpx_tune(81, 0) == 1
        fn("chained")
    finally:
        tools.rudpx_tune(81, 1)
        _native.use_product()


def reply_frames(seq, ack, flags, usable, H, payloads=None):
    """The replies as datagrams (numpy buffer, offsets, rudp5 sideband checksums);
    an unusable one has a flipped ack bit under its old checksum."""
    frames, cs = [], []
    for i in range(len(ack)):
        pay = payloads[i] if payloads else b""
        s, a, f = int(seq[i]), int(ack[i]), int(flags[i])
        cs.append(csum_of(s, a, f, pay))
        fr = bytearray(header(s, a, f, H, pay))
        if not usable[i]:
            fr[3] ^= 0x10
        frames.append(bytes(fr))
    buf, off = pack_frames(frames)
    return buf, off, np.array(cs, np.uint16)


def _state_tensor(cuda, state):
    import torch
    return torch.tensor([int(v) for v in state], dtype=torch.int64).to(cuda)


def guarded_progress(cuda, seq, ack, flags, usable, *, isn, T_, C, state, mode=EXACT, sent=None, alias=False):
    """rudp_ack_progress with every output between sentinels; outputs as numpy."""
    import torch
    n = len(ack)
    size = dict(valid=n, pointer=n, state_out=4, info=8)
    bufs = {k: torch.full((2 * PAD + size[k] * NP[KINDS[k]]().itemsize,), SENT, dtype=torch.uint8, device=cuda)
            for k in size}
    ptr = {k: b.data_ptr() + PAD for k, b in bufs.items()}
    st_in = _state_tensor(cuda, state)
    if alias:
        ptr["state_out"] = st_in.data_ptr()
    d = [_dev(cuda, np.asarray(a, t)) for a, t in ((seq, np.uint16), (ack, np.uint16), (flags, np.uint8))]
    us = None if usable is None else _dev(cuda, np.asarray(usable, np.uint8))
    tab = n > 0
    _native.check(_native.lib().rudp_ack_progress(
        *(t.data_ptr() if tab else None for t in d), us.data_ptr() if us is not None and tab else None, n, isn, T_, C,
        MODE[mode], T_ if sent is None else sent, st_in.data_ptr(), ptr["valid"] if tab else None,
        ptr["pointer"] if tab else None, ptr["state_out"], ptr["info"], 0, None))
    got = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert (a[:PAD] == SENT).all() and (a[len(a) - PAD:] == SENT).all(), k
        got[k] = a[PAD:len(a) - PAD].view(NP[KINDS[k]])
    if alias:
        assert (got["state_out"].view(np.uint8) == SENT).all()
        got["state_out"] = st_in.cpu().numpy().view(np.uint64)
    return got


def expect(seq, ack, flags, usable, *, isn, T_, C, state, mode=EXACT, sent=None):
    """The rule's answer as the device lays it out."""
    n = len(ack)
    r = ack_ref(seq, ack, flags, usable, isn=isn, T=T_, C=C, state=state, mode=mode, sent=sent)
    first = n
    if n and not state[3]:
        first = scan_model(ack, flags, usable, isn=isn, T=T_, C=C, state=state, mode=mode, sent=sent).first_anomaly
    return r, dict(valid=r.valid, pointer=r.pointer.astype(np.uint64), state_out=np.array(r.state, np.uint64),
                   info=np.array(info_ref(r, n, C, first), np.uint64))


def check_progress(cuda, stream, **kw):
    alias = kw.pop("alias", False)
    seq, ack, flags, usable = stream
    r, want = expect(seq, ack, flags, usable, **kw)
    got = guarded_progress(cuda, seq, ack, flags, usable, alias=alias, **kw)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, len(ack), kw, got[k][:8], want[k][:8])
    return r, want


class Case:
    """Reply datagrams on the device, and the chain's and the rule's answer for them."""

    def __init__(self, cuda, stream, H, *, isn, T_, C=1, state=None, mode=EXACT, sent=None, sideband=True, mis=0,
                 payloads=None, frames=None):
        import torch
        self.cuda, self.H, self.mode = cuda, H, mode
        self.kw = dict(isn=isn, T_=T_, C=C, state=fresh_state(T_, C) if state is None else tuple(state), mode=mode,
                       sent=sent)
        if frames is None:
            buf, off, cs = reply_frames(*stream, H, payloads)
        else:
            buf, off, cs = frames
        self.n, self.nbytes = len(off) - 1, len(buf)
        self.room = torch.full((len(buf) + 64,), SENT, dtype=torch.uint8, device=cuda)  # guard bytes around the view
        self.frames = self.room[16 + mis:16 + mis + len(buf)]
        assert self.frames.data_ptr() % 16 == mis
        self.frames.copy_(_dev(cuda, np.asarray(buf, np.uint8)))
        self.off = _dev(cuda, np.asarray(off, np.int64))
        self.csum = _dev(cuda, cs) if H == 5 and sideband and cs is not None else None
        self.want = self._chain()

    def _chain(self):
        n, H, kw, w = self.n, self.H, self.kw, {}
        if n == 0:
            r, want = expect([], [], [], None, **kw)
            return dict(want, status=0, rule=r)
        dec = batch.unpack_batch_varlen(self.frames, self.off, H, csum=self.csum, check=False)
        usable = ((dec.ok == _native.OK_GOOD) | (dec.ok == _native.OK_UNVERIFIED)).to(dec.ok.dtype)
        prog = batch.ack_progress(dec.seq, dec.ack, dec.flags, isn=kw["isn"], total_chars=kw["T_"], chunk=kw["C"],
                                  usable=usable, state=kw["state"], mode=kw["mode"], sent=kw["sent"])
        for name, t in (("seq", dec.seq), ("ack", dec.ack), ("flags", dec.flags), ("ok", dec.ok),
                        ("csum_out", dec.csum), ("usable", usable), ("valid", prog.valid)):
            w[name] = t.cpu().numpy().copy()
        w["pointer"] = prog.pointer.cpu().numpy().view(np.uint64).copy()
        w["state_out"] = prog.state.cpu().numpy().view(np.uint64).copy()
        w["info"] = prog.info.cpu().numpy().view(np.uint64).copy()
        w["status"] = _native.ST_OFFSETS if (w["ok"] == _native.OK_BAD_OFFSETS).any() else 0
        # the chain is the rule
        r, want = expect(w["seq"], w["ack"], w["flags"], w["usable"], **kw)
        for k in want:
            assert np.array_equal(w[k], want[k]), ("chain", k, n)
        assert (prog.end, prog.count, prog.pointer_after, prog.done) == (r.end, r.count, r.state[0], bool(r.done))
        assert prog.fast == (prog.first_anomaly == n) and prog.next_frame == -(-r.state[0] // kw["C"])
        w["rule"] = r
        if r.final:
            w["final_frame"] = np.frombuffer(header(*r.final, ACK, H), np.uint8)
            w["final_csum"] = csum_of(*r.final, ACK)
        return w

    def call(self, alias=False, with_csum_out=True, with_final_csum=True):
        """rudp_acknowledge with every output between sentinels; outputs as numpy."""
        import torch
        n, H, cuda, kw = self.n, self.H, self.cuda, self.kw
        size = {k: n for k in KINDS}
        size.update(state_out=4, info=8, final_frame=H, final_csum=1, status=1)
        bufs = {k: torch.full((2 * PAD + size[k] * NP[KINDS[k]]().itemsize,), SENT, dtype=torch.uint8, device=cuda)
                for k in KINDS}
        st_in = _state_tensor(cuda, kw["state"])
        ptr = {k: b.data_ptr() + PAD for k, b in bufs.items()}
        if alias:
            ptr["state_out"] = st_in.data_ptr()
        skip = (set() if with_csum_out else {"csum_out"}) | (set() if with_final_csum else {"final_csum"})
        o = _native.RudpAcknowledged(**{k: (ptr[k] if (n or k in ("state_out", "info", "status")) and k not in skip
                                            else None) for k in KINDS})
        _native.check(_native.lib().rudp_acknowledge(
            self.frames.data_ptr() if self.nbytes else None, self.nbytes, self.off.data_ptr(),
            self.nbytes // n if n else 0, n, self.csum.data_ptr() if self.csum is not None and n else None,
            kw["isn"], kw["T_"], kw["C"], MODE[kw["mode"]], kw["T_"] if kw["sent"] is None else kw["sent"],
            st_in.data_ptr(), o, H, 0, None))
        got = {}
        for k, b in bufs.items():
            a = b.cpu().numpy()
            assert (a[:PAD] == SENT).all() and (a[len(a) - PAD:] == SENT).all(), k
            got[k] = a[PAD:len(a) - PAD].view(NP[KINDS[k]])
        if alias:
            assert (got["state_out"].view(np.uint8) == SENT).all()
            got["state_out"] = st_in.cpu().numpy().view(np.uint64)
        for k in skip:
            assert (got[k].view(np.uint8) == SENT).all(), k
        room = self.room.cpu().numpy()
        lo = 16 + self.frames.data_ptr() % 16
        assert (room[:lo] == SENT).all() and (room[lo + self.nbytes:] == SENT).all()
        return got, skip

    def check(self, form="", **kw):
        """One call equals the chain, array by array, and writes nothing else."""
        got, skip = self.call(**kw)
        w, n, tag = self.want, self.n, (form, self.n, self.H, self.mode)
        sent = lambda a: (a.view(np.uint8) == SENT).all()
        assert np.array_equal(got["state_out"], w["state_out"]), tag + (got["state_out"], w["state_out"])
        assert np.array_equal(got["info"], w["info"]), tag + (got["info"], w["info"])
        assert int(got["status"][0]) == w["status"], tag
        if n == 0:
            assert all(sent(got[k]) for k in got if k not in ("state_out", "info", "status")), tag
            return got
        for k in ("seq", "ack", "flags", "ok", "csum_out", "usable", "valid", "pointer"):
            if k not in skip:
                assert np.array_equal(got[k], w[k]), (k,) + tag
        if w["rule"].final:  # the closing datagram, Packet().to_byte() byte for byte
            assert np.array_equal(got["final_frame"], w["final_frame"]), tag
            if "final_csum" not in skip:
                assert int(got["final_csum"][0]) == w["final_csum"], tag
        else:                # end == n: nothing is written there
            assert sent(got["final_frame"]) and sent(got["final_csum"]), tag
        return got

    def check_forms(self, **kw):
        if self.n and self.n <= T and self.nbytes <= FB and self.nbytes <= MEAN * self.n:
            _forms(lambda form: self.check(form, **kw))
        elif self.n and self.n <= T and self.nbytes <= FB:
            # past the mean frame length the product chains; the fused kernel (knob 81 = 2) stays exact
            self.check("chained", **kw)
            tools = _native.tools_lib(activate=True)
            try:
                assert tools.rudpx_tune(81, 2) == 1
                self.check("fused past the mean", **kw)
            finally:
                tools.rudpx_tune(81, 1)
                _native.use_product()
        else:
            self.check("chained", **kw)


# ------------------------------------------------------- the reference's transfers
def _golden_stream(c):
    frames = [bytes.fromhex(h) for h in c["replies"]]
    seq = np.array([int.from_bytes(f[0:2], "big") for f in frames], np.uint16)
    ack = np.array([int.from_bytes(f[2:4], "big") for f in frames], np.uint16)
    flags = np.array([f[4] for f in frames], np.uint8)
    return frames, (seq, ack, flags, np.ones(len(frames), np.uint8))


def test_golden_one_call(cuda):
    """Every transfer the reference sent, its replies through batch.acknowledge in
    one call: the pointer and done it ended with, and its closing datagram."""
    def run(form):
        for c in golden_cases():
            frames, _ = _golden_stream(c)
            buf, off = pack_frames(frames)
            res = batch.acknowledge(_dev(cuda, buf), _dev(cuda, off), "rudp5", isn=c["isn"],
                                    total_chars=len(c["message"]), chunk=c["chunk"])
            name = (form, c["name"])
            assert (res.pointer_after, int(res.done)) == (c["pointer"], c["done"]), name
            assert res.state.cpu().tolist()[0] == c["pointer"] and int(res.check().status.item()) == 0, name
            if c["done"]:
                index, sent = c["sent"][-1]
                assert res.end == index and bytes(res.final_frame.cpu().numpy()).hex() == sent, name
            else:
                assert res.end == len(frames), name
            assert res.next_frame == -(-c["pointer"] // c["chunk"]), name

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
    """Every transfer cut at every reply boundary into two calls, the state carried
    on the device: the same valid, pointer, end, state and closing datagram."""
    import torch

    def run(form):
        for c in GROUPS[group]:
            frames, (seq, ack, flags, _) = _golden_stream(c)
            n, Tc, C, isn = len(frames), len(c["message"]), c["chunk"], c["isn"]
            r = ack_ref(seq, ack, flags, isn=isn, T=Tc, C=C)
            buf, off = pack_frames(frames)
            d_buf, d_off = _dev(cuda, buf), _dev(cuda, off)
            sig = _dev(cuda, np.concatenate([r.valid, r.pointer.view(np.uint8)]))
            st_after = torch.tensor(r.state, dtype=torch.int64, device=cuda)
            final = _dev(cuda, np.frombuffer(header(*r.final, ACK), np.uint8).copy()) if r.final else None
            bad = torch.zeros((), dtype=torch.int64, device=cuda)
            kw = dict(isn=isn, total_chars=Tc, chunk=C)

            def differs(res, lo, hi):
                got = torch.cat([res.valid, res.pointer.view(torch.uint8)])
                return (got != torch.cat([sig[lo:hi], sig[n + 8 * lo:n + 8 * hi]])).sum() + (res.status != 0).sum()

            for k in range(1, n):
                one = batch.acknowledge(d_buf[:off[k]], d_off[:k + 1], "rudp5", **kw)
                if r.end < k:
                    bad += differs(one, 0, k) + (one.info[0] != r.end) + (one.state != st_after).sum()
                    bad += (one.final_frame != final).sum()
                    continue
                two = batch.acknowledge(d_buf[off[k]:], d_off[k:] - int(off[k]), "rudp5", state=one.state, **kw)
                bad += differs(one, 0, k) + differs(two, k, n)
                bad += (one.info[0] != k) + (two.info[0] != r.end - k) + (two.state != st_after).sum()
                if final is not None:
                    bad += (two.final_frame != final).sum()
            assert int(bad.item()) == 0, (form, c["name"])

    _forms(run)


# ------------------------------------------------------------------- sizes
def _clean(n, *, isn=3611, C=1, W=8, seed=0, fin=True, T_=None, **kw):
    rng = random.Random(1000 * n + seed)
    T_ = max(n // 6, 1) * C if T_ is None else T_
    return clean_replies(rng, n, isn=isn, T=T_, C=C, W=W, fin=fin, **kw), dict(isn=isn, T_=T_, C=C)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5000])
def test_sizes(cuda, n):
    """Clean reply streams around every wave, tile and form boundary, both entry
    points, layouts 5 with its sideband, 5 unverified and 7; T is the last one-launch size."""
    for mode in (EXACT, CUMULATIVE):
        stream, kw = _clean(n, C=2 if mode == CUMULATIVE else 1)
        r, want = check_progress(cuda, stream, state=fresh_state(kw["T_"], kw["C"]), mode=mode, **kw)
        assert int(want["info"][4]) == n  # clean: the one-scan form alone
        if n > 2:
            assert r.done and r.end < n
        for H, sideband in ((5, True), (5, False), (7, False)):
            case = Case(cuda, stream, H, mode=mode, sideband=sideband, **kw)
            if not sideband and H == 5 and n:
                assert set(case.want["ok"]) == {3}
            case.check_forms()
    if n == 0:  # the Python entries' empty batch
        import torch
        z8, z16 = torch.zeros(0, dtype=torch.uint8, device=cuda), torch.zeros(0, dtype=torch.uint16, device=cuda)
        res = batch.acknowledge(z8, torch.zeros(1, dtype=torch.int64, device=cuda), "rudp5", isn=5, total_chars=9,
                                chunk=2, state=(4, 2, 0, 0))
        assert res.state.cpu().tolist() == [4, 2, 0, 0] and res.info.cpu().tolist() == [0, 0, 0, 4, 0, 2, 0, 0]
        assert not res.done and res.fast and res.next_frame == 2 and int(res.status.item()) == 0
        prog = batch.ack_progress(z16, z16, z8, isn=5, total_chars=9, chunk=2)
        assert prog.state.cpu().tolist() == [0, 2, 0, 0] and prog.info.cpu().tolist() == [0] * 8


def test_progress_300k(cuda):
    """300k replies: a clean stream (one scan), and the same with an anomaly in
    the middle (the walk over the rest)."""
    n, C = 300_000, 3
    stream, kw = _clean(n, C=C, isn=100, T_=60_000, fin=False)
    state = fresh_state(kw["T_"], C)
    r, want = check_progress(cuda, stream, state=state, **kw)
    assert int(want["info"][4]) == n and r.state[0] > 30_000
    seq, ack, flags, usable = (a.copy() for a in stream)
    at = 30_001
    flags[at], usable[at] = 0, 1   # a reply without the ACK flag: valid when it repeats the expected ack
    ack[at] = 100 + int(r.pointer[at - 1]) + C
    r2, want2 = check_progress(cuda, (seq, ack, flags, usable), state=state, **kw)
    assert int(want2["info"][4]) == at


# ------------------------------------------------------ anomalies and the FIN at tile edges
@pytest.mark.parametrize("at", [T - 1, T, T + 1])
def test_anomaly_and_fin_at_tile_edges(cuda, at):
    n, C, isn = 2 * T + 30, 2, 500
    for kind in ("future", "no_ack_flag", "fin", "fin_without_ack"):
        rng = random.Random(at)
        seq, ack, flags, usable = clean_replies(rng, n, isn=isn, T=4 * n, C=C, W=8, fin=False, p_unusable=0.02)
        state = fresh_state(4 * n, C)
        before = ack_ref(seq[:at], ack[:at], flags[:at], usable[:at], isn=isn, T=4 * n, C=C, state=state)
        p = before.state[0]
        usable[at] = 1
        if kind == "future":
            ack[at], flags[at] = isn + p + 3 * C, ACK
        elif kind == "no_ack_flag":
            ack[at], flags[at] = isn + p + C, 0
        else:
            ack[at], flags[at], seq[at] = isn + p + C, (ACK | FIN) if kind == "fin" else FIN, 65535
        stream = (seq, ack, flags, usable)
        r, want = check_progress(cuda, stream, isn=isn, T_=4 * n, C=C, state=state, alias=at == T)
        if kind in ("future", "no_ack_flag"):
            assert int(want["info"][4]) == at and not r.done, kind
        else:
            assert r.end == at and int(want["info"][4]) == n and r.final[1] == 0, kind
            assert not want["valid"][at + 1:].any() and not want["pointer"][at + 1:].any()
        Case(cuda, stream, 7, isn=isn, T_=4 * n, C=C, state=state).check_forms()
    # the same inside one launch: the anomaly on the last reply of the tile
    for m, a in ((T, T - 1), (T, 0), (65, 64)):
        seq, ack, flags, usable = clean_replies(random.Random(m), m, isn=isn, T=4 * m, C=C, fin=False)
        ack[a], flags[a], usable[a] = isn + 2 * m * C, ACK, 1
        case = Case(cuda, (seq, ack, flags, usable), 5, isn=isn, T_=4 * m, C=C)
        assert int(case.want["info"][4]) == a
        case.check_forms()


# ------------------------------------------------------------------ frames
def test_unaligned_frames_and_payloads(cuda):
    """d_frames a view at byte offsets 1, 5 and 15 of a larger buffer whose guard
    bytes stay as they were; replies that carry payloads (any bytes: wait_ack
    never decodes them), one long enough to leave the fused limits; the optional
    outputs left out."""
    rng = random.Random(7)
    n = 300
    stream, kw = _clean(n, C=3, seed=7)
    payloads = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 1, 2, 3, 7, 40)))) for _ in range(n)]
    for H, sideband in ((5, True), (7, False), (5, False)):
        for mis in (0, 1, 5, 15):
            case = Case(cuda, stream, H, sideband=sideband, mis=mis, payloads=payloads, **kw)
            assert case.want["rule"].done and case.want["usable"].sum() > n // 2
            case.check_forms(with_csum_out=mis != 5, with_final_csum=mis != 15)
    long = list(payloads)
    long[17] = bytes(rng.randrange(256) for _ in range(FB))  # the batch no longer fits the fused form's bytes
    case = Case(cuda, stream, 7, payloads=long, mis=3, **kw)
    assert case.nbytes > FB and case.want["rule"].done
    case.check_forms()
    few = [bytes(300) for _ in range(40)]                      # within the bytes, past the mean frame length
    stream40, kw40 = _clean(40, C=1, seed=3)
    case = Case(cuda, stream40, 5, payloads=few, **kw40)
    assert MEAN * 40 < case.nbytes <= FB
    case.check_forms()
    res = batch.acknowledge(case.frames, case.off, 5, csum=case.csum, isn=kw40["isn"], total_chars=kw40["T_"])
    assert np.array_equal(res.csum.cpu().numpy(), case.want["csum_out"]) and len(res) == 40
    assert np.array_equal(res.usable.cpu().numpy(), case.want["usable"]) and res.done == bool(case.want["rule"].done)


def test_bad_frames(cuda):
    """A corrupted checksum, a frame shorter than the header, an empty datagram, a
    decreasing offset pair and an offset past frames_bytes among good replies:
    the call's answer is the chain's, RUDP_ST_OFFSETS is set, the rejected
    frames are not usable and their bytes were not read (poisoning them changes
    nothing)."""
    for H, sideband in ((5, True), (7, False)):
        n = 64
        stream, kw = _clean(n, C=1, seed=H, p_unusable=0.0, p_repeat=0.0, T_=100)
        buf, off, cs = reply_frames(*stream, H)
        buf[off[20] + 2] ^= 0x40             # a header bit: the checksum no longer matches
        frames = [bytes(buf[off[i]:off[i + 1]]) for i in range(n)]
        frames[30] = frames[30][:3]          # shorter than the header
        frames[31] = b""                     # an empty datagram
        buf, off = pack_frames(frames)
        case = Case(cuda, None, H, frames=(buf, off, cs), sideband=sideband, **kw)
        assert [int(case.want["ok"][i]) for i in (20, 30, 31)] == [0, 2, 2] and case.want["status"] == 0
        assert not case.want["usable"][[20, 30, 31]].any() and case.want["valid"][:20].all()
        assert not case.want["valid"][20:].any()  # exact mode: the lost reply stalls the sender
        case.check_forms()
        cum = Case(cuda, None, H, frames=(buf, off, cs), sideband=sideband, mode=CUMULATIVE, **kw)
        assert cum.want["valid"][21] and cum.want["valid"][32:].all()  # cumulative mode goes on
        cum.check_forms()
        bad = off.copy()
        bad[41] = off[42] + 1                # frame 40 runs into 41, 41 has a decreasing pair
        bad[50] = len(buf) + 7               # frame 49 ends past the buffer, 50 starts there
        want = None
        for poison in (False, True):
            b2 = buf.copy()
            if poison:  # the bytes no valid frame covers: those of the rejected frames 49 and 50
                b2[off[49]:off[51]] ^= 0xFF
            case = Case(cuda, None, H, frames=(b2, bad, cs), sideband=sideband, mode=CUMULATIVE, **kw)
            assert case.want["status"] == _native.ST_OFFSETS
            rejected = [i for i in (40, 41, 49, 50) if case.want["ok"][i] == 4]
            assert len(rejected) >= 3 and not case.want["usable"][rejected].any()
            got = []
            _forms(lambda form: got.append(case.check(form)))
            for g in got:
                sig = {k: g[k].tobytes() for k in g}
                want = want or sig
                assert sig == want, poison


# ------------------------------------------------------ adversarial streams
def test_adversarial_streams(cuda):
    """Random ack_num, flags and usable bits, canonical and other seed states,
    both modes: the one-scan form and the sequential walk must both have run,
    and both entry points and forms stay exact; state_out aliasing state_in."""
    paths = {"fast": 0, "slow": 0}
    rng = random.Random(0xADE6)
    for k in range(16):
        n = rng.choice((7, 64, 257, 600, T, T + 1, 2 * T + 5))
        C = rng.choice((1, 2, 5))
        Tc = rng.choice((0, 3 * C, 7 * C - 1, 40 * C))
        isn = rng.choice((0, 100, 65530))
        mode = (EXACT, CUMULATIVE)[k % 2]
        sent = rng.randint(0, Tc) if mode == CUMULATIVE and k % 4 == 1 else None
        stream = adversarial_replies(rng, n, isn=isn, T=Tc, C=C)
        p = min(rng.randrange(0, Tc // C + 2) * C, Tc)
        L = min(C, Tc - p)
        state = rng.choice((fresh_state(Tc, C), (p, L, int(p + L == Tc), 0), (p, 0, 1, 0), (p, L + 1, 0, 0)))
        kw = dict(isn=isn, T_=Tc, C=C, state=state, mode=mode, sent=sent)
        r, want = check_progress(cuda, stream, alias=k % 2 == 0, **kw)
        case = Case(cuda, stream, (5, 7)[k % 2], **kw)
        case.check_forms(alias=k % 3 == 0)
        paths["fast" if int(want["info"][4]) == n else "slow"] += 1
        if not canonical(state, Tc, C):
            assert int(want["info"][4]) == 0
    assert paths["slow"] >= 3, paths  # (the clean streams of the other tests take the one-scan form alone)


def test_done_on_entry(cuda):
    """With done set nothing is judged: valid and pointer zero, end = n, the state
    copied, no closing datagram -- whatever the replies say."""
    for n in (5, T + 7):
        stream, kw = _clean(n, seed=1)
        state = (3, 1, 0, 1)
        r, want = check_progress(cuda, stream, state=state, alias=n == 5, **kw)
        assert not want["valid"].any() and not want["pointer"].any()
        assert want["info"].tolist() == [n, 0, 0, 3, n, 3, 1, 0] and want["state_out"].tolist() == [3, 1, 0, 1]
        Case(cuda, stream, 7, state=state, **kw).check_forms(alias=n != 5)


# ------------------------------------------------------------ stream capture
def _capture(cuda, n):
    import torch
    inputs = []
    for k in range(2):  # two inputs of one shape
        stream, kw = _clean(n, seed=k, C=2, p_repeat=0.0, p_unusable=0.0, fin=True, T_=n)
        if k:
            stream[1][n // 3] += 4   # a reply from the future: the walk runs in the replay
        buf, off, cs = reply_frames(*stream, 5)
        inputs.append((buf, cs, Case(cuda, None, 5, frames=(buf, off, cs), **kw).want))
    d_buf, d_cs = _dev(cuda, inputs[0][0]), _dev(cuda, inputs[0][1])
    d_off = _dev(cuda, off)
    state = _state_tensor(cuda, fresh_state(n, 2))
    call = lambda: batch.acknowledge(d_buf, d_off, "rudp5", csum=d_cs, isn=kw["isn"], total_chars=n, chunk=2,
                                     state=state)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        call()  # (warm: the stream's scratch set)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap = call()
    for buf, cs, want in (inputs[1], inputs[0]):
        d_buf.copy_(_dev(cuda, buf))
        d_cs.copy_(_dev(cuda, cs))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cap.valid.cpu().numpy(), want["valid"])
        assert np.array_equal(cap.pointer.cpu().numpy().view(np.uint64), want["pointer"])
        assert np.array_equal(cap.info.cpu().numpy().view(np.uint64), want["info"])
        assert np.array_equal(cap.state.cpu().numpy().view(np.uint64), want["state_out"])
        if want["rule"].final:
            assert np.array_equal(cap.final_frame.cpu().numpy(), want["final_frame"])


def test_capture_fused(cuda):
    """One capture of the one-launch form (n = 300), replayed on changed input."""
    _capture(cuda, 300)


def test_capture_chained(cuda):
    """One capture of the chained form (n = 3000, three tiles), replayed on changed input."""
    _capture(cuda, 3000)
