"""accept_window, receive_window and gather_ordered against the yardsticks
they are judged by, for one recvmmsg batch of 1024 one-character rudp5
datagrams (the stream a stop-and-wait sender leaves: accept_ref.clean_stream,
every frame usable on the wire).

Every result is first compared (accept_window at a window of one character
with accept_inorder bit for bit; receive_window's message and state with
receive_batch's and the fused receive's; gather_ordered with identity ranks
with gather_payloads); then the forms run in rotation (median of --reps rounds,
HIP events around 200 back-to-back calls) and, per form, the latency of one
call plus its synchronize:

  floor            one tiny torch kernel: the box's launch floor
  accept_inorder   the parent's acceptance                       (yardstick)
  accept_window    the same tables, window 1 / 8 / 1024
  accept_window_ws a windowed sender's stream (loss, duplicates, swaps), window 8
  receive_batch    the parent's chain of calls                   (yardstick)
  receive          the parent's fused call
  receive_window   the new chain, window 8 (two ordered gathers)
  gather_payloads  keep = every frame                            (yardstick)
  gather_ordered   identity ranks, skip = the header
  copy             rudpx_copy_vpt moving the gather's algorithmic bytes

With --windowed-out the one-call form is measured as well (receive_windowed):
for windows of 1, 8 and 1024 characters, one batch of 1024 one-character rudp5
datagrams of a windowed sender's stream (loss, duplication, swaps) behind the
frames the rule leaves pending in front of it, the forms in rotation in one
process, every round kept:

  receive_window            the chain of calls (the parent's code)     (yardstick)
  receive_windowed          the one call, fused kernel (librudp.so)
  receive_windowed_chained  the one call, knob 82 = 0 (diagnostics build)
  receive_batch, receive    the in-order forms on the new frames
  accept_window             the rule alone, on the decoded tables

and the mean-frame sweep of the fused kernel's limit (6 B, 32 B, 125 x 261 B,
32 x 1005 B: fused at knob 82 = 2 against chained).

usage: python tools/window_probe.py [--reps 7] [--out profiles/r12/window_probe.json]
                                    [--windowed-out profiles/r13/receive_window.json]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import random
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd"), str(REPO / "tests"), str(REPO / "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from accept_probe import copy_form, frames_for, latency, stream_arrays, timed  # noqa: E402
from rudp import _native, batch  # noqa: E402
from window_ref import window_ref, window_stream  # noqa: E402


class Knob:
    """Calls made inside run through the diagnostics build with knob 82 = value."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.tools = _native.tools_lib(activate=True)
        self.old = self.tools.rudpx_tune(82, self.value)

    def __exit__(self, *exc):
        self.tools.rudpx_tune(82, self.old)
        _native.use_product()


def rounds(forms, reps, inner=200):
    """forms: name -> (context or None, fn).  Every round times every form once,
    in rotation; returns name -> the rounds' microseconds per call."""
    per = {k: [] for k in forms}
    for _ in range(reps):
        for k, (ctx, fn) in forms.items():
            with ctx if ctx is not None else contextlib.nullcontext():
                per[k].append(timed(fn, inner) * 1e3)
    return per


def summary(per):
    return {k: {"us_per_call": statistics.median(v), "rounds": v} for k, v in per.items()}


def carried_of(dev, buf, off, H):
    """Frames on the host as an earlier receive_windowed result's ``carried``."""
    nc, nbytes = len(off) - 1, len(buf)
    lay = batch.ReceivedWindowed.layout(0, 0, H, 0, nbytes)
    owner = batch.ReceivedWindowed(torch.zeros(lay["size"], dtype=torch.uint8, device=dev), 0, 0, H, 0, nbytes, False)
    owner.carried.frames.copy_(torch.from_numpy(buf).to(dev))
    owner.carried.frame_off[:nc + 1].copy_(torch.from_numpy(off).to(dev))
    owner._info = [0, 0, 0, 0, 0, nc, 0, 0, 0, 0, nbytes, 0]
    return owner.carried


def windowed_section(args, dev):
    from accept_ref import pack_frames
    n, H = args.n, 5
    out = {"n_new": n, "layout": H, "reps": args.reps, "inner": 200, "windows": {}, "mean_sweep": {}}
    one = torch.zeros(1, device=dev)

    def frames_of(seq, flags, chars, rng):
        return [int(s).to_bytes(2, "big") + b"\x00\x00" + bytes([int(f)]) + bytes(rng.choice(b"abcdefgh") for _ in range(c))
                for s, f, c in zip(seq.tolist(), flags.tolist(), chars.tolist())]
    for Wc in (1, 8, 1024):
        rng = random.Random(1300 + Wc)
        seq, flags, chars, usable, state = window_stream(rng, 800 + n, Wc, 1)
        # the cut of [600, 800) that leaves the most frames pending
        k = max(range(600, 800, 7), key=lambda k: int(
            (window_ref(seq[:k], flags[:k], chars[:k], None, state, window_chars=Wc).accept == 2).sum()))
        r1 = window_ref(seq[:k], flags[:k], chars[:k], None, state, window_chars=Wc)
        pend = np.flatnonzero(r1.accept == 2)
        idx = np.concatenate([pend, np.arange(k, k + n)]).astype(np.int64)
        fr = frames_of(seq[idx], flags[idx], chars[idx], rng)
        m = len(pend)
        cbuf, coff = pack_frames(fr[:m]) if m else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
        nbuf, noff = pack_frames(fr[m:])
        d_new, d_off = torch.from_numpy(nbuf).to(dev), torch.from_numpy(noff).to(dev)
        st = torch.tensor([r1.state[0], r1.state[1], 1 if r1.state[2] else 0, 0], dtype=torch.int64, device=dev)
        car = carried_of(dev, cbuf, coff, H) if m else None
        chain_car = None
        if m:
            o = batch.OrderedPayloads(torch.from_numpy(cbuf).to(dev), torch.from_numpy(coff).to(dev),
                                      torch.arange(m, dtype=torch.int32, device=dev), None, None)
            o._total = (m, len(cbuf))
            chain_car = batch.CarriedFrames(o, None)
        kw = dict(window_chars=Wc, state=st)
        chain = lambda: batch.receive_window(d_new, d_off, H, carried=chain_car, **kw)
        call = lambda: batch.receive_windowed(d_new, d_off, H, carried=car, **kw)
        want = chain()
        dec = batch.unpack_batch_varlen(d_new, d_off, H, check=False, utf8=True)
        tabs = (dec.seq, dec.flags, batch.payload_chars(d_new, d_off, H))
        forms = {"floor": (None, lambda: one.add_(1)),
                 "receive_window": (None, chain),
                 "receive_windowed": (None, call),
                 "receive_windowed_chained": (Knob(0), call),
                 "receive_batch": (None, lambda: batch.receive_batch(d_new, d_off, H, state=st)),
                 "receive": (None, lambda: batch.receive(d_new, d_off, H, state=st)),
                 "accept_window": (None, lambda: batch.accept_window(*tabs, window_chars=Wc, state=st))}
        exact = {}
        for name in ("receive_windowed", "receive_windowed_chained"):
            ctx, fn = forms[name]
            with ctx if ctx is not None else contextlib.nullcontext():
                got = fn()
                exact[name] = bool(
                    torch.equal(got.message.payload, want.message.payload) and torch.equal(got.state, want.state)
                    and torch.equal(got.accepted.rank, want.accepted.rank)
                    and torch.equal(got.accepted.carry_rank, want.accepted.carry_rank)
                    and got.info.tolist()[:8] == want.accepted.info.tolist()
                    and got.carried.count == want.carried.count
                    and torch.equal(got.carried.frames[:got.carried.nbytes], want.carried.frames)
                    and got.reply_index.tolist() == want.reply_index.tolist()
                    and torch.equal(got.reply_frames, want.reply_frames(H)) and int(got.status.item()) == 0)
        per = rounds(forms, args.reps)
        rec = {"n_carried": m, "carried_bytes": int(len(cbuf)), "frames_bytes": int(len(nbuf)),
               "pending_after": want.carried.count, "first_anomaly": want.accepted.first_anomaly, "exact": exact,
               "ops": summary(per)}
        rec["fused_below_chain_every_round"] = all(a < b for a, b in zip(per["receive_windowed"], per["receive_window"]))
        rec["fused_below_chained_form_every_round"] = all(
            a < b for a, b in zip(per["receive_windowed"], per["receive_windowed_chained"]))
        us = {k: v["us_per_call"] for k, v in rec["ops"].items()}
        rec["ratios"] = {"receive_window_over_receive_windowed": us["receive_window"] / us["receive_windowed"],
                         "receive_windowed_over_receive": us["receive_windowed"] / us["receive"],
                         "receive_windowed_over_accept_window": us["receive_windowed"] / us["accept_window"]}
        out["windows"][str(Wc)] = rec
    # the fused kernel's mean-frame limit: a live in-order transfer, frames of one length
    for count, flen in ((1024, 6), (1024, 32), (125, 261), (32, 1005)):
        c = flen - H
        seq = np.array([(100 + j * c) & 0xFFFF for j in range(count)], np.uint16)
        rng = random.Random(flen)
        fr = frames_of(seq, np.zeros(count, np.uint8), np.full(count, c), rng)
        nbuf, noff = pack_frames(fr)
        d_new, d_off = torch.from_numpy(nbuf).to(dev), torch.from_numpy(noff).to(dev)
        st = torch.tensor([100, 99, 1, 0], dtype=torch.int64, device=dev)
        call = lambda: batch.receive_windowed(d_new, d_off, H, window_chars=8, state=st)
        forms = {"fused": (Knob(2), call), "chained": (Knob(0), call),
                 "receive_window": (None, lambda: batch.receive_window(d_new, d_off, H, window_chars=8, state=st))}
        with Knob(2):
            a = call()
        with Knob(0):
            b = call()
        same = bool(torch.equal(a.message.payload, b.message.payload) and a.info.tolist() == b.info.tolist()
                    and a.message_bytes == count * c)
        per = rounds(forms, args.reps)
        out["mean_sweep"][f"{count}x{flen}"] = {
            "frames": count, "frame_bytes": flen, "exact": same, "ops": summary(per),
            "fused_below_chained_every_round": all(x < y for x, y in zip(per["fused"], per["chained"]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--windowed-out", default=None)
    ap.add_argument("--windowed-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.windowed_out:
        text = json.dumps(windowed_section(args, dev), indent=1)
        print(text)
        path = Path(args.windowed_out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text + "\n")
        res = json.loads(text)
        if not all(v for w in res["windows"].values() for v in w["exact"].values()) or not all(
                v["exact"] for v in res["mean_sweep"].values()):
            raise SystemExit("a result differs from its reference")
        if args.windowed_only:
            return
    tools = _native.tools_lib(activate=False)  # the copy ceiling only; the calls are librudp.so's
    n = args.n
    host, d = stream_arrays(n, dev, seed=1024)
    H, frames, frame_off = frames_for("onechar", n, dev, host)
    seq, flags, chars, usable = d
    ws = window_stream(random.Random(8), n, 8, 1)
    wd = [torch.from_numpy(a).to(dev) for a in (ws[0], ws[1], ws[2].view(np.int32), ws[3])]
    wstate = torch.tensor(list(ws[4]) + [0], dtype=torch.int64, device=dev)
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n], dtype=torch.int64, device=dev)
    one = torch.zeros(1, device=dev)
    ops = {"floor": lambda: one.add_(1),
           "accept_inorder": lambda: batch.accept_inorder(seq, flags, chars, usable=usable),
           "accept_window_1": lambda: batch.accept_window(seq, flags, chars, window_chars=1, usable=usable),
           "accept_window_8": lambda: batch.accept_window(seq, flags, chars, window_chars=8, usable=usable),
           "accept_window_1024": lambda: batch.accept_window(seq, flags, chars, window_chars=1024, usable=usable),
           "accept_window_ws": lambda: batch.accept_window(wd[0], wd[1], wd[2], window_chars=8, usable=wd[3],
                                                           state=wstate),
           "receive_batch": lambda: batch.receive_batch(frames, frame_off, H),
           "receive": lambda: batch.receive(frames, frame_off, H),
           "receive_window": lambda: batch.receive_window(frames, frame_off, H, window_chars=8),
           "gather_payloads": lambda: batch.gather_payloads(frames, frame_off, H, check=False),
           "gather_ordered": lambda: batch.gather_ordered(frames, frame_off, ident, count, skip=H),
           "copy": copy_form(tools, int(frames.numel()) + 8 * (n + 1) + n + 8 * (n + 1), dev)}
    a, w = ops["accept_inorder"](), ops["accept_window_1"]()
    exact = {"accept_window_1": bool(
        torch.equal(w.accept, a.accept) and torch.equal((w.rank != -1).to(torch.uint8), a.keep)
        and torch.equal(w.reply, a.reply) and torch.equal(w.reply_ack.view(torch.uint8), a.reply_ack.view(torch.uint8))
        and torch.equal(w.state, a.state) and w.info.tolist()[:1] + w.info.tolist()[2:4] ==
        a.info.tolist()[:1] + a.info.tolist()[2:4] and w.fast)}
    r = window_ref(*ws[:4], ws[4], window_chars=8)
    g = ops["accept_window_ws"]()
    exact["accept_window_ws"] = bool(np.array_equal(g.accept.cpu().numpy(), r.accept)
                                     and np.array_equal(g.rank.cpu().numpy().view(np.uint32), r.rank)
                                     and g.info.tolist()[:4] == r.info[:4] and g.fast)
    rb, rf, rw = ops["receive_batch"](), ops["receive"](), ops["receive_window"]()
    exact["receive_window"] = bool(torch.equal(rw.message.payload, rb.message.payload)
                                   and torch.equal(rw.message.payload, rf.message.payload)
                                   and torch.equal(rw.state, rb.accepted.state) and torch.equal(rw.state, rf.state)
                                   and rw.reply_count == rf.reply_count)
    gp, go = ops["gather_payloads"](), ops["gather_ordered"]()
    exact["gather_ordered"] = bool(torch.equal(go.payload, gp.payload)
                                   and torch.equal(go.out_off, gp.payload_off) and int(go.status.item()) == 0)
    per = {k: [] for k in ops}
    for _ in range(args.reps):
        for k, fn in ops.items():
            per[k].append(timed(fn, 200) * 1e3)
    out = {"n": n, "layout": H, "frames_bytes": int(frames.numel()), "reps": args.reps, "exact": exact, "ops": {}}
    for k, fn in ops.items():
        out["ops"][k] = {"us_per_call": statistics.median(per[k]), "us_min_max": [min(per[k]), max(per[k])],
                         **latency(fn)}
    us = {k: v["us_per_call"] for k, v in out["ops"].items()}
    out["ratios"] = {"accept_window_1_over_accept_inorder": us["accept_window_1"] / us["accept_inorder"],
                     "accept_window_8_over_accept_inorder": us["accept_window_8"] / us["accept_inorder"],
                     "accept_window_ws_over_accept_inorder": us["accept_window_ws"] / us["accept_inorder"],
                     "receive_window_over_receive_batch": us["receive_window"] / us["receive_batch"],
                     "receive_window_over_receive": us["receive_window"] / us["receive"],
                     "gather_ordered_over_gather_payloads": us["gather_ordered"] / us["gather_payloads"],
                     "gather_ordered_over_copy": us["gather_ordered"] / us["copy"]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text + "\n")
    if not all(exact.values()):
        raise SystemExit("a result differs from its reference")


if __name__ == "__main__":
    main()
