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

usage: python tools/window_probe.py [--reps 7] [--out profiles/r12/window_probe.json]
"""
from __future__ import annotations

import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
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
