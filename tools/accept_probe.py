"""payload_chars and accept_inorder against the yardsticks they are judged by.

Every result is first compared bit for bit (payload_chars with the torch
formulation, accept_inorder with the CPU loop of tests/accept_ref.py); then the
forms of a shape run in rotation (median of --reps rounds, HIP events around
--inner back-to-back calls):

payload_chars
  chars   batch.payload_chars (rudp_payload_chars: one launch);
  torch   what a caller writes without it: the lead-byte mask of the whole
          buffer, its cumsum, and the difference at the frames' offsets;
  copy    rudpx_copy_vpt (diagnostics build) moving the call's algorithmic
          bytes: a copy of (read + written) / 2 bytes reads and writes as much
          as the call must -- frames and offsets once, 4 B per frame out.
accept_inorder
  accept  batch.accept_inorder on a stream a stop-and-wait sender produces
          (accept_ref.clean_stream: retransmissions, unusable copies, new
          transfers), where the one-scan form is exact;
  copy    the same copy yardstick: seq, flags, chars and usable read twice
          (9 B per frame each time), 5 B per frame written, and accept and
          reply read again by the last pass;
  cpu     accept_ref.accept_ref over the same arrays, once (a Python loop: the
          per-datagram loop the call replaces);
  walk    the same batch with a frame from the future put at index 0, so the
          sequential continuation walks every frame.

shapes: onechar (1M one-character rudp5 datagrams), mtu (1M x 1479-B rudp7
frames; payload_chars only: accept_inorder never sees the frames), batch1024
(one recvmmsg batch: per-call time back to back and the latency of one call
plus its synchronize, next to the box's launch + synchronize floor and the
whole receive_batch chain).

usage: python tools/accept_probe.py [--shapes onechar,mtu,batch1024] [--reps 7] [--n 1048576]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd"), str(REPO / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from accept_ref import accept_ref, clean_stream  # noqa: E402
from rudp import _native, batch  # noqa: E402


def torch_chars(frames, frame_off, H):
    """The formulation a caller writes today."""
    lead = (frames & 0xC0) != 0x80
    cs = torch.zeros(frames.numel() + 1, dtype=torch.int32, device=frames.device)
    torch.cumsum(lead, 0, dtype=torch.int32, out=cs[1:])
    start = torch.minimum(frame_off[:-1] + H, frame_off[1:])
    return cs[frame_off[1:]] - cs[start]


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def rotate(forms, reps):
    times = {name: [] for name, _, _ in forms}
    for _ in range(reps):
        for name, fn, inner in forms:
            times[name].append(timed(fn, inner))
    return ({k: statistics.median(v) for k, v in times.items()},
            {k: [min(v), max(v)] for k, v in times.items()})


def copy_form(tools, nbytes, dev):
    n16 = max(nbytes // 2 // 16, 1)
    src = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
    dst = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run():
        rc = tools.rudpx_copy_vpt(src.data_ptr(), dst.data_ptr(), n16, 4, 1, stream)
        assert rc == 0, rc
    return run


def stream_arrays(n, dev, seed=0xACCE97):
    """A clean stop-and-wait stream of n one-character datagrams, on the host and the device."""
    seq, flags, chars, usable = clean_stream(random.Random(seed), n, p_reset=0.0005, high_isn=0.0)
    d = [torch.from_numpy(a).to(dev) for a in (seq, flags, chars.view(np.int32), usable)]
    return (seq, flags, chars, usable), d


def frames_for(kind, n, dev, host=None):
    if kind == "mtu":
        tab, pay = batch.synth_batch(n, 1472, 0x5EED0004, device=dev)
        res = batch.pack_batch_varlen(tab, pay.view(-1), torch.full((n,), 1472, dtype=torch.int32, device=dev), 7)
        return 7, res.frames.clone(), res.frame_off.clone()
    _, pay = batch.synth_batch(n, 1, 0x5EED0004, device=dev)
    seq, flags = (torch.from_numpy(a).to(dev) for a in host[:2])
    res = batch.pack_batch_varlen((seq, torch.zeros_like(seq), flags), pay.view(-1),
                                  torch.ones(n, dtype=torch.int32, device=dev), 5, want_csum=False)
    return 5, res.frames.clone(), res.frame_off.clone()


def future_first(host, dev):
    """The stream with a frame from the future at index 0 and the live state it meets."""
    seq, flags = host[0].copy(), host[1].copy()
    isn = int(seq[0])
    seq[0], flags[0] = isn + 40000, 0
    return (seq, flags, host[2], host[3]), torch.from_numpy(seq).to(dev), torch.from_numpy(flags).to(dev), \
        (isn, isn, 1)


def accept_exact(acc, host, state=(0, 0, 0)):
    t0 = time.perf_counter()
    r = accept_ref(*host, state, None)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    ok = (np.array_equal(acc.accept.cpu().numpy(), r.accept) and np.array_equal(acc.keep.cpu().numpy(), r.keep)
          and np.array_equal(acc.reply.cpu().numpy(), r.reply)
          and np.array_equal(acc.reply_ack.cpu().numpy(), r.reply_ack)
          and acc.state.cpu().tolist() == [r.state[0], r.state[1], r.state[2], 0]
          and [acc.end, acc.count, acc.msg_start, acc.characters] == [r.end, r.count, r.msg_start, r.characters])
    return bool(ok), cpu_ms


def probe_chars(tools, kind, H, frames, frame_off, args, dev):
    n = frame_off.numel() - 1
    want = torch_chars(frames, frame_off, H)
    exact = bool(torch.equal(batch.payload_chars(frames, frame_off, H), want))
    del want
    read, written = int(frames.numel()) + 8 * (n + 1), 4 * n
    forms = (("chars", lambda: batch.payload_chars(frames, frame_off, H), args.inner),
             ("torch", lambda: torch_chars(frames, frame_off, H), args.torch_inner),
             ("copy", copy_form(tools, read + written, dev), args.inner))
    ms, span = rotate(forms, args.reps)
    return {"layout": H, "n": n, "frames_bytes": int(frames.numel()), "lanes_per_frame":
            batch.payload_chars_lanes(frames.numel() // n, H), "algorithmic_bytes": {"read": read, "written": written},
            "exact": exact, "ms": ms, "ms_min_max": span, "chars_over_torch": ms["chars"] / ms["torch"],
            "copy_over_chars": ms["copy"] / ms["chars"], "chars_TBps_algorithmic": (read + written) / ms["chars"] / 1e9}


def probe_accept(tools, host, d, args, dev):
    n = len(host[0])
    seq, flags, chars, usable = d
    run = lambda: batch.accept_inorder(seq, flags, chars, usable=usable)  # noqa: E731
    acc = run()
    exact, cpu_ms = accept_exact(acc, host)
    fast = acc.fast
    # a frame from the future at index 0 of a live receiver: the sequential form walks every frame
    whost, wseq, wflags, wstate = future_first(host, dev)
    walk = lambda: batch.accept_inorder(wseq, wflags, chars, usable=usable, state=wstate_t)  # noqa: E731
    wstate_t = torch.tensor(list(wstate) + [0], dtype=torch.int64, device=dev)
    wacc = walk()
    wexact, _ = accept_exact(wacc, whost, wstate)
    read, written = 2 * 9 * n + 2 * n, 5 * n
    forms = (("accept", run, args.inner), ("copy", copy_form(tools, read + written, dev), args.inner),
             ("walk", walk, 1))
    ms, span = rotate(forms, args.reps)
    ms["cpu"] = cpu_ms
    return {"n": n, "algorithmic_bytes": {"read": read, "written": written}, "exact": exact, "fast": fast,
            "walk_exact": wexact, "walk_first_anomaly": wacc.first_anomaly, "walk_end": wacc.end, "ms": ms,
            "ms_min_max": span, "copy_over_accept": ms["copy"] / ms["accept"], "cpu_over_accept": cpu_ms / ms["accept"],
            "walk_ns_per_frame": ms["walk"] * 1e6 / max(wacc.end if wacc.end < n else n, 1)}


def latency(fn, reps=200):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return {"us_latency": out[len(out) // 2], "p10_p90": [out[len(out) // 10], out[9 * len(out) // 10]]}


def probe_batch(tools, args, dev, n=1024):
    host, d = stream_arrays(n, dev, seed=1024)
    H, frames, frame_off = frames_for("onechar", n, dev, host)
    seq, flags, chars, usable = d
    one = torch.zeros(1, device=dev)
    _, wseq, wflags, wst = future_first(host, dev)
    wstate = torch.tensor(list(wst) + [0], dtype=torch.int64, device=dev)
    ops = {"floor": lambda: one.add_(1),
           "payload_chars": lambda: batch.payload_chars(frames, frame_off, H),
           "accept_inorder": lambda: batch.accept_inorder(seq, flags, chars, usable=usable),
           "accept_inorder_walk": lambda: batch.accept_inorder(wseq, wflags, chars, usable=usable, state=wstate),
           "decode_utf8": lambda: batch.unpack_batch_varlen(frames, frame_off, H, check=False, utf8=True),
           "receive_batch": lambda: batch.receive_batch(frames, frame_off, H)}
    acc = ops["accept_inorder"]()
    exact, cpu_ms = accept_exact(acc, host)
    wacc = ops["accept_inorder_walk"]()
    res = ops["receive_batch"]()
    every = batch.accept_inorder(seq, flags, chars)  # (the frames themselves are all usable)
    chain_exact = bool(torch.equal(res.accepted.accept, every.accept) and res.accepted.end == every.end
                       and torch.equal(res.accepted.state, every.state)
                       and int(res.message.payload_off[-1].item()) == int(every.keep.sum().item()))
    out = {"n": n, "exact": exact, "fast": acc.fast, "walk_first_anomaly": wacc.first_anomaly,
           "receive_batch_exact": chain_exact, "cpu_loop_us": cpu_ms * 1e3, "ops": {}}
    per = {k: [] for k in ops}
    for _ in range(args.reps):
        for k, fn in ops.items():
            per[k].append(timed(fn, 200) * 1e3)
    for k, fn in ops.items():
        out["ops"][k] = {"us_per_call": statistics.median(per[k]), **latency(fn)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="onechar,mtu,batch1024")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-inner", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tools = _native.tools_lib(activate=False)  # the copy ceiling only; the calls are librudp.so's
    out = {"n": args.n, "reps": args.reps, "inner": args.inner, "payload_chars": {}, "accept_inorder": {}}
    for kind in args.shapes.split(","):
        if kind == "batch1024":
            out["batch1024"] = probe_batch(tools, args, dev)
            print(kind, json.dumps(out["batch1024"]), file=sys.stderr, flush=True)
            continue
        host = d = None
        if kind == "onechar":
            host, d = stream_arrays(args.n, dev)
        elif kind != "mtu":
            raise SystemExit(f"unknown shape {kind!r}")
        H, frames, frame_off = frames_for(kind, args.n, dev, host)
        out["payload_chars"][kind] = probe_chars(tools, kind, H, frames, frame_off, args, dev)
        print(kind, "payload_chars", json.dumps(out["payload_chars"][kind]), file=sys.stderr, flush=True)
        del frames, frame_off
        torch.cuda.empty_cache()
        if host is not None:
            out["accept_inorder"][kind] = probe_accept(tools, host, d, args, dev)
            print(kind, "accept_inorder", json.dumps(out["accept_inorder"][kind]), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))
    recs = list(out["payload_chars"].values()) + list(out["accept_inorder"].values())
    small = out.get("batch1024", {"exact": True, "receive_batch_exact": True})
    if not all(r["exact"] and r.get("walk_exact", True) for r in recs) or not (small["exact"] and
                                                                                small["receive_batch_exact"]):
        raise SystemExit("a result differs from its reference")


if __name__ == "__main__":
    main()
