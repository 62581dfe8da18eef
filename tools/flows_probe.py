"""rudp_accept_flows on one recvmmsg batch (1024 datagrams) against what a
caller has without it.

Every result is first compared with the CPU oracle (tests/flows_ref.py); then
the forms run in rotation (median of --reps rounds, HIP events around --inner
back-to-back calls, every library call made directly through ctypes on
preallocated outputs, so the time is the dispatch and not Python's):

  flows_1 / flows_37 / flows_1024
          rudp_accept_flows on 1024 datagrams of 1, 37 and 1024 flows, each a
          clean stop-and-wait stream (accept_ref.clean_stream), interleaved.
          The table is written in place, so every timed call follows a copy of
          the pristine rows (32 KiB, device to device); `reset` is that copy
          alone and `us` the difference.
  flows_1_n256 / flows_1_n64
          one flow in a batch of 256 and of 64 datagrams: the sort runs 36 and
          21 barrier rounds instead of 55, the rest of the kernel as before.
  inorder / inorder_parent
          rudp_accept_inorder on the one-flow batch, from this tree's library
          and, with --parent, from another build's (the parent commit's), in
          the same rotation.
  loop_37 what a caller does for 37 peers today: the tables split on the host
          (done once, outside the timing) and 37 rudp_accept_inorder calls.
  receive_flows / receive_batch
          the Python chains (decode + usable + characters + acceptance +
          gather) on the one-flow batch's frames: batch.receive_flows against
          batch.receive_batch.

usage: python tools/flows_probe.py [--parent path/to/librudp.so] [--out profiles/r14/flows_probe.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd"), str(REPO / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from accept_ref import clean_stream  # noqa: E402
from flows_ref import flows_ref, interleave  # noqa: E402
from rudp import _native, batch  # noqa: E402

N = 1024
P, U64, U32, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / inner  # us


def rotate(forms, reps, inner):
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            times[name].append(timed(fn, inner))
    return {k: {"us": statistics.median(v), "min_max": [min(v), max(v)]} for k, v in times.items()}


def flow_batch(n_active, dev, seed, n=N):
    """n datagrams of n_active clean flows on slots 0 .. n_active - 1."""
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, n), n_active - 1)) if n_active > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    streams = [clean_stream(rng, m, p_reset=0.0, high_isn=0.0) for m in lens]
    host = interleave(rng, streams, list(range(n_active)))
    seq, flags, chars, usable, flow = host
    d = [torch.from_numpy(a).to(dev) for a in (seq, flags, chars.view(np.int32), usable, flow.view(np.int32))]
    return host, d


def inorder_call(h, d, n, state, outs, stream):
    m = (n + 7) & ~7
    at = [outs.data_ptr() + k for k in (0, m, 2 * m, 3 * m, 5 * m, 5 * m + 32)]

    def call():
        rc = h.rudp_accept_inorder(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, 0xFFFFFFFF,
                                   state.data_ptr(), *at, 0, stream)
        assert rc == 0, rc
    return call


def declare_inorder(h):
    h.rudp_accept_inorder.argtypes = [P] * 4 + [U64, U32] + [P] * 7 + [I, P]
    h.rudp_accept_inorder.restype = I
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="another build of librudp.so (the parent commit's)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r14" / "flows_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": N, "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(dev), "exact": {},
           "walked": {}}
    forms = {}

    # accept_flows with 1, 37 and 1024 flows, and one flow in smaller batches (fewer sort rounds)
    pristine = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    states = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    forms["reset"] = lambda: states.copy_(pristine)
    keep = []
    for n_active, n in ((1, N), (37, N), (1024, N), (1, 256), (1, 64)):
        name = f"flows_{n_active}" + (f"_n{n}" if n != N else "")
        host, d = flow_batch(n_active, dev, 0xF10 + n_active, n)
        lay = batch.FlowsAccepted.layout(n)
        buf = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
        base = buf.data_ptr()

        def call(d=d, base=base, n=n, lay=lay):
            states.copy_(pristine)
            rc = lib.rudp_accept_flows(
                d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n,
                states.data_ptr(), N, *(base + lay[k] for k in ("accept", "keep", "reply", "reply_ack", "rank", "order",
                                                                "order_off", "flow_info", "info", "status")), 0, stream)
            assert rc == 0, rc
        call()
        res = batch.FlowsAccepted(buf, n, states)
        f = flows_ref(*host, np.zeros((N, 4), np.uint64))
        out["exact"][name] = bool(
            res.accept.cpu().numpy().tolist() == f.accept.tolist() and res.keep.cpu().numpy().tolist() == f.keep.tolist()
            and res.reply_ack.cpu().numpy().tolist() == f.reply_ack.tolist()
            and res.rank.cpu().numpy().view(np.uint32).tolist() == f.rank.tolist()
            and np.array_equal(res.flows().view(np.uint64), f.flow_info)
            and np.array_equal(states.cpu().numpy().view(np.uint64), f.states)
            and res.info.cpu().tolist()[:5] == f.info)
        out["walked"][name] = int(res.info[5].item())
        forms[name] = call
        keep.append((d, buf))
        if name == "flows_1":
            one_d = d
        if n_active == 37:
            many_host = host

    # accept_inorder on the one-flow batch: this build and the parent's
    zero = torch.zeros(4, dtype=torch.int64, device=dev)
    outs = torch.zeros(5 * N + 80, dtype=torch.uint8, device=dev)
    forms["inorder"] = inorder_call(lib, one_d, N, zero, outs, stream)
    forms["inorder"]()
    mine = outs.clone()
    if args.parent:
        parent = declare_inorder(ctypes.CDLL(str(Path(args.parent).resolve())))
        forms["inorder_parent"] = inorder_call(parent, one_d, N, zero, outs, stream)
        outs.zero_()
        forms["inorder_parent"]()
        out["exact"]["inorder_parent_equals_inorder"] = bool(torch.equal(outs, mine))

    # 37 accept_inorder calls on host-split tables
    seq, flags, chars, usable, flow = many_host
    parts = []
    for slot in range(37):
        idx = np.flatnonzero(flow == slot)
        d = [torch.from_numpy(np.ascontiguousarray(a[idx])).to(dev) for a in (seq, flags, chars.view(np.int32), usable)]
        parts.append(inorder_call(lib, d, len(idx), zero, torch.zeros(5 * N + 80, dtype=torch.uint8, device=dev), stream))

    def loop_37():
        for call in parts:
            call()
    forms["loop_37"] = loop_37

    # the chains on the one-flow batch's frames
    pay = torch.from_numpy(np.full(N, 0x61, np.uint8)).to(dev)
    packed = batch.pack_batch_varlen((one_d[0], torch.zeros_like(one_d[0]), one_d[1]), pay,
                                     one_d[2].clone(), 5, want_csum=False)
    frames, off = packed.frames.clone(), packed.frame_off.clone()
    chain_states = torch.zeros((N, 4), dtype=torch.int64, device=dev)

    def receive_flows():
        chain_states.copy_(pristine)
        return batch.receive_flows(frames, off, one_d[4], 5, states=chain_states)
    got, want = receive_flows(), batch.receive_batch(frames, off, 5)
    out["exact"]["receive_flows_equals_receive_batch"] = bool(
        torch.equal(got.accepted.keep, want.accepted.keep)
        and got.pieces.payload.cpu().numpy().tobytes() == want.message.payload.cpu().numpy().tobytes())
    chains = {"receive_flows": receive_flows, "receive_batch": lambda: batch.receive_batch(frames, off, 5)}

    ms = rotate(forms, args.reps, args.inner)
    ms.update(rotate(chains, args.reps, 50))
    for k in ("flows_1", "flows_37", "flows_1024", "flows_1_n256", "flows_1_n64", "receive_flows"):
        ms[k]["us_with_reset"] = ms[k]["us"]
        ms[k]["min_max_with_reset"] = ms[k].pop("min_max")
        ms[k]["us"] = ms[k]["us"] - ms["reset"]["us"]
    out["us_per_call"] = ms
    out["ratios"] = {
        "flows_1_over_inorder": ms["flows_1"]["us"] / ms["inorder"]["us"],
        "loop_37_over_flows_37": ms["loop_37"]["us"] / ms["flows_37"]["us"],
        "receive_flows_over_receive_batch": ms["receive_flows"]["us"] / ms["receive_batch"]["us"],
    }
    if args.parent:
        out["ratios"]["inorder_over_inorder_parent"] = ms["inorder"]["us"] / ms["inorder_parent"]["us"]
    text = json.dumps(out, indent=1)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    if not all(out["exact"].values()):
        raise SystemExit("a result differs from its reference")


if __name__ == "__main__":
    main()
