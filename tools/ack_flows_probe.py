"""rudp_ack_flows on one recvmmsg batch (1024 replies) against what a caller
has without it.

Every result is first compared with the CPU oracle (tests/ack_flows_ref.py,
tests/flows_ref.py, tests/ack_ref.py); then the forms run in rotation (median
of --reps rounds, HIP events around --inner back-to-back calls, every library
call made directly through ctypes on preallocated outputs, so the time is the
dispatch and not Python's):

  ack_flows_1 / ack_flows_37 / ack_flows_1024
          rudp_ack_flows (final_layout 5) on 1024 replies of 1, 37 and 1024
          sends, each a clean reply stream (ack_ref.clean_replies, W = 4),
          interleaved.  The table is written in place, so every timed call
          follows a copy of the pristine rows (64 KiB, device to device);
          `reset_ack` is that copy alone and `us` the difference.
  loop_1 / loop_37 / loop_1024
          (a) what a caller has at the parent commit: the replies split by peer
          on the host (done once, outside the timing) and one rudp_ack_progress
          call per peer, 1, 37 and 1024 chained calls.
  accept_flows_1 / accept_flows_37 / accept_flows_1024
          (b) rudp_accept_flows on 1024 datagrams of as many flows, as
          tools/flows_probe.py times it (`reset_accept`: its 32 KiB table).
  floor   (c) a one-element torch add, the call-latency floor of DESIGN.

usage: python tools/ack_flows_probe.py [--out profiles/r15/ack_flows_probe.json]
"""
from __future__ import annotations

import argparse
import json
import random
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd"), str(REPO / "tests"), str(REPO / "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ack_flows_ref import ack_flows_ref, open_row  # noqa: E402
from ack_ref import ack_ref, clean_replies, fresh_state  # noqa: E402
from flows_probe import flow_batch, rotate  # noqa: E402
from flows_ref import arrival_order, flows_ref  # noqa: E402
from rudp import _native, batch  # noqa: E402

N = 1024
C, W = 3, 4


def reply_batch(n_active, seed):
    """N replies of n_active clean sends on slots 0 .. n_active - 1: the host
    arrays, the table, and every flow's constants."""
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, N), n_active - 1)) if n_active > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [N])]
    table = np.zeros((N, 8), np.uint64)
    streams, consts = [], []
    for k, m in enumerate(lens):
        isn, T = rng.randint(1, 5000), C * rng.randint(1, 40)
        streams.append(clean_replies(rng, m, isn=isn, T=T, C=C, W=W))
        table[k] = open_row(isn, T, C)
        consts.append((isn, T))
    pick = arrival_order(rng, lens)
    at = [0] * n_active
    cols = [np.zeros(N, np.uint16), np.zeros(N, np.uint16), np.zeros(N, np.uint8), np.zeros(N, np.uint8)]
    flow = np.zeros(N, np.uint32)
    for i, k in enumerate(pick):
        for c in range(4):
            cols[c][i] = streams[k][c][at[k]]
        at[k] += 1
        flow[i] = k
    return (*cols, flow), table, consts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r15" / "ack_flows_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": N, "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(dev), "exact": {},
           "walked": {}}
    forms, keep = {}, []
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    for n_active in (1, 37, 1024):
        host, table, consts = reply_batch(n_active, 0xAF + n_active)
        seq, ack, flags, usable, flow = host
        d = [to(seq), to(ack), to(flags), to(usable), to(flow.view(np.int32))]
        pristine = to(table.view(np.int64))
        states = pristine.clone()
        lay = batch.AckFlows.layout(N, 5)
        buf = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
        base = buf.data_ptr()

        def call(d=d, base=base, lay=lay, states=states, pristine=pristine):
            states.copy_(pristine)
            rc = lib.rudp_ack_flows(
                d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), N, 0,
                states.data_ptr(), N, *(base + lay[k] for k in ("valid", "pointer", "order", "order_off", "flow_info",
                                                                "info", "status")), 5,
                *(base + lay[k] for k in ("final_frames", "final_csum", "final_flow")), 0, stream)
            assert rc == 0, rc
        call()
        res = batch.AckFlows(buf, N, 5, states)
        f = ack_flows_ref(seq, ack, flags, usable, flow, table)
        out["exact"][f"ack_flows_{n_active}"] = bool(
            res.valid.cpu().numpy().tolist() == f.valid.tolist()
            and res.pointer.cpu().numpy().view(np.uint64).tolist() == f.pointer.tolist()
            and np.array_equal(res.flows().view(np.uint64), f.flow_info)
            and np.array_equal(states.cpu().numpy().view(np.uint64), f.states)
            and res.info.cpu().tolist()[:5] == f.info
            and [a for a, _ in res.finals()] == [a for a, _, _ in f.finals])
        out["walked"][f"ack_flows_{n_active}"] = int(res.info[5].item())
        forms[f"ack_flows_{n_active}"] = call
        if n_active == 1:
            forms["reset_ack"] = lambda states=states, pristine=pristine: states.copy_(pristine)

        # (a) one rudp_ack_progress call per peer on host-split tables
        parts, exact = [], True
        for k, (isn, T) in enumerate(consts):
            idx = np.flatnonzero(flow == k)
            m = len(idx)
            dk = [to(a[idx]) for a in (seq, ack, flags, usable)]
            st = to(np.array(fresh_state(T, C), np.int64))
            lay1 = batch.AckProgress.layout(m)
            b1 = torch.zeros(lay1["size"], dtype=torch.uint8, device=dev)

            def one(dk=dk, m=m, isn=isn, T=T, st=st, b=b1.data_ptr(), lay1=lay1):
                rc = lib.rudp_ack_progress(dk[0].data_ptr(), dk[1].data_ptr(), dk[2].data_ptr(), dk[3].data_ptr(), m,
                                           isn, T, C, 0, T, st.data_ptr(), b + lay1["valid"], b + lay1["pointer"],
                                           b + lay1["state"], b + lay1["info"], 0, stream)
                assert rc == 0, rc
            one()
            if k < 40:  # (the first flows' results against the rule)
                r = ack_ref(seq[idx], ack[idx], flags[idx], usable[idx], isn=isn, T=T, C=C)
                got = batch.AckProgress(b1, m)
                exact = exact and got.state.cpu().tolist() == list(r.state) and got.end == r.end
            parts.append(one)
            keep.append((dk, st, b1))

        def loop(parts=parts):
            for one in parts:
                one()
        out["exact"][f"loop_{n_active}"] = bool(exact)
        forms[f"loop_{n_active}"] = loop
        keep.append((d, buf, states, pristine))

    # (b) accept_flows at the same n and flow counts
    zero4 = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    states4 = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    forms["reset_accept"] = lambda: states4.copy_(zero4)
    for n_active in (1, 37, 1024):
        host, d = flow_batch(n_active, dev, 0xF10 + n_active, N)
        lay = batch.FlowsAccepted.layout(N)
        buf = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
        base = buf.data_ptr()

        def call(d=d, base=base, lay=lay):
            states4.copy_(zero4)
            rc = lib.rudp_accept_flows(
                d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), N,
                states4.data_ptr(), N, *(base + lay[k] for k in ("accept", "keep", "reply", "reply_ack", "rank", "order",
                                                                 "order_off", "flow_info", "info", "status")), 0, stream)
            assert rc == 0, rc
        call()
        res = batch.FlowsAccepted(buf, N, states4)
        f = flows_ref(*host, np.zeros((N, 4), np.uint64))
        out["exact"][f"accept_flows_{n_active}"] = bool(
            res.accept.cpu().numpy().tolist() == f.accept.tolist()
            and np.array_equal(res.flows().view(np.uint64), f.flow_info))
        forms[f"accept_flows_{n_active}"] = call
        keep.append((d, buf))

    # (c) the call-latency floor
    cell = torch.zeros(1, device=dev)
    forms["floor"] = lambda: cell.add_(1)

    if not all(out["exact"].values()):
        print(json.dumps(out["exact"], indent=1))
        raise SystemExit("a result differs from its reference")
    ms = rotate(forms, args.reps, args.inner)
    for kind, reset in (("ack_flows", "reset_ack"), ("accept_flows", "reset_accept")):
        for n_active in (1, 37, 1024):
            k = f"{kind}_{n_active}"
            ms[k]["us_with_reset"] = ms[k]["us"]
            ms[k]["min_max_with_reset"] = ms[k].pop("min_max")
            ms[k]["us"] = ms[k]["us"] - ms[reset]["us"]
    out["us_per_call"] = ms
    out["ratios"] = {f"loop_{k}_over_ack_flows_{k}": ms[f"loop_{k}"]["us"] / ms[f"ack_flows_{k}"]["us"]
                     for k in (1, 37, 1024)}
    out["ratios"].update({f"ack_flows_{k}_over_accept_flows_{k}": ms[f"ack_flows_{k}"]["us"]
                          / ms[f"accept_flows_{k}"]["us"] for k in (1, 37, 1024)})
    out["ratios"]["ack_flows_37_over_floor"] = ms["ack_flows_37"]["us"] / ms["floor"]["us"]
    text = json.dumps(out, indent=1)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
