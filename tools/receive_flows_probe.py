"""rudp_receive_flows on one recvmmsg batch against what a caller has without it.

Shapes: 1024 one-character datagrams (layout 5, no sideband) of 1, 37 and 1024
flows (flows_probe.flow_batch), and one-flow batches of longer frames that fill
32768 bytes (receive_probe.frames_for): 125 x 261 B and 32 x 1005 B, the shapes
of profiles/r10/receive.json, and frames of 21, 69, 133 and 197 B between them
and the one-character batch.  They decide kRfFusedMeanFrame: the largest
measured mean at which the fused form beat the chained one in every round.

Every leg's result is first compared with the fused form's (and the fused
form's with the CPU oracle, tests/receive_flows_ref.py); then the legs of a
shape run in rotation (median of --reps rounds, HIP events around --inner
back-to-back calls; every library call made directly through ctypes on
preallocated outputs, so the time is the dispatch and not Python's).  The
table is written in place, so every timed call follows a copy of the pristine
rows (32 KiB, device to device); `reset` is that copy alone and `us` the
difference.

  fused     rudp_receive_flows, the one-workgroup kernel (diagnostics build,
            knob 83 = 2: also past the mean frame length)
  chained   the same call with knob 83 = 0
  product   the call from librudp.so, whichever form its constants choose
  calls     what a caller of the parent commit can do through ctypes:
            rudp_decode_varlen_utf8, the usable mask (three torch operations
            into preallocated tensors), rudp_payload_chars, rudp_accept_flows,
            rudp_gather_ordered.  It stops at the message: no reply and no
            closing datagrams.
  python    batch.receive_flows (no reply datagrams either)
  receive   rudp_receive on the one-flow batches (batch.receive's allocation
            made once, the call through ctypes)
  accept_flows / accept_flows_parent
            rudp_accept_flows alone on the 37-flow batch's tables, from this
            tree's library and, with --parent, from another build's (the parent
            commit's) in the same rotation: what the split of step 1 in
            flows_device.hpp costs.

usage: python tools/receive_flows_probe.py [--parent path/to/librudp.so] [--out profiles/r15/receive_flows.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd"), str(REPO / "tests"), str(REPO / "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flows_probe import flow_batch, timed  # noqa: E402
from receive_flows_ref import receive_flows_ref  # noqa: E402
from receive_probe import frames_for  # noqa: E402
from rudp import _native, batch  # noqa: E402

N = 1024
P, U64, U32, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
H = 5


def rotate(legs, reps, inner):
    """legs: name -> (before, call); `before` runs once ahead of each timing."""
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, (before, fn) in legs.items():
            if before:
                before()
            times[name].append(timed(fn, inner))
    return {k: {"us": statistics.median(v), "min_max": [min(v), max(v)], "rounds": v} for k, v in times.items()}


class Shape:
    def __init__(self, name, frames, off, flow, dev, tools, stream):
        self.name, self.frames, self.off, self.flow, self.dev = name, frames, off, flow, dev
        self.n, self.nbytes = off.shape[0] - 1, frames.numel()
        self.tools, self.stream = tools, stream
        self.pristine = torch.zeros((N, 4), dtype=torch.int64, device=dev)
        self.states = torch.zeros((N, 4), dtype=torch.int64, device=dev)
        self.lay = batch.ReceivedFlowsFused.layout(self.n, H, self.nbytes)
        self.bufs = {k: torch.zeros(self.lay["size"], dtype=torch.uint8, device=dev)
                     for k in ("fused", "chained", "product", "calls")}

    def reset(self):
        self.states.copy_(self.pristine)

    def call_new(self, h, which):
        base, lay, n = self.bufs[which].data_ptr(), self.lay, self.n
        out = _native.RudpReceivedFlows(payload_cap=self.nbytes, **{
            k: base + lay[{"csum_out": "csum"}.get(k, k)][0] for k, _ in _native.RudpReceivedFlows._fields_
            if k != "payload_cap"})
        ref = ctypes.byref(out)

        def call():
            self.reset()
            rc = h.rudp_receive_flows(self.frames.data_ptr(), self.nbytes, self.off.data_ptr(), self.nbytes // n, n,
                                      None, self.flow.data_ptr(), self.states.data_ptr(), N, ref, H, 0, self.stream)
            assert rc == 0, rc
        call.keep = out
        return call

    def call_parts(self, h):
        """The five steps a caller of the parent commit chains (no replies)."""
        base, lay, n = self.bufs["calls"].data_ptr(), self.lay, self.n
        at = {k: base + v[0] for k, v in lay.items() if k != "size"}
        res = batch.ReceivedFlowsFused(self.bufs["calls"], n, H, self.nbytes, self.states)
        ok, valid, usable = res.ok, res.valid, res.usable
        tmp = torch.empty(n, dtype=torch.bool, device=self.dev)
        tmp2 = torch.empty(n, dtype=torch.bool, device=self.dev)
        fr, nb, off = self.frames.data_ptr(), self.nbytes, self.off.data_ptr()

        def call():
            self.reset()
            rc = h.rudp_decode_varlen_utf8(fr, nb, off, nb // n, n, None, at["seq"], at["ack"], at["flags"], at["ok"],
                                           at["csum"], at["valid"], at["status"], H, 0, self.stream)
            assert rc == 0, rc
            torch.eq(ok, 1, out=tmp)
            torch.eq(ok, 3, out=tmp2)
            tmp.logical_or_(tmp2)
            torch.eq(valid, 1, out=tmp2)
            tmp.logical_and_(tmp2)
            usable.copy_(tmp)
            rc = h.rudp_payload_chars(fr, nb, off, nb // n, n, at["chars"], H, 0, self.stream)
            assert rc == 0, rc
            rc = h.rudp_accept_flows(at["seq"], at["flags"], at["chars"], at["usable"], self.flow.data_ptr(), n,
                                     self.states.data_ptr(), N, at["accept"], at["keep"], at["reply"], at["reply_ack"],
                                     at["rank"], at["order"], at["order_off"], at["flow_info"], at["info"],
                                     at["status"], 0, self.stream)
            assert rc == 0, rc
            rc = h.rudp_gather_ordered(fr, nb, off, nb // n, n, at["rank"], at["info"] + 8, H, at["payload"], nb,
                                       at["payload_off"], at["payload_src"], at["status"], 0, self.stream)
            assert rc == 0, rc
        return call

    def call_receive(self, h):
        n = self.n
        lay = batch.Received.layout(n, H, self.nbytes)
        buf = torch.zeros(lay["size"], dtype=torch.uint8, device=self.dev)
        base = buf.data_ptr()
        alay, acc = batch.Accepted.layout(n), base + lay["accepted"]
        out = _native.RudpReceived(
            seq=base + lay["seq"], ack=base + lay["ack"], flags=base + lay["flags"], ok=base + lay["ok"],
            csum_out=base + lay["csum"], valid=base + lay["valid"], usable=base + lay["usable"],
            chars=base + lay["chars"], accept=acc + alay[0], keep=acc + alay[1], reply=acc + alay[2],
            reply_ack=acc + alay[3], state_out=acc + alay[4], payload=base + lay["payload"], payload_cap=self.nbytes,
            payload_off=base + lay["payload_off"], reply_frames=base + lay["reply_frames"],
            reply_csum=base + lay["reply_csum"], reply_index=base + lay["reply_index"],
            reply_peer=base + lay["reply_peer"], info=acc + alay[5], status=base + lay["payload_off"] + 8 * (n + 1))
        ref, zero = ctypes.byref(out), torch.zeros(4, dtype=torch.int64, device=self.dev)

        def call():
            rc = h.rudp_receive(self.frames.data_ptr(), self.nbytes, self.off.data_ptr(), self.nbytes // n, n, None,
                                0xFFFFFFFF, zero.data_ptr(), ref, H, 0, self.stream)
            assert rc == 0, rc
        call.keep = (out, buf)
        return call

    def same(self, a, b, upto_message=False):
        """Leg b's buffer holds what leg a's holds (for `calls`: up to the message)."""
        ra = batch.ReceivedFlowsFused(self.bufs[a], self.n, H, self.nbytes, None)
        rb = batch.ReceivedFlowsFused(self.bufs[b], self.n, H, self.nbytes, None)
        names = ["seq", "ack", "flags", "ok", "valid", "usable", "chars", "accept", "keep", "reply", "reply_ack",
                 "rank", "order"]
        ok = all(ra.host(k).tobytes() == rb.host(k).tobytes() for k in names)
        A, K, R, E, total = ra.active, ra.kept, ra.replies, ra.ended, ra.message_bytes
        ok = ok and ra.host("info")[:5] == rb.host("info")[:5]
        ok = ok and np.array_equal(ra.flows(), rb.flows()) and np.array_equal(ra.host("order_off")[:A + 1],
                                                                              rb.host("order_off")[:A + 1])
        ok = ok and np.array_equal(ra.host("payload_off")[:K + 1], rb.host("payload_off")[:K + 1])
        ok = ok and np.array_equal(ra.host("payload_src")[:K], rb.host("payload_src")[:K])
        ok = ok and ra.host("payload")[:total].tobytes() == rb.host("payload")[:total].tobytes()
        if not upto_message:
            ok = ok and ra.host("info") == rb.host("info") and ra.host("status")[0] == rb.host("status")[0]
            for k, cnt in (("reply_frames", R * H), ("reply_csum", R), ("reply_index", R), ("fin_frames", E * H),
                           ("fin_csum", E), ("fin_flow", E)):
                ok = ok and np.array_equal(ra.host(k)[:cnt], rb.host(k)[:cnt])
        return bool(ok)

    def oracle(self):
        r = receive_flows_ref(self.frames.cpu().numpy(), self.off.cpu().numpy(),
                              self.flow.cpu().numpy().view(np.uint32), np.zeros((N, 4), np.uint64), H)
        g = batch.ReceivedFlowsFused(self.bufs["fused"], self.n, H, self.nbytes, None)
        K, R, E = r.flows.info[1], r.flows.info[2], r.flows.info[3]
        return bool(g.host("usable").tolist() == r.usable.tolist() and g.host("keep").tolist() == r.flows.keep.tolist()
                    and g.host("rank").view(np.uint32).tolist() == r.flows.rank.tolist()
                    and np.array_equal(g.flows().view(np.uint64), r.flows.flow_info)
                    and g.host("info")[:5] == r.flows.info and g.host("info")[8] == r.info[8]
                    and g.host("payload")[:r.info[8]].tobytes() == r.payload
                    and g.host("payload_off")[:K + 1].tolist() == r.payload_off.tolist()
                    and g.host("reply_frames")[:R * H].tobytes() == r.reply_frames
                    and g.host("fin_frames")[:E * H].tobytes() == r.fin_frames
                    and g.host("fin_flow")[:E].tolist() == r.fin_flow.tolist()
                    and np.array_equal(self.states.cpu().numpy().view(np.uint64), r.flows.states)
                    and int(g.host("status")[0]) == r.status)

    def measure(self, lib, reps, inner, one_flow):
        tune = self.tools.rudpx_tune
        legs = {"reset": (None, self.reset),
                "fused": (lambda: tune(83, 2), self.call_new(self.tools, "fused")),
                "chained": (lambda: tune(83, 0), self.call_new(self.tools, "chained")),
                "product": (None, self.call_new(lib, "product")),
                "calls": (None, self.call_parts(lib))}
        if one_flow:
            legs["receive"] = (None, self.call_receive(lib))
        for name, (before, fn) in legs.items():
            if before:
                before()
            fn()
        torch.cuda.synchronize(self.dev)
        exact = {"fused_equals_oracle": self.oracle(), "chained_equals_fused": self.same("fused", "chained"),
                 "product_equals_fused": self.same("fused", "product"),
                 "calls_equal_fused_up_to_the_message": self.same("fused", "calls", upto_message=True)}
        us = rotate(legs, reps, inner)
        tune(83, 1)

        def python():
            self.reset()
            return batch.receive_flows(self.frames, self.off, self.flow, H, states=self.states)
        us.update(rotate({"python": (None, python)}, reps, 50))
        wins = [a < b for a, b in zip(us["fused"]["rounds"], us["chained"]["rounds"])]  # (both with the reset)
        for k in ("fused", "chained", "product", "calls", "python"):
            us[k]["us_with_reset"] = us[k]["us"]
            us[k]["min_max_with_reset"] = us[k].pop("min_max")
            us[k]["us"] = us[k]["us"] - us["reset"]["us"]
        for v in us.values():
            v["rounds"] = [round(t, 2) for t in v["rounds"]]
        return {"n": self.n, "frames_bytes": self.nbytes, "mean_frame": self.nbytes / self.n, "exact": exact,
                "fused_beat_chained_in_every_round": all(wins), "us_per_call": us}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="another build of librudp.so (the parent commit's)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r15" / "receive_flows.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    tools = _native.tools_lib(activate=False)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"command": "python tools/receive_flows_probe.py" + (" --parent <the parent commit's librudp.so>"
                                                                if args.parent else ""),
           "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(dev), "layout": H,
           "shapes": {}}
    bad = []
    tables_37 = None
    for n_active in (1, 37, 1024):
        _, d = flow_batch(n_active, dev, 0xF10 + n_active)
        pay = torch.full((N,), 0x61, dtype=torch.uint8, device=dev)
        packed = batch.pack_batch_varlen((d[0], torch.zeros_like(d[0]), d[1]), pay, d[2].clone(), H, want_csum=False)
        shape = Shape(f"flows_{n_active}", packed.frames.clone(), packed.frame_off.clone(), d[4], dev, tools, stream)
        rec = shape.measure(lib, args.reps, args.inner, n_active == 1)
        out["shapes"][shape.name] = rec
        bad += [f"{shape.name}: {k}" for k, v in rec["exact"].items() if not v]
        print(shape.name, json.dumps(rec), file=sys.stderr, flush=True)
        if n_active == 37:
            res = batch.ReceivedFlowsFused(shape.bufs["fused"], N, H, shape.nbytes, None)
            tables_37 = (shape, res)
    for plen in (16, 64, 128, 192, 256, 1000):  # (16 .. 192: the means between the shapes above)
        n = min(N, batch.FLOWS_FUSED_BYTES // (plen + H))
        frames, off = frames_for(n, plen, H, dev, plen)
        shape = Shape(f"{n}x{plen + H}", frames, off, torch.zeros(n, dtype=torch.int32, device=dev), dev, tools, stream)
        rec = shape.measure(lib, args.reps, args.inner, True)
        rec["fused_over_chained"] = rec["us_per_call"]["fused"]["us"] / rec["us_per_call"]["chained"]["us"]
        out["shapes"][shape.name] = rec
        bad += [f"{shape.name}: {k}" for k, v in rec["exact"].items() if not v]
        print(shape.name, json.dumps(rec), file=sys.stderr, flush=True)

    # rudp_accept_flows alone, this build against the parent's, on the 37-flow batch's tables
    shape, res = tables_37
    lay = batch.FlowsAccepted.layout(N)
    sig = [P, P, P, P, P, U64, P, U64, P, P, P, P, P, P, P, P, P, P, I, P]

    def accept_call(h, buf):
        base = buf.data_ptr()

        def call():
            shape.reset()
            rc = h.rudp_accept_flows(
                res.seq.data_ptr(), res.flags.data_ptr(), res.chars.data_ptr(), res.usable.data_ptr(),
                shape.flow.data_ptr(), N, shape.states.data_ptr(), N,
                *(base + lay[k] for k in ("accept", "keep", "reply", "reply_ack", "rank", "order", "order_off",
                                          "flow_info", "info", "status")), 0, stream)
            assert rc == 0, rc
        return call
    mine = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
    legs = {"reset": (None, shape.reset), "accept_flows": (None, accept_call(lib, mine))}
    if args.parent:
        parent = ctypes.CDLL(str(Path(args.parent).resolve()))
        parent.rudp_accept_flows.argtypes, parent.rudp_accept_flows.restype = sig, I
        theirs = torch.zeros(lay["size"], dtype=torch.uint8, device=dev)
        legs["accept_flows_parent"] = (None, accept_call(parent, theirs))
    for _, fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    ab = {"us_per_call": rotate(legs, args.reps, args.inner)}
    for v in ab["us_per_call"].values():
        v["rounds"] = [round(t, 2) for t in v["rounds"]]
    if args.parent:
        ab["parent_equals_this"] = bool(torch.equal(mine, theirs))
        ab["this_minus_parent_us"] = (ab["us_per_call"]["accept_flows"]["us"]
                                      - ab["us_per_call"]["accept_flows_parent"]["us"])
        if not ab["parent_equals_this"]:
            bad.append("accept_flows: parent differs")
    out["accept_flows_ab"] = ab
    text = json.dumps(out, indent=1)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    if bad:
        raise SystemExit("a result differs from its reference: " + "; ".join(bad))


if __name__ == "__main__":
    main()
