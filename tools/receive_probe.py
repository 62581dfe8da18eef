"""batch.receive (rudp_receive) against what it replaces and the floor.

Every result is first compared bit for bit with the chain it stands for
(batch.receive_batch: decode + UTF-8, keep_mask, payload_chars, accept_inorder,
gather_payloads) and its reply datagrams with the torch formulation (nonzero +
index + pack_batch); then the forms of a shape run in rotation (median of
--reps rounds with the spread between rounds):

  receive_batch    the Python chain, product library (the yardstick);
  fused            batch.receive, product library: one launch of one workgroup
                   for a batch of at most RECV_TILE frames in RECV_FUSED_BYTES;
  chained          batch.receive through the diagnostics build with knob 80 off:
                   the chain's launches and the reply builder inside one call;
  fused_tools      the fused form through the diagnostics build (what the
                   runtime knobs of that build cost a call), also for batches
                   past the mean frame length at which the product stops using it;
  replies_torch    the reply datagrams alone, the torch formulation, from the
                   chain's tables;
  reply_builder    the chained form's reply builder alone (its three launches,
                   rudpx_receive_replies of the diagnostics build) on the tables
                   of one receive; reply_copy: rudpx_copy_vpt over (read +
                   written) / 2 of its algorithmic bytes;
  floor            one elementwise torch kernel on one element.

shapes
  batch1024  one recvmmsg batch of 1024 one-character rudp5 datagrams: us per
             call back to back and the latency of one call plus its synchronize;
  sweep      batches that fill the fused form's byte limit with payloads of 1,
             16, 64, 256 and 1000 bytes (1024 frames where they fit, else the
             most that do), fused against chained;
  large      1M one-character rudp5 datagrams and 64k x 1479-B rudp7 frames,
             batch.receive (the product: chained at these sizes) against receive_batch.

usage: python tools/receive_probe.py [--shapes batch1024,sweep,large] [--reps 7]
"""
from __future__ import annotations

import argparse
import ctypes
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

from rudp import _native, batch  # noqa: E402

SYN = 0x80


def stream(n, chars, seed):
    """seq, flags of n datagrams of `chars` characters a stop-and-wait sender
    leaves: in-order frames, one in five sent twice, a new transfer before the
    sequence numbers reach 2^16 (a transfer stalls there, as in the reference)."""
    rng = random.Random(seed)
    seq, flags = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    isn = sent = 0
    for i in range(n):
        if i == 0 or isn + sent + chars > 60000:
            isn, sent = rng.randint(1, 5000), 0
            seq[i], flags[i] = isn, SYN
            sent = chars
        elif not flags[i - 1] & SYN and rng.random() < 0.2:
            seq[i], flags[i] = seq[i - 1], 0
        else:
            seq[i], flags[i] = isn + sent, 0
            sent += chars
    return seq, flags


def frames_for(n, plen, H, dev, seed):
    seq, flags = (torch.from_numpy(a).to(dev) for a in stream(n, plen, seed))
    pay = torch.randint(0x20, 0x7F, (n * plen,), dtype=torch.uint8, device=dev)
    res = batch.pack_batch_varlen((seq, torch.zeros_like(seq), flags), pay,
                                  torch.full((n,), plen, dtype=torch.int32, device=dev), H, want_csum=False)
    return res.frames.clone(), res.frame_off.clone()


def replies_torch(acc, H):
    idx = torch.nonzero(acc.reply).view(-1)
    ack = acc.reply_ack.view(torch.int16)[idx].view(torch.uint16)  # (torch indexes no uint16)
    fr, cs = batch.pack_batch(batch.HeaderTable(torch.zeros_like(ack), ack, torch.full_like(idx, batch.ACK,
                                                                                          dtype=torch.uint8)),
                              torch.empty((idx.numel(), 0), dtype=torch.uint8, device=idx.device), H, want_csum=True)
    return fr, cs, idx


def exact(res, chain, H):
    a, b, R = res.accepted, chain.accepted, res.reply_count
    total = int(chain.message.payload_off[-1].item())
    fr, cs, idx = replies_torch(b, H)
    return bool(torch.equal(a.accept, b.accept) and torch.equal(a.keep, b.keep) and torch.equal(a.reply, b.reply)
                and torch.equal(a.reply_ack.view(torch.uint8), b.reply_ack.view(torch.uint8))
                and torch.equal(a.state, b.state) and torch.equal(a.info[:5], b.info[:5])
                and torch.equal(res.message.payload_off, chain.message.payload_off)
                and torch.equal(res.message.buffer[:total], chain.message.buffer[:total])
                and res.message_bytes == total and R == idx.numel()
                and torch.equal(res.reply_frames[:R * H], fr.view(-1))
                and torch.equal(res.reply_csum[:R].view(torch.uint8), cs.view(torch.uint8))
                and torch.equal(res.reply_index[:R].to(torch.int64), idx)
                and int(res.status.item()) == int(chain.message.status.item()))


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3


def latency(fn, reps=200):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return out[len(out) // 2]


class Forms:
    """The forms of one input; each switches to its library before it is timed."""

    def __init__(self, frames, frame_off, H, tools, dev):
        self.args, self.H, self.tools = (frames, frame_off, H), H, tools
        n = frame_off.numel() - 1
        fits = n <= batch.RECV_TILE and frames.numel() <= batch.RECV_FUSED_BYTES  # the fused kernel can take it
        self.fusable = fits and frames.numel() <= batch.RECV_FUSED_MEAN * n       # and the product gives it to it
        one = torch.zeros(1, device=dev)
        self.forms = {"receive_batch": (self._product, lambda: batch.receive_batch(*self.args)),
                      "chained": (self._chained, lambda: batch.receive(*self.args)),
                      "receive": (self._product, lambda: batch.receive(*self.args)),  # the form the product picks
                      "floor": (self._product, lambda: one.add_(1))}
        if self.fusable:
            self.forms["fused"] = (self._product, lambda: batch.receive(*self.args))
        if fits:
            self.forms["fused_tools"] = (self._tools, lambda: batch.receive(*self.args))
        _native.use_product()
        self.chain = batch.receive_batch(*self.args)
        self.forms["replies_torch"] = (self._product, lambda: replies_torch(self.chain.accepted, H))

    def add_reply_builder(self, dev):
        """The reply builder alone (rudpx_receive_replies of the diagnostics build) over the
        tables of one receive, and the copy of its algorithmic bytes; returns its exactness."""
        self._product()
        res = self.res = batch.receive(*self.args)
        n, H, R = len(res), self.H, res.reply_count
        ptr = lambda t: t.data_ptr()  # noqa: E731
        out = self.out = _native.RudpReceived(
            seq=ptr(res.seq), flags=ptr(res.flags), usable=ptr(res.usable), reply=ptr(res.accepted.reply),
            reply_ack=ptr(res.accepted.reply_ack), payload_off=ptr(res.message.payload_off),
            reply_frames=ptr(res.reply_frames), reply_csum=ptr(res.reply_csum), reply_index=ptr(res.reply_index),
            reply_peer=ptr(res.reply_peer), info=ptr(res.info))
        fn = self.tools.rudpx_receive_replies
        fn.argtypes = [ctypes.POINTER(_native.RudpReceived), ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
        stream = torch.cuda.current_stream(dev).cuda_stream

        def run():
            rc = fn(ctypes.byref(out), n, batch.NO_ISN, H, stream)
            assert rc == 0, rc
        # read: reply, usable, flags, seq by both passes, reply_ack once; written: frame, csum, index, peer
        self.reply_bytes = {"read": 2 * 5 * n + 2 * R, "written": R * (H + 2 + 4 + 8)}
        n16 = max(sum(self.reply_bytes.values()) // 2 // 16, 1)
        src = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
        dst = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)

        def copy():
            rc = self.tools.rudpx_copy_vpt(src.data_ptr(), dst.data_ptr(), n16, 4, 1, stream)
            assert rc == 0, rc
        self.forms["reply_builder"] = (self._product, run)
        self.forms["reply_copy"] = (self._product, copy)
        want = (res.reply_frames[:R * H].clone(), res.reply_csum[:R].clone().view(torch.uint8),
                res.reply_index[:R].clone(), res.reply_peer[:R].clone(), res.info.clone())
        for t in (res.reply_frames, res.reply_index, res.reply_peer):
            t.zero_()
        run()
        got = (res.reply_frames[:R * H], res.reply_csum[:R].view(torch.uint8), res.reply_index[:R],
               res.reply_peer[:R], res.info)
        return bool(all(torch.equal(g, w) for g, w in zip(got, want)) and not res.reply_frames[R * H:].any())

    def _product(self):
        self.tools.rudpx_tune(80, 1)
        _native.use_product()

    def _tools(self):
        self.tools.rudpx_tune(80, 2)  # (the fused kernel whatever the mean frame length)
        _native.tools_lib(activate=True)

    def _chained(self):
        _native.tools_lib(activate=True)
        self.tools.rudpx_tune(80, 0)

    def check(self):
        ok = {}
        for name in ("receive", "fused", "chained", "fused_tools"):
            if name in self.forms:
                setup, fn = self.forms[name]
                setup()
                ok[name] = exact(fn(), self.chain, self.H)
        self._product()
        return ok

    def measure(self, names, reps, inner, with_latency):
        per, lat = {k: [] for k in names}, {k: [] for k in names}
        for _ in range(reps):
            for k in names:
                setup, fn = self.forms[k]
                setup()
                per[k].append(timed(fn, inner))
                if with_latency:
                    lat[k].append(latency(fn, 50))
        self._product()
        out = {}
        for k in names:
            out[k] = {"us_per_call": statistics.median(per[k]), "us_per_call_min_max": [min(per[k]), max(per[k])]}
            if with_latency:
                out[k].update(us_latency=statistics.median(lat[k]), us_latency_min_max=[min(lat[k]), max(lat[k])])
        return out


def decide(ops):
    """fused is the default only if its median beats chained's by more than the
    spread between rounds (the wider of the two forms'), on every metric measured."""
    verdict = {}
    for metric in ("us_per_call", "us_latency"):
        if metric not in ops["chained"]:
            continue
        f, c = ops.get("fused") or ops["fused_tools"], ops["chained"]
        spread = max(f[metric + "_min_max"][1] - f[metric + "_min_max"][0],
                     c[metric + "_min_max"][1] - c[metric + "_min_max"][0])
        verdict[metric] = {"fused": f[metric], "chained": c[metric], "spread": spread,
                           "fused_wins": c[metric] - f[metric] > spread}
    verdict["fused_default"] = all(v["fused_wins"] for v in verdict.values())
    return verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="batch1024,sweep,large")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tools = _native.tools_lib(activate=False)
    out = {"reps": args.reps, "inner": args.inner, "recv_tile": batch.RECV_TILE,
           "recv_fused_bytes": batch.RECV_FUSED_BYTES}
    shapes = args.shapes.split(",")
    bad = []
    if "batch1024" in shapes:
        f = Forms(*frames_for(1024, 1, 5, dev, 1024), 5, tools, dev)
        rec = {"n": 1024, "layout": 5, "frames_bytes": int(f.args[0].numel()), "exact": f.check()}
        rec["ops"] = f.measure([k for k in f.forms if k != "receive"], args.reps, args.inner, True)
        rec["decision"] = decide(rec["ops"])
        out["batch1024"] = rec
        bad += [k for k, v in rec["exact"].items() if not v]
        print("batch1024", json.dumps(rec), file=sys.stderr, flush=True)
    if "sweep" in shapes:
        out["sweep"] = []
        for plen in (1, 16, 64, 256, 1000):
            n = min(1024, batch.RECV_FUSED_BYTES // (plen + 5))
            f = Forms(*frames_for(n, plen, 5, dev, plen), 5, tools, dev)
            rec = {"n": n, "payload": plen, "frames_bytes": int(f.args[0].numel()), "exact": f.check()}
            rec["ops"] = f.measure([k for k in ("fused", "fused_tools", "chained", "receive_batch") if k in f.forms],
                                   args.reps, args.inner, True)
            rec["decision"] = decide(rec["ops"])
            out["sweep"].append(rec)
            bad += [k for k, v in rec["exact"].items() if not v]
            print("sweep", json.dumps(rec), file=sys.stderr, flush=True)
    if "large" in shapes:
        out["large"] = []
        for n, plen, H in ((1 << 20, 1, 5), (1 << 16, 1472, 7)):
            f = Forms(*frames_for(n, plen, H, dev, n), H, tools, dev)
            rec = {"n": n, "payload": plen, "layout": H, "frames_bytes": int(f.args[0].numel()), "exact": f.check()}
            rec["exact"]["reply_builder"] = f.add_reply_builder(dev)
            rec["replies"], rec["reply_builder_bytes"] = f.res.reply_count, f.reply_bytes
            rec["ops"] = f.measure(["receive", "receive_batch", "replies_torch", "reply_builder", "reply_copy"],
                                   args.reps, 10, False)
            c, b = rec["ops"]["receive"], rec["ops"]["receive_batch"]
            spread = max(c["us_per_call_min_max"][1] - c["us_per_call_min_max"][0],
                         b["us_per_call_min_max"][1] - b["us_per_call_min_max"][0])
            rec["receive_minus_chain_us"] = c["us_per_call"] - b["us_per_call"]
            rec["spread_us"] = spread
            rec["not_slower_beyond_spread"] = c["us_per_call"] - b["us_per_call"] <= spread
            out["large"].append(rec)
            bad += [k for k, v in rec["exact"].items() if not v]
            print("large", json.dumps(rec), file=sys.stderr, flush=True)
            del f
            torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    if bad:
        raise SystemExit(f"a result differs from the chain: {bad}")


if __name__ == "__main__":
    main()
