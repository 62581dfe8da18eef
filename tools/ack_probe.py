"""batch.acknowledge / batch.ack_progress against what they replace and the floor.

Every result is first compared bit for bit with the chain it stands for
(unpack_batch_varlen -> the usable rule -> ack_progress) and with the plain-loop
rule (tests/ack_ref.py); then the forms of a shape run in rotation (median of
--reps rounds with the spread between rounds):

  fused          batch.acknowledge, product library: one launch of one workgroup
                 for a batch of at most ACK_TILE replies in ACK_FUSED_BYTES;
  chained        batch.acknowledge through the diagnostics build with knob 81
                 off: the decode, usable, rule and closing launches in one call;
  fused_tools    the fused form through the diagnostics build, also for batches
                 past the mean frame length at which the product stops using it;
  parse_loop     the per-datagram sender's host work for the same replies:
                 transport.parse() on every datagram and wait_ack's rule in
                 Python (no device involved);
  receive_fused  batch.receive on as many one-character datagrams (the fused
                 receive of the same run: the yardstick that does strictly more);
  floor          one elementwise torch kernel on one element.

shapes
  batch1024  one recvmmsg batch of 1024 five-byte rudp5 replies: us per call back
             to back and the latency of one call plus its synchronize;
  sweep      batches that fill the fused form's byte limit with reply frames of
             5, 16, 64, 256 and 1000 bytes (1024 frames where they fit, else the
             most that do), and header-only batches of 64..1024 replies: fused
             against chained (the byte limit and the cross-over);
  large      ack_progress over 1M replies (a clean stream in EXACT mode) against
             rudpx_copy_vpt over (read + written) / 2 of its algorithmic bytes
             and the torch formulation (cummax over the candidates);
  loopback   a 10k-character message over 127.0.0.1 to ReliableUDP(batch_recv=
             True): the windowed sender at windows 1, 8, 64 and 256 (exact and
             cumulative), seconds per transfer.

usage: python tools/ack_probe.py [--shapes batch1024,sweep,large,loopback] [--reps 7]
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

import ack_ref  # noqa: E402
from receive_probe import frames_for as datagrams_for  # noqa: E402
from rudp import _native, batch, transport  # noqa: E402

ISN = 3611


def replies_for(n, frame_len, seed, T=None):
    """n reply datagrams of frame_len bytes (rudp5; the payload, if any, is random
    bytes) of a clean stream; returns numpy frames, offsets and the stream."""
    rng = random.Random(seed)
    T = max(n // 3, 1) if T is None else T
    seq, ack, flags, usable = ack_ref.clean_replies(rng, n, isn=ISN, T=T, C=1, W=8, p_unusable=0.0)
    pay = bytes(rng.randrange(256) for _ in range(frame_len - 5))
    buf, off = ack_ref.pack_frames([ack_ref.header(int(seq[i]), int(ack[i]), int(flags[i]), 5, pay) for i in range(n)])
    return buf, off, (seq, ack, flags, usable), T


def exact(res, chain, rule, n):
    dec, prog = chain
    usable = ((dec.ok == 1) | (dec.ok == 3)).to(torch.uint8)
    same = (torch.equal(res.valid, prog.valid) and torch.equal(res.pointer, prog.pointer)
            and torch.equal(res.state, prog.state) and torch.equal(res.info, prog.info)
            and torch.equal(res.usable, usable) and torch.equal(res.ack.view(torch.uint8), dec.ack.view(torch.uint8))
            and torch.equal(res.seq.view(torch.uint8), dec.seq.view(torch.uint8)) and torch.equal(res.flags, dec.flags)
            and torch.equal(res.ok, dec.ok) and int(res.status.item()) == 0)
    same = same and np.array_equal(res.valid.cpu().numpy(), rule.valid) and res.state.cpu().tolist() == list(rule.state)
    if rule.final:
        same = same and bytes(res.final_frame.cpu().numpy()) == ack_ref.header(*rule.final, ack_ref.ACK)
    return bool(same and res.end == rule.end and res.first_anomaly == n)


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner * 1e3


def latency(fn, reps=50):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return out[len(out) // 2]


def host_timed(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    return (time.perf_counter() - t0) / inner * 1e6


class Forms:
    """The forms of one input; each switches to its library before it is timed."""

    def __init__(self, buf, off, stream, T, tools, dev, with_host=False):
        self.tools, self.T, n = tools, T, len(off) - 1
        self.n = n
        frames, frame_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
        kw = dict(isn=ISN, total_chars=T, chunk=1)
        call = lambda: batch.acknowledge(frames, frame_off, "rudp5", **kw)  # noqa: E731
        fits = n <= batch.ACK_TILE and len(buf) <= batch.ACK_FUSED_BYTES
        self.fusable = fits and len(buf) <= batch.ACK_FUSED_MEAN * n
        one = torch.zeros(1, device=dev)
        self.forms = {"chained": (self._chained, call), "floor": (self._product, lambda: one.add_(1))}
        if self.fusable:
            self.forms["fused"] = (self._product, call)
        if fits:
            self.forms["fused_tools"] = (self._tools, call)
        self._product()
        dec = batch.unpack_batch_varlen(frames, frame_off, 5, check=False)
        usable = ((dec.ok == 1) | (dec.ok == 3)).to(torch.uint8)
        self.chain = (dec, batch.ack_progress(dec.seq, dec.ack, dec.flags, usable=usable, **kw))
        self.rule = ack_ref.ack_ref(*stream[:3], None, isn=ISN, T=T, C=1)
        if with_host:
            datagrams = [bytes(buf[off[i]:off[i + 1]]) for i in range(n)]

            def parse_loop():
                p, L, last = ack_ref.fresh_state(T, 1)[:3]
                for d in datagrams:
                    r = transport.parse(d)
                    if r.ack != ISN + p + L:
                        continue
                    if r.flags & batch.ACK:
                        p = r.ack - ISN
                    if r.flags & batch.FIN:
                        return transport.build(ISN + p, r.seq + 1, batch.ACK)
                    if last:
                        L = 0
                    else:
                        L = min(1, T - p)
                        last = p + L == T
            self.parse_loop = parse_loop
            rf, ro = datagrams_for(n, 1, 5, dev, n)
            self.forms["receive_fused"] = (self._product, lambda: batch.receive(rf, ro, "rudp5"))

    def _product(self):
        self.tools.rudpx_tune(81, 1)
        _native.use_product()

    def _tools(self):
        self.tools.rudpx_tune(81, 2)  # (the fused kernel whatever the mean frame length)
        _native.tools_lib(activate=True)

    def _chained(self):
        _native.tools_lib(activate=True)
        self.tools.rudpx_tune(81, 0)

    def check(self):
        ok = {}
        for name in ("fused", "chained", "fused_tools"):
            if name in self.forms:
                setup, fn = self.forms[name]
                setup()
                ok[name] = exact(fn(), self.chain, self.rule, self.n)
        self._product()
        return ok

    def measure(self, names, reps, inner, with_latency=True):
        per, lat = {k: [] for k in names}, {k: [] for k in names}
        for _ in range(reps):
            for k in names:
                setup, fn = self.forms[k]
                setup()
                per[k].append(timed(fn, inner))
                if with_latency:
                    lat[k].append(latency(fn))
        self._product()
        out = {}
        for k in names:
            out[k] = {"us_per_call": statistics.median(per[k]), "us_per_call_min_max": [min(per[k]), max(per[k])]}
            if with_latency:
                out[k].update(us_latency=statistics.median(lat[k]), us_latency_min_max=[min(lat[k]), max(lat[k])])
        return out


def spread_of(a, b, metric):
    return max(a[metric + "_min_max"][1] - a[metric + "_min_max"][0], b[metric + "_min_max"][1] - b[metric + "_min_max"][0])


def decide(ops):
    """fused is the default only if its median beats chained's by more than the
    spread between rounds (the wider of the two forms'), on every metric measured."""
    verdict = {}
    f, c = ops.get("fused") or ops["fused_tools"], ops["chained"]
    for metric in ("us_per_call", "us_latency"):
        spread = spread_of(f, c, metric)
        verdict[metric] = {"fused": f[metric], "chained": c[metric], "spread": spread,
                           "fused_wins": c[metric] - f[metric] > spread}
    verdict["fused_default"] = all(v["fused_wins"] for v in verdict.values())
    return verdict


def torch_progress(ack, flags, usable, T):
    """The guess in torch: cummax of the candidates, then valid and the pointer
    (a clean stream: what ack_progress computes without its walk)."""
    d = (ack.view(torch.int16).to(torch.int64) & 0xFFFF) - ISN  # (torch converts no uint16)
    cand = (usable != 0) & ((flags & batch.ACK) != 0) & (d >= 0) & (d <= T)
    incl = torch.cummax(torch.where(cand, d, torch.zeros_like(d)), 0).values
    before = torch.cat((torch.zeros(1, dtype=torch.int64, device=d.device), incl[:-1]))
    valid = (usable != 0) & (d == before + torch.clamp(T - before, max=1))
    fin = valid & ((flags & batch.FIN) != 0)
    first = torch.where(fin.any(), torch.argmax(fin.to(torch.uint8)), torch.tensor(d.numel(), device=d.device))
    keep = torch.arange(d.numel(), device=d.device) <= first
    return (valid & keep).to(torch.uint8), torch.where(keep, incl, torch.zeros_like(incl))


def loopback(message, window, cumulative):
    """Seconds send() takes for one transfer to a batched receiver on this host."""
    import threading
    server = transport.ReliableUDP(codec_device="cuda:0", batch_recv=True).create()
    server.bind("127.0.0.1", 0)
    got, flushed = [], threading.Event()
    flush = server.flush_recv_buffer
    server.flush_recv_buffer = lambda: (flush(), flushed.set())
    t = threading.Thread(target=lambda: got.append(server.recv()), daemon=True)
    t.start()
    flushed.wait(10)
    client = transport.ReliableUDP(timeout=1, isn_source=lambda: 1000, codec_device="cuda:0", batch_send=True,
                                   window=window, cumulative=cumulative).create()
    t0 = time.perf_counter()
    client.send(message, "127.0.0.1", server.socket.getsockname()[1])
    dt = time.perf_counter() - t0
    t.join(30)
    client.close()
    server.close()
    return dt, got == [message]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="batch1024,sweep,large,loopback")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tools = _native.tools_lib(activate=False)
    out = {"reps": args.reps, "inner": args.inner, "ack_tile": batch.ACK_TILE, "ack_fused_bytes": batch.ACK_FUSED_BYTES,
           "ack_fused_mean": batch.ACK_FUSED_MEAN}
    shapes = args.shapes.split(",")
    bad = []
    if "batch1024" in shapes:
        f = Forms(*replies_for(1024, 5, 1024), tools, dev, with_host=True)
        rec = {"n": 1024, "layout": 5, "frames_bytes": 5 * 1024, "exact": f.check()}
        rec["ops"] = f.measure(list(f.forms), args.reps, args.inner)
        host = sorted(host_timed(f.parse_loop, 3) for _ in range(args.reps))
        rec["ops"]["parse_loop"] = {"us_per_call": host[len(host) // 2], "us_per_call_min_max": [host[0], host[-1]]}
        rec["decision"] = decide(rec["ops"])
        a, r = rec["ops"]["fused"], rec["ops"]["receive_fused"]
        rec["against_receive_fused"] = {m: {"acknowledge": a[m], "receive": r[m], "spread": spread_of(a, r, m),
                                            "not_slower_beyond_spread": a[m] - r[m] <= spread_of(a, r, m)}
                                        for m in ("us_per_call", "us_latency")}
        out["batch1024"] = rec
        bad += [k for k, v in rec["exact"].items() if not v]
        print("batch1024", json.dumps(rec), file=sys.stderr, flush=True)
    if "sweep" in shapes:
        out["sweep"] = []
        cases = [(min(1024, batch.ACK_FUSED_BYTES // flen), flen) for flen in (5, 16, 64, 256, 1000)]
        cases += [(n, 5) for n in (64, 256, 512)]
        for n, flen in cases:
            f = Forms(*replies_for(n, flen, flen + n), tools, dev)
            rec = {"n": n, "frame": flen, "frames_bytes": n * flen, "product_form": "fused" if f.fusable else "chained",
                   "exact": f.check()}
            rec["ops"] = f.measure([k for k in ("fused", "fused_tools", "chained") if k in f.forms], args.reps,
                                   args.inner)
            rec["decision"] = decide(rec["ops"])
            out["sweep"].append(rec)
            bad += [k for k, v in rec["exact"].items() if not v]
            print("sweep", json.dumps(rec), file=sys.stderr, flush=True)
    if "large" in shapes:
        n, T = 1 << 20, 60000
        rng = random.Random(n)
        seq, ack, flags, usable = ack_ref.clean_replies(rng, n, isn=ISN, T=T, C=1, W=64, fin=False, p_unusable=0.01)
        rule = ack_ref.ack_ref(seq, ack, flags, usable, isn=ISN, T=T, C=1)
        d = [torch.from_numpy(a).to(dev) for a in (seq, ack, flags, usable)]
        call = lambda: batch.ack_progress(d[0], d[1], d[2], usable=d[3], isn=ISN, total_chars=T)  # noqa: E731
        res = call()
        tv, tp = torch_progress(d[1], d[2], d[3], T)
        ok = {"ack_progress": bool(np.array_equal(res.valid.cpu().numpy(), rule.valid)
                                   and np.array_equal(res.pointer.cpu().numpy(), rule.pointer)
                                   and res.state.cpu().tolist() == list(rule.state) and res.fast),
              "torch": bool(torch.equal(tv, res.valid) and torch.equal(tp, res.pointer))}
        # read: ack, flags, usable by the join and the tile pass, valid by the count; written: valid, pointer
        nbytes = {"read": 2 * 4 * n + n, "written": 9 * n}
        n16 = sum(nbytes.values()) // 2 // 16
        src = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
        dst = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def copy():
            rc = tools.rudpx_copy_vpt(src.data_ptr(), dst.data_ptr(), n16, 4, 1, stream)
            assert rc == 0, rc
        forms = {"ack_progress": call, "copy": copy, "torch": lambda: torch_progress(d[1], d[2], d[3], T)}
        per = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                per[k].append(timed(fn, 20))
        rec = {"n": n, "algorithmic_bytes": nbytes, "exact": ok, "pointer_after": res.pointer_after,
               "ops": {k: {"us_per_call": statistics.median(v), "us_per_call_min_max": [min(v), max(v)]}
                       for k, v in per.items()}}
        out["large"] = rec
        bad += [k for k, v in ok.items() if not v]
        print("large", json.dumps(rec), file=sys.stderr, flush=True)
    if "loopback" in shapes:
        rng = random.Random(10000)
        message = "".join(rng.choice(("a", "é", "€", "😀")) for _ in range(10000))
        loopback(message[:50], 8, False)  # (warm: the first calls of every kernel)
        out["loopback"] = []
        for window, cumulative in ((1, False), (8, False), (64, False), (256, False), (64, True), (256, True)):
            runs = [loopback(message, window, cumulative) for _ in range(3)]
            secs = sorted(r[0] for r in runs)
            rec = {"characters": len(message), "window": window, "cumulative": cumulative, "delivered": all(r[1] for r in runs),
                   "seconds": secs[1], "seconds_min_max": [secs[0], secs[-1]]}
            out["loopback"].append(rec)
            bad += [] if rec["delivered"] else [f"loopback window {window}"]
            print("loopback", json.dumps(rec), file=sys.stderr, flush=True)
    out = json.loads(json.dumps(out), parse_float=lambda x: round(float(x), 3))  # (ns are below every spread here)
    print("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}")  # a line per shape
    if bad:
        raise SystemExit(f"a result differs from the chain or the rule: {bad}")


if __name__ == "__main__":
    main()
