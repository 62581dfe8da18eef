"""segment_message against the two yardsticks it is judged by, interleaved.

For every shape, three forms run in rotation (median of --reps rounds, HIP
events around --inner back-to-back calls), after the segment table has been
compared bit for bit with the torch form's:

  segment  batch.segment_message(check=False, reuse=...) on the device message
           into a preallocated table (rudp_segment_utf8: three launches for chunks up to 16 characters,
           four above);
  torch    what a caller writes without it: the lead mask, nonzero (one
           synchronization for its size), a strided pick of the starts, diff
           for the lengths, arange for seq and flags;
  copy     rudpx_copy_vpt (diagnostics build) moving the call's algorithmic
           bytes: a copy of (read + written) / 2 bytes reads and writes as much
           as the call must -- the message once, the table once (seq, ack,
           flags, len and the payload offsets: 17 B per packet).

It also times frame_message (segment + pack_batch_varlen, packet count given,
no wait) against pack_batch_varlen alone on the same table: what the segment
step adds to framing a message.

shapes: ascii1 (1M ASCII characters, one per datagram: the reference's
traffic), mixed1 (1M characters of 1-4 bytes, one per datagram), mtu (1M x
1472 ASCII characters, 1472 per datagram).

With --rounds the call is also timed through the diagnostics build: by tile
size (knob 76) and, for chunks up to 16 characters, by the form of len[]
(knob 77: apron or differences), interleaved.

usage: python tools/segment_probe.py [--shapes ascii1,mixed1,mtu] [--reps 7] [--n 1048576] [--rounds 1,2,4,8,16]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd")]

import torch  # noqa: E402

from rudp import _native, batch  # noqa: E402

ISN = 3611


def make_message(kind, n, dev):
    """(device u8 message, characters per datagram)."""
    g = torch.Generator(device=dev).manual_seed(0x5EED0008)
    if kind == "ascii1":
        return torch.randint(32, 127, (n,), dtype=torch.uint8, device=dev, generator=g), 1
    if kind == "mixed1":
        rng = random.Random(0x5EED0008)
        text = "".join(rng.choices("aé€😀", k=n))
        return torch.frombuffer(bytearray(text.encode()), dtype=torch.uint8).to(dev), 1
    if kind == "mtu":
        return torch.randint(32, 127, (n * 1472,), dtype=torch.uint8, device=dev, generator=g), 1472
    raise SystemExit(f"unknown shape {kind!r}")


def torch_segment(msg, chunk, isn):
    """The formulation a caller writes today: (seq, ack, flags, lengths, payload_off)."""
    dev = msg.device
    pos = ((msg & 0xC0) != 0x80).nonzero().flatten()  # (synchronizes: the output size)
    starts = pos[::chunk]
    n = max(int(starts.numel()), 1)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    off[1:n] = starts[1:]
    off[0] = 0
    off[n] = msg.numel()
    lens = off.diff().to(torch.int32)
    k = torch.arange(n, dtype=torch.int64, device=dev)
    seq = ((isn + k * chunk) & 0xFFFF).to(torch.int16).view(torch.uint16)
    ack = torch.zeros(n, dtype=torch.int16, device=dev).view(torch.uint16)
    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    flags[0] |= batch.SYN
    flags[-1] |= batch.FIN
    return seq, ack, flags, lens, off


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ascii1,mixed1,mtu")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-inner", type=int, default=2)
    ap.add_argument("--rounds", default="", help="also time the call through the diagnostics build with these "
                    "rounds of 4096 bytes per tile (rudpx_tune 76), e.g. 1,2,4,8,16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tools = _native.tools_lib(activate=False)  # the copy ceiling only; the segment call is librudp.so's
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": args.n, "reps": args.reps, "inner": args.inner, "len_form": "apron for chunks up to 16 characters, differences above", "shapes": {}}
    for kind in args.shapes.split(","):
        msg, chunk = make_message(kind, args.n, dev)
        want = torch_segment(msg, chunk, ISN)
        n = int(want[0].numel())
        seg = batch.segment_message(msg, ISN, chunk=chunk, max_packets=n, check=False)

        def run_segment():
            return batch.segment_message(msg, ISN, chunk=chunk, max_packets=n, check=False, reuse=seg)

        got = run_segment()
        torch.cuda.synchronize()
        tab = got.table(n)
        exact = bool(int(got.status.item()) == 0 and got.count == n and same(tab.headers.seq, want[0])
                     and same(tab.headers.ack, want[1]) and same(tab.headers.flags, want[2])
                     and same(tab.lengths, want[3]) and same(tab.payload_off, want[4]))
        del want
        # algorithmic bytes: the message read once; the table written once
        read, written = int(msg.numel()), 17 * n + 8 + 24
        n16 = (read + written) // 2 // 16
        src = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
        dst = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)

        def run_copy():
            rc = tools.rudpx_copy_vpt(src.data_ptr(), dst.data_ptr(), n16, 4, 1, stream)
            assert rc == 0, rc

        def run_torch():
            torch_segment(msg, chunk, ISN)

        def run_frame():
            return batch.frame_message(msg, ISN, chunk=chunk, layout="rudp5", n=n, max_packets=n, check=False)

        def run_pack():
            return batch.pack_batch_varlen(tab.headers, msg, tab.lengths, "rudp5", want_csum=False, check=False)

        framed, packed = run_frame(), run_pack()
        torch.cuda.synchronize()
        exact = exact and int(framed.status.item()) == 0 and torch.equal(framed.frames, packed.frames) \
            and torch.equal(framed.frame_off, packed.frame_off)
        del framed, packed
        forms = (("segment", run_segment, args.inner), ("torch", run_torch, args.torch_inner),
                 ("copy", run_copy, args.inner), ("frame", run_frame, args.inner), ("pack", run_pack, args.inner))
        times = {name: [] for name, _, _ in forms}
        for _ in range(args.reps):
            for name, fn, inner in forms:
                times[name].append(timed(fn, inner))
        ms = {k: statistics.median(v) for k, v in times.items()}
        rec = {"chunk": chunk, "message_bytes": read, "packets": n,
               "algorithmic_bytes": {"read": read, "written": written}, "exact": exact, "ms": ms,
               "ms_min_max": {k: [min(v), max(v)] for k, v in times.items()},
               "segment_over_torch": ms["segment"] / ms["torch"],
               "copy_over_segment": ms["copy"] / ms["segment"],
               "frame_minus_pack_ms": ms["frame"] - ms["pack"],
               "frame_over_pack": ms["frame"] / ms["pack"]}
        if args.rounds:
            # the tile-size A/B: the same call through the diagnostics build, one knob value at a time
            _native.tools_lib(activate=True)
            sweep = {}
            try:
                for r in (int(x) for x in args.rounds.split(",")):
                    tools.rudpx_tune(76, r)
                    chk = run_segment()
                    torch.cuda.synchronize()
                    assert int(chk.status.item()) == 0 and same(chk.table(n).lengths, tab.lengths)
                    sweep[str(r)] = statistics.median(timed(run_segment, args.inner) for _ in range(args.reps))
                if chunk <= 16:
                    # the A/B of the two len forms (knob 77), interleaved, at the shipped tile size
                    tools.rudpx_tune(76, 0)
                    ab = {"differences": [], "apron": []}
                    for _ in range(args.reps):
                        for v, name in ((0, "differences"), (1, "apron")):
                            tools.rudpx_tune(77, v)
                            chk = run_segment()
                            torch.cuda.synchronize()
                            assert int(chk.status.item()) == 0 and same(chk.table(n).lengths, tab.lengths) \
                                and same(chk.table(n).payload_off, tab.payload_off) \
                                and same(chk.table(n).headers.flags, tab.headers.flags)
                            ab[name].append(timed(run_segment, args.inner))
                    rec["segment_ms_by_len_form"] = {k: statistics.median(v) for k, v in ab.items()}
            finally:
                tools.rudpx_tune(76, 0)
                tools.rudpx_tune(77, 1)
                _native.use_product()
            rec["segment_ms_by_rounds"] = sweep
        out["shapes"][kind] = rec
        print(kind, json.dumps(rec), file=sys.stderr, flush=True)
        del src, dst, msg, seg, got, tab
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    if not all(r["exact"] for r in out["shapes"].values()):
        raise SystemExit("segment output differs from the torch formulation")


if __name__ == "__main__":
    main()
