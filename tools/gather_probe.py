"""gather_payloads against the two yardsticks it is judged by, interleaved.

For every shape, three forms run in rotation (median of --reps rounds, HIP
events around --inner back-to-back calls), after the gather's output has been
compared bit for bit with the torch form's:

  gather  batch.gather_payloads(check=False) into a preallocated buffer
          (rudp_gather_payloads: three launches);
  torch   what a caller writes without it: a byte-level index built with
          repeat_interleave, then frames[idx] (8 B of index per payload byte,
          and one synchronization for the total);
  copy    rudpx_copy_vpt (diagnostics build) moving the gather's algorithmic
          bytes: a copy of (read + written) / 2 bytes reads and writes as much
          as the gather must -- frames once, offsets twice, the keep mask twice,
          payload and payload_off once.

shapes: mtu (1M x 1479-B rudp7 frames), ragged (1M rudp7 frames, payload
lengths uniform in [0, 2944]), onechar (1M one-character rudp5 datagrams, the
reference's traffic); each with keep=None and with a random half dropped.

usage: python tools/gather_probe.py [--shapes mtu,ragged,onechar] [--reps 7] [--n 1048576]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "reliable-udp_amd")]

import torch  # noqa: E402

from rudp import _native, batch  # noqa: E402


def make_frames(kind, n, dev):
    g = torch.Generator(device=dev).manual_seed(0x5EED0007)
    if kind == "mtu":
        H = 7
        tab, pay = batch.synth_batch(n, 1472, 0x5EED0004, device=dev)
        flat, lens = pay.view(-1), torch.full((n,), 1472, dtype=torch.int32, device=dev)
    elif kind == "ragged":
        H = 7
        lens = torch.randint(0, 2945, (n,), dtype=torch.int32, device=dev, generator=g)
        tab, _ = batch.synth_batch(n, 0, 0x5EED0004, device=dev)
        flat = torch.randint(0, 256, (int(lens.sum().item()),), dtype=torch.uint8, device=dev, generator=g)
    elif kind == "onechar":
        H = 5
        tab, pay = batch.synth_batch(n, 1, 0x5EED0004, device=dev)
        flat, lens = pay.view(-1), torch.ones(n, dtype=torch.int32, device=dev)
    else:
        raise SystemExit(f"unknown shape {kind!r}")
    res = batch.pack_batch_varlen(tab, flat, lens, H)
    frames, frame_off = res.frames.clone(), res.frame_off.clone()
    half = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    return H, frames, frame_off, half


def torch_gather(frames, frame_off, H, keep):
    """The formulation a caller writes today: (payload, payload_off)."""
    start = frame_off[:-1] + H
    plen = (frame_off[1:] - start).clamp_(min=0)
    if keep is not None:
        plen = plen * keep
    poff = torch.zeros(plen.numel() + 1, dtype=torch.int64, device=frames.device)
    torch.cumsum(plen, 0, out=poff[1:])
    idx = torch.repeat_interleave(start - poff[:-1], plen)  # (synchronizes: the output size)
    idx += torch.arange(idx.numel(), device=frames.device)
    return frames[idx], poff


def timed(fn, inner):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mtu,ragged,onechar")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-inner", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tools = _native.tools_lib(activate=False)  # the copy ceiling only; the gather is librudp.so's
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": args.n, "reps": args.reps, "inner": args.inner, "shapes": {}}
    for kind in args.shapes.split(","):
        H, frames, frame_off, half = make_frames(kind, args.n, dev)
        n = frame_off.numel() - 1
        for kname, keep in (("all", None), ("half", half)):
            want, want_off = torch_gather(frames, frame_off, H, keep)
            total = int(want.numel())
            buf = torch.full((frames.numel(),), 0xA5, dtype=torch.uint8, device=dev)

            def run_gather():
                return batch.gather_payloads(frames, frame_off, H, keep=keep, out=buf, check=False)

            got = run_gather()
            torch.cuda.synchronize()
            exact = bool(int(got.status.item()) == 0 and torch.equal(got.payload_off, want_off)
                         and torch.equal(buf[:total], want) and bool((buf[total:] == 0xA5).all()))
            del want
            # algorithmic bytes: frames read once (the kept ones), offsets twice, keep twice;
            # payload and payload_off written once
            kept_frame_bytes = int(((frame_off[1:] - frame_off[:-1]) * (keep if keep is not None else 1)).sum().item())
            read = kept_frame_bytes + 2 * 8 * (n + 1) + (2 * n if keep is not None else 0)
            written = total + 8 * (n + 1)
            n16 = (read + written) // 2 // 16
            src = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)
            dst = torch.empty(n16 * 16, dtype=torch.uint8, device=dev)

            def run_copy():
                rc = tools.rudpx_copy_vpt(src.data_ptr(), dst.data_ptr(), n16, 4, 1, stream)
                assert rc == 0, rc

            def run_torch():
                torch_gather(frames, frame_off, H, keep)

            forms = (("gather", run_gather, args.inner), ("torch", run_torch, args.torch_inner),
                     ("copy", run_copy, args.inner))
            times = {name: [] for name, _, _ in forms}
            for _ in range(args.reps):
                for name, fn, inner in forms:
                    times[name].append(timed(fn, inner))
            ms = {k: statistics.median(v) for k, v in times.items()}
            rec = {"layout": H, "frames_bytes": int(frames.numel()), "payload_bytes": total,
                   "algorithmic_bytes": {"read": read, "written": written}, "exact": exact, "ms": ms,
                   "ms_min_max": {k: [min(v), max(v)] for k, v in times.items()},
                   "gather_over_torch": ms["gather"] / ms["torch"],
                   "copy_over_gather": ms["copy"] / ms["gather"],
                   "gather_TBps_algorithmic": (read + written) / ms["gather"] / 1e9}
            out["shapes"][f"{kind}_{kname}"] = rec
            print(f"{kind}_{kname}", json.dumps(rec), file=sys.stderr, flush=True)
            del src, dst, buf
            torch.cuda.empty_cache()
        del frames, frame_off, half
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    if not all(r["exact"] for r in out["shapes"].values()):
        raise SystemExit("gather output differs from the torch formulation")


if __name__ == "__main__":
    main()
