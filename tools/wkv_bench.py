"""Times the WKV kernels (csrc/wkv.hip) at the encoder's training shape against the step-by-step
PyTorch formulation on the same GPU in the same process.

  shape     B=32, T=1500, C=768, bf16 and fp32, forward (with checkpoints) and backward
  baseline  tests/rwkv_ref.wkv in float32 on device tensors (one small torch kernel per operation
            and step) and its autograd backward
  timing    device events around one call, median of --reps calls after --warmup calls; for the
            kernels also the events ops.py records right around the launch (kernel_us: the call's
            own figure includes the host time between its two event records)

Design bytes per launch: forward k + v read, y written = 3 C e per frame, plus the checkpoints;
backward k, v, dy read and dk, dv written = 5 C e per frame, plus the checkpoints.  Reported as
achieved bytes/s and as a fraction of the 8 TB/s HBM peak (the scans' figures in DESIGN 3 use the
same peak).  Nothing here asserts a time.

usage: python tools/wkv_bench.py [--out profiles/wkv_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)   # us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--channels", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wkv_bench: needs a ROCm GPU (a CPU timing says nothing here)")
    from statecatcher_amd import _lib, ops
    from tests import rwkv_ref, wkv_cases
    dev = torch.device("cuda:0")
    B, T, C = args.batch, args.frames, args.channels
    case = wkv_cases.make("init", "random", B, T, C)
    td, tf = case["td"].to(dev), case["tf"].to(dev)
    state = tuple(s.to(dev) for s in case["state"])
    ckpt_bytes = _lib.load().sc_wkv_ckpt_numel(B, T, C) * 4
    rows = [{"shape": dict(B=B, T=T, C=C, chunk=ops.WKV_CHUNK, ckpt_bytes=ckpt_bytes),
             "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}]
    print(json.dumps(rows[0]), flush=True)

    def report(impl, dtype, what, us, nbytes=None, base=None, kernel=None):
        med = statistics.median(us)
        row = {"impl": impl, "dtype": dtype, "pass": what, "us_per_call": round(med, 1),
               "us_min": round(min(us), 1), "us_max": round(max(us), 1), "reps": len(us)}
        if kernel is not None:
            evs = [e0.elapsed_time(e1) * 1e3 for n, e0, e1, _, _ in ops.LAUNCH_EVENTS if n == kernel]
            ops.LAUNCH_EVENTS.clear()
            med = statistics.median(evs[-len(us):])
            row["kernel_us"] = round(med, 1)
        if nbytes is not None:
            row.update(design_bytes=nbytes, bytes_per_s=round(nbytes / med * 1e6),
                       frac_hbm_peak=round(nbytes / med * 1e6 / HBM_PEAK, 3))
        if base is not None:
            row["speedup_vs_torch_steps"] = round(base / med, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    # ---- the baseline: float32 step by step on the device
    k32, v32, r32 = (case[n].to(dev) for n in ("k", "v", "r"))

    def base_fwd():
        with torch.no_grad():
            return rwkv_ref.wkv(td, tf, k32, v32, state, torch.float32)

    ins = [t.clone().requires_grad_(True) for t in (td, tf, k32, v32)]
    held = {}

    def base_graph():
        held["y"] = rwkv_ref.wkv(*ins, state, torch.float32)[0]

    def base_bwd():
        base_graph()   # not timed apart: autograd frees the graph, so each backward needs its own
        for t in ins:
            t.grad = None
        held["y"].backward(r32)

    bf = report("torch_steps", "fp32", "fwd", event_times(base_fwd, args.reps, args.warmup))
    bg = statistics.median(event_times(base_graph, args.reps, args.warmup))
    bb = report("torch_steps", "fp32", "fwd+bwd", event_times(base_bwd, args.reps, args.warmup))
    bb_only = max(bb - bg, 1.0)
    rows.append({"impl": "torch_steps", "dtype": "fp32", "pass": "bwd (fwd+bwd minus graph fwd)",
                 "us_per_call": round(bb_only, 1)})
    print(json.dumps(rows[-1]), flush=True)
    held.clear()

    # ---- the kernels (bytes/s, the peak fraction and the ratio are of kernel_us)
    ops.LAUNCH_EVENTS = []
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        e = 2 if dt == torch.bfloat16 else 4
        k = case["k"].to(dev, dt).requires_grad_(True)
        v = case["v"].to(dev, dt).requires_grad_(True)
        r = case["r"].to(dev, dt)
        tdg, tfg = td.clone().requires_grad_(True), tf.clone().requires_grad_(True)
        fwd_bytes = 3 * B * T * C * e + ckpt_bytes
        bwd_bytes = 5 * B * T * C * e + ckpt_bytes

        def fwd():
            held["y"] = ops.wkv(tdg, tfg, k, v, state)[0]

        report("hip", name, "fwd", event_times(fwd, args.reps, args.warmup), fwd_bytes, bf,
               "wkv_fwd")
        fwd()
        ops.LAUNCH_EVENTS.clear()

        def bwd():
            torch.autograd.grad(held["y"], (tdg, tfg, k, v), r, retain_graph=True)

        report("hip", name, "bwd", event_times(bwd, args.reps, args.warmup), bwd_bytes, bb_only,
               "wkv_bwd")
        held.clear()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
