#!/usr/bin/env python3
"""CTC forced alignment time on one GPU at C2's size (B=32, T=1500, V=1024), beside sc_ctc_fwd.

Seeded logits (scale * N(0,1), ragged input lengths) and seeded transcripts are aligned by
  * sc_ctc_align itself: the C call on buffers made once (pre-pass, walk + backtrace, finish);
  * ops.ctc_align: the same plus its allocations and the torch ops that build `labels`;
  * sc_ctc_fwd on the same tensors, in the same process: the only comparable kernel here (the same
    pre-pass and two lattice directions with a log-sum-exp, where alignment does one with a max),
for transcript lengths U = 150 and U drawn from [50, 150], in bf16 and fp32.  Each sample is a
device-event pair around --inner calls; reported is the median per call of --reps samples after
--warmup calls, the three implementations taken in turn within every round.

Prints one JSON object per measurement and, with --out, writes them to a JSON file.  The
per-kernel split comes from a profiler run of its own over `--only bf16_u150 --reps 2`.

usage: python tools/ctc_align_bench.py [--out profiles/ctc_align_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="calls per timed window (~20 ms and up)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="one configuration, e.g. bf16_u150")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench: needs a ROCm GPU (a CPU timing says nothing here)")
    from statecatcher_amd import _lib, ops
    from statecatcher_amd._lib import check, dtype_code, ptr, stream_of
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, V = args.batch, args.frames, args.vocab
    rng = np.random.default_rng(0)
    x = (args.scale * rng.standard_normal((B, T, V))).astype(np.float32)
    lens = np.full(B, T, np.int64)
    lens[1::2] -= rng.integers(0, T // 10, size=len(lens[1::2]))   # ragged, as a real batch
    umax = 150
    targets = torch.as_tensor(rng.integers(1, V, (B, umax))).to(dev)
    in_lens = torch.as_tensor(lens).to(dev)
    tgt = {"u150": np.full(B, umax, np.int64), "u50_150": rng.integers(50, umax + 1, B)}
    rows = []

    def report(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    report({"shape": dict(B=B, T=T, V=V, U_max=umax, live_frames=int(lens.sum()))})
    for dname, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        xd = torch.as_tensor(x).to(dev, dt)
        for uname, tl in tgt.items():
            cfg = f"{dname}_{uname}"
            if args.only and args.only != cfg:
                continue
            tgt_lens = torch.as_tensor(tl).to(dev)
            states = torch.empty(B, T, dtype=torch.int32, device=dev)
            frame_lp = torch.empty(B, T, dtype=torch.float32, device=dev)
            spans = torch.empty(B, umax, 2, dtype=torch.int32, device=dev)
            token_lp = torch.empty(B, umax, dtype=torch.float32, device=dev)
            score = torch.empty(B, dtype=torch.float32, device=dev)
            nll = torch.empty(B, dtype=torch.float32, device=dev)
            awb = lib.sc_ctc_align_workspace_bytes(B, T, umax)
            fwb = lib.sc_ctc_workspace_bytes(B, T, umax)
            aws = torch.empty(awb, dtype=torch.uint8, device=dev)
            fws = torch.empty(fwb, dtype=torch.uint8, device=dev)
            head = (ptr(xd), dtype_code(xd), 1, B, T, V, xd.stride(0), xd.stride(1), ptr(targets),
                    targets.stride(0), umax, ptr(in_lens), ptr(tgt_lens), 0)

            def c_align():
                check(lib.sc_ctc_align(*head, ptr(states), ptr(frame_lp), ptr(spans), ptr(token_lp),
                                       ptr(score), ptr(aws), awb, stream_of(xd)), "sc_ctc_align")

            def c_fwd():
                check(lib.sc_ctc_fwd(*head, ptr(nll), ptr(fws), fwb, stream_of(xd)), "sc_ctc_fwd")

            def op_align():
                ops.ctc_align(xd, targets, in_lens, tgt_lens, 0, True)

            impls = (("sc_ctc_align", c_align), ("ops.ctc_align", op_align), ("sc_ctc_fwd", c_fwd))
            for _, fn in impls:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            # the best path cannot beat the sum over all paths: a sanity check of what is timed
            assert bool((score <= -nll + 1e-4 * nll.abs()).all()), (score, nll)
            us = {name: [] for name, _ in impls}
            for _ in range(args.reps):
                for name, fn in impls:
                    us[name].append(sample(fn, args.inner))
            med = {name: statistics.median(v) for name, v in us.items()}
            for name, _ in impls:
                row = {"impl": name, "config": cfg, "us_per_call": round(med[name], 1),
                       "us_min": round(min(us[name]), 1), "us_max": round(max(us[name]), 1),
                       "reps": args.reps, "inner": args.inner,
                       "ratio_to_sc_ctc_fwd": round(med[name] / med["sc_ctc_fwd"], 2),
                       "workspace_MB": round((awb if "align" in name else fwb) / 1e6, 1)}   # 10^6 B
                if "align" in name:
                    row["mean_score_per_frame"] = round(float((score / in_lens).mean()), 3)
                report(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
