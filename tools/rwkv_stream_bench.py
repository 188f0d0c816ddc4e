#!/usr/bin/env python3
"""Streaming RWKV decode time per frame on one GPU: StreamingRWKV against the per-frame forward.

Model: RWKV-4 encoder, H = A = 512, I = 2048, L = 6, input 80, V = 1024, bf16 weights; B in
{1, 16, 64} concurrent streams, K in {1, 8} frames per call.  Two paths, in the same process and
taken in turn within every repeat:
  * stream    StreamingRWKV(encoder, B, K, dtype=bf16, graph=True).step(x): the copy of the block's
              input into the static buffer and one graph replay (RWKVEncoder.step on the step
              kernels of csrc/rwkv_step.hip and lucy_frame_gemm, then ctc_greedy_frames);
  * baseline  what there was before it: RWKVEncoder.forward(x[:, t:t+1], state) one frame at a
              time under bf16 autocast with the state carried, then ops.ctc_greedy_frames on the
              frame's logits.  It does not depend on K; it is measured beside every K all the same,
              so each ratio comes from one stretch of time on the machine.
Every shape is warmed up (kernel loading, library workspaces, the capture).  A sample is a
device-event pair around --blocks stream blocks, or around --baseline-frames baseline frames;
reported are the median, minimum and maximum per frame over --reps samples.

Prints one JSON object per point and, with --out, writes them to a JSON file.

usage: python tools/rwkv_stream_bench.py [--out profiles/rwkv_stream_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n):
    """ms per call of fn over n calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--inter", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--input", type=int, default=80)
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--blocks", type=int, default=200, help="stream blocks per timed window")
    ap.add_argument("--baseline-frames", type=int, default=200,
                    help="baseline frames per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rwkv_stream_bench: needs a ROCm GPU (a CPU timing says nothing here)")
    import statecatcher_amd as sc
    from statecatcher_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = sc.RWKVEncoder(sc.RWKVConfig(
        input_dim=args.input, hidden_size=args.hidden, num_layers=args.layers,
        vocab_size=args.vocab, attention_hidden_size=args.hidden,
        intermediate_size=args.inter)).to(dev).eval().requires_grad_(False)
    rows = []

    def report(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    report({"model": dict(H=args.hidden, A=args.hidden, I=args.inter, L=args.layers,
                          input=args.input, V=args.vocab, dtype="bf16"),
            "device": torch.cuda.get_device_name(0), "blocks": args.blocks,
            "baseline_frames": args.baseline_frames, "reps": args.reps})
    for B in args.batches:
        for K in args.ks:
            g = torch.Generator().manual_seed(B * 100 + K)
            xb = torch.randn(B, K, args.input, generator=g).to(dev)
            st = sc.StreamingRWKV(enc, batch=B, frames_per_call=K, dtype=torch.bfloat16, graph=True)
            # the baseline's carried state and static decode buffers
            base = {"state": None}
            prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
            emit = torch.full((1, B), -1, dtype=torch.int32, device=dev)
            x1 = xb[:, :1].contiguous()

            def stream_block():
                st.step(xb)

            def baseline_frame():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    logits, base["state"] = enc(x1, base["state"])
                ops.ctc_greedy_frames(logits.transpose(0, 1), prev, emit)

            for _ in range(args.warmup):
                stream_block()
                baseline_frame()
            torch.cuda.synchronize()
            # what is timed computes the same thing: the first frame of both from the zero state
            st.reset()
            base["state"] = None
            st.step(xb)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                lg, _ = enc(x1)
            a, b = st.logits[0].float(), lg[:, 0].float()
            agree = float((a - b).norm() / b.norm())
            ms = {"stream": [], "baseline": []}
            for _ in range(args.reps):
                ms["stream"].append(timed(stream_block, args.blocks) / K)
                ms["baseline"].append(timed(baseline_frame, args.baseline_frames))
            med = {k: statistics.median(v) for k, v in ms.items()}
            report({"B": B, "K": K,
                    "stream_ms_per_frame": round(med["stream"], 4),
                    "stream_min": round(min(ms["stream"]), 4),
                    "stream_max": round(max(ms["stream"]), 4),
                    "baseline_ms_per_frame": round(med["baseline"], 4),
                    "baseline_min": round(min(ms["baseline"]), 4),
                    "baseline_max": round(max(ms["baseline"]), 4),
                    "baseline_over_stream": round(med["baseline"] / med["stream"], 2),
                    "gemm": st.gemm, "first_frame_rel_diff": round(agree, 5)})
            del st
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
