#!/usr/bin/env python3
"""Streaming decode of the xLSTM encoder (config C4) on one GPU: statecatcher_amd.StreamingXLSTM.

C4: 12 blocks x 768, 4 heads (DQ 96, DV 192), 80-d input, V = 1024.  Sweep: concurrent streams
x frames per call K x weight dtype x hipGraph / eager x GEMM engine.  One JSON line per
configuration:
  ms_per_frame          wall time of one block / K
  stream_frames_per_s   streams x frames / s
  launches_per_block    kernel launches of one block (counted on an eager run by the profiler;
                        null when the profiler is unavailable).  A graph replays them as one
                        host launch.
  state_bytes_per_frame 2 |state| / K: the mLSTM state (C, n, m of every block and stream, fp32)
                        is read once and written once per block
  state_traffic_share   that traffic at --hbm-gbs (default 8000, the MI355X's HBM3E peak) as a
                        fraction of the measured block time
  baseline_*            what a user had before: xLSTMLarge.forward on 64-frame chunks with
                        carried state + ctc_greedy_decode under no_grad (bf16: under autocast),
                        same process: ms per frame AND ms per call -- a chunk is its latency floor.

--kernel: the step kernel alone at C4's head size instead (us per call, state GB/s).

usage: python tools/xlstm_stream_bench.py [--kernel] [--frames 64] [--streams 1,16,64] [--ks 1,8]
           [--dtypes float32,bfloat16] [--gemms frame,library] [--blocks 12] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F_IN, V = 80, 1024


def timed(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def count_launches(st):
    """Kernel launches of one eager block (the stream's state is put back afterwards)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        saved, prev = st.state(), st.prev.clone()
        st._block()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st._block()
            torch.cuda.synchronize()
        st.reset(saved)
        st.prev.copy_(prev)
        n = sum(1 for e in prof.events()
                if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())
        return n or None
    except Exception as e:   # the count is a report field, not a result
        print(f"# launch count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def baseline(model, B, dt, chunks=4):
    """(seconds per 64-frame call) of xLSTMLarge.forward with carried state + greedy decode."""
    import statecatcher_amd as sc
    dev = next(model.parameters()).device
    x = torch.randn(B, 64, F_IN, device=dev)
    lens = torch.full((B,), 64, dtype=torch.int64, device=dev)
    state = [None]

    @torch.no_grad()
    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            lg, state[0] = model(x, state[0])
        sc.ctc_greedy_decode(lg.float(), lens)
    return timed(run, chunks)


def kernel_sweep(args):
    """The step kernel alone at C4's head size (NH 4, DQ 96, DV 192): us per call and the state
    traffic it sustains (2 |state| per call), per streams x K x operand dtype."""
    from statecatcher_amd import ops
    dev = torch.device("cuda:0")
    NH, DQ, DV = 4, 96, 192
    lines = []
    for B in [int(b) for b in args.streams.split(",")]:
        for dname in args.dtypes.split(","):
            dt = getattr(torch, dname)
            for K in [int(k) for k in args.ks.split(",")]:
                q, k = (torch.randn(B, NH, K, DQ, device=dev).to(dt) for _ in range(2))
                v = torch.randn(B, NH, K, DV, device=dev).to(dt)
                ig, fg = torch.randn(B, NH, K, device=dev), torch.randn(B, NH, K, device=dev) + 3
                st = [torch.zeros(B, NH, DQ, DV, device=dev), torch.zeros(B, NH, DQ, device=dev),
                      torch.zeros(B, NH, 1, device=dev)]
                ops.mlstm_step(q, k, v, ig, fg, *st)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()   # 10 calls per replay: device time, not host time
                with torch.cuda.graph(g):
                    for _ in range(10):
                        ops.mlstm_step(q, k, v, ig, fg, *st)
                sec = timed(g.replay, 20, warm=3) / 10
                nbytes = 2 * sum(t.numel() * 4 for t in st)
                lines.append({"impl": "sc_mlstm_step", "dtype": dname, "streams": B, "K": K,
                              "us_per_call": round(1e6 * sec, 2),
                              "state_gb_per_s": round(nbytes / sec / 1e9, 1),
                              "state_traffic_share": round(nbytes / (args.hbm_gbs * 1e9) / sec, 4)})
                print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true",
                    help="time the step kernel alone (10 calls per hipGraph replay)")
    ap.add_argument("--frames", type=int, default=64, help="frames per stream per measurement")
    ap.add_argument("--streams", default="1,16,64")
    ap.add_argument("--ks", default="1,8")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--gemms", default="frame,library")
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None, help="also write the lines to this JSON file")
    args = ap.parse_args()
    import statecatcher_amd as sc
    from statecatcher_amd.model import build_xlstm_config
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.kernel:
        lines = kernel_sweep(args)
        return write_out(args, lines)
    cfg = build_xlstm_config(F_IN, V, num_heads=4, num_blocks=args.blocks, embedding_dim=768,
                             autocast_kernel_dtype="bfloat16")
    model = sc.xLSTMLarge(cfg).to(dev).eval()
    lines = []
    for B in [int(b) for b in args.streams.split(",")]:
        for dname in args.dtypes.split(","):
            dt = getattr(torch, dname)
            base = baseline(model, B, dt)
            for K in [int(k) for k in args.ks.split(",")]:
                x = torch.randn(B, K, F_IN, device=dev)
                for gemm in args.gemms.split(","):
                    launches = None
                    for graph in (True, False):
                        st = sc.StreamingXLSTM(model, batch=B, frames_per_call=K, dtype=dt,
                                               graph=graph, gemm=gemm)
                        if not graph:
                            launches = count_launches(st)
                        sec = timed(lambda: st.step(x), max(1, args.frames // K))
                        state_b = sum(t.numel() * 4 for s in st.states.values() for t in s)
                        lines.append({
                            "impl": f"hip_xlstm_step_{gemm}" + ("_graph" if graph else "_eager"),
                            "dtype": dname, "streams": B, "K": K, "blocks": args.blocks,
                            "ms_per_frame": round(1e3 * sec / K, 4),
                            "stream_frames_per_s": round(B * K / sec, 1),
                            "launches_per_block": launches,
                            "state_bytes_per_frame": 2 * state_b // K,
                            "state_traffic_share": round(2 * state_b / (args.hbm_gbs * 1e9) / sec, 4),
                            "baseline_ms_per_frame": round(1e3 * base / 64, 4),
                            "baseline_ms_per_call": round(1e3 * base, 3)})
                        del st
                    # (the eager run counted the launches: both lines of the pair carry them)
                    lines[-2]["launches_per_block"] = launches
                    for ln in lines[-2:]:
                        print(json.dumps(ln), flush=True)
    write_out(args, lines)


def write_out(args, lines):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"command": "python tools/xlstm_stream_bench.py " + " ".join(sys.argv[1:]),
                       "device": torch.cuda.get_device_name(0), "results": lines}, f, indent=1)


if __name__ == "__main__":
    main()
