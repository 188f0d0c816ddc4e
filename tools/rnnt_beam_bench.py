#!/usr/bin/env python3
"""Transducer beam search time on one GPU at the C5 shape (B=32, T=1500, V=1024, J=64).

The inputs are tools/rnnt_decode_bench.py's (seeded; the blank bias calibrated so that the greedy
path emits about one token per ten frames).  On the same device tensors the tool times
  * ops.rnnt_beam_decode (csrc/rnnt_beam.hip, the register-resident fast path, fp32) for
    (beam, top_k, max_symbols) = (8, 8, 1), (8, 8, 2) and (32, 32, 2): a chunk call on a reset
    state with static outputs (reset + walk + result launches), device events, median and range
    over --reps calls after --warmup calls;
  * ops.rnnt_greedy_decode, the same way;
  * the loop a user would write in PyTorch without the kernel, for (8, 8, 2): all streams and
    hypotheses in lock step, per round a gather, tanh, matmul, log_softmax and two topk on the
    device, the merge into A on the host, two host syncs per round.  It runs over the first
    --loop-frames frames only (host clock, median over --loop-reps) and is compared
    with the kernel on the same frames; its best hypotheses are compared with the kernel's.

Prints one JSON object per measurement and, with --out, writes them to a JSON file.

usage: python tools/rnnt_beam_bench.py [--out profiles/rnnt_beam_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CONFIGS = ((8, 8, 1), (8, 8, 2), (32, 32, 2))


@torch.no_grad()
def torch_beam_loop(E, P, W, bias, frames, blank, beam, top_k, ms):
    """The contract of include/statecatcher.h (sc_rnnt_beam_*) as a batched PyTorch loop with the
    merge on the host.  Returns per stream the beam as a list of (prefix tuple, score)."""
    B, dev = E.shape[0], E.device
    Wt = W.t()
    hyps = [[((), 0.0)] for _ in range(B)]
    ninf = float("-inf")
    for t in range(frames):
        A = [dict() for _ in range(B)]
        cur = hyps
        for r in range(ms + 1):
            n = max(len(c) for c in cur)
            if n == 0:
                break
            last = torch.tensor([[(p[-1] if p else blank) for p, _ in c] + [blank] * (n - len(c))
                                 for c in cur], device=dev)
            sc = torch.tensor([[s for _, s in c] + [ninf] * (n - len(c)) for c in cur], device=dev)
            z = torch.tanh(E[:, t, None, :] + P[last])
            lp = torch.log_softmax(torch.matmul(z, Wt) + bias, -1)          # [B, n, V]
            stay = (sc + lp[..., blank]).tolist()                           # host sync
            for b in range(B):
                for (p, _), s in zip(cur[b], stay[b]):
                    if p in A[b]:
                        m = max(A[b][p], s)
                        A[b][p] = m + torch.log1p(torch.exp(torch.tensor(-abs(A[b][p] - s)))).item() \
                            if m > ninf else m
                    else:
                        A[b][p] = s
            if r == ms:
                break
            lp[..., blank] = ninf
            tv, ti = lp.topk(top_k, -1)                                     # [B, n, K]
            cand = (sc[..., None] + tv).view(B, n * top_k)
            bv, bi = cand.topk(min(beam, n * top_k), -1)
            bv, bi, ti = bv.tolist(), bi.tolist(), ti.view(B, n * top_k).tolist()   # host sync
            cur = [[(cur[b][i // top_k][0] + (ti[b][i],), v) for v, i in zip(bv[b], bi[b])
                    if v > ninf] for b in range(B)]
        hyps = [sorted(((p, s) for p, s in A[b].items() if s > ninf), key=lambda e: -e[1])[:beam]
                for b in range(B)]
    return hyps


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
    ap.add_argument("--vocab", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=150, help="greedy emissions per stream to aim for")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=100)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--configs", default=None,
                    help="beam,top_k,max_symbols triples to time instead of the three of the report, "
                         "e.g. '1,1,2 8,1,2' (no PyTorch loop then)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_beam_bench: needs a ROCm GPU (a CPU timing says nothing here)")
    from rnnt_decode_bench import make_inputs
    from statecatcher_amd import ops
    dev = torch.device("cuda:0")
    B, T, V, J = args.batch, args.frames, args.vocab, 64
    E, P, W, bias, lens = make_inputs(B, T, V, J, args.tokens, 4)
    Ed, Pd, Wd, bias_d = (torch.as_tensor(a).to(dev) for a in (E, P, W, bias))
    lens_d = torch.as_tensor(lens).to(dev)
    live = int(lens.sum())
    shape = dict(B=B, T=T, V=V, J=J, live_frames=live, dtype="fp32")
    print(json.dumps({"shape": shape}), flush=True)
    rows = [{"shape": shape}]

    def stats(us, extra):
        row = dict(extra, us_per_call=round(statistics.median(us), 1), us_min=round(min(us), 1),
                   us_max=round(max(us), 1), reps=len(us))
        print(json.dumps(row), flush=True)
        rows.append(row)
        return row

    tok = torch.full((B, T * 4), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    us = event_times(lambda: ops.rnnt_greedy_decode(Ed, Pd, Wd, bias_d, lengths=lens_d,
                                                    max_symbols=4, out=(tok, cnt, None)),
                     args.reps, args.warmup)
    greedy = stats(us, {"impl": "hip_greedy_fp32", "max_symbols": 4,
                        "tokens_per_stream": round(float(cnt.double().mean()), 1)})

    states = {}
    configs = CONFIGS if args.configs is None else tuple(
        tuple(int(x) for x in c.split(",")) for c in args.configs.split())
    for beam, top_k, ms in configs:
        st = ops.rnnt_beam_state(B, beam, ms, T, dev)
        states[beam, top_k, ms] = st
        out = (torch.full((B, 1, T * ms), -1, dtype=torch.int32, device=dev),
               torch.zeros(B, 1, dtype=torch.int32, device=dev),
               torch.zeros(B, 1, dtype=torch.float32, device=dev))

        def run(st=st, out=out, top_k=top_k):
            st.reset()
            ops.rnnt_beam_decode(Ed, Pd, Wd, bias_d, lengths=lens_d, top_k=top_k, state=st, out=out)

        us = event_times(run, args.reps, args.warmup)
        med = statistics.median(us)
        same = sum(int(out[1][b, 0]) == int(cnt[b]) and torch.equal(out[0][b, 0, :int(cnt[b])],
                                                                  tok[b, :int(cnt[b])])
                   for b in range(B))
        stats(us, {"impl": "hip_beam_fp32", "beam": beam, "top_k": top_k, "max_symbols": ms,
                   "us_per_frame": round(med / T, 2), "us_per_round": round(med / T / (ms + 1), 2),
                   "state_bytes": st.nbytes, "ratio_to_greedy": round(med / greedy["us_per_call"], 1),
                   "best_equals_greedy_streams": same,
                   "tokens_per_stream": round(float(out[1].double().mean()), 1)})

    if args.configs is not None:
        return
    # the PyTorch loop, (8, 8, 2), on the first frames only; the kernel on the same frames
    beam, top_k, ms = CONFIGS[1]
    F = min(args.loop_frames, T, int(lens.min()))
    st = states[beam, top_k, ms]
    out = (torch.full((B, beam, F * ms), -1, dtype=torch.int32, device=dev),
           torch.zeros(B, beam, dtype=torch.int32, device=dev),
           torch.zeros(B, beam, dtype=torch.float32, device=dev))

    def run_f():
        st.reset()
        ops.rnnt_beam_decode(Ed[:, :F], Pd, Wd, bias_d, top_k=top_k, nbest=beam, state=st, out=out)

    kernel_f = statistics.median(event_times(run_f, args.reps, args.warmup))
    loop = lambda: torch_beam_loop(Ed, Pd, Wd, bias_d, F, 0, beam, top_k, ms)   # noqa: E731
    hyps = loop()   # warm-up
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.loop_reps):
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    ln, tk = out[1].cpu(), out[0].cpu()
    agree = sum(bool(hyps[b]) and list(hyps[b][0][0]) == tk[b, 0, :max(int(ln[b, 0]), 0)].tolist()
                for b in range(B))
    med = statistics.median(wall)
    stats(wall, {"impl": "torch_lockstep_beam_loop_fp32", "beam": beam, "top_k": top_k,
                 "max_symbols": ms, "frames": F, "us_per_frame": round(med / F, 1),
                 "hip_us_same_frames": round(kernel_f, 1),
                 "ratio_to_hip_same_frames": round(med / kernel_f, 1),
                 "best_equals_hip_streams": agree})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
