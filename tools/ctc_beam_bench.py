#!/usr/bin/env python3
"""CTC prefix beam search time on one GPU at C2's decode size (B=32, T=1500, V=1024, bf16 logits).

Seeded logits (scale * N(0,1), + blank-bias * scale on the blank so that most frames are blank,
ragged lengths) are decoded by
  * ops.ctc_beam_decode offline (a fresh state, reset, pre-pass + beam walk, result: what
    decoder.ctc_beam_decoder runs before its one host copy) for (beam, top_k) = (8, 8) and
    (32, 32);
  * the same on a state made once (reset + frames + result, no allocation): the chunked form;
  * the pre-pass alone: the same call on a state with room for no frame, whose walk returns at
    its first live frame (reported with the logits' bytes over its time);
  * ops.ctc_beam_result alone on the decoded state (one lane per hypothesis follows its parent
    pointers: its time grows with the hypotheses' length);
  * ops.ctc_greedy_decode on the same tensor.
Each is timed with device events around one call, median of --reps calls after --warmup calls.

Prints one JSON object per measurement and, with --out, writes them to a JSON file.

usage: python tools/ctc_beam_bench.py [--out profiles/ctc_beam_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--blank-bias", type=float, default=4.0, help="in units of --scale")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench: needs a ROCm GPU (a CPU timing says nothing here)")
    from statecatcher_amd import ops
    dev = torch.device("cuda:0")
    B, T, V = args.batch, args.frames, args.vocab
    rng = np.random.default_rng(0)
    x = (args.scale * rng.standard_normal((B, T, V))).astype(np.float32)
    x[:, :, 0] += args.blank_bias * args.scale
    lens = np.full(B, T, np.int64)
    lens[1::2] -= rng.integers(0, T // 10, size=len(lens[1::2]))   # ragged, as a real batch
    xd = torch.as_tensor(x).to(dev, torch.bfloat16)
    ld = torch.as_tensor(lens).to(dev)
    shape = dict(B=B, T=T, V=V, dtype="bf16", live_frames=int(lens.sum()),
                 logits_bytes=int(lens.sum()) * V * 2)
    print(json.dumps({"shape": shape}), flush=True)
    rows = [{"shape": shape}]

    def report(impl, us, **extra):
        med = statistics.median(us)
        row = {"impl": impl, "us_per_call": round(med, 1), "us_min": round(min(us), 1),
               "us_max": round(max(us), 1), "reps": len(us), **extra}
        print(json.dumps(row), flush=True)
        rows.append(row)
        return med

    greedy = report("ctc_greedy_decode", event_times(lambda: ops.ctc_greedy_decode(xd, ld),
                                                     args.reps, args.warmup))
    for beam, top_k in ((8, 8), (32, 32)):
        kw = dict(lengths=ld, top_k=top_k, nbest=1, is_logits=True)
        off = lambda: ops.ctc_beam_decode(xd, beam=beam, **kw)   # noqa: E731
        tok, ln, sc = off()
        mean_len = float(ln[:, 0].double().mean())
        us = event_times(off, args.reps, args.warmup)
        med = statistics.median(us)
        report("ctc_beam_decode_offline", us, beam=beam, top_k=top_k,
               tokens_per_stream=round(mean_len, 1),
               us_per_frame_of_the_longest_stream=round(med / int(lens.max()), 3),
               ratio_to_ctc_greedy_decode=round(med / greedy, 1))
        st = ops.ctc_beam_state(B, beam, T, dev)
        out = (torch.full((B, 1, T), -1, dtype=torch.int32, device=dev),
               torch.empty(B, 1, dtype=torch.int32, device=dev),
               torch.empty(B, 1, dtype=torch.float32, device=dev))

        def steady():
            st.reset()
            ops.ctc_beam_decode(xd, state=st, out=out, **kw)

        steady()
        assert torch.equal(out[1], ln) and torch.equal(out[2], sc)
        report("ctc_beam_state_reset_frames_result", event_times(steady, args.reps, args.warmup),
               beam=beam, top_k=top_k)
        none = ops.ctc_beam_state(B, beam, 0, dev)
        pre = lambda: ops.ctc_beam_decode(xd, state=none, cap=0, **kw)   # noqa: E731
        us = event_times(pre, args.reps, args.warmup)
        report("ctc_beam_prepass_and_empty_walk", us, beam=beam, top_k=top_k,
               logits_GB_per_s=round(shape["logits_bytes"] / statistics.median(us) / 1e3, 1))
        res = lambda: ops.ctc_beam_result(st, 1, out=out)   # noqa: E731
        report("ctc_beam_result", event_times(res, args.reps, args.warmup), beam=beam, top_k=top_k,
               nbest=1, tokens_per_stream=round(mean_len, 1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
