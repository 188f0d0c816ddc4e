"""fp64 numpy restatement of the greedy transducer decode contract (include/statecatcher.h,
sc_rnnt_greedy_decode) -- a helper for the tests, like tests/torch_ref.py.

Per stream b, u = prev[b] (blank when prev is None), for each live frame t in order, at most
max_symbols times: z = tanh(E[b,t] + P[u]); logit = W z + bias; k = argmax (first maximal index,
a NaN counting as maximal); k == blank -> next frame; else emit k at frame t, u = k.
"""
from types import SimpleNamespace

import numpy as np


def argmax_beats(x):
    """csrc/decode.hip's `beats`: the first NaN if there is one, else the first maximum."""
    nan = np.isnan(x)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(x))


def rnnt_greedy_ref(E, P, W, bias, lengths=None, mask=None, blank=0, max_symbols=4, prev=None,
                    gap_exclude=()):
    """E [B,T,J], P [V,J], W [V,J], bias [V] (any float dtype; computed in fp64).

    Returns a namespace with
      tokens, frames   per-stream lists of the emitted tokens and their frame indices
      counts           [B] number of emissions
      prev             [B] last emitted token at exit (the entry value if nothing was emitted)
      min_gap          smallest top-1 minus top-2 logit over every node visited (inf if none; a
                       node with a NaN logit is skipped; rows in gap_exclude do not count as
                       runner-up -- for inputs with deliberately duplicated rows)
      per_frame        per-stream lists: emissions at each live frame, in frame order
      path             per-stream lists of (t, emitted_before, k): every node visited and its
                       decision
      evals            total number of joint evaluations (sum_b live frames + emissions, minus
                       the frames that ended on max_symbols)
    """
    E, P, W, bias = (np.asarray(a, np.float64) for a in (E, P, W, bias))
    B, T, _ = E.shape
    keep = np.ones(W.shape[0], bool)
    keep[list(gap_exclude)] = False
    out = SimpleNamespace(tokens=[], frames=[], counts=np.zeros(B, np.int32),
                          prev=np.zeros(B, np.int32), min_gap=np.inf, per_frame=[], path=[],
                          evals=0)
    for b in range(B):
        u = blank if prev is None else int(prev[b])
        if not 0 <= u < W.shape[0]:
            u = blank
        n = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
        toks, frs, per, path = [], [], [], []
        for t in range(n):
            if mask is not None and mask[b][t] == 0:
                continue
            emitted = 0
            for _ in range(max_symbols):
                # row by row in one order: identical rows give identical logits (BLAS need not)
                logit = (W * np.tanh(E[b, t] + P[u])).sum(1) + bias
                out.evals += 1
                k = argmax_beats(logit)
                if not np.isnan(logit).any():
                    rest = keep.copy()
                    rest[k] = False
                    if rest.any():
                        out.min_gap = min(out.min_gap, float(logit[k] - logit[rest].max()))
                path.append((t, len(toks), k))
                if k == blank:
                    break
                toks.append(k)
                frs.append(t)
                emitted += 1
                u = k
            per.append(emitted)
        out.tokens.append(toks)
        out.frames.append(frs)
        out.counts[b] = len(toks)
        out.prev[b] = u
        out.per_frame.append(per)
        out.path.append(path)
    return out


def padded(lists, cap, fill=-1):
    """[B, cap] int32 of per-stream lists truncated to cap, `fill` elsewhere."""
    a = np.full((len(lists), cap), fill, np.int32)
    for b, row in enumerate(lists):
        m = min(len(row), cap)
        a[b, :m] = row[:m]
    return a
