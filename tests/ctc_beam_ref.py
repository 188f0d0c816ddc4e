"""numpy restatement of the CTC prefix beam search contract (include/statecatcher.h,
sc_ctc_beam_*) -- a helper for the tests, like tests/rnnt_decode_ref.py.  Prefixes are tuples, so
prefix identity is exact here (the kernel decides it by hash and length).

Per stream the beam starts as [(empty prefix, pb = 0, pnb = -inf)].  For each live frame:
lp = x - logsumexp(x) (is_logits) or x; the frame's tokens are the top_k non-blank v by lp (ties
to the lower index, NaN last); stay candidates in beam order, then extension candidates in
(beam rank, top_k rank) order, an extension that spells an existing beam entry being folded into
that entry's stay candidate as pnb' = lae(repeat term, extension term); candidates whose total is
-inf (or NaN) are dropped; the `beam` largest totals (ties to the earlier candidate), sorted by
total descending, are the new beam.

Every operation is done in ``dtype`` (np.float64 for the reference proper, np.float32 to measure
how far a correct fp32 evaluation may drift from it: score_drift).
"""
from types import SimpleNamespace

import numpy as np


def ctc_beam_ref(x, lengths=None, mask=None, blank=0, beam=8, top_k=8, is_logits=False,
                 dtype=np.float64, max_frames=None):
    """x [B,T,V] (any float dtype; computed in ``dtype``).

    Returns a namespace with
      tokens, scores   per stream: the beam's prefixes (lists of ints) and lae(pb, pnb), best first
      status           [B] bit 0: the stream met more than max_frames live frames (the rest ignored)
      cand             per stream, per live frame consumed: the total of every candidate (stays,
                       then the extensions that were not folded into one), -inf for dropped ones
      topk_margin      smallest lp gap between the top_k-th and the next non-blank token of a frame
      beam_margin      smallest gap between the beam-th and the next candidate total of a frame
      final_margin     smallest gap between adjacent final scores of a stream
                       (each inf where there is no such pair)
      merges           extensions folded into an existing beam entry (step 4)
      repeats          stay candidates whose repeat term pnb + lp[last] was taken (step 3)
    """
    ft = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    B, T, V = x.shape
    ninf = ft(-np.inf)
    out = SimpleNamespace(tokens=[], scores=[], status=np.zeros(B, np.int32), cand=[],
                          topk_margin=np.inf, beam_margin=np.inf, final_margin=np.inf, merges=0,
                          repeats=0)

    def lae(a, b):
        with np.errstate(invalid="ignore"):
            return ft(np.logaddexp(a, b))

    for b in range(B):
        hyps = [((), ft(0.0), ninf)]
        n = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
        done, frames = 0, []
        for t in range(n):
            if mask is not None and mask[b][t] == 0:
                continue
            if max_frames is not None and done >= max_frames:
                out.status[b] |= 1
                break
            row = x[b, t]
            if is_logits:
                m = row.max()
                with np.errstate(invalid="ignore", divide="ignore"):
                    lp = row - (m + np.log(np.exp(row - m).sum(dtype=dtype)))
            else:
                lp = row
            nb = np.array([v for v in range(V) if v != blank])
            with np.errstate(invalid="ignore"):
                order = nb[np.argsort(-lp[nb], kind="stable")]   # NaN last, ties: lower index
            top = [int(v) for v in order[:top_k]]
            if len(order) > top_k and not np.isnan(lp[order[top_k]]):
                out.topk_margin = min(out.topk_margin, float(lp[order[top_k - 1]] - lp[order[top_k]]))
            index = {p: i for i, (p, _, _) in enumerate(hyps)}
            tots = [lae(pb, pnb) for _, pb, pnb in hyps]
            stays = []
            for (p, pb, pnb), tot in zip(hyps, tots):
                rep = ninf
                if p and p[-1] in top:
                    rep = ft(pnb + lp[p[-1]])
                    out.repeats += 1
                stays.append([p, ft(tot + lp[blank]), rep])
            exts = []
            for (p, pb, pnb), tot in zip(hyps, tots):
                for c in top:
                    e_pnb = ft((pb if p and c == p[-1] else tot) + lp[c])
                    q = p + (c,)
                    if q in index:
                        stays[index[q]][2] = lae(stays[index[q]][2], e_pnb)
                        out.merges += 1
                    else:
                        exts.append([q, ninf, e_pnb])
            cands = stays + exts
            total = np.array([lae(c[1], c[2]) for c in cands], dtype)
            alive = [i for i in range(len(cands)) if total[i] > ninf]     # NaN is dropped too
            alive.sort(key=lambda i: -total[i])                            # stable: earlier first
            if len(alive) > beam:
                out.beam_margin = min(out.beam_margin,
                                      float(total[alive[beam - 1]] - total[alive[beam]]))
            hyps = [tuple(cands[i]) for i in alive[:beam]]
            frames.append(np.where(total > ninf, total, ninf))
            done += 1
        scores = [lae(pb, pnb) for _, pb, pnb in hyps]
        for a, c in zip(scores, scores[1:]):
            out.final_margin = min(out.final_margin, float(a - c))
        out.tokens.append([list(p) for p, _, _ in hyps])
        out.scores.append([float(s) for s in scores])
        out.cand.append(frames)
    return out


def score_drift(ref_a, ref_b):
    """Largest difference between the candidate scores of two runs of ctc_beam_ref on one input
    (fp64 and fp32): inf when the two runs did not form the same candidates."""
    d = 0.0
    for fa, fb in zip(ref_a.cand, ref_b.cand):
        if len(fa) != len(fb):
            return np.inf
        for a, c in zip(fa, fb):
            a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
            if a.shape != c.shape or (np.isfinite(a) != np.isfinite(c)).any():
                return np.inf
            ok = np.isfinite(a)
            if ok.any():
                d = max(d, float(np.abs(a[ok] - c[ok]).max()))
    return d


def min_margin(ref):
    return min(ref.topk_margin, ref.beam_margin, ref.final_margin)


def padded_nbest(tokens, nbest, cap, fill=-1):
    """(tokens [B, nbest, cap] int32 truncated to cap and `fill` elsewhere, lens [B, nbest] with -1
    where a stream has fewer hypotheses) of per-stream lists of token lists."""
    B = len(tokens)
    tok = np.full((B, nbest, cap), fill, np.int32)
    lens = np.full((B, nbest), -1, np.int32)
    for b, hyps in enumerate(tokens):
        for n, h in enumerate(hyps[:nbest]):
            lens[b, n] = len(h)
            m = min(len(h), cap)
            tok[b, n, :m] = h[:m]
    return tok, lens
