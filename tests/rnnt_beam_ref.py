"""numpy restatement of the transducer beam search contract (include/statecatcher.h,
sc_rnnt_beam_*) -- a helper for the tests, like tests/ctc_beam_ref.py.  Prefixes are tuples, so
prefix identity is exact here (the kernel decides it by hash and length).

Per stream the beam starts as [(empty prefix, 0)]; the empty prefix feeds the predictor `blank`.
For each live frame, with A = [] and C = the beam:

    for r = 0 .. max_symbols:
        every (p, s) of C in order takes a blank: s' = s + lp_p[blank]; a p already in A gets
        lae(its score, s'), else (p, s') is appended to A
        r == max_symbols: stop
        D = every (p + c, s + lp_p[c]) for p of C in order and c over p's top_k non-blank tokens
        (lp descending, ties to the lower index, NaN last); scores of -inf / NaN are dropped
        C = the `beam` largest of D (ties to the earlier candidate), sorted descending; empty: stop
    the beam = the `beam` largest of A without -inf / NaN (ties to the earlier insertion), sorted

where lp_p = log_softmax(W tanh(enc_p[b,t] + pred_tab[last(p)]) + bias).

Every operation is done in ``dtype``: np.float64 for the reference proper, np.float32 to measure
how far a correct fp32 evaluation may drift from it (score_drift).  The fp32 run uses the kernel's
tanh form 1 - 2 / (exp2(2 log2(e) x) + 1) and a plain sequential dot product.
"""
from types import SimpleNamespace

import numpy as np


def rnnt_lp_row(e, p, W, bias, dtype=np.float64):
    """log_softmax(W tanh(e + p) + bias) in ``dtype``: e, p [J], W [V,J], bias [V]."""
    ft = np.dtype(dtype).type
    e, p, W, bias = (np.asarray(a).astype(dtype) for a in (e, p, W, bias))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if dtype == np.float32:
            x = e + p
            z = ft(1.0) - ft(2.0) / (np.exp2(ft(2.0 * 1.4426950408889634) * x) + ft(1.0))
            logit = bias.copy()
            for j in range(W.shape[1]):
                logit = logit + W[:, j] * z[j]
        else:
            logit = (W * np.tanh(e + p)).sum(1) + bias
        m = logit.max()
        return logit - (m + np.log(np.exp(logit - m).sum(dtype=dtype)))


def rnnt_beam_ref(E, P, W, bias, lengths=None, mask=None, blank=0, beam=8, top_k=8, max_symbols=2,
                  dtype=np.float64, max_frames=None):
    """E [B,T,J], P [V,J], W [V,J], bias [V] (any float dtype; computed in ``dtype``).

    Returns a namespace with
      tokens, scores   per stream: the beam's prefixes (lists of ints) and their scores, best first
      frames           per stream, per hypothesis: the live-frame ordinal of each token's emission
                       (of the entry first inserted, where alignments merged)
      status           [B] bit 0: the stream met more than max_frames live frames (the rest ignored)
      cand             per stream, per live frame consumed: the score of every candidate formed --
                       each round's D in order, then A in insertion order; -inf for dropped ones
      topk_margin      smallest lp gap between the top_k-th and the next non-blank token of a row
                       that was expanded
      beam_margin      smallest gap between the beam-th and the next score of a D or A selection
      final_margin     smallest gap between adjacent final scores of a stream
                       (each inf where there is no such pair)
      merges           blank steps folded into an existing entry of A
      per_frame        the set of per-frame emission counts met in the final hypotheses
    """
    ft = np.dtype(dtype).type
    E, P, W, bias = (np.asarray(a) for a in (E, P, W, bias))
    B, T, _ = E.shape
    V = W.shape[0]
    top_k = min(int(top_k), V - 1)
    ninf = ft(-np.inf)
    out = SimpleNamespace(tokens=[], scores=[], frames=[], status=np.zeros(B, np.int32), cand=[],
                          topk_margin=np.inf, beam_margin=np.inf, final_margin=np.inf, merges=0,
                          per_frame=set())
    nb = np.array([v for v in range(V) if v != blank])

    def lae(a, b):
        with np.errstate(invalid="ignore"):
            return ft(np.logaddexp(a, b))

    def select(scores, what):
        """indices of the `beam` largest valid scores, ties to the earlier one, descending"""
        alive = [i for i in range(len(scores)) if scores[i] > ninf]     # NaN is dropped too
        alive.sort(key=lambda i: -scores[i])                             # stable: earlier first
        if len(alive) > beam:
            out.beam_margin = min(out.beam_margin,
                                  float(scores[alive[beam - 1]] - scores[alive[beam]]))
        return alive[:beam]

    for b in range(B):
        hyps = [((), ft(0.0), ())]            # (prefix, score, emission frames)
        n = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
        done, per_stream = 0, []
        for t in range(n):
            if mask is not None and mask[b][t] == 0:
                continue
            if max_frames is not None and done >= max_frames:
                out.status[b] |= 1
                break
            rows = {}

            def row(p):
                u = p[-1] if p else blank
                if u not in rows:
                    rows[u] = rnnt_lp_row(E[b, t], P[u], W, bias, dtype)
                return rows[u]

            A, where, cur, rec = [], {}, hyps, []
            for r in range(max_symbols + 1):
                for p, s, fr in cur:
                    s1 = ft(s + row(p)[blank])
                    if p in where:
                        A[where[p]][1] = lae(A[where[p]][1], s1)
                        out.merges += 1
                    else:
                        where[p] = len(A)
                        A.append([p, s1, fr])
                if r == max_symbols:
                    break
                D = []
                for p, s, fr in cur:
                    lp = row(p)
                    with np.errstate(invalid="ignore"):
                        order = nb[np.argsort(-lp[nb], kind="stable")]   # NaN last, ties: lower
                    if len(order) > top_k and not np.isnan(lp[order[top_k]]):
                        out.topk_margin = min(out.topk_margin,
                                              float(lp[order[top_k - 1]] - lp[order[top_k]]))
                    for c in order[:top_k]:
                        D.append((p + (int(c),), ft(s + lp[c]), fr + (done,)))
                ds = np.array([d[1] for d in D], dtype)
                rec.append(np.where(ds > ninf, ds, ninf))
                cur = [D[i] for i in select(ds, "D")]
                if not cur:
                    break
            sa = np.array([a[1] for a in A], dtype)
            rec.append(np.where(sa > ninf, sa, ninf))
            hyps = [tuple(A[i]) for i in select(sa, "A")]
            per_stream.append(np.concatenate(rec))
            done += 1
        scores = [s for _, s, _ in hyps]
        for a, c in zip(scores, scores[1:]):
            out.final_margin = min(out.final_margin, float(a - c))
        out.tokens.append([list(p) for p, _, _ in hyps])
        out.scores.append([float(s) for s in scores])
        out.frames.append([list(fr) for _, _, fr in hyps])
        for _, _, fr in hyps:
            cnt = np.bincount(np.array(fr, np.int64), minlength=done) if done else np.zeros(0, int)
            out.per_frame |= set(int(c) for c in cnt)
        out.cand.append(per_stream)
    return out


def score_drift(ref_a, ref_b):
    """Largest difference between the candidate scores of two runs of rnnt_beam_ref on one input
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
    if ref_a.tokens != ref_b.tokens:
        return np.inf
    return d


def min_margin(ref):
    return min(ref.topk_margin, ref.beam_margin, ref.final_margin)


def padded_nbest(lists, nbest, cap, fill=-1):
    """(values [B, nbest, cap] int32 truncated to cap and `fill` elsewhere, lens [B, nbest] with -1
    where a stream has fewer hypotheses) of per-stream lists of token (or frame) lists."""
    B = len(lists)
    tok = np.full((B, nbest, cap), fill, np.int32)
    lens = np.full((B, nbest), -1, np.int32)
    for b, hyps in enumerate(lists):
        for n, h in enumerate(hyps[:nbest]):
            lens[b, n] = len(h)
            m = min(len(h), cap)
            tok[b, n, :m] = h[:m]
    return tok, lens


def exact_prefix_scores(lp_of, T, V, blank, max_symbols, max_len):
    """An independent fp64 forward lattice: log P(prefix | x) over every alignment with at most
    max_symbols emissions per frame, for every prefix of at most max_len non-blank tokens.
    lp_of(t, u) is the log-prob row at frame t after last token u (blank for the empty prefix).
    alpha[t][k][m]: log-probability of having emitted the first k tokens, m of them at frame t,
    before frame t's blank."""
    import itertools
    labels = [v for v in range(V) if v != blank]
    res = {}
    for n in range(max_len + 1):
        for y in itertools.product(labels, repeat=n):
            alpha = np.full((T + 1, n + 1), -np.inf)    # at the start of frame t, k tokens emitted
            alpha[0, 0] = 0.0
            for t in range(T):
                a = np.full((n + 1, max_symbols + 1), -np.inf)
                a[:, 0] = alpha[t]
                for m in range(max_symbols):
                    for k in range(n):
                        u = y[k - 1] if k else blank
                        a[k + 1, m + 1] = np.logaddexp(a[k + 1, m + 1], a[k, m] + lp_of(t, u)[y[k]])
                for k in range(n + 1):
                    u = y[k - 1] if k else blank
                    alpha[t + 1, k] = np.logaddexp.reduce(a[k]) + lp_of(t, u)[blank]
            res[y] = float(alpha[T, n])
    return res
