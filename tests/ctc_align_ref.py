"""Numpy restatement of the CTC forced alignment contract (include/statecatcher.h, sc_ctc_align) --
a helper for the tests, like tests/ctc_beam_ref.py.  It takes the float type, so the same code runs
in fp64 (the reference) and in fp32 (how far fp32 arithmetic can drift from it).

Same tie rule (stay, then step, then skip), same per-frame emission shift, re-centring on the
row maximum at EVERY frame (the kernel: at least every 16), the sum of shifts in fp64.

Besides the alignment it returns what the tests' preconditions need:
  margin  the smallest gap between the best and the second-best predecessor over the decisions on
          the returned path, the choice of the final state included (inf where there is no
          second candidate)
  rows    the re-centred lattice rows [T_b][2U+1], for d32
  lp      the log-probabilities [T_b][V], for e32
"""
from types import SimpleNamespace

import numpy as np


def log_probs(x, is_logits, dtype):
    x = np.asarray(x).astype(dtype)
    if not is_logits or x.shape[0] == 0:
        return x
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=dtype)))


def ctc_align_ref(x, targets, blank=0, is_logits=True, dtype=np.float64):
    """One sequence: x [T_b][V] (the values the kernel sees), targets [U] -> SimpleNamespace(
    feasible, states [T_b], labels [T_b], frame_lp [T_b], spans [U][2], token_lp [U], score,
    margin, rows, lp)."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x)
    tg = [int(v) for v in targets]
    T, U, S = x.shape[0], len(tg), 2 * len(tg) + 1
    ninf = dtype(-np.inf)
    lp = log_probs(x, is_logits, dtype)
    ext = np.array([blank if s % 2 == 0 else tg[s // 2] for s in range(S)], np.int64)
    dead = SimpleNamespace(feasible=False, states=np.full(T, -1, np.int32),
                           labels=np.full(T, -1, np.int32), frame_lp=np.zeros(T, dtype),
                           spans=np.full((U, 2), -1, np.int32), token_lp=np.zeros(U, dtype),
                           score=-np.inf, margin=np.inf, rows=np.zeros((T, S), dtype), lp=lp)
    if T == 0:
        if U == 0:
            dead.feasible, dead.score = True, 0.0
        return dead
    can_skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        can_skip[s] = ext[s] != ext[s - 2]
    e = lp[:, ext]                                   # [T][S]
    c = e.max(1)                                     # the frame's shift
    c = np.where(np.isfinite(c), c, dtype(0))
    es = e - c[:, None]
    v = np.full(S, ninf, dtype)
    v[0] = es[0, 0]
    if U:
        v[1] = es[0, 1]
    shift = 0.0
    dec = np.zeros((T, S), np.int8)
    gap = np.full((T, S), np.inf)
    rows = np.empty((T, S), dtype)

    def recentre(v):
        m = v.max()
        if np.isfinite(m):
            with np.errstate(invalid="ignore"):
                return v - m, float(m)
        return v, 0.0

    v, m = recentre(v)
    shift += m + float(c[0])
    rows[0] = v
    for t in range(1, T):
        step = np.concatenate(([ninf], v))[:S]
        skp = np.where(can_skip, np.concatenate(([ninf, ninf], v))[:S], ninf)
        cand = np.stack([v, step, skp])              # argmax: the first maximum = the smaller move
        d = cand.argmax(0)
        srt = np.sort(cand.astype(np.float64), 0)
        with np.errstate(invalid="ignore"):
            g = srt[2] - srt[1]
        gap[t] = np.where(np.isnan(g), np.inf, g)
        dec[t] = d
        v = es[t] + cand[d, np.arange(S)]
        v, m = recentre(v)
        shift += m + float(c[t])
        rows[t] = v
    end, fgap = S - 1, np.inf
    if U:
        a, b = v[S - 1], v[S - 2]
        if b > a:
            end = S - 2
        if np.isfinite(a) and np.isfinite(b):
            fgap = abs(float(a) - float(b))
    dead.rows = rows
    if not v[end] > ninf:
        return dead
    states = np.empty(T, np.int32)
    s, margin = end, fgap
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t:
            margin = min(margin, gap[t, s])
            s -= int(dec[t, s])
    assert s in (0, 1) and (U or s == 0)
    frame_lp = lp[np.arange(T), ext[states]]
    spans = np.full((U, 2), -1, np.int32)
    token_lp = np.zeros(U, dtype)
    for u in range(U):
        (idx,) = np.nonzero(states == 2 * u + 1)
        assert len(idx) and (np.diff(idx) == 1).all()
        spans[u] = idx[0], idx[-1] + 1
        acc = dtype(0)
        for t in idx:                                # frame order, in the float type
            acc = dtype(acc + frame_lp[t])
        token_lp[u] = acc / dtype(len(idx))
    return SimpleNamespace(feasible=True, states=states, labels=ext[states].astype(np.int32),
                           frame_lp=frame_lp, spans=spans, token_lp=token_lp,
                           score=float(v[end]) + shift, margin=float(margin), rows=rows, lp=lp)


def drift(ref64, ref32):
    """(d32, e32) of one sequence: the largest difference between the fp64 and the fp32 re-centred
    rows over entries within 200 of their row's maximum (0 after re-centring), and between the
    fp64 and the fp32 log-probabilities."""
    near = ref64.rows > -200
    with np.errstate(invalid="ignore"):
        dr = np.abs(ref64.rows - ref32.rows.astype(np.float64))
        de = np.abs(ref64.lp - ref32.lp.astype(np.float64))
    d32 = float(np.nanmax(np.where(near, dr, 0.0), initial=0.0))
    e32 = float(np.nanmax(np.where(np.isfinite(ref64.lp), de, 0.0), initial=0.0))
    return d32, e32


def min_feasible_len(targets):
    """The shortest T_b a transcript aligns to: U + the number of adjacent equal labels."""
    tg = list(targets)
    return len(tg) + sum(1 for a, b in zip(tg, tg[1:]) if a == b)


def brute_force(lp, targets, blank=0):
    """Every alignment of `targets` to the T rows of lp [T][V], enumerated: -> (best score, the
    set of state paths that reach it) or (-inf, empty)."""
    tg = [int(v) for v in targets]
    T, S = lp.shape[0], 2 * len(tg) + 1
    ext = [blank if s % 2 == 0 else tg[s // 2] for s in range(S)]
    best, arg = -np.inf, []

    def walk(t, s, score, path):
        nonlocal best, arg
        score = score + lp[t, ext[s]]
        path = path + [s]
        if t == T - 1:
            if s in (S - 1, S - 2) or S == 1:
                if score > best:
                    best, arg = score, [path]
                elif score == best:
                    arg.append(path)
            return
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and (n % 2 == 0 or ext[n] == ext[s])):
                continue
            walk(t + 1, n, score, path)

    if T:
        for s0 in range(min(2, S)):
            walk(0, s0, 0.0, [])
    elif not tg:
        best, arg = 0.0, [[]]
    return best, arg


def tie_rule_path(paths):
    """Of several best paths the contract's tie rule returns: the final tie goes to the higher
    state and, walking back, every tie goes to the smaller move (the higher predecessor) -- the
    path whose reversed state sequence is the largest."""
    return max(paths, key=lambda p: p[::-1])


def tie_cases(n=32, T=8, V=4, umax=3, seed=0):
    """n small sequences of integer-valued log-probs in [-3, 0] (fp32 sums of them are exact, so
    ties are exact ties): (x [n][T][V], targets [n][umax], in_lens [n], tgt_lens [n]).  Labels are
    1 .. V-1, blank 0; lengths vary, infeasible pairs included."""
    rng = np.random.default_rng(seed)
    x = -rng.integers(0, 4, (n, T, V)).astype(np.float64)
    targets = rng.integers(1, V, (n, umax))
    in_lens = rng.integers(1, T + 1, n)
    tgt_lens = rng.integers(0, umax + 1, n)
    return x, targets, in_lens, tgt_lens
