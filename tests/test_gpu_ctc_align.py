"""GPU tests of the CTC forced alignment (csrc/ctc_align.hip) through every layer: the ctypes op
ops.ctc_align, the dispatcher op and decoder.ctc_forced_align.

The reference is the numpy restatement tests/ctc_align_ref.py in fp64 (pinned against enumeration
of every alignment in tests/test_ctc_align_host.py).  states, labels and spans must equal it
exactly; frame_lp and token_lp within 8 * e32 + 2^-22 |value| and score within 8 * e32 * T_b +
1e-6 |score|, where e32 is the largest difference between the reference's fp64 and fp32
log-probabilities on the same input (the factor 8 covers an fp32 summation order other than
numpy's, as in tests/test_gpu_ctc_beam.py).  An exact path is a fair demand because every parity
test first asserts, on the CPU, a condition on its INPUT: the smallest gap between the best and the
second-best predecessor over the decisions on the reference's path (the final choice included) is
at least max(1e-3, 100 * d32), d32 being how far the reference's own fp32 lattice rows drift from
its fp64 ones; the reference's fp32 path equals its fp64 path; and the targets hold an adjacent
repeat.  The seed of each (case, use) is the first for which that holds.  Each case is
milliseconds of GPU work.
"""
import functools

import numpy as np
import pytest
import torch

from tests.ctc_align_ref import ctc_align_ref, drift, min_feasible_len, tie_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
B = 3

# name: (T, V, U, scale, in_lens or None = (T, T - 7, T // 2)); the kernel's block sizes a case
# straddles are named: kAlNorm = 16 frames between halo exchanges and re-centrings (and per
# emission prefetch buffer), 8 frames per decision word, kAlBt = 64 frames per backtrace block
CASES = {
    "v37": (40, 37, 9, 2.0, None),            # V not a multiple of 64
    "repeats": (30, 5, 12, 2.0, None),        # many repeats, U near T
    "v1030": (96, 1030, 40, 3.0, None),       # V not a multiple of the load width; two waves
    "halo2": (160, 64, 70, 2.0, None),        # halo exchange between two waves
    "halo3": (300, 128, 140, 2.0, None),      # ... between three
    "widest": (1100, 32, 1007, 2.0, None),    # the widest lattice: 16 waves, one frame per exchange
    "k16_full": (830, 32, 767, 2.0, None),    # the last U_max of the K = 16 walk: 16 full waves
    "k1_first": (830, 32, 768, 2.0, None),    # the first U_max of the K = 1 walk
    "v16390": (12, 16390, 3, 3.0, None),      # a long row (the pre-pass streams it: no LDS limit)
    "word8": (9, 20, 5, 2.0, (9, 8, 7)),      # one below, at, one above a decision word
    "norm16": (17, 20, 5, 2.0, (17, 16, 15)),   # ... kAlNorm: the first exchange / re-centring
    "norm32": (33, 20, 9, 2.0, (33, 32, 31)),   # ... two prefetch buffers
    "bt64": (65, 20, 9, 2.0, (65, 64, 63)),     # ... kAlBt: one backtrace block
    "bt128": (129, 20, 9, 2.0, (129, 128, 127)),  # ... two backtrace blocks
}
# (case, use) -> the first seed for which the precondition of that use holds
SEEDS = {
    ("v37", "fp32"): 0, ("v37", "bf16"): 0, ("v37", "f16"): 0,
    ("repeats", "fp32"): 0, ("repeats", "bf16"): 0, ("repeats", "f16"): 0,
    ("v1030", "fp32"): 0, ("halo2", "fp32"): 4, ("halo3", "fp32"): 2, ("widest", "fp32"): 0,
    ("v16390", "fp32"): 0, ("word8", "fp32"): 0, ("norm16", "fp32"): 0, ("norm32", "fp32"): 0,
    ("bt64", "fp32"): 0, ("bt128", "fp32"): 0,
    ("v37", "u0"): 0, ("v37", "u1"): 0, ("v37", "t1"): 0, ("v37", "minlen"): 0,
    ("v37", "infeasible"): 0, ("v37", "zero_len"): 0, ("v37", "blank_last"): 0,
    ("v37", "logprob"): 0, ("v37", "nan"): 0, ("v37", "masked"): 0,
    # 16-bit rows of whole 8-element pieces: the pre-pass's 16-byte loads of 16-bit elements
    ("halo2", "bf16"): 0, ("halo2", "f16"): 0, ("halo3", "bf16"): 1, ("halo3", "f16"): 2,
    ("k16_full", "fp32"): 1, ("k1_first", "fp32"): 1,
}


def lengths_of(case):
    T, _, U, _, lens = CASES[case]
    return (list(lens) if lens else [max(1, n) for n in (T, T - 7, T // 2)],
            [U, max(U - 2, 0), max(U // 3, 1)])


def as_dtype(a, dtype):
    """The values the kernel sees: rounded to dtype, as fp64 numpy."""
    return torch.as_tensor(a, dtype=torch.float32).to(TDT[dtype]).double().numpy()


def make_inputs(case, seed, dtype="fp32", blank=0):
    """(x [B][T][V] fp64 holding dtype's values, targets [B][U] int64) of a seed: iid normal
    logits, labels drawn from every token but blank, and the first two labels of every
    transcript made equal (an adjacent repeat whatever V is)."""
    T, V, U, scale, _ = CASES[case]
    rng = np.random.default_rng(seed)
    x = as_dtype(scale * rng.standard_normal((B, T, V)), dtype)
    labels = np.array([v for v in range(V) if v != blank])
    targets = labels[rng.integers(0, V - 1, (B, U))]
    if U >= 2:
        targets[:, 1] = targets[:, 0]
    return x, targets.astype(np.int64)


@functools.lru_cache(maxsize=None)
def inputs(case, use="fp32", dtype="fp32", blank=0):
    x, targets = make_inputs(case, SEEDS[case, use], dtype, blank)
    x.setflags(write=False)
    targets.setflags(write=False)
    return x, targets


def freeze(a):
    return a.shape, a.dtype.str, a.tobytes()


def thaw(f):
    return np.frombuffer(f[2], np.dtype(f[1])).reshape(f[0])


def precondition(refs64, refs32, tgts, need_repeat=True, forced=False):
    """The condition on the input; None when it holds, else what failed.  (A transcript of one
    token cannot repeat: the repeat is asked of every longer one, and of one at least.)"""
    if need_repeat and not any(len(tg) >= 2 for tg in tgts):
        return "no transcript long enough for an adjacent repeat"
    for b, (r, r32, tg) in enumerate(zip(refs64, refs32, tgts)):
        if not r.feasible or r.states.size == 0:
            continue
        if need_repeat and len(tg) >= 2 and not any(a == c for a, c in zip(tg, tg[1:])):
            return f"stream {b}: no adjacent repeat"
        if not np.array_equal(r.states, r32.states):
            return f"stream {b}: the reference's fp32 path differs from its fp64 path"
        d32, _ = drift(r, r32)
        if not forced and r.margin < max(1e-3, 100 * d32):
            return f"stream {b}: margin {r.margin:.3g} < max(1e-3, 100 * {d32:.3g})"
    return None


def reference(x, targets, in_lens, tgt_lens, blank=0, is_logits=True):
    """Per stream the fp64 and the fp32 run of the reference."""
    out = []
    for dt in (np.float64, np.float32):
        out.append([ctc_align_ref(x[b, :in_lens[b]], targets[b, :tgt_lens[b]], blank, is_logits, dt)
                    for b in range(x.shape[0])])
    return out


def expect(x, targets, in_lens, tgt_lens, blank=0, is_logits=True, need_repeat=True, forced=False):
    """(fp64 references, e32 per stream) of one input after asserting the precondition."""
    return _expect(freeze(x), freeze(targets), tuple(in_lens), tuple(tgt_lens), blank, is_logits,
                   need_repeat, forced)


@functools.lru_cache(maxsize=None)
def _expect(xf, tf, in_lens, tgt_lens, blank, is_logits, need_repeat, forced):
    x, targets = thaw(xf), thaw(tf)
    r64, r32 = reference(x, targets, in_lens, tgt_lens, blank, is_logits)
    tgts = [targets[b, :tgt_lens[b]].tolist() for b in range(len(in_lens))]
    bad = precondition(r64, r32, tgts, need_repeat, forced)
    assert bad is None, bad
    return r64, [drift(a, c)[1] for a, c in zip(r64, r32)]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV, dtype)


def gpu_align(x, targets, in_lens, tgt_lens, dtype="fp32", blank=0, is_logits=True, op=None):
    """ops.ctc_align (or `op`) -> (states, labels, frame_lp, spans, token_lp, score) numpy."""
    from statecatcher_amd import ops
    out = (op or ops.ctc_align)(dev(x, TDT[dtype]), dev(targets, torch.int64),
                                dev(list(in_lens), torch.int64), dev(list(tgt_lens), torch.int64),
                                blank, is_logits)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(got, refs, e32s, in_lens, what=None, streams=None):
    states, labels, frame_lp, spans, token_lp, score = got
    T, U = states.shape[1], spans.shape[1]
    worst = 0.0
    for b in (range(len(refs)) if streams is None else streams):
        r, e32, Tb = refs[b], e32s[b], min(max(in_lens[b], 0), T)
        n, u = len(r.states), len(r.spans)
        assert n == Tb
        np.testing.assert_array_equal(states[b, :n], r.states)
        np.testing.assert_array_equal(labels[b, :n], r.labels)
        assert (states[b, n:] == -1).all() and (labels[b, n:] == -1).all()
        assert (frame_lp[b, n:] == 0).all()
        np.testing.assert_array_equal(spans[b, :u], r.spans)
        assert (spans[b, u:] == -1).all() and (token_lp[b, u:] == 0).all()
        if not r.feasible:
            assert np.isneginf(score[b]) and (frame_lp[b] == 0).all() and (token_lp[b] == 0).all()
            continue
        for name, a, w in (("frame_lp", frame_lp[b, :n], r.frame_lp),
                           ("token_lp", token_lp[b, :u], r.token_lp)):
            err = np.abs(a.astype(np.float64) - w)
            tol = 8 * e32 + 2.0 ** -22 * np.abs(w)
            assert (err <= tol).all(), (b, name, float((err - tol).max()), e32)
            worst = max(worst, float((err / e32).max()) if e32 > 0 and err.size else 0.0)
        err = abs(float(score[b]) - r.score)
        assert err <= 8 * e32 * max(Tb, 1) + 1e-6 * abs(r.score), (b, float(score[b]), r.score, e32)
    if what:
        print(f"ctc_align lp error / e32 [{what}]: {worst:.3f}")


PARITY = [(c, "fp32") for c in CASES] + [(c, d) for c in ("v37", "repeats", "halo2", "halo3")
                                         for d in ("bf16", "f16")]


@pytest.mark.parametrize("case,dtype", PARITY)
def test_parity_with_fp64_reference(case, dtype):
    x, targets = inputs(case, dtype, dtype)
    in_lens, tgt_lens = lengths_of(case)
    refs, e32s = expect(x, targets, in_lens, tgt_lens)
    assert all(r.feasible for r in refs)
    check(gpu_align(x, targets, in_lens, tgt_lens, dtype), refs, e32s, in_lens, f"{case}/{dtype}")


# ------------------------------------------------------------------------------ edge cases ----
def test_empty_transcripts_align_to_all_blank():
    x, targets = inputs("v37", "u0")
    in_lens, _ = lengths_of("v37")
    for tg in (targets, targets[:, :0]):     # U = 0 inside a padded batch, and U_max = 0
        refs, e32s = expect(x, tg, in_lens, [0, 0, 0], need_repeat=False, forced=True)
        got = gpu_align(x, tg, in_lens, [0, 0, 0])
        check(got, refs, e32s, in_lens)
        assert all((got[0][b, :in_lens[b]] == 0).all() for b in range(B))


def test_single_token_transcripts():
    x, targets = inputs("v37", "u1")
    in_lens, _ = lengths_of("v37")
    refs, e32s = expect(x, targets, in_lens, [1, 1, 1], need_repeat=False)
    check(gpu_align(x, targets, in_lens, [1, 1, 1]), refs, e32s, in_lens)


def test_single_frame_sequences():
    x, targets = inputs("v37", "t1")
    in_lens, tgt_lens = [1, 1, 1], [1, 0, 2]      # the last cannot be aligned
    refs, e32s = expect(x, targets, in_lens, tgt_lens, need_repeat=False)
    assert [r.feasible for r in refs] == [True, True, False]
    check(gpu_align(x, targets, in_lens, tgt_lens), refs, e32s, in_lens)


def test_minimum_feasible_length_forces_the_path():
    x, targets = inputs("v37", "minlen")
    _, tgt_lens = lengths_of("v37")
    in_lens = [min_feasible_len(targets[b, :tgt_lens[b]]) for b in range(B)]
    refs, e32s = expect(x, targets, in_lens, tgt_lens, forced=True)
    assert all(r.feasible and np.isinf(r.margin) for r in refs)   # no decision had a choice
    check(gpu_align(x, targets, in_lens, tgt_lens), refs, e32s, in_lens)


def test_infeasible_stream_beside_feasible_ones():
    x, targets = inputs("v37", "infeasible")
    _, tgt_lens = lengths_of("v37")
    in_lens = [40, min_feasible_len(targets[1, :tgt_lens[1]]) - 1, 20]
    refs, e32s = expect(x, targets, in_lens, tgt_lens)
    assert [r.feasible for r in refs] == [True, False, True]
    check(gpu_align(x, targets, in_lens, tgt_lens), refs, e32s, in_lens)


def test_zero_length_stream_and_empty_time_axis():
    x, targets = inputs("v37", "zero_len")
    _, tgt_lens = lengths_of("v37")
    in_lens = [40, 0, 20]
    refs, e32s = expect(x, targets, in_lens, tgt_lens)
    got = gpu_align(x, targets, in_lens, tgt_lens)
    check(got, refs, e32s, in_lens)
    assert np.isneginf(got[5][1])
    # T_b = 0 with U = 0 scores 0; T = 0 altogether
    got = gpu_align(x, targets, in_lens, [tgt_lens[0], 0, tgt_lens[2]])
    assert got[5][1] == 0.0 and (got[0][1] == -1).all() and (got[3][1] == -1).all()
    got = gpu_align(x[:, :0], targets, [0, 0, 0], [0, 2, 3])
    assert got[0].shape == (B, 0) and got[2].shape == (B, 0)
    assert got[5].tolist() == [0.0, -np.inf, -np.inf]
    assert (got[3] == -1).all() and (got[4] == 0).all()


def test_blank_is_the_last_token():
    V = CASES["v37"][1]
    x, targets = inputs("v37", "blank_last", blank=V - 1)
    assert targets.max() < V - 1
    in_lens, tgt_lens = lengths_of("v37")
    refs, e32s = expect(x, targets, in_lens, tgt_lens, blank=V - 1)
    check(gpu_align(x, targets, in_lens, tgt_lens, blank=V - 1), refs, e32s, in_lens)


def test_log_prob_input_gives_the_path_of_the_logits():
    x, targets = inputs("v37", "logprob")
    in_lens, tgt_lens = lengths_of("v37")
    lp = torch.log_softmax(torch.as_tensor(np.array(x), dtype=torch.float32), -1).double().numpy()
    refs_l, _ = expect(x, targets, in_lens, tgt_lens)
    refs_p, e32s = expect(lp, targets, in_lens, tgt_lens, is_logits=False)
    for a, c in zip(refs_l, refs_p):
        np.testing.assert_array_equal(a.states, c.states)
    check(gpu_align(lp, targets, in_lens, tgt_lens, is_logits=False), refs_p, e32s, in_lens)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_vocabulary_entries_are_minus_infinity(dtype):
    """-inf logits (a masked vocabulary) at tokens the transcripts do not use, the first columns
    of a row among them: exp(-inf) = 0 in the row's normaliser, nothing becomes NaN."""
    x, targets = inputs("v37", "masked", dtype)
    in_lens, tgt_lens = lengths_of("v37")
    x = np.array(x)
    free = [v for v in range(1, CASES["v37"][1]) if v not in set(targets.ravel().tolist())]
    assert len(free) >= 4 and free[0] < 8
    x[:, :, free[::2]] = -np.inf
    refs, e32s = expect(x, targets, in_lens, tgt_lens)
    assert all(r.feasible for r in refs)
    check(gpu_align(x, targets, in_lens, tgt_lens, dtype), refs, e32s, in_lens)


def test_tie_rule_on_integer_log_probs():
    """The integer-valued case of tests/test_ctc_align_host.py (pinned there against enumeration):
    fp32 sums are exact, so every output must match exactly."""
    x, targets, in_lens, tgt_lens = tie_cases()
    got = gpu_align(x, targets, in_lens, tgt_lens, is_logits=False)
    tied = 0
    for b in range(len(x)):
        r = ctc_align_ref(x[b, :in_lens[b]], targets[b, :tgt_lens[b]], is_logits=False,
                          dtype=np.float32)
        n, u = in_lens[b], tgt_lens[b]
        if not r.feasible:
            assert np.isneginf(got[5][b]) and (got[0][b] == -1).all() and (got[3][b] == -1).all()
            continue
        tied += r.margin == 0.0
        np.testing.assert_array_equal(got[0][b, :n], r.states)
        np.testing.assert_array_equal(got[1][b, :n], r.labels)
        np.testing.assert_array_equal(got[2][b, :n], r.frame_lp)
        np.testing.assert_array_equal(got[3][b, :u], r.spans)
        np.testing.assert_array_equal(got[4][b, :u], r.token_lp)
        assert got[5][b] == r.score
    assert tied >= 8


# ------------------------------------------------------------- tests that need no reference ----
def test_own_greedy_transcript_aligns_to_the_argmax_and_score_is_below_the_likelihood():
    from statecatcher_amd import ops
    T, V = 60, 24
    rng = np.random.default_rng(5)
    x = 2.0 * rng.standard_normal((B, T, V))
    x[:, :, 0] += 2.0
    lp = torch.log_softmax(dev(x), -1)
    lens = dev([T, T - 7, T // 2], torch.int64)
    tokens, counts = ops.ctc_greedy_decode(lp, lens)
    targets = tokens[:, :max(int(counts.max()), 1)].to(torch.int64).clamp_min(0)
    out = ops.ctc_align(lp, targets, lens, counts)
    nll = ops.ctc_nll(lp, targets, lens, counts.to(torch.int64), is_logits=False)
    torch.cuda.synchronize()
    labels, score, nll = out[1].cpu().numpy(), out[5].cpu().numpy(), nll.cpu().numpy()
    top2 = torch.topk(lp, 2, -1)
    clear = ((top2.values[..., 0] - top2.values[..., 1]) >= 1e-3).cpu().numpy()
    arg = top2.indices[..., 0].cpu().numpy()
    for b, n in enumerate(lens.tolist()):
        assert clear[b, :n].sum() > n // 2
        np.testing.assert_array_equal(labels[b, :n][clear[b, :n]], arg[b, :n][clear[b, :n]])
        # the best path cannot beat the sum over all paths
        assert np.isfinite(score[b]) and score[b] <= -nll[b] + 1e-4 * abs(nll[b])


# ---------------------------------------------------------------------------- plumbing --------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_16bit_rows_align_as_their_fp32_values(case, dtype):
    """Inputs are widened on load, all arithmetic is fp32 and the pre-pass sums a row in pieces of
    8 elements whatever the element type and the alignment: a 16-bit tensor aligns bitwise as the
    fp32 tensor of the same values, ties and all (no margin is needed for that).  Every case:
    rows of whole pieces in 16-byte loads (V = 20 .. 128 in 16-bit against two loads per piece in
    fp32), rows with a partial last piece (V = 37, 5, 1030, 16390) and rows that are aligned in
    one type only (V = 20 in 16-bit: every second row; V = 37, 5)."""
    x, targets = make_inputs(case, 1, dtype)
    in_lens, tgt_lens = lengths_of(case)
    a = gpu_align(x, targets, in_lens, tgt_lens, dtype)
    c = gpu_align(x, targets, in_lens, tgt_lens, "fp32")
    for p, q in zip(a, c):
        assert p.tobytes() == q.tobytes()


def test_layers_agree_bitwise_and_opcheck():
    import statecatcher_amd as sc
    from statecatcher_amd import torch_library
    x, targets = inputs("v37", "bf16", "bf16")
    in_lens, tgt_lens = lengths_of("v37")
    a = gpu_align(x, targets, in_lens, tgt_lens, "bf16")
    c = gpu_align(x, targets, in_lens, tgt_lens, "bf16", op=torch_library.ctc_align)
    for p, q in zip(a, c):
        assert p.tobytes() == q.tobytes()
    args = (dev(x, torch.bfloat16), dev(targets, torch.int64), dev(in_lens, torch.int64),
            dev(tgt_lens, torch.int64), 0, True)
    torch.library.opcheck(torch.ops.statecatcher.ctc_align.default, args,
                          test_utils=("test_schema", "test_faketensor"))
    # decoder.ctc_forced_align: the same alignment as dicts
    res = sc.ctc_forced_align(args[0], args[1], in_lens, tgt_lens, is_logits=True)
    for b, r in enumerate(res):
        n, u = in_lens[b], tgt_lens[b]
        assert r["score"] == float(a[5][b]) and r["score_per_frame"] == r["score"] / n
        assert r["labels"] == a[1][b, :n].tolist()
        assert [t[:3] for t in r["tokens"]] == [(int(targets[b, k]), *a[3][b, k].tolist())
                                                for k in range(u)]
        assert [t[3] for t in r["tokens"]] == a[4][b, :u].tolist()
    bad = sc.ctc_forced_align(args[0], args[1], [3, 40, 20], tgt_lens, is_logits=True)[0]
    assert bad == {"score": -np.inf, "score_per_frame": -np.inf, "tokens": [], "labels": []}


def test_no_host_sync_and_two_runs_are_bitwise_equal():
    from statecatcher_amd import ops
    x, targets = inputs("halo2")
    in_lens, tgt_lens = lengths_of("halo2")
    args = (dev(x), dev(targets, torch.int64), dev(in_lens, torch.int64),
            dev(tgt_lens, torch.int64), 0, True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ops.ctc_align(*args)
        c = ops.ctc_align(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for p, q in zip(a, c):
        assert p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes()


def test_graph_capture_replays_bitwise_equal_to_eager():
    from statecatcher_amd import ops
    x, targets = inputs("v37")
    x2, _ = make_inputs("v37", 7)
    in_lens, tgt_lens = lengths_of("v37")
    xs = dev(x)
    args = (xs, dev(targets, torch.int64), dev(in_lens, torch.int64), dev(tgt_lens, torch.int64),
            0, True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.ctc_align(*args)    # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ctc_align(*args)
    for xv in (x2, x):
        xs.copy_(dev(xv))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().tobytes() for t in out]
        want = ops.ctc_align(*args)
        torch.cuda.synchronize()
        assert got == [t.cpu().numpy().tobytes() for t in want]


@pytest.mark.parametrize("is_logits", [True, False])
def test_nan_row_leaves_the_other_streams_alone(is_logits):
    x, targets = inputs("v37", "nan")
    in_lens, tgt_lens = lengths_of("v37")
    if not is_logits:
        x = torch.log_softmax(torch.as_tensor(np.array(x), dtype=torch.float32), -1).double().numpy()
    refs, e32s = expect(x, targets, in_lens, tgt_lens, is_logits=is_logits)
    xn = np.array(x)
    xn[1, 5] = np.nan
    got = gpu_align(xn, targets, in_lens, tgt_lens, is_logits=is_logits)
    check(got, refs, e32s, in_lens, streams=(0, 2))
    U = tgt_lens[1]
    assert (got[0][1] >= -1).all() and (got[0][1] <= 2 * U).all()      # every index in range
    assert (got[3][1] >= -1).all() and (got[3][1] <= in_lens[1]).all()
