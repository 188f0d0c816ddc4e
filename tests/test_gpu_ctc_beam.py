"""GPU tests of the CTC prefix beam search (csrc/ctc_beam.hip) through every layer: the ctypes
ops (ops.ctc_beam_decode / ctc_beam_state / ctc_beam_result), the dispatcher ops and
decoder.ctc_beam_decoder.

The reference is the numpy restatement tests/ctc_beam_ref.py in fp64 (pinned against exact
enumeration in tests/test_ctc_beam_host.py).  Tokens and lens must equal it exactly and scores
within 8 * d32 + 1e-6 |score|, where d32 is the largest difference between the fp64 and an fp32
run of the reference on the same input over every candidate score (the factor 8 covers an fp32
evaluation order other than numpy's).  Exact tokens are a fair demand because every test first
asserts, on the CPU, that all three margins of the reference -- top_k-th to next lp, beam-th to
next candidate total, adjacent final scores -- are at least max(1e-3, 100 d32), and that the input
exercises at least one prefix merge and one repeat term.  Each case is milliseconds of GPU work.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ctc as octc
from tests.ctc_beam_ref import ctc_beam_ref, min_margin, padded_nbest, score_drift

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
B = 3

# name: (T, V, beam, top_k, scale)
CASES = {
    "small_v": (40, 37, 4, 5, 3.0),        # V not a multiple of 64
    "gen_v1030": (24, 1030, 8, 8, 4.0),    # V not a multiple of the load width
    "merges": (30, 5, 16, 4, 1.5),         # many prefix merges
    "max_width": (16, 1024, 32, 32, 4.0),  # widest beam and top_k: 1056 candidates
    "no_prune": (4, 3, 32, 2, 1.0),        # nothing is pruned
    "v5000": (8, 5000, 4, 4, 4.0),         # two rows per pre-pass workgroup
    "v9001": (8, 9001, 4, 4, 4.0),         # one row per pre-pass workgroup, scalar loads
    "v16390": (6, 16390, 4, 4, 4.0),       # a row that does not fit the LDS: re-read path
}
# (case, use) -> the first seed for which the precondition of that use holds (a use is one way
# the tests below decode the case: its dtype, or the variation named)
SEEDS = {
    ("small_v", "fp32"): 2, ("small_v", "bf16"): 750, ("small_v", "f16"): 1,
    ("small_v", "chunk"): 2, ("small_v", "logprob"): 2, ("small_v", "blank_last"): 4,
    ("small_v", "beam1"): 0, ("small_v", "zero_len"): 2, ("small_v", "max_frames"): 2,
    ("small_v", "graph"): 2,
    ("merges", "fp32"): 4, ("merges", "bf16"): 9, ("merges", "chunk"): 1,
    ("no_prune", "fp32"): 0, ("no_prune", "bf16"): 0,
    ("max_width", "fp32"): 75,
    ("gen_v1030", "fp32"): 609, ("gen_v1030", "logprob"): 609, ("gen_v1030", "blank_last"): 1040,
    ("v5000", "fp32"): 0, ("v9001", "fp32"): 0, ("v16390", "fp32"): 0,
}
# what the reference must have exercised, per case (precondition): the three cases that are here
# for the pre-pass's launch shapes have vocabularies in which iid logits never repeat a token
NEED = {c: ("merges", "repeats") for c in CASES}
NEED.update(v5000=(), v9001=(), v16390=())


def lengths_of(T):
    return [max(1, n) for n in (T, T - 7, T // 2)]


def as_dtype(a, dtype):
    """The values the kernel sees: rounded to dtype, as fp64 numpy."""
    return torch.as_tensor(a, dtype=torch.float32).to(TDT[dtype]).double().numpy()


@functools.lru_cache(maxsize=None)
def logits(case, use="fp32", dtype="fp32", blank=0):
    T, V, _, _, scale = CASES[case]
    rng = np.random.default_rng(SEEDS[case, use])
    x = scale * rng.standard_normal((B, T, V))
    x[:, :, blank] += scale
    x = as_dtype(x, dtype)
    x.setflags(write=False)
    return x


def freeze(a):
    return None if a is None else (a.shape, a.tobytes())


def expect(x, lengths=None, mask=None, blank=0, beam=8, top_k=8, is_logits=True, max_frames=None,
           need=("merges", "repeats")):
    """(fp64 reference, d32) of one input after asserting the precondition on the CPU."""
    return _expect(freeze(x), x.dtype.str, None if lengths is None else tuple(lengths),
                   freeze(mask), blank, beam, top_k, is_logits, max_frames, tuple(need))


@functools.lru_cache(maxsize=None)
def _expect(xf, xdt, lengths, maskf, blank, beam, top_k, is_logits, max_frames, need):
    x = np.frombuffer(xf[1], np.dtype(xdt)).reshape(xf[0])
    mask = None if maskf is None else np.frombuffer(maskf[1], np.float32).reshape(maskf[0])
    kw = dict(lengths=lengths, mask=mask, blank=blank, beam=beam, top_k=top_k, is_logits=is_logits,
              max_frames=max_frames)
    ref = ctc_beam_ref(x, dtype=np.float64, **kw)
    d32 = score_drift(ref, ctc_beam_ref(x, dtype=np.float32, **kw))
    bound = max(1e-3, 100 * d32)
    assert min_margin(ref) >= bound, (ref.topk_margin, ref.beam_margin, ref.final_margin, d32)
    for what in need:
        assert getattr(ref, what) >= 1, what
    return ref, d32


def log_probs32(x):
    """fp32 log_softmax of x as fp64 numpy: log-prob input for is_logits=False."""
    return torch.log_softmax(torch.as_tensor(np.array(x), dtype=torch.float32), -1).double().numpy()


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV, dtype)


def gpu_decode(x, dtype="fp32", lengths=None, mask=None, nbest=None, cap=None, **kw):
    """ops.ctc_beam_decode offline -> (tokens, lens, scores) numpy."""
    from statecatcher_amd import ops
    out = ops.ctc_beam_decode(dev(x, TDT[dtype]), lengths=dev(lengths, torch.int64),
                              mask=dev(mask), nbest=kw["beam"] if nbest is None else nbest,
                              cap=cap, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


RATIOS = {}   # the largest observed |score error| / d32 per test, printed for DESIGN.md


def check(got, ref, d32, nbest, cap, what=None, streams=None):
    tok, lens, scores = got
    want_tok, want_lens = padded_nbest(ref.tokens, nbest, cap)
    rows = range(len(ref.tokens)) if streams is None else streams
    worst = 0.0
    for b in rows:
        full = np.array([len(h) for h in ref.tokens[b][:nbest]], np.int32)
        np.testing.assert_array_equal(lens[b, :len(full)], full)       # full count, even past cap
        assert (lens[b, len(full):] == -1).all() and np.isneginf(scores[b, len(full):]).all()
        np.testing.assert_array_equal(tok[b], want_tok[b])             # -1 past lens: untouched
        for n, s in enumerate(ref.scores[b][:nbest]):
            err = abs(float(scores[b, n]) - s)
            worst = max(worst, err / d32 if d32 > 0 else 0.0)
            assert err <= 8 * d32 + 1e-6 * abs(s), (b, n, float(scores[b, n]), s, d32)
    if what:
        RATIOS[what] = worst
        print(f"ctc_beam score error / d32 [{what}]: {worst:.3f} (d32 = {d32:.3g})")


def live_lp(x, lengths, mask, b, is_logits=True):
    """fp64 log-probs of stream b's live frames."""
    lp = octc.log_softmax(x[b]) if is_logits else np.asarray(x[b], np.float64)
    keep = np.arange(x.shape[1]) < (x.shape[1] if lengths is None else lengths[b])
    if mask is not None:
        keep &= mask[b] != 0
    return lp[keep]


# bf16 parity runs where a seed can satisfy the precondition.  Rounded to bf16, the logits of a
# 1000-token frame sit on a grid of 2^-5 .. 2^-4 around the top_k-th largest, as wide as the gap
# to the next one: some frame of every input has the two exactly equal (a top_k margin of 0), and
# no seed passes.  Those cases run in bf16 in test_16bit_rows_decode_as_their_fp32_values.
PARITY = [(c, "fp32") for c in CASES] + [(c, "bf16") for c in ("small_v", "merges", "no_prune")]


@pytest.mark.parametrize("case,dtype", PARITY)
def test_parity_with_fp64_reference(case, dtype):
    """Check 1, and check 2: no hypothesis scores more than its full CTC likelihood (a beam can
    only lose alignments); where nothing is pruned the two are equal."""
    T, V, beam, top_k, _ = CASES[case]
    x, lens = logits(case, dtype, dtype), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k, need=NEED[case])
    got = gpu_decode(x, dtype, lengths=lens, beam=beam, top_k=top_k, is_logits=True)
    check(got, ref, d32, beam, T, what=f"{case}-{dtype}")
    tok, ln, scores = got
    for b in range(B):
        lp = live_lp(x, lens, None, b)
        for n in range(beam):
            if ln[b, n] < 0:
                continue
            nll, _ = octc.ctc_single(lp, tok[b, n, :ln[b, n]].astype(np.int64), 0)
            tol = 8 * d32 + 1e-6 * abs(nll)
            assert scores[b, n] <= -nll + tol, (b, n, scores[b, n], -nll)
            if case == "no_prune":
                assert abs(scores[b, n] + nll) <= tol


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_16bit_rows_decode_as_their_fp32_values(case, dtype):
    """Inputs are widened on load and all arithmetic is fp32: a 16-bit tensor decodes bitwise as
    the fp32 tensor of the same values, ties and all (no margin is needed for that).  With the
    fp32 parity above this covers the 16-byte loads of 16-bit rows at every vocabulary size."""
    T, V, beam, top_k, _ = CASES[case]
    x, lens = logits(case, "fp32", dtype), lengths_of(T)
    a = gpu_decode(x, dtype, lengths=lens, beam=beam, top_k=top_k, is_logits=True)
    c = gpu_decode(x, "fp32", lengths=lens, beam=beam, top_k=top_k, is_logits=True)
    assert (a[1] >= 0).any()
    for u, v in zip(a, c):
        assert u.tobytes() == v.tobytes()


def test_f16_inputs():
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v", "f16", "f16"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    check(gpu_decode(x, "f16", lengths=lens, beam=beam, top_k=top_k, is_logits=True), ref, d32,
          beam, T)


def chunk_mask(T):
    mask = np.ones((B, T), np.float32)
    mask[:, 10:13] = 0      # inside the third chunk
    mask[1, 3] = 0          # inside the second
    mask[0, 0] = 0          # the whole first chunk of stream 0
    return mask


@pytest.mark.parametrize("case", ["small_v", "merges"])
def test_chunked_equals_offline_bitwise(case):
    """Check 3: chunks of 1, 7 and the rest with mask-0 frames mid-chunk; lengths and mask given
    together and saying the same about the tail."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES[case]
    x, lens, mask = logits(case, "chunk"), lengths_of(T), chunk_mask(T)
    ref, d32 = expect(x, lens, mask, beam=beam, top_k=top_k)
    off = gpu_decode(x, lengths=lens, mask=mask, beam=beam, top_k=top_k, is_logits=True)
    check(off, ref, d32, beam, T)
    # the mask alone, zero past each length, says the same as lengths and mask
    tail = mask * (np.arange(T)[None, :] < np.array(lens)[:, None])
    only = gpu_decode(x, mask=tail, beam=beam, top_k=top_k, is_logits=True)
    for a, c in zip(off, only):
        np.testing.assert_array_equal(a, c)
    st = ops.ctc_beam_state(B, beam, T, DEV)
    xd = dev(x)
    t0 = 0
    for n in (1, 7, T - 8):
        cl = [max(0, min(l - t0, n)) for l in lens]
        out = ops.ctc_beam_decode(xd[:, t0:t0 + n], lengths=dev(cl, torch.int64),
                                  mask=dev(mask[:, t0:t0 + n]), top_k=top_k, nbest=beam,
                                  is_logits=True, state=st)
        t0 += n
    torch.cuda.synchronize()
    for a, c in zip(off, out):
        assert a.tobytes() == c.cpu().numpy().tobytes()
    again = ops.ctc_beam_result(st, beam)   # reading a state does not change it
    for a, c in zip(out, again):
        assert torch.equal(a, c)


@pytest.mark.parametrize("case", ["small_v", "gen_v1030"])
def test_logits_equal_log_softmax_input(case):
    """Check 4."""
    T, V, beam, top_k, _ = CASES[case]
    x, lens = logits(case, "logprob"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    lp = log_probs32(x)
    refp, d32p = expect(lp, lens, beam=beam, top_k=top_k, is_logits=False)
    assert refp.tokens == ref.tokens
    a = gpu_decode(x, lengths=lens, beam=beam, top_k=top_k, is_logits=True)
    c = gpu_decode(lp, lengths=lens, beam=beam, top_k=top_k, is_logits=False)
    check(a, ref, d32, beam, T)
    check(c, refp, d32p, beam, T)
    np.testing.assert_array_equal(a[0], c[0])
    np.testing.assert_array_equal(a[1], c[1])


@pytest.mark.parametrize("case", ["small_v", "gen_v1030"])
def test_blank_is_the_last_token(case):
    """Check 5."""
    T, V, beam, top_k, _ = CASES[case]
    x, lens = logits(case, "blank_last", blank=V - 1), lengths_of(T)
    ref, d32 = expect(x, lens, blank=V - 1, beam=beam, top_k=top_k)
    check(gpu_decode(x, lengths=lens, blank=V - 1, beam=beam, top_k=top_k, is_logits=True), ref,
          d32, beam, T)


def test_beam_one_top_one():
    """Check 6: one hypothesis, one token per frame (no merge can happen: not asked for)."""
    T, V, _, _, _ = CASES["small_v"]
    x, lens = logits("small_v", "beam1"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=1, top_k=1, need=("repeats",))
    check(gpu_decode(x, lengths=lens, beam=1, top_k=1, is_logits=True), ref, d32, 1, T)


def test_nbest_below_beam_and_short_cap():
    """Checks 7 and 8: nbest < beam returns the first nbest; cap below the longest hypothesis
    keeps lens full, writes the first cap tokens and leaves the -1 fill behind them."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    check(gpu_decode(x, lengths=lens, nbest=2, beam=beam, top_k=top_k, is_logits=True), ref, d32,
          2, T)
    cap = 3
    assert max(len(h) for hyps in ref.tokens for h in hyps) > cap
    check(gpu_decode(x, lengths=lens, cap=cap, beam=beam, top_k=top_k, is_logits=True), ref, d32,
          beam, cap)
    # into caller buffers: nothing is written at or beyond cap (sentinels behind the rows stay)
    flat = torch.full((B * beam * cap + 64,), -7, dtype=torch.int32, device=DEV)
    tok = flat[:B * beam * cap].view(B, beam, cap)
    ln = torch.empty(B, beam, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, beam, dtype=torch.float32, device=DEV)
    ops.ctc_beam_decode(dev(x), lengths=lens, beam=beam, top_k=top_k, is_logits=True,
                        nbest=beam, out=(tok, ln, sc))
    want, _ = padded_nbest(ref.tokens, beam, cap, fill=-7)
    np.testing.assert_array_equal(tok.cpu().numpy(), want)
    assert (flat[B * beam * cap:] == -7).all()


def test_zero_length_stream_and_empty_time_axis():
    """Check 9."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v", "zero_len"), [T, 0, T // 2]
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    assert ref.tokens[1] == [[]] and ref.scores[1] == [0.0]
    got = gpu_decode(x, lengths=lens, beam=beam, top_k=top_k, is_logits=True)
    check(got, ref, d32, beam, T)
    assert got[1][1].tolist() == [0] + [-1] * (beam - 1) and got[2][1, 0] == 0.0
    tok, ln, sc = ops.ctc_beam_decode(dev(x)[:, :0], beam=beam, top_k=top_k, nbest=2)
    assert tok.shape == (B, 2, 0) and ln.tolist() == [[0, -1]] * B
    assert sc[:, 0].tolist() == [0.0] * B
    tok, ln, sc = ops.ctc_beam_decode(dev(x)[:0], beam=beam, top_k=top_k, nbest=2)
    assert tok.shape == (0, 2, T) and ln.shape == (0, 2)


def test_max_frames_sets_status_and_stops():
    """Check 10."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens, mf = logits("small_v", "max_frames"), lengths_of(T), T - 5
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k, max_frames=mf)
    assert ref.status.tolist() == [1, 0, 0]
    st = ops.ctc_beam_state(B, beam, mf, DEV)
    ops.ctc_beam_decode(dev(x), lengths=lens, top_k=top_k, is_logits=True, state=st)
    tok, ln, sc, status = ops.ctc_beam_result(st, beam, return_status=True)
    assert tok.shape == (B, beam, mf)
    check((tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()), ref, d32, beam, mf)
    assert status.tolist() == [1, 0, 0]
    # frames offered after that are ignored too
    ops.ctc_beam_decode(dev(x), lengths=[2, 0, 0], top_k=top_k, is_logits=True, state=st)
    tok2, ln2, sc2, status2 = ops.ctc_beam_result(st, beam, return_status=True)
    assert torch.equal(tok, tok2) and torch.equal(sc, sc2) and status2.tolist() == [1, 0, 0]


def test_reset_of_some_streams():
    """Check 11."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    st = ops.ctc_beam_state(B, beam, 2 * T, DEV)
    feed = lambda: ops.ctc_beam_decode(dev(x), lengths=lens, top_k=top_k, nbest=beam,   # noqa: E731
                                       is_logits=True, state=st, cap=T)
    first = [t.clone() for t in feed()]
    check(tuple(t.cpu().numpy() for t in first), ref, d32, beam, T)
    st.reset(torch.tensor([0.0, 1.0, 0.0], device=DEV))
    tok, ln, sc = ops.ctc_beam_result(st, beam, cap=T)
    assert ln[1].tolist() == [0] + [-1] * (beam - 1) and sc[1, 0] == 0.0
    for b in (0, 2):
        assert torch.equal(tok[b], first[0][b]) and torch.equal(sc[b], first[2][b])
    second = feed()     # stream 1 decodes x afresh; the others went on from where they were
    for a, c in zip(first, second):
        assert torch.equal(a[1], c[1])
    assert not torch.equal(first[2][0], second[2][0])
    st.reset([0, 2])
    st.reset(streams=[1])
    assert ops.ctc_beam_result(st, 1)[1].tolist() == [[0]] * B


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layers_agree_bitwise_and_opcheck(dtype):
    """Check 12."""
    import statecatcher_amd as sc
    from statecatcher_amd import ops, torch_library
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v", dtype, dtype), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    xd, ld = dev(x, TDT[dtype]), dev(lens, torch.int64)
    mask = torch.ones(B, T, device=DEV)
    mask[:, 4] = 0
    a = ops.ctc_beam_decode(xd, lengths=ld, mask=mask, beam=beam, top_k=top_k, nbest=beam,
                            is_logits=True)
    c = torch_library.ctc_beam_decode(xd, lengths=ld, mask=mask, beam=beam, top_k=top_k,
                                      nbest=beam, is_logits=True)
    state = torch_library.ctc_beam_state(B, beam, T, DEV)
    torch_library.ctc_beam_frames_(xd[:, :9], state, ld.clamp(max=9), mask[:, :9], 0, beam, top_k,
                                   True)
    torch_library.ctc_beam_frames_(xd[:, 9:], state, (ld - 9).clamp(min=0), mask[:, 9:], 0, beam,
                                   top_k, True)
    d = torch_library.ctc_beam_result(state, beam, beam, T)
    for u, v, w in zip(a, c, d):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert d[3].tolist() == [0] * B
    # the drop-in: log-probs in, lists out (nbest = 1 as ctc_greedy_decoder, nbest > 1 per stream)
    lp = torch.log_softmax(xd.float(), -1)
    e = ops.ctc_beam_decode(lp, lengths=ld, beam=beam, top_k=top_k, nbest=beam)
    tok, ln = e[0].cpu(), e[1].cpu().tolist()
    want = [[tok[b, n, :ln[b][n]].tolist() for n in range(beam) if ln[b][n] >= 0] for b in range(B)]
    assert sc.ctc_beam_decoder(lp, lens, beam=beam, top_k=top_k) == [w[0] for w in want]
    hyps, scores = sc.ctc_beam_decoder(lp, ld, beam=beam, top_k=top_k, nbest=beam,
                                       return_scores=True)
    assert hyps == want
    for b in range(B):
        assert scores[b] == e[2][b, :len(want[b])].tolist()
    if dtype == "fp32":
        assert hyps == ref.tokens
    stt = torch.ops.statecatcher
    torch.library.opcheck(stt.ctc_beam_decode.default,
                          (xd, ld, mask, 0, beam, top_k, 2, True, None, 7),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.ctc_beam_frames_.default, (xd, state, ld, mask, 0, beam, top_k, True),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.ctc_beam_result.default, (state, beam, 2, 5),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.ctc_beam_reset_.default, (state, beam, T, None),
                          test_utils=("test_schema", "test_faketensor"))


def test_no_host_sync():
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    xd, ld = dev(x), dev(lens, torch.int64)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.ctc_beam_decode(xd, lengths=ld, beam=beam, top_k=top_k, nbest=beam,
                                  is_logits=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(tuple(t.cpu().numpy() for t in out), ref, d32, beam, T)


def test_graph_capture_of_one_chunk_call():
    """Check 13: the frame counter lives in the state, so one captured chunk call replayed over
    three chunks equals the three eager chunk calls."""
    from statecatcher_amd import ops
    T, V, beam, top_k, _ = CASES["small_v"]
    C = 13
    x, lens = logits("small_v", "graph")[:, :3 * C], [3 * C, 3 * C - 7, C + 6]
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    xd = dev(x)
    chunk_lens = [dev([max(0, min(l - k * C, C)) for l in lens], torch.int64) for k in range(3)]
    eager = ops.ctc_beam_state(B, beam, 3 * C, DEV)
    for k in range(3):
        want = ops.ctc_beam_decode(xd[:, k * C:(k + 1) * C], lengths=chunk_lens[k], top_k=top_k,
                                   nbest=beam, is_logits=True, state=eager)
    check(tuple(t.cpu().numpy() for t in want), ref, d32, beam, 3 * C)
    st = ops.ctc_beam_state(B, beam, 3 * C, DEV)
    xs, ls = xd[:, :C].clone(), chunk_lens[0].clone()
    tok = torch.full((B, beam, 3 * C), -1, dtype=torch.int32, device=DEV)
    ln = torch.empty(B, beam, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, beam, dtype=torch.float32, device=DEV)
    run = lambda: ops.ctc_beam_decode(xs, lengths=ls, top_k=top_k, nbest=beam,   # noqa: E731
                                      is_logits=True, state=st, out=(tok, ln, sc))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run()               # warm-up: sizes the state's workspace outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    st.reset()
    for k in range(3):
        xs.copy_(xd[:, k * C:(k + 1) * C])
        ls.copy_(chunk_lens[k])
        tok.fill_(-1)
        graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(want, (tok, ln, sc)):
        assert a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


@pytest.mark.parametrize("is_logits", [True, False])
def test_nan_row_leaves_the_other_streams_alone(is_logits):
    """Check 14: a row of NaN in stream 1: the call completes, every returned token is a token,
    the other streams equal the reference."""
    T, V, beam, top_k, _ = CASES["small_v"]
    x, lens = logits("small_v", "fp32" if is_logits else "logprob"), lengths_of(T)
    ref, d32 = expect(x, lens, beam=beam, top_k=top_k)
    bad = x.copy()
    bad[1, 5] = np.nan
    if not is_logits:
        bad = log_probs32(bad)
        ref, d32 = expect(log_probs32(x), lens, beam=beam, top_k=top_k, is_logits=False)
    got = gpu_decode(bad, lengths=lens, beam=beam, top_k=top_k, is_logits=is_logits)
    check(got, ref, d32, beam, T, streams=(0, 2))
    tok, ln, _ = got
    assert ((ln >= -1) & (ln <= T)).all()
    for b in range(B):
        for n in range(beam):
            if ln[b, n] >= 0:
                row = tok[b, n, :ln[b, n]]
                assert ((row >= 0) & (row < V)).all()
