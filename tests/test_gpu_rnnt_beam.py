"""GPU tests of the transducer beam search (csrc/rnnt_beam.hip) through every layer: the ctypes
ops (ops.rnnt_beam_decode / rnnt_beam_state / rnnt_beam_result), the dispatcher ops and
decoder.rnnt_beam_decoder.

The reference is the numpy restatement tests/rnnt_beam_ref.py in fp64 (pinned against exact
lattices in tests/test_rnnt_beam_host.py).  Tokens, lens and frames must equal it exactly and
scores within 8 * d32 + 1e-6 |score|, where d32 is the largest difference between the fp64 and an
fp32 run of the reference on the same input over every candidate score (the fp32 run uses the
kernel's tanh form and a sequential dot product; the factor 8 covers an fp32 evaluation order
other than numpy's).  Exact tokens are a fair demand because every test first asserts, on the CPU,
that all margins of the reference -- top_k-th to next lp on every row expanded, beam-th to next in
every D and A selection, adjacent final scores -- are at least max(1e-3, 100 d32), and that the
input has at least one merge into A.  Each case is milliseconds of GPU work.

Observed |score error| / d32 on an MI355X (bound: 8): fast_v37 0.58 (fp32), 0.55 (bf16), 0.38
(f16); fast_v1024 0.43; gen_j20 0.39; gen_v1030 0.56; max_width 0.44; two_tok 0.98; no_prune 0.97.
"""
import functools

import numpy as np
import pytest
import torch

from tests.rnnt_beam_ref import (exact_prefix_scores, min_margin, padded_nbest, rnnt_beam_ref,
                                 rnnt_lp_row, score_drift)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# name: (B, T, V, J, blank bias, beam, top_k, max_symbols); inputs by the greedy test's recipe
CASES = {
    "fast_v37": (3, 40, 37, 64, 4.5, 4, 5, 2),         # fast path, V not a multiple of the wave size
    "fast_v1024": (2, 24, 1024, 64, 9.0, 8, 8, 2),     # fast path, one row per lane exactly
    "gen_j20": (2, 30, 50, 20, 3.5, 4, 4, 3),          # general path, J not a multiple of 4
    "gen_v1030": (2, 12, 1030, 64, 9.0, 8, 8, 2),      # general path, V just over one workgroup's rows
    "max_width": (1, 4, 1024, 64, 9.0, 32, 32, 1),     # widest beam and top_k: 1024 candidates, two passes
    "two_tok": (2, 30, 37, 64, 2.0, 4, 5, 2),          # a final hypothesis with two tokens on one frame
    "no_prune": (1, 2, 3, 64, 0.0, 32, 2, 2),          # nothing is pruned: 31 hypotheses
}
# (case, use) -> the first seed for which the precondition of that use holds (a use is one way
# the tests below decode the case: its dtype, or the variation named)
SEEDS = {
    ("fast_v37", "fp32"): 5, ("fast_v37", "bf16"): 6, ("fast_v37", "f16"): 1,
    ("fast_v37", "chunk"): 5, ("fast_v37", "blank_last"): 1, ("fast_v37", "beam1"): 0,
    ("fast_v37", "zero_len"): 1, ("fast_v37", "max_frames"): 5,
    ("fast_v1024", "fp32"): 717,
    ("gen_j20", "fp32"): 11, ("gen_j20", "chunk"): 21, ("gen_j20", "blank_last"): 15,
    ("gen_v1030", "fp32"): 12,
    ("max_width", "fp32"): 19,
    ("two_tok", "fp32"): 0,
    ("no_prune", "fp32"): 0,
}


def lengths_of(B, T):
    return [T, T - 7, T // 2][:B]


def as_dtype(a, dtype):
    """The values the kernel sees: rounded to dtype, as fp64 numpy."""
    return torch.as_tensor(a, dtype=torch.float32).to(TDT[dtype]).double().numpy()


@functools.lru_cache(maxsize=None)
def inputs(case, use="fp32", dtype="fp32", blank=0):
    B, T, V, J, bb = CASES[case][:5]
    rng = np.random.default_rng(SEEDS[case, use])
    E = rng.standard_normal((B, T, J))
    P = rng.standard_normal((V, J))
    W = 0.5 * rng.standard_normal((V, J))
    bias = rng.standard_normal(V)
    bias[blank] += bb
    E, P, W = (as_dtype(a, dtype) for a in (E, P, W))
    bias = as_dtype(bias, "fp32")
    for a in (E, P, W, bias):
        a.setflags(write=False)
    return E, P, W, bias


def freeze(a):
    return None if a is None else (a.shape, a.dtype.str, np.ascontiguousarray(a).tobytes())


def thaw(f):
    return None if f is None else np.frombuffer(f[2], np.dtype(f[1])).reshape(f[0])


def expect(ins, lengths=None, mask=None, blank=0, beam=8, top_k=8, max_symbols=2, max_frames=None,
           need_merge=True):
    """(fp64 reference, d32) of one input after asserting the precondition on the CPU."""
    return _expect(tuple(freeze(np.asarray(a)) for a in ins),
                   None if lengths is None else tuple(lengths), freeze(mask), blank, beam, top_k,
                   max_symbols, max_frames, need_merge)


@functools.lru_cache(maxsize=None)
def _expect(insf, lengths, maskf, blank, beam, top_k, max_symbols, max_frames, need_merge):
    E, P, W, bias = (thaw(f) for f in insf)
    kw = dict(lengths=lengths, mask=thaw(maskf), blank=blank, beam=beam, top_k=top_k,
              max_symbols=max_symbols, max_frames=max_frames)
    ref = rnnt_beam_ref(E, P, W, bias, dtype=np.float64, **kw)
    d32 = score_drift(ref, rnnt_beam_ref(E, P, W, bias, dtype=np.float32, **kw))
    bound = max(1e-3, 100 * d32)
    assert min_margin(ref) >= bound, (ref.topk_margin, ref.beam_margin, ref.final_margin, d32)
    assert ref.merges >= 1 or not need_merge
    return ref, d32


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV, dtype)


def dev_inputs(ins, dtype="fp32"):
    E, P, W, bias = ins
    return dev(E, TDT[dtype]), dev(P, TDT[dtype]), dev(W, TDT[dtype]), dev(bias)


def gpu_decode(ins, dtype="fp32", lengths=None, mask=None, nbest=None, cap=None, **kw):
    """ops.rnnt_beam_decode offline -> (tokens, lens, scores, frames) numpy."""
    from statecatcher_amd import ops
    out = ops.rnnt_beam_decode(*dev_inputs(ins, dtype), lengths=dev(lengths, torch.int64),
                               mask=dev(mask), nbest=kw["beam"] if nbest is None else nbest,
                               cap=cap, return_frames=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(got, ref, d32, nbest, cap, what=None, streams=None):
    tok, lens, scores, frames = got
    want_tok, _ = padded_nbest(ref.tokens, nbest, cap)
    want_frm, _ = padded_nbest(ref.frames, nbest, cap)
    rows = range(len(ref.tokens)) if streams is None else streams
    worst = 0.0
    for b in rows:
        full = np.array([len(h) for h in ref.tokens[b][:nbest]], np.int32)
        np.testing.assert_array_equal(lens[b, :len(full)], full)       # full count, even past cap
        assert (lens[b, len(full):] == -1).all() and np.isneginf(scores[b, len(full):]).all()
        np.testing.assert_array_equal(tok[b], want_tok[b])             # -1 past lens: untouched
        if frames is not None:
            np.testing.assert_array_equal(frames[b], want_frm[b])
        for n, s in enumerate(ref.scores[b][:nbest]):
            err = abs(float(scores[b, n]) - s)
            worst = max(worst, err / d32 if d32 > 0 else 0.0)
            assert err <= 8 * d32 + 1e-6 * abs(s), (b, n, float(scores[b, n]), s, d32)
    if what:
        print(f"rnnt_beam score error / d32 [{what}]: {worst:.3f} (d32 = {d32:.3g})")


def params(case):
    B, T, V, J, bb, beam, top_k, ms = CASES[case]
    return B, T, V, dict(beam=beam, top_k=top_k, max_symbols=ms)


PARITY = [(c, "fp32") for c in CASES] + [("fast_v37", "bf16"), ("fast_v37", "f16")]


@pytest.mark.parametrize("case,dtype", PARITY)
def test_parity_with_fp64_reference(case, dtype):
    B, T, V, kw = params(case)
    ins, lens = inputs(case, dtype, dtype), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    if case == "two_tok":
        assert max(ref.per_frame) >= 2, ref.per_frame
    got = gpu_decode(ins, dtype, lengths=lens, **kw)
    check(got, ref, d32, kw["beam"], T * kw["max_symbols"], what=f"{case}-{dtype}")
    if case == "no_prune":
        # every prefix of up to T * max_symbols tokens, against the exact lattice
        E, P, W, bias = ins
        exact = exact_prefix_scores(lambda t, u: rnnt_lp_row(E[0, t], P[u], W, bias), T, V, 0,
                                    kw["max_symbols"], T * kw["max_symbols"])
        tok, ln, scores, _ = got
        assert (ln[0] >= 0).sum() == 31 == len(exact)
        for n in range(31):
            y = tuple(tok[0, n, :ln[0, n]].tolist())
            assert abs(scores[0, n] - exact[y]) <= 8 * d32 + 1e-6 * abs(exact[y]), (y, scores[0, n])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["fast_v37", "fast_v1024", "gen_j20", "gen_v1030", "max_width"])
def test_16bit_inputs_decode_as_their_fp32_values(case, dtype):
    """Inputs are widened on load and all arithmetic is fp32: 16-bit tensors decode bitwise as the
    fp32 tensors of the same values, ties and all (no margin is needed for that).  With the fp32
    parity above this covers the 16-byte loads of 16-bit rows of W on both paths."""
    B, T, V, kw = params(case)
    ins, lens = inputs(case, "fp32", dtype), lengths_of(B, T)
    a = gpu_decode(ins, dtype, lengths=lens, **kw)
    c = gpu_decode(ins, "fp32", lengths=lens, **kw)
    assert (a[1] >= 0).any()
    for u, v in zip(a, c):
        assert u.tobytes() == v.tobytes()


def chunk_mask(B, T):
    mask = np.ones((B, T), np.float32)
    mask[:, 10:13] = 0
    mask[1, 20] = 0
    mask[0, 0] = 0
    return mask


@pytest.mark.parametrize("case", ["fast_v37", "gen_j20"])
def test_chunked_equals_offline_bitwise(case):
    """Chunks of 1, 5 and 7 with mask-0 frames equal the decode in one call."""
    from statecatcher_amd import ops
    B, T, V, kw = params(case)
    ins, lens, mask = inputs(case, "chunk"), lengths_of(B, T), chunk_mask(B, T)
    ref, d32 = expect(ins, lens, mask, **kw)
    off = gpu_decode(ins, lengths=lens, mask=mask, **kw)
    check(off, ref, d32, kw["beam"], T * kw["max_symbols"])
    E, P, W, bias = dev_inputs(ins)
    for chunk in (1, 5, 7):
        st = ops.rnnt_beam_state(B, kw["beam"], kw["max_symbols"], T, DEV)
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            cl = [max(0, min(l - t0, n)) for l in lens]
            out = ops.rnnt_beam_decode(E[:, t0:t0 + n], P, W, bias, lengths=dev(cl, torch.int64),
                                       mask=dev(mask[:, t0:t0 + n]), top_k=kw["top_k"],
                                       nbest=kw["beam"], state=st, return_frames=True)
        torch.cuda.synchronize()
        for a, c in zip(off, out):
            assert a.tobytes() == c.cpu().numpy().tobytes()
        again = ops.rnnt_beam_result(st, kw["beam"], return_frames=True)   # reading changes nothing
        for a, c in zip(out, again):
            assert torch.equal(a, c)


@pytest.mark.parametrize("case", ["fast_v37", "gen_j20"])
def test_blank_is_the_last_token(case):
    B, T, V, kw = params(case)
    ins, lens = inputs(case, "blank_last", blank=V - 1), lengths_of(B, T)
    ref, d32 = expect(ins, lens, blank=V - 1, **kw)
    check(gpu_decode(ins, lengths=lens, blank=V - 1, **kw), ref, d32, kw["beam"],
          T * kw["max_symbols"])


def test_beam_one():
    """One hypothesis (no merge can happen: not asked for)."""
    B, T, V, kw = params("fast_v37")
    kw["beam"] = 1
    ins, lens = inputs("fast_v37", "beam1"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, need_merge=False, **kw)
    check(gpu_decode(ins, lengths=lens, **kw), ref, d32, 1, T * kw["max_symbols"])


def test_zero_length_stream_and_empty_time_axis():
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    ins, lens = inputs("fast_v37", "zero_len"), [T, 0, T // 2]
    ref, d32 = expect(ins, lens, **kw)
    assert ref.tokens[1] == [[]] and ref.scores[1] == [0.0]
    got = gpu_decode(ins, lengths=lens, **kw)
    check(got, ref, d32, kw["beam"], T * kw["max_symbols"])
    assert got[1][1].tolist() == [0] + [-1] * (kw["beam"] - 1) and got[2][1, 0] == 0.0
    E, P, W, bias = dev_inputs(ins)
    tok, ln, sc = ops.rnnt_beam_decode(E[:, :0], P, W, bias, nbest=2, **kw)
    assert tok.shape == (B, 2, 0) and ln.tolist() == [[0, -1]] * B
    assert sc[:, 0].tolist() == [0.0] * B
    tok, ln, sc = ops.rnnt_beam_decode(E[:0], P, W, bias, nbest=2, **kw)
    assert tok.shape == (0, 2, T * kw["max_symbols"]) and ln.shape == (0, 2)


def test_nbest_below_beam_and_short_cap():
    """nbest < beam returns the first nbest; cap below the longest hypothesis keeps lens full,
    writes the first cap tokens and frames and leaves the sentinels behind them."""
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    beam = kw["beam"]
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    check(gpu_decode(ins, lengths=lens, nbest=2, **kw), ref, d32, 2, T * kw["max_symbols"])
    cap = 2
    assert max(len(h) for hyps in ref.tokens for h in hyps) > cap
    check(gpu_decode(ins, lengths=lens, cap=cap, **kw), ref, d32, beam, cap)
    # into caller buffers: nothing is written at or beyond cap (sentinels behind the rows stay)
    flat = [torch.full((B * beam * cap + 64,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
    tok, frm = (f[:B * beam * cap].view(B, beam, cap) for f in flat)
    ln = torch.empty(B, beam, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, beam, dtype=torch.float32, device=DEV)
    ops.rnnt_beam_decode(*dev_inputs(ins), lengths=lens, nbest=beam, out=(tok, ln, sc, frm), **kw)
    np.testing.assert_array_equal(tok.cpu().numpy(), padded_nbest(ref.tokens, beam, cap, fill=-7)[0])
    np.testing.assert_array_equal(frm.cpu().numpy(), padded_nbest(ref.frames, beam, cap, fill=-7)[0])
    np.testing.assert_array_equal(ln.cpu().numpy(), padded_nbest(ref.tokens, beam, cap)[1])
    for f in flat:
        assert (f[B * beam * cap:] == -7).all()


def test_max_frames_sets_status_and_stops():
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    beam, ms = kw["beam"], kw["max_symbols"]
    ins, lens, mf = inputs("fast_v37", "max_frames"), lengths_of(B, T), T - 5
    ref, d32 = expect(ins, lens, max_frames=mf, **kw)
    assert ref.status.tolist() == [1, 0, 0]
    st = ops.rnnt_beam_state(B, beam, ms, mf, DEV)
    ops.rnnt_beam_decode(*dev_inputs(ins), lengths=lens, top_k=kw["top_k"], state=st)
    tok, ln, sc, frm, status = ops.rnnt_beam_result(st, beam, return_frames=True,
                                                    return_status=True)
    assert tok.shape == (B, beam, mf * ms)
    check(tuple(t.cpu().numpy() for t in (tok, ln, sc, frm)), ref, d32, beam, mf * ms)
    assert status.tolist() == [1, 0, 0]
    # frames offered after that are ignored too
    ops.rnnt_beam_decode(*dev_inputs(ins), lengths=[2, 0, 0], top_k=kw["top_k"], state=st)
    tok2, ln2, sc2, status2 = ops.rnnt_beam_result(st, beam, return_status=True)
    assert torch.equal(tok, tok2) and torch.equal(sc, sc2) and status2.tolist() == [1, 0, 0]


def test_reset_of_some_streams():
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    beam, ms = kw["beam"], kw["max_symbols"]
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    st = ops.rnnt_beam_state(B, beam, ms, 2 * T, DEV)
    args = dev_inputs(ins)
    feed = lambda: ops.rnnt_beam_decode(*args, lengths=lens, top_k=kw["top_k"],   # noqa: E731
                                        nbest=beam, state=st, cap=T * ms, return_frames=True)
    first = [t.clone() for t in feed()]
    check(tuple(t.cpu().numpy() for t in first), ref, d32, beam, T * ms)
    st.reset(torch.tensor([0.0, 1.0, 0.0], device=DEV))
    tok, ln, sc = ops.rnnt_beam_result(st, beam, cap=T * ms)
    assert ln[1].tolist() == [0] + [-1] * (beam - 1) and sc[1, 0] == 0.0
    for b in (0, 2):
        assert torch.equal(tok[b], first[0][b]) and torch.equal(sc[b], first[2][b])
    second = feed()     # stream 1 decodes afresh; the others went on from where they were
    for a, c in zip(first, second):
        assert torch.equal(a[1], c[1])
    assert not torch.equal(first[2][0], second[2][0])
    st.reset([0, 2])
    st.reset(streams=[1])
    assert ops.rnnt_beam_result(st, 1)[1].tolist() == [[0]] * B


def test_strided_enc_p():
    B, T, V, kw = params("fast_v37")
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    from statecatcher_amd import ops
    E, P, W, bias = dev_inputs(ins)
    wide = torch.full((B, T + 3, 64 + 24), float("nan"), device=DEV)
    view = wide[:, 2:2 + T, 8:8 + 64]
    view.copy_(E)
    assert not view.is_contiguous() and view.stride(2) == 1
    out = ops.rnnt_beam_decode(view, P, W, bias, lengths=lens, nbest=kw["beam"],
                               return_frames=True, **kw)
    check(tuple(t.cpu().numpy() for t in out), ref, d32, kw["beam"], T * kw["max_symbols"])


def test_no_host_sync():
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    args, ld = dev_inputs(ins), dev(lens, torch.int64)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.rnnt_beam_decode(*args, lengths=ld, nbest=kw["beam"], return_frames=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(tuple(t.cpu().numpy() for t in out), ref, d32, kw["beam"], T * kw["max_symbols"])


def test_graph_capture_of_one_chunk_call():
    """The frame counter lives in the state, so one captured chunk call replayed over four chunks
    equals the decode in one call."""
    from statecatcher_amd import ops
    B, T, V, kw = params("fast_v37")
    beam, ms, C = kw["beam"], kw["max_symbols"], 10
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    E, P, W, bias = dev_inputs(ins)
    chunk_lens = [dev([max(0, min(l - k * C, C)) for l in lens], torch.int64) for k in range(T // C)]
    st = ops.rnnt_beam_state(B, beam, ms, T, DEV)
    xs, ls = E[:, :C].clone(), chunk_lens[0].clone()
    tok = torch.full((B, beam, T * ms), -1, dtype=torch.int32, device=DEV)
    frm = torch.full_like(tok, -1)
    ln = torch.empty(B, beam, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, beam, dtype=torch.float32, device=DEV)
    run = lambda: ops.rnnt_beam_decode(xs, P, W, bias, lengths=ls, top_k=kw["top_k"],   # noqa: E731
                                       nbest=beam, state=st, out=(tok, ln, sc, frm))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run()               # warm-up: sizes the state's workspace outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    st.reset()
    for k in range(T // C):
        xs.copy_(E[:, k * C:(k + 1) * C])
        ls.copy_(chunk_lens[k])
        tok.fill_(-1)
        frm.fill_(-1)
        graph.replay()
    torch.cuda.synchronize()
    check(tuple(t.cpu().numpy() for t in (tok, ln, sc, frm)), ref, d32, beam, T * ms)


def test_nan_frame_leaves_the_other_streams_alone():
    """A frame of NaN in stream 1: the call completes, every returned token is a token, the other
    streams equal the reference."""
    B, T, V, kw = params("fast_v37")
    ins, lens = inputs("fast_v37"), lengths_of(B, T)
    ref, d32 = expect(ins, lens, **kw)
    E = ins[0].copy()
    E[1, 5] = np.nan
    got = gpu_decode((E,) + ins[1:], lengths=lens, **kw)
    check(got, ref, d32, kw["beam"], T * kw["max_symbols"], streams=(0, 2))
    tok, ln, _, _ = got
    assert ((ln >= -1) & (ln <= T * kw["max_symbols"])).all()
    for b in range(B):
        for n in range(kw["beam"]):
            if ln[b, n] >= 0:
                row = tok[b, n, :ln[b, n]]
                assert ((row >= 0) & (row < V)).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layers_agree_bitwise_and_opcheck(dtype):
    from statecatcher_amd import ops, torch_library
    B, T, V, kw = params("fast_v37")
    beam, top_k, ms = kw["beam"], kw["top_k"], kw["max_symbols"]
    ins, lens = inputs("fast_v37", dtype, dtype), lengths_of(B, T)
    E, P, W, bias = dev_inputs(ins, dtype)
    ld = dev(lens, torch.int64)
    mask = torch.ones(B, T, device=DEV)
    mask[:, 4] = 0
    a = ops.rnnt_beam_decode(E, P, W, bias, lengths=ld, mask=mask, nbest=beam, return_frames=True,
                             **kw)
    c = torch_library.rnnt_beam_decode(E, P, W, bias, lengths=ld, mask=mask, nbest=beam,
                                       return_frames=True, **kw)
    state = torch_library.rnnt_beam_state(B, beam, ms, T, DEV)
    torch_library.rnnt_beam_frames_(E[:, :9], P, W, bias, state, ld.clamp(max=9), mask[:, :9], 0,
                                    beam, top_k, ms)
    torch_library.rnnt_beam_frames_(E[:, 9:], P, W, bias, state, (ld - 9).clamp(min=0),
                                    mask[:, 9:], 0, beam, top_k, ms)
    d = torch_library.rnnt_beam_result(state, beam, ms, beam, T * ms)
    assert (a[1] > 0).any()
    for u, v, w in zip(a, c, d):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert d[4].tolist() == [0] * B
    stt = torch.ops.statecatcher
    torch.library.opcheck(stt.rnnt_beam_decode.default,
                          (E, P, W, bias, ld, mask, 0, beam, top_k, ms, 2, None, 7),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.rnnt_beam_frames_.default,
                          (E, P, W, bias, state, ld, mask, 0, beam, top_k, ms),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.rnnt_beam_result.default, (state, beam, ms, 2, 5),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(stt.rnnt_beam_reset_.default, (state, beam, ms, T, None),
                          test_utils=("test_schema", "test_faketensor"))


def make_joiner(cls, D, J, V, blank, seed, bb=1.5, scale=4.0):
    """A joiner whose paths mix blanks and emissions (fresh initialisation gives nearly flat
    logits), as the greedy decoder's tests build it."""
    import statecatcher_amd as sc
    torch.manual_seed(seed)
    jm = getattr(sc, cls)(D, 24, J, V)
    with torch.no_grad():
        jm.joiner.weight.mul_(scale)
        jm.enc_proj.weight.mul_(2.0)
        jm.pred_proj.weight.mul_(2.0)
        jm.joiner.bias[blank] += bb
    return jm


JOINER_SEEDS = {"RNNTPredictorJoiner": 38, "RNNTCompactPredictorJoiner": 38}


@pytest.mark.parametrize("cls", ["RNNTPredictorJoiner", "RNNTCompactPredictorJoiner"])
def test_rnnt_beam_decoder_drop_in(cls):
    import statecatcher_amd as sc
    from statecatcher_amd.decoder import rnnt_joiner_tables
    B, T, D, J, V, blank = 3, 30, 16, 64, 37, 0
    kw = dict(beam=4, top_k=5, max_symbols=2)
    seed = JOINER_SEEDS[cls]
    jm = make_joiner(cls, D, J, V, blank, seed=seed).to(DEV)
    enc_out = torch.randn(B, T, D, generator=torch.Generator().manual_seed(seed)).to(DEV)
    lens = lengths_of(B, T)
    f = lambda a: a.detach().double().cpu().numpy()   # noqa: E731
    with torch.no_grad():
        ins = (f(jm.enc_proj(enc_out)),) + tuple(f(a) for a in rnnt_joiner_tables(jm))
    ref, d32 = expect(ins, lens, blank=blank, **kw)
    assert max(len(h[0]) for h in ref.tokens) > 0
    hyps, scores, frames = sc.rnnt_beam_decoder(enc_out, jm, torch.tensor(lens), blank=blank,
                                                nbest=4, return_scores=True, return_frames=True,
                                                **kw)
    assert hyps == ref.tokens and frames == ref.frames
    for b in range(B):
        for got, want in zip(scores[b], ref.scores[b]):
            assert abs(got - want) <= 8 * d32 + 1e-6 * abs(want)
    assert sc.rnnt_beam_decoder(enc_out, jm, lens, blank=blank, **kw) == [h[0] for h in ref.tokens]


# ------------------------------------------------------------------------------ streaming ---
STREAM = dict(B=3, K=4, T=14, V=32, J=64, blank=0, beam=4, top_k=5, ms=2, nbest=4, max_frames=24)
# kind -> the first joiner seed for which the precondition holds on the streaming path's logits
STREAM_SEEDS = {"native": 9, "triton": 3}


def stream_setup(kind, seed):
    """(streaming class, model, joiner, x [B,T,16], masks [B,T]) on the device."""
    from statecatcher_amd.streaming import StreamingLucyRNN, StreamingLucyRNNtriton
    c = STREAM
    jm = make_joiner("RNNTPredictorJoiner", c["V"], c["J"], c["V"], c["blank"], seed=seed).to(DEV)
    if kind == "native":
        from tests.test_gpu_rnnt_decode import tiny_stream_model
        cls, m = StreamingLucyRNN, tiny_stream_model().to(DEV)
    else:
        from tests.test_gpu_streaming_triton import RNNT, conditioned_params, model_from
        p = conditioned_params(RNNT["L"], RNNT["Din"], RNNT["D"], c["V"], seed=RNNT["seed"])
        cls, m = StreamingLucyRNNtriton, model_from(p, RNNT["L"], RNNT["Din"], RNNT["D"], c["V"]).to(DEV)
    x = torch.randn(c["B"], c["T"], 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    masks = torch.ones(c["B"], c["T"], dtype=torch.bool, device=DEV)
    masks[1, c["T"] - 5:] = False
    return cls, m, jm, x, masks


def stream_inputs(jm, logits):
    """The helper's inputs of the streaming path's own logits [B,T,V]: enc_proj in fp64, the
    tables as the stream snapshots them (fp32)."""
    from statecatcher_amd.decoder import rnnt_joiner_tables
    f = lambda a: a.detach().double().cpu()   # noqa: E731
    enc_p = torch.nn.functional.linear(f(logits), f(jm.enc_proj.weight), f(jm.enc_proj.bias))
    return (enc_p.numpy(),) + tuple(f(a).numpy() for a in rnnt_joiner_tables(jm, torch.float32))


@pytest.mark.parametrize("kind", ["native", "triton"])
def test_streaming_beam(kind):
    """StreamingLucyRNN / StreamingLucyRNNtriton(joiner=, beam=): the n-best equals the helper
    run on the streaming path's own logits, identically with the graph on and off;
    reset(streams=[1]) restarts only stream 1's beam."""
    from statecatcher_amd import ops
    c = STREAM
    cls, m, jm, x, masks = stream_setup(kind, STREAM_SEEDS[kind])
    kw = dict(beam=c["beam"], top_k=c["top_k"], max_symbols=c["ms"])
    cap = c["max_frames"] * c["ms"]
    results = []
    for graph in (True, False):
        st = cls(m, batch=c["B"], frames_per_call=c["K"], graph=graph, joiner=jm, nbest=c["nbest"],
                 max_frames=c["max_frames"], **kw)
        toks, logits = st.decode(x, masks, return_logits=True)
        ref, d32 = expect(stream_inputs(jm, logits), [c["T"]] * c["B"],
                          masks.float().cpu().numpy(), blank=c["blank"], **kw)
        assert max(len(h[0]) for h in ref.tokens) > 0
        got = ops.rnnt_beam_result(st.beam_state, c["nbest"], return_frames=True)
        check(tuple(t.cpu().numpy() for t in got), ref, d32, c["nbest"], cap)
        assert toks == [h[0] for h in ref.tokens]
        before = [t.clone() for t in got]
        st.reset(streams=[1])
        tok, ln, sc = ops.rnnt_beam_result(st.beam_state, c["nbest"])
        assert ln[1].tolist() == [0] + [-1] * (c["nbest"] - 1) and sc[1, 0] == 0.0
        for b in (0, 2):
            assert torch.equal(tok[b], before[0][b]) and torch.equal(sc[b], before[2][b])
        tk, ln, sc = st.step(x[:, :c["K"]])     # one more block: the current n-best comes back
        assert tk.shape == (c["B"], c["nbest"], cap) and ln.shape == sc.shape == (c["B"], c["nbest"])
        results.append((toks, tk.cpu().clone(), ln.cpu().clone(), sc.cpu().clone()))
    (ta, ka, la, sa), (tb, kb, lb, sb) = results
    assert ta == tb and torch.equal(la, lb) and torch.equal(sa, sb)
    for b in range(c["B"]):
        for n in range(c["nbest"]):
            k = max(int(la[b, n]), 0)
            assert torch.equal(ka[b, n, :k], kb[b, n, :k])


def test_streaming_without_beam_is_unchanged():
    from statecatcher_amd.streaming import StreamingLucyRNN
    cls, m, jm, x, masks = stream_setup("native", 4)
    st = StreamingLucyRNN(m, batch=3, frames_per_call=2, graph=False, joiner=jm)
    assert st.beam is None and not hasattr(st, "beam_state")
    out = st.step(x[:, :2])
    assert len(out) == 3 and out[0].shape == (3, 2 * 4) and out[2].shape == (3,)
    with pytest.raises(ValueError, match="joiner"):
        StreamingLucyRNN(m, batch=3, frames_per_call=2, graph=False, beam=4)
