"""GPU tests of the greedy transducer decoder (csrc/rnnt_decode.hip) through every layer: the
ctypes op, the dispatcher op, decoder.rnnt_greedy_decoder and StreamingLucyRNN(joiner=...).

The reference is the fp64 restatement tests/rnnt_decode_ref.py.  Tokens, frames and counts must
equal it exactly; that is a fair demand because every case first asserts, on the CPU, that the
smallest top-1 / top-2 logit gap along the reference's path is >= 1e-3 -- about 100x the fp32
error of a 64-term dot product of these magnitudes.  Each case is milliseconds of GPU work.
"""
import functools

import numpy as np
import pytest
import torch

from tests.rnnt_decode_ref import padded, rnnt_greedy_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
MIN_GAP = 1e-3
MS = 3   # max_symbols of the parity cases

# (B, T, V, J, bb, seed): the seed is one for which both CPU preconditions hold in fp32 and bf16
CASES = {
    "fast_v37": (3, 40, 37, 64, 4.5, 0),       # fast path, V not a multiple of the wave size
    "fast_v1024": (2, 24, 1024, 64, 9.0, 4),   # fast path, one row per lane exactly
    "gen_v1030": (2, 24, 1030, 64, 9.0, 0),    # general path, V just over one workgroup's rows
    "gen_j20": (2, 30, 50, 20, 3.5, 0),        # general path, J not a multiple of 4
}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def lengths_of(B, T):
    return [T, T - 7, T // 2][:B]


def as_dtype(a, dtype):
    """The values the kernel sees: rounded to dtype, as fp64 numpy."""
    return torch.as_tensor(a, dtype=torch.float32).to(TDT[dtype]).double().numpy()


@functools.lru_cache(maxsize=None)
def inputs(B, T, V, J, bb, seed, dtype="fp32", blank=0):
    rng = np.random.default_rng(seed)
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


def gpu_decode(E, P, W, bias, dtype="fp32", lengths=None, mask=None, blank=0, max_symbols=MS,
               prev=None, cap=None):
    """One decode on the GPU into -1-filled buffers -> (tokens, frames, counts, prev) numpy."""
    from statecatcher_amd import ops
    dt = TDT[dtype]
    t = lambda a, d=dt: torch.as_tensor(np.array(a)).to(DEV, d)   # noqa: E731
    Ed = E if isinstance(E, torch.Tensor) else t(E)
    B, T = Ed.shape[:2]
    cap = T * max_symbols if cap is None else cap
    tok = torch.full((B, cap), -1, dtype=torch.int32, device=DEV)
    frm = torch.full((B, cap), -1, dtype=torch.int32, device=DEV)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pv = None if prev is None else t(prev, torch.int32)
    ops.rnnt_greedy_decode(Ed, t(P), t(W), t(bias, torch.float32),
                           lengths=None if lengths is None else t(lengths, torch.int64),
                           mask=None if mask is None else t(mask, torch.float32), blank=blank,
                           max_symbols=max_symbols, prev=pv, out=(tok, cnt, frm))
    torch.cuda.synchronize()
    return (tok.cpu().numpy(), frm.cpu().numpy(), cnt.cpu().numpy(),
            None if pv is None else pv.cpu().numpy())


def check(got, ref, cap):
    tok, frm, cnt, _ = got
    np.testing.assert_array_equal(cnt, ref.counts)
    np.testing.assert_array_equal(tok, padded(ref.tokens, cap))   # -1 past counts: untouched
    np.testing.assert_array_equal(frm, padded(ref.frames, cap))


def emission_kinds(ref):
    return {n for per in ref.per_frame for n in per}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_fp64_reference(case, dtype):
    B, T, V, J, bb, seed = CASES[case]
    E, P, W, bias = inputs(B, T, V, J, bb, seed, dtype)
    lens = lengths_of(B, T)
    ref = rnnt_greedy_ref(E, P, W, bias, lens, max_symbols=MS)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    assert {0, 1, 2, MS} <= emission_kinds(ref), emission_kinds(ref)
    check(gpu_decode(E, P, W, bias, dtype, lengths=lens), ref, T * MS)


def test_f16_inputs():
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed, "f16")
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=MS)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    check(gpu_decode(E, P, W, bias, "f16", lengths=lengths_of(B, T)), ref, T * MS)


@pytest.mark.parametrize("where", ["copy_above", "copy_below"])
def test_ties_take_the_lower_index(where):
    """Two identical rows of W and bias that win some nodes: the lower index is emitted."""
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    base = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=MS)
    emitted = [k for row in base.tokens for k in row]
    src = max(set(emitted), key=emitted.count)          # a row that wins nodes
    dup = V - 1 if where == "copy_above" else 1
    assert src not in (0, dup) and 1 < src < V - 1
    W, bias = W.copy(), bias.copy()
    W[dup], bias[dup] = W[src], bias[src]
    lo, hi = min(src, dup), max(src, dup)
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=MS, gap_exclude=[hi])
    wins = sum(k == lo for row in ref.tokens for k in row)
    assert wins > 0 and not any(k == hi for row in ref.tokens for k in row)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    check(gpu_decode(E, P, W, bias, lengths=lengths_of(B, T)), ref, T * MS)


@pytest.mark.parametrize("blank", ["first", "last"])
def test_nan_frame_takes_the_first_index(blank):
    """All logits NaN: index 0 wins (`beats`).  blank = 0: a blank, the frame emits nothing;
    blank = V-1: token 0, max_symbols times."""
    B, T, V, J, bb, seed = CASES["fast_v37"]
    bl = 0 if blank == "first" else V - 1
    E, P, W, bias = inputs(B, T, V, J, bb, seed, blank=bl)
    E = E.copy()
    E[0, 5] = np.nan
    E[2, 0] = np.nan
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), blank=bl, max_symbols=MS)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    assert ref.per_frame[0][5] == (0 if bl == 0 else MS)
    assert bl == 0 or ref.tokens[2][:MS] == [0] * MS
    check(gpu_decode(E, P, W, bias, lengths=lengths_of(B, T), blank=bl), ref, T * MS)


@pytest.mark.parametrize("ms", [1, 8])
def test_max_symbols(ms):
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=ms)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    assert ms != 1 or 1 in emission_kinds(ref)
    check(gpu_decode(E, P, W, bias, lengths=lengths_of(B, T), max_symbols=ms), ref, T * ms)


@pytest.mark.parametrize("case", ["fast_v37", "gen_j20"])
def test_blank_is_the_last_token(case):
    B, T, V, J, bb, seed = CASES[case]
    E, P, W, bias = inputs(B, T, V, J, bb, seed, blank=V - 1)
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), blank=V - 1, max_symbols=MS)
    assert ref.min_gap >= MIN_GAP and ref.counts.min() > 0, ref.min_gap
    check(gpu_decode(E, P, W, bias, lengths=lengths_of(B, T), blank=V - 1), ref, T * MS)


def test_zero_lengths_and_empty_time_axis():
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    lens = [T, 0, T // 2]
    ref = rnnt_greedy_ref(E, P, W, bias, lens, max_symbols=MS)
    assert ref.min_gap >= MIN_GAP and ref.counts[1] == 0
    prev0 = np.array([0, 7, 0], np.int32)
    ref = rnnt_greedy_ref(E, P, W, bias, lens, max_symbols=MS, prev=prev0)
    assert ref.min_gap >= MIN_GAP
    got = gpu_decode(E, P, W, bias, lengths=lens, prev=prev0)
    check(got, ref, T * MS)
    np.testing.assert_array_equal(got[3], ref.prev)
    assert got[3][1] == 7   # a dead stream keeps its prev
    # T = 0: counts zeroed, prev kept, nothing else touched
    tok, frm, cnt, pv = gpu_decode(E[:, :0], P, W, bias, prev=prev0)
    assert tok.shape == (B, 0) and cnt.tolist() == [0, 0, 0] and pv.tolist() == prev0.tolist()


def test_truncation_reports_the_full_count():
    """cap below the emission count: counts is the full count, the first cap tokens are right
    and nothing is written at or beyond cap (sentinels behind the last row stay)."""
    from statecatcher_amd import ops
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    lens = lengths_of(B, T)
    ref = rnnt_greedy_ref(E, P, W, bias, lens, max_symbols=MS)
    cap = 5
    assert ref.min_gap >= MIN_GAP and ref.counts.min() > cap
    t = lambda a, d=torch.float32: torch.as_tensor(np.array(a)).to(DEV, d)   # noqa: E731
    flat = [torch.full((B * cap + 64,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
    tok, frm = (f[:B * cap].view(B, cap) for f in flat)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.rnnt_greedy_decode(t(E), t(P), t(W), t(bias), lengths=t(lens, torch.int64),
                           max_symbols=MS, out=(tok, cnt, frm))
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref.counts)
    np.testing.assert_array_equal(tok.cpu().numpy(), padded(ref.tokens, cap))
    np.testing.assert_array_equal(frm.cpu().numpy(), padded(ref.frames, cap))
    for f in flat:
        assert (f[B * cap:] == -7).all()
    # cap = 0 through the allocating form: only counts
    tok0, cnt0 = ops.rnnt_greedy_decode(t(E), t(P), t(W), t(bias), lengths=t(lens, torch.int64),
                                        max_symbols=MS, cap=0)
    assert tok0.shape == (B, 0)
    np.testing.assert_array_equal(cnt0.cpu().numpy(), ref.counts)


@pytest.mark.parametrize("case", ["fast_v37", "gen_j20"])
@pytest.mark.parametrize("chunk", [1, 5, 7])
def test_chunked_decode_equals_one_shot(case, chunk):
    """prev carried from chunk to chunk, some mask-0 frames in the middle."""
    B, T, V, J, bb, seed = CASES[case]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    lens = lengths_of(B, T)
    mask = np.ones((B, T), np.float32)
    mask[:, 10:13] = 0
    mask[1, 20] = 0
    mask[0, 0] = 0
    ref = rnnt_greedy_ref(E, P, W, bias, lens, mask=mask, max_symbols=MS)
    assert ref.min_gap >= MIN_GAP and ref.counts.min() > 0
    check(gpu_decode(E, P, W, bias, lengths=lens, mask=mask), ref, T * MS)
    prev = np.zeros(B, np.int32)
    toks, frs = [[] for _ in range(B)], [[] for _ in range(B)]
    for t0 in range(0, T, chunk):
        n = min(chunk, T - t0)
        cl = [max(0, min(l - t0, n)) for l in lens]
        tok, frm, cnt, prev = gpu_decode(E[:, t0:t0 + n], P, W, bias, lengths=cl,
                                         mask=mask[:, t0:t0 + n], prev=prev)
        for b in range(B):
            toks[b] += tok[b, :cnt[b]].tolist()
            frs[b] += (frm[b, :cnt[b]] + t0).tolist()
    assert toks == ref.tokens and frs == ref.frames
    np.testing.assert_array_equal(prev, ref.prev)


def test_strided_enc_p():
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=MS)
    wide = torch.full((B, T + 3, J + 24), float("nan"), device=DEV)
    view = wide[:, 2:2 + T, 8:8 + J]
    view.copy_(torch.as_tensor(E.copy()).float())
    assert not view.is_contiguous() and view.stride(2) == 1
    check(gpu_decode(view, P, W, bias, lengths=lengths_of(B, T)), ref, T * MS)


def test_no_host_sync():
    from statecatcher_amd import ops
    B, T, V, J, bb, seed = CASES["fast_v37"]
    E, P, W, bias = inputs(B, T, V, J, bb, seed)
    t = lambda a, d=torch.float32: torch.as_tensor(np.array(a)).to(DEV, d)   # noqa: E731
    args = (t(E), t(P), t(W), t(bias))
    lens, prev = t(lengths_of(B, T), torch.int64), torch.zeros(B, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tok, cnt, frm = ops.rnnt_greedy_decode(*args, lengths=lens, max_symbols=MS, prev=prev,
                                               return_frames=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = rnnt_greedy_ref(E, P, W, bias, lengths_of(B, T), max_symbols=MS)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref.counts)
    np.testing.assert_array_equal(prev.cpu().numpy(), ref.prev)


def test_graph_capture_and_replay():
    """Captured once; each replay decodes what was copied into the static buffers."""
    from statecatcher_amd import ops
    B, T, V, J, bb, _ = CASES["fast_v37"]
    lens = lengths_of(B, T)
    sets = [inputs(B, T, V, J, bb, seed) for seed in (0, 3, 8)]
    refs = [rnnt_greedy_ref(*s, lens, max_symbols=MS) for s in sets]
    assert min(r.min_gap for r in refs) >= MIN_GAP
    assert refs[0].tokens != refs[1].tokens != refs[2].tokens
    t = lambda a, d=torch.float32: torch.as_tensor(np.array(a)).to(DEV, d)   # noqa: E731
    E, P, W, bias = (t(a) for a in sets[0])
    ld = t(lens, torch.int64)
    cap = T * MS
    tok = torch.full((B, cap), -1, dtype=torch.int32, device=DEV)
    frm, cnt = torch.full_like(tok, -1), torch.zeros(B, dtype=torch.int32, device=DEV)
    run = lambda: ops.rnnt_greedy_decode(E, P, W, bias, lengths=ld, max_symbols=MS,   # noqa: E731
                                         out=(tok, cnt, frm))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for s, ref in list(zip(sets, refs))[1:] + [(sets[0], refs[0])]:
        for dst, src in zip((E, P, W, bias), s):
            dst.copy_(t(src))
        tok.fill_(-1)
        frm.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        check((tok.cpu().numpy(), frm.cpu().numpy(), cnt.cpu().numpy(), None), ref, cap)


def make_joiner(cls, D, J, V, blank, seed, bb=1.5, scale=4.0):
    """A joiner whose greedy path mixes blanks and emissions (fresh initialisation gives nearly
    flat logits): built on the CPU so the same weights can be checked there."""
    import statecatcher_amd as sc
    torch.manual_seed(seed)
    jm = getattr(sc, cls)(D, 24, J, V)
    with torch.no_grad():
        jm.joiner.weight.mul_(scale)
        jm.enc_proj.weight.mul_(2.0)
        jm.pred_proj.weight.mul_(2.0)
        jm.joiner.bias[blank] += bb
    return jm


def joiner_reference(jm, enc_p, lens, blank, ms, mask=None):
    with torch.no_grad():
        P = jm.pred_proj(jm.embedding.weight)
    f = lambda a: a.detach().double().cpu().numpy()   # noqa: E731
    return rnnt_greedy_ref(f(enc_p), f(P), f(jm.joiner.weight), f(jm.joiner.bias), lens, mask=mask,
                           blank=blank, max_symbols=ms)


@pytest.mark.parametrize("cls", ["RNNTPredictorJoiner", "RNNTCompactPredictorJoiner"])
def test_rnnt_greedy_decoder_drop_in(cls):
    import statecatcher_amd as sc
    B, T, D, J, V, blank, ms = 3, 40, 16, 64, 37, 0, 4
    jm = make_joiner(cls, D, J, V, blank, seed=5).to(DEV)
    enc_out = torch.randn(B, T, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    lens = lengths_of(B, T)
    with torch.no_grad():
        ref = joiner_reference(jm, jm.enc_proj(enc_out), lens, blank, ms)
    assert ref.min_gap >= MIN_GAP, ref.min_gap
    assert ref.counts.min() > 0 and 0 in emission_kinds(ref)
    toks, frames = sc.rnnt_greedy_decoder(enc_out, jm, torch.tensor(lens), blank=blank,
                                          max_symbols=ms, return_frames=True)
    assert toks == ref.tokens and frames == ref.frames
    assert sc.rnnt_greedy_decoder(enc_out, jm, lens, blank=blank, max_symbols=ms) == ref.tokens


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dispatcher_op_is_bitwise_the_ctypes_path(dtype):
    from statecatcher_amd import ops, torch_library
    B, T, V, J, bb, seed = CASES["fast_v37"]
    dt = TDT[dtype]
    t = lambda a, d=dt: torch.as_tensor(np.array(a)).to(DEV, d)   # noqa: E731
    E, P, W = (t(a) for a in inputs(B, T, V, J, bb, seed)[:3])
    bias = t(inputs(B, T, V, J, bb, seed)[3], torch.float32)
    lens = t(lengths_of(B, T), torch.int64)
    mask = torch.ones(B, T, device=DEV)
    mask[:, 4] = 0
    pa, pb = (torch.full((B,), 2, dtype=torch.int32, device=DEV) for _ in range(2))
    a = ops.rnnt_greedy_decode(E, P, W, bias, lengths=lens, mask=mask, max_symbols=MS, prev=pa,
                               return_frames=True)
    b = torch_library.rnnt_greedy_decode(E, P, W, bias, lengths=lens, mask=mask, max_symbols=MS,
                                         prev=pb, return_frames=True)
    assert torch.equal(a[1], b[1]) and torch.equal(pa, pb) and int(a[1].sum()) > 0
    for r, n in enumerate(a[1].tolist()):
        assert torch.equal(a[0][r, :n], b[0][r, :n]) and torch.equal(a[2][r, :n], b[2][r, :n])
    t2, c2 = torch_library.rnnt_greedy_decode(E, P, W, bias, lengths=lens, mask=mask,
                                              max_symbols=MS, prev=torch.full_like(pa, 2), cap=6)
    assert t2.shape == (B, 6) and torch.equal(c2, a[1])


def tiny_stream_model(seed=0):
    import statecatcher_amd as sc
    torch.manual_seed(seed)
    cfg = sc.LucyRNNConfig(input_dim=16, hidden_dim=32, num_layers=2, vocab_size=32,
                           kernel_impl="native", is_training=False, fused_ops=True,
                           layer_norm=True, stack_order=1)
    m = sc.LucyRNN(cfg)
    with torch.no_grad():   # output_proj starts at zero: give the logits some spread
        m.output_proj.weight.normal_(0.0, 0.5)
        m.output_proj.bias.normal_(0.0, 0.1)
    return m


@pytest.mark.parametrize("engine", ["frame", "library"])
def test_streaming_transducer(engine):
    """StreamingLucyRNN(joiner=...): tokens equal the reference run on the streaming path's own
    logits, identically with the graph on and off; reset(streams=[1]) restarts only stream 1."""
    from statecatcher_amd.streaming import StreamingLucyRNN
    B, K, T, V, J, blank, ms = 3, 4, 14, 32, 64, 0, 3
    m = tiny_stream_model().to(DEV)
    jm = make_joiner("RNNTPredictorJoiner", V, J, V, blank, seed=4).to(DEV)
    x = torch.randn(B, T, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    masks = torch.ones(B, T, dtype=torch.bool, device=DEV)
    masks[1, T - 5:] = False
    results = []
    for graph in (True, False):
        st = StreamingLucyRNN(m, batch=B, frames_per_call=K, graph=graph, engine=engine, joiner=jm,
                              max_symbols=ms)
        assert st.prev.tolist() == [blank] * B
        toks, logits = st.decode(x, masks, return_logits=True)
        enc_p = torch.nn.functional.linear(logits.double(), jm.enc_proj.weight.detach().double(),
                                           jm.enc_proj.bias.detach().double())
        ref = joiner_reference(jm, enc_p, [T] * B, blank, ms, mask=masks.float().cpu().numpy())
        assert ref.min_gap >= MIN_GAP, ref.min_gap
        assert ref.counts.min() > 0 and {0, 1} <= emission_kinds(ref)
        assert toks == ref.tokens
        np.testing.assert_array_equal(st.prev.cpu().numpy(), ref.prev)
        # one more block by hand: step() hands back (tokens, frames, counts)
        st.reset(streams=[1])
        want = ref.prev.copy()
        want[1] = blank
        assert ref.prev[1] != blank
        np.testing.assert_array_equal(st.prev.cpu().numpy(), want)
        tk, fr, ct = st.step(x[:, :K])
        assert tk.shape == fr.shape == (B, K * ms) and ct.shape == (B,)
        results.append((toks, tk.cpu(), fr.cpu(), ct.cpu()))
    (ta, ka, fa, ca), (tb, kb, fb, cb) = results
    assert ta == tb and torch.equal(ca, cb)
    for r, n in enumerate(ca.tolist()):
        assert torch.equal(ka[r, :n], kb[r, :n]) and torch.equal(fa[r, :n], fb[r, :n])


def test_streaming_without_joiner_is_unchanged():
    from statecatcher_amd.streaming import StreamingLucyRNN
    st = StreamingLucyRNN(tiny_stream_model().to(DEV), batch=2, frames_per_call=2, graph=False)
    assert st.joiner is False and not hasattr(st, "enc_p") and st.prev.tolist() == [-1, -1]
    out = st.step(torch.zeros(2, 2, 16, device=DEV))
    assert isinstance(out, torch.Tensor) and out.shape == (2, 2)
