"""StreamingRWKV and RWKVEncoder.step on the GPU against the held-frame reference
(tests/rwkv_stream_ref.encoder_live: a stream with held frames is the stream with those frames
removed, on the float64 checker of tests/rwkv_ref.py).

Tiny encoders built as tests/test_gpu_rwkv.py::make_encoder builds its own (LayerNorms off their
identity init): d64 (input 16, H 64, A 64, I 128, L 2, V 32), d96 (H 96, A 128, I 264: widths
that are no multiple of 64), L1 (d64 with one layer: pre_ln and ln_out act in one block).
B = 3, T = 70, and the ragged mask of tests/test_gpu_streaming_xlstm.py.

Tolerances.  fp32: tests/test_gpu_rwkv.py::within (8 d32 + 1e-5 scale, d32 the reference's own
float32 run).  bf16: the relative Frobenius error of the live logits against float64 is at most
twice that of the offline bf16-autocast RWKVEncoder.forward on all-live input of the same model,
measured here and printed (the rule of test_bf16_stream_within_twice_the_offline_error).
"""
import pytest
import torch

from tests import rwkv_stream_ref as rs
from tests.test_gpu_rwkv import state_parts, within
from tests.test_gpu_streaming_xlstm import ragged, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DIMS = {"d64": dict(H=64, A=64, I=128, L=2), "d96": dict(H=96, A=128, I=264, L=2),
        "L1": dict(H=64, A=64, I=128, L=1)}
FIN, V, B, T = 16, 32, 3, 70
_CACHE = {}


def sc():
    import statecatcher_amd as s
    return s


def make_encoder(name, fin=FIN, seed=0):
    d = DIMS[name]
    torch.manual_seed(seed)
    enc = sc().RWKVEncoder(sc().RWKVConfig(input_dim=fin, hidden_size=d["H"], num_layers=d["L"],
                                           vocab_size=V, attention_hidden_size=d["A"],
                                           intermediate_size=d["I"]))
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if ".ln" in n or "pre_ln" in n or n.startswith("ln_out"):
                p.add_(0.1 * torch.randn_like(p))
        enc.output_proj.weight.mul_(4.0)   # logits that are not all alike: the decode has tokens
    return enc


def setup(name):
    """(encoder on the GPU, its CPU state_dict), one per configuration."""
    if name not in _CACHE:
        enc = make_encoder(name)
        sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        _CACHE[name] = (enc.to(DEV), sd)
    return _CACHE[name]


def inputs(b=B, t=T, seed=1, fin=FIN):
    return torch.randn(b, t, fin, generator=torch.Generator().manual_seed(seed))


def ref(name, x, live=None, dtype=torch.float64):
    """encoder_live from the zero state, computed once per (model, input, mask, dtype)."""
    key = ("ref", name, tuple(x.shape), float(x.sum()), None if live is None else float(live.sum()),
           dtype)
    if key not in _CACHE:
        _CACHE[key] = rs.encoder_live(setup(name)[1], x, live, dtype=dtype)
    return _CACHE[key]


def stream(name, dtype, K, graph, **kw):
    return sc().StreamingRWKV(setup(name)[0], batch=kw.pop("batch", B), frames_per_call=K,
                              dtype=dtype, graph=graph, **kw)


def check_fp32(tag, logits, state, x, live, name):
    """Live logits and the state parts against the float64 reference under `within`."""
    (w64, s64), (w32, s32) = ref(name, x, live), ref(name, x, live, torch.float32)
    lv = torch.ones(x.shape[:2], dtype=torch.bool) if live is None else live
    print(tag)
    within(logits.cpu()[lv], w64[lv], w32[lv])
    for g, a, b in zip(state_parts(state), state_parts(s64), state_parts(s32)):
        within(g, a, b)


def greedy(logits_b):
    out, prev = [], None
    for t in logits_b.argmax(-1).tolist():
        if t != prev and t != 0:
            out.append(t)
        prev = t
    return out


# ------------------------------------------------------------------------------ fp32 ------
@pytest.mark.parametrize("name,K,graph", [
    ("d64", 1, True), ("d64", 1, False), ("d64", 4, True), ("d64", 4, False),
    ("d96", 4, True), ("d96", 1, False), ("L1", 4, True), ("L1", 1, False)])
def test_fp32_stream_against_ref(name, K, graph):
    x, live = inputs(), ragged(B, T)
    st = stream(name, torch.float32, K, graph)
    assert st.gemm == "frame"
    toks, logits = st.decode(x.to(DEV), live.to(DEV), return_logits=True)
    assert logits.shape == (B, T, V) and logits.dtype == torch.float32
    check_fp32(f"fp32 stream {name} K={K} graph={graph}", logits, st.state(), x, live, name)
    for b in range(B):   # decoder.py's greedy path over the stream's live frames
        assert toks[b] == greedy(logits[b][live[b].to(DEV)])
    assert any(toks)


def test_held_frame_content_is_irrelevant():
    x, live = inputs(), ragged(B, T)
    x2 = x.clone()
    x2[~live] = 3.0 * torch.randn(int((~live).sum()), FIN, generator=torch.Generator().manual_seed(9))
    for dtype, K in ((torch.float32, 4), (torch.bfloat16, 1)):
        runs = []
        for xx in (x, x2):
            st = stream("d64", dtype, K, True)
            toks, logits = st.decode(xx.to(DEV), live.to(DEV), return_logits=True)
            runs.append((toks, logits[live.to(DEV)], st.state()))
        (ta, la, sa), (tb, lb, sb) = runs
        assert ta == tb and torch.equal(la, lb)
        assert all(torch.equal(a, b) for a, b in zip(sa, sb))


# ------------------------------------------------------------------------------ bf16 ------
def yardstick(name):
    """The offline bf16-autocast forward's own error against float64 on all-live input."""
    key = ("yard", name)
    if key not in _CACHE:
        x = inputs()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            logits, _ = setup(name)[0](x.to(DEV))
        _CACHE[key] = rel(logits, ref(name, x)[0])
        print(f"offline bf16 {name} vs fp64 at T={T}: logits {_CACHE[key]:.3e}")
    return _CACHE[key]


@pytest.mark.parametrize("name", ["d64", "d96", "L1"])
def test_bf16_stream_within_twice_the_offline_error(name):
    x, live = inputs(), ragged(B, T)
    e_off = yardstick(name)
    st = stream(name, torch.bfloat16, 4, True)
    toks, logits = st.decode(x.to(DEV), live.to(DEV), return_logits=True)
    e = rel(logits.cpu()[live], ref(name, x, live)[0][live])
    print(f"bf16 stream {name}: live logits {e:.3e} (offline {e_off:.3e})")
    assert e <= 2 * e_off


# ------------------------------------------------------------- graph / block invariance ---
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graph_and_block_invariance_bitwise(dtype):
    t = 24
    x, live = inputs(t=t, seed=2).to(DEV), ragged(B, t).to(DEV)
    runs = {}
    for K, graph in ((4, True), (4, False), (1, True), (1, False)):
        st = stream("d96", dtype, K, graph, gemm="frame")
        toks, logits = st.decode(x, live, return_logits=True)
        runs[K, graph] = (toks, logits, st.state())
    t0, l0, s0 = runs[4, True]
    for key, (tk, lg, s) in runs.items():
        assert tk == t0, key
        assert torch.equal(lg[live], l0[live]), f"logits differ: {key} vs (4, graph)"
        assert all(torch.equal(a, b) for a, b in zip(s, s0)), key


def test_encoder_step_equals_the_stream_bitwise():
    """RWKVEncoder.step at any K on the stream's own snapshot: the same logits and state."""
    t = 13
    enc = setup("d64")[0]
    x, live = inputs(t=t, seed=3).to(DEV), ragged(B, 32)[:, :t].to(DEV)
    live[2, 5:9] = False
    st = stream("d64", torch.bfloat16, 4, True)
    _, want = st.decode(x, live, return_logits=True)
    for cuts in ((0, 13), (0, 1, 6, 13), tuple(range(14))):
        state, parts = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            lg, state = enc.step(x[:, a:b], state, live[:, a:b].float(), st.weights)
            parts.append(lg.clone())
        got = torch.cat(parts, 1)
        assert got.shape == (B, t, V) and got.dtype == torch.float32
        assert torch.equal(got[live], want[live]), cuts
        assert all(torch.equal(a, b) for a, b in zip(state, st.state())), cuts
    # a default snapshot is taken when none is given, and a state of another dtype is refused
    lg, state = enc.step(x[:, :2])
    assert lg.shape == (B, 2, V) and len(state) == 5 and lg.grad_fn is None
    with pytest.raises(ValueError, match="contiguous fp32"):
        enc.step(x[:, :2], tuple(s.double() for s in state))


# ------------------------------------------------------------------------ GEMM engines ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_library_gemm_engine(dtype):
    """gemm="library" (what a model beyond lucy_frame_gemm's limits gets): the same tolerances,
    and graph replay == eager bitwise."""
    name = "d64"
    x, live = inputs(), ragged(B, T)
    out = {}
    for graph in (True, False):
        st = stream(name, dtype, 4, graph, gemm="library")
        assert st.gemm == "library"
        toks, logits = st.decode(x.to(DEV), live.to(DEV), return_logits=True)
        out[graph] = (logits, st.state())
    assert torch.equal(out[True][0][live.to(DEV)], out[False][0][live.to(DEV)])
    assert all(torch.equal(a, b) for a, b in zip(out[True][1], out[False][1]))
    if dtype == torch.float32:
        check_fp32("library GEMM fp32", *out[True], x, live, name)
    else:
        e, e_off = rel(out[True][0].cpu()[live], ref(name, x, live)[0][live]), yardstick(name)
        print(f"library GEMM bf16: live logits {e:.3e} (offline {e_off:.3e})")
        assert e <= 2 * e_off


def test_gemm_engine_limits():
    """An input width of 20 is no multiple of 8: "auto" takes the library engine and "frame" is
    refused with the documented message; the library engine then streams it."""
    key = "odd"
    if key not in _CACHE:
        enc = make_encoder("d64", fin=20, seed=5)
        sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}   # (on the CPU)
        _CACHE[key] = (enc.to(DEV), sd)
    enc, sd = _CACHE[key]
    assert stream("d64", torch.bfloat16, 1, False).gemm == "frame"
    with pytest.raises(ValueError, match='gemm="frame" needs fp32 / bf16 weights and every reduction '
                                         'length a multiple of 8, at most 2048; use gemm="library"'):
        sc().StreamingRWKV(enc, batch=B, gemm="frame", graph=False)
    with pytest.raises(ValueError, match="gemm must be"):
        sc().StreamingRWKV(enc, batch=B, gemm="hipblas", graph=False)
    with pytest.raises(TypeError, match="RWKVEncoder"):
        sc().StreamingRWKV(enc.blocks[0], batch=B)
    t = 9
    x = inputs(t=t, seed=6, fin=20)
    st = sc().StreamingRWKV(enc, batch=B, frames_per_call=4, dtype=torch.float32)
    assert st.gemm == "library"
    _, logits = st.decode(x.to(DEV), return_logits=True)
    (w64, _), (w32, _) = (rs.encoder_live(sd, x, None, dtype=dt) for dt in (torch.float64, torch.float32))
    within(logits, w64, w32)


# ------------------------------------------------------------------------ hand-over ------
def test_handover_offline_to_stream_and_back():
    name, cut = "d64", 33
    enc = setup(name)[0]
    x = inputs(seed=4)
    (w64, s64), (w32, s32) = ref(name, x), ref(name, x, dtype=torch.float32)
    # offline forward on the first 33 frames -> reset(state) -> stream the rest
    with torch.no_grad():
        lgA, state = enc(x[:, :cut].to(DEV))
    st = stream(name, torch.float32, 4, True)
    st.reset(state)
    _, lgB = st.decode(x[:, cut:].to(DEV), return_logits=True)
    print("offline -> stream")
    within(torch.cat([lgA, lgB], 1), w64, w32)
    for g, a, b in zip(state_parts(st.state()), state_parts(s64), state_parts(s32)):
        within(g, a, b)
    # stream the first 33 frames -> state() -> offline forward on the rest
    st.reset()
    _, lgC = st.decode(x[:, :cut].to(DEV), return_logits=True)
    with torch.no_grad():
        lgD, stD = enc(x[:, cut:].to(DEV), st.state())
    print("stream -> offline")
    within(torch.cat([lgC, lgD], 1), w64, w32)
    for g, a, b in zip(state_parts(stD), state_parts(s64), state_parts(s32)):
        within(g, a, b)
    # the reference's own state (float64, on the CPU) is taken too
    _, r33 = rs.encoder_live(setup(name)[1], x[:, :cut], None)
    st.reset(r33)
    _, lgE = st.decode(x[:, cut:].to(DEV), return_logits=True)
    within(lgE, w64[:, cut:], w32[:, cut:])


def test_reset_one_stream():
    name = "d64"
    x = inputs(t=16, seed=5).to(DEV)
    st = stream(name, torch.bfloat16, 4, True)
    _, first = st.decode(x, return_logits=True)
    s_first = st.state()
    st.reset(streams=[1])
    zero = setup(name)[0].zero_state(B, DEV)
    for got, was, z in zip(st.state(), s_first, zero):
        assert torch.equal(got[:, 1], z[:, 1])
        assert torch.equal(got[:, 0], was[:, 0]) and torch.equal(got[:, 2], was[:, 2])
    assert st.prev.tolist()[1] == -1
    _, second = st.decode(x, return_logits=True)
    assert torch.equal(second[1], first[1])          # stream 1 started over
    assert not torch.equal(second[0], first[0])      # the others went on from their state
    cont = stream(name, torch.bfloat16, 4, True)
    cont.decode(x)
    _, ref2 = cont.decode(x, return_logits=True)
    assert torch.equal(second[0], ref2[0]) and torch.equal(second[2], ref2[2])


# ---------------------------------------------------------------------------- decoding ----
def test_decode_tokens_are_the_offline_greedy_decoder():
    x = inputs(seed=7)
    lens = [T, T - 29, T - 15]
    masks = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    for dtype, K in ((torch.float32, 4), (torch.bfloat16, 1)):
        st = stream("d64", dtype, K, True)
        toks, logits = st.decode(x.to(DEV), masks.to(DEV), return_logits=True)
        assert toks == sc().ctc_greedy_decoder(logits, lens) and any(toks)


def test_joiner_tails():
    """The greedy transducer tail and the beam tail on the stream's own logits against their
    offline decoders (as test_joiner_tail of tests/test_gpu_streaming_xlstm.py)."""
    from tests.test_gpu_rnnt_decode import make_joiner
    t, K, ms = 22, 4, 3
    jm = make_joiner("RNNTPredictorJoiner", V, 64, V, 0, seed=4).to(DEV)
    x = inputs(t=t, seed=9)
    lens = [t, t - 5, t]
    masks = torch.arange(t)[None, :] < torch.tensor(lens)[:, None]
    st = stream("d64", torch.float32, K, True, joiner=jm, max_symbols=ms)
    assert st.prev.tolist() == [0] * B
    toks, logits = st.decode(x.to(DEV), masks.to(DEV), return_logits=True)
    assert toks == sc().rnnt_greedy_decoder(logits, jm, torch.tensor(lens), blank=0, max_symbols=ms)
    assert any(toks)
    kw = dict(beam=4, top_k=5, max_symbols=2)
    sb = stream("d64", torch.float32, K, True, joiner=jm, max_frames=32, **kw)
    btoks, blogits = sb.decode(x.to(DEV), masks.to(DEV), return_logits=True)
    assert torch.equal(blogits, logits)
    assert btoks == sc().rnnt_beam_decoder(blogits, jm, torch.tensor(lens), blank=0, **kw)
    with pytest.raises(ValueError, match="joiner"):
        stream("d64", torch.float32, K, False, beam=4)
