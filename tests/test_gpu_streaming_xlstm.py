"""StreamingXLSTM, xLSTMLarge.step and mode="inference" on the GPU against the fp64 restatement
of the encoder (tests/xlstm_stream_ref.py, pinned to transformers on the host).

Tiny model: embedding_dim 128, 2 heads (DQ 32, DV 64), 2 blocks, input_dim 16, V 32; one case at
1 head x 192 (DQ 96, DV 192) and one at 4 heads x 256 (the projection width is then a multiple
of 8: the step kernel reads q / k / v / gates in place, as at C4).

Tolerances.  fp32 stream: the error of the SAME restatement run in fp32 on the CPU against its
fp64 run, times 4 (the GPU GEMMs sum in another order), floor 1e-6 of max |logits|.  bf16: the
relative Frobenius error against fp64 is at most 2x that of the offline bf16-autocast
xLSTMLarge.forward (the rule of tests/test_gpu_c4.py), measured on the same model.
"""
import pytest
import torch

from tests import xlstm_stream_ref as xr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DIMS = {"d128-nh2": (128, 2), "d192-nh1": (192, 1), "d256-nh4": (256, 4)}
_CACHE = {}


def sc():
    import statecatcher_amd as s
    return s


def setup(name="d128-nh2", mode="train"):
    """(model on the GPU, its CPU state_dict, num_heads), one per configuration."""
    key = (name, mode)
    if key not in _CACHE:
        d, nh = DIMS[name]
        model = xr.tiny_model(embedding_dim=d, num_heads=nh, seed=3, mode=mode)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _CACHE[key] = (model.to(DEV), sd, nh)
    return _CACHE[key]


def inputs(B, T, seed=1):
    return torch.randn(B, T, 16, generator=torch.Generator().manual_seed(seed))


def ragged(B, T):
    """Stream 0 whole, stream 1 ends early, stream 2 has held frames inside and ends early."""
    m = torch.ones(B, T, dtype=torch.bool)
    m[1, T - 29:] = False
    if B > 2:
        m[2, 5:9] = False
        m[2, T - 15:] = False
    return m


def ref(name, x, live=None, state=None, dtype=torch.float64):
    key = ("ref", name, tuple(x.shape), float(x.sum()), None if live is None else float(live.sum()),
           state is None, dtype)
    if key not in _CACHE or state is not None:
        _, sd, nh = setup(name)
        out = xr.encoder(sd, nh, x, state=state, live=live, dtype=dtype)
        if state is not None:
            return out
        _CACHE[key] = out
    return _CACHE[key]


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def state_rel(got, want):
    """Relative Frobenius error of (C, n) over all blocks after rescaling to the reference's m,
    and the largest |m - m_ref|."""
    num = den = 0.0
    dm = 0.0
    for i in want:
        C, n, m = (t.detach().double().cpu() for t in got[i])
        rC, rn, rm = (t.detach().double().cpu() for t in want[i])
        m = m.reshape(rm.shape)
        s = torch.exp(m - rm)
        num += float((C * s[..., None] - rC).pow(2).sum() + (n * s - rn).pow(2).sum())
        den += float(rC.pow(2).sum() + rn.pow(2).sum())
        dm = max(dm, float((m - rm).abs().max()))
    return (num / den) ** 0.5, dm


def offline_bf16(name, x, state=None):
    model, _, _ = setup(name)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return model(x.to(DEV), state)


def yardstick(name):
    """The offline bf16 forward's own error against fp64 at T = 128 (logits; state)."""
    key = ("yard", name)
    if key not in _CACHE:
        x = inputs(3, 128)
        logits, st = offline_bf16(name, x)
        want, wst = ref(name, x)
        _CACHE[key] = (rel(logits, want), state_rel(st, wst)[0])
        print(f"offline bf16 {name} vs fp64 at T=128: logits {_CACHE[key][0]:.3e}, state {_CACHE[key][1]:.3e}")
    return _CACHE[key]


def stream(name, dtype, K, graph, **kw):
    model, _, _ = setup(name)
    return sc().StreamingXLSTM(model, batch=kw.pop("batch", 3), frames_per_call=K, dtype=dtype,
                               graph=graph, **kw)


# ------------------------------------------------------------------------------ fp32 ------
@pytest.mark.parametrize("name,K,graph", [
    ("d128-nh2", 1, True), ("d128-nh2", 1, False), ("d128-nh2", 4, True), ("d128-nh2", 4, False),
    ("d192-nh1", 4, True), ("d256-nh4", 4, True)])
def test_fp32_stream_against_ref(name, K, graph):
    B, T = 3, 70
    x, live = inputs(B, T), ragged(B, T)
    want, _ = ref(name, x, live)
    noise32, _ = ref(name, x, live, dtype=torch.float32)
    lv = live[..., None].expand_as(want)
    noise = float((noise32.double() - want)[lv].abs().max())
    tol = max(4 * noise, 1e-6 * float(want[lv].abs().max()))
    st = stream(name, torch.float32, K, graph)
    toks, logits = st.decode(x.to(DEV), live.to(DEV), return_logits=True)
    err = float((logits.double().cpu() - want)[lv].abs().max())
    print(f"fp32 stream {name} K={K} graph={graph}: max |d logits| {err:.3e}, fp32-restatement "
          f"noise {noise:.3e}, allowed {tol:.3e}")
    assert logits.shape == (B, T, 32) and err <= tol
    # the decode: decoder.py's greedy path over each stream's live frames of these logits
    for b in range(B):
        am = logits[b][live[b].to(DEV)].argmax(-1).tolist()
        exp, prev = [], None
        for t in am:
            if t != prev and t != 0:
                exp.append(t)
            prev = t
        assert toks[b] == exp


# ------------------------------------------------------------------------------ bf16 ------
@pytest.mark.parametrize("name", ["d128-nh2", "d192-nh1", "d256-nh4"])
def test_bf16_stream_within_twice_the_offline_error(name):
    B, T = 3, 128
    x = inputs(B, T)
    want, wst = ref(name, x)
    e_off, s_off = yardstick(name)
    st = stream(name, torch.bfloat16, 4, True)
    toks, logits = st.decode(x.to(DEV), return_logits=True)
    e, (s, dm) = rel(logits, want), state_rel(st.state(), wst)
    print(f"bf16 stream {name}: logits {e:.3e} (offline {e_off:.3e}), state {s:.3e} "
          f"(offline {s_off:.3e}), |dm| {dm:.2e}")
    assert e <= 2 * e_off and s <= 2 * s_off
    tk, ct = sc().ctc_greedy_decode(logits, [T] * B)
    tk, ct = tk.cpu(), ct.cpu()
    assert toks == [tk[b, :ct[b]].tolist() for b in range(B)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_library_gemm_engine(dtype):
    """gemm="library" (the GEMMs autocast would run; what a model beyond lucy_frame_gemm's limits
    gets): the same tolerances, graph replay == eager bitwise, and K = 4 against K = 1 to the
    same tolerance (the library picks its kernel by the row count: not bitwise)."""
    name, B, T = "d128-nh2", 3, 128
    x = inputs(B, T)
    want, _ = ref(name, x)
    out = {}
    for K, graph in ((4, True), (4, False), (1, True)):
        st = stream(name, dtype, K, graph, gemm="library")
        assert st.gemm == "library"
        out[K, graph] = st.decode(x.to(DEV), return_logits=True)[1]
    assert torch.equal(out[4, True], out[4, False])
    if dtype == torch.bfloat16:
        e_off, _ = yardstick(name)
        errs = [rel(o, want) for o in out.values()]
        print(f"library GEMM bf16: {errs} (offline {e_off:.3e})")
        assert max(errs) <= 2 * e_off
    else:
        noise32, _ = ref(name, x, dtype=torch.float32)
        tol = max(4 * float((noise32.double() - want).abs().max()), 1e-6 * float(want.abs().max()))
        errs = [float((o.double().cpu() - want).abs().max()) for o in out.values()]
        print(f"library GEMM fp32: {errs} (allowed {tol:.3e})")
        assert max(errs) <= tol


def test_gemm_engine_limits():
    model, _, _ = setup("d128-nh2")
    assert stream("d128-nh2", torch.bfloat16, 1, False).gemm == "frame"
    from statecatcher_amd.xlstm import step_gemm_frame_ok
    assert step_gemm_frame_ok(768, 2048, 80) and not step_gemm_frame_ok(4096) and not step_gemm_frame_ok(20)
    with pytest.raises(ValueError):
        stream("d128-nh2", torch.bfloat16, 1, False, gemm="hipblas")


# ------------------------------------------------------------- graph / block invariance ---
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graph_and_block_invariance_bitwise(dtype):
    B, T = 3, 24
    x, live = inputs(B, T, seed=2).to(DEV), ragged(B, T).to(DEV)
    runs = {}
    for K, graph in ((4, True), (4, False), (1, True), (1, False)):
        st = stream("d128-nh2", dtype, K, graph)
        toks, logits = st.decode(x, live, return_logits=True)
        runs[K, graph] = (toks, logits, st.state())
    t0, l0, s0 = runs[4, True]
    for key, (t, l, s) in runs.items():
        assert t == t0, key
        assert torch.equal(l[live], l0[live]), f"logits differ: {key} vs (4, graph)"
        for i in s0:
            for a, b in zip(s[i], s0[i]):
                assert torch.equal(a, b), (key, i)


# ------------------------------------------------------------------------ hand-over ------
def test_handover_offline_to_stream_and_back():
    name, B = "d128-nh2", 3
    x = inputs(B, 165, seed=4)
    want, _ = ref(name, x)
    e_off, s_off = yardstick(name)
    # offline 128 frames -> reset(states) -> stream 37 frames
    lg128, states = offline_bf16(name, x[:, :128])
    st = stream(name, torch.bfloat16, 4, True)
    st.reset(states)
    _, lg37 = st.decode(x[:, 128:].to(DEV), return_logits=True)
    e1 = rel(lg37, want[:, 128:])
    # stream 37 frames -> state() -> offline 64 frames
    st.reset()
    _, lgA = st.decode(x[:, :37].to(DEV), return_logits=True)
    lgB, stB = offline_bf16(name, x[:, 37:101], st.state())
    e2, e3 = rel(lgA, want[:, :37]), rel(lgB, want[:, 37:101])
    _, wst = ref(name, x[:, :101])
    s3, _ = state_rel(stB, wst)
    print(f"hand-over: offline->stream {e1:.3e}, stream {e2:.3e}, stream->offline {e3:.3e} "
          f"(offline alone {e_off:.3e}); state {s3:.3e} (offline alone {s_off:.3e})")
    assert max(e1, e2, e3) <= 2 * e_off and s3 <= 2 * s_off
    # fp32 stream from an fp64-exact state: within the fp32 tolerance of the ref on the tail
    _, rst = ref(name, x[:, :128])
    want_tail, _ = ref(name, x[:, 128:], state=rst)
    noise_tail, _ = ref(name, x[:, 128:], state=rst, dtype=torch.float32)
    tol = max(4 * float((noise_tail.double() - want_tail).abs().max()),
              1e-6 * float(want_tail.abs().max()))
    st32 = stream(name, torch.float32, 4, True)
    st32.reset(rst)
    _, lg = st32.decode(x[:, 128:].to(DEV), return_logits=True)
    err = float((lg.double().cpu() - want_tail).abs().max())
    print(f"fp32 stream from the reference's state: {err:.3e} (allowed {tol:.3e})")
    assert err <= tol


def test_reset_one_stream():
    name, B = "d128-nh2", 3
    x = inputs(B, 16, seed=5).to(DEV)
    st = stream(name, torch.bfloat16, 4, True)
    _, first = st.decode(x, return_logits=True)
    s_first = st.state()
    st.reset(streams=[1])
    for i, (C, n, m) in st.state().items():
        assert not C[1].any() and not n[1].any() and not m[1].any()
        for a, b in zip((C, n, m), s_first[i]):
            assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert st.prev.tolist()[1] == -1
    _, second = st.decode(x, return_logits=True)
    assert torch.equal(second[1], first[1])          # stream 1 started over
    assert not torch.equal(second[0], first[0])      # the others went on from their state
    cont = stream(name, torch.bfloat16, 4, True)
    cont.decode(x)
    _, ref2 = cont.decode(x, return_logits=True)
    assert torch.equal(second[0], ref2[0]) and torch.equal(second[2], ref2[2])


# ------------------------------------------------------------------- inference mode ------
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_inference_mode_any_length(T):
    name = "d128-nh2"
    model, sd, nh = setup(name)
    inf, _, _ = setup(name, mode="inference")
    inf.load_state_dict(model.state_dict())
    x = inputs(3, T, seed=6)
    e_off, s_off = yardstick(name)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits, st = inf(x.to(DEV))
    want, wst = ref(name, x)
    e, (s, dm) = rel(logits, want), state_rel(st, wst)
    print(f"inference mode T={T}: logits {e:.3e} (offline {e_off:.3e}), state {s:.3e} "
          f"(offline {s_off:.3e})")
    assert logits.shape == (3, T, 32)
    assert e <= 2 * e_off and s <= 2 * s_off


def test_inference_mode_is_train_mode_on_whole_chunks_and_refuses_grad():
    name = "d128-nh2"
    model, _, _ = setup(name)
    inf, _, _ = setup(name, mode="inference")
    inf.load_state_dict(model.state_dict())
    x = inputs(2, 128, seed=7).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        a, sa = model(x)
        b, sb = inf(x)
    assert torch.equal(a, b)
    for i in sa:
        for u, v in zip(sa[i], sb[i]):
            assert torch.equal(u, v)
    with pytest.raises(RuntimeError, match="no backward"):
        inf(x[:, :70])
    with pytest.raises(ValueError):      # train mode keeps its T % 64 rule
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            model(x[:, :70])


def test_zero_padding_is_state_active():
    """ASRModel at T = 70.  mode="inference" returns 70 frames and the state the stream reaches;
    mode="train" pads to 128 with zero frames, which advance the state: it ends elsewhere.  (The
    defect the step path removes.)"""
    from statecatcher_amd.model import ASRModel
    name = "d128-nh2"
    model, sd, nh = setup(name)
    x = inputs(3, 70, seed=8)
    asr = {}
    for mode in ("train", "inference"):
        m = ASRModel(None, setup(name, mode)[0].config, vocab_size=32, feat_dim=16, proj_dim=-1).to(DEV)
        m.encoder.load_state_dict(model.state_dict())
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            asr[mode] = m(x.to(DEV), torch.ones(3, 70, dtype=torch.bool, device=DEV))
    assert asr["inference"][0].shape[1] == 70 and asr["train"][0].shape[1] == 128
    st = stream(name, torch.bfloat16, 1, True)
    st.decode(x.to(DEV))
    streamed = st.state()
    _, wst = ref(name, x)
    _, s_off = yardstick(name)
    d_inf, _ = state_rel(asr["inference"][1], streamed)
    d_train, dm_train = state_rel(asr["train"][1], streamed)
    e_stream, _ = state_rel(streamed, wst)
    print(f"state at T=70 vs the stream's: inference mode {d_inf:.3e}, padded train mode "
          f"{d_train:.3e} (|dm| {dm_train:.2f}); stream vs fp64 {e_stream:.3e}")
    assert e_stream <= 2 * s_off and d_inf <= 4 * s_off     # two bf16 runs of the same state
    assert d_train > 10 * max(d_inf, s_off) and d_train > 1e-2


# ------------------------------------------------------------------------ transducer ------
def test_joiner_tail():
    from tests.test_gpu_rnnt_decode import joiner_reference, make_joiner
    name, B, T, K, ms = "d128-nh2", 3, 22, 4, 3
    jm = make_joiner("RNNTPredictorJoiner", 32, 64, 32, 0, seed=4).to(DEV)
    x = inputs(B, T, seed=9)
    masks = torch.ones(B, T, dtype=torch.bool)
    masks[1, T - 5:] = False
    st = stream(name, torch.float32, K, True, joiner=jm, max_symbols=ms)
    assert st.prev.tolist() == [0] * B
    toks, logits = st.decode(x.to(DEV), masks.to(DEV), return_logits=True)
    with torch.no_grad():
        fref = joiner_reference(jm, jm.enc_proj(logits), [T, T - 5, T], 0, ms)
    assert fref.min_gap >= 1e-3 and fref.counts.min() > 0, (fref.min_gap, fref.counts)
    assert toks == fref.tokens
    lens = torch.tensor([T, T - 5, T])
    assert toks == sc().rnnt_greedy_decoder(logits, jm, lens, blank=0, max_symbols=ms)
