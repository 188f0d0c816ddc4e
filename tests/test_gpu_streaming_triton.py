"""GPU parity of StreamingLucyRNNtriton (statecatcher_amd/streaming.py; the FR_CELL_T epilogue of
csrc/lucy_frame.hip): the LucyRNNtriton encoder decoded frame by frame, one launch per layer and
frame.

* the reference module's own goldens (tests/golden/module.npz, Din 10: the padded layer-0 path),
  two segments on one object, under tests.conftest.assert_ref_parity;
* the conditioned oracle model on ragged masks (suffix cuts of length 0 and 1, interior holes):
  per stream, oracle.lucy_step.forward on its live frames only; rtol 1e-4 + 1e-4 max|ref| (the
  native streaming tests' tolerance; the conditioned oracle's own fp32-vs-fp64 noise is 7e-7 of
  max);
* wavefront == frame-by-frame schedule and hipGraph on == off, bitwise;
* hand-over between the offline forward and the stream, both ways; reset of one stream; blocks;
* bf16 weights against the offline module's own bf16-autocast drift;
* the transducer tail against tests/rnnt_decode_ref on the stream's own logits.
Tokens are always bit-exact with oracle/decode.py on the GPU's own logits.
"""
import numpy as np
import pytest
import torch

from oracle import decode as odec
from oracle import lucy_step
from tests.conftest import assert_ref_parity, load_golden
from tests.tframe_ref import (conditioned_params, greedy_live, model_from, oracle_stream,
                              ragged_masks)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def to_np(t):
    return t.detach().double().cpu().numpy()


def close(got, ref, rtol=1e-4, afrac=1e-4):
    got = to_np(got) if isinstance(got, torch.Tensor) else got
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=afrac * max(np.abs(ref).max(), 1e-30))


def stream_cls():
    from statecatcher_amd.streaming import StreamingLucyRNNtriton
    return StreamingLucyRNNtriton


def copy_state(state):
    """LucyRNNtriton.forward writes the new state into the lists it is given."""
    return [[t.clone() for t in trk] for trk in state[0]], [[t.clone() for t in trk] for trk in state[1]]


# ------------------------------------------------------------------------ reference goldens ---
@pytest.mark.parametrize("name", ["d64_init", "d64_proj"])
@pytest.mark.parametrize("K,graph", [(1, True), (4, True), (3, False)])
def test_streaming_vs_reference_module_goldens(name, K, graph):
    """Din 10, D 64, L 3, B 2, T 11: seg0 from zero state, seg1 on the same object without a
    reset.  T is no multiple of 4 or 3: the padded frames are masked and must not disturb the
    state seg1 continues from.

    Measured on MI355X (identical for K = 1, 4, 3; |gpu - ref64| / reference fp32 noise /
    fraction within 1e-3 of the reference's fp32 run):
      d64_init  every tensor 1.0000 (h 2.3e-4 / 1.5e-4, 2.8e-4 / 3.3e-4)
      d64_proj  seg0 logits 1.02e-3 / 1.13e-3 / 1.0000   h 6.6e-4 / 7.3e-4 / 1.0000   s 1.0000
                seg1 logits 2.79e-3 / 3.03e-3 / 0.9962   h 1.07e-3 / 1.49e-3 / 1.0000   s 1.0000
    At the reference init fp32 rounding is amplified to ~1e-3 (the "noise"), and the element-wise
    half of the check is sensitive to the summation ORDER of layer 0's gate projection (the numpy
    oracle in fp32 on these goldens: k-ascending fma chain, which is what a BLAS sgemm computes,
    1.0000 on every tensor; layer 0's GEMM computed exactly in fp64 and rounded once, 0.9394 on
    the seg1 logits; split accumulators 0.8144).  The kernel therefore sums each K slice of the
    fp32 projection in ascending k on one accumulator (csrc/lucy_frame.hip, KORD); with two
    interleaved accumulators it measured 0.8712 on the seg1 logits."""
    from tests.test_gpu_parity_step import load_module_case
    z = load_golden("module")
    m, L = load_module_case(z, name)
    st = stream_cls()(m, batch=2, frames_per_call=K, graph=graph)
    assert (st.graph is not None) == graph and st.Dp == 16
    checks = []
    for seg in range(2):
        x = torch.from_numpy(z[f"{name}/seg{seg}/x"]).to(DEV)
        toks, logits = st.decode(x, return_logits=True)
        h, s = st.state()
        pre = f"{name}/seg{seg}/"
        for got, key in [(logits, "logits"), (torch.stack(h[0]), "h"), (torch.stack(s[0]), "s")]:
            g, r32, r64 = to_np(got), z[pre + key].astype(np.float64), z[pre + key + "64"]
            scale = max(1.0, float(np.abs(r32).max()))
            frac = float((np.abs(g - r32) <= 1e-3 * np.abs(r32) + 1e-4 * scale).mean())
            print(f"{name} K={K} seg{seg} {key}: |gpu - ref64| {np.abs(g - r64).max():.2e}, "
                  f"reference fp32 noise {np.abs(r32 - r64).max():.2e}, within 1e-3 of ref fp32: "
                  f"{frac:.4f}")
            checks.append((g, r32, r64))   # (asserted below: every figure is printed first)
        lg = logits.cpu().numpy()
        # (the decode carries prev across the segments: compare per segment from a fresh prev)
        if seg == 0:
            assert toks == odec.ctc_greedy(lg, [lg.shape[1]] * 2)
            lg0 = lg
        else:
            both = odec.ctc_greedy(np.concatenate([lg0, lg], 1), [lg0.shape[1] + lg.shape[1]] * 2)
            assert [a + b for a, b in zip(toks0, toks)] == both
        toks0 = toks
        assert h[0][0].dtype == torch.float32
    for g, r32, r64 in checks:
        assert_ref_parity(g, r32, r64)


# ------------------------------------------------------------------------- oracle, ragged ---
@pytest.mark.parametrize("Din,D,B", [(40, 128, 5), (10, 48, 17), (16, 1024, 2)])
def test_streaming_vs_oracle_ragged(Din, D, B):
    """D 48: three record blocks (odd); B 17: two row blocks, the second ragged; D 1024: exactly
    64 records."""
    L, V, T = 3, 50, 23
    p = conditioned_params(L, Din, D, V, seed=D + B)
    m = model_from(p, L, Din, D, V).to(DEV)
    x = np.random.default_rng(B).standard_normal((B, T, Din)).astype(np.float32)
    masks = ragged_masks(B, T, seed=D)
    live = masks.sum(1)
    assert live[0] > 1 and 1 in live and (B < 4 or 0 in live)
    assert any((np.diff(mk.astype(int)) == 1).any() for mk in masks)   # an interior hole
    idx, rl, rh, rs = oracle_stream(p, x, masks, L, D)
    for K, graph, sched in ((1, True, "frame"), (4, True, "wavefront"), (2, False, "wavefront")):
        st = stream_cls()(m, batch=B, frames_per_call=K, graph=graph, schedule=sched)
        toks, logits = st.decode(torch.from_numpy(x).to(DEV), torch.from_numpy(masks).to(DEV),
                                 return_logits=True)
        lg = logits.cpu().numpy()
        scale = max(np.abs(r).max() for r in rl if len(r))
        for b in range(B):
            if len(idx[b]):
                np.testing.assert_allclose(lg[b, idx[b]], rl[b], rtol=1e-4, atol=1e-4 * scale)
        h, s = st.state()
        close(torch.stack(h[0]), rh)
        close(torch.stack(s[0]), rs)
        assert toks == greedy_live(lg, masks)


def test_more_than_64_records_and_large_lds():
    """D 1040: 65 statistics records per row (the prologue's serial combine path) and A rows
    beyond the default LDS window."""
    L, Din, D, V, B, T = 2, 8, 1040, 20, 3, 5
    p = conditioned_params(L, Din, D, V, seed=1)
    m = model_from(p, L, Din, D, V).to(DEV)
    x = np.random.default_rng(1).standard_normal((B, T, Din)).astype(np.float32)
    masks = np.ones((B, T), bool)
    masks[1, 3:] = False
    _, rl, rh, rs = oracle_stream(p, x, masks, L, D)
    st = stream_cls()(m, batch=B, frames_per_call=2)
    _, logits = st.decode(torch.from_numpy(x).to(DEV), torch.from_numpy(masks).to(DEV),
                          return_logits=True)
    close(logits[0], rl[0])
    close(logits[1, :3], rl[1])
    h, s = st.state()
    close(torch.stack(h[0]), rh)
    close(torch.stack(s[0]), rs)


# ------------------------------------------------------------------------------ schedules ---
def random_model(L, Din, D, V, seed):
    torch.manual_seed(seed)
    m = model_from(None, L, Din, D, V)
    with torch.no_grad():   # the reference zero-inits output_proj; make the logits informative
        m.output_proj.weight.normal_(0.0, 0.05)
    return m.to(DEV)


@pytest.mark.parametrize("L,D,V,B,K,dtype", [
    (6, 512, 1024, 77, 8, torch.float32), (6, 512, 1024, 77, 2, torch.float32),
    (6, 512, 1024, 77, 8, torch.bfloat16), (6, 512, 1024, 77, 2, torch.bfloat16),
    (10, 64, 40, 3, 3, torch.float32)])
def test_wavefront_equals_frame_schedule_and_graph_equals_eager(L, D, V, B, K, dtype):
    """Same kernel, same arithmetic per (layer, frame): logits, tokens and state BITWISE equal
    between the wavefront (multi-job launches, one projection over the block) and the
    frame-by-frame schedule, and with the hipGraph on and off.  K = 2 < L; L = 10 has more than
    8 active layers in a stage (the launch splits)."""
    m = random_model(L, 80, D, V, seed=21)
    T = 20
    g = torch.Generator().manual_seed(L + K)
    x = torch.randn(B, T, 80, generator=g).to(DEV)
    lens = torch.randint(0, T + 1, (B,), generator=g)
    masks = (torch.arange(T)[None, :] < lens[:, None]).to(DEV)
    out = []
    for sched, graph in (("wavefront", True), ("frame", True), ("wavefront", False)):
        st = stream_cls()(m, B, K, dtype=dtype, schedule=sched, graph=graph)
        toks, lg = st.decode(x, masks, return_logits=True)
        out.append((toks, lg, st.state()))
    assert torch.isfinite(out[0][1]).all() and float(out[0][1].abs().max()) > 0
    assert out[0][0] == odec.ctc_greedy(out[0][1].cpu().numpy(), lens.numpy())
    for toks, lg, (h, s) in out[1:]:
        assert toks == out[0][0]
        assert torch.equal(lg, out[0][1])
        for a, b in zip(h[0] + s[0], out[0][2][0][0] + out[0][2][1][0]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------ hand-over ---
def test_handover_between_offline_forward_and_stream():
    """offline model(xA) -> st.reset(state) -> stream xB == offline model(xB, state); then
    st.state() -> model(xC, ...) == the oracle continuing through all three segments."""
    L, Din, D, V, B, T = 3, 40, 128, 50, 5, 7
    p = conditioned_params(L, Din, D, V, seed=5)
    m = model_from(p, L, Din, D, V).to(DEV)
    rng = np.random.default_rng(9)
    xa, xb, xc = (rng.standard_normal((B, T, Din)).astype(np.float32) for _ in range(3))
    full = np.ones((B, T), bool)
    _, _, ha, sa = oracle_stream(p, xa, full, L, D)
    _, lb, hb, sb = oracle_stream(p, xb, full, L, D, (list(ha), list(sa)))
    _, lc, hc, sc_ = oracle_stream(p, xc, full, L, D, (list(hb), list(sb)))
    dev = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    with torch.no_grad():
        _, state_a = m(dev(xa))
        lg_off, state_b = m(dev(xb), copy_state(state_a))
    st = stream_cls()(m, batch=B, frames_per_call=4)
    st.reset(state_a)
    _, lg = st.decode(dev(xb), return_logits=True)
    close(lg, to_np(lg_off))
    close(lg, np.stack(lb))
    h, s = st.state()
    close(torch.stack(h[0]), to_np(torch.stack(state_b[0][0])))
    close(torch.stack(s[0]), to_np(torch.stack(state_b[1][0])))
    close(torch.stack(h[0]), hb)
    with torch.no_grad():
        lg_c, state_c = m(dev(xc), st.state())
    close(lg_c, np.stack(lc))
    close(torch.stack(state_c[0][0]), hc)
    close(torch.stack(state_c[1][0]), sc_)


def test_reset_subset_and_blocks_equal_one_pass():
    """Feeding an utterance in two calls equals one call; resetting one stream mid-utterance
    restarts only that stream (its tokens equal a fresh decoder's)."""
    p = conditioned_params(2, 20, 64, 12, seed=5)
    m = model_from(p, 2, 20, 64, 12).to(DEV)
    x = torch.randn(3, 16, 20, generator=torch.Generator().manual_seed(5)).to(DEV)
    cls = stream_cls()
    one = cls(m, 3, 4)
    e_all = torch.cat([one.step(x[:, i:i + 4]).clone() for i in range(0, 16, 4)], 1)
    assert (e_all >= 0).any()
    whole = cls(m, 3, 16)
    assert torch.equal(whole.step(x), e_all)
    for a, b in zip(whole.state()[0][0] + whole.state()[1][0], one.state()[0][0] + one.state()[1][0]):
        assert torch.equal(a, b)
    two = cls(m, 3, 4)
    for i in range(0, 8, 4):
        two.step(x[:, i:i + 4])
    two.reset(streams=[1])
    e_tail = torch.cat([two.step(x[:, i:i + 4]).clone() for i in range(8, 16, 4)], 1)
    fresh = cls(m, 3, 4)
    e_fresh = torch.cat([fresh.step(x[:, i:i + 4]).clone() for i in range(8, 16, 4)], 1)
    assert torch.equal(e_tail[[0, 2]], e_all[[0, 2], 8:])
    assert torch.equal(e_tail[1], e_fresh[1])


# ----------------------------------------------------------------------------------- bf16 ---
def test_bf16_stream_tracks_fp32_stream():
    """bf16 weights (fp32 activations and state): the relative L2 drift of the logits from the
    fp32 stream is at most 1.5x the drift of the offline module under bf16 autocast from its own
    fp32 run on the same input, plus 1e-3 (the native bf16 test's form; the yardstick is the
    existing offline code)."""
    L, Din, D, V, B, T = 6, 80, 512, 256, 8, 40
    p = conditioned_params(L, Din, D, V, seed=3)
    m = model_from(p, L, Din, D, V).to(DEV)
    x = torch.randn(B, T, Din, generator=torch.Generator().manual_seed(3)).to(DEV)
    _, l32 = stream_cls()(m, B, 8).decode(x, return_logits=True)
    st16 = stream_cls()(m, B, 8, dtype=torch.bfloat16)
    _, l16 = st16.decode(x, return_logits=True)
    rel = float((l16 - l32).norm() / l32.norm())
    with torch.no_grad():
        o32 = m(x)[0].float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o16 = m(x)[0].float()
    rel_ac = float((o16 - o32).norm() / o32.norm())
    print(f"bf16 stream drift {rel:.3e}; offline bf16 autocast drift {rel_ac:.3e}")
    assert rel <= 1.5 * rel_ac + 1e-3, (rel, rel_ac)
    h, s = st16.state()
    for t in h[0] + s[0]:
        assert t.dtype == torch.float32 and torch.isfinite(t).all()


# ----------------------------------------------------------------------------- transducer ---
RNNT = dict(B=3, K=4, T=14, V=32, J=64, Din=16, D=32, L=2, blank=0, ms=3, seed=1, jseed=4)


def rnnt_case():
    from tests.test_gpu_rnnt_decode import make_joiner
    c = RNNT
    p = conditioned_params(c["L"], c["Din"], c["D"], c["V"], seed=c["seed"])
    jm = make_joiner("RNNTPredictorJoiner", c["V"], c["J"], c["V"], c["blank"], seed=c["jseed"])
    x = torch.randn(c["B"], c["T"], c["Din"], generator=torch.Generator().manual_seed(3))
    masks = torch.ones(c["B"], c["T"], dtype=torch.bool)
    masks[1, c["T"] - 5:] = False
    return p, jm, x, masks


def rnnt_reference(jm, logits, masks):
    from tests.test_gpu_rnnt_decode import joiner_reference
    c = RNNT
    enc_p = torch.nn.functional.linear(torch.as_tensor(logits).double().cpu(),
                                       jm.enc_proj.weight.detach().double().cpu(),
                                       jm.enc_proj.bias.detach().double().cpu())
    return joiner_reference(jm, enc_p, [c["T"]] * c["B"], c["blank"], c["ms"],
                            mask=masks.float().cpu().numpy())


def test_streaming_transducer():
    """joiner=RNNTPredictorJoiner: tokens, counts and prev equal the fp64 reference decode of the
    streaming path's own logits, identically with the graph on and off.  Exact equality is
    demanded only where the reference path's smallest top-1 / top-2 gap is >= 1e-3, asserted
    first; the seed is one where the CPU oracle's logits give a gap >= 1e-2 and every stream
    emits (checked here before the GPU runs)."""
    c = RNNT
    p, jm, x, masks = rnnt_case()
    lg_cpu = lucy_step.forward(p, x.numpy(), c["L"], c["D"])[0]
    pre = rnnt_reference(jm, lg_cpu, masks)
    assert pre.min_gap >= 1e-2 and pre.counts.min() > 0, (pre.min_gap, pre.counts)
    m = model_from(p, c["L"], c["Din"], c["D"], c["V"]).to(DEV)
    jd = jm.to(DEV)
    results = []
    for graph in (True, False):
        st = stream_cls()(m, batch=c["B"], frames_per_call=c["K"], graph=graph, joiner=jd,
                          max_symbols=c["ms"])
        assert st.prev.tolist() == [c["blank"]] * c["B"]
        toks, logits = st.decode(x.to(DEV), masks.to(DEV), return_logits=True)
        ref = rnnt_reference(jd, logits, masks)
        assert ref.min_gap >= 1e-3, ref.min_gap
        assert toks == ref.tokens
        np.testing.assert_array_equal([len(t) for t in toks], ref.counts)
        np.testing.assert_array_equal(st.prev.cpu().numpy(), ref.prev)
        tk, fr, ct = st.step(x[:, :c["K"]].to(DEV))
        assert tk.shape == fr.shape == (c["B"], c["K"] * c["ms"]) and ct.shape == (c["B"],)
        results.append((toks, tk.cpu(), fr.cpu(), ct.cpu()))
    (ta, ka, fa, ca), (tb, kb, fb, cb) = results
    assert ta == tb and torch.equal(ca, cb)
    for r, n in enumerate(ca.tolist()):
        assert torch.equal(ka[r, :n], kb[r, :n]) and torch.equal(fa[r, :n], fb[r, :n])
