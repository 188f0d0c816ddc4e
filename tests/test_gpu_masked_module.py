"""mask_mode="hold" of LucyRNNtriton and masking="hold" of ASRModel on the GPU: a masked frame
leaves the carried (h, s) untouched, as the streaming classes already treat it.  The reference is
the oracle on each stream's live frames (tests/tframe_ref.oracle_stream), at
test_streaming_vs_oracle_ragged's bound for the same comparison."""
import numpy as np
import pytest
import torch

from tests import scan_mask_cases as mc
from tests.tframe_ref import model_from, oracle_stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _np(t):
    return t.detach().float().cpu().numpy()


def close(got, ref, rtol=1e-4, afrac=1e-4):
    np.testing.assert_allclose(_np(got) if isinstance(got, torch.Tensor) else got, ref, rtol=rtol,
                               atol=afrac * max(np.abs(ref).max(), 1e-30))


def _model(p, cfg, mode):
    Din, D, B, L, V, T = cfg
    m = model_from(p, L, Din, D, V).to(DEV)
    m.mask_mode = mode
    return m


def _check_segment(logits, state, masks, idx, rl, rh, rs):
    lg = _np(logits)
    scale = max(np.abs(r).max() for r in rl if len(r))
    for b in range(masks.shape[0]):
        if len(idx[b]):
            np.testing.assert_allclose(lg[b, idx[b]], rl[b], rtol=1e-4, atol=1e-4 * scale)
    close(torch.stack(state[0][0]), rh)
    close(torch.stack(state[1][0]), rs)


@pytest.mark.parametrize("cfg", mc.MODULE_CASES)
def test_hold_matches_the_per_stream_oracle_over_two_segments(cfg):
    """Logits at live frames and the final (h, s) against the per-stream oracle, then a second
    segment from the carried state in which row 2 is all padding (the "padding" batch strategy:
    zero features, an all-false mask): its state must come out as it went in.  With the mask
    ignored (the parent commit) the padded frames step the recurrence and wipe the state."""
    Din, D, B, L, V, T = cfg
    p, x, masks, _ = mc.module_inputs(*cfg)
    m = _model(p, cfg, "hold")
    xd, md = torch.from_numpy(x).to(DEV), torch.from_numpy(masks).to(DEV)
    with torch.no_grad():
        logits, state = m(xd * md.unsqueeze(-1), None, masks=md)
    idx, rl, rh, rs = oracle_stream(p, x, masks, L, D)
    _check_segment(logits, state, masks, idx, rl, rh, rs)
    assert state[0][0][0].dtype == torch.float32
    # segment 2, carried state; row 2 all held, row 0 a held prefix
    x2 = np.random.default_rng(B + 7).standard_normal((B, T, Din)).astype(np.float32)
    masks2 = masks[::-1].copy()
    masks2[2] = False
    masks2[0, :3] = False
    before = [[t.clone() for t in state[0][0]], [t.clone() for t in state[1][0]]]
    x2d, m2d = torch.from_numpy(x2).to(DEV), torch.from_numpy(masks2).to(DEV)
    with torch.no_grad():
        logits2, state2 = m(x2d * m2d.unsqueeze(-1), state, masks=m2d)
    idx2, rl2, rh2, rs2 = oracle_stream(p, x2, masks2, L, D, (list(rh), list(rs)))
    _check_segment(logits2, state2, masks2, idx2, rl2, rh2, rs2)
    for l in range(L):
        assert torch.equal(state2[0][0][l][2], before[0][l][2])
        assert torch.equal(state2[1][0][l][2], before[1][l][2])
    assert float(torch.stack(before[1]).abs()[:, 2].max()) > 1e-3   # (there was a state to keep)


@pytest.mark.parametrize("cfg", mc.MODULE_CASES)
def test_ignore_is_the_unmasked_forward(cfg):
    """mask_mode="ignore" (the default) with masks given is bitwise the call without masks."""
    Din, D, B, L, V, T = cfg
    p, x, masks, w = mc.module_inputs(*cfg)
    m = _model(p, cfg, "ignore")
    assert model_from(None, L, Din, D, V).mask_mode == "ignore"
    xd, md = torch.from_numpy(x).to(DEV), torch.from_numpy(masks).to(DEV)
    outs = []
    for kw in ({}, {"masks": md}):
        m.zero_grad()
        logits, (h, s) = m(xd, None, **kw)
        (logits * torch.from_numpy(w).to(DEV)).sum().backward()
        outs.append([logits, *h[0], *s[0]] + [q.grad.clone() for q in m.parameters()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cfg", mc.MODULE_CASES)
def test_hold_parameter_gradients(cfg):
    """fp32 parameter gradients of a loss on the live logits against torch_ref.lucyrnn64 autograd
    (fp64) on each row's live frames, summed over rows: relative L2 per parameter within 4 x the
    error of that same restatement run in fp32 on the CPU on these inputs
    (test_scan_mask_checker.test_module_gradient_restatement_error measures it: 8e-8 .. 1.0e-6;
    the factor 4 is scan_cases.C's: hardware rsq / rcp / exp2, another order of composition)."""
    Din, D, B, L, V, T = cfg
    p, x, masks, w = mc.module_inputs(*cfg)
    g64 = mc.ref_param_grads(p, x, masks, w, L, D, torch.float64)
    g32 = mc.ref_param_grads(p, x, masks, w, L, D, torch.float32)
    m = _model(p, cfg, "hold")
    xd, md = torch.from_numpy(x).to(DEV), torch.from_numpy(masks).to(DEV)
    logits, _ = m(xd * md.unsqueeze(-1), None, masks=md)
    (logits * torch.from_numpy(w).to(DEV)).sum().backward()
    got = {k: _np(v.grad).astype(np.float64) for k, v in m.named_parameters()}
    assert set(got) == set(g64)
    rows = {k: (mc.rel_l2(got[k], g64[k]), 4 * mc.rel_l2(g32[k], g64[k])) for k in g64}
    print(f"{cfg}: rel L2 (kernel, bound) " + ", ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in rows.items()))
    bad = {k: v for k, v in rows.items() if not v[0] <= v[1]}
    assert not bad, bad


def _asr(masking, hidden=128, layers=2, V=32, seed=3):
    from statecatcher_amd.model import ASRModel, CTCLoss, build_lucyrnn_config
    from statecatcher_amd.train import SegmentTrainer
    torch.manual_seed(seed)
    model = ASRModel(None, build_lucyrnn_config(80, hidden, layers, V), vocab_size=V, feat_dim=80,
                     proj_dim=-1, masking=masking).to(DEV)
    with torch.no_grad():
        model.encoder.output_proj.weight.normal_(0, 0.02)
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=3e-4)
    tr = SegmentTrainer(model, CTCLoss(blank=0, zero_infinity=True), opt, amp_dtype=torch.bfloat16,
                        max_grad_norm=50.0)
    return tr, model, params


def _padded_segments(n, B, T, V, U, seed):
    """Ragged segments: row 1 ends inside segment 0 and is all padding afterwards."""
    g = torch.Generator().manual_seed(seed)
    segs = []
    for i in range(n):
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        lens[0] = T
        lens[1] = T // 3 if i == 0 else 0
        tl = torch.minimum(torch.randint(U // 2, U + 1, (B,), generator=g), lens // 4)
        tok = torch.randint(1, V, (B, U), generator=g)
        for b in range(B):
            tok[b, tl[b]:] = 0
        masks = torch.arange(T)[None, :] < lens[:, None]
        feats = torch.randn(B, T, 80, generator=g) * masks.unsqueeze(-1)
        segs.append(dict(feats=feats.to(DEV), masks=masks.to(DEV), tokens=tok.to(DEV),
                         in_lens=lens.to(DEV), tgt_lens=tl.to(DEV)))
    return segs


def test_asr_model_hold_under_autocast_with_the_fused_head():
    """ASRModel(masking="hold") + compute_loss, CTC, bf16 autocast, fused head: a finite loss, a
    fully padded row's state exactly kept, and weight gradients bitwise indifferent to what the
    padded frames' features hold."""
    from statecatcher_amd.model import compute_loss
    B, T, V, U = 4, 130, 32, 8
    tr, model, params = _asr("hold")
    segs = _padded_segments(2, B, T, V, U, seed=11)

    def run(noise):
        state, grads, losses = None, [], []
        for s in segs:
            feats = s["feats"]
            if noise:
                g = torch.Generator().manual_seed(5)
                feats = torch.where(s["masks"].unsqueeze(-1), feats,
                                    torch.randn(B, T, 80, generator=g).to(DEV) * 7)
            model.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss, state_out, _, _ = compute_loss("ctc", tr.criterion, model, feats, s["masks"],
                                                     s["tokens"], s["in_lens"], s["tgt_lens"], 0,
                                                     input_state=state)
            loss.backward()
            losses.append(loss.detach().clone())
            grads.append([q.grad.clone() for q in params])
            if state is not None:   # row 1 is all padding in segment 1
                for l in range(len(state[0][0])):
                    assert torch.equal(state_out[0][0][l][1], state[0][0][l][1])
                    assert torch.equal(state_out[1][0][l][1], state[1][0][l][1])
            state = state_out
        return losses, grads

    losses, grads = run(False)
    assert all(torch.isfinite(x) for x in losses)
    assert all(torch.isfinite(q).all() for gs in grads for q in gs)
    assert any(float(q.abs().max()) > 0 for q in grads[1])
    _, noisy = run(True)   # (ASRModel zeroes the padded features itself)
    for ga, gb in zip(grads, noisy):
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_graphed_segments_with_hold_masking_bitwise_as_eager():
    from statecatcher_amd.graphs import GraphedSegments
    n, B, T, V, U = 2, 4, 130, 32, 8
    segs = _padded_segments(n, B, T, V, U, seed=12)
    tr, _, p_eager = _asr("hold")
    l_eager = []
    for k in range(2 * n):
        if k % n == 0:
            tr.begin_batch()
        s = segs[k % n]
        l_eager.append(tr.train_segment(s["feats"], s["masks"], s["tokens"], s["in_lens"],
                                        s["tgt_lens"]).detach().clone())
    torch.cuda.synchronize()
    tr2, _, p_graph = _asr("hold")
    gs = GraphedSegments(tr2, segs).capture()
    l_graph = []
    for k in range(2 * n):
        if k % n == 0:
            gs.begin_batch()
        l_graph.append(gs.step().detach().clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in l_eager)
    assert all(torch.equal(a, b) for a, b in zip(l_eager, l_graph))
    assert all(torch.equal(a, b) for a, b in zip(p_eager, p_graph))
