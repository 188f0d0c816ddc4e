"""The RWKV encoder (statecatcher_amd/rwkv.py) on the GPU against the plain-torch encoder of
tests/rwkv_ref.py in float64 and against transformers' recorded outputs (tests/golden/rwkv.npz):
logits and state over carried segments, frame-by-frame inference, the gradients of a CTC loss
through compute_loss, and SegmentTrainer steps in CTC and RNN-T mode."""
import numpy as np
import pytest
import torch

from tests import rwkv_ref as ref
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
S = 64   # ops.WKV_CHUNK
F, H, A, I, L, V, B = 20, 64, 64, 128, 2, 24, 2


def sc():
    import statecatcher_amd
    return statecatcher_amd


def make_encoder(seed=0):
    torch.manual_seed(seed)
    enc = sc().RWKVEncoder(sc().RWKVConfig(input_dim=F, hidden_size=H, num_layers=L, vocab_size=V,
                                           attention_hidden_size=A, intermediate_size=I))
    with torch.no_grad():   # LayerNorms off their identity init, so their parameters matter
        for n, p in enc.named_parameters():
            if ".ln" in n or "pre_ln" in n or n.startswith("ln_out"):
                p.add_(0.1 * torch.randn_like(p))
    return enc


def state_parts(st):
    """The state as comparable tensors: the shift frames, num / den and max + log den."""
    x_att, x_ffn, num, den, mx = (s.double().cpu() for s in st)
    return [x_att, x_ffn, *ref.canonical_state((num, den, mx))]


def within(got, r64, r32, floor=1e-5):
    """max |got - ref64| <= 8 d32 + floor * scale, d32 the float32 checker's own error."""
    got, r64, r32 = (t.double().cpu() for t in (got, r64, r32))
    d32 = float((r32 - r64).abs().max())
    err, scale = float((got - r64).abs().max()), float(r64.abs().max())
    print(f"err {err:.3e} d32 {d32:.3e} scale {scale:.3e} ratio {err / (8 * d32 + floor * scale):.3f}")
    assert err <= 8 * d32 + floor * scale, (err, d32, scale)


@pytest.fixture(scope="module")
def two_segments():
    """The encoder, two input segments and the checker's float64 / float32 runs over them."""
    enc = make_encoder()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, S + 3, F, generator=g), torch.randn(B, 7, F, generator=g)]
    sd = enc.state_dict()
    runs = {}
    for dt in (torch.float64, torch.float32):
        st, outs = None, []
        for x in xs:
            y, st = ref.encoder(sd, x, st, dtype=dt)
            outs.append((y, st))
        runs[dt] = outs
    return enc.to(DEV), xs, runs


def test_logits_and_state_over_two_segments(two_segments):
    enc, xs, runs = two_segments
    st = None
    with torch.no_grad():
        for i, x in enumerate(xs):
            y, st = enc(x.to(DEV), st)
            (y64, s64), (y32, s32) = runs[torch.float64][i], runs[torch.float32][i]
            within(y, y64, y32)
            for g, a, b in zip(state_parts(st), state_parts(s64), state_parts(s32)):
                within(g, a, b)
    assert all(s.shape == (L, B, H) for s in st) and all(s.dtype == torch.float32 for s in st[2:])


def test_frame_by_frame_equals_whole(two_segments):
    enc, xs, runs = two_segments
    x = xs[0].to(DEV)
    st, ys = None, []
    with torch.no_grad():
        for t in range(x.shape[1]):
            y, st = enc(x[:, t:t + 1], st)
            ys.append(y)
    (y64, s64), (y32, s32) = runs[torch.float64][0], runs[torch.float32][0]
    within(torch.cat(ys, 1), y64, y32)
    for g, a, b in zip(state_parts(st), state_parts(s64), state_parts(s32)):
        within(g, a, b)


def test_transformers_fixture_through_load_state_dict():
    """A transformers RWKV-4 stack loaded block for block (identity input / output projections):
    its recorded last_hidden_state over two carried segments, the second started from ITS state
    through state_from_hf, and its final state.  The fixture is float32: d32 is its own distance
    from the float64 checker."""
    z = load_golden("rwkv")
    enc = sc().RWKVEncoder(sc().RWKVConfig(input_dim=32, hidden_size=32, num_layers=2, vocab_size=32,
                                           intermediate_size=64))
    enc.blocks.load_state_dict({k[len("model/blocks."):]: torch.from_numpy(z[k]) for k in z.files
                                if k.startswith("model/blocks.")})
    enc.ln_out.load_state_dict({k[len("model/ln_out."):]: torch.from_numpy(z[k]) for k in z.files
                                if k.startswith("model/ln_out.")})
    with torch.no_grad():
        for proj in (enc.input_proj, enc.output_proj):
            proj.weight.copy_(torch.eye(32))
            proj.bias.zero_()
    sd = enc.state_dict()
    x1, x2 = torch.from_numpy(z["model/x1"]), torch.from_numpy(z["model/x2"])
    h1_64, s1_64 = ref.encoder(sd, x1, None)
    h2_64, s2_64 = ref.encoder(sd, x2, s1_64)
    enc = enc.to(DEV)
    with torch.no_grad():
        h1, s1 = enc(x1.to(DEV))
        h2, s2 = enc(x2.to(DEV), s1)
    within(h1, h1_64, torch.from_numpy(z["model/h1"]))
    within(h2, h2_64, torch.from_numpy(z["model/h2"]))
    hf = [torch.from_numpy(z[f"model/state{i}"]) for i in range(5)]
    fix = sc().RWKVEncoder.state_from_hf(hf)
    for g, a, b in zip(state_parts(s2), state_parts(s2_64), state_parts(fix)):
        within(g, a, b)
    # the round trip through transformers' layout feeds the same state back
    back = sc().RWKVEncoder.state_from_hf(sc().RWKVEncoder.state_to_hf(s1))
    with torch.no_grad():
        h2b, _ = enc(x2.to(DEV), back)
    assert torch.equal(h2b, h2)


def _ctc_batch():
    g = torch.Generator().manual_seed(5)
    T = S + 9
    feats = torch.randn(B, T, F, generator=g)
    masks = torch.ones(B, T, dtype=torch.bool)
    masks[1, T - 11:] = False
    tokens = torch.randint(1, V, (B, 9), generator=g)
    tgt, inl = [9, 6], [T, T - 11]
    tokens[1, 6:] = 0
    return feats, masks, tokens, inl, tgt


@pytest.fixture(scope="module")
def ctc_reference():
    """float64 gradients of the CTC loss through the checker's encoder, once for both dtypes."""
    model = sc().ASRModel(None, make_encoder(3).config, V, F, -1)
    model.encoder.load_state_dict(make_encoder(3).state_dict())
    feats, masks, tokens, inl, tgt = _ctc_batch()
    params = {k: v.detach().double().requires_grad_(True) for k, v in model.encoder.named_parameters()}
    logits, _ = ref.encoder(params, (feats * masks.unsqueeze(-1)).double(), None)
    loss = torch.nn.CTCLoss(blank=0, zero_infinity=True)(logits.log_softmax(-1).transpose(0, 1),
                                                         tokens, inl, tgt)
    loss.backward()
    return model, float(loss), {k: p.grad for k, p in params.items()}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16-autocast"])
def test_ctc_gradients_through_compute_loss(ctc_reference, amp):
    model, ref_loss, ref_grads = ctc_reference
    model = model.to(DEV)
    model.zero_grad(set_to_none=True)
    feats, masks, tokens, inl, tgt = _ctc_batch()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        loss, st, enc_out, _ = sc().compute_loss("ctc", sc().CTCLoss(blank=0, zero_infinity=True),
                                                 model, feats.to(DEV), masks.to(DEV),
                                                 tokens.to(DEV), inl, tgt, 0)
    loss.backward()
    assert enc_out.shape == (B, S + 9, V) and len(st) == 5
    print(f"loss {loss.item():.6f} ref {ref_loss:.6f}")
    if not amp:
        np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-4)
    assert bool(torch.isfinite(loss))
    for k, p in model.encoder.named_parameters():
        assert p.grad is not None, k
        g, r = p.grad.double().cpu().flatten(), ref_grads[k].flatten()
        rel = float((g - r).norm() / r.norm())
        cos = float(torch.dot(g, r) / (g.norm() * r.norm()))
        print(f"{k}: rel Frobenius {rel:.3e} cosine {cos:.6f}")
        if amp:
            assert cos >= 0.999, (k, cos)
        else:
            assert rel <= 1e-3, (k, rel)


@pytest.mark.parametrize("mode", ["ctc", "rnnt"])
def test_segment_trainer_step(mode):
    """begin_batch + two segments with Adam: runs, changes every parameter, carries a detached
    state of the encoder's shape."""
    from statecatcher_amd.model import RNNTPredictorJoiner
    from statecatcher_amd.train import SegmentTrainer
    torch.manual_seed(11)
    model = sc().ASRModel(None, sc().build_rwkv_config(F, V, H, L), V, F, -1).to(DEV)
    joiner = RNNTPredictorJoiner(V, 16, 32, V).to(DEV) if mode == "rnnt" else None
    plist = list(model.parameters()) + (list(joiner.parameters()) if joiner is not None else [])
    opt = torch.optim.Adam(plist, lr=1e-3)
    crit = sc().CTCLoss() if mode == "ctc" else sc().RNNTLoss()
    tr = SegmentTrainer(model, crit, opt, mode=mode, joiner=joiner, amp_dtype=torch.bfloat16)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    T, U = S + 5, 6
    feats = torch.randn(B, T, F, device=DEV)
    masks = torch.ones(B, T, dtype=torch.bool, device=DEV)
    tok = torch.randint(1, V, (B, U), device=DEV)
    tr.begin_batch()
    losses = [tr.train_segment(feats, masks, tok, [T] * B, [U] * B) for _ in range(2)]
    assert all(bool(torch.isfinite(l)) for l in losses)
    st = tr.encoder_state
    assert isinstance(st, tuple) and len(st) == 5 and all(s.shape == (L, B, H) for s in st)
    assert float(st[3].min()) > 0.0   # den: two segments of frames went in
    nxt = sc().detach_states(st)
    assert all(not s.requires_grad for s in nxt)
    for k, v in model.named_parameters():
        assert not torch.equal(v.detach(), before[k]), k
