"""tests/xlstm_stream_ref.py pinned on the host: against transformers' own xLSTMBlock /
xLSTMRMSNorm composition in fp64 (built as tests/test_gpu_c4.py builds it) at T = 64 and 128,
its cell against oracle.mlstm.mlstm_recurrent, and its live mask against the compacted sequence.
Plus the configuration logic that needs no GPU: mode="inference" is accepted, refuses autograd,
and ASRModel pads to 64 only in train mode."""
import numpy as np
import pytest
import torch

from tests import xlstm_stream_ref as xr


def _hf_logits(model, x):
    from transformers import xLSTMConfig
    from transformers.models.xlstm import modeling_xlstm as M
    c = model.config
    cfg = xLSTMConfig(hidden_size=c.embedding_dim, embedding_dim=c.embedding_dim,
                      num_heads=c.num_heads, num_blocks=c.num_blocks, vocab_size=c.vocab_size,
                      mode="train", chunkwise_kernel="chunkwise--native_autograd",
                      autocast_kernel_dtype="float32", return_last_states=True,
                      # (its default casts every norm's input to fp32, also in an fp64 module:
                      # off here, so that the composition really is fp64)
                      norm_reduction_force_float32=False)
    sd = model.state_dict()
    hf = torch.nn.ModuleList([M.xLSTMBlock(cfg) for _ in range(c.num_blocks)]).double()
    hf.load_state_dict({k[len("blocks."):]: v.double() for k, v in sd.items()
                        if k.startswith("blocks.")})
    norm = M.xLSTMRMSNorm(c.embedding_dim, eps=cfg.norm_eps, force_float32_reductions=False).double()
    norm.load_state_dict({"weight": sd["out_norm.weight"].double()})
    with torch.no_grad():
        h = torch.nn.functional.linear(x.double(), sd["embedding.weight"].double(),
                                       sd["embedding.bias"].double())
        states = {}
        for i, blk in enumerate(hf):
            h, states[i] = blk(h)
        out = torch.nn.functional.linear(norm(h), sd["lm_head.weight"].double())
    return 30.0 * torch.tanh(out / 30.0), states


@pytest.mark.parametrize("dims", [(128, 2), (192, 1)], ids=["d128-nh2", "d192-nh1"])
@pytest.mark.parametrize("T", [64, 128])
def test_ref_equals_transformers_fp64(T, dims):
    model = xr.tiny_model(embedding_dim=dims[0], num_heads=dims[1], seed=T + dims[0])
    x = torch.randn(2, T, 16, generator=torch.Generator().manual_seed(T))
    want, hf_states = _hf_logits(model, x)
    got, states = xr.encoder(model.state_dict(), dims[1], x)
    err = float((got - want).abs().max())
    print(f"ref vs transformers fp64, T={T} {dims}: max |d logits| {err:.2e} of {float(want.abs().max()):.2f}")
    assert err <= 1e-9 * max(1.0, float(want.abs().max()))
    for i, st in hf_states.items():      # same stabilised state convention
        for a, b in zip(states[i], st):
            scale = max(1.0, float(b.abs().max()))
            assert float((a - b.reshape(a.shape)).abs().max()) <= 1e-9 * scale


def test_ref_cell_is_the_oracle_recurrence():
    from oracle.mlstm import mlstm_recurrent
    g = torch.Generator().manual_seed(4)
    B, NH, T, DQ, DV = 2, 2, 37, 32, 64
    q, k = torch.randn(B, NH, T, DQ, generator=g).double(), torch.randn(B, NH, T, DQ, generator=g).double()
    v = torch.randn(B, NH, T, DV, generator=g).double()
    ig, fg = 4 * torch.randn(B, NH, T, generator=g).double(), 4 * torch.randn(B, NH, T, generator=g).double() + 2
    st = (torch.randn(B, NH, DQ, DV, generator=g).double(), torch.randn(B, NH, DQ, generator=g).double(),
          3 * torch.randn(B, NH, 1, generator=g).double())
    h, (C, n, m) = xr.cell(q, k, v, ig, fg, st, None, 1e-6)
    rh, (rC, rn, rm) = mlstm_recurrent(*(t.numpy() for t in (q, k, v, ig, fg, *st)))
    for a, b in ((h, rh), (C, rC), (n, rn), (m, rm)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-12, atol=1e-300)


def test_ref_live_mask_holds_the_state():
    model = xr.tiny_model(seed=5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 12, 16, generator=g)
    live = torch.tensor([[1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0], [1] * 12], dtype=torch.bool)
    got, st = xr.encoder(model.state_dict(), 2, x, live=live)
    idx = live[0]
    want, st0 = xr.encoder(model.state_dict(), 2, x[:1, idx])
    assert torch.allclose(got[0, idx], want[0], rtol=1e-12, atol=1e-12)
    for i in st:
        for a, b in zip(st[i], st0[i]):
            assert torch.allclose(a[:1], b, rtol=1e-12, atol=1e-14)
    full, st1 = xr.encoder(model.state_dict(), 2, x[1:])
    assert torch.equal(got[1:], full)


# ------------------------------------------------------------------ configuration logic ---
def test_inference_mode_is_accepted_and_refuses_autograd():
    from statecatcher_amd.model import build_xlstm_config
    from statecatcher_amd.xlstm import xLSTMLargeConfig
    assert build_xlstm_config(16, 32).mode == "train"
    assert xLSTMLargeConfig(embedding_dim=128, num_heads=2, num_blocks=1, vocab_size=8).mode == "train"
    model = xr.tiny_model(mode="inference")
    assert model.config.mode == "inference"
    with pytest.raises(RuntimeError, match="no backward"):
        model(torch.randn(1, 5, 16))


@pytest.mark.parametrize("mode,T,want", [("train", 70, 128), ("train", 64, 64),
                                         ("inference", 70, 70), ("inference", 1, 1)])
def test_asr_model_pads_only_in_train_mode(mode, T, want):
    """The shape logic of ASRModel.forward with a stub in the encoder's place."""
    from statecatcher_amd.model import ASRModel
    from statecatcher_amd.xlstm import xLSTMLargeConfig
    cfg = xLSTMLargeConfig(embedding_dim=32, num_heads=2, num_blocks=1, vocab_size=8, input_dim=16,
                           mode=mode)
    model = ASRModel(None, cfg, vocab_size=8, feat_dim=16, proj_dim=-1)
    seen = {}

    def stub(feats, states=None):
        seen["x"] = feats
        return feats[..., :8], {}
    model.encoder.forward = stub
    feats = torch.ones(2, T, 16)
    mask = torch.ones(2, T, dtype=torch.bool)
    mask[1, T // 2:] = False
    logits, _ = model(feats, mask)
    assert seen["x"].shape[1] == want and logits.shape[1] == want
    assert not seen["x"][1, T // 2:].any() and seen["x"][0, :T].all()   # the mask multiply
    if want > T:
        assert not seen["x"][:, T:].any()
