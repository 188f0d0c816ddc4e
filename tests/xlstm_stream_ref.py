"""The xLSTM-large encoder restated step by step in torch on the CPU -- TEST INFRASTRUCTURE ONLY.

fp64 by default: the reference of the streaming / inference-mode tests.  Input projection
(optional), embedding Linear, per block RMSNorm -> the six projections -> soft cap 15 on the
gates -> the mLSTM recurrence of oracle/mlstm.py one step at a time -> MultiHeadLayerNorm ->
sigmoid output gate -> out_proj -> residual; RMSNorm -> SwiGLU FFN -> residual; then out_norm,
lm_head and the logit soft cap 30.  A ``live`` mask holds every block's state on frames with 0
(their logits are whatever the held state gives and are not compared).

Pinned by tests/test_xlstm_stream_ref.py against transformers' own xLSTMBlock / xLSTMRMSNorm
composition in fp64 and against oracle.mlstm.mlstm_recurrent.  ``dtype=torch.float32`` runs the
same code in fp32: its distance from the fp64 run is the measured rounding noise the fp32
streaming tests scale their tolerance by.
"""
import torch
import torch.nn.functional as F


def rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def soft_cap(x, cap):
    return cap * torch.tanh(x / cap)


def cell(q, k, v, ig, fg, state, live, eps):
    """oracle/mlstm.py's recurrence in q's dtype, one step at a time.  q, k [B,NH,T,DQ],
    v [B,NH,T,DV], gates [B,NH,T], state (C, n, m [B,NH,1]) or None, live [B,T] bool or None."""
    B, NH, T, DQ = q.shape
    DV = v.shape[-1]
    z = dict(dtype=q.dtype)
    if state is None:
        C, n, m = torch.zeros(B, NH, DQ, DV, **z), torch.zeros(B, NH, DQ, **z), torch.zeros(B, NH, **z)
    else:
        C, n, m = state[0].to(**z), state[1].to(**z), state[2].to(**z).reshape(B, NH)
    s = DQ ** -0.5
    h = torch.zeros(B, NH, T, DV, **z)
    for t in range(T):
        lf = F.logsigmoid(fg[..., t])
        mn = torch.maximum(lf + m, ig[..., t])
        fa, ia = torch.exp(lf + m - mn)[..., None], torch.exp(ig[..., t] - mn)[..., None]
        Cn = fa[..., None] * C + ia[..., None] * (k[..., t, :, None] * v[..., t, None, :])
        nn = fa * n + ia * k[..., t, :]
        qs = q[..., t, :] * s
        den = torch.maximum((qs * nn).sum(-1).abs(), torch.exp(-mn)) + eps
        ht = torch.einsum("bhi,bhij->bhj", qs, Cn) / den[..., None]
        if live is None:
            C, n, m, h[..., t, :] = Cn, nn, mn, ht
        else:
            on = live[:, t].reshape(B, 1)
            C = torch.where(on[..., None, None], Cn, C)
            n = torch.where(on[..., None], nn, n)
            m = torch.where(on, mn, m)
            h[..., t, :] = torch.where(on[..., None], ht, torch.zeros_like(ht))
    return h, (C, n, m[..., None])


def encoder(sd, num_heads, x, state=None, live=None, dtype=torch.float64, input_proj=None,
            gate_cap=15.0, logit_cap=30.0, norm_eps=1e-6, eps=1e-6):
    """sd: an xLSTMLarge state_dict (CPU).  x [B,T,input_dim].  Returns logits [B,T,V] and the
    state {block: (C, n, m)} in ``dtype``."""
    W = lambda name: sd[name].detach().cpu().to(dtype)   # noqa: E731
    NH = num_heads
    h = x.detach().cpu().to(dtype)
    if live is not None:
        live = live.detach().cpu().bool()
    if input_proj is not None:
        h = F.linear(h, input_proj.weight.detach().cpu().to(dtype),
                     input_proj.bias.detach().cpu().to(dtype))
    h = F.linear(h, W("embedding.weight"), W("embedding.bias"))
    B, T, _ = h.shape
    new_state = {}
    nb = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    for i in range(nb):
        p = f"blocks.{i}."
        n = rms(h, W(p + "norm_mlstm.weight"), norm_eps)
        lin = lambda name, bias=False: F.linear(   # noqa: E731
            n, W(p + f"mlstm_layer.{name}.weight"), W(p + f"mlstm_layer.{name}.bias") if bias else None)
        heads = lambda t: t.reshape(B, T, NH, -1).transpose(1, 2)   # noqa: E731
        q, k, v, o = heads(lin("q")), heads(lin("k")), heads(lin("v")), lin("ogate_preact")
        ig = soft_cap(lin("igate_preact", True), gate_cap).transpose(1, 2)
        fg = soft_cap(lin("fgate_preact", True), gate_cap).transpose(1, 2)
        hc, new_state[i] = cell(q, k, v, ig, fg, None if state is None else state.get(i), live, eps)
        hc = hc.transpose(1, 2)                                   # [B,T,NH,DV]
        hn = (hc - hc.mean(-1, keepdim=True)) * torch.rsqrt(
            hc.var(-1, keepdim=True, unbiased=False) + norm_eps)
        hn = hn.reshape(B, T, -1) * W(p + "mlstm_layer.multihead_norm.weight")
        h = h + F.linear(torch.sigmoid(o) * hn, W(p + "mlstm_layer.out_proj.weight"))
        n = rms(h, W(p + "norm_ffn.weight"), norm_eps)
        up = F.silu(F.linear(n, W(p + "ffn.proj_up_gate.weight"))) * F.linear(n, W(p + "ffn.proj_up.weight"))
        h = h + F.linear(up, W(p + "ffn.proj_down.weight"))
    h = rms(h, W("out_norm.weight"), norm_eps)
    return soft_cap(F.linear(h, W("lm_head.weight")), logit_cap), new_state


def tiny_model(embedding_dim=128, num_heads=2, num_blocks=2, input_dim=16, vocab=32, seed=0,
               mode="train"):
    """The tests' tiny xLSTMLarge (CPU, fp32 parameters) with a trained-like spread: random norm
    weights and gate biases, lm_head scaled up so the logits are not all alike."""
    from statecatcher_amd.xlstm import xLSTMLarge, xLSTMLargeConfig
    torch.manual_seed(seed)
    cfg = xLSTMLargeConfig(embedding_dim=embedding_dim, num_heads=num_heads, num_blocks=num_blocks,
                           vocab_size=vocab, input_dim=input_dim, mode=mode,
                           autocast_kernel_dtype="bfloat16")
    model = xLSTMLarge(cfg)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name:
                p.normal_(1.0, 0.1)
            elif name.endswith("gate_preact.bias"):
                p.normal_(0.0, 1.0)
        model.lm_head.weight.mul_(4.0)
    return model
