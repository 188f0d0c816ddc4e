"""The RWKV encoder with held frames, for the streaming tests -- TEST INFRASTRUCTURE ONLY.

encoder_live() is defined by one property: a stream with held frames equals the same stream with
those frames removed.  So it gathers each stream's live frames, runs the checker's encoder
(tests/rwkv_ref.encoder, unchanged) on them with B = 1, and scatters the logits back; the rows of
held frames are zero and are not to be compared.  A stream with no live frame returns the state
it came with.  Run in float32 it measures its own rounding noise (the ``d32`` of the GPU tests'
bounds), as rwkv_ref does.
"""
import torch

from tests import rwkv_ref


def zero_state(sd, B, dtype=torch.float64):
    """(x_att, x_ffn, num, den, max), each [L,B,C]: the state before the first frame."""
    L = 1 + max(int(n.split(".")[1]) for n in sd if n.startswith("blocks."))
    H = sd["ln_out.weight"].shape[0]
    A = sd["blocks.0.attention.time_decay"].shape[0]
    z = lambda C: torch.zeros(L, B, C, dtype=dtype)   # noqa: E731
    return z(H), z(H), z(A), z(A), torch.full((L, B, A), rwkv_ref.EMPTY_MAX, dtype=dtype)


def encoder_live(sd, x, live, state=None, dtype=torch.float64):
    """sd: an RWKVEncoder state_dict (CPU).  x [B,T,input_dim]; live [B,T] (bool or 0 / 1), None =
    all live.  Returns (logits [B,T,V], zero rows on held frames; (x_att, x_ffn, num, den, max)
    each [L,B,C]) in ``dtype``."""
    x = x.detach().cpu()
    B, T, _ = x.shape
    live = torch.ones(B, T, dtype=torch.bool) if live is None else live.detach().cpu().bool()
    V = sd["output_proj.weight"].shape[0]
    st0 = zero_state(sd, B, dtype) if state is None else \
        tuple(s.detach().cpu().to(dtype) for s in state)
    logits = torch.zeros(B, T, V, dtype=dtype)
    out = [s.clone() for s in st0]
    for b in range(B):
        idx = live[b].nonzero().flatten()
        if idx.numel() == 0:
            continue
        y, st = rwkv_ref.encoder(sd, x[b:b + 1, idx], tuple(s[:, b:b + 1] for s in st0),
                                 dtype=dtype)
        logits[b, idx] = y[0]
        for o, s in zip(out, st):
            o[:, b] = s[:, 0]
    return logits, tuple(out)
