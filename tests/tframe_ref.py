"""Helpers of the StreamingLucyRNNtriton tests (tests/test_tframe_host.py,
tests/test_gpu_streaming_triton.py), like tests/rnnt_decode_ref.py: the conditioned oracle model
and its per-stream reference on ragged masks."""
import numpy as np
import torch

from oracle import decode as odec
from oracle import lucy_step


def conditioned_params(L, Din, D, V, seed):
    """test_gpu_parity_step.oracle_params' recipe at any size: the reference init, gate planes
    1..6 with 0.1x weights and biases of +-3, informative output projection (out_std 0.3).  There
    the oracle's own fp32 and fp64 runs agree to 7e-7 of max (3 x 128, T 23 and 6 x 512, T 40);
    at the reference init the forward is chaotic."""
    p = lucy_step.init_params(L, Din, D, V, seed=seed, out_std=0.3)
    rng = np.random.default_rng(3)
    for l in range(L):
        W = p[f"W{l}"].reshape(7, D, -1)
        b = p[f"b{l}"].reshape(7, D)
        W[1:] *= 0.1
        b[1:] = 3.0 * (rng.integers(0, 2, (6, D)) * 2 - 1)
    return p


def model_from(p, L, Din, D, V, num_tracks=1):
    """A LucyRNNtriton (CPU) holding the oracle parameters p."""
    import statecatcher_amd as sc
    cfg = sc.LucyRNNConfig(input_dim=Din, hidden_dim=D, num_layers=L, vocab_size=V,
                           kernel_impl="triton", fused_ops=True, layer_norm=False)
    if num_tracks != 1:
        cfg.num_tracks = num_tracks
    m = sc.LucyRNNtriton(cfg)
    if p is None:
        return m
    with torch.no_grad():
        for l in range(L):
            m.tracks[0][l].linear.weight.copy_(torch.from_numpy(p[f"W{l}"]))
            m.tracks[0][l].linear.bias.copy_(torch.from_numpy(p[f"b{l}"]))
            if l < L - 1:
                m.norms[0][l].weight.copy_(torch.from_numpy(p[f"g{l}"]))
                m.norms[0][l].bias.copy_(torch.from_numpy(p[f"be{l}"]))
        m.output_proj.weight.copy_(torch.from_numpy(p["Wo"]))
        m.output_proj.bias.copy_(torch.from_numpy(p["bo"]))
    return m


def ragged_masks(B, T, seed):
    """bool [B, T]: suffix cuts (stream 0 full; lengths 1 and, from 4 streams on, 0 among them)
    and interior holes in every other stream."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    if B > 3:
        lens[3] = 0
    m = np.arange(T)[None, :] < lens[:, None]
    for b in range(0, B, 2):
        n = int(lens[b])
        if n > 4:
            m[b, rng.choice(np.arange(1, n - 1), size=max(1, n // 5), replace=False)] = False
    return m


def oracle_stream(p, x, masks, L, D, state=None):
    """Per stream b: oracle.lucy_step.forward on its live frames only (B = 1), from ``state``
    ((h list, s list) of [B, D]) or zero.  Returns (per-stream live indices, per-stream logits
    [n_b, V], h [L, B, D], s [L, B, D])."""
    B = x.shape[0]
    idx, lg = [], []
    h = np.zeros((L, B, D)) if state is None else np.stack(state[0]).astype(np.float64)
    s = np.zeros((L, B, D)) if state is None else np.stack(state[1]).astype(np.float64)
    for b in range(B):
        live = np.nonzero(masks[b])[0]
        idx.append(live)
        if len(live) == 0:
            lg.append(np.zeros((0, p["bo"].shape[0])))
            continue
        st = None if state is None else ([state[0][l][b:b + 1].astype(np.float32) for l in range(L)],
                                         [state[1][l][b:b + 1].astype(np.float32) for l in range(L)])
        logits, (nh, ns), _, _ = lucy_step.forward(p, x[b:b + 1, live], L, D, st)
        lg.append(logits[0].astype(np.float64))
        for l in range(L):
            h[l, b], s[l, b] = nh[l][0], ns[l][0]
    return idx, lg, h, s


def greedy_live(logits, masks):
    """decoder.py:3-30 (oracle.decode.ctc_greedy) over each stream's live frames of logits
    [B, T, V]."""
    out = []
    for b in range(logits.shape[0]):
        live = np.nonzero(masks[b])[0]
        out.append(odec.ctc_greedy(logits[b:b + 1, live], [len(live)])[0])
    return out
