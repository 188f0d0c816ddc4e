"""The RWKV-4 encoder on the HIP WKV kernels (csrc/wkv.hip), stateful over segments.

The reference's README names RWKV among its recurrent encoders ("Planned/WiP": its code has
none).  This is the RWKV-4 block stack of transformers' ``RwkvModel`` (modeling_rwkv.py: RwkvBlock,
RwkvSelfAttention, RwkvFeedForward) behind an input projection in place of the token embedding and
an output projection to the vocabulary, with the encoders' calling convention here:
``forward(x [B,T,input_dim], state=None) -> (logits [B,T,vocab], state)``.

``blocks`` carries transformers' parameter names and shapes, so
``encoder.blocks.load_state_dict(hf_model.blocks.state_dict())`` loads a published RWKV-4 stack.

The state is a tuple ``(x_att, x_ffn, num, den, max)``, each ``[L, B, C]``: the last post-ln1 and
post-ln2 frame of every block (what the time-shift mixes read at the next segment's first frame)
and the WKV state (fp32).  Any T >= 1: a sequence fed in pieces with the state carried equals the
sequence fed whole, down to one frame at a time.  The WKV operator runs on ``ops.wkv``; the
linears, LayerNorms and elementwise mixes are PyTorch's.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import ops

EMPTY_MAX = -1e38   # transformers' sentinel for the empty WKV state


@dataclass
class RWKVConfig:
    input_dim: int
    hidden_size: int
    num_layers: int
    vocab_size: int
    attention_hidden_size: Optional[int] = None   # None: hidden_size
    intermediate_size: Optional[int] = None       # None: 4 * hidden_size
    layer_norm_epsilon: float = 1e-5
    return_last_states: bool = True


def _shift(x, prev):
    """x delayed by one frame, its first frame taken from the carried ``prev`` [B,C]."""
    return torch.cat([prev.to(x.dtype).unsqueeze(1), x[:, :-1]], 1)


def _mix(x, shifted, m):
    return x * m + shifted * (1 - m)


class RWKVSelfAttention(nn.Module):
    """transformers' RwkvSelfAttention (time mix): parameter names and shapes kept."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H = cfg.hidden_size
        A = cfg.attention_hidden_size or H
        L = cfg.num_layers
        self.time_decay = nn.Parameter(torch.empty(A))
        self.time_first = nn.Parameter(torch.empty(A))
        self.time_mix_key = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_value = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_receptance = nn.Parameter(torch.empty(1, 1, H))
        self.key = nn.Linear(H, A, bias=False)
        self.value = nn.Linear(H, A, bias=False)
        self.receptance = nn.Linear(H, A, bias=False)
        self.output = nn.Linear(A, H, bias=False)
        # the published RWKV-4 initialisation
        r0 = layer_id / max(L - 1, 1)
        r1 = 1.0 - layer_id / L
        x = (torch.arange(H, dtype=torch.float64) / H).reshape(1, 1, H)
        h = torch.arange(A, dtype=torch.float64)
        with torch.no_grad():
            self.time_decay.copy_(-5.0 + 8.0 * (h / max(A - 1, 1)) ** (0.7 + 1.3 * r0))
            self.time_first.copy_(math.log(0.3) + ((h + 1) % 3 - 1) * 0.5)
            self.time_mix_key.copy_(x ** r1)
            self.time_mix_value.copy_(x ** r1 + 0.3 * r0)
            self.time_mix_receptance.copy_(x ** (0.5 * r1))

    def forward(self, x, x_prev, wkv_state):
        s = _shift(x, x_prev)
        k = self.key(_mix(x, s, self.time_mix_key))
        v = self.value(_mix(x, s, self.time_mix_value))
        r = torch.sigmoid(self.receptance(_mix(x, s, self.time_mix_receptance)))
        if v.dtype != k.dtype:
            v = v.to(k.dtype)
        y, wkv_state = ops.wkv(self.time_decay, self.time_first, k, v, wkv_state)
        return self.output(r * y.to(r.dtype)), wkv_state


class RWKVFeedForward(nn.Module):
    """transformers' RwkvFeedForward (channel mix, squared ReLU)."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H = cfg.hidden_size
        I = cfg.intermediate_size or 4 * H
        self.time_mix_key = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_receptance = nn.Parameter(torch.empty(1, 1, H))
        self.key = nn.Linear(H, I, bias=False)
        self.receptance = nn.Linear(H, H, bias=False)
        self.value = nn.Linear(I, H, bias=False)
        r1 = 1.0 - layer_id / cfg.num_layers
        x = (torch.arange(H, dtype=torch.float64) / H).reshape(1, 1, H)
        with torch.no_grad():
            self.time_mix_key.copy_(x ** r1)
            self.time_mix_receptance.copy_(x ** r1)

    def forward(self, x, x_prev):
        s = _shift(x, x_prev)
        k = torch.square(torch.relu(self.key(_mix(x, s, self.time_mix_key))))
        r = torch.sigmoid(self.receptance(_mix(x, s, self.time_mix_receptance)))
        return r * self.value(k)


class RWKVBlock(nn.Module):
    """transformers' RwkvBlock: (pre_ln at layer 0,) ln1 + attention, ln2 + feed_forward, residuals."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H, eps = cfg.hidden_size, cfg.layer_norm_epsilon
        if layer_id == 0:
            self.pre_ln = nn.LayerNorm(H, eps=eps)
        self.ln1 = nn.LayerNorm(H, eps=eps)
        self.ln2 = nn.LayerNorm(H, eps=eps)
        self.attention = RWKVSelfAttention(cfg, layer_id)
        self.feed_forward = RWKVFeedForward(cfg, layer_id)
        self.layer_id = layer_id

    def forward(self, h, x_att, x_ffn, wkv_state):
        """h [B,T,H]; x_att / x_ffn [B,H]; wkv_state (num, den, max) [B,A].  Returns (h, last
        post-ln1 frame, last post-ln2 frame, wkv state)."""
        if self.layer_id == 0:
            h = self.pre_ln(h)
        a = self.ln1(h)
        att, wkv_state = self.attention(a, x_att, wkv_state)
        h = h + att
        f = self.ln2(h)
        h = h + self.feed_forward(f, x_ffn)
        return h, a[:, -1], f[:, -1], wkv_state


class RWKVEncoder(nn.Module):
    def __init__(self, cfg: RWKVConfig):
        super().__init__()
        self.config = cfg
        self.input_proj = nn.Linear(cfg.input_dim, cfg.hidden_size)
        self.blocks = nn.ModuleList(RWKVBlock(cfg, l) for l in range(cfg.num_layers))
        self.ln_out = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_epsilon)
        self.output_proj = nn.Linear(cfg.hidden_size, cfg.vocab_size)

    # ------------------------------------------------------------------------- state ----------
    def zero_state(self, B, device=None, dtype=torch.float32):
        """The state before the first frame: zero shift frames, the empty WKV state."""
        cfg = self.config
        L, H = cfg.num_layers, cfg.hidden_size
        A = cfg.attention_hidden_size or H
        device = device if device is not None else self.input_proj.weight.device
        return (torch.zeros(L, B, H, dtype=dtype, device=device),
                torch.zeros(L, B, H, dtype=dtype, device=device),
                torch.zeros(L, B, A, dtype=torch.float32, device=device),
                torch.zeros(L, B, A, dtype=torch.float32, device=device),
                torch.full((L, B, A), EMPTY_MAX, dtype=torch.float32, device=device))

    @staticmethod
    def state_from_hf(state):
        """transformers' state list [ffn shift, attention shift, num, den, max], each [B,C,L]
        -> (x_att, x_ffn, num, den, max), each [L,B,C]."""
        x_ffn, x_att, num, den, mx = (s.permute(2, 0, 1).contiguous() for s in state)
        return x_att, x_ffn, num.float(), den.float(), mx.float()

    @staticmethod
    def state_to_hf(state):
        """The inverse of state_from_hf."""
        x_att, x_ffn, num, den, mx = (s.permute(1, 2, 0).contiguous() for s in state)
        return [x_ffn, x_att, num, den, mx]

    # ------------------------------------------------------------------------- forward --------
    def forward(self, x, state=None):
        if x.dim() != 3 or x.shape[1] < 1:
            raise ValueError(f"RWKVEncoder: x must be [B,T,input_dim] with T >= 1, got {tuple(x.shape)}")
        B = x.shape[0]
        if state is None:
            state = self.zero_state(B, x.device)
        if len(state) != 5 or any(s.shape[0] != len(self.blocks) or s.shape[1] != B for s in state):
            raise ValueError("RWKVEncoder: state must be (x_att, x_ffn, num, den, max), each [L,B,C]")
        x_att, x_ffn, num, den, mx = state
        h = self.input_proj(x)
        out = [[], [], [], [], []]
        for l, blk in enumerate(self.blocks):
            h, xa, xf, (n1, d1, m1) = blk(h, x_att[l], x_ffn[l], (num[l], den[l], mx[l]))
            for lst, val in zip(out, (xa, xf, n1, d1, m1)):
                lst.append(val)
        logits = self.output_proj(self.ln_out(h))
        if not self.config.return_last_states:
            return logits
        return logits, tuple(torch.stack(o) for o in out)
