"""Seeded inputs of the WKV tests: the regimes of (k, time_decay, time_first) and the kinds of
incoming state, shared by the CPU checker tests and the GPU parity tests.

All regimes are well conditioned (checked on the CPU at B=2, C=33, T <= 300: the float32 run of
the checker is within 1e-7 .. 8e-6 of each tensor's scale, 8e-5 in ``extreme``); ``extreme`` is the
one whose unstabilised float32 evaluation overflows."""
import math

import torch

REGIMES = ("init", "sharp", "slow", "fast", "bonus", "extreme")
STATES = ("none", "sentinel", "random")
EMPTY_MAX = -1e38


def _ramp(C):
    h = torch.arange(C, dtype=torch.float64) / max(C - 1, 1)
    return -5.0 + 8.0 * h ** 0.7


def _zig(C):
    return torch.tensor([((i + 1) % 3 - 1) * 0.5 for i in range(C)], dtype=torch.float64)


# regime -> (k scale, time_decay, time_first offset)
_TABLE = {
    "init": (1.0, _ramp, math.log(0.3)),
    "sharp": (8.0, _ramp, math.log(0.3)),
    "slow": (1.0, lambda C: torch.full((C,), -8.0, dtype=torch.float64), 0.0),
    "fast": (1.0, lambda C: torch.full((C,), 3.0, dtype=torch.float64), 2.0),
    "bonus": (1.0, _ramp, 6.0),
    "extreme": (60.0, _ramp, math.log(0.3)),
}


def make(regime, state, B, T, C, seed=0):
    """float32 CPU tensors: dict(td, tf [C]; k, v, r [B,T,C] (r: the weights of the loss
    sum(y * r)); state: None or (num, den, max) [B,C])."""
    kscale, td_fn, tf0 = _TABLE[regime]
    g = torch.Generator().manual_seed(1000 * seed + 17 * REGIMES.index(regime) + STATES.index(state))
    k = (kscale * torch.randn(B, T, C, generator=g, dtype=torch.float64)).float()
    v = torch.randn(B, T, C, generator=g, dtype=torch.float64).float()
    r = torch.randn(B, T, C, generator=g, dtype=torch.float64).float()
    td = td_fn(C).float()
    tf = (tf0 + _zig(C)).float()
    if state == "none":
        st = None
    elif state == "sentinel":
        st = (torch.zeros(B, C), torch.zeros(B, C), torch.full((B, C), EMPTY_MAX))
    else:
        num = torch.randn(B, C, generator=g, dtype=torch.float64).float()
        den = (torch.randn(B, C, generator=g, dtype=torch.float64).abs() + 0.1).float()
        mx = (kscale * torch.randn(B, C, generator=g, dtype=torch.float64)).float()
        st = (num, den, mx)
    return dict(td=td, tf=tf, k=k, v=v, r=r, state=st)


def rounded(case, dtype):
    """The case with k, v and r rounded to ``dtype`` (what the kernel is handed), as float32."""
    out = dict(case)
    for n in ("k", "v", "r"):
        out[n] = case[n].to(dtype).float()
    return out
