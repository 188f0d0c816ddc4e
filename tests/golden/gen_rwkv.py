"""Writes tests/golden/rwkv.npz from transformers' RWKV-4 (models/rwkv/modeling_rwkv.py, pure torch
on the CPU): an independent restatement of the WKV recurrence and of the block stack that
statecatcher_amd/rwkv.py and tests/rwkv_ref.py are held to.

    python tests/golden/gen_rwkv.py

  model/*   RwkvModel(rescale_every=0), float32, hidden 32, intermediate 64, 2 layers, B=2, fed
            T=19 then T=18 through inputs_embeds with the state carried: every blocks.* and
            ln_out.* parameter, both inputs, both last_hidden_state, the final state list
            (5 x [B,C,L]: ffn shift, attention shift, num, den, max).
  wkv/<regime>/*   rwkv_linear_attention_cpu on two regimes of tests/wkv_cases.py (B=2, T=21, C=33)
            from a random state, float32: y and the returned state.
Plain arrays only.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import wkv_cases  # noqa: E402


def main():
    from transformers import RwkvConfig, RwkvModel
    from transformers.models.rwkv.modeling_rwkv import rwkv_linear_attention_cpu
    out = {}
    torch.manual_seed(0)
    cfg = RwkvConfig(vocab_size=16, hidden_size=32, attention_hidden_size=32, intermediate_size=64,
                     num_hidden_layers=2, rescale_every=0, context_length=64)
    model = RwkvModel(cfg).float().eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("time_first"):   # (transformers initialises it to ones)
                h = torch.arange(p.numel(), dtype=torch.float32)
                p.copy_(math.log(0.3) + ((h + 1) % 3 - 1) * 0.5)
            elif ".ln" in name or "pre_ln" in name or name.startswith("ln_out"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    for name, p in model.state_dict().items():
        if name.startswith("blocks.") or name.startswith("ln_out."):
            out["model/" + name] = p.numpy().copy()
    x1 = torch.randn(2, 19, 32, generator=g)
    x2 = torch.randn(2, 18, 32, generator=g)
    with torch.no_grad():
        r1 = model(inputs_embeds=x1, state=None, use_cache=True)
        r2 = model(inputs_embeds=x2, state=r1.state, use_cache=True)
    out["model/x1"], out["model/x2"] = x1.numpy(), x2.numpy()
    out["model/h1"] = r1.last_hidden_state.numpy().copy()
    out["model/h2"] = r2.last_hidden_state.numpy().copy()
    for i, s in enumerate(r2.state):
        out[f"model/state{i}"] = s.numpy().copy()
    for regime in ("init", "extreme"):
        c = wkv_cases.make(regime, "random", 2, 21, 33, seed=3)
        with torch.no_grad():
            y, st = rwkv_linear_attention_cpu(c["td"], c["tf"], c["k"], c["v"],
                                              state=tuple(s.clone() for s in c["state"]),
                                              return_state=True)
        out[f"wkv/{regime}/y"] = y.numpy().copy()
        for n, s in zip(("num", "den", "max"), st):
            out[f"wkv/{regime}/{n}"] = s.numpy().copy()
    path = os.path.join(HERE, "rwkv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
