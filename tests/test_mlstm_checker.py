"""The mLSTM parity tests' checker, pinned on the CPU: tests/torch_ref.mlstm64 against the numpy
step recurrence (oracle/mlstm.py, itself pinned to transformers' chunkwise mLSTM by
tests/test_oracle_golden.py) in every gate regime of tests/mlstm_cases.py, and the identities
the kernels' host side takes the gate gradients from -- with the final-state term -- against
fp64 autograd."""
import numpy as np
import pytest
import torch

from oracle import mlstm as omlstm
from tests.mlstm_cases import (REGIMES, draw_case, floor_branch_share, gate_grads_from_pairs,
                               reference)
from tests.torch_ref import mlstm64

SHAPE = (1, 2, 192, 32, 64)   # B, NH, T, DQ, DV


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_mlstm64_equals_step_oracle_in_every_regime(regime, init):
    c = draw_case(*SHAPE, torch.bfloat16, regime, init)
    args = [c.get(k) for k in ("q", "k", "v", "igate", "fgate", "c0", "n0", "m0")]
    with torch.no_grad():
        h, (C, n, m) = mlstm64(*[None if t is None else t.double() for t in args])
    rh, (rC, rn, rm) = omlstm.mlstm_recurrent(*[None if t is None else t.double().numpy()
                                                for t in args])
    for got, ref in ((h, rh), (C, rC), (n, rn)):
        np.testing.assert_allclose(got.numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max())
    np.testing.assert_allclose(m.numpy(), rm, rtol=1e-5, atol=1e-5)


def test_regimes_reach_the_floor_branch_they_are_named_for():
    """The premises of the GPU regime cases at their shape, with and without an initial state."""
    for init in (False, True):
        share = {r: floor_branch_share(draw_case(*SHAPE, torch.bfloat16, r, init))
                 for r in REGIMES}
        print(f"floor-branch share (init={init}):", {r: round(s, 3) for r, s in share.items()})
        assert share["dead"] >= 0.9
        assert 0.3 <= share["forgetful"] <= 0.9
        assert share["default"] <= 0.1


@pytest.mark.parametrize("loss", ["h", "state", "mixed"])
def test_gate_gradient_identities_vs_autograd(loss):
    """d igate = k.dk and d fgate = sigmoid(-f) revcumsum(q.dq - k.dk), the latter with
    <dC_T, C~_T> + <dn_T, n~_T> added at the last step, equal autograd's gate gradients in fp64
    to 1e-10 (measured 1e-15) for an h-only, a state-only and a mixed loss.  Without the term
    the state-only loss misses d fgate by more than 100%: the final state depends on the last
    forget gate with no query partner."""
    B, NH, T, DQ, DV = 1, 2, 128, 32, 64
    c = draw_case(B, NH, T, DQ, DV, torch.bfloat16, "default", True)
    w = {"h": {"h": 1.0}, "state": {"c": 1.0, "n": 1.0}, "mixed": {"h": 1.0, "c": 1.0, "n": 1.0}}[loss]
    ref = reference(c, w)
    g = ref["grad"]
    state = loss != "h"
    dcT, dnT = (c["Rc"].double(), c["Rn"].double()) if state else (None, None)
    di, df = gate_grads_from_pairs(c, g["q"], g["k"], dcT, ref["cT"], dnT, ref["nT"])

    def rel(a, b):
        return float((a - b).norm() / b.norm())
    print(f"{loss}: d igate {rel(di, g['igate']):.2e}  d fgate {rel(df, g['fgate']):.2e}")
    assert rel(di, g["igate"]) <= 1e-10
    assert rel(df, g["fgate"]) <= 1e-10
    if loss == "state":
        _, bare = gate_grads_from_pairs(c, g["q"], g["k"])
        print(f"state: d fgate without the final-state term {rel(bare, g['fgate']):.2e}")
        assert rel(bare, g["fgate"]) > 1.0
