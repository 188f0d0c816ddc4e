"""CPU checks of the WKV checker itself (tests/rwkv_ref.py), which the GPU kernels are held to:
against a direct O(T^2) evaluation of the sums, against transformers (recorded in
tests/golden/rwkv.npz, and live where it is installed), its written adjoint against autograd, the
premise of the ``extreme`` regime, and chunked feeding against whole."""
import numpy as np
import pytest
import torch

from tests import rwkv_ref as ref
from tests import wkv_cases as cases
from tests.conftest import load_golden


def _grads(c, dtype, state="keep"):
    ins = [c[n].to(dtype).clone().requires_grad_(True) for n in ("td", "tf", "k", "v")]
    y, st = ref.wkv(*ins, c["state"], dtype)
    (y * c["r"].to(dtype)).sum().backward()
    return y.detach(), st, [i.grad if i.grad is not None else torch.zeros_like(i) for i in ins]


@pytest.mark.parametrize("state", cases.STATES)
@pytest.mark.parametrize("regime", cases.REGIMES)
def test_checker_equals_direct_sums(regime, state):
    c = cases.make(regime, state, 2, 12, 5)
    y, _ = ref.wkv(c["td"], c["tf"], c["k"], c["v"], c["state"], torch.float64)
    yd = ref.wkv_direct(c["td"], c["tf"], c["k"], c["v"], c["state"])
    assert torch.isfinite(y).all()
    assert float((y - yd).abs().max()) <= 1e-12 * max(1.0, float(yd.abs().max()))


@pytest.mark.parametrize("regime", ["init", "extreme"])
def test_checker_equals_fixture(regime):
    """transformers' rwkv_linear_attention_cpu ran in float32: the float64 checker is within the
    float32 checker's own distance of it (the two float32 runs do the same arithmetic)."""
    z = load_golden("rwkv")
    c = cases.make(regime, "random", 2, 21, 33, seed=3)
    y64, s64 = ref.wkv(c["td"], c["tf"], c["k"], c["v"], c["state"], torch.float64)
    y32, s32 = ref.wkv(c["td"], c["tf"], c["k"], c["v"], c["state"], torch.float32)
    got = torch.from_numpy(z[f"wkv/{regime}/y"]).double()
    scale = float(y64.abs().max())
    noise = float((y32.double() - y64).abs().max())
    assert float((got - y64).abs().max()) <= 2 * noise + 1e-7 * scale
    fix = tuple(torch.from_numpy(z[f"wkv/{regime}/{n}"]).double() for n in ("num", "den", "max"))
    for a, b, b32 in zip(ref.canonical_state(fix), ref.canonical_state(s64), ref.canonical_state(s32)):
        noise = float((b32.double() - b).abs().max())
        assert float((a - b).abs().max()) <= 2 * noise + 1e-7 * float(b.abs().max())


@pytest.mark.parametrize("regime", ["init", "sharp", "bonus"])
def test_checker_equals_transformers_live(regime):
    mod = pytest.importorskip("transformers.models.rwkv.modeling_rwkv")
    c = cases.make(regime, "random", 2, 40, 7)
    args = [c[n].double() for n in ("td", "tf", "k", "v")]
    st = tuple(s.double() for s in c["state"])
    y, s = mod.rwkv_linear_attention_cpu(*args, state=st, return_state=True)
    yr, sr = ref.wkv(*args, st, torch.float64)
    assert float((y - yr).abs().max()) == 0.0
    for a, b in zip(s, sr):
        assert float((a - b).abs().max()) == 0.0


@pytest.mark.parametrize("state", cases.STATES)
@pytest.mark.parametrize("regime", ["init", "sharp", "slow", "fast", "bonus"])
def test_written_adjoint_equals_autograd(regime, state):
    c = cases.make(regime, state, 2, 30, 9)
    _, _, (dtd, dtf, dk, dv) = _grads(c, torch.float64)
    adk, adv, adtd, adtf = ref.wkv_adjoint(c["td"], c["tf"], c["k"], c["v"], c["r"], c["state"])
    for got, want in ((adk, dk), (adv, dv), (adtd, dtd), (adtf, dtf)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1e-30, float(want.abs().max()))


def test_extreme_premise_naive_float32_overflows():
    c = cases.make("extreme", "none", 2, 300, 33)
    assert not torch.isfinite(ref.wkv_naive(c["td"], c["tf"], c["k"], c["v"], torch.float32)).all()
    y32, gs = _grads(c, torch.float32)[0], _grads(c, torch.float32)[2]
    assert torch.isfinite(y32).all() and all(torch.isfinite(g).all() for g in gs)


@pytest.mark.parametrize("regime", cases.REGIMES)
def test_float32_checker_is_well_conditioned(regime):
    """The premise of the GPU bounds (8 x the checker's own float32 error): that error is small on
    every regime, so the bound means something.  Observed 1e-7 .. 2e-5 of each tensor's scale,
    2e-4 for the parameter gradients of ``sharp`` and ``extreme``; asserted at 1e-3 (float32 keeps
    four of its seven digits) and finite."""
    c = cases.make(regime, "random", 2, 300, 33)
    y64, _, g64 = _grads(c, torch.float64)
    y32, _, g32 = _grads(c, torch.float32)
    lim = 1e-3
    for a, b in zip([y32] + g32, [y64] + g64):
        assert torch.isfinite(a).all()
        assert float((a.double() - b).abs().max()) <= lim * float(b.abs().max())


@pytest.mark.parametrize("state", cases.STATES)
def test_chunked_feeding_equals_whole(state):
    c = cases.make("init", state, 2, 50, 9)
    args = [c[n].double() for n in ("td", "tf")]
    k, v = c["k"].double(), c["v"].double()
    y, s = ref.wkv(*args, k, v, c["state"], torch.float64)
    st, ys = c["state"], []
    for lo, hi in ((0, 1), (1, 20), (20, 20), (20, 50)):
        yc, st = ref.wkv(*args, k[:, lo:hi], v[:, lo:hi], st, torch.float64)
        ys.append(yc)
    assert torch.equal(torch.cat(ys, 1), y)
    assert all(torch.equal(a, b) for a, b in zip(st, s))


def test_encoder_checker_equals_fixture_and_chunks():
    """The plain-torch encoder on the fixture's transformers weights (identity input / output
    projections): both segments' last_hidden_state and the final state, float32 noise apart."""
    z = load_golden("rwkv")
    sd = {k[len("model/"):]: torch.from_numpy(z[k]) for k in z.files
          if k.startswith("model/blocks.") or k.startswith("model/ln_out.")}
    H = 32
    sd.update({"input_proj.weight": torch.eye(H), "input_proj.bias": torch.zeros(H),
               "output_proj.weight": torch.eye(H), "output_proj.bias": torch.zeros(H)})
    x1, x2 = torch.from_numpy(z["model/x1"]), torch.from_numpy(z["model/x2"])
    for dtype, lim in ((torch.float64, 2e-5), (torch.float32, 2e-5)):
        h1, st = ref.encoder(sd, x1, None, dtype=dtype)
        h2, st = ref.encoder(sd, x2, st, dtype=dtype)
        for got, name in ((h1, "h1"), (h2, "h2")):
            want = torch.from_numpy(z["model/" + name]).double()
            assert float((got.double() - want).abs().max()) <= lim * float(want.abs().max())
        x_att, x_ffn, num, den, mx = st
        hf = [torch.from_numpy(z[f"model/state{i}"]).double().permute(2, 0, 1) for i in range(5)]
        for got, want in ((x_ffn, hf[0]), (x_att, hf[1])):
            assert float((got.double() - want).abs().max()) <= lim * float(want.abs().max())
        for a, b in zip(ref.canonical_state((num.double(), den.double(), mx.double())),
                        ref.canonical_state(hf[2:])):
            assert float((a - b).abs().max()) <= lim * float(b.abs().max())
    # whole == pieces (float64: exact up to the summation order of the linears)
    xw = torch.cat([x1, x2], 1)
    hw, sw = ref.encoder(sd, xw, None)
    h64a, s64 = ref.encoder(sd, x1, None)
    h64b, s64 = ref.encoder(sd, x2, s64)
    assert float((hw - torch.cat([h64a, h64b], 1)).abs().max()) <= 1e-12
    for a, b in zip(sw, s64):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
