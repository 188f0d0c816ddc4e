"""The recurrent WKV step kernel (csrc/rwkv_step.hip, ops.wkv_step) on the GPU against the float64
checker (tests/rwkv_ref.wkv) on the same dtype-rounded inputs, over the regimes and state kinds of
tests/wkv_cases.py at B = 2, C in {64, 80} (80: the tail lanes of the second wave), K in {1, 5}.

Bounds, per tensor with scale = max |ref64| (the rule of tests/test_gpu_wkv.py; the step kernel
sums in the checker's own order, so it is generous):
  fp32   max |got - ref64| <= 8 d32 + 2e-6 scale, d32 the checker's float32-vs-float64 error;
  bf16   y elementwise: that plus 2^-8 |ref64| for the rounding on store;
  state  num / den and max + log den (canonical_state) under the fp32 bound.
With r: the output against sigmoid(r) * y, y from a second call without r -- an fp32 call on the
same dtype-rounded operands, so that y is the value the kernel holds before its store and not a
second rounding of it.  Tolerance: one rounding of the product in the output dtype (bf16: half an
ulp, <= 2^-8 |ref|) plus 2^-20 |ref| for the fp32 arithmetic -- inside the sigmoid the argument
r log2 e is rounded (|r| 2^-24 relative in e^-r, |r| < 6 here), v_exp_f32 and v_rcp_f32 are about
an ulp (2^-23) each, the add and the fp32 product half an ulp each: under 12 x 2^-24.
"""
import functools

import pytest
import torch

from tests import rwkv_ref as ref
from tests import wkv_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DTYPES = [torch.float32, torch.bfloat16]
B = 2


def ops():
    from statecatcher_amd import ops as o
    return o


def explicit_state(c, C):
    """The case's state as the step kernel takes it: never None (the empty state is explicit)."""
    return c["state"] if c["state"] is not None else ref.empty_state(B, C, torch.float32)


@functools.lru_cache(maxsize=None)
def reference(regime, state, K, C, dtype):
    """(case rounded to dtype, ref64 [y, num/den, max + log den], fp32 bounds) -- once per case."""
    c = cases.rounded(cases.make(regime, state, B, K, C), dtype)
    runs = []
    for dt in (torch.float64, torch.float32):
        y, st = ref.wkv(c["td"], c["tf"], c["k"], c["v"], c["state"], dt)
        runs.append([t.double() for t in (y, *ref.canonical_state(st))])
    r64, r32 = runs
    bounds = [8 * float((a - b).abs().max()) + 2e-6 * float(b.abs().max()) for a, b in zip(r32, r64)]
    return c, r64, bounds


def run(c, dtype, C, r=False, live=None, steps=None):
    """(y [B,K,C], state) of ops.wkv_step on the case; steps: feed the frames in calls of that
    many (the state carried in place)."""
    o = ops()
    td, tf = c["td"].to(DEV), c["tf"].to(DEV)
    k, v, rr = (c[n].to(DEV, dtype) for n in ("k", "v", "r"))
    st = tuple(s.to(DEV).clone() for s in explicit_state(c, C))
    K = k.shape[1]
    lv = None if live is None else live.to(DEV)
    ys = []
    n = K if steps is None else steps
    for t0 in range(0, K, n):
        sl = slice(t0, t0 + n)
        ys.append(o.wkv_step(td, tf, k[:, sl], v[:, sl], st, r=rr[:, sl] if r else None,
                             live=None if lv is None else lv[:, sl]))
    y = torch.cat(ys, 1)
    assert y.dtype == dtype and y.shape == k.shape
    return y, st


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("C", [64, 80])
@pytest.mark.parametrize("state", cases.STATES)
@pytest.mark.parametrize("regime", cases.REGIMES)
def test_parity(regime, state, C, K, dtype):
    c, r64, bounds = reference(regime, state, K, C, dtype)
    y, st = run(c, dtype, C)
    got = [y.double().cpu()] + [t.double().cpu() for t in ref.canonical_state(st)]
    fails = []
    for name, g, r, bd in zip(("y", "state num/den", "state max+log den"), got, r64, bounds):
        assert torch.isfinite(g).all(), name
        err = (g - r).abs()
        lim = 2.0 ** -8 * r.abs() + bd if (dtype == torch.bfloat16 and name == "y") \
            else torch.full_like(r, bd)
        ratio = float((err / lim.clamp_min(1e-300)).max())
        print(f"{regime}/{state} K={K} C={C} {str(dtype)[6:]} {name}: max err {float(err.max()):.3e} "
              f"bound {bd:.3e} ratio {ratio:.3f}")
        if not bool((err <= lim).all()):
            fails.append((name, float(err.max()), bd, ratio))
    assert not fails, fails


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [64, 80])
@pytest.mark.parametrize("regime", ["init", "sharp"])
def test_receptance_gate_is_sigmoid_r_times_y(regime, C, dtype):
    c = cases.rounded(cases.make(regime, "random", B, 5, C), dtype)
    y, s0 = run(c, torch.float32, C)   # (c is rounded to dtype: the same arithmetic, y unrounded)
    g, s1 = run(c, dtype, C, r=True)
    assert g.dtype == dtype
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))   # the gate does not touch the state
    want = torch.sigmoid(c["r"].double()) * y.double().cpu()
    err = (g.double().cpu() - want).abs()
    lim = (2.0 ** -20 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)) * want.abs() + 1e-37
    print(f"gate {regime} C={C} {str(dtype)[6:]}: worst err / limit {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all()), float((err / lim).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("gate", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("C", [64, 80])
def test_k_steps_in_one_call_equal_k_calls_bitwise(C, gate, dtype):
    live = torch.tensor([[1.0, 1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0, 0.0]])
    for regime in ("init", "extreme"):
        c = cases.rounded(cases.make(regime, "random", B, 5, C), dtype)
        for lv in (None, live):
            y5, s5 = run(c, dtype, C, r=gate, live=lv)
            y1, s1 = run(c, dtype, C, r=gate, live=lv, steps=1)
            y2, s2 = run(c, dtype, C, r=gate, live=lv, steps=2)
            assert torch.equal(y5, y1) and torch.equal(y5, y2)
            assert all(torch.equal(a, b) and torch.equal(a, d) for a, b, d in zip(s5, s1, s2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("state", cases.STATES)
def test_held_steps_leave_the_state_alone_and_write_zero_rows(state, dtype):
    C, K = 80, 5
    c = cases.rounded(cases.make("init", state, B, K, C), dtype)
    before = tuple(s.clone() for s in explicit_state(c, C))
    # stream 0 has holes, stream 1 is held throughout
    live = torch.tensor([[0.0, 1.0, 0.0, 0.0, 1.0], [0.0] * K])
    y, st = run(c, dtype, C, r=True, live=live)
    assert not y[1].any() and not y[0, [0, 2, 3]].any() and y[0, [1, 4]].any()
    for a, b in zip(st, before):
        assert torch.equal(a[1].cpu(), b[1])            # bitwise: the sentinel -1e38 included
    # the stream with holes is the stream with those steps removed, bitwise
    cc = dict(c, k=c["k"][:, [1, 4]], v=c["v"][:, [1, 4]], r=c["r"][:, [1, 4]])
    yc, sc = run(cc, dtype, C, r=True)
    assert torch.equal(y[0, [1, 4]], yc[0])
    assert all(torch.equal(a[0], b[0]) for a, b in zip(st, sc))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_runs_are_bitwise_and_extreme_is_finite(dtype):
    for state in cases.STATES:
        c = cases.rounded(cases.make("extreme", state, B, 5, 80), dtype)
        y, st = run(c, dtype, 80, r=True)
        y2, st2 = run(c, dtype, 80, r=True)
        assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(st, st2))
        assert torch.isfinite(y).all() and all(torch.isfinite(s).all() for s in st)


def test_strided_operands_given_output_and_refusals():
    """The layout the encoder's step uses: [K,B,C] buffers passed as their [B,K,C] views, the
    output buffer given; the state is never cast or copied."""
    o = ops()
    C, K = 80, 5
    c = cases.make("init", "random", B, K, C)
    y, st = run(c, torch.float32, C, r=True)
    td, tf = c["td"].to(DEV), c["tf"].to(DEV)
    k, v, r = (c[n].to(DEV).transpose(0, 1).contiguous().transpose(0, 1) for n in ("k", "v", "r"))
    assert not k.is_contiguous()
    s2 = tuple(s.to(DEV).clone() for s in c["state"])
    out = torch.full((K, B, C + 16), 7.0, device=DEV)[..., :C].transpose(0, 1)
    got = o.wkv_step(td, tf, k, v, s2, r=r, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, y)
    assert all(torch.equal(a, b) for a, b in zip(st, s2))
    with pytest.raises(ValueError, match="contiguous fp32"):
        o.wkv_step(td, tf, k, v, tuple(s.double() for s in s2))
    with pytest.raises(ValueError, match="state must be"):
        o.wkv_step(td, tf, k, v, None)
    with pytest.raises(ValueError, match="k's strides"):
        o.wkv_step(td, tf, k, v.contiguous(), s2)
    with pytest.raises(TypeError, match="fp32 or bf16"):
        o.wkv_step(td, tf, k.half(), v.half(), s2)
    assert o.wkv_step(td, tf, k[:, :0], v[:, :0], s2).shape == (B, 0, C)
    assert all(torch.equal(a, b) for a, b in zip(st, s2))
