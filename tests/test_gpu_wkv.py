"""The WKV kernels (csrc/wkv.hip) on the GPU against the float64 checker (tests/rwkv_ref.py) on the
same dtype-rounded inputs: y, the final state and all four gradients under the loss sum(y * r).

Bounds, per tensor with scale = max |ref64| (each case prints its measured errors first):
  fp32   max |got - ref64| <= 8 d32 + 2e-6 scale, d32 the checker's own float32-vs-float64 error on
         the case (8: another summation order across chunks; 2e-6: the argument rounding
         |x| 2^-24 of exp2(x log2 e) for the |x| <~ 17 that still reach one ulp of the sum);
  bf16   y, dk, dv elementwise |got - ref64| <= 2^-8 |ref64| + the fp32 bound (one rounding on
         store: half a bf16 ulp is 2^-9 .. 2^-8 of the value, so the ratio reaches 1 only for a
         mantissa just above a power of two); the parameter gradients stay on the fp32 bound;
  state  num / den and max + log den (the triple is not unique) under the fp32 bound.
"""
import functools

import pytest
import torch

from tests import rwkv_ref as ref
from tests import wkv_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DTYPES = [torch.float32, torch.bfloat16]
NAMES = ("y", "d_time_decay", "d_time_first", "dk", "dv", "state num/den", "state max+log den")


def ops():
    from statecatcher_amd import ops as o
    return o


S = 64   # ops.WKV_CHUNK (asserted below: the cases sit on its edges)


def test_chunk_is_what_the_cases_assume():
    assert ops().WKV_CHUNK == S


def _checker(c, dtype):
    ins = [c[n].to(dtype).clone().requires_grad_(True) for n in ("td", "tf", "k", "v")]
    y, st = ref.wkv(*ins, c["state"], dtype)
    (y * c["r"].to(dtype)).sum().backward()
    out = [y.detach()] + [i.grad if i.grad is not None else torch.zeros_like(i) for i in ins]
    out += [t.detach() for t in ref.canonical_state(st)]
    return [t.double() for t in out]


@functools.lru_cache(maxsize=None)
def reference(regime, state, B, T, C, dtype):
    """(case rounded to dtype, ref64 tensors, fp32 bounds) -- computed once per case."""
    c = cases.rounded(cases.make(regime, state, B, T, C), dtype)
    r64, r32 = _checker(c, torch.float64), _checker(c, torch.float32)
    bounds = [8 * float((a - b).abs().max()) + 2e-6 * float(b.abs().max()) for a, b in zip(r32, r64)]
    return c, r64, bounds


def run(c, dtype, wkv=None):
    o = ops()
    td, tf = (c[n].to(DEV).requires_grad_(True) for n in ("td", "tf"))
    k, v = (c[n].to(DEV, dtype).requires_grad_(True) for n in ("k", "v"))
    st = None if c["state"] is None else tuple(s.to(DEV) for s in c["state"])
    y, s1 = (wkv or o.wkv)(td, tf, k, v, st)
    assert y.dtype == dtype and all(s.dtype == torch.float32 and not s.requires_grad for s in s1)
    (y.float() * c["r"].to(DEV)).sum().backward()
    assert k.grad.dtype == dtype and td.grad.dtype == torch.float32
    return [y.detach(), td.grad, tf.grad, k.grad, v.grad], s1


def check(regime, state, B, T, C, dtype):
    c, r64, bounds = reference(regime, state, B, T, C, dtype)
    got, s1 = run(c, dtype)
    got = [g.double().cpu() for g in got] + [t.double().cpu() for t in ref.canonical_state(s1)]
    worst = 0.0
    fails = []
    for name, g, r, bd in zip(NAMES, got, r64, bounds):
        assert torch.isfinite(g).all(), name
        err = (g - r).abs()
        if dtype == torch.bfloat16 and name in ("y", "dk", "dv"):
            lim = 2.0 ** -8 * r.abs() + bd
        else:
            lim = torch.full_like(r, bd)
        ratio = float((err / lim.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"{regime}/{state} B={B} T={T} C={C} {str(dtype)[6:]} {name}: max err "
              f"{float(err.max()):.3e} bound {bd:.3e} ratio {ratio:.3f}")
        worst = max(worst, ratio)
        if not bool((err <= lim).all()):
            fails.append((name, float(err.max()), bd, ratio))
    assert not fails, fails
    if T == 1:   # y_0 does not depend on the decay
        assert float(got[1].abs().max()) == 0.0
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [33, 64])
@pytest.mark.parametrize("T", [1, 2, S - 1, S, S + 1, 3 * S + 5])
def test_parity_over_lengths(T, C, B, dtype):
    check("init", "random", B, T, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("state", cases.STATES)
@pytest.mark.parametrize("regime", cases.REGIMES)
def test_parity_over_regimes(regime, state, dtype):
    check(regime, state, 2, 3 * S + 5, 33, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_parity_wide(dtype):
    check("init", "random", 2, 2 * S + 2, 768, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_runs_and_rows_are_bitwise(dtype):
    """Two runs agree bitwise, parameter gradients included (no atomics); permuting the batch rows
    permutes every per-row output bitwise (no cross-row arithmetic)."""
    c = cases.rounded(cases.make("init", "random", 3, 2 * S + 7, 33), dtype)
    a, sa = run(c, dtype)
    b, sb = run(c, dtype)
    assert all(torch.equal(x, y) for x, y in zip(a + list(sa), b + list(sb)))
    perm = torch.tensor([2, 0, 1])
    cp = dict(c, k=c["k"][perm], v=c["v"][perm], r=c["r"][perm],
              state=tuple(s[perm] for s in c["state"]))
    p, sp = run(cp, dtype)
    pd = perm.to(DEV)
    for i in (0, 3, 4):
        assert torch.equal(p[i], a[i][pd])
    assert all(torch.equal(x, y[pd]) for x, y in zip(sp, sa))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_ctypes_path_and_dispatcher_op_are_bitwise(dtype):
    from statecatcher_amd import torch_library as tl
    c = cases.rounded(cases.make("sharp", "random", 2, S + 9, 40), dtype)
    a, sa = run(c, dtype)
    b, sb = run(c, dtype, wkv=tl.wkv)
    assert all(torch.equal(x, y) for x, y in zip(a + list(sa), b + list(sb)))


def test_no_host_sync_and_no_grad_saves_nothing():
    o = ops()
    c = cases.make("init", "random", 2, S + 3, 33)
    td, tf, k, v = (c[n].to(DEV) for n in ("td", "tf", "k", "v"))
    st = tuple(s.to(DEV) for s in c["state"])
    r = c["r"].to(DEV)
    kg, vg = k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    tdg = td.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, s1 = o.wkv(tdg, tf, kg, vg, st)
        (y * r).sum().backward()
        with torch.no_grad():
            y2, s2 = o.wkv(td, tf, k, v, st)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(y2, y.detach()) and all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert y2.grad_fn is None and kg.grad is not None and tdg.grad is not None


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_pieces_equal_whole_and_empty_calls(dtype):
    """Feeding in pieces with the state carried: the same y (each piece recomposes its chunks, so
    equal within the fp32 bound, not bitwise); T = 0 returns the state unchanged; B = 0 runs."""
    o = ops()
    T = 2 * S + 5
    c, r64, bounds = reference("init", "random", 2, T, 33, dtype)
    td, tf = c["td"].to(DEV), c["tf"].to(DEV)
    k, v = c["k"].to(DEV, dtype), c["v"].to(DEV, dtype)
    st = tuple(s.to(DEV) for s in c["state"])
    ys = []
    for lo, hi in ((0, 1), (1, S), (S, S), (S, T)):
        y, st2 = o.wkv(td, tf, k[:, lo:hi], v[:, lo:hi], st)
        if lo == hi:
            assert y.shape == (2, 0, 33) and all(torch.equal(a, b) for a, b in zip(st, st2))
        st = st2
        ys.append(y)
    err = (torch.cat(ys, 1).double().cpu() - r64[0]).abs()
    lim = bounds[0] + (2.0 ** -8 * r64[0].abs() if dtype == torch.bfloat16 else 0.0)
    assert bool((err <= lim).all()), float(err.max())
    for g, r, bd in zip(ref.canonical_state(tuple(s.double().cpu() for s in st)), r64[5:], bounds[5:]):
        assert float((g - r).abs().max()) <= bd
    y0, s0 = o.wkv(td, tf, k[:0], v[:0], None)
    assert y0.shape == (0, T, 33) and s0[0].shape == (0, 33)
