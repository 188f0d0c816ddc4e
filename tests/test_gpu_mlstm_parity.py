"""The mLSTM cell kernels (mlstm.hip) against fp64 at every compiled head size, over four chunks,
in five gate regimes, under both grid mappings, and with a gradient arriving at the final state.

The checker is tests/torch_ref.mlstm64 in fp64 on the same rounded inputs (pinned on the CPU by
tests/test_mlstm_checker.py), the inputs and regimes are tests/mlstm_cases.py.  Bounds, as in
tests/test_gpu_mlstm.py: h, cT, nT relative Frobenius <= 1e-2; mT rtol = atol = 1e-5; q / k / v /
c0 / n0 gradients <= 3e-2; gate gradients <= 3e-2 at T <= 128 and, at T >= 192 where they are sums
over the sequence, cosine >= 0.999 and <= 5e-2 (tests/test_gpu_c4.py's bound for them).  Every
case prints its measured errors before it asserts."""
import numpy as np
import pytest
import torch

from tests.mlstm_cases import (LEAVES, REGIMES, assert_fits_f16, draw_case, floor_branch_share,
                               reference, weighted_loss)
from tests.test_gpu_mlstm import close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DTYPES = [torch.bfloat16, torch.float16]
H_ONLY = {"h": 1.0}
STATE_ONLY = {"c": 1.0, "n": 1.0}


def ops():
    from statecatcher_amd import ops as o
    return o


def cell(q, k, v, ig, fg, c0, n0, m0):
    return ops().mlstm_chunkwise(q, k, v, ig, fg, c0, n0, m0, return_last_states=True)


def dispatcher_op(q, k, v, ig, fg, c0, n0, m0):
    from statecatcher_amd import torch_library
    return torch_library.mlstm(q, k, v, ig, fg, c0, n0, m0)


def run(case, w, fn=cell):
    """The cell on the GPU and the gradients of weighted_loss: the same dict as reference()."""
    leaves = {k: case[k].to(DEV).requires_grad_(True) for k in LEAVES if k in case}
    m0 = case["m0"].to(DEV) if "m0" in case else None
    h, (c, n, m) = fn(*[leaves.get(k) for k in LEAVES], m0)
    weighted_loss(case, h.float(), c, n, w, to=lambda t: t.to(DEV)).backward()
    torch.cuda.synchronize()
    return {"h": h.detach(), "cT": c.detach(), "nT": n.detach(), "mT": m.detach(),
            "grad": {k: t.grad for k, t in leaves.items()}}


def _err(got, ref):
    g, r = got.detach().double().cpu(), ref.double()
    rel = float((g - r).norm() / max(float(r.norm()), 1e-300))
    cos = float((g * r).sum() / max(float(g.norm() * r.norm()), 1e-300))
    return rel, cos


def compare(label, got, ref, T, rows=False, loose=None):
    """Print every error, then assert the module's bounds.  rows: every sequence bh on its own
    as well (a permutation of sequences cannot pass).  loose: {leaf: (rel, cos)} bounds of a
    case shown to be bf16 rounding (check())."""
    loose = loose or {}
    lines = []
    for name in ("h", "cT", "nT"):
        lines.append(f"{name} {_err(got[name], ref[name])[0]:.2e}")
    lines.append(f"mT {float((got['mT'].double().cpu() - ref['mT']).abs().max()):.1e}")
    for name, r in ref["grad"].items():
        g = got["grad"][name]
        rel, cos = (0.0, 1.0) if g is None else _err(g, r)
        lines.append(f"d{name} {rel:.2e}" + (f" cos {cos:.5f}" if name.endswith("gate") else ""))
    print(f"{label}: " + "; ".join(lines))

    def each(name, g, r, check):
        if not rows:
            return check(g, r)
        B, NH = r.shape[:2]
        for b in range(B):
            for hd in range(NH):
                try:
                    check(g[b, hd], r[b, hd])
                except AssertionError as e:
                    raise AssertionError(f"{label} {name} sequence ({b}, {hd}): {e}") from e

    for name in ("h", "cT", "nT"):
        each(name, got[name], ref[name], lambda g, r: close(g, r, 1e-2))
    np.testing.assert_allclose(got["mT"].cpu().numpy(), ref["mT"].numpy(), rtol=1e-5, atol=1e-5)

    for name, r in ref["grad"].items():
        g = got["grad"][name]
        brel, bcos = loose.get(name, (5e-2 if name.endswith("gate") and T >= 192 else 3e-2, 0.999))

        def gate(g, r, brel=brel, bcos=bcos):
            rel, cos = _err(g, r)
            assert cos >= bcos and rel <= brel, (rel, cos)

        if float(r.abs().max()) == 0.0:   # q under a state-only loss: exactly no gradient
            assert g is None or float(g.abs().max()) == 0.0, name
        elif name.endswith("gate") and T >= 192:
            each("d" + name, g, r, gate)
        else:
            each("d" + name, g, r, lambda g, r, brel=brel: close(g, r, brel))


def check(label, case, w, T, fn=cell, rows=False, loose=None):
    """loose: a bf16 case that misses a bound through rounding, not a defect.  It is shown on the
    same case every run: the f16 cell (8x finer mantissa) must be at least 4x closer to fp64
    than the bf16 cell on each loosened tensor; the bound is then twice the error measured when
    the case was added, never above 1e-1 (DESIGN.md 3.2c lists both cells' numbers)."""
    ref = reference(case, w)
    if case["q"].dtype == torch.float16:
        assert_fits_f16(ref)
    got = run(case, w, fn)
    if loose:
        assert case["q"].dtype == torch.bfloat16 and all(b <= 1e-1 for b, _ in loose.values())
        twin = draw_case(*case["key"][:5], torch.float16, *case["key"][6:])
        tref = reference(twin, w)
        assert_fits_f16(tref)
        tgot = run(twin, w, fn)
        for name in loose:
            e16, ebf = _err(tgot["grad"][name], tref["grad"][name])[0], _err(got["grad"][name], ref["grad"][name])[0]
            print(f"{label}: d{name} f16 cell {e16:.2e} against bf16 cell {ebf:.2e}")
            assert 4 * e16 <= ebf, (name, e16, ebf)
    compare(label, got, ref, T, rows, loose)


# Seeds: 1, except where the f16 case at seed 1 has fp64 gradients beyond f16's range
# (mlstm_cases.assert_fits_f16; found from the fp64 side alone): the smallest seed that fits.
# bf16 runs the same seed, so that the two cells are compared with fp64 on one case.


# ------------------------------------------------------------ 1. head sizes, four chunks ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("DQ,DV", [(32, 64), (64, 64), (64, 128), (96, 192)])
def test_every_head_size_over_four_chunks_with_state(DQ, DV, dtype):
    """Every compiled (DQ, DV), T = 256 (a first, two middle and a last chunk for the reverse
    walk), an initial state in and its gradient out."""
    c = draw_case(1, 3, 256, DQ, DV, dtype, "default", True, seed=3 if (DQ, DV) == (32, 64) else 1)
    check(f"({DQ},{DV}) {dtype} nc=4", c, H_ONLY, 256)


# ------------------------------------------------------------ 2. final-state gradient ----
@pytest.mark.parametrize("fn", [cell, dispatcher_op], ids=["cell", "op"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("DQ,DV", [(32, 64), (96, 192)])
def test_final_state_gradient_alone(DQ, DV, dtype, fn):
    """Loss (cT.Rc).sum() + (nT.Rn).sum(), h unused (dh is None in the backward): every input
    gradient against fp64, through ops.MLSTMFn and through torch.ops.statecatcher.mlstm_fwd.
    The final state depends on the last forget gate with no query partner, so d fgate needs
    <dC_T, C~_T> + <dn_T, n~_T> next to the pair identity q.dq - k.dk
    (ops._mlstm_state_grad_term); without it d fgate is off by more than 100% here."""
    c = draw_case(1, 3, 256, DQ, DV, dtype, "default", True)
    check(f"state-only loss ({DQ},{DV}) {dtype} {fn.__name__}", c, STATE_ONLY, 256, fn)


def test_final_state_gradient_op_bitwise_equals_cell():
    c = draw_case(1, 3, 256, 32, 64, torch.bfloat16, "default", True)
    a, b = run(c, STATE_ONLY, cell), run(c, STATE_ONLY, dispatcher_op)
    for k in LEAVES:
        assert torch.equal(a["grad"][k], b["grad"][k]), k


@pytest.mark.parametrize("kernel_dtype", ["bfloat16", "float16"])
def test_final_state_gradient_core_equals_composed(kernel_dtype, monkeypatch):
    """The same state-only loss through ops.MLSTMCoreFn (dy is None) against the composed path
    (soft caps, MLSTMFn, gated head norm), as test_mlstm_core_equals_composed_ops is built:
    state bit-identical, gradients to 1e-2.  The composed path is the cell checked against fp64
    above, so the core path carries the final-state term too."""
    from statecatcher_amd import xlstm
    cfg = xlstm.xLSTMLargeConfig(embedding_dim=256, num_heads=4, num_blocks=1, vocab_size=64,
                                 autocast_kernel_dtype=kernel_dtype)
    torch.manual_seed(1)
    layer = xlstm.mLSTMLayer(cfg).to(DEV)
    with torch.no_grad():
        for m in layer._mods():
            m.weight.mul_(3.0)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 256, 256, generator=g).to(DEV)
    st = (0.5 * torch.randn(2, 4, 32, 64, generator=g), 0.5 * torch.randn(2, 4, 32, generator=g),
          torch.randn(2, 4, 1, generator=g))
    Rc, Rn = torch.randn(2, 4, 32, 64, generator=g).to(DEV), torch.randn(2, 4, 32, generator=g).to(DEV)
    res = []
    for core in (True, False):
        if not core:
            monkeypatch.setattr(xlstm.ops, "mlstm_core_supported", lambda *a: False)
        layer.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        sti = tuple(t.to(DEV).requires_grad_(i < 2) for i, t in enumerate(st))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, (c, n, m) = layer(xi, sti)
        ((c * Rc).sum() + (n * Rn).sum()).backward()
        named = {"x": xi.grad, "c0": sti[0].grad, "n0": sti[1].grad}
        named.update({k: p.grad for k, p in layer.named_parameters() if p.grad is not None})
        res.append(((c, n, m), named))
    for u, v in zip(res[0][0], res[1][0]):
        assert torch.equal(u, v)
    for k in res[0][1].keys() - res[1][1].keys():   # (no gradient there: the core node's zeros)
        assert not res[0][1][k].any(), k
    assert res[1][1].keys() <= res[0][1].keys()
    rels = {k: _err(res[0][1][k], res[1][1][k].cpu())[0] for k in res[1][1]
            if float(res[1][1][k].abs().max()) > 0}
    print(f"core vs composed, state-only loss ({kernel_dtype}):",
          {k: f"{r:.1e}" for k, r in rels.items()})
    assert any("fgate" in k for k in rels)
    for k, r in rels.items():
        assert r <= 1e-2, (k, r)


# ------------------------------------------------------------ 3. carried segments ----
def test_two_carried_segments_backward_equals_one_pass():
    """T = 128 + 128 at (64, 128), bf16: segment 2 starts from segment 1's returned state, not
    detached, and the loss is on both segments' h.  Segment 1's gradients (which receive
    segment 2's through dcT / dnT and the final-state term) against mlstm64 over all 256 steps;
    segment 2's as well.  The gate gradients are sums over the 256 steps of both segments, so
    they take the bound of T >= 192."""
    c = draw_case(1, 3, 256, 64, 128, torch.bfloat16, "default", False)
    ref = reference(c, H_ONLY)
    names = ("q", "k", "v", "igate", "fgate")
    seg = [[c[k][:, :, s].to(DEV).requires_grad_(True) for k in names]
           for s in (slice(0, 128), slice(128, 256))]
    h1, st = cell(*seg[0], None, None, None)
    h2, (cT, nT, mT) = cell(*seg[1], *st)
    h = torch.cat([h1, h2], 2)
    (h.float() * c["R"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"h": h.detach(), "cT": cT.detach(), "nT": nT.detach(), "mT": mT.detach()}
    for i, sl in enumerate((slice(0, 128), slice(128, 256))):
        part = dict(got, grad={k: t.grad for k, t in zip(names, seg[i])})
        rpart = dict(ref, grad={k: ref["grad"][k][:, :, sl] for k in names})
        compare(f"carried segment {i + 1} of 2", part, rpart, 256)


# ------------------------------------------------------------ 4. gate regimes ----
@pytest.mark.parametrize("init", [False, True], ids=["zero-state", "state"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_gate_regimes(regime, dtype, init):
    """(32, 64), T = 192 in the five regimes of tests/mlstm_cases.py; `dead` and `forgetful`
    assert on the fp64 side that they reach the normaliser's floor branch.

    saturated / f16 / with state is the case that showed the f16 backward losing the gradient
    w.r.t. the initial state (d c0 2.70e-1, d n0 3.03e-1 from fp64; bf16 2.6e-3): with gates at
    the cap, rowf_t and dh_t / z_t each span e^{+-25} over a chunk's rows and sat in two f16
    images scaled once per chunk.  mlstm_bw_walk now normalises both per row and combines the
    row factors in fp32 (d c0 3.6e-4, d n0 4.6e-4)."""
    c = draw_case(1, 2, 192, 32, 64, dtype, regime, init,
                  seed=2 if (regime, init) == ("default", False) else 1)
    share = floor_branch_share(c)
    print(f"{regime}: floor-branch share {share:.2f}")
    if regime == "dead":
        assert share >= 0.9
    if regime == "forgetful":
        assert 0.3 <= share <= 0.9
    loose = None
    if (regime, dtype, init) == ("default", torch.bfloat16, True):
        # one row (t = 132 of head 1) whose normaliser nearly cancels carries 99.9% of |dq|^2 and
        # |dk|^2: the tensor errors are that row's bf16 rounding.  Measured bf16 / f16: dq 3.76e-2
        # / 3.43e-4, dk 3.88e-2 / 3.10e-4, d igate 3.64e-2 / 2.49e-4, d fgate 6.51e-2 (cos
        # 0.99885) / 1.35e-3
        loose = {"q": (7.6e-2, 0.999), "k": (7.8e-2, 0.999), "igate": (7.3e-2, 0.999),
                 "fgate": (1e-1, 0.9977)}
    check(f"{regime} {dtype} init={init}", c, H_ONLY, 192, loose=loose)


# ------------------------------------------------------------ 5. grid mappings ----
@pytest.mark.parametrize("B,NH,DQ,DV", [(2, 8, 32, 64), (2, 8, 64, 128), (3, 3, 96, 192)],
                         ids=["xcd-ncb1-bh16", "xcd-ncb2-bh16", "2d-ncb3-bh9"])
def test_grid_mappings_per_sequence(B, NH, DQ, DV):
    """BH = 16 takes the XCD-ordered 1-D grid (BH % 8 == 0; two slices of 8 sequences) with one
    and two column blocks, BH = 9 the 2-D grid with three.  Every sequence is drawn on its own
    and compared on its own."""
    c = draw_case(B, NH, 128, DQ, DV, torch.bfloat16, "default", True)
    # (64, 128): d fgate of sequence (1, 2) alone is 3.64e-2 from fp64 in bf16 and 2.40e-3 in f16
    # (the whole tensor 4.62e-3 / 3.79e-4): rounding, twice the measured error for that tensor
    loose = {"fgate": (7.3e-2, 0.999)} if (DQ, DV) == (64, 128) else None
    check(f"BH={B * NH} ({DQ},{DV})", c, H_ONLY, 128, rows=True, loose=loose)


# ------------------------------------------------------------ 6. chunk-count edges ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_chunk_with_state_and_state_gradient(dtype):
    """T = 64 at (64, 64): the reverse walk's first and last chunk coincide."""
    w = {"h": 1.0, "c": 1.0, "n": 1.0}
    c = draw_case(1, 3, 64, 64, 64, dtype, "default", True)
    check(f"nc=1 (64,64) {dtype}", c, w, 64)


@pytest.mark.parametrize("fn", [cell, dispatcher_op], ids=["cell", "op"])
@pytest.mark.parametrize("init", [False, True], ids=["zero-state", "state"])
def test_T0_returns_initial_state(init, fn):
    """T = 0: empty h and the state unchanged -- c0, n0, m0 when given, zeros when not -- and the
    state's gradient passed through to the initial state."""
    c = draw_case(2, 3, 0, 32, 64, torch.bfloat16, "default", init)
    leaves = {k: c[k].to(DEV).requires_grad_(True) for k in LEAVES if k in c}
    m0 = c["m0"].to(DEV) if init else None
    h, (cT, nT, mT) = fn(*[leaves.get(k) for k in LEAVES], m0)
    assert h.shape == (2, 3, 0, 64) and cT.shape == (2, 3, 32, 64)
    assert nT.shape == (2, 3, 32) and mT.shape == (2, 3, 1)
    if init:
        assert torch.equal(cT, leaves["c0"]) and torch.equal(nT, leaves["n0"])
        assert torch.equal(mT, m0)
        Rc, Rn = c["Rc"].to(DEV), c["Rn"].to(DEV)
        ((cT * Rc).sum() + (nT * Rn).sum()).backward()
        assert torch.equal(leaves["c0"].grad, Rc) and torch.equal(leaves["n0"].grad, Rn)
    else:
        assert not cT.any() and not nT.any() and not mT.any()


# ------------------------------------------------------------ 7. f16 gradient scaling ----
@pytest.mark.parametrize("w", [{"h": 1e-6}, {"h": 1.0, "c": 1e3}], ids=["dh-1e-6", "dcT-1e3"])
def test_f16_gradient_scaling(w):
    """(96, 192), f16, T = 256.  dh-1e-6: the incoming dh is below f16's normal range.  dcT-1e3:
    the carried dC~ (bounded by 2^10 in the walk) sets the per-chunk gradient scale, not dnum.
    Relative errors are scale-free: the usual bounds.
    dh reaches the cell as an f16 tensor (autograd casts h's gradient to h's dtype), so at 1e-6
    it sits on f16's subnormal grid of 6e-8 before any kernel runs; that cast alone moves the
    fp64 gradients by 5e-2.  Like q / k / v, the 1e-6 R is therefore rounded to f16 before both
    sides see it: the kernel's handling of such a dh is what is measured."""
    c = draw_case(1, 3, 256, 96, 192, torch.float16, "default", True)
    if w == {"h": 1e-6}:
        c = dict(c, key=c["key"] + ("R 1e-6 in f16",), R=(1e-6 * c["R"]).half().float())
        assert 0 < float(c["R"].abs().max()) < 6.1e-5   # all of dh below f16's normal range
        w = H_ONLY
    check(f"f16 scaling {w}", c, w, 256)
