"""GPU parity of the fused CTC (HIP) against ATen fixtures and the fp64 oracle, and of the
greedy decoder (integer path: bit-exact) against the reference decoder fixtures.
Tolerances: nll 1e-4 relative (fp32 log-space recursions); gradients 1e-4 absolute on the
softmax-scale quantities (|grad| <= 1) for fp32 logits, 2e-2 for bf16 logits / bf16 gradients.
"""
import numpy as np
import pytest
import torch

from oracle import ctc as octc
from oracle import decode as odec
from tests.conftest import cases, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def sc():
    import statecatcher_amd as s
    return s


@pytest.mark.parametrize("name", cases(load_golden("ctc"), "logits"))
def test_ctc_fused_vs_aten_fixture(name):
    z = load_golden("ctc")
    x = torch.as_tensor(z[name + "/logits"]).float().to(DEV).requires_grad_(True)
    tg = torch.as_tensor(z[name + "/targets"]).to(DEV)
    il, tl = z[name + "/in_lens"].tolist(), z[name + "/tgt_lens"].tolist()
    nll = sc().ctc_nll(x, tg, il, tl)
    ref = z[name + "/nll"]
    got = nll.detach().cpu().numpy()
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-4, atol=1e-4)
    # mean + zero_infinity reduction and its gradient (nn.CTCLoss semantics)
    loss = sc().ctc_loss(x, tg, il, tl, blank=0, reduction="mean", zero_infinity=True)
    np.testing.assert_allclose(loss.item(), float(z[name + "/mean_loss"]), rtol=1e-4, atol=1e-6)
    loss.backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), z[name + "/mean_grad"], rtol=1e-3, atol=2e-6)


@pytest.mark.parametrize("name", ["basic", "repeats", "long"])
def test_ctc_logprob_interface_vs_aten(name):
    """CTCLoss.forward takes (T,B,V) log-probs exactly like nn.CTCLoss (train.py:142)."""
    z = load_golden("ctc")
    x = torch.as_tensor(z[name + "/logits"]).float().to(DEV).requires_grad_(True)
    tg = torch.as_tensor(z[name + "/targets"]).to(DEV)
    il, tl = z[name + "/in_lens"].tolist(), z[name + "/tgt_lens"].tolist()
    crit = sc().CTCLoss(blank=0, zero_infinity=True)
    loss = crit(x.log_softmax(-1).transpose(0, 1), tg, il, tl)
    np.testing.assert_allclose(loss.item(), float(z[name + "/mean_loss"]), rtol=1e-4, atol=1e-6)
    loss.backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), z[name + "/mean_grad"], rtol=1e-3, atol=2e-6)


def test_ctc_full_size_vs_aten_cpu():
    """C2 shape: B=32, T=1500, V=1024, U in [50,150] vs ATen ctc_loss on CPU (fp64)."""
    g = torch.Generator().manual_seed(4321)
    B, T, V = 32, 1500, 1024
    logits = torch.randn(B, T, V, generator=g) * 2
    tl = torch.randint(50, 151, (B,), generator=g)
    il = torch.full((B,), T, dtype=torch.int64)
    il[3] = 1000
    tg = torch.randint(1, V, (B, 150), generator=g)
    for b in range(B):
        tg[b, tl[b]:] = 0
    x = logits.to(DEV).requires_grad_(True)
    loss = sc().ctc_loss(x, tg.to(DEV), il, tl)
    loss.backward()
    xr = logits.double().requires_grad_(True)
    ref = torch.nn.CTCLoss(blank=0, zero_infinity=True)(xr.log_softmax(-1).transpose(0, 1), tg, il, tl)
    ref.backward()
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
    # the gradient to north_star's 1e-3 in norm (measured 3.3e-4 with the per-frame emission
    # shift of ctc.hip; 2.5e-3 before it)
    g64 = xr.grad.numpy()
    assert np.linalg.norm(x.grad.cpu().numpy() - g64) / np.linalg.norm(g64) <= 1e-3
    # at least as accurate as the reference's own criterion in fp32 (ATen ctc_loss, CPU fp32)
    x32 = logits.clone().requires_grad_(True)
    torch.nn.CTCLoss(blank=0, zero_infinity=True)(x32.log_softmax(-1).transpose(0, 1), tg, il, tl).backward()
    rg = xr.grad.numpy()
    ours = np.linalg.norm(x.grad.cpu().numpy() - rg) / np.linalg.norm(rg)
    aten32 = np.linalg.norm(x32.grad.numpy() - rg) / np.linalg.norm(rg)
    print(f"CTC grad rel err vs fp64: HIP {ours:.2e}, ATen fp32 {aten32:.2e}")
    assert ours <= max(aten32, 1e-4)


@pytest.mark.parametrize("U", [57, 100, 150, 200, 300, 1007])
def test_ctc_long_targets_many_waves_vs_aten_cpu(U):
    """Targets from the one-wave lattice (U + 1 <= 256 pairs: 1, 2, 3 and 4 pairs per lane at
    U = 57, 100, 150, 200) to the multi-wave one (U = 300, 1007: 6 and 16 waves, K = 24 / 4 steps
    between halo exchanges), with runs of repeated labels (no skip transition) and blank-free
    stretches, vs ATen fp64 on CPU; U = 1007 is the longest target the ABI accepts."""
    g = torch.Generator().manual_seed(U)
    B, V = 2, 40
    T = 2 * U + 40
    logits = torch.randn(B, T, V, generator=g) * 2
    tg = torch.randint(1, V, (B, U), generator=g)
    tg[0, 10:20] = 7                      # a run of repeats
    tl = torch.tensor([U, U - 3])
    tg[1, U - 3:] = 0
    il = torch.tensor([T, T - 17])
    x = logits.to(DEV).requires_grad_(True)
    nll = sc().ctc_nll(x, tg.to(DEV), il, tl)
    nll.sum().backward()
    xr = logits.double().requires_grad_(True)
    ref = torch.nn.functional.ctc_loss(xr.log_softmax(-1).transpose(0, 1), tg, il, tl,
                                       reduction="none", zero_infinity=False)
    ref.sum().backward()
    np.testing.assert_allclose(nll.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-4)
    # |grad| <= 1: 1e-4 absolute per element, and 1e-3 in norm (north_star)
    g, g64 = x.grad.cpu().numpy(), xr.grad.numpy()
    np.testing.assert_allclose(g, g64, rtol=1e-2, atol=1e-4)
    rel = np.linalg.norm(g - g64) / np.linalg.norm(g64)
    print(f"U={U}: CTC grad rel err vs fp64 {rel:.2e}")
    assert rel <= 1e-3


def _lattice_case(scales, dtype="f32", is_logits=True):
    """nll / gradient errors of the HIP CTC against ATen fp64 (and ATen fp32) for four sequences
    with the given logit scales (the fourth infeasible); returns a dict (JSON-able).  dtype
    "bf16": the logits rounded to bf16 first (both sides see the rounded values); is_logits
    False: fp32 log-probs in (ATen's log-prob gradient convention on both sides)."""
    g = torch.Generator().manual_seed(int(sum(scales)))
    B, V, U, T = 4, 40, 120, 400
    logits = torch.randn(B, T, V, generator=g)
    for b, sc_ in enumerate(scales):
        logits[b] *= sc_
    if dtype == "bf16":
        logits = logits.bfloat16().float()
    if not is_logits:
        logits = logits.log_softmax(-1)
    tg = torch.randint(1, V, (B, U), generator=g)
    tl = torch.tensor([U, U - 7, U - 20, U])
    il = torch.tensor([T, T - 9, T, U - 10])   # sequence 3: infeasible
    for b in range(B):
        tg[b, tl[b]:] = 0
    x = (logits.bfloat16() if dtype == "bf16" else logits).to(DEV).requires_grad_(True)
    nll = sc().ctc_nll(x, tg.to(DEV), il, tl, is_logits=is_logits)
    xr = logits.double().requires_grad_(True)
    ref = torch.nn.functional.ctc_loss(xr.log_softmax(-1).transpose(0, 1) if is_logits
                                       else xr.transpose(0, 1), tg, il, tl,
                                       reduction="none", zero_infinity=False)
    got, r = nll.detach().cpu().numpy(), ref.detach().numpy()
    out = {"finite_match": bool(np.array_equal(np.isfinite(got), np.isfinite(r))),
           "infeasible_inf": bool(not np.isfinite(got[3]))}
    fin = np.isfinite(r)
    out["nll_rel"] = float(np.max(np.abs(got[fin] - r[fin]) / np.abs(r[fin])))
    nll[:3].sum().backward()
    ref[:3].sum().backward()
    x32 = logits.clone().requires_grad_(True)
    torch.nn.functional.ctc_loss(x32.log_softmax(-1).transpose(0, 1) if is_logits else
                                 x32.transpose(0, 1), tg, il, tl, reduction="none",
                                 zero_infinity=False)[:3].sum().backward()
    g32, g64 = x.grad.float().cpu().numpy(), xr.grad.numpy()
    out["grad_row3_zero"] = bool(not g32[3].any())
    out["grad_rel"] = [float(np.linalg.norm(g32[b] - g64[b]) / np.linalg.norm(g64[b])) for b in range(3)]
    out["aten32_rel"] = [float(np.linalg.norm(x32.grad[b].numpy() - g64[b]) / np.linalg.norm(g64[b]))
                         for b in range(3)]
    return out


@pytest.mark.parametrize("scales", [(2.0, 2.0, 2.0), (8.0, 30.0, 2.0), (100.0, 2.0, 400.0)])
def test_ctc_lattices_with_sharp_logits_vs_aten_cpu(scales):
    """The log-space lattice with its per-sequence hand-over to the exact one (ctc_x64_kernel):
    logits x 30 .. x 400 over V = 40 (log-prob gaps of hundreds of bits) drift the log-space
    lattice past kDrift, while their neighbours in the same launch stay where they are.  nll 1e-4
    and gradient vs ATen fp64, with an infeasible sequence (T < U) among them (inf, zero
    gradient)."""
    out = _lattice_case(scales)
    print(scales, out)
    assert out["finite_match"] and out["infeasible_inf"] and out["grad_row3_zero"]
    assert out["nll_rel"] <= 1e-4
    for b in range(3):
        # 1e-3 (north_star) for every case: logits x 100 .. x 400 (log-probs down to -2000 nats)
        # drift the log-space lattice past kDrift between re-centrings, and the exact lattice
        # (ctc_x64_kernel) recomputes those sequences; ATen fp32 is 1e-2 .. 7e-2 off on them
        assert out["grad_rel"][b] <= 1e-3


@pytest.mark.parametrize("dtype,is_logits", [("bf16", True), ("f32", False)])
def test_ctc_exact_lattice_bf16_logits_and_log_probs(dtype, is_logits):
    """The exact lattice's other inputs: bf16 logits (emissions read through Elem<bf16>) and fp32
    log-probs (is_logits = 0: no lse), at the sharp scales that send sequences 0 and 2 to it."""
    out = _lattice_case((100.0, 2.0, 400.0), dtype, is_logits)
    print(dtype, is_logits, out)
    assert out["finite_match"] and out["infeasible_inf"] and out["grad_row3_zero"]
    assert out["nll_rel"] <= 1e-4
    # (bf16 gradients: the stored gradient rounds to 2^-9 of each element)
    lim = 1e-3 if dtype == "f32" else 4e-3
    assert max(out["grad_rel"]) <= lim, out["grad_rel"]


def test_ctc_sharp_long_targets_keep_log_space():
    """Targets longer than the exact lattice holds (U = 300 > 255) with logits x 100: the
    log-space lattice drifts past kDrift and flags the sequence, but ctc_x64_kernel does not run
    for U > 255, so the gradient must read the LOG-SPACE offsets (one per re-centring), not the
    exact lattice's per-step ones (it read unwritten offset entries).  A x 2 neighbour
    in the same launch, and the same pair at U = 200 (which the exact lattice does redo)."""
    out = {}
    for U in (300, 200):
        g = torch.Generator().manual_seed(U + 1)
        B, V = 2, 40
        T = 2 * U + 40
        logits = torch.randn(B, T, V, generator=g)
        logits[0] *= 100.0
        logits[1] *= 2.0
        tg = torch.randint(1, V, (B, U), generator=g)
        tl = torch.tensor([U, U - 5])
        tg[1, U - 5:] = 0
        il = torch.tensor([T, T - 11])
        x = logits.to(DEV).requires_grad_(True)
        nll = sc().ctc_nll(x, tg.to(DEV), il, tl)
        nll.sum().backward()
        xr = logits.double().requires_grad_(True)
        ref = torch.nn.functional.ctc_loss(xr.log_softmax(-1).transpose(0, 1), tg, il, tl,
                                           reduction="none", zero_infinity=False)
        ref.sum().backward()
        got, r = nll.detach().cpu().numpy(), ref.detach().numpy()
        gg, g64 = x.grad.cpu().numpy(), xr.grad.numpy()
        assert np.isfinite(gg).all()
        rel = [float(np.linalg.norm(gg[b] - g64[b]) / np.linalg.norm(g64[b])) for b in range(B)]
        out[U] = (np.abs(got - r) / np.abs(r), rel)
        print(f"U={U}: nll rel {out[U][0]}, grad rel {rel}")
        np.testing.assert_allclose(got, r, rtol=1e-4)
        assert rel[1] <= 1e-3
    # U = 200: exact lattice, north_star's 1e-3; U = 300: the log-space lattice at x 100 (fp32
    # rounding of values ~1e4 per step), documented as outside the exact lattice's range
    assert out[200][1][0] <= 1e-3
    assert out[300][1][0] <= 2e-2


def test_ctc_bf16_logits_vs_oracle():
    g = torch.Generator().manual_seed(5)
    B, T, V = 3, 120, 64
    logits = (torch.randn(B, T, V, generator=g) * 2).bfloat16()
    tg = torch.randint(1, V, (B, 20), generator=g)
    il, tl = [120, 90, 40], [20, 11, 0]
    x = logits.to(DEV).requires_grad_(True)
    nll = sc().ctc_nll(x, tg.to(DEV), il, tl)
    nll.sum().backward()
    rn, rg = octc.ctc_loss_grad(logits.float().numpy(), tg.numpy(), il, tl)
    np.testing.assert_allclose(nll.detach().cpu().numpy(), rn, rtol=1e-4)
    np.testing.assert_allclose(x.grad.float().cpu().numpy(), rg, atol=2e-2)


def test_ctc_edge_cases():
    """U=0, infeasible (T < U + repeats), in_len=0 and in_len=1."""
    g = torch.Generator().manual_seed(9)
    B, T, V = 4, 6, 5
    logits = torch.randn(B, T, V, generator=g)
    tg = torch.tensor([[1, 1, 1, 1], [2, 3, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0]])
    il, tl = [6, 0, 1, 6], [4, 2, 1, 0]
    x = logits.to(DEV).requires_grad_(True)
    nll = sc().ctc_nll(x, tg.to(DEV), il, tl)
    rn, rg = octc.ctc_loss_grad(logits.numpy(), tg.numpy(), il, tl)
    got = nll.detach().cpu().numpy()
    assert np.isinf(got[0]) and np.isinf(rn[0])          # 1,1,1,1 needs 7 frames
    assert np.isinf(got[1]) and np.isinf(rn[1])          # in_len 0, U 2
    np.testing.assert_allclose(got[2:], rn[2:], rtol=1e-5)
    loss = sc().ctc_loss(x, tg.to(DEV), il, tl)
    loss.backward()
    gr = x.grad.cpu().numpy()
    assert np.all(gr[0] == 0) and np.all(gr[1] == 0)      # zero_infinity zeroes the rows
    assert np.all(gr[2, 1:] == 0)                          # t >= in_len
    sc_ = octc.ctc_mean_grad_scale(rn, tl)
    np.testing.assert_allclose(gr[2:], (rg * sc_[:, None, None])[2:], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("pref", ["ties", "big"])
def test_greedy_decoder_bit_exact_vs_reference(pref):
    z = load_golden("greedy")
    lp = torch.as_tensor(z[pref + "_lp"]).to(DEV)
    dec = sc().ctc_greedy_decoder(lp, torch.as_tensor(z[pref + "_in_lens"]), blank=0)
    counts, flat = z[pref + "_counts"], z[pref + "_tokens"]
    exp, o = [], 0
    for c in counts:
        exp.append(flat[o:o + c].tolist())
        o += c
    assert dec == exp


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_greedy_full_size_vs_oracle(dtype):
    g = torch.Generator().manual_seed(2)
    B, T, V = 32, 1500, 1024
    # few distinct values -> many ties; blank-heavy rows
    lp = torch.randint(-3, 1, (B, T, V), generator=g).to(dtype)
    lens = torch.randint(0, T + 1, (B,), generator=g)
    dec = sc().ctc_greedy_decoder(lp.to(DEV), lens, blank=0)
    assert dec == odec.ctc_greedy(lp.float().numpy(), lens.numpy(), blank=0)
