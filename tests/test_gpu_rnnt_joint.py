"""GPU parity of the fused RNN-T joiner + loss (rnnt.hip joint_* kernels, ops.RNNTJointFn).

The reference computes RNNTPredictorJoiner (model.py:129-145) -> (B, T, U+1, V) logits ->
log_softmax in fp32 (model.py:93) -> warp_rnnt (gather=True).  The fused kernels never build the
logits; W and z = tanh(enc + pred) enter the MFMA in bf16 with fp32 accumulation.

* Small lattices against an fp64 CPU restatement with the SAME bf16 roundings as the kernels --
  W and z, and the dlogits that enter the backward's dW / dZ MFMAs (oracle/rnnt.py lattice,
  pinned by brute-force alignment sums): nll to 1e-4 relative, the gradients of enc_proj /
  pred_proj outputs, W and bias to 1e-3 in norm (north_star); against fp64 without the dlogits
  rounding to 5e-3 (that rounding's own size).
* A C5-sized lattice (T=1500, U=150, V=1024, B=2) against the unfused HIP path on materialised
  fp32 logits (the validated sc_rnnt_* kernels) with the same roundings: nll 1e-4, gradients
  1e-3 in norm; deterministic.
* The same references slice by slice (d enc / d pred per sequence, dW / d bias per 32-row
  vocabulary block, so a wrong block or sequence cannot hide in the tensor's norm) over the
  kernels' geometry: one and two vocabulary splits (V <= 512 / V > 512, ragged at V = 544),
  t-blocks of 32 frames around their edges and wholly past a sequence's frames, u-splits wider
  than the lattice, a non-zero blank, a sequence without labels, a zero upstream weight.
* compute_loss(mode="rnnt") with RNNTLoss runs the fused path for both joiners, DDP-safe
  (through the joiner's forward), and equals the materialised path.
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as ornnt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def sc():
    import statecatcher_amd as s
    return s


class _Bf16Grad(torch.autograd.Function):
    """Identity forward; the backward rounds the incoming gradient to bf16 (RNE) and hands it on
    in the input's dtype: the joiner backward's dlogits p enter its dW and dZ MFMAs as bf16
    (rnnt.hip joint_bwd_kernel: pack8(p) is the A operand of both), while d bias sums the fp32 p."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def ref_fp64(enc_p, pred_p, W, bias, labels, fl, ll, blank, round_p=False, weights=None):
    """nll and gradients (enc_p, pred_p, W, bias) in fp64 with the kernels' bf16 roundings of W
    and z; round_p: also the bf16 rounding of the dlogits that feed dW / dZ (d bias unrounded).
    Gradients of sum_b weights[b] nll[b] (None: the mean)."""
    e = enc_p.double().cpu().requires_grad_(True)
    p = pred_p.double().cpu().requires_grad_(True)
    w = W.double().cpu().requires_grad_(True)
    b = bias.double().cpu().requires_grad_(True)
    z = torch.tanh(e.unsqueeze(2) + p.unsqueeze(1))
    zq = z + (z.to(torch.bfloat16).double() - z).detach()          # bf16 value, identity grad
    wq = w + (w.to(torch.bfloat16).double() - w).detach()
    mm = zq @ wq.t()
    logits = (_Bf16Grad.apply(mm) if round_p else mm) + b
    lp = logits.log_softmax(-1)
    nll = []
    glp = torch.zeros_like(lp)
    for i in range(lp.shape[0]):
        Tb, Ub = int(fl[i]), int(ll[i])
        if Tb == 0:
            nll.append(np.inf)
            continue
        n, g = ornnt.rnnt_single(lp[i, :Tb, :Ub + 1].detach().numpy(), labels[i, :Ub].numpy(), blank)
        nll.append(n)
        glp[i, :Tb, :Ub + 1] = torch.from_numpy(g) * (1.0 / lp.shape[0] if weights is None
                                                          else float(weights[i]))
    lp.backward(glp)
    return np.array(nll), e.grad, p.grad, w.grad, b.grad


def case(B, T, Umax, V, seed, Tb=None, Ub=None, Din=24):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    joiner = sc().RNNTPredictorJoiner(Din, 16, 64, V)
    with torch.no_grad():
        joiner.joiner.weight.mul_(3.0)   # sharper output than nn.Linear's init
    enc_out = torch.randn(B, T, Din, generator=g)
    labels = torch.randint(1, V, (B, Umax), generator=g)
    fl = torch.tensor(Tb if Tb is not None else [T] * B)
    ll = torch.tensor(Ub if Ub is not None else [Umax] * B)
    return joiner, enc_out, labels, fl, ll


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / max(b.norm(), 1e-30))


@pytest.mark.parametrize("B,T,Umax,V,Tb,Ub", [(3, 37, 7, 64, [37, 20, 33], [7, 3, 0]),
                                              (2, 64, 12, 96, None, [12, 5]),
                                              (2, 5, 1, 32, [5, 1], [1, 1]),
                                              (1, 70, 40, 128, None, None)])
def test_fused_joint_vs_fp64(B, T, Umax, V, Tb, Ub):
    joiner, enc_out, labels, fl, ll = case(B, T, Umax, V, B * 100 + T, Tb, Ub)
    joiner = joiner.to(DEV)
    prefix = torch.cat([torch.zeros(B, 1, dtype=torch.long), labels], 1).to(DEV)
    enc_p, pred_p, W, bias = joiner(enc_out.to(DEV), prefix, project_only=True)
    enc_p = enc_p.detach().requires_grad_(True)
    pred_p = pred_p.detach().requires_grad_(True)
    W = W.detach().requires_grad_(True)
    bias = bias.detach().requires_grad_(True)
    nll = sc().ops.RNNTJointFn.apply(enc_p, pred_p, W, bias, labels.to(DEV), fl.to(DEV), ll.to(DEV), 0)
    nll.mean().backward()
    args = (enc_p.detach(), pred_p.detach(), W.detach(), bias.detach(), labels, fl, ll, 0)
    rn, *plain = ref_fp64(*args)
    _, *rounded = ref_fp64(*args, round_p=True)
    np.testing.assert_allclose(nll.detach().cpu().numpy(), rn, rtol=1e-4)
    for got, ref, refq, name in zip([enc_p.grad, pred_p.grad, W.grad, bias.grad], plain, rounded,
                                    ["enc", "pred", "W", "bias"]):
        assert torch.isfinite(got).all(), name
        print(f"fused joint B={B} T={T} U={Umax} V={V} {name}: rel {rel(got, refq):.2e} vs fp64 "
              f"with the kernel's roundings (plain fp64 with W / z rounded: {rel(got, ref):.2e})")
        # north_star's 1e-3 against the reference that models every bf16 rounding the kernels
        # make; against fp64 without the dlogits rounding the gap is that rounding itself (p sums
        # to ~0 over the vocabulary, so dZ = p W cancels and magnifies it): measured <= 1.8e-3
        assert rel(got, refq) <= 1e-3, (name, rel(got, refq))
        assert rel(got, ref) <= 5e-3, (name, rel(got, ref))


def slice_rels(got, ref, dim_slices):
    """Relative error in norm of every slice; a slice whose reference is exactly zero must be
    exactly zero (reported as 0 or inf)."""
    out = []
    for sl in dim_slices:
        g, r = got[sl].double().cpu(), ref[sl].double().cpu()
        if float(r.norm()) == 0.0:
            out.append(0.0 if not g.any() else float("inf"))
        else:
            out.append(float((g - r).norm() / r.norm()))
    return out


_V5 = [(2, 9, 4, V, [9, 6], [4, 2], 0, None) for V in (160, 512, 544, 800, 1024)]
_T4 = [(2, T, 2, 64, [T, T - 2], [2, 1], 0, None) for T in (31, 32, 33, 65)]
_U5 = [(2, 9, U, 64, [9, 7], [U, U // 2], 0, None) for U in (0, 2, 4, 8, 9)]
SLICE_CASES = _V5 + _T4 + _U5 + [
    (2, 70, 3, 64, [70, 20], [3, 2], 0, None),          # t-blocks 1 and 2 lie past Tb = 20
    (2, 9, 4, 64, [9, 6], [4, 2], 33, None),            # non-zero blank, mid-block
    (2, 9, 4, 64, [9, 6], [4, 2], 63, None),            # blank = V - 1
    (2, 9, 4, 544, [9, 6], [4, 2], 543, None),          # ... in the ragged second split
    (2, 9, 4, 64, [9, 6], [4, 0], 0, None),             # a sequence without labels
    (2, 9, 4, 64, [9, 6], [4, 2], 0, [1.0, 0.0]),       # zero upstream weight: an exactly zero row
    (2, 9, 4, 1024, [9, 6], [4, 2], 0, [-0.5, 1e3]),
]


@pytest.mark.parametrize("B,T,Umax,V,Tb,Ub,blank,w", SLICE_CASES)
def test_fused_joint_slices_vs_fp64(B, T, Umax, V, Tb, Ub, blank, w):
    """Every sequence's d enc / d pred and every 32-row vocabulary block of dW / d bias against
    fp64: 1e-3 in norm with the kernels' roundings, 5e-3 plain (the numbers of
    test_fused_joint_vs_fp64, applied per slice)."""
    joiner, enc_out, labels, fl, ll = case(B, T, Umax, V, 7 * T + Umax + V + blank, Tb, Ub)
    labels[labels == blank] = 0 if blank else 1
    joiner = joiner.to(DEV)
    prefix = torch.cat([torch.zeros(B, 1, dtype=torch.long), labels], 1).to(DEV)
    enc_p, pred_p, W, bias = (t.detach().requires_grad_(True)
                              for t in joiner(enc_out.to(DEV), prefix, project_only=True))
    nll = sc().ops.RNNTJointFn.apply(enc_p, pred_p, W, bias, labels.to(DEV), fl.to(DEV), ll.to(DEV),
                                     blank)
    wt = torch.tensor(w if w is not None else [1.0 / B] * B)
    (nll * wt.to(DEV)).sum().backward()
    args = (enc_p.detach(), pred_p.detach(), W.detach(), bias.detach(), labels, fl, ll, blank)
    rn, *plain = ref_fp64(*args, weights=wt)
    _, *rounded = ref_fp64(*args, round_p=True, weights=wt)
    np.testing.assert_allclose(nll.detach().cpu().numpy(), rn, rtol=1e-4)
    per_seq = [(slice(b, b + 1),) for b in range(B)]
    per_blk = [(slice(v, v + 32),) for v in range(0, V, 32)]
    worst = {}
    for got, ref, refq, name, sls in zip([enc_p.grad, pred_p.grad, W.grad, bias.grad], plain, rounded,
                                         ["enc", "pred", "W", "bias"],
                                         [per_seq, per_seq, per_blk, per_blk]):
        assert torch.isfinite(got).all(), name
        rq, rp = slice_rels(got, refq, sls), slice_rels(got, ref, sls)
        worst[name] = (max(rq), max(rp))
        assert max(rq) <= 1e-3, (name, "rounded reference", rq)
        assert max(rp) <= 5e-3, (name, "plain fp64", rp)
    print(f"fused joint slices T={T} U={Umax} V={V} blank={blank} w={w}: worst slice (rounded, "
          "plain) " + ", ".join(f"{k} {a:.1e} {b:.1e}" for k, (a, b) in worst.items()))
    if w is not None and 0.0 in w:
        z = w.index(0.0)
        assert not enc_p.grad[z].any() and not pred_p.grad[z].any()


def test_fused_joint_zero_frames_is_inf():
    joiner, enc_out, labels, fl, ll = case(2, 9, 3, 32, 5, [9, 0], [3, 2])
    joiner = joiner.to(DEV)
    prefix = torch.cat([torch.zeros(2, 1, dtype=torch.long), labels], 1).to(DEV)
    enc_p, pred_p, W, bias = joiner(enc_out.to(DEV), prefix, project_only=True)
    nll = sc().ops.RNNTJointFn.apply(enc_p, pred_p, W, bias, labels.to(DEV), fl.to(DEV), ll.to(DEV), 0)
    v = nll.detach().cpu().numpy()
    assert np.isfinite(v[0]) and np.isinf(v[1])


def test_fused_joint_c5_size_vs_materialised_path():
    """T=1500, U=150, V=1024 (C5 lattice), B=2: fused vs the unfused sc_rnnt_* kernels on
    materialised fp32 logits built from the same bf16-rounded z and W."""
    B, T, Umax, V = 2, 1500, 150, 1024
    joiner, enc_out, labels, fl, ll = case(B, T, Umax, V, 77, Din=512)
    joiner = joiner.to(DEV)
    prefix = torch.cat([torch.zeros(B, 1, dtype=torch.long), labels], 1).to(DEV)
    enc_p, pred_p, W, bias = (t.detach() for t in joiner(enc_out.to(DEV), prefix, project_only=True))
    labels, fl, ll = labels.to(DEV), fl.to(DEV), ll.to(DEV)
    outs = []
    for _ in range(2):
        e, p, w, b = (t.clone().requires_grad_(True) for t in (enc_p, pred_p, W, bias))
        nll = sc().ops.RNNTJointFn.apply(e, p, w, b, labels, fl, ll, 0)
        nll.mean().backward()
        outs.append([nll.detach(), e.grad, p.grad, w.grad, b.grad])
    for x, y in zip(*outs):
        assert torch.equal(x, y)   # deterministic: fixed-order partial sums, no atomics
    assert all(torch.isfinite(t).all() for t in outs[0])
    # materialised path (fp32 logits, the validated sc_rnnt_* lattice) with the same roundings:
    # bf16 z and W, and the dlogits rounded to bf16 before the dW / dZ products (_Bf16Grad)
    e, p, w, b = (t.clone().requires_grad_(True) for t in (enc_p, pred_p, W, bias))
    z = torch.tanh(e.unsqueeze(2) + p.unsqueeze(1))
    zq = z + (z.to(torch.bfloat16).float() - z).detach()
    wq = w + (w.to(torch.bfloat16).float() - w).detach()
    logits = _Bf16Grad.apply(zq @ wq.t()) + b
    nll_u = sc().rnnt_loss(logits, labels, fl, ll, reduction="none", is_logits=True)
    nll_u.mean().backward()
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), nll_u.detach().cpu().numpy(), rtol=1e-4)
    for got, ref, name in zip(outs[0][1:], [e.grad, p.grad, w.grad, b.grad], ["enc", "pred", "W", "bias"]):
        r = rel(got, ref)
        print(f"C5 lattice {name}: rel {r:.2e}")
        assert r <= 1e-3, (name, r)


def _count_fused(monkeypatch):
    import statecatcher_amd.model as m
    calls = []
    orig = m.rnnt_joint_loss

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(m, "rnnt_joint_loss", counted)
    return calls


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("mode", ["bf16-autocast", "forced"])
def test_compute_loss_rnnt_uses_fused_path(compact, mode, monkeypatch):
    """compute_loss(mode='rnnt') with statecatcher RNNTLoss takes the fused path under a 16-bit
    autocast (or when forced), equal to the materialised joiner + criterion.forward_logits (the
    reference's data flow) on the same bf16-rounded joiner operands."""
    B, T, Umax, V = 2, 50, 6, 64
    Cls = sc().RNNTCompactPredictorJoiner if compact else sc().RNNTPredictorJoiner
    torch.manual_seed(3)
    joiner = Cls(V, 16, 64, V).to(DEV)
    enc = torch.randn(B, T, V, device=DEV)
    tokens = torch.randint(1, V, (B, Umax), device=DEV)
    in_lens, tgt_lens = [T, 41], [Umax, 4]
    tokens[1, 4:] = 0

    class Enc(torch.nn.Module):
        def forward(self, feats, masks, states=None):
            return feats, None
    calls = _count_fused(monkeypatch)
    crit = sc().RNNTLoss(blank=0, fused_joint=True if mode == "forced" else None)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "forced"):
        loss, _, _, _ = sc().compute_loss("rnnt", crit, Enc(), enc, None, tokens, in_lens, tgt_lens,
                                          0, use_rnnt_joiner=joiner, compact=compact)
    assert calls, "the fused joiner path was not taken"
    loss.backward()
    g_fused = [p.grad.clone() for p in joiner.parameters()]
    joiner.zero_grad()
    prefix = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=DEV), tokens], 1)
    if compact:
        logits = joiner(enc, prefix, in_lens, tgt_lens)
    else:
        logits = joiner(enc, prefix)
    ref = crit.forward_logits(logits, tokens, in_lens, tgt_lens, blank_id=0, compact=compact)
    ref.backward()
    print(f"{mode} compact={compact}: loss {loss.item():.6f} vs {ref.item():.6f}; grad rel "
          + " ".join(f"{rel(gf, p.grad):.2e}" for gf, p in zip(g_fused, joiner.parameters())))
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=2e-3)
    for gf, p in zip(g_fused, joiner.parameters()):
        assert rel(gf, p.grad) < 3e-2


@pytest.mark.parametrize("compact", [False, True])
def test_compute_loss_rnnt_fp32_keeps_fp32_logits(compact, monkeypatch):
    """Plain fp32 training (no autocast): compute_loss keeps the reference's fp32 joiner logits
    (materialised path, no bf16 rounding of W or z) -- bitwise the same as building the logits
    and calling criterion.forward_logits directly."""
    B, T, Umax, V = 2, 40, 5, 64
    Cls = sc().RNNTCompactPredictorJoiner if compact else sc().RNNTPredictorJoiner
    torch.manual_seed(4)
    joiner = Cls(V, 16, 64, V).to(DEV)
    enc = torch.randn(B, T, V, device=DEV)
    tokens = torch.randint(1, V, (B, Umax), device=DEV)
    in_lens, tgt_lens = [T, 33], [Umax, 3]
    tokens[1, 3:] = 0

    class Enc(torch.nn.Module):
        def forward(self, feats, masks, states=None):
            return feats, None
    calls = _count_fused(monkeypatch)
    crit = sc().RNNTLoss(blank=0)
    loss, _, _, _ = sc().compute_loss("rnnt", crit, Enc(), enc, None, tokens, in_lens, tgt_lens, 0,
                                      use_rnnt_joiner=joiner, compact=compact)
    assert not calls, "fp32 training must not take the bf16 fused joiner"
    prefix = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=DEV), tokens], 1)
    logits = joiner(enc, prefix, in_lens, tgt_lens) if compact else joiner(enc, prefix)
    assert logits.dtype == torch.float32
    ref = crit.forward_logits(logits, tokens, in_lens, tgt_lens, blank_id=0, compact=compact)
    assert torch.equal(loss.detach(), ref.detach())


def test_compute_loss_rnnt_fp16_autocast_keeps_materialised_joiner(monkeypatch):
    """Under float16 autocast (the reference's own training dtype, train.py:516) the automatic
    choice keeps the materialised joiner: the fused kernels' bf16 rounding of W and z is coarser
    than float16's."""
    B, T, Umax, V = 2, 30, 4, 64
    torch.manual_seed(5)
    joiner = sc().RNNTPredictorJoiner(V, 16, 64, V).to(DEV)
    enc = torch.randn(B, T, V, device=DEV)
    tokens = torch.randint(1, V, (B, Umax), device=DEV)

    class Enc(torch.nn.Module):
        def forward(self, feats, masks, states=None):
            return feats, None
    calls = _count_fused(monkeypatch)
    with torch.autocast("cuda", dtype=torch.float16):
        loss, _, _, _ = sc().compute_loss("rnnt", sc().RNNTLoss(blank=0), Enc(), enc, None, tokens,
                                          [T, T], [Umax, Umax], 0, use_rnnt_joiner=joiner)
    assert not calls, "float16 autocast must not take the bf16 fused joiner"
    assert torch.isfinite(loss)
