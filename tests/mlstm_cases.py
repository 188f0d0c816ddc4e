"""Inputs and the fp64 side of the mLSTM parity tests (test infrastructure, no GPU needed).

Gate regimes, all inside the xLSTM layer's soft cap of +-15:
  default    igate 3 N(0,1),          fgate 2 N(0,1) + 3    the regime of the older tests
  dead       igate -4 + 0.5 N(0,1),   fgate 6 + N(0,1)      normaliser floor e^{-m} on ~every row
  forgetful  igate N(0,1),            fgate -6 + 2 N(0,1)   state wiped each step, both branches
  saturated  15 tanh(3 N(0,1)),       15 tanh(3 N(0,1) + 1) gates at the cap, m jumps of +-25
  longmem    igate 0.5 N(0,1),        fgate 12              no decay: n~, C~ grow over the sequence
"""
import torch

from tests.torch_ref import mlstm64

REGIMES = {
    "default": lambda rn, s: (3 * rn(*s), 2 * rn(*s) + 3),
    "dead": lambda rn, s: (-4 + 0.5 * rn(*s), 6 + rn(*s)),
    "forgetful": lambda rn, s: (rn(*s), -6 + 2 * rn(*s)),
    "saturated": lambda rn, s: (15 * torch.tanh(3 * rn(*s)), 15 * torch.tanh(3 * rn(*s) + 1)),
    "longmem": lambda rn, s: (0.5 * rn(*s), torch.full(s, 12.0)),
}
LEAVES = ("q", "k", "v", "igate", "fgate", "c0", "n0")


def draw_case(B, NH, T, DQ, DV, dtype, regime="default", init=True, seed=1):
    """CPU tensors from one seeded generator: q / k / v randn rounded to the cell dtype (both
    sides see the rounded values), fp32 gates of the regime, the initial state c0, n0 ~ 0.5 N,
    m0 ~ N when init, and the loss weights R [B,NH,T,DV], Rc [B,NH,DQ,DV], Rn [B,NH,DQ].  Every
    sequence bh is drawn independently."""
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g)
    c = {"key": (B, NH, T, DQ, DV, dtype, regime, init, seed)}
    c["q"], c["k"] = rn(B, NH, T, DQ).to(dtype), rn(B, NH, T, DQ).to(dtype)
    c["v"] = rn(B, NH, T, DV).to(dtype)
    c["igate"], c["fgate"] = REGIMES[regime](rn, (B, NH, T))
    if init:
        c["c0"], c["n0"], c["m0"] = 0.5 * rn(B, NH, DQ, DV), 0.5 * rn(B, NH, DQ), rn(B, NH, 1)
    c["R"], c["Rc"], c["Rn"] = rn(B, NH, T, DV), rn(B, NH, DQ, DV), rn(B, NH, DQ)
    return c


def weighted_loss(case, h, c, n, w, to=lambda t: t):
    """w["h"] (h.R).sum() + w["c"] (C.Rc).sum() + w["n"] (n.Rn).sum() over the weights given."""
    terms = []
    for key, x, r in (("h", h, "R"), ("c", c, "Rc"), ("n", n, "Rn")):
        if w.get(key) is not None:
            terms.append(w[key] * (x * to(case[r])).sum())
    return sum(terms)


_REF = {}


def reference(case, w):
    """mlstm64 in fp64 on the case's (rounded) inputs and the gradients of weighted_loss:
    {"h", "cT", "nT", "mT", "grad": {leaf: gradient}}.  Computed once per (case, loss) and
    shared; callers leave it unchanged."""
    key = (case["key"], tuple(sorted(w.items())))
    if key not in _REF:
        leaves = {k: case[k].double().requires_grad_(True) for k in LEAVES if k in case}
        m0 = case["m0"].double() if "m0" in case else None
        h, (c, n, m) = mlstm64(*[leaves.get(k) for k in LEAVES], m0)
        weighted_loss(case, h, c, n, w, to=lambda t: t.double()).backward()
        _REF[key] = {"h": h.detach(), "cT": c.detach(), "nT": n.detach(), "mT": m.detach(),
                     "grad": {k: torch.zeros_like(t) if t.grad is None else t.grad
                              for k, t in leaves.items()}}   # (q under a state-only loss)
    return _REF[key]


F16_MAX = 65504.0


def assert_fits_f16(ref):
    """Premise of an f16 case: the cell returns dq / dk / dv in f16, so the fp64 gradients must be
    representable there.  In the default regime a row whose normaliser q.n nearly cancels has
    gradients ~ 1 / den^2 that reach 1e5 at some seeds: inf in f16 whatever the kernel does (a
    dtype limit, not a kernel property).  25% headroom: the elementwise check allows 10% of the
    tensor's scale."""
    for k in ("q", "k", "v"):
        mx = float(ref["grad"][k].abs().max())
        assert mx <= 0.75 * F16_MAX, f"fp64 d{k} reaches {mx:.0f}: not an f16 case, change the seed"


def floor_branch_share(case):
    """Share of rows (b, h, t) whose normaliser takes the floor e^{-m_t}: |s q_t.n~_t| < e^{-m_t},
    from the fp64 recurrence of n~ and m (oracle/mlstm.py) on the case's inputs."""
    q, k = case["q"].double(), case["k"].double()
    ig, fg = case["igate"].double(), case["fgate"].double()
    B, NH, T, DQ = q.shape
    n = case["n0"].double() if "n0" in case else torch.zeros(B, NH, DQ, dtype=torch.float64)
    m = case["m0"].double().reshape(B, NH) if "m0" in case else torch.zeros(B, NH, dtype=torch.float64)
    hit = 0
    for t in range(T):
        lf = torch.nn.functional.logsigmoid(fg[..., t])
        mn = torch.maximum(lf + m, ig[..., t])
        n = torch.exp(lf + m - mn)[..., None] * n + torch.exp(ig[..., t] - mn)[..., None] * k[..., t, :]
        hit += int(((q[..., t, :] * DQ ** -0.5 * n).sum(-1).abs() < torch.exp(-mn)).sum())
        m = mn
    return hit / (B * NH * T)


def gate_grads_from_pairs(case, dq, dk, dcT=None, cT=None, dnT=None, nT=None):
    """The gate gradients as the kernels' host side forms them, from dq / dk:
    d igate_s = k_s.dk_s;  d fgate_t = sigmoid(-f_t) sum_{r >= t} (q_r.dq_r - k_r.dk_r), with
    <dC_T, C~_T> + <dn_T, n~_T> added at r = T - 1 when the final state carries a gradient (it
    depends on F_T with no query partner)."""
    q, k, fg = case["q"].double(), case["k"].double(), case["fgate"].double()
    kdk = (k * dk).sum(-1)
    dF = (q * dq).sum(-1) - kdk
    if dcT is not None:
        dF[..., -1] += (dcT * cT).flatten(2).sum(-1)
    if dnT is not None:
        dF[..., -1] += (dnT * nT).sum(-1)
    return kdk, torch.sigmoid(-fg) * dF.flip(-1).cumsum(-1).flip(-1)
