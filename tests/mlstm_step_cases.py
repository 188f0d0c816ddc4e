"""Inputs, the fp64 side and the checker of the recurrent mLSTM step tests (test infrastructure,
no GPU needed; shared by tests/test_mlstm_step_checker.py and tests/test_gpu_mlstm_step.py).

Inputs: q, k, v ~ N(0,1) (rounded to the operand dtype: both sides see the rounded values),
igate = cap15(8 N(0,1)), fgate = cap15(8 N(0,1) + 3) with cap15(x) = 15 tanh(x / 15), carried
states C0, n0 ~ N(0,1), m0 ~ U(-20, 20).  With B = 2..3, NH = 2 and K >= 8 both branches of the
normaliser max(|q~.n|, e^{-m}) occur in the fp64 oracle at every head size; case_set() asserts it.

The reference is oracle.mlstm.mlstm_recurrent (fp64).  A ``live`` mask is applied by compacting
each batch row's live steps, running the oracle on them and scattering the rows back (a held
step returns a zero row and leaves the state alone).
"""
import numpy as np
import torch

from oracle.mlstm import _logsig, mlstm_recurrent

HEADS = ((32, 64), (64, 64), (64, 128), (96, 192))
U32 = 2.0 ** -24    # unit roundoff of fp32
U_BF16 = 2.0 ** -8  # unit roundoff of bf16 (8 significant bits)


def cap15(x):
    return 15.0 * torch.tanh(x / 15.0)


def draw_case(B, NH, K, DQ, DV, carried, seed, dtype=torch.float32, live=None):
    """One case as fp32 / ``dtype`` CPU tensors from one seeded generator.  live: optional
    [B, K] 0/1 array."""
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g)
    c = {"key": (B, NH, K, DQ, DV, carried, seed, dtype,
                 None if live is None else tuple(map(tuple, np.asarray(live).tolist()))),
         "dims": (B, NH, K, DQ, DV), "dtype": dtype}
    c["q"], c["k"] = rn(B, NH, K, DQ).to(dtype), rn(B, NH, K, DQ).to(dtype)
    c["v"] = rn(B, NH, K, DV).to(dtype)
    # raw pre-activations as a projection in ``dtype`` holds them, and their soft cap (fp64,
    # rounded once to fp32): the gates the oracle and a kernel fed capped gates see
    c["iraw"], c["fraw"] = (8 * rn(B, NH, K)).to(dtype), (8 * rn(B, NH, K) + 3).to(dtype)
    c["igate"], c["fgate"] = cap15(c["iraw"].double()).float(), cap15(c["fraw"].double()).float()
    if carried:
        c["c0"], c["n0"] = rn(B, NH, DQ, DV), rn(B, NH, DQ)
        c["m0"] = 40 * torch.rand(B, NH, 1, generator=g) - 20
    else:
        c["c0"], c["n0"] = torch.zeros(B, NH, DQ, DV), torch.zeros(B, NH, DQ)
        c["m0"] = torch.zeros(B, NH, 1)
    c["live"] = None if live is None else np.asarray(live, np.float32).reshape(B, K)
    return c


def _np64(t):
    return t.detach().double().cpu().numpy()


def _scales(q, k, v, ig, fg, C, n, m, eps):
    """The recurrence of oracle/mlstm.py for one batch row in fp64 [NH, T, ...], with the
    quantities the checker scales by: the running absolute sums
        SC_t = fa SC_{t-1} + ia |k v^T|,  Sn_t = fa Sn_{t-1} + ia |k|   (SC_0 = |C_0|, Sn_0 = |n_0|)
    A_tj = sum_i |q~_i| SC_ij, Nn_t = sum_i |q~_i| Sn_i, den_t, the per-step weight w_t of
    check_step's c(t), the stabiliser trajectory and which branch the normaliser took."""
    NH, T, DQ = q.shape
    DV = v.shape[-1]
    s = DQ ** -0.5
    SC, Sn = np.abs(C), np.abs(n)
    out = {k_: np.zeros((NH, T)) for k_ in ("Nn", "den", "w", "wcap", "m", "floor", "mag")}
    out["A"], out["h"] = np.zeros((NH, T, DV)), np.zeros((NH, T, DV))
    for t in range(T):
        lf = _logsig(fg[:, t])
        a = lf + m
        mn = np.maximum(a, ig[:, t])
        fa, ia = np.exp(a - mn)[:, None], np.exp(ig[:, t] - mn)[:, None]
        kv = k[:, t, :, None] * v[:, t, None, :]
        C = fa[..., None] * C + ia[..., None] * kv
        n = fa * n + ia * k[:, t]
        SC = fa[..., None] * SC + ia[..., None] * np.abs(kv)
        Sn = fa * Sn + ia * np.abs(k[:, t])
        qs = q[:, t] * s
        qn = np.abs((qs * n).sum(-1))
        den = np.maximum(qn, np.exp(-mn)) + eps
        out["h"][:, t] = np.einsum("hi,hij->hj", qs, C) / den[:, None]
        out["A"][:, t] = np.einsum("hi,hij->hj", np.abs(qs), SC)
        out["Nn"][:, t] = (np.abs(qs) * Sn).sum(-1)
        out["den"][:, t] = den
        out["floor"][:, t] = qn < np.exp(-mn)
        out["w"][:, t] = 8 + 2 * np.abs(a) + 2 * np.abs(lf) + np.abs(a - mn) + np.abs(ig[:, t] - mn)
        out["m"][:, t] = mn
        out["wcap"][:, t] = 5 * (np.abs(ig[:, t]) + np.abs(fg[:, t]))
        out["mag"][:, t] = np.maximum.reduce([np.abs(a), np.abs(mn), np.abs(ig[:, t]),
                                              np.ones_like(mn)])
        m = mn
    out.update(C=C, n=n, mT=m, SC=SC, Sn=Sn)
    return out


_REF = {}


def reference(case, eps=1e-6):
    """The fp64 oracle on the case and the checker's scales.  {"h" [B,NH,K,DV], "C", "n", "m"
    [B,NH] final state, "SC", "Sn", "unit" (u of check_step, per h element), "c" (c(t) per
    (b, head, step)), "cstate" / "mtol" (per (b, head)), "floor" (1 where the normaliser took
    e^{-m}, nan on held steps)}.  Computed once per case and shared; callers leave it unchanged."""
    if case["key"] in _REF:
        return _REF[case["key"]]
    B, NH, K, DQ, DV = case["dims"]
    q, k, v = _np64(case["q"]), _np64(case["k"]), _np64(case["v"])
    ig, fg = _np64(case["igate"]), _np64(case["fgate"])
    c0, n0, m0 = _np64(case["c0"]), _np64(case["n0"]), _np64(case["m0"]).reshape(B, NH)
    live = np.ones((B, K)) if case["live"] is None else case["live"]
    r = {"h": np.zeros((B, NH, K, DV)), "unit": np.zeros((B, NH, K, DV)),
         "c": np.zeros((B, NH, K)), "ccap": np.zeros((B, NH, K)), "ccap_state": np.zeros((B, NH)),
         "mtol_cap": np.zeros((B, NH)), "floor": np.full((B, NH, K), np.nan),
         "C": c0.copy(), "n": n0.copy(), "m": m0.copy(), "SC": np.abs(c0), "Sn": np.abs(n0),
         "cstate": np.full((B, NH), 4.0), "mtol": np.zeros((B, NH))}
    for b in range(B):
        idx = np.nonzero(live[b])[0]
        if idx.size == 0:
            continue
        sub = [x[b][:, idx] for x in (q, k, v, ig, fg)]
        h, (C, n, m) = mlstm_recurrent(*[x[None] for x in sub], c0[b:b + 1], n0[b:b + 1],
                                       m0[b:b + 1], eps)
        s = _scales(*sub, c0[b], n0[b], m0[b], eps)
        np.testing.assert_allclose(s["h"], h[0], rtol=1e-11, atol=1e-300)   # the same recurrence
        np.testing.assert_allclose(s["C"], C[0], rtol=1e-11, atol=1e-300)
        G = np.cumsum(s["w"], -1)
        r["h"][b][:, idx] = h[0]
        r["unit"][b][:, idx] = U32 * (s["A"] + np.abs(h[0]) * s["Nn"][..., None]) / s["den"][..., None]
        r["c"][b][:, idx] = DQ + 8 + G + 2 * (2 + np.abs(s["m"]))
        r["floor"][b][:, idx] = s["floor"]
        r["C"][b], r["n"][b], r["m"][b] = C[0], n[0], m[0, :, 0]
        r["SC"][b], r["Sn"][b] = s["SC"], s["Sn"]
        r["cstate"][b] = 4 + G[:, -1]
        Gc = np.cumsum(s["wcap"], -1)
        r["ccap"][b][:, idx], r["ccap_state"][b] = Gc, Gc[:, -1]
        r["mtol_cap"][b] = U32 * Gc[:, -1]
        r["mtol"][b] = (3 * idx.size + 1) * U32 * np.maximum(s["mag"].max(-1), np.abs(m0[b]))
    _REF[case["key"]] = r
    return r


def check_step(case, h, C, n, m, out_unit=0.0, cap_in_kernel=False, what=""):
    """Compare one run of the step (h [B,NH,K,DV] and the state after it) element by element
    against the fp64 oracle at the scale of its own step.  Returns the largest error seen as a
    fraction of the allowance (h, C, n, m), so a caller can assert headroom.

    Error model (fp32, unit roundoff u = 2^-24; none of it fitted to a kernel).
    * C_t,ij is a sum of at most t + 1 terms e^{..} k_i v_j.  A term that has lived through the
      steps s..t has been multiplied by one gate factor per step, and each step adds one rounded
      multiply-add (2u).  A gate factor is e^x with x = (logsig(f) + m_{s-1}) - m_s or i_s - m_s
      formed in fp32: logsig carries ~2u |logsig f|, the sum a = logsig f + m_{s-1} carries u |a|,
      the difference u |x|, and e^x itself 2u, so a factor's relative error is at most
      u (2 + 2 |logsig f| + |a| + |x|); both factors of a step together stay below
      u w_s,  w_s = 8 + 2 |a_s| + 2 |logsig f_s| + |a_s - m_s| + |i_s - m_s|
      (the 8 holds the 2u multiply-add and the two exponentials).  First-order, every term of
      C_t is off by at most u G_t relative, G_t = sum_{s <= t} w_s over the LIVE steps, i.e. C_t by
      u G_t SC_t elementwise with SC the same recurrence on absolute values.  n_t alike with Sn.
      (The stabiliser itself may drift: h does not depend on its value as long as C~, n~ and the
      floor use the same one, so its rounding enters only through the factors above.)
    * The numerator sum_i q~_i C_ij is a length-DQ dot product of rounded q~ (u) with rounded
      products, accumulated in any order: (DQ + 1) u A_j more, A_j = sum_i |q~_i| SC_ij.  The
      normaliser's dot product alike with Nn = sum_i |q~_i| Sn_i; on the floor branch it is
      e^{-m_t} instead, off by u (2 + |m_t|) relative, and since |h| <= A / den that is at most
      u (2 + |m_t|) A_j / den in h.  The max, the + eps and the division add 3u.
    * Together |h - h_ref| <= c(t) u_j with the unit u_j = 2^-24 (A_j + |h_j| Nn) / den and
          c(t) = DQ + 8 + G_t + 2 (2 + |m_t|)  (>= DQ + t).
      An output rounded to ``out_unit`` (bf16: 2^-8) adds out_unit |h|.
    * State: C~, n~ are rescaled to the oracle's stabiliser (times e^{m_got - m_ref}, exact here)
      and compared to (4 + G_T) u SC_T / Sn_T.  m: every live step rounds one sum and one
      logsig, so |m - m_ref| <= (3 T_live + 1) u max(|a|, |m|, |i|, 1) over the trajectory.
    * cap_in_kernel: the kernel was given the RAW pre-activations and applied cap tanh(x / cap)
      itself in fp32 (a division, a tanh of ~2u, a multiplication: 4u |gate|), while the oracle
      sees the fp64 cap rounded once to fp32 (u |gate|).  The gates enter exponents, so that is a
      relative error of 5u (|i_s| + |f_s|) on the step's factors (|d logsig / df| <= 1): it is
      added to w_s, and its sum over the live steps to m's allowance.
    """
    r = reference(case)
    h, C, n, m = (np.asarray(x, np.float64) for x in (h, C, n, m))
    B, NH, K, DQ, DV = case["dims"]
    m = m.reshape(B, NH)
    worst = {}
    extra = float(bool(cap_in_kernel))
    tol = (r["c"] + extra * r["ccap"])[..., None] * r["unit"]
    tol = tol + out_unit * (np.abs(r["h"]) + tol)
    err = np.abs(h - r["h"])
    held = np.isnan(r["floor"])
    assert not np.any(h[held] != 0.0), f"{what}: a held step returned a non-zero row"
    frac = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    worst["h"] = float(frac.max()) if frac.size else 0.0
    assert np.isfinite(h).all() and worst["h"] <= 1.0, (
        f"{what}: h off by {worst['h']:.3g} x the allowance c(t) u at "
        f"{np.unravel_index(np.argmax(frac), frac.shape)} (c = {r['c'].max():.0f} units at most)")
    mtol = r["mtol"] + extra * r["mtol_cap"]
    merr = np.abs(m - r["m"])
    worst["m"] = float((merr / np.maximum(mtol, 1e-300)).max()) if np.any(mtol > 0) else 0.0
    assert np.all(merr <= mtol), f"{what}: m off by {merr.max():.3g} (allowed {mtol.max():.3g})"
    rescale = np.exp(m - r["m"])
    for name, got, ref, S in (("C", C * rescale[..., None, None], r["C"], r["SC"]),
                              ("n", n * rescale[..., None], r["n"], r["Sn"])):
        cs = (r["cstate"] + extra * r["ccap_state"]).reshape(B, NH, *([1] * (S.ndim - 2)))
        stol = cs * U32 * S
        serr = np.abs(got - ref)
        f = np.where(stol > 0, serr / np.where(stol > 0, stol, 1.0), np.where(serr > 0, np.inf, 0.0))
        worst[name] = float(f.max())
        assert np.isfinite(got).all() and worst[name] <= 1.0, (
            f"{what}: state {name} off by {worst[name]:.3g} x the allowance")
    return worst


def case_set(DQ, DV, dtype=torch.float32, Ks=(1, 3, 8, 64), B=2, NH=2):
    """The kernel cases of one head size: K in Ks x {zero, carried} state.  Asserts that over
    the set the fp64 oracle's normaliser takes BOTH branches (|q~.n| and the floor e^{-m}), so no
    run of the set can pass with one of them unexercised."""
    cases = [draw_case(B + (i % 2), NH, K, DQ, DV, carried, seed=100 * DQ + 10 * i + carried,
                       dtype=dtype)
             for i, K in enumerate(Ks) for carried in (0, 1)]
    hits = np.concatenate([reference(c)["floor"].ravel() for c in cases])
    assert 0 < np.nansum(hits) < np.sum(~np.isnan(hits)), (
        f"head ({DQ}, {DV}): the case set reaches only one branch of the normaliser")
    return cases


# ------------------------------------------------------------- fp32 restatement (numpy) ----
DEFECTS = ("scale", "nofloor", "sigmoid", "m_reset", "n_garbage", "mask_decay")


def numpy_step_fp32(case, defect=None, eps=1e-6):
    """The step recurrence restated in fp32 numpy: (h, C, n, m) as a kernel would return them.
    ``defect`` plants one of DEFECTS: s = 1/DQ; the e^{-m} floor dropped; sigmoid in place of
    logsigmoid; m not carried between steps; n updated with v in one column; a held step that
    still decays the state."""
    f = np.float32
    B, NH, K, DQ, DV = case["dims"]
    q, k, v = (case[x].float().numpy() for x in ("q", "k", "v"))
    ig, fg = case["igate"].numpy().astype(f), case["fgate"].numpy().astype(f)
    C, n = case["c0"].numpy().astype(f).copy(), case["n0"].numpy().astype(f).copy()
    m = case["m0"].numpy().astype(f).reshape(B, NH).copy()
    live = np.ones((B, K), f) if case["live"] is None else case["live"]
    s = f(1.0 / DQ) if defect == "scale" else f(DQ ** -0.5)
    h = np.zeros((B, NH, K, DV), f)
    for t in range(K):
        on = live[:, t] != 0
        x = fg[..., t]
        if defect == "sigmoid":
            lf = (f(1) / (f(1) + np.exp(-x))).astype(f)
        else:
            lf = (np.minimum(x, f(0)) - np.log1p(np.exp(-np.abs(x)))).astype(f)
        mp = np.zeros_like(m) if defect == "m_reset" else m
        a = lf + mp
        mn = np.maximum(a, ig[..., t])
        fa, ia = np.exp(a - mn).astype(f), np.exp(ig[..., t] - mn).astype(f)
        Cn = fa[..., None, None] * C + (ia[..., None] * k[..., t, :])[..., None] * v[..., t, None, :]
        nn = fa[..., None] * n + ia[..., None] * k[..., t, :]
        if defect == "n_garbage":
            nn[..., 0] = fa * n[..., 0] + ia * v[..., t, 0]
        qs = q[..., t, :] * s
        num = np.einsum("bhi,bhij->bhj", qs, Cn).astype(f)
        qn = np.abs((qs * nn).sum(-1))
        den = (qn if defect == "nofloor" else np.maximum(qn, np.exp(-mn))) + f(eps)
        ht = (num / den[..., None]).astype(f)
        for b in range(B):
            if on[b]:
                C[b], n[b], m[b], h[b, :, t] = Cn[b], nn[b], mn[b], ht[b]
            elif defect == "mask_decay":
                C[b], n[b] = fa[b, :, None, None] * C[b], fa[b, :, None] * n[b]
    return h, C, n, m
