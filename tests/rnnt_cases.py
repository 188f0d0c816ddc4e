"""Inputs, the fp64 reference and the elementwise checker of the RNN-T loss parity tests (test
infrastructure, no GPU needed).

Reference.  oracle.rnnt.rnnt_single in fp64 on the values the kernel sees (16-bit inputs are
rounded first).  Its log-prob gradient at the blank and label columns are the arc occupancies
gb[t,u], gy[t,u] (<= 0, the gradient of nll); they, the row softmax sm and the upstream weight
s_b = d loss / d nll_b are kept separate, so the expected gradient is

    log-prob input   s_b gb at the blank column, s_b gy at the label column, 0 elsewhere;
    logits input     s_b (gb [v = blank] + gy [v = label] - sm[v] (gb + gy)).

Rule.  Sequence b has nd = Tb + Ub diagonals.  An occupancy is exp2 of a sum of ~nd rounded
terms, so its RELATIVE error grows with nd; a tolerance relative to the tensor's largest element
checks only the dominant paths, while occupancies span hundreds of binary orders.

    nll              rtol 1e-5 (the project's number); +inf where the oracle is +inf
    log-prob input   every column other than blank and label, every padding row (t >= Tb or
                     u > Ub) and every row of a sequence with s_b = 0: exactly 0.
                     At the two columns  |got - ref| <= |ref| (C nd mag_b + r) + a
    logits input     |got - ref| <= (C nd mag_b + C_sm mag_b + r) env[v] + a,
                     env[v] = |s_b| (sm[v] (|gb| + |gy|) + |gb| [v = blank] + |gy| [v = label]):
                     the cancelling sum replaced by its absolute terms
    r, a             storage rounding and underflow of the gradient dtype: RTOL as in
                     tests/scan_cases.py; a = 2^-126 for fp32 and bf16 (their smallest normal: at
                     sharp logits sm[v] (gb + gy) ~ 1e-17 x 1e-28 lies below it and is flushed or
                     loses its bits whatever the kernel does), 2^-24 for f16
    tiny arcs        an arc whose fp64 occupancy is below 2^-100 need only satisfy
                     |got| <= 2^-99 |s_b| (fp32 exp2 flushes there): the arc's reference becomes 0
                     and its elements get that allowance (times sm[v] + [v = column] for logits).
                     A floor on single elements, not a share of cases; nothing else is skipped.
    mag_b            max(1, largest finite |log-prob| of the sequence's arcs in nats, largest
                     |row log-sum-exp| when fed logits).  Derivation: the kernels keep every
                     emission and normaliser in fp32, so one arc's log-prob is known to
                     2^-24 |value| absolutely, and that absolute error of the exponent is the
                     relative error of the occupancy, and of the softmax exp(x - lse) in the
                     row stage.  At nominal logits mag ~ 10, at logits x100 ~ 600; without the
                     term both constants would be set by the sharp cases alone and be ~50 times
                     too loose for every other case.

C and C_sm are measured, never tuned on kernel output: restate_fp32 below (an fp32 numpy
restatement of the documented algorithm of csrc/rnnt.hip: base-2 logs, the exact emission shift
cb[t] / cy[u], re-centring on the diagonal maximum into an fp64 offset every 2K diagonals, K from
ab_halo_k) against the fp64 oracle in this metric over cpu_cases():

    C      whole restatement, the row term not granted: worst 6.02e-8 (halo, Umax = 895;
           0 .. 6e-8 everywhere, the sharp cases 1e-8 .. 3.6e-8);  C = 4 x 6.02e-8 = 2.41e-7
    C_sm   row stage alone, fed the fp64 occupancies: worst 4.26e-8 (logits x8, (40, 12));
                                                                C_sm = 4 x 4.26e-8 = 1.70e-7

The factor 4 is the margin tests/scan_cases.py took for the hardware exp2 / log2 / rcp
approximations (1 ulp each) and another summation order (the kernel's wave reductions).
tests/test_rnnt_checker.py asserts both measurements.

Case map (K = diagonals between halo exchanges, waves = ceil((Umax + 1) / (64 - K)), nvec = 16-byte
vectors per lane of the row kernels, 0 = scalar loop), from ab_halo_k / set_vec in csrc/rnnt.hip:

    halo   V = 4, T = 40   Umax  46  47  48  95  96 767 768 895 896 959 960 991 992 1007
                           K     16  16  16  16  16  16   8   8   4   4   2   2   1    1
                           waves  1   1   2   2   3  16  14  16  15  16  16  16  16   16
    diag   Umax = 3        nd 5 (ragged 1, 2), 15 .. 65 (ragged nd - 1, nd - 2): K = 16, one
                           wave; nd crosses the 16-diagonal pipeline blocks and the 32-diagonal
                           re-centring
    u0 / t1                U = 0 (T 1 .. 33), T = 1 (U 15 .. 32): K = 16, one wave
    rows   T = 5, U = 3    f32  V 256 512 768 1024 -> nvec 1 2 3 4; V 64 260 1280 -> 0
                           16b  V 512 1536 2048 -> nvec 1 3 4; V 520 -> 0
                           V = 256 one element off alignment -> 0; V = 512 compact -> nvec 2
    sharp / masked / dtype (T, U) = (40, 12) one wave, (130, 70) two waves, K = 16, nvec 0
"""
import numpy as np
import torch

from oracle import rnnt as ornnt

C = 2.41e-7
C_SM = 1.70e-7
NLL_RTOL = 1e-5
RTOL = {"f32": 1e-6, "bf16": 2.0 ** -8, "f16": 2.0 ** -10}
# the smallest normal of fp32 / bf16 (a product such as sm[v] (gb + gy) below it is flushed or
# loses its bits whatever the kernel does), the subnormal spacing of f16
ATOL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -24}
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TINY = 2.0 ** -100
TINY_BOUND = 2.0 ** -99


# ---- the kernels' launch rules, restated (csrc/rnnt.hip: ab_halo_k, launch_ab, set_vec) -------
def ab_halo_k(umax):
    for k in (16, 8, 4, 2, 1):
        if -(-(umax + 1) // (64 - k)) <= 16:
            return k
    return 0


def ab_waves(umax):
    k = ab_halo_k(umax)
    return -(-(umax + 1) // (64 - k))


def row_nvec(V, dtype, aligned=True):
    n = 16 // (4 if dtype == "f32" else 2)
    return V // (64 * n) if aligned and V % (64 * n) == 0 and V // (64 * n) <= 4 else 0


# ---- inputs ------------------------------------------------------------------------------------
def _round(x, dtype):
    return torch.as_tensor(np.asarray(x, np.float32)).to(TORCH_DTYPE[dtype]).float().numpy()


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def draw_labels(rng, shape, V, blank):
    y = rng.integers(0, V - 1, shape)
    return y + (y >= blank)


def make_case(key, T, U, V, fl, ll, w, dtype="f32", logits=True, blank=0, gain=1.5, seed=0,
              labels=None, grad_dtype=None, compact=False, misaligned=False):
    """x [B,T,U+1,V] fp32 holding values of `dtype` (logits, or fp64-normalised log-probs rounded
    once), labels [B,max(U,1)] avoiding the blank, lengths, upstream weights w [B]."""
    B = len(fl)
    rng = np.random.default_rng(seed)
    x = gain * rng.standard_normal((B, T, U + 1, V))
    if not logits:
        x = log_softmax64(x)
    y = draw_labels(rng, (B, max(U, 1)), V, blank) if labels is None else np.asarray(labels)
    return {"key": key, "dtype": dtype, "grad_dtype": grad_dtype or dtype, "logits": logits,
            "blank": blank, "x": _round(x, dtype), "labels": y.astype(np.int64),
            "fl": np.asarray(fl, np.int64), "ll": np.asarray(ll, np.int64),
            "w": np.asarray(w, np.float32), "compact": compact, "misaligned": misaligned}


# ---- fp64 reference ----------------------------------------------------------------------------
_REF = {}


def reference(case):
    """{"nll" [B], "gb", "gy" [B,T,U1] (0 outside the lattice), "sm" [B,T,U1,V] (logits only),
    "mag" [B], "nd" [B]}; computed once per case and shared, callers leave it unchanged."""
    key = case["key"]
    if key is not None and key in _REF:
        return _REF[key]
    x = case["x"].astype(np.float64)
    B, T, U1, V = x.shape
    lp = log_softmax64(x) if case["logits"] else x
    ref = {"nll": np.zeros(B), "gb": np.zeros((B, T, U1)), "gy": np.zeros((B, T, U1)),
           "mag": np.ones(B), "nd": case["fl"] + case["ll"]}
    if case["logits"]:
        ref["sm"] = np.exp(lp)
    for b in range(B):
        Tb, Ub = int(case["fl"][b]), int(case["ll"][b])
        if Tb == 0:
            ref["nll"][b] = np.inf
            continue
        y = case["labels"][b, :Ub]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            nll, g = ornnt.rnnt_single(lp[b, :Tb, :Ub + 1], y, case["blank"])
        ref["nll"][b] = nll
        arcs = [lp[b, :Tb, :Ub + 1, case["blank"]].ravel()]
        if Ub:
            arcs.append(lp[b, :Tb, np.arange(Ub), y].ravel())
        if case["logits"]:   # the row normaliser, from any unmasked column
            with np.errstate(invalid="ignore"):
                arcs.append(np.nanmax(x[b, :Tb, :Ub + 1] - lp[b, :Tb, :Ub + 1], -1).ravel())
        arcs = np.concatenate(arcs)
        arcs = np.abs(arcs[np.isfinite(arcs)])
        ref["mag"][b] = max(1.0, arcs.max() if arcs.size else 0.0)
        if not np.isfinite(nll):
            continue   # no alignment: the loss is +inf and carries no gradient
        ref["gb"][b, :Tb, :Ub + 1] = g[:, :, case["blank"]]
        if Ub:
            ref["gy"][b, :Tb, :Ub] = g[:, np.arange(Ub), y]
    if key is not None:
        _REF[key] = ref
    return ref


def label_index(case):
    """[B,U1] label column of node (., u); -1 where the node has no label arc."""
    B, U1 = case["x"].shape[0], case["x"].shape[2]
    idx = np.full((B, U1), -1, np.int64)
    for b in range(B):
        Ub = int(case["ll"][b])
        idx[b, :Ub] = case["labels"][b, :Ub]
    return idx


def assemble(case, gb, gy, sm=None, lab=None):
    """The gradient tensor [B,T,U1,V] (fp64) of sum_b w_b nll_b from arc occupancies, the row
    softmax (logits input) and the label columns."""
    B, T, U1, V = case["x"].shape
    lab = label_index(case) if lab is None else lab
    s = case["w"].astype(np.float64)[:, None, None]
    g = np.zeros((B, T, U1, V))
    if case["logits"]:
        sm = np.zeros_like(g) if sm is None else sm
        g -= sm * (s * (gb + gy))[..., None]
    g[..., case["blank"]] += s * gb
    bi, ui = np.nonzero(lab >= 0)
    g[bi, :, ui, lab[bi, ui]] += (s * gy)[bi, :, ui]
    return g


def expected(case, ref=None):
    """(ref gradient with tiny arcs set to 0, tolerance parts) -- see the module docstring:
    pass iff |got - g0| <= fixed + c * unit_c + c_sm * unit_sm elementwise, and got == 0 where
    `zero` holds."""
    ref = reference(case) if ref is None else ref
    B, T, U1, V = case["x"].shape
    gd = case["grad_dtype"]
    s = np.abs(case["w"].astype(np.float64))[:, None, None]
    gb, gy = ref["gb"], ref["gy"]
    tb, ty = (np.abs(gb) < TINY) & (gb != 0), (np.abs(gy) < TINY) & (gy != 0)
    gb0, gy0 = np.where(tb, 0.0, gb), np.where(ty, 0.0, gy)
    sm = ref.get("sm")
    g0 = assemble(case, gb0, gy0, sm)
    one = dict(case, w=np.ones(B, np.float32))
    # assemble() with -sm adds the softmax term instead of subtracting it: the absolute form
    env = assemble(one, s * np.abs(gb0), s * np.abs(gy0), None if sm is None else -sm)
    floor = TINY_BOUND * assemble(one, s * tb, s * ty, None if sm is None else -sm)
    depth = (ref["nd"] * ref["mag"])[:, None, None, None]
    fixed = RTOL[gd] * env + np.where(env > 0, ATOL[gd], 0.0) + floor
    zero = (env == 0) & (floor == 0)
    mag = ref["mag"][:, None, None, None]
    return {"g0": g0, "fixed": fixed, "unit_c": depth * env,
            "unit_sm": mag * env if case["logits"] else np.zeros_like(env), "zero": zero}


def check(case, got, ref=None):
    """got: {"nll": [B], "grad": [B,T,U1,V]} (either may be absent).  Returns
    {"nll": worst error in units of its bound, "nonzero": elements that must be exactly 0 and are
    not, "grad": worst (|got - ref| - fixed) / (C unit_c + C_sm unit_sm)}; pass iff nll <= 1,
    nonzero == 0, grad <= 1."""
    ref = reference(case) if ref is None else ref
    m = {}
    if "nll" in got:
        g = np.asarray(got["nll"], np.float64)
        r = ref["nll"]
        fin = np.isfinite(r)
        bad = (~fin & ~(np.isposinf(g))) | (fin & ~np.isfinite(g))
        with np.errstate(invalid="ignore"):
            e = np.where(fin, np.abs(g - r) / (NLL_RTOL * np.abs(r)), 0.0)
        m["nll"] = float(np.where(bad, np.inf, e).max()) if g.size else 0.0
    if "grad" in got:
        g = np.asarray(got["grad"], np.float64)
        ex = expected(case, ref)
        m["nonzero"] = int((ex["zero"] & ~(g == 0)).sum())
        err = np.where(np.isfinite(g), np.abs(g - ex["g0"]), np.inf)
        excess = np.maximum(err - ex["fixed"], 0.0)
        unit = C * ex["unit_c"] + C_SM * ex["unit_sm"]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(ex["zero"] | (excess == 0), 0.0, excess / unit)
        m["grad"] = float(q.max()) if q.size else 0.0
    return m


def failures(m):
    return {k: v for k, v in m.items() if not (v == 0 if k == "nonzero" else v <= 1.0)}


def assert_parity(case, got, label=""):
    m = check(case, got)
    print(f"rnnt parity {label or case['key']}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
    bad = failures(m)
    assert not bad, f"{label or case['key']}: {bad} (nll, grad: over 1; nonzero: must be 0)"
    return m


def measure(case, got, ref=None):
    """The c at which the worst element of got["grad"] would just pass with c_sm = 0 (per unit of
    nd mag env): what C is measured with on log-prob cases, and, with the arcs taken exact, the
    c_sm (per unit of env) on logits cases."""
    ref = reference(case) if ref is None else ref
    ex = expected(case, ref)
    g = np.asarray(got["grad"], np.float64)
    excess = np.maximum(np.abs(g - ex["g0"]) - ex["fixed"], 0.0)
    out = {}
    for name in ("unit_c", "unit_sm"):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(excess > 0, excess / ex[name], 0.0)
        out[name] = float(q.max()) if q.size else 0.0
    return out


# ---- the documented algorithm in fp32 numpy (what C and C_sm are measured with) ----------------
F32 = np.float32
DEAD = F32(-1e30)
LOG2E = F32(1.4426950408889634)
LN2 = 0.6931471805599453


def _lse2(x, y):
    m = np.maximum(x, y)
    return m + np.log2(np.exp2(x - m) + np.exp2(y - m))


def _restate_lattice(lb, ly, K):
    """lb, ly fp32 [Tb,U1] base-2 emissions (dead = -1e30; ly[:, Ub] dead) -> (nll, gb, gy): the
    emission shift, the two diagonal sweeps re-centred every 2K diagonals into an fp64 offset,
    the occupancies recombined in fp64 and one fp32 exp2 each."""
    Tb, U1 = lb.shape
    Ub, nd = U1 - 1, Tb + U1 - 1
    live_b, live_y = lb > -1e29, ly > -1e29
    cb = np.where(live_b.any(1), np.where(live_b, lb, DEAD).max(1), F32(0))
    cy = np.where(live_y.any(0), np.where(live_y, ly, DEAD).max(0), F32(0))
    lb = np.where(live_b, np.maximum(lb - cb[:, None], DEAD), lb).astype(F32)
    ly = np.where(live_y, np.maximum(ly - cy[None, :], DEAD), ly).astype(F32)
    ctot = cb.astype(np.float64).sum() + cy.astype(np.float64).sum()
    u = np.arange(U1)
    dead = np.full(1, DEAD, F32)
    out = []
    for beta in (False, True):
        tab = np.full((Tb, U1), -np.inf)
        v = np.full(U1, DEAD, F32)
        off = 0.0
        for i in range(nd):
            n = nd - 1 - i if beta else i
            t = n - u
            valid = (t >= 0) & (t < Tb)
            tc = np.clip(t, 0, Tb - 1)
            if not beta:
                vn = np.concatenate([dead, v[:-1]])
                if i == 0:
                    nv = np.where(u == 0, F32(0), DEAD)
                else:
                    nv = _lse2(np.where(t >= 1, v + lb[np.clip(t - 1, 0, Tb - 1), u], DEAD),
                               np.where(u >= 1, vn + ly[tc, np.maximum(u - 1, 0)], DEAD))
            else:
                vn = np.concatenate([v[1:], dead])
                if i == 0:
                    nv = np.where(u == Ub, lb[tc, u], DEAD)
                else:
                    nv = _lse2(np.where(t + 1 < Tb, v + lb[tc, u], DEAD),
                               np.where(u < Ub, vn + ly[tc, u], DEAD))
            v = np.where(valid, np.maximum(nv, DEAD), DEAD).astype(F32)
            if i % (2 * K) == 2 * K - 1:
                m = v.max()
                if m > 0.5 * DEAD:
                    v = (v - m).astype(F32)
                    off += float(m)
            tab[t[valid], u[valid]] = v[valid].astype(np.float64) + off
        out.append((tab, v, off))
    (al, va, offa), (be, _, _) = out
    gb, gy = np.zeros((Tb, U1)), np.zeros((Tb, U1))
    if not (va[Ub] > 0.5 * DEAD and lb[Tb - 1, Ub] > 0.5 * DEAD):
        return np.inf, gb, gy
    lp2 = float(va[Ub]) + float(lb[Tb - 1, Ub]) + offa
    with np.errstate(over="ignore", invalid="ignore"):
        gb[:-1] = -np.exp2((al[:-1] + lb[:-1] + be[1:] - lp2).astype(F32))
        gb[-1, Ub] = -np.exp2(F32(al[-1, Ub] + lb[-1, Ub] - lp2))
        gy[:, :-1] = -np.exp2((al[:, :-1] + ly[:, :-1] + be[:, 1:] - lp2).astype(F32))
    return float(F32(-(lp2 + ctot) * LN2)), gb, gy


def restate_fp32(case, exact_arcs=False):
    """{"nll", "grad"} of the fp32 restatement.  exact_arcs: the occupancies come from the fp64
    reference (rounded to fp32), so only the row stage's error is left (C_sm)."""
    x = case["x"].astype(F32)
    B, T, U1, V = x.shape
    K = ab_halo_k(U1 - 1)
    lab = label_index(case)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if case["logits"]:
            m = x.max(-1, keepdims=True)
            lse = (m + np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=F32))).astype(F32)
        else:
            lse = np.zeros((B, T, U1, 1), F32)
        lpall = np.maximum((x - lse) * LOG2E, DEAD)
    nll = np.zeros(B)
    gb, gy = np.zeros((B, T, U1), F32), np.zeros((B, T, U1), F32)
    ref = reference(case) if exact_arcs else None
    for b in range(B):
        Tb, Ub = int(case["fl"][b]), int(case["ll"][b])
        if Tb == 0:
            nll[b] = np.inf
            continue
        if exact_arcs:
            gb[b], gy[b] = ref["gb"][b], ref["gy"][b]
            continue
        lb = np.where(np.isnan(lpall[b, :Tb, :Ub + 1, case["blank"]]), DEAD,
                      lpall[b, :Tb, :Ub + 1, case["blank"]]).astype(F32)
        ly = np.full((Tb, Ub + 1), DEAD, F32)
        if Ub:
            ly[:, :Ub] = lpall[b, :Tb, np.arange(Ub), lab[b, :Ub]].T
        nll[b], gbb, gyb = _restate_lattice(lb, ly, K)
        gb[b, :Tb, :Ub + 1], gy[b, :Tb, :Ub + 1] = gbb, gyb
    s = case["w"].astype(F32)[:, None, None]
    gb, gy = (gb * s).astype(F32), (gy * s).astype(F32)
    g = np.zeros((B, T, U1, V), F32)
    if case["logits"]:
        with np.errstate(invalid="ignore", over="ignore"):
            g = (-np.exp(x - lse) * (gb + gy)[..., None]).astype(F32)
        for b in range(B):
            g[b, int(case["fl"][b]):] = 0
            g[b, :, int(case["ll"][b]) + 1:] = 0
    g[..., case["blank"]] += gb
    bi, ui = np.nonzero(lab >= 0)
    g[bi, :, ui, lab[bi, ui]] += gy[bi, :, ui]
    return {"nll": nll, "grad": _round(g, case["grad_dtype"])}


# ---- the case list: C is measured over it (test_rnnt_checker), the GPU tests run it ------------
HALO_UMAX = (46, 47, 48, 95, 96, 767, 768, 895, 896, 959, 960, 991, 992, 1007)
DIAG_ND = (5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)     # 1 and 2: ragged rows of nd = 5
U0_T = (1, 16, 17, 32, 33)
T1_U = (15, 16, 31, 32)
W3 = (1.0, -0.5, 1e3)
ROW_V = {"f32": (256, 512, 768, 1024, 64, 260, 1280), "bf16": (512, 1536, 2048, 520),
         "f16": (512, 1536, 2048, 520)}
SHARP = [(g, T, U) for g in (8, 30, 100) for (T, U) in ((40, 12), (130, 70))]
MASKS = ("unused", "some", "final_blank", "label_column")


def halo_case(umax):
    """V = 4, T = 40; the second sequence ends one label short of the last wave seam below Umax
    (64 - K owned label positions per wave)."""
    ow = 64 - ab_halo_k(umax)
    seam = (umax // ow) * ow
    u1 = seam - 1 if seam > 0 and seam - 1 < umax else umax - 1
    return make_case(("halo", umax), 40, umax, 4, [40, 37], [umax, u1], [1.0, -0.5],
                     logits=umax % 2 == 0, seed=1000 + umax)


def diag_case(nd):
    """Umax = 3; Tb + Ub = nd for sequence 0, nd - 1 and nd - 2 for the ragged ones (nd = 5:
    1 and 2 instead); the zero weight of nd = 33 gives an exactly zero row."""
    T = nd - 3
    fl, ll = ([T, 1, 1], [3, 0, 1]) if nd == 5 else ([T, T - 1, T], [3, 3, 1])
    w = (1.0, 0.0, 1e3) if nd == 33 else W3
    return make_case(("diag", nd), T, 3, 6, fl, ll, w, logits=nd % 2 == 1, seed=2000 + nd)


def u0_case(T):
    return make_case(("u0", T), T, 0, 5, [T, max(1, T - 1)], [0, 0], [1.0, -0.5], seed=3000 + T,
                     logits=T % 2 == 1)


def t1_case(U):
    return make_case(("t1", U), 1, U, 5, [1, 1], [U, U - 1], [1.0, -0.5], seed=3100 + U,
                     logits=U % 2 == 1)


def row_blanks(V):
    return [b for b in (0, 77, V - 1) if b < V]


def row_case(dtype, V, blank, logits, compact=False, misaligned=False):
    """B = 2, T = 5, U = 3; sequence 0's labels sit in the first column, the last column and
    mid-vector (next to the blank where they would collide)."""
    first = 0 if blank != 0 else 1
    last = V - 1 if blank != V - 1 else V - 2
    mid = V // 2 + 1 if blank != V // 2 + 1 else V // 2 + 2
    rng = np.random.default_rng(V + blank)
    labels = np.stack([[first, last, mid], draw_labels(rng, 3, V, blank)])
    return make_case(("row", dtype, V, blank, logits, compact, misaligned), 5, 3, V, [5, 4],
                     [3, 2], [1.0, -0.5], dtype=dtype, logits=logits, blank=blank, labels=labels,
                     seed=4000 + V + blank, compact=compact, misaligned=misaligned)


def row_cases():
    for dtype, vs in ROW_V.items():
        for V in vs:
            for blank in row_blanks(V):
                yield row_case(dtype, V, blank, True)
            yield row_case(dtype, V, V - 1, False)
    yield row_case("f32", 256, 77, True, misaligned=True)
    yield row_case("f32", 256, 77, False, misaligned=True)
    yield row_case("f32", 512, 77, True, compact=True)
    yield row_case("bf16", 512, 511, True, compact=True)


def dtype_case(dtype):
    return make_case(("dtype", dtype), 40, 12, 16, [40, 33, 40], [12, 12, 7], W3, dtype=dtype,
                     seed=5000)


def gradtype_case(dtype, V):
    """16-bit logits with an fp32 gradient (the C ABI's grad_dtype)."""
    return make_case(("grad32", dtype, V), 5, 3, V, [5, 4], [3, 2], [1.0, -0.5], dtype=dtype,
                     grad_dtype="f32", blank=V - 1, seed=5100 + V)


def sharp_case(gain, T, U):
    return make_case(("sharp", gain, T, U), T, U, 16, [T, T - 7], [U, U - 5], [1.0, -0.5],
                     gain=float(gain), seed=6000 + gain + T)


def masked_case(kind, logits):
    """(T, U) = (40, 12), V = 8, B = 3: -inf log-probs (or logits).  `unused`: a column no arc
    uses; `some`: single arcs, paths left; `final_blank` / `label_column`: every path of
    sequence 1 blocked (its nll is +inf, its gradient exactly zero, the neighbours untouched)."""
    T, U, V = 40, 12, 8
    c = make_case(("masked", kind, logits), T, U, V, [T, 33, T], [U, 9, U], W3, logits=logits,
                  labels=draw_labels(np.random.default_rng(7), (3, U), V - 1, 0), seed=7000)
    x = c["x"]
    if kind == "unused":
        x[..., V - 1] = -np.inf                 # labels are drawn from 1 .. V-2
    elif kind == "some":
        x[:, 5, 3, 0] = -np.inf
        x[:, 20, 6, 0] = -np.inf
        for b in range(3):
            x[b, 11, 4, c["labels"][b, 4]] = -np.inf
            x[b, 30:, 8, c["labels"][b, 8]] = -np.inf
    elif kind == "final_blank":
        x[1, 32, 9, 0] = -np.inf
    elif kind == "label_column":
        x[1, :, 5, c["labels"][1, 5]] = -np.inf
    return c


def mid_case():
    """The determinism case."""
    return make_case(("mid",), 130, 70, 17, [130, 101], [70, 44], [1.0, -0.5], seed=8000)


def cpu_cases():
    for umax in HALO_UMAX:
        yield halo_case(umax)
    for nd in DIAG_ND:
        yield diag_case(nd)
    for T in U0_T:
        yield u0_case(T)
    for U in T1_U:
        yield t1_case(U)
    yield from row_cases()
    for dtype in ("f32", "bf16", "f16"):
        yield dtype_case(dtype)
    for dtype in ("bf16", "f16"):
        for V in (512, 24):
            yield gradtype_case(dtype, V)
    for g, T, U in SHARP:
        yield sharp_case(g, T, U)
    for kind in MASKS:
        for logits in (False, True):
            yield masked_case(kind, logits)
    yield mid_case()
