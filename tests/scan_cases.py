"""Inputs, fp64 references and the elementwise checker of the LucyRNN scan parity tests (test
infrastructure, no GPU needed).

Rule.  Every gate gradient is adjoint x coefficient (oracle.lucy_scan.lucy_scan_bwd_envelope):
the adjoint is O(|dout|), the coefficient carries the heavy tail (x / sqrt(x^2 + 1e-6) has slope
1e3 at zero, d kv reaches 1e8).  A tolerance relative to the tensor's largest element therefore
checks nothing but the outliers; instead, per element of plane g

    |got - ref| <= rtol |ref| + atol + C env[b,t,g,d] (A_g + cond[b,t,g,d]),
    A_g = max(max |adj_g|, max |dout|)

  env    the coefficient with every cancelling sum replaced by the sum of absolute values;
  cond   the adjoint's first-order movement per unit of relative error in the state s, which
         any working-precision implementation knows only to ~u sa_t (adj_cond in the oracle);
         O(|adj|) while sa is O(1), dominant on the chains where kv ~ 1e5 has blown s up;
  rtol   twice the storage rounding of the returned gradient: 1e-6 fp32, 2^-8 bf16, 2^-10 f16;
  atol   the storage format's underflow: 2^-24 for f16 (the spacing of its subnormals; a
         saturated gate's gradient ~ 1e-6 / |x|^3 ~ 1e-11 rounds to 0 there whatever the kernel
         does), 0 for bf16 and fp32 (fp32's exponent range);
  dh0, ds0 (fp32 for every gate dtype): rtol |ref| + C x the adjoint recurrences run on |dout|,
         |ds_last| with 1 - c^2 in its absolute-term form 1 + c^2, plus cond;
  dbias [B,7,D]: against the fp64 sum over T of dgates, the sum over T of the tolerances above;
  s_last |got - ref| <= C sa_T + 1e-6, sa the absolute-accumulated state;
  out    max |got - out64| <= 4 max |out32 - out64| + 2e-5 (the conditioning check of
         conftest.assert_ref_parity), both oracles run on the case; 16-bit outputs add 2^-8
         (bf16) / 2^-11 (f16) of |out64| elementwise.

C is measured, never tuned from kernel output: the fp32 oracle against the fp64 oracle in this
metric over cpu_cases() (every regime, the time and column edges).  Measured worst value 5.1e-7
(s_last of the D = 63 column case; the gradients reach 3.2e-7); C = 4 x 5.1e-7 = 2.04e-6.  The
factor 4: the kernels use the hardware rsq / rcp / exp2 approximations (1 ulp each) and compose
chunks in another order.  tests/test_scan_checker.py asserts the measurement.  (Without cond and
the 1 + c^2 form the fp32 oracle itself reaches 8.8e-4 on `mixed` and 4.9 on ds0 of `tiny`: the
error of an adjoint is then set by one chain's state, not by the tensor's scale.)

Gate regimes (all 7 planes alike):
  nominal    0.6 N(0,1)                       the regime of the older tests
  saturated  30 N(0,1)                        every normaliser at +-1, coefficients ~ 1e-6 / |x|^3
  zeros      nominal, 30% of the elements exactly 0 (masked features)
  pad        nominal, second half of T all zero (padded frames)
  mixed      N(0,1) 10^U(-4, 1.5) per element   near-zero and large gates side by side
  tiny       3e-3 N(0,1)                      s reaches ~1e5 and c = tanh saturates: the fp64
                                              gradients of all planes but the first steps' are
                                              ~0 -- a forward and finiteness case
"""
import numpy as np
import torch

from oracle import lucy_scan as oscan

C = 2.04e-6
RTOL = {"f32": 1e-6, "bf16": 2.0 ** -8, "f16": 2.0 ** -10}
ATOL = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -24}
OUT_REL = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F16_MAX = 65504.0
PLANES = oscan.GATE_NAMES


def _nominal(rng, s):
    return 0.6 * rng.standard_normal(s)


def _zeros(rng, s):
    g = _nominal(rng, s)
    g[rng.random(s) < 0.3] = 0.0
    return g


def _pad(rng, s):
    g = _nominal(rng, s)
    g[:, s[1] // 2:] = 0.0
    return g


REGIMES = {
    "nominal": _nominal,
    "saturated": lambda rng, s: 30.0 * rng.standard_normal(s),
    "zeros": _zeros,
    "pad": _pad,
    "mixed": lambda rng, s: rng.standard_normal(s) * 10.0 ** rng.uniform(-4.0, 1.5, s),
    "tiny": lambda rng, s: 3e-3 * rng.standard_normal(s),
}


def _round(x, dtype):
    return torch.as_tensor(np.asarray(x, np.float32)).to(TORCH_DTYPE[dtype]).float().numpy()


def draw_case(regime, B, T, D, dtype="f32", seed=0, bias=False):
    """fp32 arrays from one seeded generator: gates [B,T,7,D] and dout [B,T,D] rounded to the gate
    dtype (both sides see the rounded values), h0, s0 ~ 0.3 N, ds_last ~ N, all nonzero.
    bias: also a gate bias [7,D] ~ 0.2 N that the kernel adds on load (the oracle is fed
    gates + bias)."""
    rng = np.random.default_rng(seed)
    c = {"key": (regime, B, T, D, dtype, seed, bias), "dtype": dtype}
    c["gates"] = _round(REGIMES[regime](rng, (B, T, 7, D)), dtype)
    c["h0"] = (0.3 * rng.standard_normal((B, D))).astype(np.float32)
    c["s0"] = (0.3 * rng.standard_normal((B, D))).astype(np.float32)
    c["dout"] = _round(rng.standard_normal((B, T, D)), dtype)
    c["ds_last"] = rng.standard_normal((B, D)).astype(np.float32)
    if bias:
        c["bias"] = (0.2 * rng.standard_normal((7, D))).astype(np.float32)
    return c


def make_case(gates, h0, s0, dout, ds_last, dtype="f32", key=None):
    """A case from given arrays (already rounded to the gate dtype)."""
    return {"key": key, "dtype": dtype, "gates": np.asarray(gates), "h0": np.asarray(h0),
            "s0": np.asarray(s0), "dout": np.asarray(dout), "ds_last": np.asarray(ds_last)}


def oracle_gates(case):
    """What the recurrence sees, in fp64: gates (+ bias)."""
    g = case["gates"].astype(np.float64)
    return g + case["bias"].astype(np.float64)[None, None] if "bias" in case else g


_REF = {}


def reference(case):
    """fp64 forward and adjoint of the case, its error model, and the fp32 oracle's forward:
    {"out", "s_last", "out32", "dgates", "dh0", "ds0", "dbias", "adj", "env", "sa_last",
    "dh0_env", "ds0_env"}.  Computed once per case and shared; callers leave it unchanged."""
    key = case["key"]
    if key is not None and key in _REF:
        return _REF[key]
    g = oracle_gates(case)
    ref = {}
    ref["out"], ref["s_last"] = oscan.lucy_scan_fwd(g, case["h0"], case["s0"])
    ref["out32"], _ = oscan.lucy_scan_fwd(g.astype(np.float32), case["h0"], case["s0"],
                                          dtype=np.float32)
    ref["dgates"], ref["dh0"], ref["ds0"] = oscan.lucy_scan_bwd(g, case["h0"], case["s0"],
                                                                case["dout"], case["ds_last"])
    ref["dbias"] = ref["dgates"].sum(1)
    ref.update(oscan.lucy_scan_bwd_envelope(g, case["h0"], case["s0"], case["dout"],
                                            case["ds_last"]))
    if key is not None:
        _REF[key] = ref
    return ref


def oracle_fp32(case):
    """The fp32 oracle's results on the case (what C is measured with)."""
    g = oracle_gates(case).astype(np.float32)
    out, s = oscan.lucy_scan_fwd(g, case["h0"], case["s0"], dtype=np.float32)
    dg, dh0, ds0 = oscan.lucy_scan_bwd(g, case["h0"], case["s0"], case["dout"], case["ds_last"],
                                       dtype=np.float32)
    return {"out": out, "s_last": s, "dgates": dg, "dh0": dh0, "ds0": ds0, "dbias": dg.sum(1)}


def assert_fits_f16(ref):
    """Premise of an f16 case, judged from the fp64 side alone: the kernel returns dgates in f16,
    so the fp64 gradients must be representable there (d kv reaches 1e8 when k and v are both
    ~1e-2: inf in f16 whatever the kernel does).  25% headroom."""
    mx = float(np.abs(ref["dgates"]).max())
    assert mx <= 0.75 * F16_MAX, f"fp64 dgates reach {mx:.0f}: not an f16 case, change the seed"


def gate_scale(ref, dout):
    """A_g [7] = max(max |adj_g|, max |dout|)."""
    return np.maximum(np.abs(ref["adj"]).max(axis=(0, 1, 3)), np.abs(dout).max())


def gate_tolerance(ref, dout, dtype, c=C):
    """(fixed, per unit of c) parts of the dgates tolerance, [B,T,7,D] each."""
    fixed = RTOL[dtype] * np.abs(ref["dgates"]) + ATOL[dtype]
    return fixed, ref["env"] * (gate_scale(ref, dout)[None, None, :, None] + ref["adj_cond"])


def _metric(got, ref, fixed, unit):
    """max over elements of (|got - ref| - fixed) / unit, floored at 0: the c at which the
    element would just pass.  inf where got is not finite or the excess has no envelope."""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    excess = np.maximum(err - fixed, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(excess > 0, excess / unit, 0.0)
    return m


def check(case, got, ref=None):
    """got: dict with any of dgates [B,T,7,D], dh0, ds0, s_last [B,D], dbias [B,7,D], out [B,T,D]
    (arrays in fp32 / fp64; 16-bit results converted exactly).  Returns {name: worst metric}:
    gradients per plane ("dgates/r", ...) and dh0 / ds0 / dbias / s_last in units of c (pass iff
    <= C), "out" in units of its bound (pass iff <= 1)."""
    ref = reference(case) if ref is None else ref
    dtype = case["dtype"]
    m = {}
    if "dgates" in got:
        fixed, unit = gate_tolerance(ref, case["dout"], dtype)
        e = _metric(got["dgates"], ref["dgates"], fixed, unit)
        for i, name in enumerate(PLANES):
            m["dgates/" + name] = float(e[:, :, i].max()) if e.size else 0.0
    if "dbias" in got:
        fixed, unit = gate_tolerance(ref, case["dout"], dtype)
        m["dbias"] = float(_metric(got["dbias"], ref["dbias"], fixed.sum(1), unit.sum(1)).max())
    for name in ("dh0", "ds0"):
        if name in got:
            m[name] = float(_metric(got[name], ref[name], RTOL["f32"] * np.abs(ref[name]),
                                    ref[name + "_env"]).max())
    if "s_last" in got:
        m["s_last"] = float(_metric(got["s_last"], ref["s_last"], 1e-6, ref["sa_last"]).max())
    if "out" in got and ref["out"].size:
        bound = 4.0 * np.abs(ref["out32"] - ref["out"]).max() + 2e-5
        m["out"] = float(_metric(got["out"], ref["out"], OUT_REL[dtype] * np.abs(ref["out"]),
                                 bound).max())
    return m


def failures(metrics, c=C):
    return {k: v for k, v in metrics.items() if not v <= (1.0 if k == "out" else c)}


def assert_parity(case, got, ref=None, label=""):
    m = check(case, got, ref)
    print(f"scan parity {label or case['key']}: worst metric "
          + ", ".join(f"{k} {v:.1e}" for k, v in m.items()))
    bad = failures(m)
    assert not bad, f"{label or case['key']}: over C = {C:g} (out: over 1): {bad}"
    return m


def assert_s_last(gates, h0, s0, got, label="s_last"):
    """The elementwise s_last rule alone: |got - ref| <= C sa_T + 1e-6 against the fp64 forward."""
    case = make_case(gates, h0, s0, np.zeros(np.shape(gates)[:2] + np.shape(gates)[3:]),
                     np.zeros(np.shape(h0)))
    return assert_parity(case, {"s_last": got}, label=label)


def zero_plane_share(case, plane, ref=None):
    """Share of the plane's elements on which an all-zero gradient passes the rule."""
    ref = reference(case) if ref is None else ref
    fixed, unit = gate_tolerance(ref, case["dout"], case["dtype"])
    ok = np.abs(ref["dgates"]) <= fixed + C * unit
    return float(ok[:, :, plane].mean())


# ---- the case list C is measured over (test_scan_checker) and the GPU tests draw from --------
REGIME_SHAPE = (2, 130, 64)
T_EDGES = (1, 4, 5, 8, 9, 63, 64, 65, 128, 129)      # fwd 4 steps / wave, bwd 8, chunk 64
D_EDGES = (1, 63, 65, 72, 200)                       # narrow pieces; wide with a partial block
T_COLS = 70
# f16 premise (assert_fits_f16): nominal fits at seed 0 and D = 72 at seed 273 (272 reaches 4e5).
# `zeros` never fits: k = 0 beside |v| < 0.04 gives dk = gs alp 4 / v^3 > 65504 on ~1% of the
# elements at every seed, so its f16 run checks dgates only where the fp64 value fits
F16_REGIMES = ("nominal", "saturated")
COL_SEED = {(72, "f16"): 273}


def regime_case(regime, dtype):
    return draw_case(regime, *REGIME_SHAPE, dtype=dtype, seed=0)


def time_edge_case(T, dtype):
    return draw_case("nominal", 2, T, 64, dtype=dtype, seed=100 + T)


def col_edge_case(D, dtype):
    return draw_case("nominal", 2, T_COLS, D, dtype=dtype, seed=COL_SEED.get((D, dtype), 200 + D))


def cpu_cases():
    for regime in REGIMES:
        for dtype in ("f32", "bf16"):
            yield regime_case(regime, dtype)
    for regime in F16_REGIMES:
        yield regime_case(regime, "f16")
    for T in T_EDGES:
        yield time_edge_case(T, "f32")
    for D in D_EDGES:
        yield col_edge_case(D, "f32")
    yield draw_case("nominal", 2, 70, 128, dtype="bf16", seed=300, bias=True)
    yield draw_case("nominal", 2, 130, 64, dtype="f32", seed=400)
