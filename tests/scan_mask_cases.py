"""Cases, masks, references and the row checker of the masked LucyRNN scan (test infrastructure,
no GPU needed).

Definition.  For a mask m[b,t] (nonzero = live) the masked scan on a row IS the unmasked scan on
that row's live frames, scattered back: a held frame leaves (h, s) untouched, writes zero to out
and gets zero gradient; s_last / h_last are the state after the last live frame and dL/dh_last
reaches that frame.  So the reference of a row is scan_cases.make_case on its live frames with
B = 1, dout compacted the same way and dh_last added to dout at the last live step in fp64.  It is
judged by scan_cases.check at scan_cases.C: no new tolerance.  (The oracle needs no change.)

tests/test_scan_mask_checker.py asserts the premise (the fp32 oracle on every compacted row stays
within C / 4) and that this checker rejects the mutants a wrong kernel would produce.
"""
import numpy as np

from oracle import lucy_scan as oscan
from tests import scan_cases as sc

B = 3
# (T, D): one step; less than a forward (4 steps) and a backward (8 steps) wave segment; exactly
# one super-chunk; one step over it, with a partial column block; two super-chunks plus a tail, on
# full blocks and with a partial column block
SHAPES = ((1, 64), (5, 64), (64, 64), (65, 72), (130, 64), (130, 72))
MASKS = ("all_live", "prefix", "holes", "random")


# f16 premise (scan_cases.assert_fits_f16 on the compacted rows, found from the fp64 side alone):
# at (130, 72) seeds 1102 and 1103 have d kv at 2e5 and 8e5; 1104 is the first that fits (3.1e3)
F16_SEED = {(130, 72): 1104}


def base_case(T, D, dtype, bias=False):
    seed = F16_SEED.get((T, D), 900 + T + D) if dtype == "f16" else 900 + T + D
    return sc.draw_case("nominal", B, T, D, dtype, seed=seed, bias=bias)


def draw_extras(T, D, dtype):
    """(dh_last [B,D] rounded to the gate dtype, {mask name: bool [B,T]})."""
    rng = np.random.default_rng(7 + T)
    dh_last = sc._round(rng.standard_normal((B, D)), dtype)
    masks = {"all_live": np.ones((B, T), bool)}
    lens = (T, max(2 * T // 3 - 1, 0), 0)
    masks["prefix"] = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    h = np.ones((B, T), bool)
    h[0, 0] = False
    h[1, T - 1] = False
    h[:, T // 2] = False
    if T > 70:
        h[0, 60:70] = False     # crosses the super-chunk boundary
        h[2, 64:128] = False    # a whole super-chunk
    masks["holes"] = h
    masks["random"] = rng.random((B, T)) < 0.6
    return dh_last, masks


def row_case(case, mask, dh_last, b, name=None):
    """The compacted B = 1 case of row b (None when the row has no live frame)."""
    idx = np.nonzero(mask[b])[0]
    if len(idx) == 0:
        return None
    dout = case["dout"][b:b + 1, idx].astype(np.float64)
    dout[0, -1] += dh_last[b].astype(np.float64)
    key = None if name is None or case["key"] is None else ("masked", case["key"], name, b)
    rc = sc.make_case(case["gates"][b:b + 1, idx], case["h0"][b:b + 1], case["s0"][b:b + 1], dout,
                      case["ds_last"][b:b + 1], case["dtype"], key=key)
    if "bias" in case:
        rc["bias"] = case["bias"]
    return rc


def row_metrics(case, mask, dh_last, got, name=None):
    """got: dict of full arrays (out [B,T,D], s_last, h_last, dh0, ds0 [B,D], dgates [B,T,7,D],
    dbias [B,7,D]; any subset).  Returns {(b, quantity): metric} in scan_cases.check's units, plus
    "held_out" / "held_dgates" (number of nonzero elements at held frames: must be 0) and, for a
    row with no live frame, "pass/<name>" (number of elements that are not passed through
    exactly: must be 0)."""
    m = {}
    for b in range(mask.shape[0]):
        live = mask[b].astype(bool)
        idx = np.nonzero(live)[0]
        for k in ("out", "dgates"):
            if k in got:
                held = np.asarray(got[k])[b, ~live]
                m[(b, "held_" + k)] = float(np.count_nonzero(held) + np.isnan(held).sum())
        rc = row_case(case, mask, dh_last, b, name)
        if rc is None:
            through = {"s_last": case["s0"], "h_last": case["h0"], "dh0": dh_last,
                       "ds0": case["ds_last"]}
            for k, want in through.items():
                if k in got:
                    m[(b, "pass/" + k)] = float((np.asarray(got[k])[b] != want[b]).sum())
            if "dbias" in got:
                m[(b, "pass/dbias")] = float(np.count_nonzero(np.asarray(got["dbias"])[b]))
            continue
        ref = sc.reference(rc)
        g = {}
        for k in ("out", "dgates"):
            if k in got:
                g[k] = np.asarray(got[k])[b:b + 1, idx]
        for k in ("s_last", "dh0", "ds0", "dbias"):
            if k in got:
                g[k] = np.asarray(got[k])[b:b + 1]
        for k, v in sc.check(rc, g, ref).items():
            m[(b, k)] = v
        if "h_last" in got:   # fp32, unrounded: the out rule of the last live step
            bound = 4.0 * np.abs(ref["out32"] - ref["out"]).max() + 2e-5
            m[(b, "h_last")] = float(sc._metric(np.asarray(got["h_last"])[b], ref["out"][0, -1],
                                                0.0, bound).max())
    return m


def row_failures(metrics):
    bad = {}
    for (b, k), v in metrics.items():
        if k.startswith("held_") or k.startswith("pass/"):
            lim = 0.0
        elif k in ("out", "h_last"):
            lim = 1.0
        else:
            lim = sc.C
        if not v <= lim:
            bad[(b, k)] = v
    return bad


def assert_rows(case, mask, dh_last, got, name=None, label=""):
    m = row_metrics(case, mask, dh_last, got, name)
    worst = {}
    for (b, k), v in m.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"masked scan {label or (case['key'], name)}: worst "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    bad = row_failures(m)
    assert not bad, f"{label or (case['key'], name)}: over C = {sc.C:g} (out, h_last: over 1; held, pass: over 0): {bad}"
    return m


def identity_loop(case, mask, dh_last, held_dout=False):
    """The definition restated step by step in fp64: every live frame is one step of the oracle
    from the running (h, s), every held frame an identity step (state kept, out zero); backwards,
    the adjoints (Gh, Gs) start at (dh_last, ds_last), a live frame runs the oracle's one-step
    adjoint, a held frame passes them on and gets zero gradient with its dout ignored.
    held_dout=True is the mutant that lets a held frame's dout into the Gh chain."""
    g = sc.oracle_gates(case)
    Bn, T, _, D = g.shape
    h = case["h0"].astype(np.float64)
    s = case["s0"].astype(np.float64)
    hs, ss = [h], [s]
    out = np.zeros((Bn, T, D))
    for t in range(T):
        o, sn = oscan.lucy_scan_fwd(g[:, t:t + 1], h, s)
        live = mask[:, t, None].astype(bool)
        h = np.where(live, o[:, 0], h)
        s = np.where(live, sn, s)
        out[:, t] = np.where(live, o[:, 0], 0.0)
        hs.append(h)
        ss.append(s)
    gh = dh_last.astype(np.float64)
    gs = case["ds_last"].astype(np.float64)
    dg = np.zeros_like(g)
    for t in range(T - 1, -1, -1):
        live = mask[:, t, None].astype(bool)
        d = case["dout"][:, t].astype(np.float64)
        dgt, dh, ds = oscan.lucy_scan_bwd(g[:, t:t + 1], hs[t], ss[t], (d + gh)[:, None], gs)
        dg[:, t] = np.where(live[:, None], dgt[:, 0], 0.0)
        gh = np.where(live, dh, gh + d if held_dout else gh)
        gs = np.where(live, ds, gs)
    return {"out": out, "s_last": s, "h_last": h, "dgates": dg, "dh0": gh, "ds0": gs,
            "dbias": dg.sum(1)}


def compacted_reference(case, mask, dh_last, name=None):
    """The per-row fp64 references scattered back into full arrays (the definition)."""
    Bn, T, _, D = case["gates"].shape
    r = {"out": np.zeros((Bn, T, D)), "dgates": np.zeros((Bn, T, 7, D)),
         "s_last": case["s0"].astype(np.float64), "h_last": case["h0"].astype(np.float64),
         "dh0": dh_last.astype(np.float64), "ds0": case["ds_last"].astype(np.float64)}
    for b in range(Bn):
        rc = row_case(case, mask, dh_last, b, name)
        if rc is None:
            continue
        idx = np.nonzero(mask[b])[0]
        ref = sc.reference(rc)
        r["out"][b, idx] = ref["out"][0]
        r["dgates"][b, idx] = ref["dgates"][0]
        r["s_last"][b], r["h_last"][b] = ref["s_last"][0], ref["out"][0, -1]
        r["dh0"][b], r["ds0"][b] = ref["dh0"][0], ref["ds0"][0]
    r["dbias"] = r["dgates"].sum(1)
    return r


# ---- the module-level cases (tests/test_gpu_masked_module.py) ---------------------------------
MODULE_CASES = ((40, 128, 5, 3, 32, 70), (10, 48, 17, 2, 12, 23))   # (Din, D, B, L, V, T)


def module_inputs(Din, D, Bn, L, V, T):
    """(oracle parameters, x [B,T,Din] fp32, masks bool [B,T], loss weights [B,T,V] fp32 that are
    zero at held frames): test_streaming_vs_oracle_ragged's recipe."""
    from tests.tframe_ref import conditioned_params, ragged_masks
    p = conditioned_params(L, Din, D, V, seed=D + Bn)
    x = np.random.default_rng(Bn).standard_normal((Bn, T, Din)).astype(np.float32)
    masks = ragged_masks(Bn, T, seed=D)
    w = np.random.default_rng(Bn + 1).standard_normal((Bn, T, V)).astype(np.float32)
    return p, x, masks, w * masks[..., None]


def state_dict_of(p, L, dtype):
    """The oracle parameters under LucyRNNtriton.state_dict()'s names, as torch leaves."""
    import torch
    names = {}
    for l in range(L):
        names[f"tracks.0.{l}.linear.weight"] = p[f"W{l}"]
        names[f"tracks.0.{l}.linear.bias"] = p[f"b{l}"]
        if l < L - 1:
            names[f"norms.0.{l}.weight"] = p[f"g{l}"]
            names[f"norms.0.{l}.bias"] = p[f"be{l}"]
    names["output_proj.weight"], names["output_proj.bias"] = p["Wo"], p["bo"]
    return {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in names.items()}


def ref_param_grads(p, x, masks, w, L, D, dtype):
    """Gradients of sum over live frames of logits * w with respect to every parameter:
    torch_ref.lucyrnn64 autograd on each row's live frames (B = 1), summed over rows, in `dtype`
    on the CPU.  {state_dict name: float64 array}."""
    import torch
    from tests.torch_ref import lucyrnn64
    params = state_dict_of(p, L, dtype)
    total = None
    for b in range(x.shape[0]):
        idx = np.nonzero(masks[b])[0]
        if len(idx) == 0:
            continue
        xb = torch.tensor(x[b:b + 1, idx], dtype=dtype)
        logits, _ = lucyrnn64(params, xb, L, D)
        loss = (logits * torch.tensor(w[b:b + 1, idx], dtype=dtype)).sum()
        total = loss if total is None else total + loss
    total.backward()
    return {k: v.grad.double().numpy() for k, v in params.items()}


def rel_l2(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / np.linalg.norm(ref))
