"""Every output of the LucyRNN scan kernels against the fp64 oracle, elementwise at the scale of
each element's own step (the rule and the cases: tests/scan_cases.py).  Forward and backward run
with h0, s0, dout and ds_last all nonzero; dgates, dh0, ds0, out and s_last are all checked.

Kernel instances reached (dispatch_fwd / dispatch_bwd in lucy_scan.hip): fp32 / bf16 / f16 x
16-byte pieces or one-element pieces (D % (16 / esize) != 0, or an unaligned base), the 16-bit
wide store of dgates, a partial last column block, the step-blocked layout with the bias on
load, and the split forward on both piece widths."""
import numpy as np
import pytest
import torch

from oracle import lucy_scan as oscan
from tests import scan_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def ops():
    from statecatcher_amd import ops as o
    return o


def _np(t):
    return t.detach().float().cpu().numpy()


def _blocked(g):
    B, T, _, D = g.shape
    return g.view(B, T, 7, D // 64, 64).permute(0, 1, 3, 2, 4).contiguous()


def _unblocked(g):
    B, T, NB = g.shape[:3]
    return g.permute(0, 1, 3, 2, 4).reshape(B, T, 7, NB * 64)


def device_gates(case, blocked=False, offset=0):
    """The case's gates on the device in its dtype; offset: as a slice [..., offset:] of a wider
    tensor, so the base is not 16-byte aligned (one-element pieces)."""
    g = torch.as_tensor(case["gates"]).to(sc.TORCH_DTYPE[case["dtype"]])
    if offset:
        full = torch.zeros(g.shape[:3] + (g.shape[3] + offset,), dtype=g.dtype)
        full[..., offset:] = g
        g = full.to(DEV)[..., offset:]
        assert g.stride(3) == 1 and g.data_ptr() % 16
        return g
    g = g.to(DEV)
    return _blocked(g) if blocked else g


def run_kernels(case, blocked=False, offset=0, want_dbias=False):
    """Forward and backward through the C ABI: {out, s_last, dgates, dh0, ds0 (, dbias)}."""
    dt = sc.TORCH_DTYPE[case["dtype"]]
    g = device_gates(case, blocked, offset)
    bias = torch.as_tensor(case["bias"]).to(DEV) if "bias" in case else None
    h0, s0 = torch.as_tensor(case["h0"]).to(DEV), torch.as_tensor(case["s0"]).to(DEV)
    g, out, s_last, ckpt = ops()._scan_fwd(g, h0, s0, True, bias)
    dg, dh0, ds0, dbias = ops()._scan_bwd(g, ckpt, torch.as_tensor(case["dout"]).to(DEV, dt),
                                          torch.as_tensor(case["ds_last"]).to(DEV), want_dbias, bias)
    assert dg.dtype == dt and out.dtype == dt
    got = {"out": _np(out), "s_last": _np(s_last), "dgates": _np(_unblocked(dg) if blocked else dg),
           "dh0": _np(dh0), "ds0": _np(ds0)}
    if want_dbias:
        got["dbias"] = _np(dbias)
    return got


def _beyond_f16(case, got):
    """f16 `zeros` (scan_cases.F16_REGIMES): where the fp64 gradient does not fit f16 the kernel
    must return inf or a value at the top of the range, of the right sign; those elements are
    then taken out of the elementwise check."""
    ref = sc.reference(case)["dgates"]
    big = np.abs(ref) > 0.75 * sc.F16_MAX
    assert 0 < big.mean() < 0.05
    g = got["dgates"]
    assert (np.sign(g[big]) == np.sign(ref[big])).all() and (np.abs(g[big]) >= 0.74 * sc.F16_MAX).all()
    got["dgates"] = np.where(big, ref, g)
    return got


INSTANCES = [(r, d) for r in ("nominal", "saturated", "zeros") for d in ("f32", "bf16", "f16")]
INSTANCES += [(r, d) for r in ("mixed", "pad", "tiny") for d in ("f32", "bf16")]


@pytest.mark.parametrize("regime,dtype", INSTANCES)
def test_kernel_instances_vs_fp64(regime, dtype):
    case = sc.regime_case(regime, dtype)
    got = run_kernels(case)
    if dtype == "f16":
        if regime in sc.F16_REGIMES:
            sc.assert_fits_f16(sc.reference(case))
        else:
            got = _beyond_f16(case, got)
    assert all(np.isfinite(v).all() for k, v in got.items())
    sc.assert_parity(case, got)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("T", sc.T_EDGES)
def test_time_edges_vs_fp64(T, dtype):
    case = sc.time_edge_case(T, dtype)
    sc.assert_parity(case, run_kernels(case))


@pytest.mark.parametrize("D,dtype", [(D, d) for D in sc.D_EDGES for d in ("f32", "bf16")] + [(72, "f16")])
def test_column_edges_vs_fp64(D, dtype):
    case = sc.col_edge_case(D, dtype)
    if dtype == "f16":
        sc.assert_fits_f16(sc.reference(case))
    sc.assert_parity(case, run_kernels(case))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("blocked", [False, True])
def test_layouts_and_bias_vs_fp64(blocked, dtype):
    """gate_bias added on load in both layouts; dbias [B,7,D] against the fp64 sum over T."""
    case = sc.draw_case("nominal", 2, 70, 128, dtype=dtype, seed=300, bias=True)
    sc.assert_parity(case, run_kernels(case, blocked=blocked, want_dbias=True))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unaligned_slice_vs_fp64(dtype):
    """D = 64 from a slice one element into a wider tensor: one-element pieces at a full block."""
    case = sc.draw_case("nominal", 2, 70, 64, dtype=dtype, seed=301)
    sc.assert_parity(case, run_kernels(case, offset=1))


@pytest.mark.parametrize("D,offset", [(72, 0), (64, 1)])
def test_split_forward_vs_fp64(D, offset):
    """sc_lucy_scan_fwd_split on 16-byte pieces with a partial last block (D = 72) and on
    one-element pieces (D = 64 from an unaligned slice)."""
    case = sc.draw_case("nominal", 2, 70, D, dtype="bf16", seed=310 + D)
    ref = sc.reference(case)
    g = device_gates(case, offset=offset)
    h0, s0 = torch.as_tensor(case["h0"]).to(DEV), torch.as_tensor(case["s0"]).to(DEV)
    _, out, s_last, _, h_out, wide = ops()._scan_fwd(g, h0, s0, False, want_h=True, split=True)
    _, plain, s_plain, _ = ops()._scan_fwd(g, h0, s0, False)
    assert torch.equal(out, plain) and torch.equal(s_last, s_plain)
    assert torch.equal(wide[..., D:2 * D], out)
    sc.assert_parity(case, {"out": _np(out), "s_last": _np(s_last)})
    noise = np.abs(ref["out32"] - ref["out"]).max()
    hs = _np(out).astype(np.float64) + _np(wide[..., 2 * D:])
    # hi + lo carries h to 2^-15 relative (test_split_scan_planes' bound), on top of the fp32
    # recurrence's own distance from fp64 (4 x the fp32 oracle's)
    err = np.abs(hs - ref["out"])
    bound = 2.0 ** -15 * np.maximum(np.abs(ref["out"]), 1e-3) + 4 * noise
    print(f"split D={D}: max |hi + lo - h64| / bound {(err / bound).max():.2f}, "
          f"max rel {(err / np.maximum(np.abs(ref['out']), 1e-3)).max():.2e}")
    assert (err <= bound).all()
    eh = np.abs(_np(h_out) - ref["out"][:, -1]).max()
    assert eh <= 4 * noise + 2e-5, (eh, noise)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_carried_segments_vs_one_pass_fp64(dtype):
    """T = 130 cut at 70 (no chunk multiple).  Segment 2 starts from segment 1's last h (fp32:
    out1[:, -1]; bf16: the unrounded h_out) and s; its dh0 joins dout1's last step and its ds0 is
    segment 1's ds_last.  The concatenated dgates, segment 1's dh0 / ds0, out and s_last are checked
    against the ONE-PASS fp64 run; segment 2's dh0 / ds0 against the one-pass carries at the cut.

    bf16: dout is a bf16 tensor, so the join dout1[:, -1] + dh0_2 is rounded to bf16 before the
    kernel sees it.  That is a rounding of an input: the one-pass reference is fed the dout whose
    last step of segment 1 makes its Gh there exactly the joined value (the kernel's dh0_2 does not
    enter the reference otherwise, and is itself checked against fp64)."""
    cut = 70
    case = sc.draw_case("nominal", 2, 130, 64, dtype=dtype, seed=320)
    dt = sc.TORCH_DTYPE[dtype]
    g = device_gates(case)
    dev = lambda k: torch.as_tensor(case[k]).to(DEV)
    g1, out1, s1, ck1, h1 = ops()._scan_fwd(g[:, :cut], dev("h0"), dev("s0"), True, want_h=True)
    carry = out1[:, -1].float() if dtype == "f32" else h1
    g2, out2, s2, ck2 = ops()._scan_fwd(g[:, cut:], carry, s1, True)
    dout = dev("dout").to(dt)
    dg2, dh2, ds2, _ = ops()._scan_bwd(g2, ck2, dout[:, cut:], dev("ds_last"), False)
    dout1 = dout[:, :cut].clone()
    dout1[:, -1] += dh2.to(dt)
    dg1, dh0, ds0, _ = ops()._scan_bwd(g1, ck1, dout1, ds2, False)
    # segment 2 alone, from the fp64 state at the cut: the one-pass carries zg Gh and dec Gs there
    gg = sc.oracle_gates(case)
    o64, s64 = oscan.lucy_scan_fwd(gg[:, :cut], case["h0"], case["s0"])
    seg2 = sc.make_case(case["gates"][:, cut:], o64[:, -1], s64, case["dout"][:, cut:],
                        case["ds_last"], dtype)
    ref2 = sc.reference(seg2)
    sc.assert_parity(seg2, {"dh0": _np(dh2), "ds0": _np(ds2)}, ref2, label=f"segment 2 {dtype}")
    one = case
    if dtype != "f32":
        d = np.array(case["dout"], np.float64)
        d[:, cut - 1] = _np(dout1[:, -1]).astype(np.float64) - ref2["dh0"]
        one = sc.make_case(case["gates"], case["h0"], case["s0"], d, case["ds_last"], dtype)
    got = {"out": _np(torch.cat([out1, out2], 1)), "s_last": _np(s2),
           "dgates": _np(torch.cat([dg1, dg2], 1)), "dh0": _np(dh0), "ds0": _np(ds0)}
    sc.assert_parity(one, got, label=f"two segments {dtype}")
