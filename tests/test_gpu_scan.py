"""GPU parity of the LucyRNN scan (HIP, through the C ABI) against the reference fixtures and
the oracle.  Tolerances:
  fp32 gates/outputs: 1e-3 relative (north_star) + small absolute floor — observed ~1e-6;
  bf16 gates: compared with the oracle fed the SAME bf16-rounded gates; outputs are stored in
              bf16 so the bound is 1e-2 rel + 1e-2 abs (2.5 bf16 ulps);
  gradients: 1e-3 relative to the largest |grad| of the tensor (mixed abs/rel; the per-element
              normaliser x/sqrt(x^2+1e-6) has derivatives up to ~1e3 near 0) -- a bound
              that one outlier of the k / v planes sets, so every gradient and s_last is ALSO
              checked elementwise at the scale of its own step (tests/scan_cases.py).
"""
import numpy as np
import pytest
import torch

from oracle import lucy_scan as oscan
from tests import scan_cases
from tests.conftest import cases, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def ops():
    from statecatcher_amd import ops as o
    return o


def run_fwd(gates, h0, s0, dtype=torch.float32):
    g = torch.as_tensor(gates).to(DEV, dtype)
    out, s = ops().lucy_scan(g, torch.as_tensor(h0).to(DEV), torch.as_tensor(s0).to(DEV))
    return out.float().cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("name", cases(load_golden("scan_fwd"), "gates"))
def test_fwd_fp32_vs_reference_triton(name):
    z = load_golden("scan_fwd")
    out, s = run_fwd(z[name + "/gates"], z[name + "/h0"], z[name + "/s0"])
    np.testing.assert_allclose(out, z[name + "/out"], rtol=1e-3, atol=1e-5)
    ref_s = z[name + "/s_out"]
    np.testing.assert_allclose(s, ref_s, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(ref_s).max()))


def test_fwd_segment_carry_contiguous():
    z = load_golden("scan_fwd")
    out1, s1 = run_fwd(z["carry/g1"], np.zeros((3, 16), np.float32), np.zeros((3, 16), np.float32))
    np.testing.assert_allclose(out1, z["carry/out1"], rtol=1e-4, atol=1e-6)
    out2, s2 = run_fwd(z["carry/g2"], np.ascontiguousarray(out1[:, -1]), s1)
    np.testing.assert_allclose(out2, z["carry/out2_contig"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(s2, z["carry/s2_contig"], rtol=1e-4, atol=1e-5)


def test_strided_h0_view_is_read_correctly():
    """passing out[:, -1] (a strided view) must behave like its contiguous copy."""
    z = load_golden("scan_fwd")
    g1 = torch.as_tensor(z["carry/g1"]).to(DEV)
    g2 = torch.as_tensor(z["carry/g2"]).to(DEV)
    zero = torch.zeros(3, 16, device=DEV)
    o1, s1 = ops().lucy_scan(g1, zero, zero)
    view = o1[:, -1, :]
    assert not view.is_contiguous()
    o2, _ = ops().lucy_scan(g2, view, s1)
    np.testing.assert_allclose(o2.cpu().numpy(), z["carry/out2_contig"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("B,T,D", [(1, 1, 1), (2, 63, 64), (2, 64, 64), (3, 65, 65), (2, 129, 200),
                                   (1, 300, 7), (5, 200, 130)])
def test_fwd_shapes_vs_oracle(B, T, D):
    rng = np.random.default_rng(B * 1000 + T + D)
    gates = (rng.standard_normal((B, T, 7, D)) * 0.6).astype(np.float32)
    h0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    s0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    out, s = run_fwd(gates, h0, s0)
    ro, rs = oscan.lucy_scan_fwd(gates, h0, s0)
    np.testing.assert_allclose(out, ro, rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(s, rs, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(rs).max()))
    scan_cases.assert_s_last(gates, h0, s0, s)


def test_T0_returns_initial_state():
    h0 = torch.randn(2, 8, device=DEV)
    s0 = torch.randn(2, 8, device=DEV)
    out, s = ops().lucy_scan(torch.empty(2, 0, 7, 8, device=DEV), h0, s0)
    assert out.shape == (2, 0, 8)
    torch.testing.assert_close(s, s0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fwd_half_gates_vs_oracle_on_rounded_inputs(dtype):
    rng = np.random.default_rng(7)
    B, T, D = 3, 257, 128
    gates = torch.as_tensor(rng.standard_normal((B, T, 7, D)).astype(np.float32) * 0.5).to(dtype)
    h0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    s0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    out, s = run_fwd(gates, h0, s0, dtype=dtype)
    ro, rs = oscan.lucy_scan_fwd(gates.float().numpy(), h0, s0)
    np.testing.assert_allclose(out, ro, rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(s, rs, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(rs).max()))
    scan_cases.assert_s_last(gates.float().numpy(), h0, s0, s)


@pytest.mark.parametrize("name", cases(load_golden("scan_bwd"), "dgates"))
def test_bwd_fp32_vs_autograd_fixture(name):
    zf = load_golden("scan_fwd")
    zb = load_golden("scan_bwd")
    g = torch.as_tensor(zf[name + "/gates"]).to(DEV).requires_grad_(True)
    h0 = torch.as_tensor(zf[name + "/h0"]).to(DEV).requires_grad_(True)
    s0 = torch.as_tensor(zf[name + "/s0"]).to(DEV).requires_grad_(True)
    out, s_last = ops().lucy_scan(g, h0, s0)
    dout = torch.as_tensor(zb[name + "/dout"]).float().to(DEV)
    ds = torch.as_tensor(zb[name + "/ds_last"]).float().to(DEV)
    ((out * dout).sum() + (s_last * ds).sum()).backward()
    for got, key in [(g.grad, "/dgates"), (h0.grad, "/dh0"), (s0.grad, "/ds0")]:
        ref = zb[name + key]
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())
    # elementwise, against the fp64 oracle on the fixture's inputs (test_oracle_golden pins the
    # oracle to these autograd fixtures)
    case = scan_cases.make_case(zf[name + "/gates"], zf[name + "/h0"], zf[name + "/s0"],
                                zb[name + "/dout"], zb[name + "/ds_last"])
    scan_cases.assert_parity(case, {"dgates": g.grad.cpu().numpy(), "dh0": h0.grad.cpu().numpy(),
                                    "ds0": s0.grad.cpu().numpy(), "out": out.detach().cpu().numpy(),
                                    "s_last": s_last.detach().cpu().numpy()}, label=name)


@pytest.mark.parametrize("B,T,D", [(2, 1, 16), (2, 64, 64), (3, 65, 100), (2, 300, 64), (4, 1500, 128)])
def test_bwd_shapes_vs_oracle(B, T, D):
    rng = np.random.default_rng(T + D)
    gates = (rng.standard_normal((B, T, 7, D)) * 0.6).astype(np.float32)
    h0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    s0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    dout = rng.standard_normal((B, T, D)).astype(np.float32)
    ds = rng.standard_normal((B, D)).astype(np.float32)
    g = torch.as_tensor(gates).to(DEV).requires_grad_(True)
    hh = torch.as_tensor(h0).to(DEV).requires_grad_(True)
    ss = torch.as_tensor(s0).to(DEV).requires_grad_(True)
    out, s_last = ops().lucy_scan(g, hh, ss)
    ((out * torch.as_tensor(dout).to(DEV)).sum() + (s_last * torch.as_tensor(ds).to(DEV)).sum()).backward()
    rg, rh, rs = oscan.lucy_scan_bwd(gates, h0, s0, dout, ds)
    for got, ref in [(g.grad, rg), (hh.grad, rh), (ss.grad, rs)]:
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())
    case = scan_cases.make_case(gates, h0, s0, dout, ds)
    scan_cases.assert_parity(case, {"dgates": g.grad.cpu().numpy(), "dh0": hh.grad.cpu().numpy(),
                                    "ds0": ss.grad.cpu().numpy(), "out": out.detach().cpu().numpy(),
                                    "s_last": s_last.detach().cpu().numpy()}, label=f"{B}x{T}x{D}")


def test_bwd_bf16_vs_oracle_on_rounded_inputs():
    rng = np.random.default_rng(11)
    B, T, D = 2, 200, 64
    gates = torch.as_tensor(rng.standard_normal((B, T, 7, D)).astype(np.float32) * 0.5).bfloat16()
    dout = torch.as_tensor(rng.standard_normal((B, T, D)).astype(np.float32)).bfloat16()
    g = gates.to(DEV).requires_grad_(True)
    zero = torch.zeros(B, D, device=DEV)
    out, _ = ops().lucy_scan(g, zero, zero)
    (out.float() * dout.float().to(DEV)).sum().backward()
    rg, _, _ = oscan.lucy_scan_bwd(gates.float().numpy(), np.zeros((B, D)), np.zeros((B, D)),
                                   dout.float().numpy(), np.zeros((B, D)))
    got = g.grad.float().cpu().numpy()
    # bf16-stored gradients: relative to the tensor's scale
    np.testing.assert_allclose(got, rg, rtol=2e-2, atol=1e-2 * np.abs(rg).max())
    case = scan_cases.make_case(gates.float().numpy(), np.zeros((B, D)), np.zeros((B, D)),
                                dout.float().numpy(), np.zeros((B, D)), "bf16")
    scan_cases.assert_parity(case, {"dgates": got, "out": out.detach().float().cpu().numpy()},
                             label="bf16 200x64")


def test_full_size_bf16_determinism_and_segment_consistency():
    """B=32, T=1500, D=512 (the C2 training shape): bitwise deterministic, and running the
    sequence as two carried segments equals one pass (chunk-boundary placement only)."""
    torch.manual_seed(0)
    B, T, D = 32, 1500, 512
    gates = (torch.randn(B, T, 7, D, device=DEV) * 0.5).bfloat16()
    h0 = torch.zeros(B, D, device=DEV)
    s0 = torch.zeros(B, D, device=DEV)
    o1, s1 = ops().lucy_scan(gates, h0, s0)
    o2, s2 = ops().lucy_scan(gates, h0, s0)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    a, sa = ops().lucy_scan(gates[:, :700], h0, s0)
    b, sb = ops().lucy_scan(gates[:, 700:], a[:, -1].float(), sa)
    torch.testing.assert_close(torch.cat([a, b], 1).float(), o1.float(), rtol=2e-2, atol=2e-2)
    # every batch row against the oracle fed the same bf16 gates: the output is stored in bf16
    # (<= half an ulp = 2^-9 relative of rounding, plus fp32 noise), s_last in fp32
    ro, rs = oscan.lucy_scan_fwd(gates.float().cpu().numpy(), np.zeros((B, D)), np.zeros((B, D)))
    got = o1.float().cpu().numpy()
    err = np.abs(got - ro)
    print(f"full-size scan fwd, all {B} rows: max |out - oracle| {err.max():.2e}, max rel "
          f"{(err / np.maximum(np.abs(ro), 1e-6)).max():.2e}; s_last max rel "
          f"{(np.abs(s1.cpu().numpy() - rs) / np.maximum(np.abs(rs), 1.0)).max():.2e}")
    np.testing.assert_allclose(got, ro, rtol=2.0 ** -8, atol=2e-5)
    np.testing.assert_allclose(s1.cpu().numpy(), rs, rtol=1e-3, atol=1e-3)


def test_full_size_bwd_deterministic():
    torch.manual_seed(1)
    B, T, D = 32, 1500, 512
    gates = (torch.randn(B, T, 7, D, device=DEV) * 0.5).bfloat16().requires_grad_(True)
    zero = torch.zeros(B, D, device=DEV)
    dout = torch.randn(B, T, D, device=DEV).bfloat16()
    grads = []
    for _ in range(2):
        gates.grad = None
        out, _ = ops().lucy_scan(gates, zero, zero)
        out.backward(dout)
        grads.append(gates.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert torch.isfinite(grads[0].float()).all()
    # every batch row against the oracle's adjoint on the same bf16 gates and dout (gradients
    # stored in bf16: 2^-8 relative, floor 1e-3 of the tensor's scale)
    rg, _, _ = oscan.lucy_scan_bwd(gates.detach().float().cpu().numpy(), np.zeros((B, D)),
                                   np.zeros((B, D)), dout.float().cpu().numpy(), np.zeros((B, D)))
    got = grads[0].float().cpu().numpy()
    sc = np.abs(rg).max()
    print(f"full-size scan bwd, all {B} rows: max |dgates - oracle| / scale "
          f"{np.abs(got - rg).max() / sc:.2e}")
    np.testing.assert_allclose(got, rg, rtol=2.0 ** -7, atol=1e-3 * sc)


def test_decay_scan_vs_reference_triton():
    z = load_golden("decay_scan")
    for name in ["small", "t1"]:
        kv = torch.as_tensor(z[name + "/kv"]).to(DEV)
        dec = torch.as_tensor(z[name + "/decay"]).to(DEV)
        s = ops().decay_scan(kv, dec)
        np.testing.assert_allclose(s.cpu().numpy(), z[name + "/s_all"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("B,T,D", [(2, 1, 5), (3, 130, 70), (4, 1500, 512)])
def test_decay_scan_fwd_bwd_vs_oracle(B, T, D):
    rng = np.random.default_rng(3)
    kv = rng.standard_normal((B, T, D)).astype(np.float32)
    dec = (1 / (1 + np.exp(-rng.standard_normal((B, T, D))))).astype(np.float32)
    init = rng.standard_normal((B, D)).astype(np.float32)
    dout = rng.standard_normal((B, T, D)).astype(np.float32)
    tkv = torch.as_tensor(kv).to(DEV).requires_grad_(True)
    tdec = torch.as_tensor(dec).to(DEV).requires_grad_(True)
    tinit = torch.as_tensor(init).to(DEV).requires_grad_(True)
    s = ops().decay_scan(tkv, tdec, tinit)
    (s * torch.as_tensor(dout).to(DEV)).sum().backward()
    # oracle with init: prepend the init as a step with decay 0
    kv2 = np.concatenate([init[:, None], kv], 1)
    dec2 = np.concatenate([np.zeros((B, 1, D)), dec], 1)
    ref = oscan.decay_scan(kv2, dec2, dtype=np.float64)
    np.testing.assert_allclose(s.detach().cpu().numpy(), ref[:, 1:], rtol=1e-4, atol=1e-4)
    dout2 = np.concatenate([np.zeros((B, 1, D)), dout], 1)
    dkv, ddec = oscan.decay_scan_bwd(dec2, ref, dout2)
    np.testing.assert_allclose(tkv.grad.cpu().numpy(), dkv[:, 1:], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(tdec.grad.cpu().numpy(), ddec[:, 1:], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(tinit.grad.cpu().numpy(), dkv[:, 0], rtol=1e-4, atol=1e-4)


def _blocked(g):
    """[B,T,7,D] -> step-blocked [B,T,D/64,7,64] (include/statecatcher.h)."""
    B, T, _, D = g.shape
    return g.view(B, T, 7, D // 64, 64).permute(0, 1, 3, 2, 4).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_blocked_layout_bitwise_equals_plain(dtype):
    """The step-blocked gate layout (what LucyCellFn's permuted projection writes) gives the
    same bits as the reference layout, forward and backward, with the gate bias on load."""
    torch.manual_seed(5)
    B, T, D = 3, 200, 192
    g = (torch.randn(B, T, 7, D, device=DEV) * 0.6).to(dtype)
    bias = torch.randn(7, D, device=DEV) * 0.2
    h0 = torch.randn(B, D, device=DEV) * 0.3
    s0 = torch.randn(B, D, device=DEV) * 0.3
    dout = torch.randn(B, T, D, device=DEV).to(dtype)
    ds = torch.randn(B, D, device=DEV)
    o = ops()
    _, out1, s1, ck1 = o._scan_fwd(g, h0, s0, True, bias)
    gb = _blocked(g)
    _, out2, s2, ck2 = o._scan_fwd(gb, h0, s0, True, bias)
    assert torch.equal(out1, out2) and torch.equal(s1, s2) and torch.equal(ck1, ck2)
    dg1, dh1, dss1, db1 = o._scan_bwd(g, ck1, dout, ds, True, bias)
    dg2, dh2, dss2, db2 = o._scan_bwd(gb, ck2, dout, ds, True, bias)
    assert dg2.shape == gb.shape
    assert torch.equal(_blocked(dg1), dg2)
    assert torch.equal(dh1, dh2) and torch.equal(dss1, dss2) and torch.equal(db1, db2)


@pytest.mark.parametrize("dtype,D,offset", [(torch.bfloat16, 20, 0), (torch.bfloat16, 64, 1),
                                            (torch.float16, 36, 0), (torch.float32, 64, 1)])
def test_narrow_piece_path_vs_oracle(dtype, D, offset):
    """Gates whose base or strides are not whole 16-byte pieces take the one-element-per-lane
    LDS-DMA path (unaligned slice, D % 8 != 0)."""
    rng = np.random.default_rng(D + offset)
    B, T = 2, 150
    full = torch.as_tensor(rng.standard_normal((B, T, 7, D + offset)).astype(np.float32) * 0.5)
    full = full.to(dtype).to(DEV)
    g = full[..., offset:]
    assert g.stride(3) == 1 and (offset == 0 or g.data_ptr() % 16)
    gr = g.detach().float().cpu().numpy()
    h0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    s0 = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
    dout = rng.standard_normal((B, T, D)).astype(np.float32)
    gg = g
    _, out, s, ck = ops()._scan_fwd(gg, torch.as_tensor(h0).to(DEV), torch.as_tensor(s0).to(DEV), True)
    ro, rs = oscan.lucy_scan_fwd(gr, h0, s0)
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    np.testing.assert_allclose(out.float().cpu().numpy(), ro, rtol=tol, atol=tol)
    np.testing.assert_allclose(s.cpu().numpy(), rs, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(rs).max()))
    dg, dh0g, ds0g, _ = ops()._scan_bwd(gg, ck, torch.as_tensor(dout).to(dtype).to(DEV), None, False)
    rg, _, _ = oscan.lucy_scan_bwd(gr, h0, s0, torch.as_tensor(dout).to(dtype).float().numpy(),
                                   np.zeros((B, D)))
    np.testing.assert_allclose(dg.float().cpu().numpy(), rg, rtol=2 * tol,
                               atol=tol * np.abs(rg).max())
    name = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]
    case = scan_cases.make_case(gr, h0, s0, torch.as_tensor(dout).to(dtype).float().numpy(),
                                np.zeros((B, D)), name)
    if name == "f16":
        scan_cases.assert_fits_f16(scan_cases.reference(case))
    scan_cases.assert_parity(case, {"dgates": dg.float().cpu().numpy(), "dh0": dh0g.cpu().numpy(),
                                    "ds0": ds0g.cpu().numpy(), "out": out.float().cpu().numpy(),
                                    "s_last": s.cpu().numpy()}, label=f"narrow {name} D={D}")
