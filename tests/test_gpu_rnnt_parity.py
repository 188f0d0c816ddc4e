"""GPU parity of the dense RNN-T loss (csrc/rnnt.hip: rnnt_emit, rnnt_shift, rnnt_ab<K>, rnnt_grad)
with the fp64 oracle on every path its kernels take, element by element at the scale of each arc
(tests/rnnt_cases.py: the rule, the measured constants and the case map; tests/test_rnnt_checker.py
judges the checker itself on the CPU)."""
import numpy as np
import pytest
import torch

from tests import rnnt_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def ops():
    from statecatcher_amd import ops as o
    return o


def _device_input(case):
    """The case's x on the device as a leaf: dense, compact rows, or one element off 16 bytes."""
    dt = rc.TORCH_DTYPE[case["dtype"]]
    x = torch.as_tensor(case["x"]).to(dt)
    if case["compact"]:
        x = torch.cat([x[b, :int(t), :int(u) + 1].reshape(-1, x.shape[-1])
                       for b, (t, u) in enumerate(zip(case["fl"], case["ll"]))])
    if case["misaligned"]:
        buf = torch.empty(x.numel() + 1, dtype=dt, device=DEV)
        buf[1:].copy_(x.reshape(-1))
        xt = buf[1:].view(x.shape).detach()
        assert xt.data_ptr() % 16 != 0
    else:
        xt = x.to(DEV)
    return xt.requires_grad_(True)


def _dense(case, g):
    """A compact gradient back in the dense layout (padding rows do not exist there: zeros)."""
    if not case["compact"]:
        return g
    out = np.zeros(case["x"].shape, g.dtype)
    r = 0
    for b, (t, u) in enumerate(zip(case["fl"], case["ll"])):
        n = int(t) * (int(u) + 1)
        out[b, :int(t), :int(u) + 1] = g[r:r + n].reshape(int(t), int(u) + 1, -1)
        r += n
    assert r == g.shape[0]
    return out


def run(case):
    xt = _device_input(case)
    args = (torch.as_tensor(case["labels"]).to(DEV), torch.as_tensor(case["fl"]).to(DEV),
            torch.as_tensor(case["ll"]).to(DEV))
    nll = ops().rnnt_loss(xt, *args, reduction="none", blank=case["blank"],
                          is_logits=case["logits"], compact=case["compact"])
    (nll * torch.as_tensor(case["w"]).to(DEV)).sum().backward()
    assert xt.grad.dtype == xt.dtype
    return {"nll": nll.detach().cpu().numpy(),
            "grad": _dense(case, xt.grad.float().cpu().numpy())}


def run_grad32(case):
    """16-bit input, fp32 gradient: the C ABI's grad_dtype (launch_bwd<16-bit, fp32>)."""
    from statecatcher_amd import _lib
    from statecatcher_amd._lib import check, dtype_code, ptr, stream_of
    lib = _lib.load()
    x = torch.as_tensor(case["x"]).to(rc.TORCH_DTYPE[case["dtype"]]).to(DEV)
    B, T, U1, V = x.shape
    labels = torch.as_tensor(case["labels"]).to(DEV)
    fl, ll = torch.as_tensor(case["fl"]).to(DEV), torch.as_tensor(case["ll"]).to(DEV)
    scale = torch.as_tensor(case["w"]).to(DEV)
    nll = torch.empty(B, dtype=torch.float32, device=DEV)
    grad = torch.full(x.shape, float("nan"), dtype=torch.float32, device=DEV)
    wsb = lib.sc_rnnt_workspace_bytes(B, T, U1 - 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    lay = (B, T, U1 - 1, V, x.stride(0), x.stride(1), x.stride(2), None, ptr(labels),
           labels.stride(0), ptr(fl), ptr(ll), case["blank"])
    check(lib.sc_rnnt_fwd(ptr(x), dtype_code(x), int(case["logits"]), *lay, ptr(nll), ptr(ws), wsb,
                          stream_of(x)), "sc_rnnt_fwd")
    check(lib.sc_rnnt_bwd(ptr(x), dtype_code(x), int(case["logits"]), *lay, ptr(scale), ptr(grad),
                          dtype_code(grad), ptr(ws), wsb, stream_of(x)), "sc_rnnt_bwd")
    torch.cuda.synchronize()
    return {"nll": nll.cpu().numpy(), "grad": grad.cpu().numpy()}


# ---- halo widths and waves: K = 16, 8, 4, 2, 1; 1 .. 16 waves ----------------------------------
@pytest.mark.parametrize("umax", rc.HALO_UMAX)
def test_halo_widths_and_waves(umax):
    case = rc.halo_case(umax)
    print(f"Umax {umax}: K {rc.ab_halo_k(umax)}, {rc.ab_waves(umax)} waves, ragged U {case['ll'][1]}")
    rc.assert_parity(case, run(case))


def test_too_many_labels_are_rejected():
    x = torch.zeros(1, 2, 1009, 4, device=DEV)
    with pytest.raises(ValueError, match="max label count 1008 exceeds 1007"):
        ops().rnnt_loss(x, torch.ones(1, 1008, dtype=torch.int64, device=DEV), [2], [1008],
                        is_logits=True)


# ---- diagonal counts across the 16-diagonal pipeline blocks and the 32-diagonal re-centring ----
@pytest.mark.parametrize("nd", rc.DIAG_ND)
def test_diagonal_counts(nd):
    case = rc.diag_case(nd)
    print(f"Tb + Ub = {list(case['fl'] + case['ll'])}")
    rc.assert_parity(case, run(case))


@pytest.mark.parametrize("T", rc.U0_T)
def test_no_labels(T):
    case = rc.u0_case(T)
    rc.assert_parity(case, run(case))


@pytest.mark.parametrize("U", rc.T1_U)
def test_one_frame(U):
    case = rc.t1_case(U)
    rc.assert_parity(case, run(case))


# ---- row paths: 16-byte vectors (nvec 1 .. 4 of either element size) and the scalar loop -------
ROW_CASES = list(rc.row_cases())


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "-".join(str(k) for k in c["key"][1:]))
def test_row_paths(case):
    V = case["x"].shape[-1]
    print(f"V {V} {case['dtype']}: nvec {rc.row_nvec(V, case['dtype'], not case['misaligned'])}")
    rc.assert_parity(case, run(case))


# ---- dtypes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_dtypes_through_autograd(dtype):
    case = rc.dtype_case(dtype)
    rc.assert_parity(case, run(case))


@pytest.mark.parametrize("V", [512, 24])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fp32_gradient_of_16bit_logits(dtype, V):
    case = rc.gradtype_case(dtype, V)
    rc.assert_parity(case, run_grad32(case))


# ---- sharp and masked emissions ----------------------------------------------------------------
@pytest.mark.parametrize("gain,T,U", rc.SHARP)
def test_sharp_logits(gain, T, U):
    case = rc.sharp_case(gain, T, U)
    rc.assert_parity(case, run(case))


@pytest.mark.parametrize("logits", [False, True], ids=["logprobs", "logits"])
@pytest.mark.parametrize("kind", rc.MASKS)
def test_masked_emissions(kind, logits):
    """-inf log-probs / logits: unused columns, single arcs with paths left, and every path of
    sequence 1 blocked: nll = +inf, that sequence's gradient exactly zero, neighbours untouched."""
    case = rc.masked_case(kind, logits)
    got = run(case)
    print(f"masked {kind} logits={logits}: nll {got['nll']}, |grad| of sequence 1 "
          f"{np.abs(got['grad'][1]).max():.3e}")
    rc.assert_parity(case, got)
    if kind in ("final_blank", "label_column"):
        assert np.isposinf(got["nll"][1]) and not got["grad"][1].any()
        assert np.isfinite(got["nll"][[0, 2]]).all() and got["grad"][0].any() and got["grad"][2].any()


# ---- strided dense input -----------------------------------------------------------------------
def test_strided_view_forward_equals_contiguous():
    """A [B,T,U+1,V] view of a buffer padded in t and u: the forward reads it in place; the
    backward's documented RuntimeError stays."""
    case = rc.dtype_case("f32")
    x = torch.as_tensor(case["x"]).to(DEV)
    B, T, U1, V = x.shape
    big = torch.full((B, T + 3, U1 + 2, V), float("nan"), device=DEV)
    big[:, :T, :U1] = x
    view = big[:, :T, :U1].requires_grad_(True)
    assert not view.is_contiguous()
    args = (torch.as_tensor(case["labels"]).to(DEV), torch.as_tensor(case["fl"]).to(DEV),
            torch.as_tensor(case["ll"]).to(DEV))
    nll_v = ops().rnnt_loss(view, *args, reduction="none", is_logits=True)
    nll_c = ops().rnnt_loss(x, *args, reduction="none", is_logits=True)
    assert torch.equal(nll_v, nll_c)
    rc.assert_parity(case, {"nll": nll_v.detach().cpu().numpy()})
    with pytest.raises(RuntimeError, match="rnnt backward expects a contiguous input"):
        nll_v.sum().backward()


# ---- determinism -------------------------------------------------------------------------------
def test_deterministic():
    case = rc.mid_case()
    a, b = run(case), run(case)
    assert np.array_equal(a["nll"], b["nll"]) and np.array_equal(a["grad"], b["grad"])
    rc.assert_parity(case, a)
