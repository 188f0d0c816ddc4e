"""The masked LucyRNN scan kernels (sc_lucy_scan_fwd_masked / sc_lucy_scan_bwd_masked) against the
fp64 oracle on each row's live frames (tests/scan_mask_cases.py: the definition, the cases and
the checker; no tolerance beyond scan_cases.C), and the properties the semantics fix exactly:
zeros at held frames, pass-through of an all-held row, bitwise equality with the unmasked entry
points on an all-live mask, and indifference to whatever a held frame's gates and dout hold."""
import numpy as np
import pytest
import torch

from tests import scan_cases as sc
from tests import scan_mask_cases as mc
from tests.test_gpu_scan_parity import _np, _unblocked, device_gates

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
KEYS = ("out", "s_last", "h_last", "dgates", "dh0", "ds0", "dbias")


def ops():
    from statecatcher_amd import ops as o
    return o


def _poisoned(case, mask):
    """The case with NaN in the gates and dout of every held frame."""
    held = ~mask.astype(bool)
    p = dict(case, gates=case["gates"].copy(), dout=case["dout"].copy())
    p["gates"][held] = np.nan
    p["dout"][held] = np.nan
    return p


def run_masked(case, mask, dh_last, blocked=False, offset=0, split=False, raw=False):
    """Forward and backward through the C ABI with the mask (None: the unmasked entry points).
    raw: the device tensors as they are (bitwise comparisons), else fp32 numpy."""
    dt = sc.TORCH_DTYPE[case["dtype"]]
    g = device_gates(case, blocked, offset)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    bias = dev(case["bias"]) if "bias" in case else None
    B, T = case["gates"].shape[:2]
    mk = None if mask is None else ops().scan_mask(dev(mask), B, T, DEV)
    res = ops()._scan_fwd(g, dev(case["h0"]), dev(case["s0"]), True, bias, want_h=True, split=split,
                          mask=mk)
    g, out, s_last, ckpt, h_last = res[:5]
    dg, dh0, ds0, dbias = ops()._scan_bwd(g, ckpt, dev(case["dout"]).to(dt), dev(case["ds_last"]),
                                          True, bias, mask=mk,
                                          dh_last=None if dh_last is None else dev(dh_last))
    assert dg.dtype == dt and out.dtype == dt and h_last.dtype == torch.float32
    got = dict(zip(KEYS, (out, s_last, h_last, _unblocked(dg) if blocked else dg, dh0, ds0, dbias)))
    if split:
        got["wide"] = res[5]
    torch.cuda.synchronize()
    return got if raw else {k: _np(v) for k, v in got.items()}


def _setup(T, D, dtype, name, bias=False):
    case = mc.base_case(T, D, dtype, bias=bias)
    dh_last, masks = mc.draw_extras(T, D, dtype)
    return case, masks[name], dh_last


PARITY = [(T, D, n, d) for T, D in mc.SHAPES for n in mc.MASKS for d in ("f32", "bf16")]
PARITY.append((130, 72, "prefix", "f16"))


@pytest.mark.parametrize("T,D,name,dtype", PARITY)
def test_masked_scan_vs_fp64(T, D, name, dtype):
    """Every live row passes scan_cases.check for out, s_last, dgates, dh0, ds0, dbias and h_last
    the out rule of its last live step; out and dgates at held frames are exactly 0; a row with no
    live frame returns (h0, s0), dh0 = dh_last, ds0 = ds_last exactly and a zero dbias."""
    case, mask, dh_last = _setup(T, D, dtype, name)
    if dtype == "f16":
        for b in range(mc.B):
            rc = mc.row_case(case, mask, dh_last, b, name)
            if rc is not None:
                sc.assert_fits_f16(sc.reference(rc))
    got = run_masked(case, mask, dh_last)
    assert all(np.isfinite(v).all() for v in got.values())
    mc.assert_rows(case, mask, dh_last, got, name)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("T,D", mc.SHAPES)
def test_all_live_is_bitwise_the_unmasked_scan(T, D, dtype):
    """An all-live mask takes the unmasked kernels' FULL / guarded bodies: every output bitwise
    equal to the unmasked entry points', with dh_last joined onto dout[:, -1] the old way for
    both (ops._join_dh_last)."""
    case, mask, dh_last = _setup(T, D, dtype, "all_live")
    dt = sc.TORCH_DTYPE[dtype]
    dout = torch.as_tensor(case["dout"]).to(dt)
    dout[:, -1] += torch.as_tensor(dh_last).to(dt)
    joined = dict(case, dout=dout.float().numpy())
    plain = run_masked(joined, None, None, raw=True)
    masked = run_masked(joined, mask, None, raw=True)
    for k in KEYS:
        assert torch.equal(plain[k], masked[k]), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("T,D,name", [(130, 72, "holes"), (130, 64, "random"), (65, 72, "prefix"),
                                      (5, 64, "holes")])
def test_held_gates_and_dout_never_read_into_a_result(T, D, name, dtype):
    """NaN in the gates and dout of every held frame: every result bitwise as without it."""
    case, mask, dh_last = _setup(T, D, dtype, name)
    assert not mask.all()
    clean = run_masked(case, mask, dh_last, raw=True)
    dirty = run_masked(_poisoned(case, mask), mask, dh_last, raw=True)
    for k in KEYS:
        assert torch.isfinite(dirty[k].float()).all(), k
        assert torch.equal(clean[k], dirty[k]), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_blocked_layout_with_bias_on_load(dtype):
    case, mask, dh_last = _setup(130, 64, dtype, "random", bias=True)
    got = run_masked(_poisoned(case, mask), mask, dh_last, blocked=True)
    mc.assert_rows(case, mask, dh_last, got, "random", label=f"blocked + bias {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unaligned_base_one_element_pieces(dtype):
    case, mask, dh_last = _setup(130, 64, dtype, "random")
    got = run_masked(_poisoned(case, mask), mask, dh_last, offset=1)
    mc.assert_rows(case, mask, dh_last, got, "random", label=f"unaligned {dtype}")


@pytest.mark.parametrize("D,offset", [(72, 0), (64, 1)])
def test_split_forward_masked(D, offset):
    """The split planes under a mask, on 16-byte pieces with a partial block (D = 72) and on
    one-element pieces (D = 64 from an unaligned slice): out and out_dup are the plain masked
    out, hi + lo carries h to 2^-15 relative on top of the fp32 recurrence's own distance from
    fp64 (test_split_forward_vs_fp64's bound), and all three planes are zero at held frames."""
    T, name = 130, "holes"
    case, mask, dh_last = _setup(T, D, "bf16", name)
    plain = run_masked(case, mask, dh_last, offset=offset, raw=True)
    got = run_masked(_poisoned(case, mask), mask, dh_last, offset=offset, split=True, raw=True)
    wide = got["wide"]
    for k in KEYS:
        assert torch.equal(plain[k], got[k]), k
    assert torch.equal(wide[..., :D], got["out"]) and torch.equal(wide[..., D:2 * D], got["out"])
    held = torch.as_tensor(~mask).to(DEV)
    assert held.any() and not wide[held].any()
    hs = _np(got["out"]).astype(np.float64) + _np(wide[..., 2 * D:])
    for b in range(mc.B):
        idx = np.nonzero(mask[b])[0]
        ref = sc.reference(mc.row_case(case, mask, dh_last, b, name))
        noise = np.abs(ref["out32"] - ref["out"]).max()
        err = np.abs(hs[b, idx] - ref["out"][0])
        bound = 2.0 ** -15 * np.maximum(np.abs(ref["out"][0]), 1e-3) + 4 * noise
        print(f"split masked D={D} row {b}: max |hi + lo - h64| / bound {(err / bound).max():.2f}")
        assert (err <= bound).all()


# ------------------------------------------------------------------------- dispatcher ops ---
def _tl():
    from statecatcher_amd import torch_library as tl
    tl.load()
    return tl


def _leaves(case, mask, dtype):
    dt = sc.TORCH_DTYPE[dtype]
    dev = lambda a: torch.as_tensor(a).to(DEV)
    return (dev(case["gates"]).to(dt).requires_grad_(), dev(case["h0"]).requires_grad_(),
            dev(case["s0"]).requires_grad_(), dev(mask))


def _loss(out, s_last, h_last, case, dh_last):
    dev = lambda a: torch.as_tensor(a).to(DEV)
    return ((out.float() * dev(case["dout"])).sum() + (s_last * dev(case["ds_last"])).sum()
            + (h_last * dev(dh_last)).sum())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dispatcher_ops_bitwise_vs_ctypes_nodes(dtype):
    """torch.ops.statecatcher.lucy_scan_masked_fwd / _bwd launch the kernels ops.lucy_scan(mask=)
    launches: outputs and the gradients of gates, h0 and s0 bitwise equal, and both equal the
    C-ABI run that test_masked_scan_vs_fp64 checks against fp64."""
    case, mask, dh_last = _setup(130, 72, dtype, "random")
    outs = []
    for fn in (_tl().lucy_scan_masked, ops().lucy_scan):
        g, h0, s0, mk = _leaves(case, mask, dtype)
        out, s_last, h_last = fn(g, h0, s0, mk)
        _loss(out, s_last, h_last, case, dh_last).backward()
        outs.append((out, s_last, h_last, g.grad, h0.grad, s0.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    abi = run_masked(case, mask, dh_last, raw=True)
    for k, v in zip(("out", "s_last", "h_last", "dgates", "dh0", "ds0"), outs[0]):
        assert torch.equal(abi[k], v), k
    # a float mask and an integer one are the bool one
    g, h0, s0, mk = _leaves(case, mask, dtype)
    for m2 in (mk.float() * 0.5, mk.int() * 3):
        o2, s2, h2 = ops().lucy_scan(g, h0, s0, m2)
        assert torch.equal(o2, outs[0][0]) and torch.equal(h2, outs[0][2])
    with pytest.raises(ValueError):
        ops().lucy_scan(g, h0, s0, mk[:, :-1])
    with pytest.raises(ValueError):
        ops().lucy_scan(g, h0, s0, mk.cpu())


def test_dispatcher_ops_opcheck_and_compile():
    tl = _tl()
    scn = torch.ops.statecatcher
    case, mask, dh_last = _setup(65, 72, "f32", "holes")
    g, h0, s0, mk = _leaves(case, mask, "f32")
    torch.library.opcheck(scn.lucy_scan_masked_fwd.default, (g, h0, s0, mk, None, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    _, _, _, ckpt = scn.lucy_scan_masked_fwd(g.detach(), h0.detach(), s0.detach(), mk, None, True)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    torch.library.opcheck(scn.lucy_scan_masked_bwd.default,
                          (g.detach(), ckpt, dev(case["dout"]), mk, dev(case["ds_last"]),
                           dev(dh_last), None, True), test_utils=("test_schema", "test_faketensor"))

    def f(g, h0, s0):
        out, s_last, h_last = tl.lucy_scan_masked(g, h0, s0, mk)
        return _loss(out, s_last, h_last, case, dh_last)

    def run(fn):
        leaves = _leaves(case, mask, "f32")[:3]
        loss = fn(*leaves)
        loss.backward()
        return [loss.detach()] + [t.grad for t in leaves]

    torch._dynamo.reset()
    eager = run(f)
    compiled = run(torch.compile(f, fullgraph=True, backend="aot_eager"))
    for a, b in zip(eager, compiled):
        assert torch.equal(a, b)
