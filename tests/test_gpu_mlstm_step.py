"""The recurrent mLSTM step kernel (csrc/mlstm_step.hip) on the GPU against the fp64 oracle
(oracle/mlstm.py) through tests/mlstm_step_cases.check_step: every head size x K in {1, 3, 8, 64}
x {zero, carried} state, fp32 and bf16 operands, gates as plain fp32 and read in place from a
[B][K][N] projection with the soft cap in the kernel; K-independence, the live mask and the
hand-over with the chunkwise kernel bitwise / at the oracle's scale; refused arguments.

The fused head-norm epilogue of the issue is not built: ops.gated_head_norm or the
torch chain follows the step, so there is no epilogue test here.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import mlstm_step_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
DTYPES = [torch.float32, torch.bfloat16]


def ops():
    from statecatcher_amd import ops as o
    return o


def dev_state(case):
    return [case[k].to(DEV).contiguous().clone() for k in ("c0", "n0", "m0")]


def run_plain(case, sl=slice(None), state=None, live=None):
    """ops.mlstm_step on steps ``sl`` of the case (capped fp32 gates); returns h and the state
    tensors (advanced in place)."""
    st = dev_state(case) if state is None else state
    q, k, v, ig, fg = (case[x][:, :, sl].to(DEV) for x in ("q", "k", "v", "igate", "fgate"))
    if live is None and case["live"] is not None:
        live = torch.from_numpy(case["live"])[:, sl]
    h = ops().mlstm_step(q, k, v, ig, fg, *st, live=None if live is None else live.to(DEV))
    return h, st


def run_proj(case):
    """sc_mlstm_step reading q / k / v and the RAW gates in place from a [B][K][Np] projection
    (row padded to the kernels' 8-element grid), soft cap 15 inside the kernel."""
    from statecatcher_amd import _lib
    B, NH, K, DQ, DV = case["dims"]
    dt = case["dtype"]
    ko, vo, io = NH * DQ, 2 * NH * DQ, 2 * NH * DQ + NH * DV
    fo = io + NH
    Np = (fo + NH + 7) // 8 * 8
    a = torch.randn(B, K, Np).to(dt)
    a[..., :ko] = case["q"].transpose(1, 2).reshape(B, K, -1)
    a[..., ko:vo] = case["k"].transpose(1, 2).reshape(B, K, -1)
    a[..., vo:io] = case["v"].transpose(1, 2).reshape(B, K, -1)
    a[..., io:fo] = case["iraw"].transpose(1, 2)
    a[..., fo:fo + NH] = case["fraw"].transpose(1, 2)
    a = a.to(DEV)
    st = dev_state(case)
    h = torch.empty(B, NH, K, DV, dtype=dt, device=DEV)
    lay = (ctypes.c_int64 * 7)(NH, K * Np, DQ, Np, K * Np, DV, Np)
    glay = (ctypes.c_int64 * 3)(K * Np, 1, Np)
    esz, base = a.element_size(), a.data_ptr()
    rc = _lib.load().sc_mlstm_step(base, base + ko * esz, base + vo * esz, _lib.dtype_code(a),
                                   base + io * esz, base + fo * esz, glay, 15.0, None,
                                   *[_lib.ptr(t) for t in st], B * NH, K, NH, DQ, DV, 1e-6,
                                   _lib.ptr(h), lay, _lib.stream_of(a))
    _lib.check(rc, "sc_mlstm_step")
    return h, st


def host(h, st):
    torch.cuda.synchronize()
    return [x.float().cpu().numpy() for x in (h, *st)]


@pytest.mark.parametrize("form", ["plain", "proj"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_kernel_against_oracle(DQ, DV, dtype, form):
    worst = {}
    for case in sc.case_set(DQ, DV, dtype):
        h, st = run_plain(case) if form == "plain" else run_proj(case)
        w = sc.check_step(case, *host(h, st), out_unit=sc.U_BF16 if dtype == torch.bfloat16 else 0.0,
                          cap_in_kernel=form == "proj", what=f"{form} {case['key'][:7]}")
        for k, x in w.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"step kernel ({DQ}, {DV}) {dtype} {form}: worst error / allowance {worst}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_k_independence_bitwise(DQ, DV, dtype):
    """One call of K = 8 == 8 calls of K = 1 == calls of 3 + 5, bitwise, in h and the state."""
    case = sc.draw_case(3, 2, 8, DQ, DV, 1, seed=11, dtype=dtype)
    h8, st8 = run_plain(case)
    for split in ([1] * 8, [3, 5]):
        st, hs, t0 = dev_state(case), [], 0
        for n in split:
            hs.append(run_plain(case, slice(t0, t0 + n), st)[0])
            t0 += n
        assert torch.equal(torch.cat(hs, 2), h8), split
        for a, b in zip(st, st8):
            assert torch.equal(a, b), split


LIVE = [[1, 1, 1, 0, 0, 0, 0, 0], [1] * 8, [0] * 8]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_live_mask(DQ, DV, dtype):
    """Held steps leave C, n, m bitwise as they were and return exact zero rows; the live rows
    equal the unmasked run of the compacted sequence bitwise; the whole passes the checker."""
    case = sc.draw_case(3, 2, 8, DQ, DV, 1, seed=13, dtype=dtype, live=LIVE)
    h, st = run_plain(case)
    sc.check_step(case, *host(h, st), out_unit=sc.U_BF16 if dtype == torch.bfloat16 else 0.0)
    live = torch.tensor(LIVE, dtype=torch.bool)
    assert not h.cpu()[~live[:, None, :].expand(3, 2, 8)].any()
    for got, key in zip(st, ("c0", "n0", "m0")):   # stream 2 never moved
        assert torch.equal(got[2].cpu(), case[key][2])
    # stream 0: the state after the masked call == after its 3 live steps alone; stays put after
    ref = sc.draw_case(3, 2, 8, DQ, DV, 1, seed=13, dtype=dtype)
    h3, st3 = run_plain(ref, slice(0, 3))
    assert torch.equal(h3[0], h[0, :, :3]) and torch.equal(h3[1], h[1, :, :3])
    for a, b in zip(st3, st):
        assert torch.equal(a[0], b[0])
    hfull, stfull = run_plain(ref)
    assert torch.equal(hfull[1], h[1])
    for a, b in zip(stfull, st):
        assert torch.equal(a[1], b[1])
    # a mask with holes: the live rows are the compacted sequence's, bitwise
    holes = torch.tensor([[1, 0, 1, 1, 0, 0, 1, 0]] * 3, dtype=torch.float32)
    hm, stm = run_plain(ref, live=holes)
    idx = holes[0].bool()
    comp = dict(ref)
    for k in ("q", "k", "v", "igate", "fgate"):
        comp[k] = ref[k][:, :, idx]
    hc, stc = run_plain(comp)
    assert torch.equal(hm[:, :, idx], hc) and not hm[:, :, ~idx].any()
    for a, b in zip(stm, stc):
        assert torch.equal(a, b)


def _chunk(case, dtype=torch.bfloat16):
    """ops.mlstm_chunkwise (sc_mlstm_fwd) over the case's steps from its carried state."""
    q, k, v = (case[x].to(DEV, dtype) for x in ("q", "k", "v"))
    return ops().mlstm_chunkwise(q, k, v, case["igate"].to(DEV), case["fgate"].to(DEV),
                                 *dev_state(case), return_last_states=True)


@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_handover_from_chunkwise(DQ, DV):
    """sc_mlstm_fwd over T = 64 from a carried state, then 5 steps of the step kernel from the
    state it returns, handed over as it is.  (a) The 5 steps against the oracle started from that
    very state, through the checker: the state convention is shared.  (b) Against the oracle on
    all 69 steps the step rows are as close as the chunk's own rows (the carried error is the
    bf16 MFMA cell's): relative Frobenius error at most 2x the chunk rows' (floor 1e-3)."""
    full = sc.draw_case(2, 2, 69, DQ, DV, 1, seed=17, dtype=torch.bfloat16)
    head = dict(full, dims=(2, 2, 64, DQ, DV))
    for k in ("q", "k", "v", "igate", "fgate"):
        head[k] = full[k][:, :, :64]
    hc, (C, n, m) = _chunk(head)
    st = [C.clone(), n.clone(), m.clone()]
    tail = sc.draw_case(2, 2, 5, DQ, DV, 1, seed=17, dtype=torch.bfloat16)
    for k in ("q", "k", "v", "igate", "fgate"):
        tail[k] = full[k][:, :, 64:]
    tail["c0"], tail["n0"], tail["m0"] = (t.cpu() for t in (C, n, m))
    tail["key"] = ("handover", DQ, DV)
    h5, st5 = run_plain(tail, state=st)
    sc.check_step(tail, *host(h5, st5), out_unit=sc.U_BF16, what="handover tail")
    ref = sc.reference(full)["h"]
    rel = lambda g, r: float(np.linalg.norm(g - r) / np.linalg.norm(r))   # noqa: E731
    e_chunk = rel(hc.float().cpu().numpy(), ref[:, :, :64])
    e_step = rel(h5.float().cpu().numpy(), ref[:, :, 64:])
    print(f"handover ({DQ}, {DV}): chunk rows {e_chunk:.2e}, step rows {e_step:.2e}")
    assert e_step <= max(2 * e_chunk, 1e-3)


@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_64_single_steps_beat_the_chunk_cell(DQ, DV):
    """64 calls of one step against sc_mlstm_fwd's c_last / n / m at T = 64, both rescaled to
    the oracle's m and measured in units of the oracle's absolute sums: the fp32 step's largest
    error does not exceed the bf16 MFMA cell's."""
    case = sc.draw_case(2, 2, 64, DQ, DV, 1, seed=19, dtype=torch.bfloat16)
    r = sc.reference(case)
    _, (C, n, m) = _chunk(case)
    st = dev_state(case)
    for t in range(64):
        run_plain(case, slice(t, t + 1), st)
    torch.cuda.synchronize()
    errs = []
    for Cg, ng, mg in ((C, n, m), st):
        mg = mg.double().cpu().numpy().reshape(2, 2)
        sc_ = np.exp(mg - r["m"])
        eC = np.abs(Cg.double().cpu().numpy() * sc_[..., None, None] - r["C"]) / r["SC"]
        en = np.abs(ng.double().cpu().numpy() * sc_[..., None] - r["n"]) / r["Sn"]
        errs.append(max(float(eC.max()), float(en.max())))
    print(f"({DQ}, {DV}) state error / absolute sum: chunk cell {errs[0]:.2e}, step {errs[1]:.2e}")
    assert errs[1] <= errs[0]


def test_proj_wrapper_in_place_equals_copies():
    """ops.mlstm_step_proj at NH = 4 (N % 8 == 0: the in-place strided reads) equals
    ops.mlstm_step on contiguous copies of the same projection bitwise, with the cap in the
    kernel both ways; at NH = 2 (N % 8 == 4) the wrapper takes the copies itself."""
    o = ops()
    for NH, dtype in ((4, torch.bfloat16), (4, torch.float32), (2, torch.bfloat16)):
        B, K, DQ, DV = 2, 5, 32, 64
        N = 2 * NH * DQ + 2 * NH * DV + 2 * NH
        g = torch.Generator().manual_seed(NH)
        a = torch.randn(B, K, N, generator=g)
        a[..., -2 * NH:] *= 8
        a = a.to(DEV, dtype)
        assert o.mlstm_step_inplace_ok(a, NH, DQ, DV) == (NH == 4)
        z = dict(dtype=torch.float32, device=DEV)
        st = [torch.randn(B, NH, DQ, DV, **z), torch.randn(B, NH, DQ, **z), torch.randn(B, NH, 1, **z)]
        st2 = [t.clone() for t in st]
        h = o.mlstm_step_proj(a, *st, NH, DQ, DV, cap=15.0)
        ko, vo, oo = NH * DQ, 2 * NH * DQ, 2 * NH * DQ + NH * DV
        io = oo + NH * DV
        sp = lambda x, D: x.reshape(B, K, NH, D).transpose(1, 2)   # noqa: E731
        h2 = o.mlstm_step(sp(a[..., :ko], DQ), sp(a[..., ko:vo], DQ), sp(a[..., vo:oo], DV),
                          a[..., io:io + NH].transpose(1, 2), a[..., io + NH:].transpose(1, 2),
                          *st2, cap=15.0)
        assert torch.equal(h, h2)
        for x, y in zip(st, st2):
            assert torch.equal(x, y)
        # with the head norm: ops.gated_head_norm (bf16) / the torch chain on the raw h
        w = torch.randn(NH * DV, generator=g).to(DEV)
        st3 = [t.clone() for t in st2]
        y = o.mlstm_step_proj(a, *st3, NH, DQ, DV, cap=15.0, o_norm=w)
        h3 = o.mlstm_step_proj(a, *st2, NH, DQ, DV, cap=15.0)
        if dtype == torch.bfloat16:
            assert torch.equal(y, o.gated_head_norm(h3, a[..., oo:io], w, 1e-6))
        else:
            hn = torch.nn.functional.layer_norm(h3.transpose(1, 2), (DV,), eps=1e-6)
            ref = torch.sigmoid(a[..., oo:io]) * hn.reshape(B, K, -1) * w
            assert torch.allclose(y, ref, rtol=1e-5, atol=1e-5)


def test_refused_arguments_launch_nothing():
    o = ops()
    from statecatcher_amd import _lib
    assert o.mlstm_step_supported(torch.float32, 96, 192)
    assert o.mlstm_step_supported(torch.bfloat16, 32, 64)
    assert not o.mlstm_step_supported(torch.float16, 32, 64)
    assert not o.mlstm_step_supported(torch.float32, 48, 64)
    B, NH, K, DQ, DV = 2, 2, 4, 32, 64
    z = dict(dtype=torch.float32, device=DEV)
    st = [torch.randn(B, NH, DQ, DV, **z), torch.randn(B, NH, DQ, **z), torch.randn(B, NH, 1, **z)]
    keep = [t.clone() for t in st]
    q, k, v = torch.randn(B, NH, K, DQ, **z), torch.randn(B, NH, K, DQ, **z), torch.randn(B, NH, K, DV, **z)
    ig, fg = torch.randn(B, NH, K, **z), torch.randn(B, NH, K, **z)
    with pytest.raises(ValueError):   # head size not compiled in
        o.mlstm_step(q[..., :24], k[..., :24], v, ig, fg, torch.randn(B, NH, 24, DV, **z),
                     torch.randn(B, NH, 24, **z), st[2])
    with pytest.raises(TypeError):    # f16 operands
        o.mlstm_step(q.half(), k.half(), v.half(), ig, fg, *st)
    with pytest.raises(ValueError):   # the state is updated in place: no silent cast
        o.mlstm_step(q, k, v, ig, fg, st[0].double(), st[1], st[2])
    h = torch.empty(B, NH, K, DV, **z)
    args = lambda lay, dt=_lib.SC_F32, dq=DQ: (   # noqa: E731
        _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), dt, _lib.ptr(ig), _lib.ptr(fg), None, 0.0, None,
        *[_lib.ptr(t) for t in st], B * NH, K, NH, dq, DV, 1e-6, _lib.ptr(h), lay, _lib.stream_of(q))
    lib = _lib.load()
    bad_stride = (ctypes.c_int64 * 7)(NH, NH * K * DQ, K * DQ, DQ + 4, NH * K * DV, K * DV, DV)
    wrong_nh = (ctypes.c_int64 * 7)(1, NH * K * DQ, K * DQ, DQ, NH * K * DV, K * DV, DV)
    for a in (args(bad_stride), args(wrong_nh), args(None, _lib.SC_F16), args(None, dq=48)):
        assert lib.sc_mlstm_step(*a) == _lib.SC_EINVAL
        assert b"sc_mlstm_step" in lib.sc_last_error()
    torch.cuda.synchronize()
    for a, b in zip(st, keep):
        assert torch.equal(a, b)
    # K == 0 and BH == 0 are no-ops
    assert o.mlstm_step(q[:, :, :0], k[:, :, :0], v[:, :, :0], ig[..., :0], fg[..., :0], *st).shape == (B, NH, 0, DV)
    for a, b in zip(st, keep):
        assert torch.equal(a, b)
