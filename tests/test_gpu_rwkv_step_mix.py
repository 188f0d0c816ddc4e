"""The RWKV shift-mix kernel (csrc/rwkv_step.hip, ops.rwkv_step_mix) and the squared ReLU on the GPU
against the same steps in float64 torch: the residual prologue (h += add, h += sigmoid(gate) *
add), pre_ln, LayerNorm, the time shift through held frames, the mixes and the carried x_prev, at
B = 3, H in {64, 96} (96: a half-filled second wave), K in {1, 4}, nmix in {0, 2, 3}.

Bound per tensor: max |got - ref64| <= 8 d32 + 1e-5 scale, d32 the float32 run of the same torch
steps against their float64 run and scale = max |ref64| (tests/test_gpu_rwkv.py::within).  With
bf16 operands the outputs add 2^-8 |ref64| elementwise for their rounding on store.  Output rows
of held frames are not compared (they must be finite).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
B, EPS = 3, 1e-5
# stream 0: first frame held; stream 1: a hole inside the block; stream 2: every frame held
MASKS = {1: [[0.0], [1.0], [0.0]],
         4: [[0.0, 1.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]]}


def ops():
    from statecatcher_amd import ops as o
    return o


def make(H, K, nmix, pre, prologue, seed=0):
    g = torch.Generator().manual_seed(100 * seed + H + 7 * K + nmix)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    c = dict(h=rn(B, K, H) * 2.0 + 0.3, ln=(1.0 + 0.1 * rn(H), 0.1 * rn(H)), x_prev=rn(B, H),
             mixes=tuple(torch.rand(H, generator=g) for _ in range(nmix)),
             pre=(1.0 + 0.1 * rn(H), 0.1 * rn(H)) if pre else None,
             add=rn(B, K, H) if prologue != "none" else None,
             gate=rn(B, K, H) * 2.0 if prologue == "gate" else None,
             live=torch.tensor(MASKS[K]))
    return c


def mix_ref(c, dtype):
    """(h after, a, outs, x_prev after) of the kernel's steps in plain torch, in ``dtype``."""
    t = lambda x: None if x is None else x.to(dtype)   # noqa: E731
    h, H = t(c["h"]).clone(), c["h"].shape[-1]
    if c["add"] is not None:
        h = h + (torch.sigmoid(t(c["gate"])) * t(c["add"]) if c["gate"] is not None else t(c["add"]))
    if c["pre"] is not None:
        h = F.layer_norm(h, (H,), t(c["pre"][0]), t(c["pre"][1]), EPS)
    a = F.layer_norm(h, (H,), t(c["ln"][0]), t(c["ln"][1]), EPS)
    s = t(c["x_prev"]).clone()
    outs = [torch.zeros_like(a) for _ in c["mixes"]]
    for k in range(a.shape[1]):
        for o, m in zip(outs, c["mixes"]):
            o[:, k] = a[:, k] * t(m) + s * (1 - t(m))
        on = c["live"][:, k].bool()
        s = torch.where(on[:, None], a[:, k], s)
    return h, a, (outs if c["mixes"] else [a]), s


def run(c, dtype=torch.float32, steps=None):
    """(h after, outs, x_prev after) of ops.rwkv_step_mix; steps: in calls of that many frames."""
    o = ops()
    d = lambda x, dt=torch.float32: None if x is None else x.to(DEV, dt)   # noqa: E731
    K, H = c["h"].shape[1:]
    h, xp, live = d(c["h"]).clone(), d(c["x_prev"]).clone(), d(c["live"])
    add, gate = d(c["add"], dtype), d(c["gate"], dtype)
    ln, pre = tuple(d(p) for p in c["ln"]), None if c["pre"] is None else tuple(d(p) for p in c["pre"])
    mixes = tuple(d(m) for m in c["mixes"])
    outs = [torch.full((B, K, H), float("nan"), dtype=dtype, device=DEV)
            for _ in range(max(len(mixes), 1))]
    n = K if steps is None else steps
    for t0 in range(0, K, n):
        sl = slice(t0, t0 + n)
        got = o.rwkv_step_mix(h[:, sl], ln, xp, mixes, [x[:, sl] for x in outs],
                              add=None if add is None else add[:, sl],
                              gate=None if gate is None else gate[:, sl], pre_ln=pre,
                              live=live[:, sl], eps=EPS)
        assert [g.data_ptr() for g in got] == [x[:, sl].data_ptr() for x in outs]
    return h, outs, xp


def within(name, got, r64, r32, rows=None, bf16=False):
    got, r64, r32 = (x.double().cpu() for x in (got, r64, r32))
    d32, scale = float((r32 - r64).abs().max()), float(r64.abs().max())
    err = (got - r64).abs()
    lim = torch.full_like(r64, 8 * d32 + 1e-5 * scale) + (2.0 ** -8 * r64.abs() if bf16 else 0.0)
    if rows is not None:
        err, lim = err[rows], lim[rows]
    ratio = float((err / lim).max()) if err.numel() else 0.0
    print(f"{name}: err {float(err.max()) if err.numel() else 0.0:.3e} d32 {d32:.3e} "
          f"scale {scale:.3e} ratio {ratio:.3f}")
    assert bool((err <= lim).all()), (name, ratio)


@pytest.mark.parametrize("prologue", ["none", "add", "gate"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre_ln"])
@pytest.mark.parametrize("nmix", [0, 2, 3])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("H", [64, 96])
def test_parity_and_carried_frame(H, K, nmix, pre, prologue):
    c = make(H, K, nmix, pre, prologue)
    r64, r32 = mix_ref(c, torch.float64), mix_ref(c, torch.float32)
    h, outs, xp = run(c)
    live = c["live"].bool()
    assert all(torch.isfinite(x).all() for x in (h, xp, *outs))
    tag = f"H={H} K={K} nmix={nmix} pre={pre} {prologue}"
    within(f"{tag} h", h, r64[0], r32[0], rows=live)
    for i, (g, a, b) in enumerate(zip(outs, r64[2], r32[2])):
        within(f"{tag} out{i}", g, a, b, rows=live)
    # x_prev: the last live a, and bitwise what it was where nothing was live
    within(f"{tag} x_prev", xp, r64[3], r32[3])
    idle = ~live.any(1)
    assert idle.any() and torch.equal(xp.cpu()[idle], c["x_prev"][idle])
    if prologue == "none" and not pre:
        assert torch.equal(h.cpu(), c["h"])   # nothing to write back: the residual row is read only


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nmix", [0, 3])
@pytest.mark.parametrize("H", [64, 96])
def test_k_frames_in_one_call_equal_k_calls_bitwise(H, nmix, dtype):
    for pre, prologue in ((True, "gate"), (False, "add"), (False, "none")):
        c = make(H, 4, nmix, pre, prologue, seed=1)
        h4, o4, x4 = run(c, dtype)
        for steps in (1, 2):
            h1, o1, x1 = run(c, dtype, steps=steps)
            assert torch.equal(h4, h1) and torch.equal(x4, x1)
            assert all(torch.equal(a, b) for a, b in zip(o4, o1))
        h4b, o4b, x4b = run(c, dtype)   # and two runs agree
        assert torch.equal(h4, h4b) and torch.equal(x4, x4b)
        assert all(torch.equal(a, b) for a, b in zip(o4, o4b))


@pytest.mark.parametrize("H", [64, 96, 2048, 1000])
def test_bf16_operands_and_wide_rows(H):
    """add / gate / outs in bf16 (the library engine's activations), and the row widths that take
    the kernel's other register tilings (1000: 4 elements per thread with a ragged tail; 2048: 8)."""
    c = make(H, 4, 3, True, "gate", seed=2)
    c["add"], c["gate"] = c["add"].bfloat16().float(), c["gate"].bfloat16().float()
    r64, r32 = mix_ref(c, torch.float64), mix_ref(c, torch.float32)
    h, outs, xp = run(c, torch.bfloat16)
    live = c["live"].bool()
    within(f"bf16 H={H} h", h, r64[0], r32[0], rows=live)
    for i, (g, a, b) in enumerate(zip(outs, r64[2], r32[2])):
        assert g.dtype == torch.bfloat16
        within(f"bf16 H={H} out{i}", g, a, b, rows=live, bf16=True)
    within(f"bf16 H={H} x_prev", xp, r64[3], r32[3])


def test_refusals_and_strided_layout():
    o = ops()
    c = make(96, 4, 2, False, "add", seed=3)
    h, outs, xp = run(c)
    # the encoder's layout: [K,B,H] buffers seen as [B,K,H]
    kb = lambda x: x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)   # noqa: E731
    h2, add, xp2 = kb(c["h"]), kb(c["add"]), c["x_prev"].to(DEV).clone()
    ln, mixes = tuple(p.to(DEV) for p in c["ln"]), tuple(m.to(DEV) for m in c["mixes"])
    live_kb = c["live"].to(DEV).t().contiguous()
    got = o.rwkv_step_mix(h2, ln, xp2, mixes, None, add=add, live=live_kb.t(), eps=EPS)
    assert torch.equal(h2, h) and torch.equal(xp2, xp)
    assert all(torch.equal(a, b) for a, b in zip(got, outs))
    with pytest.raises(ValueError, match="need x_prev"):
        o.rwkv_step_mix(h2, ln, None, mixes)
    with pytest.raises(ValueError, match="contiguous fp32"):
        o.rwkv_step_mix(h2, ln, xp2.double(), mixes)
    with pytest.raises(ValueError, match="gate without add"):
        o.rwkv_step_mix(h2, ln, xp2, mixes, gate=add)
    with pytest.raises(TypeError, match="h must be fp32"):
        o.rwkv_step_mix(h2.bfloat16(), ln, xp2, mixes)
    with pytest.raises(ValueError, match="outside \\[1, 2048\\]"):
        wide = torch.zeros(1, 1, 2056, device=DEV)
        o.rwkv_step_mix(wide, (wide[0, 0], wide[0, 0]), None, ())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 3 * 264 + 5])
def test_relu_sq(n, dtype):
    o = ops()
    g = torch.Generator().manual_seed(n)
    x = (3.0 * torch.randn(n + 3, generator=g)).to(dtype)
    for off in (0, 1):   # a 16-byte aligned base and one that is not
        buf = x.to(DEV).clone()
        view = buf[off:off + n]
        assert o.relu_sq_(view) is view
        want = torch.square(torch.relu(x[off:off + n].float())).to(dtype)   # one rounding on store
        assert torch.equal(view.cpu(), want)
        assert torch.equal(buf.cpu()[:off], x[:off]) and torch.equal(buf.cpu()[off + n:], x[off + n:])
    with pytest.raises(ValueError, match="contiguous"):
        o.relu_sq_(torch.zeros(4, 4, device=DEV).t())
