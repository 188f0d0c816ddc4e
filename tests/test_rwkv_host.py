"""CPU checks of the RWKV encoder's host side: parameter names against transformers', the
initialisation formulas, the state helpers, the ASRModel wiring, and the WKV entry points at
every layer (C ABI argument validation, dispatcher schemas / Meta kernels / autograd trace,
refusal of CPU tensors and of a state that requires grad)."""
import ctypes
import math

import pytest
import torch
from torch.fx.experimental.proxy_tensor import make_fx

import statecatcher_amd as sc
from statecatcher_amd import _lib, ops
from statecatcher_amd import torch_library as tl
from statecatcher_amd.rwkv import EMPTY_MAX, RWKVConfig, RWKVEncoder

META = torch.device("meta")

# transformers.models.rwkv.modeling_rwkv.RwkvModel(num_hidden_layers=2).blocks.state_dict() keys
HF_BLOCK_KEYS = [
    "0.pre_ln.weight", "0.pre_ln.bias", "0.ln1.weight", "0.ln1.bias", "0.ln2.weight", "0.ln2.bias",
    "0.attention.time_decay", "0.attention.time_first", "0.attention.time_mix_key",
    "0.attention.time_mix_value", "0.attention.time_mix_receptance", "0.attention.key.weight",
    "0.attention.value.weight", "0.attention.receptance.weight", "0.attention.output.weight",
    "0.feed_forward.time_mix_key", "0.feed_forward.time_mix_receptance",
    "0.feed_forward.key.weight", "0.feed_forward.receptance.weight", "0.feed_forward.value.weight",
    "1.ln1.weight", "1.ln1.bias", "1.ln2.weight", "1.ln2.bias",
    "1.attention.time_decay", "1.attention.time_first", "1.attention.time_mix_key",
    "1.attention.time_mix_value", "1.attention.time_mix_receptance", "1.attention.key.weight",
    "1.attention.value.weight", "1.attention.receptance.weight", "1.attention.output.weight",
    "1.feed_forward.time_mix_key", "1.feed_forward.time_mix_receptance",
    "1.feed_forward.key.weight", "1.feed_forward.receptance.weight", "1.feed_forward.value.weight",
]


def _enc(L=2, H=32, A=None, I=64, V=11, F=8):
    return RWKVEncoder(RWKVConfig(input_dim=F, hidden_size=H, num_layers=L, vocab_size=V,
                                  attention_hidden_size=A, intermediate_size=I))


def test_block_parameter_names_are_transformers():
    enc = _enc()
    assert list(enc.blocks.state_dict().keys()) == HF_BLOCK_KEYS
    sd = enc.state_dict()
    assert sd["blocks.0.attention.time_decay"].shape == (32,)
    assert sd["blocks.0.attention.time_mix_key"].shape == (1, 1, 32)
    assert sd["blocks.1.feed_forward.key.weight"].shape == (64, 32)
    assert sd["input_proj.weight"].shape == (32, 8) and sd["output_proj.weight"].shape == (11, 32)
    assert sd["ln_out.weight"].shape == (32,)
    assert _enc(I=None).state_dict()["blocks.0.feed_forward.key.weight"].shape == (128, 32)
    assert _enc(A=16).state_dict()["blocks.0.attention.output.weight"].shape == (32, 16)


def test_block_names_match_transformers_live():
    tr = pytest.importorskip("transformers")
    cfg = tr.RwkvConfig(vocab_size=16, hidden_size=32, attention_hidden_size=32,
                        intermediate_size=64, num_hidden_layers=2)
    hf = tr.RwkvModel(cfg)
    sd = hf.blocks.state_dict()
    assert list(sd.keys()) == HF_BLOCK_KEYS
    enc = _enc()
    enc.blocks.load_state_dict(sd)
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in enc.blocks.state_dict().items())


@pytest.mark.parametrize("L", [1, 3])
def test_init_formulas(L):
    C = 12
    enc = _enc(L=L, H=C, I=24)
    x = torch.arange(C, dtype=torch.float64) / C
    h = torch.arange(C, dtype=torch.float64)
    for l, blk in enumerate(enc.blocks):
        r0, r1 = l / max(L - 1, 1), 1 - l / L
        at, ff = blk.attention, blk.feed_forward
        want = {
            at.time_decay: -5 + 8 * (h / (C - 1)) ** (0.7 + 1.3 * r0),
            at.time_first: math.log(0.3) + ((h + 1) % 3 - 1) / 2,
            at.time_mix_key: x ** r1, at.time_mix_value: x ** r1 + 0.3 * r0,
            at.time_mix_receptance: x ** (r1 / 2),
            ff.time_mix_key: x ** r1, ff.time_mix_receptance: x ** r1,
        }
        for p, w in want.items():
            assert torch.allclose(p.detach().double().flatten(), w, rtol=0, atol=1e-6)
    assert enc.blocks[0].attention.time_first[:3].tolist() == pytest.approx(
        [math.log(0.3), math.log(0.3) + 0.5, math.log(0.3) - 0.5], abs=1e-6)


def test_state_helpers_round_trip():
    enc = _enc(L=3)
    z = enc.zero_state(2, "cpu")
    assert [tuple(s.shape) for s in z] == [(3, 2, 32)] * 5
    assert torch.equal(z[4], torch.full((3, 2, 32), EMPTY_MAX)) and float(z[2].abs().max()) == 0.0
    assert all(s.dtype == torch.float32 for s in z[2:])
    hf = [torch.randn(2, 32, 3) for _ in range(5)]
    st = RWKVEncoder.state_from_hf(hf)
    assert torch.equal(st[0], hf[1].permute(2, 0, 1)) and torch.equal(st[1], hf[0].permute(2, 0, 1))
    assert torch.equal(st[4][1], hf[4][:, :, 1])
    back = RWKVEncoder.state_to_hf(st)
    assert all(torch.equal(a, b) for a, b in zip(back, hf))
    assert sc.detach_states(st)[0].requires_grad is False


def test_asr_model_builds_with_rwkv_config():
    cfg = sc.build_rwkv_config(80, 30, 64, 2)
    assert isinstance(cfg, sc.RWKVConfig) and cfg.return_last_states
    assert (cfg.input_dim, cfg.vocab_size, cfg.hidden_size, cfg.num_layers) == (80, 30, 64, 2)
    m = sc.ASRModel(None, cfg, 30, 80, -1)
    assert isinstance(m.encoder, sc.RWKVEncoder) and m.enc_out_dim == 30
    assert m.input_seq_pad_factor == 1 and not hasattr(m, "proj")
    assert hasattr(sc.ASRModel(None, sc.build_rwkv_config(40, 30, 64, 1), 30, 80, 40), "proj")
    assert sc.wkv is ops.wkv and ops.WKV_CHUNK == _lib.load().sc_wkv_chunk() == 64


def test_entry_points_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    null = ctypes.c_void_p()
    p = ctypes.c_void_p(4096)   # never dereferenced: validation fails before any launch
    fwd = lambda dt, st, B, T, C: lib.sc_wkv_fwd(p, p, p, p, dt, *st, p, p, p, p, null, B, T, C, null)  # noqa: E731
    assert fwd(2, (null,) * 3, 1, 1, 1) == -1 and b"dtype" in lib.sc_last_error()
    assert fwd(7, (null,) * 3, 1, 1, 1) == -1 and b"dtype" in lib.sc_last_error()
    for shape in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (65536, 1, 1)):
        assert fwd(0, (null,) * 3, *shape) == -1 and b"shape" in lib.sc_last_error()
    assert fwd(0, (p, null, p), 1, 1, 1) == -1 and b"state" in lib.sc_last_error()
    assert lib.sc_wkv_fwd(null, p, p, p, 0, null, null, null, p, p, p, p, null, 1, 1, 1, null) == -1
    assert b"null" in lib.sc_last_error()
    assert lib.sc_wkv_fwd(p, p, null, p, 1, null, null, null, p, p, p, p, null, 1, 1, 1, null) == -1
    assert lib.sc_wkv_fwd(p, p, p, p, 1, null, null, null, p, null, p, p, null, 1, 0, 1, null) == -1
    # empty problems launch nothing
    assert fwd(0, (null,) * 3, 0, 5, 5) == 0 and fwd(1, (null,) * 3, 5, 5, 0) == 0
    bwd = lambda dt, B, T, C, ck=p, ws=p: lib.sc_wkv_bwd(p, p, p, p, p, dt, ck, p, p, p, p, ws, B, T, C, null)  # noqa: E731
    assert bwd(2, 1, 1, 1) == -1 and b"dtype" in lib.sc_last_error()
    assert bwd(0, 1, -1, 1) == -1 and b"shape" in lib.sc_last_error()
    assert bwd(0, 1, 1, 1, ck=null) == -1 and b"null" in lib.sc_last_error()
    assert bwd(1, 1, 1, 1, ws=null) == -1 and b"null" in lib.sc_last_error()
    assert bwd(0, 3, 3, 0) == 0
    assert lib.sc_wkv_ckpt_numel(32, 1500, 768) == 32 * 24 * 3 * 768
    assert lib.sc_wkv_ckpt_numel(2, 64, 3) == 2 * 1 * 3 * 3 and lib.sc_wkv_ckpt_numel(2, 65, 3) == 36
    assert lib.sc_wkv_ckpt_numel(2, 0, 3) == 0 and lib.sc_wkv_ckpt_numel(-1, 5, 3) == 0
    assert lib.sc_wkv_bwd_ws_numel(4, 100, 33) == 4 * 2 * 33 and lib.sc_wkv_bwd_ws_numel(4, -1, 3) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_meta_kernels_and_schema(dtype):
    t = tl.load()
    assert "wkv_fwd" in tl.OPS and "wkv_bwd" in tl.OPS
    s = str(torch.ops.statecatcher.wkv_fwd.default._schema)
    assert "Tensor? num0=None" in s and "bool need_ckpt=True" in s
    B, T, C = 3, 130, 33
    k = torch.empty(B, T, C, device=META, dtype=dtype)
    p = torch.empty(C, device=META)
    st = torch.empty(B, C, device=META)
    y, num, den, mx, ck = t.wkv_fwd(p, p, k, k, st, st, st, True)
    assert y.shape == k.shape and y.dtype == dtype
    assert num.shape == den.shape == mx.shape == (B, C) and num.dtype == torch.float32
    assert ck.numel() == _lib.load().sc_wkv_ckpt_numel(B, T, C) and ck.dtype == torch.float32
    assert t.wkv_fwd(p, p, k, k, None, None, None, False)[4].numel() == 0
    dtd, dtf, dk, dv = t.wkv_bwd(p, p, k, k, k, ck)
    assert dtd.shape == dtf.shape == (C,) and dtd.dtype == torch.float32
    assert dk.shape == dv.shape == k.shape and dk.dtype == dtype
    with pytest.raises(RuntimeError, match="equal \\[B,T,C\\]"):
        t.wkv_fwd(p, p, k, k[:, :5], None, None, None, True)
    with pytest.raises(RuntimeError, match="time_decay"):
        t.wkv_fwd(p[:5], p, k, k, None, None, None, True)
    with pytest.raises(RuntimeError, match="together"):
        t.wkv_fwd(p, p, k, k, st, None, st, True)
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        t.wkv_fwd(p, p, k.half(), k.half(), None, None, None, True)


def test_autograd_traces_into_wkv_bwd():
    tl.load()

    def step(td, tf, k, v, n0, d0, m0):
        y, (num, den, mx) = tl.wkv(td, tf, k, v, (n0, d0, m0))
        return torch.autograd.grad(y.float().sum(), (td, tf, k, v))

    B, T, C = 2, 70, 9
    mk = lambda *s, **kw: torch.zeros(*s, device=META, **kw)  # noqa: E731
    args = (mk(C).requires_grad_(), mk(C).requires_grad_(),
            mk(B, T, C, dtype=torch.bfloat16).requires_grad_(),
            mk(B, T, C, dtype=torch.bfloat16).requires_grad_(), mk(B, C), mk(B, C), mk(B, C))
    grads = step(*args)
    assert [tuple(g.shape) for g in grads] == [(C,), (C,), (B, T, C), (B, T, C)]
    assert grads[0].dtype == torch.float32 and grads[2].dtype == torch.bfloat16
    gm = make_fx(step)(*args)
    names = [str(n.target) for n in gm.graph.nodes if "statecatcher" in str(n.target)]
    assert "statecatcher.wkv_fwd.default" in names and "statecatcher.wkv_bwd.default" in names


def test_cpu_tensors_are_refused():
    td, k = torch.zeros(4), torch.zeros(1, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wkv(td, td, k, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _enc()(torch.zeros(1, 3, 8))
    t = tl.load()
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.wkv_fwd(td, td, k, k, None, None, None, True)


def test_bad_operands_raise_before_any_launch(monkeypatch):
    monkeypatch.setattr(ops, "require_device", lambda *t: None)
    td, k = torch.zeros(4), torch.zeros(2, 3, 4)
    st = tuple(torch.zeros(2, 4) for _ in range(3))
    with pytest.raises(ValueError, match="must not require grad"):
        ops.wkv(td, td, k, k, (st[0], st[1].clone().requires_grad_(), st[2]))
    with pytest.raises(ValueError, match="must not require grad"):
        tl.wkv(td, td, k, k, (st[0].clone().requires_grad_(), st[1], st[2]))
    with pytest.raises(ValueError, match="equal \\[B,T,C\\]"):
        ops.wkv(td, td, k, k[:, :2])
    with pytest.raises(TypeError, match="fp32 or bf16"):
        ops.wkv(td, td, k.half(), k.half())
    with pytest.raises(ValueError, match="time_decay"):
        ops.wkv(td[:3], td, k, k)
    with pytest.raises(ValueError, match="state must be"):
        ops.wkv(td, td, k, k, st[:2])
    with pytest.raises(ValueError, match="T >= 1"):
        _enc()(torch.zeros(1, 0, 8))
