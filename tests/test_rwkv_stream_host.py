"""CPU checks of the RWKV streaming path: the held-frame reference (tests/rwkv_stream_ref.py)
against the checker's encoder, the C ABI of sc_wkv_step / sc_rwkv_step_mix / sc_relu_sq
(exports, argument validation and empty calls without a GPU), the Python ops' refusals, the
snapshot's engine choice, and a symbolic replay of one block that counts its launches."""
import ctypes

import pytest
import torch

from tests import rwkv_ref, rwkv_stream_ref

F = ctypes.c_float
FAKE = 0x10000   # never dereferenced: validation fails before any launch


def tiny(F_=16, H=32, A=32, I=64, L=2, V=12, seed=0):
    import statecatcher_amd as sc
    torch.manual_seed(seed)
    enc = sc.RWKVEncoder(sc.RWKVConfig(input_dim=F_, hidden_size=H, num_layers=L, vocab_size=V,
                                       attention_hidden_size=A, intermediate_size=I))
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if ".ln" in n or "pre_ln" in n or n.startswith("ln_out"):
                p.add_(0.1 * torch.randn_like(p))
    return enc


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------ the reference -----
def test_all_live_is_the_checker_exactly():
    sd = tiny().state_dict()
    x = torch.randn(1, 9, 16, generator=torch.Generator().manual_seed(1))
    a, sa = rwkv_stream_ref.encoder_live(sd, x, torch.ones(1, 9))
    b, sb = rwkv_ref.encoder(sd, x)
    assert torch.equal(a, b) and all(torch.equal(u, v) for u, v in zip(sa, sb))
    # None is all live; a carried state goes through unchanged in form
    c, sc_ = rwkv_stream_ref.encoder_live(sd, x, None, state=sb)
    d, sd_ = rwkv_ref.encoder(sd, x, sb)
    assert torch.equal(c, d) and all(torch.equal(u, v) for u, v in zip(sc_, sd_))


def test_batch_rows_are_the_streams_one_by_one():
    """B streams at once equal each stream alone (the reference loops over the streams, so this
    pins the batched checker to it within float64 rounding of another GEMM shape)."""
    sd = tiny().state_dict()
    x = torch.randn(3, 7, 16, generator=torch.Generator().manual_seed(2))
    a, sa = rwkv_stream_ref.encoder_live(sd, x, None)
    b, sb = rwkv_ref.encoder(sd, x)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    for u, v in zip(sa[:2], sb[:2]):
        assert float((u - v).abs().max()) <= 1e-12


def test_holes_equal_the_compacted_stream_in_two_pieces():
    sd = tiny().state_dict()
    g = torch.Generator().manual_seed(3)
    T = 12
    x = torch.randn(2, T, 16, generator=g)
    live = torch.ones(2, T, dtype=torch.bool)
    live[0, 0] = live[0, 4:7] = live[0, 10:] = False     # first frame held, a hole, an early end
    live[1] = False                                      # nothing live
    st0 = tuple(torch.randn(s.shape, generator=g, dtype=torch.float64).abs() + 0.1
                for s in rwkv_stream_ref.zero_state(sd, 2))
    got, st = rwkv_stream_ref.encoder_live(sd, x, live, state=st0)
    idx = live[0].nonzero().flatten()
    xs = x[0:1, idx]
    s0 = tuple(s[:, 0:1] for s in st0)
    y1, s1 = rwkv_ref.encoder(sd, xs[:, :3], s0)
    y2, s2 = rwkv_ref.encoder(sd, xs[:, 3:], s1)
    want = torch.cat([y1, y2], 1)[0]
    assert float((got[0, idx] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert not got[0, ~live[0]].any() and not got[1].any()
    for a, b, c in zip(rwkv_ref.canonical_state(tuple(s[:, 0] for s in st[2:])),
                       rwkv_ref.canonical_state(tuple(s[:, 0] for s in s2[2:])), (0, 1)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    for a, b in zip(st[:2], s2[:2]):
        assert float((a[:, 0] - b[:, 0]).abs().max()) <= 1e-12
    # the stream with no live frame keeps the state it came with, bit for bit
    assert all(torch.equal(a[:, 1], b[:, 1]) for a, b in zip(st, st0))
    # held frames' inputs do not matter
    x2 = x.clone()
    x2[~live] = 7.0
    got2, st2 = rwkv_stream_ref.encoder_live(sd, x2, live, state=st0)
    assert torch.equal(got2, got) and all(torch.equal(a, b) for a, b in zip(st2, st))


# ------------------------------------------------------------------------------ C ABI -------
def wkv_call(lib, **kw):
    a = dict(td=FAKE, tf=FAKE, k=FAKE, v=FAKE, r=None, dtype=0, st=64, sb=64, live=None, num=FAKE,
             den=FAKE, mx=FAKE, y=FAKE, yt=64, yb=64, K=1, B=2, C=64, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sc_wkv_step(*a.values())


def mix_call(lib, **kw):
    a = dict(h=FAKE, ht=64, hb=64, add=None, gate=None, at=0, ab=0, io=0, pre_w=None, pre_b=None,
             ln_w=FAKE, ln_b=FAKE, eps=F(1e-5), x_prev=FAKE, live=None, nmix=2, m0=FAKE, m1=FAKE,
             m2=None, o0=FAKE, o1=FAKE, o2=None, ot=64, ob=64, K=1, B=2, H=64, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sc_rwkv_step_mix(*a.values())


def test_library_exports_the_step_symbols_and_keeps_the_abi(lib):
    from statecatcher_amd import _lib
    for name in ("sc_wkv_step", "sc_rwkv_step_mix", "sc_relu_sq"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.sc_abi_version() == 14


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype=2), b"sc_wkv_step: dtype 2 (fp32 or bf16 only)"),
    (dict(num=None), b"sc_wkv_step: null state"),
    (dict(den=None), b"sc_wkv_step: null state"),
    (dict(mx=None), b"sc_wkv_step: null state"),
    (dict(k=None), b"sc_wkv_step: null pointer"),
    (dict(y=None), b"sc_wkv_step: null pointer"),
    (dict(K=-1), b"sc_wkv_step: bad shape K=-1"),
    (dict(B=65536), b"B <= 65535"),
    (dict(st=-64), b"negative stride"),
    (dict(yb=32), b"y rows overlap"),
    (dict(K=2, yt=8), b"y rows overlap"),
])
def test_wkv_step_rejects_bad_arguments_without_gpu(lib, kw, msg):
    assert wkv_call(lib, **kw) == -1
    assert msg in lib.sc_last_error(), lib.sc_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(io=2), b"sc_rwkv_step_mix: io_dtype 2 (fp32 or bf16 only)"),
    (dict(H=2049, hb=2049, ob=2049), b"sc_rwkv_step_mix: H = 2049 outside [1, 2048]"),
    (dict(H=0), b"H = 0 outside [1, 2048]"),
    (dict(nmix=4), b"nmix = 4 outside [0, 3]"),
    (dict(x_prev=None), b"sc_rwkv_step_mix: null state"),
    (dict(h=None), b"null pointer"),
    (dict(ln_b=None), b"null pointer"),
    (dict(pre_w=FAKE), b"pre_ln needs weight and bias"),
    (dict(gate=FAKE), b"gate without add"),
    (dict(m1=None), b"mix / out 1 is null"),
    (dict(o0=None), b"mix / out 0 is null"),
    (dict(nmix=0, o0=None, x_prev=None), b"mix / out 0 is null"),
    (dict(hb=32), b"rows overlap"),
    (dict(K=2, ot=8), b"rows overlap"),
])
def test_step_mix_rejects_bad_arguments_without_gpu(lib, kw, msg):
    assert mix_call(lib, **kw) == -1
    assert msg in lib.sc_last_error(), lib.sc_last_error()


def test_relu_sq_rejects_bad_arguments_without_gpu(lib):
    assert lib.sc_relu_sq(FAKE, 2, 8, None) == -1
    assert b"sc_relu_sq: dtype 2 (fp32 or bf16 only)" in lib.sc_last_error()
    assert lib.sc_relu_sq(None, 0, 8, None) == -1 and b"null pointer" in lib.sc_last_error()
    assert lib.sc_relu_sq(FAKE, 0, -1, None) == -1 and b"bad length" in lib.sc_last_error()


def test_empty_calls_return_zero(lib):
    for kw in (dict(K=0), dict(B=0), dict(C=0)):
        assert wkv_call(lib, k=None, v=None, num=None, den=None, mx=None, y=None, **kw) == 0
    for kw in (dict(K=0), dict(B=0)):
        assert mix_call(lib, h=None, x_prev=None, ln_w=None, ln_b=None, o0=None, o1=None, **kw) == 0
    assert lib.sc_relu_sq(None, 0, 0, None) == 0 and lib.sc_relu_sq(None, 1, 0, None) == 0
    assert lib.sc_last_error() == b""


# -------------------------------------------------------------------------- Python side -----
def test_ops_refuse_cpu_tensors_and_bad_state():
    from statecatcher_amd import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.wkv_step(z(4), z(4), z(2, 1, 4), z(2, 1, 4), (z(2, 4), z(2, 4), z(2, 4)))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.rwkv_step_mix(z(2, 1, 4), (z(4), z(4)), z(2, 4), (z(4),))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.relu_sq_(z(4))
    dev = torch.device("meta")   # shape / dtype checks come before anything touches memory
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)   # noqa: E731
    for bad, msg in ((m(2, 4, dt=torch.float64), "contiguous fp32"),
                     (m(4, 2).t(), "contiguous fp32"), (m(2, 5), "has shape"), (None, "has shape")):
        with pytest.raises(ValueError, match=msg):   # the in-place state is never cast or copied
            ops._step_state("wkv_step", [("num", bad)], (2, 4), dev)
    ops._step_state("wkv_step", [("num", m(2, 4))], (2, 4), dev)


def test_snapshot_engine_choice_and_refusals():
    import statecatcher_amd as sc
    enc = tiny()
    w = enc.step_weights(torch.bfloat16)
    assert w["gemm"] == "frame" and w["frame"] and w["act"] == torch.float32
    assert w["blocks"][0]["pre_ln"] is not None and w["blocks"][1]["pre_ln"] is None
    assert w["blocks"][0]["key"][0].dtype == torch.bfloat16
    assert w["blocks"][0]["key"][1].dtype == torch.float32          # the frame engine's zero bias
    assert w["blocks"][0]["ln1"][0].dtype == torch.float32 and not w["emb"][0].requires_grad
    lw = enc.step_weights(torch.bfloat16, gemm="library")
    assert lw["gemm"] == "library" and lw["act"] == torch.bfloat16 and lw["blocks"][0]["key"][1] is None
    odd = tiny(F_=20)   # input width 20 is no multiple of 8
    assert not odd.step_gemm_frame_ok() and odd.step_weights(torch.float32)["gemm"] == "library"
    with pytest.raises(ValueError, match='gemm="frame" needs fp32 / bf16 weights and every '
                                         'reduction length a multiple of 8, at most 2048'):
        odd.step_weights(torch.float32, gemm="frame")
    assert not tiny(I=4096).step_gemm_frame_ok()
    proj = torch.nn.Linear(12, 16)
    assert not enc.step_gemm_frame_ok(proj) and enc.step_gemm_frame_ok(torch.nn.Linear(24, 16))
    with pytest.raises(ValueError, match="gemm must be"):
        enc.step_weights(torch.float32, gemm="hipblas")
    with pytest.raises(ValueError, match="fp32 or bf16"):
        enc.step_weights(torch.float16)
    assert "StreamingRWKV" in sc.__all__
    with pytest.raises(TypeError, match="RWKVEncoder"):
        sc.StreamingRWKV(torch.nn.Linear(4, 4), batch=2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # a supported model gets to the device check
        sc.StreamingRWKV(enc, batch=2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        enc.step(torch.zeros(2, 3, 16))


# ------------------------------------------------------------------------ symbolic replay ---
@pytest.mark.parametrize("L,K,proj", [(2, 1, False), (3, 4, True)])
def test_block_is_a_chain_of_at_most_eight_launches_per_layer(monkeypatch, L, K, proj):
    """One block on recorded ops: 8 launches per layer of the stack for the K frames, plus the
    input projection(s), the final mix and the output projection; every launch reads what an
    earlier one wrote; layer l works on its own state rows; two blocks use the same buffers."""
    from statecatcher_amd import ops
    enc = tiny(L=L)
    B = 3
    ip = torch.nn.Linear(24, 16) if proj else None
    w = enc.step_weights(torch.bfloat16, ip, "frame")
    ws = enc.step_workspace(B, K, w, torch.device("cpu"))
    state = enc.zero_state(B, torch.device("cpu"))
    log = []
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    monkeypatch.setattr(ops._lib, "stream_of", lambda t: None)
    monkeypatch.setattr(ops, "frame_gemm_job", lambda x, wt, b, y: (P(x), P(y), x.shape[0]))
    monkeypatch.setattr(ops, "lucy_frame_gemm_multi", lambda epi, dt, jobs, stream:
                        log.append(("gemm", [j[0] for j in jobs], [j[1] for j in jobs])))
    monkeypatch.setattr(ops, "lucy_frame_gemm", lambda epi, x, wt, b, y:
                        log.append(("gemm", [P(x)], [P(y)])))
    monkeypatch.setattr(ops, "rwkv_step_mix", lambda h, ln, x_prev, mixes, outs, add=None,
                        gate=None, pre_ln=None, live=None, eps=1e-5:
                        log.append(("mix", [P(h), P(add), P(gate)], [P(o) for o in outs] + [P(h)],
                                    P(x_prev), pre_ln is not None, len(mixes), P(live))))
    monkeypatch.setattr(ops, "wkv_step", lambda td, tf, k, v, st, r=None, live=None, out=None:
                        log.append(("wkv", [P(k), P(v), P(r)], [P(out)], [P(s) for s in st], P(live))))
    monkeypatch.setattr(ops, "relu_sq_", lambda x: log.append(("relu", [P(x)], [P(x)])))
    enc._step_block(ws, state, ws["live"], w)
    first = list(log)
    enc._step_block(ws, state, ws["live"], w)
    assert log[len(first):] == first
    kinds = [e[0] for e in first]
    per_layer = ["mix", "gemm", "wkv", "gemm", "mix", "gemm", "relu", "gemm"]
    assert kinds == ["gemm"] * (2 if proj else 1) + per_layer * L + ["mix", "gemm"]
    written = {P(ws["x"])}
    for e in first:
        for p in e[1]:
            assert p is None or p in written, e
        written.update(e[2])
    assert first[-1][2] == [P(ws["logits"])]
    mixes = [e for e in first if e[0] == "mix"]
    x_att, x_ffn, num, den, mx = state
    for l in range(L):
        a, f = mixes[2 * l], mixes[2 * l + 1]
        assert a[3] == P(x_att[l]) and f[3] == P(x_ffn[l])
        assert a[4] == (l == 0) and not f[4] and (a[5], f[5]) == (3, 2)
        assert a[6] == f[6] == P(ws["live"])
    assert mixes[-1][3] is None and mixes[-1][5] == 0
    for l, e in enumerate(e for e in first if e[0] == "wkv"):
        assert e[3] == [P(num[l]), P(den[l]), P(mx[l])] and e[4] == P(ws["live"])
        assert e[1][2] is not None   # the receptance gate rides in the WKV launch
