"""CPU checks of the LucyRNNtriton streaming path: the C ABI of sc_lucy_tframe_layer / _multi
(exports, argument validation without a GPU), StreamingLucyRNNtriton's constructor refusals, and
a symbolic replay of both schedules.

The replay replaces the ops by recorders (as tests/test_streaming_schedule.py does for the native
class) and identifies buffers by their data pointers.  A launch's jobs run concurrently, so all
of a launch's reads are checked against the state BEFORE the launch, and no job of a launch may
read what another job of it writes.  Every (layer, frame) must
  * read the previous layer's output AND records of its own frame, not yet overwritten (the
    double-buffer check inside one multi launch);
  * update its state h[l], s[l] after (l, j - 1) did, in an earlier launch;
  * be one of at most 8 jobs of its launch;
the projection and the greedy launch come last, and two consecutive blocks use the same pointers
(the block is captured once)."""
import ctypes
import types

import pytest
import torch

F = ctypes.c_float
FAKE = 0x10000   # never dereferenced: validation fails before any launch


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


def layer_call(lib, **kw):
    """sc_lucy_tframe_layer on fake pointers with a valid argument set, overridden by kw."""
    a = dict(x=FAKE, ldx=64, K=64, ln_w=None, ln_b=None, st_in=None, nst_in=0, eps=F(1e-5), w=FAKE,
             w_dtype=0, ldw=64, bias=FAKE, B=3, D=32, h=FAKE, s=FAKE, out=FAKE, ldo=32, st_out=None,
             mask=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sc_lucy_tframe_layer(*a.values())


def test_library_exports_tframe_symbols(lib):
    from statecatcher_amd import _lib
    for name in ("sc_lucy_tframe_layer", "sc_lucy_tframe_layer_multi"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.sc_abi_version() == 14


@pytest.mark.parametrize("kw,msg", [
    (dict(w_dtype=2), b"fp32 or bf16"),
    (dict(D=40), b"multiple of 16"),
    (dict(K=6), b"16-byte aligned"),
    (dict(w_dtype=1, K=12, ldx=12), b"K % 8"),
    (dict(x=FAKE + 4), b"16-byte aligned"),
    (dict(ldw=60), b"16-byte aligned"),
    (dict(ln_w=FAKE + 4, ln_b=FAKE, st_in=FAKE, nst_in=2), b"LayerNorm parameters"),
    (dict(K=2052, ldx=2052, ldw=2056), b"above 2048"),
    (dict(h=None), b"null"),
    (dict(s=None), b"null"),
    (dict(out=None), b"null"),
    (dict(bias=None), b"null"),
    (dict(ln_w=FAKE, ln_b=FAKE), b"weight, bias and statistics"),
    (dict(ln_w=FAKE, st_in=FAKE, nst_in=2), b"weight, bias and statistics"),
])
def test_tframe_layer_rejects_bad_arguments_without_gpu(lib, kw, msg):
    assert layer_call(lib, **kw) == -1
    assert msg in lib.sc_last_error(), lib.sc_last_error()


def test_tframe_noops_and_job_count(lib):
    from statecatcher_amd._lib import TFrameJob
    null = ctypes.c_void_p()
    assert layer_call(lib, B=0, x=None, w=None, bias=None, h=None, s=None, out=None) == 0
    assert lib.sc_lucy_tframe_layer_multi(0, F(1e-5), null, 0, null) == 0
    jobs = (TFrameJob * 9)()
    assert lib.sc_lucy_tframe_layer_multi(0, F(1e-5), jobs, 9, null) == -1
    assert b"jobs per call" in lib.sc_last_error()
    assert lib.sc_lucy_tframe_layer_multi(0, F(1e-5), jobs, -1, null) == -1
    # every job is validated before anything is launched: job 1 has null pointers
    for i in range(2):
        jobs[i].B, jobs[i].K, jobs[i].D, jobs[i].ldx, jobs[i].ldw = 0, 64, 32, 64, 64
    jobs[1].B = 2
    assert lib.sc_lucy_tframe_layer_multi(0, F(1e-5), jobs, 2, null) == -1
    assert b"null" in lib.sc_last_error()
    jobs[1].B = 0   # all jobs empty: a no-op
    assert lib.sc_lucy_tframe_layer_multi(0, F(1e-5), jobs, 2, null) == 0
    assert lib.sc_lucy_tframe_layer_multi(3, F(1e-5), jobs, 2, null) == -1
    assert b"fp32 or bf16" in lib.sc_last_error()


def test_frame_gemm_still_rejects_the_new_epilogue_code(lib):
    """The LucyRNNtriton epilogue is reachable through the new entry points only."""
    null = ctypes.c_void_p()
    rc = lib.sc_lucy_frame_gemm(4, null, 4, 4, null, null, null, 0, F(1e-5), null, 0, 8, null, 1, 64,
                                null, 4, null, null, null, null, null, null)
    assert rc == -1 and b"bad epilogue" in lib.sc_last_error()
    rc = lib.sc_lucy_frame_gemm_multi(4, 0, F(1e-5), null, 0, null)
    assert rc == 0   # (no jobs: nothing to check)
    from statecatcher_amd._lib import FrameGemmJob
    jobs = (FrameGemmJob * 1)()
    jobs[0].B, jobs[0].K, jobs[0].N = 1, 4, 64
    rc = lib.sc_lucy_frame_gemm_multi(4, 0, F(1e-5), jobs, 1, null)
    assert rc == -1 and b"bad epilogue" in lib.sc_last_error()


def test_constructor_refusals_on_cpu_models():
    import statecatcher_amd as sc
    from tests.tframe_ref import model_from
    assert "StreamingLucyRNNtriton" in sc.__all__
    with pytest.raises(ValueError, match="num_tracks.*forward"):
        sc.StreamingLucyRNNtriton(model_from(None, 2, 8, 32, 10, num_tracks=2), batch=2)
    with pytest.raises(ValueError, match="multiple of 16.*forward"):
        sc.StreamingLucyRNNtriton(model_from(None, 2, 8, 40, 10), batch=2)
    with pytest.raises(ValueError, match="2048.*forward"):
        sc.StreamingLucyRNNtriton(model_from(None, 1, 8, 2064, 10), batch=2)
    native = sc.LucyRNN(sc.LucyRNNConfig(input_dim=8, hidden_dim=32, num_layers=2, vocab_size=10,
                                         kernel_impl="native", is_training=False))
    with pytest.raises(TypeError, match="LucyRNNtriton"):
        sc.StreamingLucyRNNtriton(native, batch=2)
    # a supported model on the CPU gets as far as the device requirement
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        sc.StreamingLucyRNNtriton(model_from(None, 2, 8, 32, 10), batch=2)


# ------------------------------------------------------------------------ symbolic replay ---
def fake_stream(L, K, schedule, B=3, D=32, Din=10, V=10):
    from statecatcher_amd.streaming import StreamingLucyRNNtriton
    z = lambda *s: torch.zeros(*s)   # noqa: E731
    st = StreamingLucyRNNtriton.__new__(StreamingLucyRNNtriton)
    st.cfg = types.SimpleNamespace(stack_order=1)
    st.L, st.K, st.B, st.D, st.V, st.Din, st.Dp, st.blank = L, K, B, D, V, Din, 16, 0
    st.schedule, st.eps, st.dtype = schedule, 1e-5, torch.float32
    st.x, st.mask = z(K, B, 16), torch.ones(K, B)
    st.layers = [dict(w=z(7 * D, 16 if l == 0 else D), b=z(7 * D), ln=(z(D), z(D)) if l else None)
                 for l in range(L)]
    st.h = [z(B, D) for _ in range(L)]
    st.s = [z(B, D) for _ in range(L)]
    st.xo = [(z(B, D), z(B, D)) for _ in range(L - 1)]
    st.rec = [(z(D // 16, B, 4), z(D // 16, B, 4)) for _ in range(L - 1)]
    st.xlast = z(K, B, D)
    st.w_out, st.b_out = z(V, D), z(V)
    st.logits = z(K, B, V)
    st.prev = torch.full((B,), -1, dtype=torch.int32)
    st.emit = torch.full((K, B), -1, dtype=torch.int32)
    return st


def record_ops(monkeypatch, launches):
    from statecatcher_amd import ops
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    job = lambda j: dict(x=j.x, st_in=j.st_in, h=j.h, s=j.s, out=j.out, st_out=j.st_out,   # noqa: E731
                         ln=j.ln_w is not None, mask=j.mask)
    monkeypatch.setattr(ops._lib, "stream_of", lambda t: None)

    def multi(w_dtype, jobs, stream, eps=1e-5):
        for k in range(0, len(jobs), 8):   # (ops.lucy_tframe_layer_multi's own split)
            launches.append(("layers", [job(j) for j in jobs[k:k + 8]]))

    def single(x, w, bias, h, s, out, st_out=None, ln=None, st_in=None, mask=None, eps=1e-5):
        launches.append(("layers", [dict(x=P(x), st_in=P(st_in), h=P(h), s=P(s), out=P(out),
                                         st_out=P(st_out), ln=ln is not None, mask=P(mask))]))
    monkeypatch.setattr(ops, "lucy_tframe_layer_multi", multi)
    monkeypatch.setattr(ops, "lucy_tframe_layer", single)
    monkeypatch.setattr(ops, "lucy_frame_gemm", lambda epi, x, w, bias, y, **kw: launches.append(
        ("out", (P(x), x.shape[0], P(y)))))
    monkeypatch.setattr(ops, "ctc_greedy_frames", lambda logits, prev, emit, mask=None, blank=0:
                        launches.append(("greedy", (P(logits), logits.shape[0]))))
    monkeypatch.setattr(ops, "ctc_greedy_step", lambda logits, prev, emit, mask=None, blank=0:
                        launches.append(("greedy", (P(logits), 1))))


@pytest.mark.parametrize("L,K", [(6, 8), (6, 2), (3, 1), (2, 5), (10, 3)])
@pytest.mark.parametrize("schedule", ["wavefront", "frame"])
def test_schedule_respects_dependencies(monkeypatch, L, K, schedule):
    st = fake_stream(L, K, schedule)
    launches = []
    record_ops(monkeypatch, launches)
    st._block()
    first = list(launches)
    st._block()
    assert launches[len(first):] == first   # the same pointers in two consecutive blocks

    P = lambda t: t.data_ptr()   # noqa: E731
    holds = {}          # buffer -> (layer, frame) of the value it holds
    done = {}           # (l, j) -> index of its launch
    projected, decoded = set(), set()   # frames whose logits / tokens are out
    for li, (kind, what) in enumerate(first):
        if kind == "out":
            xp, rows, yp = what
            j0 = [j for j in range(K) if P(st.xlast[j]) == xp][0]
            assert yp == P(st.logits[j0])
            for j in range(j0, j0 + rows // st.B):
                assert holds[P(st.xlast[j])] == (L - 1, j)
                projected.add(j)
            continue
        if kind == "greedy":
            lp, n = what
            j0 = [j for j in range(K) if P(st.logits[j]) == lp][0]
            for j in range(j0, j0 + n):
                assert j in projected and j not in decoded and (j == 0 or j - 1 in decoded)
                decoded.add(j)
            continue
        jobs = what
        assert 1 <= len(jobs) <= 8
        reads = {p for jb in jobs for p in (jb["x"], jb["st_in"]) if p is not None}
        writes = [p for jb in jobs for p in (jb["out"], jb["st_out"], jb["h"], jb["s"])
                  if p is not None]
        assert len(set(writes)) == len(writes) and not reads & set(writes)
        new = {}
        for jb in jobs:
            l = [i for i in range(L) if P(st.h[i]) == jb["h"]][0]
            assert jb["s"] == P(st.s[l])
            j = len([1 for (ll, _) in done if ll == l])
            assert j < K and (j == 0 or done[(l, j - 1)] < li)
            assert jb["mask"] == P(st.mask[j])
            if l == 0:
                assert jb["x"] == P(st.x[j]) and not jb["ln"] and jb["st_in"] is None
            else:
                assert done[(l - 1, j)] < li and jb["ln"]
                assert holds[jb["x"]] == (l - 1, j) and holds[jb["st_in"]] == (l - 1, j)
                assert jb["x"] in [P(t) for t in st.xo[l - 1]]
                assert jb["st_in"] in [P(t) for t in st.rec[l - 1]]
            if l == L - 1:
                assert jb["out"] == P(st.xlast[j]) and jb["st_out"] is None
            else:
                p = [P(t) for t in st.xo[l]].index(jb["out"])
                assert jb["st_out"] == P(st.rec[l][p])
            new[(l, j)] = (jb["out"], jb["st_out"])
        for (l, j), bufs in new.items():   # the launch's writes land after all of its reads
            done[(l, j)] = li
            for b in bufs:
                if b is not None:
                    holds[b] = (l, j)
    assert sorted(done) == sorted((l, j) for l in range(L) for j in range(K))
    assert decoded == projected == set(range(K))
    kinds = [k for k, _ in first]
    if schedule == "wavefront":
        per_stage = [min(L, K, t + 1, K + L - 1 - t) for t in range(K + L - 1)]
        assert kinds.count("layers") == sum((n + 7) // 8 for n in per_stage)
        assert L > 8 or len(first) == (K + L - 1) + 2
        assert kinds[-2:] == ["out", "greedy"] and kinds.count("out") == kinds.count("greedy") == 1
    else:
        assert kinds == (["layers"] * L + ["out", "greedy"]) * K
