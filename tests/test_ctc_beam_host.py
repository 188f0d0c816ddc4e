"""CPU checks of the CTC prefix beam search (csrc/ctc_beam.hip, sc_ctc_beam_*):

* the numpy helper tests/ctc_beam_ref.py, before it judges the kernel, against exact enumeration:
  where nothing is pruned every prefix's score is -nll of that prefix from oracle/ctc.py;
* the C ABI validates its arguments before launching and names the offender; empty calls are
  no-ops; the size functions grow with each argument;
* the dispatcher ops have their schemas and Meta kernels give the documented shapes.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import ctc as octc
from tests.ctc_beam_ref import ctc_beam_ref, padded_nbest, score_drift


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_equals_exact_enumeration(seed, blank):
    """T=4, V=3, beam=32, top_k=2: at most 31 prefixes exist, so nothing is pruned."""
    T, V, beam, top_k = 4, 3, 32, 2
    rng = np.random.default_rng(seed)
    lp = octc.log_softmax(2.0 * rng.standard_normal((2, T, V)))
    lens = [T, T - 1]
    ref = ctc_beam_ref(lp, lens, blank=blank, beam=beam, top_k=top_k)
    assert ref.beam_margin == np.inf and ref.merges > 0 and ref.repeats > 0
    labels = [v for v in range(V) if v != blank]
    for b in range(2):
        got = {tuple(p): s for p, s in zip(ref.tokens[b], ref.scores[b])}
        assert len(got) == len(ref.tokens[b])                 # no prefix twice
        assert ref.scores[b] == sorted(ref.scores[b], reverse=True)
        feasible = 0
        for n in range(lens[b] + 1):
            for p in itertools.product(labels, repeat=n):
                nll, _ = octc.ctc_single(lp[b, :lens[b]], np.array(p, np.int64), blank)
                if np.isinf(nll):
                    assert p not in got
                    continue
                feasible += 1
                assert abs(got[p] + nll) <= 1e-9, (p, got[p], -nll)
        assert feasible == len(got)
        assert abs(np.logaddexp.reduce(ref.scores[b])) <= 1e-9   # the prefixes' probabilities sum to 1


def test_reference_logits_mask_and_max_frames():
    rng = np.random.default_rng(5)
    x = 3.0 * rng.standard_normal((2, 12, 7))
    a = ctc_beam_ref(x, [12, 9], beam=4, top_k=3, is_logits=True)
    b = ctc_beam_ref(octc.log_softmax(x), [12, 9], beam=4, top_k=3)
    assert a.tokens == b.tokens and np.allclose(a.scores[0], b.scores[0], atol=1e-12)
    # mask and lengths say the same thing in two ways
    mask = np.ones((2, 12), np.float32)
    mask[1, 9:] = 0
    c = ctc_beam_ref(x, None, mask=mask, beam=4, top_k=3, is_logits=True)
    assert c.tokens == a.tokens and c.scores == a.scores
    # max_frames cuts the stream and says so
    d = ctc_beam_ref(x, [12, 9], beam=4, top_k=3, is_logits=True, max_frames=9)
    e = ctc_beam_ref(x, [9, 9], beam=4, top_k=3, is_logits=True)
    assert d.tokens == e.tokens and d.status.tolist() == [1, 0] and e.status.tolist() == [0, 0]
    # fp32 evaluation: the same candidates, scores within fp32 rounding of scores up to ~30
    f = ctc_beam_ref(x, [12, 9], beam=4, top_k=3, is_logits=True, dtype=np.float32)
    assert 0 < score_drift(a, f) < 1e-4
    tok, lens = padded_nbest(a.tokens, 2, 3)
    assert tok.shape == (2, 2, 3) and lens[0, 0] == len(a.tokens[0][0])


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(4096)   # never dereferenced: validation fails before any launch


def _frames(lib, dtype=0, B=1, T=2, V=8, blank=0, beam=4, top_k=3, x=P, state=P, ws=P,
            state_bytes=None, ws_bytes=None):
    null = ctypes.c_void_p()
    if state_bytes is None:
        state_bytes = lib.sc_ctc_beam_state_bytes(B, min(max(beam, 1), 32), 10)
    if ws_bytes is None:
        ws_bytes = lib.sc_ctc_beam_workspace_bytes(B, T, min(max(top_k, 1), 32))
    return lib.sc_ctc_beam_frames(x, dtype, 1, B, T, V, T * V, V, null, null, 0, 0, blank, beam,
                                  top_k, state, state_bytes, ws, ws_bytes, null)


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=7), b"dtype"),
    (dict(beam=0), b"beam"),
    (dict(beam=33), b"beam"),
    (dict(top_k=0), b"top_k"),
    (dict(top_k=33, V=64), b"top_k"),
    (dict(top_k=8, V=8), b"top_k"),          # top_k <= V - 1
    (dict(blank=8), b"blank"),
    (dict(blank=-1), b"blank"),
    (dict(V=1, top_k=1), b"shape"),
    (dict(x=ctypes.c_void_p()), b"null pointer"),
    (dict(state=ctypes.c_void_p()), b"null pointer"),
    (dict(ws=ctypes.c_void_p()), b"null pointer"),
    (dict(state_bytes=5), b"state_bytes"),
    (dict(ws_bytes=4), b"workspace_bytes"),
])
def test_frames_rejects_bad_arguments_without_gpu(lib, kw, word):
    assert _frames(lib, **kw) == -1
    msg = lib.sc_last_error()
    assert b"sc_ctc_beam_frames" in msg and word in msg, msg


def test_reset_and_result_reject_bad_arguments_without_gpu(lib):
    null = ctypes.c_void_p()
    n = lib.sc_ctc_beam_state_bytes(2, 4, 10)

    def err(rc, fn, word):
        msg = lib.sc_last_error()
        assert rc == -1 and fn in msg and word in msg, msg

    err(lib.sc_ctc_beam_reset(P, n, 2, 0, 10, null, null), b"sc_ctc_beam_reset", b"beam")
    err(lib.sc_ctc_beam_reset(P, n, 2, 4, -1, null, null), b"sc_ctc_beam_reset", b"max_frames")
    err(lib.sc_ctc_beam_reset(null, n, 2, 4, 10, null, null), b"sc_ctc_beam_reset", b"null pointer")
    err(lib.sc_ctc_beam_reset(P, n - 8, 2, 4, 10, null, null), b"sc_ctc_beam_reset", b"state_bytes")
    res = lib.sc_ctc_beam_result
    err(res(P, n, 2, 40, 1, P, 4, P, P, null, null), b"sc_ctc_beam_result", b"beam")
    err(res(P, n, 2, 4, 0, P, 4, P, P, null, null), b"sc_ctc_beam_result", b"nbest")
    err(res(P, n, 2, 4, 5, P, 4, P, P, null, null), b"sc_ctc_beam_result", b"nbest")
    err(res(P, n, 2, 4, 1, P, -1, P, P, null, null), b"sc_ctc_beam_result", b"cap")
    err(res(null, n, 2, 4, 1, P, 4, P, P, null, null), b"sc_ctc_beam_result", b"null pointer")
    err(res(P, n, 2, 4, 1, null, 4, P, P, null, null), b"sc_ctc_beam_result", b"null pointer")
    err(res(P, n, 2, 4, 1, P, 4, null, P, null, null), b"sc_ctc_beam_result", b"null pointer")
    err(res(P, n + 4, 2, 4, 1, P, 4, P, P, null, null), b"sc_ctc_beam_result", b"state_bytes")


def test_empty_calls_are_noops(lib):
    null = ctypes.c_void_p()
    assert lib.sc_ctc_beam_reset(null, 0, 0, 4, 10, null, null) == 0
    assert lib.sc_last_error() == b""
    assert lib.sc_ctc_beam_frames(null, 0, 1, 0, 5, 8, 0, 0, null, null, 0, 0, 0, 4, 3, null, 0,
                                  null, 0, null) == 0
    assert lib.sc_ctc_beam_frames(null, 0, 1, 2, 0, 8, 0, 0, null, null, 0, 0, 0, 4, 3, null, 0,
                                  null, 0, null) == 0
    assert lib.sc_ctc_beam_result(null, 0, 0, 4, 1, null, 0, null, null, null, null) == 0
    assert lib.sc_last_error() == b""


def test_size_functions_grow_with_each_argument(lib):
    sb, wb = lib.sc_ctc_beam_state_bytes, lib.sc_ctc_beam_workspace_bytes
    base = sb(2, 4, 10)
    assert 0 < base < sb(3, 4, 10) and base < sb(2, 5, 10) and base < sb(2, 4, 11)
    assert sb(2, 4, 10) == 2 * sb(1, 4, 10)
    # the trie alone: (parent, token) for the empty prefix and max_frames * beam extensions
    assert sb(1, 4, 10) >= 8 * (1 + 10 * 4) and sb(1, 4, 11) - sb(1, 4, 10) == 8 * 4
    assert sb(1, 0, 10) == 0 and sb(1, 33, 10) == 0 and sb(1, 4, -1) == 0 and sb(-1, 4, 10) == 0
    wbase = wb(2, 10, 4)
    assert 0 < wbase < wb(3, 10, 4) and wbase < wb(2, 11, 4) and wbase < wb(2, 10, 5)
    assert wbase >= 2 * 10 * (1 + 2 * 4) * 4      # lp[blank] and top_k (index, lp) pairs per row
    assert wb(2, 10, 0) == 0 and wb(2, 10, 33) == 0 and wb(2, -1, 4) == 0
    # C2's decode size fits comfortably: the widest state is ~12 MB per 32 streams
    assert sb(32, 32, 1500) < 16 << 20 and wb(32, 1500, 32) < 16 << 20


def test_dispatcher_schemas_and_meta_shapes():
    import statecatcher_amd
    from statecatcher_amd import torch_library as tl
    sc = tl.load()
    for name in ("ctc_beam_state_bytes", "ctc_beam_reset_", "ctc_beam_frames_", "ctc_beam_result",
                 "ctc_beam_decode"):
        assert name in tl.OPS and hasattr(sc, name)
    for name in ("ctc_beam_decode", "ctc_beam_state", "ctc_beam_result", "ctc_beam_decoder"):
        assert name in statecatcher_amd.__all__ and hasattr(statecatcher_amd, name)
    s = str(torch.ops.statecatcher.ctc_beam_decode.default._schema)
    for part in ("Tensor x", "Tensor? lengths=None", "Tensor? mask=None", "int blank=0", "int beam=8",
                 "int top_k=8", "int nbest=1", "bool is_logits=False", "int? max_frames=None",
                 "int? cap=None", "-> (Tensor tokens, Tensor lens, Tensor scores)"):
        assert part in s, (part, s)
    s = str(torch.ops.statecatcher.ctc_beam_frames_.default._schema)
    for part in ("Tensor x", "Tensor(a!) state", "int top_k=8", "-> ()"):
        assert part in s, (part, s)
    assert "Tensor(a!) state" in str(torch.ops.statecatcher.ctc_beam_reset_.default._schema)
    assert "Tensor status" in str(torch.ops.statecatcher.ctc_beam_result.default._schema)
    lib_bytes = statecatcher_amd._lib.load().sc_ctc_beam_state_bytes(1, 8, 20)
    assert sc.ctc_beam_state_bytes(1, 8, 20) == lib_bytes
    with pytest.raises(RuntimeError, match="beam"):
        sc.ctc_beam_state_bytes(1, 40, 20)
    meta = torch.device("meta")
    B, T, V = 3, 20, 37
    x = torch.empty(B, T, V, device=meta, dtype=torch.bfloat16)
    tok, lens, scores = sc.ctc_beam_decode(x, nbest=4)
    assert tok.shape == (B, 4, T) and lens.shape == scores.shape == (B, 4)
    assert tok.dtype == lens.dtype == torch.int32 and scores.dtype == torch.float32
    tok, lens, scores = sc.ctc_beam_decode(x, max_frames=9, cap=5)
    assert tok.shape == (B, 1, 5)
    state = torch.empty(B, lib_bytes, device=meta, dtype=torch.uint8)
    tok, lens, scores, status = sc.ctc_beam_result(state, 8, 2, 6)
    assert tok.shape == (B, 2, 6) and lens.shape == (B, 2) and status.shape == (B,)
    with pytest.raises((RuntimeError, NotImplementedError)):   # no CPU kernel, no fallback
        sc.ctc_beam_decode(torch.zeros(1, 4, V))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        statecatcher_amd.ctc_beam_decode(torch.zeros(1, 4, V))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        statecatcher_amd.ctc_beam_state(1, 8, 4, "cpu")
