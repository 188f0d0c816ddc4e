"""CPU checks of the transducer beam search (csrc/rnnt_beam.hip, sc_rnnt_beam_*):

* the numpy helper tests/rnnt_beam_ref.py, before it judges the kernel, against exact lattices:
  where nothing is pruned every prefix's score is log P(prefix | x) over the alignments with at
  most max_symbols emissions per frame, from an independent forward lattice and, where
  max_symbols does not bind, from oracle/rnnt.py;
* the helper's lp rows against RNNTPredictorJoiner.forward;
* the C ABI validates its arguments before launching and names the offender; empty calls are
  no-ops; the state size grows with each argument;
* the dispatcher ops have their schemas and Meta kernels give the documented shapes.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rnnt as ornnt
from tests.rnnt_beam_ref import (exact_prefix_scores, padded_nbest, rnnt_beam_ref, rnnt_lp_row,
                                 score_drift)


def small_inputs(seed, T, V, J=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((1, T, J)), rng.standard_normal((V, J)),
            rng.standard_normal((V, J)), rng.standard_normal(V))


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("T,ms,count", [(2, 1, 7), (2, 2, 31), (3, 1, 15)])
def test_reference_equals_exact_lattices(T, ms, count, blank):
    """V=3, top_k=2 and a beam that holds every prefix: nothing is pruned."""
    V = 3
    E, P, W, bias = small_inputs(T * 10 + ms, T, V)
    ref = rnnt_beam_ref(E, P, W, bias, blank=blank, beam=count, top_k=V - 1, max_symbols=ms)
    assert ref.beam_margin == np.inf and ref.merges > 0
    got = {tuple(p): s for p, s in zip(ref.tokens[0], ref.scores[0])}
    assert len(got) == len(ref.tokens[0]) == count                # every prefix, none twice
    assert ref.scores[0] == sorted(ref.scores[0], reverse=True)
    row = lambda t, u: rnnt_lp_row(E[0, t], P[u], W, bias)         # noqa: E731
    exact = exact_prefix_scores(row, T, V, blank, ms, T * ms)
    assert set(exact) == set(got)
    for y, s in exact.items():
        assert abs(got[y] - s) <= 1e-12, (y, got[y], s)
    for y in got:
        if len(y) > ms:
            continue   # max_symbols binds: the unrestricted lattice has more alignments
        lp = np.stack([np.stack([row(t, y[u - 1] if u else blank) for u in range(len(y) + 1)])
                       for t in range(T)])
        nll, _ = ornnt.rnnt_single(lp, np.array(y, np.int64), blank)
        assert abs(got[y] + nll) <= 1e-12, (y, got[y], -nll)


def test_reference_mask_max_frames_frames_and_fp32():
    rng = np.random.default_rng(5)
    E, P = rng.standard_normal((2, 12, 8)), rng.standard_normal((7, 8))
    W, bias = rng.standard_normal((7, 8)), rng.standard_normal(7)
    bias[0] += 2.0
    kw = dict(beam=4, top_k=3, max_symbols=2)
    a = rnnt_beam_ref(E, P, W, bias, [12, 9], **kw)
    mask = np.ones((2, 12), np.float32)
    mask[1, 9:] = 0
    c = rnnt_beam_ref(E, P, W, bias, None, mask=mask, **kw)
    assert c.tokens == a.tokens and c.scores == a.scores and c.frames == a.frames
    d = rnnt_beam_ref(E, P, W, bias, [12, 9], max_frames=9, **kw)
    e = rnnt_beam_ref(E, P, W, bias, [9, 9], **kw)
    assert d.tokens == e.tokens and d.status.tolist() == [1, 0] and e.status.tolist() == [0, 0]
    for b in range(2):
        for toks, frs in zip(a.tokens[b], a.frames[b]):
            assert len(toks) == len(frs) and frs == sorted(frs)
            assert all(0 <= f < [12, 9][b] for f in frs)
            assert max(np.bincount(frs), default=0) <= kw["max_symbols"]
    f = rnnt_beam_ref(E, P, W, bias, [12, 9], dtype=np.float32, **kw)
    assert 0 < score_drift(a, f) < 1e-4
    tok, lens = padded_nbest(a.tokens, 2, 3)
    assert tok.shape == (2, 2, 3) and lens[0, 0] == len(a.tokens[0][0])
    # top_k above V - 1 is clipped
    g = rnnt_beam_ref(E, P, W, bias, [12, 9], beam=4, top_k=6, max_symbols=2)
    h = rnnt_beam_ref(E, P, W, bias, [12, 9], beam=4, top_k=30, max_symbols=2)
    assert g.tokens == h.tokens and g.scores == h.scores


@pytest.mark.parametrize("seed", [0, 1])
def test_helper_rows_agree_with_the_trained_joiner(seed):
    """At the nodes of the best hypothesis the helper's lp rows are log_softmax of
    RNNTPredictorJoiner.forward on that prefix."""
    from statecatcher_amd.model import RNNTPredictorJoiner
    torch.manual_seed(seed)
    B, T, D, V, J, blank = 2, 12, 6, 11, 8, 0
    jm = RNNTPredictorJoiner(D, 5, J, V).double()
    with torch.no_grad():
        jm.joiner.bias[blank] += 0.3
        jm.joiner.weight *= 3.0   # spread the logits: emissions and blanks both occur
        enc_out = torch.randn(B, T, D, dtype=torch.float64)
        E = jm.enc_proj(enc_out).numpy()
        P = jm.pred_proj(jm.embedding.weight).numpy()
        W, bias = jm.joiner.weight.numpy(), jm.joiner.bias.numpy()
        ref = rnnt_beam_ref(E, P, W, bias, [T, T - 5], blank=blank, beam=4, top_k=4, max_symbols=2)
        best = [hyps[0] for hyps in ref.tokens]
        U = max(max(len(h) for h in best), 1)
        prefix = torch.full((B, U + 1), blank, dtype=torch.long)
        for b, toks in enumerate(best):
            prefix[b, 1:1 + len(toks)] = torch.tensor(toks, dtype=torch.long)
        lp = torch.log_softmax(jm(enc_out, prefix), -1).numpy()   # (B, T, U+1, V)
    assert sum(len(h) for h in best) > 0
    for b in range(B):
        for t in range([T, T - 5][b]):
            for u in range(len(best[b]) + 1):
                last = best[b][u - 1] if u else blank
                np.testing.assert_allclose(rnnt_lp_row(E[b, t], P[last], W, bias), lp[b, t, u],
                                           rtol=0, atol=1e-12)


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


P_ = ctypes.c_void_p(4096)   # never dereferenced: validation fails before any launch


def _frames(lib, dtype=0, B=1, T=2, V=8, J=16, blank=0, beam=4, top_k=3, ms=2, enc=P_, state=P_,
            ws=P_, state_bytes=None, ws_bytes=None):
    null = ctypes.c_void_p()
    if state_bytes is None:
        state_bytes = lib.sc_rnnt_beam_state_bytes(B, min(max(beam, 1), 32), min(max(ms, 1), 8), 10)
    if ws_bytes is None:
        ws_bytes = lib.sc_rnnt_beam_workspace_bytes(B, max(V, 1))
    return lib.sc_rnnt_beam_frames(enc, P_, P_, dtype, ctypes.cast(P_, ctypes.POINTER(ctypes.c_float)),
                                   B, T, V, J, T * J, J, null, None, 0, 0, blank, beam, top_k, ms,
                                   state, state_bytes, ws, ws_bytes, null)


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=7), b"dtype"),
    (dict(beam=0), b"beam"),
    (dict(beam=33), b"beam"),
    (dict(top_k=0), b"top_k"),
    (dict(top_k=33, V=64), b"top_k"),
    (dict(ms=0), b"max_symbols"),
    (dict(ms=9), b"max_symbols"),
    (dict(blank=8), b"blank"),
    (dict(blank=-1), b"blank"),
    (dict(J=257), b"J=257"),
    (dict(J=0), b"J=0"),
    (dict(V=0), b"shape"),
    (dict(enc=ctypes.c_void_p()), b"null pointer"),
    (dict(state=ctypes.c_void_p()), b"null pointer"),
    (dict(ws=ctypes.c_void_p()), b"null pointer"),
    (dict(state_bytes=5), b"state_bytes"),
    (dict(state_bytes=64), b"state_bytes"),      # a state that is too small
    (dict(ws_bytes=4), b"workspace_bytes"),
])
def test_frames_rejects_bad_arguments_without_gpu(lib, kw, word):
    assert _frames(lib, **kw) == -1
    msg = lib.sc_last_error()
    assert b"sc_rnnt_beam_frames" in msg and word in msg, msg


def test_reset_and_result_reject_bad_arguments_without_gpu(lib):
    null = ctypes.c_void_p()
    n = lib.sc_rnnt_beam_state_bytes(2, 4, 2, 10)

    def err(rc, fn, word):
        msg = lib.sc_last_error()
        assert rc == -1 and fn in msg and word in msg, msg

    rst = lib.sc_rnnt_beam_reset
    err(rst(P_, n, 2, 0, 2, 10, None, null), b"sc_rnnt_beam_reset", b"beam")
    err(rst(P_, n, 2, 33, 2, 10, None, null), b"sc_rnnt_beam_reset", b"beam")
    err(rst(P_, n, 2, 4, 0, 10, None, null), b"sc_rnnt_beam_reset", b"max_symbols")
    err(rst(P_, n, 2, 4, 9, 10, None, null), b"sc_rnnt_beam_reset", b"max_symbols")
    err(rst(P_, n, 2, 4, 2, -1, None, null), b"sc_rnnt_beam_reset", b"max_frames")
    err(rst(null, n, 2, 4, 2, 10, None, null), b"sc_rnnt_beam_reset", b"null pointer")
    err(rst(P_, n - 8, 2, 4, 2, 10, None, null), b"sc_rnnt_beam_reset", b"state_bytes")
    res = lib.sc_rnnt_beam_result
    fp = ctypes.cast(P_, ctypes.POINTER(ctypes.c_float))
    err(res(P_, n, 2, 40, 2, 1, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result", b"beam")
    err(res(P_, n, 2, 4, 9, 1, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result",
        b"max_symbols")
    err(res(P_, n, 2, 4, 2, 0, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result", b"nbest")
    err(res(P_, n, 2, 4, 2, 5, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result", b"nbest")
    err(res(P_, n, 2, 4, 2, 1, P_, null, -1, P_, fp, null, null), b"sc_rnnt_beam_result", b"cap")
    err(res(null, n, 2, 4, 2, 1, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result",
        b"null pointer")
    err(res(P_, n, 2, 4, 2, 1, null, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result",
        b"null pointer")
    err(res(P_, n, 2, 4, 2, 1, P_, null, 4, null, fp, null, null), b"sc_rnnt_beam_result",
        b"null pointer")
    err(res(P_, n + 4, 2, 4, 2, 1, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result",
        b"state_bytes")
    err(res(P_, 64, 2, 4, 2, 1, P_, null, 4, P_, fp, null, null), b"sc_rnnt_beam_result",
        b"state_bytes")


def test_empty_calls_are_noops(lib):
    null = ctypes.c_void_p()
    assert lib.sc_rnnt_beam_reset(null, 0, 0, 4, 2, 10, None, null) == 0
    assert lib.sc_last_error() == b""
    for B, T in ((0, 5), (2, 0)):
        assert lib.sc_rnnt_beam_frames(null, null, null, 0, None, B, T, 8, 16, 0, 0, null, None, 0,
                                       0, 0, 4, 3, 2, null, 0, null, 0, null) == 0
    assert lib.sc_rnnt_beam_result(null, 0, 0, 4, 2, 1, null, null, 0, null, None, null,
                                   null) == 0
    assert lib.sc_last_error() == b""


def test_state_bytes_grow_with_each_argument(lib):
    sb, wb = lib.sc_rnnt_beam_state_bytes, lib.sc_rnnt_beam_workspace_bytes
    base = sb(2, 4, 2, 10)
    assert 0 < base < sb(3, 4, 2, 10) and base < sb(2, 5, 2, 10) and base < sb(2, 4, 3, 10)
    assert base < sb(2, 4, 2, 11) and base == 2 * sb(1, 4, 2, 10)
    # the trie alone: (parent, token) for the empty prefix and max_frames * max_symbols * beam nodes
    assert sb(1, 4, 2, 10) >= 8 * (1 + 10 * 2 * 4) and sb(1, 4, 2, 11) - sb(1, 4, 2, 10) == 8 * 2 * 4
    assert sb(1, 0, 2, 10) == 0 and sb(1, 33, 2, 10) == 0 and sb(1, 4, 0, 10) == 0
    assert sb(1, 4, 9, 10) == 0 and sb(1, 4, 2, -1) == 0 and sb(-1, 4, 2, 10) == 0
    assert 0 < wb(2, 100) < wb(3, 100) and wb(2, 100) < wb(2, 101)
    assert wb(2, 0) == 0 and wb(-1, 8) == 0
    # the C5 decode shape (B = 32, T = 1500): 6 MB at beam 8, max_symbols 2
    assert sb(32, 8, 2, 1500) == 32 * (16 + 24 * 8 + 8 * (1 + 1500 * 2 * 8)) < 7 << 20


def test_dispatcher_schemas_and_meta_shapes():
    import statecatcher_amd
    from statecatcher_amd import torch_library as tl
    sc = tl.load()
    for name in ("rnnt_beam_state_bytes", "rnnt_beam_reset_", "rnnt_beam_frames_",
                 "rnnt_beam_result", "rnnt_beam_decode"):
        assert name in tl.OPS and hasattr(sc, name)
    for name in ("rnnt_beam_decode", "rnnt_beam_state", "rnnt_beam_result", "rnnt_beam_decoder"):
        assert name in statecatcher_amd.__all__ and hasattr(statecatcher_amd, name)
    s = str(torch.ops.statecatcher.rnnt_beam_decode.default._schema)
    for part in ("Tensor enc_p", "Tensor pred_tab", "Tensor W", "Tensor bias", "Tensor? lengths=None",
                 "Tensor? mask=None", "int blank=0", "int beam=8", "int top_k=8",
                 "int max_symbols=2", "int nbest=1", "int? max_frames=None", "int? cap=None",
                 "-> (Tensor tokens, Tensor lens, Tensor scores, Tensor frames)"):
        assert part in s, (part, s)
    s = str(torch.ops.statecatcher.rnnt_beam_frames_.default._schema)
    for part in ("Tensor enc_p", "Tensor(a!) state", "int top_k=8", "int max_symbols=2", "-> ()"):
        assert part in s, (part, s)
    assert "Tensor(a!) state" in str(torch.ops.statecatcher.rnnt_beam_reset_.default._schema)
    s = str(torch.ops.statecatcher.rnnt_beam_result.default._schema)
    assert "Tensor frames" in s and "Tensor status" in s
    lib_bytes = statecatcher_amd._lib.load().sc_rnnt_beam_state_bytes(1, 8, 2, 20)
    assert sc.rnnt_beam_state_bytes(1, 8, 2, 20) == lib_bytes
    with pytest.raises(RuntimeError, match="beam"):
        sc.rnnt_beam_state_bytes(1, 40, 2, 20)
    with pytest.raises(RuntimeError, match="max_symbols"):
        sc.rnnt_beam_state_bytes(1, 8, 9, 20)
    meta = torch.device("meta")
    B, T, V, J = 3, 20, 37, 64
    E = torch.empty(B, T, J, device=meta, dtype=torch.bfloat16)
    Pt = torch.empty(V, J, device=meta, dtype=torch.bfloat16)
    bias = torch.empty(V, device=meta)
    tok, lens, scores, frames = sc.rnnt_beam_decode(E, Pt, Pt, bias, nbest=4)
    assert tok.shape == frames.shape == (B, 4, 2 * T) and lens.shape == scores.shape == (B, 4)
    assert tok.dtype == lens.dtype == frames.dtype == torch.int32 and scores.dtype == torch.float32
    tok, lens, scores, frames = sc.rnnt_beam_decode(E, Pt, Pt, bias, max_symbols=3, max_frames=9)
    assert tok.shape == (B, 1, 27)
    tok, lens, scores, frames = sc.rnnt_beam_decode(E, Pt, Pt, bias, cap=5)
    assert tok.shape == (B, 1, 5)
    state = torch.empty(B, lib_bytes, device=meta, dtype=torch.uint8)
    tok, lens, scores, frames, status = sc.rnnt_beam_result(state, 8, 2, 2, 6)
    assert tok.shape == frames.shape == (B, 2, 6) and lens.shape == (B, 2) and status.shape == (B,)
    cpu = (torch.zeros(1, 4, J), torch.zeros(V, J), torch.zeros(V, J), torch.zeros(V))
    with pytest.raises((RuntimeError, NotImplementedError)):   # no CPU kernel, no fallback
        sc.rnnt_beam_decode(*cpu)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        statecatcher_amd.rnnt_beam_decode(*cpu)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        statecatcher_amd.rnnt_beam_state(1, 8, 2, 4, "cpu")
