"""CPU checks of the greedy transducer decoder (csrc/rnnt_decode.hip, sc_rnnt_greedy_decode):

* the fp64 helper tests/rnnt_decode_ref.py decides, at every lattice node it visits, what the
  argmax of the joiner users train (RNNTPredictorJoiner.forward on the decoded prefix) decides;
* sc_rnnt_greedy_decode validates its arguments before launching and names the offender;
* the dispatcher op has its schema and its Meta kernel gives the documented shapes.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.rnnt_decode_ref import rnnt_greedy_ref


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_helper_agrees_with_the_trained_joiner(seed):
    from statecatcher_amd.model import RNNTPredictorJoiner
    torch.manual_seed(seed)
    B, T, D, V, J, blank, ms = 2, 12, 6, 11, 8, 0, 3
    jm = RNNTPredictorJoiner(D, 5, J, V).double()
    with torch.no_grad():
        jm.joiner.bias[blank] += 0.3
        jm.joiner.weight *= 3.0   # spread the logits: emissions and blanks both occur
        enc_out = torch.randn(B, T, D, dtype=torch.float64)
        E = jm.enc_proj(enc_out).numpy()
        P = jm.pred_proj(jm.embedding.weight).numpy()
        lens = [T, T - 5]
        ref = rnnt_greedy_ref(E, P, jm.joiner.weight.numpy(), jm.joiner.bias.numpy(), lens,
                              blank=blank, max_symbols=ms)
        U = max(int(ref.counts.max()), 1)
        prefix = torch.full((B, U + 1), blank, dtype=torch.long)
        for b, toks in enumerate(ref.tokens):
            prefix[b, 1:1 + len(toks)] = torch.tensor(toks, dtype=torch.long)
        logits = jm(enc_out, prefix).numpy()   # (B, T, U+1, V)
    assert ref.counts.sum() > 0 and any(k == blank for p in ref.path for _, _, k in p)
    assert ref.min_gap > 1e-9
    for b in range(B):
        assert len(ref.path[b]) > 0
        for t, u, k in ref.path[b]:
            assert int(np.argmax(logits[b, t, u])) == k, (b, t, u)
        assert all(t < lens[b] for t, _, _ in ref.path[b])
        assert ref.frames[b] == sorted(ref.frames[b])
        assert sum(ref.per_frame[b]) == ref.counts[b] and max(ref.per_frame[b]) <= ms


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


def _call(lib, dtype=0, B=1, T=1, V=8, J=64, blank=0, max_symbols=4, cap=4, counts=1):
    """sc_rnnt_greedy_decode with non-null dummy pointers (validation fails before any launch)."""
    p = ctypes.c_void_p(64)
    null = ctypes.c_void_p()
    return lib.sc_rnnt_greedy_decode(p, p, p, dtype, p, B, T, V, J, T * J, J, null, null, 0, 0,
                                     blank, max_symbols, null, p, null, cap,
                                     p if counts else null, null)


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=7), b"dtype"),
    (dict(max_symbols=0), b"max_symbols"),
    (dict(max_symbols=65), b"max_symbols"),
    (dict(blank=8), b"blank"),
    (dict(blank=-1), b"blank"),
    (dict(counts=0), b"counts"),
    (dict(cap=-1), b"cap"),
    (dict(J=257), b"J="),
    (dict(V=0), b"shape"),
])
def test_capi_rejects_bad_arguments_without_gpu(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.sc_last_error()
    assert b"sc_rnnt_greedy_decode" in msg and word in msg, msg


def test_capi_empty_batch_is_a_noop(lib):
    null = ctypes.c_void_p()
    assert lib.sc_rnnt_greedy_decode(null, null, null, 0, null, 0, 5, 8, 64, 0, 0, null, null, 0, 0,
                                     0, 4, null, null, null, 0, null, null) == 0
    assert lib.sc_last_error() == b""


def test_dispatcher_schema_and_meta_shapes():
    from statecatcher_amd import torch_library as tl
    sc = tl.load()
    assert "rnnt_greedy_decode" in tl.OPS and hasattr(sc, "rnnt_greedy_decode")
    s = str(torch.ops.statecatcher.rnnt_greedy_decode.default._schema)
    for part in ("Tensor? lengths=None", "Tensor? mask=None", "int blank=0", "int max_symbols=4",
                 "prev=None", "int? cap=None", "bool return_frames=False"):
        assert part in s, (part, s)
    meta = torch.device("meta")
    B, T, V, J = 3, 20, 37, 64
    e = torch.empty(B, T, J, device=meta, dtype=torch.bfloat16)
    w = torch.empty(V, J, device=meta, dtype=torch.bfloat16)
    bias = torch.empty(V, device=meta)
    tok, cnt, frm = sc.rnnt_greedy_decode(e, w, w, bias, None, None, 0, 3, None, None, True)
    assert tok.shape == frm.shape == (B, T * 3) and cnt.shape == (B,)
    assert tok.dtype == cnt.dtype == frm.dtype == torch.int32
    tok, cnt, frm = sc.rnnt_greedy_decode(e, w, w, bias, cap=7)
    assert tok.shape == (B, 7) and frm.shape == (B, 0)
    with pytest.raises((RuntimeError, NotImplementedError)):   # no CPU kernel, no fallback
        sc.rnnt_greedy_decode(torch.zeros(1, 2, J), torch.zeros(V, J), torch.zeros(V, J),
                              torch.zeros(V))
