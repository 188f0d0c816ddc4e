"""CPU checks of the CTC forced alignment (csrc/ctc_align.hip, sc_ctc_align): the numpy restatement
tests/ctc_align_ref.py against brute-force enumeration of every alignment, its tie rule on exact
arithmetic, and what the library, the dispatcher op and the package export -- argument checks run
before any launch, so none of this needs a GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.ctc_align_ref import (brute_force, ctc_align_ref, drift, log_probs, min_feasible_len,
                                 tie_cases, tie_rule_path)


def test_reference_matches_enumeration_of_every_alignment():
    """All T <= 6, U <= 3 over V = 3 (labels 1, 2, every transcript, repeats included)."""
    rng = np.random.default_rng(0)
    seen_infeasible = seen_repeat = 0
    for T in range(0, 7):
        for U in range(0, 4):
            for tg in itertools.product((1, 2), repeat=U):
                x = 2.0 * rng.standard_normal((T, 3))
                lp = log_probs(x, True, np.float64)
                best, paths = brute_force(lp, tg)
                ref = ctc_align_ref(x, tg)
                if T < min_feasible_len(tg) or (T == 0 and U > 0):
                    assert best == -np.inf and not ref.feasible and ref.score == -np.inf
                    assert (ref.states == -1).all() and (ref.spans == -1).all()
                    seen_infeasible += 1
                    continue
                assert ref.feasible and abs(ref.score - best) <= 1e-12 * max(1.0, abs(best))
                if T == 0:
                    continue
                assert len(paths) == 1 and ref.states.tolist() == paths[0]
                seen_repeat += any(a == b for a, b in zip(tg, tg[1:]))
                # what the path implies for the other outputs
                assert abs(ref.frame_lp.sum() - best) <= 1e-12 * max(1.0, abs(best))
                for u in range(U):
                    s, e = ref.spans[u]
                    assert (ref.states[s:e] == 2 * u + 1).all() and (ref.labels[s:e] == tg[u]).all()
                    assert abs(ref.token_lp[u] - ref.frame_lp[s:e].mean()) < 1e-12
                # the margin: the second-best complete alignment is at least that far behind
                if np.isfinite(ref.margin):
                    second = _second_best(lp, tg, paths[0])
                    assert second <= best - ref.margin + 1e-12
    assert seen_infeasible > 10 and seen_repeat > 10


def _second_best(lp, tg, best_path):
    S = 2 * len(tg) + 1
    ext = [0 if s % 2 == 0 else tg[s // 2] for s in range(S)]
    T = lp.shape[0]
    out = -np.inf

    def walk(t, s, score, path):
        nonlocal out
        score += lp[t, ext[s]]
        path = path + [s]
        if t == T - 1:
            if (s in (S - 1, S - 2) or S == 1) and path != best_path:
                out = max(out, score)
            return
        for d in (0, 1, 2):
            n = s + d
            if n < S and not (d == 2 and (n % 2 == 0 or ext[n] == ext[s])):
                walk(t + 1, n, score, path)

    for s0 in range(min(2, S)):
        walk(0, s0, 0.0, [])
    return out


def test_tie_rule_on_exact_arithmetic():
    """Integer log-probs: fp32 and fp64 sums are exact, ties are exact, and of the tied best paths
    the contract returns the one with the smaller move at every tie."""
    x, targets, in_lens, tgt_lens = tie_cases()
    tied = 0
    for b in range(len(x)):
        xb, tg = x[b, :in_lens[b]], targets[b, :tgt_lens[b]]
        best, paths = brute_force(xb, tg)
        for dtype in (np.float64, np.float32):
            ref = ctc_align_ref(xb, tg, is_logits=False, dtype=dtype)
            if not paths:
                assert not ref.feasible
                continue
            assert ref.score == best and ref.states.tolist() == tie_rule_path(paths)
        if len(paths) > 1:
            tied += 1
            assert ref.margin == 0.0
    assert tied >= 8   # the cases do exercise the rule


def test_fp32_reference_drift_is_small_when_recentred():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((300, 64))
    tg = rng.integers(1, 64, 100)
    a, b = ctc_align_ref(x, tg), ctc_align_ref(x, tg, dtype=np.float32)
    d32, e32 = drift(a, b)
    assert 0 < d32 < 1e-3 and 0 < e32 < 1e-5
    assert abs(a.score - b.score) <= 8 * e32 * 300 + 1e-6 * abs(a.score)


def test_new_names_are_exported():
    import statecatcher_amd
    from statecatcher_amd import _lib
    from statecatcher_amd import torch_library as tl
    for name in ("sc_ctc_align", "sc_ctc_align_workspace_bytes"):
        assert name in _lib.EXPORTED
    assert "ctc_align" in tl.OPS and hasattr(tl, "ctc_align")
    for name in ("ctc_align", "ctc_forced_align"):
        assert name in statecatcher_amd.__all__ and hasattr(statecatcher_amd, name)
    assert _lib.ABI_VERSION == 14   # two functions added, no signature or struct changed


@pytest.fixture(scope="module")
def lib():
    from statecatcher_amd import _lib
    return _lib.load()


P = ctypes.c_void_p(4096)   # never dereferenced: validation fails before any launch
NULL = ctypes.c_void_p()


def _align(lib, dtype=0, B=2, T=5, V=8, umax=3, blank=0, x=P, targets=P, in_lens=P, tgt_lens=P,
           states=P, frame_lp=P, spans=P, token_lp=P, score=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sc_ctc_align_workspace_bytes(B, T, min(max(umax, 0), 1007))
    return lib.sc_ctc_align(x, dtype, 1, B, T, V, T * V, V, targets, umax, umax, in_lens, tgt_lens,
                            blank, states, frame_lp, spans, token_lp, score, ws, ws_bytes, NULL)


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=7), b"dtype"),
    (dict(B=-1), b"shape"),
    (dict(V=0), b"shape"),
    (dict(umax=-1), b"shape"),
    (dict(umax=1008), b"1007"),
    (dict(blank=8), b"blank"),
    (dict(blank=-1), b"blank"),
    (dict(x=NULL), b"null pointer"),
    (dict(targets=NULL), b"null pointer"),
    (dict(in_lens=NULL), b"null pointer"),
    (dict(tgt_lens=NULL), b"null pointer"),
    (dict(states=NULL), b"null pointer"),
    (dict(frame_lp=NULL), b"null pointer"),
    (dict(spans=NULL), b"null pointer"),
    (dict(token_lp=NULL), b"null pointer"),
    (dict(score=NULL), b"null pointer"),
    (dict(ws=NULL), b"null pointer"),
    (dict(ws=ctypes.c_void_p(4100)), b"aligned"),
    (dict(ws_bytes=16), b"workspace_bytes"),
])
def test_align_rejects_bad_arguments_without_gpu(lib, kw, word):
    assert _align(lib, **kw) == -1
    msg = lib.sc_last_error()
    assert b"sc_ctc_align" in msg and word in msg, msg


def test_empty_batch_is_a_noop_and_sizes_grow(lib):
    assert _align(lib, B=0, x=NULL, targets=NULL, in_lens=NULL, tgt_lens=NULL, states=NULL,
                  frame_lp=NULL, spans=NULL, token_lp=NULL, score=NULL, ws=NULL, ws_bytes=0) == 0
    assert lib.sc_last_error() == b""
    wb = lib.sc_ctc_align_workspace_bytes
    base = wb(2, 40, 9)
    assert 0 < base < wb(3, 40, 9) and base < wb(2, 400, 9) and base < wb(2, 40, 90)
    assert wb(2, 40, 1008) == 0 and wb(-1, 40, 9) == 0 and wb(2, -1, 9) == 0 and wb(2, 40, -1) == 0
    assert wb(2, 0, 9) > 0 and wb(2, 40, 1007) > 0
    # emission rows, and 2 bits per state and frame: half a byte per (frame, pair)
    assert base >= 2 * 40 * 10 * 4 + 2 * 5 * 10 * 4
    # the flagship shape: 29 MB of emission rows + 3.6 MB of decisions for 32 sequences
    assert wb(32, 1500, 150) < 34 << 20


def test_dispatcher_schema_and_meta_shapes():
    from statecatcher_amd import torch_library as tl
    sc = tl.load()
    assert hasattr(sc, "ctc_align")
    s = str(torch.ops.statecatcher.ctc_align.default._schema)
    for part in ("Tensor x", "Tensor targets", "Tensor in_lens", "Tensor tgt_lens", "int blank=0",
                 "bool is_logits=False", "Tensor states", "Tensor labels", "Tensor frame_lp",
                 "Tensor spans", "Tensor token_lp", "Tensor score"):
        assert part in s, (part, s)
    meta = torch.device("meta")
    B, T, V, U = 3, 20, 37, 6
    x = torch.empty(B, T, V, device=meta, dtype=torch.bfloat16)
    tg = torch.empty(B, U, device=meta, dtype=torch.int64)
    n = torch.empty(B, device=meta, dtype=torch.int64)
    states, labels, frame_lp, spans, token_lp, score = sc.ctc_align(x, tg, n, n)
    assert states.shape == labels.shape == frame_lp.shape == (B, T)
    assert spans.shape == (B, U, 2) and token_lp.shape == (B, U) and score.shape == (B,)
    assert states.dtype == labels.dtype == spans.dtype == torch.int32
    assert frame_lp.dtype == token_lp.dtype == score.dtype == torch.float32
    with pytest.raises(RuntimeError, match="1007"):
        sc.ctc_align(x, torch.empty(B, 1008, device=meta, dtype=torch.int64), n, n)
