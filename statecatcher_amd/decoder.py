"""Drop-in of /root/reference/decoder.py:3-30 running on the GPU (one host copy, no per-frame sync),
and the transducer counterpart the reference does not have."""
import torch

from .ops import ctc_align, ctc_beam_decode, ctc_greedy_decode, rnnt_beam_decode, rnnt_greedy_decode


def ctc_greedy_decoder(log_probs, input_lengths, blank=0):
    """log_probs [B,T,V], input_lengths [B] -> List[List[int]] (argmax, trim, collapse, drop blank)."""
    tokens, counts = ctc_greedy_decode(log_probs, input_lengths, blank)
    tokens = tokens.cpu()
    counts = counts.cpu().tolist()
    return [tokens[b, :c].tolist() for b, c in enumerate(counts)]


def ctc_beam_decoder(log_probs, input_lengths, blank=0, beam=8, top_k=8, nbest=1,
                     return_scores=False):
    """CTC prefix beam search of log_probs [B,T,V] (ops.ctc_beam_decode: every frame extends each
    hypothesis by its top_k likeliest tokens and keeps the ``beam`` best).  nbest=1 returns the
    List[List[int]] of ctc_greedy_decoder; nbest>1 a list per stream of up to nbest token lists,
    best first.  return_scores adds the log-probabilities in the same nesting.  One host copy at
    the end."""
    tokens, lens, scores = ctc_beam_decode(log_probs, input_lengths, blank=blank, beam=beam,
                                           top_k=top_k, nbest=nbest)
    B, N, cap = tokens.shape
    packed = torch.cat([lens.unsqueeze(2), scores.view(torch.int32).unsqueeze(2), tokens], 2).cpu()
    lens, scores = packed[:, :, 0].tolist(), packed[:, :, 1].contiguous().view(torch.float32).tolist()
    hyps = [[packed[b, n, 2:2 + lens[b][n]].tolist() for n in range(N) if lens[b][n] >= 0]
            for b in range(B)]
    scs = [[scores[b][n] for n in range(N) if lens[b][n] >= 0] for b in range(B)]
    if nbest == 1:
        hyps, scs = [h[0] if h else [] for h in hyps], [s[0] if s else float("-inf") for s in scs]
    return (hyps, scs) if return_scores else hyps


def ctc_forced_align(log_probs, targets, input_lengths, target_lengths, blank=0, is_logits=False):
    """CTC forced alignment of the padded transcripts targets [B,U_max] to log_probs [B,T,V]
    (ops.ctc_align: the Viterbi path through the CTC lattice) -> one dict per stream:
      score            the path's total log-probability (-inf: the transcript cannot be aligned)
      score_per_frame  score / max(T_b, 1)
      tokens           [(token, start, end, mean_lp), ...]: frames [start, end) and the mean
                       log-probability the path takes there, per transcript token
      labels           the token per frame (blank between tokens), T_b entries
    An infeasible stream has empty lists.  A segment whose score_per_frame, or whose lowest
    mean_lp, is under a threshold of the caller's choosing is a candidate hallucinated or shifted
    transcript.  One host copy at the end."""
    states, labels, _, spans, token_lp, score = ctc_align(log_probs, targets, input_lengths,
                                                          target_lengths, blank, is_logits)
    B, T = labels.shape
    U = spans.shape[1]
    tgt = targets.to(device=labels.device, dtype=torch.int32).reshape(B, U)
    packed = torch.cat([score.view(torch.int32).unsqueeze(1), labels, spans.reshape(B, 2 * U),
                        token_lp.view(torch.int32), tgt], 1).cpu()
    scores = packed[:, 0].contiguous().view(torch.float32).tolist()
    labs = packed[:, 1:1 + T]
    sp = packed[:, 1 + T:1 + T + 2 * U].reshape(B, U, 2)
    tlp = packed[:, 1 + T + 2 * U:1 + T + 3 * U].contiguous().view(torch.float32)
    tg = packed[:, 1 + T + 3 * U:]
    out = []
    for b in range(B):
        Tb = int((labs[b] >= 0).sum())
        n = int((sp[b, :, 0] >= 0).sum())
        if scores[b] == float("-inf"):
            Tb = n = 0
        toks = [(t, s, e, m) for t, (s, e), m in zip(tg[b, :n].tolist(), sp[b, :n].tolist(),
                                                     tlp[b, :n].tolist())]
        # (an infeasible stream has no labelled frame: -inf / 1 stays -inf)
        out.append({"score": scores[b], "score_per_frame": scores[b] / max(Tb, 1),
                    "tokens": toks, "labels": labs[b, :Tb].tolist()})
    return out


def rnnt_joiner_tables(joiner, dtype=None):
    """(pred_tab [V,J], W [V,J], bias fp32 [V]) of an RNNTPredictorJoiner /
    RNNTCompactPredictorJoiner for ops.rnnt_greedy_decode: the stateless predictor's output for
    every possible previous token, and the output projection.  dtype: of pred_tab and W (default:
    the joiner's own)."""
    jm = getattr(joiner, "module", joiner)   # DDP-wrapped or not
    with torch.no_grad():
        pred_tab = jm.pred_proj(jm.embedding.weight)
        W = jm.joiner.weight.detach()
        dtype = dtype or W.dtype
        return (pred_tab.to(dtype).contiguous(), W.to(dtype).contiguous(),
                jm.joiner.bias.detach().float().contiguous())


def rnnt_greedy_decoder(enc_out, joiner, input_lengths, blank=0, max_symbols=4, return_frames=False):
    """Greedy transducer decode of encoder output enc_out [B,T,D] with ``joiner`` (either joiner
    class of model.py) -> List[List[int]], plus the frame index of every token when asked.
    Streams start at ``blank`` as compute_loss's predictor prefix does; at most max_symbols tokens
    per frame.  enc_proj and the [V,J] predictor table are computed once per call, the decode is
    one launch (ops.rnnt_greedy_decode, fp32 arithmetic) and there is one host copy at the end."""
    jm = getattr(joiner, "module", joiner)
    with torch.no_grad():
        enc_p = jm.enc_proj(enc_out)
        pred_tab, W, bias = rnnt_joiner_tables(jm, enc_p.dtype)
        out = rnnt_greedy_decode(enc_p, pred_tab, W, bias, lengths=input_lengths, blank=blank,
                                 max_symbols=max_symbols, return_frames=return_frames)
    n = len(out)
    packed = torch.cat([out[1].unsqueeze(1)] + [t for i, t in enumerate(out) if i != 1], 1).cpu()
    counts = packed[:, 0].tolist()
    cap = out[0].shape[1]
    toks = [packed[b, 1:1 + c].tolist() for b, c in enumerate(counts)]
    if n == 2:
        return toks
    return toks, [packed[b, 1 + cap:1 + cap + c].tolist() for b, c in enumerate(counts)]


def rnnt_beam_decoder(enc_out, joiner, input_lengths, blank=0, beam=8, top_k=8, max_symbols=2,
                      nbest=1, return_scores=False, return_frames=False):
    """Transducer beam search of encoder output enc_out [B,T,D] with ``joiner`` (either joiner
    class of model.py; ops.rnnt_beam_decode, fp32 arithmetic).  nbest=1 returns the List[List[int]]
    of rnnt_greedy_decoder; nbest>1 a list per stream of up to nbest token lists, best first.
    return_scores adds the log-probabilities and return_frames the live-frame index of every
    token, each in the same nesting: (hyps[, scores][, frames]).  The cost of a frame grows with
    max_symbols + 1 joint rounds, and a trained transducer of this project emits about 0.1 tokens
    per frame, so max_symbols defaults to 2 (the greedy decoder's 4 buys nothing here).  enc_proj
    and the predictor table (rnnt_joiner_tables) are computed once per call; one host copy at the
    end."""
    jm = getattr(joiner, "module", joiner)
    with torch.no_grad():
        enc_p = jm.enc_proj(enc_out)
        pred_tab, W, bias = rnnt_joiner_tables(jm, enc_p.dtype)
        out = rnnt_beam_decode(enc_p, pred_tab, W, bias, lengths=input_lengths, blank=blank,
                               beam=beam, top_k=top_k, max_symbols=max_symbols, nbest=nbest,
                               return_frames=return_frames)
    tokens, lens, scores = out[:3]
    B, N, cap = tokens.shape
    parts = [lens.unsqueeze(2), scores.view(torch.int32).unsqueeze(2), tokens] + list(out[3:])
    packed = torch.cat(parts, 2).cpu()
    lens, scores = packed[:, :, 0].tolist(), packed[:, :, 1].contiguous().view(torch.float32).tolist()
    alive = [[n for n in range(N) if lens[b][n] >= 0] for b in range(B)]
    hyps = [[packed[b, n, 2:2 + lens[b][n]].tolist() for n in alive[b]] for b in range(B)]
    res = [hyps]
    if return_scores:
        res.append([[scores[b][n] for n in alive[b]] for b in range(B)])
    if return_frames:
        res.append([[packed[b, n, 2 + cap:2 + cap + lens[b][n]].tolist() for n in alive[b]]
                    for b in range(B)])
    if nbest == 1:
        empty = [[], float("-inf"), []]
        kinds = [0] + ([1] if return_scores else []) + ([2] if return_frames else [])
        res = [[r[0] if r else empty[k] for r in part] for part, k in zip(res, kinds)]
    return tuple(res) if len(res) > 1 else res[0]
