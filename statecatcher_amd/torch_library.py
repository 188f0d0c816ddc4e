"""The hot-path ops as dispatcher ops: ``torch.ops.statecatcher.*`` (csrc/torch_ops.cpp,
``TORCH_LIBRARY(statecatcher, m)``).

The C++ extension registers each op's schema, its HIP kernel (CUDA dispatch key) and a Meta
kernel (shapes only).  This module loads it and registers the autograd formulas over the
``*_bwd`` ops, so the functions below are differentiable, traceable by FakeTensor /
``torch.compile(fullgraph=True)`` and checkable with ``torch.library.opcheck``.  They launch the
same kernels as the ctypes autograd nodes of ``ops.py`` (the training hot path), which stay the
lower-overhead route for eager training.

Reference interfaces (what a ``train.py`` user swaps in):
  lucy_scan   <- rnn_forward_unfused_rmsnorm                        lucyrnn_triton.py:61-73, :180-244
  lucy_scan_masked <- (planned in the reference's README: "proper input masking") lucy_scan that
                 holds the state at masked frames
  decay_scan  <- fused_decay_scan                                    lucyrnn_triton.py:158-177
  layer_norm  <- nn.LayerNorm(D) between layers                      lucyrnn_triton.py:96-97, :136-137
  ctc_loss    <- nn.CTCLoss(blank, reduction='mean', zero_infinity)  train.py:142 (on model.py:70's
                 log_softmax, fused here when is_logits)
  ctc_greedy_decode <- decoder.py:3-30
  mlstm       <- the xLSTM encoder's mLSTM cell (fork mlstm_kernels)  model.py:214-229
  rnnt_joint_nll <- RNNTPredictorJoiner + log_softmax + warp_rnnt      model.py:73-145
  gemm_tn     <- LinearSafe's forward / input-gradient GEMM (bf16)    lucyrnn_triton.py:20-25
  gemm_wgrad  <- LinearSafe / output_proj weight gradient             lucyrnn_triton.py:20-25, :107-109
  clip_adam_  <- clip_grad_norm_(params, 50) + optim.Adam/AdamW.step() train.py:543-552
  rnnt_greedy_decode <- (absent in the reference) greedy decode of RNNTPredictorJoiner, model.py:112-145
  ctc_beam_decode <- (absent in the reference: decoder.py is greedy only) CTC prefix beam search
  rnnt_beam_decode <- (absent in the reference) transducer beam search of RNNTPredictorJoiner
  ctc_align   <- (absent in the reference) CTC forced alignment: path, token spans, scores
  wkv         <- (planned in the reference's README) the RWKV-4 WKV operator with carried state
"""
import os

import torch

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_torch_ops.so")
OPS = ("abi_version", "lucy_scan_fwd", "lucy_scan_bwd", "decay_scan_fwd", "decay_scan_bwd",
       "layer_norm_fwd", "layer_norm_bwd", "ctc_fwd", "ctc_bwd", "ctc_mean", "ctc_greedy_decode",
       "mlstm_fwd", "mlstm_bwd", "mlstm_gate_bwd", "rnnt_joint_fwd", "rnnt_joint_bwd",
       "gemm_tn", "gemm_wgrad", "clip_adam_", "rnnt_greedy_decode", "ctc_beam_state_bytes",
       "ctc_beam_reset_", "ctc_beam_frames_", "ctc_beam_result", "ctc_beam_decode",
       "rnnt_beam_state_bytes", "rnnt_beam_reset_", "rnnt_beam_frames_", "rnnt_beam_result",
       "rnnt_beam_decode", "ctc_align", "wkv_fwd", "wkv_bwd", "lucy_scan_masked_fwd",
       "lucy_scan_masked_bwd")

_LOADED = False


def load():
    """Load the extension (once) and register the autograd formulas.  Raises if it is not built:
    there is no Python fallback for these ops."""
    global _LOADED
    if _LOADED:
        return torch.ops.statecatcher
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"statecatcher TORCH_LIBRARY extension not built: {LIB_PATH} missing "
                           "(make -C statecatcher_amd/csrc)")
    torch.ops.load_library(LIB_PATH)
    _register_autograd()
    _LOADED = True
    return torch.ops.statecatcher


# ------------------------------------------------------------------------------- autograd -----
def _scan_setup(ctx, inputs, output):
    gates, h0, s0, bias, need_ckpt = inputs
    ctx.save_for_backward(gates, output[3], bias)
    ctx.has_bias = bias is not None
    ctx.dtypes = (h0.dtype, s0.dtype, None if bias is None else bias.dtype)


def _scan_backward(ctx, dout, ds_last, dh_last, dckpt):
    gates, ckpt, bias = ctx.saved_tensors
    sc = torch.ops.statecatcher
    B, T = gates.shape[:2]
    D = gates.shape[-1] if gates.dim() == 4 else gates.shape[2] * 64
    if dout is None:
        dout = gates.new_zeros(B, T, D)
    if dh_last is not None:   # h_last is out[:, -1] before rounding: its gradient joins dout's
        dout = dout.clone()
        dout[:, -1] += dh_last.to(dout.dtype)
    want_db = ctx.has_bias and ctx.needs_input_grad[3]
    dgates, dh0, ds0, dbias = sc.lucy_scan_bwd(gates, ckpt, dout, ds_last, bias, want_db)
    hd, sd, bd = ctx.dtypes
    db = None
    if want_db:   # per-row partials [B,7,D] -> the bias's [7,D] (logical g*D + d) order
        db = dbias.sum(0).reshape(bias.shape).to(bd)
    return dgates, dh0.to(hd), ds0.to(sd), db, None


def _scan_masked_setup(ctx, inputs, output):
    gates, h0, s0, mask, bias, need_ckpt = inputs
    ctx.save_for_backward(gates, output[3], mask, bias)
    ctx.has_bias = bias is not None
    ctx.dtypes = (h0.dtype, s0.dtype, None if bias is None else bias.dtype)


def _scan_masked_backward(ctx, dout, ds_last, dh_last, dckpt):
    """h_last is the state after the last live frame, not out[:, -1]: its gradient goes to the
    kernel as the start of the Gh chain."""
    gates, ckpt, mask, bias = ctx.saved_tensors
    B, T = gates.shape[:2]
    D = gates.shape[-1] if gates.dim() == 4 else gates.shape[2] * 64
    if dout is None:
        dout = gates.new_zeros(B, T, D)
    want_db = ctx.has_bias and ctx.needs_input_grad[4]
    dgates, dh0, ds0, dbias = torch.ops.statecatcher.lucy_scan_masked_bwd(
        gates, ckpt, dout, mask, ds_last, dh_last, bias, want_db)
    hd, sd, bd = ctx.dtypes
    db = dbias.sum(0).reshape(bias.shape).to(bd) if want_db else None
    return dgates, dh0.to(hd), ds0.to(sd), None, db, None


def _decay_setup(ctx, inputs, output):
    kv, decay, init = inputs
    ctx.save_for_backward(decay, output, init)
    ctx.init_dtype = None if init is None else init.dtype


def _decay_backward(ctx, dout):
    decay, s_all, init = ctx.saved_tensors
    dkv, ddec, dinit = torch.ops.statecatcher.decay_scan_bwd(decay, s_all, dout, init)
    return dkv, ddec.to(decay.dtype), (dinit.to(ctx.init_dtype) if init is not None else None)


def _ln_setup(ctx, inputs, output):
    x, gamma, beta, eps = inputs
    ctx.save_for_backward(x, gamma, output[1], output[2])
    ctx.pdtypes = (gamma.dtype, beta.dtype)


def _ln_backward(ctx, dy, dmean, drstd):
    x, gamma, mean, rstd = ctx.saved_tensors
    dx, dg, db = torch.ops.statecatcher.layer_norm_bwd(x, dy, gamma, mean, rstd)
    gd, bd = ctx.pdtypes
    return dx, dg.to(gd), db.to(bd), None


def _ctc_setup(ctx, inputs, output):
    x, targets, in_lens, tgt_lens, blank, is_logits = inputs
    ctx.save_for_backward(x, targets, in_lens, tgt_lens, output[0], output[1])
    ctx.meta = (blank, is_logits)


def _ctc_backward(ctx, grad_nll, grad_ws):
    x, targets, in_lens, tgt_lens, nll, ws = ctx.saved_tensors
    blank, is_logits = ctx.meta
    if grad_nll is None:
        return None, None, None, None, None, None
    grad = torch.ops.statecatcher.ctc_bwd(x, targets, in_lens, tgt_lens, nll, ws, grad_nll,
                                          blank, is_logits)
    return grad, None, None, None, None, None


def _mean_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _mean_backward(ctx, grad_loss, grad_factor):
    (factor,) = ctx.saved_tensors
    return (factor * grad_loss if grad_loss is not None else None), None


def _mlstm_setup(ctx, inputs, output):
    q, k, v, ig, fg, c0, n0, m0, eps = inputs
    h, c_last, ns, ms, cs, mrow, den = output
    ctx.save_for_backward(q, k, v, ig, fg, h, cs, ns, ms, mrow, den, c_last)
    ctx.eps = eps
    ctx.has = (c0 is not None, n0 is not None)
    ctx.nc = ns.shape[1] - 1


def _mlstm_backward(ctx, dh, dc_last, dns, dms, dcs, dmrow, dden):
    """Gradients of (h, final C, final n) -- the n / m state outputs beyond the final chunk are
    internal (their gradients are ignored, as the stabiliser is not differentiated)."""
    q, k, v, ig, fg, h, cs, ns, ms, mrow, den, c_last = ctx.saved_tensors
    B, NH, T = q.shape[:3]
    if dh is None:
        dh = torch.zeros_like(h)
    dn_last = None if dns is None else dns[:, ctx.nc].reshape(B, NH, -1)
    dq, dk, dv, dc0, dn0, qdq, kdk = torch.ops.statecatcher.mlstm_bwd(
        q, k, v, ig, fg, h, dh, dc_last, dn_last, cs, ns, ms, mrow, den, ctx.eps)
    # the final state depends on the last forget gate with no query partner: <dC_T, C~_T> +
    # <dn_T, n~_T> joins q.dq - k.dk at T - 1 (ops._mlstm_state_grad_term), only when a state
    # gradient arrives
    if T > 0 and (dc_last is not None or dn_last is not None):
        term = 0.0
        if dc_last is not None:
            term = (dc_last.float() * c_last).flatten(2).sum(-1)
        if dn_last is not None:
            term = term + (dn_last.float() * ns[:, ctx.nc].reshape(B, NH, -1)).sum(-1)
        qdq = torch.cat([qdq[..., :-1], qdq[..., -1:] + term.reshape(B, NH, 1)], -1)
    # d igate_s = k_s.dk_s ; d fgate_t = sigmoid(-f_t) sum_{r >= t} (q_r.dq_r - k_r.dk_r)
    dfg = torch.ops.statecatcher.mlstm_gate_bwd(qdq, kdk, fg)
    has_c0, has_n0 = ctx.has
    return (dq, dk, dv, kdk.to(ig.dtype), dfg.to(fg.dtype), dc0 if has_c0 else None,
            dn0 if has_n0 else None, None, None)


def _joint_setup(ctx, inputs, output):
    enc, pred, W, bias, labels, flen, llen, blank = inputs
    ctx.save_for_backward(enc, pred, W, bias, labels, flen, llen, output[1])
    ctx.blank = blank
    ctx.dtypes = (enc.dtype, pred.dtype, W.dtype, bias.dtype)


def _joint_backward(ctx, grad_nll, grad_ws):
    enc, pred, W, bias, labels, flen, llen, ws = ctx.saved_tensors
    if grad_nll is None:
        return (None,) * 8
    de, dp, dW, db = torch.ops.statecatcher.rnnt_joint_bwd(enc, pred, W, bias, labels, flen, llen,
                                                           ws, grad_nll, ctx.blank)
    ed, pd, wd, bd = ctx.dtypes
    return de.to(ed), dp.to(pd), dW.to(wd), db.to(bd), None, None, None, None


def _wkv_setup(ctx, inputs, output):
    td, tf, k, v = inputs[:4]
    ctx.save_for_backward(td, tf, k, v, output[4])
    ctx.pdt = (td.dtype, tf.dtype)


def _wkv_backward(ctx, dy, dnum, dden, dmax, dckpt):
    """Gradients of y alone: the incoming state is a constant and the outgoing one carries none."""
    td, tf, k, v, ckpt = ctx.saved_tensors
    if dy is None:
        dy = torch.zeros_like(k)
    dtd, dtf, dk, dv = torch.ops.statecatcher.wkv_bwd(td, tf, k, v, dy, ckpt)
    return dtd.to(ctx.pdt[0]), dtf.to(ctx.pdt[1]), dk, dv, None, None, None, None


def _register_autograd():
    reg = torch.library.register_autograd
    reg("statecatcher::lucy_scan_fwd", _scan_backward, setup_context=_scan_setup)
    reg("statecatcher::lucy_scan_masked_fwd", _scan_masked_backward, setup_context=_scan_masked_setup)
    reg("statecatcher::decay_scan_fwd", _decay_backward, setup_context=_decay_setup)
    reg("statecatcher::layer_norm_fwd", _ln_backward, setup_context=_ln_setup)
    reg("statecatcher::ctc_fwd", _ctc_backward, setup_context=_ctc_setup)
    reg("statecatcher::ctc_mean", _mean_backward, setup_context=_mean_setup)
    reg("statecatcher::mlstm_fwd", _mlstm_backward, setup_context=_mlstm_setup)
    reg("statecatcher::rnnt_joint_fwd", _joint_backward, setup_context=_joint_setup)
    reg("statecatcher::wkv_fwd", _wkv_backward, setup_context=_wkv_setup)


# ------------------------------------------------------------------------------- functions ----
def lucy_scan(gates, h0, s0, gate_bias=None):
    """(out [B,T,D] in gates' dtype, s_last fp32, h_last fp32) of the LucyRNN scan over gates
    [B,T,7,D] (the reference layout) or step-blocked [B,T,D/64,7,64]; gate_bias fp32 [7,D] is
    added on load.  Differentiable in gates, h0, s0 and gate_bias."""
    sc = load()
    need = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (gates, h0, s0, gate_bias))
    out, s_last, h_last, _ = sc.lucy_scan_fwd(gates, h0, s0, gate_bias, need)
    return out, s_last, h_last


def lucy_scan_masked(gates, h0, s0, mask, gate_bias=None):
    """lucy_scan with a per-frame mask [B,T] (nonzero = live; bool, integer or float): a held
    frame leaves (h, s) untouched, writes zero to out and gets zero gradient, so each row is the
    scan of its live frames scattered back and (s_last, h_last) is the state after the last live
    frame."""
    sc = load()
    need = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (gates, h0, s0, gate_bias))
    out, s_last, h_last, _ = sc.lucy_scan_masked_fwd(gates, h0, s0, mask, gate_bias, need)
    return out, s_last, h_last


def decay_scan(kv, decay, init=None):
    """s_t = decay_t s_{t-1} + kv_t with s_{-1} = init (zeros if None); fused_decay_scan."""
    return load().decay_scan_fwd(kv, decay, init)


def layer_norm(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm over the last dim in x's dtype with fp32 statistics."""
    return load().layer_norm_fwd(x, gamma, beta, eps)[0]


def ctc_nll(x, targets, in_lens, tgt_lens, blank=0, is_logits=True):
    """Per-sequence CTC negative log-likelihood [B] fp32 (+inf when infeasible)."""
    return load().ctc_fwd(x, targets, in_lens, tgt_lens, blank, is_logits)[0]


def ctc_loss(x, targets, in_lens, tgt_lens, blank=0, is_logits=True):
    """nn.CTCLoss(blank, reduction='mean', zero_infinity=True) (train.py:142)."""
    sc = load()
    nll = sc.ctc_fwd(x, targets, in_lens, tgt_lens, blank, is_logits)[0]
    return sc.ctc_mean(nll, tgt_lens)[0]


def ctc_greedy_decode(log_probs, lengths, blank=0):
    """(tokens int32 [B,T], counts int32 [B]) of decoder.py's greedy CTC decode."""
    return load().ctc_greedy_decode(log_probs, lengths, blank)


def mlstm(q, k, v, igate, fgate, c0=None, n0=None, m0=None, eps=1e-6):
    """transformers' mlstm_chunkwise(return_last_states=True) on the HIP walk kernels:
    (h [B,NH,T,DV], (C [B,NH,DQ,DV], n [B,NH,DQ], m [B,NH,1])).  q, k, v bf16 / f16, gates fp32
    [B,NH,T]; differentiable in q, k, v, the gates, c0 and n0."""
    h, c_last, ns, ms, _, _, _ = load().mlstm_fwd(q, k, v, igate, fgate, c0, n0, m0, eps)
    B, NH = q.shape[:2]
    return h, (c_last, ns[:, -1].reshape(B, NH, -1), ms[:, -1].reshape(B, NH, 1))


def wkv(time_decay, time_first, k, v, state=None):
    """(y [B,T,C], (num, den, max) fp32 [B,C]) of the RWKV-4 WKV operator (ops.wkv) from the state
    (num, den, max), or the empty state.  Differentiable in time_decay, time_first, k and v; the
    state is a constant going in and carries no gradient coming out."""
    sc = load()
    if state is not None and any(s.requires_grad for s in state):
        raise ValueError("wkv: the incoming state is a constant (detach it); it must not require grad")
    need = torch.is_grad_enabled() and any(t.requires_grad for t in (time_decay, time_first, k, v))
    n0, d0, m0 = state if state is not None else (None, None, None)
    y, num, den, mx, _ = sc.wkv_fwd(time_decay, time_first, k, v, n0, d0, m0, need)
    return y, (num.detach(), den.detach(), mx.detach())


def rnnt_joint_nll(enc_p, pred_p, W, bias, labels, frames_lengths, labels_lengths, blank=0):
    """Per-sequence RNN-T nll [B] of the fused joiner (RNNTPredictorJoiner's joint, log_softmax,
    warp_rnnt's gathered lattice) without materialising the (B, T, U+1, V) logits."""
    return load().rnnt_joint_fwd(enc_p, pred_p, W, bias, labels, frames_lengths, labels_lengths,
                                 blank)[0]


def rnnt_greedy_decode(enc_p, pred_tab, W, bias, lengths=None, mask=None, blank=0, max_symbols=4,
                       prev=None, cap=None, return_frames=False):
    """(tokens int32 [B,cap], counts int32 [B][, frames int32 [B,cap]]) of the greedy transducer
    decode (ops.rnnt_greedy_decode); prev int32 [B] is updated in place when given."""
    tokens, counts, frames = load().rnnt_greedy_decode(enc_p, pred_tab, W, bias, lengths, mask,
                                                       blank, max_symbols, prev, cap, return_frames)
    return (tokens, counts, frames) if return_frames else (tokens, counts)


def ctc_beam_decode(x, lengths=None, mask=None, blank=0, beam=8, top_k=8, nbest=1, is_logits=False,
                    max_frames=None, cap=None):
    """(tokens int32 [B,nbest,cap], lens int32 [B,nbest], scores fp32 [B,nbest]) of the offline
    CTC prefix beam search (ops.ctc_beam_decode with state=None)."""
    return load().ctc_beam_decode(x, lengths, mask, blank, beam, top_k, nbest, is_logits,
                                  max_frames, cap)


def ctc_beam_state(B, beam, max_frames, device):
    """A reset state tensor (uint8 [B, bytes per stream]) for ctc_beam_frames_ / ctc_beam_result."""
    sc = load()
    state = torch.zeros(B, sc.ctc_beam_state_bytes(1, beam, max_frames), dtype=torch.uint8,
                        device=device)
    sc.ctc_beam_reset_(state, beam, max_frames)
    return state


def ctc_beam_reset_(state, beam, max_frames, streams=None):
    """Every stream of ``state`` (or those with a non-zero entry in streams fp32 [B]) afresh."""
    load().ctc_beam_reset_(state, beam, max_frames, streams)
    return state


def ctc_beam_frames_(x, state, lengths=None, mask=None, blank=0, beam=8, top_k=8, is_logits=False):
    """Consume x [B,T,V] as the next chunk of every stream of ``state``, in place."""
    load().ctc_beam_frames_(x, state, lengths, mask, blank, beam, top_k, is_logits)
    return state


def ctc_beam_result(state, beam, nbest=1, cap=0):
    """(tokens [B,nbest,cap], lens [B,nbest], scores [B,nbest], status [B]) of a state."""
    return load().ctc_beam_result(state, beam, nbest, cap)


def ctc_align(x, targets, in_lens, tgt_lens, blank=0, is_logits=False):
    """(states int32 [B,T], labels int32 [B,T], frame_lp fp32 [B,T], spans int32 [B,U_max,2],
    token_lp fp32 [B,U_max], score fp32 [B]) of the CTC forced alignment (ops.ctc_align).  Not
    differentiable."""
    return load().ctc_align(x, targets, in_lens, tgt_lens, blank, is_logits)


def rnnt_beam_decode(enc_p, pred_tab, W, bias, lengths=None, mask=None, blank=0, beam=8, top_k=8,
                     max_symbols=2, nbest=1, max_frames=None, cap=None, return_frames=False):
    """(tokens int32 [B,nbest,cap], lens int32 [B,nbest], scores fp32 [B,nbest][, frames]) of the
    offline transducer beam search (ops.rnnt_beam_decode with state=None)."""
    tok, lens, scores, frames = load().rnnt_beam_decode(enc_p, pred_tab, W, bias, lengths, mask,
                                                        blank, beam, top_k, max_symbols, nbest,
                                                        max_frames, cap)
    return (tok, lens, scores, frames) if return_frames else (tok, lens, scores)


def rnnt_beam_state(B, beam, max_symbols, max_frames, device):
    """A reset state tensor (uint8 [B, bytes per stream]) for rnnt_beam_frames_ / rnnt_beam_result."""
    sc = load()
    state = torch.zeros(B, sc.rnnt_beam_state_bytes(1, beam, max_symbols, max_frames),
                        dtype=torch.uint8, device=device)
    sc.rnnt_beam_reset_(state, beam, max_symbols, max_frames)
    return state


def rnnt_beam_reset_(state, beam, max_symbols, max_frames, streams=None):
    """Every stream of ``state`` (or those with a non-zero entry in streams fp32 [B]) afresh."""
    load().rnnt_beam_reset_(state, beam, max_symbols, max_frames, streams)
    return state


def rnnt_beam_frames_(enc_p, pred_tab, W, bias, state, lengths=None, mask=None, blank=0, beam=8,
                      top_k=8, max_symbols=2):
    """Consume enc_p [B,T,J] as the next chunk of every stream of ``state``, in place."""
    load().rnnt_beam_frames_(enc_p, pred_tab, W, bias, state, lengths, mask, blank, beam, top_k,
                             max_symbols)
    return state


def rnnt_beam_result(state, beam, max_symbols, nbest=1, cap=0):
    """(tokens [B,nbest,cap], lens [B,nbest], scores [B,nbest], frames [B,nbest,cap], status [B])
    of a state."""
    return load().rnnt_beam_result(state, beam, max_symbols, nbest, cap)


def gemm_tn(a, b, tile_m=0):
    """C [M,N] bf16 = a [M,K] b [N,K]^T on the persistent MFMA kernel (K % 64 == 0, N % 256 == 0;
    include/statecatcher.h sc_gemm_tn_bf16).  Not differentiable: a building block of the
    projection nodes' forward and input gradient."""
    return load().gemm_tn(a, b, tile_m)


def gemm_wgrad(dy, x, block_d=0):
    """dW [N,K] fp32 = dy [M,N]^T x [M,K] (bf16 operands) on the split-L MFMA kernel plus the
    fixed-order slab sum; block_d = D: dy's columns in step-blocked gate order, dW returned in
    the reference's row order.  Raises outside the kernel's tiling (sc_gemm_wgrad_splits)."""
    return load().gemm_wgrad(dy, x, block_d)


def clip_adam_(params, grads, exp_avgs, exp_avg_sqs, n_clip, max_norm, lr, betas, eps,
               weight_decay, decoupled, step):
    """clip_grad_norm_(params[:n_clip], max_norm) then one Adam (decoupled=False) / AdamW step
    at step count `step` on every tensor, in place (params, exp_avgs, exp_avg_sqs; grads read
    only), as optim.clip_and_adam_step does for an optimizer.  Returns clip_grad_norm_'s total
    norm (0-dim fp32 tensor; 0 without clipping)."""
    import math
    beta1, beta2 = betas
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return load().clip_adam_(list(params), list(grads), list(exp_avgs), list(exp_avg_sqs),
                             int(n_clip), float(max_norm), float(lr), float(beta1), float(beta2),
                             float(eps), float(weight_decay), bool(decoupled), lr / bc1,
                             math.sqrt(bc2))
