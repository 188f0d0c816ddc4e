"""The callers of the hot path, with the reference's signatures (model.py:11-110, :282-398).

`compute_loss` / `ASRModel` / `detach_states` keep /root/reference/model.py's call pattern so
the reference train.py segment loop drives them unchanged.  Only the LucyRNN encoders are
built here (the hot path); the CTC branch runs the fused HIP CTC when the criterion is
statecatcher_amd.model.CTCLoss and otherwise exactly the reference's
`log_softmax -> transpose -> criterion` sequence.
"""
from typing import Any, Optional

import torch
import torch.nn as nn

from .lucyrnn_conf import LucyRNNConfig
from .lucyrnn_triton import DEFERRED_LOGITS, LucyRNNtriton, defer_output_head
from .xlstm import xLSTMLarge, xLSTMLargeConfig
from .rwkv import RWKVConfig, RWKVEncoder
from .ops import ctc_head_loss, ctc_head_supported, ctc_loss, rnnt_joint_loss, rnnt_joint_supported, rnnt_loss


def detach_states(states):
    """Recursively detach tensors in nested dict/tuple/list states (model.py:11-25)."""
    if states is None:
        return None
    if isinstance(states, torch.Tensor):
        return states.detach()
    if isinstance(states, dict):
        return {k: detach_states(v) for k, v in states.items()}
    if isinstance(states, tuple):
        return tuple(detach_states(s) for s in states)
    if isinstance(states, list):
        return [detach_states(s) for s in states]
    return states


def assert_all_detached(x):
    """model.py:27-35."""
    if isinstance(x, torch.Tensor):
        assert not x.requires_grad, "Tensor still requires grad"
    elif isinstance(x, (list, tuple)):
        for v in x:
            assert_all_detached(v)
    elif isinstance(x, dict):
        for v in x.values():
            assert_all_detached(v)


class CTCLoss(nn.Module):
    """nn.CTCLoss(blank, reduction, zero_infinity) on the HIP alpha-beta kernels.

    forward(log_probs [T,B,V], targets [B,U], input_lengths, target_lengths) follows
    nn.CTCLoss's interface (train.py:142); forward_logits(logits [B,T,V], ...) fuses the
    log_softmax that model.py:70 applies first and skips the transpose.
    """

    def __init__(self, blank=0, reduction="mean", zero_infinity=True, fused_head=True):
        super().__init__()
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity
        # compute_loss under bf16 autocast: the encoder's output projection joins the loss
        # (ops.CTCHeadFn, fp32 logits) when reduction is the training criterion's
        self.fuse_output_head = fused_head

    def fused_head(self):
        return self.fuse_output_head and self.reduction == "mean" and self.zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs.transpose(0, 1), targets, input_lengths, target_lengths,
                        blank=self.blank, reduction=self.reduction,
                        zero_infinity=self.zero_infinity, is_logits=False)

    def forward_logits(self, logits, targets, input_lengths, target_lengths):
        return ctc_loss(logits, targets, input_lengths, target_lengths, blank=self.blank,
                        reduction=self.reduction, zero_infinity=self.zero_infinity,
                        is_logits=True)


def compute_loss(mode: str, criterion: nn.Module, model: nn.Module, feats: torch.Tensor,
                 masks: torch.Tensor, tokens: torch.Tensor, in_lens, tgt_lens, blank_id: int,
                 use_rnnt_joiner: Optional[nn.Module] = None, input_state: Optional[Any] = None,
                 args=None, compact=False):
    """model.py:37-110: returns (loss, output_state, enc_out, output_state)."""
    if input_state:
        input_state = detach_states(input_state)
        if args is not None and getattr(args, "debug", False):
            assert_all_detached(input_state)
    fuse_head = (mode == "ctc" and isinstance(criterion, CTCLoss) and criterion.fused_head()
                 and feats.is_cuda and torch.is_autocast_enabled("cuda")
                 and torch.get_autocast_dtype("cuda") == torch.bfloat16)
    if fuse_head:
        # the LucyRNNtriton encoder hands its output projection to the loss (ops.CTCHeadFn):
        # fp32 logits into the lattice, a bf16 gradient straight into the projection backward
        with defer_output_head() as head:
            enc_out, output_state = model(feats, masks, input_state)
        if enc_out is DEFERRED_LOGITS:
            x, proj, imgs, wide = head.taken
            if not ctc_head_supported(x, proj.weight, proj.bias, imgs):
                enc_out = proj(x.contiguous(), imgs)   # the encoder's own (unfused) projection
                return criterion.forward_logits(enc_out, tokens, in_lens, tgt_lens), \
                    output_state, enc_out, output_state
            with torch.autocast("cuda", enabled=False):
                loss, enc_out = ctc_head_loss(x, proj.weight, proj.bias, imgs, tokens, in_lens,
                                              tgt_lens, blank=criterion.blank, wide=wide)
            return loss, output_state, enc_out, output_state
    else:
        enc_out, output_state = model(feats, masks, input_state)
    if mode == "ctc":
        if isinstance(criterion, CTCLoss):
            loss = criterion.forward_logits(enc_out, tokens, in_lens, tgt_lens)
        else:
            logp = enc_out.log_softmax(-1).transpose(0, 1)
            loss = criterion(logp, tokens, in_lens, tgt_lens)
    elif mode == "rnnt":
        # model.py:73-105: blank-prefixed predictor input, joiner logits (B,T,U+1,V) or compact
        # rows, log_softmax in fp32, transducer loss with gather semantics
        assert use_rnnt_joiner is not None, "Joiner module required for RNN-T mode"
        blank_prefix = torch.full((tokens.size(0), 1), blank_id, dtype=tokens.dtype,
                                  device=tokens.device)
        predictor_input = torch.cat([blank_prefix, tokens], dim=1)
        use_compact = bool(getattr(args, "compact_rnnt", False)) if args is not None else compact
        jm = getattr(use_rnnt_joiner, "module", use_rnnt_joiner)   # DDP-wrapped or not
        if isinstance(criterion, RNNTLoss) and enc_out.is_cuda and criterion.use_fused_joint() \
                and rnnt_joint_supported(jm.joiner.in_features, jm.joiner.out_features):
            # fused joiner + log_softmax + lattice (rnnt.hip joint_*): the (B, T, U+1, V) logits
            # are never materialised; same value as the compact and dense paths below
            enc_p, pred_p, W, bias = (use_rnnt_joiner(enc_out, predictor_input, in_lens, tgt_lens,
                                                      project_only=True) if use_compact else
                                      use_rnnt_joiner(enc_out, predictor_input, project_only=True))
            loss = criterion.forward_joint(enc_p, pred_p, W, bias, tokens, in_lens, tgt_lens,
                                           blank_id=blank_id)
            return loss, output_state, enc_out, output_state
        if use_compact:
            logits = use_rnnt_joiner(enc_out, predictor_input, in_lens, tgt_lens)
        else:
            logits = use_rnnt_joiner(enc_out, predictor_input)
        if isinstance(criterion, RNNTLoss):
            # the log_softmax is fused into the loss kernels (no fp32 copy of the 4-D logits)
            loss = criterion.forward_logits(logits, tokens, in_lens, tgt_lens, blank_id=blank_id,
                                            compact=use_compact)
        else:
            log_probs = logits.log_softmax(dim=-1)
            if log_probs.dtype != torch.float32:
                log_probs = log_probs.to(torch.float32)
            loss = criterion(log_probs=log_probs, labels=tokens, frames_lengths=in_lens,
                             labels_lengths=tgt_lens, blank_id=blank_id, compact=compact,
                             gather=True)
    else:
        raise ValueError(f"Unknown mode: {mode}")
    return loss, output_state, enc_out, output_state


class RNNTLoss(nn.Module):
    """The transducer loss the reference takes from warp_rnnt (train.py:38-42, :144), as a
    module accepting model.py:97-105's keyword call (blank given as ``blank_id``).  SURVEY F8:
    the reference assigns the class itself as criterion, so its call constructs a module instead
    of computing a loss; this is the intended loss (warp_rnnt.rnnt_loss, reduction 'mean')."""

    def __init__(self, blank=0, reduction="mean", average_frames=False, fused_joint=None):
        super().__init__()
        self.blank = blank
        self.reduction = reduction
        self.average_frames = average_frames
        # fused joiner + loss (ops.RNNTJointFn) rounds W and tanh(enc + pred) to bf16 before its
        # MFMAs.  None: only where the step already computes in a 16-bit autocast dtype; fp32
        # training keeps the reference's fp32 logits (materialised path).  True / False force it.
        self.fused_joint = fused_joint

    def use_fused_joint(self):
        if self.fused_joint is not None:
            return bool(self.fused_joint)
        # bf16 autocast only: the fused kernels round W and z to bf16, coarser than the 10-bit
        # mantissa of a float16 autocast run (the reference's own training dtype, train.py:516),
        # which keeps the materialised joiner in float16
        return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16

    def forward(self, log_probs, labels, frames_lengths, labels_lengths, blank_id=None,
                compact=False, gather=True):
        return rnnt_loss(log_probs, labels, frames_lengths, labels_lengths,
                         average_frames=self.average_frames, reduction=self.reduction,
                         blank=self.blank if blank_id is None else blank_id, gather=gather,
                         compact=compact, is_logits=False)

    def forward_logits(self, logits, labels, frames_lengths, labels_lengths, blank_id=None,
                       compact=False):
        return rnnt_loss(logits, labels, frames_lengths, labels_lengths,
                         average_frames=self.average_frames, reduction=self.reduction,
                         blank=self.blank if blank_id is None else blank_id, compact=compact,
                         is_logits=True)

    def forward_joint(self, enc_p, pred_p, W, bias, labels, frames_lengths, labels_lengths,
                      blank_id=None):
        """The loss straight from the joiner's projections (ops.RNNTJointFn)."""
        return rnnt_joint_loss(enc_p, pred_p, W, bias, labels, frames_lengths, labels_lengths,
                               blank=self.blank if blank_id is None else blank_id,
                               reduction=self.reduction, average_frames=self.average_frames)


class RNNTPredictorJoiner(nn.Module):
    """model.py:112-145: embedding predictor + additive joint + tanh + output projection over
    the full (B, T, U+1) grid.  Parameter names as the reference (embedding, enc_proj,
    pred_proj, joiner).  debug prints are off by default here."""

    def __init__(self, enc_out_dim: int, pred_emb_dim: int, join_dim: int, vocab_size: int,
                 debug: bool = False):
        super().__init__()
        self.embedding = nn.Embedding(vocab_size, pred_emb_dim)
        self.enc_proj = nn.Linear(enc_out_dim, join_dim)
        self.pred_proj = nn.Linear(pred_emb_dim, join_dim)
        self.debug = debug
        self.joiner = nn.Linear(join_dim, vocab_size)

    def forward(self, enc_out: torch.Tensor, prefix: torch.Tensor, project_only: bool = False):
        pred = self.pred_proj(self.embedding(prefix))            # (B, U+1, J)
        enc = self.enc_proj(enc_out)                             # (B, T, J)
        if project_only:   # inputs of the fused joiner + loss (compute_loss); through forward()
            return enc, pred, self.joiner.weight, self.joiner.bias   # so DDP sees the call
        joint = torch.tanh(enc.unsqueeze(2) + pred.unsqueeze(1))  # (B, T, U+1, J)
        return self.joiner(joint)                                # (B, T, U+1, V)


class RNNTCompactPredictorJoiner(nn.Module):
    """model.py:147-200: the joint only over each sequence's valid (T_b, U_b+1) nodes, packed
    to (sum_b T_b (U_b+1), V) rows in (b, t, u) order."""

    def __init__(self, enc_out_dim: int, pred_emb_dim: int, join_dim: int, vocab_size: int,
                 debug: bool = False):
        super().__init__()
        self.embedding = nn.Embedding(vocab_size, pred_emb_dim)
        self.enc_proj = nn.Linear(enc_out_dim, join_dim)
        self.pred_proj = nn.Linear(pred_emb_dim, join_dim)
        self.joiner = nn.Linear(join_dim, vocab_size)
        self.debug = debug

    def forward_compact(self, enc_out, prefix, in_lens, tgt_lens):
        enc = self.enc_proj(enc_out)
        pred = self.pred_proj(self.embedding(prefix))
        rows = []
        for b in range(enc_out.size(0)):
            T, U = int(in_lens[b]), int(tgt_lens[b]) + 1
            rows.append(torch.tanh(enc[b, :T].unsqueeze(1) + pred[b, :U].unsqueeze(0))
                        .reshape(T * U, -1))
        return self.joiner(torch.cat(rows, 0))

    def forward(self, enc_out, prefix, in_lens, tgt_lens, project_only: bool = False):
        if project_only:   # the fused path needs no packing: it never builds the rows
            return (self.enc_proj(enc_out), self.pred_proj(self.embedding(prefix)),
                    self.joiner.weight, self.joiner.bias)
        return self.forward_compact(enc_out, prefix, in_lens, tgt_lens)


class ASRModel(nn.Module):
    """model.py:282-398, LucyRNN branch: optional input projection, zero-masking of padded
    frames, encoder call with/without carried state.

    masking: "zero" (the reference: padded frames are zeroed, the recurrence still steps over
    them) or "hold" (LucyRNN only: the features are zeroed as before and the mask also goes to
    the encoder, whose scans hold (h, s) at masked frames, so padding does not decay the state
    carried to the next segment)."""

    def __init__(self, frontend: Optional[nn.Module], encoder, vocab_size: int, feat_dim: int,
                 proj_dim: int, debug: bool = False, masking: str = "zero"):
        super().__init__()
        if masking not in ("zero", "hold"):
            raise ValueError(f'masking must be "zero" or "hold", got {masking!r}')
        if masking == "hold" and not isinstance(encoder, LucyRNNConfig):
            raise NotImplementedError('masking="hold" is implemented for the LucyRNN encoder only '
                                      f"(got {type(encoder).__name__})")
        self.masking = masking
        self.frontend = frontend
        self.debug = debug
        if isinstance(encoder, xLSTMLargeConfig):   # model.py:301-307
            self.cfg = encoder
            self.encoder = xLSTMLarge(self.cfg)
            self.enc_out_dim = vocab_size
            self.input_seq_pad_factor = 64
            if proj_dim > 0:
                self.proj = nn.Linear(feat_dim, proj_dim)
        elif isinstance(encoder, LucyRNNConfig):
            self.cfg = encoder
            self.encoder = LucyRNNtriton(self.cfg)
            if masking == "hold":
                self.encoder.mask_mode = "hold"
            self.enc_out_dim = vocab_size
            self.input_seq_pad_factor = 8
            if proj_dim > 0:
                self.proj = nn.Linear(feat_dim, proj_dim)
        elif isinstance(encoder, RWKVConfig):
            # (the reference's README plans an RWKV encoder; its model.py builds none)
            self.cfg = encoder
            self.encoder = RWKVEncoder(self.cfg)
            self.enc_out_dim = vocab_size
            self.input_seq_pad_factor = 1   # any T: no time padding
            if proj_dim > 0:
                self.proj = nn.Linear(feat_dim, proj_dim)
        else:
            raise ValueError(f"Unknown encoder provided: {type(encoder)}")

    def forward(self, feats, mask, states=None):
        if hasattr(self, "proj"):
            feats = self.proj(feats)
        if isinstance(self.encoder, xLSTMLarge) and self.encoder.config.mode != "inference":
            # (mode="inference" takes any T: its remainder runs on the step kernel, and zero
            # frames would advance the carried state)
            # model.py:341-347: pad time to the 64-step chunk.  The reference then multiplies by
            # the UNPADDED mask (a broadcast error whenever T % 64 != 0); the mask is padded
            # with zeros here so padded frames are zero, as intended.
            rem = feats.size(1) % self.input_seq_pad_factor
            if rem:
                pad = self.input_seq_pad_factor - rem
                feats = torch.nn.functional.pad(feats, (0, 0, 0, pad))
                if mask is not None:
                    mask = torch.nn.functional.pad(mask, (0, pad))
        if mask is not None:
            feats = feats * mask.unsqueeze(-1).to(feats.dtype)
        if self.masking == "hold" and mask is not None:
            logits, new_states = self.encoder(feats, states, masks=mask)
        elif states is not None:
            logits, new_states = self.encoder(feats, states)
        else:
            logits, new_states = self.encoder(feats)
        return logits, new_states


def build_xlstm_config(feat_dim, vocab_size, num_heads=2, num_blocks=3, embedding_dim=None,
                       autocast_kernel_dtype="float16"):
    """model.py:214-229: the xLSTM config train.py builds (embedding_dim = input_dim = feat_dim
    in the reference; C4 uses a 768-wide model behind the input projection).  The reference
    passes autocast_kernel_dtype="float16" (model.py:227), and so does this builder by default:
    the mLSTM cell then computes in fp16 (on the bf16 projection, ops.MLSTMCoreFn)."""
    return xLSTMLargeConfig(embedding_dim=embedding_dim or feat_dim, input_dim=feat_dim,
                            num_heads=num_heads, num_blocks=num_blocks, vocab_size=vocab_size,
                            return_last_states=True, mode="train",
                            autocast_kernel_dtype=autocast_kernel_dtype)


def build_lucyrnn_config(input_dim, hidden_size, num_layers, vocab_size, is_training=True):
    """model.py:231-245: the LucyRNN config train.py builds (triton kernel, fused ops, no LN)."""
    return LucyRNNConfig(input_dim=input_dim, hidden_dim=hidden_size, num_layers=num_layers,
                         vocab_size=vocab_size, return_last_states=True, kernel_impl="triton",
                         fused_ops=True, stack_order=1, layer_norm=False, is_training=is_training)


def build_rwkv_config(feat_dim, vocab_size, hidden_size, num_layers):
    """The RWKV-4 encoder config in the builders' style (attention width = hidden_size,
    intermediate = 4 * hidden_size: the published RWKV-4 proportions)."""
    return RWKVConfig(input_dim=feat_dim, hidden_size=hidden_size, num_layers=num_layers,
                      vocab_size=vocab_size, return_last_states=True)
