"""The RWKV-4 encoder on the HIP WKV kernels (csrc/wkv.hip), stateful over segments.

The reference's README names RWKV among its recurrent encoders ("Planned/WiP": its code has
none).  This is the RWKV-4 block stack of transformers' ``RwkvModel`` (modeling_rwkv.py: RwkvBlock,
RwkvSelfAttention, RwkvFeedForward) behind an input projection in place of the token embedding and
an output projection to the vocabulary, with the encoders' calling convention here:
``forward(x [B,T,input_dim], state=None) -> (logits [B,T,vocab], state)``.

``blocks`` carries transformers' parameter names and shapes, so
``encoder.blocks.load_state_dict(hf_model.blocks.state_dict())`` loads a published RWKV-4 stack.

The state is a tuple ``(x_att, x_ffn, num, den, max)``, each ``[L, B, C]``: the last post-ln1 and
post-ln2 frame of every block (what the time-shift mixes read at the next segment's first frame)
and the WKV state (fp32).  Any T >= 1: a sequence fed in pieces with the state carried equals the
sequence fed whole, down to one frame at a time.  The WKV operator runs on ``ops.wkv``; the
linears, LayerNorms and elementwise mixes are PyTorch's.

``step`` is the same encoder frame by frame for streaming decode: K frames of B streams on the
step kernels of csrc/rwkv_step.hip (the recurrent WKV step with the receptance gate, the fused
residual / LayerNorm / shift / mix kernel, the squared ReLU) and the frame GEMM, the state
advanced in place, frames with ``live == 0`` held, no gradient.  streaming.StreamingRWKV replays
it on static buffers.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import ops

EMPTY_MAX = -1e38   # transformers' sentinel for the empty WKV state


@dataclass
class RWKVConfig:
    input_dim: int
    hidden_size: int
    num_layers: int
    vocab_size: int
    attention_hidden_size: Optional[int] = None   # None: hidden_size
    intermediate_size: Optional[int] = None       # None: 4 * hidden_size
    layer_norm_epsilon: float = 1e-5
    return_last_states: bool = True


def _shift(x, prev):
    """x delayed by one frame, its first frame taken from the carried ``prev`` [B,C]."""
    return torch.cat([prev.to(x.dtype).unsqueeze(1), x[:, :-1]], 1)


def _mix(x, shifted, m):
    return x * m + shifted * (1 - m)


class RWKVSelfAttention(nn.Module):
    """transformers' RwkvSelfAttention (time mix): parameter names and shapes kept."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H = cfg.hidden_size
        A = cfg.attention_hidden_size or H
        L = cfg.num_layers
        self.time_decay = nn.Parameter(torch.empty(A))
        self.time_first = nn.Parameter(torch.empty(A))
        self.time_mix_key = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_value = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_receptance = nn.Parameter(torch.empty(1, 1, H))
        self.key = nn.Linear(H, A, bias=False)
        self.value = nn.Linear(H, A, bias=False)
        self.receptance = nn.Linear(H, A, bias=False)
        self.output = nn.Linear(A, H, bias=False)
        # the published RWKV-4 initialisation
        r0 = layer_id / max(L - 1, 1)
        r1 = 1.0 - layer_id / L
        x = (torch.arange(H, dtype=torch.float64) / H).reshape(1, 1, H)
        h = torch.arange(A, dtype=torch.float64)
        with torch.no_grad():
            self.time_decay.copy_(-5.0 + 8.0 * (h / max(A - 1, 1)) ** (0.7 + 1.3 * r0))
            self.time_first.copy_(math.log(0.3) + ((h + 1) % 3 - 1) * 0.5)
            self.time_mix_key.copy_(x ** r1)
            self.time_mix_value.copy_(x ** r1 + 0.3 * r0)
            self.time_mix_receptance.copy_(x ** (0.5 * r1))

    def forward(self, x, x_prev, wkv_state):
        s = _shift(x, x_prev)
        k = self.key(_mix(x, s, self.time_mix_key))
        v = self.value(_mix(x, s, self.time_mix_value))
        r = torch.sigmoid(self.receptance(_mix(x, s, self.time_mix_receptance)))
        if v.dtype != k.dtype:
            v = v.to(k.dtype)
        y, wkv_state = ops.wkv(self.time_decay, self.time_first, k, v, wkv_state)
        return self.output(r * y.to(r.dtype)), wkv_state


class RWKVFeedForward(nn.Module):
    """transformers' RwkvFeedForward (channel mix, squared ReLU)."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H = cfg.hidden_size
        I = cfg.intermediate_size or 4 * H
        self.time_mix_key = nn.Parameter(torch.empty(1, 1, H))
        self.time_mix_receptance = nn.Parameter(torch.empty(1, 1, H))
        self.key = nn.Linear(H, I, bias=False)
        self.receptance = nn.Linear(H, H, bias=False)
        self.value = nn.Linear(I, H, bias=False)
        r1 = 1.0 - layer_id / cfg.num_layers
        x = (torch.arange(H, dtype=torch.float64) / H).reshape(1, 1, H)
        with torch.no_grad():
            self.time_mix_key.copy_(x ** r1)
            self.time_mix_receptance.copy_(x ** r1)

    def forward(self, x, x_prev):
        s = _shift(x, x_prev)
        k = torch.square(torch.relu(self.key(_mix(x, s, self.time_mix_key))))
        r = torch.sigmoid(self.receptance(_mix(x, s, self.time_mix_receptance)))
        return r * self.value(k)


class RWKVBlock(nn.Module):
    """transformers' RwkvBlock: (pre_ln at layer 0,) ln1 + attention, ln2 + feed_forward, residuals."""

    def __init__(self, cfg: RWKVConfig, layer_id: int):
        super().__init__()
        H, eps = cfg.hidden_size, cfg.layer_norm_epsilon
        if layer_id == 0:
            self.pre_ln = nn.LayerNorm(H, eps=eps)
        self.ln1 = nn.LayerNorm(H, eps=eps)
        self.ln2 = nn.LayerNorm(H, eps=eps)
        self.attention = RWKVSelfAttention(cfg, layer_id)
        self.feed_forward = RWKVFeedForward(cfg, layer_id)
        self.layer_id = layer_id

    def forward(self, h, x_att, x_ffn, wkv_state):
        """h [B,T,H]; x_att / x_ffn [B,H]; wkv_state (num, den, max) [B,A].  Returns (h, last
        post-ln1 frame, last post-ln2 frame, wkv state)."""
        if self.layer_id == 0:
            h = self.pre_ln(h)
        a = self.ln1(h)
        att, wkv_state = self.attention(a, x_att, wkv_state)
        h = h + att
        f = self.ln2(h)
        h = h + self.feed_forward(f, x_ffn)
        return h, a[:, -1], f[:, -1], wkv_state


class RWKVEncoder(nn.Module):
    def __init__(self, cfg: RWKVConfig):
        super().__init__()
        self.config = cfg
        self.input_proj = nn.Linear(cfg.input_dim, cfg.hidden_size)
        self.blocks = nn.ModuleList(RWKVBlock(cfg, l) for l in range(cfg.num_layers))
        self.ln_out = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_epsilon)
        self.output_proj = nn.Linear(cfg.hidden_size, cfg.vocab_size)

    # ------------------------------------------------------------------------- state ----------
    def zero_state(self, B, device=None, dtype=torch.float32):
        """The state before the first frame: zero shift frames, the empty WKV state."""
        cfg = self.config
        L, H = cfg.num_layers, cfg.hidden_size
        A = cfg.attention_hidden_size or H
        device = device if device is not None else self.input_proj.weight.device
        return (torch.zeros(L, B, H, dtype=dtype, device=device),
                torch.zeros(L, B, H, dtype=dtype, device=device),
                torch.zeros(L, B, A, dtype=torch.float32, device=device),
                torch.zeros(L, B, A, dtype=torch.float32, device=device),
                torch.full((L, B, A), EMPTY_MAX, dtype=torch.float32, device=device))

    @staticmethod
    def state_from_hf(state):
        """transformers' state list [ffn shift, attention shift, num, den, max], each [B,C,L]
        -> (x_att, x_ffn, num, den, max), each [L,B,C]."""
        x_ffn, x_att, num, den, mx = (s.permute(2, 0, 1).contiguous() for s in state)
        return x_att, x_ffn, num.float(), den.float(), mx.float()

    @staticmethod
    def state_to_hf(state):
        """The inverse of state_from_hf."""
        x_att, x_ffn, num, den, mx = (s.permute(1, 2, 0).contiguous() for s in state)
        return [x_ffn, x_att, num, den, mx]

    # ------------------------------------------------------------------------- step path ------
    # K frames of B streams on the recurrent kernels of csrc/rwkv_step.hip: what
    # streaming.StreamingRWKV replays per block.  Per block of the stack, on the frame engine:
    #     mix        h += the previous block's sigmoid(r) * value(k); (pre_ln;) ln1; shift; 3 mixes
    #     k / v / r  one multi-job lucy_frame_gemm launch
    #     WKV step   y = sigmoid(r) * wkv(k, v), the state in place
    #     output     lucy_frame_gemm
    #     mix        h += output; ln2; shift; 2 mixes
    #     key / receptance   one multi-job launch
    #     squared ReLU       in place
    #     value      lucy_frame_gemm
    # 8 launches for the block's K frames; the encoder adds the input projection(s), the final
    # mix (the last residual and ln_out) and the output projection.
    def _step_ks(self, input_proj=None):
        cfg = self.config
        H = cfg.hidden_size
        ks = [cfg.input_dim, H, cfg.attention_hidden_size or H, cfg.intermediate_size or 4 * H]
        if input_proj is not None:
            ks.append(input_proj.in_features)
        return ks

    def step_gemm_frame_ok(self, input_proj=None):
        """Whether every GEMM of step() fits ops.lucy_frame_gemm (step_weights(gemm="frame"))."""
        from .xlstm import step_gemm_frame_ok
        return step_gemm_frame_ok(*self._step_ks(input_proj))

    def step_weights(self, dtype, input_proj=None, gemm="auto"):
        """A detached snapshot for step(): every linear weight cast to ``dtype`` once, the
        LayerNorm, mix and decay parameters in fp32.  input_proj: an nn.Linear applied before the
        encoder's own (ASRModel.proj).  gemm: "frame" (ops.lucy_frame_gemm: fp32 activations,
        arithmetic per row independent of the block size; fp32 / bf16 weights, every reduction
        length a multiple of 8 and at most 2048), "library" (the library GEMM in ``dtype``,
        activations in ``dtype``), or "auto": "frame" where its limits hold."""
        if gemm not in ("auto", "library", "frame"):
            raise ValueError('gemm must be "auto", "library" or "frame"')
        ok = self.step_gemm_frame_ok(input_proj) and dtype in (torch.float32, torch.bfloat16)
        if gemm == "auto":
            gemm = "frame" if ok else "library"
        frame = gemm == "frame"
        if frame and not ok:
            raise ValueError('gemm="frame" needs fp32 / bf16 weights and every reduction length '
                             'a multiple of 8, at most 2048; use gemm="library"')
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("step_weights: fp32 or bf16 (the step kernels' operand types)")
        dev = self.input_proj.weight.device
        cast = lambda t: t.detach().to(dtype).contiguous()   # noqa: E731
        f32 = lambda t: t.detach().float().reshape(-1).contiguous()   # noqa: E731
        ln = lambda m: (f32(m.weight), f32(m.bias))   # noqa: E731
        zeros = {}

        def bias(m):
            """fp32 and never None for the frame engine (a shared zero row for the bias-free
            linears); in the weight dtype, or None, for the library GEMM."""
            if m.bias is not None:
                return f32(m.bias) if frame else cast(m.bias)
            if not frame:
                return None
            n = m.weight.shape[0]
            if n not in zeros:
                zeros[n] = torch.zeros(n, dtype=torch.float32, device=dev)
            return zeros[n]

        lin = lambda m: (cast(m.weight), bias(m))   # noqa: E731
        w = {"dtype": dtype, "frame": frame, "gemm": gemm, "act": torch.float32 if frame else dtype,
             "eps": float(self.config.layer_norm_epsilon), "emb": lin(self.input_proj),
             "out": lin(self.output_proj), "ln_out": ln(self.ln_out), "blocks": []}
        if input_proj is not None:
            w["in"] = lin(input_proj)
        for blk in self.blocks:
            at, ff = blk.attention, blk.feed_forward
            w["blocks"].append({
                "pre_ln": ln(blk.pre_ln) if blk.layer_id == 0 else None,
                "ln1": ln(blk.ln1), "ln2": ln(blk.ln2),
                "att_mix": (f32(at.time_mix_key), f32(at.time_mix_value),
                            f32(at.time_mix_receptance)),
                "td": f32(at.time_decay), "tf": f32(at.time_first),
                "key": lin(at.key), "value": lin(at.value), "receptance": lin(at.receptance),
                "output": lin(at.output),
                "ffn_mix": (f32(ff.time_mix_key), f32(ff.time_mix_receptance)),
                "ffn_key": lin(ff.key), "ffn_receptance": lin(ff.receptance),
                "ffn_value": lin(ff.value)})
        return w

    def step_workspace(self, B, K, weights, device=None):
        """The static buffers of one step() call of K frames of B streams, all [K,B,width]: the
        input ``x`` and the ``live`` mask (fp32), the residual rows, the activations between the
        kernels (fp32 on the frame engine, the weight dtype on the library engine) and the fp32
        ``logits``.  A caller that keeps it (StreamingRWKV) runs step's launches with no
        allocation, which is what lets the block be captured."""
        cfg, w = self.config, weights
        H = cfg.hidden_size
        A = cfg.attention_hidden_size or H
        I = cfg.intermediate_size or 4 * H
        dev = device if device is not None else self.input_proj.weight.device
        act, f32 = w["act"], torch.float32
        z = lambda n, dt=act: torch.zeros(K, B, n, dtype=dt, device=dev)   # noqa: E731
        Din = w["in"][0].shape[1] if "in" in w else cfg.input_dim
        ws = {"x": z(Din, f32), "live": torch.ones(K, B, dtype=f32, device=dev), "h": z(H, f32),
              "m0": z(H), "m1": z(H), "m2": z(H), "k": z(A), "v": z(A), "r": z(A), "y": z(A),
              "att": z(H), "fk": z(I), "fr": z(H), "fv": z(H), "hout": z(H),
              "logits": z(cfg.vocab_size, f32)}
        if "in" in w:
            ws["p"] = z(cfg.input_dim)
        if act != f32:   # the library engine in bf16: its GEMMs read and write the weight dtype
            ws["xc"], ws["emb"], ws["lg"] = z(Din), z(H), z(cfg.vocab_size)
        return ws

    @staticmethod
    def _step_gemm(w, jobs, stream):
        """y = x W^T + b for every (x [K,B,n], (W, b), y [K,B,m]) of ``jobs``: one (multi-job)
        lucy_frame_gemm launch on the frame engine, the library GEMM per job otherwise."""
        flat = [(x.view(-1, x.shape[-1]), wb, y.view(-1, y.shape[-1])) for x, wb, y in jobs]
        if not w["frame"]:
            for x, (wt, b), y in flat:
                if b is None:
                    torch.mm(x, wt.t(), out=y)
                else:
                    torch.addmm(b, x, wt.t(), out=y)
        elif len(flat) == 1:
            x, (wt, b), y = flat[0]
            ops.lucy_frame_gemm(ops.FRAME_PLAIN, x, wt, b, y)
        else:
            ops.lucy_frame_gemm_multi(ops.FRAME_PLAIN, w["dtype"],
                                      [ops.frame_gemm_job(x, wt, b, y) for x, (wt, b), y in flat],
                                      stream)

    def _step_block(self, ws, state, live, w):
        """step() on the buffers of a workspace: ws["x"] [K,B,Din] -> ws["logits"] [K,B,V], the
        state in place.  live: ws["live"], or None for all frames live.  A linear chain of
        launches on the current stream with no allocation."""
        x_att, x_ffn, num, den, mx = state
        eps, frame = w["eps"], w["frame"]
        stream = ops._lib.stream_of(ws["x"])
        tr = lambda t: t.transpose(0, 1)   # noqa: E731  ([K,B,n] buffer -> the ops' [B,K,n])
        lv = None if live is None else live.t()
        gemm = lambda *jobs: self._step_gemm(w, jobs, stream)   # noqa: E731
        x = ws["x"]
        if "xc" in ws:
            ws["xc"].copy_(x)
            x = ws["xc"]
        if "in" in w:
            gemm((x, w["in"], ws["p"]))
            x = ws["p"]
        h = ws["h"]
        if "emb" in ws:
            gemm((x, w["emb"], ws["emb"]))
            h.copy_(ws["emb"])
        else:
            gemm((x, w["emb"], h))
        add = gate = None
        for l, bw in enumerate(w["blocks"]):
            ops.rwkv_step_mix(tr(h), bw["ln1"], x_att[l], bw["att_mix"],
                              [tr(ws["m0"]), tr(ws["m1"]), tr(ws["m2"])], add=add, gate=gate,
                              pre_ln=bw["pre_ln"], live=lv, eps=eps)
            gemm((ws["m0"], bw["key"], ws["k"]), (ws["m1"], bw["value"], ws["v"]),
                 (ws["m2"], bw["receptance"], ws["r"]))
            ops.wkv_step(bw["td"], bw["tf"], tr(ws["k"]), tr(ws["v"]), (num[l], den[l], mx[l]),
                         r=tr(ws["r"]), live=lv, out=tr(ws["y"]))
            gemm((ws["y"], bw["output"], ws["att"]))
            ops.rwkv_step_mix(tr(h), bw["ln2"], x_ffn[l], bw["ffn_mix"],
                              [tr(ws["m0"]), tr(ws["m1"])], add=tr(ws["att"]), live=lv, eps=eps)
            gemm((ws["m0"], bw["ffn_key"], ws["fk"]), (ws["m1"], bw["ffn_receptance"], ws["fr"]))
            ops.relu_sq_(ws["fk"])
            gemm((ws["fk"], bw["ffn_value"], ws["fv"]))
            add, gate = tr(ws["fv"]), tr(ws["fr"])
        ops.rwkv_step_mix(tr(h), w["ln_out"], None, (), [tr(ws["hout"])], add=add, gate=gate,
                          live=lv, eps=eps)
        if "lg" in ws:
            gemm((ws["hout"], w["out"], ws["lg"]))
            ws["logits"].copy_(ws["lg"])
        else:
            gemm((ws["hout"], w["out"], ws["logits"]))

    def _check_step_state(self, state, B):
        cfg = self.config
        L, H = cfg.num_layers, cfg.hidden_size
        A = cfg.attention_hidden_size or H
        if len(state) != 5:
            raise ValueError("RWKVEncoder.step: state must be (x_att, x_ffn, num, den, max)")
        for name, s, C in zip(("x_att", "x_ffn", "num", "den", "max"), state, (H, H, A, A, A)):
            if tuple(s.shape) != (L, B, C) or s.dtype != torch.float32 or not s.is_contiguous():
                raise ValueError(f"RWKVEncoder.step: state {name} must be a contiguous fp32 "
                                 f"[L,B,C]=({L},{B},{C}) tensor (it is updated in place); got "
                                 f"{s.dtype} {tuple(s.shape)}")

    @torch.no_grad()
    def step(self, x, state=None, live=None, weights=None, workspace=None):
        """K frames x [B,K,input_dim] through the whole encoder on the recurrent step kernels: any
        K >= 1.  Returns (logits fp32 [B,K,V], state); the five state tensors (fp32, contiguous;
        None: zero_state is made) are advanced IN PLACE.  live [B,K]: frames with 0 hold every
        block's state (their logits are not meaningful), so a stream with held frames equals the
        same stream with those frames removed.  weights: step_weights() (default: taken now, in
        the autocast dtype under autocast, else x's dtype).  workspace: step_workspace(B, K,
        weights) to run without allocation (the logits are then a view of its buffer).  The
        analogue of xLSTMLarge.step.  No gradient."""
        from .xlstm import _step_dtype
        if x.dim() != 3 or x.shape[1] < 1:
            raise ValueError(f"RWKVEncoder.step: x must be [B,K,input_dim] with K >= 1, got "
                             f"{tuple(x.shape)}")
        ops._lib.require_device(x)
        w = self.step_weights(_step_dtype(x)) if weights is None else weights
        B, K, _ = x.shape
        if state is None:
            state = self.zero_state(B, x.device)
        self._check_step_state(state, B)
        ws = self.step_workspace(B, K, w, x.device) if workspace is None else workspace
        if tuple(ws["x"].shape) != (K, B, x.shape[2]):
            raise ValueError(f"RWKVEncoder.step: workspace is for x {tuple(ws['x'].shape)} "
                             f"([K,B,Din]), got x {tuple(x.shape)}")
        with torch.autocast("cuda", enabled=False):
            ws["x"].copy_(x.transpose(0, 1))
            lv = None
            if live is not None:
                if tuple(live.shape) != (B, K):
                    raise ValueError(f"RWKVEncoder.step: live must be [B,K]=({B},{K})")
                ws["live"].copy_(live.t())
                lv = ws["live"]
            self._step_block(ws, state, lv, w)
        return ws["logits"].transpose(0, 1), state

    # ------------------------------------------------------------------------- forward --------
    def forward(self, x, state=None):
        if x.dim() != 3 or x.shape[1] < 1:
            raise ValueError(f"RWKVEncoder: x must be [B,T,input_dim] with T >= 1, got {tuple(x.shape)}")
        B = x.shape[0]
        if state is None:
            state = self.zero_state(B, x.device)
        if len(state) != 5 or any(s.shape[0] != len(self.blocks) or s.shape[1] != B for s in state):
            raise ValueError("RWKVEncoder: state must be (x_att, x_ffn, num, den, max), each [L,B,C]")
        x_att, x_ffn, num, den, mx = state
        h = self.input_proj(x)
        out = [[], [], [], [], []]
        for l, blk in enumerate(self.blocks):
            h, xa, xf, (n1, d1, m1) = blk(h, x_att[l], x_ffn[l], (num[l], den[l], mx[l]))
            for lst, val in zip(out, (xa, xf, n1, d1, m1)):
                lst.append(val)
        logits = self.output_proj(self.ln_out(h))
        if not self.config.return_last_states:
            return logits
        return logits, tuple(torch.stack(o) for o in out)
