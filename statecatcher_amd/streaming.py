"""Streaming (frame-synchronous) decode of a native LucyRNN with fused greedy CTC — SURVEY §8(f)
row 2.

The reference's streaming path is the infer-mode loop of lucyrnn.py:172-184: for every frame,
every layer runs ``LucyRNNCell.forward`` (lucyrnn.py:44-70) on the previous layer's h, then
``output_proj`` (:186), and decoding is decoder.py:3-30 (argmax, collapse repeats, drop blanks)
over the finished sequence.  Here a frame is:

    per layer:  a = input_proj(x)             library GEMM (hipBLASLt)
                u = LayerNorm_in(a)           sc_lucy_step_ln      (csrc/lucy_step.hip)
                g = gate projection(u)        library GEMM; fused: W_fused minus the dead r rows
                h, s <- cell(g, h, s)         sc_lucy_step_cell    (+ W_h GEMM + a second cell
                                                                    stage when fused_ops=False)
    logits = output_proj(h_L)                 library GEMM
    emit   = greedy step(logits, prev)        sc_ctc_greedy_step   (csrc/decode.hip)

with h, s resident on the GPU in fp32 between calls and every buffer static, so one block of
``frames_per_call`` frames is captured once as a hipGraph (torch.cuda.CUDAGraph) and replayed:
one host launch per block instead of ~(4-6 L + 2) kernel launches per frame.

schedule="wavefront" (the default with the frame engine) runs a block of K frames as K + L - 1
stages over (frame, layer), each stage one launch per kernel kind for all its layers
(_block_wavefront): 4 (K + L - 1) + 2 launches per block instead of K (4 L + 2), identical
arithmetic.

engine="frame" (the default where it applies: hidden_dim a multiple of 16) replaces the library
GEMMs and the LayerNorm / cell kernels by the fused chain of csrc/lucy_frame.hip: per layer
    a = x W_in^T + b_in (+ row statistics)            lucy_frame_gemm
    gates on LN_in(a), cell stage in the epilogue     lucy_frame_gemm  (s, z, y / hp, statistics)
    hp = y W_h^T + b_h (+ statistics)  [unfused]      lucy_frame_gemm
    h = (1 - z~) tanh(LN_h hp) + z~ h                 lucy_frame_cellb
then logits (lucy_frame_gemm) and the greedy step: 3-4 launches per layer instead of 5-6, no
LayerNorm launch (statistics ride with the producing GEMM), MFMA on fp32 (exact f32) or bf16
weights, fp32 activations.

The decode is incremental: ``prev`` holds each stream's last argmax (-1 at stream start, as
decoder.py's ``prev_token = None``), and emit[b, t] is the token decoder.py would append at
frame t, or -1.  Frames with mask 0 (past a stream's end) keep state (lucyrnn.py:66-68) and
emit nothing.

With ``joiner`` (an RNNTPredictorJoiner / RNNTCompactPredictorJoiner) the block ends in a greedy
transducer decode instead (the reference has none): enc_p = joiner.enc_proj(logits) over the
block's K frames (lucy_frame_gemm on the frame engine, addmm on the library engine), then ONE
sc_rnnt_greedy_decode launch (csrc/rnnt_decode.hip) with each stream's last emitted token carried
in ``prev`` (``blank`` at stream start, compute_loss's predictor prefix), inside the same graph.
With ``beam`` as well the block ends in the transducer beam search instead (csrc/rnnt_beam.hip):
one sc_rnnt_beam_frames launch on a persistent state plus one result launch, and step() returns
the current n-best of every stream since its reset.

StreamingLucyRNNtriton streams a LucyRNNtriton (lucyrnn_triton.py, the encoder the training step
runs) the same way.  Its cell normalises per element, so a layer of a frame is ONE launch
(lucy_tframe_layer: LayerNorm on load, 7-gate projection, cell in the epilogue), a frame L + 2
launches and a wavefront block (K + L - 1) + 2.  Both classes share the block / capture / tail /
API code (_StreamBase).

StreamingXLSTM and StreamingRWKV stream the other two encoders on their own step methods
(xLSTMLarge.step, RWKVEncoder.step) with the same capture, tails and API.
"""
import torch

from . import ops
from .lucyrnn import LucyRNN


def _ln_params(mod, on):
    return (mod.weight.detach().float().contiguous(), mod.bias.detach().float().contiguous()) \
        if on else None


class _StreamBase:
    """What the streaming decoders share: the block (frame by frame or as a wavefront), its
    capture as a hipGraph, the greedy CTC / transducer tail, and step / decode / reset / state.
    A subclass builds the static buffers (x, mask, h, s, logits, emit, prev, ...) and provides
    _frame(j) and _block_wavefront()."""

    joiner = False   # True on an instance built with a joiner: the block ends in the transducer decode
    beam = None      # the beam width on an instance built with a joiner and beam=

    def _init_joiner(self, joiner, max_symbols, dev, beam=None, top_k=8, nbest=1, max_frames=4096):
        """Snapshot the joiner: enc_proj for the block's projection, the [V, J] predictor table
        and the output projection for the decode (fp32 on the frame engine, whose activations
        are fp32; ``dtype`` on the library engine), and the static decode outputs."""
        from .decoder import rnnt_joiner_tables
        jm = getattr(joiner, "module", joiner)
        B, K, V = self.B, self.K, self.V
        if jm.enc_proj.in_features != V or jm.joiner.out_features != V:
            raise ValueError(f"joiner must project the model's {V} outputs and emit {V} tokens")
        if not 1 <= int(max_symbols) <= 64:
            raise ValueError("max_symbols must be in [1, 64]")
        self.max_symbols, self.J = int(max_symbols), jm.enc_proj.out_features
        frame = self.engine == "frame"
        if frame and (V % 8 != 0 or V > 2048):
            raise ValueError("engine='frame' with a joiner needs vocab_size % 8 == 0 and <= 2048 "
                             "(enc_proj runs on lucy_frame_gemm); use engine='library'")
        wdt = self.dtype
        self.w_enc = jm.enc_proj.weight.detach().to(wdt).contiguous()
        self.b_enc = jm.enc_proj.bias.detach().to(torch.float32 if frame else wdt).contiguous()
        self.pred_tab, self.w_join, self.b_join = rnnt_joiner_tables(
            jm, torch.float32 if frame else wdt)
        cap = K * self.max_symbols
        self.tokens = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
        self.tok_frames = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(B, dtype=torch.int32, device=dev)
        if beam is not None:
            # the beam search's persistent state (room for max_frames live frames per stream
            # between resets) and the static n-best buffers step() hands back
            self.beam, self.top_k, self.nbest = int(beam), int(top_k), int(nbest)
            if not 1 <= self.nbest <= self.beam:
                raise ValueError("nbest must be in [1, beam]")
            if not 1 <= self.top_k <= 32:
                raise ValueError("top_k must be in [1, 32]")
            self.beam_state = ops.rnnt_beam_state(B, self.beam, self.max_symbols, max_frames, dev)
            cap = int(max_frames) * self.max_symbols
            self.beam_tokens = torch.full((B, self.nbest, cap), -1, dtype=torch.int32, device=dev)
            self.beam_lens = torch.zeros(B, self.nbest, dtype=torch.int32, device=dev)
            self.beam_scores = torch.zeros(B, self.nbest, dtype=torch.float32, device=dev)

    def _rnnt_block(self):
        """enc_proj over the block's K frames of logits, then one greedy transducer launch."""
        K, B = self.K, self.B
        lg, ep = self.logits.view(K * B, self.V), self.enc_p.view(K * B, self.J)
        if self.engine == "frame":
            ops.lucy_frame_gemm(ops.FRAME_PLAIN, lg, self.w_enc, self.b_enc, ep)
        else:
            torch.addmm(self.b_enc, lg, self.w_enc.t(), out=ep)
        if self.beam is not None:
            ops.rnnt_beam_decode(self.enc_p.transpose(0, 1), self.pred_tab, self.w_join,
                                 self.b_join, mask=self.mask.t(), blank=self.blank,
                                 top_k=self.top_k, nbest=self.nbest, state=self.beam_state,
                                 out=(self.beam_tokens, self.beam_lens, self.beam_scores))
            return
        ops.rnnt_greedy_decode(self.enc_p.transpose(0, 1), self.pred_tab, self.w_join, self.b_join,
                               mask=self.mask.t(), blank=self.blank, max_symbols=self.max_symbols,
                               prev=self.prev, out=(self.tokens, self.counts, self.tok_frames))

    def _block(self):
        if self.schedule == "wavefront":
            return self._block_wavefront()
        for j in range(self.K):
            self._frame(j)
        if self.joiner:
            self._rnnt_block()

    def _capture(self):
        side = torch.cuda.Stream(self.x.device)
        side.wait_stream(torch.cuda.current_stream(self.x.device))
        with torch.cuda.stream(side):   # warm-up: library workspaces, kernel loading
            self._block()
        torch.cuda.current_stream(self.x.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._block()

    # ------------------------------------------------------------------------------- API ---
    def reset(self, hidden_states=None, streams=None):
        """Start streams afresh: state from ``hidden_states`` ((h list, s list) of [B,D], as the
        reference's forward takes) or zero, prev token = none (``blank`` with a joiner).
        ``streams``: index tensor/list of the streams to reset (default all)."""
        idx = slice(None) if streams is None else torch.as_tensor(streams, device=self.x.device)
        for l in range(self.L):
            for buf, src in ((self.h[l], None if hidden_states is None else hidden_states[0][l]),
                             (self.s[l], None if hidden_states is None else hidden_states[1][l])):
                if src is None:
                    buf[idx] = 0.0
                else:
                    buf[idx] = src.to(buf.device, torch.float32)[idx]
        self.prev[idx] = self.blank if self.joiner else -1
        if self.beam is not None:
            self.beam_state.reset(None if streams is None else torch.as_tensor(streams).tolist())

    def state(self):
        """(h list, s list) fp32 copies — the reference's (h, s) return (lucyrnn.py:188-189)."""
        return [t.clone() for t in self.h], [t.clone() for t in self.s]

    def _x_in(self):
        """The [K, B, Din] view of the static input buffer that step() fills."""
        return self.x

    def step(self, x, mask=None):
        """Advance every stream by K = frames_per_call model frames.  x [B, K, input_dim *
        stack_order] (already stacked); mask [B, K] (bool/float, None = all live).  Returns
        emit int32 [B, K] on the device: the token decoder.py appends at that frame, or -1.
        The logits of the block stay in ``self.logits`` ([K, B, V]).
        With a joiner: returns (tokens int32 [B, K * max_symbols], frames, counts int32 [B]) on
        the device instead: row b's first counts[b] tokens are this block's emissions, frames
        their frame index within the block; later entries are stale.
        With a joiner and beam: returns (tokens int32 [B, nbest, max_frames * max_symbols], lens
        int32 [B, nbest], scores fp32 [B, nbest]): the current n-best of every stream since its
        reset, best first (ops.rnnt_beam_result's layout; entries past lens are stale)."""
        self._x_in().copy_(x.transpose(0, 1))
        if mask is None:
            self.mask.fill_(1.0)
        else:
            self.mask.copy_(mask.transpose(0, 1))
        if self.graph is not None:
            self.graph.replay()
        else:
            self._block()
        if self.beam is not None:
            return self.beam_tokens, self.beam_lens, self.beam_scores
        if self.joiner:
            return self.tokens, self.tok_frames, self.counts
        return self.emit.t()

    def decode(self, feats, masks=None, return_logits=False):
        """Whole utterances through the streaming path: feats [B, T, input_dim] raw frames,
        stacked as the model does (lucyrnn.py:92-99: the tail T % stack_order is dropped, a
        stacked frame is live when all its frames are).  Returns the decoder.py token lists
        (and logits [B, T', V] if asked).  One host sync at the end.  With beam: the best
        hypothesis of every stream since its reset."""
        B, T, F = feats.shape
        k = getattr(self.cfg, "stack_order", 1)   # (the xLSTM config has none: 1)
        Tt = T - T % k
        x = feats[:, :Tt].reshape(B, Tt // k, F * k)
        m = None
        if masks is not None:
            m = masks.reshape(B, -1)[:, :Tt].reshape(B, Tt // k, k).all(-1).float()
        T2 = x.shape[1]
        emits, logits = [], []
        for t0 in range(0, T2, self.K):
            n = min(self.K, T2 - t0)
            xb = torch.zeros(B, self.K, x.shape[2], dtype=self.dtype, device=self.x.device)
            xb[:, :n] = x[:, t0:t0 + n]
            mb = torch.zeros(B, self.K, device=self.x.device)   # padding frames are masked out
            mb[:, :n] = 1.0 if m is None else m[:, t0:t0 + n]
            if self.beam is not None:
                self.step(xb, mb)
            elif self.joiner:
                tk, _, ct = self.step(xb, mb)
                emits.append(torch.cat([ct.unsqueeze(1), tk], 1))   # (a copy: count, tokens)
            else:
                emits.append(self.step(xb, mb)[:, :n].clone())
            if return_logits:
                logits.append(self.logits[:n].transpose(0, 1).clone())
        em = torch.cat(emits, 1).cpu() if emits else torch.zeros(B, 0, dtype=torch.int32)
        if self.beam is not None:
            ln = self.beam_lens[:, 0].clamp(min=0)
            best = self.beam_tokens[:, 0, :max(int(ln.max()), 1)].cpu()
            toks = [best[b, :n].tolist() for b, n in enumerate(ln.tolist())]
        elif self.joiner:
            w = 1 + self.K * self.max_symbols
            toks = [[t for k in range(0, em.shape[1], w) for t in row[k + 1:k + 1 + row[k]]]
                    for row in em.tolist()]
        else:
            toks = [[int(t) for t in row if t >= 0] for row in em]
        if return_logits:
            return toks, torch.cat(logits, 1) if logits else None
        return toks


class StreamingLucyRNN(_StreamBase):
    """Decode ``batch`` concurrent streams through ``model`` (a native LucyRNN; its weights are
    snapshotted at construction) ``frames_per_call`` model frames per call.

    dtype: activation/weight dtype of the GEMMs (fp32 = the reference's arithmetic; bf16 for
    throughput); state is fp32 either way.  graph: capture the block as a hipGraph.
    joiner: decode as a transducer with this joiner (at most ``max_symbols`` tokens per frame)
    instead of greedy CTC; its weights are snapshotted too.
    beam (with a joiner): transducer beam search of this width instead of the greedy decode, each
    hypothesis extended by its ``top_k`` likeliest tokens (max_symbols 1..8 then); step() returns
    the ``nbest`` best hypotheses since the stream's reset, which may span ``max_frames`` live
    frames.
    """

    def __init__(self, model: LucyRNN, batch: int, frames_per_call: int = 1,
                 dtype=torch.float32, blank: int = 0, graph: bool = True, engine: str = "auto",
                 schedule: str = "wavefront", joiner=None, max_symbols: int = 4, beam=None,
                 top_k: int = 8, nbest: int = 1, max_frames: int = 4096):
        cfg = model.config
        dev = next(model.parameters()).device
        ops._lib.require_device(next(model.parameters()))
        self.cfg, self.B, self.K, self.dtype, self.blank = cfg, batch, frames_per_call, dtype, blank
        self.L, self.D, self.V = cfg.num_layers, cfg.hidden_dim, cfg.vocab_size
        self.Din = cfg.input_dim * cfg.stack_order
        D, B, K = self.D, batch, frames_per_call
        if not ops._lib.load().sc_lucy_step_supported(ops.dtype_code(torch.empty(0, dtype=dtype)), D):
            raise ValueError(f"streaming step: hidden_dim {D} / dtype {dtype} unsupported")
        w = lambda t: t.detach().to(dtype).contiguous()   # noqa: E731
        ln = cfg.layer_norm
        self.layers = []
        for cell in model.layers:
            e = {"w_in": w(cell.input_proj.weight), "b_in": w(cell.input_proj.bias),
                 "ln_in": _ln_params(cell.layernorm_in, ln), "lnz": _ln_params(cell.layernorm_z, ln),
                 "lnh": _ln_params(cell.layernorm_h, ln)}
            if cfg.fused_ops:
                # rows [0, D) are r: sigmoid(LN_r(r)) is computed by the reference and never used
                e["w_g"], e["b_g"] = w(cell.W_fused.weight[D:]), w(cell.W_fused.bias[D:])
            else:
                mods = (cell.W_z, cell.W_k, cell.W_v, cell.W_decay)
                e["w_g"] = w(torch.cat([m.weight for m in mods]))
                e["b_g"] = w(torch.cat([m.bias for m in mods]))
                e["w_h"], e["b_h"] = w(cell.W_h.weight), w(cell.W_h.bias)
            self.layers.append(e)
        self.w_out, self.b_out = w(model.output_proj.weight), w(model.output_proj.bias)
        # sc_lucy_frame_gemm keeps a workgroup's A rows in LDS: K <= 2048 (D and Din)
        frame_ok = (D % 16 == 0 and self.Din % 8 == 0 and D <= 2048 and self.Din <= 2048
                    and dtype in (torch.float32, torch.bfloat16))
        if engine == "auto":
            engine = "frame" if frame_ok else "library"
        if engine == "frame" and not frame_ok:
            raise ValueError("engine='frame' needs hidden_dim % 16 == 0, input width % 8 == 0, "
                             "both <= 2048, and fp32 / bf16 weights")
        self.engine = engine
        if schedule not in ("wavefront", "frame"):
            raise ValueError("schedule must be 'wavefront' or 'frame'")
        # wavefront: the frame engine's block as stages over (frame, layer) (_block_wavefront)
        self.schedule = schedule if engine == "frame" else "frame"
        self.joiner = joiner is not None
        if beam is not None and not self.joiner:
            raise ValueError("beam= needs a joiner (the beam search is the transducer's)")
        if self.joiner:
            self._init_joiner(joiner, max_symbols, dev, beam, top_k, nbest, max_frames)
        z = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
        if engine == "frame":
            f32 = torch.float32
            fb = lambda t: t.detach().float().contiguous()   # noqa: E731
            for e, cell in zip(self.layers, model.layers):
                e["b_in"] = fb(cell.input_proj.bias)
                e["b_g"] = fb(cell.W_fused.bias[D:]) if cfg.fused_ops else fb(torch.cat(
                    [m.bias for m in (cell.W_z, cell.W_k, cell.W_v, cell.W_decay)]))
                if not cfg.fused_ops:
                    e["b_h"] = fb(cell.W_h.bias)
            self.b_out = fb(model.output_proj.bias)
            self.x = z(K, B, self.Din, dt=f32)
            self.mask = torch.ones(K, B, dtype=f32, device=dev)
            self.fa, self.fz, self.fy, self.fhp = (z(B, D, dt=f32) for _ in range(4))
            self.st_a = z((D + 31) // 32, B, 4, dt=f32)   # (one record per 32 columns)
            self.st_z = z(D // 16, B, 4, dt=f32)
            self.st_h = z(D // 16, B, 4, dt=f32)
            self.xo = [z(B, D, dt=f32) for _ in range(self.L)]
            self.h = [z(B, D, dt=f32) for _ in range(self.L)]
            self.s = [z(B, D, dt=f32) for _ in range(self.L)]
            if self.schedule == "wavefront":
                # the layers of a stage run at once: each its own scratch; the last layer's
                # output per frame, for one output projection over the block
                self.wf = [dict(fa=z(B, D, dt=f32), fz=z(B, D, dt=f32), fy=z(B, D, dt=f32),
                                fhp=z(B, D, dt=f32), st_a=z((D + 31) // 32, B, 4, dt=f32),
                                st_z=z(D // 16, B, 4, dt=f32), st_h=z(D // 16, B, 4, dt=f32))
                           for _ in range(self.L)]
                self.xlast = z(K, B, D, dt=f32)
            self.logits = z(K, B, self.V, dt=f32)
            self.emit = torch.full((K, B), -1, dtype=torch.int32, device=dev)
            self.prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
            if self.joiner:
                self.enc_p = z(K, B, self.J, dt=f32)
            self.graph = None
            if graph:
                self._capture()
            self.reset()
            return
        ng = 5 if cfg.fused_ops else 4
        self.x = z(K, B, self.Din)
        self.mask = torch.ones(K, B, dtype=torch.float32, device=dev)
        self.a, self.u, self.g = z(B, D), z(B, D), z(B, ng * D)
        self.y, self.hp = z(B, D), z(B, D)
        self.xo = [z(B, D) for _ in range(self.L)]
        self.h = [z(B, D, dt=torch.float32) for _ in range(self.L)]
        self.s = [z(B, D, dt=torch.float32) for _ in range(self.L)]
        self.logits = z(K, B, self.V)
        self.emit = torch.full((K, B), -1, dtype=torch.int32, device=dev)
        self.prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if self.joiner:
            self.enc_p = z(K, B, self.J)
        self.graph = None
        if graph:
            self._capture()
        self.reset()

    # ------------------------------------------------------------------------------ frame --
    def _frame_fused_chain(self, j):
        """One frame on csrc/lucy_frame.hip's fused kernels (engine="frame")."""
        cfg, m, D = self.cfg, self.mask[j], self.D
        inp = self.x[j]
        for l, e in enumerate(self.layers):
            ln = e["ln_in"] is not None
            nst_a = (D + 31) // 32
            ops.lucy_frame_gemm(ops.FRAME_STATS if ln else ops.FRAME_PLAIN, inp, e["w_in"], e["b_in"],
                                self.fa, st_out=self.st_a[:nst_a] if ln else None)
            lnin = dict(ln=e["ln_in"], st_in=self.st_a[:nst_a]) if ln else {}
            if cfg.fused_ops:
                ops.lucy_frame_gemm(ops.FRAME_CELL_FUSED, self.fa, e["w_g"], e["b_g"], self.fhp,
                                    st_out=self.st_h, z=self.fz, st_z=self.st_z, s=self.s[l],
                                    mask=m, **lnin)
                st_h = self.st_h
            else:
                ops.lucy_frame_gemm(ops.FRAME_CELL_UNFUSED, self.fa, e["w_g"], e["b_g"], self.fy,
                                    z=self.fz, st_z=self.st_z, s=self.s[l], mask=m, **lnin)
                lnh = e["lnh"] is not None
                st_h = self.st_h[:nst_a]
                ops.lucy_frame_gemm(ops.FRAME_STATS if lnh else ops.FRAME_PLAIN, self.fy, e["w_h"],
                                    e["b_h"], self.fhp, st_out=st_h if lnh else None)
            ops.lucy_frame_cellb(self.fz, self.fhp, self.h[l], self.xo[l], st_z=self.st_z,
                                 st_h=st_h, lnz=e["lnz"], lnh=e["lnh"], mask=m)
            inp = self.xo[l]
        ops.lucy_frame_gemm(ops.FRAME_PLAIN, inp, self.w_out, self.b_out, self.logits[j])
        if not self.joiner:
            ops.ctc_greedy_step(self.logits[j], self.prev, self.emit[j], mask=m, blank=self.blank)

    def _frame(self, j):
        if self.engine == "frame":
            return self._frame_fused_chain(j)
        cfg, m = self.cfg, self.mask[j]
        inp = self.x[j]
        for l, e in enumerate(self.layers):
            torch.addmm(e["b_in"], inp, e["w_in"].t(), out=self.a)
            u = self.a
            if e["ln_in"] is not None:
                ops.lucy_step_ln(self.a, *e["ln_in"], self.u)
                u = self.u
            torch.addmm(e["b_g"], u, e["w_g"].t(), out=self.g)
            if cfg.fused_ops:
                ops.lucy_step_cell(ops.STEP_FUSED, self.g, self.h[l], self.s[l], self.xo[l],
                                   e["lnz"], e["lnh"], mask=m)
            else:
                ops.lucy_step_cell(ops.STEP_UNFUSED_A, self.g, self.h[l], self.s[l], self.y,
                                   e["lnz"], e["lnh"], u=u, mask=m)
                torch.addmm(e["b_h"], self.y, e["w_h"].t(), out=self.hp)
                ops.lucy_step_cell(ops.STEP_UNFUSED_B, self.g, self.h[l], self.s[l], self.xo[l],
                                   e["lnz"], e["lnh"], hp=self.hp, mask=m)
            inp = self.xo[l]
        torch.addmm(self.b_out, inp, self.w_out.t(), out=self.logits[j])
        if not self.joiner:
            ops.ctc_greedy_step(self.logits[j], self.prev, self.emit[j], mask=m, blank=self.blank)

    def _block_wavefront(self):
        """The frame engine's block as K + L - 1 stages: stage tau runs layer l of frame tau - l
        for every l at once (layer l of frame j needs layer l - 1 of frame j, from stage tau - 1,
        and layer l of frame j - 1, from stage tau - 1: its state).  A stage is the four kernels
        of a layer, each ONE launch over the stage's layers (sc_lucy_frame_gemm_multi /
        _cellb_multi); then one output projection over the K frames and one greedy launch.
        4 (K + L - 1) + 2 launches per block instead of K (4 L + 2), the same arithmetic per
        (frame, layer) as _frame_fused_chain.  Layer l's input xo[l - 1] is read by the stage's
        first launch and rewritten (next frame) by its last, so one buffer per layer suffices."""
        cfg, D, K, L = self.cfg, self.D, self.K, self.L
        stream = ops._lib.stream_of(self.x)
        wdt = self.w_out.dtype
        nst_a = (D + 31) // 32
        for tau in range(K + L - 1):
            act = [(l, tau - l) for l in range(L) if 0 <= tau - l < K]
            ln = self.layers[0]["ln_in"] is not None
            inproj, gates, whs, cells = [], [], [], []
            for l, j in act:
                e, sc, m = self.layers[l], self.wf[l], self.mask[j]
                inp = self.x[j] if l == 0 else self.xo[l - 1]
                inproj.append(ops.frame_gemm_job(inp, e["w_in"], e["b_in"], sc["fa"],
                                                 st_out=sc["st_a"][:nst_a] if ln else None))
                lnin = dict(ln=e["ln_in"], st_in=sc["st_a"][:nst_a]) if ln else {}
                if cfg.fused_ops:
                    gates.append(ops.frame_gemm_job(sc["fa"], e["w_g"], e["b_g"], sc["fhp"],
                                                    st_out=sc["st_h"], z=sc["fz"], st_z=sc["st_z"],
                                                    s=self.s[l], mask=m, **lnin))
                    st_h = sc["st_h"]
                else:
                    gates.append(ops.frame_gemm_job(sc["fa"], e["w_g"], e["b_g"], sc["fy"],
                                                    z=sc["fz"], st_z=sc["st_z"], s=self.s[l],
                                                    mask=m, **lnin))
                    lnh = e["lnh"] is not None
                    st_h = sc["st_h"][:nst_a]
                    whs.append(ops.frame_gemm_job(sc["fy"], e["w_h"], e["b_h"], sc["fhp"],
                                                  st_out=st_h if lnh else None))
                out = self.xlast[j] if l == L - 1 else self.xo[l]
                cells.append(ops.frame_cell_job(sc["fz"], sc["fhp"], self.h[l], out,
                                                st_z=sc["st_z"], st_h=st_h, lnz=e["lnz"],
                                                lnh=e["lnh"], mask=m))
            ops.lucy_frame_gemm_multi(ops.FRAME_STATS if ln else ops.FRAME_PLAIN, wdt, inproj, stream)
            ops.lucy_frame_gemm_multi(ops.FRAME_CELL_FUSED if cfg.fused_ops else ops.FRAME_CELL_UNFUSED,
                                      wdt, gates, stream)
            if whs:
                lnh = self.layers[0]["lnh"] is not None
                ops.lucy_frame_gemm_multi(ops.FRAME_STATS if lnh else ops.FRAME_PLAIN, wdt, whs,
                                          stream)
            ops.lucy_frame_cellb_multi(cells, stream)
        ops.lucy_frame_gemm(ops.FRAME_PLAIN, self.xlast.view(K * self.B, D), self.w_out, self.b_out,
                            self.logits.view(K * self.B, self.V))
        if self.joiner:
            return self._rnnt_block()
        ops.ctc_greedy_frames(self.logits, self.prev, self.emit, mask=self.mask, blank=self.blank)


class StreamingLucyRNNtriton(_StreamBase):
    """Decode ``batch`` concurrent streams through a LucyRNNtriton (the model the training step
    runs; weights snapshotted at construction) ``frames_per_call`` frames per call.

    A layer of a frame is ONE launch (ops.lucy_tframe_layer, csrc/lucy_frame.hip): the inter-layer
    LayerNorm applied on load from the previous layer's records, the 7-gate projection on MFMA
    (fp32 or bf16 weights per ``dtype``; activations and state fp32), the cell in the epilogue,
    h / s updated in place.  schedule="frame": L launches, the output projection and the greedy
    step per frame.  schedule="wavefront" (default): stage tau runs layer l of frame tau - l for
    every l as one multi-job launch, then one output projection over the block and one greedy /
    transducer launch: (K + L - 1) + 2 launches per block.

    The jobs of a stage run concurrently, and layer l - 1 (frame j + 1) writes what layer l
    (frame j) reads, so each layer's output and records are double-buffered by the frame's parity
    within the block: xo[l][j & 1] is written in stage l + j, read in stage l + j + 1, and next
    written (frame j + 2) in stage l + j + 2.  The same buffers serve every block, so the block
    is captured once.

    reset() takes and state() returns LucyRNNtriton's own nesting ([[h] * L], [[s] * L])
    ([track][layer] of fp32 [B, D]): ``model(x, st.state())`` and ``st.reset(model(x)[1])`` hand
    over between an offline segment and the stream.  Multi-track models, hidden_dim not a
    multiple of 16 or above 2048 are refused: use the offline forward with carried state there.
    """

    engine = "frame"   # (the transducer tail's enc_proj runs on lucy_frame_gemm)

    def __init__(self, model, batch: int, frames_per_call: int = 1, dtype=torch.float32,
                 blank: int = 0, graph: bool = True, schedule: str = "wavefront", joiner=None,
                 max_symbols: int = 4, beam=None, top_k: int = 8, nbest: int = 1,
                 max_frames: int = 4096):
        from .lucyrnn_triton import LucyRNNtriton
        alt = ("; use LucyRNNtriton.forward(x, hidden_states) on chunks with carried state "
               "instead")
        if not isinstance(model, LucyRNNtriton):
            raise TypeError("StreamingLucyRNNtriton streams a LucyRNNtriton (StreamingLucyRNN "
                            f"takes the native LucyRNN), got {type(model).__name__}")
        cfg = model.config
        if model.num_tracks > 1:
            raise ValueError(f"streaming: num_tracks = {model.num_tracks} > 1 is not supported" + alt)
        if cfg.hidden_dim % 16 != 0:
            raise ValueError(f"streaming: hidden_dim {cfg.hidden_dim} is not a multiple of 16" + alt)
        if cfg.hidden_dim > 2048 or cfg.input_dim > 2048:
            raise ValueError(f"streaming: hidden_dim {cfg.hidden_dim} / input_dim {cfg.input_dim} "
                             "above 2048 (a workgroup keeps its input rows in LDS)" + alt)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("streaming: weights fp32 or bf16")
        if schedule not in ("wavefront", "frame"):
            raise ValueError("schedule must be 'wavefront' or 'frame'")
        dev = next(model.parameters()).device
        ops._lib.require_device(next(model.parameters()))
        self.cfg, self.B, self.K, self.dtype, self.blank = cfg, batch, frames_per_call, dtype, blank
        self.L, self.D, self.V, self.Din = cfg.num_layers, cfg.hidden_dim, cfg.vocab_size, cfg.input_dim
        self.schedule = schedule
        L, D, B, K = self.L, self.D, batch, frames_per_call
        f32 = torch.float32
        fb = lambda t: t.detach().float().contiguous()   # noqa: E731
        # layer 0's weight columns and the x buffer zero-padded to 8: exact, the zeros add nothing
        self.Dp = (self.Din + 7) // 8 * 8
        norms = model.norms[0]
        self.eps = float(norms[0].eps) if len(norms) else 1e-5
        if any(float(n.eps) != self.eps for n in norms):
            raise ValueError("streaming: the inter-layer LayerNorms must share one eps" + alt)
        self.layers = []
        for l, cell in enumerate(model.tracks[0]):
            wl = cell.linear.weight.detach()
            if l == 0 and self.Dp != self.Din:
                wl = torch.nn.functional.pad(wl, (0, self.Dp - self.Din))
            bl = cell.linear.bias
            self.layers.append({
                "w": wl.to(dtype).contiguous(),
                "b": fb(bl) if bl is not None else torch.zeros(7 * D, dtype=f32, device=dev),
                "ln": (fb(norms[l - 1].weight), fb(norms[l - 1].bias)) if l > 0 else None})
        self.w_out = model.output_proj.weight.detach().to(dtype).contiguous()
        ob = model.output_proj.bias
        self.b_out = fb(ob) if ob is not None else torch.zeros(self.V, dtype=f32, device=dev)
        self.joiner = joiner is not None
        if beam is not None and not self.joiner:
            raise ValueError("beam= needs a joiner (the beam search is the transducer's)")
        if self.joiner:
            self._init_joiner(joiner, max_symbols, dev, beam, top_k, nbest, max_frames)
        z = lambda *s: torch.zeros(*s, dtype=f32, device=dev)   # noqa: E731
        self.x = z(K, B, self.Dp)
        self.mask = torch.ones(K, B, dtype=f32, device=dev)
        self.h = [z(B, D) for _ in range(L)]
        self.s = [z(B, D) for _ in range(L)]
        # layer l < L - 1: output and records per frame parity; the last layer's output per frame
        self.xo = [(z(B, D), z(B, D)) for _ in range(L - 1)]
        self.rec = [(z(D // 16, B, 4), z(D // 16, B, 4)) for _ in range(L - 1)]
        self.xlast = z(K, B, D)
        self.logits = z(K, B, self.V)
        self.emit = torch.full((K, B), -1, dtype=torch.int32, device=dev)
        self.prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if self.joiner:
            self.enc_p = z(K, B, self.J)
        self.graph = None
        if graph:
            self._capture()
        self.reset()

    def _layer_args(self, l, j):
        """The arguments of layer l at frame j of the block (ops.lucy_tframe_layer / tframe_job)."""
        e, p, last = self.layers[l], j & 1, l == self.L - 1
        kw = dict(mask=self.mask[j], st_out=None if last else self.rec[l][p])
        if l > 0:
            kw.update(ln=e["ln"], st_in=self.rec[l - 1][p])
        return (self.x[j] if l == 0 else self.xo[l - 1][p], e["w"], e["b"], self.h[l], self.s[l],
                self.xlast[j] if last else self.xo[l][p]), kw

    def _frame(self, j):
        for l in range(self.L):
            args, kw = self._layer_args(l, j)
            ops.lucy_tframe_layer(*args, eps=self.eps, **kw)
        ops.lucy_frame_gemm(ops.FRAME_PLAIN, self.xlast[j], self.w_out, self.b_out, self.logits[j])
        if not self.joiner:
            ops.ctc_greedy_step(self.logits[j], self.prev, self.emit[j], mask=self.mask[j],
                                blank=self.blank)

    def _block_wavefront(self):
        K, L, D = self.K, self.L, self.D
        stream = ops._lib.stream_of(self.x)
        for tau in range(K + L - 1):
            jobs = []
            for l in range(L):
                if 0 <= tau - l < K:
                    args, kw = self._layer_args(l, tau - l)
                    jobs.append(ops.tframe_job(*args, **kw))
            ops.lucy_tframe_layer_multi(self.w_out.dtype, jobs, stream, eps=self.eps)
        ops.lucy_frame_gemm(ops.FRAME_PLAIN, self.xlast.view(K * self.B, D), self.w_out, self.b_out,
                            self.logits.view(K * self.B, self.V))
        if self.joiner:
            return self._rnnt_block()
        ops.ctc_greedy_frames(self.logits, self.prev, self.emit, mask=self.mask, blank=self.blank)

    def _x_in(self):
        return self.x[..., :self.Din]

    def reset(self, hidden_states=None, streams=None):
        """As StreamingLucyRNN.reset, with ``hidden_states`` in LucyRNNtriton's nesting
        ([[h] * L], [[s] * L]) (what its forward returns and takes)."""
        if hidden_states is not None:
            hidden_states = (hidden_states[0][0], hidden_states[1][0])
        super().reset(hidden_states, streams)

    def state(self):
        """([[h] * L], [[s] * L]) fp32 copies: LucyRNNtriton.forward's ``hidden_states``."""
        h, s = super().state()
        return [h], [s]


class StreamingXLSTM(_StreamBase):
    """Decode ``batch`` concurrent streams through an xLSTMLarge (xlstm.py; weights snapshotted at
    construction) ``frames_per_call`` frames per call.

    A block is xLSTMLarge.step on static buffers: per xLSTM block the fused projection GEMM, ONE
    recurrent mLSTM launch for the block's K frames (csrc/mlstm_step.hip: the matrix state C is
    read once, held in registers over the K steps and written once, in place), the gated head
    norm, out_proj, the residual / RMSNorm glue and the FFN; then out_norm, lm_head, the logit
    soft cap, and the greedy CTC / transducer tail of the LucyRNN streamers.  It is a linear
    chain of launches, captured once as a hipGraph.

    dtype: the weight and GEMM dtype; activations between kernels are what the offline model has
    under the same dtype (bf16 under bf16 autocast, fp32 without).  State: {block: (C [B,NH,DQ,DV],
    n [B,NH,DQ], m [B,NH,1])} fp32, the dict xLSTMLarge.forward returns and takes: reset(states)
    and state() hand over between an offline segment and the stream.  Frames with mask 0 hold
    every block's state and emit nothing -- where the offline model, padded to a 64-frame chunk
    with zero frames, advances its state through the padding.
    input_proj: an nn.Linear applied before the encoder's embedding (an ASRModel's ``proj``).
    gemm: "frame" runs the linears on lucy_frame_gemm (csrc/lucy_frame.hip), whose arithmetic per
    row does not depend on the block size: a block of K frames equals K calls of one frame
    bitwise.  "library" runs the library GEMM autocast would run (it picks its kernel by the row
    count, so block sizes agree to rounding only).  "auto": "frame" where its limits hold (every
    reduction length a multiple of 8 and <= 2048), else "library".
    """

    engine = "frame"     # (the transducer tail's enc_proj runs on lucy_frame_gemm)
    schedule = "frame"

    def __init__(self, model, batch: int, frames_per_call: int = 1, dtype=torch.bfloat16,
                 graph: bool = True, blank: int = 0, joiner=None, max_symbols: int = 4, beam=None,
                 top_k: int = 8, nbest: int = 1, max_frames: int = 4096, input_proj=None,
                 gemm: str = "auto"):
        import copy

        from .xlstm import xLSTMLarge
        if not isinstance(model, xLSTMLarge):
            raise TypeError(f"StreamingXLSTM streams an xLSTMLarge, got {type(model).__name__}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("streaming: weights fp32 or bf16")
        cfg = model.config
        dev = next(model.parameters()).device
        ops._lib.require_device(next(model.parameters()))
        NH = cfg.num_heads
        lay = model.blocks[0].mlstm_layer
        if not ops.mlstm_step_supported(dtype, lay.qk_dim // NH, lay.v_dim // NH):
            raise ValueError(f"streaming: mLSTM step head dims (DQ={lay.qk_dim // NH}, "
                             f"DV={lay.v_dim // NH}) not compiled in")
        self.cfg, self.B, self.K, self.dtype, self.blank = cfg, batch, frames_per_call, dtype, blank
        self.L, self.V = cfg.num_blocks, cfg.vocab_size
        self.stack_order = 1
        B, K = batch, frames_per_call
        # the snapshot: a private copy of the module (its norms' fp32 parameters) and every
        # linear weight cast to dtype once
        self.model = copy.deepcopy(model).eval().requires_grad_(False)
        # gemm="frame": the linears on lucy_frame_gemm, whose arithmetic per row does not depend
        # on the block size (K frames per call == K calls of one frame bitwise); "library": the
        # library GEMM, which picks its kernel by the row count (equal to rounding only)
        if gemm == "auto":
            gemm = "frame" if self.model.step_gemm_frame_ok(input_proj) else "library"
        self.gemm = gemm
        self.weights = self.model.step_weights(dtype, input_proj, gemm)
        self.Din = (input_proj.in_features if input_proj is not None
                    else self.model.embedding.in_features)
        self.joiner = joiner is not None
        if beam is not None and not self.joiner:
            raise ValueError("beam= needs a joiner (the beam search is the transducer's)")
        if self.joiner:
            self._init_joiner(joiner, max_symbols, dev, beam, top_k, nbest, max_frames)
        f32 = torch.float32
        self.x = torch.zeros(K, B, self.Din, dtype=f32, device=dev)
        self.mask = torch.ones(K, B, dtype=f32, device=dev)
        self.states = self.model.zero_state(B, dev)
        self.logits = torch.zeros(K, B, self.V, dtype=f32, device=dev)
        self.emit = torch.full((K, B), -1, dtype=torch.int32, device=dev)
        self.prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if self.joiner:
            self.enc_p = torch.zeros(K, B, self.J, dtype=f32, device=dev)
        self.graph = None
        if graph:
            self._capture()
        self.reset()

    def _block(self):
        logits, _ = self.model.step(self.x.transpose(0, 1), self.states, self.mask.t(),
                                    self.weights)
        self.logits.copy_(logits.transpose(0, 1))
        if self.joiner:
            return self._rnnt_block()
        ops.ctc_greedy_frames(self.logits, self.prev, self.emit, mask=self.mask, blank=self.blank)

    # ------------------------------------------------------------------------------- API ---
    def reset(self, states=None, streams=None):
        """Start streams afresh: state from ``states`` ({block: (C, n, m)}, what
        xLSTMLarge.forward returns; a missing block or entry is zero) or zero, prev token = none
        (``blank`` with a joiner).  ``streams``: the streams to reset (default all)."""
        idx = slice(None) if streams is None else torch.as_tensor(streams, device=self.x.device)
        for i, bufs in self.states.items():
            src = None if states is None else states.get(i)
            for j, buf in enumerate(bufs):
                if src is None or src[j] is None:
                    buf[idx] = 0.0
                else:
                    buf[idx] = src[j].detach().to(buf.device, torch.float32).reshape(buf.shape)[idx]
        self.prev[idx] = self.blank if self.joiner else -1
        if self.beam is not None:
            self.beam_state.reset(None if streams is None else torch.as_tensor(streams).tolist())

    def state(self):
        """{block: (C, n, m)} fp32 copies: xLSTMLarge.forward's ``state``."""
        return {i: tuple(t.clone() for t in st) for i, st in self.states.items()}


class StreamingRWKV(_StreamBase):
    """Decode ``batch`` concurrent streams through an RWKVEncoder (rwkv.py; weights snapshotted
    at construction) ``frames_per_call`` frames per call.

    A block is RWKVEncoder.step on static buffers (its step_workspace): per RWKV block the
    shift-mix kernel (residual, LayerNorm, time shift and the mixes of the block's K frames in one
    launch), the k / v / r GEMMs as one multi-job launch, ONE recurrent WKV launch (csrc/
    rwkv_step.hip: (num, den, max) read once, held in registers over the K steps, written once,
    in place; the receptance gate in its epilogue), the output GEMM, the second shift-mix, the
    feed-forward's two GEMM launches and its squared ReLU: 8 launches per block of the stack for
    the K frames; then the final LayerNorm, the output projection and the greedy CTC / transducer
    tail of the other streamers.  A linear chain on one stream, captured once as a hipGraph.

    dtype: the weight dtype of the GEMMs.  State: RWKVEncoder.forward's (x_att, x_ffn, num, den,
    max), each fp32 [L,B,C]: reset(state) and state() hand over between an offline segment and
    the stream in both directions.  Frames with mask 0 hold every block's state (both shift
    frames and the WKV triple, bitwise) and emit nothing -- where the offline forward on zero
    padding pushes the padding into the WKV state and overwrites the shift frames.
    input_proj: an nn.Linear applied before the encoder's own input projection (an ASRModel's
    ``proj``).
    gemm: "frame" runs the linears on lucy_frame_gemm (csrc/lucy_frame.hip: fp32 activations,
    arithmetic per row independent of the block size, so a block of K frames equals K calls of
    one frame bitwise).  "library" runs the library GEMM in ``dtype`` with activations in
    ``dtype`` (it picks its kernel by the row count, so block sizes agree to rounding only).
    "auto": "frame" where its limits hold (every reduction length -- input_dim, H, A, I and
    input_proj's width -- a multiple of 8 and <= 2048), else "library".
    """

    engine = "frame"     # (the transducer tail's enc_proj runs on lucy_frame_gemm)
    schedule = "frame"

    def __init__(self, model, batch: int, frames_per_call: int = 1, dtype=torch.bfloat16,
                 graph: bool = True, blank: int = 0, joiner=None, max_symbols: int = 4, beam=None,
                 top_k: int = 8, nbest: int = 1, max_frames: int = 4096, input_proj=None,
                 gemm: str = "auto"):
        import copy

        from .rwkv import RWKVEncoder
        if not isinstance(model, RWKVEncoder):
            raise TypeError(f"StreamingRWKV streams an RWKVEncoder, got {type(model).__name__}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("streaming: weights fp32 or bf16")
        cfg = model.config
        dev = next(model.parameters()).device
        ops._lib.require_device(next(model.parameters()))
        self.cfg, self.B, self.K, self.dtype, self.blank = cfg, batch, frames_per_call, dtype, blank
        self.L, self.V = cfg.num_layers, cfg.vocab_size
        B, K = batch, frames_per_call
        # the snapshot: a private copy of the module and every weight cast once
        self.model = copy.deepcopy(model).eval().requires_grad_(False)
        self.weights = self.model.step_weights(dtype, input_proj, gemm)
        self.gemm = self.weights["gemm"]
        self.joiner = joiner is not None
        if beam is not None and not self.joiner:
            raise ValueError("beam= needs a joiner (the beam search is the transducer's)")
        if self.joiner:
            self._init_joiner(joiner, max_symbols, dev, beam, top_k, nbest, max_frames)
        self.ws = self.model.step_workspace(B, K, self.weights, dev)
        self.x, self.mask, self.logits = self.ws["x"], self.ws["live"], self.ws["logits"]
        self.Din = self.x.shape[2]
        self.states = self.model.zero_state(B, dev)
        self.emit = torch.full((K, B), -1, dtype=torch.int32, device=dev)
        self.prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if self.joiner:
            self.enc_p = torch.zeros(K, B, self.J, dtype=torch.float32, device=dev)
        self.graph = None
        if graph:
            self._capture()
        self.reset()

    def _block(self):
        self.model._step_block(self.ws, self.states, self.mask, self.weights)
        if self.joiner:
            return self._rnnt_block()
        ops.ctc_greedy_frames(self.logits, self.prev, self.emit, mask=self.mask, blank=self.blank)

    # ------------------------------------------------------------------------------- API ---
    def reset(self, state=None, streams=None):
        """Start streams afresh: state from ``state`` ((x_att, x_ffn, num, den, max), each
        [L,B,C]: what RWKVEncoder.forward returns and takes) or the state before the first frame
        (zero shift frames, the empty WKV state), prev token = none (``blank`` with a joiner).
        ``streams``: the streams to reset (default all)."""
        idx = slice(None) if streams is None else torch.as_tensor(streams, device=self.x.device)
        if state is not None and len(state) != 5:
            raise ValueError("StreamingRWKV.reset: state must be (x_att, x_ffn, num, den, max)")
        zero = self.model.zero_state(self.B, self.x.device) if state is None else None
        for i, buf in enumerate(self.states):
            src = zero[i] if state is None else \
                state[i].detach().to(buf.device, torch.float32).reshape(buf.shape)
            buf[:, idx] = src[:, idx]
        self.prev[idx] = self.blank if self.joiner else -1
        if self.beam is not None:
            self.beam_state.reset(None if streams is None else torch.as_tensor(streams).tolist())

    def state(self):
        """(x_att, x_ffn, num, den, max) fp32 copies: RWKVEncoder.forward's ``state``."""
        return tuple(t.clone() for t in self.states)
