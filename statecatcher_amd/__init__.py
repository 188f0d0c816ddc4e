"""statecatcher_amd — MI355X-native hot path of the statecatcher stateful recurrent ASR step.

LucyRNN gated scan (fwd + bwd), decay scan, CTC alpha-beta (+ fused log_softmax) and greedy
CTC decode as hand-written HIP kernels for gfx950 behind a C ABI (include/statecatcher.h),
wrapped in drop-ins of the reference's module API (lucyrnn_triton.py, decoder.py, model.py).
"""
from .lucyrnn_conf import LucyRNNConfig
from .lucyrnn_triton import LinearSafe, LucyRNNCellTriton, LucyRNNtriton
from .lucyrnn import LucyRNN, LucyRNNCell
from .xlstm import xLSTMLarge, xLSTMLargeConfig
from .rwkv import RWKVConfig, RWKVEncoder
from .model import (ASRModel, CTCLoss, RNNTCompactPredictorJoiner, RNNTLoss, RNNTPredictorJoiner,
                    build_lucyrnn_config, build_rwkv_config, build_xlstm_config, compute_loss,
                    detach_states)
from .ops import (ctc_align, ctc_beam_decode, ctc_beam_result, ctc_beam_state, ctc_greedy_decode,
                  ctc_loss, ctc_nll, decay_scan, lucy_scan, mlstm_chunkwise, rnnt_beam_decode,
                  rnnt_beam_result, rnnt_beam_state, rnnt_greedy_decode, rnnt_loss, wkv)
from .decoder import (ctc_beam_decoder, ctc_forced_align, ctc_greedy_decoder, rnnt_beam_decoder,
                      rnnt_greedy_decoder)
from .streaming import (StreamingLucyRNN, StreamingLucyRNNtriton, StreamingRWKV,
                        StreamingXLSTM)
from .frontend import make_frontend

__all__ = [
    "LucyRNNConfig", "LinearSafe", "LucyRNNCellTriton", "LucyRNNtriton", "LucyRNN", "LucyRNNCell", "ASRModel", "CTCLoss",
    "compute_loss", "detach_states", "build_lucyrnn_config", "build_xlstm_config", "ctc_greedy_decode", "ctc_loss", "ctc_nll", "decay_scan",
    "lucy_scan", "ctc_greedy_decoder", "rnnt_loss", "RNNTLoss", "RNNTPredictorJoiner",
    "RNNTCompactPredictorJoiner", "xLSTMLarge", "xLSTMLargeConfig", "mlstm_chunkwise",
    "StreamingLucyRNN", "StreamingLucyRNNtriton", "StreamingXLSTM", "StreamingRWKV", "make_frontend", "rnnt_greedy_decode", "rnnt_greedy_decoder",
    "ctc_beam_decode", "ctc_beam_state", "ctc_beam_result", "ctc_beam_decoder",
    "rnnt_beam_decode", "rnnt_beam_state", "rnnt_beam_result", "rnnt_beam_decoder",
    "ctc_align", "ctc_forced_align", "RWKVConfig", "RWKVEncoder", "build_rwkv_config", "wkv",
]
