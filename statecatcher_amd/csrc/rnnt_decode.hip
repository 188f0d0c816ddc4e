// Greedy RNN-T (transducer) decoding on device for the stateless predictor of
// RNNTPredictorJoiner (model.py:112-145): pred_proj(embedding(prev_token)) depends only on the last
// emitted token, so the predictor is a [V, J] table and the decoder's whole state is one int32 per
// stream.  The reference has no transducer decoder (its decoder.py is CTC greedy); in PyTorch this
// is a loop of T + U joint evaluations with a host sync each (the decoder.py:24 pattern).
//
// Per stream b, u = prev[b] (blank at stream start), for every live frame t in order, at most
// max_symbols times:
//     z = tanh(enc_p[b,t] + pred_tab[u]);  logit = W z + bias;  k = argmax logit (decode.hip's
//     `beats`: first maximal index, NaN maximal);  k == blank -> next frame;  else emit (k, t), u = k
// Everything is widened to fp32 on load and stays fp32 (z is NOT rounded to bf16 as the fused
// training joint of rnnt.hip does): decoding follows the reference's fp32 arithmetic.
//
// One persistent workgroup of 1024 threads per stream; every branch is workgroup-uniform and every
// loop is bounded by T, max_symbols, V or J.  One evaluation:
//     wave 0: z -> LDS | barrier | every lane: its row(s) . z (z by broadcast 16-byte LDS reads),
//     wave (value, index) reduction on DPP (beam_common.h's wave_argmax in dec_beats' order) ->
//     LDS | barrier | every wave reduces the 16 candidates
//   rnnt_decode_kernel<DT, true>   J = 64, V <= 1024: lane v holds row v of W in 64 VGPRs + its bias
//                                  for the whole stream (under the 128 VGPRs of 4 waves per SIMD)
//   rnnt_decode_kernel<DT, false>  any V, J <= 256: rows v = tid, tid + 1024, ... read from memory
//                                  at every evaluation (correct, not tuned)
// enc_p[b,t+1] (and its mask) is loaded while frame t is resolved; pred_tab[u] only after an emission.
#include "beam_common.h"

namespace sc {

struct RnntDecodeArgs {
  const void* enc;
  const void* pred;
  const void* W;
  const float* bias;
  int B, T, V, J;
  int64_t sb, st;
  const int64_t* lengths;
  const float* mask;
  int64_t mb, mt;
  int blank, max_symbols;
  int32_t* prev;
  int32_t* tokens;
  int32_t* frames;
  int cap;
  int32_t* counts;
};

constexpr int kDecThreads = 1024, kDecWaves = kDecThreads / 64, kDecMaxJ = 256;
constexpr int kNoIdx = 0x7fffffff;   // index of a lane without a row: loses every comparison

// a beats b?  (decode.hip's `beats`: NaN beats everything; ties -> lower index.)  Written without
// short-circuit operators so that it compiles to compares and selects: as control flow every one
// of the ~10 comparisons of an evaluation's reduction became a divergent branch.
__device__ __forceinline__ bool dec_beats(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb, lower = ia < ib;
  const bool nan_win = na & (!nb | lower);
  const bool num_win = (va > vb) | ((va == vb) & lower);
  return (na | nb) ? nan_win : num_win;
}

template <int DT, bool FAST>
__global__ void __launch_bounds__(kDecThreads) rnnt_decode_kernel(RnntDecodeArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  __shared__ __attribute__((aligned(16))) float zs[kDecMaxJ];
  __shared__ float cv[kDecWaves];
  __shared__ int ci[kDecWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int J = FAST ? 64 : a.J;
  const T* enc = (const T*)a.enc + (int64_t)b * a.sb;
  const T* pred = (const T*)a.pred;
  const T* Wp = (const T*)a.W;

  // fast path: this lane's row of W and its bias, for the whole stream
  float w[FAST ? 64 : 1];
  float bs = 0.0f;
  if constexpr (FAST) {
    constexpr int N = Vec16<DT>::N;
    const int row = min(tid, a.V - 1);   // lanes past V read a valid row and never compete
#pragma unroll
    for (int c = 0; c < 64 / N; ++c) {
      float f[N];
      Vec16<DT>::ld(Wp + (int64_t)row * 64 + c * N, f);
#pragma unroll
      for (int k = 0; k < N; ++k) w[c * N + k] = f[k];
    }
    bs = a.bias[row];
  }

  int len = a.T;
  if (a.lengths) len = (int)min<int64_t>(max<int64_t>(a.lengths[b], 0), a.T);
  int u = uniform(a.prev ? a.prev[b] : a.blank);
  if (u < 0 || u >= a.V) u = a.blank;   // a prev that is no token starts the stream afresh
  int count = 0;
  const bool zlane = tid < J;   // the lanes that compute z (wave 0 when J = 64)
  float pr = 0.0f, e_next = 0.0f, m_next = 1.0f;
  // rows of enc_p and pred_tab through buffer loads: a wave-uniform row base in SGPRs and one
  // constant 32-bit lane offset, instead of a 64-bit address per lane (which spilled)
  const uint32_t voff = (uint32_t)tid * (uint32_t)sizeof(T);
  if (zlane) pr = E::ld(Buf<T>(pred + (int64_t)u * J).ld(voff, 0));
  // frame t + 1's enc_p row and mask are requested once frame t's z is on its way, so the load
  // flies during the evaluation and nothing is outstanding when the next frame needs it (issued
  // before z, the wait for this frame's row would also wait for the row just requested)
  auto fetch = [&](int t) {
    if (t >= len) return;
    if (zlane) e_next = E::ld(Buf<T>(enc + (int64_t)t * a.st).ld(voff, 0));
    if (a.mask) m_next = a.mask[(int64_t)b * a.mb + (int64_t)t * a.mt];
  };
  fetch(0);

  for (int t = 0; t < len; ++t) {
    const float e = e_next;
    if (m_next == 0.0f) {   // a dead frame
      fetch(t + 1);
      continue;
    }
#pragma unroll 1
    for (int s = 0; s < a.max_symbols; ++s) {
      if (zlane) zs[tid] = dec_tanh(e + pr);
      if (s == 0) fetch(t + 1);
      lds_barrier();
      float bv = -__builtin_huge_valf();
      int bi = kNoIdx;
      if constexpr (FAST) {
        float acc[4] = {bs, 0.0f, 0.0f, 0.0f};
        typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const f4 z4 = ((const f4*)zs)[c];   // same address in every lane: a broadcast read
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[4 * c + k], z4[k], acc[k]);
        }
        if (tid < a.V) {
          bv = (acc[0] + acc[1]) + (acc[2] + acc[3]);
          bi = tid;
        }
      } else {
        for (int v = tid; v < a.V; v += kDecThreads) {
          const T* wr = Wp + (int64_t)v * J;
          float acc = a.bias[v];
          for (int j = 0; j < J; ++j) acc = fmaf(E::ld(wr[j]), zs[j], acc);
          if (bi == kNoIdx || dec_beats(acc, v, bv, bi)) {
            bv = acc;
            bi = v;
          }
        }
      }
      wave_argmax<dec_beats>(bv, bi);
      if (lane == 0) {
        cv[wv] = bv;
        ci[wv] = bi;
      }
      lds_barrier();
      // every wave: the 16 wave winners, one per lane of each row
      float fv = cv[lane & (kDecWaves - 1)];
      int fi = ci[lane & (kDecWaves - 1)];
      row_argmax<dec_beats>(fv, fi);
      const int k = uniform(fi);
      if (k == a.blank) break;
      if (tid == 0 && count < a.cap) {
        a.tokens[(int64_t)b * a.cap + count] = k;
        if (a.frames) a.frames[(int64_t)b * a.cap + count] = t;
      }
      ++count;
      u = k;
      if (zlane) pr = E::ld(Buf<T>(pred + (int64_t)u * J).ld(voff, 0));
    }
  }
  if (tid == 0) {
    a.counts[b] = count;
    if (a.prev) a.prev[b] = u;
  }
}

template <int DT>
static void launch(const RnntDecodeArgs& a, bool fast, hipStream_t st) {
  if (fast)
    hipLaunchKernelGGL((rnnt_decode_kernel<DT, true>), dim3(a.B), dim3(kDecThreads), 0, st, a);
  else
    hipLaunchKernelGGL((rnnt_decode_kernel<DT, false>), dim3(a.B), dim3(kDecThreads), 0, st, a);
}

}  // namespace sc

using namespace sc;

extern "C" int sc_rnnt_greedy_decode(const void* enc_p, const void* pred_tab, const void* W,
                                     int dtype, const float* bias, int B, int T, int V, int J,
                                     int64_t stride_b, int64_t stride_t, const int64_t* lengths,
                                     const float* mask, int64_t mask_b, int64_t mask_t, int blank,
                                     int max_symbols, int32_t* prev, int32_t* tokens,
                                     int32_t* frames, int cap, int32_t* counts, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16 || dtype == SC_F16,
             "sc_rnnt_greedy_decode: unsupported dtype %d", dtype);
  SC_REQUIRE(B >= 0 && T >= 0 && V > 0, "sc_rnnt_greedy_decode: bad shape B=%d T=%d V=%d", B, T, V);
  SC_REQUIRE(J >= 1 && J <= kDecMaxJ, "sc_rnnt_greedy_decode: J=%d outside [1, %d]", J, kDecMaxJ);
  SC_REQUIRE(max_symbols >= 1 && max_symbols <= 64,
             "sc_rnnt_greedy_decode: max_symbols=%d outside [1, 64]", max_symbols);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_rnnt_greedy_decode: blank=%d outside [0, V=%d)", blank, V);
  SC_REQUIRE(cap >= 0, "sc_rnnt_greedy_decode: cap=%d is negative", cap);
  if (B == 0) return 0;
  SC_REQUIRE(counts, "sc_rnnt_greedy_decode: counts is null");
  hipStream_t st = (hipStream_t)stream;
  if (T == 0) {
    zero_async(counts, sizeof(int32_t) * B, st);
    return launch_status("sc_rnnt_greedy_decode");
  }
  SC_REQUIRE(enc_p, "sc_rnnt_greedy_decode: enc_p is null");
  SC_REQUIRE(pred_tab, "sc_rnnt_greedy_decode: pred_tab is null");
  SC_REQUIRE(W, "sc_rnnt_greedy_decode: W is null");
  SC_REQUIRE(bias, "sc_rnnt_greedy_decode: bias is null");
  SC_REQUIRE(cap == 0 || tokens, "sc_rnnt_greedy_decode: tokens is null with cap=%d", cap);
  RnntDecodeArgs a{enc_p, pred_tab, W, bias, B, T, V, J, stride_b, stride_t, lengths, mask, mask_b,
                   mask_t, blank, max_symbols, prev, tokens, frames, cap, counts};
  // the register-resident path reads rows of W by 16-byte pieces
  const bool fast = J == 64 && V <= kDecThreads && ((uintptr_t)W & 15) == 0;
  switch (dtype) {
    case SC_F32: launch<SC_F32>(a, fast, st); break;
    case SC_BF16: launch<SC_BF16>(a, fast, st); break;
    default: launch<SC_F16>(a, fast, st); break;
  }
  return launch_status("sc_rnnt_greedy_decode");
}
