// What the CTC and RNN-T beam decoders (ctc_beam.hip, rnnt_beam.hip) share, and the wave argmax
// and tanh they share with the greedy RNN-T decoder (rnnt_decode.hip): the orders and keys of the
// rankings, the top_k rounds over a row, the list-and-rank step, and the per-stream state with
// its reset and result kernels and their argument checks.  DESIGN.md §3.5d describes the pieces.
#pragma once

#include <stdio.h>

#include "sc_common.h"

namespace sc {

constexpr int kBeamMax = 32, kTopkMax = 32, kSymMax = 8;
constexpr int kRankAll = 128;   // up to this many candidates are ranked without a floor
constexpr int kNoTok = -1;
constexpr float kNegInf = -__builtin_huge_valf();

// lae(a, b) = max(a, b) + log1p(exp(-|a - b|)), lae(-inf, b) = b
__device__ __forceinline__ float lae(float a, float b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  return fmaxf(a, b) + log1pf(expf(-fabsf(a - b)));
}
// Prefix identity is (64-bit rolling hash of the tokens, length), not a comparison of tokens.
__device__ __forceinline__ uint64_t hash_push(uint64_t h, int c) {
  h = (h ^ (uint64_t)(uint32_t)(c + 1)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 32);
}
// (value, index) order of the rankings: larger value first, NaN as -inf, ties to the lower index
__device__ __forceinline__ float rank_key(float v) { return v != v ? kNegInf : v; }
__device__ __forceinline__ bool key_beats(float ka, int ia, float kb, int ib) {
  return (ka > kb) | ((ka == kb) & (ia < ib));
}
// a candidate as one sortable word: larger total first (NaN never gets here), then the lower index
__device__ __forceinline__ uint64_t cand_key(float tot, int c) {
  uint32_t u = __float_as_uint(tot + 0.0f);   // -0 -> +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)c);
}
__device__ __forceinline__ int key_cand(uint64_t key) { return (int)(0xffffffffu - (uint32_t)key); }
// tanh in expf form, ~1e-7 absolute; NaN stays NaN
__device__ __forceinline__ float dec_tanh(float x) {
  return 1.0f - 2.0f * rcp(exp2_(2.0f * kLog2e * x) + 1.0f);
}
// An opaque copy of a lane-varying value.  What a phase of a walk derives from its own copy
// (lane masks, LDS addresses) cannot be computed once before the frame loop and kept alive across
// the RNN-T dot products, where the row of W leaves 64 registers for everything else.
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// ------------------------------------------------------------------ (value, index) argmax ----
// BEATS(va, ia, vb, ib): a strict total order written as compares and selects (key_beats here,
// dec_beats in rnnt_decode.hip); being total, any reduction tree finds the same winner.
using Beats = bool (*)(float, int, float, int);

// one DPP exchange inside a row of 16 lanes (every lane has a partner), keeping the winner
template <Beats BEATS, int CTRL>
__device__ __forceinline__ void argmax_dpp(float& v, int& i) {
  const float ov = __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
  const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false);
  const bool take = BEATS(ov, oi, v, i);
  v = take ? ov : v;
  i = take ? oi : i;
}
// after this every lane of a 16-lane row holds its row's winner
template <Beats BEATS>
__device__ __forceinline__ void row_argmax(float& v, int& i) {
  argmax_dpp<BEATS, 0xB1>(v, i);    // quad_perm [1,0,3,2]
  argmax_dpp<BEATS, 0x4E>(v, i);    // quad_perm [2,3,0,1]
  argmax_dpp<BEATS, 0x141>(v, i);   // row_half_mirror
  argmax_dpp<BEATS, 0x140>(v, i);   // row_mirror
}
// after this every lane holds the wave's winner: rows of 16 on DPP, then the four row winners
// (lanes 0, 16, 32, 48)
template <Beats BEATS>
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
  row_argmax<BEATS>(v, i);
  float wv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  int wi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
    const int oi = __builtin_amdgcn_readlane(i, r);
    const bool take = BEATS(ov, oi, wv, wi);
    wv = take ? ov : wv;
    wi = take ? oi : wi;
  }
  v = wv;
  i = wi;
}

// ------------------------------------------------------------------ top_k rounds -------------
// One wave ranks the top_k non-blank elements of a row of V keys: round j finds the best element
// strictly after round j - 1's winner.  scan(pk, pi, bk, bi) improves the lane's best (bk, bi)
// among its elements after (pk, pi); reduce(bk, bi) leaves the wave's winner in every lane;
// emit(j, index) stores it.  top_k <= V - 1 non-blank elements: a winner exists in every round.
template <class Scan, class Reduce, class Emit>
__device__ __forceinline__ void topk_rounds(int top_k, int V, Scan scan, Reduce reduce, Emit emit) {
  float pk = __builtin_huge_valf();
  int pi = -1;
  for (int j = 0; j < top_k; ++j) {
    float bk = kNegInf;
    int bi = 0x7fffffff;
    scan(pk, pi, bk, bi);
    reduce(bk, bi);
    bi = min(bi, V - 1);
    emit(j, bi);
    pk = bk;
    pi = bi;
  }
}
// lane `lane` holds elements lane, lane + 64, ...; key(v) reads one (an LDS row, or memory)
template <class Key, class Reduce, class Emit>
__device__ __forceinline__ void topk_rounds_row(int top_k, int V, int blank, int lane, Key key,
                                                Reduce reduce, Emit emit) {
  topk_rounds(top_k, V, [&](float pk, int pi, float& bk, int& bi) {
    for (int v = lane; v < V; v += 64) {
      const float k = key(v);
      const bool after = key_beats(pk, pi, k, v);
      if (after & (v != blank) & key_beats(k, v, bk, bi)) {
        bk = k;
        bi = v;
      }
    }
  }, reduce, emit);
}
// V <= 1024 and the lane's 16 keys in registers: compares and selects on registers, no reads
template <class Reduce, class Emit>
__device__ __forceinline__ void topk_rounds_regs(int top_k, int V, int blank, int lane,
                                                 const float (&rv)[16], Reduce reduce, Emit emit) {
  topk_rounds(top_k, V, [&](float pk, int pi, float& bk, int& bi) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int v = lane + 64 * q;
      const bool after = key_beats(pk, pi, rv[q], v), best = key_beats(rv[q], v, bk, bi);
      const bool take = after & best & (v < V) & (v != blank);
      bk = take ? rv[q] : bk;
      bi = take ? v : bi;
    }
  }, reduce, emit);
}

// ------------------------------------------------------------------ list and rank ------------
// Wave 0, lane's value v (-inf where it has none): the beam-th largest of the 64 goes to *theta.
// A candidate below that floor has `beam` candidates above it and beats none that is not below it.
__device__ __forceinline__ void beam_floor(float v, int lane, int beam, float* theta) {
  v = v > kNegInf ? v : kNegInf;
  int above = 0;
#pragma unroll 8
  for (int o = 0; o < 64; ++o) {
    const float ov = __shfl(v, o);
    above += ((ov > v) | ((ov == v) & (o < lane))) ? 1 : 0;
  }
  if (above == beam - 1) *theta = v;
}
// The workgroup's nthr threads keep the `beam` largest of nc candidates.  Those whose total
// tot(c) is at or above floor_v (-inf and NaN are dropped) go to the list as sortable keys |
// barrier | the rank of each is the number of listed keys that beat it (larger total; ties: the
// earlier candidate); write(c, rank) stores the ranks below `beam` and *n_next becomes their
// count | barrier.  The caller zeroes *n_keys and *n_next a barrier earlier.
template <int UNROLL, class Tot, class Write>
__device__ __forceinline__ void list_and_rank(int tid, int nthr, int nc, float floor_v, int beam,
                                              uint64_t* keys, int* n_keys, int* n_next, Tot tot,
                                              Write write) {
  for (int c = opaque(tid); c < nc; c += nthr) {
    const float tc = tot(c);
    if (tc > kNegInf && !(tc < floor_v)) keys[atomicAdd(n_keys, 1)] = cand_key(tc, c);
  }
  __syncthreads();
  const int nk = uniform(*n_keys);
  for (int k = opaque(tid); k < nk; k += nthr) {
    const uint64_t kc = keys[k];
    int rank = 0;
#pragma unroll UNROLL
    for (int o = 0; o < nk; ++o) rank += keys[o] > kc ? 1 : 0;
    if (rank >= beam) continue;
    atomicMax(n_next, rank + 1);
    write(key_cand(kc), rank);
  }
  __syncthreads();
}

// ------------------------------------------------------------------ state --------------------
// per stream, 8-byte aligned, NS score floats per entry (CTC: pb, pnb; RNN-T: score) and
// max_symbols = ms (CTC: 0):
//   int32  hdr[4]       live frames consumed, status, hypotheses alive, beam | ms << 8
//   uint64 hash[beam];  float score[NS][beam];  int32 node[beam], len[beam], last[beam]
//   int32  trie[1 + max_frames * max(ms, 1) * beam][2]   (parent, token), node 0: the empty prefix
struct BeamLayout {
  size_t hdr, stream;   // bytes before the trie, bytes of one stream
  int64_t max_frames;
};
static int beam_frame_nodes(int beam, int ms) { return beam * (ms > 0 ? ms : 1); }
static size_t beam_hdr_bytes(int ns, int beam) {
  return ((size_t)16 + (20 + 4 * (size_t)ns) * (size_t)beam + 7) & ~(size_t)7;
}
static size_t beam_stream_bytes(int ns, int beam, int ms, int64_t max_frames) {
  return beam_hdr_bytes(ns, beam) + 8 * (1 + (size_t)max_frames * beam_frame_nodes(beam, ms));
}
// ns == 1 is the RNN-T state, whose ms is 1 .. kSymMax; ns == 2 the CTC state, whose ms is 0
static bool beam_ms_ok(int ns, int ms) { return ns == 2 ? ms == 0 : ms >= 1 && ms <= kSymMax; }
// sc_*_beam_state_bytes: 0 where (B, beam, ms, max_frames) describe no state
static size_t beam_state_bytes(int ns, int B, int beam, int ms, int max_frames) {
  if (B < 0 || beam < 1 || beam > kBeamMax || !beam_ms_ok(ns, ms) || max_frames < 0) return 0;
  if ((size_t)max_frames * (size_t)beam_frame_nodes(beam, ms) >= (size_t)0x7ffffff0) return 0;
  return (size_t)B * beam_stream_bytes(ns, beam, ms, max_frames);
}
// the layout of a state of state_bytes bytes for B streams; max_frames < 0 when it is none
static BeamLayout beam_layout(int ns, size_t state_bytes, int B, int beam, int ms) {
  BeamLayout L{beam_hdr_bytes(ns, beam), 0, -1};
  if (B <= 0 || state_bytes % (size_t)B) return L;
  L.stream = state_bytes / (size_t)B;
  const size_t per = 8 * (size_t)beam_frame_nodes(beam, ms);
  if (L.stream < L.hdr + 8 || (L.stream - L.hdr - 8) % per) return L;
  const size_t mf = (L.stream - L.hdr - 8) / per;
  if (mf * (per / 8) < (size_t)0x7ffffff0) L.max_frames = (int64_t)mf;
  return L;
}

struct BeamView {   // one stream's arrays; score is [NS][beam]
  int32_t* hdr;
  uint64_t* hash;
  float* score;
  int32_t *node, *len, *last, *trie;
};
template <int NS>
__device__ __forceinline__ BeamView beam_view(void* state, size_t stream_bytes, size_t hdr_bytes,
                                              int b, int beam) {
  char* p = (char*)state + (size_t)b * stream_bytes;
  BeamView v;
  v.hdr = (int32_t*)p;
  v.hash = (uint64_t*)(p + 16);
  v.score = (float*)(p + 16 + 8 * (size_t)beam);
  v.node = (int32_t*)(v.score + NS * beam);
  v.len = v.node + beam;
  v.last = v.len + beam;
  v.trie = (int32_t*)(p + hdr_bytes);
  return v;
}
__device__ __forceinline__ int beam_tag(int beam, int ms) { return beam | (ms << 8); }

struct BeamResetArgs {
  void* state;
  size_t stream_bytes, hdr_bytes;
  int B, beam, ms;
  const float* streams;
};
// the whole state, or the streams whose entry is non-zero, back to [(empty prefix, score 0)]
template <int NS>
__global__ void __launch_bounds__(64) beam_reset_kernel(BeamResetArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (a.streams && a.streams[b] == 0.0f) return;
  const BeamView s = beam_view<NS>(a.state, a.stream_bytes, a.hdr_bytes, b, a.beam);
  if (i < a.beam) {   // entry 0: the empty prefix; the rest: dead
    s.hash[i] = 0;
    s.score[i] = i == 0 ? 0.0f : kNegInf;
    if (NS == 2) s.score[a.beam + i] = kNegInf;
    s.node[i] = 0;
    s.len[i] = 0;
    s.last[i] = kNoTok;
  }
  if (i == 0) {
    s.hdr[0] = 0;
    s.hdr[1] = 0;
    s.hdr[2] = 1;
    s.hdr[3] = beam_tag(a.beam, a.ms);
    s.trie[0] = -1;
    s.trie[1] = kNoTok;
  }
}

struct BeamResultArgs {
  const void* state;
  size_t stream_bytes, hdr_bytes;
  int B, beam, ms, nbest, cap, max_frames;
  int32_t* tokens;
  int32_t* frames;   // optional: the live frame of each token, read off its node
  int32_t* lens;
  float* scores;
  int32_t* status;
};
// one lane per (stream, hypothesis): walks the parent pointers and writes the tokens forwards
// from the stored length
template <int NS>
__global__ void __launch_bounds__(64) beam_result_kernel(BeamResultArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  const BeamView s = beam_view<NS>((void*)a.state, a.stream_bytes, a.hdr_bytes, b, a.beam);
  const bool ok = s.hdr[3] == beam_tag(a.beam, a.ms);
  if (i == 0 && a.status) a.status[b] = ok ? s.hdr[1] : 2;
  if (i >= a.nbest) return;
  const int64_t o = (int64_t)b * a.nbest + i;
  const int n = ok ? min(max(s.hdr[2], 0), a.beam) : 0;
  if (i >= n) {
    a.lens[o] = -1;
    a.scores[o] = kNegInf;
    return;
  }
  const int L = s.len[i];
  a.lens[o] = L;
  a.scores[o] = NS == 2 ? lae(s.score[i], s.score[a.beam + i]) : s.score[i];
  const int per = a.beam * max(a.ms, 1);   // nodes of one live frame
  const int64_t nodes = 1 + (int64_t)a.max_frames * per;
  int node = s.node[i];
  // backwards along the parent pointers, written forwards; a state that is not one (a node
  // outside the trie) ends the walk
  for (int pos = L - 1; pos >= 0 && node > 0 && node < nodes; --pos) {
    const int parent = s.trie[2 * (size_t)node], tok = s.trie[2 * (size_t)node + 1];
    if (pos < a.cap) {
      a.tokens[o * a.cap + pos] = tok;
      if (a.frames) a.frames[o * a.cap + pos] = (node - 1) / per;
    }
    if (parent >= node) break;   // parents precede their children
    node = parent;
  }
}

// ------------------------------------------------------------------ entry points (host) ------
// What the sc_ctc_beam_* (NS = 2, ms = 0) and sc_rnnt_beam_* (NS = 1) entry points share; fn is
// the entry point's name for the messages.  A check returns 0 or SC_EINVAL with the message set.
static int beam_check_shape(const char* fn, int ns, int beam, int ms) {
  SC_REQUIRE(beam >= 1 && beam <= kBeamMax, "%s: beam=%d outside [1, %d]", fn, beam, kBeamMax);
  SC_REQUIRE(beam_ms_ok(ns, ms), "%s: max_symbols=%d outside [1, %d]", fn, ms, kSymMax);
  return 0;
}
static int beam_check_state_ptr(const char* fn, const void* state) {
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "%s: state is a null pointer or not 8-byte aligned", fn);
  return 0;
}
// "sc_ctc_beam_state_bytes(B=.., beam=.., " or its RNN-T form with max_symbols, for the messages
struct BeamSizeCall {
  char s[96];
  BeamSizeCall(int ns, int B, int beam, int ms) {
    if (ns == 2) snprintf(s, sizeof s, "sc_ctc_beam_state_bytes(B=%d, beam=%d, ", B, beam);
    else snprintf(s, sizeof s, "sc_rnnt_beam_state_bytes(B=%d, beam=%d, max_symbols=%d, ", B, beam, ms);
  }
};
// the layout of a state whose max_frames the caller does not know (frames, result)
static int beam_check_layout(const char* fn, int ns, size_t state_bytes, int B, int beam, int ms,
                             BeamLayout* L) {
  *L = beam_layout(ns, state_bytes, B, beam, ms);
  SC_REQUIRE(L->max_frames >= 0, "%s: state_bytes=%zu is no %s.)", fn, state_bytes,
             BeamSizeCall(ns, B, beam, ms).s);
  return 0;
}

template <int NS>
static int beam_reset(const char* fn, void* state, size_t state_bytes, int B, int beam, int ms,
                      int max_frames, const float* streams, void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "%s: bad shape B=%d", fn, B);
  if (beam_check_shape(fn, NS, beam, ms)) return SC_EINVAL;
  SC_REQUIRE(max_frames >= 0, "%s: max_frames=%d is negative", fn, max_frames);
  if (B == 0) return 0;
  if (beam_check_state_ptr(fn, state)) return SC_EINVAL;
  const size_t want = beam_state_bytes(NS, B, beam, ms, max_frames);
  SC_REQUIRE(want != 0 && state_bytes == want, "%s: state_bytes=%zu is not %smax_frames=%d)=%zu", fn,
             state_bytes, BeamSizeCall(NS, B, beam, ms).s, max_frames, want);
  BeamResetArgs a{state, beam_stream_bytes(NS, beam, ms, max_frames), beam_hdr_bytes(NS, beam), B,
                  beam, ms, streams};
  hipLaunchKernelGGL(beam_reset_kernel<NS>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

template <int NS>
static int beam_result(const char* fn, const void* state, size_t state_bytes, int B, int beam,
                       int ms, int nbest, int32_t* tokens, int32_t* frames, int cap, int32_t* lens,
                       float* scores, int32_t* status, void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "%s: bad shape B=%d", fn, B);
  if (beam_check_shape(fn, NS, beam, ms)) return SC_EINVAL;
  SC_REQUIRE(nbest >= 1 && nbest <= beam, "%s: nbest=%d outside [1, beam=%d]", fn, nbest, beam);
  SC_REQUIRE(cap >= 0, "%s: cap=%d is negative", fn, cap);
  if (B == 0) return 0;
  if (beam_check_state_ptr(fn, state)) return SC_EINVAL;
  SC_REQUIRE(lens && scores, "%s: lens or scores is a null pointer", fn);
  SC_REQUIRE(cap == 0 || tokens, "%s: tokens is a null pointer with cap=%d", fn, cap);
  BeamLayout L;
  if (beam_check_layout(fn, NS, state_bytes, B, beam, ms, &L)) return SC_EINVAL;
  BeamResultArgs a{state, L.stream, L.hdr, B, beam, ms, nbest, cap, (int)L.max_frames, tokens,
                   frames, lens, scores, status};
  hipLaunchKernelGGL(beam_result_kernel<NS>, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // namespace sc

