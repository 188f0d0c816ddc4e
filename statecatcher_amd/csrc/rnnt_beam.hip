// Transducer (RNN-T) beam search on device for the stateless predictor of RNNTPredictorJoiner,
// offline and chunked (include/statecatcher.h, sc_rnnt_beam_*).
//
// sc_rnnt_greedy_decode follows one path and returns no score.  This is the time-synchronous beam
// search over the same joint: a hypothesis is a token prefix and one score, the predictor being a
// [V, J] table of the last token.  All arithmetic is fp32; inputs are widened on load; z = tanh(..)
// has the greedy kernel's form; lp = logit - logsumexp(logit); lae as in ctc_beam.hip.
//
// Three kernels:
//   rbeam_reset_kernel   the whole state or the selected streams back to [(empty, 0)]
//   rbeam_walk_kernel    one persistent workgroup of 1024 threads per stream consumes the call's
//                        frames.  Per live frame, for r = 0 .. max_symbols, with C the round's
//                        hypotheses (the beam when r = 0):
//                          z of every hypothesis of C -> LDS | barrier |
//                          in passes of 16 hypotheses: every lane forms its row's logit for each
//                          (FAST: the row of W in registers) -> image [16][V] | barrier | wave w:
//                          max, sum of exponentials, lp[blank] and the top_k rounds of hypothesis
//                          w of the pass (as ctc_beam.hip's beam_rows_kernel) | barrier |
//                          wave 0: blank steps into A (merge by (hash, length), else append in
//                          order) and a floor under the beam-th largest extension | barrier |
//                          extensions at or above the floor -> key list | barrier | rank by
//                          counting, the first `beam` ranks are the next C and get trie nodes.
//                        Then the `beam` largest of A are the new beam.  Every branch is
//                        workgroup-uniform; every loop is bounded by T, max_symbols, beam, top_k,
//                        V or J; nothing waits on another workgroup; nothing is allocated or
//                        counted atomically in memory.
//     <DT, true>   J = 64, V <= 1024, W 16-byte aligned: lane v keeps row v of W in registers,
//                  the image lives in LDS (64 KB dynamic) and a wave's row statistics keep each
//                  lane's 16 elements of the row in registers through the top_k rounds
//     <DT, false>  any V, J <= 256: rows of W are read from memory and the image lives in the
//                  workspace (correct, not tuned)
//   rbeam_result_kernel  one lane per (stream, hypothesis) walks the parent pointers
//
// Token history is a parent-pointer trie in the state: node 0 is the empty prefix, the candidate
// kept at rank k of round r of live frame f is node 1 + (f * max_symbols + r) * beam + k =
// (parent node, token), so nothing is counted in memory and a token's frame is read off its node.
#include "sc_common.h"

namespace sc {
namespace rbeam {

constexpr int kBeamMax = 32, kTopkMax = 32, kSymMax = 8;
constexpr int kAMax = kBeamMax * (kSymMax + 1);   // entries of one frame's A
constexpr int kThreads = 1024, kMaxJ = 256;
constexpr int kRows = 16;                         // hypotheses of one pass: one per wave
constexpr int kRankAll = 128;                     // up to this many extensions are ranked without a floor
constexpr int kNoTok = -1;
constexpr float kNegInf = -__builtin_huge_valf();

// ------------------------------------------------------------------ state layout -------------
// per stream, 8-byte aligned:
//   int32  hdr[4]       live frames consumed, status, hypotheses alive, beam | max_symbols << 8
//   uint64 hash[beam];  float score[beam];  int32 node[beam], len[beam], last[beam]
//   int32  trie[1 + max_frames * max_symbols * beam][2]   (parent, token)
struct Layout {
  size_t hdr, stream;
  int64_t max_frames;
};
static size_t hdr_bytes(int beam) { return (size_t)16 + 24 * (size_t)beam; }
static size_t stream_bytes(int beam, int ms, int64_t max_frames) {
  return hdr_bytes(beam) + 8 * (1 + (size_t)max_frames * ms * beam);
}
static Layout layout(size_t state_bytes, int B, int beam, int ms) {
  Layout L{hdr_bytes(beam), 0, -1};
  if (B <= 0 || state_bytes % (size_t)B) return L;
  L.stream = state_bytes / (size_t)B;
  const size_t per = 8 * (size_t)beam * ms;
  if (L.stream < L.hdr + 8 || (L.stream - L.hdr - 8) % per) return L;
  const size_t mf = (L.stream - L.hdr - 8) / per;
  if (mf * (size_t)beam * ms < (size_t)0x7ffffff0) L.max_frames = (int64_t)mf;
  return L;
}

struct View {
  int32_t* hdr;
  uint64_t* hash;
  float* score;
  int32_t *node, *len, *last, *trie;
};
__device__ __forceinline__ View view(void* state, size_t stream, size_t hdr, int b, int beam) {
  char* p = (char*)state + (size_t)b * stream;
  View v;
  v.hdr = (int32_t*)p;
  v.hash = (uint64_t*)(p + 16);
  v.score = (float*)(p + 16 + 8 * (size_t)beam);
  v.node = (int32_t*)(v.score + beam);
  v.len = v.node + beam;
  v.last = v.len + beam;
  v.trie = (int32_t*)(p + hdr);
  return v;
}

// ctc_beam.hip's helpers, unchanged
__device__ __forceinline__ float lae(float a, float b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  return fmaxf(a, b) + log1pf(expf(-fabsf(a - b)));
}
__device__ __forceinline__ uint64_t hash_push(uint64_t h, int c) {
  h = (h ^ (uint64_t)(uint32_t)(c + 1)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 32);
}
__device__ __forceinline__ float rank_key(float v) { return v != v ? kNegInf : v; }
__device__ __forceinline__ bool key_beats(float ka, int ia, float kb, int ib) {
  return (ka > kb) | ((ka == kb) & (ia < ib));
}
__device__ __forceinline__ uint64_t cand_key(float tot, int c) {
  uint32_t u = __float_as_uint(tot + 0.0f);   // -0 -> +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)c);
}
// (key, index) argmax of a wave on DPP, as rnnt_decode.hip's row_argmax but in key_beats' order:
// one exchange inside a row of 16 lanes (every lane has a partner), keeping the winner
template <int CTRL>
__device__ __forceinline__ void kmax_dpp(float& k, int& i) {
  const float ok = __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(k), __float_as_int(k), CTRL, 0xf, 0xf, false));
  const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false);
  const bool take = key_beats(ok, oi, k, i);
  k = take ? ok : k;
  i = take ? oi : i;
}
// after this every lane holds the wave's winner (the order is total: any reduction tree agrees)
__device__ __forceinline__ void wave_kmax(float& k, int& i) {
  kmax_dpp<0xB1>(k, i);    // quad_perm [1,0,3,2]
  kmax_dpp<0x4E>(k, i);    // quad_perm [2,3,0,1]
  kmax_dpp<0x141>(k, i);   // row_half_mirror
  kmax_dpp<0x140>(k, i);   // row_mirror: every lane of a row holds its row's winner
  float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k), 0));
  int wi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    const float ok = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k), r));
    const int oi = __builtin_amdgcn_readlane(i, r);
    const bool take = key_beats(ok, oi, wk, wi);
    wk = take ? ok : wk;
    wi = take ? oi : wi;
  }
  k = wk;
  i = wi;
}
// An opaque copy of a lane-varying value.  What a phase of the walk derives from its own copy
// (lane masks, LDS addresses) cannot be computed once before the frame loop and kept alive across
// the dot products, where the row of W leaves 64 registers for everything else.
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
// rnnt_decode.hip's tanh: expf form, ~1e-7 absolute; NaN stays NaN
__device__ __forceinline__ float dec_tanh(float x) {
  return 1.0f - 2.0f * rcp(exp2_(2.0f * kLog2e * x) + 1.0f);
}

// ------------------------------------------------------------------ reset --------------------
struct ResetArgs {
  void* state;
  size_t stream, hdr;
  int B, beam, ms;
  const float* streams;
};

__global__ void __launch_bounds__(64) rbeam_reset_kernel(ResetArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (a.streams && a.streams[b] == 0.0f) return;
  const View s = view(a.state, a.stream, a.hdr, b, a.beam);
  if (i < a.beam) {   // entry 0: the empty prefix; the rest: dead
    s.hash[i] = 0;
    s.score[i] = i == 0 ? 0.0f : kNegInf;
    s.node[i] = 0;
    s.len[i] = 0;
    s.last[i] = kNoTok;
  }
  if (i == 0) {
    s.hdr[0] = 0;
    s.hdr[1] = 0;
    s.hdr[2] = 1;
    s.hdr[3] = a.beam | (a.ms << 8);
    s.trie[0] = -1;
    s.trie[1] = kNoTok;
  }
}

// ------------------------------------------------------------------ walk ---------------------
struct WalkArgs {
  const void* enc;
  const void* pred;
  const void* W;
  const float* bias;
  int B, T, V, J;
  int64_t sb, st;
  const int64_t* lengths;
  const float* mask;
  int64_t mb, mt;
  int blank, beam, top_k, ms;
  void* state;
  size_t stream, hdr;
  int max_frames;
  float* ws;   // general path: the logit image, [B][kRows][V]
};

struct Ents {   // the hypotheses of one round
  uint64_t hash[kBeamMax];
  float score[kBeamMax];
  int node[kBeamMax], len[kBeamMax], last[kBeamMax];
};
struct AEnts {   // one frame's A, in insertion order
  uint64_t hash[kAMax];
  float score[kAMax];
  int node[kAMax], len[kAMax], last[kAMax];
};

template <int DT, bool FAST>
__global__ void __launch_bounds__(kThreads) rbeam_walk_kernel(WalkArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  constexpr int JS = FAST ? 64 : kMaxJ;
  extern __shared__ __attribute__((aligned(16))) float img_lds[];   // FAST: [kRows][V]
  __shared__ __attribute__((aligned(16))) float zs[kBeamMax][JS];
  __shared__ float es[JS];
  __shared__ Ents ents[2];
  __shared__ AEnts A;
  __shared__ float lpb[kBeamMax], tk_lp[kBeamMax][kTopkMax];
  __shared__ int tk_idx[kBeamMax][kTopkMax];
  __shared__ uint64_t keys[kBeamMax * kTopkMax];
  __shared__ int n_cnt[2], n_keys, n_a;
  __shared__ float theta;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int J = FAST ? 64 : a.J, V = a.V, Bm = a.beam, K = a.top_k, MS = a.ms;
  const View s = view(a.state, a.stream, a.hdr, b, Bm);
  if (s.hdr[3] != (Bm | (MS << 8))) {   // not a state of this shape: touch nothing else
    if (tid == 0) s.hdr[1] |= 2;
    return;
  }
  const T* enc = (const T*)a.enc + (int64_t)b * a.sb;
  const T* pred = (const T*)a.pred;
  const T* Wp = (const T*)a.W;
  float* img = FAST ? img_lds : a.ws + (size_t)b * kRows * V;

  // fast path: this lane's row of W and its bias, for the whole call
  float w[FAST ? 64 : 1];
  float bs = 0.0f;
  if constexpr (FAST) {
    constexpr int N = Vec16<DT>::N;
    const int row = min(tid, V - 1);   // lanes past V read a valid row and store nothing
#pragma unroll
    for (int c = 0; c < 64 / N; ++c) {
      float f[N];
      Vec16<DT>::ld(Wp + (int64_t)row * 64 + c * N, f);
#pragma unroll
      for (int k = 0; k < N; ++k) w[c * N + k] = f[k];
    }
    bs = a.bias[row];
  }

  int f = uniform(s.hdr[0]), status = uniform(s.hdr[1]);
  int n = uniform(min(max(s.hdr[2], 0), Bm));
  int cur = 0;
  if (tid < Bm) {
    Ents& q = ents[0];
    q.hash[tid] = s.hash[tid];
    q.score[tid] = s.score[tid];
    q.node[tid] = s.node[tid];
    q.len[tid] = s.len[tid];
    q.last[tid] = s.last[tid];
  }
  int len = a.T;
  if (a.lengths) len = (int)min<int64_t>(max<int64_t>(a.lengths[b], 0), a.T);
  // frame t + 1's enc_p row and mask are requested while frame t is resolved
  float e_next = 0.0f, m_next = 1.0f;
  // rows of enc_p through buffer loads: a wave-uniform row base in SGPRs and one 32-bit lane
  // offset, instead of a 64-bit address per lane (which spilled, as in rnnt_decode.hip)
  const uint32_t voff = (uint32_t)tid * (uint32_t)sizeof(T);
  auto fetch = [&](int t) {
    if (t >= len) return;
    if (tid < J) e_next = E::ld(Buf<T>(enc + (int64_t)t * a.st).ld(voff, 0));
    if (a.mask) m_next = a.mask[(int64_t)b * a.mb + (int64_t)t * a.mt];
  };
  fetch(0);
  __syncthreads();

  for (int t = 0; t < len; ++t) {
    const float e_cur = e_next;
    const bool live = m_next != 0.0f;
    fetch(t + 1);
    if (!live) continue;
    if (f >= a.max_frames) {   // the trie is full: this and every later live frame is ignored
      status |= 1;
      break;
    }
    if (tid < J) es[tid] = e_cur;
    if (tid == 0) n_a = 0;
    // (the barrier after z below orders both before their first readers)

#pragma unroll 1
    for (int r = 0; r <= MS; ++r) {
      const Ents& q = ents[cur];
      Ents& nx = ents[cur ^ 1];
      const bool expand = r < MS;
      if (tid == 0) {
        n_cnt[cur ^ 1] = 0;
        n_keys = 0;
        theta = kNegInf;
      }
      __syncthreads();
      // z of every hypothesis of the round
      for (int e = opaque(tid); e < n * J; e += kThreads) {
        const int i = e / J, j = e - i * J;
        const int u = q.last[i] < 0 ? a.blank : q.last[i];
        zs[i][j] = dec_tanh(es[j] + E::ld(pred[(int64_t)u * J + j]));
      }
      __syncthreads();
#pragma unroll 1
      for (int r0 = 0; r0 < n; r0 += kRows) {
        const int nr = min(kRows, n - r0);
        if constexpr (FAST) {
          typedef float f4 __attribute__((ext_vector_type(4)));
          const int tv = opaque(tid);
#pragma unroll 1
          for (int i = 0; i < nr; ++i) {
            float acc[4] = {bs, 0.0f, 0.0f, 0.0f};
            const f4* zr = (const f4*)zs[r0 + i];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              const f4 z4 = zr[c];   // same address in every lane: a broadcast read
#pragma unroll
              for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[4 * c + k], z4[k], acc[k]);
            }
            if (tv < V) img[(size_t)i * V + tv] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
          }
        } else {
          for (int v = tid; v < V; v += kThreads) {
            const T* wr = Wp + (int64_t)v * J;
            const float bv = a.bias[v];
            for (int i = 0; i < nr; ++i) {
              float acc = bv;
              for (int j = 0; j < J; ++j) acc = fmaf(E::ld(wr[j]), zs[r0 + i][j], acc);
              img[(size_t)i * V + v] = acc;
            }
          }
        }
        __syncthreads();
        const int ts = opaque(tid);
        if ((ts >> 6) < nr) {   // wave wv: hypothesis r0 + wv of the round
          const int lane = ts & 63, wv = ts >> 6;
          const int i = r0 + wv;
          const float* row = img + (size_t)wv * V;
          if constexpr (FAST) {
            // V <= 1024: the lane's 16 elements of the row stay in registers from here on, so the
            // top_k rounds are compares on registers instead of dependent LDS reads
            float rv[16];
            float mx = kNegInf;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int v = lane + 64 * q;
              rv[q] = v < V ? row[v] : kNegInf;
              mx = fmaxf(mx, rv[q]);   // (a NaN never enters mx)
            }
            mx = wave_max_dpp(mx);
            float sm = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) sm += lane + 64 * q < V ? expf(rv[q] - mx) : 0.0f;
            sm = wave_sum_dpp(sm);
            const float lse = mx + logf(sm);
            if (lane == 0) lpb[i] = row[a.blank] - lse;
            if (expand) {
#pragma unroll
              for (int q = 0; q < 16; ++q) rv[q] = rank_key(rv[q] - lse);
              float pk = __builtin_huge_valf();
              int pi = -1;
              for (int j = 0; j < K; ++j) {
                float bk = kNegInf;
                int bi = 0x7fffffff;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                  const int v = lane + 64 * q;
                  const bool after = key_beats(pk, pi, rv[q], v), best = key_beats(rv[q], v, bk, bi);
                  const bool take = after & best & (v < V) & (v != a.blank);
                  bk = take ? rv[q] : bk;
                  bi = take ? v : bi;
                }
                wave_kmax(bk, bi);
                bi = min(bi, V - 1);
                if (lane == 0) {
                  tk_idx[i][j] = bi;
                  tk_lp[i][j] = row[bi] - lse;
                }
                pk = bk;
                pi = bi;
              }
            }
          } else {
            float mx = kNegInf;
            for (int v = lane; v < V; v += 64) mx = fmaxf(mx, row[v]);   // (a NaN never enters mx)
            mx = wave_max_dpp(mx);
            float sm = 0.0f;
            for (int v = lane; v < V; v += 64) sm += expf(row[v] - mx);
            sm = wave_sum_dpp(sm);
            const float lse = mx + logf(sm);
            if (lane == 0) lpb[i] = row[a.blank] - lse;
            if (expand) {
              // top_k rounds: the best non-blank element strictly after the previous round's winner
              float pk = __builtin_huge_valf();
              int pi = -1;
              for (int j = 0; j < K; ++j) {
                float bk = kNegInf;
                int bi = 0x7fffffff;
                for (int v = lane; v < V; v += 64) {
                  const float k = rank_key(row[v] - lse);
                  const bool after = key_beats(pk, pi, k, v);
                  if (after & (v != a.blank) & key_beats(k, v, bk, bi)) {
                    bk = k;
                    bi = v;
                  }
                }
                wave_kmax(bk, bi);
                // top_k <= V - 1 non-blank elements: a winner exists in every round
                bi = min(bi, V - 1);
                if (lane == 0) {
                  tk_idx[i][j] = bi;
                  tk_lp[i][j] = row[bi] - lse;
                }
                pk = bk;
                pi = bi;
              }
            }
          }
        }
        __syncthreads();
      }
      const int nc = expand ? n * K : 0;
      const int tw = opaque(tid);
      if (tw < 64) {
        const int lane = tw;
        // blank steps, in the round's order: into the entry of A that spells the same prefix
        // (only entries of earlier rounds can), else appended
        const int na = uniform(n_a);
        const bool act = lane < n;
        float s1 = kNegInf;
        uint64_t h = 0;
        int l = 0, hit = -1;
        if (act) {
          s1 = q.score[lane] + lpb[lane];
          h = q.hash[lane];
          l = q.len[lane];
          for (int m = 0; m < na; ++m)
            if (A.len[m] == l && A.hash[m] == h) hit = m;
        }
        const uint64_t fresh = __ballot(act && hit < 0);
        const int pos = na + __popcll(fresh & ((1ull << lane) - 1ull));
        if (act) {
          if (hit >= 0) {
            A.score[hit] = lae(A.score[hit], s1);
          } else {
            A.hash[pos] = h;
            A.score[pos] = s1;
            A.node[pos] = q.node[lane];
            A.len[pos] = l;
            A.last[pos] = q.last[lane];
          }
        }
        if (lane == 0) n_a = na + __popcll(fresh);
        // a floor under the beam-th largest extension, so that few have to be ranked: the
        // beam-th largest among every hypothesis's two best (<= 64 values; nc > kRankAll means
        // top_k >= 5).  An extension below it has `beam` above it.
        if (nc > kRankAll) {
          float v = kNegInf;
          if (lane < 2 * n) v = q.score[lane >> 1] + tk_lp[lane >> 1][lane & 1];
          v = v > kNegInf ? v : kNegInf;
          int above = 0;
#pragma unroll 8
          for (int o = 0; o < 64; ++o) {
            const float ov = __shfl(v, o);
            above += ((ov > v) | ((ov == v) & (o < lane))) ? 1 : 0;
          }
          if (above == Bm - 1) theta = v;
        }
      }
      __syncthreads();
      if (!expand) break;
      // the extensions at or above the floor (-inf and NaN are dropped), as sortable keys:
      // score, then the earlier candidate
      const float floor_v = theta;
      {   // candidate c = 32 i + j: one thread each, in the contract's order
        const int c = opaque(tid), i = c >> 5, j = c & 31;
        const float tc = (i < n && j < K) ? q.score[i] + tk_lp[i][j] : kNegInf;
        if (tc > kNegInf && !(tc < floor_v)) keys[atomicAdd(&n_keys, 1)] = cand_key(tc, c);
      }
      __syncthreads();
      // rank = number of candidates that beat this one; the first `beam` are the next round
      const int nk = uniform(n_keys);
      for (int k = opaque(tid); k < nk; k += kThreads) {
        const uint64_t kc = keys[k];
        const int c = (int)(0xffffffffu - (uint32_t)kc);
        int rank = 0;
#pragma unroll 4
        for (int o = 0; o < nk; ++o) rank += keys[o] > kc ? 1 : 0;
        if (rank >= Bm) continue;
        atomicMax(&n_cnt[cur ^ 1], rank + 1);
        const int i = c >> 5, j = c & 31;
        const int tok = tk_idx[i][j], node = 1 + (f * MS + r) * Bm + rank;
        nx.hash[rank] = hash_push(q.hash[i], tok);
        nx.score[rank] = q.score[i] + tk_lp[i][j];
        nx.node[rank] = node;
        nx.len[rank] = q.len[i] + 1;
        nx.last[rank] = tok;
        s.trie[2 * (size_t)node] = q.node[i];
        s.trie[2 * (size_t)node + 1] = tok;
      }
      __syncthreads();
      cur ^= 1;
      n = uniform(n_cnt[cur]);
      if (n == 0) break;
    }
    // the new beam: the `beam` largest of A (-inf and NaN are dropped; ties to the earlier
    // insertion), sorted descending
    __syncthreads();
    if (tid == 0) {
      n_cnt[cur ^ 1] = 0;
      n_keys = 0;
    }
    __syncthreads();
    {
      Ents& nx = ents[cur ^ 1];
      const int na = uniform(n_a);
      for (int c = opaque(tid); c < na; c += kThreads) {
        const float sc = A.score[c];
        if (!(sc > kNegInf)) continue;
        keys[atomicAdd(&n_keys, 1)] = cand_key(sc, c);
      }
      __syncthreads();
      const int nk = uniform(n_keys);
      for (int k = opaque(tid); k < nk; k += kThreads) {
        const uint64_t kc = keys[k];
        const int c = (int)(0xffffffffu - (uint32_t)kc);
        int rank = 0;
#pragma unroll 4
        for (int o = 0; o < nk; ++o) rank += keys[o] > kc ? 1 : 0;
        if (rank >= Bm) continue;
        atomicMax(&n_cnt[cur ^ 1], rank + 1);
        nx.hash[rank] = A.hash[c];
        nx.score[rank] = A.score[c];
        nx.node[rank] = A.node[c];
        nx.len[rank] = A.len[c];
        nx.last[rank] = A.last[c];
      }
      __syncthreads();
      cur ^= 1;
      n = uniform(n_cnt[cur]);
    }
    ++f;
  }
  __syncthreads();
  int ti = tid;
  asm volatile("" : "+v"(ti));   // fresh addresses: the ones of the load above are not kept alive
  if (ti < Bm) {   // entries past the alive ones leave in their reset form
    const Ents& q = ents[cur];
    const bool on = ti < n;
    s.hash[ti] = on ? q.hash[ti] : 0;
    s.score[ti] = on ? q.score[ti] : kNegInf;
    s.node[ti] = on ? q.node[ti] : 0;
    s.len[ti] = on ? q.len[ti] : 0;
    s.last[ti] = on ? q.last[ti] : kNoTok;
  }
  if (tid == 0) {
    s.hdr[0] = f;
    s.hdr[1] = status;
    s.hdr[2] = n;
  }
}

// ------------------------------------------------------------------ result -------------------
struct ResultArgs {
  const void* state;
  size_t stream, hdr;
  int B, beam, ms, nbest, cap, max_frames;
  int32_t* tokens;
  int32_t* frames;
  int32_t* lens;
  float* scores;
  int32_t* status;
};

__global__ void __launch_bounds__(64) rbeam_result_kernel(ResultArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  const View s = view((void*)a.state, a.stream, a.hdr, b, a.beam);
  const bool ok = s.hdr[3] == (a.beam | (a.ms << 8));
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
  a.scores[o] = s.score[i];
  const int per = a.ms * a.beam;   // nodes of one live frame
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

template <int DT>
static bool launch_walk(const WalkArgs& a, bool fast, hipStream_t st) {
  if (fast) {
    // static + dynamic LDS exceed the 64 KB a kernel gets without asking
    static const bool ok =
        hipFuncSetAttribute((const void*)rbeam_walk_kernel<DT, true>,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            kRows * kThreads * (int)sizeof(float)) == hipSuccess;
    if (!ok) return false;
    hipLaunchKernelGGL((rbeam_walk_kernel<DT, true>), dim3(a.B), dim3(kThreads),
                       (size_t)kRows * a.V * sizeof(float), st, a);
  } else {
    hipLaunchKernelGGL((rbeam_walk_kernel<DT, false>), dim3(a.B), dim3(kThreads), 0, st, a);
  }
  return true;
}

}  // namespace rbeam
}  // namespace sc

using namespace sc;
using namespace sc::rbeam;

#define RBEAM_REQUIRE_SHAPE(fn, beam, ms)                                                        \
  SC_REQUIRE((beam) >= 1 && (beam) <= kBeamMax, fn ": beam=%d outside [1, %d]", (beam), kBeamMax); \
  SC_REQUIRE((ms) >= 1 && (ms) <= kSymMax, fn ": max_symbols=%d outside [1, %d]", (ms), kSymMax)

extern "C" size_t sc_rnnt_beam_state_bytes(int B, int beam, int max_symbols, int max_frames) {
  if (B < 0 || beam < 1 || beam > kBeamMax || max_symbols < 1 || max_symbols > kSymMax ||
      max_frames < 0)
    return 0;
  if ((size_t)max_frames * (size_t)beam * (size_t)max_symbols >= (size_t)0x7ffffff0) return 0;
  return (size_t)B * stream_bytes(beam, max_symbols, max_frames);
}

extern "C" size_t sc_rnnt_beam_workspace_bytes(int B, int V) {
  if (B < 0 || V < 1) return 0;
  return (size_t)B * kRows * (size_t)V * sizeof(float);
}

extern "C" int sc_rnnt_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_symbols,
                                  int max_frames, const float* streams, void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "sc_rnnt_beam_reset: bad shape B=%d", B);
  RBEAM_REQUIRE_SHAPE("sc_rnnt_beam_reset", beam, max_symbols);
  SC_REQUIRE(max_frames >= 0, "sc_rnnt_beam_reset: max_frames=%d is negative", max_frames);
  if (B == 0) return 0;
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_rnnt_beam_reset: state is a null pointer or not 8-byte aligned");
  const size_t want = sc_rnnt_beam_state_bytes(B, beam, max_symbols, max_frames);
  SC_REQUIRE(want != 0 && state_bytes == want,
             "sc_rnnt_beam_reset: state_bytes=%zu is not sc_rnnt_beam_state_bytes(B=%d, beam=%d, "
             "max_symbols=%d, max_frames=%d)=%zu", state_bytes, B, beam, max_symbols, max_frames,
             want);
  ResetArgs a{state, stream_bytes(beam, max_symbols, max_frames), hdr_bytes(beam), B, beam,
              max_symbols, streams};
  hipLaunchKernelGGL(rbeam_reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("sc_rnnt_beam_reset");
}

extern "C" int sc_rnnt_beam_frames(const void* enc_p, const void* pred_tab, const void* W, int dtype,
                                   const float* bias, int B, int T, int V, int J, int64_t stride_b,
                                   int64_t stride_t, const int64_t* lengths, const float* mask,
                                   int64_t mask_b, int64_t mask_t, int blank, int beam, int top_k,
                                   int max_symbols, void* state, size_t state_bytes,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16 || dtype == SC_F16,
             "sc_rnnt_beam_frames: unsupported dtype %d", dtype);
  SC_REQUIRE(B >= 0 && T >= 0 && V > 0, "sc_rnnt_beam_frames: bad shape B=%d T=%d V=%d", B, T, V);
  SC_REQUIRE(J >= 1 && J <= kMaxJ, "sc_rnnt_beam_frames: J=%d outside [1, %d]", J, kMaxJ);
  RBEAM_REQUIRE_SHAPE("sc_rnnt_beam_frames", beam, max_symbols);
  SC_REQUIRE(top_k >= 1 && top_k <= kTopkMax, "sc_rnnt_beam_frames: top_k=%d outside [1, %d]",
             top_k, kTopkMax);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_rnnt_beam_frames: blank=%d outside [0, V=%d)", blank, V);
  if (B == 0 || T == 0) return 0;
  SC_REQUIRE(enc_p && pred_tab && W && bias,
             "sc_rnnt_beam_frames: enc_p, pred_tab, W or bias is a null pointer");
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_rnnt_beam_frames: state is a null pointer or not 8-byte aligned");
  SC_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0,
             "sc_rnnt_beam_frames: workspace is a null pointer or not 4-byte aligned");
  const Layout L = layout(state_bytes, B, beam, max_symbols);
  SC_REQUIRE(L.max_frames >= 0,
             "sc_rnnt_beam_frames: state_bytes=%zu is no sc_rnnt_beam_state_bytes(B=%d, beam=%d, "
             "max_symbols=%d, .)", state_bytes, B, beam, max_symbols);
  const size_t need = sc_rnnt_beam_workspace_bytes(B, V);
  SC_REQUIRE(workspace_bytes >= need, "sc_rnnt_beam_frames: workspace_bytes=%zu below the %zu of "
             "sc_rnnt_beam_workspace_bytes(B=%d, V=%d)", workspace_bytes, need, B, V);
  const int K = top_k < V - 1 ? top_k : V - 1;   // clipped to the non-blank tokens there are
  WalkArgs a{enc_p, pred_tab, W, bias, B, T, V, J, stride_b, stride_t, lengths, mask, mask_b,
             mask_t, blank, beam, K, max_symbols, state, L.stream, L.hdr, (int)L.max_frames,
             (float*)workspace};
  // the register-resident path reads rows of W by 16-byte pieces
  const bool fast = J == 64 && V <= kThreads && ((uintptr_t)W & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  bool ok;
  switch (dtype) {
    case SC_F32: ok = launch_walk<SC_F32>(a, fast, st); break;
    case SC_BF16: ok = launch_walk<SC_BF16>(a, fast, st); break;
    default: ok = launch_walk<SC_F16>(a, fast, st); break;
  }
  SC_REQUIRE(ok, "sc_rnnt_beam_frames: the device refused the kernel's LDS size");
  return launch_status("sc_rnnt_beam_frames");
}

extern "C" int sc_rnnt_beam_result(const void* state, size_t state_bytes, int B, int beam,
                                   int max_symbols, int nbest, int32_t* tokens, int32_t* frames,
                                   int cap, int32_t* lens, float* scores, int32_t* status,
                                   void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "sc_rnnt_beam_result: bad shape B=%d", B);
  RBEAM_REQUIRE_SHAPE("sc_rnnt_beam_result", beam, max_symbols);
  SC_REQUIRE(nbest >= 1 && nbest <= beam, "sc_rnnt_beam_result: nbest=%d outside [1, beam=%d]",
             nbest, beam);
  SC_REQUIRE(cap >= 0, "sc_rnnt_beam_result: cap=%d is negative", cap);
  if (B == 0) return 0;
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_rnnt_beam_result: state is a null pointer or not 8-byte aligned");
  SC_REQUIRE(lens && scores, "sc_rnnt_beam_result: lens or scores is a null pointer");
  SC_REQUIRE(cap == 0 || tokens, "sc_rnnt_beam_result: tokens is a null pointer with cap=%d", cap);
  const Layout L = layout(state_bytes, B, beam, max_symbols);
  SC_REQUIRE(L.max_frames >= 0,
             "sc_rnnt_beam_result: state_bytes=%zu is no sc_rnnt_beam_state_bytes(B=%d, beam=%d, "
             "max_symbols=%d, .)", state_bytes, B, beam, max_symbols);
  ResultArgs a{state, L.stream, L.hdr, B, beam, max_symbols, nbest, cap, (int)L.max_frames, tokens,
               frames, lens, scores, status};
  hipLaunchKernelGGL(rbeam_result_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("sc_rnnt_beam_result");
}
