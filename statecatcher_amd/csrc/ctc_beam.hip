// CTC prefix beam search on device, offline and chunked (include/statecatcher.h, sc_ctc_beam_*).
//
// The reference's decoder.py is CTC greedy only (its README lists the beam search decoder as
// planned).  Greedy takes the best frame-wise path; prefix beam search sums every alignment of a
// hypothesis and returns an n-best list with scores.  All arithmetic is fp32; inputs are widened
// on load.  lae(a, b) = max(a, b) + log1p(exp(-|a - b|)), lae(-inf, b) = b.
//
// Three kernels:
//   beam_rows_kernel    frame-parallel pre-pass, one wave per live (b, t) row: the row goes to LDS
//                       once (16-byte pieces when aligned, as decode.hip's wave_argmax), then its
//                       log-sum-exp (is_logits), lp[blank] and the top_k non-blank (index, lp)
//                       pairs in rank order go to the workspace.  Rows longer than kRowLds
//                       elements do not fit the LDS row and are re-read from memory at every
//                       ranking round instead (correct, not tuned).
//   beam_walk_kernel    one workgroup per stream walks the frames in order.  The beam (two
//                       buffers) and the frame's <= beam * (top_k + 1) candidates live in LDS.
//                       Per live frame: extensions (and their merge into an existing entry) |
//                       barrier | stays | barrier | wave 0: a floor under the beam-th largest
//                       total | barrier | candidates at or above the floor go to a list |
//                       barrier | rank each by counting the listed ones that beat it, the first
//                       `beam` ranks write the new beam | barrier.  Every loop is bounded by T, beam and top_k; nothing waits on
//                       another workgroup; nothing is allocated or counted atomically in memory.
//   beam_result_kernel  one lane per (stream, hypothesis): walks the parent pointers and writes
//                       the tokens forwards from the stored length.
//
// Token history is a parent-pointer trie in the state: node 0 is the empty prefix, the extension
// kept at rank r of live frame f is node 1 + f * beam + r = (parent node, token).  Prefix identity
// (step 4 of the contract: "l + c is already a beam entry") is decided by (64-bit rolling hash of
// the tokens, length), not by comparing token sequences.
//
// NaN: a candidate whose total is NaN is dropped like one whose total is -inf, and the pre-pass
// ranks a NaN lp as -inf, so both rankings are strict total orders and every index stays in range.
#include "sc_common.h"

namespace sc {

constexpr int kBeamMax = 32, kTopkMax = 32;
constexpr int kCandMax = kBeamMax * (kTopkMax + 1);   // 1056 candidates of one frame
constexpr int kRowLds = 16384;                        // elements of one LDS row (64 KB as fp32)
constexpr int kNoTok = -1;
constexpr float kNegInf = -__builtin_huge_valf();

// ------------------------------------------------------------------ state layout -------------
// per stream, 8-byte aligned:
//   int32  hdr[4]       live frames consumed, status, hypotheses alive, beam
//   uint64 hash[beam]
//   float  pb[beam], pnb[beam];  int32 node[beam], len[beam], last[beam]
//   int32  trie[1 + max_frames * beam][2]   (parent, token)
struct BeamLayout {
  size_t hdr, stream;   // bytes before the trie, bytes of one stream
  int64_t max_frames;
};
static size_t beam_hdr_bytes(int beam) { return ((size_t)16 + 28 * (size_t)beam + 7) & ~(size_t)7; }
static size_t beam_stream_bytes(int beam, int64_t max_frames) {
  return beam_hdr_bytes(beam) + 8 * (1 + (size_t)max_frames * beam);
}
// the layout of a state of state_bytes bytes for B streams; max_frames < 0 when it is none
static BeamLayout beam_layout(size_t state_bytes, int B, int beam) {
  BeamLayout L{beam_hdr_bytes(beam), 0, -1};
  if (B <= 0 || state_bytes % (size_t)B) return L;
  L.stream = state_bytes / (size_t)B;
  if (L.stream < L.hdr + 8 || (L.stream - L.hdr - 8) % (8 * (size_t)beam)) return L;
  const size_t mf = (L.stream - L.hdr - 8) / (8 * (size_t)beam);
  if (mf * (size_t)beam < (size_t)0x7ffffff0) L.max_frames = (int64_t)mf;
  return L;
}

struct BeamView {   // one stream's arrays
  int32_t* hdr;
  uint64_t* hash;
  float *pb, *pnb;
  int32_t *node, *len, *last, *trie;
};
__device__ __forceinline__ BeamView beam_view(void* state, size_t stream_bytes, size_t hdr_bytes,
                                              int b, int beam) {
  char* p = (char*)state + (size_t)b * stream_bytes;
  BeamView v;
  v.hdr = (int32_t*)p;
  v.hash = (uint64_t*)(p + 16);
  v.pb = (float*)(p + 16 + 8 * (size_t)beam);
  v.pnb = v.pb + beam;
  v.node = (int32_t*)(v.pnb + beam);
  v.len = v.node + beam;
  v.last = v.len + beam;
  v.trie = (int32_t*)(p + hdr_bytes);
  return v;
}

__device__ __forceinline__ float lae(float a, float b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  return fmaxf(a, b) + log1pf(expf(-fabsf(a - b)));
}
__device__ __forceinline__ uint64_t hash_push(uint64_t h, int c) {
  h = (h ^ (uint64_t)(uint32_t)(c + 1)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 32);
}

// ------------------------------------------------------------------ reset --------------------
struct BeamResetArgs {
  void* state;
  size_t stream_bytes, hdr_bytes;
  int B, beam;
  const float* streams;
};

__global__ void __launch_bounds__(64) beam_reset_kernel(BeamResetArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (a.streams && a.streams[b] == 0.0f) return;
  const BeamView s = beam_view(a.state, a.stream_bytes, a.hdr_bytes, b, a.beam);
  if (i < a.beam) {   // entry 0: the empty prefix; the rest: dead
    s.hash[i] = 0;
    s.pb[i] = i == 0 ? 0.0f : kNegInf;
    s.pnb[i] = kNegInf;
    s.node[i] = 0;
    s.len[i] = 0;
    s.last[i] = kNoTok;
  }
  if (i == 0) {
    s.hdr[0] = 0;
    s.hdr[1] = 0;
    s.hdr[2] = 1;
    s.hdr[3] = a.beam;
    s.trie[0] = -1;
    s.trie[1] = kNoTok;
  }
}

// ------------------------------------------------------------------ frame pre-pass -----------
// workspace record of row (b, t), 2 + 2 top_k words: lp[blank], 0, index[top_k], lp[top_k]
struct BeamRowsArgs {
  const void* x;
  int is_logits, B, T, V;
  int64_t sb, st;
  const int64_t* lengths;
  const float* mask;
  int64_t mb, mt;
  int blank, top_k, waves;
  float* ws;
};

// (value, index) order of the rankings: larger value first, NaN as -inf, ties to the lower index
__device__ __forceinline__ float rank_key(float v) { return v != v ? kNegInf : v; }
__device__ __forceinline__ bool key_beats(float ka, int ia, float kb, int ib) {
  return (ka > kb) | ((ka == kb) & (ia < ib));
}

template <int DT, bool LDS>
__global__ void __launch_bounds__(256) beam_rows_kernel(BeamRowsArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  extern __shared__ __attribute__((aligned(16))) float rows_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * a.waves + wv;
  if (r >= (int64_t)a.B * a.T) return;   // whole waves leave; no barrier below
  const int b = (int)(r / a.T), t = (int)(r % a.T);
  if (a.lengths && t >= a.lengths[b]) return;
  if (a.mask && a.mask[(int64_t)b * a.mb + (int64_t)t * a.mt] == 0.0f) return;
  const T* p = (const T*)a.x + (int64_t)b * a.sb + (int64_t)t * a.st;
  float* row = rows_lds + (size_t)wv * (LDS ? a.V : 0);
  const int V = a.V;

  // the row -> LDS (this wave's own slice: no barrier), its maximum on the way
  float mx = kNegInf;
  if constexpr (LDS) {
    constexpr int N = Vec16<DT>::N;
    if (V % N == 0 && ((uintptr_t)p & 15) == 0) {
      for (int c = lane; c < V / N; c += 64) {
        float f[N];
        Vec16<DT>::ld(p + (size_t)N * c, f);
#pragma unroll
        for (int k = 0; k < N; ++k) {
          row[N * c + k] = f[k];
          mx = fmaxf(mx, f[k]);
        }
      }
    } else {
      for (int v = lane; v < V; v += 64) {
        const float f = E::ld(p[v]);
        row[v] = f;
        mx = fmaxf(mx, f);
      }
    }
  } else {
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, E::ld(p[v]));
  }
  __builtin_amdgcn_wave_barrier();
  auto val = [&](int v) -> float {
    if constexpr (LDS) return row[v];
    return E::ld(p[v]);
  };
  float lse = 0.0f;
  if (a.is_logits) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float s = 0.0f;
    for (int v = lane; v < V; v += 64) s += expf(val(v) - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    lse = mx + logf(s);
  }
  // lp replaces x in the LDS row; the ranking below reads lp, as the contract ranks lp
  if constexpr (LDS) {
    if (a.is_logits)
      for (int v = lane; v < V; v += 64) row[v] -= lse;
    __builtin_amdgcn_wave_barrier();
  }
  auto lpv = [&](int v) -> float {
    if constexpr (LDS) return row[v];
    return E::ld(p[v]) - lse;
  };
  const int RW = 2 + 2 * a.top_k;
  float* rec = a.ws + r * RW;
  if (lane == 0) {
    rec[0] = lpv(a.blank);
    rec[1] = 0.0f;
  }
  // top_k rounds: the best non-blank element strictly after the previous round's winner
  float pk = __builtin_huge_valf();
  int pi = -1;
  for (int j = 0; j < a.top_k; ++j) {
    float bk = kNegInf;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float k = rank_key(lpv(v));
      const bool after = key_beats(pk, pi, k, v);
      if (after & (v != a.blank) & key_beats(k, v, bk, bi)) {
        bk = k;
        bi = v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o);
      const int oi = __shfl_xor(bi, o);
      if (key_beats(ok, oi, bk, bi)) {
        bk = ok;
        bi = oi;
      }
    }
    // top_k <= V - 1 non-blank elements: a winner exists in every round
    bi = min(bi, V - 1);
    if (lane == 0) {
      ((int32_t*)rec)[2 + j] = bi;
      rec[2 + a.top_k + j] = lpv(bi);
    }
    pk = bk;
    pi = bi;
  }
}

// ------------------------------------------------------------------ beam walk ----------------
struct BeamWalkArgs {
  const float* ws;
  int B, T;
  const int64_t* lengths;
  const float* mask;
  int64_t mb, mt;
  int beam, top_k;
  void* state;
  size_t stream_bytes, hdr_bytes;
  int max_frames;
};

constexpr int kRankAll = 128;   // up to this many candidates are ranked without a floor

// a candidate as one sortable word: larger total first (NaN never gets here), then the lower index
__device__ __forceinline__ uint64_t cand_key(float tot, int c) {
  uint32_t u = __float_as_uint(tot + 0.0f);   // -0 -> +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)c);
}

struct BeamLds {   // one beam buffer
  uint64_t hash[kBeamMax];
  float pb[kBeamMax], pnb[kBeamMax];
  int node[kBeamMax], len[kBeamMax], last[kBeamMax];
};

__global__ void __launch_bounds__(1024) beam_walk_kernel(BeamWalkArgs a) {
  __shared__ BeamLds beams[2];
  __shared__ float c_pb[kCandMax], c_pnb[kCandMax], c_tot[kCandMax];
  __shared__ float rec[2 + 2 * kTopkMax];
  __shared__ float ext_term[kBeamMax], tot_s[kBeamMax];
  __shared__ int n_cnt[2];   // alive count of each beam buffer
  __shared__ uint64_t keys[kCandMax];
  __shared__ int n_keys;
  __shared__ float theta;
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int Bm = a.beam, K = a.top_k, RW = 2 + 2 * K;
  const BeamView s = beam_view(a.state, a.stream_bytes, a.hdr_bytes, b, Bm);
  if (s.hdr[3] != Bm) {   // not a state of this beam width: touch nothing else
    if (tid == 0) s.hdr[1] |= 2;
    return;
  }
  int f = uniform(s.hdr[0]), status = uniform(s.hdr[1]);
  int n = uniform(min(max(s.hdr[2], 0), Bm));
  int cur = 0;
  if (tid < Bm) {
    BeamLds& q = beams[0];
    q.hash[tid] = s.hash[tid];
    q.pb[tid] = s.pb[tid];
    q.pnb[tid] = s.pnb[tid];
    q.node[tid] = s.node[tid];
    q.len[tid] = s.len[tid];
    q.last[tid] = s.last[tid];
  }
  int len = a.T;
  if (a.lengths) len = (int)min<int64_t>(max<int64_t>(a.lengths[b], 0), a.T);
  const float* ws = a.ws + (int64_t)b * a.T * RW;
  // frame t + 1's record and mask are requested while frame t is resolved
  float r_next = 0.0f, m_next = 1.0f;
  auto fetch = [&](int t) {
    if (t >= len) return;
    if (tid < RW) r_next = ws[(int64_t)t * RW + tid];
    if (a.mask) m_next = a.mask[(int64_t)b * a.mb + (int64_t)t * a.mt];
  };
  fetch(0);
  __syncthreads();

  for (int t = 0; t < len; ++t) {
    const float r_cur = r_next;
    const bool live = m_next != 0.0f;
    fetch(t + 1);
    if (!live) continue;
    if (f >= a.max_frames) {   // the trie is full: this and every later live frame is ignored
      status |= 1;
      break;
    }
    if (tid < RW) rec[tid] = r_cur;
    if (tid < Bm) ext_term[tid] = kNegInf;
    if (tid < n) tot_s[tid] = lae(beams[cur].pb[tid], beams[cur].pnb[tid]);
    if (tid == 0) {
      n_cnt[cur ^ 1] = 0;
      n_keys = 0;
      theta = kNegInf;
    }
    __syncthreads();
    const BeamLds& q = beams[cur];
    BeamLds& w = beams[cur ^ 1];
    const int* r_idx = (const int*)rec + 2;
    const float* r_lp = rec + 2 + K;
    // extensions (i, j) -> candidate n + i K + j; one that spells an existing entry is folded
    // into that entry's stay candidate instead
    for (int e = tid; e < n * K; e += nthr) {
      const int i = e / K, j = e - i * K;
      const int c = r_idx[j];
      const float pnb = ((q.len[i] > 0 && c == q.last[i]) ? q.pb[i] : tot_s[i]) + r_lp[j];
      const uint64_t h = hash_push(q.hash[i], c);
      const int l1 = q.len[i] + 1;
      int hit = -1;
#pragma unroll 8
      for (int m = 0; m < n; ++m)
        if (q.len[m] == l1 && q.hash[m] == h) hit = m;
      if (hit >= 0) ext_term[hit] = pnb;
      c_pb[n + e] = kNegInf;
      c_pnb[n + e] = pnb;
      c_tot[n + e] = hit >= 0 ? kNegInf : pnb;
    }
    __syncthreads();
    if (tid < n) {   // stays
      const int i = tid;
      float rep = kNegInf;
      if (q.len[i] > 0)
#pragma unroll 8
        for (int j = 0; j < K; ++j)
          if (r_idx[j] == q.last[i]) rep = q.pnb[i] + r_lp[j];
      const float pb = tot_s[i] + rec[0];
      const float pnb = lae(rep, ext_term[i]);
      c_pb[i] = pb;
      c_pnb[i] = pnb;
      c_tot[i] = lae(pb, pnb);
    }
    __syncthreads();
    // A floor under the beam-th largest total, so that few candidates have to be ranked: the
    // beam-th largest among the stays and every entry's first extension (<= 64 values, wave 0).
    // A candidate below it has `beam` candidates above it and beats none that is not below it.
    const int nc = n + n * K;
    if (nc > kRankAll) {
      if (tid < 64) {
        float v = kNegInf;
        if (tid < n) v = c_tot[tid];
        else if (tid < 2 * n) v = c_tot[n + (tid - n) * K];
        v = v > kNegInf ? v : kNegInf;
        int above = 0;
#pragma unroll 8
        for (int o = 0; o < 64; ++o) {
          const float ov = __shfl(v, o);
          above += ((ov > v) | ((ov == v) & (o < tid))) ? 1 : 0;
        }
        if (above == Bm - 1) theta = v;
      }
      __syncthreads();
    }
    // the candidates at or above the floor (totals of -inf and NaN are dropped), as sortable
    // keys: total, then the earlier candidate
    const float floor_v = theta;
    for (int c = tid; c < nc; c += nthr) {
      const float tc = c_tot[c];
      if (!(tc > kNegInf) || tc < floor_v) continue;
      keys[atomicAdd(&n_keys, 1)] = cand_key(tc, c);
    }
    __syncthreads();
    // rank = number of candidates that beat this one (larger total; ties: the earlier one)
    const int nk = n_keys;
    for (int k = tid; k < nk; k += nthr) {
      const uint64_t kc = keys[k];
      const int c = (int)(0xffffffffu - (uint32_t)kc);
      int rank = 0;
#pragma unroll 8
      for (int o = 0; o < nk; ++o) rank += keys[o] > kc ? 1 : 0;
      if (rank >= Bm) continue;
      atomicMax(&n_cnt[cur ^ 1], rank + 1);
      w.pb[rank] = c_pb[c];
      w.pnb[rank] = c_pnb[c];
      if (c < n) {
        w.hash[rank] = q.hash[c];
        w.node[rank] = q.node[c];
        w.len[rank] = q.len[c];
        w.last[rank] = q.last[c];
      } else {
        const int e = c - n, i = e / K, j = e - i * K;
        const int tok = r_idx[j], node = 1 + f * Bm + rank;
        w.hash[rank] = hash_push(q.hash[i], tok);
        w.node[rank] = node;
        w.len[rank] = q.len[i] + 1;
        w.last[rank] = tok;
        s.trie[2 * (size_t)node] = q.node[i];
        s.trie[2 * (size_t)node + 1] = tok;
      }
    }
    __syncthreads();
    cur ^= 1;
    n = n_cnt[cur];
    ++f;
  }
  __syncthreads();
  if (tid < Bm) {   // entries past the alive ones leave in their reset form
    const BeamLds& q = beams[cur];
    const bool on = tid < n;
    s.hash[tid] = on ? q.hash[tid] : 0;
    s.pb[tid] = on ? q.pb[tid] : kNegInf;
    s.pnb[tid] = on ? q.pnb[tid] : kNegInf;
    s.node[tid] = on ? q.node[tid] : 0;
    s.len[tid] = on ? q.len[tid] : 0;
    s.last[tid] = on ? q.last[tid] : kNoTok;
  }
  if (tid == 0) {
    s.hdr[0] = f;
    s.hdr[1] = status;
    s.hdr[2] = n;
  }
}

// ------------------------------------------------------------------ result -------------------
struct BeamResultArgs {
  const void* state;
  size_t stream_bytes, hdr_bytes;
  int B, beam, nbest, cap, max_frames;
  int32_t* tokens;
  int32_t* lens;
  float* scores;
  int32_t* status;
};

__global__ void __launch_bounds__(64) beam_result_kernel(BeamResultArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  const BeamView s = beam_view((void*)a.state, a.stream_bytes, a.hdr_bytes, b, a.beam);
  const bool ok = s.hdr[3] == a.beam;
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
  a.scores[o] = lae(s.pb[i], s.pnb[i]);
  const int64_t nodes = 1 + (int64_t)a.max_frames * a.beam;
  int node = s.node[i];
  // backwards along the parent pointers, written forwards; a state that is not one (a node
  // outside the trie) ends the walk
  for (int pos = L - 1; pos >= 0 && node > 0 && node < nodes; --pos) {
    const int parent = s.trie[2 * (size_t)node], tok = s.trie[2 * (size_t)node + 1];
    if (pos < a.cap) a.tokens[o * a.cap + pos] = tok;
    if (parent >= node) break;   // parents precede their children
    node = parent;
  }
}

}  // namespace sc

using namespace sc;

#define BEAM_REQUIRE_WIDTH(fn, beam) \
  SC_REQUIRE((beam) >= 1 && (beam) <= kBeamMax, fn ": beam=%d outside [1, %d]", (beam), kBeamMax)

extern "C" size_t sc_ctc_beam_state_bytes(int B, int beam, int max_frames) {
  if (B < 0 || beam < 1 || beam > kBeamMax || max_frames < 0) return 0;
  if ((size_t)max_frames * (size_t)beam >= (size_t)0x7ffffff0) return 0;
  return (size_t)B * beam_stream_bytes(beam, max_frames);
}

extern "C" size_t sc_ctc_beam_workspace_bytes(int B, int T, int top_k) {
  if (B < 0 || T < 0 || top_k < 1 || top_k > kTopkMax) return 0;
  return (size_t)B * (size_t)T * (2 + 2 * (size_t)top_k) * sizeof(float);
}

extern "C" int sc_ctc_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_frames,
                                 const float* streams, void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "sc_ctc_beam_reset: bad shape B=%d", B);
  BEAM_REQUIRE_WIDTH("sc_ctc_beam_reset", beam);
  SC_REQUIRE(max_frames >= 0, "sc_ctc_beam_reset: max_frames=%d is negative", max_frames);
  if (B == 0) return 0;
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_ctc_beam_reset: state is a null pointer or not 8-byte aligned");
  const size_t want = sc_ctc_beam_state_bytes(B, beam, max_frames);
  SC_REQUIRE(want != 0 && state_bytes == want,
             "sc_ctc_beam_reset: state_bytes=%zu is not sc_ctc_beam_state_bytes(B=%d, beam=%d, "
             "max_frames=%d)=%zu", state_bytes, B, beam, max_frames, want);
  BeamResetArgs a{state, beam_stream_bytes(beam, max_frames), beam_hdr_bytes(beam), B, beam, streams};
  hipLaunchKernelGGL(beam_reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("sc_ctc_beam_reset");
}

template <int DT>
static void launch_rows(const BeamRowsArgs& a0, hipStream_t st) {
  BeamRowsArgs a = a0;
  const int64_t rows = (int64_t)a.B * a.T;
  if (a.V <= kRowLds) {   // as many rows per workgroup as fit 64 KB of LDS, at most 4
    a.waves = a.V <= kRowLds / 4 ? 4 : a.V <= kRowLds / 2 ? 2 : 1;
    hipLaunchKernelGGL((beam_rows_kernel<DT, true>), dim3((unsigned)((rows + a.waves - 1) / a.waves)),
                       dim3(64 * a.waves), (size_t)a.waves * a.V * sizeof(float), st, a);
  } else {
    a.waves = 4;
    hipLaunchKernelGGL((beam_rows_kernel<DT, false>), dim3((unsigned)((rows + 3) / 4)), dim3(256),
                       0, st, a);
  }
}

extern "C" int sc_ctc_beam_frames(const void* x, int dtype, int is_logits, int B, int T, int V,
                                  int64_t stride_b, int64_t stride_t, const int64_t* lengths,
                                  const float* mask, int64_t mask_b, int64_t mask_t, int blank,
                                  int beam, int top_k, void* state, size_t state_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16 || dtype == SC_F16,
             "sc_ctc_beam_frames: unsupported dtype %d", dtype);
  SC_REQUIRE(B >= 0 && T >= 0 && V >= 2, "sc_ctc_beam_frames: bad shape B=%d T=%d V=%d", B, T, V);
  SC_REQUIRE((int64_t)B * T <= 0x7fffffff, "sc_ctc_beam_frames: bad shape: B*T exceeds 2^31 - 1");
  BEAM_REQUIRE_WIDTH("sc_ctc_beam_frames", beam);
  SC_REQUIRE(top_k >= 1 && top_k <= kTopkMax && top_k <= V - 1,
             "sc_ctc_beam_frames: top_k=%d outside [1, min(%d, V - 1 = %d)]", top_k, kTopkMax, V - 1);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_ctc_beam_frames: blank=%d outside [0, V=%d)", blank, V);
  if (B == 0 || T == 0) return 0;
  SC_REQUIRE(x, "sc_ctc_beam_frames: x is a null pointer");
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_ctc_beam_frames: state is a null pointer or not 8-byte aligned");
  SC_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0,
             "sc_ctc_beam_frames: workspace is a null pointer or not 4-byte aligned");
  const BeamLayout L = beam_layout(state_bytes, B, beam);
  SC_REQUIRE(L.max_frames >= 0,
             "sc_ctc_beam_frames: state_bytes=%zu is no sc_ctc_beam_state_bytes(B=%d, beam=%d, .)",
             state_bytes, B, beam);
  const size_t need = sc_ctc_beam_workspace_bytes(B, T, top_k);
  SC_REQUIRE(workspace_bytes >= need, "sc_ctc_beam_frames: workspace_bytes=%zu below the %zu of "
             "sc_ctc_beam_workspace_bytes(B=%d, T=%d, top_k=%d)", workspace_bytes, need, B, T, top_k);
  hipStream_t st = (hipStream_t)stream;
  BeamRowsArgs r{x, is_logits ? 1 : 0, B, T, V, stride_b, stride_t, lengths, mask, mask_b, mask_t,
                 blank, top_k, 4, (float*)workspace};
  switch (dtype) {
    case SC_F32: launch_rows<SC_F32>(r, st); break;
    case SC_BF16: launch_rows<SC_BF16>(r, st); break;
    default: launch_rows<SC_F16>(r, st); break;
  }
  BeamWalkArgs w{(const float*)workspace, B, T, lengths, mask, mask_b, mask_t, beam, top_k, state,
                 L.stream, L.hdr, (int)L.max_frames};
  // one thread per candidate where they fit, and at least one per record word
  int nthr = (beam * (top_k + 1) + 63) / 64 * 64;
  nthr = nthr < 128 ? 128 : nthr > 1024 ? 1024 : nthr;
  hipLaunchKernelGGL(beam_walk_kernel, dim3(B), dim3(nthr), 0, st, w);
  return launch_status("sc_ctc_beam_frames");
}

extern "C" int sc_ctc_beam_result(const void* state, size_t state_bytes, int B, int beam, int nbest,
                                  int32_t* tokens, int cap, int32_t* lens, float* scores,
                                  int32_t* status, void* stream) {
  clear_error();
  SC_REQUIRE(B >= 0, "sc_ctc_beam_result: bad shape B=%d", B);
  BEAM_REQUIRE_WIDTH("sc_ctc_beam_result", beam);
  SC_REQUIRE(nbest >= 1 && nbest <= beam, "sc_ctc_beam_result: nbest=%d outside [1, beam=%d]",
             nbest, beam);
  SC_REQUIRE(cap >= 0, "sc_ctc_beam_result: cap=%d is negative", cap);
  if (B == 0) return 0;
  SC_REQUIRE(state && ((uintptr_t)state & 7) == 0,
             "sc_ctc_beam_result: state is a null pointer or not 8-byte aligned");
  SC_REQUIRE(lens && scores, "sc_ctc_beam_result: lens or scores is a null pointer");
  SC_REQUIRE(cap == 0 || tokens, "sc_ctc_beam_result: tokens is a null pointer with cap=%d", cap);
  const BeamLayout L = beam_layout(state_bytes, B, beam);
  SC_REQUIRE(L.max_frames >= 0,
             "sc_ctc_beam_result: state_bytes=%zu is no sc_ctc_beam_state_bytes(B=%d, beam=%d, .)",
             state_bytes, B, beam);
  BeamResultArgs a{state, L.stream, L.hdr, B, beam, nbest, cap, (int)L.max_frames, tokens, lens,
                   scores, status};
  hipLaunchKernelGGL(beam_result_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  return launch_status("sc_ctc_beam_result");
}
