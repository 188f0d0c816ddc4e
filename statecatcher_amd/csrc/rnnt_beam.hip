// Transducer (RNN-T) beam search on device for the stateless predictor of RNNTPredictorJoiner,
// offline and chunked (include/statecatcher.h, sc_rnnt_beam_*).
//
// sc_rnnt_greedy_decode follows one path and returns no score.  This is the time-synchronous beam
// search over the same joint: a hypothesis is a token prefix and one score, the predictor being a
// [V, J] table of the last token.  All arithmetic is fp32; inputs are widened on load; z = tanh(..)
// has the greedy kernel's form; lp = logit - logsumexp(logit).  The state, its reset and result
// kernels, the rankings' order, the top_k rounds and the list-and-rank step are beam_common.h's,
// shared with ctc_beam.hip.
//
// The kernel of this file:
//   rbeam_walk_kernel    one persistent workgroup of 1024 threads per stream consumes the call's
//                        frames.  Per live frame, for r = 0 .. max_symbols, with C the round's
//                        hypotheses (the beam when r = 0):
//                          z of every hypothesis of C -> LDS | barrier |
//                          in passes of 16 hypotheses: every lane forms its row's logit for each
//                          (FAST: the row of W in registers) -> image [16][V] | barrier | wave w:
//                          max, sum of exponentials, lp[blank] and the top_k rounds of hypothesis
//                          w of the pass | barrier |
//                          wave 0: blank steps into A (merge by (hash, length), else append in
//                          order) and a floor under the beam-th largest extension | barrier |
//                          list and rank the extensions: the first `beam` ranks are the next C
//                          and get trie nodes.
//                        Then A is listed and ranked: its `beam` largest are the new beam.  Every
//                        branch is workgroup-uniform; every loop is bounded by T, max_symbols,
//                        beam, top_k, V or J; nothing waits on another workgroup; nothing is
//                        allocated or counted atomically in memory.  The opaque() copy of tid at
//                        the head of each phase (list_and_rank takes its own) keeps the fast path
//                        under 128 VGPRs: leave them where they are.
//     <DT, true>   J = 64, V <= 1024, W 16-byte aligned: lane v keeps row v of W in registers,
//                  the image lives in LDS (64 KB dynamic) and a wave's row statistics keep each
//                  lane's 16 elements of the row in registers through the top_k rounds
//     <DT, false>  any V, J <= 256: rows of W are read from memory and the image lives in the
//                  workspace (correct, not tuned)
//
// The candidate kept at rank k of round r of live frame f is trie node
// 1 + (f * max_symbols + r) * beam + k, so nothing is counted in memory and a token's frame is
// read off its node.
#include "beam_common.h"

namespace sc {
namespace rbeam {

constexpr int kAMax = kBeamMax * (kSymMax + 1);   // entries of one frame's A
constexpr int kThreads = 1024, kMaxJ = 256;
constexpr int kRows = 16;                         // hypotheses of one pass: one per wave
constexpr int kNS = 1;                            // score floats of a state entry

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
  const BeamView s = beam_view<kNS>(a.state, a.stream, a.hdr, b, Bm);
  if (s.hdr[3] != beam_tag(Bm, MS)) {   // not a state of this shape: touch nothing else
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
          float lse;
          const auto kmax = [](float& k, int& v) { wave_argmax<key_beats>(k, v); };
          const auto emit = [&](int j, int bi) {
            if (lane == 0) {
              tk_idx[i][j] = bi;
              tk_lp[i][j] = row[bi] - lse;
            }
          };
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
            lse = mx + logf(sm);
            if (lane == 0) lpb[i] = row[a.blank] - lse;
            if (expand) {
#pragma unroll
              for (int q = 0; q < 16; ++q) rv[q] = rank_key(rv[q] - lse);
              topk_rounds_regs(K, V, a.blank, lane, rv, kmax, emit);
            }
          } else {
            float mx = kNegInf;
            for (int v = lane; v < V; v += 64) mx = fmaxf(mx, row[v]);   // (a NaN never enters mx)
            mx = wave_max_dpp(mx);
            float sm = 0.0f;
            for (int v = lane; v < V; v += 64) sm += expf(row[v] - mx);
            sm = wave_sum_dpp(sm);
            lse = mx + logf(sm);
            if (lane == 0) lpb[i] = row[a.blank] - lse;
            if (expand)
              topk_rounds_row(K, V, a.blank, lane, [&](int v) { return rank_key(row[v] - lse); },
                              kmax, emit);
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
        // top_k >= 5)
        if (nc > kRankAll) {
          float v = kNegInf;
          if (lane < 2 * n) v = q.score[lane >> 1] + tk_lp[lane >> 1][lane & 1];
          beam_floor(v, lane, Bm, &theta);
        }
      }
      __syncthreads();
      if (!expand) break;
      // the extensions, candidate c = 32 i + j: one thread each, in the contract's order; the
      // first `beam` are the next round
      list_and_rank<4>(
          tid, kThreads, kBeamMax * kTopkMax, theta, Bm, keys, &n_keys, &n_cnt[cur ^ 1],
          [&](int c) {
            const int i = c >> 5, j = c & 31;
            return (i < n && j < K) ? q.score[i] + tk_lp[i][j] : kNegInf;
          },
          [&](int c, int rank) {
            const int i = c >> 5, j = c & 31;
            const int tok = tk_idx[i][j], node = 1 + (f * MS + r) * Bm + rank;
            nx.hash[rank] = hash_push(q.hash[i], tok);
            nx.score[rank] = q.score[i] + tk_lp[i][j];
            nx.node[rank] = node;
            nx.len[rank] = q.len[i] + 1;
            nx.last[rank] = tok;
            s.trie[2 * (size_t)node] = q.node[i];
            s.trie[2 * (size_t)node + 1] = tok;
          });
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
      list_and_rank<4>(
          tid, kThreads, uniform(n_a), kNegInf, Bm, keys, &n_keys, &n_cnt[cur ^ 1],
          [&](int c) { return A.score[c]; },
          [&](int c, int rank) {
            nx.hash[rank] = A.hash[c];
            nx.score[rank] = A.score[c];
            nx.node[rank] = A.node[c];
            nx.len[rank] = A.len[c];
            nx.last[rank] = A.last[c];
          });
      cur ^= 1;
      n = uniform(n_cnt[cur]);
    }
    ++f;
  }
  __syncthreads();
  const int ti = opaque(tid);   // fresh addresses: the ones of the load above are not kept alive
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

extern "C" size_t sc_rnnt_beam_state_bytes(int B, int beam, int max_symbols, int max_frames) {
  return beam_state_bytes(kNS, B, beam, max_symbols, max_frames);
}

extern "C" size_t sc_rnnt_beam_workspace_bytes(int B, int V) {
  if (B < 0 || V < 1) return 0;
  return (size_t)B * kRows * (size_t)V * sizeof(float);
}

extern "C" int sc_rnnt_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_symbols,
                                  int max_frames, const float* streams, void* stream) {
  return beam_reset<kNS>("sc_rnnt_beam_reset", state, state_bytes, B, beam, max_symbols, max_frames,
                         streams, stream);
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
  if (beam_check_shape("sc_rnnt_beam_frames", kNS, beam, max_symbols)) return SC_EINVAL;
  SC_REQUIRE(top_k >= 1 && top_k <= kTopkMax, "sc_rnnt_beam_frames: top_k=%d outside [1, %d]",
             top_k, kTopkMax);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_rnnt_beam_frames: blank=%d outside [0, V=%d)", blank, V);
  if (B == 0 || T == 0) return 0;
  SC_REQUIRE(enc_p && pred_tab && W && bias,
             "sc_rnnt_beam_frames: enc_p, pred_tab, W or bias is a null pointer");
  if (beam_check_state_ptr("sc_rnnt_beam_frames", state)) return SC_EINVAL;
  SC_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0,
             "sc_rnnt_beam_frames: workspace is a null pointer or not 4-byte aligned");
  BeamLayout L;
  if (beam_check_layout("sc_rnnt_beam_frames", kNS, state_bytes, B, beam, max_symbols, &L))
    return SC_EINVAL;
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
  return beam_result<kNS>("sc_rnnt_beam_result", state, state_bytes, B, beam, max_symbols, nbest,
                          tokens, frames, cap, lens, scores, status, stream);
}
