// CTC prefix beam search on device, offline and chunked (include/statecatcher.h, sc_ctc_beam_*).
//
// The reference's decoder.py is CTC greedy only (its README lists the beam search decoder as
// planned).  Greedy takes the best frame-wise path; prefix beam search sums every alignment of a
// hypothesis and returns an n-best list with scores.  All arithmetic is fp32; inputs are widened
// on load.  The state, its reset and result kernels, the rankings' order, the top_k rounds and
// the list-and-rank step are beam_common.h's, shared with rnnt_beam.hip.
//
// The two kernels of this file:
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
//                       total | barrier | list and rank: the first `beam` ranks write the new
//                       beam.  Every loop is bounded by T, beam and top_k; nothing waits on
//                       another workgroup; nothing is allocated or counted atomically in memory.
//
// The extension kept at rank r of live frame f is trie node 1 + f * beam + r.  Prefix identity
// (step 4 of the contract: "l + c is already a beam entry") is decided by (hash, length).
//
// NaN: a candidate whose total is NaN is dropped like one whose total is -inf, and the pre-pass
// ranks a NaN lp as -inf, so both rankings are strict total orders and every index stays in range.
#include "beam_common.h"

namespace sc {

constexpr int kCandMax = kBeamMax * (kTopkMax + 1);   // 1056 candidates of one frame
constexpr int kRowLds = 16384;                        // elements of one LDS row (64 KB as fp32)
constexpr int kNS = 2;                                // score floats of a state entry: pb, pnb

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
  topk_rounds_row(
      a.top_k, V, a.blank, lane, [&](int v) { return rank_key(lpv(v)); },
      [](float& bk, int& bi) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ok = __shfl_xor(bk, o);
          const int oi = __shfl_xor(bi, o);
          if (key_beats(ok, oi, bk, bi)) {
            bk = ok;
            bi = oi;
          }
        }
      },
      [&](int j, int bi) {
        if (lane == 0) {
          ((int32_t*)rec)[2 + j] = bi;
          rec[2 + a.top_k + j] = lpv(bi);
        }
      });
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
  const BeamView s = beam_view<kNS>(a.state, a.stream_bytes, a.hdr_bytes, b, Bm);
  if (s.hdr[3] != beam_tag(Bm, 0)) {   // not a state of this beam width: touch nothing else
    if (tid == 0) s.hdr[1] |= 2;
    return;
  }
  int f = uniform(s.hdr[0]), status = uniform(s.hdr[1]);
  int n = uniform(min(max(s.hdr[2], 0), Bm));
  int cur = 0;
  if (tid < Bm) {
    BeamLds& q = beams[0];
    q.hash[tid] = s.hash[tid];
    q.pb[tid] = s.score[tid];
    q.pnb[tid] = s.score[Bm + tid];
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
    const int nc = n + n * K;
    if (nc > kRankAll) {
      if (tid < 64) {
        float v = kNegInf;
        if (tid < n) v = c_tot[tid];
        else if (tid < 2 * n) v = c_tot[n + (tid - n) * K];
        beam_floor(v, tid, Bm, &theta);
      }
      __syncthreads();
    }
    list_and_rank<8>(
        tid, nthr, nc, theta, Bm, keys, &n_keys, &n_cnt[cur ^ 1], [&](int c) { return c_tot[c]; },
        [&](int c, int rank) {
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
        });
    cur ^= 1;
    n = n_cnt[cur];
    ++f;
  }
  __syncthreads();
  if (tid < Bm) {   // entries past the alive ones leave in their reset form
    const BeamLds& q = beams[cur];
    const bool on = tid < n;
    s.hash[tid] = on ? q.hash[tid] : 0;
    s.score[tid] = on ? q.pb[tid] : kNegInf;
    s.score[Bm + tid] = on ? q.pnb[tid] : kNegInf;
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

}  // namespace sc

using namespace sc;

extern "C" size_t sc_ctc_beam_state_bytes(int B, int beam, int max_frames) {
  return beam_state_bytes(kNS, B, beam, 0, max_frames);
}

extern "C" size_t sc_ctc_beam_workspace_bytes(int B, int T, int top_k) {
  if (B < 0 || T < 0 || top_k < 1 || top_k > kTopkMax) return 0;
  return (size_t)B * (size_t)T * (2 + 2 * (size_t)top_k) * sizeof(float);
}

extern "C" int sc_ctc_beam_reset(void* state, size_t state_bytes, int B, int beam, int max_frames,
                                 const float* streams, void* stream) {
  return beam_reset<kNS>("sc_ctc_beam_reset", state, state_bytes, B, beam, 0, max_frames, streams,
                         stream);
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
  if (beam_check_shape("sc_ctc_beam_frames", kNS, beam, 0)) return SC_EINVAL;
  SC_REQUIRE(top_k >= 1 && top_k <= kTopkMax && top_k <= V - 1,
             "sc_ctc_beam_frames: top_k=%d outside [1, min(%d, V - 1 = %d)]", top_k, kTopkMax, V - 1);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_ctc_beam_frames: blank=%d outside [0, V=%d)", blank, V);
  if (B == 0 || T == 0) return 0;
  SC_REQUIRE(x, "sc_ctc_beam_frames: x is a null pointer");
  if (beam_check_state_ptr("sc_ctc_beam_frames", state)) return SC_EINVAL;
  SC_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0,
             "sc_ctc_beam_frames: workspace is a null pointer or not 4-byte aligned");
  BeamLayout L;
  if (beam_check_layout("sc_ctc_beam_frames", kNS, state_bytes, B, beam, 0, &L)) return SC_EINVAL;
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
  return beam_result<kNS>("sc_ctc_beam_result", state, state_bytes, B, beam, 0, nbest, tokens,
                          nullptr, cap, lens, scores, status, stream);
}
