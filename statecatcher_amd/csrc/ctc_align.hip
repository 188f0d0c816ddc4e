// CTC forced alignment on device (include/statecatcher.h, sc_ctc_align): the Viterbi path of a
// transcript through the CTC lattice, its per-frame and per-token log-probabilities and its score.
//
// The reference trains on podcast audio cut along subtitle cues and lists "on-the-fly
// hallucination detection & filtering" as planned; the score of the best alignment, per frame and
// per token, is the usual tool for it.  ctc.hip sums over every alignment (alpha / beta with a
// log-sum-exp); this file takes the best one (one direction, a max) and walks it back.
//
// Kernels (all on the caller's stream, no atomics, every reduction in a fixed order):
//   align_emit_kernel    frame-parallel pre-pass, one wave per live (b, t) row: the row is read
//                        once (an online max / sum in pieces of 8 elements, so any V and the same
//                        bits for every element type; 16-byte loads where a piece is aligned), its
//                        natural-log normaliser goes to lse[b][t] (0 for log-prob input), and the
//                        compact emission row em[b][t][0] = lp[blank], em[b][t][1 + u] = lp[label u]
//                        is written SHIFTED by c_t = the largest of them (kept in cst[b][t]).
//                        Every path takes one emission per frame, so the shift moves every path
//                        by sum_t c_t: the path does not depend on it and the lattice's fp32
//                        values stay near 0.
//   align_walk_kernel    one workgroup per sequence.  Each lane holds a PAIR of blank-extended
//                        states, p -> (blank 2p, label 2p + 1), as ctc_ab_kernel does; wave w
//                        computes 64 consecutive pairs, 64 - K owned plus a K-pair halo of its left
//                        neighbour's, so K frames need DPP wave_shr:1 only, then the owned pairs
//                        are published to LDS, one barrier, and the halo lanes re-read theirs.
//                        Every kAlNorm frames the values are re-centred on the workgroup maximum
//                        (the sum of maxima is carried in fp64).  Emission rows are prefetched 16
//                        frames ahead.  A decision is 2 bits (0 stay, 1 step, 2 skip); a pair's 4
//                        bits of 8 frames make one 32-bit word, stored dec[b][t / 8][p].
//                        The score and the path's last state (end[b]) leave with the last frame.
//   align_backtrace_kernel  one workgroup per sequence: blocks of kAlBt frames of decision rows
//                        are staged in LDS with coalesced loads (the next block's in flight
//                        meanwhile), one lane walks the block inside LDS, and the block's lanes
//                        write `states`.  A launch of its own, so a kernel trace shows its share.
//   align_finish_kernel  one workgroup per sequence: frame_lp[t] = x[label] - lse (the pre-pass's
//                        own expression, unshifted), span starts / ends from the neighbouring
//                        states, then one lane per token sums its span in frame order.
//
// "Dead" lattice values are the finite sentinel -1e30 (branch-free max; nothing becomes NaN), and
// emissions are clamped to it: a sequence whose best final value is dead is infeasible.  A NaN
// emission is clamped dead by fmaxf.  The backtrace clamps the state at 0, so whatever the
// decisions hold, every index stays in range.
#include "sc_common.h"

namespace sc {
namespace al {

constexpr float kDead = -1e30f;
constexpr int kAlNorm = 16;    // frames between re-centrings (and the emission prefetch depth)
constexpr int kAlBt = 64;      // frames per backtrace staging block (8 decision rows)
constexpr int kAlUmax = 1007;  // 16 waves x 63 owned pairs - 1, as sc_ctc_fwd
constexpr int kAlPairs = 1008;

struct AlignArgs {
  const void* x;
  int is_logits, B, T, V, Umax, blank;
  int W;     // emission row width: Umax + 1
  int NT8;   // decision rows: ceil(T / 8)
  int64_t sb, stt;
  const int64_t* tg;
  int64_t tgs;
  const int64_t* in_lens;
  const int64_t* tgt_lens;
  float* em;       // [B][T][W]    shifted emissions: blank, then label u
  float* lse;      // [B][T]       natural-log row normaliser (0 for log-prob input)
  float* cst;      // [B][T]       the row's shift c_t
  uint32_t* dec;   // [B][NT8][W]  packed decisions
  int32_t* end;    // [B]          the path's last state; -1: no valid alignment
  int32_t* states;
  float* frame_lp;
  int32_t* spans;
  float* token_lp;
  float* score;
};

__device__ __forceinline__ int clampi(int64_t v, int lo, int hi) {
  return (int)(v < lo ? lo : (v > hi ? hi : v));
}
// the emission column of a label: clamped into [0, V) so no load leaves the row (sc_ctc_fwd's rule)
__device__ __forceinline__ int label_col(int64_t lab, int V) {
  return lab < 0 ? 0 : (lab >= V ? V - 1 : (int)lab);
}

// ------------------------------------------------------------------ frame pre-pass -----------
template <int DT>
__global__ void __launch_bounds__(256) align_emit_kernel(AlignArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)a.B * a.T) return;   // whole waves leave; no workgroup barrier below
  const int b = (int)(row / a.T), t = (int)(row % a.T);
  if (t >= clampi(a.in_lens[b], 0, a.T)) return;
  const T* p = (const T*)a.x + (int64_t)b * a.sb + (int64_t)t * a.stt;
  const int Ub = clampi(a.tgt_lens[b], 0, a.Umax);
  const int64_t* tg = a.tg + (int64_t)b * a.tgs;
  float lse = 0.0f;
  if (a.is_logits) {
    // Online max / sum over pieces of kPiece consecutive elements, piece c to lane c % 64, whatever
    // the element type and the row's alignment: a 16-bit row and its widened fp32 copy are summed
    // in the same order, so they give the same lse bit for bit.  A whole piece of an aligned row
    // comes in 16-byte loads (one for 16-bit, two for fp32); the last, partial piece and the
    // pieces of an unaligned row come element by element, padded with -inf (exp = 0 exactly).
    constexpr int kPiece = 8, N = Vec16<DT>::N;
    constexpr float kNInf = -__builtin_huge_valf();
    float m = kNInf, l = 0.0f;
    const bool vec = ((uintptr_t)p & 15) == 0;
    for (int c = lane; c * kPiece < a.V; c += 64) {
      const int v0 = c * kPiece, n = min(kPiece, a.V - v0);
      float xv[kPiece];
      if (vec && n == kPiece) {
        if constexpr (N == kPiece) {
          Vec16<DT>::ld(p + v0, xv);
        } else {
          float lo[N], hi[N];
          Vec16<DT>::ld(p + v0, lo);
          Vec16<DT>::ld(p + v0 + N, hi);
#pragma unroll
          for (int k = 0; k < N; ++k) {
            xv[k] = lo[k];
            xv[N + k] = hi[k];
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < kPiece; ++k) xv[k] = k < n ? E::ld(p[v0 + k]) : kNInf;
      }
      float cm = xv[0];
#pragma unroll
      for (int k = 1; k < kPiece; ++k) cm = fmaxf(cm, xv[k]);
      const float mn = fmaxf(m, cm);
      if (mn == kNInf) continue;   // nothing but -inf (masked tokens) so far: exp(-inf + inf) is NaN
      float cs = 0.0f;
#pragma unroll
      for (int k = 0; k < kPiece; ++k) cs += expf(xv[k] - mn);
      l = l * expf(m - mn) + cs;
      m = mn;
    }
    const float M = wave_max_dpp(m);
    l = wave_sum_dpp(m == -__builtin_huge_valf() ? 0.0f : l * expf(m - M));
    lse = M + logf(l);
  }
  float* out = a.em + row * a.W;
  const float lb = E::ld(p[a.blank]) - lse;
  float c = fmaxf(lb, kDead);
  for (int u = lane; u < Ub; u += 64) c = fmaxf(c, E::ld(p[label_col(tg[u], a.V)]) - lse);
  c = wave_max_dpp(c);
  if (!(c > 0.1f * kDead)) c = 0.0f;   // every state dead: no shift
  for (int u = lane; u < Ub; u += 64)
    out[1 + u] = fmaxf(E::ld(p[label_col(tg[u], a.V)]) - lse - c, kDead);
  if (lane == 0) {
    out[0] = fmaxf(lb - c, kDead);
    a.lse[row] = lse;
    a.cst[row] = c;
  }
}

// ------------------------------------------------------------------ forward walk -------------
// wave_shr:1 with bound_ctrl: lane 0 reads 0.  Lane 0 is always a halo lane (K >= 1), whose
// values are never published and are replaced at each exchange.
__device__ __forceinline__ float shr1z(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf, 0xf, true));
}

template <int K>
__global__ void __launch_bounds__(1024) align_walk_kernel(AlignArgs a) {
  constexpr int OW = 64 - K;   // owned pairs per wave
  constexpr int P = kAlNorm;   // frames per prefetch buffer: a multiple of K and of 8
  static_assert(P % K == 0 && P % 8 == 0 && kAlBt % 8 == 0, "block sizes");
  __shared__ float2 full2[2][kAlPairs];            // published pairs, double-buffered
  __shared__ float wmax[2][16];
  __shared__ double csum[16];
  __shared__ float fin[2];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, w = uniform(tid >> 6), nw = blockDim.x >> 6, nthr = blockDim.x;
  const int Tb = clampi(a.in_lens[b], 0, a.T);
  const int Ub = clampi(a.tgt_lens[b], 0, a.Umax);
  if (Tb == 0) {
    if (tid == 0) {
      a.score[b] = Ub == 0 ? 0.0f : -__builtin_huge_valf();
      a.end[b] = -1;
    }
    return;
  }
  const int p = w * OW + lane - K;
  const bool own = lane >= K;
  const bool liveB = p >= 0 && p <= Ub;   // state 2p
  const bool liveL = p >= 0 && p < Ub;    // state 2p + 1
  const int64_t* tg = a.tg + (int64_t)b * a.tgs;
  bool skip = false;   // 2p - 1 -> 2p + 1 allowed (sc_ctc_fwd's rule, on the labels as given)
  if (liveL && p >= 1) {
    const int lab = (int)tg[p];
    skip = lab != a.blank && lab != (int)tg[p - 1];
  }
  if (tid == 0) fin[0] = fin[1] = kDead;

  const float* emb = a.em + (int64_t)b * a.T * a.W;
  const int lidx = min(max(1 + p, 0), a.W - 1);   // clamped for addressing only
  float bufA_l[P], bufA_b[P], bufB_l[P], bufB_b[P];
  auto load = [&](float (&bl)[P], float (&bb)[P], int i0) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float* r = emb + (int64_t)min(i0 + j, Tb - 1) * a.W;
      bl[j] = r[lidx];
      bb[j] = r[0];
    }
  };
  uint32_t* decb = a.dec + (int64_t)b * a.NT8 * a.W;
  const bool dec_w = own && p < a.W;   // (own lanes have p >= 0)
  float vB = kDead, vL = kDead;
  double off = 0.0;
  uint32_t acc = 0;
  int exch = 0;
  auto body = [&](const float (&bl)[P], const float (&bb)[P], int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = i0 + j;
      if (i >= Tb) break;   // Tb is uniform over the workgroup: the barriers below stay matched
      const float eb = bb[j], el = bl[j];
      if (i == 0) {
        vB = (liveB && p == 0) ? eb : kDead;
        vL = (liveL && p == 0) ? el : kDead;
      } else {
        const float lp = shr1z(vL);
        // ties go to the smaller move: stay, then step by 1, then skip
        const bool dB = lp > vB;
        const float nB = (dB ? lp : vB) + eb;
        float best = vL;
        uint32_t dL = 0;
        if (vB > best) {
          best = vB;
          dL = 1;
        }
        if (skip && lp > best) {
          best = lp;
          dL = 2;
        }
        const float nL = best + el;
        vB = liveB ? nB : kDead;
        vL = liveL ? nL : kDead;
        acc |= ((dB ? 1u : 0u) | (dL << 2)) << (4 * (j & 7));
      }
      if ((j & 7) == 7 || i == Tb - 1) {
        if (dec_w) decb[(int64_t)(i >> 3) * a.W + p] = acc;
        acc = 0;
      }
      if (j % K == K - 1) {   // halo exchange; at the buffer's last frame also the re-centring
        const int par = exch & 1;
        const bool norm = j == P - 1;
        if (own) full2[par][p] = make_float2(vB, vL);
        if (norm) {
          const float m = wave_max_dpp(own ? fmaxf(vB, vL) : kDead);
          if (lane == 0) wmax[par][w] = m;
        }
        lds_barrier();
        if (!own) {
          const float2 q = p >= 0 ? full2[par][p] : make_float2(kDead, kDead);
          vB = q.x;
          vL = q.y;
        }
        if (norm) {
          float m = kDead;
          for (int q = 0; q < nw; ++q) m = fmaxf(m, wmax[par][q]);
          if (m > 0.5f * kDead) {   // all dead (infeasible so far): keep the sentinel
            vB -= m;
            vL -= m;
            off += (double)m;
          }
        }
        ++exch;
      }
    }
  };
  load(bufA_l, bufA_b, 0);
  for (int i0 = 0; i0 < Tb; i0 += 2 * P) {
    load(bufB_l, bufB_b, i0 + P);
    body(bufA_l, bufA_b, i0);
    if (i0 + P >= Tb) break;
    load(bufA_l, bufA_b, i0 + 2 * P);
    body(bufB_l, bufB_b, i0 + P);
  }

  // sum_t c_t in fp64 and a fixed order; the two candidate final states
  double cs = 0.0;
  for (int t = tid; t < Tb; t += nthr) cs += (double)a.cst[(int64_t)b * a.T + t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o);
  __syncthreads();   // fin's initialisation, and every wave is past its last exchange
  if (lane == 0) csum[w] = cs;
  if (own && p == Ub) fin[0] = vB;
  if (own && p == Ub - 1) fin[1] = vL;
  __syncthreads();
  if (tid == 0) {
    const float f0 = fin[0], f1 = fin[1];
    const bool label_end = Ub > 0 && f1 > f0;   // a tie goes to state 2U
    const float best = label_end ? f1 : f0;
    const bool feasible = best > 0.5f * kDead;
    double ctot = 0.0;
    for (int q = 0; q < nw; ++q) ctot += csum[q];
    a.score[b] = feasible ? (float)((double)best + off + ctot) : -__builtin_huge_valf();
    a.end[b] = feasible ? (label_end ? 2 * Ub - 1 : 2 * Ub) : -1;
  }
}

// ------------------------------------------------------------------ backtrace ----------------
// One workgroup per sequence follows the recorded moves back from end[b], a block of kAlBt frames
// (8 decision rows, contiguous in memory) at a time: the block goes to LDS with coalesced loads,
// lane 0 walks it inside LDS (a chain of dependent global loads would cost ~1 us each), then the
// block's lanes write `states`.  The next block's rows are requested into registers before the
// walk, so their latency hides behind it.
constexpr int kBtThreads = 1024;
constexpr int kBtRegs = (kAlBt / 8) * kAlPairs / kBtThreads + 1;   // words per thread and block

__global__ void __launch_bounds__(kBtThreads) align_backtrace_kernel(AlignArgs a) {
  __shared__ uint32_t dst[(kAlBt / 8) * kAlPairs];
  __shared__ int path[kAlBt];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = clampi(a.in_lens[b], 0, a.T);
  const int Ub = clampi(a.tgt_lens[b], 0, a.Umax);
  int32_t* states = a.states + (int64_t)b * a.T;
  int s = Tb > 0 ? a.end[b] : -1;
  const int live = s >= 0 ? Tb : 0;   // an infeasible sequence has no path
  for (int t = live + tid; t < a.T; t += kBtThreads) states[t] = -1;
  if (live == 0) return;
  s = min(s, 2 * Ub);
  const uint32_t* decb = a.dec + (int64_t)b * a.NT8 * a.W;
  uint32_t r[kBtRegs];
  auto words = [&](int blk) {   // whole rows of block blk
    const int t0 = blk * kAlBt, t1 = min(t0 + kAlBt, Tb);
    return (((t1 - 1) >> 3) - (t0 >> 3) + 1) * a.W;
  };
  auto fetch = [&](int blk) {
    const int n = words(blk);
    const uint32_t* src = decb + (int64_t)(blk * (kAlBt / 8)) * a.W;
#pragma unroll
    for (int k = 0; k < kBtRegs; ++k) {
      const int i = tid + k * kBtThreads;
      if (i < n) r[k] = src[i];
    }
  };
  int blk = (Tb - 1) / kAlBt;
  fetch(blk);
  for (; blk >= 0; --blk) {
    const int t0 = blk * kAlBt, t1 = min(t0 + kAlBt, Tb), n = words(blk);
#pragma unroll
    for (int k = 0; k < kBtRegs; ++k) {
      const int i = tid + k * kBtThreads;
      if (i < n) dst[i] = r[k];
    }
    __syncthreads();
    if (blk > 0) fetch(blk - 1);
    if (tid == 0) {
      for (int t = t1 - 1; t >= t0; --t) {
        path[t - t0] = s;
        if (t > 0) {
          const uint32_t word = dst[((t - t0) >> 3) * a.W + (s >> 1)];
          const int d = (int)((word >> (4 * (t & 7) + 2 * (s & 1))) & 3u);
          s = max(s - d, 0);
        }
      }
    }
    __syncthreads();
    if (tid < t1 - t0) states[t0 + tid] = path[tid];
  }
}

// ------------------------------------------------------------------ per-frame / per-token ----
template <int DT>
__global__ void __launch_bounds__(256) align_finish_kernel(AlignArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = clampi(a.in_lens[b], 0, a.T);
  const int Ub = clampi(a.tgt_lens[b], 0, a.Umax);
  const int32_t* st = a.states + (int64_t)b * a.T;
  const int64_t* tg = a.tg + (int64_t)b * a.tgs;
  int32_t* spans = a.spans + (int64_t)b * a.Umax * 2;
  float* token_lp = a.token_lp + (int64_t)b * a.Umax;
  float* frame_lp = a.frame_lp + (int64_t)b * a.T;
  const bool feasible = Tb > 0 && st[0] >= 0;
  for (int u = tid; u < a.Umax; u += 256) {
    spans[2 * u] = spans[2 * u + 1] = -1;
    token_lp[u] = 0.0f;
  }
  __threadfence();
  __syncthreads();
  for (int t = tid; t < a.T; t += 256) {
    const int s = (feasible && t < Tb) ? min(st[t], 2 * Ub) : -1;
    float f = 0.0f;
    if (s >= 0) {
      const int col = (s & 1) ? label_col(tg[s >> 1], a.V) : a.blank;
      const T* p = (const T*)a.x + (int64_t)b * a.sb + (int64_t)t * a.stt;
      f = E::ld(p[col]) - a.lse[(int64_t)b * a.T + t];
      if (s & 1) {
        if (t == 0 || st[t - 1] != s) spans[2 * (s >> 1)] = t;
        if (t == Tb - 1 || st[t + 1] != s) spans[2 * (s >> 1) + 1] = t + 1;
      }
    }
    frame_lp[t] = f;
  }
  __threadfence();
  __syncthreads();
  for (int u = tid; u < (feasible ? Ub : 0); u += 256) {
    const int t0 = spans[2 * u], t1 = spans[2 * u + 1];
    if (t0 < 0 || t1 <= t0 || t1 > Tb) continue;   // (a path a NaN bent: no span)
    float sum = 0.0f;
    for (int t = t0; t < t1; ++t) sum += frame_lp[t];
    token_lp[u] = sum / (float)(t1 - t0);
  }
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t ws_layout(int B, int T, int Umax, AlignArgs* a, void* base) {
  const size_t W = (size_t)Umax + 1, NT8 = ((size_t)T + 7) / 8, BT = (size_t)B * T;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p + off;
    off += align256(bytes);
    return (void*)r;
  };
  float* em = (float*)take(BT * W * 4);
  float* lse = (float*)take(BT * 4);
  float* cst = (float*)take(BT * 4);
  uint32_t* dec = (uint32_t*)take((size_t)B * NT8 * W * 4);
  int32_t* end = (int32_t*)take((size_t)B * 4);
  if (a) {
    a->end = end;
    a->em = em;
    a->lse = lse;
    a->cst = cst;
    a->dec = dec;
  }
  return off > 256 ? off : 256;
}

}  // namespace al
}  // namespace sc

using namespace sc;
using namespace sc::al;

extern "C" size_t sc_ctc_align_workspace_bytes(int B, int T, int max_target_len) {
  if (B < 0 || T < 0 || max_target_len < 0 || max_target_len > kAlUmax) return 0;
  return ws_layout(B, T, max_target_len, nullptr, nullptr);
}

extern "C" int sc_ctc_align(const void* x, int x_dtype, int is_logits, int B, int T, int V,
                            int64_t stride_b, int64_t stride_t, const int64_t* targets,
                            int64_t target_stride, int max_target_len, const int64_t* in_lens,
                            const int64_t* tgt_lens, int blank, int32_t* states, float* frame_lp,
                            int32_t* spans, float* token_lp, float* score, void* workspace,
                            size_t workspace_bytes, void* stream) {
  clear_error();
  SC_REQUIRE(x_dtype == SC_F32 || x_dtype == SC_BF16 || x_dtype == SC_F16,
             "sc_ctc_align: unsupported dtype %d", x_dtype);
  SC_REQUIRE(B >= 0 && T >= 0 && V > 0 && max_target_len >= 0,
             "sc_ctc_align: bad shape B=%d T=%d V=%d max_target_len=%d", B, T, V, max_target_len);
  SC_REQUIRE(max_target_len <= kAlUmax, "sc_ctc_align: max target length %d exceeds %d",
             max_target_len, kAlUmax);
  SC_REQUIRE(blank >= 0 && blank < V, "sc_ctc_align: blank %d outside [0, %d)", blank, V);
  SC_REQUIRE((int64_t)B * T <= 0x7fffffff, "sc_ctc_align: B*T exceeds 2^31 - 1");
  if (B == 0) return 0;
  SC_REQUIRE(in_lens && tgt_lens && score, "sc_ctc_align: null pointer (in_lens, tgt_lens, score)");
  SC_REQUIRE(T == 0 || (x && states && frame_lp),
             "sc_ctc_align: null pointer (x, states, frame_lp)");
  SC_REQUIRE(max_target_len == 0 || (targets && spans && token_lp),
             "sc_ctc_align: null pointer (targets, spans, token_lp)");
  SC_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0,
             "sc_ctc_align: workspace is a null pointer or not 16-byte aligned");
  const size_t need = sc_ctc_align_workspace_bytes(B, T, max_target_len);
  SC_REQUIRE(workspace_bytes >= need, "sc_ctc_align: workspace_bytes=%zu below the %zu of "
             "sc_ctc_align_workspace_bytes(B=%d, T=%d, max_target_len=%d)", workspace_bytes, need,
             B, T, max_target_len);
  AlignArgs a;
  a.x = x;
  a.is_logits = is_logits ? 1 : 0;
  a.B = B;
  a.T = T;
  a.V = V;
  a.Umax = max_target_len;
  a.blank = blank;
  a.W = max_target_len + 1;
  a.NT8 = (T + 7) / 8;
  a.sb = stride_b;
  a.stt = stride_t;
  a.tg = targets;
  a.tgs = target_stride;
  a.in_lens = in_lens;
  a.tgt_lens = tgt_lens;
  a.states = states;
  a.frame_lp = frame_lp;
  a.spans = spans;
  a.token_lp = token_lp;
  a.score = score;
  ws_layout(B, T, max_target_len, &a, workspace);
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * T;
  const dim3 eg((unsigned)((rows + 3) / 4));
  // the widest halo whose waves fit a 1024-thread group: 16 frames between barriers up to 767
  // labels, else one
  const int K = (a.W + 47) / 48 <= 16 ? 16 : 1;
  const int nw = (a.W + (64 - K) - 1) / (64 - K);
  switch (x_dtype) {
    case SC_F32:
      if (rows) hipLaunchKernelGGL((align_emit_kernel<SC_F32>), eg, dim3(256), 0, st, a);
      break;
    case SC_BF16:
      if (rows) hipLaunchKernelGGL((align_emit_kernel<SC_BF16>), eg, dim3(256), 0, st, a);
      break;
    default:
      if (rows) hipLaunchKernelGGL((align_emit_kernel<SC_F16>), eg, dim3(256), 0, st, a);
      break;
  }
  if (K == 16) hipLaunchKernelGGL((align_walk_kernel<16>), dim3(B), dim3(64 * nw), 0, st, a);
  else hipLaunchKernelGGL((align_walk_kernel<1>), dim3(B), dim3(64 * nw), 0, st, a);
  hipLaunchKernelGGL(align_backtrace_kernel, dim3(B), dim3(kBtThreads), 0, st, a);
  switch (x_dtype) {
    case SC_F32: hipLaunchKernelGGL((align_finish_kernel<SC_F32>), dim3(B), dim3(256), 0, st, a); break;
    case SC_BF16: hipLaunchKernelGGL((align_finish_kernel<SC_BF16>), dim3(B), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((align_finish_kernel<SC_F16>), dim3(B), dim3(256), 0, st, a); break;
  }
  return launch_status("sc_ctc_align");
}
