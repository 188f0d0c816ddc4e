// The RWKV-4 WKV operator (forward and adjoint), gfx950.
//
// Per batch row and channel, with W = -exp(time_decay), u = time_first and the state S = (A, B):
//     y_t     = (A_t + e^{u+k_t} v_t) / (B_t + e^{u+k_t})
//     S_{t+1} = e^W S_t + e^{k_t} (v_t, 1)
// S is held as (num, den, max) with A = num e^max, B = den e^max, and every step renormalises to
// the running maximum (as transformers' rwkv_linear_attention_cpu does), so no exponential
// overflows.  The empty state is num = den = 0, max = -1e38.
//
// Same decomposition as decay_scan.hip: workgroup = (b, 64 channels) x NW waves splitting each
// 64-step super-chunk in time.  A segment of n steps is the affine map S -> e^{nW} S + L with L
// the segment's aggregate from the empty state, itself a stabilised triple; every wave publishes
// its L in LDS, one LDS-only barrier, then composes the maps of the earlier waves with the state
// carried from the previous super-chunk and walks its own steps.  Next super-chunk's inputs are
// in flight during the compute.  The forward writes the carried state at every super-chunk start
// when asked (the checkpoints); nothing else is saved.
//
// Adjoint (g = dL/dy, D_t = B_t + e^{u+k_t}, dN_t = g_t / D_t, dD_t = -g_t y_t / D_t):
//     GS_t = (dN_t, dD_t) + e^W GS_{t+1},  GS_T = 0
//     dv_t = e^{u+k_t} dN_t + e^{k_t} GA_{t+1}
//     dk_t = e^{u+k_t} (v_t dN_t + dD_t) + e^{k_t} (v_t GA_{t+1} + GB_{t+1})
//     d time_first = sum e^{u+k_t} (v_t dN_t + dD_t)      (= sum e^{u+k_t} g_t (v_t B_t - A_t) / D_t^2)
//     d time_decay = W sum e^W <GS_{t+1}, S_t>
// GS scales like e^{-max}: it is held as (ga, gb, q) with GS = (ga, gb) e^q and
// q_t = max(-mo_t, W + q_{t+1}), mo_t = max(max_t, u + k_t) the forward's output maximum, which is
// the forward's recurrence again with key -mo_t and values (g / dd, -g y / dd).  The exponents
// that appear are bounded: k_t + q_{t+1} <= 0 and W + q_{t+1} + max_t <= 0 up to the den of a
// caller's state.  The backward walks the super-chunks in reverse: per super-chunk it recomputes
// the forward from the checkpoint, then runs the reverse scan with the same map composition.
// The parameter gradients are summed in a fixed order (per thread over its steps, the waves in
// order, then the rows in order): two runs are bitwise equal.
//
// Bytes per (b, t, c): fwd 2e in + e out; bwd 3e in + 2e out; checkpoints 12 bytes per 64 steps.

#include "sc_common.h"

namespace sc {

constexpr int kWkvChunk = 64;
constexpr float kWkvEmpty = -1e38f;

struct WkvArgs {
  const float* td;
  const float* tf;
  const void* k;
  const void* v;
  const void* dy;       // bwd only
  void* y;              // fwd
  void* dk;             // bwd
  void* dv;             // bwd
  const float *n0, *d0, *m0;   // incoming state [B,C] each, or all null (empty)
  float *n1, *d1, *m1;         // outgoing state (fwd)
  float* ckpt;          // [B, nsc, 3, C]: fwd writes it when non-null, bwd reads it
  float* part;          // bwd: per-row partials [B, 2, C] (time_decay sum, time_first sum)
  int B, T, C, nsc;
};

struct Wkv3 {
  float n, d, m;
};

// S <- e^W S + e^key (val, 1) (forward), GS <- e^W GS + e^key (va, vb) (reverse)
__device__ __forceinline__ void wkv_push(Wkv3& s, float W, float key, float va, float vb) {
  const float ms = vmax(s.m + W, key);
  const float f1 = fexp(s.m + W - ms), f2 = fexp(key - ms);
  s.n = f1 * s.n + f2 * va;
  s.d = f1 * s.d + f2 * vb;
  s.m = ms;
}
// s <- e^{dW} s + l
__device__ __forceinline__ void wkv_compose(Wkv3& s, float dW, const Wkv3& l) {
  const float ms = vmax(s.m + dW, l.m);
  const float f1 = fexp(s.m + dW - ms), f2 = fexp(l.m - ms);
  s.n = f1 * s.n + f2 * l.n;
  s.d = f1 * s.d + f2 * l.d;
  s.m = ms;
}

template <int DT, int NW, int LC>
__global__ void __launch_bounds__(NW * 64) wkv_fwd_kernel(WkvArgs a) {
  static_assert(NW * LC == kWkvChunk, "super-chunk must be 64 steps");
  using E = Elem<DT>;
  using T = typename E::T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const bool cok = c < a.C;
  const int cc = cok ? c : a.C - 1;
  __shared__ float agg[NW][3][64];
  __shared__ float car[2][3][64];
  const float W = -expf(a.td[cc]), u = a.tf[cc];
  const int64_t row = (int64_t)b * a.T * a.C;
  const T* kp = (const T*)a.k + row + cc;
  const T* vp = (const T*)a.v + row + cc;
  T* yp = (T*)a.y + row + c;
  if (w == 0) {
    const int64_t i = (int64_t)b * a.C + cc;
    car[0][0][lane] = a.n0 ? a.n0[i] : 0.0f;
    car[0][1][lane] = a.n0 ? a.d0[i] : 0.0f;
    car[0][2][lane] = a.n0 ? a.m0[i] : kWkvEmpty;
  }
  T ck[LC], cv[LC], pk[LC], pv[LC];
  const int Tm1 = a.T - 1;
  auto load = [&](T (&kb)[LC], T (&vb)[LC], int sc) {
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      const int64_t t = min(sc * kWkvChunk + w * LC + j, Tm1);
      kb[j] = kp[t * a.C];
      vb[j] = vp[t * a.C];
    }
  };
  if (a.nsc > 0) load(ck, cv, 0);
  lds_barrier();
  for (int sc = 0; sc < a.nsc; ++sc) {
    if (sc + 1 < a.nsc) load(pk, pv, sc + 1);
    const int t0 = sc * kWkvChunk + w * LC;
    const int nv = min(max(a.T - t0, 0), LC);
    float kk[LC], vv[LC];
    Wkv3 l{0.0f, 0.0f, kWkvEmpty};
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      kk[j] = E::ld(ck[j]);
      vv[j] = E::ld(cv[j]);
      if (j < nv) wkv_push(l, W, kk[j], vv[j], 1.0f);
    }
    agg[w][0][lane] = l.n;
    agg[w][1][lane] = l.d;
    agg[w][2][lane] = l.m;
    lds_barrier();
    Wkv3 s{car[sc & 1][0][lane], car[sc & 1][1][lane], car[sc & 1][2][lane]};
    if (a.ckpt && w == 0 && cok) {
      float* cp = a.ckpt + ((int64_t)b * a.nsc + sc) * 3 * a.C + c;
      cp[0] = s.n;
      cp[a.C] = s.d;
      cp[2 * (int64_t)a.C] = s.m;
    }
    for (int q = 0; q < w; ++q) {
      const int nq = min(max(a.T - (sc * kWkvChunk + q * LC), 0), LC);
      if (nq > 0) wkv_compose(s, (float)nq * W, Wkv3{agg[q][0][lane], agg[q][1][lane], agg[q][2][lane]});
    }
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      if (j < nv) {
        const float uk = u + kk[j];
        const float mo = vmax(s.m, uk);
        const float e1 = fexp(s.m - mo), e2 = fexp(uk - mo);
        const float y = (e1 * s.n + e2 * vv[j]) / (e1 * s.d + e2);
        if (cok) yp[(int64_t)(t0 + j) * a.C] = E::st(y);
        wkv_push(s, W, kk[j], vv[j], 1.0f);
      }
    }
    if (w == NW - 1) {
      car[(sc + 1) & 1][0][lane] = s.n;
      car[(sc + 1) & 1][1][lane] = s.d;
      car[(sc + 1) & 1][2][lane] = s.m;
    }
    lds_barrier();   // agg reuse + carry visibility
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      ck[j] = pk[j];
      cv[j] = pv[j];
    }
  }
  if (w == 0 && cok) {
    const int64_t i = (int64_t)b * a.C + c;
    a.n1[i] = car[a.nsc & 1][0][lane];
    a.d1[i] = car[a.nsc & 1][1][lane];
    a.m1[i] = car[a.nsc & 1][2][lane];
  }
}

template <int DT, int NW, int LC>
__global__ void __launch_bounds__(NW * 64) wkv_bwd_kernel(WkvArgs a) {
  static_assert(NW * LC == kWkvChunk, "super-chunk must be 64 steps");
  using E = Elem<DT>;
  using T = typename E::T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const bool cok = c < a.C;
  const int cc = cok ? c : a.C - 1;
  __shared__ float aggf[NW][3][64];   // forward segment aggregates
  __shared__ float aggr[NW][3][64];   // reverse segment aggregates; the final wave sums
  __shared__ float car[2][3][64];     // GS carried from the later super-chunk
  const float W = -expf(a.td[cc]), u = a.tf[cc];
  const int64_t row = (int64_t)b * a.T * a.C;
  const T* kp = (const T*)a.k + row + cc;
  const T* vp = (const T*)a.v + row + cc;
  const T* gp = (const T*)a.dy + row + cc;
  T* dkp = (T*)a.dk + row + c;
  T* dvp = (T*)a.dv + row + c;
  if (w == 0) {
    car[0][0][lane] = 0.0f;
    car[0][1][lane] = 0.0f;
    car[0][2][lane] = kWkvEmpty;
  }
  T ck[LC], cv[LC], cg[LC], pk[LC], pv[LC], pg[LC];
  const int Tm1 = a.T - 1;
  auto load = [&](T (&kb)[LC], T (&vb)[LC], T (&gb)[LC], int sc) {
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      const int64_t t = min(sc * kWkvChunk + w * LC + j, Tm1);
      kb[j] = kp[t * a.C];
      vb[j] = vp[t * a.C];
      gb[j] = gp[t * a.C];
    }
  };
  if (a.nsc > 0) load(ck, cv, cg, a.nsc - 1);
  float acc_td = 0.0f, acc_tf = 0.0f;
  lds_barrier();
  for (int it = 0; it < a.nsc; ++it) {
    const int sc = a.nsc - 1 - it;
    if (sc > 0) load(pk, pv, pg, sc - 1);
    const float* cp = a.ckpt + ((int64_t)b * a.nsc + sc) * 3 * a.C + cc;
    Wkv3 s{cp[0], cp[a.C], cp[2 * (int64_t)a.C]};
    const int t0 = sc * kWkvChunk + w * LC;
    const int nv = min(max(a.T - t0, 0), LC);
    // ---- the forward again: segment aggregates, then this wave's states step by step
    float kk[LC], vv[LC];
    Wkv3 l{0.0f, 0.0f, kWkvEmpty};
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      kk[j] = E::ld(ck[j]);
      vv[j] = E::ld(cv[j]);
      if (j < nv) wkv_push(l, W, kk[j], vv[j], 1.0f);
    }
    aggf[w][0][lane] = l.n;
    aggf[w][1][lane] = l.d;
    aggf[w][2][lane] = l.m;
    lds_barrier();
    for (int q = 0; q < w; ++q) {
      const int nq = min(max(a.T - (sc * kWkvChunk + q * LC), 0), LC);
      if (nq > 0) wkv_compose(s, (float)nq * W, Wkv3{aggf[q][0][lane], aggf[q][1][lane], aggf[q][2][lane]});
    }
    // per step: the state before it, the output maximum, e^{u+k-mo}, g / dd, -g y / dd and
    // p1 = e^{u+k} (v dN + dD), taken as e^{u+k-mo} e1 (g / dd) (v den - num) / dd: v dN + dD is
    // (g / D)(v - y), which cancels where the bonus term dominates y
    float sn[LC], sd[LC], sm[LC], mo[LC], eu[LC], gn[LC], gd[LC], p1[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      sn[j] = s.n;
      sd[j] = s.d;
      sm[j] = s.m;
      const float uk = u + kk[j];
      mo[j] = vmax(s.m, uk);
      const float e1 = fexp(s.m - mo[j]);
      eu[j] = fexp(uk - mo[j]);
      const float r = 1.0f / (e1 * s.d + eu[j]);
      const float y = (e1 * s.n + eu[j] * vv[j]) * r;
      const float g = E::ld(cg[j]);
      gn[j] = g * r;
      gd[j] = -g * y * r;
      p1[j] = eu[j] * e1 * gn[j] * r * (vv[j] * s.d - s.n);
      if (j < nv) wkv_push(s, W, kk[j], vv[j], 1.0f);
    }
    // ---- the reverse scan: segment aggregates from the empty GS, composed from the later waves
    Wkv3 rl{0.0f, 0.0f, kWkvEmpty};
#pragma unroll
    for (int j = LC - 1; j >= 0; --j)
      if (j < nv) wkv_push(rl, W, -mo[j], gn[j], gd[j]);
    aggr[w][0][lane] = rl.n;
    aggr[w][1][lane] = rl.d;
    aggr[w][2][lane] = rl.m;
    lds_barrier();
    Wkv3 G{car[it & 1][0][lane], car[it & 1][1][lane], car[it & 1][2][lane]};
    for (int q = NW - 1; q > w; --q) {
      const int nq = min(max(a.T - (sc * kWkvChunk + q * LC), 0), LC);
      if (nq > 0) wkv_compose(G, (float)nq * W, Wkv3{aggr[q][0][lane], aggr[q][1][lane], aggr[q][2][lane]});
    }
#pragma unroll
    for (int j = LC - 1; j >= 0; --j) {
      if (j < nv) {   // G = GS_{t+1}
        const float ek = fexp(kk[j] + G.m);
        const float dv = eu[j] * gn[j] + ek * G.n;
        const float dk = p1[j] + ek * (vv[j] * G.n + G.d);
        acc_tf += p1[j];
        acc_td += fexp(W + G.m + sm[j]) * (G.n * sn[j] + G.d * sd[j]);
        if (cok) {
          dkp[(int64_t)(t0 + j) * a.C] = E::st(dk);
          dvp[(int64_t)(t0 + j) * a.C] = E::st(dv);
        }
        wkv_push(G, W, -mo[j], gn[j], gd[j]);
      }
    }
    if (w == 0) {
      car[(it + 1) & 1][0][lane] = G.n;
      car[(it + 1) & 1][1][lane] = G.d;
      car[(it + 1) & 1][2][lane] = G.m;
    }
    lds_barrier();   // aggregate reuse + carry visibility
#pragma unroll
    for (int j = 0; j < LC; ++j) {
      ck[j] = pk[j];
      cv[j] = pv[j];
      cg[j] = pg[j];
    }
  }
  // the waves' sums in wave order (every wave passed the loop's last barrier: aggr is free)
  aggr[w][0][lane] = acc_td;
  aggr[w][1][lane] = acc_tf;
  lds_barrier();
  if (w == 0 && cok) {
    float std_ = 0.0f, stf = 0.0f;
    for (int q = 0; q < NW; ++q) {
      std_ += aggr[q][0][lane];
      stf += aggr[q][1][lane];
    }
    a.part[((int64_t)b * 2 + 0) * a.C + c] = std_;
    a.part[((int64_t)b * 2 + 1) * a.C + c] = stf;
  }
}

// d time_decay[c] = W_c sum_b part[b,0,c], d time_first[c] = sum_b part[b,1,c], rows in order
__global__ void __launch_bounds__(64) wkv_param_kernel(const float* part, const float* td, float* dtd,
                                                       float* dtf, int B, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  float s0 = 0.0f, s1 = 0.0f;
  for (int b = 0; b < B; ++b) {
    s0 += part[((int64_t)b * 2 + 0) * C + c];
    s1 += part[((int64_t)b * 2 + 1) * C + c];
  }
  dtd[c] = -expf(td[c]) * s0;
  dtf[c] = s1;
}

template <int DT>
static void launch_wkv(const WkvArgs& a, bool bwd, hipStream_t st) {
  dim3 grid((a.C + 63) / 64, a.B);
  if (bwd)
    hipLaunchKernelGGL((wkv_bwd_kernel<DT, 8, 8>), grid, dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((wkv_fwd_kernel<DT, 8, 8>), grid, dim3(512), 0, st, a);
}

static bool wkv_shape_ok(int B, int T, int C) {
  return B >= 0 && T >= 0 && C >= 0 && B <= 65535 && (int64_t)T + kWkvChunk < INT32_MAX;
}

}  // namespace sc

using namespace sc;

extern "C" int sc_wkv_chunk(void) { return kWkvChunk; }

extern "C" int64_t sc_wkv_ckpt_numel(int B, int T, int C) {
  if (B < 0 || T < 0 || C < 0) return 0;
  return (int64_t)B * ((T + kWkvChunk - 1) / kWkvChunk) * 3 * C;
}

extern "C" int64_t sc_wkv_bwd_ws_numel(int B, int T, int C) {
  if (B < 0 || T < 0 || C < 0) return 0;
  return (int64_t)B * 2 * C;
}

extern "C" int sc_wkv_fwd(const float* time_decay, const float* time_first, const void* k,
                          const void* v, int dtype, const float* num_in, const float* den_in,
                          const float* max_in, void* y, float* num_out, float* den_out,
                          float* max_out, float* ckpt, int B, int T, int C, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16, "sc_wkv_fwd: unsupported dtype %d (fp32 or bf16)",
             dtype);
  SC_REQUIRE(wkv_shape_ok(B, T, C), "sc_wkv_fwd: bad shape B=%d T=%d C=%d", B, T, C);
  SC_REQUIRE((num_in != nullptr) == (den_in != nullptr) && (num_in != nullptr) == (max_in != nullptr),
             "sc_wkv_fwd: the incoming state is num, den and max together, or all null");
  if (B == 0 || C == 0) return 0;
  SC_REQUIRE(time_decay && time_first && num_out && den_out && max_out, "sc_wkv_fwd: null pointer");
  SC_REQUIRE(T == 0 || (k && v && y), "sc_wkv_fwd: null pointer");
  WkvArgs a{time_decay, time_first, k, v, nullptr, y, nullptr, nullptr, num_in, den_in, max_in,
            num_out, den_out, max_out, ckpt, nullptr, B, T, C, (T + kWkvChunk - 1) / kWkvChunk};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SC_F32) launch_wkv<SC_F32>(a, false, st);
  else launch_wkv<SC_BF16>(a, false, st);
  return launch_status("sc_wkv_fwd");
}

extern "C" int sc_wkv_bwd(const float* time_decay, const float* time_first, const void* k,
                          const void* v, const void* dy, int dtype, const float* ckpt, void* dk,
                          void* dv, float* d_time_decay, float* d_time_first, float* ws, int B, int T,
                          int C, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16, "sc_wkv_bwd: unsupported dtype %d (fp32 or bf16)",
             dtype);
  SC_REQUIRE(wkv_shape_ok(B, T, C), "sc_wkv_bwd: bad shape B=%d T=%d C=%d", B, T, C);
  if (C == 0) return 0;
  SC_REQUIRE(time_decay && d_time_decay && d_time_first, "sc_wkv_bwd: null pointer");
  SC_REQUIRE(B == 0 || (time_first && ws), "sc_wkv_bwd: null pointer");
  SC_REQUIRE(B == 0 || T == 0 || (k && v && dy && ckpt && dk && dv), "sc_wkv_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (B > 0) {
    WkvArgs a{time_decay, time_first, k, v, dy, nullptr, dk, dv, nullptr, nullptr, nullptr,
              nullptr, nullptr, nullptr, (float*)ckpt, ws, B, T, C, (T + kWkvChunk - 1) / kWkvChunk};
    if (dtype == SC_F32) launch_wkv<SC_F32>(a, true, st);
    else launch_wkv<SC_BF16>(a, true, st);
  }
  hipLaunchKernelGGL(wkv_param_kernel, dim3((C + 63) / 64), dim3(64), 0, st, ws, time_decay,
                     d_time_decay, d_time_first, B, C);
  return launch_status("sc_wkv_bwd");
}
