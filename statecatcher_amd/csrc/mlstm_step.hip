// mLSTM recurrent step (xLSTM matrix memory) for streaming / any-length inference: advances
// BH = batch x heads sequences by K >= 1 steps from a carried state, in fp32, state in place.
//   m_t = max(logsig(f_t) + m_{t-1}, i_t)
//   C_t = e^{logsig(f_t)+m_{t-1}-m_t} C_{t-1} + e^{i_t-m_t} k_t v_t^T      (n_t alike)
//   h_t = (q_t s C_t) / (max(|q_t s . n_t|, e^{-m_t}) + eps),  s = DQ^-1/2
// (oracle/mlstm.py; the stabilised state convention of sc_mlstm_fwd's c_last / states_n / states_m).
//
// Mapping: one workgroup of DV threads per sequence; thread j owns column j of C (DQ fp32
// registers) for the whole call, so C is read once and written once whatever K is.  q_t and k_t
// are loaded one element per lane (coalesced) and broadcast with v_readlane inside the unrolled
// row loop; n is held one element per lane (every wave keeps its own copy, computed identically)
// and q.n is a DPP wave sum.  No LDS; the one barrier separates the initial read of the shared
// n / m from their write-back.  A step's arithmetic does not depend on K or on its position in
// the call: K steps in one call equal K calls of one step bitwise.
#include <math.h>

#include "sc_common.h"

namespace sc {

namespace {

struct StepArgs {
  const void* q;
  const void* k;
  const void* v;
  const void* ig;      // fp32 [BH][K] (gproj == 0) or the io dtype inside the projection
  const void* fg;
  const float* live;   // [BH / NH][K] or NULL
  float* C;
  float* n;
  float* m;
  void* h;
  int BH, K, NH, gproj;
  int64_t qb, qh, qt, vb, vh, vt, gb, gh, gt;
  float cap, eps, scale;
};

__device__ __forceinline__ float soft_cap(float x, float cap) {
  return cap > 0.0f ? cap * tanhf(x / cap) : x;
}
// log sigmoid(x) = min(x, 0) - log1p(e^{-|x|})
__device__ __forceinline__ float logsig(float x) {
  return fminf(x, 0.0f) - log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float bcast(float x, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

template <int IO, int DQ, int DV>
__global__ void __launch_bounds__(DV) mlstm_step_kernel(StepArgs a) {
  using T = typename Elem<IO>::T;
  constexpr int R = (DQ + 63) / 64;   // q / k / n elements per lane
  const int bh = blockIdx.x, j = threadIdx.x, lane = threadIdx.x & 63;
  const int b = bh / a.NH, hh = bh % a.NH;
  const T* qp = (const T*)a.q + (int64_t)b * a.qb + (int64_t)hh * a.qh;
  const T* kp = (const T*)a.k + (int64_t)b * a.qb + (int64_t)hh * a.qh;
  const T* vp = (const T*)a.v + (int64_t)b * a.vb + (int64_t)hh * a.vh + j;
  const int64_t g0 = (int64_t)b * a.gb + (int64_t)hh * a.gh;
  const float* livep = a.live ? a.live + (int64_t)b * a.K : nullptr;
  float* Cp = a.C + (int64_t)bh * DQ * DV + j;
  float* np = a.n + (int64_t)bh * DQ;
  T* hp = (T*)a.h + (int64_t)bh * a.K * DV + j;

  float C[DQ], nl[R];
#pragma unroll
  for (int i = 0; i < DQ; ++i) C[i] = Cp[(int64_t)i * DV];
#pragma unroll
  for (int r = 0; r < R; ++r) nl[r] = lane + 64 * r < DQ ? np[lane + 64 * r] : 0.0f;
  float m = a.m[bh];
  __syncthreads();   // every wave has read n and m before wave 0 writes them back

  for (int t = 0; t < a.K; ++t) {
    if (livep && livep[t] == 0.0f) {   // held: state untouched, zero output row
      hp[(int64_t)t * DV] = Elem<IO>::st(0.0f);
      continue;
    }
    float ql[R], kl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = lane + 64 * r;
      ql[r] = i < DQ ? Elem<IO>::ld(qp[(int64_t)t * a.qt + i]) : 0.0f;
      kl[r] = i < DQ ? Elem<IO>::ld(kp[(int64_t)t * a.qt + i]) : 0.0f;
    }
    const float vj = Elem<IO>::ld(vp[(int64_t)t * a.vt]);
    float xi, xf;
    if (a.gproj) {
      xi = Elem<IO>::ld(((const T*)a.ig)[g0 + (int64_t)t * a.gt]);
      xf = Elem<IO>::ld(((const T*)a.fg)[g0 + (int64_t)t * a.gt]);
    } else {
      xi = ((const float*)a.ig)[(int64_t)bh * a.K + t];
      xf = ((const float*)a.fg)[(int64_t)bh * a.K + t];
    }
    xi = soft_cap(xi, a.cap);
    xf = soft_cap(xf, a.cap);
    const float am = logsig(xf) + m;
    const float mn = fmaxf(am, xi);
    const float fa = expf(am - mn), ia = expf(xi - mn);
    float qn = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      kl[r] *= ia;
      ql[r] *= a.scale;
      nl[r] = fa * nl[r] + kl[r];
      qn += ql[r] * nl[r];
    }
    qn = wave_sum_dpp(qn);
    float num = 0.0f;
#pragma unroll
    for (int i = 0; i < DQ; ++i) {
      const float ki = bcast(kl[i / 64], i % 64), qi = bcast(ql[i / 64], i % 64);
      C[i] = fa * C[i] + ki * vj;
      num += qi * C[i];
    }
    const float den = fmaxf(fabsf(qn), expf(-mn)) + a.eps;
    hp[(int64_t)t * DV] = Elem<IO>::st(num / den);
    m = mn;
  }

#pragma unroll
  for (int i = 0; i < DQ; ++i) Cp[(int64_t)i * DV] = C[i];
  if (j < 64) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (lane + 64 * r < DQ) np[lane + 64 * r] = nl[r];
    if (j == 0) a.m[bh] = m;
  }
}

// head dimensions compiled in (DQ, DV): those of sc_mlstm_fwd
#define SC_MLSTM_STEP_DIMS(X) X(32, 64) X(64, 64) X(64, 128) X(96, 192)

bool step_dims_supported(int DQ, int DV) {
#define SC_CASE(q, v) if (DQ == q && DV == v) return true;
  SC_MLSTM_STEP_DIMS(SC_CASE)
#undef SC_CASE
  return false;
}

template <int IO>
void step_dispatch(const StepArgs& a, int DQ, int DV, hipStream_t st) {
#define SC_CASE(q, v)                                                                        \
  if (DQ == q && DV == v)                                                                    \
    hipLaunchKernelGGL((mlstm_step_kernel<IO, q, v>), dim3(a.BH), dim3(v), 0, st, a);
  SC_MLSTM_STEP_DIMS(SC_CASE)
#undef SC_CASE
}

}  // namespace

}  // namespace sc

using namespace sc;

extern "C" int sc_mlstm_step_supported(int io_dtype, int DQ, int DV) {
  return (io_dtype == SC_F32 || io_dtype == SC_BF16) && step_dims_supported(DQ, DV);
}

extern "C" int sc_mlstm_step(const void* q, const void* k, const void* v, int io_dtype,
                             const void* igate, const void* fgate, const int64_t* gate_layout,
                             float cap, const float* live, float* C, float* n, float* m, int BH,
                             int K, int NH, int DQ, int DV, float eps, void* h,
                             const int64_t* layout, void* stream) {
  clear_error();
  SC_REQUIRE(io_dtype == SC_F32 || io_dtype == SC_BF16,
             "sc_mlstm_step: operand dtype %d (fp32 or bf16 only)", io_dtype);
  SC_REQUIRE(BH >= 0 && K >= 0, "sc_mlstm_step: bad shape");
  SC_REQUIRE(step_dims_supported(DQ, DV), "sc_mlstm_step: head dims (%d, %d) not compiled in", DQ,
             DV);
  SC_REQUIRE(NH > 0 && BH % NH == 0, "sc_mlstm_step: NH=%d does not divide BH=%d", NH, BH);
  if (BH == 0 || K == 0) return 0;
  SC_REQUIRE(q && k && v && igate && fgate && C && n && m && h, "sc_mlstm_step: null pointer");
  StepArgs a{};
  a.q = q; a.k = k; a.v = v; a.ig = igate; a.fg = fgate; a.live = live;
  a.C = C; a.n = n; a.m = m; a.h = h;
  a.BH = BH; a.K = K; a.NH = NH; a.cap = cap; a.eps = eps; a.scale = 1.0f / sqrtf((float)DQ);
  if (layout) {
    SC_REQUIRE(layout[0] == NH, "sc_mlstm_step: layout NH=%lld differs from NH=%d",
               (long long)layout[0], NH);
    for (int i = 1; i < 7; ++i)
      SC_REQUIRE(layout[i] >= 0 && layout[i] % 8 == 0,
                 "sc_mlstm_step: layout stride %lld is not a multiple of 8 elements",
                 (long long)layout[i]);
    a.qb = layout[1]; a.qh = layout[2]; a.qt = layout[3];
    a.vb = layout[4]; a.vh = layout[5]; a.vt = layout[6];
    SC_REQUIRE(a.qt >= DQ && a.vt >= DV, "sc_mlstm_step: layout row strides overlap the rows");
    for (const void* p : {q, k, v})
      SC_REQUIRE(((uintptr_t)p & 15) == 0,
                 "sc_mlstm_step: strided operands must be 16-byte aligned");
  } else {   // contiguous [BH][K][D]
    a.qb = (int64_t)NH * K * DQ; a.qh = (int64_t)K * DQ; a.qt = DQ;
    a.vb = (int64_t)NH * K * DV; a.vh = (int64_t)K * DV; a.vt = DV;
  }
  if (gate_layout) {   // {gb, gh, gt}: pre-activations in the io dtype inside the projection
    for (int i = 0; i < 3; ++i)
      SC_REQUIRE(gate_layout[i] >= 0, "sc_mlstm_step: negative gate stride");
    a.gproj = 1;
    a.gb = gate_layout[0]; a.gh = gate_layout[1]; a.gt = gate_layout[2];
  }
  hipStream_t st = (hipStream_t)stream;
  if (io_dtype == SC_F32) step_dispatch<SC_F32>(a, DQ, DV, st);
  else step_dispatch<SC_BF16>(a, DQ, DV, st);
  return launch_status("sc_mlstm_step");
}
