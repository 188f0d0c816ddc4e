// The RWKV-4 encoder's streaming step (gfx950): what a block of K frames of B concurrent streams
// needs besides its GEMMs, in three kernels.
//
//   wkv_step_kernel       the recurrent WKV operator: one thread per (stream, channel) reads
//                         (num, den, max) once, holds them in registers over the K steps and writes
//                         them back once, in place.  The arithmetic of a step is wkv_push and the
//                         y_t formula of wkv.hip; with r given the output is sigmoid(r) y (the
//                         receptance gate).  A step with live == 0 leaves the state alone and
//                         writes a zero row.
//   rwkv_step_mix_kernel  residual update, LayerNorm(s), time shift and the time mixes: one
//                         workgroup of 256 threads per stream walks its K frames with the row in
//                         registers (thread i holds elements i, i + 256, ...: coalesced, H <= 2048
//                         is at most 8 per thread) and the previous live frame's LayerNorm output
//                         beside it, so the shift costs no memory traffic inside a block.  The
//                         statistics are two-pass fp32 (mean, then the centred squares), each a DPP
//                         wave sum and one LDS exchange between the four waves.
//   relu_sq_kernel        max(x, 0)^2 in place (the feed-forward's squared ReLU).
//
// Bitwise rules.  A frame's arithmetic depends on nothing but its own operands and the carried
// state: K frames in one call equal K calls of one frame.  The floating-point contraction is
// switched off in this file and every fused multiply-add is written out, so the compiler cannot
// fuse one unrolled step differently from another.
//
// All three are latency-bound at streaming sizes (B x K rows of 512 .. 2048 elements): they are
// written for few launches and no scratch, not for bandwidth.

#include "sc_common.h"

#pragma clang fp contract(off)

namespace sc {

constexpr float kStepEmpty = -1e38f;
constexpr int kMixThreads = 256;
constexpr int kMixMaxH = 2048;

// ---------------------------------------------------------------------------- WKV step -------
struct WkvStepArgs {
  const float* td;
  const float* tf;
  const void* k;
  const void* v;
  const void* r;        // or null
  const float* live;    // [K][B] or null
  float *num, *den, *mx;
  void* y;
  int64_t st, sb;       // k / v / r strides (elements): frame, row
  int64_t yt, yb;       // y strides
  int K, B, C;
};

template <int DT>
__global__ void __launch_bounds__(64) wkv_step_kernel(WkvStepArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= a.C) return;
  const float W = -expf(a.td[c]), u = a.tf[c];
  const int64_t si = (int64_t)b * a.C + c;
  float n = a.num[si], d = a.den[si], m = a.mx[si];
  const T* kp = (const T*)a.k + b * a.sb + c;
  const T* vp = (const T*)a.v + b * a.sb + c;
  const T* rp = a.r ? (const T*)a.r + b * a.sb + c : nullptr;
  T* yp = (T*)a.y + b * a.yb + c;
  // the next step's operands are in flight during a step's arithmetic
  T ck = kp[0], cv = vp[0], cr = rp ? rp[0] : E::st(0.0f);
  bool any = false;
  for (int t = 0; t < a.K; ++t) {
    const T nk = ck, nv = cv, nr = cr;
    if (t + 1 < a.K) {
      ck = kp[(t + 1) * a.st];
      cv = vp[(t + 1) * a.st];
      if (rp) cr = rp[(t + 1) * a.st];
    }
    const bool on = !a.live || a.live[(int64_t)t * a.B + b] != 0.0f;   // workgroup-uniform
    float y = 0.0f;
    if (on) {
      const float kk = E::ld(nk), vv = E::ld(nv);
      const float uk = u + kk;
      const float mo = vmax(m, uk);
      const float e1 = fexp(m - mo), e2 = fexp(uk - mo);
      y = __builtin_fmaf(e1, n, e2 * vv) / __builtin_fmaf(e1, d, e2);
      if (rp) y = sigm(E::ld(nr)) * y;
      const float mw = m + W;
      const float ms = vmax(mw, kk);
      const float f1 = fexp(mw - ms), f2 = fexp(kk - ms);
      n = __builtin_fmaf(f1, n, f2 * vv);
      d = __builtin_fmaf(f1, d, f2);
      m = ms;
      any = true;
    }
    yp[t * a.yt] = E::st(y);
  }
  if (any) {
    a.num[si] = n;
    a.den[si] = d;
    a.mx[si] = m;
  }
}

// ---------------------------------------------------------------------------- step mix -------
struct StepMixArgs {
  float* h;             // [K][B][H] residual rows, in place
  const void* add;      // or null
  const void* gate;     // or null
  const float *pre_w, *pre_b;   // or null
  const float *ln_w, *ln_b;
  float* x_prev;        // [B][H], in place (null: nmix == 0 and nothing carried)
  const float* live;    // [K][B] or null
  const float* mix[3];
  void* out[3];
  int64_t ht, hb, at, ab, ot, ob;   // strides (elements): frame, row
  float eps;
  int nmix, K, B, H;
};

// sum over the workgroup's 256 threads in a fixed order; every thread gets the result
__device__ __forceinline__ float block_sum(float x, float* red) {
  const float w = wave_sum_dpp(x);
  __syncthreads();   // the previous exchange has been read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// x <- LayerNorm(x) over the H elements the workgroup holds (element j * 256 + tid in x[j])
template <int NE>
__device__ __forceinline__ void layer_norm_rows(float (&x)[NE], const float* w, const float* b,
                                                int H, float eps, float* red) {
  const int tid = threadIdx.x;
  const float inv = 1.0f / (float)H;
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < NE; ++j) s += (j * kMixThreads + tid < H) ? x[j] : 0.0f;
  const float mean = block_sum(s, red) * inv;
  float q = 0.0f;
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const float dlt = x[j] - mean;
    q += (j * kMixThreads + tid < H) ? dlt * dlt : 0.0f;
  }
  const float rstd = 1.0f / sqrtf(block_sum(q, red) * inv + eps);
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int i = j * kMixThreads + tid;
    if (i < H) x[j] = __builtin_fmaf((x[j] - mean) * rstd, w[i], b[i]);
  }
}

template <int DT, int NE>
__global__ void __launch_bounds__(kMixThreads) rwkv_step_mix_kernel(StepMixArgs a) {
  using E = Elem<DT>;
  using T = typename E::T;
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.x, H = a.H;
  float s[NE], x[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int i = j * kMixThreads + tid;
    s[j] = (a.x_prev && i < H) ? a.x_prev[(int64_t)b * H + i] : 0.0f;
  }
  bool any = false;
  for (int t = 0; t < a.K; ++t) {
    const bool on = !a.live || a.live[(int64_t)t * a.B + b] != 0.0f;   // workgroup-uniform
    float* hp = a.h + t * a.ht + b * a.hb;
    const int64_t ao = t * a.at + b * a.ab;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int i = j * kMixThreads + tid;
      x[j] = 0.0f;
      if (i < H) {
        x[j] = hp[i];
        if (a.add) {
          const float ad = E::ld(((const T*)a.add)[ao + i]);
          x[j] = a.gate ? __builtin_fmaf(sigm(E::ld(((const T*)a.gate)[ao + i])), ad, x[j])
                        : x[j] + ad;
        }
      }
    }
    if (a.pre_w) layer_norm_rows<NE>(x, a.pre_w, a.pre_b, H, a.eps, red);
    if (a.add || a.pre_w) {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const int i = j * kMixThreads + tid;
        if (i < H) hp[i] = x[j];
      }
    }
    layer_norm_rows<NE>(x, a.ln_w, a.ln_b, H, a.eps, red);
    const int64_t oo = t * a.ot + b * a.ob;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int i = j * kMixThreads + tid;
      if (i < H) {
        if (a.nmix == 0) {
          ((T*)a.out[0])[oo + i] = E::st(x[j]);
        } else {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            if (q < a.nmix) {
              const float mq = a.mix[q][i];
              ((T*)a.out[q])[oo + i] = E::st(__builtin_fmaf(x[j], mq, s[j] * (1.0f - mq)));
            }
          }
        }
      }
    }
    if (on) {
#pragma unroll
      for (int j = 0; j < NE; ++j) s[j] = x[j];
      any = true;
    }
  }
  if (any && a.x_prev) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int i = j * kMixThreads + tid;
      if (i < H) a.x_prev[(int64_t)b * H + i] = s[j];
    }
  }
}

template <int DT>
static void launch_mix(const StepMixArgs& a, hipStream_t st) {
  const int ne = (a.H + kMixThreads - 1) / kMixThreads;
  const dim3 grid(a.B), block(kMixThreads);
  if (ne <= 1) hipLaunchKernelGGL((rwkv_step_mix_kernel<DT, 1>), grid, block, 0, st, a);
  else if (ne <= 2) hipLaunchKernelGGL((rwkv_step_mix_kernel<DT, 2>), grid, block, 0, st, a);
  else if (ne <= 4) hipLaunchKernelGGL((rwkv_step_mix_kernel<DT, 4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((rwkv_step_mix_kernel<DT, 8>), grid, block, 0, st, a);
}

// ---------------------------------------------------------------------------- squared ReLU ---
// 16 bytes per thread where the array allows it (16-byte aligned base), the tail element-wise
template <int DT>
__global__ void __launch_bounds__(256) relu_sq_kernel(void* xv, int64_t nvec, int64_t n) {
  using E = Elem<DT>;
  using T = typename E::T;
  using V = Vec16<DT>;
  T* x = (T*)xv;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nvec) {
    float f[V::N];
    V::ld(x + i * V::N, f);
#pragma unroll
    for (int j = 0; j < V::N; ++j) {
      const float p = vmax(f[j], 0.0f);
      f[j] = p * p;
    }
    V::st(x + i * V::N, f);
  } else {
    const int64_t e = nvec * V::N + (i - nvec);
    if (e < n) {
      const float p = vmax(E::ld(x[e]), 0.0f);
      x[e] = E::st(p * p);
    }
  }
}

}  // namespace sc

using namespace sc;

extern "C" int sc_wkv_step(const float* time_decay, const float* time_first, const void* k,
                           const void* v, const void* r, int dtype, int64_t stride_t,
                           int64_t stride_b, const float* live, float* num, float* den, float* max,
                           void* y, int64_t y_stride_t, int64_t y_stride_b, int K, int B, int C,
                           void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16, "sc_wkv_step: dtype %d (fp32 or bf16 only)",
             dtype);
  SC_REQUIRE(K >= 0 && B >= 0 && C >= 0 && B <= 65535,
             "sc_wkv_step: bad shape K=%d B=%d C=%d (B <= 65535)", K, B, C);
  if (K == 0 || B == 0 || C == 0) return 0;
  SC_REQUIRE(num && den && max, "sc_wkv_step: null state (num, den, max are updated in place)");
  SC_REQUIRE(time_decay && time_first && k && v && y, "sc_wkv_step: null pointer");
  SC_REQUIRE(stride_t >= 0 && stride_b >= 0 && y_stride_t >= 0 && y_stride_b >= 0,
             "sc_wkv_step: negative stride");
  SC_REQUIRE(y_stride_b >= C && (K == 1 || y_stride_t >= C),
             "sc_wkv_step: y rows overlap (strides %lld, %lld below C=%d)", (long long)y_stride_t,
             (long long)y_stride_b, C);
  WkvStepArgs a{};
  a.td = time_decay; a.tf = time_first; a.k = k; a.v = v; a.r = r; a.live = live;
  a.num = num; a.den = den; a.mx = max; a.y = y;
  a.st = stride_t; a.sb = stride_b; a.yt = y_stride_t; a.yb = y_stride_b;
  a.K = K; a.B = B; a.C = C;
  const dim3 grid((C + 63) / 64, B), block(64);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SC_F32) hipLaunchKernelGGL(wkv_step_kernel<SC_F32>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(wkv_step_kernel<SC_BF16>, grid, block, 0, st, a);
  return launch_status("sc_wkv_step");
}

extern "C" int sc_rwkv_step_mix(float* h, int64_t h_stride_t, int64_t h_stride_b, const void* add,
                                const void* gate, int64_t add_stride_t, int64_t add_stride_b,
                                int io_dtype, const float* pre_w, const float* pre_b,
                                const float* ln_w, const float* ln_b, float eps, float* x_prev,
                                const float* live, int nmix, const float* mix0, const float* mix1,
                                const float* mix2, void* out0, void* out1, void* out2,
                                int64_t out_stride_t, int64_t out_stride_b, int K, int B, int H,
                                void* stream) {
  clear_error();
  SC_REQUIRE(io_dtype == SC_F32 || io_dtype == SC_BF16,
             "sc_rwkv_step_mix: io_dtype %d (fp32 or bf16 only)", io_dtype);
  SC_REQUIRE(K >= 0 && B >= 0, "sc_rwkv_step_mix: bad shape K=%d B=%d", K, B);
  SC_REQUIRE(H >= 1 && H <= kMixMaxH, "sc_rwkv_step_mix: H = %d outside [1, %d]", H, kMixMaxH);
  SC_REQUIRE(nmix >= 0 && nmix <= 3, "sc_rwkv_step_mix: nmix = %d outside [0, 3]", nmix);
  if (K == 0 || B == 0) return 0;
  SC_REQUIRE(h && ln_w && ln_b, "sc_rwkv_step_mix: null pointer (h, ln_w, ln_b)");
  SC_REQUIRE(x_prev || nmix == 0,
             "sc_rwkv_step_mix: null state (x_prev is what the mixes shift in)");
  SC_REQUIRE((pre_w == nullptr) == (pre_b == nullptr),
             "sc_rwkv_step_mix: pre_ln needs weight and bias");
  SC_REQUIRE(add || !gate, "sc_rwkv_step_mix: gate without add");
  const float* mix[3] = {mix0, mix1, mix2};
  void* out[3] = {out0, out1, out2};
  for (int i = 0; i < (nmix ? nmix : 1); ++i)
    SC_REQUIRE(out[i] && (nmix == 0 || mix[i]), "sc_rwkv_step_mix: mix / out %d is null", i);
  SC_REQUIRE(h_stride_t >= 0 && h_stride_b >= H && add_stride_t >= 0 && add_stride_b >= 0 &&
                 out_stride_t >= 0 && out_stride_b >= H && (K == 1 || (h_stride_t >= H &&
                                                                       out_stride_t >= H)),
             "sc_rwkv_step_mix: h / out rows overlap or a stride is negative");
  StepMixArgs a{};
  a.h = h; a.add = add; a.gate = gate; a.pre_w = pre_w; a.pre_b = pre_b; a.ln_w = ln_w;
  a.ln_b = ln_b; a.x_prev = x_prev; a.live = live;
  for (int i = 0; i < 3; ++i) {
    a.mix[i] = mix[i];
    a.out[i] = out[i];
  }
  a.ht = h_stride_t; a.hb = h_stride_b; a.at = add_stride_t; a.ab = add_stride_b;
  a.ot = out_stride_t; a.ob = out_stride_b;
  a.eps = eps; a.nmix = nmix; a.K = K; a.B = B; a.H = H;
  hipStream_t st = (hipStream_t)stream;
  if (io_dtype == SC_F32) launch_mix<SC_F32>(a, st);
  else launch_mix<SC_BF16>(a, st);
  return launch_status("sc_rwkv_step_mix");
}

extern "C" int sc_relu_sq(void* x, int dtype, int64_t n, void* stream) {
  clear_error();
  SC_REQUIRE(dtype == SC_F32 || dtype == SC_BF16, "sc_relu_sq: dtype %d (fp32 or bf16 only)",
             dtype);
  SC_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "sc_relu_sq: bad length %lld", (long long)n);
  if (n == 0) return 0;
  SC_REQUIRE(x, "sc_relu_sq: null pointer");
  const int vn = dtype == SC_F32 ? 4 : 8;
  const int64_t nvec = ((uintptr_t)x % 16 == 0) ? n / vn : 0;
  const int64_t threads = nvec + (n - nvec * vn);
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SC_F32) hipLaunchKernelGGL(relu_sq_kernel<SC_F32>, grid, block, 0, st, x, nvec, n);
  else hipLaunchKernelGGL(relu_sq_kernel<SC_BF16>, grid, block, 0, st, x, nvec, n);
  return launch_status("sc_relu_sq");
}
