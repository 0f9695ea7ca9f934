// viscy_amd — SpotlightLoss (viscy_utils/losses/spotlight.py): masked MSE + Dice on the soft-thresholded prediction, per row
// r = (b, c) of N = Z*Y*X voxels, and the per-row Otsu thresholds of its default mode.
//
//   m   = mask weight (uint8 / bool byte, fp32 weight, or  t >= thr[r])
//   d   = p - t;   den = k - 2k|p| + 1;   raw = (p - k p) / den;   s = clamp(raw, 0, 1)
//   F = sum m,  Em = sum m d^2,  E = sum d^2,  S = sum s,  I = sum s m
//   mse_r = F > 0 ? Em / (F + eps) : E / N;   dice_r = 1 - 2 I / (S + F + eps);   real_r = 0 < F < N
//   loss  = lambda * mean_r mse_r + (1 - lambda) * (n_real > 0 ? sum_r real_r dice_r / n_real : 0)
//
// For k in (-1, 0) den is positive, raw has the sign of p and raw <= 1 exactly where p <= 1, so the clamp is decided on p
// itself: s = 0 for p <= 0, 1 for p >= 1, and the clamp passes a gradient exactly on 0 <= p <= 1 (both ends, as torch's clamp
// backward does), whatever the last bit of raw is.
//
// Every sum is formed in a fixed order: a workgroup owns one chunk of VSX_SPOTLIGHT_CHUNK voxels of one row, each thread adds
// its voxels in fp32 (<= 64 of them), the 256 thread sums are folded in float64 and stored (plain stores, no atomics) as the
// chunk's partial; one wave per row then folds the row's partials in float64 in a fixed order.  A chunk's count of ones is <= 16384,
// exact in fp32 — a running fp32 count over a whole 21 M-voxel row would not be.  Loss and gradient are bit-identical from run
// to run.
//
// Row starts are only element-aligned (odd N): a chunk is a scalar head up to the next 4-element boundary of the whole array,
// a body of 4-element vectors (16 B of fp32, 8 B of bf16, 4 B of mask bytes per lane) and a scalar tail.
#include "vsx_common.h"
#include "../../include/vsx.h"

#define SL_CHUNK VSX_SPOTLIGHT_CHUNK
#define SL_THREADS 256
#define SL_MAX_BINS 1024

struct SlConst {
  float c0, c1, num, dnum;  // den = c1 |p| + c0 (c0 = k + 1, c1 = -2k);  raw = num p / den (num = 1 - k);  s' = dnum / den^2 (1 - k^2)
};

static SlConst sl_const(double k) {
  SlConst c;
  c.c0 = (float)(k + 1.0);
  c.c1 = (float)(-2.0 * k);
  c.num = (float)(1.0 - k);
  c.dnum = (float)(1.0 - k * k);
  return c;
}

// where a chunk lies: [g0, g0 + len) of the flat (rows, N) array, split into head | 4-vectors | tail
struct SlSpan {
  long g0, gb, gt;
  int head, nv, tail;
};
__device__ __forceinline__ SlSpan sl_span(long r, int c, long N, int vec) {
  SlSpan s;
  const long e0 = (long)c * SL_CHUNK;
  const long rest = N - e0;
  const int len = (int)(rest < SL_CHUNK ? rest : (long)SL_CHUNK);
  s.g0 = r * N + e0;
  const int to_boundary = (int)((4 - (s.g0 & 3)) & 3);
  s.head = vec ? (to_boundary < len ? to_boundary : len) : len;
  s.nv = (len - s.head) >> 2;
  s.gb = s.g0 + s.head;
  s.gt = s.gb + 4L * s.nv;
  s.tail = len - s.head - 4 * s.nv;
  return s;
}

template <typename TP>
__device__ __forceinline__ void sl_load4(const TP* P, long g, float* p);
template <>
__device__ __forceinline__ void sl_load4<float>(const float* P, long g, float* p) {
  const float4 v = *reinterpret_cast<const float4*>(P + g);
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
template <>
__device__ __forceinline__ void sl_load4<bf16_t>(const bf16_t* P, long g, float* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(P + g);
  p[0] = __uint_as_float(v.x << 16); p[1] = __uint_as_float(v.x & 0xffff0000u);
  p[2] = __uint_as_float(v.y << 16); p[3] = __uint_as_float(v.y & 0xffff0000u);
}
template <typename TP>
__device__ __forceinline__ void sl_store4(TP* P, long g, const float* p);
template <>
__device__ __forceinline__ void sl_store4<float>(float* P, long g, const float* p) {
  *reinterpret_cast<float4*>(P + g) = make_float4(p[0], p[1], p[2], p[3]);
}
template <>
__device__ __forceinline__ void sl_store4<bf16_t>(bf16_t* P, long g, const float* p) {
  uint2 v;
  v.x = f32x2_to_bf16x2_bits(p[0], p[1]);
  v.y = f32x2_to_bf16x2_bits(p[2], p[3]);
  *reinterpret_cast<uint2*>(P + g) = v;
}

template <int MODE>
__device__ __forceinline__ float sl_mask1(const void* M, long g, float t, float thr) {
  if (MODE == VSX_SPOTLIGHT_THRESHOLD) return t >= thr ? 1.f : 0.f;
  if (MODE == VSX_SPOTLIGHT_MASK_U8) return (float)reinterpret_cast<const uint8_t*>(M)[g];
  return reinterpret_cast<const float*>(M)[g];
}
template <int MODE>
__device__ __forceinline__ void sl_mask4(const void* M, long g, const float* t, float thr, float* m) {
  if (MODE == VSX_SPOTLIGHT_THRESHOLD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = t[j] >= thr ? 1.f : 0.f;
  } else if (MODE == VSX_SPOTLIGHT_MASK_U8) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(M) + g);
    m[0] = (float)(w & 0xffu); m[1] = (float)((w >> 8) & 0xffu); m[2] = (float)((w >> 16) & 0xffu); m[3] = (float)(w >> 24);
  } else {
    sl_load4<float>(reinterpret_cast<const float*>(M), g, m);
  }
}

// s and the denominator it was formed with
__device__ __forceinline__ float sl_soft(float p, const SlConst& k, float& den) {
  den = fmaf(k.c1, fabsf(p), k.c0);
  const float raw = (k.num * p) / den;
  return p <= 0.f ? 0.f : (p >= 1.f ? 1.f : fminf(raw, 1.f));
}

struct SlAcc {
  float F, Em, E, S, I;
};
__device__ __forceinline__ void sl_add(SlAcc& a, float p, float t, float m, const SlConst& k) {
  const float d = p - t, d2 = d * d;
  float den;
  const float s = sl_soft(p, k, den);
  a.F += m;
  a.Em = fmaf(m, d2, a.Em);
  a.E += d2;
  a.S += s;
  a.I = fmaf(s, m, a.I);
}

// ------------------------------------------------------------------ forward: per-chunk partials of the five sums
template <typename TP, int MODE>
__global__ __launch_bounds__(SL_THREADS) void spotlight_sums_kernel(const TP* __restrict__ P, const float* __restrict__ T,
                                                                     const void* __restrict__ M, const float* __restrict__ thr,
                                                                     double* __restrict__ part, long N, int cpr, int vec, SlConst k) {
  const long bid = blockIdx.x;
  const long r = bid / cpr;
  const SlSpan sp = sl_span(r, (int)(bid - r * cpr), N, vec);
  const float th = MODE == VSX_SPOTLIGHT_THRESHOLD ? thr[r] : 0.f;
  const int tid = threadIdx.x;
  SlAcc a = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < sp.head; i += SL_THREADS) {
    const long g = sp.g0 + i;
    const float t = T[g];
    sl_add(a, to_f32<TP>(P[g]), t, sl_mask1<MODE>(M, g, t, th), k);
  }
  for (int i = tid; i < sp.nv; i += SL_THREADS) {
    const long g = sp.gb + 4L * i;
    float p[4], t[4], m[4];
    sl_load4<TP>(P, g, p);
    sl_load4<float>(T, g, t);
    sl_mask4<MODE>(M, g, t, th, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) sl_add(a, p[j], t[j], m[j], k);
  }
  for (int i = tid; i < sp.tail; i += SL_THREADS) {
    const long g = sp.gt + i;
    const float t = T[g];
    sl_add(a, to_f32<TP>(P[g]), t, sl_mask1<MODE>(M, g, t, th), k);
  }
  double v[5] = {(double)a.F, (double)a.Em, (double)a.E, (double)a.S, (double)a.I};
  __shared__ double red[SL_THREADS / 64][5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    v[j] = wave_sum_f64(v[j]);
    if ((tid & 63) == 0) red[tid >> 6][j] = v[j];
  }
  __syncthreads();
  if (tid < 5) part[bid * 5 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ------------------------------------------------------------------ finalise: fold the partials in a fixed order
// rowstat[r] = {mse_r, real_r * dice_r, real_r, F, I, D};  coef[r] = {a, b, c, e}:  dP = gout (d (a m + b) + s' (c m + e))
// One wave per row: lane l adds the partials of chunks l, l + 64, ... in order, then the 64 lane sums meet in a butterfly.
__global__ __launch_bounds__(SL_THREADS) void spotlight_rows_kernel(const double* __restrict__ part, double* __restrict__ rowstat,
                                                                     long R, long N, int cpr, double eps) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (SL_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= R) return;  // whole waves leave
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = lane; c < cpr; c += 64) {
    const double* q = part + (r * cpr + c) * 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] += q[j];
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) v[j] = wave_sum_f64(v[j]);
  if (lane == 0) {
    const double F = v[0], Em = v[1], E = v[2], S = v[3], I = v[4];
    const double D = S + F + eps;
    const double real = (F > 0.0 && F < (double)N) ? 1.0 : 0.0;
    double* o = rowstat + r * 6;
    o[0] = F > 0.0 ? Em / (F + eps) : E / (double)N;
    o[1] = real * (1.0 - 2.0 * I / D);
    o[2] = real;
    o[3] = F;
    o[4] = I;
    o[5] = D;
  }
}

// one workgroup: the sums over the rows (each thread its rows in order, then a fixed tree), the loss, the coefficients
__global__ __launch_bounds__(SL_THREADS) void spotlight_finalize_kernel(const double* __restrict__ rowstat, float* __restrict__ loss,
                                                                         float* __restrict__ coef, long R, long N, double lam,
                                                                         double eps) {
  const int tid = threadIdx.x;
  double t[3] = {0.0, 0.0, 0.0};
  for (long r = tid; r < R; r += SL_THREADS) {
    t[0] += rowstat[r * 6];
    t[1] += rowstat[r * 6 + 1];
    t[2] += rowstat[r * 6 + 2];
  }
  __shared__ double red[3][SL_THREADS];
#pragma unroll
  for (int j = 0; j < 3; ++j) red[j][tid] = t[j];
  __syncthreads();
  for (int h = SL_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int j = 0; j < 3; ++j) red[j][tid] += red[j][tid + h];
    }
    __syncthreads();
  }
  const double sum_mse = red[0][0], sum_dice = red[1][0], n_real = red[2][0];
  if (tid == 0) loss[0] = (float)(lam * sum_mse / (double)R + (1.0 - lam) * (n_real > 0.0 ? sum_dice / n_real : 0.0));
  const double wd = n_real > 0.0 ? (1.0 - lam) / n_real : 0.0;
  for (long r = tid; r < R; r += SL_THREADS) {
    const double real = rowstat[r * 6 + 2], F = rowstat[r * 6 + 3], I = rowstat[r * 6 + 4], D = rowstat[r * 6 + 5];
    const double wm = 2.0 * lam / (double)R;
    float* o = coef + r * 4;
    o[0] = F > 0.0 ? (float)(wm / (F + eps)) : 0.f;
    o[1] = F > 0.0 ? 0.f : (float)(wm / (double)N);
    o[2] = real > 0.0 ? (float)(-2.0 * wd / D) : 0.f;
    o[3] = real > 0.0 ? (float)(2.0 * wd * I / (D * D)) : 0.f;
  }
}

// ------------------------------------------------------------------ backward: one elementwise pass
__device__ __forceinline__ float sl_grad(float p, float t, float m, const float4& cf, float go, const SlConst& k) {
  const float den = fmaf(k.c1, fabsf(p), k.c0);
  const float ds = (p >= 0.f && p <= 1.f) ? k.dnum / (den * den) : 0.f;
  return go * ((p - t) * fmaf(cf.x, m, cf.y) + ds * fmaf(cf.z, m, cf.w));
}

template <typename TP, int MODE>
__global__ __launch_bounds__(SL_THREADS) void spotlight_bwd_kernel(const TP* __restrict__ P, const float* __restrict__ T,
                                                                    const void* __restrict__ M, const float* __restrict__ thr,
                                                                    const float* __restrict__ coef, const float* __restrict__ gout,
                                                                    TP* __restrict__ dP, long N, int cpr, int vec, SlConst k) {
  const long bid = blockIdx.x;
  const long r = bid / cpr;
  const SlSpan sp = sl_span(r, (int)(bid - r * cpr), N, vec);
  const float th = MODE == VSX_SPOTLIGHT_THRESHOLD ? thr[r] : 0.f;
  const float4 cf = make_float4(coef[r * 4], coef[r * 4 + 1], coef[r * 4 + 2], coef[r * 4 + 3]);
  const float go = gout[0];
  const int tid = threadIdx.x;
  for (int i = tid; i < sp.head; i += SL_THREADS) {
    const long g = sp.g0 + i;
    const float t = T[g];
    dP[g] = from_f32<TP>(sl_grad(to_f32<TP>(P[g]), t, sl_mask1<MODE>(M, g, t, th), cf, go, k));
  }
  for (int i = tid; i < sp.nv; i += SL_THREADS) {
    const long g = sp.gb + 4L * i;
    float p[4], t[4], m[4], o[4];
    sl_load4<TP>(P, g, p);
    sl_load4<float>(T, g, t);
    sl_mask4<MODE>(M, g, t, th, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = sl_grad(p[j], t[j], m[j], cf, go, k);
    sl_store4<TP>(dP, g, o);
  }
  for (int i = tid; i < sp.tail; i += SL_THREADS) {
    const long g = sp.gt + i;
    const float t = T[g];
    dP[g] = from_f32<TP>(sl_grad(to_f32<TP>(P[g]), t, sl_mask1<MODE>(M, g, t, th), cf, go, k));
  }
}

// ------------------------------------------------------------------ host side of the loss
static inline long sl_cpr(long n) { return (n + SL_CHUNK - 1) / SL_CHUNK; }

extern "C" int64_t vsx_spotlight_workspace(int32_t op, int64_t rows, int64_t n) {
  if (rows <= 0 || n <= 0) return 0;
  const long cpr = sl_cpr(n);
  if (op == VSX_SPOTLIGHT_WS_FWD) return (int64_t)sizeof(double) * (rows * cpr * 5 + rows * 6);
  if (op == VSX_SPOTLIGHT_WS_OTSU) return (int64_t)sizeof(float) * (rows * cpr * 2 + rows * 2 + rows * SL_MAX_BINS);
  return 0;
}

// dtype x the three mask modes: f(vsx_type<T>, integral_constant<int, mode>)
template <class F>
static __forceinline__ void sl_dispatch(int dtype, int mask_mode, F&& f) {
  vsx_by_dtype(dtype, [&](auto tag) {
    vsx_by_int<VSX_SPOTLIGHT_THRESHOLD, VSX_SPOTLIGHT_MASK_U8, VSX_SPOTLIGHT_MASK_F32>(mask_mode, [&](auto mode) { f(tag, mode); });
  });
}

static int sl_check(const char* who, const void* pred, int32_t dtype, const float* target, const void* mask, int32_t mask_mode,
                    const float* thr, int64_t rows, int64_t n, double k) {
  VSX_CHECK(pred && target && rows > 0 && n > 0, "%s: bad arguments", who);
  VSX_CHECK(dtype == VSX_F32 || dtype == VSX_BF16, "%s: pred must be fp32 or bf16 (dtype=%d)", who, dtype);
  VSX_CHECK(mask_mode >= VSX_SPOTLIGHT_THRESHOLD && mask_mode <= VSX_SPOTLIGHT_MASK_F32, "%s: unknown mask_mode %d", who, mask_mode);
  VSX_CHECK(mask_mode == VSX_SPOTLIGHT_THRESHOLD ? thr != nullptr : mask != nullptr, "%s: mask_mode %d without its %s", who,
            mask_mode, mask_mode == VSX_SPOTLIGHT_THRESHOLD ? "thresholds" : "mask");
  VSX_CHECK(k > -1.0 && k < 0.0, "%s: sigmoid_k must be in (-1, 0)", who);
  VSX_CHECK(rows * sl_cpr(n) < (1L << 24), "%s: %ld rows of %ld values need more than 2^24 workgroups", who, (long)rows, (long)n);
  return 0;
}

extern "C" int32_t vsx_spotlight_fwd(const void* pred, int32_t dtype, const float* target, const void* mask, int32_t mask_mode,
                                     const float* thr, int64_t rows, int64_t n, double lambda_mse, double sigmoid_k, double eps,
                                     void* ws, float* loss, float* coef, vsx_stream_t stream) {
  if (int rc = sl_check("vsx_spotlight_fwd", pred, dtype, target, mask, mask_mode, thr, rows, n, sigmoid_k)) return rc;
  VSX_CHECK(ws && loss && coef && ((uintptr_t)ws & 7) == 0, "vsx_spotlight_fwd: workspace (8-byte aligned), loss and coef are required");
  const int cpr = (int)sl_cpr(n);
  const int vec = (!pred || vsx_al16(pred)) && (!target || vsx_al16(target)) && (!mask || vsx_al16(mask));
  const SlConst k = sl_const(sigmoid_k);
  double* part = (double*)ws;
  double* rowstat = part + rows * cpr * 5;
  const dim3 grid((unsigned)(rows * cpr)), block(SL_THREADS);
  hipStream_t s = (hipStream_t)stream;
  sl_dispatch(dtype, mask_mode, [&](auto tag, auto mode) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((spotlight_sums_kernel<T, decltype(mode)::value>), grid, block, 0, s, (const T*)pred, target, mask, thr, part,
                       (long)n, cpr, vec, k);
  });
  hipLaunchKernelGGL(spotlight_rows_kernel, dim3((unsigned)((rows + SL_THREADS / 64 - 1) / (SL_THREADS / 64))), block, 0, s,
                     (const double*)part, rowstat, (long)rows, (long)n, cpr, eps);
  hipLaunchKernelGGL(spotlight_finalize_kernel, dim3(1), block, 0, s, (const double*)rowstat, loss, coef, (long)rows, (long)n,
                     lambda_mse, eps);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_spotlight_bwd(const void* pred, int32_t dtype, const float* target, const void* mask, int32_t mask_mode,
                                     const float* thr, const float* coef, const float* gout, void* dpred, int64_t rows, int64_t n,
                                     double sigmoid_k, vsx_stream_t stream) {
  if (int rc = sl_check("vsx_spotlight_bwd", pred, dtype, target, mask, mask_mode, thr, rows, n, sigmoid_k)) return rc;
  VSX_CHECK(coef && gout && dpred, "vsx_spotlight_bwd: coef, gout and dpred are required");
  const int cpr = (int)sl_cpr(n);
  const int vec = (!pred || vsx_al16(pred)) && (!target || vsx_al16(target)) && (!mask || vsx_al16(mask)) && (!dpred || vsx_al16(dpred));
  const SlConst k = sl_const(sigmoid_k);
  const dim3 grid((unsigned)(rows * cpr)), block(SL_THREADS);
  hipStream_t s = (hipStream_t)stream;
  sl_dispatch(dtype, mask_mode, [&](auto tag, auto mode) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((spotlight_bwd_kernel<T, decltype(mode)::value>), grid, block, 0, s, (const T*)pred, target, mask, thr, coef, gout,
                       (T*)dpred, (long)n, cpr, vec, k);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ Otsu thresholds (spotlight.py:50-110), all on the device
// 1. per-chunk min / max (plain stores)   2. per-row fold of them + zeroing of the row's counts   3. per-chunk histogram in LDS,
// merged with integer atomics (order-independent)   4. per-row scan in float64.
__global__ __launch_bounds__(SL_THREADS) void otsu_minmax_kernel(const float* __restrict__ T, float* __restrict__ mm, long N, int cpr,
                                                                  int vec) {
  const long bid = blockIdx.x;
  const long r = bid / cpr;
  const SlSpan sp = sl_span(r, (int)(bid - r * cpr), N, vec);
  const int tid = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < sp.head; i += SL_THREADS) {
    const float x = T[sp.g0 + i];
    lo = fminf(lo, x); hi = fmaxf(hi, x);
  }
  for (int i = tid; i < sp.nv; i += SL_THREADS) {
    float t[4];
    sl_load4<float>(T, sp.gb + 4L * i, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo = fminf(lo, t[j]); hi = fmaxf(hi, t[j]); }
  }
  for (int i = tid; i < sp.tail; i += SL_THREADS) {
    const float x = T[sp.gt + i];
    lo = fminf(lo, x); hi = fmaxf(hi, x);
  }
  hi = wave_max(hi);
  lo = -wave_max(-lo);
  __shared__ float red[2][SL_THREADS / 64];
  if ((tid & 63) == 0) { red[0][tid >> 6] = lo; red[1][tid >> 6] = hi; }
  __syncthreads();
  if (tid == 0) {
    mm[bid * 2] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    mm[bid * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__global__ __launch_bounds__(64) void otsu_fold_kernel(const float* __restrict__ mm, float* __restrict__ lohi,
                                                        uint32_t* __restrict__ hist, int cpr, int nb) {
  const long r = blockIdx.x;
  const int lane = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int c = lane; c < cpr; c += 64) {
    lo = fminf(lo, mm[(r * cpr + c) * 2]);
    hi = fmaxf(hi, mm[(r * cpr + c) * 2 + 1]);
  }
  hi = wave_max(hi);
  lo = -wave_max(-lo);
  if (lane == 0) { lohi[r * 2] = lo; lohi[r * 2 + 1] = hi; }
  for (int i = lane; i < nb; i += 64) hist[r * nb + i] = 0u;
}

// bin = min((int)((x - lo) * nb / (hi - lo)), nb - 1): every operation rounded on its own in fp32, IEEE division — the form that
// gives torch.histc's counts on the CPU
#pragma clang fp contract(off)
__device__ __forceinline__ int otsu_bin(float x, float lo, float width, float fnb, int nb) {
  int b = (int)(((x - lo) * fnb) / width);
  b = b < 0 ? 0 : b;
  return b > nb - 1 ? nb - 1 : b;
}

__global__ __launch_bounds__(SL_THREADS) void otsu_hist_kernel(const float* __restrict__ T, const float* __restrict__ lohi,
                                                                uint32_t* __restrict__ hist, long N, int cpr, int vec, int nb) {
  const long bid = blockIdx.x;
  const long r = bid / cpr;
  const float lo = lohi[r * 2], hi = lohi[r * 2 + 1];
  if (!(hi > lo)) return;  // constant row (or NaN bounds): no histogram, the scan answers lo
  const SlSpan sp = sl_span(r, (int)(bid - r * cpr), N, vec);
  const int tid = threadIdx.x;
  __shared__ uint32_t h[SL_MAX_BINS];
  for (int i = tid; i < nb; i += SL_THREADS) h[i] = 0u;
  __syncthreads();
  const float width = hi - lo, fnb = (float)nb;
  for (int i = tid; i < sp.head; i += SL_THREADS) atomicAdd(&h[otsu_bin(T[sp.g0 + i], lo, width, fnb, nb)], 1u);
  for (int i = tid; i < sp.nv; i += SL_THREADS) {
    float t[4];
    sl_load4<float>(T, sp.gb + 4L * i, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicAdd(&h[otsu_bin(t[j], lo, width, fnb, nb)], 1u);
  }
  for (int i = tid; i < sp.tail; i += SL_THREADS) atomicAdd(&h[otsu_bin(T[sp.gt + i], lo, width, fnb, nb)], 1u);
  __syncthreads();
  for (int i = tid; i < nb; i += SL_THREADS)
    if (h[i]) atomicAdd(&hist[r * nb + i], h[i]);
}

// inter-class variance as the reference writes it (mu^2 / (w0 w1 + 1e-10), mu = cum_mean * total - global_mean * cum_sum), first
// maximum; cumulative counts and means in float64; threshold = centre of the chosen bin
__global__ __launch_bounds__(64) void otsu_scan_kernel(const uint32_t* __restrict__ hist, const float* __restrict__ lohi,
                                                        float* __restrict__ thr, int nb) {
  const long r = blockIdx.x;
  const int lane = threadIdx.x;
  const float lo = lohi[r * 2], hi = lohi[r * 2 + 1];
  if (!(hi > lo)) {
    if (lane == 0) thr[r] = lo;
    return;
  }
  __shared__ uint32_t h[SL_MAX_BINS];
  for (int i = lane; i < nb; i += 64) h[i] = hist[r * nb + i];
  __syncthreads();
  if (lane != 0) return;
  const double dlo = (double)lo, w = (double)hi - (double)lo;
  double total = 0.0, gmean = 0.0;
  for (int i = 0; i < nb; ++i) {
    const double c = dlo + ((i + 0.5) * w) / (double)nb;
    total += (double)h[i];
    gmean += (double)h[i] * c;
  }
  double cs = 0.0, cm = 0.0, best = -1.0;
  int bi = 0;
  for (int i = 0; i < nb; ++i) {
    const double c = dlo + ((i + 0.5) * w) / (double)nb;
    cs += (double)h[i];
    cm += (double)h[i] * c;
    const double mu = cm * total - gmean * cs;
    const double var = mu * mu / (cs * (total - cs) + 1e-10);
    if (var > best) { best = var; bi = i; }
  }
  thr[r] = (float)(dlo + ((bi + 0.5) * w) / (double)nb);
}

extern "C" int32_t vsx_otsu_threshold(const float* target, float* thr, void* ws, int64_t rows, int64_t n, int32_t n_bins,
                                      vsx_stream_t stream) {
  VSX_CHECK(target && thr && ws && rows > 0 && n > 0, "vsx_otsu_threshold: bad arguments");
  VSX_CHECK(n_bins >= 2 && n_bins <= SL_MAX_BINS, "vsx_otsu_threshold: n_bins=%d must be in [2, %d]", n_bins, SL_MAX_BINS);
  VSX_CHECK(((uintptr_t)ws & 3) == 0, "vsx_otsu_threshold: the workspace must be 4-byte aligned");
  VSX_CHECK(rows * sl_cpr(n) < (1L << 24), "vsx_otsu_threshold: %ld rows of %ld values need more than 2^24 workgroups", (long)rows, (long)n);
  const int cpr = (int)sl_cpr(n);
  const int vec = (!target || vsx_al16(target));
  float* mm = (float*)ws;
  float* lohi = mm + rows * cpr * 2;
  uint32_t* hist = (uint32_t*)(lohi + rows * 2);
  const dim3 chunks((unsigned)(rows * cpr)), per_row((unsigned)rows);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(otsu_minmax_kernel, chunks, dim3(SL_THREADS), 0, s, target, mm, (long)n, cpr, vec);
  hipLaunchKernelGGL(otsu_fold_kernel, per_row, dim3(64), 0, s, (const float*)mm, lohi, hist, cpr, (int)n_bins);
  hipLaunchKernelGGL(otsu_hist_kernel, chunks, dim3(SL_THREADS), 0, s, target, (const float*)lohi, hist, (long)n, cpr, vec, (int)n_bins);
  hipLaunchKernelGGL(otsu_scan_kernel, per_row, dim3(64), 0, s, (const uint32_t*)hist, (const float*)lohi, thr, (int)n_bins);
  VSX_LAUNCH_CHECK();
  return 0;
}
