// viscy_amd — the exact-fp32 tile of dot products that the k-NN probe (online_eval.hip), the classifier head (aux_head.hip) and
// the MMD kernel sums (mmd.hip) share: a workgroup of FT_THREADS = 256 forms the FT_T x FT_T = 128 x 128 dots of 128 "query"
// rows with 128 "column" rows on the f32-in / f32-accumulate MFMA (v_mfma_f32_32x32x2_f32).  Both operands are staged through
// LDS in chunks of FT_KC = 32 features; each of the four waves owns a 64 x 64 quadrant of four 32 x 32 accumulators.  This
// header serves exactly this shape.
//
// Summation order.  A dot accumulates in fp32, 32 features per chunk in ascending chunk order.  Inside a chunk the feature
// index is permuted between the MFMA steps (lane half h, step s of group p reads feature 8p + 4h + s, for both operands
// alike), so that each lane fetches four steps' operands with one 16-byte LDS read; a sum over k does not care which k meets
// which step.  There is ONE order: the same for every (row, column), for every kernel built on ft_dots and for every entry
// point behind them — a similarity of vsx_knn_topk, a logit of vsx_cls_* and a distance of vsx_sqdist_upper over the same two
// rows hold the same dot, bit for bit, and so do the gathered target logit and the scanned one.  What fixes that order is
// written once, here: the operand map and issue order (ft_mma_step), the C/D map (ft_each) and the row loader (ft_row4).
#pragma once
#include "vsx_common.h"

constexpr int FT_T = 128;                    // rows of either operand per tile
constexpr int FT_KC = 32;                    // features per staged chunk
constexpr int FT_LD = 36;                    // floats per staged row: 32 + 4, keeps 16-byte alignment and spreads rows over the banks
constexpr int FT_SLD = 65;                   // floats per row of the result half-tile
constexpr int FT_THREADS = 256;
constexpr int FT_STAGE = 2 * FT_T * FT_LD;   // floats of the staging area (query chunk | column chunk); the half-tile (128 x 65) reuses it

typedef float ft_f32x16 __attribute__((ext_vector_type(16)));

static_assert(FT_T * FT_SLD <= FT_STAGE, "the result half-tile must fit the staging area");

// wave (wq, wc) owns rows wq * 64 .., columns wc * 64 .. of the tile; r32 / hh: the lane's place in the MFMA operand and C/D maps
struct FtLane {
  int t, wq, wc, r32, hh;
};
__device__ __forceinline__ FtLane ft_lane() {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  return {t, wave & 1, wave >> 1, lane & 31, lane >> 5};
}
// C/D map of the 32 x 32 MFMA: element e of accumulator acc[a][b] is tile row ft_row(l, a, e), tile column wc * 64 + b * 32 + r32
__device__ __forceinline__ int ft_row(const FtLane& l, int a, int e) { return l.wq * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * l.hh; }
// f(dot, tile row, tile column) for the lane's 64 dots
template <class F>
__device__ __forceinline__ void ft_each(const ft_f32x16 (&acc)[2][2], const FtLane& l, F&& f) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) f(acc[a][b][e], ft_row(l, a, e), l.wc * 64 + b * 32 + l.r32);
}

// the tiles of a workgroup: query rows q0 .. q0 + 127 (blockIdx.x), column tiles ct0 .. ct1 - 1 of ceil(ncols / 128)
// (blockIdx.y-th run of tiles_per_split), nchunks chunks of the d features
struct FtRange {
  int q0, ct0, ct1, nchunks;
};
__device__ __forceinline__ FtRange ft_range(int ncols, int d, int tiles_per_split) {
  const int ct0 = blockIdx.y * tiles_per_split;
  return {(int)blockIdx.x * FT_T, ct0, min(ct0 + tiles_per_split, (ncols + FT_T - 1) / FT_T), (d + FT_KC - 1) / FT_KC};
}
// a per-row side value of the tile's 128 rows i0 ..: dst[t] = src[i0 + t], pad past n
template <class T>
__device__ __forceinline__ void ft_side(T* dst, const T* __restrict__ src, int i0, int n, T pad) {
  const int t = threadIdx.x;
  if (t < FT_T) dst[t] = i0 + t < n ? src[i0 + t] : pad;
}

// four features of row `row` of x [nrows, d] from feature kk on; zeros past the row's end or for a row outside [0, nrows).
// VEC: d % 4 == 0 and x 16-byte aligned (ft_vec_ok), the four are one 16-byte read; else feature by feature
template <bool VEC>
__device__ __forceinline__ float4 ft_row4(const float* __restrict__ x, int row, int nrows, int d, int kk) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)row < (unsigned)nrows) {
    const float* src = x + (size_t)row * d + kk;
    if (VEC) {
      if (kk < d) v = *reinterpret_cast<const float4*>(src);
    } else {
      if (kk < d) v.x = src[0];
      if (kk + 1 < d) v.y = src[1];
      if (kk + 2 < d) v.z = src[2];
      if (kk + 3 < d) v.w = src[3];
    }
  }
  return v;
}
static inline bool ft_vec_ok(const float* x, int d) { return d % 4 == 0 && vsx_al16(x); }

// one thread's share of a chunk: 8 x 4 features; f = t + 256 u -> operand f >> 10, row (f & 1023) >> 3, feature quad f & 7, so
// that 8 consecutive lanes read 128 contiguous bytes of one row.  load(operand, row in tile, feature) -> that row's four
// features from `feature` on, zeros where there are none
template <class Load>
__device__ __forceinline__ void ft_fetch(float4* r, int t, int kc0, Load&& load) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int f = t + FT_THREADS * u;
    const int g = f & 1023;
    r[u] = load(f >> 10, g >> 3, kc0 + 4 * (g & 7));
  }
}

__device__ __forceinline__ void ft_zero(ft_f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
}
// acc += the products over eight features of the lane's rows: a0 / a1 hold four features of query rows r32 and 32 + r32 of the
// wave's quadrant, b0 / b1 the same four of its columns r32 and 32 + r32; the lane halves hold different fours.  The issue order
// is part of every result
__device__ __forceinline__ void ft_mma_step(ft_f32x16 (&acc)[2][2], const float4& a0, const float4& a1, const float (&b0)[4],
                                            const float (&b1)[4]) {
  const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], b0[s], acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], b1[s], acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], b0[s], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], b1[s], acc[1][1], 0, 0, 0);
  }
}

// acc = the tile's dots over nchunks chunks of features.  stage: FT_STAGE floats of LDS, 16-byte aligned.  first() runs once,
// between the first barrier and the first store to the staging area: LDS that the previous tile's readers are done with may be
// rewritten there, and is visible after the loop's second barrier.  The caller puts a barrier between the return and a rewrite
// of `stage`.
template <class Load, class First>
__device__ __forceinline__ void ft_dots(ft_f32x16 (&acc)[2][2], float* stage, const FtLane& l, int nchunks, Load&& load, First&& first) {
  ft_zero(acc);
  float4 pre[8];
  ft_fetch(pre, l.t, 0, load);
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // the previous chunk's reads (or the previous tile's scan of the half-tile) are done
    if (ch == 0) first();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = l.t + FT_THREADS * u;
      *reinterpret_cast<float4*>(stage + (size_t)(f >> 3) * FT_LD + 4 * (f & 7)) = pre[u];  // row f >> 3 of [query | column]
    }
    __syncthreads();
    if (ch + 1 < nchunks) ft_fetch(pre, l.t, (ch + 1) * FT_KC, load);
    const float* qa = stage + (size_t)(l.wq * 64 + l.r32) * FT_LD + 4 * l.hh;
    const float* cb = stage + (size_t)(FT_T + l.wc * 64 + l.r32) * FT_LD + 4 * l.hh;
#pragma unroll
    for (int p = 0; p < FT_KC / 8; ++p) {
      const float4 a0 = *reinterpret_cast<const float4*>(qa + 8 * p);
      const float4 a1 = *reinterpret_cast<const float4*>(qa + 32 * FT_LD + 8 * p);
      const float4 b0 = *reinterpret_cast<const float4*>(cb + 8 * p);
      const float4 b1 = *reinterpret_cast<const float4*>(cb + 32 * FT_LD + 8 * p);
      const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
      ft_mma_step(acc, a0, a1, bv0, bv1);
    }
  }
}

// the waves of column half h write stage[row * FT_SLD + (col & 63)] = val(dot, tile row, tile column) for their 64 x 64 dots;
// a barrier follows at the caller before thread r < 128 reads row r, and another before the next write
template <class Val>
__device__ __forceinline__ void ft_put_half(float* stage, const ft_f32x16 (&acc)[2][2], const FtLane& l, int h, Val&& val) {
  if (l.wc != h) return;
  ft_each(acc, l, [&](float dot, int row, int col) { stage[(size_t)row * FT_SLD + (col & 63)] = val(dot, row, col); });
}
__device__ __forceinline__ const float* ft_half_row(const float* stage, int row) { return stage + (size_t)row * FT_SLD; }

// ------------------------------------------------------------------ wave-per-row sums next to the dots
// the wave's total in every lane: the __shfl_xor butterfly from 32 down to 1.  wave_sum of vsx_common.h is NOT a substitute: that
// DPP butterfly pairs the lanes in another order and would change the last bits of every norm, similarity, logit and gradient
// that passes through here.  The order is part of the result
__device__ __forceinline__ float ft_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// inverse row norms that scale the dots, one wave per row: fmaf accumulation over c = lane, lane + 64, ..., then ft_wave_sum.
// CLAMP: inv = 1 / max(||x||, eps) (F.normalize's rule);  else inv = 1 / (||x|| + eps), 0 where the denominator is 0
template <bool CLAMP>
__global__ __launch_bounds__(256) void ft_inv_norm_kernel(const float* __restrict__ x, float* __restrict__ inv, int N, int d, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* xr = x + (size_t)row * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) ss = fmaf(xr[c], xr[c], ss);
  ss = ft_wave_sum(ss);
  if (lane != 0) return;
  if (CLAMP) {
    inv[row] = __fdiv_rn(1.f, fmaxf(sqrtf(ss), eps));
  } else {
    const float den = __fadd_rn(sqrtf(ss), eps);
    inv[row] = den == 0.f ? 0.f : __fdiv_rn(1.f, den);
  }
}
template <bool CLAMP>
static int ft_inv_norm(const char* who, const float* x, float* inv, int N, int d, float eps, hipStream_t s) {
  VSX_CHECK(x && inv && N >= 1 && d >= 1, "%s: bad arguments", who);
  hipLaunchKernelGGL(ft_inv_norm_kernel<CLAMP>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, x, inv, N, d, eps);
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ host: the column tiles of a row tile over workgroups
// `want` workgroups (clamped to 1 .. tiles) share `tiles` column tiles in equal runs of *tps, the last one shorter; *splits <= want
// is how many runs are not empty
static inline void ft_even_split(int tiles, long want, int* splits, int* tps) {
  const int s = (int)(want < 1 ? 1 : (want > tiles ? tiles : want));
  *tps = (tiles + s - 1) / s;
  *splits = (tiles + *tps - 1) / *tps;
}
