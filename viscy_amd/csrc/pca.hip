// viscy_amd — the data passes of PCA (viscy_utils/evaluation/dimensionality_reduction.py: StandardScaler -> sklearn PCA) over
// x [n, d] fp32 row-major, n up to 2^31 - 1 rows, d <= 4096 features.  Everything after them is a d x d problem for the host.
//
//   vsx_col_moments     mean_j = sum_i x_ij / n,  m2_j = sum_i (x_ij - mean_j)^2            float64, two passes
//   vsx_gram_centered   G_jl = sum_i fl32(x_ij - mean_j) fl32(x_il - mean_l)               float64 [d, d], symmetric, full
//   vsx_gram_scaled     G_jl = sum_i fl32(q_i c_ij) fl32(q_i c_il),  c_ij = fl32(x_ij - mean_j)   the same kernel, one multiply more
//   vsx_center_project  z_ic = sum_j fl32(x_ij - mean_j) w_cj                              fp32 [n, k], the dots of f32_tile.h
//
// No atomics anywhere: workgroups write partials to rows of the workspace that are theirs alone and a second kernel folds them in
// ascending order, so every result is a pure function of (x, n, d), bit-identical from run to run.
//
// The Gram pass.  A workgroup owns one 128 x 128 tile of feature pairs (upper-triangular tile pairs only) and one contiguous
// split of the rows.  Both MFMA operands are slabs of the SAME GM_KC rows of x, 128 features wide, contiguous along d: the slab
// goes to LDS as [row][feature] with the mean subtracted (in float64, rounded once to fp32), and lane (feature = lane & 31,
// k = lane >> 5) of v_mfma_f32_32x32x2_f32 reads slab[2 s + k][feature]: 32 consecutive lanes read 32 consecutive floats, the two
// halves rows that GM_LD = 160 floats apart put on the other 32 banks.  No transpose.  The products accumulate in fp32 over a
// block of GM_R = 128 rows in ascending row order and the block sum is then added to a float64 accumulator, block after block:
// the fp32 part of the error is that of a 128-term sum (worst case 128 * 2^-24 relative to sum |c_j c_l|, the bound
// vsx_mmd_sums' label product already carries) whatever n is; past the block everything is float64.
#include "col_split.h"
#include "f32_tile.h"
#include "../../include/vsx.h"

#define PCA_MAX_D VSX_PCA_MAX_D
#define GM_R 128             // rows per fp32 block
#define GM_KC 32             // rows per staged slab
#define GM_LD 160            // floats per slab row: 128 + 32, rows 2 s and 2 s + 1 on different banks
#define GM_SLAB (GM_KC * GM_LD)
#define GM_MIN_BLOCKS 4      // blocks per split at least: a split reads >= 512 rows for the 128 KiB it writes
#define GM_MAX_SPLITS 32
#define GM_WANT_WGS 512      // two rounds of one workgroup per compute unit (the float64 accumulators leave room for one)

static_assert(GM_R % GM_KC == 0 && GM_KC % 8 == 0, "a block is whole slabs, a slab whole groups of eight rows");

// ------------------------------------------------------------------ (a) column moments
// PASS 0: sum of x;  PASS 1: sum of (x - mean)^2, the difference in float64.  Thread (column lane, row lane) adds rows
// r0 + lane, r0 + lane + 4, ... in float64; the four row lanes are folded 0 .. 3; part[split][column]
template <int PASS>
__global__ __launch_bounds__(CM_COLS * CM_LANES) void pca_moment_kernel(const float* __restrict__ x, const double* __restrict__ mean, long n,
                                                                        int d, long rows_per_split, double* __restrict__ part) {
  __shared__ double red[CM_LANES][CM_COLS];
  const int cl = threadIdx.x & (CM_COLS - 1), rl = threadIdx.x / CM_COLS;
  const int col = blockIdx.x * CM_COLS + cl;
  const long r0 = (long)blockIdx.y * rows_per_split;
  const long r1 = min(r0 + rows_per_split, n);
  double s = 0.0;
  if (col < d) {
    const double m = PASS ? mean[col] : 0.0;
    const float* p = x + (size_t)col;
#pragma unroll 4
    for (long r = r0 + rl; r < r1; r += CM_LANES) {
      const double v = (double)p[(size_t)r * (size_t)d] - m;
      s += PASS ? v * v : v;
    }
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < d) {
    double tot = red[0][cl];
    for (int q = 1; q < CM_LANES; ++q) tot += red[q][cl];
    part[(size_t)blockIdx.y * d + col] = tot;
  }
}
// ------------------------------------------------------------------ (b) centred Gram
// the centring of four fetched features as they go to LDS: float64 differences, each rounded once.  mu: the tile's means, 0
// past d, where ft_row4 has fetched zeros; a row outside the split stays zero.  SCALED: each centred value times the row's
// q in fp32, rounded once more
template <bool SCALED>
__device__ __forceinline__ float4 gm_centre4(const float4& v, bool row_ok, const double* mu, float q) {
  if (!row_ok) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 c = make_float4((float)((double)v.x - mu[0]), (float)((double)v.y - mu[1]), (float)((double)v.z - mu[2]), (float)((double)v.w - mu[3]));
  if (!SCALED) return c;
  return make_float4(__fmul_rn(q, c.x), __fmul_rn(q, c.y), __fmul_rn(q, c.z), __fmul_rn(q, c.w));
}

// grid (tile pairs, splits).  ws [split][pair][128][128] doubles, row-major in the tile.  SCALED: qrow [n] scales the rows and
// mean may be null (no centring)
template <bool VEC, bool SCALED>
__global__ __launch_bounds__(FT_THREADS, 1) void pca_gram_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                                 const float* __restrict__ qrow, long n, int d, int tiles,
                                                                 long rows_per_split, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float slab[2 * GM_SLAB];  // features of tile ti | of tile tj, the same rows
  __shared__ double mu[2][FT_T];

  const FtLane l = ft_lane();
  const int t = l.t;
  int ti = 0, p = blockIdx.x;
  while (p >= tiles - ti) p -= tiles - ti, ++ti;  // pair p of the upper triangle, row-major
  const int tj = ti + p;
  const bool diag = ti == tj;
  const long r0 = (long)blockIdx.y * rows_per_split;
  const long r1 = min(r0 + rows_per_split, n);
  const int nch = (int)((r1 - r0 + GM_KC - 1) / GM_KC);

  if (t < FT_T) {
    const int ca = ti * FT_T + t, cb = tj * FT_T + t;
    const bool centred = !SCALED || mean != nullptr;
    mu[0][t] = centred && ca < d ? mean[ca] : 0.0;
    mu[1][t] = centred && cb < d ? mean[cb] : 0.0;
  }
  __syncthreads();

  // one thread's share of a slab pair: f = t + 256 u -> operand u >> 2, slab row (f & 1023) >> 5, feature quad f & 31, so that 32
  // consecutive lanes read 512 contiguous bytes of one row.  The fetch keeps the raw values: they are centred when they go to LDS,
  // one slab later, so the loads are in flight while the MFMAs of the slab before run
  const int nu = diag ? 4 : 8;
  float4 pre[8];
  float qpre[4] = {1.f, 1.f, 1.f, 1.f};  // SCALED: q of the thread's four slab rows, (t >> 5) + 8 u
  auto fetch = [&](int ch) {
    if (SCALED) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long r = r0 + (long)ch * GM_KC + (t >> 5) + 8 * u;
        qpre[u] = r < r1 ? qrow[r] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < nu) {
        const int g = (t + FT_THREADS * u) & 1023, op = u >> 2;
        const int q4 = 4 * (g & 31);
        pre[u] = ft_row4<VEC>(x, (int)(r0 + (long)ch * GM_KC + (g >> 5)), (int)r1, d, (op ? tj : ti) * FT_T + q4);
      }
    }
  };

  double acc64[2][2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc64[a][b][e] = 0.0;
  ft_f32x16 acc[2][2];
  ft_zero(acc);

  const float* sa = slab + l.hh * GM_LD + l.wq * 64 + l.r32;                         // slab[2 s + hh][feature of the lane's row]
  const float* sb = slab + (diag ? 0 : GM_SLAB) + l.hh * GM_LD + l.wc * 64 + l.r32;  // ... of the lane's column

  fetch(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < nu) {
        const int g = (t + FT_THREADS * u) & 1023, q4 = 4 * (g & 31);
        *reinterpret_cast<float4*>(slab + (u >> 2) * GM_SLAB + (g >> 5) * GM_LD + q4) =
            gm_centre4<SCALED>(pre[u], r0 + (long)ch * GM_KC + (g >> 5) < r1, &mu[u >> 2][q4], qpre[u & 3]);
      }
    }
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
#pragma unroll
    for (int p8 = 0; p8 < GM_KC / 8; ++p8) {  // eight rows: four MFMA steps of two rows
      float a0[4], a1[4], b0[4], b1[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int o = (8 * p8 + 2 * s) * GM_LD;
        a0[s] = sa[o], a1[s] = sa[o + 32], b0[s] = sb[o], b1[s] = sb[o + 32];
      }
      ft_mma_step(acc, make_float4(a0[0], a0[1], a0[2], a0[3]), make_float4(a1[0], a1[1], a1[2], a1[3]), b0, b1);
    }
    if ((ch + 1) % (GM_R / GM_KC) == 0 || ch + 1 == nch) {  // the block's fp32 sum goes to float64, blocks in ascending order
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc64[a][b][e] += (double)acc[a][b][e];
      ft_zero(acc);
    }
  }

  double* dst = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(FT_T * FT_T);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[ft_row(l, a, e) * FT_T + l.wc * 64 + b * 32 + l.r32] = acc64[a][b][e];
}

// gram[j][l] = gram[l][j] = the splits' tiles in split order; of a diagonal tile only j <= l is read, so both triangles hold the
// same bits.  grid (tile pairs, 64): 256 elements of the tile per workgroup
__global__ __launch_bounds__(256) void pca_gram_fold_kernel(const double* __restrict__ ws, int splits, int pairs, int tiles, int d,
                                                            double* __restrict__ gram) {
  int ti = 0, p = blockIdx.x;
  while (p >= tiles - ti) p -= tiles - ti, ++ti;
  const int tj = ti + p;
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int row = e >> 7, col = e & 127;
  const int gj = ti * FT_T + row, gl = tj * FT_T + col;
  if (gj >= d || gl >= d || (ti == tj && row > col)) return;
  double tot = 0.0;
  for (int s = 0; s < splits; ++s) tot += ws[((size_t)s * pairs + blockIdx.x) * (size_t)(FT_T * FT_T) + e];
  gram[(size_t)gj * d + gl] = tot;
  gram[(size_t)gl * d + gj] = tot;
}

// ------------------------------------------------------------------ (c) centred projection on the tile engine
// VEC: d % 4 == 0 and x, w 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(FT_THREADS, 2) void pca_project_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                                    const float* __restrict__ w, int n, int d, int k, float* __restrict__ z) {
  __shared__ __attribute__((aligned(16))) float stage[FT_STAGE];
  const FtLane l = ft_lane();
  const int q0 = blockIdx.x * FT_T, c0 = blockIdx.y * FT_T;
  ft_f32x16 acc[2][2];
  ft_dots(
      acc, stage, l, (d + FT_KC - 1) / FT_KC,
      [&](int operand, int r, int kk) {
        if (operand) return ft_row4<VEC>(w, c0 + r, k, d, kk);
        float4 v = ft_row4<VEC>(x, q0 + r, n, d, kk);
        if (q0 + r < n) {  // the centring: float64 difference, rounded once; features past d and rows past n stay zero
          if (kk < d) v.x = (float)((double)v.x - mean[kk]);
          if (kk + 1 < d) v.y = (float)((double)v.y - mean[kk + 1]);
          if (kk + 2 < d) v.z = (float)((double)v.z - mean[kk + 2]);
          if (kk + 3 < d) v.w = (float)((double)v.w - mean[kk + 3]);
        }
        return v;
      },
      [] {});
  ft_each(acc, l, [&](float dot, int row, int col) {
    const int gi = q0 + row, gc = c0 + col;
    if (gi < n && gc < k) z[(size_t)gi * (size_t)k + (size_t)gc] = dot;
  });
}

// ------------------------------------------------------------------ host
static int pca_shape(const char* who, int64_t n, int64_t d) {
  VSX_CHECK(n >= 2 && n < ((int64_t)1 << 31), "%s: n=%ld must be in [2, 2^31)", who, (long)n);
  VSX_CHECK(d >= 1 && d <= PCA_MAX_D, "%s: d=%ld must be in [1, %d]", who, (long)d, PCA_MAX_D);
  return 0;
}
static bool pca_shape_ok(int64_t n, int64_t d) { return n >= 2 && n < ((int64_t)1 << 31) && d >= 1 && d <= PCA_MAX_D; }

// the Gram pass: splits of whole blocks, at least GM_MIN_BLOCKS each, so that pairs * splits is at most GM_WANT_WGS (or pairs)
static void gm_split(int64_t n, int d, int* tiles, int* pairs, int* splits, int64_t* rps) {
  *tiles = (d + FT_T - 1) / FT_T;
  *pairs = *tiles * (*tiles + 1) / 2;
  const int64_t blocks = (n + GM_R - 1) / GM_R;
  int64_t want = GM_WANT_WGS / *pairs;  // rounded down: one workgroup past a full round of the chip costs a whole round
  if (want < 1) want = 1;
  if (want > GM_MAX_SPLITS) want = GM_MAX_SPLITS;
  int64_t bps = (blocks + want - 1) / want;
  if (bps < GM_MIN_BLOCKS) bps = GM_MIN_BLOCKS;
  *rps = bps * GM_R;
  *splits = (int)((n + *rps - 1) / *rps);
}

extern "C" int64_t vsx_col_moments_ws_bytes(int64_t n, int32_t d) {
  if (!pca_shape_ok(n, d)) return 0;
  int splits;
  int64_t rps;
  cm_split(n, d, &splits, &rps);
  return (int64_t)splits * d * 8;
}

extern "C" int32_t vsx_col_moments(const float* x, int64_t n, int32_t d, double* mean, double* m2, void* ws, int64_t ws_bytes,
                                   vsx_stream_t stream) {
  if (int rc = pca_shape("vsx_col_moments", n, d)) return rc;
  VSX_CHECK(x && mean && m2 && ws, "vsx_col_moments: null argument");
  VSX_CHECK(((uintptr_t)x & 3) == 0 && (((uintptr_t)mean | (uintptr_t)m2 | (uintptr_t)ws) & 7) == 0,
            "vsx_col_moments: x must be 4-byte aligned, mean, m2 and ws 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_col_moments_ws_bytes(n, d), "vsx_col_moments: the workspace must hold vsx_col_moments_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_col_moments_ws_bytes(n, d), (long)ws_bytes);
  int splits;
  int64_t rps;
  cm_split(n, d, &splits, &rps);
  VSX_CHECK(splits <= 65535, "vsx_col_moments: %d row splits", splits);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((d + CM_COLS - 1) / CM_COLS), (unsigned)splits), block(CM_COLS * CM_LANES), fgrid((unsigned)((d + 255) / 256));
  double* part = (double*)ws;
  hipLaunchKernelGGL(pca_moment_kernel<0>, grid, block, 0, s, x, (const double*)nullptr, (long)n, d, (long)rps, part);
  hipLaunchKernelGGL(cm_fold_kernel, fgrid, dim3(256), 0, s, (const double*)part, splits, d, (double)n, mean);
  hipLaunchKernelGGL(pca_moment_kernel<1>, grid, block, 0, s, x, (const double*)mean, (long)n, d, (long)rps, part);
  hipLaunchKernelGGL(cm_fold_kernel, fgrid, dim3(256), 0, s, (const double*)part, splits, d, 0.0, m2);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_gram_rows_per_split(int64_t n, int32_t d) {
  if (!pca_shape_ok(n, d)) return 0;
  int tiles, pairs, splits;
  int64_t rps;
  gm_split(n, d, &tiles, &pairs, &splits, &rps);
  return rps;
}

extern "C" int64_t vsx_gram_ws_bytes(int64_t n, int32_t d) {
  if (!pca_shape_ok(n, d)) return 0;
  int tiles, pairs, splits;
  int64_t rps;
  gm_split(n, d, &tiles, &pairs, &splits, &rps);
  return (int64_t)splits * pairs * FT_T * FT_T * 8;
}

// the Gram pass and its fold; q: the row scales of vsx_gram_scaled, null for vsx_gram_centered
static int gm_launch(const char* who, const float* x, int64_t n, int32_t d, const double* mean, const float* q, double* gram, void* ws,
                     int64_t ws_bytes, vsx_stream_t stream) {
  if (int rc = pca_shape(who, n, d)) return rc;
  VSX_CHECK(x && (mean || q) && gram && ws, "%s: null argument", who);
  VSX_CHECK((((uintptr_t)x | (uintptr_t)q) & 3) == 0 && (((uintptr_t)mean | (uintptr_t)gram | (uintptr_t)ws) & 7) == 0,
            "%s: x%s must be 4-byte aligned, mean, gram and ws 8-byte aligned", who, q ? " and q" : "");
  VSX_CHECK(ws_bytes >= vsx_gram_ws_bytes(n, d), "%s: the workspace must hold vsx_gram_ws_bytes = %ld bytes (got %ld)", who,
            (long)vsx_gram_ws_bytes(n, d), (long)ws_bytes);
  int tiles, pairs, splits;
  int64_t rps;
  gm_split(n, d, &tiles, &pairs, &splits, &rps);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)pairs, (unsigned)splits), block(FT_THREADS);
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    vsx_by_bool(q != nullptr, [&](auto scaled) {
      hipLaunchKernelGGL((pca_gram_kernel<decltype(vec)::value, decltype(scaled)::value>), grid, block, 0, s, x, mean, q, (long)n, d, tiles,
                         (long)rps, (double*)ws);
    });
  });
  hipLaunchKernelGGL(pca_gram_fold_kernel, dim3((unsigned)pairs, FT_T * FT_T / 256), dim3(256), 0, s, (const double*)ws, splits, pairs, tiles, d,
                     gram);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_gram_centered(const float* x, int64_t n, int32_t d, const double* mean, double* gram, void* ws, int64_t ws_bytes,
                                     vsx_stream_t stream) {
  VSX_CHECK(mean, "vsx_gram_centered: null argument");
  return gm_launch("vsx_gram_centered", x, n, d, mean, nullptr, gram, ws, ws_bytes, stream);
}

extern "C" int32_t vsx_gram_scaled(const float* x, int64_t n, int32_t d, const double* mean, const float* q, double* gram, void* ws,
                                   int64_t ws_bytes, vsx_stream_t stream) {
  VSX_CHECK(q, "vsx_gram_scaled: null argument");
  return gm_launch("vsx_gram_scaled", x, n, d, mean, q, gram, ws, ws_bytes, stream);
}

extern "C" int32_t vsx_center_project(const float* x, int64_t n, int32_t d, const double* mean, const float* w, int32_t k, float* z,
                                      vsx_stream_t stream) {
  if (int rc = pca_shape("vsx_center_project", n, d)) return rc;
  VSX_CHECK(k >= 1 && k <= 65535 * FT_T, "vsx_center_project: k=%ld must be in [1, %d]", (long)k, 65535 * FT_T);
  VSX_CHECK(x && mean && w && z, "vsx_center_project: null argument");
  VSX_CHECK((((uintptr_t)x | (uintptr_t)w | (uintptr_t)z) & 3) == 0 && ((uintptr_t)mean & 7) == 0,
            "vsx_center_project: x, w and z must be 4-byte aligned, mean 8-byte aligned");
  const dim3 grid((unsigned)((n + FT_T - 1) / FT_T), (unsigned)((k + FT_T - 1) / FT_T)), block(FT_THREADS);
  hipStream_t s = (hipStream_t)stream;
  vsx_by_bool(ft_vec_ok(x, d) && vsx_al16(w), [&](auto vec) {
    hipLaunchKernelGGL(pca_project_kernel<decltype(vec)::value>, grid, block, 0, s, x, mean, w, (int)n, d, k, z);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}
