// viscy_amd — the data passes of a Newton iteration on the weighted logistic objective (viscy_utils/evaluation/linear_classifier.py:
// sklearn LogisticRegression on frozen embeddings) over x [n, d] fp32 row-major, 2 <= n < 2^31 rows, d <= 4096 features.  The
// third pass, the row-scaled Gram of the Hessian, is vsx_gram_scaled of pca.hip; what is left is a (d + 1)^2 problem for the host.
//
//   vsx_logreg_rows   z_i = b + sum_j x_ij w_j;  loss, r_i = dloss/dz, s_i = d2loss/dz2, q_i = fl32(sqrt(s_i));  {sum loss, sum r, sum s}
//   vsx_wcolsum       out_kj = sum_i v_ki x_ij     float64, x read once for all k <= 4
//
// No atomics: workgroups write partials to workspace rows that are theirs alone and a second kernel folds them in a fixed order, so
// every output is a pure function of the inputs, bit-identical from run to run.
//
// The row pass.  A workgroup of four waves owns one contiguous run of rows, a wave a quarter of it, and w is kept in LDS.  The
// whole wave forms one row's dot at a time: lane l holds features 4 l .. 4 l + 3, 256 + 4 l .., one float4 load each where VEC
// (ft_row4); the scalar loads of an unaligned x or of d % 4 != 0 fetch the same features into the same lanes, so the dot has ONE
// order: per lane fma over ascending features from 0, the lanes added by the xor butterfly 32, 16, .. 1, then b added last.  After
// 64 rows lane l keeps the margin of row l of the batch and the float64 part after the dot (exp, log1p, the divisions, the square
// root) runs once per row, one row per lane, with coalesced stores.  Everything after the loads is float64.
#include "col_split.h"
#include "f32_tile.h"
#include "../../include/vsx.h"

#define LR_MAX_D VSX_PCA_MAX_D
#define LR_WAVES 4
#define LR_WANT_WGS 2048     // eight workgroups per compute unit
#define LR_MIN_ROWS 16       // rows per workgroup at least: w is staged once for them

// FULL: labels, loss and derivatives; else the margins alone.  part [workgroup][3] = the run's {sum loss, sum r, sum s}: lane l of
// a wave adds rows l, 64 + l, .. of the wave's run in ascending order, the lanes are added by the butterfly, the waves 0 .. 3
template <bool VEC, bool FULL>
__global__ __launch_bounds__(LR_WAVES * 64) void lr_rows_kernel(const float* __restrict__ x, const double* __restrict__ w, double b,
                                                                const int* __restrict__ labels, int pos, double cp, double cn, int n, int d,
                                                                int rows_per_wg, double* __restrict__ z, double* __restrict__ r,
                                                                double* __restrict__ s, float* __restrict__ q, double* __restrict__ part) {
  extern __shared__ double lr_w[];  // [d]
  __shared__ double red[3][LR_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < d; j += LR_WAVES * 64) lr_w[j] = w[j];
  __syncthreads();

  const int rows_per_wave = rows_per_wg / LR_WAVES;  // rows_per_wg is a multiple of LR_WAVES
  const long w0 = (long)blockIdx.x * rows_per_wg + (long)wave * rows_per_wave;
  const int w1 = (int)min(w0 + rows_per_wave, (long)n);
  double t_loss = 0.0, t_r = 0.0, t_s = 0.0;
  for (long base = w0; base < w1; base += 64) {
    const int cnt = min(64, w1 - (int)base);
    double zi = 0.0;  // the margin of row base + lane
    for (int j = 0; j < cnt; ++j) {
      const int row = (int)base + j;
      double acc = 0.0;
      for (int c = 4 * lane; c < d; c += 256) {
        const float4 v = ft_row4<VEC>(x, row, n, d, c);
        acc = fma((double)v.x, lr_w[c], acc);
        if (VEC || c + 1 < d) acc = fma((double)v.y, lr_w[c + 1], acc);
        if (VEC || c + 2 < d) acc = fma((double)v.z, lr_w[c + 2], acc);
        if (VEC || c + 3 < d) acc = fma((double)v.w, lr_w[c + 3], acc);
      }
      const double dot = wave_sum_f64(acc) + b;
      if (lane == j) zi = dot;
    }
    if (lane < cnt) {
      const int row = (int)base + lane;
      if (z) z[row] = zi;
      if (FULL) {
        const bool is_pos = labels[row] == pos;
        const double y = is_pos ? 1.0 : -1.0, c = is_pos ? cp : cn;
        const double m = y * zi;
        const double e = exp(-fabs(m));
        const double den = 1.0 + e;
        const double big = 1.0 / den, small = e / den;  // sigma and 1 - sigma, whichever way round: no 1 - x anywhere
        const double sig = m >= 0.0 ? big : small, om = m >= 0.0 ? small : big;
        const double li = c * (log1p(e) + fmax(-m, 0.0));
        const double ri = -c * y * om;
        const double si = c * sig * om;
        t_loss += li, t_r += ri, t_s += si;
        if (r) r[row] = ri;
        if (s) s[row] = si;
        if (q) q[row] = (float)sqrt(si);
      }
    }
  }
  if (FULL && part) {
    t_loss = wave_sum_f64(t_loss), t_r = wave_sum_f64(t_r), t_s = wave_sum_f64(t_s);
    if (lane == 0) red[0][wave] = t_loss, red[1][wave] = t_r, red[2][wave] = t_s;
    __syncthreads();
    if (threadIdx.x < 3) {
      double tot = red[threadIdx.x][0];
      for (int k = 1; k < LR_WAVES; ++k) tot += red[threadIdx.x][k];
      part[(size_t)blockIdx.x * 3 + threadIdx.x] = tot;
    }
  }
}

// sums[k] = the workgroups' partials: lane l of wave k adds workgroups l, l + 64, .. in ascending order, then the xor butterfly.
// one workgroup of 192
__global__ __launch_bounds__(192) void lr_sums_fold_kernel(const double* __restrict__ part, int wgs, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  double tot = 0.0;
  for (int g = lane; g < wgs; g += 64) tot += part[(size_t)g * 3 + k];
  tot = wave_sum_f64(tot);
  if (lane == 0) sums[k] = tot;
}

// the split of pca_moment_kernel: thread (column lane, row lane) adds rows r0 + lane, r0 + lane + 4, ... with fma in float64, the
// four row lanes are folded 0 .. 3; part[split][k][column].  All column lanes read the same v[k][row]: one broadcast load
template <int M>
__global__ __launch_bounds__(CM_COLS * CM_LANES) void lr_wcolsum_kernel(const float* __restrict__ x, const double* __restrict__ v, long n, int d,
                                                                        long rows_per_split, double* __restrict__ part) {
  __shared__ double red[M][CM_LANES][CM_COLS];
  const int cl = threadIdx.x & (CM_COLS - 1), rl = threadIdx.x / CM_COLS;
  const int col = blockIdx.x * CM_COLS + cl;
  const long r0 = (long)blockIdx.y * rows_per_split;
  const long r1 = min(r0 + rows_per_split, n);
  double acc[M];
#pragma unroll
  for (int k = 0; k < M; ++k) acc[k] = 0.0;
  if (col < d) {
    const float* p = x + (size_t)col;
#pragma unroll 4
    for (long i = r0 + rl; i < r1; i += CM_LANES) {
      const double xv = (double)p[(size_t)i * (size_t)d];
#pragma unroll
      for (int k = 0; k < M; ++k) acc[k] = fma(v[(size_t)k * (size_t)n + (size_t)i], xv, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < M; ++k) red[k][rl][cl] = acc[k];
  __syncthreads();
  if (rl == 0 && col < d) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
      double tot = red[k][0][cl];
      for (int u = 1; u < CM_LANES; ++u) tot += red[k][u][cl];
      part[((size_t)blockIdx.y * M + k) * d + col] = tot;
    }
  }
}

// ------------------------------------------------------------------ host
static bool lr_shape_ok(int64_t n, int64_t d) { return n >= 2 && n < ((int64_t)1 << 31) && d >= 1 && d <= LR_MAX_D; }
static int lr_shape(const char* who, int64_t n, int64_t d) {
  VSX_CHECK(n >= 2 && n < ((int64_t)1 << 31), "%s: n=%ld must be in [2, 2^31)", who, (long)n);
  VSX_CHECK(d >= 1 && d <= LR_MAX_D, "%s: d=%ld must be in [1, %d]", who, (long)d, LR_MAX_D);
  return 0;
}
// runs of whole groups of LR_WAVES rows, at least LR_MIN_ROWS, about LR_WANT_WGS workgroups
static void lr_rows_split(int64_t n, int* wgs, int* rows_per_wg) {
  int64_t rpw = (n + LR_WANT_WGS - 1) / LR_WANT_WGS;
  if (rpw < LR_MIN_ROWS) rpw = LR_MIN_ROWS;
  rpw = (rpw + LR_WAVES - 1) / LR_WAVES * LR_WAVES;
  *rows_per_wg = (int)rpw;
  *wgs = (int)((n + rpw - 1) / rpw);
}

extern "C" int64_t vsx_logreg_rows_ws_bytes(int64_t n, int32_t d) {
  if (!lr_shape_ok(n, d)) return 0;
  int wgs, rpw;
  lr_rows_split(n, &wgs, &rpw);
  return (int64_t)wgs * 3 * 8;
}

extern "C" int32_t vsx_logreg_rows(const float* x, int64_t n, int32_t d, const double* w, double b, const int32_t* labels, int32_t pos,
                                   double cp, double cn, double* z, double* r, double* s, float* q, double* sums, void* ws, int64_t ws_bytes,
                                   vsx_stream_t stream) {
  if (int rc = lr_shape("vsx_logreg_rows", n, d)) return rc;
  const bool full = r || s || q || sums;
  VSX_CHECK(x && w && (full || z), "vsx_logreg_rows: null argument");
  VSX_CHECK(!full || labels, "vsx_logreg_rows: labels are needed for anything but the margins");
  VSX_CHECK(!sums || ws, "vsx_logreg_rows: the sums need a workspace");
  VSX_CHECK((((uintptr_t)x | (uintptr_t)labels | (uintptr_t)q) & 3) == 0, "vsx_logreg_rows: x, labels and q must be 4-byte aligned");
  VSX_CHECK((((uintptr_t)w | (uintptr_t)z | (uintptr_t)r | (uintptr_t)s | (uintptr_t)sums | (uintptr_t)ws) & 7) == 0,
            "vsx_logreg_rows: w, z, r, s, sums and ws must be 8-byte aligned");
  VSX_CHECK(!sums || ws_bytes >= vsx_logreg_rows_ws_bytes(n, d),
            "vsx_logreg_rows: the workspace must hold vsx_logreg_rows_ws_bytes = %ld bytes (got %ld)", (long)vsx_logreg_rows_ws_bytes(n, d),
            (long)ws_bytes);
  int wgs, rpw;
  lr_rows_split(n, &wgs, &rpw);
  hipStream_t st = (hipStream_t)stream;
  double* part = sums ? (double*)ws : nullptr;
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    vsx_by_bool(full, [&](auto full_) {
      hipLaunchKernelGGL((lr_rows_kernel<decltype(vec)::value, decltype(full_)::value>), dim3((unsigned)wgs), dim3(LR_WAVES * 64),
                         (size_t)d * sizeof(double), st, x, w, b, labels, pos, cp, cn, (int)n, d, rpw, z, r, s, q, part);
    });
  });
  if (sums) hipLaunchKernelGGL(lr_sums_fold_kernel, dim3(1), dim3(192), 0, st, (const double*)part, wgs, sums);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_wcolsum_ws_bytes(int64_t n, int32_t d, int32_t m) {
  if (!lr_shape_ok(n, d) || m < 1 || m > 4) return 0;
  int splits;
  int64_t rps;
  cm_split(n, d, &splits, &rps);
  return (int64_t)splits * m * d * 8;
}

extern "C" int32_t vsx_wcolsum(const float* x, int64_t n, int32_t d, const double* v, int32_t m, double* out, void* ws, int64_t ws_bytes,
                               vsx_stream_t stream) {
  if (int rc = lr_shape("vsx_wcolsum", n, d)) return rc;
  VSX_CHECK(m >= 1 && m <= 4, "vsx_wcolsum: m=%ld must be in [1, 4]", (long)m);
  VSX_CHECK(x && v && out && ws, "vsx_wcolsum: null argument");
  VSX_CHECK(((uintptr_t)x & 3) == 0 && (((uintptr_t)v | (uintptr_t)out | (uintptr_t)ws) & 7) == 0,
            "vsx_wcolsum: x must be 4-byte aligned, v, out and ws 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_wcolsum_ws_bytes(n, d, m), "vsx_wcolsum: the workspace must hold vsx_wcolsum_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_wcolsum_ws_bytes(n, d, m), (long)ws_bytes);
  int splits;
  int64_t rps;
  cm_split(n, d, &splits, &rps);
  VSX_CHECK(splits <= 65535, "vsx_wcolsum: %d row splits", splits);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((d + CM_COLS - 1) / CM_COLS), (unsigned)splits), block(CM_COLS * CM_LANES);
  double* part = (double*)ws;
  vsx_by_int<1, 2, 3, 4>(m, [&](auto m_) {
    hipLaunchKernelGGL(lr_wcolsum_kernel<decltype(m_)::value>, grid, block, 0, st, x, v, (long)n, d, (long)rps, part);
  });
  hipLaunchKernelGGL(cm_fold_kernel, dim3((unsigned)((m * d + 255) / 256)), dim3(256), 0, st, (const double*)part, splits, m * d, 0.0, out);
  VSX_LAUNCH_CHECK();
  return 0;
}
