// viscy_amd — the device passes of the temporal-smoothness evaluation (viscy_utils/evaluation/smoothness.py
// compute_embeddings_smoothness, viscy_utils/evaluation/distance.py compute_track_displacement): sklearn's standard scaling of a
// float32 matrix, float64 distances of listed row pairs, and the unnormalised Gaussian kernel-density sum on a grid.
//
//   vsx_standardize   z_ij = fl32(double(fl32(double(x_ij) - mean_j)) / scale_j)              elementwise, may run in place
//   vsx_pair_dist     out_p = cosine or Euclidean distance of rows pi[p], pj[p]               one wave per pair, float64
//   vsx_kde_gauss     out_g = sum_i exp(-a (grid_g - data_i)^2)                               float64, library exp
//
// No atomics.  Every output is a pure function of the inputs, bit-identical from run to run: the pair pass has ONE summation order
// (vsx_logreg_rows': lane l takes features 4 l .. 4 l + 3, 256 + 4 l .., ascending; the 64 lanes are added by the xor butterfly
// 32 .. 1) whatever the alignment, and the density pass splits the data into chunks whose length and count depend on (n, m) alone,
// writes one partial per (chunk, grid point) to the workspace and folds them in ascending chunk order.
#include "f32_tile.h"
#include "../../include/vsx.h"

#define SM_WAVES 4
#define SM_PAIR_MAX_WGS (1 << 20)  // the pair pass strides over the list past this many workgroups
#define KD_THREADS 256
#define KD_GP 2                    // grid points a thread keeps in registers
#define KD_TILE VSX_KDE_TILE       // grid points of a workgroup
#define KD_CHUNK VSX_KDE_CHUNK     // shortest chunk of data; also the slab staged in LDS at a time
#define KD_WANT_WGS 2048           // eight workgroups per compute unit
static_assert(KD_TILE == KD_THREADS * KD_GP, "a workgroup's grid tile is its threads' registers");

// acc + (u - v)^2 with the difference, the square and the add each rounded once.  The __dmul_rn / __dadd_rn of this toolchain are
// plain operators, which the compiler's default contraction would fuse into one fma: the pragma is what keeps them apart
__device__ __forceinline__ double sm_add_sqdiff(double acc, double u, double v) {
#pragma clang fp contract(off)
  const double diff = u - v;
  const double sq = diff * diff;
  return acc + sq;
}

// ------------------------------------------------------------------ standardize
// block = cx column lanes x (256 / cx) row lanes, cx = the power of two >= d, at most 256; a thread walks its columns c, c + cx, ..
__global__ __launch_bounds__(256) void sm_standardize_kernel(const float* x, const double* __restrict__ mean, const double* __restrict__ scale,
                                                             float* z, long n, int d, int cx) {
  const int c0 = threadIdx.x % cx, rl = threadIdx.x / cx, ry = 256 / cx;
  for (long row = (long)blockIdx.x * ry + rl; row < n; row += (long)gridDim.x * ry) {
    const size_t base = (size_t)row * (size_t)d;
    for (int c = c0; c < d; c += cx) {
      const float centred = (float)((double)x[base + c] - mean[c]);
      z[base + c] = (float)((double)centred / scale[c]);
    }
  }
}

// ------------------------------------------------------------------ pair distances
// METRIC 0 cosine, 1 Euclidean.  A row index outside [0, n) never reaches memory: the pair's distance is NaN
template <bool VEC, int METRIC>
__global__ __launch_bounds__(SM_WAVES * 64) void sm_pair_kernel(const float* __restrict__ x, const int* __restrict__ pi, const int* __restrict__ pj,
                                                                long P, int n, int d, double eps, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long p = (long)blockIdx.x * SM_WAVES + wave; p < P; p += (long)gridDim.x * SM_WAVES) {
    const int i = pi[p], j = pj[p];
    if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) {  // uniform over the wave
      if (lane == 0) out[p] = __longlong_as_double(0x7ff8000000000000LL);
      continue;
    }
    double uv = 0.0, uu = 0.0, vv = 0.0;
    for (int c = 4 * lane; c < d; c += 256) {
      const float4 a = ft_row4<VEC>(x, i, n, d, c), b = ft_row4<VEC>(x, j, n, d, c);
      const float ua[4] = {a.x, a.y, a.z, a.w}, vb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (VEC || c + k < d) {
          const double u = (double)ua[k], v = (double)vb[k];
          if (METRIC == 0) {
            uv = fma(u, v, uv), uu = fma(u, u, uu), vv = fma(v, v, vv);  // fp32 x fp32 is exact in float64: fma = mul, add
          } else {
            uu = sm_add_sqdiff(uu, u, v);
          }
        }
      }
    }
    uu = wave_sum_f64(uu);
    if (METRIC == 0) uv = wave_sum_f64(uv), vv = wave_sum_f64(vv);
    if (lane == 0) {
      if (METRIC == 0) {
        const double nu = fmax(sqrt(uu), eps), nv = fmax(sqrt(vv), eps);
        out[p] = 1.0 - uv / (nu * nv);  // a product, a division, a difference: nothing here can contract
      } else {
        out[p] = sqrt(uu);
      }
    }
  }
}

// ------------------------------------------------------------------ Gaussian kernel-density sums
// Workgroup (tile, chunk): thread t keeps grid points tile * KD_TILE + t + 256 k in registers, the chunk's data pass through LDS in
// slabs of KD_CHUNK, read back as broadcasts; a thread adds its chunk in ascending i.  part [chunks][m]
__global__ __launch_bounds__(KD_THREADS) void kd_partial_kernel(const double* __restrict__ data, long n, const double* __restrict__ grid, int m,
                                                                double a, long chunk_len, double* __restrict__ part) {
  __shared__ double slab[KD_CHUNK];
  const int t = threadIdx.x;
  double g[KD_GP], acc[KD_GP];
#pragma unroll
  for (int k = 0; k < KD_GP; ++k) {
    const int gi = blockIdx.x * KD_TILE + t + KD_THREADS * k;
    g[k] = gi < m ? grid[gi] : 0.0;
    acc[k] = 0.0;
  }
  const long c0 = (long)blockIdx.y * chunk_len;
  const long c1 = min(c0 + chunk_len, n);
  for (long base = c0; base < c1; base += KD_CHUNK) {
    const int cnt = (int)min((long)KD_CHUNK, c1 - base);
    __syncthreads();
    for (int i = t; i < cnt; i += KD_THREADS) slab[i] = data[base + i];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const double xi = slab[i];
#pragma unroll
      for (int k = 0; k < KD_GP; ++k) {
        const double dlt = g[k] - xi;
        acc[k] += exp(-(a * (dlt * dlt)));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KD_GP; ++k) {
    const int gi = blockIdx.x * KD_TILE + t + KD_THREADS * k;
    if (gi < m) part[(size_t)blockIdx.y * (size_t)m + gi] = acc[k];
  }
}

// out_g = the chunks' partials in ascending chunk order
__global__ __launch_bounds__(256) void kd_fold_kernel(const double* __restrict__ part, int chunks, int m, double* __restrict__ out) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi >= m) return;
  double tot = part[gi];
  for (int c = 1; c < chunks; ++c) tot += part[(size_t)c * (size_t)m + gi];
  out[gi] = tot;
}

// ------------------------------------------------------------------ host
extern "C" int32_t vsx_standardize(const float* x, const double* mean, const double* scale, float* z, int64_t n, int32_t d,
                                   vsx_stream_t stream) {
  VSX_CHECK(n >= 1 && d >= 1, "vsx_standardize: n=%ld, d=%ld must be at least 1", (long)n, (long)d);
  VSX_CHECK(x && mean && scale && z, "vsx_standardize: null argument");
  VSX_CHECK((((uintptr_t)x | (uintptr_t)z) & 3) == 0 && (((uintptr_t)mean | (uintptr_t)scale) & 7) == 0,
            "vsx_standardize: x and z must be 4-byte aligned, mean and scale 8-byte aligned");
  int cx = 1;
  while (cx < d && cx < 256) cx <<= 1;
  const int ry = 256 / cx;
  const long want = (n + ry - 1) / ry;
  const unsigned wgs = (unsigned)(want < 65536 ? want : 65536);
  hipLaunchKernelGGL(sm_standardize_kernel, dim3(wgs), dim3(256), 0, (hipStream_t)stream, x, mean, scale, z, (long)n, d, cx);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_pair_dist(const float* x, int32_t n, const int32_t* pi, const int32_t* pj, int64_t P, int32_t d, int32_t metric,
                                 double eps, double* out, vsx_stream_t stream) {
  VSX_CHECK(P >= 1 && P < ((int64_t)1 << 33), "vsx_pair_dist: P=%ld must be in [1, 2^33)", (long)P);
  VSX_CHECK(n >= 1 && d >= 1, "vsx_pair_dist: n=%ld, d=%ld must be at least 1", (long)n, (long)d);
  VSX_CHECK(metric == VSX_PAIR_COSINE || metric == VSX_PAIR_EUCLIDEAN, "vsx_pair_dist: metric=%ld must be 0 (cosine) or 1 (Euclidean)", (long)metric);
  VSX_CHECK(eps >= 0.0, "vsx_pair_dist: eps must be >= 0 and not NaN");
  VSX_CHECK(x && pi && pj && out, "vsx_pair_dist: null argument");
  VSX_CHECK((((uintptr_t)x | (uintptr_t)pi | (uintptr_t)pj) & 3) == 0 && ((uintptr_t)out & 7) == 0,
            "vsx_pair_dist: x, pi and pj must be 4-byte aligned, out 8-byte aligned");
  const int64_t want = (P + SM_WAVES - 1) / SM_WAVES;
  const unsigned wgs = (unsigned)(want < SM_PAIR_MAX_WGS ? want : SM_PAIR_MAX_WGS);
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    vsx_by_int<0, 1>(metric, [&](auto metric_) {
      hipLaunchKernelGGL((sm_pair_kernel<decltype(vec)::value, decltype(metric_)::value>), dim3(wgs), dim3(SM_WAVES * 64), 0, (hipStream_t)stream,
                         x, pi, pj, (long)P, n, d, eps, out);
    });
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

static bool kd_shape_ok(int64_t n, int64_t m) { return n >= 1 && n < ((int64_t)1 << 31) && m >= 1 && m <= ((int64_t)1 << 20); }
// chunks of whole slabs, as many as give about KD_WANT_WGS workgroups over all grid tiles: a function of (n, m) alone
static void kd_split(int64_t n, int64_t m, int* tiles, int* chunks, int64_t* chunk_len) {
  *tiles = (int)((m + KD_TILE - 1) / KD_TILE);
  int64_t want = KD_WANT_WGS / *tiles;
  if (want < 1) want = 1;
  const int64_t slabs = (n + KD_CHUNK - 1) / KD_CHUNK;
  if (want > slabs) want = slabs;
  *chunk_len = (slabs + want - 1) / want * KD_CHUNK;
  *chunks = (int)((n + *chunk_len - 1) / *chunk_len);
}

extern "C" int64_t vsx_kde_gauss_ws_bytes(int64_t n, int64_t m) {
  if (!kd_shape_ok(n, m)) return 0;
  int tiles, chunks;
  int64_t len;
  kd_split(n, m, &tiles, &chunks, &len);
  return (int64_t)chunks * m * 8;
}

extern "C" int32_t vsx_kde_gauss(const double* data, int64_t n, const double* grid, int64_t m, double a, double* out, void* ws, int64_t ws_bytes,
                                 vsx_stream_t stream) {
  VSX_CHECK(n >= 1 && n < ((int64_t)1 << 31), "vsx_kde_gauss: n=%ld must be in [1, 2^31)", (long)n);
  VSX_CHECK(m >= 1 && m <= ((int64_t)1 << 20), "vsx_kde_gauss: m=%ld must be in [1, 2^20]", (long)m);
  VSX_CHECK(data && grid && out && ws, "vsx_kde_gauss: null argument");
  VSX_CHECK((((uintptr_t)data | (uintptr_t)grid | (uintptr_t)out | (uintptr_t)ws) & 7) == 0, "vsx_kde_gauss: data, grid, out and ws must be 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_kde_gauss_ws_bytes(n, m), "vsx_kde_gauss: the workspace must hold vsx_kde_gauss_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_kde_gauss_ws_bytes(n, m), (long)ws_bytes);
  int tiles, chunks;
  int64_t len;
  kd_split(n, m, &tiles, &chunks, &len);
  VSX_CHECK(chunks <= 65535, "vsx_kde_gauss: %d chunks", chunks);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  hipLaunchKernelGGL(kd_partial_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(KD_THREADS), 0, st, data, (long)n, grid, (int)m, a, (long)len, part);
  hipLaunchKernelGGL(kd_fold_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const double*)part, chunks, (int)m, out);
  VSX_LAUNCH_CHECK();
  return 0;
}
