// viscy_amd — the device passes of the clustering evaluation (viscy_utils/evaluation/clustering.py: pairwise_distance_matrix,
// dbscan_clustering, knn_accuracy) on the float64 tile engine of f64_tile.h.
//
//   vsx_row_sqnorm_f64   norms[i] = dot_ii, the diagonal of a tile whose two operands are the same rows
//   vsx_pdist_f64        a block of the float64 cosine / Euclidean / squared Euclidean distance matrix
//   vsx_eps_graph        the eps-neighbourhood graph as a bit matrix (ballots, ordinary stores) and its row popcounts
//   vsx_cc_round         one round of minimum-label hooking over core-core edges plus pointer jumping
//   vsx_dbscan_finish    cluster numbers of core rows, border rows (smallest number among their core neighbours) and noise
//
// No kernel waits on another workgroup, every loop has a bound known at launch, there are no floating-point atomics (and no
// integer ones).  The labels of a round are updated in place by plain 4-byte stores: a reader sees a row's old or new label, both
// of which name a core row of the same component and are never smaller than the component's smallest core index, so the fixed
// point (every core row carries that smallest index) does not depend on scheduling.
#include "f64_tile.h"

#define CL_WAVES 4

// the epilogue's value from a dot and the two rows' side values (squared norms; for the cosine their clamped inverse roots).
// Every operation is rounded on its own: with contraction on, 1 - dot * p and s - 2 dot would each become one fma
template <int METRIC>
__device__ __forceinline__ double cl_value(double dot, double a, double b, bool diag) {
#pragma clang fp contract(off)
  if (diag) return 0.0;
  if (METRIC == VSX_PDIST_COSINE) {
    const double scale = a * b;  // commutative: d_ij == d_ji
    const double sim = dot * scale;
    return 1.0 - sim;
  }
  const double s = a + b;
  const double twice = 2.0 * dot;
  const double d2 = fmax(s - twice, 0.0);
  return METRIC == VSX_PDIST_EUCLIDEAN ? sqrt(d2) : d2;
}
// inv = 1 / max(sqrt(n), 1e-12): F.normalize's rule
__device__ __forceinline__ double cl_inv_norm(double n) { return 1.0 / fmax(sqrt(n), 1e-12); }

// MODE 0 .. 2: the metric of a distance block; CL_NORMS: the diagonal dots of rows r0 .. r1 - 1 to out[i]
#define CL_NORMS 3
template <bool VEC, int MODE>
__global__ __launch_bounds__(DT_THREADS) void cl_pdist_kernel(const float* __restrict__ x, const double* __restrict__ norms, int d, int r0, int r1,
                                                              int c0, int c1, double* __restrict__ out, size_t ld) {
  __shared__ __align__(16) double stage[DT_STAGE];
  __shared__ double side[2][DT_T];
  const DtLane l = dt_lane();
  const int i0 = r0 + (int)blockIdx.y * DT_T;
  const int j0 = MODE == CL_NORMS ? i0 : c0 + (int)blockIdx.x * DT_T;
  if (MODE != CL_NORMS && l.t < 2 * DT_T) {
    const int op = l.t >> 6, row = (op ? j0 : i0) + (l.t & 63);
    const double n = row < (op ? c1 : r1) ? norms[row] : 0.0;
    side[op][l.t & 63] = MODE == VSX_PDIST_COSINE ? cl_inv_norm(n) : n;
  }
  dt_f64x4 acc[2][2];
  dt_dots(acc, stage, l, (d + DT_KC - 1) / DT_KC,
          [&](int op, int row, int kk) { return ft_row4<VEC>(x, (op ? j0 : i0) + row, op ? c1 : r1, d, kk); });
  dt_each(acc, l, [&](double dot, int r, int c) {
    const int i = i0 + r, j = j0 + c;
    if (MODE == CL_NORMS) {
      if (r == c && i < r1) out[i] = dot;
    } else if (i < r1 && j < c1) {
      out[(size_t)(i - r0) * ld + (size_t)(j - c0)] = cl_value<MODE>(dot, side[0][r], side[1][c], i == j);
    }
  });
}

// workgroup (word w = blockIdx.x, row tile blockIdx.y): the 64 x 64 predicates j < N && (i == j || d2_ij <= eps2) go to LDS as
// bytes; wave v then turns rows 16 v .. 16 v + 15 into one ballot each, lane r keeps the word of row 16 v + r and stores it
template <bool VEC>
__global__ __launch_bounds__(DT_THREADS) void cl_graph_kernel(const float* __restrict__ x, const double* __restrict__ norms, int N, int d, double eps2,
                                                              unsigned long long* __restrict__ adj, int W) {
  __shared__ __align__(16) double stage[DT_STAGE];
  __shared__ double side[2][DT_T];
  __shared__ unsigned char pred[DT_T][DT_T + 4];
  const DtLane l = dt_lane();
  const int i0 = (int)blockIdx.y * DT_T, j0 = (int)blockIdx.x * DT_T;
  if (l.t < 2 * DT_T) {
    const int op = l.t >> 6, row = (op ? j0 : i0) + (l.t & 63);
    side[op][l.t & 63] = row < N ? norms[row] : 0.0;
  }
  dt_f64x4 acc[2][2];
  dt_dots(acc, stage, l, (d + DT_KC - 1) / DT_KC, [&](int op, int row, int kk) { return ft_row4<VEC>(x, (op ? j0 : i0) + row, N, d, kk); });
  dt_each(acc, l, [&](double dot, int r, int c) {
    const int i = i0 + r, j = j0 + c;
    pred[r][c] = j < N && (i == j || cl_value<VSX_PDIST_SQEUCLIDEAN>(dot, side[0][r], side[1][c], false) <= eps2);
  });
  __syncthreads();
  const int lane = l.t & 63, wave = l.t >> 6;
  unsigned long long mine = 0;
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const unsigned long long word = __ballot(pred[16 * wave + rr][lane] != 0);
    if (lane == rr) mine = word;
  }
  const int i = i0 + 16 * wave + lane;
  if (lane < 16 && i < N) adj[(size_t)i * (size_t)W + blockIdx.x] = mine;
}

__device__ __forceinline__ int cl_wave_sum_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int cl_wave_min_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// one wave per row: deg[i] = the popcount of the row's W words
__global__ __launch_bounds__(CL_WAVES * 64) void cl_degree_kernel(const unsigned long long* __restrict__ adj, int N, int W, int* __restrict__ deg) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;
  int n = 0;
  for (int w = lane; w < W; w += 64) n += __popcll(adj[(size_t)i * (size_t)W + w]);
  n = cl_wave_sum_i32(n);
  if (lane == 0) deg[i] = n;
}

__global__ void cl_clear_kernel(int* changed) { changed[0] = 0; }

// the smallest value[j] over the core neighbours j of row i (the wave's lanes share the row's words), INT_MAX where there is none.
// `value` is read through a volatile pointer where other workgroups of the launch may be storing to it
template <class Value>
__device__ __forceinline__ int cl_min_over_core_neighbours(const unsigned long long* __restrict__ adj, const unsigned char* __restrict__ core, int i,
                                                           int N, int W, int lane, Value&& value) {
  int m = 0x7fffffff;
  for (int w = lane; w < W; w += 64) {
    unsigned long long word = adj[(size_t)i * (size_t)W + w];
    for (int n = 0; n < 64 && word; ++n) {  // at most 64 set bits
      const int b = __ffsll((long long)word) - 1;
      word &= word - 1;
      const int j = 64 * w + b;
      if (j < N && core[j]) m = min(m, value(j));
    }
  }
  return cl_wave_min_i32(m);
}

// hooking: a core row takes the smallest label among itself and its core neighbours
__global__ __launch_bounds__(CL_WAVES * 64) void cl_hook_kernel(const unsigned long long* __restrict__ adj, const unsigned char* __restrict__ core,
                                                                int* labels, int N, int W, int* changed) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
  if (i >= N || !core[i]) return;
  const volatile int* lab = labels;
  const int m = cl_min_over_core_neighbours(adj, core, i, N, W, lane, [&](int j) { return (int)lab[j]; });
  if (lane == 0 && m < lab[i]) {
    labels[i] = m;
    changed[0] = 1;
  }
}
// pointer jumping: labels[i] <- labels[labels[i]], at most CL_JUMPS times.  A label is a core row's index in [0, i]
#define CL_JUMPS 32
__global__ __launch_bounds__(256) void cl_jump_kernel(const unsigned char* __restrict__ core, int* labels, int N, int* changed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N || !core[i]) return;
  const volatile int* lab = labels;
  const int first = lab[i];
  int cur = first;
  for (int n = 0; n < CL_JUMPS; ++n) {
    const int up = (unsigned)cur < (unsigned)N ? (int)lab[cur] : cur;
    if (up >= cur) break;
    cur = up;
  }
  if (cur < first) {
    labels[i] = cur;
    changed[0] = 1;
  }
}

__global__ __launch_bounds__(CL_WAVES * 64) void cl_finish_kernel(const unsigned long long* __restrict__ adj, const unsigned char* __restrict__ core,
                                                                  const int* __restrict__ labels, const int* __restrict__ cid, int N, int W,
                                                                  int* __restrict__ out) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
  if (i >= N) return;
  int v;
  if (core[i]) {
    const int root = labels[i];
    v = (unsigned)root < (unsigned)N ? cid[root] : -1;
  } else {
    v = cl_min_over_core_neighbours(adj, core, i, N, W, lane, [&](int j) {
      const int root = labels[j];
      return (unsigned)root < (unsigned)N ? cid[root] : 0x7fffffff;
    });
    if (v == 0x7fffffff) v = -1;
  }
  if (lane == 0) out[i] = v;
}

// ------------------------------------------------------------------ host
#define CL_MAX_TILES 65535  // row tiles of a launch (gridDim.y)
static bool cl_shape_ok(const char* who, int64_t N, int64_t d) {
  if (N >= 1 && N <= (int64_t)CL_MAX_TILES * DT_T && d >= 1 && d <= (1 << 20)) return true;
  vsx_set_error("%s: N=%ld must be in [1, %ld], d=%ld in [1, 2^20]", who, (long)N, (long)CL_MAX_TILES * DT_T, (long)d);
  return false;
}
static inline bool cl_al(const void* p, int a) { return p && ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

extern "C" int32_t vsx_row_sqnorm_f64(const float* x, int32_t N, int32_t d, double* norms, vsx_stream_t stream) {
  if (!cl_shape_ok("vsx_row_sqnorm_f64", N, d)) return 1;
  VSX_CHECK(cl_al(x, 4) && cl_al(norms, 8), "vsx_row_sqnorm_f64: x must be 4-byte aligned, norms 8-byte aligned, neither null");
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    hipLaunchKernelGGL((cl_pdist_kernel<decltype(vec)::value, CL_NORMS>), dim3(1, (unsigned)vsx_cdiv(N, DT_T)), dim3(DT_THREADS), 0, (hipStream_t)stream,
                       x, (const double*)nullptr, d, 0, N, 0, N, norms, (size_t)0);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_pdist_f64(const float* x, const double* norms, int32_t N, int32_t d, int32_t metric, int32_t r0, int32_t r1, int32_t c0,
                                 int32_t c1, double* out, int64_t ld, vsx_stream_t stream) {
  if (!cl_shape_ok("vsx_pdist_f64", N, d)) return 1;
  VSX_CHECK(metric >= VSX_PDIST_COSINE && metric <= VSX_PDIST_SQEUCLIDEAN, "vsx_pdist_f64: metric=%ld must be 0 (cosine), 1 (Euclidean) or 2 (squared)", (long)metric);
  VSX_CHECK(0 <= r0 && r0 < r1 && r1 <= N && 0 <= c0 && c0 < c1 && c1 <= N, "vsx_pdist_f64: the block [%ld, %ld) x [%ld, %ld) must lie in [0, %ld)",
            (long)r0, (long)r1, (long)c0, (long)c1, (long)N);
  VSX_CHECK(ld >= (int64_t)c1 - c0, "vsx_pdist_f64: ld=%ld is shorter than the block's %ld columns", (long)ld, (long)(c1 - c0));
  VSX_CHECK(cl_al(x, 4) && cl_al(norms, 8) && cl_al(out, 8), "vsx_pdist_f64: x must be 4-byte aligned, norms and out 8-byte aligned, none null");
  const dim3 grid((unsigned)vsx_cdiv(c1 - c0, DT_T), (unsigned)vsx_cdiv(r1 - r0, DT_T));
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    vsx_by_int<0, 1, 2>(metric, [&](auto m) {
      hipLaunchKernelGGL((cl_pdist_kernel<decltype(vec)::value, decltype(m)::value>), grid, dim3(DT_THREADS), 0, (hipStream_t)stream, x, norms, d, r0, r1,
                         c0, c1, out, (size_t)ld);
    });
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_eps_graph(const float* x, const double* norms, int32_t N, int32_t d, double eps2, uint64_t* adj, int32_t* deg,
                                 vsx_stream_t stream) {
  if (!cl_shape_ok("vsx_eps_graph", N, d)) return 1;
  VSX_CHECK(eps2 >= 0.0 && eps2 <= 1.79769313486231570815e308, "vsx_eps_graph: eps2 must be finite and >= 0");
  VSX_CHECK(cl_al(x, 4) && cl_al(norms, 8) && cl_al(adj, 8) && cl_al(deg, 4),
            "vsx_eps_graph: x and deg must be 4-byte aligned, norms and adj 8-byte aligned, none null");
  const int W = vsx_cdiv(N, 64);
  hipStream_t st = (hipStream_t)stream;
  vsx_by_bool(ft_vec_ok(x, d), [&](auto vec) {
    hipLaunchKernelGGL((cl_graph_kernel<decltype(vec)::value>), dim3((unsigned)W, (unsigned)W), dim3(DT_THREADS), 0, st, x, norms, N, d, eps2,
                       (unsigned long long*)adj, W);
  });
  hipLaunchKernelGGL(cl_degree_kernel, dim3((unsigned)vsx_cdiv(N, CL_WAVES)), dim3(CL_WAVES * 64), 0, st, (const unsigned long long*)adj, N, W, deg);
  VSX_LAUNCH_CHECK();
  return 0;
}

static bool cl_graph_args_ok(const char* who, int64_t N, const void* adj, const void* core, const void* labels) {
  if (N >= 1 && N <= (int64_t)CL_MAX_TILES * DT_T && cl_al(adj, 8) && core && cl_al(labels, 4)) return true;
  vsx_set_error("%s: N=%ld must be in [1, %ld], adj 8-byte and labels 4-byte aligned, none null", who, (long)N, (long)CL_MAX_TILES * DT_T);
  return false;
}

extern "C" int32_t vsx_cc_round(const uint64_t* adj, const uint8_t* core, int32_t* labels, int32_t N, int32_t* changed, vsx_stream_t stream) {
  if (!cl_graph_args_ok("vsx_cc_round", N, adj, core, labels)) return 1;
  VSX_CHECK(cl_al(changed, 4), "vsx_cc_round: changed must be 4-byte aligned and not null");
  hipStream_t st = (hipStream_t)stream;
  const int W = vsx_cdiv(N, 64);
  hipLaunchKernelGGL(cl_clear_kernel, dim3(1), dim3(1), 0, st, changed);
  hipLaunchKernelGGL(cl_hook_kernel, dim3((unsigned)vsx_cdiv(N, CL_WAVES)), dim3(CL_WAVES * 64), 0, st, (const unsigned long long*)adj, core, labels, N, W,
                     changed);
  hipLaunchKernelGGL(cl_jump_kernel, dim3((unsigned)vsx_cdiv(N, 256)), dim3(256), 0, st, core, labels, N, changed);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_dbscan_finish(const uint64_t* adj, const uint8_t* core, const int32_t* labels, const int32_t* cid, int32_t N, int32_t* out,
                                     vsx_stream_t stream) {
  if (!cl_graph_args_ok("vsx_dbscan_finish", N, adj, core, labels)) return 1;
  VSX_CHECK(cl_al(cid, 4) && cl_al(out, 4), "vsx_dbscan_finish: cid and out must be 4-byte aligned and not null");
  hipLaunchKernelGGL(cl_finish_kernel, dim3((unsigned)vsx_cdiv(N, CL_WAVES)), dim3(CL_WAVES * 64), 0, (hipStream_t)stream, (const unsigned long long*)adj,
                     core, labels, cid, N, vsx_cdiv(N, 64), out);
  VSX_LAUNCH_CHECK();
  return 0;
}
