// viscy_amd — the device side of OnlineEvalCallback (viscy_utils/callbacks/online_eval.py): cosine k-nearest neighbours among the
// rows of OTHER groups (cross-validation folds, or the train part of a holdout split), the neighbours' majority vote, and the
// cosine distance of listed row pairs.  All arithmetic is fp32; dot products run on the exact f32-in / f32-accumulate MFMA
// (v_mfma_f32_32x32x2_f32), so neighbour ranks do not depend on a reduced-precision rounding.
//
//   inv_i  = 1 / (||x_i|| + eps)                       (0 where the denominator is 0)
//   s_ij   = fl32(fl32(dot_ij * inv_i) * inv_j)        candidate iff group[j] >= 0 && group[j] != group[i]
//   result = the min(k, #candidates) best candidates of every row in the total order (s descending, j ascending)
//
// vsx_knn_topk never stores an N x N matrix.  A workgroup owns 128 query rows and one contiguous range of candidate tiles
// (128 rows each).  Per tile it forms the 128 x 128 tile of dot products in registers with the tile engine of f32_tile.h (which
// also fixes the dots' summation order), writes the scaled and masked similarities to LDS one 64-column half at a time, and
// thread r < 128 scans row r of that half against the row's k-th best, which it keeps in registers; the few survivors are
// inserted into the row's sorted list in LDS.  The candidate range of a query tile is split over up to KT_MAX_SPLITS workgroups
// to fill the machine; every split stores its sorted list to the workspace (O(N k)), and a second kernel merges the splits'
// lists per row in the same total order.  Since the order is total, the result does not depend on the split count or on the
// order in which survivors were inserted.
//
// A masked entry travels through LDS as NaN: every comparison with it is false, so it is never inserted (a NaN similarity of
// non-finite input rows is dropped in the same way).
#include "f32_tile.h"
#include "../../include/vsx.h"

#include <math.h>

#define KT_MAX_SPLITS 8
#define KT_MAX_K VSX_KNN_MAX_K

// (a) inverse row norms: ft_inv_norm_kernel of f32_tile.h
// ------------------------------------------------------------------ (d) cosine distance of listed pairs: one wave per pair
__global__ __launch_bounds__(256) void pair_cosine_dist_kernel(const float* __restrict__ x, const float* __restrict__ inv,
                                                               const int* __restrict__ pi, const int* __restrict__ pj, long P, int d,
                                                               float* __restrict__ out) {
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= P) return;
  const int i = pi[p], j = pj[p];
  const float* xi = x + (size_t)i * d;
  const float* xj = x + (size_t)j * d;
  float dot = 0.f;
  for (int c = lane; c < d; c += 64) dot = fmaf(xi[c], xj[c], dot);
  dot = ft_wave_sum(dot);
  if (lane == 0) out[p] = __fsub_rn(1.f, __fmul_rn(__fmul_rn(dot, inv[i]), inv[j]));
}

// ------------------------------------------------------------------ (b) streaming similarity + top-k
__device__ __forceinline__ bool kt_better(float s, int j, float s0, int j0) { return s > s0 || (s == s0 && j < j0); }

// KB: the list capacity the LDS is sized for (k <= KB); the lists themselves are laid out for the k of the call.
// VEC: d % 4 == 0 and x 16-byte aligned, rows are read as float4; else feature by feature
template <bool VEC, int KB>
__global__ __launch_bounds__(FT_THREADS, KB <= 24 ? 2 : 1) void knn_topk_kernel(const float* __restrict__ x, const float* __restrict__ inv,
                                                                const int* __restrict__ group, int N, int d, int k,
                                                                int tiles_per_split, int* __restrict__ pidx,
                                                                float* __restrict__ psim, int* __restrict__ pcnt) {
  __shared__ __attribute__((aligned(16))) float kt_smem[FT_STAGE + 2 * KB * FT_T];
  float* stage = kt_smem;                       // the engine's staging area; later the similarity half-tile
  float* ls = kt_smem + FT_STAGE;               // [k][FT_T] sorted similarities of every query row
  int* li = reinterpret_cast<int*>(ls + (size_t)k * FT_T);  // [k][FT_T] their row indices
  __shared__ float invq[FT_T], invc[FT_T];
  __shared__ int gq[FT_T], gc[FT_T];

  const FtLane l = ft_lane();
  const int t = l.t;
  const FtRange g = ft_range(N, d, tiles_per_split);
  const int q0 = g.q0;

  ft_side(gq, group, q0, N, -1);
  ft_side(invq, inv, q0, N, 0.f);
  // the owner of query row t keeps the row's count and its k-th best in registers
  const bool owner = t < FT_T && q0 + t < N;
  int cnt = 0;
  float thr_s = 0.f;
  int thr_j = 0;

  for (int ct = g.ct0; ct < g.ct1; ++ct) {
    const int c0 = ct * FT_T;
    ft_f32x16 acc[2][2];
    ft_dots(
        acc, stage, l, g.nchunks, [&](int operand, int r, int kk) { return ft_row4<VEC>(x, (operand ? c0 : q0) + r, N, d, kk); },
        [&] {
          ft_side(gc, group, c0, N, -1);
          ft_side(invc, inv, c0, N, 0.f);
        });
    __syncthreads();  // every wave is done with the staged chunk: the half-tile takes its place

    for (int h = 0; h < 2; ++h) {
      ft_put_half(stage, acc, l, h, [&](float dot, int row, int col) {
        const int gj = gc[col];
        const bool ok = gj >= 0 && gj != gq[row];
        const float s = __fmul_rn(__fmul_rn(dot, invq[row]), invc[col]);
        return ok ? s : __builtin_nanf("");
      });
      __syncthreads();
      if (owner) {
        const float* srow = ft_half_row(stage, t);
        const int jbase = c0 + h * 64;
        for (int c = 0; c < 64; ++c) {
          const float s = srow[c];
          const int j = jbase + c;
          if (!(s == s)) continue;
          if (cnt == k && !kt_better(s, j, thr_s, thr_j)) continue;
          int p = cnt < k ? cnt++ : k - 1;        // a full list drops its last entry
          while (p > 0) {
            const float sp = ls[(size_t)(p - 1) * FT_T + t];
            const int jp = li[(size_t)(p - 1) * FT_T + t];
            if (!kt_better(s, j, sp, jp)) break;
            ls[(size_t)p * FT_T + t] = sp;
            li[(size_t)p * FT_T + t] = jp;
            --p;
          }
          ls[(size_t)p * FT_T + t] = s;
          li[(size_t)p * FT_T + t] = j;
          if (cnt == k) {
            thr_s = ls[(size_t)(k - 1) * FT_T + t];
            thr_j = li[(size_t)(k - 1) * FT_T + t];
          }
        }
      }
      __syncthreads();
    }
  }

  if (owner) {
    const size_t base = ((size_t)blockIdx.y * N + (size_t)(q0 + t)) * k;
    for (int p = 0; p < cnt; ++p) {
      psim[base + p] = ls[(size_t)p * FT_T + t];
      pidx[base + p] = li[(size_t)p * FT_T + t];
    }
    pcnt[(size_t)blockIdx.y * N + q0 + t] = cnt;
  }
}

// merges the splits' sorted lists of every row; writes every slot of idx / sim and cnt
__global__ __launch_bounds__(256) void knn_merge_kernel(const int* __restrict__ pidx, const float* __restrict__ psim,
                                                        const int* __restrict__ pcnt, int N, int k, int splits, int* __restrict__ idx,
                                                        float* __restrict__ sim, int* __restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int head[KT_MAX_SPLITS], len[KT_MAX_SPLITS];
#pragma unroll
  for (int s = 0; s < KT_MAX_SPLITS; ++s) {
    head[s] = 0;
    len[s] = s < splits ? pcnt[(size_t)s * N + i] : 0;
  }
  int total = 0;
  for (int p = 0; p < k; ++p) {
    int best = -1, bj = 0;
    float bs = 0.f;
#pragma unroll
    for (int s = 0; s < KT_MAX_SPLITS; ++s) {
      if (head[s] < len[s]) {
        const size_t at = ((size_t)s * N + i) * k + head[s];
        const float v = psim[at];
        const int j = pidx[at];
        if (best < 0 || kt_better(v, j, bs, bj)) {
          best = s;
          bs = v;
          bj = j;
        }
      }
    }
    if (best >= 0) {
#pragma unroll
      for (int s = 0; s < KT_MAX_SPLITS; ++s) head[s] += (s == best);
      ++total;
    }
    idx[(size_t)i * k + p] = best >= 0 ? bj : -1;
    sim[(size_t)i * k + p] = best >= 0 ? bs : -INFINITY;
  }
  cnt[i] = total;
}

// ------------------------------------------------------------------ (c) majority vote: most frequent label, ties to the smallest
#define KV_THREADS 64
__global__ __launch_bounds__(KV_THREADS) void knn_vote_kernel(const int* __restrict__ idx, const int* __restrict__ cnt,
                                                              const int* __restrict__ labels, int N, int k, int* __restrict__ pred) {
  __shared__ int lab[KT_MAX_K][KV_THREADS];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * KV_THREADS + tid;
  if (i >= N) return;
  const int c = min(cnt[i], k);
  for (int q = 0; q < c; ++q) lab[q][tid] = labels[idx[(size_t)i * k + q]];
  int best_n = 0, best_l = -1;
  for (int p = 0; p < c; ++p) {
    const int l = lab[p][tid];
    int n = 0;
    for (int q = 0; q < c; ++q) n += lab[q][tid] == l;
    if (n > best_n || (n == best_n && l < best_l)) {
      best_n = n;
      best_l = l;
    }
  }
  pred[i] = best_l;
}

// ------------------------------------------------------------------ host
static int kt_range(const char* who, int64_t N, int64_t d, int64_t k) {
  VSX_CHECK(N >= 1 && N <= (1 << 30), "%s: N=%ld must be in [1, 2^30]", who, (long)N);
  VSX_CHECK(d >= 1 && d <= (1 << 20), "%s: d=%ld must be in [1, 2^20]", who, (long)d);
  VSX_CHECK(k >= 1 && k <= KT_MAX_K, "%s: k=%ld must be in [1, %d]", who, (long)k, KT_MAX_K);
  return 0;
}

extern "C" int32_t vsx_row_inv_norm(const float* x, float* inv, int32_t N, int32_t d, float eps, vsx_stream_t stream) {
  return ft_inv_norm<false>("vsx_row_inv_norm", x, inv, N, d, eps, (hipStream_t)stream);
}

extern "C" int64_t vsx_knn_topk_ws_bytes(int32_t N, int32_t d, int32_t k) {
  if (N < 1 || d < 1 || k < 1 || k > KT_MAX_K) return 0;
  return (int64_t)KT_MAX_SPLITS * N * ((int64_t)k * 8 + 4);  // per split: idx[N][k], sim[N][k], cnt[N]
}

// how many workgroups share the candidate range of one query tile: the count in 1 .. KT_MAX_SPLITS that leaves the fewest idle
// workgroup slots in the last round (two workgroups per compute unit), the smaller count on a tie
static int kt_splits(int qtiles, int ctiles, int cus) {
  const long slots = 2L * (cus > 0 ? cus : 256);
  int best = 1;
  double best_eff = 0.0;
  for (int s = 1; s <= KT_MAX_SPLITS && s <= ctiles; ++s) {
    int n, tps;
    ft_even_split(ctiles, s, &n, &tps);
    if (n != s) continue;  // the last split would be empty
    const long wgs = (long)qtiles * s;
    const double eff = (double)wgs / (double)(((wgs + slots - 1) / slots) * slots);
    if (eff > best_eff * 1.02) {
      best_eff = eff;
      best = s;
    }
  }
  return best;
}

extern "C" int32_t vsx_knn_topk(const float* x, const float* inv, const int32_t* group, int32_t N, int32_t d, int32_t k, int32_t* idx,
                                float* sim, int32_t* cnt, void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  if (int rc = kt_range("vsx_knn_topk", N, d, k)) return rc;
  VSX_CHECK(x && inv && group && idx && sim && cnt && ws, "vsx_knn_topk: null argument");
  VSX_CHECK(ws_bytes >= vsx_knn_topk_ws_bytes(N, d, k) && ((uintptr_t)ws & 3) == 0,
            "vsx_knn_topk: the workspace must be 4-byte aligned and hold vsx_knn_topk_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_knn_topk_ws_bytes(N, d, k), (long)ws_bytes);
  const int qtiles = (N + FT_T - 1) / FT_T, ctiles = qtiles;
  int splits, tps;
  ft_even_split(ctiles, kt_splits(qtiles, ctiles, vsx_cu_count()), &splits, &tps);
  int* pidx = (int*)ws;
  float* psim = (float*)(pidx + (size_t)splits * N * k);
  int* pcnt = (int*)(psim + (size_t)splits * N * k);
  const bool vec = ft_vec_ok(x, d);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)qtiles, (unsigned)splits), block(FT_THREADS);
  vsx_by_int<8, 24, 64>(k <= 8 ? 8 : k <= 24 ? 24 : 64, [&](auto kb) {  // the smallest candidate buffer that holds k
    vsx_by_bool(vec, [&](auto vec_) {
      hipLaunchKernelGGL((knn_topk_kernel<decltype(vec_)::value, decltype(kb)::value>), grid, block, 0, s, x, inv, group, N, d, k, tps, pidx,
                         psim, pcnt);
    });
  });
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const int*)pidx, (const float*)psim,
                     (const int*)pcnt, N, k, splits, idx, sim, cnt);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_knn_vote(const int32_t* idx, const int32_t* cnt, const int32_t* labels, int32_t N, int32_t k, int32_t* pred,
                                vsx_stream_t stream) {
  if (int rc = kt_range("vsx_knn_vote", N, 1, k)) return rc;
  VSX_CHECK(idx && cnt && labels && pred, "vsx_knn_vote: null argument");
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)((N + KV_THREADS - 1) / KV_THREADS)), dim3(KV_THREADS), 0, (hipStream_t)stream,
                     idx, cnt, labels, N, k, pred);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_pair_cosine_dist(const float* x, const float* inv, const int32_t* pi, const int32_t* pj, int64_t P, int32_t d,
                                        float* out, vsx_stream_t stream) {
  VSX_CHECK(x && inv && pi && pj && out && d >= 1, "vsx_pair_cosine_dist: bad arguments");
  VSX_CHECK(P >= 1 && P < (1L << 33), "vsx_pair_cosine_dist: P=%ld must be in [1, 2^33)", (long)P);
  hipLaunchKernelGGL(pair_cosine_dist_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, inv, pi, pj,
                     (long)P, d, out);
  VSX_LAUNCH_CHECK();
  return 0;
}
