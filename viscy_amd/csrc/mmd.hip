// viscy_amd — the device side of the MMD two-sample permutation test (viscy_utils/evaluation/mmd.py): Gaussian RBF kernel sums of
// the pooled rows [X; Y] under P 0/1 label vectors, the median-heuristic bandwidth's squared distances, and rectangles of the
// kernel matrix.  fp32 kernel values from dots on the exact f32 MFMA (the tile engine of f32_tile.h), sums folded in float64.
//
//   c_i   = x_i - mean (pooled column mean, formed in a fixed order);   n_i = sum_c c_ic^2        (vsx_mmd_prepare)
//   d2_ij = max(fl32(fl32(n_i + n_j) - 2 dot_ij), 0);   k_ij = expf(-fl32(d2_ij / fl32(2 bandwidth)));   k_ii = 0   (mmd_kval)
//   per label vector z:  quad = z' K z,  zr = 1' K z,  T = 1' K 1
//   sum_XX = quad,  sum_XY = zr - quad,  sum_YY = T - 2 zr + quad
//
// vsx_mmd_sums never stores an N x N matrix.  A workgroup owns 128 pooled rows and a contiguous range of column tiles.  Per tile
// it forms the 128 x 128 dots in registers (ft_dots), turns them into kernel values in LDS (the tile takes the place of the
// engine's staging area) ONCE, and then, for chunks of MM_PC = 128 label vectors, multiplies the tile by the label tile of the
// same columns on the f32 MFMA (labels sit in LDS as bytes; 0/1 factors make every product exact), weights the product with the
// labels of its own rows and reduces over rows in float64.  Label vector P is a virtual row of ones: its `zr` is T.  Partials go
// to a workspace row that only this workgroup touches (no atomics); a second kernel folds the rows in ascending order.  How the
// column tiles are split over workgroups depends on N alone, so the result is a pure function of the inputs.
#include "f32_tile.h"
#include "../../include/vsx.h"

#include <math.h>

#define MM_PC 128          // label vectors per chunk
#define MM_KLD 132         // floats per row of the kernel tile: 128 + 4, as FT_LD = 32 + 4
#define MM_ZLD 132         // bytes per row of a label tile: 33 words
#define MM_MAX_SPLITS 32
#define MM_WANT_WGS 512    // workgroups aimed at when the column range is split

// the one definition of a kernel value; every operation rounded on its own, IEEE division, library expf
__device__ __forceinline__ float mmd_d2(float ni, float nj, float dot) {
  return fmaxf(__fsub_rn(__fadd_rn(ni, nj), __fmul_rn(2.f, dot)), 0.f);
}
__device__ __forceinline__ float mmd_kval(float ni, float nj, float dot, float two_bw) { return expf(-__fdiv_rn(mmd_d2(ni, nj, dot), two_bw)); }

// ------------------------------------------------------------------ (a) centring: pooled column mean, centred rows, squared norms
// 16 columns x 16 row lanes per workgroup; a row lane sums its rows in ascending order in float64, the lanes are folded 0 .. 15
__global__ __launch_bounds__(256) void mmd_colmean_kernel(const float* __restrict__ x, float* __restrict__ mean, int N, int d) {
  __shared__ double part[16][16];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  double s = 0.0;
  if (col < d)
    for (int r = rl; r < N; r += 16) s += (double)x[(size_t)r * d + col];
  part[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < d) {
    double tot = 0.0;
    for (int q = 0; q < 16; ++q) tot += part[q][cl];
    mean[col] = (float)(tot / (double)N);
  }
}
// one wave per row; the norm's reduction is that of ft_inv_norm_kernel
__global__ __launch_bounds__(256) void mmd_centre_kernel(const float* __restrict__ x, const float* __restrict__ mean, float* __restrict__ xc,
                                                         float* __restrict__ nrm, int N, int d) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* xr = x + (size_t)row * d;
  float* cr = xc + (size_t)row * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = __fsub_rn(xr[c], mean[c]);
    cr[c] = v;
    ss = fmaf(v, v, ss);
  }
  ss = ft_wave_sum(ss);
  if (lane == 0) nrm[row] = ss;
}

// ------------------------------------------------------------------ (b) streaming kernel sums
// 64 bytes (16 words) of label row p, columns cb .. cb + 63; row P is the virtual row of ones; zeros past N or P
template <bool VECZ>
__device__ __forceinline__ void mmd_fetch_labels(uint32_t* r, const uint8_t* __restrict__ z, long p, long P, int cb, int N) {
  if (VECZ) {  // N % 16 == 0 and z 16-byte aligned: a 16-byte group lies inside the row or past it
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int col = cb + 16 * v;
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (col < N) {
        if (p < P) w = *reinterpret_cast<const uint4*>(z + (size_t)p * N + col);
        else if (p == P) w = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
      }
      r[4 * v] = w.x; r[4 * v + 1] = w.y; r[4 * v + 2] = w.z; r[4 * v + 3] = w.w;
    }
  } else {
    const uint8_t* zr = z + (size_t)(p < P ? p : 0) * N;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      uint32_t w = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = cb + 4 * u + i;
        uint32_t b = 0u;
        if (col < N) b = p < P ? (uint32_t)zr[col] : (p == P ? 1u : 0u);
        w |= b << (8 * i);
      }
      r[u] = w;
    }
  }
}

// VEC: d % 4 == 0 and xc 16-byte aligned.  ws: [workgroup][2][P + 1] doubles: quad | zr (entry P of zr: this workgroup's share of T)
template <bool VEC, bool VECZ>
__global__ __launch_bounds__(FT_THREADS, 1) void mmd_sums_kernel(const float* __restrict__ xc, const float* __restrict__ nrm,
                                                                 const uint8_t* __restrict__ z, int N, int d, int P, float two_bw,
                                                                 int tiles_per_split, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float ktile[FT_T * MM_KLD];  // the engine's staging area, then the kernel tile
  __shared__ __attribute__((aligned(16))) uint8_t zc[MM_PC * MM_ZLD];  // labels of the tile's columns  [p][column]
  __shared__ __attribute__((aligned(16))) uint8_t zq[MM_PC * MM_ZLD];  // labels of the workgroup's rows [p][row]
  __shared__ double red[2][2][2][MM_PC];                               // [quad | zr][wq][lane half][p]
  __shared__ float nq[FT_T], nc[FT_T];
  static_assert(FT_STAGE <= FT_T * MM_KLD, "the staging area must fit the kernel tile");

  const FtLane l = ft_lane();
  const int t = l.t;
  const FtRange g = ft_range(N, d, tiles_per_split);
  const int q0 = g.q0;
  const int Pp = P + 1;
  const int npc = (Pp + MM_PC - 1) / MM_PC;
  double* wsq = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * (size_t)Pp;
  const int zrow = t >> 1, zoff = (t & 1) * 64;  // this thread's share of a label tile: row, first column

  ft_side(nq, nrm, q0, N, 0.f);

  for (int ct = g.ct0; ct < g.ct1; ++ct) {
    const int c0 = ct * FT_T;
    ft_f32x16 acc[2][2];
    ft_dots(
        acc, ktile, l, g.nchunks, [&](int operand, int r, int kk) { return ft_row4<VEC>(xc, (operand ? c0 : q0) + r, N, d, kk); },
        [&] { ft_side(nc, nrm, c0, N, 0.f); });
    __syncthreads();  // every wave is done with the staged chunk: the kernel tile takes its place
    ft_each(acc, l, [&](float dot, int row, int col) {
      const int gi = q0 + row, gj = c0 + col;
      const bool ok = gi < N && gj < N && gi != gj;
      ktile[row * MM_KLD + col] = ok ? mmd_kval(nq[row], nc[col], dot, two_bw) : 0.f;
    });

    uint32_t lc[16], lq[16];
    mmd_fetch_labels<VECZ>(lc, z, zrow, P, c0 + zoff, N);
    mmd_fetch_labels<VECZ>(lq, z, zrow, P, q0 + zoff, N);
    for (int pc = 0; pc < npc; ++pc) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        *reinterpret_cast<uint32_t*>(zc + zrow * MM_ZLD + zoff + 4 * u) = lc[u];
        *reinterpret_cast<uint32_t*>(zq + zrow * MM_ZLD + zoff + 4 * u) = lq[u];
      }
      __syncthreads();  // the label tiles (and, for the first chunk, the kernel tile) are in place
      if (pc + 1 < npc) {
        mmd_fetch_labels<VECZ>(lc, z, (long)(pc + 1) * MM_PC + zrow, P, c0 + zoff, N);
        mmd_fetch_labels<VECZ>(lq, z, (long)(pc + 1) * MM_PC + zrow, P, q0 + zoff, N);
      }

      // S = K tile (128 rows x 128 columns) x labels' (128 columns x 128 label vectors)
      ft_f32x16 s2[2][2];
      ft_zero(s2);
      const float* ka = ktile + (l.wq * 64 + l.r32) * MM_KLD + 4 * l.hh;
      const uint8_t* zb = zc + (l.wc * 64 + l.r32) * MM_ZLD + 4 * l.hh;
#pragma unroll 4
      for (int p8 = 0; p8 < FT_T / 8; ++p8) {
        const float4 a0 = *reinterpret_cast<const float4*>(ka + 8 * p8);
        const float4 a1 = *reinterpret_cast<const float4*>(ka + 32 * MM_KLD + 8 * p8);
        const uint32_t w0 = *reinterpret_cast<const uint32_t*>(zb + 8 * p8);
        const uint32_t w1 = *reinterpret_cast<const uint32_t*>(zb + 32 * MM_ZLD + 8 * p8);
        float b0[4], b1[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) b0[s] = (float)((w0 >> (8 * s)) & 0xffu), b1[s] = (float)((w1 >> (8 * s)) & 0xffu);
        ft_mma_step(s2, a0, a1, b0, b1);
      }

      // the lane's 32 rows of label vector pcol, in float64: all of them (zr) and those the vector labels 1 (quad)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int pcol = l.wc * 64 + b * 32 + l.r32;
        double sq = 0.0, sa = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(zq + pcol * MM_ZLD + l.wq * 64 + a * 32 + 8 * g + 4 * l.hh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const double v = (double)s2[a][b][4 * g + i];
              sa += v;
              sq += ((w >> (8 * i)) & 1u) ? v : 0.0;
            }
          }
        red[0][l.wq][l.hh][pcol] = sq;
        red[1][l.wq][l.hh][pcol] = sa;
      }
      __syncthreads();  // the partials are in place; every read of the label tiles is done
      const int p = pc * MM_PC + (t & (MM_PC - 1));
      if (p < Pp) {
        const int which = t >> 7;  // threads 0 .. 127 fold quad, 128 .. 255 zr
        const int tp = t & (MM_PC - 1);
        const double v = ((red[which][0][0][tp] + red[which][0][1][tp]) + red[which][1][0][tp]) + red[which][1][1][tp];
        double* dst = wsq + (size_t)which * Pp + p;
        *dst = ct == g.ct0 ? v : *dst + v;  // only this workgroup touches its row of the workspace
      }
    }
  }
}

// sums[p] = {sum_XX, sum_YY, sum_XY}: the workgroups' rows folded in ascending order
__global__ __launch_bounds__(256) void mmd_fold_kernel(const double* __restrict__ ws, int nwg, int P, double* __restrict__ sums) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const size_t Pp = (size_t)P + 1;
  double quad = 0.0, zr = 0.0, T = 0.0;
  for (int w = 0; w < nwg; ++w) {
    const double* row = ws + (size_t)w * 2 * Pp;
    quad += row[p];
    zr += row[Pp + p];
    T += row[Pp + P];
  }
  sums[3 * (size_t)p] = quad;
  sums[3 * (size_t)p + 1] = (T - 2.0 * zr) + quad;
  sums[3 * (size_t)p + 2] = zr - quad;
}

// ------------------------------------------------------------------ (c) a rectangle of the pooled kernel, materialised
template <bool VEC>
__global__ __launch_bounds__(FT_THREADS, 2) void mmd_rbf_block_kernel(const float* __restrict__ xc, const float* __restrict__ nrm, int d,
                                                                      int r0, int r1, int c0, int c1, float two_bw, int zero_diag,
                                                                      float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float stage[FT_STAGE];
  __shared__ float nq[FT_T], nc[FT_T];
  const FtLane l = ft_lane();
  const int q0 = r0 + blockIdx.y * FT_T, cb = c0 + blockIdx.x * FT_T;
  ft_side(nq, nrm, q0, r1, 0.f);
  ft_side(nc, nrm, cb, c1, 0.f);
  ft_f32x16 acc[2][2];
  ft_dots(
      acc, stage, l, (d + FT_KC - 1) / FT_KC,
      [&](int operand, int r, int kk) { return operand ? ft_row4<VEC>(xc, cb + r, c1, d, kk) : ft_row4<VEC>(xc, q0 + r, r1, d, kk); }, [] {});
  const size_t ld = (size_t)(c1 - c0);
  ft_each(acc, l, [&](float dot, int row, int col) {
    const int gi = q0 + row, gj = cb + col;
    if (gi < r1 && gj < c1)
      out[(size_t)(gi - r0) * ld + (size_t)(gj - c0)] = (zero_diag && gi == gj) ? 0.f : mmd_kval(nq[row], nc[col], dot, two_bw);
  });
}

// ------------------------------------------------------------------ (d) strict upper triangle of squared distances, one row
template <bool VEC>
__global__ __launch_bounds__(FT_THREADS, 2) void mmd_sqdist_upper_kernel(const float* __restrict__ xc, const float* __restrict__ nrm, int M,
                                                                         int d, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float stage[FT_STAGE];
  __shared__ float nq[FT_T], nc[FT_T];
  if (blockIdx.x < blockIdx.y) return;  // the tile lies below the diagonal (uniform over the workgroup)
  const FtLane l = ft_lane();
  const int q0 = blockIdx.y * FT_T, cb = blockIdx.x * FT_T;
  ft_side(nq, nrm, q0, M, 0.f);
  ft_side(nc, nrm, cb, M, 0.f);
  ft_f32x16 acc[2][2];
  ft_dots(
      acc, stage, l, (d + FT_KC - 1) / FT_KC, [&](int operand, int r, int kk) { return ft_row4<VEC>(xc, (operand ? cb : q0) + r, M, d, kk); },
      [] {});
  ft_each(acc, l, [&](float dot, int row, int col) {
    const long gi = q0 + row, gj = cb + col;
    if (gi < gj && gj < M) out[gi * (2L * M - gi - 1) / 2 + (gj - gi - 1)] = mmd_d2(nq[row], nc[col], dot);
  });
}

// ------------------------------------------------------------------ host
static int mm_range(const char* who, int64_t N, int64_t d) {
  VSX_CHECK(N >= 1 && N <= (1 << 24), "%s: N=%ld must be in [1, 2^24]", who, (long)N);
  VSX_CHECK(d >= 1 && d <= (1 << 20), "%s: d=%ld must be in [1, 2^20]", who, (long)d);
  return 0;
}
static int mm_bandwidth(const char* who, double bandwidth, float* two_bw) {
  *two_bw = (float)(2.0 * bandwidth);
  VSX_CHECK(bandwidth > 0.0 && *two_bw > 0.f && isfinite(*two_bw), "%s: bandwidth=%g must be positive and 2 * bandwidth a finite float", who,
            bandwidth);
  return 0;
}

extern "C" int32_t vsx_mmd_prepare(const float* x, float* xc, float* norms, float* mean, int32_t N, int32_t d, vsx_stream_t stream) {
  if (int rc = mm_range("vsx_mmd_prepare", N, d)) return rc;
  VSX_CHECK(x && xc && norms && mean, "vsx_mmd_prepare: null argument");
  VSX_CHECK((((uintptr_t)x | (uintptr_t)xc | (uintptr_t)norms | (uintptr_t)mean) & 3) == 0, "vsx_mmd_prepare: pointers must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mmd_colmean_kernel, dim3((unsigned)((d + 15) / 16)), dim3(256), 0, s, x, mean, N, d);
  hipLaunchKernelGGL(mmd_centre_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, x, (const float*)mean, xc, norms, N, d);
  VSX_LAUNCH_CHECK();
  return 0;
}

// how many workgroups share the column tiles of one row tile: a function of N alone
static void mm_split(int N, int* tiles, int* splits, int* tps) {
  *tiles = (N + FT_T - 1) / FT_T;
  const int want = (MM_WANT_WGS + *tiles - 1) / *tiles;
  ft_even_split(*tiles, want > MM_MAX_SPLITS ? MM_MAX_SPLITS : want, splits, tps);
}

extern "C" int64_t vsx_mmd_sums_ws_bytes(int32_t N, int32_t P) {
  if (N < 2 || N > (1 << 24) || P < 1 || P > (1 << 24)) return 0;
  int tiles, splits, tps;
  mm_split(N, &tiles, &splits, &tps);
  return (int64_t)tiles * splits * 2 * ((int64_t)P + 1) * 8;
}

extern "C" int32_t vsx_mmd_sums(const float* xc, const float* norms, const uint8_t* labels, int32_t N, int32_t d, int32_t P,
                                double bandwidth, double* sums, void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  if (int rc = mm_range("vsx_mmd_sums", N, d)) return rc;
  VSX_CHECK(N >= 2, "vsx_mmd_sums: N=%ld must be at least 2", (long)N);
  VSX_CHECK(P >= 1 && P <= (1 << 24), "vsx_mmd_sums: P=%ld must be in [1, 2^24]", (long)P);
  float two_bw;
  if (int rc = mm_bandwidth("vsx_mmd_sums", bandwidth, &two_bw)) return rc;
  VSX_CHECK(xc && norms && labels && sums && ws, "vsx_mmd_sums: null argument");
  VSX_CHECK((((uintptr_t)xc | (uintptr_t)norms) & 3) == 0 && (((uintptr_t)sums | (uintptr_t)ws) & 7) == 0,
            "vsx_mmd_sums: xc and norms must be 4-byte aligned, sums and ws 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_mmd_sums_ws_bytes(N, P), "vsx_mmd_sums: the workspace must hold vsx_mmd_sums_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_mmd_sums_ws_bytes(N, P), (long)ws_bytes);
  int tiles, splits, tps;
  mm_split(N, &tiles, &splits, &tps);
  const bool vec = ft_vec_ok(xc, d);
  const bool vecz = N % 16 == 0 && vsx_al16(labels);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, (unsigned)splits), block(FT_THREADS);
  vsx_by_bool(vec, [&](auto vec_) {
    vsx_by_bool(vecz, [&](auto vecz_) {
      hipLaunchKernelGGL((mmd_sums_kernel<decltype(vec_)::value, decltype(vecz_)::value>), grid, block, 0, s, xc, norms, labels, N, d, P, two_bw,
                         tps, (double*)ws);
    });
  });
  hipLaunchKernelGGL(mmd_fold_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const double*)ws, tiles * splits, P, sums);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_rbf_block(const float* xc, const float* norms, int32_t N, int32_t d, int32_t r0, int32_t r1, int32_t c0, int32_t c1,
                                 double bandwidth, int32_t zero_diag, float* out, vsx_stream_t stream) {
  if (int rc = mm_range("vsx_rbf_block", N, d)) return rc;
  VSX_CHECK(0 <= r0 && r0 < r1 && r1 <= N && 0 <= c0 && c0 < c1 && c1 <= N, "vsx_rbf_block: [%ld, %ld) x [%ld, %ld) is not a rectangle of %ld rows",
            (long)r0, (long)r1, (long)c0, (long)c1, (long)N);
  float two_bw;
  if (int rc = mm_bandwidth("vsx_rbf_block", bandwidth, &two_bw)) return rc;
  VSX_CHECK(xc && norms && out, "vsx_rbf_block: null argument");
  VSX_CHECK((((uintptr_t)xc | (uintptr_t)norms | (uintptr_t)out) & 3) == 0, "vsx_rbf_block: pointers must be 4-byte aligned");
  const dim3 grid((unsigned)((c1 - c0 + FT_T - 1) / FT_T), (unsigned)((r1 - r0 + FT_T - 1) / FT_T)), block(FT_THREADS);
  VSX_CHECK(grid.y <= 65535u, "vsx_rbf_block: at most %d rows per call (got %ld)", 65535 * FT_T, (long)(r1 - r0));
  hipStream_t s = (hipStream_t)stream;
  vsx_by_bool(ft_vec_ok(xc, d), [&](auto vec) {
    hipLaunchKernelGGL(mmd_rbf_block_kernel<decltype(vec)::value>, grid, block, 0, s, xc, norms, d, r0, r1, c0, c1, two_bw, zero_diag, out);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_sqdist_upper(const float* xc, const float* norms, int32_t M, int32_t d, float* out, vsx_stream_t stream) {
  VSX_CHECK(M >= 2 && M <= 65536, "vsx_sqdist_upper: M=%ld must be in [2, 65536]", (long)M);  // M (M - 1) / 2 < 2^31: one row of vsx_row_select
  VSX_CHECK(d >= 1 && d <= (1 << 20), "vsx_sqdist_upper: d=%ld must be in [1, 2^20]", (long)d);
  VSX_CHECK(xc && norms && out, "vsx_sqdist_upper: null argument");
  VSX_CHECK((((uintptr_t)xc | (uintptr_t)norms | (uintptr_t)out) & 3) == 0, "vsx_sqdist_upper: pointers must be 4-byte aligned");
  const unsigned nt = (unsigned)((M + FT_T - 1) / FT_T);
  const dim3 grid(nt, nt), block(FT_THREADS);
  hipStream_t s = (hipStream_t)stream;
  vsx_by_bool(ft_vec_ok(xc, d), [&](auto vec) {
    hipLaunchKernelGGL(mmd_sqdist_upper_kernel<decltype(vec)::value>, grid, block, 0, s, xc, norms, M, d, out);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}
