// viscy_amd — the float64 tile of dot products of fp32 rows (clustering.hip): a workgroup of DT_THREADS = 256 forms the
// DT_T x DT_T = 64 x 64 dots of 64 "query" rows with 64 "column" rows on the float64 MFMA (v_mfma_f64_16x16x4_f64).  Both
// operands are read as fp32, converted to float64 where they are staged in LDS, in chunks of DT_KC = 32 features; each of the
// four waves owns a 32 x 32 quadrant of four 16 x 16 accumulators (four float64 per lane each).  The product of two fp32 values
// is exact in float64, so a dot's only roundings are the accumulator's.
//
// Summation order.  A dot accumulates in float64 from +0.0, 32 features per chunk in ascending chunk order (features past d are
// zeros, which change nothing).  A chunk is eight MFMA steps of four features: the step (p, s), p = 0 .. 3 outer, s = 0 .. 1
// inner, takes features 8 p + 2 q + s of the chunk from lane quarter q = 0 .. 3 (the instruction's k index), for both operands
// alike, so that a lane fetches two steps' operands with one 16-byte LDS read; inside a step the hardware adds the four products
// to the accumulator in its own fixed order.  There is ONE order: the same for every (row, column), for either operand role
// (a product does not care which factor is the query), for every tile position and for every kernel built on dt_dots —
// vsx_row_sqnorm_f64 takes the diagonal of a tile whose two operands are the same rows, so norms[i] holds the bits that dot_ii
// holds in any tile, and the dot of two bit-identical rows equals both their norms.  What fixes the order is written once, here:
// the operand map and issue order (dt_dots) and the C/D map (dt_each).
#pragma once
#include "f32_tile.h"
#include "../../include/vsx.h"

constexpr int DT_T = VSX_F64_TILE;           // rows of either operand per tile
constexpr int DT_KC = VSX_F64_KC;            // features per staged chunk
constexpr int DT_LD = DT_KC + 2;             // doubles per staged row: keeps 16-byte alignment, shifts rows by four banks
constexpr int DT_THREADS = 256;
constexpr int DT_STAGE = 2 * DT_T * DT_LD;   // doubles of the staging area (query chunk | column chunk)
static_assert(DT_T == 64 && DT_KC == 32, "this header serves exactly this shape");

typedef double dt_f64x4 __attribute__((ext_vector_type(4)));

// wave (wq, wc) owns rows wq * 32 .., columns wc * 32 .. of the tile; r16 / q: the lane's place in the MFMA operand and C/D maps
struct DtLane {
  int t, wq, wc, r16, q;
};
__device__ __forceinline__ DtLane dt_lane() {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  return {t, wave & 1, wave >> 1, lane & 15, lane >> 4};
}
// C/D map of the 16 x 16 float64 MFMA (NOT the fp32 forms' map): element e of acc[a][b] is tile row wq * 32 + a * 16 + q + 4 e,
// tile column wc * 32 + b * 16 + r16.  f(dot, tile row, tile column) for the lane's 16 dots
template <class F>
__device__ __forceinline__ void dt_each(const dt_f64x4 (&acc)[2][2], const DtLane& l, F&& f) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) f(acc[a][b][e], l.wq * 32 + a * 16 + l.q + 4 * e, l.wc * 32 + b * 16 + l.r16);
}

// one thread's share of a chunk: 4 x 4 features; f = t + 256 u -> operand f >> 9, row (f & 511) >> 3, feature quad f & 7, so that
// 8 consecutive lanes read 128 contiguous bytes of one row.  load(operand, row in tile, feature) -> that row's four features
// from `feature` on, zeros where there are none
template <class Load>
__device__ __forceinline__ void dt_fetch(float4* r, int t, int kc0, Load&& load) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int f = t + DT_THREADS * u;
    r[u] = load(f >> 9, (f & 511) >> 3, kc0 + 4 * (f & 7));
  }
}

// acc = the tile's dots over nchunks >= 1 chunks of features.  stage: DT_STAGE doubles of LDS, 16-byte aligned.  LDS that the
// caller wrote before the call is visible after it; the caller puts a barrier between the return and a rewrite of `stage`.
template <class Load>
__device__ __forceinline__ void dt_dots(dt_f64x4 (&acc)[2][2], double* stage, const DtLane& l, int nchunks, Load&& load) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[a][b][e] = 0.0;
  float4 pre[4];
  dt_fetch(pre, l.t, 0, load);
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = l.t + DT_THREADS * u;
      double2* dst = reinterpret_cast<double2*>(stage + (size_t)(f >> 3) * DT_LD + 4 * (f & 7));  // row f >> 3 of [query | column]
      dst[0] = make_double2((double)pre[u].x, (double)pre[u].y);
      dst[1] = make_double2((double)pre[u].z, (double)pre[u].w);
    }
    __syncthreads();
    if (ch + 1 < nchunks) dt_fetch(pre, l.t, (ch + 1) * DT_KC, load);
    const double* qa = stage + (size_t)(l.wq * 32 + l.r16) * DT_LD + 2 * l.q;
    const double* cb = stage + (size_t)(DT_T + l.wc * 32 + l.r16) * DT_LD + 2 * l.q;
#pragma unroll
    for (int p = 0; p < DT_KC / 8; ++p) {
      const double2 a0 = *reinterpret_cast<const double2*>(qa + 8 * p);
      const double2 a1 = *reinterpret_cast<const double2*>(qa + 16 * DT_LD + 8 * p);
      const double2 b0 = *reinterpret_cast<const double2*>(cb + 8 * p);
      const double2 b1 = *reinterpret_cast<const double2*>(cb + 16 * DT_LD + 8 * p);
      const double av0[2] = {a0.x, a0.y}, av1[2] = {a1.x, a1.y}, bv0[2] = {b0.x, b0.y}, bv1[2] = {b1.x, b1.y};
#pragma unroll
      for (int s = 0; s < 2; ++s) {  // the issue order is part of every result
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0[s], bv0[s], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0[s], bv1[s], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1[s], bv0[s], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1[s], bv1[s], acc[1][1], 0, 0, 0);
      }
    }
  }
}
