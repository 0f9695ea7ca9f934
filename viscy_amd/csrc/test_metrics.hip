// viscy_amd — the device passes of the test stage (cytoland/engine.py:334-392): the sums behind MAE / MSE / cosine / Pearson / R2 of
// an image pair in one read, and SSIM over the windows that lie inside the image (torchmetrics' structural_similarity_index_measure
// after it has cropped its padding).
//
//   vsx_pair_sums     out[13] = sums, extrema and the row-cosine sum of a strided pair of fp32 image stacks      float64 throughout
//   vsx_ssim_window   sums[plane] = sum of the plane's SSIM map (separable window weights, fp32 map, float64 sum), optional map
//
// No atomics.  Every output is a pure function of the inputs, the strides' alignment and the shape, bit-identical from run to run:
// a lane adds its elements in ascending order, the lanes of a wave by the xor butterfly 32 .. 1, the waves of a workgroup and the
// workgroups' partials in index order (the fold cuts the list into PS_FOLD_SEGS / SS_FOLD_SEGS runs first: a fixed association).
#include "vsx_common.h"
#include "../../include/vsx.h"

#define PS_WAVES VSX_PAIR_SUMS_WAVES
#define PS_Q VSX_PAIR_SUMS
#define PS_MAX_WGS VSX_PAIR_SUMS_MAX_WGS
#define PS_FOLD_SEGS 16
static_assert(VSX_PAIR_SUMS_VEC == 4, "a lane loads one float4");
static_assert(PS_Q <= 16, "the fold keeps a quantity per lane of a 16-lane row");

// quantities 7 .. 10 are extrema (min p, max p, min t, max t); every other one is a sum
__device__ __forceinline__ double ps_join(int q, double a, double b) {
  if (q == 7 || q == 9) return fmin(a, b);
  if (q == 8 || q == 10) return fmax(a, b);
  return a + b;
}
__device__ __forceinline__ double ps_identity(int q) {
  if (q == 7 || q == 9) return (double)INFINITY;
  if (q == 8 || q == 10) return -(double)INFINITY;
  return 0.0;
}

struct PsLane {
  double sp, st, sabs, sd2;    // over every element the lane has seen
  double rpp, rtt, rpt;        // over the lane's elements of the row in hand
  float mnp, mxp, mnt, mxt;
};
// fp32 x fp32 and fp32 - fp32 are exact in float64: each fma below is one rounding, of the add
__device__ __forceinline__ void ps_take(PsLane& a, float pf, float tf) {
  const double p = (double)pf, t = (double)tf, d = p - t;
  a.sp += p;
  a.st += t;
  a.sabs += fabs(d);
  a.sd2 = fma(d, d, a.sd2);
  a.rpp = fma(p, p, a.rpp);
  a.rtt = fma(t, t, a.rtt);
  a.rpt = fma(p, t, a.rpt);
  a.mnp = fminf(a.mnp, pf), a.mxp = fmaxf(a.mxp, pf);
  a.mnt = fminf(a.mnt, tf), a.mxt = fmaxf(a.mxt, tf);
}

// wave w of workgroup g takes rows g * PS_WAVES + w, + gridDim.x * PS_WAVES, ...; part [gridDim.x][PS_Q]
__global__ __launch_bounds__(PS_WAVES * 64) void ps_partial_kernel(const float* __restrict__ P, long pps, long prs, const float* __restrict__ T,
                                                                   long tps, long trs, long rows, int H, int W, double* __restrict__ part) {
  __shared__ double sh[PS_WAVES][PS_Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PsLane a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY};
  double wpp = 0.0, wtt = 0.0, wpt = 0.0, wcos = 0.0, wrows = 0.0;  // the wave's rows, the same in every lane
  for (long r = (long)blockIdx.x * PS_WAVES + wave; r < rows; r += (long)gridDim.x * PS_WAVES) {
    const long pl = r / H;
    const long y = r - pl * H;
    const float* p = P + pl * pps + y * prs;
    const float* t = T + pl * tps + y * trs;
    a.rpp = a.rtt = a.rpt = 0.0;
    int done = 0;
    if ((((uintptr_t)p | (uintptr_t)t) & 15) == 0) {  // uniform over the wave
      done = W & ~3;
      int c = 4 * lane;
      for (; c + 256 < done; c += 512) {  // two vectors of each image in flight; the elements are still taken in ascending order
        const float4 p0 = *reinterpret_cast<const float4*>(p + c), t0 = *reinterpret_cast<const float4*>(t + c);
        const float4 p1 = *reinterpret_cast<const float4*>(p + c + 256), t1 = *reinterpret_cast<const float4*>(t + c + 256);
        ps_take(a, p0.x, t0.x), ps_take(a, p0.y, t0.y), ps_take(a, p0.z, t0.z), ps_take(a, p0.w, t0.w);
        ps_take(a, p1.x, t1.x), ps_take(a, p1.y, t1.y), ps_take(a, p1.z, t1.z), ps_take(a, p1.w, t1.w);
      }
      for (; c < done; c += 256) {
        const float4 pv = *reinterpret_cast<const float4*>(p + c), tv = *reinterpret_cast<const float4*>(t + c);
        ps_take(a, pv.x, tv.x), ps_take(a, pv.y, tv.y), ps_take(a, pv.z, tv.z), ps_take(a, pv.w, tv.w);
      }
    }
    for (int c = done + lane; c < W; c += 64) ps_take(a, p[c], t[c]);
    const double rpp = wave_sum_f64(a.rpp), rtt = wave_sum_f64(a.rtt), rpt = wave_sum_f64(a.rpt);
    wpp += rpp, wtt += rtt, wpt += rpt;
    wcos += rpt / (fmax(sqrt(rpp), 1e-8) * fmax(sqrt(rtt), 1e-8));
    wrows += 1.0;
  }
  double v[PS_Q];
  v[0] = wave_sum_f64(a.sp), v[1] = wave_sum_f64(a.st), v[2] = wpp, v[3] = wtt, v[4] = wpt;
  v[5] = wave_sum_f64(a.sabs), v[6] = wave_sum_f64(a.sd2);
  float mnp = a.mnp, mxp = a.mxp, mnt = a.mnt, mxt = a.mxt;
  for (int o = 32; o > 0; o >>= 1) {
    mnp = fminf(mnp, __shfl_xor(mnp, o, 64)), mxp = fmaxf(mxp, __shfl_xor(mxp, o, 64));
    mnt = fminf(mnt, __shfl_xor(mnt, o, 64)), mxt = fmaxf(mxt, __shfl_xor(mxt, o, 64));
  }
  v[7] = mnp, v[8] = mxp, v[9] = mnt, v[10] = mxt, v[11] = wcos, v[12] = wrows;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < PS_Q; ++q) sh[wave][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < PS_Q) {
    const int q = threadIdx.x;
    double tot = sh[0][q];
    for (int w = 1; w < PS_WAVES; ++w) tot = ps_join(q, tot, sh[w][q]);
    part[(size_t)blockIdx.x * PS_Q + q] = tot;
  }
}

// thread (q, s) joins run s of the workgroups' partials in ascending order; thread (q, 0) then joins the runs in ascending order
__global__ __launch_bounds__(256) void ps_fold_kernel(const double* __restrict__ part, int wgs, double* __restrict__ out) {
  __shared__ double run[PS_FOLD_SEGS][16];
  const int q = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int len = (wgs + PS_FOLD_SEGS - 1) / PS_FOLD_SEGS;
  if (q < PS_Q) {
    double tot = ps_identity(q);
    const int g1 = min((s + 1) * len, wgs);
    for (int g = s * len; g < g1; ++g) tot = ps_join(q, tot, part[(size_t)g * PS_Q + q]);
    run[s][q] = tot;
  }
  __syncthreads();
  if (s == 0 && q < PS_Q) {
    double tot = run[0][q];
    for (int k = 1; k < PS_FOLD_SEGS; ++k) tot = ps_join(q, tot, run[k][q]);
    out[q] = tot;
  }
}

// ------------------------------------------------------------------ windowed SSIM
#define SS_TS VSX_SSIM_TILE              // a workgroup's outputs: SS_TS x SS_TS, worked in two halves of SS_HR rows
#define SS_HR (SS_TS / 2)
#define SS_MAXK VSX_SSIM_MAX_K
#define SS_HW (SS_TS + SS_MAXK - 1)      // staged columns, at most
#define SS_HH (SS_HR + SS_MAXK - 1)      // staged rows, at most
#define SS_FOLD_SEGS 256
static_assert(SS_TS == 32, "a half-wave is a row of outputs: the LDS images below are conflict-free for 32 columns");

// the window's five means -> SSIM, every product, sum and the quotient rounded once (no contraction: for p == t the numerator and
// the denominator are the same two factors, bit for bit)
__device__ __forceinline__ float ss_formula(float mx, float my, float exx, float eyy, float exy, float sp, float st, float c1, float c2) {
#pragma clang fp contract(off)
  const float vxx = fmaxf(exx - mx * mx, 0.f), vyy = fmaxf(eyy - my * my, 0.f), vxy = exy - mx * my;
  const float mp = mx + sp, mt = my + st;
  const float a = mp * mt, pp = mp * mp, tt = mt * mt;
  const float num = (2.f * a + c1) * (2.f * vxy + c2);
  const float den = ((pp + tt) + c1) * ((vxx + vyy) + c2);
  return num / den;
}

// workgroup = (plane, tile); part [planes][tiles]
__global__ __launch_bounds__(256) void ss_tile_kernel(const float* __restrict__ P, long pps, long prs, const float* __restrict__ T, long tps, long trs,
                                                      int H, int W, const float* __restrict__ wy, int Ky, const float* __restrict__ wx, int Kx,
                                                      const float* __restrict__ cc, const float* __restrict__ shift, int tiles_x, int tiles,
                                                      double* __restrict__ part, float* __restrict__ map) {
  __shared__ float xs[SS_HH][SS_HW + 1], ys[SS_HH][SS_HW + 1];  // the centred halo tiles
  __shared__ float hs[5][SS_HH][SS_TS + 1];                     // after the pass along X: E_x of x, y, x^2, y^2, x y
  __shared__ float wxs[SS_MAXK], wys[SS_MAXK];
  __shared__ double red[256];
  const int t = threadIdx.x;
  const long plane = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - plane * tiles);
  const int OH = H - Ky + 1, OW = W - Kx + 1;
  const int ox0 = (tile % tiles_x) * SS_TS, oy_tile = (tile / tiles_x) * SS_TS;
  const int cols = min(SS_TS, OW - ox0), hc = cols + Kx - 1;
  const float sp = shift[0], st = shift[1], c1 = cc[0], c2 = cc[1];
  if (t < Kx) wxs[t] = wx[t];
  if (t >= 64 && t - 64 < Ky) wys[t - 64] = wy[t - 64];
  const float* Pp = P + plane * pps;
  const float* Tp = T + plane * tps;
  double acc = 0.0;
  for (int half = 0; half < 2; ++half) {
    const int oy0 = oy_tile + half * SS_HR;
    if (oy0 >= OH) break;  // uniform
    const int rows = min(SS_HR, OH - oy0), hr = rows + Ky - 1;
    // input rows oy0 .. oy0 + hr - 1 <= H - 1 and columns ox0 .. ox0 + hc - 1 <= W - 1: a window inside the plane needs no padding
    for (int i = t; i < hr * hc; i += 256) {
      const int j = i / hc, c = i - j * hc;
      xs[j][c] = Pp[(long)(oy0 + j) * prs + ox0 + c] - sp;
      ys[j][c] = Tp[(long)(oy0 + j) * trs + ox0 + c] - st;
    }
    __syncthreads();
    for (int i = t; i < hr * SS_TS; i += 256) {
      const int j = i >> 5, c = i & 31;
      if (c < cols) {
        float ex = 0.f, ey = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
        for (int k = 0; k < Kx; ++k) {
          const float w = wxs[k], a = xs[j][c + k], b = ys[j][c + k];
          const float wa = w * a, wb = w * b;
          ex += wa, ey += wb;
          exx = fmaf(wa, a, exx), eyy = fmaf(wb, b, eyy), exy = fmaf(wa, b, exy);
        }
        hs[0][j][c] = ex, hs[1][j][c] = ey, hs[2][j][c] = exx, hs[3][j][c] = eyy, hs[4][j][c] = exy;
      }
    }
    __syncthreads();
    for (int i = t; i < SS_HR * SS_TS; i += 256) {
      const int oy = i >> 5, ox = i & 31;
      if (oy < rows && ox < cols) {
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < Ky; ++k) {
          const float w = wys[k];
#pragma unroll
          for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hs[q][oy + k][ox], m[q]);
        }
        const float s = ss_formula(m[0], m[1], m[2], m[3], m[4], sp, st, c1, c2);
        if (map) map[(plane * OH + oy0 + oy) * (long)OW + ox0 + ox] = s;
        acc += (double)s;
      }
    }
    // the next half stages xs / ys, which nobody reads after the barrier above, and writes hs only after its own first barrier
  }
  red[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = red[0];
}

// one workgroup per plane: thread s adds run s of the plane's tile partials in ascending order, then the binary tree over the runs
__global__ __launch_bounds__(SS_FOLD_SEGS) void ss_fold_kernel(const double* __restrict__ part, int tiles, double* __restrict__ sums) {
  __shared__ double red[SS_FOLD_SEGS];
  const int s = threadIdx.x;
  const int len = (tiles + SS_FOLD_SEGS - 1) / SS_FOLD_SEGS;
  const double* mine = part + (size_t)blockIdx.x * tiles;
  double tot = 0.0;
  const int g1 = min((s + 1) * len, tiles);
  for (int g = s * len; g < g1; ++g) tot += mine[g];
  red[s] = tot;
  __syncthreads();
  for (int o = SS_FOLD_SEGS / 2; o > 0; o >>= 1) {
    if (s < o) red[s] += red[s + o];
    __syncthreads();
  }
  if (s == 0) sums[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------ host
static bool tm_shape_ok(int64_t planes, int32_t H, int32_t W) {
  return planes >= 1 && H >= 1 && W >= 1 && planes <= ((int64_t)1 << 40) / H;  // rows = planes * H fits easily in a long
}
static int ps_wgs(int64_t planes, int32_t H) {
  const int64_t want = (planes * H + PS_WAVES - 1) / PS_WAVES;
  return (int)(want < PS_MAX_WGS ? want : PS_MAX_WGS);
}

extern "C" int64_t vsx_pair_sums_ws_bytes(int64_t planes, int32_t H) {
  if (!tm_shape_ok(planes, H, 1)) return 0;
  return (int64_t)ps_wgs(planes, H) * PS_Q * 8;
}

extern "C" int32_t vsx_pair_sums(const float* P, int64_t pps, int64_t prs, const float* T, int64_t tps, int64_t trs, int64_t planes, int32_t H,
                                 int32_t W, double* out, void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  VSX_CHECK(tm_shape_ok(planes, H, W), "vsx_pair_sums: planes=%ld, H=%ld, W=%ld must be at least 1", (long)planes, (long)H, (long)W);
  VSX_CHECK(P && T && out && ws, "vsx_pair_sums: null argument");
  VSX_CHECK(pps >= 0 && prs >= 0 && tps >= 0 && trs >= 0, "vsx_pair_sums: strides must not be negative");
  VSX_CHECK((((uintptr_t)P | (uintptr_t)T) & 3) == 0 && (((uintptr_t)out | (uintptr_t)ws) & 7) == 0,
            "vsx_pair_sums: P and T must be 4-byte aligned, out and ws 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_pair_sums_ws_bytes(planes, H), "vsx_pair_sums: the workspace must hold vsx_pair_sums_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_pair_sums_ws_bytes(planes, H), (long)ws_bytes);
  const int wgs = ps_wgs(planes, H);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  hipLaunchKernelGGL(ps_partial_kernel, dim3((unsigned)wgs), dim3(PS_WAVES * 64), 0, st, P, (long)pps, (long)prs, T, (long)tps, (long)trs,
                     (long)(planes * H), H, W, part);
  hipLaunchKernelGGL(ps_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)part, wgs, out);
  VSX_LAUNCH_CHECK();
  return 0;
}

static bool ss_window_ok(int32_t K) { return K >= 3 && K <= SS_MAXK && (K & 1); }
// tiles of one plane, or 0 where the arguments are refused
static int64_t ss_tiles(int64_t planes, int32_t H, int32_t W, int32_t Ky, int32_t Kx, int* tiles_x) {
  if (!tm_shape_ok(planes, H, W) || !ss_window_ok(Ky) || !ss_window_ok(Kx) || H < Ky || W < Kx) return 0;
  const int64_t tx = (W - Kx + 1 + SS_TS - 1) / SS_TS, ty = (H - Ky + 1 + SS_TS - 1) / SS_TS;
  if (tx * ty > ((int64_t)1 << 31) - 1 || planes * tx * ty > ((int64_t)1 << 31) - 1) return 0;
  if (tiles_x) *tiles_x = (int)tx;
  return tx * ty;
}

extern "C" int64_t vsx_ssim_window_ws_bytes(int64_t planes, int32_t H, int32_t W, int32_t Ky, int32_t Kx) {
  return planes * ss_tiles(planes, H, W, Ky, Kx, nullptr) * 8;
}

extern "C" int32_t vsx_ssim_window(const float* P, int64_t pps, int64_t prs, const float* T, int64_t tps, int64_t trs, int64_t planes, int32_t H,
                                   int32_t W, const float* wy, int32_t Ky, const float* wx, int32_t Kx, const float* c, const float* shift,
                                   double* sums, float* map, void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  VSX_CHECK(tm_shape_ok(planes, H, W), "vsx_ssim_window: planes=%ld, H=%ld, W=%ld must be at least 1", (long)planes, (long)H, (long)W);
  VSX_CHECK(ss_window_ok(Ky) && ss_window_ok(Kx), "vsx_ssim_window: Ky=%ld, Kx=%ld must be odd and in [3, %d]", (long)Ky, (long)Kx, SS_MAXK);
  VSX_CHECK(H >= Ky && W >= Kx, "vsx_ssim_window: a %ldx%ld plane holds no %ldx%ld window", (long)H, (long)W, (long)Ky, (long)Kx);
  VSX_CHECK(P && T && wy && wx && c && shift && sums && ws, "vsx_ssim_window: null argument");
  VSX_CHECK(pps >= 0 && prs >= 0 && tps >= 0 && trs >= 0, "vsx_ssim_window: strides must not be negative");
  VSX_CHECK((((uintptr_t)P | (uintptr_t)T | (uintptr_t)wy | (uintptr_t)wx | (uintptr_t)c | (uintptr_t)shift | (uintptr_t)map) & 3) == 0 &&
                (((uintptr_t)sums | (uintptr_t)ws) & 7) == 0,
            "vsx_ssim_window: fp32 arguments must be 4-byte aligned, sums and ws 8-byte aligned");
  int tiles_x = 0;
  const int64_t tiles = ss_tiles(planes, H, W, Ky, Kx, &tiles_x);
  VSX_CHECK(tiles > 0, "vsx_ssim_window: %ld planes of %ldx%ld are more than 2^31 - 1 tiles", (long)planes, (long)H, (long)W);
  VSX_CHECK(ws_bytes >= planes * tiles * 8, "vsx_ssim_window: the workspace must hold vsx_ssim_window_ws_bytes = %ld bytes (got %ld)",
            (long)(planes * tiles * 8), (long)ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  hipLaunchKernelGGL(ss_tile_kernel, dim3((unsigned)(planes * tiles)), dim3(256), 0, st, P, (long)pps, (long)prs, T, (long)tps, (long)trs, H, W, wy,
                     Ky, wx, Kx, c, shift, tiles_x, (int)tiles, part, map);
  hipLaunchKernelGGL(ss_fold_kernel, dim3((unsigned)planes), dim3(SS_FOLD_SEGS), 0, st, (const double*)part, (int)tiles, sums);
  VSX_LAUNCH_CHECK();
  return 0;
}
