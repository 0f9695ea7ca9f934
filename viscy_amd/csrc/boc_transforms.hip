// DynaCLR bag-of-channels augmentations (DESIGN §3 "row order statistics"):
//   vsx_row_select        exact per-row order statistics by radix select (BatchedScaleIntensityRangePercentiles' quantiles)
//   vsx_percentile_scale  the percentile rescale itself, every operation rounded separately as the tensor expressions are
//   vsx_crop_zreduce      per-sample crop window + Z max-projection / centre plane in one gather
#include "vsx_common.h"
#include "../../include/vsx.h"

// ------------------------------------------------------------------ radix select
// Four passes of 8 bits, most significant first.  State per (row, rank) slot in the caller's workspace:
//   hist[slots][256] | prefix[slots] | remaining[slots] | nan[rows]      (all uint32)
// prefix = the key bits resolved so far, remaining = the rank among the elements that carry this prefix.
#define RS_BITS 8
#define RS_BINS 256
#define RS_PASSES 4
#define RS_MAX_RANKS 4

struct RsRanks {
  uint32_t r[RS_MAX_RANKS];
};

// monotone float -> uint32: negative values have all bits flipped, the others the sign bit set (as atomic_minmax orders them)
__device__ __forceinline__ uint32_t rs_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rs_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void rs_init_kernel(uint32_t* __restrict__ ws, long slots, long rows, int nranks, RsRanks ranks) {
  uint32_t* prefix = ws + slots * RS_BINS;
  uint32_t* remaining = prefix + slots;
  uint32_t* nan = remaining + slots;
  const long total = slots * RS_BINS;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    ws[i] = 0u;
    if (i < slots) {
      prefix[i] = 0u;
      remaining[i] = ranks.r[i % nranks];
    }
    if (i < rows) nan[i] = 0u;
  }
}

// one element into the LDS histograms of the ranks whose prefix it carries (a rank that shares its prefix with an earlier one
// is counted once, under that one: `rep`)
template <bool FIRST>
__device__ __forceinline__ void rs_count(float v, uint32_t (*h)[RS_BINS], const uint32_t* pre, const int* rep, int nranks, int shift,
                                         uint32_t& saw_nan) {
  const uint32_t key = rs_key(v);
  const uint32_t bin = (key >> shift) & (RS_BINS - 1);
  if (FIRST) {
    saw_nan |= (v != v) ? 1u : 0u;
    atomicAdd(&h[0][bin], 1u);
  } else {
    const uint32_t high = key >> (shift + RS_BITS);
#pragma unroll
    for (int r = 0; r < RS_MAX_RANKS; ++r)
      if (r < nranks && rep[r] == r && high == pre[r]) atomicAdd(&h[r][bin], 1u);
  }
}

// grid = rows * gx workgroups; workgroup (row, bx) counts vectors bx*256 + t, step gx*256, of the row's 16-byte aligned body and,
// for bx == 0, the scalar head and tail around it
template <bool FIRST>
__global__ __launch_bounds__(256) void rs_hist_kernel(const float* __restrict__ x, uint32_t* __restrict__ ws, long slots, long n,
                                                      int nranks, int gx, int shift) {
  __shared__ uint32_t h[RS_MAX_RANKS][RS_BINS];
  __shared__ uint32_t pre[RS_MAX_RANKS];
  __shared__ int rep[RS_MAX_RANKS];
  const int t = threadIdx.x;
  const long row = blockIdx.x / gx;
  const int bx = (int)(blockIdx.x - row * gx);
  uint32_t* prefix = ws + slots * RS_BINS;
  uint32_t* nan = prefix + 2 * slots;
#pragma unroll
  for (int r = 0; r < RS_MAX_RANKS; ++r) h[r][t] = 0u;
  if (t == 0) {
    for (int r = 0; r < RS_MAX_RANKS; ++r) {
      pre[r] = (!FIRST && r < nranks) ? prefix[row * nranks + r] : 0u;
      rep[r] = r;
      for (int q = r - 1; q >= 0; --q)
        if (r < nranks && pre[q] == pre[r]) rep[r] = q;
    }
    if (FIRST)
      for (int r = 1; r < RS_MAX_RANKS; ++r) rep[r] = 0;
  }
  __syncthreads();
  const float* xs = x + row * n;
  long head = (long)(((16u - (uint32_t)((uintptr_t)xs & 15u)) & 15u) >> 2);  // floats up to the first 16-byte boundary
  if (head > n) head = n;
  const long nvec = (n - head) >> 2;
  const long tail0 = head + 4 * nvec;
  uint32_t saw_nan = 0u;
  const float4* xv = reinterpret_cast<const float4*>(xs + head);
  for (long i = (long)bx * 256 + t; i < nvec; i += (long)gx * 256) {
    const float4 v = xv[i];
    rs_count<FIRST>(v.x, h, pre, rep, nranks, shift, saw_nan);
    rs_count<FIRST>(v.y, h, pre, rep, nranks, shift, saw_nan);
    rs_count<FIRST>(v.z, h, pre, rep, nranks, shift, saw_nan);
    rs_count<FIRST>(v.w, h, pre, rep, nranks, shift, saw_nan);
  }
  if (bx == 0) {
    if (t < head) rs_count<FIRST>(xs[t], h, pre, rep, nranks, shift, saw_nan);
    if (t >= 4 && tail0 + (t - 4) < n) rs_count<FIRST>(xs[tail0 + (t - 4)], h, pre, rep, nranks, shift, saw_nan);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RS_MAX_RANKS; ++r) {
    if (r < nranks) {
      const uint32_t c = h[rep[r]][t];
      if (c) atomicAdd(ws + (row * nranks + r) * RS_BINS + t, c);
    }
  }
  if (FIRST && saw_nan) atomicOr(nan + row, 1u);
}

// one workgroup per (row, rank): the bin that holds the rank extends the prefix; the histogram is cleared for the next pass.
// LAST: the prefix is the whole key, which goes to out (NaN where the row holds one).
__global__ __launch_bounds__(256) void rs_scan_kernel(uint32_t* __restrict__ ws, float* __restrict__ out, long slots, int nranks,
                                                      int last) {
  __shared__ uint32_t inc[RS_BINS];
  const int t = threadIdx.x;
  const long slot = blockIdx.x;
  uint32_t* hist = ws + slot * RS_BINS;
  uint32_t* prefix = ws + slots * RS_BINS;
  uint32_t* remaining = prefix + slots;
  const uint32_t* nan = remaining + slots;
  const uint32_t c = hist[t];
  const uint32_t pre = prefix[slot], rem = remaining[slot];
  hist[t] = 0u;
  inc[t] = c;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < RS_BINS; o <<= 1) {  // inclusive scan over the 256 bins
    const uint32_t a = t >= o ? inc[t - o] : 0u;
    __syncthreads();
    inc[t] += a;
    __syncthreads();
  }
  const uint32_t below = inc[t] - c;
  if (rem >= below && rem < inc[t]) {  // exactly one bin: the counts of a slot sum to more than its remaining rank
    const uint32_t p = (pre << RS_BITS) | (uint32_t)t;
    prefix[slot] = p;
    remaining[slot] = rem - below;
    if (last) out[slot] = nan[slot / nranks] ? __uint_as_float(0x7fc00000u) : rs_unkey(p);
  }
}

extern "C" int64_t vsx_row_select_ws_bytes(int64_t rows, int32_t nranks) {
  if (rows < 1 || nranks < 1 || nranks > RS_MAX_RANKS) return 0;
  return 4 * (rows * nranks * (RS_BINS + 2) + rows);
}

/* out[row][k] = the element torch.sort(x[row]).values[ranks[k]] holds; NaN for every rank of a row that holds a NaN. */
extern "C" int32_t vsx_row_select(const float* x, float* out, void* ws, int64_t ws_bytes, int64_t rows, int64_t n,
                                  const int64_t* ranks, int32_t nranks, vsx_stream_t stream) {
  VSX_CHECK(x && out && ws && ranks, "vsx_row_select: null argument");
  VSX_CHECK(((uintptr_t)x & 3u) == 0 && ((uintptr_t)ws & 3u) == 0, "vsx_row_select: x and ws must be 4-byte aligned");
  VSX_CHECK(rows >= 1 && n >= 1 && n <= 2147483647LL, "vsx_row_select: rows >= 1 and 1 <= n <= 2^31 - 1 (rows %ld, n %ld)", (long)rows, (long)n);
  VSX_CHECK(nranks >= 1 && nranks <= RS_MAX_RANKS, "vsx_row_select: 1 to %d ranks (got %d)", RS_MAX_RANKS, nranks);
  RsRanks rk = {{0u, 0u, 0u, 0u}};
  for (int k = 0; k < nranks; ++k) {
    VSX_CHECK(ranks[k] >= 0 && ranks[k] < n, "vsx_row_select: rank %ld outside [0, %ld)", (long)ranks[k], (long)n);
    rk.r[k] = (uint32_t)ranks[k];
  }
  VSX_CHECK(ws_bytes >= vsx_row_select_ws_bytes(rows, nranks), "vsx_row_select: workspace of %ld bytes, %ld needed", (long)ws_bytes,
            (long)vsx_row_select_ws_bytes(rows, nranks));
  // workgroups per row: 8 vectors per thread, about 4096 workgroups in flight over all rows
  long gx = ((n >> 2) + 256L * 8 - 1) / (256L * 8);
  const long cap = 4096 / rows > 1 ? 4096 / rows : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  VSX_CHECK(rows * gx <= 2147483647LL && rows * nranks <= 2147483647LL, "vsx_row_select: too many rows (%ld)", (long)rows);
  const long slots = rows * nranks;
  uint32_t* w = (uint32_t*)ws;
  hipStream_t s = (hipStream_t)stream;
  int gi = vsx_cdiv(slots * RS_BINS, 256);
  if (gi > 4096) gi = 4096;
  hipLaunchKernelGGL(rs_init_kernel, dim3(gi), dim3(256), 0, s, w, slots, (long)rows, (int)nranks, rk);
  for (int p = 0; p < RS_PASSES; ++p) {
    const int shift = 32 - RS_BITS * (p + 1);
    vsx_by_bool(p == 0, [&](auto first) {
      hipLaunchKernelGGL(rs_hist_kernel<decltype(first)::value>, dim3((unsigned)(rows * gx)), dim3(256), 0, s, x, w, slots, (long)n, (int)nranks,
                         (int)gx, shift);
    });
    hipLaunchKernelGGL(rs_scan_kernel, dim3((unsigned)slots), dim3(256), 0, s, w, out, slots, (int)nranks, (int)(p == RS_PASSES - 1));
  }
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ percentile rescale
// y = (x - a_min) / (a_max - a_min)  [* (b_max - b_min) + b_min]  [clip]; where degenerate[row] is set: y = x - a_min [+ b_min].
// Every operation is rounded on its own, like the tensor expression it restates: contraction off, IEEE division.
struct PsArgs {
  float b_min, b_max, b_span;
  int flags;  // 1: rescale to [b_min, b_max]; 2: clip below at b_min; 4: clip above at b_max; 8: b_min is added in the degenerate branch
};

#pragma clang fp contract(off)
__device__ __forceinline__ float ps_one(float v, float lo, float hi, int deg, const PsArgs& a) {
#pragma clang fp contract(off)
  if (deg) {
    float r = v - lo;
    if (a.flags & 8) r = r + a.b_min;
    return r;
  }
  const float d = hi - lo;
  float r = (v - lo) / d;
  if (a.flags & 1) {
    r = r * a.b_span;
    r = r + a.b_min;
  }
  if ((a.flags & 2) && r < a.b_min) r = a.b_min;  // comparisons, not fmin / fmax: a NaN stays one, as in torch.clip
  if ((a.flags & 4) && r > a.b_max) r = a.b_max;
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void percentile_scale_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               const float* __restrict__ a_min, const float* __restrict__ a_max,
                                                               const int* __restrict__ degenerate, long n, long total, PsArgs a) {
  if (VEC) {
    const long nvec = total >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
      const long e = i * 4;
      long row = e / n;
      long next = (row + 1) * n;  // first element of the following row
      float lo = a_min[row], hi = a_max[row];
      int dg = degenerate[row];
      float4 v = reinterpret_cast<const float4*>(x)[i];
      float* p = &v.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e + j >= next) {  // n >= 1: at most one row boundary per element
          ++row;
          next += n;
          lo = a_min[row];
          hi = a_max[row];
          dg = degenerate[row];
        }
        p[j] = ps_one(p[j], lo, hi, dg, a);
      }
      reinterpret_cast<float4*>(y)[i] = v;
    }
    const long e = (nvec << 2) + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && e < total) {
      const long row = e / n;
      y[e] = ps_one(x[e], a_min[row], a_max[row], degenerate[row], a);
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const long row = e / n;
      y[e] = ps_one(x[e], a_min[row], a_max[row], degenerate[row], a);
    }
  }
}

extern "C" int32_t vsx_percentile_scale(const float* x, float* y, const float* a_min, const float* a_max, const int32_t* degenerate,
                                        int64_t rows, int64_t n, double b_min, double b_max, int32_t flags, vsx_stream_t stream) {
  VSX_CHECK(x && y && a_min && a_max && degenerate && rows >= 1 && n >= 1, "vsx_percentile_scale: bad arguments");
  VSX_CHECK(flags >= 0 && flags <= 15, "vsx_percentile_scale: flags is a 4-bit mask");
  VSX_CHECK(rows <= (int64_t)0x7fffffffffffffffLL / n, "vsx_percentile_scale: rows * n overflows");
  const long total = rows * n;
  // the scalars reach the tensor expression as Python floats: differences in double, then one rounding to float32
  PsArgs a = {(float)b_min, (float)b_max, (float)(b_max - b_min), (int)flags};
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15u) == 0;
  int g = vsx_cdiv(vec ? (total + 3) / 4 : total, 256L * 4);
  g = g > 8192 ? 8192 : (g < 1 ? 1 : g);
  vsx_by_bool(vec, [&](auto vec_) {
    hipLaunchKernelGGL(percentile_scale_kernel<decltype(vec_)::value>, dim3(g), dim3(256), 0, (hipStream_t)stream, x, y, a_min, a_max, degenerate,
                       (long)n, total, a);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ crop window + Z reduction
// y[b, c, 0, yy, xx] = mode[b] ? x[b, c, z0 + cz / 2, y0 + yy, x0 + xx] : max over z < cz of x[b, c, z0 + z, y0 + yy, x0 + xx]
// (z0, y0, x0) = starts[b] clamped into [0, dim - c]; the maximum keeps a NaN, as amax does.  Only the window is read.
__global__ __launch_bounds__(256) void crop_zreduce_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int* __restrict__ starts, const int* __restrict__ mode, int B, int C,
                                                           int Z, int Y, int X, int cz, int cy, int cx) {
  const long total = (long)B * C * cy * cx;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int xx = (int)(i % cx);
    long r = i / cx;
    const int yy = (int)(r % cy);
    r /= cy;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    int z0 = 0, y0 = 0, x0 = 0;
    if (starts) {
      z0 = min(max(starts[3 * b], 0), Z - cz);
      y0 = min(max(starts[3 * b + 1], 0), Y - cy);
      x0 = min(max(starts[3 * b + 2], 0), X - cx);
    }
    const size_t plane = (size_t)Y * X;
    const float* src = x + (((size_t)b * C + c) * Z + z0) * plane + (size_t)(y0 + yy) * X + x0 + xx;
    float m;
    if (mode[b]) {
      m = src[(size_t)(cz / 2) * plane];
    } else {
      m = src[0];
      for (int z = 1; z < cz; ++z) {
        const float v = src[(size_t)z * plane];
        m = (v > m || v != v) ? v : m;
      }
    }
    y[i] = m;
  }
}

extern "C" int32_t vsx_crop_zreduce(const float* x, float* y, const int32_t* starts, const int32_t* mode, int32_t B, int32_t C,
                                    int32_t Z, int32_t Y, int32_t X, int32_t cz, int32_t cy, int32_t cx, vsx_stream_t stream) {
  VSX_CHECK(x && y && mode && B > 0 && C > 0 && cz > 0 && cy > 0 && cx > 0 && cz <= Z && cy <= Y && cx <= X,
            "vsx_crop_zreduce: bad arguments (window (%d,%d,%d) in (%d,%d,%d))", cz, cy, cx, Z, Y, X);
  const long total = (long)B * C * cy * cx;
  int g = vsx_cdiv(total, 256);
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(crop_zreduce_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, y, starts, mode, B, C, Z, Y, X, cz, cy, cx);
  VSX_LAUNCH_CHECK();
  return 0;
}
