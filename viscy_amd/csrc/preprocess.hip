// viscy_amd — the device passes of `viscy preprocess` (viscy_utils/meta_utils.py generate_normalization_metadata / generate_fg_masks,
// viscy_utils/mp_utils.py get_val_stats; host layer: viscy_amd/preprocess.py):
//
//   vsx_grid_sample   out[z, i, j] = (float) src[z, i g, j g]                       what numpy's `::g` slice yields, fp32
//   vsx_median3x3     3 x 3 median per plane, scipy's mode="reflect"                fp32 out, or the uint8 mask `median >= thr`
//   vsx_nan_moments   count / min / max / sum of the non-NaN values, then the centred sums about a given mean      float64 / int64
//   vsx_hist_int      counts of integer-valued fp32 values, one bin per integer     uint64
//   vsx_hist_edges    counts between caller-supplied ascending edges                uint64, np.histogram's rule
//
// A source plane set is [Z, H, W] of VSX_PG_F32 / U16 / I16 / U8 with element strides for z and y, x contiguous: a view into a
// [T, C, Z, H, W] block serves as it is.  Integer sources convert to fp32 exactly, float32 travels as 32-bit integers where it is only
// copied (grid sample).  The median ASSUMES NaN-free input (scipy's result with a NaN is unspecified as well); of -0.0 and +0.0, which
// compare equal, either may come back.
// No floating-point atomics.  The sums are per-chunk partials written by plain stores (every word is written before it is read: the
// workspace needs no initialisation) and folded in a fixed order; the histograms add integers.  Every output is bit-identical from
// run to run.  No allocation, synchronisation or device-to-host copy; every check runs before any launch.
#include "src_frame.h"

#define MED_COLS VSX_MEDIAN_COLS        // output columns of a wave: lanes 1 .. 62 of the 64 loaded columns
#define MED_ROWS VSX_MEDIAN_ROWS        // output rows a wave walks down before it moves to its next strip
#define MOM_CHUNK VSX_MOMENTS_CHUNK     // values per workgroup partial
#define MOM_FOLD_SEGS 256
#define HIST_LDS_BINS VSX_HIST_LDS_BINS
static_assert(MED_COLS == 62, "a wave loads 64 columns: its outputs and one halo column on each side");
static_assert(MOM_CHUNK % 1024 == 0, "256 threads take float4 vectors round by round");

// ------------------------------------------------------------------ grid sample
template <typename T>
__global__ __launch_bounds__(256) void grid_sample_kernel(const T* __restrict__ src, long sz, long sy, int ho, int wo, int g, long total,
                                                          uint32_t* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % wo);
    const long r = i / wo;
    const int y = (int)(r % ho);
    const long z = r / ho;
    out[i] = vsx_src_bits_at<T>(src + z * sz + (long)y * g * sy + (long)x * g);  // y g <= H - 1, x g <= W - 1
  }
}

extern "C" int32_t vsx_grid_sample(const void* src, int32_t src_dtype, int64_t z_stride, int64_t y_stride, int32_t Z, int32_t H, int32_t W,
                                   int32_t g, float* out, vsx_stream_t stream) {
  VSX_CHECK(src && out && Z > 0 && H > 0 && W > 0 && g >= 1, "vsx_grid_sample: bad arguments");
  VSX_CHECK_SRC("vsx_grid_sample", src_dtype);
  VSX_CHECK(y_stride >= W && z_stride >= 0, "vsx_grid_sample: y_stride %ld < W or z_stride %ld < 0", (long)y_stride, (long)z_stride);
  const int ho = (H + g - 1) / g, wo = (W + g - 1) / g;
  const long total = (long)Z * ho * wo;
  const dim3 grid(vsx_capped_grid(total, 256, 8)), block(256);
  vsx_by_src(src_dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(grid_sample_kernel<T>, grid, block, 0, (hipStream_t)stream, (const T*)src, (long)z_stride, (long)y_stride, ho, wo, g,
                       total, reinterpret_cast<uint32_t*>(out));
    return 0;
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ 3 x 3 median
// A wave owns a strip: MED_COLS output columns, MED_ROWS output rows of one plane.  Lane l holds column x0 - 1 + l (reflected; for a
// radius of one, reflect is a clamp) and walks down the strip with three rows in registers: every row is loaded once per strip, so an
// element is read 64 / 62 * (MED_ROWS + 2) / MED_ROWS times.  The 9-element median is the classic network on sorted columns: each
// lane sorts its own column triple (lo, mid, hi) once, takes its neighbours' triples by lane shuffles, and
//   median = med3(max3(lo's), med3(mid's), min3(hi's)).
__device__ __forceinline__ float pp_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

template <typename T, bool MASK>
__global__ __launch_bounds__(256) void median3x3_kernel(const T* __restrict__ src, long sz, long sy, int H, int W, int sx, int sr, long strips,
                                                        float thr, float* __restrict__ outf, uint8_t* __restrict__ outm) {
  const int lane = threadIdx.x & 63;
  for (long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6); s < strips; s += (long)gridDim.x * 4) {  // uniform over the wave
    const int cs = (int)(s % sx);
    const long r = s / sx;
    const int rs = (int)(r % sr);
    const long z = r / sr;
    const int x0 = cs * MED_COLS, y0 = rs * MED_ROWS;
    const int y1 = min(y0 + MED_ROWS, H);
    const int c = x0 - 1 + lane;
    const int cc = min(max(c, 0), W - 1);  // every load stays inside its row
    const T* col = src + z * sz + cc;
    const bool writes = lane >= 1 && lane <= MED_COLS && c < W;
    float a = vsx_src_value(col[(long)max(y0 - 1, 0) * sy]);
    float b = vsx_src_value(col[(long)y0 * sy]);
    for (int y = y0; y < y1; ++y) {
      const float d = vsx_src_value(col[(long)min(y + 1, H - 1) * sy]);
      const float lo = fminf(fminf(a, b), d), hi = fmaxf(fmaxf(a, b), d), mid = pp_med3(a, b, d);
      const float lo_l = __shfl_up(lo, 1, 64), lo_r = __shfl_down(lo, 1, 64);
      const float mid_l = __shfl_up(mid, 1, 64), mid_r = __shfl_down(mid, 1, 64);
      const float hi_l = __shfl_up(hi, 1, 64), hi_r = __shfl_down(hi, 1, 64);
      const float m = pp_med3(fmaxf(fmaxf(lo_l, lo), lo_r), pp_med3(mid_l, mid, mid_r), fminf(fminf(hi_l, hi), hi_r));
      if (writes) {
        const long o = (z * H + y) * (long)W + c;  // c in [x0, min(x0 + MED_COLS, W)), y in [y0, y1)
        if (MASK) outm[o] = m >= thr ? 1 : 0;
        else outf[o] = m;
      }
      a = b, b = d;
    }
  }
}

extern "C" int32_t vsx_median3x3(const void* src, int32_t src_dtype, int64_t z_stride, int64_t y_stride, int32_t Z, int32_t H, int32_t W,
                                 float* out, uint8_t* mask, float thr, vsx_stream_t stream) {
  VSX_CHECK(src && Z > 0 && H > 0 && W > 0, "vsx_median3x3: bad arguments");
  VSX_CHECK((out != nullptr) != (mask != nullptr), "vsx_median3x3: exactly one of out (fp32 median) and mask (uint8 median >= thr)");
  VSX_CHECK_SRC("vsx_median3x3", src_dtype);
  VSX_CHECK(out == nullptr || src_dtype == VSX_PG_F32, "vsx_median3x3: the fp32 epilogue takes an fp32 source");
  VSX_CHECK(y_stride >= W && z_stride >= 0, "vsx_median3x3: y_stride %ld < W or z_stride %ld < 0", (long)y_stride, (long)z_stride);
  const int sx = vsx_cdiv(W, MED_COLS), sr = vsx_cdiv(H, MED_ROWS);
  const long strips = (long)Z * sx * sr;
  const dim3 grid(vsx_capped_grid(strips, 4, 16)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (out) {
    hipLaunchKernelGGL((median3x3_kernel<float, false>), grid, block, 0, s, (const float*)src, (long)z_stride, (long)y_stride, H, W, sx, sr,
                       strips, thr, out, (uint8_t*)nullptr);
  } else {
    vsx_by_src(src_dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((median3x3_kernel<T, true>), grid, block, 0, s, (const T*)src, (long)z_stride, (long)y_stride, H, W, sx, sr, strips,
                         thr, (float*)nullptr, mask);
      return 0;
    });
  }
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ NaN-aware moments
// One workgroup per chunk of MOM_CHUNK values.  A thread takes its elements in ascending order (float4 vectors 4 (t + 256 k) .. where x
// is 16-byte aligned, else single values t + 256 k), the lanes of a wave join by the xor butterfly 32 .. 1, thread 0 joins the four waves
// in order and stores the chunk's partial; the fold kernel joins the partials in index order (MOM_FOLD_SEGS runs first: one fixed
// association).  An alignment is a different, equally fixed, order.
// integral: x holds integers with |x| <= 65535 (uint8 / uint16 / int16 stores) and n <= 2^31 - 1, so |sum x| <= 65535 * 2^31 < 2^47 and
// sum x^2 <= 65535^2 * (2^31 - 1) < 2^63: both int64 sums are exact.
struct MomPart {
  double q[4];   // pass 1: count, min, max, sum          pass 2: sum (x - mean)^2, sum (x - mean), 0, 0
  long long i[2];  // pass 1, integral: sum x, sum x^2
};
static_assert(sizeof(MomPart) == VSX_MOMENTS_PART_BYTES, "vsx_nan_moments_ws_bytes");

__device__ __forceinline__ long long pp_shfl_xor_i64(long long v, int o) {
  const int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
  return ((long long)hi << 32) | (unsigned int)lo;
}
// quantities 1 and 2 of pass 1 are extrema; everything else is a sum
template <int PASS>
__device__ __forceinline__ double mom_join(int q, double a, double b) {
  if (PASS == 1 && q == 1) return fmin(a, b);
  if (PASS == 1 && q == 2) return fmax(a, b);
  return a + b;
}
template <int PASS>
__device__ __forceinline__ double mom_identity(int q) {
  if (PASS == 1 && q == 1) return (double)INFINITY;
  if (PASS == 1 && q == 2) return -(double)INFINITY;
  return 0.0;
}

template <int PASS, bool INTEGRAL>
struct MomLane {
  double q[4];
  long long i[2];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = mom_identity<PASS>(k);
    i[0] = i[1] = 0;
  }
  __device__ __forceinline__ void take(float xf, double mean) {
    if (xf != xf) return;
    const double x = (double)xf;
    if (PASS == 1) {
      q[0] += 1.0, q[1] = fmin(q[1], x), q[2] = fmax(q[2], x), q[3] += x;
      if (INTEGRAL) {
        const long long xi = (long long)xf;
        i[0] += xi, i[1] += xi * xi;
      }
    } else {
      const double d = x - mean;  // fp32 - double: one rounding
      q[0] = fma(d, d, q[0]), q[1] += d;
    }
  }
};

template <int PASS, bool INTEGRAL, bool VEC>
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, long n, double mean, MomPart* __restrict__ part) {
  __shared__ MomPart sh[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long base = (long)blockIdx.x * MOM_CHUNK;
  const long end = min(base + (long)MOM_CHUNK, n);
  MomLane<PASS, INTEGRAL> a;
  a.init();
  long done = base;
  if (VEC) {  // x is 16-byte aligned and MOM_CHUNK is a multiple of four: so is x + base
    done = base + ((end - base) & ~3l);
    for (long i = base + 4 * t; i < done; i += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(x + i);
      a.take(v.x, mean), a.take(v.y, mean), a.take(v.z, mean), a.take(v.w, mean);
    }
  }
  for (long i = done + t; i < end; i += 256) a.take(x[i], mean);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int o = 32; o > 0; o >>= 1) a.q[k] = mom_join<PASS>(k, a.q[k], __shfl_xor(a.q[k], o, 64));
  if (INTEGRAL) {
    for (int o = 32; o > 0; o >>= 1) a.i[0] += pp_shfl_xor_i64(a.i[0], o), a.i[1] += pp_shfl_xor_i64(a.i[1], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[wave].q[k] = a.q[k];
    sh[wave].i[0] = a.i[0], sh[wave].i[1] = a.i[1];
  }
  __syncthreads();
  if (t == 0) {
    MomPart p = sh[0];
    for (int w = 1; w < 4; ++w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) p.q[k] = mom_join<PASS>(k, p.q[k], sh[w].q[k]);
      p.i[0] += sh[w].i[0], p.i[1] += sh[w].i[1];
    }
    part[blockIdx.x] = p;
  }
}

// thread s joins run s of the partials in ascending order; thread 0 then joins the runs in ascending order
template <int PASS>
__global__ __launch_bounds__(MOM_FOLD_SEGS) void moments_fold_kernel(const MomPart* __restrict__ part, long chunks, double* __restrict__ out,
                                                                     long long* __restrict__ isums) {
  __shared__ MomPart run[MOM_FOLD_SEGS];
  const int s = threadIdx.x;
  const long len = (chunks + MOM_FOLD_SEGS - 1) / MOM_FOLD_SEGS;
  MomPart p;
#pragma unroll
  for (int k = 0; k < 4; ++k) p.q[k] = mom_identity<PASS>(k);
  p.i[0] = p.i[1] = 0;
  const long g1 = min((s + 1) * len, chunks);
  for (long g = s * len; g < g1; ++g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) p.q[k] = mom_join<PASS>(k, p.q[k], part[g].q[k]);
    p.i[0] += part[g].i[0], p.i[1] += part[g].i[1];
  }
  run[s] = p;
  __syncthreads();
  if (s == 0) {
    for (int r = 1; r < MOM_FOLD_SEGS; ++r) {
#pragma unroll
      for (int k = 0; k < 4; ++k) p.q[k] = mom_join<PASS>(k, p.q[k], run[r].q[k]);
      p.i[0] += run[r].i[0], p.i[1] += run[r].i[1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = p.q[k];
    if (isums) isums[0] = p.i[0], isums[1] = p.i[1];
  }
}

extern "C" int64_t vsx_nan_moments_ws_bytes(int64_t n) {
  if (n < 1) return 0;
  return ((n + MOM_CHUNK - 1) / MOM_CHUNK) * (int64_t)sizeof(MomPart);
}

extern "C" int32_t vsx_nan_moments(const float* x, int64_t n, int32_t pass, int32_t integral, double mean, double* out, int64_t* isums,
                                   void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  VSX_CHECK(x && out && ws && n >= 1 && n <= 2147483647ll, "vsx_nan_moments: bad arguments (1 <= n <= 2^31 - 1)");
  VSX_CHECK(pass == 1 || pass == 2, "vsx_nan_moments: pass %d is neither 1 nor 2", pass);
  VSX_CHECK(integral == 0 || (integral == 1 && pass == 1 && isums), "vsx_nan_moments: integral sums belong to pass 1 and want isums");
  VSX_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)isums & 7) == 0,
            "vsx_nan_moments: x 4-byte, out / isums / ws 8-byte aligned");
  VSX_CHECK(ws_bytes >= vsx_nan_moments_ws_bytes(n), "vsx_nan_moments: workspace of %ld bytes, %ld wanted", (long)ws_bytes,
            (long)vsx_nan_moments_ws_bytes(n));
  const long chunks = (n + MOM_CHUNK - 1) / MOM_CHUNK;
  MomPart* part = reinterpret_cast<MomPart*>(ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks), block(256);
  vsx_by_bool(vsx_al16(x), [&](auto vec) {
    constexpr bool V = decltype(vec)::value;
    if (pass == 2) hipLaunchKernelGGL((moments_partial_kernel<2, false, V>), grid, block, 0, s, x, (long)n, mean, part);
    else if (integral) hipLaunchKernelGGL((moments_partial_kernel<1, true, V>), grid, block, 0, s, x, (long)n, mean, part);
    else hipLaunchKernelGGL((moments_partial_kernel<1, false, V>), grid, block, 0, s, x, (long)n, mean, part);
    return 0;
  });
  VSX_LAUNCH_CHECK();
  long long* is = integral ? reinterpret_cast<long long*>(isums) : nullptr;
  if (pass == 2) hipLaunchKernelGGL(moments_fold_kernel<2>, dim3(1), dim3(MOM_FOLD_SEGS), 0, s, part, chunks, out, is);
  else hipLaunchKernelGGL(moments_fold_kernel<1>, dim3(1), dim3(MOM_FOLD_SEGS), 0, s, part, chunks, out, is);
  VSX_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ histograms
// counts are uint64 in memory: no limit on n follows from them.  A workgroup's private LDS counters are 32-bit; the host gives a
// workgroup at most HIST_WG_MAX < 2^32 values.  Integer atomics only: the counts do not depend on arrival order.
#define HIST_WG_MAX (1l << 31)

__global__ __launch_bounds__(256) void zero_u64_kernel(unsigned long long* __restrict__ p, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = 0ull;
}

// a value outside [lo, lo + nbins) (a NaN included) is not counted: no index leaves the table
template <bool LDS>
__global__ __launch_bounds__(256) void hist_int_kernel(const float* __restrict__ x, long n, int lo, int nbins, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int sh[LDS ? HIST_LDS_BINS : 1];
  if (LDS) {
    for (int b = threadIdx.x; b < nbins; b += 256) sh[b] = 0u;
    __syncthreads();
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = x[i];
    if (!(v >= -2147483648.f && v < 2147483648.f)) continue;
    const long b = (long)(int)v - lo;
    if (b < 0 || b >= nbins) continue;
    if (LDS) atomicAdd(&sh[b], 1u);
    else atomicAdd(&counts[b], 1ull);
  }
  if (LDS) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += 256) {
      const unsigned int c = sh[b];
      if (c) atomicAdd(&counts[b], (unsigned long long)c);
    }
  }
}

static inline unsigned hist_grid(long n) {
  unsigned g = vsx_capped_grid(n, 256 * 16, 4);
  const long need = (n + HIST_WG_MAX - 1) / HIST_WG_MAX;  // grid-stride: a workgroup sees at most ceil(n / g) + 256 values
  return (unsigned)(g < need ? need : g);
}

extern "C" int32_t vsx_hist_int(const float* x, int64_t n, int32_t lo, int32_t nbins, uint64_t* counts, vsx_stream_t stream) {
  VSX_CHECK(x && counts && n >= 1, "vsx_hist_int: bad arguments");
  VSX_CHECK(nbins >= 1 && nbins <= 65536, "vsx_hist_int: nbins %d outside [1, 65536]", nbins);
  VSX_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)counts & 7) == 0, "vsx_hist_int: x 4-byte, counts 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(zero_u64_kernel, dim3(vsx_cdiv(nbins, 256)), dim3(256), 0, s, c, nbins);
  VSX_LAUNCH_CHECK();
  const dim3 grid(hist_grid(n)), block(256);
  if (nbins <= HIST_LDS_BINS) hipLaunchKernelGGL(hist_int_kernel<true>, grid, block, 0, s, x, (long)n, lo, nbins, c);
  else hipLaunchKernelGGL(hist_int_kernel<false>, grid, block, 0, s, x, (long)n, lo, nbins, c);
  VSX_LAUNCH_CHECK();
  return 0;
}

// bin i holds edges[i] <= x < edges[i + 1], the last bin is closed on the right; x outside [edges[0], edges[nbins]] (a NaN included)
// is not counted.  The guess (x - e0) nbins / (eN - e0) only says where the comparisons against the table start: whatever its
// rounding, the bin is the one the edges define.  Both walks stop inside [0, nbins - 1].
__global__ __launch_bounds__(256) void hist_edges_kernel(const float* __restrict__ x, long n, const double* __restrict__ edges, int nbins,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ double e[VSX_HIST_EDGES_MAX_BINS + 1];
  __shared__ unsigned int sh[VSX_HIST_EDGES_MAX_BINS];
  for (int b = threadIdx.x; b <= nbins; b += 256) e[b] = edges[b];
  for (int b = threadIdx.x; b < nbins; b += 256) sh[b] = 0u;
  __syncthreads();
  const double e0 = e[0], eN = e[nbins];
  const double scale = eN > e0 ? (double)nbins / (eN - e0) : 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double v = (double)x[i];
    if (!(v >= e0 && v <= eN)) continue;
    int b = (int)fmin((v - e0) * scale, (double)(nbins - 1));  // v >= e0: the product is >= 0
    while (b > 0 && v < e[b]) --b;
    while (b < nbins - 1 && v >= e[b + 1]) ++b;
    atomicAdd(&sh[b], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += 256) {
    const unsigned int c = sh[b];
    if (c) atomicAdd(&counts[b], (unsigned long long)c);
  }
}

extern "C" int32_t vsx_hist_edges(const float* x, int64_t n, const double* edges, int32_t nbins, uint64_t* counts, vsx_stream_t stream) {
  VSX_CHECK(x && edges && counts && n >= 1, "vsx_hist_edges: bad arguments");
  VSX_CHECK(nbins >= 2 && nbins <= VSX_HIST_EDGES_MAX_BINS, "vsx_hist_edges: nbins %d outside [2, %d]", nbins, VSX_HIST_EDGES_MAX_BINS);
  VSX_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)edges & 7) == 0,
            "vsx_hist_edges: x 4-byte, edges / counts 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(zero_u64_kernel, dim3(vsx_cdiv(nbins, 256)), dim3(256), 0, s, c, nbins);
  VSX_LAUNCH_CHECK();
  hipLaunchKernelGGL(hist_edges_kernel, dim3(hist_grid(n)), dim3(256), 0, s, x, (long)n, edges, nbins, c);
  VSX_LAUNCH_CHECK();
  return 0;
}
