// Patch gather of the DynaCLR data feed (viscy_amd/data/triplet.py): n patches [C, Z, Yp, Xp] cut out of frames that are
// resident in device memory, written as one dense fp32 tensor [n, C, Z, Yp, Xp].  A streaming copy: no LDS, no atomics.
//
// Work unit = one output row (Xp elements).  A group of `lpr` lanes (16 / 32 / 64, chosen by the host from Xp) owns a row, so
// a wave serves 64 / lpr rows at once; rows go round the bounded grid.  Per row, measured from the row's first SOURCE byte:
//   head   the elements in front of the first 16-byte boundary of the source        narrow loads (one element per lane)
//   body   whole 16-byte vectors, each one completely inside [x0, x0 + Xp)          one 16-byte load per lane
//   tail   what is left behind the last whole vector                               narrow loads
// No load touches a byte outside the row segment [x0, x0 + Xp): a frame may end where its allocation ends.  The stores of the
// body take the widest form the OUTPUT address of the row allows (16 / 8 / 4 bytes; Xp is even, so rows start 8-byte aligned,
// and the head shifts that by its own length), decided once per row.
// float32 sources travel as 32-bit integers: NaN payloads, signed zeros and denormals arrive bit for bit.
#include "src_frame.h"

// raw: the type a source element is loaded as;  bits(v): its fp32 bit pattern;  unpack(w, f): the 16 / sizeof(T) elements of one vector
template <typename T>
struct PgSrc {
  typedef typename vsx_src_raw<T>::type raw;
  static __device__ __forceinline__ uint32_t bits(raw v) { return vsx_src_bits(v); }
  static __device__ __forceinline__ void unpack(const uint4& w, uint32_t* f);
};
template <>
__device__ __forceinline__ void PgSrc<float>::unpack(const uint4& w, uint32_t* f) { f[0] = w.x; f[1] = w.y; f[2] = w.z; f[3] = w.w; }
template <>
__device__ __forceinline__ void PgSrc<uint16_t>::unpack(const uint4& w, uint32_t* f) {
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __float_as_uint((float)(d[i] & 0xffffu));
    f[2 * i + 1] = __float_as_uint((float)(d[i] >> 16));
  }
}
template <>
__device__ __forceinline__ void PgSrc<int16_t>::unpack(const uint4& w, uint32_t* f) {
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __float_as_uint((float)(int16_t)(d[i] & 0xffffu));
    f[2 * i + 1] = __float_as_uint((float)(int16_t)(d[i] >> 16));
  }
}
template <>
__device__ __forceinline__ void PgSrc<uint8_t>::unpack(const uint4& w, uint32_t* f) {
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) f[4 * i + j] = __float_as_uint((float)((d[i] >> (8 * j)) & 0xffu));
}

// lanes per row: enough for the row's `vecs` 16-byte vectors in one sweep, at most a wave
static inline int pg_lanes_per_row(int vecs) { return vecs <= 16 ? 16 : (vecs <= 32 ? 32 : 64); }

// desc: VSX_PG_DESC int64 per patch {frame base address, stride c, stride z, stride y (elements), y0, x0}
template <typename T>
__global__ __launch_bounds__(256) void patch_gather_kernel(const int64_t* __restrict__ desc, uint32_t* __restrict__ out, long rows,
                                                           int C, int Z, int Yp, int Xp, int lpr) {
  typedef typename PgSrc<T>::raw raw_t;
  constexpr int VE = 16 / (int)sizeof(T);  // elements per 16-byte vector
  const int l = threadIdx.x % lpr;
  const long rows_per_block = 256 / lpr;
  for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / lpr; row < rows; row += (long)gridDim.x * rows_per_block) {
    const int y = (int)(row % Yp);
    long r = row / Yp;
    const int z = (int)(r % Z); r /= Z;
    const int c = (int)(r % C);
    const int64_t* d = desc + (r / C) * VSX_PG_DESC;
    const raw_t* src = reinterpret_cast<const raw_t*>((uintptr_t)d[0]) + ((long)c * d[1] + (long)z * d[2] + (d[4] + y) * d[3] + d[5]);
    uint32_t* dst = out + row * Xp;
    int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T));  // src is sizeof(T)-aligned: a whole number of elements
    if (head > Xp) head = Xp;
    const int nvec = (Xp - head) / VE;
    for (int i = l; i < head; i += lpr) dst[i] = PgSrc<T>::bits(src[i]);
    for (int i = head + nvec * VE + l; i < Xp; i += lpr) dst[i] = PgSrc<T>::bits(src[i]);
    const uintptr_t dst_body = (uintptr_t)(dst + head);
    const int dst_align = (dst_body & 15) == 0 ? 16 : ((dst_body & 7) == 0 ? 8 : 4);
    for (int v = l; v < nvec; v += lpr) {
      const raw_t* s = src + head + v * VE;   // 16-byte aligned, s + VE <= src + Xp
      uint32_t* o = dst + head + v * VE;      // o + VE <= dst + Xp
      uint32_t f[VE];
      PgSrc<T>::unpack(*reinterpret_cast<const uint4*>(s), f);
      if (dst_align == 16) {
#pragma unroll
        for (int k = 0; k < VE; k += 4) *reinterpret_cast<uint4*>(o + k) = make_uint4(f[k], f[k + 1], f[k + 2], f[k + 3]);
      } else if (dst_align == 8) {
#pragma unroll
        for (int k = 0; k < VE; k += 2) *reinterpret_cast<uint2*>(o + k) = make_uint2(f[k], f[k + 1]);
      } else {
#pragma unroll
        for (int k = 0; k < VE; ++k) o[k] = f[k];
      }
    }
  }
}

extern "C" int32_t vsx_patch_gather(const int64_t* desc, float* out, int32_t n, int32_t C, int32_t Z, int32_t Yp, int32_t Xp,
                                    int32_t src_dtype, vsx_stream_t stream) {
  VSX_CHECK(desc && out && n > 0 && C > 0 && Z > 0 && Yp > 0 && Xp > 0, "vsx_patch_gather: bad arguments");
  VSX_CHECK(((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0, "vsx_patch_gather: out must be 16-byte aligned, desc 8-byte aligned");
  VSX_CHECK_SRC("vsx_patch_gather", src_dtype);
  const int lpr = pg_lanes_per_row(vsx_cdiv(Xp, vsx_src_vec_elems(src_dtype)));
  const long rows = (long)n * C * Z * Yp;
  const dim3 grid(vsx_capped_grid(rows, 256 / lpr, 8)), block(256);
  vsx_by_src(src_dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(patch_gather_kernel<T>, grid, block, 0, (hipStream_t)stream, desc, reinterpret_cast<uint32_t*>(out), rows, C, Z, Yp,
                       Xp, lpr);
    return 0;
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Scaled patch gather of the multi-experiment feed (viscy_amd/data/multi_experiment.py): every patch names its own channels and
// its own source planes, rows and columns through int32 index tables, so one launch cuts boxes of different native sizes out of
// frames of different shapes and resamples each to the batch's (Zt, Yt, Xt).  The tables hold ABSOLUTE positions in the frame.
//
// Work unit = (patch, channel, plane, block of `rb` rows); units go round the bounded grid.  The workgroup keeps the unit's x
// table (Xt ints) in LDS and reloads it only when the next unit names another table.  A group of `lpr` lanes owns a row.  Per
// row, measured from the row's first OUTPUT byte (rows of an odd Xt start 4-byte aligned):
//   head   the elements in front of the first 16-byte boundary of the output       one element per lane
//   body   whole 16-byte vectors of the output: four table entries per lane; where they are consecutive columns and the
//          source address is aligned to four elements, one load of four elements, else four element loads; one 16-byte store
//   tail   what is left behind the last whole vector                               one element per lane
// Every load reads exactly the (plane, row, column) the tables name, or four consecutive named columns of one row.
template <typename T>
struct alignas(4 * sizeof(T)) PgQuad {
  typename PgSrc<T>::raw e[4];
};

// desc: VSX_PGS_DESC int64 per patch {frame base address, stride c, stride z, stride y (elements), offsets of the channel, z, y
// and x tables in idx}
template <typename T>
__global__ __launch_bounds__(256) void patch_gather_scaled_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ idx,
                                                                  uint32_t* __restrict__ out, long units, int C, int Zt, int Yt,
                                                                  int Xt, int lpr, int rb, int yblocks) {
  typedef typename PgSrc<T>::raw raw_t;
  extern __shared__ int32_t pgs_x[];  // the unit's x table
  const int l = threadIdx.x % lpr, g = threadIdx.x / lpr, groups = 256 / lpr;
  int64_t held = -1;  // offset of the x table in LDS (workgroup-uniform)
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const int yb = (int)(u % yblocks);
    long r = u / yblocks;
    const int z = (int)(r % Zt); r /= Zt;
    const int c = (int)(r % C);
    const long p = r / C;
    const int64_t* d = desc + p * VSX_PGS_DESC;
    const int64_t xoff = d[7];
    if (xoff != held) {
      __syncthreads();  // the previous unit's rows have been read out of pgs_x
      for (int i = threadIdx.x; i < Xt; i += 256) pgs_x[i] = idx[xoff + i];
      __syncthreads();
      held = xoff;
    }
    const raw_t* plane = reinterpret_cast<const raw_t*>((uintptr_t)d[0]) + ((long)idx[d[4] + c] * d[1] + (long)idx[d[5] + z] * d[2]);
    const int32_t* ytab = idx + d[6];
    const int y_end = min(Yt, (yb + 1) * rb);
    for (int y = yb * rb + g; y < y_end; y += groups) {
      const raw_t* src = plane + (long)ytab[y] * d[3];
      const long row = ((p * C + c) * Zt + z) * Yt + y;
      uint32_t* dst = out + row * Xt;
      int head = (4 - (int)((row * Xt) & 3)) & 3;  // out is 16-byte aligned: the element offset decides
      if (head > Xt) head = Xt;
      const int nvec = (Xt - head) / 4;
      for (int i = l; i < head; i += lpr) dst[i] = PgSrc<T>::bits(src[pgs_x[i]]);
      for (int i = head + nvec * 4 + l; i < Xt; i += lpr) dst[i] = PgSrc<T>::bits(src[pgs_x[i]]);
      for (int v = l; v < nvec; v += lpr) {
        const int x = head + 4 * v;
        const int a0 = pgs_x[x], a1 = pgs_x[x + 1], a2 = pgs_x[x + 2], a3 = pgs_x[x + 3];
        uint4 f;
        const raw_t* s = src + a0;
        if (a1 == a0 + 1 && a2 == a0 + 2 && a3 == a0 + 3 && ((uintptr_t)s & (4 * sizeof(T) - 1)) == 0) {
          const PgQuad<T> q = *reinterpret_cast<const PgQuad<T>*>(s);  // columns a0 .. a0 + 3, all named
          f = make_uint4(PgSrc<T>::bits(q.e[0]), PgSrc<T>::bits(q.e[1]), PgSrc<T>::bits(q.e[2]), PgSrc<T>::bits(q.e[3]));
        } else {
          f = make_uint4(PgSrc<T>::bits(src[a0]), PgSrc<T>::bits(src[a1]), PgSrc<T>::bits(src[a2]), PgSrc<T>::bits(src[a3]));
        }
        *reinterpret_cast<uint4*>(dst + x) = f;  // (row * Xt + head) % 4 == 0
      }
    }
  }
}

extern "C" int32_t vsx_patch_gather_scaled(const int64_t* desc, const int32_t* idx, float* out, int32_t n, int32_t C, int32_t Zt,
                                           int32_t Yt, int32_t Xt, int32_t src_dtype, vsx_stream_t stream) {
  VSX_CHECK(desc && idx && out && n > 0 && C > 0 && Zt > 0 && Yt > 0 && Xt > 0, "vsx_patch_gather_scaled: bad arguments");
  VSX_CHECK(((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)idx & 3) == 0,
            "vsx_patch_gather_scaled: out must be 16-byte aligned, desc 8-byte, idx 4-byte");
  VSX_CHECK_SRC("vsx_patch_gather_scaled", src_dtype);
  VSX_CHECK(Xt <= VSX_PGS_MAX_XT, "vsx_patch_gather_scaled: Xt=%d, the x table in LDS holds %d", Xt, VSX_PGS_MAX_XT);
  // a row's vectors are the 16-byte vectors of the OUTPUT; a unit gives each group of lanes VSX_PGS_ROWS_PER_GROUP rows
  const int lpr = pg_lanes_per_row(vsx_cdiv(Xt, 4));
  const int rb = (256 / lpr) * VSX_PGS_ROWS_PER_GROUP;
  const int yblocks = vsx_cdiv(Yt, rb);
  const long units = (long)n * C * Zt * yblocks;
  const dim3 grid(vsx_capped_grid(units, 1, 8)), block(256);
  const size_t lds = (size_t)Xt * sizeof(int32_t);
  vsx_by_src(src_dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(patch_gather_scaled_kernel<T>, grid, block, lds, (hipStream_t)stream, desc, idx, reinterpret_cast<uint32_t*>(out),
                       units, C, Zt, Yt, Xt, lpr, rb, yblocks);
    return 0;
  });
  VSX_LAUNCH_CHECK();
  return 0;
}
