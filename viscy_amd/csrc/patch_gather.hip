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
#include "vsx_common.h"
#include "../../include/vsx.h"

template <typename T>
struct PgSrc;  // bits(v): the fp32 bit pattern of source element v;  unpack(w, f): the 16 / sizeof(T) elements of one vector
template <>
struct PgSrc<float> {
  typedef uint32_t raw;
  static __device__ __forceinline__ uint32_t bits(uint32_t v) { return v; }
  static __device__ __forceinline__ void unpack(const uint4& w, uint32_t* f) { f[0] = w.x; f[1] = w.y; f[2] = w.z; f[3] = w.w; }
};
template <>
struct PgSrc<uint16_t> {
  typedef uint16_t raw;
  static __device__ __forceinline__ uint32_t bits(uint16_t v) { return __float_as_uint((float)v); }
  static __device__ __forceinline__ void unpack(const uint4& w, uint32_t* f) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __float_as_uint((float)(d[i] & 0xffffu));
      f[2 * i + 1] = __float_as_uint((float)(d[i] >> 16));
    }
  }
};
template <>
struct PgSrc<int16_t> {
  typedef int16_t raw;
  static __device__ __forceinline__ uint32_t bits(int16_t v) { return __float_as_uint((float)v); }
  static __device__ __forceinline__ void unpack(const uint4& w, uint32_t* f) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __float_as_uint((float)(int16_t)(d[i] & 0xffffu));
      f[2 * i + 1] = __float_as_uint((float)(int16_t)(d[i] >> 16));
    }
  }
};
template <>
struct PgSrc<uint8_t> {
  typedef uint8_t raw;
  static __device__ __forceinline__ uint32_t bits(uint8_t v) { return __float_as_uint((float)v); }
  static __device__ __forceinline__ void unpack(const uint4& w, uint32_t* f) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * i + j] = __float_as_uint((float)((d[i] >> (8 * j)) & 0xffu));
  }
};

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
  VSX_CHECK(src_dtype >= VSX_PG_F32 && src_dtype <= VSX_PG_U8, "vsx_patch_gather: unknown source dtype code %d", src_dtype);
  const int ve = src_dtype == VSX_PG_F32 ? 4 : (src_dtype == VSX_PG_U8 ? 16 : 8);
  // lanes per row: enough for the row's whole vectors in one sweep, at most a wave
  const int vecs = vsx_cdiv(Xp, ve);
  const int lpr = vecs <= 16 ? 16 : (vecs <= 32 ? 32 : 64);
  const long rows = (long)n * C * Z * Yp;
  long g = (rows + 256 / lpr - 1) / (256 / lpr);
  const long cap = (long)vsx_cu_count() * 8;  // eight 256-thread workgroups per CU fill every wave slot; the rest loops
  if (g > cap) g = cap;
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  const dim3 grid((unsigned)g), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (src_dtype) {
    case VSX_PG_F32: hipLaunchKernelGGL(patch_gather_kernel<float>, grid, block, 0, s, desc, o, rows, C, Z, Yp, Xp, lpr); break;
    case VSX_PG_U16: hipLaunchKernelGGL(patch_gather_kernel<uint16_t>, grid, block, 0, s, desc, o, rows, C, Z, Yp, Xp, lpr); break;
    case VSX_PG_I16: hipLaunchKernelGGL(patch_gather_kernel<int16_t>, grid, block, 0, s, desc, o, rows, C, Z, Yp, Xp, lpr); break;
    default: hipLaunchKernelGGL(patch_gather_kernel<uint8_t>, grid, block, 0, s, desc, o, rows, C, Z, Yp, Xp, lpr); break;
  }
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
  VSX_CHECK(src_dtype >= VSX_PG_F32 && src_dtype <= VSX_PG_U8, "vsx_patch_gather_scaled: unknown source dtype code %d", src_dtype);
  VSX_CHECK(Xt <= VSX_PGS_MAX_XT, "vsx_patch_gather_scaled: Xt=%d, the x table in LDS holds %d", Xt, VSX_PGS_MAX_XT);
  // lanes per row: enough for the row's 16-byte output vectors in one sweep, at most a wave; a unit gives each group four rows
  const int vecs = vsx_cdiv(Xt, 4);
  const int lpr = vecs <= 16 ? 16 : (vecs <= 32 ? 32 : 64);
  const int rb = (256 / lpr) * VSX_PGS_ROWS_PER_GROUP;
  const int yblocks = vsx_cdiv(Yt, rb);
  const long units = (long)n * C * Zt * yblocks;
  long g = units;
  const long cap = (long)vsx_cu_count() * 8;  // eight 256-thread workgroups per CU fill every wave slot; the rest loops
  if (g > cap) g = cap;
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  const dim3 grid((unsigned)g), block(256);
  const size_t lds = (size_t)Xt * sizeof(int32_t);
  hipStream_t s = (hipStream_t)stream;
#define VSX_PGS_LAUNCH(T) \
  hipLaunchKernelGGL(patch_gather_scaled_kernel<T>, grid, block, lds, s, desc, idx, o, units, C, Zt, Yt, Xt, lpr, rb, yblocks)
  switch (src_dtype) {
    case VSX_PG_F32: VSX_PGS_LAUNCH(float); break;
    case VSX_PG_U16: VSX_PGS_LAUNCH(uint16_t); break;
    case VSX_PG_I16: VSX_PGS_LAUNCH(int16_t); break;
    default: VSX_PGS_LAUNCH(uint8_t); break;
  }
#undef VSX_PGS_LAUNCH
  VSX_LAUNCH_CHECK();
  return 0;
}
