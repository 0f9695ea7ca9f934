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
