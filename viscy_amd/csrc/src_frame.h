// viscy_amd — a stored frame as the kernels that read one see it: elements of VSX_PG_F32 / U16 / I16 / U8 in their storage dtype,
// converted to fp32 on the way (exact for the integer types).  Shared by patch_gather.hip and preprocess.hip: the runtime code ->
// element type dispatch with its range check, the element helpers, and the bounded grid of the grid-stride frame kernels.
#pragma once
#include "vsx_common.h"
#include "../../include/vsx.h"

// ------------------------------------------------------------------ host: source dtype code -> element type
// as vsx_by_dtype does for the compute dtypes: `f` gets vsx_type<float / uint16_t / int16_t / uint8_t>; check the code first
#define VSX_CHECK_SRC(entry, code) \
  VSX_CHECK((code) >= VSX_PG_F32 && (code) <= VSX_PG_U8, "%s: unknown source dtype code %d", entry, (int)(code))
template <class F>
static __forceinline__ auto vsx_by_src(int code, F&& f) -> decltype(f(vsx_type<float>{})) {
  if (code == VSX_PG_U16) return f(vsx_type<uint16_t>{});
  if (code == VSX_PG_I16) return f(vsx_type<int16_t>{});
  if (code == VSX_PG_U8) return f(vsx_type<uint8_t>{});
  return f(vsx_type<float>{});
}
static inline int vsx_src_vec_elems(int code) {  // elements per 16-byte vector of the source
  return vsx_by_src(code, [](auto tag) { return 16 / (int)sizeof(typename decltype(tag)::type); });
}
// grid of a grid-stride kernel: one workgroup per `per_block` items, at most `blocks_per_cu` per compute unit; the rest loops.
// Eight 256-thread workgroups per CU fill every wave slot.
static inline unsigned vsx_capped_grid(long items, long per_block, int blocks_per_cu) {
  long g = (items + per_block - 1) / per_block;
  const long cap = (long)vsx_cu_count() * blocks_per_cu;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ------------------------------------------------------------------ device: one element
// float32 sources travel as 32-bit integers where they are only copied: NaN payloads, signed zeros and denormals arrive bit for bit
template <typename T>
struct vsx_src_raw { typedef T type; };
template <>
struct vsx_src_raw<float> { typedef uint32_t type; };

template <typename R>
__device__ __forceinline__ uint32_t vsx_src_bits(R v) {  // the fp32 bit pattern of a stored element, given as its raw type
  if constexpr (std::is_same<R, uint32_t>::value) return v;
  else return __float_as_uint((float)v);
}
template <typename T>
__device__ __forceinline__ uint32_t vsx_src_bits_at(const T* p) {
  return vsx_src_bits(*reinterpret_cast<const typename vsx_src_raw<T>::type*>(p));
}
template <typename T>
__device__ __forceinline__ float vsx_src_value(T v) { return (float)v; }  // exact for the integer types; the identity for float
