// viscy_amd — the instruction-level vocabulary of the 16x16 MFMA kernels (gemm, gemm_nt2, mlp, conv3d, dwconv_mfma, head,
// headconv): fragment types, the MFMA step, the lane map, the transposing LDS read, LDS-DMA, counted waits.  Facts of gfx950,
// stated once; schedules, tile shapes and LDS layouts stay with the kernels.  (The exact-fp32 32x32 engine is f32_tile.h.)
#pragma once
#include "vsx_common.h"

typedef float mf_f32x4 __attribute__((ext_vector_type(4)));    // one 16x16 accumulator fragment
typedef __bf16 mf_bf16x8 __attribute__((ext_vector_type(8)));  // one A / B operand fragment of the 32-deep bf16 MFMA
typedef short mf_s16x4 __attribute__((ext_vector_type(4)));    // 4 bf16 as the transposing read / the 16-deep MFMA take them

// operand fragment of element type T and the contraction depth of one MFMA
template <typename T>
struct Frag;
template <>
struct Frag<bf16_t> {
  typedef mf_bf16x8 type;
  static constexpr int MK = 32;
};
template <>
struct Frag<float> {
  typedef float type;
  static constexpr int MK = 4;
};

// ------------------------------------------------------------------ the lane map
// A and B alike: lane (p16, kq) supplies k = kq*8 .. kq*8+7 (fp32: k = kq) of row p16 of its operand, both operands
// "row x k".  C / D: accumulator element i of the lane is row kq*4 + i (a row of A), column p16 (a row of B).
struct MfLane {
  int lane, wave, p16, kq;  // wave: uniform (readfirstlane), for wave-uniform LDS bases and scalar branches
};
__device__ __forceinline__ MfLane mf_lane(int tid) {
  const int lane = tid & 63;
  return {lane, __builtin_amdgcn_readfirstlane(tid >> 6), lane & 15, lane >> 4};
}

// ------------------------------------------------------------------ the MFMA step: c += a . b^T
// (operands by value: by const reference head.hip's row kernels allocated their accumulators differently)
__device__ __forceinline__ mf_f32x4 mfma16(mf_bf16x8 a, mf_bf16x8 b, mf_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ mf_f32x4 mfma16(float a, float b, mf_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// the 16-deep bf16 form: lane (p16, kq) supplies k = kq*4 .. kq*4+3, i.e. ONE transposing read (lds_tr4) per operand
__device__ __forceinline__ mf_f32x4 mfma16_k16(mf_s16x4 a, mf_s16x4 b, mf_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------------ fragment constants
__device__ __forceinline__ mf_bf16x8 mf_zero8() { return (mf_bf16x8){0, 0, 0, 0, 0, 0, 0, 0}; }
// bf16 1.0 in all 8 slots where `on`, zeros elsewhere (a ones operand sums the other operand's rows: bias gradients)
__device__ __forceinline__ mf_bf16x8 mf_ones8(bool on = true) {
  const uint32_t one2 = on ? 0x3F803F80u : 0u;
  union { uint4 u; mf_bf16x8 v; } t;
  t.u = make_uint4(one2, one2, one2, one2);
  return t.v;
}
__device__ __forceinline__ mf_s16x4 mf_ones4() { return {(short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80}; }
__device__ __forceinline__ mf_bf16x8 mf_pack8(const float* f) {  // 8 floats -> one operand fragment (round to nearest even)
  union { uint4 u; mf_bf16x8 v; } t;
  t.u = make_uint4(f32x2_to_bf16x2_bits(f[0], f[1]), f32x2_to_bf16x2_bits(f[2], f[3]), f32x2_to_bf16x2_bits(f[4], f[5]),
                   f32x2_to_bf16x2_bits(f[6], f[7]));
  return t.v;
}
// zero an accumulator ARRAY (1-D or 2-D, not a pointer).  A macro on purpose: a function's loop is unrolled before it is inlined,
// which reorders the callers' instructions (the GEMM kernels' register allocation moved); this loop unrolls where it stands.
#define mfma_zero(acc) \
  _Pragma("unroll") for (int z_ = 0; z_ < (int)(sizeof(acc) / sizeof(mf_f32x4)); ++z_) \
    reinterpret_cast<mf_f32x4*>(acc)[z_] = (mf_f32x4){0.f, 0.f, 0.f, 0.f}

// ------------------------------------------------------------------ the transposing LDS read (ds_read_b64_tr_b16)
// An MFMA operand needs 8 consecutive CONTRACTION values per lane; a row-major [m][column] bf16 tile whose contraction
// index is the row m has them a row stride apart.  The transposing 8-byte read delivers them anyway: within each group of 16
// lanes, lane q reads 8 bytes at row (q >> 2), columns (q & 3)*4 .. +3 of its own address pattern, and RECEIVES column q of the
// group's 4 x 16 block: 4 values, rows 0 .. 3.  With the group kq starting at row kq*4, two reads (rows r and r + 16 of a 32-row
// step) fill a fragment: k-slot (kq, j) holds m = kq*4 + j for j < 4 and m = 16 + kq*4 + (j - 4) for j >= 4.  Both operands of
// an MFMA must use the same slot <-> m mapping (any permutation of k is a valid contraction order).  The read exchanges data
// between lanes: never under divergent control flow.
__device__ __forceinline__ mf_s16x4 lds_tr4(const void* a) {  // one read: the whole operand of the 16-deep MFMA
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((mf_s16x4 __attribute__((address_space(3)))*)(a));
}
__device__ __forceinline__ mf_bf16x8 lds_tr8(const void* a0, const void* a1) {  // a0 / a1: THIS lane's two addresses
  union { struct { mf_s16x4 lo, hi; } s; mf_bf16x8 v; } u;
  u.s.lo = lds_tr4(a0);
  u.s.hi = lds_tr4(a1);
  return u.v;
}
// tile: [32][..] bf16, row stride ldb BYTES; the fragment of column col0 + p16
__device__ __forceinline__ mf_bf16x8 lds_tr8(const void* tile, int ldb, int col0, int p16, int kq) {
  const char* a0 = (const char*)tile + (kq * 4 + (p16 >> 2)) * ldb + (col0 + (p16 & 3) * 4) * 2;
  return lds_tr8(a0, a0 + 16 * ldb);
}

// ------------------------------------------------------------------ LDS-DMA (global_load_lds_dwordx4 / _dword)
// One wave-wide piece: lane l's 16 (4) bytes at `gsrc` land at LDS address (wave-uniform base) + l * 16 (4); no staging VGPRs,
// no ds_write pass, counted by vmcnt like any load.  Two spellings, both needed:
//   lds_dma16 / lds_dma4: the compiler builtin.  hipcc knows the LDS object written and orders later reads of it itself — by
//     `s_waitcnt vmcnt(0)` in front of every LDS read it cannot tell apart from the DMA's target.  Right where each buffer is
//     its own __shared__ object named at compile time, or where the kernel waits for everything before it reads anyway.
//   lds_dma16_raw: inline assembly (M0 = LDS base, lds_addr(p)), invisible to that bookkeeping.  Right where the builtin's
//     vmcnt(0) would land in front of reads of OTHER buffers and serialise the prefetch (dwconv_mfma's raw / plane buffers,
//     headconv's alternating weight buffers): such a kernel counts its own waits (wait_vm<N>) and orders LDS traffic with
//     barrier_lds().
// (macros: the two address expressions are evaluated and cast in the order the sites had them; as function arguments they are not,
// and hipcc then schedules the address arithmetic around the M0 writes differently)
#define lds_dma_n(gsrc, lds_dst, bytes)                                                    \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc), \
                                   (__attribute__((address_space(3))) void*)(lds_dst), bytes, 0, 0)
#define lds_dma16(gsrc, lds_dst) lds_dma_n(gsrc, lds_dst, 16)
#define lds_dma4(gsrc, lds_dst) lds_dma_n(gsrc, lds_dst, 4)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ void lds_dma16_raw(const void* gsrc, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_base) : "memory", "m0");
}

// ------------------------------------------------------------------ counted waits
// Loads (DMA pieces included) return in order: "at most N vector-memory operations outstanding" proves every older one landed.
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void wait_vm0_lgkm0() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }  // one instruction
// this wave's LDS traffic done, then the workgroup barrier — WITHOUT the vmcnt(0) a __syncthreads() carries (DMA stays in flight);
// the compiler moves nothing across it (gemm_nt2 wants its s_barrier sunk under later arithmetic and spells the two halves out)
__device__ __forceinline__ void barrier_lds() {
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
