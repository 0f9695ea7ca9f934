// Fused GRN-MLP of a ConvNeXt-V2 block (timm ConvNeXtBlock / GlobalResponseNormMlp as called from
// viscy_models/unet/unext2.py:79; block math restated at viscy_models/unet/fcmae.py:174-221):
//
//     out = shortcut + drop_path( fc2( GRN( gelu( fc1( LN(dwconv(x)) ) ) ) ) )
//
// in TWO passes over the C-wide LayerNorm output, with the 4C-wide hidden activation never leaving the CU:
//   MODE 0 (statistics): fc1 -> +bias -> GELU -> per-sample column sums of g^2 (the GRN statistics), nothing stored;
//   MODE 1 (output)    : fc1 recomputed -> +bias -> GELU -> g * s[b] + beta -> fc2 -> +bias -> * drop-path scale -> + shortcut.
//   MODE 2 (training fc1): MODE 0 that also stores the pre-activation h and the activation g (bf16) for the backward — the
//                        same outputs as the unfused fc1 GEMM, whose 3-slab K loop pays one HBM round trip per slab and per
//                        tile (its waves sit in s_waitcnt 41 % of the time); here the activation rows are loaded once.
//   MODE 3 (backward statistics): dz = dout . W2 (recomputed per 32-column sub-chunk), P[b] += sum_hw dz * g, S[b] += sum_hw dz
//                        — the GRN statistics path of the backward; dz is NOT stored.
//   MODE 4 (backward dh): dz recomputed, dh = (dz * s[b] + gelu(h) * t[b]) * gelu'(h) stored (the fc1 gradient operand), column
//                        sums of dh (the fc1 bias gradient) into one workspace row per workgroup.
//                        Modes 3 + 4 replace the fc2 data-gradient GEMM (which wrote the 4C-wide dz) and the GRN / GELU backward
//                        pass (which read it back and wrote dh over it): one 4C-wide write instead of two.  (The
//                        write-dominated launches of THIS kernel family land at 3.5 - 3.9 TB/s; linear and tile-shaped store
//                        probes reach 5.5 - 6.9 TB/s on the part, tools/micro/write_rate.hip — the limit is the kernels'
//                        structure, DESIGN.md §3 item 10, not the memory.)
//   MODE 5 (backward dh, h RECOMPUTED): MODE 4 without a stored pre-activation — h = x^ . W1'^T + b1 is recomputed from the
//                        C-wide normalised rows (the same MFMA sequence as the forward: bit-identical h) beside dz = dout . W2;
//   MODE 6 (training fc1, g only): MODE 2 that stores the activation g but NOT h.  Together they take the 4C-wide h out of HBM
//                        (one 4C-wide write in the forward, one 4C-wide read in the backward, per block): K = C is short and the
//                        matrix cores were idle 85 % of these passes (round 4).
// (SURVEY §7 step 4 / VERDICT r1 "what's missing" 1.  The unfused schedule moved 8 of its 15 C-units per pixel as 4C-wide
// h / g tensors through HBM in inference; this one moves 1 + 3.)
//
// gfx950 mapping
//   * a workgroup owns BM = NW * 16 * MF pixel rows of ONE sample; each wave64 owns 16 * MF of them for the whole kernel:
//     its LayerNorm rows live in registers as MFMA B fragments (loaded once, straight from HBM in fragment layout);
//   * the hidden axis is walked in sub-chunks of 32 columns.  fc1 runs with SWAPPED roles (A = 16 weight rows, B = 16 pixel
//     rows), so v_mfma_f32_16x16x32_bf16 leaves lane (p, q) holding hidden q*4..q*4+3 of pixel p — which IS an A fragment
//     of the following fc2 MFMA (pixel rows x 32-deep contraction) once the contraction index is permuted
//     (slot (q, j) <-> hidden j < 4 ? 4q + j : 16 + 4q + j - 4).  The activation therefore goes accumulator -> VALU
//     (bias, GELU, GRN) -> bf16 pack -> MFMA operand without touching LDS or HBM; the permutation is baked into the fc2
//     weight image;
//   * weights are the only LDS traffic: both matrices are pre-packed (vsx_mlp_pack) into a FRAGMENT-MAJOR image — 1 KiB
//     per (16 rows x 32 k) fragment, lane-linear — so a sub-chunk's stage is one contiguous block that
//     global_load_lds_dwordx4 copies HBM/L2 -> LDS with no VGPR staging and no padding, and every fragment read is a
//     conflict-free ds_read_b128 at (fragment base + lane * 16).  Double-buffered, one barrier per sub-chunk;
//   * per-channel vectors (b1, beta, this sample's GRN scale, b2) sit in LDS for the whole kernel: no ordinary global load
//     is live inside the loop (hipcc drains vmcnt(0) — and with it the weight prefetch — at the first use of one);
//   * the shortcut is added with one identity-matrix MFMA per output fragment (exact: products with 1.0 / 0.0 in fp32), so
//     the residual is read in the same 16-byte fragment layout as the input rows; the result leaves through a per-wave LDS
//     transpose as one contiguous 16-byte-vector stream.
#include "vsx_common.h"
#include "mfma16.h"
#include "wtasks.h"
#include "../../include/vsx.h"

struct MlpArgs {
  const bf16_t* xh;     // [M, C]  block LayerNorm output (affine folded into fc1)
  const char* wimg;     // fragment-major image of (W1', W2), see vsx_mlp_pack
  const float* b1;      // [4C]    folded fc1 bias
  const float* grn_s;   // [B, 4C] GRN scale 1 + gamma * N       (MODE 1)
  const float* grn_b;   // [4C]    GRN beta                      (MODE 1)
  const float* b2;      // [C]     fc2 bias                      (MODE 1)
  const bf16_t* res;    // [M, C]  shortcut                      (MODE 1)
  const float* rscale;  // [B] stochastic-depth scale or NULL    (MODE 1)
  bf16_t* out;          // [M, C]                                (MODE 1)
  float* colsq;         // [B, 4C] += sum_hw gelu(h)^2           (MODE 0, 2)
  bf16_t* hout;         // [M, 4C] pre-activation                (MODE 2)
  bf16_t* gout;         // [M, 4C] activation                    (MODE 2)
  float ln_eps;         // > 0: `xh` holds the UN-normalised rows y; the kernel applies the block LayerNorm (no affine) itself (MODE 0, 1, 2)
  bf16_t* xh_out;       // [M, C]  the normalised rows, for the backward   (MODE 2 with ln_eps > 0)
  float* rstd_out;      // [M]     1 / sqrt(var + eps) of every row        (MODE 2 with ln_eps > 0)
  float* mean_out;      // [M]     the row means (MODE 2 / 6 with ln_eps > 0; with xh_out = NULL the backward re-normalises y: MODE 7)
  const float* ln_mean; // [M], [M]  MODE 7: `xh2` holds the UN-normalised rows y; x^ = bf16((y - mean) * rstd) as the forward formed it,
  const float* ln_rstd; //           and dh leaves scaled by the row's rstd (see vsx_mlp_bwd_dh_ln)
  const bf16_t* tin;    // [M, 4C] stored activation g (MODE 3) / stored pre-activation h (MODE 4)
  float* red0;          // [B, 4C] += sum_hw dz * g  (MODE 3)
  float* red1;          // [B, 4C] += sum_hw dz      (MODE 3)
  float* ws;            // [M / BM, 4C] per-workgroup column sums of dh (MODE 4)
  const float* gtab;    // [2 * MLP_GT_N] r(a) = a * Phi(-a), then d(a) = Phi(a) + a * phi(a) - 1/2, for every bf16 a in [2^-24, 16)  (vsx_mlp_gelu_table)
  const bf16_t* xh2;    // [M, C]  normalised rows x^ (MODE 5: `xh` holds dout, as in MODE 3 / 4)
  const char* wimg2;    // forward image (W1', W2) (MODE 5: `wimg` holds the backward image (W2^T, W2), as in MODE 3 / 4)
  int M, hw;
  int nt;               // bit 0: non-temporal stores of h / g / dh (read by a later launch only), bit 1: non-temporal load of the stored
                        // activation (MODE 3: g, MODE 4: h — this pass is its last reader)
};

// GELU through a table: the pre-activation h is a bf16 value, so gelu(h) = max(h, 0) - r(|h|) with r(a) = a * Phi(-a) read
// from a table indexed by the 15 magnitude bits of h (28 binades x 128 mantissas, fp32 entries computed in double on the
// host: the result is the correctly rounded-to-fp32 erf GELU of h).  r underflows to 0 above the table and equals a / 2 to
// 1e-8 below it, so clamping the index needs no fix-up.  The exp / rcp / polynomial evaluation it replaces cost ~120 VALU
// cycles per element and made every pass of this kernel VALU-bound (measured: the statistics pass took the same time per
// hidden element for C = 96 and C = 224); the table costs 6 VALU operations and one LDS read.
#define MLP_GT_BASE (103 << 7)            /* bf16 magnitude bits of 2^-24 */
#define MLP_GT_LIM (131 << 7)             /* ... of 16 */
#define MLP_GT_N (MLP_GT_LIM - MLP_GT_BASE)

// max(h, 0) on the bit pattern: a negative float is a negative integer.  (fmaxf costs two instructions here: kernels run in IEEE
// mode, where the compiler has to canonicalise the operand first.)
__device__ __forceinline__ float mlp_relu(float h) {
  const int b = __float_as_int(h);
  return __int_as_float(b > 0 ? b : 0);
}

// max(h, 0) of BOTH bf16 halves of a pair in one instruction (v_pk_max_i16: a negative bf16 is a negative 16-bit integer)
__device__ __forceinline__ uint32_t mlp_relu_pair(uint32_t w) {
  typedef short mlp_s16x2 __attribute__((ext_vector_type(2)));
  const mlp_s16x2 z = {0, 0};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(mlp_s16x2, w), z));
}

// MLP_TS (probe builds only: hipcc -DMLP_TS=1): s_memtime stamps of ONE workgroup's waves at the phase boundaries of every
// sub-chunk step, read back with vsx_debug_mlp_ts — where a step's cycles go (tools/mlp_timeline.py)
#ifdef MLP_TS
__device__ unsigned long long g_mlp_ts[8 * 64 * 8];
#define MLP_STAMP(k) do { if (blockIdx.x == gridDim.x / 2 + 7 && lane == 0) g_mlp_ts[(wave * 64 + hs) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MLP_STAMP(k) do { } while (0)
#endif

// Waves that issue the LDS-DMA of the weight stages and fold the per-step column sums.  A workgroup's first four waves are the
// FIRST wave on each SIMD; the arbiter favours the older wave, so waves 0 - 3 reach every step's barrier ~1 000 cycles before
// waves 4 - 7 (profiles/r05_mlp_timeline.txt: barrier wait 1 050 vs 220 cycles at C = 224, MODE 7) while a DMA piece costs its
// issuing wave ~175 cycles (610 cycles per wave and step when all eight share them): the early waves take all of them.
#ifndef MLP_DMA_WAVES
#define MLP_DMA_WAVES 4
#endif

template <int C, int MF, int NW, int MODE>
struct MlpGeom {
  static constexpr int H4 = 4 * C, NHS = H4 / 32, KK = C / 32, NF = C / 16;
  static constexpr int WM = 16 * MF, BM = NW * WM;
  static constexpr int W1_PIECES = 2 * KK, IMG_PIECES = 2 * KK + NF;   // KiB per hidden sub-chunk in the image
  static constexpr bool RE = MODE == 5 || MODE == 7;                   // dh pass that recomputes h (7: and re-normalises y)
  static constexpr int NP = RE ? 2 * W1_PIECES : (MODE != 1 ? W1_PIECES : IMG_PIECES);  // pieces staged per sub-chunk
  static constexpr int STAGE_BYTES = NP * 1024;
  static constexpr int OB_COLS = MODE == 0 ? 32 : 64;                  // output leaves in blocks of 64 columns (MODE 0: the
                                                                       // wave-private g tile of ONE sub-chunk, for the statistics)
  static constexpr int OB_RS = OB_COLS * 2 + 16;                       // staging row stride (bytes)
  static constexpr int OUT_BYTES = MODE == 2 ? NW * 2 * WM * OB_RS : NW * WM * OB_RS;  // MODE 6: g only
  // MODE 6: the bias vector b1 lives in the 16 pad bytes behind every row of the staging tile (256 rows x 4 floats >= 4C for
  // C <= 256) instead of an array of its own: at C = 224 that is exactly what two workgroups per CU need (2 x 81 920 B = 160 KiB;
  // measured 1803 -> ~1600 us for that pass at B = 512, tools/perf_mlp_train.py)
  static constexpr bool B1_IN_PADS = MODE == 6;
  static constexpr int VEC_FLOATS = MODE == 1 ? 3 * H4 + C : (MODE == 4 ? 2 * H4 : (RE ? 3 * H4 : (MODE == 3 || B1_IN_PADS ? 4 : H4)));
  static constexpr int RED_FLOATS = MODE == 1 ? 4 : (MODE == 3 || MODE == 7 ? 4 * NW * 32 : 2 * NW * 32);
  static constexpr int GT_FLOATS = (MODE <= 2 || MODE == 6) ? MLP_GT_N : ((MODE == 4 || RE) ? 2 * MLP_GT_N : 4);
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES + OUT_BYTES + (VEC_FLOATS + RED_FLOATS) * 4;
};

// The dh pass of the C = 96 blocks needs 143 registers and 54 KB of LDS: capped at 128 registers (52 bytes of spill per lane)
// two workgroups share a CU and the pass runs 4 % faster (1018 -> ~975 us at B = 512).  The same cap on C = 192 / 224 (132 / 160
// bytes of spill) makes the pass 30 % slower: measured, not applied.
template <int C, int MF, int NW, int MODE>
__device__ __forceinline__ void mlp_fused_body(const MlpArgs& a) {
  typedef MlpGeom<C, MF, NW, MODE> G;
  constexpr int H4 = G::H4, NHS = G::NHS, KK = G::KK, NF = G::NF, WM = G::WM;
  constexpr bool STATS = MODE == 0 || MODE == 2 || MODE == 6, STORE = MODE == 2 || MODE == 6, STORE_H = MODE == 2;
  constexpr bool RE = G::RE, LNF = MODE == 7;
  constexpr bool BWD = (MODE >= 3 && MODE <= 5) || MODE == 7, DH = MODE == 4 || RE;
  constexpr int DW = MLP_DMA_WAVES < NW ? MLP_DMA_WAVES : NW;
  // SEPARATE LDS objects, on purpose: the two weight stages, the per-channel vectors and the output staging are distinct
  // variables, so the compiler's alias scopes let fragment / vector reads proceed while the LDS-DMA prefetch of the OTHER
  // stage is in flight (through one array every ds_read behind a global_load_lds costs an s_waitcnt vmcnt(0): no overlap)
  __shared__ __attribute__((aligned(1024))) char buf0[G::STAGE_BYTES];
  __shared__ __attribute__((aligned(1024))) char buf1[G::STAGE_BYTES];
  __shared__ __attribute__((aligned(16))) float vec[G::VEC_FLOATS];
  __shared__ __attribute__((aligned(16))) float red[G::RED_FLOATS];
  __shared__ __attribute__((aligned(16))) char obuf[G::OUT_BYTES];
  __shared__ __attribute__((aligned(16))) float gt[G::GT_FLOATS];

  const int tid = threadIdx.x;
  const MfLane ln = mf_lane(tid);  // the operand and C / D maps of lane (p16, kq): mfma16.h
  const int lane = ln.lane, wave = ln.wave, p16 = ln.p16, kq = ln.kq;
  const int m0 = blockIdx.x * G::BM;   // the tile lies inside one sample (dispatch: hw % BM == 0)
  const int b = m0 / a.hw;
  const int row0 = m0 + wave * WM;

  // Round 5: every load of the workgroup's set-up — GELU table, per-channel vectors, and (below) the row fragments — is ISSUED before
  // the first of them is waited for.  Written as `for (i) lds[i] = global[i]` the table copy compiled to seven dependent
  // load -> wait -> ds_write round trips (the vectors to two or three more) in front of the row-fragment loads: 5 - 10 us of set-up
  // for a workgroup that lives 90 us, with nothing else on the CU to cover them (one workgroup per CU in the backward passes).
  constexpr int TPB = NW * 64;
  constexpr int NTB = (MLP_GT_N + TPB - 1) / TPB, NVB = (H4 + TPB - 1) / TPB;
  float tb0[(!BWD || DH) ? NTB : 1], tb1[DH ? NTB : 1];
  if constexpr (!BWD || DH) {
#pragma unroll
    for (int k = 0; k < NTB; ++k) {
      const int i = tid + k * TPB;
      if (i < MLP_GT_N) {
        tb0[k] = a.gtab[i];
        if constexpr (DH) tb1[k] = a.gtab[MLP_GT_N + i];
      }
    }
  }
  float vb0[NVB], vb1[(MODE == 1 || DH) ? NVB : 1], vb2[(MODE == 1 || RE) ? NVB : 1];
  if constexpr (!BWD || DH) {
#pragma unroll
    for (int k = 0; k < NVB; ++k) {
      const int i = tid + k * TPB;
      if (i < H4) {
        if constexpr (!BWD) {
          vb0[k] = a.b1[i];
          if constexpr (MODE == 1) {
            vb1[k] = a.grn_s[(size_t)b * H4 + i];
            vb2[k] = a.grn_b[i];
          }
        } else {  // this sample's GRN scale s and statistics-path factor t
          vb0[k] = a.grn_s[(size_t)b * H4 + i];
          vb1[k] = a.grn_b[(size_t)b * H4 + i];
          if constexpr (RE) vb2[k] = a.b1[i];
        }
      }
    }
  }
  auto setup_to_lds = [&]() {
    if constexpr (!BWD || DH) {
#pragma unroll
      for (int k = 0; k < NTB; ++k) {
        const int i = tid + k * TPB;
        if (i < MLP_GT_N) {
          if constexpr (DH) {  // {r(a), d(a)} pairs: one 8-byte gather per element yields gelu AND its derivative
            gt[2 * i] = tb0[k];
            gt[2 * i + 1] = tb1[k];
          } else {
            gt[i] = tb0[k];
          }
        }
      }
      // ---- per-channel vectors -> LDS (once)
#pragma unroll
      for (int k = 0; k < NVB; ++k) {
        const int i = tid + k * TPB;
        if (i < H4) {
          if constexpr (G::B1_IN_PADS) {
            static_assert(!G::B1_IN_PADS || (NW * WM * 4 >= H4 && G::OB_RS == 144), "b1 rides in the pad bytes of the staging rows");
            *reinterpret_cast<float*>(obuf + (i >> 2) * G::OB_RS + 128 + (i & 3) * 4) = vb0[k];
          } else {
            vec[i] = vb0[k];
            if constexpr (MODE == 1 || DH) vec[H4 + i] = vb1[k];
            if constexpr (MODE == 1 || RE) vec[2 * H4 + i] = vb2[k];
          }
        }
      }
    }
    if constexpr (MODE == 1) {
      for (int i = tid; i < C; i += NW * 64) vec[3 * H4 + i] = a.b2[i];
    }
  };
  // ---- this wave's LayerNorm rows as fc1 B fragments: lane (p, q) holds row p, k = kk*32 + q*8 .. +7
  mf_bf16x8 xf[MF][KK];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      xf[mf][kk] = *reinterpret_cast<const mf_bf16x8*>(a.xh + (size_t)(row0 + mf * 16 + p16) * C + kk * 32 + kq * 8);

  // MODE 5: the normalised rows x^ as a second fragment set (operand of the recomputed fc1)
  mf_bf16x8 xg[RE ? MF : 1][RE ? KK : 1];
  if constexpr (RE) {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        xg[mf][kk] = *reinterpret_cast<const mf_bf16x8*>(a.xh2 + (size_t)(row0 + mf * 16 + p16) * C + kk * 32 + kq * 8);
  }
  // MODE 7: x^ was never stored.  xg holds y: normalise it with the forward's own mean / rstd and the forward's expression
  // (bit-identical x^, hence bit-identical h).  dh leaves multiplied by the row's rstd, and the column sums of the parked tile
  // are weighted: lane (n, q) of an MFMA B operand holds contraction slots k = q*8 .. +7, which tile_frag fills with the pixels
  // q*4 .. +3 and 16 + q*4 .. +3 — the weight fragments below carry sigma = 1 / rstd (-> sum of the UNSCALED dh, the fc1 bias
  // gradient) and the row mean split into a bf16 head and tail (-> u = sum of dh' * mean to 2^-17, see vsx_mlp_bwd_dh_ln)
  setup_to_lds();   // (behind the row-fragment loads: everything is in flight together)
  float rsr[LNF ? MF : 1];
  mf_bf16x8 wS, wSl, wMh, wMl;
  if constexpr (LNF) {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      const size_t rowi = (size_t)(row0 + mf * 16 + p16);
      const float mean = a.ln_mean[rowi], rstd = a.ln_rstd[rowi];
      rsr[mf] = rstd;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        union { mf_bf16x8 b; uint4 u; } cv;
        cv.b = xg[mf][kk];
        float v[8], o[8];
        unpack<bf16_t>(cv.u, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[j] - mean) * rstd;
        cv.u = pack<bf16_t>(o);
        xg[mf][kk] = cv.b;
      }
    }
    static_assert(!LNF || MF == 2, "the weight fragments cover the 32 pixels of a wave");
    float sg[8], sl[8], mh[8], ml[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t rowi = (size_t)(row0 + (j >> 2) * 16 + kq * 4 + (j & 3));
      const float mean = a.ln_mean[rowi];
      const float sig = 1.f / a.ln_rstd[rowi];
      sg[j] = round_bf16(sig);   // sigma split into a bf16 head and tail like the mean (round 5, ADVICE r4: a bf16 sigma alone put
      sl[j] = sig - sg[j];       // 2^-9 of relative error per row into the fc1 bias gradient)
      mh[j] = round_bf16(mean);
      ml[j] = mean - mh[j];
    }
    union { mf_bf16x8 b; uint4 u; } c1, c2, c3, c4;
    c1.u = pack<bf16_t>(sg); c2.u = pack<bf16_t>(mh); c3.u = pack<bf16_t>(ml); c4.u = pack<bf16_t>(sl);
    wS = c1.b; wMh = c2.b; wMl = c3.b; wSl = c4.b;
  }

  if constexpr (!BWD) {
    if (a.ln_eps > 0.f) {
      // The block LayerNorm in the prologue (timm ConvNeXtBlock.norm: no affine here, it is folded into W1' / b1): a row's C
      // values sit in the 4 lanes (p, q = 0..3) x KK fragments this wave already holds, so its statistics are a register sum
      // and two cross-lane steps — same arithmetic as ln_fwd_kernel (norm.hip: sums shifted by the row's first element).  The
      // separate LayerNorm pass (read y, write x^) and, in inference, x^ itself disappear; MODE 2 writes x^ / rstd for the
      // backward from here.
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        float v[KK][8];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          union { mf_bf16x8 b; uint4 u; } cv;
          cv.b = xf[mf][kk];
          unpack<bf16_t>(cv.u, v[kk]);
        }
        const float x0 = __shfl(v[0][0], p16, 64);  // lane (p, q = 0) holds k = 0 of row p
        float sm = 0.f, sq2 = 0.f;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = v[kk][j] - x0;
            sm += d;
            sq2 = fmaf(d, d, sq2);
          }
        sm += __shfl_xor(sm, 16, 64);
        sq2 += __shfl_xor(sq2, 16, 64);
        sm += __shfl_xor(sm, 32, 64);
        sq2 += __shfl_xor(sq2, 32, 64);
        sm /= (float)C;
        sq2 /= (float)C;
        const float mean = x0 + sm;
        const float rstd = rsqrtf(fmaxf(sq2 - sm * sm, 0.f) + a.ln_eps);
        const size_t rowi = (size_t)(row0 + mf * 16 + p16);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (v[kk][j] - mean) * rstd;
          union { mf_bf16x8 b; uint4 u; } cv;
          cv.u = pack<bf16_t>(o);
          xf[mf][kk] = cv.b;
          if constexpr (STORE) {
            if (a.xh_out) *reinterpret_cast<uint4*>(a.xh_out + rowi * C + kk * 32 + kq * 8) = cv.u;
          }
        }
        if constexpr (STORE) {
          if (kq == 0) {
            a.rstd_out[rowi] = rstd;
            if (a.mean_out) a.mean_out[rowi] = mean;
          }
        }
      }
    }
  }

  mf_f32x4 oacc[MODE == 1 ? MF : 1][MODE == 1 ? NF : 1];
  if constexpr (MODE == 1) {
    mfma_zero(oacc);
  }

  // fc1 of one hidden sub-chunk (roles swapped): acc[hf][mf][r] = H[pixel mf*16 + p][hidden 32*hs + hf*16 + q*4 + r];
  // `W` = the W1 fragments of that sub-chunk in a stage buffer (+ lane * 16)
  auto gemm1 = [&](const char* W, const auto& xfr, mf_f32x4 (&acc)[2][MF]) {
    mfma_zero(acc);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const mf_bf16x8 wa = *reinterpret_cast<const mf_bf16x8*>(W + (hf * KK + kk) * 1024);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[hf][mf] = mfma16(wa, xfr[mf][kk], acc[hf][mf]);
      }
  };
  // bias, GELU, GRN in registers (same rounding points as the unfused kernels: h and g are bf16 values); MODE 0 adds g^2
  // into sq, MODE 1 packs z = g * s + beta as the fc2 A fragments
  // MODE 2: h / g of two consecutive sub-chunks are parked in a wave-private LDS tile [2 outputs][WM rows][64 hidden] and
  // leave as 16-byte vectors, 128-byte row segments (8-byte stores straight from the accumulator layout — 32-byte segments —
  // ran at 2.4-2.8 TB/s and made this pass slower than the unfused GEMM)
  char* sb = obuf + wave * ((STORE_H ? 2 : 1) * WM * G::OB_RS);
  auto activate = [&](int hs, const mf_f32x4 (&acc)[2][MF], mf_bf16x8 (&zf)[MF]) {
    const float* vb = vec + hs * 32 + kq * 4;
    float b1v[2][4], sv[2][4], bv[2][4];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 t1 = G::B1_IN_PADS ? *reinterpret_cast<const float4*>(obuf + (hs * 8 + hf * 4 + kq) * G::OB_RS + 128)
                                      : *reinterpret_cast<const float4*>(vb + hf * 16);
      b1v[hf][0] = t1.x; b1v[hf][1] = t1.y; b1v[hf][2] = t1.z; b1v[hf][3] = t1.w;
      if constexpr (MODE == 1) {
        const float4 t2 = *reinterpret_cast<const float4*>(vb + H4 + hf * 16);
        const float4 t3 = *reinterpret_cast<const float4*>(vb + 2 * H4 + hf * 16);
        sv[hf][0] = t2.x; sv[hf][1] = t2.y; sv[hf][2] = t2.z; sv[hf][3] = t2.w;
        bv[hf][0] = t3.x; bv[hf][1] = t3.y; bv[hf][2] = t3.z; bv[hf][3] = t3.w;
      }
    }
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      // all 8 table reads of this pixel fragment are issued before the first is consumed (one LDS latency, not eight)
      uint32_t P[4];
      float rr[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          // h as a bf16 pair; its magnitude bits index the table
          const vsx_v2f hb = (vsx_v2f){acc[hf][mf][r], acc[hf][mf][r + 1]} + (vsx_v2f){b1v[hf][r], b1v[hf][r + 1]};  // v_pk_add_f32
          const uint32_t Pq = f32x2_to_bf16x2_bits(hb.x, hb.y);
          P[hf * 2 + r / 2] = Pq;
          int a0 = (int)(Pq & 0x7FFFu), a1 = (int)((Pq >> 16) & 0x7FFFu);
          a0 = a0 < MLP_GT_BASE ? MLP_GT_BASE : (a0 > MLP_GT_LIM - 1 ? MLP_GT_LIM - 1 : a0);
          a1 = a1 < MLP_GT_BASE ? MLP_GT_BASE : (a1 > MLP_GT_LIM - 1 ? MLP_GT_LIM - 1 : a1);
          rr[hf * 4 + r] = gt[a0 - MLP_GT_BASE];
          rr[hf * 4 + r + 1] = gt[a1 - MLP_GT_BASE];
        }
      float z[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const uint32_t Pq = P[hf * 2 + r / 2];
          const uint32_t Rq = mlp_relu_pair(Pq);  // relu on the pair, then unpack: 3 instructions per pair instead of 4
          const vsx_v2f gg = (vsx_v2f){__uint_as_float(Rq << 16), __uint_as_float(Rq & 0xFFFF0000u)} -
                             (vsx_v2f){rr[hf * 4 + r], rr[hf * 4 + r + 1]};                                      // v_pk_add_f32 (neg)
          const uint32_t Gq = f32x2_to_bf16x2_bits(gg.x, gg.y);
          if constexpr (STATS) {
            // g (and h) are parked in the wave-private tile [WM pixels][hidden]: the stores leave from there, and the GRN
            // statistics are taken from the parked g by the matrix cores (stats_mfma below) — no per-lane squares, no DPP sums
            char* d = sb + (mf * 16 + p16) * G::OB_RS + ((STORE ? (hs & 1) * 32 : 0) + hf * 16 + kq * 4 + r) * 2;
            if constexpr (STORE_H) {
              *reinterpret_cast<uint32_t*>(d) = Pq;
              *reinterpret_cast<uint32_t*>(d + WM * G::OB_RS) = Gq;
            } else {
              *reinterpret_cast<uint32_t*>(d) = Gq;
            }
          } else {
            const float g0 = __uint_as_float(Gq << 16), g1 = __uint_as_float(Gq & 0xFFFF0000u);
            z[hf * 4 + r] = fmaf(g0, sv[hf][r], bv[hf][r]);
            z[hf * 4 + r + 1] = fmaf(g1, sv[hf][r + 1], bv[hf][r + 1]);
          }
        }
      if constexpr (MODE == 1) {
        union { uint4 u; mf_bf16x8 v; } pk;
        pk.u = pack<bf16_t>(z);
        zf[mf] = pk.v;
      }
    }
  };

  // Column sums over this wave's WM = 32 pixels by the matrix cores, from a bf16 tile parked row-major [pixel][hidden] in LDS:
  // the transposing read (ds_read_b64_tr_b16) hands lane (j, kq) 8 pixels of hidden column j — an MFMA operand whose
  // contraction index is the pixel.  X . X^T has the sums of squares on its diagonal (products of bf16 values are exact in
  // fp32: the arithmetic of fmaf(g, g, acc), in another order); X . 1 has the plain sums in every column.  Replaces 8 squares +
  // 32 DPP steps per lane and sub-chunk (a quarter of the VALU instructions of these passes: round 4).
  auto tile_frag = [&](const char* tile, int col0) -> mf_bf16x8 { return lds_tr8(tile, G::OB_RS, col0, p16, kq); };
  auto stats_mfma = [&](int hs, float* rw) {  // rw[32] = sum over the wave's pixels of g^2, this sub-chunk's 32 columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const char* gt_ = sb + (STORE_H ? WM * G::OB_RS : 0);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const mf_bf16x8 X = tile_frag(gt_, (STORE ? (hs & 1) * 32 : 0) + ct * 16);
      const mf_f32x4 D = mfma16(X, X, (mf_f32x4){0.f, 0.f, 0.f, 0.f});
      // lane (n, q) holds D[4q + i][n]: the diagonal element of column n sits in lane (n, n / 4), register n % 4
      const int i = p16 & 3;
      const float dsel = i == 0 ? D[0] : (i == 1 ? D[1] : (i == 2 ? D[2] : D[3]));
      if (kq == (p16 >> 2)) rw[ct * 16 + p16] = dsel;
    }
  };
  auto colsum_mfma = [&](int hs, float* rw) {  // rw[32] = sum over the wave's pixels of the parked tile (dh), 32 columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const mf_bf16x8 X = tile_frag(sb, (hs & 1) * 32 + ct * 16);
      if constexpr (LNF) {  // the parked tile holds dh' = dh * rstd: sigma-weighted sums = sums of dh; mean-weighted sums = u
        mf_f32x4 D = mfma16(X, wS, (mf_f32x4){0.f, 0.f, 0.f, 0.f});
        D = mfma16(X, wSl, D);
        mf_f32x4 U = mfma16(X, wMh, (mf_f32x4){0.f, 0.f, 0.f, 0.f});
        U = mfma16(X, wMl, U);
        if (p16 == 0) {
          *reinterpret_cast<float4*>(rw + ct * 16 + kq * 4) = make_float4(D[0], D[1], D[2], D[3]);
          *reinterpret_cast<float4*>(rw + NW * 32 + ct * 16 + kq * 4) = make_float4(U[0], U[1], U[2], U[3]);
        }
      } else {
        const mf_f32x4 D = mfma16(X, mf_ones8(), (mf_f32x4){0.f, 0.f, 0.f, 0.f});
        if (p16 == 0) *reinterpret_cast<float4*>(rw + ct * 16 + kq * 4) = make_float4(D[0], D[1], D[2], D[3]);
      }
    }
  };

  // ---- MODE 3 / 4: the stored activation (MODE 3: g, MODE 4: h) of a PAIR of sub-chunks travels HBM -> registers (16-byte
  // vectors, 128-byte row segments, issued two sub-chunks ahead) -> a wave-private LDS tile [WM rows][64 hidden], from where
  // the accumulator layout reads 8 bytes per lane; MODE 4 writes dh over h in that tile and flushes it like MODE 2
  uint4 tq[BWD && !RE ? (WM * 8) / 64 : 1];
  auto tile_load = [&](int hs) {   // hs even: the pair (hs, hs + 1)
    if constexpr (BWD && !RE) {
#pragma unroll
      for (int i = 0; i < (WM * 8) / 64; ++i) {
        const int idx = lane + 64 * i, row = idx >> 3, ch = idx & 7;
        tq[i] = ldvec_stream<bf16_t>(a.tin + (size_t)(row0 + row) * H4 + hs * 32 + ch * 8, (a.nt & 2) != 0);
      }
    }
  };
  auto tile_write = [&]() {
    if constexpr (BWD && !RE) {
#pragma unroll
      for (int i = 0; i < (WM * 8) / 64; ++i) {
        const int idx = lane + 64 * i, row = idx >> 3, ch = idx & 7;
        const uint4 v = tq[i];  // through a value: a direct array -> LDS aggregate copy keeps the array in scratch
        *reinterpret_cast<uint4*>(sb + row * G::OB_RS + ch * 16) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  auto tile_flush = [&](int hs) {  // MODE 4 / 5: dh of the pair (hs - 1, hs), hs odd
    if constexpr (DH) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < (WM * 8) / 64; ++i) {
        const int idx = lane + 64 * i, row = idx >> 3, ch = idx & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(sb + row * G::OB_RS + ch * 16);
        stvec_stream(a.hout + (size_t)(row0 + row) * H4 + (hs - 1) * 32 + ch * 8, v, (a.nt & 1) != 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  // backward activation of one sub-chunk: acc = dz (fp32) of [WM pixels] x [32 hidden] in the accumulator layout
  auto bwd_act = [&](int hs, const mf_f32x4 (&acc)[2][MF], const mf_f32x4 (&hacc)[2][MF], float (&r0)[2][4], float (&r1)[2][4]) {
    if constexpr (BWD) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) { r0[hf][r] = 0.f; r1[hf][r] = 0.f; }
      float sv[2][4], tv[2][4], b1v[2][4];
      if constexpr (DH) {
        const float* vb = vec + hs * 32 + kq * 4;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const float4 t2 = *reinterpret_cast<const float4*>(vb + hf * 16);
          const float4 t3 = *reinterpret_cast<const float4*>(vb + H4 + hf * 16);
          sv[hf][0] = t2.x; sv[hf][1] = t2.y; sv[hf][2] = t2.z; sv[hf][3] = t2.w;
          tv[hf][0] = t3.x; tv[hf][1] = t3.y; tv[hf][2] = t3.z; tv[hf][3] = t3.w;
          if constexpr (RE) {
            const float4 t4 = *reinterpret_cast<const float4*>(vb + 2 * H4 + hf * 16);
            b1v[hf][0] = t4.x; b1v[hf][1] = t4.y; b1v[hf][2] = t4.z; b1v[hf][3] = t4.w;
          }
        }
      }
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          char* tp = sb + (mf * 16 + p16) * G::OB_RS + ((hs & 1) * 32 + hf * 16 + kq * 4) * 2;
          uint2 tw;  // the pre-activation h (MODE 4 / 5) or the activation g (MODE 3) as two bf16 pairs
          if constexpr (RE) {  // recomputed: the forward's accumulator + bias, rounded to bf16 as the stored h was
            const vsx_v2f ha = (vsx_v2f){hacc[hf][mf][0], hacc[hf][mf][1]} + (vsx_v2f){b1v[hf][0], b1v[hf][1]};
            const vsx_v2f hc = (vsx_v2f){hacc[hf][mf][2], hacc[hf][mf][3]} + (vsx_v2f){b1v[hf][2], b1v[hf][3]};
            tw.x = f32x2_to_bf16x2_bits(ha.x, ha.y);
            tw.y = f32x2_to_bf16x2_bits(hc.x, hc.y);
          } else {
            tw = *reinterpret_cast<const uint2*>(tp);
          }
          if constexpr (MODE == 3) {
            const float e[4] = {__uint_as_float(tw.x << 16), __uint_as_float(tw.x & 0xFFFF0000u), __uint_as_float(tw.y << 16),
                                __uint_as_float(tw.y & 0xFFFF0000u)};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float dz = acc[hf][mf][r];   // (fp32: the per-sample-product route to the same statistics never rounds dz either)
              r0[hf][r] = fmaf(dz, e[r], r0[hf][r]);
              r1[hf][r] += dz;
            }
          } else {
            // gelu(h) = max(h, 0) - r(|h|) and gelu'(h) = 1/2 + sign(h) * d(|h|), d(a) = Phi(a) + a * phi(a) - 1/2, BOTH from one
            // 8-byte gather of the {r, d} table indexed by the magnitude bits of the bf16 value h (the forward's table, computed
            // in double): 2 VALU operations per element where the erf / exp evaluation (gelu_parts2) took 11 (round 4)
            float2 tb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t w = r < 2 ? tw.x : tw.y;
              int a0 = (int)((r & 1) ? (w >> 16) & 0x7FFFu : w & 0x7FFFu);
              a0 = a0 < MLP_GT_BASE ? MLP_GT_BASE : (a0 > MLP_GT_LIM - 1 ? MLP_GT_LIM - 1 : a0);
              tb[r] = *reinterpret_cast<const float2*>(gt + 2 * (a0 - MLP_GT_BASE));
            }
            uint32_t ob[2];
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              const uint32_t w = r < 2 ? tw.x : tw.y;
              const float h0 = __uint_as_float(w << 16), h1 = __uint_as_float(w & 0xFFFF0000u);
              // dz enters in fp32, straight from the accumulator (until round 5 it was first rounded to bf16, "as the unfused GEMM
              // stores it" — 1.5 VALU operations per element for a LESS accurate dh; the unfused pair differs by that rounding)
              const vsx_v2f d2 = {acc[hf][mf][r], acc[hf][mf][r + 1]};
              const vsx_v2f s2 = {sv[hf][r], sv[hf][r + 1]}, t2 = {tv[hf][r], tv[hf][r + 1]};
              const uint32_t Rq = mlp_relu_pair(w);
              const vsx_v2f gv = (vsx_v2f){__uint_as_float(Rq << 16), __uint_as_float(Rq & 0xFFFF0000u)} - (vsx_v2f){tb[r].x, tb[r + 1].x};
              const vsx_v2f cs = {copysignf(tb[r].y, h0), copysignf(tb[r + 1].y, h1)};
              const vsx_v2f dgv = cs + (vsx_v2f){0.5f, 0.5f};
              vsx_v2f rr = (d2 * s2 + gv * t2) * dgv;
              if constexpr (LNF) rr = rr * (vsx_v2f){rsr[mf], rsr[mf]};
              ob[r / 2] = f32x2_to_bf16x2_bits(rr.x, rr.y);
            }
            *reinterpret_cast<uint2*>(tp) = make_uint2(ob[0], ob[1]);  // dh parked: colsum_mfma and tile_flush read it
          }
        }
    }
  };

  // ---- software pipeline over the hidden sub-chunks.  Stage s (buffer s & 1) = [W1 of sub-chunk s + 1 | W2 of sub-chunk s]:
  // while the VALU works through bias / GELU / GRN of sub-chunk s, the SAME wave's MFMA pipe already runs fc1 of sub-chunk
  // s + 1 (independent instructions in one basic block), then fc2 of sub-chunk s.  Without the shift every wave of the
  // workgroup sits in the same phase between two barriers — all in MFMA, then all in VALU — and the two pipes never overlap
  // (measured: 29 % MFMA utilisation on the C = 224 blocks).
  auto stage_load2 = [&](int s, char* dst) {
    // W1 pieces of sub-chunk s + 1 (absent for the last stage), W2 pieces of sub-chunk s
    const char* src1 = a.wimg + (size_t)(s + 1) * (G::IMG_PIECES * 1024) + lane * 16;
    // MODE 5: the second half of a stage = the W1' pieces of sub-chunk s + 1 out of the FORWARD image (both halves feed the
    // next sub-chunk's two accumulator sets)
    const char* src2 = RE ? a.wimg2 + (size_t)(s + 1) * (G::IMG_PIECES * 1024) - G::W1_PIECES * 1024 + lane * 16
                          : a.wimg + (size_t)s * (G::IMG_PIECES * 1024) + lane * 16;
    if (wave >= DW) return;
    for (int p = wave; p < G::NP; p += DW) {
      if ((RE || p < G::W1_PIECES) && s + 1 >= NHS) continue;
      const char* src = p < G::W1_PIECES ? src1 : src2;
      lds_dma16(src + p * 1024, dst + p * 1024);
    }
  };
  // MODE 2: lane (p, q) owns hidden q*4 .. q*4+3 of pixel p in each 16-column half: two 8-byte stores per output and
  // fragment; the two halves of a sub-chunk complete a 64-byte row segment, consecutive sub-chunks the cache lines
  auto store_pending = [&](int hs) {  // hs = the ODD sub-chunk of the pair (hs - 1, hs) parked in the staging tile
    if constexpr (STORE) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int idx = lane; idx < (STORE_H ? 2 : 1) * WM * 8; idx += 64) {
        const int o = idx / (WM * 8), rem = idx - o * (WM * 8);
        const int row = rem >> 3, ch = rem & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(sb + (o * WM + row) * G::OB_RS + ch * 16);
        bf16_t* dst = (o || !STORE_H ? a.gout : a.hout) + (size_t)(row0 + row) * H4 + (hs - 1) * 32 + ch * 8;
        stvec_stream(dst, v, (a.nt & 1) != 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  mf_f32x4 hcur[2][MF], hnxt[2][MF];
  mf_f32x4 gcur[RE ? 2 : 1][RE ? MF : 1], gnxt[RE ? 2 : 1][RE ? MF : 1];  // MODE 5: the recomputed fc1 accumulators
  // prologue: W1 of sub-chunk 0 goes where "stage -1" would sit (buffer 1)
  {
    const char* src = a.wimg + lane * 16;
    for (int p = wave; p < G::W1_PIECES; p += NW) lds_dma16(src + p * 1024, buf1 + p * 1024);
    if constexpr (RE) {
      const char* srcf = a.wimg2 + lane * 16;
      for (int p = wave; p < G::W1_PIECES; p += NW) lds_dma16(srcf + p * 1024, buf1 + (G::W1_PIECES + p) * 1024);
    }
  }
  stage_load2(0, buf0);
  tile_load(0);
  wait_vm<0>();
  __syncthreads();
  gemm1(buf1 + lane * 16, xf, hcur);
  if constexpr (RE) gemm1(buf1 + G::W1_PIECES * 1024 + lane * 16, xg, gcur);
  // every wave must be done reading sub-chunk 0's fragments out of buffer 1 before step 0 refills that buffer by LDS-DMA.  (This
  // barrier was missing until round 4: a fast wave's prefetch could overwrite the fragments a slow wave was still multiplying —
  // hidden by the DMA latency while one workgroup owned the CU, exposed as wrong hidden columns 16..31 of the first sub-chunk in
  // whole 32-row groups once two workgroups shared a CU at C = 192 / 224: tools/det_fwd.py.)
  __syncthreads();

  // column sums of the sub-chunk `hq` of dh (parked in `red` before the last barrier): one workspace row per workgroup, no
  // atomics.  MODE 7: two sums per column (lanes 0-31: of the unscaled dh, lanes 32-63: u), rows of 2 * 4C floats
  auto ws_row = [&](int hq, bool on) {
    if constexpr (LNF) {
      if (on && wave == hq % DW) {
        const float* r = red + (hq & 1) * 2 * NW * 32 + (lane >> 5) * NW * 32 + (lane & 31);
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += r[w * 32];
        a.ws[(size_t)blockIdx.x * 2 * H4 + (lane >> 5) * H4 + hq * 32 + (lane & 31)] = t;
      }
    } else {
      if (on && wave == hq % DW && lane < 32) {
        const float* r = red + (hq & 1) * NW * 32 + lane;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += r[w * 32];
        a.ws[(size_t)blockIdx.x * H4 + hq * 32 + lane] = t;
      }
    }
  };
  auto step = [&](int hs, const char* Sb, char* other) {
    // stage hs has landed for everyone (waited + barrier by the caller); every wave is done with stage hs - 1 in `other`
    if constexpr (STORE) {
      if (hs > 0 && (hs & 1) == 0) store_pending(hs - 1);  // issued BEFORE the prefetch: the next vmcnt(0) then waits for
                                                           // stores that have had a whole sub-chunk to complete
    }
    if constexpr (BWD) {
      if ((hs & 1) == 0) {  // pair boundary: the vmcnt(0) the caller just passed covered this pair's loads and the last stores
        if (hs > 0) tile_flush(hs - 1);
        tile_write();
        if (hs + 2 < NHS) tile_load(hs + 2);
      }
    }
    MLP_STAMP(1);
    if (hs + 1 < NHS) stage_load2(hs + 1, other);
    const char* S = Sb + lane * 16;
    if constexpr (MODE == 3) {
      if (hs > 0 && wave == (hs - 1) % DW) {  // P (lanes 0-31) and S (lanes 32-63) of the previous sub-chunk
        const float* r = red + ((hs - 1) & 1) * 2 * NW * 32 + (lane >> 5) * NW * 32 + (lane & 31);
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += r[w * 32];
        atomicAdd((lane < 32 ? a.red0 : a.red1) + (size_t)b * H4 + (hs - 1) * 32 + (lane & 31), t);
      }
    }
    if constexpr (DH) ws_row(hs - 1, hs > 0);
    if constexpr (STATS) {
      if (hs > 0 && wave == (hs - 1) % DW && lane < 32) {  // column sums of the previous sub-chunk (parked before the barrier)
        const float* r = red + ((hs - 1) & 1) * NW * 32 + lane;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += r[w * 32];
        if (a.ws) a.ws[(size_t)blockIdx.x * H4 + (hs - 1) * 32 + lane] = t;   // det_reduce: one workspace row per workgroup
        else atomicAdd(a.colsq + (size_t)b * H4 + (hs - 1) * 32 + lane, t);
      }
    }
    mf_bf16x8 zf[MF];
    // three scheduling regions.  Inside the GEMM regions the fragment reads run three ahead of the MFMAs that consume them
    // (left alone, hipcc sinks every ds_read_b128 to just before its two MFMAs: read - wait - MFMA - MFMA chains with every
    // LDS latency exposed — 31 waits per sub-chunk at C = 224); the activation region in between is left to the compiler
    // (it batches the eight table reads of a fragment by itself)
    __builtin_amdgcn_sched_barrier(0);
    MLP_STAMP(2);
    gemm1(S, xf, hnxt);  // fc1 of the NEXT sub-chunk (the last step multiplies stale fragments, result unused)
    if constexpr (RE) gemm1(S + G::W1_PIECES * 1024, xg, gnxt);
    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
    for (int i = 0; i < (RE ? 4 : 2) * KK; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, MF, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    MLP_STAMP(3);
    float q0[2][4], q1[2][4];
    if constexpr (RE) bwd_act(hs, hcur, gcur, q0, q1);
    else if constexpr (BWD) bwd_act(hs, hcur, hcur, q0, q1);
    else activate(hs, hcur, zf);
    __builtin_amdgcn_sched_barrier(0);
    MLP_STAMP(4);
    if constexpr (DH) {
      colsum_mfma(hs, red + (hs & 1) * (LNF ? 2 : 1) * NW * 32 + wave * 32);  // column sums of the parked dh (the fc1 bias gradient)
    } else if constexpr (BWD) {
      float* rw = red + (hs & 1) * 2 * NW * 32 + wave * 32;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t0 = group_sum<16>(q0[hf][r]);
          if (p16 == 0) rw[hf * 16 + kq * 4 + r] = t0;
          const float t1 = group_sum<16>(q1[hf][r]);
          if (p16 == 0) rw[NW * 32 + hf * 16 + kq * 4 + r] = t1;
        }
    } else if constexpr (STATS) {
      stats_mfma(hs, red + (hs & 1) * NW * 32 + wave * 32);  // sum over this wave's pixels of g^2 (the GRN statistics)
    } else {
      // fc2: out[pixel][n] += Z[pixel][32 hidden] . W2[n][same 32 hidden, permuted alike in the image]
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const mf_bf16x8 wb = *reinterpret_cast<const mf_bf16x8*>(S + (G::W1_PIECES + nf) * 1024);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) oacc[mf][nf] = mfma16(zf[mf], wb, oacc[mf][nf]);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, MF, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    MLP_STAMP(5);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        hcur[hf][mf] = hnxt[hf][mf];
        if constexpr (RE) gcur[hf][mf] = gnxt[hf][mf];
      }
  };

  // A/B knob (round 6; MI355X_MICROARCH.md "two waves per SIMD", item 4): one static s_setprio for the second-dispatched half of
  // the workgroup (a.nt bit 2) or for the first half (bit 3) — the arbiter serves priority, then age, so waves 0 - 3 reach every
  // barrier ~1 000 cycles before waves 4 - 7 (profiles/r05_mlp_timeline.txt).  `wave` and a.nt are scalar: a scalar branch.
  if (a.nt & 4) { if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1); }
  if (a.nt & 8) { if (wave < NW / 2) __builtin_amdgcn_s_setprio(1); }
  static_assert(NHS % 2 == 0, "the hidden axis is walked two sub-chunks (one per stage buffer) per loop trip");
#pragma unroll 1
  for (int hs = 0; hs < NHS; hs += 2) {
    if (hs > 0) {
      wait_vm<0>();
      { const int hs_ = hs; { const int hs = hs_ - 1; MLP_STAMP(6); } }
      __syncthreads();
    }
    MLP_STAMP(0);
    step(hs, buf0, buf1);
    wait_vm<0>();
    MLP_STAMP(6);
    __syncthreads();
    { const int hs_ = hs; { const int hs = hs_ + 1; MLP_STAMP(0); } }
    step(hs + 1, buf1, buf0);
  }

  if constexpr (BWD) {
    tile_flush(NHS - 1);
    __syncthreads();
    if constexpr (MODE == 3) {
      if (wave == (NHS - 1) % DW) {
        const float* r = red + ((NHS - 1) & 1) * 2 * NW * 32 + (lane >> 5) * NW * 32 + (lane & 31);
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += r[w * 32];
        atomicAdd((lane < 32 ? a.red0 : a.red1) + (size_t)b * H4 + (NHS - 1) * 32 + (lane & 31), t);
      }
    } else {
      ws_row(NHS - 1, true);
    }
    return;
  } else if constexpr (STATS) {
    store_pending(NHS - 1);
    __syncthreads();
    if (wave == (NHS - 1) % DW && lane < 32) {
      const float* r = red + ((NHS - 1) & 1) * NW * 32 + lane;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += r[w * 32];
      if (a.ws) a.ws[(size_t)blockIdx.x * H4 + (NHS - 1) * 32 + lane] = t;
      else atomicAdd(a.colsq + (size_t)b * H4 + (NHS - 1) * 32 + lane, t);
    }
    return;
  } else {
    const float rs = a.rscale ? a.rscale[b] : 1.f;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const float bias = vec[3 * H4 + nf * 16 + p16];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[mf][nf][r] = (oacc[mf][nf][r] + bias) * rs;
    }
    // shortcut: OUT += RES . I  (B fragment of the identity: lane (n, q) holds 1.0 at slot j = h2*16 + n - q*8)
    mf_bf16x8 idB[2];
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      union { unsigned short h[8]; mf_bf16x8 v; } u;
#pragma unroll
      for (int j = 0; j < 8; ++j) u.h[j] = (h2 * 16 + p16 == kq * 8 + j) ? (unsigned short)0x3F80 : (unsigned short)0;
      idB[h2] = u.v;
    }
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const mf_bf16x8 rf = *reinterpret_cast<const mf_bf16x8*>(a.res + (size_t)(row0 + mf * 16 + p16) * C + kk * 32 + kq * 8);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) oacc[mf][kk * 2 + h2] = mfma16(rf, idB[h2], oacc[mf][kk * 2 + h2]);
      }
    // per-wave transpose through LDS, 64 columns at a time: accumulator layout (4 rows x 1 column per lane) -> 16-byte
    // vectors, 8 lanes per 128-byte row segment
    char* ost = obuf + wave * (WM * G::OB_RS);
    bf16_t* orow = a.out + (size_t)row0 * C;
#pragma unroll
    for (int cb = 0; cb < NF; cb += 4) {
      const int nfe = cb + 4 < NF ? cb + 4 : NF;
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = cb; nf < cb + 4; ++nf) {
          if (nf < NF) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *reinterpret_cast<unsigned short*>(ost + (mf * 16 + kq * 4 + r) * G::OB_RS + ((nf - cb) * 16 + p16) * 2) =
                  (unsigned short)f32_to_bf16_bits(oacc[mf][nf][r]);
          }
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int chs = (nfe - cb) * 2;  // 16-byte chunks per row in this block (8 for a full block)
      for (int idx = lane; idx < WM * chs; idx += 64) {
        const int row = idx / chs, ch = idx - row * chs;
        const uint4 v = *reinterpret_cast<const uint4*>(ost + row * G::OB_RS + ch * 16);
        *reinterpret_cast<uint4*>(orow + (size_t)row * C + cb * 16 + ch * 8) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// Two builds of the same body (round 5).  hipcc packs the fp32 arithmetic of the activation code into v_pk_add / v_pk_mul /
// v_pk_fma_f32 — half the VALU instructions, but on gfx950 a packed-fp32 instruction next to matrix instructions is an
// anti-lever (tools/micro/mfma_valu_overlap2.hip, MI355X: a wave that issues ONE v_pk_*_f32 behind each
// v_mfma_f32_16x16x32_bf16 takes 4 000 cycles for 128 MFMAs instead of 2 240 — ~15 cycles per packed instruction — while up
// to TWO plain v_fma / v_mul / v_and / v_cvt_pk_bf16 per MFMA are free; between waves of one SIMD the packed forms add to the
// other wave's MFMA time (2 300 cycles = the sum) where the scalar forms overlap in part (1 700 - 1 800)).  The forward passes
// (MODE 6 at 4 waves per SIMD: -15 .. -20 % at C = 192 / 224; MODE 0 -6 %; tools/perf_mlp_train.py, same box) run the SCALAR
// build (`no-packed-fp32-ops`); the dh passes spend 13 VALU operations per hidden element at 2 waves per SIMD, are bound by
// their VALU issue inside the activation region and keep the packed build (+2.5 % otherwise).  `mlp_sf32` (vsx_set_flag):
// bit m = MODE m runs the scalar build.
template <int C, int MF, int NW, int MODE>
__global__ __launch_bounds__(NW * 64, (MODE == 4 && NW == 8 && C == 96 ? 4 : 1)) void mlp_fused_kernel(const MlpArgs a) {
  mlp_fused_body<C, MF, NW, MODE>(a);
}
template <int C, int MF, int NW, int MODE>
__global__ __launch_bounds__(NW * 64, (MODE == 4 && NW == 8 && C == 96 ? 4 : 1)) __attribute__((target("no-packed-fp32-ops")))
void mlp_fused_kernel_sf(const MlpArgs a) {
  mlp_fused_body<C, MF, NW, MODE>(a);
}

// ------------------------------------------------------------------------------------------------ weight image
// (layout and body: csrc/wtasks.h — shared with the task-list kernel vsx_weight_tasks)
__global__ __launch_bounds__(256) void mlp_pack_kernel(const bf16_t* __restrict__ W1, const bf16_t* __restrict__ W2,
                                                       char* __restrict__ img, int C) {
  wt_mlp_pack(blockIdx.x, W1, W2, img, C);
}

// ------------------------------------------------------------------------------------------------ dispatch
struct MlpCfg { int C, MF, NW, modes; };  // modes: bit m set = this geometry serves MODE m
// rows per workgroup must divide the pixels of a sample; the large maps take 256-row workgroups (8 waves x 32 rows: weight
// traffic L2 -> LDS per flop is 1 / rows).  C = 384 lives on 16 x 16 maps (256 rows = one sample): its TRAINING passes (MODE 2 / 3 /
// 4, no fc2 accumulators) fit 8 waves at <= 256 registers and sit behind bit 2 of the mlp_fused flag (fc1 -12 %, backward -4 %,
// -0.7 GB per block and step at B = 512).  The C = 384 inference pair (the output pass needs 192 accumulator registers: 4 waves x
// 32 rows at one wave per SIMD, 875 us against 614 us for the unfused GEMMs at B = 512) was removed in round 4 (flag bit 4).
static inline int mlp_nt() { return (g_vsx_nt_stream >> 2) & 15; }  // bits 2 / 3 of nt_stream: the fused passes' stores / last-reader loads; bits 4 / 5: static wave priority (A/B knob, see the kernel)
static const MlpCfg kMlpCfgs[] = {{96, 2, 8, 255}, {192, 2, 8, 255}, {224, 2, 8, 255}, {384, 2, 8, 4 | 8 | 16}};

static const MlpCfg* mlp_cfg(int C, int hw, long M, int mode) {
  for (const MlpCfg& c : kMlpCfgs) {
    const int bm = c.NW * 16 * c.MF;
    if (!(c.modes & (1 << mode))) continue;
    if (c.C == 384 && !(g_vsx_mlp_fused & 4)) continue;  // bit 2: the training passes (MODE 2 / 3 / 4) on the C = 384 blocks
    if ((mode == 5 || mode == 6 || mode == 7) && !(g_vsx_mlp_fused & 64)) continue;  // bit 6: the pre-activation h is recomputed, not stored
    if (mode == 7 && !(g_vsx_mlp_fused & 128)) continue;                             // bit 7: ... and neither are the normalised rows x^
    if (c.C == C && hw % bm == 0 && M % bm == 0) return &c;
  }
  return nullptr;
}

/* inference pair (MODE 0 + 1) available? */
extern "C" int32_t vsx_mlp_supported(int32_t C, int32_t hw, int64_t M, int32_t dtype) {
  return dtype == VSX_BF16 && mlp_cfg(C, hw, M, 0) != nullptr && mlp_cfg(C, hw, M, 1) != nullptr;
}
/* one pass: mode 0 statistics, 1 output, 2 training fc1, 3 backward statistics, 4 backward dh, 5 backward dh with the
 * pre-activation recomputed (vsx_mlp_bwd_dh_re), 6 training fc1 that stores g only (vsx_mlp_fc1 / _ln with h = NULL),
 * 7 mode 5 that also re-normalises the block's LayerNorm input (vsx_mlp_bwd_dh_ln: x^ is never stored) */
extern "C" int32_t vsx_mlp_mode_supported(int32_t C, int32_t hw, int64_t M, int32_t mode, int32_t dtype) {
  return dtype == VSX_BF16 && mode >= 0 && mode <= 7 && mlp_cfg(C, hw, M, mode) != nullptr;
}

extern "C" int64_t vsx_mlp_image_bytes(int32_t C) { return (int64_t)(4 * C / 32) * (2 * (C / 32) + C / 16) * 1024; }

extern "C" int32_t vsx_mlp_pack(const void* W1, const void* W2, void* img, int32_t C, vsx_stream_t stream) {
  VSX_CHECK(W1 && W2 && img && C > 0 && C % 32 == 0, "vsx_mlp_pack: bad arguments (C = %d must be a multiple of 32)", C);
  const long total = (long)(4 * C / 32) * (2 * (C / 32) + C / 16) * 64;
  hipLaunchKernelGGL(mlp_pack_kernel, dim3(vsx_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W1,
                     (const bf16_t*)W2, (char*)img, C);
  VSX_LAUNCH_CHECK();
  return 0;
}

template <int C, int MF, int NW, int MODE>
static int mlp_launch(const MlpArgs& a, hipStream_t s) {
  typedef MlpGeom<C, MF, NW, MODE> G;
  if (g_vsx_mlp_sf32 & (1 << MODE)) hipLaunchKernelGGL((mlp_fused_kernel_sf<C, MF, NW, MODE>), dim3(a.M / G::BM), dim3(NW * 64), 0, s, a);
  else hipLaunchKernelGGL((mlp_fused_kernel<C, MF, NW, MODE>), dim3(a.M / G::BM), dim3(NW * 64), 0, s, a);
  VSX_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
static int mlp_dispatch(const MlpCfg* c, const MlpArgs& a, hipStream_t s) {
  if (c->C == 96) return mlp_launch<96, 2, 8, MODE>(a, s);
  if (c->C == 192) return mlp_launch<192, 2, 8, MODE>(a, s);
  if (c->C == 224) return mlp_launch<224, 2, 8, MODE>(a, s);
  if constexpr (MODE <= 1 || MODE >= 5) { vsx_set_error("vsx_mlp: mode %d is built for C <= 224", MODE); return 1; }  // (5, 6, 7)
  else return mlp_launch<384, 2, 8, MODE>(a, s);
}

// det_reduce: the statistics passes (MODE 0 / 2 / 6) leave one row of column sums per workgroup in the thread's workspace
// (vsx_det_workspace) and an ordered pass adds a sample's rows into colsq — no atomics, the same bits in every run
static long mlp_det_need(const MlpCfg* c, long M) { return M / (c->NW * 16 * c->MF) * 4 * c->C; }
static int mlp_det_begin(MlpArgs& a, const MlpCfg* c, const char* who) { return vsx_det_take(who, mlp_det_need(c, a.M), &a.ws); }
static int mlp_det_end(const MlpArgs& a, const MlpCfg* c, hipStream_t s) {
  if (!a.ws) return 0;
  const int bm = c->NW * 16 * c->MF;
  return vsx_det_group_sum(a.ws, 4 * c->C, 0, a.colsq, a.M / a.hw, a.hw / bm, 4 * c->C, s);
}

/* mode 0: colsq[b, 4C] += sum over the sample's pixels of gelu(fc1(xh))^2 (bf16-rounded g, as the unfused fc1 epilogue);
 * mode 1: out = res + rscale[b] * (fc2(gelu(fc1(xh)) * s[b] + beta) + b2). */
extern "C" int32_t vsx_mlp_gelu_table_len(void) { return 2 * MLP_GT_N; }

// For the bf16 value a whose magnitude bits are MLP_GT_BASE + i (double precision, once per process):
//   tab[i]            = r(a) = a * Phi(-a)                  gelu(h)  = max(h, 0) - r(|h|)
//   tab[MLP_GT_N + i] = d(a) = Phi(a) + a * phi(a) - 1/2    gelu'(h) = 1/2 + sign(h) * d(|h|)   (d >= 0; gelu'(-a) = 1 - gelu'(a))
__global__ void mlp_gelu_table_kernel(float* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= MLP_GT_N) return;
  const double a = (double)__uint_as_float((uint32_t)(MLP_GT_BASE + i) << 16);
  tab[i] = (float)(a * 0.5 * erfc(a * 0.70710678118654752440));
  const double Phi = 0.5 * erfc(-a * 0.70710678118654752440), phi = exp(-0.5 * a * a) * 0.39894228040143267794;
  tab[MLP_GT_N + i] = (float)(Phi + a * phi - 0.5);
}

extern "C" int32_t vsx_mlp_gelu_table(float* tab, vsx_stream_t stream) {
  VSX_CHECK(tab != nullptr, "vsx_mlp_gelu_table: null pointer");
  hipLaunchKernelGGL(mlp_gelu_table_kernel, dim3(vsx_cdiv(MLP_GT_N, 256)), dim3(256), 0, (hipStream_t)stream, tab);
  VSX_LAUNCH_CHECK();
  return 0;
}

// vsx_mlp_fwd and vsx_mlp_fwd_ln (ln_eps > 0: `xh` holds the un-normalised rows)
static int32_t mlp_fwd_impl(const void* xh, float ln_eps, const void* wimg, const float* b1, const float* grn_s, const float* grn_b,
                            const float* b2, const void* res, const float* rscale, void* out, float* colsq, const float* gtab,
                            int64_t M, int32_t C, int32_t hw, int32_t mode, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_fwd: bf16 only (the fp32 parity mode runs the unfused schedule)");
  VSX_CHECK(xh && wimg && b1 && gtab && M > 0 && hw > 0, "vsx_mlp_fwd: bad arguments");
  const MlpCfg* c = mlp_cfg(C, hw, M, mode == 0 ? 0 : 1);
  VSX_CHECK(c != nullptr, "vsx_mlp_fwd: unsupported shape C=%d hw=%d M=%ld (query vsx_mlp_supported first)", C, hw, (long)M);
  VSX_CHECK(M < (1ll << 31), "vsx_mlp_fwd: M too large");
  MlpArgs a = {};
  a.xh = (const bf16_t*)xh; a.wimg = (const char*)wimg; a.b1 = b1; a.gtab = gtab; a.M = (int)M; a.hw = hw; a.ln_eps = ln_eps;
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) {
    VSX_CHECK(colsq != nullptr, "vsx_mlp_fwd: mode 0 needs colsq");
    a.colsq = colsq;
    if (int e = mlp_det_begin(a, c, "vsx_mlp_fwd")) return e;
    if (int e = mlp_dispatch<0>(c, a, s)) return e;
    return mlp_det_end(a, c, s);
  }
  VSX_CHECK(mode == 1 && grn_s && grn_b && b2 && res && out, "vsx_mlp_fwd: mode 1 needs s, beta, b2, res, out");
  a.grn_s = grn_s; a.grn_b = grn_b; a.b2 = b2; a.res = (const bf16_t*)res; a.rscale = rscale; a.out = (bf16_t*)out;
  return mlp_dispatch<1>(c, a, s);
}

extern "C" int32_t vsx_mlp_fwd(const void* xh, const void* wimg, const float* b1, const float* grn_s, const float* grn_b,
                               const float* b2, const void* res, const float* rscale, void* out, float* colsq,
                               const float* gtab, int64_t M, int32_t C, int32_t hw, int32_t mode, int32_t dtype,
                               vsx_stream_t stream) {
  return mlp_fwd_impl(xh, 0.f, wimg, b1, grn_s, grn_b, b2, res, rscale, out, colsq, gtab, M, C, hw, mode, dtype, stream);
}

// vsx_mlp_fc1 and vsx_mlp_fc1_ln (ln_eps > 0: `xh` holds the un-normalised rows; xh_out / rstd_out / mean_out receive the
// normalised rows and the row statistics)
static int32_t mlp_fc1_impl(const void* xh, float ln_eps, void* xh_out, float* rstd_out, float* mean_out, const void* wimg,
                            const float* b1, float* colsq, const float* gtab, void* h, void* g, int64_t M, int32_t C, int32_t hw,
                            int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_fc1: bf16 only");
  VSX_CHECK(xh && wimg && b1 && colsq && gtab && g && M > 0 && hw > 0, "vsx_mlp_fc1: bad arguments");
  const MlpCfg* c = mlp_cfg(C, hw, M, h ? 2 : 6);
  VSX_CHECK(c != nullptr, "vsx_mlp_fc1: unsupported shape C=%d hw=%d M=%ld (query vsx_mlp_supported first)", C, hw, (long)M);
  VSX_CHECK(M < (1ll << 31), "vsx_mlp_fc1: M too large");
  MlpArgs a = {};
  a.xh = (const bf16_t*)xh; a.wimg = (const char*)wimg; a.b1 = b1; a.colsq = colsq; a.gtab = gtab; a.hout = (bf16_t*)h;
  a.gout = (bf16_t*)g; a.nt = mlp_nt(); a.M = (int)M; a.hw = hw;
  a.ln_eps = ln_eps; a.xh_out = (bf16_t*)xh_out; a.rstd_out = rstd_out; a.mean_out = mean_out;
  if (int e = mlp_det_begin(a, c, "vsx_mlp_fc1")) return e;
  if (int e = h ? mlp_dispatch<2>(c, a, (hipStream_t)stream) : mlp_dispatch<6>(c, a, (hipStream_t)stream)) return e;
  return mlp_det_end(a, c, (hipStream_t)stream);
}

/* training fc1 (MODE 2): h = bf16(xh . W1'^T + b1), g = bf16(gelu(h)) stored for the backward, colsq[b, 4C] += sum_hw g^2 —
 * the outputs of vsx_gemm_nt with VSX_EPI_BIAS_GELU_SQ, from the kernel that keeps its activation rows in registers.
 * h = NULL (MODE 6, where vsx_mlp_mode_supported(.., 6, ..)): only g is stored — the backward recomputes h (vsx_mlp_bwd_dh_re) */
extern "C" int32_t vsx_mlp_fc1(const void* xh, const void* wimg, const float* b1, float* colsq, const float* gtab, void* h,
                               void* g, int64_t M, int32_t C, int32_t hw, int32_t dtype, vsx_stream_t stream) {
  return mlp_fc1_impl(xh, 0.f, nullptr, nullptr, nullptr, wimg, b1, colsq, gtab, h, g, M, C, hw, dtype, stream);
}

/* The same passes with the block LayerNorm (eps, no affine: folded into W1' / b1) applied in the kernel's prologue: `y` holds
 * the UN-normalised rows (the depthwise convolution's output).  vsx_mlp_fwd_ln: modes 0 / 1 as vsx_mlp_fwd — the normalised
 * rows never exist in memory.  vsx_mlp_fc1_ln additionally writes them (xh_out [M, C]) and rstd_out [M] for the backward —
 * or, with xh_out = NULL and mean_out [M] given, only the two row statistics: the backward then re-normalises y itself
 * (vsx_mlp_bwd_dh_ln, vsx_gemm_nt with VSX_EPI_LN_BWD and a mean pointer) and x^ never exists in memory in training either.
 * Replaces vsx_ln_fwd + vsx_mlp_* (timm ConvNeXtBlock.norm -> .mlp, reached from viscy_models/unet/unext2.py:79). */
extern "C" int32_t vsx_mlp_fwd_ln(const void* y, float eps, const void* wimg, const float* b1, const float* grn_s,
                                  const float* grn_b, const float* b2, const void* res, const float* rscale, void* out,
                                  float* colsq, const float* gtab, int64_t M, int32_t C, int32_t hw, int32_t mode, int32_t dtype,
                                  vsx_stream_t stream) {
  VSX_CHECK(eps > 0.f, "vsx_mlp_fwd_ln: eps must be positive");
  return mlp_fwd_impl(y, eps, wimg, b1, grn_s, grn_b, b2, res, rscale, out, colsq, gtab, M, C, hw, mode, dtype, stream);
}
extern "C" int32_t vsx_mlp_fc1_ln(const void* y, float eps, void* xh_out, float* rstd_out, float* mean_out, const void* wimg,
                                  const float* b1, float* colsq, const float* gtab, void* h, void* g, int64_t M, int32_t C,
                                  int32_t hw, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(eps > 0.f && rstd_out && (xh_out || mean_out), "vsx_mlp_fc1_ln: eps must be positive, rstd_out and one of xh_out / mean_out non-null");
  return mlp_fc1_impl(y, eps, xh_out, rstd_out, mean_out, wimg, b1, colsq, gtab, h, g, M, C, hw, dtype, stream);
}

// ------------------------------------------------------------------------------------------------ backward passes
__global__ void reduce_rows_kernel(const float* __restrict__ ws, float* __restrict__ out, int R, int N);  // norm.hip

// what MODE 3 / 4 / 5 / 7 share: `xh` holds dout, `wimg` the backward image (W2^T, W2)
static MlpArgs mlp_bwd_args(const void* dout, const void* wimg, int64_t M, int32_t hw) {
  MlpArgs a = {};
  a.xh = (const bf16_t*)dout; a.wimg = (const char*)wimg; a.M = (int)M; a.hw = hw; a.nt = mlp_nt();
  return a;
}

/* MODE 3: the GRN statistics path of the block backward without a stored dz: dz = dout . W2 recomputed tile by tile
 * (wimg = vsx_mlp_pack of W2^T [4C, C] in the place of W1), P[b, 4C] += sum_hw dz * g, S[b, 4C] += sum_hw dz
 * (what the VSX_EPI_DZ epilogue of vsx_gemm_nt accumulates, minus its 4C-wide output) */
extern "C" int32_t vsx_mlp_bwd_stats(const void* dout, const void* wimg, const void* g, float* P, float* S, int64_t M, int32_t C,
                                     int32_t hw, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_bwd_stats: bf16 only");
  VSX_CHECK(dout && wimg && g && P && S && M > 0 && hw > 0, "vsx_mlp_bwd_stats: bad arguments");
  const MlpCfg* c = mlp_cfg(C, hw, M, 3);
  VSX_CHECK(c != nullptr && M < (1ll << 31), "vsx_mlp_bwd_stats: unsupported shape C=%d hw=%d M=%ld", C, hw, (long)M);
  MlpArgs a = mlp_bwd_args(dout, wimg, M, hw);
  a.tin = (const bf16_t*)g; a.red0 = P; a.red1 = S;
  return mlp_dispatch<3>(c, a, (hipStream_t)stream);
}

// The three dh passes (MODE 4 / 5 / 7) from here on: `a` carries the mode's own operands; s, t, dh, the gelu table and the
// workspace go in, the pass runs, and the per-workgroup rows of `ws` (wsN floats each) are added into colsum[wsN]
template <int MODE>
static int32_t mlp_bwd_dh_run(const char* who, MlpArgs& a, const float* s, const float* t, void* dh, float* ws, int64_t ws_rows,
                              float* colsum, int wsN, const float* gtab, int64_t M, int32_t C, int32_t hw, vsx_stream_t stream) {
  const MlpCfg* c = mlp_cfg(C, hw, M, MODE);
  VSX_CHECK(c != nullptr && M < (1ll << 31), "%s: unsupported shape C=%d hw=%d M=%ld", who, C, hw, (long)M);
  const int R = (int)(M / (c->NW * 16 * c->MF));
  VSX_CHECK(ws_rows >= R, "%s: workspace needs %d rows of %d floats", who, R, wsN);
  a.grn_s = s; a.grn_b = t; a.hout = (bf16_t*)dh; a.ws = ws; a.gtab = gtab;
  if (int e = mlp_dispatch<MODE>(c, a, (hipStream_t)stream)) return e;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(vsx_cdiv(wsN, 64), vsx_cdiv(R, 64)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, colsum, R, wsN);
  VSX_LAUNCH_CHECK();
  return 0;
}

/* MODE 4: dh = (dz * s[b] + gelu(h) * t[b]) * gelu'(h) with dz recomputed, stored [M, 4C]; colsum[4C] += sum over all pixels
 * of dh through ws ([M / rows-per-workgroup, 4C] floats, caller-owned) — vsx_gemm_nt(VSX_EPI_DZ) + vsx_grn_gelu_bwd in one
 * pass that writes the 4C-wide tensor once */
extern "C" int32_t vsx_mlp_bwd_dh(const void* dout, const void* wimg, const void* h, const float* s, const float* t, void* dh,
                                  float* ws, int64_t ws_rows, float* colsum, const float* gtab, int64_t M, int32_t C, int32_t hw,
                                  int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_bwd_dh: bf16 only");
  VSX_CHECK(dout && wimg && h && s && t && dh && ws && colsum && gtab && M > 0 && hw > 0, "vsx_mlp_bwd_dh: bad arguments");
  MlpArgs a = mlp_bwd_args(dout, wimg, M, hw);
  a.tin = (const bf16_t*)h;
  return mlp_bwd_dh_run<4>("vsx_mlp_bwd_dh", a, s, t, dh, ws, ws_rows, colsum, 4 * C, gtab, M, C, hw, stream);
}

/* MODE 5: vsx_mlp_bwd_dh WITHOUT a stored pre-activation: h = bf16(xh . W1'^T + b1) is recomputed on chip from the normalised
 * rows xh [M, C] (wimg_fwd = the forward image vsx_mlp_pack(W1', W2), b1 = the folded fc1 bias — the operands of vsx_mlp_fc1, so
 * the recomputed h is bit-identical to the one MODE 2 would have stored); everything else as vsx_mlp_bwd_dh.  Block math:
 * viscy_models/unet/fcmae.py:174-221 (backward of GRN-MLP as timm's GlobalResponseNormMlp computes it). */
extern "C" int32_t vsx_mlp_bwd_dh_re(const void* dout, const void* xh, const void* wimg_bwd, const void* wimg_fwd, const float* b1,
                                     const float* s, const float* t, void* dh, float* ws, int64_t ws_rows, float* colsum,
                                     const float* gtab, int64_t M, int32_t C, int32_t hw, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_bwd_dh_re: bf16 only");
  VSX_CHECK(dout && xh && wimg_bwd && wimg_fwd && b1 && s && t && dh && ws && colsum && gtab && M > 0 && hw > 0, "vsx_mlp_bwd_dh_re: bad arguments");
  MlpArgs a = mlp_bwd_args(dout, wimg_bwd, M, hw);
  a.xh2 = (const bf16_t*)xh; a.wimg2 = (const char*)wimg_fwd; a.b1 = b1;
  return mlp_bwd_dh_run<5>("vsx_mlp_bwd_dh_re", a, s, t, dh, ws, ws_rows, colsum, 4 * C, gtab, M, C, hw, stream);
}

/* MODE 7: vsx_mlp_bwd_dh_re for a block whose forward stored NO normalised rows (vsx_mlp_fc1_ln with xh_out = NULL): `y` [M, C]
 * is the LayerNorm input (the depthwise convolution's output), mean / rstd [M] its row statistics; x^ = bf16((y - mean) * rstd)
 * is re-formed on chip exactly as the forward formed it.  What leaves is dh' = dh * rstd (row-scaled), which is what the two
 * consumers want when they, too, read y instead of x^:
 *   fc1 weight gradient   dW1f = dh^T . x^ = dh'^T . y - u (x) 1,   u[j] = sum_r dh'[r, j] * mean[r]   (a plain TN GEMM on y)
 *   LayerNorm backward    dy = dx' - mean_c(dx') - x^ * mean_c(dx' * x^),  dx' = dh' . W1' (the trailing * rstd is already in)
 * colsum2 [2, 4C] += { sum_r dh[r, j] (the fc1 bias gradient, formed as sum dh' / rstd), u[j] }; ws: [M / rows-per-workgroup,
 * 2 * 4C] floats.  Block math: viscy_models/unet/fcmae.py:174-221; LayerNorm = timm ConvNeXtBlock.norm (unext2.py:79). */
extern "C" int32_t vsx_mlp_bwd_dh_ln(const void* dout, const void* y, const float* mean, const float* rstd, const void* wimg_bwd,
                                     const void* wimg_fwd, const float* b1, const float* s, const float* t, void* dh, float* ws,
                                     int64_t ws_rows, float* colsum2, const float* gtab, int64_t M, int32_t C, int32_t hw,
                                     int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dtype == VSX_BF16, "vsx_mlp_bwd_dh_ln: bf16 only");
  VSX_CHECK(dout && y && mean && rstd && wimg_bwd && wimg_fwd && b1 && s && t && dh && ws && colsum2 && gtab && M > 0 && hw > 0,
            "vsx_mlp_bwd_dh_ln: bad arguments");
  MlpArgs a = mlp_bwd_args(dout, wimg_bwd, M, hw);
  a.xh2 = (const bf16_t*)y; a.wimg2 = (const char*)wimg_fwd; a.b1 = b1; a.ln_mean = mean; a.ln_rstd = rstd;
  return mlp_bwd_dh_run<7>("vsx_mlp_bwd_dh_ln", a, s, t, dh, ws, ws_rows, colsum2, 8 * C, gtab, M, C, hw, stream);
}

#ifdef MLP_TS
extern "C" int32_t vsx_debug_mlp_ts(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_mlp_ts), sizeof(g_mlp_ts)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" int64_t vsx_mlp_det_floats(int32_t C, int32_t hw, int64_t M, int32_t mode) {
  const MlpCfg* c = mode == 0 || mode == 2 || mode == 6 ? mlp_cfg(C, hw, M, mode) : nullptr;
  return c ? mlp_det_need(c, M) : 0;
}

extern "C" int32_t vsx_mlp_rows_per_workgroup(int32_t C, int32_t hw, int64_t M) {
  const MlpCfg* c = mlp_cfg(C, hw, M, 4);
  return c ? c->NW * 16 * c->MF : 0;
}
