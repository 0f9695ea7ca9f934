// viscy_amd — narrow-channel kernel family (gfx950): the launches of the 2x2-stem FCMAE (VSCyto2D) that the wide kernels
// were not built for.
//
//   * stem with a patch of K = Cin*kz*ky*kx values that is not a whole number of 16-byte bf16 vectors (2x2 stem: K = 4 or 20):
//     forward straight from the fp32 input stack (no patch matrix), weight / bias gradient with the patch recomputed from x;
//   * entry projection of the last decoder stage into C in {4, 8} channels: LayerNorm2d(affine) + 1x1 convolution in one pass
//     over the concatenated map, and its data / weight gradient;
//   * ConvNeXt-V2 block at C in {4, 8} (hidden 4C <= 32): one thread per pixel, the 4C-wide hidden never leaves registers;
//     forward = (1) depthwise 7x7 + LayerNorm + fc1 + GELU + per-sample GRN sums, (2) the same recomputed from the stored
//     depthwise output + GRN + fc2 + bias + residual; backward = (A) fc2 / GRN statistics, (B) GELU' + fc1 + LayerNorm
//     backward -> dy, (C) depthwise data gradient + residual and the 7x7 weight / bias gradient;
//   * the PixelToVoxelShuffleHead adjoint with fewer channels than a 16-byte vector (Cout*D*s*s = 4 in bf16).
//
// Every reduction (GRN sums, weight / bias gradients, GRN statistics) writes one fp32 partial per workgroup into caller-owned
// scratch and is summed in a fixed order (vsx_det_group_sum): the results are the same bits from run to run, whatever
// `det_reduce` says.  Partials are at most (49 + 1) * C or C * 4C + 9C floats per workgroup: atomics would buy nothing.
// Plain C++ / vector stores only.
#include "vsx_common.h"
#include "../../include/vsx.h"

namespace {

constexpr int NB = 256;       // threads per workgroup of every kernel here
constexpr int NWG_MAX = 2048; // target workgroups of the per-pixel passes (whole tiles of 256 pixels, one sample each)

// ---- C-wide channels-last rows (C = 4 or 8): 8 .. 32 contiguous bytes, loaded / stored as whole vectors
template <int C>
__device__ __forceinline__ void ld_row(const float* p, float* f) {
#pragma unroll
  for (int i = 0; i < C; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    f[i] = v.x; f[i + 1] = v.y; f[i + 2] = v.z; f[i + 3] = v.w;
  }
}
template <int C>
__device__ __forceinline__ void ld_row(const bf16_t* p, float* f) {
  if constexpr (C == 8) {
    unpack<bf16_t>(*reinterpret_cast<const uint4*>(p), f);
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  }
}
template <int C>
__device__ __forceinline__ void st_row(float* p, const float* f) {
#pragma unroll
  for (int i = 0; i < C; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
}
template <int C>
__device__ __forceinline__ void st_row(bf16_t* p, const float* f) {
  if constexpr (C == 8) {
    *reinterpret_cast<uint4*>(p) = pack<bf16_t>(f);
  } else {
    *reinterpret_cast<uint2*>(p) = make_uint2(f32x2_to_bf16x2_bits(f[0], f[1]), f32x2_to_bf16x2_bits(f[2], f[3]));
  }
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// sum over the workgroup of N per-thread values, in a fixed order (wave butterflies, then the four waves in slot order);
// `red` is LDS of at least 4 * N floats; dst[n] is written by one thread.  Every thread of the workgroup must call it.
template <int N>
__device__ __forceinline__ void wg_sum_store(const float* acc, float* red, float* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float v = wave_sum(acc[n]);
    if (lane == 0) red[wv * N + n] = v;
  }
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += NB) dst[n] = (red[n] + red[N + n]) + (red[2 * N + n] + red[3 * N + n]);
  __syncthreads();
}

// ------------------------------------------------------------------ stem
// out[r, c] = bias[c] + sum_k W[c, k] * patch_r[k],  patch k = ((ci * kz + dz) * ky + dy) * kx + dx  (Conv3d / Conv2d weight order)
template <typename T>
__global__ __launch_bounds__(NB) void narrow_stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                             const float* __restrict__ bias, T* __restrict__ out, int B, int Cin,
                                                             int kz, int H, int Wd, int ky, int kx, int C0) {
  extern __shared__ float wl[];  // [K][C0] then bias[C0]
  constexpr int VN = VT<T>::N;
  const int K = Cin * kz * ky * kx;
  for (int e = threadIdx.x; e < K * C0; e += NB) wl[e] = W[(size_t)(e % C0) * K + e / C0];
  for (int e = threadIdx.x; e < C0; e += NB) wl[K * C0 + e] = bias[e];
  __syncthreads();
  const int h = H / ky, w = Wd / kx, nch = C0 / VN;
  const long total = (long)B * h * w * nch;
  const long plane = (long)H * Wd;
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < total; i += (long)gridDim.x * NB) {
    const int ch = (int)(i % nch);
    const long r = i / nch;
    const int xx = (int)(r % w);
    const int yy = (int)((r / w) % h);
    const int b = (int)(r / ((long)w * h));
    float acc[VN];
#pragma unroll
    for (int j = 0; j < VN; ++j) acc[j] = wl[K * C0 + ch * VN + j];
    int k = 0;
    for (int ci = 0; ci < Cin; ++ci)
      for (int dz = 0; dz < kz; ++dz) {
        const float* src = x + ((size_t)b * Cin + ci) * kz * plane + (size_t)dz * plane;
        for (int dy = 0; dy < ky; ++dy)
          for (int dx = 0; dx < kx; ++dx, ++k) {
            const float v = src[(size_t)(yy * ky + dy) * Wd + xx * kx + dx];
            const float* wk = wl + k * C0 + ch * VN;
#pragma unroll
            for (int j = 0; j < VN; ++j) acc[j] = fmaf(v, wk[j], acc[j]);
          }
      }
    stvec<T>(out + (size_t)r * C0 + ch * VN, pack<T>(acc));
  }
}

// per-workgroup partials ws[wg][C0*K + C0] of dW[c, k] = sum_r df[r, c] * patch_r[k] and db[c] = sum_r df[r, c]
constexpr int STEM_ROWS = 64;
constexpr int STEM_EPT = 16;  // entries per thread: C0 * (K + 1) <= 4096
template <typename T>
__global__ __launch_bounds__(NB) void narrow_stem_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ df,
                                                               float* __restrict__ ws, int B, int Cin, int kz, int H, int Wd, int ky,
                                                               int kx, int C0, long rows_per_wg) {
  __shared__ float dfs[STEM_ROWS * 128];
  __shared__ float ps[STEM_ROWS * 64];
  const int K = Cin * kz * ky * kx, NE = C0 * K + C0;
  const int h = H / ky, w = Wd / kx;
  const long M0 = (long)B * h * w, plane = (long)H * Wd;
  const long r_lo = (long)blockIdx.x * rows_per_wg;
  const long r_hi = r_lo + rows_per_wg < M0 ? r_lo + rows_per_wg : M0;
  float acc[STEM_EPT];
#pragma unroll
  for (int q = 0; q < STEM_EPT; ++q) acc[q] = 0.f;
  for (long r0 = r_lo; r0 < r_hi; r0 += STEM_ROWS) {
    for (int e = threadIdx.x; e < STEM_ROWS * C0; e += NB) {
      const long r = r0 + e / C0;
      dfs[e] = r < r_hi ? to_f32<T>(df[(size_t)r * C0 + e % C0]) : 0.f;
    }
    for (int e = threadIdx.x; e < STEM_ROWS * K; e += NB) {
      const long r = r0 + e / K;
      float v = 0.f;
      if (r < r_hi) {
        const int k = e % K;
        const int dx = k % kx, dy = (k / kx) % ky, dz = (k / (kx * ky)) % kz, ci = k / (kx * ky * kz);
        const int xx = (int)(r % w), yy = (int)((r / w) % h), b = (int)(r / ((long)w * h));
        v = x[((size_t)b * Cin + ci) * kz * plane + (size_t)dz * plane + (size_t)(yy * ky + dy) * Wd + xx * kx + dx];
      }
      ps[e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < STEM_EPT; ++q) {
      const int en = threadIdx.x + q * NB;
      if (en < NE) {
        const bool isb = en >= C0 * K;
        const int c = isb ? en - C0 * K : en / K, k = isb ? 0 : en % K;
        float a = acc[q];
        for (int r = 0; r < STEM_ROWS; ++r) a = fmaf(dfs[r * C0 + c], isb ? 1.f : ps[r * K + k], a);
        acc[q] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < STEM_EPT; ++q) {
    const int en = threadIdx.x + q * NB;
    if (en < NE) ws[(size_t)blockIdx.x * NE + en] = acc[q];
  }
}

// ------------------------------------------------------------------ entry projection of a narrow decoder stage
// 16 lanes per row, lane l holds channels l, l + 16, ... (< Ccat <= 16 * PJ_V); 16 rows per workgroup step
constexpr int PJ_V = 12;
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_proj_fwd_kernel(const T* __restrict__ cat, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ Wp,
                                                             const float* __restrict__ bp, T* __restrict__ out, float* __restrict__ mean,
                                                             float* __restrict__ rstd, long M, int Ccat, float eps) {
  __shared__ float wl[C * 16 * PJ_V], gl[16 * PJ_V], bl[16 * PJ_V];
  for (int e = threadIdx.x; e < C * Ccat; e += NB) wl[e] = Wp[e];
  for (int e = threadIdx.x; e < Ccat; e += NB) { gl[e] = gamma[e]; bl[e] = beta[e]; }
  __syncthreads();
  const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const float inv = 1.f / (float)Ccat;
  for (long base = (long)blockIdx.x * 16; base < M; base += (long)gridDim.x * 16) {
    const long row = base + grp;
    const bool ok = row < M;
    float v[PJ_V];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PJ_V; ++j) {
      const int k = l + 16 * j;
      v[j] = (ok && k < Ccat) ? to_f32<T>(cat[(size_t)row * Ccat + k]) : 0.f;
      s += v[j];
    }
    const float mu = group_sum<16>(s) * inv;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < PJ_V; ++j) {
      const float d = (l + 16 * j < Ccat) ? v[j] - mu : 0.f;
      q = fmaf(d, d, q);
    }
    const float rs = rsqrtf(group_sum<16>(q) * inv + eps);
    float o[C];
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = 0.f;
#pragma unroll
    for (int j = 0; j < PJ_V; ++j) {
      const int k = l + 16 * j;
      if (k < Ccat) {
        const float xn = fmaf((v[j] - mu) * rs, gl[k], bl[k]);
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = fmaf(wl[c * Ccat + k], xn, o[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = group_sum<16>(o[c]);
    if (ok && l == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] += bp[c];
      st_row<C>(out + (size_t)row * C, o);
      if (mean) mean[row] = mu;
      rstd[row] = rs;
    }
  }
}

// dxn[r, k] = sum_c d[r, c] W[c, k];  partials ws[wg][C*Ccat + C] of dW[c, k] = sum_r d[r, c] xn[r, k], db[c] = sum_r d[r, c]
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_proj_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ cat,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ Wp, T* __restrict__ dxn, float* __restrict__ ws,
                                                             long M, int Ccat) {
  __shared__ float wl[C * 16 * PJ_V], gl[16 * PJ_V], bl[16 * PJ_V];
  __shared__ float red[C * 16 * PJ_V + C];
  const int NE = C * Ccat + C;
  for (int e = threadIdx.x; e < C * Ccat; e += NB) wl[e] = Wp[e];
  for (int e = threadIdx.x; e < Ccat; e += NB) { gl[e] = gamma[e]; bl[e] = beta[e]; }
  for (int e = threadIdx.x; e < NE; e += NB) red[e] = 0.f;
  __syncthreads();
  const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
  float acc[C][PJ_V], accb[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    accb[c] = 0.f;
#pragma unroll
    for (int j = 0; j < PJ_V; ++j) acc[c][j] = 0.f;
  }
  for (long row = (long)blockIdx.x * 16 + grp; row < M; row += (long)gridDim.x * 16) {
    float d[C];
    ld_row<C>(dout + (size_t)row * C, d);
    const float mu = mean[row], rs = rstd[row];
#pragma unroll
    for (int j = 0; j < PJ_V; ++j) {
      const int k = l + 16 * j;
      if (k < Ccat) {
        const float xn = fmaf((to_f32<T>(cat[(size_t)row * Ccat + k]) - mu) * rs, gl[k], bl[k]);
        float g = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          g = fmaf(d[c], wl[c * Ccat + k], g);
          acc[c][j] = fmaf(d[c], xn, acc[c][j]);
        }
        dxn[(size_t)row * Ccat + k] = from_f32<T>(g);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) accb[c] += d[c];
  }
  // the 16 row groups add into LDS one after another (fixed order; each (c, k) has one owner lane per group)
  for (int gi = 0; gi < 16; ++gi) {
    if (grp == gi) {
#pragma unroll
      for (int j = 0; j < PJ_V; ++j) {
        const int k = l + 16 * j;
        if (k < Ccat) {
#pragma unroll
          for (int c = 0; c < C; ++c) red[c * Ccat + k] += acc[c][j];
        }
      }
      if (l == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) red[C * Ccat + c] += accb[c];
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < NE; e += NB) ws[(size_t)blockIdx.x * NE + e] = red[e];
}

// ------------------------------------------------------------------ ConvNeXt-V2 block at C = 4 / 8
// workgroup (g, b): tiles [g * tpw, (g + 1) * tpw) of 256 pixels of sample b
template <int C>
struct BlkW {  // fp32 copies of the block operands in LDS (every thread reads the same address: broadcasts)
  float w1[4 * C][C], b1[4 * C], w2[C][4 * C], b2[C], s[4 * C], gb[4 * C], t[4 * C];
};
template <typename T, int C>
__device__ __forceinline__ void load_blk(BlkW<C>& L, const T* W1f, const float* b1f, const T* W2, const float* b2, const float* s,
                                         const float* gb, const float* t, int b) {
  constexpr int HD = 4 * C;
  for (int e = threadIdx.x; e < HD * C; e += NB) {
    L.w1[e / C][e % C] = to_f32<T>(W1f[e]);
    L.w2[e / HD][e % HD] = W2 ? to_f32<T>(W2[e]) : 0.f;
  }
  for (int e = threadIdx.x; e < HD; e += NB) {
    L.b1[e] = b1f[e];
    L.s[e] = s ? s[(size_t)b * HD + e] : 0.f;
    L.gb[e] = gb ? gb[e] : 0.f;
    L.t[e] = t ? t[(size_t)b * HD + e] : 0.f;
  }
  for (int e = threadIdx.x; e < C; e += NB) L.b2[e] = b2 ? b2[e] : 0.f;
}
// LayerNorm (no affine: folded into fc1) and fc1 of one pixel: xh[C], h[4C]; returns rstd
template <int C>
__device__ __forceinline__ float ln_fc1(const BlkW<C>& L, const float* y, float* xh, float* h) {
  float mu = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) mu += y[c];
  mu *= 1.f / C;
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) var = fmaf(y[c] - mu, y[c] - mu, var);
  const float rs = rsqrtf(var * (1.f / C) + 1e-6f);
#pragma unroll
  for (int c = 0; c < C; ++c) xh[c] = (y[c] - mu) * rs;
#pragma unroll
  for (int j = 0; j < 4 * C; ++j) {
    float a = L.b1[j];
#pragma unroll
    for (int c = 0; c < C; ++c) a = fmaf(L.w1[j][c], xh[c], a);
    h[j] = a;
  }
  return rs;
}

// pass 1: y = dwconv7(x) + bias (stored), g = gelu(fc1(LN(y))); partial ws[b][g][4C] of sum g^2
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_block_fwd1_kernel(const T* __restrict__ x, const float* __restrict__ dw_w,
                                                               const float* __restrict__ dw_b, const T* __restrict__ W1f,
                                                               const float* __restrict__ b1f, T* __restrict__ y, float* __restrict__ ws,
                                                               int H, int Wd, int tpw) {
  constexpr int HD = 4 * C;
  __shared__ BlkW<C> L;
  __shared__ float dwl[49 * C + C];
  __shared__ float red[4 * HD];
  const int b = blockIdx.y;
  load_blk<T, C>(L, W1f, b1f, nullptr, nullptr, nullptr, nullptr, nullptr, b);
  for (int e = threadIdx.x; e < 49 * C; e += NB) dwl[e] = dw_w[e];
  for (int e = threadIdx.x; e < C; e += NB) dwl[49 * C + e] = dw_b[e];
  __syncthreads();
  const long hw = (long)H * Wd;
  const int nt = (int)((hw + NB - 1) / NB);
  const int t_lo = blockIdx.x * tpw, t_hi = t_lo + tpw < nt ? t_lo + tpw : nt;
  const T* xb = x + (size_t)b * hw * C;
  float acc[HD];
#pragma unroll
  for (int j = 0; j < HD; ++j) acc[j] = 0.f;
  for (int tile = t_lo; tile < t_hi; ++tile) {
    __asm__ volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (hoisted, they spill to scratch)
    const long p = (long)tile * NB + threadIdx.x;
    if (p >= hw) continue;
    const int py = (int)(p / Wd), px = (int)(p % Wd);
    float yv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) yv[c] = dwl[49 * C + c];
    for (int ky = 0; ky < 7; ++ky) {
      const int yy = py + ky - 3;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const int xx = px + kx - 3;
        if (xx < 0 || xx >= Wd) continue;
        float xv[C];
        ld_row<C>(xb + ((size_t)yy * Wd + xx) * C, xv);
#pragma unroll
        for (int c = 0; c < C; ++c) yv[c] = fmaf(xv[c], dwl[(ky * 7 + kx) * C + c], yv[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) yv[c] = round_to<T>(yv[c]);  // pass 2 and the backward see the stored values
    st_row<C>(y + ((size_t)b * hw + p) * C, yv);
    float xh[C], h[HD];
    ln_fc1<C>(L, yv, xh, h);
#pragma unroll
    for (int j = 0; j < HD; ++j) {
      const float g = gelu_erf(h[j]);
      acc[j] = fmaf(g, g, acc[j]);
    }
  }
  wg_sum_store<HD>(acc, red, ws + ((size_t)b * gridDim.x + blockIdx.x) * HD);
}

// pass 2: out = fc2(gelu(fc1(LN(y))) * s_b + grn_beta) + b2 + x
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_block_fwd2_kernel(const T* __restrict__ y, const T* __restrict__ x, const T* __restrict__ W1f,
                                                               const float* __restrict__ b1f, const float* __restrict__ s,
                                                               const float* __restrict__ gb, const T* __restrict__ W2,
                                                               const float* __restrict__ b2, T* __restrict__ out, int H, int Wd, int tpw) {
  constexpr int HD = 4 * C;
  __shared__ BlkW<C> L;
  const int b = blockIdx.y;
  load_blk<T, C>(L, W1f, b1f, W2, b2, s, gb, nullptr, b);
  __syncthreads();
  const long hw = (long)H * Wd;
  const int nt = (int)((hw + NB - 1) / NB);
  const int t_lo = blockIdx.x * tpw, t_hi = t_lo + tpw < nt ? t_lo + tpw : nt;
  for (int tile = t_lo; tile < t_hi; ++tile) {
    __asm__ volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (hoisted, they spill to scratch)
    const long p = (long)tile * NB + threadIdx.x;
    if (p >= hw) continue;
    const size_t r = (size_t)b * hw + p;
    float yv[C], xh[C], h[HD], o[C];
    ld_row<C>(y + r * C, yv);
    ln_fc1<C>(L, yv, xh, h);
    ld_row<C>(x + r * C, o);
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] += L.b2[c];
#pragma unroll
    for (int j = 0; j < HD; ++j) {
      const float z = fmaf(gelu_erf(h[j]), L.s[j], L.gb[j]);
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = fmaf(L.w2[c][j], z, o[c]);
    }
    st_row<C>(out + r * C, o);
  }
}

// backward A: dz = dout W2; partials ws[b][g][C*4C | C | 4C | 4C] of dW2 = sum dout^T z, db2 = sum dout, P = sum dz g, S = sum dz
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_block_bwd_a_kernel(const T* __restrict__ dout, const T* __restrict__ y, const T* __restrict__ W1f,
                                                                const float* __restrict__ b1f, const float* __restrict__ s,
                                                                const float* __restrict__ gb, const T* __restrict__ W2,
                                                                float* __restrict__ ws, int H, int Wd, int tpw) {
  constexpr int HD = 4 * C, NE = C * HD + C + 2 * HD;
  __shared__ BlkW<C> L;
  __shared__ float zs[NB][HD + 1];
  __shared__ float ds[NB][C + 1];
  __shared__ float red[4 * 2 * HD];
  const int b = blockIdx.y;
  load_blk<T, C>(L, W1f, b1f, W2, nullptr, s, gb, nullptr, b);
  __syncthreads();
  const long hw = (long)H * Wd;
  const int nt = (int)((hw + NB - 1) / NB);
  const int t_lo = blockIdx.x * tpw, t_hi = t_lo + tpw < nt ? t_lo + tpw : nt;
  float ps[2 * HD];  // P (0 .. HD-1), S (HD .. 2HD-1) of this thread's pixels
#pragma unroll
  for (int j = 0; j < 2 * HD; ++j) ps[j] = 0.f;
  float ew[(C * HD + C + NB - 1) / NB];  // this thread's dW2 / db2 entries
#pragma unroll
  for (int q = 0; q < (C * HD + C + NB - 1) / NB; ++q) ew[q] = 0.f;
  float* wsb = ws + ((size_t)b * gridDim.x + blockIdx.x) * NE;
  for (int tile = t_lo; tile < t_hi; ++tile) {
    __asm__ volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (hoisted, they spill to scratch)
    const long p = (long)tile * NB + threadIdx.x;
    if (p < hw) {
      const size_t r = (size_t)b * hw + p;
      float yv[C], xh[C], h[HD], d[C];
      ld_row<C>(y + r * C, yv);
      ld_row<C>(dout + r * C, d);
      ln_fc1<C>(L, yv, xh, h);
#pragma unroll
      for (int j = 0; j < HD; ++j) {
        const float g = gelu_erf(h[j]);
        float dz = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dz = fmaf(d[c], L.w2[c][j], dz);
        ps[j] = fmaf(dz, g, ps[j]);
        ps[HD + j] += dz;
        zs[threadIdx.x][j] = fmaf(g, L.s[j], L.gb[j]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) ds[threadIdx.x][c] = d[c];
    } else {
#pragma unroll
      for (int j = 0; j < HD; ++j) zs[threadIdx.x][j] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) ds[threadIdx.x][c] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (C * HD + C + NB - 1) / NB; ++q) {
      const int en = threadIdx.x + q * NB;
      if (en < C * HD) {
        const int c = en / HD, j = en % HD;
        float a = ew[q];
        for (int i = 0; i < NB; ++i) a = fmaf(ds[i][c], zs[i][j], a);
        ew[q] = a;
      } else if (en < C * HD + C) {
        const int c = en - C * HD;
        float a = ew[q];
        for (int i = 0; i < NB; ++i) a += ds[i][c];
        ew[q] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < (C * HD + C + NB - 1) / NB; ++q) {
    const int en = threadIdx.x + q * NB;
    if (en < C * HD + C) wsb[en] = ew[q];
  }
  wg_sum_store<2 * HD>(ps, red, wsb + C * HD + C);
}

// backward B: dh = (dz s + t g) gelu'(h), dy = LN_bwd(dh W1f) (stored); partials ws[b][g][4C*C | 4C] of dW1f = sum dh^T xh, db1f = sum dh
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_block_bwd_b_kernel(const T* __restrict__ dout, const T* __restrict__ y, const T* __restrict__ W1f,
                                                                const float* __restrict__ b1f, const float* __restrict__ s,
                                                                const float* __restrict__ t, const T* __restrict__ W2, T* __restrict__ dy,
                                                                float* __restrict__ ws, int H, int Wd, int tpw) {
  constexpr int HD = 4 * C, NE = HD * C + HD, NQ = (HD * C + NB - 1) / NB;
  __shared__ BlkW<C> L;
  __shared__ float hs[NB][HD + 1];
  __shared__ float xs[NB][C + 1];
  __shared__ float red[4 * HD];
  const int b = blockIdx.y;
  load_blk<T, C>(L, W1f, b1f, W2, nullptr, s, nullptr, t, b);
  __syncthreads();
  const long hw = (long)H * Wd;
  const int nt = (int)((hw + NB - 1) / NB);
  const int t_lo = blockIdx.x * tpw, t_hi = t_lo + tpw < nt ? t_lo + tpw : nt;
  float db[HD];
#pragma unroll
  for (int j = 0; j < HD; ++j) db[j] = 0.f;
  float ew[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) ew[q] = 0.f;
  float* wsb = ws + ((size_t)b * gridDim.x + blockIdx.x) * NE;
  for (int tile = t_lo; tile < t_hi; ++tile) {
    __asm__ volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (hoisted, they spill to scratch)
    const long p = (long)tile * NB + threadIdx.x;
    if (p < hw) {
      const size_t r = (size_t)b * hw + p;
      float yv[C], xh[C], h[HD], d[C], dxh[C];
      ld_row<C>(y + r * C, yv);
      ld_row<C>(dout + r * C, d);
      const float rs = ln_fc1<C>(L, yv, xh, h);
#pragma unroll
      for (int c = 0; c < C; ++c) dxh[c] = 0.f;
#pragma unroll
      for (int j = 0; j < HD; ++j) {
        float dz = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dz = fmaf(d[c], L.w2[c][j], dz);
        const float dh = fmaf(dz, L.s[j], L.t[j] * gelu_erf(h[j])) * gelu_erf_grad(h[j]);
        db[j] += dh;
        hs[threadIdx.x][j] = dh;
#pragma unroll
        for (int c = 0; c < C; ++c) dxh[c] = fmaf(dh, L.w1[j][c], dxh[c]);
      }
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        m1 += dxh[c];
        m2 = fmaf(dxh[c], xh[c], m2);
        xs[threadIdx.x][c] = xh[c];
      }
      m1 *= 1.f / C;
      m2 *= 1.f / C;
      float o[C];
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = rs * (dxh[c] - m1 - xh[c] * m2);
      st_row<C>(dy + r * C, o);
    } else {
#pragma unroll
      for (int j = 0; j < HD; ++j) hs[threadIdx.x][j] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) xs[threadIdx.x][c] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int en = threadIdx.x + q * NB;
      if (en < HD * C) {
        const int j = en / C, c = en % C;
        float a = ew[q];
        for (int i = 0; i < NB; ++i) a = fmaf(hs[i][j], xs[i][c], a);
        ew[q] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int en = threadIdx.x + q * NB;
    if (en < HD * C) wsb[en] = ew[q];
  }
  wg_sum_store<HD>(db, red, wsb + HD * C);
}

// backward C: dx = dwconv7^T(dy) + dout (shortcut); partials ws[b][g][49*C | C] of ddw[t, c] = sum dy[p, c] x[p + off_t, c], ddb = sum dy
template <typename T, int C>
__global__ __launch_bounds__(NB) void narrow_block_bwd_c_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ dout,
                                                                const float* __restrict__ dw_w, T* __restrict__ dx, float* __restrict__ ws,
                                                                int H, int Wd, int tpw) {
  constexpr int NE = 49 * C + C, NQ = (49 * C + NB - 1) / NB;
  __shared__ float dwl[49 * C];
  __shared__ float ds[NB][C + 1];
  __shared__ float red[4 * C];
  const int b = blockIdx.y;
  for (int e = threadIdx.x; e < 49 * C; e += NB) dwl[e] = dw_w[e];
  __syncthreads();
  const long hw = (long)H * Wd;
  const int nt = (int)((hw + NB - 1) / NB);
  const int t_lo = blockIdx.x * tpw, t_hi = t_lo + tpw < nt ? t_lo + tpw : nt;
  const T* dyb = dy + (size_t)b * hw * C;
  const T* xb = x + (size_t)b * hw * C;
  float dbv[C];
#pragma unroll
  for (int c = 0; c < C; ++c) dbv[c] = 0.f;
  float ew[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) ew[q] = 0.f;
  float* wsb = ws + ((size_t)b * gridDim.x + blockIdx.x) * NE;
  for (int tile = t_lo; tile < t_hi; ++tile) {
    __asm__ volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (hoisted, they spill to scratch)
    const long p = (long)tile * NB + threadIdx.x;
    if (p < hw) {
      const int py = (int)(p / Wd), px = (int)(p % Wd);
      float o[C], dv[C];
      ld_row<C>(dout + ((size_t)b * hw + p) * C, o);
      for (int ky = 0; ky < 7; ++ky) {
        const int yy = py - ky + 3;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int xx = px - kx + 3;
          if (xx < 0 || xx >= Wd) continue;
          float v[C];
          ld_row<C>(dyb + ((size_t)yy * Wd + xx) * C, v);
#pragma unroll
          for (int c = 0; c < C; ++c) o[c] = fmaf(v[c], dwl[(ky * 7 + kx) * C + c], o[c]);
        }
      }
      st_row<C>(dx + ((size_t)b * hw + p) * C, o);
      ld_row<C>(dyb + (size_t)p * C, dv);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        ds[threadIdx.x][c] = dv[c];
        dbv[c] += dv[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) ds[threadIdx.x][c] = 0.f;
    }
    __syncthreads();
    const long p0 = (long)tile * NB;
    const int cnt = hw - p0 < NB ? (int)(hw - p0) : NB;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int en = threadIdx.x + q * NB;
      if (en < 49 * C) {
        const int tap = en / C, c = en % C;
        const int oy = tap / 7 - 3, ox = tap % 7 - 3;
        float a = ew[q];
        int py = (int)(p0 / Wd), px = (int)(p0 % Wd);
        for (int i = 0; i < cnt; ++i) {
          const int yy = py + oy, xx = px + ox;
          if (yy >= 0 && yy < H && xx >= 0 && xx < Wd) a = fmaf(ds[i][c], to_f32<T>(xb[((size_t)yy * Wd + xx) * C + c]), a);
          if (++px == Wd) { px = 0; ++py; }
        }
        ew[q] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int en = threadIdx.x + q * NB;
    if (en < 49 * C) wsb[en] = ew[q];
  }
  wg_sum_store<C>(dbv, red, wsb + 49 * C);
}

// ------------------------------------------------------------------ PixelToVoxelShuffleHead adjoint, one element per thread
template <typename T>
__global__ __launch_bounds__(NB) void narrow_voxel_shuffle_bwd_kernel(const float* __restrict__ dout, T* __restrict__ dfeat, int B, int h,
                                                                       int w, int Cout, int D, int s, int pool) {
  const int H = h * s, W = w * s;
  const int Cd = Cout * D * s * s;
  const long total = (long)B * h * w * Cd;
  const float inv = pool ? 1.f / (float)(s * s) : 1.f;
  const int nt = pool ? s : 1;
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < total; i += (long)gridDim.x * NB) {
    const int c = (int)(i % Cd);
    const long pix = i / Cd;
    const int x = (int)(pix % w);
    const long r = pix / w;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int dx = c % s, dy = (c / s) % s, cz = c / (s * s);
    const float* plane = dout + ((size_t)b * Cout * D + cz) * H * W;
    const int Y = y * s + dy, X = x * s + dx;
    float acc = 0.f;
    for (int ty = 0; ty < nt && Y + ty < H; ++ty)
      for (int tx = 0; tx < nt && X + tx < W; ++tx) acc += plane[(size_t)(Y + ty) * W + X + tx];
    dfeat[i] = from_f32<T>(acc * inv);
  }
}

// workgroups per sample and tiles per workgroup of the per-pixel passes
void blk_grid(int B, long hw, int& gps, int& tpw) {
  const int nt = (int)((hw + NB - 1) / NB);
  int want = vsx_cdiv(NWG_MAX, B);
  if (want < 1) want = 1;
  if (want > nt) want = nt;
  tpw = vsx_cdiv(nt, want);
  gps = vsx_cdiv(nt, tpw);
}
long stem_rows_per_wg(long M0) {
  long r = (M0 + 1023) / 1024;
  return (r + STEM_ROWS - 1) / STEM_ROWS * STEM_ROWS;
}
int proj_wgs(long M) {
  const long g = (M + 15) / 16;
  return (int)(g < 1024 ? g : 1024);
}
bool al16(const void* p) { return vsx_al16(p); }

}  // namespace

// ================================================================== C-ABI
extern "C" int64_t vsx_narrow_ws_floats(int32_t op, int32_t B, int64_t n, int32_t C, int32_t K) {
  if (B <= 0 || n <= 0 || C <= 0) return -1;
  switch (op) {
    case VSX_NARROW_STEM: { const long rpw = stem_rows_per_wg(n); return (int64_t)((n + rpw - 1) / rpw) * (C * K + C); }
    case VSX_NARROW_PROJ: return (int64_t)proj_wgs(n) * (C * K + C);
    default: break;
  }
  int gps, tpw;
  blk_grid(B, n, gps, tpw);
  const long G = (long)B * gps;
  switch (op) {
    case VSX_NARROW_FWD1: return G * 4 * C;
    case VSX_NARROW_BWD_A: return G * (C * 4 * C + C + 8 * C);
    case VSX_NARROW_BWD_B: return G * (4 * C * C + 4 * C);
    case VSX_NARROW_BWD_C: return G * (49 * C + C);
    default: return -1;
  }
}

extern "C" int32_t vsx_narrow_stem_fwd(const float* x, const float* W, const float* bias, void* out, int32_t B, int32_t Cin, int32_t Z,
                                       int32_t H, int32_t Wd, int32_t kz, int32_t ky, int32_t kx, int32_t C0, int32_t dtype,
                                       vsx_stream_t stream) {
  const int K = Cin * kz * ky * kx, vn = vsx_vec_elems(dtype);
  VSX_CHECK(x && W && bias && out && B > 0 && Cin > 0 && kz > 0 && ky > 0 && kx > 0 && Z == kz && H % ky == 0 && Wd % kx == 0,
            "vsx_narrow_stem_fwd: bad arguments (Z=%d must equal kz=%d, H=%d / W=%d multiples of the kernel)", Z, kz, H, Wd);
  VSX_CHECK(C0 > 0 && C0 % vn == 0 && K * C0 + C0 <= 16384 && al16(out), "vsx_narrow_stem_fwd: C0=%d K=%d not served", C0, K);
  const long total = (long)B * (H / ky) * (Wd / kx) * (C0 / vn);
  int g = vsx_cdiv(total, NB);
  if (g > 65536) g = 65536;
  const size_t lds = (size_t)(K * C0 + C0) * sizeof(float);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(narrow_stem_fwd_kernel<T>, dim3(g), dim3(NB), lds, (hipStream_t)stream, x, W, bias, (T*)out, B, Cin, kz, H, Wd, ky, kx, C0);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_narrow_stem_wgrad(const float* x, const void* df, float* dW, float* db, float* ws, int64_t ws_floats, int32_t B,
                                         int32_t Cin, int32_t Z, int32_t H, int32_t Wd, int32_t kz, int32_t ky, int32_t kx, int32_t C0,
                                         int32_t dtype, vsx_stream_t stream) {
  const int K = Cin * kz * ky * kx;
  VSX_CHECK(x && df && dW && db && ws && B > 0 && Cin > 0 && kz > 0 && ky > 0 && kx > 0 && Z == kz && H % ky == 0 && Wd % kx == 0,
            "vsx_narrow_stem_wgrad: bad arguments");
  VSX_CHECK(C0 > 0 && C0 <= 128 && K <= 64 && C0 * (K + 1) <= STEM_EPT * NB, "vsx_narrow_stem_wgrad: C0=%d K=%d not served", C0, K);
  const long M0 = (long)B * (H / ky) * (Wd / kx);
  const long rpw = stem_rows_per_wg(M0);
  const int G = (int)((M0 + rpw - 1) / rpw);
  const int NE = C0 * K + C0;
  VSX_CHECK(ws_floats >= (int64_t)G * NE, "vsx_narrow_stem_wgrad: workspace needs %ld floats", (long)G * NE);
  hipStream_t st = (hipStream_t)stream;
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(narrow_stem_wgrad_kernel<T>, dim3(G), dim3(NB), 0, st, x, (const T*)df, ws, B, Cin, kz, H, Wd, ky, kx, C0, rpw);
  });
  VSX_LAUNCH_CHECK();
  if (vsx_det_group_sum(ws, NE, 0, dW, 1, G, C0 * K, st)) return 2;
  return vsx_det_group_sum(ws, NE, C0 * K, db, 1, G, C0, st) ? 2 : 0;
}

// dtype x C in {4, 8} (the entries check C first): f(vsx_type<T>, integral_constant<int, C>)
template <class F>
static __forceinline__ void narrow_dispatch(int dtype, int C, F&& f) {
  vsx_by_dtype(dtype, [&](auto tag) { vsx_by_int<4, 8>(C, [&](auto c) { f(tag, c); }); });
}

extern "C" int32_t vsx_narrow_proj_fwd(const void* cat, const float* gamma, const float* beta, const float* Wp, const float* bp, void* out,
                                       float* mean, float* rstd, int64_t M, int32_t Ccat, int32_t C, float eps, int32_t dtype,
                                       vsx_stream_t stream) {
  VSX_CHECK(cat && gamma && beta && Wp && bp && out && rstd && M > 0, "vsx_narrow_proj_fwd: bad arguments");
  VSX_CHECK((C == 4 || C == 8) && Ccat > 0 && Ccat <= 16 * PJ_V && al16(out), "vsx_narrow_proj_fwd: C=%d Ccat=%d not served", C, Ccat);
  hipStream_t st = (hipStream_t)stream;
  const long rows16 = (M + 15) / 16;
  const dim3 grid((int)(rows16 < 65536 ? rows16 : 65536));
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_proj_fwd_kernel<T, decltype(c)::value>), grid, dim3(NB), 0, st, (const T*)cat, gamma, beta, Wp, bp, (T*)out,
                       mean, rstd, (long)M, Ccat, eps);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_narrow_proj_bwd(const void* dout, const void* cat, const float* mean, const float* rstd, const float* gamma,
                                       const float* beta, const float* Wp, void* dxn, float* dW, float* db, float* ws, int64_t ws_floats,
                                       int64_t M, int32_t Ccat, int32_t C, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dout && cat && mean && rstd && gamma && beta && Wp && dxn && dW && db && ws && M > 0, "vsx_narrow_proj_bwd: bad arguments");
  VSX_CHECK((C == 4 || C == 8) && Ccat > 0 && Ccat <= 16 * PJ_V && al16(dout), "vsx_narrow_proj_bwd: C=%d Ccat=%d not served", C, Ccat);
  const int G = proj_wgs(M), NE = C * Ccat + C;
  VSX_CHECK(ws_floats >= (int64_t)G * NE, "vsx_narrow_proj_bwd: workspace needs %ld floats", (long)G * NE);
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_proj_bwd_kernel<T, decltype(c)::value>), dim3(G), dim3(NB), 0, st, (const T*)dout, (const T*)cat, mean,
                       rstd, gamma, beta, Wp, (T*)dxn, ws, (long)M, Ccat);
  });
  VSX_LAUNCH_CHECK();
  if (vsx_det_group_sum(ws, NE, 0, dW, 1, G, C * Ccat, st)) return 2;
  return vsx_det_group_sum(ws, NE, C * Ccat, db, 1, G, C, st) ? 2 : 0;
}

#define NARROW_BLK_CHECK(name)                                                                                              \
  VSX_CHECK((C == 4 || C == 8) && B > 0 && H > 0 && Wd > 0 && (long)B * H * Wd < (1l << 31), name ": C=%d B=%d %dx%d not served", C, B, \
            H, Wd)

extern "C" int32_t vsx_narrow_block_fwd1(const void* x, const float* dw_w, const float* dw_b, const void* W1f, const float* b1f, void* y,
                                         float* colsq, float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C,
                                         int32_t dtype, vsx_stream_t stream) {
  NARROW_BLK_CHECK("vsx_narrow_block_fwd1");
  VSX_CHECK(x && dw_w && dw_b && W1f && b1f && y && colsq && ws && al16(x) && al16(y), "vsx_narrow_block_fwd1: bad arguments");
  int gps, tpw;
  blk_grid(B, (long)H * Wd, gps, tpw);
  VSX_CHECK(ws_floats >= (int64_t)B * gps * 4 * C, "vsx_narrow_block_fwd1: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_block_fwd1_kernel<T, decltype(c)::value>), dim3(gps, B), dim3(NB), 0, st, (const T*)x, dw_w, dw_b,
                       (const T*)W1f, b1f, (T*)y, ws, H, Wd, tpw);
  });
  VSX_LAUNCH_CHECK();
  return vsx_det_group_sum(ws, 4 * C, 0, colsq, B, gps, 4 * C, st) ? 2 : 0;
}

extern "C" int32_t vsx_narrow_block_fwd2(const void* y, const void* x, const void* W1f, const float* b1f, const float* s, const float* grn_b,
                                         const void* W2, const float* b2, void* out, int32_t B, int32_t H, int32_t Wd, int32_t C,
                                         int32_t dtype, vsx_stream_t stream) {
  NARROW_BLK_CHECK("vsx_narrow_block_fwd2");
  VSX_CHECK(y && x && W1f && b1f && s && grn_b && W2 && b2 && out && al16(x) && al16(y) && al16(out), "vsx_narrow_block_fwd2: bad arguments");
  int gps, tpw;
  blk_grid(B, (long)H * Wd, gps, tpw);
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_block_fwd2_kernel<T, decltype(c)::value>), dim3(gps, B), dim3(NB), 0, st, (const T*)y, (const T*)x,
                       (const T*)W1f, b1f, s, grn_b, (const T*)W2, b2, (T*)out, H, Wd, tpw);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_narrow_block_bwd_a(const void* dout, const void* y, const void* W1f, const float* b1f, const float* s,
                                          const float* grn_b, const void* W2, float* dW2, float* db2, float* P, float* S, float* ws,
                                          int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C, int32_t dtype,
                                          vsx_stream_t stream) {
  NARROW_BLK_CHECK("vsx_narrow_block_bwd_a");
  VSX_CHECK(dout && y && W1f && b1f && s && grn_b && W2 && dW2 && db2 && P && S && ws && al16(dout) && al16(y),
            "vsx_narrow_block_bwd_a: bad arguments");
  int gps, tpw;
  blk_grid(B, (long)H * Wd, gps, tpw);
  const int HD = 4 * C, NE = C * HD + C + 2 * HD;
  VSX_CHECK(ws_floats >= (int64_t)B * gps * NE, "vsx_narrow_block_bwd_a: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_block_bwd_a_kernel<T, decltype(c)::value>), dim3(gps, B), dim3(NB), 0, st, (const T*)dout, (const T*)y,
                       (const T*)W1f, b1f, s, grn_b, (const T*)W2, ws, H, Wd, tpw);
  });
  VSX_LAUNCH_CHECK();
  if (vsx_det_group_sum(ws, NE, 0, dW2, 1, B * gps, C * HD, st) || vsx_det_group_sum(ws, NE, C * HD, db2, 1, B * gps, C, st) ||
      vsx_det_group_sum(ws, NE, C * HD + C, P, B, gps, HD, st) || vsx_det_group_sum(ws, NE, C * HD + C + HD, S, B, gps, HD, st))
    return 2;
  return 0;
}

extern "C" int32_t vsx_narrow_block_bwd_b(const void* dout, const void* y, const void* W1f, const float* b1f, const float* s, const float* t,
                                          const void* W2, void* dy, float* dW1f, float* db1f, float* ws, int64_t ws_floats, int32_t B,
                                          int32_t H, int32_t Wd, int32_t C, int32_t dtype, vsx_stream_t stream) {
  NARROW_BLK_CHECK("vsx_narrow_block_bwd_b");
  VSX_CHECK(dout && y && W1f && b1f && s && t && W2 && dy && dW1f && db1f && ws && al16(dout) && al16(y) && al16(dy),
            "vsx_narrow_block_bwd_b: bad arguments");
  int gps, tpw;
  blk_grid(B, (long)H * Wd, gps, tpw);
  const int HD = 4 * C, NE = HD * C + HD;
  VSX_CHECK(ws_floats >= (int64_t)B * gps * NE, "vsx_narrow_block_bwd_b: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_block_bwd_b_kernel<T, decltype(c)::value>), dim3(gps, B), dim3(NB), 0, st, (const T*)dout, (const T*)y,
                       (const T*)W1f, b1f, s, t, (const T*)W2, (T*)dy, ws, H, Wd, tpw);
  });
  VSX_LAUNCH_CHECK();
  if (vsx_det_group_sum(ws, NE, 0, dW1f, 1, B * gps, HD * C, st) || vsx_det_group_sum(ws, NE, HD * C, db1f, 1, B * gps, HD, st)) return 2;
  return 0;
}

extern "C" int32_t vsx_narrow_block_bwd_c(const void* dy, const void* x, const void* dout, const float* dw_w, void* dx, float* ddw,
                                          float* ddb, float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C,
                                          int32_t dtype, vsx_stream_t stream) {
  NARROW_BLK_CHECK("vsx_narrow_block_bwd_c");
  VSX_CHECK(dy && x && dout && dw_w && dx && ddw && ddb && ws && al16(dy) && al16(x) && al16(dout) && al16(dx),
            "vsx_narrow_block_bwd_c: bad arguments");
  int gps, tpw;
  blk_grid(B, (long)H * Wd, gps, tpw);
  const int NE = 49 * C + C;
  VSX_CHECK(ws_floats >= (int64_t)B * gps * NE, "vsx_narrow_block_bwd_c: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  narrow_dispatch(dtype, C, [&](auto tag, auto c) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((narrow_block_bwd_c_kernel<T, decltype(c)::value>), dim3(gps, B), dim3(NB), 0, st, (const T*)dy, (const T*)x,
                       (const T*)dout, dw_w, (T*)dx, ws, H, Wd, tpw);
  });
  VSX_LAUNCH_CHECK();
  if (vsx_det_group_sum(ws, NE, 0, ddw, 1, B * gps, 49 * C, st) || vsx_det_group_sum(ws, NE, 49 * C, ddb, 1, B * gps, C, st)) return 2;
  return 0;
}

extern "C" int32_t vsx_narrow_voxel_shuffle_bwd(const float* dout, void* dfeat, int32_t B, int32_t h, int32_t w, int32_t Cout, int32_t D,
                                                int32_t s, int32_t pool, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(dout && dfeat && B > 0 && h > 0 && w > 0 && Cout > 0 && D > 0 && s > 0, "vsx_narrow_voxel_shuffle_bwd: bad arguments");
  const long total = (long)B * h * w * Cout * D * s * s;
  int g = vsx_cdiv(total, NB);
  if (g > 65536) g = 65536;
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(narrow_voxel_shuffle_bwd_kernel<T>, dim3(g), dim3(NB), 0, (hipStream_t)stream, dout, (T*)dfeat, B, h, w, Cout, D, s,
                       pool);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}
