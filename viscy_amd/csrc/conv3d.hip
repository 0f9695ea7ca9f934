// Dense 3x3x3 convolution family (FNet3D, viscy_amd/unet3d.py): implicit-GEMM convolution / transposed convolution on the
// matrix cores, split-K weight gradients, BatchNorm3d statistics / apply + ReLU / backward, channels-last conversions.
//
// Activations are channels-last [B*D*H*W, C] with a row stride and a channel offset, so the decoder's cat([up, skip]) is one
// [M, 2C] buffer that the transposed convolution writes columns [0, C) of and the encoder block writes columns [C, 2C) of.
//
// conv3d_igemm_kernel: M = query voxels, N = output channels, K = taps * Cin.  The query grid is
//   * a plain convolution (stride 1 or 2, zero padding 1): the output grid; input voxel of tap (kz, ky, kx) = q * s + k - 1;
//   * a transposed convolution (k 3, stride 2, padding 1, output_padding 1): one of 8 output parity classes (blockIdx.z), the
//     query grid is the input grid, output voxel = 2 q + p.  Per dimension an even output takes tap 1 (input q) and an odd
//     output taps 0 (input q + 1) and 2 (input q), so no zero is multiplied.
// The B operand is a prepared weight [N][27 * Cin] (tap-major rows, conv3d_prep_weight_kernel); a tap's weight index is its
// (kz, ky, kx), so the flipped / channel-transposed copies of the data gradients use the same kernel.
// Tile 64 x 64, 4 waves of 32 x 32, v_mfma_f32_16x16x32_bf16 (bf16) or v_mfma_f32_16x16x4f32 (exact fp32 parity mode).
// The epilogue adds the bias (optionally the old value of C: data gradients that meet in the skip slice) and, when a
// BatchNorm follows, writes per-workgroup column partials of z and z^2 of the values as stored.
//
// Every reduction is per-workgroup partials + a fold in a fixed order: no atomics, bit-identical from run to run.
#include "vsx_common.h"
#include "mfma16.h"
#include "../../include/vsx.h"

namespace {

constexpr int C3_BM = 64, C3_BN = 64, C3_THREADS = 256;
constexpr int C3_RED_THREADS = 256;

// K step of a tile: one bf16 MFMA (32 deep) or four fp32 MFMAs (4 deep each)
template <typename T>
constexpr int C3_BK = sizeof(T) == 4 ? 16 : Frag<T>::MK;

struct Tap {
  int dz, dy, dx, wt;
};

// tap t of query class cls: input offset (relative to q * stride) and weight tap index
__device__ __forceinline__ Tap c3_tap(int transposed, int cls, int t) {
  Tap r;
  if (!transposed) {
    const int kz = t / 9, ky = (t / 3) % 3, kx = t % 3;
    r.dz = kz - 1; r.dy = ky - 1; r.dx = kx - 1; r.wt = t;
    return r;
  }
  const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
  const int ny = 1 + py, nx = 1 + px;
  const int iz = t / (ny * nx), iy = (t / nx) % ny, ix = t % nx;
  const int kz = pz ? (iz ? 2 : 0) : 1, ky = py ? (iy ? 2 : 0) : 1, kx = px ? (ix ? 2 : 0) : 1;
  r.dz = kz == 0 ? 1 : 0; r.dy = ky == 0 ? 1 : 0; r.dx = kx == 0 ? 1 : 0;
  r.wt = kz * 9 + ky * 3 + kx;
  return r;
}

struct C3Args {
  const void* A; const void* Bw; void* C; const float* bias; float* stats;
  int B, Di, Hi, Wi;      // input grid
  int Dq, Hq, Wq;         // query grid
  int Do, Ho, Wo;         // output grid
  int Cin, lda, acoff;
  int N, ldc, ccoff;
  int stride, transposed, accumulate;
  int tiles_m;
};

template <typename T, typename TO, bool VEC>
__global__ __launch_bounds__(C3_THREADS) void conv3d_igemm_kernel(const C3Args p) {
  constexpr int BK = C3_BK<T>;
  constexpr int VN = VT<T>::N;
  constexpr int ES = sizeof(T);
  constexpr int CPR = BK / VN;                  // 16-byte chunks per tile row (4)
  constexpr int RS = BK * ES + 16;              // LDS row stride in bytes
  constexpr int MAIN = (C3_BM + C3_BN) * RS;
  constexpr int CS_LD = C3_BN + 4;
  constexpr int EPI = C3_BM * CS_LD * 4;
  constexpr int LDS = MAIN > EPI ? MAIN : EPI;
  typedef typename VT<T>::vec vec;
  typedef typename Frag<T>::type frag_t;
  __shared__ __attribute__((aligned(16))) char smem[LDS];
  __shared__ int orow[C3_BM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int p16 = lane & 15, kq = lane >> 4;
  const int cls = blockIdx.z;
  const int tile_m = blockIdx.x, m0 = tile_m * C3_BM, n0 = blockIdx.y * C3_BN;
  const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
  const long Mq = (long)p.B * p.Dq * p.Hq * p.Wq;
  const int ntaps = p.transposed ? (1 + pz) * (1 + py) * (1 + px) : 27;
  const int K = ntaps * p.Cin;
  const int ldb = 27 * p.Cin;

  if (tid < C3_BM) {
    const long m = m0 + tid;
    int r = -1;
    if (m < Mq) {
      int xq = (int)(m % p.Wq);
      long t = m / p.Wq;
      int yq = (int)(t % p.Hq); t /= p.Hq;
      int zq = (int)(t % p.Dq);
      int b = (int)(t / p.Dq);
      int zo = zq, yo = yq, xo = xq;
      if (p.transposed) { zo = 2 * zq + pz; yo = 2 * yq + py; xo = 2 * xq + px; }
      r = ((b * p.Do + zo) * p.Ho + yo) * p.Wo + xo;
    }
    orow[tid] = r;
  }

  // A staging: one chunk of VN consecutive k per thread per K step, always the same tile row
  const int arow = tid / CPR, ach = tid % CPR;
  int ab = 0, az = 0, ay = 0, ax = 0;
  bool avalid;
  {
    const long m = m0 + arow;
    avalid = m < Mq;
    if (avalid) {
      ax = (int)(m % p.Wq);
      long t = m / p.Wq;
      ay = (int)(t % p.Hq); t /= p.Hq;
      az = (int)(t % p.Dq);
      ab = (int)(t / p.Dq);
    }
  }
  const int s = p.transposed ? 1 : p.stride;
  const T* Ag = reinterpret_cast<const T*>(p.A);
  const T* Bg = reinterpret_cast<const T*>(p.Bw);
  const int brow = tid / CPR, bch = tid % CPR;
  const int bn = n0 + brow;

  auto a_addr = [&](int k, long& off) -> bool {  // element offset of A(k) for this thread's row; false = zero
    const int t = k / p.Cin, c = k - t * p.Cin;
    const Tap tp = c3_tap(p.transposed, cls, t);
    const int zi = az * s + tp.dz, yi = ay * s + tp.dy, xi = ax * s + tp.dx;
    if (zi < 0 || zi >= p.Di || yi < 0 || yi >= p.Hi || xi < 0 || xi >= p.Wi) return false;
    off = ((((long)ab * p.Di + zi) * p.Hi + yi) * p.Wi + xi) * p.lda + p.acoff + c;
    return true;
  };
  auto b_addr = [&](int k) -> long {
    const int t = k / p.Cin, c = k - t * p.Cin;
    return (long)bn * ldb + c3_tap(p.transposed, cls, t).wt * p.Cin + c;
  };

  auto load = [&](int kt, vec& ar, vec& br) {
    const int k = kt * BK + ach * VN;
    if constexpr (VEC) {
      long off;
      ar = (avalid && k < K && a_addr(k, off)) ? ldvec<T>(Ag + off) : vzero<T>();
      br = (bn < p.N && k < K) ? ldvec<T>(Bg + b_addr(k)) : vzero<T>();
    } else {
      float fa[VN], fb[VN];
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        long off;
        fa[j] = (avalid && k + j < K && a_addr(k + j, off)) ? to_f32<T>(Ag[off]) : 0.f;
        fb[j] = (bn < p.N && k + j < K) ? to_f32<T>(Bg[b_addr(k + j)]) : 0.f;
      }
      ar = pack<T>(fa);
      br = pack<T>(fb);
    }
  };

  mf_f32x4 acc[2][2];
  mfma_zero(acc);

  char* As = smem;
  char* Bs = smem + C3_BM * RS;
  const int nk = (K + BK - 1) / BK;
  vec ar, br;
  load(0, ar, br);
  for (int kt = 0; kt < nk; ++kt) {
    *reinterpret_cast<vec*>(As + arow * RS + ach * 16) = ar;
    *reinterpret_cast<vec*>(Bs + brow * RS + bch * 16) = br;
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1, ar, br);
#pragma unroll
    for (int kk = 0; kk < (ES == 2 ? 1 : BK / 4); ++kk) {
      frag_t af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ra = (wm * 2 + i) * 16 + p16, rb = (wn * 2 + i) * 16 + p16;
        if constexpr (ES == 2) {
          af[i] = *reinterpret_cast<const frag_t*>(As + ra * RS + kq * 16);
          bf[i] = *reinterpret_cast<const frag_t*>(Bs + rb * RS + kq * 16);
        } else {
          af[i] = *reinterpret_cast<const float*>(As + ra * RS + (kk * 4 + kq) * 4);
          bf[i] = *reinterpret_cast<const float*>(Bs + rb * RS + (kk * 4 + kq) * 4);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
    }
    __syncthreads();
  }

  // ---- epilogue: accumulators -> LDS -> bias (+ old C) -> store; column partials of the stored values
  float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[((wm * 2 + i) * 16 + kq * 4 + r) * CS_LD + (wn * 2 + j) * 16 + p16] = acc[i][j][r];
  __syncthreads();
  TO* Cg = reinterpret_cast<TO*>(p.C);
  for (int idx = tid; idx < C3_BM * C3_BN; idx += C3_THREADS) {
    const int r = idx / C3_BN, c = idx % C3_BN, n = n0 + c;
    const int orw = orow[r];
    float v = 0.f;
    if (orw >= 0 && n < p.N) {
      v = Cs[r * CS_LD + c];
      if (p.bias) v += p.bias[n];
      TO* dst = Cg + (size_t)orw * p.ldc + p.ccoff + n;
      if (p.accumulate) v += to_f32<TO>(*dst);
      const TO o = from_f32<TO>(v);
      *dst = o;
      v = to_f32<TO>(o);
    }
    Cs[r * CS_LD + c] = v;
  }
  if (p.stats) {
    __syncthreads();
    if (tid < C3_BN && n0 + tid < p.N) {
      float s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < C3_BM; ++r) {
        const float v = Cs[r * CS_LD + tid];
        s1 += v;
        s2 += v * v;
      }
      const long row = (long)cls * p.tiles_m + tile_m;
      p.stats[row * 2 * p.N + n0 + tid] = s1;
      p.stats[row * 2 * p.N + p.N + n0 + tid] = s2;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// weight gradient: out[r][c][t] += sum over P-grid voxels m of P[m][r] * Q[m * stride + k(t) - 1][c]
// GEMM M' = R, N' = 27 C (column t * C + c), K' = voxels; split-K partial tiles in ws[split][R][27 C], folded in split order.
// Both operands are voxel-major in memory: they are staged [voxel][row] in LDS and the fragments are gathered element-wise.
struct C3WArgs {
  const void* P; const void* Q; float* ws;
  int B, Dg, Hg, Wg;      // P grid
  int Dq, Hq, Wq;         // Q grid (= P grid * stride)
  int R, C, ldp, pcoff, ldq, qcoff, stride;
  long vox_per_split;
};

template <typename T>
__global__ __launch_bounds__(C3_THREADS) void conv3d_wgrad_kernel(const C3WArgs p) {
  constexpr int BK = C3_BK<T>;
  constexpr int PAD = 2;
  constexpr int LDP = C3_BM + PAD;             // LDS row (one voxel) of the P tile, in elements
  constexpr int LDQ = C3_BN + PAD;
  typedef typename Frag<T>::type frag_t;
  __shared__ T Ps[BK * LDP];
  __shared__ T Qs[BK * LDQ];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int p16 = lane & 15, kq = lane >> 4;
  const int NC = 27 * p.C;
  const int r0 = blockIdx.y * C3_BM, c0 = blockIdx.x * C3_BN;
  const long V = (long)p.B * p.Dg * p.Hg * p.Wg;
  const long v0 = (long)blockIdx.z * p.vox_per_split;
  const long v1 = v0 + p.vox_per_split < V ? v0 + p.vox_per_split : V;
  const T* Pg = reinterpret_cast<const T*>(p.P);
  const T* Qg = reinterpret_cast<const T*>(p.Q);

  mf_f32x4 acc[2][2];
  mfma_zero(acc);

  // per-thread staging: element e of the (BK x 64) tiles, e = tid + 256 * i; voxel = e / 64, column = e % 64
  constexpr int EPT = BK * 64 / C3_THREADS;  // 8 (bf16) or 4 (fp32)
  for (long vb = v0; vb < v1; vb += BK) {
    float pv[EPT], qv[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + C3_THREADS * i, vv = e / 64, col = e % 64;
      const long m = vb + vv;
      float a = 0.f, b = 0.f;
      if (m < v1) {
        const int r = r0 + col;
        if (r < p.R) a = to_f32<T>(Pg[m * p.ldp + p.pcoff + r]);
        const int nc = c0 + col;
        if (nc < NC) {
          const int t = nc / p.C, c = nc - t * p.C;
          int x = (int)(m % p.Wg);
          long u = m / p.Wg;
          int y = (int)(u % p.Hg); u /= p.Hg;
          int z = (int)(u % p.Dg);
          int bb = (int)(u / p.Dg);
          const int zi = z * p.stride + t / 9 - 1, yi = y * p.stride + (t / 3) % 3 - 1, xi = x * p.stride + t % 3 - 1;
          if (zi >= 0 && zi < p.Dq && yi >= 0 && yi < p.Hq && xi >= 0 && xi < p.Wq)
            b = to_f32<T>(Qg[((((long)bb * p.Dq + zi) * p.Hq + yi) * p.Wq + xi) * p.ldq + p.qcoff + c]);
        }
      }
      pv[i] = a;
      qv[i] = b;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + C3_THREADS * i, vv = e / 64, col = e % 64;
      Ps[vv * LDP + col] = from_f32<T>(pv[i]);
      Qs[vv * LDQ + col] = from_f32<T>(qv[i]);
    }
    __syncthreads();
    frag_t af[2], bf[2];
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ra = (wm * 2 + i) * 16 + p16, rb = (wn * 2 + i) * 16 + p16;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          af[i][j] = Ps[(kq * 8 + j) * LDP + ra];
          bf[i][j] = Qs[(kq * 8 + j) * LDQ + rb];
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
    } else {
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int ra = (wm * 2 + i) * 16 + p16, rb = (wn * 2 + i) * 16 + p16;
          af[i] = to_f32<T>(Ps[(kk * 4 + kq) * LDP + ra]);
          bf[i] = to_f32<T>(Qs[(kk * 4 + kq) * LDQ + rb]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
      }
    }
  }
  float* W = p.ws + (size_t)blockIdx.z * p.R * NC;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + (wm * 2 + i) * 16 + kq * 4 + r, col = c0 + (wn * 2 + j) * 16 + p16;
        if (row < p.R && col < NC) W[(size_t)row * NC + col] = acc[i][j][r];
      }
}

// out[r * C * 27 + c * 27 + t] += sum over splits, in order, of ws[s][r][t * C + c]
__global__ void conv3d_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ out, int R, int C, int splits) {
  const long n = (long)R * C * 27;
  const long NC = 27L * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % 27);
    const long rc = i / 27;
    const int c = (int)(rc % C), r = (int)(rc / C);
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += ws[(size_t)k * R * NC + (size_t)r * NC + (size_t)t * C + c];
    out[i] += s;
  }
}

// ------------------------------------------------------------------------------------------------
// column reductions over rows [g * rpg, (g + 1) * rpg): CT column threads x RL row lanes, lanes folded in order.
// mode 0: ws[g][c] = sum x;   mode 1 (BatchNorm backward): ws[g][c] = sum g, ws[g][C + c] = sum g * xhat,
// g = dy * [z * scale + shift > 0], xhat = (z - mean) * rstd.
template <typename T, int MODE>
__global__ __launch_bounds__(C3_RED_THREADS) void conv3d_colsum_kernel(const T* __restrict__ x, int ldx, int xcoff,
                                                                        const T* __restrict__ z, const float* __restrict__ ss,
                                                                        float* __restrict__ ws, long M, int C, long rpg, int CT) {
  __shared__ float red[2 * 2048];
  const int RL = C3_RED_THREADS / CT;
  const int cl = threadIdx.x % CT, rl = threadIdx.x / CT;
  const long r0 = blockIdx.x * rpg, r1 = r0 + rpg < M ? r0 + rpg : M;
  for (int c = cl; c < C; c += CT) {
    float s1 = 0.f, s2 = 0.f;
    float sc = 0.f, sh = 0.f, mu = 0.f, rs = 0.f;
    if (MODE == 1) { sc = ss[c]; sh = ss[C + c]; mu = ss[2 * C + c]; rs = ss[3 * C + c]; }
    for (long r = r0 + rl; r < r1; r += RL) {
      const float v = to_f32<T>(x[r * ldx + xcoff + c]);
      if (MODE == 0) {
        s1 += v;
      } else {
        const float zz = to_f32<T>(z[r * C + c]);
        const float g = (zz * sc + sh > 0.f) ? v : 0.f;
        s1 += g;
        s2 += g * ((zz - mu) * rs);
      }
    }
    red[rl * C + c] = s1;
    if (MODE == 1) red[RL * C + rl * C + c] = s2;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += C3_RED_THREADS) {
    float s1 = 0.f, s2 = 0.f;
    for (int l = 0; l < RL; ++l) {
      s1 += red[l * C + c];
      if (MODE == 1) s2 += red[RL * C + l * C + c];
    }
    if (MODE == 0) {
      ws[(size_t)blockIdx.x * C + c] = s1;
    } else {
      ws[(size_t)blockIdx.x * 2 * C + c] = s1;
      ws[(size_t)blockIdx.x * 2 * C + C + c] = s2;
    }
  }
}

// fixed-order fold of G partial rows of width W (double), one workgroup per column: out[col] (+)= sum
__device__ __forceinline__ double c3_fold(const float* ws, int G, int W, int col) {
  __shared__ double part[C3_RED_THREADS];
  double s = 0.0;
  for (int g = threadIdx.x; g < G; g += C3_RED_THREADS) s += (double)ws[(size_t)g * W + col];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = C3_RED_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  const double r = part[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(C3_RED_THREADS) void conv3d_colsum_fold_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                             int G, int C) {
  const int c = blockIdx.x;
  const double s = c3_fold(ws, G, C, c);
  if (threadIdx.x == 0) out[c] += (float)s;
}

// BatchNorm finalize.  ss = [scale | shift | mean | rstd] ([4][C]).  Training: batch statistics from the partials (biased
// variance), running stats updated with the unbiased one, num_batches_tracked += 1.  Eval: running statistics.
__global__ __launch_bounds__(C3_RED_THREADS) void bn3d_finalize_kernel(const float* __restrict__ ws, int G, long M, int C,
                                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                       float* __restrict__ rmean, float* __restrict__ rvar,
                                                                       long long* __restrict__ nbt, float* __restrict__ ss,
                                                                       float eps, float momentum, int training) {
  const int c = blockIdx.x;
  double mean, var;
  if (training) {
    const double s1 = c3_fold(ws, G, 2 * C, c), s2 = c3_fold(ws, G, 2 * C, C + c);
    mean = s1 / (double)M;
    var = s2 / (double)M - mean * mean;
    if (var < 0.0) var = 0.0;
  } else {
    mean = rmean[c];
    var = rvar[c];
  }
  if (threadIdx.x == 0) {
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * rstd;
    ss[c] = sc;
    ss[C + c] = beta[c] - (float)mean * sc;
    ss[2 * C + c] = (float)mean;
    ss[3 * C + c] = rstd;
    if (training) {
      const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
      rmean[c] = (float)((1.0 - momentum) * rmean[c] + momentum * mean);
      rvar[c] = (float)((1.0 - momentum) * rvar[c] + momentum * unb);
      if (c == 0 && nbt) nbt[0] += 1;
    }
  }
}

template <typename T>
__global__ void bn3d_apply_relu_kernel(const T* __restrict__ z, const float* __restrict__ ss, T* __restrict__ dst, int ldd,
                                       int dcoff, long M, int C) {
  const long n = M * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float v = fmaxf(to_f32<T>(z[i]) * ss[c] + ss[C + c], 0.f);
    dst[r * ldd + dcoff + c] = from_f32<T>(v);
  }
}

// folds the backward partials: dgamma += sum g xhat, dbeta += sum g; coef = [sum g / M | sum g xhat / M] (training) or 0
__global__ __launch_bounds__(C3_RED_THREADS) void bn3d_bwd_finalize_kernel(const float* __restrict__ ws, int G, long M, int C,
                                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                           float* __restrict__ coef, int training) {
  const int c = blockIdx.x;
  const double sg = c3_fold(ws, G, 2 * C, c), sgx = c3_fold(ws, G, 2 * C, C + c);
  if (threadIdx.x == 0) {
    dgamma[c] += (float)sgx;
    dbeta[c] += (float)sg;
    coef[c] = training ? (float)(sg / (double)M) : 0.f;
    coef[C + c] = training ? (float)(sgx / (double)M) : 0.f;
  }
}

template <typename T>
__global__ void bn3d_bwd_apply_kernel(const T* __restrict__ dy, int ldy, int ycoff, const T* __restrict__ z,
                                      const float* __restrict__ ss, const float* __restrict__ gamma,
                                      const float* __restrict__ coef, T* __restrict__ dz, long M, int C) {
  const long n = M * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float zz = to_f32<T>(z[i]);
    const float g = (zz * ss[c] + ss[C + c] > 0.f) ? to_f32<T>(dy[r * ldy + ycoff + c]) : 0.f;
    const float rstd = ss[3 * C + c], xh = (zz - ss[2 * C + c]) * rstd;
    dz[i] = from_f32<T>(gamma[c] * rstd * (g - coef[c] - xh * coef[C + c]));
  }
}

// prepared weight: out[n][t * Kc + c] = src[n * sn + c * sc + (flip ? 26 - t : t)]
template <typename T>
__global__ void conv3d_prep_weight_kernel(const float* __restrict__ src, T* __restrict__ out, int N, int Kc, int sn, int sc,
                                          int flip) {
  const long n = (long)N * 27 * Kc;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / (27L * Kc));
    const int k = (int)(i - (long)row * 27 * Kc);
    const int t = k / Kc, c = k - t * Kc;
    out[i] = from_f32<T>(src[(long)row * sn + (long)c * sc + (flip ? 26 - t : t)]);
  }
}

// NCDHW fp32 <-> channels-last [B*S][C]
template <typename T>
__global__ void conv3d_to_cl_kernel(const float* __restrict__ x, T* __restrict__ out, int B, int C, long S) {
  const long n = (long)B * C * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long bs = i / C;
    const long b = bs / S, s = bs - b * S;
    out[i] = from_f32<T>(x[(b * C + c) * S + s]);
  }
}
template <typename T>
__global__ void conv3d_from_cl_kernel(const T* __restrict__ y, float* __restrict__ out, int B, int C, long S) {
  const long n = (long)B * C * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long s = i % S;
    const long bc = i / S;
    const long b = bc / C;
    const int c = (int)(bc - b * C);
    out[i] = to_f32<T>(y[(b * S + s) * C + c]);
  }
}

int c3_grid(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

long c3_colsum_groups(long M) {
  long g = (M + 511) / 512;
  return g < 1 ? 1 : g > 2048 ? 2048 : g;
}

int c3_splits(int R, int C, long V, int BK) {
  const long tiles = (long)((R + C3_BM - 1) / C3_BM) * ((27L * C + C3_BN - 1) / C3_BN);
  long s = (1024 + tiles - 1) / tiles;
  const long maxs = (V + 8L * BK - 1) / (8L * BK);  // at least 8 K steps per split
  if (s > maxs) s = maxs;
  if (s > 256) s = 256;
  return (int)(s < 1 ? 1 : s);
}

bool c3_al(const void* p, int vn, int es) { return ((uintptr_t)p % (vn * es)) == 0; }

}  // namespace

extern "C" int32_t vsx_conv3d_prep_weight(const float* w, void* out, int32_t N, int32_t Kc, int32_t sn, int32_t sc, int32_t flip,
                                          int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(w && out && N > 0 && Kc > 0, "vsx_conv3d_prep_weight: bad arguments");
  const long n = (long)N * 27 * Kc;
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv3d_prep_weight_kernel<T>, dim3(c3_grid(n)), dim3(256), 0, (hipStream_t)stream, w, (T*)out, N, Kc, sn, sc, flip);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_conv3d_stats_rows(int32_t B, int32_t Di, int32_t Hi, int32_t Wi, int32_t stride, int32_t transposed) {
  if (B <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || (stride != 1 && stride != 2)) return -1;
  const long Mq = transposed ? (long)B * Di * Hi * Wi : (long)B * (Di / stride) * (Hi / stride) * (Wi / stride);
  return (long)((Mq + C3_BM - 1) / C3_BM) * (transposed ? 8 : 1);
}

extern "C" int32_t vsx_conv3d_fwd(const void* a, int32_t lda, int32_t acoff, const void* wp, const float* bias, void* c, int32_t ldc,
                                  int32_t ccoff, float* stats, int32_t B, int32_t Di, int32_t Hi, int32_t Wi, int32_t Cin, int32_t Cout,
                                  int32_t stride, int32_t transposed, int32_t accumulate, int32_t dtype, int32_t out_f32,
                                  vsx_stream_t stream) {
  VSX_CHECK(a && wp && c && B > 0 && Di > 0 && Hi > 0 && Wi > 0 && Cin > 0 && Cout > 0, "vsx_conv3d_fwd: bad arguments");
  VSX_CHECK(transposed ? stride == 2 : (stride == 1 || (stride == 2 && Di % 2 == 0 && Hi % 2 == 0 && Wi % 2 == 0)),
            "vsx_conv3d_fwd: stride %d on %dx%dx%d not served", stride, Di, Hi, Wi);
  VSX_CHECK(lda >= acoff + Cin && ldc >= ccoff + Cout && acoff >= 0 && ccoff >= 0, "vsx_conv3d_fwd: row strides too small");
  C3Args p;
  p.A = a; p.Bw = wp; p.C = c; p.bias = bias; p.stats = stats;
  p.B = B; p.Di = Di; p.Hi = Hi; p.Wi = Wi;
  if (transposed) {
    p.Dq = Di; p.Hq = Hi; p.Wq = Wi;
    p.Do = 2 * Di; p.Ho = 2 * Hi; p.Wo = 2 * Wi;
  } else {
    p.Dq = p.Do = Di / stride; p.Hq = p.Ho = Hi / stride; p.Wq = p.Wo = Wi / stride;
  }
  p.Cin = Cin; p.lda = lda; p.acoff = acoff;
  p.N = Cout; p.ldc = ldc; p.ccoff = ccoff;
  p.stride = stride; p.transposed = transposed; p.accumulate = accumulate;
  const long Mq = (long)B * p.Dq * p.Hq * p.Wq;
  VSX_CHECK(Mq / C3_BM < 2147483647L && (long)B * p.Do * p.Ho * p.Wo * ldc < (1L << 40), "vsx_conv3d_fwd: problem too large");
  p.tiles_m = (int)((Mq + C3_BM - 1) / C3_BM);
  dim3 grid(p.tiles_m, (Cout + C3_BN - 1) / C3_BN, transposed ? 8 : 1);
  hipStream_t s = (hipStream_t)stream;
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int VN = VT<T>::N, ES = sizeof(T);
    const bool vec = Cin % VN == 0 && lda % VN == 0 && acoff % VN == 0 && c3_al(a, VN, ES) && c3_al(wp, VN, ES);
    vsx_by_bool(out_f32, [&](auto f32_out) {
      using TO = std::conditional_t<decltype(f32_out)::value, float, T>;  // fp32 input writes fp32 either way
      vsx_by_bool(vec, [&](auto vec_) {
        hipLaunchKernelGGL((conv3d_igemm_kernel<T, TO, decltype(vec_)::value>), grid, dim3(C3_THREADS), 0, s, p);
      });
    });
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_conv3d_wgrad_ws_floats(int32_t B, int32_t Dg, int32_t Hg, int32_t Wg, int32_t R, int32_t C, int32_t dtype) {
  const long V = (long)B * Dg * Hg * Wg;
  return (long)c3_splits(R, C, V, dtype == VSX_BF16 ? 32 : 16) * R * 27 * C;
}

extern "C" int32_t vsx_conv3d_wgrad(const void* P, int32_t ldp, int32_t pcoff, const void* Q, int32_t ldq, int32_t qcoff, float* ws,
                                    int64_t ws_floats, float* out, int32_t B, int32_t Dg, int32_t Hg, int32_t Wg, int32_t R, int32_t C,
                                    int32_t stride, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(P && Q && ws && out && B > 0 && Dg > 0 && Hg > 0 && Wg > 0 && R > 0 && C > 0 && (stride == 1 || stride == 2),
            "vsx_conv3d_wgrad: bad arguments");
  VSX_CHECK(ldp >= pcoff + R && ldq >= qcoff + C, "vsx_conv3d_wgrad: row strides too small");
  const int BK = dtype == VSX_BF16 ? 32 : 16;
  const long V = (long)B * Dg * Hg * Wg;
  const int splits = c3_splits(R, C, V, BK);
  VSX_CHECK(ws_floats >= (long)splits * R * 27 * C, "vsx_conv3d_wgrad: workspace of %ld floats too small", (long)ws_floats);
  C3WArgs p;
  p.P = P; p.Q = Q; p.ws = ws;
  p.B = B; p.Dg = Dg; p.Hg = Hg; p.Wg = Wg;
  p.Dq = Dg * stride; p.Hq = Hg * stride; p.Wq = Wg * stride;
  p.R = R; p.C = C; p.ldp = ldp; p.pcoff = pcoff; p.ldq = ldq; p.qcoff = qcoff; p.stride = stride;
  long per = (V + splits - 1) / splits;
  p.vox_per_split = (per + BK - 1) / BK * BK;
  const int gs = (int)((V + p.vox_per_split - 1) / p.vox_per_split);  // splits that own voxels (<= splits)
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((27 * C + C3_BN - 1) / C3_BN, (R + C3_BM - 1) / C3_BM, gs);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv3d_wgrad_kernel<T>, grid, dim3(C3_THREADS), 0, s, p);
  });
  VSX_LAUNCH_CHECK();
  const long n = (long)R * C * 27;
  hipLaunchKernelGGL(conv3d_wgrad_fold_kernel, dim3(c3_grid(n)), dim3(256), 0, s, ws, out, R, C, gs);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_conv3d_colsum_groups(int64_t M) { return c3_colsum_groups(M); }

static int c3_ct(int C) {
  int ct = 1;
  while (ct < C && ct < C3_RED_THREADS) ct <<= 1;
  return ct;
}

extern "C" int32_t vsx_conv3d_colsum(const void* x, int32_t ldx, int32_t xcoff, int64_t M, int32_t C, float* ws, float* out,
                                     int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(x && ws && out && M > 0 && C > 0 && C <= 2048 && ldx >= xcoff + C, "vsx_conv3d_colsum: bad arguments");
  const long G = c3_colsum_groups(M), rpg = (M + G - 1) / G;
  const int ct = c3_ct(C);
  VSX_CHECK((long)(C3_RED_THREADS / ct) * C <= 2048, "vsx_conv3d_colsum: C=%d not served", C);
  hipStream_t s = (hipStream_t)stream;
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((conv3d_colsum_kernel<T, 0>), dim3(G), dim3(C3_RED_THREADS), 0, s, (const T*)x, ldx, xcoff, (const T*)nullptr,
                       (const float*)nullptr, ws, M, C, rpg, ct);
  });
  VSX_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv3d_colsum_fold_kernel, dim3(C), dim3(C3_RED_THREADS), 0, s, ws, out, (int)G, C);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_bn3d_finalize(const float* ws, int64_t G, int64_t M, int32_t C, const float* gamma, const float* beta,
                                     float* rmean, float* rvar, int64_t* nbt, float* ss, float eps, float momentum, int32_t training,
                                     vsx_stream_t stream) {
  VSX_CHECK(gamma && beta && rmean && rvar && ss && C > 0 && (!training || (ws && G > 0 && M > 0)), "vsx_bn3d_finalize: bad arguments");
  hipLaunchKernelGGL(bn3d_finalize_kernel, dim3(C), dim3(C3_RED_THREADS), 0, (hipStream_t)stream, ws, (int)G, M, C, gamma, beta, rmean,
                     rvar, (long long*)nbt, ss, eps, momentum, training);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_bn3d_apply_relu(const void* z, const float* ss, void* dst, int32_t ldd, int32_t dcoff, int64_t M, int32_t C,
                                       int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(z && ss && dst && M > 0 && C > 0 && ldd >= dcoff + C, "vsx_bn3d_apply_relu: bad arguments");
  const int g = c3_grid(M * C);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(bn3d_apply_relu_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)z, ss, (T*)dst, ldd, dcoff, M, C);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_bn3d_bwd_ws_floats(int64_t M, int32_t C) { return c3_colsum_groups(M) * 2 * C + 2 * C; }

extern "C" int32_t vsx_bn3d_bwd(const void* dy, int32_t ldy, int32_t ycoff, const void* z, const float* ss, const float* gamma,
                                float* ws, float* dgamma, float* dbeta, void* dz, int64_t M, int32_t C, int32_t training, int32_t dtype,
                                vsx_stream_t stream) {
  VSX_CHECK(dy && z && ss && gamma && ws && dgamma && dbeta && dz && M > 0 && C > 0 && C <= 1024 && ldy >= ycoff + C,
            "vsx_bn3d_bwd: bad arguments");
  const long G = c3_colsum_groups(M), rpg = (M + G - 1) / G;
  const int ct = c3_ct(C);
  VSX_CHECK((long)(C3_RED_THREADS / ct) * C <= 2048, "vsx_bn3d_bwd: C=%d not served", C);
  float* coef = ws + G * 2 * C;
  hipStream_t s = (hipStream_t)stream;
  const int g = c3_grid(M * C);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((conv3d_colsum_kernel<T, 1>), dim3(G), dim3(C3_RED_THREADS), 0, s, (const T*)dy, ldy, ycoff, (const T*)z, ss, ws,
                       M, C, rpg, ct);
  });
  VSX_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn3d_bwd_finalize_kernel, dim3(C), dim3(C3_RED_THREADS), 0, s, ws, (int)G, M, C, dgamma, dbeta, coef, training);
  VSX_LAUNCH_CHECK();
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(bn3d_bwd_apply_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)dy, ldy, ycoff, (const T*)z, ss, gamma, coef,
                       (T*)dz, M, C);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_conv3d_to_cl(const float* x, void* out, int32_t B, int32_t C, int64_t S, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(x && out && B > 0 && C > 0 && S > 0, "vsx_conv3d_to_cl: bad arguments");
  const int g = c3_grid((long)B * C * S);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv3d_to_cl_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, x, (T*)out, B, C, S);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_conv3d_from_cl(const void* y, float* out, int32_t B, int32_t C, int64_t S, int32_t dtype, vsx_stream_t stream) {
  VSX_CHECK(y && out && B > 0 && C > 0 && S > 0, "vsx_conv3d_from_cl: bad arguments");
  const int g = c3_grid((long)B * C * S);
  vsx_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv3d_from_cl_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)y, out, B, C, S);
  });
  VSX_LAUNCH_CHECK();
  return 0;
}
