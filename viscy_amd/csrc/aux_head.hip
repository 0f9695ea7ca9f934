// viscy_amd — classifier and loss of the DynaCLR auxiliary ClassificationHead (viscy_models/components/heads.py:159-272, 420-453):
// cross-entropy over the logits of a cosine or a linear classifier, with top-1 / top-k accuracy, without storing the [B, C]
// logits on the training path.  All arithmetic is fp32; dot products run on the exact f32-in / f32-accumulate MFMA
// (v_mfma_f32_32x32x2_f32), so a class rank does not depend on a reduced-precision rounding.
//
//   inv(x)  = 1 / max(||x||, 1e-12)                         F.normalize's rule: a zero row has inv = 1e12 and a zero unit vector
//   cosine:   z_bc = fl32(fl32(fl32(dot_bc * inv_h[b]) * inv_w[c]) * scale),   scale = expf(log_scale[0])
//   linear:   z_bc = fl32(dot_bc + bias[c])                 (bias == nullptr: z_bc = dot_bc)
//   dot_bc accumulates h[b, :] . W[c, :] in fp32 on the tile engine of f32_tile.h, whose one summation order holds for every
//   (b, c) and for every entry point of this file.
//
// Forward (vsx_cls_ce_fwd), four launches, no atomics:
//   (1) the target logit z_y of every row: one 128 x 128 MFMA tile per 128 rows whose class operand is the GATHERED rows
//       W[y_b]; its diagonal is z_y, bit-identical to what (2) forms for class y_b (same instruction, same feature order)
//   (2) a workgroup owns 128 rows and a contiguous range of class tiles (128 classes each).  Per tile it forms the logits in
//       registers, passes them through LDS one 64-class half at a time, and thread r < 128 scans row r: the tile's
//       (max m, sum of exp(z - m), number of classes ahead of the target).  "Ahead" is the total order (z descending, class
//       ascending): z_c > z_y, or z_c == z_y and c < y.  The triple of every (tile, row) goes to the workspace, so the
//       partials are those of the TILES and do not depend on how many workgroups share the class range
//   (3) per row: the tiles' triples merged in ascending tile order -> rows [B, 4] = {lse, z_y, rank, valid}
//   (4) one workgroup folds the rows in a fixed order -> acc [4] = {loss, top-1, top-k, n_valid}
//       loss = sum_valid (lse - z_y) / n_valid, top-1 = #(rank == 0) / B, top-k = #(rank < k) / B
// rows and acc are bit-identical from run to run and for every split count.
//
// Labels: -100 (F.cross_entropy's ignore_index) marks a row invalid (valid = 0): it counts in no sum and its gradient is exactly
// zero; all rows ignored -> loss = 0 / 0 = NaN, as torch.  Any other label outside [0, C) NEVER indexes memory: the row is
// invalid (valid = -1) and the loss is set to NaN.  A non-finite logit reaches the loss as in torch (+inf or NaN -> NaN).
//
// Backward (vsx_cls_ce_bwd) keeps dZ = (softmax - onehot) * gout / n_valid in a [B, C] workspace (as vsx_ntxent_* keeps dS),
// re-forming the logits with the same tile loop, and contracts it with two launches of one plain-FMA kernel (eight output
// rows per workgroup, the contraction range cut into four fixed quarters that are added in order):
//   dh[b] = inv_h[b] * (r - (r . h^[b]) h^[b]),  r = scale * sum_c dZ[b, c] w^[c]        (h^ = h * inv_h, w^ = W * inv_w)
//   dW[c] += inv_w[c] * (q - (q . w^[c]) w^[c]), q = scale * sum_b dZ[b, c] h^[b]
//   d log_scale += sum_b r_b . h^[b]             (= sum_bc dZ z, folded by one workgroup in row order)
// where a row at the 1e-12 clamp takes no projection term (the clamp's derivative, as torch).  Linear: dh = sum_c dZ W,
// dW += dZ^T h, dbias += column sums of dZ.  Every sum has a fixed order: ALL gradients are bit-reproducible; nothing here
// goes through the split-K GEMMs.
#include "f32_tile.h"
#include "../../include/vsx.h"

#include <math.h>

#define CH_IGNORE (-100)
#define CH_NORM_EPS 1e-12f

#define CH_SCAN 0        // modes of the tile kernel
#define CH_DZ 1
#define CH_LOGITS 2
#define CH_TARGET 3

struct ChArgs {
  const float* h;          // [B, H]
  const float* W;          // [C, H]
  const int64_t* labels;   // [B] (not read by CH_LOGITS)
  const float* inv_h;      // cosine: [B]; nullptr = linear
  const float* inv_w;      // cosine: [C]
  const float* log_scale;  // cosine: [1]
  const float* bias;       // linear: [C] or nullptr
  int B, H, C;
};

__device__ __forceinline__ float ch_logit(bool cosine, float dot, float ih, float cw, float scale) {
  return cosine ? __fmul_rn(__fmul_rn(__fmul_rn(dot, ih), cw), scale) : __fadd_rn(dot, cw);
}

// CH_SCAN:   in0 = zy [B];                                   out = partials [ctiles][B][3]
// CH_DZ:     in0 = rows [B, 4], in1 = acc [4], in2 = gout;   out = dZ [B, C]
// CH_LOGITS:                                                 out = Z [B, C]
// CH_TARGET:                                                 out = zy [B]   (grid.y = 1, one gathered tile)
template <int MODE>
__global__ __launch_bounds__(FT_THREADS, 2) void ch_tile_kernel(ChArgs a, int tiles_per_split, const float* __restrict__ in0,
                                                                const float* __restrict__ in1, const float* __restrict__ in2,
                                                                float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float stage[FT_STAGE];  // the engine's staging area; later the logit half-tile
  __shared__ float invq[FT_T], colw[FT_T], rowl[FT_T];
  __shared__ int ylab[FT_T];

  const FtLane l = ft_lane();
  const int t = l.t;
  FtRange g = ft_range(a.C, a.H, tiles_per_split);
  if (MODE == CH_TARGET) g.ct0 = 0, g.ct1 = 1;  // the one gathered tile
  const int q0 = g.q0;
  const bool cosine = a.inv_h != nullptr;
  const float scale = cosine ? expf(a.log_scale[0]) : 1.f;

  // the row's label, -1 where the row is invalid (ignored, out of range, past B)
  int yown = -1;
  float zyown = 0.f;
  if (t < FT_T) {
    const int i = q0 + t;
    if (MODE != CH_LOGITS && i < a.B) {
      const int64_t y = a.labels[i];
      if (y >= 0 && y < (int64_t)a.C) yown = (int)y;
      if (MODE == CH_DZ && !(in0[(size_t)i * 4 + 3] > 0.5f)) yown = -1;
    }
    ylab[t] = yown;
    invq[t] = cosine && i < a.B ? a.inv_h[i] : 0.f;
    if (MODE == CH_SCAN) zyown = i < a.B ? in0[i] : 0.f;
    if (MODE == CH_DZ) rowl[t] = i < a.B ? in0[(size_t)i * 4] : 0.f;
    if (MODE == CH_TARGET) colw[t] = yown >= 0 ? (cosine ? a.inv_w[yown] : (a.bias ? a.bias[yown] : 0.f)) : 0.f;
  }
  const bool owner = t < FT_T && q0 + t < a.B;
  const float coef = MODE == CH_DZ ? __fdiv_rn(in2[0], in1[3]) : 0.f;
  __syncthreads();

  for (int ct = g.ct0; ct < g.ct1; ++ct) {
    const int c0 = ct * FT_T;
    ft_f32x16 acc[2][2];
    ft_dots(
        acc, stage, l, g.nchunks,
        // the class operand's row is c0 + r, or, for the target tile, the label of query row r (-1 = none, the row stays zero);
        // H % 4 == 0 and both operands 16-byte aligned
        [&](int operand, int r, int kk) {
          if (!operand) return ft_row4<true>(a.h, q0 + r, a.B, a.H, kk);
          return ft_row4<true>(a.W, MODE == CH_TARGET ? ylab[r] : c0 + r, a.C, a.H, kk);
        },
        [&] {
          if (MODE != CH_TARGET && t < FT_T) {
            const int j = c0 + t;
            colw[t] = j < a.C ? (cosine ? a.inv_w[j] : (a.bias ? a.bias[j] : 0.f)) : 0.f;
          }
        });

    if (MODE == CH_TARGET) {
      ft_each(acc, l, [&](float dot, int row, int col) {  // the tile's diagonal
        if (row == col && q0 + row < a.B) out[q0 + row] = ylab[row] >= 0 ? ch_logit(cosine, dot, invq[row], colw[row], scale) : 0.f;
      });
    } else if (MODE == CH_DZ || MODE == CH_LOGITS) {
      ft_each(acc, l, [&](float dot, int row, int lc) {
        const int col = c0 + lc;
        const float cw = colw[lc];  // ahead of the bounds test: one LDS read per column, not one per dot
        if (q0 + row < a.B && col < a.C) {
          const float z = ch_logit(cosine, dot, invq[row], cw, scale);
          float v = z;
          if (MODE == CH_DZ) {
            const int y = ylab[row];
            v = y >= 0 ? __fmul_rn(__fsub_rn(expf(__fsub_rn(z, rowl[row])), col == y ? 1.f : 0.f), coef) : 0.f;
          }
          out[(size_t)(q0 + row) * a.C + col] = v;
        }
      });
    } else {
      float m = -INFINITY, ssum = 0.f;
      int ahead = 0;
      __syncthreads();  // every wave is done with the staged chunk: the half-tile takes its place
      for (int h = 0; h < 2; ++h) {
        ft_put_half(stage, acc, l, h, [&](float dot, int row, int col) {
          return c0 + col < a.C ? ch_logit(cosine, dot, invq[row], colw[col], scale) : -INFINITY;
        });
        __syncthreads();
        if (owner) {
          const float* srow = ft_half_row(stage, t);
          const int jbase = c0 + h * 64;
          float hm = -INFINITY;
          for (int c = 0; c < 64; ++c) hm = fmaxf(hm, srow[c]);  // a NaN is skipped here and reaches the sum below
          const float nm = fmaxf(m, hm);
          if (nm == -INFINITY) {
            for (int c = 0; c < 64; ++c)
              if (srow[c] != srow[c]) ssum = srow[c];
          } else {
            float sh = 0.f;
            for (int c = 0; c < 64; ++c) sh = __fadd_rn(sh, expf(__fsub_rn(srow[c], nm)));
            ssum = __fadd_rn(__fmul_rn(ssum, expf(__fsub_rn(m, nm))), sh);
            m = nm;
          }
          if (yown >= 0)
            for (int c = 0; c < 64; ++c) {
              const float z = srow[c];
              const int j = jbase + c;
              ahead += (j != yown) && (z > zyown || (z == zyown && j < yown));
            }
        }
        __syncthreads();
      }
      if (owner) {
        float* p = out + ((size_t)ct * a.B + (size_t)(q0 + t)) * 3;
        p[0] = m;
        p[1] = ssum;
        p[2] = (float)ahead;
      }
    }
  }
}

// (3) the tiles' triples of every row in ascending tile order
__global__ __launch_bounds__(256) void ch_merge_kernel(const float* __restrict__ part, const float* __restrict__ zy,
                                                       const int64_t* __restrict__ labels, int B, int C, int ntiles,
                                                       float* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  float M = -INFINITY;
  for (int ct = 0; ct < ntiles; ++ct) M = fmaxf(M, part[((size_t)ct * B + i) * 3]);
  float S = 0.f, ahead = 0.f;
  for (int ct = 0; ct < ntiles; ++ct) {
    const float* p = part + ((size_t)ct * B + i) * 3;
    S = __fadd_rn(S, p[0] == -INFINITY ? p[1] : __fmul_rn(p[1], expf(__fsub_rn(p[0], M))));
    ahead += p[2];
  }
  const int64_t y = labels[i];
  const bool ok = y >= 0 && y < (int64_t)C;
  float* r = rows + (size_t)i * 4;
  r[0] = __fadd_rn(M, logf(S));
  r[1] = ok ? zy[i] : 0.f;
  r[2] = ok ? ahead : (float)C;
  r[3] = ok ? 1.f : (y == CH_IGNORE ? 0.f : -1.f);
}

// (4) one workgroup: thread t sums rows t, t + 256, ... in order, then the 256 partials fold as a fixed tree
__global__ __launch_bounds__(256) void ch_fold_kernel(const float* __restrict__ rows, int B, int k, float* __restrict__ acc) {
  __shared__ float red[5][256];
  const int t = threadIdx.x;
  float loss = 0.f, top1 = 0.f, topk = 0.f, n = 0.f, bad = 0.f;
  for (int i = t; i < B; i += 256) {
    const float* r = rows + (size_t)i * 4;
    if (r[3] > 0.5f) {
      loss = __fadd_rn(loss, __fsub_rn(r[0], r[1]));
      n += 1.f;
      top1 += r[2] == 0.f ? 1.f : 0.f;
      topk += r[2] < (float)k ? 1.f : 0.f;
    } else if (r[3] < -0.5f) {
      bad = 1.f;
    }
  }
  red[0][t] = loss; red[1][t] = top1; red[2][t] = topk; red[3][t] = n; red[4][t] = bad;
  block_tree_sum<5>(red, t);
  if (t == 0) {
    acc[0] = red[4][0] > 0.f ? __builtin_nanf("") : __fdiv_rn(red[0][0], red[3][0]);
    acc[1] = __fdiv_rn(red[1][0], (float)B);
    acc[2] = __fdiv_rn(red[2][0], (float)B);
    acc[3] = red[3][0];
  }
}

// ------------------------------------------------------------------ backward contractions
// raw[r, :] = scale * sum_j G(r, j) * inv_y[j] * Y[j, :],  G(r, j) = G[r * gs_r + j * gs_j]
// COS:  dst[r, :] (+)= inv_x[r] * (raw - (raw . x^[r]) x^[r]),  x^ = X * inv_x;  tdot[r] = raw . x^[r]
// else: dst[r, :] (+)= raw;  gsum[r] += sum_j G(r, j)
// A workgroup owns CC_RB rows; wave w takes the w-th quarter of j; the quarters are added in order.  Wave w then finishes rows
// w and w + 4: it re-reads what its own lanes stored to `raw` (== dst where dst is not accumulated into).
#define CC_RB 8
template <bool COS>
__global__ __launch_bounds__(256) void ch_contract_kernel(const float* __restrict__ G, long gs_r, long gs_j, int R, int J, int H,
                                                          const float* __restrict__ Y, const float* __restrict__ inv_y,
                                                          const float* __restrict__ X, const float* __restrict__ inv_x,
                                                          const float* __restrict__ log_scale, float* raw, float* dst,
                                                          int accumulate, float* __restrict__ tdot, float* __restrict__ gsum) {
  __shared__ float4 part[4][CC_RB][64];
  __shared__ float gred[4][CC_RB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r0 = blockIdx.x * CC_RB;
  const float scale = COS ? expf(log_scale[0]) : 1.f;
  const int jper = (J + 3) / 4;
  const int j0 = min(wave * jper, J), j1 = min(j0 + jper, J);
  float dot[2] = {0.f, 0.f};

  for (int h0 = 0; h0 < H; h0 += 256) {
    const int hc = h0 + 4 * lane;
    const bool hin = hc < H;
    float4 acc[CC_RB];
    float gs[CC_RB];
#pragma unroll
    for (int r = 0; r < CC_RB; ++r) {
      acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      gs[r] = 0.f;
    }
    for (int j = j0; j < j1; ++j) {
      float4 y = hin ? *reinterpret_cast<const float4*>(Y + (size_t)j * H + hc) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (COS) {
        const float iy = inv_y[j];
        y.x = __fmul_rn(y.x, iy); y.y = __fmul_rn(y.y, iy); y.z = __fmul_rn(y.z, iy); y.w = __fmul_rn(y.w, iy);
      }
#pragma unroll
      for (int r = 0; r < CC_RB; ++r) {
        const float g = r0 + r < R ? G[(size_t)(r0 + r) * gs_r + (size_t)j * gs_j] : 0.f;
        acc[r].x = fmaf(g, y.x, acc[r].x); acc[r].y = fmaf(g, y.y, acc[r].y);
        acc[r].z = fmaf(g, y.z, acc[r].z); acc[r].w = fmaf(g, y.w, acc[r].w);
        gs[r] = __fadd_rn(gs[r], g);
      }
    }
#pragma unroll
    for (int r = 0; r < CC_RB; ++r) part[wave][r][lane] = acc[r];
    if (!COS && h0 == 0 && lane == 0)
#pragma unroll
      for (int r = 0; r < CC_RB; ++r) gred[wave][r] = gs[r];
    __syncthreads();
    if (!COS && gsum && h0 == 0 && t < CC_RB && r0 + t < R)
      gsum[r0 + t] = __fadd_rn(gsum[r0 + t], __fadd_rn(__fadd_rn(__fadd_rn(gred[0][t], gred[1][t]), gred[2][t]), gred[3][t]));
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = wave + 4 * u, row = r0 + r;
      if (row < R && hin) {
        float4 v = part[0][r][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const float4 p = part[w][r][lane];
          v.x = __fadd_rn(v.x, p.x); v.y = __fadd_rn(v.y, p.y); v.z = __fadd_rn(v.z, p.z); v.w = __fadd_rn(v.w, p.w);
        }
        if (COS) {
          v.x = __fmul_rn(v.x, scale); v.y = __fmul_rn(v.y, scale); v.z = __fmul_rn(v.z, scale); v.w = __fmul_rn(v.w, scale);
          const float ix = inv_x[row];
          const float4 x = *reinterpret_cast<const float4*>(X + (size_t)row * H + hc);
          dot[u] = fmaf(v.x, __fmul_rn(x.x, ix), dot[u]); dot[u] = fmaf(v.y, __fmul_rn(x.y, ix), dot[u]);
          dot[u] = fmaf(v.z, __fmul_rn(x.z, ix), dot[u]); dot[u] = fmaf(v.w, __fmul_rn(x.w, ix), dot[u]);
        }
        *reinterpret_cast<float4*>(raw + (size_t)row * H + hc) = v;
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = r0 + wave + 4 * u;
    if (row >= R) continue;  // wave-uniform
    float d = 0.f, ix = 1.f;
    if (COS) {
      d = ft_wave_sum(dot[u]);
      ix = inv_x[row];
      if (tdot && lane == 0) tdot[row] = d;
      if (ix >= __fdiv_rn(1.f, CH_NORM_EPS)) d = 0.f;  // at the clamp x^ = x / eps: no projection term
    }
    if (!COS && !accumulate && raw == dst) continue;  // the sums are the result
    for (int hc = 4 * lane; hc < H; hc += 256) {
      float4 v = *reinterpret_cast<const float4*>(raw + (size_t)row * H + hc);
      if (COS) {
        const float4 x = *reinterpret_cast<const float4*>(X + (size_t)row * H + hc);
        v.x = __fmul_rn(ix, __fsub_rn(v.x, __fmul_rn(d, __fmul_rn(x.x, ix))));
        v.y = __fmul_rn(ix, __fsub_rn(v.y, __fmul_rn(d, __fmul_rn(x.y, ix))));
        v.z = __fmul_rn(ix, __fsub_rn(v.z, __fmul_rn(d, __fmul_rn(x.z, ix))));
        v.w = __fmul_rn(ix, __fsub_rn(v.w, __fmul_rn(d, __fmul_rn(x.w, ix))));
      }
      float4* o = reinterpret_cast<float4*>(dst + (size_t)row * H + hc);
      if (accumulate) {
        const float4 old = *o;
        v.x = __fadd_rn(old.x, v.x); v.y = __fadd_rn(old.y, v.y); v.z = __fadd_rn(old.z, v.z); v.w = __fadd_rn(old.w, v.w);
      }
      *o = v;
    }
  }
}

// dst[0] += sum_i v[i]: thread t sums i = t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void ch_sum_add_kernel(const float* __restrict__ v, int n, float* __restrict__ dst) {
  __shared__ float red[1][256];
  const int t = threadIdx.x;
  float s = 0.f;
  for (int i = t; i < n; i += 256) s = __fadd_rn(s, v[i]);
  red[0][t] = s;
  block_tree_sum<1>(red, t);
  if (t == 0) dst[0] = __fadd_rn(dst[0], red[0][0]);
}

// ------------------------------------------------------------------ host
static int ch_range(const char* who, int64_t B, int64_t H, int64_t C) {
  VSX_CHECK(B >= 1 && B <= (1 << 24), "%s: B=%ld must be in [1, 2^24]", who, (long)B);
  VSX_CHECK(H >= 4 && H <= (1 << 20) && H % 4 == 0, "%s: H=%ld must be a multiple of 4 in [4, 2^20]", who, (long)H);
  VSX_CHECK(C >= 1 && C <= (1 << 24), "%s: C=%ld must be in [1, 2^24]", who, (long)C);
  return 0;
}

static int ch_operands(const char* who, const float* h, const float* W, const float* inv_h, const float* inv_w,
                       const float* log_scale, const float* bias) {
  VSX_CHECK(h && W && vsx_al16(h) && vsx_al16(W), "%s: h and W must be non-null and 16-byte aligned", who);
  if (inv_h || inv_w || log_scale)
    VSX_CHECK(inv_h && inv_w && log_scale && !bias, "%s: the cosine classifier takes inv_h, inv_w and log_scale, and no bias", who);
  return 0;
}

extern "C" int32_t vsx_cls_inv_norm(const float* x, float* inv, int32_t N, int32_t d, vsx_stream_t stream) {
  return ft_inv_norm<true>("vsx_cls_inv_norm", x, inv, N, d, CH_NORM_EPS, (hipStream_t)stream);
}

extern "C" int64_t vsx_cls_ce_fwd_ws_bytes(int32_t B, int32_t H, int32_t C) {
  if (B < 1 || H < 4 || H % 4 || C < 1) return 0;
  const int64_t ntiles = (C + FT_T - 1) / FT_T;
  return (ntiles * B * 3 + B) * 4;  // the tiles' triples, then zy[B]
}

extern "C" int32_t vsx_cls_ce_fwd(const float* h, const float* W, const int64_t* labels, const float* inv_h, const float* inv_w,
                                  const float* log_scale, const float* bias, int32_t B, int32_t H, int32_t C, int32_t k,
                                  int32_t splits, float* rows, float* acc, void* ws, int64_t ws_bytes, vsx_stream_t stream) {
  if (int rc = ch_range("vsx_cls_ce_fwd", B, H, C)) return rc;
  VSX_CHECK(k >= 1 && k <= C, "vsx_cls_ce_fwd: k=%d must be in [1, C=%d]", k, C);
  if (int rc = ch_operands("vsx_cls_ce_fwd", h, W, inv_h, inv_w, log_scale, bias)) return rc;
  VSX_CHECK(labels && rows && acc && ws, "vsx_cls_ce_fwd: null argument");
  VSX_CHECK(ws_bytes >= vsx_cls_ce_fwd_ws_bytes(B, H, C) && ((uintptr_t)ws & 3) == 0,
            "vsx_cls_ce_fwd: the workspace must be 4-byte aligned and hold vsx_cls_ce_fwd_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_cls_ce_fwd_ws_bytes(B, H, C), (long)ws_bytes);
  const int qtiles = (B + FT_T - 1) / FT_T, ntiles = (C + FT_T - 1) / FT_T;
  VSX_CHECK(splits >= 0, "vsx_cls_ce_fwd: splits=%d (0 = chosen here)", splits);
  int tps;  // splits = 0: fill two workgroup slots per compute unit
  ft_even_split(ntiles, splits ? splits : (2L * vsx_cu_count() + qtiles - 1) / qtiles, &splits, &tps);
  float* part = (float*)ws;
  float* zy = part + (size_t)ntiles * B * 3;
  const ChArgs a = {h, W, labels, inv_h, inv_w, log_scale, bias, B, H, C};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL((ch_tile_kernel<CH_TARGET>), dim3((unsigned)qtiles), dim3(FT_THREADS), 0, s, a, 1, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, zy);
  hipLaunchKernelGGL((ch_tile_kernel<CH_SCAN>), dim3((unsigned)qtiles, (unsigned)splits), dim3(FT_THREADS), 0, s, a, tps,
                     (const float*)zy, (const float*)nullptr, (const float*)nullptr, part);
  hipLaunchKernelGGL(ch_merge_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (const float*)part, (const float*)zy, labels,
                     B, C, ntiles, rows);
  hipLaunchKernelGGL(ch_fold_kernel, dim3(1), dim3(256), 0, s, (const float*)rows, B, k, acc);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t vsx_cls_logits(const float* h, const float* W, const float* inv_h, const float* inv_w, const float* log_scale,
                                  const float* bias, int32_t B, int32_t H, int32_t C, float* Z, vsx_stream_t stream) {
  if (int rc = ch_range("vsx_cls_logits", B, H, C)) return rc;
  if (int rc = ch_operands("vsx_cls_logits", h, W, inv_h, inv_w, log_scale, bias)) return rc;
  VSX_CHECK(Z != nullptr, "vsx_cls_logits: null argument");
  const int qtiles = (B + FT_T - 1) / FT_T, ntiles = (C + FT_T - 1) / FT_T;
  const ChArgs a = {h, W, nullptr, inv_h, inv_w, log_scale, bias, B, H, C};
  hipLaunchKernelGGL((ch_tile_kernel<CH_LOGITS>), dim3((unsigned)qtiles, (unsigned)ntiles), dim3(FT_THREADS), 0, (hipStream_t)stream,
                     a, 1, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, Z);
  VSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t vsx_cls_ce_bwd_ws_bytes(int32_t B, int32_t H, int32_t C) {
  if (B < 1 || H < 4 || H % 4 || C < 1) return 0;
  const int64_t dz = ((int64_t)B * C + 3) / 4 * 4;
  return (dz + (int64_t)C * H + B) * 4;  // dZ [B, C] (rounded up to 16 bytes), the raw dW sums [C, H], the rows' dots [B]
}

extern "C" int32_t vsx_cls_ce_bwd(const float* h, const float* W, const int64_t* labels, const float* inv_h, const float* inv_w,
                                  const float* log_scale, const float* bias, const float* rows, const float* acc, const float* gout,
                                  int32_t B, int32_t H, int32_t C, float* dh, float* dW, float* dbias, float* dlog_scale, void* ws,
                                  int64_t ws_bytes, vsx_stream_t stream) {
  if (int rc = ch_range("vsx_cls_ce_bwd", B, H, C)) return rc;
  if (int rc = ch_operands("vsx_cls_ce_bwd", h, W, inv_h, inv_w, log_scale, bias)) return rc;
  VSX_CHECK(labels && rows && acc && gout && dh && dW && ws && vsx_al16(dh) && vsx_al16(dW),
            "vsx_cls_ce_bwd: null argument, or dh / dW not 16-byte aligned");
  const bool cosine = inv_h != nullptr;
  VSX_CHECK(cosine ? (dlog_scale && !dbias) : !dlog_scale, "vsx_cls_ce_bwd: cosine takes dlog_scale (no dbias), linear dbias or none");
  VSX_CHECK(ws_bytes >= vsx_cls_ce_bwd_ws_bytes(B, H, C) && vsx_al16(ws),
            "vsx_cls_ce_bwd: the workspace must be 16-byte aligned and hold vsx_cls_ce_bwd_ws_bytes = %ld bytes (got %ld)",
            (long)vsx_cls_ce_bwd_ws_bytes(B, H, C), (long)ws_bytes);
  const int qtiles = (B + FT_T - 1) / FT_T, ntiles = (C + FT_T - 1) / FT_T;
  float* dZ = (float*)ws;
  float* rawW = dZ + ((size_t)B * C + 3) / 4 * 4;
  float* tdot = rawW + (size_t)C * H;
  const ChArgs a = {h, W, labels, inv_h, inv_w, log_scale, bias, B, H, C};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL((ch_tile_kernel<CH_DZ>), dim3((unsigned)qtiles, (unsigned)ntiles), dim3(FT_THREADS), 0, s, a, 1, rows, acc, gout, dZ);
  const dim3 gh((unsigned)((B + CC_RB - 1) / CC_RB)), gw((unsigned)((C + CC_RB - 1) / CC_RB)), block(256);
  if (cosine) {
    hipLaunchKernelGGL((ch_contract_kernel<true>), gh, block, 0, s, (const float*)dZ, (long)C, 1L, B, C, H, W, inv_w, h, inv_h, log_scale,
                       dh, dh, 0, tdot, (float*)nullptr);
    hipLaunchKernelGGL((ch_contract_kernel<true>), gw, block, 0, s, (const float*)dZ, 1L, (long)C, C, B, H, h, inv_h, W, inv_w, log_scale,
                       rawW, dW, 1, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(ch_sum_add_kernel, dim3(1), dim3(256), 0, s, (const float*)tdot, B, dlog_scale);
  } else {
    hipLaunchKernelGGL((ch_contract_kernel<false>), gh, block, 0, s, (const float*)dZ, (long)C, 1L, B, C, H, W, (const float*)nullptr, h,
                       (const float*)nullptr, (const float*)nullptr, dh, dh, 0, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL((ch_contract_kernel<false>), gw, block, 0, s, (const float*)dZ, 1L, (long)C, C, B, H, h, (const float*)nullptr, W,
                       (const float*)nullptr, (const float*)nullptr, rawW, dW, 1, (float*)nullptr, dbias);
  }
  VSX_LAUNCH_CHECK();
  return 0;
}
