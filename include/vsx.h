/* vsx.h — C-ABI of libvsx.so: hand-written gfx950 (MI355X / CDNA4) kernels for the VisCy
 * UNeXt2 virtual-staining hot path (forward, backward, MixedLoss, normalisation, AdamW).
 *
 * The reference (mehta-lab/VisCy) has no FFI: every device op on this path is an ATen/cuDNN
 * call reached through torch.nn / timm / MONAI.  Each entry point
 * below names the reference op(s) it replaces (paths relative to /root/reference/packages).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a contiguous buffer owned by the caller
 *     (PyTorch caching allocator: tensor.data_ptr()); the library never allocates, frees,
 *     synchronises or changes device; kernels are enqueued on `stream`
 *     (torch.cuda.current_stream().cuda_stream) and are hipGraph-capturable.
 *   - `dtype`: VSX_F32 (0) = fp32 storage + exact-fp32 MFMA (parity mode),
 *              VSX_BF16 (1) = bf16 storage + bf16 MFMA, fp32 accumulation / statistics.
 *   - activations inside the trunk are channels-last: [B, H, W, C] ("pixel rows x channels").
 *   - return 0 on success; non-zero → vsx_last_error() (thread-local) has the message.
 *   - re-entrant; the only mutable global state is the set of kernel-selection flags behind vsx_set_flag (plain ints read at
 *     launch time: set them before launching from several threads, not while launches are in flight) and the thread-local
 *     error string.
 */
#ifndef VSX_H
#define VSX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vsx_stream_t; /* hipStream_t */

#define VSX_F32 0
#define VSX_BF16 1

int32_t vsx_version(void);
const char* vsx_last_error(void);
/* kernel template the last vsx_gemm_nt / vsx_gemm_tn call on this thread dispatched to: "gemm_nt_fast", "gemm_nt_generic",
 * "gemm_nt2" (both kernels of gemm_nt2.hip), "gemm_tn_fast", "gemm_tn_generic" ("" before the first call).  Measurement aid:
 * bench.py groups its live launch timings by kernel family with it. */
const char* vsx_last_kernel(void);
/* debug / A-B knobs: "tn_tr" (1 = ds_read_b64_tr_b16 fragments in the wgrad GEMM, default 1) */
int32_t vsx_set_flag(const char* name, int32_t value);
int32_t vsx_get_flag(const char* name);
/* vsx_set_flag("det_reduce", 1): the forward's per-sample sums (GRN sum of squares of the fused GRN-MLP passes and of gemm_nt's
 * GELU epilogue on the 256-row-tile kernel, InstanceNorm sum / sum of squares of vsx_head_conv_fwd) are formed in a fixed order
 * — per-workgroup partials in this caller-owned scratch (`floats` fp32 values, thread-local, used by the NEXT launches of this
 * thread; every launch checks the size and names what it needs), then one ordered pass — instead of by fp32 atomics, whose order
 * differs from run to run (timm GlobalResponseNorm / nn.InstanceNorm3d reduce deterministically on the CPU: reference behaviour
 * restated at viscy_models/unet/fcmae.py:174-221, components/heads.py:617-627).  NULL / 0 releases the scratch.
 * Lifetime: a launch writes through this pointer, and a launch captured into a hipGraph keeps the pointer it was recorded with —
 * the memory must stay allocated for as long as any graph captured under it may be replayed (viscy_amd.ops never frees it).
 * How much a launch wants: VsxGemmPlan.det_floats of vsx_gemm_plan, vsx_mlp_det_floats, vsx_head_conv_det_floats — each the
 * expression the launch itself checks against. */
int32_t vsx_det_workspace(float* ws, int64_t floats);
/* The same fixed-order sums for the launches of the CALLING THREAD only, whatever the process-wide flag says: vsx_det_scope(1)
 * opens the scope, and the call returns the previous value, so that vsx_det_scope(previous) closes it and scopes nest.
 * vsx_det_active: 1 where the det_reduce flag is set or the calling thread's scope is open — what every launch and the planner ask. */
int32_t vsx_det_scope(int32_t on);
int32_t vsx_det_active(void);

/* ---------------------------------------------------------------------------------------------
 * Operand "gather" description shared by the two GEMM kernels.  Row m of the logical
 * [M, K] operand is a pixel (b, y, x) of a gh x gw grid; K = ntaps * cs.
 *   VSX_A_ROWS   : plain row-major, K contiguous per row (ntaps = 1)
 *   VSX_A_PATCH2 : 2x2 stride-2 patch of a [B, 2gh, 2gw, cs] tensor  (k = (ky, kx, c))
 *   VSX_A_CONV3  : 3x3 zero-padded neighbourhood of a [B, gh, gw, *] tensor, cs channels
 *                  starting at coff                                   (k = (ky, kx, c))
 * --------------------------------------------------------------------------------------------- */
#define VSX_A_ROWS 0
#define VSX_A_PATCH2 1
#define VSX_A_CONV3 2

#define VSX_PRO_NONE 0
#define VSX_PRO_GRN 1 /* a = g * s[b, k] + beta[k]   (GRN applied on the fly to the stored activation g = gelu(h)) */

#define VSX_EPI_NONE 0
#define VSX_EPI_BIAS 1         /* c = acc + bias[n] */
#define VSX_EPI_BIAS_GELU_SQ 2 /* c = h = acc + bias; c2 = g = gelu(h); red0[b, n] += g^2     (fc1 + GRN pass A) */
#define VSX_EPI_BIAS_RES 3     /* c = acc + bias[n] + res[m, n]   (bias may be NULL)      (fc2 + residual)   */
#define VSX_EPI_DZ 4           /* c = dz = acc; red0[b, n] += dz * aux[m, n] (aux = g); red1[b, n] += dz  (fc2 dgrad) */
#define VSX_EPI_BIAS_STATS 5   /* c = acc + bias; red0[b, n] += c; red1[b, n] += c^2      (head conv + IN)   */
#define VSX_EPI_LN_BWD 6       /* c = rstd[m] * (d - mean_n(d) - xh * mean_n(d * xh)),  d = acc rounded to the storage type:
                                * the backward of an affine-free LayerNorm over the N columns applied to the GEMM result (fc1 data
                                * gradient + block LayerNorm backward in one launch).  aux = xh [M, ldx] (the normalised rows),
                                * grn_s = rstd [M] (fp32).  bf16, plain row operands, N <= 256, M % 256 == 0, K % 32 == 0 only
                                * (vsx_gemm_nt_ln_bwd_supported).  With grn_b = mean [M] non-NULL: aux holds the UN-normalised rows y
                                * (xh = bf16((y - mean) * rstd) is re-formed in the epilogue) and A is expected row-scaled by rstd
                                * (vsx_mlp_bwd_dh_ln), so c = d - mean_n(d) - xh * mean_n(d * xh) without the leading factor. */

typedef struct VsxGemm {
  /* C[M, N] = pro(A)[M, K] * B[N, K]^T  (vsx_gemm_nt)   |   W[N, K] += X[M, N]^T * pro(A)[M, K]  (vsx_gemm_tn) */
  const void* A; /* NT: left operand; TN: the "A-like" (gathered) operand Y[M, K] */
  const void* B; /* NT: weights [N, K], K contiguous, row stride ldb; TN: X[M, N], row stride ldb */
  void* C;       /* NT: output (dtype); TN: fp32 accumulation target [N, ldc] (atomicAdd) */
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  int32_t a_mode, gh, gw, cs;
  int32_t nz;           /* z-batch count (gridDim.z), 1 if unused */
  int32_t a_coff[8];    /* per-z channel offset into A rows */
  int32_t b_off[8];     /* per-z offset: NT → element offset into B; TN → column offset into X rows */
  int32_t c_coff[8];    /* per-z: NT → column offset into C rows; TN → element offset into W */
  int32_t c_mode;       /* NT only: VSX_A_ROWS or VSX_A_PATCH2 (scatter C rows back to 2x2 patches, n = (ky,kx,c)) */
  int32_t c_cs;         /* channels per tap for c_mode PATCH2 */
  int32_t pro;
  const float* grn_s;   /* [nb, K] */
  const float* grn_b;   /* [K] */
  int32_t hw;           /* rows per batch sample (b = m / hw) */
  int32_t epi;
  const float* bias;    /* [N] */
  const void* res;      /* [M, ldr] dtype */
  int32_t ldr;
  const void* aux;      /* [M, ldx] dtype (EPI_DZ: stored activation g) */
  int32_t ldx;
  float* red0;
  float* red1;
  float* colsum;        /* TN only: [N] += sum_m X[m, n] (bias gradient), may be NULL */
  void* C2;             /* NT, EPI_BIAS_GELU_SQ: second output g = gelu(h), same layout as C (C itself may be NULL then:
                           inference keeps only the activation) */
  int64_t b_bstride;    /* NT: element stride between PER-SAMPLE weight matrices B[b] (b = m / hw); 0 = one shared B.
                         * Needs hw % 128 == 0, plain row operands, N > 64, K % 32 == 0 (the lean instantiation). Used to
                         * fold the GRN scale into fc2: a·W2^T with a = g·s[b] + beta  ==  g·(W2·diag(s[b]))^T + W2·beta
                         * TN: element stride between PER-SAMPLE OUTPUT matrices C[b] (and colsum rows [b][N]): one product
                         * X_b^T·Y_b per sample of hw rows, plain stores (bf16, no prologue, hw % 64 == 0).  The block backward
                         * derives the fc2 weight gradient and the GRN statistics from these (vsx_grn_q_reduce) */
  const float* rscale;  /* NT, EPI_BIAS_RES: per-sample scale of the branch, c = (acc + bias) * rscale[m / hw] + res — stochastic
                         * depth (timm DropPath: 0 or 1 / keep_prob per sample), NULL = 1.  Needs hw > 0. */
} VsxGemm;

/* K5/K8/K9/K11/K13 (pointwise / patch / 3x3 convolutions as MFMA GEMMs) — replaces
 * nn.Linear / 1x1 nn.Conv2d inside timm GlobalResponseNormMlp, the 2x2-s2 downsample conv,
 * the decoder 1x1 projection (viscy_models/components/blocks.py:54-74) and the head Conv3d
 * (viscy_models/components/heads.py:617-625). */
int32_t vsx_gemm_nt(const VsxGemm* p, int32_t dtype, vsx_stream_t stream);
/* 1 if vsx_gemm_nt takes VSX_EPI_LN_BWD for this shape (otherwise: a plain vsx_gemm_nt followed by vsx_ln_bwd) */
int32_t vsx_gemm_nt_ln_bwd_supported(int64_t M, int32_t N, int32_t K, int32_t dtype);
/* weight-gradient GEMM (contraction over pixels) for the same layers */
int32_t vsx_gemm_tn(const VsxGemm* p, int32_t dtype, vsx_stream_t stream);

/* What vsx_gemm_nt / vsx_gemm_tn would launch for these parameters under the current flags, decided from the flags and the
 * fields of VsxGemm alone (pointer fields are only tested for NULL; no GPU is needed).  The numbers are the template arguments of
 * the kernel that runs, 0 where it has no such parameter. */
typedef struct VsxGemmPlan {
  const char* family;   /* what vsx_last_kernel reports after the launch */
  int32_t esize;        /* bytes per operand element: 2 (bf16) or 4 */
  int32_t tile[2];      /* output tile.  NT: rows x columns of C (BM x BN);  TN: tile N x tile K of W */
  int32_t step;         /* contraction depth per LDS stage.  NT: BK;  TN: pixel rows (0: the generic TN kernel) */
  int32_t nbuf;         /* LDS buffers / stages */
  int32_t pro_kind;     /* 0 none, 1 GRN prologue, 2 (TN) GRN prologue with the backward statistics */
  int32_t tr;           /* TN: transposing LDS reads */
  int32_t epi;          /* NT: VSX_EPI_* */
  int32_t grid[3], block;
  int32_t pro_bits;     /* kernel-side flag bits the launch ORs into VsxGemm.pro */
  int64_t zero_c, zero_colsum; /* TN: floats of C / colsum zero-filled before the launch (per-sample outputs in several splits) */
  int64_t det_floats;   /* NT: workspace floats of the fixed-order sums (det_reduce), 0 = none */
} VsxGemmPlan;
#define VSX_GEMM_NT 0
#define VSX_GEMM_TN 1
/* 0 and *out filled, or the return code and vsx_last_error of the launch that would be refused */
int32_t vsx_gemm_plan(int32_t kind, const VsxGemm* p, int32_t dtype, VsxGemmPlan* out);


/* =============================================================================================
 * Remaining entry points (one per fused kernel of the path).  `ws` arguments are caller-owned fp32
 * scratch for two-stage reductions (per-block partials + a fold kernel): same-address global atomics
 * serialise at ~0.2 us each on MI355X, so no kernel issues more than a few dozen per address.
 * ============================================================================================= */

/* K3 depthwise 7x7 conv — timm ConvNeXtBlock.conv_dw = nn.Conv2d(C, C, 7, padding=3, groups=C) (block math restated in-repo at
 * viscy_models/unet/fcmae.py:174-221).  x,y: [B,H,W,C] channels-last; w: tap-major fp32 [49][C]; y = conv(x) + bias [+ add]. */
int32_t vsx_dwconv7_fwd(const void* x, const float* w, const float* bias, const void* add, void* y,
    int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, vsx_stream_t stream);

/* data gradient of K3: dx = conv(dy, flipped w) [+ add]; add = gradient arriving through the residual branch. */
int32_t vsx_dwconv7_bwd_data(const void* dy, const float* w, const void* add, void* dx, int32_t B, int32_t H,
    int32_t W, int32_t C, int32_t dtype, vsx_stream_t stream);

/* weight/bias gradient of K3 accumulated into dw[49][C], db[C] (fp32).  ws: caller-owned workspace of ws_rows*50*C floats. */
int32_t vsx_dwconv7_bwd_weight(const void* dy, const void* x, float* dw, float* db, float* ws,
    int32_t ws_rows, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, vsx_stream_t stream);

/* K12 direct: the head's 3x3x3 Conv3d (MONAI Convolution conv, viscy_models/components/heads.py:607-616) as LDS-tiled MFMA
 * kernels for the production shape — bf16, C3 = 8 -> Cmid = 32, 5 output planes, H2 and W2 multiples of 16
 * (vsx_head_conv_supported tells; everything else runs through vsx_gemm_nt / vsx_gemm_tn with VSX_A_CONV3).
 * hin [B*H2*W2, 7*8], U / dU [B*H2*W2, 5*32], Wc [32][27*8] (k = ((dy*3+dx)*3+dz)*8 + c, the prepared conv weight),
 * ssum / ssq [B,32] += InstanceNorm statistics of the stored U, dW fp32 [32][216] += , db fp32 [32] += (may be NULL),
 * Wp: 45*2*64*8 bf16 packed by vsx_head_conv_dgrad_prep from Wc. */
int32_t vsx_head_conv_supported(int32_t H2, int32_t W2, int32_t c3, int32_t cmid, int32_t zo, int32_t dtype);
/* vsx_det_workspace floats that vsx_head_conv_fwd wants while vsx_det_active(): 64 partials per workgroup (0: shape not served) */
int64_t vsx_head_conv_det_floats(int32_t B, int32_t H2, int32_t W2);
int32_t vsx_head_conv_fwd(const void* hin, const void* Wc, const float* bias, void* U, float* ssum, float* ssq,
    int32_t B, int32_t H2, int32_t W2, int32_t c3, int32_t cmid, int32_t zo, int32_t dtype, vsx_stream_t stream);
int32_t vsx_head_conv_wgrad(const void* hin, const void* dU, float* dW, float* db, int32_t B, int32_t H2, int32_t W2,
    int32_t c3, int32_t cmid, int32_t zo, int32_t dtype, vsx_stream_t stream);
int32_t vsx_head_conv_dgrad_prep(const void* Wc, void* Wp, int32_t dtype, vsx_stream_t stream);
int32_t vsx_head_conv_dgrad(const void* dU, const void* Wp, void* dhin, int32_t B, int32_t H2, int32_t W2, int32_t c3,
    int32_t cmid, int32_t zo, int32_t dtype, vsx_stream_t stream);

/* FCMAE head: viscy_models.components.heads.PixelToVoxelShuffleHead (heads.py:656-685) = MONAI UpSample(pixelshuffle, scale s,
 * pre_conv None, apply_pad_pool) + reshape: feat [B*h*w, Cout*D*s*s] (dtype) <-> out / dout fp32 (B, Cout, D, s*h, s*w). */
int32_t vsx_voxel_shuffle_fwd(const void* feat, float* out, int32_t B, int32_t h, int32_t w, int32_t Cout, int32_t D,
    int32_t s, int32_t pool, int32_t dtype, vsx_stream_t stream);
int32_t vsx_voxel_shuffle_bwd(const float* dout, void* dfeat, int32_t B, int32_t h, int32_t w, int32_t Cout, int32_t D,
    int32_t s, int32_t pool, int32_t dtype, vsx_stream_t stream);

/* Narrow-channel family (csrc/narrow.hip): the 2x2-stem FCMAE (VSCyto2D).  Every reduction writes per-workgroup fp32 partials into
 * `ws` (vsx_narrow_ws_floats(op, B, n, C, K) floats: n = pixels per sample for the block passes, rows M for the projection and the
 * stem; C = channels (C0 for the stem); K = stem patch size / concatenated width) and sums them in a fixed order: the same bits from
 * run to run.  Gradient outputs are ACCUMULATED (+=).  Block passes: C in {4, 8}, maps [B*H*W, C] channels-last, dtype storage,
 * W1f [4C, C] / W2 [C, 4C] in dtype (the prepared fc operands, LayerNorm affine folded into fc1), everything else fp32. */
#define VSX_NARROW_STEM 0
#define VSX_NARROW_PROJ 1
#define VSX_NARROW_FWD1 2
#define VSX_NARROW_BWD_A 3
#define VSX_NARROW_BWD_B 4
#define VSX_NARROW_BWD_C 5
int64_t vsx_narrow_ws_floats(int32_t op, int32_t B, int64_t n, int32_t C, int32_t K);
/* stem, Z == kz: out[b*h*w, C0] = bias + W [C0, Cin*kz*ky*kx] . patch(x), x fp32 (B, Cin, Z, H, W) read directly */
int32_t vsx_narrow_stem_fwd(const float* x, const float* W, const float* bias, void* out, int32_t B, int32_t Cin, int32_t Z,
    int32_t H, int32_t Wd, int32_t kz, int32_t ky, int32_t kx, int32_t C0, int32_t dtype, vsx_stream_t stream);
/* dW [C0, K] += df^T . patch(x), db [C0] += column sums of df */
int32_t vsx_narrow_stem_wgrad(const float* x, const void* df, float* dW, float* db, float* ws, int64_t ws_floats, int32_t B,
    int32_t Cin, int32_t Z, int32_t H, int32_t Wd, int32_t kz, int32_t ky, int32_t kx, int32_t C0, int32_t dtype, vsx_stream_t stream);
/* out [M, C] = bp + Wp [C, Ccat] . (LN(cat) * gamma + beta), LN over the Ccat channels of a row (eps); mean / rstd [M] fp32 */
int32_t vsx_narrow_proj_fwd(const void* cat, const float* gamma, const float* beta, const float* Wp, const float* bp, void* out,
    float* mean, float* rstd, int64_t M, int32_t Ccat, int32_t C, float eps, int32_t dtype, vsx_stream_t stream);
/* dxn [M, Ccat] = dout . Wp (gradient of the normalised affine rows); dW += dout^T . xn (xn re-formed from cat, mean, rstd);
 * db += column sums of dout */
int32_t vsx_narrow_proj_bwd(const void* dout, const void* cat, const float* mean, const float* rstd, const float* gamma,
    const float* beta, const float* Wp, void* dxn, float* dW, float* db, float* ws, int64_t ws_floats, int64_t M, int32_t Ccat,
    int32_t C, int32_t dtype, vsx_stream_t stream);
/* block pass 1: y = dwconv7(x; dw_w [49, C], dw_b) (stored), colsq [B, 4C] += per-sample sum of gelu(fc1(LN(y)))^2 */
int32_t vsx_narrow_block_fwd1(const void* x, const float* dw_w, const float* dw_b, const void* W1f, const float* b1f, void* y,
    float* colsq, float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C, int32_t dtype, vsx_stream_t stream);
/* block pass 2: out = fc2(gelu(fc1(LN(y))) * s[b] + grn_b) + b2 + x */
int32_t vsx_narrow_block_fwd2(const void* y, const void* x, const void* W1f, const float* b1f, const float* s, const float* grn_b,
    const void* W2, const float* b2, void* out, int32_t B, int32_t H, int32_t Wd, int32_t C, int32_t dtype, vsx_stream_t stream);
/* backward A: dW2 += dout^T z, db2 += sum dout, P [B, 4C] += per-sample sum dz * g, S [B, 4C] += per-sample sum dz (dz = dout . W2) */
int32_t vsx_narrow_block_bwd_a(const void* dout, const void* y, const void* W1f, const float* b1f, const float* s, const float* grn_b,
    const void* W2, float* dW2, float* db2, float* P, float* S, float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd,
    int32_t C, int32_t dtype, vsx_stream_t stream);
/* backward B: dh = (dz * s + t * g) * gelu'(h); dy = LayerNorm backward of dh . W1f (stored); dW1f [4C, C] += dh^T xh, db1f += sum dh */
int32_t vsx_narrow_block_bwd_b(const void* dout, const void* y, const void* W1f, const float* b1f, const float* s, const float* t,
    const void* W2, void* dy, float* dW1f, float* db1f, float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C,
    int32_t dtype, vsx_stream_t stream);
/* backward C: dx = dwconv7 adjoint of dy + dout (shortcut); ddw [49, C] += 7x7 weight gradient, ddb [C] += sum dy */
int32_t vsx_narrow_block_bwd_c(const void* dy, const void* x, const void* dout, const float* dw_w, void* dx, float* ddw, float* ddb,
    float* ws, int64_t ws_floats, int32_t B, int32_t H, int32_t Wd, int32_t C, int32_t dtype, vsx_stream_t stream);
/* vsx_voxel_shuffle_bwd for any Cout*D*s*s (one element per thread: the pre-training head's 4 channels in bf16) */
int32_t vsx_narrow_voxel_shuffle_bwd(const float* dout, void* dfeat, int32_t B, int32_t h, int32_t w, int32_t Cout, int32_t D,
    int32_t s, int32_t pool, int32_t dtype, vsx_stream_t stream);

/* out[m, :] = x[m, :] * scale[m / hw]  (rows of C elements, dtype): the gradient of a stochastic-depth branch
 * (timm DropPath in the ConvNeXt blocks, `drop_path_rate` / `encoder_drop_path_rate` of the reference models). */
int32_t vsx_scale_rows_samples(const void* x, const float* scale, void* out, int64_t M, int32_t C, int32_t hw, int32_t dtype,
    vsx_stream_t stream);

/* FCMAE masked pre-training.  masked_patchify / masked_unpatchify / `x *= unmasked`
 * (viscy_models/unet/fcmae.py:95-141,216-226) on channels-last row matrices, as one row permutation:
 *   dst[r,:] = map[r] >= 0 ? src[map[r],:] (+ add[r,:] when add != NULL) : 0        r < n_out; rows of C elements (dtype)
 * gather: map = dense row per kept token; scatter: map = compact row per dense row or -1 (zero fill); mask: map[r] = r or -1. */
int32_t vsx_rows_select(const void* src, const int32_t* map, const void* add, void* dst, int64_t n_out, int32_t C,
    int32_t dtype, vsx_stream_t stream);

/* cytoland.engine.MaskedMSELoss.forward (applications/cytoland/src/cytoland/engine.py:104-125):
 *   loss = sum(mask * mean_z (pred - orig)^2) / sum(mask);  pred / orig fp32 (B,C,Z,H,W), mask uint8 (B,1,H,W), H*W % 4 == 0.
 * acc: 2 floats of scratch kept for the backward {sum mask*(p-o)^2, sum(mask)}; dpred = gout * d loss / d pred. */
int32_t vsx_masked_mse_fwd(const float* pred, const float* orig, const uint8_t* mask, float* acc, float* loss, int32_t B,
    int32_t C, int32_t Z, int64_t HW, vsx_stream_t stream);
int32_t vsx_masked_mse_bwd(const float* pred, const float* orig, const uint8_t* mask, const float* acc, const float* gout,
    float* dpred, int32_t B, int32_t C, int32_t Z, int64_t HW, vsx_stream_t stream);

/* viscy_utils.losses.SpotlightLoss.forward (packages/viscy-utils/src/viscy_utils/losses/spotlight.py:161-225) on `rows` = B*C
 * contiguous rows of n = Z*Y*X voxels:
 *   m = mask weight;  d = p - t;  s = clamp((p - k p) / (k - 2k|p| + 1), 0, 1)
 *   F = sum m, Em = sum m d^2, E = sum d^2, S = sum s, I = sum s m                                     (per row)
 *   mse_r = F > 0 ? Em / (F + eps) : E / n;  dice_r = 1 - 2 I / (S + F + eps);  real_r = 0 < F < n
 *   loss = lambda_mse * mean_r mse_r + (1 - lambda_mse) * (n_real > 0 ? sum_r real_r dice_r / n_real : 0)
 * pred: fp32 or bf16 (dtype), read as stored; target fp32.  mask_mode selects m: VSX_SPOTLIGHT_THRESHOLD m = t >= thr[row]
 * (thr: `rows` floats on the device: a fixed threshold repeated, or vsx_otsu_threshold's; mask unused), VSX_SPOTLIGHT_MASK_U8
 * m = (float)byte of a uint8 / bool mask, VSX_SPOTLIGHT_MASK_F32 m = an fp32 weight (thr unused).  Row starts may have any
 * alignment (odd n); 16-byte loads are used where all array bases are 16-byte aligned.
 * One workgroup sums one chunk of VSX_SPOTLIGHT_CHUNK voxels of one row and stores its five partial sums into ws (plain stores,
 * every word written before it is read: ws needs no initialisation); the finalise kernel folds them in float64 in a fixed
 * order, so loss and gradient are bit-identical from run to run.  ws: vsx_spotlight_workspace(VSX_SPOTLIGHT_WS_FWD, rows, n)
 * bytes, 8-byte aligned.  loss: 1 float.  coef: 4 floats per row {a, b, c, e}, kept for the backward:
 *   dpred = gout[0] * (d * (a m + b) + s' * (c m + e)),   s' = (1 - k^2) / (k - 2k|p| + 1)^2 on 0 <= p <= 1, else 0
 * (dpred in pred's dtype; gout: 1 float on the device). */
#define VSX_SPOTLIGHT_CHUNK 16384
#define VSX_SPOTLIGHT_THRESHOLD 0
#define VSX_SPOTLIGHT_MASK_U8 1
#define VSX_SPOTLIGHT_MASK_F32 2
#define VSX_SPOTLIGHT_WS_FWD 0
#define VSX_SPOTLIGHT_WS_OTSU 1
int64_t vsx_spotlight_workspace(int32_t op, int64_t rows, int64_t n);
int32_t vsx_spotlight_fwd(const void* pred, int32_t dtype, const float* target, const void* mask, int32_t mask_mode,
    const float* thr, int64_t rows, int64_t n, double lambda_mse, double sigmoid_k, double eps, void* ws, float* loss,
    float* coef, vsx_stream_t stream);
int32_t vsx_spotlight_bwd(const void* pred, int32_t dtype, const float* target, const void* mask, int32_t mask_mode,
    const float* thr, const float* coef, const float* gout, void* dpred, int64_t rows, int64_t n, double sigmoid_k,
    vsx_stream_t stream);
/* Otsu threshold of each of `rows` contiguous rows of n fp32 values (spotlight.py:50-110): row min / max, an n_bins-bin
 * histogram (2 <= n_bins <= 1024; bin = min((int)((x - lo) * n_bins / (hi - lo)), n_bins - 1) in fp32, integer counts), the
 * reference's inter-class variance on cumulative counts and means in float64, first maximum; thr[row] = the centre of that bin,
 * lo + (idx + 0.5) * (hi - lo) / n_bins, or lo for a constant row.  ws: vsx_spotlight_workspace(VSX_SPOTLIGHT_WS_OTSU, rows, n)
 * bytes, 4-byte aligned, no initialisation needed. */
int32_t vsx_otsu_threshold(const float* target, float* thr, void* ws, int64_t rows, int64_t n, int32_t n_bins,
    vsx_stream_t stream);

/* ConvNeXt-V1 layer scale (timm ConvNeXtBlock.gamma, ls_init_value 1e-6; the `convnext_tiny` trunk of
 * viscy_models.contrastive.ContrastiveEncoder, encoder.py:93-99) folded into the block's second pointwise layer:
 * Ws = diag(gamma) W [R,K], bs = gamma * b; unfold ADDS dW += diag(gamma) dWs, db += gamma dbs,
 * dgamma += rowsum(dWs * W) + dbs * b.  fp32. */
int32_t vsx_layer_scale_fold(const float* W, const float* b, const float* gamma, float* Ws, float* bs, int32_t R, int32_t K,
    vsx_stream_t stream);
int32_t vsx_layer_scale_unfold(const float* dWs, const float* dbs, const float* W, const float* b, const float* gamma,
    float* dW, float* db, float* dgamma, int32_t R, int32_t K, vsx_stream_t stream);

/* DynaCLR contrastive path: tail of viscy_models.contrastive.ContrastiveEncoder
 * (packages/viscy-models/src/viscy_models/contrastive/encoder.py:93-154) behind the ConvNeXt trunk.
 * Global average pool of a channels-last feature map x [B*hw, C] (dtype) -> out [B, C] fp32 (timm head.global_pool) and
 * its transpose. */
int32_t vsx_avgpool_rows_fwd(const void* x, float* out, int32_t B, int32_t hw, int32_t C, int32_t dtype, vsx_stream_t stream);
int32_t vsx_avgpool_rows_bwd(const float* dout, void* dx, int32_t B, int32_t hw, int32_t C, int32_t dtype, vsx_stream_t stream);
/* nn.BatchNorm1d on [B, F] fp32 (projection MLP, encoder.py:115-121), optional fused ReLU.  training != 0: batch
 * statistics, running_{mean,var} updated in place (momentum, unbiased variance); else the running statistics normalise.
 * save_{mean,rstd} [F] feed the backward, which ADDS into dw / db. */
int32_t vsx_bn1d_fwd(const float* x, const float* w, const float* b, float* running_mean, float* running_var, float* y,
    float* save_mean, float* save_rstd, int32_t B, int32_t F, float eps, float momentum, int32_t training, int32_t relu,
    vsx_stream_t stream);
int32_t vsx_bn1d_bwd(const float* dy, const float* x, const float* y, const float* w, const float* save_mean,
    const float* save_rstd, float* dx, float* dw, float* db, int32_t B, int32_t F, int32_t training, int32_t relu,
    vsx_stream_t stream);
/* viscy_models.contrastive.loss.NTXentLoss / NTXentHCL (loss.py:20-186; pytorch-metric-learning pair semantics):
 * E [N, D] fp32 embeddings, labels [N]; equal labels = positive pairs, different labels = negatives; cosine similarity;
 * beta = 0: NT-Xent, beta > 0: hard-negative re-weighting.  Scratch owned by the caller: En [N,D], inv [N], S [N,N],
 * dS [N,N], rows [2N]; acc [2] = {loss, number of positive pairs}.  vsx_ntxent_bwd: dE = gout * d loss / d E. */
int32_t vsx_ntxent_fwd(const float* E, const int32_t* labels, float* En, float* inv, float* S, float* dS, float* rows, float* acc,
    int32_t N, int32_t D, float temperature, float beta, vsx_stream_t stream);
int32_t vsx_ntxent_bwd(const float* dS, const float* En, const float* inv, const float* acc, const float* gout, float* dE,
    int32_t N, int32_t D, vsx_stream_t stream);
/* torch.nn.TripletMarginLoss(margin, p = 2, eps, swap = False), the default loss of dynaclr.engine.ContrastiveModule
 * (engine.py:39-41), with the per-row similarities its _log_metrics reports (engine.py:135-146).  A, P, N [B, D] fp32.
 * rows [B, 5] = {d_ap, d_an, hinge, cos_ap, cos_an} per row: d = F.pairwise_distance (eps added to the difference),
 * hinge = max(d_ap - d_an + margin, 0), cos = F.cosine_similarity.  acc [6] = {loss, mean cos_ap, mean d_ap, mean cos_an,
 * mean d_an, share of rows with hinge > 0}, summed in a fixed order (bit-identical from run to run).  reduction: 0 = mean,
 * 1 = sum.  vsx_triplet_bwd: dA, dP, dN [B, D] = gout[0] * d loss / d (A, P, N); rows without hinge get exact zeros. */
int32_t vsx_triplet_fwd(const float* A, const float* P, const float* N, float* rows, float* acc, int32_t B, int32_t D,
    float margin, float eps, int32_t reduction, vsx_stream_t stream);
int32_t vsx_triplet_bwd(const float* A, const float* P, const float* N, const float* rows, const float* gout, float* dA,
    float* dP, float* dN, int32_t B, int32_t D, float margin, float eps, int32_t reduction, vsx_stream_t stream);

/* K13 (norm+act) + K14: MONAI Convolution ADN (InstanceNorm3d eps 1e-5 → PReLU) → nn.Conv3d(mid, 4*out, 1) → transpose /
 * nn.PixelShuffle(2) / transpose (viscy_models/components/heads.py:617-625,638-641).  U: [B,H2,W2,Z,Cmid] conv output;
 * ssum/ssq: [B,Cmid] from the conv GEMM epilogue (VSX_EPI_BIAS_STATS); out: (B, Cout, Z, 2*H2, 2*W2) fp32. */
int32_t vsx_head_out_fwd(const void* U, const float* ssum, const float* ssq, const float* w2,
    const float* b2, const float* alpha, float* out, int32_t B, int32_t H2, int32_t W2, int32_t Z, int32_t Cmid,
    int32_t Cout, float eps, int32_t dtype, vsx_stream_t stream);

/* backward pass 1 of the head tail: writes act = PReLU(IN(U)) and dv (gathered output gradient) for the 1x1x1 weight-gradient GEMM;
 * accumulates S1 = Σ dn, S2 = Σ dn·n̂ per (b, channel) and the PReLU slope gradient. */
int32_t vsx_head_out_bwd1(const void* U, const float* ssum, const float* ssq, const float* w2,
    const float* alpha, const float* dout, void* act, void* dv, float* S1, float* S2, float* dalpha, int32_t B,
    int32_t H2, int32_t W2, int32_t Z, int32_t Cmid, int32_t Cout, float eps, int32_t dtype,
    vsx_stream_t stream);

/* backward pass 1 with the weight gradient of the 1x1x1 convolution folded in (bf16 only; replaces vsx_head_out_bwd1 +
 * the vsx_gemm_tn over act/dv = autograd of nn.Conv3d(mid, 4*out, 1), heads.py:617-625): act is never materialised, the
 * contraction over the voxels runs on MFMA inside the kernel.  dW2 [4*Cout, Cmid] and db2 [4*Cout] are ACCUMULATED into;
 * scratch: B * (4*Cout*Cmid + 4*Cout) floats (zeroed here).  dv, S1, S2, dalpha as vsx_head_out_bwd1. */
int32_t vsx_head_out_bwd1_wgrad(const void* U, const float* ssum, const float* ssq, const float* w2,
    const float* alpha, const float* dout, void* dv, float* S1, float* S2, float* dalpha, float* dW2, float* db2,
    float* scratch, int32_t B, int32_t H2, int32_t W2, int32_t Z, int32_t Cmid, int32_t Cout, float eps, int32_t dtype,
    vsx_stream_t stream);

/* backward pass 2: dU = rstd * (dn - S1/cnt - n̂ * S2/cnt)  (InstanceNorm3d backward). */
int32_t vsx_head_out_bwd2(const void* U, const float* ssum, const float* ssq, const float* w2,
    const float* alpha, const void* dv, const float* S1, const float* S2, void* dU, int32_t B, int32_t H2,
    int32_t W2, int32_t Z, int32_t Cmid, int32_t Cout, float eps, int32_t dtype, vsx_stream_t stream);

/* avg_pool3d(·,(1,2,2)) of preds/target (viscy_utils/evaluation/metrics.py:340-341), target.max() of the INPUT planes (metrics.py:298) and the
 * L1 / L2 sums of MixedLoss (viscy_utils/losses/mixed_loss.py:58-63) in one pass.  tmax must be pre-set to -inf. */
int32_t vsx_loss_pool(const float* P, const float* T, float* Po, float* To, float* tmax, float* l1sum,
    float* l2sum, int32_t planes, int32_t H, int32_t W, vsx_stream_t stream);

/* one scale of ssim_25d (metrics.py:174-305): per-sample sums of the SSIM and contrast-sensitivity maps, bf16 rounding points as in
 * _compute_ssim_and_cs_bf16 (metrics.py:243-255). */
int32_t vsx_ssim_scale_fwd(const float* P, const float* T, const float* tmax, float* sum_ssim, float* sum_cs,
    int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, vsx_stream_t stream);

/* backward of one scale (+ pooled-gradient chain from the next scale, + L1/L2 gradient at scale 0); gout: device scalar (upstream gradient) or NULL = 1. */
int32_t vsx_ssim_scale_bwd(const float* P, const float* T, const float* tmax, const float* coef, float* dmu,
    const float* dPnext, float* dP, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, float l1c, float l2c,
    const float* gout, int32_t has_ssim, vsx_stream_t stream);

/* ms_ssim_25d combination with clamp(min=1e-4) (metrics.py:326-349) + MixedLoss weights (mixed_loss.py:56-69); writes loss, MS-SSIM and the per-(scale, sample) map-pixel gradients. */
/* Training variant of the two calls above with one pass over the stack less: vsx_ssim_scale_fwd_dmu = the sums of
 * vsx_ssim_scale_fwd plus the UNSCALED gradient field dmu [3][B*C][H-10][W-10] of this scale (last != 0: the SSIM map, else
 * the contrast map — what ms_ssim_25d uses of it, metrics.py:326-349), kept by the caller; vsx_ssim_scale_bwd_in = the
 * second half of vsx_ssim_scale_bwd, applying this scale's per-sample coef [B][2] (vsx_loss_finalize) to the stored field. */
int32_t vsx_ssim_scale_fwd_dmu(const float* P, const float* T, const float* tmax, float* sum_ssim, float* sum_cs, float* dmu,
                               int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, int32_t last, vsx_stream_t stream);
int32_t vsx_ssim_scale_bwd_in(const float* P, const float* T, const float* dmu, const float* coef, const float* dPnext,
                              float* dP, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, float l1c, float l2c,
                              const float* gout, int32_t has_ssim, int32_t last, vsx_stream_t stream);
/* One-pass training forward of a scale: vsx_ssim_scale_fwd_dmu + the vsx_loss_pool pass of the NEXT scale (pooled stacks Po / To,
 * their data range tmax_next, and with l1sum != NULL this scale's L1 / L2 sums) from the same reads of P / T; tmax[0] must be
 * final (vsx_loss_tmax for scale 0).  tmax, tmax_next, l1sum, l2sum are SLOTTED here: VSX_LOSS_SLOTS partial values,
 * VSX_LOSS_SLOT_STRIDE floats apart (range = their max, sums = their sum; vsx_loss_finalize takes sum_slots = VSX_LOSS_SLOTS).
 * Reference: metrics.py:272-305 + 340-341, mixed_loss.py:58-63. */
#define VSX_LOSS_SLOTS 64        /* partial accumulators per scalar of the one-pass forward (same-address atomics serialise) */
#define VSX_LOSS_SLOT_STRIDE 32  /* floats between two slots (one 128-byte line each) */
int32_t vsx_loss_tmax(const float* T, int64_t n, float* tmax, vsx_stream_t stream);
int32_t vsx_ssim_scale_fwd_fused(const float* P, const float* T, const float* tmax, float* sum_ssim, float* sum_cs, float* dmu,
                                 float* Po, float* To, float* tmax_next, float* l1sum, float* l2sum, int32_t B, int32_t C,
                                 int32_t D, int32_t H, int32_t W, int32_t last, vsx_stream_t stream);
int32_t vsx_loss_finalize(const float* sum_ssim, const float* sum_cs, const float* l1sum, const float* l2sum,
    const float* npix, float nelem, int32_t B, int32_t nscale, int32_t sum_slots, float a1, float a2, float a3,
    const float* gout, float* loss, float* coef, float* ms_out, vsx_stream_t stream);  /* sum_slots: 0 / 1 = l1sum, l2sum are scalars (vsx_loss_pool); VSX_LOSS_SLOTS = slotted (vsx_ssim_scale_fwd_fused) */

/* K2/K4: timm LayerNorm2d / nn.LayerNorm over channels, eps 1e-6 (reached via timm ConvNeXtStage / ConvNeXtBlock at viscy_models/unet/unext2.py:79,
 * viscy_models/components/blocks.py:60-69).  gamma == NULL → no affine (the block LN's affine is folded into fc1). */
int32_t vsx_ln_fwd(const void* x, void* y, float* mean, float* rstd, const float* gamma, const float* beta,
    int32_t rows, int32_t C, float eps, int32_t dtype, vsx_stream_t stream);

/* LayerNorm backward: x̂ = mean ? (x-mean)*rstd : x; dx = rstd*(g - mean(g) - x̂*mean(g*x̂)) [+ add], g = dy*gamma; dgamma/dbeta accumulated. */
int32_t vsx_ln_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
    const void* add, void* dx, float* dgamma, float* dbeta, int32_t rows, int32_t C, int32_t dtype,
    vsx_stream_t stream);

/* K7: timm GlobalResponseNorm statistics: s[b,n] = 1 + gamma[n]*g/(mean_n g + eps), g = sqrt(colsq[b,n]); colsq comes from the fc1 GEMM epilogue. */
int32_t vsx_grn_scale(const float* colsq, const float* gamma, float* s, int32_t nb, int32_t N, float eps,
    vsx_stream_t stream);

/* backward of the GRN statistics path: P[b,n] = Σ_hw dz*g, Sb[b,n] = Σ_hw dz → t[b,n] (factor of g in dG), dgamma, dbeta
 * (both ADDED to).  rowst: nb*N floats of scratch (per-sample dgamma contributions, column-reduced by a second launch).
 * dgamma == NULL (then Sb, dbeta NULL too): only t and rowst are produced, the caller reduces rowst / its Sb over the samples
 * itself (VSX_WTASK_REDUCE_ROWS jobs of vsx_weight_tasks). */
int32_t vsx_grn_bwd_stats(const float* colsq, const float* P, const float* Sb, const float* gamma, float* t,
    float* dgamma, float* dbeta, float* rowst, int32_t nb, int32_t N, float eps, vsx_stream_t stream);

/* K6/K7 backward, elementwise pass: dh = (dz*s + gelu(h)*t) * gelu'(h) written over dz; colsum[n] += Σ_m dh.  ws: ws_rows*N floats. */
int32_t vsx_grn_gelu_bwd(void* dz, const void* h, const float* s, const float* t, float* colsum, float* ws,
    int32_t ws_rows, int32_t M, int32_t N, int32_t hw, int32_t dtype, vsx_stream_t stream);

/* K26: torch.optim.AdamW step (viscy_utils/optimizers.py:50) on flat fp32 buffers; hyper = device array
 * {lr, beta1, beta2, eps, weight_decay, 1-beta1^t, 1-beta2^t, grad_scale} so the launch is hipGraph-replayable. */
int32_t vsx_adamw(float* p, const float* g, float* m, float* v, const float* hyper, int64_t n,
    vsx_stream_t stream);

/* Fused GRN-MLP of a ConvNeXt-V2 block (timm ConvNeXtBlock as called from viscy_models/unet/unext2.py:79; math restated at
 * viscy_models/unet/fcmae.py:174-221), bf16: the 4C-wide hidden activation never leaves the CU (csrc/mlp.hip).
 *   vsx_mlp_supported : 1 when a fused instantiation exists for (C, pixels per sample hw, rows M, dtype)
 *   vsx_mlp_image_bytes / vsx_mlp_pack : fragment-major LDS image of the prepared weights W1' [4C, C] (LayerNorm affine folded)
 *                       and W2 [C, 4C] (both bf16, row-major as vsx_prep_weight writes them)
 *   vsx_mlp_fwd mode 0: colsq[b, 4C] += sum_hw gelu(fc1(xh))^2   (GRN statistics; nothing else is stored)
 *               mode 1: out = res + rscale[b] * (fc2(gelu(fc1(xh)) * s[b] + beta) + b2) */
int32_t vsx_mlp_supported(int32_t C, int32_t hw, int64_t M, int32_t dtype);   /* the inference pair (modes 0 and 1) */
/* vsx_det_workspace floats that a statistics pass (mode 0: vsx_mlp_fwd, 2 / 6: vsx_mlp_fc1 with / without h) wants while
 * vsx_det_active(): one row of 4C column sums per workgroup (0: not a statistics mode, or the shape is not served) */
int64_t vsx_mlp_det_floats(int32_t C, int32_t hw, int64_t M, int32_t mode);
int32_t vsx_mlp_mode_supported(int32_t C, int32_t hw, int64_t M, int32_t mode, int32_t dtype);  /* one pass (mode 0..7) */
int64_t vsx_mlp_image_bytes(int32_t C);
int32_t vsx_mlp_pack(const void* W1, const void* W2, void* img, int32_t C, vsx_stream_t stream);
/* vsx_mlp_fwd / vsx_mlp_fc1 with the block LayerNorm (eps, no affine) applied in the kernel's prologue: y = the UN-normalised
 * rows (output of the depthwise convolution).  Modes 0 / 1: the normalised rows never exist in memory; vsx_mlp_fc1_ln also
 * writes them (xh_out [M, C]) and rstd_out [M] for the backward — or, with xh_out = NULL and mean_out [M] non-NULL, only the
 * two row statistics (the backward then re-normalises y: vsx_mlp_bwd_dh_ln).  Replaces vsx_ln_fwd + vsx_mlp_fwd / vsx_mlp_fc1. */
int32_t vsx_mlp_fwd_ln(const void* y, float eps, const void* wimg, const float* b1, const float* grn_s, const float* grn_b,
    const float* b2, const void* res, const float* rscale, void* out, float* colsq, const float* gtab, int64_t M, int32_t C,
    int32_t hw, int32_t mode, int32_t dtype, vsx_stream_t stream);
int32_t vsx_mlp_fc1_ln(const void* y, float eps, void* xh_out, float* rstd_out, float* mean_out, const void* wimg, const float* b1,
    float* colsq, const float* gtab, void* h, void* g, int64_t M, int32_t C, int32_t hw, int32_t dtype, vsx_stream_t stream);
int32_t vsx_mlp_fwd(const void* xh, const void* wimg, const float* b1, const float* grn_s, const float* grn_b, const float* b2,
    const void* res, const float* rscale, void* out, float* colsq, const float* gelu_table, int64_t M, int32_t C, int32_t hw,
    int32_t mode, int32_t dtype, vsx_stream_t stream);
/* training fc1 on the same kernel: h = bf16(xh . W1'^T + b1) and g = bf16(gelu(h)) stored ([M, 4C] each), colsq[b, 4C] +=
 * sum_hw g^2 — the outputs of vsx_gemm_nt with VSX_EPI_BIAS_GELU_SQ */
int32_t vsx_mlp_fc1(const void* xh, const void* wimg, const float* b1, float* colsq, const float* gelu_table, void* h, void* g,
    int64_t M, int32_t C, int32_t hw, int32_t dtype, vsx_stream_t stream);
/* GRN statistics and fc2 weight gradient from the per-sample products Q[b] = dout_b^T . g_b ([C, 4C] fp32 each, vsx_gemm_tn
 * with b_bstride) and the per-sample column sums cs[b][C] of dout — dz = dout . W2 is linear in dout, so
 *   P[b, j] = sum_hw dz*g = sum_c W2[c, j] * Q[b, c, j]          S[b, j] = sum_hw dz = sum_c W2[c, j] * cs[b, c]
 *   dW2[c, j] += sum_b s[b, j] * Q[b, c, j] + beta[j] * sum_b cs[b, c]        db2[c] += sum_b cs[b, c]
 * (W2 = the bf16 GEMM operand [C, 4C]): neither dz nor a pass over the 4C-wide activations is needed for the statistics. */
int32_t vsx_grn_q_reduce(const float* Q, const float* cs, const void* W2, const float* s, const float* beta, float* P, float* S,
    float* dW2, float* db2, float* ws, int64_t ws_floats, int32_t nb, int32_t C, int32_t dtype, vsx_stream_t stream);
/* floats of caller-owned scratch vsx_grn_q_reduce needs (Q is read ONCE: the per-sample-group partials of dW2 pass through it) */
int64_t vsx_grn_q_reduce_ws_floats(int32_t nb, int32_t C);
/* Block backward without a stored dz (csrc/mlp.hip MODE 3 / 4; wimg = vsx_mlp_pack with W2^T [4C, C] in the place of W1'):
 *   vsx_mlp_bwd_stats: P[b, 4C] += sum_hw dz * g, S[b, 4C] += sum_hw dz with dz = bf16(dout . W2) recomputed tile by tile —
 *                      what vsx_gemm_nt(VSX_EPI_DZ) accumulates, minus its 4C-wide output
 *   vsx_mlp_bwd_dh   : dh = (dz * s[b] + gelu(h) * t[b]) * gelu'(h) stored [M, 4C] (dz recomputed), colsum[4C] += sum of dh over
 *                      all rows through the caller-owned workspace ws [ws_rows >= M / vsx_mlp_rows_per_workgroup, 4C] —
 *                      vsx_gemm_nt(VSX_EPI_DZ) + vsx_grn_gelu_bwd with ONE 4C-wide write instead of two */
int32_t vsx_mlp_bwd_stats(const void* dout, const void* wimg, const void* g, float* P, float* S, int64_t M, int32_t C, int32_t hw,
    int32_t dtype, vsx_stream_t stream);
int32_t vsx_mlp_bwd_dh(const void* dout, const void* wimg, const void* h, const float* s, const float* t, void* dh, float* ws,
                       int64_t ws_rows, float* colsum, const float* gelu_table, int64_t M, int32_t C, int32_t hw, int32_t dtype,
                       vsx_stream_t stream);
int32_t vsx_mlp_rows_per_workgroup(int32_t C, int32_t hw, int64_t M);
/* vsx_mlp_bwd_dh WITHOUT a stored pre-activation (csrc/mlp.hip MODE 5; round 4): h = bf16(xh . W1'^T + b1) is recomputed on chip
 * from the normalised rows xh [M, C] — wimg_fwd = vsx_mlp_pack(W1', W2) and b1 are the operands vsx_mlp_fc1 ran with, so the
 * recomputed h is bit-identical to the one it would have stored — beside dz = dout . W2 (wimg_bwd as for vsx_mlp_bwd_dh).  With
 * vsx_mlp_fc1 / vsx_mlp_fc1_ln called with h = NULL (MODE 6: only g is stored) the 4C-wide h never exists in memory: one 4C-wide
 * write less in the forward, one 4C-wide read less in the backward, per block.  Available where
 * vsx_mlp_mode_supported(.., 5, ..) / (.., 6, ..) (C <= 224, `mlp_fused` bit 6).  Reference math: timm GlobalResponseNormMlp as
 * restated in viscy_models/unet/fcmae.py:174-221. */
int32_t vsx_mlp_bwd_dh_re(const void* dout, const void* xh, const void* wimg_bwd, const void* wimg_fwd, const float* b1, const float* s,
                          const float* t, void* dh, float* ws, int64_t ws_rows, float* colsum, const float* gelu_table, int64_t M,
                          int32_t C, int32_t hw, int32_t dtype, vsx_stream_t stream);
/* vsx_mlp_bwd_dh_re for a block whose forward stored NO normalised rows (csrc/mlp.hip MODE 7; vsx_mlp_fc1_ln with xh_out = NULL):
 * y [M, C] = the LayerNorm input (depthwise output), mean / rstd [M] = its row statistics; x^ = bf16((y - mean) * rstd) is re-formed
 * on chip as the forward formed it.  The pass writes dh' = dh * rstd (row-scaled) — what the consumers want once they read y, too:
 *   fc1 weight gradient  dh^T . x^ = dh'^T . y - u (x) 1  with u[j] = sum_r dh'[r, j] * mean[r]   (plain vsx_gemm_tn on y; then
 *                        vsx_unprep_grad(.., rowsub = u))
 *   LayerNorm backward   dy = dx' - mean_c(dx') - x^ * mean_c(dx' * x^), dx' = dh' . W1'   (vsx_gemm_nt VSX_EPI_LN_BWD with
 *                        aux = y, grn_s = rstd, grn_b = mean: the trailing "* rstd" is already in dx')
 * colsum2 [2, 4C] += { sum_r dh[r, j] (the fc1 bias gradient), u[j] }; ws [ws_rows >= M / vsx_mlp_rows_per_workgroup, 2 * 4C].
 * Available where vsx_mlp_mode_supported(.., 7, ..) (C <= 224, `mlp_fused` bits 5, 6 and 7).  Reference math: the LayerNorm
 * -> Linear pair of timm's ConvNeXtBlock (norm, mlp.fc1) as restated in viscy_models/unet/fcmae.py:174-221. */
int32_t vsx_mlp_bwd_dh_ln(const void* dout, const void* y, const float* mean, const float* rstd, const void* wimg_bwd,
                          const void* wimg_fwd, const float* b1, const float* s, const float* t, void* dh, float* ws, int64_t ws_rows,
                          float* colsum2, const float* gelu_table, int64_t M, int32_t C, int32_t hw, int32_t dtype,
                          vsx_stream_t stream);
/* GELU of a bf16 value through a table (csrc/mlp.hip): vsx_mlp_gelu_table fills `tab` (vsx_mlp_gelu_table_len() = 2 N floats)
 * with r(a) = a * Phi(-a) (first N) and d(a) = Phi(a) + a * phi(a) - 1/2 (second N) for every bf16 magnitude a in [2^-24, 16):
 * gelu(h) = max(h, 0) - r(|h|), gelu'(h) = 1/2 + sign(h) * d(|h|).  The forward passes read the first half, the dh passes both. */
int32_t vsx_mlp_gelu_table_len(void);
int32_t vsx_mlp_gelu_table(float* tab, vsx_stream_t stream);

/* Device-side half of the optimiser schedule (viscy_utils/optimizers.py:50-61: AdamW + MONAI WarmupCosineSchedule stepped per
 * batch): reads cfg = {base_lr, beta1, beta2, eps, weight_decay, grad_scale, schedule (0 constant | 1 warm-up cosine),
 * warmup_steps, t_total, warmup_multiplier, cycles} and the int32 step counter, writes the 8 scalars vsx_adamw reads for
 * THIS step and increments the counter.  No host memory is touched: a captured step replays correctly however far the
 * host runs ahead. */
int32_t vsx_adamw_advance(const double* cfg, int32_t* step, float* hyper, vsx_stream_t stream);

/* p[0 .. n) = value (16-byte aligned p): `optimizer.zero_grad()` on the flat gradient buffer, the zero-filled reduction
 * targets of a pass, start values of running maxima — ordinary kernel nodes in the captured step. */
int32_t vsx_fill_f32(float* p, int64_t n, float value, vsx_stream_t stream);

/* fp32 parameter viewed as [R, Cs, Tn] (out, in, taps) → GEMM operand dst [R, Tn*Cs] and/or dstT [Tn*Cs, R] in `dtype`, optionally scaled per
 * input channel by gamma (LayerNorm fold).  tapmode 1 = head Conv3d tap order (kz,ky,kx) → (ky,kx,kz). */
int32_t vsx_prep_weight(const float* src, void* dst, void* dstT, const float* gamma, int32_t R, int32_t Cs,
    int32_t Tn, int32_t tapmode, int32_t dtype, vsx_stream_t stream);

/* inverse of vsx_prep_weight for gradients: dparam[r][c][t] += g'[r][k]*gamma[c] + u[r]*beta[c]; dgamma[c] += Σ g'*W, with
 * g'[r][k] = g[r][k] - rowsub[r] (rowsub may be NULL: the rank-1 term of a weight gradient that was contracted with un-centred
 * rows, see vsx_mlp_bwd_dh_ln). */
int32_t vsx_unprep_grad(const float* g, float* dparam, const float* gamma, const float* W, float* dgamma,
    const float* u, const float* beta, const float* rowsub, int32_t R, int32_t Cs, int32_t Tn, int32_t tapmode,
    vsx_stream_t stream);

/* fold of the GRN affine into the fc2 weights (timm GlobalResponseNorm inside GlobalResponseNormMlp, between act and fc2):
 * out[b][r][k] = dtype(W[r][k] * s[b][k]) for b < B; W fp32 [R][K], s fp32 [B][K].  Pairs with VsxGemm.b_bstride = R*K. */
int32_t vsx_scale_weight_samples(const float* W, const float* s, void* out, int32_t B, int32_t R, int32_t K,
    int32_t dtype, vsx_stream_t stream);

/* out[r] = (b ? b[r] : 0) + Σ_c W[r][c]*v[c]   (fold LayerNorm beta into the fc1 bias). */
int32_t vsx_matvec(const float* W, const float* v, const float* b, float* out, int32_t R, int32_t C,
    vsx_stream_t stream);

/* out[c] += Σ_r W[r][c]*u[r]   (gradient of the folded LayerNorm beta). */
int32_t vsx_matvec_t_add(const float* W, const float* u, float* out, int32_t R, int32_t C,
    vsx_stream_t stream);

/* dst[j][i] (+)= src[i][j]  (depthwise weights [C][49] <-> [49][C]). */
int32_t vsx_transpose_f32(const float* src, float* dst, int32_t A, int32_t Bn, int32_t accumulate,
    vsx_stream_t stream);

/* A list of independent weight-space jobs in one launch per VSX_WTASK_MAX tasks (the step refreshes ~200 prepared operands
 * per weight update; as single launches each leaves the chip idle for 4 - 7 us).  kind selects which single-op entry point
 * the task stands for; fields as documented at vsx_weight_tasks in csrc/optim.hip:
 *   PREP: p0 src, p1 dst, p2 dstT, p3 gamma, i0 R, i1 Cs, i2 Tn, i3 tapmode, dtype;  TRANSPOSE: p0 src, p1 dst, i0 A, i1 Bn,
 *   i2 accumulate;  MATVEC: p0 W, p3 v, p2 b, p1 out, i0 R, i1 C;  MLP_PACK: p0 W1, p3 W2, p1 img, i0 C.
 * No task may read or accumulate into what another task of the same call writes. */
#define VSX_WTASK_PREP 0
#define VSX_WTASK_TRANSPOSE 1
#define VSX_WTASK_MATVEC 2
#define VSX_WTASK_MLP_PACK 3
#define VSX_WTASK_UNPREP 4    /* vsx_unprep_grad: p0 g, p1 dparam, p3 gamma, p4 W, p2 dgamma, p5 u, p6 beta, p7 rowsub, i0 R, i1 Cs, i2 Tn, i3 tapmode */
#define VSX_WTASK_MATVEC_T 5  /* vsx_matvec_t_add: p0 W, p3 u, p1 out, i0 R, i1 C */
#define VSX_WTASK_REDUCE_ROWS 6  /* p1 out[n] += sum_r p0 ws[r][n], i0 rows, i1 columns */
#define VSX_WTASK_MAX 40
typedef struct VsxWTask {
  int32_t kind, dtype, i0, i1, i2, i3;
  const void* p0;
  void* p1;
  void* p2;
  const void* p3;
  const void* p4;
  const void* p5;
  const void* p6;
  const void* p7;
} VsxWTask;
int32_t vsx_weight_tasks(const VsxWTask* tasks, int32_t n, vsx_stream_t stream);

/* head Conv3d data-gradient weights: [Zout+2][C3][27*Cmid], zero where the depth tap falls outside [0,2]. */
int32_t vsx_prep_head_dgrad(const float* W, void* dst, int32_t Cmid, int32_t C3, int32_t Zout, int32_t dtype,
    vsx_stream_t stream);

/* K1 gather half of UNeXt2Stem (viscy_models/components/stems.py:26-50): the Conv3d with kernel = stride = (kz,ky,kx) is a GEMM over
 * non-overlapping patches; writes the patch matrix [B*h*w, D'*K].  Optional per-sample (sub, div) fuses NormalizeSampled
 * (viscy_transforms/_normalize.py:72-80): (x - sub)/(div + 1e-8). */
int32_t vsx_stem_im2col(const float* x, void* P, const float* sub, const float* div, int32_t B, int32_t Cin,
    int32_t Z, int32_t H, int32_t W, int32_t kz, int32_t ky, int32_t kx, int32_t dtype, vsx_stream_t stream);
/* the same gather with rows of ldp >= patch-size elements (tail zero-filled), and the matching weight-space helper
 * dst[r][k] = k < K ? src[r][k] : 0: K = 80 of the 5x4x4 stem becomes 96 = a whole number of 32-deep MFMA slabs */
int32_t vsx_stem_im2col_ld(const float* x, void* P, const float* sub, const float* div, int32_t B, int32_t Cin, int32_t Z,
    int32_t H, int32_t W, int32_t kz, int32_t ky, int32_t kx, int32_t ldp, int32_t dtype, vsx_stream_t stream);
int32_t vsx_pad_cols(const void* src, void* dst, int32_t R, int32_t K, int32_t Kp, int32_t dtype, vsx_stream_t stream);

/* Dense 3x3 convolution (padding 1) of a channels-last map as a GEMM — MONAI SubpixelUpsample's pre-convolution, selected by
 * UNeXt2(decoder_upsample_pre_conv=True) (/root/reference/packages/viscy-models/src/viscy_models/components/blocks.py:138-146).
 * vsx_im2col3x3: col[m][t*C + c] = x[b, y + t/3 - 1, x + t%3 - 1, c], zero outside the image (t = 3*ky + kx: the K order of
 * vsx_prep_weight(conv.weight, Cout, C, 9)).  vsx_col2im3x3: its transpose, dx[m][c] = sum_t dcol[m - shift(t)][t*C + c]. */
int32_t vsx_im2col3x3(const void* x, void* col, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, vsx_stream_t stream);
int32_t vsx_col2im3x3(const void* dcol, void* dx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, vsx_stream_t stream);

/* K10: MONAI UpSample(mode="pixelshuffle", pre_conv=None) + torch.cat([up, skip], 1) (viscy_models/components/blocks.py:138-146,170-171). */
int32_t vsx_pixel_shuffle_cat_fwd(const void* low, const void* skip, void* out, int32_t B, int32_t h,
    int32_t w, int32_t c, int32_t cs, int32_t dtype, vsx_stream_t stream);

/* backward of K10: scatter dcat into dlow (inverse shuffle) and dskip. */
int32_t vsx_pixel_shuffle_cat_bwd(const void* dcat, void* dlow, void* dskip, int32_t B, int32_t h, int32_t w,
    int32_t c, int32_t cs, int32_t dtype, vsx_stream_t stream);

/* K12: PixelToVoxelHead.upsample (pixel shuffle x2 + optional ConstantPad2d((1,0,1,0)) + AvgPool2d(2,1)) + reshape (heads.py:607-615,632-637);
 * output channel = z*C3 + c3 so the 3x3x3 conv reads contiguous channel slices per depth. */
int32_t vsx_head_shuffle_fwd(const void* dec, void* hin, int32_t B, int32_t h, int32_t w, int32_t C3,
    int32_t D, int32_t pool, int32_t dtype, vsx_stream_t stream);

/* backward of K12. */
int32_t vsx_head_shuffle_bwd(const void* dhin, void* ddec, int32_t B, int32_t h, int32_t w, int32_t C3,
    int32_t D, int32_t pool, int32_t dtype, vsx_stream_t stream);

/* K17 NormalizeSampled.__call__ (viscy_transforms/_normalize.py:72-80) on a (B, ...) fp32 batch with (B,) statistics. */
int32_t vsx_normalize(const float* x, float* y, const float* sub, const float* div, int32_t B, int64_t per_sample,
    vsx_stream_t stream);

/* MinMaxSampled.__call__ (viscy_transforms/_normalize.py:124-134). */
int32_t vsx_minmax_norm(const float* x, float* y, const float* lo, const float* hi, int32_t B, int64_t per_sample,
    vsx_stream_t stream);

/* per-sample min / max needed by MONAI AdjustContrast (K19); mn / mx must be pre-set to +inf / -inf. */
int32_t vsx_sample_minmax(const float* x, float* mn, float* mx, int32_t B, int64_t per_sample, vsx_stream_t stream);

/* K19-K21 fused: BatchedRandAdjustContrast (_adjust_contrast.py:54-86) -> BatchedRandScaleIntensity
 * (_scale_intensity.py:59-77) -> BatchedRandGaussianNoise (_noise.py:158-204) with injected per-sample parameters. */
int32_t vsx_intensity_aug(const float* x, float* y, const float* mn, const float* mx, const float* gamma,
    const float* factor, const float* noise, const float* nstd, float nmean, int32_t invert, int32_t B, int64_t per_sample,
    vsx_stream_t stream);
/* invert: bit 0 = the gamma curve runs on -x (MONAI AdjustContrast(invert_image=True), called at _adjust_contrast.py:76-80),
 * bit 1 = the result is negated back; 0 or 3 in normal use, 1 when the retain_stats affine follows on the host side.
 * vsx_sample_moments: per-sample sum and sum of squares in double (sums[B][2], pre-set to 0) — the mean / std that
 * AdjustContrast(retain_stats=True) measures before and restores after the curve. */
int32_t vsx_sample_moments(const float* x, double* sums, int32_t B, int64_t per_sample, vsx_stream_t stream);

/* K25 _blend_in (viscy_utils/callbacks/prediction_writer.py:74-111): Z-feathered running average, fz[Z] = factors. */
int32_t vsx_blend_in(const float* oldp, const float* newp, float* out, const float* fz, int32_t Z, int64_t plane,
    int64_t total, vsx_stream_t stream);

/* K23 viscy_transforms.BatchedRandWeightedCropd (_crop.py:263-386): window weights = clamp(sum over (C, Z), 0) summed over
 * every (cy, cx) window (stride 1) -> wpool [B, (Y-cy+1)*(X-cx+1)]; tmp = caller scratch of B*Y*X + B*Y*(X-cx+1) floats. */
int32_t vsx_crop_weights(const float* w, float* wpool, float* tmp, int32_t B, int32_t CZ, int32_t Y, int32_t X,
    int32_t cy, int32_t cx, vsx_stream_t stream);
/* inverse-CDF draw: idx[b] = smallest i with sum_{j<=i} wpool[b,j] > u[b] * sum_j wpool[b,j]  (uniform when the sum is 0) */
int32_t vsx_sample_index(const float* wpool, const float* u, int32_t* idx, int32_t B, int64_t n, vsx_stream_t stream);
/* y[b,c,z,yy,xx] = x[b,c, starts[b][0]+z, starts[b][1]+yy, starts[b][2]+xx]   (starts int32 [B,3] on the device) */
int32_t vsx_crop3d(const float* x, float* y, const int32_t* starts, int32_t B, int32_t C, int32_t Z, int32_t Y, int32_t X,
    int32_t cz, int32_t cy, int32_t cx, vsx_stream_t stream);

/* Per-row order statistics by radix select (the quantiles of BatchedScaleIntensityRangePercentiles, _percentile_scale.py:59-68,
 * without torch.quantile's sort and its 2^24-element limit).  x: rows contiguous rows of n fp32 values, any alignment of the
 * row starts; ranks[nranks] (host array, 1 <= nranks <= 4, 0 <= rank < n <= 2^31 - 1): zero-based positions in the sorted row,
 * the same for every row; out[rows][nranks] = exactly the element torch.sort(row).values[rank] holds (-0.0 / +0.0 may come
 * back as either).  A row that holds a NaN yields NaN for all its ranks.  ws: caller-owned device scratch of
 * vsx_row_select_ws_bytes(rows, nranks) bytes, initialised by the call.  Integer atomics only: bit-identical from run to run;
 * 9 launches whatever the data, no allocation, synchronisation or device-to-host copy. */
int64_t vsx_row_select_ws_bytes(int64_t rows, int32_t nranks);
int32_t vsx_row_select(const float* x, float* out, void* ws, int64_t ws_bytes, int64_t rows, int64_t n, const int64_t* ranks,
    int32_t nranks, vsx_stream_t stream);

/* BatchedScaleIntensityRangePercentiles._normalize (_percentile_scale.py:78-90) on rows contiguous rows of n values with
 * per-row bounds a_min / a_max [rows]:  y = (x - a_min) / (a_max - a_min); flags bit 0: then * (b_max - b_min) + b_min;
 * bit 1 / bit 2: then clip below at b_min / above at b_max.  Where degenerate[row] != 0 (int32 [rows], the reference's
 * batch-wide `(a_min == a_max).any()` expanded by the caller): y = x - a_min, + b_min with bit 3.  Every operation is rounded on
 * its own (no contraction, IEEE division), so the result equals the reference's tensor expressions bit for bit. */
int32_t vsx_percentile_scale(const float* x, float* y, const float* a_min, const float* a_max, const int32_t* degenerate,
    int64_t rows, int64_t n, double b_min, double b_max, int32_t flags, vsx_stream_t stream);

/* BatchedRandSpatialCrop's gather (_crop.py:98-125) followed by BatchedChannelWiseZReduction (_z_reduction.py:49-61) in one
 * pass: y[b,c,0,yy,xx] over the window (cz,cy,cx) at starts[b] (int32 [B,3]; NULL = zeros), each start clamped into
 * [0, dim - c] inside the kernel; mode[b] (int32 [B]) 0 = maximum over the window's Z (NaN propagates, as amax), 1 = its
 * centre plane cz / 2.  Only the window is read. */
int32_t vsx_crop_zreduce(const float* x, float* y, const int32_t* starts, const int32_t* mode, int32_t B, int32_t C, int32_t Z,
    int32_t Y, int32_t X, int32_t cz, int32_t cy, int32_t cx, vsx_stream_t stream);

/* The DynaCLR data feed (viscy_data/triplet.py:224-253, read there patch by patch through tensorstore on the host): n patches
 * cut out of frames resident in device memory, out[p, c, z, y, x] = (float) frame_p[c, z, y0_p + y, x0_p + x], fp32
 * [n, C, Z, Yp, Xp].  desc: n rows of VSX_PG_DESC int64 on the device: {address of the frame's element [0, 0, 0, 0], element
 * strides of c, z and y (x is contiguous), y0, x0}; a frame is a [C, Z, H, W] block of src_dtype, or a view into a larger one.
 * Descriptors may repeat and may name different frames.  float32 sources are copied bit for bit, integer sources convert
 * exactly.  No load leaves [x0, x0 + Xp) of its row.  The kernel trusts the table: the caller has checked 0 <= y0,
 * y0 + Yp <= H, 0 <= x0, x0 + Xp <= W (viscy_amd.ops.patch_gather does).  out 16-byte aligned. */
#define VSX_PG_F32 0
#define VSX_PG_U16 1
#define VSX_PG_I16 2
#define VSX_PG_U8 3
#define VSX_PG_DESC 6
int32_t vsx_patch_gather(const int64_t* desc, float* out, int32_t n, int32_t C, int32_t Z, int32_t Yp, int32_t Xp,
    int32_t src_dtype, vsx_stream_t stream);

/* The multi-experiment DynaCLR feed (dynaclr/data/dataset.py `_slice_patch`: one tensorstore read and one host
 * F.interpolate(mode="nearest-exact") per patch there): per-patch channel lists, per-patch native boxes and the resampling to
 * one target size in one launch, out[p, c, z, y, x] = (float) frame_p[chan_p[c], zi_p[z], yi_p[y], xi_p[x]], fp32
 * [n, C, Zt, Yt, Xt].  desc: n rows of VSX_PGS_DESC int64 on the device: {address of the frame's element [0, 0, 0, 0], element
 * strides of c, z and y (x is contiguous), offsets (in ints) into idx of the patch's channel table (C entries), z table (Zt), y
 * table (Yt) and x table (Xt)}.  idx: int32 on the device.  Table entries are ABSOLUTE positions in the patch's frame (the host
 * has added the box origin); patches may share tables by naming the same offset, and may name different frames of different
 * shapes.  A frame is a [Cf, Zf, H, W] block of src_dtype (a VSX_PG_* code), or a view into a larger one.  float32 sources are
 * copied bit for bit, integer sources convert exactly.  Every load reads an element the tables name.  The kernel trusts the
 * tables: the caller has checked every entry against the frame's shape (viscy_amd.ops.patch_gather_scaled does).  With arange
 * tables the result is vsx_patch_gather's.  out 16-byte aligned; Xt <= VSX_PGS_MAX_XT (the x table is held in LDS).  The grid is
 * capped at eight workgroups per compute unit; a workgroup's row groups take VSX_PGS_ROWS_PER_GROUP rows each per work unit. */
#define VSX_PGS_DESC 8
#define VSX_PGS_MAX_XT 16384
#define VSX_PGS_ROWS_PER_GROUP 4
int32_t vsx_patch_gather_scaled(const int64_t* desc, const int32_t* idx, float* out, int32_t n, int32_t C, int32_t Zt,
    int32_t Yt, int32_t Xt, int32_t src_dtype, vsx_stream_t stream);

/* K18 kornia warp_affine3d as used by BatchedRandAffined (viscy_transforms/_affine.py:33-47,358-393): trilinear (or
 * nearest) resampling; Minv[B][3][4] maps output-voxel to input-voxel coordinates (x, y, z order).
 * The kernel applies Minv as given; the caller folds kornia's align_corners convention into it (with align_corners=False — kornia's
 * RandomAffine3D default, which the reference forwards — output voxel i reads Da^-1 (R Da (i + 1/2) + t) - 1/2, a = (size - 1) / size
 * per axis: viscy_amd.transforms.kornia_sampling_matrix).
 * mode: bit 0 = nearest-neighbour; bits 1-2 = padding_mode of _affine.py:102-108 as torch's grid_sample treats it: 0 "zeros",
 * 1 "border" (coordinates clamped to the volume), 2 "reflection" with align_corners=True (mirrored about 0 and n-1),
 * 3 "reflection" with align_corners=False (mirrored about -1/2 and n-1/2, then clamped). */
int32_t vsx_warp_affine3d(const float* x, float* y, const float* Minv, int32_t B, int32_t C, int32_t D, int32_t H,
    int32_t W, int32_t mode, vsx_stream_t stream);
/* the same warp restricted to the output window [z0,z0+Do) x [y0,y0+Ho) x [x0,x0+Wo) of the (D,H,W) frame: fuses the
 * BatchedCenterSpatialCrop that follows the affine in the recipes (_crop.py:164-187); y: (B,C,Do,Ho,Wo). */
int32_t vsx_warp_affine3d_roi(const float* x, float* y, const float* Minv, int32_t B, int32_t C, int32_t D, int32_t H,
    int32_t W, int32_t z0, int32_t y0, int32_t x0, int32_t Do, int32_t Ho, int32_t Wo, int32_t mode, vsx_stream_t stream);

/* K22 one pass of the separable Gaussian of BatchedRandGaussianSmooth (viscy_transforms/_gaussian_smooth.py:141-167):
 * per-sample 1-D taps along the axis with element stride `stride` and length L, zero border. */
int32_t vsx_conv1d_axis(const float* x, float* y, const float* taps, int32_t k, int32_t B, int64_t per_sample,
    int64_t stride, int32_t L, vsx_stream_t stream);

/* Dense 3x3x3 convolution family (csrc/conv3d.hip): FNet3D.  Activations channels-last [B*D*H*W][C] with a row stride (ld*) and a
 * channel offset (*coff); dtype VSX_BF16 (MFMA bf16) or VSX_F32 (exact fp32 MFMA).  Reductions: per-workgroup partials, fixed-order fold.
 * prep_weight: out[n][t * Kc + c] = w[n * sn + c * sc + (flip ? 26 - t : t)]  (tap-major GEMM operand, dtype).
 * fwd: c[o][ccoff + n] = bias[n] (+ c, accumulate) + sum over taps / channels of a * W (prepared [Cout][27 Cin]); zero padding 1,
 * stride 1 or 2, or (transposed = 1) ConvTranspose3d k 3 / stride 2 / padding 1 / output_padding 1 over the 2x output grid.  B, Di, Hi,
 * Wi: input grid.  out_f32: c is fp32 (bf16 operands).  stats (optional): [vsx_conv3d_stats_rows][2][Cout] column partials of z, z^2.
 * wgrad: out[r][c][t] += sum over voxels m of the P grid (B, Dg, Hg, Wg) of P[m][r] * Q[m * stride + k(t) - 1][c], Q on the grid
 * (Dg, Hg, Wg) * stride; ws: vsx_conv3d_wgrad_ws_floats floats.
 * colsum: out[c] += sum over M rows of x[row][xcoff + c]; ws: vsx_conv3d_colsum_groups(M) * C floats.
 * bn3d_finalize: ss = [scale | shift | mean | rstd] ([4][C]) from the stats partials (training; running stats and num_batches_tracked
 * updated on the device) or the running statistics (eval).  bn3d_apply_relu: dst[r][dcoff + c] = max(z * scale + shift, 0).
 * bn3d_bwd: g = dy * [z * scale + shift > 0]; dgamma += sum g xhat, dbeta += sum g, dz = gamma rstd (g - mean g - xhat mean(g xhat))
 * (training) or gamma rstd g (eval); ws: vsx_bn3d_bwd_ws_floats floats.  to_cl / from_cl: NCDHW fp32 <-> channels-last. */
int32_t vsx_conv3d_prep_weight(const float* w, void* out, int32_t N, int32_t Kc, int32_t sn, int32_t sc, int32_t flip, int32_t dtype,
    vsx_stream_t stream);
int64_t vsx_conv3d_stats_rows(int32_t B, int32_t Di, int32_t Hi, int32_t Wi, int32_t stride, int32_t transposed);
int32_t vsx_conv3d_fwd(const void* a, int32_t lda, int32_t acoff, const void* wp, const float* bias, void* c, int32_t ldc,
    int32_t ccoff, float* stats, int32_t B, int32_t Di, int32_t Hi, int32_t Wi, int32_t Cin, int32_t Cout, int32_t stride,
    int32_t transposed, int32_t accumulate, int32_t dtype, int32_t out_f32, vsx_stream_t stream);
int64_t vsx_conv3d_wgrad_ws_floats(int32_t B, int32_t Dg, int32_t Hg, int32_t Wg, int32_t R, int32_t C, int32_t dtype);
int32_t vsx_conv3d_wgrad(const void* P, int32_t ldp, int32_t pcoff, const void* Q, int32_t ldq, int32_t qcoff, float* ws,
    int64_t ws_floats, float* out, int32_t B, int32_t Dg, int32_t Hg, int32_t Wg, int32_t R, int32_t C, int32_t stride,
    int32_t dtype, vsx_stream_t stream);
int64_t vsx_conv3d_colsum_groups(int64_t M);
int32_t vsx_conv3d_colsum(const void* x, int32_t ldx, int32_t xcoff, int64_t M, int32_t C, float* ws, float* out, int32_t dtype,
    vsx_stream_t stream);
int32_t vsx_bn3d_finalize(const float* ws, int64_t G, int64_t M, int32_t C, const float* gamma, const float* beta, float* rmean,
    float* rvar, int64_t* nbt, float* ss, float eps, float momentum, int32_t training, vsx_stream_t stream);
int32_t vsx_bn3d_apply_relu(const void* z, const float* ss, void* dst, int32_t ldd, int32_t dcoff, int64_t M, int32_t C,
    int32_t dtype, vsx_stream_t stream);
int64_t vsx_bn3d_bwd_ws_floats(int64_t M, int32_t C);
int32_t vsx_bn3d_bwd(const void* dy, int32_t ldy, int32_t ycoff, const void* z, const float* ss, const float* gamma, float* ws,
    float* dgamma, float* dbeta, void* dz, int64_t M, int32_t C, int32_t training, int32_t dtype, vsx_stream_t stream);
int32_t vsx_conv3d_to_cl(const float* x, void* out, int32_t B, int32_t C, int64_t S, int32_t dtype, vsx_stream_t stream);
int32_t vsx_conv3d_from_cl(const void* y, float* out, int32_t B, int32_t C, int64_t S, int32_t dtype, vsx_stream_t stream);

/* OnlineEvalCallback (csrc/online_eval.hip + f32_tile.h): cosine k-NN probe, neighbour vote, pair distances; fp32 throughout (exact f32 MFMA).
 * row_inv_norm: inv[i] = 1 / (||x_i||_2 + eps), 0 where that denominator is 0 (an all-zero row with eps = 0).
 * knn_topk: row j is a candidate of query i iff group[j] >= 0 && group[j] != group[i]; s_ij = fl32(fl32(dot_ij * inv[i]) * inv[j]),
 * dot accumulated in fp32.  Per query: its min(k, #candidates) best candidates in the total order (s descending, j ascending) in
 * idx / sim [N][k], their number in cnt[N]; unused slots idx = -1, sim = -inf.  1 <= k <= 64, any d >= 1 and N >= 1.  No N x N buffer:
 * ws (4-byte aligned) holds vsx_knn_topk_ws_bytes(N, d, k) = O(N k) bytes, any contents.
 * knn_vote: pred[i] = the most frequent label among labels[idx[i][0 .. cnt[i])], ties to the smallest label; -1 for cnt[i] = 0.
 * pair_cosine_dist: out[p] = 1 - fl32(fl32(dot(x_pi[p], x_pj[p]) * inv[pi[p]]) * inv[pj[p]]). */
#define VSX_KNN_MAX_K 64 /* largest k of vsx_knn_topk / vsx_knn_vote */
int32_t vsx_row_inv_norm(const float* x, float* inv, int32_t N, int32_t d, float eps, vsx_stream_t stream);
int64_t vsx_knn_topk_ws_bytes(int32_t N, int32_t d, int32_t k);
int32_t vsx_knn_topk(const float* x, const float* inv, const int32_t* group, int32_t N, int32_t d, int32_t k, int32_t* idx, float* sim,
    int32_t* cnt, void* ws, int64_t ws_bytes, vsx_stream_t stream);
int32_t vsx_knn_vote(const int32_t* idx, const int32_t* cnt, const int32_t* labels, int32_t N, int32_t k, int32_t* pred,
    vsx_stream_t stream);
int32_t vsx_pair_cosine_dist(const float* x, const float* inv, const int32_t* pi, const int32_t* pj, int64_t P, int32_t d, float* out,
    vsx_stream_t stream);

/* ClassificationHead's classifier + cross-entropy (csrc/aux_head.hip + f32_tile.h; heads.py:159-272, 420-453); fp32 throughout, dot products
 * on the exact f32 MFMA.  h [B, H], W [C, H], labels [B] int64.  Cosine classifier: inv_h [B], inv_w [C] from vsx_cls_inv_norm
 * (inv = 1 / max(||x||, 1e-12), F.normalize's rule: a zero row gives zero logits and finite gradients) and the device scalar
 * log_scale; bias must be null.  Linear: inv_h = inv_w = log_scale = null, bias [C] or null.
 *   cosine  z_bc = fl32(fl32(fl32(dot_bc * inv_h[b]) * inv_w[c]) * expf(log_scale[0]));   linear  z_bc = fl32(dot_bc + bias[c])
 * vsx_cls_ce_fwd: rows [B, 4] = {lse, target logit, rank, valid}, acc [4] = {loss, top-1, top-k, n_valid}; rank = the number of
 * classes ahead of the target in the total order (logit descending, class ascending), a top-k hit is rank < k; loss =
 * sum_valid (lse - z_y) / n_valid, top-1 / top-k are divided by B.  No [B, C] buffer, no atomics; rows and acc are bit-identical
 * from run to run and for every `splits` (how many workgroups share the class range of 128 rows; 0 = chosen by the library).
 * Label -100 = ignore_index: valid = 0, the row counts in no sum and has exactly zero gradient (all ignored: loss NaN).  Any other
 * label outside [0, C) never indexes memory: valid = -1 and the loss is NaN.  Non-finite logits reach the loss as in torch.
 * vsx_cls_logits: Z [B, C], the same logits materialised (inference).
 * vsx_cls_ce_bwd: dh [B, H] = gout[0] * d loss / d h (written); dW [C, H], dbias [C] (linear, may be null), dlog_scale [1]
 * (cosine) are ACCUMULATED into; the two normalisations' backward is included.  All gradients are sums in a fixed order:
 * bit-reproducible.  Served: H % 4 == 0, 1 <= k <= C, any C >= 1 and B >= 1; h, W, dh, dW 16-byte aligned; anything else is
 * refused with a non-zero status and no launch.  Workspaces: any contents, vsx_cls_ce_{fwd,bwd}_ws_bytes. */
int32_t vsx_cls_inv_norm(const float* x, float* inv, int32_t N, int32_t d, vsx_stream_t stream);
int64_t vsx_cls_ce_fwd_ws_bytes(int32_t B, int32_t H, int32_t C);
int32_t vsx_cls_ce_fwd(const float* h, const float* W, const int64_t* labels, const float* inv_h, const float* inv_w,
    const float* log_scale, const float* bias, int32_t B, int32_t H, int32_t C, int32_t k, int32_t splits, float* rows, float* acc,
    void* ws, int64_t ws_bytes, vsx_stream_t stream);
int32_t vsx_cls_logits(const float* h, const float* W, const float* inv_h, const float* inv_w, const float* log_scale,
    const float* bias, int32_t B, int32_t H, int32_t C, float* Z, vsx_stream_t stream);
int64_t vsx_cls_ce_bwd_ws_bytes(int32_t B, int32_t H, int32_t C);
int32_t vsx_cls_ce_bwd(const float* h, const float* W, const int64_t* labels, const float* inv_h, const float* inv_w,
    const float* log_scale, const float* bias, const float* rows, const float* acc, const float* gout, int32_t B, int32_t H,
    int32_t C, float* dh, float* dW, float* dbias, float* dlog_scale, void* ws, int64_t ws_bytes, vsx_stream_t stream);

/* MMD two-sample permutation test (csrc/mmd.hip + f32_tile.h; viscy_utils/evaluation/mmd.py): Gaussian RBF kernel sums of N pooled rows
 * [X; Y] under P label vectors, without an N x N buffer.  fp32 kernel values from dots on the exact f32 MFMA, sums in float64.
 * mmd_prepare: mean[d] = the column mean of x [N, d] (float64 sums in a fixed order, rounded to fp32), xc = fl32(x - mean) (xc may be
 * x), norms[i] = sum_c xc_ic^2.
 * Kernel value, one device function for every entry point:  d2_ij = max(fl32(fl32(n_i + n_j) - 2 dot_ij), 0),
 * k_ij = expf(-fl32(d2_ij / fl32(2 bandwidth))) (IEEE division, library expf), k_ij == k_ji bit for bit; in the pooled kernel k_ii = 0.
 * mmd_sums: labels uint8 [P][N] of 0 / 1 (1 = the row belongs to X); sums [P][3] doubles = {sum_XX, sum_YY, sum_XY} =
 * {z'Kz, T - 2 z'r + z'Kz, z'r - z'Kz} with r = K 1, T = 1'K1.  The kernel tile of a (row tile, column tile) pair is formed once,
 * whatever P.  No floating-point atomics; per-workgroup partials in ws are folded in ascending order in float64, and how the column
 * tiles are shared among workgroups depends on N alone: sums is a pure function of the inputs, bit-identical from run to run.
 * 2 <= N <= 2^24, 1 <= d <= 2^20, 1 <= P <= 2^24, bandwidth > 0.  ws (8-byte aligned): vsx_mmd_sums_ws_bytes(N, P) bytes (0 for shapes
 * that are not served), O(P N / 128), any contents.
 * rbf_block: out [(r1 - r0)][(c1 - c0)] = k_ij for i in [r0, r1), j in [c0, c1) (0 <= r0 < r1 <= N, likewise c; at most 65535 * 128 rows);
 * zero_diag != 0 stores 0 for i == j, else the diagonal holds its computed value.
 * sqdist_upper: out[i (2M - i - 1) / 2 + (j - i - 1)] = d2_ij for 0 <= i < j < M, 2 <= M <= 65536: one contiguous row of M (M - 1) / 2 values
 * (the median heuristic takes its middle ranks with vsx_row_select).
 * Every check runs before any launch; anything not served is refused with a non-zero status. */
int32_t vsx_mmd_prepare(const float* x, float* xc, float* norms, float* mean, int32_t N, int32_t d, vsx_stream_t stream);
int64_t vsx_mmd_sums_ws_bytes(int32_t N, int32_t P);
int32_t vsx_mmd_sums(const float* xc, const float* norms, const uint8_t* labels, int32_t N, int32_t d, int32_t P, double bandwidth,
    double* sums, void* ws, int64_t ws_bytes, vsx_stream_t stream);
int32_t vsx_rbf_block(const float* xc, const float* norms, int32_t N, int32_t d, int32_t r0, int32_t r1, int32_t c0, int32_t c1,
    double bandwidth, int32_t zero_diag, float* out, vsx_stream_t stream);
int32_t vsx_sqdist_upper(const float* xc, const float* norms, int32_t M, int32_t d, float* out, vsx_stream_t stream);

/* The data passes of PCA (csrc/pca.hip; viscy_utils/evaluation/dimensionality_reduction.py compute_pca = StandardScaler -> sklearn PCA):
 * x [n, d] fp32 row-major, any 4-byte alignment, 2 <= n < 2^31, 1 <= d <= 4096.  No atomics: per-workgroup partials in ws, folded in
 * ascending order, so every output is bit-identical from run to run for fixed (n, d).  ws: 8-byte aligned, any contents.
 * col_moments: mean[d] = sum_i x_ij / n, m2[d] = sum_i (x_ij - mean_j)^2, float64 throughout (two passes over x).
 * gram_centered: gram [d, d] float64 = sum_i c_ij c_il with c_ij = fl32(x_ij - mean_j) (float64 difference, rounded once), both triangles
 * written and equal bit for bit.  128 x 128 tiles of feature pairs on v_mfma_f32_32x32x2_f32, upper-triangular tile pairs only; fp32
 * accumulation over blocks of 128 rows, each block sum added to float64 accumulators in ascending block order; the rows are split over
 * workgroups in runs of vsx_gram_rows_per_split(n, d) rows (a multiple of 128, a function of n and d alone) whose float64 tiles are folded
 * in split order.  Standard scaling is the caller's: gram_jl / (s_j s_l) in float64.  ws: vsx_gram_ws_bytes(n, d) = splits * pairs * 128 KiB.
 * center_project: z [n, k] fp32 = (x - mean) w' for w [k, d] fp32, k >= 1: the dots of csrc/f32_tile.h (one summation order) over the
 * centred rows; fold 1 / scale into w for standardised data.
 * The size queries answer 0 for shapes that are not served.  Every check runs before any launch. */
#define VSX_PCA_MAX_D 4096 /* largest d of the PCA passes and of the logistic-regression passes below */
int64_t vsx_col_moments_ws_bytes(int64_t n, int32_t d);
int32_t vsx_col_moments(const float* x, int64_t n, int32_t d, double* mean, double* m2, void* ws, int64_t ws_bytes, vsx_stream_t stream);
int64_t vsx_gram_ws_bytes(int64_t n, int32_t d);
int64_t vsx_gram_rows_per_split(int64_t n, int32_t d);
int32_t vsx_gram_centered(const float* x, int64_t n, int32_t d, const double* mean, double* gram, void* ws, int64_t ws_bytes,
    vsx_stream_t stream);
int32_t vsx_center_project(const float* x, int64_t n, int32_t d, const double* mean, const float* w, int32_t k, float* z,
    vsx_stream_t stream);

/* The data passes of a Newton iteration on the weighted logistic objective (csrc/logreg.hip, csrc/pca.hip;
 * viscy_utils/evaluation/linear_classifier.py: sklearn LogisticRegression on frozen embeddings).  x, n, d, alignment, workspaces, the
 * absence of atomics and the refusals are those of the PCA passes above: every output is a pure function of the inputs.
 * logreg_rows: for every row i, in float64,
 *     z_i = (sum_j x_ij w_j) + b      w [d] float64 on the device; fma over the features 4 l .. 4 l + 3, 256 + 4 l .. of lane l in ascending
 *                                     order from 0, the 64 lanes added by the xor butterfly 32 .. 1, b last: one order for every alignment
 *     y = +1 where labels[i] == pos, else -1;  c = cp or cn accordingly;  m = y z;  e = exp(-|m|)
 *     sigma = 1 / (1 + e), 1 - sigma = e / (1 + e) for m >= 0, the two swapped for m < 0 (no cancellation)
 *     loss = c (log1p(e) + max(-m, 0));  r = -c y (1 - sigma) = dloss/dz;  s = c sigma (1 - sigma) = d2loss/dz2;  q = fl32(sqrt(s))
 *   z, r, s [n] float64, q [n] fp32, sums [3] float64 = {sum loss, sum r, sum s} (a wave owns a contiguous run of rows; its lane l adds rows
 *   l, 64 + l, .. of the run in ascending order, then the butterfly; the four waves of a workgroup 0 .. 3; then the workgroups l, l + 64, ..
 *   per lane and the butterfly); any of the five may be null.  With r, s, q and sums all
 *   null the call computes the margins z alone and labels may be null: the decision function, with the dot order of the fit.
 *   ws: vsx_logreg_rows_ws_bytes(n, d), needed where sums is not null.
 * wcolsum: out [m, d] float64 = sum_i v_ki x_ij for v [m, n] float64, 1 <= m <= 4: fma in float64, x read once for all m; the row
 *   split and fold of col_moments.  With v = {r, s} it yields the gradient X'r and the intercept column X's of the Hessian together.
 * gram_scaled: gram [d, d] float64 = sum_i fl32(q_i c_ij) fl32(q_i c_il) with c_ij = fl32(x_ij - mean_j) as in gram_centered, q [n] fp32;
 *   mean may be null (c_ij = x_ij).  The kernel, tiling, split plan (vsx_gram_rows_per_split, vsx_gram_ws_bytes), block sums and fold are
 *   gram_centered's; the one difference is the fp32 multiply where the slab goes to LDS.  With q = fl32(sqrt(s)) it is the Hessian block
 *   X' diag(s) X as a true Gram: symmetric bit for bit and positive semi-definite. */
int64_t vsx_logreg_rows_ws_bytes(int64_t n, int32_t d);
int32_t vsx_logreg_rows(const float* x, int64_t n, int32_t d, const double* w, double b, const int32_t* labels, int32_t pos, double cp,
    double cn, double* z, double* r, double* s, float* q, double* sums, void* ws, int64_t ws_bytes, vsx_stream_t stream);
int64_t vsx_wcolsum_ws_bytes(int64_t n, int32_t d, int32_t m);
int32_t vsx_wcolsum(const float* x, int64_t n, int32_t d, const double* v, int32_t m, double* out, void* ws, int64_t ws_bytes,
    vsx_stream_t stream);
int32_t vsx_gram_scaled(const float* x, int64_t n, int32_t d, const double* mean, const float* q, double* gram, void* ws, int64_t ws_bytes,
    vsx_stream_t stream);

/* The device passes of the temporal-smoothness evaluation (csrc/smoothness.hip; viscy_utils/evaluation/smoothness.py
 * compute_embeddings_smoothness and find_distribution_peak, viscy_utils/evaluation/distance.py compute_track_displacement).  No atomics;
 * every output is a pure function of the inputs, bit-identical from run to run.  Every check runs before any launch; anything not served
 * is refused with a non-zero status.
 * standardize: z_ij = fl32( double(fl32(double(x_ij) - mean_j)) / scale_j ), IEEE float64 subtraction and division: what sklearn's
 *   StandardScaler.transform does to a float32 matrix with its float64 mean_ and scale_ (X -= mean_; X /= scale_).  x, z [n, d] fp32
 *   row-major, any 4-byte alignment, z may be x; mean, scale [d] float64; n >= 1, d >= 1.
 * pair_dist: out[p] float64 = the distance of rows u = x[pi[p]] and v = x[pj[p]] of x [n, d] fp32 (any 4-byte alignment; one 16-byte read
 *   per four features where d % 4 == 0 and x is 16-byte aligned, else scalar reads of the same features into the same lanes).  One wave per
 *   pair.  ONE summation order for every alignment, vsx_logreg_rows': lane l adds features 4 l .. 4 l + 3, 256 + 4 l .. in ascending order
 *   from 0.0, then the 64 lane sums s are added by the xor butterfly, s_l <- s_l + s_(l xor o) for o = 32, 16, .. 1.
 *     metric VSX_PAIR_COSINE     uv = sum u_c v_c, uu = sum u_c^2, vv = sum v_c^2 in float64 (each product is exact, so fma = mul, add);
 *                                out = 1 - uv / (max(sqrt(uu), eps) * max(sqrt(vv), eps)), the product, division and difference each rounded
 *                                once.  eps = 0: a zero row gives 0 / 0 = NaN (scipy's cdist); eps = 1e-12: F.normalize's rule, distance 1.
 *     metric VSX_PAIR_EUCLIDEAN  out = sqrt(sum (u_c - v_c)^2): the float64 difference, its square and the add are rounded separately
 *                                (no fma); eps is not read.  i == j gives exactly 0.
 *   1 <= P < 2^33, 1 <= n < 2^31, d >= 1, eps >= 0.  A pair with an index outside [0, n) reads nothing and gets NaN.
 * kde_gauss: out[g] = sum_i exp(-a (grid[g] - data[i])^2), float64 throughout, library exp; the normalisation 1 / (n sqrt(2 pi cov)) with
 *   a = 1 / (2 cov) is the caller's.  data [n], grid [m], out [m] float64, 1 <= n < 2^31, 1 <= m <= 2^20.  A workgroup keeps a tile of
 *   VSX_KDE_TILE grid points in registers and streams one chunk of data through LDS; a thread adds its chunk's terms in ascending i from
 *   0.0; the per-chunk partials [chunks][m] go to ws and are added in ascending chunk order.  The chunk length is a whole number of slabs
 *   of VSX_KDE_CHUNK data, chosen so that tiles x chunks is about 2048 workgroups, and is a function of (n, m) alone:
 *   chunks = vsx_kde_gauss_ws_bytes(n, m) / (8 m); n <= VSX_KDE_CHUNK is one chunk.  ws: 8-byte aligned, any contents,
 *   vsx_kde_gauss_ws_bytes(n, m) bytes (0 for shapes that are not served). */
#define VSX_PAIR_COSINE 0
#define VSX_PAIR_EUCLIDEAN 1
#define VSX_KDE_TILE 512   /* grid points of a workgroup of vsx_kde_gauss */
#define VSX_KDE_CHUNK 1024 /* data per LDS slab of vsx_kde_gauss; chunks are whole slabs */
int32_t vsx_standardize(const float* x, const double* mean, const double* scale, float* z, int64_t n, int32_t d, vsx_stream_t stream);
int32_t vsx_pair_dist(const float* x, int32_t n, const int32_t* pi, const int32_t* pj, int64_t P, int32_t d, int32_t metric, double eps,
    double* out, vsx_stream_t stream);
int64_t vsx_kde_gauss_ws_bytes(int64_t n, int64_t m);
int32_t vsx_kde_gauss(const double* data, int64_t n, const double* grid, int64_t m, double a, double* out, void* ws, int64_t ws_bytes,
    vsx_stream_t stream);

/* The device passes of the clustering evaluation (csrc/clustering.hip + f64_tile.h; viscy_utils/evaluation/clustering.py
 * pairwise_distance_matrix, dbscan_clustering, knn_accuracy).  x [N, d] fp32 row-major, any 4-byte alignment (one 16-byte read per four
 * features where d % 4 == 0 and x is 16-byte aligned, else scalar reads of the same features), 1 <= N <= 65535 * VSX_F64_TILE,
 * 1 <= d <= 2^20.  The dots are float64 throughout, on v_mfma_f64_16x16x4_f64: a workgroup forms a VSX_F64_TILE x VSX_F64_TILE tile from
 * chunks of VSX_F64_KC features converted to float64 where they are staged; a product of two fp32 values is exact in float64.  ONE
 * summation order for every (row, column), tile position and entry point, written down in f64_tile.h: ascending chunks from +0.0, eight
 * MFMA steps of four features per chunk.  No kernel waits on another workgroup, every loop has a bound known at launch, no atomics; every
 * output buffer may hold any contents on entry and is a pure function of the inputs.  Every check runs before any launch; anything not
 * served is refused with a non-zero status.
 * row_sqnorm_f64: norms[i] = dot_ii, computed as the diagonal of a tile: the bits that any tile holds for the dot of row i with itself,
 *   and, for two bit-identical rows i and j, for dot_ij.
 * pdist_f64: out[(i - r0) ld + (j - c0)] float64 for r0 <= i < r1, c0 <= j < c1 (0 <= r0 < r1 <= N, likewise c; ld >= c1 - c0), norms from
 *   row_sqnorm_f64.  i == j gives exactly 0.  Otherwise, every operation rounded once (no contraction):
 *     VSX_PDIST_COSINE       1 - dot_ij * (inv_i * inv_j), inv = 1 / max(sqrt(n), 1e-12): F.normalize's rule, a zero row is at distance 1
 *     VSX_PDIST_SQEUCLIDEAN  max((n_i + n_j) - 2 dot_ij, 0)
 *     VSX_PDIST_EUCLIDEAN    the correctly rounded sqrt of that
 *   d_ij == d_ji bit for bit; two bit-identical rows are at Euclidean distance exactly 0 (n_i + n_j = 2 dot_ij exactly); a block equals the
 *   matching slice of the whole matrix bit for bit.
 * eps_graph: adj uint64 [N][W], W = ceil(N / 64): bit b of word w of row i is 1 iff j = 64 w + b < N and (i == j or the SQEUCLIDEAN value
 *   <= eps2); bits past N are 0; deg[i] = the popcount of row i.  The words are ballots written by ordinary vector stores.  eps2 finite, >= 0.
 * cc_round: one round of connected components over the edges between core rows (core [N] uint8, 0 / 1): changed[0] = 0; then every core row
 *   takes the smallest label among itself and its core neighbours; then labels[i] <- labels[labels[i]] up to 32 times.  changed[0] = 1
 *   (plain stores) iff a label was lowered.  The caller starts with labels[i] = i and repeats until changed[0] == 0, at most N + 1 rounds
 *   (a round settles every row one more edge away from its component's smallest core index).  Labels move in place by plain stores; the
 *   fixed point, labels[i] = the smallest core index of the component of core row i, does not depend on scheduling.
 * dbscan_finish: out[i] = cid[labels[i]] for a core row; for any other row the smallest cid[labels[j]] over its core neighbours j, or -1
 *   where it has none.  cid [N] int32: the exclusive prefix count of the roots (core rows with labels[i] == i) in ascending index. */
#define VSX_F64_TILE 64 /* rows of either operand per tile of the float64 engine */
#define VSX_F64_KC 32   /* features per staged chunk of the float64 engine */
#define VSX_PDIST_COSINE 0
#define VSX_PDIST_EUCLIDEAN 1
#define VSX_PDIST_SQEUCLIDEAN 2
int32_t vsx_row_sqnorm_f64(const float* x, int32_t N, int32_t d, double* norms, vsx_stream_t stream);
int32_t vsx_pdist_f64(const float* x, const double* norms, int32_t N, int32_t d, int32_t metric, int32_t r0, int32_t r1, int32_t c0,
    int32_t c1, double* out, int64_t ld, vsx_stream_t stream);
int32_t vsx_eps_graph(const float* x, const double* norms, int32_t N, int32_t d, double eps2, uint64_t* adj, int32_t* deg,
    vsx_stream_t stream);
int32_t vsx_cc_round(const uint64_t* adj, const uint8_t* core, int32_t* labels, int32_t N, int32_t* changed, vsx_stream_t stream);
int32_t vsx_dbscan_finish(const uint64_t* adj, const uint8_t* core, const int32_t* labels, const int32_t* cid, int32_t N, int32_t* out,
    vsx_stream_t stream);

/* Test stage (cytoland/engine.py:334-392, csrc/test_metrics.hip): the sums behind the regression metrics of VSUNet.test_step in one
 * read of an image pair, and SSIM over the windows that lie inside the image.
 * P, T: `planes` fp32 images of H rows x W columns each, element (pl, y, x) at pl * plane_stride + y * row_stride + x (strides in
 *   elements, row_stride >= W is not required of the caller: any non-negative strides that stay inside the buffer), 4-byte aligned.
 * pair_sums: out [VSX_PAIR_SUMS] float64 = { sum p, sum t, sum p^2, sum t^2, sum p t, sum |p - t|, sum (p - t)^2, min p, max p,
 *   min t, max t, sum over rows of cos(row), rows }; a row is one line along X of one plane and
 *   cos = p.t / (max(|p|, 1e-8) max(|t|, 1e-8)) (F.cosine_similarity(dim=-1)).  Every accumulator is float64.  A wave owns whole
 *   rows (VSX_PAIR_SUMS_WAVES waves per workgroup, VSX_PAIR_SUMS_VEC elements per lane and load where both rows are 16-byte
 *   aligned); at most VSX_PAIR_SUMS_MAX_WGS workgroups, a function of planes * H alone, write one partial each to ws
 *   (vsx_pair_sums_ws_bytes) and one launch folds them in workgroup order.  No atomics: the same bits in every run.
 * ssim_window: separable weights wy [Ky], wx [Kx] (device fp32; odd sizes in [3, VSX_SSIM_MAX_K], H >= Ky, W >= Kx), c = {c1, c2} and
 *   shift = {s_p, s_t} device floats.  With x = p - s_p, y = t - s_t formed where a tile is staged and E the weighted window mean:
 *     mx = E[x], my = E[y], vxx = max(E[x^2] - mx^2, 0), vyy = max(E[y^2] - my^2, 0), vxy = E[xy] - mx my, mp = mx + s_p, mt = my + s_t
 *     ssim = ((2 mp mt + c1) (2 vxy + c2)) / ((mp^2 + mt^2 + c1) (vxx + vyy + c2))                                 (fp32)
 *   for each of the (H - Ky + 1) x (W - Kx + 1) windows inside a plane: what torchmetrics' structural_similarity_index_measure
 *   averages after it has cropped its reflect padding.  sums [planes] float64 = the sum of each plane's map (one partial per
 *   VSX_SSIM_TILE x VSX_SSIM_TILE tile of outputs in ws, vsx_ssim_window_ws_bytes, folded in a fixed order, no atomics);
 *   map: NULL, or [planes][H - Ky + 1][W - Kx + 1] fp32. */
#define VSX_PAIR_SUMS 13
#define VSX_PAIR_SUMS_WAVES 4
#define VSX_PAIR_SUMS_VEC 4
#define VSX_PAIR_SUMS_MAX_WGS 2048
#define VSX_SSIM_MAX_K 33
#define VSX_SSIM_TILE 32
int64_t vsx_pair_sums_ws_bytes(int64_t planes, int32_t H);
int32_t vsx_pair_sums(const float* P, int64_t p_plane_stride, int64_t p_row_stride, const float* T, int64_t t_plane_stride,
    int64_t t_row_stride, int64_t planes, int32_t H, int32_t W, double* out, void* ws, int64_t ws_bytes, vsx_stream_t stream);
int64_t vsx_ssim_window_ws_bytes(int64_t planes, int32_t H, int32_t W, int32_t Ky, int32_t Kx);
int32_t vsx_ssim_window(const float* P, int64_t p_plane_stride, int64_t p_row_stride, const float* T, int64_t t_plane_stride,
    int64_t t_row_stride, int64_t planes, int32_t H, int32_t W, const float* wy, int32_t Ky, const float* wx, int32_t Kx,
    const float* c, const float* shift, double* sums, float* map, void* ws, int64_t ws_bytes, vsx_stream_t stream);

/* The device passes of `viscy preprocess` (csrc/preprocess.hip; viscy_utils/meta_utils.py generate_normalization_metadata /
 * generate_fg_masks, viscy_utils/mp_utils.py get_val_stats; host layer viscy_amd/preprocess.py).  A source plane set is [Z, H, W] of
 * src_dtype (VSX_PG_F32 / U16 / I16 / U8) with ELEMENT strides z_stride >= 0 and y_stride >= W, x contiguous; it may be a view into a
 * [T, C, Z, H, W] block, and the kernels trust the strides.  Integer sources convert to fp32 exactly, float32 is copied bit for bit.
 * No floating-point atomics, no allocation, synchronisation or device-to-host copy; every output is a pure function of the inputs
 * (and, for the moments, of x's 16-byte alignment), bit-identical from run to run.  Every check runs before any launch; anything
 * not served is refused with a non-zero status.
 * grid_sample: out [Z][ceil(H / g)][ceil(W / g)] fp32, out[z, i, j] = src[z, i g, j g]: numpy's `[:, ::g, ::g]`.  g >= 1; g > H gives one row.
 * median3x3: the 3 x 3 median of every plane with scipy.ndimage's default mode="reflect" (d c b a | a b c d): what
 *   median_filter(size=(1, 1, 3, 3)) and size=(1, 3, 3) compute; planes never mix; H or W of 1 and 2 repeat the rows there are.
 *   Exactly one of out / mask is given: out [Z][H][W] fp32 (the source must be VSX_PG_F32), or mask [Z][H][W] uint8 = median >= thr ? 1 : 0
 *   from a source of any dtype.  A wave walks down a strip of VSX_MEDIAN_COLS columns, VSX_MEDIAN_ROWS rows with three rows in
 *   registers.  The input is ASSUMED NaN-free (scipy's result with a NaN is unspecified as well); of -0.0 / +0.0 either may come back.
 * nan_moments: x [n] fp32, 4-byte aligned, 1 <= n <= 2^31 - 1; ws: vsx_nan_moments_ws_bytes(n) bytes, 8-byte aligned, no
 *   initialisation needed (one partial of VSX_MOMENTS_PART_BYTES per chunk of VSX_MOMENTS_CHUNK values, plain stores, then ONE
 *   fixed-order fold); out [4] float64 on the device.
 *     pass 1: out = {count of non-NaN values, their min, max, sum}; no such value: {0, +inf, -inf, 0}.  integral = 1 (the values are
 *             integers with |x| <= 65535: uint8 / uint16 / int16 stores): isums [2] int64 = {sum x, sum x^2}, exact, since
 *             65535^2 (2^31 - 1) < 2^63.
 *     pass 2: out = {sum (x - mean)^2, sum (x - mean), 0, 0} over the non-NaN values, x - mean formed in float64.
 * hist_int: x [n] fp32 holding integers; counts [nbins] uint64, counts[v - lo] = how many x equal v; 1 <= nbins <= 65536.  A value
 *   outside [lo, lo + nbins) (a NaN included) is not counted.  counts is zeroed by the call.  uint64 counts set no limit on n; private
 *   32-bit LDS counters serve nbins <= VSX_HIST_LDS_BINS (a workgroup sees fewer than 2^32 values), global integer atomics beyond.
 * hist_edges: edges [nbins + 1] ascending float64 on the device, 2 <= nbins <= VSX_HIST_EDGES_MAX_BINS; counts [nbins] uint64, zeroed by
 *   the call: bin i counts edges[i] <= x < edges[i + 1], the last bin is closed on the right, anything else (a NaN included) is
 *   dropped: np.histogram's rule.  A value is placed by an arithmetic guess and then walked to the bin the table defines, so the
 *   counts are those of the edges whatever the guess rounds to. */
#define VSX_MEDIAN_COLS 62
#define VSX_MEDIAN_ROWS 32
#define VSX_MOMENTS_CHUNK 8192
#define VSX_MOMENTS_PART_BYTES 48
#define VSX_HIST_LDS_BINS 8192
#define VSX_HIST_EDGES_MAX_BINS 1024
int32_t vsx_grid_sample(const void* src, int32_t src_dtype, int64_t z_stride, int64_t y_stride, int32_t Z, int32_t H, int32_t W,
    int32_t g, float* out, vsx_stream_t stream);
int32_t vsx_median3x3(const void* src, int32_t src_dtype, int64_t z_stride, int64_t y_stride, int32_t Z, int32_t H, int32_t W,
    float* out, uint8_t* mask, float thr, vsx_stream_t stream);
int64_t vsx_nan_moments_ws_bytes(int64_t n);
int32_t vsx_nan_moments(const float* x, int64_t n, int32_t pass, int32_t integral, double mean, double* out, int64_t* isums,
    void* ws, int64_t ws_bytes, vsx_stream_t stream);
int32_t vsx_hist_int(const float* x, int64_t n, int32_t lo, int32_t nbins, uint64_t* counts, vsx_stream_t stream);
int32_t vsx_hist_edges(const float* x, int64_t n, const double* edges, int32_t nbins, uint64_t* counts, vsx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSX_H */
