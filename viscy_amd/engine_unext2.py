"""Kernel schedule of UNeXt2 forward / backward on MI355X (see viscy_amd/unext2.py).

``Engine`` owns
  * the flat fp32 master-parameter buffer (every nn.Parameter of the model is a view into it, in
    *reverse forward order* so gradient buckets become ready front-to-back during backward) and
    the matching flat gradient buffer;
  * ``prepare()``: per-step re-layout of master weights into GEMM operands (compute dtype);
  * ``forward()`` / ``backward_stages()``: the launch sequences, as loops over the stages.  Each layer is a pair of adjacent
    methods (``_stem_*``, ``_down_*``, ``_preconv_*``, ``_up_*``, ``_block_*``, a row of ``_HEADS`` per head kind) joined by a
    named record of what the forward keeps; a block's GRN-MLP runs by its ``_MlpPlan``.  Only ``backward_stages`` yields.

``ops`` is the kernel backend: ``viscy_amd.ops`` (HIP, the only backend the product ever uses).
Tests may inject a reference implementation of the same call surface to validate the schedule
itself on CPU (tests/ref_ops.py); nothing in the package does.
"""

from __future__ import annotations

import math
import os
from collections import namedtuple
from typing import NamedTuple

import torch
from torch import Tensor

from . import _lib as L
from . import ops as hip_ops
from .flat import FlatEngine, engine_apply


class _BlockW:
    """prepared operands + parameter handles of one ConvNeXt-V2 block"""

    __slots__ = ("C", "p", "dw_w", "W1f", "W1fT", "b1f", "W2", "W2T", "v1", "fc2_w", "fc2_b", "grn_w", "grn_b", "dp", "img", "img2", "b2f")


class _ProjW:
    __slots__ = ("cin", "cout", "taps", "ln", "conv", "W", "WT")


FWD_UNFUSED, FWD_PAIR, FWD_FC1 = 0, 1, 2


class _MlpPlan(NamedTuple):
    """how one ConvNeXt block runs its GRN-MLP: decided once per block and forward (``_plan_mlp``), saved with the block's
    tensors and executed as saved by the backward"""

    fwd: int        # FWD_UNFUSED (GEMMs) | FWD_PAIR (inference: statistics + output pass) | FWD_FC1 (training fc1, MODE 2 / 6)
    ln_in: bool     # the block LayerNorm rides in the prologue of the fused passes (no LayerNorm pass over y)
    keep_h: bool    # the forward stores the pre-activation h (False: the dh pass recomputes it, MODE 6 here / 5 or 7 there)
    keep_xh: bool   # ... and the normalised rows x^ (False: it keeps y, mean, rstd and the backward re-normalises, MODE 7)
    bwd: int        # 0 unfused | fused dh pass (MODE 4 / 5 / 7), GRN statistics from 1: the per-sample products dout_b^T g_b, 2:
    tn_stats: bool  # the fc2 weight-gradient TN GEMM if tn_stats, else the MODE 3 pass


def _plan_mlp(flag: int, supported, C: int, hw: int, M: int, B: int, dt: torch.dtype, training: bool, ln_bwd_ok: bool,
              tn_stats_ok: bool) -> _MlpPlan:
    """Pure: the plan from the value of ``mlp_fused``, ``supported(mode)`` (csrc/mlp.hip serves MODE ``mode`` — None: the
    inference pair — at this shape) and whether the data-gradient GEMM's LayerNorm epilogue / the TN GEMM's GRN statistics
    serve the shape.  Flag bits: 0 inference pair, 1 training fc1 (fc2 stays the unfused GEMM, which reads the stored g), 3 the
    backward writes dh once (MODE 4) instead of dz and then dh, 5 LayerNorm in the prologue, 6 h recomputed instead of stored
    (needs the fused backward), 7 (with 5 and 6) x^ not stored either (needs the LayerNorm epilogue, C <= 256: the stand-alone
    LayerNorm backward reads a stored x^).  bf16 only."""
    if dt != torch.bfloat16:
        flag = 0
    if not training:
        pair = bool(flag & 1) and supported(None)
        return _MlpPlan(FWD_PAIR if pair else FWD_UNFUSED, pair and bool(flag & 32), False, False, 0, False)
    fc1 = bool(flag & 2) and supported(2)
    bwd = 0
    if flag & 8 and supported(4):
        if B * C * 4 * C * 4 <= (512 << 20) and C >= 96 and hw % 64 == 0:  # the B products [C, 4C] (fp32) fit 512 MB
            bwd = 1
        elif supported(3):
            bwd = 2
    recompute_h = bool(flag & 64) and bwd != 0 and supported(5) and supported(6)
    drop_xh = bool(flag & 128) and bool(flag & 32) and recompute_h and supported(7) and ln_bwd_ok
    ln_in = fc1 and bool(flag & 32)
    return _MlpPlan(FWD_FC1 if fc1 else FWD_UNFUSED, ln_in, not (fc1 and recompute_h), not (ln_in and drop_xh), bwd,
                    bwd == 2 and bool(tn_stats_ok))


# what a block's forward keeps for its backward: xh = the normalised rows [M, C] (plan.keep_xh), else y = the depthwise output
# and mean = its row means; h = the pre-activation [M, 4C] (plan.keep_h), gact = gelu(h).  (The first nine fields are in the
# order readers by position know: tests/test_gpu_model.py takes colsq as item 5.)
_BlockSaved = namedtuple("_BlockSaved", "x xh rstd h gact colsq s rows dpm plan y mean")
_NarrowSaved = namedtuple("_NarrowSaved", "x y colsq s")
# the other layers.  Stem: P = the patch matrix (kind "narrow": the input stack), f = the LayerNorm's input, kind = "patch" |
# "narrow" | "blockdiag" (ratio > 1), conv = the module that ran.  Down / Up: x / cat -> LayerNorm -> xn (None: narrow projection)
_StemSaved = namedtuple("_StemSaved", "P f mean rstd kind conv kern")
_DownSaved = namedtuple("_DownSaved", "x xn mean rstd")
_UpSaved = namedtuple("_UpSaved", "cat xn mean rstd c_up sc pre_in")
_HeadConvSaved = namedtuple("_HeadConvSaved", "hin U stats fh fw")
_HeadShuffleSaved = namedtuple("_HeadShuffleSaved", "fh fw")
_EmbedSaved = namedtuple("_EmbedSaved", "pooled mean rstd emb z0 y1 sm1 sr1 z3 y4 sm4 sr4 training fh fw fc")


class _ZeroArena:
    """One zero-filled fp32 allocation per pass, handed out as views: the ~130 small reduction targets of a step
    (GRN sums, bias / weight gradient staging, InstanceNorm sums) used to cost one fill launch each (154 launches,
    0.74 ms per step in the kernel trace).  Sized from the previous pass with the same key; a pass that needs more than
    was recorded falls back to individual allocations (and records the new size)."""

    def __init__(self, dev, numel: int, ops):
        self.dev, self.ops = dev, ops
        self.buf = self._zeros(numel) if numel > 0 else None
        self.off = 0
        self.used = 0

    def _zeros(self, *shape) -> Tensor:
        return self.ops.zeros(*shape, device=self.dev)  # vsx_fill_f32: the captured step holds no ATen fill

    def take(self, *shape) -> Tensor:
        n = math.prod(int(d) for d in shape)
        n_al = (n + 63) // 64 * 64  # 256-byte granules: every view stays 16-byte aligned
        self.used += n_al
        if self.buf is not None and self.off + n_al <= self.buf.numel():
            v = self.buf[self.off:self.off + n].view(*shape)
            self.off += n_al
            return v
        return self._zeros(*shape)


class Engine(FlatEngine):
    name = "UNeXt2"

    def __init__(self, model, ops=None):
        ops = hip_ops if ops is None else ops
        self._hip = ops is hip_ops  # the HIP backend: the only one that has the library's flags and fused GRN-MLP passes
        self._mlp_flag = 0          # `mlp_fused` as read by the forward in flight (0 on any other backend)
        self.cfg = model.cfg
        self.head = self.cfg.get("head", "conv")  # "conv" | "shuffle" | "embed": a row of _HEADS
        self._zeros4c = {}       # C -> zeros(4C): the identity GRN of ConvNeXt-V1 blocks
        self._dp_inject = None   # tests: list of per-sample branch scales [B], consumed in forward block order
        self._za = None          # zero arena of the pass in flight
        self._za_need = {}       # (pass, B, H, W) -> fp32 elements the pass took last time
        self._prepared_for = None
        self.W = None
        super().__init__(model, ops)  # flat buffers in reverse forward order (head first, stem last)

    # ------------------------------------------------------------------ parameter ordering
    def _stage_params_rev(self, stage):
        ps = []
        for blk in reversed(list(stage.blocks)):
            v1 = hasattr(blk, "gamma")  # ConvNeXt-V1 block: layer scale in front, no GRN
            ps += ([blk.gamma] if v1 else []) + [blk.mlp.fc2.weight, blk.mlp.fc2.bias]
            ps += ([] if v1 else [blk.mlp.grn.weight, blk.mlp.grn.bias]) + [blk.mlp.fc1.weight, blk.mlp.fc1.bias]
            ps += [blk.norm.weight, blk.norm.bias, blk.conv_dw.weight, blk.conv_dw.bias]
        if not isinstance(stage.downsample, torch.nn.Identity):
            ps += [stage.downsample[1].weight, stage.downsample[1].bias, stage.downsample[0].weight, stage.downsample[0].bias]
        return ps

    def _param_order(self):
        m = self.model
        ps = self._HEADS[self.head][0](self)
        self._bucket_marks = [0]
        if self.head != "embed":  # ContrastiveEncoder: pooled-embedding tail instead of decoder + head
            for st in reversed(list(m.decoder.decoder_stages)):
                ps += self._stage_params_rev(st.conv)
                if getattr(st, "pre_conv", None) is not None:  # decoder_upsample_pre_conv: runs before the stage in the forward
                    ps += [st.pre_conv.weight, st.pre_conv.bias]
        self._bucket_marks.append(len(ps))  # bucket 0 = head + decoder (or the embedding tail)
        for i in (3, 2):
            ps += self._stage_params_rev(getattr(m.encoder_stages, f"stages_{i}"))
        self._bucket_marks.append(len(ps))  # bucket 1 = encoder stages 3, 2
        for i in (1, 0):
            ps += self._stage_params_rev(getattr(m.encoder_stages, f"stages_{i}"))
        ps += [m.encoder_stages.stem_1.weight, m.encoder_stages.stem_1.bias, m.stem.conv.weight, m.stem.conv.bias]
        if getattr(m, "stem2d", None) is not None:  # FCMAE: the Conv2d stem of Z == 1 inputs
            ps += [m.stem2d.weight, m.stem2d.bias]
        self._bucket_marks.append(len(ps))  # bucket 2 = encoder stages 1, 0 + stem
        return ps

    def encoder_frozen(self) -> bool:
        """``model.encoder.requires_grad_(False)`` (cytoland engine.py:204-206, the FCMAE fine-tuning recipe): every
        parameter from the encoder bucket on (encoder stages + stem: the tail of the flat buffer) is frozen — the backward
        stops after the decoder and the optimiser skips the tail.  Any other pattern of frozen parameters is not built."""
        lo = self._bucket_marks[1]
        frozen = [not p.requires_grad for p in self.order]
        if not any(frozen):
            return False
        if all(frozen[lo:]) and not any(frozen[:lo]):
            return True
        raise NotImplementedError("only a fully frozen encoder (+ stem) with a fully trainable decoder / head is built")

    def trainable_numel(self) -> int:
        return self.offsets[self._bucket_marks[1]] if self.encoder_frozen() else self.flat.numel()

    # ------------------------------------------------------------------ weight preparation
    def _prep_block(self, blk, dt, need_bwd):
        o = self.ops
        w = _BlockW()
        C = blk.conv_dw.weight.shape[0]
        w.C, w.p = C, blk
        w.dw_w = torch.empty((49, C), dtype=torch.float32, device=self.device)
        o.transpose_f32(blk.conv_dw.weight, w.dw_w, C, 49, False)
        need_t = need_bwd and C >= 16  # the narrow block kernels (C < 16) read W1f / W2 only
        w.W1f, w.W1fT = o.prep_weight(blk.mlp.fc1.weight, 4 * C, C, 1, dt, want=True, want_t=need_t,
                                      gamma=blk.norm.weight)
        w.b1f = o.matvec(blk.mlp.fc1.weight, blk.norm.bias, blk.mlp.fc1.bias, 4 * C, C)
        w.dp = 0.0  # stochastic-depth rate of this block (set by prepare() from cfg["drop_path"])
        w.img = None  # fragment-major LDS image of (W1f, W2) for the fused GRN-MLP kernel (prepare())
        w.v1 = hasattr(blk, "gamma")
        if w.v1:
            # ConvNeXt-V1: y = x + gamma * fc2(gelu(fc1(.))) — the layer scale is folded into fc2 (vsx_layer_scale_fold) and
            # the block runs the V2 schedule with a zero (identity) GRN; the fc2 gradients are unfolded in _block_bwd
            w.fc2_w, w.fc2_b = o.layer_scale_fold(blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.gamma)
            z = self._zeros4c.get(C)
            if z is None:
                z = self._zeros4c[C] = torch.zeros(4 * C, dtype=torch.float32, device=self.device)
            w.grn_w = w.grn_b = z
        else:
            w.fc2_w, w.fc2_b = blk.mlp.fc2.weight, blk.mlp.fc2.bias
            w.grn_w, w.grn_b = blk.mlp.grn.weight, blk.mlp.grn.bias
        w.W2, w.W2T = o.prep_weight(w.fc2_w, C, 4 * C, 1, dt, want=True, want_t=need_t)
        # fc2 bias with the GRN beta folded in (b2 + W2 . beta): what fc2 needs when the GRN scale lives in per-sample weights
        w.b2f = o.matvec(w.fc2_w, w.grn_b, w.fc2_b, C, 4 * C) if dt == torch.bfloat16 and C > 64 else None
        w.img2 = None  # image of (W2^T, W2) for the block backward without a stored dz
        return w

    def _prep_proj(self, ln, conv, dt, need_bwd):
        o = self.ops
        w = _ProjW()
        cout, cin = conv.weight.shape[0], conv.weight.shape[1]
        taps = conv.weight.shape[2] * conv.weight.shape[3]
        w.cin, w.cout, w.taps, w.ln, w.conv = cin, cout, taps, ln, conv
        if cout < 16:  # narrow stage: the fused projection reads the fp32 master weight itself
            w.W = w.WT = None
        else:
            w.W, w.WT = o.prep_weight(conv.weight, cout, cin, taps, dt, want=True, want_t=need_bwd)
        return w

    def _prep_stem(self, conv, dt, narrow_stem):
        """-> the [Cout, K] operand of a stem's patch GEMM; None: the narrow stem runs"""
        o, K = self.ops, conv.weight[0].numel()
        if narrow_stem and K % 8:
            # 2x2 stem (K = Cin * kz * 4): the patch is not a whole number of 16-byte bf16 vectors — the narrow stem reads the
            # fp32 stack and the master weight directly (csrc/narrow.hip), no patch matrix, no GEMM operand
            return None
        Wp, _ = o.prep_weight(conv.weight, conv.weight.shape[0], K, 1, dt)
        if dt == torch.bfloat16 and K % 32:
            o.flush()  # pad_cols reads what the task list has yet to write
            # K = 80 (the 5x4x4 single-channel stem) is not a whole number of 32-deep MFMA slabs: the projection fell to
            # the generic GEMM (2.9 ms at B = 512, 250 GB/s).  Zero-padded to 96 on both operands it runs on the lean one.
            Wp = o.pad_cols(Wp, (K + 31) // 32 * 32)
        return Wp

    def prepare(self, dt: torch.dtype, need_bwd: bool, mlp_flag: int = 0):
        o = self.ops
        with o.batch():  # ~150 weight-space jobs -> a handful of task-list launches (ops.batch)
            W = self._prepare_ops(dt, need_bwd)
        if dt == torch.bfloat16 and mlp_flag:
            # fragment-major weight images of the fused GRN-MLP kernels, every block's in one task list (their inputs are the
            # outputs of the list above); a block whose shape the fused kernels do not serve simply never reads its image.
            # `_plan_mlp` fuses a pass only where mode None / 2 / 4 is served (and the backward only with bit 3), from the same
            # flag value: every image a plan of this forward reads is packed here
            bwd_img = need_bwd and bool(mlp_flag & 8)
            with o.batch():
                for _, blocks in list(W["enc"]) + list(W["dec"]):
                    for w in blocks:
                        if any(o.mlp_supported(w.C, 1 << 20, 1 << 20, dt, md) for md in (None, 2, 4)):  # a width the kernels serve
                            w.img = o.mlp_pack(w.W1f, w.W2, w.C)
                            if bwd_img:
                                w.img2 = o.mlp_pack(w.W2T, w.W2, w.C)
        self.W, self._prepared_for = W, (dt, need_bwd)
        return W

    def _prepare_ops(self, dt: torch.dtype, need_bwd: bool):
        m, cfg, o = self.model, self.cfg, self.ops
        W = {"dt": dt}
        # stem: [Cout3d, K] (block-diagonal expansion when the stem keeps D' > 1 depth slabs)
        sw, Dp = m.stem.conv.weight, cfg["ratio"]
        narrow_stem = self.head == "shuffle" and tuple(cfg["stem_kernel"][1:]) == (2, 2)  # built only for the 2x2 FCMAE
        if Dp == 1:
            W["stem_W"], W["stem_b"] = self._prep_stem(m.stem.conv, dt, narrow_stem), m.stem.conv.bias
        else:  # rare configuration (Z = 15): tiny weight-space expansion done with tensor ops
            co3, K = sw.shape[0], sw[0].numel()
            we = torch.zeros((co3, Dp, Dp, K), dtype=torch.float32, device=self.device)
            for d in range(Dp):
                we[:, d, d, :] = sw.detach().reshape(co3, K)
            W["stem_W"] = we.reshape(co3 * Dp, Dp * K).to(dt).contiguous()
            W["stem_b"] = m.stem.conv.bias.detach().repeat_interleave(Dp).contiguous()
        s2 = getattr(m, "stem2d", None)
        if s2 is not None:  # FCMAE: Conv2d stem of Z == 1 inputs (fcmae.py:348-353,369-370) — the same patch GEMM with kz = 1
            W["stem2d_W"], W["stem2d_b"] = self._prep_stem(s2, dt, narrow_stem), s2.bias
        enc = []
        for i in range(4):
            st = getattr(m.encoder_stages, f"stages_{i}")
            proj = None
            if not isinstance(st.downsample, torch.nn.Identity):
                proj = self._prep_proj(st.downsample[0], st.downsample[1], dt, need_bwd)
            enc.append((proj, [self._prep_block(b, dt, need_bwd) for b in st.blocks]))
        rates = cfg.get("drop_path")  # per encoder block, forward order (timm: linspace over all blocks; FCMAE: constant)
        if rates:
            flat_blocks = [bw for _, blocks in enc for bw in blocks]
            assert len(rates) == len(flat_blocks)
            for bw, r in zip(flat_blocks, rates):
                bw.dp = float(r)
        W["enc"] = enc
        dec = []
        if self.head != "embed":
            for us in m.decoder.decoder_stages:
                st = us.conv
                proj = self._prep_proj(st.downsample[0], st.downsample[1], dt, need_bwd)
                dec.append((proj, [self._prep_block(b, dt, need_bwd) for b in st.blocks]))
            # decoder_upsample_pre_conv: Conv2d(C, C, 3, padding 1) in front of each pixel shuffle = patch matrix x [C, 9C]
            pre = []
            for us in m.decoder.decoder_stages:
                pc = getattr(us, "pre_conv", None)
                if pc is None:
                    pre.append(None)
                else:
                    cpc = pc.weight.shape[0]
                    pre.append((pc, *o.prep_weight(pc.weight, cpc, cpc, 9, dt, want=True, want_t=need_bwd)))
            W["dec_pre"] = pre
        W["dec"] = dec
        self._HEADS[self.head][1](self, W, dt, need_bwd)
        return W

    def _head_dtype(self, dt: torch.dtype) -> torch.dtype:
        """PixelToVoxelHead works on 4 * out_channels channels per depth plane: with out_channels odd (1 -> 1 virtual staining)
        that is not a whole number of 16-byte bf16 vectors, and the (small) head then runs in fp32 behind a bf16 trunk"""
        if dt == torch.bfloat16 and self.model.head.conv[0].conv.weight.shape[1] % 8:
            return torch.float32
        return dt

    # ------------------------------------------------------------------ block forward / backward
    def _plan(self, C, hw, M, B, dt, training: bool) -> _MlpPlan:
        o, flag = self.ops, self._mlp_flag
        ask = training and dt == torch.bfloat16 and flag != 0  # the two shape queries only matter to a fused training block
        return _plan_mlp(flag, lambda mode: o.mlp_supported(C, hw, M, dt, mode), C, hw, M, B, dt, training,
                         ask and bool(L.lib().vsx_gemm_nt_ln_bwd_supported(M, C, 4 * C, L.dtype_code(dt))),
                         ask and o.tn_grn_stats_ok(M, C, 4 * C, hw, dt))

    def _block_fwd(self, x, w, B, H, Wd, dt, save, rows=None):
        """One ConvNeXt-V2 block on a dense channels-last map [B*H*W, C].  ``rows = (idx, inv, keep, L)`` selects the FCMAE
        masked path (fcmae.py:196-230): ``x`` arrives already multiplied by the mask, the depthwise convolution runs dense,
        LayerNorm / GRN-MLP run on the L kept tokens per sample only (compact rows), and the result is scattered back into
        zeros and added to the (masked) shortcut."""
        if w.C < 16:
            return self._block_fwd_narrow(x, w, B, H, Wd, save, rows)
        o = self.ops
        C, M = w.C, B * H * Wd
        blk = w.p
        hw = H * Wd
        y = o.dwconv7_fwd(x, w.dw_w, blk.conv_dw.bias, B, H, Wd, C)
        xres = x
        if rows is not None:
            idx, inv, _, Lr = rows
            M, hw = B * Lr, Lr
            y = o.rows_select(y, idx, M, C)      # masked_patchify
            xres = o.rows_select(x, idx, M, C)   # the shortcut of the kept tokens
        plan = self._plan(C, hw, M, B, dt, save is not None)
        # plan.ln_in: the block LayerNorm rides in the prologue of the fused GRN-MLP passes (csrc/mlp.hip) — no LayerNorm pass
        # over y, and in inference no normalised rows in memory at all
        mean = rstd = None
        if plan.ln_in:
            xh = None
        else:
            xh, _, rstd = o.ln_fwd(y, None, None, M, C, 1e-6, need_mean=False)
            y = None
        colsq = self._za.take(B, 4 * C)
        # stochastic depth (timm DropPath, scale_by_keep): the whole branch of a sample is dropped with probability dp and
        # the survivors are scaled by 1 / (1 - dp); training mode only.  One device-side draw per block (graph-capturable).
        dpm = None
        if w.dp > 0.0 and self.model.training:
            inj = self._dp_inject
            dpm = inj.pop(0) if inj else (torch.rand(B, device=x.device) < (1.0 - w.dp)).float() / (1.0 - w.dp)
        assert plan.fwd == FWD_UNFUSED or w.img is not None  # packed by prepare() from the flag value this plan was made from
        if plan.fwd == FWD_PAIR:
            # inference: the 4C-wide hidden never leaves the CU (csrc/mlp.hip) — pass 1 = GRN statistics, pass 2 = fc1
            # recomputed, GELU, GRN, fc2, bias, shortcut
            src, lne = (y, 1e-6) if plan.ln_in else (xh, 0.0)
            o.mlp_stats(src, w.img, w.b1f, colsq, M, C, hw, ln_eps=lne)
            s = o.grn_scale(colsq, w.grn_w)
            out = o.mlp_out(src, w.img, w.b1f, s, w.grn_b, w.fc2_b, xres, dpm, M, C, hw, ln_eps=lne)
            if rows is not None:
                out = o.rows_select(out, rows[1], B * H * Wd, C)
            return out
        # fc1 writes the pre-activation h (needed for gelu' in backward) AND the activation g = gelu(h):
        # fc2, the fc2 weight gradient and the GRN statistics path all consume g, so GELU is evaluated once
        # (inference keeps the activation only: C = NULL skips the pre-activation store, a third of the block's 4C-wide traffic)
        if plan.fwd == FWD_FC1:
            # training fc1 on the fused kernel's statistics pass, which also stores h and g (csrc/mlp.hip MODE 2).
            # not plan.keep_h: the pre-activation h is NOT stored — the backward's dh pass recomputes it from the C-wide
            # normalised rows (csrc/mlp.hip MODE 6 here, MODE 5 there): one 4C-wide write and one 4C-wide read less per block
            if plan.ln_in:
                # not plan.keep_xh: ... and neither is x^ — the backward re-normalises from y and the row means
                first, rstd, h, gact = o.mlp_fc1_ln(y, w.img, w.b1f, colsq, M, C, hw, 1e-6, store_h=plan.keep_h,
                                                    store_xh=plan.keep_xh)
                xh, y, mean = (first, None, None) if plan.keep_xh else (None, *first)
                del first
            else:
                h, gact = o.mlp_fc1(xh, w.img, w.b1f, colsq, M, C, hw, store_h=plan.keep_h)
        else:
            h = torch.empty((M, 4 * C), dtype=dt, device=x.device) if save is not None else None
            gact = torch.empty((M, 4 * C), dtype=dt, device=x.device)
            o.gemm("nt", xh, w.W1f, h, M, 4 * C, C, C, C, 4 * C, dtype=dt, epi=L.EPI_BIAS_GELU_SQ, bias=w.b1f, red0=colsq,
                   hw=hw, C2=gact)
        s = o.grn_scale(colsq, w.grn_w)
        out = torch.empty((M, C), dtype=dt, device=x.device)
        if dt == torch.bfloat16 and C > 64 and hw % 128 == 0 and hw // 128 >= 8:
            # large feature maps: fold the GRN affine into per-sample fc2 weights,
            #   (g·s_b + β)·W2ᵀ = g·(W2·diag(s_b))ᵀ + W2·β,
            # so fc2 is a plain GEMM (the operand prologue costs +60 % on these launches); B·C·4C extra weight bytes
            # are small next to the M·4C activation bytes when a sample spans >= 8 row tiles
            Ws = o.scale_weight_samples(w.fc2_w, s, dt)
            b2 = w.b2f
            if b2 is None:
                b2 = o.matvec(w.fc2_w, w.grn_b, w.fc2_b, C, 4 * C)
                o.flush()
            o.gemm("nt", gact, Ws, out, M, C, 4 * C, 4 * C, 4 * C, C, dtype=dt, hw=hw, b_bstride=C * 4 * C,
                   epi=L.EPI_BIAS_RES, bias=b2, res=xres, ldr=C, rscale=dpm)
        else:
            o.gemm("nt", gact, w.W2, out, M, C, 4 * C, 4 * C, 4 * C, C, dtype=dt, pro=L.PRO_GRN, grn_s=s,
                   grn_b=w.grn_b, hw=hw, epi=L.EPI_BIAS_RES, bias=w.fc2_b, res=xres, ldr=C, rscale=dpm)
        if rows is not None:
            out = o.rows_select(out, rows[1], B * H * Wd, C)  # masked_unpatchify: zero rows where masked (shortcut is 0 there)
        if save is not None:
            save.append(_BlockSaved(x, xh, rstd, h, gact, colsq, s, rows, dpm, plan, y, mean))
        return out

    def _block_fwd_narrow(self, x, w, B, H, Wd, save, rows):
        """ConvNeXt-V2 block of C < 16 channels (the last decoder stage of a 2x2-stem FCMAE: C = 4 or 8) on the narrow family
        (csrc/narrow.hip): pass 1 = depthwise 7x7 + LayerNorm + fc1 + GELU + GRN sums (stores only the C-wide depthwise output y),
        pass 2 = the same recomputed from y + GRN + fc2 + bias + shortcut.  The 4C-wide hidden never goes to memory."""
        o, C = self.ops, w.C
        if rows is not None or w.v1 or (w.dp > 0.0 and self.model.training):
            raise NotImplementedError("narrow ConvNeXt blocks are built for dense ConvNeXt-V2 decoder stages only")
        colsq = self._za.take(B, 4 * C)
        y = o.narrow_block_fwd1(x, w.dw_w, w.p.conv_dw.bias, w.W1f, w.b1f, colsq, B, H, Wd, C)
        s = o.grn_scale(colsq, w.grn_w)
        out = o.narrow_block_fwd2(y, x, w.W1f, w.b1f, s, w.grn_b, w.W2, w.fc2_b, B, H, Wd, C)
        if save is not None:
            save.append(_NarrowSaved(x, y, colsq, s))
        return out

    def _block_bwd_narrow(self, dout, w, saved, B, H, Wd):
        """backward of ``_block_fwd_narrow``: (A) fc2 weight / bias gradient and the GRN statistics, (B) GELU' + fc1 + LayerNorm
        backward -> dy with the folded fc1 gradient, (C) depthwise data gradient + shortcut and the 7x7 weight / bias gradient;
        the folded gradients are unfolded exactly as in the generic path"""
        o, g = self.ops, self.g
        C, blk = w.C, w.p
        x, y, colsq, s = saved
        PS = self._za.take(2, B, 4 * C)
        o.narrow_block_bwd_a(dout, y, w.W1f, w.b1f, s, w.grn_b, w.W2, g(blk.mlp.fc2.weight), g(blk.mlp.fc2.bias), PS[0], PS[1],
                             B, H, Wd, C)
        t = o.grn_bwd_stats(colsq, PS[0], w.grn_w, g(blk.mlp.grn.weight), Sb=PS[1], dbeta=g(blk.mlp.grn.bias))
        dW1f, db1f = self._za.take(4 * C, C), self._za.take(4 * C)
        dy = o.narrow_block_bwd_b(dout, y, w.W1f, w.b1f, s, t, w.W2, dW1f, db1f, B, H, Wd, C)
        self._fc1_unfold(blk, dW1f, db1f, C)
        ddw = self._za.take(49, C)
        dx = o.narrow_block_bwd_c(dy, x, dout, w.dw_w, ddw, g(blk.conv_dw.bias), B, H, Wd, C)
        o.transpose_f32(ddw, g(blk.conv_dw.weight), 49, C, True)
        return dx

    def _fc1_unfold(self, blk, dW1f, db1f, C, rowsub=None):
        # unfold the LayerNorm affine: dW1 = dW1f·diag(γ) + db1f ⊗ β, dγ = Σ_r dW1f ⊙ W1, dβ = W1ᵀ db1f, db1 = db1f
        o, g = self.ops, self.g
        o.unprep_grad(dW1f, g(blk.mlp.fc1.weight), 4 * C, C, 1, gamma=blk.norm.weight, W=blk.mlp.fc1.weight,
                      dgamma=g(blk.norm.weight), u=db1f, beta=blk.norm.bias, rowsub=rowsub)
        o.matvec_t_add(blk.mlp.fc1.weight, db1f, g(blk.norm.bias), 4 * C, C)
        o.transpose_f32(db1f, g(blk.mlp.fc1.bias), 4 * C, 1, True)  # g(b1) += db1f (a [4C, 1] "transpose": no ATen launch in the step)

    def _block_bwd(self, dout, w, saved, B, H, Wd, dt):
        # four phases on the schedule the forward planned (``saved.plan``), whatever `mlp_fused` says by now (a pass whose flag
        # bit was cleared in between is refused by the library); dz and dx^ are released here, where they die, not by a phase
        if w.C < 16:
            return self._block_bwd_narrow(dout, w, saved, B, H, Wd)
        o, C, sv = self.ops, w.C, saved
        M, hw, dfull = B * H * Wd, H * Wd, dout
        if sv.rows is not None:  # masked path: the MLP branch only sees the gradient of the kept tokens
            M, hw = B * sv.rows[3], sv.rows[3]
            dout = o.rows_select(dfull, sv.rows[0], M, C)
        if sv.dpm is not None:  # the branch saw dout * (0 | 1/keep) of its sample; the shortcut keeps the full gradient (dfull)
            dout = o.scale_rows_samples(dout, sv.dpm, M, C, hw)
        PS, dgw, dgb = self._mlp_bwd_fc2(dout, w, sv, B, M, C, hw, dt)
        dz, db1f, u1 = self._mlp_bwd_dh(dout, w, sv, PS, dgw, dgb, M, C, hw, dt)
        dy, dxh, dW1f = self._mlp_bwd_fc1(dz, w, sv, M, C, dt)
        del dz
        self._fc1_unfold(w.p, dW1f, db1f, C, rowsub=u1)
        if dy is None:
            dy = o.ln_bwd(dxh, sv.xh, None, sv.rstd, None, None, None, None, M, C)
        del dxh
        if sv.rows is not None:
            dy = o.rows_select(dy, sv.rows[1], B * H * Wd, C)  # adjoint of the gather: zero-filled scatter
        return self._dw_bwd(dy, dfull, w, sv, B, H, Wd)

    def _mlp_bwd_fc2(self, dout, w, sv, B, M, C, hw, dt):
        """phase 1: fc2 weight / bias gradient, with the GRN statistics PS = {P_b, S_b} where they ride in it; -> PS, dgw, dgb"""
        o, g, blk, plan, gact, s = self.ops, self.g, w.p, sv.plan, sv.gact, sv.s
        if w.v1:  # gradients of the folded (Ws, bs) and of the (constant, zero) GRN land in scratch
            dW2, db2 = self._za.take(C, 4 * C), self._za.take(C)
            dgw, dgb = self._za.take(4 * C), self._za.take(4 * C)
        else:
            dW2, db2 = g(blk.mlp.fc2.weight), g(blk.mlp.fc2.bias)
            dgw, dgb = g(blk.mlp.grn.weight), g(blk.mlp.grn.bias)
        PS = self._za.take(2, B, 4 * C)
        if plan.bwd == 1:
            # dz = dout·W2 is LINEAR in dout, so everything the backward needs from "Σ over the sample of dz·(something)" comes
            # out of the per-sample products Q_b = dout_bᵀ·g_b that the weight gradient computes anyway:
            #   P_b = Σ_hw dz·g = Σ_c W2[c,:]·Q_b[c,:],  S_b = Σ_hw dz = Σ_c W2[c,:]·cs_b[c],  dW2 = Σ_b s_b·Q_b + cs⊗β
            # — one TN GEMM without operand prologue (30 % faster than the prologue form) and a tiny reduction replace the
            # fc2 weight-gradient GEMM AND the statistics pass over the 4C-wide tensors; dz is never formed for them
            Qb = torch.empty((B, C, 4 * C), dtype=torch.float32, device=dout.device)
            csb = torch.empty((B, C), dtype=torch.float32, device=dout.device)
            o.gemm("tn", gact, dout, Qb, M, C, 4 * C, 4 * C, C, 4 * C, dtype=dt, hw=hw, colsum=csb, b_bstride=C * 4 * C)
            o.grn_q_reduce(Qb, csb, w.W2, s, w.grn_b, PS[0], PS[1], dW2, db2)
            del Qb
        elif plan.tn_stats:
            # round 5: the products are too large to store (C = 384 at B = 512), but each per-sample TILE of Q_b passes through the
            # accumulators of the fc2 weight-gradient GEMM anyway — that launch scales it by s_b into dW2 and contracts it with its
            # W2 tile into P_b on the way (csrc/gemm.hip, gemm_tn_fast_kernel PRO == 2).  The statistics pass that recomputed dz for
            # P and S (csrc/mlp.hip MODE 3, a full M x 4C x C contraction per block) is gone; S only ever fed dbeta = sum_b S_b =
            # (column sums of dout) . W2, a matvec on the sums this launch produces for the bias gradient.
            # ConvNeXt-V1 blocks: db2 is zeroed scratch that `layer_scale_unfold` reads in a DIRECT launch right below, while
            # `transpose_f32` is only queued inside the backward segment's task-list batch — the GEMM writes the column sums into
            # db2 itself there (fc2.bias gradient and its share of dgamma were lost on v1 backbones at this path)
            cs = db2 if w.v1 else self._za.take(C)
            o.gemm("tn", gact, dout, dW2, M, C, 4 * C, 4 * C, C, 4 * C, dtype=dt, pro=L.PRO_GRN, grn_s=s, grn_b=w.grn_b, hw=hw,
                   colsum=cs, aux=w.W2, ldx=4 * C, red0=PS[0])
            if not w.v1:
                o.transpose_f32(cs, db2, C, 1, True)     # db2 += cs
            o.matvec_t_add(w.fc2_w, cs, dgb, C, 4 * C)   # dbeta += W2^T cs
        else:
            # fc2: weight gradient (Z recomputed in the operand prologue) + bias gradient
            o.gemm("tn", gact, dout, dW2, M, C, 4 * C, 4 * C, C, 4 * C, dtype=dt, pro=L.PRO_GRN, grn_s=s,
                   grn_b=w.grn_b, hw=hw, colsum=db2)
        if w.v1:
            o.layer_scale_unfold(dW2, db2, blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.gamma, g(blk.mlp.fc2.weight),
                                 g(blk.mlp.fc2.bias), g(blk.gamma))
        return PS, dgw, dgb

    def _mlp_bwd_dh(self, dout, w, sv, PS, dgw, dgb, M, C, hw, dt):
        """phase 2: -> (dz holding dh, its column sums db1f, u1 = Σ_r dh' · mean where the forward kept y instead of x^)"""
        o, plan, s = self.ops, sv.plan, sv.s
        # not keep_xh: the forward stored y and the row means, no normalised rows (MODE 7); cs2 = {column sums of dh, u = sum_r dh' * mean}
        cs2 = None if plan.keep_xh else self._za.take(2, 4 * C)
        db1f, u1 = (self._za.take(4 * C), None) if cs2 is None else (cs2[0], cs2[1])
        if plan.bwd:
            # the 4C-wide dz is never written: the statistics came from the per-sample products above; this pass recomputes
            # dz = dout·W2 tile by tile (K = C is short) and writes dh directly (csrc/mlp.hip MODE 4) — one 4C-wide write
            # where the unfused pair (dz GEMM, then GRN / GELU backward over it) has two
            img2 = w.img2
            assert img2 is not None  # plan.bwd != 0 needs bit 3 and MODE 4 at the forward: prepare() packed it then
            if plan.bwd == 2 and not plan.tn_stats:  # statistics by recomputing dz tile by tile (P = Σ dz·g, S = Σ dz), nothing stored
                o.mlp_bwd_stats(dout, img2, sv.gact, PS[0], PS[1], M, C, hw)
            if plan.tn_stats:
                t = o.grn_bwd_stats(sv.colsq, PS[0], w.grn_w, dgw)
            else:
                t = o.grn_bwd_stats(sv.colsq, PS[0], w.grn_w, dgw, Sb=PS[1], dbeta=dgb)
            if not plan.keep_xh:  # h recomputed from y re-normalised on chip; dz holds dh * rstd (MODE 7)
                dz = o.mlp_bwd_dh_ln(dout, sv.y, sv.mean, sv.rstd, img2, w.img, w.b1f, s, t, cs2, M, C, hw)
            elif not plan.keep_h:  # h recomputed on chip from the normalised rows (MODE 5)
                dz = o.mlp_bwd_dh_re(dout, sv.xh, img2, w.img, w.b1f, s, t, db1f, M, C, hw)
            else:
                dz = o.mlp_bwd_dh(dout, img2, sv.h, s, t, db1f, M, C, hw)  # (named dz: it holds dH)
        else:
            # fc2 data gradient dZ, with Σ dZ·gelu(h) (GRN statistics path) and Σ dZ (GRN beta gradient)
            dz = torch.empty((M, 4 * C), dtype=dt, device=dout.device)
            o.gemm("nt", dout, w.W2T, dz, M, 4 * C, C, C, C, 4 * C, dtype=dt, epi=L.EPI_DZ, aux=sv.gact, ldx=4 * C, red0=PS[0],
                   red1=PS[1], hw=hw)
            t = o.grn_bwd_stats(sv.colsq, PS[0], w.grn_w, dgw, Sb=PS[1], dbeta=dgb)
            o.grn_gelu_bwd(dz, sv.h, s, t, db1f, M, 4 * C, hw)  # dz now holds dH
        return dz, db1f, u1

    def _mlp_bwd_fc1(self, dz, w, sv, M, C, dt):
        """phase 3, the two GEMMs over dz: fc1 data gradient and folded weight gradient; -> (dy | None, dx^ | None, dW1f)"""
        o, xh = self.ops, sv.xh
        if not sv.plan.keep_xh:
            # dz = dh * rstd: the accumulator is rstd * dx^ already, x^ is re-formed from y in the epilogue; the weight gradient
            # contracts dz with y itself, dh^T x^ = dz^T y - u (x) 1 — the rank-1 term goes in the unfold (`rowsub`)
            xh = sv.y
        # where one column tile spans the row (C <= 256) the block LayerNorm's backward rides in the data-gradient GEMM's epilogue
        # (VSX_EPI_LN_BWD): dx^ is never written, the LayerNorm-backward launch and two C-wide passes go
        # (a HIP kernel only; None: the shape is not served)
        dy = o.dgrad_ln_bwd(dz, w.W1fT, xh, sv.rstd, M, C, 4 * C, mean=sv.mean) if self._hip else None
        assert dy is not None or sv.plan.keep_xh  # the plan drops x^ only where this epilogue serves the shape
        dxh = None
        if dy is None:
            dxh = torch.empty((M, C), dtype=dt, device=dz.device)
            o.gemm("nt", dz, w.W1fT, dxh, M, C, 4 * C, 4 * C, 4 * C, C, dtype=dt)
        dW1f = self._za.take(4 * C, C)
        o.gemm("tn", xh, dz, dW1f, M, 4 * C, C, C, 4 * C, C, dtype=dt)
        return dy, dxh, dW1f

    def _dw_bwd(self, dy, dfull, w, sv, B, H, Wd):
        """phase 4: depthwise 7x7 data gradient + the shortcut's gradient ``dfull``, and the 7x7 weight / bias gradient"""
        o, g, C, blk = self.ops, self.g, w.C, w.p
        dx = o.dwconv7_bwd_data(dy, w.dw_w, dfull, B, H, Wd, C)
        ddw = self._za.take(49, C)
        o.dwconv7_bwd_weight(dy, sv.x, ddw, g(blk.conv_dw.bias), B, H, Wd, C)
        o.transpose_f32(ddw, g(blk.conv_dw.weight), 49, C, True)
        if sv.rows is not None:
            dx = o.rows_select(dx, sv.rows[2], B * H * Wd, C)  # adjoint of `x *= unmasked` (shortcut and dwconv input alike)
        return dx

    # ------------------------------------------------------------------ one dense layer's backward
    def _dense_bwd(self, x, d, WT, dW, db, M, N, K, dt, patch2=None):
        """out[M, N] = x[M, K]·Wᵀ + b: dW += dᵀx by a TN GEMM with the column sums of d into db, then dx = d·W by an NT GEMM
        through the prepared transpose WT.  patch2 = (gh, gw): x is the 2x2-patch gather (A_PATCH2) of a [4M, K / 4] map, to
        which dx is scattered back; the weight gradient is staged in the arena and unfolded into dW tap by tap"""
        o, ldx, ka, kc = self.ops, K, {}, {}
        if patch2 is not None:
            ldx = K // 4
            ka = dict(a_mode=L.A_PATCH2, gh=patch2[0], gw=patch2[1], cs=ldx)
            kc = dict(c_mode=L.A_PATCH2, c_cs=ldx, gh=patch2[0], gw=patch2[1])
        stage = dW if patch2 is None else self._za.take(N, K)
        o.gemm("tn", x, d, stage, M, N, K, ldx, N, K, dtype=dt, colsum=db, **ka)
        if patch2 is not None:
            o.unprep_grad(stage, dW, N, ldx, 4)
        dx = torch.empty((M * K // ldx, ldx), dtype=dt, device=d.device)
        o.gemm("nt", d, WT, dx, M, K, N, N, N, ldx, dtype=dt, **kc)
        return dx

    # ------------------------------------------------------------------ layers: forward, backward and the record between them
    def _stem_fwd(self, x, W, flat_stem, dt, sv):
        """patch gather + projection GEMM (or the narrow stem), then the encoder's stem_1 LayerNorm2d; -> [B*h*w, C0]"""
        o, cfg, m = self.ops, self.cfg, self.model
        stem_W, stem_b, conv = (W["stem2d_W"], W["stem2d_b"], m.stem2d) if flat_stem else (W["stem_W"], W["stem_b"], m.stem.conv)
        kern = (1 if flat_stem else cfg["stem_kernel"][0], *cfg["stem_kernel"][1:])
        if stem_W is None:  # narrow stem (K not a multiple of 8): no patch matrix; the backward re-reads the stack
            P, kind = x.contiguous(), "narrow"
            f = o.narrow_stem_fwd(P, conv.weight, stem_b, kern, dt)
        else:
            P, kind = o.stem_im2col(x.contiguous(), kern, dt, ld=stem_W.shape[1]), "patch"
            if cfg["ratio"] > 1 and not flat_stem:
                kind = "blockdiag"  # stem_W is the block-diagonal expansion over the ratio depth slabs (_prepare_ops)
            M0, C0, K0 = P.shape[0], cfg["dims"][0], P.shape[1]
            f = torch.empty((M0, C0), dtype=dt, device=x.device)
            o.gemm("nt", P, stem_W, f, M0, C0, K0, K0, K0, C0, dtype=dt, epi=L.EPI_BIAS, bias=stem_b)
        ln1 = m.encoder_stages.stem_1
        cur, mean, rstd = o.ln_fwd(f, ln1.weight, ln1.bias, f.shape[0], f.shape[1])
        if sv is not None:
            sv["stem"] = _StemSaved(P, f, mean, rstd, kind, conv, kern)
        return cur

    def _stem_bwd(self, d, s, dt):
        o, g, Dp, ln1 = self.ops, self.g, self.cfg["ratio"], self.model.encoder_stages.stem_1
        P, f, conv, (M0, C0), K0 = s.P, s.f, s.conv, s.f.shape, s.P.shape[1]
        df = o.ln_bwd(d, f, s.mean, s.rstd, ln1.weight, None, g(ln1.weight), g(ln1.bias), M0, C0)
        if s.kind == "narrow":  # patches recomputed from the stored stack (P is x here)
            o.narrow_stem_wgrad(P, df, g(conv.weight), g(conv.bias), s.kern)
        elif s.kind == "patch":
            Kw = conv.weight[0].numel()  # the patch matrix may carry zero-padded tail columns (lda = K0 >= Kw)
            o.gemm("tn", P, df, g(conv.weight), M0, C0, Kw, K0, C0, Kw, dtype=dt, colsum=g(conv.bias))
        else:  # block-diagonal expansion (ratio > 1): the gradient of the expanded weight, folded back onto its diagonal blocks
            co3, K = C0 // Dp, K0 // Dp
            dWe, dbe = self._za.take(C0, K0), self._za.take(C0)
            o.gemm("tn", P, df, dWe, M0, C0, K0, K0, C0, K0, dtype=dt, colsum=dbe)
            dWe = dWe.view(co3, Dp, Dp, K)
            g(conv.weight).add_(torch.stack([dWe[:, dd, dd] for dd in range(Dp)], 0).sum(0).view_as(conv.weight))
            g(conv.bias).add_(dbe.view(co3, Dp).sum(1))

    def _down_fwd(self, cur, proj, B, ch, cw, dt, st_sv):
        """encoder downsampling onto the ch x cw grid: LayerNorm2d, then the 2x2 stride-2 convolution as a patch-gather GEMM"""
        o, cc = self.ops, proj.cin
        xn, mean, rstd = o.ln_fwd(cur, proj.ln.weight, proj.ln.bias, B * 4 * ch * cw, cc)
        nxt = torch.empty((B * ch * cw, proj.cout), dtype=dt, device=cur.device)
        o.gemm("nt", xn, proj.W, nxt, B * ch * cw, proj.cout, 4 * cc, cc, 4 * cc, proj.cout, dtype=dt,
               a_mode=L.A_PATCH2, gh=ch, gw=cw, cs=cc, epi=L.EPI_BIAS, bias=proj.conv.bias)
        st_sv["proj"] = _DownSaved(cur, xn, mean, rstd)
        return nxt

    def _down_bwd(self, d, proj, s, dskip, B, ch, cw, dt):
        """... and the gradient ``dskip`` that the decoder sent to this layer's input (the skip) rides in the LayerNorm backward"""
        o, g, cin = self.ops, self.g, proj.cin
        dxn = self._dense_bwd(s.xn, d, proj.WT, g(proj.conv.weight), g(proj.conv.bias), B * ch * cw, proj.cout, 4 * cin, dt, (ch, cw))
        return o.ln_bwd(dxn, s.x, s.mean, s.rstd, proj.ln.weight, dskip, g(proj.ln.weight), g(proj.ln.bias), B * 4 * ch * cw, cin)

    def _preconv_fwd(self, feat, pre, B, fh, fw, fc, dt):
        """decoder_upsample_pre_conv (MONAI SubpixelUpsample conv_block): dense 3x3 convolution at the low resolution"""
        o, (pc, Wp, _) = self.ops, pre
        col = o.im2col3x3(feat, B, fh, fw, fc)
        out = torch.empty((B * fh * fw, fc), dtype=dt, device=feat.device)
        o.gemm("nt", col, Wp, out, B * fh * fw, fc, 9 * fc, 9 * fc, 9 * fc, fc, dtype=dt, epi=L.EPI_BIAS, bias=pc.bias)
        return out

    def _preconv_bwd(self, d, pre, pre_in, B, lh, lw, dt):
        """weight gradient from the re-gathered patch matrix, data gradient through its transpose"""
        o, g, (pc, _, WpT) = self.ops, self.g, pre
        cpc, Ml = pc.weight.shape[0], B * lh * lw
        col = o.im2col3x3(pre_in, B, lh, lw, cpc)
        dWp = self._za.take(cpc, 9 * cpc)
        o.gemm("tn", col, d, dWp, Ml, cpc, 9 * cpc, 9 * cpc, cpc, 9 * cpc, dtype=dt, colsum=g(pc.bias))
        o.unprep_grad(dWp, g(pc.weight), cpc, cpc, 9)
        del col
        dcol = torch.empty((Ml, 9 * cpc), dtype=dt, device=d.device)
        o.gemm("nt", d, WpT, dcol, Ml, 9 * cpc, cpc, cpc, cpc, 9 * cpc, dtype=dt)
        return o.col2im3x3(dcol, B, lh, lw, cpc)

    def _up_fwd(self, feat, skip, pre, proj, B, fh, fw, fc, dt, st_sv):
        """decoder stage entry: (pre-convolution,) pixel shuffle x2 concatenated with the skip, LayerNorm2d, 1x1 projection"""
        o, (skip, sh, sw_, sc) = self.ops, skip
        assert sh == 2 * fh and sw_ == 2 * fw
        c_up = fc // 4
        low = feat if pre is None else self._preconv_fwd(feat, pre, B, fh, fw, fc, dt)
        cat = o.pixel_shuffle_cat_fwd(low, skip, B, fh, fw, c_up, sc)
        Mk, ccat = B * sh * sw_, c_up + sc
        if proj.cout < 16:  # narrow stage (2x2 stem: C = 4 or 8): LayerNorm + 1x1 projection in one pass, xn not stored
            cur, mean, rstd = o.narrow_proj_fwd(cat, proj.ln.weight, proj.ln.bias, proj.conv.weight, proj.conv.bias, Mk, ccat,
                                                proj.cout)
            xn = None
        else:
            xn, mean, rstd = o.ln_fwd(cat, proj.ln.weight, proj.ln.bias, Mk, ccat)
            cur = torch.empty((Mk, proj.cout), dtype=dt, device=feat.device)
            o.gemm("nt", xn, proj.W, cur, Mk, proj.cout, ccat, ccat, ccat, proj.cout, dtype=dt, epi=L.EPI_BIAS,
                   bias=proj.conv.bias)
        st_sv["proj"] = _UpSaved(cat, xn, mean, rstd, c_up, sc, None if pre is None else feat)
        return cur

    def _up_bwd(self, d, proj, s, B, sh, sw_, dt):
        """-> (gradient of the low map in front of the shuffle, gradient of the skip)"""
        o, g, Mk, ccat = self.ops, self.g, B * sh * sw_, s.c_up + s.sc
        if proj.cout < 16:
            dxn = o.narrow_proj_bwd(d, s.cat, s.mean, s.rstd, proj.ln.weight, proj.ln.bias, proj.conv.weight, g(proj.conv.weight),
                                    g(proj.conv.bias), Mk, ccat, proj.cout)
        else:
            dxn = self._dense_bwd(s.xn, d, proj.WT, g(proj.conv.weight), g(proj.conv.bias), Mk, proj.cout, ccat, dt)
        dcat = o.ln_bwd(dxn, s.cat, s.mean, s.rstd, proj.ln.weight, None, g(proj.ln.weight), g(proj.ln.bias), Mk, ccat)
        del dxn
        return o.pixel_shuffle_cat_bwd(dcat, B, sh // 2, sw_ // 2, s.c_up, s.sc)

    # ------------------------------------------------------------------ ContrastiveEncoder tail (contrastive/encoder.py:93-154)
    def _bn_groups_fwd(self, z, bn, training, relu, groups):
        """BatchNorm1d over ``groups`` consecutive row blocks, each with its own batch statistics and its own running-stat
        update, in order (== that many separate forward calls of the module)"""
        o = self.ops
        n = z.shape[0] // groups
        ys, sms, srs = [], [], []
        for gi in range(groups):
            y, sm, sr = o.bn1d_fwd(z[gi * n:(gi + 1) * n], bn.weight, bn.bias, bn.running_mean, bn.running_var, training, relu)
            ys.append(y); sms.append(sm); srs.append(sr)
        return (ys[0] if groups == 1 else torch.cat(ys)), sms, srs

    def _bn_groups_bwd(self, dy, z, y, bn, sms, srs, training, relu):
        o, g = self.ops, self.g
        groups = len(sms)
        n = z.shape[0] // groups
        dx = [o.bn1d_bwd(dy[gi * n:(gi + 1) * n], z[gi * n:(gi + 1) * n], y[gi * n:(gi + 1) * n], bn.weight, sms[gi], srs[gi],
                         g(bn.weight), g(bn.bias), training, relu) for gi in range(groups)]
        return dx[0] if groups == 1 else torch.cat(dx)

    def _embed_tail_params(self):
        t = self.model.tail
        return [t.bn4.weight, t.bn4.bias, t.fc3.weight, t.fc3.bias, t.bn1.weight, t.bn1.bias, t.fc0.weight, t.fc0.bias,
                t.norm.weight, t.norm.bias]

    def _embed_tail_prep(self, W, dt, need_bwd):
        o, t = self.ops, self.model.tail
        (E, Cf), P = t.fc0.weight.shape, t.fc3.weight.shape[0]
        W["fc0"], W["fc0T"] = o.prep_weight(t.fc0.weight, E, Cf, 1, torch.float32, want=True, want_t=need_bwd)
        W["fc3"], W["fc3T"] = o.prep_weight(t.fc3.weight, P, E, 1, torch.float32, want=True, want_t=need_bwd)

    def _embed_tail_fwd(self, feat3, B, dt, sv, bn_groups: int = 1):
        """global average pool -> LayerNorm (timm head.norm) = embedding; Linear -> BN -> ReLU -> Linear -> BN = projection.
        fp32 throughout ([B, 768]-sized tensors); BatchNorm statistics are those of THIS call's batch (the reference runs
        anchor and positive through separate forwards, dynaclr/engine.py:265-266); ``bn_groups = 2`` gives a concatenated
        [anchor; positive] batch exactly those per-call statistics while the trunk runs once."""
        o, m, W = self.ops, self.model, self.W
        feat, fh, fw, fc = feat3
        t, training = m.tail, bool(m.training)
        pooled = o.avgpool_rows_fwd(feat, B, fh * fw, fc)
        emb, mean, rstd = o.ln_fwd(pooled, t.norm.weight, t.norm.bias, B, fc)
        E, P = t.fc0.weight.shape[0], t.fc3.weight.shape[0]
        z0 = torch.empty((B, E), dtype=torch.float32, device=feat.device)
        o.gemm("nt", emb, W["fc0"], z0, B, E, fc, fc, fc, E, dtype=torch.float32, epi=L.EPI_BIAS, bias=t.fc0.bias)
        if B % bn_groups:
            raise ValueError(f"batch {B} is not divisible into {bn_groups} BatchNorm groups")
        y1, sm1, sr1 = self._bn_groups_fwd(z0, t.bn1, training, True, bn_groups)
        z3 = torch.empty((B, P), dtype=torch.float32, device=feat.device)
        o.gemm("nt", y1, W["fc3"], z3, B, P, E, E, E, P, dtype=torch.float32, epi=L.EPI_BIAS, bias=t.fc3.bias)
        y4, sm4, sr4 = self._bn_groups_fwd(z3, t.bn4, training, False, bn_groups)
        if training:
            t.bn1.num_batches_tracked += bn_groups
            t.bn4.num_batches_tracked += bn_groups
        if sv is not None:
            sv["head"] = _EmbedSaved(pooled, mean, rstd, emb, z0, y1, sm1, sr1, z3, y4, sm4, sr4, training, fh, fw, fc)
        return emb, y4

    def _embed_tail_bwd(self, sv, dout, dt, B):
        o, t, W, g, s = self.ops, self.model.tail, sv["W"], self.g, sv["head"]
        E, P, fc, f32 = t.fc0.weight.shape[0], t.fc3.weight.shape[0], s.fc, torch.float32
        demb, dproj = dout
        d_emb = demb.contiguous().float() if demb is not None else None
        if dproj is not None:
            dz3 = self._bn_groups_bwd(dproj.contiguous().float(), s.z3, s.y4, t.bn4, s.sm4, s.sr4, s.training, False)
            dy1 = self._dense_bwd(s.y1, dz3, W["fc3T"], g(t.fc3.weight), g(t.fc3.bias), B, P, E, f32)
            dz0 = self._bn_groups_bwd(dy1, s.z0, s.y1, t.bn1, s.sm1, s.sr1, s.training, True)
            de = self._dense_bwd(s.emb, dz0, W["fc0T"], g(t.fc0.weight), g(t.fc0.bias), B, E, fc, f32)
            d_emb = de if d_emb is None else d_emb + de
        if d_emb is None:
            d_emb = torch.zeros((B, fc), dtype=f32, device=s.emb.device)
        dpooled = o.ln_bwd(d_emb, s.pooled, s.mean, s.rstd, t.norm.weight, None, g(t.norm.weight), g(t.norm.bias), B, fc)
        return o.avgpool_rows_bwd(dpooled, B, s.fh * s.fw, fc, dt)

    # ------------------------------------------------------------------ PixelToVoxelHead ("conv") and the shuffle head
    def _head_conv_dims(self):
        cfg, hc = self.cfg, self.model.head.conv[0].conv
        return hc, hc.weight.shape[0], hc.weight.shape[1], cfg["out_channels"], cfg["out_stack_depth"], cfg["out_stack_depth"] + 2

    def _head_conv_params(self):
        hd = self.model.head.conv
        return [hd[1].weight, hd[1].bias, hd[0].adn.A.weight, hd[0].conv.weight, hd[0].conv.bias]

    def _head_conv_prep(self, W, dt, need_bwd):
        o, hdt, (hc, cmid, c3, _, Zo, _) = self.ops, self._head_dtype(dt), self._head_conv_dims()
        W["head_Wc"], _ = o.prep_weight(hc.weight, cmid, c3, 27, hdt, tapmode=1)
        if need_bwd:
            if hdt == torch.bfloat16 and c3 == 8 and cmid == 32 and Zo == 5:
                o.flush()  # reads head_Wc
                W["head_Wp"] = o.head_conv_dgrad_prep(W["head_Wc"])  # direct LDS-tiled dgrad (csrc/headconv.hip)
            W["head_Wd"] = o.prep_head_dgrad(hc.weight, cmid, c3, Zo, hdt)

    def _head_conv_fwd(self, feat3, B, dt, sv, bn_groups=1):
        o, m, W, hdt, (feat, fh, fw, _) = self.ops, self.model, self.W, self._head_dtype(dt), feat3
        hc, cmid, c3, cout, Zo, D7 = self._head_conv_dims()
        hin = o.head_shuffle_fwd(feat if hdt == dt else feat.float(), B, fh, fw, c3, D7, self.cfg["head_pool"])
        H2, W2, Mh = 2 * fh, 2 * fw, B * 4 * fh * fw
        stats = self._za.take(2, B, cmid)
        if o.head_conv_supported(H2, W2, c3, cmid, Zo, hdt):
            U = o.head_conv_fwd(hin, W["head_Wc"], hc.bias, stats[0], stats[1], B, H2, W2, c3, cmid, Zo)
        else:
            U = torch.empty((Mh, Zo * cmid), dtype=hdt, device=feat.device)
            o.gemm_z("nt", hin, W["head_Wc"], U, Mh, cmid, 27 * c3, D7 * c3, 27 * c3, Zo * cmid, dtype=hdt,
                     a_mode=L.A_CONV3, gh=H2, gw=W2, cs=3 * c3, nz=Zo, a_coff=[z * c3 for z in range(Zo)],
                     b_off=[0] * Zo, c_coff=[z * cmid for z in range(Zo)], epi=L.EPI_BIAS_STATS, bias=hc.bias,
                     red0=stats[0], red1=stats[1], hw=H2 * W2)
        w2 = m.head.conv[1].weight.view(4 * cout, cmid)
        out = o.head_out_fwd(U, stats[0], stats[1], w2, m.head.conv[1].bias, m.head.conv[0].adn.A.weight, B, H2, W2, Zo,
                             cmid, cout)
        if sv is not None:
            sv["head"] = _HeadConvSaved(hin, U, stats, fh, fw)
        return out

    def _head_conv_bwd(self, sv, dout, dt, B):
        """PixelToVoxelHead backward; returns the gradient of the decoder feature map."""
        o, cfg, m, g, W = self.ops, self.cfg, self.model, self.g, sv["W"]
        hc, cmid, c3, cout, Zo, D7 = self._head_conv_dims()
        trunk_dt, dt, dev = dt, self._head_dtype(dt), self.device
        hin, U, stats, fh, fw = sv["head"]
        H2, W2, Mh = 2 * fh, 2 * fw, B * 4 * fh * fw
        alpha = m.head.conv[0].adn.A.weight
        w2 = m.head.conv[1].weight.view(4 * cout, cmid)
        S = self._za.take(2, B, cmid)
        if dt == torch.bfloat16 and (cmid, cout) in ((32, 2), (64, 4)):
            # pass 1 with the 1x1x1 weight gradient folded in (voxel contraction on MFMA inside the kernel): the
            # [M5, cmid] activation is never written and the skinny TN GEMM over it disappears
            dv = o.head_out_bwd1_wgrad(U, stats[0], stats[1], w2, alpha, dout.contiguous().float(), S[0], S[1], g(alpha),
                                       g(m.head.conv[1].weight), g(m.head.conv[1].bias), B, H2, W2, Zo, cmid, cout)
        else:
            act, dv = o.head_out_bwd1(U, stats[0], stats[1], w2, alpha, dout.contiguous().float(), S[0], S[1], g(alpha), B,
                                      H2, W2, Zo, cmid, cout)
            o.gemm("tn", act, dv, g(m.head.conv[1].weight), Mh * Zo, 4 * cout, cmid, cmid, 4 * cout, cmid, dtype=dt,
                   colsum=g(m.head.conv[1].bias))
            del act
        dU = o.head_out_bwd2(U, stats[0], stats[1], w2, alpha, dv, S[0], S[1], B, H2, W2, Zo, cmid, cout)
        del dv
        dWc = self._za.take(cmid, 27 * c3)
        direct = "head_Wp" in W and o.head_conv_supported(H2, W2, c3, cmid, Zo, dt)
        if direct:
            o.head_conv_wgrad(hin, dU, dWc, g(hc.bias), B, H2, W2, c3, cmid, Zo)
        else:
            o.gemm_z("tn", hin, dU, dWc, Mh, cmid, 27 * c3, D7 * c3, Zo * cmid, 27 * c3, dtype=dt, a_mode=L.A_CONV3, gh=H2,
                     gw=W2, cs=3 * c3, nz=Zo, a_coff=[z * c3 for z in range(Zo)], b_off=[z * cmid for z in range(Zo)],
                     c_coff=[0] * Zo, colsum=g(hc.bias))
        o.unprep_grad(dWc, g(hc.weight), cmid, c3, 27, tapmode=1)
        if direct:
            dhin = o.head_conv_dgrad(dU, W["head_Wp"], B, H2, W2, c3, cmid, Zo)
        else:
            dhin = torch.empty((Mh, D7 * c3), dtype=dt, device=dev)
            zs = [min(max(zp - 2, 0), Zo - 3) for zp in range(D7)]
            o.gemm_z("nt", dU, W["head_Wd"], dhin, Mh, c3, 27 * cmid, Zo * cmid, 27 * cmid, D7 * c3, dtype=dt,
                     a_mode=L.A_CONV3, gh=H2, gw=W2, cs=3 * cmid, nz=D7, a_coff=[z * cmid for z in zs],
                     b_off=[zp * c3 * 27 * cmid for zp in range(D7)], c_coff=[zp * c3 for zp in range(D7)])
        del dU
        d = o.head_shuffle_bwd(dhin, B, fh, fw, c3, D7, cfg["head_pool"])
        del dhin
        return d if dt == trunk_dt else d.to(trunk_dt)

    def _head_shuffle_fwd(self, feat3, B, dt, sv, bn_groups=1):
        """PixelToVoxelShuffleHead (heads.py:656-685): pixel shuffle x s + pad-pool + reshape, parameter free"""
        cfg, (feat, fh, fw, _) = self.cfg, feat3
        out = self.ops.voxel_shuffle_fwd(feat, B, fh, fw, cfg["out_channels"], cfg["out_stack_depth"], cfg["stem_kernel"][-1], True)
        if sv is not None:
            sv["head"] = _HeadShuffleSaved(fh, fw)
        return out

    def _head_shuffle_bwd(self, sv, dout, dt, B):
        o, cfg, s, sxy = self.ops, self.cfg, sv["head"], self.cfg["stem_kernel"][-1]
        vs = o.voxel_shuffle_bwd
        if (cfg["out_channels"] * cfg["out_stack_depth"] * sxy * sxy) % (8 if dt == torch.bfloat16 else 4):
            vs = o.narrow_voxel_shuffle_bwd  # fewer channels than a 16-byte vector (2x2 pre-training head: 4)
        return vs(dout.contiguous().float(), B, s.fh, s.fw, cfg["out_channels"], cfg["out_stack_depth"], sxy, True, dt)

    # head kind -> (parameters in backward order, prepare(W, dt, need_bwd), forward(feat3, B, dt, sv, bn_groups), backward)
    _HEADS = {"conv": (_head_conv_params, _head_conv_prep, _head_conv_fwd, _head_conv_bwd),
              "shuffle": (lambda self: [], lambda self, W, dt, need_bwd: None, _head_shuffle_fwd, _head_shuffle_bwd),
              "embed": (_embed_tail_params, _embed_tail_prep, _embed_tail_fwd, _embed_tail_bwd)}

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, dt: torch.dtype, need_bwd: bool, masks=None, bn_groups: int = 1):
        """A forward WITHOUT a backward behind it (predict / validation / `InferStep` captures) forms the per-sample GRN and
        InstanceNorm sums in a fixed order (`ops.det_scope`: what the `det_reduce` flag does, for this thread only), as the
        reference's CPU path is deterministic: with fp32 atomics the bf16 forward at 2048^2 differs by 7e-3 of the output maximum
        from run to run, the fixed order costs 0.3 % of a pass (profiles/r05_det_reduce.txt).  Training forwards
        keep the atomics unless the `det_reduce` flag is set by hand;
        ``VSX_DET_INFER=0`` in the environment switches the automatic setting off."""
        auto = (not need_bwd) and self._hip and os.environ.get("VSX_DET_INFER", "1") != "0"
        with hip_ops.det_scope(auto):  # per thread: the process-wide flag is left alone
            return self._forward(x, dt, need_bwd, masks, bn_groups)

    def _forward(self, x: Tensor, dt: torch.dtype, need_bwd: bool, masks=None, bn_groups: int = 1):
        """``masks``: None (dense) or, per encoder stage, ``(idx, inv, keep, L)`` int32 row maps of the FCMAE mask at that
        stage's resolution (see ``viscy_amd.fcmae.stage_row_maps``)."""
        o, cfg = self.ops, self.cfg
        # read once: prepare() packs the weight images and every block of this forward plans its schedule from this value
        self._mlp_flag = L.lib().vsx_get_flag(b"mlp_fused") if self._hip else 0
        W = self.prepare(dt, need_bwd, self._mlp_flag)
        B, Cin, Z, H, Wd = x.shape
        za_key = ("fwd", B, H, Wd, masks is not None)
        self._za = za = _ZeroArena(x.device, self._za_need.get(za_key, 0), o)
        # FCMAE 2-D branch (fcmae.py:369-370): the reference runs conv2d whenever x.shape[2] == 1, whatever in_stack_depth is —
        # a 2-D FCMAE (in_stack_depth = 1) trains and loads its conv2d weights, never the conv3d ones
        flat_stem = Z == 1 and "stem2d_W" in W
        if Cin != cfg["in_channels"] or (Z != cfg["in_stack_depth"] and not flat_stem):
            raise ValueError(f"expected input (B,{cfg['in_channels']},{cfg['in_stack_depth']},Y,X), got {tuple(x.shape)}")
        _, ky, kx = cfg["stem_kernel"]
        if H % (8 * ky) or Wd % (8 * kx):
            raise ValueError(f"Y and X must be divisible by {8 * ky} (got {H}x{Wd}); VSUNet pads to a multiple of 64")
        # the prepared operands travel with the forward that used them: a later (no_grad / other dtype) forward re-prepares
        # self.W, and the backward of THIS forward must still see its own transposed weights
        sv = {"shape": (B, H, Wd), "dt": dt, "masked": masks is not None, "W": W} if need_bwd else None
        if need_bwd:
            self._count_forward()
        cur = self._stem_fwd(x, W, flat_stem, dt, sv)
        # ---- encoder
        feats, enc_sv, dec_sv = [], [], []
        ch, cw = H // ky, Wd // kx
        for i, (proj, blocks) in enumerate(W["enc"]):
            st_sv = {"blocks": []}
            if proj is not None:
                ch, cw = ch // 2, cw // 2
                cur = self._down_fwd(cur, proj, B, ch, cw, dt, st_sv)
            rows = None
            if masks is not None:
                rows = masks[i]
                # first block of the stage: `x *= unmasked` (fcmae.py:216-217); later blocks receive masked maps already
                cur = o.rows_select(cur, rows[2], B * ch * cw, cur.shape[1])
            for bw in blocks:
                cur = self._block_fwd(cur, bw, B, ch, cw, dt, st_sv["blocks"] if need_bwd else None, rows)
            feats.append((cur, ch, cw, cur.shape[1]))
            enc_sv.append(st_sv)
        # ---- decoder (none in front of the embedding tail), then the head
        feat, fh, fw, fc = feats[3]
        for k, (proj, blocks) in enumerate(W["dec"]):
            st_sv = {"blocks": []}
            cur = self._up_fwd(feat, feats[2 - k], W["dec_pre"][k], proj, B, fh, fw, fc, dt, st_sv)
            fh, fw = 2 * fh, 2 * fw
            for bw in blocks:
                cur = self._block_fwd(cur, bw, B, fh, fw, dt, st_sv["blocks"] if need_bwd else None)
            feat, fc = cur, proj.cout
            dec_sv.append(st_sv)
        out = self._HEADS[self.head][2](self, (feat, fh, fw, fc), B, dt, sv, bn_groups)
        if need_bwd:
            sv.update(enc=enc_sv, dec=dec_sv, feat_dims=[(a, b_, c) for (_, a, b_, c) in feats])
        self._za_need[za_key] = za.used
        return out, sv

    # ------------------------------------------------------------------ backward
    def backward_stages(self, sv, dout: Tensor):
        """Generator form of the backward schedule: yields the bucket index (0 = head + decoder, 1 = encoder stages 3-2,
        2 = stages 1-0 + stem) right after the last launch that writes into that bucket of the flat gradient buffer.
        ``viscy_amd.step.TrainStep`` captures the stretch between two yields as one hipGraph segment and issues the
        bucket's RCCL all-reduce between the segments."""
        # the gradient finalisers of a segment (unprep_grad / matvec_t_add / accumulating transposes: ~100 launches of 5 - 20 us
        # that only touch weight-sized data) are collected and launched as task lists when the segment ends (ops.batch_open)
        self.ops.batch_open()
        try:
            W, dt, (B, H, Wd) = sv["W"], sv["dt"], sv["shape"]
            za_key = ("bwd", B, H, Wd, sv["masked"])
            self._za = za = _ZeroArena(self.device, self._za_need.get(za_key, 0), self.ops)
            d = self._HEADS[self.head][3](self, sv, dout, dt, B)
            # ---- decoder (reverse)
            dskips = {}
            for k in reversed(range(len(W["dec"]))):
                (proj, blocks), st_sv, pre = W["dec"][k], sv["dec"][k], W["dec_pre"][k]
                sh, sw_, _ = sv["feat_dims"][2 - k]
                for bw, bsv in zip(reversed(blocks), reversed(st_sv["blocks"])):
                    d = self._block_bwd(d, bw, bsv, B, sh, sw_, dt)
                d, dskips[2 - k] = self._up_bwd(d, proj, st_sv["proj"], B, sh, sw_, dt)
                if pre is not None:
                    d = self._preconv_bwd(d, pre, st_sv["proj"].pre_in, B, sh // 2, sw_ // 2, dt)
            yield from self._segment_end(0)
            if self.encoder_frozen():  # nothing below the decoder needs a gradient: skip ~40 % of the backward
                self._za_need[za_key] = za.used
                yield from self._segment_end(1)
                yield from self._segment_end(2)
                return
            # ---- encoder (reverse); d = gradient w.r.t. feats[3]
            for i in (3, 2, 1, 0):
                (proj, blocks), st_sv = W["enc"][i], sv["enc"][i]
                ch, cw, _ = sv["feat_dims"][i]
                for bw, bsv in zip(reversed(blocks), reversed(st_sv["blocks"])):
                    d = self._block_bwd(d, bw, bsv, B, ch, cw, dt)
                if proj is not None:
                    d = self._down_bwd(d, proj, st_sv["proj"], dskips.get(i - 1), B, ch, cw, dt)
                if i == 2:
                    yield from self._segment_end(1)
            self._stem_bwd(d, sv["stem"], dt)  # stem_1 LayerNorm + stem projection
            self._za_need[za_key] = za.used
            yield from self._segment_end(2)
        finally:
            self.ops.batch_close()

    def _segment_end(self, k: int):
        self.ops.batch_close()
        yield k
        self.ops.batch_open()


def unext2_apply(model, x: Tensor, masks=None, bn_groups: int = 1) -> Tensor:
    return engine_apply(model, x.float(), masks, bn_groups)
