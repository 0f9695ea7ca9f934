"""Kernel schedule of FNet3D (``viscy_amd.unet3d.Unet3d``): flat fp32 parameter / gradient buffers, forward and backward as
explicit sequences of the ``csrc/conv3d.hip`` kernels, one autograd node for the whole network.

The ops module is injectable (``Engine(model, ops=...)``): ``tests/ref_ops_fnet3d.py`` states every op in torch so that the
schedule itself can be checked on the CPU.

Level l has the grid (D, H, W) / 2^l and c_l = mult_chan * 2^l channels.  Forward, per encoder level: block(e_l) -> cat_l[:, c:2c]
(the skip), e_{l+1} = stride-2 conv(cat_l[:, c:2c]); bottleneck; per decoder level, deepest first: cat_l[:, 0:c] = convT(d_{l+1}),
d_l = block(cat_l); outconv(d_0).  Backward walks the same buffers in reverse: the decoder block's data gradient fills all of
g_cat_l, the transposed convolution reads its columns [0, c), the downsampling convolution's data gradient (the transposed kernel)
is added into its columns [c, 2c) where the encoder block's backward then reads it.
"""

from __future__ import annotations

import torch
from torch import Tensor

from .flat import FlatEngine, engine_apply


class Engine(FlatEngine):
    name = "Unet3d"

    def __init__(self, model, ops=None):
        if ops is None:
            from . import ops
        super().__init__(model, ops)

    # ------------------------------------------------------------------ parameter ordering (backward order)
    @staticmethod
    def _conv_params(c):
        return [c.weight, c.bias]

    def _block_params(self, db):
        ps = []
        for b in (db.block2, db.block1):
            ps += [b.norm.weight, b.norm.bias, b.proj.weight, b.proj.bias]
        return ps

    def _param_order(self):
        m = self.model
        depth = m.num_blocks
        ps = self._conv_params(m.outconv)
        self._bucket_marks = [0]
        for l in range(depth):  # decoder, shallowest first (backward order); _upsamples / _decoder_blocks index i = depth-1-l
            i = depth - 1 - l
            ps += self._block_params(m._decoder_blocks[i][0]) + self._conv_params(m._upsamples[i])
        self._bucket_marks.append(len(ps))  # bucket 0 = outconv + decoder
        ps += self._block_params(m.bottleneck.block)
        for l in reversed(range(1, depth)):
            ps += self._conv_params(m._downsamples[l]) + self._block_params(m._encoder_blocks[l][0])
        self._bucket_marks.append(len(ps))  # bucket 1 = bottleneck + encoder levels depth-1 .. 1
        ps += self._conv_params(m._downsamples[0]) + self._block_params(m._encoder_blocks[0][0]) + self._conv_params(m.inconv)
        self._bucket_marks.append(len(ps))  # bucket 2 = encoder level 0 + inconv
        return ps

    # ------------------------------------------------------------------ building blocks
    def _block_fwd(self, db, inp, icoff, cin, out, ocoff, cout, grid, dt, training, save):
        ops = self.ops
        B, D, H, W = grid
        M = B * D * H * W
        sv = []
        a = inp
        acoff, ac = icoff, cin
        for k, b in enumerate((db.block1, db.block2)):
            wp = ops.c3_prep(b.proj.weight, "conv", dt)
            z = torch.empty((M, cout), dtype=dt, device=self.device)
            stats = ops.c3_conv(a, acoff, ac, wp, b.proj.bias, z, 0, cout, grid, 1, False, False, training)
            bn = b.norm
            ss = ops.bn3d_finalize(stats, M, cout, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                   training, bn.eps, bn.momentum if bn.momentum is not None else 0.1)
            if k == 0:
                dst, dcoff = torch.empty((M, cout), dtype=dt, device=self.device), 0
            else:
                dst, dcoff = out, ocoff
            ops.bn3d_apply_relu(z, ss, dst, dcoff)
            if save:
                sv.append((z, ss, dst if k == 0 else None))
            a, acoff, ac = dst, dcoff, cout
        return sv

    def _block_bwd(self, db, sv, gout, gcoff, inp, icoff, cin, cout, grid, dt, training):
        """returns the gradient of the block input, [M, cin]"""
        ops = self.ops
        (z1, ss1, a1), (z2, ss2, _) = sv
        b1, b2 = db.block1, db.block2
        dz2 = ops.bn3d_bwd(gout, gcoff, z2, ss2, b2.norm.weight, self.g(b2.norm.weight), self.g(b2.norm.bias), training)
        ops.c3_wgrad(dz2, 0, cout, a1, 0, cout, self.g(b2.proj.weight), grid, 1)
        ops.c3_colsum(dz2, 0, cout, self.g(b2.proj.bias))
        ga1 = torch.empty_like(z1)
        ops.c3_conv(dz2, 0, cout, ops.c3_prep(b2.proj.weight, "conv_dgrad_s1", dt), None, ga1, 0, cout, grid)
        del dz2
        dz1 = ops.bn3d_bwd(ga1, 0, z1, ss1, b1.norm.weight, self.g(b1.norm.weight), self.g(b1.norm.bias), training)
        del ga1
        ops.c3_wgrad(dz1, 0, cout, inp, icoff, cin, self.g(b1.proj.weight), grid, 1)
        ops.c3_colsum(dz1, 0, cout, self.g(b1.proj.bias))
        gin = torch.empty((dz1.shape[0], cin), dtype=dt, device=self.device)
        ops.c3_conv(dz1, 0, cout, ops.c3_prep(b1.proj.weight, "conv_dgrad_s1", dt), None, gin, 0, cin, grid)
        return gin

    # ------------------------------------------------------------------ forward / backward
    def forward(self, x: Tensor, dt: torch.dtype, need_bwd: bool):
        ops, m = self.ops, self.model
        training = m.training
        depth, dims = m.num_blocks, m.dims
        B, _, D, H, W = x.shape
        grids = [(B, D >> l, H >> l, W >> l) for l in range(depth + 1)]
        Ms = [g[0] * g[1] * g[2] * g[3] for g in grids]
        h0 = ops.c3_to_cl(x, dt)
        e = torch.empty((Ms[0], dims[0]), dtype=dt, device=self.device)
        ops.c3_conv(h0, 0, m.in_channels, ops.c3_prep(m.inconv.weight, "conv", dt), m.inconv.bias, e, 0, dims[0], grids[0])
        es, cats, enc_sv = [e], [], []
        for l in range(depth):
            c = dims[l]
            cat = torch.empty((Ms[l], 2 * c), dtype=dt, device=self.device)
            enc_sv.append(self._block_fwd(m._encoder_blocks[l][0], es[l], 0, c, cat, c, c, grids[l], dt, training, need_bwd))
            cats.append(cat)
            e = torch.empty((Ms[l + 1], dims[l + 1]), dtype=dt, device=self.device)
            ds = m._downsamples[l]
            ops.c3_conv(cat, c, c, ops.c3_prep(ds.weight, "conv", dt), ds.bias, e, 0, dims[l + 1], grids[l], 2)
            es.append(e)
        d = torch.empty((Ms[depth], dims[depth]), dtype=dt, device=self.device)
        bot_sv = self._block_fwd(m.bottleneck.block, es[depth], 0, dims[depth], d, 0, dims[depth], grids[depth], dt, training,
                                 need_bwd)
        ds_ = [None] * depth + [d]
        dec_sv = [None] * depth
        for i, l in enumerate(reversed(range(depth))):
            c = dims[l]
            up = m._upsamples[i]
            ops.c3_conv(ds_[l + 1], 0, dims[l + 1], ops.c3_prep(up.weight, "convT", dt), up.bias, cats[l], 0, c, grids[l + 1], 2,
                        True)
            d = torch.empty((Ms[l], c), dtype=dt, device=self.device)
            dec_sv[l] = self._block_fwd(m._decoder_blocks[i][0], cats[l], 0, 2 * c, d, 0, c, grids[l], dt, training, need_bwd)
            ds_[l] = d
        yc = torch.empty((Ms[0], m.out_channels), dtype=torch.float32 if dt == torch.bfloat16 else dt, device=self.device)
        ops.c3_conv(ds_[0], 0, dims[0], ops.c3_prep(m.outconv.weight, "conv", dt), m.outconv.bias, yc, 0, m.out_channels, grids[0])
        y = ops.c3_from_cl(yc, B, (D, H, W))
        sv = None
        if need_bwd:
            self._count_forward()
            sv = dict(dt=dt, training=training, grids=grids, h0=h0, es=es, cats=cats, ds=ds_, enc=enc_sv, bot=bot_sv, dec=dec_sv)
        return y, sv

    def backward_stages(self, sv, dout: Tensor):
        ops, m = self.ops, self.model
        dt, training, grids = sv["dt"], sv["training"], sv["grids"]
        depth, dims = m.num_blocks, m.dims
        es, cats, ds_ = sv["es"], sv["cats"], sv["ds"]
        g = ops.c3_to_cl(dout.contiguous().float(), dt)
        co = m.out_channels
        ops.c3_wgrad(g, 0, co, ds_[0], 0, dims[0], self.g(m.outconv.weight), grids[0], 1)
        ops.c3_colsum(g, 0, co, self.g(m.outconv.bias))
        gd = torch.empty((ds_[0].shape[0], dims[0]), dtype=dt, device=self.device)
        ops.c3_conv(g, 0, co, ops.c3_prep(m.outconv.weight, "conv_dgrad_s1", dt), None, gd, 0, dims[0], grids[0])
        del g
        gcats = [None] * depth
        for l in range(depth):
            i = depth - 1 - l
            c = dims[l]
            gcat = self._block_bwd(m._decoder_blocks[i][0], sv["dec"][l], gd, 0, cats[l], 0, 2 * c, c, grids[l], dt, training)
            sv["dec"][l] = None
            up = m._upsamples[i]
            ops.c3_wgrad(ds_[l + 1], 0, dims[l + 1], gcat, 0, c, self.g(up.weight), grids[l + 1], 2)
            ops.c3_colsum(gcat, 0, c, self.g(up.bias))
            gd = torch.empty((ds_[l + 1].shape[0], dims[l + 1]), dtype=dt, device=self.device)
            ops.c3_conv(gcat, 0, c, ops.c3_prep(up.weight, "convT_dgrad", dt), None, gd, 0, dims[l + 1], grids[l], 2)
            gcats[l] = gcat
        yield 0
        ge = self._block_bwd(m.bottleneck.block, sv["bot"], gd, 0, es[depth], 0, dims[depth], dims[depth], grids[depth], dt, training)
        del gd
        for l in reversed(range(depth)):
            c = dims[l]
            dsm = m._downsamples[l]
            ops.c3_wgrad(ge, 0, dims[l + 1], cats[l], c, c, self.g(dsm.weight), grids[l + 1], 2)
            ops.c3_colsum(ge, 0, dims[l + 1], self.g(dsm.bias))
            ops.c3_conv(ge, 0, dims[l + 1], ops.c3_prep(dsm.weight, "conv_dgrad_s2", dt), None, gcats[l], c, c, grids[l + 1], 2,
                        True, True)
            ge = self._block_bwd(m._encoder_blocks[l][0], sv["enc"][l], gcats[l], c, es[l], 0, c, c, grids[l], dt, training)
            sv["enc"][l] = None
            gcats[l] = None
            if l == 1:
                yield 1
        if depth == 1:
            yield 1
        ops.c3_wgrad(ge, 0, dims[0], sv["h0"], 0, m.in_channels, self.g(m.inconv.weight), grids[0], 1)
        ops.c3_colsum(ge, 0, dims[0], self.g(m.inconv.bias))
        yield 2


def unet3d_apply(model, x: Tensor) -> Tensor:
    return engine_apply(model, x.float().contiguous())
