"""TEST INFRASTRUCTURE — ``tests.ref_ops`` plus plain-PyTorch statements of the narrow-channel family (csrc/narrow.hip, the
2x2-stem FCMAE): the same call surface as ``viscy_amd.ops.narrow_*``, written with high-level tensor ops.  Injected into
``Engine`` on CPU to validate the narrow branch of the schedule, and the per-op reference of the GPU tests."""

from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.ref_ops import *  # noqa: F401,F403  (every op of the wide path)
from tests.ref_ops import dwconv7_bwd_data, dwconv7_bwd_weight, dwconv7_fwd, stem_im2col, voxel_shuffle_bwd


def _patches(x, kernel):
    return stem_im2col(x.float(), kernel, torch.float32)


def narrow_stem_fwd(x, W, b, kernel, dtype):
    P = _patches(x, kernel)
    return (P @ W.reshape(W.shape[0], -1).float().t() + b.float()).to(dtype)


def narrow_stem_wgrad(x, df, dW, db, kernel):
    P = _patches(x, kernel)
    dW += (df.float().t() @ P).view_as(dW)
    db += df.float().sum(0)


def _ln_rows(x, eps):
    xf = x.float()
    mean = xf.mean(1)
    rstd = torch.rsqrt(xf.var(1, unbiased=False) + eps)
    return (xf - mean[:, None]) * rstd[:, None], mean, rstd


def narrow_proj_fwd(cat, gamma, beta, W, b, M, Ccat, C, eps=1e-6):
    xh, mean, rstd = _ln_rows(cat.view(M, Ccat), eps)
    xn = xh * gamma + beta
    out = xn @ W.reshape(C, Ccat).float().t() + b
    return out.to(cat.dtype), mean, rstd


def narrow_proj_bwd(dout, cat, mean, rstd, gamma, beta, W, dW, db, M, Ccat, C):
    xn = (cat.float().view(M, Ccat) - mean[:, None]) * rstd[:, None] * gamma + beta
    d = dout.float().view(M, C)
    dW += (d.t() @ xn).view_as(dW)
    db += d.sum(0)
    return (d @ W.reshape(C, Ccat).float()).to(cat.dtype)


def _hidden(y, W1f, b1f, C):
    xh, _, rstd = _ln_rows(y.view(-1, C), 1e-6)
    h = xh @ W1f.float().t() + b1f
    return xh, rstd, h


def narrow_block_fwd1(x, dw_w, dw_b, W1f, b1f, colsq, B, H, W, C):
    y = dwconv7_fwd(x, dw_w, dw_b, B, H, W, C)
    _, _, h = _hidden(y, W1f, b1f, C)
    colsq += (F.gelu(h) ** 2).view(B, H * W, 4 * C).sum(1)
    return y


def narrow_block_fwd2(y, x, W1f, b1f, s, grn_b, W2, b2, B, H, W, C):
    _, _, h = _hidden(y, W1f, b1f, C)
    z = F.gelu(h).view(B, H * W, 4 * C) * s[:, None, :] + grn_b
    out = z.reshape(-1, 4 * C) @ W2.float().t() + b2 + x.float()
    return out.to(x.dtype)


def narrow_block_bwd_a(dout, y, W1f, b1f, s, grn_b, W2, dW2, db2, P, S, B, H, W, C):
    _, _, h = _hidden(y, W1f, b1f, C)
    g = F.gelu(h)
    z = (g.view(B, H * W, 4 * C) * s[:, None, :] + grn_b).reshape(-1, 4 * C)
    d = dout.float()
    dz = d @ W2.float()
    dW2 += (d.t() @ z).view_as(dW2)
    db2 += d.sum(0)
    P += (dz * g).view(B, H * W, 4 * C).sum(1)
    S += dz.view(B, H * W, 4 * C).sum(1)


@torch.enable_grad()
def narrow_block_bwd_b(dout, y, W1f, b1f, s, t, W2, dW1f, db1f, B, H, W, C):
    xh, rstd, h = _hidden(y, W1f, b1f, C)
    hv = h.detach().requires_grad_(True)
    g = F.gelu(hv)
    dz = dout.float() @ W2.float()
    sb = s.repeat_interleave(H * W, 0)
    tb = t.repeat_interleave(H * W, 0)
    (dh,) = torch.autograd.grad(g, hv, dz * sb + g.detach() * tb)
    dW1f += dh.t() @ xh
    db1f += dh.sum(0)
    dxh = dh @ W1f.float()
    dy = rstd[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    return dy.to(y.dtype)


def narrow_block_bwd_c(dy, x, dout, dw_w, ddw, ddb, B, H, W, C):
    dwconv7_bwd_weight(dy, x, ddw, ddb, B, H, W, C)
    return dwconv7_bwd_data(dy, dw_w, dout, B, H, W, C)


def narrow_voxel_shuffle_bwd(dout, B, h, w, Cout, D, s, pool, dtype):
    return voxel_shuffle_bwd(dout, B, h, w, Cout, D, s, pool, dtype)
