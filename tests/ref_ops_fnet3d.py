"""Torch statements of the ops ``viscy_amd.engine_unet3d.Engine`` calls (the ``c3_*`` / ``bn3d_*`` wrappers of viscy_amd.ops), for
running the FNet3D kernel schedule on the CPU (tests/test_fnet3d_cpu.py) and as the GPU op tests' yardstick.  Same signatures and
in-place semantics as the HIP wrappers; a "prepared weight" is the fp32 weight itself together with its role."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def _ncdhw(a: Tensor, coff: int, C: int, grid) -> Tensor:
    B, D, H, W = grid
    return a[:, coff:coff + C].float().reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)


def _cl(x: Tensor) -> Tensor:
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])


def c3_prep(w: Tensor, role: str, dtype: torch.dtype):
    return (w.detach().float(), role)


def c3_conv(a, acoff, cin, wp, bias, out, ccoff, cout, grid, stride=1, transposed=False, accumulate=False, want_stats=False):
    w, role = wp
    x = _ncdhw(a, acoff, cin, grid)
    if role == "conv":
        y = F.conv3d(x, w, None, stride=stride, padding=1)
    elif role == "conv_dgrad_s1":
        y = F.conv_transpose3d(x, w, None, stride=1, padding=1)
    elif role in ("conv_dgrad_s2", "convT"):
        y = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
    elif role == "convT_dgrad":
        y = F.conv3d(x, w, None, stride=2, padding=1)
    else:
        raise ValueError(role)
    if bias is not None:
        y = y + bias.detach().float().view(1, -1, 1, 1, 1)
    y = _cl(y)
    if accumulate:
        y = y + out[:, ccoff:ccoff + cout].float()
    out[:, ccoff:ccoff + cout] = y.to(out.dtype)
    if want_stats:
        z = out[:, ccoff:ccoff + cout].double()
        return torch.stack([z.sum(0), (z * z).sum(0)])[None]
    return None


def c3_wgrad(P, pcoff, R, Q, qcoff, Cq, dW, gridP, stride):
    B, D, H, W = gridP
    gP = _ncdhw(P, pcoff, R, gridP)
    gQ = _ncdhw(Q, qcoff, Cq, (B, D * stride, H * stride, W * stride))
    dW += torch.nn.grad.conv3d_weight(gQ, (R, Cq, 3, 3, 3), gP, stride=stride, padding=1)


def c3_colsum(x, xcoff, C, out):
    out += x[:, xcoff:xcoff + C].float().sum(0)


def bn3d_finalize(stats, M, C, gamma, beta, rmean, rvar, nbt, training, eps=1e-5, momentum=0.1):
    with torch.no_grad():
        if training:
            s = stats.sum(0)
            mean = s[0] / M
            var = (s[1] / M - mean * mean).clamp_min(0)
            rmean.mul_(1 - momentum).add_(momentum * mean.float())
            rvar.mul_(1 - momentum).add_(momentum * (var * M / max(M - 1, 1)).float())
            if nbt is not None:
                nbt += 1
            mean, var = mean.float(), var.float()
        else:
            mean, var = rmean.clone(), rvar.clone()
        rstd = torch.rsqrt(var.double() + eps).float()
        scale = gamma.detach() * rstd
        return torch.stack([scale, beta.detach() - mean * scale, mean, rstd])


def bn3d_apply_relu(z, ss, dst, dcoff):
    C = z.shape[1]
    dst[:, dcoff:dcoff + C] = torch.relu(z.float() * ss[0] + ss[1]).to(dst.dtype)


def bn3d_bwd(dy, ycoff, z, ss, gamma, dgamma, dbeta, training):
    M, C = z.shape
    zf = z.float()
    g = dy[:, ycoff:ycoff + C].float() * ((zf * ss[0] + ss[1]) > 0)
    xh = (zf - ss[2]) * ss[3]
    sg, sgx = g.sum(0), (g * xh).sum(0)
    dgamma += sgx
    dbeta += sg
    if training:
        dz = gamma.detach() * ss[3] * (g - sg / M - xh * sgx / M)
    else:
        dz = gamma.detach() * ss[3] * g
    return dz.to(z.dtype)


def c3_to_cl(x, dtype):
    return _cl(x.float()).to(dtype).contiguous()


def c3_from_cl(y, B, spatial):
    D, H, W = spatial
    return y.float().reshape(B, D, H, W, -1).permute(0, 4, 1, 2, 3).contiguous()
