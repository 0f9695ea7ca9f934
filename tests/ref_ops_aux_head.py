"""TEST INFRASTRUCTURE — ``tests.ref_ops`` plus plain-PyTorch statements of the classifier + cross-entropy family
(csrc/aux_head.hip): the same call surface as ``viscy_amd.ops.cls_*``, written with high-level tensor ops in fp32 and in the
rounding order the kernel's header states.  Injected into ``AuxHeadsEngine`` (and the trunk's ``Engine``) on CPU to validate
the head schedule, and the per-op statement of the GPU tests' edge cases."""

from __future__ import annotations

import torch

from tests.ref_ops import *  # noqa: F401,F403  (every op of the trunk and of the hidden layers)

NORM_EPS = 1e-12
IGNORE = -100


def cls_inv_norm(x):
    return 1.0 / x.detach().float().norm(dim=1).clamp_min(NORM_EPS)


def _at_clamp(inv):
    return inv >= (1.0 / torch.tensor(NORM_EPS, dtype=torch.float32))


def cls_logits(h, W, *, inv_h=None, inv_w=None, log_scale=None, bias=None):
    """cosine: fl(fl(fl(dot * inv_h) * inv_w) * exp(log_scale));  linear: fl(dot + bias)"""
    dot = h.detach().float() @ W.detach().float().t()
    if inv_h is not None:
        return ((dot * inv_h[:, None]) * inv_w[None, :]) * torch.exp(log_scale.detach().float()).reshape(())
    return dot + bias.detach() if bias is not None else dot


def cls_ce_fwd(h, W, labels, k, *, inv_h=None, inv_w=None, log_scale=None, bias=None, splits=0):
    Z = cls_logits(h, W, inv_h=inv_h, inv_w=inv_w, log_scale=log_scale, bias=bias)
    B, C = Z.shape
    ok = (labels >= 0) & (labels < C)
    bad = ~ok & (labels != IGNORE)
    ys = labels.clamp(0, C - 1)
    lse = torch.logsumexp(Z, 1)
    zy = Z.gather(1, ys[:, None])[:, 0]
    idx = torch.arange(C)[None]
    ahead = ((Z > zy[:, None]) | ((Z == zy[:, None]) & (idx < ys[:, None]))).sum(1)
    rows = torch.stack([lse, torch.where(ok, zy, torch.zeros(())), torch.where(ok, ahead, torch.tensor(C)).float(),
                        ok.float() - bad.float()], 1)
    n = ok.sum().float()
    loss = torch.where(ok, lse - zy, torch.zeros(())).sum() / n
    if bad.any():
        loss = loss * float("nan")
    acc = torch.stack([loss, (ok & (ahead == 0)).sum() / B, (ok & (ahead < k)).sum() / B, n]).float()
    return rows, acc


def cls_ce_bwd(h, W, labels, rows, acc, gout, dW, *, inv_h=None, inv_w=None, log_scale=None, bias=None, dbias=None,
               dlog_scale=None):
    h, W = h.detach().float(), W.detach().float()
    Z = cls_logits(h, W, inv_h=inv_h, inv_w=inv_w, log_scale=log_scale, bias=bias)
    C = Z.shape[1]
    valid = rows[:, 3] > 0.5
    onehot = torch.nn.functional.one_hot(labels.clamp(0, C - 1), C).float()
    dZ = torch.where(valid[:, None], (torch.exp(Z - rows[:, :1]) - onehot) * (gout.reshape(()) / acc[3]), torch.zeros(()))
    if inv_h is None:
        dW += dZ.t() @ h
        if dbias is not None:
            dbias += dZ.sum(0)
        return dZ @ W
    s = torch.exp(log_scale.detach().float()).reshape(())
    hh, wh = h * inv_h[:, None], W * inv_w[:, None]
    r, q = s * (dZ @ wh), s * (dZ.t() @ hh)
    d, e = (r * hh).sum(1), (q * wh).sum(1)
    dlog_scale += d.sum()
    d = torch.where(_at_clamp(inv_h), torch.zeros(()), d)  # at the 1e-12 clamp the unit vector is x / eps: no projection
    e = torch.where(_at_clamp(inv_w), torch.zeros(()), e)
    dW += inv_w[:, None] * (q - e[:, None] * wh)
    return inv_h[:, None] * (r - d[:, None] * hh)
