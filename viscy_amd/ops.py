"""Tensor-level wrappers over the libvsx C-ABI: PyTorch-ROCm tensors in, tensors out.

PyTorch is used for device memory (caching allocator) and the current stream only; all
arithmetic happens in the HIP kernels.  Every wrapper raises if a tensor is not on the GPU.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from ._lib import VsxGemm, VsxGemmPlan, check, dtype_code, lib, ptr, stream


class Scratch:
    """fp32 scratch of the two-stage reductions: the launches that write one row of partial sums per workgroup — into a workspace
    argument, or into the thread's ``vsx_det_workspace`` — and then fold the rows in a fixed order.

    One rule: a buffer that has been handed to a launch is never released for the life of the process.  The launch holds a raw
    pointer, and a launch captured into a hipGraph replays with the pointer it was recorded with, however much later and whatever
    has been requested in between.

    There is one arena per (thread, device): the library's det workspace is per thread.  ``take`` answers with the arena's newest
    buffer; where that is too small it appends a buffer of at least twice its size, so what an arena retains is at most twice
    its largest buffer (s + s/2 + s/4 + ...).  ``held`` keeps every buffer of every thread, also those of threads that have ended.
    Launches of one thread on different streams share the arena's buffer, as they shared the single workspace before this class:
    the engine issues its reductions on one stream per thread.  No entry point takes both a workspace argument and the det
    workspace, so one arena serves both."""

    def __init__(self, alloc=None):
        self._alloc = alloc or (lambda floats, dev: torch.empty(floats, dtype=torch.float32, device=dev))
        self._tls = threading.local()
        self.held: list = []

    def take(self, dev, floats: int):
        arenas = getattr(self._tls, "arenas", None)
        if arenas is None:
            arenas = self._tls.arenas = {}
        last = arenas.get(dev)
        if last is None or last.numel() < floats:
            last = arenas[dev] = self._alloc(max(int(floats), 2 * last.numel() if last is not None else 0), dev)
            self.held.append(last)
        return last


_SCRATCH = Scratch()


def _workspace(dev, floats: int) -> Tensor:
    """>= ``floats`` fp32 values for the per-workgroup partials of the next launch"""
    return _SCRATCH.take(dev, floats)


def _det(dev, floats) -> None:
    """fixed-order sums active on this thread (``det_reduce`` flag or ``det_scope``): hand the library the scratch for the
    per-workgroup partial sums of the next launch; ``floats()`` is the library's own size query for that launch"""
    if not lib().vsx_det_active():
        return
    n = int(floats())
    if n > 0:
        ws = _workspace(dev, n)
        check(lib().vsx_det_workspace(ptr(ws), ws.numel()), "det_workspace")


@contextlib.contextmanager
def det_scope(on: bool = True):
    """the launches of this thread inside the block form their per-sample sums in a fixed order (vsx_det_scope); nests"""
    if not on:
        yield
        return
    prev = lib().vsx_det_scope(1)
    try:
        yield
    finally:
        lib().vsx_det_scope(prev)


def _fill8(arr, vals: Sequence[int] | None):
    if vals:
        for i, v in enumerate(vals):
            arr[i] = int(v)


def gemm(
    kind: str,
    A: Tensor,
    B: Tensor,
    Cout: Tensor,
    M: int,
    N: int,
    K: int,
    lda: int,
    ldb: int,
    ldc: int,
    *,
    dtype: torch.dtype,
    a_mode: int = L.A_ROWS,
    gh: int = 0,
    gw: int = 0,
    cs: int = 0,
    nz: int = 1,
    a_coff: Sequence[int] | None = None,
    b_off: Sequence[int] | None = None,
    c_coff: Sequence[int] | None = None,
    c_mode: int = L.A_ROWS,
    c_cs: int = 0,
    pro: int = L.PRO_NONE,
    grn_s: Tensor | None = None,
    grn_b: Tensor | None = None,
    hw: int = 0,
    epi: int = L.EPI_NONE,
    bias: Tensor | None = None,
    res: Tensor | None = None,
    ldr: int = 0,
    aux: Tensor | None = None,
    ldx: int = 0,
    red0: Tensor | None = None,
    red1: Tensor | None = None,
    colsum: Tensor | None = None,
    C2: Tensor | None = None,
    b_bstride: int = 0,
    rscale: Tensor | None = None,
    plan: VsxGemmPlan | None = None,
) -> None:
    """kind='nt': C[M,N] = pro(A)[M,K]·B[N,K]^T (+epilogue);  kind='tn': C[N,K](fp32) += B[M,N]^T·pro(A)[M,K].
    With ``plan``: nothing is launched; ``plan`` receives what the call would launch under the current flags (vsx_gemm_plan)."""
    for t in (bias, grn_s, grn_b, red0, red1, colsum):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("bias / GRN / reduction buffers must be float32")
    p = VsxGemm()
    p.A, p.B, p.C = ptr(A), ptr(B), ptr(Cout)
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldb, p.ldc = lda, ldb, ldc
    p.a_mode, p.gh, p.gw, p.cs = a_mode, gh, gw, cs
    p.nz = nz
    _fill8(p.a_coff, a_coff)
    _fill8(p.b_off, b_off)
    _fill8(p.c_coff, c_coff)
    p.c_mode, p.c_cs = c_mode, c_cs
    p.pro = pro
    p.grn_s, p.grn_b = ptr(grn_s), ptr(grn_b)
    p.hw = hw
    p.epi = epi
    p.bias, p.res, p.ldr = ptr(bias), ptr(res), ldr
    p.aux, p.ldx = ptr(aux), ldx
    p.red0, p.red1, p.colsum = ptr(red0), ptr(red1), ptr(colsum)
    p.C2 = ptr(C2)
    p.b_bstride = b_bstride
    p.rscale = ptr(rscale)
    if plan is not None:
        return check(lib().vsx_gemm_plan(L.GEMM_NT if kind == "nt" else L.GEMM_TN, C.byref(p), dtype_code(dtype), C.byref(plan)), f"gemm_plan_{kind}")
    if kind == "nt" and epi == L.EPI_BIAS_GELU_SQ:
        _det(A.device, lambda: _gemm_det_floats(p, dtype))
    fn = lib().vsx_gemm_nt if kind == "nt" else lib().vsx_gemm_tn
    check(fn(C.byref(p), dtype_code(dtype), stream()), f"gemm_{kind}")


def _gemm_det_floats(p: VsxGemm, dtype: torch.dtype) -> int:
    plan = VsxGemmPlan()
    check(lib().vsx_gemm_plan(L.GEMM_NT, C.byref(p), dtype_code(dtype), C.byref(plan)), "gemm_plan_nt")
    return plan.det_floats


def tn_grn_stats_ok(M: int, N: int, K: int, hw: int, dtype: torch.dtype) -> bool:
    """``gemm("tn", g, dout, dW2, ..., pro=PRO_GRN, aux=W2 (bf16 [N, K]), ldx=K, red0=P)`` — the fc2 weight gradient that also
    delivers the GRN backward statistics P[b, k] = sum_hw dz * g from the per-sample tiles in its accumulators (csrc/gemm.hip,
    gemm_tn_fast_kernel PRO == 2) — serves this shape"""
    if dtype != torch.bfloat16 or not lib().vsx_get_flag(b"tn_rect") & 8:
        return False
    p = VsxGemm()   # the statistics launch as the block issues it: pointer fields only say which operands are there
    p.A = p.B = p.C = p.grn_s = p.grn_b = p.aux = p.red0 = 1
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.ldx, p.nz, p.pro, p.hw = M, N, K, K, N, K, K, 1, L.PRO_GRN, hw
    return lib().vsx_gemm_plan(L.GEMM_TN, C.byref(p), L.VSX_BF16, C.byref(VsxGemmPlan())) == 0


def dgrad_ln_bwd(dh: Tensor, WT: Tensor, xh: Tensor, rstd: Tensor, M: int, C: int, K: int,
                 mean: Tensor | None = None) -> Tensor | None:
    """fc1 data gradient with the block LayerNorm's backward in the GEMM epilogue (VSX_EPI_LN_BWD, csrc/gemm_nt2.hip):
    dy = LN_backward(dh . WT^T; xh, rstd) [M, C] in ONE launch — dx^ is never written.  None if the shape is not served
    (the caller then runs the GEMM and vsx_ln_bwd).  With ``mean``: ``xh`` holds the UN-normalised rows y and ``dh`` the
    row-scaled dh * rstd of mlp_bwd_dh_ln."""
    if dh.dtype != torch.bfloat16 or not lib().vsx_gemm_nt_ln_bwd_supported(M, C, K, dtype_code(dh.dtype)):
        return None
    dy = torch.empty((M, C), dtype=dh.dtype, device=dh.device)
    gemm("nt", dh, WT, dy, M, C, K, K, K, C, dtype=dh.dtype, epi=L.EPI_LN_BWD, aux=xh, ldx=C, grn_s=rstd, grn_b=mean)
    return dy


def gemm_z(kind: str, *args, nz: int, a_coff, b_off, c_coff, **kw) -> None:
    """z-batched GEMM with more than 8 slabs: issue in groups of <= 8."""
    for s in range(0, nz, 8):
        e = min(nz, s + 8)
        gemm(kind, *args, nz=e - s, a_coff=a_coff[s:e], b_off=b_off[s:e], c_coff=c_coff[s:e], **kw)


def ln_fwd(x: Tensor, gamma: Tensor | None, beta: Tensor | None, rows: int, Cc: int, eps: float = 1e-6,
           need_mean: bool = True):
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if need_mean else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().vsx_ln_fwd(ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), rows, Cc, eps,
                           dtype_code(x.dtype), stream()), "ln_fwd")
    return y, mean, rstd


def ln_bwd(dy: Tensor, x: Tensor, mean: Tensor | None, rstd: Tensor, gamma: Tensor | None, add: Tensor | None,
           dgamma: Tensor | None, dbeta: Tensor | None, rows: int, Cc: int) -> Tensor:
    dx = torch.empty_like(dy)
    check(lib().vsx_ln_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(add), ptr(dx), ptr(dgamma),
                           ptr(dbeta), rows, Cc, dtype_code(dy.dtype), stream()), "ln_bwd")
    return dx


def grn_scale(colsq: Tensor, gamma: Tensor, eps: float = 1e-6) -> Tensor:
    s = torch.empty_like(colsq)
    check(lib().vsx_grn_scale(ptr(colsq), ptr(gamma), ptr(s), colsq.shape[0], colsq.shape[1], eps, stream()), "grn_scale")
    return s


def grn_bwd_stats(colsq: Tensor, P: Tensor, gamma: Tensor, dgamma: Tensor, eps: float = 1e-6, Sb: Tensor | None = None,
                  dbeta: Tensor | None = None) -> Tensor:
    """Sb [nb, N] = per-sample Σ_hw dz (EPI_DZ red1); dbeta[N] += Σ_b Sb."""
    t = torch.empty_like(colsq)
    rowst = torch.empty_like(colsq)
    if _BATCH is not None:  # the two column reductions into the parameter gradients join the segment's task list
        nb, N = colsq.shape
        check(lib().vsx_grn_bwd_stats(ptr(colsq), ptr(P), None, ptr(gamma), ptr(t), None, None, ptr(rowst), nb, N, eps, stream()),
              "grn_bwd_stats")
        _queue(L.WTASK_REDUCE_ROWS, 0, (nb, N), rowst, dgamma, None, None)
        if Sb is not None:
            _queue(L.WTASK_REDUCE_ROWS, 0, (nb, N), Sb, dbeta, None, None)
        return t
    check(lib().vsx_grn_bwd_stats(ptr(colsq), ptr(P), ptr(Sb), ptr(gamma), ptr(t), ptr(dgamma), ptr(dbeta), ptr(rowst), colsq.shape[0],
                                  colsq.shape[1], eps, stream()), "grn_bwd_stats")
    return t


def grn_gelu_bwd(dz: Tensor, h: Tensor, s: Tensor, t: Tensor, colsum: Tensor, M: int, N: int, hw: int) -> None:
    rows = 2048
    ws = _workspace(dz.device, rows * N)
    check(lib().vsx_grn_gelu_bwd(ptr(dz), ptr(h), ptr(s), ptr(t), ptr(colsum), ptr(ws), rows, M, N, hw,
                                 dtype_code(dz.dtype), stream()), "grn_gelu_bwd")


def dwconv7_fwd(x: Tensor, w: Tensor, bias: Tensor | None, B: int, H: int, W: int, Cc: int) -> Tensor:
    y = torch.empty_like(x)
    check(lib().vsx_dwconv7_fwd(ptr(x), ptr(w), ptr(bias), None, ptr(y), B, H, W, Cc, dtype_code(x.dtype), stream()),
          "dwconv7_fwd")
    return y


def dwconv7_bwd_data(dy: Tensor, w: Tensor, add: Tensor | None, B: int, H: int, W: int, Cc: int) -> Tensor:
    dx = torch.empty_like(dy)
    check(lib().vsx_dwconv7_bwd_data(ptr(dy), ptr(w), ptr(add), ptr(dx), B, H, W, Cc, dtype_code(dy.dtype), stream()),
          "dwconv7_bwd_data")
    return dx


def dwconv7_bwd_weight(dy: Tensor, x: Tensor, dw: Tensor, db: Tensor | None, B: int, H: int, W: int, Cc: int) -> None:
    rows = 256
    ws = _workspace(dy.device, rows * 50 * Cc)
    check(lib().vsx_dwconv7_bwd_weight(ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), rows, B, H, W, Cc, dtype_code(dy.dtype),
                                       stream()), "dwconv7_bwd_weight")


def stem_im2col(x: Tensor, kernel: tuple[int, int, int], dtype: torch.dtype, sub: Tensor | None = None,
                div: Tensor | None = None, ld: int | None = None) -> Tensor:
    """patch matrix of the stem; ``ld`` > patch size pads every row with zeros (see vsx_stem_im2col_ld)"""
    if x.dtype != torch.float32:
        raise TypeError("input stacks are float32")
    B, Cin, Z, H, W = x.shape
    kz, ky, kx = kernel
    K = (Z // kz) * Cin * kz * ky * kx
    ld = K if ld is None else ld
    P = torch.empty((B * (H // ky) * (W // kx), ld), dtype=dtype, device=x.device)
    check(lib().vsx_stem_im2col_ld(ptr(x), ptr(P), ptr(sub), ptr(div), B, Cin, Z, H, W, kz, ky, kx, ld, dtype_code(dtype),
                                   stream()), "stem_im2col")
    return P


def im2col3x3(x: Tensor, B: int, H: int, W: int, Cc: int) -> Tensor:
    """[B*H*W, C] channels-last map -> [B*H*W, 9*C] patch matrix of a 3x3 / padding-1 convolution (tap-major columns)"""
    col = torch.empty((B * H * W, 9 * Cc), dtype=x.dtype, device=x.device)
    check(lib().vsx_im2col3x3(ptr(x), ptr(col), B, H, W, Cc, dtype_code(x.dtype), stream()), "im2col3x3")
    return col


def col2im3x3(dcol: Tensor, B: int, H: int, W: int, Cc: int) -> Tensor:
    """transpose of im2col3x3: [B*H*W, 9*C] -> [B*H*W, C]"""
    dx = torch.empty((B * H * W, Cc), dtype=dcol.dtype, device=dcol.device)
    check(lib().vsx_col2im3x3(ptr(dcol), ptr(dx), B, H, W, Cc, dtype_code(dcol.dtype), stream()), "col2im3x3")
    return dx


def pad_cols(src: Tensor, Kp: int) -> Tensor:
    """[R, K] -> [R, Kp] with zero-filled tail columns"""
    R, K = src.shape
    dst = torch.empty((R, Kp), dtype=src.dtype, device=src.device)
    check(lib().vsx_pad_cols(ptr(src), ptr(dst), R, K, Kp, dtype_code(src.dtype), stream()), "pad_cols")
    return dst


def pixel_shuffle_cat_fwd(low: Tensor, skip: Tensor | None, B: int, h: int, w: int, c: int, cs: int) -> Tensor:
    out = torch.empty((B * 4 * h * w, c + cs), dtype=low.dtype, device=low.device)
    check(lib().vsx_pixel_shuffle_cat_fwd(ptr(low), ptr(skip), ptr(out), B, h, w, c, cs, dtype_code(low.dtype), stream()),
          "pixel_shuffle_cat_fwd")
    return out


def pixel_shuffle_cat_bwd(dcat: Tensor, B: int, h: int, w: int, c: int, cs: int):
    dlow = torch.empty((B * h * w, 4 * c), dtype=dcat.dtype, device=dcat.device)
    dskip = torch.empty((B * 4 * h * w, cs), dtype=dcat.dtype, device=dcat.device) if cs else None
    check(lib().vsx_pixel_shuffle_cat_bwd(ptr(dcat), ptr(dlow), ptr(dskip), B, h, w, c, cs, dtype_code(dcat.dtype),
                                          stream()), "pixel_shuffle_cat_bwd")
    return dlow, dskip


def head_shuffle_fwd(dec: Tensor, B: int, h: int, w: int, C3: int, D: int, pool: bool) -> Tensor:
    hin = torch.empty((B * 4 * h * w, C3 * D), dtype=dec.dtype, device=dec.device)
    check(lib().vsx_head_shuffle_fwd(ptr(dec), ptr(hin), B, h, w, C3, D, int(pool), dtype_code(dec.dtype), stream()),
          "head_shuffle_fwd")
    return hin


def head_shuffle_bwd(dhin: Tensor, B: int, h: int, w: int, C3: int, D: int, pool: bool) -> Tensor:
    ddec = torch.empty((B * h * w, 4 * C3 * D), dtype=dhin.dtype, device=dhin.device)
    check(lib().vsx_head_shuffle_bwd(ptr(dhin), ptr(ddec), B, h, w, C3, D, int(pool), dtype_code(dhin.dtype), stream()),
          "head_shuffle_bwd")
    return ddec


def head_out_fwd(U, ssum, ssq, w2, b2, alpha, B, H2, W2, Z, Cmid, Cout, eps=1e-5) -> Tensor:
    out = torch.empty((B, Cout, Z, 2 * H2, 2 * W2), dtype=torch.float32, device=U.device)
    check(lib().vsx_head_out_fwd(ptr(U), ptr(ssum), ptr(ssq), ptr(w2), ptr(b2), ptr(alpha), ptr(out), B, H2, W2, Z, Cmid,
                                 Cout, eps, dtype_code(U.dtype), stream()), "head_out_fwd")
    return out


def head_out_bwd1(U, ssum, ssq, w2, alpha, dout, S1, S2, dalpha, B, H2, W2, Z, Cmid, Cout, eps=1e-5):
    M5 = B * H2 * W2 * Z
    act = torch.empty((M5, Cmid), dtype=U.dtype, device=U.device)
    dv = torch.empty((M5, 4 * Cout), dtype=U.dtype, device=U.device)
    check(lib().vsx_head_out_bwd1(ptr(U), ptr(ssum), ptr(ssq), ptr(w2), ptr(alpha), ptr(dout), ptr(act), ptr(dv), ptr(S1),
                                  ptr(S2), ptr(dalpha), B, H2, W2, Z, Cmid, Cout, eps, dtype_code(U.dtype), stream()),
          "head_out_bwd1")
    return act, dv


def head_out_bwd1_wgrad(U, ssum, ssq, w2, alpha, dout, S1, S2, dalpha, dW2, db2, B, H2, W2, Z, Cmid, Cout, eps=1e-5) -> Tensor:
    """bf16: pass 1 + the 1x1x1 weight / bias gradient (accumulated into dW2 / db2) in one launch; returns dv."""
    M5 = B * H2 * W2 * Z
    dv = torch.empty((M5, 4 * Cout), dtype=U.dtype, device=U.device)
    scratch = torch.empty((B, 4 * Cout * (Cmid + 1)), dtype=torch.float32, device=U.device)
    check(lib().vsx_head_out_bwd1_wgrad(ptr(U), ptr(ssum), ptr(ssq), ptr(w2), ptr(alpha), ptr(dout), ptr(dv), ptr(S1), ptr(S2),
                                        ptr(dalpha), ptr(dW2), ptr(db2), ptr(scratch), B, H2, W2, Z, Cmid, Cout, eps,
                                        dtype_code(U.dtype), stream()), "head_out_bwd1_wgrad")
    return dv


def head_out_bwd2(U, ssum, ssq, w2, alpha, dv, S1, S2, B, H2, W2, Z, Cmid, Cout, eps=1e-5) -> Tensor:
    dU = torch.empty_like(U)
    check(lib().vsx_head_out_bwd2(ptr(U), ptr(ssum), ptr(ssq), ptr(w2), ptr(alpha), ptr(dv), ptr(S1), ptr(S2), ptr(dU), B,
                                  H2, W2, Z, Cmid, Cout, eps, dtype_code(U.dtype), stream()), "head_out_bwd2")
    return dU


# ------------------------------------------------------------------ weight-space task lists
# prep_weight / transpose_f32 / matvec / mlp_pack are tiny (4 - 7 us, the chip idle behind each one) and the step refreshes
# ~200 of them per weight update.  Inside ``with batch():`` they are not launched but collected and handed to
# vsx_weight_tasks when the block ends (or at flush()): a handful of launches.  Nothing inside a batch may consume the output
# of an op queued in the SAME batch — call flush() first.
_BATCH: list | None = None
_BATCH_ON = os.environ.get("VSX_WBATCH", "1") != "0"  # VSX_WBATCH=0: every job its own launch (A/B measurements)
_BATCH_KEEP: list = []  # the queued jobs' tensors stay alive (and their memory un-recycled) until the list is launched
_BATCH_WRITTEN: list = []  # byte ranges [lo, hi) the queued jobs write / read: a later job that overlaps a written range, or writes
_BATCH_READ: list = []     # into a range an earlier job reads, launches the list collected so far first (see _queue)


@contextlib.contextmanager
def batch():
    global _BATCH
    outer = _BATCH
    if _BATCH_ON:
        _BATCH = [] if outer is None else outer
    try:
        yield
    finally:
        if outer is None:
            flush()
            _BATCH = None


def batch_open() -> None:
    """generator-friendly form of ``batch()`` (a context manager must not be held across a yield): start collecting ..."""
    global _BATCH
    if _BATCH is None and _BATCH_ON:
        _BATCH = []


def batch_close() -> None:
    """... launch what was collected and stop collecting"""
    global _BATCH
    if _BATCH is not None:
        flush()
        _BATCH = None


def flush() -> None:
    """launch what the current batch has collected so far (keeps collecting afterwards)"""
    if not _BATCH:
        return
    arr = (L.VsxWTask * len(_BATCH))(*_BATCH)
    del _BATCH[:]
    try:
        check(lib().vsx_weight_tasks(arr, len(arr), stream()), "weight_tasks")
    finally:  # (a failed launch must not leave stale addresses behind for the next list: ADVICE r4)
        del _BATCH_KEEP[:]
        del _BATCH_WRITTEN[:]
        del _BATCH_READ[:]


def _span(t: Tensor):
    """byte range [lo, hi) a (possibly strided) tensor touches"""
    if t.numel() == 0:
        return (t.data_ptr(), t.data_ptr())
    ext = 1 + sum((n - 1) * abs(st) for n, st in zip(t.shape, t.stride()))
    return (t.data_ptr(), t.data_ptr() + ext * t.element_size())


def _overlaps(a, ranges) -> bool:
    return any(a[0] < hi and lo < a[1] for lo, hi in ranges)


def _queue(kind: int, dtype: int, ints, p0, p1, p2, p3, p4=None, p5=None, p6=None, p7=None) -> bool:
    if _BATCH is None:
        return False
    # The jobs of one list run CONCURRENTLY (one launch): a job must not read, write or accumulate into what another job of the
    # same list writes (UNPREP and the accumulating TRANSPOSE / MATVEC_T / REDUCE_ROWS are non-atomic read-modify-writes).
    # Outputs are p1 (+ p2 for PREP / UNPREP); a job that touches memory an already queued job writes — a tied parameter, two
    # finalisers on one gradient, overlapping views of the flat buffers — or WRITES what an already queued job reads launches the
    # list collected so far first (read-after-write, write-after-write and write-after-read, by byte range).
    outs = [t for t in ((p1, p2) if kind in (L.WTASK_PREP, L.WTASK_UNPREP) else (p1,)) if torch.is_tensor(t)]
    ins = [t for t in (p0, p1, p2, p3, p4, p5, p6, p7) if torch.is_tensor(t) and not any(t is o for o in outs)]
    wr, rd = [_span(t) for t in outs], [_span(t) for t in ins]
    if (_BATCH_WRITTEN and any(_overlaps(a, _BATCH_WRITTEN) for a in wr + rd)) or (_BATCH_READ and any(_overlaps(a, _BATCH_READ) for a in wr)):
        flush()
    _BATCH_WRITTEN.extend(wr)
    _BATCH_READ.extend(rd)
    i = list(ints) + [0] * (4 - len(ints))
    _BATCH.append(L.VsxWTask(kind, dtype, i[0], i[1], i[2], i[3], ptr(p0), ptr(p1), ptr(p2), ptr(p3), ptr(p4), ptr(p5), ptr(p6), ptr(p7)))
    _BATCH_KEEP.append((p0, p1, p2, p3, p4, p5, p6, p7))
    return True


def prep_weight(src: Tensor, R: int, Cs: int, Tn: int, dtype: torch.dtype, *, want: bool = True, want_t: bool = False,
                gamma: Tensor | None = None, tapmode: int = 0):
    K = Cs * Tn
    dst = torch.empty((R, K), dtype=dtype, device=src.device) if want else None
    dstT = torch.empty((K, R), dtype=dtype, device=src.device) if want_t else None
    if (dst is not None or dstT is not None) and _queue(L.WTASK_PREP, dtype_code(dtype), (R, Cs, Tn, tapmode), src, dst, dstT, gamma):
        return dst, dstT
    check(lib().vsx_prep_weight(ptr(src), ptr(dst), ptr(dstT), ptr(gamma), R, Cs, Tn, tapmode, dtype_code(dtype), stream()),
          "prep_weight")
    return dst, dstT


def unprep_grad(g: Tensor, dparam: Tensor, R: int, Cs: int, Tn: int, *, gamma=None, W=None, dgamma=None, u=None,
                beta=None, rowsub=None, tapmode=0):
    """``rowsub`` [R]: subtracted from every column of row r of ``g`` first (the rank-1 term of a weight gradient contracted
    with un-centred rows: mlp_bwd_dh_ln)"""
    if _queue(L.WTASK_UNPREP, 0, (R, Cs, Tn, tapmode), g, dparam, dgamma, gamma, W, u, beta, rowsub):
        return
    check(lib().vsx_unprep_grad(ptr(g), ptr(dparam), ptr(gamma), ptr(W), ptr(dgamma), ptr(u), ptr(beta), ptr(rowsub), R, Cs, Tn,
                                tapmode, stream()), "unprep_grad")


def matvec(W: Tensor, v: Tensor, b: Tensor | None, R: int, Cc: int) -> Tensor:
    out = torch.empty(R, dtype=torch.float32, device=W.device)
    if _queue(L.WTASK_MATVEC, 0, (R, Cc), W, out, b, v):
        return out
    check(lib().vsx_matvec(ptr(W), ptr(v), ptr(b), ptr(out), R, Cc, stream()), "matvec")
    return out


def matvec_t_add(W: Tensor, u: Tensor, out: Tensor, R: int, Cc: int) -> None:
    if _queue(L.WTASK_MATVEC_T, 0, (R, Cc), W, out, None, u):
        return
    check(lib().vsx_matvec_t_add(ptr(W), ptr(u), ptr(out), R, Cc, stream()), "matvec_t_add")


def transpose_f32(src: Tensor, dst: Tensor, A: int, Bn: int, accumulate: bool) -> None:
    if _queue(L.WTASK_TRANSPOSE, 0, (A, Bn, int(accumulate)), src, dst, None, None):
        return
    check(lib().vsx_transpose_f32(ptr(src), ptr(dst), A, Bn, int(accumulate), stream()), "transpose_f32")


def prep_head_dgrad(W: Tensor, Cmid: int, C3: int, Zout: int, dtype: torch.dtype) -> Tensor:
    dst = torch.empty(((Zout + 2) * C3, 27 * Cmid), dtype=dtype, device=W.device)
    check(lib().vsx_prep_head_dgrad(ptr(W), ptr(dst), Cmid, C3, Zout, dtype_code(dtype), stream()), "prep_head_dgrad")
    return dst


def fill_(t: Tensor, value: float = 0.0) -> Tensor:
    """t[...] = value for a contiguous fp32 tensor (vsx_fill_f32: a kernel node of this library, not an ATen fill)"""
    if t.dtype != torch.float32:
        raise TypeError("fill_ is for float32 buffers")
    check(lib().vsx_fill_f32(ptr(t), t.numel(), float(value), stream()), "fill_f32")
    return t


def zeros(*shape, device) -> Tensor:
    """zero-filled fp32 tensor (allocation by the caching allocator, fill by vsx_fill_f32)"""
    return fill_(torch.empty(shape, dtype=torch.float32, device=device), 0.0)


def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor) -> None:
    check(lib().vsx_adamw(ptr(p), ptr(g), ptr(m), ptr(v), ptr(hyper), p.numel(), stream()), "adamw")


# ------------------------------------------------------------------ fused GRN-MLP (csrc/mlp.hip)
def mlp_supported(C: int, hw: int, M: int, dtype: torch.dtype, mode: int | None = None) -> bool:
    """fused GRN-MLP kernel available: the inference pair (mode None), or one pass — 2 training fc1, 3 backward statistics,
    4 backward dh"""
    if dtype != torch.bfloat16:
        return False
    if mode is None:
        return bool(lib().vsx_mlp_supported(C, hw, M, dtype_code(dtype)))
    return bool(lib().vsx_mlp_mode_supported(C, hw, M, mode, dtype_code(dtype)))


def mlp_pack(W1f: Tensor, W2: Tensor, C: int) -> Tensor:
    """fragment-major LDS image of the prepared fc1 / fc2 weights (bf16 [4C, C] and [C, 4C])"""
    img = torch.empty(int(lib().vsx_mlp_image_bytes(C)), dtype=torch.uint8, device=W1f.device)
    if _queue(L.WTASK_MLP_PACK, 0, (C,), W1f, img, None, W2):
        return img
    check(lib().vsx_mlp_pack(ptr(W1f), ptr(W2), ptr(img), C, stream()), "mlp_pack")
    return img


_GTAB: dict = {}


def _gelu_table(dev) -> Tensor:
    """r(a) = a * Phi(-a) for every bf16 magnitude in [2^-24, 16) (computed once per device, in double precision)"""
    t = _GTAB.get(dev)
    if t is None:
        t = torch.empty(int(lib().vsx_mlp_gelu_table_len()), dtype=torch.float32, device=dev)
        check(lib().vsx_mlp_gelu_table(ptr(t), stream()), "mlp_gelu_table")
        _GTAB[dev] = t
    return t


def _mlp_fwd(who: str, mode: int, xh: Tensor, ln_eps: float, img: Tensor, b1: Tensor, *operands, M: int, C: int, hw: int) -> None:
    """vsx_mlp_fwd, or vsx_mlp_fwd_ln where ``ln_eps`` > 0; ``operands`` = (s, beta, b2, res, rscale, out, colsq)"""
    tail = (ptr(img), ptr(b1), *(ptr(t) for t in operands), ptr(_gelu_table(xh.device)), M, C, hw, mode, dtype_code(xh.dtype), stream())
    check(lib().vsx_mlp_fwd_ln(ptr(xh), ln_eps, *tail) if ln_eps > 0.0 else lib().vsx_mlp_fwd(ptr(xh), *tail), who)


def mlp_stats(xh: Tensor, img: Tensor, b1: Tensor, colsq: Tensor, M: int, C: int, hw: int, ln_eps: float = 0.0) -> None:
    """colsq[b, 4C] += per-sample column sums of gelu(fc1(xh))^2 — nothing 4C-wide is written.  ``ln_eps`` > 0: ``xh`` holds the
    UN-normalised rows and the kernel applies the block LayerNorm (no affine) in its prologue"""
    _det(xh.device, lambda: lib().vsx_mlp_det_floats(C, hw, M, 0))
    _mlp_fwd("mlp_stats", 0, xh, ln_eps, img, b1, None, None, None, None, None, None, colsq, M=M, C=C, hw=hw)


def mlp_fc1(xh: Tensor, img: Tensor, b1: Tensor, colsq: Tensor, M: int, C: int, hw: int, store_h: bool = True):
    """training fc1 on the fused kernel: returns (h, g) [M, 4C] and accumulates the GRN statistics into colsq.  ``store_h=False``
    (where ``mlp_supported(.., 6)``): h is None — the backward recomputes it (mlp_bwd_dh_re)"""
    h = torch.empty((M, 4 * C), dtype=xh.dtype, device=xh.device) if store_h else None
    g = torch.empty((M, 4 * C), dtype=xh.dtype, device=xh.device)
    _det(xh.device, lambda: lib().vsx_mlp_det_floats(C, hw, M, 2 if store_h else 6))
    check(lib().vsx_mlp_fc1(ptr(xh), ptr(img), ptr(b1), ptr(colsq), ptr(_gelu_table(xh.device)), ptr(h), ptr(g), M, C, hw,
                            dtype_code(xh.dtype), stream()), "mlp_fc1")
    return h, g


def mlp_fc1_ln(y: Tensor, img: Tensor, b1: Tensor, colsq: Tensor, M: int, C: int, hw: int, eps: float = 1e-6, store_h: bool = True,
               store_xh: bool = True):
    """the block LayerNorm (no affine) + training fc1 in one pass over the depthwise convolution's output ``y``: returns
    (xh, rstd, h, g) — what ln_fwd + mlp_fc1 return, without the LayerNorm pass (``store_h=False``: h is None, see mlp_fc1).
    ``store_xh=False``: the normalised rows are not written either; the first item is then the pair (y, mean) the backward
    re-normalises from (mlp_bwd_dh_ln, dgrad_ln_bwd(mean=...))"""
    xh = torch.empty_like(y) if store_xh else None
    mean = None if store_xh else torch.empty(M, dtype=torch.float32, device=y.device)
    rstd = torch.empty(M, dtype=torch.float32, device=y.device)
    h = torch.empty((M, 4 * C), dtype=y.dtype, device=y.device) if store_h else None
    g = torch.empty((M, 4 * C), dtype=y.dtype, device=y.device)
    _det(y.device, lambda: lib().vsx_mlp_det_floats(C, hw, M, 2 if store_h else 6))
    check(lib().vsx_mlp_fc1_ln(ptr(y), eps, ptr(xh), ptr(rstd), ptr(mean), ptr(img), ptr(b1), ptr(colsq), ptr(_gelu_table(y.device)),
                               ptr(h), ptr(g), M, C, hw, dtype_code(y.dtype), stream()), "mlp_fc1_ln")
    return (xh if store_xh else (y, mean)), rstd, h, g


def grn_q_reduce(Q: Tensor, cs: Tensor, W2: Tensor, s: Tensor, beta: Tensor, P: Tensor, S: Tensor, dW2: Tensor, db2: Tensor) -> None:
    """GRN statistics P, S and the fc2 weight / bias gradient from the per-sample products Q[b] = dout_b^T g_b and the per-sample
    column sums cs[b] of dout (see vsx_grn_q_reduce)"""
    nb, C = cs.shape
    nws = int(lib().vsx_grn_q_reduce_ws_floats(nb, C))
    ws = _workspace(Q.device, nws)
    check(lib().vsx_grn_q_reduce(ptr(Q), ptr(cs), ptr(W2), ptr(s), ptr(beta), ptr(P), ptr(S), ptr(dW2), ptr(db2), ptr(ws), nws,
                                 nb, C, dtype_code(W2.dtype), stream()), "grn_q_reduce")


def mlp_bwd_stats(dout: Tensor, img2: Tensor, g: Tensor, P: Tensor, S: Tensor, M: int, C: int, hw: int) -> None:
    """P[b, 4C] += sum_hw dz * g, S[b, 4C] += sum_hw dz with dz = dout . W2 recomputed on chip (img2 = mlp_pack(W2T, ...))"""
    check(lib().vsx_mlp_bwd_stats(ptr(dout), ptr(img2), ptr(g), ptr(P), ptr(S), M, C, hw, dtype_code(dout.dtype), stream()),
          "mlp_bwd_stats")


def _mlp_dh_alloc(dout: Tensor, M: int, C: int, hw: int, ws_cols: int):
    """what the three dh passes allocate: dh [M, 4C], and the workspace of one row of ``ws_cols`` column sums per workgroup"""
    dh = torch.empty((M, 4 * C), dtype=dout.dtype, device=dout.device)
    rows = M // int(lib().vsx_mlp_rows_per_workgroup(C, hw, M))
    return dh, _workspace(dout.device, rows * ws_cols), rows


def mlp_bwd_dh(dout: Tensor, img2: Tensor, h: Tensor, s: Tensor, t: Tensor, colsum: Tensor, M: int, C: int, hw: int) -> Tensor:
    """dh = (dz * s + gelu(h) * t) * gelu'(h), dz recomputed; colsum[4C] += column sums of dh"""
    dh, ws, rows = _mlp_dh_alloc(dout, M, C, hw, 4 * C)
    check(lib().vsx_mlp_bwd_dh(ptr(dout), ptr(img2), ptr(h), ptr(s), ptr(t), ptr(dh), ptr(ws), rows, ptr(colsum),
                               ptr(_gelu_table(dout.device)), M, C, hw, dtype_code(dout.dtype), stream()), "mlp_bwd_dh")
    return dh


def mlp_bwd_dh_re(dout: Tensor, xh: Tensor, img2: Tensor, img: Tensor, b1: Tensor, s: Tensor, t: Tensor, colsum: Tensor, M: int, C: int,
                  hw: int) -> Tensor:
    """mlp_bwd_dh without a stored pre-activation: h = xh . W1'^T + b1 is recomputed on chip from the normalised rows (img = the
    forward image mlp_pack(W1f, W2), b1 = the folded fc1 bias: bit-identical to what mlp_fc1 would have stored)"""
    dh, ws, rows = _mlp_dh_alloc(dout, M, C, hw, 4 * C)
    check(lib().vsx_mlp_bwd_dh_re(ptr(dout), ptr(xh), ptr(img2), ptr(img), ptr(b1), ptr(s), ptr(t), ptr(dh), ptr(ws), rows, ptr(colsum),
                                  ptr(_gelu_table(dout.device)), M, C, hw, dtype_code(dout.dtype), stream()), "mlp_bwd_dh_re")
    return dh


def mlp_bwd_dh_ln(dout: Tensor, y: Tensor, mean: Tensor, rstd: Tensor, img2: Tensor, img: Tensor, b1: Tensor, s: Tensor, t: Tensor,
                  colsum2: Tensor, M: int, C: int, hw: int) -> Tensor:
    """mlp_bwd_dh_re for a block that stored no normalised rows: x^ is re-formed from the LayerNorm input ``y`` and its row
    statistics; returns dh' = dh * rstd (row-scaled); colsum2 [2, 4C] += {column sums of the UNSCALED dh, u = sum_r dh' * mean}
    (see vsx_mlp_bwd_dh_ln for what the consumers do with them)"""
    dh, ws, rows = _mlp_dh_alloc(dout, M, C, hw, 8 * C)
    check(lib().vsx_mlp_bwd_dh_ln(ptr(dout), ptr(y), ptr(mean), ptr(rstd), ptr(img2), ptr(img), ptr(b1), ptr(s), ptr(t), ptr(dh), ptr(ws),
                                  rows, ptr(colsum2), ptr(_gelu_table(dout.device)), M, C, hw, dtype_code(dout.dtype), stream()),
          "mlp_bwd_dh_ln")
    return dh


def mlp_out(xh: Tensor, img: Tensor, b1: Tensor, s: Tensor, beta: Tensor, b2: Tensor, res: Tensor, rscale: Tensor | None,
            M: int, C: int, hw: int, ln_eps: float = 0.0) -> Tensor:
    """out = res + rscale * (fc2(gelu(fc1(xh)) * s + beta) + b2), hidden activation kept on chip (``ln_eps``: see mlp_stats)"""
    out = torch.empty((M, C), dtype=xh.dtype, device=xh.device)
    _mlp_fwd("mlp_out", 1, xh, ln_eps, img, b1, s, beta, b2, res, rscale, out, None, M=M, C=C, hw=hw)
    return out


def adamw_advance(cfg: Tensor, step: Tensor, hyper: Tensor) -> None:
    """schedule / bias corrections of the next optimiser step from device state (csrc/optim.hip): no host memory involved"""
    if step.dtype != torch.int32 or cfg.dtype != torch.float64:
        raise TypeError("the optimiser step counter is int32, the schedule constants float64")
    check(lib().vsx_adamw_advance(ptr(cfg), ptr(step), ptr(hyper), stream()), "adamw_advance")


# ------------------------------------------------------------------ direct head convolution (csrc/headconv.hip)
def head_conv_supported(H2: int, W2: int, c3: int, cmid: int, zo: int, dtype: torch.dtype) -> bool:
    return bool(lib().vsx_head_conv_supported(H2, W2, c3, cmid, zo, dtype_code(dtype)))


def head_conv_fwd(hin: Tensor, Wc: Tensor, bias: Tensor | None, ssum: Tensor, ssq: Tensor, B: int, H2: int, W2: int, c3: int,
                  cmid: int, zo: int) -> Tensor:
    U = torch.empty((B * H2 * W2, zo * cmid), dtype=hin.dtype, device=hin.device)
    _det(hin.device, lambda: lib().vsx_head_conv_det_floats(B, H2, W2))
    check(lib().vsx_head_conv_fwd(ptr(hin), ptr(Wc), ptr(bias), ptr(U), ptr(ssum), ptr(ssq), B, H2, W2, c3, cmid, zo,
                                  dtype_code(hin.dtype), stream()), "head_conv_fwd")
    return U


def head_conv_wgrad(hin: Tensor, dU: Tensor, dW: Tensor, db: Tensor | None, B: int, H2: int, W2: int, c3: int, cmid: int,
                    zo: int) -> None:
    check(lib().vsx_head_conv_wgrad(ptr(hin), ptr(dU), ptr(dW), ptr(db), B, H2, W2, c3, cmid, zo, dtype_code(hin.dtype),
                                    stream()), "head_conv_wgrad")


def head_conv_dgrad_prep(Wc: Tensor) -> Tensor:
    Wp = torch.empty(45 * 2 * 64 * 8, dtype=Wc.dtype, device=Wc.device)
    check(lib().vsx_head_conv_dgrad_prep(ptr(Wc), ptr(Wp), dtype_code(Wc.dtype), stream()), "head_conv_dgrad_prep")
    return Wp


def head_conv_dgrad(dU: Tensor, Wp: Tensor, B: int, H2: int, W2: int, c3: int, cmid: int, zo: int) -> Tensor:
    dhin = torch.empty((B * H2 * W2, (zo + 2) * c3), dtype=dU.dtype, device=dU.device)
    check(lib().vsx_head_conv_dgrad(ptr(dU), ptr(Wp), ptr(dhin), B, H2, W2, c3, cmid, zo, dtype_code(dU.dtype), stream()),
          "head_conv_dgrad")
    return dhin


def scale_weight_samples(W: Tensor, s: Tensor, dtype: torch.dtype) -> Tensor:
    """out[b] = dtype(W * s[b][None, :]) — the GRN scale folded into the fc2 weights, one matrix per batch sample"""
    R = W.shape[0]
    K = W.numel() // R  # nn.Linear [R, K] or 1x1 nn.Conv2d [R, K, 1, 1] (timm conv_mlp backbones)
    B = s.shape[0]
    out = torch.empty((B, R, K), dtype=dtype, device=W.device)
    check(lib().vsx_scale_weight_samples(ptr(W), ptr(s), ptr(out), B, R, K, dtype_code(dtype), stream()), "scale_weight_samples")
    return out


def layer_scale_fold(W: Tensor, b: Tensor, gamma: Tensor):
    R = W.shape[0]
    K = W.numel() // R
    Ws, bs = torch.empty((R, K), dtype=torch.float32, device=W.device), torch.empty(R, dtype=torch.float32, device=W.device)
    check(lib().vsx_layer_scale_fold(ptr(W), ptr(b), ptr(gamma), ptr(Ws), ptr(bs), R, K, stream()), "layer_scale_fold")
    return Ws, bs


def layer_scale_unfold(dWs: Tensor, dbs: Tensor, W: Tensor, b: Tensor, gamma: Tensor, dW: Tensor, db: Tensor, dgamma: Tensor) -> None:
    R = W.shape[0]
    K = W.numel() // R
    check(lib().vsx_layer_scale_unfold(ptr(dWs), ptr(dbs), ptr(W), ptr(b), ptr(gamma), ptr(dW), ptr(db), ptr(dgamma), R, K, stream()),
          "layer_scale_unfold")


def avgpool_rows_fwd(x: Tensor, B: int, hw: int, C: int) -> Tensor:
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    check(lib().vsx_avgpool_rows_fwd(ptr(x), ptr(out), B, hw, C, dtype_code(x.dtype), stream()), "avgpool_rows_fwd")
    return out


def avgpool_rows_bwd(dout: Tensor, B: int, hw: int, C: int, dtype: torch.dtype) -> Tensor:
    dx = torch.empty((B * hw, C), dtype=dtype, device=dout.device)
    check(lib().vsx_avgpool_rows_bwd(ptr(dout), ptr(dx), B, hw, C, dtype_code(dtype), stream()), "avgpool_rows_bwd")
    return dx


def bn1d_fwd(x: Tensor, w: Tensor, b: Tensor, rmean: Tensor, rvar: Tensor, training: bool, relu: bool, eps: float = 1e-5,
             momentum: float = 0.1):
    B, F = x.shape
    y = torch.empty_like(x)
    sm = torch.empty(F, dtype=torch.float32, device=x.device)
    sr = torch.empty(F, dtype=torch.float32, device=x.device)
    check(lib().vsx_bn1d_fwd(ptr(x), ptr(w), ptr(b), ptr(rmean), ptr(rvar), ptr(y), ptr(sm), ptr(sr), B, F, eps, momentum,
                             int(training), int(relu), stream()), "bn1d_fwd")
    return y, sm, sr


def bn1d_bwd(dy: Tensor, x: Tensor, y: Tensor, w: Tensor, sm: Tensor, sr: Tensor, dw: Tensor, db: Tensor, training: bool,
             relu: bool) -> Tensor:
    B, F = x.shape
    dx = torch.empty_like(x)
    check(lib().vsx_bn1d_bwd(ptr(dy), ptr(x), ptr(y), ptr(w), ptr(sm), ptr(sr), ptr(dx), ptr(dw), ptr(db), B, F, int(training),
                             int(relu), stream()), "bn1d_bwd")
    return dx


def ntxent_fwd(E: Tensor, labels: Tensor, temperature: float, beta: float):
    N, D = E.shape
    dev = E.device
    En, inv = torch.empty_like(E), torch.empty(N, dtype=torch.float32, device=dev)
    S, dS = torch.empty((N, N), dtype=torch.float32, device=dev), torch.empty((N, N), dtype=torch.float32, device=dev)
    rows, acc = torch.empty(2 * N, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
    check(lib().vsx_ntxent_fwd(ptr(E), ptr(labels), ptr(En), ptr(inv), ptr(S), ptr(dS), ptr(rows), ptr(acc), N, D,
                               float(temperature), float(beta), stream()), "ntxent_fwd")
    return acc, (dS, En, inv)


def ntxent_bwd(saved, acc: Tensor, gout: Tensor) -> Tensor:
    dS, En, inv = saved
    N, D = En.shape
    dE = torch.empty_like(En)
    check(lib().vsx_ntxent_bwd(ptr(dS), ptr(En), ptr(inv), ptr(acc), ptr(gout), ptr(dE), N, D, stream()), "ntxent_bwd")
    return dE


TRIPLET_REDUCTIONS = {"mean": 0, "sum": 1}  # the `reduction` argument of vsx_triplet_*


def triplet_fwd(A: Tensor, P: Tensor, N: Tensor, margin: float, eps: float, reduction: str):
    """rows [B, 5] = {d_ap, d_an, hinge, cos_ap, cos_an}, acc [6] = {loss, mean cos_ap, mean d_ap, mean cos_an, mean d_an,
    share of rows with hinge > 0} (include/vsx.h)"""
    B, D = A.shape
    rows = torch.empty((B, 5), dtype=torch.float32, device=A.device)
    acc = torch.empty(6, dtype=torch.float32, device=A.device)
    check(lib().vsx_triplet_fwd(ptr(A), ptr(P), ptr(N), ptr(rows), ptr(acc), B, D, float(margin), float(eps),
                                TRIPLET_REDUCTIONS[reduction], stream()), "triplet_fwd")
    return rows, acc


def triplet_bwd(A: Tensor, P: Tensor, N: Tensor, rows: Tensor, gout: Tensor, margin: float, eps: float, reduction: str):
    B, D = A.shape
    dA, dP, dN = torch.empty_like(A), torch.empty_like(A), torch.empty_like(A)
    check(lib().vsx_triplet_bwd(ptr(A), ptr(P), ptr(N), ptr(rows), ptr(gout), ptr(dA), ptr(dP), ptr(dN), B, D, float(margin),
                                float(eps), TRIPLET_REDUCTIONS[reduction], stream()), "triplet_bwd")
    return dA, dP, dN


def scale_rows_samples(x: Tensor, scale: Tensor, M: int, C: int, hw: int) -> Tensor:
    out = torch.empty_like(x)
    check(lib().vsx_scale_rows_samples(ptr(x), ptr(scale), ptr(out), M, C, hw, dtype_code(x.dtype), stream()), "scale_rows_samples")
    return out


def rows_select(src: Tensor, row_map: Tensor, n_out: int, C: int, add: Tensor | None = None) -> Tensor:
    """dst[r] = map[r] >= 0 ? src[map[r]] (+ add[r]) : 0 — masked_patchify / masked_unpatchify / mask multiply of fcmae.py:95-141."""
    assert row_map.dtype == torch.int32 and row_map.numel() == n_out
    dst = torch.empty((n_out, C), dtype=src.dtype, device=src.device)
    check(lib().vsx_rows_select(ptr(src), ptr(row_map), ptr(add) if add is not None else None, ptr(dst), n_out, C,
                                dtype_code(src.dtype), stream()), "rows_select")
    return dst


def masked_mse_fwd(pred: Tensor, orig: Tensor, mask_u8: Tensor):
    B, C, Z, H, W = pred.shape
    acc = torch.empty(2, dtype=torch.float32, device=pred.device)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    check(lib().vsx_masked_mse_fwd(ptr(pred), ptr(orig), ptr(mask_u8), ptr(acc), ptr(loss), B, C, Z, H * W, stream()), "masked_mse_fwd")
    return loss, acc


def masked_mse_bwd(pred: Tensor, orig: Tensor, mask_u8: Tensor, acc: Tensor, gout: Tensor) -> Tensor:
    B, C, Z, H, W = pred.shape
    dpred = torch.empty_like(pred)
    check(lib().vsx_masked_mse_bwd(ptr(pred), ptr(orig), ptr(mask_u8), ptr(acc), ptr(gout), ptr(dpred), B, C, Z, H * W, stream()),
          "masked_mse_bwd")
    return dpred


# ------------------------------------------------------------------ SpotlightLoss (csrc/spotlight.hip)
SPOTLIGHT_CHUNK = L.SPOTLIGHT_CHUNK  # voxels per workgroup: a row longer than this is summed by several workgroups


def _rows_n(t: Tensor) -> tuple[int, int]:
    rows = t.shape[0] * t.shape[1]
    return rows, t.numel() // rows


def _spotlight_mask(pred: Tensor, target: Tensor, mask: Tensor | None, thr: Tensor | None, rows: int):
    """(mask operand, thresholds, mask mode) of the vsx_spotlight_* calls: a bool mask is read as its bytes, no copy"""
    if target.dtype != torch.float32 or target.shape != pred.shape:
        raise ValueError(f"spotlight: target must be float32 of pred's shape {tuple(pred.shape)}, got {target.dtype} {tuple(target.shape)}")
    if mask is not None:
        if mask.shape != target.shape:
            raise ValueError(f"spotlight: mask shape {tuple(mask.shape)} differs from target's {tuple(target.shape)}")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype == torch.uint8:
            return mask, None, L.SPOTLIGHT_MASK_U8
        if mask.dtype == torch.float32:
            return mask, None, L.SPOTLIGHT_MASK_F32
        raise TypeError(f"spotlight: the mask must be bool, uint8 or float32, got {mask.dtype}")
    if thr is None or thr.dtype != torch.float32 or thr.numel() != rows:  # (B, C) or flat
        raise ValueError(f"spotlight: without a mask, {rows} float32 thresholds (one per row) are required")
    return None, thr, L.SPOTLIGHT_THRESHOLD


def spotlight_workspace_floats(rows: int, n: int, op: int = L.SPOTLIGHT_WS_FWD) -> int:
    """fp32 words of workspace of ``spotlight_fwd`` (or, with ``op=SPOTLIGHT_WS_OTSU``, of ``otsu_threshold``)"""
    return (int(lib().vsx_spotlight_workspace(op, rows, n)) + 3) // 4


def spotlight_fwd(pred: Tensor, target: Tensor, mask: Tensor | None = None, thr: Tensor | None = None, *, lambda_mse: float = 0.5,
                  sigmoid_k: float = -0.95, eps: float = 1e-6, workspace: Tensor | None = None):
    """-> (loss (), coef (rows, 4)).  ``pred`` fp32 or bf16 (B, C, ...), ``target`` fp32; ``mask`` (bool / uint8 / float32, the
    shape of target) or ``thr`` (one float32 threshold per (b, c) row).  ``workspace``: float32, at least
    ``spotlight_workspace_floats`` words, any contents (every word is written before it is read)."""
    rows, n = _rows_n(pred)
    mask, thr, mode = _spotlight_mask(pred, target, mask, thr, rows)
    need = spotlight_workspace_floats(rows, n)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=pred.device)
    elif workspace.dtype != torch.float32 or workspace.numel() < need:
        raise ValueError(f"spotlight_fwd: the workspace must hold {need} float32 words")
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    coef = torch.empty((rows, 4), dtype=torch.float32, device=pred.device)
    check(lib().vsx_spotlight_fwd(ptr(pred), dtype_code(pred.dtype), ptr(target), ptr(mask), mode, ptr(thr), rows, n, lambda_mse,
                                  sigmoid_k, eps, ptr(workspace), ptr(loss), ptr(coef), stream()), "spotlight_fwd")
    return loss, coef


def spotlight_bwd(pred: Tensor, target: Tensor, mask: Tensor | None, thr: Tensor | None, coef: Tensor, gout: Tensor,
                  sigmoid_k: float = -0.95) -> Tensor:
    """d loss / d pred * gout, in pred's dtype; ``gout`` is one float32 on the device"""
    rows, n = _rows_n(pred)
    mask, thr, mode = _spotlight_mask(pred, target, mask, thr, rows)
    dpred = torch.empty_like(pred)
    check(lib().vsx_spotlight_bwd(ptr(pred), dtype_code(pred.dtype), ptr(target), ptr(mask), mode, ptr(thr), ptr(coef), ptr(gout),
                                  ptr(dpred), rows, n, sigmoid_k, stream()), "spotlight_bwd")
    return dpred


def otsu_threshold(target: Tensor, n_bins: int = 256) -> Tensor:
    """Otsu threshold of every (b, c) row of a float32 (B, C, ...) tensor -> (B, C) float32, computed on the device"""
    if target.dtype != torch.float32:
        raise TypeError(f"otsu_threshold: target must be float32, got {target.dtype}")
    rows, n = _rows_n(target)
    ws = torch.empty(spotlight_workspace_floats(rows, n, L.SPOTLIGHT_WS_OTSU), dtype=torch.float32, device=target.device)
    thr = torch.empty((target.shape[0], target.shape[1]), dtype=torch.float32, device=target.device)
    check(lib().vsx_otsu_threshold(ptr(target), ptr(thr), ptr(ws), rows, n, n_bins, stream()), "otsu_threshold")
    return thr


def voxel_shuffle_fwd(feat: Tensor, B: int, h: int, w: int, Cout: int, D: int, s: int, pool: bool) -> Tensor:
    out = torch.empty((B, Cout, D, s * h, s * w), dtype=torch.float32, device=feat.device)
    check(lib().vsx_voxel_shuffle_fwd(ptr(feat), ptr(out), B, h, w, Cout, D, s, int(pool), dtype_code(feat.dtype), stream()),
          "voxel_shuffle_fwd")
    return out


def voxel_shuffle_bwd(dout: Tensor, B: int, h: int, w: int, Cout: int, D: int, s: int, pool: bool, dtype: torch.dtype) -> Tensor:
    dfeat = torch.empty((B * h * w, Cout * D * s * s), dtype=dtype, device=dout.device)
    check(lib().vsx_voxel_shuffle_bwd(ptr(dout), ptr(dfeat), B, h, w, Cout, D, s, int(pool), dtype_code(dtype), stream()),
          "voxel_shuffle_bwd")
    return dfeat


# ------------------------------------------------------------------ test stage (csrc/test_metrics.hip)
def _planes_ws(dev, nbytes: int) -> Tensor:
    """float64 per-workgroup partials of a test-stage launch, sized by the library, from the reduction scratch"""
    if nbytes <= 0:
        raise ValueError(f"test-stage workspace query answered {nbytes}: the shape is refused")
    return _workspace(dev, (int(nbytes) + 3) // 4)


def pair_sums(P: Tensor, p_strides: tuple[int, int], T: Tensor, t_strides: tuple[int, int], planes: int, H: int, W: int) -> Tensor:
    """vsx_pair_sums on two runs of ``planes`` fp32 images starting at the tensors' first elements, (plane, row) strides in
    elements -> [VSX_PAIR_SUMS] float64.  The tensors may be views: only their first address is taken."""
    if not (P.is_cuda and T.is_cuda and P.dtype == T.dtype == torch.float32):
        raise RuntimeError("viscy_amd.pair_sums takes float32 tensors on the HIP device (no CPU fallback)")
    out = torch.empty(L.PAIR_SUMS, dtype=torch.float64, device=P.device)
    ws = _planes_ws(P.device, lib().vsx_pair_sums_ws_bytes(planes, H))
    check(lib().vsx_pair_sums(P.data_ptr(), p_strides[0], p_strides[1], T.data_ptr(), t_strides[0], t_strides[1], planes, H, W, ptr(out),
                              ptr(ws), ws.numel() * 4, stream()), "pair_sums")
    return out


def ssim_window(P: Tensor, p_strides: tuple[int, int], T: Tensor, t_strides: tuple[int, int], planes: int, H: int, W: int, wy: Tensor,
                wx: Tensor, c: Tensor, shift: Tensor, full: bool = False) -> tuple[Tensor, Tensor | None]:
    """vsx_ssim_window -> (sums [planes] float64, the map [planes, H - Ky + 1, W - Kx + 1] fp32 or None); wy / wx / c / shift are
    fp32 device tensors (taps, {c1, c2}, {s_p, s_t})"""
    if not (P.is_cuda and T.is_cuda and P.dtype == T.dtype == torch.float32):
        raise RuntimeError("viscy_amd.ssim_window takes float32 tensors on the HIP device (no CPU fallback)")
    ky, kx = int(wy.numel()), int(wx.numel())
    sums = torch.empty(planes, dtype=torch.float64, device=P.device)
    fmap = torch.empty((planes, H - ky + 1, W - kx + 1), dtype=torch.float32, device=P.device) if full else None
    ws = _planes_ws(P.device, lib().vsx_ssim_window_ws_bytes(planes, H, W, ky, kx))
    check(lib().vsx_ssim_window(P.data_ptr(), p_strides[0], p_strides[1], T.data_ptr(), t_strides[0], t_strides[1], planes, H, W, ptr(wy), ky,
                                ptr(wx), kx, ptr(c), ptr(shift), ptr(sums), ptr(fmap), ptr(ws), ws.numel() * 4, stream()), "ssim_window")
    return sums, fmap


# ------------------------------------------------------------------ narrow-channel family (csrc/narrow.hip): the 2x2-stem FCMAE
def _narrow_ws(dev, op: int, B: int, n: int, C: int, K: int = 0) -> Tensor:
    """per-workgroup partials of a narrow launch, sized by the library"""
    floats = int(lib().vsx_narrow_ws_floats(op, B, n, C, K))
    if floats <= 0:
        raise ValueError(f"vsx_narrow_ws_floats({op}, {B}, {n}, {C}, {K}) = {floats}")
    return _workspace(dev, floats)


def narrow_stem_fwd(x: Tensor, W: Tensor, b: Tensor, kernel: tuple[int, int, int], dtype: torch.dtype) -> Tensor:
    """stem whose patch (K = Cin*kz*ky*kx) is not a whole number of 16-byte bf16 vectors: [B*h*w, C0] straight from the fp32 stack"""
    if x.dtype != torch.float32:
        raise TypeError("input stacks are float32")
    B, Cin, Z, H, Wd = x.shape
    kz, ky, kx = kernel
    C0 = W.shape[0]
    out = torch.empty((B * (H // ky) * (Wd // kx), C0), dtype=dtype, device=x.device)
    check(lib().vsx_narrow_stem_fwd(ptr(x), ptr(W), ptr(b), ptr(out), B, Cin, Z, H, Wd, kz, ky, kx, C0, dtype_code(dtype), stream()),
          "narrow_stem_fwd")
    return out


def narrow_stem_wgrad(x: Tensor, df: Tensor, dW: Tensor, db: Tensor, kernel: tuple[int, int, int]) -> None:
    B, Cin, Z, H, Wd = x.shape
    kz, ky, kx = kernel
    C0, K = df.shape[1], Cin * kz * ky * kx
    ws = _narrow_ws(x.device, L.NARROW_STEM, B, df.shape[0], C0, K)
    check(lib().vsx_narrow_stem_wgrad(ptr(x), ptr(df), ptr(dW), ptr(db), ptr(ws), ws.numel(), B, Cin, Z, H, Wd, kz, ky, kx, C0,
                                      dtype_code(df.dtype), stream()), "narrow_stem_wgrad")


def narrow_proj_fwd(cat: Tensor, gamma: Tensor, beta: Tensor, W: Tensor, b: Tensor, M: int, Ccat: int, C: int, eps: float = 1e-6):
    """LayerNorm2d(Ccat, affine) + 1x1 convolution into C in {4, 8} channels; returns (out [M, C], mean [M], rstd [M])"""
    out = torch.empty((M, C), dtype=cat.dtype, device=cat.device)
    mean = torch.empty(M, dtype=torch.float32, device=cat.device)
    rstd = torch.empty(M, dtype=torch.float32, device=cat.device)
    check(lib().vsx_narrow_proj_fwd(ptr(cat), ptr(gamma), ptr(beta), ptr(W), ptr(b), ptr(out), ptr(mean), ptr(rstd), M, Ccat, C, eps,
                                    dtype_code(cat.dtype), stream()), "narrow_proj_fwd")
    return out, mean, rstd


def narrow_proj_bwd(dout: Tensor, cat: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, beta: Tensor, W: Tensor, dW: Tensor,
                    db: Tensor, M: int, Ccat: int, C: int) -> Tensor:
    """returns dxn [M, Ccat] (gradient of the LayerNorm's affine output); dW [C, Ccat] / db [C] accumulate"""
    dxn = torch.empty((M, Ccat), dtype=cat.dtype, device=cat.device)
    ws = _narrow_ws(cat.device, L.NARROW_PROJ, 1, M, C, Ccat)
    check(lib().vsx_narrow_proj_bwd(ptr(dout), ptr(cat), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(W), ptr(dxn), ptr(dW), ptr(db),
                                    ptr(ws), ws.numel(), M, Ccat, C, dtype_code(cat.dtype), stream()), "narrow_proj_bwd")
    return dxn


def narrow_block_fwd1(x: Tensor, dw_w: Tensor, dw_b: Tensor, W1f: Tensor, b1f: Tensor, colsq: Tensor, B: int, H: int, W: int,
                      C: int) -> Tensor:
    """ConvNeXt-V2 block at C in {4, 8}, pass 1: returns the depthwise output y; colsq [B, 4C] += per-sample sum gelu(h)^2"""
    y = torch.empty_like(x)
    ws = _narrow_ws(x.device, L.NARROW_FWD1, B, H * W, C)
    check(lib().vsx_narrow_block_fwd1(ptr(x), ptr(dw_w), ptr(dw_b), ptr(W1f), ptr(b1f), ptr(y), ptr(colsq), ptr(ws), ws.numel(), B, H, W,
                                      C, dtype_code(x.dtype), stream()), "narrow_block_fwd1")
    return y


def narrow_block_fwd2(y: Tensor, x: Tensor, W1f: Tensor, b1f: Tensor, s: Tensor, grn_b: Tensor, W2: Tensor, b2: Tensor, B: int, H: int,
                      W: int, C: int) -> Tensor:
    out = torch.empty_like(x)
    check(lib().vsx_narrow_block_fwd2(ptr(y), ptr(x), ptr(W1f), ptr(b1f), ptr(s), ptr(grn_b), ptr(W2), ptr(b2), ptr(out), B, H, W, C,
                                      dtype_code(x.dtype), stream()), "narrow_block_fwd2")
    return out


def narrow_block_bwd_a(dout: Tensor, y: Tensor, W1f: Tensor, b1f: Tensor, s: Tensor, grn_b: Tensor, W2: Tensor, dW2: Tensor, db2: Tensor,
                       P: Tensor, S: Tensor, B: int, H: int, W: int, C: int) -> None:
    ws = _narrow_ws(y.device, L.NARROW_BWD_A, B, H * W, C)
    check(lib().vsx_narrow_block_bwd_a(ptr(dout), ptr(y), ptr(W1f), ptr(b1f), ptr(s), ptr(grn_b), ptr(W2), ptr(dW2), ptr(db2), ptr(P),
                                       ptr(S), ptr(ws), ws.numel(), B, H, W, C, dtype_code(y.dtype), stream()), "narrow_block_bwd_a")


def narrow_block_bwd_b(dout: Tensor, y: Tensor, W1f: Tensor, b1f: Tensor, s: Tensor, t: Tensor, W2: Tensor, dW1f: Tensor, db1f: Tensor,
                       B: int, H: int, W: int, C: int) -> Tensor:
    dy = torch.empty_like(y)
    ws = _narrow_ws(y.device, L.NARROW_BWD_B, B, H * W, C)
    check(lib().vsx_narrow_block_bwd_b(ptr(dout), ptr(y), ptr(W1f), ptr(b1f), ptr(s), ptr(t), ptr(W2), ptr(dy), ptr(dW1f), ptr(db1f),
                                       ptr(ws), ws.numel(), B, H, W, C, dtype_code(y.dtype), stream()), "narrow_block_bwd_b")
    return dy


def narrow_block_bwd_c(dy: Tensor, x: Tensor, dout: Tensor, dw_w: Tensor, ddw: Tensor, ddb: Tensor, B: int, H: int, W: int,
                       C: int) -> Tensor:
    dx = torch.empty_like(x)
    ws = _narrow_ws(x.device, L.NARROW_BWD_C, B, H * W, C)
    check(lib().vsx_narrow_block_bwd_c(ptr(dy), ptr(x), ptr(dout), ptr(dw_w), ptr(dx), ptr(ddw), ptr(ddb), ptr(ws), ws.numel(), B, H, W,
                                       C, dtype_code(x.dtype), stream()), "narrow_block_bwd_c")
    return dx


def narrow_voxel_shuffle_bwd(dout: Tensor, B: int, h: int, w: int, Cout: int, D: int, s: int, pool: bool, dtype: torch.dtype) -> Tensor:
    dfeat = torch.empty((B * h * w, Cout * D * s * s), dtype=dtype, device=dout.device)
    check(lib().vsx_narrow_voxel_shuffle_bwd(ptr(dout), ptr(dfeat), B, h, w, Cout, D, s, int(pool), dtype_code(dtype), stream()),
          "narrow_voxel_shuffle_bwd")
    return dfeat


# ------------------------------------------------------------------------------------------------
# dense 3x3x3 convolution family (csrc/conv3d.hip): FNet3D.  Activations are channels-last [M, ld] matrices; an operand is the
# column slice [coff, coff + C) of one.  ``grid`` = (B, D, H, W) of the convolution's INPUT.
# roles of a prepared weight (the GEMM operand [N][27 K] read by vsx_conv3d_fwd):
#   conv          Conv3d weight [Cout, Cin, 3, 3, 3]            -> forward (stride 1 / 2)
#   conv_dgrad_s1 Conv3d weight, flipped + channel-transposed   -> data gradient of a stride-1 convolution
#   conv_dgrad_s2 Conv3d weight, channel-transposed             -> data gradient of the stride-2 convolution (transposed kernel)
#   convT         ConvTranspose3d weight [Cin, Cout, 3, 3, 3]   -> forward (8 parity classes)
#   convT_dgrad   ConvTranspose3d weight                        -> its data gradient (stride-2 convolution)
_C3_ROLES = {  # role -> (N, Kc, sn, sc, flip) from the weight's dims (d0, d1)
    "conv": lambda d0, d1: (d0, d1, d1 * 27, 27, 0),
    "conv_dgrad_s1": lambda d0, d1: (d1, d0, 27, d1 * 27, 1),
    "conv_dgrad_s2": lambda d0, d1: (d1, d0, 27, d1 * 27, 0),
    "convT": lambda d0, d1: (d1, d0, 27, d1 * 27, 0),
    "convT_dgrad": lambda d0, d1: (d0, d1, d1 * 27, 27, 0),
}


def c3_prep(w: Tensor, role: str, dtype: torch.dtype) -> Tensor:
    """prepared GEMM operand [N, 27 * K] of a 3x3x3 weight (fp32 master view) for ``role``"""
    d0, d1 = w.shape[0], w.shape[1]
    N, Kc, sn, sc, flip = _C3_ROLES[role](d0, d1)
    out = torch.empty((N, 27 * Kc), dtype=dtype, device=w.device)
    check(lib().vsx_conv3d_prep_weight(ptr(w), ptr(out), N, Kc, sn, sc, flip, dtype_code(dtype), stream()), "conv3d_prep_weight")
    return out


def c3_conv(a: Tensor, acoff: int, cin: int, wp: Tensor, bias: Tensor | None, out: Tensor, ccoff: int, cout: int,
            grid: Sequence[int], stride: int = 1, transposed: bool = False, accumulate: bool = False,
            want_stats: bool = False) -> Tensor | None:
    """out[:, ccoff:ccoff+cout] (+)= conv(a[:, acoff:acoff+cin]) + bias; returns the BatchNorm statistics partials if asked"""
    B, D, H, W = grid
    if a.dtype != wp.dtype:
        raise TypeError("conv3d: activation and prepared weight dtypes differ")
    Mo = B * D * H * W * 8 if transposed else B * (D // stride) * (H // stride) * (W // stride)
    if a.ndim != 2 or out.ndim != 2 or a.shape[0] != B * D * H * W or out.shape[0] != Mo or acoff + cin > a.shape[1] \
            or ccoff + cout > out.shape[1] or tuple(wp.shape) != (cout, 27 * cin):
        raise ValueError(f"conv3d: operand shapes {tuple(a.shape)} / {tuple(wp.shape)} / {tuple(out.shape)} do not fit grid {tuple(grid)}")
    stats = None
    if want_stats:
        rows = lib().vsx_conv3d_stats_rows(B, D, H, W, stride, int(transposed))
        stats = torch.empty((rows, 2, cout), dtype=torch.float32, device=a.device)
    out_f32 = int(out.dtype == torch.float32 and a.dtype == torch.bfloat16)
    if not out_f32 and out.dtype != a.dtype:
        raise TypeError("conv3d: output dtype must be the operand dtype or float32")
    check(lib().vsx_conv3d_fwd(ptr(a), a.shape[1], acoff, ptr(wp), ptr(bias), ptr(out), out.shape[1], ccoff, ptr(stats), B, D, H, W,
                               cin, cout, stride, int(transposed), int(accumulate), dtype_code(a.dtype), out_f32, stream()),
          "conv3d_fwd")
    return stats


def c3_wgrad(P: Tensor, pcoff: int, R: int, Q: Tensor, qcoff: int, Cq: int, dW: Tensor, gridP: Sequence[int], stride: int) -> None:
    """dW[r, c, kz, ky, kx] += sum over the voxels m of P's grid of P[m, r] * Q[m * stride + k - 1, c]  (zero outside Q's grid)"""
    B, D, H, W = gridP
    if P.dtype != Q.dtype or P.shape[0] != B * D * H * W or Q.shape[0] != P.shape[0] * stride ** 3 or pcoff + R > P.shape[1] \
            or qcoff + Cq > Q.shape[1] or dW.numel() != R * Cq * 27 or dW.dtype != torch.float32:
        raise ValueError("conv3d_wgrad: operand shapes do not fit")
    dt = dtype_code(P.dtype)
    n = lib().vsx_conv3d_wgrad_ws_floats(B, D, H, W, R, Cq, dt)
    ws = torch.empty(n, dtype=torch.float32, device=P.device)
    check(lib().vsx_conv3d_wgrad(ptr(P), P.shape[1], pcoff, ptr(Q), Q.shape[1], qcoff, ptr(ws), n, ptr(dW), B, D, H, W, R, Cq, stride,
                                 dt, stream()), "conv3d_wgrad")


def c3_colsum(x: Tensor, xcoff: int, C: int, out: Tensor) -> None:
    """out += column sums of x[:, xcoff:xcoff+C] (bias gradients)"""
    M = x.shape[0]
    ws = torch.empty(lib().vsx_conv3d_colsum_groups(M) * C, dtype=torch.float32, device=x.device)
    check(lib().vsx_conv3d_colsum(ptr(x), x.shape[1], xcoff, M, C, ptr(ws), ptr(out), dtype_code(x.dtype), stream()), "conv3d_colsum")


def bn3d_finalize(stats: Tensor | None, M: int, C: int, gamma: Tensor, beta: Tensor, rmean: Tensor, rvar: Tensor, nbt: Tensor | None,
                  training: bool, eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """[4, C] = scale | shift | mean | rstd of the BatchNorm (batch statistics + running-stat update, or running statistics)"""
    ss = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    G = stats.shape[0] if stats is not None else 0
    check(lib().vsx_bn3d_finalize(ptr(stats) if training else None, G, M, C, ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
                                  ptr(nbt) if training else None, ptr(ss), float(eps), float(momentum), int(training), stream()),
          "bn3d_finalize")
    return ss


def bn3d_apply_relu(z: Tensor, ss: Tensor, dst: Tensor, dcoff: int) -> None:
    M, C = z.shape
    if dst.shape[0] != M or dcoff + C > dst.shape[1] or ss.numel() != 4 * C:
        raise ValueError("bn3d_apply_relu: destination does not fit")
    check(lib().vsx_bn3d_apply_relu(ptr(z), ptr(ss), ptr(dst), dst.shape[1], dcoff, M, C, dtype_code(z.dtype), stream()),
          "bn3d_apply_relu")


def bn3d_bwd(dy: Tensor, ycoff: int, z: Tensor, ss: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor, training: bool) -> Tensor:
    """dz of relu(batch_norm(z)) for the upstream gradient dy[:, ycoff:ycoff+C]; dgamma / dbeta accumulate"""
    M, C = z.shape
    if dy.shape[0] != M or ycoff + C > dy.shape[1] or ss.numel() != 4 * C:
        raise ValueError("bn3d_bwd: gradient does not fit")
    ws = torch.empty(lib().vsx_bn3d_bwd_ws_floats(M, C), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    check(lib().vsx_bn3d_bwd(ptr(dy), dy.shape[1], ycoff, ptr(z), ptr(ss), ptr(gamma), ptr(ws), ptr(dgamma), ptr(dbeta), ptr(dz), M, C,
                             int(training), dtype_code(z.dtype), stream()), "bn3d_bwd")
    return dz


def c3_to_cl(x: Tensor, dtype: torch.dtype) -> Tensor:
    """NCDHW float32 -> channels-last [B*D*H*W, C] in ``dtype``"""
    if x.dtype != torch.float32:
        raise TypeError("conv3d_to_cl reads float32")
    B, C = x.shape[:2]
    S = x[0, 0].numel()
    out = torch.empty((B * S, C), dtype=dtype, device=x.device)
    check(lib().vsx_conv3d_to_cl(ptr(x), ptr(out), B, C, S, dtype_code(dtype), stream()), "conv3d_to_cl")
    return out


def c3_from_cl(y: Tensor, B: int, spatial: Sequence[int]) -> Tensor:
    """channels-last [B*D*H*W, C] -> NCDHW float32"""
    C = y.shape[1]
    out = torch.empty((B, C, *spatial), dtype=torch.float32, device=y.device)
    S = out[0, 0].numel()
    check(lib().vsx_conv3d_from_cl(ptr(y), ptr(out), B, C, S, dtype_code(y.dtype), stream()), "conv3d_from_cl")
    return out


# ------------------------------------------------------------------ OnlineEvalCallback (csrc/online_eval.hip)
KNN_MAX_K = L.KNN_MAX_K


def _rows_f32(x: Tensor, what: str) -> tuple[int, int]:
    ptr(x)  # raises for a CPU or non-contiguous tensor
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError(f"{what}: features must be a float32 (N, d) tensor, got {x.dtype} {tuple(x.shape)}")
    return x.shape[0], x.shape[1]


def _i32(t: Tensor, n: int, what: str) -> Tensor:
    ptr(t)
    if t.dtype != torch.int32 or t.numel() != n:
        raise TypeError(f"{what} must be {n} int32 values, got {t.dtype} {tuple(t.shape)}")
    return t


def _f32_vec(t: Tensor, n: int, what: str) -> None:
    ptr(t)
    if t.dtype != torch.float32 or t.numel() != n:
        raise TypeError(f"{what} must be {n} float32 values")


def _ws(dev, nbytes: int, dtype: torch.dtype, min_elems: int = 1) -> Tensor:
    """a workspace of ``dtype`` that holds ``nbytes`` bytes and at least ``min_elems`` elements; ``ws.nbytes`` is its size"""
    return torch.empty(max(-(-int(nbytes) // dtype.itemsize), min_elems), dtype=dtype, device=dev)


def row_inv_norm(x: Tensor, eps: float = 0.0) -> Tensor:
    """inv[i] = 1 / (||x_i||_2 + eps); 0 where that denominator is 0 (an all-zero row with eps = 0, as sklearn's ``normalize``)"""
    n, d = _rows_f32(x, "row_inv_norm")
    inv = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib().vsx_row_inv_norm(ptr(x), ptr(inv), n, d, eps, stream()), "row_inv_norm")
    return inv


def knn_topk(x: Tensor, inv: Tensor, group: Tensor, k: int):
    """-> (idx (N, k) int32, sim (N, k) float32, cnt (N,) int32): for every row its min(k, #candidates) most similar rows of the
    OTHER groups (``group[j] >= 0 and group[j] != group[i]``), s = fl32(fl32(dot * inv_i) * inv_j), in the total order
    (s descending, j ascending); unused slots idx = -1, sim = -inf.  No N x N buffer: the workspace is O(N k)."""
    n, d = _rows_f32(x, "knn_topk")
    _f32_vec(inv, n, "knn_topk: inv")
    _i32(group, n, "knn_topk: group")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:  # the library refuses it too; here before anything is allocated
        raise ValueError(f"knn_topk: k={k} must be in [1, {KNN_MAX_K}]")
    ws = _ws(x.device, lib().vsx_knn_topk_ws_bytes(n, d, k), torch.int32, 0)
    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
    sim = torch.empty((n, k), dtype=torch.float32, device=x.device)
    cnt = torch.empty(n, dtype=torch.int32, device=x.device)
    check(lib().vsx_knn_topk(ptr(x), ptr(inv), ptr(group), n, d, k, ptr(idx), ptr(sim), ptr(cnt), ptr(ws), ws.nbytes, stream()), "knn_topk")
    return idx, sim, cnt


def knn_vote(idx: Tensor, cnt: Tensor, labels: Tensor) -> Tensor:
    """pred[i] = the most frequent of labels[idx[i, :cnt[i]]], ties to the smallest label; -1 where cnt[i] = 0"""
    ptr(idx)
    if idx.dtype != torch.int32 or idx.dim() != 2:
        raise TypeError("knn_vote: idx must be an int32 (N, k) tensor")
    n, k = idx.shape
    _i32(cnt, n, "knn_vote: cnt")
    _i32(labels, labels.numel(), "knn_vote: labels")
    pred = torch.empty(n, dtype=torch.int32, device=idx.device)
    check(lib().vsx_knn_vote(ptr(idx), ptr(cnt), ptr(labels), n, k, ptr(pred), stream()), "knn_vote")
    return pred


def pair_cosine_dist(x: Tensor, inv: Tensor, pi: Tensor, pj: Tensor) -> Tensor:
    """out[p] = 1 - fl32(fl32(dot(x[pi[p]], x[pj[p]]) * inv[pi[p]]) * inv[pj[p]])"""
    n, d = _rows_f32(x, "pair_cosine_dist")
    _f32_vec(inv, n, "pair_cosine_dist: inv")
    p = pi.numel()
    _i32(pi, p, "pair_cosine_dist: pi")
    _i32(pj, p, "pair_cosine_dist: pj")
    out = torch.empty(p, dtype=torch.float32, device=x.device)
    if p:
        check(lib().vsx_pair_cosine_dist(ptr(x), ptr(inv), ptr(pi), ptr(pj), p, d, ptr(out), stream()), "pair_cosine_dist")
    return out


# ------------------------------------------------------------------ ClassificationHead: classifier + cross-entropy (csrc/aux_head.hip)
def _cls_operands(h: Tensor, W: Tensor, inv_h, inv_w, log_scale, bias):
    for t in (h, W):
        ptr(t)
        if t.dtype != torch.float32 or t.dim() != 2:
            raise TypeError(f"cls: h and W must be float32 matrices, got {t.dtype} {tuple(t.shape)}")
    if W.shape[1] != h.shape[1]:
        raise ValueError(f"cls: h {tuple(h.shape)} and W {tuple(W.shape)} differ in width")
    for t in (inv_h, inv_w, log_scale, bias):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("cls: inv_h / inv_w / log_scale / bias must be float32")
    return h.shape[0], h.shape[1], W.shape[0]


def cls_inv_norm(x: Tensor) -> Tensor:
    """inv[i] = 1 / max(||x_i||_2, 1e-12): ``F.normalize``'s rule (a zero row gets 1e12 and a zero unit vector)"""
    n, d = _rows_f32(x, "cls_inv_norm")
    inv = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib().vsx_cls_inv_norm(ptr(x), ptr(inv), n, d, stream()), "cls_inv_norm")
    return inv


def cls_ce_fwd(h: Tensor, W: Tensor, labels: Tensor, k: int, *, inv_h: Tensor | None = None, inv_w: Tensor | None = None,
               log_scale: Tensor | None = None, bias: Tensor | None = None, splits: int = 0):
    """-> (rows [B, 4] = {lse, target logit, rank, valid}, acc [4] = {loss, top-1, top-k, n_valid}) of the cross-entropy over the
    cosine (``inv_h``, ``inv_w``, ``log_scale``) or linear (``bias``) classifier's logits; no [B, C] buffer (include/vsx.h)"""
    B, H, Cn = _cls_operands(h, W, inv_h, inv_w, log_scale, bias)
    ptr(labels)
    if labels.dtype != torch.int64 or labels.numel() != B:
        raise TypeError(f"cls_ce_fwd: labels must be {B} int64 values, got {labels.dtype} {tuple(labels.shape)}")
    k = int(k)
    if not 1 <= k <= Cn:  # the library refuses it too; here before anything is allocated
        raise ValueError(f"cls_ce_fwd: k={k} must be in [1, C={Cn}]")
    ws = _ws(h.device, lib().vsx_cls_ce_fwd_ws_bytes(B, H, Cn), torch.float32)
    rows = torch.empty((B, 4), dtype=torch.float32, device=h.device)
    acc = torch.empty(4, dtype=torch.float32, device=h.device)
    check(lib().vsx_cls_ce_fwd(ptr(h), ptr(W), ptr(labels), ptr(inv_h), ptr(inv_w), ptr(log_scale), ptr(bias), B, H, Cn, k,
                               int(splits), ptr(rows), ptr(acc), ptr(ws), ws.nbytes, stream()), "cls_ce_fwd")
    return rows, acc


def cls_logits(h: Tensor, W: Tensor, *, inv_h: Tensor | None = None, inv_w: Tensor | None = None, log_scale: Tensor | None = None,
               bias: Tensor | None = None) -> Tensor:
    """the classifier's logits [B, C], materialised, with the rounding of ``cls_ce_fwd``"""
    B, H, Cn = _cls_operands(h, W, inv_h, inv_w, log_scale, bias)
    Z = torch.empty((B, Cn), dtype=torch.float32, device=h.device)
    check(lib().vsx_cls_logits(ptr(h), ptr(W), ptr(inv_h), ptr(inv_w), ptr(log_scale), ptr(bias), B, H, Cn, ptr(Z), stream()),
          "cls_logits")
    return Z


def cls_ce_bwd(h: Tensor, W: Tensor, labels: Tensor, rows: Tensor, acc: Tensor, gout: Tensor, dW: Tensor, *,
               inv_h: Tensor | None = None, inv_w: Tensor | None = None, log_scale: Tensor | None = None, bias: Tensor | None = None,
               dbias: Tensor | None = None, dlog_scale: Tensor | None = None) -> Tensor:
    """-> dh [B, H]; ``dW`` [C, H] and ``dbias`` [C] (linear) or ``dlog_scale`` [1] (cosine) are accumulated into"""
    B, H, Cn = _cls_operands(h, W, inv_h, inv_w, log_scale, bias)
    for t in (dW, dbias, dlog_scale, rows, acc, gout):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("cls_ce_bwd: gradient and statistics buffers must be float32")
    if dW.shape != W.shape:
        raise ValueError(f"cls_ce_bwd: dW {tuple(dW.shape)} must have W's shape {tuple(W.shape)}")
    ws = _ws(h.device, lib().vsx_cls_ce_bwd_ws_bytes(B, H, Cn), torch.float32, 4)
    dh = torch.empty_like(h)
    check(lib().vsx_cls_ce_bwd(ptr(h), ptr(W), ptr(labels), ptr(inv_h), ptr(inv_w), ptr(log_scale), ptr(bias), ptr(rows), ptr(acc),
                               ptr(gout), B, H, Cn, ptr(dh), ptr(dW), ptr(dbias), ptr(dlog_scale), ptr(ws), ws.nbytes, stream()),
          "cls_ce_bwd")
    return dh


# ------------------------------------------------------------------ MMD permutation test (csrc/mmd.hip)
def mmd_prepare(x: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """-> (xc (N, d), norms (N,), mean (d,)): the rows minus their column mean (float64 sums in a fixed order, rounded to
    float32) and the squared norms of the centred rows"""
    n, d = _rows_f32(x, "mmd_prepare")
    xc = torch.empty_like(x)
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    mean = torch.empty(d, dtype=torch.float32, device=x.device)
    check(lib().vsx_mmd_prepare(ptr(x), ptr(xc), ptr(norms), ptr(mean), n, d, stream()), "mmd_prepare")
    return xc, norms, mean


def _mmd_pool(xc: Tensor, norms: Tensor, what: str) -> tuple[int, int]:
    n, d = _rows_f32(xc, what)
    _f32_vec(norms, n, f"{what}: norms")
    return n, d


def mmd_sums(xc: Tensor, norms: Tensor, labels: Tensor, bandwidth: float) -> Tensor:
    """-> (P, 3) float64 {sum_XX, sum_YY, sum_XY} of the pooled Gaussian kernel (zero diagonal) of the centred rows ``xc`` under
    every 0 / 1 label vector of ``labels`` uint8 (P, N).  No N x N buffer: the workspace is O(P N / 128).  Bit-identical from run
    to run."""
    n, d = _mmd_pool(xc, norms, "mmd_sums")
    ptr(labels)
    if labels.dtype != torch.uint8 or labels.dim() != 2 or labels.shape[1] != n or labels.shape[0] < 1:
        raise TypeError(f"mmd_sums: labels must be a uint8 (P, {n}) tensor, got {labels.dtype} {tuple(labels.shape)}")
    P = labels.shape[0]
    ws = _ws(xc.device, lib().vsx_mmd_sums_ws_bytes(n, P), torch.float64)
    sums = torch.empty((P, 3), dtype=torch.float64, device=xc.device)
    check(lib().vsx_mmd_sums(ptr(xc), ptr(norms), ptr(labels), n, d, P, float(bandwidth), ptr(sums), ptr(ws), ws.nbytes, stream()), "mmd_sums")
    return sums


def rbf_block(xc: Tensor, norms: Tensor, rows: tuple[int, int], cols: tuple[int, int], bandwidth: float, zero_diag: bool) -> Tensor:
    """-> float32 (r1 - r0, c1 - c0): the kernel values k_ij of rows [r0, r1) x columns [c0, c1) of the centred pool, the very
    values ``mmd_sums`` sums; ``zero_diag`` stores 0 where i == j"""
    n, d = _mmd_pool(xc, norms, "rbf_block")
    (r0, r1), (c0, c1) = (int(v) for v in rows), (int(v) for v in cols)
    out = torch.empty((max(r1 - r0, 0), max(c1 - c0, 0)), dtype=torch.float32, device=xc.device)
    check(lib().vsx_rbf_block(ptr(xc), ptr(norms), n, d, r0, r1, c0, c1, float(bandwidth), int(bool(zero_diag)), ptr(out), stream()),
          "rbf_block")
    return out


def sqdist_upper(xc: Tensor, norms: Tensor) -> Tensor:
    """-> float32 (1, M (M - 1) / 2): max(n_i + n_j - 2 dot_ij, 0) for i < j, row-major over the strict upper triangle"""
    m, d = _mmd_pool(xc, norms, "sqdist_upper")
    out = torch.empty((1, max(m * (m - 1) // 2, 1)), dtype=torch.float32, device=xc.device)
    check(lib().vsx_sqdist_upper(ptr(xc), ptr(norms), m, d, ptr(out), stream()), "sqdist_upper")
    return out


# ------------------------------------------------------------------ PCA data passes (csrc/pca.hip)
def _f64_vec(t: Tensor, n: int, what: str) -> None:
    ptr(t)
    if t.dtype != torch.float64 or t.numel() != n:
        raise TypeError(f"{what} must be {n} float64 values, got {t.dtype} {tuple(t.shape)}")


def col_moments(x: Tensor) -> tuple[Tensor, Tensor]:
    """-> (mean (d,), m2 (d,)) float64: the column mean and the centred sum of squares of x float32 (n, d), two fixed-order
    float64 passes; bit-identical from run to run"""
    n, d = _rows_f32(x, "col_moments")
    ws = _ws(x.device, lib().vsx_col_moments_ws_bytes(n, d), torch.float64)
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    m2 = torch.empty(d, dtype=torch.float64, device=x.device)
    check(lib().vsx_col_moments(ptr(x), n, d, ptr(mean), ptr(m2), ptr(ws), ws.nbytes, stream()), "col_moments")
    return mean, m2


def gram_rows_per_split(n: int, d: int) -> int:
    """rows one workgroup of ``gram_centered`` folds into its float64 tile: a multiple of 128, a function of (n, d) alone"""
    return int(lib().vsx_gram_rows_per_split(int(n), int(d)))


def gram_centered(x: Tensor, mean: Tensor) -> Tensor:
    """-> float64 (d, d): (x - mean)' (x - mean), symmetric bit for bit; fp32 products on the MFMA summed over blocks of 128 rows,
    float64 past the block.  The workspace is O(splits d^2)."""
    n, d = _rows_f32(x, "gram_centered")
    _f64_vec(mean, d, "gram_centered: mean")
    ws = _ws(x.device, lib().vsx_gram_ws_bytes(n, d), torch.float64)
    gram = torch.empty((d, d), dtype=torch.float64, device=x.device)
    check(lib().vsx_gram_centered(ptr(x), n, d, ptr(mean), ptr(gram), ptr(ws), ws.nbytes, stream()), "gram_centered")
    return gram


def center_project(x: Tensor, mean: Tensor, w: Tensor) -> Tensor:
    """-> float32 (n, k): (x - mean) w' for w float32 (k, d), the dots of the f32 tile engine over the centred rows"""
    n, d = _rows_f32(x, "center_project")
    _f64_vec(mean, d, "center_project: mean")
    ptr(w)
    if w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != d or w.shape[0] < 1:
        raise TypeError(f"center_project: w must be a float32 (k, {d}) tensor, got {w.dtype} {tuple(w.shape)}")
    k = w.shape[0]
    z = torch.empty((n, k), dtype=torch.float32, device=x.device)
    check(lib().vsx_center_project(ptr(x), n, d, ptr(mean), ptr(w), k, ptr(z), stream()), "center_project")
    return z


# ------------------------------------------------------------------ logistic-regression data passes (csrc/logreg.hip, csrc/pca.hip)
def gram_scaled(x: Tensor, q: Tensor, mean: Tensor | None = None) -> Tensor:
    """-> float64 (d, d): sum_i fl32(q_i c_i)' fl32(q_i c_i) with c = fl32(x - mean) (``mean=None``: c = x), q float32 (n,):
    ``gram_centered``'s kernel, split plan and fold with one fp32 multiply more; symmetric bit for bit"""
    n, d = _rows_f32(x, "gram_scaled")
    _f32_vec(q, n, "gram_scaled: q")
    if mean is not None:
        _f64_vec(mean, d, "gram_scaled: mean")
    ws = _ws(x.device, lib().vsx_gram_ws_bytes(n, d), torch.float64)
    gram = torch.empty((d, d), dtype=torch.float64, device=x.device)
    check(lib().vsx_gram_scaled(ptr(x), n, d, ptr(mean), ptr(q), ptr(gram), ptr(ws), ws.nbytes, stream()), "gram_scaled")
    return gram


def wcolsum(x: Tensor, v: Tensor) -> Tensor:
    """-> float64 (m, d): v x for v float64 (m, n), 1 <= m <= 4, x float32 (n, d) read once; float64 fma, fixed-order folds"""
    n, d = _rows_f32(x, "wcolsum")
    ptr(v)
    if v.dtype != torch.float64 or v.dim() != 2 or v.shape[1] != n or not 1 <= v.shape[0] <= 4:
        raise TypeError(f"wcolsum: v must be a float64 (m, {n}) tensor with 1 <= m <= 4, got {v.dtype} {tuple(v.shape)}")
    m = v.shape[0]
    ws = _ws(x.device, lib().vsx_wcolsum_ws_bytes(n, d, m), torch.float64)
    out = torch.empty((m, d), dtype=torch.float64, device=x.device)
    check(lib().vsx_wcolsum(ptr(x), n, d, ptr(v), m, ptr(out), ptr(ws), ws.nbytes, stream()), "wcolsum")
    return out


def logreg_margins(x: Tensor, w: Tensor, b: float) -> Tensor:
    """-> float64 (n,): z = x w + b, the dot order of ``logreg_rows`` (the decision function shares it with the fit)"""
    n, d = _rows_f32(x, "logreg_margins")
    _f64_vec(w, d, "logreg_margins: w")
    z = torch.empty(n, dtype=torch.float64, device=x.device)
    check(lib().vsx_logreg_rows(ptr(x), n, d, ptr(w), float(b), None, 0, 0.0, 0.0, ptr(z), None, None, None, None, None, 0, stream()),
          "logreg_margins")
    return z


def logreg_rows(x: Tensor, w: Tensor, b: float, labels: Tensor, pos: int, cp: float, cn: float, *, margins: bool = False,
                derivatives: bool = True) -> dict[str, Tensor]:
    """The row pass of the weighted logistic objective, float64: y = +1 where ``labels == pos`` else -1, c = cp | cn, m = y z.
    -> {"sums": (3,) {sum loss, sum r, sum s}} and, with ``derivatives``, "r" = dloss/dz, "s" = d2loss/dz2 (float64 (n,), the two rows of "rs") and
    "q" = fl32(sqrt(s)) (float32 (n,), the row scale of ``gram_scaled``); with ``margins`` also "z".  A line-search trial asks for
    the sums alone."""
    n, d = _rows_f32(x, "logreg_rows")
    _f64_vec(w, d, "logreg_rows: w")
    _i32(labels, n, "logreg_rows: labels")
    dev = x.device
    out = {"sums": torch.empty(3, dtype=torch.float64, device=dev)}
    if derivatives:
        out["rs"] = torch.empty((2, n), dtype=torch.float64, device=dev)   # r over s: the v of ``wcolsum``
        out["r"], out["s"] = out["rs"][0], out["rs"][1]
        out["q"] = torch.empty(n, dtype=torch.float32, device=dev)
    if margins:
        out["z"] = torch.empty(n, dtype=torch.float64, device=dev)
    ws = _ws(dev, lib().vsx_logreg_rows_ws_bytes(n, d), torch.float64)
    check(lib().vsx_logreg_rows(ptr(x), n, d, ptr(w), float(b), ptr(labels), int(pos), float(cp), float(cn), ptr(out.get("z")),
                                ptr(out.get("r")), ptr(out.get("s")), ptr(out.get("q")), ptr(out["sums"]), ptr(ws), ws.nbytes, stream()),
          "logreg_rows")
    return out


# ------------------------------------------------------------------ temporal smoothness (csrc/smoothness.hip)
PAIR_METRICS = {"cosine": L.PAIR_COSINE, "euclidean": L.PAIR_EUCLIDEAN}


def standardize(x: Tensor, mean: Tensor, scale: Tensor, out: Tensor | None = None) -> Tensor:
    """-> float32 (n, d): fl32(double(fl32(double(x) - mean)) / scale), sklearn's ``StandardScaler.transform`` of a float32 matrix
    bit for bit; mean, scale float64 (d,).  ``out`` may be ``x`` (in place)"""
    n, d = _rows_f32(x, "standardize")
    _f64_vec(mean, d, "standardize: mean")
    _f64_vec(scale, d, "standardize: scale")
    if out is None:
        out = torch.empty_like(x)
    elif _rows_f32(out, "standardize: out") != (n, d):
        raise TypeError(f"standardize: out must be a float32 ({n}, {d}) tensor, got {tuple(out.shape)}")
    check(lib().vsx_standardize(ptr(x), ptr(mean), ptr(scale), ptr(out), n, d, stream()), "standardize")
    return out


def pair_dist(x: Tensor, pi: Tensor, pj: Tensor, metric: str = "cosine", eps: float = 0.0) -> Tensor:
    """-> float64 (P,): the ``metric`` ("cosine" | "euclidean") distance of rows pi[p] and pj[p] of x float32 (n, d), float64 sums
    in one fixed order.  Cosine: 1 - uv / (max(|u|, eps) max(|v|, eps)); ``eps=0`` is scipy's cdist (NaN for a zero row), ``1e-12``
    is ``F.normalize``'s rule.  An index outside [0, n) gives NaN"""
    n, d = _rows_f32(x, "pair_dist")
    if metric not in PAIR_METRICS:
        raise ValueError(f"pair_dist: metric {metric!r} must be 'cosine' or 'euclidean'")
    if n >= 2 ** 31:  # the library takes n as int32: ctypes would wrap it silently
        raise ValueError(f"pair_dist: x has {n} rows, the kernel serves fewer than 2^31")
    p = pi.numel()
    _i32(pi, p, "pair_dist: pi")
    _i32(pj, p, "pair_dist: pj")
    out = torch.empty(p, dtype=torch.float64, device=x.device)
    if p:
        check(lib().vsx_pair_dist(ptr(x), n, ptr(pi), ptr(pj), p, d, PAIR_METRICS[metric], float(eps), ptr(out), stream()), "pair_dist")
    return out


def kde_chunks(n: int, m: int) -> int:
    """how many chunks ``kde_gauss`` splits n data into for m grid points: a function of (n, m) alone"""
    return int(lib().vsx_kde_gauss_ws_bytes(int(n), int(m))) // (8 * int(m))


def kde_gauss(data: Tensor, grid: Tensor, a: float) -> Tensor:
    """-> float64 (m,): sum_i exp(-a (grid_g - data_i)^2) for data (n,), grid (m,) float64; fixed-order sums, bit-identical from run
    to run.  The caller normalises (``1 / (n sqrt(2 pi cov))`` with ``a = 1 / (2 cov)``)"""
    n, m = data.numel(), grid.numel()
    _f64_vec(data, n, "kde_gauss: data")
    _f64_vec(grid, m, "kde_gauss: grid")
    ws = _ws(data.device, lib().vsx_kde_gauss_ws_bytes(n, m), torch.float64)
    out = torch.empty(m, dtype=torch.float64, device=data.device)
    check(lib().vsx_kde_gauss(ptr(data), n, ptr(grid), m, float(a), ptr(out), ptr(ws), ws.nbytes, stream()), "kde_gauss")
    return out


# ------------------------------------------------------------------ clustering evaluation (csrc/clustering.hip + f64_tile.h)
F64_TILE, F64_KC = L.F64_TILE, L.F64_KC
PDIST_METRICS = {"cosine": L.PDIST_COSINE, "euclidean": L.PDIST_EUCLIDEAN, "sqeuclidean": L.PDIST_SQEUCLIDEAN}
F64_MAX_ROWS = 65535 * L.F64_TILE


def _f64_rows(x: Tensor, what: str) -> tuple[int, int]:
    n, d = _rows_f32(x, what)
    if not 1 <= n <= F64_MAX_ROWS:  # the library takes N as int32: ctypes would wrap it silently
        raise ValueError(f"{what}: x has {n} rows, the kernels serve 1 .. {F64_MAX_ROWS}")
    return n, d


def _typed(t: Tensor, dtype: torch.dtype, shape: tuple, what: str) -> Tensor:
    ptr(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise TypeError(f"{what} must be a {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def row_sqnorm_f64(x: Tensor) -> Tensor:
    """-> float64 (N,): the float64 engine's own dot of every row with itself, the bits a tile holds for dot_ii"""
    n, d = _f64_rows(x, "row_sqnorm_f64")
    norms = torch.empty(n, dtype=torch.float64, device=x.device)
    check(lib().vsx_row_sqnorm_f64(ptr(x), n, d, ptr(norms), stream()), "row_sqnorm_f64")
    return norms


def pdist_f64(x: Tensor, norms: Tensor, metric: str = "cosine", rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
              out: Tensor | None = None) -> Tensor:
    """-> float64 (r1 - r0, c1 - c0): the block ``rows`` x ``cols`` (the whole matrix by default) of the ``metric`` ("cosine" |
    "euclidean" | "sqeuclidean") distance matrix of x float32 (N, d); ``norms`` from ``row_sqnorm_f64``.  Exactly 0 for i == j,
    symmetric bit for bit, and a block equals the slice of the whole matrix.  ``out``: a contiguous float64 tensor of that shape"""
    n, d = _f64_rows(x, "pdist_f64")
    _f64_vec(norms, n, "pdist_f64: norms")
    if metric not in PDIST_METRICS:
        raise ValueError(f"pdist_f64: metric {metric!r} must be one of {sorted(PDIST_METRICS)}")
    (r0, r1), (c0, c1) = rows or (0, n), cols or (0, n)
    if not (0 <= r0 < r1 <= n and 0 <= c0 < c1 <= n):
        raise ValueError(f"pdist_f64: the block [{r0}, {r1}) x [{c0}, {c1}) must lie in [0, {n})")
    if out is None:
        out = torch.empty((r1 - r0, c1 - c0), dtype=torch.float64, device=x.device)
    _typed(out, torch.float64, (r1 - r0, c1 - c0), "pdist_f64: out")
    check(lib().vsx_pdist_f64(ptr(x), ptr(norms), n, d, PDIST_METRICS[metric], r0, r1, c0, c1, ptr(out), c1 - c0, stream()), "pdist_f64")
    return out


def eps_graph_words(n: int) -> int:
    """64-bit words per row of the bit matrix of ``eps_graph``"""
    return -(-int(n) // 64)


def eps_graph(x: Tensor, norms: Tensor, eps2: float, adj: Tensor | None = None, deg: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """-> (adj int64 (N, ceil(N / 64)) holding the uint64 words, deg int32 (N,)): bit b of word w of row i is set iff j = 64 w + b < N
    and (i == j or the squared Euclidean distance <= eps2); deg = the popcount of the row.  ``adj`` / ``deg``: buffers to fill, any
    contents"""
    n, d = _f64_rows(x, "eps_graph")
    _f64_vec(norms, n, "eps_graph: norms")
    eps2 = float(eps2)
    if not 0.0 <= eps2 < float("inf"):
        raise ValueError(f"eps_graph: eps2={eps2} must be finite and >= 0")
    w = eps_graph_words(n)
    adj = torch.empty((n, w), dtype=torch.int64, device=x.device) if adj is None else _typed(adj, torch.int64, (n, w), "eps_graph: adj")
    deg = torch.empty(n, dtype=torch.int32, device=x.device) if deg is None else _typed(deg, torch.int32, (n,), "eps_graph: deg")
    check(lib().vsx_eps_graph(ptr(x), ptr(norms), n, d, eps2, ptr(adj), ptr(deg), stream()), "eps_graph")
    return adj, deg


def _graph(adj: Tensor, core: Tensor, labels: Tensor, what: str) -> int:
    n = int(core.numel())
    if not 1 <= n <= F64_MAX_ROWS:
        raise ValueError(f"{what}: {n} rows, the kernels serve 1 .. {F64_MAX_ROWS}")
    _typed(adj, torch.int64, (n, eps_graph_words(n)), f"{what}: adj")
    _typed(core, torch.uint8, (n,), f"{what}: core")
    _typed(labels, torch.int32, (n,), f"{what}: labels")
    return n


def cc_round(adj: Tensor, core: Tensor, labels: Tensor, changed: Tensor) -> None:
    """one round of minimum-label hooking over core-core edges plus pointer jumping, in place on ``labels`` int32 (N,); ``changed``
    int32 (1,) is 1 afterwards iff a label was lowered"""
    n = _graph(adj, core, labels, "cc_round")
    _typed(changed, torch.int32, (1,), "cc_round: changed")
    check(lib().vsx_cc_round(ptr(adj), ptr(core), ptr(labels), n, ptr(changed), stream()), "cc_round")


def dbscan_finish(adj: Tensor, core: Tensor, labels: Tensor, cid: Tensor, out: Tensor | None = None) -> Tensor:
    """-> int32 (N,): ``cid[labels[i]]`` for a core row, the smallest ``cid[labels[j]]`` over the core neighbours j of any other row,
    -1 where it has none"""
    n = _graph(adj, core, labels, "dbscan_finish")
    _typed(cid, torch.int32, (n,), "dbscan_finish: cid")
    out = torch.empty(n, dtype=torch.int32, device=adj.device) if out is None else _typed(out, torch.int32, (n,), "dbscan_finish: out")
    check(lib().vsx_dbscan_finish(ptr(adj), ptr(core), ptr(labels), ptr(cid), n, ptr(out), stream()), "dbscan_finish")
    return out


# ------------------------------------------------------------------------------------------------ stored frames: patch gathers (DynaCLR data feeds)
# the storage dtypes the frame kernels read, each converting to float32 exactly: (numpy dtype, torch dtype, VSX_PG_* code)
FRAME_DTYPES = ((np.dtype(np.float32), torch.float32, L.PG_F32), (np.dtype(np.uint16), torch.uint16, L.PG_U16),
                (np.dtype(np.int16), torch.int16, L.PG_I16), (np.dtype(np.uint8), torch.uint8, L.PG_U8))
PATCH_GATHER_DTYPES = {t: code for _, t, code in FRAME_DTYPES}
STORAGE_DTYPES = {n: t for n, t, _ in FRAME_DTYPES}


def frame_dtype_code(dtype: torch.dtype, who: str) -> int:
    """the ``VSX_PG_*`` code of a frame's storage dtype; one the kernels do not read raises ``NotImplementedError``"""
    code = PATCH_GATHER_DTYPES.get(dtype)
    if code is None:
        raise NotImplementedError(f"{who}: frames stored as {dtype} are not built (float32, uint16, int16, uint8 are)")
    return code


def _frame_info(who: str, i: int, f: Tensor, f0: Tensor, seen: dict, same_cz: bool = False) -> tuple:
    """``(data_ptr, stride c, stride z, stride y), shape, f`` of frame ``i`` of a launch whose frame 0 is ``f0``: a (C, Z, H, W) tensor
    (any view whose last axis is contiguous) of frame 0's dtype and device and, with ``same_cz``, its C and Z.  A frame serves many
    patches of a batch and is inspected once per object: ``seen`` maps ``id`` to the answer, which holds the object (a temporary must
    not hand its address to the next one), and the loops ask it first: ``seen.get(id(f)) or _frame_info(...)``."""
    if f.ndim != 4 or f.dtype != f0.dtype or f.device != f0.device or (same_cz and tuple(f.shape[:2]) != tuple(f0.shape[:2])):
        raise ValueError(f"{who}: frame {i} is {tuple(f.shape)} {f.dtype} on {f.device}, frame 0 is {tuple(f0.shape)} {f0.dtype} on "
                         f"{f0.device}: one launch serves (C, Z, H, W) frames of one dtype" + (", C and Z" if same_cz else " and device"))
    sc, sz, sy, sx = f.stride()
    if (sx != 1 and f.shape[3] > 1) or min(sc, sz, sy) < 0:
        raise ValueError(f"{who}: frame {i} has strides {f.stride()}: x must be contiguous, the others >= 0")
    info = seen[id(f)] = ((f.data_ptr(), sc, sz, sy), tuple(f.shape), f)
    return info


def _gather_out(who: str, f0: Tensor, host_path: str, shape: tuple, out: Tensor | None, table_words: int = 0) -> Tensor:
    """the checks a gather makes once its tables stand, and its float32 output"""
    if not f0.is_cuda:
        raise RuntimeError(f"viscy_amd: {who} runs on the HIP device only (host patches: {host_path})")
    if shape[0] * shape[1] * shape[2] * shape[3] * shape[4] >= 2 ** 62 or max(shape) >= 2 ** 31 or table_words >= 2 ** 31:
        raise ValueError(f"{who}: sizes exceed the kernel's index range")
    return torch.empty(shape, dtype=torch.float32, device=f0.device) if out is None else _typed(out, torch.float32, shape, f"{who}: out")


def patch_descriptors(frames: Sequence[Tensor], origins: Sequence[Sequence[int]], size: Sequence[int]) -> Tensor:
    """The descriptor table of ``vsx_patch_gather`` as an int64 (n, PG_DESC) host tensor, every row checked: frame ``i`` is a
    (C, Z, H, W) tensor (any view whose last axis is contiguous), ``origins[i] = (y0, x0)``, ``size = (Yp, Xp)``.  A patch that
    leaves its frame on any side raises ``ValueError``; a storage dtype the kernel does not read raises ``NotImplementedError``.
    Host code: works on tensors of any device."""
    yp, xp = (int(v) for v in size)
    if len(frames) == 0 or len(frames) != len(origins):
        raise ValueError(f"patch_gather: {len(frames)} frames for {len(origins)} origins")
    if yp <= 0 or xp <= 0:
        raise ValueError(f"patch_gather: patch size {(yp, xp)} must be positive")
    f0 = frames[0]
    frame_dtype_code(f0.dtype, "patch_gather")
    rows, seen = [], {}
    for i, (f, (y0, x0)) in enumerate(zip(frames, origins)):
        desc, (_, _, H, W), _ = seen.get(id(f)) or _frame_info("patch_gather", i, f, f0, seen, same_cz=True)
        y0, x0 = int(y0), int(x0)
        if y0 < 0 or y0 + yp > H:
            raise ValueError(f"patch_gather: patch {i} rows [{y0}, {y0 + yp}) leave the frame's [0, {H})")
        if x0 < 0 or x0 + xp > W:
            raise ValueError(f"patch_gather: patch {i} columns [{x0}, {x0 + xp}) leave the frame's [0, {W})")
        rows.append(desc + (y0, x0))
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), L.PG_DESC)


def patch_gather(frames: Sequence[Tensor], origins: Sequence[Sequence[int]], size: Sequence[int], out: Tensor | None = None) -> Tensor:
    """-> float32 (n, C, Z, Yp, Xp): ``out[i] = frames[i][:, :, y0:y0 + Yp, x0:x0 + Xp]`` converted exactly, ONE launch for all n.
    The table is checked and uploaded here (one small pinned copy); the frames must stay alive until the launch has been issued
    on the current stream, which the caller's references guarantee."""
    table = patch_descriptors(frames, origins, size)
    f0 = frames[0]
    n, (C, Z), (yp, xp) = len(frames), f0.shape[:2], (int(v) for v in size)
    out = _gather_out("patch_gather", f0, "viscy_amd.data.triplet.host_cut", (n, C, Z, yp, xp), out)
    dev_table = table.pin_memory().to(f0.device, non_blocking=True)
    check(lib().vsx_patch_gather(ptr(dev_table), ptr(out), n, C, Z, yp, xp, PATCH_GATHER_DTYPES[f0.dtype], stream()), "patch_gather")
    return out


PGS_AXES = ("channel", "z", "y", "x")


def patch_tables(frames: Sequence[Tensor], channels: Sequence, zs: Sequence, ys: Sequence, xs: Sequence) -> tuple[Tensor, Tensor, tuple]:
    """The descriptor rows and the index tables of ``vsx_patch_gather_scaled`` as host tensors: int64 (n, PGS_DESC) and int32 (T,),
    plus the output shape (n, C, Zt, Yt, Xt).  Frame ``i`` is a (Cf, Zf, H, W) tensor (any view whose last axis is contiguous;
    frames of one launch share the dtype and the device, not the shape); ``channels[i]``, ``zs[i]``, ``ys[i]``, ``xs[i]`` are its
    1-D integer tables of ABSOLUTE positions in that frame (arrays, rows of a 2-D array, tensors, lists).  A table OBJECT named
    by several patches is stored once; objects are told apart by identity and held until the call returns.  Every
    entry is checked against its frame: one outside raises ``ValueError`` naming the patch and the axis.  Host code."""
    n = len(frames)
    if n == 0 or not (len(channels) == len(zs) == len(ys) == len(xs) == n):
        raise ValueError(f"patch_gather_scaled: {n} frames for {len(channels)} / {len(zs)} / {len(ys)} / {len(xs)} tables")
    f0 = frames[0]
    frame_dtype_code(f0.dtype, "patch_gather_scaled")
    segs, seg_of, seg = [], {}, np.empty((n, 4), dtype=np.int64)  # distinct tables, id -> position in segs, per patch and axis
    held = []  # every table whose id() is a key: a temporary (a row of a 2-D array) must not hand its address to the next one
    rows, dims, seen = np.empty((n, 4), dtype=np.int64), np.empty((n, 4), dtype=np.int64), {}
    for i, f in enumerate(frames):
        rows[i], dims[i], _ = seen.get(id(f)) or _frame_info("patch_gather_scaled", i, f, f0, seen)
        for a, t in enumerate((channels[i], zs[i], ys[i], xs[i])):
            k = seg_of.get(id(t))
            if k is None:
                arr = np.asarray(t)
                if arr.ndim != 1 or arr.size == 0 or arr.dtype.kind not in "iu":
                    raise ValueError(f"patch_gather_scaled: patch {i} {PGS_AXES[a]} table must be a non-empty 1-D integer array")
                k = seg_of[id(t)] = len(segs)
                held.append(t)
                segs.append(arr.astype(np.int64, copy=False))
            seg[i, a] = k
    lengths = np.array([s.size for s in segs], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    flat = np.concatenate(segs)
    lo, hi = np.minimum.reduceat(flat, starts), np.maximum.reduceat(flat, starts)
    size = lengths[seg]  # (n, 4): C, Zt, Yt, Xt of every patch
    if (size != size[0]).any():
        i, a = (int(v[0]) for v in np.nonzero(size != size[0]))
        raise ValueError(f"patch_gather_scaled: patch {i} {PGS_AXES[a]} table has {int(size[i, a])} entries, patch 0 has "
                         f"{int(size[0, a])}: one launch writes one (C, Zt, Yt, Xt)")
    bad = (lo[seg] < 0) | (hi[seg] >= dims)
    if bad.any():
        i, a = (int(v[0]) for v in np.nonzero(bad))
        raise ValueError(f"patch_gather_scaled: patch {i} {PGS_AXES[a]} table spans [{int(lo[seg[i, a]])}, {int(hi[seg[i, a]])}], "
                         f"which leaves the frame's [0, {int(dims[i, a])})")
    desc = torch.from_numpy(np.concatenate((rows, starts[seg]), axis=1))
    return desc, torch.from_numpy(flat.astype(np.int32)), (n, *(int(v) for v in size[0]))


def patch_gather_scaled(frames: Sequence[Tensor], channels: Sequence, zs: Sequence, ys: Sequence, xs: Sequence,
                        out: Tensor | None = None) -> Tensor:
    """-> float32 (n, C, Zt, Yt, Xt): ``out[i] = frames[i][channels[i]][:, zs[i]][:, :, ys[i]][:, :, :, xs[i]]`` converted exactly, ONE
    launch for all n: per-patch channel lists, per-patch boxes in frames of different shapes, and the resampling that the tables
    spell out (``viscy_amd.data.multi_experiment.nearest_exact_index``).  Tables and descriptors are checked on the host
    (``patch_tables``) and travel in one pinned copy; nothing is launched when a check fails.  The frames must stay alive until
    the launch has been issued on the current stream, which the caller's references guarantee."""
    desc, idx, shape = patch_tables(frames, channels, zs, ys, xs)
    f0 = frames[0]
    n, C, Zt, Yt, Xt = shape
    if Xt > L.PGS_MAX_XT:
        raise ValueError(f"patch_gather_scaled: Xt={Xt}, the kernel holds x tables of at most {L.PGS_MAX_XT} entries")
    out = _gather_out("patch_gather_scaled", f0, "viscy_amd.data.multi_experiment.host_gather", shape, out, idx.numel())
    words = n * L.PGS_DESC
    both = torch.empty(words + (idx.numel() + 1) // 2, dtype=torch.int64, pin_memory=True)  # descriptors, then the int32 tables
    both[:words] = desc.reshape(-1)
    both[words:].view(torch.int32)[: idx.numel()] = idx
    dev = both.to(f0.device, non_blocking=True)
    check(lib().vsx_patch_gather_scaled(ptr(dev), ptr(dev[words:]), ptr(out), n, C, Zt, Yt, Xt, PATCH_GATHER_DTYPES[f0.dtype], stream()),
          "patch_gather_scaled")
    return out
