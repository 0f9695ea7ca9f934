"""GPU: the MMD kernels of csrc/mmd.hip on the exact cluster pools of tests/ref_exact_tile.py, at sizes where a workgroup of
mmd_sums_kernel walks two and three column tiles (N >= 2945; the case table's legs are asserted in tests/test_tile_exact_cpu.py).

Every comparison is on bits.  Kernel values are 1 inside a cluster and +0 across (zero diagonal), so rectangles of
ops.rbf_block equal the indicator, ops.sqdist_upper equals the integer distances, ops.mmd_prepare returns a zero mean, the rows
themselves and the integer norms, and ops.mmd_sums equals the integer closed form for P + 1 on both sides of the 128-vector label
chunk.  The rectangles come first, so that a surprise in expf reports as such and not as a wrong sum.

The probe's share (knn_topk_kernel past one candidate tile per workgroup) lives in tests/test_gpu_online_eval.py; the leg it
needs depends on the device's compute-unit count and is asserted here and there, never skipped."""

import functools
import time

import numpy as np
import pytest
import torch

from tests import ref_exact_tile as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _off_grid(a, off):
    """a copy of ``a`` on the device whose first element lies ``off`` elements past a 16-byte boundary"""
    t = torch.tensor(a)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (off * t.element_size()) % 16 != 0
    return view


@functools.lru_cache(maxsize=None)
def _device_pool(name):
    """-> (x, norms, cluster ids) on the device, once per case; the views case holds x 4 bytes off the 16-byte grid"""
    c = X.mmd_case(name)
    x, cid = X.cluster_pool(c["N"], c["d"])
    xd = _off_grid(x, 1) if c["views"] else torch.tensor(x, device=DEV)
    return xd, torch.tensor(X.integer_norms(x), device=DEV), torch.tensor(cid, device=DEV)


def _labels(c, P):
    z = X.labels_for(c["N"], P)
    return z, (_off_grid(z, 1) if c["views"] else torch.tensor(z, device=DEV))


@functools.lru_cache(maxsize=None)
def _sums(name, P):
    from viscy_amd import debug, ops

    c = X.mmd_case(name)
    xd, norms, _ = _device_pool(name)
    with debug.poison_empty():            # the workspace and the output start as NaN: the call initialises what it reads
        return ops.mmd_sums(xd, norms, _labels(c, P)[1], X.BANDWIDTH).cpu().numpy()


def _same_matrix(got, want, r0, c0, what, N):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i, j = (int(v) for v in bad[0])
    plan = X.mmd_plan(N)
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; first at row {r0 + i} (tile {(r0 + i) // X.T}), "
                         f"column {c0 + j} (tile {(c0 + j) // X.T}, split / position {X.split_of(plan, (c0 + j) // X.T)}): "
                         f"got {float(got[i, j])!r}, want {float(want[i, j])!r}")


def _same_sums(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    p, q = bad[0]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} sums differ, label vectors {sorted(set(bad[:, 0]))[:8]} ..; first at "
                         f"p = {p}, {('sum_XX', 'sum_YY', 'sum_XY')[q]}: got {got[p, q]!r}, want {want[p, q]!r}")


def test_the_device_gives_the_probes_cases_two_tiles_per_workgroup():
    """kt_splits depends on the compute-unit count.  A device on which these sizes fall back to one candidate tile per workgroup
    must fail here, loudly, instead of passing the bit-exact table without covering the carried lists"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for N in sorted({c["case"][0] for c in X.KNN_CASES} | {X.KNN_ORDER_CASE[0]}):
        print(f"\nknn_plan({N}, {cus} compute units): {X.knn_leg(N, cus)}")
        assert X.knn_plan(N, cus)[2] >= 2, (N, cus, X.knn_plan(N, cus))


@pytest.mark.parametrize("c", X.MMD_CASES, ids=lambda c: c["name"])
def test_mmd_kernels_on_the_cluster_pool_bit_for_bit(c):
    from viscy_amd import ops

    t0 = time.perf_counter()
    N, d, name = c["N"], c["d"], c["name"]
    assert c["leg"].startswith(X.plan_leg(N))
    xd, norms, cid = _device_pool(name)
    cid_np = X.cluster_pool(N, d)[1]

    # 1. kernel values first: rectangles inside the second tile of a split, over the last split, across the tail
    for (r0, r1), (c0, c1) in X.rectangles(N):
        K = ops.rbf_block(xd, norms, (r0, r1), (c0, c1), X.BANDWIDTH, True)
        want = torch.from_numpy(X.indicator(cid_np, (r0, r1), (c0, c1))).to(DEV)
        _same_matrix(K, want, r0, c0, f"{name}: rbf_block rows {r0}..{r1} x columns {c0}..{c1}", N)
    # ... and then every tile, in slices of 1024 rows against the indicator formed on the device
    col = torch.arange(N, device=DEV)
    for r0 in range(0, N, 1024):
        r1 = min(r0 + 1024, N)
        want = ((cid[r0:r1, None] == cid[None, :]) & (col[r0:r1, None] != col[None, :])).float()
        _same_matrix(ops.rbf_block(xd, norms, (r0, r1), (0, N), X.BANDWIDTH, True), want, r0, 0, f"{name}: rbf_block rows {r0}..{r1}", N)

    # 2. the distances behind them, where the tail tile is 3 rows
    if N == 3075 and not c["views"]:
        x64 = xd.double()
        n64 = norms.double()
        i, j = torch.triu_indices(N, N, 1, device=DEV)
        want = ((n64[:, None] + n64[None, :]) - 2.0 * (x64 @ x64.t()))[i, j].float()
        got = ops.sqdist_upper(xd, norms)[0]
        assert got.shape == want.shape and float(want.min()) == 0.0 and float(want[want > 0].min()) >= 1.0
        assert torch.equal(got, want), f"{name}: sqdist_upper differs at {int((got != want).sum())} of {got.numel()} pairs"

    # 3. the public path's front end: zero mean, the rows themselves, the integer norms
    xc, nrm, mean = ops.mmd_prepare(xd)
    assert torch.equal(mean, torch.zeros(d, device=DEV)) and torch.equal(xc, xd) and torch.equal(nrm, norms)

    # 4. the sums, P + 1 on both sides of the label chunk
    for P in X.P_EDGES:
        z, _ = _labels(c, P)
        got = _sums(name, P)
        assert got.shape == (P, 3) and got.dtype == np.float64
        _same_sums(got, X.closed_form(cid_np, z), f"{name} P = {P} against the closed form ({c['leg']})")
        if c["views"]:
            _same_sums(got, _sums(name.replace("_views", ""), P), f"{name} P = {P} against the aligned run")
    print(f"\n{name}: {c['leg']}\n{name}: {time.perf_counter() - t0:.2f} s")


def test_label_rows_do_not_depend_on_their_chunk():
    """the same label vector gives the same three integers as row 0 of P = 1, row 0 of P = 300 and row 126 / 127 next to the
    virtual ones-row: s(P)[p] == s(300)[p] wherever labels_for keeps the row"""
    for c in X.MMD_CASES:
        big = _sums(c["name"], 300)
        for P in X.P_EDGES[:-1]:
            s = _sums(c["name"], P)
            keep = max(P - 2, 1) if P >= 3 else P
            assert np.array_equal(s[:keep], big[:keep]), (c["name"], P)
            if P >= 3:
                assert np.array_equal(s[-2:], big[-2:]), (c["name"], P)      # the all-zero and the all-one row
                Tt = X.closed_form(X.cluster_pool(c["N"], c["d"])[1], X.labels_for(c["N"], P))[-1, 0]
                assert (s[-2] == 0.0).sum() == 2 and s[-2, 1] == Tt and s[-1, 0] == Tt and (s[-1, 1:] == 0.0).all()
