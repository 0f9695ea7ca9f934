"""GPU: viscy_amd.smoothness and the kernels under it (csrc/smoothness.hip).

Bit-equal to the numpy restatements of tests/ref_smoothness.py: vsx_standardize (any shape, in place, a base 4 bytes off the
16-byte grid, a constant column) and vsx_pair_dist for both metrics (d around the 256-feature round of a wave, P around the four
pairs of a workgroup, both alignments; i == j gives exactly 0 under Euclidean; a zero row gives NaN with eps 0 and 1 with 1e-12).
Fed sklearn's recorded mean_ / scale_, the device's distances are within 4 (d + 8) 2^-53 of scipy's (absolute for cosine, relative
for Euclidean: both sides sum d exactly representable products in float64).  Past the grid caps of the two launches (65 536 and
2^20 workgroups) the strided loops give the same bits.

vsx_kde_gauss against the float64 terms summed in long double, and against scipy's recorded curves: B = 2 (n + 4096) 2^-53 relative
per grid value plus 1e-300 (all terms are positive, so any order errs by at most (n - 1) u; 4096 u covers exp and an argument up to
745; a dropped datum would move a value by about 1/n), at (n, m) one below, at and one above the chunk length and the grid tile,
and on a sample of a 131 072-point grid whose chunks hold three slabs each;
two runs and a run on poisoned allocations give the same bits; the peaks of the recorded distributions EQUAL the recorded peaks
(tests/test_smoothness_cpu.py shows that the curves decide them by more than 2 B).

End to end, cases A-H and the displacement fixture: exceptions by type and message; structure of the piecewise lists and of the
displacement dicts; distances within E_p = 2^-19 (cosine) or 2^-21 (|u| + |v|) (Euclidean) of the reference's (this package's
mean_ / scale_ may differ from sklearn's in the last bit: at most 2 ulp of a standardised fp32 element); mean, std and median within
max E_p; peaks within one grid step; the global numpy random state is left alone."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ref_smoothness as RS
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("smoothness.pt")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def off_grid(xd):
    """a copy of xd 4 bytes off the 16-byte grid"""
    flat = torch.empty(xd.numel() + 1, dtype=xd.dtype, device=DEV)
    view = flat[1:].view(xd.shape)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4
    return view


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ vsx_standardize
@pytest.mark.parametrize("n,d", [(1, 1), (5, 3), (130, 33), (64, 768), (3, 4097)])
def test_standardize_is_bit_equal(n, d):
    from viscy_amd import ops

    rng = np.random.RandomState(n + d)
    x = (rng.standard_normal((n, d)) * 3.0 + rng.uniform(-50, 50, d)).astype(np.float32)
    mean = x.astype(np.float64).mean(0) + rng.standard_normal(d) * 1e-9     # not representable in fp32: the float64 subtraction shows
    scale = x.astype(np.float64).std(0) + rng.uniform(0.1, 1.0, d)
    x[:, d // 2] = 7.5                                                      # a constant column: mean = the value, scale 1, zeros
    mean[d // 2], scale[d // 2] = 7.5, 1.0
    want = RS.standardize(x, mean, scale)
    assert (want[:, d // 2] == 0.0).all()
    xd, md, sd = dev(x), dev(mean), dev(scale)
    z = ops.standardize(xd, md, sd)
    assert z.dtype == torch.float32 and same_bits(z.cpu().numpy(), want)
    assert same_bits(ops.standardize(off_grid(xd), md, sd).cpu().numpy(), want)
    out = off_grid(xd)
    assert ops.standardize(xd, md, sd, out=out) is out and same_bits(out.cpu().numpy(), want)
    inplace = xd.clone()
    ops.standardize(inplace, md, sd, out=inplace)
    assert same_bits(inplace.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ vsx_pair_dist
@pytest.mark.parametrize("d", [1, 3, 4, 255, 256, 257, 260, 768, 1028])
def test_pair_dist_is_bit_equal(d):
    from viscy_amd import ops

    n = 37
    rng = np.random.RandomState(100 + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)
    x[5] = 0.0
    xd = dev(x)
    views = [xd, off_grid(xd)]
    assert views[0].data_ptr() % 16 == 0
    for P in (1, 3, 4, 5, 1025):
        pi, pj = rng.randint(0, n, P), rng.randint(0, n, P)
        pi[0], pj[0] = 9, 9                      # i == j
        if P >= 3:
            pi[1], pj[1] = 5, 11                 # a zero row
            pi[2], pj[2] = 12, 5
        pid, pjd = dev(pi.astype(np.int32)), dev(pj.astype(np.int32))
        for metric in ("cosine", "euclidean"):
            for eps in ((0.0, 1e-12) if metric == "cosine" else (0.0,)):
                want = RS.pair_dist(x, pi, pj, metric, eps)
                for v in views:
                    got = ops.pair_dist(v, pid, pjd, metric, eps)
                    assert got.dtype == torch.float64
                    assert same_bits(got.cpu().numpy(), want), (d, P, metric, eps, v.data_ptr() % 16)
                if metric == "euclidean":
                    assert want[0] == 0.0
                elif P >= 3 and d > 1:
                    assert (np.isnan(want[1:3]).all() if eps == 0.0 else (want[1:3] == 1.0).all()), (eps, want[1:3])


def test_standardize_and_pair_dist_past_their_grid_caps():
    """the launches stop growing at 65 536 (standardize) and 2^20 (pair_dist) workgroups and stride from there"""
    from viscy_amd import ops

    rng = np.random.RandomState(77)
    n = 65536 * 256 + 3                              # d = 1: 256 rows per workgroup
    x = rng.randint(-1000, 1000, (n, 1)).astype(np.float32)
    mean, scale = np.array([0.3]), np.array([1.7])
    assert same_bits(ops.standardize(dev(x), dev(mean), dev(scale)).cpu().numpy(), RS.standardize(x, mean, scale))
    # pair_dist: the list in one call equals its two halves in two calls (each below the cap), bit for bit, and the restatement
    rows = dev((rng.standard_normal((37, 3)) * 2).astype(np.float32))
    P = 4 * (1 << 20) + 5                            # four pairs per workgroup
    pi, pj = dev(rng.randint(0, 37, P).astype(np.int32)), dev(rng.randint(0, 37, P).astype(np.int32))
    for metric in ("cosine", "euclidean"):
        whole = ops.pair_dist(rows, pi, pj, metric)
        h = P // 2
        halves = torch.cat((ops.pair_dist(rows, pi[:h].contiguous(), pj[:h].contiguous(), metric),
                            ops.pair_dist(rows, pi[h:].contiguous(), pj[h:].contiguous(), metric)))
        assert torch.equal(whole.view(torch.int64), halves.view(torch.int64))
        tail = slice(P - 1000, P)
        want = RS.pair_dist(rows.cpu().numpy(), pi[tail].cpu().numpy(), pj[tail].cpu().numpy(), metric)
        assert same_bits(whole[tail].cpu().numpy(), want)


def test_pair_dist_never_reads_a_row_outside_x():
    from viscy_amd import ops

    x = dev(np.ones((4, 8), dtype=np.float32))
    pi, pj = dev(np.array([0, 4, -1, 1], dtype=np.int32)), dev(np.array([1, 0, 2, 2 ** 31 - 1], dtype=np.int32))
    got = ops.pair_dist(x, pi, pj, "euclidean").cpu().numpy()
    assert got[0] == 0.0 and np.isnan(got[1:]).all()


@functools.lru_cache(maxsize=None)
def reference_rows(name):
    """-> (x, obs, metric, offsets, z of sklearn's mean_ / scale_ (restated), pi, pj, ri, rj)"""
    from viscy_amd import smoothness as S

    x, obs, metric, offsets = RS.build(name)
    g = golden()["cases"][name]
    z = RS.standardize(x, g["mean_"].numpy(), g["scale_"].numpy())
    pi, pj, _, _ = S.adjacent_pairs(obs["fov_name"], obs["track_id"], offsets)
    ri, rj = S.random_pairs(len(x), len(pi))
    return x, obs, metric, offsets, z, pi, pj, ri, rj


def recorded(g, key, got):
    """pairs of (device values, recorded values) for a distribution: case C keeps every 16th and the run around 10 000"""
    if key + "_s16" in g:
        return [(got[::16], g[key + "_s16"].numpy()), (got[9936:10064], g[key + "_mid"].numpy())]
    return [(got, g[key].numpy())]


RUNNING = [n for n in RS.CASES if n != "F"]


@pytest.mark.parametrize("name", RUNNING)
def test_device_distances_from_sklearns_moments_are_scipys(name):
    from viscy_amd import ops

    x, obs, metric, offsets, z, pi, pj, ri, rj = reference_rows(name)
    g = golden()["cases"][name]
    zd = ops.standardize(dev(x), dev(g["mean_"].numpy()), dev(g["scale_"].numpy()))
    assert same_bits(zd.cpu().numpy(), z)
    bound = RS.pair_bound(x.shape[1])
    for key, (a, b) in (("adjacent", (pi, pj)), ("random", (ri, rj))):
        got = ops.pair_dist(zd, dev(a.astype(np.int32)), dev(b.astype(np.int32)), metric, 0.0).cpu().numpy()
        for mine, want in recorded(g, key, got):
            err = np.abs(mine - want)
            lim = bound * (np.abs(want) if metric == "euclidean" else 1.0)
            print(name, key, "max err / bound", float((err / np.maximum(lim, 1e-300)).max()))
            assert (err <= lim).all(), (name, key, float(err.max()))


# ------------------------------------------------------------------------------------------------ vsx_kde_gauss
def kde_ok(got, want, n):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    lim = RS.kde_bound(n) * want + 1e-300
    print("kde max err / bound", float((err / lim).max()))
    return bool((err <= lim).all())


KDE_SHAPES = [(n, m) for n in (RS.KDE_CHUNK - 1, RS.KDE_CHUNK, RS.KDE_CHUNK + 1) for m in (RS.KDE_TILE - 1, RS.KDE_TILE, RS.KDE_TILE + 1)]


@pytest.mark.parametrize("n,m", KDE_SHAPES + [(1, 1), (2, 1000), (70000, 257)])
def test_kde_gauss_against_long_double(n, m):
    from viscy_amd import _lib, debug, ops

    assert (_lib.KDE_TILE, _lib.KDE_CHUNK) == (RS.KDE_TILE, RS.KDE_CHUNK)
    assert ops.kde_chunks(n, m) == (1 if n <= RS.KDE_CHUNK else 2 if n <= 2 * RS.KDE_CHUNK else -(-n // RS.KDE_CHUNK))
    rng = np.random.RandomState(n + m)
    data = np.concatenate([rng.normal(0.3, 0.05, n // 2), rng.normal(0.7, 0.1, n - n // 2)])
    grid = np.linspace(data.min() - 0.2, data.max() + 0.2, m) if m > 1 else np.array([0.4])
    for a in (RS.kde_a(data) if n > 1 else 3.0, 2.0e3):      # Scott's bandwidth, and one whose far terms underflow
        want = RS.kde_sums(data, grid, a)
        dd, gd = dev(data), dev(grid)
        out = ops.kde_gauss(dd, gd, a)
        assert out.dtype == torch.float64 and out.shape == (m,)
        assert kde_ok(out.cpu().numpy(), want, n), (n, m, a)
        assert torch.equal(ops.kde_gauss(dd, gd, a), out)
        with debug.poison_empty():
            assert torch.equal(ops.kde_gauss(dd, gd, a), out)
        with debug.poison_empty(1e300):
            assert torch.equal(ops.kde_gauss(dd, gd, a), out)


def test_kde_gauss_chunks_of_several_slabs():
    """256 grid tiles leave 2048 / 256 = 8 workgroups per tile: 21 slabs of data go into 7 chunks of 3 slabs.  The grid is too
    large to restate whole; a sample of its points (tile edges, both ends, random ones) is held to the same bound"""
    from viscy_amd import debug, ops

    n, m = 20 * RS.KDE_CHUNK + 7, 256 * RS.KDE_TILE
    assert ops.kde_chunks(n, m) == 7
    rng = np.random.RandomState(9)
    data = np.concatenate([rng.normal(0.3, 0.05, n // 2), rng.normal(0.7, 0.1, n - n // 2)])
    grid = np.linspace(data.min() - 0.2, data.max() + 0.2, m)
    a = RS.kde_a(data)
    dd, gd = dev(data), dev(grid)
    out = ops.kde_gauss(dd, gd, a)
    with debug.poison_empty():
        assert torch.equal(ops.kde_gauss(dd, gd, a), out)
    pick = np.unique(np.concatenate([[0, 1, 255, 256, RS.KDE_TILE - 1, RS.KDE_TILE, m - RS.KDE_TILE - 1, m - RS.KDE_TILE, m - 1],
                                     rng.randint(0, m, 200)]))
    assert kde_ok(out.cpu().numpy()[pick], RS.kde_sums(data, grid[pick], a), n)


@pytest.mark.parametrize("key", ["adjacent", "random"])
def test_kde_on_recorded_distances_is_scipys_curve_and_peak(key):
    from viscy_amd import ops
    from viscy_amd import smoothness as S

    g = golden()
    data, curve = g["cases"]["A"][key].numpy(), g["curves"][key].numpy()
    grid = np.linspace(data.min(), data.max(), RS.GRID)
    sums = ops.kde_gauss(dev(data), dev(grid), RS.kde_a(data)).cpu().numpy()
    assert kde_ok(S.kde_curve(data, sums), curve, len(data))


    # the curve decides its peak by more than 2 B (tests/test_smoothness_cpu.py): equal, not close
    assert S.find_distribution_peak(data) == g["cases"]["A"]["stats"][key + "_frame_peak"]
    assert S.find_distribution_peak(dev(data)) == g["cases"]["A"]["stats"][key + "_frame_peak"]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone():
    from viscy_amd import _lib, ops

    l = _lib.lib()
    s = _lib.stream()
    x = dev(np.ones((4, 8), dtype=np.float32))
    vec = dev(np.ones(8))
    idx = dev(np.zeros(4, dtype=np.int32))
    out32 = torch.full((4, 8), 5.0, device=DEV)
    out64 = torch.full((8,), 5.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(8, dtype=torch.float64, device=DEV)
    p = _lib.ptr
    assert l.vsx_kde_gauss_ws_bytes(8, 8) == 64 and l.vsx_kde_gauss_ws_bytes(0, 8) == 0 and l.vsx_kde_gauss_ws_bytes(8, 0) == 0
    assert l.vsx_kde_gauss_ws_bytes(2 ** 31, 8) == 0 and l.vsx_kde_gauss_ws_bytes(8, 2 ** 20 + 1) == 0
    refused = [
        l.vsx_standardize(None, p(vec), p(vec), p(out32), 4, 8, s),
        l.vsx_standardize(p(x), None, p(vec), p(out32), 4, 8, s),
        l.vsx_standardize(p(x), p(vec), p(vec), None, 4, 8, s),
        l.vsx_standardize(p(x), p(vec), p(vec), p(out32), 0, 8, s),
        l.vsx_standardize(p(x), p(vec), p(vec), p(out32), 4, 0, s),
        l.vsx_pair_dist(None, 4, p(idx), p(idx), 4, 8, 0, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, None, p(idx), 4, 8, 0, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 4, 8, 0, 0.0, None, s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 0, 8, 0, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 2 ** 33, 8, 0, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 4, 0, 0, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 4, 8, 2, 0.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 4, 8, 0, -1.0, p(out64), s),
        l.vsx_pair_dist(p(x), 4, p(idx), p(idx), 4, 8, 0, float("nan"), p(out64), s),
        l.vsx_kde_gauss(None, 8, p(vec), 8, 1.0, p(out64), p(ws), 64, s),
        l.vsx_kde_gauss(p(vec), 8, p(vec), 8, 1.0, p(out64), None, 64, s),
        l.vsx_kde_gauss(p(vec), 0, p(vec), 8, 1.0, p(out64), p(ws), 64, s),
        l.vsx_kde_gauss(p(vec), 8, p(vec), 0, 1.0, p(out64), p(ws), 64, s),
        l.vsx_kde_gauss(p(vec), 8, p(vec), 8, 1.0, p(out64), p(ws), 63, s),
        l.vsx_kde_gauss(p(vec), 8, p(vec), 8, 1.0, p(out64), ctypes.c_void_p(p(ws) + 4), 64, s),
    ]
    assert all(rc != 0 for rc in refused), refused
    assert b"workspace" in l.vsx_last_error() or b"aligned" in l.vsx_last_error()
    torch.cuda.synchronize()
    assert (out32 == 5.0).all() and (out64 == 5.0).all()
    with pytest.raises(ValueError):
        ops.pair_dist(x, idx, idx, "cityblock")
    assert ops.pair_dist(x, idx[:0], idx[:0]).shape == (0,)


# ------------------------------------------------------------------------------------------------ end to end
TEN_KEYS = ["adjacent_frame_mean", "adjacent_frame_std", "adjacent_frame_median", "adjacent_frame_peak", "random_frame_mean",
            "random_frame_std", "random_frame_median", "random_frame_peak", "smoothness_score", "dynamic_range"]


@functools.lru_cache(maxsize=None)
def run_case(name):
    from viscy_amd import smoothness as S

    ad, metric, offsets = RS.adata(name)
    state = np.random.get_state()
    res = S.compute_embeddings_smoothness(ad, distance_metric=metric, time_offsets=offsets)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    return res


@pytest.mark.parametrize("name", RUNNING)
def test_smoothness_end_to_end(name):
    x, obs, metric, offsets, z, pi, pj, ri, rj = reference_rows(name)
    g = golden()["cases"][name]
    stats, dist, piecewise = run_case(name)
    assert list(stats) == TEN_KEYS == list(g["stats"]) and all(type(v) is float for v in stats.values())
    assert list(dist) == ["adjacent_frame_distribution", "random_frame_distribution"]
    tol = {"adjacent": RS.pair_tolerance(z, pi, pj, metric), "random": RS.pair_tolerance(z, ri, rj, metric)}
    for key in ("adjacent", "random"):
        got = dist[key + "_frame_distribution"]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(pi),)
        E = tol[key]
        for (mine, want), e in zip(recorded(g, key, got), recorded(g, key, E)):
            err = np.abs(mine - want)
            print(name, key, "max err / E_p", float((err / e[0]).max()))
            assert (err <= e[0]).all(), (name, key, float(err.max()))
        for stat, fn in (("mean", np.mean), ("std", np.std), ("median", np.median)):
            k = f"{key}_frame_{stat}"
            assert stats[k] == float(fn(got))
            assert abs(stats[k] - g["stats"][k]) <= E.max(), (name, k, stats[k], g["stats"][k])
        step = (got.max() - got.min()) / (RS.GRID - 1)
        peak_err = abs(stats[key + "_frame_peak"] - g["stats"][key + "_frame_peak"])
        print(name, key, "peak err / grid step", float(peak_err / step))
        assert peak_err <= step, (name, key, stats[key + "_frame_peak"], g["stats"][key + "_frame_peak"])
    assert stats["smoothness_score"] == stats["adjacent_frame_mean"] / stats["random_frame_mean"]
    assert stats["dynamic_range"] == stats["random_frame_peak"] - stats["adjacent_frame_peak"]
    # the piecewise lists: the reference's structure, and the offset-1 distances of the adjacent distribution
    assert [len(p) for p in piecewise] == g["piecewise_lengths"]
    assert all(type(v) is float for p in piecewise for v in p)
    _, _, pieces = RS.adjacent_pairs_loop(obs["fov_name"], obs["track_id"], offsets)
    assert piecewise == [dist["adjacent_frame_distribution"][p].tolist() for p in pieces]
    if "piecewise" in g:
        for mine, want, idx in zip(piecewise, g["piecewise"], pieces):
            assert (np.abs(np.array(mine) - np.array(want)) <= tol["adjacent"][idx]).all()


def test_smoothness_inputs_and_exceptions():
    from viscy_amd import smoothness as S

    stats, dist, piecewise = run_case("A")
    ad, metric, offsets = RS.adata("A", frame=True)
    ad.X = torch.from_numpy(ad.X).to(DEV)
    before = ad.X.clone()
    stats2, dist2, piecewise2 = S.compute_embeddings_smoothness(ad)          # the defaults are A's: cosine, [1]
    assert torch.equal(ad.X, before)
    assert stats2 == stats and piecewise2 == piecewise
    assert all(np.array_equal(dist[k], dist2[k]) for k in dist)
    err = golden()["cases"]["F"]["error"]
    ad, metric, offsets = RS.adata("F")
    with pytest.raises(ValueError) as e:
        S.compute_embeddings_smoothness(ad, distance_metric=metric, time_offsets=offsets)
    assert err[0] == "ValueError" and str(e.value) == err[1]
    with pytest.raises(ValueError):
        S.compute_embeddings_smoothness(RS.adata("A")[0], distance_metric="cityblock")


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_track_displacement(metric):
    from viscy_amd import smoothness as S

    ds = RS.msd_dataset()
    got = S.compute_track_displacement(ds, distance_metric=metric)
    rec = golden()["msd"][metric]
    assert list(got) == [tau for tau, _ in rec] and all(type(k) is int for k in got)
    bound = RS.pair_bound(ds["features"].shape[1])
    ones = 0
    for tau, want in rec:
        mine = got[tau]
        assert type(mine) is list and len(mine) == len(want) and all(type(v) is float for v in mine)
        err = np.abs(np.array(mine) - np.array(want))
        lim = bound * (np.abs(np.array(want)) if metric == "euclidean" else 1.0)
        assert (err <= lim).all(), (tau, float(err.max()))
        ones += sum(v == 1.0 for v in mine)
    if metric == "cosine":
        assert ones == 6          # the all-zero row of its 7-row track: distance exactly 1 to each of the other six
    # a device tensor, and chunked calls, give the same dict
    ds_dev = dict(ds, features=torch.from_numpy(ds["features"]).to(DEV))
    assert S.compute_track_displacement(ds_dev, distance_metric=metric) == got
    old, S.MSD_CHUNK = S.MSD_CHUNK, 7
    try:
        assert S.compute_track_displacement(ds, distance_metric=metric) == got
        assert list(S.compute_track_displacement(ds, distance_metric=metric)) == list(got)
    finally:
        S.MSD_CHUNK = old
    with pytest.raises(ValueError):
        S.compute_track_displacement(ds, distance_metric="cityblock")
