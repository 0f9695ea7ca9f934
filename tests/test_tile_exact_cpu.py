"""CPU: the exact fixtures of tests/ref_exact_tile.py without a GPU.

1. the restated dispatch arithmetic equals the library's (vsx_mmd_sums_ws_bytes is tiles * splits * 2 (P + 1) * 8 and loads
   without a device), and every case's ``leg`` quotes the plan that the arithmetic gives: the cases reach two and three tiles per
   workgroup, an even and a shorter last split, and nothing below N = 2945 does;
2. the cluster pools keep what exactness rests on: integer bounds, column sums exactly 0, d2 >= 1 across clusters, at least one
   1 in every (row tile, column tile) pair, the tail tile included;
3. the closed form equals tests/ref_mmd.sums of the indicator matrix, and a numpy model of the stream (tile by tile, fp32 kernel
   values, workspace rows, fold) equals the closed form;
4. sensitivity: four mistakes of the multi-tile loop each move an integer on every case with two or more tiles per split, and
   none of them is visible at N = 1100, the largest N of the tolerance tests;
5. the probe's new cases carry their lists across tiles: neighbour lists hold rows of the first and of a later tile of one split."""

import numpy as np
import pytest

from tests import ref_exact_tile as X
from tests import ref_mmd as RM

MULTI = [c for c in X.MMD_CASES if X.mmd_plan(c["N"])[2] >= 2 and not c["views"]]
MODEL_P = 12   # label rows of the CPU model: the observed split, nine permutations, zeros, ones


def _pool(c):
    x, cid = X.cluster_pool(c["N"], c["d"])
    return x, cid, X.integer_norms(x)


# ------------------------------------------------------------------------------------------------ 1. dispatch arithmetic
def test_plans_are_the_ones_the_cases_were_chosen_for():
    assert X.even_split(24, 22) == (12, 2) and X.even_split(9, 64) == (9, 1) and X.even_split(5, 0) == (1, 5)
    assert X.mmd_plan(3072) == (24, 12, 2, 2) and X.mmd_plan(3075) == (25, 13, 2, 1) and X.mmd_plan(4100) == (33, 11, 3, 3)
    assert X.mmd_plan(130) == (2, 2, 1, 1) and X.mmd_plan(1100) == (9, 9, 1, 1) and X.mmd_plan(20000) == (157, 4, 40, 37)
    assert X.knn_plan(1030, 256) == (9, 5, 2, 1) and X.knn_plan(1153, 256) == (10, 5, 2, 2) and X.knn_plan(2171, 256) == (17, 6, 3, 2)
    assert X.knn_plan(385, 256) == (4, 4, 1, 1)                       # the largest N of the bit-exact table before these cases
    # one column tile per workgroup up to 23 tiles, two from 24 on: no N <= 2944 reaches the accumulation
    assert all(X.mmd_plan(N)[2] == 1 for N in range(2, 2945)) and X.mmd_plan(2945)[2] == 2
    # the empty-split skip of kt_splits: 9 tiles cannot be cut in 6, 7 or 8 runs.  4 slots: 3 splits fill 27 of 28, 5 only 45 of 48
    assert [X.even_split(9, s)[0] for s in (5, 6, 7, 8)] == [5, 5, 5, 5]
    assert X.knn_plan(1030, 2) == (9, 3, 3, 3)
    # the 1.02 rule: with 10 tiles and 10 slots every count fills its last round, and the first one stays
    assert X.knn_plan(1153, 5) == (10, 1, 10, 10)


def test_mmd_plan_is_the_librarys():
    from viscy_amd import _lib

    L = _lib.lib()
    for N in sorted(set(range(2, 6001, 61)) | {c["N"] for c in X.MMD_CASES} | {X.INVISIBLE_N, 2944, 2945, 20000}):
        tiles, splits, tps, last = X.mmd_plan(N)
        assert 1 <= last <= tps and (splits - 1) * tps + last == tiles
        for P in (1, 40, 129):
            assert L.vsx_mmd_sums_ws_bytes(N, P) == tiles * splits * 2 * (P + 1) * 8, (N, P)


def test_every_case_quotes_its_plan():
    assert len({c["name"] for c in X.MMD_CASES}) == len(X.MMD_CASES)
    for c in X.MMD_CASES:
        assert c["leg"].startswith(X.plan_leg(c["N"])), (c["name"], X.plan_leg(c["N"]))
    for c in X.KNN_CASES:
        assert c["leg"].startswith(X.knn_leg(c["case"][0], 256)), (c["case"], X.knn_leg(c["case"][0], 256))
        assert X.knn_plan(c["case"][0], 256)[2] >= 2
    assert {(8 if k <= 8 else 24 if k <= 24 else 64) for _, _, k, _, _ in (c["case"] for c in X.KNN_CASES)} == {8, 24, 64}
    assert X.knn_plan(X.KNN_ORDER_CASE[0], 256)[2] >= 2 and X.KNN_VIEW_CASE[1] % 4 == 0
    # what the MMD cases claim besides the plan
    by = {c["name"]: c for c in X.MMD_CASES}
    assert by["n3072_d4"]["N"] % 16 == 0 and by["n3072_d4"]["d"] % 4 == 0
    assert by["n3075_d5"]["N"] % 128 == 3 and by["n3075_d5"]["d"] % 4 != 0 and X.mmd_plan(3075)[3] < X.mmd_plan(3075)[2]
    assert by["n4100_d36"]["d"] == 32 + 4 and X.mmd_plan(4100)[2] == 3
    assert by["n3072_d4_views"]["views"] and (by["n3072_d4_views"]["N"], by["n3072_d4_views"]["d"]) == (3072, 4)
    assert 128 in [P + 1 for P in X.P_EDGES] and 129 in [P + 1 for P in X.P_EDGES]


def test_the_new_cases_are_in_the_gpu_tables():
    from tests import test_gpu_mmd as GM
    from tests import test_gpu_online_eval as GO

    for c in X.KNN_CASES:
        assert c["case"] in GO.EXACT
    assert "n3075_d12" in GM.POOLS
    tiles, splits, tps, last = X.mmd_plan(3075)
    where = {X.split_of((tiles, splits, tps, last), j // X.T) + (j // X.T,) for _, j in GM._pairs(3075)}
    assert any(pos >= 1 for _, pos, _ in where)                                  # the second tile of a split
    assert any(s == splits - 1 for s, _, _ in where) and last < tps               # the short last split, which is the tail tile
    assert len({s for s, _, _ in where}) >= 3
    assert all((i, j) in GM._pairs(N) for N in (272, 357) for i, j in [(0, 127), (127, 128), (0, N - 1), (N - 2, N - 1), (5, 133)])


# ------------------------------------------------------------------------------------------------ 2. the pools
@pytest.mark.parametrize("c", X.MMD_CASES + [dict(name="n1100_d16", N=X.INVISIBLE_N, d=X.INVISIBLE_D)], ids=lambda c: c["name"])
def test_pool_keeps_what_exactness_rests_on(c):
    x, cid, norms = _pool(c)
    N, d = c["N"], c["d"]
    assert x.dtype == np.float32 and x.shape == (N, d) and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
    assert (x.astype(np.float64).sum(0) == 0.0).all()                            # mmd_prepare's mean is exactly 0
    assert norms.max() <= 9 * d and 2 * 9 * d < X.LIMIT                          # n_i + n_j and 2 dot are exact
    xi = x.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (xi * xi).sum(1)[None, :] - 2 * (xi @ xi.T)
    same = cid[:, None] == cid[None, :]
    assert (d2[same] == 0).all() and d2[~same].min() >= 1                        # exponent 0 or <= -256
    assert np.float32(np.exp(np.float32(-256.0))) == 0.0 and np.exp(np.float32(-0.0)) == 1.0
    n_c = np.bincount(cid)
    assert (n_c[0:X.CLUSTERS:2] == n_c[1:X.CLUSTERS:2]).all() and len(n_c) == X.CLUSTERS + N % 2 and (N % 2 == 0 or n_c[-1] == 1)
    # every (row tile, column tile) pair holds a 1: a tile skipped or taken twice moves T
    K = X.indicator(cid)
    tiles = X.cdiv(N, X.T)
    pad = np.zeros((tiles * X.T, tiles * X.T), dtype=np.float32)
    pad[:N, :N] = K
    per_tile = pad.reshape(tiles, X.T, tiles, X.T).sum((1, 3))
    assert per_tile.min() >= 1, np.argwhere(per_tile < 1)[:4]
    # the integers stay below 2^24 for every P of the GPU test (asserted inside closed_form), and no sum is trivially zero
    for P in X.P_EDGES:
        s = X.closed_form(cid, X.labels_for(N, P))
        assert s.shape == (P, 3) and s.max() < X.LIMIT and (s[0] > 0).all()
    z = X.labels_for(N, 300)
    assert not z[-2].any() and z[-1].all() and np.array_equal(z[:127], X.labels_for(N, 129)[:127])


def test_rectangles_lie_where_they_claim():
    for c in X.MMD_CASES:
        N = c["N"]
        plan = X.mmd_plan(N)
        tiles, splits, tps, last = plan
        (_, a), (_, b), (rc, cc) = X.rectangles(N)
        for (r0, r1), (c0, c1) in X.rectangles(N):
            assert 0 <= r0 < r1 <= N and 0 <= c0 < c1 <= N
        if tps >= 2:
            assert a[0] // X.T == (a[1] - 1) // X.T and X.split_of(plan, a[0] // X.T)[1] == 1      # inside a split's second tile
        assert X.split_of(plan, (b[1] - 1) // X.T)[0] == splits - 1 and b[1] == N and b[0] < (splits - 1) * tps * X.T
        assert rc[1] == N and cc[1] == N and rc[0] // X.T < (N - 1) // X.T                          # across the tail


# ------------------------------------------------------------------------------------------------ 3. closed form, model
@pytest.mark.parametrize("name", ["n130_d3", "n3075_d5"])
def test_closed_form_is_the_restatements_sums_of_the_indicator(name):
    c = X.mmd_case(name)
    _, cid, _ = _pool(c)
    z = X.labels_for(c["N"], MODEL_P)
    assert np.array_equal(X.closed_form(cid, z), RM.sums(X.indicator(cid).astype(np.float64), z))


@pytest.mark.parametrize("c", [c for c in X.MMD_CASES if not c["views"]], ids=lambda c: c["name"])
def test_stream_model_equals_the_closed_form(c):
    x, cid, norms = _pool(c)
    z = X.labels_for(c["N"], MODEL_P)
    assert np.array_equal(X.stream_model(x, norms, z), X.closed_form(cid, z))


# ------------------------------------------------------------------------------------------------ 4. sensitivity
@pytest.mark.parametrize("mutation", X.MUTATIONS)
@pytest.mark.parametrize("c", MULTI, ids=lambda c: c["name"])
def test_each_mutation_moves_an_integer_where_a_split_holds_two_tiles(c, mutation):
    x, cid, norms = _pool(c)
    z = X.labels_for(c["N"], MODEL_P)
    want, got = X.closed_form(cid, z), X.stream_model(x, norms, z, mutation)
    moved = want != got
    print(f"{c['name']} {mutation}: {int(moved.sum())} of {moved.size} integers move, largest by {np.abs(want - got).max():.0f}")
    assert moved.any()
    assert moved[:MODEL_P - 2].any()          # on a permutation row, not only on the all-zero / all-one rows


def test_no_mutation_is_visible_with_one_tile_per_split():
    """N = 1100 is the largest N of the tolerance tests (n600_m500_d16_p40): 9 tiles in 9 splits of 1"""
    assert len(MULTI) == 3 and X.mmd_plan(X.INVISIBLE_N)[2] == 1
    x, cid = X.cluster_pool(X.INVISIBLE_N, X.INVISIBLE_D)
    norms = X.integer_norms(x)
    z = X.labels_for(X.INVISIBLE_N, X.INVISIBLE_P)
    want = X.closed_form(cid, z)
    assert np.array_equal(X.stream_model(x, norms, z), want)
    for mutation in X.MUTATIONS:
        assert np.array_equal(X.stream_model(x, norms, z, mutation), want), mutation


# ------------------------------------------------------------------------------------------------ 5. the probe's cases
@pytest.mark.parametrize("c", X.KNN_CASES, ids=lambda c: "N%d_d%d_k%d_%s_%s" % c["case"])
def test_probe_cases_keep_their_lists_across_tiles(c):
    from tests.test_gpu_online_eval import _exact_case

    N, d, k, gkind, _ = c["case"]
    x, inv, group, idx, sim, cnt = _exact_case(*c["case"])
    plan = X.knn_plan(N, 256)
    tile = np.where(idx >= 0, idx // X.T, -1)
    split, pos = tile // plan[2], tile % plan[2]
    carried = np.zeros(N, dtype=bool)       # rows whose final list holds rows of the first AND of a later tile of one split
    for s in range(plan[1]):
        carried |= ((split == s) & (pos == 0) & (tile >= 0)).any(1) & ((split == s) & (pos >= 1) & (tile >= 0)).any(1)
    print(f"{c['case']}: {int(carried.sum())} of {N} rows keep entries of two tiles of one split; cnt < k on {int((cnt < k).sum())} rows")
    if gkind == "few":
        assert (cnt[group == 0] < k).all() and (cnt[group == 1] == k).all() and carried[group == 1].all()
    else:
        assert (cnt == k)[group >= -1].mean() > 0.99 and carried.mean() > 0.5
        full = cnt == k
        assert (sim[full, :-1] == sim[full, 1:]).mean() > 0.2                  # the GPU test's tie condition holds
