"""Exact fixtures for the kernels of csrc/f32_tile.h past one column tile per workgroup (csrc/mmd.hip, csrc/online_eval.hip).

Dispatch arithmetic, restated: ``even_split`` (ft_even_split), ``mmd_plan`` (mm_split: the MMD's column split, a function of N
alone) and ``knn_plan`` (kt_splits + ft_even_split: the probe's, a function of N and the compute-unit count).  mm_split gives
every workgroup ONE column tile up to N = 2944 (23 tiles, 512 / 23 > 22 wanted workgroups per row tile), so the accumulation into
the workspace row, the second ``first()`` (``nc`` rewritten between tiles), the kernel tile's place handed back to the staging
area, the refetch of the row labels and a shorter last split only run from N = 2945 on.  The cases below sit there.

The cluster pool.  Rows are points of {-3 .. 3}^d: C / 2 distinct non-zero points and their negations, p and -p with the same
number of rows, one all-zero row for an odd N, permuted so that every tile mixes clusters.  With ``norms`` the integer squared
norms and bandwidth 2^-9 (2 bw = 2^-8) every step of mmd_d2 is exact integer arithmetic: d2 = 0 inside a cluster, an integer
>= 1 across clusters, the exponent is -256 d2, and a kernel value is expf(-0) = 1 or expf(<= -256) = +0:

    K_ij = [cluster_i == cluster_j] [i != j]

The sums of a label vector z follow in integers (m_c ones in cluster c of n_c rows):

    quad = sum m_c^2 - sum m_c      zr = sum m_c n_c - sum m_c      T = sum n_c^2 - N
    sums = {quad, (T - 2 zr) + quad, zr - quad}

all below 2^24; the kernel's fp32 partial of a 128-term tile row is at most 128 and everything after it is float64, so
ops.mmd_sums equals ``closed_form`` bit for bit.  A stale ``nc``, a tile skipped or taken twice, a label tile of the wrong columns
or ``=`` for ``+`` in the workspace row each move an integer (``stream_model`` and its mutants show it on the CPU).

Importable without a GPU; nothing here touches a device."""

import functools

import numpy as np

from tests import ref_mmd as RM

T = 128                  # FT_T
MM_WANT_WGS = 512
MM_MAX_SPLITS = 32
KT_MAX_SPLITS = 8
BANDWIDTH = 2.0 ** -9    # 2 bw = 2^-8: the exponent is -256 d2
LIMIT = 2 ** 24


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ 1. dispatch arithmetic
def even_split(tiles, want):
    """ft_even_split -> (splits, tiles_per_split): ``want`` clamped to 1 .. tiles, equal runs, no empty split"""
    s = min(max(int(want), 1), tiles)
    tps = cdiv(tiles, s)
    return cdiv(tiles, tps), tps


def mmd_plan(N):
    """mm_split -> (tiles, splits, tiles_per_split, tiles of the last split)"""
    tiles = cdiv(N, T)
    splits, tps = even_split(tiles, min(cdiv(MM_WANT_WGS, tiles), MM_MAX_SPLITS))
    return tiles, splits, tps, tiles - (splits - 1) * tps


def knn_plan(N, cus):
    """kt_splits + ft_even_split -> (tiles, splits, tiles_per_split, tiles of the last split).  The split count in 1 .. 8 that
    leaves the fewest idle workgroup slots (two per compute unit) in the last round; a larger count must be better by more than
    1.02 x, and a count whose last split would be empty is not a candidate"""
    tiles = cdiv(N, T)
    slots = 2 * (cus if cus > 0 else 256)
    best, best_eff = 1, 0.0
    for s in range(1, min(KT_MAX_SPLITS, tiles) + 1):
        n, _ = even_split(tiles, s)
        if n != s:
            continue
        wgs = tiles * s
        eff = wgs / (cdiv(wgs, slots) * slots)
        if eff > best_eff * 1.02:
            best, best_eff = s, eff
    splits, tps = even_split(tiles, best)
    return tiles, splits, tps, tiles - (splits - 1) * tps


def split_of(plan, tile):
    """(split, position inside the split) of column tile ``tile``"""
    return tile // plan[2], tile % plan[2]


# ------------------------------------------------------------------------------------------------ 2. the cluster pool
CLUSTERS = 16   # 8 rows of a cluster per 128-row tile on average: every pair of full tiles shares clusters (asserted per case)


@functools.lru_cache(maxsize=None)
def cluster_pool(N, d, C=CLUSTERS, seed=0):
    """-> (x float32 (N, d), cluster id int64 (N,)); never written to.  Cluster ids 2q / 2q + 1 are point q and its negation, id C
    the all-zero row of an odd N.  Where N leaves a tail tile, its last two rows are rows of cluster 0 (one of the most
    populous), so that the tail tile holds a pair of its own; the rows that stood there take the places those two came from"""
    assert C % 2 == 0 and N >= 2 * C
    rng = np.random.RandomState(seed)
    pts, seen = [], set()
    while len(pts) < C // 2:
        p = tuple(int(v) for v in rng.randint(-3, 4, d))
        if any(p) and p not in seen:
            seen.update((p, tuple(-v for v in p)))
            pts.append(p)
    pts = np.asarray(pts, dtype=np.int64)
    pairs = N // 2                                        # rows of p and of -p each, over all points
    per = np.full(C // 2, pairs // (C // 2)) + (np.arange(C // 2) < pairs % (C // 2))
    cid = np.concatenate([np.repeat(np.arange(0, C, 2), per), np.repeat(np.arange(1, C, 2), per), np.full(N % 2, C)])
    cid = cid[rng.permutation(N)]
    if N % T:
        want = [N - 2, N - 1]
        have = [i for i in np.nonzero(cid == 0)[0] if i < N - 2][:2]
        for a, b in zip(want, have):
            if cid[a] != 0:
                cid[a], cid[b] = cid[b], cid[a]
    points = np.concatenate([np.stack([pts, -pts], 1).reshape(C, d), np.zeros((1, d), dtype=np.int64)])
    x = np.ascontiguousarray(points[cid].astype(np.float32))
    for a in (x, cid):
        a.setflags(write=False)
    return x, cid


def integer_norms(x):
    n = (x.astype(np.int64) ** 2).sum(1)
    return n.astype(np.float32)


def indicator(cid, rows=None, cols=None):
    """the expected kernel rectangle, float32: 1 where the clusters agree off the diagonal"""
    N = len(cid)
    r0, r1 = rows or (0, N)
    c0, c1 = cols or (0, N)
    i, j = np.arange(r0, r1), np.arange(c0, c1)
    return ((cid[i][:, None] == cid[j][None, :]) & (i[:, None] != j[None, :])).astype(np.float32)


def labels_for(N, P, seed=5):
    """uint8 (P, N): the observed split and permutations of it (tests/ref_mmd.permutation_labels), then an all-zero and an all-one
    row; P = 1 is the observed split alone.  The first rows are the same for every P"""
    base = _label_base(N, seed)
    if P < 3:
        return np.ascontiguousarray(base[:P])
    return np.concatenate([base[:P - 2], np.zeros((1, N), np.uint8), np.ones((1, N), np.uint8)])


@functools.lru_cache(maxsize=None)
def _label_base(N, seed):
    z = RM.permutation_labels(N // 2, N - N // 2, 297, seed)
    z.setflags(write=False)
    return z


def closed_form(cid, z):
    """float64 (P, 3) {sum_XX, sum_YY, sum_XY} of the indicator kernel under the label rows z, from cluster counts alone"""
    ncl = int(cid.max()) + 1
    n_c = np.bincount(cid, minlength=ncl).astype(np.int64)
    onehot = np.zeros((len(cid), ncl), dtype=np.int64)
    onehot[np.arange(len(cid)), cid] = 1
    m = z.astype(np.int64) @ onehot                       # (P, clusters)
    quad = (m * m).sum(1) - m.sum(1)
    zr = (m * n_c[None, :]).sum(1) - m.sum(1)
    Tt = int((n_c * n_c).sum()) - len(cid)
    assert Tt < LIMIT and 0 <= quad.min() and quad.max() <= Tt and zr.max() <= Tt
    return np.stack([quad, (Tt - 2 * zr) + quad, zr - quad], axis=1).astype(np.float64)


P_EDGES = (1, 127, 128, 129, 300)   # P + 1 = 128: the virtual ones-row ends the first label chunk; 129: alone in the second

# name, N, d, unaligned views, leg.  The leg quotes mmd_plan(N) as "T tiles = S splits x R" and the last split's length
MMD_CASES = [
    dict(name="n130_d3", N=130, d=3, views=False,
         leg="2 tiles = 2 splits x 1, last 1: one tile per workgroup; d % 4 != 0: scalar row loads; N % 16 != 0: byte label loads; "
             "the baseline of the P edges"),
    dict(name="n3072_d4", N=3072, d=4, views=False,
         leg="24 tiles = 12 splits x 2, last 2: every workgroup accumulates a second tile; N % 16 == 0: 16-byte label loads; "
             "d % 4 == 0: float4 row loads"),
    dict(name="n3075_d5", N=3075, d=5, views=False,
         leg="25 tiles = 13 splits x 2, last 1: a shorter last split; byte label loads; scalar row loads; 3-row tail tile"),
    dict(name="n4100_d36", N=4100, d=36, views=False,
         leg="33 tiles = 11 splits x 3, last 3: three tiles per workgroup; two feature chunks (32 + 4); float4 row loads, "
             "byte label loads"),
    dict(name="n3072_d4_views", N=3072, d=4, views=True,
         leg="24 tiles = 12 splits x 2, last 2: the rows 4 bytes and the labels 1 byte off the 16-byte grid, so d % 4 == 0 takes "
             "scalar row loads and N % 16 == 0 byte label loads; bit-equal to the aligned run"),
]
INVISIBLE_N, INVISIBLE_D, INVISIBLE_P = 1100, 16, 40   # the shape of ref_mmd's largest case: 9 tiles = 9 splits x 1


def mmd_case(name):
    return next(c for c in MMD_CASES if c["name"] == name)


def plan_leg(N):
    tiles, splits, tps, last = mmd_plan(N)
    return f"{tiles} tiles = {splits} splits x {tps}, last {last}"


def rectangles(N):
    """three (rows, cols) rectangles of the kernel matrix, each starting inside a tile: columns inside the second tile of a
    split, columns over the last split (the short one, if there is one), columns across the tail.  With one tile per split the
    'second tile of a split' is the last tile of the first row of tiles that has one"""
    tiles, splits, tps, last = mmd_plan(N)
    second = (min(1, tiles - 1)) * T if tps == 1 else ((splits // 2) * tps + 1) * T
    lo = (splits - 1) * tps * T
    r = lambda a, b: (max(a, 0), min(b, N))  # noqa: E731
    return [(r(3, 131), r(min(second + 5, N - 2), second + 120)),
            (r(N - 200, N - 70), r(lo - 3, lo + last * T)),
            (r(N - 131, N), r(N - 140, N))]


# ------------------------------------------------------------------------------------------------ the probe's cases
# (N, d, k, groups, inv) rows for EXACT of tests/test_gpu_online_eval.py, one per KB instance of knn_topk_kernel with at least two
# candidate tiles per workgroup: cnt / thr_s / thr_j carried in registers and the sorted lists kept in LDS across tiles.  The leg
# quotes knn_plan(N, 256) in the same words as above; the GPU test evaluates it with the device's own compute-unit count
KNN_CASES = [
    dict(case=(1153, 3, 7, "folds", "ones"), leg="10 tiles = 5 splits x 2, last 2: KB 8; d % 4 != 0: scalar row loads"),
    dict(case=(1030, 4, 20, "folds", "pow2"), leg="9 tiles = 5 splits x 2, last 1: KB 24; a shorter last split"),
    dict(case=(2171, 33, 64, "folds", "pow2"), leg="17 tiles = 6 splits x 3, last 2: KB 64; three tiles per split; chunk + 1 feature"),
    dict(case=(1030, 4, 20, "few", "pow2"), leg="9 tiles = 5 splits x 2, last 1: KB 24; cnt < k carried across tiles"),
]
KNN_VIEW_CASE = (1030, 4, 20, "folds", "pow2")   # run once more with x 4 bytes off the 16-byte grid: d % 4 == 0 on scalar loads
KNN_ORDER_CASE = (1030, 36, 64)                  # float rows, probe against head: one summation order over two tiles per workgroup


def knn_leg(N, cus):
    tiles, splits, tps, last = knn_plan(N, cus)
    return f"{tiles} tiles = {splits} splits x {tps}, last {last}"


# ------------------------------------------------------------------------------------------------ 3. a model of the stream
MUTATIONS = ("overwrite_instead_of_accumulate", "stale_nc", "label_tile_of_ct0", "last_split_dropped")


def stream_model(x, norms, z, mutation=None):
    """float64 (P, 3): the streaming sums as mmd_sums_kernel + mmd_fold_kernel form them, tile by tile, in plain numpy.  Per row
    tile and split: the fp32 kernel tile from mmd_d2 / expf, times the label tile of the same columns, weighted with the row
    labels, into the workgroup's workspace row; then the fold over workgroups.  It shares no code with ``closed_form``.

    mutation: one of MUTATIONS, each a mistake that cannot show with one tile per split —
      overwrite_instead_of_accumulate   ``*dst = v`` for every tile of the split
      stale_nc                          the second and later tiles of a split keep the previous tile's column norms
      label_tile_of_ct0                 the second and later tiles multiply with the label tile of the split's first tile
      last_split_dropped                where a split holds two or more tiles, the last split's workgroups never run"""
    assert mutation is None or mutation in MUTATIONS
    N, P = len(x), len(z)
    tiles, splits, tps, _ = mmd_plan(N)
    pad = tiles * T
    xp = np.zeros((pad, x.shape[1]), dtype=np.float32)
    xp[:N] = x
    npad = np.zeros(pad, dtype=np.float32)
    npad[:N] = norms
    zp = np.zeros((P + 1, pad), dtype=np.float32)           # row P: the virtual row of ones
    zp[:P, :N] = z
    zp[P, :N] = 1.0
    valid = np.arange(pad) < N
    two_bw = np.float32(2.0 * BANDWIDTH)
    ws = np.zeros((splits, tiles, 2, P + 1), dtype=np.float64)
    run_splits = splits - 1 if mutation == "last_split_dropped" and tps >= 2 else splits
    for rt in range(tiles):
        q = slice(rt * T, (rt + 1) * T)
        for s in range(run_splits):
            ct0, ct1 = s * tps, min((s + 1) * tps, tiles)
            for ct in range(ct0, ct1):
                c = slice(ct * T, (ct + 1) * T)
                nc = npad[c]
                if mutation == "stale_nc" and ct > ct0:
                    nc = npad[(ct - 1) * T:ct * T]
                dot = xp[q] @ xp[c].T                                                                   # exact: small integers
                d2 = np.maximum((npad[q][:, None] + nc[None, :]) - np.float32(2.0) * dot, np.float32(0.0))
                with np.errstate(under="ignore"):
                    k = np.exp(-(d2 / two_bw)).astype(np.float32)
                ok = valid[q][:, None] & valid[c][None, :] & (np.arange(rt * T, (rt + 1) * T)[:, None] != np.arange(ct * T, (ct + 1) * T)[None, :])
                k = np.where(ok, k, np.float32(0.0))
                lab = zp[:, (ct0 * T if mutation == "label_tile_of_ct0" else ct * T):][:, :T]
                s2 = (k @ lab.T).astype(np.float64)                                                      # (rows, P + 1); fp32, exact here
                v = np.stack([(s2 * zp[:, q].T).sum(0), s2.sum(0)])
                if ct == ct0 or mutation == "overwrite_instead_of_accumulate":
                    ws[s, rt] = v
                else:
                    ws[s, rt] += v
    quad, zr, Tt = np.zeros(P), np.zeros(P), 0.0
    for w in ws.reshape(-1, 2, P + 1):                     # mmd_fold_kernel: ascending workgroup order
        quad += w[0, :P]
        zr += w[1, :P]
        Tt += w[1, P]
    return np.stack([quad, (Tt - 2.0 * zr) + quad, zr - quad], axis=1)
