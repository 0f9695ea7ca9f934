"""The case table of the OnlineEvalCallback tests and a float64 numpy restatement of the kernels' contract
(csrc/online_eval.hip): the candidate rule, the total order (similarity descending, row index ascending) and the vote (most
frequent label, ties to the smallest).  Inputs are rebuilt from seeds; tests/golden/online_eval.pt (tools/gen_golden_online_eval.py)
holds what sklearn / scipy / the reference give on them."""

import functools

import numpy as np

# name: N rows, d features, C classes, k, mode, latent rank (None: full rank d), noise (class centres are unit normal in the
# latent space), seed; "sizes": explicit class sizes instead of a random assignment
KNN_CASES = {
    "n257_d48_cv": dict(N=257, d=48, C=5, k=20, mode="cv", rank=8, noise=1.5, seed=11),
    "n130_d33_cv": dict(N=130, d=33, C=3, k=7, mode="cv", rank=6, noise=1.5, seed=12),
    "n515_d768_cv_noise1.5": dict(N=515, d=768, C=12, k=20, mode="cv", rank=16, noise=1.5, seed=13),
    "n515_d768_cv_noise2.5": dict(N=515, d=768, C=12, k=20, mode="cv", rank=16, noise=2.5, seed=13),
    "n515_d768_holdout": dict(N=515, d=768, C=12, k=20, mode="holdout", rank=16, noise=1.5, seed=14),
    "n1030_d64_holdout": dict(N=1030, d=64, C=40, k=20, mode="holdout", rank=16, noise=1.5, seed=15),
    "n131_d32_cv_3folds": dict(N=131, d=32, C=4, k=7, mode="cv", rank=8, noise=1.5, seed=16, sizes=(60, 3, 40, 28)),
}
HOLDOUT_TEST_SIZE = 0.2
ERANK_CASES = ("n257_d48_cv", "n130_d33_cv", "n515_d768_cv_noise1.5")  # the feature matrices the effective rank is checked on


@functools.lru_cache(maxsize=None)
def build_knn(name):
    """-> (features float32 (N, d), labels int64 (N,)); never written to"""
    c = KNN_CASES[name]
    rng = np.random.RandomState(c["seed"])
    N, d, C, r = c["N"], c["d"], c["C"], c["rank"] or c["d"]
    if "sizes" in c:
        labels = np.repeat(np.arange(C), c["sizes"])
    else:
        labels = np.concatenate((np.arange(C), rng.randint(0, C, N - C)))  # every class present
    labels = labels[rng.permutation(N)]
    centres = rng.randn(C, r)
    latent = centres[labels] + c["noise"] * rng.randn(N, r)
    x = latent if c["rank"] is None else latent @ (rng.randn(r, d) / np.sqrt(r))
    x = np.ascontiguousarray(x.astype(np.float32))
    x.setflags(write=False)
    labels.setflags(write=False)
    return x, labels.astype(np.int64)


# ------------------------------------------------------------------------------------------------ temporal smoothness fixtures
SMOOTH_CASES = {
    "tracks40": dict(tracks=40, lo=2, hi=12, singletons=9, d=32, noise=2.0, seed=21),
    "two_pairs": dict(tracks=2, lo=2, hi=2, singletons=5, d=8, noise=0.35, seed=22),
}


@functools.lru_cache(maxsize=None)
def build_smooth(name):
    """-> (features float32 (N, d), track_ids int64, timepoints int64), rows of all tracks interleaved: a track is a point that
    moves along a smooth curve (a random rotation plane) with t, plus noise"""
    c = SMOOTH_CASES[name]
    rng = np.random.RandomState(c["seed"])
    feats, tids, ts = [], [], []
    lens = list(rng.randint(c["lo"], c["hi"] + 1, c["tracks"])) + [1] * c["singletons"]
    for tid, n in enumerate(lens):
        centre, u, v = rng.randn(c["d"]), rng.randn(c["d"]), rng.randn(c["d"])
        t0, omega = rng.randint(0, 30), 0.15 + 0.1 * rng.rand()
        for s in range(n):
            t = t0 + s
            feats.append(centre + 1.5 * (np.cos(omega * t) * u + np.sin(omega * t) * v) + c["noise"] * rng.randn(c["d"]))
            tids.append(100 + 7 * tid)
            ts.append(t)
    perm = rng.permutation(len(tids))
    x = np.ascontiguousarray(np.asarray(feats, dtype=np.float32)[perm])
    tids, ts = np.asarray(tids, dtype=np.int64)[perm], np.asarray(ts, dtype=np.int64)[perm]
    for a in (x, tids, ts):
        a.setflags(write=False)
    return x, tids, ts


def track_pairs_loop(track_ids):
    """the pair order of the reference's loops (online_eval.py:104-117), literally"""
    pi, pj = [], []
    for tid in np.unique(track_ids):
        rows = np.nonzero(track_ids == tid)[0]
        for a in range(len(rows)):
            for b in range(a + 1, len(rows)):
                pi.append(rows[a])
                pj.append(rows[b])
    return np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the kernels' contract
def inv_norm(x, eps=0.0):
    """1 / (||x_i|| + eps) in float64; 0 where the denominator is 0"""
    den = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(1)) + eps
    return np.where(den == 0, 0.0, 1.0 / np.where(den == 0, 1.0, den))


def similarity(x, inv, exact32=False):
    """s_ij = (dot_ij * inv_i) * inv_j.  exact32: the dot products are exact integers below 2^24 and both products are rounded to
    fp32 as the kernel rounds them, so the result is bit for bit the kernel's; otherwise plain float64"""
    x64 = np.asarray(x, dtype=np.float64)
    dot = x64 @ x64.T
    if exact32:
        assert np.abs(dot).max() < 2 ** 24 and (dot == np.round(dot)).all()
        i32 = np.asarray(inv, dtype=np.float32)
        return (dot.astype(np.float32) * i32[:, None]) * i32[None, :]
    i64 = np.asarray(inv, dtype=np.float64)
    return (dot * i64[:, None]) * i64[None, :]


def knn_topk(s, group, k):
    """-> idx (N, k) int32, sim (N, k) of s's dtype, cnt (N,) int32 — candidates of row i: group[j] >= 0 and group[j] != group[i];
    order: s descending, j ascending; unused slots -1 / -inf.  Also the similarity of candidate k + 1 (-inf if there is none)."""
    group = np.asarray(group)
    N = s.shape[0]
    idx = np.full((N, k), -1, dtype=np.int32)
    sim = np.full((N, k), -np.inf, dtype=s.dtype)
    cnt = np.zeros(N, dtype=np.int32)
    nxt = np.full(N, -np.inf, dtype=np.float64)
    for i in range(N):
        cand = np.nonzero((group >= 0) & (group != group[i]))[0]
        order = cand[np.lexsort((cand, -s[i, cand]))]
        m = min(k, len(order))
        idx[i, :m], sim[i, :m], cnt[i] = order[:m], s[i, order[:m]], m
        if len(order) > k:
            nxt[i] = s[i, order[k]]
    return idx, sim, cnt, nxt


def knn_vote(idx, cnt, labels):
    """-> (pred, margin): the most frequent label of the first cnt neighbours, ties to the smallest label, -1 for cnt = 0; the
    top count minus the runner-up's (another label's) count"""
    labels = np.asarray(labels)
    pred = np.full(len(cnt), -1, dtype=np.int32)
    margin = np.zeros(len(cnt), dtype=np.int64)
    for i in range(len(cnt)):
        if cnt[i] == 0:
            continue
        vals, counts = np.unique(labels[idx[i, : cnt[i]]], return_counts=True)  # vals ascending: argmax takes the smallest on a tie
        top = int(np.argmax(counts))
        pred[i] = vals[top]
        margin[i] = counts[top] - (np.delete(counts, top).max() if len(counts) > 1 else 0)
    return pred, margin


def undecided(x, labels, group, k):
    """-> (pred, mask) of the float64 restatement.  A row is undecided if the gap between its k-th and (k+1)-th candidate
    similarity is below tau = d 2^-23 (the sum of the worst-case fp32 rounding of two unit-vector dot products, the kernel's and
    sklearn's) AND its vote margin is below 3 (one swapped neighbour moves the margin by at most 2)."""
    x = np.asarray(x)
    s = similarity(x, inv_norm(x, 0.0))
    idx, sim, cnt, nxt = knn_topk(s, group, k)
    pred, margin = knn_vote(idx, cnt, labels)
    kth = np.where(cnt == k, sim[:, k - 1], np.inf)
    tau = x.shape[1] * 2.0 ** -23
    return pred, ((kth - nxt) < tau) & (margin < 3)


# ------------------------------------------------------------------------------------------------ exact fixtures (integer rows)
def integer_rows(N, d, seed, lo=-3, hi=3, dup=0.75):
    """integer-valued float32 rows with many exact duplicates (ties in s broken by index only); |dot| <= 9 d < 2^24"""
    rng = np.random.RandomState(seed)
    base = rng.randint(lo, hi + 1, (max(2, N // 8), d))
    x = np.where(rng.rand(N, 1) < dup, base[rng.randint(0, len(base), N)], rng.randint(lo, hi + 1, (N, d)))
    return np.ascontiguousarray(x.astype(np.float32))
