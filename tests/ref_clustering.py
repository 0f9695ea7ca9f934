"""Seeded fixtures and a numpy float64 restatement of viscy_amd.clustering, for tests/test_clustering_cpu.py,
tests/test_gpu_clustering.py and tools/gen_golden_clustering.py (which records what the reference gives on the same fixtures).

Truth.  ``sqdist_truth`` is the squared Euclidean distance in difference form, sum (x_i - x_j)^2 in float64: every difference of
two fp32 values is exact in float64 unless their exponents are more than 29 apart, so its error is the sum's, d u relative, and
it has no cancellation.  ``cosine_truth`` takes its dots and norms in long double.  The bounds are the issue's, u = 2^-53:

    squared Euclidean   2 (d + 8) u (n_i + n_j)        against sqdist_truth
    cosine              4 (d + 8) u                     against cosine_truth
    NMI                 (R C + 16) u absolute           for an R x C contingency table

Lattice features are integers with |v| <= 512: every dot is an exact float64 integer, so the kernel's squared distances are
exact and its Euclidean distances are np.sqrt of them.

Real-valued DBSCAN and k-NN fixtures carry two conditions (``eps_margin_ok``, ``knn_margin_ok``): no pair has |d2 - eps^2| under
2 (d + 8) 2^-24 (n_i + n_j), sklearn's float32 worst case, and no row's k-th and (k + 1)-th distances differ by less than the
d2 bound unless both neighbours vote alike.  A builder walks seeds 0, 1, 2, .. and takes the first that meets both."""

import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ truth and bounds
def sqnorms(x):
    x = np.asarray(x, dtype=np.float64)
    return (x * x).sum(axis=1)


def sqdist_truth(x, rows=None):
    x = np.asarray(x, dtype=np.float64)
    rows = range(len(x)) if rows is None else rows
    return np.stack([((x[i][None, :] - x) ** 2).sum(axis=1) for i in rows]) if len(x) else np.zeros((0, 0))


def sqdist_bound(x):
    n = sqnorms(x)
    return 2.0 * (x.shape[1] + 8) * U * (n[:, None] + n[None, :])


def cosine_truth(x):
    """1 - <x_i, x_j> / (max(|x_i|, 1e-12) max(|x_j|, 1e-12)), F.normalize's rule (a zero row: distance 1, also from itself)"""
    xl = np.asarray(x, dtype=np.longdouble)
    inv = 1.0 / np.maximum(np.sqrt((xl * xl).sum(axis=1)), np.longdouble(1e-12))
    return np.asarray(1.0 - (xl @ xl.T) * inv[:, None] * inv[None, :], dtype=np.float64)


def cosine_bound(x):
    return 4.0 * (x.shape[1] + 8) * U


def nmi_bound(n_true, n_pred):
    return (n_true * n_pred + 16) * U


def off_diagonal(n):
    return ~np.eye(n, dtype=bool)


# ------------------------------------------------------------------------------------------------ restatement
def pairwise_distance_matrix(x, metric):
    """the module's contract: exact zero diagonal, else the truth"""
    out = cosine_truth(x) if metric == "cosine" else np.sqrt(sqdist_truth(x))
    np.fill_diagonal(out, 0.0)
    return out


def rank_nearest_neighbors(dist, normalize=True):
    ranks = np.argsort(np.argsort(dist, axis=1, kind="stable"), axis=1, kind="stable").astype(np.int64)
    return ranks.astype(np.float64) / (ranks.shape[1] - 1) if normalize else ranks


def graph_bits(d2, eps2):
    """-> (adj uint64 (N, ceil(N / 64)), deg): bit b of word w of row i <=> j = 64 w + b < N and (i == j or d2_ij <= eps2)"""
    n = len(d2)
    near = (d2 <= eps2) | np.eye(n, dtype=bool)
    words = -(-n // 64)
    padded = np.zeros((n, words * 64), dtype=bool)
    padded[:, :n] = near
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    adj = (padded.reshape(n, words, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)
    return adj, near.sum(axis=1).astype(np.int32)


def dbscan(d2, eps2, min_samples):
    """sklearn's labelling, order-free: core = at least min_samples rows within eps (itself included); clusters = components of
    the core rows, numbered by smallest core index; a border row takes the smallest number among its core neighbours; else -1"""
    n = len(d2)
    near = (d2 <= eps2) | np.eye(n, dtype=bool)
    core = near.sum(axis=1) >= min_samples
    root = np.arange(n)
    for _ in range(n + 1):
        cand = np.where(near & core[None, :], root[None, :], n).min(axis=1)
        new = np.where(core, np.minimum(root, cand), root)
        if (new == root).all():
            break
        root = new
    roots = np.flatnonzero(core & (root == np.arange(n)))
    number = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
    number[roots] = np.arange(len(roots))
    label = np.where(core, number[root], np.where(near & core[None, :], number[root][None, :], np.iinfo(np.int64).max).min(axis=1))
    return np.where(label == np.iinfo(np.int64).max, -1, label).astype(np.int64)


def contingency(a, b):
    ca, ia = np.unique(np.asarray(a), return_inverse=True)
    cb, ib = np.unique(np.asarray(b), return_inverse=True)
    table = np.zeros((len(ca), len(cb)), dtype=np.int64)
    np.add.at(table, (ia.reshape(-1), ib.reshape(-1)), 1)
    return table


def nmi(a, b):
    """sum_ij p_ij log(p_ij / (p_i p_j)) over the arithmetic mean of the entropies, in long double, natural logarithms"""
    t = contingency(a, b).astype(np.longdouble)
    if t.shape == (1, 1):
        return 1.0
    p = t / t.sum()
    pi, pj = p.sum(axis=1), p.sum(axis=0)
    nz = p > 0
    mi = (p[nz] * np.log(p[nz] / np.outer(pi, pj)[nz])).sum()
    h = -0.5 * ((pi * np.log(pi)).sum() + (pj * np.log(pj)).sum())
    return float(max(mi, 0.0) / h) if mi > np.finfo(np.float64).eps else 0.0


def ari(a, b):
    t = contingency(a, b)
    n = int(t.sum())
    ss = sum(int(v) ** 2 for v in t.reshape(-1))
    tp, fp, fn = ss - n, sum(int(v) ** 2 for v in t.sum(axis=0)) - ss, sum(int(v) ** 2 for v in t.sum(axis=1)) - ss
    tn = n * n - fp - fn - ss
    return 1.0 if fp == 0 and fn == 0 else float(2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)))


def knn_neighbours(d2, k):
    """the k nearest of every row in the total order (d2 ascending, index ascending), the row itself included"""
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def knn_predict(d2, y, k):
    classes, codes = np.unique(np.asarray(y), return_inverse=True)
    votes = codes.reshape(-1)[knn_neighbours(d2, k)]
    counts = np.stack([(votes == c).sum(axis=1) for c in range(len(classes))], axis=1)
    return classes[np.argmax(counts, axis=1)]      # argmax: the first maximum, the smallest class


def knn_accuracy(d2, y, k):
    return float(np.mean(knn_predict(d2, y, k) == np.asarray(y)))


# ------------------------------------------------------------------------------------------------ the two fixture conditions
def eps_margin_ok(x, eps):
    d2, n = sqdist_truth(x), sqnorms(x)
    margin = 2.0 * (x.shape[1] + 8) * U32 * (n[:, None] + n[None, :])
    return not (np.abs(d2 - eps * eps) < margin)[off_diagonal(len(x))].any()


def knn_margin_ok(x, y, k):
    """no row's k-th and (k + 1)-th squared distances closer than the d2 bound, unless both neighbours vote alike"""
    d2, bound = sqdist_truth(x), sqdist_bound(x)
    if k >= len(x):
        return True
    order = np.argsort(d2, axis=1, kind="stable")
    rows = np.arange(len(x))
    a, b = order[:, k - 1], order[:, k]
    close = d2[rows, b] - d2[rows, a] < bound[rows, a] + bound[rows, b]
    y = np.asarray(y)
    return not (close & (y[a] != y[b])).any()


# ------------------------------------------------------------------------------------------------ fixtures
def real_features(n, d, seed, zero_row=None, duplicates=()):
    """float32 normal rows; ``zero_row``: an all-zero row; ``duplicates``: (i, j) pairs, row j becomes a copy of row i"""
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    if zero_row is not None and zero_row < n:
        x[zero_row] = 0.0
    for i, j in duplicates:
        if max(i, j) < n:
            x[j] = x[i]
    return x


def lattice_features(n, d, seed, span=512):
    """integers in [-span, span] as float32, span <= 512: every dot is exact in float64"""
    return np.random.RandomState(seed).randint(-span, span + 1, size=(n, d)).astype(np.float32)


# the distance cases of the golden: name -> features
def distance_case(name):
    if name == "real_30x16":
        return real_features(30, 16, 11)
    if name == "real_20x3":       # the reference's N <= 25 cdist path; a zero row and two duplicate rows
        return real_features(20, 3, 12, zero_row=4, duplicates=((2, 9), (2, 17)))
    if name == "real_130x768":
        return real_features(130, 768, 13, zero_row=77, duplicates=((5, 100),))
    if name == "lattice_50x7":
        return lattice_features(50, 7, 14)
    raise KeyError(name)


DISTANCE_CASES = ("real_30x16", "real_20x3", "real_130x768", "lattice_50x7")
RANK_CASES = ("real_30x16", "real_20x3", "lattice_50x7")


def blobs(d, seed):
    """three blobs of 45 rows around 0, e_0 and e_1 and five far singletons; -> (x float32 (140, d), blob number, 3 = singleton).
    The spread puts the rows of a blob about 0.43 apart: at eps = 0.5 nearly, at d = 16 not quite, all of a blob is one neighbourhood"""
    rs = np.random.RandomState(seed)
    sigma = 0.43 / np.sqrt(2.0 * d)
    centres = np.zeros((3, d))
    centres[1, 0] = centres[2, 1 % d] = 1.5
    if d == 1:
        centres[2, 0] = -1.5
    x = np.concatenate([c + sigma * rs.standard_normal((45, d)) for c in centres])
    far = np.zeros((5, d))
    far[np.arange(5), np.arange(5) % d] = -3.0 - np.arange(5)
    x = np.concatenate((x, far)).astype(np.float32)
    y = np.concatenate((np.repeat(np.arange(3), 45), np.full(5, 3)))
    perm = rs.permutation(len(x))
    return x[perm], y[perm]


def first_seed(build, ok, limit=200):
    for seed in range(limit):
        case = build(seed)
        if ok(case):
            return seed, case
    raise RuntimeError("no seed below %d meets the fixture conditions" % limit)


KNN_K = 5


_blob_cases = {}


def blob_case(d):
    """-> (seed, (x, y, noisy)): the first seed whose blobs meet the eps condition at the default eps = 0.5 and the k-NN condition
    at k = KNN_K under the labels ``noisy`` (y with a fifth of the rows moved to the next class); row 0 is duplicated into another
    row of its blob, both keep their label, so that the k-NN sees a distance-0 tie that votes alike.  Built once per d"""
    def build(seed):
        x, y = blobs(d, seed)
        twin = np.flatnonzero(y == y[0])[1]
        x[twin] = x[0]
        flip = np.random.RandomState(1000 + seed).rand(len(y)) < 0.2
        flip[[0, twin]] = False
        noisy = np.where(flip, (y + 1) % 4, y)
        return x, y, noisy

    if d not in _blob_cases:
        _blob_cases[d] = first_seed(build, lambda c: eps_margin_ok(c[0], 0.5) and knn_margin_ok(c[0], c[2], KNN_K))
    return _blob_cases[d]


def chain(tile):
    """3 T + 5 points on a line one eps = 1 apart: one cluster, whose smallest label has 3 T + 4 edges to travel"""
    return np.arange(3 * tile + 5, dtype=np.float32)[:, None]


def shared_border():
    """row 0 is a border point of two clusters: its neighbours a = (0, 0) and b = (2, 0) are core at min_samples <= 5 (each has
    exactly 5 rows within eps = 1, itself included), it is not (3 rows).  b's cluster comes first in the array, so it is number 0
    and the border point takes 0.  min_samples = 6: no core row, everything is noise"""
    p = [(1, 0)]
    b = [(2, 0), (2, 1), (2, -1), (3, 0)]
    a = [(0, 0), (0, 1), (0, -1), (-1, 0)]
    return np.array(p + b + a, dtype=np.float32)


def lattice_cloud(n, d, side, seed):
    """n integer points in [0, side)^d: many pairs at distance exactly 1, sqrt 2, 2"""
    return np.random.RandomState(seed).randint(0, side, size=(n, d)).astype(np.float32)


def dbscan_cases(tile=64):
    """name -> (x, eps, min_samples).  Every case but the blobs is an integer lattice with pairs at exactly eps"""
    cases = {
        "lattice_2d": (lattice_cloud(120, 2, 24, 21), 2.0, 4),
        "lattice_3d": (lattice_cloud(150, 3, 7, 22), 1.0, 3),
        "lattice_2d_min1": (lattice_cloud(90, 2, 16, 23), 1.0, 1),
        "chain": (chain(tile), 1.0, 3),
        "shared_border_4": (shared_border(), 1.0, 4),
        "shared_border_5": (shared_border(), 1.0, 5),
        "all_noise": (shared_border(), 1.0, 6),
    }
    for d in (16, 768):
        cases["blobs_%d" % d] = (blob_case(d)[1][0], 0.5, 5)
    return cases


def vote_tie():
    """pairs of points 1 apart, 10 between pairs, labelled (1, 0): at k = 2 every vote is a 1 : 1 tie, which goes to class 0"""
    x = (10 * np.repeat(np.arange(6), 2) + np.tile(np.arange(2), 6)).astype(np.float32)[:, None]
    return x, np.tile(np.array([1, 0]), 6)


def knn_cases():
    """name -> (x, y, k)"""
    out = {"vote_tie": (*vote_tie(), 2)}
    for d in (16, 768):
        x, _, noisy = blob_case(d)[1]
        out["blobs_%d" % d] = (x, noisy, KNN_K)
    return out


def random_labelings(count=40):
    """seeded pairs of labelings for the NMI / ARI restatement: sizes 2 .. 200, 1 .. 7 classes, some identical, some single-class"""
    out = []
    for seed in range(count):
        rs = np.random.RandomState(100 + seed)
        n = int(rs.randint(2, 201))
        a = rs.randint(0, rs.randint(1, 8), size=n)
        b = a.copy() if seed % 9 == 0 else rs.randint(-1, rs.randint(0, 7), size=n)
        out.append((a, b))
    return out
