"""The case table of the MMD tests and a float64 numpy restatement of the arithmetic contract of csrc/mmd.hip: the pooled Gaussian
kernel from float64 distances of the float32 inputs (zero diagonal), the three sums per label vector, mmd2.  Inputs are rebuilt
from seeds; tests/golden/mmd.pt (tools/gen_golden_mmd.py) holds what the reference's mmd.py gives on them."""

import functools

import numpy as np

# name: n rows of X, m rows of Y, d features, P permutations; X is unit normal, Y unit normal + shift on every feature, both
# + offset on every feature; seed: the data's, pseed: the permutation test's
CASES = {
    "n70_m61_d33_p130": dict(n=70, m=61, d=33, P=130, shift=0.25, offset=0.0, seed=101, pseed=42),     # 3-row tail tile, d % 4 != 0, P tail
    "n64_m64_d32_p64": dict(n=64, m=64, d=32, P=64, shift=0.3, offset=0.0, seed=102, pseed=42),        # exactly one tile
    "n20_m23_d5_p50": dict(n=20, m=23, d=5, P=50, shift=0.5, offset=0.0, seed=103, pseed=42),          # less than a tile
    "n200_m157_d768_p257": dict(n=200, m=157, d=768, P=257, shift=0.15, offset=0.0, seed=104, pseed=42),  # three tiles, P crosses 256
    "n150_m150_d16_p200_null": dict(n=150, m=150, d=16, P=200, shift=0.0, offset=0.0, seed=5326, pseed=42),  # mid-range p-value; seed searched for gap >= 100 err_ref
    "n90_m100_d64_p100_offset10": dict(n=90, m=100, d=64, P=100, shift=0.2, offset=10.0, seed=106, pseed=42),  # fails without centring
    "n600_m500_d16_p40": dict(n=600, m=500, d=16, P=40, shift=0.1, offset=0.0, seed=107, pseed=42),    # 9 tiles = 9 splits x 1 tile (two per split from N = 2945: ref_exact_tile.py); subsampled median
    "n2_m2_d1_p1": dict(n=2, m=2, d=1, P=1, shift=1.0, offset=0.0, seed=108, pseed=43),                # tiny; pseed 43 draws a mixed split
}
LABEL_CASES = ("n20_m23_d5_p50", "n2_m2_d1_p1")          # the golden stores the reference's label matrix
KERNEL_CASES = ("n70_m61_d33_p130", "n20_m23_d5_p50")    # the golden stores the reference's gaussian_rbf_kernel(X, Y)
SUBSAMPLE = 1000                                         # median_heuristic's default


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (X float32 (n, d), Y float32 (m, d)); never written to"""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    X = (rng.randn(c["n"], c["d"]) + c["offset"]).astype(np.float32)
    Y = (rng.randn(c["m"], c["d"]) + c["shift"] + c["offset"]).astype(np.float32)
    for a in (X, Y):
        a.setflags(write=False)
    return X, Y


def sqdist64(a, b):
    """float64 squared distances of the rows of a and b, from differences (no Gram form)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((len(a), len(b)))
    step = max(1, (1 << 22) // max(1, len(b) * a.shape[1]))
    for i in range(0, len(a), step):
        diff = a[i:i + step, None, :] - b[None, :, :]
        out[i:i + step] = (diff * diff).sum(-1)
    return out


def pooled_kernel(X, Y, bandwidth):
    """float64 (N, N): exp(-D / (2 bandwidth)) with a zero diagonal"""
    pool = np.concatenate([X, Y], axis=0)
    K = np.exp(-sqdist64(pool, pool) / (2.0 * bandwidth))
    np.fill_diagonal(K, 0.0)
    return K


def sums(K, labels):
    """float64 (P, 3) {sum_XX, sum_YY, sum_XY} by the contract's expressions: quad, T - 2 z'r + quad, z'r - quad"""
    z = np.asarray(labels, dtype=np.float64)
    r = K.sum(1)
    T = r.sum()
    quad = ((z @ K) * z).sum(1)
    zr = z @ r
    return np.stack([quad, T - 2.0 * zr + quad, zr - quad], axis=1)


def mmd2(s, n, m):
    return s[:, 0] / (n * (n - 1.0)) + s[:, 1] / (m * (m - 1.0)) - 2.0 * s[:, 2] / (float(n) * m)


def permutation_labels(n, m, P, seed):
    """the reference's z_obs / z_null (mmd.py:185-195) as one uint8 matrix, row 0 the observed split"""
    N = n + m
    z = np.zeros((P + 1, N), dtype=np.uint8)
    z[0, :n] = 1
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(N) for _ in range(P)])
    z[np.arange(P)[:, None] + 1, perms[:, :n]] = 1
    return z


@functools.lru_cache(maxsize=None)
def restatement(name, bandwidth):
    """-> float64 (P + 1,): mmd2 of the observed split and of every permutation; computed once per (case, bandwidth)"""
    c = CASES[name]
    X, Y = build(name)
    K = pooled_kernel(X, Y, bandwidth)
    v = mmd2(sums(K, permutation_labels(c["n"], c["m"], c["P"], c["pseed"])), c["n"], c["m"])
    v.setflags(write=False)
    return v


def median_pool(X, Y, subsample=SUBSAMPLE):
    """the rows the median heuristic looks at (mmd.py:29-33)"""
    pool = np.concatenate([X, Y], axis=0).astype(np.float32)
    if len(pool) > subsample:
        pool = pool[np.random.default_rng(0).choice(len(pool), subsample, replace=False)]
    return pool


def gram_sqdist_f32(pool, rows=None, cols=None):
    """a float32 numpy emulation of the centred Gram form (numpy's own fp32 summation order): mean in float64 rounded to fp32,
    c = x - mean, n_i = sum c^2, D = max(n_i + n_j - 2 c_i . c_j, 0)"""
    pool = np.asarray(pool, dtype=np.float32)
    mean = pool.astype(np.float64).mean(0).astype(np.float32)
    c = pool - mean
    nrm = (c * c).sum(1, dtype=np.float32)
    a = c if rows is None else c[rows]
    b = c if cols is None else c[cols]
    na = nrm if rows is None else nrm[rows]
    nb = nrm if cols is None else nrm[cols]
    return np.maximum((na[:, None] + nb[None, :]) - np.float32(2.0) * (a @ b.T), np.float32(0.0))


def dist_err_f32(X, Y):
    """max |D - D64| of the emulation over the strict upper triangle of the median heuristic's rows"""
    pool = median_pool(X, Y)
    iu = np.triu_indices(len(pool), 1)
    return float(np.abs(gram_sqdist_f32(pool).astype(np.float64) - sqdist64(pool, pool))[iu].max())


def exponent_err_f32(X, Y, bandwidth):
    """max |D / fl32(2 bandwidth) - D64 / (2 bandwidth)| of the emulation over the X x Y block of the pooled kernel"""
    pool = np.concatenate([X, Y], axis=0).astype(np.float32)
    n = len(X)
    rows, cols = np.arange(n), np.arange(n, len(pool))
    e32 = gram_sqdist_f32(pool, rows, cols) / np.float32(2.0 * bandwidth)
    return float(np.abs(e32.astype(np.float64) - sqdist64(X, Y) / (2.0 * bandwidth)).max())
