"""The case table of the PCA tests, a float64 numpy restatement of what viscy_amd.reduce computes (mean -> centred Gram -> scale ->
eigh -> flip), a float32 emulation of the arithmetic of csrc/pca.hip (centred values rounded to fp32, fp32 sums over blocks of 128
rows, float64 past the block, fp32 projection) and integer fixtures on which float64 is exact.  Inputs are rebuilt from seeds;
tests/golden/pca.pt (tools/gen_golden_pca.py) holds what the reference's compute_pca and sklearn give on them.

Data.  x = offset + latent @ diag(s) @ Q' + floor * noise: eight planted orthonormal directions Q whose standard deviations s fall
by sqrt(2) each (variances 64, 32, .. 0.5), an isotropic floor, and a column offset of up to 10 x the largest planted standard
deviation (uniform in [-80, 80]), so a Gram that is not centred first loses the spectrum in fp32.  The eight leading eigenvalues
are then about 2 x apart and their eigenvectors well conditioned; ``gaps_ok`` is the condition the tests put on every component
they compare.

Importable without a GPU; nothing here touches a device or viscy_amd."""

import functools

import numpy as np

R = 128                   # GM_R: rows per fp32 block
T = 128                   # FT_T: features per tile
GM_MIN_BLOCKS, GM_MAX_SPLITS, GM_WANT_WGS = 4, 32, 512
CM_COLS, CM_MIN_ROWS, CM_WANT_WGS = 64, 512, 2048
MAX_D = 4096
GAP = 1.2                 # eigenvalue ratio to both neighbours of a compared component
PLANTED = 8
OFFSET = 80.0             # 10 x the largest planted standard deviation


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch arithmetic, restated
def gram_plan(n, d):
    """gm_split -> (tiles, tile pairs, splits, rows per split)"""
    tiles = cdiv(d, T)
    pairs = tiles * (tiles + 1) // 2
    want = min(max(GM_WANT_WGS // pairs, 1), GM_MAX_SPLITS)
    bps = max(cdiv(cdiv(n, R), want), GM_MIN_BLOCKS)
    return tiles, pairs, cdiv(n, bps * R), bps * R


def gram_ws_bytes(n, d):
    _, pairs, splits, _ = gram_plan(n, d)
    return splits * pairs * T * T * 8


def moments_ws_bytes(n, d):
    want = min(cdiv(CM_WANT_WGS, cdiv(d, CM_COLS)), cdiv(n, CM_MIN_ROWS))
    rps = cdiv(n, want)
    return cdiv(n, rps) * d * 8


# ------------------------------------------------------------------------------------------------ the case table
R132 = gram_plan(512, 132)[3]   # rows per split at d = 132 for every N of the table: 512
# name: N rows, d features, k = n_components (None, int or fraction), seed; floor: the isotropic standard deviation;
# offset: the column means are uniform in [-offset, offset] (default 80); const: a column set to one value
CASES = {
    "n2_d4_k1": dict(N=2, d=4, k=1, seed=201, floor=0.3),                    # the minimum
    "n33_d33_all": dict(N=33, d=33, k=None, seed=202, floor=0.1),            # d % 4 != 0: scalar loads; N = D
    "n129_d128_k8": dict(N=129, d=128, k=8, seed=203, floor=0.1),            # exactly one tile; one row past a 128 block
    "n300_d132_k8": dict(N=300, d=132, k=8, seed=204, floor=0.1),            # a second tile of 4 columns
    "n257_d260_k8": dict(N=257, d=260, k=8, seed=205, floor=0.1),            # three tiles: off-diagonal tile pairs and the mirror
    "n1300_d768_k8": dict(N=1300, d=768, k=8, seed=206, floor=0.1),          # the product's width: 21 tile pairs, three splits
    # sklearn's covariance_eigh case, all 64 components.  That route forms X'X - n mean mean' in the input's float32, so the
    # reference's own error grows with (offset / spread)^2: the offset is a quarter of the leading spread here, 10 x elsewhere
    "n1000_d64_all": dict(N=1000, d=64, k=None, seed=207, floor=0.1, offset=2.0),
    "n600_d96_f09": dict(N=600, d=96, k=0.9, seed=209, floor=0.2),           # the fraction rule (seeds searched for the gap)
    # row counts at d = 132 (k = 3 keeps the golden small; the eight leading components are still conditioned)
    "n300_d132_const": dict(N=300, d=132, k=3, seed=309, floor=0.1, const=(5, 3.25)),   # a constant column: scale 1, eigenvalue 0
    "n100_d132_wide": dict(N=100, d=132, k=3, seed=210, floor=0.1),          # N < D: d - N + 1 zero eigenvalues
    "n511_d132": dict(N=R132 - 1, d=132, k=3, seed=211, floor=0.1),          # one split, ragged last block
    "n512_d132": dict(N=R132, d=132, k=3, seed=212, floor=0.1),              # one full split
    "n513_d132": dict(N=R132 + 1, d=132, k=3, seed=213, floor=0.1),          # two splits, the second of one row
    "n127_d132": dict(N=R - 1, d=132, k=3, seed=214, floor=0.1),             # one below the block
    "n129_d132": dict(N=R + 1, d=132, k=3, seed=215, floor=0.1),             # one above: a block of one row
}
NORMALIZE = (True, False)
PROJECT_K = (1, 127, 128, 129)     # k edges of vsx_center_project: below, at and past one column tile
PROJECT_D = (33, 768)
PROJECT_N = 130                    # two row tiles, the second of two rows


@functools.lru_cache(maxsize=None)
def build(name):
    """-> x float32 (N, d); never written to"""
    c = CASES[name]
    N, d = c["N"], c["d"]
    rng = np.random.RandomState(c["seed"])
    r = min(PLANTED, d)
    Q, _ = np.linalg.qr(rng.randn(d, r))
    s = 8.0 * np.sqrt(0.5) ** np.arange(r)
    x = (rng.randn(N, r) * s) @ Q.T + c["floor"] * rng.randn(N, d) + rng.uniform(-1.0, 1.0, d) * c.get("offset", OFFSET)
    if "const" in c:
        x[:, c["const"][0]] = c["const"][1]
    x = np.ascontiguousarray(x.astype(np.float32))
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ float64 restatement
def scale_of(n, mean, m2):
    """StandardScaler's rule: ddof 0; scale 1 where sklearn's _is_constant_feature holds"""
    var = m2 / n
    eps = np.finfo(np.float64).eps
    scale = np.sqrt(var)
    scale[var <= n * eps * var + (n * mean * eps) ** 2] = 1.0
    return var, scale


def spectrum(n, d, gram, scale, k):
    """covariance -> (variances, ratios, singular values, components (rows), n_components, noise variance), all d of them but for
    the last two; sklearn's _fit_full on the covariance_eigh route, restated"""
    C = gram / np.outer(scale, scale) / (n - 1.0)
    C = 0.5 * (C + C.T)
    w, v = np.linalg.eigh(C)
    w, v = w[::-1].copy(), v[:, ::-1].T.copy()
    w[w < 0.0] = 0.0
    for i in range(d):   # svd_flip(u_based_decision=False)
        if v[i, np.argmax(np.abs(v[i]))] < 0.0:
            v[i] = -v[i]
    ratio = w / w.sum()
    if k is None:
        kk = min(n, d)
    elif isinstance(k, float):
        kk = int(np.searchsorted(np.cumsum(ratio), k, side="right")) + 1
    else:
        kk = k
    noise = float(w[kk:].mean()) if kk < min(n, d) else 0.0
    return w, ratio, np.sqrt(w * (n - 1.0)), v, kk, noise


def _result(x64, mean, m2, gram, normalize, k, project):
    n, d = x64.shape
    var, scale = scale_of(n, mean, m2)
    if not normalize:
        scale = np.ones(d)
    w, ratio, sv, v, kk, noise = spectrum(n, d, gram, scale, k)
    out = dict(mean=mean, m2=m2, gram=gram, var=var, scale=scale, all_variance=w, explained_variance=w[:kk], ratio=ratio[:kk],
               singular_values=sv[:kk], components=v[:kk], n_components=kk, noise_variance=noise)
    out["Z"] = project(out)
    return out


@functools.lru_cache(maxsize=None)
def restatement(name, normalize=True):
    """float64 throughout, from differences: nothing is rounded to fp32 on the way.  Computed once per (case, normalize)"""
    x64 = build(name).astype(np.float64)
    mean = x64.mean(0)
    c = x64 - mean
    out = _result(x64, mean, (c * c).sum(0), c.T @ c, normalize, CASES[name]["k"], lambda o: (c / o["scale"]) @ o["components"].T)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def gaps_ok(all_variance, i):
    """component i is compared: its eigenvalue is GAP x away from both neighbours'"""
    w = all_variance
    up = i == 0 or w[i - 1] >= GAP * w[i]
    down = i + 1 >= len(w) or w[i] >= GAP * w[i + 1]
    return bool(up and down and w[i] > 0.0)


def compared(name, normalize=True):
    """indices below n_components whose components_ rows are compared: the planted directions.  (A floor eigenvalue can pass
    ``gaps_ok`` by chance at small N; its eigenvector is then conditioned by a gap of a few 1e-3 of the leading variance and moves
    by 1e-3 rad under any fp32-class perturbation: nothing a factor 4 between two fp32 summation orders would bound)"""
    r = restatement(name, normalize)
    return [i for i in range(min(r["n_components"], PLANTED)) if gaps_ok(r["all_variance"], i)]


def errors(res, ref, idx):
    """(variance error relative to the largest variance | max ratio error, max 1 - |cos| over the components idx, max |dZ| / max |Z|)
    of a result against a restatement; ``res``: dict with explained_variance, ratio, components, Z of the same k"""
    ev, ev0 = np.asarray(res["explained_variance"], dtype=np.float64), ref["explained_variance"]
    e_var = float(max(np.abs(ev - ev0).max() / ev0[0], np.abs(np.asarray(res["ratio"], dtype=np.float64) - ref["ratio"]).max()))
    comp = np.asarray(res["components"], dtype=np.float64)
    e_cos = 0.0
    for i in idx:
        # 1 - |cos| = |u -+ v|^2 / 2 for unit vectors: no cancellation, so angles below 1e-8 rad are still told apart
        u, v = comp[i] / np.linalg.norm(comp[i]), ref["components"][i] / np.linalg.norm(ref["components"][i])
        e_cos = max(e_cos, 0.5 * float(min(((u - v) ** 2).sum(), ((u + v) ** 2).sum())))
    Z, Z0 = np.asarray(res["Z"], dtype=np.float64), ref["Z"]
    cols = list(idx)   # the projection on a component that is not compared is as arbitrary as the component
    # a column follows its component's sign; whether the signs agree is ``signs_agree``'s question, asked where the flip is decided
    sg = np.array([1.0 if float(comp[i] @ ref["components"][i]) >= 0.0 else -1.0 for i in cols])
    e_z = float(np.abs(Z[:, cols] * sg - Z0[:, cols]).max() / np.abs(Z0).max()) if cols else 0.0
    return e_var, e_cos, e_z


def sign_decided(row):
    """svd_flip looks at the entry of largest magnitude: decided where it leads the runner-up by 1e-4, a hundred times what fp32 moves an entry by (two standardised rows give
    components whose entries all have magnitude 1 / sqrt(d): any of them may win)"""
    a = np.sort(np.abs(np.asarray(row, dtype=np.float64)))
    return len(a) < 2 or a[-1] > 1.0001 * a[-2]


def decided(name, normalize=True):
    r = restatement(name, normalize)
    return [i for i in compared(name, normalize) if sign_decided(r["components"][i])]


def signs_agree(comp, ref, idx):
    return all(float(np.asarray(comp[i], dtype=np.float64) @ ref["components"][i]) > 0.0 for i in idx)


# ------------------------------------------------------------------------------------------------ float32 emulation of csrc/pca.hip
def gram_f32_blocks(x, mean):
    """(d, d) float64: c = fl32(x - mean) (float64 difference), the products summed in fp32 row after row over blocks of R rows
    (elementwise numpy, no BLAS: the same bits on every host), the block sums added in float64"""
    c = (x.astype(np.float64) - mean).astype(np.float32)
    d = x.shape[1]
    g = np.zeros((d, d))
    for r0 in range(0, len(c), R):
        blk = np.zeros((d, d), dtype=np.float32)
        for row in c[r0:r0 + R]:
            blk += row[:, None] * row[None, :]
        g += blk.astype(np.float64)
    return g


def project_f32(c32, w32):
    """(n, k) float32: the dots summed in fp32 feature after feature (elementwise numpy)"""
    z = np.zeros((c32.shape[0], w32.shape[0]), dtype=np.float32)
    for j in range(c32.shape[1]):
        z += c32[:, j:j + 1] * w32[None, :, j]
    return z


@functools.lru_cache(maxsize=None)
def _emulated_gram(name):
    x = build(name)
    return gram_f32_blocks(x, x.astype(np.float64).mean(0))


@functools.lru_cache(maxsize=None)
def emulation(name, normalize=True):
    """the restatement's pipeline on the emulated Gram, with the fp32 projection fl32(c) @ fl32(components / scale)'"""
    x64 = build(name).astype(np.float64)
    mean = x64.mean(0)
    c = x64 - mean

    def project(o):
        return project_f32(c.astype(np.float32), (o["components"] / o["scale"][None, :]).astype(np.float32)).astype(np.float64)

    return _result(x64, mean, (c * c).sum(0), _emulated_gram(name), normalize, CASES[name]["k"], project)


@functools.lru_cache(maxsize=None)
def gram_err_f32(name, normalize=True):
    """-> the emulation's (variance, cosine, projection) errors against the restatement, as ``errors``"""
    return errors(emulation(name, normalize), restatement(name, normalize), compared(name, normalize))


# ------------------------------------------------------------------------------------------------ integer fixtures: float64 is exact
VMAX, CMAX = 256, 768   # |x - mean| <= 2^8, |mean| <= 768: |x| <= 2^10; a block's sum of products <= 128 * 2^16 = 2^23 < 2^24


@functools.lru_cache(maxsize=None)
def int_fixture(N, d, seed=0):
    """-> (x float32 (N, d), mean int64 (d,), m2 int64 (d,), gram int64 (d, d)).  Rows come as +v / -v pairs around the integer
    column centre c (an odd N adds the row c itself), permuted: every column mean is c exactly, every centred product an integer,
    every fp32 partial sum inside a block below 2^24 (the 2^24 method of tests/ref_exact_tile.py), every float64 fold exact"""
    rng = np.random.RandomState(1000 + seed)
    v = rng.randint(-VMAX, VMAX + 1, (N // 2, d)).astype(np.int64)
    rows = np.concatenate([v, -v, np.zeros((N % 2, d), dtype=np.int64)])[rng.permutation(N)]
    c = rng.randint(-CMAX, CMAX + 1, d).astype(np.int64)
    x = np.ascontiguousarray((rows + c).astype(np.float32))
    assert np.abs(x).max() <= 1024 and R * VMAX * VMAX < 2 ** 24
    r64 = rows.astype(np.float64)
    gram = (r64.T @ r64).astype(np.int64)   # exact: every sum is an integer below 2^53
    x.setflags(write=False)
    return x, c, np.diag(gram).copy(), gram


@functools.lru_cache(maxsize=None)
def int_weights(k, d, seed=0):
    """float32 (k, d) of integers in [-3, 3]: a centred row's dot stays below 768 * 256 * 3 < 2^24"""
    return np.ascontiguousarray(np.random.RandomState(2000 + seed).randint(-3, 4, (k, d)).astype(np.float32))


# (N, d) edges of the exact tests: the case table's shapes, both sides of a split and of a block, and a shape with a ragged
# multi-block second split
def exact_shapes():
    shapes = sorted({(c["N"], c["d"]) for c in CASES.values()})
    return shapes + [(R132 + R + 2, 132)]
