"""The case table of the logistic-regression tests, the float64 numpy evaluator of the data term that ``newton_fit`` takes, the
objective's gradient in the solver's coordinates, a tight reference solve ``w*`` (Newton until ``|g| <= 1e-13 |g(0)|``) and the
duck-typed adata of the pipeline tests.  Inputs are rebuilt from seeds; tests/golden/logreg.pt (tools/gen_golden_logreg.py) holds
what sklearn and the reference's train_linear_classifier give on them.

Data.  x = mean[class] + noise: class means of norm ``sep`` along random directions, unit Gaussian noise, rounded to fp32 (the
shape of standardised embeddings); ``flip`` relabels that fraction of the rows at random, which keeps accuracy and AUROC below 1
while the rows stay far from the decision boundary.

Importable without a GPU; nothing here touches a device or imports viscy_amd."""

import functools

import numpy as np

LIBLINEAR = dict(solver="liblinear", max_iter=1000)
# name: n rows, d features, counts per class, seed, sep; params: the estimator's keywords.  What each case covers is in the
# issue's table: d % 4 != 0 under one block; a second tile of 4 columns at 1:5 imbalance; the workload's width with 21 tile pairs
# and 3 row splits; the one-vs-rest cp / cn rule; saturated sigmoids; no intercept with C = 0.1; the unpenalised intercept; dict weights
CASES = {
    "bin_n40_d5": dict(counts=(22, 18), d=5, seed=401, sep=2.0, params=dict(LIBLINEAR)),
    "bin_n300_d132_bal": dict(counts=(250, 50), d=132, seed=402, sep=3.0, params=dict(LIBLINEAR, class_weight="balanced")),
    "bin_n1300_d768_bal": dict(counts=(900, 400), d=768, seed=403, sep=3.0, params=dict(LIBLINEAR, class_weight="balanced")),
    "ovr3_n600_d96_bal": dict(counts=(300, 220, 80), d=96, seed=404, sep=3.0, params=dict(LIBLINEAR, class_weight="balanced")),
    "bin_sep_n200_d20": dict(counts=(100, 100), d=20, seed=405, sep=30.0, params=dict(LIBLINEAR, C=100.0)),
    "bin_n257_d260_noint_C01": dict(counts=(130, 127), d=260, seed=406, sep=3.0, params=dict(LIBLINEAR, fit_intercept=False, C=0.1)),
    "bin_n300_d132_lbfgs": dict(counts=(200, 100), d=132, seed=407, sep=3.0, params=dict(solver="lbfgs", max_iter=1000, class_weight="balanced")),
    "dictw_n300_d20": dict(counts=(180, 120), d=20, seed=408, sep=2.0, params=dict(LIBLINEAR, class_weight={0: 0.5, 1: 3.0})),
}
SPLIT_SEEDS = (0, 7, 42)
UNDECIDED_CAP = 0.02


def planted(counts, d, seed, sep, flip=0.0, names=None):
    """-> (x float32 (n, d), y (n,)): rows in a seeded random order; labels 0 .. K - 1, or ``names``"""
    rng = np.random.RandomState(seed)
    K = len(counts)
    means = rng.randn(K, d)
    means *= sep / np.linalg.norm(means, axis=1, keepdims=True)
    y = np.repeat(np.arange(K), counts)
    x = means[y] + rng.randn(len(y), d)
    if flip:
        hit = rng.rand(len(y)) < flip
        y = np.where(hit, rng.randint(0, K, len(y)), y)
    order = rng.permutation(len(y))
    x, y = np.ascontiguousarray(x[order].astype(np.float32)), y[order]
    if names is not None:
        y = np.asarray(names, dtype=object)[y]
    x.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    return planted(c["counts"], c["d"], c["seed"], c["sep"])


# ------------------------------------------------------------------------------------------------ the objective, restated
def data_terms(x64, y_pm, c, w, b, want_hessian=True):
    """(sum loss, X'r, sum r, X' diag(s) X, X's, sum s) of sum_i c_i log(1 + exp(-y_i z_i)), z = x.w + b, float64, the sigmoid
    formed without cancellation"""
    z = x64 @ w + b
    m = y_pm * z
    e = np.exp(-np.abs(m))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sig, om = np.where(m >= 0, big, small), np.where(m >= 0, small, big)
    loss = float(np.sum(c * (np.log1p(e) + np.maximum(-m, 0.0))))
    if not want_hessian:
        return loss, None, None, None, None, None
    r = -c * y_pm * om
    s = c * sig * om
    return loss, x64.T @ r, float(r.sum()), x64.T @ (s[:, None] * x64), x64.T @ s, float(s.sum())


def class_weight_values(class_weight, K, y_idx):
    if class_weight is None:
        return np.ones(K)
    if class_weight == "balanced":
        return len(y_idx) / (K * np.bincount(y_idx, minlength=K).astype(np.float64))
    return np.array([float(class_weight.get(k, 1.0)) for k in range(K)])


def problems(params, y_idx):
    """-> [(y in {-1, +1} (n,), c (n,), n_pos)]: the binary problem (positive: the second class, cp = C weight_1,
    cn = C weight_0), or for K > 2 one per class with cp = C weight_k and cn = C"""
    K = int(y_idx.max()) + 1
    wt = class_weight_values(params.get("class_weight"), K, y_idx)
    C = float(params.get("C", 1.0))
    out = []
    for k, cp, cn in ([(1, C * wt[1], C * wt[0])] if K == 2 else [(k, C * wt[k], C) for k in range(K)]):
        pos = y_idx == k
        out.append((np.where(pos, 1.0, -1.0), np.where(pos, cp, cn), int(pos.sum())))
    return out


def penalty_of(params, d):
    """the diagonal of P over u = [w; w_b] (w_b only with an intercept): liblinear penalises w_b, the other solvers do not"""
    if not params.get("fit_intercept", True):
        return np.ones(d)
    return np.concatenate((np.ones(d), [1.0 if params["solver"] == "liblinear" else 0.0]))


def full_terms(x64, prob, params, u):
    """objective, gradient and Hessian at u = [w; w_b] (intercept_scaling 1: b = w_b)"""
    d = x64.shape[1]
    pen = penalty_of(params, d)
    icpt = len(pen) > d
    loss, g, g_b, G, h_b, ss = data_terms(x64, prob[0], prob[1], u[:d], u[d] if icpt else 0.0)
    grad = pen * u
    grad[:d] += g
    H = np.diag(pen)
    H[:d, :d] += G
    if icpt:
        grad[d] += g_b
        H[:d, d] += h_b
        H[d, :d] += h_b
        H[d, d] += ss
    return 0.5 * float(pen @ (u * u)) + loss, grad, H


def gradient(x64, prob, params, coef, intercept):
    """the gradient at (coef, intercept) in the coordinates u"""
    d = x64.shape[1]
    u = np.concatenate((coef, [intercept])) if len(penalty_of(params, d)) > d else np.asarray(coef, dtype=np.float64).copy()
    return full_terms(x64, prob, params, u)[1]


def epsilon(params, n_pos, n):
    """the solver's stopping rule: min(liblinear's tol min(n_pos, n_neg) / n, 1e-10)"""
    return min(params.get("tol", 1e-4) * max(min(n_pos, n - n_pos), 1) / n, 1e-10)


def solve(x64, prob, params, rtol=1e-13, max_iter=200):
    """-> (u*, |g(0)|, smallest eigenvalue of the Hessian at u*): plain Newton with halving on the objective, float64"""
    k = len(penalty_of(params, x64.shape[1]))
    u = np.zeros(k)
    f, g, H = full_terms(x64, prob, params, u)
    g0 = np.linalg.norm(g)
    for _ in range(max_iter):
        if np.linalg.norm(g) <= rtol * g0:
            break
        p = np.linalg.solve(H, -g)
        t = 1.0
        while t > 1e-10:
            f_new, g_new, H_new = full_terms(x64, prob, params, u + t * p)
            if f_new <= f + 1e-4 * t * float(g @ p) + 8 * np.finfo(float).eps * abs(f):
                break
            t *= 0.5
        if np.linalg.norm(g_new) >= np.linalg.norm(g) and f_new >= f:
            break
        u, f, g, H = u + t * p, f_new, g_new, H_new
    assert np.linalg.norm(g) <= 100 * rtol * g0, (np.linalg.norm(g), g0)
    return u, float(g0), float(np.linalg.eigvalsh(H)[0])


@functools.lru_cache(maxsize=None)
def optimum(name):
    """-> [(u*, |g(0)|, lambda_min, eps)] per problem of the case"""
    x, y = build(name)
    x64, params = x.astype(np.float64), CASES[name]["params"]
    out = []
    for prob in problems(params, y):
        u, g0, lam = solve(x64, prob, params)
        u.setflags(write=False)
        out.append((u, g0, lam, epsilon(params, prob[2], len(y))))
    return out


def stack_u(coef, intercept, params, d):
    """(problems, k): [coef | intercept] rows in the coordinates u"""
    coef = np.atleast_2d(np.asarray(coef, dtype=np.float64))
    if len(penalty_of(params, d)) > d:
        return np.concatenate((coef, np.asarray(intercept, dtype=np.float64).reshape(-1, 1)), axis=1)
    return coef


def row_bound(x, dist):
    """how far a margin of row i moves when u moves by ``dist``: (|x_i| + 1) dist, and twice that between two such fits"""
    return 2.0 * (np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1) + 1.0) * dist


def decided(z, bound):
    """rows whose label a margin error of ``bound`` cannot change: |z| for one problem, else the gap of the two largest"""
    z = np.asarray(z, dtype=np.float64)
    if z.ndim == 1:
        return np.abs(z) > bound
    top = np.sort(z, axis=1)
    return top[:, -1] - top[:, -2] > bound


# ------------------------------------------------------------------------------------------------ splits and metrics fixtures
def split_labels(seed):
    """string labels (three classes, one rare) and group ids of the split tests"""
    rng = np.random.RandomState(500 + seed)
    y = np.asarray(["infected", "uninfected", "dividing"], dtype=object)[rng.choice(3, 203, p=(0.5, 0.4, 0.1))]
    return y, rng.randint(0, 37, len(y))


def metric_fixtures():
    """name -> (y_true, y_pred, score of the positive / per-class scores): ties in the scores, a class never predicted"""
    rng = np.random.RandomState(600)
    yb = rng.randint(0, 2, 120)
    sb = np.round(rng.rand(120) + 0.5 * yb, 1)            # rounded: many tied scores
    y3 = np.asarray(["a", "b", "c"], dtype=object)[rng.choice(3, 150, p=(0.5, 0.4, 0.1))]
    p3 = rng.dirichlet(np.ones(3), 150) + 0.8 * (y3[:, None] == np.asarray(["a", "b", "c"], dtype=object)[None, :])
    p3 /= p3.sum(1, keepdims=True)
    pred3 = np.asarray(["a", "b"], dtype=object)[np.argmax(p3[:, :2], axis=1)]   # "c" is absent from the predictions
    return {"binary_ties": (yb, (sb > 0.7).astype(int), sb), "three_absent": (y3, pred3, p3)}


# ------------------------------------------------------------------------------------------------ the pipeline's adata
PIPE_CLASSES = ("dividing", "infected", "uninfected")
PIPE_COUNTS = (40, 280, 280)
# tol: liblinear at its default 1e-4 stops 1e-3 away from the optimum, which leaves the labels of rows within 0.5 of the boundary
# to its stopping point; at 1e-7 every row of the fixture is decided and the count metrics are a property of the objective
PIPE_PARAMS = dict(solver="liblinear", class_weight="balanced", max_iter=1000, tol=1e-7)
# name: (use_scaling, use_pca, n_pca_components, grouped, split_train_data)
PIPE_CONFIGS = {
    "raw": (False, False, None, False, 0.8),
    "scaled": (True, False, None, False, 0.8),
    "scaled_pca8": (True, True, 8, False, 0.8),
    "scaled_groups": (True, False, None, True, 0.75),
    "scaled_all": (True, False, None, False, 1.0),
}


class FakeAnnData:
    """what the reference reads of an AnnData: X, obs, obsm, uns and a length"""

    def __init__(self, X, obs):
        self.X, self.obs, self.obsm, self.uns = X, obs, {}, {}

    def __len__(self):
        return len(self.obs)


def pipe_task():
    return "cell_state"


PIPE_LATENT = (8.0, 7.0, 6.0, 5.0, 4.2, 3.5)


@functools.lru_cache(maxsize=None)
def pipe_arrays():
    """-> (x float32 (600, 96), y strings, groups, fov names): well separated class means, 8 % of the labels redrawn, and six
    planted directions of falling spread, so that with the two of the class means the eight leading principal components stand
    clear of the noise floor and of each other (sklearn's PCA takes its randomized solver at this shape; it is exact to rounding
    only on such a spectrum)"""
    x, y = planted(PIPE_COUNTS, 96, 450, 9.0, flip=0.08, names=PIPE_CLASSES)
    rng = np.random.RandomState(451)
    groups = rng.randint(0, 60, len(y))
    fov = np.asarray([f"{'AB'[i % 2]}/{1 + i % 3}/{i % 5}" for i in range(len(y))], dtype=object)
    Q, _ = np.linalg.qr(rng.randn(96, len(PIPE_LATENT)))
    x = np.ascontiguousarray((x.astype(np.float64) + (rng.randn(len(y), len(PIPE_LATENT)) * np.asarray(PIPE_LATENT)) @ Q.T).astype(np.float32))
    x.setflags(write=False)
    return x, y, groups, fov


def pipe_adata(X=None):
    import pandas as pd

    x, y, _, fov = pipe_arrays()
    return FakeAnnData(np.array(x) if X is None else X, pd.DataFrame({pipe_task(): y, "fov_name": fov}))
