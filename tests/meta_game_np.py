"""The maximin mixtures of an n_a x n_b zero-sum matrix game (include/soccer_hip.h, "the meta-game") restated in numpy: the saddle-point
test, the dense tableau with its shadow right-hand side, Dantzig's column, the ratio test whose ties the shadow column and
then the index break, the rank-1 update that skips no row, the strategies read from the true right-hand side and the bracket they
certify on the caller's matrix.  Everything is float64, a product and the sum that takes it are two roundings, and every sum
that the definition calls sequential is a loop here.  tests/test_gpu_meta_game.py holds the device to it bit for bit;
tests/test_meta_game_np.py checks what it computes where there is no GPU."""
import numpy as np

TOL = 1e-12
SHADOW = 2.0 ** -26


def lds_bytes(n_a, n_b):
    """the fit rule of the LDS kernel as the header states it"""
    stride = (n_a + n_b + 2) | 1
    return 128 + 8 * ((n_a + 2) * stride + n_a + 1) + 4 * n_a


def _seq_sum(z):
    acc = 0.0
    for v in z.tolist():
        acc = acc + v
    return acc


def _normalise(z):
    z = np.where(z > 0.0, z, 0.0)
    s = _seq_sum(z)
    return z / s if s > 0.0 else np.full(z.shape, 1.0 / z.size)


def bracket(A, x, y):
    """lo = min_j sum_i x[i] * A[i][j], hi = max_i sum_j A[i][j] * y[j], the sums sequential from 0.0 in index order"""
    n_a, n_b = A.shape
    col = np.zeros(n_b)
    for i in range(n_a):
        col = col + x[i] * A[i]
    row = np.zeros(n_a)
    for j in range(n_b):
        row = row + A[:, j] * y[j]
    return float(col[np.argmin(col)]), float(row[np.argmax(row)])


def solve(A, max_pivots=None):
    """One game.  Returns a dict of value, x, y, lo, hi, pivots, status and ties (the ratio tests that had more than one
    row at the minimum of the true ratio; not part of the definition, counted for the tests)."""
    A = np.ascontiguousarray(A, np.float64)
    n_a, n_b = A.shape
    if max_pivots is None:
        max_pivots = 100 * (n_a + n_b)
    rmin, cmax = A.min(1), A.max(0)
    i_s, j_s = int(np.argmax(rmin)), int(np.argmin(cmax))
    if rmin[i_s] == cmax[j_s]:
        x = np.zeros(n_a); y = np.zeros(n_b)
        x[i_s] = 1.0; y[j_s] = 1.0
        v = float(A[i_s, j_s])
        return {"value": v, "x": x, "y": y, "lo": v, "hi": v, "pivots": 0, "status": 1, "ties": 0}
    lo_a, hi_a = float(A.min()), float(A.max())
    rng = hi_a - lo_a
    ncol = n_b + n_a + 2
    R, S = n_b + n_a, n_b + n_a + 1
    T = np.zeros((n_a + 1, ncol))
    T[:n_a, :n_b] = (A - lo_a) / rng + 1.0
    T[:n_a, n_b:n_b + n_a] = np.eye(n_a)
    T[:n_a, R] = 1.0
    T[:n_a, S] = 1.0 + np.arange(1, n_a + 1) * SHADOW
    T[n_a, :n_b] = -1.0
    basis = np.arange(n_b, n_b + n_a)
    pivots, status, ties = 0, -1, 0
    while True:
        c = int(np.argmin(T[n_a, :n_a + n_b]))
        if not T[n_a, c] < -TOL:
            break
        if pivots == max_pivots:
            status = 3
            break
        col = T[:n_a, c]
        ok = col > TOL
        if not ok.any():
            status = 3
            break
        ratio = np.full(n_a, np.inf)
        ratio[ok] = T[:n_a, R][ok] / col[ok]
        tied = np.flatnonzero(ratio == ratio.min())                     # ascending, so argmin's first is the lowest row
        r = int(tied[np.argmin(T[tied, S] / col[tied])])
        ties += int(tied.size > 1)
        rowp = T[r] / T[r, c]
        rowp[c] = 1.0
        f = T[:, c].copy()
        T = T - f[:, None] * rowp[None, :]
        T[:, c] = 0.0
        T[r] = rowp
        basis[r] = c
        pivots += 1
    yq = np.zeros(n_b)
    for r in range(n_a):
        if basis[r] < n_b:
            yq[basis[r]] = T[r, R]
    x = _normalise(T[n_a, n_b:n_b + n_a].copy())
    y = _normalise(yq)
    lo, hi = bracket(A, x, y)
    if status != 3:
        amax = max(hi_a, -lo_a)
        eps = 1e-10 * (amax if amax > 1.0 else 1.0)
        status = 0 if hi - lo <= eps else 2
    return {"value": 0.5 * (lo + hi), "x": x, "y": y, "lo": lo, "hi": hi, "pivots": pivots, "status": status, "ties": ties}


def solve_batch(A, max_pivots=None):
    """[g, n_a, n_b] -> a dict of stacked arrays, each game solved alone"""
    A = np.asarray(A, np.float64)
    res = [solve(a, max_pivots) for a in A.reshape((-1,) + A.shape[-2:])]
    return {k: np.array([r[k] for r in res]) for k in res[0]}


def eps_of(A):
    return 1e-10 * max(1.0, float(np.abs(A).max()))


# ---- the input families of the tests (CPU and GPU draw the same matrices) ---------------------------------------------
def family(kind, n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((n_a, n_b))
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, (n_a, n_b))
    if kind == "integer":
        return rng.integers(-1, 2, (n_a, n_b)).astype(np.float64)
    if kind == "antisymmetric":
        n = min(n_a, n_b)
        M = rng.standard_normal((n, n))
        return M - M.T
    if kind == "duplicated":
        M = rng.standard_normal((n_a, n_b))
        M[rng.integers(0, n_a, n_a // 3)] = M[rng.integers(0, n_a, n_a // 3)]
        M[:, rng.integers(0, n_b, n_b // 3)] = M[:, rng.integers(0, n_b, n_b // 3)]
        return M
    if kind.startswith("rank"):                     # "rank3" or "rank3c" (clipped to [-1, 1])
        k = int(kind[4])
        M = product(rng.standard_normal((n_a, k)), rng.standard_normal((k, n_b)))
        return np.clip(M, -1.0, 1.0) if kind.endswith("c") else M
    raise ValueError(kind)


def product(U, V):
    """U @ V as a sum of outer products in index order: elementwise, so every machine draws the same bits (a BLAS may not)"""
    M = np.zeros((U.shape[0], V.shape[1]))
    for k in range(U.shape[1]):
        M = M + U[:, k, None] * V[None, k, :]
    return M


def large_game():
    """1024 x 1024: a rank-3 product plus 1e-3 uniform noise"""
    rng = np.random.default_rng(0)
    return product(rng.standard_normal((1024, 3)), rng.standard_normal((3, 1024))) + 1e-3 * rng.uniform(-1, 1, (1024, 1024))


def highs_value(A):
    """the game's value from scipy's HiGHS: max v s.t. A^T x >= v, sum x = 1, x >= 0"""
    from scipy.optimize import linprog
    n_a, n_b = A.shape
    c = np.zeros(n_a + 1); c[-1] = -1.0
    A_ub = np.hstack([-A.T, np.ones((n_b, 1))])
    A_eq = np.ones((1, n_a + 1)); A_eq[0, -1] = 0.0
    res = linprog(c, A_ub=A_ub, b_ub=np.zeros(n_b), A_eq=A_eq, b_eq=[1.0], bounds=[(0, None)] * n_a + [(None, None)],
                  method="highs")
    assert res.status == 0, res.message
    return float(res.x[-1])


# (name, kind, n_a, n_b, seed): what tests/test_gpu_meta_game.py holds to the bits and tests/test_meta_game_np.py to HiGHS
SHAPES = [("1x1", "normal", 1, 1, 11), ("1x7", "normal", 1, 7, 12), ("7x1", "normal", 7, 1, 13), ("2x2", "uniform", 2, 2, 14),
          ("3x7", "normal", 3, 7, 15), ("7x3", "normal", 7, 3, 16), ("5x5", "uniform", 5, 5, 17),
          ("63x65", "uniform", 63, 65, 18), ("64x64", "antisymmetric", 64, 64, 19), ("65x63", "normal", 65, 63, 20),
          ("40x150", "rank5", 40, 150, 21), ("150x40", "uniform", 150, 40, 22),
          ("130x70-integer", "integer", 130, 70, 1),        # ties in 26 of its 180 ratio tests
          ("45x37-duplicated", "duplicated", 45, 37, 23), ("100x90-rank3c", "rank3c", 100, 90, 24),
          ("256x256", "uniform", 256, 256, 25),
          ("300x20", "uniform", 300, 20, 26), ("20x300", "normal", 20, 300, 27)]       # more rows, more columns than threads


def shape(name):
    _, kind, n_a, n_b, seed = next(s for s in SHAPES if s[0] == name)
    return family(kind, n_a, n_b, seed)
