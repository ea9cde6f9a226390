"""The maximin mixtures of an n_a x n_b zero-sum matrix game (include/soccer_hip.h, "the meta-game") restated in numpy: the saddle-point
test, the dense tableau with its shadow right-hand side, Dantzig's column, the ratio test whose ties the shadow column and
then the index break, the rank-1 update that skips no row, the strategies read from the true right-hand side and the bracket they
certify on the caller's matrix.  Everything is float64, a product and the sum that takes it are two roundings, and every sum
that the definition calls sequential is a loop here.  tests/test_gpu_meta_game.py and tests/test_gpu_meta_game_edges.py hold the
device to it bit for bit;
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
    """One game.  Returns a dict of value, x, y, lo, hi, pivots, status and, not part of the definition and counted for the
    tests: ties (the ratio tests that had more than one row at the minimum of the true ratio), decided (those of them in
    which the shadow quotient chose another row than the lowest tied one, so that the middle key of the reduction mattered)
    and across (those of them whose two rows belong to different waves of a 256-thread workgroup that takes row i in thread
    i % 256, so that the cross-wave step of the kernels' reduction had to carry the middle key)."""
    A = np.ascontiguousarray(A, np.float64)
    n_a, n_b = A.shape
    if max_pivots is None:
        max_pivots = 100 * (n_a + n_b)
    with np.errstate(over="ignore", invalid="ignore"):
        if not np.isfinite(A.max() - A.min()):                          # refused before the saddle-point test, as the host does
            raise ValueError("max A - min A is not finite (%r - %r)" % (float(A.max()), float(A.min())))
    rmin, cmax = A.min(1), A.max(0)
    i_s, j_s = int(np.argmax(rmin)), int(np.argmin(cmax))
    if rmin[i_s] == cmax[j_s]:
        x = np.zeros(n_a); y = np.zeros(n_b)
        x[i_s] = 1.0; y[j_s] = 1.0
        v = float(A[i_s, j_s])
        return {"value": v, "x": x, "y": y, "lo": v, "hi": v, "pivots": 0, "status": 1, "ties": 0, "decided": 0, "across": 0}
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
    pivots, status, ties, decided, across = 0, -1, 0, 0, 0
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
        decided += int(r != tied[0])
        across += int(r % 256 // 64 != tied[0] % 256 // 64)
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
    return {"value": 0.5 * (lo + hi), "x": x, "y": y, "lo": lo, "hi": hi, "pivots": pivots, "status": status, "ties": ties,
            "decided": decided, "across": across}


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


# ---- the edges: games with closed-form values, tie-heavy games, shapes at the kernels' boundaries, numeric edges ----------
def identity(n):
    """value 1 / n"""
    return np.eye(n)


def cyclic(n):
    """odd n, antisymmetric, value 0: policy i beats the n // 2 after it and loses to the n // 2 before it"""
    assert n % 2 == 1
    A = np.zeros((n, n))
    for i in range(n):
        for d in range(1, n // 2 + 1):
            A[i, (i + d) % n] = 1.0
            A[i, (i - d) % n] = -1.0
    return A


def diagonal(n):
    """diag(1 .. n): value 1 / sum(1 / d)"""
    return np.diag(np.arange(1.0, n + 1.0))


def shuffled_cyclic(n, seed):
    """cyclic(n) with its rows and its columns permuted: value 0 still, and unlike cyclic(n), whose tied rows the shadow
    quotient orders as their indices do, a game in which the shadow quotient decides ties against the index"""
    rng = np.random.default_rng(seed)
    return cyclic(n)[rng.permutation(n)][:, np.random.default_rng(seed + 10).permutation(n)]


def block_base(m, seed):
    return np.random.default_rng(seed).integers(-2, 3, (m, m)).astype(np.float64)


def block(m, rep, seed):
    """every policy of a small integer game rep times: the small game's value, and every ratio test ties"""
    return np.kron(block_base(m, seed), np.ones((rep, rep)))


def padded_identity(n):
    """identity n with one more row and column, both strictly dominated: value 1 / n still"""
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = np.eye(n)
    A[n, :n] = -1.0
    A[:n, n] = 2.0
    return A


ULP1 = 2.0 ** -52                                   # one ulp of 1.0
LITERALS = {
    "8e307": [[8e307, -8e307], [-8e307, 8e307]],                        # the largest range that does not overflow
    "denormal": [[5e-324, 0.0], [0.0, 5e-324]],
    "ulp-apart": [[1.0, 1.0 + ULP1], [1.0 + ULP1, 1.0]],
    "1e6-ulp-apart": [[1e6, float(np.nextafter(1e6, np.inf))], [float(np.nextafter(1e6, np.inf)), 1e6]],
    "minus-zeros": [[-0.0, -0.0], [-0.0, -0.0]],                        # a saddle point whose value is -0.0
    "minus-zero-diagonal": [[-0.0, 1.0], [1.0, -0.0]],
}
OVERFLOWING = np.array([[1e308, -1e308], [-1e308, 1e308]])              # finite entries, max A - min A = inf: refused
SCALES = (-1000, -500, 500, 1000)


def edge_game(kind, args):
    if kind == "identity":
        return identity(*args)
    if kind == "cyclic":
        return cyclic(*args)
    if kind == "shuffled-cyclic":
        return shuffled_cyclic(*args)
    if kind == "diagonal":
        return diagonal(*args)
    if kind == "block":
        return block(*args)
    if kind == "literal":
        return np.array(LITERALS[args[0]])
    if kind == "scaled":                            # the 7 x 9 uniform game times 2^k, exactly
        return np.ldexp(family("uniform", 7, 9, args[1]), args[0])
    return family(kind, *args)


# (name, kind, args).  Boundary shapes: every loop of the kernels strides by 256 threads and meta_update_kernel cuts the
# tableau into tiles of 16 rows x 256 columns, so stride = (n_a + n_b + 2) | 1 of 255 / 257 / 513, rows = n_a + 1 of 16 / 17,
# n_a or n_b of 255 / 256 / 257 and of 1024 (the maximum) are where an off-by-one would show.
EDGE_SHAPES = [
    ("15x238", "uniform", (15, 238, 51)), ("16x238", "integer", (16, 238, 52)),
    ("127x127", "uniform", (127, 127, 53)), ("128x128", "integer", (128, 128, 54)),
    ("255x2", "uniform", (255, 2, 55)), ("256x2", "normal", (256, 2, 56)), ("257x2", "uniform", (257, 2, 57)),
    ("2x255", "uniform", (2, 255, 58)), ("2x256", "normal", (2, 256, 59)), ("2x257", "uniform", (2, 257, 60)),
    ("257x257-integer", "integer", (257, 257, 61)),
    ("17x494", "uniform", (17, 494, 62)), ("494x17", "uniform", (494, 17, 63)),
    ("2x1024", "uniform", (2, 1024, 64)), ("3x1024", "normal", (3, 1024, 65)),
    ("1024x2", "uniform", (1024, 2, 66)), ("1024x3", "normal", (1024, 3, 67)),
    ("1x1024", "normal", (1, 1024, 68)), ("1024x1", "normal", (1024, 1, 69)),
    ("identity-3", "identity", (3,)), ("identity-64", "identity", (64,)), ("identity-99", "identity", (99,)),
    ("identity-100", "identity", (100,)), ("identity-257", "identity", (257,)),
    ("cyclic-5", "cyclic", (5,)), ("cyclic-63", "cyclic", (63,)), ("cyclic-99", "cyclic", (99,)),
    ("cyclic-101", "cyclic", (101,)), ("cyclic-255", "cyclic", (255,)),
    ("shuffled-cyclic-99", "shuffled-cyclic", (99, 2)), ("shuffled-cyclic-255", "shuffled-cyclic", (255, 2)),
    ("diagonal-40", "diagonal", (40,)),
    ("block-6x10", "block", (6, 10, 100)), ("block-5x20", "block", (5, 20, 127)),      # seeds whose every ratio test ties
] + [(k, "literal", (k,)) for k in LITERALS] + [
    ("7x9", "scaled", (0, 90))] + [("7x9*2^%d" % k, "scaled", (k, 90)) for k in SCALES]


def edge(name):
    _, kind, args = next(s for s in EDGE_SHAPES if s[0] == name)
    return edge_game(kind, args)


def known_value(name):
    """(lo, hi) that hold the game's value, from a closed form (identity 1 / n, cyclic 0, diagonal 1 / sum(1 / d), +-a
    matching pennies 0) or, for a block game, the bracket of the small game it replicates; None where there is none"""
    from fractions import Fraction
    _, kind, args = next(s for s in EDGE_SHAPES if s[0] == name)
    if kind == "identity":
        return (1.0 / args[0],) * 2
    if kind in ("cyclic", "shuffled-cyclic") or name == "8e307":
        return 0.0, 0.0
    if kind == "diagonal":
        return (float(1 / sum(Fraction(1, d) for d in range(1, args[0] + 1))),) * 2
    if kind == "block":
        r = solve(block_base(args[0], args[2]))
        return r["lo"], r["hi"]
    return None


def value_margin(A):
    """How far outside a computed [lo, hi] a game's value may lie.  lo and hi are sequential sums of at most max(n_a, n_b)
    rounded products, each sum wrong by at most n * 2^-53 * max|A|: (n_a + n_b) * 2^-52 * max(1, max|A|) bounds it (identity
    64 gives lo - 1/64 = 3.5e-18).  Derived, not measured."""
    return (A.shape[0] + A.shape[1]) * 2.0 ** -52 * max(1.0, float(np.abs(A).max()))


def small_games(n=257):
    """n distinct 3 x 4 games, uniform, integer and normal in turn: saddle points and games of 2 to 6 pivots"""
    return np.stack([family(("uniform", "integer", "normal")[g % 3], 3, 4, 3000 + g) for g in range(n)])
