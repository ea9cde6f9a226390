"""The meta-game on the device (soccer_solve_meta_games): every output to the bits of the numpy restatement
(tests/meta_game_np.py) through the LDS kernel and the global kernels; no result depends on the path, on pivots_per_sync, on
the batch a game is in or on the pass it falls into; the fit rule of the LDS kernel; the pivot cap; the refusals; no tick and
the lanes left alone; planners.meta_game and the three populations; and one 1024 x 1024 game whose certificate is checked."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv, core
from gym_soccer_littman94_amd import planners as pl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_game_np as mg  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_LIMIT = 163840                  # what a workgroup may be given on gfx950
KEYS = ("x", "y", "value", "lo", "hi", "pivots", "status")
_ref = {}


@pytest.fixture(scope="module")
def batch():
    b = SoccerBatch(1, 5, 4, 0.0)
    yield b
    b.close()


def ref(name, cap=None):
    """the restatement's result on a game of mg.SHAPES, computed once"""
    if (name, cap) not in _ref:
        _ref[(name, cap)] = mg.solve(mg.shape(name), cap)
    return _ref[(name, cap)]


def same(got, want, what):
    """bit for bit: got is solve_meta_game's dict (or row g of a batch's), want the restatement's"""
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, "%s of %s: shape %s, not %s" % (k, what, a.shape, b.shape)
        if a.dtype.kind == "f":
            a, b = a.view(np.int64), b.astype(np.float64).view(np.int64)
        assert np.array_equal(a, b), "%s of %s differs: %s, not %s" % (k, what, got[k], want[k])


def row(out, g):
    return {k: out[k][g] for k in KEYS}


def paths(n_a, n_b):
    return (0, 1, 2) if mg.lds_bytes(n_a, n_b) <= LDS_LIMIT else (0, 2)


def saddle_game(rng, n_a, n_b):
    """no pivots: a random matrix with a saddle point made at a random place"""
    A = rng.uniform(-1, 1, (n_a, n_b))
    i, j = rng.integers(0, n_a), rng.integers(0, n_b)
    A[i, :] = np.abs(A[i, :]) + 0.5; A[:, j] = -np.abs(A[:, j]) - 0.5; A[i, j] = 0.25
    return A


def short_game(rng, n_a, n_b):
    """two pivots: a 2 x 2 game without a saddle point; every other row is dominated, every other column too"""
    A = np.full((n_a, n_b), 5.0)
    A[2:, :] = -5.0
    A[:2, :2] = np.array([[1.0, -1.0], [-1.0, 1.0]]) * rng.uniform(0.5, 1.0, (2, 2))
    return A


def mixed_games(n_games, n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    kinds = [lambda: saddle_game(rng, n_a, n_b), lambda: rng.uniform(-1, 1, (n_a, n_b)), lambda: short_game(rng, n_a, n_b),
             lambda: rng.integers(-1, 2, (n_a, n_b)).astype(np.float64), lambda: np.full((n_a, n_b), 0.5)]
    return np.stack([kinds[g % 5]() for g in range(n_games)])


# ---- 1. bits against the restatement, every shape through every path it may take -----------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in mg.SHAPES])
def test_bits_against_the_restatement(batch, name):
    A = mg.shape(name)
    want = ref(name)
    for path in paths(*A.shape):
        got = batch.solve_meta_game(A, path=path)
        same(got, want, "%s through path %d" % (name, path))
        assert got["gap"] == got["hi"] - got["lo"] and bool(got["certified"]) == (want["status"] <= 1)
    print("%s: %d pivots, status %d, hi - lo = %.3g, %d ties" % (name, want["pivots"], want["status"], want["hi"] - want["lo"],
                                                                  want["ties"]))
    assert want["status"] in (0, 1)


def test_the_fit_rule_of_the_lds_kernel(batch):
    n = max(k for k in range(1, 200) if core.meta_lds_bytes(k, k) <= LDS_LIMIT)
    assert n == 99 and core.meta_lds_bytes(n, n) == mg.lds_bytes(n, n)
    A = mg.family("uniform", n, n, 71)
    same(batch.solve_meta_game(A, path=1), mg.solve(A), "the largest square game of the LDS kernel")
    B = mg.family("uniform", n + 1, n + 1, 72)
    with pytest.raises(AssertionError, match="100 x 100 game does not fit"):
        batch.solve_meta_game(B, path=1)
    want = mg.solve(B)
    same(batch.solve_meta_game(B, path=0), want, "100 x 100 with the library's choice")
    same(batch.solve_meta_game(B, path=2), want, "100 x 100 through the global kernels")


def test_no_result_depends_on_pivots_per_sync(batch):
    want = ref("130x70-integer")
    assert want["pivots"] > 64                                          # more than one batch: the loop continues, and ends early
    for pps in (1, 3, 16, 0):
        same(batch.solve_meta_game(mg.shape("130x70-integer"), path=2, pivots_per_sync=pps), want, "pivots_per_sync %d" % pps)


# ---- 2. batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_games,n_a,n_b", [(1, 8, 8), (3, 8, 8), (257, 8, 8), (5, 130, 70)])
def test_a_game_of_a_batch_is_the_game_alone(batch, n_games, n_a, n_b):
    A = mixed_games(n_games, n_a, n_b, 100 + n_games)
    want = mg.solve_batch(A)
    if n_games >= 5:
        piv = want["pivots"]
        assert (piv == 0).any() and (piv == 2).any() and (piv >= 5).any(), "saddle points, short games and long ones"
    for path in paths(n_a, n_b):
        got = batch.solve_meta_game(A, path=path)
        assert got["x"].shape == (n_games, n_a) and got["y"].shape == (n_games, n_b) and got["pivots"].dtype == np.int32
        same(got, want, "%d games of %d x %d through path %d" % (n_games, n_a, n_b, path))
        for g in sorted({0, n_games // 2, n_games - 1}):
            same(batch.solve_meta_game(A[g], path=path), row(got, g), "game %d alone through path %d" % (g, path))


@pytest.mark.parametrize("n_a,n_b,cap", [(130, 70, 40), (40, 50, 10)])
def test_a_batch_under_a_cap_closes_its_games_at_different_pivots(batch, n_a, n_b, cap):
    A = mixed_games(5, n_a, n_b, 105)
    want = mg.solve_batch(A, cap)
    assert want["status"].tolist() == [1, 3, 0, 3, 1] and want["pivots"].tolist() == [0, cap, 2, cap, 0]
    for path in paths(n_a, n_b):
        with pytest.raises(RuntimeError, match="2 of 5 games stopped at max_pivots = %d" % cap) as e:
            batch.solve_meta_game(A, max_pivots=cap, path=path, pivots_per_sync=16)
        same(e.value.results, want, "the capped batch through path %d" % path)


def test_2048_games_of_64_x_64(batch):
    base = np.stack([mg.family(k, 64, 64, 200 + i) for i, k in enumerate(("uniform", "integer", "normal", "antisymmetric"))])
    want = mg.solve_batch(base)
    A = np.tile(base, (512, 1, 1))
    got = batch.solve_meta_game(A)
    same(got, {k: np.tile(want[k], (512,) + (1,) * (want[k].ndim - 1)) for k in KEYS}, "2048 games of 64 x 64")


def test_games_beyond_one_pass(batch):
    """the LDS path solves at most 2**20 games in a pass: 1 x 2 games, each a saddle point at the smaller entry"""
    n = (1 << 20) + 3
    A = np.random.default_rng(9).integers(-3, 4, (n, 1, 2)).astype(np.float64)
    got = batch.solve_meta_game(A)
    v = A[:, 0, :].min(1)
    assert (got["status"] == 1).all() and (got["pivots"] == 0).all() and (got["x"] == 1.0).all()
    assert np.array_equal(got["value"], v) and np.array_equal(got["lo"], v) and np.array_equal(got["hi"], v)
    assert np.array_equal(got["y"][:, 1], (A[:, 0, 1] < A[:, 0, 0]).astype(np.float64)) and (got["y"].sum(1) == 1.0).all()


# ---- 3. the pivot cap --------------------------------------------------------------------------------------------------------
def test_the_cap_returns_the_last_iterate(batch):
    A = mg.shape("63x65")
    need = ref("63x65")["pivots"]
    for cap in (1, need - 1):
        want = mg.solve(A, cap)
        assert want["status"] == 3 and want["pivots"] == cap
        for path in (1, 2):
            with pytest.raises(RuntimeError, match="1 of 1 games stopped at max_pivots = %d" % cap) as e:
                batch.solve_meta_game(A, max_pivots=cap, path=path)
            same(e.value.results, want, "cap %d through path %d" % (cap, path))
    for path in (1, 2):
        same(batch.solve_meta_game(A, max_pivots=need, path=path), ref("63x65"), "a cap of exactly the pivots needed")
    # in a batch the other games are complete
    rng = np.random.default_rng(4)
    B = np.stack([saddle_game(rng, 63, 65), A, short_game(rng, 63, 65)])
    want = mg.solve_batch(B, need - 1)
    assert want["status"].tolist() == [1, 3, 0]
    for path in (1, 2):
        with pytest.raises(RuntimeError, match="1 of 3 games stopped") as e:
            batch.solve_meta_game(B, max_pivots=need - 1, path=path)
        same(e.value.results, want, "the batch with one capped game through path %d" % path)


# ---- 4. refusals and side effects ----------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(batch):
    A = mg.family("uniform", 4, 6, 1)
    for shape in ((0, 3), (1025, 2), (2, 0), (2, 1025)):
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and %d" % shape):
            batch.solve_meta_game(np.zeros(shape))
    for bad in (float("nan"), float("inf"), -float("inf")):
        B = np.stack([A, A, A])
        B[1, 2, 3] = bad
        with pytest.raises(AssertionError, match=r"A\[game 1\]\[row 2\]\[column 3\] is not finite"):
            batch.solve_meta_game(B)
    with pytest.raises(AssertionError, match="path must be 0 .* not 3"):
        batch.solve_meta_game(A, path=3)
    with pytest.raises(AssertionError, match="pivots_per_sync must be >= 0"):
        batch.solve_meta_game(A, pivots_per_sync=-1)
    with pytest.raises(AssertionError, match="max_pivots must be >= 1"):
        batch.solve_meta_game(A, max_pivots=0)
    assert batch.solve_meta_game(np.zeros((0, 4, 6)))["value"].shape == (0,)        # no games: nothing to do
    same(batch.solve_meta_game(A), mg.solve(A), "a call after the refusals")


def test_capture_no_ticks_and_the_lanes_are_left_alone():
    A = mg.shape("63x65")
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.reset()
    n = 64
    a = b.alloc(n, np.int8).fill(0); c = b.alloc(n, np.int8).fill(1)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    b.graph_begin()
    b.step_plain(a, c, obs, rew, term, trunc)
    with pytest.raises(RuntimeError, match="graph capture"):
        b.solve_meta_game(A)
    b.graph_destroy(b.graph_end())
    b.close()
    # a completed, a capped and a refused call consume no tick and leave the lanes alone, on a two-player handle and on one
    # whose player B follows a fixed policy: the tick and the lanes' state before and after
    for fixed in (False, True):
        env = VectorSoccerEnv(4096, slip_prob=0.2, seed=3, player_b_policy=[1] * 761 if fixed else None)
        env.reset()
        tick, state = env.batch.tick, env.batch.get_state()
        what = "a fixed-policy handle" if fixed else "a two-player handle"
        for path in (1, 2):
            same(env.solve_meta_game(A, path=path), ref("63x65"), "a solve on %s" % what)
        with pytest.raises(RuntimeError, match="stopped at max_pivots"):
            env.solve_meta_game(A, max_pivots=3)
        with pytest.raises(AssertionError, match="path must be"):
            env.solve_meta_game(A, path=7)
        assert env.batch.tick == tick
        after = env.batch.get_state()
        for k in state:
            np.testing.assert_array_equal(after[k], state[k])
        env.close()
    # and what follows is what would have followed: the same two-player rollout with and without a solve before it
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(4096, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            env.solve_meta_game(A)
        O, R, TE, TR, _ = env.rollout(50, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------
def test_planners_meta_game_is_cross_play_then_the_solve():
    from test_gpu_cross_play import sets
    GAMMA, THETA = 0.9, 1e-10
    A, B = sets(5, 4, 0.2, 3, 5)
    b = SoccerBatch(1, 5, 4, 0.2)
    got = pl.meta_game(b, A, B, THETA, GAMMA)
    cp = pl.cross_play(b, A, B, THETA, GAMMA)
    m = b.solve_meta_game(cp["payoff"])
    for k in ("payoff", "iterations", "row_min", "col_max"):
        assert np.array_equal(got[k], cp[k])
    assert got["bounds"] == cp["bounds"]
    for k in ("x", "y", "value", "lo", "hi", "status"):
        assert np.array_equal(got[k], m[k])
    same(m, mg.solve(cp["payoff"]), "the 3 x 5 meta-game")
    eps = mg.eps_of(cp["payoff"])
    print("bounds %r, lo %r, hi %r, gain %r, status %d, x %s" % (cp["bounds"], got["lo"], got["hi"], got["gain"], got["status"], got["x"]))
    assert got["lo"] >= cp["bounds"][0] - eps and got["hi"] <= cp["bounds"][1] + eps and got["status"] in (0, 1)
    assert got["gain"] == got["lo"] - cp["bounds"][0]
    acc = np.zeros(5)                                                   # x's mixture row by hand
    for i in range(3):
        acc = acc + got["x"][i] * cp["payoff"][i]
    assert acc.min() == got["lo"] and abs((got["x"] @ cp["payoff"]).min() - got["lo"]) <= 1e-15
    b.close()


@pytest.mark.parametrize("kind", ["q", "wolf", "minimax_q"])
def test_a_population_s_meta_game_is_the_planner_s_on_what_read_returns(kind):
    n, GAMMA, THETA = 8, 0.9, 1e-10
    make = {"q": lambda b, g: b.q_population(g), "wolf": lambda b, g: b.wolf_population(g),
            "minimax_q": lambda b, g: b.minimax_q_population(g)}[kind]
    b = SoccerBatch(n, 5, 4, 0.2, seed=7, autoreset=True)
    pop = make(b, GAMMA)
    b.reset(); pop.run(300)
    r = pop.read()

    def check(got, want):
        assert sorted(got) == sorted(want) and got["payoff"].shape == (n, n) and got["x"].shape == (n,)
        for k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k

    check(pop.meta_game(), pl.meta_game(b, r["pi_a"], r["pi_b"], THETA, GAMMA))
    if kind == "wolf":
        check(pop.meta_game("avg"), pl.meta_game(b, r["avg_a"], r["avg_b"], THETA, GAMMA))
    part = pop.meta_game(first=1, count=3, discount_factor=0.5, theta=1e-8)
    want = pl.meta_game(b, r["pi_a"][1:4], r["pi_b"][1:4], 1e-8, 0.5)
    assert np.array_equal(part["payoff"], want["payoff"]) and np.array_equal(part["x"], want["x"]) and part["lo"] == want["lo"]
    pop.close(); b.close()


# ---- 6. one large game ---------------------------------------------------------------------------------------------------------
HIGHS_VALUE_1024 = 1.0266165402552101e-07      # scipy.optimize.linprog(method="highs") on mg.large_game(), 13 s on a CPU


def test_one_1024_x_1024_game(batch):
    """A rank-3 product plus 1e-3 uniform noise through path=0 (the global kernels).  Not compared with the restatement, which
    takes about a minute on this input; its certificate is: the bracket is what numpy's products of x and y give, and the
    game's value from scipy's HiGHS (computed beforehand on the same matrix, HIGHS_VALUE_1024) lies inside it."""
    A = mg.large_game()
    got = batch.solve_meta_game(A)
    print("1024 x 1024: %d pivots, status %d, lo %r, hi %r, gap %.3g" % (got["pivots"], got["status"], got["lo"], got["hi"], got["gap"]))
    scale = max(1.0, float(np.abs(A).max()))
    assert (got["x"] >= 0).all() and (got["y"] >= 0).all() and abs(got["x"].sum() - 1) <= 1e-12 and abs(got["y"].sum() - 1) <= 1e-12
    assert abs((got["x"] @ A).min() - got["lo"]) <= 1e-12 * scale and abs((A @ got["y"]).max() - got["hi"]) <= 1e-12 * scale
    m = 1e-7 * scale
    assert got["lo"] - m <= HIGHS_VALUE_1024 <= got["hi"] + m
    assert got["status"] in (0, 2) and 0 < got["pivots"] < 100 * 2048
