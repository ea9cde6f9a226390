"""The meta-game on the device at its edges (soccer_solve_meta_games): every game of mg.EDGE_SHAPES — shapes at the thread,
wave and tile boundaries of the kernels, tie-heavy and closed-form games, numeric edges — to the bits of the numpy restatement
through every path it may take, and its known value inside the device's bracket; tie-heavy games in one batch; more than one
pass of the global path, complete and under a cap; no result depends on what the handle solved before; a range that overflows
is refused by game index."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_game_np as mg  # noqa: E402
from test_gpu_meta_game import KEYS, LDS_LIMIT, paths, row, same  # noqa: E402

pytestmark = pytest.mark.gpu

_ref = {}


@pytest.fixture(scope="module")
def batch():
    b = SoccerBatch(1, 5, 4, 0.0)
    yield b
    b.close()


def ref(name):
    """the restatement's result on a game of mg.EDGE_SHAPES, computed once"""
    if name not in _ref:
        _ref[name] = mg.solve(mg.edge(name))
    return _ref[name]


def small_ref(cap=None):
    """the restatement on the 257 small games, computed once per cap"""
    if ("small", cap) not in _ref:
        _ref[("small", cap)] = mg.solve_batch(mg.small_games(), cap)
    return _ref[("small", cap)]


def tiled(want, n):
    """the results of a batch that repeats the games of `want` in order up to n games"""
    idx = np.arange(n) % want["status"].shape[0]
    return {k: want[k][idx] for k in KEYS}


# ---- 1. bits against the restatement, every edge through every path it may take -------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in mg.EDGE_SHAPES])
def test_bits_against_the_restatement(batch, name):
    A = mg.edge(name)
    want = ref(name)
    known = mg.known_value(name)
    m = mg.value_margin(A)
    for path in paths(*A.shape):
        got = batch.solve_meta_game(A, path=path)
        print("%s through path %d: %d pivots (%d ties in the restatement, %d decided by the shadow quotient), status %d, lo %r, hi %r, hi - lo = %.3g" % (
            name, path, got["pivots"], want["ties"], want["decided"], got["status"], got["lo"], got["hi"], got["hi"] - got["lo"]))
        same(got, want, "%s through path %d" % (name, path))
        assert got["status"] in (0, 1)
        if known is not None:
            assert got["lo"] - m <= known[0] and known[1] <= got["hi"] + m
    if name == "minus-zeros":
        assert np.signbit(got["value"]) and np.signbit(got["lo"]) and np.signbit(got["hi"])


# ---- 2. the tie-heavy games in one batch -----------------------------------------------------------------------------------
def test_tie_heavy_games_in_one_batch(batch):
    """ties in half the ratio tests, none, and ties of another kind side by side: the reductions of one workgroup (the LDS
    kernel at the largest square it takes) and of a grid's blocks (the global kernels) do not mix games"""
    A = np.stack([mg.edge("cyclic-99"), mg.edge("identity-99"), mg.family("uniform", 99, 99, 71), mg.edge("shuffled-cyclic-99")])
    assert mg.lds_bytes(99, 99) <= LDS_LIMIT < mg.lds_bytes(100, 100)
    want = mg.solve_batch(A)
    assert want["ties"][0] >= 47 and want["across"][3] > 0 and (want["status"] == 0).all()
    same(batch.solve_meta_game(A, path=1), want, "cyclic 99, identity 99, uniform and shuffled cyclic 99 x 99 through path 1")
    B = np.stack([mg.edge("cyclic-101"), mg.padded_identity(100), mg.family("uniform", 101, 101, 72), mg.shuffled_cyclic(101, 2)])
    want = mg.solve_batch(B)
    assert want["ties"][0] >= 48 and want["across"][3] > 0 and (want["status"] == 0).all()
    m = mg.value_margin(B[1])
    assert want["lo"][1] - m <= 0.01 <= want["hi"][1] + m               # the dominated row and column change nothing
    got = batch.solve_meta_game(B, path=2)
    same(got, want, "cyclic 101, identity 100 padded, uniform and shuffled cyclic 101 x 101 through path 2")
    assert got["x"][1][100] == 0.0 and got["y"][1][100] == 0.0


# ---- 3. passes on the global path ------------------------------------------------------------------------------------------
def test_passes_on_the_global_path(batch):
    """32 768 games are one pass of the global path (grid.y is the game): three more make a second, ragged one, with its
    own count of open games, its own offsets into the outputs and its share of the capped games"""
    base = mg.small_games()
    n = 32768 + 3
    assert np.unique(base.reshape(257, -1), axis=0).shape[0] == 257, "257 distinct games"
    want = small_ref()
    assert (want["status"] <= 1).all() and (want["pivots"] == 0).sum() >= 40 and want["pivots"].max() >= 5
    A = base[np.arange(n) % 257]
    same(batch.solve_meta_game(A, path=2), tiled(want, n), "32 768 + 3 games of 3 x 4 through path 2")
    capped = tiled(small_ref(2), n)
    stopped = int((capped["status"] == 3).sum())
    assert (capped["status"][-3:] == 3).any() and (capped["status"][:32768] == 3).any(), "both passes hold capped games"
    with pytest.raises(RuntimeError, match="%d of %d games stopped at max_pivots = 2" % (stopped, n)) as e:
        batch.solve_meta_game(A, max_pivots=2, path=2)
    same(e.value.results, capped, "the capped batch of 32 768 + 3 games")


# ---- 4. no result depends on earlier calls ---------------------------------------------------------------------------------
def test_no_result_depends_on_what_the_handle_solved_before():
    """the buffers only grow and the records, counts and statuses are carved out of one of them at offsets that depend on
    the games of a pass: a small call after a large one, on either path, returns a fresh handle's bits"""
    small = mg.small_games()
    one = small[129]
    assert small_ref()["pivots"][129] >= 3
    want_one = {k: small_ref()[k][129] for k in KEYS}
    fresh = {}
    for path in (1, 2):
        b = SoccerBatch(1, 5, 4, 0.0)
        fresh[path] = b.solve_meta_game(one, path=path)
        b.close()
    b = SoccerBatch(1, 5, 4, 0.0)
    first = b.solve_meta_game(one, path=1)
    same(first, want_one, "3 x 4 through path 1, the handle's first call")
    same(first, fresh[1], "3 x 4 through path 1 against a fresh handle")
    same(b.solve_meta_game(mg.edge("257x257-integer"), path=2), ref("257x257-integer"), "257 x 257 through path 2")
    same(b.solve_meta_game(small[np.arange(2048) % 257], path=2), tiled(small_ref(), 2048), "2 048 games of 3 x 4 through path 2")
    same(b.solve_meta_game(mg.edge("2x1024"), path=1), ref("2x1024"), "2 x 1024 through path 1")
    fifth = b.solve_meta_game(one, path=2)
    same(fifth, want_one, "one 3 x 4 game through path 2 after the larger calls")
    same(fifth, fresh[2], "one 3 x 4 game through path 2 against a fresh handle")
    same(b.solve_meta_game(mg.edge("cyclic-99"), path=1), ref("cyclic-99"), "99 x 99 through path 1")
    b.close()


# ---- 5. a range that overflows ---------------------------------------------------------------------------------------------
def test_a_range_that_overflows_is_refused_by_game_index(batch):
    ok = np.array(mg.LITERALS["8e307"])
    B = np.stack([ok, mg.OVERFLOWING, ok])
    assert np.isfinite(B).all()
    for path in (0, 1, 2):
        with pytest.raises(AssertionError, match=r"A\[game 1\]: max A - min A is not finite"):
            batch.solve_meta_game(B, path=path)
    with pytest.raises(AssertionError, match=r"A\[game 0\]: max A - min A is not finite"):
        batch.solve_meta_game(np.array([[1e308, -1e308]]))              # a saddle point, refused all the same
    want = ref("8e307")
    got = batch.solve_meta_game(np.stack([ok, ok, ok]))
    for g in range(3):
        same(row(got, g), want, "game %d of the call after the refusal" % g)
