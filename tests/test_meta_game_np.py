"""Where there is no GPU: soccer_solve_meta_games is part of the C ABI and checks its handle first, and the numpy restatement
of its definition (tests/meta_game_np.py), which tests/test_gpu_meta_game.py pins the device to bit for bit, solves games:
known ones exactly, 5 x 5 ones like the host build of soccer_games.hpp, larger ones like scipy's HiGHS, and under a pivot cap
it stops where it is told with a bracket that still holds.  The edges (mg.EDGE_SHAPES: shapes at the kernels' thread and tile
boundaries, tie-heavy games, games with closed-form values, numeric edges) finish, reach the ties they are there for, bracket
their known values and scale exactly by powers of two; a range that overflows is refused.  None of that needs scipy."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib, core

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_game_np as mg  # noqa: E402
from test_matrix_game_host import build_games_host, solve_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def margin(A):
    """HiGHS's own feasibility tolerance, scaled like eps"""
    return 1e-7 * max(1.0, float(np.abs(A).max()))


def check_bracket(A, r):
    """x and y are mixtures, and the bracket is what numpy's own products of them give"""
    assert (r["x"] >= 0).all() and (r["y"] >= 0).all()
    assert abs(r["x"].sum() - 1) <= 1e-12 and abs(r["y"].sum() - 1) <= 1e-12
    tol = 1e-12 * max(1.0, float(np.abs(A).max()))
    assert abs((r["x"] @ A).min() - r["lo"]) <= tol and abs((A @ r["y"]).max() - r["hi"]) <= tol
    assert r["lo"] <= r["hi"] + tol and r["value"] == 0.5 * (r["lo"] + r["hi"])


def test_the_symbol_is_declared_exported_and_mirrored():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    assert re.search(r"\bint soccer_solve_meta_games\(", text), "soccer_solve_meta_games is not declared"
    assert "soccer_solve_meta_games" in _lib.PROTOTYPES and hasattr(lib, "soccer_solve_meta_games")
    assert int(re.search(r"#define\s+SOCCER_META_MAX_POLICIES\s+(\d+)", text).group(1)) == _lib.META_MAX_POLICIES == 1024
    assert len(_lib.PROTOTYPES["soccer_solve_meta_games"][1]) == 9
    fields = re.search(r"typedef struct soccer_meta_game_result \{(.*?)\} soccer_meta_game_result;", text, re.S).group(1)
    assert re.findall(r"\*\s+(\w+);", fields) == [n for n, _ in _lib.MetaGameResult._fields_]
    assert "soccer_solve_meta_games" in re.search(r"#define SOCCER_ABI_VERSION 3.*?\*/", text, re.S).group(0)
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    # the fit rule of the LDS kernel as the header states it: 96 x 96 is about 154 KB, 99 x 99 the largest square on gfx950
    assert core.meta_lds_bytes(96, 96) == mg.lds_bytes(96, 96) == 154168
    assert mg.lds_bytes(99, 99) <= 163840 < mg.lds_bytes(100, 100)


@pytest.mark.parametrize("n_games,n_a,n_b,cap,path,pps", [
    (1, 2, 2, 10, 0, 0), (0, 2, 2, 10, 0, 0), (1, 0, 2, 10, 0, 0), (1, 2, 1025, 10, 0, 0), (1, 2, 2, 0, 0, 0), (1, 2, 2, 10, 3, 0),
    (1, 2, 2, 10, 0, -1), (-1, 2, 2, 10, 0, 0)])
def test_the_call_rejects_a_null_handle_whatever_else_it_is_given(n_games, n_a, n_b, cap, path, pps):
    lib = _lib.load()
    A = np.array([[1.0, -1.0], [-1.0, 1.0]])
    out = {k: np.full(4, 7.0) for k in ("value", "x", "y", "lo", "hi")}
    out.update({k: np.full(4, 7, np.int32) for k in ("pivots", "status")})
    res = _lib.MetaGameResult(**{k: v.ctypes.data for k, v in out.items()})
    assert lib.soccer_solve_meta_games(None, n_games, n_a, n_b, A.ctypes.data, cap, path, pps, C.byref(res)) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    assert all((v == 7).all() for v in out.values())


def test_known_games():
    """Matching pennies and rock-paper-scissors: the mixtures 1/2 and 1/3 and the value 0, to the rounding of the definition's
    own last steps — an entry is a quotient of two tableau entries that each carry a few roundings, and the bracket is a sum
    of two or three products of them, so ULPS = 4 units of 2^-52 (the spacing of doubles below 1) bound every figure."""
    ULPS = 4 * 2.0 ** -52
    pennies = np.array([[1.0, -1.0], [-1.0, 1.0]])
    r = mg.solve(pennies)
    print("matching pennies: x %r y %r value %r lo %r hi %r" % (r["x"].tolist(), r["y"].tolist(), r["value"], r["lo"], r["hi"]))
    assert np.abs(r["x"] - 0.5).max() <= ULPS and np.abs(r["y"] - 0.5).max() <= ULPS
    assert abs(r["value"]) <= ULPS and r["status"] == 0 and r["hi"] - r["lo"] <= ULPS
    check_bracket(pennies, r)
    rps = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    r = mg.solve(rps)
    print("rock-paper-scissors: x %r y %r value %r lo %r hi %r" % (r["x"].tolist(), r["y"].tolist(), r["value"], r["lo"], r["hi"]))
    third = np.full(3, 1.0 / 3.0)
    assert np.abs(r["x"] - third).max() <= ULPS and np.abs(r["y"] - third).max() <= ULPS
    assert abs(r["value"]) <= ULPS and r["status"] == 0 and r["hi"] - r["lo"] <= ULPS
    check_bracket(rps, r)
    rng = np.random.default_rng(3)
    for A in (np.full((4, 6), 0.25), rng.standard_normal((1, 1)), rng.standard_normal((1, 7)), rng.standard_normal((7, 1))):
        r = mg.solve(A)
        assert r["status"] == 1 and r["pivots"] == 0 and r["lo"] == r["hi"] == r["value"]
        i, j = int(np.argmax(r["x"])), int(np.argmax(r["y"]))
        assert r["x"].sum() == 1.0 and r["y"].sum() == 1.0 and r["x"][i] == 1.0 and r["y"][j] == 1.0
        assert r["value"] == A[i, j] == A.min(1).max() == A.max(0).min()
    # two equal saddle rows and two equal saddle columns: the first of each
    A = np.array([[0.0, -1.0, 3.0, -2.0], [2.0, 1.0, 4.0, 1.0], [2.0, 1.0, 5.0, 1.0]])
    r = mg.solve(A)
    assert r["status"] == 1 and r["x"].tolist() == [0, 1, 0] and r["y"].tolist() == [0, 1, 0, 0] and r["value"] == 1.0


def test_against_the_host_build_of_the_5x5_solver(tmp_path):
    host = build_games_host(tmp_path)
    rng = np.random.default_rng(55)
    A = np.concatenate([rng.uniform(-1, 1, (120, 5, 5)), rng.integers(-2, 3, (80, 5, 5)).astype(np.float64)])
    v, x, y, _ = solve_host(host, A)
    worst = 0.0
    for g in range(A.shape[0]):
        r = mg.solve(A[g])
        eps = mg.eps_of(A[g])
        check_bracket(A[g], r)
        assert r["status"] in (0, 1) and r["hi"] - r["lo"] <= eps
        assert abs(r["value"] - v[g]) <= 2 * eps                        # each within its own eps of the game's value
        lo_h, hi_h = (x[g] @ A[g]).min(), (A[g] @ y[g]).max()           # the host's bracket is valid too, and the two overlap
        assert hi_h - lo_h <= eps + 1e-15 and lo_h <= r["hi"] + 1e-15 and r["lo"] <= hi_h + 1e-15
        worst = max(worst, abs(r["value"] - v[g]) / eps)
    print("200 games: max |value - host value| = %.3g eps" % worst)


HIGHS = [(kind, n_a, n_b, seed) for _, kind, n_a, n_b, seed in mg.SHAPES] + [
    ("normal", 30, 40, 31), ("uniform", 130, 70, 32), ("integer", 64, 64, 33), ("integer", 8, 8, 34), ("antisymmetric", 33, 33, 35),
    ("antisymmetric", 100, 100, 36), ("duplicated", 130, 70, 37), ("rank1", 20, 30, 38), ("rank1c", 70, 130, 39),
    ("rank2", 50, 50, 40), ("rank2c", 64, 65, 41), ("rank3", 100, 90, 42), ("rank4", 130, 70, 43), ("rank4c", 30, 130, 44),
    ("rank5", 70, 70, 45), ("rank5c", 130, 70, 46)]


@pytest.mark.parametrize("kind,n_a,n_b,seed", HIGHS, ids=["%s-%dx%d" % c[:3] for c in HIGHS])
def test_against_highs(kind, n_a, n_b, seed):
    pytest.importorskip("scipy")
    A = mg.family(kind, n_a, n_b, seed)
    r = mg.solve(A)
    ref = mg.highs_value(A)
    print("%s %dx%d: %d pivots, status %d, hi - lo = %.3g, %d ties, value - HiGHS = %.3g" % (
        kind, A.shape[0], A.shape[1], r["pivots"], r["status"], r["hi"] - r["lo"], r["ties"], r["value"] - ref))
    check_bracket(A, r)
    m = margin(A)
    assert r["lo"] - m <= ref <= r["hi"] + m
    assert r["status"] in (0, 1)
    assert r["pivots"] <= 100 * (A.shape[0] + A.shape[1])


def test_ratio_tests_with_ties_are_among_the_shapes():
    """the restatement counts the ratio tests in which more than one row attains the smallest true quotient, where the shadow
    column decides: integer entries and duplicated policies have them, and those inputs are in SHAPES for the GPU as well"""
    ties = {name: mg.solve(mg.shape(name))["ties"] for name in ("130x70-integer", "45x37-duplicated", "100x90-rank3c", "63x65")}
    print(ties)
    assert ties["130x70-integer"] >= 10 and ties["45x37-duplicated"] >= 1 and ties["100x90-rank3c"] >= 1 and ties["63x65"] == 0


def test_the_pivot_cap():
    A = mg.family("uniform", 20, 30, 77)
    full = mg.solve(A)
    ref = mg.highs_value(A) if pytest.importorskip("scipy") else None
    need = full["pivots"]
    assert need > 3 and full["status"] == 0
    for cap in (1, 2, need - 1):
        r = mg.solve(A, cap)
        assert r["status"] == 3 and r["pivots"] == cap
        check_bracket(A, r)
        assert r["lo"] - margin(A) <= ref <= r["hi"] + margin(A)
        assert r["hi"] - r["lo"] > mg.eps_of(A)
    r = mg.solve(A, need)
    assert r["status"] == 0 and r["pivots"] == need
    assert all(np.array_equal(r[k], full[k]) for k in ("x", "y", "value", "lo", "hi"))


# ---- the edges: what tests/test_gpu_meta_game_edges.py holds the device to, checked here for what it computes -------------
_edge = {}


def edge_ref(name):
    if name not in _edge:
        _edge[name] = mg.solve(mg.edge(name))
    return _edge[name]


def test_the_edge_list_holds_what_it_is_there_for():
    """the boundary shapes by their strides and rows, the fit rule as the list assumes it, and the families' sizes"""
    shapes = {name: mg.edge(name).shape for name, _, _ in mg.EDGE_SHAPES}
    assert len(shapes) == len(mg.EDGE_SHAPES), "a name twice"
    stride = {name: (a + b + 2) | 1 for name, (a, b) in shapes.items()}
    assert stride["15x238"] == 255 and stride["16x238"] == 257 and stride["127x127"] == 257 and stride["128x128"] == 259
    assert stride["17x494"] == stride["494x17"] == 513
    for n in (255, 256, 257):
        assert shapes["%dx2" % n] == (n, 2) and shapes["2x%d" % n] == (2, n)
    assert shapes["257x257-integer"] == (257, 257) and shapes["1024x2"] == (1024, 2) and shapes["3x1024"] == (3, 1024)
    assert shapes["1x1024"] == (1, 1024) and shapes["1024x1"] == (1024, 1)
    assert mg.lds_bytes(2, 1024) == 33088 and mg.lds_bytes(3, 1024) == 41332
    LIMIT = 163840
    fit = {name for name, (a, b) in shapes.items() if mg.lds_bytes(a, b) <= LIMIT}
    for name in ("15x238", "16x238", "2x255", "2x256", "2x257", "17x494", "2x1024", "3x1024", "1x1024", "identity-99", "cyclic-99"):
        assert name in fit, name
    for name in ("127x127", "128x128", "255x2", "256x2", "257x2", "257x257-integer", "494x17", "1024x2", "1024x3", "1024x1",
                 "identity-100", "cyclic-101", "block-5x20"):
        assert name not in fit, name
    for n in (3, 64, 99, 100, 257):
        assert shapes["identity-%d" % n] == (n, n)
    for n in (5, 63, 99, 101, 255):
        A = mg.edge("cyclic-%d" % n)
        assert A.shape == (n, n) and np.array_equal(A, -A.T) and (np.abs(A).sum(1) == n - 1).all()
    for n in (99, 255):
        A = mg.edge("shuffled-cyclic-%d" % n)
        assert A.shape == (n, n) and (np.abs(A).sum(1) == n - 1).all() and (A.sum(0) == 0).all() and (A.sum(1) == 0).all()
    assert shapes["diagonal-40"] == (40, 40) and shapes["block-6x10"] == (60, 60) and shapes["block-5x20"] == (100, 100)
    for m, seed in ((6, 100), (5, 127)):
        assert np.abs(mg.block_base(m, seed)).max() <= 2 and mg.solve(mg.block_base(m, seed))["pivots"] > 0


@pytest.mark.parametrize("name", [s[0] for s in mg.EDGE_SHAPES])
def test_an_edge_game_finishes_with_mixtures_and_brackets_its_known_value(name):
    A = mg.edge(name)
    r = edge_ref(name)
    known = mg.known_value(name)
    print("%s: %d pivots, %d ties, status %d, lo %r, hi %r, known %r" % (name, r["pivots"], r["ties"], r["status"], r["lo"], r["hi"], known))
    assert r["status"] in (0, 1)
    assert (r["x"] >= 0).all() and (r["y"] >= 0).all() and abs(r["x"].sum() - 1) <= 1e-12 and abs(r["y"].sum() - 1) <= 1e-12
    kind = next(s[1] for s in mg.EDGE_SHAPES if s[0] == name)
    if kind == "cyclic":
        assert r["ties"] >= A.shape[0] // 2 - 2
    if kind == "block":
        assert r["ties"] == r["pivots"] > 0
    if name == "257x257-integer":
        assert r["ties"] > 0
    # in cyclic and block games the shadow quotient orders the tied rows as their indices do; these are the games in which it
    # decides against the index, within a wave and across waves: a reduction that dropped or mixed up the middle key differs
    if name in ("128x128", "257x257-integer", "shuffled-cyclic-99", "shuffled-cyclic-255"):
        assert r["decided"] > r["across"] > 0 and r["ties"] >= r["decided"]
    if known is not None:
        m = mg.value_margin(A)
        assert r["lo"] - m <= known[0] and known[1] <= r["hi"] + m
    else:
        assert kind not in ("identity", "cyclic", "shuffled-cyclic", "diagonal", "block")


def test_the_saddle_point_of_minus_zeros_returns_minus_zero():
    r = edge_ref("minus-zeros")
    assert r["status"] == 1 and r["pivots"] == 0
    for k in ("value", "lo", "hi"):
        assert r[k] == 0.0 and np.signbit(r[k]), k


@pytest.mark.parametrize("k", mg.SCALES)
def test_a_power_of_two_scales_the_bracket_and_nothing_else(k):
    """(A - min A) / range is the same tableau to the bit, so are the pivots and the mixtures; lo and hi are sums of products
    with A and scale exactly; both branches of eps = 1e-10 * max(1, max|A|) are taken"""
    one, r = edge_ref("7x9"), edge_ref("7x9*2^%d" % k)
    assert np.array_equal(mg.edge("7x9*2^%d" % k), np.ldexp(mg.edge("7x9"), k)) and one["pivots"] > 0
    assert r["pivots"] == one["pivots"] and r["status"] == one["status"] == 0
    assert np.array_equal(r["x"], one["x"]) and np.array_equal(r["y"], one["y"])
    assert r["lo"] == np.ldexp(one["lo"], k) and r["hi"] == np.ldexp(one["hi"], k)
    assert (mg.eps_of(mg.edge("7x9*2^%d" % k)) == 1e-10) == (k < 0)


def test_a_range_that_overflows_is_refused():
    """finite entries whose max - min is inf would put inf / inf = NaN into the tableau; the largest range that works stays"""
    assert np.isfinite(mg.OVERFLOWING).all()
    with pytest.raises(ValueError, match="max A - min A is not finite"):
        mg.solve(mg.OVERFLOWING)
    with pytest.raises(ValueError, match="max A - min A is not finite"):
        mg.solve(np.array([[1e308, -1e308]]))                           # a saddle point, refused all the same
    with pytest.raises(ValueError, match="max A - min A is not finite"):
        mg.solve_batch(np.stack([np.eye(2), mg.OVERFLOWING, np.eye(2)]))
    r = edge_ref("8e307")
    assert r["pivots"] == 2 and r["status"] == 0
