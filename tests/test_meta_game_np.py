"""Where there is no GPU: soccer_solve_meta_games is part of the C ABI and checks its handle first, and the numpy restatement
of its definition (tests/meta_game_np.py), which tests/test_gpu_meta_game.py pins the device to bit for bit, solves games:
known ones exactly, 5 x 5 ones like the host build of soccer_games.hpp, larger ones like scipy's HiGHS, and under a pivot cap
it stops where it is told with a bracket that still holds."""
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
