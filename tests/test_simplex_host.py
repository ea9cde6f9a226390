"""CPU: the simplex projection of gradient play (csrc/soccer_simplex.hpp, the header the device's step kernel includes) run by a
stand-alone host program (tests/host/simplex_host.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer) against
tests/policy_gradient_np.py's project bit for bit: random rows, ties, rows far outside the simplex, and both zeros."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_gradient_np as pgn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("simplex_host")), "simplex_host")
    # the sanitizers' runtimes are linked statically: the program runs as it is, with nothing preloaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "simplex_host.cpp")])
    return exe


def run(host, tmp_path, rows):
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 5)
    path = os.path.join(str(tmp_path), "rows.txt")
    with open(path, "w") as f:
        f.write("%d\n" % rows.shape[0])
        f.write("\n".join(" ".join(str(int(b)) for b in r) for r in rows.view(np.uint64)) + "\n")
    # (the leak check at exit needs ptrace, which a container may withhold; the checks of every access stay on)
    p = subprocess.run([host, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stderr
    return np.array(p.stdout.split(), dtype=np.uint64).reshape(-1, 5)


def same(host, tmp_path, rows, what):
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    got = run(host, tmp_path, rows)
    want = pgn.project(rows).view(np.uint64)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, "%s: %d of %d rows differ, the first %s -> %s, numpy %s" % (
        what, bad.size, rows.shape[0], rows[bad[0]].tolist(), got[bad[0]].view(np.float64).tolist(), want[bad[0]].view(np.float64).tolist())
    return got.view(np.float64)


def test_random_rows(host, tmp_path):
    rng = np.random.default_rng(11)
    rows = np.concatenate([rng.dirichlet(np.ones(5), 3000) + rng.uniform(-1, 1, (3000, 5)), rng.dirichlet(np.full(5, 0.3), 2000),
                           rng.normal(0, 1, (3000, 5))])
    p = same(host, tmp_path, rows, "random rows")
    assert (p >= 0).all() and np.abs(p.sum(1) - 1).max() < 1e-14


def test_ties_and_every_order_of_a_row(host, tmp_path):
    rng = np.random.default_rng(12)
    ties = np.round(rng.normal(0.2, 0.4, (3000, 5)), 1)
    same(host, tmp_path, ties, "rows with ties")
    # the sorting network sorts: every order of five distinct values, and of values with repeats, gives numpy's result
    for base in ([0.9, 0.4, 0.1, -0.3, -0.8], [0.5, 0.5, 0.2, 0.2, 0.2], [0.3, 0.3, 0.3, 0.3, -1.0], [1.0, 0.0, 0.0, 0.0, 0.0]):
        perms = np.array(sorted(set(itertools.permutations(base))))
        p = same(host, tmp_path, perms, "the orders of %s" % base)
        order = np.argsort(perms, axis=1, kind="stable")
        assert (np.take_along_axis(p, order, 1) == np.take_along_axis(p, order, 1)[0]).all()


def test_rows_far_outside_the_simplex(host, tmp_path):
    rng = np.random.default_rng(13)
    rows = np.concatenate([rng.normal(0, 1e3, (2000, 5)), rng.normal(0, 1e6, (1000, 5)), -np.abs(rng.normal(0, 50, (1000, 5))),
                           1e3 + rng.normal(0, 1e-3, (1000, 5)), [[1e20, 1.0, 0.5, -3.0, 2.0], [-1e20] * 5, [1e300, 1e300, 0, 0, 0]]])
    p = same(host, tmp_path, rows, "rows far outside")
    assert np.isfinite(p).all() and (p >= 0).all()


def test_both_zeros(host, tmp_path):
    z = [0.0, -0.0]
    rows = [list(r) for r in itertools.product(z, repeat=5)]                                  # sum 0: tau = -0.2, every entry 0.2
    rows += [[1.0] + list(r) for r in itertools.product(z, repeat=4)]                         # a vertex with zeros of either sign
    rows += [[0.5, 0.5] + list(r) for r in itertools.product(z, repeat=3)]
    rows += [[-0.0, 0.25, 0.75, 0.0, -0.0], [2.0, -0.0, 0.0, -0.0, 0.0], [-0.0, -1.0, 0.0, -2.0, -0.0]]
    p = same(host, tmp_path, rows, "zeros of either sign")
    assert not np.signbit(p).any()                                      # an entry that is not positive is +0.0
    assert (p[:32] == 0.2).all() and (p[32:48] == [1.0, 0, 0, 0, 0]).all()
