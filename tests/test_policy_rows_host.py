"""CPU: the compiled host checks of the learners (csrc/soccer_policy_rows.hpp through tests/host/policy_rows_host.cpp): a
fixed policy's threshold rows against SoccerBatch.mixed_policy_thresholds bit for bit, the row check at its bound
1e-8 + 1e-5 and at its first bad place, and the Q-bounds check with its unread row 0.

tests/golden/threshold_draws.json does not apply here: it records Philox draws next to the integer thresholds of the slip
lists (tests/test_host_logic.py reads it), and holds no policy row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("policy_rows_host")), "libpolicy_rows_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "host", "policy_rows_host.cpp")])
    L = C.CDLL(so)
    L.policy_rows_check_host.restype = C.c_int
    L.policy_rows_check_host.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.fixed_thresholds_host.restype = C.c_int
    L.fixed_thresholds_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.q_bounds_check_host.restype = C.c_long
    L.q_bounds_check_host.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long]
    return L


def thresholds(host, rows):
    """(uint16[nS, 4], None) of the header, or (None, (state, action)) where it refuses"""
    p = np.ascontiguousarray(rows, np.float64)
    out = np.zeros((p.shape[0], 4), np.uint16)
    bad = np.full(3, -7, np.int64)
    if host.fixed_thresholds_host(p.ctypes.data, p.shape[0], out.ctypes.data, bad.ctypes.data):
        return out, None
    assert bad[0] == 0
    return None, (int(bad[1]), int(bad[2]))


def rows_check(host, policy, first_row):
    """None where [members, nS, 5] holds, else the first bad (member, state, action)"""
    p = np.ascontiguousarray(policy, np.float64)
    bad = np.full(3, -7, np.int64)
    ok = host.policy_rows_check_host(p.ctypes.data, p.shape[0], p.shape[1], first_row, bad.ctypes.data)
    return None if ok else tuple(int(x) for x in bad)


def grid_rows(rng, n):
    """rows of multiples of 2^-15 summing to 1 exactly: every cumulative sum lands on a threshold's boundary"""
    cuts = np.sort(rng.integers(0, 32769, (n, 4)), axis=1)
    k = np.diff(np.concatenate([np.zeros((n, 1), np.int64), cuts, np.full((n, 1), 32768)], axis=1), axis=1)
    return k / 32768.0


def threshold_cases():
    rng = np.random.default_rng(1994)
    zeros = rng.dirichlet(np.ones(5), 200)
    zeros[rng.random((200, 5)) < 0.4] = 0.0
    zeros = zeros[zeros.sum(1) > 0]
    zeros /= zeros.sum(1, keepdims=True)
    return {"random": rng.dirichlet(np.ones(5), 400), "peaked": rng.dirichlet(np.full(5, 0.05), 400), "one-hot": np.eye(5),
            "uniform": np.full((3, 5), 0.2), "zeros": zeros, "grid": grid_rows(rng, 400),
            "grid edges": np.array([[0, 0, 0, 0, 1.0], [1 / 32768, 0, 0, 0, 32767 / 32768], [32767 / 32768, 0, 0, 0, 1 / 32768],
                                    [0.25, 0.25, 0.25, 0.25, 0.0]])}


CASES = threshold_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_thresholds_are_the_package_s_bit_for_bit(host, name):
    rows = CASES[name]
    got, bad = thresholds(host, rows)
    assert bad is None
    want = SoccerBatch.mixed_policy_thresholds(rows)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == want.dtype == np.uint16 and (np.diff(got.astype(int), axis=1) >= 0).all() and got.max() <= 32768
    if name == "grid":                                      # the point of the case: the thresholds ARE the cumulative counts
        np.testing.assert_array_equal(got, np.round(np.cumsum(rows, 1)[:, :4] * 32768).astype(np.uint16))


def test_thresholds_check_every_row_row_0_too(host):
    rows = np.full((6, 5), 0.2)
    for s in (0, 3, 5):
        r = rows.copy(); r[s, 2] = -1e-300
        assert thresholds(host, r) == (None, (s, 2))
        r = rows.copy(); r[s, 4] = 0.3
        assert thresholds(host, r) == (None, (s, 5))


def test_row_check_refuses_a_negative_entry_and_nan(host):
    base = np.full((3, 4, 5), 0.2)
    assert rows_check(host, base, 0) is None
    for value in (-1e-300, -0.2, np.nan, -np.inf):
        p = base.copy(); p[1, 2, 3] = value
        assert rows_check(host, p, 0) == (1, 2, 3)
    p = base.copy(); p[2, 1, 0] = np.inf                     # not negative: the sum fails
    assert rows_check(host, p, 0) == (2, 1, 5)
    p = base.copy(); p[0, 0, :] = [0.0, -0.0, 0.5, 0.5, 0.0]  # a negative zero is zero
    assert rows_check(host, p, 0) is None


@pytest.mark.parametrize("delta, holds", [(1.0e-5, True), (-1.0e-5, True), (1.1e-5, False), (-1.1e-5, False)])
def test_row_check_at_the_bound_of_the_sum(host, delta, holds):
    """the bound is 1e-8 + 1e-5: sums of 1 +- 1.0e-5 lie within, 1 +- 1.1e-5 outside, rounding is 1e-16"""
    for k in range(5):
        p = np.full((1, 2, 5), 0.2)
        p[0, 1, k] += delta
        assert rows_check(host, p, 0) == (None if holds else (0, 1, 5))


def test_row_check_reports_the_first_bad_place(host):
    p = np.full((4, 5, 5), 0.2)
    p[3, 0, 0] = -1.0; p[2, 4, 1] = np.nan; p[2, 3, 2] = 0.9; p[2, 3, 4] = -0.5
    assert rows_check(host, p, 0) == (2, 3, 4)               # member, then state, then action; an entry before the row's sum
    p[2, 3, 4] = 0.2
    assert rows_check(host, p, 0) == (2, 3, 5)
    p[2, 3, 2] = 0.2
    assert rows_check(host, p, 0) == (2, 4, 1)


def test_row_check_honours_first_row(host):
    p = np.full((3, 4, 5), 0.2)
    p[:, 0, :] = np.nan                                      # row 0 of a checkpoint is not read
    assert rows_check(host, p, 1) is None
    assert rows_check(host, p, 0) == (0, 0, 0)
    p[1, 1, 4] = -1.0
    assert rows_check(host, p, 1) == (1, 1, 4)


@pytest.mark.parametrize("width", [1, 5, 25])
def test_q_bounds_skip_row_0_of_every_member_and_report_the_first_bad_index(host, width):
    members, nS = 3, 4
    rng = np.random.default_rng(width)
    q = rng.uniform(-1.0, 1.0, (members, nS, width))
    q[0, 1, 0] = -1.0; q[2, 3, width - 1] = 1.0               # the bounds themselves are inside
    q[:, 0, :] = [[np.nan], [7.0], [-np.inf]]                # row 0 of EVERY member is not read
    check = lambda a, m=members: host.q_bounds_check_host(np.ascontiguousarray(a).ctypes.data, m, nS, width)  # noqa: E731
    assert check(q) == -1
    assert check(q[:1], 1) == -1                             # one table: a single learner's
    for value in (np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.nan, np.inf):
        bad = q.copy()
        bad[2, 3, width - 1] = value; bad[1, 2, 0] = value
        assert check(bad) == (1 * nS + 2) * width
        bad[1, 2, 0] = 0.0
        assert check(bad) == members * nS * width - 1
        bad[0, 1, width // 2] = value                        # the first live value region of member 0
        assert check(bad) == 1 * width + width // 2
