"""The packed resident state (csrc/soccer_swar.hpp: pack3 / unpack3 — poss << 7 | row_a << 4 | col_a, need << 7 | row_b << 4 |
col_b, t) on the CPU, EXHAUSTIVELY: the round trip of every field value in every byte position with its neighbours untouched,
and a step taken through packed dwords against the step through the six-stream swar::Group and against the oracle, over the
enumeration tests/test_swar_host.py uses (every reachable tuple x 25 joint actions x 4 outcome draws x 4 reset draws) on the
two pitches the packed layout is timed on, 5x4 and 11x7, and on 14x8, the corner of the layout (row 7, column 15, H * W = 128).
tests/host/state_pack_host.cpp compiles the header for the host, so this is the code the kernels run.  SWAR_HOST_SANITIZE=1 builds it with UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pack") / "libstate_pack_host.so")
    san = ["-fsanitize=undefined", "-fno-sanitize-recover=all", "-g"] if os.environ.get("SWAR_HOST_SANITIZE") else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror"] + san + ["-o", so,
                           os.path.join(ROOT, "tests", "host", "state_pack_host.cpp")])
    L = C.CDLL(so)
    L.state_pack_roundtrip.restype = C.c_long
    L.state_pack_roundtrip.argtypes = [C.c_void_p]
    L.state_pack_step.restype = C.c_long
    L.state_pack_step.argtypes = [C.c_int] * 7 + [C.c_long] + [C.c_void_p] * 14
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_round_trip_of_every_field_value_in_every_byte_position(host):
    first = np.full(7, -1, np.int32)
    bad = host.state_pack_roundtrip(_p(first))
    assert bad == 0, "%d failures, first (ra, ca, rb, cb, poss|need<<1, t, byte position) = %s" % (bad, first.tolist())


def _tuples(o, kinds):
    lut, kind, gv, isd, isdp = o.tables()
    f = np.flatnonzero(np.isin(kind, kinds))
    p = f & 1; r = f >> 1
    cb = r % o.W; r //= o.W; rb = r % o.H; r //= o.H; ca = r % o.W; ra = r // o.W
    return np.stack([ra, ca, rb, cb, p], 1).astype(np.int64)


def _grid(tup, t_values, need_values, rng):
    """every tuple x 25 joint actions x 4 outcome draws x 4 reset draws, timestep / frozen flag cycled"""
    idx = np.arange(len(tup) * 25 * 16)
    ti = idx // 400; r = idx % 400
    aa = r // 80; r %= 80
    ab = r // 16; r %= 16
    top2 = r // 4; reset2 = r % 4
    n = len(idx)
    assert n % 4 == 0
    mid = rng.integers(0, 1 << 28, size=n, dtype=np.uint32)
    words = (top2.astype(np.uint32) << 30) | (mid << 2) | reset2.astype(np.uint32)
    t = np.asarray(t_values)[rng.integers(0, len(t_values), size=n)]
    need = np.asarray(need_values)[rng.integers(0, len(need_values), size=n)]
    return tup[ti], t, need.astype(np.int64), aa, ab, words


def _step_both_ways(L, w, h, autoreset, general, full, geo0, st, t, need, aa, ab, words):
    n = len(t)
    ra, ca, rb, cb = (np.ascontiguousarray(st[:, k], np.uint8) for k in range(4))
    ps = np.ascontiguousarray(st[:, 4] | (need << 1), np.uint8)
    tt = np.ascontiguousarray(t, np.uint8)
    out = dict(obs=np.zeros(n, np.uint16), reward=np.zeros(n, np.uint8), terminated=np.zeros(n, np.uint8), truncated=np.zeros(n, np.uint8))
    first = np.full(1, -1, np.int64)
    bad = L.state_pack_step(w, h, 100, int(autoreset), int(general), int(full), int(geo0), n, _p(ra), _p(ca), _p(rb), _p(cb), _p(ps), _p(tt),
                            _p(np.ascontiguousarray(aa, np.uint8)), _p(np.ascontiguousarray(ab, np.uint8)), _p(np.ascontiguousarray(words, np.uint32)),
                            _p(out["obs"]), _p(out["reward"]), _p(out["terminated"]), _p(out["truncated"]), _p(first))
    assert bad == 0, "the packed step differs from the six-stream step in %d groups, first group %d" % (bad, first[0])
    out["reward"] = out["reward"].view(np.int8)
    out["state"] = (ra, ca, rb, cb, ps, tt)
    return out


def _oracle_step(w, h, autoreset, st, t, need, aa, ab, words):
    o = Oracle(w, h, 0.0, n=len(t), autoreset=autoreset, max_steps=100)
    o.set_state(st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], t=t, needs_reset=need)
    c = o.step(aa, ab, u_step=((words >> 2).astype(np.float64) + 0.5) * 2.0 ** -30, u_reset=((words & 3).astype(np.float64) + 0.5) * 0.25)
    c["state"] = (o.row_a.view(np.uint8), o.col_a.view(np.uint8), o.row_b.view(np.uint8), o.col_b.view(np.uint8), o.poss, o.t)
    return c


def _against_oracle(got, exp):
    for k in ("obs", "reward", "terminated", "truncated"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    for k, name in enumerate(("row_a", "col_a", "row_b", "col_b", "poss|needs_reset<<1", "t")):
        np.testing.assert_array_equal(got["state"][k], exp["state"][k], err_msg=name)


@pytest.mark.parametrize("w,h", [(5, 4), (11, 7), (14, 8)])
@pytest.mark.parametrize("autoreset", [True, False])
def test_general_step_through_packed_dwords(host, w, h, autoreset):
    """live and goal tuples, frozen lanes, timesteps around the truncation: Out and next state of the packed walk equal the
    six-stream walk's (every field, FULL and lean), and the oracle's"""
    rng = np.random.default_rng(w * 100 + h)
    tup = _tuples(Oracle(w, h, 0.0, n=1), [1, 2])
    st, t, need, aa, ab, words = _grid(tup, [0, 1, 57, 98, 99, 100], [0, 0, 0, 1], rng)
    t = np.where(need == 1, t, np.minimum(t, 99))              # a lane that is not frozen has t < max_steps
    exp = _oracle_step(w, h, autoreset, st, t, need, aa, ab, words)
    for full in (True, False):
        for geo0 in ((False, True) if (w, h) == (5, 4) else (False,)):     # byte tables and arithmetic on the small pitch
            _against_oracle(_step_both_ways(host, w, h, autoreset, True, full, geo0, st, t, need, aa, ab, words), exp)


@pytest.mark.parametrize("w,h", [(5, 4), (11, 7), (14, 8)])
def test_steady_state_step_through_packed_dwords(host, w, h):
    """the instantiation without the frozen-lane / goal-tuple code, on every live tuple"""
    rng = np.random.default_rng(w * 100 + h + 1)
    tup = _tuples(Oracle(w, h, 0.0, n=1), [1])
    st, t, need, aa, ab, words = _grid(tup, [0, 3, 98, 99], [0], rng)
    exp = _oracle_step(w, h, True, st, t, need, aa, ab, words)
    for full in (True, False):
        _against_oracle(_step_both_ways(host, w, h, True, False, full, False, st, t, need, aa, ab, words), exp)
