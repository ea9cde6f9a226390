"""The steady state's carried step (csrc/soccer_swar.hpp: swar::Carry4 — possession as a byte mask, the timestep biased by
trunc_add — and step4_carry, what the rollout's step loop runs) on the CPU, EXHAUSTIVELY: convert in, two carried steps,
convert out, against the same two steps as swar::step4<false, ...> calls, which tests/test_swar_host.py pins to the
oracle.  The second step consumes a carried state that came out of the first, its in-step reset included.  Every live
tuple x 25 joint actions x 4 outcome draws x 4 reset draws x 4 timesteps; nothing is thinned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("obs", "final_obs", "reward", "terminated", "truncated", "prob_code", "finished")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("swar_carry") / "libswar_carry_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "host", "swar_carry_host.cpp")])
    L = C.CDLL(so)
    L.swar_carry_host.restype = C.c_int
    L.swar_carry_host.argtypes = [C.c_int] * 8 + [C.c_long] + [C.c_void_p] * 9 + [C.c_double] + [C.c_void_p] * 8
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _live(w, h, slip=0.0):
    o = Oracle(w, h, slip, n=1)
    lut, kind, gv, isd, isdp = o.tables()
    f = np.flatnonzero(kind == 1)
    p = f & 1; r = f >> 1
    cb = r % o.W; r //= o.W; rb = r % o.H; r //= o.H; ca = r % o.W; ra = r // o.W
    return np.stack([ra, ca, rb, cb, p], 1).astype(np.uint8)


def _run(L, w, h, max_steps, full, geo, sel, carried, st, t, aa, ab, words, slip=0.0):
    """aa / ab / words: [steps, n].  Returns the outputs as [steps, n] arrays and the six state streams after the last step."""
    steps, n = aa.shape
    assert n % 4 == 0
    state = [np.array(st[:, k], np.uint8) for k in range(5)] + [np.array(t, np.uint8)]      # copies: the shim steps them in place
    out = {k: np.zeros((steps, n), np.uint16 if "obs" in k else np.uint8) for k in OUTS}
    out["bad"] = np.zeros((steps, n // 4), np.uint8)
    aa = np.ascontiguousarray(aa, np.uint8); ab = np.ascontiguousarray(ab, np.uint8); words = np.ascontiguousarray(words, np.uint32)
    rc = L.swar_carry_host(w, h, max_steps, int(full), geo, sel, int(carried), steps, n, *[_p(x) for x in state],
                           _p(aa), _p(ab), _p(words), float(slip),
                           *[_p(out[k]) for k in OUTS], _p(out["bad"]))
    if rc == -4:
        return None
    assert rc == 0
    out["state"] = state
    return out


def _same(got, exp, full):
    for k in OUTS:
        if not full and k in ("final_obs", "prob_code"):
            continue
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, "%s differs on %d lane-steps, first (step, lane) %s: got %s expected %s" % (
            k, len(bad), tuple(bad[0]), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])
    for k, name in enumerate(("row_a", "col_a", "row_b", "col_b", "poss", "t")):
        bad = np.flatnonzero(got["state"][k] != exp["state"][k])
        assert bad.size == 0, "state %s differs on %d lanes, first %d: got %d expected %d" % (
            name, bad.size, bad[0], got["state"][k][bad[0]], exp["state"][k][bad[0]])
    np.testing.assert_array_equal(got["bad"], exp["bad"])


def _two_steps(x, shift):
    """the second step's row: the first one rolled, so that it meets other combinations than the first"""
    return np.stack([x, np.roll(x, shift)])


def _grid(tup, rng):
    """every tuple x 25 joint actions x 4 outcome draws x 4 reset draws (the 16 nibble draws)"""
    idx = np.arange(len(tup) * 400)
    ti = idx // 400; r = idx % 400
    aa = r // 80; r %= 80
    ab = r // 16; r %= 16
    top2 = r // 4; reset2 = r % 4
    mid = rng.integers(0, 1 << 28, size=len(idx), dtype=np.uint32)
    words = (top2.astype(np.uint32) << 30) | (mid << 2) | reset2.astype(np.uint32)
    return tup[ti], aa.astype(np.uint8), ab.astype(np.uint8), words           # len(tup) * 400: a multiple of 4


PITCHES = [(5, 4, -1), (6, 4, -1), (6, 6, -1), (6, 6, 0), (7, 5, -1), (11, 7, -1), (14, 8, -1), (15, 4, -1), (5, 9, -1)]


@pytest.mark.parametrize("w,h,geo", PITCHES, ids=["%dx%d%s" % (w, h, "-arithmetic" if g == 0 else "") for w, h, g in PITCHES])
def test_two_carried_steps_every_live_tuple_action_draw_and_timestep(host, w, h, geo):
    rng = np.random.default_rng(w * 100 + h + 7)
    ms = 100
    st, aa, ab, words = _grid(_live(w, h), rng)
    aa2, ab2, words2 = _two_steps(aa, 1237), _two_steps(ab, 4111), _two_steps(words, 97)
    for t0 in (0, 3, ms - 2, ms - 1):
        t = np.full(len(st), t0, np.uint8)
        for full in (True, False):
            exp = _run(host, w, h, ms, full, geo, 1, False, st, t, aa2, ab2, words2)
            got = _run(host, w, h, ms, full, geo, 1, True, st, t, aa2, ab2, words2)
            _same(got, exp, full)
            assert not got["bad"].any()
        if t0 >= ms - 2:      # the grid does reach the in-step reset, in the first step or the second
            assert exp["truncated"][ms - 1 - t0].any() and exp["terminated"][0].any()


@pytest.mark.parametrize("ms", [1, 2, 17, 127])
def test_other_episode_lengths(host, ms):
    """the bias 0x80 - max_steps takes the values 0x7f, 0x7e and 1"""
    rng = np.random.default_rng(ms)
    st, aa, ab, words = _grid(_live(5, 4), rng)
    aa2, ab2, words2 = _two_steps(aa, 1237), _two_steps(ab, 4111), _two_steps(words, 97)
    for geo in (-1, 0):
        for t0 in sorted({0, max(ms - 2, 0), ms - 1}):
            t = np.full(len(st), t0, np.uint8)
            exp = _run(host, 5, 4, ms, True, geo, 1, False, st, t, aa2, ab2, words2)
            got = _run(host, 5, 4, ms, True, geo, 1, True, st, t, aa2, ab2, words2)
            _same(got, exp, True)


def _slip_words(slip, n, rng):
    """as tests/test_swar_host.py chooses them: uniform words, plus words exactly on, one below and one above every scaled
    threshold of the handle"""
    s = slip
    c = [(1 - s) * (1 - s), (1 - s) * s * 0.5, (1 - s) * s * 0.5, s * (1 - s) * 0.5, s * (1 - s) * 0.5] + [s * s * 0.25] * 4
    edges = []
    acc = 0.0
    for wgt in c:
        if wgt == 0.0:
            continue
        for q in (0.25, 0.5, 0.75, 1.0):
            edges.append(acc + wgt * q)
        acc += wgt
    m_edge = np.array([int(np.ceil(e * 2 ** 30 - 0.5)) for e in edges if e < 1.0], dtype=np.int64)
    special = np.concatenate([m_edge - 1, m_edge, m_edge + 1, [0, 1, 2 ** 30 - 1]])
    special = special[(special >= 0) & (special < 2 ** 30)]
    m = rng.integers(0, 1 << 30, size=n, dtype=np.int64)
    pick = rng.random(n) < 0.25
    m[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return ((m << 2) | rng.integers(0, 4, size=n)).astype(np.uint32)


@pytest.mark.parametrize("sel", [1, 2], ids=["one_by_one", "table"])
@pytest.mark.parametrize("w,h,geo", [(5, 4, -1), (5, 4, 0), (7, 5, -1)])
@pytest.mark.parametrize("slip", [0.2, 0.03])
def test_two_carried_slip_steps_with_draws_on_every_threshold(host, slip, w, h, geo, sel):
    rng = np.random.default_rng(int(slip * 100) + w + geo)
    tup = _live(w, h, slip)
    reps = 6
    idx = np.arange(len(tup) * 25 * reps)
    idx = idx[:len(idx) - len(idx) % 4]
    ti = idx // (25 * reps); r = idx % (25 * reps)
    aa = ((r // reps) // 5).astype(np.uint8); ab = ((r // reps) % 5).astype(np.uint8)
    n = len(idx)
    words2 = np.stack([_slip_words(slip, n, rng), _slip_words(slip, n, rng)])
    aa2, ab2 = _two_steps(aa, 1237), _two_steps(ab, 4111)
    t = np.asarray([0, 40, 98, 99], np.uint8)[rng.integers(0, 4, size=n)]
    for full in (True, False):
        exp = _run(host, w, h, 100, full, geo, sel, False, tup[ti], t, aa2, ab2, words2, slip=slip)
        got = _run(host, w, h, 100, full, geo, sel, True, tup[ti], t, aa2, ab2, words2, slip=slip)
        if exp is None:
            assert got is None and sel == 2      # this slip has no bucket table: the kernels compare one by one
            return
        _same(got, exp, full)


@pytest.mark.parametrize("geo", [-1, 0], ids=["tables", "arithmetic"])
@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_actions_outside_0_4_are_reported_per_group_and_execute_as_their_low_three_bits(host, geo, slip):
    rng = np.random.default_rng(9)
    tup = _live(5, 4)
    n = 4 * 20000
    st = tup[rng.integers(0, len(tup), size=n)]
    aa = rng.integers(0, 5, size=(2, n)).astype(np.uint8); ab = rng.integers(0, 5, size=(2, n)).astype(np.uint8)
    vals = np.array([5, 6, 7, 8, 127, 128, 255, 0x85], np.uint8)
    flagged = np.zeros((2, n // 4), bool)
    aa_bad = aa.copy(); ab_bad = ab.copy()
    for k in range(2):
        bad_lane = np.arange(0, n, 8) + rng.integers(0, 8, size=n // 8)       # one per two groups
        which = rng.integers(0, 2, size=len(bad_lane)).astype(bool)
        aa_bad[k, bad_lane[which]] = vals[rng.integers(0, len(vals), size=which.sum())]
        ab_bad[k, bad_lane[~which]] = vals[rng.integers(0, len(vals), size=(~which).sum())]
        flagged[k, bad_lane // 4] = True
    words = rng.integers(0, 1 << 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
    t = rng.integers(0, 99, size=n).astype(np.uint8)
    got = _run(host, 5, 4, 100, True, geo, 1, True, st, t, aa_bad, ab_bad, words, slip=slip)
    # flagged groups are exactly the groups holding such a byte
    np.testing.assert_array_equal(got["bad"].astype(bool), flagged)
    # every lane executes table[b & 7], and 5..7 are NOOP: the same run with those actions written out, by the plain step
    canon = lambda x: np.where((x & 7) > 4, 0, x & 7).astype(np.uint8)
    exp = _run(host, 5, 4, 100, True, geo, 1, False, st, t, canon(aa_bad), canon(ab_bad), words, slip=slip)
    assert not exp["bad"].any()
    exp["bad"] = got["bad"]
    _same(got, exp, True)
