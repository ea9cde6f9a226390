"""Where there is no GPU: every case of tests/test_gpu_pair_evaluator_shapes.py and tests/test_gpu_pair_evaluator_edges.py reaches
the path it is there for, shown on the numpy restatements alone (tests/match_outcomes_np.py, tests/occupancy_np.py,
tests/policy_gradient_np.py) — the pitches' residues modulo the 64 x 64 transpose tile, both kick-off counts and the three in-list
regimes of slip 0, an ordinary slip and slip 1; on 5x4 at slips 0.0 and 0.2 sweep 2 at continue_prob 0, sweep 1 at theta = +inf,
the cap itself at theta = 0, converged and capped solves side by side at continue_prob 1, the unusual rows solved to finite
numbers, and the sweep bound and the size of the matrices that each call's own pass split is run on.  The cases are those of
tests/pair_evaluator_cases.py, which the GPU modules import too, so all see the same inputs; 13x8 is not restated here."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import match_outcomes_np as mon  # noqa: E402
import occupancy_np as ocn  # noqa: E402
import pair_evaluator_cases as pc  # noqa: E402
import two_player_cases as tpc  # noqa: E402
from two_player_cases import (INF, NS, SLIPS, THETA, THETA0_CAPS, UNDISCOUNTED_CAP, boundary_sample, edge_policies, odd_rows,  # noqa: E402
                              pitch, row_accepted)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_PITCHES = [p for p in pc.PITCHES if p != pc.LARGEST]


@pytest.fixture(scope="module", autouse=True)
def drop_the_lists():
    yield
    pc.forget_shapes()


def edge_pair():
    pol = edge_policies()
    return pol, np.roll(pol, 1, 0)


# ---- the pitches ------------------------------------------------------------------------------------------------------------
def test_the_pitches_sit_where_they_should():
    assert pc.PITCHES == [(5, 4, 0.0), (6, 4, 0.2), (6, 5, 0.2), (7, 5, 1.0), (5, 9, 0.3), (8, 7, 0.0), (11, 7, 0.2), (13, 8, 0.1)]
    nS = {p[:2]: pc.n_states(*p[:2]) for p in pc.PITCHES}
    # the ragged edge of cross_values_kernel's / match_values_kernel's 64 x 64 tile: the three existing suites see 57 and 13 only
    assert nS[(6, 4)] % 64 == 17 and nS[(13, 8)] % 64 == 49 and nS[(6, 5)] % 64 == nS[(7, 5)] % 64 == 13 and nS[(5, 4)] % 64 == 57
    assert {n % 64 for n in nS.values()} >= {13, 17, 49, 57} and 0 not in {n % 64 for n in nS.values()}
    # both kick-off counts, away from 5x4 too
    assert {pc.kickoffs(h) for _, h, _ in pc.PITCHES} == {2, 4}
    assert [pc.kickoffs(h) for _, h, _ in pc.PITCHES] == [4, 4, 2, 2, 2, 2, 2, 4]
    # slips 0 and 1 and one in between; slip 0 on a large pitch; an even width; taller than wide; above the planners' 19 013 states
    assert {0.0, 1.0} <= {p[2] for p in pc.PITCHES} and any(0.0 < p[2] < 1.0 for p in pc.PITCHES)
    assert (8, 7, 0.0) in pc.PITCHES and any(w % 2 == 0 for w, _, _ in pc.PITCHES) and any(h > w for w, h, _ in pc.PITCHES)
    assert max(nS.values()) == nS[pc.LARGEST[:2]] == 21425 > 19013 and max(nS.values()) <= 65535
    assert [pc.discount(*p[:2]) for p in pc.PITCHES] == [0.9, 0.9, 0.9, 0.9, 0.5, 0.5, 0.5, 0.5]
    assert 0.5 ** 34 < pc.THETA <= 0.5 ** 33                    # at 0.5 every solve stops by sweep 35 (36 is the issue's ceiling)
    assert sorted(pc.IN_LISTS) == sorted(pc.PITCHES)


@pytest.mark.parametrize("w,h,slip", CPU_PITCHES, ids=pc.IDS[:len(CPU_PITCHES)])
def test_the_in_lists_and_kick_offs_of_every_pitch(w, h, slip):
    g = pc.shape(w, h, slip)
    assert g.nS == pc.n_states(w, h)
    off, in_prob, in_key = g.inl
    size = np.diff(off)
    K = g.lists[0].shape[2]
    print("%dx%d slip %.1f: nS %d (mod 64: %d), %d kick-offs, K %d, in-lists of %d .. %d, %d in-entries with padding" % (
        w, h, slip, g.nS, g.nS % 64, len(g.starts), K, size[1:].min(), size.max(), off[-1]))
    assert (g.longest_in_list(), K) == pc.IN_LISTS[(w, h, slip)]
    assert {0.0: (40, 4), 1.0: (152, 7)}.get(slip, (344, 15)) == pc.IN_LISTS[(w, h, slip)]     # the regime is the slip's alone
    assert (size % ocn.PAD == 0).all() and size[0] == 0
    # the kick-off states: distinct, live, as many as the height says, and mu is 1 / their number
    assert len(g.starts) == len(set(g.starts)) == pc.kickoffs(h) and min(g.starts) >= 1
    mu = ocn.start_distribution(g.nS, g.starts)
    assert sorted(np.flatnonzero(mu).tolist()) == sorted(g.starts) and set(mu[g.starts].tolist()) == {1.0 / pc.kickoffs(h)}
    # the matrix: a one-hot policy on both sides
    assert g.A.shape == (2, g.nS, 5) and g.B.shape == (3, g.nS, 5) and (g.A[1] == g.B[1]).all() and set(np.unique(g.A[1]).tolist()) == {0.0, 1.0}


# ---- the parameter ends, on 5x4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_continue_prob_0_stops_at_sweep_2(slip):
    A, B = edge_pair()
    r = pc.three_calls("edge", slip, A, B, 0.0, THETA)
    k = pc.counts(r)
    assert (k["match"] == 2).all() and (k["occupancy"] == 2).all() and (k["D"] == 2).all()
    # (a pair under which nobody scores at once has V_1 = 0 = V_0 and stops at sweep 1; with slip somebody always may)
    assert set(k["V"].reshape(-1).tolist()) == ({1, 2} if slip == 0.0 else {2})
    # a game of exactly one step: L_2 = L_1 = sum_ab x[s][a] * y[s][b] * sum prob, which is 1.0 to the bit where both rows are
    # one-hot (policies 2 and 3 against their roll: columns 3 and 0) and the list's probabilities are 1 or 0.5 and 0.5 (slip
    # 0), and 1.0 up to the rounding of at most 25 * 15 + 30 additions and products elsewhere (a Dirichlet row, or 0.8 + 0.1
    # + 0.1, sums to 1 only up to an ulp) — the device is held to these bits
    L = r["match"]["length"]
    assert (slip != 0.0 or (L[2:, [0, 3]] == 1.0).all()) and np.abs(L - 1.0).max() <= 405 * 2.0 ** -53 and (r["match"]["values"][:, :, 2, 0] == 0.0).all()
    mu = ocn.start_distribution(NS, pitch(slip)[1])
    assert (r["occupancy"]["occupancy"] == mu).all() and (r["gradient"]["occupancy"] == mu).all()


@pytest.mark.parametrize("slip", SLIPS)
def test_theta_inf_stops_at_sweep_1_and_theta_0_never(slip):
    A, B = edge_pair()
    k = pc.counts(pc.three_calls("edge", slip, A, B, 0.9, INF))
    assert all((v == 1).all() for v in k.values())
    # theta = 0: even the solve that has reached its fixed point exactly (continue_prob 0, sweep 2) goes on to the cap
    assert THETA0_CAPS == [15, 16, 17, 32, 33]
    for cap in (THETA0_CAPS[0], THETA0_CAPS[-1]):
        for c in (0.9, 0.0):
            k = pc.counts(pc.three_calls("edge", slip, A, B, c, 0.0, cap))
            assert all((v == cap).all() for v in k.values()), (cap, c)


@pytest.mark.parametrize("slip", SLIPS)
def test_continue_prob_1_leaves_converged_and_capped_solves_side_by_side(slip):
    A, B = edge_pair()
    cap = UNDISCOUNTED_CAP
    k = pc.counts(pc.three_calls("edge", slip, A, B, 1.0, THETA, cap))
    print("slip %.1f, continue_prob 1, cap %d: V sweeps %s" % (slip, cap, k["V"].reshape(-1).tolist()))
    assert (k["match"] == cap).all() and (k["occupancy"] == cap).all() and (k["D"] == cap).all()
    assert int((k["V"] == cap).sum()) == {0.0: 11, 0.2: 14}[slip] and (k["V"] < cap).sum() == 16 - {0.0: 11, 0.2: 14}[slip]
    # no V solve converges exactly at the cap: the solves at the cap are the ones still open one sweep later
    lists, _ = pitch(slip)
    later = brn.evaluate(lists, np.repeat(A, 4, axis=0), np.tile(B, (4, 1, 1)), 1.0, THETA, cap + 1)[1].reshape(4, 4)
    assert ((later == cap + 1) == (k["V"] == cap)).all() and (later[later <= cap] == k["V"][later <= cap]).all()


# ---- unusual rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_the_unusual_rows_are_solved_to_finite_numbers_in_every_call(slip):
    pol = odd_rows()
    assert all(row_accepted(pol[i, s]) for i in range(2) for s in range(1, NS))
    r = pc.three_calls("odd", slip, pol, pol[::-1], 0.9, THETA)
    k = pc.counts(r)
    print("slip %.1f, unusual rows: sweeps %s" % (slip, {n: v.reshape(-1).tolist() for n, v in k.items()}))
    assert 0.9 ** 219 < THETA <= 0.9 ** 218
    assert all((v > 100).all() and (v < pc.UNUSUAL_SWEEPS).all() for v in k.values())
    assert (k["match"] == 220).all() and (k["V"] < k["D"]).all() and (k["occupancy"] == k["D"]).all()
    assert all(np.isfinite(v).all() for d in r.values() for v in d.values())
    # the per-entry product x[s][a] * y[s][b] meets -0.0 and subnormal factors, the normalisation a reach of exactly 0.0
    assert np.signbit(pol[pol == 0.0]).sum() > 500 and ((pol > 0.0) & (pol < 2.3e-308)).sum() > 500
    g = r["gradient"]
    assert (g["reach_a"][:, 1:] > 0.0).any() and (g["grad_a"][:, 0] == 0.0).all() and (np.abs(g["grad_a"]) > 1e-3).any()


# ---- 1024 policies a side -------------------------------------------------------------------------------------------------------
def test_the_limit_matrices_and_their_samples():
    assert pc.LIMIT_SHAPES == [(1024, 1), (1, 1024), (1024, 2)]
    for n_a, n_b in pc.LIMIT_SHAPES:
        A, B = pc.limit_policies(n_a, n_b)
        assert A.shape == (n_a, NS, 5) and B.shape == (n_b, NS, 5)
        flat = boundary_sample(n_a * n_b)
        assert len(flat) == n_a * n_b // 32 and {0, 63, 64, n_a * n_b - 1} <= set(flat)
    # 67 x 7 in passes of 64 and of 128: every column's pairs, a stride of n_b = 7 apart, lie in all 8 (4) passes; the pass
    # boundaries are no multiples of 7 (but for 448 = 64 * 7), so the first pair of a column in a pass is found by rounding up
    n_a, n_b = pc.SPAN_SHAPE
    for per in pc.SPAN_PASSES:
        firsts = list(range(0, n_a * n_b, per))
        assert len(firsts) == -(-469 // per) and [f for f in firsts[1:] if f % n_b == 0] == ([448] if per == 64 else [])
        for j in (0, n_b - 1):
            assert all(any(f <= i * n_b + j < f + per for i in range(n_a)) for f in firsts)
    assert len(boundary_sample(n_a * n_b)) == 16


# ---- the library's own pass split --------------------------------------------------------------------------------------------------
def test_the_pass_sizes_are_the_library_s():
    assert pc.PASS_PAIRS == {"occupancy": 88128, "match": 29376, "gradient": 12544}
    for call in pc.CALLS:
        per, total = pc.PASS_PAIRS[call], 1024 * pc.PASS_NB[call]
        assert per < total < per + 1024 and 0 < total - per and (total - per) % 64 == 0          # a ragged second pass, whole waves
        assert 1024 * (pc.PASS_NB[call] - 1) <= per                                              # one column fewer is one pass
        flat = pc.pass_sample(call)
        assert {0, per - 1, per, total - 1} <= set(flat) and 16 <= len(flat) <= 24
    assert (89088, 29696, 13312) == tuple(1024 * pc.PASS_NB[c] for c in ("occupancy", "match", "gradient"))
    # the boundary of the policy gradient's split lies inside row 964: its pairs 0 .. 11 in the first pass, pair 12 in the second
    assert divmod(pc.PASS_PAIRS["gradient"], 13) == (964, 12)
    # the divisors are the source's: the bytes a pair and state that soccer_cross_play, soccer_occupancy, soccer_match_outcomes
    # (16 * kMatchChannels) and gradient_solve hand to pass_pairs, which holds the rule itself, once
    with open(os.path.join(ROOT, "gym_soccer_littman94_amd", "csrc", "soccer_pairs.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "gym_soccer_littman94_amd", "csrc", "soccer_pair_kernels.hpp")) as f:
        assert re.search(r"constexpr int kMatchChannels = 3;", f.read())
    rule = re.findall(r"static int pass_pairs\(int32_t pairs_per_pass, size_t bytes, int nS, int total\) \{\n"
                      r"    const int per_pass = pairs_per_pass \? pairs_per_pass : std::max\(64, \(int\)\(\(\(size_t\)1 << 30\) / "
                      r"\(bytes \* nS\) / 64 \* 64\)\);\n", src)
    assert len(rule) == 1 and src.count("1 << 30") == 1

    def per_pass_of(function):
        body = src[src.index(function):]
        body = body[:body.index("\n}\n")]                                # the function's own lines
        calls = re.findall(r"const int per_pass = pass_pairs\(pairs_per_pass, ([0-9a-zA-Z* ]+), nS, total\);", body)
        assert len(calls) == 1
        return calls[0]
    assert per_pass_of('extern "C" int soccer_cross_play(') == "16" and tpc.PASS_PAIRS == 2 ** 30 // (16 * NS) // 64 * 64
    assert per_pass_of('extern "C" int soccer_occupancy(') == "16" and pc.PASS_BYTES["occupancy"] == 16
    assert per_pass_of('extern "C" int soccer_match_outcomes(') == "16 * kMatchChannels" and pc.PASS_BYTES["match"] == 16 * 3
    assert per_pass_of("static int gradient_solve(") == "112" and pc.PASS_BYTES["gradient"] == 112


@pytest.mark.parametrize("slip", SLIPS)
def test_the_low_continuation_matrices_stop_within_their_bound(slip):
    assert pc.PASS_C ** (pc.PASS_SWEEPS - 1) < THETA <= pc.PASS_C ** (pc.PASS_SWEEPS - 2)
    for call in pc.CALLS:
        A, B = pc.pass_matrix(call)
        assert A.shape[0] == 1024 and B.shape[0] == pc.PASS_NB[call]
        r = pc.restate(call, slip, A, B, pc.PASS_C, THETA, pairs=pc.pass_sample(call))
        it = r["iterations"]
        print("slip %.1f, %s: sweeps of the %d sampled pairs %d .. %d" % (slip, call, len(it), it.min(), it.max()))
        assert 2 < it.min() and it.max() <= pc.PASS_SWEEPS
    # the bound itself, channel by channel, on the kinds of policy the matrices hold: sweep k moves no entry by more than
    # 0.05^(k-1) (the first sweep by at most 1: a probability, one step, the start distribution)
    lists, starts = pitch(slip)
    A, B = pc.pool()
    x, y = A[:4], B[:4]
    chans = mon.channel_lists(lists)
    xs, ys = brn._policies(x), brn._policies(y)
    F = np.zeros((4, NS, 3))
    D = np.zeros((4, NS))
    for k in range(1, pc.PASS_SWEEPS + 1):
        f = mon.sweep(chans, xs, ys, F, pc.PASS_C)
        d = ocn.solve(lists, starts, x, y, pc.PASS_C, 0.0, k, pc.in_lists(slip))[0]
        # (L_1 is 1 up to the rounding of a row's sum, and a difference of two values below 2 carries a few of their ulps, 2^-52)
        bound = pc.PASS_C ** (k - 1) * (1.0 + 1e-12) + 2.0 ** -48
        assert (np.abs(f - F).max((0, 1)) <= bound).all() and np.abs(d - D).max() <= bound, k
        F, D = f, d
    assert np.abs(f - mon.sweep(chans, xs, ys, F, pc.PASS_C)).max() < THETA
