"""What can be said without a GPU about the pitches of tests/large_pitch_cases.py: each has the classification its row claims
(which kernels, which state layout, which geometry, where the observation table lives), its named neighbour falls on the other side
of the predicate, no accepted pitch asks for more LDS or has more states than the table says, and the oracle's side of every GPU
test reaches what the case is there for — the last row and column, observation indices with the top bit set, episodes of every
ending — before any device is involved."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_pitch_cases as lp  # noqa: E402
from large_pitch_cases import CASES, NAMES  # noqa: E402


@pytest.mark.parametrize("name", NAMES)
def test_each_case_has_the_classification_its_row_claims(name):
    c = CASES[name]
    assert {k: c[k] for k in c["claim"]} == c["claim"]
    assert (c["kickoffs"], c["nS"]) == (c["claim_kickoffs"], c["claim_nS"])
    assert name == "%dx%d" % (c["w"], c["h"]) and c["W"] == c["w"] + 2 and c["NI"] == c["h"] * c["w"]
    o = Oracle(c["w"], c["h"], 0.0, n=1)
    assert (o.nS, o.W, o.H, o.n_isd, o.n_tuples) == (c["nS"], c["W"], c["H"], c["kickoffs"], c["lut_bytes"] // 2)


def test_the_edges_the_rows_name():
    C = CASES
    assert (C["6x6"]["W"], C["6x6"]["H"] + 2) == (8, 8)
    assert (C["14x8"]["W"], C["14x8"]["H"], C["14x8"]["W"] * C["14x8"]["H"], C["14x8"]["lds_bytes"]) == (16, 8, 128, 70720) and 70720 > 48 * 1024
    assert (C["30x4"]["W"], C["30x4"]["W"] * C["30x4"]["H"], C["30x4"]["NI"]) == (32, 128, 120)
    assert C["5x18"]["W"] * C["5x18"]["H"] == 126 and C["5x19"]["W"] * C["5x19"]["H"] == 133
    assert (C["36x5"]["lut_bytes"], C["36x5"]["nc_bytes"], C["36x5"]["lds_bytes"]) == (144400, 7600 + 64, 152064) and lp.LDS_LINE - 152064 == 1536
    assert C["45x4"]["W"] - 1 == 46 and C["5x36"]["lut_bytes"] == 254016 and C["5x36"]["H"] - 1 == 35
    assert 4 * 191 * 191 + (10 * 191 + 16) * 4 - lp.LDS_LINE == 28          # HW = 191 would be 28 B over the line (191 is prime)
    for name in ("12x14", "30x6", "5x36"):                      # the move/bounds table alone is what these handles ask for
        assert not C[name]["lut_lds"] and 0 < C[name]["lds_bytes"] == C[name]["nc_bytes"] < 48 * 1024
    for name in lp.ACCEPTED_AT_THE_LIMIT:
        assert C[name]["nS"] == lp.LARGEST_NS > 32768
    assert max(c["lds_bytes"] for c in C.values()) == lp.LARGEST_LDS > 150000


@pytest.mark.parametrize("name", NAMES)
def test_the_named_neighbour_falls_on_the_other_side(name):
    c = CASES[name]
    w, h, predicate = c["neighbour"]
    assert c[predicate] != lp.classify(w, h)[predicate]


def test_over_every_accepted_pitch_none_asks_for_more_lds_or_has_more_states():
    accepted = [(w, h) for w in range(1, 124) for h in range(1, 124) if lp.refusal(w, h) is None]
    # the uint16 observation index is what binds: NI = width * height <= 181, and 181 is prime
    assert accepted == [(w, h) for w in range(5, 121) for h in range(4, 121) if w * h <= 180] and len(accepted) == 278
    cls = [lp.classify(w, h) for w, h in accepted]
    in_lds = [c for c in cls if c["lut_lds"]]
    assert max(c["lds_bytes"] for c in in_lds) == lp.LARGEST_LDS == CASES["36x5"]["lds_bytes"]
    assert max(c["lds_bytes"] for c in cls) == lp.LARGEST_LDS            # without the table a handle asks for the moves alone
    assert max(c["nS"] for c in cls) == lp.LARGEST_NS
    assert sorted((c["w"], c["h"]) for c in cls if c["nS"] == lp.LARGEST_NS) == [(5, 36), (6, 30), (9, 20), (10, 18), (12, 15), (15, 12), (18, 10),
                                                                               (20, 9), (30, 6), (36, 5), (45, 4)]
    assert max(c["nS"] for c in in_lds) == lp.LARGEST_NS and max(c["W"] for c in in_lds if c["nS"] == lp.LARGEST_NS) == CASES["45x4"]["W"]
    # every refusal is one of Rules::build's; soccer_create's own (the move/bounds table beyond the line) is never met
    assert {lp.refusal(w, h) for w in range(1, 124) for h in range(1, 124)} - {None} == {
        "Width must be at least 5 columns.", "Height must be at least 4 rows.", "pitch too large (rows/cols must fit int8)",
        "pitch too large (tuple table)", "pitch too large (observation index must fit uint16)"}
    for (w, h), text in lp.REFUSED:
        assert text in lp.refusal(w, h), (w, h)
    # the oracle takes every pitch the library takes, at the sizes where they could part: the largest ones
    for name in lp.ACCEPTED_AT_THE_LIMIT:
        assert Oracle(CASES[name]["w"], CASES[name]["h"], 0.0, n=1).nS == lp.LARGEST_NS


@pytest.mark.parametrize("name", NAMES)
def test_the_sweep_reaches_every_tuple_and_every_ending(name):
    """(a) on the oracle alone, at slip 0.2 and t = max_steps - 1: every live and goal tuple x 25 action pairs"""
    c = CASES[name]
    o1 = Oracle(c["w"], c["h"], 0.2, n=1)
    tup = lp.tuples_of(o1, [1, 2])
    st, aa, ab = lp.sweep_lanes(tup)
    n = len(st)
    assert n % 4 == 3 and n >= 25 * (c["nS"] - 1) and n <= 1_700_000
    assert len(lp.tuples_of(o1, [1])) == c["nS"] - 1
    o = Oracle(c["w"], c["h"], 0.2, n=n, seed=3, autoreset=True, max_steps=lp.MAX_STEPS)
    o.set_state(st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], t=np.full(n, lp.MAX_STEPS - 1), needs_reset=np.zeros(n, np.uint8))
    seen = lp.reach_of_step(c, st, o.step(aa, ab))
    print(name, n, seen)
    floors = lp.sweep_floors(c)
    assert (seen["row"], seen["col"]) == (c["H"] - 1, c["W"] - 1)
    assert seen["final_obs"] == c["nS"] - 1 and (c["nS"] <= 32768 or seen["final_obs"] >= 32768)
    assert seen["plus"] >= floors["plus"] and seen["minus"] >= floors["minus"] and seen["truncated"] >= floors["truncated"]


@pytest.mark.parametrize("name", NAMES)
def test_the_rollout_reaches_the_last_row_and_column_and_every_ending(name):
    """(b) on the oracle alone: T streamed steps from rollout_start"""
    c = CASES[name]
    for slip in lp.SLIPS:
        rng = np.random.default_rng(NAMES.index(name))
        o = Oracle(c["w"], c["h"], slip, n=lp.N, seed=5, autoreset=True, max_steps=lp.MAX_STEPS)
        o.reset()
        st = lp.rollout_start(o, rng)
        o.set_state(**st)
        assert lp.observations(o)[[1, 2, 6]].tolist() == [c["nS"] - 1, 1, c["nS"] - 1]
        acts = rng.integers(0, 5, size=(lp.T, 2, lp.N), dtype=np.int8)
        seen = lp.streamed_run(o, acts)
        print(name, slip, seen)
        assert seen["row"] == c["H"] - 1 and seen["col"] >= c["W"] - 2
        assert c["nS"] <= 32768 or (seen["obs"] >= 32768 and seen["final_obs"] >= 32768)
        for k, v in lp.ROLLOUT_FLOORS.items():
            assert seen[k] >= v, (k, seen[k])
