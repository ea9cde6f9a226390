"""The public surface of the Python layer, pinned: every public method and property of the wrapper classes, the config
functions, the training drivers of planners and SoccerBatch's factories and evaluators keep their names, their signatures
(the text inspect.signature gives, written out here) and, where they had one, their docstrings; and everything that could be
imported from gym_soccer_littman94_amd.core still can be.  No library and no GPU."""
import inspect

import pytest

import gym_soccer_littman94_amd as pkg
from gym_soccer_littman94_amd import core, planners

UPDATE = "(self, obs, act_a, act_b, reward, terminated, next_obs)"
HYPER = "alpha=1.0, decay=0.9999953948404178, explor=0.2, q_init=1.0"
DELTAS = "delta_win=0.01, delta_lose=0.04, delta_decay=1.0"
RANGE = "theta=1e-10, first=0, count=None"

# name -> (signature or "property", has a docstring)
LEARNER = {"run": ("(self, n_steps)", True), "close": ("(self)", False), "update": (UPDATE, True), "steps": ("property", False)}


def population(which, load):
    w = "which=%r, " % which if which else ""
    return dict(LEARNER, alpha=("property", True), read=("(self, first=0, count=None)", True), load=(load, True),
                exploitability=("(self, %s%s)" % (w, RANGE), True),
                cross_play=("(self, %s%s, discount_factor=None)" % (w, RANGE), True),
                meta_game=("(self, %s%s, discount_factor=None, max_pivots=None)" % (w, RANGE), True),
                match_outcomes=("(self, %s%s, continue_prob=None)" % (w, RANGE), True),
                occupancy=("(self, %s%s, continue_prob=None, features=None, values=False)" % (w, RANGE), True))


CLASSES = {
    "DeviceArray": {"download": ("(self, out=None)", False), "download_rows": ("(self, first_row, n_rows)", False),
                    "fill": ("(self, value)", False), "free": ("(self)", False), "row": ("(self, k)", True),
                    "upload": ("(self, host)", False), "upload_rows": ("(self, first_row, host)", True)},
    "MinimaxQLearner": dict(LEARNER, Q=("property", False), V=("property", False), pi_a=("property", False), pi_b=("property", False),
                            visits=("property", False), alpha=("property", False), read=("(self)", True),
                            exploitability=("(self, theta=1e-10)", True),
                            load=("(self, Q, visits=None, alpha=None, steps=None)", True)),
    "QLearner": dict(LEARNER, alpha=("property", False), read=("(self)", True), exploitability=("(self, theta=1e-10)", True),
                     load=("(self, Q_a, Q_b, visits=None, alpha=None, steps=None)", True)),
    "QPopulation": dict(population(None, "(self, Q_a=None, Q_b=None, alpha=None, steps=None, first=0)"),
                        picks=("(self, first=0, count=None)", True), load_picks=("(self, picks, first=0)", True)),
    "OpponentModelPopulation": population("greedy", "(self, Q_a=None, Q_b=None, C_a=None, C_b=None, alpha=None, steps=None, first=0)"),
    "WolfPHCLearner": dict(LEARNER, alpha=("property", False), dscale=("property", False), read=("(self)", True),
                           exploitability=("(self, which='pi', theta=1e-10)", True),
                           load=("(self, Q_a, Q_b, pi_a=None, pi_b=None, avg_a=None, avg_b=None, visits=None, updates=None, "
                                 "alpha=None, dscale=None, steps=None)", True)),
    "WolfPopulation": dict(population("pi", "(self, Q_a=None, Q_b=None, pi_a=None, pi_b=None, avg_a=None, avg_b=None, updates=None, "
                                            "alpha=None, dscale=None, steps=None, first=0)"),
                           dscale=("property", True), adopt=("(self, player, src, src_player, which='pi')", True),
                           challengers=("(self, against, which='pi', **hyper)", True)),
    "MinimaxQPopulation": population(None, "(self, Q=None, V=None, pi_a=None, pi_b=None, alpha=None, steps=None, first=0)"),
    "GradientPlay": {"run": ("(self, n_steps, trace=False)", True), "close": ("(self)", False), "read": ("(self)", True),
                     "load": ("(self, pi_a=None, pi_b=None, prev_a=None, prev_b=None, payoff=None, steps=None, **ignored)", True),
                     "weights": ("(self, w_a=None, w_b=None)", True), "exploitability": ("(self, theta=None)", True),
                     "cross_play": ("(self, theta=None)", True), "meta_game": ("(self, theta=None, max_pivots=None)", True)},
}

CONFIGS = {
    "minimax_q_config": "(nS, discount_factor, %s, opponent='uniform')" % HYPER,
    "q_learning_config": "(nS, discount_factor, %s, act_a='greedy', act_b='greedy')" % HYPER,
    "league_config": "(nS, act_a, act_b, league_policies, league_weights)",
    "q_population_config": "(n, nS, discount_factor, %s, act_a='greedy', act_b='greedy', league=None)" % HYPER,
    "om_population_config": "(n, nS, discount_factor, %s, act_a='greedy', act_b='greedy')" % HYPER,
    "wolf_phc_config": "(nS, discount_factor, %s, %s, act_a='learn', act_b='learn')" % (HYPER, DELTAS),
    "wolf_population_config": "(n, nS, discount_factor, %s, %s, act_a='learn', act_b='learn')" % (HYPER, DELTAS),
    "minimax_q_population_config": "(n, nS, discount_factor, %s, opponent='uniform')" % HYPER,
}

DRIVER = "(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, "
DRIVERS = {
    "minimax_q_learning": DRIVER + "opponent='uniform')",
    "q_learning": DRIVER + "act_a='greedy', act_b='greedy')",
    "q_population": DRIVER + "act_a='greedy', act_b='greedy', first=0, count=None, league_policies=None, league_weights=None)",
    "om_population": DRIVER + "act_a='greedy', act_b='greedy', first=0, count=None)",
    "wolf_phc": DRIVER + DELTAS + ", act_a='learn', act_b='learn')",
    "wolf_population": DRIVER + DELTAS + ", act_a='learn', act_b='learn', first=0, count=None)",
    "minimax_q_population": DRIVER + "opponent='uniform', first=0, count=None)",
}

PAIRS = "(self, pi_a, pi_b, theta, "
BATCH = {
    "minimax_q": "(self, discount_factor, %s, opponent='uniform')" % HYPER,
    "q_learning": "(self, discount_factor, %s, act_a='greedy', act_b='greedy')" % HYPER,
    "q_population": "(self, discount_factor, %s, act_a='greedy', act_b='greedy', league_policies=None, league_weights=None)" % HYPER,
    "om_population": "(self, discount_factor, %s, act_a='greedy', act_b='greedy')" % HYPER,
    "wolf_phc": "(self, discount_factor, %s, %s, act_a='learn', act_b='learn')" % (HYPER, DELTAS),
    "wolf_population": "(self, discount_factor, %s, %s, act_a='learn', act_b='learn')" % (HYPER, DELTAS),
    "minimax_q_population": "(self, discount_factor, %s, opponent='uniform')" % HYPER,
    "best_response": "(self, policy, player, theta, discount_factor, max_sweeps=1000000)",
    "evaluate_policies": PAIRS + "discount_factor, max_sweeps=1000000)",
    "cross_play": PAIRS + "discount_factor, max_sweeps=1000000, pairs_per_pass=0, values=False)",
    "match_outcomes": PAIRS + "continue_prob, max_sweeps=1000000, pairs_per_pass=0, values=False)",
    "occupancy": PAIRS + "continue_prob, features=None, values=False, max_sweeps=1000000, pairs_per_pass=0)",
    "policy_gradient": PAIRS + "discount_factor, w_a=None, w_b=None, normalize=False, values=False, max_sweeps=1000000, pairs_per_pass=0)",
    "gradient_play": "(self, n_a=1, n_b=1, discount_factor=0.9, eta_a=1.0, eta_b=1.0, optimism=0.0, normalize=True, theta=1e-10, "
                     "max_sweeps=1000000, pairs_per_pass=0, pi_a=None, pi_b=None)",
    "solve_meta_game": "(self, payoff, max_pivots=None, path=0, pivots_per_sync=0)",
}


def described(obj):
    return bool(obj.__doc__ and obj.__doc__.strip())


@pytest.mark.parametrize("name", list(CLASSES))
def test_wrapper_class_keeps_its_public_names_signatures_and_docstrings(name):
    cls = getattr(core, name)
    assert getattr(pkg, name) is cls and described(cls)
    assert sorted(n for n in dir(cls) if not n.startswith("_")) == sorted(CLASSES[name])
    for attr, (sig, doc) in CLASSES[name].items():
        static = inspect.getattr_static(cls, attr)
        if sig == "property":
            assert isinstance(static, property), "%s.%s is no longer a property" % (name, attr)
        else:
            assert str(inspect.signature(getattr(cls, attr))) == sig, "%s.%s" % (name, attr)
        assert described(static) or not doc, "%s.%s has lost its docstring" % (name, attr)


@pytest.mark.parametrize("owner, table", [(core, CONFIGS), (planners, DRIVERS), (core.SoccerBatch, BATCH)],
                         ids=["configs", "drivers", "batch"])
def test_functions_keep_their_signatures_and_docstrings(owner, table):
    for name, sig in table.items():
        fn = getattr(owner, name)
        assert str(inspect.signature(fn)) == sig, name
        assert described(fn), "%s has lost its docstring" % name


def test_core_still_exports_what_it_did():
    for name in list(CLASSES) + list(CONFIGS) + ["SoccerBatch", "om_derive", "om_model", "meta_lds_bytes", "_meta_of_cross_play"]:
        assert callable(getattr(core, name)), name
    assert pkg.__all__ == ["SoccerBatch", "DeviceArray", "GradientPlay", "MinimaxQLearner", "MinimaxQPopulation",
                           "OpponentModelPopulation", "QLearner", "QPopulation", "WolfPHCLearner", "WolfPopulation",
                           "SoccerSimultaneousEnv", "VectorSoccerEnv", "make", "register_all", "planners", "policies",
                           "install_as_gym_soccer"]
