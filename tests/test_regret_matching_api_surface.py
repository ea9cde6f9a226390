"""The public surface the regret matchers of one table add to the Python layer, pinned as tests/test_python_api_surface.py pins
the rest: the class's public names, signatures and docstrings, its config function, its driver in planners and its factories;
it is importable from learners, core and the package; and __all__ stays what it was.  No library and no GPU."""
import inspect

import numpy as np
import pytest

import gym_soccer_littman94_amd as pkg
from gym_soccer_littman94_amd import _lib, core, learners, planners
from gym_soccer_littman94_amd.envs import VectorSoccerEnv

from test_python_api_surface import HYPER, LEARNER, described

FLAGS = "plus=True, linear=False, act_a='learn', act_b='learn'"
CLASS = dict(LEARNER, alpha=("property", False), read=("(self)", True), exploitability=("(self, which='avg', theta=1e-10)", True),
             load=("(self, Q_a, Q_b, R_a=None, R_b=None, Z_a=None, Z_b=None, visits=None, updates=None, alpha=None, steps=None)", True))


def test_the_class_is_importable_from_learners_core_and_the_package():
    assert pkg.RegretLearner is core.RegretLearner is learners.RegretLearner and described(pkg.RegretLearner)
    assert "RegretLearner" not in pkg.__all__                           # __all__ stays what tests/test_python_api_surface.py pins
    assert core.regret_learner_config is learners.regret_learner_config and described(core.regret_learner_config)


def test_the_class_has_these_public_names_signatures_and_docstrings():
    cls = core.RegretLearner
    assert sorted(n for n in dir(cls) if not n.startswith("_")) == sorted(CLASS)
    for attr, (sig, doc) in CLASS.items():
        static = inspect.getattr_static(cls, attr)
        if sig == "property":
            assert isinstance(static, property), attr
        else:
            assert str(inspect.signature(getattr(cls, attr))) == sig, attr
        assert described(static) or not doc, attr
    assert cls._C == "soccer_regret_learner" and cls._STATE is _lib.RegretLearnerState
    assert cls._WHICH == {"avg": ("avg_a", "avg_b"), "pi": ("pi_a", "pi_b")}
    assert [f[0] for f in cls._FIELDS] == ["Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b", "visits", "updates", "alpha", "steps"]
    assert issubclass(cls, learners._Learner) and not issubclass(cls, learners._Population)


def test_the_functions_have_these_signatures_and_docstrings():
    for owner, name, sig in ((core, "regret_learner_config", "(nS, discount_factor, %s, %s)" % (HYPER, FLAGS)),
                             (core.SoccerBatch, "regret_matching", "(self, discount_factor, **params)"),
                             (VectorSoccerEnv, "regret_matching", "(self, discount_factor, **params)"),
                             (planners, "regret_matching", "(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, "
                                                          "%s)" % FLAGS)):
        fn = getattr(owner, name)
        assert str(inspect.signature(fn)) == sig, name
        assert described(fn), name


def test_the_config_function_checks_before_any_library_call():
    cfg, keep = core.regret_learner_config(20, 0.9, plus=False, linear=True, act_b=np.full((20, 5), 0.2))
    assert (cfg.act_a, cfg.act_b, cfg.plus, cfg.linear) == (_lib.PHC_LEARN, _lib.PHC_FIXED, 0, 1)
    assert not cfg.policy_a and cfg.policy_b == keep[1].ctypes.data
    for kw, msg in ((dict(plus=2), "plus"), (dict(linear="yes"), "linear"), (dict(explor=1.5), "explor"), (dict(act_a="greedy"), "act_a"),
                    (dict(act_b=np.full((20, 5), 0.3)), "state 0")):
        with pytest.raises(AssertionError, match=msg):
            core.regret_learner_config(20, 0.9, **kw)
