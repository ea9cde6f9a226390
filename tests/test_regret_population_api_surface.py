"""The public surface the regret-matching population adds to the Python layer, pinned as tests/test_python_api_surface.py pins
the rest: the class's public names, signatures and docstrings, its config function, its driver in planners and its factories;
it is importable from learners, core and the package; and __all__ stays what it was.  No library and no GPU."""
import inspect

import gym_soccer_littman94_amd as pkg
from gym_soccer_littman94_amd import core, learners, planners
from gym_soccer_littman94_amd.envs import VectorSoccerEnv

from test_python_api_surface import HYPER, described, population

FLAGS = "plus=True, linear=False, act_a='learn', act_b='learn'"
CLASS = population("avg", "(self, Q_a=None, Q_b=None, R_a=None, R_b=None, Z_a=None, Z_b=None, updates=None, alpha=None, steps=None, first=0)")


def test_the_class_is_importable_from_learners_core_and_the_package():
    assert pkg.RegretPopulation is core.RegretPopulation is learners.RegretPopulation and described(pkg.RegretPopulation)
    assert "RegretPopulation" not in pkg.__all__                        # __all__ stays what tests/test_python_api_surface.py pins
    for name in ("regret_population_config", "regret_policy", "regret_average"):
        assert getattr(core, name) is getattr(learners, name) and described(getattr(core, name))


def test_the_class_has_these_public_names_signatures_and_docstrings():
    cls = core.RegretPopulation
    assert sorted(n for n in dir(cls) if not n.startswith("_")) == sorted(CLASS)
    for attr, (sig, doc) in CLASS.items():
        static = inspect.getattr_static(cls, attr)
        if sig == "property":
            assert isinstance(static, property), attr
        else:
            assert str(inspect.signature(getattr(cls, attr))) == sig, attr
        assert described(static) or not doc, attr
    assert cls._C == "soccer_regret_population" and cls._WHICH == {"avg": ("avg_a", "avg_b"), "pi": ("pi_a", "pi_b")}
    assert [f[0] for f in cls._FIELDS] == ["Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b", "updates", "alpha", "steps"]
    assert issubclass(cls, learners._Population)


def test_the_functions_have_these_signatures_and_docstrings():
    for owner, name, sig in ((core, "regret_population_config", "(n, nS, discount_factor, %s, %s)" % (HYPER, FLAGS)),
                             (core.SoccerBatch, "regret_population", "(self, discount_factor, %s, %s)" % (HYPER, FLAGS)),
                             (VectorSoccerEnv, "regret_population", "(self, discount_factor, **params)"),
                             (planners, "regret_population", "(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, "
                                                            "%s, first=0, count=None)" % FLAGS)):
        fn = getattr(owner, name)
        assert str(inspect.signature(fn)) == sig, name
        assert described(fn), name
