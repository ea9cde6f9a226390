"""CPU-side checks of the independent Q-learners' C ABI: the symbols are exported, soccer_q_learner_config has the layout
the C compiler gives the header, the constants agree, and argument checks happen before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import q_learning_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_q_learner_create", "soccer_q_learner_destroy", "soccer_q_learner_run", "soccer_q_learner_update",
           "soccer_q_learner_read", "soccer_q_learner_load"]


def test_learner_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert "learners, independent Q" in text
    assert lib.soccer_abi_version() == 3          # nothing that existed changed


def test_config_layout_and_constants_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(soccer_q_learner_config), offsetof(soccer_q_learner_config, discount_factor),
           offsetof(soccer_q_learner_config, alpha), offsetof(soccer_q_learner_config, decay), offsetof(soccer_q_learner_config, explor),
           offsetof(soccer_q_learner_config, q_init), offsetof(soccer_q_learner_config, act_a), offsetof(soccer_q_learner_config, act_b),
           offsetof(soccer_q_learner_config, policy_a), offsetof(soccer_q_learner_config, policy_b));
    printf("%d %d %d %llu\\n", SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM, SOCCER_QL_FIXED, (unsigned long long)SOCCER_MQ_MAX_LANES);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.QLearnerConfig
    assert got == [C.sizeof(M), M.discount_factor.offset, M.alpha.offset, M.decay.offset, M.explor.offset, M.q_init.offset,
                   M.act_a.offset, M.act_b.offset, M.policy_a.offset, M.policy_b.offset,
                   _lib.QL_GREEDY, _lib.QL_UNIFORM, _lib.QL_FIXED, _lib.MQ_MAX_LANES]
    assert (_lib.QL_GREEDY, _lib.QL_UNIFORM, _lib.QL_FIXED) == (0, 1, 2)


@pytest.mark.parametrize("kw,msg", [
    (dict(discount_factor=1.0), "discount_factor"),
    (dict(discount_factor=-0.1), "discount_factor"),
    (dict(discount_factor=float("nan")), "discount_factor"),
    (dict(alpha=1.5), "alpha"),
    (dict(decay=0.0), "decay"),
    (dict(decay=1.01), "decay"),
    (dict(explor=-0.1), "explor"),
    (dict(q_init=1.5), "q_init"),
    (dict(act_a="self"), "act_a"),
    (dict(act_b="random"), "act_b"),
    (dict(act_a=np.full((761, 4), 0.25)), "fixed act_a"),
    (dict(act_b=np.full((761, 5), 0.3)), "fixed act_b"),
    (dict(act_b=np.full((10, 5), 0.2)), "fixed act_b"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        q_learning_config(761, **args)


def test_config_carries_the_defaults_and_the_fixed_policies():
    cfg, keep = q_learning_config(761, 0.9)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.act_a, cfg.act_b) == (0.9, 1.0, 0.2, 1.0, _lib.QL_GREEDY, _lib.QL_GREEDY)
    assert cfg.decay == 0.01 ** (1 / 1e6) and keep == [None, None] and not cfg.policy_a and not cfg.policy_b
    pol = np.full((761, 5), 0.2)
    cfg, keep = q_learning_config(761, 0.5, act_a=pol, act_b="uniform")
    assert (cfg.act_a, cfg.act_b) == (_lib.QL_FIXED, _lib.QL_UNIFORM) and cfg.policy_a == keep[0].ctypes.data and not cfg.policy_b
    cfg, keep = q_learning_config(761, 0.5, act_b=pol)
    assert (cfg.act_a, cfg.act_b) == (_lib.QL_GREEDY, _lib.QL_FIXED) and cfg.policy_b == keep[1].ctypes.data and not cfg.policy_a


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = q_learning_config(761, 0.9)
    q = C.c_void_p()
    assert lib.soccer_q_learner_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_q_learner_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_q_learner_update(None, None, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_q_learner_read(None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_q_learner_load(None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_q_learner_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
