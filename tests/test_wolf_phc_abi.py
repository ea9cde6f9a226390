"""CPU-side checks of the policy hill-climbers' C ABI: the symbols are exported, soccer_wolf_phc_config and
soccer_wolf_phc_state have the layout the C compiler gives the header, the constants agree, and argument checks happen
before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import wolf_phc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_wolf_phc_create", "soccer_wolf_phc_destroy", "soccer_wolf_phc_run", "soccer_wolf_phc_update",
           "soccer_wolf_phc_read", "soccer_wolf_phc_load"]
CONFIG_FIELDS = ["discount_factor", "alpha", "decay", "explor", "q_init", "delta_win", "delta_lose", "delta_decay", "act_a", "act_b",
                 "policy_a", "policy_b"]
STATE_FIELDS = ["Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "visits", "updates", "alpha", "dscale", "steps"]


def test_learner_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert "learners, policy hill-climbing" in text
    assert lib.soccer_abi_version() == 3          # nothing that existed changed


def test_struct_layouts_and_constants_match_the_header(tmp_path):
    lines = ['printf("%%zu\\n", sizeof(%s));' % s for s in ("soccer_wolf_phc_config", "soccer_wolf_phc_state")]
    lines += ['printf("%%zu\\n", offsetof(soccer_wolf_phc_config, %s));' % f for f in CONFIG_FIELDS]
    lines += ['printf("%%zu\\n", offsetof(soccer_wolf_phc_state, %s));' % f for f in STATE_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    %s
    printf("%%d %%d %%d %%llu\\n", SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM, SOCCER_PHC_FIXED, (unsigned long long)SOCCER_MQ_MAX_LANES);
    return 0;
}
""" % "\n    ".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M, S = _lib.WolfPHCConfig, _lib.WolfPHCState
    assert [n for n, _ in M._fields_] == CONFIG_FIELDS and [n for n, _ in S._fields_] == STATE_FIELDS
    assert got == [C.sizeof(M), C.sizeof(S)] + [getattr(M, f).offset for f in CONFIG_FIELDS] + [getattr(S, f).offset for f in STATE_FIELDS] + \
        [_lib.PHC_LEARN, _lib.PHC_UNIFORM, _lib.PHC_FIXED, _lib.MQ_MAX_LANES]
    assert (_lib.PHC_LEARN, _lib.PHC_UNIFORM, _lib.PHC_FIXED) == (0, 1, 2)


@pytest.mark.parametrize("kw,msg", [
    (dict(discount_factor=1.0), "discount_factor"),
    (dict(discount_factor=float("nan")), "discount_factor"),
    (dict(alpha=1.5), "alpha"),
    (dict(decay=0.0), "decay"),
    (dict(explor=-0.1), "explor"),
    (dict(q_init=1.5), "q_init"),
    (dict(delta_win=-0.01), "delta_win"),
    (dict(delta_win=1.5), "delta_win"),
    (dict(delta_lose=float("nan")), "delta_lose"),
    (dict(delta_lose=1.01), "delta_lose"),
    (dict(delta_decay=0.0), "delta_decay"),
    (dict(delta_decay=1.01), "delta_decay"),
    (dict(act_a="greedy"), "act_a"),
    (dict(act_b="self"), "act_b"),
    (dict(act_a=np.full((761, 4), 0.25)), "fixed act_a"),
    (dict(act_b=np.full((761, 5), 0.3)), "fixed act_b"),
    (dict(act_b=np.full((10, 5), 0.2)), "fixed act_b"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        wolf_phc_config(761, **args)


def test_config_carries_the_defaults_and_the_fixed_policies():
    cfg, keep = wolf_phc_config(761, 0.9)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.act_a, cfg.act_b) == (0.9, 1.0, 0.2, 1.0, _lib.PHC_LEARN, _lib.PHC_LEARN)
    assert (cfg.delta_win, cfg.delta_lose, cfg.delta_decay) == (0.01, 0.04, 1.0)
    assert cfg.decay == 0.01 ** (1 / 1e6) and keep == [None, None] and not cfg.policy_a and not cfg.policy_b
    pol = np.full((761, 5), 0.2)
    cfg, keep = wolf_phc_config(761, 0.5, act_a=pol, act_b="uniform", delta_win=0.04, delta_decay=0.5)
    assert (cfg.act_a, cfg.act_b) == (_lib.PHC_FIXED, _lib.PHC_UNIFORM) and cfg.policy_a == keep[0].ctypes.data and not cfg.policy_b
    assert (cfg.delta_win, cfg.delta_lose, cfg.delta_decay) == (0.04, 0.04, 0.5)
    cfg, keep = wolf_phc_config(761, 0.5, act_b=pol)
    assert (cfg.act_a, cfg.act_b) == (_lib.PHC_LEARN, _lib.PHC_FIXED) and cfg.policy_b == keep[1].ctypes.data and not cfg.policy_a


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = wolf_phc_config(761, 0.9)
    q = C.c_void_p()
    state = _lib.WolfPHCState()
    assert lib.soccer_wolf_phc_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_wolf_phc_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_wolf_phc_update(None, None, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_wolf_phc_read(None, None, C.byref(state)) == _lib.E_INVALID
    assert lib.soccer_wolf_phc_load(None, None, C.byref(state)) == _lib.E_INVALID
    assert lib.soccer_wolf_phc_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
