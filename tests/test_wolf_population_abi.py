"""CPU-side checks of the C ABI of the population of policy hill-climbers: the symbols are exported and declared,
soccer_wolf_population_config and soccer_wolf_population_state have the layout the C compiler gives the header, nothing that
existed changed, and argument checks happen before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import wolf_population_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_wolf_population_create", "soccer_wolf_population_destroy", "soccer_wolf_population_run", "soccer_wolf_population_update",
           "soccer_wolf_population_read", "soccer_wolf_population_load", "soccer_wolf_population_adopt"]
FIELDS = ["discount_factor", "alpha", "decay", "explor", "q_init", "delta_win", "delta_lose", "delta_decay", "act_a", "act_b", "policy_a",
          "policy_b", "policy_a_per_member", "policy_b_per_member", "alpha_per_member", "decay_per_member", "explor_per_member",
          "discount_factor_per_member", "delta_win_per_member", "delta_lose_per_member", "delta_decay_per_member"]
STATE = ["Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "updates", "alpha", "dscale", "steps"]


def test_population_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert "learners, a population of policy hill-climbers" in text
    assert re.search(r"soccer_wolf_population_\*,[^;]*were ADDED", text)
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    assert re.search(r"#define SOCCER_ABI_VERSION 3\b", text)


def test_config_and_state_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    printf("%%zu %%zu %%zu", sizeof(soccer_wolf_population_config), sizeof(soccer_wolf_phc_config), sizeof(soccer_wolf_population_state));
%s
%s
    printf("\\n");
    return 0;
}
""" % ("\n".join('    printf(" %%zu", offsetof(soccer_wolf_population_config, %s));' % f for f in FIELDS),
       "\n".join('    printf(" %%zu", offsetof(soccer_wolf_population_state, %s));' % f for f in STATE)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M, S = _lib.WolfPopulationConfig, _lib.WolfPopulationState
    assert got == [C.sizeof(M), C.sizeof(_lib.WolfPHCConfig), C.sizeof(S)] + [getattr(M, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATE]
    # soccer_wolf_phc_config's fields, in place, then the per-member pointers
    assert [f for f, _ in M._fields_] == FIELDS and [f for f, _ in _lib.WolfPHCConfig._fields_] == FIELDS[:12]
    assert all(getattr(M, f).offset == getattr(_lib.WolfPHCConfig, f).offset for f in FIELDS[:12])
    assert [f for f, _ in S._fields_] == STATE


@pytest.mark.parametrize("kw,msg", [
    (dict(discount_factor=1.0), "discount_factor"),
    (dict(discount_factor=np.full(8, 1.0)), "per-member discount_factor"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=np.array([0.5] * 7 + [-0.1])), "per-member alpha"),
    (dict(alpha=np.full(9, 0.5)), "one value per lane"),
    (dict(decay=0.0), "decay"),
    (dict(decay=np.array([1.0] * 7 + [float("nan")])), "per-member decay"),
    (dict(explor=-0.1), "explor"),
    (dict(explor=np.linspace(0.0, 1.1, 8)), "per-member explor"),
    (dict(q_init=1.5), "q_init"),
    (dict(delta_win=1.5), "delta_win"),
    (dict(delta_win=np.linspace(-0.1, 1.0, 8)), "per-member delta_win"),
    (dict(delta_lose=-0.5), "delta_lose"),
    (dict(delta_lose=np.full(8, 2.0)), "per-member delta_lose"),
    (dict(delta_decay=0.0), "delta_decay"),
    (dict(delta_decay=np.linspace(0.0, 1.0, 8)), "per-member delta_decay"),
    (dict(act_a="greedy"), "act_a"),
    (dict(act_b=np.full((761, 5), 0.3)), "fixed act_b"),
    (dict(act_b=np.full((7, 761, 5), 0.2)), "fixed act_b"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        wolf_population_config(8, 761, **args)


def test_config_carries_scalars_arrays_and_the_fixed_policies():
    cfg, ((shared, each), arrays) = wolf_population_config(8, 761, 0.9)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.delta_win, cfg.delta_lose, cfg.delta_decay, cfg.act_a, cfg.act_b) == \
        (0.9, 1.0, 0.2, 1.0, 0.01, 0.04, 1.0, _lib.PHC_LEARN, _lib.PHC_LEARN)
    assert not any(getattr(cfg, f) for f in FIELDS[10:])
    pol = np.full((761, 5), 0.2); per = np.full((8, 761, 5), 0.2); e = np.linspace(0.0, 1.0, 8); w = np.linspace(0.1, 0.9, 8)
    cfg, ((shared, each), arrays) = wolf_population_config(8, 761, 0.9, explor=e, delta_win=w, act_a=pol, act_b=per)
    assert (cfg.act_a, cfg.act_b) == (_lib.PHC_FIXED, _lib.PHC_FIXED)
    assert cfg.policy_a == shared[0].ctypes.data and not cfg.policy_b and not cfg.policy_a_per_member and cfg.policy_b_per_member == each[1].ctypes.data
    assert cfg.explor_per_member == arrays["explor"].ctypes.data and cfg.delta_win_per_member == arrays["delta_win"].ctypes.data
    assert not cfg.alpha_per_member and not cfg.decay_per_member and not cfg.discount_factor_per_member and not cfg.delta_decay_per_member
    np.testing.assert_array_equal(arrays["explor"], e); np.testing.assert_array_equal(arrays["delta_win"], w)
    cfg, _ = wolf_population_config(8, 761, 0.9, act_a="uniform")
    assert (cfg.act_a, cfg.act_b) == (_lib.PHC_UNIFORM, _lib.PHC_LEARN)


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = wolf_population_config(8, 761, 0.9)
    q = C.c_void_p()
    st = _lib.WolfPopulationState()
    assert lib.soccer_wolf_population_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_wolf_population_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_wolf_population_update(None, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_wolf_population_read(None, None, 0, 0, C.byref(st)) == _lib.E_INVALID
    assert lib.soccer_wolf_population_load(None, None, 0, 0, C.byref(st)) == _lib.E_INVALID
    assert lib.soccer_wolf_population_adopt(None, None, 0, None, 0, 0) == _lib.E_INVALID
    assert lib.soccer_wolf_population_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
