"""CPU-side checks of the C ABI of the population of minimax-Q learners: the symbols are exported and declared,
soccer_minimax_q_population_config has the layout the C compiler gives the header, nothing that existed changed, and argument
checks happen before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import minimax_q_population_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_minimax_q_population_create", "soccer_minimax_q_population_destroy", "soccer_minimax_q_population_run",
           "soccer_minimax_q_population_update", "soccer_minimax_q_population_read", "soccer_minimax_q_population_load"]
FIELDS = ["discount_factor", "alpha", "decay", "explor", "q_init", "opponent", "reserved_", "opponent_policy", "opponent_policy_per_member",
          "alpha_per_member", "decay_per_member", "explor_per_member", "discount_factor_per_member"]


def test_population_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert "learners, a population of minimax-Q learners" in text
    assert re.search(r"soccer_minimax_q_population_\*,[^;]*were ADDED", text)
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    assert re.search(r"#define SOCCER_ABI_VERSION 3\b", text)


def test_config_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    printf("%%zu %%zu", sizeof(soccer_minimax_q_population_config), sizeof(soccer_minimax_q_config));
%s
    printf("\\n");
    return 0;
}
""" % "\n".join('    printf(" %%zu", offsetof(soccer_minimax_q_population_config, %s));' % f for f in FIELDS))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.MinimaxQPopulationConfig
    assert got == [C.sizeof(M), C.sizeof(_lib.MinimaxQConfig)] + [getattr(M, f).offset for f in FIELDS]
    # soccer_minimax_q_config's fields, in place, then the per-member pointers
    assert [f for f, _ in M._fields_] == FIELDS and [f for f, _ in _lib.MinimaxQConfig._fields_] == FIELDS[:8]
    assert all(getattr(M, f).offset == getattr(_lib.MinimaxQConfig, f).offset for f in FIELDS[:8])


def _bad_each():
    p = np.full((8, 761, 5), 0.2); p[5, 17] = [0.5, 0.5, 0.5, 0.0, 0.0]
    return p


def _bad_shared():
    p = np.full((761, 5), 0.2); p[3, 2] = -0.2; p[3, 1] = 0.6
    return p


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
    (dict(explor=np.full((8, 1), 0.5)), "one value per lane"),
    (dict(q_init=1.5), "q_init"),
    (dict(opponent="greedy"), "opponent must be"),
    (dict(opponent=np.full((760, 5), 0.2)), "fixed opponent must be"),
    (dict(opponent=np.full((7, 761, 5), 0.2)), "fixed opponent must be"),
    (dict(opponent=_bad_shared()), "state 3 is not"),
    (dict(opponent=_bad_each()), "member 5, state 17 is not"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        minimax_q_population_config(8, 761, **args)


def test_config_carries_scalars_arrays_and_the_fixed_policy():
    cfg, ((shared, each), arrays) = minimax_q_population_config(8, 761, 0.9)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.opponent, cfg.reserved_) == (0.9, 1.0, 0.2, 1.0, _lib.MQ_UNIFORM, 0)
    assert not any(getattr(cfg, f) for f in FIELDS[7:]) and shared is None and each is None
    pol = np.full((761, 5), 0.2); per = np.full((8, 761, 5), 0.2); e = np.linspace(0.0, 1.0, 8); g = np.linspace(0.1, 0.9, 8)
    cfg, ((shared, each), arrays) = minimax_q_population_config(8, 761, g, explor=e, opponent=pol)
    assert cfg.opponent == _lib.MQ_FIXED and cfg.opponent_policy == shared.ctypes.data and not cfg.opponent_policy_per_member
    assert cfg.explor_per_member == arrays["explor"].ctypes.data and cfg.discount_factor_per_member == arrays["discount_factor"].ctypes.data
    assert not cfg.alpha_per_member and not cfg.decay_per_member
    np.testing.assert_array_equal(arrays["explor"], e); np.testing.assert_array_equal(arrays["discount_factor"], g)
    cfg, ((shared, each), arrays) = minimax_q_population_config(8, 761, 0.9, opponent=per)
    assert cfg.opponent == _lib.MQ_FIXED and not cfg.opponent_policy and cfg.opponent_policy_per_member == each.ctypes.data
    cfg, _ = minimax_q_population_config(8, 761, 0.9, opponent="self")
    assert cfg.opponent == _lib.MQ_SELF and not cfg.opponent_policy and not cfg.opponent_policy_per_member


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = minimax_q_population_config(8, 761, 0.9)
    q = C.c_void_p()
    assert lib.soccer_minimax_q_population_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_minimax_q_population_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_minimax_q_population_update(None, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_population_read(None, None, 0, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_population_load(None, None, 0, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_population_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
