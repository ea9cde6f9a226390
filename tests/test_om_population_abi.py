"""CPU-side checks of the opponent-modelling population's C ABI: the symbols are exported and declared,
soccer_om_population_config has the layout the C compiler gives the header, nothing that existed changed, and argument checks
happen before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import om_derive, om_model, om_population_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_om_population_create", "soccer_om_population_destroy", "soccer_om_population_run", "soccer_om_population_update",
           "soccer_om_population_read", "soccer_om_population_load"]
FIELDS = ["discount_factor", "alpha", "decay", "explor", "q_init", "act_a", "act_b", "policy_a", "policy_b",
          "alpha_per_member", "decay_per_member", "explor_per_member", "discount_factor_per_member"]


def test_population_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert "learners, a population of opponent-modelling Q-learners" in text
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    assert re.search(r"#define SOCCER_ABI_VERSION 3\b", text)


def test_config_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    printf("%%zu %%zu", sizeof(soccer_om_population_config), sizeof(soccer_q_population_config));
%s
    printf("\\n");
    return 0;
}
""" % "\n".join('    printf(" %%zu", offsetof(soccer_om_population_config, %s));' % f for f in FIELDS))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.OMPopulationConfig
    assert got == [C.sizeof(M), C.sizeof(_lib.QPopulationConfig)] + [getattr(M, f).offset for f in FIELDS]
    # soccer_q_population_config's fields, in place
    assert [f for f, _ in M._fields_] == FIELDS
    assert all(getattr(M, f).offset == getattr(_lib.QPopulationConfig, f).offset for f in FIELDS)


@pytest.mark.parametrize("kw,msg", [
    (dict(discount_factor=1.0), "discount_factor"),
    (dict(discount_factor=np.full(8, 1.0)), "per-member discount_factor"),
    (dict(alpha=1.5), "alpha"),
    (dict(alpha=np.full(9, 0.5)), "one value per lane"),
    (dict(decay=0.0), "decay"),
    (dict(explor=np.linspace(0.0, 1.1, 8)), "per-member explor"),
    (dict(q_init=1.5), "q_init"),
    (dict(act_a="self"), "act_a"),
    (dict(act_b=np.full((761, 5), 0.3)), "fixed act_b"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        om_population_config(8, 761, **args)


def test_config_carries_scalars_arrays_and_the_fixed_policy():
    cfg, (pols, arrays) = om_population_config(8, 761, 0.9)
    assert isinstance(cfg, _lib.OMPopulationConfig)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.act_a, cfg.act_b) == (0.9, 1.0, 0.2, 1.0, _lib.QL_GREEDY, _lib.QL_GREEDY)
    assert not any((cfg.policy_a, cfg.policy_b, cfg.alpha_per_member, cfg.decay_per_member, cfg.explor_per_member, cfg.discount_factor_per_member))
    pol = np.full((761, 5), 0.2); e = np.linspace(0.0, 1.0, 8); g = np.linspace(0.1, 0.9, 8)
    cfg, (pols, arrays) = om_population_config(8, 761, g, explor=e, act_a=pol, act_b="uniform")
    assert (cfg.act_a, cfg.act_b) == (_lib.QL_FIXED, _lib.QL_UNIFORM) and cfg.policy_a == pols[0].ctypes.data and not cfg.policy_b
    assert cfg.explor_per_member == arrays["explor"].ctypes.data and cfg.discount_factor_per_member == arrays["discount_factor"].ctypes.data
    assert not cfg.alpha_per_member and not cfg.decay_per_member


def test_the_python_derive_and_model_follow_the_definition():
    Q = np.zeros((2, 5, 5)); Q[0, 3, 4] = 1.0; Q[0, 1, 0] = 0.5; Q[1] = 0.25
    V, g = om_derive(Q, np.array([[3, 0, 0, 0, 1], [0, 0, 0, 0, 0]], np.uint64))
    assert V.tolist() == [(3.0 * 0.5) / 4.0, ((((0.25 + 0.25) + 0.25) + 0.25) + 0.25) / 5.0] and g.tolist() == [1, 0]
    m = om_model(np.array([[3, 0, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 0, 0]], np.uint64))
    assert m[0].tolist() == [0.75, 0.0, 0.0, 0.0, 0.25] and m[1].tolist() == [0.2] * 5
    assert np.abs(m.sum(1) - 1.0).max() <= 2.0 ** -52 and np.allclose(m[2], [1 / 3, 1 / 3, 1 / 3, 0, 0], rtol=0, atol=1e-15)


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = om_population_config(8, 761, 0.9)
    q = C.c_void_p()
    assert lib.soccer_om_population_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_om_population_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_om_population_update(None, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_om_population_read(None, None, 0, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_om_population_load(None, None, 0, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_om_population_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
