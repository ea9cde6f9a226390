"""CPU-side checks of the minimax-Q learner's C ABI: the symbols are exported, soccer_minimax_q_config has the layout the C
compiler gives the header, the constants agree, and argument checks happen before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import minimax_q_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["soccer_minimax_q_create", "soccer_minimax_q_destroy", "soccer_minimax_q_run", "soccer_minimax_q_update",
           "soccer_minimax_q_read", "soccer_minimax_q_load"]


def test_learner_symbols_are_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES and re.search(r"\bint %s\(" % name, text)
    assert lib.soccer_abi_version() == 3          # nothing that existed changed


def test_config_layout_and_constants_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "soccer_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(soccer_minimax_q_config), offsetof(soccer_minimax_q_config, discount_factor),
           offsetof(soccer_minimax_q_config, alpha), offsetof(soccer_minimax_q_config, decay), offsetof(soccer_minimax_q_config, explor),
           offsetof(soccer_minimax_q_config, q_init), offsetof(soccer_minimax_q_config, opponent),
           offsetof(soccer_minimax_q_config, opponent_policy));
    printf("%d %d %d %llu %u %u %u\\n", SOCCER_MQ_UNIFORM, SOCCER_MQ_SELF, SOCCER_MQ_FIXED, (unsigned long long)SOCCER_MQ_MAX_LANES,
           SOCCER_MISUSE_FROZEN, SOCCER_MISUSE_ACTION, SOCCER_MISUSE_OBSERVATION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.MinimaxQConfig
    assert got == [C.sizeof(M), M.discount_factor.offset, M.alpha.offset, M.decay.offset, M.explor.offset, M.q_init.offset,
                   M.opponent.offset, M.opponent_policy.offset,
                   _lib.MQ_UNIFORM, _lib.MQ_SELF, _lib.MQ_FIXED, _lib.MQ_MAX_LANES,
                   _lib.MISUSE_FROZEN, _lib.MISUSE_ACTION, _lib.MISUSE_OBSERVATION]


@pytest.mark.parametrize("kw,msg", [
    (dict(discount_factor=1.0), "discount_factor"),
    (dict(discount_factor=-0.1), "discount_factor"),
    (dict(discount_factor=float("nan")), "discount_factor"),
    (dict(alpha=1.5), "alpha"),
    (dict(decay=0.0), "decay"),
    (dict(decay=1.01), "decay"),
    (dict(explor=-0.1), "explor"),
    (dict(q_init=1.5), "q_init"),
    (dict(opponent="random"), "opponent"),
    (dict(opponent=np.full((761, 4), 0.25)), "fixed opponent"),
    (dict(opponent=np.full((761, 5), 0.3)), "fixed opponent"),
    (dict(opponent=np.full((10, 5), 0.2)), "fixed opponent"),
])
def test_python_argument_checks_raise_before_any_library_call(kw, msg):
    args = dict(discount_factor=0.9)
    args.update(kw)
    with pytest.raises(AssertionError, match=msg):
        minimax_q_config(761, **args)


def test_config_carries_the_defaults_and_the_fixed_policy():
    cfg, keep = minimax_q_config(761, 0.9)
    assert (cfg.discount_factor, cfg.alpha, cfg.explor, cfg.q_init, cfg.opponent) == (0.9, 1.0, 0.2, 1.0, _lib.MQ_UNIFORM)
    assert cfg.decay == 0.01 ** (1 / 1e6) and keep is None and not cfg.opponent_policy
    pol = np.full((761, 5), 0.2)
    cfg, keep = minimax_q_config(761, 0.5, opponent=pol)
    assert cfg.opponent == _lib.MQ_FIXED and cfg.opponent_policy == keep.ctypes.data
    assert minimax_q_config(761, 0.5, opponent="self")[0].opponent == _lib.MQ_SELF


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    cfg, _ = minimax_q_config(761, 0.9)
    q = C.c_void_p()
    assert lib.soccer_minimax_q_create(None, C.byref(cfg), C.byref(q)) == _lib.E_INVALID and not q.value
    assert lib.soccer_minimax_q_run(None, None, 1) == _lib.E_INVALID
    assert lib.soccer_minimax_q_update(None, None, 0, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_read(None, None, None, None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_load(None, None, None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_minimax_q_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
