"""hot_config.deterministic (ABI 7): the field takes the slot of reserved[0], so the structure keeps its size, and the ctypes mirrors agree
with the header.  The CPU checker compiles against the same header, sees the field in its old reserved slot and ignores it."""
import ctypes as C
import os
import subprocess

import numpy as np

from hot_amd import binding, synth
from tests import golden_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "hot_mi355x.h"
int main(void)
{
    printf("%zu %zu %zu %d\n", offsetof(hot_config, deterministic), offsetof(hot_config, reserved), sizeof(hot_config), HOT_ABI_VERSION);
    return 0;
}
"""


def test_header_layout_matches_the_mirrors(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    off_det, off_res, size, abi = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert off_det == binding.hot_config.deterministic.offset
    assert off_res == binding.hot_config.reserved.offset == off_det + 4
    assert size == C.sizeof(binding.hot_config)
    assert abi == binding.ABI_VERSION == 7
    # tests/golden_checks.py keeps its own copy of the structure with reserved[5]: the size did not change
    assert size == C.sizeof(golden_checks.Config)
    assert off_det == golden_checks.Config.reserved.offset


def test_default_config_leaves_the_flag_off(oracle):
    cfg = oracle.default_config()
    assert cfg.deterministic == 0
    assert oracle.default_config(deterministic=1).deterministic == 1


def test_checker_accepts_the_flag_and_converges(oracle):
    c = synth.cube_cloud(6, ppc=8)
    ctx = oracle.context(dtype=1, dx=c["dx"], levelCnt=2, gravity=(0, -9.8, 0), deterministic=1)
    ctx.set_particles(c["X"], c["V"], c["mass"], c["vol"], c["mu"], c["lam"])
    o, n = synth.sticky_floor(5.0, c["dx"])
    ctx.set_sticky_halfspaces(o, n)
    st = ctx.advance(1.0 / 24)
    assert st["converged"] == 1
    assert np.isfinite(ctx.get_particles()["X"]).all()
