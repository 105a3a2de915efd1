"""Deterministic mode (hot_config.deterministic = 1): bitwise-reproducible time steps.

The five scatters that otherwise sum with floating-point LDS atomics run fixed-order kernels under the flag; these tests check that the
flag is validated, that it selects those kernels (by their launch labels), that every pass and every whole step repeats its bits — between
contexts of one process and between processes —, that the fixed-order sums agree with the atomic ones to round-off, that the C1 step
still matches the CPU checker, and that a simulated spin time-out is redone with the same launch structure."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hot_amd import HotError
from tests import det_scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LABELS = ("p2g", "force_scatter", "hessian_assemble")
DET_LABELS = ("p2g_det", "force_scatter_det", "hessian_assemble_det")
MF_LABELS = ("matfree_hessian_product", "matfree_diag_scatter")
MF_DET_LABELS = ("matfree_hessian_product_det", "matfree_diag_scatter_det")


def child(name, env=None, **over):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-m", "tests.det_scenes", name] + [f"{k}={v}" for k, v in over.items()], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---- 1. validation
@pytest.mark.parametrize("value", [2, -1])
def test_invalid_flag_is_rejected(hotlib, value):
    with pytest.raises(HotError, match="rc=-1"):
        hotlib.context(deterministic=value)


# ---- 2. selection
def _one_step_labels(hotlib, det, **kw):
    ctx, cfg = det_scenes.make(hotlib, "C1", n=12, ppc=8, deterministic=det, profile=1, **kw)
    st = ctx.advance(cfg["dt"])
    assert st["converged"] == 1
    return set(ctx.profile())


@pytest.mark.parametrize("det", [1, 0])
def test_flag_selects_the_kernels(hotlib, det):
    labels = _one_step_labels(hotlib, det)
    on, off = (DET_LABELS, DEFAULT_LABELS) if det else (DEFAULT_LABELS, DET_LABELS)
    for k in on:
        assert k in labels, (k, sorted(labels))
    for k in off:
        assert k not in labels, (k, sorted(labels))


@pytest.mark.parametrize("det", [1, 0])
def test_flag_selects_the_matrix_free_kernels(hotlib, det):
    labels = _one_step_labels(hotlib, det, lsolver=2, matrixFree=1, levelCnt=1)
    on, off = (MF_DET_LABELS, MF_LABELS) if det else (MF_LABELS, MF_DET_LABELS)
    for k in on:
        assert k in labels, (k, sorted(labels))
    for k in off:
        assert k not in labels, (k, sorted(labels))


# ---- 3. / 4. per pass, on the C1 body (the densest per-cell load of the configurations)
def _passes(hotlib, dtype, det):
    ctx, cfg = det_scenes.make(hotlib, "C1", dtype=dtype, deterministic=det)
    ctx.sort()
    ctx.p2g()
    out = {}
    g = ctx.grid()
    out["grid_mass"], out["grid_v"] = g["mass"], g["v"]
    ctx.begin_step(cfg["dt"])
    out["cn_tolerance"] = ctx.cn_tolerance()
    nn = ctx.Nn
    rng = np.random.default_rng(7)
    dv = (rng.standard_normal((nn, 3)) * 1e-3).astype(ctx.T)
    ctx.update_state(dv)
    out["residual"] = ctx.residual()
    ctx.build_hessian()
    out["matrix"] = ctx.matrix(0)[1]
    x = rng.standard_normal((nn, 3)).astype(ctx.T)
    out["matfree"] = ctx.matfree_multiply(x)
    del ctx
    return out


@pytest.mark.parametrize("dtype", [1, 0])
def test_passes_repeat_their_bits_and_match_the_atomic_kernels(hotlib, dtype):
    runs = [_passes(hotlib, dtype, 1) for _ in range(5)]
    for k in runs[0]:
        for r in runs[1:]:
            assert runs[0][k].tobytes() == r[k].tobytes(), (k, "differs between repetitions")
    ref = _passes(hotlib, dtype, 0)
    tol = 1e-12 if dtype == 1 else 1e-5
    for k, a in runs[0].items():
        b = ref[k]
        assert a.shape == b.shape, k
        scale = max(np.abs(b.astype(np.float64)).max(), 1e-300)
        err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / scale
        print(f"dtype {dtype} {k}: max |det - atomic| / max |atomic| = {err:.3g}")
        assert err <= tol, (k, err)


# ---- 5. whole steps, two contexts in this process and one child process
@pytest.mark.parametrize("name", ["C1", "C3_fp32", "C4_von_mises", "C5_snow", "matrix_free", "minres", "baseline_mg", "frame"])
def test_whole_steps_are_bitwise_reproducible(hotlib, name):
    a = det_scenes.run_scene(hotlib, name)
    b = det_scenes.run_scene(hotlib, name)
    c = child(name)
    print(name, a["iterations"], a["particles"][:16])
    assert a["particles"] == b["particles"] == c["particles"], (a, b, c)
    assert a["stats"] == b["stats"] == c["stats"], (a, b, c)


# ---- 6. still correct: the C1 step against the CPU checker, the tolerances of test_gpu_fullsize.py::test_c1_full_step_against_oracle
def test_c1_deterministic_step_against_oracle(hotlib, oracle):
    out = {}
    for name, lib, over in (("gpu", hotlib, dict(deterministic=1)), ("cpu", oracle, {})):
        ctx, cfg = det_scenes.make(lib, "C1", cneps=1e-7, **over)
        st = ctx.advance(cfg["dt"])
        out[name] = (ctx.get_particles(), st)
        del ctx
    sg, sc = out["gpu"][1], out["cpu"][1]
    assert sg["converged"] == 1 and sc["converged"] == 1
    assert sg["num_nodes"] == sc["num_nodes"]
    assert abs(sg["iterations"] - sc["iterations"]) <= max(2, sc["iterations"] // 10), (sg, sc)
    if sg["iterations"] == sc["iterations"]:
        assert sg["linesearch_trials"] == sc["linesearch_trials"], (sg, sc)
    else:
        assert abs((sg["linesearch_trials"] - sg["iterations"]) - (sc["linesearch_trials"] - sc["iterations"])) <= max(2, (sc["linesearch_trials"] - sc["iterations"]) // 10), (sg, sc)
    pg, pcpu = out["gpu"][0], out["cpu"][0]
    assert np.abs(pg["X"] - pcpu["X"]).max() < 1e-3 * 0.01
    ev = np.abs(pg["V"] - pcpu["V"]).max() / max(np.abs(pcpu["V"]).max(), 1e-3)
    assert ev < 1e-3, ev
    assert abs(sg["energy"] - sc["energy"]) < 1e-5 * max(abs(sc["energy"]), 1e-6)


# ---- 7. a simulated time-out of a chained structure is redone with the same structure
def test_timeout_recovery_keeps_the_bits():
    ab = {"HOT_AMD_AB": "1"}
    clean = child("chained", env=ab, profile_last=1)
    faked = child("chained", env=dict(ab, HOT_GS_FAKE_TIMEOUT="2"), profile_last=1)
    chained = [k for k in clean["labels"] if k.startswith("cg_persistent")]
    assert chained, clean["labels"]  # the scene does use the persistent PCG
    assert faked["particles"] == clean["particles"] and faked["stats"] == clean["stats"], (clean, faked)
    for k in chained:  # the second step, after the time-out of the first, still runs the persistent PCG
        assert k in faked["labels"], (k, faked["labels"])
    # control: without the flag the same time-out switches the context to one launch per pass for good
    legacy = child("chained", env=dict(ab, HOT_GS_FAKE_TIMEOUT="2"), profile_last=1, deterministic=0)
    assert not [k for k in legacy["labels"] if k.startswith("cg_persistent")], legacy["labels"]
