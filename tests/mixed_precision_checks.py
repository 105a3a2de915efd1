"""Helpers of the mixed-precision tests (tests/test_gpu_mixed_precision.py, tools/mg_precision_cost.py): an fp64 context whose
preconditioner runs on an fp32 hierarchy (hot_set_preconditioner_dtype)."""
import ctypes as C
import json
import os

import numpy as np

from tests import det_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_LABELS = os.path.join(ROOT, "tests", "golden", "mg_precision_parent_labels.json")

# bodies of the convergence tests: name -> (configuration whose material is used, cells per edge, particles per cell or None, gated)
BODIES = {
    "C1_body": ("C1", None, None, True),  # 22^3 cells x 20 particles, E = 5e4
    "C3_material_24": ("C3", 24, None, True),  # E = 1e9
    "C4_material_24": ("C4", 24, None, False),  # E = 69e9, von Mises: recorded, not gated
}


class MixedLib:
    """a library whose contexts are created with preconditioner_dtype = 0 (for builders written for plain contexts)"""

    def __init__(self, lib, **extra):
        self._lib, self._extra = lib, extra

    def context(self, **kw):
        kw.setdefault("preconditioner_dtype", 0)
        for k, v in self._extra.items():
            kw.setdefault(k, v)
        return self._lib.context(**kw)

    def __getattr__(self, name):
        return getattr(self._lib, name)


class RoundedLevel0:
    """a context whose exported level-0 matrix is rounded to nearest fp32, entry by entry, by numpy: what level 0 of the fp32 hierarchy must be"""

    def __init__(self, ctx):
        self._ctx = ctx

    def matrix(self, level):
        col, val = self._ctx.matrix(level)
        if level == 0:
            val = val.astype(np.float32).astype(np.float64)
        return col, val

    def __getattr__(self, name):
        return getattr(self._ctx, name)


def make_body(lib, body, **kw):
    cname, n, ppc, _ = BODIES[body]
    kw.setdefault("dtype", 1)
    return det_scenes.make(lib, cname, n, ppc, **kw)


def step_members(ctx, dt):
    """hot_advance member by member (sort, p2g, begin_step, solve, g2p) with an independent fp64 evaluation of the exit test (hot_residual, hot_should_exit) at the
    solution between solve and g2p; returns (stats of the solve, exit flag of should_exit on that residual, its scaled residual).
    What "independent" covers: hot_residual and hot_should_exit are fp64 calls that read no hierarchy, issued from outside the solver.  The state they
    evaluate is the one hot_solve left, that of its last line-search point.  A fresh hot_update_state(dv) before hot_residual would be a stricter check,
    and it does not pass in EITHER mode (n = 12 C1 body: scaled residual 2.3 with the fp64 hierarchy too), so it says nothing about mixed precision
    and is not what this helper does."""
    ctx.sort(), ctx.p2g(), ctx.begin_step(dt)
    st = ctx.solve()
    ex, scaled = ctx.should_exit(ctx.residual())  # hot_residual: fp64, from the force tiles of the solution's state pass; hot_should_exit: the fp64 exit test
    ctx.g2p(dt)
    return st, ex, scaled


def velocity_distance(pa, pb):
    """max-norm distance of the particle velocities relative to the largest speed"""
    va, vb = np.asarray(pa["V"], np.float64), np.asarray(pb["V"], np.float64)
    return float(np.abs(va - vb).max() / np.linalg.norm(vb, axis=1).max())


_hip = None


def device_mib_used():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    f, t = C.c_size_t(), C.c_size_t()
    rc = _hip.hipMemGetInfo(C.byref(f), C.byref(t))
    assert rc == 0, rc
    return (t.value - f.value) / 2.0 ** 20


def one_c1_step_profile(lib, setter=None):
    """{label: calls} of one deterministic step of the C1 body on a fresh profiled context; setter(ctx) runs before the step"""
    ctx, cfg = det_scenes.make(lib, "C1", deterministic=1, profile=1)
    if setter is not None:
        setter(ctx)
    st = ctx.advance(cfg["dt"])
    prof = {k: int(v["calls"]) for k, v in ctx.profile().items()}
    del ctx
    return prof, st


def parent_labels():
    with open(PARENT_LABELS) as f:
        return json.load(f)
