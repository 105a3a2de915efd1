"""Mixed precision (hot_set_preconditioner_dtype): an fp64 context whose preconditioner runs on an fp32 hierarchy.

 3  the fp32 V-cycle is a correct fp32 V-cycle: the operators of the exported levels against the fp64 reference (tests/mg_reference.py) on level 0
    rounded to nearest by numpy, bounds K u with u = 2^-24 and the derived constants K_* as they stand
 4  exact scale invariance of hot_vcycle under powers of two, all-zero input
 5  one step converges to the fp64 answer: exit test re-evaluated in fp64, iteration count, particle velocities against the distance between two
    fp64 solves that differ only in the preconditioner (levelCnt 3 against 2)
 6  projected Newton: the operator stays the fp64 Hessian, bit for bit
 7  determinism   8  nothing moves when the switch is untouched   9  switching back and forth   10  rejections   11  the time-out path"""
import os

import numpy as np
import pytest

import hot_amd
from hot_amd import HotError, synth
from tests import det_scenes
from tests import mg_reference as mr
from tests import mixed_precision_checks as mx
from tests import test_gpu_mg_reference as tm

pytestmark = pytest.mark.gpu

MG32_LABELS = ("mg32_matrix", "mg32_enter", "mg32_exit")


# ---- 3. operators and V-cycle of the fp32 hierarchy against the fp64 reference
@pytest.mark.parametrize("name", ["cube8", "cube8_per_colour", "irregular", "cube44"])
def test_fp32_hierarchy_against_fp64_reference(hotlib, name):
    _, _, nlev, path, _, full = tm.SCENES[name]
    ctx = tm.build(mx.MixedLib(hotlib), name, 1)  # dtype 1, C2's material, coarseSolver 5, profile 1 — and preconditioner_dtype 0
    assert ctx.preconditioner_dtype == 0
    assert ctx.profile()["mg32_matrix"]["calls"] == 1  # hot_build_mg rounded level 0 once
    ref = mr.Hierarchy(mx.RoundedLevel0(ctx), nlev)
    counts = ref.levels[0].colour_blocks
    got = tm.level0_path(ctx, counts)
    sizes = [L.n for L in ref.levels]
    label = f"{name} mixed"
    print(f"\n[{label}] level-0 path {got}, level sizes {sizes}, level-0 blocks per colour {counts}")
    assert got == path, (name, got)
    T = np.float32  # the vectors of the checks are made fp32-representable first
    rep = mr.Report(label, mr.U32)
    mr.check_operators(ctx, ref, T, rep, nlev, gs_levels=None if full else (0,), jacobi_levels=(0, 1) if full else (), galerkin=full, pcg_its=(), pcg_levels=())
    x = np.asarray(ctx.project(np.random.default_rng(5).standard_normal((ctx.Nn, 3))), T).astype(np.float64)
    v, m, K = ref.vcycle(x)
    ctx.profile_reset()
    rep.add(f"vcycle{nlev}", 0, ctx.vcycle(x), v, m, K)
    prof = ctx.profile()
    assert prof["mg32_enter"]["calls"] == 2 and prof["mg32_exit"]["calls"] == 1 and "vcycle_start" not in prof, sorted(prof)
    rep.check()


# ---- 4. exact scale invariance
def test_vcycle_is_exactly_scale_invariant(hotlib):
    cfg = tm.MATERIAL[1]
    c = synth.cube_cloud(8, ppc=8, dtype=np.float64, E=cfg["E"], nu=cfg["nu"], rho=cfg["rho"])
    ctx = hotlib.context(dtype=1, dx=c["dx"], gravity=(0, -9.8, 0), levelCnt=3, preconditioner_dtype=0)  # default solvers: smoother 5, coarse solver 2
    assert ctx.cfg.smoother == 5 and ctx.cfg.coarseSolver == 2
    ctx.set_particles(c["X"], c["V"], c["mass"], c["vol"], c["mu"], c["lam"])
    o, nrm = synth.sticky_floor(5.0, c["dx"])
    ctx.set_sticky_halfspaces(o, nrm)
    ctx.sort(), ctx.p2g(), ctx.begin_step(1.0 / 24)
    ctx.update_state(ctx.get_dv())
    ctx.build_hessian(), ctx.build_mg()
    x = ctx.project(np.random.default_rng(11).standard_normal((ctx.Nn, 3)))
    y = ctx.vcycle(x)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    for k in (-300, -60, 60, 300):
        s = 2.0 ** k
        yk = ctx.vcycle(x * s)
        assert np.array_equal(yk, y * s), (k, float(np.abs(yk - y * s).max()))
    # what a plain cast would do at k = -300: every entry underflows to zero in fp32
    assert not np.any((x * 2.0 ** -300).astype(np.float32))
    z = ctx.vcycle(np.zeros((ctx.Nn, 3)))
    assert np.array_equal(z, np.zeros((ctx.Nn, 3))), "an all-zero input must give an all-zero output (no NaN from the exponent)"


# ---- 5. the solve converges to the fp64 answer
def _solve_body(lib, body, **kw):
    ctx, cfg = mx.make_body(lib, body, deterministic=1, lsolver=3, **kw)
    st, ex, scaled = mx.step_members(ctx, cfg["dt"])
    p = ctx.get_particles()
    del ctx
    return st, ex, scaled, p


@pytest.mark.parametrize("body", list(mx.BODIES))
def test_one_step_converges_to_the_fp64_answer(hotlib, body):
    gated = mx.BODIES[body][3]
    st64, ex64, _, p64 = _solve_body(hotlib, body, levelCnt=3)
    st64b, _, _, p64b = _solve_body(hotlib, body, levelCnt=2)  # the yardstick: the same solve behind another (existing) preconditioner
    stmx, exmx, scaled, pmx = _solve_body(hotlib, body, levelCnt=3, preconditioner_dtype=0)
    yard = mx.velocity_distance(p64b, p64)
    dist = mx.velocity_distance(pmx, p64)
    line = (f"[{body}] iterations fp64 {st64['iterations']} (levelCnt 2: {st64b['iterations']}) mixed {stmx['iterations']}; converged fp64 {st64['converged']} mixed {stmx['converged']}; "
            f"fp64 exit test on the mixed solution: exit={int(exmx)} scaled residual {scaled:.3e}; velocity distance mixed-fp64 {dist:.3e}, fp64(levelCnt 2)-fp64(levelCnt 3) {yard:.3e}; "
            f"vcycles fp64 {st64['vcycles']} mixed {stmx['vcycles']}; ms_mg_build fp64 {st64['ms_mg_build']:.1f} mixed {stmx['ms_mg_build']:.1f}")
    print("\n" + line)
    assert stmx["num_levels"] == 3 and stmx["vcycles"] > 0 and stmx["ms_mg_build"] > 0
    if not gated:
        return
    assert st64["converged"] == 1 and ex64
    assert stmx["converged"] == 1, line  # (a)
    assert exmx, line
    assert stmx["iterations"] <= 1.10 * st64["iterations"] + 1, line  # (b)
    assert dist <= 2.0 * yard, line  # (c)


# ---- 6. projected Newton: the operator is the fp64 Hessian
def test_projected_newton_keeps_the_fp64_operator(hotlib):
    kw = dict(n=12, ppc=8, levelCnt=2, lsolver=2, linear_iteration_cap=10, deterministic=1)
    out = {}
    for mode, extra in (("fp64", {}), ("mixed", dict(preconditioner_dtype=0))):
        ctx, cfg = det_scenes.make(hotlib, "C1", **kw, **extra)
        ctx.sort(), ctx.p2g(), ctx.begin_step(cfg["dt"])
        ctx.update_state(ctx.get_dv())
        ctx.build_hessian()
        col0, val0 = ctx.matrix(0)  # the assembled matrix, stencil-slot order
        x = np.random.default_rng(2).standard_normal((ctx.Nn, 3))
        y0 = ctx.spmv(0, x)
        ctx.build_mg()
        col1, val1 = ctx.matrix(0)
        y1 = ctx.spmv(0, x)
        st = ctx.solve()
        out[mode] = dict(col0=col0, val0=val0, y0=y0, col1=col1, val1=val1, y1=y1, st=st, nlev=st["num_levels"])
        del ctx
    a, b = out["fp64"], out["mixed"]
    print(f"\n[newton] iterations fp64 {a['st']['iterations']} mixed {b['st']['iterations']}, linear iterations fp64 {a['st']['linear_iterations']} mixed {b['st']['linear_iterations']}")
    assert a["st"]["converged"] == 1 and b["st"]["converged"] == 1
    assert b["nlev"] == 2
    # the assembly is bit-reproducible under deterministic = 1: both contexts hold the same fp64 matrix
    assert np.array_equal(a["col0"], b["col0"]) and np.array_equal(a["val0"], b["val0"])
    # hot_build_mg of a mixed context leaves the fp64 level 0 alone (an fp64 build regroups its rows): matrix and product keep their bits
    assert np.array_equal(b["col1"], b["col0"]) and np.array_equal(b["val1"], b["val0"])
    assert np.array_equal(b["y1"], b["y0"]) and np.array_equal(b["y0"], a["y0"])
    assert not np.array_equal(a["col1"], a["col0"])  # (the fp64 build did regroup: the comparison above is not vacuous)
    assert np.abs(a["y1"] - a["y0"]).max() <= 1e-12 * np.abs(a["y0"]).max()


# ---- 7. determinism
def test_two_mixed_contexts_give_the_same_bits(hotlib):
    a = det_scenes.run_scene(hotlib, "chained", profile_last=True, preconditioner_dtype=0)
    b = det_scenes.run_scene(hotlib, "chained", profile_last=True, preconditioner_dtype=0)
    assert a["converged"] == [1, 1], a
    for k in MG32_LABELS:
        assert k in a["labels"], a["labels"]
    assert a["particles"] == b["particles"] and a["stats"] == b["stats"], (a, b)


# ---- 8. nothing moves when the switch is untouched
def test_default_context_launches_what_the_parent_launched(hotlib):
    want = mx.parent_labels()
    untouched, st0 = mx.one_c1_step_profile(hotlib)
    set_to_1, st1 = mx.one_c1_step_profile(hotlib, lambda ctx: ctx.set_preconditioner_dtype(1))
    assert st0["converged"] == 1 and st0["iterations"] == want["iterations"], (st0["iterations"], want["iterations"])
    for got in (untouched, set_to_1):
        assert not [k for k in got if k.startswith("mg32")], sorted(got)
        diff = {k: (got.get(k), want["calls"].get(k)) for k in set(got) | set(want["calls"]) if got.get(k) != want["calls"].get(k)}
        assert not diff, diff


# ---- 9. switching
def test_switching_back_and_forth(hotlib):
    ctx, cfg = det_scenes.make(hotlib, "C1", levelCnt=3, deterministic=1, profile=1)
    used, labels = [], []
    for mode in (0, 1, 0):
        ctx.set_preconditioner_dtype(mode)
        assert ctx.preconditioner_dtype == mode
        ctx.profile_reset()
        st = ctx.advance(cfg["dt"])
        assert st["converged"] == 1 and st["num_levels"] == 3, (mode, st)
        labels.append(set(ctx.profile()))
        used.append(mx.device_mib_used())
    print(f"\n[switching] device MiB in use after the steps (mixed, fp64, mixed): {[round(u, 1) for u in used]}")
    for k in MG32_LABELS:
        assert k in labels[0] and k not in labels[1] and k in labels[2], (k, [sorted(l) for l in labels])
    assert "vcycle_start" in labels[1] and "vcycle_start" not in labels[0]
    # the fp64 step built its own hierarchy; the mixed step after it gives that back and finds its fp32 levels in the pool
    assert used[1] > used[0]
    assert used[2] <= used[0], used


# ---- 10. rejections
def test_rejections(hotlib):
    c32 = hotlib.context(dtype=0)
    c32.set_preconditioner_dtype(0)
    assert c32.preconditioner_dtype == 0
    with pytest.raises(HotError, match="fp64 hierarchy under an fp32 context"):
        c32.set_preconditioner_dtype(1)
    c64 = hotlib.context(dtype=1)
    assert c64.preconditioner_dtype == 1
    for bad in (2, -1):
        with pytest.raises(HotError, match="dtype must be 1"):
            c64.set_preconditioner_dtype(bad)
    assert c64.preconditioner_dtype == 1
    with pytest.raises(HotError, match="useBaselineMultigrid"):
        hotlib.context(dtype=1, useBaselineMultigrid=1, preconditioner_dtype=0)
    with pytest.raises(HotError, match="matrixFree"):
        hotlib.context(dtype=1, lsolver=2, matrixFree=1, levelCnt=1, systemBCProject=0, preconditioner_dtype=0)
    # a communicator of size > 1, either order (the callbacks are never reached: both calls fail before anything is exchanged)
    from hot_amd import dist
    comm = dist.hot_comm()
    comm.rank, comm.size = 0, 2
    comm.allreduce = dist._ALLREDUCE(lambda *a: 0)
    comm.allgather = dist._ALLGATHER(lambda *a: 0)
    comm.alltoallv = dist._ALLTOALLV(lambda *a: 0)

    class Holder:
        struct = comm

    c64.set_preconditioner_dtype(0)
    with pytest.raises(HotError, match="communicator of size > 1"):
        c64.set_comm(Holder)
    c64.set_preconditioner_dtype(1)
    c64.set_comm(Holder)
    with pytest.raises(HotError, match="communicator of size > 1"):
        c64.set_preconditioner_dtype(0)
    c64.set_comm(None)
    c64.set_preconditioner_dtype(0)
    # Ainv = 2 (no hierarchy): accepted, nothing to act on
    ctx, cfg = det_scenes.make(hotlib, "C1", n=8, ppc=8, lsolver=2, levelCnt=1, Ainv=2, preconditioner_dtype=0, profile=1)
    st = ctx.advance(cfg["dt"])
    assert st["converged"] == 1 and not [k for k in ctx.profile() if k.startswith("mg32")]


# ---- 11. the time-out path
# which time-out flag the A/B build's hook raises at the first synchronisation inside the operation (a word in pinned host memory, nothing happens on the device):
#   HOT_GS_FAKE_TIMEOUT         the fp64 context's own: it books the time-out and switches itself and the fp32 hierarchy's context to launches
#   HOT_GS_FAKE_TIMEOUT_SHADOW  the fp32 hierarchy's context's, as a chained sweep or persistent PCG of the fp32 V-cycle would: the fp64 context's sync() sees it,
#                               the fp32 context books it (path switch, count) and throws through the fp64 context's operation, which redoes itself
@pytest.mark.parametrize("hook", ["HOT_GS_FAKE_TIMEOUT", "HOT_GS_FAKE_TIMEOUT_SHADOW"])
def test_timed_out_vcycle_redoes_itself(hook):
    """The redone V-cycle against the launch-per-pass path (gs_chain = 1) of a context that never timed out: the 1e-12 bound of tests/test_gpu_variants.py in fp32 units,
    1e-12 u32 / u64 normwise; the two run the same launches on the same data, so they are also required to agree bit for bit."""
    lib = hot_amd.HotLib(hot_amd.AB_LIB_PATH)
    hooks = ("HOT_GS_FAKE_TIMEOUT", "HOT_GS_FAKE_TIMEOUT_SHADOW")
    for h in hooks:
        os.environ.pop(h, None)
    try:
        clean = tm.build(mx.MixedLib(lib), "cube8", 1)
        ref = mr.Hierarchy(mx.RoundedLevel0(clean), 3)
        x = np.asarray(clean.project(np.random.default_rng(5).standard_normal((clean.Nn, 3))), np.float32).astype(np.float64)
        v, m, K = ref.vcycle(x)
        clean.profile_reset()
        y_clean = clean.vcycle(x)
        assert clean.profile()["gs_forward_L0"]["calls"] == 2  # chained: one launch per half sweep, two sweeps of level 0 a V-cycle
        per_pass = tm.build(mx.MixedLib(lib, gs_chain=1), "cube8", 1)  # the launch-per-pass path by configuration
        y_pass = per_pass.vcycle(x)
        faked = tm.build(mx.MixedLib(lib), "cube8", 1)
        os.environ[hook] = "1"
        faked.profile_reset()
        y_faked = faked.vcycle(x)
        os.environ.pop(hook, None)
        prof = faked.profile()
        # the V-cycle ran twice: chained (2 launches on level 0), then one launch per non-empty colour and half sweep
        ncol = sum(b > 0 for b in ref.levels[0].colour_blocks)
        assert prof["gs_forward_L0"]["calls"] == 2 + 2 * ncol, (prof["gs_forward_L0"], ncol)
        assert prof["mg32_exit"]["calls"] == 2
        q_clean, q_faked = mr.ratio(y_clean, v, m, mr.U32), mr.ratio(y_faked, v, m, mr.U32)
        nw = mr.normwise(y_faked, y_pass)
        bound = 1e-12 * (mr.U32 / mr.U64)
        print(f"\n[timeout {hook}] |err|/(u32 m) against the fp64 reference: chained {q_clean:.4g}, redone {q_faked:.4g}; K = {K}; "
              f"redone against gs_chain=1: normwise {nw:.3e} (bound {bound:.3e}), bitwise equal: {np.array_equal(y_faked, y_pass)}")
        assert q_clean <= K and q_faked <= K  # both are correct fp32 V-cycles by the derived bound
        assert nw <= bound
        assert np.array_equal(y_faked, y_pass)
        y_again = faked.vcycle(x)  # the context stays on the launch-per-pass path and keeps its result
        assert np.array_equal(y_again, y_faked)
    finally:
        for h in hooks:
            os.environ.pop(h, None)
