"""Per-particle plasticity classes on the GPU (hot_set_plasticity_classes): elastic, von Mises and snow particles in one context.

The partner for floating-point results is the checker's element-wise projectStrain (tests.oracle_lib.plasticity: PlasticityApplier.cpp:18-50, 96-131),
applied per class to that class's particles on the trial F an elastic context (plasticity = 0, no table) computes — the method of
test_fullsize_plastic_return_mapping.  Tolerances are those of the existing tests of this path: F to 1e-9 (fp64) / 2e-5 (fp32) of max |F|, mu / lam / Jp
to ten times that (test_fullsize_plastic_return_mapping); X 1e-13 / 1e-6, V 1e-11 / 1e-4 against the elastic run (same test: the two runs differ by the rounding
of their atomic node sums, nothing else), C and the strain of class-0 particles like V."""
import struct

import numpy as np
import pytest

import hot_amd
from hot_amd import synth
from tests import det_scenes, golden_checks, pipeline_checks as pc
from tests.oracle_lib import plasticity

pytestmark = pytest.mark.gpu

CLASSES = [
    dict(kind=0),
    dict(kind=1, yield_stress=30.0),
    dict(kind=2, snow=(10, 2e-2, 7.5e-3, 0.6, 20)),
    dict(kind=1, yield_stress=300.0),
    dict(kind=2, snow=(0, 0.01, 0.001, -2, 5)),
]
N, NP = 8, 4096


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def assignment(kind, c):
    if kind == "random":  # divergent wavefronts
        return np.random.default_rng(11).integers(0, 5, NP).astype(np.int32)
    x = (c["X"][:, 0].astype(np.float64) - 5.0) / (N * c["dx"])  # five x-slabs: wavefronts of one class, and the skip paths
    return np.clip((x * 5).astype(np.int32), 0, 4)


def step(ctx, dt):
    ctx.sort(), ctx.p2g(), ctx.begin_step(dt)
    ctx.set_dv(np.zeros((ctx.Nn, 3), ctx.T))
    ctx.g2p(dt)


def project(state, cls, classes=CLASSES):
    """The checker's projectStrain, class by class, on copies of a particle state: F, mu, lam, Jp (float64) and the mask of particles whose F it changed."""
    F, mu, lam, Jp = (np.array(state[k], np.float64) for k in ("F", "mu", "lam", "Jp"))
    F0 = F.copy()
    for k, d in enumerate(classes):
        s = cls == k
        if d["kind"] == 0 or not s.any():
            continue
        F[s], mu[s], lam[s], Jp[s] = plasticity(d["kind"], F[s], mu[s], lam[s], Jp[s], d.get("yield_stress", 0.0), d.get("snow", (10, 2e-2, 7.5e-3, 0.6, 20)))
    return F, mu, lam, Jp, np.abs(F - F0).max(1) > 1e-7


def compare(got, trial, cls, f64, classes=CLASSES):
    """got: the class context's particles; trial: the elastic context's (same step).  Returns the share of every class the mapping changed."""
    tol = 1e-9 if f64 else 2e-5
    Fp, mu, lam, Jp, yielded = project(trial, cls, classes)
    figures = dict(F=rel(got["F"], Fp), mu=rel(got["mu"], mu), lam=rel(got["lam"], lam), Jp=rel(got["Jp"], Jp), X=rel(got["X"], trial["X"]), V=rel(got["V"], trial["V"]),
                   C=rel(got["C"], trial["C"]))
    elastic = np.isin(cls, [k for k, d in enumerate(classes) if d["kind"] == 0])
    if elastic.any():
        figures["F_elastic"] = np.abs(got["F"][elastic].astype(np.float64) - trial["F"][elastic]).max() / np.abs(trial["F"]).max()
    print("plasticity classes:", {k: "%.2e" % v for k, v in figures.items()}, "yielded:", {k: round(float(yielded[cls == k].mean()), 3) for k in range(len(classes)) if (cls == k).any()})
    assert figures["F"] < tol, figures
    assert figures["mu"] < 10 * tol and figures["lam"] < 10 * tol and figures["Jp"] < 10 * tol, figures
    assert figures["X"] < (1e-13 if f64 else 1e-6), figures
    assert figures["V"] < (1e-11 if f64 else 1e-4) and figures["C"] < (1e-11 if f64 else 1e-4), figures
    if elastic.any():
        assert figures["F_elastic"] < (1e-11 if f64 else 2e-5), figures
        for k in ("mu", "lam", "Jp"):
            assert np.array_equal(got[k][elastic], trial[k][elastic]), k  # never written
    not_snow = ~np.isin(cls, [k for k, d in enumerate(classes) if d["kind"] == 2])
    for k in ("mu", "lam", "Jp"):
        assert np.array_equal(got[k][not_snow], trial[k][not_snow]), k  # written by lanes of kind 2 only
    return {k: float(yielded[cls == k].mean()) for k in range(len(classes)) if (cls == k).any()}


@pytest.mark.parametrize("dt", [4e-3, 1.0 / 24], ids=["dt4e-3", "dt1_24"])
@pytest.mark.parametrize("assign", ["random", "slab"])
@pytest.mark.parametrize("dtype", [1, 0], ids=["fp64", "fp32"])
def test_mixed_classes_in_g2p(hotlib, dtype, assign, dt):
    """Test 1: five classes (none, two von Mises, two snow) in one G2P, random per particle and by x-slab, at a small and a large strain increment."""
    ctx, c = pc.make_ctx(hotlib, n=N, dtype=dtype, bc=False, E=5e4)
    assert ctx.Np == NP
    cls = assignment(assign, c)
    ctx.set_plasticity_classes(CLASSES, cls)
    step(ctx, dt)
    ela, _ = pc.make_ctx(hotlib, n=N, dtype=dtype, bc=False, E=5e4, plasticity=0)
    step(ela, dt)
    share = compare(ctx.get_particles(), ela.get_particles(), cls, dtype == 1)
    assert np.array_equal(ctx.plasticity_classes()[1], cls)
    # not vacuous (checked with the checker alone, random assignment, dt = 4e-3: the mapping changes F for 100 % of class 1, 32 % of class 2, 73 % of
    # class 3, 96 % of class 4; at dt = 1 / 24 all four classes yield completely)
    if dt > 1e-2:
        assert all(share[k] > 0.95 for k in (1, 2, 3, 4)), share
    elif assign == "random":
        assert all(share[k] >= 0.2 for k in (1, 2, 3, 4)), share
        assert share[2] <= 0.8 and share[3] <= 0.8, share  # both sides of the von Mises `return false` and of the clamp are compared


@pytest.mark.parametrize("dtype", [1, 0], ids=["fp64", "fp32"])
def test_classes_follow_their_particles(hotlib, dtype):
    """Test 2: a second step on the same context (another sort, with another order): the classes come back in the caller's order, and the step equals an
    elastic context started from the first step's state followed by the per-class projection with THAT state's mu, lam, Jp."""
    dt = 4e-3
    ctx, c = pc.make_ctx(hotlib, n=N, dtype=dtype, bc=False, E=5e4)
    cls = assignment("random", c)
    ctx.set_plasticity_classes(CLASSES, cls)
    step(ctx, dt)
    s1 = ctx.get_particles()
    step(ctx, dt)
    classes, back = ctx.plasticity_classes()
    assert np.array_equal(back, cls)
    assert [d["kind"] for d in classes] == [d["kind"] for d in CLASSES] and classes[3]["yield_stress"] == 300.0 and classes[4]["snow"] == (0, 0.01, 0.001, -2, 5)
    ela = hotlib.context(dtype=dtype, dx=c["dx"], gravity=(0, -9.8, 0), debug_store=1)
    ela.set_particles(s1["X"], s1["V"], c["mass"], c["vol"], s1["mu"], s1["lam"], C_=s1["C"], F=s1["F"], Jp=s1["Jp"])
    step(ela, dt)
    assert not np.array_equal(s1["Jp"], np.ones_like(s1["Jp"]))  # the second step starts from hardened snow
    compare(ctx.get_particles(), ela.get_particles(), cls, dtype == 1)


@pytest.mark.parametrize("kind", [1, 2], ids=["von_mises", "snow"])
def test_one_class_equals_the_global_setting(hotlib, kind):
    """Test 3: a one-class table against hot_config.plasticity with the values of test_plasticity_in_g2p; and which kernel ran (profile labels)."""
    dt = 1.0 / 24
    snow = (10, 2e-2, 7.5e-3, 0.6, 20)  # hot_default_config
    out, prof = {}, {}
    for name in ("table", "cfg"):
        kw = dict(plasticity=kind, yield_stress=30.0) if name == "cfg" else {}
        ctx, c = pc.make_ctx(hotlib, n=6, dtype=1, bc=False, E=5e4, profile=1, **kw)
        if name == "table":
            ctx.set_plasticity_classes([dict(kind=kind, yield_stress=30.0, snow=snow)], np.zeros(ctx.Np, np.int32))
        step(ctx, dt)
        out[name], prof[name] = ctx.get_particles(), ctx.profile()
    for k in ("F", "mu", "lam", "Jp"):
        print("one class against cfg.plasticity = %d: %s %.2e" % (kind, k, rel(out["table"][k], out["cfg"][k])))
    for k in ("F", "mu", "lam", "Jp"):
        assert rel(out["table"][k], out["cfg"][k]) < 1e-12, k
    assert rel(out["cfg"]["F"], np.tile(np.eye(3).reshape(1, 9), (len(out["cfg"]["F"]), 1))) > 1e-3
    assert prof["table"].get("g2p_classes", {}).get("calls") == 1 and "g2p" not in prof["table"]
    assert prof["cfg"].get("g2p", {}).get("calls") == 1 and "g2p_classes" not in prof["cfg"]
    # n = 0 removes the table: the kernel of hot_config.plasticity again
    ctx.set_plasticity_classes([dict(kind=1, yield_stress=1.0)], np.zeros(ctx.Np, np.int32))
    ctx.set_plasticity_classes([])
    ctx.profile_reset()
    step(ctx, dt)
    assert "g2p" in ctx.profile() and "g2p_classes" not in ctx.profile()
    assert ctx.plasticity_classes() == ([], None)


@pytest.mark.parametrize("dtype", [1, 0], ids=["fp64", "fp32"])
def test_numpy_goldens_through_the_class_path(hotlib, dtype):
    """Test 4: the von Mises and snow vectors of tests/golden/fp_golden.npz (golden_checks.check_plasticity) through hot_plasticity_eval_classes: a two-class
    table, the two sample sets interleaved with their classes, check_plasticity's tolerances."""
    g = np.load(golden_checks.GOLDEN)
    T = np.float64 if dtype == 1 else np.float32
    n = g["pl_F"].shape[0]
    tol = 1e-11 if dtype == 1 else 2e-5
    ctx, _ = pc.make_ctx(hotlib, n=4, dtype=dtype, bc=False)
    ctx.set_plasticity_classes([dict(kind=1, yield_stress=float(g["vm_yield"])), dict(kind=2, snow=tuple(float(v) for v in g["snow_params"]))], np.zeros(ctx.Np, np.int32))
    order = np.arange(2 * n).reshape(2, n).T.ravel()  # vm 0, snow 0, vm 1, snow 1, ...
    F0 = np.concatenate([g["pl_F"], g["pl_F"]])[order].astype(T)
    Jp0 = np.concatenate([np.ones(n), g["snow_Jp0"]])[order].astype(T)
    cls = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])[order]
    F, mu, lam, Jp = ctx.plasticity_eval_classes(F0, float(g["mu"]), float(g["lam"]), Jp0, cls)
    vm, sn = cls == 0, cls == 1
    relerr = golden_checks.relerr
    assert relerr(F[vm], g["vm_F"]) < tol, relerr(F[vm], g["vm_F"])
    stay = ~g["vm_hit"]
    assert np.array_equal(F[vm][stay], F0[vm][stay])  # inside the yield surface nothing moves
    assert np.array_equal(mu[vm], np.full(n, float(g["mu"]), T)) and np.array_equal(Jp[vm], np.ones(n, T))
    assert relerr(F[sn], g["snow_F"]) < tol and relerr(Jp[sn], g["snow_Jp"]) < tol * 10
    assert relerr(mu[sn], g["snow_mu"]) < tol * 50 and relerr(lam[sn], g["snow_lam"]) < tol * 50
    with pytest.raises(hot_amd.HotError):
        ctx.plasticity_eval_classes(F0, float(g["mu"]), float(g["lam"]), Jp0, cls + 1)  # class 2 of a two-class table


def _restart_arrays(path):
    with open(path, "rb") as f:
        count, narr = struct.unpack("<iQ", f.read(12))
    return count, narr


def test_validation_and_restart(hotlib, tmp_path):
    """Test 5: the rejected inputs leave the context as it was; the class column round-trips through a restart file and the restarted context continues
    bit for bit (deterministic = 1) once its parameter table is installed again."""
    dt = 4e-3
    ctx, c = pc.make_ctx(hotlib, n=N, dtype=1, bc=False, E=5e4, deterministic=1)
    cls = assignment("random", c)
    with pytest.raises(hot_amd.HotError):
        ctx.set_plasticity_classes(CLASSES, None)  # no classes held yet
    ctx.write_restart(tmp_path / "plain.dat")
    assert _restart_arrays(tmp_path / "plain.dat") == (NP, 9)
    ctx.set_plasticity_classes(CLASSES, cls)
    bad = [
        ([dict(kind=3)], np.zeros(NP, np.int32)),  # kind outside 0, 1, 2
        ([dict(kind=-1)], np.zeros(NP, np.int32)),
        ([dict(kind=0)] * 17, np.zeros(NP, np.int32)),  # n > 16
        (CLASSES, np.where(np.arange(NP) == 77, 5, cls).astype(np.int32)),  # a particle class == n
        (CLASSES, np.where(np.arange(NP) == NP - 1, -1, cls).astype(np.int32)),  # a negative one
        (CLASSES[:2], None),  # the context holds classes >= 2
    ]
    for classes, pcl in bad:
        with pytest.raises(hot_amd.HotError) as e:
            ctx.set_plasticity_classes(classes, pcl)
        assert "hot_set_plasticity_classes" in str(e.value), str(e.value)
        held, back = ctx.plasticity_classes()
        assert len(held) == 5 and np.array_equal(back, cls)  # a rejected call changes nothing
    step(ctx, dt)
    ctx.write_restart(tmp_path / "classes.dat")
    assert _restart_arrays(tmp_path / "classes.dat") == (NP, 10)
    re = hotlib.context(dtype=1, dx=c["dx"], gravity=(0, -9.8, 0), debug_store=1, deterministic=1)
    re.read_restart(tmp_path / "classes.dat")
    assert re.plasticity_classes()[0] == []  # the parameter table is not particle data
    re.set_plasticity_classes(CLASSES, None)
    assert np.array_equal(re.plasticity_classes()[1], cls)
    step(ctx, dt), step(re, dt)
    a, b = ctx.get_particles(), re.get_particles()
    for k in ("F", "mu", "lam", "Jp", "X", "V", "C"):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["Jp"], np.ones_like(a["Jp"]))
    re.read_restart(tmp_path / "plain.dat")  # a file without the column clears the table
    assert re.plasticity_classes() == ([], None)
    ctx.set_particles(c["X"], c["V"], c["mass"], c["vol"], c["mu"], c["lam"])  # and so does a new particle set
    assert ctx.plasticity_classes() == ([], None)


def two_body(lib, classes=True, **kw):
    c = synth.two_body_cloud(8)
    ctx = lib.context(dtype=1, dx=c["dx"], gravity=(0, -9.8, 0), **kw)
    ctx.set_particles(c["X"], c["V"], c["mass"], c["vol"], c["mu"], c["lam"])
    if classes:
        ctx.set_plasticity_classes(c["classes"], c["cls"])
    o, nrm = synth.sticky_floor(5.0, c["dx"])
    ctx.set_sticky_halfspaces(o, nrm)
    return ctx, c


def test_deterministic_mode(hotlib):
    """Test 6: deterministic = 1, the two-body scene, two contexts, two whole steps each: identical bytes and counters."""
    res = []
    for _ in range(2):
        ctx, _c = two_body(hotlib, deterministic=1)
        sts = [ctx.advance(1.0 / 24) for _ in range(2)]
        p = ctx.get_particles()
        res.append((det_scenes.digest_arrays([p[k] for k in ("F", "mu", "lam", "Jp", "X")]), [det_scenes.digest_stats(s) for s in sts], p))
        del ctx
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert not np.array_equal(res[0][2]["Jp"], np.ones_like(res[0][2]["Jp"]))


def test_two_body_scene(hotlib):
    """Test 7: the snow block with the stiff elastic ball dropped on it, sticky floor, three whole steps in fp64.  The ball is never touched by a return mapping:
    its mu, lam, Jp keep their bits.  Its strain stays elastic: the largest |sigma - 1| of its F is bounded by twice the purely elastic run's (the contact
    stress, which is all that strains a ball 700 times stiffer than what it lands on, scales with the snow's stiffness, and compaction hardening raises that
    by exp(psi (1 - Jp)) < 2 for the Jp >= 0.93 three steps can reach at theta_c = 2.5e-2)."""
    dt = 1.0 / 24
    dev, state = {}, {}
    for name in ("classes", "elastic"):
        ctx, c = two_body(hotlib, classes=name == "classes")
        for s in range(3):
            st = ctx.advance(dt)
            assert st["converged"] == 1, (name, s, st)
        p = ctx.get_particles()
        ball = c["cls"] == 1
        sv = np.linalg.svd(p["F"][ball].reshape(-1, 3, 3), compute_uv=False)
        dev[name], state[name] = np.abs(sv - 1).max(), p
    p, ball = state["classes"], c["cls"] == 1
    moved = np.abs(p["Jp"][~ball] - 1) > 1e-6
    print("two-body scene: ball max |sigma - 1| %.3e with classes, %.3e elastic; snow particles with Jp != 1: %.1f %%, Jp in [%.4f, %.4f]"
          % (dev["classes"], dev["elastic"], 100 * moved.mean(), p["Jp"].min(), p["Jp"].max()))
    for k in ("mu", "lam"):
        assert np.array_equal(p[k][ball], c[k][ball]), k
    assert np.array_equal(p["Jp"][ball], np.ones(ball.sum()))
    assert np.isfinite(p["F"]).all() and np.isfinite(p["X"]).all()
    assert dev["classes"] <= 2 * dev["elastic"], dev
    assert moved.mean() > 0, moved.mean()
    hard = p["mu"][~ball] / c["mu"][~ball]
    assert np.allclose(hard, p["lam"][~ball] / c["lam"][~ball], rtol=1e-12) and np.abs(hard[moved] - 1).max() > 0  # snow hardening: mu and lambda by one factor
    assert np.array_equal(state["elastic"]["Jp"], np.ones(len(ball)))


def test_classes_over_two_ranks(hotlib):
    """Test 8: two ranks from a deliberately poor partition (even / odd global ids: the first hot_sort migrates about half of the particles); after one solve
    and G2P the classes by global id equal the input and the particle state equals the single-rank run to the tolerance of test_one_body_over_ranks_hip."""
    from tests import multirank_worker as mw, plasticity_classes_worker as pw
    kw = dict(lsolver=3, levelCnt=3, max_iterations=5, cneps=1e-7)
    ranks = pw.launch(2, 8, 1, kw)
    ref = pw.single(hotlib, 8, 1, kw)
    cls = pw.classes_of(len(ref["particles"]["X"]))
    assert np.array_equal(ref["cls"], cls)
    ids = np.concatenate([o["ids"] for o in ranks])
    got = np.concatenate([o["cls"] for o in ranks])
    assert np.array_equal(np.sort(ids), np.arange(len(cls)))
    assert np.array_equal(got, cls[ids])  # every class arrived with its particle
    moved = sum(int((o["ids"] % 2 != r).sum()) for r, o in enumerate(ranks))
    print("two ranks: %d of %d particles changed rank at the first hot_sort" % (moved, len(cls)))
    assert 0.3 * len(cls) < moved < 0.7 * len(cls), moved
    mw.compare(ranks, ref, 1e-11)
    for k in ("mu", "lam", "Jp"):
        g = np.concatenate([o["particles"][k] for o in ranks])
        assert mw.rel(g, ref["particles"][k][ids]) < 1e-11 * 100, (k, mw.rel(g, ref["particles"][k][ids]))
    assert not np.array_equal(ref["particles"]["Jp"], np.ones(len(cls)))
