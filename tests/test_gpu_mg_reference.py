"""The device's multigrid level operators against the fp64 reference (tests/mg_reference.py) on the device's own exported levels,
componentwise: |gpu - ref| <= K u m with u = 2^-53 (fp64, C2's material) or 2^-24 (fp32, C3's material), whatever the conditioning.

The scenes are chosen by the path `Ctx::gs_plan` (hot_amd/csrc/mg_gs.hip) takes on level 0, and every case asserts that path from
the launch profile, so that a change of the plan's thresholds cannot silently remove the coverage:
  CHAINED     the n = 8 cube (one k_gs_sweep launch per half sweep), also with one particle per cell and on an irregular body
  PER_COLOUR  the n = 8 cube with gs_chain = 1 (one k_gs_block launch per non-empty colour)
  COLOUR      the smallest cube whose colours hold more than 256 blocks (n = 44: 13 blocks an edge), and a slab one block thick in y,
              whose colours 2, 3, 6 and 7 are empty (the forward sweep's turn is colour 5), at full size and at 8 x 2 x 8 cells with
              gs_chain = 1, gs_sub_block = 32
  PAIR        the n = 44 cube through the A/B build with HOT_GS_PAIR = 1 (k_gs_offblock + k_gs_subst)"""
import os
import time

import numpy as np
import pytest

from hot_amd import synth
from tests import mg_reference as mr

pytestmark = pytest.mark.gpu

MATERIAL = {1: synth.CONFIGS["C2"], 0: synth.CONFIGS["C3"]}
SLAB = dict(cells=(132, 2, 132), corner=(5.0, 4.965, 5.0))  # y nodes 496 - 499 only: the blocks of y index 124, even parity


def _irregular(T, cfg):
    """the multi-rank tests' body: a hollow ball with a bar through it (partial blocks, short rows, boundary-projected rows)"""
    c = synth.cube_cloud(14, ppc=8, dtype=np.float64, E=cfg["E"], nu=cfg["nu"], rho=cfg["rho"])
    X = c["X"]
    ctr = X.mean(0)
    r = np.linalg.norm(X - ctr, axis=1)
    keep = ((r < 0.066) & (r > 0.03)) | ((np.abs(X[:, 0] - ctr[0]) < 0.012) & (np.abs(X[:, 1] - ctr[1]) < 0.012))
    out = {k: (v[keep].astype(T) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return out, ctr[1] - 0.07


# name -> (cloud arguments, context arguments, levelCnt, path, A/B build with HOT_GS_PAIR, full operator set)
SCENES = {
    "cube8": (dict(n=8), {}, 3, "CHAINED", False, True),
    "cube8_per_colour": (dict(n=8), dict(gs_chain=1), 4, "PER_COLOUR", False, True),
    "cube8_ppc1": (dict(n=8, ppc=1), {}, 3, "CHAINED", False, True),
    "irregular": ("irregular", {}, 3, "CHAINED", False, True),
    "slab_small": (dict(n=0, cells=(8, 2, 8), corner=SLAB["corner"], floor=False), dict(gs_chain=1, gs_sub_block=32), 3, "COLOUR", False, True),
    "cube44": (dict(n=44), {}, 4, "COLOUR", False, True),
    "slab": (dict(n=0, floor=False, **SLAB), {}, 3, "COLOUR", False, True),
    "cube44_pair": (dict(n=44), {}, 3, "PAIR", True, False),
}


def build(lib, name, dtype, pair=False):
    cloud_kw, ctx_kw, levelCnt, _, _, _ = SCENES[name]
    cfg = MATERIAL[dtype]
    T = np.float64 if dtype == 1 else np.float32
    if cloud_kw == "irregular":
        c, floor_y = _irregular(T, cfg)
    else:
        kw = dict(cloud_kw)
        floor = kw.pop("floor", True)
        n = kw.pop("n")
        c = synth.cube_cloud(n, ppc=kw.pop("ppc", 8), dtype=T, E=cfg["E"], nu=cfg["nu"], rho=cfg["rho"], **kw)
        floor_y = kw.get("corner", (5.0, 5.0, 5.0))[1] if floor else None
    ctx = lib.context(dtype=dtype, dx=c["dx"], gravity=(0, -9.8, 0), levelCnt=levelCnt, coarseSolver=5, profile=1, **ctx_kw)
    ctx.set_particles(c["X"], c["V"], c["mass"], c["vol"], c["mu"], c["lam"])
    if floor_y is not None:
        o, nrm = synth.sticky_floor(floor_y, c["dx"])
        ctx.set_sticky_halfspaces(o, nrm)
    ctx.sort(), ctx.p2g(), ctx.begin_step(1.0 / 24)
    ctx.update_state(ctx.get_dv())
    ctx.build_hessian()
    os.environ.pop("HOT_GS_PAIR", None)
    if pair:
        os.environ["HOT_GS_PAIR"] = "1"  # read when the hierarchy is built: the kernel pair's slot lists instead of k_gs_colour's four
    try:
        ctx.build_mg()
    finally:
        os.environ.pop("HOT_GS_PAIR", None)
    return ctx


def level0_path(ctx, counts):
    """the GS path of level 0, from the launches of one symmetric sweep"""
    n = ctx.level(0, coords=False)["nrows"]
    ctx.profile_reset()
    ctx.smooth(0, 5, 2, np.zeros((n, 3)), np.ones((n, 3)))
    prof = ctx.profile()
    calls = lambda k: prof.get(k, {}).get("calls", 0)
    if calls("gs_forward_fused_L0"):
        return "COLOUR"
    if calls("gs_forward_off_L0"):
        return "PAIR"
    if calls("gs_forward_L0") == 1:
        return "CHAINED"
    if calls("gs_forward_L0") == sum(b > 0 for b in counts):
        return "PER_COLOUR"
    return "unknown: " + str({k: v["calls"] for k, v in prof.items() if k.startswith("gs_")})


@pytest.mark.parametrize("dtype", [1, 0], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(SCENES))
def test_mg_operators_against_fp64_reference(hotlib, name, dtype):
    import hot_amd
    _, _, nlev, path, pair, full = SCENES[name]
    t0 = time.time()
    lib = hot_amd.HotLib(hot_amd.AB_LIB_PATH) if pair else hotlib
    ctx = build(lib, name, dtype, pair)
    T = np.float64 if dtype == 1 else np.float32
    ref = mr.Hierarchy(ctx, nlev)
    counts = ref.levels[0].colour_blocks
    # the scene is the one it claims to be
    if name.startswith("slab"):
        assert [counts[c] for c in (2, 3, 6, 7)] == [0, 0, 0, 0] and all(counts[c] > 0 for c in (0, 1, 4, 5)), counts
    if name == "slab" or name.startswith("cube44"):
        assert max(counts) > 256, counts  # COLOUR by level size, not forced
    if name.startswith("cube8"):
        assert all(b > 0 for b in counts) and max(counts) <= 256, counts
    got = level0_path(ctx, counts)
    sizes = [L.n for L in ref.levels]
    label = f"{name} {'fp64' if dtype == 1 else 'fp32'}"
    print(f"\n[{label}] level-0 path {got}, level sizes {sizes}, level-0 blocks per colour {counts}")
    assert got == path, (name, got)
    rep = mr.Report(label, mr.U64 if dtype == 1 else mr.U32)
    top = nlev - 1
    mr.check_operators(ctx, ref, T, rep, nlev, gs_levels=None if full else (0,), jacobi_levels=(0, 1) if full else (), galerkin=full,
                       pcg_its=(1, 3, 10) if (full and dtype == 1) else (), pcg_levels=(0, top) if (full and dtype == 1) else ())
    x = np.asarray(ctx.project(np.random.default_rng(5).standard_normal((ctx.Nn, 3))), T)
    v, m, K = ref.vcycle(x)
    rep.add(f"vcycle{nlev}", 0, ctx.vcycle(x), v, m, K)
    print(f"[{label}] {time.time() - t0:.1f} s")
    rep.check()
