"""Scenes of the deterministic-mode tests (hot_config.deterministic = 1) and the digests they compare.

`run_scene(name)` builds one scene from hot_amd.synth / hot_amd.parallel, advances it and returns the sha256 of the particle state and of
the stats without their ms_* timings.  `python -m tests.det_scenes NAME [KEY=VALUE ...]` does the same in a fresh process and prints the
result as one JSON line (tests/test_gpu_deterministic.py runs it as a child process: no exec).  KEY=VALUE pairs override hot_config fields."""
import hashlib
import json
import sys

import numpy as np

from hot_amd import parallel, synth

PARTICLE_KEYS = ("X", "V", "C", "F", "Jp", "mu", "lam")


def make(lib, cname, n=None, ppc=None, **kw):
    cfg = dict(synth.CONFIGS[cname])
    if ppc is not None:
        cfg["ppc"] = ppc
    cloud = parallel.shard_cloud(cfg, 0, 1, n=n if n is not None else cfg["n"])
    args = dict(dtype=1 if cfg["dtype"] == np.float64 else 0, dx=cloud["dx"], gravity=(0, -9.8, 0), levelCnt=cfg["levelCnt"])
    args.update(synth.plasticity_kwargs(cfg))
    args.update(kw)
    ctx = lib.context(**args)
    ctx.set_particles(cloud["X"], cloud["V"], cloud["mass"], cloud["vol"], cloud["mu"], cloud["lam"])
    o, nrm = synth.sticky_floor(cloud["corner"][1], cloud["dx"])
    ctx.set_sticky_halfspaces(o, nrm)
    return ctx, cfg


def digest_arrays(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digest_stats(st):
    return hashlib.sha256(json.dumps({k: v for k, v in sorted(st.items()) if not k.startswith("ms_")}, sort_keys=True).encode()).hexdigest()


# name -> (configuration, cells per edge, particles per cell or None, hot_config overrides, steps; "frame" = one advance_frame)
SCENES = {
    "C1": ("C1", None, None, {}, 2),  # the full C1 body (22^3 cells x 20 particles), fp64
    "C3_fp32": ("C3", 30, None, {}, 1),
    "C4_von_mises": ("C4", 30, None, {}, 1),
    "C5_snow": ("C5", 30, None, {}, 1),
    "matrix_free": ("C2", 30, None, dict(lsolver=2, matrixFree=1, levelCnt=1), 1),
    "minres": ("C2", 30, None, dict(lsolver=1, levelCnt=1, max_iterations=4, linear_iteration_cap=200), 1),
    "baseline_mg": ("C2", 30, None, dict(useBaselineMultigrid=1), 1),
    "frame": ("C1", 12, 8, {}, "frame"),
    "chained": ("C2", 30, None, {}, 2),  # coarse levels small enough for the chained sweep and the persistent PCG
}


def run_scene(lib, name, deterministic=1, profile_last=False, **over):
    cname, n, ppc, kw, steps = SCENES[name]
    kw = dict(kw, deterministic=deterministic, **over)
    if profile_last:
        kw["profile"] = 1
    ctx, cfg = make(lib, cname, n, ppc, **kw)
    stats = []
    labels = []
    if steps == "frame":
        sub, its, st = ctx.advance_frame(1.0 / 24)
        stats.append(dict(st, substeps=sub, iterations_total=its))
    else:
        for s in range(steps):
            if profile_last and s == steps - 1:
                ctx.profile_reset()
            stats.append(ctx.advance(cfg["dt"]))
        if profile_last:
            labels = sorted(ctx.profile())
    p = ctx.get_particles()
    out = dict(particles=digest_arrays([p[k] for k in PARTICLE_KEYS]), stats=[digest_stats(st) for st in stats],
               converged=[int(st["converged"]) for st in stats], iterations=[int(st["iterations"]) for st in stats], labels=labels)
    del ctx
    return out


def main(argv):
    import hot_amd
    name = argv[0]
    over = {}
    for a in argv[1:]:
        k, v = a.split("=", 1)
        over[k] = int(v)
    print(json.dumps(run_scene(hot_amd.load(), name, **over)))


if __name__ == "__main__":
    main(sys.argv[1:])
