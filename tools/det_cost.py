"""Cost and evidence of deterministic mode (hot_config.deterministic = 1), one GPU.

  python tools/det_cost.py [--steps K] [--reps R] [--configs C1,C2,...] [--out FILE]

1. per configuration, one context per mode, stepped ALTERNATELY (0, 1, 0, 1, ...) after one warm-up step each: ms per step (host wall clock
   around hot_advance, which synchronises) and nonlinear iterations per step;
2. a separate profiled run (cfg.profile = 1), one step per mode after a warm-up step: per-launch-label kernel times of the scatter passes;
3. R repetitions of one step per mode on a fresh context of C1 and of C4's per-GPU body: the number of distinct sha256 digests of the
   particle state and of the stats without their ms_* fields.

Bodies: C1 - C3 at their bench.py sizes (synth.CONFIGS), C4 / C5 at their per-GPU sizes (79 / 100 cells per edge: 16 M particles over 4 GPUs,
64 M over 8), all built with hot_amd.parallel.shard_cloud and a sticky floor like bench.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hot_amd  # noqa: E402
from hot_amd import parallel, synth  # noqa: E402
from tests.det_scenes import PARTICLE_KEYS, digest_arrays, digest_stats  # noqa: E402

SIZES = {"C1": 22, "C2": 63, "C3": 100, "C4": 79, "C5": 100}
LABELS = [("p2g", "p2g_det"), ("force_scatter", "force_scatter_det"), ("hessian_assemble", "hessian_assemble_det"),
          ("matfree_hessian_product", "matfree_hessian_product_det"), ("matfree_diag_scatter", "matfree_diag_scatter_det")]


def make(lib, cname, cloud, **kw):
    cfg = synth.CONFIGS[cname]
    args = dict(dtype=1 if cfg["dtype"] == np.float64 else 0, dx=cloud["dx"], gravity=(0, -9.8, 0), levelCnt=cfg["levelCnt"])
    args.update(synth.plasticity_kwargs(cfg))
    args.update(kw)
    ctx = lib.context(**args)
    ctx.set_particles(cloud["X"], cloud["V"], cloud["mass"], cloud["vol"], cloud["mu"], cloud["lam"])
    o, n = synth.sticky_floor(cloud["corner"][1], cloud["dx"])
    ctx.set_sticky_halfspaces(o, n)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="C1,C2,C3,C4,C5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = hot_amd.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    names = args.configs.split(",")
    say(f"deterministic mode cost, {lib.version()}; bodies: " + ", ".join(f"{c} {SIZES[c]}^3 cells" for c in names))
    clouds = {}
    say("")
    say(f"1. whole steps, modes alternating, {args.steps} timed steps per mode after one warm-up step each")
    say(f"{'config':8s} {'particles':>10s} {'ms/step det=0':>14s} {'ms/step det=1':>14s} {'ratio':>7s} {'iters/step det=0':>17s} {'iters/step det=1':>17s}")
    for c in names:
        cfg = synth.CONFIGS[c]
        cloud = parallel.shard_cloud(cfg, 0, 1, n=SIZES[c])
        clouds[c] = cloud
        ctx = [make(lib, c, cloud, deterministic=0), make(lib, c, cloud, deterministic=1)]
        for m in (0, 1):
            ctx[m].advance(cfg["dt"])
        ms, its = [[], []], [[], []]
        for _ in range(args.steps):
            for m in (0, 1):
                t0 = time.perf_counter()
                st = ctx[m].advance(cfg["dt"])
                ms[m].append(1e3 * (time.perf_counter() - t0))
                its[m].append(st["iterations"])
        del ctx
        a, b = np.mean(ms[0]), np.mean(ms[1])
        say(f"{c:8s} {cloud['X'].shape[0]:10d} {a:14.1f} {b:14.1f} {b / a:7.2f} {np.mean(its[0]):17.1f} {np.mean(its[1]):17.1f}")

    say("")
    say("2. per-label kernel times of one profiled step per mode (cfg.profile = 1, after a warm-up step), ms [calls]")
    for c in names:
        cfg = synth.CONFIGS[c]
        prof = []
        for m in (0, 1):
            ctx = make(lib, c, clouds[c], deterministic=m, profile=1)
            ctx.advance(cfg["dt"])
            ctx.profile_reset()
            st = ctx.advance(cfg["dt"])
            prof.append((ctx.profile(), st))
            del ctx
        for a, b in LABELS:
            pa, pb = prof[0][0].get(a), prof[1][0].get(b)
            if pa is None and pb is None:
                continue
            fa = f"{pa['total_ms']:9.3f} [{pa['calls']:4d}]" if pa else f"{'-':>16s}"
            fb = f"{pb['total_ms']:9.3f} [{pb['calls']:4d}]" if pb else f"{'-':>16s}"
            ratio = (pb["total_ms"] / pb["calls"]) / (pa["total_ms"] / pa["calls"]) if (pa and pb and pa["total_ms"] > 0) else float("nan")
            say(f"{c:8s} {a:28s} {fa}   {b:32s} {fb}   per call x{ratio:5.2f}")
        tot = [sum(v["total_ms"] for v in p.values()) for p, _ in prof]
        say(f"{c:8s} {'all kernels':28s} {tot[0]:9.3f}          {'all kernels':32s} {tot[1]:9.3f}          (iterations {prof[0][1]['iterations']} / {prof[1][1]['iterations']})")

    say("")
    say(f"3. distinct digests of the particle state and stats (ms_* excluded) over {args.reps} repetitions of one step on a fresh context")
    for c in ("C1", "C4"):
        cfg = synth.CONFIGS[c]
        cloud = clouds.get(c) or parallel.shard_cloud(cfg, 0, 1, n=SIZES[c])
        for m in (0, 1):
            dig, its = set(), []
            for _ in range(args.reps):
                ctx = make(lib, c, cloud, deterministic=m)
                st = ctx.advance(cfg["dt"])
                p = ctx.get_particles()
                dig.add((digest_arrays([p[k] for k in PARTICLE_KEYS]), digest_stats(st)))
                its.append(st["iterations"])
                del ctx
            say(f"{c:8s} {SIZES[c]}^3 cells  deterministic={m}: {len(dig)} distinct digest(s) in {args.reps} runs; iterations {its}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
