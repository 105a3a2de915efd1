"""What the per-particle plasticity classes cost in G2P: the kernel of hot_config.plasticity (profile label g2p) against
k_g2p<T, 3> (label g2p_classes) on one MI355X, at the per-GPU bodies of C4 (79^3 cells, fp64, von Mises) and C5 (100^3 cells, fp32, snow).

  python tools/plasticity_classes_cost.py [--reps 5] [--out profiles/plasticity_classes.txt]

Variants, alternating within one process: hot_config.plasticity alone; a one-class table of the same kind; five classes (none, the
configuration's own mapping, the other mapping, and one more of each) assigned by x-slab (wavefronts of one class); the same five drawn at random per
particle (divergent wavefronts).  Every repetition starts from the same particle state (hot_set_particles again), runs sort / P2G / begin_step and one G2P
at dt = 2e-3 (strains of ~1 %: past both yield criteria, as tests/test_gpu_fullsize.py); the figure is the HIP-event time of the G2P launch
(hot_config.profile = 1) averaged over the repetitions after a warm-up.  Registers and wavefronts per SIMD come from the code objects."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hot_amd  # noqa: E402
from hot_amd import kernel_resources as kr, parallel, synth  # noqa: E402

DT = 2e-3
SNOW_DEFAULT = (10, 2e-2, 7.5e-3, 0.6, 20)


def variants(cfg, cloud):
    """name -> (hot_config overrides, class table or None, particle classes or None)"""
    n = cloud["X"].shape[0]
    own = synth.plasticity_kwargs(cfg)
    kind = own["plasticity"]
    one = dict(kind=kind, yield_stress=own.get("yield_stress", 0.0), snow=own.get("snow", SNOW_DEFAULT))
    ys = own.get("yield_stress", 1e-3 * cfg["E"])
    five = [dict(kind=0), dict(kind=1, yield_stress=ys), dict(kind=2, snow=own.get("snow", SNOW_DEFAULT)), dict(kind=1, yield_stress=10 * ys), dict(kind=2, snow=(0.0, 0.01, 0.001, -2.0, 5.0))]
    x = (cloud["X"][:, 0].astype(np.float64) - cloud["corner"][0]) / (cloud["cells"] * cloud["dx"])
    slab = np.clip((x * 5).astype(np.int32), 0, 4)
    rnd = np.random.default_rng(11).integers(0, 5, n).astype(np.int32)
    return {
        "cfg.plasticity = %d" % kind: (own, None, None),
        "one class, kind %d" % kind: ({}, [one], np.zeros(n, np.int32)),
        "five classes by x-slab": ({}, five, slab),
        "five classes at random": ({}, five, rnd),
    }


def measure(lib, cname, n, reps):
    cfg = synth.CONFIGS[cname]
    cloud = parallel.shard_cloud(cfg, 0, 1, n=n)
    f64 = cfg["dtype"] == np.float64
    ctxs = {}
    for name, (over, table, pcl) in variants(cfg, cloud).items():
        ctxs[name] = (lib.context(dtype=1 if f64 else 0, dx=cloud["dx"], gravity=(0, -9.8, 0), levelCnt=cfg["levelCnt"], profile=1, debug_store=0, **over), table, pcl)
    ms = {name: [] for name in ctxs}
    for rep in range(reps + 1):  # the first one warms up
        for name, (ctx, table, pcl) in ctxs.items():
            ctx.set_particles(cloud["X"], cloud["V"], cloud["mass"], cloud["vol"], cloud["mu"], cloud["lam"])
            if table is not None:
                ctx.set_plasticity_classes(table, pcl)
            ctx.sort(), ctx.p2g(), ctx.begin_step(DT)
            ctx.profile_reset()
            ctx.g2p(DT)
            prof = ctx.profile()
            label = "g2p_classes" if table is not None else "g2p"
            assert prof[label]["calls"] == 1 and ("g2p" if table is not None else "g2p_classes") not in prof, prof.keys()
            if rep > 0:
                ms[name].append(prof[label]["total_ms"])
    return cloud["X"].shape[0], {name: (float(np.mean(v)), float(np.min(v)), float(np.max(v))) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plasticity_classes.txt"))
    args = ap.parse_args()
    lib = hot_amd.load()
    res = {k["name"]: k for k in kr.read(hot_amd.LIB_PATH)} if kr.tools_missing() is None else {}
    lines = ["G2P with per-particle plasticity classes against hot_config.plasticity (tools/plasticity_classes_cost.py): HIP-event ms per launch, one MI355X,",
             "dt = %g, %d repetitions after a warm-up, variants alternating within one process" % (DT, args.reps), ""]
    for cname, n, kind, T in (("C4", 79, 1, "double"), ("C5", 100, 2, "float")):
        Np, ms = measure(lib, cname, n, args.reps)
        lines.append("%s per GPU: %d^3 cells, %d particles, %s" % (cname, n, Np, T))
        base = None
        for name, (mean, lo, hi) in ms.items():
            base = mean if base is None else base
            lines.append("  %-28s %8.3f ms  (min %.3f, max %.3f)  x %.3f" % (name, mean, lo, hi, mean / base))
        for kname in ("hot::k_g2p<%s, %d, true>" % (T, kind), "hot::k_g2p<%s, 3, true>" % T):
            if kname in res:
                k = res[kname]
                lines.append("  %-28s %d VGPRs, %d spilled, %d B scratch per lane, %d B LDS, %d wavefronts per SIMD" % (kname[5:], k["vgpr"], k["vgpr_spill"], k["scratch"], k["lds"], k["waves_per_simd"]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
