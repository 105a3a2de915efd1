"""Cost and evidence of mixed precision (hot_set_preconditioner_dtype = 0: an fp32 multigrid hierarchy under an fp64 context), one GPU.

  python tools/mg_precision_cost.py [--steps K] [--configs C2,C4] [--limit SECONDS] [--out profiles/mg_precision.txt]

1. per configuration one context per mode (fp64 hierarchy / fp32 hierarchy), deterministic = 1 so that the iteration counts are comparable, stepped
   ALTERNATELY after one warm-up step each, in one process: ms per step (host wall clock around hot_advance, which synchronises), nonlinear
   iterations, ms per iteration, ms_mg_build;
2. a separate profiled run (cfg.profile = 1), one context at a time, one step per mode after a warm-up step: per-launch times of the V-cycle's
   launches (level-0 colour pass, residual, A P products, the coarse-level sweeps, the top-level PCG), the three launches of the boundary
   (mg32_matrix, mg32_enter, mg32_exit), and the device memory in use;
3. the matrix down-conversion with and without the non-temporal hint (A/B build, HOT_MG32_NT);
4. the convergence bodies of tests/test_gpu_mixed_precision.py: iteration counts and velocity distances.

Bodies: C2 at its bench.py size (63^3 cells), C4 at its per-GPU size (79^3), built with hot_amd.parallel.shard_cloud and a sticky floor like bench.py.
Every step runs under its own time limit (--limit): a step that exceeds it ends the process."""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hot_amd  # noqa: E402
from hot_amd import parallel, synth  # noqa: E402
from tests import mixed_precision_checks as mx  # noqa: E402

SIZES = {"C1": 22, "C2": 63, "C4": 79}
PREFIXES = ("gs_forward", "gs_backward", "gs_residual", "gs_", "apmv_", "cg_", "spmv_L", "restrict", "prolong", "vcycle_start", "diag_scale", "mg32_")
MODES = (("fp64", 1), ("mixed", 0))


def make(lib, cname, cloud, **kw):
    cfg = synth.CONFIGS[cname]
    args = dict(dtype=1, dx=cloud["dx"], gravity=(0, -9.8, 0), levelCnt=cfg["levelCnt"], deterministic=1)
    args.update(synth.plasticity_kwargs(cfg))
    args.update(kw)
    ctx = lib.context(**args)
    ctx.set_particles(cloud["X"], cloud["V"], cloud["mass"], cloud["vol"], cloud["mu"], cloud["lam"])
    o, n = synth.sticky_floor(cloud["corner"][1], cloud["dx"])
    ctx.set_sticky_halfspaces(o, n)
    return ctx


class Limit:
    """a step under its own time limit: the process ends (exit status 124) when the body takes longer"""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expired, (what, seconds))
        self.t.daemon = True

    @staticmethod
    def _expired(what, seconds):
        sys.stderr.write(f"mg_precision_cost: {what} exceeded its limit of {seconds} s\n")
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *a):
        self.t.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-bodies", action="store_true")
    args = ap.parse_args()
    lib = hot_amd.load()
    fout = open(args.out, "w") if args.out else None

    def say(s=""):
        print(s, flush=True)
        if fout:  # line by line: a step that exceeds its limit ends the process, what was measured before it stays
            fout.write(s + "\n")
            fout.flush()

    names = args.configs.split(",")
    say(f"mixed precision (fp32 multigrid hierarchy under an fp64 context), {lib.version()}; bodies: " + ", ".join(f"{c} {SIZES[c]}^3 cells" for c in names) + "; deterministic = 1")
    say()
    say(f"1. whole steps, modes alternating, {args.steps} timed steps per mode after one warm-up step each (ms_mg_build: mean over the timed steps; warm-up: the first build, which allocates)")
    say(f"{'config':7s} {'particles':>9s} {'mode':>6s} {'ms/step':>9s} {'iterations':>14s} {'ms/iteration':>13s} {'ms_mg_build':>12s} {'warm-up build':>14s} {'ms_hessian':>11s} {'ms_solve':>9s}")
    clouds = {}
    for c in names:
        cfg = synth.CONFIGS[c]
        cloud = parallel.shard_cloud(cfg, 0, 1, n=SIZES[c])
        clouds[c] = cloud
        ctx = [make(lib, c, cloud, preconditioner_dtype=pd) for _, pd in MODES]
        warm = []
        for m in (0, 1):
            with Limit(args.limit, f"{c} warm-up step, {MODES[m][0]}"):
                warm.append(ctx[m].advance(cfg["dt"]))
        rec = [[], []]
        for s in range(args.steps):
            for m in (0, 1):
                with Limit(args.limit, f"{c} step {s}, {MODES[m][0]}"):
                    t0 = time.perf_counter()
                    st = ctx[m].advance(cfg["dt"])
                    rec[m].append((1e3 * (time.perf_counter() - t0), st))
        del ctx
        for m in (0, 1):
            ms = np.mean([r[0] for r in rec[m]])
            its = [r[1]["iterations"] for r in rec[m]]
            per = np.mean([r[1]["ms_solve"] / max(r[1]["iterations"], 1) for r in rec[m]])
            say(f"{c:7s} {cloud['X'].shape[0]:9d} {MODES[m][0]:>6s} {ms:9.1f} {str(its):>14s} {per:13.3f} {np.mean([r[1]['ms_mg_build'] for r in rec[m]]):12.1f} {warm[m]['ms_mg_build']:14.1f} "
                f"{np.mean([r[1]['ms_hessian'] for r in rec[m]]):11.1f} {np.mean([r[1]['ms_solve'] for r in rec[m]]):9.1f}")
        a, b = np.mean([r[0] for r in rec[0]]), np.mean([r[0] for r in rec[1]])
        say(f"{c:7s} mixed / fp64 per step: {b / a:.3f}")

    say()
    say("2. per-launch times of one profiled step per mode (cfg.profile = 1, after a warm-up step, one context at a time): us per launch [launches]; device memory in use after the step")
    for c in names:
        cfg = synth.CONFIGS[c]
        prof, stats, mem = [], [], []
        for name, pd in MODES:
            ctx = make(lib, c, clouds[c], preconditioner_dtype=pd, profile=1)
            with Limit(args.limit, f"{c} profiled warm-up, {name}"):
                ctx.advance(cfg["dt"])
            ctx.profile_reset()
            with Limit(args.limit, f"{c} profiled step, {name}"):
                stats.append(ctx.advance(cfg["dt"]))
            prof.append(ctx.profile())
            mem.append(mx.device_mib_used())
            del ctx
        labels = sorted(k for k in set(prof[0]) | set(prof[1]) if k.startswith(PREFIXES) or k.startswith("mg_"))
        say(f"{c}: iterations fp64 {stats[0]['iterations']} mixed {stats[1]['iterations']}, V-cycles {stats[0]['vcycles']} / {stats[1]['vcycles']}, levels {stats[0]['num_levels']} / {stats[1]['num_levels']}; "
            f"device MiB in use fp64 {mem[0]:.0f} mixed {mem[1]:.0f}")
        say(f"{'label':28s} {'fp64 us/launch':>15s} {'[n]':>7s} {'mixed us/launch':>16s} {'[n]':>7s} {'mixed / fp64':>13s}")
        for k in labels:
            a, b = prof[0].get(k), prof[1].get(k)
            ua = 1e3 * a["total_ms"] / a["calls"] if a and a["calls"] else float("nan")
            ub = 1e3 * b["total_ms"] / b["calls"] if b and b["calls"] else float("nan")
            say(f"{k:28s} {ua:15.1f} {a['calls'] if a else 0:7d} {ub:16.1f} {b['calls'] if b else 0:7d} {ub / ua if ua == ua and ub == ub and ua > 0 else float('nan'):13.2f}")
        tot = [sum(v["total_ms"] for v in p.values()) for p in prof]
        vc = [sum(v["total_ms"] for k, v in p.items() if k.startswith(PREFIXES)) for p in prof]
        say(f"{'all launches, ms':28s} {tot[0]:15.1f} {'':7s} {tot[1]:16.1f} {'':7s} {tot[1] / tot[0]:13.2f}")
        say(f"{'the labels above, ms':28s} {vc[0]:15.1f} {'':7s} {vc[1]:16.1f} {'':7s} {vc[1] / vc[0]:13.2f}")
        say()

    if os.path.exists(hot_amd.AB_LIB_PATH):
        say("3. mg32_matrix (fp64 level 0 -> fp32, 16-byte loads and stores) with and without the non-temporal hint (A/B build, HOT_MG32_NT), us per launch")
        ab = hot_amd.HotLib(hot_amd.AB_LIB_PATH)
        for c in names:
            cfg = synth.CONFIGS[c]
            ctx = make(ab, c, clouds[c], preconditioner_dtype=0, profile=1)
            ctx.sort(), ctx.p2g(), ctx.begin_step(cfg["dt"])
            ctx.update_state(ctx.get_dv())
            ctx.build_hessian()
            out = {}
            for nt in (0, 1, 0, 1):
                os.environ.pop("HOT_MG32_NT", None)
                if nt:
                    os.environ["HOT_MG32_NT"] = "1"
                ctx.profile_reset()
                with Limit(args.limit, f"{c} hot_build_mg, NT {nt}"):
                    ctx.build_mg()
                p = ctx.profile()["mg32_matrix"]
                out.setdefault(nt, []).append(1e3 * p["total_ms"] / p["calls"])
            os.environ.pop("HOT_MG32_NT", None)
            n = ctx.level(0, coords=False)["nrows"]
            gb = n * 1125 * 12 / 1e9
            say(f"{c}: {n} rows, {gb:.2f} GB moved; plain {[round(v, 1) for v in out[0]]} us ({gb / (min(out[0]) * 1e-6) / 1e3:.2f} TB/s), non-temporal {[round(v, 1) for v in out[1]]} us ({gb / (min(out[1]) * 1e-6) / 1e3:.2f} TB/s)")
            del ctx
        say()

    if not args.skip_bodies:
        say("4. convergence bodies (tests/test_gpu_mixed_precision.py item 5): one step from identical states, deterministic = 1, lsolver 3")
        say(f"{'body':16s} {'it fp64 L3':>10s} {'it fp64 L2':>10s} {'it mixed':>9s} {'conv':>5s} {'exit(fp64 test)':>16s} {'|v mixed - v fp64|':>19s} {'|v fp64 L2 - v fp64 L3|':>24s}")
        for body in mx.BODIES:
            res = []
            for kw in (dict(levelCnt=3), dict(levelCnt=2), dict(levelCnt=3, preconditioner_dtype=0)):
                ctx, cfg = mx.make_body(lib, body, deterministic=1, lsolver=3, **kw)
                with Limit(args.limit, f"{body} {kw}"):
                    st, ex, scaled = mx.step_members(ctx, cfg["dt"])
                res.append((st, ex, scaled, ctx.get_particles()))
                del ctx
            say(f"{body:16s} {res[0][0]['iterations']:10d} {res[1][0]['iterations']:10d} {res[2][0]['iterations']:9d} {res[2][0]['converged']:5d} {int(res[2][1]):6d} ({res[2][2]:.3f}) "
                f"{mx.velocity_distance(res[2][3], res[0][3]):19.3e} {mx.velocity_distance(res[1][3], res[0][3]):24.3e}")
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
