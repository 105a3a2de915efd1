"""Worker of the two-rank test of the per-particle plasticity classes (tests/test_gpu_plasticity_classes.py): multirank_worker's cube, five classes drawn
per global particle id, and a deliberately poor starting partition — rank r holds the particles whose global id is r modulo the number of ranks — so that
the first hot_sort hands about half of them to the other rank, each with its class."""
import os
import sys

import numpy as np

from tests import multirank_worker as mw

CLASSES = [
    dict(kind=0),
    dict(kind=1, yield_stress=30.0),
    dict(kind=2, snow=(10, 2e-2, 7.5e-3, 0.6, 20)),
    dict(kind=1, yield_stress=300.0),
    dict(kind=2, snow=(0, 0.01, 0.001, -2, 5)),
]


def classes_of(n_particles):
    return np.random.default_rng(11).integers(0, 5, n_particles).astype(np.int32)


def run_case(lib, cloud, cls, comm, cfgkw, dt=1.0 / 24):
    """One solve with the iteration cap of cfgkw, then G2P with the class table."""
    from hot_amd import synth
    ctx = lib.context(dx=cloud["dx"], gravity=(0, -9.8, 0), **cfgkw)
    if comm is not None:
        ctx.set_comm(comm)
    ctx.set_particles(cloud["X"], cloud["V"], cloud["mass"], cloud["vol"], cloud["mu"], cloud["lam"])
    if comm is not None:
        ctx.set_particle_ids(cloud["index"])
    ctx.set_plasticity_classes(CLASSES, cls)
    o, nrm = synth.sticky_floor(5.0, cloud["dx"])
    ctx.set_sticky_halfspaces(o, nrm)
    ctx.sort(), ctx.p2g(), ctx.begin_step(dt)
    out = dict(stats=ctx.solve())
    ctx.g2p(dt)
    out["particles"] = ctx.get_particles()
    out["ids"] = ctx.particle_ids() if comm is not None else np.arange(len(out["particles"]["X"]), dtype=np.int32)
    out["cls"] = ctx.plasticity_classes()[1]
    return out


def worker(rank, world, port, q, n, dtype, cfgkw):
    sys.path.insert(0, mw.ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("OMP_NUM_THREADS", "2")
    try:
        import torch
        import torch.distributed as dist
        import hot_amd
        from hot_amd import dist as hdist
        dev = rank % torch.cuda.device_count()
        torch.cuda.set_device(dev)
        lib = hot_amd.load()
        dist.init_process_group("gloo", rank=rank, world_size=world)
        comm = hdist.TorchComm(device=torch.device("cuda", dev), partition_min_rows=1)
        cloud = mw.scene(n, dtype)
        sel = np.arange(rank, len(cloud["X"]), world)
        shard = {k: (v[sel] if isinstance(v, np.ndarray) and len(v) == len(cloud["X"]) else v) for k, v in cloud.items()}
        shard["index"] = sel.astype(np.int32)
        out = run_case(lib, shard, classes_of(len(cloud["X"]))[sel], comm, dict(cfgkw, dtype=dtype, device=dev))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # surface the failure in the parent instead of hanging it
        import traceback
        q.put((rank, dict(error=traceback.format_exc())))
        raise


def launch(world, n, dtype, cfgkw, timeout=900):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() * 7 + n + 311) % 2000
    procs = [ctx.Process(target=worker, args=(r, world, port, q, n, dtype, cfgkw)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=timeout)
            if "error" in out:
                raise RuntimeError(f"rank {r} failed:\n{out['error']}")
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    for p in procs:
        if p.exitcode != 0:
            raise RuntimeError(f"a rank exited with code {p.exitcode}")
    return [res[r] for r in range(world)]


def single(lib, n, dtype, cfgkw):
    cloud = mw.scene(n, dtype)
    return run_case(lib, cloud, classes_of(len(cloud["X"])), None, dict(cfgkw, dtype=dtype))
