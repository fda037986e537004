#!/usr/bin/env python3
"""Times the one-call coupled projection mgps_project_free_surface_rigid_slab with a world of one against the composition
fields.project_free_surface_rigid on one device: the scene of tools/coupled_bench.py (projection_scene at N^3, default 480^3, its
box as B bodies of the liquid's density, V* with spin), both from a zero pressure with the same switches, in interleaved repeats in
one process.  The time is the host's wall clock around the call with the device synchronised on both sides; the fields are cloned
outside it.  Prints one JSON line: medians and spreads (max - min) of both, every repeat's time with the one-call's stages and the
composition's solve time beside it, and the iteration counts.

    python tools/projection_rigid_time.py [N] [--bodies 1] [--repeats 7] [--tolerance 1e-7] [--out profiles/NAME.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def world_of_one(Dd):
    """a complete mgps_comm of one rank; a world of one asks it nothing"""
    cm = Dd.CommStruct()
    cm.struct_size, cm.size = C.sizeof(Dd.CommStruct), 1
    keep = [Dd._EXCH(lambda *a: 1), Dd._ALLR(lambda *a: 1)]
    cm.exchange, cm.allreduce = keep
    return types.SimpleNamespace(struct=cm, rank=0, size=1, keep=keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=480)
    ap.add_argument("--bodies", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tolerance", type=float, default=1e-7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from coupled_bench import piece_tables
    from geometricmultigridpressuresolver_amd import distributed as Dd
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd import fields as F
    from solid_forces_bench import box_ids

    n, bodies = a.size, a.bodies
    shape = (n, n, n)
    sc = D.projection_scene(shape)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    phi, solid, cw, vel = dev(sc["liquid_phi"]), dev(sc["solid_phi"]), [dev(x) for x in sc["cut_weights"]], [dev(x) for x in sc["velocity"]]
    body = [dev(x) for x in box_ids(sc, shape, bodies)]
    centres, inv_mass, inv_inertia = piece_tables(n, bodies)
    rng = np.random.default_rng(bodies)
    motions = np.zeros((bodies + 1, 6))
    motions[1:, :3], motions[1:, 3:] = 0.3 * rng.standard_normal((bodies, 3)), 0.3 / n * rng.standard_normal((bodies, 3))
    comm = world_of_one(Dd)
    splits = F.projection_slab_layout(shape, True, 1, True)["splits"]
    kw = dict(use_old_pressure=False, use_gauss_seidel=True, tolerance=a.tolerance, max_iterations=500, power_of_two=True)

    def composed(v, p):
        out = F.project_free_surface_rigid(phi, solid, cw, v, p, body, centres, inv_mass, inv_inertia, motions, **kw)
        return out["stats"]["iterations"], out["motions"], {"solve": out["stats"]["solve_ms"]}

    def one_call(v, p):
        _, info = F.project_free_surface_rigid_slab(comm, splits, shape, phi, solid, cw, v, p, body, centres, inv_mass, inv_inertia, motions, **kw)
        return info["iterations"], info["motions"], info["stage_ms"]

    runs = {"composed": composed, "one_call": one_call}
    t, its, v_out, stages = {k: [] for k in runs}, {}, {}, {k: [] for k in runs}
    for rep in range(a.repeats + 1):  # (the first round warms up: code objects, the allocator's blocks)
        for k, fn in runs.items():  # interleaved: a drift of the clocks meets both alike
            v, p = [x.clone() for x in vel], torch.zeros(shape, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its[k], v_out[k], st = fn(v, p)
            torch.cuda.synchronize()
            if rep:
                t[k].append(1e3 * (time.perf_counter() - t0))
                stages[k].append(st)
    out = {"tool": "projection_rigid_time", "size": n, "bodies": bodies, "repeats": a.repeats, "tolerance": a.tolerance, "iterations": its,
           "total_ms_median": {k: float(np.median(v)) for k, v in t.items()}, "total_ms_spread": {k: float(max(v) - min(v)) for k, v in t.items()},
           "total_ms": t, "stage_ms": stages,
           "motions_out_difference": float(np.abs(v_out["one_call"] - v_out["composed"]).sum() / np.abs(v_out["composed"]).sum())}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
