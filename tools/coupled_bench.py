#!/usr/bin/env python3
"""Times mgps_solve_pcg_coupled against mgps_solve_pcg under pcg_fp64_vectors = 1 (the loop it hooks into) on one solver:
projection_scene at N^3 (default 480^3) with its box as one body or cut into B bodies by z planes, bodies of the liquid's density,
V* with spin.  Both solves start from zero on the same right-hand side b = buildRHS(u, rigidVelocity(V*)) and run in interleaved
repeats in one process; the time is the library's own event pair around the solve (stats.solve_ms).  Prints one JSON line per body
count: medians and spreads (max - min) of the solve time, the iteration counts, the solve time over the iterations and the
difference of the two quotients (a solve's set-up passes are spread over its iterations: where the counts differ much, time the list
kernels with rocprofv3 --kernel-trace --stats instead).

    python tools/coupled_bench.py [N] [--bodies 1 255] [--repeats 7] [--tolerance 1e-7] [--out profiles/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def piece_tables(n, bodies):
    """centres, inv_mass, inv_inertia for the ids of solid_forces_bench.box_ids (1 + k % bodies: one id per z plane of the box of
    projection_scene): every id is taken as a plate of 1 / bodies of the box's height and the liquid's density, about the box's centre"""
    lo, hi = np.array([0.31, 0.27, 0.18]) * n, np.array([0.62, 0.71, 0.44]) * n
    ext = hi - lo
    ext[2] = max(ext[2] / bodies, 1.0)
    mass = ext.prod()
    centres, inv_mass, inv_inertia = np.zeros((bodies + 1, 3)), np.zeros(bodies + 1), np.zeros((bodies + 1, 6))
    centres[1:] = 0.5 * (lo + hi)
    inv_mass[1:] = 1.0 / mass
    inv_inertia[1:, 0] = 12.0 / (mass * (ext[1] ** 2 + ext[2] ** 2))
    inv_inertia[1:, 1] = 12.0 / (mass * (ext[0] ** 2 + ext[2] ** 2))
    inv_inertia[1:, 2] = 12.0 / (mass * (ext[0] ** 2 + ext[1] ** 2))
    return centres, inv_mass, inv_inertia


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=480)
    ap.add_argument("--bodies", type=int, nargs="+", default=[1, 255])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tolerance", type=float, default=1e-7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd import fields as F
    from solid_forces_bench import box_ids

    n = a.size
    shape = (n, n, n)
    sc = D.projection_scene(shape)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    phi, cw, vel = dev(sc["liquid_phi"]), [dev(x) for x in sc["cut_weights"]], [dev(x) for x in sc["velocity"]]
    material = F.buildMaterialCellLabels(phi, dev(sc["solid_phi"]), cw)
    valid = F.buildValidFaces(material, cw)
    eshape, offset, levels = G.expanded_layout(shape, 0, power_of_two=True)
    labels, weights = F.buildMGDomain(material, cw, phi, valid, eshape, offset)
    opt = G.default_options()
    opt.pcg_fp64_vectors = 1
    solver = G.GeometricMultigridPoissonSolver(labels, weights, levels, True, options=opt)
    results = []
    for bodies in a.bodies:
        body = [dev(x) for x in box_ids(sc, shape, bodies)]
        centres, inv_mass, inv_inertia = piece_tables(n, bodies)
        rng = np.random.default_rng(bodies)
        motions = np.zeros((bodies + 1, 6))
        motions[1:, :3], motions[1:, 3:] = 0.3 * rng.standard_normal((bodies, 3)), 0.3 / n * rng.standard_normal((bodies, 3))
        sv = F.rigidVelocity([torch.zeros_like(w) for w in cw], body, centres, motions)
        rhs = F.buildRHS(material, vel, cw, eshape, offset, sv)
        coupling = F.RigidCoupling(material, cw, body, centres, inv_mass, inv_inertia, eshape, offset)
        x = torch.zeros_like(rhs)
        runs = {"uncoupled": lambda: solver.solveGeometricConjugateGradient(x, rhs, a.tolerance, 500, True),
                "coupled": lambda: solver.solve_pcg_coupled(coupling, x, rhs, a.tolerance, 500, True)}
        t, its = {k: [] for k in runs}, {}
        for k, fn in runs.items():  # warm-up: code objects, the solver's CG grids
            x.zero_()
            fn()
        for _ in range(a.repeats):  # interleaved: a drift of the clocks meets both alike
            for k, fn in runs.items():
                x.zero_()
                st = fn()
                assert st["outcome"] == "converged", st
                t[k].append(st["solve_ms"])
                its[k] = st["iterations"]
        med = {k: float(np.median(v)) for k, v in t.items()}
        per = {k: med[k] / max(its[k], 1) for k in runs}
        out = {"tool": "coupled_bench", "size": n, "expanded": list(eshape), "bodies": bodies, "coupled_cells": coupling.cells(), "repeats": a.repeats,
               "tolerance": a.tolerance, "iterations": its, "solve_ms_median": med, "solve_ms_spread": {k: float(max(v) - min(v)) for k, v in t.items()},
               "ms_per_iteration": per, "coupling_us_per_iteration": 1e3 * (per["coupled"] - per["uncoupled"])}
        coupling.close()
        print(json.dumps(out), flush=True)
        results.append(out)
    solver.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
