#!/usr/bin/env python3
"""Surface tension on one MI355X: cost of its device passes and of the projection with it.

    python tools/surface_tension_time.py [--size 480] [--rounds 3] [--out profiles/r07_surface_tension_480.json]

On domains.projection_scene at --size^3 (tight solver grid, as the Houdini shim builds it):
- the three new passes (surface pressure, rhs term, gradient with p_G x3) and, in the same run, the plain rhs and gradient passes,
  each timed with HIP events on torch's stream (mean of 20 launches after one warm-up);
- mgps_project_free_surface with sigma = 0 and sigma > 0, interleaved, --rounds each: the call's own clocks, the time outside the
  solve (total_ms - solve_ms) and the PCG iteration counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402


def timed(fn, reps=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.size
    shape = (n, n, n)
    sc = D.projection_scene(shape, with_solid_velocity=True)
    dx, dt, density = sc["dx"], 1.0 / 60.0, 1000.0
    sigma = 1.0 * density * dx * dx / dt  # s = sigma dt / (density dx^2) = 1: sp = kappa (grid units)
    out = {"size": n, "device": torch.cuda.get_device_name(0), "sigma": sigma, "dt": dt, "dx": dx, "density": density, "scale": 1.0}

    # ---- device passes ----
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    cw = [dev(x) for x in sc["cut_weights"]]
    phi, sphi = dev(sc["liquid_phi"]), dev(sc["solid_phi"])
    vel = [dev(x) for x in sc["velocity"]]
    sv = [dev(x) for x in sc["solid_velocity"]]
    eshape, offset, levels = G.expanded_layout(shape, 0, power_of_two=False)
    material = F.buildMaterialCellLabels(phi, sphi, cw)
    valid = F.buildValidFaces(material, cw)
    labels, weights = F.buildMGDomain(material, cw, phi, valid, eshape, offset)
    rhs = F.buildRHS(material, vel, cw, eshape, offset, sv)
    sp = F.buildSurfacePressure(phi, material, 1.0)
    pmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    pressure = torch.where(material == 1, torch.rand(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    torch.cuda.synchronize()
    cells = float(n) ** 3
    interface = int((sp != 0).sum().item())
    passes = {
        "surface_pressure": timed(lambda: F.buildSurfacePressure(phi, material, 1.0)),
        "rhs_plain": timed(lambda: F.buildRHS(material, vel, cw, eshape, offset, sv)),
        "rhs_surface_term": timed(lambda: F.addSurfacePressureToRHS(rhs, weights, phi, material, sp, offset, pmax)),
        "gradient_plain_x3": timed(lambda: F.applyPressureGradient(vel, phi, pressure, valid, material)),
        "gradient_surface_x3": timed(lambda: F.applyPressureGradient(vel, phi, pressure, valid, material, surface_pressure=sp)),
    }
    passes = {k: round(v, 4) for k, v in passes.items()}
    out["passes_ms"] = passes
    out["interface_cells"] = interface
    # the surface-pressure pass reads the labels (4 B) and writes sp (4 B) per cell, phi (4 B) where it matters: ~12 B per cell
    out["surface_pressure_GBps_at_12B_per_cell"] = round(12 * cells / passes["surface_pressure"] / 1e6, 1)
    out["ratios"] = {
        "rhs_with_term_over_plain": round((passes["rhs_plain"] + passes["rhs_surface_term"]) / passes["rhs_plain"], 3),
        "gradient_surface_over_plain": round(passes["gradient_surface_x3"] / passes["gradient_plain_x3"], 3),
    }
    del cw, phi, sphi, vel, sv, material, valid, labels, weights, rhs, sp, pressure
    torch.cuda.empty_cache()

    # ---- the projection, sigma = 0 against sigma > 0, interleaved ----
    runs = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name in ("off", "on"):
            v = [x.copy() for x in sc["velocity"]]
            p = np.zeros(shape, dtype=np.float32)
            kw = dict(surface_tension=sigma, dt=dt, dx=dx, density=density) if name == "on" else {}
            _, info = F.project_free_surface(sc["liquid_phi"], sc["solid_phi"], sc["cut_weights"], v, p, sc["solid_velocity"],
                                             use_old_pressure=False, tolerance=1e-5, max_iterations=500, power_of_two=False, **kw)
            runs[name].append({"iterations": info["iterations"], "outcome": info["outcome"], "setup_ms": round(info["setup_ms"], 2),
                               "solve_ms": round(info["solve_ms"], 2), "total_ms": round(info["total_ms"], 2),
                               "outside_solve_ms": round(info["total_ms"] - info["solve_ms"], 2),
                               "surface_pressure_max": info["surface_pressure_max"], "divergence_max": info["divergence_max"]})
            print(name, json.dumps(runs[name][-1]), flush=True)
    out["projection"] = runs
    med = {k: float(np.median([r["outside_solve_ms"] for r in v])) for k, v in runs.items()}
    out["outside_solve_ms_median"] = med
    out["outside_solve_delta_ms"] = round(med["on"] - med["off"], 2)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
