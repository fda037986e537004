#!/usr/bin/env python3
"""Times the device field passes of include/mgps_fields.h on an N^3 base grid (default 480^3 -> 512^3 solver grid) with HIP events
on torch's stream: ms per pass and algorithmic GB/s (bytes each pass has to move).  The whole-grid passes, the surface-tension
passes, and the slab passes on the one-rank window of the same scene.

    python tools/fields_bench.py [N]                                      one process, one JSON line
    python tools/fields_bench.py [N] --rounds 3 --parent-lib PATH/libmgps.so [--out profiles/NAME.json]

With --parent-lib the two libraries run in turn, --rounds times, every run a fresh process (a library is chosen when it is loaded:
MGPS_LIBRARY) under its own time limit; the first failure ends the job.  A pass counts as unchanged when this build's median is no
more than the parent's median plus the parent's own spread (max - min over its rounds of this same run)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["liquid_phi", "solid_phi", "cw0", "cw1", "cw2", "v0", "v1", "v2", "sv0", "sv1", "sv2"]


def scene(n, scratch):
    """domains.projection_scene at n^3 with solid velocities; with `scratch`, kept there so that every process reads the same arrays"""
    from geometricmultigridpressuresolver_amd import domains as D

    if scratch and os.path.exists(os.path.join(scratch, NAMES[-1] + ".npy")):
        return [np.load(os.path.join(scratch, name + ".npy")) for name in NAMES]
    sc = D.projection_scene((n, n, n), with_solid_velocity=True)
    arrays = [sc["liquid_phi"], sc["solid_phi"], *sc["cut_weights"], *sc["velocity"], *sc["solid_velocity"]]
    if scratch:
        for name, a in zip(NAMES, arrays):
            np.save(os.path.join(scratch, name + ".npy"), a)
    return arrays


def measure(n, scratch):
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    shape = (n, n, n)
    arrays = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in scene(n, scratch)]
    phi, sphi, cw, vel, sv = arrays[0], arrays[1], arrays[2:5], arrays[5:8], arrays[8:11]
    eshape, offset, levels = G.expanded_layout(shape, 5, power_of_two=False)
    cells, ecells = float(n) ** 3, float(np.prod(eshape))
    material = F.buildMaterialCellLabels(phi, sphi, cw)
    valid = F.buildValidFaces(material, cw)
    labels, weights = F.buildMGDomain(material, cw, phi, valid, eshape, offset)
    rhs = F.buildRHS(material, vel, cw, eshape, offset, sv)
    pressure = torch.rand(shape, device="cuda")
    sp = F.buildSurfacePressure(phi, material, 1.0)
    pmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    # the one-rank window of the same scene (the layout the slab call would use: no halo planes)
    lay = F.projection_slab_layout(shape, False, 1, True)
    d = F.slab_window(shape, False, lay["splits"], 0)
    wcells = float(np.prod(d.expanded_shape))
    s_valid, s_weights = F.buildFacesSlab(d, material, None, phi, None, cw)
    s_rhs = F.buildRHSSlab(d, material, vel, cw, sv)
    s_x = torch.rand(d.expanded_shape, device="cuda")

    def timed(fn, reps=20):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # algorithmic bytes: inputs read once + outputs written once, per base cell (b) or expanded cell (e)
    front_b, rhs_b, grad_b = (4 + 4 + 12 + 4) + 3 * (4 + 4 + 1), 4 + 12 + 12 + 12, 3 * (8 + 1) + (4 + 4 + 4)
    passes = [
        ("buildMaterialCellLabels", lambda: F.buildMaterialCellLabels(phi, sphi, cw), (4 + 4 + 12 + 4) * cells),
        ("buildValidFaces x3", lambda: F.buildValidFaces(material, cw), 3 * (4 + 4 + 1) * cells),
        ("buildMGDomain (labels, 3 weights, boundary labels)", lambda: F.buildMGDomain(material, cw, phi, valid, eshape, offset),
         (4 + 3 * (4 + 1 + 4) + 4) * cells + (1 + 12 + 1 + 12 + 1) * ecells),
        ("buildRHS", lambda: F.buildRHS(material, vel, cw, eshape, offset, sv), rhs_b * cells + 4 * ecells),
        ("applyOldPressure", lambda: F.applyOldPressure(pressure, material, eshape, offset), (4 + 4) * cells + 4 * ecells),
        ("applySolutionToPressure", lambda: F.applySolutionToPressure(pressure, rhs, material, offset), (4 + 4 + 4) * cells),
        ("applyPressureGradient x3", lambda: F.applyPressureGradient(vel, phi, pressure, valid, material), grad_b * cells),
        ("computeResultingDivergence", lambda: F.computeResultingDivergence(material, vel, cw, sv), rhs_b * cells),
        # surface tension: labels and sp per cell, phi and the rest on the interface shell only
        ("buildSurfacePressure", lambda: F.buildSurfacePressure(phi, material, 1.0), (4 + 4 + 4) * cells),
        ("addSurfacePressureToRHS", lambda: F.addSurfacePressureToRHS(rhs, weights, phi, material, sp, offset, pmax), 4 * cells),
        ("applyPressureGradient x3, surface", lambda: F.applyPressureGradient(vel, phi, pressure, valid, material, surface_pressure=sp), grad_b * cells),
        ("slab buildMaterialCellLabels", lambda: F.buildMaterialCellLabelsSlab(d, phi, None, sphi, cw), (4 + 4 + 12 + 4) * cells),
        ("slab buildFaces", lambda: F.buildFacesSlab(d, material, None, phi, None, cw), (4 + 4 + 3 * (4 + 1)) * cells + 12 * wcells),
        ("slab buildLabels", lambda: F.buildLabelsSlab(d, material, None, s_weights), 4 * cells + (12 + 1) * wcells),
        ("slab buildRHS", lambda: F.buildRHSSlab(d, material, vel, cw, sv), rhs_b * cells + 4 * wcells),
        ("slab applyOldPressure", lambda: F.applyOldPressureSlab(d, pressure, material), (4 + 4) * cells + 4 * wcells),
        ("slab applySolutionToPressure", lambda: F.applySolutionToPressureSlab(d, pressure, s_x, material, clear_others=True), (4 + 4 + 4) * cells),
        ("slab applyPressureGradient", lambda: F.applyPressureGradientSlab(d, vel, phi, None, pressure, None, s_valid, material, None), grad_b * cells),
        ("slab buildSurfacePressure", lambda: F.buildSurfacePressureSlab(d, phi, None, material, None, 1.0), (4 + 4 + 4) * cells),
        ("slab addSurfacePressureToRHS", lambda: F.addSurfacePressureToRHSSlab(d, s_rhs, s_weights, phi, None, material, None, sp, None, pmax), 4 * cells),
        ("slab applyPressureGradient, surface", lambda: F.applyPressureGradientSlab(d, vel, phi, None, pressure, None, s_valid, material, None, sp, None),
         grad_b * cells),
    ]
    out = {"base_grid": n, "solver_grid": list(eshape), "slab_window": list(d.expanded_shape), "passes": {}}
    for name, fn, nbytes in passes:
        ms = timed(fn)
        out["passes"][name] = {"ms": round(ms, 4), "algorithmic_GBps": round(nbytes / ms / 1e6, 1)}
    return out


def compare(a):
    """the two libraries in turn, every run a process of its own; returns the table"""
    runs = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as scratch:
        scene(a.size, scratch)
        for _ in range(a.rounds):
            for which in ("parent", "this"):
                env = dict(os.environ)
                env.pop("MGPS_LIBRARY", None)
                if which == "parent":
                    env["MGPS_LIBRARY"] = os.path.abspath(a.parent_lib)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.size), "--scratch", scratch], env=env, stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
                line = [ln for ln in res.stdout.splitlines() if ln.startswith('{"base_grid"')]
                if res.returncode != 0 or not line:
                    sys.exit(f"{which} run failed (exit {res.returncode}); nothing further is started\n{res.stdout[-3000:]}")
                runs[which].append(json.loads(line[-1]))
                print(which, line[-1], flush=True)
    table = {}
    for name in runs["this"][0]["passes"]:
        p = [r["passes"][name]["ms"] for r in runs["parent"]]
        t = [r["passes"][name]["ms"] for r in runs["this"]]
        table[name] = {"parent_ms": p, "this_ms": t, "parent_median": float(np.median(p)), "parent_spread": round(max(p) - min(p), 4),
                       "this_median": float(np.median(t)), "unchanged": bool(np.median(t) <= np.median(p) + (max(p) - min(p)))}
    first = runs["this"][0]
    return {"base_grid": first["base_grid"], "solver_grid": first["solver_grid"], "slab_window": first["slab_window"], "rounds": a.rounds,
            "rule": "unchanged: this_median <= parent_median + parent_spread (max - min of the parent's rounds in this run)", "passes": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=480)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="the library of the commit to compare with; without it one run of this build")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a single run may take")
    ap.add_argument("--scratch", default="", help="a directory that holds the scene (or will)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = compare(a) if a.parent_lib else measure(a.size, a.scratch)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if a.parent_lib and not all(v["unchanged"] for v in out["passes"].values()):
        sys.exit("slower than the parent beyond its spread: " + ", ".join(k for k, v in out["passes"].items() if not v["unchanged"]))


if __name__ == "__main__":
    main()
