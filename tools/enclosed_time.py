"""options.enclosed_liquid on one MI355X: set-up cost of the labelling and solve cost of the projection.

    python tools/enclosed_time.py [--size 512] [--reps 3] [--out profiles/r06_enclosed_512.json]

Cases: the free-surface pool (BASELINE config 3: no enclosed component, so the labelling is the only extra work) with the option
off / on, interleaved; a sealed tank (liquid in the EXTERIOR shell, no DIRICHLET cell) with the option on against the same tank
with its top liquid layer DIRICHLET.  Set-up = wall time of the constructor (device set-up, synchronised), median of --reps."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402


def tank(n, levels, open_top):
    s = 2 ** (levels - 1)
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[s:n - s, s:n - s, s:n - s] = D.INTERIOR
    if open_top:
        lab[n - s - 1, s:n - s, s:n - s] = D.DIRICHLET
    w = [np.ones(D.face_shape(n, n, n, a), dtype=np.float32) for a in range(3)]
    D.set_boundary_labels(lab, w)
    return lab, w


def build(lab, w, levels, enclosed):
    o = G.default_options()
    o.enclosed_liquid = enclosed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = G.GeometricMultigridPoissonSolver(lab, w, levels, False, options=o)
    torch.cuda.synchronize()
    return s, (time.perf_counter() - t0) * 1e3


def solve(s, b, tol=1e-6):
    bd = s.to_device(b)
    s.solveGeometricConjugateGradient(s.new_grid(), bd, tol, 400, True)  # warm-up (first-use grids)
    st = s.solveGeometricConjugateGradient(s.new_grid(), bd, tol, 400, True)
    return {"iterations": st["iterations"], "solve_ms": st["solve_ms"], "ms_per_iteration": st["solve_ms"] / max(1, st["iterations"]),
            "outcome": st["outcome"], "rel_residual": st["rel_residual"], "rel_residual_recomputed": st["rel_residual_recomputed"]}


def history(lab, w, levels, gs, mode, b, tol=1e-6):
    """the residual after every iteration (options.print_stats prints it on the library's stdout: captured through a file)"""
    import tempfile

    o = G.default_options()
    o.enclosed_liquid, o.pcg_fp64_vectors = 1, mode
    s = G.GeometricMultigridPoissonSolver(lab, w, levels, gs, options=o)
    x, bd = s.new_grid(), s.to_device(b)
    s.synchronize()
    sys.stdout.flush()
    with tempfile.TemporaryFile(mode="w+") as f:
        saved = os.dup(1)
        os.dup2(f.fileno(), 1)
        try:
            s2 = G.GeometricMultigridPoissonSolver(lab, w, levels, gs, do_print_stats=True, options=o)
            s2.solveGeometricConjugateGradient(x, bd, tol, 400, True)
            s2.close()
        finally:
            import ctypes

            ctypes.CDLL(None).fflush(None)  # (the library's printf buffer, before the descriptor goes back)
            os.dup2(saved, 1)
            os.close(saved)
        f.seek(0)
        lines = [ln for ln in f.read().splitlines() if "Relative error:" in ln]
    s.close()
    return [float(ln.split("Relative error:")[1]) for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.size
    levels = int(np.log2(n)) - 3  # coarsest level 16^3
    out = {"size": n, "levels": levels, "device": torch.cuda.get_device_name(0)}
    lab, w, dx = D.free_surface_pool(n, levels)
    b = D.random_rhs(lab, dx)
    setup = {0: [], 1: []}
    for _ in range(a.reps):
        for enc in (0, 1):  # interleaved
            s, ms = build(lab, w, levels, enc)
            setup[enc].append(ms)
            s.close()
    pool = {"setup_ms_off": float(np.median(setup[0])), "setup_ms_on": float(np.median(setup[1])), "setup_ms_off_all": setup[0],
            "setup_ms_on_all": setup[1]}
    for enc in (0, 1):
        s, _ = build(lab, w, levels, enc)
        pool[f"pcg_{'on' if enc else 'off'}"] = solve(s, b)
        s.close()
    out["pool"] = pool
    tanks = {}
    for name, open_top, enc in (("open_top", True, 0), ("sealed", False, 1)):
        tl, tw = tank(n, levels, open_top)
        times = []
        for _ in range(a.reps):
            s, ms = build(tl, tw, levels, enc)
            times.append(ms)
            s.close()
        s, _ = build(tl, tw, levels, enc)
        tb = D.random_rhs(tl, 1.0 / n)
        tanks[name] = {"setup_ms": float(np.median(times)), "setup_ms_all": times, "enclosed": s.enclosed_components(), "pcg": solve(s, tb)}
        s.close()
        # every CG vector mode with both smoothers (pcg above: Jacobi, the default mode 2)
        modes = {}
        for gs in (False, True):
            for mode in (0, 1, 2):
                o = G.default_options()
                o.enclosed_liquid, o.pcg_fp64_vectors = enc, mode
                s = G.GeometricMultigridPoissonSolver(tl, tw, levels, gs, options=o)
                modes[f"{'gs' if gs else 'jacobi'}_mode{mode}"] = solve(s, tb)
                s.close()
        tanks[name]["modes"] = modes
        if not open_top:
            tanks[name]["history_jacobi_mode2"] = history(tl, tw, levels, False, 2, tb)
    cells = n ** 3
    # what the labelling reads and writes at least: codes 1 B, three weight grids 12 B, parents 4 B written + read twice, a flag byte
    tanks["labelling_min_bytes"] = cells * (1 + 12 + 4 * 3 + 1)
    tanks["labelling_ms_estimate"] = tanks["sealed"]["setup_ms"] - tanks["open_top"]["setup_ms"]
    out["tank"] = tanks
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
