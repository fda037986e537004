#!/usr/bin/env python3
"""Times mgps_fields_solid_forces against mgps_fields_divergence on the same arrays: projection_scene at N^3 (default 480^3) with its
box as body 1, both passes in interleaved repeats with HIP events on torch's stream.  Both calls synchronise the stream and bring
their result to the host, so a repeat is one call between two events.  Prints one JSON line: medians, spreads (max - min) and the
algorithmic GB/s of both (the divergence streams three velocity grids, three weight grids and the labels; the forces pass streams
the three weight grids and, next to closed faces, ids, labels and pressure).

    python tools/solid_forces_bench.py [N] [--repeats 15] [--bodies B] [--out profiles/NAME.json]

--bodies B cuts the box into B pieces by z plane (255: the largest tables, 64 KiB of LDS per workgroup and 16 MiB of partial
tables); --bodies -B scatters B ids face by face, the worst case of the per-wave row loop."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_ids(sc, shape, bodies):
    """the faces of the cells inside the scene's solid box belong to a body, the others (the domain walls) to row 0.  With more than
    one body the box is cut into `bodies` pieces: layers of z planes (a wave, which runs along x, meets one row per axis), or with
    `bodies` < 0 ids scattered face by face over -bodies pieces (a wave meets up to 64 rows per axis: the worst case of the row loop)"""
    inside = sc["solid_phi"] >= 0
    ids = []
    for a in range(3):
        ax = 2 - a
        pad = [(0, 0)] * 3
        pad[ax] = (1, 0)
        behind = np.pad(inside, pad)
        pad[ax] = (0, 1)
        owned = behind | np.pad(inside, pad)
        k, j, i = np.meshgrid(*[np.arange(n) for n in owned.shape], indexing="ij", sparse=True)
        piece = k % bodies if bodies > 0 else (i * 7 + j * 13 + k * 29) % -bodies
        ids.append(np.where(owned, 1 + piece, 0).astype(np.int32))
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=480)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--bodies", type=int, default=1, help="pieces the box is cut into; negative: ids scattered face by face")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd import fields as F

    n = a.size
    shape = (n, n, n)
    sc = D.projection_scene(shape, with_solid_velocity=True)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    cw, vel, sv = [dev(x) for x in sc["cut_weights"]], [dev(x) for x in sc["velocity"]], [dev(x) for x in sc["solid_velocity"]]
    body = [dev(x) for x in box_ids(sc, shape, a.bodies)]
    a.scattered, a.bodies = a.bodies < 0, abs(a.bodies)
    material = F.buildMaterialCellLabels(dev(sc["liquid_phi"]), dev(sc["solid_phi"]), cw)
    pressure = torch.rand(shape, device="cuda")
    centres = np.zeros((a.bodies + 1, 3))
    centres[1:] = [0.31 * n, 0.49 * n, 0.31 * n]  # (the box's centre for every piece)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    forces = lambda: F.solidForces(pressure, material, cw, body, centres, 1.0)  # noqa: E731
    divergence = lambda: F.computeResultingDivergence(material, vel, cw, sv)  # noqa: E731
    rows = forces()
    divergence()
    t = {"solid_forces": [], "divergence": []}
    for _ in range(a.repeats):  # interleaved: a drift of the clocks meets both alike
        t["solid_forces"].append(timed(forces)[0])
        t["divergence"].append(timed(divergence)[0])
    cells = float(n) ** 3
    nbytes = {"solid_forces": 12 * cells, "divergence": (4 + 12 + 12 + 12) * cells}
    out = {"base_grid": n, "bodies": a.bodies, "ids_scattered": a.scattered, "repeats": a.repeats,
           "wet_faces_unowned": int(rows[0, 7]), "wet_faces_owned": int(rows[1:, 7].sum()), "force_on_the_box": [float(v) for v in rows[1:, :3].sum(0)]}
    for name, ms in t.items():
        med = float(np.median(ms))
        out[name] = {"median_ms": round(med, 4), "spread_ms": round(max(ms) - min(ms), 4), "min_ms": round(min(ms), 4),
                     "algorithmic_GBps": round(nbytes[name] / med / 1e6, 1)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
