#!/usr/bin/env python3
"""Times the FLIP particle passes (mgps_particles_bin / _to_grid in both of its forms / _update) beside the
semi-Lagrangian advection pass on the same grid and in the same run: the projection_scene of an N^3 base grid (default 256^3: seeding its liquid takes a few
seconds on the host), seedParticles at 8 per cell of the liquid, particle velocities sampled from the scene's velocity, dt chosen so
that max |dt u| = `reach` cells (default 2), trace_order 2, flip 0.95.  The particles are moved by one update first, so that bin sorts a
set that is nearly, not exactly, in cell order -- what a sub-step hands it.  HIP events on torch's stream around the Python calls;
three warm-up calls each, then `rounds` rounds in which the calls alternate; the median of each with min and max.  No threshold.
Beside each time: the bytes the pass must move (every input read once, every output written once) and the rate that makes, with its
fraction of the HBM rate (8 TB/s).  Prints one JSON line and writes it to --out (default profiles/particles_bench_mi355x.json).
Next to solids, in the same rounds: a rasterised sphere in the pool, sized so that about 5 % of the moved particles
lie within `margin` of it or inside; collideParticles on the moved set, updateParticlesSolid, updateParticles followed by
collideParticles (the pair the fused call replaces, timed as one), and resampleParticles (min 4, max 12) of the binned set.
--parent-lib=PATH: another build of libmgps.so (the parent commit's) whose mgps_particles_update is called with the same desc in the
same rounds, as `update_parent`.
   tools/particles_bench.py [N=256] [rounds=7] [reach=2.0] [--out=PATH] [--parent-lib=PATH]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
n = int(args[0]) if len(args) > 0 else 256
rounds = int(args[1]) if len(args) > 1 else 7
reach = float(args[2]) if len(args) > 2 else 2.0
out_path = flags.get("out", os.path.join(ROOT, "profiles", "particles_bench_mi355x.json"))
HBM_GBPS = 8000.0
RADIUS, FLIP = 1.0, 0.95

shape = (n, n, n)
sc = D.projection_scene(shape)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
phi = dev(sc["liquid_phi"])
grid = [dev(a) for a in sc["velocity"]]
dt = reach / max(float(v.abs().max()) for v in grid)
t0 = time.time()
seeded = F.seedParticles(phi, per_cell=8, seed=0)
torch.cuda.synchronize()
seed_s = time.time() - t0
count = seeded[0].numel()
zero = [torch.zeros_like(q) for q in seeded]
_, sampled = F.updateParticles(seeded, zero, grid, 0.0, None, 0.0, 2)  # PIC with dt = 0: the scene's velocity at the particles
pos, vel = F.updateParticles(seeded, sampled, grid, dt, grid, FLIP, 2)  # one step: nearly in cell order
del seeded, zero, sampled

cells = n * n * n
faces = sum(v.numel() for v in grid)
new = lambda like: [torch.empty_like(t) for t in like]  # noqa: E731
bin_out = (new(pos), new(vel), torch.empty(count, dtype=torch.int32, device="cuda"), torch.empty(cells + 2, dtype=torch.int32, device="cuda"))
bpos, bvel, order, cell_start, bin_counts = F.binParticles(pos, vel, shape, out=bin_out)
grid_out = (new(grid), new(grid), [torch.empty(v.shape, dtype=torch.uint8, device="cuda") for v in grid], torch.empty_like(phi))
p2g, _, known, _, grid_counts = F.particlesToGrid(bpos, bvel, cell_start, shape, RADIUS, out=grid_out)
moved = (new(pos), new(vel))
adv_out = (new(grid), [torch.empty_like(phi)])
tally = torch.zeros(2, dtype=torch.int64, device="cuda")
F.updateParticles(bpos, bvel, grid, dt, p2g, FLIP, 2, out=moved, counts=tally)

# the solid: a sphere in the pool whose radius is the 5 % quantile of the moved particles' distance from its centre, less the margin
MARGIN, ITERATIONS, LEAST, MOST = 0.1, 2, 4, 12
centre = (0.5 * n, 0.5 * n, 0.3 * n)
pick = torch.randint(0, count, (1000000,), device="cuda")
dist = torch.sqrt(sum((moved[0][a][pick].double() - centre[a]) ** 2 for a in range(3)))
radius = float(dist.kthvalue(50000).values) - MARGIN
solid_phi, _, _ = F.rasterizeBodies(shape, [F.BodyShape.sphere(centre, radius)], 3.0, 0.0)
hits, both = torch.zeros(3, dtype=torch.int64, device="cuda"), (new(pos), new(vel))
F.collideParticles(moved[0], moved[1], solid_phi, None, MARGIN, ITERATIONS, 0.0, out=both, counts=hits)
fused = (new(pos), new(vel))
capacity = count + count // 4
re_out = ([torch.empty(capacity, device="cuda") for _ in range(3)], [torch.empty(capacity, device="cuda") for _ in range(3)],
          torch.empty(cells + 2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
resample = lambda: F.resampleParticles(bpos, bvel, cell_start, shape, capacity, LEAST, MOST, phi, 1.0 / n, 1.0, solid_phi, grid, 0, False, out=re_out)  # noqa: E731
_, _, _, n_out, re_counts = resample()


def pair():
    F.updateParticles(bpos, bvel, grid, dt, p2g, FLIP, 2, out=moved)
    F.collideParticles(moved[0], moved[1], solid_phi, None, MARGIN, ITERATIONS, 0.0, out=both)


calls = {
    "bin": lambda: F.binParticles(pos, vel, shape, out=bin_out),
    "to_grid_gather": lambda: F.particlesToGrid(bpos, bvel, cell_start, shape, RADIUS, out=grid_out, form="gather"),
    "to_grid_staged": lambda: F.particlesToGrid(bpos, bvel, cell_start, shape, RADIUS, out=grid_out, form="staged"),
    "update": lambda: F.updateParticles(bpos, bvel, grid, dt, p2g, FLIP, 2, out=moved),
    "advect_semi_lagrangian": lambda: F.advect(grid, dt, [phi], "semi_lagrangian", 2, out=adv_out),
    "collide": lambda: F.collideParticles(moved[0], moved[1], solid_phi, None, MARGIN, ITERATIONS, 0.0, out=both),
    "update_solid": lambda: F.updateParticlesSolid(bpos, bvel, grid, dt, solid_phi, p2g, FLIP, 2, None, MARGIN, ITERATIONS, 0.0, out=fused),
    "update_then_collide": pair,
    "resample": resample,
}
if "parent-lib" in flags:  # the same desc through another build's entry
    parent = C.CDLL(flags["parent-lib"])
    parent.mgps_particles_update.argtypes, parent.mgps_particles_update.restype = [C.c_void_p, C.c_void_p], C.c_int
    parent_out = (new(pos), new(vel))
    parent_desc = F._update_desc(bpos, bvel, grid, dt, p2g, FLIP, 2, parent_out, None)[0]

    def update_parent():
        assert parent.mgps_particles_update(C.byref(parent_desc), F._stream()) == 0

    calls = dict(list(calls.items())[:4] + [("update_parent", update_parent)] + list(calls.items())[4:])  # (next to `update` in a round)
must_move = {  # every input read once, every output written once
    "bin": 4 * (6 * count + 6 * count + count + cells + 2),
    "to_grid_gather": 4 * (6 * count + cells + 2) + (4 + 4 + 1) * faces + 4 * cells,
    "update": 4 * (6 * count + 6 * count + 2 * faces),
    "advect_semi_lagrangian": 2 * 4 * (faces + cells),
}
must_move["to_grid_staged"] = must_move["to_grid_gather"]
must_move["update_parent"] = must_move["update"]
must_move["collide"] = 4 * (6 * count + 6 * count + cells)
must_move["update_solid"] = must_move["update"] + 4 * cells
must_move["update_then_collide"] = must_move["update"] + must_move["collide"]
must_move["resample"] = 4 * (6 * count + 6 * int(n_out) + 2 * (cells + 2) + 2 * cells + faces)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for _ in range(3):
    for fn in calls.values():
        fn()
torch.cuda.synchronize()
ms = {name: [] for name in calls}
for _ in range(rounds):
    for name, fn in calls.items():
        ms[name].append(once(fn))
out = {"grid": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "particles": count, "per_cell": 8, "seeding_s": round(seed_s, 2),
       "liquid_cells": int((phi < 0).sum()), "max_dt_u": reach, "trace_order": 2, "flip": FLIP, "radius": RADIUS,
       "outside": int(bin_counts[0]), "occupied_cells": int(bin_counts[1]), "known_faces": int(grid_counts[0]), "cells_phi_le_0": int(grid_counts[1]),
       "clamped_particles": int(tally[0]), "solid_radius": round(radius, 3), "margin": MARGIN, "iterations": ITERATIONS,
       "pushed_particles": int(hits[0]), "pushed_still_inside": int(hits[1]), "stuck_particles": int(hits[2]), "resample_min_max": [LEAST, MOST],
       "resample_n_out": int(n_out), "resample_thinned": int(re_counts[0]), "resample_seeded": int(re_counts[1]), "resample_deep_cells": int(re_counts[2]),
       "fused_equals_pair": all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(fused[0] + fused[1], both[0] + both[1]))}
for name, t in ms.items():
    row = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4), "bytes_moved": int(must_move[name])}
    row["GBps"] = round(must_move[name] / row["median"] / 1e6, 1)
    row["fraction_of_hbm"] = round(row["GBps"] / HBM_GBPS, 4)
    out[name + "_ms"] = row
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
