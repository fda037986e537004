#!/usr/bin/env python3
"""Times the redistancing pass (mgps_fields_redistance) beside the advection it follows, on the same build
and the same grids: the projection_scene of an N^3 base grid (default 480^3), liquid_phi with dx = 1 / N, band 8.  The rounds to
the fixpoint are taken from counts[1], round by round through the window entries on [0, gz): R* rounds change a cell, round R* + 1
changes none.  Timed: the single call with rounds = R* + 1 (the initial launch, the rounds, no synchronisation) for inner = 1 and
inner = 4, the convenience form (rounds = None, inner = 4: batches with one synchronisation each), and advect (MacCormack and
semi-Lagrangian, max |dt u| = 2 cells, the velocity and liquid_phi).  HIP events on torch's stream; three warm-up calls each, then
`rounds` rounds in which the calls alternate; the median of each with min and max.  No threshold.  Beside the time: the bytes a
round must move (the grid read once and written once) and the achieved fraction of the HBM rate (8 TB/s).  Prints one JSON line.
   tools/redistance_bench.py [N=480] [rounds=7] [band=8.0]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402
from geometricmultigridpressuresolver_amd.solver import expanded_layout  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 480
rounds = int(args[1]) if len(args) > 1 else 7
band = float(args[2]) if len(args) > 2 else 8.0
HBM_GBPS = 8000.0

shape = (n, n, n)
sc = D.projection_scene(shape)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
phi = dev(sc["liquid_phi"])
vel = [dev(a) for a in sc["velocity"]]
dx = 1.0 / n
dt = 2.0 / max(float(v.abs().max()) for v in vel)
out, scratch = torch.empty_like(phi), torch.empty_like(phi)
adv_out = ([torch.empty_like(v) for v in vel], [torch.empty_like(phi)])
adv_scratch = ([torch.empty_like(v) for v in vel], [torch.empty_like(phi)])
grid_bytes = 4.0 * phi.numel()


def rounds_to_fixpoint(inner):
    """(R*, interface cells, the cells each round changed)"""
    w = F.slab_window(shape, True, [0, expanded_layout(shape)[0][0]], 0)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    a, b = F.redistanceInitSlab(w, phi, band, 0, counts=counts), scratch
    moved = []
    while True:
        counts[1] = 0
        a, b = F.redistanceRoundSlab(w, a, band, 0, inner=inner, last=True, out=b, counts=counts), a
        moved.append(int(counts[1]))
        if moved[-1] == 0:
            return len(moved) - 1, int(counts[0]), moved


fix = {inner: rounds_to_fixpoint(inner) for inner in (1, 4)}
calls = {
    "redistance_inner1": lambda: F.redistance(phi, band, dx, fix[1][0] + 1, 1, out=out, scratch=scratch),
    "redistance_inner4": lambda: F.redistance(phi, band, dx, fix[4][0] + 1, 4, out=out, scratch=scratch),
    "redistance_to_fixpoint_inner4": lambda: F.redistance(phi, band, dx, None, 4, out=out, scratch=scratch),
    "advect_maccormack": lambda: F.advect(vel, dt, [phi], "maccormack", 2, out=adv_out, scratch=adv_scratch),
    "advect_semi_lagrangian": lambda: F.advect(vel, dt, [phi], "semi_lagrangian", 2, out=adv_out),
}
launches = {"redistance_inner1": fix[1][0] + 2, "redistance_inner4": fix[4][0] + 2}  # the initial launch and R* + 1 rounds


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
res = {"grid": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "band": band, "grid_bytes": int(grid_bytes),
       "interface_cells": fix[1][1], "cells_within_band": int((out.abs() < np.float32(band) * np.float32(dx)).sum()),
       "rounds_to_fixpoint": {"inner1": fix[1][0], "inner4": fix[4][0]}, "cells_changed_per_round": {"inner1": fix[1][2], "inner4": fix[4][2]}}
for name, t in ms.items():
    row = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    if name in launches:
        row["launches"] = launches[name]
        row["ms_per_launch"] = round(row["median"] / launches[name], 4)
        row["bytes_moved"] = int(2 * launches[name] * grid_bytes)
        row["GBps"] = round(row["bytes_moved"] / row["median"] / 1e6, 1)
        row["fraction_of_hbm"] = round(row["GBps"] / HBM_GBPS, 4)
    res[name + "_ms"] = row
print(json.dumps(res))
