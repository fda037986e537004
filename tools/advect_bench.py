#!/usr/bin/env python3
"""Times the advection pass (mgps_fields_advect) beside the velocity extrapolation it follows, on the same
build and the same grids: the projection_scene of an N^3 base grid (default 480^3), the three face grids of the velocity plus
liquid_phi, dt chosen so that max |dt u| = `reach` cells (default 2), trace_order 2.  advect under both schemes and
extrapolateVelocity (8 layers, with cut weights) on the scene's valid faces.  HIP events on torch's stream; three warm-up calls each,
then `rounds` rounds in which the three calls alternate; the median of each with min and max.  No threshold.  The one figure the pass
can be judged against is the bytes it must move -- (4 + scalars) grids read once and written once; MacCormack's second launch reads
the inputs and the scratch and writes again, 5 grid passes in all against 2 --: the achieved fraction of the HBM rate (8 TB/s) for
those bytes is printed beside the time.  Prints one JSON line.
   tools/advect_bench.py [N=480] [rounds=7] [reach=2.0]"""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 480
rounds = int(args[1]) if len(args) > 1 else 7
reach = float(args[2]) if len(args) > 2 else 2.0
HBM_GBPS = 8000.0

shape = (n, n, n)
sc = D.projection_scene(shape)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
cw = [dev(a) for a in sc["cut_weights"]]
phi = dev(sc["liquid_phi"])
vel = [dev(a) for a in sc["velocity"]]
material = F.buildMaterialCellLabels(phi, dev(sc["solid_phi"]), cw)
valid = F.buildValidFaces(material, cw)
del material
dt = reach / max(float(v.abs().max()) for v in vel)
out_grids = ([torch.empty_like(v) for v in vel], [torch.empty_like(phi)])
scratch = ([torch.empty_like(v) for v in vel], [torch.empty_like(phi)])
counts = torch.zeros(2, dtype=torch.int64, device="cuda")
grid_bytes = 4.0 * (sum(v.numel() for v in vel) + phi.numel())

calls = {
    "advect_maccormack": lambda: F.advect(vel, dt, [phi], "maccormack", 2, out=out_grids, scratch=scratch),
    "advect_semi_lagrangian": lambda: F.advect(vel, dt, [phi], "semi_lagrangian", 2, out=out_grids),
    "extrapolate_velocity_8": lambda: F.extrapolateVelocity(vel, valid, 8, cw),
}
passes = {"advect_maccormack": 5, "advect_semi_lagrangian": 2}  # grid sets read or written once


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
F.advect(vel, dt, [phi], "semi_lagrangian", 2, out=out_grids, counts=counts)
out = {"grid": n, "rounds": rounds, "device": torch.cuda.get_device_name(0), "max_dt_u": reach, "trace_order": 2, "scalars": 1,
       "grid_bytes": int(grid_bytes), "clamped_targets": int(counts[0])}
for name, t in ms.items():
    row = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    if name in passes:
        row["bytes_moved"] = int(passes[name] * grid_bytes)
        row["GBps"] = round(passes[name] * grid_bytes / row["median"] / 1e6, 1)
        row["fraction_of_hbm"] = round(row["GBps"] / HBM_GBPS, 4)
    out[name + "_ms"] = row
print(json.dumps(out))
