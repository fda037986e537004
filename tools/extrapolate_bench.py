#!/usr/bin/env python3
"""Times the velocity extrapolation (mgps_fields_extrapolate3) on the projection_scene of an N^3 base grid
(default 480^3) for L = 4 and 8 layers, and the three mgps_fields_pressure_gradient passes on the same grid, with HIP events on
torch's stream: warm-up, then the median of `reps` calls.  Prints one JSON line: ms per call, ms per layer (the slope between
L = 4 and L = 8, and the call's share that is not layers: the pass that writes `layer` from `valid`), bytes per face and layer by
the sweep's model -- 1 B of `layer` per face, plus for every face filled its 6 neighbour bytes, the known neighbours' velocities
and its own three stores, plus the cut weight -- and the ratio of one layer to the gradient passes."""
import json
import statistics
import sys

import numpy as np
import torch

from geometricmultigridpressuresolver_amd import domains as D
from geometricmultigridpressuresolver_amd import fields as F

n = int(sys.argv[1]) if len(sys.argv) > 1 else 480
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
shape = (n, n, n)
sc = D.projection_scene(shape)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
cw = [dev(a) for a in sc["cut_weights"]]
phi = dev(sc["liquid_phi"])
vel = [dev(a) for a in sc["velocity"]]
material = F.buildMaterialCellLabels(phi, dev(sc["solid_phi"]), cw)
valid = F.buildValidFaces(material, cw)
pressure = torch.rand(shape, device="cuda")
faces = float(sum(v.numel() for v in vel))


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


out = {"base_grid": n, "faces": int(faces), "reps": reps, "extrapolate3": {}}
grad = timed(lambda: F.applyPressureGradient(vel, phi, pressure, valid, material))
out["pressure_gradient_x3_ms"] = {"median": round(grad[0], 4), "min": round(grad[1], 4), "max": round(grad[2], 4)}
for name, weights in (("cut_weights", cw), ("no_cut_weights", None)):
    t, filled = {}, {}
    for layers in (4, 8):
        t[layers] = timed(lambda: F.extrapolateVelocity(vel, valid, layers, weights))
        filled[layers] = sum(F.extrapolateVelocity(vel, valid, layers, weights)[1])
    per_layer = (t[8][0] - t[4][0]) / 4
    shell = (filled[8] - filled[4]) / 4  # faces filled per layer, layers 5 .. 8
    model = 1.0 + shell * (6 + 4 * 3 + 4 + 1 + (4 if weights is not None else 0)) / faces
    out["extrapolate3"][name] = {
        "L4_ms": {"median": round(t[4][0], 4), "min": round(t[4][1], 4), "max": round(t[4][2], 4)},
        "L8_ms": {"median": round(t[8][0], 4), "min": round(t[8][1], 4), "max": round(t[8][2], 4)},
        "filled_L4": filled[4], "filled_L8": filled[8],
        "ms_per_layer": round(per_layer, 4), "init_pass_ms": round(t[4][0] - 4 * per_layer, 4),
        "model_bytes_per_face_per_layer": round(model, 3), "model_GBps": round(model * faces / per_layer / 1e6, 1),
        "layer_over_gradient_x3": round(per_layer / grad[0], 3),
    }
print(json.dumps(out))
