#!/usr/bin/env python3
"""Times the two passes of the deforming mesh colliders beside the passes they sit next to, on the same build.
Mesh stage: section 19's unit icosphere of 20 480 triangles onto 128^3 samples (band = 3 spacings), mgps_fields_mesh_sdf_velocity
against mgps_fields_mesh_sdf, the whole call each (host checks, binning and upload included).  Face stage: an N^3 grid with 8 box
meshes about N / 12 cells across, rasterised once; mgps_fields_sampled_velocity against mgps_fields_rigid_velocity on the same face
grids.  HIP events on torch's stream; three warm-up calls each, then `rounds` rounds in which the two calls alternate; the median
of each with min and max, and the median of the per-round ratios.  No threshold.  Prints one JSON line.
   tools/mesh_velocity_bench.py [N=480] [rounds=7]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mesh_reference as MR  # noqa: E402
import raster_reference as RR  # noqa: E402

from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 480
rounds = int(args[1]) if len(args) > 1 else 7


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(new, old):
    """(new, old, ratio): medians of `rounds` alternating calls, with the spread"""
    for _ in range(3):
        new()
        old()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(once(new))
        b.append(once(old))
    stat = lambda ms: {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}  # noqa: E731
    return stat(a), stat(b), round(statistics.median([p / q for p, q in zip(a, b)]), 3)


out = {"rounds": rounds, "device": torch.cuda.get_device_name(0)}

# ---- the mesh stage ----
v, t = MR.icosphere(1.0, 5)
m = 128
spacing = 2.0 / (m - 9)
nn, origin, band = (m, m, m), -(1.0 + 4 * spacing) * np.ones(3), 3 * spacing
V = np.random.default_rng(1).uniform(-1.0, 1.0, v.shape)
new, old, ratio = interleaved(lambda: F.meshSDFVelocity(v, t, V, nn, origin, spacing, band), lambda: F.meshSDF(v, t, nn, origin, spacing, band))
sdf, vel = F.meshSDFVelocity(v, t, V, nn, origin, spacing, band)
out["mesh_stage"] = {"scene": f"{len(t)} triangles, {m}^3 samples", "mesh_sdf_velocity_ms": new, "mesh_sdf_ms": old, "ratio": ratio,
                     "within_band": int((sdf.abs() < band).sum().item()), "same_sdf_bits": bool(torch.equal(sdf, F.meshSDF(v, t, nn, origin, spacing, band)))}
del sdf, vel

# ---- the face stage ----
shape = (n, n, n)
rng = np.random.default_rng(8)
shapes = []
for r in range(8):
    c = (0.2 + 0.6 * rng.random(3)) * n
    half = n / 24 * (1 + rng.random(3))
    mesh = MR.box(-half, half)
    h = max(0.5, float(half.max()) / 40)  # (sample spacing: about 100 samples along the longest side)
    shapes.append(F.BodyShape.mesh(c, *mesh, h, 3.0 + np.sqrt(3.0) * h, RR.rotation(rng.standard_normal(3), rng.random() * 3),
                                   vertex_velocities=rng.uniform(-1.0, 1.0, mesh[0].shape)))
solid, cw, body = F.rasterizeBodies(shape, shapes, 3.0, 0.05)
del solid, cw
sv = [torch.zeros_like(b, dtype=torch.float32) for b in body]
centres, motions = np.zeros((9, 3)), np.zeros((9, 6))
for r, s in enumerate(shapes, start=1):
    centres[r] = s.centre[:]
    motions[r] = 0.1 * rng.standard_normal(6)
new, old, ratio = interleaved(lambda: F.sampledVelocity(sv, body, shapes, motions[1:]), lambda: F.rigidVelocity(sv, body, centres, motions))
cells = float(n) ** 3
out["face_stage"] = {"grid": n, "bodies": 8, "owned_faces": int(sum((b > 0).sum().item() for b in body)), "sampled_velocity_ms": new,
                     "rigid_velocity_ms": old, "ratio": ratio, "ids_GBps": round(12.0 * cells / new["median"] / 1e6, 1)}
print(json.dumps(out))
