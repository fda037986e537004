#!/usr/bin/env python3
"""Times the rigid-body rasterisation (mgps_fields_rasterize_bodies) on an N^3 grid with static walls, for
8 bodies (spheres, rotated boxes and one sampled SDF, about N / 12 cells across) and for 255 small spheres on a jittered lattice:
HIP events on torch's stream, warm-up, then the median of `reps` calls.  Also times an empty scene (one body outside the grid: every
tile streams) for the pass's rate on its empty-tile traffic, 16 B read and 28 B written per cell, and the path the pass replaces:
the upload of the seven grids from pageable host memory, and -- with --host, which takes minutes and gigabytes beyond 128^3 -- the
numpy restatement of tests/raster_reference.py that would produce them.  Prints one JSON line.
   tools/raster_time.py [N=256] [reps=30] [--host]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import raster_reference as RR  # noqa: E402
from test_raster_bodies import device_shapes  # noqa: E402  (restatement shapes -> BodyShape, GRID samples uploaded)

from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 256
reps = int(args[1]) if len(args) > 1 else 30
host = "--host" in sys.argv
shape = (n, n, n)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def scene(bodies):
    rng = np.random.default_rng(bodies)
    if bodies == 0:
        return [RR.sphere((-100.0, -100.0, -100.0), 1.0)]
    if bodies == 8:
        out = []
        for r in range(8):
            c = (0.2 + 0.6 * rng.random(3)) * n
            size = n / 24 * (1 + rng.random(3))
            rot = RR.rotation(rng.standard_normal(3), rng.random() * 3)
            if r == 7:
                m, h = 24, size.max() * 2.4 / 23
                origin = -0.5 * 23 * h * np.ones(3)
                k, j, i = np.meshgrid(*(origin[0] + h * np.arange(m),) * 3, indexing="ij")
                out.append(RR.sdf_grid(c, RR.box_sdf([i, j, k], size).astype(np.float32), origin, h, rot))
            else:
                out.append(RR.sphere(c, size[0]) if r % 2 else RR.box(c, size, rot))
        return out
    side = 7  # 7^3 = 343 lattice sites, the first 255 taken
    sites = [(i, j, k) for k in range(side) for j in range(side) for i in range(side)][:bodies]
    return [RR.sphere((np.array(s) + 0.5 + 0.3 * (rng.random(3) - 0.5)) * n / side, n / 40 * (1 + 0.5 * rng.random())) for s in sites]


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
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


static_phi = np.full(shape, 5.0, dtype=np.float32)
static_cw = []
for a in range(3):
    s = list(shape)
    s[2 - a] += 1
    w = np.ones(s, dtype=np.float32)
    sl = [slice(None)] * 3
    for end in (0, n):
        sl[2 - a] = end
        w[tuple(sl)] = 0.0
    static_cw.append(w)
sphi, scw = dev(static_phi), [dev(w) for w in static_cw]
cells = float(n) ** 3
out = {"grid": n, "reps": reps, "device": torch.cuda.get_device_name(0), "raster_ms": {}}
for bodies in (0, 8, 255):
    shapes = device_shapes(scene(bodies))
    t = timed(lambda: F.rasterizeBodies(shape, shapes, 3.0, 0.05, sphi, scw))
    solid, cw, body = F.rasterizeBodies(shape, shapes, 3.0, 0.05, sphi, scw)
    t["owned_faces"] = int(sum((b > 0).sum().item() for b in body))
    t["model_GBps"] = round(44.0 * cells / t["median"] / 1e6, 1)  # (the empty-tile traffic; the whole story for bodies = 0 only)
    out["raster_ms"]["empty" if bodies == 0 else str(bodies)] = t
    del solid, cw, body

# the path the pass replaces: seven grids from the host ...
grids = [static_phi] + static_cw + [np.zeros_like(w, dtype=np.int32) for w in static_cw]
wall = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = [dev(g) for g in grids]
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
    del keep
out["upload_seven_grids_ms"] = {"median": round(statistics.median(wall), 2), "min": round(min(wall), 2), "bytes": int(sum(g.nbytes for g in grids))}
# ... that numpy made
if host:
    t0 = time.perf_counter()
    RR.rasterize(shape, scene(8), 3.0, 0.05, static_phi, static_cw)
    out["numpy_restatement_8_bodies_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
print(json.dumps(out))
