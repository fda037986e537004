#!/usr/bin/env python3
"""Times the mesh signed distance (mgps_fields_mesh_sdf): a unit icosphere of 20 480 and of 327 680 triangles
onto N^3 samples, N = 64 and 128, at band = 3 spacings, the sample box holding the sphere grown by band + spacing.  HIP events on
torch's stream around the whole call -- the host's mesh checks, binning and upload included, since the call makes them every time --
three warm-up calls, then the median of `reps` calls with min and max; beside it host_checks_ms, the wall time of
mgps_mesh_mass_properties, which makes the same mesh checks.  With --host the numpy restatement of tests/mesh_reference.py on one
thread at the smallest case (half an hour; it needs no GPU: --host-only skips the device part).  Prints one JSON line.
   tools/mesh_sdf_time.py [reps=30] [--host | --host-only]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mesh_reference as MR  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if len(args) > 0 else 30
host, host_only = "--host" in sys.argv or "--host-only" in sys.argv, "--host-only" in sys.argv


def samples(n):
    """(n, origin, spacing, band) of n^3 samples around the unit sphere"""
    spacing = 2.0 / (n - 9)
    return (n, n, n), -(1.0 + 4 * spacing) * np.ones(3), spacing, 3 * spacing


out = {"reps": reps, "mesh_sdf_ms": {}}
if not host_only:
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    out["device"] = torch.cuda.get_device_name(0)

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

    for level in (5, 7):
        v, t = MR.icosphere(1.0, level)
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            F.meshMassProperties(v, t)
            wall.append((time.perf_counter() - t0) * 1e3)
        for n in (64, 128):
            nn, origin, spacing, band = samples(n)
            r = timed(lambda: F.meshSDF(v, t, nn, origin, spacing, band))
            sdf = F.meshSDF(v, t, nn, origin, spacing, band)
            r["inside"], r["within_band"] = int((sdf < 0).sum().item()), int((sdf.abs() < band).sum().item())
            r["host_checks_ms"] = round(statistics.median(wall), 3)
            out["mesh_sdf_ms"][f"{len(t)} triangles, {n}^3"] = r
if host:
    v, t = MR.icosphere(1.0, 5)
    nn, origin, spacing, band = samples(64)
    t0 = time.perf_counter()
    MR.mesh_sdf(v, t, nn, origin, spacing, band)
    out["numpy_restatement_20480_triangles_64^3_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
print(json.dumps(out))
