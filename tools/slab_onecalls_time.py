#!/usr/bin/env python3
"""total_ms of the two light slab one-calls, mgps_extrapolate_velocity_slab (6 layers, cut weights) and mgps_solid_forces_slab (3
bodies), on the projection_scene of an N^3 base grid, the ranks sharing one GPU over TorchDistComm/gloo (host staging: this says
nothing about RCCL between GPUs).  Per call the slowest rank's total_ms; two warm-up calls, then the median of `reps`.  Rank 0 prints
one "RESULT {json}" line.  Another build of the library is chosen with MGPS_LIBRARY.

    python -m torch.distributed.run --nproc-per-node=2 tools/slab_onecalls_time.py [N] [reps]"""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402
from geometricmultigridpressuresolver_amd.distributed import TorchDistComm  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dist.init_process_group("gloo")
torch.cuda.set_device(0)
comm = TorchDistComm()
shape = (n, n, n)
splits = F.projection_slab_layout(shape, True, comm.size, False)["splits"]
d = F.slab_window(shape, True, splits, comm.rank)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
sc = D.projection_scene(shape)
cw, vel = [dev(a) for a in sc["cut_weights"]], [dev(a) for a in sc["velocity"]]
mat = F.buildMaterialCellLabels(dev(sc["liquid_phi"]), dev(sc["solid_phi"]), cw)
valid = F.buildValidFaces(mat, cw)
win = lambda g: [g[0][d.c0:d.c1].contiguous(), g[1][d.c0:d.c1].contiguous(), g[2][d.c0:d.c1 + 1].contiguous()]  # noqa: E731
w_cw, w_valid = win(cw), win(valid)
rng = np.random.default_rng(31)
body = win([dev(rng.integers(-1, 5, size=tuple(v.shape)).astype(np.int32)) for v in vel])
centres = rng.random((4, 3)) * n
pressure = torch.rand(d.base_shape, dtype=torch.float32, device="cuda")
phi, sphi = dev(sc["liquid_phi"][d.c0:d.c1]), dev(sc["solid_phi"][d.c0:d.c1])
ex, fo = [], []
for i in range(reps + 2):
    w_vel = [t.clone() for t in win(vel)]
    torch.cuda.synchronize()
    dist.barrier()
    ex.append(F.extrapolate_velocity_slab(comm, splits, shape, w_vel, w_valid, 6, cut_weights=w_cw)["total_ms"])
    torch.cuda.synchronize()
    dist.barrier()
    fo.append(F.solid_forces_slab(comm, splits, shape, pressure, phi, sphi, w_cw, body, centres, 0.37)["total_ms"])
seen = [None] * comm.size
dist.all_gather_object(seen, (ex[2:], fo[2:]))
if comm.rank == 0:
    exm = np.max([s[0] for s in seen], axis=0)
    fom = np.max([s[1] for s in seen], axis=0)
    print("RESULT " + json.dumps({"extrapolate_slab_total_ms": round(float(np.median(exm)), 4), "solid_forces_slab_total_ms": round(float(np.median(fom)), 4)}), flush=True)
dist.barrier()
dist.destroy_process_group()
