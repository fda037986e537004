"""options.enclosed_liquid on slab solvers: what the cross-rank labelling and the summed projection cost.

    python tools/enclosed_slab_time.py [--size 512] [--small 256] [--out profiles/r07_enclosed_slab.json]

Part 1 (--size): the P = 1 slab solver over RCCL (the transport `bench.py --force-slab` uses) against the single-device solver,
on the sealed tank (option on) and the free-surface pool (BASELINE config 3, m = 0; option off and on): set-up ms (wall time of
the constructor, synchronised), MG-PCG iterations and ms per iteration (Jacobi, pcg_fp64_vectors 2, tolerance 1e-6).  Part 2
(--small): 2 and 4 ranks sharing the one GPU over gloo (host staged: it says nothing about RCCL), the labelling and merge stage
lines of MGPS_SETUP_TIMING per rank on the sealed tank.  One GPU cannot show what the all-reduce of every projection costs
between GPUs.  The script starts its rank processes itself (torch.distributed.run children)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def tank(n, levels):
    from geometricmultigridpressuresolver_amd import domains as D

    s = 2 ** (levels - 1)
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[s:n - s, s:n - s, s:n - s] = D.INTERIOR
    w = [np.ones(D.face_shape(n, n, n, a), dtype=np.float32) for a in range(3)]
    D.set_boundary_labels(lab, w)
    return lab, w


def part1(n):
    """one rank: RCCL slab and single device, interleaved per case"""
    import torch
    import torch.distributed as dist

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import RcclComm, SlabSolver

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    comm = RcclComm(device=0)
    levels = int(np.log2(n)) - 3
    out = {"size": n, "levels": levels, "device": torch.cuda.get_device_name(0), "transport": "rccl, P = 1"}
    pool = D.free_surface_pool(n, levels)
    cases = [("sealed_tank", tank(n, levels), (1,)), ("pool", pool[:2], (0, 1))]
    for name, (lab, w), encs in cases:
        b = D.random_rhs(lab, 1.0 / n)
        for enc in encs:
            o = G.default_options()
            o.enclosed_liquid = enc
            row = {}
            for kind in ("single", "slab"):
                setups = []
                for rep in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    s = G.GeometricMultigridPoissonSolver(lab, w, levels, False, options=o) if kind == "single" else \
                        SlabSolver(lab, w, levels, False, comm, device=0, options=o)
                    torch.cuda.synchronize()
                    setups.append((time.perf_counter() - t0) * 1e3)
                    if rep < 2:
                        s.close()
                bd = s.to_device(b)
                s.solveGeometricConjugateGradient(s.new_grid(), bd, 1e-6, 400, True)  # (warm-up: first-use grids)
                st = s.solveGeometricConjugateGradient(s.new_grid(), bd, 1e-6, 400, True)
                row[kind] = {"setup_ms": float(np.median(setups)), "setup_ms_all": setups, "enclosed": s.enclosed_components(),
                             "iterations": st["iterations"], "outcome": st["outcome"], "ms_per_iteration": st["solve_ms"] / max(1, st["iterations"])}
                s.close()
            out[f"{name}_option{'on' if enc else 'off'}"] = row
    comm.close()
    dist.destroy_process_group()
    return out


def part2_worker(n):
    """one of P ranks over gloo: the set-up's stage lines (the library prints them on stdout) captured per rank"""
    import ctypes
    import tempfile

    import torch
    import torch.distributed as dist

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    levels = int(np.log2(n)) - 3
    lab, w = tank(n, levels)
    nzl = n // size
    z0, z1 = rank * nzl, (rank + 1) * nzl
    o = G.default_options()
    o.enclosed_liquid = 1
    o.min_cells_per_rank = 0
    stages = []
    for rep in range(3):
        sys.stdout.flush()
        with tempfile.TemporaryFile(mode="w+") as f:
            saved = os.dup(1)
            os.dup2(f.fileno(), 1)
            try:
                s = SlabSolver(lab, [w[0][z0:z1], w[1][z0:z1], w[2][z0:z1 + 1]], levels, False, TorchDistComm(), device=0, options=o)
            finally:
                ctypes.CDLL(None).fflush(None)
                os.dup2(saved, 1)
                os.close(saved)
            f.seek(0)
            lines = f.read().splitlines()
        got = {}
        for ln in lines:
            for key in ("slab: enclosed local labelling", "slab: enclosed merge"):
                if key in ln:
                    got[key.split(": ")[1]] = float(ln.split()[-2])
        stages.append(got)
        m = s.enclosed_components()
        s.close()
    res = [None] * size
    dist.all_gather_object(res, {"rank": rank, "stages_ms": stages, "enclosed": m})
    if rank == 0:
        print("RESULT " + json.dumps(res), flush=True)
    dist.destroy_process_group()


def launch(args_list, nproc, env):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port()), os.path.abspath(__file__)] + args_list
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    for ln in res.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[len("RESULT "):])
    raise RuntimeError(res.stdout[-3000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--small", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--role", default="")
    a = ap.parse_args()
    if a.role == "part1":
        print("RESULT " + json.dumps(part1(a.size)), flush=True)
        return
    if a.role == "part2":
        part2_worker(a.small)
        return
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = {"part1_rccl_p1": launch(["--role", "part1", "--size", str(a.size)], 1, env)}
    env2 = dict(env, MGPS_SETUP_TIMING="1")
    out["part2_gloo"] = {"note": "ranks share one GPU; gloo stages every message through the host: no statement about RCCL", "size": a.small}
    for p in (2, 4):
        out["part2_gloo"][f"P{p}"] = launch(["--role", "part2", "--small", str(a.small)], p, env2)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
