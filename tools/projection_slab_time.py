#!/usr/bin/env python3
"""The fields layer on Z-slabs, timed on one MI355X against another build of the library (the parent commit's).

    python tools/projection_slab_time.py [--size 480] [--rounds 3] [--parent-lib PATH/libmgps.so] [--out profiles/r08_projection_slab.json]

domains.projection_scene at --size^3 with solid velocities, tight solver grid (as profiles/r07_surface_tension_480.json); the scene
is written once to --scratch (a temporary directory by default) and every measurement runs in a child process of its own, the two libraries in turn, --rounds times
(a library is chosen when it is loaded: MGPS_LIBRARY).  Each child makes one warm-up call and one timed call.
 (a) mgps_project_free_surface on host arrays (--parent-lib) against mgps_project_free_surface_slab with one rank over RcclComm on
     device tensors: total_ms, total - solve, and the slab call's stages.
 (b) the whole-grid front-end passes of --parent-lib (material, valid x3, domain labels, weights x3, BOUNDARY marking, with the
     fills they issue; rhs; gradient x3) against the slab passes of this build on the one-rank window (material, faces, labels; rhs;
     gradient), HIP events, mean of 10 launches.
 (c) 2 and 4 ranks sharing the GPU over TorchDistComm/gloo, surface tension on (four plane exchanges): every rank's stages.  Host
     staging on one device: this says nothing about RCCL between GPUs.
 With --parent-lib, (a)'s slab call and (c) also run on the parent's library, in turn with this build's ("slab_parent",
 "c_gloo_shared_gpu_parent"): what a change of the slab call itself gains, stage by stage, against the parent's own spread.
 (d) --part count: mgps_label_plane_counts (the counting kernel of mgps_slab_partition_device) over the expanded grid's labels, ten
     calls; the kernel's own time comes from running this part under `rocprofv3 --kernel-trace --stats -- python tools/... --part count`."""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["liquid_phi", "solid_phi", "cw0", "cw1", "cw2", "v0", "v1", "v2", "sv0", "sv1", "sv2"]
DT, DENSITY = 1.0 / 60.0, 1000.0


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def write_scene(n, scratch):
    from geometricmultigridpressuresolver_amd import domains as D

    sc = D.projection_scene((n, n, n), with_solid_velocity=True)
    arrays = [sc["liquid_phi"], sc["solid_phi"], *sc["cut_weights"], *sc["velocity"], *sc["solid_velocity"]]
    os.makedirs(scratch, exist_ok=True)
    for name, a in zip(NAMES, arrays):
        np.save(os.path.join(scratch, name + ".npy"), a)
    return sc["dx"]


def read_scene(scratch, z0=None, z1=None):
    """the scene, or the planes [z0, z1) of it (z-face grids: one plane more)"""
    out = {}
    for name in NAMES:
        a = np.load(os.path.join(scratch, name + ".npy"), mmap_mode="r")
        if z0 is not None:
            a = a[z0:z1 + (1 if name in ("cw2", "v2", "sv2") else 0)]
        out[name] = np.array(a, dtype=np.float32, order="C", copy=True)
    return out


def events(fn, reps=10):
    import torch

    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


def brief(info):
    keep = ("iterations", "outcome", "setup_ms", "solve_ms", "total_ms", "divergence_max", "liquid_cells")
    out = {k: (round(info[k], 2) if k.endswith("_ms") else info[k]) for k in keep}
    out["outside_solve_ms"] = round(info["total_ms"] - info["solve_ms"], 2)
    if "stage_ms" in info:
        out["stage_ms"] = {k: round(v, 2) for k, v in info["stage_ms"].items()}
    return out


def part_whole(a):
    """--parent-lib's side: the host-array call and the whole-grid passes"""
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    n = a.size
    shape = (n, n, n)
    s = read_scene(a.scratch)
    cw, vel, sv = [s["cw0"], s["cw1"], s["cw2"]], [s["v0"], s["v1"], s["v2"]], [s["sv0"], s["sv1"], s["sv2"]]
    res = {}
    for which in ("warm_up", "timed"):
        v = [x.copy() for x in vel]
        _, info = F.project_free_surface(s["liquid_phi"], s["solid_phi"], cw, v, np.zeros(shape, np.float32), sv, use_old_pressure=False,
                                         tolerance=1e-5, max_iterations=500, power_of_two=False)
        res[which] = brief(info)
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    dcw, dvel, dsv, phi, sphi = [dev(x) for x in cw], [dev(x) for x in vel], [dev(x) for x in sv], dev(s["liquid_phi"]), dev(s["solid_phi"])
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=False)
    st = {}

    def front():
        st["m"] = F.buildMaterialCellLabels(phi, sphi, dcw)
        st["valid"] = F.buildValidFaces(st["m"], dcw)
        st["labels"], st["w"] = F.buildMGDomain(st["m"], dcw, phi, st["valid"], eshape, offset)

    passes = {"front_end": events(front)}
    passes["rhs"] = events(lambda: F.buildRHS(st["m"], dvel, dcw, eshape, offset, dsv))
    pressure = torch.where(st["m"] == 1, torch.rand(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    passes["gradient_x3"] = events(lambda: F.applyPressureGradient(dvel, phi, pressure, st["valid"], st["m"]))
    res["passes_ms"] = passes
    print("RESULT " + json.dumps(res), flush=True)


def part_slab(a):
    """this build's side: the slab call with one rank over RcclComm, and the slab passes on the one-rank window"""
    import torch
    import torch.distributed as dist

    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd.distributed import RcclComm

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    torch.cuda.set_device(0)
    comm = RcclComm()
    n = a.size
    shape = (n, n, n)
    s = read_scene(a.scratch)
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    dcw, dsv, phi, sphi = [dev(s[k]) for k in ("cw0", "cw1", "cw2")], [dev(s[k]) for k in ("sv0", "sv1", "sv2")], dev(s["liquid_phi"]), dev(s["solid_phi"])
    lay = F.projection_slab_layout(shape, False, 1, True)
    res = {}
    for which in ("warm_up", "timed"):
        dvel = [dev(s[k]) for k in ("v0", "v1", "v2")]
        _, info = F.project_free_surface_slab(comm, lay["splits"], shape, phi, sphi, dcw, dvel, torch.zeros(shape, device="cuda"), dsv,
                                              use_old_pressure=False, tolerance=1e-5, max_iterations=500, power_of_two=False)
        torch.cuda.synchronize()
        res[which] = brief(info)
    d = F.slab_window(shape, False, lay["splits"], 0)
    st = {}

    def front():
        st["m"] = F.buildMaterialCellLabelsSlab(d, phi, None, sphi, dcw)
        st["valid"], st["w"] = F.buildFacesSlab(d, st["m"], None, phi, None, dcw)
        st["labels"] = F.buildLabelsSlab(d, st["m"], None, st["w"])

    passes = {"front_end": events(front)}
    passes["rhs"] = events(lambda: F.buildRHSSlab(d, st["m"], dvel, dcw, dsv))
    pressure = torch.where(st["m"] == 1, torch.rand(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    passes["gradient_x3"] = events(lambda: F.applyPressureGradientSlab(d, dvel, phi, None, pressure, None, st["valid"], st["m"], None))
    res["passes_ms"] = passes
    print("RESULT " + json.dumps(res), flush=True)
    comm.close()
    dist.destroy_process_group()


def part_ranks(a):
    """under torch.distributed.run: every rank's window over TorchDistComm/gloo, surface tension on"""
    import torch
    import torch.distributed as dist

    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd.distributed import TorchDistComm

    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    comm = TorchDistComm()
    n = a.size
    shape = (n, n, n)
    lay = F.projection_slab_layout(shape, False, comm.size, True)
    d = F.slab_window(shape, False, lay["splits"], comm.rank)
    s = read_scene(a.scratch, d.c0, d.c1)
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    dcw, dsv, phi, sphi = [dev(s[k]) for k in ("cw0", "cw1", "cw2")], [dev(s[k]) for k in ("sv0", "sv1", "sv2")], dev(s["liquid_phi"]), dev(s["solid_phi"])
    dx = 1.0 / n
    res = {}
    for which in ("warm_up", "timed"):
        dvel = [dev(s[k]) for k in ("v0", "v1", "v2")]
        _, info = F.project_free_surface_slab(comm, lay["splits"], shape, phi, sphi, dcw, dvel, torch.zeros(d.base_shape, device="cuda"), dsv,
                                              use_old_pressure=False, tolerance=1e-5, max_iterations=500, power_of_two=False,
                                              surface_tension=DENSITY * dx * dx / DT, dt=DT, dx=dx, density=DENSITY)
        torch.cuda.synchronize()
        res[which] = brief(info)
    seen = [None] * comm.size
    dist.all_gather_object(seen, res["timed"])
    if comm.rank == 0:
        print("RESULT " + json.dumps({"cuts": lay["splits"], "label_bytes_per_rank": int(np.prod(lay["expanded"])), "plane_bytes": 4 * n * n,
                                      "ranks": seen}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def part_count(a):
    """the plane counts of the expanded grid's labels (random labels: the kernel's time does not depend on them)"""
    import ctypes as C
    import time

    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd._lib import check

    n = a.size
    (ez, ey, ex), _, _ = G.expanded_layout((n, n, n), 0, power_of_two=False)
    lab = torch.randint(0, 4, (ez, ey, ex), dtype=torch.uint8, device="cuda")
    act, bnd = (C.c_int64 * ez)(), (C.c_int64 * ez)()
    times = []
    for _ in range(11):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        check(G.lib().mgps_label_plane_counts(ex, ey, ez, C.c_void_p(lab.data_ptr()), act, bnd))
        times.append((time.perf_counter() - t0) * 1e3)
    assert sum(act) == int(((lab == 0) | (lab == 3)).sum().item()) and sum(bnd) == int((lab == 3).sum().item())
    print("RESULT " + json.dumps({"expanded": [ez, ey, ex], "bytes": ez * ey * ex, "call_ms_min": round(min(times[1:]), 4),
                                  "call_ms_median": round(float(np.median(times[1:])), 4)}), flush=True)


def child(args, lib=None, nproc=0, timeout=900):
    env = dict(os.environ)
    if lib:
        env["MGPS_LIBRARY"] = os.path.abspath(lib)
    cmd = [sys.executable] + (["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(free_port())]
                              if nproc else []) + [os.path.abspath(__file__)] + args
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError(f"{cmd} failed:\n{out.stdout[-3000:]}")
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="the library of the commit to compare with (default: this build, whose whole-grid entry points are the parent's)")
    ap.add_argument("--scratch", default="", help="where the scene is written (default: a fresh temporary directory, removed at the end)")
    ap.add_argument("--ranks", default="2,4")
    ap.add_argument("--skip-whole", action="store_true", help="leave (a)'s host-array call and (b) out (a change that does not touch them)")
    ap.add_argument("--out", default="")
    ap.add_argument("--part", default="")
    a = ap.parse_args()
    if a.part:
        return {"whole": part_whole, "slab": part_slab, "ranks": part_ranks, "count": part_count}[a.part](a)
    import torch

    own_scratch = None
    if not a.scratch:
        own_scratch = tempfile.TemporaryDirectory(prefix="projection_slab_scene_")
        a.scratch = own_scratch.name
    write_scene(a.size, a.scratch)
    common = ["--size", str(a.size), "--scratch", a.scratch]
    out = {"size": a.size, "device": torch.cuda.get_device_name(0), "power_of_two": False, "rounds": a.rounds,
           "parent_library": "given" if a.parent_lib else "this build", "whole": [], "slab": [], "slab_parent": []}
    for r in range(a.rounds):  # the sides in turn
        if not a.skip_whole:
            out["whole"].append(child(common + ["--part", "whole"], lib=a.parent_lib))
            print("whole", json.dumps(out["whole"][-1]), flush=True)
        if a.parent_lib:
            out["slab_parent"].append(child(common + ["--part", "slab"], lib=a.parent_lib))
            print("slab_parent", json.dumps(out["slab_parent"][-1]), flush=True)
        out["slab"].append(child(common + ["--part", "slab"]))
        print("slab", json.dumps(out["slab"][-1]), flush=True)
    med = lambda side, f: round(float(np.median([f(r) for r in out[side]])), 3)  # noqa: E731
    sides = [s for s in ("whole", "slab_parent", "slab") if out[s]] if out["slab"] else []
    spread = lambda side, f: [round(float(min(f(r) for r in out[side])), 3), round(float(max(f(r) for r in out[side])), 3)]  # noqa: E731
    out["median"] = {} if not sides else {
        "a_total_ms": {s: med(s, lambda r: r["timed"]["total_ms"]) for s in sides},
        "a_outside_solve_ms": {s: med(s, lambda r: r["timed"]["outside_solve_ms"]) for s in sides},
        "a_outside_solve_ms_min_max": {s: spread(s, lambda r: r["timed"]["outside_solve_ms"]) for s in sides},
        "a_solve_ms": {s: med(s, lambda r: r["timed"]["solve_ms"]) for s in sides},
        "a_slab_stage_ms": {s: {k: med(s, lambda r, k=k: r["timed"]["stage_ms"][k]) for k in out[s][0]["timed"]["stage_ms"]} for s in sides if s != "whole"},
        "a_slab_stage_1_plus_2_ms_min_max": {s: spread(s, lambda r: sum(list(r["timed"]["stage_ms"].values())[1:3])) for s in sides if s != "whole"},
        "b_passes_ms": {k: {s: med(s, lambda r, k=k: r["passes_ms"][k]) for s in sides} for k in ("front_end", "rhs", "gradient_x3")},
    }
    out["c_gloo_shared_gpu"], out["c_gloo_shared_gpu_parent"] = {}, {}
    for nproc in [int(v) for v in a.ranks.split(",") if v]:
        if a.parent_lib:
            out["c_gloo_shared_gpu_parent"][str(nproc)] = child(common + ["--part", "ranks"], lib=a.parent_lib, nproc=nproc, timeout=1500)
            print(nproc, "ranks, parent", json.dumps(out["c_gloo_shared_gpu_parent"][str(nproc)]), flush=True)
        out["c_gloo_shared_gpu"][str(nproc)] = child(common + ["--part", "ranks"], nproc=nproc, timeout=1500)
        print(nproc, "ranks", json.dumps(out["c_gloo_shared_gpu"][str(nproc)]), flush=True)
    out["d_plane_counts"] = child(common + ["--part", "count"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
