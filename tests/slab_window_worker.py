"""Worker of tests/test_slab_window.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.  Slab solvers built
from the rank's own label planes on the device (mgps_create_slab_device_labels: SlabSolver.from_device_labels) against the solver
built from the whole grid's labels; the one-call slab projection that uses it; the cuts from label windows
(mgps_slab_partition_device) against mgps_slab_partition on the assembled labels.

modes: "ranks" (2 or 4 ranks over TorchDistComm/gloo: constructor, enclosed liquid, a failing rank, projection, partition),
"one" (one rank over RcclComm).  Prints "WORKER_OK <rank>" on success.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402
from geometricmultigridpressuresolver_amd.distributed import (  # noqa: E402
    RcclComm, SlabSolver, TorchDistComm, slab_partition, slab_partition_device)
from slab_slices import all_ranks, dev, worker_main  # noqa: E402

LEVEL_ARRAYS = sorted(G.GeometricMultigridPoissonSolver.LEVEL_ARRAYS)


def copy_options(opt):
    o = G.default_options()
    C.memmove(C.addressof(o), C.addressof(opt), C.sizeof(opt))
    return o


def options(**kw):
    o = G.default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def even_cuts(nz, size):
    return [nz // size * r for r in range(size + 1)]


def level_array(solver, level, name):
    """the array, or the library's refusal of it (a list a level does not have): the two solvers must agree on that too"""
    try:
        return solver.level_array(level, name)
    except G.MgpsError as e:
        return f"status {e.status}"


def build_pair(lab, w, lev, gs, opt, cuts, make_comm=TorchDistComm):
    """(solver from the whole grid's labels, solver from the rank's slice of them on the device, their transports)"""
    rank = dist.get_rank()
    z0, z1 = cuts[rank], cuts[rank + 1]
    slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0:z1 + 1]]
    ca, cb = make_comm(), make_comm()
    ref = SlabSolver(lab, [dev(a, np.float32) for a in slab_w], lev, gs, ca, device=0, options=copy_options(opt), splits=cuts)
    win = SlabSolver.from_device_labels(dev(lab[z0:z1], np.uint8), [dev(a, np.float32) for a in slab_w], lab.shape[0], lev, gs, cb, device=0,
                                        options=copy_options(opt), splits=cuts)
    return ref, win, ca, cb


def compare_solvers(what, lab, w, lev, gs, opt, cuts, dx, expect_d=None, comms=None):
    """every set-up array of every distributed level, the shape of the hierarchy, two V-cycles, the MG-PCG iterate and the exchanges a
    cycle costs: all exactly equal -- the same kernels run on the same bytes"""
    rank = dist.get_rank()
    z0, z1 = cuts[rank], cuts[rank + 1]
    ref, win, ca, cb = comms if comms else build_pair(lab, w, lev, gs, opt, cuts)
    try:
        assert win.distributed_levels == ref.distributed_levels and win.getMGLevels() == ref.getMGLevels(), what
        assert expect_d is None or ref.distributed_levels == expect_d, (what, ref.distributed_levels, expect_d)
        assert win.ghost_planes == ref.ghost_planes == 5 and win.slab_range(0) == ref.slab_range(0) == (z0, z1), what
        for l in range(ref.distributed_levels):
            assert win.band_stage_form(l) == ref.band_stage_form(l), (what, l)
            for name in LEVEL_ARRAYS:
                a, b = level_array(ref, l, name), level_array(win, l, name)
                same = (a == b) if isinstance(a, str) or isinstance(b, str) else np.array_equal(a, b)
                assert same, (what, l, name)
        b_glob = D.random_rhs(lab, dx)
        xa, xb = ref.new_grid(), win.new_grid()
        ba, bb = ref.to_device(b_glob[z0:z1]), win.to_device(b_glob[z0:z1])
        for it in range(2):
            ea, eb = ca.exchanges, cb.exchanges
            ref.applyVCycle(xa, ba, it > 0)
            win.applyVCycle(xb, bb, it > 0)
            assert ca.exchanges - ea == cb.exchanges - eb, (what, it, ca.exchanges - ea, cb.exchanges - eb)
        assert torch.equal(xa, xb), (what, "V-cycles")
        assert any(all_ranks(float(xa.abs().max()) > 0)), (what, "the V-cycles left zero everywhere")  # (a rank may own no liquid)
        b_pcg = D.random_rhs(lab, dx, seed=9)
        xa, xb = ref.new_grid(), win.new_grid()
        sa = ref.solveGeometricConjugateGradient(xa, ref.to_device(b_pcg[z0:z1]), 1e-5, 30, True)
        sb = win.solveGeometricConjugateGradient(xb, win.to_device(b_pcg[z0:z1]), 1e-5, 30, True)
        assert sa["iterations"] == sb["iterations"] and sa["outcome"] == sb["outcome"] and torch.equal(xa, xb), (what, sa, sb)
        if rank == 0:
            print(f"  {what}: D={ref.distributed_levels} of {ref.getMGLevels()} levels, cuts {cuts}, pcg {sa['outcome']} at {sa['iterations']}", flush=True)
    finally:
        ref.close()
        win.close()


# ---- the constructor --------------------------------------------------------------------------------------------------------------
def constructor_checks():
    from conftest import make_domain
    from dist_worker import scene_domain
    from test_device_setup import random_domain

    size = dist.get_world_size()
    free = options(min_cells_per_rank=0)
    # the four domains of dist_worker.gpu_mode.  "solid": D = 3 and a label halo of 38 of the neighbour's 64 planes at 2 ranks, D = 2
    # and 18 of 32 at 4; "random": 4 ranks at the 16-plane minimum of a rank (the halo is 8 of the neighbour's 16 planes)
    for kind, g, levels, shape, expect_d in (("solid", 96, 5, (128, 128, 128), 3 if size == 2 else 2), ("simple", 40 if size == 2 else 48, 4, (64, 64, 64), None),
                                             ("scene", 48, 4, (64, 64, 64), None), ("random", 0, 3, (64, 64, 96), None)):
        if kind == "scene":
            lab, w, off, lev, dx = scene_domain(g, levels, shape)
        elif kind == "random":
            lab, w = random_domain(shape, levels, 4, closed_faces=False)
            lev, dx = levels, 1.0 / shape[2]
        else:
            lab, w, off, lev, dx = make_domain(kind, g, levels, shape)
        compare_solvers(kind, lab, w, lev, False, free, even_cuts(lab.shape[0], size), dx, expect_d)
        if kind == "random":  # the halo depth depends on band_width and band_iterations
            compare_solvers("random, band 4 / 4", lab, w, lev, False, options(min_cells_per_rank=0, band_width=4, band_iterations=4),
                            even_cuts(lab.shape[0], size), dx)
    # the uneven cuts of dist_worker.balanced_mode, from slab_partition
    lab, w, lev, dx, opt = balanced_domain(size)
    cuts = slab_partition(lab, lev, size, False, opt)
    assert len({b - a for a, b in zip(cuts, cuts[1:])}) > 1, cuts
    compare_solvers("balanced cuts", lab, w, lev, False, opt, cuts, dx, 2)
    if size == 2:  # Gauss-Seidel with the caller's own cuts
        compare_solvers("gauss-seidel, uneven cuts", lab, w, lev, True, opt, [0, 32, lab.shape[0]], dx, 2)


def balanced_domain(size):
    from conftest import make_domain

    if size == 2:
        lab, w, off, lev, dx = make_domain("simple", 40, 4, (128, 64, 64))
    else:
        bl, bw, dx = D.build_complex_domain((184, 48, 48), dtype=np.float32)
        lab, w, off, lev = D.expand_domain(bl, bw, levels=4, solver_shape=(256, 64, 64))
    return lab, w, lev, dx, options(min_cells_per_rank=10000)


def enclosed_checks():
    """the pockets domain of tests/enclosed_slab_worker.py: components, ranks and the projected solve"""
    from test_enclosed_liquid import three_pockets

    size, rank = dist.get_world_size(), dist.get_rank()
    lab, w = three_pockets()
    cuts = even_cuts(lab.shape[0], size)
    z0, z1 = cuts[rank], cuts[rank + 1]
    opt = options(enclosed_liquid=1)
    ref, win, ca, cb = build_pair(lab, w, 4, False, opt, cuts)
    assert ref.enclosed_components() == win.enclosed_components() and ref.enclosed_components()[0] >= 1, (ref.enclosed_components(), win.enclosed_components())
    assert np.array_equal(ref.enclosed_ranks(), win.enclosed_ranks())
    compare_solvers("enclosed pockets", lab, w, 4, False, opt, cuts, 1.0 / 64, comms=(ref, win, ca, cb))


def failing_rank_check():
    """dist_worker.violation_mode: a BOUNDARY label deep in the liquid of the last rank's planes.  Every rank returns
    MGPS_ERR_HIERARCHY; nobody waits in a collective for the rank that found it"""
    from conftest import make_domain

    size, rank = dist.get_world_size(), dist.get_rank()
    lab, w, off, lev, dx = make_domain("simple", 40 if size == 2 else 48, 4, (64, 64, 64))
    nzl = lab.shape[0] // size
    z0b, z1b = (size - 1) * nzl, size * nzl
    inner = lab == 0
    core = inner.copy()
    core[1:-1, 1:-1, 1:-1] &= inner[:-2, 1:-1, 1:-1] & inner[2:, 1:-1, 1:-1] & inner[1:-1, :-2, 1:-1] & inner[1:-1, 2:, 1:-1] & inner[1:-1, 1:-1, :-2] & inner[1:-1, 1:-1, 2:]
    cand = np.argwhere(core[z0b + 2:z1b - 2])
    assert len(cand) > 0
    k, j, i = (int(v) for v in cand[len(cand) // 2])
    lab = lab.copy()
    lab[k + z0b + 2, j, i] = 3
    z0, z1 = rank * nzl, (rank + 1) * nzl
    try:
        SlabSolver.from_device_labels(dev(lab[z0:z1], np.uint8), [dev(a, np.float32) for a in (w[0][z0:z1], w[1][z0:z1], w[2][z0:z1 + 1])], lab.shape[0], lev, False,
                                      TorchDistComm(), device=0, options=options(min_cells_per_rank=0))
    except G.MgpsError as e:
        status, msg = e.status, str(e)
    else:
        raise AssertionError(f"rank {rank}: labels that break the BOUNDARY-cell rule were accepted")
    assert all(s == 5 for s in all_ranks(status)), all_ranks(status)
    assert ("BOUNDARY-cell rules" if rank == size - 1 else "another rank") in msg, (rank, msg)
    dist.barrier()
    if rank == 0:
        print(f"  violation on rank {size - 1}: rank 0 got '{msg[:90]}'", flush=True)


# ---- the projection ----------------------------------------------------------------------------------------------------------------
class RecordingComm(TorchDistComm):
    """TorchDistComm that notes the bytes of every gatherv / scatterv call as this rank sees them"""

    def __init__(self, group=None):
        self.gatherv_bytes, self.scatterv_bytes = [], []
        super().__init__(group)

    def _gatherv(self, user, send, send_bytes, recv, counts, displs, root, stream):
        self.gatherv_bytes.append(int(send_bytes) + (sum(int(counts[r]) for r in range(self.size) if r != root) if self.rank == root else 0))
        return super()._gatherv(user, send, send_bytes, recv, counts, displs, root, stream)

    def _scatterv(self, user, send, counts, displs, recv, recv_bytes, root, stream):
        self.scatterv_bytes.append(int(recv_bytes))
        return super()._scatterv(user, send, counts, displs, recv, recv_bytes, root, stream)


def projection_checks():
    from projection_slab_worker import CUTS, SHAPE, check_against_single, scene_rhs_max

    size, rank = dist.get_world_size(), dist.get_rank()
    sc = D.projection_scene(SHAPE, with_solid_velocity=True)
    rhs_max, _, _ = scene_rhs_max(sc, SHAPE, True)
    eshape, _, _ = G.expanded_layout(SHAPE, 0, power_of_two=True)
    ecells = int(np.prod(eshape))
    kw = {"use_gauss_seidel": False, "power_of_two": True, "tolerance": 1e-6, "max_iterations": 300}
    comm = RecordingComm()
    check_against_single("projection from label windows", comm, CUTS[size], SHAPE, sc, rhs_max, kw)
    # nobody receives the whole grid's labels any more (before: every rank but 0 received exactly ex * ey * ez bytes in one scatterv)
    assert all(n < ecells for n in comm.scatterv_bytes), (rank, ecells, comm.scatterv_bytes)
    if size == 2:  # the host builder still gets them, and still works
        hosted = RecordingComm()
        check_against_single("projection, host set-up", hosted, CUTS[size], SHAPE, sc, rhs_max, dict(kw, options=options(host_setup=1)))
        assert (max(hosted.scatterv_bytes, default=0) == ecells) == (rank != 0), (rank, ecells, hosted.scatterv_bytes)
    if rank == 0:
        print(f"  projection: largest scatterv {max(comm.scatterv_bytes, default=0)} B of {ecells} B of labels", flush=True)


# ---- the cuts ----------------------------------------------------------------------------------------------------------------------
def odd_cuts(nz, size):
    """uneven cuts whose boundaries are odd plane numbers"""
    even = even_cuts(nz, size)
    return [0] + [c + d for c, d in zip(even[1:-1], (5, -7, 9))] + [nz]


def partition_checks():
    size, rank = dist.get_world_size(), dist.get_rank()
    lab, w, lev, dx, opt = balanced_domain(size)
    nz = lab.shape[0]
    empty = np.full_like(lab, D.EXTERIOR)
    for what, labels, gs in (("balanced", lab, False), ("all EXTERIOR", empty, False), ("gauss-seidel", lab, True)):
        want = slab_partition(labels, lev, size, gs, opt)
        if what == "balanced":
            assert len({b - a for a, b in zip(want, want[1:])}) > 1, want
        else:
            assert want == even_cuts(nz, size), (what, want)
        for now in (even_cuts(nz, size), odd_cuts(nz, size)):
            assert all(c % 2 == 1 for c in now[1:-1]) or now == even_cuts(nz, size)
            got = slab_partition_device(dev(labels[now[rank]:now[rank + 1]], np.uint8), now, lev, gs, TorchDistComm(), opt)
            assert got == want, (what, now, got, want)
        if rank == 0:
            print(f"  partition {what}: {want}", flush=True)


def ranks_mode():
    constructor_checks()
    enclosed_checks()
    failing_rank_check()
    projection_checks()
    partition_checks()


def one_mode():
    """one rank over the library's RCCL transport: the device-resident projection, and the constructor with nobody to trade with"""
    from conftest import make_domain
    from projection_slab_worker import CUTS, SHAPE, check_against_single, scene_rhs_max

    comm = RcclComm()
    try:
        assert comm.size == 1
        sc = D.projection_scene(SHAPE, with_solid_velocity=True)
        for gs in (False, True):
            rhs_max, _, _ = scene_rhs_max(sc, SHAPE, True)
            kw = {"use_gauss_seidel": gs, "power_of_two": True, "tolerance": 1e-6, "max_iterations": 300}
            check_against_single(f"one rank gs={gs}", comm, CUTS[1], SHAPE, sc, rhs_max, kw)
        lab, w, off, lev, dx = make_domain("simple", 40, 4, (64, 64, 64))
        opt = options(min_cells_per_rank=0)
        ref = SlabSolver(lab, [dev(a, np.float32) for a in w], lev, False, comm, device=0, options=copy_options(opt))
        win = SlabSolver.from_device_labels(dev(lab, np.uint8), [dev(a, np.float32) for a in w], lab.shape[0], lev, False, comm, device=0, options=copy_options(opt))
        try:
            assert win.distributed_levels == ref.distributed_levels >= 1 and win.getMGLevels() == ref.getMGLevels()
            for l in range(ref.distributed_levels):
                for name in LEVEL_ARRAYS:
                    a, b = level_array(ref, l, name), level_array(win, l, name)
                    assert (a == b) if isinstance(a, str) or isinstance(b, str) else np.array_equal(a, b), (l, name)
            assert slab_partition_device(dev(lab, np.uint8), [0, lab.shape[0]], lev, False, comm, opt) == [0, lab.shape[0]]
        finally:
            ref.close()
            win.close()
    finally:
        comm.close()


if __name__ == "__main__":
    worker_main({"ranks": ranks_mode, "one": one_mode})
