"""Worker of tests/test_solid_forces_slabs.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.  The pressure
forces on Z-slabs (include/mgps_fields.h) against the single-device pass on the gathered fields.

modes: "missing" (one rank without one of its arrays: the same refusal on every rank), "slabs" (mgps_solid_forces_slab over
TorchDistComm against mgps_fields_solid_forces and the numpy restatement), "one" (a world
of one over RcclComm behind mgps_project_free_surface_slab, bit for bit, without a transport call), "fail" (a transport whose exchange
fails on one rank).  Prints "WORKER_OK <rank>" on success.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import solid_forces_reference as R  # noqa: E402
import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402
from geometricmultigridpressuresolver_amd.distributed import CommStruct, RcclComm, TorchDistComm  # noqa: E402
from slab_slices import BrokenComm, all_ranks, dev, worker_main  # noqa: E402

SHAPE = (48, 40, 56)  # (gz, gy, gx): 48 base planes
BODIES = 3
SCALE = 0.37


def window(grids, d):
    """the rank's window of three whole-grid face grids: planes c0 .. c1 - 1, of the z-faces c0 .. c1"""
    return [dev(grids[0][d.c0:d.c1]), dev(grids[1][d.c0:d.c1]), dev(grids[2][d.c0:d.c1 + 1])]


def inputs():
    """the scene every rank builds alike: the fields of projection_scene, random ids from -1 .. BODIES + 1, random centres"""
    sc = D.projection_scene(SHAPE)
    rng = np.random.default_rng(31)
    body = [rng.integers(-1, BODIES + 2, size=R.face_shape(SHAPE, a)).astype(np.int32) for a in range(3)]
    centres = rng.random((BODIES + 1, 3)) * np.array([SHAPE[2], SHAPE[1], SHAPE[0]])
    return sc, body, centres


def single_device(sc, pressure, body, centres):
    """the whole-grid pass on the gathered fields, and the restatement on the same"""
    cw = [dev(a) for a in sc["cut_weights"]]
    mat = F.buildMaterialCellLabels(dev(sc["liquid_phi"]), dev(sc["solid_phi"]), cw)
    rows = F.solidForces(dev(pressure), mat, cw, [dev(b) for b in body], centres, SCALE)
    ref, mag = R.solid_forces(pressure, mat.cpu().numpy(), sc["cut_weights"], body, centres, SCALE)
    return rows, ref, mag


def slabs_mode():
    comm = TorchDistComm()
    rank, size = comm.rank, comm.size
    sc, body, centres = inputs()
    pressure = (np.random.default_rng(32).random(SHAPE) * 2 - 0.5).astype(np.float32)  # (junk outside the liquid: the pass masks it)
    whole, ref, mag = single_device(sc, pressure, body, centres)
    assert ref[:, 7].min() > 100, ref[:, 7]
    assert (np.abs(whole[:, :7] - ref[:, :7]) <= 1e-10 * mag[:, :7]).all() and np.array_equal(whole[:, 7], ref[:, 7])
    for p2 in (True, False):
        splits = F.projection_slab_layout(SHAPE, p2, size, False)["splits"]
        d = F.slab_window(SHAPE, p2, splits, rank)
        before = comm.exchanges
        out = F.solid_forces_slab(comm, splits, SHAPE, dev(pressure[d.c0:d.c1]), dev(sc["liquid_phi"][d.c0:d.c1]), dev(sc["solid_phi"][d.c0:d.c1]),
                                  window(sc["cut_weights"], d), window(body, d), centres, SCALE, power_of_two=p2)
        rows = out["rows"]
        assert comm.exchanges - before == 2, comm.exchanges - before  # the liquid_phi plane, then pressure and material in one message
        err = np.abs(rows[:, :7] - whole[:, :7])
        assert (err <= 1e-10 * mag[:, :7]).all() and np.array_equal(rows[:, 7], whole[:, 7]), (p2, float((err / mag[:, :7]).max()))
        seen = all_ranks(rows.tobytes())
        assert all(b == seen[0] for b in seen), "the ranks hold different bits"
        assert out["exchange_ms"] > 0 and out["total_ms"] >= out["exchange_ms"], out
        if rank == 0:
            print(f"slabs power_of_two={p2} cuts {splits}: worst |error| / sum |term| = {float((err / mag[:, :7]).max()):.2e} (bound 1e-10), "
                  f"{int(rows[:, 7].sum())} wet faces, {out['total_ms']:.1f} ms ({out['exchange_ms']:.1f} ms in exchanges)", flush=True)


def one_mode():
    """behind the one-call projection on one rank over RCCL: the published pressure, against the whole-grid pass bit for bit; the
    call is given a vtable whose every entry fails, so a transport call would show as MGPS_ERR_COMM"""
    comm = RcclComm()
    try:
        assert comm.size == 1
        sc, body, centres = inputs()
        splits = F.projection_slab_layout(SHAPE, True, 1, True)["splits"]
        phi, sphi = dev(sc["liquid_phi"]), dev(sc["solid_phi"])
        cw, vel = [dev(a) for a in sc["cut_weights"]], [dev(a) for a in sc["velocity"]]
        pressure = torch.zeros(SHAPE, dtype=torch.float32, device="cuda")
        valid, info = F.project_free_surface_slab(comm, splits, SHAPE, phi, sphi, cw, vel, pressure, None, use_old_pressure=False,
                                                  tolerance=1e-6, max_iterations=300)
        assert info["outcome"] == 0 and pressure.abs().max().item() > 0, info
        ids = [dev(b) for b in body]
        calls = []
        silent = CommStruct()
        silent.struct_size, silent.size = C.sizeof(CommStruct), 1
        keep = [type(silent.exchange)(lambda *a: calls.append("exchange") or 1), type(silent.allreduce)(lambda *a: calls.append("allreduce") or 1)]
        silent.exchange, silent.allreduce = keep
        for transport in (comm, types.SimpleNamespace(struct=silent, rank=0)):
            out = F.solid_forces_slab(transport, splits, SHAPE, pressure, phi, sphi, cw, ids, centres, SCALE)
            whole, ref, mag = single_device(sc, pressure.cpu().numpy(), body, centres)
            assert np.abs(whole[:, :6]).max() > 0 and np.array_equal(out["rows"], whole), "one rank differs from mgps_fields_solid_forces"
            assert (np.abs(whole[:, :7] - ref[:, :7]) <= 1e-10 * mag[:, :7]).all() and np.array_equal(whole[:, 7], ref[:, 7])
            assert out["exchange_ms"] == 0 and not calls, (out, calls)
        print(f"one rank: {int(whole[:, 7].sum())} wet faces, force on body 1 {whole[1, :3]}, equal bits, no transport call", flush=True)
    finally:
        comm.close()


def fail_mode():
    """rank 1's second exchange (pressure and material planes) fails: MGPS_ERR_COMM there, at once.  Rank 0 is left with a transport
    whose peer is gone: its next transport call -- the all-reduce of the rows -- fails too"""
    rank = dist.get_rank()
    comm = BrokenComm(exchange_fails_at=2 if rank == 1 else 0, allreduce_fails_at=1 if rank == 0 else 0)
    assert comm.size == 2
    sc, body, centres = inputs()
    splits = F.projection_slab_layout(SHAPE, True, 2, False)["splits"]
    d = F.slab_window(SHAPE, True, splits, rank)
    pressure = torch.rand(d.base_shape, dtype=torch.float32, device="cuda")
    try:
        F.solid_forces_slab(comm, splits, SHAPE, pressure, dev(sc["liquid_phi"][d.c0:d.c1]), dev(sc["solid_phi"][d.c0:d.c1]),
                            window(sc["cut_weights"], d), window(body, d), centres, SCALE)
    except G.MgpsError as e:
        assert e.status == 8, (rank, e.status, str(e))
        assert ("exchange failed (pressure and material planes)" if rank == 1 else "all-reduce failed") in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: a failing transport went unnoticed")
    assert comm.exchanges == 2, (rank, comm.exchanges)
    print(f"rank {rank}: MGPS_ERR_COMM after {comm.exchanges} exchanges and {comm.allreduces} all-reduces", flush=True)


def missing_mode():
    """rank 1 comes without its y-face ids: it still takes part in both exchanges (with whatever its buffers hold), its status
    travels in the all-reduce, and both ranks return MGPS_ERR_INVALID_ARGUMENT -- rank 1 with its own message, rank 0 naming rank 1.
    The same transport then serves a complete call: nobody was left behind in a collective"""
    comm = TorchDistComm()
    rank = comm.rank
    assert comm.size == 2
    sc, body, centres = inputs()
    pressure = (np.random.default_rng(32).random(SHAPE) * 2 - 0.5).astype(np.float32)
    splits = F.projection_slab_layout(SHAPE, True, 2, False)["splits"]
    d = F.slab_window(SHAPE, True, splits, rank)
    fields = (dev(pressure[d.c0:d.c1]), dev(sc["liquid_phi"][d.c0:d.c1]), dev(sc["solid_phi"][d.c0:d.c1]), window(sc["cut_weights"], d))
    ids = window(body, d)
    try:
        F.solid_forces_slab(comm, splits, SHAPE, *fields, [ids[0], None if rank == 1 else ids[1], ids[2]], centres, SCALE)
    except G.MgpsError as e:
        assert e.status == 1, (rank, e.status, str(e))
        assert ("body: three grids are required" if rank == 1 else "rank 1 failed (rows, status 1)") in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: a missing array on rank 1 went unnoticed")
    assert comm.exchanges == 2, (rank, comm.exchanges)
    rows = F.solid_forces_slab(comm, splits, SHAPE, *fields, ids, centres, SCALE)["rows"]
    whole, ref, mag = single_device(sc, pressure, body, centres)
    assert (np.abs(rows[:, :7] - whole[:, :7]) <= 1e-10 * mag[:, :7]).all() and np.array_equal(rows[:, 7], whole[:, 7])
    print(f"rank {rank}: MGPS_ERR_INVALID_ARGUMENT on both ranks after {comm.exchanges} exchanges; the next call is complete", flush=True)


if __name__ == "__main__":
    worker_main({"slabs": slabs_mode, "one": one_mode, "fail": fail_mode, "missing": missing_mode})
