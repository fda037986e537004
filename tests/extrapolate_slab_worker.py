"""Worker of tests/test_extrapolation_slabs.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.  The velocity
extrapolation on Z-slabs (include/mgps_fields.h) against the single-device passes of the same scene.

modes: "slabs" (mgps_extrapolate_velocity_slab and the slab pass by hand against mgps_fields_extrapolate3, bit for bit), "one"
(RcclComm with a world of one, behind mgps_project_free_surface_slab, against the numpy restatement), "fail" (a transport whose
exchange fails on one rank), "missing" (one rank without one of its cut-weight grids: the refusal every rank gets, and a complete
call on the same transport).  Prints "WORKER_OK <rank>" on success.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extrapolation_reference as R  # noqa: E402
import geometricmultigridpressuresolver_amd as G  # noqa: E402
from geometricmultigridpressuresolver_amd import domains as D  # noqa: E402
from geometricmultigridpressuresolver_amd import fields as F  # noqa: E402
from geometricmultigridpressuresolver_amd.distributed import RcclComm, TorchDistComm  # noqa: E402
from slab_slices import BrokenComm, all_ranks, dev, worker_main  # noqa: E402

SHAPE = (96, 64, 64)  # (gz, gy, gx): offset 16, 128 expanded planes with either expansion
CUTS = {1: [0, 128], 2: [0, 64, 128], 4: [0, 32, 64, 96, 128]}  # base cuts at 48 / at 16, 48, 80
LAYERS = 6


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return a.view(np.uint32) if a.dtype == np.float32 else a


def window(grids, d):
    """the rank's window of three whole-grid face grids: planes c0 .. c1 - 1, of the z-faces c0 .. c1"""
    return [grids[0][d.c0:d.c1], grids[1][d.c0:d.c1], grids[2][d.c0:d.c1 + 1]]


def halos(grids, d):
    """the planes next to the window as an exchange delivers them: base planes c0 - 1 and c1, of the z-faces planes c0 - 1 and c1 + 1"""
    lo = [grids[0][d.c0 - 1], grids[1][d.c0 - 1], grids[2][d.c0 - 1]] if d.c0 > 0 else None
    hi = [grids[0][d.c1], grids[1][d.c1], grids[2][d.c1 + 1]] if d.c1 < d.gz else None
    return ([t.contiguous() for t in lo] if lo else None, [t.contiguous() for t in hi] if hi else None)


def device_scene():
    """projection_scene on the device with the valid faces of the device passes (tests/test_fields.py holds them to the oracle)"""
    sc = D.projection_scene(SHAPE)
    cw, vel = [dev(a) for a in sc["cut_weights"]], [dev(a) for a in sc["velocity"]]
    mat = F.buildMaterialCellLabels(dev(sc["liquid_phi"]), dev(sc["solid_phi"]), cw)
    return sc, cw, vel, F.buildValidFaces(mat, cw)


def whole_grid(vel, valid, layers, cw):
    v = [t.clone() for t in vel]
    layer, filled = F.extrapolateVelocity(v, valid, layers, cw)
    return v, layer, filled


def slabs_mode():
    comm = TorchDistComm()
    rank, size = comm.rank, comm.size
    splits = CUTS[size]
    sc, cw_all, vel, valid = device_scene()
    for p2 in (True, False):
        d = F.slab_window(SHAPE, p2, splits, rank)
        for with_cw in (True, False):
            what = f"power_of_two={p2} cut weights {with_cw}"
            cw = cw_all if with_cw else None
            ref_v, ref_layer, ref_filled = whole_grid(vel, valid, LAYERS, cw)
            # non-vacuity: the front crosses a cut -- faces of layers >= 2 within two planes of it on both sides
            crossed = []
            for e in splits[1:-1]:
                k = e - d.offset
                below = [((g[k - 2:k] >= 2) & (g[k - 2:k] < R.OPEN)).any().item() for g in ref_layer[:2]]  # (the x-face and y-face grids)
                above = [((g[k:k + 2] >= 2) & (g[k:k + 2] < R.OPEN)).any().item() for g in ref_layer[:2]]
                crossed.append(any(below) and any(above))
            assert any(crossed), (what, crossed)
            assert all(min(int((g == l).sum()) for l in range(1, LAYERS + 1)) > 0 for g in ref_layer), what
            # the one call
            w_vel = [t.clone() for t in window(vel, d)]
            w_cw = [t.contiguous() for t in window(cw, d)] if with_cw else None
            before = comm.exchanges
            out = F.extrapolate_velocity_slab(comm, splits, SHAPE, w_vel, [t.contiguous() for t in window(valid, d)], LAYERS, cut_weights=w_cw, power_of_two=p2)
            torch.cuda.synchronize()
            assert comm.exchanges - before == LAYERS, (what, comm.exchanges - before)  # one message per neighbour and layer
            for a in range(3):
                assert np.array_equal(bits(w_vel[a]), bits(window(ref_v, d)[a])), (what, "velocity", a)
                assert np.array_equal(bits(out["layer"][a]), bits(window(ref_layer, d)[a])), (what, "layer", a)
            assert out["filled"] == ref_filled, (what, out["filled"], ref_filled)
            assert out["exchange_ms"] > 0 and out["total_ms"] >= out["exchange_ms"], out
            planes = all_ranks((bits(w_vel[2][0]), bits(w_vel[2][-1]), bits(out["layer"][2][0]), bits(out["layer"][2][-1])))
            for r in range(size - 1):  # rank r's last z-face plane is rank r + 1's first
                assert np.array_equal(planes[r][1], planes[r + 1][0]) and np.array_equal(planes[r][3], planes[r + 1][2]), (what, r)
            if rank == 0:
                print(f"slabs {what}: filled {out['filled']}, cuts crossed by the front {crossed}, {out['total_ms']:.1f} ms ({out['exchange_ms']:.1f} ms in exchanges)", flush=True)
    # the slab pass by hand: layer 0 from the valid flags, then layer 3 on the whole grid's state after layer 2
    d = F.slab_window(SHAPE, True, splits, rank)
    v2, l2, f2 = whole_grid(vel, valid, 2, cw_all)
    v3, l3, f3 = whole_grid(vel, valid, 3, cw_all)
    w_layer = [torch.full_like(t, 77) for t in window(l2, d)]
    F.extrapolateVelocityLayerSlab(d, 0, [t.clone() for t in window(vel, d)], w_layer, valid_faces=[t.contiguous() for t in window(valid, d)])
    for a in range(3):
        assert np.array_equal(bits(w_layer[a]), np.where(bits(window(valid, d)[a]) == 1, 0, 255)), ("layer 0", a)
    w_vel, w_layer = [t.clone() for t in window(v2, d)], [t.clone() for t in window(l2, d)]
    count = torch.zeros(3, dtype=torch.int64, device="cuda")
    F.extrapolateVelocityLayerSlab(d, 3, w_vel, w_layer, velocity_halo=halos(v2, d), layer_halo=halos(l2, d),
                                   cut_cell_weights=[t.contiguous() for t in window(cw_all, d)], filled=count)
    torch.cuda.synchronize()
    for a in range(3):
        assert np.array_equal(bits(w_vel[a]), bits(window(v3, d)[a])) and np.array_equal(bits(w_layer[a]), bits(window(l3, d)[a])), ("layer 3 by hand", a)
    counts = np.sum(all_ranks(count.cpu().numpy()), axis=0)
    assert counts.tolist() == [f3[a] - f2[a] for a in range(3)] and min(counts) > 0, (counts, f2, f3)


def one_mode():
    """behind the one-call projection on one rank over RCCL: the restatement applied to the projected velocity"""
    comm = RcclComm()
    try:
        assert comm.size == 1
        sc = D.projection_scene(SHAPE)
        cw, vel = [dev(a) for a in sc["cut_weights"]], [dev(a) for a in sc["velocity"]]
        pressure = torch.zeros(SHAPE, dtype=torch.float32, device="cuda")
        valid, info = F.project_free_surface_slab(comm, CUTS[1], SHAPE, dev(sc["liquid_phi"]), dev(sc["solid_phi"]), cw, vel, pressure, None,
                                                  use_old_pressure=False, tolerance=1e-6, max_iterations=300)
        assert info["outcome"] == 0, info
        projected = [t.cpu().numpy() for t in vel]
        out = F.extrapolate_velocity_slab(comm, CUTS[1], SHAPE, vel, valid, LAYERS, cut_weights=cw)
        torch.cuda.synchronize()
        assert out["exchange_ms"] == 0, out
        for a in range(3):
            flags, c = valid[a].cpu().numpy(), sc["cut_weights"][a]
            ref_v, ref_layer, ref_filled = R.extrapolate(projected[a], flags, LAYERS, c, np.float64)
            got = vel[a].cpu().numpy()
            assert np.array_equal(out["layer"][a].cpu().numpy(), ref_layer) and out["filled"][a] == sum(ref_filled) and min(ref_filled) > 0, a
            err, lim = float(np.abs(got - ref_v).max()), R.bound(LAYERS, float(np.abs(projected[a]).max()))
            exact = np.array_equal(got, R.extrapolate(projected[a], flags, LAYERS, c)[0])
            print(f"one rank axis {a}: max error {err:.2e} (bound {lim:.2e}), equal to the float32 restatement: {exact}; filled {out['filled'][a]}", flush=True)
            assert err <= lim, (a, err, lim)
            keep = ref_layer != 0
            assert (flags == 1).sum() > 0 and np.array_equal(bits(got[~keep]), bits(projected[a][~keep])), a  # valid faces keep the projected bits
            rest = ref_layer == R.OPEN
            assert np.array_equal(bits(got[rest]), bits(projected[a][rest])), a
    finally:
        comm.close()


def fail_mode():
    """rank 1's exchange in front of the last layer fails: MGPS_ERR_COMM there, at once.  Rank 0 is left with a transport whose peer
    is gone, as on the slab solvers: its next transport call -- the all-reduce at the end -- fails too"""
    rank = dist.get_rank()
    layers = 3
    comm = BrokenComm(exchange_fails_at=layers if rank == 1 else 0, allreduce_fails_at=2 if rank == 0 else 0)
    assert comm.size == 2
    splits = CUTS[2]
    d = F.slab_window(SHAPE, True, splits, rank)
    sc, cw, vel, valid = device_scene()
    w_vel = [t.clone() for t in window(vel, d)]
    try:
        F.extrapolate_velocity_slab(comm, splits, SHAPE, w_vel, [t.contiguous() for t in window(valid, d)], layers)
    except G.MgpsError as e:
        assert e.status == 8, (rank, e.status, str(e))
        assert ("exchange failed (layer 3)" if rank == 1 else "all-reduce failed") in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: a failing transport went unnoticed")
    assert comm.exchanges == layers, (rank, comm.exchanges)
    print(f"rank {rank}: MGPS_ERR_COMM after {comm.exchanges} exchanges and {comm.allreduces} all-reduces", flush=True)


def missing_mode():
    """rank 1 comes with two of its three cut-weight grids: its status travels in the agreement on the arguments, before any exchange,
    and both ranks return MGPS_ERR_INVALID_ARGUMENT -- rank 1 with its own message, rank 0 naming rank 1 and the place.  The same
    transport then serves a complete call, bit-equal to mgps_fields_extrapolate3: nobody was left behind in a collective"""
    comm = TorchDistComm()
    rank = comm.rank
    assert comm.size == 2
    splits = CUTS[2]
    d = F.slab_window(SHAPE, True, splits, rank)
    sc, cw, vel, valid = device_scene()
    w_vel, w_valid = [t.clone() for t in window(vel, d)], [t.contiguous() for t in window(valid, d)]
    w_cw = [t.contiguous() for t in window(cw, d)]
    try:
        F.extrapolate_velocity_slab(comm, splits, SHAPE, w_vel, w_valid, LAYERS, cut_weights=[w_cw[0], None if rank == 1 else w_cw[1], w_cw[2]])
    except G.MgpsError as e:
        assert e.status == 1, (rank, e.status, str(e))
        assert ("cut_weights: all three grids, or none" if rank == 1 else "rank 1 failed (arguments, status 1)") in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: a missing cut-weight grid on rank 1 went unnoticed")
    assert comm.exchanges == 0, (rank, comm.exchanges)
    for a in range(3):
        assert np.array_equal(bits(w_vel[a]), bits(window(vel, d)[a])), a  # (nothing was touched)
    out = F.extrapolate_velocity_slab(comm, splits, SHAPE, w_vel, w_valid, LAYERS, cut_weights=w_cw)
    torch.cuda.synchronize()
    ref_v, ref_layer, ref_filled = whole_grid(vel, valid, LAYERS, cw)
    for a in range(3):
        assert np.array_equal(bits(w_vel[a]), bits(window(ref_v, d)[a])), ("velocity", a)
        assert np.array_equal(bits(out["layer"][a]), bits(window(ref_layer, d)[a])), ("layer", a)
    assert out["filled"] == ref_filled and comm.exchanges == LAYERS, (out["filled"], ref_filled, comm.exchanges)
    print(f"rank {rank}: MGPS_ERR_INVALID_ARGUMENT on both ranks before any exchange; the next call is complete, filled {out['filled']}", flush=True)


if __name__ == "__main__":
    worker_main({"slabs": slabs_mode, "one": one_mode, "fail": fail_mode, "missing": missing_mode})
