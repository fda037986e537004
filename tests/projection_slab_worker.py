"""Worker of tests/test_projection_slabs.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.  The fields
layer on Z-slabs (include/mgps_fields.h) against the single-device passes and the single-device one-call
projection of the same scene.

modes: "passes" (every slab pass against the whole-grid pass, sliced), "onecall" (mgps_project_free_surface_slab against
mgps_project_free_surface), "options" (enclosed liquid, surface tension, a caller's surface pressure), "edges" (no liquid, liquid
on one rank, a bad argument on one rank, a transport without gatherv), "missing" (one rank without one of its solid velocities: the
refusal every rank gets, and a complete call on the same transport), "one" (RcclComm with a world of one).  Prints
"WORKER_OK <rank>" on success.
"""
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
from geometricmultigridpressuresolver_amd.distributed import RcclComm, TorchDistComm  # noqa: E402
from slab_slices import all_ranks, cell, dev, faces, halo, worker_main, zface  # noqa: E402

SHAPE = (96, 64, 64)  # (gz, gy, gx): 5 levels, offset 16, 128 expanded planes with either expansion
CUTS = {1: [0, 128], 2: [0, 64, 128], 4: [0, 32, 64, 96, 128]}  # every rank owns base planes; valid for both smoothers
LIQUID, AIR = 1, 2


def h(a):
    return np.array(a, dtype=np.float32, order="C", copy=True)


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def cut_faces(material, cw, splits, offset):
    """liquid-air z-faces and fractional cut-cell z-faces on the base planes of the interior cuts"""
    la = frac = 0
    for e in splits[1:-1]:
        k = e - offset
        if 0 < k < material.shape[0]:
            a, b = material[k - 1], material[k]
            la += int((((a == LIQUID) & (b == AIR)) | ((a == AIR) & (b == LIQUID))).sum())
            frac += int(((cw[2][k] > 0) & (cw[2][k] < 1)).sum())
    return la, frac


# ---- 2. every slab pass against the whole-grid pass ------------------------------------------------------------------------------
def passes_mode():
    size, rank = dist.get_world_size(), dist.get_rank()
    splits = CUTS[size]
    scenes = [("default", {}, True), ("default tight", {}, False), ("seed 1", {"seed": 1, "randomize": True}, True), ("seed 2", {"seed": 2, "randomize": True}, True)]
    seen_la = seen_frac = 0
    bit_equal = {}
    for name, kw, p2 in scenes:
        sc = D.projection_scene(SHAPE, with_solid_velocity=True, **kw)
        eshape, offset, levels = G.expanded_layout(SHAPE, 0, power_of_two=p2)
        d = F.slab_window(SHAPE, p2, splits, rank)
        assert (d.ez, d.ey, d.ex) == tuple(eshape) and d.offset == offset and (d.e0, d.e1) == (splits[rank], splits[rank + 1]) and d.c0 < d.c1
        # the whole grid, pass by pass
        phi, sphi = dev(sc["liquid_phi"]), dev(sc["solid_phi"])
        cw, vel, sv = [dev(a) for a in sc["cut_weights"]], [dev(a) for a in sc["velocity"]], [dev(a) for a in sc["solid_velocity"]]
        mat = F.buildMaterialCellLabels(phi, sphi, cw)
        valid = F.buildValidFaces(mat, cw)
        labels, weights = F.buildMGDomain(mat, cw, phi, valid, eshape, offset)
        rhs = F.buildRHS(mat, vel, cw, eshape, offset, sv)
        material = mat.cpu().numpy()
        la, frac = cut_faces(material, sc["cut_weights"], splits, offset)
        seen_la, seen_frac = seen_la + la, seen_frac + frac
        if name == "default":
            assert la >= 1, "no liquid-air face on a cut: the scene no longer tests the halo"
        rng = np.random.default_rng(11)
        p_seed = np.where(material == LIQUID, rng.random(SHAPE) * 0.3, 0.0).astype(np.float32)
        x = F.applyOldPressure(dev(p_seed), mat, eshape, offset)
        p_back = torch.full(SHAPE, 7.0, dtype=torch.float32, device="cuda")
        F.applySolutionToPressure(p_back, x, mat, offset)
        vel_g = [v.clone() for v in vel]
        F.applyPressureGradient(vel_g, phi, dev(p_seed), valid, mat)
        sp = F.buildSurfacePressure(phi, mat, 0.5)
        rhs_s = rhs.clone()
        pmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        F.addSurfacePressureToRHS(rhs_s, weights, phi, mat, sp, offset, pmax)
        vel_s = [v.clone() for v in vel]
        F.applyPressureGradient(vel_s, phi, dev(p_seed), valid, mat, surface_pressure=sp)
        div = F.computeResultingDivergence(mat, vel_g, cw, sv)
        # the window, pass by pass; the halo planes are the neighbours' planes of the whole-grid arrays
        sp_h, mat_h = sp.cpu().numpy(), material
        w_phi, w_cw = dev(cell(sc["liquid_phi"], d)), [dev(a) for a in faces(sc["cut_weights"], d)]
        w_vel, w_sv = [dev(a) for a in faces(sc["velocity"], d)], [dev(a) for a in faces(sc["solid_velocity"], d)]
        phi_halo, mat_halo, sp_halo, p_halo = halo(sc["liquid_phi"], d), halo(mat_h, d), halo(sp_h, d), halo(p_seed, d)
        w_mat = F.buildMaterialCellLabelsSlab(d, w_phi, phi_halo, dev(cell(sc["solid_phi"], d)), w_cw)
        assert np.array_equal(w_mat.cpu().numpy(), cell(material, d)), name
        w_valid, w_weights = F.buildFacesSlab(d, w_mat, mat_halo, w_phi, phi_halo, w_cw)
        ref_valid = faces([v.cpu().numpy() for v in valid], d)
        e = slice(d.e0, d.e1)
        ref_w = [weights[0][e].cpu().numpy(), weights[1][e].cpu().numpy(), weights[2][d.e0:d.e1 + 1].cpu().numpy()]

        def note(what, got, ref):
            bit_equal[what] = bit_equal.get(what, True) and bool(np.array_equal(got, ref))

        for a in range(3):
            assert np.array_equal(w_valid[a].cpu().numpy(), ref_valid[a]), (name, a)
            got = w_weights[a].cpu().numpy()
            assert np.abs(got - ref_w[a]).max() <= 2e-6 * np.abs(ref_w[a]).max(), (name, a)
            note("weights", got, ref_w[a])
        w_labels = F.buildLabelsSlab(d, w_mat, mat_halo, w_weights)
        assert np.array_equal(w_labels.cpu().numpy(), labels[e].cpu().numpy()), name
        w_rhs = F.buildRHSSlab(d, w_mat, w_vel, w_cw, w_sv)
        assert np.abs(w_rhs.cpu().numpy() - rhs[e].cpu().numpy()).max() < 1e-5, name
        note("rhs", w_rhs.cpu().numpy(), rhs[e].cpu().numpy())
        w_x = F.applyOldPressureSlab(d, dev(cell(p_seed, d)), w_mat)
        assert np.array_equal(w_x.cpu().numpy(), x[e].cpu().numpy()), name
        w_p = torch.full(d.base_shape, 7.0, dtype=torch.float32, device="cuda")
        F.applySolutionToPressureSlab(d, w_p, w_x, w_mat)
        assert np.array_equal(w_p.cpu().numpy(), cell(p_back.cpu().numpy(), d)), name
        F.applySolutionToPressureSlab(d, w_p, w_x, w_mat, clear_others=True)
        assert np.array_equal(w_p.cpu().numpy(), cell(p_seed, d)), name
        w_vel_g = [v.clone() for v in w_vel]
        F.applyPressureGradientSlab(d, w_vel_g, w_phi, phi_halo, dev(cell(p_seed, d)), p_halo, w_valid, w_mat, mat_halo)
        for a, ref in enumerate(faces([v.cpu().numpy() for v in vel_g], d)):
            got = w_vel_g[a].cpu().numpy()
            assert np.abs(got - ref).max() < 2e-5 * np.abs(ref).max(), (name, a)
            note("gradient", got, ref)
        # surface tension: the bounds of tests/test_surface_tension.py::test_device_passes_match_numpy
        w_sp = F.buildSurfacePressureSlab(d, w_phi, phi_halo, w_mat, mat_halo, 0.5)
        ref = cell(sp_h, d)
        assert np.abs(sp_h).max() > 0 and np.abs(w_sp.cpu().numpy() - ref).max() <= 1e-5 * np.abs(sp_h).max(), name
        note("surface pressure", w_sp.cpu().numpy(), ref)
        w_pmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        w_rhs_s = w_rhs.clone()
        F.addSurfacePressureToRHSSlab(d, w_rhs_s, w_weights, w_phi, phi_halo, w_mat, mat_halo, w_sp, sp_halo, w_pmax)
        ref = rhs_s[e].cpu().numpy()
        assert np.abs(w_rhs_s.cpu().numpy() - ref).max() <= 1e-6 * np.abs(rhs_s.cpu().numpy()).max(), name
        note("surface rhs term", w_rhs_s.cpu().numpy(), ref)
        pmaxes = all_ranks(w_pmax.item())
        assert abs(max(pmaxes) - pmax.item()) <= 1e-6 * pmax.item(), (name, pmaxes, pmax.item())
        w_vel_s = [v.clone() for v in w_vel]
        F.applyPressureGradientSlab(d, w_vel_s, w_phi, phi_halo, dev(cell(p_seed, d)), p_halo, w_valid, w_mat, mat_halo, w_sp, sp_halo)
        for a, ref in enumerate(faces([v.cpu().numpy() for v in vel_s], d)):
            got = w_vel_s[a].cpu().numpy()
            assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), (name, a)
            note("surface gradient", got, ref)
        # divergence partials: the ranks' sums, maxima and counts give the whole grid's report
        parts = all_ranks(F.computeResultingDivergenceSlab(d, w_mat, w_vel_g, w_cw, w_sv))
        total = (sum(q[0] for q in parts), max(q[1] for q in parts), sum(q[2] for q in parts))
        assert total[2] == div[2] and abs(total[0] - div[0]) < 1e-4 * div[2] and abs(total[1] - div[1]) <= 1e-5 * div[1], (name, total, div)
        if rank == 0:
            print(f"passes {name}: {la} liquid-air and {frac} fractional z-faces on the cuts {splits[1:-1]}", flush=True)
    assert seen_la >= 1 and seen_frac >= 1, (seen_la, seen_frac)
    print(f"rank {rank}: bit-equal float arrays {bit_equal}", flush=True)
    # one definition per rule: the two kernel families round alike, not only within the bounds above
    assert len(bit_equal) == 6 and all(bit_equal.values()), bit_equal


# ---- 3. the one call against the single-device call -------------------------------------------------------------------------------
def window_tensors(sc, d, pressure=None):
    t = {
        "liquid_phi": dev(cell(sc["liquid_phi"], d)), "solid_phi": dev(cell(sc["solid_phi"], d)),
        "cut_weights": [dev(a) for a in faces(sc["cut_weights"], d)], "velocity": [dev(a) for a in faces(sc["velocity"], d)],
        "solid_velocity": [dev(a) for a in faces(sc["solid_velocity"], d)] if sc.get("solid_velocity") is not None else None,
        "pressure": dev(cell(pressure, d)) if pressure is not None else torch.zeros(d.base_shape, dtype=torch.float32, device="cuda"),
    }
    return t


def single_device(sc, shape, pressure=None, **kw):
    vel = [h(a) for a in sc["velocity"]]
    p = h(pressure) if pressure is not None else np.zeros(shape, dtype=np.float32)
    sv = [h(a) for a in sc["solid_velocity"]] if sc.get("solid_velocity") is not None else None
    valid, info = F.project_free_surface(h(sc["liquid_phi"]), h(sc["solid_phi"]), [h(a) for a in sc["cut_weights"]], vel, p, sv, **kw)
    return vel, p, valid, info


def slab_call(comm, splits, shape, sc, d, pressure=None, **kw):
    t = window_tensors(sc, d, pressure)
    valid, info = F.project_free_surface_slab(comm, splits, shape, t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"],
                                              t["solid_velocity"], **kw)
    torch.cuda.synchronize()
    return t, valid, info


def check_against_single(what, comm, splits, shape, sc, rhs_max, kw, perr_bound=1e-4):
    """the bounds of test 3: exact flags and layout, converged, iterations +-1, pressure 1e-4 relative L2 (the bounds
    tests/dist_worker.py puts on slab-against-whole MG-PCG), divergence_max < 2e-4 max|rhs|, one report on every rank, equal copies
    of every cut's z-face plane, and a warm start from the answer that leaves at iteration 0"""
    rank, size = comm.rank, comm.size
    d = F.slab_window(shape, kw.get("power_of_two", True), splits, rank)
    vel_h, p_h, valid_h, info_h = single_device(sc, shape, use_old_pressure=False, **kw)
    t, valid, info = slab_call(comm, splits, shape, sc, d, use_old_pressure=False, **kw)
    for a, ref in enumerate(faces(valid_h, d)):
        assert np.array_equal(valid[a].cpu().numpy(), ref), (what, a)
    for key in ("liquid_cells", "mg_levels", "offset", "expanded"):
        assert info[key] == info_h[key], (what, key, info[key], info_h[key])
    assert info["outcome"] == 0 and info_h["outcome"] == 0, (what, info, info_h)
    assert abs(info["iterations"] - info_h["iterations"]) <= 1, (what, info["iterations"], info_h["iterations"])
    p_all = np.concatenate(all_ranks(t["pressure"].cpu().numpy()))
    perr = rel_l2(p_all, p_h)
    assert perr < perr_bound, (what, perr)
    assert info["divergence_max"] < 2e-4 * rhs_max, (what, info["divergence_max"], rhs_max)
    reports = all_ranks((info["divergence_sum"], info["divergence_max"], info["liquid_cells"], info["surface_pressure_max"], info["iterations"]))
    assert all(r == reports[0] for r in reports), (what, reports)
    planes = all_ranks((t["velocity"][2][0].cpu().numpy(), t["velocity"][2][-1].cpu().numpy()))
    for r in range(size - 1):  # rank r's last z-face plane is rank r + 1's first
        assert np.array_equal(planes[r][1], planes[r + 1][0]), (what, r)
    uerr = 0.0
    for a in range(3):  # (the bound tests/test_fields.py puts on the device passes against the host-array call)
        u_all = np.concatenate(all_ranks(t["velocity"][a][:d.c1 - d.c0].cpu().numpy()))
        err = float(np.abs(u_all - vel_h[a][:shape[0]]).max())
        assert err < 1e-6 * max(1.0, np.abs(vel_h[a]).max()), (what, a, err)
        uerr = max(uerr, err)
    # warm start from the answer: CG leaves at its first test on every rank
    _, _, info2 = slab_call(comm, splits, shape, sc, d, pressure=p_all, use_old_pressure=True, **dict(kw, tolerance=1e-5))
    assert info2["iterations"] == 0 and info2["outcome"] == 2, (what, info2)
    if rank == 0:
        print(f"{what}: {info['iterations']} it (single device {info_h['iterations']}), pressure rel_l2 {perr:.1e}, velocity max diff {uerr:.1e}, "
              f"divergence max {info['divergence_max']:.2e} (rhs max {rhs_max:.2e}), total {info['total_ms']:.0f} ms", flush=True)
    return info, info_h


def scene_rhs_max(sc, shape, p2, surface_scale=None):
    """max |rhs| of the whole grid's system (with the surface term when `surface_scale` is given), its material labels, the offset"""
    eshape, offset, _ = G.expanded_layout(shape, 0, power_of_two=p2)
    cw, phi = [dev(a) for a in sc["cut_weights"]], dev(sc["liquid_phi"])
    mat = F.buildMaterialCellLabels(phi, dev(sc["solid_phi"]), cw)
    sv = [dev(a) for a in sc["solid_velocity"]] if sc.get("solid_velocity") is not None else None
    rhs = F.buildRHS(mat, [dev(a) for a in sc["velocity"]], cw, eshape, offset, sv)
    if surface_scale is not None:
        _, weights = F.buildMGDomain(mat, cw, phi, F.buildValidFaces(mat, cw), eshape, offset)
        F.addSurfacePressureToRHS(rhs, weights, phi, mat, F.buildSurfacePressure(phi, mat, surface_scale), offset)
    return float(rhs.abs().max().item()), mat.cpu().numpy(), offset


def onecall_mode():
    comm = TorchDistComm()
    splits = CUTS[comm.size]
    for solid in (False, True):
        sc = D.projection_scene(SHAPE, with_solid_velocity=solid)
        for p2 in (False, True):
            rhs_max, material, offset = scene_rhs_max(sc, SHAPE, p2)
            la, _ = cut_faces(material, sc["cut_weights"], splits, offset)
            assert la >= 1, "no liquid-air face on a cut"
            for gs in (False, True):
                kw = {"use_gauss_seidel": gs, "power_of_two": p2, "tolerance": 1e-6, "max_iterations": 300}
                check_against_single(f"onecall gs={gs} power_of_two={p2} solid_velocity={solid}", comm, splits, SHAPE, sc, rhs_max, kw)


# ---- 4. options ------------------------------------------------------------------------------------------------------------------
def sealed_scene(shape):
    """tests/test_enclosed_liquid.py::test_fields_sealed_box, "full": a closed box filled with liquid, no air anywhere; with solid
    velocities on the closed walls, so that the right-hand side has a mean to remove"""
    sc = D.projection_scene(shape, seed=3, with_solid_velocity=True)
    dx = sc["dx"]
    cw = [np.where(c > 0, 1.0, 0.0).astype(np.float32) for c in sc["cut_weights"]]
    for a in range(3):
        sl = [slice(None)] * 3
        sl[2 - a] = slice(1, -1)
        cw[a][tuple(sl)] = 1.0
    return {"liquid_phi": np.full(shape, -dx, dtype=np.float32), "solid_phi": np.full(shape, -dx, dtype=np.float32), "cut_weights": cw,
            "velocity": sc["velocity"], "solid_velocity": sc["solid_velocity"]}


def options_mode():
    from test_surface_tension import N, S_DROP, _sigma_for, droplet

    comm = TorchDistComm()
    rank, size = comm.rank, comm.size
    # enclosed liquid: a sealed box cut by the slabs
    shape = (64, 48, 48)
    lay = F.projection_slab_layout(shape, False, size, False)
    sc = sealed_scene(shape)
    o = G.default_options()
    o.enclosed_liquid = 1
    kw = {"use_gauss_seidel": False, "power_of_two": False, "tolerance": 1e-6, "max_iterations": 300, "options": o}
    _, _, _, info_h = single_device(sc, shape, use_old_pressure=False, **kw)
    d = F.slab_window(shape, False, lay["splits"], rank)
    t, _, info = slab_call(comm, lay["splits"], shape, sc, d, use_old_pressure=False, **kw)
    assert info_h["enclosed_components"] == 1 and info["enclosed_components"] == 1, (info, info_h)
    assert info_h["rhs_mean_removed_max"] > 1e-4, info_h  # (a mean worth the name, not round-off)
    # (the same rhs bits summed in fp64 in another order)
    assert abs(info["rhs_mean_removed_max"] - info_h["rhs_mean_removed_max"]) <= 1e-9 * info_h["rhs_mean_removed_max"], (info, info_h)
    assert info["outcome"] == 0 and abs(info["iterations"] - info_h["iterations"]) <= 1, (info, info_h)
    assert all(r == (info["enclosed_components"], info["rhs_mean_removed_max"]) for r in all_ranks((info["enclosed_components"], info["rhs_mean_removed_max"])))
    if rank == 0:
        print(f"enclosed: cuts {lay['splits']}, {info['iterations']} it (single device {info_h['iterations']}), mean removed {info['rhs_mean_removed_max']:.6e}", flush=True)
    # surface tension: the static sphere of tests/test_surface_tension.py, its centre on the cut
    phi, solid, cw, vel = droplet()
    shape = (N, N, N)
    sc = {"liquid_phi": phi, "solid_phi": solid, "cut_weights": cw, "velocity": vel, "solid_velocity": None}
    _, offset, _ = G.expanded_layout(shape, 0, power_of_two=False)
    lay = F.projection_slab_layout(shape, False, size, False)
    assert lay["splits"][size // 2] - offset == N // 2, lay  # (the cut through the sphere's centre)
    kw = dict(_sigma_for(S_DROP), use_gauss_seidel=True, power_of_two=False, tolerance=1e-6, max_iterations=500)
    rhs_max, material, _ = scene_rhs_max(sc, shape, False, surface_scale=S_DROP)
    below, above = material[N // 2 - 1], material[N // 2]  # (the planes on either side of the cut: the sphere's surface crosses it)
    assert all((q == LIQUID).any() and (q == AIR).any() for q in (below, above)) and rhs_max > 0, rhs_max
    info, info_h = check_against_single("surface tension", comm, lay["splits"], shape, sc, rhs_max, kw)
    assert info_h["surface_pressure_max"] > 0
    assert abs(info["surface_pressure_max"] - info_h["surface_pressure_max"]) <= 1e-6 * info_h["surface_pressure_max"], (info, info_h)
    # a caller's surface-pressure field
    rng = np.random.default_rng(3)
    field = (0.2 + 0.1 * rng.random(shape)).astype(np.float32)
    kw = {"use_gauss_seidel": True, "power_of_two": False, "tolerance": 1e-6, "max_iterations": 500}
    d = F.slab_window(shape, False, lay["splits"], rank)
    _, p_h, _, info_h = single_device(sc, shape, use_old_pressure=False, surface_pressure=field, **kw)
    t = window_tensors(sc, d)
    _, info = F.project_free_surface_slab(comm, lay["splits"], shape, t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"], None,
                                          use_old_pressure=False, surface_pressure=dev(cell(field, d)), **kw)
    perr = rel_l2(np.concatenate(all_ranks(t["pressure"].cpu().numpy())), p_h)
    assert info["outcome"] == 0 and abs(info["iterations"] - info_h["iterations"]) <= 1 and perr < 1e-4, (info, info_h, perr)
    assert abs(info["surface_pressure_max"] - info_h["surface_pressure_max"]) <= 1e-6 * info_h["surface_pressure_max"], (info, info_h)
    if rank == 0:
        print(f"caller's surface pressure: {info['iterations']} it, pressure rel_l2 {perr:.1e}, p_G max {info['surface_pressure_max']:.5f}", flush=True)


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
def edges_mode():
    comm = TorchDistComm()
    rank, size = comm.rank, comm.size
    splits = CUTS[size]
    sc = D.projection_scene(SHAPE, with_solid_velocity=True)
    d = F.slab_window(SHAPE, True, splits, rank)
    kw = {"use_gauss_seidel": False, "power_of_two": True, "tolerance": 1e-6, "max_iterations": 300}
    # no liquid anywhere: valid faces and zero pressure are published, velocities stay
    air = dict(sc, liquid_phi=np.full(SHAPE, 1.0, dtype=np.float32))
    _, _, valid_h, info_h = single_device(air, SHAPE, pressure=np.full(SHAPE, 7.0, np.float32), use_old_pressure=True, **kw)
    t, valid, info = slab_call(comm, splits, SHAPE, air, d, pressure=np.full(SHAPE, 7.0, np.float32), use_old_pressure=True, **kw)
    assert info["liquid_cells"] == 0 and info["iterations"] == 0 and info["outcome"] == 1 and info_h["outcome"] == 1, (info, info_h)
    assert (t["pressure"] == 0).all()
    for a, ref in enumerate(faces(valid_h, d)):
        assert np.array_equal(valid[a].cpu().numpy(), ref)
        assert np.array_equal(t["velocity"][a].cpu().numpy(), faces(sc["velocity"], d)[a])
    # liquid on rank 0 only: the pool ends below the first cut
    low = dict(sc, liquid_phi=(sc["liquid_phi"] + (SHAPE[0] * 0.5) * sc["dx"]).astype(np.float32))
    rhs_max, material, offset = scene_rhs_max(low, SHAPE, True)
    per_rank = [int((material[max(s - offset, 0):max(splits[r + 1] - offset, 0)] == LIQUID).sum()) for r, s in enumerate(splits[:-1])]
    assert per_rank[0] > 0 and not any(per_rank[1:]), per_rank
    check_against_single("liquid on rank 0 only", comm, splits, SHAPE, low, rhs_max, kw)
    # one rank passes two of the three solid velocities: every rank gets the same error, none hangs
    t = window_tensors(sc, d)
    sv = list(t["solid_velocity"])
    if rank == size - 1:
        sv[1] = None
    try:
        F.project_free_surface_slab(comm, splits, SHAPE, t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"], sv,
                                    use_old_pressure=False, **kw)
    except G.MgpsError as e:
        assert e.status == 1, str(e)
        assert ("solid velocities" in str(e)) == (rank == size - 1) and (rank == size - 1 or f"rank {size - 1} failed" in str(e)), str(e)
    else:
        raise AssertionError("two of three solid velocities were accepted")
    assert np.array_equal(t["velocity"][2].cpu().numpy(), zface(sc["velocity"][2], d))  # (nothing was touched)
    # a transport without gatherv: refused on every rank, before any device work
    bare = TorchDistComm()
    bare.struct.gatherv = type(bare.struct.gatherv)()  # (NULL)
    try:
        F.project_free_surface_slab(bare, splits, SHAPE, t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"], t["solid_velocity"],
                                    use_old_pressure=False, **kw)
    except G.MgpsError as e:
        assert e.status == 1 and "gatherv" in str(e), str(e)
    else:
        raise AssertionError("a transport without gatherv was accepted")
    # cuts that leave a rank without base planes: refused on every rank (the even cut of a grid with much padding)
    try:
        F.slab_window((48, 48, 48), True, [0, 32, 64, 96, 128], rank)
    except G.MgpsError as e:
        assert e.status == 1 and "owns no plane" in str(e), str(e)
    else:
        raise AssertionError("a rank without base planes was accepted")


# ---- 5b. a rank's own refusal travels in the first agreement ----------------------------------------------------------------------
def missing_mode():
    """rank 1 comes with two of its three solid velocities: its status travels in the agreement on the arguments, and both ranks return
    MGPS_ERR_INVALID_ARGUMENT -- rank 1 with its own message, rank 0 naming rank 1 and the place.  The same transport then serves a
    complete call that agrees with the single-device call: nobody was left behind in a collective"""
    comm = TorchDistComm()
    rank = comm.rank
    assert comm.size == 2
    splits = CUTS[2]
    sc = D.projection_scene(SHAPE, with_solid_velocity=True)
    d = F.slab_window(SHAPE, True, splits, rank)
    kw = {"use_gauss_seidel": False, "power_of_two": True, "tolerance": 1e-6, "max_iterations": 300}
    t = window_tensors(sc, d)
    sv = list(t["solid_velocity"])
    if rank == 1:
        sv[1] = None
    try:
        F.project_free_surface_slab(comm, splits, SHAPE, t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"], sv,
                                    use_old_pressure=False, **kw)
    except G.MgpsError as e:
        assert e.status == 1, (rank, e.status, str(e))
        assert ("all three or none" if rank == 1 else "rank 1 failed (arguments, status 1)") in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: two of three solid velocities on rank 1 went unnoticed")
    for a, ref in enumerate(faces(sc["velocity"], d)):
        assert np.array_equal(t["velocity"][a].cpu().numpy(), ref), a  # (nothing was touched)
    rhs_max, _, _ = scene_rhs_max(sc, SHAPE, True)
    check_against_single("after a refusal", comm, splits, SHAPE, sc, rhs_max, kw)


# ---- 6. one rank over RCCL: the device-resident projection ------------------------------------------------------------------------
def one_mode():
    comm = RcclComm()
    try:
        assert comm.size == 1
        sc = D.projection_scene(SHAPE, with_solid_velocity=True)
        for p2 in (False, True):
            rhs_max, _, _ = scene_rhs_max(sc, SHAPE, p2)
            for gs in (False, True):
                kw = {"use_gauss_seidel": gs, "power_of_two": p2, "tolerance": 1e-6, "max_iterations": 300}
                check_against_single(f"one rank gs={gs} power_of_two={p2}", comm, CUTS[1], SHAPE, sc, rhs_max, kw)
    finally:
        comm.close()


if __name__ == "__main__":
    worker_main({"passes": passes_mode, "onecall": onecall_mode, "options": options_mode, "edges": edges_mode, "missing": missing_mode, "one": one_mode})
