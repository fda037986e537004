"""Worker of tests/test_distributed.py: run under torch.distributed.run with 2+ ranks.

mode "gpu":  every rank drives a SlabSolver on cuda:0 (ranks share the GPU) over TorchDistComm/gloo
             and compares V-cycle / operators / MG-PCG with a whole-grid solver on the same device.
Prints "WORKER_OK <rank>" on success.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def scene_domain(gz, levels, eshape):
    """labels / weights of D.projection_scene through the oracle's field passes (tests/test_fields.py)"""
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from oracle.mg_oracle import FieldsOracle, Oracle

    shape = (gz, eshape[1] - 16, eshape[2] - 16)
    sc = D.projection_scene(shape, seed=int(os.environ.get("MGPS_SCENE_SEED", "3")), dtype=np.float64, randomize="MGPS_SCENE_SEED" in os.environ)
    fo = FieldsOracle()
    material = fo.material_labels(sc["liquid_phi"] - 0.2 * gz * sc["dx"], sc["solid_phi"], sc["cut_weights"])  # raise the fill level
    valid = fo.valid_faces(material, sc["cut_weights"])
    eshape2, offset, lev = G.expanded_layout(shape, levels, power_of_two=False)
    assert tuple(eshape2) == tuple(eshape) and lev == levels
    lab = fo.domain_labels(material, eshape, offset)
    w = fo.boundary_weights(sc["cut_weights"], sc["liquid_phi"] - 0.2 * gz * sc["dx"], valid, material, eshape, offset)
    Oracle().set_boundary_labels(lab, w)
    return lab.astype(np.uint8), [a.astype(np.float32) for a in w], offset, lev, sc["dx"]


def compare_with_host_builder(slab, lab, slab_w, lev, use_gs, opt, what):
    """The rank's own lists as the device built them (createSlabOnDevice: cut out of the lists of its label buffer) against the
    host builder's (options.host_setup = 1: buildSlabLevel over the global hierarchy): codes, band list with diagonals and rows,
    activity runs, plane blocks, Gauss-Seidel tiles -- array_equal where the rank's planes start on a tile of the whole grid
    (the band list is in tile order), equal as sets otherwise."""
    import ctypes

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    oh = G.default_options()
    ctypes.memmove(ctypes.addressof(oh), ctypes.addressof(opt), ctypes.sizeof(opt))
    oh.host_setup = 1
    host = SlabSolver(lab, slab_w, lev, use_gs, TorchDistComm(), device=0, options=oh, splits=slab.splits)
    try:
        assert host.ghost_planes == 1 and host.distributed_levels == slab.distributed_levels
        for l in range(slab.distributed_levels):
            z0, _ = slab.slab_range(l)
            aligned = z0 % 16 == 0
            assert np.array_equal(slab.level_array(l, "codes"), host.level_array(l, "codes")), (what, l, "codes")
            # (the host builder puts the runs next to a cut first and pads both parts: the same runs in another order)
            cd, ch = slab.level_array(l, "chunks"), host.level_array(l, "chunks")
            assert np.array_equal(np.sort(cd[cd >= 0]), np.sort(ch[ch >= 0])), (what, l, "chunks")
            # (plane blocks: the device list also holds the blocks next to a cut whose only active cells lie across it)
            assert np.isin(host.level_array(l, "plane_blocks"), slab.level_array(l, "plane_blocks")).all(), (what, l, "plane_blocks")
            bd, bh = slab.level_array(l, "band"), host.level_array(l, "band")
            dd, dh = slab.level_array(l, "band_diag"), host.level_array(l, "band_diag")
            rd, rh = slab.level_array(l, "rows").reshape(7, -1), host.level_array(l, "rows").reshape(7, -1)
            assert bd.size == bh.size and rd.shape == rh.shape, (what, l, bd.size, bh.size, rd.shape, rh.shape)
            ngen = rd.shape[1]
            if aligned:
                assert np.array_equal(bd, bh) and np.array_equal(dd, dh) and np.array_equal(rd, rh), (what, l)
                for name in ("pure_even", "pure_odd", "mixed_even", "mixed_odd", "tile_bnd_start"):
                    assert np.array_equal(slab.level_array(l, name), host.level_array(l, name)), (what, l, name)
            else:  # the same cells with the same rows, general cells first
                for a, b2 in ((0, ngen), (ngen, bd.size)):
                    od, oh2 = np.argsort(bd[a:b2], kind="stable"), np.argsort(bh[a:b2], kind="stable")
                    assert np.array_equal(bd[a:b2][od], bh[a:b2][oh2]) and np.array_equal(dd[a:b2][od], dh[a:b2][oh2]), (what, l)
                    if a == 0:
                        assert np.array_equal(rd[:, od], rh[:, oh2]), (what, l)
    finally:
        host.close()


def gpu_mode():
    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    # liquid must straddle every slab cut, otherwise the exchanges carry nothing
    for kind, g, levels, shape in (("solid", 96, 5, (128, 128, 128)), ("simple", 40 if size == 2 else 48, 4, (64, 64, 64)),
                                   ("scene", 48, 4, (64, 64, 64)), ("random", 0, 3, (64, 64, 96))):
        if kind == "scene":  # a seeded projection scene (wavy free surface, cut-cell box): general cells near the cuts
            lab, w, off, lev, dx = scene_domain(g, levels, shape)
        elif kind == "random":  # blobs of every label, fractional weights everywhere (tests/test_device_setup.py): general cells in every group across the cuts
            from test_device_setup import random_domain

            lab, w = random_domain(shape, levels, int(os.environ.get("MGPS_DIST_SEED", "4")), closed_faces=False)  # (MGPS_DIST_SEED: a one-off sweep over other seeds)
            off, lev, dx = 0, levels, 1.0 / shape[2]
        else:
            lab, w, off, lev, dx = make_domain(kind, g, levels, shape)
        nz = lab.shape[0]
        cuts = [D.active_mask(lab[c - 1 : c + 1]).any() for c in range(nz // size, nz, nz // size)]
        assert all(cuts) or (kind in ("scene", "random") and any(cuts))
        nzl = nz // size
        z0, z1 = rank * nzl, (rank + 1) * nzl
        slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
        b_glob = D.random_rhs(lab, dx)
        counts = {}
        for use_gs, deep in ((False, 1), (False, 0), (True, 1), (True, 0)):
            comm = TorchDistComm()
            opt = G.default_options()
            opt.min_cells_per_rank = 0  # small test grids: keep every level that can be cut distributed
            opt.deep_band_halo = deep   # one exchange per band stage / one per band pass
            slab = SlabSolver(lab, slab_w, lev, use_gs, comm, device=0, options=opt)
            whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0)
            assert slab.slab_range(0) == (z0, z1), (slab.slab_range(0), z0, z1)
            assert slab.getMGLevels() == whole.getMGLevels()
            assert 1 <= slab.distributed_levels < slab.getMGLevels()
            bw = whole.to_device(b_glob)
            bs = slab.to_device(b_glob[z0:z1])
            # operators across the cut
            xw, xs = whole.to_device(b_glob * 3.0), slab.to_device(b_glob[z0:z1] * 3.0)
            yw, ys = whole.new_grid(), slab.new_grid()
            whole.applyPoissonMatrix(yw, xw)
            slab.applyPoissonMatrix(ys, xs)
            assert np.array_equal(slab.gather_global(ys), yw.cpu().numpy())
            assert abs(slab.dotProduct(xs, bs) - whole.dotProduct(xw, bw)) <= 1e-12 * abs(whole.dotProduct(xw, bw))
            assert slab.infNorm(xs) == whole.infNorm(xw)
            # V-cycles: same arithmetic per cell, so the slab run reproduces the single-GPU run
            xw, xs = whole.new_grid(), slab.new_grid()
            for it in range(2):
                whole.applyVCycle(xw, bw, it > 0)
                slab.applyVCycle(xs, bs, it > 0)
                err = rel_l2(slab.gather_global(xs), xw.cpu().numpy())
                assert err < 1e-6, (kind, use_gs, it, err)
            # MG-PCG
            bd = D.delta_rhs(lab, g, off, dx) if kind not in ("scene", "random") else D.random_rhs(lab, dx, seed=9)
            xw, xs = whole.new_grid(), slab.new_grid()
            sw = whole.solveGeometricConjugateGradient(xw, whole.to_device(bd), 1e-5, 200, True)
            ss = slab.solveGeometricConjugateGradient(xs, slab.to_device(bd[z0:z1]), 1e-5, 200, True)
            # (other seeds of the random-label domain, MGPS_DIST_SEED: blobs of labels and weights do not promise a definite operator --
            # the fp64 oracle's MG-PCG grows without bound on seeds 10 and 12 as well; there both solvers must fail alike)
            definite = not (kind == "random" and sw["outcome"] != "converged")
            if not definite:
                assert ss["outcome"] == sw["outcome"], (ss, sw)
            else:
                assert ss["outcome"] == "converged" and abs(ss["iterations"] - sw["iterations"]) <= 1, (ss, sw)
                assert rel_l2(slab.gather_global(xs), xw.cpu().numpy()) < 1e-4
            # alpha and beta stayed on the device: the CG scalars were summed through the transport's device all-reduce
            assert comm.device_allreduces >= 3 * ss["iterations"], (comm.device_allreduces, ss)
            counts[(use_gs, deep)] = comm.exchanges
            # the box form of a cut level's band stage (deep = 1) sends the boundary plane straight from the grid (mgps_comm::exchange2), only the lists packed
            assert (comm.segmented_exchanges > 0) == (deep == 1), (deep, comm.segmented_exchanges)
            assert slab.ghost_planes == 5 and all(slab.band_stage_form(l) == ("boxes" if deep == 1 else "passes") for l in range(slab.distributed_levels))
            if deep == 1 and not use_gs:
                compare_with_host_builder(slab, lab, slab_w, lev, use_gs, opt, (kind, size))
            if deep == 1 and definite:  # the CG vectors in fp64 (options.pcg_fp64_vectors): their ghost planes travel as doubles
                o64 = G.default_options()
                o64.min_cells_per_rank, o64.pcg_fp64_vectors = 0, 1
                slab64 = SlabSolver(lab, slab_w, lev, use_gs, TorchDistComm(), device=0, options=o64)
                ow = G.default_options()
                ow.pcg_fp64_vectors = 1
                whole64 = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0, options=ow)
                xw, xs = whole64.new_grid(), slab64.new_grid()
                sw = whole64.solveGeometricConjugateGradient(xw, whole64.to_device(bd), 1e-6, 200, True)
                ss = slab64.solveGeometricConjugateGradient(xs, slab64.to_device(bd[z0:z1]), 1e-6, 200, True)
                assert ss["outcome"] == "converged" and abs(ss["iterations"] - sw["iterations"]) <= 1, (ss, sw)
                assert ss["rel_residual_recomputed"] < 1e-6 and rel_l2(slab64.gather_global(xs), xw.cpu().numpy()) < 1e-5
                slab64.close()
                whole64.close()
                # the slab's face weights handed over on the device (mgps_create_slab_device_weights: rows evaluated by a kernel,
                # nothing of the weights crosses PCIe): the same solver bit for bit
                slabd = SlabSolver(lab, [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in slab_w], lev, use_gs,
                                   TorchDistComm(), device=0, options=opt)
                xa, xb = slab.new_grid(), slabd.new_grid()
                slab.applyVCycle(xa, bs, False)
                slabd.applyVCycle(xb, slabd.to_device(b_glob[z0:z1]), False)
                assert torch.equal(xa, xb), (kind, use_gs, "device weights")
                slabd.close()
            if rank == 0:
                print(f"  {kind} gs={use_gs} deep={deep}: D={slab.distributed_levels} exchanges={comm.exchanges} "
                      f"({comm.bytes_sent / 1e6:.1f} MB sent) pcg it {ss['iterations']}", flush=True)
            slab.close()
            whole.close()
            dist.barrier()
        # the one-exchange band stage must actually cut exchanges (fine levels with general BOUNDARY cells included:
        # the ranks trade the rows of the cells next to the cuts at set-up)
        assert counts[(False, 1)] < 0.6 * counts[(False, 0)] and counts[(True, 1)] < 0.7 * counts[(True, 0)], counts


def band_options_mode():
    """options.band_width / band_iterations / jacobi_weight away from 3 / 3 / 2/3 on cut levels, random-label domain of gpu_mode
    (general cells in every group across the cuts): (4, 4, 0.5) -- depth 4 fills the 5 ghost planes of the grids, a box region
    reaches depth + 1 planes past its owned box (on level 1; the fine level cannot form depth-4 boxes among its general cells and
    runs pass by pass on every rank) -- and (1, 1, 0.8), box form (deep_band_halo = 1) and an exchange per pass (0),
    both smoothers, against the whole-grid solver at the same options (which tests/test_band_options.py holds to the oracle), to
    gpu_mode's bounds.  Then (8, 4, 2/3): the widest label reach the options allow, (8 - 1) + (4 + 2) + 1 = 14 of 16 planes."""
    import ctypes as C

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm
    from test_device_setup import random_domain

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    shape, lev = (64, 64, 96), 3
    lab, w = random_domain(shape, lev, 4, closed_faces=False)
    dx = 1.0 / shape[2]
    nz = lab.shape[0]
    nzl = nz // size
    z0, z1 = rank * nzl, (rank + 1) * nzl
    assert any(D.active_mask(lab[c - 1 : c + 1]).any() for c in range(nzl, nz, nzl))
    slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
    b_glob, b_pcg = D.random_rhs(lab, dx), D.random_rhs(lab, dx, seed=9)

    def options(bw, bi, om, slab_run, deep=1):
        o = G.default_options()
        o.band_width, o.band_iterations, o.jacobi_weight = bw, bi, om
        if slab_run:
            o.min_cells_per_rank, o.deep_band_halo = 0, deep
        return o

    for bw, bi, om in ((4, 4, 0.5), (1, 1, 0.8), (8, 4, 2.0 / 3.0)):
        widest = bw == 8
        for use_gs, deep in ((False, 1),) if widest else ((False, 1), (False, 0), (True, 1), (True, 0)):
            opt = options(bw, bi, om, True, deep)
            comm = TorchDistComm()
            slab = SlabSolver(lab, slab_w, lev, use_gs, comm, device=0, options=opt)
            whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0, options=options(bw, bi, om, False))
            assert slab.slab_range(0) == (z0, z1) and 1 <= slab.distributed_levels < slab.getMGLevels() == whole.getMGLevels()
            # the form of a cut level: the whole-grid solver's -- boxes, but for the fine level at depth 4: among this domain's general
            # cells a box of one cell still holds more than kBoxMaxGeneral of them (tests/test_band_options.py: _boxes_expected), and
            # the ranks agree on pass by pass there; level 1 (unit weights) takes the depth-4 boxes with their 5 ghost planes
            wform = C.c_int(-1)
            for l in range(slab.distributed_levels):
                G.lib().mgps_band_stage_form(whole.h, l, C.byref(wform))
                assert wform.value == (0 if bi == 4 and l == 0 else 1), (bw, bi, l, wform.value)
                assert slab.band_stage_form(l) == ("boxes" if deep == 1 and wform.value == 1 else "passes"), (bw, bi, l, deep)
            assert slab.ghost_planes == 5 and (bi != 4 or slab.distributed_levels >= 2)
            boxed = deep == 1 and any(slab.band_stage_form(l) == "boxes" for l in range(slab.distributed_levels))
            bw_, bs = whole.to_device(b_glob), slab.to_device(b_glob[z0:z1])
            xw, xs = whole.new_grid(), slab.new_grid()
            for it in range(2):
                whole.applyVCycle(xw, bw_, it > 0)
                slab.applyVCycle(xs, bs, it > 0)
                err = rel_l2(slab.gather_global(xs), xw.cpu().numpy())
                assert float(xw.abs().max()) > 0 and err < 1e-6, (bw, bi, om, use_gs, deep, it, err)
            assert (comm.segmented_exchanges > 0) == boxed, (deep, comm.segmented_exchanges)
            if not widest:
                xw, xs = whole.new_grid(), slab.new_grid()
                sw = whole.solveGeometricConjugateGradient(xw, whole.to_device(b_pcg), 1e-5, 200, True)
                ss = slab.solveGeometricConjugateGradient(xs, slab.to_device(b_pcg[z0:z1]), 1e-5, 200, True)
                assert sw["outcome"] == ss["outcome"] == "converged" and abs(ss["iterations"] - sw["iterations"]) <= 1, (ss, sw)
                assert rel_l2(slab.gather_global(xs), xw.cpu().numpy()) < 1e-4
            if deep == 1 and not use_gs:
                compare_with_host_builder(slab, lab, slab_w, lev, use_gs, opt, ("random", size, bw, bi))
            if rank == 0:
                print(f"  band options ({bw}, {bi}, {om:.2f}) gs={use_gs} deep={deep}: D={slab.distributed_levels} exchanges={comm.exchanges}"
                      + ("" if widest else f" pcg it {ss['iterations']} (whole grid {sw['iterations']})"), flush=True)
            slab.close()
            whole.close()
            dist.barrier()


def plane_mode():
    """The plane-marching sweep (stencilPlaneKernel, the 1024^3 kernel) on cut slabs: its ghostLo / ghostHi reads of the
    plane below the first and above the last owned plane.  options.stencil_path = 2 forces it onto a 264 x 40 x 32 (two ranks) or 272 x 72 x 64 (four ranks, four levels)
    free-surface + cut-cell grid; slab runs must reproduce the whole-grid run of the same kernel (A.x bit for bit)."""
    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    # (four levels on the larger grid: with three its coarsest level has ~10 000 unknowns, and factorising that -- rank 0's tail on
    # the host, the whole-grid solver on every rank -- took 70 of this test's 75 seconds)
    g, levels = (24, 3) if size == 2 else (48, 4)
    shape = (32, 40, 264) if size == 2 else (64, 72, 272)
    lab, w, off, lev, dx = make_domain("widesolid", g, levels, shape)
    nz = lab.shape[0]
    nzl = nz // size
    z0, z1 = rank * nzl, (rank + 1) * nzl
    assert all(D.active_mask(lab[c - 1 : c + 1]).any() for c in range(nzl, nz, nzl))
    slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
    b_glob = D.random_rhs(lab, dx)
    import time
    for use_gs, deep in ((False, 1), (False, 0)):
        t0 = time.time()
        opt = G.default_options()
        opt.min_cells_per_rank, opt.deep_band_halo, opt.stencil_path = 0, deep, 2
        ow = G.default_options()
        ow.stencil_path = 2
        slab = SlabSolver(lab, slab_w, lev, use_gs, TorchDistComm(), device=0, options=opt)
        whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0, options=ow)
        assert slab.stencil_kernel(0) == "plane" and whole.stencil_kernel(0) == "plane"
        if os.environ.get("MGPS_EXPECT_FUSED_RR") == "1":  # (the residual + restriction pair on the cut fine level)
            assert slab.residual_restrict_fused(0) and whole.residual_restrict_fused(0)
        t1 = time.time()
        bw, bs = whole.to_device(b_glob), slab.to_device(b_glob[z0:z1])
        xw, xs = whole.to_device(b_glob * 3.0), slab.to_device(b_glob[z0:z1] * 3.0)
        yw, ys = whole.new_grid(), slab.new_grid()
        whole.applyPoissonMatrix(yw, xw)
        slab.applyPoissonMatrix(ys, xs)
        assert np.array_equal(slab.gather_global(ys), yw.cpu().numpy())
        whole.computePoissonResidual(yw, xw, bw)
        slab.computePoissonResidual(ys, xs, bs)
        assert np.array_equal(slab.gather_global(ys), yw.cpu().numpy())
        whole.jacobiPoissonSmoother(xw, bw)
        slab.jacobiPoissonSmoother(xs, bs)
        assert np.array_equal(slab.gather_global(xs), xw.cpu().numpy())
        xw, xs = whole.new_grid(), slab.new_grid()
        for it in range(2):
            whole.applyVCycle(xw, bw, it > 0)
            slab.applyVCycle(xs, bs, it > 0)
            err = rel_l2(slab.gather_global(xs), xw.cpu().numpy())
            # (the residual + restriction pair adds a coarse cell's terms along z first: with it the last bits differ where general cells meet a cut)
            assert err < (2e-6 if os.environ.get("MGPS_EXPECT_FUSED_RR") == "1" else 1e-6), (deep, it, err)
        t2 = time.time()
        xw, xs = whole.new_grid(), slab.new_grid()
        sw = whole.solveGeometricConjugateGradient(xw, bw, 1e-5, 200, True)  # A.p + <p, A p> from the DOT variant on the whole grid
        ss = slab.solveGeometricConjugateGradient(xs, bs, 1e-5, 200, True)
        assert ss["outcome"] == "converged" and abs(ss["iterations"] - sw["iterations"]) <= 1, (ss, sw)
        assert rel_l2(slab.gather_global(xs), xw.cpu().numpy()) < 1e-4
        if rank == 0:
            print(f"  plane sweep on {size} slabs, deep={deep}: D={slab.distributed_levels}, pcg it {ss['iterations']}; set-up {t1 - t0:.1f} s, "
                  f"operators + cycles {t2 - t1:.1f} s, pcg {time.time() - t2:.1f} s, exchanges {slab.exchange_count}", flush=True)
        slab.close()
        whole.close()
        dist.barrier()


def balanced_mode():
    """Slabs of different sizes (mgps_slab_partition / explicit cuts): the liquid sits at the low end of a long grid, the
    balanced cuts give the ranks equal active cells instead of equal planes, the collapse gathers / scatters shares of
    different sizes (gatherv / scatterv).  Must reproduce the whole-grid solver like the even cut does."""
    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm, slab_partition

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    if size == 2:
        lab, w, off, lev, dx = make_domain("simple", 40, 4, (128, 64, 64))
        min_cells = 10000
    else:
        bl, bw, dx = D.build_complex_domain((184, 48, 48), dtype=np.float32)
        lab, w, off, lev = D.expand_domain(bl, bw, levels=4, solver_shape=(256, 64, 64))
        min_cells = 10000
    # (min_cells_per_rank = 10000 keeps two levels distributed on these grids: every rank then needs 32 fine planes, the rest is free)
    opt = G.default_options()
    opt.min_cells_per_rank = min_cells
    nz = lab.shape[0]
    b_glob = D.random_rhs(lab, dx)
    cases = [(False, slab_partition(lab, lev, size, False, opt))]
    if size == 2:
        cases.append((True, [0, 32, nz]))  # Gauss-Seidel with the caller's own cuts (multiples of 16 on both distributed levels)
    assert slab_partition(lab, lev, size, True, opt) == [nz // size * r for r in range(size + 1)]  # GS: the even cut
    for use_gs, cuts in cases:
        planes = [cuts[r + 1] - cuts[r] for r in range(size)]
        assert len(set(planes)) > 1, cuts  # really uneven
        load = lambda a, c: int(D.active_mask(lab[a:c]).sum()) + 6 * int((lab[a:c] == 3).sum())  # noqa: E731  (the partition's load model, box form of the band stage)
        active = [load(cuts[r], cuts[r + 1]) for r in range(size)]
        even = [load(nz // size * r, nz // size * (r + 1)) for r in range(size)]
        assert max(active) < max(even) or use_gs, (active, even)
        z0, z1 = cuts[rank], cuts[rank + 1]
        slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
        for deep in (1, 0):
            o = G.default_options()
            o.min_cells_per_rank, o.deep_band_halo = min_cells, deep
            slab = SlabSolver(lab, slab_w, lev, use_gs, TorchDistComm(), device=0, options=o, splits=cuts)
            whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0)
            assert slab.slab_range(0) == (z0, z1) and slab.distributed_levels == 2, (slab.slab_range(0), slab.distributed_levels)
            bw, bs = whole.to_device(b_glob), slab.to_device(b_glob[z0:z1])
            xw, xs = whole.to_device(b_glob * 3.0), slab.to_device(b_glob[z0:z1] * 3.0)
            yw, ys = whole.new_grid(), slab.new_grid()
            whole.applyPoissonMatrix(yw, xw)
            slab.applyPoissonMatrix(ys, xs)
            assert np.array_equal(slab.gather_global(ys), yw.cpu().numpy())
            assert abs(slab.dotProduct(xs, bs) - whole.dotProduct(xw, bw)) <= 1e-12 * abs(whole.dotProduct(xw, bw))
            xw, xs = whole.new_grid(), slab.new_grid()
            for it in range(2):
                whole.applyVCycle(xw, bw, it > 0)
                slab.applyVCycle(xs, bs, it > 0)
                err = rel_l2(slab.gather_global(xs), xw.cpu().numpy())
                assert err < 1e-6, (use_gs, deep, it, err)
            xw, xs = whole.new_grid(), slab.new_grid()
            sw = whole.solveGeometricConjugateGradient(xw, bw, 1e-5, 200, True)
            ss = slab.solveGeometricConjugateGradient(xs, bs, 1e-5, 200, True)
            assert ss["outcome"] == "converged" and abs(ss["iterations"] - sw["iterations"]) <= 1, (ss, sw)
            assert rel_l2(slab.gather_global(xs), xw.cpu().numpy()) < 1e-4
            if rank == 0:
                print(f"  balanced cuts {cuts} gs={use_gs} deep={deep}: active per rank {active} (even cut {even}), pcg it {ss['iterations']}", flush=True)
            slab.close()
            whole.close()
            dist.barrier()


def violation_mode():
    """Labels that break the BOUNDARY-cell rule (unitTestBoundaryCells) on ONE rank's planes: a BOUNDARY label on a cell deep in the
    liquid, all of whose neighbours are active across faces of weight 1.  Every rank checks its own cells only, so one rank alone
    finds it -- and every rank must come back with an error instead of waiting in a collective for the one that left.
    Device-side set-up (the default) and the host builder with device weights."""
    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    lab, w, off, lev, dx = make_domain("simple", 40 if size == 2 else 48, 4, (64, 64, 64))
    nz = lab.shape[0]
    nzl = nz // size
    bad_rank = size - 1
    # an INTERIOR cell of the bad rank's planes whose six neighbours are INTERIOR too, two planes away from the cut at least
    z0b, z1b = bad_rank * nzl, (bad_rank + 1) * nzl
    inner = lab == 0
    core = inner.copy()
    core[1:-1, 1:-1, 1:-1] &= inner[:-2, 1:-1, 1:-1] & inner[2:, 1:-1, 1:-1] & inner[1:-1, :-2, 1:-1] & inner[1:-1, 2:, 1:-1] & inner[1:-1, 1:-1, :-2] & inner[1:-1, 1:-1, 2:]
    cand = np.argwhere(core[z0b + 2 : z1b - 2])
    assert len(cand) > 0, "the test domain has no INTERIOR cell deep in the last rank's planes"
    k, j, i = (int(v) for v in cand[len(cand) // 2])
    k += z0b + 2
    assert all(lab[k + dk, j + dj, i + di] in (0, 3) for dk, dj, di in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
    lab = lab.copy()
    lab[k, j, i] = 3
    z0, z1 = rank * nzl, (rank + 1) * nzl
    for host_setup, on_device in ((0, False), (0, True), (1, True)):
        slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
        if on_device:
            slab_w = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in slab_w]
        opt = G.default_options()
        opt.min_cells_per_rank, opt.host_setup = 0, host_setup
        try:
            SlabSolver(lab, slab_w, lev, False, TorchDistComm(), device=0, options=opt)
        except Exception as e:
            msg = str(e)
        else:
            raise AssertionError(f"rank {rank}: the constructor accepted labels that break the BOUNDARY-cell rule on rank {bad_rank}")
        # the bad rank names the rule; every other rank learns of it through the set-up all-reduce
        assert ("BOUNDARY-cell rules" if rank == bad_rank else "another rank") in msg, (rank, msg)
        dist.barrier()  # (nobody is stuck in a set-up collective)
        if rank == 0:
            print(f"  violation on rank {bad_rank}, host_setup={host_setup}, device weights={on_device}: rank 0 got '{msg[:90]}'", flush=True)


def interrupt_mode():
    """options.interrupt on slab solvers: the callback answers 1 on rank 1 alone, at its 4th poll.  Slab runs poll at the top of
    every CG iteration only and agree on the answer through an all-reduce (max over the ranks), so every rank must come back
    with MGPS_ERR_INTERRUPTED from the top of iteration 3, after the same number of polls, and the gathered x must be the
    whole-grid solver's solve capped at three iterations (to the bound gpu_mode puts on slab against whole MG-PCG, 1e-4)."""
    import ctypes as C

    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, TorchDistComm

    rank, size = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    lab, w, off, lev, dx = make_domain("simple", 40 if size == 2 else 48, 4, (64, 64, 64))
    nz = lab.shape[0]
    nzl = nz // size
    z0, z1 = rank * nzl, (rank + 1) * nzl
    slab_w = [w[0][z0:z1], w[1][z0:z1], w[2][z0 : z1 + 1]]
    b = D.random_rhs(lab, dx)
    polls = []

    def poll(user):
        polls.append(1)
        return int(rank == 1 and len(polls) >= 4)

    cb = C.CFUNCTYPE(C.c_int, C.c_void_p)(poll)
    for use_gs in (False, True):
        del polls[:]
        opt = G.default_options()
        opt.min_cells_per_rank = 0
        opt.interrupt = C.cast(cb, C.c_void_p)
        slab = SlabSolver(lab, slab_w, lev, use_gs, TorchDistComm(), device=0, options=opt)
        whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0)
        xs = slab.new_grid()
        try:
            slab.solveGeometricConjugateGradient(xs, slab.to_device(b[z0:z1]), 1e-12, 200, True)
        except G.MgpsError as e:
            status, stats = e.status, e.stats
        else:
            raise AssertionError(f"rank {rank}: the solve was not interrupted")
        assert status == 9 and len(polls) == 4, (rank, status, len(polls))
        assert stats["outcome"] == "max_iterations" and stats["iterations"] == 3, (rank, stats)
        seen = [None] * size
        dist.all_gather_object(seen, (status, stats["iterations"], len(polls)))
        assert all(v == seen[0] for v in seen), seen
        xw = whole.new_grid()
        sw = whole.solveGeometricConjugateGradient(xw, whole.to_device(b), 1e-12, 3, True)
        assert sw["outcome"] == "max_iterations" and sw["iterations"] == 3
        err = rel_l2(slab.gather_global(xs), xw.cpu().numpy())
        assert float(xw.abs().max()) > 0 and err < 1e-4, (use_gs, err)
        if rank == 0:
            print(f"  interrupt on rank 1 of {size}, gs={use_gs}: every rank left iteration 3, x {err:.1e} from the whole grid's third iterate", flush=True)
        slab.close()
        whole.close()
        dist.barrier()


def cpu_mode():
    """Slab emulation on the CPU (no GPU involved): tests/slab_emulation.py over gloo vs the
    whole-grid oracle."""
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from oracle.mg_oracle import Oracle
    from slab_emulation import SlabEmulation

    rank, size = dist.get_rank(), dist.get_world_size()
    orc = Oracle()
    orc.set_threads(2)
    # liquid must straddle every slab cut (z = 16, 32, 48), otherwise the exchanges carry nothing
    for kind, g, levels, shape in (("solid", 48, 4, (64, 64, 64)), ("simple", 56, 3, (64, 64, 64))):
        lab, w, off, lev, dx = make_domain(kind, g, levels, shape, dtype=np.float64)
        lab32 = lab.astype(np.int32)
        assert all(D.active_mask(lab[c - 1 : c + 1]).any() for c in range(64 // size, 64, 64 // size))
        b_glob = D.random_rhs(lab, dx, dtype=np.float64)
        for use_gs in (False, True):
            emu = SlabEmulation(orc, lab32, w, lev, use_gs)
            z0, z1 = emu.z0[0], emu.z1[0]
            x, b = emu.new(0), emu.new(0)
            emu.owned(b)[:] = b_glob[z0:z1]
            whole = orc.solver(lab32, w, lev, use_gs)
            x_ref = np.zeros(lab.shape)
            for it in range(2):
                emu.vcycle(x, b, it > 0)
                whole.apply_vcycle(x_ref, b_glob, it > 0)
                err = np.abs(emu.owned(x) - x_ref[z0:z1]).max() / np.abs(x_ref).max()
                assert err < 1e-13, (kind, use_gs, it, err)
            if rank == 0:
                print(f"  cpu emulation {kind} gs={use_gs}: D={emu.D} of {emu.L} levels, {emu.exchanges} exchanges, "
                      f"{emu.bytes_sent / 1e6:.2f} MB sent, err {err:.1e}", flush=True)
            # dropping the exchange in front of the Jacobi sweep / GS passes must break the match:
            # proves the comparison is sensitive to the schedule
            broken = SlabEmulation(orc, lab32, w, lev, use_gs)
            real_exchange, count = broken.exchange, [0]

            def lossy(a, *args, **kw):
                count[0] += 1
                if count[0] % 4:
                    real_exchange(a, *args, **kw)

            broken.exchange = lossy
            xb = broken.new(0)
            broken.vcycle(xb, b, False)
            x_one = np.zeros(lab.shape)
            whole.apply_vcycle(x_one, b_glob, False)
            bad = np.array([np.abs(broken.owned(xb) - x_one[z0:z1]).max()])
            t = torch.from_numpy(bad)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            assert t.item() > 1e-9 * np.abs(x_one).max(), "schedule check is not sensitive"
            dist.barrier()


def rccl_single_rank_mode():
    """World size 1 over the library's own RCCL transport: exercises dlopen(librccl), the unique id,
    ncclCommInitRank, the all-reduce and the root-only gather / scatter of the collapse."""
    import geometricmultigridpressuresolver_amd as G
    from conftest import make_domain
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd.distributed import RcclComm, SlabSolver

    torch.cuda.set_device(0)
    lab, w, off, lev, dx = make_domain("solid", 96, 5, (128, 128, 128))
    comm = RcclComm(device=0)
    comm.selftest(1 << 20)  # ncclSend / ncclRecv to self: the point-to-point path of librccl on this box
    comm.selftest(3)
    b_glob = D.random_rhs(lab, dx)
    for use_gs in (False, True):
        opt = G.default_options()
        opt.min_cells_per_rank = 0
        slab = SlabSolver(lab, w, lev, use_gs, comm, device=0, options=opt)
        whole = G.GeometricMultigridPoissonSolver(lab, w, lev, use_gs, device=0)
        xs, xw = slab.new_grid(), whole.new_grid()
        bs, bw = slab.to_device(b_glob), whole.to_device(b_glob)
        for it in range(2):
            slab.applyVCycle(xs, bs, it > 0)
            whole.applyVCycle(xw, bw, it > 0)
        assert rel_l2(xs.cpu().numpy(), xw.cpu().numpy()) < 1e-6
        assert abs(slab.dotProduct(xs, bs) - whole.dotProduct(xw, bw)) <= 1e-12 * abs(whole.dotProduct(xw, bw))
        st = slab.solveGeometricConjugateGradient(slab.new_grid(), bs, 1e-5, 100, True)
        assert st["outcome"] == "converged"
        slab.close()
        whole.close()
    comm.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    dist.init_process_group("gloo")
    if mode == "gpu":
        gpu_mode()
    elif mode == "plane":
        plane_mode()
    elif mode == "bandopts":
        band_options_mode()
    elif mode == "balanced":
        balanced_mode()
    elif mode == "rccl1":
        rccl_single_rank_mode()
    elif mode == "violation":
        violation_mode()
    elif mode == "interrupt":
        interrupt_mode()
    elif mode == "cpu":
        cpu_mode()
    else:
        raise SystemExit(f"unknown mode {mode}")
    dist.barrier()
    print(f"WORKER_OK {dist.get_rank()}", flush=True)
    dist.destroy_process_group()
