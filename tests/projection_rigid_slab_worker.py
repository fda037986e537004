"""Worker of tests/test_projection_rigid_slabs.py: run under torch.distributed.run with 1, 2 or 4 ranks sharing the one GPU.
mgps_project_free_surface_rigid_slab (include/mgps_fields.h) against the plain slab one-call in the kinematic
limit, against the composed whole-grid projection project_free_surface_rigid, and against the host's V* - K G^T p.  The scenes and
references are those of tests/rigid_coupling_slab_worker.py.

modes: "one_anchor", "one_real", "one_interrupt" (one rank over a transport whose every entry fails: no transport call is made),
"ranks" (scene B at two and four ranks), "scene_a" (two ranks), "fail" (two ranks).  Prints "WORKER_OK <rank>" on success.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rigid_coupling_reference as RC  # noqa: E402
import rigid_coupling_slab_worker as W  # noqa: E402
import solid_forces_reference as R  # noqa: E402
from conftest import rel_l2  # noqa: E402
from test_rigid_coupling import TOL  # noqa: E402

COUNTS_B = {1: [3432], 2: [2464, 968], 4: [416, 2048, 968, 0]}  # scene B's coupled cells per rank
KW_B = {"use_gauss_seidel": False, "power_of_two": False, "tolerance": TOL, "max_iterations": 300}
SURFACE = {"surface_tension": 2.0, "dt": 0.01, "dx": 1.0 / 48, "density": 1000.0}


def setup(sc, size, rank, g, p2):
    lay = g.F.projection_slab_layout(sc["shape"], p2, size, False)
    assert W.base_cuts(lay["splits"], lay["offset"], sc["shape"][0]) == W.BASE_CUTS[size], lay
    return lay["splits"], g.F.slab_window(sc["shape"], p2, lay["splits"], rank)


def fp64_vectors(g):
    opt = g.G.default_options()
    opt.pcg_fp64_vectors = 1
    return opt


def zeros3(shape, g):
    return [g.torch.zeros(fs, dtype=g.torch.float32, device="cuda") for fs in g.F._face3(shape)]


def tensors(sc, d, g, base_sv=None, pressure=None):
    torch = g.torch
    return {
        "liquid_phi": g.dev(sc["liquid_phi"][d.c0:d.c1]), "solid_phi": g.dev(sc["solid_phi"][d.c0:d.c1]), "cut_weights": W.window(sc["cut_weights"], d, g.dev),
        "velocity": W.window(sc["velocity"], d, g.dev), "body": W.window(sc["body"], d, g.dev),
        "solid_velocity": W.window(base_sv, d, g.dev) if base_sv is not None else None,
        "pressure": g.dev(pressure[d.c0:d.c1]) if pressure is not None else torch.zeros(d.base_shape, dtype=torch.float32, device="cuda"),
        "sv_out": [torch.full(fs, 7.0, dtype=torch.float32, device="cuda") for fs in g.F._face3(d.base_shape)],  # (junk: the call writes every face)
    }


def rigid_call(comm, splits, sc, d, g, kinematic=False, base_sv=None, pressure=None, t=None, **kw):
    z = 0.0 if kinematic else 1.0
    t = t or tensors(sc, d, g, base_sv, pressure)
    valid, info = g.F.project_free_surface_rigid_slab(comm, splits, sc["shape"], t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"],
                                                      t["body"], sc["centres"], z * sc["inv_mass"], z * sc["inv_inertia"], sc["motions"],
                                                      solid_velocity=t["solid_velocity"], solid_velocity_out=t["sv_out"], **kw)
    g.torch.cuda.synchronize()
    return t, valid, info


def star_window(sc, d, g, base_sv=None):
    """rigidVelocitySlab(base or zeros, V*) on the window"""
    sv = W.window(base_sv, d, g.dev) if base_sv is not None else zeros3(d.base_shape, g)
    return g.F.rigidVelocitySlab(d, sv, W.window(sc["body"], d, g.dev), sc["centres"], sc["motions"])


def plain_call(comm, splits, sc, d, g, base_sv=None, **kw):
    """the plain one-call with the bodies kinematic: solid_velocity = rigidVelocitySlab(base, V*)"""
    t = tensors(sc, d, g)
    t["solid_velocity"] = star_window(sc, d, g, base_sv)
    valid, info = g.F.project_free_surface_slab(comm, splits, sc["shape"], t["liquid_phi"], t["solid_phi"], t["cut_weights"], t["velocity"], t["pressure"],
                                                t["solid_velocity"], **kw)
    g.torch.cuda.synchronize()
    return t, valid, info


def whole(windows, size, g):
    """the whole grid's face arrays (numpy) from every rank's windows"""
    parts = g.S.all_ranks([a.cpu().numpy() for a in windows])
    return [np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2][:-1] for p in parts[:-1]] + [parts[-1][2]])]


def equal_cut_planes(what, grids, size, g):
    planes = g.S.all_ranks((grids[2][0].cpu().numpy(), grids[2][-1].cpu().numpy()))
    for r in range(size - 1):  # rank r's last z-face plane is rank r + 1's first
        assert np.array_equal(planes[r][1].view(np.int32), planes[r + 1][0].view(np.int32)), (what, r)


# ---- 4. the kinematic anchor ---------------------------------------------------------------------------------------------------------
def check_anchor(what, comm, splits, sc, d, g, kw, base_sv=None):
    """K = 0 under pcg_fp64_vectors = 1: the plain one-call on solid_velocity = rigidVelocitySlab(base, V*), bit for bit"""
    kw = dict(kw, options=fp64_vectors(g), use_old_pressure=False)
    tp, valid_p, info_p = plain_call(comm, splits, sc, d, g, base_sv, **kw)
    t, valid, info = rigid_call(comm, splits, sc, d, g, kinematic=True, base_sv=base_sv, **kw)
    same = lambda a, b: np.array_equal(a.cpu().numpy(), b.cpu().numpy())  # noqa: E731
    assert info_p["outcome"] == 0 and info_p["iterations"] > 3 and float(t["pressure"].abs().max()) > 0, info_p
    assert same(t["pressure"], tp["pressure"]), what
    for a in range(3):
        assert same(t["velocity"][a], tp["velocity"][a]) and same(valid[a], valid_p[a]), (what, a)
        assert same(t["sv_out"][a], tp["solid_velocity"][a]), (what, a)  # V_out = V*
    for key in ("iterations", "outcome", "rel_residual", "divergence_sum", "divergence_max", "liquid_cells", "surface_pressure_max"):
        assert info[key] == info_p[key], (what, key, info[key], info_p[key])
    assert np.array_equal(info["motions"], sc["motions"]), what
    if comm.rank == 0:
        print(f"{what}: K = 0 equals the plain one-call bit for bit; {info['iterations']} it, rel_residual {info['rel_residual']:.3e}, divergence max "
              f"{info['divergence_max']:.3e}, residual_inf {info['residual_inf']:.3e} (plain {info_p['residual_inf']:.3e})", flush=True)
    return info_p


# ---- 5. real K against the composed whole-grid projection ----------------------------------------------------------------------------
def host_motions_error(sc, mat_h, p_all, v_out):
    """|V_out - (V* - K G^T p)| / sum |V_out| with the product formed on the host in fp64 from the published pressure"""
    Gb, K = RC.coupling_matrix(mat_h, sc["cut_weights"], sc["body"], sc["centres"]), RC.stiffness(sc["inv_mass"], sc["inv_inertia"])
    p_base = np.where(mat_h == R.LIQUID, p_all.astype(np.float64), 0.0).reshape(-1)
    host = RC.table(RC.flat(sc["motions"]) - K @ (Gb.T @ p_base))
    return float(np.abs(v_out - host).sum() / np.abs(v_out).sum())


def check_real(what, comm, splits, sc, d, g, kw, kin_div, base_sv=None, cells=None):
    torch, F = g.torch, g.F
    rank, size, shape = comm.rank, comm.size, sc["shape"]
    dev3 = lambda grids: [g.dev(a) for a in grids]  # noqa: E731
    phi, solid, cw, body = g.dev(sc["liquid_phi"]), g.dev(sc["solid_phi"]), dev3(sc["cut_weights"]), dev3(sc["body"])
    ref = F.project_free_surface_rigid(phi, solid, cw, dev3(sc["velocity"]), torch.zeros(shape, dtype=torch.float32, device="cuda"), body, sc["centres"],
                                       sc["inv_mass"], sc["inv_inertia"], sc["motions"], solid_velocity=dev3(base_sv) if base_sv is not None else None,
                                       use_old_pressure=False, **kw)
    t, valid, info = rigid_call(comm, splits, sc, d, g, base_sv=base_sv, use_old_pressure=False, **kw)
    material, mat_h = ref["material"], ref["material"].cpu().numpy()
    for a, want in enumerate(g.S.faces([v.cpu().numpy() for v in ref["valid_faces"]], d)):
        assert np.array_equal(valid[a].cpu().numpy(), want), (what, a)
    assert info["outcome"] == 0 and ref["stats"]["outcome"] == "converged", (what, info, ref["stats"])
    assert abs(info["iterations"] - ref["stats"]["iterations"]) <= 1, (what, info["iterations"], ref["stats"]["iterations"])
    p_all = np.concatenate(g.S.all_ranks(t["pressure"].cpu().numpy()))
    perr = rel_l2(p_all, ref["pressure"].cpu().numpy())
    u_all, sv_all = whole(t["velocity"], size, g), whole(t["sv_out"], size, g)
    uerr = 0.0
    for a in range(3):
        want = ref["velocity"][a].cpu().numpy()
        err = float(np.abs(u_all[a] - want).max())
        uerr = max(uerr, err / max(1.0, float(np.abs(want).max())))
    v_out, imp = info["motions"], info["impulses"]
    e_host = host_motions_error(sc, mat_h, p_all, v_out)
    rows = F.solidForces(g.dev(p_all), material, cw, body, sc["centres"], 1.0)
    _, fmag = R.solid_forces(p_all, mat_h, sc["cut_weights"], sc["body"], sc["centres"], 1.0)
    ierr = float((np.abs(imp[1:] - rows[1:, :6]) / np.maximum(fmag[1:, :6], 1e-300)).max())
    base_win = W.window(base_sv, d, g.dev) if base_sv is not None else zeros3(d.base_shape, g)
    sv_want = F.rigidVelocitySlab(d, base_win, t["body"], sc["centres"], v_out)
    div_fields = F.computeResultingDivergence(material, dev3(u_all), cw, dev3(sv_all))[1]
    base_all = dev3(base_sv) if base_sv is not None else zeros3(shape, g)
    star = F.computeResultingDivergence(material, dev3(u_all), cw, F.rigidVelocity(base_all, body, sc["centres"], sc["motions"]))[1]
    end = info["divergence_max"]
    if rank == 0:
        print(f"{what}: {info['iterations']} it (whole grid {ref['stats']['iterations']}), pressure rel_l2 {perr:.2e} (bound 1e-4), velocity {uerr:.2e} of max(1, max|u|) "
              f"(bound 1e-6), coupled cells {info['coupled_cells']}; V_out against the host's {e_host:.2e}, impulses against solidForces {ierr:.2e} (bounds 1e-10); "
              f"divergence max {end:.3e}, from the published fields {div_fields:.3e} (bound 1e-5 relative), kinematic {kin_div:.3e} (bound 4 x), against "
              f"rigidVelocity(V*) {star:.3e} ({star / end:.0f} x, bound > 100 x); residual_inf {info['residual_inf']:.3e}, residual_l2 {info['residual_l2']:.3e}", flush=True)
    assert perr < 1e-4, (what, perr)
    assert uerr < 1e-6, (what, uerr)
    assert info["coupled_cells"] == ref["coupled_cells"] and (cells is None or info["coupled_cells"] == cells), (what, info["coupled_cells"], ref["coupled_cells"])
    assert e_host <= 1e-10 and not np.array_equal(v_out, sc["motions"]), (what, e_host)
    assert np.array_equal(imp[0], np.zeros(6)) and ierr <= 1e-10, (what, ierr)
    for a in range(3):
        assert np.array_equal(t["sv_out"][a].cpu().numpy().view(np.int32), sv_want[a].cpu().numpy().view(np.int32)), (what, a)
    assert abs(end - div_fields) <= 1e-5 * div_fields, (what, end, div_fields)
    assert end <= 4 * kin_div, (what, end, kin_div)
    assert star > 100 * end, (what, star, end)
    # one report on every rank, equal copies of every cut's z-face plane
    report = (info["iterations"], info["rel_residual"], info["divergence_sum"], info["divergence_max"], info["residual_inf"], info["residual_l2"],
              info["liquid_cells"], info["coupled_cells"])
    seen = g.S.all_ranks(v_out.tobytes() + imp.tobytes() + repr(report).encode())
    assert all(q == seen[0] for q in seen), (what, "the ranks hold different results")
    equal_cut_planes(what + " velocity", t["velocity"], size, g)
    equal_cut_planes(what + " solid_velocity_out", t["sv_out"], size, g)
    return info, p_all, mat_h


# ---- GPU, one rank --------------------------------------------------------------------------------------------------------------------
def silent_comm(g):
    """W.failing_vtable completed with the entries the slab solver's constructor asks for: every one fails and says so in `calls`"""
    Dd, calls = g.Dd, []
    comm = W.failing_vtable(g, calls)
    more = [Dd._GATH(lambda *a: calls.append("gather") or 1), Dd._GATH(lambda *a: calls.append("scatter") or 1),
            Dd._GATHV(lambda *a: calls.append("gatherv") or 1), Dd._SCATV(lambda *a: calls.append("scatterv") or 1),
            Dd._EXCH2(lambda *a: calls.append("exchange2") or 1)]
    comm.struct.gather, comm.struct.scatter, comm.struct.gatherv, comm.struct.scatterv, comm.struct.exchange2 = more
    comm.keep += more
    return comm, calls


def one_anchor_mode():
    g = W._gpu()
    sc = W.scene_b()
    comm, calls = silent_comm(g)
    splits, d = setup(sc, 1, 0, g, False)
    check_anchor("one rank, surface tension off", comm, splits, sc, d, g, KW_B)
    info = check_anchor("one rank, surface tension on", comm, splits, sc, d, g, dict(KW_B, **SURFACE))
    assert info["iterations"] > 3
    assert not calls, calls


def one_real_mode():
    g = W._gpu()
    sc = W.scene_b()
    comm, calls = silent_comm(g)
    splits, d = setup(sc, 1, 0, g, False)
    _, _, kin = plain_call(comm, splits, sc, d, g, options=fp64_vectors(g), use_old_pressure=False, **KW_B)
    info, p_all, mat_h = check_real("one rank", comm, splits, sc, d, g, KW_B, kin["divergence_max"], cells=sum(COUNTS_B[1]))
    assert info["coupled_cells_rank"] == info["coupled_cells"]
    # 6. a warm start from the answer leaves at iteration 0
    t, _, info2 = rigid_call(comm, splits, sc, d, g, pressure=p_all, use_old_pressure=True, **dict(KW_B, tolerance=1e-5))
    e_host = host_motions_error(sc, mat_h, t["pressure"].cpu().numpy(), info2["motions"])
    print(f"warm start: iterations {info2['iterations']}, outcome {info2['outcome']}, V_out against the host's {e_host:.2e}", flush=True)
    assert info2["iterations"] == 0 and info2["outcome"] == 2, info2
    assert e_host <= 1e-10, e_host
    assert not calls, calls


def one_interrupt_mode():
    """an interrupt at the top of iteration 2: the pressure of the call truncated there, motions_out of that pressure"""
    from test_pcg_exits import INTERRUPTED, UNREACHABLE, Poller, ulps

    g = W._gpu()
    sc = W.scene_b()
    comm, calls = silent_comm(g)
    splits, d = setup(sc, 1, 0, g, False)
    poller = Poller()
    opt = poller.install(g.G.default_options())
    kw = dict(KW_B, tolerance=UNREACHABLE, options=opt, use_old_pressure=False)
    polls = {}
    for u in (2, 3):  # where the polls sit: every iteration polls once at its top, a cycle that polls does so equally often each time
        poller.arm(None)
        _, _, info = rigid_call(comm, splits, sc, d, g, **dict(kw, max_iterations=u))
        assert info["iterations"] == u and info["outcome"] == 3, info  # MGPS_PCG_MAX_ITERATIONS
        polls[u] = poller.polls
    cycle = polls[3] - polls[2] - 1
    site = cycle + 2 * (cycle + 1)
    poller.arm(site)
    t = tensors(sc, d, g)
    try:
        rigid_call(comm, splits, sc, d, g, t=t, **dict(kw, max_iterations=200))
    except g.G.MgpsError as err:
        assert err.status == INTERRUPTED and poller.polls == site + 1, (err.status, poller.polls, site)
        info = err.info
    else:
        raise AssertionError("the interrupt went unnoticed")
    g.torch.cuda.synchronize()
    poller.arm(None)
    tt, _, info_t = rigid_call(comm, splits, sc, d, g, **dict(kw, max_iterations=info["iterations"]))
    worst = ulps(t["pressure"].cpu().numpy(), tt["pressure"].cpu().numpy())
    mat_h = W.material_of(sc, g).cpu().numpy()
    e_host = host_motions_error(sc, mat_h, t["pressure"].cpu().numpy(), info["motions"])
    sv_want = g.F.rigidVelocitySlab(d, zeros3(d.base_shape, g), t["body"], sc["centres"], info["motions"])
    print(f"interrupt at poll {site} ({cycle} polls per cycle): iteration {info['iterations']}, {worst} ulp from the truncated call, V_out against the host's "
          f"{e_host:.2e}", flush=True)
    assert info["iterations"] == 2 and worst <= 1 and float(t["pressure"].abs().max()) > 0, (info, worst)
    assert e_host <= 1e-10 and np.abs(info["motions"] - info_t["motions"]).sum() <= 1e-6 * np.abs(info_t["motions"]).sum(), e_host
    for a in range(3):
        assert g.torch.equal(t["sv_out"][a], sv_want[a]), a
    assert not calls, calls


# ---- GPU, two and four ranks ------------------------------------------------------------------------------------------------------------
def ranks_mode():
    g = W._gpu()
    comm = g.Dd.TorchDistComm()
    sc = W.scene_b()
    splits, d = setup(sc, comm.size, comm.rank, g, False)
    kin = check_anchor(f"{comm.size} ranks", comm, splits, sc, d, g, KW_B)
    info, _, _ = check_real(f"{comm.size} ranks", comm, splits, sc, d, g, KW_B, kin["divergence_max"], cells=sum(COUNTS_B[comm.size]))
    counts = g.S.all_ranks(info["coupled_cells_rank"])
    if comm.rank == 0:
        print(f"coupled cells per rank {counts}", flush=True)
    assert counts == COUNTS_B[comm.size], counts


def scene_a_mode():
    """scene A: fractional z-face weights on the cut planes, ids -1 .. 4, the power-of-two expansion, a base solid velocity"""
    from geometricmultigridpressuresolver_amd import domains as D

    g = W._gpu()
    comm = g.Dd.TorchDistComm()
    sc = W.scene_a()
    shape, bodies = sc["shape"], sc["bodies"]
    rng = np.random.default_rng(33)
    sc["motions"] = np.concatenate([rng.standard_normal((bodies + 1, 3)), 0.1 * rng.standard_normal((bodies + 1, 3))], axis=1)
    sc["motions"][0] = 0.0  # (row 0 is nobody's: the call copies it, the host's table holds zeros there)
    sc["velocity"] = D.projection_scene(shape)["velocity"]
    base_sv = [(0.1 * rng.standard_normal(R.face_shape(shape, a))).astype(np.float32) for a in range(3)]
    splits, d = setup(sc, comm.size, comm.rank, g, True)
    kw = dict(KW_B, power_of_two=True)
    kin = check_anchor("scene A", comm, splits, sc, d, g, kw, base_sv)
    check_real("scene A", comm, splits, sc, d, g, kw, kin["divergence_max"], base_sv)


def fail_mode():
    g = W._gpu()
    torch = g.torch
    comm = g.Dd.TorchDistComm()
    rank = comm.rank
    assert comm.size == 2
    sc = W.scene_b()
    splits, d = setup(sc, 2, rank, g, False)

    def refused(what, words, t=None, sc_=sc, **kw):
        t = t or tensors(sc_, d, g)
        before = [t["pressure"].clone()] + [v.clone() for v in t["velocity"]] + [v.clone() for v in t["sv_out"]]
        try:
            rigid_call(comm, splits, sc_, d, g, t=t, use_old_pressure=False, **dict(KW_B, **kw))
        except g.G.MgpsError as err:
            assert err.status == 1 and all(w in str(err) for w in words), (what, rank, str(err))
        else:
            raise AssertionError(f"rank {rank}: {what} was accepted")
        after = [t["pressure"]] + t["velocity"] + t["sv_out"]
        assert all(torch.equal(a, b) for a, b in zip(before, after)), what  # pressure, velocity and solid_velocity_out hold what they held
        if rank == 0:
            print(f"{what}: refused on every rank", flush=True)

    # a body grid missing on rank 1: its own text there, "rank 1 failed" on rank 0
    t = tensors(sc, d, g)
    if rank == 1:
        t["body"][1] = None
    refused("a body grid missing on rank 1", ("body: three grids",) if rank == 1 else ("rank 1 failed (arguments, status 1)",), t=t)
    # bodies 2 on rank 0 and 3 on rank 1
    three = dict(sc)
    if rank == 1:
        for key in ("centres", "inv_mass", "inv_inertia", "motions"):
            three[key] = np.concatenate([sc[key], sc[key][-1:]])
    refused("bodies 2 and 3", ("bodies differs between the ranks", "2 .. 3"), sc_=three)
    # precision = 1: the slab solver's constructor refuses it before the coupled solve, which would, is reached
    mixed = g.G.default_options()
    mixed.precision = 1
    refused("precision = 1", ("precision",), options=mixed)
    # what the coupled solve refuses, with its message
    sealed = dict(sc, liquid_phi=np.full(sc["shape"], -1.0 / max(sc["shape"]), dtype=np.float32))  # no air: nothing open
    enclosed = g.G.default_options()
    enclosed.enclosed_liquid = 1
    refused("an enclosed component", ("mgps_solve_pcg_coupled", "enclosed"), sc_=sealed, options=enclosed)
    # enclosed_liquid = 1 without an enclosed component is accepted, and the transport is as good as new
    _, _, info = rigid_call(comm, splits, sc, d, g, use_old_pressure=False, options=enclosed, **KW_B)
    assert info["outcome"] == 0 and info["enclosed_components"] == 0 and info["coupled_cells"] == sum(COUNTS_B[2]), info
    if rank == 0:
        print(f"enclosed_liquid = 1 on the open scene: accepted, {info['iterations']} it", flush=True)


if __name__ == "__main__":
    from slab_slices import worker_main

    worker_main({"one_anchor": one_anchor_mode, "one_real": one_real_mode, "one_interrupt": one_interrupt_mode, "ranks": ranks_mode,
                 "scene_a": scene_a_mode, "fail": fail_mode})
