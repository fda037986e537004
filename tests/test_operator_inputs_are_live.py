"""The inputs of the operator parity tests, checked on the CPU before anything runs on a GPU (no test here needs one).

1. tests/operator_bounds.py's stencil -- the thing every per-cell bound is made of -- without its absolute values equals
   oracle.apply_poisson / oracle.residual to 1e-13 on every domain the bounds are used on, the unit-weight coarse levels included;
   its restriction and prolongation equal oracle.downsample / oracle.upsample_add.
2. Liveness.  For every case of the GPU tests that carry a per-cell assertion (tests/test_gpu_parity.py, test_rz_xfold.py,
   test_fused_downstroke.py, test_plain_quads.py), every operator that reads a rhs and every transfer's source grid: the share of
   active cells at which the input's own term is under 4 x the cell's bound (operator_bounds.dead_share) is at most 1 % with the
   balanced inputs.  A condition on the inputs, not a measurement.
3. The same check on the OLD inputs (x of order 1 with b = random * dx^2, all non-negative; still what the maximum-normalised
   assertions run on).  OLD_DEAD names the (case, operator) pairs at which they fail it -- a kernel that dropped the rhs there
   would pass the old assertion in that share of the cells.  The set is asserted as it stands, so the reason for the balanced
   inputs stays on record."""
import numpy as np
import pytest

import operator_bounds as OB
from conftest import make_domain

LIVE_SHARE = 0.01

PARITY_DOMAINS = [("simple", 32), ("complex", 32), ("solid", 48), ("wide", 24), ("odd", 36), ("random", 4), ("wide512", 40), ("widesolid", 24)]
WIDE = {"wide": (3, (32, 32, 256)), "odd": (3, (44, 44, 44)), "wide512": (3, (64, 64, 512)), "widesolid": (3, (32, 40, 264))}
CHILD_CASES = {  # case -> (seed of the child's generator, operators its assertions cover)
    "pair/stair": (5, ("residual_restrict",)), "pair/wsolid": (5, ("residual_restrict",)), "pair/rag264": (5, ("residual_restrict",)),
    "rz_xfold/seams776": (5, ("residual_restrict",)), "rz_xfold/mid520": (5, ("residual_restrict",)),
    "rz_xfold/stair520": (5, ("residual_restrict",)), "rz_xfold/wsolid": (5, ("residual_restrict",)),
    "downstroke/seams776": (15, ("jacobi", "residual_restrict")), "downstroke/mid520": (15, ("jacobi", "residual_restrict")),
    "downstroke/stair520": (15, ("jacobi", "residual_restrict")), "downstroke/rag264": (15, ("jacobi", "residual_restrict")),
    "downstroke/tall264": (15, ("jacobi", "residual_restrict")), "downstroke/ragz264": (15, ("jacobi", "residual_restrict")),
    "downstroke/wsolid": (15, ("jacobi", "residual_restrict")),
    "plain_quads/seams776": (5, ("residual", "jacobi", "residual_restrict")), "plain_quads/mid520": (5, ("residual", "jacobi", "residual_restrict")),
    "plain_quads/wsolid": (5, ("residual", "jacobi", "residual_restrict")), "plain_quads/speckled": (5, ("residual", "jacobi", "residual_restrict")),
}

# (case, operator) at which the OLD inputs leave more than 1 % of the active cells dead (measured shares: DESIGN.md 6.2): the rhs of
# every fine-level operator on every domain (1.3 % of the cells on simple-32, where dx^2 is largest, to 100 % on the long grids
# that take the plane marches), and of every operator in every child and on both sheets (77 - 100 %).  The coarse levels' old
# rhs is of order 1 and live, as are the transfers' sources.
OLD_DEAD = {f"parity/{kind}-{g}/L0": {"residual", "jacobi", "gs"} for kind, g in PARITY_DOMAINS}
OLD_DEAD.update({case: set(ops) for case, (seed, ops) in CHILD_CASES.items()})
OLD_DEAD.update({"sheet/992": {"residual", "jacobi", "residual_restrict"}, "sheet/1248": {"residual", "jacobi"}})


def _old_rand(lab, seed, scale=1.0):
    """tests/test_gpu_parity.py's _rand_active"""
    v = np.random.Generator(np.random.PCG64(seed)).random(lab.shape) * scale
    v[~OB.active_mask(lab)] = 0
    return v


def _level_labels(oracle, lab, levels):
    labs = [np.ascontiguousarray(lab, dtype=np.int32)]
    for _ in range(1, levels):
        labs.append(oracle.build_coarse_labels(labs[-1]))
    return labs


def _rhs_shares(st, ops, x, b, coarse_lab=None):
    out = {}
    for op in ops:
        if op == "gs":  # no derived bound of its own (its yardstick is the fp32 oracle): the undamped Jacobi form stands in
            out[op] = OB.dead_share("jacobi", st, x, b, omega=1.0)
        elif op == "band":
            out[op] = OB.dead_share("jacobi", st, x, b)
        else:
            out[op] = OB.dead_share(op, st, x, b, coarse_lab=coarse_lab)
    return out


def _report(case, new, old):
    for op in new:
        print(f"LIVE {case} {op}: balanced {new[op]:.4f} old {old[op]:.4f}")
    assert all(v <= LIVE_SHARE for v in new.values()), (case, new)
    dead = {op for op, v in old.items() if v > LIVE_SHARE}
    assert dead == OLD_DEAD.get(case, set()), (case, old)


def _validate(oracle, st, lab32, w64, seed):
    """the stencil without its absolute values is the oracle's operator"""
    x, b = OB.balanced_inputs(lab32, w64, seed, st)
    y, r = np.zeros(lab32.shape), np.zeros(lab32.shape)
    oracle.apply_poisson(y, x, lab32, w64)
    oracle.residual(r, x, b, lab32, w64)
    scale = max(float(np.abs(y).max()), 1.0)
    assert np.abs(st.apply(x) - st.cut(y)).max() <= 1e-13 * scale
    assert np.abs(st.residual(x, b) - st.cut(r)).max() <= 1e-13 * scale
    return x, b


@pytest.mark.parametrize("kind,g", PARITY_DOMAINS)
def test_parity_domains(kind, g, oracle):
    """test_fine_level_operators, test_coarse_level_operators, test_fused_band_stage, test_transfer_operators and the
    test_plane_sweep_operators_match_oracle domains, level by level"""
    levels, shape = WIDE.get(kind, (None, None))
    lab, w, off, lev, dx = make_domain(kind, g, levels, shape)
    w64 = [a.astype(np.float64) for a in w]
    labs = _level_labels(oracle, lab, lev)
    for l, ll in enumerate(labs):
        wl = w64 if l == 0 else None
        st = OB.Stencil(ll, wl)
        x, b = _validate(oracle, st, ll, wl, 100 + l)
        case = f"parity/{kind}-{g}/L{l}"
        ops = ("residual", "jacobi", "gs", "band")
        new = _rhs_shares(st, ops, x, b)
        if l == 0:
            old = _rhs_shares(st, ("residual", "jacobi", "gs"), _old_rand(lab, 1), _old_rand(lab, 2, dx * dx))
        else:
            old = _rhs_shares(st, ("residual", "jacobi", "gs"), _old_rand(ll, 10 + l), _old_rand(ll, 20 + l))
        old.update(_rhs_shares(st, ("band",), _old_rand(ll, 30 + l), _old_rand(ll, 40 + l)))
        if l + 1 < len(labs):
            cl = labs[l + 1]
            fine, csrc, fdst = OB.signed_source(ll, 130 + l), OB.signed_source(cl, 140 + l), OB.signed_source(ll, 150 + l)
            ref = np.zeros(cl.shape)
            oracle.downsample(ref, fine, cl)
            assert np.abs(OB.restrict(fine, cl) - ref).max() <= 1e-13
            ref = fdst.copy()
            oracle.upsample_add(ref, csrc, ll)
            assert np.abs(fdst + OB.prolong(csrc, ll) - ref).max() <= 1e-13
            new["restrict"] = OB.dead_share("restrict", fine=fine, coarse_lab=cl)
            new["prolong"] = OB.dead_share("prolong", fine=fdst, coarse=csrc, fine_lab=ll)
            new["residual_restrict"] = OB.dead_share("residual_restrict", st, x, b, coarse_lab=cl)
            ofine, ocsrc, ofdst = _old_rand(ll, 30 + l), _old_rand(cl, 40 + l), _old_rand(ll, 50 + l)
            old["restrict"] = OB.dead_share("restrict", fine=ofine, coarse_lab=cl)
            old["prolong"] = OB.dead_share("prolong", fine=ofdst, coarse=ocsrc, fine_lab=ll)
            old["residual_restrict"] = new["residual_restrict"]  # (no old assertion on these domains' pair)
        _report(case, new, old)


@pytest.mark.parametrize("case", sorted(CHILD_CASES))
def test_stroke_children(case, oracle):
    """the domains the children of the stroke tests build, with the children's own old inputs (standard normal x, standard
    normal * dx^2 rhs)"""
    seed, ops = CHILD_CASES[case]
    lab, w, lev = OB.stroke_case(case.split("/")[1])
    w64 = [a.astype(np.float64) for a in w]
    lab32 = np.ascontiguousarray(lab, dtype=np.int32)
    cl = oracle.build_coarse_labels(lab32)
    st = OB.Stencil(lab32, w64)
    x, b = _validate(oracle, st, lab32, w64, 100)
    new = _rhs_shares(st, ops, x, b, cl)
    rng = np.random.default_rng(seed)
    act, dx = OB.active_mask(lab), 1.0 / lab.shape[2]
    x0 = OB.as_f32(np.where(act, rng.standard_normal(lab.shape), 0.0))
    b0 = OB.as_f32(np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0))
    old = _rhs_shares(st, ops, x0, b0, cl)
    _report(case, new, old)


def _sheet(nx):
    """the 16 x 992 x nx free-surface sheet with a cut-cell solid of test_plane_sweep_natural_dispatch_matches_oracle (nx = 992)
    and test_plane_sweep_by_size_matches_oracle (nx = 1248)"""
    from geometricmultigridpressuresolver_amd import domains as D

    shape = (16, 992, nx)
    z, y, x = np.meshgrid(np.arange(16) / 16, np.arange(992) / 992, np.arange(nx) / nx, indexing="ij")
    phi = y - 0.5 + 0.02 * np.sin(4.0 * np.pi * z) + 0.0 * x
    del z, y, x
    bl, bw, dx = D._complex_from_phi(phi, shape, True, (0.4, 0.6), np.float32, 1.0 / 992)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=5, solver_shape=(48, 1024, nx + 32))
    return lab, w, dx


@pytest.mark.parametrize("nx,ops", [(992, ("residual", "jacobi", "residual_restrict")), (1248, ("residual", "jacobi"))])
def test_large_plane_domains(nx, ops, oracle):
    """the two 50 / 63 M-cell sheets, on the box of their active cells (a third of the grid)"""
    lab, w, dx = _sheet(nx)
    box = OB.active_box(lab)
    st = OB.Stencil(lab, w, box)
    x, b = OB.balanced_inputs(lab, w, 1, st)
    cl = oracle.build_coarse_labels(np.ascontiguousarray(lab, dtype=np.int32)) if "residual_restrict" in ops else None
    new = _rhs_shares(st, ops, x, b, cl)
    old = _rhs_shares(st, ops, _old_rand(lab, 1), _old_rand(lab, 2, dx * dx), cl)
    _report(f"sheet/{nx}", new, old)


def test_extents_not_multiples_of_four_domain(oracle):
    """test_extents_not_multiples_of_four's 66-wide domain (two levels): its operator assertions are new, there are no old inputs"""
    from geometricmultigridpressuresolver_amd import domains as D

    bl, bw, dx = D.build_complex_domain((32, 36, 58), use_solid=True, dtype=np.float32)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=2, solver_shape=(40, 44, 66))
    w64 = [a.astype(np.float64) for a in w]
    labs = _level_labels(oracle, lab, lev)
    for l, ll in enumerate(labs):
        wl = w64 if l == 0 else None
        st = OB.Stencil(ll, wl)
        x, b = _validate(oracle, st, ll, wl, 100 + l)
        new = _rhs_shares(st, ("residual", "jacobi", "gs", "band"), x, b)
        if l == 0:
            new["residual_restrict"] = OB.dead_share("residual_restrict", st, x, b, coarse_lab=labs[1])
        print(f"LIVE ext66/L{l}", new)
        assert all(v <= LIVE_SHARE for v in new.values()), new
