"""options.enclosed_liquid on the coarsest level, host only (mgps_hierarchy_create + mgps_hierarchy_coarse_solve): a liquid
region that touches no DIRICHLET cell makes the coarsest matrix a graph Laplacian with the constant on that region as its null
space.  The reference's Cholesky only asserts (MG.cpp:409-411); without the option the banded factor accepts the tiny positive
last pivot rounding leaves and the solve returns values of 1e15.  With it, the minimum-index cell of each such component is pinned
to 0 and the rest is an exact solve of the consistent system."""
import numpy as np
import pytest

import geometricmultigridpressuresolver_amd as G
from geometricmultigridpressuresolver_amd import domains as D
from test_oracle_properties import assemble


def sealed_box(n, levels, wall=False, dirichlet_top=False):
    """INTERIOR liquid in an EXTERIOR shell of 2^(levels-1) cells; wall: an EXTERIOR slab of that thickness across x splits it
    into two pockets; dirichlet_top: the top layer of the first pocket's region is DIRICHLET."""
    s = 2 ** (levels - 1)
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[s:n - s, s:n - s, s:n - s] = D.INTERIOR
    if wall:
        lab[:, :, n // 2:n // 2 + s] = D.EXTERIOR
    if dirichlet_top:
        lab[n - s - 1, s:n - s, s:n // 2] = D.DIRICHLET
    return lab


def hierarchy(lab, levels, enclosed):
    o = G.default_options()
    o.enclosed_liquid = enclosed
    return G.Hierarchy(lab, levels, options=o)


def coarse_system(h):
    lc = h.level_labels(h.levels - 1)
    A, idx, act = assemble(lc)
    return lc, A.tocsr(), idx, act


def mean_free_rhs(A, idx, act, seed):
    """a random rhs with its mean removed on every component of the coarse level that has no DIRICHLET contact"""
    from scipy.sparse.csgraph import connected_components

    rng = np.random.default_rng(seed)
    b = rng.standard_normal(int(act.sum()))
    _, comp = connected_components(A, directed=False)
    dirichlet = np.asarray(A.sum(axis=1)).ravel() > 0.5  # row sum = the DIRICHLET neighbours
    for c in np.unique(comp):
        on = comp == c
        if not dirichlet[on].any():
            b[on] -= b[on].mean()
    grid = np.zeros(idx.shape, dtype=np.float32)
    grid[act] = b
    return grid, comp, dirichlet


@pytest.mark.parametrize("n,levels,unknowns", [(32, 3, 216), (64, 3, 2744)])
def test_sealed_box_coarse_solve_is_pinned(n, levels, unknowns):
    h = hierarchy(sealed_box(n, levels), levels, 1)
    assert h.coarse_unknowns == unknowns
    lc, A, idx, act = coarse_system(h)
    b, _, _ = mean_free_rhs(A, idx, act, 3)
    x = h.coarse_solve(b)
    xa, ba = x[act].astype(np.float64), b[act].astype(np.float64)
    assert np.linalg.norm(A @ xa - ba) / np.linalg.norm(ba) <= 1e-5
    pinned = np.flatnonzero(act.ravel())[0]  # the minimum linear index of the single component
    assert x.ravel()[pinned] == 0.0
    assert np.abs(x).max() <= 1e3 * np.linalg.norm(ba), np.abs(x).max()  # (without the pin: 1e15 at 32^3, 6e16 at 64^3)


def test_two_pockets_two_pins():
    n, levels = 32, 3
    h = hierarchy(sealed_box(n, levels, wall=True), levels, 1)
    lc, A, idx, act = coarse_system(h)
    b, comp, dirichlet = mean_free_rhs(A, idx, act, 5)
    assert len(np.unique(comp)) == 2 and not dirichlet.any()
    x = h.coarse_solve(b)
    xa, ba = x[act].astype(np.float64), b[act].astype(np.float64)
    assert np.linalg.norm(A @ xa - ba) / np.linalg.norm(ba) <= 1e-5
    cells = np.flatnonzero(act.ravel())
    for c in np.unique(comp):
        first = cells[comp == c].min()
        assert x.ravel()[first] == 0.0
    assert np.count_nonzero(x[act] == 0.0) >= 2


def test_pins_only_where_no_dirichlet_contact():
    """one pocket open (a DIRICHLET layer on top), one sealed: one pin, in the sealed pocket"""
    n, levels = 32, 3
    h = hierarchy(sealed_box(n, levels, wall=True, dirichlet_top=True), levels, 1)
    lc, A, idx, act = coarse_system(h)
    b, comp, dirichlet = mean_free_rhs(A, idx, act, 9)
    x = h.coarse_solve(b)
    xa, ba = x[act].astype(np.float64), b[act].astype(np.float64)
    assert np.linalg.norm(A @ xa - ba) / np.linalg.norm(ba) <= 1e-5
    cells = np.flatnonzero(act.ravel())
    for c in np.unique(comp):
        first = cells[comp == c].min()
        if dirichlet[comp == c].any():
            assert x.ravel()[first] != 0.0
        else:
            assert x.ravel()[first] == 0.0


def test_dirichlet_contact_bit_identical_to_option_off():
    n, levels = 32, 3
    lab = sealed_box(n, levels)
    lab[n - 2 ** (levels - 1) - 1, 4:28, 4:28] = D.DIRICHLET
    outs = []
    for enclosed in (0, 1):
        h = hierarchy(lab, levels, enclosed)
        _, A, idx, act = coarse_system(h)
        b, _, _ = mean_free_rhs(A, idx, act, 11)
        b[act] += 0.25  # (not mean-free: the system is non-singular)
        outs.append(h.coarse_solve(b))
    assert np.array_equal(outs[0], outs[1])


def test_option_values_are_checked():
    lab = sealed_box(32, 3)
    o = G.default_options()
    o.enclosed_liquid = 2
    with pytest.raises(G.MgpsError) as e:
        G.Hierarchy(lab, 3, options=o)
    assert e.value.status == 1


def test_shim_has_the_enclosed_toggle():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "geometricmultigridpressuresolver_amd", "host")
    shim = open(os.path.join(host, "HDK_GeometricFreeSurfacePressureSolver.cpp")).read()
    header = open(os.path.join(host, "HDK_GeometricFreeSurfacePressureSolver.h")).read()
    assert '"handleEnclosedLiquid"' in shim and '"handleEnclosedLiquid"' in header and "opt.enclosed_liquid" in shim
