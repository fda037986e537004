"""The z-folded residual handed over folded along x as well (residualZKernel<true> / residualZEdgeKernel<true> + restrictYKernel,
round 8) against the full-resolution layout of the same build (MGPS_RZ_XFOLD=0: residualZKernel<false> + restrictXYKernel) and
against the oracle.  The pair is forced onto small grids with MGPS_FUSE_RR=1 MGPS_STENCIL=plane; both switches are read once
per process, so every layout runs in a child process of its own.  The two layouts share foldX4 and the order z, x, y of the
sum: their results must be EQUAL.

MEASURED on an MI355X, balanced inputs (tests/operator_bounds.py): worst error / bound of the coarse rhs per coarse
cell 0.024 over the four cases and both layouts (bound = 1)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

OP_TOL = 5e-6       # the pair as an operator against the oracle's downsample(residual(x)): test_residual_restriction_pair_matches_oracle
VCYCLE_TOL = 1e-5   # tests/test_gpu_parity.py

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import geometricmultigridpressuresolver_amd as G
from geometricmultigridpressuresolver_amd import domains as D
from oracle.mg_oracle import Oracle

case, xfold, out, cycles = sys.argv[1], sys.argv[2] == '1', sys.argv[3], sys.argv[4] == 'cycles'


def boxed(shape, fill):
    bl = np.full(shape, D.DIRICHLET, dtype=np.uint8)
    fill(bl)
    bw = []
    for axis in range(3):
        wa = np.zeros(D.face_shape(*shape, axis), dtype=np.float32)
        back, fwd = D._shift_pair(bl, axis)
        wa[D._inner_faces(wa, axis)] = np.where((back == D.INTERIOR) | (fwd == D.INTERIOR), 1.0, 0.0)
        bw.append(wa)
    return bl, bw


def inner(bl):
    bl[1:-1, 1:-1, 1:-1] = D.INTERIOR


def middle(bl):
    bl[1:-1, 1:-1, 64:448] = D.INTERIOR


def stair(bl):
    bl[1:8, 1:12, 1:-1] = D.INTERIOR
    bl[1:16, 12:31, 1:-1] = D.INTERIOR


# (3 levels: 4 cells of padding per side, the base grid sits at +4)
if case == 'seams776':    # liquid on x in [5, 771): tiles 0 .. 2 full, tile 3 is 8 cells wide with 3 of them liquid
    bl, bw = boxed((20, 44, 768), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 776))
    xrange = (5, 771)
elif case == 'mid520':    # liquid on x in [68, 452): the range begins in lane 17 of tile 0 and ends in lane 48 of tile 1, tile 2 is dead
    bl, bw = boxed((20, 44, 512), middle)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 520))
    xrange = (68, 452)
elif case == 'stair520':  # the step of test_residual_restriction_pair_matches_oracle: blocks without active cells owe terms, across a seam too
    bl, bw = boxed((24, 32, 512), stair)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 520))
    xrange = (5, 515)
else:                     # wsolid: general BOUNDARY cells, the level keeps the full-resolution layout
    bl, bw, _ = D.build_complex_domain((24, 32, 256), use_solid=True)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
    xrange = None
act = D.active_mask(lab)
if xrange:
    xs = np.nonzero(act.any(axis=(0, 1)))[0]
    assert (xs[0], xs[-1] + 1) == xrange, (xs[0], xs[-1] + 1)
dx = 1.0 / lab.shape[2]
s = G.GeometricMultigridPoissonSolver(lab, w, lev, False)
assert s.stencil_kernel(0) == 'plane' and s.residual_restrict_fused(0), (s.stencil_kernel(0), s.residual_restrict_fused(0))
# the switch was live: the level reports the layout the child was started for -- never on a level with general cells
assert s.residual_restrict_xfolded(0) == (xfold and case != 'wsolid'), (case, xfold, s.residual_restrict_xfolded(0))
lab32, w64 = lab.astype(np.int32), [a.astype(np.float64) for a in w]
rng = np.random.default_rng(5)
res = {}
if not cycles:
    x0 = np.where(act, rng.standard_normal(lab.shape), 0.0).astype(np.float32)
    b0 = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    cd = s.new_grid(1)
    s.residualDownsample(cd, s.to_device(x0), s.to_device(b0), 0)
    got = cd.cpu().numpy()
    orc = Oracle()
    r = np.zeros(lab.shape)
    orc.residual(r, x0.astype(np.float64), b0.astype(np.float64), lab32, w64)
    lab1 = s.hierarchy().level_labels(1).astype(np.int32)
    ref = np.zeros(lab1.shape)
    orc.downsample(ref, r, lab1)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print('err', err)
    assert np.abs(ref).max() > 0 and err < %(op_tol)r, err
    # a second call lands on the same entries of rz: the same bits
    s.residualDownsample(cd, s.to_device(x0), s.to_device(b0), 0)
    assert np.array_equal(cd.cpu().numpy(), got)
    np.save(out, got)
    res['err'] = float(err)
    # per coarse cell on balanced inputs (tests/operator_bounds.py: the rhs of the size of A x, the bound from the operation count;
    # the weights as the float32 values the device holds)
    import operator_bounds as OB
    wf = [OB.as_f32(a) for a in w]
    st = OB.Stencil(lab, wf)
    xb, bb = OB.balanced_inputs(lab, wf, 105, st)
    cb = s.new_grid(1)
    s.residualDownsample(cb, s.to_device(xb), s.to_device(bb), 0)
    rb = np.zeros(lab.shape)
    orc.residual(rb, xb, bb, lab32, wf)
    refb = np.zeros(lab1.shape)
    orc.downsample(refb, rb, lab1)
    res['per_cell'] = OB.assert_within('rz_xfold %%s xfold=%%d residual+restriction' %% (case, xfold), cb.cpu().numpy(), refb,
                                       OB.bound_residual_restrict(st, xb, bb, lab1))
else:
    b = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    bd = s.to_device(b)
    x = s.new_grid()
    ref = Oracle().solver(lab32, w64, lev, False)
    xr = np.zeros(lab.shape)
    b64 = b.astype(np.float64)
    errs = []
    for it in range(3):
        s.applyVCycle(x, bd, it > 0)
        ref.apply_vcycle(xr, b64, it > 0)
        e = np.linalg.norm(x.cpu().numpy() - xr) / np.linalg.norm(xr)
        print('cycle', it, e)
        assert np.linalg.norm(xr) > 0 and e < %(vcycle_tol)r * (it + 1), (it, e)
        errs.append(float(e))
    got = x.cpu().numpy()
    assert np.all(got[~act] == 0.0)
    np.save(out, got)
    res['errs'] = errs
print('RZ_XFOLD_OK', json.dumps(res))
"""


def _run(case, xfold, path, what="operator"):
    env = dict(os.environ, MGPS_FUSE_RR="1", MGPS_STENCIL="plane", MGPS_RZ_XFOLD=xfold)
    code = CHILD % {"root": ROOT, "op_tol": OP_TOL, "vcycle_tol": VCYCLE_TOL}
    res = subprocess.run([sys.executable, "-c", code, case, xfold, path, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=600, env=env)
    assert res.returncode == 0 and "RZ_XFOLD_OK" in res.stdout, res.stdout[-3000:]
    print("".join(line for line in res.stdout.splitlines(True) if line.startswith("PERCELL")), end="")
    return np.load(path)


def _both(case, what="operator"):
    with tempfile.TemporaryDirectory() as tmp:
        return [_run(case, f, os.path.join(tmp, f"c{f}.npy"), what) for f in ("1", "0")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seams776", "mid520", "stair520"])
def test_xfolded_pair_equals_full_resolution_pair(case):
    """downsample(residual(x)) through mgps_residual_downsample on a random x and rhs, the x-folded layout against the
    full-resolution one bit for bit, each within 5e-6 of the oracle (asserted in the child, with the layout the level reports) --
    and, on balanced inputs, within the per-cell bound of tests/operator_bounds.py in every coarse cell (in the child too; with
    rhs = normal * dx^2 the 5e-6 cannot see the rhs at all, tests/test_operator_inputs_are_live.py).
    seams776: solver shape (28, 52, 776), liquid from one cell inside the padding on every axis -- three interior tile
    boundaries (x = 256, 512, 768) with liquid on both sides, whose straddling columns come from the seam array, and a last
    tile 8 cells wide.  mid520: (28, 52, 520), liquid on x in [68, 452) -- the active range begins and ends on quads in the
    middle of a wave, the first and the last live lane take zeros from their neighbours, the lanes next to the range store the
    columns they share with it, one boundary is live on both sides and the last tile is dead.  stair520: the step of
    test_residual_restriction_pair_matches_oracle at nx = 520 -- blocks without active cells owe rz a plane of terms on either
    side of a tile boundary (residualZEdgeKernel's fold and its seam entries)."""
    folded, full = _both(case)
    assert np.array_equal(folded, full), np.abs(folded - full).max()


@pytest.mark.gpu
def test_general_cells_keep_the_full_resolution_layout():
    """wsolid (free surface + cut-cell solid: general BOUNDARY cells, whose patch launches add into full-resolution entries): the
    level reports the full-resolution layout whatever the switch says (asserted in the child), and the switch moves no bit."""
    a, b = _both("wsolid")
    assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.gpu
def test_three_vcycles_on_the_xfolded_layout():
    """Three V-cycles from zero on seams776 (every level the pair fits takes it): x equal bit for bit between the two layouts, and each
    cycle within VCYCLE_TOL * (cycle + 1) of the fp64 oracle's, as the parity tests ask (asserted in the child); inactive cells
    exactly 0."""
    folded, full = _both("seams776", "cycles")
    assert np.array_equal(folded, full), np.abs(folded - full).max()
