"""The closure launch of the fused up-stroke with its coarse input staged in LDS (bandBoxBody, PRO without general cells, round 8):
the coarse cells a group's corrections interpolate from are loaded once per group as a dense box instead of eight scattered loads
per listed cell.  The yardstick is the one of tests/test_fused_upstroke.py: MGPS_FUSE_UP=1 against MGPS_FUSE_UP=0 (the separate
prolongation pass) in child processes of their own, x EQUAL after three V-cycles -- the same lerps in the same order."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import geometricmultigridpressuresolver_amd as G
from geometricmultigridpressuresolver_amd import domains as D
from oracle.mg_oracle import Oracle

case, fused, out = sys.argv[1], sys.argv[2] == '1', sys.argv[3]


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


def shifted(bl):  # rag264's box of liquid, begun one cell later on every axis
    bl[2:-1, 2:-1, 2:-1] = D.INTERIOR


def shelled(bl):  # liquid up to a one-cell DIRICHLET shell
    bl[1:-1, 1:-1, 1:-1] = D.INTERIOR


def speckled(bl):  # tests/test_fused_upstroke.py's random labels
    bl[1:-1, 1:-1, 1:-1] = np.where(np.random.default_rng(3).random((22, 30, 246)) < 0.95, D.INTERIOR, D.DIRICHLET)


if case == 'odd264':     # 3 levels, 4 cells of padding: the liquid begins at the even cell 6 where rag264's begins at 5 -- box origins of the other parity
    bl, bw = boxed((20, 44, 248), shifted)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 264))
elif case == 'edge264':  # 2 levels, 2 cells of padding, liquid on cells 3 .. n - 4: the regions (with the inactive neighbours) span cells 2 .. n - 3
    bl, bw = boxed((8, 16, 260), shelled)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=2, solver_shape=(12, 20, 264))
else:                    # random: DIRICHLET cells scattered through the liquid
    bl, bw = boxed((24, 32, 248), speckled)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
s = G.GeometricMultigridPoissonSolver(lab, w, lev, False)
flags = [s.up_stroke_fused(l) for l in range(s.getMGLevels())]
assert s.stencil_kernel(0) == 'plane' and flags[0] == fused, (s.stencil_kernel(0), flags)
act = D.active_mask(lab)
rng = np.random.default_rng(11)
b = np.where(act, rng.standard_normal(lab.shape) / 264.0 ** 2, 0.0).astype(np.float32)
bd = s.to_device(b)
x = s.new_grid()
s.applyVCycle(x, bd, False)
x1 = x.cpu().numpy()
for _ in range(2):
    s.applyVCycle(x, bd, True)
x3 = x.cpu().numpy()
assert np.all(x3[~act] == 0.0)
ref = Oracle().solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, False)
xr = np.zeros(lab.shape)
ref.apply_vcycle(xr, b.astype(np.float64), False)
err = np.linalg.norm(x1 - xr) / np.linalg.norm(xr)
assert np.linalg.norm(xr) > 0 and err < 1e-5, err
np.save(out, x3)
print('COARSE_BOX_OK', json.dumps({'err': err, 'flags': flags}))
"""


def _run(case, fused, path):
    env = dict(os.environ, MGPS_FUSE_UP=fused, MGPS_STENCIL="plane")
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, case, fused, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600, env=env)
    assert res.returncode == 0 and "COARSE_BOX_OK" in res.stdout, res.stdout[-3000:]
    return np.load(path)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["odd264", "edge264", "random"])
def test_staged_coarse_box_equals_separate_prolongation(case):
    """x after three V-cycles from zero, bit for bit with and without the fused up-stroke; the first cycle within 1e-5 of the fp64
    oracle's and the form the level reports (asserted in the child).  odd264: rag264's (28, 52, 264) box of liquid begun one
    cell later on every axis -- the regions' origins have the other parity, and with ragged regions every parity of (ci, cj, ck)
    occurs at a region's rim (the first and the last staged row of every axis).  edge264: two levels on a (12, 20, 264) grid, the
    least padding the hierarchy allows (two cells) and a one-cell shell -- the regions span cells 2 .. n - 3 of every axis, so the
    staged boxes begin at the coarse grid's row 0 (bi = 0) and end at its last row (bi + 1 = cn - 1, the cn - 2 bound of
    prolongAddKernel's clamp) on every axis; the coarsest level (6, 10, 132) keeps the dense factorisation small.  random: DIRICHLET cells scattered through the liquid, tests/test_fused_upstroke.py's domain at its
    only size -- with wsolid there (general cells: the loads from global memory stay) the fallback's yardstick."""
    with tempfile.TemporaryDirectory() as tmp:
        a1, a0 = (_run(case, f, os.path.join(tmp, f"r{f}.npy")) for f in ("1", "0"))
        assert np.array_equal(a1, a0), np.abs(a1 - a0).max()
