"""The up-stroke with the prolongation inside its Jacobi sweep (prolongJacobiPlaneKernel + the closure launch that reads
x + 4 P e, round 6).  By size only levels with 4 MiB x-y planes take it; MGPS_FUSE_UP=1 forces it onto every level where it is
valid, MGPS_FUSE_UP=0 keeps the separate prolongation pass.  Each domain runs in two child processes (the switch is read once
per process), and the results must be EQUAL: same lerps in the same order, same sweep epilogue."""
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
# optional: band_width,band_iterations,jacobi_weight for the solver and the oracle (default: the options' defaults)
band = None
if len(sys.argv) > 4:
    bw, bi, om = sys.argv[4].split(',')
    band = (int(bw), int(bi), float(om))


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


def stair(bl):
    bl[1:8, 1:12, 1:-1] = D.INTERIOR
    bl[1:16, 12:31, 1:-1] = D.INTERIOR


lev = 3
if case == 'cube':
    bl, bw = boxed((24, 24, 248), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 32, 256))
elif case in ('pool', 'wsolid'):
    bl, bw, _ = D.build_complex_domain((24, 32, 256), use_solid=case == 'wsolid')
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
elif case == 'stair':
    bl, bw = boxed((24, 32, 248), stair)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
elif case == 'rag264':
    bl, bw = boxed((20, 44, 248), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 264))
else:  # random labels: liquid with DIRICHLET cells scattered through it (every pocket of liquid touches one: not singular)
    def speckled(bl):
        bl[1:-1, 1:-1, 1:-1] = np.where(np.random.default_rng(3).random((22, 30, 246)) < 0.95, D.INTERIOR, D.DIRICHLET)
    bl, bw = boxed((24, 32, 248), speckled)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
opt = G.default_options()
okw = {}
if band:
    opt.band_width, opt.band_iterations, opt.jacobi_weight = band
    okw = dict(band_width=band[0], band_iterations=band[1], jacobi_weight=float(np.float32(band[2])))
s = G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=opt)
flags = [s.up_stroke_fused(l) for l in range(s.getMGLevels())]
assert s.stencil_kernel(0) == 'plane' and flags[0] == fused, (s.stencil_kernel(0), flags)
assert not any(flags[1:]), flags  # (level 1 is too narrow for plane blocks: the MG-PCG arm, whose level 0 gathers <z, r>, never fuses)
if fused and not band:  # where it must not run: Gauss-Seidel, binary16 fine level, 2 + 2 sweeps
    assert not G.GeometricMultigridPoissonSolver(lab, w, lev, True).up_stroke_fused(0)
    for name, value in (('precision', 1), ('post_sweeps', 2)):
        o = G.default_options()
        setattr(o, name, value)
        if name == 'post_sweeps':
            o.pre_sweeps = 2
        assert not G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=o).up_stroke_fused(0), name
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
for _ in range(3):
    s.applyVCycle(x, bd, True)
x6 = x.cpu().numpy()
assert np.all(x6[~act] == 0.0) and np.all(x3[~act] == 0.0)
ref = Oracle().solver(lab.astype(np.int32), [a.astype(np.float64) for a in w], lev, False, **okw)
xr = np.zeros(lab.shape)
ref.apply_vcycle(xr, b.astype(np.float64), False)
err = np.linalg.norm(x1 - xr) / np.linalg.norm(xr)
assert np.linalg.norm(xr) > 0 and err < 1e-5, err
xp = s.new_grid()
st = s.solveGeometricConjugateGradient(xp, bd, 1e-5, 200, True)
np.savez(out, x3=x3, x6=x6, xp=xp.cpu().numpy())
print('FUSED_UP_OK', json.dumps({'err': err, 'iterations': st['iterations'], 'outcome': st['outcome'], 'flags': flags}))
"""


def _run(case, fused, path, band=None):
    env = dict(os.environ, MGPS_FUSE_UP=fused, MGPS_STENCIL="plane")
    args = [case, fused, path] + ([band] if band else [])
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600, env=env)
    assert res.returncode == 0 and "FUSED_UP_OK" in res.stdout, res.stdout[-3000:]
    return json.loads(res.stdout.split("FUSED_UP_OK", 1)[1].strip().splitlines()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cube", "pool", "stair", "wsolid", "rag264", "random"])
def test_fused_upstroke_equals_separate_prolongation(case):
    """x after three V-cycles from zero and three more from that guess, and the MG-PCG solve, bit for bit with and without the
    fusion (ragged tiles in rag264: nx = 264 is not a multiple of 256, ny = 52 not one of 16; along z the march depth and nz are
    both even, so the last block of a column is short but never odd); both against the fp64 oracle's V-cycle; inactive cells
    exactly 0.  The fused child asserts up_stroke_fused(0) and not on the coarser levels, and that Gauss-Seidel, mixed precision
    and 2 + 2 keep the separate pass.  The MG-PCG arm therefore runs the separate pass in both children (level 0 of a
    preconditioning cycle gathers <z, r>): it checks that the switch leaves the solve alone, not the fused kernel."""
    with tempfile.TemporaryDirectory() as tmp:
        runs = {f: (_run(case, f, os.path.join(tmp, f"r{f}.npz")), np.load(os.path.join(tmp, f"r{f}.npz"))) for f in ("1", "0")}
        (m1, a1), (m0, a0) = runs["1"], runs["0"]
        for key in ("x3", "x6", "xp"):
            assert np.array_equal(a1[key], a0[key]), (key, np.abs(a1[key] - a0[key]).max())
        assert m1["iterations"] == m0["iterations"] and m1["outcome"] == m0["outcome"] == "converged", (m1, m0)


@pytest.mark.gpu
@pytest.mark.parametrize("band", ["2,2,0.8", "4,4,0.5"])
@pytest.mark.parametrize("case", ["wsolid", "random"])
def test_fused_upstroke_at_band_options(case, band):
    """The same at band_width, band_iterations, jacobi_weight = 2, 2, 0.8 and 4, 4, 0.5 (the closure launch of the fused up-stroke
    runs depth + 1 passes over the prolonged input and the sweep damps by the option's weight): bit for bit with and without the
    fusion, and the first cycle within 1e-5 of the oracle's at the same options (asserted in the child)."""
    with tempfile.TemporaryDirectory() as tmp:
        runs = {f: (_run(case, f, os.path.join(tmp, f"r{f}.npz"), band), np.load(os.path.join(tmp, f"r{f}.npz"))) for f in ("1", "0")}
        (m1, a1), (m0, a0) = runs["1"], runs["0"]
        assert m1["flags"][0] and not m0["flags"][0], (m1, m0)
        for key in ("x3", "x6", "xp"):
            assert np.array_equal(a1[key], a0[key]), (key, np.abs(a1[key] - a0[key]).max())
        assert m1["iterations"] == m0["iterations"] and m1["outcome"] == m0["outcome"] == "converged", (m1, m0)
