"""The down-stroke from an initial guess with its Jacobi sweep inside the x-folded residual march (SF_DOWN_FUSED, round 15:
closure launch, plain launch into the spare grid, jacobiResidualZKernel, downSeamFixKernel, restrictYKernel) against the separate
sweep and march of the same build (MGPS_FUSE_DOWN=0) and against the oracle.  The forms are forced onto small grids with
MGPS_STENCIL=plane MGPS_FUSE_RR=1 MGPS_RZ_XFOLD=1 MGPS_FUSE_DOWN=1; the switches are read once per process, so every setting runs
in a child process of its own.  mgps_down_stroke shows one stroke: x' and the coarse rhs.

x' must be EQUAL between the two (the march forms it with the sweep's expressions).  The coarse rhs takes the terms across the
tiles' rims after the folds instead of inside r: within 2e-6 of its maximum of the separate passes' (the project's bound between the
residual pair and the separate passes).

MEASURED on an MI355X, balanced inputs (tests/operator_bounds.py), worst error / bound over the seven cases, fused and
apart (bound = 1): x' against the oracle's stroke 0.21; the coarse rhs against the oracle's downsample(residual(x')) 0.045; fused
against apart per coarse cell 0.012 of twice the bound.

The numpy model at the end (no GPU) is the layout the fix-up kernel was written from: partial march + fix-up = the full formula."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import operator_bounds as OB
from conftest import ROOT

OP_TOL = 5e-6       # tests/test_rz_xfold.py
VCYCLE_TOL = 1e-5   # tests/test_gpu_parity.py
PAIR_TOL = 2e-6

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import geometricmultigridpressuresolver_amd as G
from geometricmultigridpressuresolver_amd import domains as D
from oracle.mg_oracle import Oracle

case, fuse, out, what = sys.argv[1], sys.argv[2] == '1', sys.argv[3], sys.argv[4]


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


# (tests/test_rz_xfold.py's domains restated; 3 levels: 4 cells of padding per side)
if case == 'seams776':    # three x-seams live on both sides, y-seams at 16 / 32 / 48, a last tile 8 cells wide
    bl, bw = boxed((20, 44, 768), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 776))
elif case == 'mid520':    # the active range begins and ends mid-wave, the last tile is dead
    bl, bw = boxed((20, 44, 512), middle)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 520))
elif case == 'stair520':  # blocks without active cells below / above / beside live ones
    bl, bw = boxed((24, 32, 512), stair)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 520))
elif case == 'rag264':    # ragged last tiles on every axis
    lab, w, off, lev = D.rag264()
elif case == 'tall264':   # 18 z-blocks (the launcher takes 4 planes per block at this size), y-seams at 16 / 32, one x-seam
    bl, bw = boxed((64, 28, 256), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(72, 36, 264))
elif case == 'ragz264':   # 2 levels, nz = 10: z-blocks of 4, 4 and 2 planes -- a ragged last one (three levels need nz %% 4 == 0)
    bl, bw = boxed((6, 16, 260), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=2, solver_shape=(10, 20, 264))
else:                     # wsolid: general BOUNDARY cells
    bl, bw, _ = D.build_complex_domain((24, 32, 256), use_solid=True)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
act = D.active_mask(lab)
dx = 1.0 / lab.shape[2]
s = G.GeometricMultigridPoissonSolver(lab, w, lev, False)
assert s.stencil_kernel(0) == 'plane' and s.residual_restrict_fused(0), (s.stencil_kernel(0), s.residual_restrict_fused(0))
# the switch was live: the level reports the form the child was started for -- never on a level with general cells, never below level 0's size rules
took = s.down_stroke_fused(0)
assert took == (fuse and case != 'wsolid'), (case, fuse, took)
kept = s.level_array(0, 'kept_tiles')
assert (kept.size > 0) == took, (kept.size, took)
if took:
    nbx = (lab.shape[2] + 255) // 256
    assert kept.size == lab.shape[0] * lab.shape[1] * nbx and kept.any()
lab32, w64 = lab.astype(np.int32), [a.astype(np.float64) for a in w]
rng = np.random.default_rng(15)
res = {}
if what != 'cycles':
    x0 = np.where(act, rng.standard_normal(lab.shape), 0.0).astype(np.float32)
    b0 = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    bd = s.to_device(b0)

    def stroke():
        xd, cd = s.to_device(x0), s.new_grid(1)
        s.downStroke(xd, cd, bd, 0)
        return xd.cpu().numpy(), cd.cpu().numpy()

    xs, coarse = stroke()
    assert np.isfinite(xs).all() and np.isfinite(coarse).all()
    assert np.all(xs[~act] == 0.0) and np.count_nonzero(xs) > 0
    orc = Oracle()
    r = np.zeros(lab.shape)
    orc.residual(r, xs.astype(np.float64), b0.astype(np.float64), lab32, w64)
    lab1 = s.hierarchy().level_labels(1).astype(np.int32)
    ref = np.zeros(lab1.shape)
    orc.downsample(ref, r, lab1)
    err = np.abs(coarse - ref).max() / np.abs(ref).max()
    print('err', err)
    if case != 'wsolid':  # (where tests/test_rz_xfold.py asserts it)
        assert np.abs(ref).max() > 0 and err < %(op_tol)r, err
    xs2, coarse2 = stroke()  # a second call: the same bits
    assert np.array_equal(xs2, xs) and np.array_equal(coarse2, coarse)
    np.save(out, np.concatenate([xs.ravel(), coarse.ravel()]))
    res['err'] = float(err)
    # per cell on balanced inputs (tests/operator_bounds.py; the weights as the float32 values the device holds): x' against the
    # oracle's stroke -- three band passes, the sweep, three band passes, every pass's bound carried through the later ones -- and
    # the coarse rhs against the oracle's downsample(residual(x')) of the device's own x'
    import operator_bounds as OB
    wf = [OB.as_f32(a) for a in w]
    st = OB.Stencil(lab, wf)
    xb, bb = OB.balanced_inputs(lab, wf, 115, st)
    xbd, cbd = s.to_device(xb), s.new_grid(1)
    s.downStroke(xbd, cbd, s.to_device(bb), 0)
    xsb, cb = xbd.cpu().numpy(), cbd.cpu().numpy()
    xref, e = OB.smooth_stroke(st, orc, xb, bb, lab32, orc.build_boundary_cells(lab32, 3), wf)
    tag = 'downstroke %%s fused=%%d ' %% (case, fuse)
    res['x'] = OB.assert_within(tag + "x'", xsb, xref, e)
    rb = np.zeros(lab.shape)
    orc.residual(rb, xsb.astype(np.float64), bb, lab32, wf)
    refb = np.zeros(lab1.shape)
    orc.downsample(refb, rb, lab1)
    bound = OB.bound_residual_restrict(st, xsb, bb, lab1)
    res['coarse'] = OB.assert_within(tag + 'coarse rhs', cb, refb, bound)
    np.savez(out + '.balanced.npz', x=xsb, coarse=cb, bound=bound)
else:
    b = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    bd = s.to_device(b)
    x = s.new_grid()
    ref = Oracle().solver(lab32, w64, lev, False)
    xr = np.zeros(lab.shape)
    b64 = b.astype(np.float64)
    errs = []
    for it in range(3):
        s.applyVCycle(x, bd, True)
        ref.apply_vcycle(xr, b64, True)
        e = np.linalg.norm(x.cpu().numpy() - xr) / np.linalg.norm(xr)
        print('cycle', it, e)
        assert np.linalg.norm(xr) > 0 and e < %(vcycle_tol)r * (it + 1), (it, e)
        errs.append(float(e))
    got = x.cpu().numpy()
    assert np.all(got[~act] == 0.0)
    np.save(out, got)
    res['errs'] = errs
print('FUSE_DOWN_OK', json.dumps(res))
"""


def _run(case, fuse, path, what="operator", poison=False):
    env = dict(os.environ, MGPS_FUSE_RR="1", MGPS_STENCIL="plane", MGPS_RZ_XFOLD="1", MGPS_FUSE_DOWN=fuse)
    if poison:
        env["MGPS_POISON_SPARES"] = "1"
    code = CHILD % {"root": ROOT, "op_tol": OP_TOL, "vcycle_tol": VCYCLE_TOL}
    res = subprocess.run([sys.executable, "-c", code, case, fuse, path, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=600, env=env)
    assert res.returncode == 0 and "FUSE_DOWN_OK" in res.stdout, res.stdout[-3000:]
    print("".join(line for line in res.stdout.splitlines(True) if line.startswith("PERCELL")), end="")
    if os.path.exists(path + ".balanced.npz"):  # the operator child's stroke on balanced inputs
        with np.load(path + ".balanced.npz") as z:
            BALANCED[(case, fuse)] = {k: z[k] for k in z.files}
    return np.load(path)


BALANCED = {}  # (case, MGPS_FUSE_DOWN) -> x', coarse rhs and the coarse rhs's per-cell bound of the last operator child


def _both(case, what="operator"):
    with tempfile.TemporaryDirectory() as tmp:
        return [_run(case, f, os.path.join(tmp, f"c{f}.npy"), what) for f in ("1", "0")]


def _fine_cells(case):
    return {"seams776": 28 * 52 * 776, "mid520": 28 * 52 * 520, "stair520": 32 * 40 * 520, "rag264": 28 * 52 * 264, "tall264": 72 * 36 * 264,
            "ragz264": 10 * 20 * 264, "wsolid": 32 * 40 * 264}[case]


def _compare(case, fused, apart):
    n = _fine_cells(case)
    assert np.array_equal(fused[:n], apart[:n]), (int((fused[:n] != apart[:n]).sum()), float(np.abs(fused[:n] - apart[:n]).max()))
    d, m = float(np.abs(fused[n:] - apart[n:]).max()), float(np.abs(apart[n:]).max())
    print(case, "coarse rhs: max |fused - apart|", d, "max |apart|", m, "ratio", d / m)
    assert m > 0 and d <= PAIR_TOL * m, (d, m)
    # on balanced inputs: x' equal again, the coarse rhs per coarse cell within twice the per-cell bound (both sides carry it)
    f, a = BALANCED[(case, "1")], BALANCED[(case, "0")]
    assert np.array_equal(f["x"], a["x"]), (int((f["x"] != a["x"]).sum()), float(np.abs(f["x"] - a["x"]).max()))
    OB.assert_within(f"downstroke {case} fused against apart, coarse rhs", f["coarse"], a["coarse"], 2.0 * a["bound"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seams776", "mid520", "stair520", "rag264", "tall264", "ragz264"])
def test_fused_down_stroke_equals_sweep_then_march(case):
    """One down-stroke through mgps_down_stroke on a random guess and rhs, MGPS_FUSE_DOWN=1 against =0: x' bit for bit, inactive
    cells exactly 0, the coarse rhs within 2e-6 of its maximum; in each child the coarse rhs within 5e-6 of the oracle's
    downsample(residual(x')), a second call with the same bits, and the level reports the form the child was started for (with its
    kept-quad words made or not).  The same stroke on balanced inputs (tests/operator_bounds.py): in each child x' per cell against
    the oracle's stroke and the coarse rhs per coarse cell against the oracle's downsample(residual(x')); here x' bit for bit and
    the coarse rhs of the two forms within twice the per-cell bound in every coarse cell.  seams776 / mid520 / stair520: tests/test_rz_xfold.py's domains; rag264: ragged last tiles on every
    axis; tall264: solver shape (72, 36, 264), liquid from one cell inside the padding -- 18 z-blocks of 4 planes (the block depth
    the launcher takes at this size); ragz264: (10, 20, 264), two levels, z-blocks of 4, 4 and 2 planes."""
    fused, apart = _both(case)
    _compare(case, fused, apart)


@pytest.mark.gpu
def test_general_cells_keep_sweep_and_march_apart():
    """wsolid (general BOUNDARY cells: the level keeps the full-resolution residual layout): the level reports the form as not taken
    whatever the switch says (asserted in the child), and the switch moves no bit."""
    a, b = _both("wsolid")
    assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.gpu
def test_nothing_stale_is_read_from_the_spare_grid():
    """seams776 with MGPS_POISON_SPARES=1 (the spare grid starts as NaN on every active cell): the fused stroke reads it in kept
    quads alone, where the plain launch has written -- the same bits as without the poison, all finite."""
    with tempfile.TemporaryDirectory() as tmp:
        clean = _run("seams776", "1", os.path.join(tmp, "a.npy"))
        poisoned = _run("seams776", "1", os.path.join(tmp, "b.npy"), poison=True)
    assert np.isfinite(poisoned).all() and np.array_equal(clean, poisoned)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seams776", "tall264"])
def test_three_vcycles_with_an_initial_guess(case):
    """Three V-cycles with useInitialGuess (level 0's down-stroke takes the fused form in one child, sweep and march in the other):
    each within VCYCLE_TOL * (cycle + 1) of the fp64 oracle's (asserted in the child), inactive cells exactly 0; the two
    iterates within the same bound of each other."""
    fused, apart = _both(case, "cycles")
    assert np.linalg.norm(fused - apart) <= VCYCLE_TOL * 3 * np.linalg.norm(apart)


# ---------------------------------------------------------------------------------------------
# The layout of the march's partial residual and the fix-up, in numpy (no GPU).  r = b - (diag x - sum of the six neighbours) on
# active cells.  The march of tile (bx, by) takes x' of cells outside the tile as 0; its z-blocks form r on k0 - 1 .. k1 and store
# coarse planes k0 / 2 .. k1 / 2 - 1, folded along z (w = 1, 3, 3, 1 over 8) and along x: columns inside a tile into rzx, the two
# columns astride a tile boundary from the seam array (eight floats per row, coarse plane and boundary: the z-folded quads on either
# side).  The fix-up adds, per live block, the rim rows' terms into rzx and the seam quads, and the rim columns' terms into `.w` of
# side 0 / `.x` of side 1.  restrict_y then reads what restrictYKernel reads.
# ---------------------------------------------------------------------------------------------
W = np.array([0.125, 0.375, 0.375, 0.125])
TX, TY = 256, 16


def _fold_x_full(rzf):
    """coarse column I = sum_a W[a] rz(2 I - 1 + a), zero outside the grid"""
    nz, ny, nx = rzf.shape
    p = np.zeros((nz, ny, nx + 4))
    p[:, :, 1:nx + 1] = rzf
    return sum(W[a] * p[:, :, a:a + nx:2][:, :, :nx // 2] for a in range(4))


def _model(nz, ny, nx, zc, xlo, xhi, dead, seed):
    rng = np.random.default_rng(seed)
    act = np.zeros((nz, ny, nx), bool)
    act[1:-1, 1:-1, xlo + 1:xhi - 1] = True
    nbx, nby, nbz = -(-nx // TX), -(-ny // TY), -(-nz // zc)
    for (bz, by, bx) in dead:  # tiles without active cells: off the block list
        act[bz * zc:(bz + 1) * zc, by * TY:(by + 1) * TY, bx * TX:(bx + 1) * TX] = False
    live = [(bz, by, bx) for bz in range(nbz) for by in range(nby) for bx in range(nbx)
            if act[bz * zc:(bz + 1) * zc, by * TY:(by + 1) * TY, bx * TX:(bx + 1) * TX].any()]
    xs = np.where(act, rng.standard_normal(act.shape), 0.0)
    b = np.where(act, rng.standard_normal(act.shape), 0.0)

    def residual(x, tile=None):
        p = np.zeros((nz + 2, ny + 2, nx + 2))
        p[1:-1, 1:-1, 1:-1] = x
        if tile is not None:  # nothing of x' outside the tile's x-y footprint
            by, bx = tile
            m = np.zeros_like(p, bool)
            m[:, 1 + by * TY:1 + min((by + 1) * TY, ny), 1 + bx * TX:1 + min((bx + 1) * TX, nx)] = True
            p = np.where(m, p, 0.0)
        nb = p[:-2, 1:-1, 1:-1] + p[2:, 1:-1, 1:-1] + p[1:-1, :-2, 1:-1] + p[1:-1, 2:, 1:-1] + p[1:-1, 1:-1, :-2] + p[1:-1, 1:-1, 2:]
        return np.where(act, b - (6.0 * x - nb), 0.0)

    def fold_z(r, K):  # coarse plane K from planes 2 K - 1 .. 2 K + 2 inside the grid
        return sum(W[c] * r[2 * K - 1 + c] for c in range(4) if 0 <= 2 * K - 1 + c < nz)

    full = residual(xs)
    rz_full = np.stack([fold_z(full, K) for K in range(nz // 2)])
    want = _fold_x_full(rz_full)  # what restrict_y must see in every column

    nseam = nbx - 1
    rzx = np.zeros((nz // 2, ny, nx // 2))
    seam = np.zeros((nz // 2, ny, max(nseam, 1), 8))
    gate = act  # (simple cells: every active one)
    for (bz, by, bx) in live:
        k0, k1 = bz * zc, min((bz + 1) * zc, nz)
        j0, j1, i0, i1 = by * TY, min((by + 1) * TY, ny), bx * TX, min((bx + 1) * TX, nx)
        part = residual(xs, (by, bx))
        for K in range(k0 // 2, k1 // 2):
            v = np.zeros((ny, nx))
            v[j0:j1, i0:i1] = fold_z(part, K)[j0:j1, i0:i1]  # the tile's z-folded quads, 0 in lanes that own none
            # the march's stores: every lane of the tile folds (left lane's .w, x, y, z) and (y, z, w, right lane's .x), 0 past the wave
            pad = np.zeros((ny, (i1 - i0) + 4))
            pad[:, 1:1 + i1 - i0] = v[:, i0:i1]
            fx = sum(W[a] * pad[:, a:a + (i1 - i0):2][:, :(i1 - i0) // 2] for a in range(4))
            rzx[K, j0:j1, i0 // 2:i1 // 2] = fx[j0:j1]
            if bx > 0:
                seam[K, j0:j1, bx - 1, 4:8] = v[j0:j1, i0:i0 + 4]
            if i1 < nx:
                seam[K, j0:j1, bx, 0:4] = v[j0:j1, i1 - 4:i1]
    for bz in range(nbz):  # residualZEdgeKernel: a block off the list below / above a live one owes one plane of terms, complete r from memory
        for by in range(nby):
            for bx in range(nbx):
                if (bz, by, bx) in live:
                    continue
                k0, k1 = bz * zc, min((bz + 1) * zc, nz)
                j0, j1, i0, i1 = by * TY, min((by + 1) * TY, ny), bx * TX, min((bx + 1) * TX, nx)
                for (other, k, K, wz) in (((bz - 1, by, bx), k0 - 1, k0 // 2, W[0]), ((bz + 1, by, bx), k1, k1 // 2 - 1, W[3])):
                    if other not in live:
                        continue
                    v = wz * full[k, :, i0:i1]
                    pad = np.zeros((ny, (i1 - i0) + 4))
                    pad[:, 1:1 + i1 - i0] = v
                    fx = sum(W[a] * pad[:, a:a + (i1 - i0):2][:, :(i1 - i0) // 2] for a in range(4))
                    rzx[K, j0:j1, i0 // 2:i1 // 2] = fx[j0:j1]
                    if bx > 0:
                        seam[K, j0:j1, bx - 1, 4:8] = v[j0:j1, 0:4]
                    if i1 < nx:
                        seam[K, j0:j1, bx, 0:4] = v[j0:j1, -4:]
    for (bz, by, bx) in live:  # the fix-up, block by block like the kernel
        k0, k1 = bz * zc, min((bz + 1) * zc, nz)
        j0, j1, i0, i1 = by * TY, min((by + 1) * TY, ny), bx * TX, min((bx + 1) * TX, nx)
        for K in range(k0 // 2, k1 // 2):
            for (j, jn) in ((j0, j0 - 1), (j0 + TY - 1, j0 + TY)):  # rim rows
                if jn < 0 or jn >= ny:
                    continue
                v = np.zeros(nx)
                for c in range(4):
                    k = 2 * K - 1 + c
                    if 0 <= k < nz:
                        v[i0:i1] += W[c] * np.where(gate[k, j, i0:i1], xs[k, jn, i0:i1], 0.0)
                pad = np.zeros((i1 - i0) + 4)
                pad[1:1 + i1 - i0] = v[i0:i1]
                fx = sum(W[a] * pad[a:a + (i1 - i0):2][:(i1 - i0) // 2] for a in range(4))
                rzx[K, j, i0 // 2:i1 // 2] += fx
                if bx > 0:
                    seam[K, j, bx - 1, 4:8] += v[i0:i0 + 4]
                if i1 < nx:
                    seam[K, j, bx, 0:4] += v[i1 - 4:i1]
            for j in range(j0, j1):  # rim columns
                for (i, inb, s, slot) in ((i0, i0 - 1, bx - 1, 4), (i0 + TX - 1, i0 + TX, bx, 3)):
                    if inb < 0 or inb >= nx:
                        continue
                    t = sum(W[c] * (xs[2 * K - 1 + c, j, inb] if gate[2 * K - 1 + c, j, i] else 0.0) for c in range(4) if 0 <= 2 * K - 1 + c < nz)
                    seam[K, j, s, slot] += t
    # what restrictYKernel reads: rzx, but columns 128 s - 1 and 128 s from the seam entries
    got = rzx.copy()
    for s in range(1, nseam + 1):
        e = seam[:, :, s - 1, :]
        got[:, :, 128 * s - 1] = e[:, :, 1:5] @ W  # fine 256 s - 3 .. 256 s
        got[:, :, 128 * s] = e[:, :, 3:7] @ W      # fine 256 s - 1 .. 256 s + 2
    return got, want, act, live


@pytest.mark.parametrize("name,args", [
    ("ragged", dict(nz=10, ny=36, nx=520, zc=4, xlo=0, xhi=520, dead=[])),                 # ragged last tile on every axis, three z-blocks
    ("midwave", dict(nz=12, ny=32, nx=776, zc=4, xlo=68, xhi=700, dead=[])),               # the range begins and ends mid-wave
    ("dead", dict(nz=12, ny=48, nx=776, zc=4, xlo=0, xhi=776, dead=[(1, 1, 1), (0, 2, 2), (2, 0, 0), (1, 1, 2)])),  # dead tiles on either side of a boundary
])
def test_numpy_model_partial_march_plus_fixup_is_the_full_fold(name, args):
    """The march's partial residual (nothing of x' outside the tile) folded along z and x into rzx and the seam entries, plus the
    fix-up's rim-row and rim-column terms, gives the full residual's folds in every column restrictYKernel reads.  A block
    off the list is not touched by either (its own r is 0); residualZEdgeKernel stores the plane of terms it owes a live block
    below or above, complete from memory.  Ragged last tiles on every axis, a range that begins and ends mid-wave, dead tiles on either side of a
    boundary, three z-blocks with a ragged last one."""
    got, want, act, live = _model(seed=3, **args)
    assert len(live) > 2 and np.abs(want).max() > 0
    assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max()), float(np.abs(got - want).max())
