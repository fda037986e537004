"""Plain quads (GridP::plainQ / plainT): one bit per quad of four cells along x, set where all four cell codes are INTERIOR.  The
plane marches (stencilPlaneKernel, residualZKernel, prolongJacobiPlaneKernel) take the codes of such a quad as 0 and do not load
them; levels with plane blocks have the arrays.  MGPS_PLAIN_QUADS=0 leaves them out and every code is loaded: the two must give
the SAME bits everywhere.  The switch is read once per process, so every arm runs in a child process of its own; the marches are
forced onto the small domains with MGPS_STENCIL=plane MGPS_FUSE_RR=1 MGPS_FUSE_UP=1.  The quad kernel does not read the bits
(LABNOTES R11): its arm and the binary16 case hold that the switch moves nothing there either.

MEASURED on an MI355X, balanced inputs (tests/operator_bounds.py), worst error / bound against the fp64 oracle over the four
cases, both arms, switch on and off (bound = 1): A x 0.39, residual 0.30, Jacobi sweep 0.20, residual + restriction 0.046."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

VCYCLE_TOL = 1e-5   # tests/test_gpu_parity.py
MARCHES = dict(MGPS_STENCIL="plane", MGPS_FUSE_RR="1", MGPS_FUSE_UP="1")
QUAD = dict(MGPS_STENCIL="quad")
CASES = ["seams776", "mid520", "wsolid", "speckled"]

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import geometricmultigridpressuresolver_amd as G
from geometricmultigridpressuresolver_amd import domains as D
from oracle.mg_oracle import Oracle

case, on, out, mode, marches = sys.argv[1], sys.argv[2] == '1', sys.argv[3], sys.argv[4], sys.argv[5] == '1'


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


def speckled(bl):  # tests/test_fused_upstroke.py: DIRICHLET cells scattered through the liquid -- quads that are partly INTERIOR
    bl[1:-1, 1:-1, 1:-1] = np.where(np.random.default_rng(3).random((22, 30, 246)) < 0.95, D.INTERIOR, D.DIRICHLET)


if case == 'seams776':    # tests/test_rz_xfold.py: rows of 194 quads, a last tile two quads wide
    bl, bw = boxed((20, 44, 768), inner)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 776))
elif case == 'mid520':    # the active range begins and ends in the middle of a wave, the last tile is dead
    bl, bw = boxed((20, 44, 512), middle)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(28, 52, 520))
elif case == 'wsolid':    # free surface + cut-cell solid: general BOUNDARY cells
    bl, bw, _ = D.build_complex_domain((24, 32, 256), use_solid=True)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
else:
    bl, bw = boxed((24, 32, 248), speckled)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=3, solver_shape=(32, 40, 264))
act = D.active_mask(lab)
dx = 1.0 / lab.shape[2]
opt = G.default_options()
if mode == 'half':
    opt.precision = 1
s = G.GeometricMultigridPoissonSolver(lab, w, lev, False, options=opt)
if marches:  # the switch was live (the fine level has the arrays or it has not) and the arm ran the kernels it is about
    assert (s.level_array(0, 'plain_quads').size > 0) == on, (on, s.level_array(0, 'plain_quads').size)
    assert (s.level_array(0, 'plain_tiles').size > 0) == on, (on, s.level_array(0, 'plain_tiles').size)
    assert s.stencil_kernel(0) == 'plane' and s.residual_restrict_fused(0), (s.stencil_kernel(0), s.residual_restrict_fused(0))
    assert mode == 'half' or s.up_stroke_fused(0)
elif mode != 'build':
    assert s.stencil_kernel(0) == 'quad', s.stencil_kernel(0)
lab32, w64 = lab.astype(np.int32), [a.astype(np.float64) for a in w]
rng = np.random.default_rng(5)
res = {}
if mode == 'build':
    counts = []
    for l in range(s.getMGLevels()):
        codes = s.level_array(l, 'codes')
        got = s.level_array(l, 'plain_quads')
        tiles = s.level_array(l, 'plain_tiles')
        nz, ny, nx = s.level_shape(l)
        if not on or nx %% 4 or nx < 256 or ny < 16:  # (levels without plane blocks -- planeSweepZc -- keep none)
            assert got.size == 0 and tiles.size == 0, (l, got.size, tiles.size)
            counts.append(None)
            continue
        plain = (codes.reshape(-1, 4) == 0).all(axis=1)
        bits = np.zeros((plain.size + 31) // 32 * 32, dtype=np.uint8)
        bits[:plain.size] = plain
        want = np.packbits(bits, bitorder='little').view(np.uint32)
        assert got.shape == want.shape and np.array_equal(got, want), (l, got.shape, want.shape, int((got != want).sum()))
        # the marches' copy, as plainTilesKernel left it on the device: bit l of word (row, tile) = the quad at x = 256 tile + 4 l
        nq, nbx = nx // 4, (nx + 255) // 256
        padded = np.zeros((nz * ny, nbx * 64), dtype=np.uint8)
        padded[:, :nq] = plain.reshape(nz * ny, nq)
        want_t = np.packbits(padded, axis=1, bitorder='little').view(np.uint64).reshape(-1)
        assert tiles.shape == want_t.shape and np.array_equal(tiles, want_t), (l, tiles.shape, want_t.shape, int((tiles != want_t).sum()))
        counts.append((int(plain.sum()), int(plain.size)))
    if on:
        assert 0 < counts[0][0] < counts[0][1], counts  # both kinds of quad on the fine level
    res['counts'] = counts
    np.save(out, np.zeros(1))
elif mode == 'ops':
    x0 = rng.standard_normal(lab.shape).astype(np.float32)  # (non-zero in inactive cells too)
    b0 = (rng.standard_normal(lab.shape) * dx * dx).astype(np.float32)
    xd, bd = s.to_device(x0), s.to_device(b0)
    sm = xd.clone()
    s.jacobiPoissonSmoother(sm, bd)
    r = s.new_grid()
    s.computePoissonResidual(r, xd, bd)
    ax = s.new_grid()
    s.applyPoissonMatrix(ax, xd)
    cd = s.new_grid(1)
    s.residualDownsample(cd, xd, bd, 0)
    # the same operators on balanced inputs (tests/operator_bounds.py), each against the fp64 oracle per cell; the results join the
    # arrays the two arms must agree on bit for bit
    import operator_bounds as OB
    orc = Oracle()
    wf = [OB.as_f32(a) for a in w]
    st = OB.Stencil(lab, wf)
    xb, bb = OB.balanced_inputs(lab, wf, 105, st)
    xbd, bbd = s.to_device(xb), s.to_device(bb)
    tag = 'plain_quads %%s %%s on=%%d ' %% (case, 'marches' if marches else 'quad', on)
    smb = xbd.clone()
    s.jacobiPoissonSmoother(smb, bbd)
    ref = xb.copy()
    orc.jacobi(ref, bb, lab32, wf)
    OB.assert_within(tag + 'jacobi', smb.cpu().numpy(), ref, OB.bound_jacobi(st, xb, bb))
    rb = s.new_grid()
    s.computePoissonResidual(rb, xbd, bbd)
    rref = np.zeros(lab.shape)
    orc.residual(rref, xb, bb, lab32, wf)
    OB.assert_within(tag + 'residual', rb.cpu().numpy(), rref, OB.bound_residual(st, xb, bb))
    axb = s.new_grid()
    s.applyPoissonMatrix(axb, xbd)
    ref = np.zeros(lab.shape)
    orc.apply_poisson(ref, xb, lab32, wf)
    OB.assert_within(tag + 'apply', axb.cpu().numpy(), ref, OB.bound_apply(st, xb))
    cdb = s.new_grid(1)
    s.residualDownsample(cdb, xbd, bbd, 0)
    lab1 = s.hierarchy().level_labels(1).astype(np.int32)
    ref = np.zeros(lab1.shape)
    orc.downsample(ref, rref, lab1)
    OB.assert_within(tag + 'residual+restriction', cdb.cpu().numpy(), ref, OB.bound_residual_restrict(st, xb, bb, lab1))
    np.savez(out, sm=sm.cpu().numpy(), r=r.cpu().numpy(), ax=ax.cpu().numpy(), cd=cd.cpu().numpy(),
             smb=smb.cpu().numpy(), rb=rb.cpu().numpy(), axb=axb.cpu().numpy(), cdb=cdb.cpu().numpy())
elif mode in ('cycles', 'half'):
    b = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    bd = s.to_device(b)
    x = s.new_grid()
    ref = Oracle().solver(lab32, w64, lev, False) if mode == 'cycles' and on else None  # (the other arm must equal this one)
    xr = np.zeros(lab.shape)
    b64 = b.astype(np.float64)
    errs = []
    for it in range(3):
        s.applyVCycle(x, bd, it > 0)
        if ref:
            ref.apply_vcycle(xr, b64, it > 0)
            e = np.linalg.norm(x.cpu().numpy() - xr) / np.linalg.norm(xr)
            print('cycle', it, e)
            assert np.linalg.norm(xr) > 0 and e < %(vcycle_tol)r * (it + 1), (it, e)
            errs.append(float(e))
    got = x.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(got[~act] == 0.0)
    xp = s.new_grid()
    if mode == 'cycles':
        st = s.solveGeometricConjugateGradient(xp, bd, 1e-5, 200, True)
        res['iterations'] = st['iterations']
    np.savez(out, x=got, xp=xp.cpu().numpy())
    res['errs'] = errs
else:  # 'zero': one cycle from zero (with or without MGPS_POISON_SPARES in the environment)
    b = np.where(act, rng.standard_normal(lab.shape) * dx * dx, 0.0).astype(np.float32)
    x = s.new_grid()
    s.applyVCycle(x, s.to_device(b), False)
    got = x.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.abs(got).max() > 0
    np.savez(out, x=got)
print('PLAIN_QUADS_OK', json.dumps(res))
"""


def _run(case, on, path, mode, env_extra, marches):
    env = dict(os.environ, MGPS_PLAIN_QUADS=on, **env_extra)
    code = CHILD % {"root": ROOT, "vcycle_tol": VCYCLE_TOL}
    res = subprocess.run([sys.executable, "-c", code, case, on, path, mode, "1" if marches else "0"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "PLAIN_QUADS_OK" in res.stdout, res.stdout[-3000:]
    print("".join(line for line in res.stdout.splitlines(True) if line.startswith("PERCELL")), end="")
    info = json.loads(res.stdout.split("PLAIN_QUADS_OK", 1)[1].strip().splitlines()[0])
    return np.load(path), info


def _both(case, mode, env_extra, marches):
    with tempfile.TemporaryDirectory() as tmp:
        out = []
        for on in ("1", "0"):
            data, info = _run(case, on, os.path.join(tmp, f"p{on}.npz" if mode != "build" else f"p{on}.npy"), mode, env_extra, marches)
            out.append(({k: data[k] for k in data.files} if mode != "build" else None, info))
        return out


def _assert_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_builder_matches_the_codes(case):
    """On every level level_array(l, 'plain_quads') and level_array(l, 'plain_tiles') -- the copy the marches read -- equal the bits
    numpy forms from level_array(l, 'codes') (asserted in the child; levels without plane blocks keep neither); the fine level
    holds both kinds of quad; MGPS_PLAIN_QUADS=0: no level has the arrays."""
    (_, on), (_, off) = _both(case, "build", MARCHES, True)
    assert on["counts"][0] is not None and all(c is None for c in off["counts"]), (on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["quad", "marches"])
@pytest.mark.parametrize("case", CASES)
def test_operators_equal_with_and_without_the_bits(case, arm):
    """mgps_jacobi_smooth, mgps_residual, mgps_apply_poisson and mgps_residual_downsample on a random x (non-zero in inactive cells
    too) and a random rhs: the same bits with the switch on and off, through the marches (which read the bits) and through the quad
    kernel (which does not).  The same four on balanced inputs: the same bits again, and in each child every one within its per-cell
    bound of the fp64 oracle (tests/operator_bounds.py) -- the arms' only comparison with anything but each other."""
    (a, _), (b, _) = _both(case, "ops", QUAD if arm == "quad" else MARCHES, arm == "marches")
    _assert_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seams776", "wsolid", "speckled"])
def test_cycles_and_pcg_equal_and_match_the_oracle(case):
    """Three V-cycles from zero and one MG-PCG solve (1e-5), marches forced (the child asserts stencil_kernel(0) == 'plane',
    residual_restrict_fused(0) and up_stroke_fused(0)): x equal bit for bit between on and off, each cycle within
    1e-5 * (cycle + 1) of the fp64 oracle (asserted in the child with the bits on; the other arm is equal to it), inactive cells
    exactly 0."""
    (a, ia), (b, ib) = _both(case, "cycles", MARCHES, True)
    _assert_equal(a, b)
    assert ia["iterations"] == ib["iterations"], (ia, ib)


@pytest.mark.gpu
def test_zero_start_cycle_reads_no_poisoned_spare():
    """A zero-start cycle with MGPS_POISON_SPARES=1 (NaN in the grids such a stroke neither clears nor may read), switch on, marches
    forced: finite (asserted in the child) and equal to the unpoisoned result."""
    with tempfile.TemporaryDirectory() as tmp:
        p, _ = _run("seams776", "1", os.path.join(tmp, "p.npz"), "zero", dict(MARCHES, MGPS_POISON_SPARES="1"), True)
        q, _ = _run("seams776", "1", os.path.join(tmp, "q.npz"), "zero", MARCHES, True)
        assert np.array_equal(p["x"], q["x"])


@pytest.mark.gpu
def test_binary16_cycles_equal():
    """options.precision = 1 on seams776 (stencilQuadKernel's binary16 instances, which do not read the bits): three V-cycles, on
    and off equal."""
    (a, _), (b, _) = _both("seams776", "half", {}, False)
    _assert_equal(a, b)


# ---- on the host: the two layouts against the flat definition ---------------------------------------------------------------------
def _flat_words(plain):
    """plainQuadsKernel: a wave takes 64 consecutive quads and stores their ballot as two words."""
    groups = (plain.size + 63) // 64
    words = np.zeros(2 * groups, dtype=np.uint32)
    for g in range(groups):
        chunk = plain[64 * g:64 * g + 64]
        v = sum(1 << l for l in range(chunk.size) if chunk[l])
        words[2 * g], words[2 * g + 1] = v & 0xffffffff, v >> 32
    return words


def _tile_words(words, nq, nbx, rows):
    """plainTilesKernel: the 64 bits that start at the tile's first quad, cut from three words of the flat layout."""
    out = []
    for t in range(rows * nbx):
        row, tile = divmod(t, nbx)
        left = nq - tile * 64
        q0 = row * nq + tile * 64
        w0, sh = q0 >> 5, q0 & 31
        a = int(words[w0])
        b = int(words[w0 + 1]) if w0 + 1 < words.size else 0
        c = int(words[w0 + 2]) if w0 + 2 < words.size else 0
        v = ((a | (b << 32)) >> sh) | ((c << (64 - sh)) if sh else 0)
        v &= (1 << 64) - 1
        if left < 64:
            v &= (1 << left) - 1
        out.append(v)
    return out


@pytest.mark.parametrize("nx,lo,hi", [(776, 5, 771), (520, 68, 452), (264, 4, 260), (256, 0, 256), (40, 9, 30)])
def test_layouts_against_the_flat_definition(nx, lo, hi):
    """numpy model of both layouts on rows of nx cells whose liquid is [lo, hi): rows whose quad count is no multiple of 64 (194,
    130, 66, 10), a range that begins in the middle of a wave, a dead last tile (520: tile 2 holds 8 EXTERIOR cells).  Flat: bit
    q & 31 of word q >> 5 is quad q's.  Tiles: bit l of word (row, tile) is the quad at x = 256 tile + 4 l, 0 past the row's end."""
    rows, nq, nbx = 7, nx // 4, (nx + 255) // 256
    rng = np.random.default_rng(nx)
    codes = np.ones((rows, nx), dtype=np.uint8)  # EXTERIOR
    codes[:, lo:hi] = 0
    codes[:, lo] = codes[:, hi - 1] = 5  # the row's end cells: simple BOUNDARY codes
    codes[rng.random(codes.shape) < 0.02] = 2  # a few DIRICHLET cells anywhere
    plain = (codes.reshape(-1, 4) == 0).all(axis=1)
    words = _flat_words(plain)
    for q in range(plain.size):
        assert ((int(words[q >> 5]) >> (q & 31)) & 1) == int(plain[q]), q
    assert not any((int(words[q >> 5]) >> (q & 31)) & 1 for q in range(plain.size, 32 * words.size))
    tiles = _tile_words(words, nq, nbx, rows)
    for row in range(rows):
        for tile in range(nbx):
            for lane in range(64):
                x = 256 * tile + 4 * lane
                want = int(plain[row * nq + x // 4]) if x < nx else 0
                assert ((tiles[row * nbx + tile] >> lane) & 1) == want, (row, tile, lane)
    if nx == 520:
        assert all(tiles[row * nbx + 2] == 0 for row in range(rows))  # the dead tile
