"""Per-cell rounding bounds for the solver's HIP operators, and inputs on which every term of an operator counts.

Plain numpy in fp64, no GPU, not a conftest.  Four things:

  * balanced, signed inputs of a level: x uniform in (-1, 1) on active cells, b uniform in (-1, 1) times the cell's diagonal -- of
    the size of A x in ghost-fluid cells (diagonal of order 100) and INTERIOR cells (diagonal 6) alike; 0 on inactive cells;
    every value is a float32, so the device and the fp64 oracle read the same numbers;
  * the absolute stencil M = |A| |x| + |b| and the diagonal d, written once from labels and face weights (class Stencil) and
    pinned to oracle.apply_poisson / oracle.residual by tests/test_operator_inputs_are_live.py;
  * per-cell bounds derived from the kernels' operation counts (the K_* / N_* constants below, each with its count), eps = 2^-24,
    the unit round-off of binary32.  Nothing here is fitted to a device result;
  * dead_share: the share of active cells at which an input's own term is under 4 x the cell's bound -- the cells where a kernel
    that dropped the input would still pass.

Grids are numpy arrays [k, j, i]; labels 0 INTERIOR, 1 EXTERIOR, 2 DIRICHLET, 3 BOUNDARY; face weights w[axis] (axis 0 = x = the
last array dimension) hold one more entry along their axis, None on the unit-weight coarse levels.  Active cells never touch the
border of a grid (the sweeps read all six neighbours unmasked)."""
import numpy as np

EPS = 2.0 ** -24
OMEGA = 2.0 / 3.0
INTERIOR, EXTERIOR, DIRICHLET, BOUNDARY = 0, 1, 2, 3

# apply: 7 terms (d x_c and six w x_n).  A term passes through its product and at most six additions = 7 = `terms` roundings; the
# diagonal of a general row is itself a float32 sum of six weights (5 roundings, boundaryRowsKernel), its term then passes the
# product and one addition (boundaryRow: lap = acc + diag * x_c): 7 again.  terms + 1 covers the second-order remainder.
K_APPLY = 7 + 1
# residual: the same 7 terms and b, one more addition (epilogue: b - lap): 8 terms.
K_RESIDUAL = 8 + 1
# Jacobi, x' = x + omega ((b - lap) / d): the residual's 9, the diagonal again as the divisor (5), the division (1; simple cells:
# v_rcp_f32 within 1 ulp = 2 eps and a product, 3 -- with their exact integer diagonal 9 + 3 + 2 = 14 in all), omega rounded to
# float32 (1), the product by omega (1), and one for the remainder: 9 + 5 + 1 + 1 + 1 + 1 = 18 on (b - lap) / d, whose size is at
# most M / d.  The closing addition rounds x' itself: eps (|x_c| + omega M / d), the first of which is the bound's own first term
# and the second is inside the remainder's share.
K_JACOBI = 18
# restriction: a coarse cell sums n = 4^3 fine cells; a product by an exactly representable weight and at most n - 1 additions
# whatever the order (z, y, x in restrictKernel; z then x then y in the folded layouts): (n + 1) eps sum R |r|.
N_RESTRICT = 64
# prolong-and-add, f' = f + 4 trilerp(c): n = 8 coarse cells; three nested lerps = three products and three additions per term (or
# one product by the weight and seven additions), the factor 4 exact, the closing addition: (n + 1) eps sum P |c| + eps |f|.
N_PROLONG = 8
RW = (0.125, 0.375, 0.375, 0.125)  # full weighting along one axis, fine cells 2 C - 1 .. 2 C + 2 (Ops.h:799)


def active_mask(lab):
    return (lab == INTERIOR) | (lab == BOUNDARY)


def as_f32(a):
    """the values a float32 grid holds, as fp64"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def active_box(lab, align=4, halo=2):
    """slices of the smallest box around the active cells with `halo` cells to spare, its ends on multiples of `align` (so that
    the box of the next coarser level is this one halved); for grids whose liquid fills a small part of the array"""
    act = active_mask(lab)
    box = []
    for ax in range(3):
        idx = np.nonzero(act.any(axis=tuple(a for a in range(3) if a != ax)))[0]
        lo = max(0, (int(idx[0]) - halo) // align * align)
        hi = min(lab.shape[ax], -(-(int(idx[-1]) + 1 + halo) // align) * align)
        box.append(slice(lo, hi))
    return tuple(box)


def _shift(a, ax, d):
    """a's value in the neighbour on side d (0 minus, 1 plus) along array axis ax; 0 past the grid"""
    out = np.zeros_like(a)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[ax], dst[ax] = (slice(1, None), slice(0, -1)) if d else (slice(0, -1), slice(1, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


class Stencil:
    """computeLaplacian's row of every cell (Ops.h:177-260): the diagonal `diag` and the six off-diagonal weights `off` in the
    order -x +x -y +y -z +z.  INTERIOR: six unit weights, diagonal 6.  BOUNDARY: an INTERIOR neighbour 1 / 1, a BOUNDARY neighbour
    w / w, a DIRICHLET neighbour 0 / w (off-diagonal / share of the diagonal), an EXTERIOR neighbour nothing.
    box: slices of the part of the grid to work on (active_box); full-size arrays handed to the methods are cut to it."""

    def __init__(self, lab, w=None, box=None):
        lab = np.asarray(lab)
        self.full_shape = lab.shape
        self.box = tuple(slice(*s.indices(n)[:2]) for s, n in zip(box or (slice(None),) * 3, lab.shape))
        lab = lab[self.box]
        self.lab = lab
        self.act = active_mask(lab)
        edge = np.ones(lab.shape, bool)
        edge[1:-1, 1:-1, 1:-1] = False
        assert not (self.act & edge).any(), "an active cell on the border of the grid"
        interior, bnd = lab == INTERIOR, lab == BOUNDARY
        self.diag = np.zeros(lab.shape)
        self.off = []
        for axis in range(3):
            ax = 2 - axis
            for d in (0, 1):
                nl = np.full(lab.shape, EXTERIOR, dtype=lab.dtype)
                src, dst = [slice(None)] * 3, [slice(None)] * 3
                src[ax], dst[ax] = (slice(1, None), slice(0, -1)) if d else (slice(0, -1), slice(1, None))
                nl[tuple(dst)] = lab[tuple(src)]
                if w is None:
                    wt = np.float32(1.0)
                else:
                    sl = list(self.box)
                    sl[ax] = slice(sl[ax].start + d, sl[ax].stop + d)
                    wt = np.asarray(w[axis])[tuple(sl)]
                    assert (wt.astype(np.float32) == wt).all()
                    wt = wt.astype(np.float32)
                to_int, to_bnd, to_dir = bnd & (nl == INTERIOR), bnd & (nl == BOUNDARY), bnd & (nl == DIRICHLET)
                self.off.append(np.where(interior | to_int, np.float32(1.0), np.where(to_bnd, wt, np.float32(0.0))).astype(np.float32))
                self.diag += np.where(to_int, 1.0, np.where(to_bnd | to_dir, wt, 0.0))
        self.diag[interior] = 6.0
        self.diag[~self.act] = 0.0
        assert (self.diag[self.act] > 0).all()

    def cut(self, a):
        a = np.asarray(a, dtype=np.float64)
        if a.shape == self.full_shape:
            a = a[self.box]
        assert a.shape == self.lab.shape, (a.shape, self.lab.shape)
        return a

    def _row(self, x, absolute):
        """diag x_c -/+ sum w x_n: the signed row, or the sum of the absolute terms"""
        x = self.cut(x)
        if absolute:
            x = np.abs(x)
        acc = self.diag * x
        q = 0
        for axis in range(3):
            for d in (0, 1):
                t = self.off[q] * _shift(x, 2 - axis, d)
                if absolute:
                    acc += t
                else:
                    acc -= t
                q += 1
        acc[~self.act] = 0.0
        return acc

    def apply(self, x):
        """A x on active cells, 0 elsewhere"""
        return self._row(x, False)

    def residual(self, x, b):
        r = self.cut(b) - self._row(x, False)
        r[~self.act] = 0.0
        return r

    def M(self, x, b=None):
        """|A| |x| + |b| = diag |x_c| + sum w |x_n| + |b_c| on active cells, 0 elsewhere"""
        m = self._row(x, True)
        if b is not None:
            m += np.abs(self.cut(b))
            m[~self.act] = 0.0
        return m

    def over_diag(self, a):
        out = np.zeros(self.lab.shape)
        np.divide(a, self.diag, out=out, where=self.act)
        return out

    def cells_mask(self, cells):
        """a band list (n x (i, j, k), full-grid indices) as a mask of the box"""
        m = np.zeros(self.full_shape, bool)
        cells = np.asarray(cells).reshape(-1, 3)
        m[cells[:, 2], cells[:, 1], cells[:, 0]] = True
        return m[self.box]

    def carry(self, e, omega=OMEGA, mask=None):
        """an error bound e on x taken through one damped-Jacobi pass over `mask` (default: every active cell):
        |1 - omega| e_c + omega (sum w e_n) / d there, e_c elsewhere -- the absolute iteration matrix |I - omega D^-1 A|"""
        e = self.cut(e)
        nb = self._row(e, True) - self.diag * e
        out = abs(1.0 - omega) * e + omega * self.over_diag(nb)
        mask = self.act if mask is None else (mask & self.act)
        return np.where(mask, out, e)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def signed_source(lab, seed):
    """uniform in (-1, 1) on active cells, 0 elsewhere, float32 values: a source grid for the transfers, an iterate"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return as_f32(np.where(active_mask(lab), rng.uniform(-1.0, 1.0, lab.shape), 0.0))


def balanced_inputs(lab, w, seed, stencil=None):
    """(x, b) of the full grid: x uniform in (-1, 1), b uniform in (-1, 1) times the cell's diagonal, both 0 on inactive cells"""
    st = stencil or Stencil(lab, w)
    x = signed_source(lab, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 7919))
    b = np.zeros(lab.shape)
    b[st.box] = rng.uniform(-1.0, 1.0, st.lab.shape) * st.diag
    return x, as_f32(b)


# ---- transfers ------------------------------------------------------------------------------------------------------------------
def _restrict_axis(a, ax):
    n = a.shape[ax] // 2
    pad = [(0, 0)] * 3
    pad[ax] = (1, 1)
    p = np.pad(a, pad)
    sl = lambda o: tuple(slice(o, o + 2 * n, 2) if t == ax else slice(None) for t in range(3))
    return sum(RW[o] * p[sl(o)] for o in range(4))


def restrict(fine, coarse_lab):
    """full weighting (Ops.h:734-835): coarse C = sum over 4^3 fine cells from 2 C - 1 of the product weights, 0 past the grid and
    on inactive coarse cells.  Weights are positive: restrict(|r|) is sum R |r|."""
    out = np.asarray(fine, dtype=np.float64)
    for ax in range(3):
        out = _restrict_axis(out, ax)
    assert out.shape == coarse_lab.shape, (out.shape, coarse_lab.shape)
    return np.where(active_mask(coarse_lab), out, 0.0)


def _prolong_axis(a, ax):
    n = a.shape[ax]
    out_shape = list(a.shape)
    out_shape[ax] = 2 * n
    out = np.zeros(out_shape)
    lo, hi = _shift(a, ax, 0), _shift(a, ax, 1)
    ev = tuple(slice(0, None, 2) if t == ax else slice(None) for t in range(3))
    od = tuple(slice(1, None, 2) if t == ax else slice(None) for t in range(3))
    out[ev] = 0.75 * a + 0.25 * lo  # fine 2 C samples at C - 1/4
    out[od] = 0.75 * a + 0.25 * hi  # fine 2 C + 1 at C + 1/4
    return out


def prolong(coarse, fine_lab):
    """4 x the trilinear sample at c / 2 - 1 / 4 (Ops.h:873-972) on active fine cells, 0 elsewhere (no active cell on a border)"""
    out = np.asarray(coarse, dtype=np.float64)
    for ax in range(3):
        out = _prolong_axis(out, ax)
    assert out.shape == fine_lab.shape
    return np.where(active_mask(fine_lab), 4.0 * out, 0.0)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def bound_apply(st, x):
    return K_APPLY * EPS * st.M(x)


def bound_residual(st, x, b):
    return K_RESIDUAL * EPS * st.M(x, b)


def bound_jacobi(st, x, b, omega=OMEGA, mask=None):
    """one damped-Jacobi pass over `mask` (a band pass; default: a sweep over every active cell); 0 where the pass writes nothing"""
    out = EPS * (np.abs(st.cut(x)) + K_JACOBI * omega * st.over_diag(st.M(x, b)))
    return np.where(st.act if mask is None else (mask & st.act), out, 0.0)


def bound_restrict(fine, coarse_lab):
    return (N_RESTRICT + 1) * EPS * restrict(np.abs(fine), coarse_lab)


def bound_residual_restrict(st, x, b, coarse_lab):
    """downsample(b - A x) formed in one go: every fine residual's own bound through the weights, and the restriction's term"""
    assert st.lab.shape == st.full_shape or all(s.start % 2 == 0 and s.stop % 2 == 0 for s in st.box)
    cl = coarse_lab[tuple(slice(s.start // 2, s.stop // 2) for s in st.box)]
    return restrict(bound_residual(st, x, b), cl) + bound_restrict(st.residual(x, b), cl)


def bound_prolong_add(fine, coarse, fine_lab):
    return np.where(active_mask(fine_lab), EPS * (np.abs(fine) + (N_PROLONG + 1) * prolong(np.abs(coarse), fine_lab)), 0.0)


def smooth_stroke(st, oracle, x, b, lab32, band, w64=None, omega=OMEGA, band_iterations=3):
    """The Jacobi smoothing stroke of MG.cpp:442-486 from x (float32 values): band passes, one sweep, band passes, each by the
    fp64 oracle.  Returns (x', e): the oracle's result and the per-cell bound on a float32 stroke that rounds as the K_JACOBI count
    allows at every pass, each pass's bound carried through the passes after it (Stencil.carry)."""
    assert st.lab.shape == st.full_shape
    x = np.array(x, dtype=np.float64)
    e = np.zeros(x.shape)
    mask = st.cells_mask(band)
    for stage in ["band"] * band_iterations + ["sweep"] + ["band"] * band_iterations:
        m = mask if stage == "band" else None
        e = st.carry(e, omega, m) + bound_jacobi(st, x, b, omega, m)
        if stage == "band":
            oracle.boundary_jacobi(x, b, lab32, band, w64, weight=None if omega == OMEGA else omega)
        else:
            oracle.jacobi(x, b, lab32, w64, weight=None if omega == OMEGA else omega)
    return x, e


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound, box=None):
    """(max |got - ref| / bound, the cell (k, j, i) it is at, error and bound there).  A cell whose bound is 0 -- inactive cells,
    cells a pass does not write -- must hold the reference's value exactly: any difference there counts as infinite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    off = (0, 0, 0)
    if box is not None and got.shape != bound.shape:
        outside = np.ones(got.shape, bool)
        outside[box] = False
        assert np.array_equal(got[outside], ref[outside]), "a difference outside the box of the active cells"
        got, ref, off = got[box], ref[box], tuple(s.start for s in box)
    err = np.abs(got - ref)
    ratio = np.zeros(err.shape)
    np.divide(err, bound, out=ratio, where=bound > 0)
    ratio[(bound <= 0) & (err > 0)] = np.inf
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(a + o) for a, o in zip(at, off)), float(err[at]), float(bound[at])


def assert_within(name, got, ref, bound, box=None, factor=1.0):
    """|got - ref| <= factor * bound in every cell; prints and returns the worst error / bound"""
    worst, at, err, bnd = worst_ratio(got, ref, bound, box)
    print(f"PERCELL {name}: worst error/bound {worst:.3f} at {at} (error {err:.3e}, bound {bnd:.3e})")
    assert worst <= factor, f"{name}: error {err:.3e} over {factor} x bound {bnd:.3e} at cell (k, j, i) = {at}"
    return worst


def normalised_error(st, got, ref, scale_x, b):
    """max over active cells of |got - ref| / (M / d), M from scale_x (the larger of the iterate before and after a pass) and b:
    the yardstick of the Gauss-Seidel comparison"""
    scale = st.over_diag(st.M(scale_x, b))
    err = np.abs(st.cut(got) - st.cut(ref))
    assert (err[~st.act] == 0).all()
    ratio = np.zeros(err.shape)
    np.divide(err, scale, out=ratio, where=scale > 0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(a + s.start) for a, s in zip(at, st.box))


# ---- liveness -------------------------------------------------------------------------------------------------------------------
def _share(term, bound, act):
    n = int(act.sum())
    return float(((np.abs(term) < 4.0 * bound) & act).sum()) / max(n, 1)


def dead_share(op, st=None, x=None, b=None, coarse_lab=None, fine=None, coarse=None, fine_lab=None, omega=OMEGA):
    """The share of active cells at which an input's own term is smaller than 4 x the cell's bound -- where a kernel that dropped
    the input would still be inside the bound, or nearly.
      'residual', 'jacobi', 'residual_restrict': the rhs b of the level (st, x, b; coarse_lab for the pair) -- its term is |b_c|,
          omega |b_c| / d_c, |sum R b|;
      'restrict': the source grid `fine` -- |sum R fine| per active coarse cell;
      'prolong': the source grid `coarse` of f' = f + 4 trilerp(coarse) -- |4 trilerp(coarse)| per active fine cell."""
    if op == "residual":
        return _share(st.cut(b), bound_residual(st, x, b), st.act)
    if op == "jacobi":
        return _share(omega * st.over_diag(st.cut(b)), bound_jacobi(st, x, b, omega), st.act)
    if op == "residual_restrict":
        cl = coarse_lab[tuple(slice(s.start // 2, s.stop // 2) for s in st.box)]
        bb = np.where(st.act, st.cut(b), 0.0)
        return _share(restrict(bb, cl), bound_residual_restrict(st, x, b, coarse_lab), active_mask(cl))
    if op == "restrict":  # (over the coarse cells that have an active fine cell under them)
        has = restrict((np.asarray(fine) != 0).astype(np.float64), coarse_lab) > 0
        return _share(restrict(fine, coarse_lab), bound_restrict(fine, coarse_lab), has)
    if op == "prolong":  # (over the fine cells that have an active coarse cell among the eight they sample)
        has = prolong((np.asarray(coarse) != 0).astype(np.float64), fine_lab) > 0
        return _share(prolong(coarse, fine_lab), bound_prolong_add(fine, coarse, fine_lab), has)
    raise ValueError(op)


# ---- the domains of the stroke tests' children (tests/test_rz_xfold.py, test_fused_downstroke.py, test_plain_quads.py and the
# residual-pair child of test_gpu_parity.py), restated for the CPU liveness test: (labels, weights, levels) ------------------------
def stroke_case(case):
    from geometricmultigridpressuresolver_amd import domains as D

    boxed = D.dirichlet_box

    def inner(bl):
        bl[1:-1, 1:-1, 1:-1] = D.INTERIOR

    def middle(bl):
        bl[1:-1, 1:-1, 64:448] = D.INTERIOR

    def stair(bl):
        bl[1:8, 1:12, 1:-1] = D.INTERIOR
        bl[1:16, 12:31, 1:-1] = D.INTERIOR

    def speckled(bl):
        bl[1:-1, 1:-1, 1:-1] = np.where(np.random.default_rng(3).random((22, 30, 246)) < 0.95, D.INTERIOR, D.DIRICHLET)

    levels = 3
    if case == "seams776":
        (bl, bw), shape = boxed((20, 44, 768), inner), (28, 52, 776)
    elif case == "mid520":
        (bl, bw), shape = boxed((20, 44, 512), middle), (28, 52, 520)
    elif case == "stair520":
        (bl, bw), shape = boxed((24, 32, 512), stair), (32, 40, 520)
    elif case == "stair":
        (bl, bw), shape = boxed((24, 32, 248), stair), (32, 40, 264)
    elif case == "rag264":
        (bl, bw), shape = boxed((20, 44, 248), inner), (28, 52, 264)
    elif case == "tall264":
        (bl, bw), shape = boxed((64, 28, 256), inner), (72, 36, 264)
    elif case == "ragz264":
        (bl, bw), shape, levels = boxed((6, 16, 260), inner), (10, 20, 264), 2
    elif case == "speckled":
        (bl, bw), shape = boxed((24, 32, 248), speckled), (32, 40, 264)
    elif case == "wsolid":
        bl, bw, _ = D.build_complex_domain((24, 32, 256), use_solid=True)
        shape = (32, 40, 264)
    else:
        raise ValueError(case)
    lab, w, off, lev = D.expand_domain(bl, bw, levels=levels, solver_shape=shape)
    return lab, [np.asarray(a, dtype=np.float32) for a in w], lev  # (the values the device holds)
