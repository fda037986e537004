"""NumPy / SciPy restatement of the two-way rigid-body coupling (include/mgps_fields.h): the yardstick of
tests/test_rigid_coupling.py.  Everything is float64.  G comes column by column from solid_rhs(rigid_velocity(e_j)) of
tests/solid_forces_reference.py, A is assembled from expanded labels and weights by tests/test_oracle_properties.py's assemble, and
the coupled system (A + G K G^T) p = b is solved by a direct sparse solve.

Body tables have one row per body with row 0 included (never read): centres (bodies + 1, 3), inv_mass (bodies + 1,), inv_inertia
(bodies + 1, 6) in the order xx, yy, zz, xy, xz, yz, motions (bodies + 1, 6) = U then omega."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import solid_forces_reference as R


def coupling_matrix(material, cut_weights, body, centres):
    """G: (cells of the base grid, 6 * bodies) sparse; column 6 (r - 1) + j is the solid part of the right-hand side for the unit
    motion e_j of body r"""
    shape = tuple(material.shape)
    centres = np.asarray(centres, dtype=np.float64)
    bodies = centres.shape[0] - 1
    cols = []
    for r in range(1, bodies + 1):
        for j in range(6):
            lin, ang = np.zeros((bodies + 1, 3)), np.zeros((bodies + 1, 3))
            (lin if j < 3 else ang)[r, j % 3] = 1.0
            sv = R.rigid_velocity(shape, body, centres, lin, ang, bodies)
            cols.append(sp.csc_matrix(R.solid_rhs(material, sv, cut_weights).reshape(-1, 1)))
    return sp.hstack(cols, format="csr")


def inertia_matrix(six):
    xx, yy, zz, xy, xz, yz = six
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)


def stiffness(inv_mass, inv_inertia):
    """K: (6 * bodies, 6 * bodies) block diagonal"""
    inv_mass, inv_inertia = np.asarray(inv_mass, dtype=np.float64), np.asarray(inv_inertia, dtype=np.float64).reshape(-1, 6)
    blocks = []
    for r in range(1, inv_mass.shape[0]):
        blocks += [inv_mass[r] * np.eye(3), inertia_matrix(inv_inertia[r])]
    return sp.block_diag(blocks, format="csr")


def flat(motions):
    """(bodies + 1, 6) -> the 6 * bodies vector G takes"""
    return np.asarray(motions, dtype=np.float64).reshape(-1, 6)[1:].reshape(-1)


def table(v):
    """the 6 * bodies vector -> (bodies + 1, 6) with a zero row 0"""
    return np.concatenate([np.zeros((1, 6)), np.asarray(v, dtype=np.float64).reshape(-1, 6)])


def apply_terms(G, K, x):
    """(G K G^T x, sum of |terms|) per base cell: what a reordered fp64 evaluation's error scales with -- |G| |K| |G|^T |x|"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return G @ (K @ (G.T @ x)), abs(G) @ (abs(K) @ (abs(G).T @ np.abs(x)))


def coupled_mask(material, cut_weights, body, bodies):
    """the COUPLED cells: LIQUID with at least one face of closed fraction s > 0 and row 1 .. bodies"""
    mask = np.zeros(material.shape, dtype=bool)
    for a in range(3):
        owned = (R.closed_fraction(cut_weights[a]) > 0) & (R.rows_of(body[a], bodies) > 0)
        ax, n = 2 - a, material.shape[2 - a]
        mask |= np.take(owned, np.arange(n), axis=ax) | np.take(owned, np.arange(1, n + 1), axis=ax)
    return mask & (material == R.LIQUID)


class Scene:
    """One coupled projection on expanded labels / weights: A on the active cells (index idx), G restricted to them."""

    def __init__(self, material, cut_weights, body, centres, labels, weights, offset):
        from test_oracle_properties import assemble

        self.shape, self.eshape, self.offset = tuple(material.shape), tuple(labels.shape), int(offset)
        self.A, self.idx, self.active = assemble(np.asarray(labels, dtype=np.int32), [np.asarray(w, dtype=np.float64) for w in weights])
        self.Gbase = coupling_matrix(material, cut_weights, body, centres)
        o, (gz, gy, gx) = self.offset, self.shape
        base_to_unknown = self.idx[o:o + gz, o:o + gy, o:o + gx].reshape(-1)
        liquid = (material == R.LIQUID).reshape(-1)
        assert (base_to_unknown[liquid] >= 0).all()  # every LIQUID cell is an unknown
        n = self.A.shape[0]
        pick = sp.csr_matrix((np.ones(liquid.sum()), (base_to_unknown[liquid], np.flatnonzero(liquid))), shape=(n, liquid.size))
        self.G = (pick @ self.Gbase).tocsr()

    def unknowns(self, expanded):
        return np.asarray(expanded, dtype=np.float64)[self.active]

    def expanded(self, v):
        out = np.zeros(self.eshape)
        out[self.active] = v
        return out

    def factor(self):
        if not hasattr(self, "_lu"):
            self._lu = spla.splu(self.A.tocsc())
        return self._lu

    def solve(self, b_fluid, inv_mass, inv_inertia, motions):
        """(p, V_out, b) on the unknowns: (A + G K G^T) p = b = b_fluid + G V*, V_out = V* - K G^T p.  Direct: one sparse LU of A and
        the identity (A + G K G^T)^-1 = A^-1 - Z (I + K G^T Z)^-1 K G^T A^-1 with Z = A^-1 G (6 * bodies columns), which holds for a
        singular K as well (K = 0: p = A^-1 b)"""
        K = stiffness(inv_mass, inv_inertia).toarray()
        b = np.asarray(b_fluid, dtype=np.float64) + self.G @ flat(motions)
        lu = self.factor()
        y, Z = lu.solve(b), lu.solve(self.G.toarray())
        small = np.eye(K.shape[0]) + K @ (self.G.T @ Z)
        p = y - Z @ np.linalg.solve(small, K @ (self.G.T @ y))
        return p, table(flat(motions) - K @ (self.G.T @ p)), b
