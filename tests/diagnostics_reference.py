"""numpy twin of the diagnostics of examples 02 and 06, written from the reference scripts' formulas
(signorini_dolfinx.py:293-321, 346-350; gradient_constraint_dolfinx.py:134-165).  Test infrastructure: it takes a state vector and the
mesh / dof arrays the Python classes expose.  Example 02 tabulates with the ORACLE's basis functions (oracle/sg_oracle.py).  Example 06
has a tabulator of its own (`lagrange_tabulate`, node orders of oracle/gc_oracle.py, checked against the oracle's tabulators in
tests/test_cpu_diagnostics.py): the oracle's come out of a linear solve and are nodal only up to 1e-15, which times latent dofs of 1e6
is 1e-9 in psi at a node where psi itself is small - far above the 1e-12 the fields are compared at.
"""
import numpy as np

from oracle import gc_oracle as G6
from oracle import sg_oracle as S2

_GREF = np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------------
# example 02: x = [u_x | u_y | u_z | psi] over nv nodes; n_g = -e_z, g = x_z - gap
# ---------------------------------------------------------------------------------------------------------------------
def lame(E, nu):
    return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))  # :58-66


def sg_node_gradients(cell_type, degree):
    """(reference gradients dN[n, a, :] of basis function a at the cell's own reference node n, the four local nodes spanning the
    affine cell) in the node orders of include/pgx_sg.h"""
    if cell_type == 0:
        if degree == 1:
            return np.broadcast_to(_GREF, (4, 4, 3)).copy(), (0, 1, 2, 3)
        L = np.zeros((10, 4))
        L[np.arange(4), np.arange(4)] = 1.0
        for k, (a, b) in enumerate(S2.TET_EDGES):
            L[4 + k, a] = L[4 + k, b] = 0.5
        return S2._p2_tet_grad(L), (0, 1, 2, 3)
    d, n1 = degree, degree + 1
    V, D = S2._lag1d(d, np.arange(n1) / d)  # [node, function]
    dN = np.empty((n1**3, n1**3, 3))
    for nz in range(n1):
        for ny in range(n1):
            for nx in range(n1):
                n = (nz * n1 + ny) * n1 + nx
                for iz in range(n1):
                    for iy in range(n1):
                        for ix in range(n1):
                            dN[n, (iz * n1 + iy) * n1 + ix] = (D[nx, ix] * V[ny, iy] * V[nz, iz], V[nx, ix] * D[ny, iy] * V[nz, iz],
                                                               V[nx, ix] * V[ny, iy] * D[nz, iz])
    return dN, (0, d, d * n1, d * n1 * n1)


def von_mises(x, coords, cells, E, nu, cell_type, degree):
    """sqrt(3/2 s:s), s = sigma(u) - tr(sigma(u))/3 I, sigma = 2 mu eps(u) + lambda tr(eps(u)) I (:146-153, 300-301), at every node of every
    (affine) cell: (n_cells, nodes per cell)"""
    mu, lmbda = lame(E, nu)
    nv = len(coords)
    u = np.stack([x[:nv], x[nv:2 * nv], x[2 * nv:3 * nv]], axis=1)
    dN, g = sg_node_gradients(cell_type, degree)
    X = coords[cells[:, list(g)]]
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)  # J[c, d, k]
    Ji = np.linalg.inv(J)  # Ji[c, k, d] = d xi_k / d x_d
    grad = np.einsum("cai,nak,ckd->cnid", u[cells], dN, Ji)
    eps = 0.5 * (grad + np.swapaxes(grad, 2, 3))
    eye = np.eye(3)
    sigma = 2.0 * mu * eps + lmbda * np.trace(eps, axis1=2, axis2=3)[..., None, None] * eye
    s = sigma - np.trace(sigma, axis1=2, axis2=3)[..., None, None] / 3.0 * eye
    return np.sqrt(1.5 * np.einsum("cnij,cnij->cn", s, s))


def violation(x, coords, gap):
    """u.n_g - g at every node (:307-308)"""
    nv = len(coords)
    return -x[2 * nv:3 * nv] - (coords[:, 2] - gap)


def _facet_basis(cell_type, degree, qpts):
    if cell_type == 0:
        L = np.stack([1.0 - qpts[:, 0] - qpts[:, 1], qpts[:, 0], qpts[:, 1]], axis=1)
        return (L if degree == 1 else S2._p2_tri(L)), (0, 1, 2)
    d = degree
    Vx, _ = S2._lag1d(d, qpts[:, 0])
    Vy, _ = S2._lag1d(d, qpts[:, 1])
    return np.stack([Vx[:, ix] * Vy[:, iy] for iy in range(d + 1) for ix in range(d + 1)], axis=1), (0, d, d * (d + 1))


def penetration(x, coords, facets, gap, cell_type, degree, qpts, qwts, geometry6=None):
    """sqrt(int_Gamma max(u.n_g - g, 0)^2 ds) (:307-314) with the facet rule (qpts, qwts).  Affine facets: surface element and z from
    the three nodes spanning the facet; `geometry6` = (nf, 6, 3) node coordinates of curved 6-node facets: isoparametric."""
    nv = len(coords)
    N, g = _facet_basis(cell_type, degree, qpts)
    uq = x[2 * nv:3 * nv][facets] @ N.T  # (nf, nq)
    if geometry6 is None:
        X = coords[facets[:, list(g)]]
        ds = np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)[:, None]
        zq = X[:, 0, 2][:, None] + qpts[None, :, 0] * (X[:, 1, 2] - X[:, 0, 2])[:, None] + qpts[None, :, 1] * (X[:, 2, 2] - X[:, 0, 2])[:, None]
    else:
        L = np.stack([1.0 - qpts[:, 0] - qpts[:, 1], qpts[:, 0], qpts[:, 1]], axis=1)
        t = np.einsum("fad,qak->fqdk", geometry6, S2._p2_tri_grad(L))
        ds = np.linalg.norm(np.cross(t[..., 0], t[..., 1]), axis=2)
        zq = geometry6[:, :, 2] @ S2._p2_tri(L).T
    d = -uq - (zq - gap)
    pen = np.where(d > 0, d, 0.0)
    return float(np.sqrt(np.sum(qwts[None] * ds * pen * pen)))


# ---------------------------------------------------------------------------------------------------------------------
# example 06: x = [u (n_u) | psi_x (n_p) | psi_y (n_p)]
# ---------------------------------------------------------------------------------------------------------------------
def _scaled(k, lam):
    """k lam, with values within a few roundings of an integer taken AS that integer: a point given as the nearest doubles to a lattice
    node sits on the node, where the nodal basis is exactly the Kronecker delta"""
    t = k * np.asarray(lam, dtype=float)
    r = np.rint(t)
    return np.where(np.abs(t - r) <= 8 * np.finfo(float).eps * k, r, t)


def lagrange_tabulate(k, pts, quad):
    """values (npts, n) and reference gradients (npts, n, 2) of the equispaced Lagrange basis of degree k >= 1: triangles in the node
    order of gc_oracle.pk_lattice, N = prod_m prod_{a < i_m} (k l_m - a) / (i_m - a) over the barycentric coordinates l; quadrilaterals
    lexicographic (x fastest), products of the 1-D basis prod_{a != i} (k t - a) / (i - a)"""
    pts = np.asarray(pts, dtype=float).reshape(-1, 2)
    n = len(pts)
    if quad:
        def one_d(t):
            V, D = np.ones((n, k + 1)), np.zeros((n, k + 1))
            for i in range(k + 1):
                for a in range(k + 1):
                    if a != i:
                        f = (t - a) / (i - a)
                        D[:, i] = D[:, i] * f + V[:, i] * (k / (i - a))
                        V[:, i] = V[:, i] * f
            return V, D

        Vx, Dx = one_d(_scaled(k, pts[:, 0]))
        Vy, Dy = one_d(_scaled(k, pts[:, 1]))
        N = np.stack([Vx[:, ix] * Vy[:, iy] for iy in range(k + 1) for ix in range(k + 1)], axis=1)
        dN = np.stack([np.stack([Dx[:, ix] * Vy[:, iy], Vx[:, ix] * Dy[:, iy]], axis=1) for iy in range(k + 1) for ix in range(k + 1)], axis=1)
        return N, dN
    t = _scaled(k, np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1))
    dlam = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]])

    def P(m, tc):  # prod_{a < m} (t - a) / (m - a) and its derivative with respect to lambda
        v, d = np.ones(n), np.zeros(n)
        for a in range(m):
            f = (tc - a) / (m - a)
            d = d * f + v * (k / (m - a))
            v = v * f
        return v, d

    idx = G6.pk_lattice(k)
    N, dN = np.empty((n, len(idx))), np.empty((n, len(idx), 2))
    for j, (i0, i1, i2) in enumerate(idx):
        (a, da), (b, db), (c, dc) = P(i0, t[:, 0]), P(i1, t[:, 1]), P(i2, t[:, 2])
        N[:, j] = a * b * c
        dN[:, j] = np.stack([da * b * c, a * db * c, a * b * dc], axis=1) @ dlam
    return N, dN


def gc_eval(x, coords, corners, cell_dofs_u, cell_dofs_p, phi_dofs, degree, quad, pts):
    """At the reference points `pts` of every cell: dict with grad_u (nc, npts, 2), feas = phi psi / sqrt(1 + psi.psi) (nc, npts, 2), phi
    (nc, npts), the margins |grad u| - phi and |feas| - phi, and the flags active = (margin >= 0) (:136-137), feasible_active =
    (margin > -1e-8) (:140-144)."""
    pts = np.asarray(pts, dtype=float).reshape(-1, 2)
    n_u, n_p = len(phi_dofs), (len(x) - len(phi_dofs)) // 2
    Nu, dNu = lagrange_tabulate(degree, pts, quad)
    Np, _ = lagrange_tabulate(degree - 1, pts, quad)
    X = coords[corners]
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]], axis=2)
    Ji = np.linalg.inv(J)
    u = x[:n_u][cell_dofs_u]
    grad_u = np.einsum("ca,pak,ckd->cpd", u, dNu, Ji)
    phi = phi_dofs[cell_dofs_u] @ Nu.T
    psi = np.stack([x[n_u:n_u + n_p][cell_dofs_p] @ Np.T, x[n_u + n_p:][cell_dofs_p] @ Np.T], axis=2)
    feas = phi[..., None] * psi / np.sqrt(1.0 + np.sum(psi * psi, axis=2))[..., None]
    m_active = np.sqrt(np.sum(grad_u * grad_u, axis=2)) - phi
    m_feas = np.sqrt(np.sum(feas * feas, axis=2)) - phi
    return {"grad_u": grad_u, "feas": feas, "phi": phi, "margin_active": m_active, "margin_feasible": m_feas,
            "active": (m_active >= 0).astype(np.uint8), "feasible_active": (m_feas > -1e-8).astype(np.uint8)}
