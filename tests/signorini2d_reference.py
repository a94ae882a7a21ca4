"""numpy/scipy twin of example 02 in the plane (include/pgx_sg.h: pgx_sg_create_2d), written from the formulas of the reference's
examples/02_signorini/signorini_dolfinx.py with gdim = 2.  It shares no code with the HIP path or its binding:

    state      x = [u_x | u_y | psi], psi on the contact nodes ordered by node id; n_g = -e_y, g = y - gap, f = 0
    elasticity eps in Voigt form (e_xx, e_yy, 2 e_xy) against the plane-strain matrix of mu = E / 2(1 + nu), lambda = E nu / (1 + nu)(1 - 2 nu)
               (the script's constants, :234-235) - the B^T C B form, where the kernels use the index form of sigma : eps
    bases      Lagrange polynomials built from their nodes (products of (t - s_b) / (s_a - s_b)); triangles: barycentric formulas
    quadrature cells - triangles: centroid (P1) / the three edge midpoints (P2; a different exact rule than the kernel's interior
               points); quadrilaterals: Gauss-Legendre (d + 1)^2.  Contact edges: Gauss-Legendre with (q + 2) // 2 points (basix's
               default for degree q on the interval)
    loop       the LVPP loop of :317-358 around oracle.pg_oracle.newton_solve (SNES newtonls, line search none)

Node orders are those of include/pgx_sg.h; the mesh builders below number nodes the way the package does so that states compare entry by
entry (vertices, then one node per edge in lexicographic (min, max) order; quadrilateral lattices lexicographic).
"""
import numpy as np
import scipy.sparse as sp

from oracle import pg_oracle as O

TRI_EDGES = ((0, 1), (0, 2), (1, 2))


# ------------------------------------------------------------------------------------------------------------------
# bases
# ------------------------------------------------------------------------------------------------------------------
def lagrange_1d(nodes, t):
    """values and derivatives (len(t), len(nodes)) of the Lagrange polynomials through `nodes`"""
    t = np.atleast_1d(np.asarray(t, dtype=float))
    V, D = np.empty((len(t), len(nodes))), np.empty((len(t), len(nodes)))
    for a, sa in enumerate(nodes):
        others = [s for b, s in enumerate(nodes) if b != a]
        poly = np.poly1d(others, r=True) / np.prod([sa - s for s in others])
        V[:, a], D[:, a] = poly(t), poly.deriv()(t)
    return V, D


def tri_grads(degree, X, Y):
    """reference gradients (n, npc, 2) at the points (X, Y): vertices, then the edges (0,1) (0,2) (1,2)"""
    X, Y = np.atleast_1d(X).astype(float), np.atleast_1d(Y).astype(float)
    L = np.stack([1 - X - Y, X, Y], axis=1)
    dL = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]])
    if degree == 1:
        return np.broadcast_to(dL, (len(X), 3, 2)).copy()
    out = np.empty((len(X), 6, 2))
    for a in range(3):
        out[:, a] = (4 * L[:, a] - 1)[:, None] * dL[a]
    for k, (a, b) in enumerate(TRI_EDGES):
        out[:, 3 + k] = 4 * (L[:, [a]] * dL[b] + L[:, [b]] * dL[a])
    return out


def quad_grads(degree, X, Y):
    """tensor Lagrange on the nodes k / degree, local nodes lexicographic (xi fastest)"""
    s = np.arange(degree + 1) / degree
    lx, dx = lagrange_1d(s, X)
    ly, dy = lagrange_1d(s, Y)
    n1 = degree + 1
    out = np.empty((len(lx), n1 * n1, 2))
    for iy in range(n1):
        for ix in range(n1):
            out[:, iy * n1 + ix, 0] = dx[:, ix] * ly[:, iy]
            out[:, iy * n1 + ix, 1] = lx[:, ix] * dy[:, iy]
    return out


def gauss01(n):
    t, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (t + 1.0), 0.5 * w


# ------------------------------------------------------------------------------------------------------------------
# meshes (numbered like the package's)
# ------------------------------------------------------------------------------------------------------------------
def unit_square_triangles(nx, ny):
    """right-diagonal triangulation: vertex v = j (nx + 1) + i, cells (v0, v1, v3), (v0, v2, v3) per rectangle"""
    X, Y = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="xy")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    cells = []
    for j in range(ny):
        for i in range(nx):
            v0 = j * (nx + 1) + i
            v1, v2, v3 = v0 + 1, v0 + nx + 1, v0 + nx + 2
            cells += [(v0, v1, v3), (v0, v2, v3)]
    bottom = np.array([(i, i + 1) for i in range(nx)])
    top = bottom + ny * (nx + 1)
    return coords, np.array(cells), bottom, top


def p2_triangles(coords, cells, *edge_sets):
    """vertices, then one node per edge (edges in lexicographic (min, max) order) at the midpoint -> (node coords, cells6, [edges3])"""
    nv = len(coords)
    pairs = {}
    for c in cells:
        for a, b in TRI_EDGES:
            pairs[(min(c[a], c[b]), max(c[a], c[b]))] = 0
    for k, key in enumerate(sorted(pairs)):
        pairs[key] = nv + k
    mid = np.array([0.5 * (coords[a] + coords[b]) for a, b in sorted(pairs)])
    cells6 = np.array([[*c, *(pairs[(min(c[a], c[b]), max(c[a], c[b]))] for a, b in TRI_EDGES)] for c in cells])
    out = [np.array([[a, b, pairs[(min(a, b), max(a, b))]] for a, b in e]).reshape(-1, 3) for e in edge_sets]
    return np.concatenate([coords, mid]), cells6, out


def unit_square_quads(nx, ny, degree):
    """Q_d lattice: (node coords, cells [(d+1)^2] lexicographic, bottom edges [d+1], top edges [d+1])"""
    d = degree
    Nx, Ny = d * nx + 1, d * ny + 1
    X, Y = np.meshgrid(np.linspace(0, 1, Nx), np.linspace(0, 1, Ny), indexing="xy")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    cells = np.array([[(d * j + iy) * Nx + d * i + ix for iy in range(d + 1) for ix in range(d + 1)] for j in range(ny) for i in range(nx)])
    bottom = np.array([[d * i + ix for ix in range(d + 1)] for i in range(nx)])
    top = bottom + (Ny - 1) * Nx
    return coords, cells, bottom, top


# ------------------------------------------------------------------------------------------------------------------
# the problem
# ------------------------------------------------------------------------------------------------------------------
class Signorini2D:
    """cells / contact_edges / bc_edges hold NODE ids in the orders of include/pgx_sg.h; `coords` all nodes."""

    def __init__(self, coords, cells, contact_edges, bc_edges, cell_type="triangle", degree=1, E=2.0e4, nu=0.3, gap=0.0, disp=-0.25,
                 quadrature_degree=4):
        self.coords = np.asarray(coords, dtype=float)
        self.cells = np.asarray(cells, dtype=np.int64)
        self.edges = np.asarray(contact_edges, dtype=np.int64).reshape(-1, degree + 1)
        self.cell_type, self.degree = cell_type, degree
        self.nv, self.nc = len(self.coords), len(self.cells)
        nv = self.nv
        self.node_coords = self.coords
        self.cverts = np.unique(self.edges.ravel()).astype(np.int32)
        self.npsi = len(self.cverts)
        self.ntot = 2 * nv + self.npsi
        self.mu, self.lmbda = E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
        self.gap, self.disp = float(gap), float(disp)
        self.bc_nodes = np.unique(np.asarray(bc_edges, dtype=np.int64).ravel())
        self.bc = np.concatenate([self.bc_nodes, nv + self.bc_nodes])
        self.bc_vals = np.concatenate([np.zeros(len(self.bc_nodes)), np.full(len(self.bc_nodes), self.disp)])
        self.isbc = np.zeros(2 * nv, dtype=bool)
        self.isbc[self.bc] = True
        quad = cell_type == "quadrilateral"
        npc = self.cells.shape[1]
        # affine geometry from (origin, +xi, +eta)
        gn = [0, degree, degree * (degree + 1)] if quad else [0, 1, 2]
        x = self.coords[self.cells[:, gn]]
        J = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]], axis=2)  # columns
        self.detJ, self.invJ = np.linalg.det(J), np.linalg.inv(J)
        self.grads = (lambda X, Y: quad_grads(degree, X, Y)) if quad else (lambda X, Y: tri_grads(degree, X, Y))
        if quad:
            g, w = gauss01(degree + 1)
            qx, qy, qw = np.tile(g, len(g)), np.repeat(g, len(g)), np.repeat(w, len(g)) * np.tile(w, len(g))
            s = np.arange(degree + 1) / degree
            self.ref_nodes = np.array([(sx, sy) for sy in s for sx in s])
        else:
            if degree == 1:
                qx, qy, qw = np.array([1 / 3]), np.array([1 / 3]), np.array([0.5])
            else:
                qx, qy, qw = np.array([0.5, 0.5, 0.0]), np.array([0.0, 0.5, 0.5]), np.full(3, 1 / 6)
            vr = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
            self.ref_nodes = vr if degree == 1 else np.concatenate([vr, [0.5 * (vr[a] + vr[b]) for a, b in TRI_EDGES]])
        lm, mu = self.lmbda, self.mu
        Cm = np.array([[lm + 2 * mu, lm, 0.0], [lm, lm + 2 * mu, 0.0], [0.0, 0.0, mu]])
        Ae = np.zeros((self.nc, 2 * npc, 2 * npc))  # local dof a * 2 + i
        for q in range(len(qw)):
            G = np.einsum("ak,ckd->cad", self.grads(qx[q], qy[q])[0], self.invJ)  # physical gradients (nc, npc, 2)
            B = np.zeros((self.nc, 3, 2 * npc))
            B[:, 0, 0::2] = G[:, :, 0]
            B[:, 1, 1::2] = G[:, :, 1]
            B[:, 2, 0::2] = G[:, :, 1]
            B[:, 2, 1::2] = G[:, :, 0]
            Ae += (qw[q] * np.abs(self.detJ))[:, None, None] * np.einsum("cki,kl,clj->cij", B, Cm, B)
        dofs = np.stack([self.cells + i * nv for i in range(2)], axis=2).reshape(self.nc, 2 * npc)  # (a, i) -> i nv + node
        rows, cols = np.repeat(dofs, 2 * npc, axis=1), np.tile(dofs, (1, 2 * npc))
        self.A = sp.coo_matrix((Ae.ravel(), (rows.ravel(), cols.ravel())), shape=(2 * nv, 2 * nv)).tocsr()
        # contact edges
        npe = degree + 1
        self.tq, self.wq1 = gauss01((quadrature_degree + 2) // 2)
        params = [0.0, 1.0] if npe == 2 else ([0.0, 0.5, 1.0] if quad else [0.0, 1.0, 0.5])
        self.Nq = lagrange_1d(params, self.tq)[0]  # (nq, npe)
        ends = [0, npe - 1] if quad else [0, 1]
        xe = self.coords[self.edges[:, ends]]
        self.elen = np.linalg.norm(xe[:, 1] - xe[:, 0], axis=1)
        self.wdet = self.elen[:, None] * self.wq1[None]
        self.yq = xe[:, 0, 1][:, None] + self.tq[None] * (xe[:, 1, 1] - xe[:, 0, 1])[:, None]
        self.v2psi = np.full(nv, -1, dtype=np.int64)
        self.v2psi[self.cverts] = np.arange(self.npsi)
        self.pf = self.v2psi[self.edges]
        Me = np.einsum("fq,qa,qb->fab", self.wdet, self.Nq, self.Nq)
        self.MG = sp.coo_matrix((Me.ravel(), (np.repeat(self.pf, npe, axis=1).ravel(), np.tile(self.edges, (1, npe)).ravel())),
                                shape=(self.npsi, nv)).tocsr()
        self.b_g = np.bincount(self.pf.ravel(), weights=((self.wdet * (self.yq - self.gap)) @ self.Nq).ravel(), minlength=self.npsi)
        self._rp, self._cp = np.repeat(self.pf, npe, axis=1).ravel(), np.tile(self.pf, (1, npe)).ravel()

    def exp_terms(self, psi, with_matrix=True):
        pq = psi[self.pf] @ self.Nq.T
        with np.errstate(over="ignore", under="ignore"):
            wE = self.wdet * np.exp(pq)
        b = np.bincount(self.pf.ravel(), weights=(wE @ self.Nq).ravel(), minlength=self.npsi)
        if not with_matrix:
            return b, None
        De = np.einsum("fq,qa,qb->fab", wE, self.Nq, self.Nq)
        return b, sp.coo_matrix((De.ravel(), (self._rp, self._cp)), shape=(self.npsi, self.npsi)).tocsr()

    def residual(self, x, xk, alpha):
        nv = self.nv
        u, psi, psik = x[:2 * nv], x[2 * nv:], xk[2 * nv:]
        ut = u.copy()
        ut[self.bc] = self.bc_vals
        Fu = alpha * (self.A @ ut)
        Fu[nv:] += self.MG.T @ (psi - psik)  # -<psi - psi_k, v.n_g>, n_g = -e_y
        Fp = -(self.MG @ ut[nv:]) + self.exp_terms(psi, with_matrix=False)[0] - self.b_g
        Fu[self.bc] = u[self.bc] - self.bc_vals
        return np.concatenate([Fu, Fp])

    def jacobian(self, x, alpha):
        nv = self.nv
        _, D = self.exp_terms(x[2 * nv:])
        free = sp.diags((~self.isbc).astype(float))
        A = free @ (alpha * self.A) @ free + sp.diags(self.isbc.astype(float))
        B = sp.hstack([sp.csr_matrix((self.npsi, nv)), self.MG], format="csr") @ free
        return sp.bmat([[A, free @ B.T], [-B, D]], format="csr")

    # -- what the script reports about an iterate (:293-321) ----------------------------------------------------------------
    def violation(self, x):
        return -x[self.nv:2 * self.nv] - (self.coords[:, 1] - self.gap)

    def penetration(self, x):
        uq = x[self.nv + self.edges] @ self.Nq.T
        d = -uq - (self.yq - self.gap)
        return float(np.sqrt(np.sum(self.wdet * np.maximum(d, 0.0) ** 2)))

    def von_mises(self, x):
        """the script's expression with len(u) = 2: s = sigma - tr(sigma)/3 I_2, sqrt(3/2 s:s), at each cell's own nodes"""
        nv = self.nv
        U = np.stack([x[:nv][self.cells], x[nv:2 * nv][self.cells]], axis=2)  # (nc, npc, 2)
        dN = self.grads(self.ref_nodes[:, 0], self.ref_nodes[:, 1])  # (n, npc, 2)
        G = np.einsum("nak,ckd->cnad", dN, self.invJ)
        grad = np.einsum("cai,cnad->cnid", U, G)
        eps = 0.5 * (grad + np.swapaxes(grad, 2, 3))
        sig = 2 * self.mu * eps + self.lmbda * np.trace(eps, axis1=2, axis2=3)[..., None, None] * np.eye(2)
        s = sig - np.trace(sig, axis1=2, axis2=3)[..., None, None] / 3.0 * np.eye(2)
        return np.sqrt(1.5 * np.einsum("cnij,cnij->cn", s, s))


def from_triangles(vertex_coords, tri_cells, contact_pairs, disp_pairs, degree, **kw):
    if degree == 1:
        return Signorini2D(vertex_coords, tri_cells, contact_pairs, disp_pairs, "triangle", 1, **kw)
    coords, cells6, (ce, be) = p2_triangles(np.asarray(vertex_coords), np.asarray(tri_cells), np.asarray(contact_pairs), np.asarray(disp_pairs))
    return Signorini2D(coords, cells6, ce, be, "triangle", 2, **kw)


def unit_square(nx, ny, cell_type, degree, **kw):
    if cell_type == "quadrilateral":
        coords, cells, bottom, top = unit_square_quads(nx, ny, degree)
        return Signorini2D(coords, cells, bottom, top, "quadrilateral", degree, **kw)
    coords, cells, bottom, top = unit_square_triangles(nx, ny)
    return from_triangles(coords, cells, bottom, top, degree, **kw)


def solve_contact_problem(prob, newton_tol=1e-6, max_iterations=25, alpha_0=1.0, tol=1e-6):
    """The LVPP loop of signorini_dolfinx.py:317-358, alpha doubling.  Returns (x, it, iterations, reasons); stops after a proximal
    step whose SNES reason is <= 0, as the script does."""
    x = np.zeros(prob.ntot)
    xk = x.copy()
    nu = 2 * prob.nv
    u_prev = np.zeros(nu)
    iterations, reasons = [], []
    it = 0
    for it in range(1, max_iterations + 1):
        alpha = alpha_0 * 2**it
        solver_tol = 10 * newton_tol if it < 2 else newton_tol
        xn, reason, its = O.newton_solve(prob, x, xk, alpha, O.SnesOptions(rtol=solver_tol, atol=solver_tol, stol=1e-8, max_it=50))
        iterations.append(its)
        reasons.append(reason)
        if reason <= 0:
            break
        x = xn
        if float(np.linalg.norm(x[:nu] - u_prev)) <= tol:
            break
        u_prev = x[:nu].copy()
        xk = x.copy()
    return x, it, iterations, reasons


# ------------------------------------------------------------------------------------------------------------------
# the cases both test files use (tests/test_cpu_signorini2d.py checks that the twin converges on every one of them, so that
# tests/test_gpu_signorini2d.py never compares against a diverged reference: Newton has no line search here)
# ------------------------------------------------------------------------------------------------------------------
FLAVOURS = (("triangle", 1), ("triangle", 2), ("quadrilateral", 1), ("quadrilateral", 2))
SQUARE_RUNS = ((4, 4, 0.0), (8, 6, 0.01), (6, 6, -0.1))  # (nx, ny, gap) at disp = -0.25, alpha_0 = 1
HALF_DISK = dict(c_y=0.4, R=0.4, res=0.05)
HALF_DISK_RUNS = {1: dict(disp=-0.1, alpha_0=0.005), 2: dict(disp=-0.1, alpha_0=0.005)}  # alpha_0 = 1 diverges at degree 1 (reason -9)
SYM_RUN = ("triangle", 2, 6, 5, 0.0)
CLI_RUN = ("quadrilateral", 2, 4, 3, 0.0)  # `signorini.py --dim 2 --nx 4 --ny 3`: the script's defaults otherwise

_solved = {}


def solved_square(cell_type, degree, nx, ny, gap):
    """(prob, x, it, iterations, reasons) of a unit-square run, computed once per session"""
    key = (cell_type, degree, nx, ny, gap)
    if key not in _solved:
        prob = unit_square(nx, ny, cell_type, degree, gap=gap)
        _solved[key] = (prob,) + solve_contact_problem(prob)
    return _solved[key]


def solved_half_disk(degree, vertex_coords=None, tri_cells=None, contact_pairs=None, disp_pairs=None):
    """the half-disk run of HALF_DISK_RUNS[degree]; the mesh is the package's native one (or the arrays read back from a file: the
    same numbers), computed once per session"""
    key = ("half_disk", degree)
    if key not in _solved:
        if vertex_coords is None:
            from proximalgalerkin_amd import mesh_generation

            mesh, _, tags = mesh_generation.create_half_disk(**HALF_DISK)
            vertex_coords, tri_cells, contact_pairs, disp_pairs = mesh.geometry, mesh.cells, tags[2], tags[1]
        run = HALF_DISK_RUNS[degree]
        prob = from_triangles(vertex_coords, tri_cells, contact_pairs, disp_pairs, degree, disp=run["disp"])
        _solved[key] = (prob,) + solve_contact_problem(prob, alpha_0=run["alpha_0"])
    return _solved[key]
