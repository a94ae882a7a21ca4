"""numpy / scipy restatement of example 07 (2-D Landau-de Gennes Q-tensor with eigenvalue constraints, the reference's
examples/07_eigenvalue_constraints/eigenvalue_constraints_dolfinx.py) for the tests of the HIP family pgx_ev (include/pgx_ev.h).

Test infrastructure only: the product path is libpgx.so.  Statement by statement it restates

* the conforming map 0.5 * tanh(Psi / 2) with the script's OWN tanh (:31-33, TWICE the matrix hyperbolic tangent) in closed form,
  T(psi) = g(r) psi, g(r) = tanh(r / 2) / r, and its derivative DT = g I + (g'(r) / r) psi psi^T; `T_script` evaluates the script's
  expression itself with scipy.linalg.expm;
* the residual (:78-84) with DOLFINx's Dirichlet contract - F <- F_raw(x) + J(x)[:, bc] (g - x_bc), F[bc] = x_bc - g - and the
  true Jacobian with the rows and columns of the Dirichlet dofs replaced by the identity, in the layout x = [q1 | q2 | psi1 | psi2],
  n entries each;
* the Dirichlet data of Robinson et al. (:86-141) and the norm of the increment of Q (:157, :209);
* PETSc's newtonls with the `l2` line search as the shared driver ships it (mx_newton_solve_l2 of csrc/pgx_mixed.hip, the same
  restatement as tests/fracture_reference.py), solving with scipy's splu;
* the outer loop (:162-227).

Quadrature: EVERY term is summed with the tensor Gauss rule of `nq` points per direction (quadrature_degree // 2 + 1; the script's
degree 20 gives 11).  Dofs: the points of the p-times refined vertex lattice, row by row (x fastest); a cell's local nodes run over
its (p+1) x (p+1) sub-lattice in the same order; the basis is the product of the 1-D Lagrange bases on `nodes_1d`.  With
nodes = "equispaced" this is the numbering of proximalgalerkin_amd.lagrange.numbering_quad.  Basix's default variant puts the
nodes of degree 3 at the Gauss-Lobatto-Legendre points instead ("gll"); the spanned space Q_p is the same, and when d N is an
integer the Dirichlet data are linear on every cell edge, so their interpolant is the same FUNCTION for every node family.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SNES_CONVERGED_FNORM_ABS = 2
SNES_CONVERGED_FNORM_RELATIVE = 3
SNES_CONVERGED_SNORM_RELATIVE = 4
SNES_DIVERGED_LINEAR_SOLVE = -3
SNES_DIVERGED_FNORM_NAN = -4
SNES_DIVERGED_MAX_IT = -5
SNES_DIVERGED_LINE_SEARCH = -6
SNES_DIVERGED_DTOL = -9

R_SMALL = 1.0e-4  # below: the series (their truncation errors r^4 / 120 and 0.03 r^4 are far below the unit roundoff there)


# -- the conforming map -----------------------------------------------------------------------------------------------------------
def g_of_r(r):
    """g(r) = tanh(r / 2) / r = (1 - e) / ((1 + e) r), e = exp(-r) <= 1: finite for every finite r; g(0) = 1/2"""
    r = np.asarray(r, dtype=np.float64)
    e = np.exp(-r)
    rs = np.where(r < R_SMALL, 1.0, r)
    return np.where(r < R_SMALL, 0.5 - r * r / 24.0, (1.0 - e) / ((1.0 + e) * rs))


def gp_over_r(r):
    """g'(r) / r = (r / 2 sech^2(r / 2) - tanh(r / 2)) / r^3, sech^2(r / 2) = 4 e / (1 + e)^2"""
    r = np.asarray(r, dtype=np.float64)
    e = np.exp(-r)
    rs = np.where(r < R_SMALL, 1.0, r)
    closed = (0.5 * rs * (4.0 * e / ((1.0 + e) * (1.0 + e))) - (1.0 - e) / (1.0 + e)) / (rs * rs * rs)
    return np.where(r < R_SMALL, -1.0 / 12.0 + r * r / 60.0, closed)


def conforming(psi1, psi2):
    """(T1, T2): 0.5 * tanh(Psi / 2) = [[T1, T2], [T2, -T1]] (:83, :246)"""
    g = g_of_r(np.hypot(psi1, psi2))
    return g * psi1, g * psi2


def conforming_derivative(psi1, psi2):
    """(D11, D12, D22) of DT = g I + (g' / r) psi psi^T"""
    r = np.hypot(psi1, psi2)
    g, h = g_of_r(r), gp_over_r(r)
    return g + h * psi1 * psi1, h * psi1 * psi2, g + h * psi2 * psi2


def T_script(psi1, psi2):
    """the script's own expression (:31-33, :83) at one point: 0.5 * 2 * inv(expm(Psi) + I) @ (expm(Psi) - I) -> (T1, T2).
    In doubles the expression is ill-conditioned: expm(Psi) + I has the eigenvalues exp(+-r) + 1, so the result carries an error of
    the order eps exp(r) - measured against the closed form: 1e-14 for r <= 5, 7e-13 for r <= 10, 2e-8 for r <= 20, 3e-4 for
    r <= 30; it overflows near r = 710.  `T_script_mp` evaluates the same expression in multiple precision."""
    Psi = np.array([[psi1, psi2], [psi2, -psi1]], dtype=np.float64)
    E, Id = scipy.linalg.expm(Psi), np.eye(2)
    T = 0.5 * 2.0 * np.linalg.inv(E + Id) @ (E - Id)
    return T[0, 0], T[0, 1]


def T_script_mp(psi1, psi2, digits=60):
    """the same expression, term by term, in `digits`-digit arithmetic (mpmath.expm, mpmath.inverse) -> (T1, T2) as mpmath numbers;
    psi1, psi2 may be mpmath numbers (finite differences with steps far below the double spacing)"""
    import mpmath

    with mpmath.workdps(digits):
        Psi = mpmath.matrix([[psi1, psi2], [psi2, -mpmath.mpf(psi1)]])
        E, Id = mpmath.expm(Psi), mpmath.eye(2)
        T = mpmath.mpf("0.5") * 2 * mpmath.inverse(E + Id) * (E - Id)
        return T[0, 0], T[0, 1]


# -- Dirichlet data (:86-122) -----------------------------------------------------------------------------------------------------
def ramp(z, d):
    eps = np.finfo(np.float64).eps
    i1 = (0 <= z + eps) & (z - eps < d)
    i3 = (1 - d <= z + eps) & (z - eps <= 1)
    i2 = np.invert(i1) & np.invert(i3)
    return i1 * z / d + 1 * i2 + (1 - z) / d * i3


def boundary_data(x, y, d):
    """(g_xx, g_xy) at boundary points (:92-122)"""
    tb = np.isclose(y, 0) | np.isclose(y, 1)
    lr = np.isclose(x, 0) | np.isclose(x, 1)
    s = ramp(y, d) * lr + ramp(x, d) * tb
    tht = (np.pi / 2) * lr + 0 * tb
    return 0.5 * s * np.cos(2 * tht), 0.5 * s * np.sin(2 * tht)


# -- the 1-D bases ------------------------------------------------------------------------------------------------------------------
def nodes_1d(p, family="equispaced"):
    if family == "equispaced":
        return np.arange(p + 1) / p
    if family == "gll":  # Gauss-Lobatto-Legendre points on [0, 1]: the extrema of the Legendre polynomial of degree p, and the ends
        inner = np.polynomial.legendre.Legendre.basis(p).deriv().roots() if p > 1 else np.array([])
        return np.concatenate([[0.0], 0.5 * (np.sort(inner.real) + 1.0), [1.0]])
    raise ValueError(family)


def lagrange_1d(nodes, t):
    """values (npts, len(nodes)) and derivatives of the Lagrange basis on `nodes` at the points t"""
    t = np.asarray(t, dtype=np.float64)
    V, D = np.empty((len(t), len(nodes))), np.empty((len(t), len(nodes)))
    for i, xi in enumerate(nodes):
        val, der = np.ones_like(t), np.zeros_like(t)
        for a, xa in enumerate(nodes):
            if a != i:
                der = der * (t - xa) / (xi - xa) + val / (xi - xa)
                val = val * (t - xa) / (xi - xa)
        V[:, i], D[:, i] = val, der
    return V, D


def gauss_1d(nq):
    x, w = np.polynomial.legendre.leggauss(nq)
    return 0.5 * (x + 1.0), 0.5 * w


class Eigenvalue:
    """Residual, Jacobian and norms of example 07 on Nx x Ny rectangles over the unit square, Q_p, nq Gauss points per direction."""

    def __init__(self, Nx, Ny, p, nq, A=1.0, C=4.0, d=0.06, family="equispaced"):
        self.Nx, self.Ny, self.p, self.nq = int(Nx), int(Ny), int(p), int(nq)
        self.A, self.C, self.d = float(A), float(C), float(d)
        p1 = p + 1
        self.Lx, self.Ly = p * Nx + 1, p * Ny + 1
        self.n = self.Lx * self.Ly
        self.ndofs = 4 * self.n
        self.nb, self.nc = p1 * p1, Nx * Ny
        hx, hy = 1.0 / Nx, 1.0 / Ny
        nodes = nodes_1d(p, family)
        cx, cy = np.tile(np.arange(Nx), Ny), np.repeat(np.arange(Ny), Nx)
        loc = np.repeat(np.arange(p1), p1) * self.Lx + np.tile(np.arange(p1), p1)
        self.cd = (p * cy * self.Lx + p * cx)[:, None] + loc[None, :]  # (nc, nb), local node (iy, ix) -> iy (p+1) + ix
        gx = (np.arange(Nx)[:, None] + nodes[None, :p]).ravel() * hx
        gy = (np.arange(Ny)[:, None] + nodes[None, :p]).ravel() * hy
        gx, gy = np.append(gx, 1.0), np.append(gy, 1.0)
        self.X = np.stack([np.tile(gx, self.Ly), np.repeat(gy, self.Lx)], axis=1)
        ix, iy = np.tile(np.arange(self.Lx), self.Ly), np.repeat(np.arange(self.Ly), self.Lx)
        self.bc_nodes = np.flatnonzero((ix == 0) | (ix == self.Lx - 1) | (iy == 0) | (iy == self.Ly - 1))
        g1, g2 = boundary_data(self.X[self.bc_nodes, 0], self.X[self.bc_nodes, 1], self.d)
        self.bc = np.concatenate([self.bc_nodes, self.n + self.bc_nodes])
        self.g = np.concatenate([g1, g2])
        t, w = gauss_1d(nq)
        B, dB = lagrange_1d(nodes, t)
        # point (qy, qx) -> qy nq + qx
        self.N = (B[:, None, :, None] * B[None, :, None, :]).reshape(nq * nq, self.nb)
        self.Gx = (B[:, None, :, None] * dB[None, :, None, :]).reshape(nq * nq, self.nb) / hx
        self.Gy = (dB[:, None, :, None] * B[None, :, None, :]).reshape(nq * nq, self.nb) / hy
        self.wd = (w[:, None] * w[None, :]).ravel() * hx * hy
        self.Me = np.einsum("q,qa,qb->ab", self.wd, self.N, self.N)
        self.Ke = np.einsum("q,qa,qb->ab", self.wd, self.Gx, self.Gx) + np.einsum("q,qa,qb->ab", self.wd, self.Gy, self.Gy)
        self.rows = np.repeat(self.cd, self.nb, axis=1).ravel()
        self.cols = np.tile(self.cd, (1, self.nb)).ravel()
        self.M = self._scalar(np.broadcast_to(self.Me, (self.nc, self.nb, self.nb)))
        self.K = self._scalar(np.broadcast_to(self.Ke, (self.nc, self.nb, self.nb)))

    # -- helpers ------------------------------------------------------------------------------------------------
    def _scalar(self, Ae):
        return sp.coo_matrix((np.asarray(Ae).ravel(), (self.rows, self.cols)), shape=(self.n, self.n)).tocsr()

    def _vec(self, Re):
        return np.bincount(self.cd.ravel(), weights=Re.ravel(), minlength=self.n)

    def _at_q(self, f):
        return f[self.cd] @ self.N.T  # (nc, npts)

    def _wmass(self, coef):
        """the mass form weighted by a coefficient given at the points of every cell"""
        return self._scalar(np.einsum("cq,qa,qb->cab", coef * self.wd, self.N, self.N))

    def split(self, x):
        n = self.n
        return x[:n], x[n:2 * n], x[2 * n:3 * n], x[3 * n:]

    # -- forms (:78-84) ---------------------------------------------------------------------------------------------
    def residual_raw(self, x, z_iter, alpha):
        q1, q2, p1, p2 = self.split(x)
        pk1, pk2 = self.split(z_iter)[2:]
        a1, a2, b1, b2 = self._at_q(q1), self._at_q(q2), self._at_q(p1), self._at_q(p2)
        c1, c2 = self._at_q(pk1), self._at_q(pk2)
        s = a1 * a1 + a2 * a2
        pot = 2.0 * self.A + 4.0 * self.C * s
        t1, t2 = conforming(b1, b2)
        out = []
        for qi, ai, bi, ci in ((q1, a1, b1, c1), (q2, a2, b2, c2)):
            Re = alpha * (2.0 * (qi[self.cd] @ self.Ke) + (self.wd * pot * ai) @ self.N) + 2.0 * (self.wd * (bi - ci)) @ self.N
            out.append(self._vec(Re))
        for ai, ti in ((a1, t1), (a2, t2)):
            out.append(self._vec(2.0 * (self.wd * (ai - ti)) @ self.N))
        return np.concatenate(out)

    def jacobian_raw(self, x, alpha):
        q1, q2, p1, p2 = self.split(x)
        a1, a2, b1, b2 = self._at_q(q1), self._at_q(q2), self._at_q(p1), self._at_q(p2)
        pot = 2.0 * self.A + 4.0 * self.C * (a1 * a1 + a2 * a2)
        C8 = 8.0 * self.C
        E11 = alpha * (2.0 * self.K + self._wmass(pot + C8 * a1 * a1))
        E12 = alpha * self._wmass(C8 * a1 * a2)
        E22 = alpha * (2.0 * self.K + self._wmass(pot + C8 * a2 * a2))
        d11, d12, d22 = conforming_derivative(b1, b2)
        M2 = 2.0 * self.M
        return sp.bmat([[E11, E12, M2, None], [E12, E22, None, M2],
                        [M2, None, -2.0 * self._wmass(d11), -2.0 * self._wmass(d12)],
                        [None, M2, -2.0 * self._wmass(d12), -2.0 * self._wmass(d22)]], format="csr")

    def residual(self, x, z_iter, alpha):
        F = self.residual_raw(x, z_iter, alpha)
        J = self.jacobian_raw(x, alpha).tocsc()
        F = F + J[:, self.bc] @ (self.g - x[self.bc])
        F[self.bc] = x[self.bc] - self.g
        return F

    def jacobian(self, x, alpha):
        J = self.jacobian_raw(x, alpha).tolil()
        J[self.bc, :] = 0.0
        J[:, self.bc] = 0.0
        J[self.bc, self.bc] = 1.0
        return J.tocsr()

    def l2_increment_Q(self, x, z_iter):
        """sqrt(int inner(Q - Q_iter, Q - Q_iter)) (:157, :209): inner of two such tensors carries a factor 2"""
        d1, d2 = self.split(x)[0] - self.split(z_iter)[0], self.split(x)[1] - self.split(z_iter)[1]
        return float(np.sqrt(max(2.0 * (d1 @ (self.M @ d1) + d2 @ (self.M @ d2)), 0.0)))

    def eval_nodes(self, x):
        """(4, n): the conforming approximation (T1, T2) and the largest / smallest eigenvalue of Q per dof (:245-259)"""
        q1, q2, p1, p2 = self.split(x)
        t1, t2 = conforming(p1, p2)
        m = np.hypot(q1, q2)
        return np.stack([t1, t2, m, -m])

    # -- SNES newtonls + linesearch l2 (:143), PETSc's defaults otherwise ------------------------------------------------
    def newton_l2(self, z, z_iter, alpha, atol=1e-50, rtol=1e-8, stol=1e-8, max_it=50, divtol=1e4, maxlambda=1.0, steptol=1e-12,
                  monitor=False):
        """-> (last iterate, reason, its)"""
        res = lambda y: self.residual(y, z_iter, alpha)  # noqa: E731
        z = z.copy()
        F = res(z)
        fnorm = fnorm0 = float(np.linalg.norm(F))
        if monitor:
            print(f"  0 SNES Function norm {fnorm:.12e}")
        if not np.isfinite(fnorm):
            return z, SNES_DIVERGED_FNORM_NAN, 0
        if fnorm < atol:
            return z, SNES_CONVERGED_FNORM_ABS, 0
        ttol = fnorm * rtol
        for it in range(1, max_it + 1):
            J = self.jacobian(z, alpha)
            try:
                with np.errstate(all="ignore"):
                    y = spla.splu(J.tocsc()).solve(F)
            except RuntimeError:
                return z, SNES_DIVERGED_LINEAR_SOLVE, it - 1
            if not np.all(np.isfinite(y)):
                return z, SNES_DIVERGED_LINEAR_SOLVE, it
            lam, lam_old, maxl = 1.0, 0.0, maxlambda
            fn_old = fnorm * fnorm
            lam_mid = 0.5 * (lam + lam_old)
            failed = False
            for _ in range(1):  # -snes_linesearch_max_it of l2: 1
                while True:
                    fm = np.linalg.norm(res(z - lam_mid * y)) ** 2
                    fe = np.linalg.norm(res(z - lam * y)) ** 2
                    if np.isfinite(fe):
                        break
                    if lam <= steptol:
                        failed = True
                        break
                    maxl = 0.95 * lam
                    lam = 0.5 * (lam + lam_old)
                    lam_mid = 0.5 * (lam + lam_old)
                if failed:
                    break
                dl = lam - lam_old
                d1 = (3.0 * fe - 4.0 * fm + fn_old) / dl
                d1_old = (-3.0 * fn_old + 4.0 * fm - fe) / dl
                d2 = (d1 - d1_old) / dl
                if d2 > 0.0:
                    upd = lam - d1 / d2
                elif d2 < 0.0:
                    upd = lam + d1 / d2
                else:
                    break
                if upd < steptol:
                    upd = 0.5 * (lam + lam_old)
                if not np.isfinite(upd) or upd > maxl:
                    break
                lam_old, lam, fn_old = lam, upd, fe
                lam_mid = 0.5 * (lam + lam_old)
            if failed:
                return z, SNES_DIVERGED_LINE_SEARCH, it
            z = z - lam * y
            F = res(z)
            fnorm = float(np.linalg.norm(F))
            if monitor:
                print(f"      line search: lambda {lam:.6e}\n  {it} SNES Function norm {fnorm:.12e}")
            if not np.isfinite(fnorm):
                return z, SNES_DIVERGED_FNORM_NAN, it
            if fnorm < atol:
                return z, SNES_CONVERGED_FNORM_ABS, it
            if fnorm <= ttol:
                return z, SNES_CONVERGED_FNORM_RELATIVE, it
            if np.linalg.norm(y) < stol * np.linalg.norm(z):
                return z, SNES_CONVERGED_SNORM_RELATIVE, it
            if fnorm > divtol * fnorm0:
                return z, SNES_DIVERGED_DTOL, it
        return z, SNES_DIVERGED_MAX_IT, max_it


def solve(prob: Eigenvalue, nfail_max=50, nlvpp_max=100, r=2, z0=None, verbose=False, **newton_kw):
    """The outer loop (:162-227).  -> dict(log, newton_its, z); log rows are (k, alpha, its, reason, failed), k = nlvpp at the time
    of the attempt."""
    z = np.zeros(prob.ndofs) if z0 is None else np.array(z0, dtype=np.float64)
    z_prev = np.zeros(prob.ndofs)  # never written by the script: the failed first step restarts from zero (:192-193)
    z_iter = np.zeros(prob.ndofs)
    alpha, nfail, nlvpp = 1.0, 0, 0
    log, newton = [], []
    while nfail < nfail_max and nlvpp < nlvpp_max:
        z_new, reason, its = prob.newton_l2(z, z_iter, alpha, **newton_kw)
        if (its == 0 and reason > 0) or reason < 0:
            nfail += 1
            log.append((nlvpp, alpha, its, reason, 1))
            if verbose:
                print(f"failed ({reason}) nlvpp={nlvpp} alpha={alpha}", flush=True)
            alpha /= 2
            z = (z_prev if nlvpp == 0 else z_iter).copy()
            if nfail >= nfail_max:
                break
            continue
        z = z_new
        log.append((nlvpp, alpha, its, reason, 0))
        newton.append(its)
        nlvpp += 1
        nrm = prob.l2_increment_Q(z, z_iter)
        if verbose:
            print(f"solved nlvpp={nlvpp} its={its} alpha={alpha} increment={nrm}", flush=True)
        if nrm < 1.0e-10:
            break
        if its <= 4:
            alpha *= r
        elif its >= 10:
            alpha /= r
        z_iter = z.copy()
    return dict(log=np.array(log, dtype=np.float64).reshape(-1, 5), newton_its=np.array(newton, dtype=np.int32), z=z)


def logs_agree(a, b):
    """The comparison rule of the recorded runs (that of tests/fracture_reference.py): successful attempts agree on
    (k, alpha, its, reason); failed attempts only on (k, alpha) and on the fact of failure."""
    a, b = np.asarray(a, float).reshape(-1, 5), np.asarray(b, float).reshape(-1, 5)
    if a.shape != b.shape:
        return False
    fa, fb = a[:, 4] != 0, b[:, 4] != 0
    if not np.array_equal(fa, fb) or not np.array_equal(a[:, :2], b[:, :2]):
        return False
    return bool(np.array_equal(a[~fa, 2:4], b[~fb, 2:4]))


def field_differences(n, za, zb):
    """max-norm differences of the (q1, q2, psi1, psi2) blocks of two states; the psi blocks relative to max |psi| of the second"""
    d = [float(np.abs(za[k * n:(k + 1) * n] - zb[k * n:(k + 1) * n]).max()) for k in range(4)]
    scale = max(float(np.abs(zb[2 * n:]).max()), 1e-300)
    d[2] /= scale
    d[3] /= scale
    return np.array(d)


def field_tolerances(golden):
    """what a rerun of a recorded run may differ by, per field: max(1e-10, 10 x the recorded sensitivity)"""
    return np.maximum(1e-10, 10.0 * np.asarray(golden["sensitivity"], dtype=np.float64))
