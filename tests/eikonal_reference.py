"""numpy / scipy restatement of example 09 (the eikonal equation on a Moebius strip, the reference's
examples/09_eikonal/eikonal_dolfinx.py) for the tests of the HIP family pgx_ek (include/pgx_ek.h).

Test infrastructure only: the product path is libpgx.so.  It has its OWN numbering and its OWN geometry code and imports neither from
the package, so that a wrong seam in one of the two cannot cancel against the other.  Statement by statement it restates

* the strip: parameter cells [2 pi cx / nu, 2 pi (cx + 1) / nu] x [cy / nv, (cy + 1) / nv] mapped by
  x(s, t) = scale ((1 + rho cos(s / 2)) cos s, (1 + rho cos(s / 2)) sin s, rho sin(s / 2)), rho = (t - 1/2) / 2, every cell's
  (g + 1)^2 geometry nodes sampled at its own unwrapped parameters;
* the Q_k lattice: columns I = 0 .. k nu - 1, rows J = 0 .. k nv, dof J (k nu) + I; column k nu is column 0 with J -> k nv - J;
* the spaces u in Q1, psi in [Q2]^3 (ambient components), x = [u | psi0 | psi1 | psi2], no Dirichlet rows (:29-32, :78-80);
* UFL's manifold operators: J = dx/dX (3 x 2), G = J^T J, K = G^-1 J^T, dS = sqrt(det G), grad_G N = (dN/dX) K,
  div_G psi = sum_i (grad_G psi_i)_i;
* the residual (:52-58) and its true derivative [[0, B], [B^T, D(psi)]] (:61);
* the norm of the increment of u (:88-90, :160-161) and the DG outputs u, grad(u), psi at the Q_g nodes of every cell (:84-86, :134-148);
* PETSc's newtonls with the `l2` line search as the shared driver ships it (the same restatement as tests/eigenvalue_reference.py),
  solving with scipy's splu, and the outer loop (:149-174).

Quadrature: every term uses the tensor Gauss rule of `nq` points per direction; a cell's local nodes run over its (k+1) x (k+1)
sub-lattice, first direction fastest; points likewise.
"""
from __future__ import annotations

import numpy as np
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


class NotConvergedError(Exception):
    pass


def mobius(s, t, scale=1.0):
    rho = 0.5 * (np.asarray(t, dtype=np.float64) - 0.5)
    a = 1.0 + rho * np.cos(0.5 * s)
    return scale * np.stack([a * np.cos(s), a * np.sin(s), rho * np.sin(0.5 * s)], axis=-1)


def numbering(nu, nv, k):
    """-> (n, cell dofs (nu nv, (k+1)^2)): cell cy nu + cx, local node b (k+1) + a"""
    Lu = k * nu
    cd = np.empty((nu * nv, (k + 1) ** 2), dtype=np.int64)
    for cy in range(nv):
        for cx in range(nu):
            for b in range(k + 1):
                for a in range(k + 1):
                    I, J = k * cx + a, k * cy + b
                    if I == Lu:  # the seam: upside down
                        I, J = 0, k * nv - J
                    cd[cy * nu + cx, b * (k + 1) + a] = J * Lu + I
    return Lu * (k * nv + 1), cd


def lagrange_1d(k, t):
    """values (npts, k+1) and derivatives of the Lagrange basis on the nodes i / k"""
    t = np.asarray(t, dtype=np.float64)
    nodes = np.arange(k + 1) / k
    V, D = np.empty((len(t), k + 1)), np.empty((len(t), k + 1))
    for i, xi in enumerate(nodes):
        val, der = np.ones_like(t), np.zeros_like(t)
        for a, xa in enumerate(nodes):
            if a != i:
                der = der * (t - xa) / (xi - xa) + val / (xi - xa)
                val = val * (t - xa) / (xi - xa)
        V[:, i], D[:, i] = val, der
    return V, D


def tensor_tables(k, tx, ty):
    """Q_k at the points (tx[p], ty[p]): values (npts, (k+1)^2) and reference gradients (npts, (k+1)^2, 2)"""
    Vx, Dx = lagrange_1d(k, tx)
    Vy, Dy = lagrange_1d(k, ty)
    n = len(tx)
    V = (Vy[:, :, None] * Vx[:, None, :]).reshape(n, -1)
    G = np.stack([(Vy[:, :, None] * Dx[:, None, :]).reshape(n, -1), (Dy[:, :, None] * Vx[:, None, :]).reshape(n, -1)], axis=2)
    return V, G


def gauss_1d(nq):
    x, w = np.polynomial.legendre.leggauss(nq)
    return 0.5 * (x + 1.0), 0.5 * w


class Eikonal:
    """Residual, Jacobian, norms and outputs of example 09 on the nu x nv strip with geometry order g and nq points per direction."""

    def __init__(self, nu, nv, g=3, nq=6, scale=1.0, f=1.0, phi=1.0):
        self.nu, self.nv, self.g, self.nq = int(nu), int(nv), int(g), int(nq)
        self.scale, self.f, self.phi = float(scale), float(f), float(phi)
        self.n1, self.cd1 = numbering(nu, nv, 1)
        self.n2, self.cd2 = numbering(nu, nv, 2)
        self.nc = nu * nv
        self.ndofs = self.n1 + 3 * self.n2
        cx, cy = np.arange(self.nc) % nu, np.arange(self.nc) // nu
        lat = np.arange(g + 1) / g
        S = 2.0 * np.pi * (cx[:, None] + np.tile(lat, g + 1)[None, :]) / nu
        T = (cy[:, None] + np.repeat(lat, g + 1)[None, :]) / nv
        self.X = mobius(S, T, self.scale)  # (nc, (g+1)^2, 3): every cell at its own unwrapped parameters
        t, w = gauss_1d(nq)
        tx, ty = np.tile(t, nq), np.repeat(t, nq)
        self.W = (w[:, None] * w[None, :]).ravel()
        self.N1, self.G1 = tensor_tables(1, tx, ty)
        self.N2, self.G2 = tensor_tables(2, tx, ty)
        _, Gg = tensor_tables(g, tx, ty)
        self.K, dS = self._pinv(Gg)
        self.wd = self.W[None, :] * dS  # (nc, npts)
        self.D1 = np.einsum("qna,cqai->cqni", self.G1, self.K)  # surface gradients of the bases, (nc, npts, nodes, 3)
        self.D2 = np.einsum("qna,cqai->cqni", self.G2, self.K)
        # B = (div_G psi, v): rows u, columns [psi0 | psi1 | psi2]
        Be = np.einsum("cq,qa,cqbi->caib", self.wd, self.N1, self.D2)  # (nc, 4, 3, 9)
        rows = np.broadcast_to(self.cd1[:, :, None, None], Be.shape)
        cols = np.arange(3)[None, None, :, None] * self.n2 + self.cd2[:, None, None, :]
        self.B = sp.coo_matrix((Be.ravel(), (rows.ravel(), np.broadcast_to(cols, Be.shape).ravel())), shape=(self.n1, 3 * self.n2)).tocsr()
        self.fv = np.bincount(self.cd1.ravel(), weights=(self.f * self.wd @ self.N1).ravel(), minlength=self.n1)  # (f, v)
        Me = np.einsum("cq,qa,qb->cab", self.wd, self.N1, self.N1)
        self.M1 = sp.coo_matrix((Me.ravel(), (np.repeat(self.cd1, 4, axis=1).ravel(), np.tile(self.cd1, (1, 4)).ravel())),
                                shape=(self.n1, self.n1)).tocsr()
        self.r2 = np.repeat(self.cd2, 9, axis=1).ravel()
        self.c2 = np.tile(self.cd2, (1, 9)).ravel()

    def _pinv(self, Gg):
        """K = G^-1 J^T (nc, npts, 2, 3) and dS = sqrt(det G) at the points whose Q_g reference gradients are Gg"""
        Jm = np.einsum("qna,cni->cqia", Gg, self.X)  # (nc, npts, 3, 2)
        Gm = np.einsum("cqia,cqib->cqab", Jm, Jm)
        det = Gm[..., 0, 0] * Gm[..., 1, 1] - Gm[..., 0, 1] * Gm[..., 1, 0]
        Gi = np.stack([np.stack([Gm[..., 1, 1], -Gm[..., 0, 1]], -1), np.stack([-Gm[..., 1, 0], Gm[..., 0, 0]], -1)], -2) / det[..., None, None]
        return np.einsum("cqab,cqib->cqai", Gi, Jm), np.sqrt(det)

    def area(self):
        return float(self.wd.sum())

    def split(self, x):
        n1, n2 = self.n1, self.n2
        return x[:n1], x[n1:].reshape(3, n2)

    def _psi_q(self, psi):
        return np.einsum("icb,qb->cqi", psi[:, self.cd2], self.N2)  # (nc, npts, 3)

    def residual(self, x, x_prev, alpha):
        u, psi = self.split(x)
        _, psi0 = self.split(x_prev)
        pq = self._psi_q(psi)
        s = np.sqrt(1.0 + (pq * pq).sum(axis=2))
        Rv = self.B @ (psi - psi0).ravel() + alpha * self.fv
        Re = self.phi * np.einsum("cq,cqi,qb->icb", self.wd / s, pq, self.N2)
        Rt = self.B.T @ u + np.concatenate([np.bincount(self.cd2.ravel(), weights=Re[i].ravel(), minlength=self.n2) for i in range(3)])
        return np.concatenate([Rv, Rt])

    def D(self, x):
        _, psi = self.split(x)
        pq = self._psi_q(psi)
        s = np.sqrt(1.0 + (pq * pq).sum(axis=2))
        blocks = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(i, 3):
                co = self.phi * self.wd * ((1.0 if i == j else 0.0) / s - pq[:, :, i] * pq[:, :, j] / s ** 3)
                De = np.einsum("cq,qa,qb->cab", co, self.N2, self.N2)
                De = 0.5 * (De + De.transpose(0, 2, 1))  # both triangles from the same sums: symmetric to the last bit
                blocks[i][j] = sp.coo_matrix((De.ravel(), (self.r2, self.c2)), shape=(self.n2, self.n2)).tocsr()
                blocks[j][i] = blocks[i][j]
        return sp.bmat(blocks, format="csr")

    def jacobian(self, x):
        return sp.bmat([[sp.csr_matrix((self.n1, self.n1)), self.B], [self.B.T, self.D(x)]], format="csr")

    def l2_increment_u(self, x, x_prev):
        d = x[:self.n1] - x_prev[:self.n1]
        return float(np.sqrt(max(d @ (self.M1 @ d), 0.0)))

    def eval_cells(self, x):
        """(nc, (g+1)^2, 7): u, grad_G u (3), psi (3) at the Q_g interpolation nodes of every cell"""
        g = self.g
        lat = np.arange(g + 1) / g
        tx, ty = np.tile(lat, g + 1), np.repeat(lat, g + 1)
        N1, G1 = tensor_tables(1, tx, ty)
        N2, _ = tensor_tables(2, tx, ty)
        _, Gg = tensor_tables(g, tx, ty)
        K, _ = self._pinv(Gg)
        u, psi = self.split(x)
        uc = u[self.cd1]
        out = np.empty((self.nc, (g + 1) ** 2, 7))
        out[:, :, 0] = uc @ N1.T
        out[:, :, 1:4] = np.einsum("cn,qna,cqai->cqi", uc, G1, K)
        out[:, :, 4:7] = np.einsum("icb,qb->cqi", psi[:, self.cd2], N2)
        return out

    # -- SNES newtonls + linesearch l2 (:67), the script's tolerances (:68-71) -----------------------------------------------
    def newton_l2(self, z, z_prev, alpha, atol=1e-5, rtol=1e-5, stol=1e-5, max_it=100, divtol=1e4, maxlambda=1.0, steptol=1e-12,
                  monitor=False):
        """-> (last iterate, reason, its)"""
        res = lambda y: self.residual(y, z_prev, alpha)  # noqa: E731
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
            J = self.jacobian(z)
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


def solve(prob: Eikonal, tol=1e-5, max_it=100, z0=None, verbose=False):
    """The outer loop (:149-174).  -> dict(log, increments, z); log rows are (i, alpha, Newton its, reason).  A step that does not
    converge raises NotConvergedError (snes_error_if_not_converged, :74)."""
    z = np.zeros(prob.ndofs) if z0 is None else np.array(z0, dtype=np.float64)
    z_prev = np.zeros(prob.ndofs)
    log, inc = [], []
    for i in range(1, 100):
        alpha = min(2 ** i, 10)
        z, reason, its = prob.newton_l2(z, z_prev, alpha, atol=tol, rtol=tol, stol=tol, max_it=max_it)
        if reason <= 0:
            raise NotConvergedError(f"step {i}: reason {reason} after {its} iterations")
        d = prob.l2_increment_u(z, z_prev)
        log.append((i, alpha, its, reason))
        inc.append(d)
        if verbose:
            print(f"Iteration {i}: its={its} reason={reason} |delta u|={d}", flush=True)
        z_prev = z.copy()
        if d < 5 * tol:
            break
    return dict(log=np.array(log, dtype=np.float64).reshape(-1, 4), increments=np.array(inc), z=z)


def field_differences(n1, za, zb):
    """(u absolute, psi relative to max |psi| of the second) max-norm differences of two states"""
    scale = max(float(np.abs(zb[n1:]).max()), 1e-300)
    return np.array([float(np.abs(za[:n1] - zb[:n1]).max()), float(np.abs(za[n1:] - zb[n1:]).max()) / scale])


def field_tolerances(golden):
    """what a rerun of a recorded run may differ by, per field: max(1e-10, 10 x the recorded sensitivity)"""
    return np.maximum(1e-10, 10.0 * np.asarray(golden["sensitivity"], dtype=np.float64))
