"""numpy / scipy restatement of example 03 (phase-field fracture under load stepping, the reference's
examples/03_fracture/fracture_dolfinx.py) for the tests of the HIP family pgx_fr (include/pgx_fr.h).

Test infrastructure only: the product path is libpgx.so.  Statement by statement it restates

* the residual (:118-130) with DOLFINx's Dirichlet contract - F <- F_raw(x) + J_reg(x)[:, bc] (g - x_bc), F[bc] = x_bc - g - and the
  modified Jacobian J_reg (:132-138) with the rows and columns of the Dirichlet dofs replaced by the identity, in the layout
  x = [u | c | psi], nv entries each;
* the two L2 distances (:187-188) and c_conform (:114) at reference points;
* PETSc's newtonls with the `l2` line search as the shared driver ships it (mx_newton_solve_l2 of csrc/pgx_mixed.hip, the same
  restatement as oracle/ic_oracle.py::newton_l2: the stol test reads the UNSCALED direction), solving with scipy's splu;
* the load-step loop (:207-311).

Quadrature: every term, polynomial or not, is summed with the 16-point degree-7 table tri_deg7_gj16, which integrates the
polynomial ones (degree <= 4) exactly.  The kernels integrate those in closed form instead: agreement to rounding checks both.
"""
from __future__ import annotations

import json
import pathlib

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.special import expit

_TABLES = pathlib.Path(__file__).resolve().parents[1] / "proximalgalerkin_amd" / "tables" / "quadrature.json"

SNES_CONVERGED_FNORM_ABS = 2
SNES_CONVERGED_FNORM_RELATIVE = 3
SNES_CONVERGED_SNORM_RELATIVE = 4
SNES_DIVERGED_LINEAR_SOLVE = -3
SNES_DIVERGED_FNORM_NAN = -4
SNES_DIVERGED_MAX_IT = -5
SNES_DIVERGED_LINE_SEARCH = -6
SNES_DIVERGED_DTOL = -9

# the 10 nodes of P3 on the reference triangle (vertices, two per edge, centre): where the script interpolates c_conform (:111-115)
P3_NODES = np.array([[0, 0], [1, 0], [0, 1], [2 / 3, 1 / 3], [1 / 3, 2 / 3], [0, 2 / 3], [0, 1 / 3], [1 / 3, 0], [2 / 3, 0],
                     [1 / 3, 1 / 3]], dtype=np.float64)


def quadrature7():
    t = json.loads(_TABLES.read_text())["tri_deg7_gj16"]
    return np.array(t["points"]), np.array(t["weights"])


def boundary_vertices(edges, tags, tag):
    return np.unique(np.asarray(edges)[np.asarray(tags) == tag]).astype(np.int32)


class Fracture:
    """Residual, Jacobian and the P1 forms of example 03 on a triangle mesh.  bc_minus / bc_plus: the vertices of `topleft`
    (u = -T) and `topright` (u = +T) (:141-160)."""

    def __init__(self, coords, cells, bc_minus, bc_plus, G=1.0, Gc=1.0, l=None, eps=1e-5, reps=1e-3):
        self.coords, self.cells = np.asarray(coords, float), np.asarray(cells, np.int64)
        self.nv, self.nc = len(self.coords), len(self.cells)
        self.ndofs = 3 * self.nv
        self.G, self.Gc, self.eps, self.reps = float(G), float(Gc), float(eps), float(reps)
        X = self.coords[self.cells]
        j00, j10 = X[:, 1, 0] - X[:, 0, 0], X[:, 1, 1] - X[:, 0, 1]
        j01, j11 = X[:, 2, 0] - X[:, 0, 0], X[:, 2, 1] - X[:, 0, 1]
        det = j00 * j11 - j01 * j10
        i00, i01, i10, i11 = j11 / det, -j01 / det, -j10 / det, j00 / det
        g = np.empty((self.nc, 3, 2))
        g[:, 1, 0], g[:, 1, 1], g[:, 2, 0], g[:, 2, 1] = i00, i01, i10, i11
        g[:, 0, 0], g[:, 0, 1] = -(i00 + i10), -(i01 + i11)
        self.grad = g
        self.adet = np.abs(det)
        e = [np.linalg.norm(X[:, (k + 1) % 3] - X[:, (k + 2) % 3], axis=1) for k in range(3)]
        self.l = float(np.max(4.0 * e[0] * e[1] * e[2] / (4.0 * 0.5 * self.adet))) if l is None else float(l)  # :88-93
        pts, wts = quadrature7()
        self.N = np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1)  # (nq, 3)
        self.wd = wts[None, :] * self.adet[:, None]  # (nc, nq)
        self.NN = np.einsum("qa,qb->qab", self.N, self.N)
        self.Me = np.einsum("cq,qab->cab", self.wd, self.NN)
        self.Ke = self.wd.sum(axis=1)[:, None, None] * np.einsum("cad,cbd->cab", g, g)
        self.bc_minus = np.asarray(bc_minus, np.int64)
        self.bc_plus = np.asarray(bc_plus, np.int64)
        self.bc = np.concatenate([self.bc_minus, self.bc_plus])
        self.sign = np.concatenate([-np.ones(len(self.bc_minus)), np.ones(len(self.bc_plus))])
        self.rows = np.repeat(self.cells, 3, axis=1).ravel()  # (c, a, b) -> cells[c, a]
        self.cols = np.tile(self.cells, (1, 3)).ravel()       # (c, a, b) -> cells[c, b]
        self.M = self._scalar(self.Me)

    # -- helpers ------------------------------------------------------------------------------------------------
    def _scalar(self, Ae):
        return sp.coo_matrix((Ae.ravel(), (self.rows, self.cols)), shape=(self.nv, self.nv)).tocsr()

    def _vec(self, Re):
        return np.bincount(self.cells.ravel(), weights=Re.ravel(), minlength=self.nv)

    def _at_q(self, f):
        return f[self.cells] @ self.N.T  # (nc, nq)

    def split(self, x):
        n = self.nv
        return x[:n], x[n:2 * n], x[2 * n:]

    def g_values(self, T):
        return self.sign * float(T)

    # -- forms --------------------------------------------------------------------------------------------------
    def residual_raw(self, x, z_iter, z_prev, alpha):
        u, c, p = self.split(x)
        pk = self.split(z_iter)[2]
        cp = self.split(z_prev)[1]
        e, g = self.eps, self.grad
        gu = np.einsum("ca,cad->cd", u[self.cells], g)
        gc = np.einsum("ca,cad->cd", c[self.cells], g)
        g2 = (gu * gu).sum(axis=1)
        cq, pq, pkq, cpq = self._at_q(c), self._at_q(p), self._at_q(pk), self._at_q(cp)
        w = (1.0 - e) * (1.0 - cq) ** 2 + e
        dw = -2.0 * (1.0 - e) * (1.0 - cq)
        Rv = alpha * self.G * (self.wd * w).sum(axis=1)[:, None] * np.einsum("cd,cad->ca", gu, g)
        dens = alpha * (0.5 * self.G * dw * g2[:, None] + self.Gc / self.l * cq) + pq - pkq
        Rd = (self.wd * dens) @ self.N + alpha * self.Gc * self.l * self.wd.sum(axis=1)[:, None] * np.einsum("cd,cad->ca", gc, g)
        conf = cpq + (1.0 - cpq) * expit(pq)
        Rp = (self.wd * (cq - conf)) @ self.N
        return np.concatenate([self._vec(Rv), self._vec(Rd), self._vec(Rp)])

    def jacobian_raw(self, x, z_prev, alpha, reps=None):
        """J_reg (:132-138) before the Dirichlet rows; reps=0: the true derivative of residual_raw"""
        reps = self.reps if reps is None else float(reps)
        u, c, p = self.split(x)
        cp = self.split(z_prev)[1]
        e, g = self.eps, self.grad
        gu = np.einsum("ca,cad->cd", u[self.cells], g)
        g2 = (gu * gu).sum(axis=1)
        cq, pq, cpq = self._at_q(c), self._at_q(p), self._at_q(cp)
        w = (1.0 - e) * (1.0 - cq) ** 2 + e
        dw = -2.0 * (1.0 - e) * (1.0 - cq)
        gg = np.einsum("cad,cbd->cab", g, g)
        uu = alpha * self.G * (self.wd * w).sum(axis=1)[:, None, None] * gg + reps * self.Me
        uc = alpha * self.G * np.einsum("ca,cb->cab", np.einsum("cd,cad->ca", gu, g), (self.wd * dw) @ self.N)
        cc = alpha * ((self.G * (1.0 - e) * g2[:, None, None] + self.Gc / self.l) * self.Me + self.Gc * self.l * self.Ke) + reps * self.Me
        s = expit(pq)
        pp = -np.einsum("cq,qab->cab", self.wd * (1.0 - cpq) * s * expit(-pq), self.NN) - reps * self.Me
        S = self._scalar
        return sp.bmat([[S(uu), S(uc), None], [S(uc.transpose(0, 2, 1)), S(cc), self.M], [None, self.M, S(pp)]], format="csr")

    def residual(self, x, z_iter, z_prev, alpha, T):
        F = self.residual_raw(x, z_iter, z_prev, alpha)
        gv = self.g_values(T)
        J = self.jacobian_raw(x, z_prev, alpha).tocsc()
        F = F + J[:, self.bc] @ (gv - x[self.bc])
        F[self.bc] = x[self.bc] - gv
        return F

    def jacobian(self, x, z_prev, alpha):
        J = self.jacobian_raw(x, z_prev, alpha).tolil()
        J[self.bc, :] = 0.0
        J[:, self.bc] = 0.0
        J[self.bc, self.bc] = 1.0
        return J.tocsr()

    def l2(self, d):
        return float(np.sqrt(max(d @ (self.M @ d), 0.0)))

    def l2_increment_c(self, x, z_iter):
        return self.l2(self.split(x)[1] - self.split(z_iter)[1])  # :187

    def l2_distance(self, x, y):
        return float(np.sqrt(sum(self.l2(a - b) ** 2 for a, b in zip(self.split(x), self.split(y)))))  # :188

    def conforming_damage(self, x, z_prev, ref_pts=P3_NODES):
        """c_conform (:114) at the reference points of every cell, (nc, npts)"""
        ref_pts = np.asarray(ref_pts, float)
        N = np.stack([1.0 - ref_pts[:, 0] - ref_pts[:, 1], ref_pts[:, 0], ref_pts[:, 1]], axis=1)
        pq = self.split(x)[2][self.cells] @ N.T
        cpq = self.split(z_prev)[1][self.cells] @ N.T
        return cpq + (1.0 - cpq) * expit(pq)

    # -- SNES newtonls + linesearch l2, maxlambda 1 (:163-171) -------------------------------------------------------
    def newton_l2(self, z, z_iter, z_prev, alpha, T, atol=1e-6, rtol=1e-8, stol=1e-8, max_it=50, divtol=1e4, maxlambda=1.0,
                  steptol=1e-12, monitor=False):
        """-> (last iterate, reason, its)"""
        res = lambda y: self.residual(y, z_iter, z_prev, alpha, T)  # noqa: E731
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
            J = self.jacobian(z, z_prev, alpha)
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


def solve(prob: Fracture, num_load_steps=1001, Tmin=0.0, Tmax=5.0, nfail_max=50, write_frequency=25, z0=None, verbose=False,
          **newton_kw):
    """The load-step loop (:207-311).  -> dict(log, newton_its, lvpp_its, z, z_prev, max_conform); log rows are
    (step, k, alpha, its, reason, increment), increment = nan for a failed attempt."""
    z = np.zeros(prob.ndofs) if z0 is None else np.array(z0, dtype=np.float64)
    z_prev = np.zeros(prob.ndofs)
    log, newton, lvpp, max_conform = [], [], [], []
    for step, T in enumerate(np.linspace(Tmin, Tmax, num_load_steps)[1:]):
        alpha = 1.0
        z_iter = z.copy()
        k, r, nfail = 1, 2, 0
        newton.append(0)
        lvpp.append(0)
        while nfail <= nfail_max:
            z_new, reason, its = prob.newton_l2(z, z_iter, z_prev, alpha, T, **newton_kw)
            newton[-1] += its
            if (its == 0 and reason > 0) or reason < 0:
                nfail += 1
                log.append((step, k, alpha, its, reason, np.nan))
                if verbose:
                    print(f"step {step} T={T} failed ({reason}) k={k} alpha={alpha}", flush=True)
                alpha /= 2
                z = (z_prev if k == 1 else z_iter).copy()
                if nfail >= nfail_max:
                    break
                continue
            z = z_new
            nrm = prob.l2_increment_c(z, z_iter)
            log.append((step, k, alpha, its, reason, nrm))
            lvpp[-1] += 1
            if verbose:
                print(f"step {step} T={T} solved k={k} its={its} alpha={alpha} increment={nrm}", flush=True)
            if nrm < 1.0e-4:
                break
            if its <= 4:
                alpha *= r
            elif its >= 10:
                alpha /= r
            z_iter = z.copy()
            k += 1
        norm_Z = prob.l2_distance(z, z_prev)
        if k == 1 and np.isclose(norm_Z, 0.0):
            break
        if nfail == nfail_max:
            break
        max_conform.append(float(prob.conforming_damage(z, z_prev).max()))
        if step % write_frequency == 0:
            z_prev = z.copy()
    return dict(log=np.array(log, dtype=np.float64).reshape(-1, 6), newton_its=np.array(newton, dtype=np.int32),
                lvpp_its=np.array(lvpp, dtype=np.int32), z=z, z_prev=z_prev, max_conform=np.array(max_conform))


def logs_agree(a, b):
    """The comparison rule of the recorded runs: successful attempts agree on (step, k, alpha, its, reason); failed attempts
    only on (step, k, alpha) and on the fact of failure (the iteration count inside a failing attempt is not reproducible)."""
    a, b = np.asarray(a, float).reshape(-1, 6), np.asarray(b, float).reshape(-1, 6)
    if a.shape != b.shape:
        return False
    fa, fb = np.isnan(a[:, 5]), np.isnan(b[:, 5])
    if not np.array_equal(fa, fb) or not np.array_equal(a[:, :3], b[:, :3]):
        return False
    return bool(np.array_equal(a[~fa, 3:5], b[~fb, 3:5]))


def field_differences(nv, za, zb):
    """max-norm differences of the (u, c, psi) blocks of two states; psi relative to max |psi| of the second"""
    d = [float(np.abs(za[k * nv:(k + 1) * nv] - zb[k * nv:(k + 1) * nv]).max()) for k in range(3)]
    d[2] /= max(float(np.abs(zb[2 * nv:]).max()), 1e-300)
    return np.array(d)


def field_tolerances(golden):
    """what a rerun of a recorded run may differ by, per field: max(1e-10, 10 x the recorded sensitivity); the factor 10 covers
    a linear solver that orders its elimination differently from splu"""
    return np.maximum(1e-10, 10.0 * np.asarray(golden["sensitivity"], dtype=np.float64))
