"""numpy / scipy restatement of the two self-contained comparison solvers of example 05 (the reference's
examples/05_obstacle_type_qvi/solver_comparison/thermoforming_moreau_yosida.jl, "MY", and thermoforming_fixed_point.jl, "FP")
for the tests of the HIP family pgx_qmy (include/pgx_qmy.h).

Test infrastructure only: the product path is libpgx.so.  Statement by statement it restates

* the penalised residual (MY:77-81) and its generalised Jacobian (MY:84-88) in the layout x = [u | T], nv entries each, with
  nodal (interpolated) data Phi0, phi and a constant load (MY:40-44), Dirichlet rows F = x with zeroed columns, and the
  active-field mask of pgx_qmy_set_active (a frozen field: identity rows, zero residual, zero columns);
* the two functionals of the gamma update (MY:97-98), both update formulas (MY:99-119 with its guards, FP:75-85 without) and
  the H1 "Cauchy" norm on the free dofs of u (MY:92-94,144-145);
* NLsolve's `newton` with LineSearches.BackTracking(c_1=-1e8) by the rules the shared driver ships (mx_newton_nls of
  csrc/pgx_mixed.hip; recalled from upstream, not checked against NLsolve's source), solving with scipy's splu or, to
  measure how far the linear solver moves a run, with a dense numpy.linalg.solve;
* the loops MY:121-157 and FP:87-146.

Quadrature: one rule for every integral, the 36-point collapsed Gauss-Jacobi rule of degree 11 (Measure(Omega, 11), MY:37;
which rule Gridap takes is not pinned).  Meshes: the right-diagonal triangulation of the unit square; Gridap's `simplexify`
is not pinned either.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.special import roots_jacobi

XTOL = 10 * np.finfo(np.float64).eps  # MY:130
C1 = -1.0e8


def quadrature_gj(degree=11):
    """collapsed Gauss-Jacobi rule on the reference triangle, (degree // 2 + 1)^2 points, weights sum to 1/2"""
    n = degree // 2 + 1
    (x0, w0), (x1, w1) = roots_jacobi(n, 0.0, 0.0), roots_jacobi(n, 1.0, 0.0)
    a, c = 0.5 * (x1 + 1.0), 0.5 * (x0 + 1.0)
    A, Cc = np.meshgrid(a, c, indexing="ij")
    W = (w1 / 4.0)[:, None] * (w0 / 2.0)[None, :]
    return np.stack([(Cc * (1 - A)).ravel(), A.ravel()], axis=1), W.ravel()


def unit_square(M):
    """right-diagonal triangulation, vertex v = j (M + 1) + i; returns coords, cells, boundary vertices"""
    xs = np.linspace(0.0, 1.0, M + 1)
    X, Y = np.meshgrid(xs, xs, indexing="xy")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="xy")
    v0 = (j * (M + 1) + i).ravel()
    v1, v2 = v0 + 1, v0 + M + 1
    v3 = v2 + 1
    cells = np.empty((2 * M * M, 3), dtype=np.int64)
    cells[0::2] = np.stack([v0, v1, v3], axis=1)
    cells[1::2] = np.stack([v0, v2, v3], axis=1)
    I, Jj = np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing="xy")
    on = ((I == 0) | (I == M) | (Jj == 0) | (Jj == M)).ravel()
    return coords, cells, np.flatnonzero(on)


def update_gamma_fixed_point(gamma, k, infeasibility, functional):
    """FP:75-85, no guards, IEEE arithmetic"""
    with np.errstate(all="ignore"):
        gamma, I, E0 = np.float64(gamma), np.float64(infeasibility), np.float64(functional)
        E = gamma * I / E0
        theta = E0 + I
        C2 = E * (E + gamma) * theta / gamma
        C1k = C2 / E
        return float(C2 / ((np.float64(1.0) / k) * abs(C1k - theta)) - E)


def update_gamma_moreau_yosida(gamma, k, infeasibility, functional):
    """MY:99-119: `functional ≈ 0` (no absolute tolerance: an exact zero) and a non-finite or non-positive value keep gamma"""
    if functional == 0:
        return gamma
    g = update_gamma_fixed_point(gamma, k, infeasibility, functional)
    return g if np.isfinite(g) and g > 0 else gamma


class PenalisedThermoforming:
    def __init__(self, coords, cells, bc, q=0.01, f=25.0, degree=11):
        self.coords, self.cells = np.asarray(coords, float), np.asarray(cells, np.int64)
        self.nv, self.nc = len(self.coords), len(self.cells)
        self.ntot = 2 * self.nv
        self.q, self.f = float(q), float(f)
        self.bc = np.asarray(bc, np.int64)
        self.free_u = np.ones(self.nv, bool)
        self.free_u[self.bc] = False
        pts, self.w = quadrature_gj(degree)
        self.N = np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1)  # (nq, 3)
        X = self.coords[self.cells]  # (nc, 3, 2)
        Jm = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]], axis=2)  # columns: edge vectors
        det = Jm[:, 0, 0] * Jm[:, 1, 1] - Jm[:, 0, 1] * Jm[:, 1, 0]
        inv = np.linalg.inv(Jm)
        gref = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]])
        self.G = np.einsum("ak,ckd->cad", gref, inv)  # physical gradients (nc, 3, 2)
        self.adet = np.abs(det)
        x = self.coords
        self.Phi0 = 1.0 - 2.0 * np.maximum(np.abs(x[:, 0] - 0.5), np.abs(x[:, 1] - 0.5))  # MY:40, interpolated
        self.phi = np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])  # MY:42, interpolated
        self.Ke = 0.5 * self.adet[:, None, None] * np.einsum("cad,cbd->cab", self.G, self.G)
        self.rows = np.repeat(self.cells, 3, axis=1).ravel()
        self.cols = np.tile(self.cells, (1, 3)).ravel()
        self.K = self._scalar(self.Ke)
        self.Mass = self._scalar(self._mass(np.ones((self.nc, len(self.w)))))
        fu = self.free_u.astype(float)
        self.H1 = sp.diags(fu) @ (self.K + self.Mass) @ sp.diags(fu)  # MY:92-94 on the free dofs

    # ---------------------------------------------------------------------------------------------------------------------
    def _scalar(self, Ae):
        return sp.coo_matrix((Ae.ravel(), (self.rows, self.cols)), shape=(self.nv, self.nv)).tocsr()

    def _mass(self, W):
        """element matrices of int W N_a N_b, W (nc, nq) given at the quadrature points"""
        return self.adet[:, None, None] * np.einsum("cq,qa,qb->cab", W * self.w[None, :], self.N, self.N)

    def _fields(self, x):
        u = np.where(self.free_u, x[: self.nv], 0.0)
        T = x[self.nv:]
        return u, T

    def _points(self, x):
        u, T = self._fields(x)
        uq, Tq = u[self.cells] @ self.N.T, T[self.cells] @ self.N.T
        Pq, pq = self.Phi0[self.cells] @ self.N.T, self.phi[self.cells] @ self.N.T
        return uq, Tq, pq, uq - (Pq + pq * Tq), Pq + pq * Tq - uq

    def margins(self, x):
        """(min |d|, min distance of s from {0, q}) over the quadrature points: how far x is from a kink"""
        _, _, _, d, s = self._points(x)
        return np.abs(d).min(), np.minimum(np.abs(s), np.abs(s - self.q)).min()

    def _active(self, mask):
        return np.concatenate([self.free_u & bool(mask & 1), np.full(self.nv, bool(mask & 2))])

    def g(self, s):  # MY:47-55
        return np.where(s <= 0, 1.0, np.where(s < self.q, 1.0 - s / self.q, 0.0))

    def dg(self, s):  # MY:56-64
        return np.where((s > 0) & (s < self.q), -1.0 / self.q, 0.0)

    def residual(self, x, gamma, mask=3):
        u, T = self._fields(x)
        uq, Tq, pq, d, s = self._points(x)
        wd = self.w[None, :] * self.adet[:, None]
        Ru = np.einsum("cab,cb->ca", self.Ke, u[self.cells]) + (wd * (gamma * np.maximum(0.0, d) - self.f)) @ self.N
        RT = np.einsum("cab,cb->ca", self.Ke, T[self.cells]) + (wd * (Tq - self.g(s))) @ self.N
        F = np.concatenate([np.bincount(self.cells.ravel(), Ru.ravel(), self.nv), np.bincount(self.cells.ravel(), RT.ravel(), self.nv)])
        F = np.where(self._active(mask), F, 0.0)
        if mask & 1:
            F[self.bc] = x[self.bc]
        return F

    def jacobian(self, x, gamma, mask=3):
        _, _, pq, d, s = self._points(x)
        chi, dgs = (d > 0).astype(float), self.dg(s)
        uu = self.K + gamma * self._scalar(self._mass(chi))
        uT = -gamma * self._scalar(self._mass(chi * pq))
        Tu = self._scalar(self._mass(dgs))
        TT = self.K + self.Mass - self._scalar(self._mass(dgs * pq))
        D = sp.diags(self._active(mask).astype(float))
        J = D @ sp.bmat([[uu, uT], [Tu, TT]], format="csr") @ D + sp.identity(self.ntot) - D
        return J.tocsr()

    def energy(self, x):  # MY:97
        u, _ = self._fields(x)
        uq = u[self.cells] @ self.N.T
        return 0.5 * u @ (self.K @ u) - self.f * np.sum(self.w[None, :] * self.adet[:, None] * uq)

    def penalty(self, x, gamma):  # MY:98
        d = self._points(x)[3]
        return np.sum(self.w[None, :] * self.adet[:, None] * 0.5 * gamma * np.maximum(0.0, d) ** 2)

    def cauchy(self, x, xprev):  # MY:144-145
        d = x[: self.nv] - xprev[: self.nv]
        return np.sqrt(max(d @ (self.H1 @ d), 0.0))

    # ---------------------------------------------------------------------------------------------------------------------
    def newton_nls(self, x, gamma, mask=3, ftol=1e-5, xtol=XTOL, max_it=1000, c1=C1, solver="splu", matrices=None):
        """the rules of mx_newton_nls (csrc/pgx_mixed.hip).  Returns (x, iterations, reason): 1 ftol, 2 xtol, 0 max_it, -4 no
        finite trial.  `matrices`: a list that receives every (J, rhs) handed to the linear solver."""
        x = np.array(x, float)
        F = self.residual(x, gamma, mask)
        if np.abs(F).max() <= ftol:
            return x, 0, 1
        it = 0
        while True:
            if it >= max_it:
                return x, it, 0
            J = self.jacobian(x, gamma, mask)
            if matrices is not None:
                matrices.append((J.copy(), -F))
            delta = np.linalg.solve(J.toarray(), -F) if solver == "dense" else spla.splu(J.tocsc()).solve(-F)
            slope = F @ (J @ delta)
            f0, lam = 0.5 * F @ F, 1.0
            for halvings in range(51):
                with np.errstate(all="ignore"):
                    xt = x + lam * delta
                    Ft = self.residual(xt, gamma, mask)
                    ok = bool(np.all(np.isfinite(Ft)))
                    if (ok and not 0.5 * Ft @ Ft > f0 + c1 * lam * slope) or halvings == 50:
                        break
                lam *= 0.5
            if not ok:
                return x, it, -4
            x, F = xt, Ft
            it += 1
            if np.abs(F).max() <= ftol:
                return x, it, 1
            if lam * np.abs(delta).max() <= xtol:
                return x, it, 2

    def initial_state(self):
        return np.concatenate([np.zeros(self.nv), np.ones(self.nv)])  # MY:122-124

    def solve_moreau_yosida(self, gamma0=1.0, tol=1e-5, max_outer=100, ftol=1e-5, max_newton=1000, solver="splu", matrices=None):
        """MY:121-157"""
        x = self.initial_state()
        xprev = x.copy()
        gamma = float(gamma0)
        out = {"gammas": [], "newton_its": [], "reasons": [], "cauchy": []}
        for j in range(1, max_outer + 1):
            x, its, reason = self.newton_nls(x, gamma, 3, ftol, max_it=max_newton, solver=solver, matrices=matrices)
            if reason < 0:  # where NLsolve would throw: the loop ends, the counts so far stand
                break
            out["gammas"].append(gamma), out["newton_its"].append(its), out["reasons"].append(reason)
            out["cauchy"].append(self.cauchy(x, xprev))
            xprev = x.copy()
            gamma = update_gamma_moreau_yosida(gamma, j + 1, self.penalty(x, gamma), self.energy(x))
            if out["cauchy"][-1] < tol:
                break
        out["x"] = x
        return out

    def solve_fixed_point(self, tol=1e-5, max_outer=10_000, gamma_max=1e11, ftol_u=1e-5, ftol_T=1e-10, max_newton=1000,
                          max_inner=100, solver="splu", matrices=None):
        """FP:87-146"""
        x = self.initial_state()
        u_outer = x[: self.nv].copy()
        out = {"newton_its_T": [], "inner_steps": [], "newton_its_u": [], "inner_gammas": [], "reasons_u": [], "cauchy": []}
        for j in range(1, max_outer + 1):
            x, n_T, _ = self.newton_nls(x, 1.0, 2, ftol_T, max_it=max_newton, solver=solver, matrices=matrices)
            out["newton_its_T"].append(n_T)
            gamma, xprev, stopped = 1.0, x.copy(), False
            step_its, step_gammas, step_reasons = [], [], []
            for k in range(1, max_inner + 1):
                x, n_u, reason = self.newton_nls(x, gamma, 1, ftol_u, max_it=max_newton, solver=solver, matrices=matrices)
                if reason < 0:  # where NLsolve would throw: both loops end, the counts so far stand
                    stopped = True
                    break
                step_its.append(n_u), step_gammas.append(gamma), step_reasons.append(reason)
                c = self.cauchy(x, xprev)
                xprev = x.copy()
                if c < tol:
                    break
                gamma = update_gamma_fixed_point(gamma, k + 1, self.penalty(x, gamma), self.energy(x))
                if gamma > gamma_max:
                    break
                if not np.isfinite(gamma) or gamma <= 0:  # the next solve! would start from a non-finite residual
                    stopped = True
                    break
            out["newton_its_u"].append(step_its), out["inner_steps"].append(len(step_its))
            out["inner_gammas"].append(step_gammas), out["reasons_u"].append(step_reasons)
            if stopped:
                break
            d = np.concatenate([u_outer, x[self.nv:]])
            out["cauchy"].append(self.cauchy(x, d))
            u_outer = x[: self.nv].copy()
            if out["cauchy"][-1] < tol:
                break
        out["x"] = x
        return out


def problem(M, q=0.01, f=25.0):
    coords, cells, bc = unit_square(M)
    return PenalisedThermoforming(coords, cells, bc, q=q, f=f)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def run_spread(a, b):
    """how far two runs of the same loop differ: (largest relative gamma difference, relative L2 difference of final u, of final T)"""
    ga, gb = np.array(a["gammas"] if "gammas" in a else sum(a["inner_gammas"], [])), np.array(b["gammas"] if "gammas" in b else sum(b["inner_gammas"], []))
    nv = len(a["x"]) // 2
    dg = float(np.max(np.abs(ga - gb) / np.abs(gb))) if ga.shape == gb.shape else np.inf
    return dg, rel(a["x"][:nv], b["x"][:nv]), rel(a["x"][nv:], b["x"][nv:])


# Spread of the twin against itself, splu against numpy.linalg.solve, measured once on the CPU with run_spread (largest relative
# gamma difference, relative L2 difference of the final u, of the final T).  The GPU tests allow ten times these and never more
# than the 1e-9 of example 05's LVPP run test.
MEASURED_SPREAD = {
    ("moreau_yosida", 8): (1.8156452408187976e-12, 2.689811519596992e-15, 7.068197385509393e-15),   # max_outer = 10
    ("moreau_yosida", 16): (3.850132340380569e-12, 2.1659079905391317e-15, 5.391585351488194e-15),  # max_outer = 10
    ("fixed_point", 8): (7.137468005234818e-13, 1.3518182916045557e-16, 9.020016970638352e-16),     # max_outer = 3, gamma_max = 1e7
}


def tolerances(kind, M):
    return tuple(min(10.0 * s, 1e-9) for s in MEASURED_SPREAD[(kind, M)])
