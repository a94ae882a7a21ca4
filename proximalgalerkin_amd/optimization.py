"""Comparison solvers of example 01 on the GPU.

The reference compares proximal Galerkin with three OTHER solvers of the same discrete obstacle problem
    min  1/2 u^T S u - f^T M u     subject to   lower <= u <= upper          (S, M: P1 stiffness / mass matrices)
- Galahad TRB (trust-region, bound constraints) and IPOPT through /root/reference/src/lvpp/optimization.py:13-179 with the problem
object of examples/01_obstacle_problem/obstacle_ipopt_galahad.py:44-127, and PETSc's semismooth VI Newton
(obstacle_snes.py:36-115, `snes_type vinewtonssls` + setVariableBounds) - and prints an iteration-count table
(compare_all.py:170-182).  Those packages are external optimisers; here their role is played by three solvers written for this
repository whose linear algebra - every Newton system - is the nested-dissection sparse LU on the GPU (include/pgx_nd.h):

    trb_solver(problem, x_init, bounds, ...)     projected Newton with Armijo search along the projection arc (Bertsekas 1982):
                                                 the bound-constrained second-order method in the slot of `galahad_solver`
    vi_newton_solver(S, b, lower, upper, ...)    primal-dual active set = semismooth Newton on the NCP function
                                                 lambda - max(0, lambda - c (u - lower)) (Hintermueller, Ito, Kunisch 2002): the
                                                 VI Newton method in the slot of `vinewtonssls`
    interior_point_solver(problem, x_init, bounds, ...)   Mehrotra's primal-dual predictor-corrector method for a convex quadratic
                                                 under simple bounds, the whole iteration on the device (include/pgx_ipm.h): the
                                                 interior-point method in the slot of `ipopt_solver` with the exact, constant
                                                 Hessian (src/lvpp/optimization.py:115-166), reached through
                                                 `ipopt_solver(..., method="interior_point")`

`OptimizationProblem` keeps the reference's protocol (objective / gradient / pure_hessian / hessianstructure), so a problem object
written for lvpp.optimization works unchanged; `galahad_solver` is kept as an alias of `trb_solver` with the reference's signature.
`ipopt_solver` keeps the reference's call; by default (`method="projected_newton"`) it runs `trb_solver` - projected Newton, or
projected gradient without the Hessian - and with `method="interior_point"` the interior-point solver.
Problem callbacks are host numpy/scipy exactly as in the reference; the factorisations and triangular solves run on the GPU and
fail loudly without one.  `trb_solver` and `vi_newton_solver` do their vector work in host numpy between the GPU solves; the
interior-point iteration keeps every vector on the device.  CPU twins for the parity tests: oracle/compare_oracle.py and
tests/interior_point_reference.py.
"""
from __future__ import annotations

import ctypes as C
import typing

import numpy as np
import scipy.sparse as sp

from . import _lib as L
from .direct import DirectSolver

__all__ = ["OptimizationProblem", "ObstacleProblem", "trb_solver", "galahad_solver", "ipopt_solver", "vi_newton_solver",
           "interior_point_solver", "InteriorPointSolver", "setup_problem"]


class OptimizationProblem(typing.Protocol):
    """lvpp.optimization.OptimizationProblem (src/lvpp/optimization.py:13-36)."""
    total_iteration_count: int

    def objective(self, x): ...

    def gradient(self, x): ...

    def pure_hessian(self, x): ...

    def hessian(self, x, lagrange, obj_factor):
        return obj_factor * self.pure_hessian(x)

    def hessianstructure(self): ...


class ObstacleProblem:
    """obstacle_ipopt_galahad.py:94-127: quadratic energy 1/2 x^T S x - f^T M x with the lower-triangular Hessian in coordinate form."""
    total_iteration_count: int = 0

    def __init__(self, S, M, f):
        S = sp.csr_matrix(S, copy=True)
        S.eliminate_zeros()
        self._S, self._M = S, sp.csr_matrix(M)
        self._f = np.asarray(f, dtype=np.float64)
        self._Mf = self._M @ self._f
        tri = sp.tril(self._S).tocoo()
        self._sparsity = (tri.row.astype(np.int32), tri.col.astype(np.int32))
        self._H_data = tri.data

    def objective(self, x):
        return 0.5 * x @ (self._S @ x) - self._f @ (self._M @ x)

    def gradient(self, x):
        return self._S @ x - self._Mf

    def pure_hessian(self, x):
        return self._H_data

    def hessian(self, x, lagrange, obj_factor):
        return obj_factor * self.pure_hessian(x)

    def hessianstructure(self):
        return self._sparsity

    def intermediate(self, *args):
        self.total_iteration_count = args[1]


def setup_problem(mesh, phi=None, device: int = 0):
    """obstacle_ipopt_galahad.setup_problem (:44-91) for a Mesh: P1 stiffness and mass matrices assembled by the HIP kernels of
    include/pgx.h (the K and M value streams of the shared CSR pattern), f = 0, bounds = (interpolated obstacle, +inf) with the
    Dirichlet dofs pinned to 0 in both.  Returns (S, M, f, (lower, upper), vertex coordinates)."""
    from .obstacle import phi_set, setup_problem as _setup

    problem, sol, sol_k, alpha = _setup(mesh, 1, device=device)
    rowptr, col, K, M, _ = problem.export_blocks(with_D=False)
    problem.close()
    n = mesh.num_vertices
    S = sp.csr_matrix((K, col.copy(), rowptr.copy()), shape=(n, n))  # separate index arrays: eliminate_zeros() works in place
    Mm = sp.csr_matrix((M, col.copy(), rowptr.copy()), shape=(n, n))
    lower = np.asarray((phi or phi_set)(mesh.geometry.T.copy()), dtype=np.float64).copy()
    upper = np.full(n, np.inf)
    bc = mesh.exterior_vertices()
    lower[bc] = 0.0
    upper[bc] = 0.0
    return S, Mm, np.zeros(n), (lower, upper), mesh.geometry


class _MaskedLU:
    """GPU sparse LU of  P_F A P_F + P_B  (rows / columns of the bound set B replaced by the identity) on a fixed pattern."""

    def __init__(self, A: sp.csr_matrix, coords, device=0):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.A = A
        n = A.shape[0]
        self.rows = np.repeat(np.arange(n), np.diff(A.indptr))
        self.diag = self.rows == A.indices
        self.lu = DirectSolver(A.indptr, A.indices, np.arange(n, dtype=np.int32), coords, device=device)
        # Hessians / stiffness matrices with rows AND columns of the bound set replaced by the identity: symmetric whenever A is
        if abs(A - A.T).max() <= 1e-12 * abs(A).max():
            self.lu.set_symmetric(True)

    def factor(self, bound: np.ndarray):
        keep = ~(bound[self.rows] | bound[self.A.indices])
        self.lu.factor(np.where(keep, self.A.data, 0.0) + (self.diag & bound[self.rows]))

    def solve(self, b):
        x = self.lu.solve(b)
        return x

    def close(self):
        self.lu.close()


def _coords_for(problem, coords, n):
    if coords is not None:
        return np.asarray(coords, dtype=np.float64)
    # no geometry given: a 1-D embedding by index still yields a valid (if poorer) dissection ordering
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)


def _hessian_csr(problem, x, n):
    r, c = problem.hessianstructure()
    v = problem.pure_hessian(x)
    L = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    return (L + sp.tril(L, -1).T).tocsr()


def trb_solver(problem: OptimizationProblem, x_init, bounds, log_level: int = 0, use_hessian: bool = True, max_iter: int = 100,
               tol: float = 1e-6, coords=None, device: int = 0):
    """Bound-constrained minimisation in the slot of lvpp.optimization.galahad_solver (same arguments, same return value
    (x, iterations)): projected Newton - at x, bound variables whose gradient pushes outward are held, the Newton system of the
    others is solved by the GPU sparse LU, and an Armijo search runs along the PROJECTED path P(x + t d).  Stops when the
    projected gradient |P(x - g) - x| <= tol * max(1, |P(x0 - g0) - x0|) (Galahad's stop_pg_relative).  use_hessian=False:
    projected gradient steps (first-order model)."""
    lo, up = (np.asarray(b, dtype=np.float64) for b in bounds)
    x = np.clip(np.asarray(x_init, dtype=np.float64), lo, up)
    n = len(x)
    assert len(lo) == len(up) == n, "Bounds and x_init must have the same length"
    proj = lambda z: np.minimum(np.maximum(z, lo), up)  # noqa: E731
    H = _hessian_csr(problem, x, n)
    lu = _MaskedLU(H, _coords_for(problem, coords, n), device=device) if use_hessian else None
    g = problem.gradient(x)
    pg0 = np.linalg.norm(proj(x - g) - x)
    it = 0
    try:
        for it in range(1, max_iter + 1):
            pg = np.linalg.norm(proj(x - g) - x)
            if log_level:
                print(f"  trb {it - 1:3d}  f = {problem.objective(x):.12e}  |projected gradient| = {pg:.3e}")
            if pg <= tol * max(1.0, pg0):
                it -= 1
                break
            eps = min(1e-8, pg)
            bound = ((x <= lo + eps) & (g > 0.0)) | ((x >= up - eps) & (g < 0.0)) | (lo == up)
            if use_hessian:
                lu.factor(bound)
                d = lu.solve(np.where(bound, 0.0, -g))
                d[bound] = 0.0
            else:
                d = np.where(bound, 0.0, -g)
            f0 = problem.objective(x)
            t = 1.0
            for _ in range(60):
                xn = proj(x + t * d)
                if problem.objective(xn) <= f0 + 1e-4 * (g @ (xn - x)):
                    break
                t *= 0.5
            x = xn
            g = problem.gradient(x)
    finally:
        if lu is not None:
            lu.close()
    problem.total_iteration_count = it
    return x, it


def galahad_solver(problem, x_init, bounds, log_level: int = 1, use_hessian: bool = True, max_iter: int = 100, tol: float = 1e-6,
                   **kw):
    """Drop-in for lvpp.optimization.galahad_solver (src/lvpp/optimization.py:42-96): same call, solved by `trb_solver`."""
    return trb_solver(problem, x_init, bounds, log_level=max(log_level - 1, 0), use_hessian=use_hessian, max_iter=max_iter, tol=tol,
                      **kw)


class InteriorPointSolver:
    """Host mirror of include/pgx_ipm.h: minimise 1/2 x^T H x - b^T x subject to lo <= x <= up by Mehrotra's predictor-corrector
    method on the GPU.  H: the full symmetric matrix (scipy sparse, every diagonal entry stored); coords [n][2 or 3]: one point per
    dof for the nested dissection of the KKT matrices H + diag(z/s + w/t)."""

    HISTORY_COLUMNS = ("|r_d|_inf", "mu", "max complementarity", "sigma", "alpha_p", "alpha_d")
    PROFILE_COLUMNS = ("residual + reductions", "KKT fill", "factorisation", "solves", "step kernels")

    def __init__(self, H, coords, device: int = 0, data=None):
        self._lib = L.load()
        self._h = L._H()
        H = sp.csr_matrix(H)
        H.sort_indices()
        self.n = H.shape[0]
        self.indptr = np.ascontiguousarray(H.indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(H.indices, dtype=np.int32)
        self.data = np.ascontiguousarray(H.data if data is None else data, dtype=np.float64)
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        rc = self._lib.pgx_ipm_create(H.shape[0], H.shape[1], L.iptr(self.indptr), L.iptr(self.indices), L.dptr(self.data), len(self.data),
                                      int(coords.shape[1]), L.dptr(coords), int(device), C.byref(self._h))
        if rc:
            msg = self._lib.pgx_ipm_last_error(None)
            raise L.PgxError(f"pgx_ipm_create failed (code {rc}): {msg.decode() if msg else ''}")

    def _check(self, rc, what):
        if rc:
            msg = self._lib.pgx_ipm_last_error(self._h)
            raise L.PgxError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def _vec(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.n,)
        return a

    def set_problem(self, b, lo, up):
        b, lo, up = self._vec(b), self._vec(lo), self._vec(up)
        self._check(self._lib.pgx_ipm_set_problem(self._h, L.dptr(b), L.dptr(lo), L.dptr(up)), "pgx_ipm_set_problem")

    def solve(self, x_init, tol: float = 1e-6, max_iter: int = 100, monitor: bool = False) -> dict:
        """dict(x, z, w, iterations, converged, history): history has one row of HISTORY_COLUMNS per evaluation of the stop test."""
        x0 = self._vec(x_init)
        x, z, w = (np.empty(self.n) for _ in range(3))
        it, status = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.pgx_ipm_solve(self._h, L.dptr(x0), float(tol), int(max_iter), int(bool(monitor)), L.dptr(x), L.dptr(z), L.dptr(w),
                                            C.byref(it), C.byref(status)), "pgx_ipm_solve")
        return dict(x=x, z=z, w=w, iterations=it.value, converged=status.value == 0, history=self.history())

    def history(self) -> np.ndarray:
        m = C.c_int64(0)
        self._check(self._lib.pgx_ipm_history(self._h, C.byref(m), None), "pgx_ipm_history")
        rows = np.zeros((m.value, len(self.HISTORY_COLUMNS)))
        if m.value:
            self._check(self._lib.pgx_ipm_history(self._h, C.byref(m), L.dptr(rows)), "pgx_ipm_history")
        return rows

    def profile(self, enable: bool = True) -> dict:
        """Device milliseconds per phase of the solves since the last call, then switch the recording on or off."""
        ms = np.zeros(len(self.PROFILE_COLUMNS))
        self._check(self._lib.pgx_ipm_profile(self._h, int(bool(enable)), L.dptr(ms)), "pgx_ipm_profile")
        return dict(zip(self.PROFILE_COLUMNS, ms.tolist()))

    def eval(self, x, z, w):
        """(r_d, |r_d|_inf, mu, max complementarity) at (x, z, w) - the residual kernel alone."""
        x, z, w = self._vec(x), self._vec(z), self._vec(w)
        rd, sc = np.empty(self.n), np.zeros(3)
        self._check(self._lib.pgx_ipm_eval(self._h, L.dptr(x), L.dptr(z), L.dptr(w), L.dptr(rd), L.dptr(sc)), "pgx_ipm_eval")
        return rd, sc[0], sc[1], sc[2]

    def kkt_values(self, x, z, w) -> np.ndarray:
        """The values of K = P_F (H + diag(z/s + w/t)) P_F + P_fixed on H's pattern, as the factorisation receives them."""
        x, z, w = self._vec(x), self._vec(z), self._vec(w)
        vals = np.empty(len(self.data))
        self._check(self._lib.pgx_ipm_kkt_export(self._h, L.dptr(x), L.dptr(z), L.dptr(w), L.dptr(vals)), "pgx_ipm_kkt_export")
        return vals

    def close(self):
        if self._h:
            self._lib.pgx_ipm_destroy(self._h)
            self._h = L._H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def interior_point_solver(problem: OptimizationProblem, x_init, bounds, log_level: int = 0, max_iter: int = 100, tol: float = 1e-6,
                          coords=None, device: int = 0):
    """Bound-constrained minimisation of a QUADRATIC objective by a primal-dual interior-point method on the GPU
    (include/pgx_ipm.h), for the problem objects of lvpp.optimization: what the reference asks of IPOPT with
    `hessian_approximation exact`, `hessian_constant yes` and no general constraints (src/lvpp/optimization.py:115-166).  H comes
    from hessianstructure() / pure_hessian(x_init), b = -gradient(0); an objective whose gradient is not H x - b is refused.
    Stops when max(|H x - b - z + w|_inf, mu) <= tol * max(1, |H x_0 - b|_inf).  Returns (x, iterations)."""
    lo, up = (np.asarray(b, dtype=np.float64) for b in bounds)
    x_init = np.asarray(x_init, dtype=np.float64)
    n = len(x_init)
    assert len(lo) == len(up) == n, "Bounds and x_init must have the same length"
    H = _hessian_csr(problem, x_init, n)
    b = -np.asarray(problem.gradient(np.zeros(n)), dtype=np.float64)
    # one probe of `hessian_constant yes`: the gradient at x_init (or, for x_init = 0, at the vector of ones) is H x - b to rounding
    xp = x_init if np.any(x_init) else np.ones(n)
    Hx = H @ xp
    if not np.abs(np.asarray(problem.gradient(xp)) - (Hx - b)).max() <= 1e-10 * max(1.0, np.abs(Hx).max(), np.abs(b).max()):
        raise NotImplementedError("interior_point_solver takes objectives with a constant Hessian (gradient(x) = H x - b): this one's "
                                  "gradient is not affine in x")
    ipm = InteriorPointSolver(H, _coords_for(problem, coords, n), device=device)
    try:
        ipm.set_problem(b, lo, up)
        r = ipm.solve(x_init, tol=tol, max_iter=max_iter, monitor=bool(log_level))
    finally:
        ipm.close()
    problem.total_iteration_count = r["iterations"]
    return r["x"], r["iterations"]


def ipopt_solver(problem, x_init, bounds, log_level: int = 5, max_iter: int = 100, tol: float = 1e-6, activate_hessian: bool = True,
                 method: str = "projected_newton", **kw):
    """The call of lvpp.optimization.ipopt_solver (src/lvpp/optimization.py:115-166: same arguments, returns x only; the iteration
    count is left in `problem.total_iteration_count`, which is where the reference's callers read it, compare_all.py:100-108).
    method="projected_newton" (the default): the bound-constrained problem is solved by `trb_solver`: projected Newton with
    `activate_hessian`, projected gradient without - the first-order method the reference compares against is IPOPT with its
    limited-memory Hessian approximation.  method="interior_point": `interior_point_solver`, the interior-point method of the
    reference's `hessian_approximation exact` / `hessian_constant yes` branch; no limited-memory variant exists, so
    activate_hessian=False is refused."""
    if method == "interior_point":
        if not activate_hessian:
            raise NotImplementedError("ipopt_solver(method='interior_point') needs activate_hessian=True: no limited-memory "
                                      "interior-point variant is built")
        x, _ = interior_point_solver(problem, x_init, bounds, log_level=1 if log_level > 5 else 0, max_iter=max_iter, tol=tol, **kw)
        return x
    if method != "projected_newton":
        raise ValueError(f"ipopt_solver: unknown method {method!r} (projected_newton, interior_point)")
    x, _ = trb_solver(problem, x_init, bounds, log_level=1 if log_level > 5 else 0, use_hessian=activate_hessian, max_iter=max_iter,
                      tol=tol, **kw)
    return x


def vi_newton_solver(S, b, lower, upper=None, x_init=None, max_it: int = 1000, c: float = 1.0, coords=None, device: int = 0,
                     monitor: bool = False):
    """Variational inequality  u >= lower,  S u - b >= 0,  (u - lower)^T (S u - b) = 0  (+ fixed dofs where lower == upper) by the
    primal-dual active-set method = semismooth Newton.  Each step fixes u = lower on the active set, solves the reduced system
    by the GPU sparse LU and updates the set from lambda = S u - b; it stops when the set repeats (the iterate then solves the
    VI exactly).  Returns (u, iterations) like obstacle_snes.snes_solve's (u, snes.getIterationNumber())."""
    S = sp.csr_matrix(S)
    n = S.shape[0]
    lower = np.asarray(lower, dtype=np.float64)
    upper = np.full(n, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
    fixed = lower == upper
    u = np.clip(np.zeros(n) if x_init is None else np.asarray(x_init, dtype=np.float64), lower, upper)
    lam = np.zeros(n)
    lu = _MaskedLU(S, _coords_for(None, coords, n), device=device)
    active_prev = None
    it = 0
    try:
        for it in range(1, max_it + 1):
            active = ((lam - c * (u - lower) > 0.0) | fixed)
            if active_prev is not None and np.array_equal(active, active_prev):
                it -= 1
                break
            ua = np.where(active, lower, 0.0)
            lu.factor(active)
            rhs = np.where(active, lower, b - S @ ua)
            u = lu.solve(rhs)
            u[active] = lower[active]
            lam = np.where(active & ~fixed, S @ u - b, 0.0)
            if monitor:
                print(f"  vi {it:3d}  active {int(active.sum()) - int(fixed.sum()):7d}  min(u - lower) = {(u - lower).min():.3e}  "
                      f"min(lambda) = {lam.min():.3e}")
            active_prev = active
    finally:
        lu.close()
    return u, it
