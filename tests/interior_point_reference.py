"""Numpy twin (scipy, SuperLU) of the interior-point solver of include/pgx_ipm.h / proximalgalerkin_amd/csrc/pgx_ipm.hip:
Mehrotra's predictor-corrector method for

    minimise 1/2 x^T H x - b^T x   subject to   lo <= x <= up,

H symmetric, positive definite on the free dofs; lo may hold -inf, up +inf, lo[i] == up[i] fixes dof i.  It stands in the slot of the
reference's IPOPT call (src/lvpp/optimization.py:115-166: `hessian_approximation exact`, `hessian_constant yes`, no general
constraints).  The HIP path follows this file statement by statement - same start, same stop test, one factorisation and two solves
per iteration, the same order of operations inside every formula - so the two agree iterate for iterate up to the rounding of the
linear solves and of the reductions.  TEST INFRASTRUCTURE ONLY.

`solve` returns a dict: x, z, w, iterations, converged, scale and `history`, one row per evaluation of the stop test,
(|r_d|_inf, mu, max complementarity, sigma, alpha_p, alpha_d); the row of the last evaluation - no step follows it - carries zeros in
its last three columns, so the history always has iterations + 1 rows.  `oracle_problem` and `case` build the two test problems from the P1
matrices of the CPU oracle."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def masks(lo, up):
    """(fixed, L, U): fixed dofs, non-fixed dofs with a finite lower bound, non-fixed dofs with a finite upper bound."""
    fixed = lo == up
    return fixed, ~fixed & np.isfinite(lo), ~fixed & np.isfinite(up)


def start(x_init, lo, up):
    fixed, L, U = masks(lo, up)
    x = np.array(x_init, dtype=np.float64)
    both, only_l, only_u = L & U, L & ~U, U & ~L
    x[only_l] = np.maximum(x[only_l], lo[only_l] + 1.0)
    x[only_u] = np.minimum(x[only_u], up[only_u] - 1.0)
    inside = both & (x > lo) & (x < up)
    mid = both & ~inside
    x[mid] = 0.5 * (lo[mid] + up[mid])
    x[fixed] = lo[fixed]
    return x, L.astype(np.float64), U.astype(np.float64)


def evaluate(H, b, lo, up, x, z, w):
    """r_d and the three scalars of the stop test at (x, z, w): (r_d, |r_d|_inf, mu, max complementarity)."""
    fixed, L, U = masks(lo, up)
    nc = int(L.sum()) + int(U.sum())
    s = np.where(L, x - lo, 1.0)
    t = np.where(U, up - x, 1.0)
    rd = np.where(fixed, 0.0, ((H @ x - b) - z) + w)
    sz, tw = np.where(L, s * z, 0.0), np.where(U, t * w, 0.0)
    mu = (sz.sum() + tw.sum()) / nc if nc else 0.0
    return rd, np.abs(rd).max(), mu, max(sz.max(), tw.max())


def kkt_matrix(H, lo, up, x, z, w):
    """K = P_F (H + diag D) P_F + P_fixed on H's pattern (CSR, sorted, explicit zeros kept), D = z/s on L + w/t on U."""
    H = sp.csr_matrix(H)
    fixed, L, U = masks(lo, up)
    n = H.shape[0]
    s = np.where(L, x - lo, 1.0)
    t = np.where(U, up - x, 1.0)
    D = np.where(L, z / s, 0.0) + np.where(U, w / t, 0.0)
    rows = np.repeat(np.arange(n), np.diff(H.indptr))
    diag = rows == H.indices
    masked = fixed[rows] | fixed[H.indices]
    vals = np.where(masked, diag.astype(np.float64), H.data + np.where(diag, D[rows], 0.0))
    return sp.csr_matrix((vals, H.indices.copy(), H.indptr.copy()), shape=(n, n))


def _targets_rhs(rd, fixed, L, U, s, t, cz, cw):
    return np.where(fixed, 0.0, (-rd + np.where(L, cz / s, 0.0)) - np.where(U, cw / t, 0.0))


def _boundary(L, U, s, t, z, w, dx, dz, dw):
    """largest steps in [0, 1] that keep s, t >= 0 (alpha_p) and z, w >= 0 (alpha_d)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ap = min(np.where(L & (dx < 0.0), -s / dx, np.inf).min(), np.where(U & (dx > 0.0), t / dx, np.inf).min())
        ad = min(np.where(L & (dz < 0.0), -z / dz, np.inf).min(), np.where(U & (dw < 0.0), -w / dw, np.inf).min())
    return min(1.0, ap), min(1.0, ad)


def solve(H, b, lo, up, x_init, tol=1e-6, max_iter=100, monitor=False):
    H = sp.csr_matrix(H)
    H.sort_indices()
    b, lo, up = (np.asarray(a, dtype=np.float64) for a in (b, lo, up))
    fixed, L, U = masks(lo, up)
    nc = int(L.sum()) + int(U.sum())
    x, z, w = start(x_init, lo, up)
    g0 = np.where(fixed, 0.0, H @ x - b)
    scale = max(1.0, np.abs(g0).max())
    hist = []
    converged = False
    it = 0
    while True:
        rd, rdn, mu, cmax = evaluate(H, b, lo, up, x, z, w)
        if monitor:
            print(f"  ipm {it:3d}  |r_d| = {rdn:.3e}  mu = {mu:.3e}  max s z = {cmax:.3e}")
        if max(rdn, mu) <= tol * scale:
            converged = True
        if converged or it >= max_iter:
            hist.append((rdn, mu, cmax, 0.0, 0.0, 0.0))
            break
        s = np.where(L, x - lo, 1.0)
        t = np.where(U, up - x, 1.0)
        lu = spla.splu(kkt_matrix(H, lo, up, x, z, w).tocsc())
        # predictor
        cz, cw = -(s * z), -(t * w)
        dxa = lu.solve(_targets_rhs(rd, fixed, L, U, s, t, cz, cw))
        dza = np.where(L, (cz - z * dxa) / s, 0.0)
        dwa = np.where(U, (cw + w * dxa) / t, 0.0)
        apa, ada = _boundary(L, U, s, t, z, w, dxa, dza, dwa)
        a = min(apa, ada)
        mu_aff = ((np.where(L, (s + a * dxa) * (z + a * dza), 0.0).sum() + np.where(U, (t - a * dxa) * (w + a * dwa), 0.0).sum()) / nc
                  if nc else 0.0)
        sigma = (mu_aff / mu) ** 3 if mu > 0.0 else 0.0
        # corrector
        sm = sigma * mu
        cz = (sm - s * z) - dxa * dza
        cw = (sm - t * w) + dxa * dwa
        dx = lu.solve(_targets_rhs(rd, fixed, L, U, s, t, cz, cw))
        dz = np.where(L, (cz - z * dx) / s, 0.0)
        dw = np.where(U, (cw + w * dx) / t, 0.0)
        ap, ad = _boundary(L, U, s, t, z, w, dx, dz, dw)
        alpha = min(1.0, max(0.995, 1.0 - mu) * min(ap, ad))
        hist.append((rdn, mu, cmax, sigma, ap, ad))
        x = np.where(fixed, x, x + alpha * dx)
        # floating point: alpha < alpha_p keeps s, t > 0 in exact arithmetic, but lo + s rounds to lo once s is below an ulp of lo
        # (iterates that overshoot the tolerance by many orders); such a dof is put on the first number inside the bound
        x = np.where(L & (x <= lo), np.nextafter(lo, np.inf), x)
        x = np.where(U & (x >= up), np.nextafter(up, -np.inf), x)
        z = z + alpha * dz
        w = w + alpha * dw
        it += 1
    return dict(x=x, z=z, w=w, iterations=it, converged=converged, scale=scale, history=np.array(hist))


# ------------------------------------------------------------------------------------------------------------------------------
# the two test problems: P1 obstacle problem of optimization.setup_problem on [-1, 1]^2, matrices from the CPU oracle (equal to the HIP
# assembly to 1e-13, tests/test_gpu_comparison_solvers.py)
# ------------------------------------------------------------------------------------------------------------------------------
def case_a_bounds(coords, lower, upper):
    """lower bounds only (the obstacle), b = 0"""
    return lower.copy(), upper.copy()


def case_b_data(M, coords, lower, upper):
    """two-sided bounds, dofs without a bound, non-zero load: up = max(0.3, lo + 0.05), lo = -inf where x < -0.5, up = +inf where
    y > 0.5, boundary dofs fixed at 0, b = M (4 sin 3x cos 2y)."""
    fixed = lower == upper
    X, Y = coords[:, 0], coords[:, 1]
    lo = lower.copy()
    up = np.maximum(0.3, lo + 0.05)
    lo[X < -0.5] = -np.inf
    up[Y > 0.5] = np.inf
    lo[fixed] = 0.0
    up[fixed] = 0.0
    b = M @ (4.0 * np.sin(3.0 * X) * np.cos(2.0 * Y))
    return b, lo, up


def oracle_problem(N):
    """(S, M, lower, upper, coords) of optimization.setup_problem without a GPU"""
    from oracle import pg_oracle as O

    coords, cells = O.create_rectangle(N, N)
    p = O.ObstacleP1(coords, cells, O.boundary_vertices_rectangle(N, N))
    lower = O.phi_set(coords.T.copy()).copy()
    upper = np.full(p.n, np.inf)
    lower[p.bc] = 0.0
    upper[p.bc] = 0.0
    return sp.csr_matrix(p.K), sp.csr_matrix(p.M), lower, upper, coords


# Distance between an interior-point answer and the active-set answer of the same problem: about sqrt(tol) at weakly active vertices.
# Largest |x_ipm - x_active_set|_inf measured for this twin at tol 1e-10 (tests/test_cpu_interior_point.py prints them):
# A/16 2.3e-15,  A/24 1.2e-08,  B/8 2.2e-05,  B/24 8.9e-05  (A/64, used by the GPU test, 6.0e-07).  The bar is ten times the largest.
GAP_BAR = 10 * 8.9e-5

# (case, N) whose iteration count rounding cannot move: at tol 1e-10 the last iterate passes the stop test by a factor >= 10 and the
# one before fails it by a factor >= 10 (tests/test_cpu_interior_point.py checks exactly that).  Such sizes are rare, because the method
# contracts the stop quantity by only one to two orders per iteration near the end: of the case-A sizes tried between 33 and 80 only
# 33, 35, 75 and 79 qualify, of the case-B sizes tried between 5 and 149 only 5, 7 and 11.
COUNTING_CASES = [("A", 24), ("A", 75), ("B", 7), ("B", 11)]


def case(name, S, M, lower, upper, coords):
    """(b, lo, up) of case "A" or "B" """
    if name == "A":
        lo, up = case_a_bounds(coords, lower, upper)
        return np.zeros(len(lo)), lo, up
    return case_b_data(M, np.asarray(coords)[:, :2], lower, upper)
