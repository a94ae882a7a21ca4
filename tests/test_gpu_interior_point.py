"""The interior-point solver on the GPU (include/pgx_ipm.h, proximalgalerkin_amd/csrc/pgx_ipm.hip; slot of the reference's IPOPT
call, src/lvpp/optimization.py:115-166) against its numpy twin tests/interior_point_reference.py: the residual and KKT-fill kernels
at random interior points, full solves iterate for iterate, the KKT conditions of the GPU result itself, agreement with the VI solver,
bitwise repeatability, the `ipopt_solver(method="interior_point")` front door and the argument errors.

Problems: optimization.setup_problem on fem.create_rectangle(((-1,-1),(1,1)),(N,N)); case A = lower bounds only, b = 0; case B =
two-sided bounds, dofs without a bound, non-zero load (interior_point_reference.case_b_data)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import interior_point_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
# mu (relative) and the step lengths alpha_p, alpha_d (absolute; they lie in [0, 1]) of the GPU history against the twin's, over all
# rows of all solves below: 100 x the largest discrepancy measured on the MI355X (test_full_solve_matches_the_twin lists them), far
# inside the 1e-6 that may never be exceeded.  The solves are bitwise repeatable, so the measured values do not move from run to run.
MU_BAR = 100 * 4.18e-12
ALPHA_BAR = 100 * 1.28e-13
assert MU_BAR <= 1e-6 and ALPHA_BAR <= 1e-6


@functools.lru_cache(maxsize=None)
def _setup(N):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.optimization import setup_problem

    mesh = fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), (N, N))
    S, M, f, (lower, upper), coords = setup_problem(mesh)
    S = sp.csr_matrix(S)
    S.sort_indices()
    return S, sp.csr_matrix(M), lower, upper, np.ascontiguousarray(coords, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _case(name, N):
    S, M, lower, upper, coords = _setup(N)
    b, lo, up = R.case(name, S, M, lower, upper, coords)
    return S, b, lo, up, coords


@functools.lru_cache(maxsize=None)
def _twin(name, N):
    S, b, lo, up, _ = _case(name, N)
    return R.solve(S, b, lo, up, np.zeros(len(b)), tol=TOL)


def _gpu_solve(name, N):
    from proximalgalerkin_amd.optimization import InteriorPointSolver

    S, b, lo, up, coords = _case(name, N)
    ipm = InteriorPointSolver(S, coords)
    try:
        ipm.set_problem(b, lo, up)
        return ipm.solve(np.zeros(len(b)), tol=TOL)
    finally:
        ipm.close()


@functools.lru_cache(maxsize=None)
def _gpu(name, N):
    return _gpu_solve(name, N)


def _interior_point(lo, up, seed):
    """random x strictly inside the bounds (anywhere where there is none), z > 0 on L, w > 0 on U"""
    rng = np.random.default_rng(seed)
    fixed, L, U = R.masks(lo, up)
    n = len(lo)
    x = rng.standard_normal(n)
    only_l, only_u, both = L & ~U, U & ~L, L & U
    x[only_l] = lo[only_l] + rng.uniform(1e-3, 2.0, n)[only_l]
    x[only_u] = up[only_u] - rng.uniform(1e-3, 2.0, n)[only_u]
    x[both] = lo[both] + rng.uniform(0.01, 0.99, n)[both] * (up[both] - lo[both])
    x[fixed] = lo[fixed]
    z = np.where(L, 10.0 ** rng.uniform(-6, 2, n), 0.0)
    w = np.where(U, 10.0 ** rng.uniform(-6, 2, n), 0.0)
    return x, z, w


@pytest.mark.parametrize("N", [3, 8, 33])
def test_residual_and_kkt_kernels_match_the_twin(require_gpu, N):
    """pgx_ipm_eval / pgx_ipm_kkt_export, case B: 16 rows (less than a wave), 81, 1156 (several workgroups, no multiple of 64).
    r_d to 1e-12 of its largest entry (the measure of the other kernel tests: the entries are sums that cancel), every KKT value and
    the three scalars to relative 1e-12."""
    from proximalgalerkin_amd.optimization import InteriorPointSolver

    S, b, lo, up, coords = _case("B", N)
    fixed, L, U = R.masks(lo, up)
    assert fixed.any() and (L & U).any()
    if N >= 8:  # (N = 3 has four interior vertices, all with both bounds) every kind of dof: one bound only, no bound at all
        assert (L & ~U).any() and (U & ~L).any() and (~fixed & ~L & ~U).any()
    x, z, w = _interior_point(lo, up, 100 + N)
    ipm = InteriorPointSolver(S, coords)
    try:
        ipm.set_problem(b, lo, up)
        rd, rdn, mu, cmax = ipm.eval(x, z, w)
        K = ipm.kkt_values(x, z, w)
    finally:
        ipm.close()
    rd_r, rdn_r, mu_r, cmax_r = R.evaluate(S, b, lo, up, x, z, w)
    K_r = R.kkt_matrix(S, lo, up, x, z, w)
    assert np.array_equal(K_r.indices, S.indices) and len(K) == len(K_r.data)
    e_rd = np.abs(rd - rd_r).max() / np.abs(rd_r).max()
    e_K = (np.abs(K - K_r.data) / np.where(K_r.data == 0.0, 1.0, np.abs(K_r.data))).max()
    e_s = max(abs(rdn - rdn_r) / rdn_r, abs(mu - mu_r) / mu_r, abs(cmax - cmax_r) / cmax_r)
    print(f"N = {N}: r_d {e_rd:.2e}  KKT values {e_K:.2e}  scalars {e_s:.2e}")
    assert np.array_equal(rd[fixed], np.zeros(int(fixed.sum())))
    assert e_rd <= 1e-12 and e_K <= 1e-12 and e_s <= 1e-12


# the issue's four sizes, and the sizes whose iteration count rounding cannot move (interior_point_reference.COUNTING_CASES: at A/64,
# B/8 and B/48 the twin's last two iterates pass / fail the stop test by factors 88 | 6.1, 1.9 | 4.7 and 17 | 1.8 only - still five
# orders more than the discrepancy between the two paths measured below)
SOLVES = sorted(set([("A", 24), ("A", 64), ("B", 8), ("B", 48)] + R.COUNTING_CASES))


@pytest.mark.parametrize("name,N", SOLVES)
def test_full_solve_matches_the_twin(require_gpu, name, N):
    """Same iteration count, |x - x_twin| <= 1e-10 |x_twin| (the bar of tests/test_gpu_comparison_solvers.py), histories of equal
    length with mu within MU_BAR (relative) and the step lengths within ALPHA_BAR.  Measured on the MI355X:

        case/N   iterations   |x - x_twin|/|x_twin|   mu (relative)   alpha_p, alpha_d   sigma
        A/24      8            4.1e-16                 2.9e-12         8.9e-16            6.5e-16
        A/64      9            2.4e-16                 1.2e-13         1.7e-15            2.8e-15
        A/75      9            6.5e-15                 2.6e-12         2.7e-14            1.3e-14
        B/7       8            6.8e-17                 3.5e-14         2.2e-16            8.3e-16
        B/8      10            7.2e-17                 9.3e-14         2.7e-15            2.8e-15
        B/11      7            6.6e-17                 5.0e-13         4.4e-16            6.3e-17
        B/48     15            1.3e-15                 4.2e-12         1.3e-13            3.0e-13

    The final-x bar of 1e-10 is met with five orders to spare at every size."""
    g, t = _gpu(name, N), _twin(name, N)
    hg, ht = g["history"], t["history"]
    ex = np.linalg.norm(g["x"] - t["x"]) / np.linalg.norm(t["x"])
    print(f"case {name} N = {N}: iterations {g['iterations']} / {t['iterations']}  |x - x_twin| / |x_twin| = {ex:.2e}")
    assert g["converged"] and t["converged"]
    assert g["iterations"] == t["iterations"]
    assert hg.shape == ht.shape == (t["iterations"] + 1, 6)
    e_mu = (np.abs(hg[:, 1] - ht[:, 1]) / ht[:, 1]).max()
    e_a = np.abs(hg[:, 4:6] - ht[:, 4:6]).max()
    e_sigma = np.abs(hg[:, 3] - ht[:, 3]).max()
    print(f"case {name} N = {N}: history: mu {e_mu:.2e} (relative)  alpha_p, alpha_d {e_a:.2e}  sigma {e_sigma:.2e}")
    assert ex <= 1e-10
    assert e_mu <= MU_BAR and e_a <= ALPHA_BAR


@pytest.mark.parametrize("name,N", [("A", 64), ("B", 48)])
def test_gpu_result_satisfies_the_kkt_conditions(require_gpu, name, N):
    S, b, lo, up, _ = _case(name, N)
    g = _gpu(name, N)
    x, z, w = g["x"], g["z"], g["w"]
    fixed, L, U = R.masks(lo, up)
    x0, _, _ = R.start(np.zeros(len(b)), lo, up)
    scale = max(1.0, np.abs((S @ x0 - b)[~fixed]).max())
    assert np.all(x[L] > lo[L]) and np.all(x[U] < up[U])
    assert z.min() >= 0.0 and w.min() >= 0.0 and not z[~L].any() and not w[~U].any()
    assert np.abs((S @ x - b - z + w)[~fixed]).max() <= TOL * scale
    assert np.array_equal(x[fixed], lo[fixed])


def test_agrees_with_the_vi_newton_solver(require_gpu):
    """Case A, N = 64: an interior-point answer against the active-set answer, within the bar the CPU test established for the twin
    (interior_point_reference.GAP_BAR; measured for the twin at this size: 6.0e-07)."""
    from proximalgalerkin_amd.optimization import vi_newton_solver

    S, b, lo, up, coords = _case("A", 64)
    u, _ = vi_newton_solver(S, b, lo, up, coords=coords)
    gap = np.abs(_gpu("A", 64)["x"] - u).max()
    print(f"|x_ipm - u_vi|_inf = {gap:.3e}")
    assert gap <= R.GAP_BAR


def test_two_solves_are_bitwise_equal(require_gpu):
    a, b = _gpu("B", 48), _gpu_solve("B", 48)
    assert a["iterations"] == b["iterations"]
    for k in ("x", "z", "w", "history"):
        assert np.array_equal(a[k], b[k]), k


def test_front_door(require_gpu):
    from proximalgalerkin_amd.optimization import ObstacleProblem, galahad_solver, interior_point_solver, ipopt_solver

    S, M, lower, upper, coords = _setup(24)
    f = np.zeros(S.shape[0])
    problem = ObstacleProblem(S, M, f)
    x0 = np.zeros(len(f))
    xi, it = interior_point_solver(problem, x0, (lower, upper), tol=TOL, coords=coords)
    assert problem.total_iteration_count == it == _twin("A", 24)["iterations"]
    problem.total_iteration_count = -1
    x = ipopt_solver(problem, x0, (lower, upper), log_level=0, tol=TOL, method="interior_point", coords=coords)
    assert isinstance(x, np.ndarray) and np.array_equal(x, xi) and problem.total_iteration_count == it
    # the default method is what it was
    xd = ipopt_solver(problem, x0, (lower, upper), log_level=0, tol=TOL, coords=coords)
    xg, itg = galahad_solver(problem, x0, (lower, upper), log_level=0, tol=TOL, coords=coords)
    assert np.array_equal(xd, xg) and problem.total_iteration_count == itg
    with pytest.raises(NotImplementedError, match="limited-memory"):
        ipopt_solver(problem, x0, (lower, upper), log_level=0, method="interior_point", activate_hessian=False)

    class Quartic(ObstacleProblem):
        def gradient(self, x):
            return super().gradient(x) + x**3

    with pytest.raises(NotImplementedError, match="constant Hessian"):
        ipopt_solver(Quartic(S, M, f), x0, (lower, upper), log_level=0, method="interior_point", coords=coords)


def test_argument_errors_are_reported_before_the_device_is_used(require_gpu):
    from proximalgalerkin_amd._lib import PgxError
    from proximalgalerkin_amd.optimization import InteriorPointSolver

    S, b, lo, up, coords = _case("B", 3)
    n = S.shape[0]
    ipm = InteriorPointSolver(S, coords)
    try:
        lo5, up5 = lo.copy(), up.copy()
        lo5[5], up5[5] = 0.0, -1.0
        with pytest.raises(PgxError, match=r"lo\[5\]"):
            ipm.set_problem(b, lo5, up5)
        with pytest.raises(PgxError, match="pgx_ipm_set_problem first"):
            ipm.solve(np.zeros(n))
        ipm.set_problem(b, lo, up)  # the handle is still good
        assert ipm.solve(np.zeros(n), tol=TOL)["converged"]
    finally:
        ipm.close()
    # a pattern without the diagonal entry of row 5
    C = S.tocoo()
    keep = ~((C.row == 5) & (C.col == 5))
    nodiag = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=S.shape)
    with pytest.raises(PgxError, match="row 5 .* no diagonal entry"):
        InteriorPointSolver(nodiag, coords)
    with pytest.raises(PgxError, match="Hessian values"):
        InteriorPointSolver(S, coords, data=S.data[:-1])
    with pytest.raises(PgxError, match="not square"):
        InteriorPointSolver(sp.csr_matrix(S[:, :-1]), coords)
