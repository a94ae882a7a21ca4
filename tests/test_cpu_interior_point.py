"""The numpy twin of the interior-point solver (tests/interior_point_reference.py; slot of the reference's IPOPT call,
src/lvpp/optimization.py:115-166) on its own: it converges, its result satisfies the KKT conditions of
min 1/2 x^T H x - b^T x, lo <= x <= up, and it agrees with the active-set / projected-Newton twins of oracle/compare_oracle.py.

Case A: the obstacle problem of optimization.setup_problem (lower bounds only, b = 0).  Case B: two-sided bounds, dofs without a
bound, non-zero load (interior_point_reference.case_b_data)."""
import functools

import numpy as np
import pytest

from oracle import compare_oracle as C
from tests import interior_point_reference as R

TOL = 1e-10
GAP_BAR = R.GAP_BAR


@functools.lru_cache(maxsize=None)
def solved(name, N):
    S, M, lower, upper, coords = R.oracle_problem(N)
    b, lo, up = R.case(name, S, M, lower, upper, coords)
    return S, b, lo, up, R.solve(S, b, lo, up, np.zeros(len(b)), tol=TOL)


CASES = [("A", 16), ("A", 24), ("B", 8), ("B", 24)]


@pytest.mark.parametrize("name,N", CASES)
def test_twin_converges_to_a_kkt_point(name, N):
    S, b, lo, up, r = solved(name, N)
    x, z, w = r["x"], r["z"], r["w"]
    fixed, L, U = R.masks(lo, up)
    assert r["converged"] and 3 <= r["iterations"] <= 20
    assert len(r["history"]) == r["iterations"] + 1
    assert np.all(x[L] > lo[L]) and np.all(x[U] < up[U]) and np.array_equal(x[fixed], lo[fixed])  # strictly inside
    assert z.min() >= 0.0 and w.min() >= 0.0 and not z[~L].any() and not w[~U].any()
    rd, rdn, mu, cmax = R.evaluate(S, b, lo, up, x, z, w)
    assert rdn <= TOL * r["scale"] and 0.0 <= mu <= TOL * r["scale"]
    assert np.abs((S @ x - b - z + w)[~fixed]).max() <= TOL * r["scale"]


@pytest.mark.parametrize("name,N", CASES)
def test_twin_agrees_with_the_active_set_twins(name, N):
    """Measured |x - x_ref|_inf: A/16 2.3e-15, A/24 1.2e-08 (primal_dual_active_set); B/8 2.2e-05, B/24 8.9e-05 (projected_newton
    at tol 1e-12).  Bar: 10 x the largest = 8.9e-04."""
    S, b, lo, up, r = solved(name, N)
    if name == "A":
        ref, _, _ = C.primal_dual_active_set(S, b, lo, up)
    else:
        ref, _ = C.projected_newton(S, b, lo, up, np.zeros(len(b)), tol=1e-12)
    gap = np.abs(r["x"] - ref).max()
    print(f"case {name} N = {N}: |x_ipm - x_ref|_inf = {gap:.3e}")
    assert gap <= GAP_BAR


def test_start_is_strictly_interior_for_every_kind_of_dof():
    lo = np.array([0.0, 0.0, -np.inf, -np.inf, 0.0, 0.0, 2.0])
    up = np.array([np.inf, np.inf, 1.0, np.inf, 1.0, 1.0, 2.0])
    x0 = np.array([-3.0, 5.0, 4.0, 7.0, 0.25, 1.0, 9.0])
    x, z, w = R.start(x0, lo, up)
    assert np.array_equal(x, [1.0, 5.0, 0.0, 7.0, 0.25, 0.5, 2.0])
    assert np.array_equal(z, [1, 1, 0, 0, 1, 1, 0]) and np.array_equal(w, [0, 0, 1, 0, 1, 1, 0])


def test_unconstrained_problem_is_one_newton_step():
    """no finite bound anywhere: mu = 0, the KKT matrix is H, the first step lands on H^{-1} b"""
    import scipy.sparse as sp

    n = 30
    H = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    b = np.linspace(-1.0, 2.0, n)
    r = R.solve(H, b, np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n), tol=1e-12)
    assert r["converged"] and r["iterations"] == 1
    assert np.abs(H @ r["x"] - b).max() <= 1e-12 * r["scale"]


@pytest.mark.parametrize("name,N", R.COUNTING_CASES)
def test_iteration_counts_of_the_counting_cases_are_not_borderline(name, N):
    """The (case, N) at which the GPU test pins the iteration count to the twin's by the margin rule: the last iterate passes the stop
    test by a factor 10 at least, the one before fails it by a factor 10 at least - a count that rounding cannot move.
    Measured (stop-test quantity / (tol scale), last | one before):  A/24 1.1e-02 | 2.8e+01,  A/75 5.5e-03 | 1.2e+01,
    B/7 4.7e-02 | 1.4e+01,  B/11 1.2e-02 | 9.7e+01."""
    S, b, lo, up, r = solved(name, N)
    h, ts = r["history"], TOL * r["scale"]
    last, before = max(h[-1, 0], h[-1, 1]) / ts, max(h[-2, 0], h[-2, 1]) / ts
    print(f"case {name} N = {N}: {r['iterations']} iterations, stop quantity / (tol scale): last {last:.2e}, one before {before:.2e}")
    assert r["converged"]
    assert last <= 0.1 and before >= 10.0
