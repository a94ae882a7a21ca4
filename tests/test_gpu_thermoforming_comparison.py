"""Example 05's comparison solvers on the GPU (include/pgx_qmy.h; Moreau-Yosida path following and the fixed point in T) against
their numpy twin tests/thermoforming_comparison_reference.py.

Kernels: 1e-12 relative, the project's kernel tolerance (test_gpu_thermoforming.py).  Runs: identical Newton counts; gamma and
the fields within ten times the spread the twin shows against itself when its splu is replaced by a dense numpy.linalg.solve,
capped at the 1e-9 of example 05's LVPP run test.  Measured on the CPU (thermoforming_comparison_reference.MEASURED_SPREAD):
    Moreau-Yosida M = 8,  10 outer steps: gamma 1.8e-12, u 2.7e-15, T 7.1e-15
    Moreau-Yosida M = 16, 10 outer steps: gamma 3.9e-12, u 2.2e-15, T 5.4e-15
    fixed point   M = 8,  3 outer steps, gamma_max = 1e7: gamma 7.1e-13, u 1.4e-16, T 9.0e-16
The fixed-point prefix contains no Newton solve above 20 iterations at gamma_max = 1e7 (longest: 5;
test_cpu_thermoforming_comparison.py::test_fixed_point_prefix_of_the_gpu_test_has_no_long_solve), so the issue's value stands."""
import functools

import numpy as np
import pytest

from tests import thermoforming_comparison_reference as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _twin(M, q=0.01):
    return R.problem(M, q=q)


@functools.lru_cache(maxsize=None)
def _twin_my(M):
    return _twin(M).solve_moreau_yosida(max_outer=10)


@functools.lru_cache(maxsize=None)
def _twin_fp():
    return _twin(8).solve_fixed_point(max_outer=3, gamma_max=1e7)


def _problem(M, q=0.01):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.thermoforming_comparison import PenalisedThermoformingProblem

    return PenalisedThermoformingProblem(fem.create_unit_square(M, M), q=q)


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * abs(b)


@pytest.mark.parametrize("q", [0.01, 0.5])
@pytest.mark.parametrize("M", [3, 10, 33])
def test_kernels_match_twin(require_gpu, M, q):
    problem, prob = _problem(M, q), _twin(M, q)
    assert problem.ndofs == prob.ntot
    n = prob.nv
    rng = np.random.default_rng(50 + M)
    x, xk, v = rng.standard_normal(prob.ntot), rng.standard_normal(prob.ntot), rng.standard_normal(prob.ntot)
    _, _, _, d, s = prob._points(x)
    mixed = ((d > 0).any(axis=1) & (d < 0).any(axis=1)).sum()
    band = ((s > 0) & (s < q)).sum()
    print(f"M {M} q {q}: {mixed} of {prob.nc} cells with both signs of d, {band} points in the band of g")
    assert mixed > 0 and (q < 0.5 or band > 0)
    for gamma in (1.0, 3.5e6):
        problem.set_gamma(gamma)
        for mask in (1, 2, 3):
            problem.set_active(mask)
            F, fn = problem.residual(x)
            Fr = prob.residual(x, gamma, mask)
            finf = problem.residual_inf(x)
            print(f"  gamma {gamma:g} mask {mask}: residual {R.rel(F, Fr):.1e}, inf-norm {abs(finf - abs(Fr).max()) / abs(Fr).max():.1e}")
            assert R.rel(F, Fr) < 1e-12 and _close(fn, np.linalg.norm(Fr)) and _close(finf, abs(Fr).max())
            J = problem.jacobian(x)
            Jr = prob.jacobian(x, gamma, mask)
            for blk in ((slice(0, n), slice(0, n)), (slice(0, n), slice(n, 2 * n)), (slice(n, 2 * n), slice(0, n)), (slice(n, 2 * n), slice(n, 2 * n))):
                assert abs(J[blk] - Jr[blk]).max() <= 1e-12 * abs(Jr[blk]).max()
            assert R.rel(problem.spmv(v), Jr @ v) < 1e-12
            F2, _ = problem.residual(x)
            J2 = problem.jacobian(x)
            assert np.array_equal(F, F2) and np.array_equal(J.data, J2.data) and problem.residual_inf(x) == finf  # bitwise
        problem.set_state(x)
        problem.set_prev(xk)
        e, p = problem.functionals()
        assert _close(e, prob.energy(x)) and _close(p, prob.penalty(x, gamma)) and (e, p) == problem.functionals()
    c = problem.cauchy()
    assert _close(c, prob.cauchy(x, xk)) and c == problem.cauchy()
    problem.close()


@pytest.mark.parametrize("M", [8, 16])
def test_moreau_yosida_prefix_matches_twin(require_gpu, M):
    from proximalgalerkin_amd.thermoforming_comparison import solve_moreau_yosida

    pivots = []
    out = solve_moreau_yosida(M, max_outer=10, verbose=False, return_solution=True,
                              monitor=lambda p, j: pivots.append(p.lu_stats()["perturbed_pivots"]))
    ref = _twin_my(M)
    tg, tu, tT = R.tolerances("moreau_yosida", M)
    dg, du, dT = R.run_spread(out, ref)
    print(f"M {M}: newton {out['newton_its']} twin {ref['newton_its']}; gamma {dg:.2e} (tol {tg:.1e}), u {du:.2e} (tol {tu:.1e}), T {dT:.2e} (tol {tT:.1e})")
    assert out["newton_its"] == ref["newton_its"] and out["reasons"] == ref["reasons"]
    assert pivots == [0] * 10
    assert dg <= tg and du <= tu and dT <= tT


def test_fixed_point_prefix_matches_twin(require_gpu):
    from proximalgalerkin_amd.thermoforming_comparison import solve_fixed_point

    out = solve_fixed_point(8, max_outer=3, gamma_max=1e7, verbose=False, return_solution=True)
    ref = _twin_fp()
    tg, tu, tT = R.tolerances("fixed_point", 8)
    dg, du, dT = R.run_spread(out, ref)
    print(f"T {out['newton_its_T']} inner {out['inner_steps']} u {out['newton_its_u']}; gamma {dg:.2e} (tol {tg:.1e}), u {du:.2e} (tol {tu:.1e}), T {dT:.2e} (tol {tT:.1e})")
    assert out["inner_steps"] == ref["inner_steps"]
    assert out["newton_its_T"] == ref["newton_its_T"] and out["newton_its_u"] == ref["newton_its_u"]
    assert dg <= tg and du <= tu and dT <= tT


def test_newton_driver_rules(require_gpu):
    problem, prob = _problem(8), _twin(8)
    x0 = prob.initial_state()
    problem.set_gamma(1.0)
    problem.set_state(x0)
    assert problem.solve(max_it=2)[:2] == (0, 2)  # the cap is reason 0, not an error ...
    x2 = problem.get_state()
    x2r, its, reason = prob.newton_nls(x0, 1.0, max_it=2)
    assert (its, reason) == (2, 0) and R.rel(x2, x2r) < 1e-9 and R.rel(x2, x0) > 1e-3  # ... and the iterate of step 2 stays
    reason, its, _ = problem.solve()
    assert reason == 1 and its + 2 == prob.newton_nls(x0, 1.0)[1]
    assert problem.residual_inf() <= 1e-5
    assert problem.solve()[:2] == (1, 0)  # a start within ftol: no iteration
    problem.close()
