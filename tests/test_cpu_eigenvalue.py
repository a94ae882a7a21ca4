"""Example 07 without a GPU: the conforming map of tests/eigenvalue_reference.py against the reference script's own expression, the
restatement's Jacobian against finite differences of its residual, the Dirichlet data and the recorded runs
(tests/golden/eigenvalue_*.npz, tools/make_eigenvalue_golden.py).

Needs mpmath beside numpy, scipy and pytest (the two tests of the conforming map evaluate the script's expression in 60-digit
arithmetic).  mpmath is a pure-Python package that every torch installation brings along as a dependency of sympy, and
tools/make_quadrature_tables.py uses it already; README.md lists it with the test dependencies."""
import pathlib

import numpy as np
import pytest

from tests import eigenvalue_reference as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _random_psi(rng, count, rmax):
    r, t = rng.uniform(0.0, rmax, count), rng.uniform(0.0, 2 * np.pi, count)
    return r * np.cos(t), r * np.sin(t)


def test_closed_form_is_the_scripts_expression():
    """Pins the factor 2 of the script's tanh (:31-33): with the true matrix tanh T would be half of this.  200 random psi with
    r <= 30, 1e-12 relative.  The reference is the script's expression evaluated term by term in 60-digit arithmetic: evaluated in
    doubles with scipy.linalg.expm the expression itself is only accurate to eps exp(r) (measured 3e-4 at r <= 30, see
    eigenvalue_reference.T_script), which says nothing about the closed form; that evaluation is compared where it is accurate."""
    import mpmath

    rng = np.random.default_rng(0)
    worst = worst_double = 0.0
    for p1, p2 in zip(*_random_psi(rng, 200, 30.0)):
        t1, t2 = R.conforming(p1, p2)
        s1, s2 = (float(v) for v in R.T_script_mp(p1, p2))
        worst = max(worst, np.hypot(t1 - s1, t2 - s2) / np.hypot(s1, s2))
        if np.hypot(p1, p2) <= 5.0:
            d1, d2 = R.T_script(p1, p2)
            worst_double = max(worst_double, np.hypot(t1 - d1, t2 - d2) / np.hypot(d1, d2))
    print(f"closed form vs the script's expression: {worst:.2e} (60 digits, r <= 30), {worst_double:.2e} (doubles, r <= 5)")
    assert worst <= 1e-12 and 0.0 < worst_double <= 1e-12
    assert abs(float(R.g_of_r(0.0)) - 0.5) == 0.0
    t1, _ = R.conforming(50.0, 0.0)
    assert 0.999 < t1 < 1.0 + 1e-15  # the eigenvalue bound is 1, not the 1/2 of the paper
    with mpmath.workdps(60):  # a diagonal Psi: the expression is the scalar tanh(psi1 / 2)
        assert mpmath.almosteq(R.T_script_mp(0.3, 0.0)[0], mpmath.tanh(mpmath.mpf(0.3) / 2), 1e-40)


def test_derivative_matches_finite_differences():
    """DT against central differences of the script's expression, 1e-12 relative, r <= 30.  A difference quotient in doubles cannot
    resolve 1e-12, so the differences are taken in 60-digit arithmetic with the step 1e-20 (truncation error 1e-40)."""
    import mpmath

    rng = np.random.default_rng(1)
    h = mpmath.mpf(10) ** -20
    worst = 0.0
    for p1, p2 in zip(*_random_psi(rng, 100, 30.0)):
        d11, d12, d22 = R.conforming_derivative(p1, p2)
        D = np.array([[d11, d12], [d12, d22]])
        num = np.empty((2, 2))
        with mpmath.workdps(60):
            for j, (e1, e2) in enumerate(((1, 0), (0, 1))):
                tp = R.T_script_mp(mpmath.mpf(p1) + h * e1, mpmath.mpf(p2) + h * e2)
                tm = R.T_script_mp(mpmath.mpf(p1) - h * e1, mpmath.mpf(p2) - h * e2)
                num[:, j] = [float((a - b) / (2 * h)) for a, b in zip(tp, tm)]
        worst = max(worst, np.abs(D - num).max() / np.abs(num).max())
    print(f"DT vs central differences of the script's expression: {worst:.2e}")
    assert worst <= 1e-12


def test_derivative_is_symmetric_positive_definite():
    # DT psi = (g + g' r) psi = d/dr (r g(r)) psi = 1/2 sech^2(r / 2) psi and DT t = g t for t orthogonal to psi
    rng = np.random.default_rng(2)
    p1, p2 = _random_psi(rng, 200, 30.0)
    r = np.hypot(p1, p2)
    d11, d12, d22 = R.conforming_derivative(p1, p2)
    radial = np.stack([d11 * p1 + d12 * p2, d12 * p1 + d22 * p2])
    exact = 0.5 / np.cosh(0.5 * r) ** 2 * np.stack([p1, p2])
    scale = np.hypot(d11, d22) * r
    assert (np.abs(radial - exact).max(axis=0) / scale).max() <= 1e-12
    tang = np.stack([d11 * (-p2) + d12 * p1, d12 * (-p2) + d22 * p1])
    exact_t = np.tanh(0.5 * r) / r * np.stack([-p2, p1])
    assert (np.abs(tang - exact_t).max(axis=0) / scale).max() <= 1e-12
    assert np.all(d11 * d22 - d12 * d12 > 0) and np.all(d11 + d22 > 0)


def test_small_r_branch_is_continuous():
    r0 = R.R_SMALL
    below, above = np.nextafter(r0, 0.0), r0
    for t in np.linspace(0.0, 2 * np.pi, 7):
        c, s = np.cos(t), np.sin(t)
        ta, tb = np.array(R.conforming(below * c, below * s)), np.array(R.conforming(above * c, above * s))
        assert np.abs(ta - tb).max() <= 1e-12 * np.abs(tb).max()
        da, db = np.array(R.conforming_derivative(below * c, below * s)), np.array(R.conforming_derivative(above * c, above * s))
        assert np.abs(da - db).max() <= 1e-12 * np.abs(db).max()
    # the series themselves against the closed forms evaluated in extended precision at the switch
    rl = np.longdouble(r0)
    g_ld = np.tanh(rl / 2) / rl
    assert abs(float(R.g_of_r(below)) - float(g_ld)) <= 1e-15
    assert abs(float(R.gp_over_r(below)) + 1.0 / 12.0) <= 1e-9


def test_finite_at_large_r():
    for p1, p2 in ((800.0, 0.0), (0.0, -800.0), (800.0, 800.0), (-565.7, 565.7)):
        t = np.array(R.conforming(p1, p2))
        dd = np.array(R.conforming_derivative(p1, p2))
        assert np.all(np.isfinite(t)) and np.all(np.isfinite(dd))
        assert abs(np.hypot(*t) - 1.0) <= 1e-15  # saturated: an eigenvalue at the bound 1


@pytest.mark.parametrize("case", [(3, 2, 3, 11, 1.0), (3, 3, 2, 5, -500.0), (2, 2, 1, 3, 1.0)])
def test_jacobian_is_the_derivative_of_the_residual(case):
    Nx, Ny, p, nq, A = case
    P = R.Eigenvalue(Nx, Ny, p, nq, A=A, d=1.0 / 3.0 if Nx == 3 else 0.5)
    rng = np.random.default_rng(4)
    x = rng.standard_normal(P.ndofs)
    x[2 * P.n:] *= 3.0
    z_iter = rng.standard_normal(P.ndofs)
    alpha = 3.7
    J = P.jacobian_raw(x, alpha)
    assert abs(J - J.T).max() <= 1e-13 * abs(J).max()
    v = rng.standard_normal(P.ndofs)
    h = 1e-6
    fd = (P.residual_raw(x + h * v, z_iter, alpha) - P.residual_raw(x - h * v, z_iter, alpha)) / (2 * h)
    err = np.linalg.norm(fd - J @ v) / np.linalg.norm(J @ v)
    print(f"{case}: |fd - J v| / |J v| = {err:.2e}")
    assert err <= 1e-7  # central difference: h^2 |F'''| + eps |F| / h
    Jbc = P.jacobian(x, alpha)
    assert abs(Jbc - Jbc.T).max() <= 1e-13 * abs(Jbc).max()
    # the Dirichlet contract: at a state that satisfies the data the lifted residual is the raw one off the bc rows
    xg = x.copy()
    xg[P.bc] = P.g
    F, Fr = P.residual(xg, z_iter, alpha), P.residual_raw(xg, z_iter, alpha)
    free = np.setdiff1d(np.arange(P.ndofs), P.bc)
    assert np.array_equal(F[free], Fr[free]) and not F[P.bc].any()


def test_boundary_interpolant_does_not_depend_on_the_node_family():
    t = np.linspace(0.0, 1.0, 41)

    def edge_interpolant(N, d, family, p=3):
        """the interpolant of g_xx along the bottom edge, sampled at 41 points per cell"""
        nodes = R.nodes_1d(p, family)
        V, _ = R.lagrange_1d(nodes, t)
        out = []
        for c in range(N):
            xs = (c + nodes) / N
            g, _ = R.boundary_data(xs, np.zeros_like(xs), d)
            out.append(V @ g)
        return np.concatenate(out)

    # the recorded runs' (N, d, p) and the script's d at two mesh sizes.  d = 0.5 makes the script's two ramp intervals overlap at
    # z = 1/2, where T(z) (:98-106) returns 2: nodal data that no family interpolates alike at degree 3 - that run has degree 2, where
    # both families are the one set of nodes 0, 1/2, 1
    for N, d, p in ((4, 0.25, 3), (6, 0.5, 2), (100, 0.06, 3), (50, 0.06, 3)):
        assert abs(d * N - round(d * N)) < 1e-12
        a, b = edge_interpolant(N, d, "equispaced", p), edge_interpolant(N, d, "gll", p)
        assert np.abs(a - b).max() <= 1e-14, (N, d)
    assert float(R.ramp(np.array([0.5]), 0.5)[0]) == 2.0
    # and it does where a ramp ends inside a cell: the check above is not vacuous
    a, b = edge_interpolant(4, 0.06, "equispaced"), edge_interpolant(4, 0.06, "gll")
    assert np.abs(a - b).max() > 1e-3
    # the package's data are the restatement's
    from proximalgalerkin_amd import eigenvalue

    x = np.linspace(0, 1, 13)
    for xx, yy in ((x, np.zeros_like(x)), (np.ones_like(x), x), (x, np.ones_like(x)), (np.zeros_like(x), x)):
        assert np.array_equal(np.array(eigenvalue.boundary_data(xx, yy, 0.25)), np.array(R.boundary_data(xx, yy, 0.25)))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_goldens_are_self_consistent(name):
    g = np.load(GOLDEN / f"eigenvalue_{name}.npz")
    p, N = int(g["p"]), int(g["N"])
    n = (p * N + 1) ** 2
    log = g["log"]
    assert g["z"].shape == (4 * n,) and log.shape[1] == 5 and np.all(np.isfinite(g["z"]))
    assert abs(float(g["d"]) * N - round(float(g["d"]) * N)) < 1e-12
    ok = log[:, 4] == 0
    assert np.array_equal(log[ok, 2], g["newton_its"]) and np.all(log[ok, 3] > 0) and np.all(log[ok, 2] > 0)
    assert np.array_equal(log[ok, 0], np.arange(ok.sum()))  # nlvpp counts the successful steps
    alpha = 1.0
    for k, a, its, reason, failed in log:  # the alpha schedule (:191, :219-222)
        assert a == alpha
        alpha = alpha / 2 if failed else alpha * 2 if its <= 4 else alpha / 2 if its >= 10 else alpha
    assert R.logs_agree(log, log) and np.all(g["sensitivity"] < 1e-9)
    q = np.hypot(g["z"][:n], g["z"][n:2 * n])
    assert q.max() == float(g["max_q"])
    assert {"A": abs(q.max() - 0.5) < 1e-12, "B": 0.5 < q.max() < 1.0, "C": q.max() > 1.0}[name]
    # the recorded state solves its last proximal step: a stationary point of the loop
    P = R.Eigenvalue(N, N, p, int(g["quadrature_degree"]) // 2 + 1, A=float(g["A"]), C=float(g["C"]), d=float(g["d"]))
    t1, t2 = R.conforming(g["z"][2 * n:3 * n], g["z"][3 * n:])
    assert np.hypot(t1, t2).max() < 1.0
    F = P.residual(g["z"], g["z"], log[-1, 1])
    F0 = P.residual(np.zeros(4 * n), np.zeros(4 * n), 1.0)
    print(f"golden {name}: |F(z; z_iter = z)| / |F(0)| = {np.linalg.norm(F) / np.linalg.norm(F0):.2e}")
    assert np.linalg.norm(F) <= 1e-6 * np.linalg.norm(F0)
