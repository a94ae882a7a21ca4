"""Example 07 on the GPU (include/pgx_ev.h): the kernels against the numpy restatement tests/eigenvalue_reference.py at random
states that violate the Dirichlet values, the state moves, full runs against the restatement's recorded runs
(tests/golden/eigenvalue_*.npz, tools/make_eigenvalue_golden.py), the factorisation, determinism and the halving / give-up
branches.

Every bound is the issue's or follows from the recorded sensitivities (eigenvalue_reference.field_tolerances); each test prints its
figures before it asserts.  DESIGN.md section 12d says which of the project's numbers for this example are measured."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import eigenvalue, fem
from tests import eigenvalue_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _pair(Nx, Ny, p, nq, A=1.0, C=4.0, d=0.25, **kw):
    mesh = fem.QuadMesh(((0.0, 0.0), (1.0, 1.0)), (Nx, Ny))
    return R.Eigenvalue(Nx, Ny, p, nq, A=A, C=C, d=d), eigenvalue.EigenvalueProblem(mesh, p, 2 * (nq - 1), A=A, C_=C, d=d, **kw)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# 3 x 2 cells, Q3, 11 points: unequal counts (an x / y transposition shows), 6 cells are no multiple of the 4 cells per workgroup, two
#   rounds of lanes over the 121 points and three over the 136 node pairs;
# 3 x 3 cells, Q2, 5 points: a cell without boundary dof, an odd point count; 2 x 2 cells, Q1, 3 points
@pytest.mark.parametrize("mesh", [(3, 2, 3, 11), (3, 3, 2, 5), (2, 2, 1, 3)])
@pytest.mark.parametrize("psi_scale", [3.0, 800.0])
def test_kernels_match_restatement(require_gpu, mesh, psi_scale):
    P, prob = _pair(*mesh)
    try:
        rng = np.random.default_rng(11)
        n = P.n
        assert prob.ndofs == P.ndofs and np.array_equal(prob.cell_dofs, P.cd)
        x = rng.standard_normal(P.ndofs)  # q violates the Dirichlet values
        x[2 * n:] = rng.uniform(-psi_scale, psi_scale, 2 * n)  # 800: the script's expm overflows
        z_iter = rng.standard_normal(P.ndofs)
        prob.set_state(x)
        prob.set_prev(z_iter)
        for alpha in (3.7, 0.5):  # the second value recombines the iterate-independent blocks
            prob.set_alpha(alpha)
            F, fn = prob.residual()
            Fr = P.residual(x, z_iter, alpha)
            print(f"{mesh} psi {psi_scale} alpha {alpha}: residual {_rel(F, Fr):.2e} norm {abs(fn - np.linalg.norm(Fr)) / np.linalg.norm(Fr):.2e}")
            assert np.all(np.isfinite(F)) and np.isfinite(fn)
            assert _rel(F, Fr) <= 1e-12
            assert abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
            Jd = prob.jacobian()
            assert np.all(np.isfinite(Jd.data))
            J, Jr = Jd.toarray(), P.jacobian(x, alpha).toarray()
            print(f"   jacobian {np.abs(J - Jr).max() / np.abs(Jr).max():.2e}")
            assert np.abs(J - Jr).max() <= 1e-12 * np.abs(Jr).max()
            assert np.array_equal(J, J.T)  # symmetric to the last bit: both triangles receive the same sums in the same order
            v = rng.standard_normal(P.ndofs)
            y = prob.spmv(v)
            assert np.all(np.isfinite(y)) and _rel(y, Jr @ v) <= 1e-12
        # a residual at an explicit point
        x2 = x + 0.1 * rng.standard_normal(P.ndofs)
        F2, _ = prob.residual(x2)
        assert _rel(F2, P.residual(x2, z_iter, 0.5)) <= 1e-12
        # the norm of the increment and the nodal post-processing
        inc, incr = prob.l2_increment_Q(), P.l2_increment_Q(x, z_iter)
        print(f"   increment {abs(inc - incr) / incr:.2e}")
        assert abs(inc - incr) <= 1e-12 * incr
        nd, nr = prob.eval_nodes(), P.eval_nodes(x)
        assert nd.shape == nr.shape == (4, n) and np.all(np.isfinite(nd))
        assert np.abs(nd - nr).max() <= 1e-12 * np.abs(nr).max()
        # |T| = tanh(r / 2) <= 1; the two rounded products g psi_i and the hypot add a few units in the last place
        assert np.hypot(nd[0], nd[1]).max() <= 1.0 + 4 * np.finfo(float).eps and np.array_equal(nd[2], -nd[3])
    finally:
        prob.close()


def test_state_moves_are_exact_copies(require_gpu):
    P, prob = _pair(3, 2, 3, 11)
    try:
        rng = np.random.default_rng(5)
        x, xk = rng.standard_normal(P.ndofs), rng.standard_normal(P.ndofs)
        prob.set_state(x)
        prob.set_prev(xk)
        assert np.array_equal(prob.get_state(), x) and np.array_equal(prob.get_prev(), xk)
        F, _ = prob.residual()
        assert np.array_equal(F[P.bc], x[P.bc] - np.concatenate([prob.g1, prob.g2]))  # F[bc] = x_bc - g
        assert np.abs(np.concatenate([prob.g1, prob.g2]) - P.g).max() <= 1e-15
        prob.state_from_prev()
        assert np.array_equal(prob.get_state(), xk) and np.array_equal(prob.get_prev(), xk)
        assert prob.l2_increment_Q() == 0.0
        prob.set_state(x)
        prob.advance_prev()
        assert np.array_equal(prob.get_prev(), x) and np.array_equal(prob.get_state(), x)
        prob.set_state(np.zeros(P.ndofs))
        assert not prob.get_state().any() and np.array_equal(prob.get_prev(), x)
    finally:
        prob.close()


_runs = {}


def _params(g):
    return dict(N=int(g["N"]), degree=int(g["p"]), quadrature_degree=int(g["quadrature_degree"]), A=float(g["A"]), C=float(g["C"]),
                d=float(g["d"]))


def _state(fields):
    return np.concatenate([fields[k] for k in ("q1", "q2", "psi1", "psi2")])


def _golden_run(name):
    """one run of a recorded configuration through solve_problem, shared between the tests that read it"""
    g = np.load(GOLDEN / f"eigenvalue_{name}.npz")
    if name not in _runs:
        pivots = []
        _runs[name] = eigenvalue.solve_problem(monitor=lambda p, k: pivots.append(p.lu_stats()["perturbed_pivots"]), **_params(g)) + (pivots,)
    return g, _runs[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_full_run_matches_recorded_run(require_gpu, name):
    g, (fields, log, newton, _) = _golden_run(name)
    assert R.logs_agree(log, g["log"]), (log, g["log"])
    assert np.array_equal(newton, g["newton_its"])
    n = len(fields["q1"])
    d = R.field_differences(n, _state(fields), g["z"])
    tol = R.field_tolerances(g)
    print(f"golden {name}: (q1, q2, psi1 rel, psi2 rel) {d}, tolerance {tol}")
    assert np.all(d <= tol)
    nr = R.conforming(g["z"][2 * n:3 * n], g["z"][3 * n:])
    assert np.abs(fields["conforming1"] - nr[0]).max() <= 1e-10 and np.abs(fields["conforming2"] - nr[1]).max() <= 1e-10
    assert abs(fields["m_plus"].max() - float(g["max_q"])) <= tol[0] + tol[1]


def test_factorisation_is_symmetric_without_perturbed_pivots(require_gpu):
    # perturbed_pivots is the count of the LAST completed factorisation.  The first factorisation of (B): one Newton step
    # (snes_max_it = 1) of its first attempt, from the zero state.
    g = np.load(GOLDEN / "eigenvalue_B.npz")
    kw = _params(g)
    mesh = fem.create_unit_square(kw["N"], kw["N"], cell_type="quadrilateral")
    prob = eigenvalue.EigenvalueProblem(mesh, kw["degree"], kw["quadrature_degree"], A=kw["A"], C_=kw["C"], d=kw["d"],
                                        petsc_options=dict(eigenvalue.SP, snes_max_it=1))
    try:
        prob.set_alpha(1.0)
        reason, its = prob.solve()
        st = prob.lu_stats()
        assert its == 1 and st["perturbed_pivots"] == 0
        assert st["symmetric"] is True  # the L D L^T mode was honoured, not silently replaced by the general LU
    finally:
        prob.close()
    # the last factorisation of (B): the stats read after its last attempt (and after every other attempt: the last of each)
    _, (_, log, _, pivots) = _golden_run("B")
    assert len(pivots) == len(log)
    assert pivots[-1] == 0 and not any(pivots)


def test_determinism(require_gpu):
    g, (fields, log, newton, _) = _golden_run("B")
    fields2, log2, newton2 = eigenvalue.solve_problem(**_params(g))
    assert np.array_equal(log, log2) and np.array_equal(newton, newton2)
    for k in fields:
        assert np.array_equal(fields[k], fields2[k]), k


def test_forced_failures_give_up_at_the_zero_state(require_gpu):
    # (B) with at most 2 Newton steps per attempt: its first step needs 3, so every attempt fails with MAX_IT at nlvpp = 0, alpha is
    # halved each time, the state goes back to the zero z_prev (:192-193), and after exactly nfail_max = 3 failures the run gives up
    g = np.load(GOLDEN / "eigenvalue_B.npz")
    fields, log, newton = eigenvalue.solve_problem(nfail_max=3, snes_opts=dict(eigenvalue.SP, snes_max_it=2), **_params(g))
    assert np.array_equal(log, [[0, 1.0, 2, -5, 1], [0, 0.5, 2, -5, 1], [0, 0.25, 2, -5, 1]])
    assert len(newton) == 0 and not _state(fields).any()
    assert not fields["conforming1"].any() and not fields["m_plus"].any()


def test_forced_failure_after_a_step_restores_the_previous_iterate(require_gpu):
    # (A): the first step as recorded, then one Newton step per attempt only: what the restatement does from there is what the
    # package must do; every failed attempt halves alpha and goes back to z_iter (:194-195), the state after the first step
    g = np.load(GOLDEN / "eigenvalue_A.npz")
    kw = _params(g)
    P = R.Eigenvalue(kw["N"], kw["N"], kw["degree"], kw["quadrature_degree"] // 2 + 1, A=kw["A"], C=kw["C"], d=kw["d"])
    z1, reason, its = P.newton_l2(np.zeros(P.ndofs), np.zeros(P.ndofs), 1.0)
    expected, alpha = [(0, 1.0, its, reason, 0)], 2.0 if its <= 4 else 1.0
    for _ in range(3):
        _, rsn, it1 = P.newton_l2(z1, z1, alpha, max_it=1)
        assert rsn < 0, "the restatement converges in one step here: choose another configuration"
        expected.append((1, alpha, it1, rsn, 1))
        alpha /= 2
    after_first = []

    def monitor(problem, nlvpp):
        if not after_first:
            after_first.append(problem.get_state())
            problem._opts.snes_max_it = 1

    fields, log, newton = eigenvalue.solve_problem(nfail_max=3, monitor=monitor, **kw)
    print(log)
    assert R.logs_agree(log, expected) and newton.tolist() == [its]
    assert np.array_equal(_state(fields), after_first[0])
    assert np.all(R.field_differences(P.n, after_first[0], z1) <= 1e-10)


def test_example_script_writes_its_files(require_gpu, tmp_path):
    import json
    import runpy
    import sys

    script = pathlib.Path(__file__).resolve().parents[1] / "examples" / "07_eigenvalue_constraints" / "eigenvalue_constraints.py"
    argv = sys.argv
    sys.argv = [str(script), "-N", "3", "--degree", "2", "--quadrature-degree", "8", "--result_dir", str(tmp_path),
                "--profile", str(tmp_path / "profile.json")]
    try:
        runpy.run_path(str(script), run_name="__main__")
    finally:
        sys.argv = argv
    a = np.load(tmp_path / "attempts.npz")
    assert a["log"].shape[1] == 5 and np.all(a["newton_its"] > 0)
    assert (tmp_path / "Q.vtu").exists()
    prof = json.loads((tmp_path / "profile.json").read_text())
    assert prof["unknowns"] == 4 * 49 and prof["newton_iterations"] == int(a["newton_its"].sum()) and prof["lu"]["symmetric"] is True
