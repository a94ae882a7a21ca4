"""Example 03 on the GPU (include/pgx_fr.h): the kernels against the numpy restatement tests/fracture_reference.py at random
states that violate the Dirichlet values, the state moves, full runs against the restatement's recorded runs
(tests/golden/fracture_p1_*.npz, tools/make_fracture_golden.py), the factorisation, determinism and the give-up branch.

Every bound is the issue's or follows from the recorded sensitivities (fracture_reference.field_tolerances); each test prints its
figures before it asserts.  DESIGN.md section 12c says which of the project's numbers for this example are measured."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import fracture
from proximalgalerkin_amd.mesh_generation import create_crack_mesh
from tests import fracture_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _pair(h):
    mesh, ft, names = create_crack_mesh(h)
    left = fracture.boundary_vertices(ft, "topleft", names)
    right = fracture.boundary_vertices(ft, "topright", names)
    return R.Fracture(mesh.geometry, mesh.cells, left, right), fracture.FractureProblem(mesh, left, right)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("psi_scale", [3.0, 800.0])
def test_kernels_match_restatement(require_gpu, psi_scale):
    # h = 0.2: 128 vertices, irregular valences, both Dirichlet lists, the notch, two blocks of cells
    P, prob = _pair(0.2)
    try:
        assert prob.l == P.l
        rng = np.random.default_rng(11)
        n = P.nv
        x = rng.standard_normal(P.ndofs)  # u violates the Dirichlet values
        x[2 * n:] = rng.uniform(-psi_scale, psi_scale, n)  # 800: exp(psi) overflows without the stable logistic
        z_iter = rng.standard_normal(P.ndofs)
        z_prev = rng.standard_normal(P.ndofs)
        z_prev[n:2 * n] = rng.random(n)  # c_prev in [0, 1]
        T = 0.37
        prob.set_state(x)
        prob.set_prev(z_iter)
        prob.set_zprev(z_prev)
        prob.set_load(T)
        assert np.array_equal(prob.get_zprev(), z_prev)
        for alpha in (3.7, 0.5):  # the second value recombines the iterate-independent blocks
            prob.set_alpha(alpha)
            F, fn = prob.residual()
            Fr = P.residual(x, z_iter, z_prev, alpha, T)
            print(f"psi {psi_scale} alpha {alpha}: residual {_rel(F, Fr):.2e} norm {abs(fn - np.linalg.norm(Fr)) / np.linalg.norm(Fr):.2e}")
            assert np.all(np.isfinite(F)) and np.isfinite(fn)
            assert _rel(F, Fr) <= 1e-12
            assert abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
            Jd = prob.jacobian()
            assert np.all(np.isfinite(Jd.data))
            J, Jr = Jd.toarray(), P.jacobian(x, z_prev, alpha).toarray()
            print(f"   jacobian {np.abs(J - Jr).max() / np.abs(Jr).max():.2e}")
            assert np.abs(J - Jr).max() <= 1e-12 * np.abs(Jr).max()
            # symmetric as assembled (the LU runs its L D L^T mode without a row flip): the two triangles hold the same sums of
            # the same products, at most in another order - a few units in the last place of the largest entry
            assert np.abs(J - J.T).max() <= 1e-14 * np.abs(J).max()
            v = rng.standard_normal(P.ndofs)
            y = prob.spmv(v)
            assert np.all(np.isfinite(y)) and _rel(y, Jr @ v) <= 1e-12
        # a residual at an explicit point, and a second load
        x2 = x + 0.1 * rng.standard_normal(P.ndofs)
        prob.set_load(-1.3)
        F2, _ = prob.residual(x2)
        assert _rel(F2, P.residual(x2, z_iter, z_prev, 0.5, -1.3)) <= 1e-12
        # the two norms and c_conform
        inc, dist = prob.l2_increment_c(), prob.l2_distance_zprev()
        assert abs(inc - P.l2_increment_c(x, z_iter)) <= 1e-12 * P.l2_increment_c(x, z_iter)
        assert abs(dist - P.l2_distance(x, z_prev)) <= 1e-12 * P.l2_distance(x, z_prev)
        cd, cr = prob.conforming_damage(), P.conforming_damage(x, z_prev)
        assert cd.shape == cr.shape == (P.nc, 10) and np.all(np.isfinite(cd))
        assert np.abs(cd - cr).max() <= 1e-12 * np.abs(cr).max()
        pts = rng.dirichlet(np.ones(3), size=7)[:, 1:]
        assert np.abs(prob.conforming_damage(pts) - P.conforming_damage(x, z_prev, pts)).max() <= 1e-12 * np.abs(cr).max()
    finally:
        prob.close()


def test_state_moves_are_exact_copies(require_gpu):
    P, prob = _pair(0.4)
    try:
        rng = np.random.default_rng(5)
        x, xk, zp = (rng.standard_normal(P.ndofs) for _ in range(3))
        prob.set_state(x)
        prob.set_prev(xk)
        prob.set_zprev(zp)
        prob.set_load(0.25)
        assert prob.T == 0.25
        F, _ = prob.residual()
        assert np.array_equal(F[P.bc], x[P.bc] - P.g_values(0.25))  # F[bc] = x_bc - g: the load reached the device
        prob.state_from_zprev()
        assert np.array_equal(prob.get_state(), zp) and np.array_equal(prob.get_zprev(), zp)
        assert prob.l2_distance_zprev() == 0.0
        prob.state_from_prev()
        assert np.array_equal(prob.get_state(), xk) and np.array_equal(prob.get_prev(), xk)
        assert prob.l2_increment_c() == 0.0
        prob.set_state(x)
        prob.zprev_from_state()
        assert np.array_equal(prob.get_zprev(), x) and np.array_equal(prob.get_state(), x) and np.array_equal(prob.get_prev(), xk)
        prob.advance_prev()
        assert np.array_equal(prob.get_prev(), x)
    finally:
        prob.close()


_runs = {}


def _golden_run(name, **kw):
    """one run of a recorded configuration through solve_problem, shared between the tests that read it"""
    g = np.load(GOLDEN / f"fracture_p1_{name}.npz")
    if name not in _runs:
        pivots = []
        _runs[name] = fracture.solve_problem(res=float(g["h"]), num_load_steps=int(g["num_load_steps"]), Tmin=float(g["Tmin"]),
                                             Tmax=float(g["Tmax"]), write_frequency=int(g["write_frequency"]), return_solution=True,
                                             monitor=lambda p, step, k: pivots.append(p.lu_stats()["perturbed_pivots"]), **kw) + (pivots,)  # after each attempt: its last factorisation
    return g, _runs[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_full_run_matches_recorded_run(require_gpu, name):
    g, (log, newton, lvpp, fields, _) = _golden_run(name)
    assert np.array_equal(fields["mesh"].cells, g["cells"]) and np.array_equal(fields["mesh"].geometry, g["coords"])
    assert R.logs_agree(log, g["log"]), (log[:, :5], g["log"][:, :5])
    assert np.array_equal(lvpp, g["lvpp_its"])
    ok = ~np.isnan(g["log"][:, 5])
    inc = np.abs(log[ok, 5] - g["log"][ok, 5]).max()
    z = np.concatenate([fields["u"], fields["c"], fields["psi"]])
    nv = len(fields["u"])
    d, dp = R.field_differences(nv, z, g["z"]), R.field_differences(nv, fields["z_prev"], g["z_prev"])
    tol = R.field_tolerances(g)
    print(f"golden {name}: (u, c, psi rel) state {d}, z_prev {dp}, tolerance {tol}, increments {inc:.2e}")
    assert np.all(d <= tol) and np.all(dp <= tol)


def test_factorisation_is_symmetric_without_perturbed_pivots(require_gpu):
    # perturbed_pivots is the count of the LAST completed factorisation.  The first factorisation of (A): one Newton step
    # (snes_max_it = 1) of its first attempt, from the zero state at its first load.
    g = np.load(GOLDEN / "fracture_p1_A.npz")
    mesh, ft, names = create_crack_mesh(float(g["h"]))
    prob = fracture.FractureProblem(mesh, fracture.boundary_vertices(ft, "topleft", names), fracture.boundary_vertices(ft, "topright", names),
                                    petsc_options=dict(fracture.SP, snes_max_it=1))
    try:
        prob.set_load(np.linspace(float(g["Tmin"]), float(g["Tmax"]), int(g["num_load_steps"]))[1])
        prob.set_alpha(1.0)
        reason, its = prob.solve()
        st = prob.lu_stats()
        assert its == 1 and st["perturbed_pivots"] == 0
        assert st["symmetric"] is True  # the L D L^T mode was honoured, not silently replaced by the general LU
    finally:
        prob.close()
    # the last factorisation of (A): the stats read after its last attempt (and after every other attempt: the last of each)
    _, (log, _, _, _, pivots) = _golden_run("A")
    assert len(pivots) == len(log)
    assert pivots[-1] == 0 and not any(pivots)


def test_determinism(require_gpu):
    g, (log, newton, lvpp, fields, _) = _golden_run("B")
    log2, newton2, lvpp2, fields2 = fracture.solve_problem(res=float(g["h"]), num_load_steps=int(g["num_load_steps"]), Tmin=float(g["Tmin"]),
                                                           Tmax=float(g["Tmax"]), write_frequency=int(g["write_frequency"]),
                                                           return_solution=True)
    assert np.array_equal(log, log2, equal_nan=True) and np.array_equal(newton, newton2) and np.array_equal(lvpp, lvpp2)
    for k in ("u", "c", "psi", "z_prev"):
        assert np.array_equal(fields[k], fields2[k])


def test_forced_failures_give_up(require_gpu):
    # (B)'s first two loads, at most 2 Newton steps per attempt: every attempt fails with MAX_IT, alpha is halved each time, and
    # after exactly nfail_max = 3 failures the run gives up with the state reset to z_prev
    sp = dict(fracture.SP, snes_max_it=2)
    log, newton, lvpp, fields = fracture.solve_problem(res=0.1, num_load_steps=3, Tmin=0.0, Tmax=0.4, nfail_max=3, write_frequency=1,
                                                       petsc_options=sp, return_solution=True)
    assert log.shape == (3, 6)
    assert np.array_equal(log[:, :5], [[0, 1, 1.0, 2, -5], [0, 1, 0.5, 2, -5], [0, 1, 0.25, 2, -5]])
    assert np.isnan(log[:, 5]).all()
    assert newton.tolist() == [6] and lvpp.tolist() == [0]
    z = np.concatenate([fields["u"], fields["c"], fields["psi"]])
    assert np.array_equal(z, fields["z_prev"]) and not z.any()


def test_example_script_writes_its_files(require_gpu, tmp_path):
    import runpy
    import sys

    script = pathlib.Path(__file__).resolve().parents[1] / "examples" / "03_fracture" / "fracture.py"
    argv = sys.argv
    sys.argv = [str(script), "--res", "0.2", "--num-load-steps", "4", "--Tmax", "0.3", "--write-frequency", "2", "--result_dir", str(tmp_path)]
    try:
        runpy.run_path(str(script), run_name="__main__")
    finally:
        sys.argv = argv
    a = np.load(tmp_path / "attempts.npz")
    assert a["newton_its"].shape == (3,) and np.all(a["newton_its"] > 0) and a["log"].shape[1] == 6
    for step in (0, 2):
        assert (tmp_path / f"solution_{step:06d}.vtu").exists() and (tmp_path / f"damage_{step:06d}.vtu").exists()
    assert not (tmp_path / "solution_000001.vtu").exists()
