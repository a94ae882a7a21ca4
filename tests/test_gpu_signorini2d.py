"""Example 02 in the plane (pgx_sg_create_2d of include/pgx_sg.h: triangles P1 / P2, quadrilaterals Q1 / Q2) - HIP path vs the numpy twin
tests/signorini2d_reference.py, which tests/test_cpu_signorini2d.py checks on its own and proves convergent on every full run used
here.  Tolerances are those of tests/test_gpu_signorini.py: kernels 1e-12 relative; full LVPP runs: identical Newton counts per proximal
step, displacement <= 1e-10 relative L2."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from tests import signorini2d_reference as R

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _square(cell_type, degree, nx, ny, gap=0.0, disp=-0.25):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import signorini as G

    mesh = fem.create_unit_square(nx, ny, cell_type=cell_type)
    mt, bcs = G.native_tags(mesh)
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, gap, disp, degree=degree, bc_facets=mt.find(1))
    prob = R.unit_square(nx, ny, cell_type, degree, gap=gap, disp=disp)
    return mesh, mt, bcs, problem, prob


def _half_disk(degree, gap=0.01, disp=-0.1):
    from proximalgalerkin_amd import mesh_generation
    from proximalgalerkin_amd import signorini as G

    mesh, _, tags = mesh_generation.create_half_disk(**R.HALF_DISK)
    problem = G.SignoriniProblem(mesh, tags[2], None, 2.0e4, 0.3, gap, disp, degree=degree, bc_facets=tags[1])
    prob = R.from_triangles(mesh.geometry, mesh.cells, tags[2], tags[1], degree, gap=gap, disp=disp)
    return problem, prob


def _same_discretisation(problem, prob):
    assert problem.gdim == 2 and problem.ndofs == prob.ntot and problem.npsi == prob.npsi
    assert np.array_equal(problem.contact_vertices, prob.cverts)
    assert np.array_equal(problem.node_coords, prob.node_coords)


def _state(prob, seed):
    """the recipe of tests/test_gpu_signorini.py: psi spans -2 ... -400 |N(0,1)|, so exp underflows on part of the edge"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(prob.ntot) * 0.05
    x[2 * prob.nv:] = -np.abs(rng.standard_normal(prob.npsi)) * np.where(rng.random(prob.npsi) < 0.4, 400.0, 2.0)
    xk = rng.standard_normal(prob.ntot) * 0.05
    return rng, x, xk


def _check_kernels(problem, prob, seed):
    _same_discretisation(problem, prob)
    rng, x, xk = _state(prob, seed)
    nu = 2 * prob.nv
    for alpha in (2.0, 64.0):
        problem.set_alpha(alpha)
        problem.set_prev(xk)
        F, fn = problem.residual(x)
        Fr = prob.residual(x, xk, alpha)
        assert _rel(F, Fr) < 1e-12 and abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
        J = problem.jacobian(x)
        Jr = prob.jacobian(x, alpha).tocsr()
        assert J.shape == Jr.shape and abs(J - Jr).max() <= 1e-12 * abs(Jr).max()
        assert abs(J[nu:, nu:] - Jr[nu:, nu:]).max() <= 1e-12 * abs(Jr[nu:, nu:]).max()  # D(psi) on its own scale
        assert abs(J[nu:, :nu] - Jr[nu:, :nu]).max() <= 1e-12 * abs(Jr[nu:, :nu]).max()  # -M_G on its own scale
        assert abs(J[:nu, nu:] - Jr[:nu, nu:]).max() <= 1e-12 * abs(Jr[:nu, nu:]).max()  # +M_G^T, Dirichlet rows masked
        v = rng.standard_normal(prob.ntot)
        assert _rel(problem.spmv(v), Jr @ v) < 1e-12
        F2, _ = problem.residual(x)
        assert np.array_equal(F, F2)  # atomic-free assembly: bitwise reproducible
    problem.set_state(x)
    problem.set_prev(xk)
    assert abs(problem.u_increment() - np.linalg.norm((x - xk)[:nu])) <= 1e-12 * np.linalg.norm((x - xk)[:nu])


@pytest.mark.parametrize("n", [(1, 1), (3, 2), (5, 4)])
@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
def test_kernels_match_twin(require_gpu, cell_type, degree, n):
    _, _, _, problem, prob = _square(cell_type, degree, *n, gap=0.01)
    _check_kernels(problem, prob, 31)
    problem.close()


@pytest.mark.parametrize("degree", [1, 2])
def test_kernels_on_the_half_disk_match_twin(require_gpu, degree):
    """the contact arc's end nodes are Dirichlet nodes as well: the coupling columns / rows of those u_y dofs are masked"""
    problem, prob = _half_disk(degree)
    assert len(np.intersect1d(prob.cverts, prob.bc_nodes)) == 2
    _check_kernels(problem, prob, 32)
    problem.close()


@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
def test_diagnostics_match_twin(require_gpu, cell_type, degree):
    _, _, _, problem, prob = _square(cell_type, degree, 5, 4, gap=0.01)
    _, x, _ = _state(prob, 33)
    problem.set_state(x)
    viol = problem.violation()
    ref = prob.violation(x)
    on = prob.cverts
    assert (ref[on] > 1e-3).any() and (ref[on] < -1e-3).any()  # both signs of u.n_g - g on the contact edge
    assert abs(viol - ref).max() <= 1e-12 * abs(ref).max()
    pen, pen_ref = problem.penetration(), prob.penetration(x)
    assert pen_ref > 0.0 and abs(pen - pen_ref) <= 1e-12 * pen_ref
    assert problem.penetration() == pen  # fixed-shape reduction: bitwise reproducible
    vm, vm_ref = problem.von_mises(), prob.von_mises(x)
    assert vm.shape == vm_ref.shape and abs(vm - vm_ref).max() <= 1e-12 * abs(vm_ref).max()
    st = problem.lu_stats()
    assert st["n_fronts"] >= 1 and st["factor_nnz"] > 0 and st["symmetric"] is True
    problem.close()


@pytest.mark.parametrize("nx,ny,gap", R.SQUARE_RUNS)
@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
def test_full_lvpp_run_matches_twin(require_gpu, cell_type, degree, nx, ny, gap):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import signorini as G

    mesh = fem.create_unit_square(nx, ny, cell_type=cell_type)
    mt, bcs = G.native_tags(mesh)
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, bcs, degree=degree, gap=gap, verbose=False, return_solution=True)
    prob, x_ref, it_ref, its_ref, reasons = R.solved_square(cell_type, degree, nx, ny, gap)
    assert all(r > 0 for r in reasons)
    assert it == it_ref and list(iterations) == list(its_ref), (it, iterations, it_ref, its_ref)
    nu = 2 * prob.nv
    assert x.shape == x_ref.shape and _rel(x[:nu], x_ref[:nu]) < 1e-10
    assert np.array_equal(cv, prob.cverts)
    assert np.all(x[prob.nv + prob.bc_nodes] == -0.25) and np.all(x[prob.bc_nodes] == 0.0)


@pytest.mark.parametrize("degree", [1, 2])
def test_half_disk_through_the_mesh_file_workflow(require_gpu, tmp_path, degree):
    """generate -> write_xdmf_tri -> read_tri_mesh -> solve_contact_problem, the README's alpha_0 = 0.005 and disp = -0.1 (alpha_0 = 1
    diverges in the twin as well: tests/signorini2d_reference.py HALF_DISK_RUNS): partial contact on the arc."""
    from proximalgalerkin_amd import io, mesh_generation
    from proximalgalerkin_amd import signorini as G

    mesh0, _, tags0 = mesh_generation.create_half_disk(**R.HALF_DISK)
    path = tmp_path / "meshes" / "half_disk.xdmf"
    io.write_xdmf_tri(path, mesh0, tags0)
    mesh, mt = io.read_tri_mesh(path)
    run = R.HALF_DISK_RUNS[degree]
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, {"contact": (2,), "displacement": (1,)}, degree=degree, disp=run["disp"],
                                                    alpha_0=run["alpha_0"], verbose=False, return_solution=True)
    prob, x_ref, it_ref, its_ref, reasons = R.solved_half_disk(degree, mesh.geometry, mesh.cells, mt.find(2), mt.find(1))
    assert all(r > 0 for r in reasons)
    assert it == it_ref and list(iterations) == list(its_ref), (it, iterations, it_ref, its_ref)
    nu = 2 * prob.nv
    assert _rel(x[:nu], x_ref[:nu]) < 1e-10
    assert np.array_equal(cv, prob.cverts)
    y = prob.coords[cv, 1] + x[prob.nv + cv]  # gap = 0
    h2r = 0.05**2 / 0.4  # discretisation error of the weakly imposed constraint: h^2 / R
    assert (y > 0.05).any() and (abs(y) < h2r).sum() >= 3 and y.min() > -h2r
    assert np.all(x[prob.nv + prob.bc_nodes] == run["disp"]) and np.all(x[prob.bc_nodes] == 0.0)


def test_symmetrised_lu_agrees_with_the_general_lu(require_gpu, monkeypatch):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import signorini as G

    cell_type, degree, nx, ny, gap = R.SYM_RUN
    mesh = fem.create_unit_square(nx, ny, cell_type=cell_type)
    mt, bcs = G.native_tags(mesh)
    runs = {}
    for sym in ("1", "0"):
        monkeypatch.setenv("PGX_SG_SYM", sym)
        runs[sym] = G.solve_contact_problem(mesh, mt, bcs, degree=degree, gap=gap, verbose=False, return_solution=True)
    (it1, its1, x1, _), (it0, its0, x0, _) = runs["1"], runs["0"]
    _, _, it_ref, its_ref, _ = R.solved_square(cell_type, degree, nx, ny, gap)
    assert it1 == it0 == it_ref and list(its1) == list(its0) == list(its_ref)
    assert _rel(x1, x0) < 1e-10
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, gap, -0.25, degree=degree, bc_facets=mt.find(1))
    assert problem.lu_stats()["symmetric"] is False  # (PGX_SG_SYM=0 is still set)
    problem.close()
    monkeypatch.delenv("PGX_SG_SYM")
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, gap, -0.25, degree=degree, bc_facets=mt.find(1))
    assert problem.lu_stats()["symmetric"] is True
    problem.close()


def test_unsupported_shapes_are_refused(require_gpu, monkeypatch):
    """PGX_EINVAL with a message: cells that are no parallelograms (the centre vertex of a 2 x 2 grid moved)"""
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd import signorini as G

    mesh = fem.create_unit_square(2, 2, cell_type="quadrilateral")
    mt, _ = G.native_tags(mesh)
    moved = mesh.geometry.copy()
    moved[4] += (0.1, 0.05)
    monkeypatch.setattr(G, "quad_lattice", lambda m, d: (moved, mesh.cells))
    with pytest.raises(_lib.PgxError, match="parallelogram"):
        G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.0, -0.25, degree=1, bc_facets=mt.find(1))


def test_command_line_dim_2(require_gpu, tmp_path):
    """`signorini.py --dim 2 --nx 4 --ny 3`: the quadrilateral unit square at the script's default degree 2; last line
    `it, iterations, sum, min, max` (signorini_dolfinx.py __main__)"""
    cell_type, degree, nx, ny, gap = R.CLI_RUN
    out = subprocess.run([sys.executable, str(ROOT / "examples" / "02_signorini" / "signorini.py"), "--dim", "2", "--nx", str(nx), "--ny", str(ny),
                          "--output", str(tmp_path / "output")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    _, _, it_ref, its_ref, _ = R.solved_square(cell_type, degree, nx, ny, gap)
    assert out.stdout.strip().splitlines()[-1] == f"{it_ref} {its_ref} {sum(its_ref)} {min(its_ref)} {max(its_ref)}"
    assert f"num_dofs_u={2 * (2 * nx + 1) * (2 * ny + 1)}, num_cells={nx * ny}" in out.stdout
    assert (tmp_path / "output" / "uh.vtu").exists() and (tmp_path / "output" / "von_mises.vtu").exists()
