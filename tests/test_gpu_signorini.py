"""Example 02 (Signorini contact, 3-D elasticity) HIP path vs the CPU oracle (oracle/sg_oracle.py), through the C ABI of
include/pgx_sg.h.  Tolerances: kernels 1e-12 relative; full LVPP run: identical Newton counts, final displacement field
<= 1e-10 relative L2."""
import numpy as np
import pytest

from oracle import sg_oracle as S

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _setup(nx, ny, nz, gap=0.0, disp=-0.25):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(nx, ny, nz)
    mt, bcs = G.native_tags(mesh)
    contact = mt.find(2)
    bcv = np.unique(mt.find(1).ravel())
    problem = G.SignoriniProblem(mesh, contact, bcv, 2.0e4, 0.3, gap, disp)
    coords, cells = S.create_unit_cube_tets(nx, ny, nz)
    assert np.array_equal(coords, mesh.geometry) and np.array_equal(cells, mesh.cells)
    cf = S.boundary_facets_where(coords, cells, lambda c: np.isclose(c[:, 2], 0.0))
    prob = S.SignoriniP1(coords, cells, cf, np.flatnonzero(np.isclose(coords[:, 2], 1.0)), gap=gap, disp=disp)
    assert problem.ndofs == prob.ntot and np.array_equal(problem.contact_vertices, prob.cverts)
    return problem, prob


@pytest.mark.parametrize("n", [(2, 2, 2), (5, 3, 4), (9, 9, 9)])
def test_kernels_match_oracle(require_gpu, n):
    problem, prob = _setup(*n, gap=0.01)
    rng = np.random.default_rng(11)
    x = rng.standard_normal(prob.ntot) * 0.05
    x[3 * prob.nv:] = -np.abs(rng.standard_normal(prob.npsi)) * np.where(rng.random(prob.npsi) < 0.4, 400.0, 2.0)
    xk = rng.standard_normal(prob.ntot) * 0.05
    for alpha in (2.0, 64.0):
        problem.set_alpha(alpha)
        problem.set_prev(xk)
        F, fn = problem.residual(x)
        Fr = prob.residual(x, xk, alpha)
        assert _rel(F, Fr) < 1e-12 and abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
        J = problem.jacobian(x)
        Jr = prob.jacobian(x, alpha).tocsr()
        assert abs(J - Jr).max() <= 1e-12 * abs(Jr).max()
        nu3 = 3 * prob.nv
        assert abs(J[nu3:, nu3:] - Jr[nu3:, nu3:]).max() <= 1e-12 * abs(Jr[nu3:, nu3:]).max()
        v = rng.standard_normal(prob.ntot)
        assert _rel(problem.spmv(v), Jr @ v) < 1e-12
    problem.set_state(x)
    problem.set_prev(xk)
    assert abs(problem.u_increment() - np.linalg.norm((x - xk)[: 3 * prob.nv])) < 1e-12
    problem.close()


@pytest.mark.parametrize("n,gap", [((4, 4, 4), 0.0), ((8, 6, 5), 0.0), ((6, 6, 6), -0.1)])
def test_full_lvpp_run_matches_oracle(require_gpu, n, gap):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(*n)
    mt, bcs = G.native_tags(mesh)
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, bcs, gap=gap, verbose=False, return_solution=True)
    coords, cells = S.create_unit_cube_tets(*n)
    cf = S.boundary_facets_where(coords, cells, lambda c: np.isclose(c[:, 2], 0.0))
    prob = S.SignoriniP1(coords, cells, cf, np.flatnonzero(np.isclose(coords[:, 2], 1.0)), gap=gap)
    x_ref, it_ref, its_ref = S.solve_contact_problem(prob)
    assert it == it_ref and list(iterations) == list(its_ref)
    nu3 = 3 * prob.nv
    assert _rel(x[:nu3], x_ref[:nu3]) < 1e-10


@pytest.mark.parametrize("degree", [1, 2])
def test_problem_stated_as_forms_runs_the_same_solve(require_gpu, degree):
    """signorini_dolfinx.py:146-153, 199-291 stated through the UFL-subset front end (tensor algebra, ds measure over the contact
    tags, MixedFunctionSpace with the latent variable on the contact sub-mesh) reproduces the declarative driver, at degree 1 and at
    the reference's default degree 2 (functionspace(mesh, ("Lagrange", 2, (3,))), functionspace(submesh, ("Lagrange", 2)))."""
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(5, 4, 4) if degree == 1 else G.create_unit_cube(3, 3, 2)
    mt, bcs = G.native_tags(mesh)
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, bcs, degree=degree, gap=0.02, verbose=False, return_solution=True)
    it_f, iterations_f, u = G.solve_contact_problem_forms(mesh, mt, bcs, gap=0.02, degree=degree)
    assert it_f == it and list(iterations_f) == list(iterations)
    nu3 = u.x.array.size
    assert nu3 == 3 * (mesh.geometry.shape[0] if degree == 1 else G.p2_nodes(mesh)[0].shape[0])
    assert np.linalg.norm(u.x.array - x[:nu3]) <= 1e-12 * np.linalg.norm(x[:nu3])


@pytest.mark.parametrize("degree,disp", [(1, -0.12), (2, -0.105)])
def test_half_sphere_through_the_mesh_file_workflow(require_gpu, tmp_path, degree, disp):
    """The reference's own workflow for its flagship contact geometry (examples/02_signorini/generate_mesh.py +
    `signorini_dolfinx.py file`): half sphere of lvpp.mesh_generation.create_half_sphere (curved surface tagged 2 = contact, flat top
    tagged 1 = prescribed displacement) -> XDMF file -> read_mesh / read_meshtags -> LVPP solve.  Curved contact facets, unstructured
    vertex numbering after the file round trip; HIP path vs oracle on the same mesh, degrees 1 and 2."""
    from proximalgalerkin_amd import io, mesh_generation
    from proximalgalerkin_amd import signorini as G

    mesh0, _, ft0 = mesh_generation.create_half_sphere(res=0.15)
    path = tmp_path / "meshes" / "half_sphere.xdmf"
    io.write_xdmf_tet(path, mesh0, ft0)
    mesh, mt = io.read_tet_mesh(path)
    bcs = {"contact": (2,), "displacement": (1,)}
    # the displacement presses the pole slightly below the plane z = 0; the reference's default -0.25 (and -0.12 at degree 2) ends in
    # SNES_DIVERGED_DTOL on this coarse mesh in the oracle as well (full Newton steps, no line search)
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, bcs, degree=degree, disp=disp, verbose=False, return_solution=True)
    # the half sphere is an ORDER-2 mesh (the reference's default, mesh_generation.py:88): curved cells and facets since round 5
    assert mesh.curved and np.abs(mesh.midside - mesh0.midside).max() == 0.0
    if degree == 1:
        prob = S.SignoriniP1(mesh.geometry, mesh.cells, mt.find(2), np.unique(mt.find(1).ravel()), gap=0.0, disp=disp, midside=mesh.midside)
        coords, top = mesh.geometry, np.unique(mt.find(1).ravel())
    else:
        prob = S.SignoriniP2(mesh.geometry, mesh.cells, mt.find(2), mt.find(1), gap=0.0, disp=disp, midside=mesh.midside)
        coords, top = prob.node_coords, prob.bc_nodes
    xr, itr, itsr = S.solve_contact_problem(prob)
    assert (it, iterations) == (itr, itsr), (it, iterations, itr, itsr)
    nv = prob.nv
    assert np.array_equal(np.sort(cv), prob.cverts)
    assert _rel(x[:3 * nv], xr[:3 * nv]) < 1e-10
    uz = x[2 * nv:3 * nv]
    # the constraint holds weakly: nodal penetration of the plane z = 0 of the order h^2 / r (h = 0.15)
    assert -0.02 < (coords[cv, 2] + uz[cv]).min() < 0.01
    assert np.all(uz[top] == disp) and np.all(x[top] == 0.0)


# ------------------------------------------------------------------------------------------------------------------
# degree 2 - the reference's default (signorini_dolfinx.py:68-73): u in (P2)^3, psi in P2 on the contact facets
# ------------------------------------------------------------------------------------------------------------------
def _setup_p2(nx, ny, nz, gap=0.0, disp=-0.25):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(nx, ny, nz)
    mt, bcs = G.native_tags(mesh)
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, gap, disp, degree=2, bc_facets=mt.find(1))
    prob = S.SignoriniP2(mesh.geometry, mesh.cells, mt.find(2), mt.find(1), gap=gap, disp=disp)
    assert problem.ndofs == prob.ntot and np.array_equal(problem.contact_vertices, prob.cverts)
    assert np.array_equal(problem.node_coords, prob.node_coords)
    return problem, prob


@pytest.mark.parametrize("n", [(1, 1, 1), (3, 2, 2), (5, 4, 3)])
def test_degree2_kernels_match_oracle(require_gpu, n):
    problem, prob = _setup_p2(*n, gap=0.01)
    rng = np.random.default_rng(12)
    x = rng.standard_normal(prob.ntot) * 0.05
    x[3 * prob.nv:] = -np.abs(rng.standard_normal(prob.npsi)) * np.where(rng.random(prob.npsi) < 0.4, 400.0, 2.0)
    xk = rng.standard_normal(prob.ntot) * 0.05
    for alpha in (2.0, 64.0):
        problem.set_alpha(alpha)
        problem.set_prev(xk)
        F, fn = problem.residual(x)
        Fr = prob.residual(x, xk, alpha)
        assert _rel(F, Fr) < 1e-12 and abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
        J = problem.jacobian(x)
        Jr = prob.jacobian(x, alpha).tocsr()
        assert abs(J - Jr).max() <= 1e-12 * abs(Jr).max()
        nu3 = 3 * prob.nv
        assert abs(J[nu3:, nu3:] - Jr[nu3:, nu3:]).max() <= 1e-12 * abs(Jr[nu3:, nu3:]).max()  # D(psi) on its own scale
        v = rng.standard_normal(prob.ntot)
        assert _rel(problem.spmv(v), Jr @ v) < 1e-12
        F2, _ = problem.residual(x)
        assert np.array_equal(F, F2)  # atomic-free assembly: bitwise reproducible
    problem.close()


@pytest.mark.parametrize("n,gap", [((2, 2, 2), 0.0), ((4, 3, 3), 0.0), ((3, 3, 3), -0.1)])
def test_degree2_full_lvpp_run_matches_oracle(require_gpu, n, gap):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(*n)
    mt, bcs = G.native_tags(mesh)
    it, iterations, x, cv = G.solve_contact_problem(mesh, mt, bcs, degree=2, gap=gap, verbose=False, return_solution=True)
    prob = S.SignoriniP2(mesh.geometry, mesh.cells, mt.find(2), mt.find(1), gap=gap)
    x_ref, it_ref, its_ref = S.solve_contact_problem(prob)
    assert it == it_ref and list(iterations) == list(its_ref), (it, iterations, it_ref, its_ref)
    nu3 = 3 * prob.nv
    assert _rel(x[:nu3], x_ref[:nu3]) < 1e-10
    assert np.array_equal(np.sort(cv), prob.cverts)
    # the degree-2 displacement agrees with the degree-1 one on a finer mesh to discretisation accuracy (independent discretisations)
    uz = x[2 * prob.nv:3 * prob.nv]
    assert abs(uz[prob.bc_nodes] + 0.25).max() == 0.0


@pytest.mark.parametrize("degree", [1, 2])
def test_curved_cell_kernels_on_the_order2_half_sphere_match_the_oracle(require_gpu, degree):
    """pgx_sg_create_curved (round 5): |det J| and J^-1 of the quadratic cell map per point of the cell rule (degree 2 (k - 1) + 3),
    surface element and z of the 6-node contact facets per facet point; degree 2: the ten nodes of a tetrahedron are its geometry nodes
    (isoparametric), degree 1: P1 fields on the same curved cells - against the oracle with the same map (oracle/sg_oracle.py
    Signorini*(midside=...)) on the natively meshed order-2 half sphere: residual, Jacobian (the elasticity block, the facet coupling
    and D(psi) each on its own scale), SpMV <= 1e-12; NOT the affine discretisation's values; the contact surface's area is the
    sphere's to 3e-3 where the flat facets miss 2e-2."""
    from proximalgalerkin_amd import mesh_generation
    from proximalgalerkin_amd import signorini as G

    mesh, _, mt = mesh_generation.create_half_sphere(res=0.15)
    assert mesh.curved
    if degree == 2:
        problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.01, -0.1, degree=2, bc_facets=mt.find(1))
        prob = S.SignoriniP2(mesh.geometry, mesh.cells, mt.find(2), mt.find(1), gap=0.01, disp=-0.1, midside=mesh.midside)
        flat = S.SignoriniP2(mesh.geometry, mesh.cells, mt.find(2), mt.find(1), gap=0.01, disp=-0.1)
        assert np.array_equal(problem.node_coords, prob.node_coords)
    else:
        bv = np.unique(mt.find(1).ravel())
        problem = G.SignoriniProblem(mesh, mt.find(2), bv, 2.0e4, 0.3, 0.01, -0.1, degree=1)
        prob = S.SignoriniP1(mesh.geometry, mesh.cells, mt.find(2), bv, gap=0.01, disp=-0.1, midside=mesh.midside)
        flat = S.SignoriniP1(mesh.geometry, mesh.cells, mt.find(2), bv, gap=0.01, disp=-0.1)
    assert problem.ndofs == prob.ntot and np.array_equal(problem.contact_vertices, prob.cverts)
    rng = np.random.default_rng(14)
    x = rng.standard_normal(prob.ntot) * 0.05
    x[3 * prob.nv:] = -np.abs(rng.standard_normal(prob.npsi)) * np.where(rng.random(prob.npsi) < 0.4, 400.0, 2.0)
    xk = rng.standard_normal(prob.ntot) * 0.05
    nu3 = 3 * prob.nv
    for alpha in (2.0, 64.0):
        problem.set_alpha(alpha)
        problem.set_prev(xk)
        F, fn = problem.residual(x)
        Fr = prob.residual(x, xk, alpha)
        assert _rel(F, Fr) < 1e-12 and abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
        assert _rel(F, flat.residual(x, xk, alpha)) > 1e-3
        J = problem.jacobian(x)
        Jr = prob.jacobian(x, alpha).tocsr()
        assert abs(J - Jr).max() <= 1e-12 * abs(Jr).max()
        assert abs(J[nu3:, nu3:] - Jr[nu3:, nu3:]).max() <= 1e-12 * abs(Jr[nu3:, nu3:]).max()
        assert abs(J[nu3:, :nu3] - Jr[nu3:, :nu3]).max() <= 1e-12 * abs(Jr[nu3:, :nu3]).max()  # the facet mass coupling on its own scale
        v = rng.standard_normal(prob.ntot)
        assert _rel(problem.spmv(v), Jr @ v) < 1e-12
    area = 2 * np.pi * 0.4**2
    assert abs(prob.MG.sum() - area) < 3e-3 and abs(flat.MG.sum() - area) > 1e-2
    problem.close()


# ------------------------------------------------------------------------------------------------------------------
# hexahedra - the reference's native mesh (signorini_dolfinx.py:376-383), Q1 and Q2 (its default degree)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,degree", [((2, 2, 2), 1), ((4, 3, 2), 1), ((2, 2, 2), 2), ((4, 3, 3), 2)])
def test_hexahedra_kernels_and_full_run_match_oracle(require_gpu, n, degree):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube_hex(*n)
    mt, bcs = G.native_tags(mesh)
    prob = S.SignoriniHex(*n, degree=degree, gap=0.01)
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.01, -0.25, degree=degree, bc_facets=mt.find(1))
    assert problem.ndofs == prob.ntot and np.array_equal(problem.contact_vertices, prob.cverts)
    assert np.array_equal(problem.node_coords, prob.node_coords)
    rng = np.random.default_rng(13)
    x = rng.standard_normal(prob.ntot) * 0.05
    x[3 * prob.nv:] = -np.abs(rng.standard_normal(prob.npsi)) * np.where(rng.random(prob.npsi) < 0.4, 400.0, 2.0)
    xk = rng.standard_normal(prob.ntot) * 0.05
    for alpha in (2.0, 64.0):
        problem.set_alpha(alpha)
        problem.set_prev(xk)
        F, fn = problem.residual(x)
        Fr = prob.residual(x, xk, alpha)
        assert _rel(F, Fr) < 1e-12
        J = problem.jacobian(x)
        Jr = prob.jacobian(x, alpha).tocsr()
        assert abs(J - Jr).max() <= 1e-12 * abs(Jr).max()
        nu3 = 3 * prob.nv
        assert abs(J[nu3:, nu3:] - Jr[nu3:, nu3:]).max() <= 1e-12 * abs(Jr[nu3:, nu3:]).max()
    problem.close()
    it, iterations, xs, cv = G.solve_contact_problem(mesh, mt, bcs, degree=degree, gap=0.01, verbose=False, return_solution=True)
    x_ref, it_ref, its_ref = S.solve_contact_problem(prob)
    assert it == it_ref and list(iterations) == list(its_ref), (it, iterations, it_ref, its_ref)
    assert _rel(xs[:3 * prob.nv], x_ref[:3 * prob.nv]) < 1e-10


def test_symmetrised_lu_agrees_with_the_general_lu(require_gpu, monkeypatch):
    """Round 5: the Newton matrix [[alpha A, M_G^T], [-M_G, D]] enters the sparse LU with the rows of its latent block negated - a
    symmetric matrix, factorised as L D L^T at half the flops (csrc/pgx_mixed.hip mx_lu_factor / lu_flip_from, pgx_nd_set_symmetric).  PGX_SG_SYM=0 keeps
    the general LU of the matrix as assembled: same Newton counts, same solution to the accuracy of the refined solves."""
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(6, 5, 4)
    mt, bcs = G.native_tags(mesh)
    runs = {}
    for sym in ("1", "0"):
        monkeypatch.setenv("PGX_SG_SYM", sym)
        runs[sym] = G.solve_contact_problem(mesh, mt, bcs, degree=2, verbose=False, return_solution=True)
    (it1, its1, x1, _), (it0, its0, x0, _) = runs["1"], runs["0"]
    assert it1 == it0 and list(its1) == list(its0)
    assert _rel(x1, x0) < 1e-10
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.0, -0.25, degree=2, bc_facets=mt.find(1))
    assert problem.lu_stats()["symmetric"] is False  # (PGX_SG_SYM=0 is still set)
    problem.close()
    monkeypatch.delenv("PGX_SG_SYM")
    problem = G.SignoriniProblem(mesh, mt.find(2), None, 2.0e4, 0.3, 0.0, -0.25, degree=2, bc_facets=mt.find(1))
    assert problem.lu_stats()["symmetric"] is True
    problem.close()
