"""The diagnostics of examples 02 and 06 on the device (include/pgx_sg.h: pgx_sg_penetration / violation / von_mises; include/pgx_gc.h:
pgx_gc_eval_cells) against their numpy twin tests/diagnostics_reference.py, which tests/test_cpu_diagnostics.py checks against closed
forms.  Tolerances: von Mises, violation and the continuous fields of example 06 1e-12 relative to the array's largest magnitude (the
project's kernel bar); penetration |a - b| <= 1e-12 |b| + 1e-14 (the absolute term covers the cancellation in -u_z - z + gap, whose
inputs are O(1)); flags equal wherever the twin's margin is farther than 1e-13 max(1, phi) from its threshold, at most 1 % of the points
left out by that rule."""
import pathlib
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tests import diagnostics_reference as R
from tests.test_cpu_diagnostics import NU, A, E, affine_state, von_mises_of_A

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"


def _close(a, b, rtol=1e-12):
    return np.abs(a - b).max() <= rtol * np.abs(b).max()


def _pen_close(a, b):
    return abs(a - b) <= 1e-12 * abs(b) + 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# example 02
# ---------------------------------------------------------------------------------------------------------------------
def _curved_cube():
    """tests/golden/cube_3x2x2_order2.msh with its mid-edge nodes (straight in the file) pushed off the edge midpoints, so that cells
    AND contact facets are genuinely quadratic: the handle is one of pgx_sg_create_curved"""
    from proximalgalerkin_amd import io
    from proximalgalerkin_amd import signorini as G

    mesh, mt = io.read_tet_mesh(GOLD / "cube_3x2x2_order2.msh")
    e = mesh.edges()
    m = 0.5 * (mesh.geometry[e[:, 0]] + mesh.geometry[e[:, 1]])
    bump = 0.02 * np.sin(np.pi * m[:, 0]) * np.sin(np.pi * m[:, 1])
    mid = m + np.stack([0.3 * bump * (1.0 - m[:, 2]), -0.2 * bump * (1.0 - m[:, 2]), bump * (1.0 - m[:, 2])], axis=1)
    mesh = G.TetMesh(mesh.geometry, mesh.cells, midside=mid)
    assert mesh.curved
    return mesh, mt


def _sg(flavour, n=None, gap=0.01):
    """(problem, twin arguments: cell_type, degree, curved 6-node facet geometry or None)"""
    from proximalgalerkin_amd import signorini as G

    if flavour.startswith("curved"):
        mesh, mt = _curved_cube()
        degree = int(flavour[-1])
    else:
        mesh = G.create_unit_cube_hex(*n) if flavour[0] == "Q" else G.create_unit_cube(*n)
        mt, _ = G.native_tags(mesh)
        degree = int(flavour[1])
    bv = np.unique(mt.find(1).ravel()) if degree == 1 and flavour[0] != "Q" else None
    problem = G.SignoriniProblem(mesh, mt.find(2), bv, E, NU, gap, -0.25, degree=degree, bc_facets=mt.find(1))
    geo6 = None
    if flavour.startswith("curved"):
        if degree == 2:
            geo6 = problem.node_coords[problem.facets]
        else:
            gcoords, _, (g6,) = G.p2_nodes(mesh, problem.facets)
            geo6 = gcoords[g6]
    return problem, (problem.cell_type, degree, geo6)


def _sg_state(problem, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(problem.ndofs) * 0.05  # (tests/test_gpu_signorini.py:35-37)


def _sg_twin(problem, tw, x):
    ct, degree, geo6 = tw
    qp, qw = problem.facet_quadrature
    pen = R.penetration(x, problem.node_coords, problem.facets, problem.gap, ct, degree, qp, qw, geo6)
    vio = R.violation(x, problem.node_coords, problem.gap)
    vm = None if geo6 is not None else R.von_mises(x, problem.node_coords, problem.cells, E, NU, ct, degree)
    return pen, vio, vm


SG_CASES = [("P1", (2, 2, 2)), ("P1", (5, 3, 4)), ("P1", (9, 9, 9)), ("P2", (3, 2, 2)), ("Q1", (3, 2, 2)), ("Q2", (3, 2, 2))]


@pytest.mark.parametrize("flavour,n", SG_CASES)
def test_signorini_diagnostics_match_the_twin(require_gpu, flavour, n):
    problem, tw = _sg(flavour, n)
    x = _sg_state(problem)
    problem.set_state(x)
    pen_r, vio_r, vm_r = _sg_twin(problem, tw, x)
    contact = np.unique(problem.facets)
    assert (vio_r[contact] > 0).any() and (vio_r[contact] < 0).any()  # mixed sign of u.n_g - g over the contact face
    pen, vio, vm = problem.penetration(), problem.violation(), problem.von_mises()
    print(f"{flavour} {n}: penetration {pen:.17g} twin {pen_r:.17g}; violation err {np.abs(vio - vio_r).max():.2e}; "
          f"von Mises err {np.abs(vm - vm_r).max():.2e} of {np.abs(vm_r).max():.2e}")
    assert pen_r > 0 and _pen_close(pen, pen_r)
    assert vio.shape == (problem.nv,) and _close(vio, vio_r)
    assert vm.shape == problem.cells.shape and _close(vm, vm_r)
    # determinism: twice the same bits, and on a fresh handle with the same state
    assert problem.penetration() == pen and np.array_equal(problem.violation(), vio) and np.array_equal(problem.von_mises(), vm)
    problem.close()
    fresh, _ = _sg(flavour, n)
    fresh.set_state(x)
    assert fresh.penetration() == pen
    fresh.close()


@pytest.mark.parametrize("degree", [1, 2])
def test_signorini_diagnostics_on_order_2_geometry(require_gpu, degree):
    from proximalgalerkin_amd._lib import PgxError

    problem, tw = _sg(f"curved{degree}")
    x = _sg_state(problem)
    problem.set_state(x)
    pen_r, vio_r, _ = _sg_twin(problem, tw, x)
    flat = R.penetration(x, problem.node_coords, problem.facets, problem.gap, 0, degree, *problem.facet_quadrature)
    assert abs(flat - pen_r) > 1e-6 * pen_r  # the curved facets matter: the affine formula gives another number
    contact = np.unique(problem.facets)
    assert (vio_r[contact] > 0).any() and (vio_r[contact] < 0).any()
    pen, vio = problem.penetration(), problem.violation()
    print(f"curved degree {degree}: penetration {pen:.17g} twin {pen_r:.17g} (affine formula {flat:.17g})")
    assert _pen_close(pen, pen_r) and _close(vio, vio_r)
    with pytest.raises(PgxError, match=r"code -1\).*pgx_sg_create_curved"):  # PGX_EINVAL, with the reason
        problem.von_mises()
    problem.close()


@pytest.mark.parametrize("flavour", ["P1", "P2", "Q1", "Q2"])
def test_signorini_closed_forms_on_the_device(require_gpu, flavour):
    problem, _ = _sg(flavour, (3, 2, 2))
    nv = problem.nv
    problem.set_state(np.concatenate([affine_state(problem.node_coords), np.zeros(problem.npsi)]))
    ref = von_mises_of_A()
    assert np.abs(problem.von_mises() - ref).max() <= 1e-12 * ref
    for c, gap in ((0.03, 0.01), (-0.03, 0.01)):
        p2, _ = _sg(flavour, (3, 2, 2), gap=gap)
        p2.set_state(np.concatenate([np.zeros(2 * nv), np.full(nv, -c), np.zeros(p2.npsi)]))
        assert _pen_close(p2.penetration(), max(c + gap, 0.0))
        p2.close()
    problem.close()


def test_signorini_diagnostics_leave_the_handle_unchanged(require_gpu):
    from proximalgalerkin_amd import _lib

    problem, _ = _sg("P2", (3, 2, 2))
    x, xk = _sg_state(problem), _sg_state(problem, seed=12)
    problem.set_alpha(4.0)
    problem.set_state(x)
    problem.set_prev(xk)
    J = problem.jacobian()
    F1, _ = problem.residual()
    s1, k1 = problem.get_state(), problem.get_prev()
    problem.penetration(), problem.violation(), problem.von_mises()
    val = np.empty(J.nnz)
    problem._call("csr_export", None, None, None, None, _lib.dptr(val))  # the filled Jacobian is still valid, and the same
    F2, _ = problem.residual()
    assert np.array_equal(val, J.data) and np.array_equal(F1, F2)
    assert np.array_equal(problem.get_state(), s1) and np.array_equal(s1, x) and np.array_equal(problem.get_prev(), k1)
    problem.close()


def _sg_lvpp(mesh, mt, bcs, record):
    """the loop of solve_contact_problem (defaults), keeping the handle: -> (problem, Newton counts); `record(problem)` runs before
    every proximal step"""
    from proximalgalerkin_amd import signorini as G

    problem = G.SignoriniProblem(mesh, mt.find(2), np.unique(mt.find(1).ravel()), E, NU, 0.0, -0.25, bc_facets=mt.find(1))
    iterations = []
    for it in range(1, 26):
        record(problem)
        problem.set_alpha(2.0**it)
        tol = 1e-5 if it < 2 else 1e-6
        problem.solver.setTolerances(atol=tol, rtol=tol)
        problem.solve()
        iterations.append(problem.solver.getIterationNumber())
        if problem.u_increment() <= 1e-6:
            break
        problem.advance_prev()
    return problem, iterations


def test_signorini_diagnostics_after_a_real_solve_and_the_penetration_collector(require_gpu):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(4, 4, 4)
    mt, bcs = G.native_tags(mesh)
    states = []
    problem, its = _sg_lvpp(mesh, mt, bcs, lambda p: states.append(p.get_state()))
    x = problem.get_state()
    tw = (0, 1, None)
    pen_r, vio_r, vm_r = _sg_twin(problem, tw, x)
    pen, vio, vm = problem.penetration(), problem.violation(), problem.von_mises()
    print(f"after the solve: penetration {pen:.17g} twin {pen_r:.17g}; max von Mises {vm_r.max():.6g}")
    assert _pen_close(pen, pen_r) and _close(vio, vio_r) and _close(vm, vm_r)
    pens_r = [_sg_twin(problem, tw, s)[0] for s in states]
    problem.close()
    it0, its0, x0, _ = G.solve_contact_problem(mesh, mt, bcs, verbose=False, return_solution=True)
    hist = []
    it1, its1, x1, _ = G.solve_contact_problem(mesh, mt, bcs, verbose=False, return_solution=True, penetration_history=hist)
    assert list(its0) == list(its1) == list(its) and it0 == it1 and np.array_equal(x0, x1) and np.array_equal(x0, x)
    assert len(hist) == len(pens_r) and all(_pen_close(a, b) for a, b in zip(hist, pens_r)), (hist, pens_r)


# ---------------------------------------------------------------------------------------------------------------------
# example 06
# ---------------------------------------------------------------------------------------------------------------------
# u = s_k N(0,1): the gradient of a random nodal field grows like k^2 (node spacing h / k, inverse estimate), so the scale is halved
# per degree to keep |grad u| - phi of either sign; |psi| = 10^U(-2, 6) puts |feas| - phi on both sides of -1e-8
S_K = {2: 0.032, 3: 0.016, 4: 0.008}
GC_CASES = [(ct, n, k, g) for ct, n in (("triangle", (13, 11)), ("triangle", (5, 3)), ("quadrilateral", (4, 3)), ("quadrilateral", (9, 7)))
            for k, g in ((2, False), (2, True), (3, True), (4, True)) if not (ct == "quadrilateral" and not g)]


def _gc(cell_type, n, k, general):
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.gradient_constraint import GradientConstraintProblem, f_default, phi_default

    mesh = fem.create_unit_square(n[0], n[1], cell_type)
    return GradientConstraintProblem(mesh, phi_default, f_default, degree=k, general=general)


def _gc_state(problem):
    rng = np.random.default_rng(7)
    u = S_K[problem.degree] * rng.standard_normal(problem.n2)
    mag, th = 10.0 ** rng.uniform(-2, 6, problem.nv), rng.uniform(0, 2 * np.pi, problem.nv)
    return np.concatenate([u, mag * np.cos(th), mag * np.sin(th)])


def _gc_points(problem):
    quad = problem.mesh.cell_name() == "quadrilateral"
    return quad, ((0.5, 0.5) if quad else (1.0 / 3.0, 1.0 / 3.0)), problem.latent_nodes()


def _gc_twin(problem, x, pts):
    quad = problem.mesh.cell_name() == "quadrilateral"
    return R.gc_eval(x, problem.mesh.geometry, problem.corners, problem.cell_dofs_u, problem.cell_dofs_p, problem.phi_dofs, problem.degree,
                     quad, pts)


def _gc_compare(problem, x, pts, label):
    """device vs twin at `pts`; returns the device outputs"""
    ref = _gc_twin(problem, x, pts)
    gu, fe, ph, ac, fa = problem.eval_cells(pts)
    nc, n = problem.mesh.num_cells, len(pts)
    assert gu.shape == fe.shape == (nc, n, 2) and ph.shape == ac.shape == fa.shape == (nc, n)
    assert ac.dtype == fa.dtype == np.uint8 and set(np.unique(ac)) <= {0, 1} and set(np.unique(fa)) <= {0, 1}
    tol = 1e-13 * np.maximum(1.0, ref["phi"])
    sure_a, sure_f = np.abs(ref["margin_active"]) > tol, np.abs(ref["margin_feasible"] + 1e-8) > tol
    left_out = 1.0 - 0.5 * (sure_a.mean() + sure_f.mean())
    print(f"{label}: grad_u err {np.abs(gu - ref['grad_u']).max():.2e} of {np.abs(ref['grad_u']).max():.2e}, feas err "
          f"{np.abs(fe - ref['feas']).max():.2e}, phi err {np.abs(ph - ref['phi']).max():.2e}; active {ac.mean():.2f} feasible_active "
          f"{fa.mean():.2f}; left out {left_out:.4f}")
    assert _close(gu, ref["grad_u"]) and _close(fe, ref["feas"]) and _close(ph, ref["phi"])
    assert (~sure_a).mean() <= 0.01 and (~sure_f).mean() <= 0.01
    assert np.array_equal(ac[sure_a], ref["active"][sure_a]) and np.array_equal(fa[sure_f], ref["feasible_active"][sure_f])
    return gu, fe, ph, ac, fa


@pytest.mark.parametrize("cell_type,n,k,general", GC_CASES)
def test_gradient_constraint_evaluation_matches_the_twin(require_gpu, cell_type, n, k, general):
    problem = _gc(cell_type, n, k, general)
    assert problem.general == general
    x = _gc_state(problem)
    problem.set_state(x)
    quad, mid, nodes = _gc_points(problem)
    label = f"{cell_type} {n} degree {k}{' general' if general else ''}"
    out_mid = _gc_compare(problem, x, [mid], label + " midpoint")
    for flag in out_mid[3:]:  # each flag takes each value in at least 5 % of the cells
        assert 0.05 <= flag.mean() <= 0.95, flag.mean()
    out_nodes = _gc_compare(problem, x, nodes, label + " latent nodes")
    a, fa = problem.active_sets()
    assert a.shape == fa.shape == (problem.mesh.num_cells,) and np.array_equal(a, out_mid[3][:, 0]) and np.array_equal(fa, out_mid[4][:, 0])
    for got, want in zip(problem.dg_fields(), out_nodes[:3]):
        assert np.array_equal(got, want)  # (and twice the same bits)
    if k == 2 and general and not quad:  # the table-driven handle against the specialised one
        spec = _gc(cell_type, n, 2, False)
        spec.set_state(x)
        for pts in ([mid], nodes):
            for g, s in zip(problem.eval_cells(pts), spec.eval_cells(pts)):
                if g.dtype == np.uint8:
                    assert np.array_equal(g, s)
                else:
                    assert _close(g, s)
        spec.close()
    problem.close()


@pytest.mark.parametrize("cell_type,k,general", [("triangle", 2, False), ("triangle", 3, True), ("quadrilateral", 2, True)])
def test_gradient_constraint_closed_form_on_the_device(require_gpu, cell_type, k, general):
    from proximalgalerkin_amd.gradient_constraint import phi_default

    problem = _gc(cell_type, (5, 3), k, general)
    xd = problem.dof_coords
    problem.set_state(np.concatenate([xd[:, 0] ** 2 + 0.5 * xd[:, 1], np.zeros(2 * problem.nv)]))
    quad, mid, _ = _gc_points(problem)
    gu, fe, ph, ac, fa = problem.eval_cells([mid])
    X = problem.mesh.geometry[problem.corners]
    xc = X[:, 0] + mid[0] * (X[:, 1] - X[:, 0]) + mid[1] * (X[:, 2] - X[:, 0])
    assert np.abs(gu[:, 0, 0] - 2.0 * xc[:, 0]).max() <= 1e-12 and np.abs(gu[:, 0, 1] - 0.5).max() <= 1e-12
    assert np.abs(ph[:, 0] - phi_default(xc.T)).max() <= 1e-13 and np.abs(fe).max() == 0.0 and not fa.any()
    problem.close()


def test_gradient_constraint_diagnostics_after_a_real_solve_leave_the_handle_unchanged(require_gpu):
    from proximalgalerkin_amd import _lib

    problem = _gc("triangle", (12, 12), 2, False)
    for i in range(25):  # the loop of solve_problem (defaults)
        problem.set_alpha(2.0**i)
        problem.solve()
        if problem.l2_increment() < 1e-8:
            break
        problem.advance_prev()
    x = problem.get_state()
    quad, mid, nodes = _gc_points(problem)
    _gc_compare(problem, x, [mid], "after the solve, midpoint")
    _gc_compare(problem, x, nodes, "after the solve, latent nodes")
    J = problem.jacobian()
    F1, _ = problem.residual()
    k1 = problem.get_prev()
    first = problem.eval_cells(nodes)
    problem.active_sets(), problem.dg_fields()
    val = np.empty(J.nnz)
    problem._call("csr_export", None, None, None, None, _lib.dptr(val))
    F2, _ = problem.residual()
    assert np.array_equal(val, J.data) and np.array_equal(F1, F2)
    assert np.array_equal(problem.get_state(), x) and np.array_equal(problem.get_prev(), k1)
    for a, b in zip(first, problem.eval_cells(nodes)):
        assert np.array_equal(a, b)
    problem.close()


# ---------------------------------------------------------------------------------------------------------------------
# output files
# ---------------------------------------------------------------------------------------------------------------------
def _vtu(path):
    """(points, cells, {point array: tuples}, {cell array: tuples}) of a VTK XML file"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid"
    piece = root.find("UnstructuredGrid").find("Piece")

    def arrays(tag):
        out = {}
        for a in piece.find(tag).findall("DataArray"):
            out[a.get("Name")] = len(a.text.split()) // int(a.get("NumberOfComponents") or 1)
        return out

    return int(piece.get("NumberOfPoints")), int(piece.get("NumberOfCells")), arrays("PointData"), arrays("CellData")


@pytest.mark.parametrize("kind,degree", [("tet", 1), ("tet", 2), ("hex", 2)])
def test_signorini_output_files(require_gpu, tmp_path, kind, degree):
    from proximalgalerkin_amd import signorini as G

    mesh = G.create_unit_cube(3, 2, 2) if kind == "tet" else G.create_unit_cube_hex(3, 2, 2)
    mt, bcs = G.native_tags(mesh)
    G.solve_contact_problem(mesh, mt, bcs, degree=degree, max_iterations=2, verbose=False, output=tmp_path)
    npts, nc, pd, cd = _vtu(tmp_path / "uh.vtu")
    assert pd == {"displacement": npts, "violation": npts}
    npts, nc, pd, cd = _vtu(tmp_path / "von_mises.vtu")
    corners = 4 if kind == "tet" else 8
    assert nc == mesh.cells.shape[0] and npts == corners * nc and pd == {"VonMises": npts, "u": npts}  # points duplicated per cell


@pytest.mark.parametrize("cell_type,k", [("triangle", 2), ("triangle", 3), ("quadrilateral", 2)])
def test_gradient_constraint_output_files(require_gpu, tmp_path, cell_type, k):
    from proximalgalerkin_amd.gradient_constraint import solve_problem

    solve_problem(4, 3, primal_degree=k, cell_type=cell_type, max_iterations=2, result_dir=tmp_path, verbose=False)
    ncell = 24 if cell_type == "triangle" else 12
    tri = 24
    npts, nc, pd, cd = _vtu(tmp_path / "active_set.vtu")
    assert nc == tri and cd == {"active_set": tri, "global_feasible_active_set": tri}
    npts, nc, pd, cd = _vtu(tmp_path / "grad_u.vtu")
    assert nc == tri and npts == ncell * (3 if cell_type == "triangle" else 4)
    assert pd == {"grad(u)": npts, "Global feasible gradient": npts, "phi": npts}
