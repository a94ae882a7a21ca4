"""The numpy twin of the diagnostics of examples 02 and 06 (tests/diagnostics_reference.py) against closed forms, and the
declaration of the new entry points.  No GPU: the GPU tests (tests/test_gpu_diagnostics.py) compare the kernels with this twin."""
import pathlib
import re

import numpy as np
import pytest

from tests import diagnostics_reference as R

ROOT = pathlib.Path(__file__).resolve().parents[1]

# a fixed non-symmetric displacement gradient: u = A x is exact in P1, P2, Q1 and Q2
A = np.array([[0.010, 0.020, -0.030], [0.005, -0.020, 0.040], [0.030, 0.000, 0.015]])
E, NU = 2.0e4, 0.3


def von_mises_of_A():
    """by hand: eps = sym(A), tr(eps) = 0.005; the deviator of sigma is 2 mu (eps - tr(eps)/3 I) - lambda drops out - so
    vm^2 = 3/2 * 4 mu^2 * (eps:eps - tr(eps)^2 / 3)"""
    mu = E / (2.0 * (1.0 + NU))
    e12, e13, e23 = 0.5 * (0.020 + 0.005), 0.5 * (-0.030 + 0.030), 0.5 * (0.040 + 0.000)
    ee = 0.010**2 + 0.020**2 + 0.015**2 + 2.0 * (e12**2 + e13**2 + e23**2)
    tr = 0.010 - 0.020 + 0.015
    return np.sqrt(1.5 * 4.0 * mu * mu * (ee - tr * tr / 3.0))


def sg_mesh(flavour, n):
    """(cell_type, degree, node coordinates, cells, contact facets z = 0) of the four element flavours, from the product's host-side
    mesh builders"""
    from proximalgalerkin_amd import signorini as G

    if flavour in ("P1", "P2"):
        mesh = G.create_unit_cube(*n)
        bottom = mesh.facets_where(lambda x: np.isclose(x[2], 0.0))
        if flavour == "P1":
            return 0, 1, mesh.geometry, mesh.cells, bottom
        coords, cells, (f6,) = G.p2_nodes(mesh, bottom)
        return 0, 2, coords, cells, f6
    mesh = G.create_unit_cube_hex(*n)
    d = 1 if flavour == "Q1" else 2
    coords, cells = mesh.lattice(d)
    return 1, d, coords, cells, mesh.facet_nodes(mesh.facets_where(lambda x: np.isclose(x[2], 0.0)), d)


def facet_rule(cell_type):
    from proximalgalerkin_amd import fem

    if cell_type == 0:
        return fem.quadrature_rule("triangle", 4)
    g, w = np.polynomial.legendre.leggauss(3)
    g, w = 0.5 * (g + 1.0), 0.5 * w
    return np.array([(g[a], g[b]) for b in range(3) for a in range(3)]), np.array([w[a] * w[b] for b in range(3) for a in range(3)])


def affine_state(coords):
    u = coords @ A.T
    return np.concatenate([u[:, 0], u[:, 1], u[:, 2]])


@pytest.mark.parametrize("flavour", ["P1", "P2", "Q1", "Q2"])
def test_von_mises_of_an_affine_displacement_is_the_hand_computed_constant(flavour):
    ct, deg, coords, cells, _ = sg_mesh(flavour, (3, 2, 2))
    vm = R.von_mises(affine_state(coords), coords, cells, E, NU, ct, deg)
    assert vm.shape == cells.shape
    ref = von_mises_of_A()
    assert np.abs(vm - ref).max() <= 1e-12 * ref


@pytest.mark.parametrize("flavour", ["P1", "P2", "Q1", "Q2"])
@pytest.mark.parametrize("c,gap", [(0.03, 0.01), (-0.03, 0.01)])
def test_penetration_of_a_uniform_displacement(flavour, c, gap):
    ct, deg, coords, cells, facets = sg_mesh(flavour, (3, 2, 2))
    nv = len(coords)
    x = np.concatenate([np.zeros(2 * nv), np.full(nv, -c)])
    qp, qw = facet_rule(ct)
    pen = R.penetration(x, coords, facets, gap, ct, deg, qp, qw)
    assert abs(pen - max(c + gap, 0.0)) <= 1e-14  # the contact face z = 0 of the unit cube has area 1
    v = R.violation(x, coords, gap)
    assert np.abs(v - (c - coords[:, 2] + gap)).max() <= 1e-15


def gc_arrays(cell_type, k, n):
    from proximalgalerkin_amd import fem, lagrange

    mesh = fem.create_unit_square(n[0], n[1], cell_type)
    if cell_type == "quadrilateral":
        n2, cd, xd = lagrange.numbering_quad(mesh, k)
        nv, cdp, _ = lagrange.numbering_quad(mesh, k - 1)
        return mesh.geometry, mesh.affine_corners, n2, nv, cd, cdp, xd
    n2, cd, xd = lagrange.numbering(mesh, k)
    nv, cdp, _ = lagrange.numbering(mesh, k - 1)
    return mesh.geometry, mesh.cells, n2, nv, cd, cdp, xd


@pytest.mark.parametrize("cell_type,k", [("triangle", 2), ("triangle", 3), ("quadrilateral", 2)])
def test_example_06_midpoint_values_of_a_quadratic(cell_type, k):
    from proximalgalerkin_amd.gradient_constraint import phi_default

    coords, corners, n2, nv, cd, cdp, xd = gc_arrays(cell_type, k, (5, 3))
    x = np.concatenate([xd[:, 0] ** 2 + 0.5 * xd[:, 1], np.zeros(2 * nv)])
    quad = cell_type == "quadrilateral"
    mid = (0.5, 0.5) if quad else (1.0 / 3.0, 1.0 / 3.0)
    out = R.gc_eval(x, coords, corners, cd, cdp, phi_default(xd.T), k, quad, [mid])
    X = coords[corners]
    xc = X[:, 0] + mid[0] * (X[:, 1] - X[:, 0]) + mid[1] * (X[:, 2] - X[:, 0])
    assert np.abs(out["grad_u"][:, 0, 0] - 2.0 * xc[:, 0]).max() <= 1e-12 and np.abs(out["grad_u"][:, 0, 1] - 0.5).max() <= 1e-12
    assert np.abs(out["phi"][:, 0] - phi_default(xc.T)).max() <= 1e-13
    assert np.abs(out["feas"]).max() == 0.0 and not out["feasible_active"].any()  # psi = 0: |0| - phi = -phi <= -0.1
    assert np.array_equal(out["active"][:, 0], (np.hypot(2.0 * xc[:, 0], 0.5) - phi_default(xc.T) >= 0).astype(np.uint8))


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_the_twins_tabulator_matches_the_oracles_and_is_nodal(k, quad):
    from oracle import gc_oracle as G6

    rng = np.random.default_rng(5)
    pts = rng.random((20, 2)) * (1.0 if quad else 0.5)
    if quad:
        t = np.arange(k + 1) / k
        nodes = np.array([(x, y) for y in t for x in t])
    else:
        nodes = G6.pk_lattice(k)[:, 1:] / k
    tab = G6.qk_tabulate if quad else G6.pk_tabulate
    for p in (pts, nodes, np.array([[0.5, 0.5] if quad else [1.0 / 3.0, 1.0 / 3.0]])):
        N, dN = R.lagrange_tabulate(k, p, quad)
        No, dNo = tab(k, p[:, 0], p[:, 1])
        assert np.abs(N - No).max() <= 1e-12 and np.abs(dN - dNo).max() <= 1e-12 * np.abs(dNo).max()
    assert np.array_equal(R.lagrange_tabulate(k, nodes, quad)[0], np.eye(len(nodes)))  # exactly the Kronecker delta at the nodes


def test_new_entry_points_are_declared():
    sg = (ROOT / "include" / "pgx_sg.h").read_text()
    gc = (ROOT / "include" / "pgx_gc.h").read_text()
    for name in ("pgx_sg_penetration", "pgx_sg_violation", "pgx_sg_von_mises"):
        assert re.search(r"\bint\s+%s\s*\(\s*pgx_sg_handle\s*\*" % name, sg), name
    assert re.search(r"\bint\s+pgx_gc_eval_cells\s*\(\s*pgx_gc_handle\s*\*\s*h\s*,\s*const\s+pgx_gc_points\s*\*", gc)
    assert "} pgx_gc_points;" in gc
