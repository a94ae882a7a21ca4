"""CPU tests of example 04's host side (crossed mesh, initial condition, degree-7 rule, refusals) and of the numpy restatement
the GPU tests compare against (tests/multiphase_reference.py)."""
import hashlib
import json
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import fem, multiphase
from tests import multiphase_reference as R

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _areas(mesh):
    g, c = mesh.geometry, mesh.cells
    a, b = g[c[:, 1]] - g[c[:, 0]], g[c[:, 2]] - g[c[:, 0]]
    return 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


@pytest.mark.parametrize("N,M", [(1, 1), (3, 2), (50, 50)])
def test_crossed_mesh(N, M):
    mesh = fem.create_unit_square(N, M, diagonal="crossed")
    assert mesh.num_vertices == (N + 1) * (M + 1) + N * M
    assert mesh.num_cells == 4 * N * M
    assert mesh.structured is None
    area = _areas(mesh)
    assert np.all(area > 0)
    assert abs(area.sum() - 1.0) < 1e-13
    nc = (N + 1) * (M + 1)
    centres = mesh.geometry[nc:]
    quads = mesh.cells[0::4]  # bottom triangle (v0, v1, centre) of every square
    assert np.array_equal(quads[:, 2], np.arange(nc, nc + N * M))
    v0 = mesh.geometry[quads[:, 0]]
    np.testing.assert_allclose(centres, v0 + [0.5 / N, 0.5 / M], rtol=0, atol=1e-15)
    coords, cells = R.crossed_unit_square(N, M)
    np.testing.assert_allclose(mesh.geometry, coords, rtol=0, atol=1e-15)
    assert np.array_equal(mesh.cells, cells)


def test_right_diagonal_unchanged():
    a = fem.create_unit_square(4, 3)
    b = fem.create_rectangle(((0.0, 0.0), (1.0, 1.0)), (4, 3))
    assert a.structured == (4, 3) and np.array_equal(a.cells, b.cells) and np.array_equal(a.geometry, b.geometry)


def test_initial_condition_matches_literal_markers():
    mesh = fem.create_unit_square(50, 50, diagonal="crossed")
    nc = 51 * 51
    assert np.any(np.abs(mesh.geometry[nc:, 1] - 0.75) < 1e-14)  # centre vertices on the rectangle's upper edge
    u = multiphase.initial_condition(mesh)
    ref = R.initial_condition_literal(mesh.geometry, mesh.cells)
    assert np.array_equal(u, ref)
    U = u.reshape(-1, 4)
    assert np.array_equal(U.sum(axis=1), np.ones(len(U)))
    assert all(np.any(U[:, m] == 1.0) for m in range(4))


def _moment(p, q):
    from math import factorial

    return factorial(p) * factorial(q) / factorial(p + q + 2)


def test_degree7_rule_exact_and_old_tables_unchanged():
    pts, wts = fem.quadrature_rule("triangle", 7)
    assert len(wts) == 16 and np.all(wts > 0)
    for p in range(8):
        for q in range(8 - p):
            s = float(np.sum(wts * pts[:, 0] ** p * pts[:, 1] ** q))
            assert abs(s - _moment(p, q)) < 1e-15, (p, q)
    tabs = json.loads((ROOT / "proximalgalerkin_amd" / "tables" / "quadrature.json").read_text())
    old = {"tri_deg6_12": "f5614b418b6ddf28491de6122f7a82ff9b0dad242d986f2c6bb9a7ca3b41bdcf",
           "tri_deg10_gj36": "f89addee6a3b744ec672bf7562fd74cce311fb5b47d038d12507ed9662991e7e",
           "tri_deg4_gj9": "d249bb40ba2e2c2fd985c2ff9ed38540a78bd1ce4fbb74370f3662920cd77462",
           "tri_vertex_3": "0af8b39002d9cc1f744c0aa3176fe6649f06fbfecaab19563fc5e79c22688a46",
           "tri_deg6_12_b": "7bd31c5dfdd4087329ec2707b23363e9b5e7028b965ab4ba3a3906d1b055ba61"}
    for k, h in old.items():
        assert hashlib.sha256(json.dumps(tabs[k], sort_keys=True).encode()).hexdigest() == h, k


def test_restatement_jacobian_matches_finite_differences():
    coords, cells = R.crossed_unit_square(3, 2)
    P = R.Multiphase(coords, cells)
    rng = np.random.default_rng(4)
    n = 4 * P.nv
    x = rng.standard_normal(P.ndofs)
    x[2 * n:] = rng.uniform(-30.0, 30.0, n)  # psi spread over +-30
    xk = rng.standard_normal(P.ndofs)
    up = rng.random(n)
    alpha = 2.5
    J = P.jacobian(x, alpha).toarray()
    h = 1e-6
    Jfd = np.empty_like(J)
    for k in range(P.ndofs):
        e = np.zeros(P.ndofs)
        e[k] = h
        Jfd[:, k] = (P.residual(x + e, xk, up, alpha) - P.residual(x - e, xk, up, alpha)) / (2 * h)
    assert np.abs(J - Jfd).max() <= 1e-8 * np.abs(J).max()


def test_restatement_conserves_species_mass():
    coords, cells = R.crossed_unit_square(4, 4)
    masses = []
    newton, lvpp, _ = R.solve(coords, cells, 3, masses=masses)
    m = np.array(masses)
    assert np.all(newton > 0) and np.all(lvpp > 0)
    np.testing.assert_allclose(m, np.broadcast_to(m[0], m.shape), rtol=0, atol=1e-12)


def test_restatement_cubic_backtracking_is_taken():
    coords, cells = R.crossed_unit_square(4, 4)
    lam, cubic = [], []
    newton, lvpp, _ = R.solve(coords, cells, 2, alpha_0=20.0, lambdas=lam, cubic=cubic)
    assert min(lam) < 1.0 and len(cubic) >= 1
    g = np.load(ROOT / "tests" / "golden" / "multiphase_p1_n4_a20_steps2.npz")
    assert np.array_equal(newton, g["newton_its"]) and np.array_equal(lvpp, g["lvpp_its"])


@pytest.mark.parametrize("kw,word", [(dict(cell_type="quadrilateral"), "Circumradius"), (dict(primal_degree=2), "P1")])
def test_refusals_name_the_reason(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        multiphase.solve_problem(N=2, M=2, result_dir=None, num_steps=1, **kw)
