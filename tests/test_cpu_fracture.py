"""CPU tests of example 03's host side (the native crack mesh, refusals) and of the numpy restatement the GPU tests compare
against (tests/fracture_reference.py): Jacobian against central differences, symmetry, the Dirichlet lifting, and the recorded
runs under tests/golden (tools/make_fracture_golden.py)."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import fracture
from proximalgalerkin_amd.mesh_generation import CRACK_BOUNDARIES, create_crack_mesh
from tests import fracture_reference as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
POLYGON = np.array([(0, 0), (2, 0), (2, 2), (1.01, 2), (1, 1.5), (0.99, 2), (0, 2)], dtype=float)


def _problem(h):
    mesh, (edges, tags), names = create_crack_mesh(h)
    return R.Fracture(mesh.geometry, mesh.cells, R.boundary_vertices(edges, tags, names["topleft"]),
                      R.boundary_vertices(edges, tags, names["topright"]))


@pytest.mark.parametrize("h,nv,nc", [(0.4, None, None), (0.2, 128, 202), (0.1, 479, 853)])
def test_crack_mesh(h, nv, nc):
    mesh, (edges, tags), names = create_crack_mesh(h)
    if nv is not None:
        assert (mesh.num_vertices, mesh.num_cells) == (nv, nc)
    assert list(names) == list(CRACK_BOUNDARIES) and list(names.values()) == list(range(1, 9))
    X = mesh.geometry[mesh.cells]
    a, b = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    area = 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
    assert np.all(area > 0)  # counter-clockwise
    m = int((tags == names["hole"]).sum())
    assert m == max(8, int(np.ceil(2 * np.pi * 0.2 / h)))
    exact = 4.0 - 0.005 - 0.5 * m * 0.2**2 * np.sin(2 * np.pi / m)
    assert abs(area.sum() - exact) <= 1e-12 * exact
    assert np.array_equal(np.unique(mesh.cells), np.arange(mesh.num_vertices))  # no unused point
    # the exterior edges (in exactly one cell) are exactly the tagged ones
    c = mesh.cells.astype(np.int64)
    e = np.sort(np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [2, 0]]]), axis=1)
    uk, cnt = np.unique(e, axis=0, return_counts=True)
    assert cnt.max() == 2
    ext = {tuple(p) for p in uk[cnt == 1]}
    assert ext == {tuple(sorted(p)) for p in edges.tolist()} and len(ext) == len(edges)
    # every tagged edge lies on its named piece of the boundary, is no longer than h, and every piece is covered end to end
    P = mesh.geometry
    for k, name in enumerate(CRACK_BOUNDARIES[:-1]):
        p0, p1 = POLYGON[k], POLYGON[(k + 1) % 7]
        ed = edges[tags == names[name]]
        d = p1 - p0
        for v in np.unique(ed):
            t = (P[v] - p0) @ d / (d @ d)
            assert -1e-14 <= t <= 1 + 1e-14 and np.linalg.norm(p0 + t * d - P[v]) <= 1e-14
        length = np.linalg.norm(P[ed[:, 0]] - P[ed[:, 1]], axis=1)
        assert length.max() <= h * (1 + 1e-12)
        assert abs(length.sum() - np.linalg.norm(d)) <= 1e-13
    hole = np.unique(edges[tags == names["hole"]])
    assert len(hole) == m
    np.testing.assert_allclose(np.hypot(P[hole, 0] - 0.3, P[hole, 1] - 0.3), 0.2, rtol=0, atol=1e-15)
    # the Dirichlet vertex lists of the two top pieces
    left = fracture.boundary_vertices((edges, tags), "topleft", names)
    right = fracture.boundary_vertices((edges, tags), "topright", names)
    assert np.all(P[left, 1] == 2.0) and np.all(P[left, 0] <= 0.99) and np.all(P[right, 1] == 2.0) and np.all(P[right, 0] >= 1.01)
    assert len(left) == len(right) == int(np.ceil(0.99 / h - 1e-12)) + 1
    assert abs(fracture.max_cell_diameter(mesh) - _problem(h).l) <= 1e-15


def test_crack_mesh_refuses_bad_resolution():
    with pytest.raises(ValueError):
        create_crack_mesh(0.0)


def _random_state(P, seed, psi_scale=1.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(P.ndofs)
    x[2 * P.nv:] *= psi_scale
    z_iter = rng.standard_normal(P.ndofs)
    z_prev = rng.random(P.ndofs)
    return x, z_iter, z_prev


def test_jacobian_is_the_derivative_of_the_raw_residual():
    P = _problem(0.4)
    x, z_iter, z_prev = _random_state(P, 0)
    alpha, h = 3.7, 1e-6
    J = P.jacobian_raw(x, z_prev, alpha, reps=0.0).toarray()
    Jfd = np.empty_like(J)
    for j in range(P.ndofs):
        d = np.zeros(P.ndofs)
        d[j] = h
        Jfd[:, j] = (P.residual_raw(x + d, z_iter, z_prev, alpha) - P.residual_raw(x - d, z_iter, z_prev, alpha)) / (2 * h)
    err = np.abs(J - Jfd).max() / np.abs(J).max()
    print("central differences: relative error", err)
    # central differences with step h: truncation h^2 |F'''| / 6 ~ 1e-12 |F'''|, rounding ~ 2.2e-16 |F| / h ~ 2e-10 |F|; with
    # |F| and |F'''| within a factor 100 of |J| at this state that is 1e-8 at most; measured 2e-10
    assert err <= 1e-8


def test_regularised_jacobian_is_symmetric_and_carries_reps():
    P = _problem(0.4)
    x, _, z_prev = _random_state(P, 1, psi_scale=3.0)
    J = P.jacobian(x, z_prev, 0.5)
    assert abs(J - J.T).max() <= 1e-14 * abs(J).max()
    bc = P.bc
    D = J.toarray()
    assert np.array_equal(D[bc][:, bc], np.eye(len(bc)))
    assert np.count_nonzero(D[bc]) == len(bc) and np.count_nonzero(D[:, bc]) == len(bc)
    n = P.nv
    diff = (P.jacobian_raw(x, z_prev, 0.5) - P.jacobian_raw(x, z_prev, 0.5, reps=0.0)).toarray()
    M = P.M.toarray()
    ref = np.zeros_like(diff)
    ref[:n, :n], ref[n:2 * n, n:2 * n], ref[2 * n:, 2 * n:] = P.reps * M, P.reps * M, -P.reps * M
    assert np.abs(diff - ref).max() <= 1e-15


def test_lifting_against_a_dense_computation():
    P = _problem(0.4)
    x, z_iter, z_prev = _random_state(P, 2)  # u violates the Dirichlet values
    alpha, T = 3.7, 0.3
    F = P.residual(x, z_iter, z_prev, alpha, T)
    g = np.where(np.isin(P.bc, P.bc_minus), -T, T)
    assert np.array_equal(g, P.g_values(T))
    Jd = P.jacobian_raw(x, z_prev, alpha).toarray()
    ref = P.residual_raw(x, z_iter, z_prev, alpha)
    for j, gj in zip(P.bc, g):
        ref += Jd[:, j] * (gj - x[j])
    ref[P.bc] = x[P.bc] - g
    assert np.linalg.norm(F - ref) <= 1e-13 * np.linalg.norm(ref)
    # R_v is linear in u: there (and only there) lifting equals evaluating at the state with its boundary values imposed,
    # up to the reps M columns of J_reg.  R_d is quadratic in u: imposing the values in the element evaluation is NOT equivalent.
    xg = x.copy()
    xg[P.bc] = g
    Fg = P.residual_raw(xg, z_iter, z_prev, alpha)
    n = P.nv
    free = np.setdiff1d(np.arange(n), P.bc)
    shift = P.reps * (P.M.tocsc()[:, P.bc] @ (g - x[P.bc]))
    assert np.linalg.norm(F[:n][free] - Fg[:n][free] - shift[free]) <= 1e-12 * np.linalg.norm(F[:n][free])
    assert np.linalg.norm(F[n:2 * n] - Fg[n:2 * n]) >= 1e-3 * np.linalg.norm(F[n:2 * n])
    assert np.array_equal(F[2 * n:], Fg[2 * n:])


def test_conforming_damage_is_overflow_free_and_bounded():
    P = _problem(0.4)
    x, _, z_prev = _random_state(P, 3, psi_scale=800.0)
    c = P.conforming_damage(x, z_prev)
    cp = z_prev[P.nv:2 * P.nv][P.cells]
    assert c.shape == (P.nc, 10) and np.all(np.isfinite(c))
    assert np.all(c >= cp.min(axis=1)[:, None] - 1e-15) and np.all(c <= 1.0 + 1e-15)
    assert np.all(np.isfinite(P.residual(x, x, z_prev, 1.0, 0.1))) and np.all(np.isfinite(P.jacobian(x, z_prev, 1.0).data))


def test_recorded_runs_cover_the_branches():
    A, B, C = (np.load(GOLDEN / f"fracture_p1_{k}.npz") for k in "ABC")
    assert A["max_conform"].max() >= 0.9 and int(A["write_frequency"]) > 1
    assert not np.isnan(A["log"][:, 5]).any() and not np.isnan(B["log"][:, 5]).any()
    assert np.isnan(C["log"][:, 5]).sum() >= 1  # a natural failed attempt
    for g in (A, B, C):
        mesh = create_crack_mesh(float(g["h"]))[0]
        assert np.array_equal(mesh.cells, g["cells"]) and np.array_equal(mesh.geometry, g["coords"])


def test_restatement_reproduces_golden_C():
    g = np.load(GOLDEN / "fracture_p1_C.npz")
    P = _problem(float(g["h"]))
    run = R.solve(P, int(g["num_load_steps"]), float(g["Tmin"]), float(g["Tmax"]), write_frequency=int(g["write_frequency"]))
    assert R.logs_agree(run["log"], g["log"])
    assert np.array_equal(run["newton_its"], g["newton_its"]) and np.array_equal(run["lvpp_its"], g["lvpp_its"])
    assert np.all(R.field_differences(P.nv, run["z"], g["z"]) <= R.field_tolerances(g))


def test_logs_agree_rule():
    a = np.array([[0, 1, 1.0, 5, 2, 0.1], [0, 2, 1.0, 44, -9, np.nan], [0, 2, 0.5, 3, 2, 1e-5]])
    b = a.copy()
    b[1, 3:5] = 33, -5  # inside a failing attempt neither the count nor the reason is compared
    assert R.logs_agree(a, b)
    b[2, 3] = 4
    assert not R.logs_agree(a, b)
    b = a.copy()
    b[1, 5] = 0.3  # the fact of failure is
    assert not R.logs_agree(a, b)
    assert not R.logs_agree(a, a[:2])


def test_refusals():
    with pytest.raises(NotImplementedError, match="degree 2"):
        fracture.solve_problem(res=0.4, num_load_steps=2, degree=2)


def test_generate_mesh_script_writes_mesh_and_facets(tmp_path):
    import runpy

    script = pathlib.Path(__file__).resolve().parents[1] / "examples" / "03_fracture" / "generate_mesh.py"
    mod = runpy.run_path(str(script), run_name="generate_mesh")
    mod["main"](["--res", "0.4", "--out", str(tmp_path)])
    mesh, (edges, tags), names = create_crack_mesh(0.4)
    f = np.load(tmp_path / "facets.npz")
    assert np.array_equal(f["edges"], edges) and np.array_equal(f["tags"], tags)
    assert f["names"].tolist() == list(CRACK_BOUNDARIES) and f["values"].tolist() == list(range(1, 9))
    text = (tmp_path / "mesh.vtu").read_text()
    assert f'NumberOfPoints="{mesh.num_vertices}"' in text and f'NumberOfCells="{mesh.num_cells}"' in text
