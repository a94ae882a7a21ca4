"""The hierarchy built from the matrix on the CPU: tests/amg_reference.py - the numpy twin the device is compared with
(tests/test_gpu_amg.py) - checked for soundness of the rule and pinned against the oracle's own matrices and runs.

Meshes (amg_reference.build_mesh), none with a hierarchy: R5 = create_disk(0.5, refinements=2) renumbered by a fixed permutation, 227
vertices; U12 = create_disk(0.12), unrefined, 237 vertices; X32p = the crossed 3 x 2 rectangle refined three times, renumbered, 809
vertices, largest vertex degree 8."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pg_oracle as O
from tests import amg_reference as AR
from tests import umg_reference as UR

MESHES = ("R5", "U12", "X32p")
VERTICES = {"R5": 227, "U12": 237, "X32p": 809}
# Krylov iterations per Newton step of the twin's full run on U12 (settings B; V(6,6), omega 0.75, 60 coarse sweeps), recorded with the
# rule as committed (theta 0.01, Jacobi step, truncation 0.2): mean 5.83
U12_KRYLOV = [6, 6, 6, 6, 6, 6, 6, 6, 6, 5, 6, 6, 5, 6, 5, 6, 6, 6]
_cache = {}


def _setup(name):
    if name not in _cache:
        mesh = AR.build_mesh(name)
        o = O.ObstacleP1(mesh.geometry, mesh.cells, mesh.exterior_vertices())
        Ps, masks = AR.build_hierarchy(o.K, o.isbc)
        _cache[name] = (mesh, o, Ps, masks)
    return _cache[name]


@pytest.mark.parametrize("name", MESHES)
def test_meshes_carry_no_hierarchy_and_coarsen(name):
    mesh, o, Ps, masks = _setup(name)
    assert mesh.hierarchy is None and mesh.num_vertices == VERTICES[name]
    sizes = [Ps[0].shape[0]] + [P.shape[1] for P in Ps]
    print(f"{name}: levels {sizes}, P entries per row {[round(P.nnz / P.shape[0], 2) for P in Ps]}")
    assert len(Ps) >= 1 and all(b <= AR.MAX_KEEP * a for a, b in zip(sizes, sizes[1:]))
    if name == "X32p":
        assert int(UR.vertex_degrees(mesh).max()) == 8
    if name == "R5":  # the same mesh as D5 of tests/umg_reference.py, renumbered: same matrix up to the permutation
        d5 = UR.build_mesh("D5")
        assert np.array_equal(np.sort(np.hypot(*d5.geometry.T)), np.sort(np.hypot(*mesh.geometry.T)))
        assert not np.array_equal(d5.geometry, mesh.geometry)


@pytest.mark.parametrize("name", MESHES)
def test_build_is_deterministic(name):
    _, o, Ps, masks = _setup(name)
    Ps2, masks2 = AR.build_hierarchy(o.K.copy(), o.isbc.copy())
    assert len(Ps) == len(Ps2)
    for P, Q, m, m2 in zip(Ps, Ps2, masks, masks2):
        assert P.indptr.tobytes() == Q.indptr.tobytes() and P.indices.tobytes() == Q.indices.tobytes() and P.data.tobytes() == Q.data.tobytes()
        assert m.tobytes() == m2.tobytes()


@pytest.mark.parametrize("name", MESHES)
def test_rule_is_sound_rows_sum_to_one_every_f_vertex_has_a_c_neighbour_masks(name):
    _, o, Ps, masks = _setup(name)
    K, mask = sp.csr_matrix(o.K), o.isbc
    for t, (P, mask_c) in enumerate(zip(Ps, masks)):
        assert np.max(np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0)) <= 1e-14, (name, t)
        assert AR.c_neighbour_counts(K, mask, P).min() >= 1, (name, t)
        is_c = AR.cf_split(AR.strength(K), mask)
        assert np.array_equal(mask_c, mask[is_c]) and P.shape == (len(mask), int(is_c.sum()))
        # coarse numbering by ascending fine index: the C rows are the unit rows, in order
        assert np.array_equal(P[np.flatnonzero(is_c)].toarray(), np.eye(int(is_c.sum())))
        # a Dirichlet row draws from Dirichlet coarse vertices only
        assert not (P[np.flatnonzero(mask)][:, np.flatnonzero(~mask_c)]).nnz
        # truncation (interior rows; Dirichlet rows keep their direct weights): nothing below TRUNC times the row's largest magnitude is left
        top = abs(P).max(axis=1).toarray().ravel()
        rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        assert np.all((np.abs(P.data) >= AR.TRUNC * top[rows] * (1 - 1e-12)) | mask[rows])
        K, mask = sp.csr_matrix(P.T @ K @ P), mask_c
    assert K.shape[0] <= AR.MIN_COARSE or int(AR.cf_split(AR.strength(K), mask).sum()) > AR.MAX_KEEP * K.shape[0]


def _r5(alpha):
    mesh, o, Ps, masks = _setup("R5")
    x, _ = UR.state(mesh.geometry)
    D = o._scalar_csr(o.exp_terms(x[o.n:])[1])
    assert np.count_nonzero(D.data == 0.0) > 0  # the underflow patch is there
    return o, x, AR.AmgReference(o.K, o.M, D, alpha, o.isbc, Ps, masks)


def test_twin_level_operator_is_the_oracle_jacobian():
    o, x, ref = _r5(2.5)
    J = o.jacobian(x, 2.5)
    assert abs(ref.matrix(0) - J).max() <= 1e-15 * abs(J).max()
    assert [L["n"] for L in ref.levels][0] == 227 and len(ref.levels) >= 2


@pytest.mark.parametrize("alpha", [2.5, 100.0])
def test_cycle_contracts_on_r5(alpha):
    _, _, ref = _r5(alpha)
    n2 = 2 * ref.n(0)
    B = ref.cycle(0, np.eye(n2), nu=6, omega=0.75)
    rho = np.max(np.abs(np.linalg.eigvals(np.eye(n2) - B @ ref.matrix(0).toarray())))
    print(f"alpha {alpha}: rho(I - B J) = {rho:.4f}")
    assert rho < 1.0


def test_u12_run_has_the_lu_oracles_newton_counts_and_the_recorded_krylov_counts():
    _, o, Ps, masks = _setup("U12")
    _, h_lu = O.solve_problem(o, 500, "double_exponential", 1e2, 1e-4)
    stats = []
    _, hist = O.solve_problem(o, 500, "double_exponential", 1e2, 1e-4, linear_solve=AR.make_linear_solve(o, Ps, masks, stats=stats))
    print(f"U12 Newton {list(hist['Newton steps'])}; Krylov per Newton step {stats}, mean {np.mean(stats):.2f}")
    assert [int(v) for v in hist["Newton steps"]] == [int(v) for v in h_lu["Newton steps"]]
    # a change of the rule shows here: every count within 1 of the recorded one
    assert len(stats) == len(U12_KRYLOV) and all(abs(s - r) <= 1 for s, r in zip(stats, U12_KRYLOV)), stats
