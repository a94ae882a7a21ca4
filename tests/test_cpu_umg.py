"""Refined general meshes on the CPU: fem.refine and its hierarchy, the prolongation, and tests/umg_reference.py - the numpy twin the
device cycle is compared with (tests/test_gpu_umg.py) - pinned against the oracle's own matrices."""
import numpy as np
import pytest

from oracle import pg_oracle as O
from proximalgalerkin_amd import fem
from tests import umg_reference as UR

SIZES = {"D5": [227, 64, 20], "D34": [469, 127, 37], "X32": [809, 213, 59, 18]}
MAX_DEGREE = {"D5": 7, "D34": 6, "X32": 8}
_meshes = {}


def _mesh(name):
    if name not in _meshes:
        _meshes[name] = UR.build_mesh(name)
    return _meshes[name]


def _signed_areas(mesh):
    x = mesh.geometry[mesh.cells]
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    return 0.5 * ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))


def _oracle(mesh):
    return O.ObstacleP1(mesh.geometry, mesh.cells, mesh.exterior_vertices())


@pytest.mark.parametrize("snap", [None, 1.0])
def test_refine_counts_orientation_parents_and_snapping(snap):
    coarse = fem.create_disk(0.5)
    assert coarse.hierarchy is None
    nv, nc = coarse.num_vertices, coarse.num_cells
    edges, cell_edges = coarse.edges()
    fine = fem.refine(coarse, snap_radius=snap)
    assert fine.structured is None and fine.num_vertices == nv + len(edges) and fine.num_cells == 4 * nc
    assert np.all(_signed_areas(fine) > 0.0)
    assert np.array_equal(fine.geometry[:nv], coarse.geometry)  # old vertices keep numbers and places
    (par,) = fine.hierarchy
    assert par.dtype == np.int32 and par.shape == (fine.num_vertices, 2)
    assert np.array_equal(par[:nv], np.stack([np.arange(nv)] * 2, axis=1)) and np.array_equal(par[nv:], edges)
    # children of cell c: 4 c + (corner 0, corner 1, corner 2, middle)
    kids = fine.cells.reshape(nc, 4, 3)
    assert np.array_equal(kids[:, 0, 0], coarse.cells[:, 0]) and np.array_equal(kids[:, 1, 1], coarse.cells[:, 1])
    assert np.array_equal(kids[:, 2, 2], coarse.cells[:, 2]) and np.array_equal(kids[:, 3], nv + cell_edges)
    straight = 0.5 * (coarse.geometry[edges[:, 0]] + coarse.geometry[edges[:, 1]])
    ext = np.bincount(cell_edges.ravel(), minlength=len(edges)) == 1
    moved = np.any(fine.geometry[nv:] != straight, axis=1)
    if snap is None:
        assert not moved.any()
    else:
        assert np.array_equal(moved, ext)  # exterior midpoints move onto the circle, and only those
        assert np.max(np.abs(np.hypot(*fine.geometry[nv:][ext].T) - snap)) <= 1e-15
    # the refined mesh's boundary vertices: the coarse ones and the exterior midpoints
    assert np.array_equal(fine.exterior_vertices(), np.concatenate([coarse.exterior_vertices(), nv + np.flatnonzero(ext)]))


@pytest.mark.parametrize("name", sorted(SIZES))
def test_hierarchy_extends_and_table_of_the_test_meshes(name):
    mesh = _mesh(name)
    sizes = [len(p) for p in mesh.hierarchy] + [UR.coarse_sizes(mesh.hierarchy)[-1]]
    assert sizes == SIZES[name]
    assert UR.coarse_sizes(mesh.hierarchy) == SIZES[name][1:]
    assert int(UR.vertex_degrees(mesh).max()) == MAX_DEGREE[name]
    assert fem.create_disk(0.5).hierarchy is None  # refinements=0 is the mesh the function always built


def test_curved_input_is_refined_flat():
    coarse = fem.create_disk(0.5)
    e = coarse.edges()[0]
    mid = 0.5 * (coarse.geometry[e[:, 0]] + coarse.geometry[e[:, 1]])
    mid *= 1.0 + 0.02 * np.hypot(*mid.T)[:, None]
    curved = fem.Mesh(coarse.geometry, coarse.cells, midside=mid)
    assert curved.curved
    a, b = fem.refine(curved), fem.refine(coarse)
    assert not a.curved and np.array_equal(a.geometry, b.geometry) and np.array_equal(a.cells, b.cells)


def test_prolongation_reproduces_affine_functions_on_x32():
    mesh = _mesh("X32")
    coords = [mesh.geometry[:n] for n in SIZES["X32"]]  # nested and unsnapped: a coarse mesh's vertices are the first of the fine one
    for t, par in enumerate(mesh.hierarchy):
        P = UR.prolongation(par, SIZES["X32"][t + 1])
        assert P.shape == (SIZES["X32"][t], SIZES["X32"][t + 1])
        assert np.array_equal(np.diff(P.indptr), np.where(par[:, 0] == par[:, 1], 1, 2))
        for c in ((1.0, 0.0, 0.0), (0.25, -1.5, 0.0), (-0.5, 0.75, 2.0)):
            f = lambda x: c[0] + c[1] * x[:, 0] + c[2] * x[:, 1]
            assert np.max(np.abs(P @ f(coords[t + 1]) - f(coords[t]))) <= 4e-16 * 4.0


def test_twin_products_equal_the_oracle_on_the_coarse_meshes_of_x32():
    """Nested spaces: P^T K P and P^T M P of the oracle's fine matrices ARE the oracle's matrices assembled on the coarse mesh.  Pins
    the numbering and the weights of the transfers independently of the device."""
    chain = [fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), (3, 2), diagonal="crossed")]
    for _ in range(3):
        chain.append(fem.refine(chain[-1]))
    chain = chain[::-1]  # fine -> coarse
    fine = _oracle(chain[0])
    x, _ = UR.state(chain[0].geometry)
    D = fine._scalar_csr(fine.exp_terms(x[fine.n:])[1])
    ref = UR.UmgReference(fine.K, fine.M, D, 2.5, fine.isbc, chain[0].hierarchy)
    assert [L["n"] for L in ref.levels] == SIZES["X32"]
    for l, mesh in enumerate(chain):
        o = _oracle(mesh)
        L = ref.levels[l]
        assert np.array_equal(L["mask"], o.isbc)
        for key, A in (("K", o.K), ("M", o.M)):
            T = L[key]
            assert np.array_equal(T.indptr, A.indptr) and np.array_equal(T.indices, A.indices), (l, key)  # the coarse mesh's P1 pattern
            assert np.max(np.abs(T.data - A.data)) <= 1e-13 * np.max(np.abs(A.data)), (l, key)
        # (scipy's sparse product drops entries that sum to exact zero, so D's stored pattern may lack some of the underflow patch)
        assert abs(L["D"]).sum() > 0 and ((abs(L["D"]) > 0).astype(int) > (abs(o.M) > 0).astype(int)).nnz == 0


def _d5(alpha):
    mesh = _mesh("D5")
    o = _oracle(mesh)
    x, _ = UR.state(mesh.geometry)
    D = o._scalar_csr(o.exp_terms(x[o.n:])[1])
    assert np.count_nonzero(D.data == 0.0) > 0  # the underflow patch is there
    return o, UR.UmgReference(o.K, o.M, D, alpha, o.isbc, mesh.hierarchy)


def test_twin_level_operator_is_the_oracle_jacobian():
    mesh = _mesh("D5")
    o = _oracle(mesh)
    x, _ = UR.state(mesh.geometry)
    D = o._scalar_csr(o.exp_terms(x[o.n:])[1])
    ref = UR.UmgReference(o.K, o.M, D, 2.5, o.isbc, mesh.hierarchy)
    J = o.jacobian(x, 2.5)
    assert abs(ref.matrix(0) - J).max() <= 1e-15 * abs(J).max()


def test_cycle_is_linear():
    _, ref = _d5(2.5)
    rng = np.random.default_rng(5)
    for level in range(3):
        n = ref.n(level)
        b1, b2 = rng.standard_normal(2 * n), rng.standard_normal(2 * n)
        if level:
            b1[:n][ref.levels[level]["mask"]] = b2[:n][ref.levels[level]["mask"]] = 0.0
        z = ref.cycle(level, 0.3 * b1 - 1.7 * b2, nu=2)
        z12 = 0.3 * ref.cycle(level, b1, nu=2) - 1.7 * ref.cycle(level, b2, nu=2)
        assert np.max(np.abs(z - z12)) <= 1e-12 * np.max(np.abs(z))
        both = ref.cycle(level, np.stack([b1, b2], axis=1), nu=2)  # columns at once
        assert np.array_equal(both[:, 0], ref.cycle(level, b1, nu=2))


@pytest.mark.parametrize("alpha", [2.5, 100.0])
def test_cycle_contracts_on_d5(alpha):
    _, ref = _d5(alpha)
    n2 = 2 * ref.n(0)
    B = ref.cycle(0, np.eye(n2), nu=6, omega=0.75)
    rho = np.max(np.abs(np.linalg.eigvals(np.eye(n2) - B @ ref.matrix(0).toarray())))
    print(f"alpha {alpha}: rho(I - B J) = {rho:.4f}")
    assert rho < 1.0
