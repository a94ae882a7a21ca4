"""The numpy twin of example 02 in the plane (tests/signorini2d_reference.py) against what can be known without a GPU: its Jacobian is
the derivative of its residual, rigid motions carry no energy, the coupling integrates the contact length, a linear field gives the
closed-form stress, and EVERY full run tests/test_gpu_signorini2d.py compares against converges (SNES reason > 0 in every proximal
step).  Also the package's host-side plane pieces: node numberings, native tags, and the mesh-file round trip of the half disk."""
import numpy as np
import pytest

from tests import signorini2d_reference as R


@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
def test_jacobian_is_the_derivative_of_the_residual(cell_type, degree):
    prob = R.unit_square(3, 2, cell_type, degree, gap=0.01)
    rng = np.random.default_rng(21)
    x, xk = rng.standard_normal(prob.ntot) * 0.05, rng.standard_normal(prob.ntot) * 0.05
    alpha, h = 2.0, 1e-6
    J = prob.jacobian(x, alpha).toarray()
    Jfd = np.empty_like(J)
    for k in range(prob.ntot):
        e = np.zeros(prob.ntot)
        e[k] = h
        Jfd[:, k] = (prob.residual(x + e, xk, alpha) - prob.residual(x - e, xk, alpha)) / (2 * h)
    # central differences: rounding eps |F| / h ~ 1e-16 * 1e4 / 1e-6 = 1e-6 absolute against |J| ~ alpha E ~ 4e4, i.e. ~ 3e-11 relative;
    # truncation h^2 exp'''/6 ~ 2e-13.  Bound: 1e-8 relative
    assert abs(J - Jfd).max() <= 1e-8 * abs(J).max()


@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
def test_rigid_motions_contact_length_and_linear_field(cell_type, degree):
    prob = R.unit_square(3, 2, cell_type, degree)
    nv, c = prob.nv, prob.coords
    scale = abs(prob.A).max()
    for rm in (np.r_[np.ones(nv), np.zeros(nv)], np.r_[np.zeros(nv), np.ones(nv)], np.r_[-c[:, 1], c[:, 0]]):
        assert abs(prob.A @ rm).max() <= 1e-12 * scale  # two translations and the infinitesimal rotation
    assert abs(prob.MG.sum() - 1.0) <= 1e-13  # the bottom of the unit square
    assert abs(prob.A - prob.A.T).max() <= 1e-12 * scale
    a, b, cc, d = 0.01, -0.02, 0.03, 0.015  # u = (a x + b y, cc x + d y)
    x = np.zeros(prob.ntot)
    x[:nv], x[nv:2 * nv] = a * c[:, 0] + b * c[:, 1], cc * c[:, 0] + d * c[:, 1]
    lm, mu = prob.lmbda, prob.mu
    assert mu == 2.0e4 / 2.6 and lm == 2.0e4 * 0.3 / (1.3 * 0.4)  # the script's constants (:234-235), not plane stress
    sxx, syy, sxy = (lm + 2 * mu) * a + lm * d, lm * a + (lm + 2 * mu) * d, mu * (b + cc)
    m = (sxx + syy) / 3.0  # the script's deviator with len(u) = 2 (:300)
    vm = np.sqrt(1.5 * ((sxx - m) ** 2 + (syy - m) ** 2 + 2 * sxy**2))
    got = prob.von_mises(x)
    assert got.shape == prob.cells.shape and abs(got - vm).max() <= 1e-12 * vm
    # constant stress is in equilibrium: no nodal force at interior nodes
    interior = (c[:, 0] > 1e-9) & (c[:, 0] < 1 - 1e-9) & (c[:, 1] > 1e-9) & (c[:, 1] < 1 - 1e-9)
    assert interior.any()
    f = prob.A @ x[:2 * nv]
    assert abs(f[:nv][interior]).max() <= 1e-12 * scale and abs(f[nv:][interior]).max() <= 1e-12 * scale
    # violation and penetration of a known state: u.n_g - g = 0.002 (1 - 3 x), positive on the first of the three bottom cells only (the
    # kink sits on a cell boundary, so the edge rule integrates max(., 0)^2 exactly): int_0^(1/3) (0.002 (1 - 3 s))^2 ds = 0.002^2 / 9
    prob = R.unit_square(3, 2, cell_type, degree, gap=0.01)
    x = np.zeros(prob.ntot)
    x[nv:2 * nv] = -(c[:, 1] - 0.01) - 0.002 * (1 - 3 * c[:, 0])
    assert abs(prob.violation(x) - 0.002 * (1 - 3 * c[:, 0])).max() <= 1e-15
    assert abs(prob.penetration(x) - 0.002 / 3.0) <= 1e-12 * 0.002


def test_half_disk_contact_length():
    from proximalgalerkin_amd import mesh_generation

    mesh, _, tags = mesh_generation.create_half_disk(**R.HALF_DISK)
    chords = np.linalg.norm(mesh.geometry[tags[2][:, 0]] - mesh.geometry[tags[2][:, 1]], axis=1).sum()
    for degree in (1, 2):
        prob = R.from_triangles(mesh.geometry, mesh.cells, tags[2], tags[1], degree)
        assert abs(prob.MG.sum() - chords) <= 1e-13
        assert 0.0 < np.pi * 0.4 - chords < 0.01  # the polygon inscribed in the half circle
        # the arc's end nodes are also Dirichlet nodes
        assert len(np.intersect1d(prob.cverts, prob.bc_nodes)) == 2


@pytest.mark.parametrize("cell_type,degree", R.FLAVOURS)
@pytest.mark.parametrize("nx,ny,gap", R.SQUARE_RUNS + (R.SYM_RUN[2:], R.CLI_RUN[2:]))
def test_square_runs_of_the_gpu_file_converge_in_the_twin(cell_type, degree, nx, ny, gap):
    prob, x, it, iterations, reasons = R.solved_square(cell_type, degree, nx, ny, gap)
    assert all(r > 0 for r in reasons), (iterations, reasons)
    assert it == len(iterations) < 25
    assert np.all(x[prob.nv + prob.bc_nodes] == -0.25) and np.all(x[prob.bc_nodes] == 0.0)


@pytest.mark.parametrize("degree", [1, 2])
def test_half_disk_runs_of_the_gpu_file_converge_in_the_twin(degree):
    prob, x, it, iterations, reasons = R.solved_half_disk(degree)
    assert all(r > 0 for r in reasons), (iterations, reasons)
    assert it == len(iterations) < 25
    y = prob.coords[prob.cverts, 1] + x[prob.nv + prob.cverts]
    assert (y > 0.05).any() and (abs(y) < 0.05**2 / 0.4).sum() >= 3 and y.min() > -(0.05**2) / 0.4  # partial contact


def test_package_numberings_are_the_twins():
    """p2_nodes_tri, quad_lattice / quad_edge_nodes and native_tags of the package against the twin's independently written mesh
    builders: same nodes, same cells, same contact and displacement nodes."""
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd import signorini as G

    for nx, ny in ((1, 1), (3, 2), (5, 4)):
        mesh = fem.create_unit_square(nx, ny, cell_type="triangle")
        mt, bcs = G.native_tags(mesh)
        assert bcs == {"contact": (2,), "displacement": (1,)}
        coords, cells, bottom, top = R.unit_square_triangles(nx, ny)
        assert np.array_equal(mesh.geometry, coords) and np.array_equal(mesh.cells, cells)
        assert np.array_equal(np.sort(np.sort(mt.find(2), axis=1), axis=0), bottom) and np.array_equal(np.sort(np.sort(mt.find(1), axis=1), axis=0), top)
        c2, cells6, (ce, be) = G.p2_nodes_tri(mesh, mt.find(2), mt.find(1))
        r2, rcells6, (rce, rbe) = R.p2_triangles(coords, cells, bottom, top)
        assert np.array_equal(c2, r2) and np.array_equal(cells6, rcells6)
        assert np.array_equal(np.unique(ce), np.unique(rce)) and np.array_equal(np.unique(be), np.unique(rbe))
        qm = fem.create_unit_square(nx, ny, cell_type="quadrilateral")
        qt, _ = G.native_tags(qm)
        assert qt.find(2).shape == (nx, 2) and qt.find(1).shape == (nx, 2)
        for d in (1, 2):
            qc, qcells = G.quad_lattice(qm, d)
            rc, rcells, rbottom, rtop = R.unit_square_quads(nx, ny, d)
            assert np.array_equal(qc, rc) and np.array_equal(qcells, rcells)
            assert np.array_equal(np.sort(G.quad_edge_nodes(qm, qt.find(2), d), axis=0), rbottom)
            assert np.array_equal(np.sort(G.quad_edge_nodes(qm, qt.find(1), d), axis=0), rtop)


def _write_msh22(path, mesh, tags):
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n%d\n" % len(mesh.geometry))
        for i, p in enumerate(mesh.geometry):
            f.write("%d %.17g %.17g 0\n" % (i + 1, p[0], p[1]))
        n = sum(len(e) for e in tags.values()) + len(mesh.cells)
        f.write("$EndNodes\n$Elements\n%d\n" % n)
        k = 1
        for tag in sorted(tags):
            for a, b in tags[tag]:
                f.write("%d 1 2 %d %d %d %d\n" % (k, tag, tag, a + 1, b + 1))
                k += 1
        for c in mesh.cells:
            f.write("%d 2 2 7 7 %d %d %d\n" % (k, c[0] + 1, c[1] + 1, c[2] + 1))
            k += 1
        f.write("$EndElements\n")


def test_half_disk_round_trip_through_xdmf_and_msh(tmp_path):
    from proximalgalerkin_amd import io, mesh_generation

    mesh, _, tags = mesh_generation.create_half_disk(**R.HALF_DISK)
    io.write_xdmf_tri(tmp_path / "meshes" / "half_disk.xdmf", mesh, tags)
    _write_msh22(tmp_path / "half_disk.msh", mesh, tags)
    for path in (tmp_path / "meshes" / "half_disk.xdmf", tmp_path / "half_disk.msh"):
        m2, mt = io.read_tri_mesh(path)
        assert np.array_equal(m2.geometry, mesh.geometry) and np.array_equal(m2.cells, mesh.cells)
        for tag in (1, 2):
            assert mt.find(tag).shape[1] == 2 and np.array_equal(mt.find(tag), tags[tag])
        assert mt.find(3).shape == (0, 2)
    # a MeshTags goes back out the same way
    io.write_xdmf_tri(tmp_path / "again.xdmf", m2, mt)
    m3, mt3 = io.read_tri_mesh(tmp_path / "again.xdmf")
    assert np.array_equal(m3.cells, mesh.cells) and np.array_equal(mt3.find(2), tags[2])
