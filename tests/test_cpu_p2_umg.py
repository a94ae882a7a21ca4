"""The twin of the P2 patch cycle over the hierarchy of a refined general mesh (tests/p2_umg_reference.py), on the CPU alone: it is
what tests/test_gpu_p2_umg.py holds the device against, so its own claims are checked here.

  * as a preconditioner the multilevel coarse cycle is as good as an exact coarse solve (tools/p2_umg_proto.py measured at most one
    Krylov iteration more on D34 and W4; the bound is 2);
  * the restriction's zeroing of the u rows of Dirichlet vertices is load-bearing: without it the count at least doubles;
  * the device's choice of slots and of the wide set, and the layout scatter_exports gives the two exports."""
import numpy as np
import pytest

from oracle import pg_oracle as O
from tests import p2_cycle_reference as PR
from tests import p2_umg_reference as Q

_runs = {}


def _run(name):
    if name not in _runs:
        msh = Q.build_mesh(name)
        prob = O.ObstacleLagrange(msh.geometry, msh.cells, 2)
        assert np.array_equal(prob.edges, msh.edges()[0])
        _runs[name] = (msh, prob) + Q.record_systems(prob)
    return _runs[name]


@pytest.mark.parametrize("name", ["D34", "W4"])
def test_multilevel_coarse_cycle_is_as_good_as_an_exact_coarse_solve(name):
    """The last system of the settings-B run (alpha = 100), FGMRES to 1e-11."""
    msh, prob, systems, hist = _run(name)
    J, b, alpha = systems[-1]
    assert alpha == 100.0
    its, _ = Q.krylov_count(prob, J, b, msh.hierarchy)
    exact, _ = Q.krylov_count(prob, J, b, msh.hierarchy, coarse="exact")
    print(f"P2UMG twin {name}: {len(systems)} systems, Newton {hist['Newton steps']}; last system: cycle {its}, exact coarse solve {exact}")
    assert exact <= its <= exact + 2 and its < 60, (its, exact)


def test_restriction_without_the_dirichlet_zeroing_at_least_doubles_the_count():
    """create_disk(0.2, refinements=2), system 20 (counted from 0) of the settings-B run."""
    msh, prob, systems, hist = _run("D2")
    assert msh.num_vertices == 1319 and len(systems) > 20
    J, b, alpha = systems[20]
    its, _ = Q.krylov_count(prob, J, b, msh.hierarchy)
    bad, _ = Q.krylov_count(prob, J, b, msh.hierarchy, zero_dirichlet=False, maxit=200)
    print(f"P2UMG twin D2 system 20 (alpha {alpha}): {its} iterations, without the zeroing {bad}")
    assert its < 60 and bad >= 2 * its, (its, bad)


@pytest.mark.parametrize("name,slots,nwide,live", [("D34", 7, 0, None), ("D5", 8, 0, None), ("W4", 8, 1, 9), ("X42", 8, 3, 9),
                                                    ("F12", 8, 1, 13), ("F16", 0, 0, None)])
def test_wide_set_selection(name, slots, nwide, live):
    msh = Q.build_mesh(name)
    edges, nv = msh.edges()[0], msh.num_vertices
    NN, wide = Q.selection(edges, nv)
    deg = Q.vertex_degrees(edges, nv)
    assert NN == slots and len(wide) == nwide
    if nwide:
        assert np.array_equal(wide, np.flatnonzero(deg >= 8))
        assert 1 + deg[wide].max() == live  # 2 * live of the 32 rows of a wide patch hold the star, the others are identity
    else:
        assert deg.max() <= 7 or deg.max() > 15
    NN0, wide0 = Q.selection(edges, nv, wide=False)  # PGX_P2_PATCH_WIDE=0: a mesh that needs the wide set has no patch smoother
    assert len(wide0) == 0 and NN0 == (0 if nwide else slots)


@pytest.mark.parametrize("name", ["W4", "X42", "F12"])
def test_scatter_exports_rebuilds_the_twins_own_table_and_inverses(name):
    """Exports built on the host as the device lays them out (narrow rows of wide vertices -1 with identity inverses, wide stars in 16
    slots) scatter back to the twin's table and to the inverses of the twin's patch matrices."""
    msh, prob, systems, _ = _run(name) if name == "W4" else (Q.build_mesh(name), None, None, None)
    if prob is None:
        prob = O.ObstacleLagrange(msh.geometry, msh.cells, 2)
        rng = np.random.default_rng(3)
        x = np.concatenate([0.1 * rng.standard_normal(prob.n), -np.abs(rng.standard_normal(prob.n)) * 3.0])
        J, alpha = prob.jacobian(x, 10.0).tocsr(), 10.0
    else:
        J, _, alpha = systems[len(systems) // 2]
    ref, Ainv = Q.reference_of_system(prob, J, msh.hierarchy)
    nv, S = prob.nv, ref.NN
    NN, wide = Q.selection(prob.edges, nv)
    assert S == 1 + Q.vertex_degrees(prob.edges, nv).max() > NN == 8
    sel = lambda k, stride: np.concatenate([np.arange(k), stride + np.arange(k)])  # noqa: E731
    pdof = ref.table[:, :NN].astype(np.int32)
    narrow = Ainv[:, sel(NN, S)[:, None], sel(NN, S)[None, :]].copy()
    pdof[wide] = -1
    narrow[wide] = np.eye(2 * NN)
    wdof = np.full((len(wide), Q.WIDE_SLOTS), -1, dtype=np.int32)
    wdof[:, :S] = ref.table[wide]
    Winv = np.tile(np.eye(2 * Q.WIDE_SLOTS), (len(wide), 1, 1))
    Winv[:, sel(S, Q.WIDE_SLOTS)[:, None], sel(S, Q.WIDE_SLOTS)[None, :]] = Ainv[wide]
    Q.check_tables(prob.edges, nv, NN, pdof, wide, wdof)
    table, inv = Q.scatter_exports(nv, pdof, narrow, wide, wdof, Winv)
    assert np.array_equal(table, ref.table) and np.array_equal(inv, Ainv)
    # and the unpivoted elimination the device runs inverts these matrices: the wide ones at P = 2 * 16 as well
    A = ref.patch_matrices()
    gj = PR.gauss_jordan_inverse(A[wide])
    assert np.allclose(gj, Ainv[wide], rtol=1e-9, atol=1e-9 * np.abs(Ainv[wide]).max())
