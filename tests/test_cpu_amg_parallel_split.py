"""The parallel form of the C/F split (tests/amg_split_reference.py; the rule csrc/pgx_amg_build.hip's k_ab_split applies) against the
serial greedy pass of tests/amg_reference.py, on every level of the hierarchies of R5, U12, X32p and create_disk(0.03).

The round counts pin the depth of the dependency chains the device meets: a mesh in its generator's order needs about 3.5 sqrt(n)
synchronous rounds, which is why the device reads its termination counter once per batch of launches and not once per round."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pg_oracle as O
from tests import amg_reference as AR
from tests import amg_split_reference as SR

MESHES = ("R5", "U12", "X32p", "disk03")
ROUNDS = {"U12": [51, 22], "disk03": [208, 34, 33]}  # synchronous rounds per transfer
_levels = {}


def _mesh(name):
    from proximalgalerkin_amd import fem

    return fem.create_disk(0.03) if name == "disk03" else AR.build_mesh(name)


def levels(name):
    """[(S, mask, is_c of the serial pass)] per transfer of the hierarchy amg_reference.build_hierarchy builds; computed once."""
    if name not in _levels:
        msh = _mesh(name)
        prob = O.ObstacleP1(msh.geometry, msh.cells, msh.exterior_vertices())
        K, mask = sp.csr_matrix(prob.K), np.asarray(prob.isbc, dtype=bool)
        Ps, masks = AR.build_hierarchy(K, mask)
        out = []
        for P, mask_c in zip(Ps, masks):
            S = AR.strength(K)
            is_c = AR.cf_split(S, mask)
            assert int(is_c.sum()) == P.shape[1]
            out.append((S, mask, is_c))
            K, mask = AR._csr(P.T @ K @ P), mask_c
        _levels[name] = out
    return _levels[name]


@pytest.mark.parametrize("name", MESHES)
def test_synchronous_rounds_reach_the_serial_split(name):
    got = []
    for t, (S, mask, is_c) in enumerate(levels(name)):
        par, rounds = SR.split_rounds(S, mask)
        assert np.array_equal(par, is_c), (name, t)
        assert 1 <= rounds <= S.shape[0]
        got.append(rounds)
    print(f"SPLIT ROUNDS {name}: vertices {[S.shape[0] for S, _, _ in levels(name)]}, rounds {got}")
    if name in ROUNDS:
        assert got == ROUNDS[name], (name, got)


@pytest.mark.parametrize("name", MESHES)
def test_random_order_in_place_sweeps_reach_the_serial_split(name):
    rng = np.random.default_rng(11)
    for t, (S, mask, is_c) in enumerate(levels(name)):
        for _ in range(2):
            par, sweeps = SR.split_in_place(S, mask, rng)
            assert np.array_equal(par, is_c), (name, t)
            assert sweeps <= S.shape[0]
