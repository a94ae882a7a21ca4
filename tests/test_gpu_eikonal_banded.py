"""Example 09 on the band LU (pgx_ek_create_banded, `EikonalProblem(linear_solver="banded")`): the assembly is the dense handle's
to the last bit and only the solver differs; the recorded runs A, B, C (tests/golden/eikonal_*.npz) are reproduced; the 200 x 13
strip, 35 200 unknowns, which the dense LU refuses, takes its first LVPP step as the restatement does; the script's 64 x 8 strip reaches
the distance bound.

The 200 x 13 reference: the restatement's first step solved with scipy's splu is RECORDED (tests/golden/eikonal_200x13_step1.npz,
tools/make_eikonal_step_golden.py: splu takes about 12 s per Newton step there); the same step with LAPACK's dgbtrf in the folded order
plus one refinement step is computed here, and the library may differ from it by ten times the spread between the two."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import _lib, eikonal, lagrange, mesh_generation
from tests import banded_reference as B
from tests import eikonal_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def test_assembly_is_the_dense_handles_and_the_band_is_numpys(require_gpu):
    mesh = mesh_generation.create_mobius_strip(5, 2, 2, 1.0)
    dense, band = eikonal.EikonalProblem(mesh, 5), eikonal.EikonalProblem(mesh, 5, linear_solver="banded")
    try:
        rng = np.random.default_rng(2)
        x, xp = rng.standard_normal(dense.ndofs), rng.standard_normal(dense.ndofs)
        out = []
        for p in (dense, band):
            p.set_state(x)
            p.set_prev(xp)
            p.set_alpha(3.7)
            F, fn = p.residual()
            out.append((F, fn, p.jacobian()))
        (F0, n0, J0), (F1, n1, J1) = out
        assert np.array_equal(F0, F1) and n0 == n1
        assert np.array_equal(J0.indptr, J1.indptr) and np.array_equal(J0.indices, J1.indices) and np.array_equal(J0.data, J1.data)
        st = band.band_stats()
        kl, ku = B.bandwidths(J1, lagrange.band_order_mobius(5, 2))
        print(f"5 x 2: band {st}")
        assert (st["n"], st["kl"], st["ku"], st["bytes"]) == (dense.ndofs, kl, ku, (2 * kl + ku + 1) * dense.ndofs * 8)
        assert kl == ku <= 38 * 2 + 22
        with pytest.raises(_lib.PgxError, match=r"code -5"):  # PGX_ESTATE: a dense handle has no band
            dense.band_stats()
    finally:
        dense.close()
        band.close()


_runs = {}


def _params(g):
    return dict(nu=int(g["nu"]), nv=int(g["nv"]), order=int(g["g"]), nq1=int(g["nq1"]), scale=float(g["scale"]), tol=float(g["tol"]))


def _state(fields):
    return np.concatenate([fields["u"], fields["psi"].ravel()])


def _golden_run(name):
    g = np.load(GOLDEN / f"eikonal_{name}.npz")
    if name not in _runs:
        stats = []
        _runs[name] = eikonal.solve_problem(monitor=lambda p, i: stats.append((p.lu_stats(), p.band_stats())), linear_solver="banded",
                                            **_params(g)) + (stats,)
    return g, _runs[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_banded_run_matches_recorded_run(require_gpu, name):
    g, (fields, log, _) = _golden_run(name)
    print(f"golden {name}, banded: steps (alpha, its, reason) {log[:, 1:4].tolist()}")
    assert np.array_equal(log[:, :4], g["log"]), (log, g["log"])
    d = R.field_differences(len(fields["u"]), _state(fields), g["z"])
    tol = R.field_tolerances(g)
    print(f"golden {name}, banded: (u absolute, psi relative) {d}, tolerance {tol}")
    assert np.all(d <= tol)


def test_banded_run_is_deterministic_and_pivots(require_gpu):
    g, (fields, log, stats) = _golden_run("B")
    fields2, log2 = eikonal.solve_problem(linear_solver="banded", **_params(g))
    assert np.array_equal(log, log2)
    for k in fields:
        assert np.array_equal(fields[k], fields2[k]), k
    lu, band = stats[-1]
    print(f"golden B, last band factorisation: {band}")
    assert (band["n"], band["kl"], band["ku"]) == (944, 174, 174)
    assert band["interchanges"] > 0 and band["zero_pivots"] == 0
    assert all(lu[k] == band[k] for k in ("n", "interchanges", "min_pivot", "max_pivot", "zero_pivots"))


def test_strip_of_200_by_13_takes_its_first_step(require_gpu, monkeypatch):
    g = np.load(GOLDEN / "eikonal_200x13_step1.npz")
    nu, nv, order, nq, tol = int(g["nu"]), int(g["nv"]), int(g["g"]), int(g["nq1"]), float(g["tol"])
    mesh = mesh_generation.create_mobius_strip(nu, nv, order, 1.0)
    with pytest.raises(_lib.PgxError, match="35200"):
        eikonal.EikonalProblem(mesh, nq)
    # the restatement's step with LAPACK's band solve: same (its, reason) as with splu, and the spread between the two
    perm = lagrange.band_order_mobius(nu, nv)
    monkeypatch.setattr(R.spla, "splu", lambda J: B.RefinedBandLU(J, perm))
    P = R.Eikonal(nu, nv, order, nq)
    z0 = np.zeros(P.ndofs)
    zb, reason_b, its_b = P.newton_l2(z0, z0, float(g["alpha"]), atol=tol, rtol=tol, stol=tol)
    assert (its_b, reason_b) == (int(g["its"]), int(g["reason"]))
    spread = R.field_differences(P.n1, zb, g["z"])
    prob = eikonal.EikonalProblem(mesh, nq, petsc_options=eikonal.solver_parameters(tol), linear_solver="banded")
    try:
        st = prob.band_stats()
        assert (st["n"], st["kl"], st["ku"]) == (35200, 38 * nv + 22, 38 * nv + 22)
        prob.set_alpha(float(g["alpha"]))
        reason, its = prob.solve()
        z = prob.get_state()
        lu = prob.lu_stats()
    finally:
        prob.close()
    d = R.field_differences(P.n1, z, zb)
    print(f"200 x 13: its {its} reason {reason}; (u absolute, psi relative) against dgbtrf {d}, splu against dgbtrf {spread}; LU {lu}")
    assert (its, reason) == (int(g["its"]), int(g["reason"]))
    assert lu["zero_pivots"] == 0 and lu["interchanges"] > 0
    assert np.all(d <= 10 * spread), (d, spread)


def test_full_size_reaches_the_distance_bound_banded(require_gpu):
    """the script's size, 64 x 8 (7 104 unknowns): u is the distance to the boundary, at most the half-width 1/4"""
    fields, log = eikonal.solve_problem(linear_solver="banded")
    umax = fields["u"].max()
    print(f"64 x 8 banded: {len(log)} LVPP steps, {int(log[:, 2].sum())} Newton steps, max u {umax:.6f}")
    assert np.all(np.isfinite(_state(fields))) and np.all(np.isfinite(fields["cells"]))
    assert 0.24 < umax <= 0.25 + 1e-3
