"""The banded LU (include/pgx_bd.h) without a GPU: the argument checks that run before any device call, the folded ordering of the
Moebius strip (lagrange.band_order_mobius), and the parity of example 09's restatement when LAPACK's band solve in that ordering,
plus one refinement step, stands where scipy's splu does (what the library computes with linear_solver="banded")."""
import ctypes
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import lagrange
from proximalgalerkin_amd.direct import BandedSolver
from tests import banded_reference as B
from tests import eikonal_reference as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
MAX_KL = BandedSolver.MAX_KL
assert MAX_KL >= 640  # strips up to nv = 16: 38 nv + 22 = 630


def _create(n, rowptr, col, perm=None):
    from proximalgalerkin_amd import _lib

    lib = _lib.load()
    h = _lib._H()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cl = np.ascontiguousarray(col, dtype=np.int32)
    pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    rc = lib.pgx_bd_create(n, _lib.iptr(rp), _lib.iptr(cl) if len(cl) else None, _lib.iptr(pm), 0, None, ctypes.byref(h))
    msg = lib.pgx_bd_last_error(None)
    return rc, (msg.decode() if msg else ""), h


def test_null_arguments():
    from proximalgalerkin_amd import _lib

    lib = _lib.load()
    assert lib.pgx_bd_factor(None, None, 0) == -1
    assert lib.pgx_bd_solve(None, None, None, 0) == -1
    assert lib.pgx_bd_get_stats(None, None) == -1
    assert lib.pgx_bd_export_pivots(None, None) == -1
    assert lib.pgx_bd_timing(None, 0, None, None) == -1
    assert lib.pgx_ek_band_stats(None, None) == -1
    assert lib.pgx_bd_create(2, None, None, None, 0, None, None) == -1
    lib.pgx_bd_destroy(None)


@pytest.mark.parametrize("rowptr,col", [([0, 2, 3], [1, 0, 1]),      # columns of row 0 not increasing
                                        ([0, 1, 2], [0, 2]),         # column out of range
                                        ([0, 2, 1], [0, 1]),         # rowptr not monotone
                                        ([1, 1, 2], [0, 1])])        # rowptr does not start at 0
def test_malformed_pattern_is_refused(rowptr, col):
    rc, msg, h = _create(2, rowptr, col)
    assert rc == -1 and not h and "CSR" in msg


@pytest.mark.parametrize("perm", [[0, 0, 1], [0, 1, 3], [-1, 1, 2]])
def test_perm_that_is_no_permutation_is_refused(perm):
    rc, msg, h = _create(3, [0, 1, 2, 3], [0, 1, 2], perm)
    assert rc == -1 and not h and "permutation" in msg


def test_band_storage_above_the_limit_is_refused_before_anything_is_allocated():
    n = 40000  # the one entry (0, n - 1): ku = n - 1 as a full pattern has, kl = 0; 40 000^2 doubles are 11.9 GiB > 8 GiB
    rowptr = np.ones(n + 1, dtype=np.int32)
    rowptr[0] = 0
    rc, msg, h = _create(n, rowptr, [n - 1])
    print(msg)
    assert rc == -1 and not h
    assert "n = 40000" in msg and "kl = 0" in msg and "ku = 39999" in msg and "GiB" in msg


def test_lower_bandwidth_above_the_limit_is_refused():
    n = MAX_KL + 2  # the one entry (n - 1, 0): kl = MAX_KL + 1
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[n] = 1
    rc, msg, h = _create(n, rowptr, [0])
    print(msg)
    assert rc == -1 and not h
    assert f"n = {n}" in msg and f"kl = {MAX_KL + 1}" in msg and "ku = 0" in msg and "PGX_BD_MAX_KL" in msg
    # kl = MAX_KL passes the argument checks: whatever follows (no device here, or a handle) is not PGX_EINVAL
    rowptr = np.zeros(n, dtype=np.int32)
    rowptr[n - 1] = 1
    rc, msg, h = _create(n - 1, rowptr, [0])
    assert rc != -1, msg
    if h:
        from proximalgalerkin_amd import _lib

        _lib.load().pgx_bd_destroy(h)


@pytest.mark.parametrize("nu,nv", [(8, 2), (16, 4), (64, 8), (3, 1)])
def test_band_order_mobius(nu, nv):
    P = R.Eikonal(nu, nv, 1, 2)  # the pattern depends on neither the geometry order nor the rule
    perm = lagrange.band_order_mobius(nu, nv)
    assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(P.ndofs))
    rng = np.random.default_rng(3)
    J = P.jacobian(rng.standard_normal(P.ndofs))
    kl, ku = B.bandwidths(J, perm)
    print(f"{nu} x {nv}: {P.ndofs} unknowns, kl = {kl}, ku = {ku}, bound {38 * nv + 22}; as numbered {B.bandwidths(J)}")
    assert kl == ku <= 38 * nv + 22


@pytest.mark.parametrize("name", ["A", "C"])
def test_restatement_with_lapack_band_solve_reproduces_the_recorded_run(name, monkeypatch):
    g = np.load(GOLDEN / f"eikonal_{name}.npz")
    nu, nv = int(g["nu"]), int(g["nv"])
    perm = lagrange.band_order_mobius(nu, nv)
    monkeypatch.setattr(R.spla, "splu", lambda J: B.RefinedBandLU(J, perm))  # restored by the fixture
    P = R.Eikonal(nu, nv, int(g["g"]), int(g["nq1"]), scale=float(g["scale"]))
    out = R.solve(P, tol=float(g["tol"]))
    assert np.array_equal(out["log"], g["log"]), (out["log"], g["log"])
    d = R.field_differences(P.n1, out["z"], g["z"])
    tol = R.field_tolerances(g)
    print(f"golden {name} with dgbtrf: (u absolute, psi relative) {d}, tolerance {tol}")
    assert np.all(d <= tol)
