"""The argument checks of the dense LU (include/pgx_dn.h) that run before any device call: no GPU needed."""
import ctypes

import numpy as np
import pytest


def _create(n, rowptr, col):
    from proximalgalerkin_amd import _lib

    lib = _lib.load()
    h = _lib._H()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cl = np.ascontiguousarray(col, dtype=np.int32)
    rc = lib.pgx_dn_create(n, _lib.iptr(rp), _lib.iptr(cl) if len(cl) else None, 0, None, ctypes.byref(h))
    msg = lib.pgx_dn_last_error(None)
    return rc, (msg.decode() if msg else ""), h


def test_order_above_the_limit_is_refused_before_anything_is_allocated():
    n = 32768 + 1
    rc, msg, h = _create(n, np.zeros(n + 1), [])
    assert rc == -1 and not h  # PGX_EINVAL
    assert str(n) in msg and "GiB" in msg


@pytest.mark.parametrize("rowptr,col", [([0, 2, 3], [1, 0, 1]),      # columns of row 0 not increasing
                                        ([0, 1, 2], [0, 2]),         # column out of range
                                        ([0, 2, 1], [0, 1]),         # rowptr not monotone
                                        ([1, 1, 2], [0, 1])])        # rowptr does not start at 0
def test_malformed_pattern_is_refused(rowptr, col):
    rc, msg, h = _create(2, rowptr, col)
    assert rc == -1 and not h and "CSR" in msg


def test_null_arguments():
    from proximalgalerkin_amd import _lib

    lib = _lib.load()
    assert lib.pgx_dn_factor(None, None, 0) == -1
    assert lib.pgx_dn_solve(None, None, None, 0) == -1
    assert lib.pgx_dn_get_stats(None, None) == -1
    assert lib.pgx_dn_export_pivots(None, None) == -1
    lib.pgx_dn_destroy(None)
