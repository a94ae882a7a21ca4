"""LAPACK's band LU (scipy.linalg.lapack.dgbtrf / dgbtrs) as the reference of the banded solver's tests (include/pgx_bd.h).
Test infrastructure only."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
from scipy.linalg import lapack


def bandwidths(A, perm=None):
    """(kl, ku) of the sparse pattern of A[perm][:, perm] (stored entries count, whatever their value)"""
    C = sp.coo_matrix(A)
    if C.nnz == 0:
        return 0, 0
    n = C.shape[0]
    inv = np.arange(n)
    if perm is not None:
        inv = np.empty(n, dtype=np.int64)
        inv[np.asarray(perm)] = np.arange(n)
    d = inv[C.row] - inv[C.col]
    return max(int(d.max()), 0), max(int(-d.min()), 0)


def band_storage(A, kl, ku):
    """LAPACK's dgbtrf input: ab[kl + ku + i - j, j] = A[i, j], (2 kl + ku + 1) x n"""
    C = sp.coo_matrix(A)
    C.sum_duplicates()
    n = C.shape[0]
    ab = np.zeros((2 * kl + ku + 1, n), order="F")
    ab[kl + ku + C.row - C.col, C.col] = C.data
    return ab


class LapackBand:
    """dgbtrf of A[perm][:, perm]; solve() answers in A's numbering.  piv is 0-based."""

    def __init__(self, A, perm=None, kl=None, ku=None):
        A = sp.csr_matrix(A)
        self.n = A.shape[0]
        self.perm = np.arange(self.n) if perm is None else np.asarray(perm, dtype=np.int64)
        P = A[self.perm][:, self.perm]
        wl, wu = bandwidths(P)
        self.kl, self.ku = wl if kl is None else kl, wu if ku is None else ku
        self.lu, self.piv, self.info = lapack.dgbtrf(band_storage(P, self.kl, self.ku), self.kl, self.ku)
        self.diag = np.abs(self.lu[self.kl + self.ku])

    def solve(self, b):
        xb, info = lapack.dgbtrs(self.lu, self.kl, self.ku, np.asarray(b, dtype=np.float64)[self.perm], self.piv)
        assert info == 0
        x = np.empty(self.n)
        x[self.perm] = xb
        return x


class RefinedBandLU:
    """stands where scipy.sparse.linalg.splu does in tests/eikonal_reference.py: LAPACK's band solve in the order `perm_of(n)` plus
    ONE step of iterative refinement (the shared Newton driver of the library refines as well)"""

    def __init__(self, J, perm):
        self.J = sp.csr_matrix(J)
        self.lu = LapackBand(self.J, perm)
        if self.lu.info != 0:
            raise RuntimeError("dgbtrf: exactly singular")

    def solve(self, b):
        x = self.lu.solve(b)
        return x + self.lu.solve(b - self.J @ x)
