"""The band LU with partial pivoting (include/pgx_bd.h, `direct.BandedSolver`) against LAPACK's dgbtrf / dgbtrs on the same band
(tests/banded_reference.py).

Sizes around the panel width nb = 32: n in {1, 2, nb - 1, nb, nb + 1, 2 nb + 2, 4 nb + 1}; bandwidths (kl, ku) in {(0, 0), (0, 3),
(2, 0), (1, 1), (5, 2), (nb - 1, nb + 1), (nb + 3, 7), (n - 1, n - 1)}, clipped to n - 1.  Matrices: (a) a random band; (b) "far
pivot", 0.01 x random with a zero diagonal plus 1.0 at (min(j + kl, n - 1), j): every column interchanges with the bottom of its band
and U fills completely; (c) only the diagonal and the offsets -kl and +ku; (d) matrix (a) scrambled by a random symmetric permutation and
handed over with the inverse as `perm`.  With ku = 0 matrix (b) has an empty first row: it is exactly singular, LAPACK reports it
(info > 0) and so must the solver; (b) is compared as a regular matrix for ku >= 1.

Checks: the pivot vector equals LAPACK's (seeded continuous random values: no ties), interchanges and zero pivots as LAPACK's, the
smallest and largest pivot to rtol 1e-9, kl, ku and bytes as computed in numpy; for two right-hand sides the normwise backward error
|Ax - b| / (|A| |x| + |b|) (2-norms) is at most max(n 2^-52, 10 x what LAPACK's band LU achieves on the same system), the rule of
tests/test_gpu_dense_lu.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import banded_reference as B

pytestmark = pytest.mark.gpu

NB = 32
SIZES = [1, 2, NB - 1, NB, NB + 1, 2 * NB + 2, 4 * NB + 1]


def _bands(n):
    out = []
    for kl, ku in [(0, 0), (0, 3), (2, 0), (1, 1), (5, 2), (NB - 1, NB + 1), (NB + 3, 7), (n - 1, n - 1)]:
        b = (min(kl, n - 1), min(ku, n - 1))
        if b not in out:
            out.append(b)
    return out


def _berr(A, x, b, normA):
    return np.linalg.norm(A @ x - b) / (normA * np.linalg.norm(x) + np.linalg.norm(b))


def _mask(n, kl, ku):
    i, j = np.indices((n, n))
    return (i - j <= kl) & (j - i <= ku)


def _random_band(n, kl, ku, rng):
    return sp.csr_matrix(rng.standard_normal((n, n)) * _mask(n, kl, ku))


def _far_pivot(n, kl, ku, rng):
    A = 0.01 * rng.standard_normal((n, n)) * _mask(n, kl, ku)
    np.fill_diagonal(A, 0.0)
    j = np.arange(n)
    A[np.minimum(j + kl, n - 1), j] += 1.0
    return sp.csr_matrix(A)


def _edges_only(n, kl, ku, rng):
    i, j = np.indices((n, n))
    return sp.csr_matrix(rng.standard_normal((n, n)) * ((i == j) | (i - j == kl) | (j - i == ku)))


def _check_against_lapack(A, kl, ku, perm=None, seed=5):
    """-> (pivots, solutions) of the GPU run; `perm` as handed to the solver, A in the caller's numbering"""
    from proximalgalerkin_amd.direct import BandedSolver

    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    Ad = A.toarray()
    ref = B.LapackBand(A, perm, kl, ku)
    assert ref.info == 0
    bs = BandedSolver(A.indptr, A.indices, perm=perm, device=0)
    try:
        bs.factor(A.data)
        mine = bs.pivots()
        assert np.array_equal(mine, ref.piv), (n, kl, ku, np.flatnonzero(mine != ref.piv)[:8], mine[:8], ref.piv[:8])
        assert np.all(mine >= np.arange(n)) and np.all(mine <= np.arange(n) + kl)
        st = bs.stats()
        assert (st["n"], st["kl"], st["ku"], st["bytes"]) == (n, kl, ku, (2 * kl + ku + 1) * n * 8), st
        assert st["zero_pivots"] == 0 and st["interchanges"] == int(np.count_nonzero(ref.piv != np.arange(n)))
        assert np.isclose(st["min_pivot"], ref.diag.min(), rtol=1e-9) and np.isclose(st["max_pivot"], ref.diag.max(), rtol=1e-9)
        normA = np.linalg.norm(Ad, 2)
        rng = np.random.default_rng(seed)
        xs = []
        for _ in range(2):
            b = rng.standard_normal(n)
            x = bs.solve(b)
            assert np.all(np.isfinite(x))
            want = _berr(Ad, ref.solve(b), b, normA)
            got = _berr(Ad, x, b, normA)
            print(f"n={n} kl={kl} ku={ku} backward error {got:.3e} (LAPACK {want:.3e})")
            assert got <= max(n * 2.0 ** -52, 10 * want), (n, kl, ku, got, want)
            xs.append(x)
        return mine, xs
    finally:
        bs.close()


@pytest.mark.parametrize("n", SIZES)
def test_random_band(require_gpu, n):
    for kl, ku in _bands(n):
        _check_against_lapack(_random_band(n, kl, ku, np.random.default_rng(1000 * n + 10 * kl + ku)), kl, ku)


@pytest.mark.parametrize("n", SIZES)
def test_far_pivot_interchanges_every_column_and_fills_u(require_gpu, n):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.direct import BandedSolver

    for kl, ku in _bands(n):
        if kl < 1:
            continue
        A = _far_pivot(n, kl, ku, np.random.default_rng(2000 * n + 10 * kl + ku))
        if ku == 0:  # an empty first row: exactly singular, for LAPACK and for the solver
            assert B.LapackBand(A, None, kl, ku).info > 0
            bs = BandedSolver(A.indptr, A.indices, device=0)
            try:
                with pytest.raises(_lib.PgxError, match="singular"):
                    bs.factor(A.data)
                assert bs.stats()["zero_pivots"] > 0
            finally:
                bs.close()
            continue
        piv, _ = _check_against_lapack(A, kl, ku)
        # every column whose band reaches its full depth pivots on the bottom of the band; the last kl columns share row n - 1 for
        # their 1.0, so only LAPACK's vector (checked above) says what they do
        j = np.arange(max(n - kl, 0))
        assert np.array_equal(piv[:len(j)], j + kl), (n, kl, ku, piv)


@pytest.mark.parametrize("n", SIZES)
def test_diagonal_and_outermost_offsets_only(require_gpu, n):
    for kl, ku in _bands(n):
        A = _edges_only(n, kl, ku, np.random.default_rng(3000 * n + 10 * kl + ku))
        assert A.nnz <= 3 * n
        _check_against_lapack(A, kl, ku)


@pytest.mark.parametrize("n", SIZES)
def test_scrambled_matrix_with_the_inverse_permutation(require_gpu, n):
    for kl, ku in _bands(n):
        rng = np.random.default_rng(1000 * n + 10 * kl + ku)  # matrix (a) of test_random_band
        A = _random_band(n, kl, ku, rng)
        piv, xs = _check_against_lapack(A, kl, ku)
        q = rng.permutation(n)
        S = sp.csr_matrix(A[q][:, q])  # S[i, j] = A[q[i], q[j]]
        perm = np.empty(n, dtype=np.int64)
        perm[q] = np.arange(n)  # S[perm][:, perm] = A
        # the same right-hand sides in S's numbering: _check_against_lapack draws b itself, so scramble through the solver directly
        from proximalgalerkin_amd.direct import BandedSolver

        S.sort_indices()
        bs = BandedSolver(S.indptr, S.indices, perm=perm, device=0)
        try:
            bs.factor(S.data)
            st = bs.stats()
            assert (st["kl"], st["ku"]) == (kl, ku)
            assert np.array_equal(bs.pivots(), piv)
            rhs = np.random.default_rng(5)
            for x in xs:
                b = rhs.standard_normal(n)
                assert np.array_equal(bs.solve(b[q]), x[q])
        finally:
            bs.close()


def test_eikonal_jacobian_in_the_folded_order(require_gpu):
    """example 09's Newton matrix at (16, 4, 3, 6), psi of scale 60: symmetric, zero (u, u) block, 944 unknowns, kl = ku = 174.  A
    symmetric matrix can hold exact ties and a blocked sum rounds differently, so the pivots are only checked for their range."""
    from proximalgalerkin_amd import lagrange
    from proximalgalerkin_amd.direct import BandedSolver
    from tests import eikonal_reference as R

    P = R.Eikonal(16, 4, 3, 6)
    rng = np.random.default_rng(9)
    x = rng.standard_normal(P.ndofs)
    x[P.n1:] = rng.uniform(-60.0, 60.0, 3 * P.n2)
    J = sp.csr_matrix(P.jacobian(x))
    J.sort_indices()
    perm = lagrange.band_order_mobius(16, 4)
    kl, ku = B.bandwidths(J, perm)
    assert kl == ku == 174
    ref = B.LapackBand(J, perm, kl, ku)
    lu = spla.splu(J.tocsc())
    Jd = J.toarray()
    normJ = np.linalg.norm(Jd, 2)
    bs = BandedSolver(J.indptr, J.indices, perm=perm, device=0)
    try:
        bs.factor(J.data)
        piv, st = bs.pivots(), bs.stats()
        n = P.ndofs
        assert np.all(piv >= np.arange(n)) and np.all(piv <= np.minimum(np.arange(n) + kl, n - 1))
        assert (st["kl"], st["ku"], st["zero_pivots"]) == (kl, ku, 0) and st["interchanges"] > 0
        for _ in range(2):
            b = rng.standard_normal(n)
            xg, xl, xs = bs.solve(b), ref.solve(b), lu.solve(b)
            want, got = _berr(Jd, xl, b, normJ), _berr(Jd, xg, b, normJ)
            spread = np.abs(xs - xl).max() / np.abs(xl).max()
            diff = np.abs(xg - xl).max() / np.abs(xl).max()
            print(f"backward error {got:.3e} (dgbtrs {want:.3e}); against dgbtrs {diff:.3e}, splu against dgbtrs {spread:.3e}")
            assert got <= max(n * 2.0 ** -52, 10 * want), (got, want)
            assert diff <= 10 * spread, (diff, spread)
    finally:
        bs.close()


def test_singular_matrix_is_refused_and_the_handle_recovers(require_gpu):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.direct import BandedSolver

    n, kl, ku = 2 * NB + 2, 5, 2
    rng = np.random.default_rng(7)
    good = _random_band(n, kl, ku, rng)
    bs = BandedSolver(good.indptr, good.indices, device=0)
    try:
        bad = good.toarray()
        bad[:, NB + 3] = 0.0  # an all-zero column in the second panel; the pattern keeps its entries
        vals = bad[np.repeat(np.arange(n), np.diff(good.indptr)), good.indices]
        with pytest.raises(_lib.PgxError, match="singular"):
            bs.factor(vals)
        assert bs.stats()["zero_pivots"] > 0
        with pytest.raises(_lib.PgxError, match="zero pivot"):
            bs.solve(np.ones(n))
        bs.factor(good.data)
        assert bs.stats()["zero_pivots"] == 0
        ref = B.LapackBand(good, None, kl, ku)
        assert np.array_equal(bs.pivots(), ref.piv)
        b = rng.standard_normal(n)
        Ad = good.toarray()
        normA = np.linalg.norm(Ad, 2)
        assert _berr(Ad, bs.solve(b), b, normA) <= max(n * 2.0 ** -52, 10 * _berr(Ad, ref.solve(b), b, normA))
    finally:
        bs.close()


def test_two_factorisations_are_bitwise_equal(require_gpu):
    from proximalgalerkin_amd.direct import BandedSolver

    n, kl, ku = 4 * NB + 1, NB + 3, 7
    rng = np.random.default_rng(11)
    A = _random_band(n, kl, ku, rng)
    b = rng.standard_normal(n)
    runs = []
    for _ in range(2):
        bs = BandedSolver(A.indptr, A.indices, device=0)
        out = []
        for _ in range(2):  # twice on one handle, and on a second handle
            bs.factor(A.data)
            out.append((bs.pivots().tobytes(), bs.solve(b).tobytes(), tuple(bs.stats().items())))
        bs.close()
        assert out[0] == out[1]
        runs.append(out[0])
    assert runs[0] == runs[1]


def test_refusals_at_create(require_gpu):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.direct import BandedSolver

    n = BandedSolver.MAX_KL + 2
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[n] = 1
    with pytest.raises(_lib.PgxError, match=f"kl = {n - 1}"):
        BandedSolver(rowptr, np.zeros(1, dtype=np.int32), device=0)
    n = 40000
    rowptr = np.ones(n + 1, dtype=np.int32)
    rowptr[0] = 0
    with pytest.raises(_lib.PgxError, match=f"n = {n}, kl = 0, ku = {n - 1}"):
        BandedSolver(rowptr, np.full(1, n - 1, dtype=np.int32), device=0)
    with pytest.raises(_lib.PgxError, match="permutation"):
        BandedSolver(np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32), perm=[0, 2, 2], device=0)
