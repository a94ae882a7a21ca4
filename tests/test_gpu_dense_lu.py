"""The dense LU with partial pivoting (include/pgx_dn.h, `direct.DenseSolver`) against LAPACK (`scipy.linalg.lu_factor`).

Sizes around the panel width nb = 64: N in {1, 2, nb - 1, nb, nb + 1, 2 nb + 2, 4 nb + 1}.  Matrices: a permuted identity plus a small
random part with zero diagonal (an interchange in every column but the last, which has no row to exchange with; N = 1 has no
permutation without a fixed point and is the 1 x 1 matrix of the random dense case there), random dense through a full CSR pattern,
a sparse pattern with structurally empty panels, and two Monge-Ampere Jacobians built by tests/monge_ampere_reference.py.

Checks: the LAPACK-style pivot vector equals LAPACK's (the random matrices have no ties); the normwise backward error
|Ax - b| / (|A| |x| + |b|) (2-norms) is at most max(N 2^-52, 10 x what LAPACK's LU achieves on the same matrix and right-hand side) -
LAPACK is the reference, the margin of ten allows for the other summation order of the MFMA update."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

NB = 64
SIZES = [1, 2, NB - 1, NB, NB + 1, 2 * NB + 2, 4 * NB + 1]


def _berr(A, x, b, normA):
    return np.linalg.norm(A @ x - b) / (normA * np.linalg.norm(x) + np.linalg.norm(b))


def _permuted_identity(N, rng):
    if N == 1:
        return sp.csr_matrix(np.array([[rng.uniform(1.0, 2.0)]]))
    A = 0.01 * rng.standard_normal((N, N))
    np.fill_diagonal(A, 0.0)
    A[(np.arange(N) + 1) % N, np.arange(N)] += 1.0  # column j: its large entry in row j + 1
    M = sp.csr_matrix(A)
    assert np.all(M.diagonal() == 0.0)
    return M


def _random_dense(N, rng):
    return sp.csr_matrix(rng.standard_normal((N, N)))


def _empty_panels(N, rng):
    """dense diagonal blocks of 40 rows (not a multiple of the panel width) and a border of 3 dense rows and columns: every panel's
    L21 and U12 are structurally zero outside its own blocks and the border"""
    A = np.zeros((N, N))
    for s in range(0, N, 40):
        e = min(s + 40, N)
        A[s:e, s:e] = rng.standard_normal((e - s, e - s))
    A[-3:, :] = rng.standard_normal(A[-3:, :].shape)
    A[:, -3:] = rng.standard_normal(A[:, -3:].shape)
    return sp.csr_matrix(A)


def _check_against_lapack(A, seed=5, expect_interchanges=False):
    from proximalgalerkin_amd.direct import DenseSolver

    A = sp.csr_matrix(A)
    A.sort_indices()
    N = A.shape[0]
    Ad = A.toarray()
    lu, piv = sla.lu_factor(Ad)
    ds = DenseSolver(A.indptr, A.indices, device=0)
    try:
        ds.factor(A.data)
        mine = ds.pivots()
        assert np.array_equal(mine, piv), (np.flatnonzero(mine != piv)[:8], mine[:8], piv[:8])
        st = ds.stats()
        assert st["n"] == N and st["zero_pivots"] == 0
        assert st["interchanges"] == int(np.count_nonzero(piv != np.arange(N)))
        if expect_interchanges:
            assert np.all(mine[:-1] != np.arange(N - 1))
        d = np.abs(np.diag(lu))
        assert np.isclose(st["min_pivot"], d.min(), rtol=1e-9) and np.isclose(st["max_pivot"], d.max(), rtol=1e-9)
        normA = np.linalg.norm(Ad, 2)
        rng = np.random.default_rng(seed)
        for _ in range(2):
            b = rng.standard_normal(N)
            x = ds.solve(b)
            assert np.all(np.isfinite(x))
            ref = _berr(Ad, sla.lu_solve((lu, piv), b), b, normA)
            got = _berr(Ad, x, b, normA)
            print(f"N={N} backward error {got:.3e} (LAPACK {ref:.3e})")
            assert got <= max(N * 2.0 ** -52, 10 * ref), (got, ref)
    finally:
        ds.close()


@pytest.mark.parametrize("N", SIZES)
def test_permuted_identity_interchanges_every_column(require_gpu, N):
    _check_against_lapack(_permuted_identity(N, np.random.default_rng(100 + N)), expect_interchanges=N > 1)


@pytest.mark.parametrize("N", SIZES)
def test_random_dense(require_gpu, N):
    _check_against_lapack(_random_dense(N, np.random.default_rng(200 + N)))


@pytest.mark.parametrize("N", SIZES)
def test_sparse_pattern_with_empty_panels(require_gpu, N):
    A = _empty_panels(N, np.random.default_rng(300 + N))
    if N > 2 * NB:
        assert A.nnz < 0.5 * N * N
    _check_against_lapack(A)


@pytest.mark.parametrize("case", ["golden_c_first_state", "n2_k3"])
def test_monge_ampere_jacobian(require_gpu, case):
    from tests import monge_ampere_reference as R

    if case == "golden_c_first_state":  # n = 2, k = 2, nonsmooth: N = 198
        prob = R.MongeAmpere((2, 2), 2, nonsmooth=True)
        expect_n = 198
    else:
        prob = R.MongeAmpere((2, 2), 3)
        expect_n = 358
    z = prob.initial_state()
    J = prob.jacobian(z)
    assert J.shape == (expect_n, expect_n)
    _check_against_lapack(J)


def test_singular_matrix_is_refused_and_the_handle_recovers(require_gpu):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.direct import DenseSolver

    N = 2 * NB + 2
    rng = np.random.default_rng(7)
    good = rng.standard_normal((N, N))
    A = sp.csr_matrix(np.ones((N, N)))  # full pattern; the values decide
    ds = DenseSolver(A.indptr, A.indices, device=0)
    try:
        bad = good.copy()
        bad[:, NB + 3] = 0.0  # an all-zero column in the second panel
        with pytest.raises(_lib.PgxError, match="singular"):
            ds.factor(bad.ravel())
        assert ds.stats()["zero_pivots"] > 0
        with pytest.raises(_lib.PgxError, match="zero pivot"):
            ds.solve(np.ones(N))
        ds.factor(good.ravel())
        assert ds.stats()["zero_pivots"] == 0
        b = rng.standard_normal(N)
        x = ds.solve(b)
        assert np.linalg.norm(good @ x - b) <= 1e-10 * np.linalg.norm(b) * np.linalg.cond(good)
        assert np.array_equal(ds.pivots(), sla.lu_factor(good)[1])
    finally:
        ds.close()


def test_order_above_the_limit_is_refused_at_create(require_gpu):
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.direct import DenseSolver

    n = DenseSolver.MAX_N + 1
    with pytest.raises(_lib.PgxError, match=str(n)):
        DenseSolver(np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), device=0)


def test_two_factorisations_are_bitwise_equal(require_gpu):
    from proximalgalerkin_amd.direct import DenseSolver

    N = 4 * NB + 1
    rng = np.random.default_rng(11)
    A = sp.csr_matrix(rng.standard_normal((N, N)))
    b = rng.standard_normal(N)
    runs = []
    for _ in range(2):
        ds = DenseSolver(A.indptr, A.indices, device=0)
        out = []
        for _ in range(2):  # twice on one handle, and on a second handle
            ds.factor(A.data)
            out.append((ds.pivots().tobytes(), ds.solve(b).tobytes(), tuple(ds.stats().items())))
        ds.close()
        assert out[0] == out[1]
        runs.append(out[0])
    assert runs[0] == runs[1]
