"""Pins tests/p2_cycle_reference.py, the numpy statement of the P2 two-level preconditioner that tests/test_gpu_p2_cycle_operator.py
holds the device to: against the prototype it restates (oracle/p2_patch_proto.py), against 60-digit inverses, and as a
preconditioner of the oracle's own Newton systems.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import nd_lu as ND
from oracle import pg_oracle as O
from oracle.krylov_proto import fgmres
from oracle.p2_patch_proto import StarSmoother
from tests import p2_cycle_reference as PR

_runs = {}


def _run(N):
    """The oracle's settings-B run on N x N: (prob, iterates, Newton systems (J, b, alpha))."""
    if N not in _runs:
        coords, cells = O.create_rectangle(N, N)
        prob = O.ObstacleLagrange(coords, cells, 2)
        ls = ND.NDLinearSolve(*ND.nodes_of_problem(prob), leaf_nodes=16)
        systems, its = [], []

        def rec(J, b):
            systems.append((J.copy(), b.copy()))
            return ls(J, b)

        O.solve_problem(prob, 100, "double_exponential", 1e2, 1e-4, linear_solve=rec, iterates=its)
        _runs[N] = (prob, its, systems)
    return _runs[N]


def _reference(prob, x, alpha, **kw):
    D = sp.csr_matrix((prob.jacobian_blocks(x), prob.indices_s, prob.indptr_s), shape=(prob.n, prob.n))
    return PR.P2CycleReference(prob.K, prob.M, D, alpha, prob.isbc, prob.edges, prob.nv, **kw)


def _states(its):
    return [(1, 1.0), (len(its) // 2, 10.0), (len(its) - 2, 100.0)]


def test_star_table_and_transfer_are_the_prototypes():
    prob, its, _ = _run(12)
    ref = _reference(prob, its[1], 1.0)
    sm = StarSmoother(prob, prob.jacobian(its[1], 1.0))
    n, NN = prob.n, ref.NN
    assert NN == 7  # the right-diagonal mesh: vertex degree 6
    for v in range(prob.nv):
        mine = ref.table[v][ref.table[v] >= 0]
        theirs = sm.idx[v][(sm.idx[v] >= 0) & (sm.idx[v] < n)]
        assert mine[0] == v == theirs[0] and set(mine) == set(theirs)
    from oracle.p2_patch_proto import p1_to_p2

    assert abs(ref.T - p1_to_p2(prob)).max() == 0.0
    assert PR.patch_slots(7) == 7 and PR.patch_slots(8) == 8 and PR.patch_slots(4) == 7


@pytest.mark.parametrize("which", [0, 1, 2])
def test_sweep_without_rounding_is_the_prototypes_sweep(which):
    """x + omega W sum R^T Ainv R (b - J x) with LAPACK inverses of the reference's patch matrices against StarSmoother.sweep, which
    cuts its patch matrices out of the oracle's Jacobian and pads with identity.  Both invert the same matrices up to a symmetric
    permutation, in float64.  Bound per dof: 1e-12 s_i, s_i = omega sum_j |Ainv_ij| |r_j|, the project's bar for two float64
    evaluations of one formula; measured |diff| / s: 4.9e-16, 3.5e-15, 3.2e-15."""
    prob, its, _ = _run(12)
    k, alpha = _states(its)[which]
    x = its[k]
    J = prob.jacobian(x, alpha)
    ref = _reference(prob, x, alpha)
    assert abs(ref.operator() - J).max() <= 1e-15 * abs(J).max()
    sm = StarSmoother(prob, J)
    rng = np.random.default_rng(3 + which)
    b, x0 = rng.standard_normal(2 * prob.n), rng.standard_normal(2 * prob.n)
    Ainv = np.linalg.inv(ref.patch_matrices())
    r = ref.residual(x0, b)
    z = ref.sweep(x0, r, Ainv, omega=0.8)
    zs = sm.sweep(x0, b, 0.8)
    s, _ = ref.sweep_scales(r, Ainv, omega=0.8)
    ratio = (np.abs(z - zs) / np.maximum(s, 1e-300)).max()
    print(f"SWEEP iterate {k} alpha {alpha}: max |ref - prototype| / s = {ratio:.2e}")
    assert ratio <= 1e-12


@pytest.mark.parametrize("which", [0, 1, 2])
def test_elimination_twin_against_60_digit_inverses(which):
    """e(Y) = max_ij sqrt |A_ii A_jj| |Y_ij - X_ij| against the mpmath inverse X.  With E_p = e(twin of k_patch_invert) the bracket of
    the device test's bound is E_p + 4 eps max_ij sqrt |A_ii A_jj| |X_ij|; the same elimination with other rounding (rows divided by
    the pivot) and LAPACK's pivoted inverse must lie within 16 brackets (measured here on 12 x 12: at most 4.3 and 1.9), and 16
    brackets is what the device's elimination - reciprocal by Newton steps, contracted multiply-adds - is allowed (measured on the
    device: at most 3.1)."""
    prob, its, _ = _run(12)
    k, alpha = _states(its)[which]
    ref = _reference(prob, its[k], alpha)
    A = ref.patch_matrices()
    X = PR.exact_inverse(A)
    resid = np.abs(np.einsum("pij,pjk->pik", A, X[0]) + np.einsum("pij,pjk->pik", A, X[1]) - np.eye(A.shape[1])).max()
    assert resid <= 1e-6  # the 60-digit inverse is one (float64 residual of the product: conditioning times eps)
    Ep = PR.inverse_error(A, PR.gauss_jordan_inverse(A), X)
    bracket = Ep + 4.0 * PR.EPS * PR.inverse_size(A, X)
    other = PR.inverse_error(A, PR.gauss_jordan_inverse_divided(A), X) / bracket
    lapack = PR.inverse_error(A, np.linalg.inv(A), X) / bracket
    print(f"INVERSE iterate {k} alpha {alpha}: max E_p {Ep.max():.2e}; e / bracket: other rounding {other.max():.2f}, LAPACK {lapack.max():.2f}")
    assert other.max() <= 16.0 and lapack.max() <= 16.0
    assert np.all(Ep > 0.0)


def test_packing_statement():
    """The mirrored entries of the symmetric packing are those strictly right of a row's 4-column diagonal block."""
    m = PR.sym_mirrored(14)
    assert m[0, 4] and m[3, 13] and not m[0, 3] and not m[13, 12] and not m[12, 13] and m[11, 12]
    assert m.sum() == 14 * 14 - sum(4 * (i // 4 + 1) if 4 * (i // 4 + 1) <= 14 else 14 for i in range(14))


def test_cycle_is_linear_in_b():
    """Without the float stash the cycle is a fixed linear operator: z(a b1 + c b2) = a z(b1) + c z(b2) to rounding (1e-10 of max |z|;
    the amplification of a rounding error through four sweeps and a V-cycle at alpha 10 is far below the 1e6 this leaves)."""
    prob, its, _ = _run(16)
    k = len(its) // 2
    ref = _reference(prob, its[k], 10.0, grid=(16, 16))
    Ainv = PR.gauss_jordan_inverse(ref.patch_matrices())
    rng = np.random.default_rng(8)
    b1, b2 = rng.standard_normal(2 * prob.n), rng.standard_normal(2 * prob.n)
    z1, z2, z12 = (ref.cycle(b, Ainv) for b in (b1, b2, 0.75 * b1 - 2.5 * b2))
    want = 0.75 * z1 - 2.5 * z2
    err = np.abs(z12 - want).max() / np.abs(want).max()
    print(f"LINEAR: {err:.2e}")
    assert err <= 1e-10


def test_reference_cycle_preconditions_the_oracles_newton_systems():
    """FGMRES (oracle/krylov_proto.py) to 1e-10 on every Newton system of the oracle's 16 x 16 settings-B run, preconditioned by the
    reference cycle with the library's defaults (2 sweeps per leg at damping 0.8, V(6, 6) at 0.75 below) against the prototype's
    variant (exact coarse solve, the same sweeps): at most the prototype's count plus MARGIN on every system.  Measured here: the
    counts are printed (`KSP ...`); 8 to 12 iterations, the reference 0 or 1 more than the exact-coarse variant, so MARGIN = 2
    (one more than measured: a count moves by one with the last digit of a residual)."""
    MARGIN = 2
    prob, its, systems = _run(16)
    free = np.flatnonzero(~prob.isbc)[0]  # alpha of a system: from its (1, 1) block, A = alpha K on the free rows
    kdiag = prob.K[free, free]
    worst = -10
    for k, (J, b) in enumerate(systems):
        alpha = J[free, free] / kdiag
        D = -J[prob.n:, prob.n:]
        ref = PR.P2CycleReference(prob.K, prob.M, D, alpha, prob.isbc, prob.edges, prob.nv, grid=(16, 16))
        assert abs(ref.operator() - J).max() <= 1e-13 * abs(J).max()
        Ainv = PR.gauss_jordan_inverse(ref.patch_matrices())
        T2 = sp.block_diag([ref.T, ref.T]).tocsr()
        lu = spla.splu((T2.T @ J @ T2).tocsc())

        def exact_coarse(r):  # run() of oracle/p2_patch_proto.py with these sweeps
            x = np.zeros_like(r)
            for _ in range(ref.patch_nu):
                x = ref.sweep(x, r - J @ x, Ainv)
            x = x + T2 @ lu.solve(T2.T @ (r - J @ x))
            for _ in range(ref.patch_nu):
                x = ref.sweep(x, r - J @ x, Ainv)
            return x

        _, n_ref, _ = fgmres(J, b, lambda r: ref.cycle(r, Ainv), 1e-10, 100)
        _, n_exact, _ = fgmres(J, b, exact_coarse, 1e-10, 100)
        print(f"KSP system {k} alpha {alpha:.3g}: reference cycle {n_ref}, exact coarse solve {n_exact}")
        worst = max(worst, n_ref - n_exact)
        assert n_ref <= n_exact + MARGIN, (k, n_ref, n_exact)
        assert n_exact <= 20  # the prototype's measurement at 16 x 16: 7 to 11 (with damping 1)
    print(f"KSP worst excess {worst}")
