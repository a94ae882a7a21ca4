"""tests/vcycle_reference.py pinned without a GPU: against oracle/krylov_proto.py: CollectiveMG on squares, as a linear and convergent
operator on a 24 x 10 rectangle, and its stored-D rule against tools/mg32_study.py: pack_d bit for bit."""
import importlib.util
import pathlib

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_proto as KP
from oracle import pg_oracle as O
from tests import vcycle_reference as VR

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _problem(nx, ny, alpha, seed):
    """(prob, D matrix, x): an obstacle Jacobian at a state whose psi spans several orders of magnitude of exp(psi), with a patch
    inside the grid where exp(psi) underflows to an exact zero."""
    coords, cells = O.create_rectangle(nx, ny)
    prob = O.ObstacleP1(coords, cells, O.boundary_vertices_rectangle(nx, ny))
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(2 * prob.n) * 0.2
    x[prob.n:] -= 4.0 * np.abs(rng.standard_normal(prob.n))
    psi = x[prob.n:].reshape(ny + 1, nx + 1)
    psi[ny // 3: ny // 3 + 4, nx // 3: nx // 3 + 5] -= 800.0
    D = sp.csr_matrix((prob.jacobian_blocks(x), prob.indices_s, prob.indptr_s), shape=(prob.n, prob.n))
    assert (D.data == 0.0).any() and D.diagonal().min() == 0.0
    return prob, D, x


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("N,nu,omega,sweeps", [(16, 2, 0.8, 60), (24, 6, 0.75, 4), (24, 3, 0.75, 7)])
def test_reproduces_collective_mg_on_squares(N, nu, omega, sweeps):
    alpha = 2.5
    prob, D, _ = _problem(N, N, alpha, 3)
    mg = KP.CollectiveMG(prob.K, prob.M, D, alpha, N, prob.isbc, nu=nu, omega=omega, coarse_sweeps=sweeps)
    ref = VR.VCycleReference(prob.K, prob.M, D, alpha, N, N, prob.isbc, min_nx=2, coarse_sweeps=sweeps)
    assert [L["N"] for L in mg.levels] == [L["nx"] for L in ref.levels]
    rng = np.random.default_rng(4)
    for l, L in enumerate(mg.levels):
        assert np.array_equal(L["mask"], ref.levels[l]["mask"]) and np.array_equal(L["mask"], VR.frame_mask(L["N"], L["N"]))
        assert abs(L["D"] - ref.levels[l]["D"]).max() == 0.0
        n = L["A"].shape[0]
        b = rng.standard_normal(2 * n)
        zu, zp = mg.vcycle(b[:n], b[n:], l)
        z = ref.vcycle(b, l, nu=nu, omega=omega)
        assert _rel(z[:n], zu) <= 1e-14 and _rel(z[n:], zp) <= 1e-14, (l, _rel(z[:n], zu), _rel(z[n:], zp))


def _rect_reference(f32_levels=(), dbf16=True):
    alpha = 100.0
    prob, D, x = _problem(24, 10, alpha, 5)
    ref = VR.VCycleReference(prob.K, prob.M, D, alpha, 24, 10, prob.isbc, min_nx=2, coarse_sweeps=4, f32_levels=f32_levels, dbf16=dbf16)
    assert [(L["nx"], L["ny"]) for L in ref.levels] == [(24, 10), (12, 5)]
    return prob, ref, x, alpha


def test_rectangle_operator_is_linear():
    """The cycle is a fixed linear map: B built column by column reproduces the cycle of a combination.  Rounding level: a cycle chains
    2 * 6 + 4 sweeps of 14-term rows and 2 x 2 solves, about 600 roundings of 1.1e-16 on the way to one entry -> 1e-12 of the scale
    |B| (|a| |r1| + |r2|) is a safe bound in float64; the float32 levels give 600 * 6e-8 = 4e-5 -> 1e-4."""
    for f32_levels, mode, tol in (((), "f64", 1e-12), ((0,), "f64", 1e-12), ((0,), "f32", 1e-4)):
        prob, ref, _, _ = _rect_reference(f32_levels)
        n2 = 2 * prob.n
        Bm = np.stack([ref.vcycle(e, mode=mode) for e in np.eye(n2)], axis=1)
        rng = np.random.default_rng(6)
        r1, r2, a = rng.standard_normal(n2), rng.standard_normal(n2), -1.7
        lhs = ref.vcycle(a * r1 + r2, mode=mode)
        scale = np.abs(Bm).sum(axis=1).max() * (abs(a) * np.abs(r1).max() + np.abs(r2).max())
        assert np.abs(lhs - a * (Bm @ r1) - Bm @ r2).max() <= tol * scale
        assert np.abs(lhs - a * ref.vcycle(r1, mode=mode) - ref.vcycle(r2, mode=mode)).max() <= tol * scale


def test_rectangle_cycle_converges_on_the_oracle_jacobian():
    """Its level-0 operator is the oracle's Jacobian, and the spectral radius of I - B J is below 1: the cycle is a convergent
    iteration for the obstacle problem's Newton matrix, in float64 and with the stored (bf16) D in the smoother."""
    for f32_levels in ((), (0,)):
        prob, ref, x, alpha = _rect_reference(f32_levels)
        J = prob.jacobian(x, alpha).toarray()
        if not f32_levels:
            assert np.abs(ref.operator(0).toarray() - J).max() <= 1e-15 * np.abs(J).max()
        n2 = 2 * prob.n
        Bm = np.stack([ref.vcycle(e) for e in np.eye(n2)], axis=1)
        rho = np.abs(np.linalg.eigvals(np.eye(n2) - Bm @ J)).max()
        print(f"f32 levels {f32_levels}: spectral radius of I - B J = {rho:.4f}")
        assert rho < 1.0, rho


def test_float32_mode_differs_by_float_rounding_only():
    prob, ref, _, _ = _rect_reference((0,))
    b = np.random.default_rng(7).standard_normal(2 * prob.n)
    z64, z32 = ref.vcycle(b), ref.vcycle(b, mode="f32")
    e = _rel(z32, z64)
    assert 1e-9 < e < 1e-4, e
    assert ref.levels[0]["op32"]["A"].dtype == np.float32 and "op32" not in ref.levels[1]


def test_float32_dirichlet_rows_as_a_product_with_one_reciprocal():
    """The option that states the kernels' Dirichlet rows: x_u = ((-d) (1 / (-d))) b_u, within two ulp of the float b_u the iterated
    form (MG32) ends at exactly; nothing else changes beyond float rounding."""
    alpha = 100.0
    prob, D, _ = _problem(24, 10, alpha, 5)
    refs = [VR.VCycleReference(prob.K, prob.M, D, alpha, 24, 10, prob.isbc, min_nx=2, f32_levels=(0,), f32_dirichlet_product=on) for on in (True, False)]
    b = np.random.default_rng(9).standard_normal(2 * prob.n)
    z_on, z_off = (r.vcycle(b, mode="f32") for r in refs)
    m = prob.isbc
    bf = b[:prob.n].astype(np.float32)
    assert np.array_equal(z_off[:prob.n][m], bf[m].astype(np.float64))
    d = refs[0].levels[0]["op32"]["d"]
    want = ((-d * (np.float32(1.0) / -d)) * bf)[m]
    assert np.array_equal(z_on[:prob.n][m], want.astype(np.float64))
    assert (np.abs(want - bf[m]) <= 2 * np.spacing(np.abs(bf[m]))).all() and (want != bf[m]).any()
    assert _rel(z_on, z_off) < 1e-6


def test_stored_d_rule_is_pack_d_bit_for_bit():
    spec = importlib.util.spec_from_file_location("mg32_study", ROOT / "tools" / "mg32_study.py")
    study = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(study)
    rng = np.random.default_rng(8)
    x = np.concatenate([np.exp(rng.uniform(-110.0, 80.0, 20000)), [0.0, 1e30, 1.0000001e30, 3e38, 1e300, 1e-46, 1e-40, 1.4e-45],
                        # exact ties of the bf16 rounding, even and odd upper halves
                        np.array([0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F807FFF, 0x00008000, 0x00018000], dtype=np.uint32).view(np.float32)])
    with np.errstate(over="ignore"):  # 1e300 is infinity as a float: the clamp takes it back
        got, want = VR.stored_d(x, True), study.pack_d(x)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(VR.bf16_round(x.astype(np.float32)).view(np.uint32), study.bf16_round(x.astype(np.float32)).view(np.uint32))
        assert (got.view(np.uint32) & np.uint32(0xFFFF) == 0).all()
        assert got.max() == study.bf16_round(np.float32(1e30)) and np.isfinite(got).all()  # (the clamp itself rounds up to 1.00026e30)
        plain = VR.stored_d(x, False)
        assert np.array_equal(plain, np.minimum(x.astype(np.float32), np.float32(1e30)))
