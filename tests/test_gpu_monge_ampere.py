"""Example 10 on the GPU (include/pgx_ma.h): the kernels against the numpy restatement tests/monge_ampere_reference.py at random
states that violate the Dirichlet values - residual, every Jacobian entry, spmv, l2_error to relative 1e-12 (the bar of the other
families) at three shapes, each with Psi of scale 0.5 and 20 (at 20, cosh(delta) alone is 2e8 and exp(m + delta) reaches 1e17) - the
symmetry of the (phi, Psi) block, bitwise state moves, and the recorded runs A, B, C through p_refinement /
h_refinement: equal reasons and Newton counts, fields to max(1e-10, 10 x sensitivity).  Each test prints its figures before it asserts."""
import pathlib

import numpy as np
import pytest

from tests import monge_ampere_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
# (n, k, quadrature degree): 49 points; 121 points; 289 points = more than one round of a 256-thread workgroup
SHAPES = [((1, 1), 2, 12), ((3, 2), 4, 20), ((2, 1), 7, 32)]
_cache = {}


def _pair(shape):
    """the GPU problem and the restatement of a shape, built once"""
    from proximalgalerkin_amd import monge_ampere as ma

    if shape not in _cache:
        n, k, deg = shape
        ref = R.MongeAmpere(n, k, deg)
        gpu = ma.setup_problem(n, k, deg)
        assert gpu.ndofs == ref.ndofs and gpu.nq == ref.nq == (deg // 2 + 1) ** 2
        _cache[shape] = (gpu, ref)
    return _cache[shape]


def _state(ref, scale, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(ref.ndofs)
    o = ref.offsets
    x[o[3]:] *= scale  # Psi; u (incl. its Dirichlet dofs), p of order 1: the state violates the boundary values
    return x


@pytest.mark.parametrize("scale", [0.5, 20.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_residual_jacobian_spmv_l2_against_the_restatement(require_gpu, shape, scale):
    gpu, ref = _pair(shape)
    x = _state(ref, scale, 17)
    F, fnorm = gpu.residual(x)
    Fr = ref.residual(x)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(Fr))
    eF = np.abs(F - Fr).max() / np.abs(Fr).max()
    J = gpu.jacobian(x)
    Jr = ref.jacobian(x)
    assert np.all(np.isfinite(J.data))
    eJ = abs(J - Jr).max() / abs(Jr).max()
    # every entry, block by block relative to the block's largest entry (the blocks differ by many orders at Psi scale 20)
    o = ref.offsets
    eB = 0.0
    for i in range(6):
        for j in range(6):
            Br = Jr[o[i]:o[i + 1], o[j]:o[j + 1]]
            Bg = J[o[i]:o[i + 1], o[j]:o[j + 1]]
            if Br.nnz == 0:
                assert Bg.nnz == 0 or abs(Bg).max() == 0.0, (i, j)
                continue
            eB = max(eB, abs(Bg - Br).max() / abs(Br).max())
    v = np.random.default_rng(5).standard_normal(ref.ndofs)
    y, yr = gpu.spmv(v), Jr @ v
    eS = np.abs(y - yr).max() / np.abs(yr).max()
    gpu.set_state(x)
    l2, l2r = gpu.l2_error(), ref.l2_error(x)
    eL = abs(l2 - l2r) / l2r
    print(f"{shape} Psi scale {scale}: residual {eF:.2e}  |F| {abs(fnorm - np.linalg.norm(Fr)) / np.linalg.norm(Fr):.2e}  Jacobian {eJ:.2e} "
          f"(worst block {eB:.2e})  spmv {eS:.2e}  l2_error {eL:.2e}   max |J| {abs(Jr).max():.2e}")
    assert eF <= 1e-12 and abs(fnorm - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
    assert eJ <= 1e-12 and eB <= 1e-12
    assert eS <= 1e-12 and eL <= 1e-12
    # the (phi, Psi) block of the export is symmetric to the last bit
    B = J[o[3]:, o[3]:].toarray()
    assert np.array_equal(B, B.T)
    # Dirichlet contract: identity rows and columns, F[bc] = x_bc - g, the state untouched
    assert np.array_equal(F[ref.bc], x[ref.bc] - ref.g)
    assert np.array_equal(gpu.get_state(), x)


def test_state_moves_are_bitwise(require_gpu):
    gpu, ref = _pair(SHAPES[0])
    x = _state(ref, 0.5, 3)
    gpu.set_state(x)
    assert gpu.get_state().tobytes() == x.tobytes()
    F1, _ = gpu.residual()  # x = None: the state
    F2, _ = gpu.residual(x)
    assert F1.tobytes() == F2.tobytes()


def _levels(g):
    return [((int(n[0]), int(n[1])), int(k), int(q)) for n, k, q in zip(g["n"], g["k"], g["quadrature_degree"])]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_goldens(require_gpu, name):
    from proximalgalerkin_amd import monge_ampere as ma

    g = np.load(GOLDEN / f"monge_ampere_{name}.npz")
    lv = _levels(g)
    assert all(q == 4 * k + 4 for _, k, q in lv)  # the studies' default rule is the recorded one
    if name == "B":  # one degree, the mesh doubling: the h-study
        out = ma.h_refinement(k=lv[0][1], levels=tuple(n for n, _, _ in lv), return_last=True)
    else:  # one mesh, the degrees in turn: the p-study
        out = ma.p_refinement(lv[0][1], lv[-1][1], lv[0][0], nonsmooth=bool(g["nonsmooth"]), return_last=True)
    lu = out["problem"].lu_stats()
    out["problem"].close()
    print(f"golden {name}: reasons {out['reasons']} Newton steps {out['newton_its']} L2 errors {out['errors']}; last LU: {lu}")
    assert out["reasons"] == g["reasons"].tolist() and out["newton_its"] == g["newton_its"].tolist()
    assert np.allclose(out["errors"], g["l2_errors"], rtol=1e-9, atol=0)
    assert lu["zero_pivots"] == 0 and lu["interchanges"] > 0 and lu["n"] == out["ndofs"][-1]
    for i, z in enumerate(out["states"]):
        P = R.MongeAmpere(*_levels(g)[i], nonsmooth=bool(g["nonsmooth"]))
        dd = R.field_differences(P, z, g[f"z{i}"])
        tol = np.maximum(1e-10, 10.0 * g["sensitivity"][i])
        print(f"  level {i}: field differences {dd} (bounds {tol})")
        assert np.all(dd <= tol), (i, dd, tol)


def test_two_runs_of_golden_a_are_bitwise_equal(require_gpu):
    from proximalgalerkin_amd import monge_ampere as ma

    g = np.load(GOLDEN / "monge_ampere_A.npz")
    lv = _levels(g)
    a = ma.p_refinement(lv[0][1], lv[-1][1], lv[0][0])
    b = ma.p_refinement(lv[0][1], lv[-1][1], lv[0][0])
    assert a["newton_its"] == b["newton_its"] and a["errors"] == b["errors"]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["states"], b["states"]))


def test_a_level_that_does_not_converge_raises_with_the_reason(require_gpu):
    from proximalgalerkin_amd import monge_ampere as ma

    with pytest.raises(ma.NotConvergedError, match="reason -5"):
        ma.p_refinement(3, 3, 2, snes_opts={"snes_linesearch_type": "l2", "snes_max_it": 2})
