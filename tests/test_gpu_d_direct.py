"""The direct D(psi) path (A/B key PGX_D_DIRECT, default 1; 0 = the launches it replaces): on a single handle of degree 1 with a uniform
finest level, k_resid_fill_grid and the compact frame kernel k_resid_fill_frame store Dh, Dd4 and Dq of level 0 themselves (no
k_csr_to_stencil_h, k_pack_d4, k_f_pack_d there), k_rap7h stores Dq of the level it produces, and the coarsenings onto levels of at
least PGX_RAP_LDS_MIN vertices read their fine stencils from an LDS image (k_rap7h_lds).  Every stored value must be bit for bit
what the replaced launches stored, so everything here is an equality of bits.

Grids (cells), the smallest on which each new code path can go wrong - resid tiles are 32 x 12 interior vertices, the staged
coarsening owns 32 x 8 coarse vertices per workgroup:
  (34, 14)               two resid-tile columns, the second holding a single interior vertex; one full tile row plus one vertex
  (66, 26)               whole 32 x 12 tiles, plus one
  (200, 72), (130, 260)  partial last tiles in both directions; coarsening rectangles partial on three levels; fast interior tiles
  (40, 90), (90, 30)     no interior tile of the operator or smoother in one or both directions
  (256, 256)             also against golden/obstacle_p1_n256_settingsB_large.npz
  (8, 8), (4, 4)         interior smaller than one tile; hierarchy of one or two levels
Tuning sets: the defaults; the sibling tests' PGX_F32_K6_MAX = 2**30, PGX_F32_MIN = PGX_FUSED_MIN = 500, with which several levels carry
Dq at these sizes; that set with PGX_F32_DBF16 = 0 (the float4 form of Dq).  The default PGX_RAP_LDS_MIN lies above every level of
these grids, so VARIANTS forces the threshold to both ends: every coarsening staged (PGX_RAP_LDS_MIN = 0), and none.  The one-
workgroup launch for the small levels (PGX_RAP_SMALL_MAX) was built, measured slower than the launches it replaced and taken out
(tools/experiments/README.md, r11_rap_chain.patch), so there is no such key to force.

golden/d_direct_parent_n200x72.npz: x, Newton counts and linear iterations of (200, 72) with the second tuning set, recorded once
on an MI355X with the library of the commit before this path existed."""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
GRIDS = [(34, 14), (66, 26), (200, 72), (130, 260), (40, 90), (90, 30), (256, 256), (8, 8), (4, 4)]
K6 = {"PGX_F32_K6_MAX": 2 ** 30, "PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500}
TUNINGS = {"defaults": {}, "k6": K6, "k6_float4": dict(K6, PGX_F32_DBF16=0)}
# both sides of the threshold at these sizes (the default lies above every level here)
VARIANTS = {
    "every coarsening staged": {"PGX_RAP_LDS_MIN": 0},
    "plain coarsening launches only": {"PGX_RAP_LDS_MIN": 2 ** 30},
}
GOLDEN = pathlib.Path(__file__).parent / "golden"
_cache = {}


def _solve(cells, tuning, again=0):
    """One LVPP run (settings B): (x, Newton counts, linear iterations).  Solves are shared between the tests of this module and
    never modified; `again` asks for a run of its own."""
    key = (cells, tuple(sorted(tuning.items())), again)
    if key in _cache:
        return _cache[key]
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    for k, v in tuning.items():
        _lib.tuning_set(k, v)
    try:
        msh = fem.create_rectangle(DOMAIN, cells)
        problem, sol, sol_k, alpha = setup_problem(msh, 1, petsc_options=dict(BASE))
        hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
        lin = int(problem.solver.getLinearSolveIterations())
        x = sol.x.array.copy()
        x.setflags(write=False)
        problem.close()
    finally:
        for k in tuning:
            _lib.tuning_set(k, None)
    _cache[key] = (x, list(hist["Newton steps"]), lin)
    return _cache[key]


def _same(a, b, what):
    print(f"{what}: newton {a[1]} / {b[1]}, linear iterations {a[2]} / {b[2]}, max |dx| = {np.abs(a[0] - b[0]).max():.3e}")
    assert a[1] == b[1], what
    assert a[2] == b[2], what
    assert np.array_equal(a[0], b[0]), what


@pytest.mark.parametrize("tuning", list(TUNINGS))
@pytest.mark.parametrize("cells", GRIDS)
def test_direct_path_against_the_replaced_launches(require_gpu, cells, tuning):
    """A/B in one library: PGX_D_DIRECT = 1 (plain coarsening, and every coarsening staged) against PGX_D_DIRECT = 0."""
    t = TUNINGS[tuning]
    old = _solve(cells, dict(t, PGX_D_DIRECT=0))
    _same(_solve(cells, dict(t, PGX_D_DIRECT=1)), old, f"{cells} {tuning}: direct / replaced")
    for what, keys in VARIANTS.items():
        _same(_solve(cells, dict(t, PGX_D_DIRECT=1, **keys)), old, f"{cells} {tuning}: direct, {what} / replaced")
    if cells == (256, 256):
        g = np.load(GOLDEN / "obstacle_p1_n256_settingsB_large.npz")
        u_ref = g["u_final"]
        x, newton, _ = _solve(cells, dict(t, PGX_D_DIRECT=1))
        assert int(g["N"]) == 256 and newton == [int(c) for c in g["hist_Newton_steps"]]
        assert np.linalg.norm(x[: len(u_ref)] - u_ref) <= 1e-10 * np.linalg.norm(u_ref)


@pytest.mark.parametrize("cells", [(200, 72), (40, 90)])
def test_operator_copy_and_csr_rows(require_gpu, cells):
    """pgx_jacobian_fill at a seeded random x (the full fill, with_d = 1: Dd4 of interior and frame, CSR rows of both), then the
    matrix-free apply of a seeded v and the exported CSR values of D: bitwise equal under both key values."""
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import setup_problem

    out = {}
    for direct in (0, 1):
        _lib.tuning_set("PGX_D_DIRECT", direct)
        try:
            msh = fem.create_rectangle(DOMAIN, cells)
            problem, sol, sol_k, alpha = setup_problem(msh)
            n2 = sol.function_space.num_dofs
            rng = np.random.default_rng(11)
            x = rng.standard_normal(n2) * 0.2
            x[n2 // 2:] -= 4.0 * np.abs(rng.standard_normal(n2 // 2))  # psi mostly negative: a few orders of magnitude of exp(psi)
            sol_k.x.array[:] = rng.standard_normal(n2) * 0.2
            alpha.value = 2.5
            v = rng.standard_normal(n2)
            problem.assemble_jacobian(x)
            assert problem.spmv_select() == 1  # the matrix-free apply, which reads Dd4
            y = problem.spmv(v)
            D = problem.export_blocks()[4]
            F, _ = problem.residual(x)  # with_d = 0: the compact frame kernel without D output
            problem.assemble_jacobian(x)
            assert np.array_equal(problem.spmv(v), y)
            out[direct] = (y, D, F)
            problem.close()
        finally:
            _lib.tuning_set("PGX_D_DIRECT", None)
    for k, what in enumerate(("J v", "CSR values of D", "F")):
        print(f"{cells} {what}: max |direct - replaced| = {np.abs(out[1][k] - out[0][k]).max():.3e}")
        assert np.array_equal(out[1][k], out[0][k]), what
    assert np.count_nonzero(out[1][1]) > 0


@pytest.mark.parametrize("direct", [0, 1])
def test_against_the_parent_library(require_gpu, direct):
    """Both key values reproduce, bit by bit, what the library computed before the direct path existed."""
    g = np.load(GOLDEN / "d_direct_parent_n200x72.npz")
    x, newton, lin = _solve((200, 72), dict(K6, PGX_D_DIRECT=direct))
    assert newton == [int(c) for c in g["newton"]] and lin == int(g["lin"])
    print(f"PGX_D_DIRECT={direct}: max |x - x_parent| = {np.abs(x - g['x']).max():.3e}")
    assert np.array_equal(x, g["x"])


def test_default_path_is_repeatable(require_gpu):
    a = _solve((200, 72), {})
    b = _solve((200, 72), {}, again=1)
    _same(a, b, "two runs of the default path")
