"""Six smoother sweeps per launch on EVERY single-precision level (csrc/pgx_mg32.hip: k_f_smooth<DT, TY, 6, ...> without the fused
restriction, tile heights 8 / 12 / 16 / 20, boundary sub-tiles of four rows).  The default path reaches these launches on 1025^2
and 2049^2 levels only (and only at 20 rows), so here PGX_F32_K6_MAX = 2**30 and PGX_F32_MIN = 500 force them onto
grids of a few ten thousand vertices that still have every kind of tile: interior tiles (nx >= 110, ny >= 30 at TY = 12, ny >= 46 at
TY = 20), partial last tiles (sides that are no multiples of 52 columns or 12 / 20 rows) and odd coarse sizes.  The V-cycle is a
preconditioner inside FGMRES: against the fp64 cycle (PGX_MG_F32=0) on the same mesh the Newton counts must be identical and the
primal field within 1e-10, the bound of tests/test_gpu_mg32.py."""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
HEIGHTS = (8, 12, 16, 20)  # the PGX_F32_TY values the library instantiates for six-sweep launches
GRIDS = [(200, 72), (130, 260), (330, 118), (124, 124), (256, 256)]
K6 = {"PGX_F32_K6_MAX": 2 ** 30, "PGX_F32_MIN": 500}
_cache = {}


def _solve(cells, tuning):
    """One LVPP run (settings B); solves are shared between the tests of this module and never modified."""
    key = (cells, tuple(sorted(tuning.items())))
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
        x = sol.x.array.copy()
        x.setflags(write=False)
        problem.close()
    finally:
        for k in tuning:
            _lib.tuning_set(k, None)
    _cache[key] = (x, list(hist["Newton steps"]))
    return _cache[key]


def _check(cells, tuning):
    x64, n64 = _solve(cells, {"PGX_MG_F32": 0})
    x, newton = _solve(cells, tuning)
    n = (cells[0] + 1) * (cells[1] + 1)
    err = np.linalg.norm(x[:n] - x64[:n]) / np.linalg.norm(x64[:n])
    print(f"{cells} {tuning}: newton {newton} rel-L2(u) vs fp64 cycle {err:.2e}")
    assert newton == n64, (cells, tuning)
    assert err <= 1e-10, (cells, tuning, err)
    return x, newton


@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", GRIDS)
def test_six_sweep_launches_without_fused_restriction(require_gpu, cells, ty):
    """Three launches per level and cycle: six sweeps from the Krylov vector, residual + restriction, six sweeps on x + P x_c."""
    x, newton = _check(cells, dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0))
    if cells == (256, 256):
        g = np.load(pathlib.Path(__file__).parent / "golden" / "obstacle_p1_n256_settingsB_large.npz")
        u_ref = g["u_final"]
        assert int(g["N"]) == 256 and newton == [int(c) for c in g["hist_Newton_steps"]]
        assert np.linalg.norm(x[: len(u_ref)] - u_ref) <= 1e-10 * np.linalg.norm(u_ref)


@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", [(200, 72), (256, 256)])
def test_six_sweep_launches_with_fused_restriction(require_gpu, cells, ty):
    """PGX_F32_RR_MAX at its default: the pre-smoothing launch restricts as well, the post-smoothing one runs at the level's height."""
    _check(cells, dict(K6, PGX_F32_TY=ty))


@pytest.mark.parametrize("form", [{"PGX_V_F32_MIN": 0}, {"PGX_V_F32": 0}, {"PGX_LAZY_NORM": 0}])
@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", [(200, 72), (256, 256)])
def test_first_launch_input_forms(require_gpu, cells, ty, form):
    """The finest level's first six-sweep launch reads the Krylov vector as two float fields (IO = 3), as an fp64 pair (IO = 1), or
    normalised in place."""
    _check(cells, dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0, **form))


@pytest.mark.parametrize("ty", HEIGHTS)
def test_fp64_result_of_the_last_launch_is_bitwise_the_float2_one(require_gpu, ty):
    """As test_float_storage_of_the_krylov_z_vectors_changes_nothing: a float cast to double and back is the identity."""
    t = dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0)
    a, na = _solve((200, 72), t)
    b, nb = _solve((200, 72), dict(t, PGX_Z_F32=0))
    assert na == nb
    assert np.array_equal(a, b)


@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", GRIDS)
def test_against_two_three_sweep_launches(require_gpu, cells, ty):
    """One six-sweep launch against two three-sweep launches (PGX_F32_K6_MAX = 0), both with the restriction as its own launch.
    NOT bitwise equal, so this asserts equal Newton counts and the 1e-10 bound against the fp64 cycle for both: the per-vertex
    operations are the same only where a vertex sits in the same KIND of tile in both launches.  A six-sweep image has a halo of
    6 instead of 3, so more vertices near the frame fall into boundary sub-tiles, whose rows use the seven K / M slots one by one
    where the interior tiles add the mirrored neighbours first - another rounding.  Measured once on an MI355X, final u against
    final u: max |u6 - u3| between 5.6e-16 and 9.0e-15 at |u| <= 0.5 over the five grids and four heights, never zero."""
    x6, n6 = _check(cells, dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0))
    x3, n3 = _check(cells, {"PGX_F32_K6_MAX": 0, "PGX_F32_MIN": 500, "PGX_F32_TY": ty, "PGX_F32_RR_MAX": 0})
    n = (cells[0] + 1) * (cells[1] + 1)
    print(f"{cells} TY={ty}: max |u6 - u3| = {np.abs(x6[:n] - x3[:n]).max():.3e} (max |u| {np.abs(x3[:n]).max():.3e}), "
          f"bitwise equal: {np.array_equal(x6, x3)}")
    assert n6 == n3
