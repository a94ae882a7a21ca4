"""Boundary tiles of the six-sweep smoother launches at the full tile height (csrc/pgx_mg32.hip: f_smooth_bnd_full; A/B key
PGX_F32_BND_FULL, default 1, 0 = four-row sub-tiles).  The default path reaches these launches on 1025^2 and 2049^2 only, so - as in
test_gpu_mg32_k6_top.py - PGX_F32_K6_MAX = 2**30 and PGX_F32_MIN = 500 force them onto grids of a few ten thousand vertices, here the
smallest ones on which every kind of boundary tile exists (a tile is 52 columns by PGX_F32_TY rows, its image 64 columns):
  (200, 72)              interior tiles, partial last tile column and row
  (130, 260)             more tile rows than columns
  (124, 124), (256, 256) square; the latter also against the 256^2 golden
  (110, 60)              ny a multiple of 20: the last tile row holds the single grid row ny
  (104, 46)              nx a multiple of 52: the last tile column holds the single grid column nx
  (40, 90)               narrower than one image: the left and the right frame column in the same image, no interior tile
  (90, 30)               no interior tile in either direction, corner tiles only
and those of their coarse levels that keep at least 500 vertices above the fused tail.  The V-cycle is a
preconditioner inside FGMRES: against the fp64 cycle (PGX_MG_F32=0) the Newton counts must be identical and the primal field within
1e-10 (relative L2), the bound of tests/test_gpu_mg32.py.  The new path is not bitwise the sub-tile path - an in-grid vertex next to
the frame now takes the interior tiles' pair-summed row formula where a sub-tile used the seven K / M slots one by one - so against
PGX_F32_BND_FULL=0 the Newton and Krylov counts are asserted and the difference of u is printed; PGX_F32_BND_FULL=0 itself must
reproduce the library before this path existed bit by bit (golden/mg32_bnd_tiles_parent_n200x72_ty20.npz: recorded once on an
MI355X with that library)."""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
HEIGHTS = (8, 12, 16, 20)  # the PGX_F32_TY values the library instantiates for six-sweep launches
GRIDS = [(200, 72), (130, 260), (124, 124), (256, 256), (110, 60), (104, 46), (40, 90), (90, 30)]
# PGX_FUSED_MIN: the single-precision legs start at max(PGX_F32_MIN, PGX_FUSED_MIN) vertices, and PGX_FUSED_MIN defaults to 4000 -
# above the 3731 and 2821 vertices of (40, 90) and (90, 30), which would otherwise run the fp64 cycle and none of these kernels
# PGX_F32_BND_FULL_MIN: whole boundary tiles are the default from 100000 vertices up only (smaller levels are faster with sub-tiles)
K6 = {"PGX_F32_K6_MAX": 2 ** 30, "PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500, "PGX_F32_BND_FULL_MIN": 0}
GOLDEN = pathlib.Path(__file__).parent / "golden"
_cache = {}


def _solve(cells, tuning, again=0):
    """One LVPP run (settings B): (x, Newton counts, Krylov iterations of the last linear solve).  Solves are shared between the
    tests of this module and never modified; `again` asks for a run of its own."""
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


def _check(cells, tuning):
    x64, n64, _ = _solve(cells, {"PGX_MG_F32": 0})
    x, newton, lin = _solve(cells, tuning)
    n = (cells[0] + 1) * (cells[1] + 1)
    err = np.linalg.norm(x[:n] - x64[:n]) / np.linalg.norm(x64[:n])
    print(f"{cells} {tuning}: newton {newton} rel-L2(u) vs fp64 cycle {err:.2e}")
    assert newton == n64, (cells, tuning)
    assert err <= 1e-10, (cells, tuning, err)
    return x, newton, lin


@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", GRIDS)
def test_full_height_boundary_tiles_without_fused_restriction(require_gpu, cells, ty):
    """Three launches per level and cycle; both six-sweep launches of every level run their boundary tiles at full height."""
    x, newton, _ = _check(cells, dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0))
    if cells == (256, 256):
        g = np.load(GOLDEN / "obstacle_p1_n256_settingsB_large.npz")
        u_ref = g["u_final"]
        assert int(g["N"]) == 256 and newton == [int(c) for c in g["hist_Newton_steps"]]
        assert np.linalg.norm(x[: len(u_ref)] - u_ref) <= 1e-10 * np.linalg.norm(u_ref)


@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", GRIDS)
def test_full_height_boundary_tiles_with_fused_restriction(require_gpu, cells, ty):
    """PGX_F32_RR_MAX at its default: the pre-smoothing launch restricts as well; both launches run whole boundary tiles."""
    _check(cells, dict(K6, PGX_F32_TY=ty))


@pytest.mark.parametrize("form", [{"PGX_V_F32_MIN": 0}, {"PGX_V_F32": 0}, {"PGX_LAZY_NORM": 0}])
@pytest.mark.parametrize("ty", HEIGHTS)
@pytest.mark.parametrize("cells", [(200, 72), (256, 256)])
def test_first_launch_input_forms(require_gpu, cells, ty, form):
    """The finest level's first launch reads the Krylov vector as two float fields (IO = 3), as an fp64 pair (IO = 1), or normalised
    in place, and leaves its float2 copy for the launches that follow: the boundary tiles' share of that copy is the new path's."""
    _check(cells, dict(K6, PGX_F32_TY=ty, PGX_F32_RR_MAX=0, **form))


@pytest.mark.parametrize("cells", GRIDS)
def test_against_sub_tiles(require_gpu, cells):
    """Full-height boundary tiles against four-row sub-tiles (PGX_F32_BND_FULL=0) at 20 rows: equal Newton counts and equal Krylov
    iterations of the last linear solve; u is expected to differ in the last bits (order 1e-15 ... 1e-14), which is printed."""
    t = dict(K6, PGX_F32_TY=20, PGX_F32_RR_MAX=0)
    x1, n1, l1 = _check(cells, t)
    x0, n0, l0 = _check(cells, dict(t, PGX_F32_BND_FULL=0))
    n = (cells[0] + 1) * (cells[1] + 1)
    print(f"{cells}: max |u_new - u_old| = {np.abs(x1[:n] - x0[:n]).max():.3e} (max |u| {np.abs(x0[:n]).max():.3e}), "
          f"bitwise equal: {np.array_equal(x1, x0)}; Krylov iterations of the last solve {l1} / {l0}")
    assert n1 == n0
    assert l1 == l0


def test_key_at_zero_is_the_sub_tile_path_bit_by_bit(require_gpu):
    """PGX_F32_BND_FULL=0: two runs are bitwise equal, and equal to what the library computed before the full-height path existed."""
    t = dict(K6, PGX_F32_TY=20, PGX_F32_RR_MAX=0, PGX_F32_BND_FULL=0)
    a, na, la = _solve((200, 72), t)
    b, nb, lb = _solve((200, 72), t, again=1)
    assert na == nb and la == lb
    assert np.array_equal(a, b)
    g = np.load(GOLDEN / "mg32_bnd_tiles_parent_n200x72_ty20.npz")
    assert na == [int(c) for c in g["newton"]] and la == int(g["lin"])
    print(f"max |x - x_parent| = {np.abs(a - g['x']).max():.3e}")
    assert np.array_equal(a, g["x"])
