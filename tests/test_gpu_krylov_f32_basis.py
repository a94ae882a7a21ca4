"""The single-precision Krylov basis of the lean P1 path (csrc/pgx_krylov.hip: fgmres; PGX_V_F32, PGX_V_F32_GAIN, PGX_V_F32_MAX).

The basis vectors are stored as float, w = J z_j stays fp64, dot products and projections are fp64 on the widened basis, and a cycle
ends once its Arnoldi estimate has gained PGX_V_F32_GAIN over the true residual it started from (the loop head then takes the true
residual in fp64).  Against the fp64 basis (PGX_V_F32=0) the Newton counts per proximal step must be equal, the final u must agree to
a relative L2 of 1e-10 (the project's bar; the CPU twin tools/krylov_f32_basis_study.py shows 3e-12) and the linear iterations may
grow by at most 15 % (the twin: +6 %, with a margin for the float kernels' own instruction order).

By default the float basis is in force from PGX_V_F32_MIN = 10^6 vertices up; every run of this file sets that key to 0, so that the
path runs at these sizes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
F64 = {"PGX_V_F32": 0}
ON = {"PGX_V_F32_MIN": 0}  # by default the float basis starts at 10^6 vertices (where it pays): every run here takes it from any size
_RUNS = {}


def _solve(cells, tuning, opts, degree=1, fresh=False):
    """One settings-B LVPP run (as tests/test_gpu_krylov_passes.py: _solve) -> final iterate, Newton counts and linear iterations per
    proximal step, number of primal unknowns.  Runs are kept: a configuration that several tests compare against is solved once and
    never modified; fresh: solve again whatever is kept (and keep nothing)."""
    key = (tuple(cells), tuple(sorted(tuning.items())), tuple(sorted(opts.items())), degree)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    tuning = dict(ON, **tuning)
    for k, v in tuning.items():
        _lib.tuning_set(k, v)
    try:
        msh = fem.create_rectangle(DOMAIN, cells)
        problem, sol, sol_k, alpha = setup_problem(msh, degree, petsc_options=dict(BASE, **opts))
        lin, inner = [], problem.solve

        def solve():
            inner()
            lin.append(int(problem.solver.getLinearSolveIterations()))

        problem.solve = solve
        hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
        x = sol.x.array.copy()
        x.setflags(write=False)
        nu = int(sol.function_space.block_size)
        problem.close()
    finally:
        for k in tuning:
            _lib.tuning_set(k, None)
    run = (x, [int(n) for n in hist["Newton steps"]], lin, nu)
    if not fresh:
        _RUNS[key] = run
    return run


def _rel_u(a, b):
    nu = a[3]
    return float(np.linalg.norm(a[0][:nu] - b[0][:nu]) / np.linalg.norm(b[0][:nu]))


def _longest(run):
    """A proximal step with `lin` linear iterations over `n` Newton steps has a solve of at least lin / n iterations."""
    return max(-(-lin // n) for lin, n in zip(run[2], run[1]) if n)


def _assert_close(new, ref, what, cap=1.15):
    err = _rel_u(new, ref)
    print(f"{what}: Newton {new[1]} / {ref[1]}, linear iterations {sum(new[2])} / {sum(ref[2])} "
          f"(ratio {sum(new[2]) / sum(ref[2]):.3f}), rel L2 of u {err:.3e}")
    assert new[1] == ref[1], what
    assert err <= 1e-10, (what, err)
    if cap is not None:
        assert sum(new[2]) <= cap * sum(ref[2]), (what, new[2], ref[2])


def _assert_bitwise(a, b, what):
    print(f"{what}: Newton {a[1]} / {b[1]}, linear iterations {sum(a[2])} / {sum(b[2])}, "
          f"max |difference| of the iterates {np.max(np.abs(a[0] - b[0])):.3e}")
    assert a[1] == b[1], what
    assert a[2] == b[2], (what, a[2], b[2])
    assert np.array_equal(a[0], b[0]), what


def test_float_basis_keeps_counts_and_solution_at_128(require_gpu):
    _assert_close(_solve((128, 128), {}, {}), _solve((128, 128), F64, {}), "float / fp64 basis, 128^2")


SMALL = {"PGX_F32_MIN": 500, "PGX_FUSED_MIN": 500}  # the single-precision cycle (and with it the float basis) from 500 vertices up


@pytest.mark.parametrize("cells,restart,tuning", [((32, 32), None, SMALL), ((32, 32), None, {}), ((200, 72), 6, {})])
def test_float_basis_on_grids_that_cut_the_tiles(require_gpu, cells, restart, tuning):
    """32^2: boundary tiles only in the cycle's first launch and in the operator.  By default its finest level (1089 vertices) runs the
    fp64 cycle, which the float basis does not reach, so the grid is also run with the single-precision cycle forced down to it.
    200 x 72: interior and boundary tiles, with restart length 6 (as tests/test_gpu_krylov_passes.py runs that grid), so cycles also
    end at the restart and V_0 = (float)(r / beta) is written for many cycles.  Vector length 2 (nx + 1)(ny + 1) = 2178 and 29346:
    both leave the two-element remainder."""
    opts = {"ksp_gmres_restart": restart} if restart else {}
    new, ref = _solve(cells, tuning, opts), _solve(cells, dict(tuning, **F64), opts)
    _assert_close(new, ref, f"float / fp64 basis, {cells}, {tuning}")
    if tuning or cells != (32, 32):  # the float basis was in force: its rounding moves the iterate in the last bits
        assert not np.array_equal(new[0], ref[0]), "the float basis did not run"


def test_chunks_of_one_to_sixteen_vectors_and_a_remainder_agree_bitwise(require_gpu):
    """PGX_V_F32_GAIN=0: no early cycle end, the estimate stalls near the float floor and the cycles run to the restart (30), so the
    float kernels run at every NV = 1 ... 16 and as 16 + remainder (PGX_GS_WIDE=8: 8 + 8 + remainder, with fp64 w between the chunks)."""
    a = _solve((128, 128), {"PGX_V_F32_GAIN": 0, "PGX_GS_WIDE": 8}, {})
    b = _solve((128, 128), {"PGX_V_F32_GAIN": 0}, {})
    print(f"PGX_V_F32_GAIN=0: Newton {b[1]}, linear iterations {b[2]}: some solve took at least {_longest(b)} iterations")
    _assert_bitwise(a, b, "PGX_GS_WIDE 8 / 16, float basis without early cycle ends")
    assert _longest(b) > 16


def test_float_basis_is_reproducible(require_gpu):
    _assert_bitwise(_solve((128, 128), {}, {}, fresh=True), _solve((128, 128), {}, {}), "float basis, the same run twice")


def test_second_projection_on_the_stored_float_vector(require_gpu):
    """PGX_CGS_ETA2=0.5: the second projection runs whenever the first one removed more than half of |w|^2 - most iterations."""
    _assert_close(_solve((128, 128), {"PGX_CGS_ETA2": 0.5}, {}), _solve((128, 128), {}, {}), "second projection mostly on / default", cap=None)


def test_guard_redoes_the_cycle_with_the_fp64_basis(require_gpu):
    """PGX_V_F32_MAX=0: the first new basis vector of every Newton solve counts as outside the float range, so the solve abandons its
    first cycle after one iteration, redoes it in fp64 from the same residual and stays in fp64: the result is that of PGX_V_F32=0
    bitwise, with one more linear iteration per call of the Newton solver (each runs at least one Newton step)."""
    a = _solve((128, 128), {"PGX_V_F32_MAX": 0}, {})
    b = _solve((128, 128), F64, {})
    extra = sum(a[2]) - sum(b[2])
    print(f"guard: Newton {a[1]} / {b[1]}, linear iterations {sum(a[2])} / {sum(b[2])} (+{extra}), "
          f"max |difference| of the iterates {np.max(np.abs(a[0] - b[0])):.3e}")
    assert a[1] == b[1]
    assert np.array_equal(a[0], b[0])
    assert 0 < extra <= sum(b[1])


@pytest.mark.parametrize("case", ["degree 2", "PGX_MG_F32=0"])
def test_key_does_not_reach_the_other_paths(require_gpu, case):
    if case == "degree 2":
        a, b = _solve((16, 16), {}, {}, degree=2), _solve((16, 16), F64, {}, degree=2)
    else:
        a, b = _solve((64, 64), {"PGX_MG_F32": 0}, {}), _solve((64, 64), {"PGX_MG_F32": 0, "PGX_V_F32": 0}, {})
    _assert_bitwise(a, b, f"PGX_V_F32 1 / 0, {case}")
