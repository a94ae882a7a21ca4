"""The second stage of the Krylov driver's reductions inside the producer launch (PGX_TICKET_REDUCE; csrc/pgx_kernels.hip: tk_arrive,
tk_finish): the last workgroup to arrive in k_multidot, k_multiaxpy_norm and k_axpy_norms sums the block partials in the shape of the
second-stage kernels and publishes the result, instead of a one-block launch behind them.  An exact transformation: every dot product,
norm and stored vector keeps its bits, so solves with the key off and on agree in their counts and BITWISE in the final iterate.

The hook test drives the two routes side by side on data of its own (include/pgx.h: pgx_reduce_selfcheck) and counts 8-byte words
that differ - results on the device, results sent to the host, the stored w'.  The data changes with every repetition, so a partial
left over from the repetition before is a wrong value."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
_RUNS = {}
_HOOK = {}

# (512, 512) P1: n = 263 169 vertices, 2 n = 526 338 entries
LENGTHS = [2,        # the tail only, one block
           514,      # more than one block
           29346,    # = 2 mod 4: the float basis' tail lane
           524288,   # the dot-product grid exactly at its cap of 1024 blocks
           526338]   # past the cap, with the tail
VECTORS = [1, 2, 9, 16, 17]  # 17: two chunks, the second stage in the last one only


def _hook_problem():
    """One (512, 512) P1 handle for all hook cases; the hook changes no state of it that a solve reads."""
    if "p" not in _HOOK:
        from proximalgalerkin_amd import fem
        from proximalgalerkin_amd.obstacle import setup_problem

        msh = fem.create_rectangle(DOMAIN, (512, 512))
        _HOOK["p"] = setup_problem(msh, 1, petsc_options=dict(BASE))[0]
    return _HOOK["p"]


@pytest.mark.parametrize("basis_f32", [False, True], ids=["fp64", "f32"])
@pytest.mark.parametrize("nv", VECTORS)
@pytest.mark.parametrize("length", LENGTHS)
def test_two_launch_and_ticket_routes_agree_word_for_word(require_gpu, length, nv, basis_f32):
    problem = _hook_problem()
    assert 2 * 513 * 513 == 526338
    bad = problem.reduce_selfcheck(nv, length, basis_f32=basis_f32, reps=50, seed=1 + length + 1000 * nv)
    print(f"len {length}, {nv} vectors, {'float' if basis_f32 else 'fp64'} basis, 50 repetitions: {bad} words differ")
    assert bad == 0


def test_hook_refuses_lengths_beyond_the_handle(require_gpu):
    problem = _hook_problem()
    with pytest.raises(Exception):
        problem.reduce_selfcheck(1, 526340)
    with pytest.raises(Exception):
        problem.reduce_selfcheck(1, 3)


def _solve(cells, tuning, degree=1, opts=None):
    """One settings-B LVPP run (as tests/test_gpu_krylov_passes.py) -> final iterate, Newton counts and linear iterations per proximal
    step.  Runs are kept: a configuration that several tests compare against is solved once and never modified."""
    opts = opts or {}
    key = (tuple(cells), degree, tuple(sorted(tuning.items())), tuple(sorted(opts.items())))
    if key in _RUNS:
        return _RUNS[key]
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

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
        problem.close()
    finally:
        for k in tuning:
            _lib.tuning_set(k, None)
    _RUNS[key] = (x, [int(n) for n in hist["Newton steps"]], lin)
    return _RUNS[key]


def _assert_same(a, b, what):
    (xa, na, la), (xb, nb, lb) = a, b
    print(f"{what}: Newton {na} / {nb}, linear iterations {la} / {lb}, "
          f"max |difference| of the iterates {np.max(np.abs(xa - xb)):.3e}")
    assert na == nb, what
    assert la == lb, what
    assert np.array_equal(xa, xb), what


@pytest.mark.parametrize("cells", [(128, 128), (200, 72)])
def test_solves_with_the_key_off_and_on_agree_bitwise(require_gpu, cells):
    _assert_same(_solve(cells, {"PGX_TICKET_REDUCE": 0}), _solve(cells, {}), f"PGX_TICKET_REDUCE 0 / 1, {cells}")


def test_float_basis_solves_agree_bitwise(require_gpu):
    """The float Krylov basis (PGX_V_F32) starts at a vertex count above these grids by default; PGX_V_F32_MIN = 1 takes the solve
    through k_multidot / k_multiaxpy_norm with a float basis and their tickets."""
    on = _solve((128, 128), {"PGX_V_F32_MIN": 1})
    _assert_same(_solve((128, 128), {"PGX_V_F32_MIN": 1, "PGX_TICKET_REDUCE": 0}), on, "float basis, PGX_TICKET_REDUCE 0 / 1")


def test_p2_solve_agrees_bitwise(require_gpu):
    _assert_same(_solve((32, 32), {"PGX_TICKET_REDUCE": 0}, degree=2), _solve((32, 32), {}, degree=2), "P2 (32, 32), PGX_TICKET_REDUCE 0 / 1")


def test_the_key_needs_the_fused_publish(require_gpu):
    """PGX_FUSED_PUBLISH = 0 keeps its meaning - the second stage and k_publish as launches of their own - whatever the new key says."""
    both_off = _solve((128, 128), {"PGX_FUSED_PUBLISH": 0, "PGX_TICKET_REDUCE": 0})
    _assert_same(_solve((128, 128), {"PGX_FUSED_PUBLISH": 0, "PGX_TICKET_REDUCE": 1}), both_off, "PGX_FUSED_PUBLISH 0, PGX_TICKET_REDUCE 1 / 0")
    _assert_same(both_off, _solve((128, 128), {}), "both keys 0 / defaults")
