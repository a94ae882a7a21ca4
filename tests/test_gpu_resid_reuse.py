"""PGX_RESID_REUSE: the entry evaluation of a Newton solve that starts where the converged solve before it ended.

The LVPP loop does sol_k <- sol, changes alpha and solves again from sol.  Of the entry residual only F_u = alpha K u + M (psi - psi_k) -
alpha f load depends on what changed; F_psi and D(psi) depend on the iterate alone and are still in device memory from the last
evaluation of the solve before.  With the key on (the default) the library then runs the interior kernel without its exp pass
(k_resid_fill_grid<., true>) and takes the rest over.  Here:

1. whole settings-B runs, key 1 against key 0 within one build: counts, every history column and the final iterate equal as bits,
   and the counters say how often the entry evaluation was reduced (tests/test_gpu_krylov_parent.py pins the default path against the
   parent library);
2. the evaluation itself, both ways at one state (include/pgx.h: pgx_resid_reuse_selfcheck): F_u equal as bits, F_psi and every stored
   D copy untouched by the reduced form and equal to what the full form writes - also with f != 0 and a nonzero Dirichlet value;
3. every call that may write the iterate or one of the buffers taken over makes the next entry evaluation a full one.

Grids: 200 x 72 (partial interior tiles of 32 x 12 vertices in both directions: 199 = 6 * 32 + 7, 71 = 5 * 12 + 11), 40 x 20 (one
partial tile row) and 64 x 64."""
import ctypes as C

import numpy as np
import pytest

DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
KEY = "PGX_RESID_REUSE"
# the stencil copies written by the evaluating kernels (default) or derived by the Jacobian fill (PGX_D_DIRECT=0); the CSR rows of the
# interior skipped inside a solve (default) or written as well (PGX_LEAN_D=0)
MODES = {"default": {}, "d_direct0": {"PGX_D_DIRECT": 0}, "lean_d0": {"PGX_LEAN_D": 0}}


class Tuning:
    def __init__(self, keys):
        self.keys = keys

    def __enter__(self):
        from proximalgalerkin_amd import _lib

        for k, v in self.keys.items():
            _lib.tuning_set(k, v)

    def __exit__(self, *exc):
        from proximalgalerkin_amd import _lib

        for k in self.keys:
            _lib.tuning_set(k, None)


def make_problem(grid, f=0.0, g=0.0):
    """The obstacle problem of proximalgalerkin_amd.obstacle.setup_problem; f, g: load and Dirichlet value (that function fixes both at
    0, as the reference does)."""
    from proximalgalerkin_amd import fem, ufl
    from proximalgalerkin_amd.obstacle import phi_set, setup_problem
    from proximalgalerkin_amd.problem import NonlinearProblem

    msh = fem.create_rectangle(DOMAIN, grid)
    if f == 0.0 and g == 0.0:
        return setup_problem(msh, 1, petsc_options=dict(BASE))
    V = fem.functionspace(msh, ("Lagrange", 1), ncomp=2)
    alpha, fc = fem.Constant(msh, 1.0), fem.Constant(msh, f)
    bcs = fem.dirichletbc(g, msh.exterior_dofs(1), V.sub(0))
    sol, sol_k = fem.Function(V), fem.Function(V)
    phi_fn = fem.QuadratureFunction(msh, 6, name="phi")
    phi_fn.interpolate(phi_set)
    u, psi = ufl.split(sol)
    u_k, psi_k = ufl.split(sol_k)
    v, w = ufl.TestFunctions(V)
    dx = ufl.Measure("dx", domain=msh, metadata={"quadrature_degree": 6})
    F = (alpha * ufl.inner(ufl.grad(u), ufl.grad(v)) * dx + psi * v * dx + u * w * dx - ufl.exp(psi) * w * dx
         - phi_fn * w * dx - alpha * fc * v * dx - psi_k * v * dx)
    problem = NonlinearProblem(F, u=sol, bcs=[bcs], J=ufl.derivative(F, sol), petsc_options=dict(BASE), petsc_options_prefix="obstacle_")
    return problem, sol, sol_k, alpha


def proximal_steps(problem, sol_k, alpha, ks, counts):
    """Steps ks of obstacle.run_outer_loop (alpha rule double_exponential, alpha_max 100), without its stopping test."""
    from proximalgalerkin_amd.obstacle import alpha_update

    for k in ks:
        alpha.value, counts["alpha_k"] = alpha_update("double_exponential", k, counts["alpha_k"], 1e2, current=alpha.value)
        problem.solve()
        counts["newton"].append(int(problem.solver.getIterationNumber()))
        counts["linear"].append(int(problem.solver.getLinearSolveIterations()))
        counts["obs"].append(problem.observables().copy())
        sol_k.x.assign_from(problem.u.x)


# ---- 1. whole runs ----------------------------------------------------------------------------------------------------------
def lvpp_run(grid, key, mode):
    from proximalgalerkin_amd.obstacle import COLUMNS, run_outer_loop

    with Tuning(dict(MODES[mode], **{KEY: key})):
        problem, sol, sol_k, alpha = make_problem(grid)
    try:
        newton, lin, inner = [], [], problem.solve

        def one_solve():
            try:
                return inner()
            finally:
                newton.append(int(problem.solver.getIterationNumber()))
                lin.append(int(problem.solver.getLinearSolveIterations()))

        problem.solve = one_solve
        hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
        return {"newton": newton, "linear": lin, "hist": {c: np.array(hist[c]) for c in COLUMNS}, "x": sol.x.array.copy(),
                "counts": problem.resid_reuse_counts()}
    finally:
        problem.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid,mode", [((200, 72), "default"), ((40, 20), "default"), ((64, 64), "default"),
                                       ((40, 20), "d_direct0"), ((40, 20), "lean_d0")])
def test_whole_runs_equal_with_and_without_reuse(require_gpu, grid, mode):
    on, off = lvpp_run(grid, 1, mode), lvpp_run(grid, 0, mode)
    steps = len(on["newton"])
    print(f"{grid} {mode}: Newton {on['newton']} / {off['newton']}, linear {on['linear']} / {off['linear']}, "
          f"entry evaluations (full, reduced) {on['counts']} / {off['counts']}")
    assert steps > 2
    assert np.array_equal(on["newton"], off["newton"])
    assert np.array_equal(on["linear"], off["linear"])
    for c in on["hist"]:
        assert np.array_equal(on["hist"][c], off["hist"][c]), c
    assert np.array_equal(on["x"], off["x"])
    assert on["counts"] == (1, steps - 1)
    assert off["counts"] == (steps, 0)


# ---- 2. the evaluation itself ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("f,g", [(0.0, 0.0), (1.5, 0.2)])
def test_reduced_evaluation_is_the_full_one(require_gpu, f, g, mode):
    grid = (200, 72)
    with Tuning(MODES[mode]):
        problem, sol, sol_k, alpha = make_problem(grid, f, g)
    try:
        problem.zero_state()
        counts = {"alpha_k": 1, "newton": [], "linear": [], "obs": []}
        proximal_steps(problem, sol_k, alpha, range(3), counts)  # ends with sol_k <- sol
        alpha.value = 7.25  # the next step's alpha: only F_u sees it
        out = problem.resid_reuse_selfcheck()
        print(f"f={f} g={g} {mode}: Newton {counts['newton']}, selfcheck {out}")
        assert out[5] == (grid[0] + 1) * (grid[1] + 1)
        assert out[0] == 0, "F_u: reduced against full"
        assert out[1] == 0 and out[2] == 0, "the reduced evaluation wrote F_psi or a D copy"
        assert out[3] == 0 and out[4] == 0, "the values taken over are not those of a full evaluation"
        assert problem.resid_reuse_counts()[1] == 2
        # the hook dropped the stamp
        proximal_steps(problem, sol_k, alpha, [3], counts)
        assert problem.resid_reuse_counts() == (2, 2)
    finally:
        problem.close()


# ---- 3. invalidation --------------------------------------------------------------------------------------------------------------
def _raw(name, *args):
    """the C entry itself, return code ignored: the measurement hooks refuse a handle whose Jacobian a solve left stale
    (PGX_ESTATE) - and have dropped the stamp by then all the same"""
    def act(problem, sol, sol_k, alpha):
        getattr(problem._lib, name)(problem._h, *args)
    return act


def _set_state_same(problem, sol, sol_k, alpha):
    from proximalgalerkin_amd import _lib

    x = np.empty(problem.ndofs)
    _lib.check(problem._lib, problem._h, problem._lib.pgx_get_state(problem._h, _lib.dptr(x)), "pgx_get_state")
    _lib.check(problem._lib, problem._h, problem._lib.pgx_set_state(problem._h, _lib.dptr(x)), "pgx_set_state")


def _host_write(problem, sol, sol_k, alpha):
    sol.x.array[:] = sol.x.array.copy()  # the push entry: the host copy counts as changed


def _one_newton_step(problem, sol, sol_k, alpha):
    """a solve that runs out of iterations: its last evaluation was at an iterate that did not become sol"""
    from proximalgalerkin_amd.problem import ConvergenceError

    keep = problem._opts.snes_max_it
    problem._opts.snes_max_it = 1
    alpha.value = 30.0
    try:
        with pytest.raises(ConvergenceError):
            problem.solve()
    finally:
        problem._opts.snes_max_it = keep


def _fill_and_export(problem, sol, sol_k, alpha):
    problem.assemble_jacobian()
    problem.export_blocks()


_ms, _by, _nl = C.c_double(0), C.c_double(0), C.c_int(0)
WRITERS = {
    "set_state_same_values": _set_state_same,
    "host_write_of_sol": _host_write,
    "zero_state": lambda problem, sol, sol_k, alpha: problem.zero_state(),
    "residual": lambda problem, sol, sol_k, alpha: problem.residual(),
    "jacobian_fill": lambda problem, sol, sol_k, alpha: problem.assemble_jacobian(),
    "jacobian_fill_csr_export": _fill_and_export,
    "spmv_bench": _raw("pgx_spmv_bench", 1, C.byref(_ms), C.byref(_by)),
    "spmv_bench_cold": _raw("pgx_spmv_bench_cold", 1, C.byref(_ms), C.byref(_by)),
    "smoother_bench": _raw("pgx_smoother_bench", 1, C.byref(_ms), C.byref(_by)),
    "vcycle_bench": _raw("pgx_vcycle_bench", 0, 1, C.byref(_ms), C.byref(_nl)),
    "solve_out_of_iterations": _one_newton_step,
}
# what leaves the stamp standing: reads, the proximal centre, alpha, the observables - and tuning keys, which a handle reads when it
# is created and never again (a key set later cannot change which copies THIS handle keeps)
KEEPERS = {
    "get_state_get_prev": lambda problem, sol, sol_k, alpha: (sol.x.array_r.sum(), sol_k.x.array_r.sum()),
    "observables": lambda problem, sol, sol_k, alpha: problem.observables(),
    "tuning_keys_after_create": None,
}
LATE_KEYS = {"PGX_D_DIRECT": 0, "PGX_F32_DBF16": 0, "PGX_LEAN_D": 0, "PGX_RESID_GRID": 0, "PGX_MG_F32": 0}


def invalidation_run(key, case):
    act = WRITERS.get(case) or KEEPERS.get(case)
    with Tuning({KEY: key}):
        problem, sol, sol_k, alpha = make_problem((40, 20))
    try:
        problem.zero_state()
        counts = {"alpha_k": 1, "newton": [], "linear": [], "obs": []}
        proximal_steps(problem, sol_k, alpha, range(3), counts)
        before = problem.resid_reuse_counts()
        if act is not None:
            act(problem, sol, sol_k, alpha)
        mid = problem.resid_reuse_counts()
        with Tuning(LATE_KEYS if case == "tuning_keys_after_create" else {}):
            proximal_steps(problem, sol_k, alpha, [3, 4], counts)
        after = problem.resid_reuse_counts()
        return {"newton": counts["newton"], "linear": counts["linear"], "obs": np.array(counts["obs"]), "x": sol.x.array.copy(),
                "xk": sol_k.x.array.copy(), "before": before, "mid": mid, "after": after}
    finally:
        problem.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(WRITERS) + list(KEEPERS))
def test_writers_force_a_full_entry_evaluation(require_gpu, case):
    on, off = invalidation_run(1, case), invalidation_run(0, case)
    print(f"{case}: Newton {on['newton']} / {off['newton']}, (full, reduced) before {on['before']} -> {on['mid']} -> {on['after']}")
    assert on["before"] == (1, 2) and off["before"] == (3, 0)
    full_mid, reduced_mid = on["mid"]
    if case in WRITERS:
        # steps 3 and 4 after the writer: a full entry evaluation, then a reduced one again
        assert on["after"] == (full_mid + 1, reduced_mid + 1)
    else:
        assert on["mid"] == on["before"] and on["after"] == (full_mid, reduced_mid + 2)
    assert off["after"][1] == 0
    assert np.array_equal(on["newton"], off["newton"])
    assert np.array_equal(on["linear"], off["linear"])
    assert np.array_equal(on["obs"], off["obs"])
    assert np.array_equal(on["x"], off["x"])
    assert np.array_equal(on["xk"], off["xk"])
