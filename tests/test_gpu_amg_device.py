"""The device pass of pgx_build_hierarchy (csrc/pgx_amg_build.hip; the default) against the host pass it replaces (csrc/pgx_amg.hip,
tuning key PGX_AMG_BUILD=0): the two must build THE SAME hierarchy, bit for bit - the level count, every level's rowptr, col, mask, K,
M, D and every transfer's rowptr, col, val.  The split, the numbering and the patterns are integer work; P, K, M and D come from the
same value kernels over index arrays that agree entry for entry, so there is no tolerance anywhere in this file.

Meshes: R5, U12, X32p of tests/amg_reference.py; create_disk(0.03), 3 561 vertices in the generator's order, whose level-0 split needs
208 synchronous rounds (tests/test_cpu_amg_parallel_split.py): chains of decisions that cross the 14 blocks of the split kernel, which
sweeps its own 256 vertices to the end inside a launch (measured: done within the first batch of 16 launches); and
create_disk(0.0069), see test_bitwise_equal_above_the_two_pass_scan, whose level-0 split goes through several batches of launches with
a read of the termination counter between them (measured: 112 launches).  How many launches a split takes depends on the order in
which the hardware runs the blocks, so the tests bound it (>= 1, <= the level's vertices) and print it.  The path of the repeated
read does not hang on that: test_split_with_a_termination_read_after_every_launch lowers the batch to one launch with the test-only
key PGX_AMG_SPLIT_BATCH, so every launch beyond the first is one more trip through it.  State and alpha: UR.state,
2.5, after assemble_jacobian, as tests/test_gpu_amg.py.

The merge that builds the plan rows (ab_merge_row) keeps no per-row buffer, so no kernel of the pass has a per-row capacity and there
is no second, "general" path to force: the one path is exact for every row length.

One live handle at a time: tuning keys are process-wide."""
import numpy as np
import pytest

from tests import amg_reference as AR
from tests import p2_umg_reference as Q  # c_stdout_to, krylov_per_newton_step: the library's monitor lines
from tests import umg_reference as UR

pytestmark = pytest.mark.gpu
PGX_EINVAL, PGX_ESTATE = -1, -5
ALPHA = 2.5
MG = {"ksp_type": "preonly", "pc_type": "pgx_mg", "ksp_error_if_not_converged": True, "snes_error_if_not_converged": True,
      "snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100}
LU = dict(MG, pc_type="pgx_lu")

_meshes, _built = {}, {}


def _mesh(name):
    from proximalgalerkin_amd import fem

    if name not in _meshes:
        if name == "disk03":
            _meshes[name] = fem.create_disk(0.03)
        elif name == "disk0069":
            _meshes[name] = fem.create_disk(0.0069)
        else:
            _meshes[name] = AR.build_mesh(name)
    return _meshes[name]


def _build(name, mode, batch=None):
    """Everything the hooks export of the hierarchy `mode` (0 host, 1 device, None: no key set) builds on mesh `name`; handle closed
    and keys cleared on return.  batch: PGX_AMG_SPLIT_BATCH (test-only: split launches between two reads of the termination counter).
    Computed once per (mesh, mode, batch)."""
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.obstacle import setup_problem

    name_key = (name, mode, batch)
    if name_key in _built:
        return _built[name_key]
    keys = {} if mode is None else {"PGX_AMG_BUILD": mode}
    if batch is not None:
        keys["PGX_AMG_SPLIT_BATCH"] = batch
    for k, v in keys.items():
        _lib.tuning_set(k, v)
    problem = None
    try:
        msh = _mesh(name)
        problem, sol, sol_k, a = setup_problem(msh)
        nlev = problem.build_hierarchy()
        info, seconds = problem.build_info(), problem.build_seconds
        x, xk = UR.state(msh.geometry)
        sol_k.x.array[:] = xk
        a.value = ALPHA
        problem.assemble_jacobian(x)
        assert problem.umg_levels() == nlev
        levels = [problem.umg_level_export(l) for l in range(nlev)]
        P = [problem.umg_transfer_export(t) for t in range(nlev - 1)]
    finally:
        if problem is not None:
            problem.close()
        for k in keys:
            _lib.tuning_set(k, None)
    _built[name_key] = dict(nlev=nlev, levels=levels, P=P, info=info, seconds=seconds)
    return _built[name_key]


def _assert_bitwise(name, batch=None):
    host, dev = _build(name, 0), _build(name, 1, batch)
    assert host["info"]["mode"] == "host" and dev["info"]["mode"] == "device"
    assert host["nlev"] == dev["nlev"] >= 2, (name, host["nlev"], dev["nlev"])
    for l, (H, D) in enumerate(zip(host["levels"], dev["levels"])):
        assert H["n"] == D["n"], (name, l, H["n"], D["n"])
        for v in ("rowptr", "col", "mask", "K", "M", "D"):
            assert H[v].dtype == D[v].dtype and H[v].tobytes() == D[v].tobytes(), (name, "level", l, v)
    for t, (H, D) in enumerate(zip(host["P"], dev["P"])):
        assert H.shape == D.shape, (name, t)
        for v in ("indptr", "indices", "data"):
            assert getattr(H, v).tobytes() == getattr(D, v).tobytes(), (name, "transfer", t, v)
    sizes = [L["n"] for L in dev["levels"]]
    launches = dev["info"]["split_launches"]
    assert len(launches) == dev["nlev"] - 1
    assert all(1 <= k <= n for k, n in zip(launches, sizes)), (name, launches, sizes)
    print(f"BITWISE {name}: levels {sizes}, split launches {launches}; build host pass {host['seconds']}, device pass {dev['seconds']} s "
          f"(host time, device and copies)")


@pytest.mark.parametrize("name", ["R5", "U12", "X32p", "disk03"])
def test_device_pass_builds_the_host_passes_hierarchy_bit_for_bit(require_gpu, name):
    _assert_bitwise(name)


def test_bitwise_equal_above_the_two_pass_scan(require_gpu):
    """create_disk(0.0069): the smallest of the generator's disks at steps of 0.0001 with more than 65 536 = 256^2 vertices.  The
    scan works in tiles of 256 and scans the tile sums by itself: up to 256 rows it is one launch, up to 65 536 two passes, above that
    three (tile sums, sums of the tile sums, one last tile) - the deepest structure any mesh below 16.7 million vertices reaches.
    Every per-row scan of level 0 runs it; the coarser levels of the same build run the two shallower ones.  No kernel of the pass has
    a single-launch capacity (grids grow with the level), so this is the one size boundary the pass has."""
    msh = _mesh("disk0069")
    assert 65536 < msh.num_vertices < 70000, msh.num_vertices
    _assert_bitwise("disk0069")
    sizes = [L["n"] for L in _build("disk0069", 1)["levels"]]
    assert any(256 < n <= 65536 for n in sizes[1:]) and sizes[-1] <= 256, sizes


def test_split_with_a_termination_read_after_every_launch(require_gpu):
    """create_disk(0.03) with one split launch per read of the counter of decided vertices: the launch count is then the number of
    launches the split needed, and each one beyond the first went through the read-and-relaunch path.  With the default batch of 16
    the same mesh ends inside the first batch.  A split that ended in one launch on every level would leave that path untested
    here: the block order decides it, so that case is reported, loudly, and not failed."""
    import warnings

    _assert_bitwise("disk03", batch=1)
    one, dflt = _build("disk03", 1, 1)["info"]["split_launches"], _build("disk03", 1)["info"]["split_launches"]
    print(f"SPLIT disk03: launches with a read after each {one}, with the default batch {dflt}")
    if max(one) < 2:
        warnings.warn("every split of create_disk(0.03) ended in one launch: the repeated termination read was not exercised")


def test_build_info_reports_the_pass_and_its_split_launches(require_gpu):
    from proximalgalerkin_amd.obstacle import setup_problem

    default = _build("X32p", None)  # no key set: the device pass
    assert default["info"]["mode"] == "device"
    sizes = [L["n"] for L in default["levels"]]
    assert len(default["info"]["split_launches"]) == default["nlev"] - 1
    assert all(1 <= k <= n for k, n in zip(default["info"]["split_launches"], sizes))
    host = _build("X32p", 0)
    assert host["info"]["mode"] == "host" and len(host["info"]["split_launches"]) == host["nlev"] - 1
    problem = setup_problem(_mesh("X32p"))[0]
    try:
        _refused(lambda: problem.build_info(), PGX_ESTATE)  # nothing built yet
        problem.build_hierarchy()
        assert problem.build_info() == default["info"]
    finally:
        problem.close()
    attached = setup_problem(UR.build_mesh("D5"))[0]  # a hierarchy that came with the mesh was not built
    try:
        _refused(lambda: attached.build_info(), PGX_ESTATE)
    finally:
        attached.close()


def _solve(msh, options, keys, monitor):
    """Settings B (double_exponential, alpha_max 100, tol 1e-4) with snes_monitor, the library's lines going to the file `monitor`:
    (u, Newton counts, Krylov iterations per Newton solve, Krylov iterations per Newton STEP, build mode)."""
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    for k, v in keys.items():
        _lib.tuning_set(k, v)
    try:
        problem, sol, sol_k, alpha = setup_problem(msh, 1, petsc_options=dict(options, snes_monitor=None))
        try:
            lin, solve = [], problem.solve

            def counted():
                r = solve()
                lin.append(problem.solver.getLinearSolveIterations())
                return r

            problem.solve = counted
            with Q.c_stdout_to(str(monitor)):
                hist = run_outer_loop(problem, sol, sol_k, alpha, 500, "double_exponential", 1e2, 1e-4)
            u = sol.x.array[: sol.function_space.block_size].copy()
            try:
                mode = problem.build_info()["mode"]
            except _lib.PgxError:
                mode = None
        finally:
            problem.close()
    finally:
        for k in keys:
            _lib.tuning_set(k, None)
    return u, [int(v) for v in hist["Newton steps"]], lin, Q.krylov_per_newton_step(str(monitor)), mode


def test_u12_solve_on_the_device_pass_repeats_the_host_pass_run(require_gpu, tmp_path):
    """Krylov iterations per Newton step, read from the library's monitor lines ("KSP its N", one per step): the device-pass run's
    list must equal the host-pass run's, entry for entry - one entry per Newton step of the whole LVPP run - and so must the sums per
    Newton solve the front end reports; the Newton counts must equal the LU run's."""
    msh = _mesh("U12")
    u_d, newton_d, lin_d, steps_d, mode_d = _solve(msh, MG, {"PGX_UMG_BUILD_MIN": 0}, tmp_path / "device.txt")
    u_h, newton_h, lin_h, steps_h, mode_h = _solve(msh, MG, {"PGX_UMG_BUILD_MIN": 0, "PGX_AMG_BUILD": 0}, tmp_path / "host.txt")
    u_lu, newton_lu, _, _, mode_lu = _solve(msh, LU, {}, tmp_path / "lu.txt")
    assert (mode_d, mode_h, mode_lu) == ("device", "host", None)
    print(f"U12 device pass: Newton {newton_d}, Krylov per Newton step {steps_d}; host pass: Newton {newton_h}, Krylov per Newton step "
          f"{steps_h}; LU: Newton {newton_lu}; max |u_device - u_host| = {np.max(np.abs(u_d - u_h)):.1e}")
    assert len(steps_d) == sum(newton_d) and len(steps_h) == sum(newton_h), (steps_d, newton_d, steps_h, newton_h)
    ends = np.cumsum(newton_d)
    assert [sum(steps_d[a:b]) for a, b in zip([0, *ends[:-1]], ends)] == lin_d  # the monitor lines are the counts the solver sums
    assert steps_d == steps_h
    assert lin_d == lin_h
    assert newton_d == newton_h == newton_lu
    assert np.linalg.norm(u_d - u_lu) <= 1e-10 * np.linalg.norm(u_lu)  # the bound of tests/test_gpu_amg.py for the same pair of runs


def _refused(call, code):
    from proximalgalerkin_amd._lib import PgxError

    with pytest.raises(PgxError) as e:
        call()
    assert e.value.code == code, (e.value.code, code, str(e.value))
    assert len(str(e.value).split("): ", 1)[1]) > 10  # a message


def test_refusals_on_the_device_pass_leave_the_handle_working(require_gpu):
    from proximalgalerkin_amd.obstacle import setup_problem

    msh = _mesh("R5")
    x, xk = UR.state(msh.geometry)
    problem, sol, sol_k, a = setup_problem(msh)
    try:
        sol_k.x.array[:] = xk
        a.value = ALPHA
        _refused(lambda: problem.build_hierarchy(theta=1.5), PGX_EINVAL)
        _refused(lambda: problem.build_hierarchy(trunc=0.0), PGX_EINVAL)
        _refused(lambda: problem.build_hierarchy(min_coarse=1000), PGX_EINVAL)
        nlev = problem.build_hierarchy()  # the handle took no harm
        assert problem.build_info()["mode"] == "device"
        _refused(lambda: problem.build_hierarchy(), PGX_ESTATE)  # once
        problem.assemble_jacobian(x)
        levels = [problem.umg_level_export(l) for l in range(problem.umg_levels())]
        assert len(levels) == nlev >= 2
    finally:
        problem.close()
    want = _build("R5", 1)["levels"]
    for L, W in zip(levels, want):
        for v in ("rowptr", "col", "K", "M", "D", "mask"):
            assert L[v].tobytes() == W[v].tobytes(), v
