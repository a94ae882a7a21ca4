"""Multigrid on general meshes WITHOUT a refinement hierarchy (include/pgx.h: pgx_build_hierarchy; csrc/pgx_amg.hip) against
tests/amg_reference.py.

Meshes (amg_reference.build_mesh), none with a hierarchy: R5 = create_disk(0.5, refinements=2) renumbered by a fixed permutation, 227
vertices; U12 = create_disk(0.12), unrefined, 237 vertices; X32p = the crossed 3 x 2 rectangle refined three times, renumbered, 809
vertices, largest vertex degree 8.  State and alpha: those of tests/test_gpu_umg.py (UR.state: exp(psi) over many orders of magnitude
and a patch of exact zeros in D; alpha in {2.5, 100}).  The twin is fed the device's own level-0 K, M, D and mask, as there.

Bounds.  P_t: the pattern equal, the values within 1e-14 relative, entry by entry (the two kernels that compute P sum in the twin's
order and keep products and sums unfused).  Stored operators: 1e-13 of the level's largest |entry|, one cycle against the twin: 1e-12 of
max |z_ref| per half - the bounds of tests/test_gpu_umg.py.

Solves on a small mesh ask for the hierarchy through the constructor with PGX_UMG_BUILD_MIN=0 (by default the constructor builds one
under "pgx_mg" from 2 000 vertices up); the round trip through a file runs on a mesh above that size with no key set."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import pg_oracle as O
from tests import amg_reference as AR
from tests import umg_reference as UR

pytestmark = pytest.mark.gpu
MESHES = ("R5", "U12", "X32p")
ALPHAS = (2.5, 100.0)
OMEGA = 0.75
NUS = (1, 2, 6)
COARSE_SWEEPS = 60
PGX_EINVAL, PGX_EHIP, PGX_ESTATE = -1, -2, -5
MG = {"ksp_type": "preonly", "pc_type": "pgx_mg", "ksp_error_if_not_converged": True, "snes_error_if_not_converged": True,
      "snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100}
LU = dict(MG, pc_type="pgx_lu")

_meshes, _refs, _zref = {}, {}, {}
_live = None  # ONE live handle: tuning keys are process-wide


def _mesh(name):
    if name not in _meshes:
        _meshes[name] = AR.build_mesh(name)
    return _meshes[name]


class _Handle:
    def __init__(self, name, alpha, keys):
        from proximalgalerkin_amd import _lib
        from proximalgalerkin_amd.obstacle import setup_problem

        self.key, self.keys, self.problem = (name, alpha, tuple(sorted(keys.items()))), dict(keys), None
        self.name, self.alpha = name, alpha
        for k, v in self.keys.items():
            _lib.tuning_set(k, v)
        try:
            msh = _mesh(name)
            self.problem, sol, sol_k, a = setup_problem(msh)
            self.nlev = self.problem.build_hierarchy()
            self.x, xk = UR.state(msh.geometry)
            sol_k.x.array[:] = xk
            a.value = alpha
            self.problem.assemble_jacobian(self.x)
            assert self.problem.umg_levels() == self.nlev
            self.levels = [self.problem.umg_level_export(l) for l in range(self.nlev)]
            self.P = [self.problem.umg_transfer_export(t) for t in range(self.nlev - 1)]
        except BaseException:
            self.close()
            raise

    def reference(self):
        """(twin, Ps, masks) from the device's level-0 values; the hierarchy depends on K and the mask alone."""
        L0 = self.levels[0]
        n = L0["n"]
        K, M, D = (sp.csr_matrix((L0[v], L0["col"], L0["rowptr"]), shape=(n, n)) for v in ("K", "M", "D"))
        if self.name not in _refs:
            _refs[self.name] = AR.build_hierarchy(K, L0["mask"])
        Ps, masks = _refs[self.name]
        k = (self.name, self.alpha)
        if k not in _refs:
            _refs[k] = AR.AmgReference(K, M, D, self.alpha, L0["mask"], Ps, masks, coarse_sweeps=COARSE_SWEEPS)
        return _refs[k], Ps, masks

    def close(self):
        from proximalgalerkin_amd import _lib

        if self.problem is not None:
            self.problem.close()
        for k in self.keys:
            _lib.tuning_set(k, None)


def _drop():
    global _live
    if _live is not None:
        live, _live = _live, None
        live.close()


def _handle(name, alpha, keys=None):
    global _live
    keys = dict({"PGX_UMG_COARSE_SWEEPS": COARSE_SWEEPS}, **(keys or {}))
    key = (name, alpha, tuple(sorted(keys.items())))
    if _live is None or _live.key != key:
        _drop()
        _live = _Handle(name, alpha, keys)
    return _live


@pytest.fixture(scope="module", autouse=True)
def _close_last_handle():
    yield
    _drop()


def _dense(L, v):
    return sp.csr_matrix((L[v], L["col"], L["rowptr"]), shape=(L["n"], L["n"])).toarray()


# ---------------------------------------------------------------------------------------------------------------------
# transfers and stored operators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_exported_transfers_equal_the_twins(require_gpu, name):
    """Level 0 decides on the same K (the twin is fed the device's).  On the coarser transfers the split and the truncation decide on
    coarse K values that the device sums in its two gather stages and the twin in scipy's P.T @ K @ P, so they agree to rounding
    only: a value within rounding of theta x (row maximum) or trunc x (row maximum) could come out on the other side and change a
    pattern with no defect in the code.  None does on these three meshes; should one ever, look at the margins of that row first."""
    h = _handle(name, 2.5)
    _, Ps, masks = h.reference()
    assert len(h.P) == len(Ps) >= 1, ([P.shape for P in h.P], [P.shape for P in Ps])
    worst = 0.0
    for t, (P, R) in enumerate(zip(h.P, Ps)):
        assert P.shape == R.shape, (name, t)
        assert np.array_equal(P.indptr, R.indptr) and np.array_equal(P.indices, R.indices), (name, t)
        err = np.max(np.abs(P.data - R.data) / np.abs(R.data))
        worst = max(worst, err)
        assert err <= 1e-14, (name, t, err)
        assert np.array_equal(h.levels[t + 1]["mask"], masks[t]), (name, t)
    print(f"TRANSFERS {name}: levels {[L['n'] for L in h.levels]}, entries per row {[round(P.nnz / P.shape[0], 2) for P in h.P]}, "
          f"worst relative difference {worst:.2e}")


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", MESHES)
def test_stored_operators_equal_the_twins_triple_products(require_gpu, name, alpha):
    h = _handle(name, alpha)
    ref, _, _ = h.reference()
    assert [L["n"] for L in h.levels] == [L["n"] for L in ref.levels]
    assert np.count_nonzero(h.levels[0]["D"] == 0.0) > 0 and np.ptp(np.log10(h.levels[0]["D"][h.levels[0]["D"] > 0])) > 4
    for l, (L, R) in enumerate(zip(h.levels, ref.levels)):
        # M has no zero entry: its twin product carries the whole pattern P^T (pattern) P (scipy drops sums that are exactly 0)
        assert np.array_equal(L["rowptr"], R["M"].indptr) and np.array_equal(L["col"], R["M"].indices), (name, l)
        assert np.array_equal(L["mask"], R["mask"]), (name, l)
        for v in ("K", "M", "D"):
            want = R[v].toarray()
            err, top = np.max(np.abs(_dense(L, v) - want)), np.max(np.abs(want))
            print(f"STORED {name} alpha {alpha} level {l} {v}: {err / top:.2e} of the largest entry")
            assert err <= 1e-13 * top, (name, alpha, l, v, err / top)
    assert np.array_equal(np.flatnonzero(h.levels[0]["mask"]), np.sort(_mesh(name).exterior_vertices()))


@pytest.mark.parametrize("name", MESHES)
def test_two_fills_of_one_state_give_identical_levels(require_gpu, name):
    h = _handle(name, 2.5)
    h.problem.assemble_jacobian(h.x)
    again = [h.problem.umg_level_export(l) for l in range(len(h.levels))]
    for a, b in zip(h.levels, again):
        for v in ("rowptr", "col", "K", "M", "D", "mask"):
            assert a[v].tobytes() == b[v].tobytes(), (name, v)
    for t, P in enumerate(h.P):
        Q = h.problem.umg_transfer_export(t)
        assert P.data.tobytes() == Q.data.tobytes() and P.indices.tobytes() == Q.indices.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# one cycle as an operator
# ---------------------------------------------------------------------------------------------------------------------
def _rhs(h, level):
    """name -> [u | psi] of the level; below the finest the u part is 0 on the Dirichlet rows, as every restricted residual is."""
    L = h.levels[level]
    n, mask = L["n"], L["mask"]
    rng = np.random.default_rng(100 * len(h.name) + 10 * level + n)
    deg = np.diff(L["rowptr"]) - 1
    A = sp.csr_matrix((np.ones(len(L["col"])), L["col"], L["rowptr"]), shape=(n, n))
    near = np.flatnonzero((A @ mask.astype(float) > 0) & ~mask)  # free vertices with a Dirichlet neighbour
    free = np.flatnonzero(~mask)

    def impulse(v):
        b = np.zeros(2 * n)
        b[v], b[n + v] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5), rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5)
        return b

    out = {"random": rng.standard_normal(2 * n), "next-to-boundary": impulse(near[len(near) // 2]), "largest-degree": impulse(int(np.argmax(deg)))}
    if level + 1 < len(h.levels):
        single = np.diff(h.P[level].indptr) == 1  # the coarse vertices (and F vertices with one C neighbour)
        out["one-entry-row"] = impulse(free[single[free]][-1])
        out["interpolated"] = impulse(free[~single[free]][np.count_nonzero(~single[free]) // 3])
    if level == 0:
        out["boundary"] = impulse(np.flatnonzero(mask)[1])
    else:
        for b in out.values():
            b[:n][mask] = 0.0
    return out


@pytest.mark.parametrize("coarse", ["one-launch", "fallback"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", MESHES)
def test_cycle_against_the_twin_on_every_level(require_gpu, name, alpha, coarse):
    from proximalgalerkin_amd._lib import PgxError

    h = _handle(name, alpha, {"PGX_UMG_COARSE_LDS": 1 if coarse == "one-launch" else 0})
    ref, _, _ = h.reference()
    worst = 0.0
    for level in range(len(h.levels)):
        n = h.levels[level]["n"]
        for rname, b in _rhs(h, level).items():
            for nu in NUS:
                k = (name, alpha, level, rname, nu)
                if k not in _zref:
                    _zref[k] = ref.cycle(level, b, nu, OMEGA)
                zr = _zref[k]
                try:
                    z = h.problem.umg_cycle_apply(level, b, nu=nu, omega=OMEGA)
                except PgxError as e:
                    if getattr(e, "code", 0) == PGX_EHIP:
                        pytest.exit(f"HIP error in pgx_umg_cycle_apply: {e}", returncode=3)
                    raise
                for half, s in (("u", slice(0, n)), ("psi", slice(n, 2 * n))):
                    err = np.max(np.abs(z[s] - zr[s])) / np.max(np.abs(zr[s]))
                    worst = max(worst, err)
                    assert err <= 1e-12, (name, alpha, coarse, level, rname, nu, half, err)
    print(f"CYCLE {name} alpha {alpha} {coarse}: worst {worst:.2e} of max |z_ref|")


# ---------------------------------------------------------------------------------------------------------------------
# solves
# ---------------------------------------------------------------------------------------------------------------------
def _solve(msh, options, keys=None, degree=1):
    """Settings B (double_exponential, alpha_max 100, tol 1e-4): (u, Newton counts, Krylov iterations per LVPP solve, levels)."""
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    _drop()
    keys = keys or {}
    for k, v in keys.items():
        _lib.tuning_set(k, v)
    try:
        problem, sol, sol_k, alpha = setup_problem(msh, degree, petsc_options=dict(options))
        try:
            lin, solve = [], problem.solve

            def counted():
                r = solve()
                lin.append(problem.solver.getLinearSolveIterations())
                return r

            problem.solve = counted
            hist = run_outer_loop(problem, sol, sol_k, alpha, 500, "double_exponential", 1e2, 1e-4)
            u = sol.x.array[: sol.function_space.block_size].copy()
            problem.assemble_jacobian()
            try:
                levels = problem.umg_levels()
            except _lib.PgxError:
                levels = 0
        finally:
            problem.close()
    finally:
        for k in keys:
            _lib.tuning_set(k, None)
    return u, [int(v) for v in hist["Newton steps"]], lin, levels


BUILD = {"PGX_UMG_BUILD_MIN": 0}


def test_u12_solve_matches_the_lu_run_and_the_twins_krylov_counts(require_gpu):
    msh = _mesh("U12")
    assert msh.num_vertices == 237
    u, newton, lin, levels = _solve(msh, MG, BUILD)
    u_lu, newton_lu, lin_lu, _ = _solve(msh, LU)
    assert levels >= 2
    prob = O.ObstacleP1(msh.geometry, msh.cells, msh.exterior_vertices())
    Ps, masks = AR.build_hierarchy(prob.K, prob.isbc)
    stats = []
    _, hist = O.solve_problem(prob, 500, "double_exponential", 1e2, 1e-4,
                              linear_solve=AR.make_linear_solve(prob, Ps, masks, nu=6, omega=OMEGA, coarse_sweeps=COARSE_SWEEPS, stats=stats))
    ends = np.cumsum(hist["Newton steps"])
    twin = [int(sum(stats[a:b])) for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)]
    print(f"U12 Newton {newton} (LU {newton_lu}); Krylov per LVPP solve {lin}, twin {twin} (per Newton step {stats}); LU {lin_lu}")
    assert newton == newton_lu == [int(v) for v in hist["Newton steps"]]
    err = np.linalg.norm(u - u_lu) / np.linalg.norm(u_lu)
    print(f"U12 rel-L2(u) against the LU run: {err:.2e}")
    assert err <= 1e-10
    assert len(lin) == len(twin) and all(d <= t + 2 for d, t in zip(lin, twin)), (lin, twin)


def test_degree_2_solve_on_r5_through_the_patch_cycle_matches_the_lu_run(require_gpu):
    msh = _mesh("R5")
    u, newton, lin, levels = _solve(msh, MG, BUILD, degree=2)
    u_lu, newton_lu, lin_lu, _ = _solve(msh, LU, degree=2)
    print(f"R5 degree 2: Newton {newton} (LU {newton_lu}); Krylov per LVPP solve {lin}; levels {levels}")
    assert levels >= 2 and newton == newton_lu


def test_mesh_read_from_a_file_gets_levels_and_solves_under_pgx_mg(require_gpu, tmp_path):
    """The reference's own workflow for example 01: a mesh written to XDMF and read back carries no hierarchy; under "pgx_mg" the
    handle builds one by itself, with no key set (the mesh has more than the 2 000 vertices from which the constructor does)."""
    from proximalgalerkin_amd import fem, io
    from proximalgalerkin_amd.obstacle import setup_problem

    _drop()
    disk = fem.create_disk(0.04)
    assert disk.num_vertices == 2044
    io.write_xdmf_mesh(tmp_path / "disk.xdmf", disk)
    msh = io.read_mesh(tmp_path / "disk.xdmf")
    assert msh.hierarchy is None and msh.num_vertices == disk.num_vertices
    auto = setup_problem(msh, 1)[0]  # the reference's option set, as the example scripts run by default: the sparse LU, no levels
    try:
        auto.assemble_jacobian(np.zeros(2 * msh.num_vertices))
        _refused(lambda: auto.umg_levels(), PGX_ESTATE)
    finally:
        auto.close()
    problem = setup_problem(msh, 1, pc_type="pgx_mg")[0]  # what obstacle_pg.py / compare_all.py --pc-type pgx_mg pass on
    try:
        problem.assemble_jacobian(np.zeros(2 * msh.num_vertices))
        assert problem.umg_levels() >= 2
        sizes = [problem.umg_level_export(l)["n"] for l in range(problem.umg_levels())]
    finally:
        problem.close()
    u, newton, lin, levels = _solve(msh, MG)
    u_lu, newton_lu, _, _ = _solve(msh, LU)
    print(f"disk(0.04) from a file: levels {sizes}; Newton {newton} (LU {newton_lu}); Krylov per LVPP solve {lin}")
    assert levels == len(sizes) and newton == newton_lu
    assert np.linalg.norm(u - u_lu) <= 1e-10 * np.linalg.norm(u_lu)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refused(call, code):
    from proximalgalerkin_amd._lib import PgxError

    with pytest.raises(PgxError) as e:
        call()
    assert e.value.code == code, (e.value.code, code, str(e.value))
    assert len(str(e.value).split("): ", 1)[1]) > 10  # a message


def test_refusals_leave_the_handle_working(require_gpu):
    """(A sharded handle is structured by construction: the structured refusal is the one it meets.)"""
    from proximalgalerkin_amd import comm as pcomm
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.obstacle import setup_problem

    _drop()
    msh = _mesh("R5")
    x, xk = UR.state(msh.geometry)
    grid = fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), (8, 8))
    for other, xo in ((setup_problem(grid)[0], np.zeros(2 * grid.num_vertices)),
                      (setup_problem(msh, 1, lu_comm=pcomm.local_group(1)[0])[0], x)):
        try:
            _refused(lambda: other.build_hierarchy(), PGX_EINVAL)
            other.assemble_jacobian(xo)  # the handle took no harm
        finally:
            other.close()

    problem, sol, sol_k, a = setup_problem(msh)
    try:
        sol_k.x.array[:] = xk
        a.value = 2.5
        _refused(lambda: problem.umg_transfer_export(0), PGX_ESTATE)  # nothing built yet
        _refused(lambda: problem.build_hierarchy(theta=1.5), PGX_EINVAL)
        _refused(lambda: problem.build_hierarchy(trunc=0.0), PGX_EINVAL)  # a truncated entry is marked by an exact 0: trunc > 0
        _refused(lambda: problem.build_hierarchy(min_coarse=1000), PGX_EINVAL)  # nothing to coarsen
        nlev = problem.build_hierarchy()  # the handle took no harm: the hierarchy goes in ...
        _refused(lambda: problem.build_hierarchy(), PGX_ESTATE)  # ... once
        refined = UR.build_mesh("D5")
        _refused(lambda: problem.set_hierarchy(refined.hierarchy), PGX_ESTATE)  # nor an attached one on top
        _refused(lambda: problem.umg_level_export(0), PGX_ESTATE)  # no Jacobian yet
        problem.assemble_jacobian(x)
        levels = [problem.umg_level_export(l) for l in range(problem.umg_levels())]
        assert len(levels) == nlev >= 2
        _refused(lambda: problem.umg_transfer_export(nlev - 1), PGX_EINVAL)
        want = _handle("R5", 2.5).levels  # the handle the stored-operator test sees
        for L, W in zip(levels, want):
            for v in ("rowptr", "col", "K", "M", "D", "mask"):
                assert L[v].tobytes() == W[v].tobytes(), v
    finally:
        problem.close()
    _drop()

    attached = setup_problem(UR.build_mesh("D5"))[0]  # a mesh that brought its hierarchy: a built one does not go on top
    try:
        _refused(lambda: attached.build_hierarchy(), PGX_ESTATE)
        attached.assemble_jacobian(UR.state(UR.build_mesh("D5").geometry)[0])
        assert attached.umg_levels() == 3
        _refused(lambda: attached.umg_transfer_export(0), PGX_ESTATE)
    finally:
        attached.close()

    late = setup_problem(msh)[0]
    try:
        late.assemble_jacobian(x)
        _refused(lambda: late.build_hierarchy(), PGX_ESTATE)  # after the first Jacobian fill
    finally:
        late.close()
