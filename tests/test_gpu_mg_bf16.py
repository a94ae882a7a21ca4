"""bf16 storage of the single-precision V-cycle's D(psi) stencil (csrc/pgx_mg32.hip; PGX_F32_DBF16, default 1) against the float4
form (PGX_F32_DBF16=0), in the corners of the template space that read the stencil differently: interior tiles and boundary
sub-tiles of the smoother with two, three and six sweeps per launch, with and without the fused residual + restriction, the
residual + restriction as a launch of its own, 8-row tiles, single precision down to levels of 500 vertices.  The cycle is a
preconditioner inside FGMRES, so what it stores may change Krylov counts but never what a Newton step computes: identical Newton
counts, primal field within 1e-10 relative (the project's parity bar) of the exact-Newton oracle's golden run."""
import pathlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}


def _solve(cells, tuning, opts):
    from proximalgalerkin_amd import _lib, fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    for k, v in tuning.items():
        _lib.tuning_set(k, v)
    try:
        msh = fem.create_rectangle(DOMAIN, cells)
        problem, sol, sol_k, alpha = setup_problem(msh, 1, petsc_options=dict(BASE, **opts))
        hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
        x = sol.x.array.copy()
        problem.close()
    finally:
        for k in tuning:
            _lib.tuning_set(k, None)
    return x, hist


@pytest.fixture(scope="module")
def golden(require_gpu):
    g = np.load(pathlib.Path(__file__).parent / "golden" / "obstacle_p1_n256_settingsB_large.npz")
    return int(g["N"]), g["u_final"], [int(c) for c in g["hist_Newton_steps"]]


@pytest.mark.parametrize("dbf16", [1, 0])
@pytest.mark.parametrize("tuning,opts", [
    ({}, {}),                                # default: three sweeps per launch on the big levels, six below 513^2
    ({"PGX_F32_K6_MAX": 0}, {}),             # three sweeps per launch everywhere, fused restriction
    ({"PGX_F32_RR_MAX": 0}, {}),             # the residual + restriction as a launch of its own
    ({"PGX_F32_TY": 8}, {}),                 # 8-row tiles
    ({"PGX_F32_MIN": 500}, {}),              # single precision down to levels of 500 vertices: mostly boundary sub-tiles
    ({}, {"mg_nu": 4}),                      # two sweeps per launch
    ({}, {"mg_nu": 3}),                      # one launch per leg: the FIRST launch restricts
])
def test_bf16_and_float_stencil_storage_match_the_golden_run(golden, dbf16, tuning, opts):
    N, u_ref, counts = golden
    x, h = _solve((N, N), dict(tuning, PGX_F32_DBF16=dbf16), opts)
    n = len(u_ref)
    err = np.linalg.norm(x[:n] - u_ref) / np.linalg.norm(u_ref)
    print(f"dbf16={dbf16} {tuning} {opts}: newton={h['Newton steps']} rel-L2(u)={err:.2e}")
    assert h["Newton steps"] == counts, (dbf16, tuning, opts)
    assert err <= 1e-10, (dbf16, tuning, opts, err)


@pytest.mark.parametrize("dbf16", [1, 0])
@pytest.mark.parametrize("cells", [(200, 72), (130, 260), (96, 48), (330, 118), (90, 270), (258, 130), (124, 124)])
def test_stencil_storage_on_rectangular_grids_that_cut_every_tile(require_gpu, cells, dbf16):
    """The grids of test_gpu_mg32's rectangular test (partial tiles, thin strips, odd coarse levels), single precision forced down
    to levels of 500 vertices, once with each storage: against the fp64 cycle on the same mesh."""
    x64, h64 = _solve(cells, {"PGX_MG_F32": 0}, {})
    n = (cells[0] + 1) * (cells[1] + 1)
    x, h = _solve(cells, {"PGX_F32_MIN": 500, "PGX_F32_DBF16": dbf16}, {})
    err = np.linalg.norm(x[:n] - x64[:n]) / np.linalg.norm(x64[:n])
    print(f"dbf16={dbf16} {cells}: newton={h['Newton steps']} rel-L2(u)={err:.2e}")
    assert h["Newton steps"] == h64["Newton steps"], (cells, dbf16)
    assert err <= 1e-10, (cells, dbf16, err)


@pytest.mark.parametrize("dbf16", [1, 0])
def test_stencil_storage_on_a_sharded_handle(require_gpu, dbf16):
    """Two strips driven by two host threads through the in-process transport (as tests/test_gpu_sharded.py): D(psi) is assembled
    per rank, ghost rows included, and never exchanged, so the sharded cycle reads the same packed words."""
    from proximalgalerkin_amd import _lib
    from proximalgalerkin_amd import comm as pcomm
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    nx, ny, R = 64, 128, 2
    sx, ng = nx + 1, (nx + 1) * (ny + 1)
    xg, hg = _solve((nx, ny), {"PGX_MG_F32": 0}, {})

    def rank_main(c):
        msh = fem.create_rectangle(DOMAIN, (nx, ny), comm=c, dist_levels=0)
        problem, sol, sol_k, alpha = setup_problem(msh, 1, petsc_options=BASE)
        hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
        x = sol.x.array.copy()
        off, cnt = problem.owned_range()
        part = msh.partition
        problem.close()
        return x, hist, part, off, cnt

    comms = pcomm.local_group(R)
    out, err = [None] * R, [None] * R

    def work(r):
        try:
            out[r] = rank_main(comms[r])
        except BaseException as e:  # noqa: BLE001 - reported below
            err[r] = e

    _lib.tuning_set("PGX_F32_DBF16", dbf16)
    try:
        th = [threading.Thread(target=work, args=(r,)) for r in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join(600)
    finally:
        _lib.tuning_set("PGX_F32_DBF16", None)
    for e in err:
        if e is not None:
            raise e
    u = np.full(ng, np.nan)
    for x, hist, part, off, cnt in out:
        assert hist["Newton steps"] == hg["Newton steps"]
        g0 = part.own0 * sx
        u[g0:g0 + cnt] = x[off:off + cnt]
    assert not np.isnan(u).any()
    rel = np.linalg.norm(u - xg[:ng]) / np.linalg.norm(xg[:ng])
    print(f"dbf16={dbf16} sharded R={R}: rel-L2(u)={rel:.2e}")
    assert rel <= 1e-10, (dbf16, rel)
