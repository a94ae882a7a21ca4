"""The Krylov driver bit for bit against the library before it moved into a source file of its own.

csrc/pgx_krylov.hip holds FGMRES (fgmres), the way of every reduced scalar to the host (read_back: ticket, launch of its own, plain
second stage) and the one basis type that hides whether the Krylov vectors are fp64 or float.  That change rearranged host code only:
which kernels a solve launches, in which order and on which data is what it was.  The switch tests (test_gpu_krylov_passes.py,
test_gpu_krylov_f32_basis.py) compare a key on against off within ONE build, so a slip that moves both sides passes them; here every
path of the driver is one settings-B LVPP run whose Newton counts per proximal step, linear iterations per proximal step and final
iterate (SHA-256 of its fp64 bytes) are compared with what the library of the parent commit gave, recorded ONCE on an MI355X by
tools/make_golden_krylov_parent.py into golden/krylov_driver_parent.json (the parent's commit id is in the file).

The recording tool runs every case twice on the parent library; a case the parent does not reproduce bitwise is flagged there and
compared by its counts only.  The structured P1 cases must not be among them: their path has no atomics (test_gpu_determinism.py)."""
import hashlib
import json
import pathlib

import numpy as np
import pytest

DOMAIN = ((-1.0, -1.0), (1.0, 1.0))
BASE = {"snes_linesearch_type": "none", "snes_rtol": 1e-6, "snes_max_it": 100, "snes_error_if_not_converged": True}
GOLDEN = pathlib.Path(__file__).parent / "golden"
RECORD = GOLDEN / "krylov_driver_parent.json"
F32 = {"PGX_V_F32_MIN": 0}  # the float basis on a grid below its default threshold
ROUTES = ("PGX_TICKET_REDUCE", "PGX_FUSED_PUBLISH", "PGX_HOST_POLL")  # = 0: launch of its own / plain second stage / copy read-back
# id -> (mesh, degree, tuning keys, solver options).  mesh: (nx, ny) of a rectangle, or a file under golden/
CASES = {
    # 1089 vertices, below PGX_F32_MIN: fp64 cycle, no lazy normalisation, every new vector normalised in place
    "p1-32x32": ((32, 32), 1, {}, {}),
    # lazy normalisation, float Z, fp64 basis (14 673 vertices, below PGX_V_F32_MIN)
    "p1-200x72": ((200, 72), 1, {}, {}),
    "p1-200x72-f32": ((200, 72), 1, F32, {}),
    "p1-200x72-f32-restart4": ((200, 72), 1, F32, {"ksp_gmres_restart": 4}),          # restarts, the cycle target of the float basis
    "p1-200x72-f32-max0": ((200, 72), 1, dict(F32, PGX_V_F32_MAX=0), {}),             # guard -> abandoned cycle -> redone in fp64
    "p1-200x72-f32-eta2": ((200, 72), 1, dict(F32, PGX_CGS_ETA2=2), {}),              # second projection, float re-projection: always
    **{f"p1-200x72-f32-eta2-{k[4:].lower()}0": ((200, 72), 1, dict(F32, PGX_CGS_ETA2=2, **{k: 0}), {}) for k in ROUTES},
    **{f"p1-200x72-{k[4:].lower()}0": ((200, 72), 1, {k: 0}, {}) for k in ROUTES},
    "p1-200x72-lazy0": ((200, 72), 1, {"PGX_LAZY_NORM": 0}, {}),
    "p1-200x72-zf32-0": ((200, 72), 1, {"PGX_Z_F32": 0}, {}),
    "p2-16x16": ((16, 16), 2, {}, {}),                # full-length basis, patch cycle first
    "p1-disk": ("disk_h0.2.xdmf", 1, {}, {}),         # general mesh: sparse-LU preconditioner, CSR operator
}
MUST_REPRODUCE = [c for c, (mesh, degree, _, _) in CASES.items() if degree == 1 and not isinstance(mesh, str)]
_RUNS = {}


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype="<f8").tobytes()).hexdigest()


def solve(case, keep=True):
    """One settings-B LVPP run (as tests/test_gpu_krylov_passes.py: _solve) -> {"newton": Newton counts per proximal step, "linear":
    linear iterations per proximal step, "sha256": digest of the final iterate, "stopped": None, or the message of the error that
    ended the run early - the counts and the iterate are then those reached}.  Kept: a case is solved once per session."""
    if keep and case in _RUNS:
        return _RUNS[case]
    from proximalgalerkin_amd import _lib, fem, io
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem
    from proximalgalerkin_amd.problem import ConvergenceError

    mesh, degree, tuning, opts = CASES[case]
    for k, v in tuning.items():
        _lib.tuning_set(k, v)
    problem = None
    try:
        msh = io.read_mesh(GOLDEN / mesh) if isinstance(mesh, str) else fem.create_rectangle(DOMAIN, mesh)
        problem, sol, sol_k, alpha = setup_problem(msh, degree, petsc_options=dict(BASE, **opts))
        newton, lin, inner = [], [], problem.solve

        def one_solve():
            try:
                return inner()
            finally:
                newton.append(int(problem.solver.getIterationNumber()))
                lin.append(int(problem.solver.getLinearSolveIterations()))

        problem.solve = one_solve
        stopped = None
        try:
            hist = run_outer_loop(problem, sol, sol_k, alpha, 100, "double_exponential", 1e2, 1e-4, verbose=False)
            assert [int(n) for n in hist["Newton steps"]] == newton, (case, hist["Newton steps"], newton)
        except ConvergenceError as e:  # snes_error_if_not_converged: what the driver did up to there is pinned all the same
            stopped = str(e)
        out = {"newton": newton, "linear": lin, "sha256": digest(sol.x.array), "stopped": stopped}
    finally:
        if problem is not None:
            problem.close()
        for k in tuning:
            _lib.tuning_set(k, None)
    if keep:
        _RUNS[case] = out
    return out


def _record():
    return json.loads(RECORD.read_text())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_driver_is_bitwise_the_parent_library(require_gpu, case):
    want = _record()["cases"][case]
    got = solve(case)
    print(f"{case}: Newton {got['newton']} / parent {want['newton']}, linear {got['linear']} / parent {want['linear']}, "
          f"sha256 {got['sha256'][:16]} / parent {(want['sha256'] or 'not reproducible')[:16]}, stopped: {got['stopped']}")
    assert got["newton"] == want["newton"], case
    assert got["linear"] == want["linear"], case
    assert got["stopped"] == want["stopped"], case
    if want["reproducible"]:
        assert got["sha256"] == want["sha256"], case


def test_record_covers_every_case():
    """(no GPU) one record per case, from a stated commit; the structured P1 cases carry their digest"""
    rec = _record()
    assert len(rec["parent_commit"]) == 40
    assert set(rec["cases"]) == set(CASES)
    for case, r in rec["cases"].items():
        assert set(r) == {"newton", "linear", "sha256", "stopped", "reproducible"}, case
        assert len(r["newton"]) == len(r["linear"]) > 0, case
        assert r["reproducible"] == (r["sha256"] is not None), case
    assert all(rec["cases"][c]["reproducible"] for c in MUST_REPRODUCE)
