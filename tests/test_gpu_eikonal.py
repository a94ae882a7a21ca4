"""Example 09 on the GPU (include/pgx_ek.h): the kernels against the numpy restatement tests/eikonal_reference.py at random states,
the structure of the exported matrix, the identity div_G x = 2 through the C ABI, the state moves, full runs against the restatement's
recorded runs (tests/golden/eikonal_*.npz, tools/make_eikonal_golden.py), determinism, the pivoting statistics and the error branch.

Every bound is the issue's or follows from the recorded sensitivities (eikonal_reference.field_tolerances); each test prints its
figures before it asserts.  DESIGN.md section 12f says which of the project's numbers for this example are measured."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import eikonal, lagrange, mesh_generation
from tests import eikonal_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _pair(nu, nv, g, nq, scale=1.0, **kw):
    mesh = mesh_generation.create_mobius_strip(nu, nv, g, scale)
    return R.Eikonal(nu, nv, g, nq, scale=scale), eikonal.EikonalProblem(mesh, nq, **kw)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# (3, 1, 1, 2): the smallest strip, flat cells, 4 points; (5, 2, 2, 5): 10 cells are no multiple of the 4 cells per workgroup, an odd
# point count; (4, 3, 3, 8): 64 points, exactly one full wave; (3, 2, 3, 9): 81 points, the second round of lanes
@pytest.mark.parametrize("shape", [(3, 1, 1, 2), (5, 2, 2, 5), (4, 3, 3, 8), (3, 2, 3, 9)])
@pytest.mark.parametrize("psi_scale", [0.5, 1e3])
def test_kernels_match_restatement(require_gpu, shape, psi_scale):
    P, prob = _pair(*shape, scale=1.3)
    try:
        rng = np.random.default_rng(11)
        n1, n2 = P.n1, P.n2
        assert prob.ndofs == P.ndofs and np.array_equal(prob.cell_dofs_u, P.cd1) and np.array_equal(prob.cell_dofs_p, P.cd2)
        x, xp = rng.standard_normal(P.ndofs), rng.standard_normal(P.ndofs)
        x[n1:] = rng.uniform(-psi_scale, psi_scale, 3 * n2)
        xp[n1:] *= psi_scale
        prob.set_state(x)
        prob.set_prev(xp)
        off = [0, n1, n1 + n2, n1 + 2 * n2, n1 + 3 * n2]
        for alpha in (3.7, 10.0):
            prob.set_alpha(alpha)
            F, fn = prob.residual()
            Fr = P.residual(x, xp, alpha)
            print(f"{shape} psi {psi_scale} alpha {alpha}: residual {_rel(F, Fr):.2e} norm {abs(fn - np.linalg.norm(Fr)) / np.linalg.norm(Fr):.2e}")
            assert np.all(np.isfinite(F)) and np.isfinite(fn)
            assert _rel(F, Fr) <= 1e-12
            assert abs(fn - np.linalg.norm(Fr)) <= 1e-12 * np.linalg.norm(Fr)
            Jd = prob.jacobian()
            assert np.all(np.isfinite(Jd.data))
            J, Jr = Jd.toarray(), P.jacobian(x).toarray()
            worst = 0.0
            for rb in range(4):
                for cb in range(4):
                    blk, ref = J[off[rb]:off[rb + 1], off[cb]:off[cb + 1]], Jr[off[rb]:off[rb + 1], off[cb]:off[cb + 1]]
                    if rb == 0 and cb == 0:
                        assert not blk.any() and not ref.any()
                        continue
                    worst = max(worst, np.abs(blk - ref).max() / np.abs(ref).max())
            print(f"   jacobian, worst block relative to its largest entry {worst:.2e}")
            assert worst <= 1e-12
            # structure: symmetric to the last bit, and the (u, u) block stores nothing at all
            assert np.array_equal(J, J.T)
            assert Jd[:n1, :n1].nnz == 0
            v = rng.standard_normal(P.ndofs)
            y = prob.spmv(v)
            print(f"   spmv {_rel(y, Jr @ v):.2e}")
            assert np.all(np.isfinite(y)) and _rel(y, Jr @ v) <= 1e-12
        x2 = x + 0.1 * rng.standard_normal(P.ndofs)  # a residual at an explicit point
        F2, _ = prob.residual(x2)
        assert _rel(F2, P.residual(x2, xp, 10.0)) <= 1e-12
        inc, incr = prob.l2_increment_u(), P.l2_increment_u(x, xp)
        print(f"   increment {abs(inc - incr) / incr:.2e}")
        assert abs(inc - incr) <= 1e-12 * incr
        ce, cr = prob.eval_cells(), P.eval_cells(x)
        assert ce.shape == cr.shape == (P.nc, (P.g + 1) ** 2, 7) and np.all(np.isfinite(ce))
        d = [np.abs(ce[..., s] - cr[..., s]).max() / np.abs(cr[..., s]).max() for s in (slice(0, 1), slice(1, 4), slice(4, 7))]
        print(f"   eval_cells (u, grad u, psi) {d}")
        assert max(d) <= 1e-12
    finally:
        prob.close()


def _position_dofs(prob):
    """the discrete surface's position vector as a [Q2]^3 function (g <= 2: x_h is in the space), from the package's own mesh"""
    mesh = prob.mesh
    t = np.arange(3) / 2.0
    N, _ = lagrange.tabulate_quad(mesh.order, np.stack([np.tile(t, 3), np.repeat(t, 3)], axis=1), snap=True)
    Xq2 = np.einsum("bn,cni->cbi", N, mesh.cell_nodes)
    out = np.zeros((3, prob.n2))
    for i in range(3):
        out[i, prob.cell_dofs_p.ravel()] = Xq2[:, :, i].ravel()
    return out


@pytest.mark.parametrize("shape", [(3, 1, 1, 3), (5, 2, 2, 5), (8, 3, 2, 9)])
def test_surface_divergence_of_the_position_vector_is_two(require_gpu, shape):
    """B x_h = 2 (1, v) through the C ABI: with alpha = 1, f = 1 and a zero previous iterate, R_v(0) = (1, v) and
    R_v([0; x_h]) = B x_h + (1, v)"""
    nu, nv, g, nq = shape
    prob = eikonal.EikonalProblem(mesh_generation.create_mobius_strip(nu, nv, g, 1.7), nq)
    try:
        n1 = prob.n1
        prob.set_alpha(1.0)
        prob.set_prev(np.zeros(prob.ndofs))
        fv = prob.residual(np.zeros(prob.ndofs))[0][:n1]
        x = np.concatenate([np.zeros(n1), _position_dofs(prob).ravel()])
        Bx = prob.residual(x)[0][:n1] - fv
        print(f"{shape}: |B x - 2 (1, v)| / |2 (1, v)| = {np.linalg.norm(Bx - 2 * fv) / np.linalg.norm(2 * fv):.2e}")
        assert fv.min() > 0
        assert np.linalg.norm(Bx - 2 * fv) <= 1e-13 * np.linalg.norm(2 * fv)
    finally:
        prob.close()


def test_state_moves_are_exact_copies(require_gpu):
    P, prob = _pair(5, 2, 2, 5)
    try:
        rng = np.random.default_rng(5)
        x, xk = rng.standard_normal(P.ndofs), rng.standard_normal(P.ndofs)
        assert not prob.get_state().any() and not prob.get_prev().any()
        prob.set_state(x)
        prob.set_prev(xk)
        assert np.array_equal(prob.get_state(), x) and np.array_equal(prob.get_prev(), xk)
        prob.advance_prev()
        assert np.array_equal(prob.get_prev(), x) and np.array_equal(prob.get_state(), x)
        assert prob.l2_increment_u() == 0.0
        prob.set_state(np.zeros(P.ndofs))
        assert not prob.get_state().any() and np.array_equal(prob.get_prev(), x)
    finally:
        prob.close()


def _create_raw(nu, nv, g=1, nq=2):
    """pgx_ek_create on the restatement's numbering and nodes, which have no guard of their own -> (return code, message)"""
    import ctypes as C

    from proximalgalerkin_amd import _lib

    lib = _lib.load()
    n1, cd1 = R.numbering(nu, nv, 1)
    n2, cd2 = R.numbering(nu, nv, 2)
    lat = np.arange(g + 1) / g
    cx, cy = np.arange(nu * nv) % nu, np.arange(nu * nv) // nu
    X = np.ascontiguousarray(R.mobius(2.0 * np.pi * (cx[:, None] + np.tile(lat, g + 1)[None, :]) / nu,
                                      (cy[:, None] + np.repeat(lat, g + 1)[None, :]) / nv))
    cd1, cd2 = np.ascontiguousarray(cd1, dtype=np.int32), np.ascontiguousarray(cd2, dtype=np.int32)
    t, w = R.gauss_1d(nq)
    t, w = np.ascontiguousarray(t), np.ascontiguousarray(w)
    pp = _lib.pgx_ek_problem(nu * nv, g, _lib.dptr(X), n1, n2, _lib.iptr(cd1), _lib.iptr(cd2), nq, _lib.dptr(t), _lib.dptr(w), 1.0, 1.0)
    h = C.c_void_p()
    rc = lib.pgx_ek_create(C.byref(pp), 0, C.byref(h))
    msg = (lib.pgx_ek_last_error(None) or b"").decode()
    if rc == 0:
        lib.pgx_ek_destroy(h)
    return rc, msg


def test_create_refuses_strips_of_fewer_than_three_cells_and_too_many_unknowns(require_gpu):
    rc, msg = _create_raw(1, 2)  # the one cell of a row meets itself
    print(rc, msg)
    assert rc == -1 and "twice" in msg
    rc, msg = _create_raw(2, 1)  # the two cells meet each other on both sides
    print(rc, msg)
    assert rc == -1 and "more than one edge" in msg
    assert _create_raw(3, 1)[0] == 0
    rc, msg = _create_raw(200, 13)  # 200 * 14 + 3 * 400 * 27 = 35 200 unknowns > PGX_DN_MAX_N = 32 768
    print(rc, msg)
    assert rc == -1 and "35200" in msg


_runs = {}


def _params(g):
    return dict(nu=int(g["nu"]), nv=int(g["nv"]), order=int(g["g"]), nq1=int(g["nq1"]), scale=float(g["scale"]), tol=float(g["tol"]))


def _state(fields):
    return np.concatenate([fields["u"], fields["psi"].ravel()])


def _golden_run(name):
    """one run of a recorded configuration through solve_problem, shared between the tests that read it"""
    g = np.load(GOLDEN / f"eikonal_{name}.npz")
    if name not in _runs:
        stats = []
        _runs[name] = eikonal.solve_problem(monitor=lambda p, i: stats.append(p.lu_stats()), **_params(g)) + (stats,)
    return g, _runs[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_full_run_matches_recorded_run(require_gpu, name):
    g, (fields, log, _) = _golden_run(name)
    print(f"golden {name}: steps (alpha, its, reason) {log[:, 1:4].tolist()}")
    assert np.array_equal(log[:, :4], g["log"]), (log, g["log"])
    d = R.field_differences(len(fields["u"]), _state(fields), g["z"])
    tol = R.field_tolerances(g)
    print(f"golden {name}: (u absolute, psi relative) {d}, tolerance {tol}, increments differ by {np.abs(log[:, 4] - g['increments']).max():.2e}")
    assert np.all(d <= tol)
    assert np.all(np.isfinite(fields["cells"])) and abs(fields["cells"][..., 0].max() - float(g["max_u"])) <= tol[0]


def test_determinism(require_gpu):
    g, (fields, log, _) = _golden_run("B")
    fields2, log2 = eikonal.solve_problem(**_params(g))
    assert np.array_equal(log, log2)
    for k in fields:
        assert np.array_equal(fields[k], fields2[k]), k


def test_pivoting_does_work_on_the_last_factorisation(require_gpu):
    _, (_, log, stats) = _golden_run("B")
    assert len(stats) == len(log)
    st = stats[-1]
    print(f"golden B, last factorisation: {st}")
    assert st["n"] == 944 and st["interchanges"] > 0 and st["zero_pivots"] == 0


def test_not_converged_raises(require_gpu):
    g = np.load(GOLDEN / "eikonal_A.npz")
    assert g["log"][0, 2] > 1  # the recorded first step needs more than one Newton step
    with pytest.raises(eikonal.NotConvergedError):
        eikonal.solve_problem(snes_opts=dict(eikonal.solver_parameters(), snes_max_it=1), **_params(g))


def test_full_size_reaches_the_distance_bound(require_gpu):
    """the script's size, 64 x 8 (7 104 unknowns): u is the distance to the boundary, at most the half-width 1/4"""
    fields, log = eikonal.solve_problem()
    umax = fields["u"].max()
    print(f"64 x 8: {len(log)} LVPP steps, {int(log[:, 2].sum())} Newton steps, max u {umax:.6f}")
    assert np.all(np.isfinite(_state(fields))) and np.all(np.isfinite(fields["cells"]))
    assert 0.24 < umax <= 0.25 + 1e-3


def test_example_script_writes_its_files(require_gpu, tmp_path):
    import json
    import runpy
    import sys

    script = pathlib.Path(__file__).resolve().parents[1] / "examples" / "09_eikonal" / "eikonal.py"
    argv = sys.argv
    sys.argv = [str(script), "--nu", "4", "--nv", "1", "--order", "2", "--nq1", "4", "--result_dir", str(tmp_path),
                "--profile", str(tmp_path / "profile.json")]
    try:
        runpy.run_path(str(script), run_name="__main__")
    finally:
        sys.argv = argv
    a = np.load(tmp_path / "steps.npz")
    assert a["log"].shape[1] == 5 and np.all(a["log"][:, 2] > 0) and np.all(a["log"][:, 3] > 0)
    assert (tmp_path / "eikonal.vtu").exists()
    prof = json.loads((tmp_path / "profile.json").read_text())
    assert prof["unknowns"] == 4 * 2 + 3 * 8 * 3 and prof["newton_iterations"] == int(a["log"][:, 2].sum())
    assert prof["lu"]["zero_pivots"] == 0 and 0.0 < prof["lu_factor_share_of_newton"] < 1.0
