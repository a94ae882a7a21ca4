"""The numpy twin of example 05's comparison solvers (tests/thermoforming_comparison_reference.py; the reference's
solver_comparison/thermoforming_moreau_yosida.jl and thermoforming_fixed_point.jl) checked on its own, the host-side gamma
updates of proximalgalerkin_amd/thermoforming_comparison.py, and the ctypes mirror of include/pgx_qmy.h.  No GPU."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from tests import thermoforming_comparison_reference as R

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_twin_jacobian_matches_central_differences():
    """At a random state away from the kinks (every quadrature-point |d| and the distance of s from {0, q} above 1e-3; rejected
    draws are redrawn from the same seeded stream) the generalised Jacobian is the derivative of the residual.  The mesh is the
    crossed one: on the right-diagonal lattice two corner cells have all three vertices on the boundary, where u = Phi0 = phi = 0
    and d vanishes identically, so no draw could pass the margin test there."""
    from proximalgalerkin_amd import fem

    mesh = fem.create_unit_square(2, 2, diagonal="crossed")
    p = R.PenalisedThermoforming(mesh.geometry, mesh.cells, mesh.exterior_dofs(1), q=0.5)
    rng = np.random.default_rng(20)
    for draw in range(5000):
        x = rng.standard_normal(p.ntot)
        if min(p.margins(x)) > 1e-3:
            break
    else:
        pytest.fail("no state away from the kinks")
    uq, Tq, pq, d, s = p._points(x)
    assert (d > 0).any() and (d < 0).any() and ((s > 0) & (s < p.q)).any()  # both branches of plus and the band of g
    h = 1e-6  # moves d and s by less than 3e-6: no point crosses a kink
    for gamma, mask in ((1.0, 3), (3.5e3, 3), (7.0, 1), (7.0, 2)):
        rows = np.concatenate([np.full(p.nv, bool(mask & 1)), np.full(p.nv, bool(mask & 2))])  # the active fields' rows
        J = p.jacobian(x, gamma, mask).toarray()[rows][:, rows]
        Jfd = np.empty_like(J)
        for k, i in enumerate(np.flatnonzero(rows)):
            e = np.zeros(p.ntot)
            e[i] = h
            Jfd[:, k] = ((p.residual(x + e, gamma, mask) - p.residual(x - e, gamma, mask)) / (2 * h))[rows]
        print(f"draw {draw} gamma {gamma} mask {mask}: max |J - J_fd| = {abs(J - Jfd).max():.2e}, max |J| = {abs(J).max():.2e}")
        # the residual is piecewise quadratic in x (phi T u products): central differences are exact up to rounding, eps |F| / h
        assert abs(J - Jfd).max() <= 1e-8 * max(abs(J).max(), 1.0)
    # a frozen field: identity rows with ZERO residual (so these rows are not a derivative), zero columns elsewhere
    for mask, frozen in ((1, slice(p.nv, None)), (2, slice(0, p.nv))):
        J = p.jacobian(x, 7.0, mask).toarray()
        keep = np.ones(p.ntot, bool)
        keep[frozen] = False
        assert np.array_equal(J[frozen][:, frozen], np.eye(p.nv)) and not J[frozen][:, keep].any() and not J[keep][:, frozen].any()
        assert not p.residual(x, 7.0, mask)[frozen].any()


@pytest.mark.parametrize("where", ["twin", "product"])
def test_gamma_updates_match_hand_computed_values(where):
    if where == "twin":
        my, fp = R.update_gamma_moreau_yosida, R.update_gamma_fixed_point
    else:
        from proximalgalerkin_amd import thermoforming_comparison as tc

        my, fp = tc.update_gamma_moreau_yosida, tc.update_gamma_fixed_point
    # gamma = 1, k = 2, infeasibility 1, functional 4: E = 1/4, theta = 5, C2 = 1/4 * 5/4 * 5 = 25/16, C1 = 25/4,
    # gamma_new = (25/16) / (1/2 * 5/4) - 1/4 = 9/4
    assert my(1.0, 2, 1.0, 4.0) == pytest.approx(2.25, rel=1e-14) and fp(1.0, 2, 1.0, 4.0) == pytest.approx(2.25, rel=1e-14)
    # a negative energy, as at the minimiser: gamma = 2, k = 3, infeasibility 1/2, functional -4: E = -1/4, theta = -7/2,
    # C2 = (-1/4)(7/4)(-7/2)/2 = 49/64, C1 = -49/16, |C1 - theta| = 7/16, gamma_new = (49/64) / (7/48) + 1/4 = 11/2
    assert my(2.0, 3, 0.5, -4.0) == pytest.approx(5.5, rel=1e-14) and fp(2.0, 3, 0.5, -4.0) == pytest.approx(5.5, rel=1e-14)
    # guards of the Moreau-Yosida update: a zero functional, and a value that is not finite (no infeasibility: 0/0; theta = 0:
    # 0/0) keep gamma.  (A finite value <= 0 cannot come out of the formula: it equals k |E + gamma| + |E| or k (E + gamma) - E
    # with E > -gamma.)  The fixed point's formula has no guard and returns the NaN.
    assert my(3.0, 4, 0.7, 0.0) == 3.0
    assert my(3.0, 4, 0.0, -2.0) == 3.0 and np.isnan(fp(3.0, 4, 0.0, -2.0))
    assert my(3.0, 4, 2.0, -2.0) == 3.0 and np.isnan(fp(3.0, 4, 2.0, -2.0))
    assert not np.isfinite(fp(3.0, 4, 0.7, 0.0))


_run = {}


def _my_run():
    if not _run:
        p = R.problem(8)
        mats = []
        _run["p"], _run["out"], _run["mats"] = p, p.solve_moreau_yosida(max_outer=10, matrices=mats), mats
    return _run


def test_twin_moreau_yosida_prefix_is_well_behaved():
    out = _my_run()["out"]
    print("gammas", out["gammas"], "newton", out["newton_its"], "cauchy", out["cauchy"])
    assert len(out["newton_its"]) == 10 and max(out["newton_its"]) <= 20 and all(r == 1 for r in out["reasons"])
    assert all(b > a for a, b in zip(out["gammas"], out["gammas"][1:]))


def test_newton_matrices_factorise_without_pivoting():
    """pgx_nd does not pivot across nodes: every matrix of the run above must factorise with the diagonal as pivot
    (diag_pivot_thresh = 0: SuperLU leaves the diagonal only for an exact zero) and give the pivoted solution to 1e-8."""
    mats = _my_run()["mats"]
    assert len(mats) == sum(_my_run()["out"]["newton_its"])
    worst = 0.0
    for J, b in mats:
        A = J.tocsc()
        x0 = spla.splu(A, diag_pivot_thresh=0.0).solve(b)
        x1 = spla.splu(A).solve(b)
        worst = max(worst, R.rel(x0, x1))
    print(f"{len(mats)} matrices, largest relative difference unpivoted vs pivoted: {worst:.2e}")
    assert worst <= 1e-8


def test_fixed_point_prefix_of_the_gpu_test_has_no_long_solve():
    """the prefix tests/test_gpu_thermoforming_comparison.py compares (M = 8, 3 outer steps, gamma_max = 1e7): no Newton solve above
    20 iterations, none capped"""
    out = R.problem(8).solve_fixed_point(max_outer=3, gamma_max=1e7)
    print(out["newton_its_T"], out["inner_steps"], out["newton_its_u"])
    assert max(out["newton_its_T"]) <= 20 and max(max(s) for s in out["newton_its_u"]) <= 20
    assert all(r > 0 for s in out["reasons_u"] for r in s)
    assert all(g[-1] < 1e7 for g in out["inner_gammas"])  # each inner path ended on gamma > gamma_max, not on its Cauchy norm


def test_newton_rules_of_the_twin():
    p = R.problem(4)
    x = p.initial_state()
    x1, its, reason = p.newton_nls(x, 1.0, max_it=2)
    assert (its, reason) == (2, 0) and not np.array_equal(x1, x)  # the cap is reported as 0 and the iterate is kept
    x2, its, reason = p.newton_nls(x, 1.0)
    assert reason == 1 and 2 < its <= 20
    assert p.newton_nls(x2, 1.0)[1:] == (0, 1)  # a start within ftol: no iteration


# -----------------------------------------------------------------------------------------------------------------------
_CTYPES = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "const double*": ctypes.POINTER(ctypes.c_double),
           "const int32_t*": ctypes.POINTER(ctypes.c_int32)}


def _header_struct(name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pgx_qmy.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)", decl)
        ctype = f"{'const ' if m.group(1) else ''}{m.group(2)}{m.group(3)}"
        for nm in m.group(4).split(","):
            fields.append((nm.strip(), _CTYPES[ctype]))
    return fields


@pytest.mark.parametrize("name", ["pgx_qmy_problem", "pgx_qmy_newton_opts"])
def test_ctypes_structs_mirror_the_header(name):
    from proximalgalerkin_amd import _lib

    declared = _header_struct(name)
    mirror = getattr(_lib, name)
    assert [(n, t) for n, t in mirror._fields_] == declared

    class Expect(ctypes.Structure):  # natural C alignment, laid out from the header's declarations
        _fields_ = declared

    assert ctypes.sizeof(mirror) == ctypes.sizeof(Expect)
    assert [getattr(mirror, n).offset for n, _ in declared] == [getattr(Expect, n).offset for n, _ in declared]


def test_python_layer_is_importable_without_a_gpu():
    from proximalgalerkin_amd import thermoforming_comparison as tc

    x = np.array([[0.5, 0.5], [0.0, 0.25], [0.25, 0.5]])
    assert np.allclose(tc.initial_mould(x), [1.0, 0.0, 0.5]) and np.allclose(tc.smoothing(x), [1.0, 0.0, np.sin(np.pi / 4)])
    assert tc.XTOL == 10 * np.finfo(float).eps and tc.C1 == -1e8
