"""Example 09 without a GPU: the Moebius numbering and mesh of the package, the numpy restatement tests/eikonal_reference.py that the
GPU tests compare against, and the recorded runs (tests/golden/eikonal_*.npz, tools/make_eikonal_golden.py).

The restatement has its own numbering and geometry; both are compared with the package's here, and each is checked on its own against
facts that need no second implementation: the topology of a Moebius strip (Euler characteristic 0, ONE boundary loop), central
differences, the area of the parametrised surface, and div_G x = 2 for the position vector of the discrete surface."""
import pathlib

import numpy as np
import pytest

from proximalgalerkin_amd import lagrange, mesh_generation
from tests import eikonal_reference as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _corner_edges(cd, k):
    """(nc, 4, 2): the four edges of every cell as pairs of its corner dofs"""
    k1 = k + 1
    c = cd[:, [0, k, k1 * k1 - 1, k1 * k]]  # counter-clockwise in the reference square
    return np.stack([c, np.roll(c, -1, axis=1)], axis=2)


@pytest.mark.parametrize("size", [(3, 1), (5, 2), (8, 3)])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("source", ["package", "restatement"])
def test_numbering_is_a_moebius_strip(size, k, source):
    nu, nv = size
    n, cd = lagrange.numbering_mobius(nu, nv, k) if source == "package" else R.numbering(nu, nv, k)
    cd = np.asarray(cd, dtype=np.int64)
    assert cd.shape == (nu * nv, (k + 1) ** 2) and cd.min() == 0 and cd.max() == n - 1 and len(np.unique(cd)) == n
    assert all(len(set(row)) == len(row) for row in cd.tolist())  # every cell's dofs are distinct
    e = np.sort(_corner_edges(cd, k).reshape(-1, 2), axis=1)
    edges, cnt = np.unique(e, axis=0, return_counts=True)
    V, E, F = len(np.unique(e)), len(edges), nu * nv
    assert V - E + F == 0  # Euler characteristic of the Moebius strip (and of the cylinder: the loop count tells them apart)
    assert set(cnt.tolist()) <= {1, 2}  # an interior edge lies in exactly two cells
    bnd = edges[cnt == 1]
    assert len(bnd) == 2 * nu
    nbr = {}
    for a, b in bnd.tolist():
        nbr.setdefault(a, []).append(b)
        nbr.setdefault(b, []).append(a)
    assert all(len(v) == 2 for v in nbr.values())
    start = int(bnd[0, 0])
    prev, cur, steps = start, nbr[start][0], 1
    while cur != start:
        nxt = nbr[cur][0] if nbr[cur][0] != prev else nbr[cur][1]
        prev, cur, steps = cur, nxt, steps + 1
    assert steps == 2 * nu  # ONE closed loop through all boundary edges; a cylinder has two loops of nu


def test_package_numbering_and_nodes_equal_the_restatements():
    for nu, nv, g, scale in [(3, 1, 1, 1.0), (5, 2, 2, 2.0), (8, 3, 3, 0.5)]:
        mesh = mesh_generation.create_mobius_strip(nu, nv, g, scale)
        P = R.Eikonal(nu, nv, g, 2, scale=scale)
        for k, cdr in ((1, P.cd1), (2, P.cd2)):
            n, cd = lagrange.numbering_mobius(nu, nv, k)
            assert cd.dtype == np.int32 and np.array_equal(cd, cdr) and n == (P.n1 if k == 1 else P.n2)
        assert np.abs(mesh.cell_nodes - P.X).max() <= 1e-15 * scale


def test_bad_arguments_are_refused():
    for nu, nv in [(2, 1), (1, 3), (3, 0)]:
        with pytest.raises(ValueError):
            mesh_generation.create_mobius_strip(nu, nv)
        with pytest.raises(ValueError):
            lagrange.numbering_mobius(nu, nv, 1)
    with pytest.raises(ValueError):
        mesh_generation.create_mobius_strip(4, 1, order=4)
    with pytest.raises(ValueError):
        mesh_generation.create_mobius_strip(4, 1, scale=0.0)


@pytest.mark.parametrize("case", [(3, 1, 1, 1.0), (5, 2, 2, 2.0), (8, 3, 3, 1.0), (4, 3, 3, 0.5)])
def test_seam_geometry(case):
    """the geometry nodes two cells share are one point of R^3, also where the two cells reach it through different parameters"""
    nu, nv, g, scale = case
    mesh = mesh_generation.create_mobius_strip(nu, nv, g, scale)
    n, cd = lagrange.numbering_mobius(nu, nv, g)
    lo, hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    np.minimum.at(lo, cd.ravel(), mesh.cell_nodes.reshape(-1, 3))
    np.maximum.at(hi, cd.ravel(), mesh.cell_nodes.reshape(-1, 3))
    print(f"{case}: largest disagreement {np.abs(hi - lo).max():.2e}")
    assert np.abs(hi - lo).max() <= 1e-15 * scale
    seam = cd[nu - 1::nu]  # the cells of the last column hold nodes of column 0
    assert np.isin(seam, cd[0::nu]).any()


@pytest.mark.parametrize("case", [(3, 1, 1, 2, 0.5), (5, 2, 2, 5, 0.5), (4, 3, 3, 4, 30.0)])
def test_restatement_jacobian_matches_central_differences(case):
    nu, nv, g, nq, psi_scale = case
    P = R.Eikonal(nu, nv, g, nq, scale=1.3)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(P.ndofs)
    x[P.n1:] *= psi_scale
    xp = rng.standard_normal(P.ndofs)
    J = P.jacobian(x).toarray()
    assert np.array_equal(J, J.T) and not J[:P.n1, :P.n1].any()
    h = 1e-6
    worst = 0.0
    for _ in range(6):
        d = rng.standard_normal(P.ndofs)
        fd = (P.residual(x + h * d, xp, 3.0) - P.residual(x - h * d, xp, 3.0)) / (2 * h)
        worst = max(worst, np.linalg.norm(J @ d - fd) / np.linalg.norm(fd))
    print(f"{case}: Jacobian against central differences {worst:.2e}")
    assert worst <= 1e-7


def _exact_area(scale):
    """the area of the parametrised strip: the integral of |x_s x x_t| over [0, 2 pi] x [0, 1]"""
    from scipy import integrate

    def dA(t, s):
        rho = 0.5 * (t - 0.5)
        a = 1.0 + rho * np.cos(0.5 * s)
        xs = np.array([-0.5 * rho * np.sin(0.5 * s) * np.cos(s) - a * np.sin(s), -0.5 * rho * np.sin(0.5 * s) * np.sin(s) + a * np.cos(s),
                       0.5 * rho * np.cos(0.5 * s)])
        xt = 0.5 * np.array([np.cos(0.5 * s) * np.cos(s), np.cos(0.5 * s) * np.sin(s), np.sin(0.5 * s)])
        return np.linalg.norm(np.cross(xs, xt))

    val, err = integrate.dblquad(dA, 0.0, 2.0 * np.pi, 0.0, 1.0, epsabs=1e-13, epsrel=1e-13)
    assert err < 1e-11
    return scale * scale * val


@pytest.mark.parametrize("g", [1, 2, 3])
def test_area_converges_at_the_rate_of_the_geometry_order(g):
    """sum of w dS -> the area of the strip.  The Q_g interpolant moves the surface by O(h^(g+1)) and tilts it by O(h^g); the area
    changes at first order in the displacement and at second order in the tilt: O(h^min(g+1, 2g)) at least."""
    scale = 2.0
    exact = _exact_area(scale)
    err = [abs(R.Eikonal(nu, nv, g, 8, scale=scale).area() - exact) / exact for nu, nv in ((8, 1), (16, 2), (32, 4))]
    rates = [np.log2(err[i] / err[i + 1]) for i in range(2)]
    print(f"g = {g}: relative area errors {err}, rates {rates}")
    assert err[-1] < err[0] and min(rates) >= min(g + 1, 2 * g) - 0.25


def _position_dofs(P):
    """the discrete surface's position vector as a [Q2]^3 function (g <= 2: x_h is in the space): (3, n2)"""
    t = np.arange(3) / 2.0
    N, _ = R.tensor_tables(P.g, np.tile(t, 3), np.repeat(t, 3))  # the Q_g basis at the Q2 nodes of the reference cell
    Xq2 = np.einsum("bn,cni->cbi", N, P.X)  # (nc, 9, 3)
    out = np.full((3, P.n2), np.nan)
    for i in range(3):
        out[i, P.cd2.ravel()] = Xq2[:, :, i].ravel()
    assert np.all(np.isfinite(out))
    return out


@pytest.mark.parametrize("case", [(3, 1, 1, 3), (5, 2, 2, 5), (8, 3, 2, 6), (6, 1, 1, 2)])
def test_surface_divergence_of_the_position_vector_is_two(case):
    """div_G x = tr(P) = 2 on any surface: B x_h = 2 (1, v).  Pins K, dS and the seam (x_h is single-valued in R^3 although its
    parameters are not) without a second implementation."""
    nu, nv, g, nq = case
    P = R.Eikonal(nu, nv, g, nq, scale=1.7, f=1.0)
    lhs, rhs = P.B @ _position_dofs(P).ravel(), 2.0 * P.fv
    print(f"{case}: |B x - 2 (1, v)| / |2 (1, v)| = {np.linalg.norm(lhs - rhs) / np.linalg.norm(rhs):.2e}")
    assert np.linalg.norm(lhs - rhs) <= 1e-13 * np.linalg.norm(rhs)


SETTINGS = {"A": (8, 2, 3, 6, 1.0, 264), "B": (16, 4, 3, 6, 1.0, 944), "C": (6, 1, 2, 5, 2.0, 120)}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_goldens_reload_and_are_self_consistent(name):
    g = np.load(GOLDEN / f"eikonal_{name}.npz")
    nu, nv, go, nq1, scale, unknowns = SETTINGS[name]
    assert (int(g["nu"]), int(g["nv"]), int(g["g"]), int(g["nq1"]), float(g["scale"])) == (nu, nv, go, nq1, scale)
    n1, n2 = nu * (nv + 1), 2 * nu * (2 * nv + 1)
    assert n1 + 3 * n2 == unknowns and g["z"].shape == (unknowns,) and np.all(np.isfinite(g["z"]))
    log, inc, tol = g["log"], g["increments"], float(g["tol"])
    assert log.shape == (len(inc), 4) and tol == 1e-5
    assert np.array_equal(log[:, 0], np.arange(1, len(log) + 1))
    assert np.array_equal(log[:, 1], np.minimum(2.0 ** log[:, 0], 10.0))  # :152
    assert np.all(log[:, 2] >= 1) and np.all(log[:, 3] > 0)
    assert inc[-1] < 5 * tol and np.all(inc[:-1] >= 5 * tol)  # :173
    assert g["sensitivity"].shape == (2,) and np.all(g["sensitivity"] >= 0) and np.all(R.field_tolerances(g) < 1e-6)
    assert float(g["max_u"]) == g["z"][:n1].max() and 0.0 < float(g["max_u"]) <= 0.25 * scale + 1e-3  # the distance to the boundary
    P = R.Eikonal(nu, nv, go, nq1, scale=scale)
    assert P.ndofs == unknowns and abs(P.l2_increment_u(g["z"], np.zeros(unknowns)) ** 2 - g["z"][:n1] @ (P.M1 @ g["z"][:n1])) < 1e-14
