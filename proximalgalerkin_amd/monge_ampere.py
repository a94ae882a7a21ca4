"""Example 10 - the Monge-Ampere equation det D^2 u = rho through a three-field mixed discretisation with the matrix logarithm of the
Hessian as latent variable - on the HIP backend.  Host-side mirror of the reference's examples/10_monge_ampere/monge_ampere_dolfinx.py:
`p_refinement` is the script's loop (:31-169), `h_refinement` the script with its commented-out `refine` line (:169) enabled, and
`MongeAmpereProblem` stands where the script builds `dolfinx.fem.petsc.NonlinearProblem(F, u=z, bcs=[bc], petsc_options=sp)` (:151-153).
Everything below `.solve()` and the L2 error run in libpgx.so (include/pgx_ma.h); the Newton matrices are factorised by the dense LU
with partial pivoting of include/pgx_dn.h, because they are not quasi-definite.

Spaces (:51-55): u in P_k, p in [P_{k+1}]^2, Psi = (Psi00, Psi01, Psi11) in [P_k]^3, continuous; numbering and basis from
`lagrange.numbering` / `tabulate` (equispaced lattice: the deviation from Basix's GLL-warped nodes is documented there - the spanned
spaces are the same).  State x = [u | p0 | p1 | Psi00 | Psi01 | Psi11].  Quadrature: the collapsed Gauss-Jacobi rule of degree 4k + 4
unless given; what DOLFINx's own estimate for this form would be is not known here.  DEVIATION of `h_refinement` from the Firedrake
variant's hierarchy: Psi stays continuous (the variant uses a DG latent space).
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np

from . import _lib, fem, lagrange
from ._mixed import _MixedHandle
from .problem import _SNES

# the script's solver parameters (:15-23); rtol 1e-8, atol 1e-50, stol 1e-8, max_it 50 and divtol 1e4 are PETSc's defaults
SP = {"snes_linesearch_type": "l2"}


class NotConvergedError(Exception):
    pass


def u_exact(X, nonsmooth=False):
    """(:35-42)"""
    r2 = X[..., 0] ** 2 + X[..., 1] ** 2
    if nonsmooth:
        return np.where(r2 <= 0.25, 2.0 * r2, 2.0 * r2 + 2.0 * (np.sqrt(r2) - 0.5) ** 2)
    return np.exp(0.5 * r2)


def rho(X, nonsmooth=False):
    """det of the Hessian of u_exact (:47): (1 + |X|^2) exp(|X|^2); nonsmooth: 16 for |X| <= 1/2 and 8 (8 - 2 / |X|) outside"""
    r2 = X[..., 0] ** 2 + X[..., 1] ** 2
    if nonsmooth:
        r = np.sqrt(np.where(r2 <= 0.25, 1.0, r2))
        return np.where(r2 <= 0.25, 16.0, 8.0 * (8.0 - 2.0 / r))
    return (1.0 + r2) * np.exp(r2)


def ln_rho(X, nonsmooth=False):
    if nonsmooth:
        return np.log(rho(X, True))
    r2 = X[..., 0] ** 2 + X[..., 1] ** 2
    return r2 + np.log1p(r2)


class MongeAmpereProblem(_MixedHandle):
    """x = [u | p0 | p1 | Psi00 | Psi01 | Psi11] on the triangular `mesh`; u = g on `bc_dofs` (default: the exterior dofs of u with the
    exact solution's values, :88-97); `ln_rho_q` [nc][nq]: ln rho at the physical quadrature points (default: the script's data)."""

    _prefix = "pgx_ma"

    def __init__(self, mesh: fem.Mesh, degree: int, quadrature_degree: int | None = None, nonsmooth=False, ln_rho_q=None, bc_dofs=None,
                 g=None, petsc_options: dict | None = None, device=0):
        if int(degree) < 2:
            raise ValueError("degree k >= 2")
        self._lib = lib = _lib.load()
        self.mesh, self.k, self.nonsmooth = mesh, int(degree), bool(nonsmooth)
        self.quadrature_degree = 4 * self.k + 4 if quadrature_degree is None else int(quadrature_degree)
        k = self.k
        self.nu, cdu, self.Xu = lagrange.numbering(mesh, k)
        self.np_, cdp, self.Xp = lagrange.numbering(mesh, k + 1)
        self.cell_dofs_u, self.cell_dofs_p = np.ascontiguousarray(cdu, np.int32), np.ascontiguousarray(cdp, np.int32)
        nu, npp = self.nu, self.np_
        self.offsets = np.array([0, nu, nu + npp, nu + 2 * npp, 2 * nu + 2 * npp, 3 * nu + 2 * npp, 4 * nu + 2 * npp])
        self.ndofs = int(self.offsets[-1])
        pts, w = fem.quadrature_rule("triangle", self.quadrature_degree, "GJ")
        self.nq = len(w)
        Nu, Gu = lagrange.tabulate(k, pts)
        Np, Gp = lagrange.tabulate(k + 1, pts)
        V = mesh.geometry[mesh.cells]
        lam = np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1)
        self.Xq = np.einsum("qa,cad->cqd", lam, V)  # physical quadrature points (nc, nq, 2)
        assert np.all(rho(self.Xp, self.nonsmooth) > 0)  # (:63)
        if ln_rho_q is None:
            ln_rho_q = ln_rho(self.Xq, self.nonsmooth)
        if bc_dofs is None:
            bc_dofs = lagrange.exterior_dofs(mesh, k, self.cell_dofs_u)
            g = u_exact(self.Xu[bc_dofs], self.nonsmooth)
        self.bc_dofs = np.ascontiguousarray(bc_dofs, dtype=np.int32)
        self.g = np.ascontiguousarray(g, dtype=np.float64)
        coords = np.ascontiguousarray(mesh.geometry, dtype=np.float64)
        cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
        w = np.ascontiguousarray(w)
        tabs = [np.ascontiguousarray(Nu.T), np.ascontiguousarray(Gu.transpose(2, 1, 0)), np.ascontiguousarray(Np.T),
                np.ascontiguousarray(Gp.transpose(2, 1, 0))]  # [node][point], [direction][node][point]
        lr = np.ascontiguousarray(ln_rho_q, dtype=np.float64)
        assert lr.shape == (len(cells), self.nq)
        self._keep = (coords, cells, w, tabs, lr)
        pp = _lib.pgx_ma_problem(len(coords), len(cells), _lib.dptr(coords), _lib.iptr(cells), k, nu, npp, _lib.iptr(self.cell_dofs_u),
                                 _lib.iptr(self.cell_dofs_p), self.nq, _lib.dptr(w), _lib.dptr(tabs[0]), _lib.dptr(tabs[1]),
                                 _lib.dptr(tabs[2]), _lib.dptr(tabs[3]), _lib.dptr(lr), len(self.bc_dofs), _lib.iptr(self.bc_dofs),
                                 _lib.dptr(self.g))
        self._h = C.c_void_p()
        rc = lib.pgx_ma_create(C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_ma_last_error(None)
            raise _lib.PgxError(f"pgx_ma_create failed (code {rc}): {msg.decode() if msg else ''}")
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))  # rtol 1e-8, atol 1e-50, stol 1e-8, max_it 50, divtol 1e4: PETSc's defaults
        for key, v in (SP if petsc_options is None else petsc_options).items():
            if key in ("snes_rtol", "snes_atol", "snes_stol", "snes_divtol"):
                setattr(self._opts, key, float(v))
            elif key == "snes_max_it":
                self._opts.snes_max_it = int(v)
            elif key == "snes_linesearch_type":
                if v not in ("l2", "bt", "none", "basic"):
                    raise NotImplementedError(f"snes_linesearch_type {v}")
                self._opts.linesearch = {"l2": 2, "bt": 3}.get(v, 0)
            elif key == "snes_monitor":
                self._opts.monitor = max(self._opts.monitor, 1)
            elif key == "snes_linesearch_monitor":
                self._opts.monitor = 2
        self._opts.ksp_max_it = 6
        self.solver = _SNES(self._opts)

    def split(self, x):
        o = self.offsets
        return tuple(x[o[i]:o[i + 1]] for i in range(6))

    def l2_error(self, u_exact_q=None):
        """sqrt(assemble_scalar((u - u_exact)^2 dx)) (:161-163) of the state; u_exact_q [nc][nq] (default: the script's solution)"""
        ue = np.ascontiguousarray(u_exact(self.Xq, self.nonsmooth) if u_exact_q is None else u_exact_q, dtype=np.float64)
        assert ue.shape == self.Xq.shape[:2]
        out = C.c_double(0)
        self._call("l2_error", _lib.dptr(ue), C.byref(out))
        return out.value

    def lu_stats(self):
        """the dense LU's statistics of the last factorisation (include/pgx_dn.h)"""
        st = _lib.pgx_dn_stats()
        self._check(self._lib.pgx_ma_lu_stats(self._h, C.byref(st)), "pgx_ma_lu_stats")
        return {key: getattr(st, key) for key, _ in st._fields_}


def setup_problem(n, k, quadrature_degree=None, nonsmooth=False, petsc_options=None, device=0):
    """The script's problem on create_rectangle([[-1, -1], [1, 1]], n) (:12): rho and g from u_exact = exp(|X|^2 / 2), or the nonsmooth
    pair (:35-48)."""
    n = (int(n), int(n)) if np.isscalar(n) else (int(n[0]), int(n[1]))
    mesh = fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), n)
    return MongeAmpereProblem(mesh, k, quadrature_degree, nonsmooth, petsc_options=petsc_options, device=device)


def initial_state(problem: MongeAmpereProblem):
    """(:112-136): u, p = nodal interpolants of u_guess = c |X|^2 and of its gradient (c = 1; nonsmooth: 2); Psi = logm of the Hessian of
    the interpolated guess at the nodes - for k >= 2 the interpolant is the guess itself, so Psi = ln(2 c) I exactly."""
    c = 2.0 if problem.nonsmooth else 1.0
    z = np.zeros(problem.ndofs)
    o = problem.offsets
    z[o[0]:o[1]] = c * (problem.Xu[:, 0] ** 2 + problem.Xu[:, 1] ** 2)
    z[o[1]:o[2]] = 2.0 * c * problem.Xp[:, 0]
    z[o[2]:o[3]] = 2.0 * c * problem.Xp[:, 1]
    z[o[3]:o[4]] = np.log(2.0 * c)
    z[o[5]:o[6]] = np.log(2.0 * c)
    return z


def _locate(mesh, X):
    V = mesh.geometry[mesh.cells]
    Jc = np.stack([V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]], axis=2)
    xi = np.einsum("crd,pcd->pcr", np.linalg.inv(Jc), X[:, None, :] - V[None, :, 0, :])
    inside = (xi[..., 0] >= -1e-9) & (xi[..., 1] >= -1e-9) & (xi[..., 0] + xi[..., 1] <= 1.0 + 1e-9)
    cell = np.argmax(inside, axis=1)
    if not np.all(inside[np.arange(len(X)), cell]):
        raise ValueError("transfer: a point of the new mesh lies outside the previous mesh")
    return cell


def transfer(prev_problem: MongeAmpereProblem, z_prev, problem: MongeAmpereProblem):
    """Every sub-function of the previous solution evaluated at the new space's nodes (:100-110), cell by cell of the NEW mesh with
    `tabulate(..., snap=True)`: valid when the degree changes on one mesh, and when n doubles (the right-diagonal meshes are nested)."""
    new, prev = problem, prev_problem
    parent = _locate(prev.mesh, new.mesh.geometry[new.mesh.cells].mean(axis=1))
    Vp = prev.mesh.geometry[prev.mesh.cells][parent]
    Ji = np.linalg.inv(np.stack([Vp[:, 1] - Vp[:, 0], Vp[:, 2] - Vp[:, 0]], axis=2))
    out = np.zeros(new.ndofs)
    spaces = {0: (new.k, prev.k, new.cell_dofs_u, prev.cell_dofs_u, new.Xu), 1: (new.k + 1, prev.k + 1, new.cell_dofs_p, prev.cell_dofs_p, new.Xp)}
    for c in range(len(new.mesh.cells)):
        for blk in range(6):
            _, kp, cdn, cdo, Xn = spaces[1 if blk in (1, 2) else 0]
            xi = (Xn[cdn[c]] - Vp[c, 0]) @ Ji[c].T
            N, _ = lagrange.tabulate(kp, xi, snap=True)
            out[new.offsets[blk] + cdn[c]] = N @ z_prev[prev.offsets[blk] + cdo[parent[c]]]
    return out


def run_levels(levels, nonsmooth=False, snes_opts=None, profile: dict | None = None, device=0, verbose=False, return_last=False):
    """levels: [(n, k, quadrature_degree or None), ...]: the first starts from `initial_state`, the others from the transferred solution
    of the one before.  -> dict(errors, newton_its, reasons, ndofs, states); raises NotConvergedError on a level that did not converge
    (:158).  `profile`: a dict that receives per level N, Newton steps and the device-event ms of the phases."""
    errors, its_, reasons, ndofs, states = [], [], [], [], []
    prev, z, problem = None, None, None
    for n, k, deg in levels:
        problem = setup_problem(n, k, deg, nonsmooth, petsc_options=snes_opts, device=device)
        z = initial_state(problem) if prev is None else transfer(prev, z, problem)
        problem.set_state(z)
        if profile is not None:
            problem.profile(True)
        reason, its = problem.solve()
        if verbose:
            print(f"Converged reason: {reason}, iterations: {its}", flush=True)
        if profile is not None:
            ms = problem.profile(False)
            N = problem.ndofs
            profile.setdefault("levels", []).append(dict(n=list(problem.mesh.structured), k=k, N=N, points=problem.nq, newton_its=its,
                                                          reason=reason, ms=ms, lu=problem.lu_stats(),
                                                          factor_flops_per_step=2.0 * N ** 3 / 3.0))
        if reason <= 0:
            raise NotConvergedError(f"Solver did not converge: reason {reason} after {its} iterations (n = {n}, k = {k})")
        z = problem.get_state()
        errors.append(problem.l2_error()), its_.append(its), reasons.append(reason), ndofs.append(problem.ndofs), states.append(z)
        if prev is not None:
            prev.close()
        prev = problem
    out = dict(errors=errors, newton_its=its_, reasons=reasons, ndofs=ndofs, states=states)
    if return_last:
        out["problem"] = problem
    elif problem is not None:
        problem.close()
    return out


def p_refinement(k_min=3, k_max=14, n=2, nonsmooth=False, **kw):
    """The script's loop (:31): degrees k_min .. k_max on one n x n mesh of [-1, 1]^2, each warm-started from the one before.  The
    equispaced lattice basis converges to k = 14 (measured with the numpy restatement: DESIGN.md section 12e)."""
    return run_levels([(n, k, None) for k in range(k_min, k_max + 1)], nonsmooth=nonsmooth, **kw)


def h_refinement(k=4, levels=(2, 4, 8), nonsmooth=False, **kw):
    """The script with its `refine` line (:169) enabled: one degree, n doubling; Psi stays continuous (see the module docstring)."""
    return run_levels([(n, k, None) for n in levels], nonsmooth=nonsmooth, **kw)


def write_profile(path, profile: dict):
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(profile, indent=1) + "\n")
