"""Example 05, solver comparison - the thermoforming quasi-variational inequality by Moreau-Yosida path following and by a
fixed point in the mould temperature - on the HIP backend.  Host-side mirrors of the reference's
examples/05_obstacle_type_qvi/solver_comparison/thermoforming_moreau_yosida.jl ("MY" below) and thermoforming_fixed_point.jl
("FP"), two flat Julia scripts on Gridap + NLsolve: `PenalisedThermoformingProblem` stands where they build their FEOperators
(MY:129, FP:70-71), `solve_moreau_yosida` is the loop MY:121-157 and `solve_fixed_point` the loop FP:87-146.  Everything below
their `solve!` runs in libpgx.so (include/pgx_qmy.h).

The third script of that directory, thermoforming_semismooth_active_set.jl, only calls the package SemismoothQVIs.jl, whose
source is not part of the reference: it has no counterpart here.

The scripts' algorithm is kept as it is: the line search BackTracking(c_1=-1e8) accepts every finite trial, so the Newton
iteration is undamped, and at large gamma it may run into `max_newton` without converging.  That is not an error - Gridap's
`solve!` does not look at NLsolve's convergence flag - and the loops go on.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib, fem
from ._mixed import _MixedHandle

XTOL = 10 * np.finfo(np.float64).eps  # MY:130, FP:118,121
C1 = -1.0e8  # MY:130 LineSearches.BackTracking(c_1=-1e8)


def initial_mould(x):  # MY:40
    return 1.0 - 2.0 * np.maximum(np.abs(x[:, 0] - 0.5), np.abs(x[:, 1] - 0.5))


def smoothing(x):  # MY:42
    return np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])


def update_gamma_moreau_yosida(gamma, k, infeasibility, functional, warn=None):
    """MY:99-119 with both guards; Julia's `functional ≈ 0` has no absolute tolerance, so it holds for an exact zero only."""
    if functional == 0:  # MY:104-107
        if warn:
            warn(f"Energy functional is (near) zero; cannot update gamma reliably. Keeping gamma = {gamma}.")
        return gamma
    gamma_new = update_gamma_fixed_point(gamma, k, infeasibility, functional)
    if not np.isfinite(gamma_new) or gamma_new <= 0:  # MY:114-117
        if warn:
            warn(f"gamma update produced invalid value ({gamma_new}); keeping gamma = {gamma}.")
        return gamma
    return gamma_new


def update_gamma_fixed_point(gamma, k, infeasibility, functional):
    """FP:75-85 as it stands - no guards; IEEE arithmetic like Julia's (0/0 is NaN, not an exception)."""
    with np.errstate(all="ignore"):
        gamma, infeasibility, functional = np.float64(gamma), np.float64(infeasibility), np.float64(functional)
        E = gamma * infeasibility / functional
        theta = functional + infeasibility
        C2 = E * (E + gamma) * theta / gamma
        C1k = C2 / E
        tau = np.float64(1.0) / k
        return float(C2 / (tau * abs(C1k - theta)) - E)


class PenalisedThermoformingProblem(_MixedHandle):
    """x = [u | T], both P1 on `mesh`; u = 0 on the boundary (MY:27-33).  The mould, the smoothing function and the load are
    interpolated into P1 as the scripts do (MY:40-44)."""

    _prefix = "pgx_qmy"

    def __init__(self, mesh: fem.Mesh, q=0.01, f=25.0, quadrature_degree=11, device=0):
        if getattr(mesh, "curved", False):
            raise NotImplementedError("example 05 integrates on affine cells: pass mesh.flattened()")
        self._lib = lib = _lib.load()
        self.mesh = mesh
        self.nv = mesh.num_vertices
        self.ndofs = 2 * self.nv
        # Measure(Omega, 11) (MY:37).  Which rule Gridap takes for degree 11 on a triangle is not pinned here: this is the
        # collapsed Gauss-Jacobi rule of that degree, 36 points.
        pts, wts = fem.quadrature_rule("triangle", quadrature_degree, "GJ")
        bc = np.ascontiguousarray(mesh.exterior_dofs(1), dtype=np.int32)  # MY:27 dirichlet_tags="boundary"
        Phi0 = np.ascontiguousarray(initial_mould(mesh.geometry))
        phi = np.ascontiguousarray(smoothing(mesh.geometry))
        self._keep = (mesh.geometry, mesh.cells, pts, wts, bc, Phi0, phi)
        pm = _lib.pgx_mesh(self.nv, mesh.num_cells, _lib.dptr(mesh.geometry), _lib.iptr(mesh.cells), 0, 0, None, 0)
        pp = _lib.pgx_qmy_problem(len(wts), _lib.dptr(pts), _lib.dptr(wts), _lib.dptr(Phi0), _lib.dptr(phi), float(f), float(q),
                                  len(bc), _lib.iptr(bc))
        self._h = C.c_void_p()
        rc = lib.pgx_qmy_create(C.byref(pm), C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_qmy_last_error(None)
            raise _lib.PgxError(f"pgx_qmy_create failed (code {rc}): {msg.decode() if msg else ''}")
        self.gamma, self.active = 1.0, 3

    # the family has gamma and the active mask where the LVPP families have alpha
    def set_alpha(self, a):
        raise NotImplementedError("the penalised problem has no proximal parameter: set_gamma")

    def set_gamma(self, gamma):
        self._call("set_gamma", float(gamma))
        self.gamma = float(gamma)

    def set_active(self, mask):
        """bit 0 = u, bit 1 = T: 3 the coupled operator (MY:129), 2 opT and 1 opu of the fixed point (FP:70-71)"""
        self._call("set_active", int(mask))
        self.active = int(mask)

    def residual_inf(self, x=None):
        out = C.c_double(0)
        self._call("residual_inf", None if x is None else _lib.dptr(np.ascontiguousarray(x, dtype=np.float64)), C.byref(out))
        return out.value

    def solve(self, ftol=1e-5, xtol=XTOL, max_it=1000, c1=C1, monitor=0):
        """solve!(zh, solver, op) (MY:139): returns (reason, Newton iterations, LU solves); reason 0 = max_it reached, which the
        scripts do not treat as a failure."""
        o = _lib.pgx_qmy_newton_opts(float(ftol), float(xtol), float(c1), int(max_it), int(monitor))
        reason, its, lin = C.c_int(0), C.c_int(0), C.c_int(0)
        self._call("newton_solve", C.byref(o), C.byref(reason), C.byref(its), C.byref(lin))
        if reason.value < 0:  # NLsolve raises on a non-finite residual (check_isfinite)
            raise ArithmeticError(f"Newton: no finite trial residual after {its.value} iterations (gamma = {self.gamma})")
        return reason.value, its.value, lin.value

    def functionals(self):
        """(sum(energy(uh)), sum(penalty(uh, Th))) (MY:97-98,101-102) at the state, with the current gamma"""
        e, p = C.c_double(0), C.c_double(0)
        self._call("functionals", C.byref(e), C.byref(p))
        return e.value, p.value

    def cauchy(self):
        """sqrt(d' J d), d = u - u_prev on the free dofs, J the H1 matrix (MY:92-94,144-145)"""
        return self._scalar("cauchy")

    def lu_stats(self):
        st = _lib.pgx_nd_stats()
        self._check(self._lib.pgx_qmy_lu_stats(self._h, C.byref(st)), "pgx_qmy_lu_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}  # perturbed_pivots: of the last completed factorisation


def _initial_state(problem):
    x0 = np.zeros(problem.ndofs)
    x0[problem.nv:] = 1.0  # MY:122-124, FP:114-116: u = 0, T = 1
    return x0


def solve_moreau_yosida(M: int = 150, gamma0: float = 1.0, tol: float = 1e-5, max_outer: int = 100, ftol: float = 1e-5,
                        max_newton: int = 1000, verbose: bool = True, return_solution: bool = False, monitor=None,
                        device: int = 0):
    """The script's body (MY:121-157).  Returns a dict: "gammas" (the gamma of each outer step), "newton_its", "reasons",
    "cauchy", "seconds", "stopped" (None, or why the loop ended early: no finite Newton trial) [, "x"]."""
    say = print if verbose else (lambda *a, **k: None)
    problem = PenalisedThermoformingProblem(fem.create_unit_square(M, M), device=device)  # MY:17-20
    problem.set_state(_initial_state(problem))
    problem.advance_prev()  # MY:128 zh_ = copy_z(zh)
    problem.set_active(3)
    gamma = float(gamma0)  # MY:134
    gammas, newton_its, reasons, cauchy, stopped = [], [], [], [], None
    t0 = time.perf_counter()
    for j in range(1, max_outer + 1):  # MY:135
        say(f"Considering gamma = {gamma}.", flush=True)
        problem.set_gamma(gamma)
        try:
            reason, its, _ = problem.solve(ftol=ftol, max_it=max_newton)  # MY:139
        except ArithmeticError as e:  # where NLsolve would throw: report and end the loop, the counts so far stand
            stopped = str(e)
            say(f"Stopping: {stopped}", flush=True)
            break
        gammas.append(gamma), newton_its.append(its), reasons.append(reason)
        cauchy.append(problem.cauchy())  # MY:144-145
        say(f"Cauchy norm: {cauchy[-1]}." + ("" if reason else f"  (Newton stopped at its cap of {max_newton})"), flush=True)
        problem.advance_prev()  # MY:147
        if monitor is not None:
            monitor(problem, j)
        functional, infeasibility = problem.functionals()
        say(f"         infeasibility: {infeasibility}, functional: {functional}.", flush=True)
        gamma = update_gamma_moreau_yosida(gamma, j + 1, infeasibility, functional, warn=say)  # MY:150
        if cauchy[-1] < tol:  # MY:153-155
            break
    out = {"gammas": gammas, "newton_its": newton_its, "reasons": reasons, "cauchy": cauchy, "seconds": time.perf_counter() - t0,
           "stopped": stopped}
    say(f"Run time(s): {out['seconds']}, moreau-yosida its: {len(newton_its)}, linear system solves: {sum(newton_its)}")  # MY:157
    if return_solution:
        out["x"] = problem.get_state()
    problem.close()
    return out


def solve_fixed_point(M: int = 150, tol: float = 1e-5, max_outer: int = 10_000, gamma_max: float = 1e11, ftol_u: float = 1e-5,
                      ftol_T: float = 1e-10, max_newton: int = 1000, max_inner: int = 100, verbose: bool = True,
                      return_solution: bool = False, device: int = 0):
    """The script's body (FP:87-146).  Returns a dict: "newton_its_T" (per outer step), "inner_steps" (path-following steps per
    outer step), "newton_its_u" (per outer step, a list per inner step), "inner_gammas", "reasons_u", "cauchy", "seconds", "stopped" (None, or why the
    loops ended early) [, "x"]."""
    say = print if verbose else (lambda *a, **k: None)
    problem = PenalisedThermoformingProblem(fem.create_unit_square(M, M), device=device)  # FP:11-14
    problem.set_state(_initial_state(problem))
    nv = problem.nv
    u_outer = np.zeros(nv)  # FP:115 uh_
    its_T, inner_steps, its_u, inner_gammas, reasons_u, cauchy, stopped = [], [], [], [], [], [], None
    t0 = time.perf_counter()
    for j in range(1, max_outer + 1):  # FP:128
        say(f"Considering Fixed Point Iteration: {j}. \n     Solving for T.", flush=True)
        problem.set_active(2)
        _, n_T, _ = problem.solve(ftol=ftol_T, max_it=max_newton)  # FP:131
        its_T.append(n_T)
        say("     Solving for u.", flush=True)
        problem.set_active(1)
        gamma = 1.0  # FP:135
        step_its, step_gammas, step_reasons = [], [], []
        problem.advance_prev()  # FP:89 u_ = u.free_values[:]
        for k in range(1, max_inner + 1):  # FP:90
            say(f"         Considering gamma={gamma}.", flush=True)
            problem.set_gamma(gamma)
            try:
                reason, n_u, _ = problem.solve(ftol=ftol_u, max_it=max_newton)  # FP:92
            except ArithmeticError as e:  # where NLsolve would throw: report and end both loops, the counts so far stand
                stopped = str(e)
                say(f"Stopping: {stopped}", flush=True)
                break
            step_its.append(n_u), step_gammas.append(gamma), step_reasons.append(reason)
            c = problem.cauchy()  # FP:94-95
            say(f"         Cauchy norm: {c}.", flush=True)
            problem.advance_prev()  # FP:97
            if c < tol:  # FP:99-101
                break
            functional, infeasibility = problem.functionals()
            say(f"         infeasibility: {infeasibility}, functional: {functional}.", flush=True)
            gamma = update_gamma_fixed_point(gamma, k + 1, infeasibility, functional)  # FP:103
            if gamma > gamma_max:  # FP:105-107
                break
            if not np.isfinite(gamma) or gamma <= 0:
                # the script would hand this gamma to the next solve!, where NLsolve raises on the non-finite residual
                stopped = f"the unguarded gamma update (FP:75-85) produced {gamma}"
                say(f"Stopping: {stopped}", flush=True)
                break
        its_u.append(step_its), inner_steps.append(len(step_its)), inner_gammas.append(step_gammas), reasons_u.append(step_reasons)
        if stopped:
            break
        x = problem.get_state()
        prev = x.copy()
        prev[:nv] = u_outer
        problem.set_prev(prev)
        cauchy.append(problem.cauchy())  # FP:138-139
        say(f"Cauchy norm: {cauchy[-1]}.", flush=True)
        u_outer = x[:nv].copy()  # FP:141
        if cauchy[-1] < tol:  # FP:142-144
            break
    out = {"newton_its_T": its_T, "inner_steps": inner_steps, "newton_its_u": its_u, "inner_gammas": inner_gammas,
           "reasons_u": reasons_u, "cauchy": cauchy, "seconds": time.perf_counter() - t0, "stopped": stopped}
    solves = sum(its_T) + sum(sum(s) for s in its_u)
    say(f"Run time(s): {out['seconds']}, fixed point its: {len(cauchy)}, linear system solves: {solves}")  # FP:146
    if return_solution:
        out["x"] = problem.get_state()
    problem.close()
    return out
