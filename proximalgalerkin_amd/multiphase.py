"""Example 04 - four-phase Cahn-Hilliard gradient flow with a simplex-constrained latent variable - on the HIP backend.
Host-side mirror of the reference's examples/04_multiphase/multiphase_dolfinx.py: `solve_problem` runs its time loop with
the LVPP iterations (:188-233) and `MultiphaseProblem` stands where the script builds
`dolfinx.fem.petsc.NonlinearProblem(F, u=sol, bcs=[], petsc_options=...)` (:127-147).  Everything below `.solve()`, and the
per-step vector updates, run in libpgx.so (include/pgx_mp.h); only scalars cross to the host, except at write steps.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib, fem
from ._mixed import _MixedHandle
from .problem import ConvergenceError, _SNES

NUM_SPECIES = 4
# the reference's solver parameters (:127-142); no snes_linesearch_type: PETSc's default bt of order 3
SP = {"snes_type": "newtonls", "snes_atol": 1e-8, "snes_rtol": 1e-8, "snes_max_it": 25, "ksp_type": "preonly", "pc_type": "lu",
      "snes_error_if_not_converged": True}


def _check_discretisation(primal_degree, cell_type):
    if cell_type == "quadrilateral":
        raise NotImplementedError("cell_type quadrilateral: the model's h = 2 Circumradius is defined on affine simplices only "
                                  "(UFL refuses it in the reference too)")
    if cell_type != "triangle":
        raise ValueError(f"cell_type {cell_type}")
    if int(primal_degree) != 1:
        raise NotImplementedError(f"primal_degree {primal_degree}: the example-04 kernels are written for P1 only")


def _markers():
    # :92-102, tolerances as written there (lower_right's `0.2 <= x[1] + tol` included)
    def rectangle(x, tol=1e-14):
        return (0.2 - tol <= x[1]) & (x[1] <= 0.75 + tol) & (0.2 - tol <= x[0]) & (x[0] <= 0.8 + tol)

    def lower_left(x, tol=1e-14):
        return (x[1] <= 0.5 + tol) & (0.2 - tol <= x[1]) & (0.2 - tol <= x[0]) & (x[0] <= 0.5 + tol)

    def lower_right(x, tol=1e-14):
        return (x[1] <= 0.5 + tol) & (0.2 <= x[1] + tol) & (0.5 - tol <= x[0]) & (x[0] <= 0.8 + tol)

    return rectangle, lower_left, lower_right


def initial_condition(mesh) -> np.ndarray:
    """u_prev of :118-122, [4 n_vertices] vertex-major: species 0 = 1 everywhere, then species 1, 2, 3 on the cells of the
    markers rectangle, lower_left, lower_right in that order.  A cell is marked only if all its vertices satisfy the marker
    (locate_entities); every vertex of a marked cell then takes the marker's unit vector (interpolate with cells0=)."""
    X = mesh.geometry.T
    u = np.zeros((mesh.num_vertices, NUM_SPECIES))
    u[:, 0] = 1.0
    for species, marker in zip((1, 2, 3), _markers()):
        ok = marker(X)
        cells = mesh.cells[np.all(ok[mesh.cells], axis=1)]
        v = np.unique(cells)
        u[v] = 0.0
        u[v, species] = 1.0
    return u.ravel()


class MultiphaseProblem(_MixedHandle):
    """x = [u | z | psi], each a P1 field of 4 species on `mesh`, vertex-major with the species fastest."""

    _prefix = "pgx_mp"

    def __init__(self, mesh: fem.Mesh, petsc_options: dict | None = None, tau=1e-5, eps=1e-9, device=0):
        if getattr(mesh, "cell_name", lambda: "triangle")() != "triangle":
            _check_discretisation(1, "quadrilateral")
        self._lib = lib = _lib.load()
        self.mesh = mesh
        self.nv = mesh.num_vertices
        self.ndofs = 3 * NUM_SPECIES * self.nv
        pts, wts = fem.quadrature_rule("triangle", 7)  # tri_deg7_gj16: UFL's degree estimate for the softmax term
        self._keep = (mesh.geometry, mesh.cells, pts, wts)
        pm = _lib.pgx_mesh(self.nv, mesh.num_cells, _lib.dptr(mesh.geometry), _lib.iptr(mesh.cells), 0, 0, None, 0)
        pp = _lib.pgx_mp_problem(len(wts), _lib.dptr(pts), _lib.dptr(wts), float(tau), float(eps))
        self._h = C.c_void_p()
        rc = lib.pgx_mp_create(C.byref(pm), C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_mp_last_error(None)
            raise _lib.PgxError(f"pgx_mp_create failed (code {rc}): {msg.decode() if msg else ''}")
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))
        self._opts.linesearch = 3  # PETSc's default: bt, order 3
        self._flags = {"snes_error_if_not_converged": False}
        for k, v in (SP if petsc_options is None else petsc_options).items():
            if k in ("snes_rtol", "snes_atol", "snes_stol"):
                setattr(self._opts, k, float(v))
            elif k == "snes_max_it":
                self._opts.snes_max_it = int(v)
            elif k == "snes_linesearch_type":
                if v not in ("bt", "none", "basic"):
                    raise NotImplementedError(f"snes_linesearch_type {v}")
                self._opts.linesearch = 3 if v == "bt" else 0
            elif k == "snes_linesearch_order":
                if int(v) not in (2, 3):
                    raise NotImplementedError("bt line search: order 2 or 3")
                if self._opts.linesearch:
                    self._opts.linesearch = 1 if int(v) == 2 else 3
            elif k == "snes_error_if_not_converged":
                self._flags[k] = bool(v) if v is not None else True
            elif k == "snes_monitor":
                self._opts.monitor = max(self._opts.monitor, 1)
        self._opts.ksp_max_it = 6
        self.solver = _SNES(self._opts)

    # -- the time loop's device-side updates -------------------------------------------------------------------------
    def set_uprev(self, u):
        self._call("set_uprev", _lib.dptr(np.ascontiguousarray(u, dtype=np.float64)))

    def get_uprev(self):
        u = np.empty(NUM_SPECIES * self.nv)
        self._call("get_uprev", _lib.dptr(u))
        return u

    def begin_step(self):
        """psi of the state and of the previous iterate <- ln(|u| + 1e-7) + 1, u of the previous iterate <- 0 (:194-200)"""
        self._call("begin_step")

    def end_step(self):
        """u_prev <- u (:226)"""
        self._call("end_step")

    def l2_increment(self):
        """||u - u_old||_L2 (:179-182, :212-213)"""
        return self._scalar("l2_increment")

    def species_mass(self):
        out = np.empty(NUM_SPECIES)
        self._call("species_mass", _lib.dptr(out))
        return out

    def lu_stats(self):
        st = _lib.pgx_nd_stats()
        self._check(self._lib.pgx_mp_lu_stats(self._h, C.byref(st)), "pgx_mp_lu_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}


def _alpha(scheme, i, alpha_0, alpha_c, alpha_max, current):
    if scheme == "constant":
        return current
    if scheme == "linear":
        return min(alpha_0 + alpha_c * i, alpha_max)
    if scheme == "doubling":
        return min(alpha_0 * 2**i, alpha_max)
    raise ValueError(f"alpha_scheme {scheme}")


def _write(result_dir: Path, mesh, step, t, u, psi):
    from . import io

    n = mesh.num_vertices
    io.write_vtu(result_dir / f"u_{step:06d}.vtu", mesh.geometry, mesh.cells, point_data={"u": u.reshape(n, NUM_SPECIES)})
    io.write_vtu(result_dir / f"psi_{step:06d}.vtu", mesh.geometry, mesh.cells, point_data={"psi": psi.reshape(n, NUM_SPECIES)})


def solve_problem(N: int = 50, M: int = 50, primal_degree: int = 1, cell_type: str = "triangle", alpha_max: float = 50.0,
                  alpha_scheme: str = "constant", alpha_0: float = 1.0, alpha_c: float = 1.0, max_iterations: int = 20,
                  stopping_tol: float = 1e-5, result_dir: Path | None = Path("results"), write_frequency: int = 25,
                  tau0: float = 1e-5, T: float = 7e-3, num_steps: int | None = None, verbose: bool = False,
                  return_solution: bool = False, profile: dict | None = None, device: int = 0):
    """The reference's solve_problem (:16-238) with its signature: returns (newton_iterations, lvpp_iterations), per time
    step; with return_solution=True also the final (u, psi).  `num_steps` cuts the run short (tests); result_dir=None
    writes nothing.  A `profile` dict receives the handle's timing split (MultiphaseProblem.profile) of the whole run.  u_prev and psi are written as VTU files every `write_frequency` steps (and at step 0) in place of the
    reference's VTX .bp output."""
    _check_discretisation(primal_degree, cell_type)
    if alpha_scheme not in ("constant", "linear", "doubling"):
        raise ValueError(f"alpha_scheme {alpha_scheme}")
    mesh = fem.create_unit_square(N, M, diagonal="crossed")
    problem = MultiphaseProblem(mesh, tau=tau0, device=device)
    try:
        n = NUM_SPECIES * problem.nv
        u0 = initial_condition(mesh)
        problem.set_uprev(u0)
        problem.set_alpha(alpha_0)
        if profile is not None:
            problem.profile(True)
        steps = int(np.ceil(T / tau0)) if num_steps is None else int(num_steps)
        newton = np.zeros(steps, dtype=np.int32)
        lvpp = np.zeros(steps, dtype=np.int32)
        if result_dir is not None:
            result_dir = Path(result_dir)
            _write(result_dir, mesh, 0, 0.0, u0, np.zeros(n))
        t = 0.0
        for j in range(1, steps + 1):
            if verbose:
                print(f"Step {j}/{steps}", flush=True)
            t += tau0
            problem.begin_step()
            i = 0
            for i in range(1, max_iterations + 1):
                a = _alpha(alpha_scheme, i, alpha_0, alpha_c, alpha_max, problem.alpha)
                if a != problem.alpha:
                    problem.set_alpha(a)
                problem.solve()  # raises ConvergenceError (snes_error_if_not_converged)
                its = problem.solver.getIterationNumber()
                newton[j - 1] += its
                diff = problem.l2_increment()
                if verbose:
                    print(f"Iteration {i}: converged={problem.solver.getConvergedReason()} alpha={problem.alpha:.2e} "
                          f"num_iterations={its} |delta u |= {diff}", flush=True)
                problem.advance_prev()  # u_old <- u, psi_old <- psi (:222-223)
                if diff < stopping_tol:
                    break
            problem.end_step()
            lvpp[j - 1] = i
            if result_dir is not None and j % write_frequency == 0:
                x = problem.get_state()
                _write(result_dir, mesh, j, t, x[:n], x[2 * n:])
        if profile is not None:
            profile.update(problem.profile(False))
        if verbose:
            print("Newton iterations:", newton)
            print("LVPP iterations:", lvpp)
        if return_solution:
            x = problem.get_state()
            return newton, lvpp, x[:n].copy(), x[2 * n:].copy()
        return newton, lvpp
    finally:
        problem.close()


__all__ = ["MultiphaseProblem", "initial_condition", "solve_problem", "ConvergenceError", "SP"]
