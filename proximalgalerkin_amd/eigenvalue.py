"""Example 07 - a 2-D Landau-de Gennes Q-tensor whose eigenvalues are kept inside an interval through a tensor-valued latent variable -
on the HIP backend.  Host-side mirror of the reference's examples/07_eigenvalue_constraints/eigenvalue_constraints_dolfinx.py:
`solve_problem` runs its LVPP loop with the alpha halving on failure (:162-227), and `EigenvalueProblem` stands where the script
builds `dolfinx.fem.petsc.NonlinearProblem(F, u=z, bcs=bcs, petsc_options=sp, ...)` (:158-160, :172-174).  Everything below
`.solve()`, the copies between z and z_iter, the norm of the increment and the nodal post-processing run in libpgx.so
(include/pgx_ev.h); only scalars cross to the host, except for the final fields.

The conforming map is the script's `0.5 * tanh(Psi / 2)` with the script's own `tanh` (:31-33), which is TWICE the matrix hyperbolic
tangent: the eigenvalues of the conforming approximation lie in (-1, 1).

Dofs are the points of the p-times refined vertex lattice (lagrange.numbering_quad, equispaced nodes).  Basix places the nodes of
degree 3 at the Gauss-Lobatto-Legendre points; the spanned space is the same.  The Dirichlet data (:92-122) are linear on every cell
edge when d N is an integer (the ramps end on cell boundaries; the script's d = 0.06 with N = 100 is such a pair), and then their
interpolant is the same function for every node family; for other (d, N) the interpolants of the two families differ in the cells that
hold a kink of the ramp.  (d = 1/2 is a corner case of the script's T(z): its two ramp intervals overlap at z = 1/2, where it returns 2.)
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib, fem, lagrange
from ._mixed import _MixedHandle
from .problem import _SNES

# the script's solver parameters (:143); rtol 1e-8, atol 1e-50, stol 1e-8, max_it 50 and divtol 1e4 are PETSc's defaults
SP = {"snes_linesearch_type": "l2"}


class NotConvergedError(Exception):
    pass


def ramp(z, d):
    """T(z) (:98-106)"""
    eps = np.finfo(np.float64).eps
    assert ((0 <= z + eps) & (z - eps <= 1)).all(), "Invalid range on variable expected to be in [0, 1]"
    interval1 = (0 <= z + eps) & (z - eps < d)
    interval3 = (1 - d <= z + eps) & (z - eps <= 1)
    interval2 = np.invert(interval1) & np.invert(interval3)
    return interval1 * z / d + 1 * interval2 + (1 - z) / d * interval3


def boundary_data(x, y, d=0.06, theta_tb=0.0, theta_lr=np.pi / 2):
    """(g_xx, g_xy) of Robinson et al. at boundary points of the unit square (:86-122)"""
    top_bottom = np.isclose(y, 0) | np.isclose(y, 1)
    left_right = np.isclose(x, 0) | np.isclose(x, 1)
    s = ramp(y, d) * left_right + ramp(x, d) * top_bottom
    tht = theta_lr * left_right + theta_tb * top_bottom
    return 1 / 2 * s * np.cos(2 * tht), 1 / 2 * s * np.sin(2 * tht)


class EigenvalueProblem(_MixedHandle):
    """x = [q1 | q2 | psi1 | psi2], each a Q_degree field on the quadrilateral `mesh` (fem.QuadMesh); q1 = g1, q2 = g2 on `bc_dofs`
    (default: the whole boundary with the script's data of ramp width d)."""

    _prefix = "pgx_ev"

    def __init__(self, mesh: fem.QuadMesh, degree=3, quadrature_degree=20, A=1.0, C_=4.0, d=0.06, bc_dofs=None, g1=None, g2=None,
                 petsc_options: dict | None = None, device=0):
        if mesh.cell_name() != "quadrilateral":
            raise NotImplementedError("example 07 runs on the structured quadrilateral mesh (:42-44)")
        if int(degree) not in (1, 2, 3):
            raise NotImplementedError(f"degree {degree}: the example-07 kernels are written for Q1, Q2 and Q3 (:46)")
        nq = int(quadrature_degree) // 2 + 1  # the tensor Gauss rule exact to that degree in each variable (:70)
        if not 1 <= nq <= 11:
            raise NotImplementedError(f"quadrature_degree {quadrature_degree}: at most 21 (11 points per direction)")
        self._lib = lib = _lib.load()
        self.mesh, self.degree = mesh, int(degree)
        self.n, self.cell_dofs, self.dof_coordinates = lagrange.numbering_quad(mesh, self.degree)
        self.ndofs = 4 * self.n
        t, w = np.polynomial.legendre.leggauss(nq)
        t, w = np.ascontiguousarray(0.5 * (t + 1.0)), np.ascontiguousarray(0.5 * w)
        if bc_dofs is None:
            bc_dofs = lagrange.exterior_dofs_quad(mesh, self.degree)  # :125-137
            g1, g2 = boundary_data(self.dof_coordinates[bc_dofs, 0], self.dof_coordinates[bc_dofs, 1], d)  # :130, :139
        self.bc_dofs = np.ascontiguousarray(bc_dofs, dtype=np.int32)
        self.g1, self.g2 = np.ascontiguousarray(g1, dtype=np.float64), np.ascontiguousarray(g2, dtype=np.float64)
        self._keep = (t, w, self.bc_dofs, self.g1, self.g2)
        (x0, y0), (x1, y1) = mesh.box
        nx, ny = mesh.structured
        pp = _lib.pgx_ev_problem(nx, ny, x0, y0, x1, y1, self.degree, nq, _lib.dptr(t), _lib.dptr(w), float(A), float(C_),
                                 len(self.bc_dofs), _lib.iptr(self.bc_dofs), _lib.dptr(self.g1), _lib.dptr(self.g2))
        self._h = C.c_void_p()
        rc = lib.pgx_ev_create(C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_ev_last_error(None)
            raise _lib.PgxError(f"pgx_ev_create failed (code {rc}): {msg.decode() if msg else ''}")
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))  # rtol 1e-8, atol 1e-50, stol 1e-8, max_it 50, divtol 1e4: PETSc's defaults
        for k, v in (SP if petsc_options is None else petsc_options).items():
            if k in ("snes_rtol", "snes_atol", "snes_stol", "snes_divtol"):
                setattr(self._opts, k, float(v))
            elif k == "snes_max_it":
                self._opts.snes_max_it = int(v)
            elif k == "snes_linesearch_type":
                if v not in ("l2", "bt", "none", "basic"):
                    raise NotImplementedError(f"snes_linesearch_type {v}")
                self._opts.linesearch = {"l2": 2, "bt": 3}.get(v, 0)
            elif k == "snes_monitor":
                self._opts.monitor = max(self._opts.monitor, 1)
            elif k == "snes_linesearch_monitor":
                self._opts.monitor = 2
        self._opts.ksp_max_it = 6
        self.solver = _SNES(self._opts)

    def state_from_prev(self):
        """z.interpolate(z_iter) (:195)"""
        self._call("state_from_prev")

    def l2_increment_Q(self):
        """sqrt(assemble(inner(Q - Q_iter, Q - Q_iter) dx)) (:157, :209)"""
        return self._scalar("l2_increment_q")

    def eval_nodes(self):
        """(4, n): ConformingApproximation (T1, T2), MaximumEigenvalue, MinimumEigenvalue per dof (:245-259)"""
        out = np.empty((4, self.n))
        self._call("eval_nodes", _lib.dptr(out))
        return out

    def lu_stats(self):
        st = _lib.pgx_nd_stats()
        self._check(self._lib.pgx_ev_lu_stats(self._h, C.byref(st)), "pgx_ev_lu_stats")
        out = {k: getattr(st, k) for k, _ in st._fields_}  # perturbed_pivots: of the last completed factorisation
        out["symmetric"] = bool(self._lib.pgx_ev_lu_is_symmetric(self._h))  # L D L^T in LU clothing: about half of `flops` executed
        return out


def _write(result_dir: Path, problem, fields):
    """t.bp and m_plus.bp of the script (:261-265) as one VTU on the dof lattice, two triangles per lattice square"""
    from . import io

    nx, ny = problem.mesh.structured
    Lx, Ly = problem.degree * nx + 1, problem.degree * ny + 1
    v0 = (np.repeat(np.arange(Ly - 1), Lx - 1) * Lx + np.tile(np.arange(Lx - 1), Ly - 1)).astype(np.int32)
    tri = np.concatenate([np.stack([v0, v0 + 1, v0 + Lx + 1], axis=1), np.stack([v0, v0 + Lx + 1, v0 + Lx], axis=1)])
    result_dir.mkdir(parents=True, exist_ok=True)
    names = {"q1": "q1", "q2": "q2", "psi1": "psi1", "psi2": "psi2", "conforming1": "ConformingApproximation1",
             "conforming2": "ConformingApproximation2", "m_plus": "MaximumEigenvalue", "m_minus": "MinimumEigenvalue"}
    io.write_vtu(result_dir / "Q.vtu", problem.dof_coordinates, tri, point_data={v: fields[k] for k, v in names.items()})


def solve_problem(N: int = 100, degree: int = 3, quadrature_degree: int = 20, A: float = 1.0, C: float = 4.0, d: float = 0.06,
                  nfail_max: int = 50, nlvpp_max: int = 100, r: float = 2, snes_opts: dict | None = None, profile: dict | None = None,
                  result_dir: Path | None = None, verbose: bool = False, monitor=None, device: int = 0):
    """The script's body (:41-265) on the handle.  Returns (fields, log, newton_iterations): `fields` holds the final q1, q2, psi1,
    psi2, the nodal conforming1, conforming2, m_plus, m_minus (:245-259) and the dof coordinates x; log rows are
    (nlvpp at the attempt, alpha, Newton iterations, converged reason, failed); newton_iterations lists the Newton steps of the
    successful LVPP steps (the script prints their number, sum, minimum and maximum, :230-240).  `snes_opts` replaces the script's
    options (SP).  A `profile` dict receives the handle's timing split of the whole run; `monitor(problem, nlvpp)` is called after
    every attempt (tests)."""
    mesh = fem.create_unit_square(N, N, cell_type="quadrilateral")
    problem = EigenvalueProblem(mesh, degree, quadrature_degree, A=A, C_=C, d=d, petsc_options=snes_opts, device=device)
    z_prev = np.zeros(problem.ndofs)  # never written by the script (:60): a failed first step restarts from zero (:192-193)
    log, newton = [], []
    try:
        if profile is not None:
            problem.profile(True)
        alpha, nfail, nlvpp = 1.0, 0, 0
        num_iterations, converged_reason = -1, -1
        while nfail < nfail_max and nlvpp < nlvpp_max:
            if verbose:
                print(f"Attempting nlvpp={nlvpp} alpha={alpha}", flush=True)
            try:
                problem.set_alpha(alpha)
                problem.solve()  # :175
                num_iterations = problem.solver.getIterationNumber()
                converged_reason = problem.solver.getConvergedReason()
                if monitor is not None:
                    monitor(problem, nlvpp)
                if num_iterations == 0 and converged_reason > 0:  # :178-182
                    raise NotConvergedError("Not converged")
                if converged_reason < 0:
                    raise NotConvergedError("Not converged")
            except NotConvergedError:
                nfail += 1
                log.append((nlvpp, alpha, num_iterations, converged_reason, 1))
                if verbose:
                    print(f"Failed to converge, nlvpp={nlvpp} alpha={alpha}", flush=True)
                alpha /= 2  # :191
                if nlvpp == 0:
                    problem.set_state(z_prev)  # :193
                else:
                    problem.state_from_prev()  # :195
                if nfail >= nfail_max:
                    if verbose:
                        print(f"Giving up. alpha={alpha} nlvpp={nlvpp}", flush=True)
                    break
                continue
            log.append((nlvpp, alpha, num_iterations, converged_reason, 0))
            newton.append(num_iterations)
            nlvpp += 1
            nrm = problem.l2_increment_Q()  # :209
            if verbose:
                print(f"Solved nlvpp={nlvpp} alpha={alpha} ||Q_{nlvpp} - Q_{nlvpp - 1}|| = {nrm}", flush=True)
            if nrm < 1.0e-10:  # :215
                break
            if num_iterations <= 4:  # :219-222
                alpha *= r
            elif num_iterations >= 10:
                alpha /= r
            problem.advance_prev()  # :225
        if verbose and newton:
            print(f"#LVPP iterations {len(newton)}", f"#Newton iterations {sum(newton)}", flush=True)
            print(f"Min/Max Newton iterations {min(newton)}/{max(newton)}", flush=True)
        if profile is not None:
            profile.update(problem.profile(False))
            profile["lu"] = problem.lu_stats()
        x, n = problem.get_state(), problem.n
        nodes = problem.eval_nodes()
        fields = dict(q1=x[:n].copy(), q2=x[n:2 * n].copy(), psi1=x[2 * n:3 * n].copy(), psi2=x[3 * n:].copy(), conforming1=nodes[0],
                      conforming2=nodes[1], m_plus=nodes[2], m_minus=nodes[3], x=problem.dof_coordinates)
        if result_dir is not None:
            _write(Path(result_dir), problem, fields)
        return fields, np.array(log, dtype=np.float64).reshape(-1, 5), np.array(newton, dtype=np.int32)
    finally:
        problem.close()


__all__ = ["EigenvalueProblem", "solve_problem", "boundary_data", "ramp", "NotConvergedError", "SP"]
