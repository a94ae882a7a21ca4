"""Example 09 - the eikonal equation on a Moebius strip, a surface PDE on quadrilaterals embedded in R^3 - on the HIP backend.
Host-side mirror of the reference's examples/09_eikonal/eikonal_dolfinx.py: `solve_problem` runs its LVPP loop (:149-174) and
`EikonalProblem` stands where the script builds `NonlinearProblem(F, u=w, bcs=[], J=J, petsc_options=sp, ...)` (:78-80).  Everything
below `.solve()`, the copy of w to w0, the norm of the increment and the DG outputs run in libpgx.so (include/pgx_ek.h); only scalars
cross to the host, except for the final fields.

The mesh is the package's own parametrised strip (mesh_generation.create_mobius_strip); reading the ParaView VTU that MFEM writes
(the script's --mesh-dir, :15-27) is out of scope, and so is the facet-normal point cloud (:93-133), a debugging output.
u is Q1 and psi is [Q2]^3 on the equispaced lattice (lagrange.numbering_mobius); every term is integrated with the tensor Gauss rule of
`nq1` points per direction - DOLFINx's automatic quadrature degree is not reproduced.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib, lagrange, mesh_generation
from ._mixed import _MixedHandle
from .problem import _SNES

TOL = 1e-5  # :63


def solver_parameters(tol: float = TOL) -> dict:
    """the script's options (:65-77); ksp preonly + pc lu + MUMPS is the dense pivoting LU of include/pgx_dn.h or, with
    linear_solver="banded", the band LU of include/pgx_bd.h"""
    return {"snes_linesearch_type": "l2", "snes_rtol": tol, "snes_atol": tol, "snes_stol": tol, "snes_max_it": 100}


class NotConvergedError(Exception):
    """stands for PETSc's error under snes_error_if_not_converged (:74)"""


class EikonalProblem(_MixedHandle):
    """x = [u | psi0 | psi1 | psi2]: u in Q1, psi in [Q2]^3 (ambient components) on `mesh` (mesh_generation.MobiusMesh), f (:44) and
    phi (:48) constant, `nq1` Gauss points per direction.  `linear_solver`: "dense" (include/pgx_dn.h, at most 32 768 unknowns) or
    "banded" (include/pgx_bd.h in the folded order lagrange.band_order_mobius: any strip whose band of 38 nv + 22 the solver admits)."""

    _prefix = "pgx_ek"

    def __init__(self, mesh: mesh_generation.MobiusMesh, nq1: int = 6, f: float = 1.0, phi: float = 1.0,
                 petsc_options: dict | None = None, device=0, linear_solver: str = "dense"):
        if linear_solver not in ("dense", "banded"):
            raise ValueError(f"linear_solver {linear_solver!r}: 'dense' or 'banded'")
        if not 1 <= int(nq1) <= 11:
            raise NotImplementedError(f"nq1 {nq1}: the example-09 kernels take 1 to 11 points per direction")
        self._lib = lib = _lib.load()
        self.mesh, self.nq1 = mesh, int(nq1)
        self.n1, self.cell_dofs_u = lagrange.numbering_mobius(mesh.nu, mesh.nv, 1)
        self.n2, self.cell_dofs_p = lagrange.numbering_mobius(mesh.nu, mesh.nv, 2)
        self.ndofs = self.n1 + 3 * self.n2
        t, w = np.polynomial.legendre.leggauss(self.nq1)
        t, w = np.ascontiguousarray(0.5 * (t + 1.0)), np.ascontiguousarray(0.5 * w)
        nodes = np.ascontiguousarray(mesh.cell_nodes, dtype=np.float64)
        assert nodes.shape == (mesh.num_cells, (mesh.order + 1) ** 2, 3)
        self._keep = (t, w, nodes)
        pp = _lib.pgx_ek_problem(mesh.num_cells, mesh.order, _lib.dptr(nodes), self.n1, self.n2, _lib.iptr(self.cell_dofs_u),
                                 _lib.iptr(self.cell_dofs_p), self.nq1, _lib.dptr(t), _lib.dptr(w), float(f), float(phi))
        self._h = C.c_void_p()
        self.linear_solver = linear_solver
        if linear_solver == "banded":
            self.band_perm = lagrange.band_order_mobius(mesh.nu, mesh.nv)
            rc = lib.pgx_ek_create_banded(C.byref(pp), _lib.iptr(self.band_perm), int(device), C.byref(self._h))
        else:
            rc = lib.pgx_ek_create(C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_ek_last_error(None)
            what = "pgx_ek_create_banded" if linear_solver == "banded" else "pgx_ek_create"
            raise _lib.PgxError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))
        for k, v in (solver_parameters() if petsc_options is None else petsc_options).items():
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

    def l2_increment_u(self):
        """sqrt(assemble_scalar((u - u0)^2 dx)) (:88-90, :160-161)"""
        return self._scalar("l2_increment_u")

    def eval_cells(self):
        """(nc, (g+1)^2, 7): u, grad_G u (3), psi (3) at the Q_g interpolation nodes of every cell: the DG outputs (:84-86, :134-148)"""
        out = np.empty((self.mesh.num_cells, (self.mesh.order + 1) ** 2, 7))
        self._call("eval_cells", _lib.dptr(out))
        return out

    def lu_stats(self):
        """the LU's statistics of the last factorisation (include/pgx_dn.h), dense or banded"""
        st = _lib.pgx_dn_stats()
        self._check(self._lib.pgx_ek_lu_stats(self._h, C.byref(st)), "pgx_ek_lu_stats")
        return {key: getattr(st, key) for key, _ in st._fields_}

    def band_stats(self):
        """the band LU's statistics (include/pgx_bd.h: n, kl, ku, bytes and the pivoting figures); raises on a dense handle"""
        st = _lib.pgx_bd_stats()
        self._check(self._lib.pgx_ek_band_stats(self._h, C.byref(st)), "pgx_ek_band_stats")
        return {key: getattr(st, key) for key, _ in st._fields_}


def _write(result_dir: Path, mesh, cells_out):
    """u.bp and psi.bp of the script (:87, :143-148) as one VTU: every cell with its own (g+1)^2 points (the outputs are DG), two
    triangles per square of its node lattice"""
    from . import io

    g1 = mesh.order + 1
    ng = g1 * g1
    v0 = (np.repeat(np.arange(g1 - 1), g1 - 1) * g1 + np.tile(np.arange(g1 - 1), g1 - 1)).astype(np.int64)
    tri = np.concatenate([np.stack([v0, v0 + 1, v0 + g1 + 1], axis=1), np.stack([v0, v0 + g1 + 1, v0 + g1], axis=1)])
    tris = (np.arange(mesh.num_cells)[:, None, None] * ng + tri[None, :, :]).reshape(-1, 3).astype(np.int32)
    flat = cells_out.reshape(-1, 7)
    io.write_vtu(Path(result_dir) / "eikonal.vtu", mesh.cell_nodes.reshape(-1, 3), tris,
                 point_data={"u": flat[:, 0], "grad(u)": flat[:, 1:4], "psi": flat[:, 4:7]})


def solve_problem(nu: int = 64, nv: int = 8, order: int = 3, nq1: int = 6, scale: float = 1.0, tol: float = TOL, f: float = 1.0,
                  phi: float = 1.0, max_lvpp: int = 99, snes_opts: dict | None = None, profile: dict | None = None,
                  result_dir: Path | None = None, verbose: bool = False, monitor=None, device: int = 0,
                  linear_solver: str = "dense"):
    """The script's body on the handle.  Returns (fields, log): `fields` holds the final u, psi (3, n2), the DG outputs `cells`
    (eval_cells) and the geometry nodes x; log rows are (i, alpha, Newton iterations, converged reason, |delta u|).  Raises
    NotConvergedError where the script's snes_error_if_not_converged (:74) would.  `snes_opts` replaces the script's options; a
    `profile` dict receives the handle's timing split of the whole run; `monitor(problem, i)` is called after every step (tests).
    `linear_solver`: "dense" or "banded" (EikonalProblem)."""
    mesh = mesh_generation.create_mobius_strip(nu, nv, order, scale)
    sp = solver_parameters(tol) if snes_opts is None else snes_opts
    problem = EikonalProblem(mesh, nq1, f=f, phi=phi, petsc_options=sp, device=device, linear_solver=linear_solver)
    log = []
    try:
        if profile is not None:
            problem.profile(True)
        for i in range(1, max_lvpp + 1):  # :151
            alpha = min(2 ** i, 10)  # :152
            problem.set_alpha(alpha)
            reason, its = problem.solve()  # :154
            if monitor is not None:
                monitor(problem, i)
            if reason <= 0:  # :74
                raise NotConvergedError(f"LVPP step {i}: SNES reason {reason} after {its} iterations")
            diff = problem.l2_increment_u()  # :160-161
            log.append((i, alpha, its, reason, diff))
            if verbose:
                print(f"Iteration {i}: converged={reason > 0} num_newton_iterations={its} ksp_converged={problem.solver.ksp.getConvergedReason()}")
                print(f"|delta u |= {diff}", flush=True)
            problem.advance_prev()  # :163
            if diff < 5 * tol:  # :173
                break
        newton = [r[2] for r in log]
        if verbose:
            print(f"Num LVPP iterations {len(log)}, Total number of newton iterations {sum(newton)}")
            print(f"min(newton_iterations)={min(newton)} and max(newton_iterations)={max(newton)}", flush=True)
        if profile is not None:
            profile.update(problem.profile(False))
            profile["lu"] = problem.lu_stats()
            if linear_solver == "banded":
                profile["band"] = problem.band_stats()
        x = problem.get_state()
        cells_out = problem.eval_cells()
        fields = dict(u=x[:problem.n1].copy(), psi=x[problem.n1:].reshape(3, problem.n2).copy(), cells=cells_out, x=mesh.cell_nodes)
        if result_dir is not None:
            _write(Path(result_dir), mesh, cells_out)
        return fields, np.array(log, dtype=np.float64).reshape(-1, 5)
    finally:
        problem.close()


__all__ = ["EikonalProblem", "solve_problem", "solver_parameters", "NotConvergedError", "TOL"]
