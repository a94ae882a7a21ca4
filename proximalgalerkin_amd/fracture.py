"""Example 03 - phase-field fracture of a notched plate under load stepping, damage irreversibility through a latent variable - on
the HIP backend.  Host-side mirror of the reference's examples/03_fracture/fracture_dolfinx.py: `solve_problem` runs its
load-step loop with the LVPP iterations and the alpha halving on failure (:207-311), and `FractureProblem` stands where the script
builds `dolfinx.fem.petsc.NonlinearProblem(F, z, bcs=bcs, J=J_reg, petsc_options=sp, ...)` (:204-206, :224-232).  Everything
below `.solve()`, the copies between z, z_iter and z_prev and the two norms run in libpgx.so (include/pgx_fr.h); only scalars
cross to the host, except at write steps.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib, fem
from ._mixed import _MixedHandle
from .mesh_generation import create_crack_mesh
from .problem import _SNES

# the reference's solver parameters (:163-171); rtol 1e-8, stol 1e-8, max_it 50 and divtol 1e4 are PETSc's defaults
SP = {"snes_linesearch_type": "l2", "snes_linesearch_maxlambda": 1, "snes_atol": 1.0e-6, "ksp_type": "preonly", "pc_type": "lu",
      "pc_factor_mat_solver_type": "mumps", "mat_mumps_icntl_14": 500}

# the 10 nodes of P3 on the reference triangle (vertices, two per edge, centre): where the script interpolates c_conform
# (:111-115), and their 9 sub-triangles for the VTU output
P3_NODES = np.ascontiguousarray([[0, 0], [1, 0], [0, 1], [2 / 3, 1 / 3], [1 / 3, 2 / 3], [0, 2 / 3], [0, 1 / 3], [1 / 3, 0], [2 / 3, 0],
                                 [1 / 3, 1 / 3]], dtype=np.float64)
_P3_SUBCELLS = np.array([[0, 7, 6], [7, 8, 9], [8, 1, 3], [6, 9, 5], [9, 3, 4], [5, 4, 2], [7, 9, 6], [8, 3, 9], [9, 4, 5]])


class NotConvergedError(Exception):
    pass


def _check_discretisation(degree):
    if int(degree) != 1:
        raise NotImplementedError(f"degree {degree}: the example-03 kernels are written for P1 only (:79)")


def max_cell_diameter(mesh: fem.Mesh) -> float:
    """l = max over the cells of 4 Circumradius (:88-93), on the host, once"""
    x = mesh.geometry[mesh.cells]
    e = [np.linalg.norm(x[:, (k + 1) % 3] - x[:, (k + 2) % 3], axis=1) for k in range(3)]
    a, b = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    area = 0.5 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
    return float(np.max(4.0 * e[0] * e[1] * e[2] / (4.0 * area)))


def boundary_vertices(facets, name_or_tag, names=None) -> np.ndarray:
    """vertices of the boundary edges with one tag (locate_dofs_topological on Z.sub(0), :145-156)"""
    edges, tags = facets
    tag = names[name_or_tag] if names is not None else name_or_tag
    return np.unique(edges[tags == tag]).astype(np.int32)


class FractureProblem(_MixedHandle):
    """x = [u | c | psi], each a P1 field on `mesh`; u = -T on `minus_dofs`, u = +T on `plus_dofs` (set_load)."""

    _prefix = "pgx_fr"

    def __init__(self, mesh: fem.Mesh, minus_dofs, plus_dofs, petsc_options: dict | None = None, G=1.0, Gc=1.0, l=None, eps=1.0e-5,
                 reps=1.0e-3, device=0):
        self._lib = lib = _lib.load()
        self.mesh = mesh
        self.nv = mesh.num_vertices
        self.ndofs = 3 * self.nv
        self.l = max_cell_diameter(mesh) if l is None else float(l)
        pts, wts = fem.quadrature_rule("triangle", 7)  # tri_deg7_gj16: UFL's degree estimate for the terms containing psi
        minus = np.ascontiguousarray(minus_dofs, dtype=np.int32)
        plus = np.ascontiguousarray(plus_dofs, dtype=np.int32)
        self._keep = (mesh.geometry, mesh.cells, pts, wts, minus, plus)
        pm = _lib.pgx_mesh(self.nv, mesh.num_cells, _lib.dptr(mesh.geometry), _lib.iptr(mesh.cells), 0, 0, None, 0)
        pp = _lib.pgx_fr_problem(len(wts), _lib.dptr(pts), _lib.dptr(wts), float(G), float(Gc), self.l, float(eps), float(reps),
                                 len(minus), _lib.iptr(minus), len(plus), _lib.iptr(plus))
        self._h = C.c_void_p()
        rc = lib.pgx_fr_create(C.byref(pm), C.byref(pp), int(device), C.byref(self._h))
        if rc:
            msg = lib.pgx_fr_last_error(None)
            raise _lib.PgxError(f"pgx_fr_create failed (code {rc}): {msg.decode() if msg else ''}")
        self._opts = _lib.pgx_snes_opts()
        lib.pgx_default_opts(C.byref(self._opts))  # rtol 1e-8, stol 1e-8, max_it 50, divtol 1e4: PETSc's defaults
        for k, v in (SP if petsc_options is None else petsc_options).items():
            if k in ("snes_rtol", "snes_atol", "snes_stol", "snes_divtol"):
                setattr(self._opts, k, float(v))
            elif k == "snes_max_it":
                self._opts.snes_max_it = int(v)
            elif k == "snes_linesearch_type":
                if v not in ("l2", "bt", "none", "basic"):
                    raise NotImplementedError(f"snes_linesearch_type {v}")
                self._opts.linesearch = {"l2": 2, "bt": 3}.get(v, 0)
            elif k == "snes_linesearch_maxlambda" and float(v) != 1.0:
                raise NotImplementedError("l2 line search: maxlambda 1 (:165)")
            elif k == "snes_monitor":
                self._opts.monitor = max(self._opts.monitor, 1)
            elif k == "snes_linesearch_monitor":
                self._opts.monitor = 2
        self._opts.ksp_max_it = 6
        self.solver = _SNES(self._opts)

    # -- the load-step loop's device-side updates --------------------------------------------------------------------
    def set_load(self, T):
        """bcminus.value = -T; bcplus.value = T (:213-214)"""
        self.T = float(T)
        self._call("set_load", self.T)

    def set_zprev(self, z):
        self._call("set_zprev", _lib.dptr(np.ascontiguousarray(z, dtype=np.float64)))

    def get_zprev(self):
        z = np.empty(self.ndofs)
        self._call("get_zprev", _lib.dptr(z))
        return z

    def zprev_from_state(self):
        """z_prev.interpolate(z) (:309)"""
        self._call("zprev_from_state")

    def state_from_zprev(self):
        """z.interpolate(z_prev) (:253)"""
        self._call("state_from_zprev")

    def state_from_prev(self):
        """z.interpolate(z_iter) (:255)"""
        self._call("state_from_prev")

    def l2_increment_c(self):
        """||c - c_iter||_L2 (:187, :267)"""
        return self._scalar("l2_increment_c")

    def l2_distance_zprev(self):
        """||z - z_prev||_L2 over the three blocks (:188, :292)"""
        return self._scalar("l2_distance_zprev")

    def conforming_damage(self, ref_pts=P3_NODES):
        """c_conform (:114) at reference points of every cell, (num_cells, npts); default: the P3 nodes (:111-115)"""
        ref_pts = np.ascontiguousarray(ref_pts, dtype=np.float64).reshape(-1, 2)
        out = np.empty((self.mesh.num_cells, len(ref_pts)))
        self._call("conforming_damage", len(ref_pts), _lib.dptr(ref_pts), _lib.dptr(out))
        return out

    def lu_stats(self):
        st = _lib.pgx_nd_stats()
        self._check(self._lib.pgx_fr_lu_stats(self._h, C.byref(st)), "pgx_fr_lu_stats")
        out = {k: getattr(st, k) for k, _ in st._fields_}  # perturbed_pivots: of the last completed factorisation
        out["symmetric"] = bool(self._lib.pgx_fr_lu_is_symmetric(self._h))  # L D L^T in LU clothing: about half of `flops` executed
        return out


def _write(result_dir: Path, mesh, step, x, conform):
    from . import io

    n = mesh.num_vertices
    result_dir.mkdir(parents=True, exist_ok=True)
    io.write_vtu(result_dir / f"solution_{step:06d}.vtu", mesh.geometry, mesh.cells,
                 point_data={"u": x[:n], "c": x[n:2 * n], "psi": x[2 * n:]})
    # ConformingDamage lives in P3 (:111-112): written on the 9 sub-triangles of every cell, nodes not shared between cells
    N = np.stack([1.0 - P3_NODES[:, 0] - P3_NODES[:, 1], P3_NODES[:, 0], P3_NODES[:, 1]], axis=1)
    pts = np.einsum("pa,cad->cpd", N, mesh.geometry[mesh.cells]).reshape(-1, 2)
    sub = (10 * np.arange(mesh.num_cells)[:, None, None] + _P3_SUBCELLS[None]).reshape(-1, 3)
    io.write_vtu(result_dir / f"damage_{step:06d}.vtu", pts, sub, point_data={"ConformingDamage": conform.ravel()})


def solve_problem(res: float = 0.0125, num_load_steps: int = 1001, Tmin: float = 0.0, Tmax: float = 5.0, nfail_max: int = 50,
                  write_frequency: int = 25, degree: int = 1, result_dir: Path | None = None, verbose: bool = False,
                  return_solution: bool = False, profile: dict | None = None, petsc_options: dict | None = None, monitor=None,
                  device: int = 0):
    """The script's body (:77-311) on the handle.  Returns (log, newton_iterations, lvpp_iterations): log rows are
    (step, k, alpha, Newton iterations, converged reason, increment), increment = nan for a failed attempt; the two counts are per
    load step.  return_solution=True appends a dict with the final u, c, psi, z_prev and the mesh.  `res` IS honoured when meshing
    (the reference's script parses --res and then meshes with max_res=0.0125 regardless, :78).  With `result_dir`, u, c, psi
    (solution_*.vtu) and ConformingDamage (damage_*.vtu) are written every `write_frequency` steps in place of the reference's
    XDMF / VTX output.  A `profile` dict receives the handle's timing split of the whole run; `monitor(problem, step, k)` is called
    after every attempt (tests)."""
    _check_discretisation(degree)
    mesh, ft, material_map = create_crack_mesh(max_res=res)
    left_dofs = boundary_vertices(ft, "topleft", material_map)  # u = -T (:145-150, :159)
    right_dofs = boundary_vertices(ft, "topright", material_map)  # u = +T (:151-158)
    problem = FractureProblem(mesh, left_dofs, right_dofs, petsc_options=petsc_options, device=device)
    if verbose:
        print(f"Using l = {problem.l}", flush=True)
    result_dir = None if result_dir is None else Path(result_dir)
    log, newton, lvpp = [], [], []
    try:
        if profile is not None:
            problem.profile(True)
        converged_reason, num_iterations = -1, -1
        for step, T in enumerate(np.linspace(Tmin, Tmax, num_load_steps)[1:]):
            if verbose:
                print(f"Solving for T = {float(T)} ({step / num_load_steps * 100:.1f}%)", flush=True)
            problem.set_load(T)  # :213-214
            alpha = 1.0  # :215
            problem.advance_prev()  # z_iter.interpolate(z) :216
            k, r, nfail = 1, 2, 0
            newton.append(0)
            lvpp.append(0)
            while nfail <= nfail_max:
                try:
                    if verbose:
                        print(f"Attempting k={k} alpha={alpha}", flush=True)
                    problem.set_alpha(alpha)
                    problem.solve()  # :233
                    num_iterations = problem.solver.getIterationNumber()
                    converged_reason = problem.solver.getConvergedReason()
                    newton[-1] += num_iterations
                    if monitor is not None:
                        monitor(problem, step, k)
                    if num_iterations == 0 and converged_reason > 0:  # :236-240
                        raise NotConvergedError("Not converged")
                    if converged_reason < 0:
                        raise NotConvergedError("Not converged")
                except NotConvergedError:
                    nfail += 1
                    log.append((step, k, alpha, num_iterations, converged_reason, np.nan))
                    if verbose:
                        print(f"Failed to converge ({converged_reason}), k={k} alpha={alpha}", flush=True)
                    alpha /= 2  # :251
                    if k == 1:
                        problem.state_from_zprev()  # :253
                    else:
                        problem.state_from_prev()  # :255
                    if nfail >= nfail_max:
                        if verbose:
                            print(f"Giving up. T={T} alpha={alpha} k={k}", flush=True)
                        break
                    continue
                nrm = problem.l2_increment_c()  # :267
                log.append((step, k, alpha, num_iterations, converged_reason, nrm))
                lvpp[-1] += 1
                if verbose:
                    print(f"Solved k={k} num_iterations={num_iterations} alpha={alpha},||c_{k} - c_{k - 1}|| = {nrm}", flush=True)
                if nrm < 1.0e-4:  # :274
                    break
                if num_iterations <= 4:  # :278-281
                    alpha *= r
                elif num_iterations >= 10:
                    alpha /= r
                problem.advance_prev()  # :284
                k += 1
            # a broken plate: one PG iteration without Newton iterations, so the solution does not change (:288-294)
            norm_Z = problem.l2_distance_zprev()
            if k == 1 and np.isclose(norm_Z, 0.0):
                break
            if nfail == nfail_max:  # :296
                break
            if step % write_frequency == 0:  # :300-310
                if result_dir is not None:
                    _write(result_dir, mesh, step, problem.get_state(), problem.conforming_damage())
                problem.zprev_from_state()  # :309: c_conform sees the c of the last WRITTEN step
        if profile is not None:
            profile.update(problem.profile(False))
        out = (np.array(log, dtype=np.float64).reshape(-1, 6), np.array(newton, dtype=np.int32), np.array(lvpp, dtype=np.int32))
        if return_solution:
            x, n = problem.get_state(), problem.nv
            out += (dict(u=x[:n].copy(), c=x[n:2 * n].copy(), psi=x[2 * n:].copy(), z_prev=problem.get_zprev(), mesh=mesh),)
        return out
    finally:
        problem.close()


__all__ = ["FractureProblem", "solve_problem", "create_crack_mesh", "boundary_vertices", "max_cell_diameter", "NotConvergedError",
           "SP", "P3_NODES"]
