"""Problem / solver classes with the call shapes of the reference, backed by libpgx.so.

    NonlinearProblem(F, u, bcs=, J=, petsc_options=, petsc_options_prefix=).solve()
        -> dolfinx.fem.petsc.NonlinearProblem as used at
           /root/reference/examples/01_obstacle_problem/obstacle_pg.py:140-142,190-192
    SNESProblem(F, u, J=None, bcs=None, ...) with .F(snes,x,F) / .J(snes,x,J,P);
    SNESSolver(problem, options).solve() -> (converged_reason, iterations)
        -> /root/reference/src/lvpp/problem.py:14-127

"UFL forms in" becomes a declarative form object (ObstacleResidual) because UFL cannot ship
(SURVEY.md section 8b); everything from `solve()` downward runs in hand-written HIP through the C ABI
of include/pgx.h.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib
from .fem import Constant, DirichletBC, Function, QuadratureFunction

# PETSc SNESConvergedReason values
SNES_CONVERGED_FNORM_ABS = 2
SNES_CONVERGED_FNORM_RELATIVE = 3
SNES_CONVERGED_SNORM_RELATIVE = 4
SNES_DIVERGED_LINEAR_SOLVE = -3
SNES_DIVERGED_FNORM_NAN = -4
SNES_DIVERGED_MAX_IT = -5
SNES_DIVERGED_DTOL = -9


class ConvergenceError(RuntimeError):
    """Raised for snes_error_if_not_converged / ksp_error_if_not_converged (obstacle_pg.py:132,135)."""


@dataclass
class ObstacleResidual:
    """The residual form of obstacle_pg.py:116-124,

        F = alpha*inner(grad(u),grad(v))*dx + psi*v*dx + u*w*dx - exp(psi)*w*dx - phi*w*dx
            - alpha*f*v*dx - psi_k*v*dx,          dx with quadrature_degree (obstacle_pg.py:115)

    for sol=(u,psi), sol_k=(u_k,psi_k) in a mixed [P_k,P_k] space."""
    sol: Function
    sol_k: Function
    alpha: Constant
    f: Constant
    phi: QuadratureFunction
    quadrature_degree: int = 6


@dataclass
class Derivative:
    form: ObstacleResidual
    u: Function


def derivative(F, u, du=None):
    """ufl.derivative(F, sol) (obstacle_pg.py:125): the exact Jacobian [[alpha K, M],[M, -D(psi)]]."""
    return Derivative(F, u)


def _compile(F, u, J):
    """Symbolic forms (proximalgalerkin_amd.ufl) -> the family description the HIP path is built from; J must be the exact
    derivative of F with respect to u (obstacle_pg.py:125) or None (NonlinearProblem's default)."""
    from . import ufl

    if isinstance(F, ufl.Form):
        spec = ufl.compile_form(F, u, J)
        if not isinstance(spec, ObstacleResidual):
            raise NotImplementedError(f"this form is a {type(spec).__name__}: construct it with the family's own NonlinearProblem "
                                      "(proximalgalerkin_amd.thermoforming.NonlinearProblem)")
        return spec, (Derivative(spec, u) if J is not None else None)
    return F, J


_IGNORED_KEYS = {"pc_factor_mat_solver_type", "mat_mumps_icntl_14", "mat_mumps_icntl_24"}


def _parse_options(lib, options: dict | None):
    o = _lib.pgx_snes_opts()
    lib.pgx_default_opts(C.byref(o))
    flags = {"snes_error_if_not_converged": False, "ksp_error_if_not_converged": False}
    for key, v in (options or {}).items():
        if key in ("snes_rtol", "snes_atol", "snes_stol", "snes_divergence_tolerance"):
            setattr(o, "snes_divtol" if key == "snes_divergence_tolerance" else key, float(v))
        elif key == "snes_max_it":
            o.snes_max_it = int(v)
        elif key in ("ksp_rtol",):
            o.ksp_rtol = float(v)
        elif key == "ksp_max_it":
            o.ksp_max_it = int(v)
        elif key == "ksp_gmres_restart":
            o.ksp_restart = int(v)
        elif key in ("mg_nu", "pc_mg_smoothup", "pc_mg_smoothdown"):
            o.mg_nu = int(v)
        elif key == "mg_omega":
            o.mg_omega = float(v)
        elif key == "snes_type":
            if v != "newtonls":
                raise NotImplementedError(f"snes_type {v}")
        elif key == "snes_linesearch_type":
            if v not in ("none", "basic"):
                raise NotImplementedError(f"snes_linesearch_type {v}: only the full Newton step is implemented")
        elif key == "pc_type":
            # "lu" (what the reference passes, obstacle_pg.py:130) does NOT force the sparse direct solver: for P1 the
            # multigrid-preconditioned FGMRES reaches LU-level accuracy (ksp_rtol) an order of magnitude faster
            # (DESIGN.md); "pgx_lu" / "pgx_mg" select explicitly, anything else keeps the automatic choice
            o.pc_type = {"pgx_lu": 2, "pgx_mg": 1}.get(v, 0)
        elif key == "ksp_type":
            pass
        elif key in ("snes_monitor", "ksp_monitor"):
            o.monitor = max(o.monitor, 2 if key == "ksp_monitor" else 1)
        elif key in flags:
            flags[key] = bool(v) if v is not None else True
        elif key in _IGNORED_KEYS:
            warnings.warn(f"PETSc option {key!r} has no meaning for the HIP backend and is ignored", stacklevel=3)
        else:
            warnings.warn(f"unknown option {key!r} ignored", stacklevel=3)
    return o, flags


class _KSP:
    def __init__(self):
        self._reason, self._its = 0, 0

    def getConvergedReason(self):
        return self._reason

    def getIterationNumber(self):
        return self._its


class _SNES:
    """The handful of petsc4py.SNES methods the examples call on `problem.solver`."""

    def __init__(self, opts):
        self._o = opts
        self._reason, self._its = 0, 0
        self.ksp = _KSP()

    def getConvergedReason(self):
        return self._reason

    def getIterationNumber(self):
        return self._its

    def getLinearSolveIterations(self):
        return self.ksp._its

    def setTolerances(self, rtol=None, atol=None, stol=None, max_it=None):
        if rtol is not None:
            self._o.snes_rtol = float(rtol)
        if atol is not None:
            self._o.snes_atol = float(atol)
        if stol is not None:
            self._o.snes_stol = float(stol)
        if max_it is not None:
            self._o.snes_max_it = int(max_it)


class NonlinearProblem:
    def __init__(self, F, u: Function, bcs=None, J=None, petsc_options=None, petsc_options_prefix="", device=0, lu_comm=None):
        """lu_comm: a comm.Communicator -> this handle is one of several REPLICAS (whole mesh on every rank) whose sparse-LU
        preconditioner is distributed over the ranks (include/pgx.h: pgx_create_lu_dist); every call is collective."""
        F, J = _compile(F, u, J)
        if not isinstance(F, ObstacleResidual):
            raise TypeError("F must be a form (proximalgalerkin_amd.ufl) or an ObstacleResidual form description")
        if J is not None and not (isinstance(J, Derivative) and J.form is F):
            raise NotImplementedError("only J = derivative(F, u) (the exact Jacobian) is supported")
        if u is not F.sol:
            raise ValueError("u must be the unknown the form was written for")
        self.F_form, self.u, self.bcs = F, u, list(bcs or [])
        self._lib = lib = _lib.load()
        self._opts, self._flags = _parse_options(lib, petsc_options)
        self.solver = _SNES(self._opts)
        V = u.function_space
        mesh = V.mesh
        if V.ncomp != 2 or F.sol_k.function_space != V:
            raise ValueError("sol and sol_k must live in the same mixed [P_k,P_k] space")
        if F.phi.degree != F.quadrature_degree:
            raise ValueError("phi must be interpolated at the quadrature degree of the measure")
        bc_dofs = np.zeros(0, dtype=np.int32)
        bc_vals = np.zeros(0)
        for bc in self.bcs:
            if not isinstance(bc, DirichletBC) or bc.sub != 0:
                raise NotImplementedError("Dirichlet conditions are supported on sub(0) (u) only")
            bc_dofs = np.concatenate([bc_dofs, bc.dofs])
            bc_vals = np.concatenate([bc_vals, bc.values])
        self._keep = (mesh.geometry, mesh.cells, F.phi.points, F.phi.weights,
                      np.ascontiguousarray(F.phi.values), np.ascontiguousarray(bc_dofs, dtype=np.int32),
                      np.ascontiguousarray(bc_vals, dtype=np.float64))
        cdofs = V.cell_dofs() if V.degree == 2 else None
        self._keep_cd = cdofs
        pm = _lib.pgx_mesh(mesh.num_vertices, mesh.num_cells, _lib.dptr(self._keep[0]), _lib.iptr(self._keep[1]),
                           *(mesh.structured or (0, 0)), _lib.iptr(cdofs), V.block_size if V.degree == 2 else 0)
        pp = _lib.pgx_problem(V.degree, len(self._keep[3]), _lib.dptr(self._keep[2]), _lib.dptr(self._keep[3]),
                              _lib.dptr(self._keep[4]), F.f.value, len(self._keep[5]), _lib.iptr(self._keep[5]),
                              _lib.dptr(self._keep[6]))
        h = C.c_void_p()
        self.partition = part = getattr(mesh, "partition", None)
        if part is None and lu_comm is not None:
            if getattr(mesh, "curved", False):
                raise NotImplementedError("order-2 geometry runs on a single handle (pgx_create_curved); mesh.flattened() gives the affine cells")
            self._lu_comm = lu_comm
            rc = lib.pgx_create_lu_dist(C.byref(pm), C.byref(pp), lu_comm._c, int(device), C.byref(h))
            _lib.check(lib, None, rc, "pgx_create_lu_dist")
        elif part is None and getattr(mesh, "curved", False):
            # order-2 geometry (round 5): degree-2 fields = isoparametric P2, degree-1 fields = hat functions on the quadratic cells
            # (the reference's default run on its own meshes).  Weights and inverse Jacobians of the quadratic cell map at every
            # quadrature point (fem.Mesh.geometry_at); phi was interpolated at the curved cells' quadrature points
            self._keep_geo = mesh.geometry_at(self._keep[2])[1]
            rc = lib.pgx_create_curved(C.byref(pm), C.byref(pp), _lib.dptr(self._keep_geo), int(device), C.byref(h))
            _lib.check(lib, None, rc, "pgx_create_curved")
        elif part is None:
            rc = lib.pgx_create(C.byref(pm), C.byref(pp), int(device), C.byref(h))
            _lib.check(lib, None, rc, "pgx_create")
        else:  # this mesh is one rank's strip: every call below is collective over part.comm (include/pgx.h)
            pt = _lib.pgx_partition(part.rank, part.size, part.global_ny, part.dist_levels)
            rc = lib.pgx_create_sharded(C.byref(pm), C.byref(pp), C.byref(pt), part.comm._c, int(device), C.byref(h))
            _lib.check(lib, None, rc, "pgx_create_sharded")
        self._h = h
        self.ndofs = V.num_dofs
        # a refined general mesh (fem.refine) hands its nested P1 hierarchy to the handle: FGMRES can then precondition with the
        # multilevel cycle (degree 1) or with the two-level patch cycle over it (degree 2; include/pgx.h: pgx_set_hierarchy).  A
        # general mesh without one - read from a file, an unrefined gmsh mesh - gets a hierarchy built from its stiffness matrix where
        # the options ask for the multigrid preconditioner ("pgx_mg") and the mesh is large enough for it to pay
        # (pgx_build_hierarchy_default); structured grids have their own
        hier = getattr(mesh, "hierarchy", None)
        self._umg_levels = 0
        if hier and V.degree in (1, 2) and part is None and lu_comm is None and not mesh.structured:
            self.set_hierarchy(hier)
        elif V.degree in (1, 2) and lib.pgx_build_hierarchy_default(self._h, int(self._opts.pc_type)):
            try:
                self.build_hierarchy()
            except _lib.PgxError as e:
                if getattr(e, "code", 0) != -1:  # not PGX_EINVAL, i.e. anything but a refusal: no half-made handle is left behind
                    self.close()
                    raise
                # refused with nothing changed (e.g. a matrix whose first step keeps too many vertices): the handle runs the
                # single-level smoother it ran before this call existed
        F.sol.x._binding = (self, "state")
        F.sol_k.x._binding = (self, "prev")
        F.sol.x._dev_valid = F.sol_k.x._dev_valid = False

    # -- host <-> device synchronisation of the two bound Functions ---------------------------------
    def _pull(self, slot, out):
        fn = self._lib.pgx_get_state if slot == "state" else self._lib.pgx_get_prev
        _lib.check(self._lib, self._h, fn(self._h, _lib.dptr(out)), "pgx_get_" + slot)

    def _push(self, slot, vec):
        if not vec._dev_valid:
            fn = self._lib.pgx_set_state if slot == "state" else self._lib.pgx_set_prev
            _lib.check(self._lib, self._h, fn(self._h, _lib.dptr(vec._a)), "pgx_set_" + slot)
            vec._dev_valid = True

    def _advance_prev(self):
        _lib.check(self._lib, self._h, self._lib.pgx_advance_prev(self._h), "pgx_advance_prev")

    def zero_state(self):
        """sol = sol_k = 0 on the device, no PCIe traffic (obstacle_pg.py:157-158)."""
        _lib.check(self._lib, self._h, self._lib.pgx_zero_state(self._h), "pgx_zero_state")
        for v in (self.F_form.sol.x, self.F_form.sol_k.x):
            v._dev_valid, v._host_valid = True, False

    def _sync_inputs(self):
        self._push("state", self.F_form.sol.x)
        self._push("prev", self.F_form.sol_k.x)
        if self.partition is not None:
            # the owners' values win over whatever sits in the ghost entries (Vec.ghostUpdate(INSERT, FORWARD),
            # lvpp/problem.py:56).  UNCONDITIONAL, like the reference's: the exchange is collective, and whether a host
            # array was touched is a per-rank fact (`if rank == 0: print(sol.x.array...)`) - a rank-local test would
            # leave the other ranks out of the exchange and hang the run.  One 16-33 KB exchange per call.
            _lib.check(self._lib, self._h, self._lib.pgx_sync_ghosts(self._h), "pgx_sync_ghosts")
        _lib.check(self._lib, self._h, self._lib.pgx_set_alpha(self._h, float(self.F_form.alpha.value)),
                   "pgx_set_alpha")

    # -- the call the examples make once per proximal step (obstacle_pg.py:190) ---------------------
    def solve(self):
        self._sync_inputs()
        reason, its, lin = C.c_int(0), C.c_int(0), C.c_int(0)
        rc = self._lib.pgx_newton_solve(self._h, C.byref(self._opts), C.byref(reason), C.byref(its), C.byref(lin))
        _lib.check(self._lib, self._h, rc, "pgx_newton_solve")
        s = self.solver
        s._reason, s._its = reason.value, its.value
        s.ksp._its = lin.value
        s.ksp._reason = -3 if reason.value == SNES_DIVERGED_LINEAR_SOLVE else 2
        if reason.value > 0:
            self.u.x._host_valid = False  # device holds the new iterate; pulled on next `.x.array`
            self.u.x._dev_valid = True
        if reason.value == SNES_DIVERGED_LINEAR_SOLVE and self._flags["ksp_error_if_not_converged"]:
            raise ConvergenceError("KSP did not converge (DIVERGED_LINEAR_SOLVE)")
        if reason.value <= 0 and self._flags["snes_error_if_not_converged"]:
            raise ConvergenceError(f"SNES did not converge: reason {reason.value} after {its.value} iterations")
        return self.u

    # -- fine-grained probes (tests, parity checks) -----------------------------------------------
    def residual(self, x=None):
        """F(x) with the callback contract of lvpp/problem.py:54-67; x=None uses the current `sol`."""
        self._sync_inputs()
        out = np.empty(self.ndofs)
        nrm = C.c_double(0)
        xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        rc = self._lib.pgx_residual(self._h, _lib.dptr(xx), _lib.dptr(out), C.byref(nrm))
        _lib.check(self._lib, self._h, rc, "pgx_residual")
        return out, nrm.value

    def assemble_jacobian(self, x=None):
        self._sync_inputs()
        xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        _lib.check(self._lib, self._h, self._lib.pgx_jacobian_fill(self._h, _lib.dptr(xx)), "pgx_jacobian_fill")

    def export_blocks(self, with_D=True):
        """(rowptr, col, K, M, D) of the scalar pattern shared by the four Jacobian blocks."""
        nrows, nnz = C.c_int64(0), C.c_int64(0)
        lib = self._lib
        _lib.check(lib, self._h, lib.pgx_csr_export(self._h, C.byref(nrows), C.byref(nnz), None, None, None, None,
                                                    None), "pgx_csr_export")
        rowptr = np.empty(nrows.value + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        K, M = np.empty(nnz.value), np.empty(nnz.value)
        D = np.empty(nnz.value) if with_D else None
        _lib.check(lib, self._h, lib.pgx_csr_export(self._h, None, None, _lib.iptr(rowptr), _lib.iptr(col),
                                                    _lib.dptr(K), _lib.dptr(M), _lib.dptr(D)), "pgx_csr_export")
        return rowptr, col, K, M, D

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        _lib.check(self._lib, self._h, self._lib.pgx_spmv(self._h, _lib.dptr(x), _lib.dptr(y)), "pgx_spmv")
        return y

    def spmv_bench(self, reps=20):
        ms, by = C.c_double(0), C.c_double(0)
        _lib.check(self._lib, self._h, self._lib.pgx_spmv_bench(self._h, int(reps), C.byref(ms), C.byref(by)),
                   "pgx_spmv_bench")
        return ms.value, by.value

    def spmv_bench_cold(self, reps=20):
        """Like spmv_bench, every apply after a 512 MB sweep (operands from HBM, not the Infinity Cache): pgx_spmv_bench_cold."""
        ms, by = C.c_double(0), C.c_double(0)
        _lib.check(self._lib, self._h, self._lib.pgx_spmv_bench_cold(self._h, int(reps), C.byref(ms), C.byref(by)),
                   "pgx_spmv_bench_cold")
        return ms.value, by.value

    def spmv_select(self, kind=-1):
        """Select / query the operator-apply kernel of the Krylov solver (include/pgx.h: pgx_spmv_select): 1 matrix-free stencil
        (default on structured P1 meshes), 0 block-CSR stream, 2 generic stencil kernel; returns the kind that will run."""
        act = C.c_int(0)
        _lib.check(self._lib, self._h, self._lib.pgx_spmv_select(self._h, int(kind), C.byref(act)), "pgx_spmv_select")
        return act.value

    def p2_stencil_info(self):
        """(state, i0, ni, j0, nj) of the structured P2 operator apply (include/pgx.h: pgx_p2_stencil_info)."""
        out = (C.c_int32 * 5)()
        _lib.check(self._lib, self._h, self._lib.pgx_p2_stencil_info(self._h, out), "pgx_p2_stencil_info")
        return tuple(int(v) for v in out)

    def comm_counts(self, reset=False):
        """Collectives this rank issued since the last reset (include/pgx.h: pgx_comm_counts)."""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib, self._h, self._lib.pgx_comm_counts(self._h, out, int(reset)), "pgx_comm_counts")
        return dict(zip(("halo_exchanges", "allreduces", "vcycles", "krylov_iterations"), (int(v) for v in out)))

    def smoother_bench(self, reps=20):
        """(avg ms, algorithmic bytes) of the finest level's fused smoother launch (include/pgx.h: pgx_smoother_bench)."""
        ms, by = C.c_double(0), C.c_double(0)
        _lib.check(self._lib, self._h, self._lib.pgx_smoother_bench(self._h, int(reps), C.byref(ms), C.byref(by)),
                   "pgx_smoother_bench")
        return ms.value, by.value

    def vcycle_bench(self, level, reps=50):
        """(avg ms, vertices of that level): the part of one V-cycle from multigrid level `level` down and back up, launches back
        to back (include/pgx.h: pgx_vcycle_bench; level -1 = the fused tail launch)."""
        ms, nl = C.c_double(0), C.c_int(0)
        _lib.check(self._lib, self._h, self._lib.pgx_vcycle_bench(self._h, int(level), int(reps), C.byref(ms), C.byref(nl)),
                   "pgx_vcycle_bench")
        return ms.value, nl.value

    def _check_code(self, rc, what):
        """_lib.check whose PgxError carries the PGX_E* code as `.code` (the tests of the refusals read it)."""
        try:
            _lib.check(self._lib, self._h, rc, what)
        except _lib.PgxError as e:
            e.code = rc
            raise

    def mg_levels(self):
        """Number of levels pgx_mg_level_export serves (the call refuses the first level that does not exist)."""
        nx, ny, f, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        l = 0
        while self._lib.pgx_mg_level_export(self._h, l, C.byref(nx), C.byref(ny), None, None, None, C.byref(f), C.byref(d)) == 0:
            l += 1
        if l == 0:
            self.mg_level_export(0)  # raises with the library's message
        return l

    def mg_level_export(self, level):
        """What multigrid level `level` stores after the last assemble_jacobian (include/pgx.h: pgx_mg_level_export; a test hook):
        dict(nx, ny, Dh [4, n] fp64 half-stored D stencil, Dq [n, 4] float32 decoded copy of the single-precision cycle or None,
        mask [n] bool, f32, dbf16)."""
        lib = self._lib
        nx, ny, f, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check_code(lib.pgx_mg_level_export(self._h, int(level), C.byref(nx), C.byref(ny), None, None, None, C.byref(f), C.byref(d)),
                         "pgx_mg_level_export")
        n = (nx.value + 1) * (ny.value + 1)
        Dh = np.empty((4, n))
        Dq = np.zeros((n, 4), dtype=np.float32) if f.value else None
        mask = np.empty(n, dtype=np.uint8)
        self._check_code(lib.pgx_mg_level_export(self._h, int(level), C.byref(nx), C.byref(ny), _lib.dptr(Dh),
                                                 None if Dq is None else Dq.ctypes.data_as(C.POINTER(C.c_float)),
                                                 mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(f), C.byref(d)), "pgx_mg_level_export")
        return dict(nx=nx.value, ny=ny.value, Dh=Dh, Dq=Dq, mask=mask.astype(bool), f32=f.value, dbf16=d.value)

    def vcycle_apply(self, level, b, nu=6, omega=0.75, in_form=0, out_form=0, scale=1.0):
        """One V(nu, nu) cycle entered on multigrid level `level` from a zero guess, b and the result [u | psi] of that level
        (include/pgx.h: pgx_vcycle_apply; a test hook)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        z = np.empty_like(b)
        nx, ny = C.c_int32(0), C.c_int32(0)
        self._check_code(self._lib.pgx_mg_level_export(self._h, int(level), C.byref(nx), C.byref(ny), None, None, None, None, None),
                         "pgx_vcycle_apply")
        if b.shape != (2 * (nx.value + 1) * (ny.value + 1),):
            raise ValueError(f"b must hold [u | psi] of level {level}: {2 * (nx.value + 1) * (ny.value + 1)} entries")
        self._check_code(self._lib.pgx_vcycle_apply(self._h, int(level), int(nu), float(omega), int(in_form), int(out_form), float(scale),
                                                    _lib.dptr(b), _lib.dptr(z)), "pgx_vcycle_apply")
        return z

    def set_hierarchy(self, parents, n_coarse=None):
        """Attach the hierarchy of a refined general mesh (include/pgx.h: pgx_set_hierarchy): `parents` as Mesh.hierarchy holds them,
        fine -> coarse; n_coarse[t] defaults to the number of (v, v) rows of parents[t]."""
        par = [np.ascontiguousarray(p, dtype=np.int32) for p in parents]
        if n_coarse is None:
            n_coarse = [int(np.count_nonzero(p[:, 0] == p[:, 1])) for p in par]
        nc = np.ascontiguousarray(n_coarse, dtype=np.int32)
        ptrs = (_lib.c_int32_p * max(len(par), 1))(*[_lib.iptr(p) for p in par])
        self._check_code(self._lib.pgx_set_hierarchy(self._h, len(par), _lib.iptr(nc), ptrs), "pgx_set_hierarchy")
        self._umg_levels = len(par) + 1

    def build_hierarchy(self, theta=None, trunc=None, min_coarse=None, max_keep=None):
        """Build the multigrid hierarchy of a general mesh that has none from the stiffness matrix (include/pgx.h: pgx_build_hierarchy;
        None: the library's defaults).  Before the first Jacobian fill, once, instead of set_hierarchy.  Returns the number of levels;
        build_seconds holds (host pass, device work and copies)."""
        nl, sec = C.c_int32(0), np.zeros(2)
        self._check_code(self._lib.pgx_build_hierarchy(self._h, -1.0 if theta is None else float(theta), -1.0 if trunc is None else float(trunc),
                                                       0 if min_coarse is None else int(min_coarse),
                                                       0.0 if max_keep is None else float(max_keep), C.byref(nl), _lib.dptr(sec)),
                         "pgx_build_hierarchy")
        self._umg_levels, self.build_seconds = int(nl.value), (float(sec[0]), float(sec[1]))
        return self._umg_levels

    def build_info(self):
        """How the built hierarchy came about (include/pgx.h: pgx_amg_build_info): dict(mode="device" | "host", split_launches=[per
        transfer the launches its C/F split took; 0 for the host pass]).  Raises without a built hierarchy."""
        mode, nt = C.c_int32(0), C.c_int32(0)
        self._check_code(self._lib.pgx_amg_build_info(self._h, C.byref(mode), C.byref(nt), None), "pgx_amg_build_info")
        launches = np.zeros(max(nt.value, 1), dtype=np.int32)
        self._check_code(self._lib.pgx_amg_build_info(self._h, None, None, _lib.iptr(launches)), "pgx_amg_build_info")
        return dict(mode="device" if mode.value == 1 else "host", split_launches=[int(v) for v in launches[: nt.value]])

    def umg_transfer_export(self, t):
        """Transfer t of a built hierarchy, level t + 1 -> level t, as a scipy CSR matrix (include/pgx.h: pgx_umg_transfer_export; a
        test hook)."""
        import scipy.sparse as sp

        nf, nc, nnz = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        lib = self._lib
        self._check_code(lib.pgx_umg_transfer_export(self._h, int(t), C.byref(nf), C.byref(nc), C.byref(nnz), None, None, None),
                         "pgx_umg_transfer_export")
        rowptr, col, val = np.empty(nf.value + 1, dtype=np.int32), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        self._check_code(lib.pgx_umg_transfer_export(self._h, int(t), None, None, None, _lib.iptr(rowptr), _lib.iptr(col), _lib.dptr(val)),
                         "pgx_umg_transfer_export")
        return sp.csr_matrix((val, col, rowptr), shape=(nf.value, nc.value))

    def umg_level_export(self, level):
        """What level `level` of the general-mesh hierarchy stores after the last assemble_jacobian (include/pgx.h:
        pgx_umg_level_export; a test hook): dict(n, rowptr, col, K, M, D, mask)."""
        n, nnz = C.c_int32(0), C.c_int32(0)
        lib = self._lib
        self._check_code(lib.pgx_umg_level_export(self._h, int(level), C.byref(n), C.byref(nnz), None, None, None, None, None, None),
                         "pgx_umg_level_export")
        rowptr, col = np.empty(n.value + 1, dtype=np.int32), np.empty(nnz.value, dtype=np.int32)
        K, M, D = np.empty(nnz.value), np.empty(nnz.value), np.empty(nnz.value)
        mask = np.empty(n.value, dtype=np.uint8)
        self._check_code(lib.pgx_umg_level_export(self._h, int(level), None, None, _lib.iptr(rowptr), _lib.iptr(col), _lib.dptr(K),
                                                  _lib.dptr(M), _lib.dptr(D), mask.ctypes.data_as(C.POINTER(C.c_uint8))),
                         "pgx_umg_level_export")
        return dict(n=n.value, rowptr=rowptr, col=col, K=K, M=M, D=D, mask=mask.astype(bool))

    def umg_levels(self):
        """Number of levels pgx_umg_level_export serves: the transfers handed to set_hierarchy, plus one, or what build_hierarchy
        built.  Raises as that hook does
        where it would not serve level 0 (no hierarchy, no filled Jacobian)."""
        n = C.c_int32(0)
        self._check_code(self._lib.pgx_umg_level_export(self._h, 0, C.byref(n), None, None, None, None, None, None, None),
                         "pgx_umg_level_export")
        return self._umg_levels

    def umg_cycle_apply(self, level, b, nu=6, omega=0.75):
        """One V(nu, nu) cycle of the general-mesh hierarchy entered on `level` from a zero guess, b and the result [u | psi] of that
        level (include/pgx.h: pgx_umg_cycle_apply; a test hook)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        z = np.empty_like(b)
        n = C.c_int32(0)
        self._check_code(self._lib.pgx_umg_level_export(self._h, int(level), C.byref(n), None, None, None, None, None, None, None),
                         "pgx_umg_cycle_apply")
        if b.shape != (2 * n.value,):
            raise ValueError(f"b must hold [u | psi] of level {level}: {2 * n.value} entries")
        self._check_code(self._lib.pgx_umg_cycle_apply(self._h, int(level), int(nu), float(omega), _lib.dptr(b), _lib.dptr(z)),
                         "pgx_umg_cycle_apply")
        return z

    P2_PATCH_FORMS = ("double", "float", "float-sym", "bf16-sym")
    P2_RESID_KERNELS = ("csr", "csr-balanced", "structured")

    def p2_cycle_info(self):
        """What the P2 two-level cycle of this handle runs (include/pgx.h: pgx_p2_cycle_info; a test hook): dict(patch_nn, form,
        patch_nu, patch_omega, resid_f32, resid_kernel, fallbacks, km_dict, hierarchy)."""
        out = np.zeros(8, dtype=np.int32)
        om = C.c_double(0)
        self._check_code(self._lib.pgx_p2_cycle_info(self._h, _lib.iptr(out), C.byref(om)), "pgx_p2_cycle_info")
        return dict(patch_nn=int(out[0]), form=self.P2_PATCH_FORMS[out[1]], patch_nu=int(out[2]), patch_omega=om.value,
                    resid_f32=bool(out[3]), resid_kernel=self.P2_RESID_KERNELS[out[4]], fallbacks=int(out[5]), km_dict=bool(out[6]),
                    hierarchy=bool(out[7]))

    def p2_patch_export(self):
        """(pdof [nv, NN] int32, Ainv [nv, 2 NN, 2 NN]) of the vertex-star patches at the last assemble_jacobian, the inverses decoded
        as the sweep kernel decodes them (include/pgx.h: pgx_p2_patch_export; a test hook)."""
        NN = self.p2_cycle_info()["patch_nn"]
        nv = self._keep[0].shape[0]  # mesh vertices
        pdof = np.empty((nv, NN), dtype=np.int32)
        Ainv = np.empty((nv, 2 * NN, 2 * NN))
        self._check_code(self._lib.pgx_p2_patch_export(self._h, _lib.iptr(pdof), _lib.dptr(Ainv)), "pgx_p2_patch_export")
        return pdof, Ainv

    def p2_wide_export(self):
        """(verts [nw] int32, wdof [nw, 16] int32, Ainv [nw, 32, 32]) of the wide stars - vertices of degree 8 ... 15 - at the last
        assemble_jacobian (include/pgx.h: pgx_p2_wide_export; a test hook).  nw = 0 on a mesh without such vertices."""
        nw = C.c_int32(0)
        self._check_code(self._lib.pgx_p2_wide_export(self._h, C.byref(nw), None, None, None), "pgx_p2_wide_export")
        verts = np.empty(nw.value, dtype=np.int32)
        wdof = np.empty((nw.value, 16), dtype=np.int32)
        Ainv = np.empty((nw.value, 32, 32))
        if nw.value:
            self._check_code(self._lib.pgx_p2_wide_export(self._h, None, _lib.iptr(verts), _lib.iptr(wdof), _lib.dptr(Ainv)),
                             "pgx_p2_wide_export")
        return verts, wdof, Ainv

    def p2_cycle_apply(self, stage, b, x0=None, nu=6, omega=0.75):
        """One stage of the P2 two-level cycle on host vectors (include/pgx.h: pgx_p2_cycle_apply; a test hook): 1 one sweep from x0
        (None: the first sweep of a cycle), 2 the residual b - J x0, 3 restriction (result [u | psi] of the P1 space), 4 x0 + T b
        (b of the P1 space), 0 the whole preconditioner."""
        nv = self._keep[0].shape[0]  # mesh vertices
        n_in = 2 * nv if stage == 4 else self.ndofs
        n_out = 2 * nv if stage == 3 else self.ndofs
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (n_in,):
            raise ValueError(f"stage {stage} takes b of {n_in} entries")
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (self.ndofs,):
                raise ValueError(f"x0 must hold [u | psi] of the P2 space: {self.ndofs} entries")
        z = np.empty(n_out)
        self._check_code(self._lib.pgx_p2_cycle_apply(self._h, int(stage), int(nu), float(omega), _lib.dptr(b), _lib.dptr(x0), _lib.dptr(z)),
                         "pgx_p2_cycle_apply")
        return z

    def observables(self):
        """[energy, |complementarity|, feasibility, dual feasibility, H1 increment, latent L2 increment]
        of obstacle_pg.py:145-152,196-201 in one device pass."""
        self._sync_inputs()
        out = np.empty(6)
        _lib.check(self._lib, self._h, self._lib.pgx_observables(self._h, _lib.dptr(out)), "pgx_observables")
        return out

    def reduce_selfcheck(self, nv, length, basis_f32=False, reps=1, seed=0):
        """Number of 8-byte words in which the two routes of the Krylov driver's reductions differ (include/pgx.h:
        pgx_reduce_selfcheck); 0 is the only right answer."""
        bad = C.c_int64(-1)
        _lib.check(self._lib, self._h, self._lib.pgx_reduce_selfcheck(self._h, int(nv), int(length), int(bool(basis_f32)), int(reps),
                                                                      int(seed), C.byref(bad)), "pgx_reduce_selfcheck")
        return bad.value

    def resid_reuse_counts(self, reset=False):
        """(full, reduced): entry evaluations of the Newton solves of this handle so far (include/pgx.h: pgx_resid_reuse_counts)."""
        out = (C.c_int64 * 2)()
        _lib.check(self._lib, self._h, self._lib.pgx_resid_reuse_counts(self._h, out, int(reset)), "pgx_resid_reuse_counts")
        return int(out[0]), int(out[1])

    def resid_reuse_selfcheck(self):
        """The next solve's entry evaluation, reduced against full, at the current sol, sol_k and alpha: six counts, the first five of
        which must be 0 (include/pgx.h: pgx_resid_reuse_selfcheck)."""
        self._sync_inputs()
        out = (C.c_int64 * 6)()
        _lib.check(self._lib, self._h, self._lib.pgx_resid_reuse_selfcheck(self._h, out), "pgx_resid_reuse_selfcheck")
        return [int(v) for v in out]

    def owned_edge_range(self):
        """(offset, count): owned EDGE dofs within each field block of a P2 local vector (include/pgx.h: pgx_owned_edge_range)."""
        off, cnt = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib, self._h, self._lib.pgx_owned_edge_range(self._h, C.byref(off), C.byref(cnt)),
                   "pgx_owned_edge_range")
        return off.value, cnt.value

    def owned_range(self):
        """(offset, count): owned VERTEX dofs of each field block of a local vector (all vertices for an unsharded mesh).  Degree 2:
        the field block is [vertex dofs | edge dofs] and this is the vertex part only - combine it with owned_edge_range()."""
        off, cnt = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib, self._h, self._lib.pgx_owned_range(self._h, C.byref(off), C.byref(cnt)),
                   "pgx_owned_range")
        return off.value, cnt.value

    def profile(self, enable=None, reset=False):
        if enable is not None:
            self._lib.pgx_profile_enable(self._h, int(enable))
        ms = np.empty(8)
        self._lib.pgx_profile_get(self._h, _lib.dptr(ms), int(reset))
        keys = ["residual", "jacobian_fill", "mg_setup", "spmv", "vcycle", "orthogonalisation", "observables",
                "newton_total"]
        return dict(zip(keys, ms.tolist()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pgx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# lvpp twins (src/lvpp/problem.py)
# ------------------------------------------------------------------------------------------------
class SNESProblem:
    """lvpp.SNESProblem(F, u, J=None, bcs=None, form_compiler_options=None, jit_options=None)
    (src/lvpp/problem.py:14-52).  `.F` / `.J` keep the SNES callback signatures (problem.py:54,69);
    `x`, `F` are numpy arrays (or objects with `.array`)."""

    def __init__(self, F, u, J=None, bcs=None, form_compiler_options=None, jit_options=None, device=0):
        self.L = F
        self.a = J if J is not None else derivative(F, u)  # problem.py:37-49
        self.bcs = bcs
        self.u = u
        self._backend = NonlinearProblem(F, u, bcs=bcs, J=self.a, device=device)

    @staticmethod
    def _arr(v):
        return v.array if hasattr(v, "array") else v

    def F(self, snes, x, F):
        """Assemble the residual at x into F (problem.py:54-67)."""
        out, _ = self._backend.residual(self._arr(x))
        self._arr(F)[:] = out

    def J(self, snes, x, J, P):
        """Assemble the Jacobian at x into the backend's fixed pattern (problem.py:69-77)."""
        self._backend.assemble_jacobian(self._arr(x))


class SNESSolver:
    """lvpp.SNESSolver(problem, options).solve() -> (converged_reason, iterations)
    (src/lvpp/problem.py:80-127)."""

    def __init__(self, problem: SNESProblem, options: dict):
        self.problem = problem
        self.options = options
        b = problem._backend
        b._opts, b._flags = _parse_options(b._lib, options)
        b.solver = _SNES(b._opts)
        self._snes = b.solver

    def solve(self):
        b = self.problem._backend
        b.solve()  # copies back only if reason>0 (problem.py:121-123), inside pgx_newton_solve
        return self._snes.getConvergedReason(), self._snes.getIterationNumber()
