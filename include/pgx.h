/*
 * pgx.h - C ABI of libpgx.so: MI355X-native LVPP / proximal-Galerkin Newton inner loop.
 *
 * Drop-in boundary for ONE hot path of METHODS-Group/ProximalGalerkin: everything below
 * `problem.solve()` in examples/01_obstacle_problem/obstacle_pg.py:190, i.e. what the reference
 * delegates to DOLFINx assembly + PETSc SNES/KSP + MUMPS.  Plain pointers and sizes only; no torch
 * or C++ types cross this boundary.  All reals are IEEE fp64, all indices int32.
 *
 * DOF layout of every state / residual vector of length 2*n_vertices:
 *      x = [u_0 .. u_{n-1}, psi_0 .. psi_{n-1}]        (n = n_vertices for P1, pgx_mesh.n_dofs for P2)
 *
 * Conventions:
 *   - every function returns 0 on success, a negative PGX_E* code otherwise; pgx_last_error() gives text.
 *   - the caller owns all host buffers passed in; they are never retained past the call.
 *   - the handle owns all device memory; a handle is bound to one HIP device and is not thread-safe.
 *   - calls are synchronous: the handle's stream is idle when a call returns.
 *   - convergence is reported with PETSc's signed SNESConvergedReason values (>0 converged).
 *
 * Reference interface each entry point replaces (paths relative to the reference checkout):
 *   pgx_create            dolfinx.fem.petsc.NonlinearProblem(F,u,bcs,J,petsc_options) construction
 *                         (examples/01_obstacle_problem/obstacle_pg.py:140-142): form compilation,
 *                         sparsity pattern, SNES creation; lvpp twin SNESProblem.__init__ +
 *                         SNESSolver.create_data_structures (src/lvpp/problem.py:14-52,106-112)
 *   pgx_set_state/get_state   sol.x.array[:] access (obstacle_pg.py:157,226)
 *   pgx_set_prev / pgx_advance_prev   sol_k.x.array[:] = sol.x.array[:] (obstacle_pg.py:158,226)
 *   pgx_zero_state        sol.x.array[:] = 0.0; sol_k.x.array[:] = sol.x.array[:] (obstacle_pg.py:157-158)
 *   pgx_set_alpha         alpha.value = ... (obstacle_pg.py:175-186)
 *   pgx_residual          SNESProblem.F(snes, x, F) (src/lvpp/problem.py:54-67)
 *   pgx_jacobian_fill     SNESProblem.J(snes, x, J, P) (src/lvpp/problem.py:69-77)
 *   pgx_csr_export        the PETSc Mat `A` of SNESSolver (src/lvpp/problem.py:110), for inspection
 *   pgx_spmv              MatMult on that Mat (inside KSP; the reference uses LU instead:
 *                         obstacle_pg.py:129-131)
 *   pgx_newton_solve      problem.solve() / SNESSolver.solve() (obstacle_pg.py:190;
 *                         src/lvpp/problem.py:114-124) incl. "copy back only if converged"
 *   pgx_observables       the six assemble_scalar + allreduce calls (obstacle_pg.py:145-152,196-201)
 *   pgx_destroy           SNESSolver.__del__ (src/lvpp/problem.py:126-127)
 */
#ifndef PGX_H
#define PGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_OK 0
#define PGX_EINVAL (-1)   /* bad argument / inconsistent sizes */
#define PGX_EHIP (-2)     /* HIP runtime error (text in pgx_last_error) */
#define PGX_ENODEV (-3)   /* no usable GPU */
#define PGX_ENOMEM (-4)
#define PGX_ESTATE (-5)   /* call order violated (e.g. spmv before jacobian_fill) */
#define PGX_ECOMM (-6)    /* communicator failure / a peer rank did not arrive (text in pgx_last_error) */

/* PETSc SNESConvergedReason values mirrored by pgx_newton_solve */
#define PGX_SNES_CONVERGED_FNORM_ABS 2
#define PGX_SNES_CONVERGED_FNORM_RELATIVE 3
#define PGX_SNES_CONVERGED_SNORM_RELATIVE 4
#define PGX_SNES_DIVERGED_LINEAR_SOLVE (-3)
#define PGX_SNES_DIVERGED_FNORM_NAN (-4)
#define PGX_SNES_DIVERGED_MAX_IT (-5)
#define PGX_SNES_DIVERGED_DTOL (-9)

typedef struct pgx_handle pgx_handle;

typedef struct {
  int32_t n_vertices;
  int32_t n_cells;
  const double* coords;   /* [n_vertices][2] */
  const int32_t* cells;   /* [n_cells][3], vertex ids */
  /* >0 only for the right-diagonal structured triangulation with vertex v = j*(nx+1)+i and cells
   * (2q, 2q+1) = [v0,v1,v3],[v0,v2,v3] of square q = j*nx+i (dolfinx create_rectangle default).
   * Enables the geometric multigrid preconditioner; 0 = general mesh.  A general mesh runs the multilevel cycle over a hierarchy
   * that pgx_set_hierarchy attaches (a refined mesh brings its own) or that pgx_build_hierarchy builds from the stiffness matrix
   * (any mesh, e.g. one read from a file); without either call it has the sparse LU and the single-level smoother. */
  int32_t structured_nx;
  int32_t structured_ny;
  /* degree 2 only (NULL / 0 for degree 1): dofs per field are [vertices | one per edge]; row c lists the 3
   * vertex ids of cell c (== cells[c]) then its 3 edge dofs (>= n_vertices), local edge i OPPOSITE local
   * vertex i (the Basix reference-triangle convention the reference's dofmap uses). */
  const int32_t* cell_dofs; /* [n_cells][6] */
  int32_t n_dofs;           /* n_vertices + n_edges */
} pgx_mesh;

typedef struct {
  int32_t degree;          /* Lagrange degree of both fields: 1 or 2 (obstacle_pg.py -p) */
  int32_t nq;              /* quadrature points per cell (<= 16) */
  const double* qpts;      /* [nq][2] on the reference triangle */
  const double* qwts;      /* [nq], summing to 1/2 */
  const double* phi_q;     /* [n_cells][nq] obstacle at physical quadrature points (obstacle_pg.py:107-111) */
  double f;                /* constant forcing (obstacle_pg.py:74) */
  int32_t n_bc;            /* Dirichlet dofs of the u block (obstacle_pg.py:76-83) */
  const int32_t* bc_dofs;  /* [n_bc] vertex ids */
  const double* bc_vals;   /* [n_bc] or NULL for homogeneous */
} pgx_problem;

/* Subset of the PETSc option dictionary the reference passes (obstacle_pg.py:128-139). */
typedef struct {
  double snes_rtol;   /* default 1e-8; ex 01 sets 1e-6 */
  double snes_atol;   /* 1e-50 */
  double snes_stol;   /* 1e-8 */
  double snes_divtol; /* 1e4 */
  int32_t snes_max_it;/* 50; ex 01 sets 100 */
  /* Newton linear solve (replaces ksp preonly + pc lu/mumps): FGMRES + multigrid V-cycle */
  double ksp_rtol;    /* relative TRUE residual target; 0 (default) = auto: 1e-10 for P1, 1e-11 for P2, chosen from the
                         measured effect on the final primal field */
  int32_t ksp_max_it; /* default 200; a sharded P2 handle (no sparse-LU fallback) raises the DEFAULT to 400, an explicit value is kept */
  int32_t ksp_restart;/* default 30 (basis storage allows up to 50) */
  int32_t mg_nu;      /* pre/post smoothing sweeps, default 6 (even values run as fused double sweeps) */
  double mg_omega;    /* collective-Jacobi damping, default 0.75 */
  int32_t monitor;    /* 1 = print per-Newton-step residuals (snes_monitor/ksp_monitor) */
  int32_t pc_type;    /* preconditioner of the FGMRES Newton solve: 0 = auto (1 for P1 on a structured mesh, 2 for P2 and for general
                         meshes), 1 = multigrid V-cycle (single-level smoother on general meshes),
                         2 = sparse LU (nested-dissection multifrontal, include/pgx_nd.h) - what the reference's
                         "pc_type": "lu" (obstacle_pg.py:130) asks for; FGMRES then acts as iterative refinement */
  int32_t linesearch; /* snes_linesearch_type: 0 = none / basic (full step: examples 01, 02, 06), 1 = bt of order 2
                         (quadratic backtracking, examples/05_obstacle_type_qvi/thermoforming_dolfinx.py:104,111); honoured by
                         the handles of pgx_qvi.h, pgx_gc.h and pgx_sg.h (pgx_newton_solve of example 01 takes the full step);
                         3 = bt of order 3 (cubic backtracking, PETSc's default order: example 04, pgx_mp.h) on the same handles */
} pgx_snes_opts;

void pgx_default_opts(pgx_snes_opts* o);

int pgx_create(const pgx_mesh* mesh, const pgx_problem* prob, int device, pgx_handle** out);
/* The same for a mesh with ORDER-2 GEOMETRY (6-node triangles: the reference's own meshes are gmsh meshes of element order 2,
 * examples/01_obstacle_problem/generate_mesh_gmsh.py:30-33, and DOLFINx then integrates on the curved cells).  geoq
 * [n_cells][nq][5] holds, for every quadrature point of prob->qpts on every cell, |det J| and the four entries of J^-1 (row-major:
 * d xi_k / d x_d) of the quadratic cell map x(xi) = sum_a X_a N2_a(xi) - what a binding reads off the coordinate element
 * (fem.Mesh.geometry_at here); prob->phi_q is phi at the PHYSICAL quadrature points of that map.  Unstructured, unpartitioned
 * meshes; degree 2 = isoparametric P2 (csrc/pgx_p2.hip), degree 1 = hat functions on the quadratic cells, the reference's default
 * run on its own meshes (the k_*_c kernels of csrc/pgx_kernels.hip): residual, Jacobian blocks, b_phi and the observables evaluate
 * weights and physical gradients per quadrature point, nothing is constant per cell.  A structured or partitioned mesh is
 * PGX_EINVAL (those have affine cells by construction). */
int pgx_create_curved(const pgx_mesh* mesh, const pgx_problem* prob, const double* geoq, int device, pgx_handle** out);
void pgx_destroy(pgx_handle* h);
const char* pgx_last_error(const pgx_handle* h); /* h may be NULL: error of the last failed pgx_create */

int pgx_num_dofs(const pgx_handle* h, int64_t* ndofs);          /* 2 * dofs per field */
int pgx_set_state(pgx_handle* h, const double* x);               /* host -> device `sol` */
int pgx_get_state(pgx_handle* h, double* x);
int pgx_set_prev(pgx_handle* h, const double* xk);               /* host -> device `sol_k` */
int pgx_get_prev(pgx_handle* h, double* xk);
int pgx_advance_prev(pgx_handle* h);                             /* sol_k <- sol on device */
int pgx_zero_state(pgx_handle* h);                               /* sol = sol_k = 0 on device (obstacle_pg.py:157-158) */
int pgx_set_alpha(pgx_handle* h, double alpha);

/* F(x) with the callback contract of problem.py:54-67. x==NULL -> use device `sol`. F may be NULL. */
int pgx_residual(pgx_handle* h, const double* x, double* F, double* fnorm);
/* Fill the Jacobian values at x (x==NULL -> device `sol`) into the fixed pattern. */
int pgx_jacobian_fill(pgx_handle* h, const double* x);

/* Scalar pattern shared by the four blocks [[alpha*K, M],[M, -D]]:
 * call once with arrays NULL to get sizes, then with host buffers to receive copies.
 * K, M are the unconstrained blocks; bc rows/cols are applied by the operator. */
int pgx_csr_export(pgx_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col,
                   double* K, double* M, double* D);

/* y = J x with J = Jacobian of the last pgx_jacobian_fill, incl. BC rows/cols (identity). */
int pgx_spmv(pgx_handle* h, const double* x, double* y);
/* Time `reps` SpMV launches on device-resident data with HIP events on the handle's stream, in the cache state of a solve
 * rather than back to back (the matrix-free kernel's footprint would fit the 256 MB Infinity Cache): multigrid handles replay
 * "one V-cycle producing z, then J z" as an FGMRES iteration does and subtract the time of the V-cycles alone; other handles
 * sweep 512 MB of idle storage between two applies.  Returns the average ms per launch and the algorithmic bytes one launch
 * moves. */
int pgx_spmv_bench(pgx_handle* h, int reps, double* avg_ms, double* algorithmic_bytes);
/* The same measurement with every apply preceded by a 512 MB sweep of unrelated device storage: the kernel's operands come from
 * HBM, not from the 256 MB Infinity Cache (the operator of the 2048^2 benchmark, 273 MB, would otherwise mostly sit in it).
 * bench.py reports it as roofline.cold_frac next to the in-solve figure. */
int pgx_spmv_bench_cold(pgx_handle* h, int reps, double* avg_ms, double* algorithmic_bytes);
/* Sharded handles: collectives issued by THIS rank since the last reset - [0] halo exchanges (one grouped send/recv batch with
 * both strip neighbours each), [1] all-reduces, [2] V-cycles, [3] Krylov iterations.  Zeros on unsharded handles. */
int pgx_comm_counts(pgx_handle* h, int64_t out[4], int reset);
/* Operator apply of the outer Krylov solver ("SpMV").  kind 1 (default on structured P1 meshes): matrix-free stencil kernel
 * k_st_spmv_r - K, M are the uniform mesh's constants, D(psi) its half-stored 7-point stencil, 65 B per vertex; kind 0: the
 * block-CSR stream kernel k_bspmv_stream (what general meshes and P2 always use, 232 B per P1 row); kind 2: generic
 * one-thread-per-vertex stencil kernel (A/B); kind -1: query only.  *active (may be NULL) receives the kind that will run on
 * this handle (0 when the mesh has no grid structure).  pgx_spmv / pgx_spmv_bench follow the selection; pgx_spmv_bench's
 * `bytes` are the algorithmic bytes of the selected kernel.  P2 handles (round 4): kind 3 (or 1; the default on the uniform
 * structured mesh) = the structured apply of csrc/pgx_p2st.hip - interior vertex / edge groups through a 46-entry table, no column
 * indices, D(psi) from a structure-of-arrays copy, 496 B per group; the frame rows in CSR form -, kind 0 = the block-CSR kernel
 * k_bspmv_bal; *active is 3 or 0. */
int pgx_spmv_select(pgx_handle* h, int kind, int* active);
/* P2 handles: out = {state, i0, ni, j0, nj} of the structured apply - state 0: not available on this mesh (general meshes,
 * fewer than 8 cells per side, a pattern or K / M entries that are not those of the uniform right-diagonal mesh), 1: pattern verified,
 * 2: in use; the interior groups are the vertices (i, j), i0 <= i < i0 + ni, j0 <= j < j0 + nj, with their three edges. */
int pgx_p2_stencil_info(pgx_handle* h, int32_t out[5]);
/* (P2 handles: pgx_smoother_bench times one additive patch sweep - k_patch_apply + k_patch_edges - on the inverses of the last
 * Jacobian; `bytes` = inverses + dof table + residual and iterate of the patch dofs + the parked edge contributions.) */
/* The same for the TIME-DOMINANT kernel of the multigrid-preconditioned solve: the fused three-sweep smoother of the finest
 * level (k_st_smoothR, post-smoothing variant: x + P x_c folded in), at the Jacobian of the last pgx_jacobian_fill.
 * algorithmic_bytes = one pass over the level: 4 D-stencil arrays + b (2) + x (2) + the coarse correction (2 arrays of n/4) read,
 * the new iterate (2) written.  PGX_ESTATE on meshes without a grid hierarchy. */
int pgx_smoother_bench(pgx_handle* h, int reps, double* avg_ms, double* algorithmic_bytes);

/* Tuning / A-B / test switches (kernel variants, tile sizes, thresholds, consistency checks such as PGX_CHECK_REPLICAS).
 * libpgx.so never reads them from the environment: they exist only in a process-wide table filled through this call
 * (value NULL clears the key; keys start with "PGX_").  Most are read when a handle is created.  The environment variables the
 * library itself honours are the three documented run-time options: PGX_COMM_TIMEOUT (seconds a transport wait may take),
 * PGX_ROCTX (roctx ranges around the solver phases) and PGX_ND_THREADS (host threads of the symbolic factorisation).
 * tools/ and tests/ opt in to the old behaviour through the Python loader (PGX_TUNING_FROM_ENV=1 copies PGX_* variables into the
 * table before each create). */
int pgx_tuning_set(const char* key, const char* value);
/* Measurement aid: average device time (HIP events on the handle's stream, launches back to back) of the part of one V(nu,nu)
 * cycle that starts on multigrid level `level` (0 = the whole preconditioner application; -1 = the fused tail launch only) with the
 * default nu and damping.  *n_level receives the vertex count of that level.  bench.py reports the "coarse part" (levels of at most
 * 513^2 vertices) with it.  Same preconditions as pgx_smoother_bench. */
int pgx_vcycle_bench(pgx_handle* h, int level, int reps, double* avg_ms, int* n_level);

/* ---- Test hooks of the multigrid preconditioner.  They replace nothing in the reference (which factorises the Newton matrix with
 * MUMPS, obstacle_pg.py:129-131, and has no multigrid cycle): like the pgx_nd_export_* family they exist so that tests can compare
 * what the device stores and computes with a numpy statement of the same algebra (tests/vcycle_reference.py).  Preconditions of both:
 * those of pgx_vcycle_bench - a structured single-GPU P1 handle with a hierarchy of at least two levels and a filled Jacobian, not
 * sharded, the LU preconditioner not active; anything else is PGX_ESTATE with a message, and nothing is launched.  Neither changes
 * how a solve runs: they read the buffers and make the calls that pgx_vcycle_bench and pgx_spmv_bench make. */
/* Host copies of what multigrid level `level` (0 = finest .. the coarsest, levels inside the fused tail included) stores after the
 * last pgx_jacobian_fill; every array may be NULL (sizes only: n = (*nx + 1) * (*ny + 1) vertices, v = j * (*nx + 1) + i).
 *   Dh4  [4n]  the fp64 D(psi) stencil in its half-stored slot order S[slot * n + v], slots 0:(0,0) 1:(+1,0) 2:(0,+1) 3:(+1,+1)
 *   Dq4  [4n]  the single-precision cycle's copy of it, decoded to four floats PER VERTEX in the same slot order, Dq4[4 v + slot]:
 *              bf16 words shifted up (*dbf16 != 0), float4 copied; written only where *f32 != 0
 *   mask [n]   1 = Dirichlet dof of the u block on this level
 *   *f32, *dbf16   the level carries single-precision storage / stores Dq as bf16
 * Copies only, after a synchronisation of the handle's stream.  PGX_EINVAL: no such level. */
int pgx_mg_level_export(pgx_handle* h, int level, int32_t* nx, int32_t* ny, double* Dh4, float* Dq4, uint8_t* mask, int32_t* f32,
                        int32_t* dbf16);
/* z = ONE V(nu, nu) cycle for b, entered on `level` from a zero guess exactly as the solver enters it; b and z are host vectors
 * [u | psi] of 2 n_level entries.  Level 0 runs through the preconditioner entry of FGMRES (right-hand side in the Krylov scratch,
 * result in the operator scratch); a level > 0 whose single-precision legs run at this nu takes b as interleaved (u, psi) float
 * pairs, converted on the host, and returns the float pairs widened; any other level > 0 - the first level of the fused tail
 * included - takes and returns fp64.  Levels 0 .. the first tail level (the coarsest level where there is no fused tail); beyond:
 * PGX_EINVAL.  On a level > 0 the u part of b must be 0 on that level's Dirichlet rows, as every restricted residual is (the fused
 * tail relies on it); PGX_EINVAL otherwise.  On level 0 only:
 *   in_form  0: the fp64 pair, multiplied by `scale` as the first launch reads it (FGMRES's lazily normalised basis vectors);
 *            1: the pair of float fields of FGMRES's float basis (the hook converts b and owns the device copy)
 *   out_form 0: fp64;  1: the interleaved float2 field FGMRES keeps as Z_j, widened - only on handles that run this form
 *               (PGX_Z_F32 with the matrix-free apply and a single-precision level 0), otherwise PGX_ESTATE
 * in_form 1 and scale != 1 need the single-precision cycle on level 0 (PGX_EINVAL otherwise: the fp64 cycle reads neither).  nu must
 * be one the entered single-precision level runs (even, or a multiple of 3 with PGX_FUSED_K3): PGX_EINVAL otherwise, never another
 * path.  The handle's input / output form state is back at its defaults on return, on every path. */
int pgx_vcycle_apply(pgx_handle* h, int level, int nu, double omega, int in_form, int out_form, double scale, const double* b,
                     double* z);

/* (pgx_mg_level_export also serves structured P2 handles: their levels are the P1 hierarchy below the P2 level, level 0 holding
 * D = T^T D_P2 T, the coarse space of the two-level cycle.  pgx_vcycle_apply keeps its P1 precondition.) */

/* ---- Refined general meshes: a multigrid hierarchy given by topology alone (csrc/pgx_umg.hip) ----
 * A mesh that came out of uniform (red) refinement has the nested P1 hierarchy; this call hands it to a single handle of degree 1 or 2.  A
 * degree-1 handle then preconditions FGMRES with the collective-smoother V-cycle on block-CSR levels, as the structured handles do on
 * stencils.  Under a degree-2 handle the hierarchy is the coarse solve of the two-level patch cycle (below): `parents` still speak of
 * vertices, level 0 is the handle's P1 block CSR with D = T^T D_P2 T (refreshed by every Jacobian fill), and level-l vectors have
 * 2 n_l vertex entries.
 *   n_transfers       number of refinements to undo (>= 1); level 0 is the handle's mesh, level t + 1 has n_coarse[t] vertices
 *   n_coarse[t]       strictly decreasing, n_coarse[0] < n_vertices
 *   parents[t]        [n_fine_t][2] with n_fine_0 = n_vertices, n_fine_t = n_coarse[t - 1]: (v, v) for the first n_coarse[t] rows (a
 *                     vertex keeps its number on the coarser level), the two ends of the bisected edge for every other row
 * The prolongation has two entries of 1/2 per row; level t + 1 stores P^T K P, P^T M P and - after every Jacobian fill - P^T D P of
 * the unconstrained level-t values; the Dirichlet set of a level is the fine one on the inherited vertices.  Order-2 geometry needs
 * nothing extra: the products start from whatever values level 0 holds.
 * Call it after pgx_create / pgx_create_curved and before the first Jacobian fill (PGX_ESTATE afterwards, and on a second call).
 * PGX_EINVAL, with a message and nothing launched or changed: a structured, sharded or LU-distributed handle; a parent
 * index outside the coarse level; a transfer whose first n_coarse[t] rows are not (v, v) (or a later row that is); n_coarse not
 * strictly decreasing.
 * Solver selection with a hierarchy attached: pc_type 1 runs the cycle (tuning key PGX_UMG=0: the single-level smoother, for A/B),
 * 2 the sparse LU, 0 the cycle from PGX_UMG_MIN vertices up and the LU below.  Degree 2: 1 the two-level patch cycle over this hierarchy
 * (it needs the patch smoother: largest vertex degree <= 15), 2 the LU, 0 the cycle first from PGX_UMG_MIN_P2 vertices up, with the
 * sparse-LU rescue of structured P2 after PGX_P2_FALLBACK_ITS iterations, and the LU below.  The coarsest level runs PGX_UMG_COARSE_SWEEPS (60)
 * smoother sweeps, in one launch where it fits the LDS of one workgroup (PGX_UMG_COARSE_LDS=0: as separate launches). */
int pgx_set_hierarchy(pgx_handle* h, int32_t n_transfers, const int32_t* n_coarse, const int32_t* const* parents);
/* ---- General meshes WITHOUT a refinement hierarchy: the hierarchy built from the matrix (csrc/pgx_amg.hip) ----
 * A sibling of pgx_set_hierarchy for a mesh that has no `parents` arrays - one read from a file, an unrefined gmsh mesh.  Per transfer,
 * from the unconstrained stiffness matrix K of the level and its Dirichlet mask:
 *   strength    j is strong for i where a_ij < 0 and -a_ij >= theta max_k (-a_ik); the graph is symmetrised
 *   C/F split   greedy maximal independent set over strong edges between vertices of one kind (Dirichlet - Dirichlet, interior -
 *               interior), Dirichlet vertices first, each kind by ascending index; coarse vertices keep their order
 *   P           direct interpolation (a Dirichlet row from Dirichlet C vertices only), one Jacobi step P <- P - diag(K)^-1 K P on the
 *               interior F rows, entries below trunc x the row's largest magnitude dropped and the row rescaled to its sum
 *   stopping    at <= min_coarse vertices, or before a step that would keep more than max_keep of the vertices
 * theta < 0, trunc < 0, min_coarse <= 0, max_keep <= 0 take the defaults 0.01, 0.2, 60, 0.8; trunc must be > 0 (PGX_EINVAL otherwise).  The split and all patterns are host work;
 * the values of P, the Galerkin products P^T K P, P^T M P (here, once) and P^T D P (every Jacobian fill), restriction and prolongation are
 * fp64 gather kernels without atomics, bitwise reproducible.  The levels, the smoother, the coarsest level, the solver selection (PGX_UMG,
 * PGX_UMG_MIN, PGX_UMG_MIN_P2, PGX_UMG_COARSE_SWEEPS, PGX_UMG_COARSE_LDS) and the role under a degree-2 handle are those of
 * pgx_set_hierarchy above.  *n_levels (may be NULL): levels built, >= 2.  seconds (may be NULL): [0] the host pass, [1] device work
 * and copies.
 * Call order as pgx_set_hierarchy: after create, before the first Jacobian fill; one hierarchy per handle, attached or built (PGX_ESTATE
 * otherwise).  PGX_EINVAL, with a message and nothing launched or changed: a structured, sharded or LU-distributed handle; a parameter
 * out of range; a mesh of no more than min_coarse vertices, or one whose first step keeps more than max_keep of them. */
int pgx_build_hierarchy(pgx_handle* h, double theta, double trunc, int32_t min_coarse, double max_keep, int32_t* n_levels, double* seconds);
/* Where the split and the patterns of pgx_build_hierarchy are computed: on the device (csrc/pgx_amg_build.hip; the default), or, with
 * the tuning key PGX_AMG_BUILD=0 (read when the handle is created), in the serial host pass that did it before.  Both build bitwise the
 * same hierarchy - split, numbering, patterns, the order inside every plan row, hence P, K, M, D of every level - and refuse the same
 * inputs with the same messages (a mesh with a row without its diagonal AND a plan beyond int32 gets the first of these from the
 * device pass, whichever row order meets first from the host pass); what the text above calls host work is device work on the default
 * path, where seconds[1] is the time the host waited for the device or copied (the reads that end the split and size the arrays, the
 * downloads of the mirrors) and seconds[0] everything else it did: launches, allocating and freeing device memory, bookkeeping.  The device split runs as launches that each decide every vertex whose lower-numbered strong
 * neighbours are decided, until a counter read every 16 launches shows none left (PGX_AMG_SPLIT_BATCH, for tests, lowers the 16).
 * pgx_amg_build_info: *mode = 1 device pass, 0 host pass; *n_transfers = levels - 1; split_launches[t] = launches of the split of
 * transfer t (device pass: >= 1 and <= the vertices of level t; host pass: 0).  Every pointer may be NULL.  PGX_ESTATE on a handle
 * without a built hierarchy. */
int pgx_amg_build_info(pgx_handle* h, int32_t* mode, int32_t* n_transfers, int32_t* split_launches);
/* 1 where a front end should call pgx_build_hierarchy (with the defaults) by itself for a handle that is to run with snes option
 * pc_type: a general, single, not LU-distributed handle without a hierarchy and before its first fill, pc_type 1 (the multigrid
 * preconditioner asked for), from PGX_UMG_BUILD_MIN (2 000) vertices up - below, the single-level smoother such a handle always ran is
 * kept.  pc_type 0 (auto) keeps the sparse LU on such meshes: 0. */
int pgx_build_hierarchy_default(const pgx_handle* h, int pc_type);
/* Test hook: transfer t of a built hierarchy (level t + 1 -> level t) as CSR; every array may be NULL.  PGX_ESTATE without a built
 * hierarchy, PGX_EINVAL: no such transfer.  numpy twin: tests/amg_reference.py. */
int pgx_umg_transfer_export(pgx_handle* h, int t, int32_t* n_fine, int32_t* n_coarse, int32_t* nnz, int32_t* rowptr, int32_t* col, double* val);

/* Test hooks of that hierarchy (attached or built), in the style of pgx_mg_level_export / pgx_vcycle_apply (whose preconditions and behaviour they leave
 * alone; numpy twin: tests/umg_reference.py).  Both need an attached hierarchy (PGX_UMG on), a filled Jacobian and the sparse LU not
 * active: PGX_ESTATE otherwise, nothing launched.
 * Level `level` (0 = the handle's own block CSR): *n vertices, *nnz entries, the CSR pattern, the stored unconstrained K, M, D values
 * and the Dirichlet mask; every array may be NULL.  Copies only.  PGX_EINVAL: no such level. */
int pgx_umg_level_export(pgx_handle* h, int level, int32_t* n, int32_t* nnz, int32_t* rowptr, int32_t* col, double* K, double* M, double* D,
                         uint8_t* mask);
/* z = ONE V(nu, nu) cycle for b, entered on `level` from a zero guess; host vectors [u | psi] of 2 n_level entries.  Level 0 runs
 * through the preconditioner entry of FGMRES (degree 2, whose entry is the two-level cycle: through the level-0 cycle that cycle calls;
 * b and z have 2 n_vertices entries).  On a level > 0 the u part of b must be 0 on that level's Dirichlet rows, as every
 * restricted residual is; PGX_EINVAL otherwise. */
int pgx_umg_cycle_apply(pgx_handle* h, int level, int nu, double omega, const double* b, double* z);

/* ---- Test hooks of the P2 two-level preconditioner (pgx_cycle.hip: pcycle_p2_patch; pgx_patch.hip): patch_nu additive vertex-star
 * sweeps | restriction to the P1 hierarchy | one P1 V-cycle | prolongation | patch_nu sweeps.  They replace nothing in the reference
 * (which factorises the P2 Newton matrix as well, obstacle_pg.py:68-70,129-131): they let tests compare what the device stores and
 * computes, stage by stage, with a numpy statement of the same algebra (tests/p2_cycle_reference.py).  Preconditions of all three: a
 * single-GPU P2 handle with a patch smoother (vertex degree <= 15; <= 7 under PGX_P2_PATCH_WIDE=0; PGX_P2_PATCH on), a filled Jacobian, not sharded, the sparse LU
 * not active; anything else is PGX_ESTATE with a message, and nothing is launched.  None changes how a solve runs: they make the
 * calls the cycle makes, on the cycle's own buffers. */
/* out = { [0] slots per patch NN (7 or 8; a patch matrix has 2 NN rows),
 *         [1] storage form of the inverses: 0 double full rows, 1 float full rows, 2 float symmetric packing, 3 bf16 symmetric packing,
 *         [2] patch_nu (sweeps per leg),
 *         [3] 1: the residual inside the cycle reads the float copy of D(psi),
 *         [4] residual kernel of the cycle: 2 structured apply (interior) + CSR rows (frame), 1 nnz-balanced CSR, 0 plain CSR,
 *         [5] Newton solves since create in which the patch cycle stagnated (p2_fallback_its Krylov iterations without convergence)
 *             and the sparse LU took over,
 *         [6] 1: kernel [4] = 1 reads K and M through its dictionary (values on a grid of 2^-40 of the largest entry),
 *         [7] 1: the handle has the P1 hierarchy the whole cycle needs (stage 0 below): the grid hierarchy of a structured mesh, or an
 *             attached one (pgx_set_hierarchy) };  *patch_omega (may be NULL): damping
 * of the sweeps.  Brings the patch data up to date for the current Jacobian, as the first cycle of a solve does. */
int pgx_p2_cycle_info(pgx_handle* h, int32_t out[8], double* patch_omega);
/* Host copies of the patch data of the current Jacobian (either may be NULL); nv patches, patch p = vertex p:
 *   pdof [nv][NN]         dofs of the scalar space in the patch, slot 0 the vertex, then its edge dofs, -1 = unused slot
 *   Ainv [nv][2NN][2NN]   the stored inverse, decoded exactly as k_patch_apply decodes it: entry (l, j) is the factor of r_j in row l,
 *                         rows / columns = (u slots, psi slots).  Symmetric packing: the chunks at or left of a row's diagonal block
 *                         as stored, the rest as the kernel mirrors them; bf16 words shifted up; float and double cast. */
int pgx_p2_patch_export(pgx_handle* h, int32_t* pdof, double* Ainv);
/* Wide stars.  A star of vertex degree 8 ... 15 does not fit the 16 lanes of a narrow patch.  On a mesh whose largest degree lies in
 * that range NN is 8, the vertices of degree >= 8 form the wide set - their rows of pdof above are all -1 and their narrow inverses the
 * identity - and a second pair of kernels (32 lanes per star, 16 slots, inverses in full rows, float or, where the narrow form is
 * double, double) serves them inside the same sweep.  Largest degree > 15, or PGX_P2_PATCH_WIDE=0 with degree > 7: no patch smoother.
 *   *nw                  number of wide stars (0 on most meshes; then nothing else is written)
 *   verts [nw]           their vertices, ascending
 *   wdof  [nw][16]       slot 0 the vertex, then its edge dofs, -1 = unused slot
 *   Ainv  [nw][32][32]   the stored inverses as k_patch_apply_wide reads them, rows / columns = (16 u slots, 16 psi slots)
 * Every pointer may be NULL; preconditions as pgx_p2_patch_export. */
int pgx_p2_wide_export(pgx_handle* h, int32_t* nw, int32_t* verts, int32_t* wdof, double* Ainv);
/* One stage of the cycle on host vectors ([u | psi] of the P2 space, 2 nd entries, unless stated), through the launches of the cycle:
 *   stage 1  one sweep, z = x0 + sweep(b - J x0): the cycle's residual kernel, then the patch sweep; x0 == NULL: the first sweep of
 *            a cycle (x = 0, r = b, no residual launch)
 *   stage 2  the residual inside the cycle alone, z = b - J x0
 *   stage 3  z [2 nv] = T^T b, the restriction to the P1 space (u rows of Dirichlet vertices 0)
 *   stage 4  z = x0 + T b with b [2 nv] (x0 == NULL: 0), the prolongation
 *   stage 0  the whole preconditioner, entered exactly as FGMRES enters it, with a V(nu, nu) cycle of damping omega below; needs
 *            the grid hierarchy or an attached one (PGX_ESTATE otherwise); x0 must be NULL
 * nu and omega are read by stage 0 only (the sweeps use patch_nu and patch_omega of the handle). */
int pgx_p2_cycle_apply(pgx_handle* h, int stage, int nu, double omega, const double* b, const double* x0, double* z);

/* One nonlinear solve from device `sol` with proximal centre `sol_k`; on reason>0 `sol` is replaced. */
int pgx_newton_solve(pgx_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
/* energy, |complementarity|, feasibility, dual feasibility, H1 increment, latent L2 increment */
int pgx_observables(pgx_handle* h, double out[6]);

/* Test hook: the second stage of the Krylov driver's reductions as a launch of its own against the same stage run by the last
 * workgroup of the producer launch (run-time option PGX_TICKET_REDUCE).  In the handle's own Krylov storage it fills nv basis
 * vectors (basis_f32 != 0: stored as float) and a vector of `len` entries from `seed`, and `reps` times, on new data each time,
 * computes the nv dot products and the projection w' = w - V h with |w'|^2 by both routes from equal inputs.  *mismatches = the
 * number of 8-byte words - results on the device, results sent to the host, the stored w' - that differ: 0 is the only right
 * answer.  len even, 2 <= len <= the handle's number of dofs; single handles with the polled read-back only (PGX_EINVAL
 * otherwise).  Changes no state a solve reads. */
int pgx_reduce_selfcheck(pgx_handle* h, int nv, int64_t len, int basis_f32, int reps, uint64_t seed, int64_t* mismatches);

/* Entry evaluations of pgx_newton_solve since the handle was created (or the last reset): out[0] in full, out[1] reduced to the first
 * residual row.  A solve of a single degree-1 handle on a uniform structured mesh that starts at the iterate where the converged solve
 * before it ended - only the proximal centre and alpha changed in between, the LVPP loop's case - takes F_psi and D(psi) over from that
 * solve's last evaluation and computes F_u only (tuning key PGX_RESID_REUSE, default 1; 0: always in full).  Any other call on the handle
 * in between, apart from pgx_get_state, pgx_get_prev, pgx_set_prev, pgx_advance_prev, pgx_set_alpha, pgx_observables and the profile
 * calls, makes the next entry evaluation a full one.  Same bits either way. */
int pgx_resid_reuse_counts(pgx_handle* h, int64_t out[2], int reset);
/* Test hook of the above, to be called where the next pgx_newton_solve would reduce its entry evaluation (PGX_EINVAL otherwise): runs
 * that evaluation reduced, then in full, at the current sol, sol_k and alpha, and counts differing words.  out[0] entries of F_u that
 * differ between the two; out[1] entries of F_psi, out[2] 8-byte words of the stored D(psi) copies (level-0 stencil forms, CSR rows)
 * that the reduced evaluation changed; out[3], out[4] the same two counts for the held values against the full evaluation's;
 * out[5] the number of vertices.  0 in out[0 .. 5) is the only right answer.  The next entry evaluation is a full one. */
int pgx_resid_reuse_selfcheck(pgx_handle* h, int64_t out[6]);

/* Accumulated device-time per phase since the last reset, ms (HIP events; only when enabled):
 * [0] residual [1] jacobian fill [2] mg setup [3] spmv (outer Krylov) [4] v-cycle [5] orthogonalisation
 * [6] observables [7] total newton_solve wall */
int pgx_profile_enable(pgx_handle* h, int on);
int pgx_profile_get(pgx_handle* h, double ms[8], int reset);

/* ---------------------------------------------------------------------------------------------------------
 * Sharded path: one handle per GPU, the structured mesh cut into horizontal strips of
 * vertex rows.  Replaces what the reference inherits from DOLFINx/PETSc over MPI:
 *   Vec.ghostUpdate(INSERT, FORWARD)   src/lvpp/problem.py:56,58,71,73  -> halo exchange of ghost vertex rows
 *   F.ghostUpdate(ADD, REVERSE)        src/lvpp/problem.py:66           -> not needed: ghost cells are assembled
 *                                                                          redundantly (owner computes whole rows)
 *   comm.allreduce(scalar)             obstacle_pg.py:50 (six calls :196-201), SNES/KSP norms and dots
 *                                                                       -> ONE packed all-reduce per use
 * Every rank passes its LOCAL strip (owned rows + ghost rows, see pgx_partition_rows) as an ordinary structured
 * pgx_mesh / pgx_problem; vectors crossing the ABI are local (owned + ghost entries), like DOLFINx's x.array.
 * All calls on a sharded handle are COLLECTIVE: every rank of the communicator must make the same calls in the
 * same order.  Iteration counts and results equal the single-handle solve (same algebra; only the summation
 * order of dot products differs).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct pgx_comm pgx_comm; /* opaque: neighbour halo exchange + all-reduce(sum) on device buffers */

typedef struct pgx_partition {
  int32_t rank, size;   /* strip index (0 = lowest rows) and number of strips */
  int32_t global_ny;    /* cell rows of the GLOBAL mesh; must be divisible by size * 2^dist_levels */
  int32_t dist_levels;  /* multigrid levels kept distributed (ghost depth 2^dist_levels on the fine grid);
                           coarser levels are replicated on every rank.  0 = choose (at most 3) */
} pgx_partition;

/* Which global vertex rows the local mesh of `part->rank` must contain: rows [row0, row0+nrows), of which
 * [own0, own0+nown) are owned (the others are ghosts).  Fills part->dist_levels when it was 0.  No GPU needed. */
int pgx_partition_rows(pgx_partition* part, int32_t* row0, int32_t* nrows, int32_t* own0, int32_t* nown);

/* RCCL transport, one process per GPU (torch.distributed launch): rank 0 creates the id, the host broadcasts
 * the 128 bytes by any means, every rank calls init.  ncclSend/ncclRecv to the two strip neighbours over xGMI,
 * ncclAllReduce for packed scalars - all enqueued on the handle's stream (no host synchronisation). */
int pgx_comm_rccl_unique_id(char id[128]);
int pgx_comm_rccl_init(const char id[128], int rank, int size, int device, pgx_comm** out);
/* In-process transport: `size` communicators for `size` handles driven by `size` host threads of ONE process
 * (any mix of devices, also all on one GPU).  Same call sequence as RCCL through host-synchronised device
 * copies; used by the test-suite to run the sharded algorithm on a single-GPU box. */
int pgx_comm_local_group(int size, pgx_comm** out /* [size] */);
/* Inter-PROCESS transport through a POSIX shared-memory segment `name` ("/..."; rank 0 creates it, the others attach, the name
 * is unlinked once all ranks are in), host-staged: one communicator per process, any mix of devices - also several processes on
 * ONE GPU, which RCCL refuses.  A torch.distributed.run launch with this transport executes everything the multi-GPU launch
 * does except RCCL's byte movement (mpirun-style process model of the reference: obstacle_pg.py:64, problem.py:56-73).
 * slot_bytes: mailbox per rank (0 = 64 MiB; larger payloads move in chunks).  host_mode != 0: the buffers handed to the
 * operations are HOST memory (protocol tests on machines without a GPU).  A peer that does not arrive within
 * PGX_COMM_TIMEOUT seconds (default 120) fails every rank with PGX_ECOMM instead of hanging. */
int pgx_comm_shm_init(const char* name, int rank, int size, uint64_t slot_bytes, int host_mode, pgx_comm** out);
/* the four operations of a communicator, callable directly (tests): in-place sum over the ranks; exchange of the entries
 * [send_lo, +n_send_lo) / [send_hi, +n_send_hi) of f0 (and f1 if non-null) with rank-1 / rank+1 into [recv_lo, ...) /
 * [recv_hi, ...); rank r > 0 -> rank 0 at recv0 + r*n; rank 0's send0 + r*n -> rank r.  Buffers: device memory, or host
 * memory for a host_mode communicator. */
int pgx_comm_allreduce(pgx_comm* c, double* buf, uint64_t n);
int pgx_comm_halo(pgx_comm* c, double* f0, double* f1, uint64_t send_lo, uint64_t n_send_lo, uint64_t recv_lo, uint64_t n_recv_lo,
                  uint64_t send_hi, uint64_t n_send_hi, uint64_t recv_hi, uint64_t n_recv_hi);
int pgx_comm_gather0(pgx_comm* c, const double* send, uint64_t n, double* recv0);
int pgx_comm_scatter0(pgx_comm* c, const double* send0, uint64_t n, double* recv);
/* Self-check before the first solve: one halo exchange with both strip neighbours and one packed all-reduce on a known pattern,
 * verified, each bounded by timeout_s (<= 0: 10 s).  Collective.  host != 0 for a host_mode communicator.  On failure the text
 * (pgx_comm_last_error) names the operation that failed or did not complete; the caller should end the process (a collective
 * that hangs cannot be cancelled).  Replaces nothing in the reference - MPI_Init fails loudly by itself; RCCL over a mis-wired
 * launch does not. */
int pgx_comm_selfcheck(pgx_comm* c, int host, double timeout_s);
void pgx_comm_free(pgx_comm* c);
const char* pgx_comm_last_error(void);

int pgx_create_sharded(const pgx_mesh* local_mesh, const pgx_problem* local_prob, const pgx_partition* part,
                       pgx_comm* comm, int device, pgx_handle** out);
/* Replicated handles with a DISTRIBUTED sparse LU (BASELINE.json config 3: P2 on 8 GPUs, where the multigrid path is not
 * robust and one GPU cannot hold the factor): every rank passes the WHOLE mesh / problem and keeps the whole iterate;
 * assembly, SpMV and the Krylov vectors are replicated, the LU preconditioner - the dominant cost - is factorised with one
 * dissection subtree per rank (include/pgx_nd.h: pgx_nd_create_dist).  Residuals and observables are broadcast from rank 0
 * so that the replicas stay bitwise identical.  All calls are collective; results are identical on every rank.  Replaces
 * `mpirun -n N python obstacle_pg.py` with MUMPS distributing the factorisation (obstacle_pg.py:129-131). */
int pgx_create_lu_dist(const pgx_mesh* mesh, const pgx_problem* prob, pgx_comm* comm, int device, pgx_handle** out);
/* Owned VERTEX dofs of a local vector: each field block holds them at [offset, offset+count) (everything - all n vertex dofs - on
 * an unsharded handle).  P1: that is the whole field.  P2: the field block is [vertex dofs | edge dofs] and this call reports the
 * vertex part ONLY, on sharded and unsharded handles alike: a caller that slices the owned dofs of a P2 field must combine it
 * with pgx_owned_edge_range below (on an unsharded P2 handle: all vertices + all edges). */
int pgx_owned_range(const pgx_handle* h, int64_t* offset, int64_t* count);
/* P2 handles: the owned EDGE dofs of each field block as (offset within the field block, count); the vertex dofs are what
 * pgx_owned_range reports.  An edge belongs to the rank that owns its lower vertex; edge dofs are numbered by their lower vertex,
 * row by row, so the owned ones are contiguous.  Unsharded handles own every edge dof. */
int pgx_owned_edge_range(const pgx_handle* h, int64_t* offset, int64_t* count);
/* refresh the ghost entries of device `sol` and `sol_k` from their owners (after pgx_set_state / pgx_set_prev
 * with host arrays whose ghost entries are stale) */
int pgx_sync_ghosts(pgx_handle* h);

#ifdef __cplusplus
}
#endif
#endif
