/*
 * pgx_qmy.h - C ABI of libpgx.so for the two self-contained comparison solvers of example 05 (thermoforming quasi-variational
 * inequality): examples/05_obstacle_type_qvi/solver_comparison/thermoforming_moreau_yosida.jl (Moreau-Yosida path following on
 * the coupled system, "MY" below) and thermoforming_fixed_point.jl (fixed point in T with an inner Moreau-Yosida path for u,
 * "FP").  Everything below their `solve!` runs here: Gridap's assembly of the penalised residual and its generalised Jacobian,
 * NLsolve's Newton iteration, the sparse LU, the two functionals of the gamma update and the H1 "Cauchy" norm.
 *
 * Mixed [P1, P1] on a triangulation (MY:24-33); x = [u (nv) | T (nv)], u = 0 on the Dirichlet vertices (MY:27,29).  The scripts
 * interpolate the mould Phi0, the smoothing function phi and the load into P1 (MY:40-44), so the data are NODAL arrays.
 * With d = u - (Phi0 + phi T) and s = Phi0 + phi T - u at the quadrature points, residual (MY:77-81):
 *     R_u = (grad u, grad v) - (f, v) + gamma (max(0, d), v)
 *     R_T = (grad T, grad R) + (T, R) - (g(s), R)                g = 1 (s <= 0), 1 - s/q (0 < s < q), 0 (s >= q)   (MY:46-55)
 * and on the Dirichlet rows F = x.  Jacobian (MY:84-88), chi = [d > 0], g' = -1/q on 0 < s < q (MY:56-74):
 *     (u,u) = K + gamma M_chi     (u,T) = -gamma M_{chi phi}     (T,u) = M_{g'}     (T,T) = K + M - M_{g' phi}
 * Every block depends on the state and the matrix is not symmetric.  One quadrature rule serves every integral
 * (Measure(Omega, 11), MY:37; which rule Gridap takes for degree 11 is not pinned here - the Python layer passes the 36-point
 * collapsed Gauss-Jacobi rule of that degree).
 *
 *   pgx_qmy_create          FEOperator(a, jac, U, V) (MY:129), FEOperator(au, jacu, Uu, Vu) and FEOperator(aT, jacT, UT, VT) (FP:70-71)
 *   pgx_qmy_set/get_state, set/get_prev, advance_prev   zh / zh_ = copy_z(zh) (MY:124,128,147); uh, Th, u_ (FP:89,97,114-116)
 *   pgx_qmy_set_gamma       global gamma = ... (MY:134,150; FP:103,135)
 *   pgx_qmy_set_active      which operator the next calls assemble: 3 the coupled one (MY:129), 2 opT (FP:64-65), 1 opu (FP:62-63)
 *   pgx_qmy_residual / pgx_qmy_residual_inf / pgx_qmy_jacobian_fill / pgx_qmy_csr_export / pgx_qmy_spmv
 *                           Gridap.Algebra.residual / jacobian of the operator, NLsolve's norm(F, Inf)
 *   pgx_qmy_newton_solve    solve!(zh, solver, op) with NLSolver(method=:newton, linesearch=BackTracking(c_1=-1e8), ftol, xtol)
 *                           (MY:130-131,139; FP:118-122,92,131)
 *   pgx_qmy_functionals     sum(energy(uh)), sum(penalty(uh, Th)) (MY:97-98,101-102; FP:73-74,76-77)
 *   pgx_qmy_cauchy          sqrt(d' * J * d), J the H1 matrix on the free dofs of u (MY:92-94,144-145; FP:94-95,112,138-139)
 *   pgx_qmy_lu_stats        pgx_nd_stats of the handle's sparse LU (perturbed_pivots: of the last completed factorisation)
 * Conventions as in pgx.h.  Linear solves: sparse LU of pgx_nd.h + iterative refinement.  No CPU fallback.
 */
#ifndef PGX_QMY_H
#define PGX_QMY_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_nd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_qmy_handle pgx_qmy_handle;

typedef struct {
  int32_t nq;             /* quadrature points per cell (<= 36): one rule for every integral (MY:37) */
  const double* qpts;     /* [nq][2] */
  const double* qwts;     /* [nq], sum 1/2 */
  const double* Phi0;     /* [n_vertices] nodal values of the initial mould (MY:40) */
  const double* phi;      /* [n_vertices] nodal values of the smoothing function (MY:42) */
  double f, q;            /* MY:44 f = 25; MY:46 knee q = 0.01 of g */
  int32_t n_bc;           /* Dirichlet vertices of u (homogeneous, MY:27,29) */
  const int32_t* bc_dofs;
} pgx_qmy_problem;

/* NLsolve's newton with LineSearches.BackTracking (MY:130): stop on norm(F, Inf) <= ftol or norm(lambda delta, Inf) <= xtol */
typedef struct {
  double ftol, xtol;      /* MY:130 ftol = 1e-5 (FP:121 1e-10 for T), xtol = 10 eps */
  double c1;              /* Armijo parameter of the backtracking; the scripts pass -1e8, which accepts every finite trial */
  int32_t max_it;         /* NLsolve's default iterations = 1000; reaching it is reason 0, not an error */
  int32_t monitor;        /* show_trace (MY:130): 1 prints one line per iteration */
} pgx_qmy_newton_opts;

/* mesh: pgx_mesh with n_vertices, n_cells, coords, cells (cell_dofs / structured_* ignored) */
int pgx_qmy_create(const pgx_mesh* mesh, const pgx_qmy_problem* prob, int device, pgx_qmy_handle** out);
void pgx_qmy_destroy(pgx_qmy_handle* h);
const char* pgx_qmy_last_error(const pgx_qmy_handle* h);
int pgx_qmy_num_dofs(const pgx_qmy_handle* h, int64_t* ntot);
int pgx_qmy_set_state(pgx_qmy_handle* h, const double* x);
int pgx_qmy_get_state(pgx_qmy_handle* h, double* x);
int pgx_qmy_set_prev(pgx_qmy_handle* h, const double* x);
int pgx_qmy_get_prev(pgx_qmy_handle* h, double* x);
int pgx_qmy_advance_prev(pgx_qmy_handle* h);
int pgx_qmy_set_gamma(pgx_qmy_handle* h, double gamma);
/* mask: bit 0 = u, bit 1 = T.  A frozen field's rows are identity rows with zero residual and its columns in the other field's
 * rows are zero, so one symbolic factorisation serves the coupled solve (3), the T-solve (2) and the u-solve (1). */
int pgx_qmy_set_active(pgx_qmy_handle* h, int mask);
int pgx_qmy_residual(pgx_qmy_handle* h, const double* x, double* F, double* fnorm);
int pgx_qmy_residual_inf(pgx_qmy_handle* h, const double* x, double* finf);
int pgx_qmy_jacobian_fill(pgx_qmy_handle* h, const double* x);
int pgx_qmy_csr_export(pgx_qmy_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_qmy_spmv(pgx_qmy_handle* h, const double* x, double* y);
/* reason: 1 ftol reached (0 iterations if the start satisfies it), 2 xtol reached, 0 max_it reached, -4 no finite trial residual
 * within 50 halvings.  The state is the last accepted iterate in every case but -4. */
int pgx_qmy_newton_solve(pgx_qmy_handle* h, const pgx_qmy_newton_opts* opts, int* reason, int* its, int* lin_its);
int pgx_qmy_functionals(pgx_qmy_handle* h, double* energy, double* penalty);
int pgx_qmy_cauchy(pgx_qmy_handle* h, double* out);
int pgx_qmy_lu_stats(const pgx_qmy_handle* h, pgx_nd_stats* st);
int pgx_qmy_profile(pgx_qmy_handle* h, int enable, double ms[6]);

#ifdef __cplusplus
}
#endif
#endif
