/*
 * pgx_mp.h - C ABI of libpgx.so for example 04 (four-phase Cahn-Hilliard gradient flow with a simplex-constrained latent
 * variable): everything below `problem.solve()` in the reference's examples/04_multiphase/multiphase_dolfinx.py, i.e. DOLFINx
 * assembly + PETSc SNES newtonls with its default line search (bt of order 3, cubic) + MUMPS LU (:127-147), plus the
 * per-step vector updates of its time loop (:188-233), kept on the device.
 *
 * Mixed [P1^4, P1^4, P1^4] on a triangulation; x = [u | z | psi], each block vertex-major with the 4 species fastest
 * (index 4 v + m).  Rows [v | y | w] (sub-space k's test function tests row block k).  Residual (:61-87):
 *     R_v = (u, v) - tau (grad z, grad v) - (u_prev, v)
 *     R_y = alpha (z, y) + alpha epsilon^2 (grad u, grad y) - 2 alpha (u, y) + (psi - psi_old, y) - alpha (1, y)
 *     R_w = (u_m - exp(psi_m) / sum_n exp(psi_n), w_m) - eps (psi_m, w_m)
 * epsilon = 2 h, h = 2 Circumradius, per cell.  psi_old and u_old are the blocks of the previous LVPP iterate (set_prev /
 * advance_prev); u_prev is the previous time step (set_uprev / end_step).  Jacobian: the true derivative.
 *
 *   pgx_mp_create          NonlinearProblem(F, u=sol, bcs=[], petsc_options=...) construction (:127-147)
 *   pgx_mp_set/get_state, set/get_prev, advance_prev   sol.x.array, lvpp_old / u_old <- sol (:222-223)
 *   pgx_mp_set_alpha       alpha.value = ... (:203-208)
 *   pgx_mp_residual / pgx_mp_jacobian_fill / pgx_mp_csr_export / pgx_mp_spmv   SNES callbacks and the PETSc Mat
 *   pgx_mp_newton_solve    problem.solve(): opts->linesearch 3 = bt of order 3 (cubic), 1 = bt of order 2, 0 = full step
 *   pgx_mp_set/get_uprev   u_prev.x.array (:118-122, :226)
 *   pgx_mp_begin_step      psi of x and of the previous iterate <- ln(|u(x)| + 1e-7) + 1; u of the previous iterate <- 0 (:194-200)
 *   pgx_mp_end_step        u_prev <- u(x) (:226)
 *   pgx_mp_l2_increment    sqrt(assemble_scalar(dot(u - u_old, u - u_old) dx)) (:179-182, :212-213), exact P1 mass form
 *   pgx_mp_species_mass    int u_m dx, m = 0..3
 *   pgx_mp_lu_stats        pgx_nd_stats of the handle's sparse LU (perturbed_pivots: the 12-dof vertex blocks as they stand)
 * Conventions as in pgx.h.  Linear solves: sparse LU of pgx_nd.h (node = vertex, 12 dofs) + iterative refinement.
 * No CPU fallback.
 */
#ifndef PGX_MP_H
#define PGX_MP_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_nd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_mp_handle pgx_mp_handle;

typedef struct {
  int32_t nq;         /* quadrature points per cell (<= 16) of the softmax term; the polynomial terms are integrated exactly */
  const double* qpts; /* [nq][2] */
  const double* qwts; /* [nq], sum 1/2 */
  double tau, eps;    /* :80 tau = dt (1e-5 by default); :84 eps = 1e-9 */
} pgx_mp_problem;

/* mesh: pgx_mesh with n_vertices, n_cells, coords, cells (cell_dofs / structured_* ignored) */
int pgx_mp_create(const pgx_mesh* mesh, const pgx_mp_problem* prob, int device, pgx_mp_handle** out);
void pgx_mp_destroy(pgx_mp_handle* h);
const char* pgx_mp_last_error(const pgx_mp_handle* h);
int pgx_mp_num_dofs(const pgx_mp_handle* h, int64_t* ntot);
int pgx_mp_set_state(pgx_mp_handle* h, const double* x);
int pgx_mp_get_state(pgx_mp_handle* h, double* x);
int pgx_mp_set_prev(pgx_mp_handle* h, const double* x);
int pgx_mp_get_prev(pgx_mp_handle* h, double* x);
int pgx_mp_advance_prev(pgx_mp_handle* h);
int pgx_mp_set_alpha(pgx_mp_handle* h, double alpha);
int pgx_mp_residual(pgx_mp_handle* h, const double* x, double* F, double* fnorm);
int pgx_mp_jacobian_fill(pgx_mp_handle* h, const double* x);
int pgx_mp_csr_export(pgx_mp_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_mp_spmv(pgx_mp_handle* h, const double* x, double* y);
int pgx_mp_newton_solve(pgx_mp_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
int pgx_mp_profile(pgx_mp_handle* h, int enable, double ms[6]);
int pgx_mp_set_uprev(pgx_mp_handle* h, const double* u);  /* [4 n_vertices] */
int pgx_mp_get_uprev(pgx_mp_handle* h, double* u);
int pgx_mp_begin_step(pgx_mp_handle* h);
int pgx_mp_end_step(pgx_mp_handle* h);
int pgx_mp_l2_increment(pgx_mp_handle* h, double* out);
int pgx_mp_species_mass(pgx_mp_handle* h, double out[4]);
int pgx_mp_lu_stats(const pgx_mp_handle* h, pgx_nd_stats* st);

#ifdef __cplusplus
}
#endif
#endif
