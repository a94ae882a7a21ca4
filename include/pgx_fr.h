/*
 * pgx_fr.h - C ABI of libpgx.so for example 03 (phase-field fracture of a notched plate under load stepping, with the damage
 * irreversibility c_prev <= c <= 1 enforced through a latent variable): everything below `problem.solve()` in the reference's
 * examples/03_fracture/fracture_dolfinx.py, i.e. DOLFINx assembly with inhomogeneous Dirichlet data + PETSc SNES newtonls with
 * the l2 line search + MUMPS LU (:163-171, :204-206), plus the vector copies and norms of its load-step loop (:207-311), kept
 * on the device.
 *
 * Mixed [P1, P1, P1] on a triangulation (:79-81); x = [u | c | psi], n_vertices entries each.  Rows [v | d | phi] (sub-space
 * k's test function tests row block k).  With w(c) = (1 - eps) (1 - c)^2 + eps (:117-122) the residual is (:124-130)
 *     R_v   = alpha G (w(c) grad u, grad v)
 *     R_d   = alpha [ 1/2 G (w'(c) |grad u|^2, d) + Gc / l (c, d) + Gc l (grad c, grad d) ] + (psi - psi_iter, d)
 *     R_phi = (c - c_conform, phi),   c_conform = (c_prev + exp(psi)) / (exp(psi) + 1)                           (:114)
 * evaluated as c_prev + (1 - c_prev) sigma(psi) with an overflow-free logistic sigma.  psi_iter is the psi block of the
 * previous LVPP iterate z_iter (set_prev / advance_prev, :107-108), c_prev the c block of z_prev, the state of the last WRITTEN
 * load step (set_zprev / zprev_from_state, :105-106, :309).  Jacobian (:132-138): the true derivative plus reps (v, v_trial) +
 * reps (d, d_trial) - reps (phi, phi_trial); symmetric, blocks [[alpha E_uu, alpha E_uc, 0], [alpha E_cu, alpha E_cc, M],
 * [0, M, -D(psi) - reps M]], D = int (1 - c_prev) sigma (1 - sigma) phi_i phi_j.  The polynomial terms are integrated exactly
 * in closed form, the terms containing psi with the caller's rule (tri_deg7_gj16: UFL's degree estimate for them is 7).
 *
 * Dirichlet data (:141-160): u = -T on `topleft`, u = +T on `topright`, T the current load (set_load, :213-214).  DOLFINx's
 * contract for NonlinearProblem: F <- F_raw(x) + J_reg(x)[:, bc] (g - x_bc), then F[bc] = x_bc - g; the rows and columns of the
 * bc dofs of the Jacobian are zeroed, diagonal 1.  The state is not overwritten with g: the first Newton step does that.
 *
 *   pgx_fr_create            NonlinearProblem(F, z, bcs=bcs, J=J_reg, petsc_options=sp) construction (:204-206, :224-232)
 *   pgx_fr_set/get_state, set/get_prev, advance_prev   z.x.array, z_iter; z_iter.interpolate(z) (:216, :284)
 *   pgx_fr_set_alpha         alpha.value = ... (:215, :251, :278-281)
 *   pgx_fr_set_load          bcminus.value = -T; bcplus.value = T (:213-214)
 *   pgx_fr_residual / pgx_fr_jacobian_fill / pgx_fr_csr_export / pgx_fr_spmv   SNES callbacks and the PETSc Mat
 *   pgx_fr_newton_solve      problem.solve() (:233): opts->linesearch 2 = l2 with maxlambda 1 (:164-165), 1 / 3 = bt, 0 = full step
 *   pgx_fr_set/get_zprev     z_prev.x.array (:105)
 *   pgx_fr_zprev_from_state  z_prev.interpolate(z) (:309)
 *   pgx_fr_state_from_zprev  z.interpolate(z_prev) (:253)
 *   pgx_fr_state_from_prev   z.interpolate(z_iter) (:255)
 *   pgx_fr_l2_increment_c    sqrt(assemble_scalar(inner(c - c_iter, c - c_iter) dx)) (:187, :267), exact P1 mass form
 *   pgx_fr_l2_distance_zprev sqrt(assemble_scalar(inner(z - z_prev, z - z_prev) dx)) (:188, :292), all three blocks
 *   pgx_fr_conforming_damage c_conform at caller-given reference points of every cell (:111-115, :298: the P3 nodes)
 *   pgx_fr_lu_stats          pgx_nd_stats of the handle's sparse LU (perturbed_pivots: of the last completed factorisation)
 *   pgx_fr_lu_is_symmetric   whether that LU runs its symmetric L D L^T mode (the request is ignored where its kernels do not apply)
 * Conventions as in pgx.h.  Linear solves: sparse LU of pgx_nd.h (node = vertex, 3 dofs) in its symmetric L D L^T mode +
 * iterative refinement.  No CPU fallback.
 */
#ifndef PGX_FR_H
#define PGX_FR_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_nd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_fr_handle pgx_fr_handle;

typedef struct {
  int32_t nq;         /* quadrature points per cell (<= 16) of the terms containing psi */
  const double* qpts; /* [nq][2] */
  const double* qwts; /* [nq], sum 1/2 */
  double G, Gc;       /* :84-85 */
  double l;           /* :88-93 max over the cells of 4 Circumradius, computed once by the caller */
  double eps, reps;   /* :117 eps = 1e-5; :132 reps = 1e-3 */
  int32_t n_minus;
  const int32_t* minus_dofs; /* vertices of `topleft`: u = -T */
  int32_t n_plus;
  const int32_t* plus_dofs;  /* vertices of `topright`: u = +T */
} pgx_fr_problem;

/* mesh: pgx_mesh with n_vertices, n_cells, coords, cells (cell_dofs / structured_* ignored) */
int pgx_fr_create(const pgx_mesh* mesh, const pgx_fr_problem* prob, int device, pgx_fr_handle** out);
void pgx_fr_destroy(pgx_fr_handle* h);
const char* pgx_fr_last_error(const pgx_fr_handle* h);
int pgx_fr_num_dofs(const pgx_fr_handle* h, int64_t* ntot);
int pgx_fr_set_state(pgx_fr_handle* h, const double* x);
int pgx_fr_get_state(pgx_fr_handle* h, double* x);
int pgx_fr_set_prev(pgx_fr_handle* h, const double* x);
int pgx_fr_get_prev(pgx_fr_handle* h, double* x);
int pgx_fr_advance_prev(pgx_fr_handle* h);
int pgx_fr_set_alpha(pgx_fr_handle* h, double alpha);
int pgx_fr_residual(pgx_fr_handle* h, const double* x, double* F, double* fnorm);
int pgx_fr_jacobian_fill(pgx_fr_handle* h, const double* x);
int pgx_fr_csr_export(pgx_fr_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_fr_spmv(pgx_fr_handle* h, const double* x, double* y);
int pgx_fr_newton_solve(pgx_fr_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
int pgx_fr_profile(pgx_fr_handle* h, int enable, double ms[6]);
int pgx_fr_set_load(pgx_fr_handle* h, double T);
int pgx_fr_set_zprev(pgx_fr_handle* h, const double* z); /* [3 n_vertices] */
int pgx_fr_get_zprev(pgx_fr_handle* h, double* z);
int pgx_fr_zprev_from_state(pgx_fr_handle* h);
int pgx_fr_state_from_zprev(pgx_fr_handle* h);
int pgx_fr_state_from_prev(pgx_fr_handle* h);
int pgx_fr_l2_increment_c(pgx_fr_handle* h, double* out);
int pgx_fr_l2_distance_zprev(pgx_fr_handle* h, double* out);
/* ref_pts [npts][2] on the reference triangle (host), out [n_cells][npts] (host); 1 <= npts <= 64 */
int pgx_fr_conforming_damage(pgx_fr_handle* h, int32_t npts, const double* ref_pts, double* out);
int pgx_fr_lu_stats(const pgx_fr_handle* h, pgx_nd_stats* st);
/* 1 if the sparse LU honoured the symmetric request (pgx_nd_is_symmetric): L D L^T, half the flops; 0: general LU */
int pgx_fr_lu_is_symmetric(const pgx_fr_handle* h);

#ifdef __cplusplus
}
#endif
#endif
