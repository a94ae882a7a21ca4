/*
 * pgx_ev.h - C ABI of libpgx.so for example 07 (2-D Landau-de Gennes Q-tensor whose eigenvalues are kept inside an interval through
 * a tensor-valued latent variable): everything below `problem.solve()` in the reference's
 * examples/07_eigenvalue_constraints/eigenvalue_constraints_dolfinx.py, i.e. DOLFINx assembly with inhomogeneous Dirichlet data +
 * PETSc SNES newtonls with the l2 line search + LU (:143, :158-160, :172-177), plus the vector copies and the norm of its outer loop
 * (:162-227) and the nodal post-processing (:245-259), kept on the device.
 *
 * Mixed [Q_p]^4 on a uniform grid of nx x ny rectangles (:41-50; the script: p = 3, 100 x 100); x = [q1 | q2 | psi1 | psi2], n =
 * (p nx + 1)(p ny + 1) entries each, the dofs being the points of the p-times refined vertex lattice, row by row (x fastest), the basis
 * the tensor product of the 1-D Lagrange bases on the equispaced nodes i / p (lagrange.numbering_quad).  Q = [[q1, q2], [q2, -q1]],
 * Psi likewise (:53-54); every inner product of two such tensors carries a factor 2.  Rows [w1 | w2 | phi1 | phi2].  With
 * s = q1^2 + q2^2, tr(Q Q) = 2 s and E = int |grad q1|^2 + |grad q2|^2 + A s + C s^2 (:71-75; B does not enter in 2-D), the residual
 * is (:78-84), i = 1, 2,
 *     R_wi   = alpha [ 2 (grad q_i, grad w_i) + ((2 A + 4 C s) q_i, w_i) ] + 2 (psi_i - psi_iter_i, w_i)
 *     R_phii = 2 (q_i, phi_i) - 2 (g(r) psi_i, phi_i),   r = sqrt(psi1^2 + psi2^2),  g(r) = tanh(r / 2) / r.
 * The last term is the script's 0.5 * tanh(Psi / 2) with the script's OWN tanh (:31-33), which is TWICE the matrix hyperbolic
 * tangent: 0.5 * tanh(Psi / 2) = T(psi) = g(r) Psi, g(0) = 1/2, eigenvalues in (-1, 1) - not the bound 1/2 of the paper.  g and
 * g'(r) / r are evaluated from e = exp(-r) <= 1 (finite for every finite r, where the script's expm overflows) and from the series
 * 1/2 - r^2 / 24 and -1/12 + r^2 / 60 below r = 1e-4.  psi_iter is the psi block of the previous LVPP iterate z_iter (set_prev /
 * advance_prev, :62-65, :225).  Jacobian: the true derivative, symmetric as assembled,
 *     [[alpha E''(q), 2 M (x) I2], [2 M (x) I2, -2 D(psi)]],
 * E''_ij = 2 K delta_ij + the mass form weighted by (2 A + 4 C s) delta_ij + 8 C q_i q_j, D_ij = the mass form weighted by
 * g delta_ij + (g' / r) psi_i psi_j.  Every term is integrated with the caller's 1-D Gauss rule in tensor form (:70: degree 20, 11
 * points per direction).
 *
 * Dirichlet data (:86-141): q1 and q2 are prescribed on the caller's boundary dofs.  DOLFINx's contract for NonlinearProblem:
 * F <- F_raw(x) + J(x)[:, bc] (g - x_bc), then F[bc] = x_bc - g; the rows and columns of the bc dofs of the Jacobian are zeroed,
 * diagonal 1.  The state is not overwritten with g: the first Newton step does that.
 *
 *   pgx_ev_create            NonlinearProblem(F, u=z, bcs=bcs, petsc_options=sp) construction (:158-160, :172-174)
 *   pgx_ev_set/get_state, set/get_prev, advance_prev   z.x.array, z_iter; z_iter.interpolate(z) (:225)
 *   pgx_ev_state_from_prev   z.interpolate(z_iter) (:195)
 *   pgx_ev_set_alpha         alpha.value = ... (:191, :219-222)
 *   pgx_ev_residual / pgx_ev_jacobian_fill / pgx_ev_csr_export / pgx_ev_spmv   SNES callbacks and the PETSc Mat
 *   pgx_ev_newton_solve      problem.solve() (:175): opts->linesearch 2 = l2 (:143), 1 / 3 = bt, 0 = full step
 *   pgx_ev_l2_increment_q    sqrt(assemble_scalar(inner(Q - Q_iter, Q - Q_iter) dx)) (:157, :209), the factor 2 included
 *   pgx_ev_eval_nodes        per dof: 0.5 * tanh(Psi / 2) (2 values, :245-246) and the largest / smallest eigenvalue of Q, +- sqrt(q1^2 +
 *                            q2^2), the closed form of the numpy.linalg.eigvals loop (:251-259)
 *   pgx_ev_lu_stats          pgx_nd_stats of the handle's sparse LU (perturbed_pivots: of the last completed factorisation)
 *   pgx_ev_lu_is_symmetric   whether that LU runs its symmetric L D L^T mode (the request is ignored where its kernels do not apply)
 * Conventions as in pgx.h.  Linear solves: sparse LU of pgx_nd.h (node = dof, 4 unknowns) in its symmetric L D L^T mode, no row
 * flip, + iterative refinement.  No CPU fallback.
 */
#ifndef PGX_EV_H
#define PGX_EV_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_nd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_ev_handle pgx_ev_handle;

typedef struct {
  int32_t nx, ny;        /* rectangles per direction */
  double x0, y0, x1, y1; /* the box (:42-44: the unit square) */
  int32_t degree;        /* p in {1, 2, 3} (:46) */
  int32_t nq;            /* points of the 1-D Gauss rule (<= 11; :70 degree 20 -> 11) */
  const double* qpts;    /* [nq] on [0, 1] */
  const double* qwts;    /* [nq], sum 1 */
  double A, C;           /* :67, :69 */
  int32_t n_bc;
  const int32_t* bc_dofs; /* [n_bc] lattice dofs carrying Dirichlet data, the same for q1 and q2 (:132, :137) */
  const double* g1;       /* [n_bc] values of q1 (:115-117, :130) */
  const double* g2;       /* [n_bc] values of q2 (:120-122, :139) */
} pgx_ev_problem;

int pgx_ev_create(const pgx_ev_problem* prob, int device, pgx_ev_handle** out);
void pgx_ev_destroy(pgx_ev_handle* h);
const char* pgx_ev_last_error(const pgx_ev_handle* h);
int pgx_ev_num_dofs(const pgx_ev_handle* h, int64_t* ntot);
int pgx_ev_set_state(pgx_ev_handle* h, const double* x);
int pgx_ev_get_state(pgx_ev_handle* h, double* x);
int pgx_ev_set_prev(pgx_ev_handle* h, const double* x);
int pgx_ev_get_prev(pgx_ev_handle* h, double* x);
int pgx_ev_advance_prev(pgx_ev_handle* h);
int pgx_ev_state_from_prev(pgx_ev_handle* h);
int pgx_ev_set_alpha(pgx_ev_handle* h, double alpha);
int pgx_ev_residual(pgx_ev_handle* h, const double* x, double* F, double* fnorm);
int pgx_ev_jacobian_fill(pgx_ev_handle* h, const double* x);
int pgx_ev_csr_export(pgx_ev_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_ev_spmv(pgx_ev_handle* h, const double* x, double* y);
int pgx_ev_newton_solve(pgx_ev_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
int pgx_ev_profile(pgx_ev_handle* h, int enable, double ms[6]);
/* the C names of this library are lower case throughout: the norm of the increment of Q */
int pgx_ev_l2_increment_q(pgx_ev_handle* h, double* out);
/* out [4][n] (host): T1, T2 of the conforming approximation, the largest and the smallest eigenvalue of Q, per lattice dof */
int pgx_ev_eval_nodes(pgx_ev_handle* h, double* out);
int pgx_ev_lu_stats(const pgx_ev_handle* h, pgx_nd_stats* st);
/* 1 if the sparse LU honoured the symmetric request (pgx_nd_is_symmetric): L D L^T, half the flops; 0: general LU */
int pgx_ev_lu_is_symmetric(const pgx_ev_handle* h);

#ifdef __cplusplus
}
#endif
#endif
