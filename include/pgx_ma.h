/*
 * pgx_ma.h - C ABI of example 10 inside libpgx.so: the three-field mixed Monge-Ampere discretisation of the reference's
 * examples/10_monge_ampere/monge_ampere_dolfinx.py on the GPU, below `problem.solve()` (:151-154).
 *
 *   u in P_k, p in [P_{k+1}]^2, Psi = (Psi00, Psi01, Psi11) in [P_k]^3, all continuous on triangles (:51-55); Psi = log D^2 u is a
 *   symmetric-matrix latent variable and expm(Psi) the conforming map.  Unknowns x = [u | p0 | p1 | Psi00 | Psi01 | Psi11], rows
 *   [v | q0 | q1 | phi00 | phi01 | phi11].  Residual (:81-87):
 *       R_v = (Psi00 + Psi11 - ln rho, v),  R_q = (p - grad u, q),  R_phi = (grad p, phi) - (expm(Psi), phi),
 *   phi = [[phi00, phi01], [phi01, phi11]]: the off-diagonal test function sees (d_y p0 + d_x p1) - 2 E01.
 *
 *   pgx_ma_create          mesh (:12), spaces (:51-55), Dirichlet condition on the exterior dofs of u (:88-97), ln rho (:47, :82)
 *   pgx_ma_residual        SNES function: form F (:81-87) with DOLFINx's NonlinearProblem contract (:151) - lifting
 *                          F += J(x)[:, bc] (g - x_bc), F[bc] = x_bc - g; the state is not overwritten with g
 *   pgx_ma_jacobian_fill   SNES Jacobian: ufl.derivative(F, z) (:138), bc rows and columns set to the identity
 *   pgx_ma_newton_solve    problem.solve() (:154) with "snes_linesearch_type": "l2" and ksp preonly + pc lu + MUMPS (:15-23): the shared
 *                          SNES driver; the linear solve is the dense LU with partial pivoting of include/pgx_dn.h (the Jacobian is
 *                          not quasi-definite: the sparse LU of pgx_nd.h, which never pivots across nodes, cannot take it) plus
 *                          iterative refinement on the exact operator; reason = getConvergedReason (:156), its = getIterationNumber (:155)
 *   pgx_ma_l2_error        sqrt(assemble_scalar((u - u_exact)^2 dx)) (:161-163), a fixed-shape two-stage reduction
 *
 * expm of a symmetric 2 x 2 in closed form (the reference's expm.py:43-79; its third branch never occurs for symmetric input):
 * m = (a + d) / 2, h = (a - d) / 2, delta = sqrt(h^2 + b^2), E = e^m (cosh(delta) I + sinh(delta) / delta [[h, b], [b, -h]]), evaluated
 * from exp(m +- delta); series below delta = 1e-4.
 * Numbering and basis are the caller's (proximalgalerkin_amd.lagrange: equispaced lattice); tables are passed at the quadrature points.
 * Plain pointers and sizes only.  Returns 0 or a negative PGX_E* code (include/pgx.h); text via pgx_ma_last_error.
 */
#ifndef PGX_MA_H
#define PGX_MA_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_dn.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_ma_handle pgx_ma_handle;

typedef struct {
  int32_t nv, nc;             /* vertices, triangles */
  const double* coords;       /* [nv][2] */
  const int32_t* cells;       /* [nc][3] */
  int32_t degree;             /* k >= 2: a run-time parameter */
  int32_t nu, np;             /* dofs of the P_k and of the P_{k+1} space */
  const int32_t* cell_dofs_u; /* [nc][(k+1)(k+2)/2] */
  const int32_t* cell_dofs_p; /* [nc][(k+2)(k+3)/2] */
  int32_t nq;                 /* quadrature points on the reference triangle */
  const double* qwts;         /* [nq], summing to 1/2 */
  const double* tab_u;        /* [nk][nq]    P_k basis at the points */
  const double* dtab_u;       /* [2][nk][nq] its reference gradient */
  const double* tab_p;        /* [nk1][nq]   P_{k+1} */
  const double* dtab_p;       /* [2][nk1][nq] */
  const double* ln_rho;       /* [nc][nq] ln rho at the physical quadrature points (coordinate expressions stay outside the form) */
  int32_t n_bc;
  const int32_t* bc_dofs;     /* [n_bc] exterior dofs of u (:94-96) */
  const double* g;            /* [n_bc] Dirichlet values (:91-93) */
} pgx_ma_problem;

int pgx_ma_create(const pgx_ma_problem* p, int device, pgx_ma_handle** out);
void pgx_ma_destroy(pgx_ma_handle* h);
const char* pgx_ma_last_error(const pgx_ma_handle* h);
int pgx_ma_num_dofs(const pgx_ma_handle* h, int64_t* ntot); /* 4 nu + 2 np */
int pgx_ma_set_state(pgx_ma_handle* h, const double* x);
int pgx_ma_get_state(pgx_ma_handle* h, double* x);
/* F(x) (host arrays; x NULL: the state), fnorm may be NULL */
int pgx_ma_residual(pgx_ma_handle* h, const double* x, double* F, double* fnorm);
int pgx_ma_jacobian_fill(pgx_ma_handle* h, const double* x);
int pgx_ma_csr_export(pgx_ma_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_ma_spmv(pgx_ma_handle* h, const double* x, double* y);
/* linesearch 2: l2 (the script's), 1 / 3: bt of order 2 / 3, every other value: plain Newton */
int pgx_ma_newton_solve(pgx_ma_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
int pgx_ma_l2_error(pgx_ma_handle* h, const double* u_exact_at_qp /* [nc][nq] host */, double* out);
int pgx_ma_lu_stats(const pgx_ma_handle* h, pgx_dn_stats* st);
/* device-event ms: [0] residual [1] Jacobian fill [2] factorisation [3] solves [4] spmv [5] Newton total */
int pgx_ma_profile(pgx_ma_handle* h, int enable, double ms[6]);

#ifdef __cplusplus
}
#endif
#endif
