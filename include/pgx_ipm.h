/*
 * pgx_ipm.h - C ABI of the primal-dual interior-point solver inside libpgx.so: Mehrotra's predictor-corrector method for
 *
 *     minimise 1/2 x^T H x - b^T x   subject to   lo <= x <= up
 *
 * with the whole iteration on the GPU.  Stands where the reference calls IPOPT through cyipopt with
 *     "hessian_approximation": "exact", "hessian_constant": "yes", m = 0 (no general constraints)
 * (src/lvpp/optimization.py:115-166; used by examples/01_obstacle_problem/compare_all.py and obstacle_ipopt_galahad.py).
 *
 * H is symmetric and positive definite on the free dofs; entries of lo may be -inf, entries of up +inf; lo[i] == up[i] FIXES dof i.
 * With L / U the non-fixed dofs that have a finite lower / upper bound, s = x - lo on L, t = up - x on U and multipliers z (on L),
 * w (on U), one iteration is
 *     r_d = H x - b - z + w (0 on fixed dofs),  mu = (sum_L s z + sum_U t w) / (|L| + |U|),  stop when max(|r_d|_inf, mu) <= tol scale
 *     K = P_F (H + diag(z/s + w/t)) P_F + P_fixed, factorised ONCE (L D L^T mode of include/pgx_nd.h) for the two solves
 *     K dx = -r_d + c_z/s - c_w/t,  dz = (c_z - z dx)/s,  dw = (c_w + w dx)/t
 *     predictor: c_z = -s z, c_w = -t w;  sigma = (mu_aff/mu)^3;  corrector: c_z = sigma mu - s z - dx_aff dz_aff, c_w = sigma mu - t w + dx_aff dw_aff
 *     one step length alpha = min(1, max(0.995, 1 - mu) min(alpha_p, alpha_d)) for x, z and w
 * with scale = max(1, |H x_0 - b|_inf over the non-fixed dofs).  tests/interior_point_reference.py is the same algorithm in numpy.
 * Per iteration four small records of scalars travel to the host (stop test, two pairs of step lengths, mu_aff); every vector stays
 * on the device.  All reductions are two-stage and atomic-free in a fixed order: a solve is bitwise repeatable.
 * Plain pointers and sizes only, host arrays unless said otherwise.  Returns 0 or a negative PGX_E* code (include/pgx.h); text via
 * pgx_ipm_last_error.  The library reads no tuning for this solver, from the environment or otherwise.
 */
#ifndef PGX_IPM_H
#define PGX_IPM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_ipm pgx_ipm;

#define PGX_IPM_HISTORY_COLS 6 /* |r_d|_inf, mu, max complementarity, sigma, alpha_p, alpha_d */
#define PGX_IPM_PROFILE_COLS 5 /* ms: residual + reductions, KKT fill, factorisation, solves, step kernels */

/* The problem matrix of the reference's `hessian_constant yes` (optimization.py:115-166: exact, constant Hessian).
 * n_rows x n_cols CSR pattern of the FULL symmetric H (both triangles), column indices strictly increasing within a row, every
 * diagonal entry present; vals [nvals] with nvals == rowptr[n_rows]; coords [n_rows][dim], dim 2 or 3: one point per dof for the
 * nested dissection.  PGX_EINVAL with a message (pgx_ipm_last_error(NULL)) for a non-square or malformed pattern, a missing diagonal
 * entry or a value array of the wrong length - all checked on the host before the device is touched.  Builds the pgx_nd factorisation
 * object of the pattern in symmetric mode and keeps H, the diagonal positions and all iterate vectors on the device. */
int pgx_ipm_create(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col, const double* vals, int64_t nvals,
                   int32_t dim, const double* coords, int device, pgx_ipm** out);
void pgx_ipm_destroy(pgx_ipm* h);
const char* pgx_ipm_last_error(const pgx_ipm* h);

/* b, lo, up [n] (the bounds handed to cyipopt.Problem(lb=, ub=), optimization.py:154-160).  PGX_EINVAL when lo[i] > up[i] somewhere
 * or a bound is NaN (the message names the first such dof); nothing reaches the device then. */
int pgx_ipm_set_problem(pgx_ipm* h, const double* b, const double* lo, const double* up);

/* nlp.solve(x_init) of optimization.py:165 with options tol and max_iter (:141-146).  x, z, w [n] receive the last iterate;
 * *status = 0 converged, 1 max_iter reached (both return PGX_OK).  monitor != 0 prints one line per iteration.  A factorisation that
 * had to perturb pivots (K not positive definite to working precision) ends the solve with PGX_ESTATE and a message. */
int pgx_ipm_solve(pgx_ipm* h, const double* x_init, double tol, int32_t max_iter, int32_t monitor, double* x, double* z, double* w,
                  int32_t* iterations, int32_t* status);
/* Per-iteration record of the last solve (what IPOPT prints at print_level 5, optimization.py:141-143): one row of
 * PGX_IPM_HISTORY_COLS per evaluation of the stop test, iterations + 1 rows; the last row, which no step follows, has zeros in its
 * last three columns.  rows == NULL: only *n_rows. */
int pgx_ipm_history(const pgx_ipm* h, int64_t* n_rows, double* rows);
/* Device time of the solves since the last call, ms[PGX_IPM_PROFILE_COLS] (HIP events; zeros until enabled), then enable / disable
 * the recording.  Diagnostic for the IPOPT slot of optimization.py:115-166; ms may be NULL. */
int pgx_ipm_profile(pgx_ipm* h, int enable, double* ms);

/* Probes for tests of the kernels behind optimization.py:115-166's slot, no solve involved (they overwrite the handle's iterate):
 * r_d [n] and scalars[3] = (|r_d|_inf, mu, max complementarity) at (x, z, w) ... */
int pgx_ipm_eval(pgx_ipm* h, const double* x, const double* z, const double* w, double* rd_out, double* scalars_out);
/* ... and the values [nvals] of K at (x, z, w) as the factorisation receives them (pattern of create). */
int pgx_ipm_kkt_export(pgx_ipm* h, const double* x, const double* z, const double* w, double* vals_out);

#ifdef __cplusplus
}
#endif
#endif
