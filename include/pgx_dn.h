/*
 * pgx_dn.h - C ABI of the dense direct solver inside libpgx.so: blocked right-looking LU with PARTIAL PIVOTING on the GPU.
 *
 * Replaces, for Newton matrices that need row interchanges, what the reference requests from PETSc with
 *     "ksp_type": "preonly", "pc_type": "lu", "pc_factor_mat_solver_type": "mumps"
 * (examples/10_monge_ampere/monge_ampere_dolfinx.py:15-23).  The sparse solver of include/pgx_nd.h eliminates node blocks without
 * pivoting, which is sound for the quasi-definite saddle-point matrices of examples 01-08 and for nothing else; the mixed
 * Monge-Ampere Jacobian (a zero (v, u) block, u entering only through -(grad du, q)) is unsymmetric and not quasi-definite in any
 * ordering.  Its systems are small and block-dense (N = 5 286 with 16 % structural nonzeros at the script's last degree), so the
 * matrix is stored DENSE, column-major, and factorised as P A = L U like LAPACK's dgetrf:
 *
 *   pgx_dn_create   the CSR pattern, once: checks it, allocates the n x n array
 *   pgx_dn_factor   MatLUFactorNumeric: zero fill, scatter of the CSR values, P A = L U
 *   pgx_dn_solve    MatSolve: blocked forward and backward substitution for one right-hand side
 *
 * The pivot of a column is its entry of largest modulus on or below the diagonal, the LOWEST row index among equals (LAPACK's
 * idamax), found by a fixed-shape reduction: the factorisation is bitwise reproducible.
 * Plain pointers and sizes only.  Returns 0 or a negative PGX_E* code (include/pgx.h); text via pgx_dn_last_error.
 */
#ifndef PGX_DN_H
#define PGX_DN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_dn pgx_dn;

#define PGX_DN_MAX_N 32768 /* 8 GiB of fp64 storage */
#define PGX_DN_NB 64       /* panel width */

typedef struct {
  int64_t n;            /* matrix order */
  int64_t interchanges; /* rows k of the last factorisation with piv[k] != k */
  double min_pivot;     /* smallest and largest |U(k, k)| of the last factorisation (0 / 0 before the first) */
  double max_pivot;
  int64_t zero_pivots;  /* columns whose pivot candidates were all exactly zero: > 0 means pgx_dn_factor failed */
} pgx_dn_stats;

/* rowptr [n+1], col [nnz]: host arrays, column indices strictly increasing within each row (PGX_EINVAL otherwise).  n > PGX_DN_MAX_N
 * is refused with PGX_EINVAL before anything is allocated; an allocation failure gives PGX_ENOMEM.  Both messages name the size
 * (pgx_dn_last_error(NULL)).  hip_stream may be NULL: own stream. */
int pgx_dn_create(int64_t n, const int32_t* rowptr, const int32_t* col, int device, void* hip_stream, pgx_dn** out);
void pgx_dn_destroy(pgx_dn* s);
const char* pgx_dn_last_error(const pgx_dn* s);
int pgx_dn_get_stats(const pgx_dn* s, pgx_dn_stats* st);

/* Numeric factorisation of the matrix whose CSR values (pattern of create) are DEVICE-resident (on_device != 0) or on the host.
 * Returns when the factorisation has finished (the pivot vector and the diagonal are read back for the statistics).
 * A column whose pivot candidates are all exactly zero is skipped - nothing is divided -, the remaining columns are still
 * eliminated as dgetrf does, and the call returns PGX_ESTATE with zero_pivots > 0; pgx_dn_solve then refuses with PGX_ESTATE until
 * a factorisation has succeeded. */
int pgx_dn_factor(pgx_dn* s, const double* vals, int on_device);
/* x = A^{-1} b; b, x device pointers (on_device != 0) or host; b == x allowed.  Asynchronous on the solver's stream when on_device. */
int pgx_dn_solve(pgx_dn* s, const double* b, double* x, int on_device);
/* The pivot vector of the last factorisation, 0-based and LAPACK-style: row k was interchanged with row piv[k] >= k. */
int pgx_dn_export_pivots(const pgx_dn* s, int32_t* piv /* [n] host */);
/* accumulated device time of the factor / solve calls since the last call in ms (HIP events; 0 until pgx_dn_timing(s, 1, ...)) */
int pgx_dn_timing(pgx_dn* s, int enable, double* factor_ms, double* solve_ms);

#ifdef __cplusplus
}
#endif
#endif
