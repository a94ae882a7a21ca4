/*
 * pgx_bd.h - C ABI of the banded direct solver inside libpgx.so: LU with PARTIAL PIVOTING of a band matrix on the GPU, LAPACK's
 * dgbtrf / dgbtrs.
 *
 * For Newton matrices that need row interchanges (so not include/pgx_nd.h) and are far too sparse for the dense array of
 * include/pgx_dn.h, on quasi-one-dimensional domains: the eikonal equation on the Moebius strip (include/pgx_ek.h), whose matrix
 * [[0, B], [B^T, D(psi)]] has a band of 38 nv + 22 in the folded order of proximalgalerkin_amd.lagrange.band_order_mobius.
 *
 *   pgx_bd_create   the CSR pattern and a symmetric permutation, once: kl and ku of the permuted pattern, the band array
 *                   (LAPACK's layout: entry (i, j) at ab[j * ldab + kl + ku + i - j], ldab = 2 kl + ku + 1), the scatter map
 *   pgx_bd_factor   zero fill, scatter of the CSR values, P A = L U
 *   pgx_bd_solve    permutation, forward sweep with the interchanges interleaved, backward sweep, permutation back
 *
 * The pivot rule is dgbtf2's: in column j the diagonal and the min(kl, n - 1 - j) rows below it are the candidates, the largest
 * modulus wins, the LOWEST row among equals, found by a fixed-shape reduction.  The multipliers stay where they were computed (they
 * are not interchanged afterwards), U fills to kl + ku superdiagonals.  No atomics: two factorisations are bitwise equal.
 * Plain pointers and sizes only.  Returns 0 or a negative PGX_E* code (include/pgx.h); text via pgx_bd_last_error.
 */
#ifndef PGX_BD_H
#define PGX_BD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_bd pgx_bd;

#define PGX_BD_MAX_BYTES 8589934592LL /* 8 GiB of band storage, the dense solver's limit */
#define PGX_BD_MAX_KL 960             /* a panel is kl + PGX_BD_NB rows tall and has one thread per row: 960 + 32 <= 1024 */
#define PGX_BD_NB 32                  /* panel width */

typedef struct {
  int64_t n;            /* matrix order */
  int64_t kl, ku;       /* sub- and superdiagonals of the permuted pattern */
  int64_t bytes;        /* band storage: (2 kl + ku + 1) n doubles */
  int64_t interchanges; /* columns j of the last factorisation with piv[j] != j */
  double min_pivot;     /* smallest and largest |U(j, j)| of the last factorisation (0 / 0 before the first) */
  double max_pivot;
  int64_t zero_pivots;  /* columns whose pivot candidates were all exactly zero: > 0 means pgx_bd_factor failed */
} pgx_bd_stats;

/* rowptr [n+1], col [nnz]: host arrays, column indices strictly increasing within each row.  perm [n]: perm[new] = old, applied to
 * rows and columns alike, or NULL for the identity.  A malformed pattern or a perm that is no permutation gives PGX_EINVAL.
 * More than PGX_BD_MAX_BYTES of band storage and kl > PGX_BD_MAX_KL are refused with PGX_EINVAL before anything is allocated, the
 * message naming n, kl and ku (pgx_bd_last_error(NULL)); an allocation failure gives PGX_ENOMEM.  hip_stream may be NULL: own stream. */
int pgx_bd_create(int64_t n, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int device, void* hip_stream, pgx_bd** out);
void pgx_bd_destroy(pgx_bd* s);
const char* pgx_bd_last_error(const pgx_bd* s);
int pgx_bd_get_stats(const pgx_bd* s, pgx_bd_stats* st);

/* Numeric factorisation of the matrix whose CSR values (pattern of create, UNpermuted) are DEVICE-resident (on_device != 0) or on
 * the host.  Returns when the factorisation has finished (the pivot vector and the diagonal are read back for the statistics; there
 * is no other host synchronisation).  A column whose pivot candidates are all exactly zero is skipped - nothing is divided -, the
 * remaining columns are still eliminated, and the call returns PGX_ESTATE with zero_pivots > 0; pgx_bd_solve then refuses with
 * PGX_ESTATE until a factorisation has succeeded. */
int pgx_bd_factor(pgx_bd* s, const double* vals, int on_device);
/* x = A^{-1} b in the caller's (unpermuted) numbering; b, x device pointers (on_device != 0) or host; b == x allowed.
 * Asynchronous on the solver's stream when on_device. */
int pgx_bd_solve(pgx_bd* s, const double* b, double* x, int on_device);
/* The pivot vector of the last factorisation in the permuted numbering, 0-based: row j was interchanged with row
 * piv[j] in [j, j + kl] (LAPACK's ipiv minus one). */
int pgx_bd_export_pivots(const pgx_bd* s, int32_t* piv /* [n] host */);
/* accumulated device time of the factor / solve calls since the last call in ms (HIP events; 0 until pgx_bd_timing(s, 1, ...)) */
int pgx_bd_timing(pgx_bd* s, int enable, double* factor_ms, double* solve_ms);

#ifdef __cplusplus
}
#endif
#endif
