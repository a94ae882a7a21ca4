// pgx_dn.hip - dense LU with partial pivoting on the GPU (include/pgx_dn.h): the direct solver for Newton matrices that are not
// quasi-definite (example 10, Monge-Ampere), where the block elimination WITHOUT pivoting of pgx_nd.hip meets singular diagonal blocks.
//
// Storage: the n x n matrix dense and column-major (leading dimension n), L\U in place like dgetrf.  Blocked right-looking
// factorisation, panel width DN_NB = 64, all synchronisation at kernel boundaries (no workgroup waits for another inside a launch):
//
//   per column j of a panel [j0, j0 + w):
//     k_dn_pivot   ONE workgroup: second stage of the argmax over the per-chunk candidates (largest |a|, lowest row among equals - a
//                  total order, so the winner does not depend on the reduction's shape, and the shape is fixed anyway), piv[j] = p,
//                  rows j <-> p exchanged inside the panel; a column of exact zeros is counted and left alone
//     k_dn_update  a workgroup per 64 rows below the diagonal, its four waves dealing the panel's remaining columns: multipliers
//                  l = a / pivot, rank-1 update of the columns (j, j0 + w), and - wave 0, on the values it has just written - the
//                  first stage of the NEXT column's argmax (one candidate per 64 rows)
//   per panel:
//     k_dn_laswp   the panel's interchanges on the columns left and right of it (one thread per column)
//     k_dn_trsm    U12 = L11^{-1} A12, one thread per column, L11 in LDS (broadcast reads)
//     k_nd_gemm*   A22 -= L21 U12 on the fp64 matrix cores: the kernels of pgx_nd_gemm.h as they are (one "front" of order n whose
//                  working matrix and factor store are the same array)
//
// Two launches per column bound the panel phase: ~N x 2 small launches per factorisation.  At the sizes this solver is for
// (N <= 5 286 in example 10) that is the larger part of the factorisation time - DESIGN.md section 12e says what was measured and
// what a recursive panel would buy.
//
// Solve: x = U^{-1} L^{-1} P b panel by panel; per panel ONE launch in which wave 0 of every workgroup solves the 64 x 64 triangle
// (redundantly: lane = row, the solved entries travel by v_readlane) and all threads then update one row each of the remaining
// right-hand side.  The solved entries go to a SECOND vector, so no workgroup reads what another one writes in the same launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pgx.h"
#include "../../include/pgx_dn.h"
#include "pgx_nd_gemm.h"
#include "pgx_scope.h"

#define DN_NB PGX_DN_NB
#define DN_CH 64  // rows per first-stage argmax candidate = one wave
static_assert(DN_NB == 64 && DN_CH == 64, "one wavefront lane per panel column / chunk row");
#define DN_MAX_CH ((PGX_DN_MAX_N + DN_CH - 1) / DN_CH)  // 512 candidates at most: two per thread of k_dn_pivot

static thread_local std::string g_dn_error;

struct pgx_dn {
  int64_t n = 0, nnz = 0;
  int device = -1;
  hipStream_t st = nullptr;
  bool own_stream = false;
  double* A = nullptr;        // [n * n] column-major: the matrix, then L\U
  int64_t* d_dest = nullptr;  // [nnz] position of each CSR entry in A
  double* d_vals = nullptr;   // [nnz] staging for host values
  int32_t *d_piv = nullptr, *d_perm = nullptr, *d_info = nullptr, *d_ci = nullptr;
  double *d_cv = nullptr, *d_w0 = nullptr, *d_w1 = nullptr, *d_io = nullptr;
  std::vector<int32_t> piv, perm;
  std::vector<double> diag;
  pgx_dn_stats stats{};
  bool factored = false;
  bool timing = false;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double factor_ms = 0, solve_ms = 0;
  std::string err;
};

extern "C" const char* pgx_dn_last_error(const pgx_dn* s) { return s ? s->err.c_str() : g_dn_error.c_str(); }

#define DNHIP(call)                                               \
  do {                                                            \
    hipError_t e_ = (call);                                       \
    if (e_ != hipSuccess) {                                       \
      s->err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return PGX_EHIP;                                            \
    }                                                             \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dn_scatter(int64_t nnz, const int64_t* __restrict__ dest, const double* __restrict__ vals,
                                                    double* __restrict__ A) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) A[dest[i]] = vals[i];
}

// candidate (v, i) against the best so far: larger modulus wins, the lower row among equals.  Lanes without a row carry (-1, INT_MAX).
__device__ __forceinline__ void dn_best(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) bv = v, bi = i;
}
__device__ __forceinline__ void dn_wave_argmax(double& v, int& i) {  // butterfly: every lane ends with the wave's winner
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    dn_best(v, i, ov, oi);
  }
}

// first stage of the argmax of column c over rows [c, n) in chunks of DN_CH rows (the first column of a panel; the others get theirs
// from k_dn_update)
__global__ __launch_bounds__(DN_CH) void k_dn_colmax(const double* __restrict__ A, int64_t n, int64_t c, double* __restrict__ cv,
                                                     int32_t* __restrict__ ci) {
  const int64_t r = c + (int64_t)blockIdx.x * DN_CH + threadIdx.x;
  double v = r < n ? fabs(A[c * n + r]) : -1.0;
  int i = r < n ? (int)r : INT_MAX;
  dn_wave_argmax(v, i);
  if (threadIdx.x == 0) cv[blockIdx.x] = v, ci[blockIdx.x] = i;
}

// second stage for column j (nch <= DN_MAX_CH candidates), the pivot record and the interchange inside the panel [j0, j0 + w)
__global__ __launch_bounds__(256) void k_dn_pivot(double* __restrict__ A, int64_t n, int j0, int w, int j, int nch,
                                                  const double* __restrict__ cv, const int32_t* __restrict__ ci, int32_t* __restrict__ piv,
                                                  int32_t* __restrict__ info) {
  __shared__ double sv[4];
  __shared__ int si[4];
  const int t = threadIdx.x;
  double v = -1.0;
  int i = INT_MAX;
  for (int q = t; q < nch; q += 256) dn_best(v, i, cv[q], ci[q]);
  dn_wave_argmax(v, i);
  if ((t & 63) == 0) sv[t >> 6] = v, si[t >> 6] = i;
  __syncthreads();
  v = sv[0], i = si[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) dn_best(v, i, sv[q], si[q]);
  // a column of NaNs leaves (-1, INT_MAX): whatever the values, the row exchanged is one of [j, n)
  const int p = (i >= j && (int64_t)i < n) ? i : j;
  if (t == 0) {
    piv[j] = p;
    if (v == 0.0) info[0] += 1;  // every candidate exactly zero (launches of one stream: no concurrent writer)
  }
  if (p != j && t < w) {
    const int64_t c = (int64_t)(j0 + t) * n;
    const double a = A[c + j], b = A[c + p];
    A[c + j] = b, A[c + p] = a;
  }
}

// multipliers of column j and the rank-1 update of the columns (j, jend) on the rows below j: workgroup = 64 rows, wave wq takes the
// columns j + 1 + wq, + 4, ...  Wave 0 - owner of column j + 1 - leaves the first-stage argmax candidate of its 64 rows for the next
// k_dn_pivot.  A zero pivot (k_dn_pivot found nothing else) divides nothing and updates nothing.
__global__ __launch_bounds__(256) void k_dn_update(double* __restrict__ A, int64_t n, int jend, int j, double* __restrict__ cv,
                                                   int32_t* __restrict__ ci) {
  const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
  const int64_t r = (int64_t)j + 1 + (int64_t)blockIdx.x * 64 + lane;
  const bool valid = r < n;
  const int64_t cj = (int64_t)j * n;
  const double pv = A[cj + j];
  const bool zero = pv == 0.0;
  const double a = valid ? A[cj + r] : 0.0;
  const double l = zero ? 0.0 : a / pv;
  __syncthreads();  // every wave has read the column before wave 0 overwrites it
  if (wq == 0 && valid && !zero) A[cj + r] = l;
  double first = 0.0;
  for (int c = j + 1 + wq; c < jend; c += 4) {
    const int64_t cc = (int64_t)c * n;
    const double u = A[cc + j];
    double x = valid ? A[cc + r] : 0.0;
    if (valid && !zero) {
      x = fma(-l, u, x);
      A[cc + r] = x;
    }
    if (c == j + 1) first = x;
  }
  if (wq == 0 && j + 1 < jend) {
    double v = valid ? fabs(first) : -1.0;
    int i = valid ? (int)r : INT_MAX;
    dn_wave_argmax(v, i);
    if (lane == 0) cv[blockIdx.x] = v, ci[blockIdx.x] = i;
  }
}

// the interchanges of the panel [j0, j0 + w) on the columns [0, j0) and [j0 + w, n), one thread per column
__global__ __launch_bounds__(256) void k_dn_laswp(double* __restrict__ A, int64_t n, int j0, int w, const int32_t* __restrict__ piv) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = t < j0 ? t : t + w;
  if (c >= n) return;
  double* col = A + c * n;
  for (int k = j0; k < j0 + w; ++k) {
    const int p = piv[k];
    if (p != k) {
      const double a = col[k], b = col[p];
      col[k] = b, col[p] = a;
    }
  }
}

// U12 = L11^{-1} A12 for a FULL panel (w = 64: only the last panel is narrower, and it has no columns to its right): L11 in LDS,
// one thread per column of A12 with the column in registers
__global__ __launch_bounds__(64) void k_dn_trsm(double* __restrict__ A, int64_t n, int j0) {
  __shared__ double Ls[DN_NB][DN_NB + 1];
  const int lane = threadIdx.x;
  for (int k = 0; k < DN_NB; ++k) Ls[lane][k] = A[(int64_t)(j0 + k) * n + j0 + lane];
  __syncthreads();
  const int64_t c = (int64_t)j0 + DN_NB + (int64_t)blockIdx.x * 64 + lane;
  if (c >= n) return;
  double* col = A + c * n + j0;
  double u[DN_NB];
#pragma unroll
  for (int i = 0; i < DN_NB; ++i) u[i] = col[i];
#pragma unroll
  for (int i = 1; i < DN_NB; ++i) {
    double v = u[i];
#pragma unroll
    for (int m = 0; m < i; ++m) v = fma(-Ls[i][m], u[m], v);
    u[i] = v;
  }
#pragma unroll
  for (int i = 1; i < DN_NB; ++i) col[i] = u[i];
}

__global__ __launch_bounds__(256) void k_dn_diag(const double* __restrict__ A, int64_t n, double* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = A[i * n + i];
}

__global__ __launch_bounds__(256) void k_dn_permute(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ b,
                                                    double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = b[perm[i]];
}

// forward substitution, panel [j0, j0 + w): z[panel] = L11^{-1} y[panel] (unit diagonal), then y[r] -= L21[r, :] z[panel] for r >= j0 + w
__global__ __launch_bounds__(256) void k_dn_fwd(const double* __restrict__ A, int64_t n, int j0, int w, double* __restrict__ y,
                                                double* __restrict__ z) {
  __shared__ double zs[DN_NB];
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int i = tid;
    double yi = i < w ? y[j0 + i] : 0.0;
    double l[DN_NB];
#pragma unroll
    for (int k = 0; k < DN_NB; ++k) l[k] = (k < i && i < w) ? A[(int64_t)(j0 + k) * n + j0 + i] : 0.0;
#pragma unroll
    for (int k = 0; k < DN_NB; ++k) {
      if (k < w) {  // uniform
        const double zk = nd_bcast(yi, k);
        if (i > k && i < w) yi = fma(-l[k], zk, yi);
      }
    }
    zs[i] = yi;
    if (blockIdx.x == 0 && i < w) z[j0 + i] = yi;
  }
  __syncthreads();
  const int64_t r = (int64_t)j0 + w + (int64_t)blockIdx.x * 256 + tid;
  if (r >= n) return;
  double acc = y[r];
  for (int k = 0; k < w; ++k) acc = fma(-A[(int64_t)(j0 + k) * n + r], zs[k], acc);
  y[r] = acc;
}

// backward substitution, panel [j0, j0 + w): x[panel] = U11^{-1} z[panel], then z[r] -= U[r, panel] x[panel] for r < j0
__global__ __launch_bounds__(256) void k_dn_bwd(const double* __restrict__ A, int64_t n, int j0, int w, double* __restrict__ z,
                                                double* __restrict__ x) {
  __shared__ double xs[DN_NB];
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int i = tid;
    double yi = i < w ? z[j0 + i] : 0.0;
    double u[DN_NB];  // row i of U11 from the diagonal on; 1 elsewhere (nothing divides by an entry that is not a pivot)
#pragma unroll
    for (int k = 0; k < DN_NB; ++k) u[k] = (k >= i && k < w) ? A[(int64_t)(j0 + k) * n + j0 + i] : 1.0;
#pragma unroll
    for (int k = DN_NB - 1; k >= 0; --k) {
      if (k < w) {  // uniform
        const double xk = nd_bcast(yi / u[k], k);  // lane k: its diagonal entry
        if (i < k)
          yi = fma(-u[k], xk, yi);
        else if (i == k)
          yi = xk;
      }
    }
    xs[i] = yi;
    if (blockIdx.x == 0 && i < w) x[j0 + i] = yi;
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  if (r >= j0) return;
  double acc = z[r];
  for (int k = 0; k < w; ++k) acc = fma(-A[(int64_t)(j0 + k) * n + r], xs[k], acc);
  z[r] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_dn_destroy(pgx_dn* s) {
  if (!s) return;
  if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess) {
    if (s->st) hipStreamSynchronize(s->st);
    for (void* p : {(void*)s->A, (void*)s->d_dest, (void*)s->d_vals, (void*)s->d_piv, (void*)s->d_perm, (void*)s->d_info, (void*)s->d_ci,
                    (void*)s->d_cv, (void*)s->d_w0, (void*)s->d_w1, (void*)s->d_io})
      if (p) hipFree(p);
    if (s->e0) hipEventDestroy(s->e0);
    if (s->e1) hipEventDestroy(s->e1);
    if (s->own_stream && s->st) hipStreamDestroy(s->st);
  }
  delete s;
}

template <typename T>
static int dn_alloc(pgx_dn* s, T** d, size_t count, const char* what) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc((void**)d, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *d = nullptr;
    s->err = "pgx_dn_create: n = " + std::to_string(s->n) + ": cannot allocate " + std::to_string(bytes) + " bytes for " + what;
    return PGX_ENOMEM;
  }
  return PGX_OK;
}

extern "C" int pgx_dn_create(int64_t n, const int32_t* rowptr, const int32_t* col, int device, void* hip_stream, pgx_dn** out) {
  if (out) *out = nullptr;
  if (!out || !rowptr || n < 1 || device < 0) {
    g_dn_error = "pgx_dn_create: bad argument (n >= 1, a device, rowptr and out are required)";
    return PGX_EINVAL;
  }
  if (n > PGX_DN_MAX_N) {  // before anything is allocated
    g_dn_error = "pgx_dn_create: n = " + std::to_string(n) + " exceeds PGX_DN_MAX_N = " + std::to_string(PGX_DN_MAX_N) +
                 " (a dense fp64 matrix of that order needs " + std::to_string((double)n * (double)n * 8.0 / 1073741824.0) + " GiB)";
    return PGX_EINVAL;
  }
  const int64_t nnz = rowptr[n];
  bool ok = rowptr[0] == 0 && nnz >= 0 && (nnz == 0 || col);
  for (int64_t i = 0; ok && i < n; ++i) {
    ok = rowptr[i + 1] >= rowptr[i] && rowptr[i + 1] <= nnz;
    for (int64_t k = rowptr[i]; ok && k < rowptr[i + 1]; ++k)
      ok = col[k] >= 0 && col[k] < n && (k == rowptr[i] || col[k] > col[k - 1]);
  }
  if (!ok) {
    g_dn_error = "pgx_dn_create: malformed CSR pattern (rowptr monotone from 0, columns in [0, n) strictly increasing within a row)";
    return PGX_EINVAL;
  }
  pgx_dn* s = new pgx_dn;
  s->n = n, s->nnz = nnz, s->device = device;
  s->stats.n = n;
  auto fail = [&](int rc) {
    g_dn_error = s->err;
    pgx_dn_destroy(s);
    return rc;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    s->err = std::string("pgx_dn_create: hipSetDevice: ") + hipGetErrorString(e);
    s->device = -1;
    return fail(PGX_ENODEV);
  }
  if (hip_stream)
    s->st = (hipStream_t)hip_stream;
  else {
    if ((e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking)) != hipSuccess) {
      s->err = std::string("pgx_dn_create: hipStreamCreate: ") + hipGetErrorString(e);
      return fail(PGX_EHIP);
    }
    s->own_stream = true;
  }
  int rc;
  if ((rc = dn_alloc(s, &s->A, (size_t)n * (size_t)n, "the dense matrix")) || (rc = dn_alloc(s, &s->d_dest, (size_t)nnz, "the scatter map")) ||
      (rc = dn_alloc(s, &s->d_vals, (size_t)nnz, "the CSR values")) || (rc = dn_alloc(s, &s->d_piv, (size_t)n, "the pivot vector")) ||
      (rc = dn_alloc(s, &s->d_perm, (size_t)n, "the row permutation")) || (rc = dn_alloc(s, &s->d_info, 1, "the info word")) ||
      (rc = dn_alloc(s, &s->d_ci, DN_MAX_CH, "the pivot candidates")) || (rc = dn_alloc(s, &s->d_cv, DN_MAX_CH, "the pivot candidates")) ||
      (rc = dn_alloc(s, &s->d_w0, (size_t)n, "a work vector")) || (rc = dn_alloc(s, &s->d_w1, (size_t)n, "a work vector")) ||
      (rc = dn_alloc(s, &s->d_io, (size_t)n, "a work vector")))
    return fail(rc);
  std::vector<int64_t> dest((size_t)nnz);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) dest[(size_t)k] = (int64_t)col[k] * n + i;
  if (nnz && (e = hipMemcpy(s->d_dest, dest.data(), (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) {
    s->err = std::string("pgx_dn_create: hipMemcpy: ") + hipGetErrorString(e);
    return fail(PGX_EHIP);
  }
  if (hipEventCreate(&s->e0) != hipSuccess || hipEventCreate(&s->e1) != hipSuccess) {
    s->err = "pgx_dn_create: hipEventCreate failed";
    return fail(PGX_EHIP);
  }
  s->piv.assign((size_t)n, 0);
  s->perm.assign((size_t)n, 0);
  s->diag.assign((size_t)n, 0.0);
  *out = s;
  return PGX_OK;
}

extern "C" int pgx_dn_get_stats(const pgx_dn* s, pgx_dn_stats* st) {
  if (!s || !st) return PGX_EINVAL;
  *st = s->stats;
  return PGX_OK;
}

extern "C" int pgx_dn_export_pivots(const pgx_dn* s, int32_t* piv) {
  if (!s || !piv) return PGX_EINVAL;
  std::memcpy(piv, s->piv.data(), (size_t)s->n * sizeof(int32_t));
  return PGX_OK;
}

extern "C" int pgx_dn_timing(pgx_dn* s, int enable, double* factor_ms, double* solve_ms) {
  if (!s) return PGX_EINVAL;
  if (factor_ms) *factor_ms = s->factor_ms;
  if (solve_ms) *solve_ms = s->solve_ms;
  s->timing = enable != 0;
  s->factor_ms = s->solve_ms = 0;
  return PGX_OK;
}

// A22 -= L21 U12 behind the panel [j0, j0 + 64): the Schur-update kernels of pgx_nd_gemm.h on ONE front of order n whose working
// matrix and factor store are both A (offsets 0, P = M = n: every column is addressed column-major with leading dimension n).
// The 64 x 64-tile kernel throughout: the eight-wave 128 x 128 one is reported with 12 bytes of scratch per lane by this compiler,
// and the update is not what bounds this factorisation (see the head of this file).
static void dn_launch_gemm(pgx_dn* s, int j0) {
  const int n = (int)s->n, o = j0 + DN_NB, m = n - o;
  if (m <= 0) return;
  const unsigned nt = (unsigned)((m + 63) / 64);  // <= 511
  const NdGatherCtx gc{};
  hipLaunchKernelGGL((k_nd_gemm<2, false>), dim3(1, nt, nt), dim3(256), 0, s->st, s->A, (int64_t)0, n, o, n, o, n, j0, o, (int64_t)0, n, gc,
                     -1, 0, 0);
}

extern "C" int pgx_dn_factor(pgx_dn* s, const double* vals, int on_device) {
  if (!s || (!vals && s->nnz)) return PGX_EINVAL;
  DNHIP(hipSetDevice(s->device));
  PgxRange range("pgx_dn:factor");
  s->factored = false;
  const int64_t n = s->n;
  const double* dv = vals;
  if (!on_device && s->nnz) {
    DNHIP(hipMemcpyAsync(s->d_vals, vals, (size_t)s->nnz * sizeof(double), hipMemcpyHostToDevice, s->st));
    dv = s->d_vals;
  }
  if (s->timing) hipEventRecord(s->e0, s->st);
  DNHIP(hipMemsetAsync(s->d_info, 0, sizeof(int32_t), s->st));
  DNHIP(hipMemsetAsync(s->A, 0, (size_t)n * (size_t)n * sizeof(double), s->st));
  if (s->nnz) {
    const int blocks = (int)std::min<int64_t>((s->nnz + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(k_dn_scatter, dim3(blocks), dim3(256), 0, s->st, s->nnz, s->d_dest, dv, s->A);
  }
  for (int j0 = 0; j0 < (int)n; j0 += DN_NB) {
    const int w = std::min<int>(DN_NB, (int)n - j0), jend = j0 + w;
    hipLaunchKernelGGL(k_dn_colmax, dim3((unsigned)((n - j0 + DN_CH - 1) / DN_CH)), dim3(DN_CH), 0, s->st, s->A, n, (int64_t)j0, s->d_cv, s->d_ci);
    for (int j = j0; j < jend; ++j) {
      const int nch = (int)((n - j + DN_CH - 1) / DN_CH);
      hipLaunchKernelGGL(k_dn_pivot, dim3(1), dim3(256), 0, s->st, s->A, n, j0, w, j, nch, s->d_cv, s->d_ci, s->d_piv, s->d_info);
      const int64_t below = n - j - 1;
      if (below > 0)
        hipLaunchKernelGGL(k_dn_update, dim3((unsigned)((below + 63) / 64)), dim3(256), 0, s->st, s->A, n, jend, j, s->d_cv, s->d_ci);
    }
    if (n > w) hipLaunchKernelGGL(k_dn_laswp, dim3((unsigned)((n - w + 255) / 256)), dim3(256), 0, s->st, s->A, n, j0, w, s->d_piv);
    if (jend < (int)n) {  // (then w == DN_NB)
      hipLaunchKernelGGL(k_dn_trsm, dim3((unsigned)((n - jend + 63) / 64)), dim3(64), 0, s->st, s->A, n, j0);
      dn_launch_gemm(s, j0);
    }
  }
  hipLaunchKernelGGL(k_dn_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, s->A, n, s->d_w0);
  if (s->timing) hipEventRecord(s->e1, s->st);
  DNHIP(hipGetLastError());
  int32_t info = 0;
  DNHIP(hipMemcpyAsync(s->piv.data(), s->d_piv, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->st));
  DNHIP(hipMemcpyAsync(s->diag.data(), s->d_w0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->st));
  DNHIP(hipMemcpyAsync(&info, s->d_info, sizeof(int32_t), hipMemcpyDeviceToHost, s->st));
  DNHIP(hipStreamSynchronize(s->st));
  if (s->timing) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) s->factor_ms += ms;
  }
  // statistics, and the interchanges composed into ONE gather for the solves: perm[i] = the row of b that ends in position i
  s->stats.interchanges = 0;
  s->stats.zero_pivots = info;
  double lo = INFINITY, hi = 0.0;
  for (int64_t i = 0; i < n; ++i) s->perm[(size_t)i] = (int32_t)i;
  for (int64_t k = 0; k < n; ++k) {
    const int32_t p = s->piv[(size_t)k];
    if (p < k || p >= n) {
      s->err = "pgx_dn_factor: pivot vector out of range (internal error)";
      return PGX_ESTATE;
    }
    if (p != k) std::swap(s->perm[(size_t)k], s->perm[(size_t)p]), ++s->stats.interchanges;
    const double d = std::fabs(s->diag[(size_t)k]);
    lo = std::min(lo, d), hi = std::max(hi, d);
  }
  s->stats.min_pivot = lo, s->stats.max_pivot = hi;
  if (info > 0) {
    s->err = "pgx_dn_factor: " + std::to_string(info) + " column(s) of order-" + std::to_string(n) +
             " matrix without a nonzero pivot candidate: the matrix is singular; pgx_dn_solve refuses this factorisation";
    return PGX_ESTATE;
  }
  DNHIP(hipMemcpyAsync(s->d_perm, s->perm.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s->st));
  DNHIP(hipStreamSynchronize(s->st));
  s->factored = true;
  s->err.clear();
  return PGX_OK;
}

extern "C" int pgx_dn_solve(pgx_dn* s, const double* b, double* x, int on_device) {
  if (!s || !b || !x) return PGX_EINVAL;
  if (!s->factored) {
    s->err = s->stats.zero_pivots > 0 ? "pgx_dn_solve: the last factorisation met " + std::to_string(s->stats.zero_pivots) +
                                            " zero pivot(s) (singular matrix); factorise a nonsingular matrix first"
                                      : std::string("pgx_dn_solve: no factorisation (call pgx_dn_factor first)");
    return PGX_ESTATE;
  }
  DNHIP(hipSetDevice(s->device));
  PgxRange range("pgx_dn:solve");
  const int64_t n = s->n;
  const double* db = b;
  double* dx = x;
  if (!on_device) {
    DNHIP(hipMemcpyAsync(s->d_io, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s->st));
    db = dx = s->d_io;
  }
  if (s->timing) hipEventRecord(s->e0, s->st);
  hipLaunchKernelGGL(k_dn_permute, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, n, s->d_perm, db, s->d_w0);
  for (int j0 = 0; j0 < (int)n; j0 += DN_NB) {
    const int w = std::min<int>(DN_NB, (int)n - j0);
    const int64_t below = n - j0 - w;
    hipLaunchKernelGGL(k_dn_fwd, dim3((unsigned)std::max<int64_t>(1, (below + 255) / 256)), dim3(256), 0, s->st, s->A, n, j0, w, s->d_w0, s->d_w1);
  }
  for (int j0 = (int)((n - 1) / DN_NB) * DN_NB; j0 >= 0; j0 -= DN_NB) {
    const int w = std::min<int>(DN_NB, (int)n - j0);
    hipLaunchKernelGGL(k_dn_bwd, dim3((unsigned)std::max(1, (j0 + 255) / 256)), dim3(256), 0, s->st, s->A, n, j0, w, s->d_w1, dx);
  }
  if (s->timing) hipEventRecord(s->e1, s->st);
  DNHIP(hipGetLastError());
  if (!on_device) {
    DNHIP(hipMemcpyAsync(x, s->d_io, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    DNHIP(hipStreamSynchronize(s->st));
  }
  if (s->timing) {
    float ms = 0;
    if (hipEventSynchronize(s->e1) == hipSuccess && hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) s->solve_ms += ms;
  }
  return PGX_OK;
}
