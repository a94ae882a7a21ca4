// pgx_ipm.hip - primal-dual interior-point method (Mehrotra predictor-corrector) for  min 1/2 x^T H x - b^T x,  lo <= x <= up,  with
// the whole iteration on the GPU (include/pgx_ipm.h; the slot of the reference's IPOPT call, src/lvpp/optimization.py:115-166).
// tests/interior_point_reference.py is the same algorithm in numpy, formula by formula.
//
// Per iteration (all launches on one stream, vectors of n doubles, H and K on the CSR pattern given at create):
//
//   k_ipm_residual  r_d = H x - b - z + w (0 on fixed dofs): one thread per row of the CSR SpMV, and in the same pass the block
//                   partials of |r_d|_inf, sum_L s z, sum_U t w and the largest complementarity product
//   k_ipm_kkt       one thread per stored entry: K = H + diag(z/s + w/t), rows AND columns of fixed dofs replaced by the identity,
//                   written into the array pgx_nd_factor(..., on_device = 1) reads
//   pgx_nd_factor   once; pgx_nd_solve twice (predictor, corrector), both on device pointers
//   k_ipm_rhs       -r_d + c_z/s - c_w/t for the complementarity targets of the predictor or the corrector
//   k_ipm_recover   dz, dw from dx, and the block partials of the four fraction-to-boundary minima (s, t, z, w)
//   k_ipm_muaff     block partials of the complementarity sums at the affine step
//   k_ipm_update    x, z, w += alpha (dx, dz, dw), x kept off the bounds where lo + s rounds to lo
//   k_ipm_final     second stage of every reduction: ONE workgroup folds the block partials
//
// Reductions: a thread folds its grid-stride elements in increasing order, a wave by the xor butterfly, a workgroup its four waves in
// order, k_ipm_final the partials the same way.  Grid sizes depend on n only and nothing is accumulated with atomics, so a solve is
// bitwise repeatable.  Four times per iteration a record of at most four doubles is read back (stop test, step lengths of the
// predictor, mu_aff, step lengths of the corrector); after the factorisation the count of perturbed pivots (include/pgx_nd.h) is read
// and, if positive, ends the solve.
//
// Streaming kernels over n doubles / nnz values, bound by memory traffic; a row of a P1 stiffness matrix has seven entries, so the
// thread-per-row SpMV keeps its loads inside a few cache lines per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pgx.h"
#include "../../include/pgx_ipm.h"
#include "../../include/pgx_nd.h"
#include "pgx_scope.h"

#define IPM_L 1      // non-fixed dof with a finite lower bound
#define IPM_U 2      // non-fixed dof with a finite upper bound
#define IPM_FIXED 4  // lo == up
#define IPM_MAXB 1024  // block partials per reduced quantity
#define IPM_SUM 0u
#define IPM_MAX 1u
#define IPM_MIN 2u
#define IPM_OPS(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))

static thread_local std::string g_ipm_error;

struct pgx_ipm {
  int n = 0;
  int64_t nnz = 0, nc = 0;
  int device = -1;
  hipStream_t st = nullptr;
  pgx_nd* lu = nullptr;
  std::vector<void*> allocs;
  int32_t *rowptr = nullptr, *col = nullptr, *row = nullptr;
  uint8_t* kind = nullptr;
  double *H = nullptr, *K = nullptr;
  double *b = nullptr, *lo = nullptr, *up = nullptr, *x = nullptr, *z = nullptr, *w = nullptr, *rd = nullptr, *rhs = nullptr;
  double *dx = nullptr, *dz = nullptr, *dw = nullptr, *dxa = nullptr, *dza = nullptr, *dwa = nullptr;
  double *part = nullptr, *scal = nullptr;  // [4][IPM_MAXB] block partials, [4] reduced values
  double* h_scal = nullptr;                 // pinned
  std::vector<double> h_lo, h_up;
  std::vector<uint8_t> h_kind;
  bool have_problem = false;
  std::vector<double> history;
  bool prof = false;
  std::vector<hipEvent_t> ev;  // pairs (begin, end) recorded since the last synchronisation
  std::vector<int> ev_bucket;
  size_t ev_used = 0;
  double prof_ms[PGX_IPM_PROFILE_COLS] = {0, 0, 0, 0, 0};
  std::string err;
};

extern "C" const char* pgx_ipm_last_error(const pgx_ipm* h) { return h ? h->err.c_str() : g_ipm_error.c_str(); }

#define IPMHIP(call)                                              \
  do {                                                            \
    hipError_t e_ = (call);                                       \
    if (e_ != hipSuccess) {                                       \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return PGX_EHIP;                                            \
    }                                                             \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ipm_comb(unsigned op, double a, double b) {
  return op == IPM_SUM ? a + b : op == IPM_MAX ? fmax(a, b) : fmin(a, b);
}
__device__ __forceinline__ double ipm_identity(unsigned op) { return op == IPM_SUM ? 0.0 : op == IPM_MAX ? -INFINITY : INFINITY; }

// the workgroup's (256 threads) value of NQ quantities, quantity q folded with operation (ops >> 2q) & 3, to out[q * stride]
template <int NQ>
__device__ __forceinline__ void ipm_block_reduce(double (&v)[NQ], unsigned ops, double* __restrict__ out, int stride) {
  __shared__ double sh[NQ][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const unsigned op = (ops >> (2 * q)) & 3u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] = ipm_comb(op, v[q], __shfl_xor(v[q], o));
    if (lane == 0) sh[q][wave] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const unsigned op = (ops >> (2 * q)) & 3u;
      double r = sh[q][0];
      for (int k = 1; k < 4; ++k) r = ipm_comb(op, r, sh[q][k]);
      out[(size_t)q * stride] = r;
    }
  }
}

// second stage: part[q][0 .. nb) -> scal[q], one workgroup
__global__ __launch_bounds__(256) void k_ipm_final(int nb, unsigned ops, const double* __restrict__ part, double* __restrict__ scal) {
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned op = (ops >> (2 * q)) & 3u;
    double a = ipm_identity(op);
    for (int j = threadIdx.x; j < nb; j += 256) a = ipm_comb(op, a, part[(size_t)q * IPM_MAXB + j]);
    v[q] = a;
  }
  ipm_block_reduce<4>(v, ops, scal, 1);
}

// r_d and the partials of (|r_d|_inf, sum_L s z, sum_U t w, max complementarity).  use_zw == 0: H x - b alone (the scale of the stop
// test at the start).
__global__ __launch_bounds__(256) void k_ipm_residual(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const double* __restrict__ H, const double* __restrict__ x, const double* __restrict__ b,
                                                      const double* __restrict__ z, const double* __restrict__ w, const double* __restrict__ lo,
                                                      const double* __restrict__ up, const uint8_t* __restrict__ kind, int use_zw,
                                                      double* __restrict__ rd, double* __restrict__ part) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned k = kind[i];
    double r = 0.0;
    if (!(k & IPM_FIXED)) {
      double acc = 0.0;
      for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) acc += H[p] * x[col[p]];
      r = acc - b[i];
      if (use_zw) r = (r - z[i]) + w[i];
    }
    rd[i] = r;
    v[0] = fmax(v[0], fabs(r));
    if (use_zw) {
      if (k & IPM_L) {
        const double c = (x[i] - lo[i]) * z[i];
        v[1] += c, v[3] = fmax(v[3], c);
      }
      if (k & IPM_U) {
        const double c = (up[i] - x[i]) * w[i];
        v[2] += c, v[3] = fmax(v[3], c);
      }
    }
  }
  ipm_block_reduce<4>(v, IPM_OPS(IPM_MAX, IPM_SUM, IPM_SUM, IPM_MAX), part + blockIdx.x, IPM_MAXB);
}

// K = P_F (H + diag(z/s + w/t)) P_F + P_fixed, entry by entry (row[p]: the row of stored entry p)
__global__ __launch_bounds__(256) void k_ipm_kkt(int64_t nnz, const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                 const double* __restrict__ H, const double* __restrict__ x, const double* __restrict__ z,
                                                 const double* __restrict__ w, const double* __restrict__ lo, const double* __restrict__ up,
                                                 const uint8_t* __restrict__ kind, double* __restrict__ K) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * 256) {
    const int i = row[p], j = col[p];
    const unsigned ki = kind[i], kj = kind[j];
    double v;
    if ((ki | kj) & IPM_FIXED)
      v = i == j ? 1.0 : 0.0;
    else {
      v = H[p];
      if (i == j) {
        double d = 0.0;
        if (ki & IPM_L) d = z[i] / (x[i] - lo[i]);
        if (ki & IPM_U) d += w[i] / (up[i] - x[i]);
        v += d;
      }
    }
    K[p] = v;
  }
}

// complementarity targets: predictor (corr == 0) c_z = -s z, c_w = -t w; corrector c_z = sigma mu - s z - dx_aff dz_aff,
// c_w = sigma mu - t w + dx_aff dw_aff
__device__ __forceinline__ void ipm_targets(int corr, double sm, double s, double t, double z, double w, double dxa, double dza, double dwa,
                                            double& cz, double& cw) {
  if (corr) {
    cz = (sm - s * z) - dxa * dza;
    cw = (sm - t * w) + dxa * dwa;
  } else {
    cz = -(s * z);
    cw = -(t * w);
  }
}

__global__ __launch_bounds__(256) void k_ipm_rhs(int n, int corr, double sm, const double* __restrict__ x, const double* __restrict__ z,
                                                 const double* __restrict__ w, const double* __restrict__ lo, const double* __restrict__ up,
                                                 const uint8_t* __restrict__ kind, const double* __restrict__ rd, const double* __restrict__ dxa,
                                                 const double* __restrict__ dza, const double* __restrict__ dwa, double* __restrict__ rhs) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned k = kind[i];
    double r = 0.0;
    if (!(k & IPM_FIXED)) {
      const double s = (k & IPM_L) ? x[i] - lo[i] : 1.0, t = (k & IPM_U) ? up[i] - x[i] : 1.0;
      double cz, cw;
      ipm_targets(corr, sm, s, t, z[i], w[i], corr ? dxa[i] : 0.0, corr ? dza[i] : 0.0, corr ? dwa[i] : 0.0, cz, cw);
      r = -rd[i];
      if (k & IPM_L) r += cz / s;
      if (k & IPM_U) r -= cw / t;
    }
    rhs[i] = r;
  }
}

// dz = (c_z - z dx)/s on L, dw = (c_w + w dx)/t on U (0 elsewhere), and the partials of the four fraction-to-boundary minima:
// -s/dx over L with dx < 0, t/dx over U with dx > 0, -z/dz over L with dz < 0, -w/dw over U with dw < 0.
// Predictor: dx == dxa, dz == dza, dw == dwa (the targets then read none of them), hence no __restrict__ on these.
__global__ __launch_bounds__(256) void k_ipm_recover(int n, int corr, double sm, const double* __restrict__ x, const double* __restrict__ z,
                                                     const double* __restrict__ w, const double* __restrict__ lo, const double* __restrict__ up,
                                                     const uint8_t* __restrict__ kind, const double* dx, const double* dxa, const double* dza,
                                                     const double* dwa, double* dz, double* dw, double* __restrict__ part) {
  double v[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned k = kind[i];
    double dzi = 0.0, dwi = 0.0;
    if (k & (IPM_L | IPM_U)) {
      const double s = (k & IPM_L) ? x[i] - lo[i] : 1.0, t = (k & IPM_U) ? up[i] - x[i] : 1.0;
      const double zi = z[i], wi = w[i], d = dx[i];
      double cz, cw;
      ipm_targets(corr, sm, s, t, zi, wi, corr ? dxa[i] : 0.0, corr ? dza[i] : 0.0, corr ? dwa[i] : 0.0, cz, cw);
      if (k & IPM_L) {
        dzi = (cz - zi * d) / s;
        if (d < 0.0) v[0] = fmin(v[0], -s / d);
        if (dzi < 0.0) v[2] = fmin(v[2], -zi / dzi);
      }
      if (k & IPM_U) {
        dwi = (cw + wi * d) / t;
        if (d > 0.0) v[1] = fmin(v[1], t / d);
        if (dwi < 0.0) v[3] = fmin(v[3], -wi / dwi);
      }
    }
    dz[i] = dzi;
    dw[i] = dwi;
  }
  ipm_block_reduce<4>(v, IPM_OPS(IPM_MIN, IPM_MIN, IPM_MIN, IPM_MIN), part + blockIdx.x, IPM_MAXB);
}

// partials of sum_L (s + a dx)(z + a dz) and sum_U (t - a dx)(w + a dw)
__global__ __launch_bounds__(256) void k_ipm_muaff(int n, double a, const double* __restrict__ x, const double* __restrict__ z,
                                                   const double* __restrict__ w, const double* __restrict__ lo, const double* __restrict__ up,
                                                   const uint8_t* __restrict__ kind, const double* __restrict__ dx, const double* __restrict__ dz,
                                                   const double* __restrict__ dw, double* __restrict__ part) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned k = kind[i];
    if (k & IPM_L) v[0] += ((x[i] - lo[i]) + a * dx[i]) * (z[i] + a * dz[i]);
    if (k & IPM_U) v[1] += ((up[i] - x[i]) - a * dx[i]) * (w[i] + a * dw[i]);
  }
  ipm_block_reduce<4>(v, IPM_OPS(IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM), part + blockIdx.x, IPM_MAXB);
}

// x, z, w += a (dx, dz, dw).  a < alpha_p keeps s, t > 0 in exact arithmetic, but lo + s rounds to lo once s is below an ulp of lo
// (iterates that overshoot the tolerance by many orders): such a dof is put on the first number inside its bound.
__global__ __launch_bounds__(256) void k_ipm_update(int n, double a, const uint8_t* __restrict__ kind, const double* __restrict__ lo,
                                                    const double* __restrict__ up, const double* __restrict__ dx, const double* __restrict__ dz,
                                                    const double* __restrict__ dw, double* __restrict__ x, double* __restrict__ z,
                                                    double* __restrict__ w) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned k = kind[i];
    if (!(k & IPM_FIXED)) {
      double v = x[i] + a * dx[i];
      if ((k & IPM_L) && v <= lo[i]) v = nextafter(lo[i], INFINITY);
      if ((k & IPM_U) && v >= up[i]) v = nextafter(up[i], -INFINITY);
      x[i] = v;
    }
    z[i] += a * dz[i];
    w[i] += a * dw[i];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_ipm_destroy(pgx_ipm* h) {
  if (!h) return;
  if (h->device >= 0 && hipSetDevice(h->device) == hipSuccess) {
    if (h->st) hipStreamSynchronize(h->st);
    if (h->lu) pgx_nd_destroy(h->lu);
    for (void* p : h->allocs) hipFree(p);
    if (h->h_scal) hipHostFree(h->h_scal);
    for (hipEvent_t e : h->ev) hipEventDestroy(e);
    if (h->st) hipStreamDestroy(h->st);
  }
  delete h;
}

template <typename T>
static int ipm_alloc(pgx_ipm* h, T** d, size_t count, const char* what) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc((void**)d, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *d = nullptr;
    h->err = "pgx_ipm_create: n = " + std::to_string(h->n) + ": cannot allocate " + std::to_string(bytes) + " bytes for " + what;
    return PGX_ENOMEM;
  }
  h->allocs.push_back((void*)*d);
  return PGX_OK;
}

extern "C" int pgx_ipm_create(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col, const double* vals, int64_t nvals,
                              int32_t dim, const double* coords, int device, pgx_ipm** out) {
  if (out) *out = nullptr;
  if (!out || !rowptr || !col || !vals || !coords || n_rows < 1 || n_rows >= INT32_MAX || device < 0 || (dim != 2 && dim != 3)) {
    g_ipm_error = "pgx_ipm_create: bad argument (n >= 1, dim 2 or 3, a device, rowptr, col, vals, coords and out are required)";
    return PGX_EINVAL;
  }
  if (n_rows != n_cols) {
    g_ipm_error = "pgx_ipm_create: the Hessian pattern is " + std::to_string(n_rows) + " x " + std::to_string(n_cols) + ", not square";
    return PGX_EINVAL;
  }
  const int64_t n = n_rows, nnz = rowptr[n];
  bool ok = rowptr[0] == 0 && nnz >= 0;
  for (int64_t i = 0; ok && i < n; ++i) {
    ok = rowptr[i + 1] >= rowptr[i] && rowptr[i + 1] <= nnz;
    for (int64_t k = rowptr[i]; ok && k < rowptr[i + 1]; ++k) ok = col[k] >= 0 && col[k] < n && (k == rowptr[i] || col[k] > col[k - 1]);
  }
  if (!ok) {
    g_ipm_error = "pgx_ipm_create: malformed CSR pattern (rowptr monotone from 0, columns in [0, n) strictly increasing within a row)";
    return PGX_EINVAL;
  }
  if (nvals != nnz) {
    g_ipm_error = "pgx_ipm_create: " + std::to_string(nvals) + " Hessian values for a pattern of " + std::to_string(nnz) + " entries";
    return PGX_EINVAL;
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t *r0 = col + rowptr[i], *r1 = col + rowptr[i + 1];
    if (!std::binary_search(r0, r1, (int32_t)i)) {
      g_ipm_error = "pgx_ipm_create: row " + std::to_string(i) + " of the pattern has no diagonal entry (the barrier terms z/s + w/t are added there)";
      return PGX_EINVAL;
    }
    for (const int32_t* c = r0; c < r1; ++c)
      if (!std::binary_search(col + rowptr[*c], col + rowptr[*c + 1], (int32_t)i)) {
        g_ipm_error = "pgx_ipm_create: entry (" + std::to_string(i) + ", " + std::to_string(*c) + ") has no transpose: the pattern of the full symmetric H is required";
        return PGX_EINVAL;
      }
  }
  pgx_ipm* h = new pgx_ipm;
  h->n = (int)n, h->nnz = nnz, h->device = device;
  auto fail = [&](int rc) {
    g_ipm_error = h->err;
    pgx_ipm_destroy(h);
    return rc;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    h->err = std::string("pgx_ipm_create: hipSetDevice: ") + hipGetErrorString(e);
    h->device = -1;
    return fail(PGX_ENODEV);
  }
  if ((e = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking)) != hipSuccess) {
    h->err = std::string("pgx_ipm_create: hipStreamCreate: ") + hipGetErrorString(e);
    return fail(PGX_EHIP);
  }
  std::vector<int32_t> ident((size_t)n), rows((size_t)nnz);
  for (int64_t i = 0; i < n; ++i) {
    ident[(size_t)i] = (int32_t)i;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) rows[(size_t)k] = (int32_t)i;
  }
  pgx_nd_matrix A{};
  A.n = n, A.rowptr = rowptr, A.col = col, A.n_nodes = (int32_t)n, A.node_of_dof = ident.data(), A.dim = dim, A.node_coords = coords;
  A.leaf_nodes = 0;
  int rc = pgx_nd_create(&A, device, (void*)h->st, &h->lu);
  if (rc) {
    h->err = std::string("pgx_ipm_create: ") + pgx_nd_last_error(nullptr);
    h->lu = nullptr;
    return fail(rc);
  }
  pgx_nd_set_symmetric(h->lu, 1);  // K is symmetric positive definite: L D L^T in LU clothing (include/pgx_nd.h)
  const size_t sn = (size_t)n, sz = (size_t)nnz;
  if ((rc = ipm_alloc(h, &h->rowptr, sn + 1, "the row pointers")) || (rc = ipm_alloc(h, &h->col, sz, "the column indices")) ||
      (rc = ipm_alloc(h, &h->row, sz, "the row indices")) || (rc = ipm_alloc(h, &h->kind, sn, "the dof kinds")) ||
      (rc = ipm_alloc(h, &h->H, sz, "the Hessian")) || (rc = ipm_alloc(h, &h->K, sz, "the KKT matrix")) ||
      (rc = ipm_alloc(h, &h->part, 4 * (size_t)IPM_MAXB, "the block partials")) || (rc = ipm_alloc(h, &h->scal, 4, "the reduced scalars")))
    return fail(rc);
  for (double** v : {&h->b, &h->lo, &h->up, &h->x, &h->z, &h->w, &h->rd, &h->rhs, &h->dx, &h->dz, &h->dw, &h->dxa, &h->dza, &h->dwa})
    if ((rc = ipm_alloc(h, v, sn, "an iterate vector"))) return fail(rc);
  if (hipHostMalloc((void**)&h->h_scal, 4 * sizeof(double)) != hipSuccess) {
    h->h_scal = nullptr;
    h->err = "pgx_ipm_create: hipHostMalloc failed";
    return fail(PGX_ENOMEM);
  }
  if ((e = hipMemcpy(h->rowptr, rowptr, (sn + 1) * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(h->col, col, sz * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(h->row, rows.data(), sz * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(h->H, vals, sz * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) {
    h->err = std::string("pgx_ipm_create: hipMemcpy: ") + hipGetErrorString(e);
    return fail(PGX_EHIP);
  }
  *out = h;
  return PGX_OK;
}

extern "C" int pgx_ipm_set_problem(pgx_ipm* h, const double* b, const double* lo, const double* up) {
  if (!h || !b || !lo || !up) return PGX_EINVAL;
  const size_t n = (size_t)h->n;
  std::vector<uint8_t> kind(n);
  int64_t nc = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!(lo[i] <= up[i])) {  // also a NaN bound
      h->err = "pgx_ipm_set_problem: lo[" + std::to_string(i) + "] = " + std::to_string(lo[i]) + " > up[" + std::to_string(i) + "] = " +
               std::to_string(up[i]) + " (or a NaN bound): the feasible set is empty";
      return PGX_EINVAL;
    }
    if (lo[i] == up[i]) {
      if (std::isinf(lo[i])) {
        h->err = "pgx_ipm_set_problem: dof " + std::to_string(i) + " is fixed at an infinite value";
        return PGX_EINVAL;
      }
      kind[i] = IPM_FIXED;
    } else {
      kind[i] = (uint8_t)((std::isfinite(lo[i]) ? IPM_L : 0) | (std::isfinite(up[i]) ? IPM_U : 0));
      nc += (kind[i] & IPM_L ? 1 : 0) + (kind[i] & IPM_U ? 1 : 0);
    }
  }
  IPMHIP(hipSetDevice(h->device));
  h->have_problem = false;
  h->h_lo.assign(lo, lo + n), h->h_up.assign(up, up + n), h->h_kind = kind, h->nc = nc;
  IPMHIP(hipMemcpyAsync(h->b, b, n * sizeof(double), hipMemcpyHostToDevice, h->st));
  IPMHIP(hipMemcpyAsync(h->lo, h->h_lo.data(), n * sizeof(double), hipMemcpyHostToDevice, h->st));
  IPMHIP(hipMemcpyAsync(h->up, h->h_up.data(), n * sizeof(double), hipMemcpyHostToDevice, h->st));
  IPMHIP(hipMemcpyAsync(h->kind, h->h_kind.data(), n, hipMemcpyHostToDevice, h->st));
  IPMHIP(hipStreamSynchronize(h->st));  // b is the caller's
  h->have_problem = true;
  h->err.clear();
  return PGX_OK;
}

// --- profile: pairs of events around a phase, turned into milliseconds at the next synchronisation of the stream ---
static void ipm_mark(pgx_ipm* h, int bucket) {  // bucket >= 0: a phase begins; -1: it ends
  if (!h->prof) return;
  if (h->ev_used >= h->ev.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    h->ev.push_back(e);
  }
  hipEventRecord(h->ev[h->ev_used++], h->st);
  if (bucket >= 0) h->ev_bucket.push_back(bucket);
}
static void ipm_collect(pgx_ipm* h) {  // after a stream synchronisation
  for (size_t p = 0; 2 * p + 1 < h->ev_used; ++p) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev[2 * p], h->ev[2 * p + 1]) == hipSuccess) h->prof_ms[h->ev_bucket[p]] += ms;
  }
  h->ev_used = 0;
  h->ev_bucket.clear();
}
struct IpmPhase {
  pgx_ipm* h;
  IpmPhase(pgx_ipm* h_, int bucket) : h(h_) { ipm_mark(h, bucket); }
  ~IpmPhase() { ipm_mark(h, -1); }
};

extern "C" int pgx_ipm_profile(pgx_ipm* h, int enable, double* ms) {
  if (!h) return PGX_EINVAL;
  for (int k = 0; k < PGX_IPM_PROFILE_COLS; ++k) {
    if (ms) ms[k] = h->prof_ms[k];
    h->prof_ms[k] = 0;
  }
  h->prof = enable != 0;
  return PGX_OK;
}

static inline int ipm_blocks(int64_t count) { return (int)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, IPM_MAXB)); }

// second stage of the reduction the last kernel left in h->part, its four values to h->h_scal; the stream is idle on return
static int ipm_reduce_to_host(pgx_ipm* h, unsigned ops) {
  hipLaunchKernelGGL(k_ipm_final, dim3(1), dim3(256), 0, h->st, ipm_blocks(h->n), ops, h->part, h->scal);
  ipm_mark(h, -1);  // (closes the phase of the caller: the read-back below is not device time)
  IPMHIP(hipGetLastError());
  IPMHIP(hipMemcpyAsync(h->h_scal, h->scal, 4 * sizeof(double), hipMemcpyDeviceToHost, h->st));
  IPMHIP(hipStreamSynchronize(h->st));
  ipm_collect(h);
  return PGX_OK;
}

static int ipm_residual(pgx_ipm* h, int use_zw) {
  ipm_mark(h, 0);
  hipLaunchKernelGGL(k_ipm_residual, dim3(ipm_blocks(h->n)), dim3(256), 0, h->st, h->n, h->rowptr, h->col, h->H, h->x, h->b, h->z, h->w, h->lo,
                     h->up, h->kind, use_zw, h->rd, h->part);
  return ipm_reduce_to_host(h, IPM_OPS(IPM_MAX, IPM_SUM, IPM_SUM, IPM_MAX));
}

static void ipm_fill(pgx_ipm* h) {
  IpmPhase ph(h, 1);
  hipLaunchKernelGGL(k_ipm_kkt, dim3(ipm_blocks(h->nnz)), dim3(256), 0, h->st, h->nnz, h->row, h->col, h->H, h->x, h->z, h->w, h->lo, h->up,
                     h->kind, h->K);
}

// direction for the targets of the predictor (corr = 0: to dxa, dza, dwa) or the corrector (to dx, dz, dw); alpha_p, alpha_d of it
static int ipm_direction(pgx_ipm* h, int corr, double sm, double* ap, double* ad) {
  const int nb = ipm_blocks(h->n);
  double *dx = corr ? h->dx : h->dxa, *dz = corr ? h->dz : h->dza, *dw = corr ? h->dw : h->dwa;
  {
    IpmPhase ph(h, 4);
    hipLaunchKernelGGL(k_ipm_rhs, dim3(nb), dim3(256), 0, h->st, h->n, corr, sm, h->x, h->z, h->w, h->lo, h->up, h->kind, h->rd, h->dxa, h->dza,
                       h->dwa, h->rhs);
  }
  {
    IpmPhase ph(h, 3);
    const int rc = pgx_nd_solve(h->lu, h->rhs, dx, 1);
    if (rc) {
      h->err = std::string("pgx_ipm_solve: ") + pgx_nd_last_error(h->lu);
      return rc;
    }
  }
  ipm_mark(h, 4);
  hipLaunchKernelGGL(k_ipm_recover, dim3(nb), dim3(256), 0, h->st, h->n, corr, sm, h->x, h->z, h->w, h->lo, h->up, h->kind, dx, h->dxa, h->dza,
                     h->dwa, dz, dw, h->part);
  const int rc = ipm_reduce_to_host(h, IPM_OPS(IPM_MIN, IPM_MIN, IPM_MIN, IPM_MIN));
  if (rc) return rc;
  *ap = std::min(1.0, std::min(h->h_scal[0], h->h_scal[1]));
  *ad = std::min(1.0, std::min(h->h_scal[2], h->h_scal[3]));
  return PGX_OK;
}

static int ipm_upload(pgx_ipm* h, const double* x, const double* z, const double* w) {
  const size_t bytes = (size_t)h->n * sizeof(double);
  h->ev_used = 0, h->ev_bucket.clear();  // (a call that failed half-way may have left an open phase behind)
  IPMHIP(hipMemcpyAsync(h->x, x, bytes, hipMemcpyHostToDevice, h->st));
  IPMHIP(hipMemcpyAsync(h->z, z, bytes, hipMemcpyHostToDevice, h->st));
  IPMHIP(hipMemcpyAsync(h->w, w, bytes, hipMemcpyHostToDevice, h->st));
  IPMHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}

static int ipm_ready(pgx_ipm* h, const char* who) {
  if (!h->have_problem) {
    h->err = std::string(who) + ": no problem set (call pgx_ipm_set_problem first)";
    return PGX_ESTATE;
  }
  return PGX_OK;
}

extern "C" int pgx_ipm_solve(pgx_ipm* h, const double* x_init, double tol, int32_t max_iter, int32_t monitor, double* x, double* z, double* w,
                             int32_t* iterations, int32_t* status) {
  if (!h || !x_init || !x || !z || !w || !iterations || !status || !(tol > 0.0) || max_iter < 0) {
    if (h) h->err = "pgx_ipm_solve: bad argument (x_init, x, z, w, iterations, status required; tol > 0; max_iter >= 0)";
    return PGX_EINVAL;
  }
  int rc = ipm_ready(h, "pgx_ipm_solve");
  if (rc) return rc;
  IPMHIP(hipSetDevice(h->device));
  PgxRange range("pgx_ipm:solve");
  const int n = h->n, nb = ipm_blocks(n);
  const double nc = (double)h->nc;
  // the start: strictly inside the bounds, unit multipliers
  std::vector<double> x0((size_t)n), z0((size_t)n), w0((size_t)n);
  for (int i = 0; i < n; ++i) {
    const unsigned k = h->h_kind[(size_t)i];
    const double l = h->h_lo[(size_t)i], u = h->h_up[(size_t)i];
    double v = x_init[i];
    if (k & IPM_FIXED)
      v = l;
    else if ((k & IPM_L) && (k & IPM_U))
      v = (v > l && v < u) ? v : 0.5 * (l + u);
    else if (k & IPM_L)
      v = std::max(v, l + 1.0);
    else if (k & IPM_U)
      v = std::min(v, u - 1.0);
    x0[(size_t)i] = v, z0[(size_t)i] = (k & IPM_L) ? 1.0 : 0.0, w0[(size_t)i] = (k & IPM_U) ? 1.0 : 0.0;
  }
  if ((rc = ipm_upload(h, x0.data(), z0.data(), w0.data()))) return rc;
  if ((rc = ipm_residual(h, 0))) return rc;
  const double scale = std::max(1.0, h->h_scal[0]);
  h->history.clear();
  *status = 1;
  int it = 0;
  for (;;) {
    if ((rc = ipm_residual(h, 1))) return rc;
    const double rdn = h->h_scal[0], mu = nc > 0 ? (h->h_scal[1] + h->h_scal[2]) / nc : 0.0, cmax = h->h_scal[3];
    if (monitor) printf("  ipm %3d  |r_d| = %.3e  mu = %.3e  max s z = %.3e\n", it, rdn, mu, cmax);
    if (!std::isfinite(rdn) || !std::isfinite(mu)) {
      h->err = "pgx_ipm_solve: non-finite iterate at iteration " + std::to_string(it);
      return PGX_ESTATE;
    }
    const bool converged = std::max(rdn, mu) <= tol * scale;
    if (converged) *status = 0;
    if (converged || it >= max_iter) {
      h->history.insert(h->history.end(), {rdn, mu, cmax, 0.0, 0.0, 0.0});
      break;
    }
    ipm_fill(h);
    {
      IpmPhase ph(h, 2);
      if ((rc = pgx_nd_factor(h->lu, h->K, 1))) {
        h->err = std::string("pgx_ipm_solve: ") + pgx_nd_last_error(h->lu);
        return rc;
      }
    }
    pgx_nd_stats st{};
    pgx_nd_get_stats(h->lu, &st);  // waits for the factorisation's pivot count
    if (st.perturbed_pivots > 0) {
      h->err = "pgx_ipm_solve: iteration " + std::to_string(it) + ": the factorisation of H + diag(z/s + w/t) perturbed " +
               std::to_string(st.perturbed_pivots) + " pivot(s): H is not positive definite on the free dofs to working precision";
      return PGX_ESTATE;
    }
    double apa, ada, ap, ad;
    if ((rc = ipm_direction(h, 0, 0.0, &apa, &ada))) return rc;
    const double a = std::min(apa, ada);
    ipm_mark(h, 0);
    hipLaunchKernelGGL(k_ipm_muaff, dim3(nb), dim3(256), 0, h->st, n, a, h->x, h->z, h->w, h->lo, h->up, h->kind, h->dxa, h->dza, h->dwa, h->part);
    if ((rc = ipm_reduce_to_host(h, IPM_OPS(IPM_SUM, IPM_SUM, IPM_SUM, IPM_SUM)))) return rc;
    const double mu_aff = nc > 0 ? (h->h_scal[0] + h->h_scal[1]) / nc : 0.0;
    const double q = mu > 0.0 ? mu_aff / mu : 0.0, sigma = q * q * q;
    if ((rc = ipm_direction(h, 1, sigma * mu, &ap, &ad))) return rc;
    const double alpha = std::min(1.0, std::max(0.995, 1.0 - mu) * std::min(ap, ad));
    h->history.insert(h->history.end(), {rdn, mu, cmax, sigma, ap, ad});
    {
      IpmPhase ph(h, 4);
      hipLaunchKernelGGL(k_ipm_update, dim3(nb), dim3(256), 0, h->st, n, alpha, h->kind, h->lo, h->up, h->dx, h->dz, h->dw, h->x, h->z, h->w);
    }
    ++it;
  }
  const size_t bytes = (size_t)n * sizeof(double);
  IPMHIP(hipMemcpyAsync(x, h->x, bytes, hipMemcpyDeviceToHost, h->st));
  IPMHIP(hipMemcpyAsync(z, h->z, bytes, hipMemcpyDeviceToHost, h->st));
  IPMHIP(hipMemcpyAsync(w, h->w, bytes, hipMemcpyDeviceToHost, h->st));
  IPMHIP(hipStreamSynchronize(h->st));
  ipm_collect(h);
  *iterations = it;
  h->err.clear();
  return PGX_OK;
}

extern "C" int pgx_ipm_history(const pgx_ipm* h, int64_t* n_rows, double* rows) {
  if (!h || !n_rows) return PGX_EINVAL;
  *n_rows = (int64_t)(h->history.size() / PGX_IPM_HISTORY_COLS);
  if (rows && !h->history.empty()) std::memcpy(rows, h->history.data(), h->history.size() * sizeof(double));
  return PGX_OK;
}

extern "C" int pgx_ipm_eval(pgx_ipm* h, const double* x, const double* z, const double* w, double* rd_out, double* scalars_out) {
  if (!h || !x || !z || !w || !rd_out || !scalars_out) return PGX_EINVAL;
  int rc = ipm_ready(h, "pgx_ipm_eval");
  if (rc) return rc;
  IPMHIP(hipSetDevice(h->device));
  if ((rc = ipm_upload(h, x, z, w)) || (rc = ipm_residual(h, 1))) return rc;
  scalars_out[0] = h->h_scal[0];
  scalars_out[1] = h->nc > 0 ? (h->h_scal[1] + h->h_scal[2]) / (double)h->nc : 0.0;
  scalars_out[2] = h->h_scal[3];
  IPMHIP(hipMemcpy(rd_out, h->rd, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost));
  return PGX_OK;
}

extern "C" int pgx_ipm_kkt_export(pgx_ipm* h, const double* x, const double* z, const double* w, double* vals_out) {
  if (!h || !x || !z || !w || !vals_out) return PGX_EINVAL;
  int rc = ipm_ready(h, "pgx_ipm_kkt_export");
  if (rc) return rc;
  IPMHIP(hipSetDevice(h->device));
  if ((rc = ipm_upload(h, x, z, w))) return rc;
  ipm_fill(h);
  IPMHIP(hipGetLastError());
  IPMHIP(hipStreamSynchronize(h->st));
  ipm_collect(h);
  IPMHIP(hipMemcpy(vals_out, h->K, (size_t)h->nnz * sizeof(double), hipMemcpyDeviceToHost));
  return PGX_OK;
}
