// pgx_bd.hip - band LU with partial pivoting on the GPU (include/pgx_bd.h): LAPACK's dgbtrf / dgbtrs for Newton matrices that need
// row interchanges and have a narrow band in the caller's ordering (example 09, the eikonal equation on the Moebius strip).
//
// Storage: LAPACK's band layout, entry (i, j) at ab[j * ldab + kv + i - j], kv = kl + ku, ldab = 2 kl + ku + 1: the kl rows on top of
// every column receive the fill of U.  As in dgbtf2 an interchange moves the part of the two rows on and right of the pivot column
// only, so the multipliers of column j stay in the rows j + 1 .. j + kl and L keeps its band.
//
// Factorisation, right-looking in panels of BD_NB = 32 columns, TWO launches per panel and no host synchronisation before the final
// read-back:
//
//   k_bd_panel   ONE workgroup, one THREAD PER ROW of the (kl + 32) x 32 panel, the row's 32 entries in registers (the panel never
//                touches LDS: kl <= PGX_BD_MAX_KL = 960 keeps it within 1024 threads).  Per column: argmax (wave butterfly, then
//                the <= 16 wave winners through LDS - larger modulus, lower row among equals: a total order), the two rows of the
//                interchange travel through 2 x 32 doubles of LDS, every thread reads the pivot row from there (broadcast), scales
//                its multiplier and updates its row.  Two barriers per column.
//   k_bd_right   the kl + ku columns right of the panel, BD_CT = 4 per workgroup, again one thread per row: the panel's 32
//                elimination steps (interchange, then axpy with the panel's multipliers, which every thread has loaded up front)
//                applied to the 4 entries of its row.  One barrier per step (the exchange buffer alternates).  This is dgbtrs's
//                forward sweep with the columns of A as right-hand sides; it does the flops of U12 = L11^-1 A12 and
//                A22 -= L21 U12 without forming either, so nothing has to be un-permuted afterwards.
//
// Solve: gather by the symmetric permutation; k_bd_fwd, ONE persistent workgroup that runs the same elimination step over the
// right-hand side panel by panel; k_bd_bwd, ONE persistent workgroup: per 64 columns wave 0 solves the 64 x 64 triangle (lane = row,
// solved entries by v_readlane) and all threads then update the kv rows above, one row each; scatter back.  Four launches per solve.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pgx.h"
#include "../../include/pgx_bd.h"
#include "pgx_scope.h"

#define BD_NB PGX_BD_NB
#define BD_NT 1024  // threads of the row-per-thread kernels at most
#define BD_CT 4     // columns per workgroup of k_bd_right
#define BD_SW 64    // columns per step of the backward sweep = one wave
static_assert(PGX_BD_MAX_KL + BD_NB <= BD_NT, "one thread per panel row");
static_assert(BD_NB % 2 == 0, "the exchange buffers alternate and every panel starts with the first");

static thread_local std::string g_bd_error;

struct pgx_bd {
  int64_t n = 0, nnz = 0;
  int kl = 0, ku = 0, kv = 0, ldab = 1;
  int device = -1;
  hipStream_t st = nullptr;
  bool own_stream = false;
  double* ab = nullptr;       // [ldab * n] the band, then L\U
  int64_t* d_dest = nullptr;  // [nnz] position of each CSR entry in ab
  double* d_vals = nullptr;   // [nnz] staging for host values
  int32_t *d_piv = nullptr, *d_perm = nullptr, *d_info = nullptr;
  double *d_diag = nullptr, *d_w = nullptr, *d_io = nullptr;
  std::vector<int32_t> piv;
  std::vector<double> diag;
  pgx_bd_stats stats{};
  bool factored = false;
  bool timing = false;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double factor_ms = 0, solve_ms = 0;
  std::string err;
};

extern "C" const char* pgx_bd_last_error(const pgx_bd* s) { return s ? s->err.c_str() : g_bd_error.c_str(); }

#define BDHIP(call)                                               \
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
__global__ __launch_bounds__(256) void k_bd_scatter(int64_t nnz, const int64_t* __restrict__ dest, const double* __restrict__ vals,
                                                    double* __restrict__ ab) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) ab[dest[i]] = vals[i];
}

// candidate (v, i) against the best so far: larger modulus wins, the lower row among equals.  Lanes without a row carry (-1, INT_MAX).
__device__ __forceinline__ void bd_best(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) bv = v, bi = i;
}
__device__ __forceinline__ double bd_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// The panel [j0, j0 + w): thread r holds row j0 + r, a[c] = A(j0 + r, j0 + c).  Entries outside the stored band (below the kl-th
// subdiagonal, above the kv-th superdiagonal, columns >= w, rows >= n) are zeros that no step changes, and are never written back.
// A column whose candidates are all exactly zero is counted and left alone.
__global__ __launch_bounds__(BD_NT) void k_bd_panel(double* __restrict__ ab, int n, int kl, int kv, int ldab, int j0, int w,
                                                    int32_t* __restrict__ piv, double* __restrict__ diag, int32_t* __restrict__ info) {
  __shared__ double sv[BD_NT / 64];
  __shared__ int si[BD_NT / 64];
  __shared__ double rows[2][BD_NB];  // [0] the pivot row, [1] the row that was in the diagonal's place
  const int r = threadIdx.x, lane = r & 63, wv = r >> 6, nw = blockDim.x >> 6;
  const int i = j0 + r;
  const bool rowok = i < n && r < kl + w;
  double a[BD_NB];
#pragma unroll
  for (int c = 0; c < BD_NB; ++c) {
    const int d = r - c;
    a[c] = (rowok && c < w && d <= kl && -d <= kv) ? (ab + ((int64_t)(j0 + c) * ldab + kv - c))[r] : 0.0;  // uniform base + row
  }
#pragma unroll
  for (int jj = 0; jj < BD_NB; ++jj) {
    if (jj < w) {  // uniform
      const int km = min(kl, n - 1 - (j0 + jj));
      const bool cand = r >= jj && r <= jj + km;
      double v = cand ? fabs(a[jj]) : -1.0;
      int p = cand ? r : INT_MAX;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(p, o);
        bd_best(v, p, ov, oi);
      }
      if (lane == 0) sv[wv] = v, si[wv] = p;
      __syncthreads();
      v = sv[0], p = si[0];
      for (int q = 1; q < nw; ++q) bd_best(v, p, sv[q], si[q]);
      if (p < jj || p > jj + km) p = jj;  // a column of NaNs leaves (-1, INT_MAX): whatever the values, the row is a candidate
      if (r == p) {
#pragma unroll
        for (int c = jj; c < BD_NB; ++c) rows[0][c] = a[c];
      }
      if (r == jj) {
#pragma unroll
        for (int c = jj; c < BD_NB; ++c) rows[1][c] = a[c];
      }
      __syncthreads();
      const double pv = rows[0][jj];
      if (r == 0) {
        piv[j0 + jj] = j0 + p;
        diag[j0 + jj] = pv;
        if (v == 0.0) info[0] += 1;  // every candidate exactly zero (launches of one stream: no concurrent writer)
      }
      if (r == jj) {
#pragma unroll
        for (int c = jj; c < BD_NB; ++c) a[c] = rows[0][c];
      } else if (r == p) {
#pragma unroll
        for (int c = jj; c < BD_NB; ++c) a[c] = rows[1][c];
      }
      if (r > jj && r <= jj + km && pv != 0.0) {
        const double l = a[jj] * (1.0 / pv);  // dgbtf2 scales by the reciprocal
        a[jj] = l;
#pragma unroll
        for (int c = jj + 1; c < BD_NB; ++c) a[c] = fma(-l, rows[0][c], a[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < BD_NB; ++c) {
    const int d = r - c;
    if (rowok && c < w && d <= kl && -d <= kv) (ab + ((int64_t)(j0 + c) * ldab + kv - c))[r] = a[c];
  }
}

// The w elimination steps of the panel [j0, j0 + w) on CT column entries of row j0 + threadIdx.x (v): per step the interchange
// (rows k and piv[k] through LDS) and v -= L(row, k) * (pivot row's v).  buf alternates between the steps, so one barrier each.
// Every thread of the workgroup must call this (barriers), whether its row takes part or not.
template <int CT>
__device__ __forceinline__ void bd_eliminate(const double* __restrict__ ab, int n, int kl, int kv, int ldab, int j0, int w,
                                             const int32_t* __restrict__ piv, double (&v)[CT], double (*buf)[2][CT]) {
  const int r = threadIdx.x;
  const bool rowok = j0 + r < n;
  double l[BD_NB];
#pragma unroll
  for (int k = 0; k < BD_NB; ++k) {
    const int d = r - k;
    l[k] = (rowok && k < w && d > 0 && d <= kl) ? (ab + ((int64_t)(j0 + k) * ldab + kv - k))[r] : 0.0;  // uniform base + row
  }
#pragma unroll
  for (int k = 0; k < BD_NB; ++k) {
    if (k < w) {  // uniform
      const int p = piv[j0 + k] - j0;
      double(*b)[CT] = buf[k & 1];
      if (r == p) {
#pragma unroll
        for (int q = 0; q < CT; ++q) b[0][q] = v[q];
      }
      if (r == k) {
#pragma unroll
        for (int q = 0; q < CT; ++q) b[1][q] = v[q];
      }
      __syncthreads();
      const bool on = rowok && r > k && r - k <= kl;
#pragma unroll
      for (int q = 0; q < CT; ++q) {
        const double t = b[0][q];
        if (r == k)
          v[q] = t;
        else if (r == p)
          v[q] = b[1][q];
        if (on) v[q] = fma(-l[k], t, v[q]);
      }
    }
  }
}

// the columns right of the full panel [j0, j0 + BD_NB) that its rows reach: [j0 + BD_NB, min(n, j0 + BD_NB + kv)), BD_CT per workgroup
__global__ __launch_bounds__(BD_NT) void k_bd_right(double* __restrict__ ab, int n, int kl, int kv, int ldab, int j0,
                                                    const int32_t* __restrict__ piv) {
  __shared__ double buf[2][2][BD_CT];
  const int r = threadIdx.x, i = j0 + r;
  const int c0 = j0 + BD_NB + (int)blockIdx.x * BD_CT;
  const int cend = (int)min((int64_t)n, (int64_t)j0 + BD_NB + kv);
  const bool rowok = i < n && r < kl + BD_NB;
  double v[BD_CT];
  bool stored[BD_CT];
#pragma unroll
  for (int q = 0; q < BD_CT; ++q) {
    const int c = c0 + q;
    stored[q] = rowok && c < cend && i - c <= kl && c - i <= kv;
    v[q] = stored[q] ? ab[(int64_t)c * ldab + kv + i - c] : 0.0;
  }
  bd_eliminate<BD_CT>(ab, n, kl, kv, ldab, j0, BD_NB, piv, v, buf);
#pragma unroll
  for (int q = 0; q < BD_CT; ++q)
    if (stored[q]) ab[(int64_t)(c0 + q) * ldab + kv + i - (c0 + q)] = v[q];
}

__global__ __launch_bounds__(256) void k_bd_gather(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ b,
                                                   double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = b[perm[i]];
}
__global__ __launch_bounds__(256) void k_bd_spread(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ y,
                                                   double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[perm[i]] = y[i];
}

// y <- L^-1 P y: ONE workgroup walks the panels; the rows j0 .. j0 + w - 1 + kl of a panel sit one per thread
__global__ __launch_bounds__(BD_NT) void k_bd_fwd(const double* __restrict__ ab, int n, int kl, int kv, int ldab,
                                                  const int32_t* __restrict__ piv, double* __restrict__ y) {
  __shared__ double buf[2][2][1];
  const int r = threadIdx.x;
#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += BD_NB) {
    const int w = min(BD_NB, n - j0);
    const bool part = j0 + r < n && r < kl + w;
    double v[1] = {part ? y[j0 + r] : 0.0};
    bd_eliminate<1>(ab, n, kl, kv, ldab, j0, w, piv, v, buf);
    if (part) y[j0 + r] = v[0];
    __syncthreads();  // the next panel's threads read what these wrote
  }
}

// y <- U^-1 y: ONE workgroup walks the panels of BD_SW columns from the last one; wave 0 solves the triangle, all threads update above
__global__ __launch_bounds__(512) void k_bd_bwd(const double* __restrict__ ab, int n, int kv, int ldab, double* __restrict__ y) {
  __shared__ double xs[BD_SW];
  __shared__ double Us[BD_SW][BD_SW];
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int j0 = ((n - 1) / BD_SW) * BD_SW; j0 >= 0; j0 -= BD_SW) {
    const int w = min(BD_SW, n - j0);
    for (int e = tid; e < BD_SW * BD_SW; e += 512) {  // U11, column k at Us[k][.]; 1 below the diagonal: nothing divides by a non-pivot
      const int k = e >> 6, i = e & 63;
      Us[k][i] = (i < w && k < w && k >= i && k - i <= kv) ? (ab + ((int64_t)(j0 + k) * ldab + kv - k))[i] : (k > i ? 0.0 : 1.0);
    }
    __syncthreads();
    if (tid < 64) {
      const int i = tid;
      double yi = i < w ? y[j0 + i] : 0.0;
      for (int k = w - 1; k >= 0; --k) {
        const double uk = Us[k][i];
        const double xk = bd_bcast(yi / uk, k);  // lane k: its diagonal entry
        if (i < k)
          yi = fma(-uk, xk, yi);
        else if (i == k)
          yi = xk;
      }
      if (i < w) xs[i] = yi, y[j0 + i] = yi;
    }
    __syncthreads();
    for (int i = max(0, j0 - kv) + tid; i < j0; i += 512) {
      double acc = y[i];
#pragma unroll 8
      for (int k = 0; k < w; ++k) {
        const int d = j0 + k - i;  // > 0
        if (d <= kv) acc = fma(-ab[(int64_t)(j0 + k) * ldab + kv - d], xs[k], acc);
      }
      y[i] = acc;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_bd_destroy(pgx_bd* s) {
  if (!s) return;
  if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess) {
    if (s->st) hipStreamSynchronize(s->st);
    for (void* p : {(void*)s->ab, (void*)s->d_dest, (void*)s->d_vals, (void*)s->d_piv, (void*)s->d_perm, (void*)s->d_info, (void*)s->d_diag,
                    (void*)s->d_w, (void*)s->d_io})
      if (p) hipFree(p);
    if (s->e0) hipEventDestroy(s->e0);
    if (s->e1) hipEventDestroy(s->e1);
    if (s->own_stream && s->st) hipStreamDestroy(s->st);
  }
  delete s;
}

template <typename T>
static int bd_alloc(pgx_bd* s, T** d, size_t count, const char* what) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc((void**)d, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *d = nullptr;
    s->err = "pgx_bd_create: n = " + std::to_string(s->n) + ", kl = " + std::to_string(s->kl) + ", ku = " + std::to_string(s->ku) +
             ": cannot allocate " + std::to_string(bytes) + " bytes for " + what;
    return PGX_ENOMEM;
  }
  return PGX_OK;
}

extern "C" int pgx_bd_create(int64_t n, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int device, void* hip_stream,
                             pgx_bd** out) {
  if (out) *out = nullptr;
  if (!out || !rowptr || n < 1 || n > (int64_t)1 << 30 || device < 0) {
    g_bd_error = "pgx_bd_create: bad argument (1 <= n <= 2^30, a device, rowptr and out are required)";
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
    g_bd_error = "pgx_bd_create: malformed CSR pattern (rowptr monotone from 0, columns in [0, n) strictly increasing within a row)";
    return PGX_EINVAL;
  }
  std::vector<int32_t> iperm((size_t)n, -1), hperm((size_t)n);  // iperm[old] = new
  for (int64_t i = 0; i < n; ++i) {
    const int64_t o = perm ? perm[i] : i;
    if (o < 0 || o >= n || iperm[(size_t)o] >= 0) {
      g_bd_error = "pgx_bd_create: perm is not a permutation of 0 .. n - 1 (entry " + std::to_string(i) + " = " + std::to_string(o) + ")";
      return PGX_EINVAL;
    }
    iperm[(size_t)o] = (int32_t)i, hperm[(size_t)i] = (int32_t)o;
  }
  int64_t kl = 0, ku = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int64_t d = (int64_t)iperm[(size_t)i] - iperm[(size_t)col[k]];
      kl = std::max(kl, d), ku = std::max(ku, -d);
    }
  const int64_t ldab = 2 * kl + ku + 1;
  const double gib = (double)ldab * (double)n * 8.0 / 1073741824.0;
  const std::string size = "n = " + std::to_string(n) + ", kl = " + std::to_string(kl) + ", ku = " + std::to_string(ku);
  if ((double)ldab * (double)n * 8.0 > (double)PGX_BD_MAX_BYTES) {  // before anything is allocated
    g_bd_error = "pgx_bd_create: " + size + ": the band storage of (2 kl + ku + 1) n doubles, " + std::to_string(gib) +
                 " GiB, exceeds PGX_BD_MAX_BYTES = 8 GiB";
    return PGX_EINVAL;
  }
  if (kl > PGX_BD_MAX_KL) {
    g_bd_error = "pgx_bd_create: " + size + ": the lower bandwidth exceeds PGX_BD_MAX_KL = " + std::to_string(PGX_BD_MAX_KL) +
                 " (one thread per row of a kl + " + std::to_string(BD_NB) + " rows tall panel)";
    return PGX_EINVAL;
  }
  pgx_bd* s = new pgx_bd;
  s->n = n, s->nnz = nnz, s->device = device;
  s->kl = (int)kl, s->ku = (int)ku, s->kv = (int)(kl + ku), s->ldab = (int)ldab;
  s->stats.n = n, s->stats.kl = kl, s->stats.ku = ku, s->stats.bytes = ldab * n * 8;
  auto fail = [&](int rc) {
    g_bd_error = s->err;
    pgx_bd_destroy(s);
    return rc;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    s->err = std::string("pgx_bd_create: hipSetDevice: ") + hipGetErrorString(e);
    s->device = -1;
    return fail(PGX_ENODEV);
  }
  if (hip_stream)
    s->st = (hipStream_t)hip_stream;
  else {
    if ((e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking)) != hipSuccess) {
      s->err = std::string("pgx_bd_create: hipStreamCreate: ") + hipGetErrorString(e);
      return fail(PGX_EHIP);
    }
    s->own_stream = true;
  }
  int rc;
  if ((rc = bd_alloc(s, &s->ab, (size_t)ldab * (size_t)n, "the band")) || (rc = bd_alloc(s, &s->d_dest, (size_t)nnz, "the scatter map")) ||
      (rc = bd_alloc(s, &s->d_vals, (size_t)nnz, "the CSR values")) || (rc = bd_alloc(s, &s->d_piv, (size_t)n, "the pivot vector")) ||
      (rc = bd_alloc(s, &s->d_perm, (size_t)n, "the permutation")) || (rc = bd_alloc(s, &s->d_info, 1, "the info word")) ||
      (rc = bd_alloc(s, &s->d_diag, (size_t)n, "the pivots")) || (rc = bd_alloc(s, &s->d_w, (size_t)n, "a work vector")) ||
      (rc = bd_alloc(s, &s->d_io, (size_t)n, "a work vector")))
    return fail(rc);
  std::vector<int64_t> dest((size_t)nnz);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int64_t in = iperm[(size_t)i], jn = iperm[(size_t)col[k]];
      dest[(size_t)k] = jn * ldab + (kl + ku) + in - jn;
    }
  if ((nnz && (e = hipMemcpy(s->d_dest, dest.data(), (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) ||
      (e = hipMemcpy(s->d_perm, hperm.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess) {
    s->err = std::string("pgx_bd_create: hipMemcpy: ") + hipGetErrorString(e);
    return fail(PGX_EHIP);
  }
  if (hipEventCreate(&s->e0) != hipSuccess || hipEventCreate(&s->e1) != hipSuccess) {
    s->err = "pgx_bd_create: hipEventCreate failed";
    return fail(PGX_EHIP);
  }
  s->piv.assign((size_t)n, 0);
  s->diag.assign((size_t)n, 0.0);
  *out = s;
  return PGX_OK;
}

extern "C" int pgx_bd_get_stats(const pgx_bd* s, pgx_bd_stats* st) {
  if (!s || !st) return PGX_EINVAL;
  *st = s->stats;
  return PGX_OK;
}

extern "C" int pgx_bd_export_pivots(const pgx_bd* s, int32_t* piv) {
  if (!s || !piv) return PGX_EINVAL;
  std::memcpy(piv, s->piv.data(), (size_t)s->n * sizeof(int32_t));
  return PGX_OK;
}

extern "C" int pgx_bd_timing(pgx_bd* s, int enable, double* factor_ms, double* solve_ms) {
  if (!s) return PGX_EINVAL;
  if (factor_ms) *factor_ms = s->factor_ms;
  if (solve_ms) *solve_ms = s->solve_ms;
  s->timing = enable != 0;
  s->factor_ms = s->solve_ms = 0;
  return PGX_OK;
}

static inline unsigned bd_threads(int64_t rows) { return (unsigned)std::min<int64_t>(BD_NT, (std::max<int64_t>(rows, 1) + 63) / 64 * 64); }

extern "C" int pgx_bd_factor(pgx_bd* s, const double* vals, int on_device) {
  if (!s || (!vals && s->nnz)) return PGX_EINVAL;
  BDHIP(hipSetDevice(s->device));
  PgxRange range("pgx_bd:factor");
  s->factored = false;
  const int n = (int)s->n, kl = s->kl, kv = s->kv, ldab = s->ldab;
  const double* dv = vals;
  if (!on_device && s->nnz) {
    BDHIP(hipMemcpyAsync(s->d_vals, vals, (size_t)s->nnz * sizeof(double), hipMemcpyHostToDevice, s->st));
    dv = s->d_vals;
  }
  if (s->timing) hipEventRecord(s->e0, s->st);
  BDHIP(hipMemsetAsync(s->d_info, 0, sizeof(int32_t), s->st));
  BDHIP(hipMemsetAsync(s->ab, 0, (size_t)ldab * (size_t)n * sizeof(double), s->st));
  if (s->nnz) {
    const int blocks = (int)std::min<int64_t>((s->nnz + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(k_bd_scatter, dim3(blocks), dim3(256), 0, s->st, s->nnz, s->d_dest, dv, s->ab);
  }
  for (int j0 = 0; j0 < n; j0 += BD_NB) {
    const int w = std::min(BD_NB, n - j0);
    hipLaunchKernelGGL(k_bd_panel, dim3(1), dim3(bd_threads(std::min(kl + w, n - j0))), 0, s->st, s->ab, n, kl, kv, ldab, j0, w, s->d_piv,
                       s->d_diag, s->d_info);
    const int64_t right = std::min<int64_t>(n, (int64_t)j0 + BD_NB + kv) - (j0 + BD_NB);  // > 0 only behind a full panel
    if (right > 0)
      hipLaunchKernelGGL(k_bd_right, dim3((unsigned)((right + BD_CT - 1) / BD_CT)), dim3(bd_threads(std::min(kl + BD_NB, n - j0))), 0, s->st,
                         s->ab, n, kl, kv, ldab, j0, s->d_piv);
  }
  if (s->timing) hipEventRecord(s->e1, s->st);
  BDHIP(hipGetLastError());
  int32_t info = 0;
  BDHIP(hipMemcpyAsync(s->piv.data(), s->d_piv, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->st));
  BDHIP(hipMemcpyAsync(s->diag.data(), s->d_diag, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->st));
  BDHIP(hipMemcpyAsync(&info, s->d_info, sizeof(int32_t), hipMemcpyDeviceToHost, s->st));
  BDHIP(hipStreamSynchronize(s->st));
  if (s->timing) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) s->factor_ms += ms;
  }
  s->stats.interchanges = 0;
  s->stats.zero_pivots = info;
  double lo = INFINITY, hi = 0.0;
  for (int k = 0; k < n; ++k) {
    const int32_t p = s->piv[(size_t)k];
    if (p < k || p >= n || p > k + kl) {
      s->err = "pgx_bd_factor: pivot vector out of range (internal error)";
      return PGX_ESTATE;
    }
    if (p != k) ++s->stats.interchanges;
    const double d = std::fabs(s->diag[(size_t)k]);
    lo = std::min(lo, d), hi = std::max(hi, d);
  }
  s->stats.min_pivot = lo, s->stats.max_pivot = hi;
  if (info > 0) {
    s->err = "pgx_bd_factor: " + std::to_string(info) + " column(s) of the order-" + std::to_string(n) + " band matrix (kl = " +
             std::to_string(kl) + ", ku = " + std::to_string(s->ku) +
             ") without a nonzero pivot candidate: the matrix is singular; pgx_bd_solve refuses this factorisation";
    return PGX_ESTATE;
  }
  s->factored = true;
  s->err.clear();
  return PGX_OK;
}

extern "C" int pgx_bd_solve(pgx_bd* s, const double* b, double* x, int on_device) {
  if (!s || !b || !x) return PGX_EINVAL;
  if (!s->factored) {
    s->err = s->stats.zero_pivots > 0 ? "pgx_bd_solve: the last factorisation met " + std::to_string(s->stats.zero_pivots) +
                                            " zero pivot(s) (singular matrix); factorise a nonsingular matrix first"
                                      : std::string("pgx_bd_solve: no factorisation (call pgx_bd_factor first)");
    return PGX_ESTATE;
  }
  BDHIP(hipSetDevice(s->device));
  PgxRange range("pgx_bd:solve");
  const int n = (int)s->n;
  const double* db = b;
  double* dx = x;
  if (!on_device) {
    BDHIP(hipMemcpyAsync(s->d_io, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s->st));
    db = dx = s->d_io;
  }
  if (s->timing) hipEventRecord(s->e0, s->st);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(k_bd_gather, grid, dim3(256), 0, s->st, (int64_t)n, s->d_perm, db, s->d_w);
  hipLaunchKernelGGL(k_bd_fwd, dim3(1), dim3(bd_threads(std::min(s->kl + BD_NB, n))), 0, s->st, s->ab, n, s->kl, s->kv, s->ldab, s->d_piv, s->d_w);
  hipLaunchKernelGGL(k_bd_bwd, dim3(1), dim3(512), 0, s->st, s->ab, n, s->kv, s->ldab, s->d_w);
  hipLaunchKernelGGL(k_bd_spread, grid, dim3(256), 0, s->st, (int64_t)n, s->d_perm, s->d_w, dx);
  if (s->timing) hipEventRecord(s->e1, s->st);
  BDHIP(hipGetLastError());
  if (!on_device) {
    BDHIP(hipMemcpyAsync(x, s->d_io, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    BDHIP(hipStreamSynchronize(s->st));
  }
  if (s->timing) {
    float ms = 0;
    if (hipEventSynchronize(s->e1) == hipSuccess && hipEventElapsedTime(&ms, s->e0, s->e1) == hipSuccess) s->solve_ms += ms;
  }
  return PGX_OK;
}
