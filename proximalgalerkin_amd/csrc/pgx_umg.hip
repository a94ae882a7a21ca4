// Multigrid on refined unstructured P1 meshes (include/pgx.h: pgx_set_hierarchy; DESIGN.md section 3, "Refined general meshes").
// The hierarchy is given by topology alone: per transfer one `parents` array [n_fine][2], (v, v) for a vertex the coarse mesh has
// too, the two ends of the bisected edge for a midpoint.  P has two entries of 1/2 per row (on the same column for an inherited
// vertex).  Every level stores the block CSR of k_bspmv (pgx_kernels.hip), which is also its smoother and its residual; this file
// holds what the transfers and the coarsest level need:
//   k_umg_rap             coarse values = P^T (fine values) P by a precomputed gather plan (K, M once; D on every Jacobian fill)
//   k_umg_resid_restrict  b_c = P^T r, gathered over each coarse vertex's child list; r = b - J x was written by k_bspmv<1>
//   k_umg_prolong_add     x_f += 1/2 (c[p0] + c[p1])
//   k_umg_coarse          all sweeps of the coarsest level in one launch of one workgroup, operator and vectors in LDS
// Everything is fp64 gather work without atomics: every sum has one fixed order, results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pgx_internal.h"

// One plan item = index of a fine entry | s << 30, its weight is 2^-s (s = number of midpoints among the fine entry's row and column).
#define PGX_UMG_SRC_MASK 0x3fffffff

// LPE lanes per coarse entry: lane k sums the plan items k, k + LPE, ... of its entry in list order, then a butterfly over the lanes.
template <int LPE>
__global__ void __launch_bounds__(PGX_BLOCK) k_umg_rap(int nnz_c, const int32_t* __restrict__ plan_ptr, const int32_t* __restrict__ plan_src,
                                                       const double* __restrict__ src, double* __restrict__ dst) {
  const int t = blockIdx.x * PGX_BLOCK + threadIdx.x;
  const int e = t / LPE, lane = t % LPE;
  int s = 0, end = 0;
  if (e < nnz_c) {
    s = plan_ptr[e];
    end = plan_ptr[e + 1];
  }
  double acc = 0.0;
  for (int k = s + lane; k < end; k += LPE) {
    const int p = plan_src[k];
    const int sh = (p >> 30) & 3;
    const double w = sh == 0 ? 1.0 : (sh == 1 ? 0.5 : 0.25);
    acc += w * src[p & PGX_UMG_SRC_MASK];
  }
#pragma unroll
  for (int o = LPE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, LPE);
  if (e < nnz_c && lane == 0) dst[e] = acc;
}

// One thread per coarse vertex: its own fine twin (weight 1) and the midpoints of its edges (weight 1/2), in list order.
__global__ void __launch_bounds__(PGX_BLOCK) k_umg_resid_restrict(int n_c, const int32_t* __restrict__ ch_ptr, const int32_t* __restrict__ ch_idx,
                                                                  const uint8_t* __restrict__ mask_c, const double* __restrict__ ru,
                                                                  const double* __restrict__ rp, double* __restrict__ bu,
                                                                  double* __restrict__ bp) {
  const int v = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (v >= n_c) return;
  double su = 0.0, sp = 0.0;
  const int end = ch_ptr[v + 1];
  for (int k = ch_ptr[v]; k < end; ++k) {
    const int c = ch_idx[k];
    const double w = c == v ? 1.0 : 0.5;
    su += w * ru[c];
    sp += w * rp[c];
  }
  bu[v] = mask_c[v] ? 0.0 : su;
  bp[v] = sp;
}

__global__ void __launch_bounds__(PGX_BLOCK) k_umg_prolong_add(int n_f, const int32_t* __restrict__ parents, const double* __restrict__ cu,
                                                               const double* __restrict__ cp, double* __restrict__ xu,
                                                               double* __restrict__ xp) {
  const int v = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (v >= n_f) return;
  const int2 p = reinterpret_cast<const int2*>(parents)[v];
  xu[v] += 0.5 * (cu[p.x] + cu[p.y]);
  xp[v] += 0.5 * (cp[p.x] + cp[p.y]);
}

// The coarsest level: `sweeps` collective-Jacobi sweeps from a zero guess, one row per thread and pass, the arithmetic of k_bspmv<2>
// row by row (sums in entry order instead of over 8 lanes).  LDS: three value arrays, column words, row pointers, b and two iterates.
#define PGX_UMG_COARSE_THREADS 1024
__global__ void __launch_bounds__(PGX_UMG_COARSE_THREADS) k_umg_coarse(int n, int nnz, const int32_t* __restrict__ rowptr,
                                                                       const int32_t* __restrict__ colm, const double* __restrict__ K,
                                                                       const double* __restrict__ M, const double* __restrict__ D, double alpha,
                                                                       double omega, int sweeps, const double* __restrict__ bu,
                                                                       const double* __restrict__ bp, double* __restrict__ xu,
                                                                       double* __restrict__ xp) {
  extern __shared__ double umg_sm[];
  double* const sK = umg_sm;
  double* const sM = sK + nnz;
  double* const sD = sM + nnz;
  double* const sbu = sD + nnz;
  double* const sbp = sbu + n;
  double* cu = sbp + n;
  double* cp = cu + n;
  double* ou = cp + n;
  double* op = ou + n;
  int32_t* const srp = reinterpret_cast<int32_t*>(op + n);
  int32_t* const scm = srp + (n + 1);
  const int tid = threadIdx.x;
  for (int k = tid; k < nnz; k += PGX_UMG_COARSE_THREADS) {
    sK[k] = K[k];
    sM[k] = M[k];
    sD[k] = D[k];
    scm[k] = colm[k];
  }
  for (int i = tid; i < n; i += PGX_UMG_COARSE_THREADS) {
    sbu[i] = bu[i];
    sbp[i] = bp[i];
    cu[i] = 0.0;
    cp[i] = 0.0;
  }
  for (int i = tid; i <= n; i += PGX_UMG_COARSE_THREADS) srp[i] = rowptr[i];
  __syncthreads();
  for (int s = 0; s < sweeps; ++s) {
    for (int row = tid; row < n; row += PGX_UMG_COARSE_THREADS) {
      double au = 0.0, ap = 0.0, da = 0.0, dm = 0.0, dd = 0.0;
      int rowbc = 0;
      const int end = srp[row + 1];
      for (int k = srp[row]; k < end; ++k) {
        const int cm = scm[k];
        const int c = cm & 0x7fffffff;
        const double kv = sK[k], mv = sM[k], dv = sD[k];
        if (c == row) {
          rowbc = cm < 0;
          da = alpha * kv;
          dm = mv;
          dd = dv;
        }
        const double xuv = (cm < 0) ? 0.0 : cu[c];
        const double xpv = cp[c];
        au += alpha * kv * xuv + mv * xpv;
        ap += mv * xuv - dv * xpv;
      }
      const double xur = cu[row], xpr = cp[row];
      if (rowbc) au = xur;
      const double su = sbu[row] - au, sp = sbp[row] - ap;
      double a = da, b = dm, om_u = omega;
      if (rowbc) {
        a = 1.0;
        b = 0.0;
        om_u = 1.0;
      }
      const double det = -a * dd - b * b;
      double du = 0.0, dpsi = 0.0;
      if (det != 0.0) {
        du = (-dd * su - b * sp) / det;
        dpsi = (-b * su + a * sp) / det;
      } else if (rowbc) {
        du = su;
      }
      ou[row] = xur + om_u * du;
      op[row] = xpr + omega * dpsi;
    }
    __syncthreads();
    double* t = cu;
    cu = ou;
    ou = t;
    t = cp;
    cp = op;
    op = t;
  }
  for (int i = tid; i < n; i += PGX_UMG_COARSE_THREADS) {
    xu[i] = cu[i];
    xp[i] = cp[i];
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
void pgxk_umg_rap(hipStream_t st, int nnz_c, int lpe, const int32_t* plan_ptr, const int32_t* plan_src, const double* src, double* dst) {
  const size_t threads = (size_t)nnz_c * lpe;
  dim3 grid((unsigned)((threads + PGX_BLOCK - 1) / PGX_BLOCK)), block(PGX_BLOCK);
  if (lpe == 8)
    hipLaunchKernelGGL(k_umg_rap<8>, grid, block, 0, st, nnz_c, plan_ptr, plan_src, src, dst);
  else
    hipLaunchKernelGGL(k_umg_rap<4>, grid, block, 0, st, nnz_c, plan_ptr, plan_src, src, dst);
}

void pgxk_umg_resid_restrict(hipStream_t st, int n_c, const int32_t* ch_ptr, const int32_t* ch_idx, const uint8_t* mask_c, const double* ru,
                             const double* rp, double* bu, double* bp) {
  hipLaunchKernelGGL(k_umg_resid_restrict, dim3((n_c + PGX_BLOCK - 1) / PGX_BLOCK), dim3(PGX_BLOCK), 0, st, n_c, ch_ptr, ch_idx, mask_c, ru,
                     rp, bu, bp);
}

void pgxk_umg_prolong_add(hipStream_t st, int n_f, const int32_t* parents, const double* cu, const double* cp, double* xu, double* xp) {
  hipLaunchKernelGGL(k_umg_prolong_add, dim3((n_f + PGX_BLOCK - 1) / PGX_BLOCK), dim3(PGX_BLOCK), 0, st, n_f, parents, cu, cp, xu, xp);
}

size_t pgxk_umg_coarse_lds(int n, int nnz) {
  return sizeof(double) * (3 * (size_t)nnz + 6 * (size_t)n) + sizeof(int32_t) * ((size_t)nnz + (size_t)n + 1);
}

// The dynamic-LDS limit of k_umg_coarse on the CURRENT device (hipFuncSetAttribute is per device): called once per handle, by
// pgx_set_hierarchy, on the handle's device.  false: the level does not fit, or the device refused - the caller sweeps with k_bspmv.
bool pgxk_umg_coarse_prepare(int n, int nnz) {
  if (pgxk_umg_coarse_lds(n, nnz) > PGX_UMG_COARSE_LDS_MAX) return false;
  if (hipFuncSetAttribute((const void*)k_umg_coarse, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PGX_UMG_COARSE_LDS_MAX) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

void pgxk_umg_coarse(hipStream_t st, int n, int nnz, const int32_t* rowptr, const int32_t* colm, const double* K, const double* M,
                     const double* D, double alpha, double omega, int sweeps, const double* bu, const double* bp, double* xu, double* xp) {
  hipLaunchKernelGGL(k_umg_coarse, dim3(1), dim3(PGX_UMG_COARSE_THREADS), pgxk_umg_coarse_lds(n, nnz), st, n, nnz, rowptr, colm, K, M, D,
                     alpha, omega, sweeps, bu, bp, xu, xp);
}
