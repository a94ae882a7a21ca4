// Multigrid on general P1 meshes that come without a refinement hierarchy (include/pgx.h: pgx_build_hierarchy; DESIGN.md section 3,
// "Built hierarchies").  The hierarchy is built from the handle's own stiffness matrix: per transfer a coarse/fine split on the
// strength graph and a CSR prolongation P with general weights (direct interpolation, one Jacobi step on the interior F rows,
// truncation).  The split and every pattern are computed on the device by default (pgx_amg_build.hip); the host pass below, which did
// that work before, stays as the comparator behind the tuning key PGX_AMG_BUILD=0 and builds bitwise the same hierarchy.  The levels
// are the block-CSR levels of pgx_umg.hip and run its cycle (k_bspmv smoother and residual, k_umg_coarse).  This file holds the host
// pass and what the general weights need on the device:
//   k_amg_direct          values of the direct interpolation from the fine K
//   k_amg_pvalues         the Jacobi step on the interior F rows, truncation and rescale; other rows copy the direct values
//   k_amg_gather2         dst[e] = sum over the plan row of e of a[ia] * b[ib]: both stages of the Galerkin product, T = A P entry by
//                         entry and P^T T over child lists (K, M once; D on every Jacobian fill).  Plans hold indices only
//   k_amg_resid_restrict  b_c = P^T r over the child list of every coarse vertex, weights read from P's value array
//   k_amg_prolong_add     x_f += P c over the CSR rows of P
// Everything is fp64 gather work without atomics, every sum runs in list order: results are bitwise reproducible.  The two kernels that
// compute P keep products and sums unfused, so that they round as the numpy twin (tests/amg_reference.py) does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pgx_handle.h"

// One thread per fine row.  src[q] = the fine K entry (row, the C neighbour behind column q), -1 on a C row (one entry of 1).
__global__ void __launch_bounds__(PGX_BLOCK) k_amg_direct(int n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ src,
                                                          const double* __restrict__ K, double* __restrict__ val) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int s = ptr[i], e = ptr[i + 1];
  if (e == s + 1 && src[s] < 0) {
    val[s] = 1.0;
    return;
  }
  double tot = 0.0;
  for (int q = s; q < e; ++q) tot = tot + (-K[src[q]]);
  for (int q = s; q < e; ++q) val[q] = (-K[src[q]]) / tot;
}

// One thread per fine row over the row's entries of the untruncated pattern.  own[f] = the direct entry on the same column (-1: none).
// diag[i] = the fine K entry (i, i) of a row that takes the Jacobi step, -1 for a row that keeps its direct values.  A Jacobi row:
// v_f = own - (sum over the plan row of f of K[pa] * P0[pb]) / K_ii, items by ascending fine column; then entries below trunc times the
// row's largest magnitude become exact zeros (the host drops them from the pattern) and the others are scaled by (sum of all) / (sum of
// the kept ones).
__global__ void __launch_bounds__(PGX_BLOCK) k_amg_pvalues(int n, const int32_t* __restrict__ fptr, const int32_t* __restrict__ own,
                                                           const int32_t* __restrict__ pptr, const int32_t* __restrict__ pa,
                                                           const int32_t* __restrict__ pb, const int32_t* __restrict__ diag,
                                                           const double* __restrict__ K, const double* __restrict__ p0, double trunc,
                                                           double* __restrict__ val) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int s = fptr[i], e = fptr[i + 1];
  const int de = diag[i];
  if (de < 0) {
    for (int f = s; f < e; ++f) val[f] = p0[own[f]];
    return;
  }
  const double d = K[de];
  double top = 0.0;
  for (int f = s; f < e; ++f) {
    double acc = 0.0;
    const int pe = pptr[f + 1];
    for (int k = pptr[f]; k < pe; ++k) {
      const double prod = K[pa[k]] * p0[pb[k]];
      acc = acc + prod;
    }
    const double o = own[f] >= 0 ? p0[own[f]] : 0.0;
    const double v = o - acc / d;
    val[f] = v;
    top = fmax(top, fabs(v));
  }
  const double cut = trunc * top;
  double all = 0.0, kept = 0.0;
  for (int f = s; f < e; ++f) {
    const double v = val[f];
    all = all + v;
    if (fabs(v) >= cut) kept = kept + v;
  }
  const double scale = all / kept;
  for (int f = s; f < e; ++f) {
    const double v = val[f];
    val[f] = fabs(v) >= cut ? v * scale : 0.0;
  }
}

__global__ void __launch_bounds__(PGX_BLOCK) k_amg_gather2(int n_dst, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ia,
                                                           const int32_t* __restrict__ ib, const double* __restrict__ a,
                                                           const double* __restrict__ b, double* __restrict__ dst) {
  const int e = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (e >= n_dst) return;
  double acc = 0.0;
  const int end = ptr[e + 1];
  for (int k = ptr[e]; k < end; ++k) acc += a[ia[k]] * b[ib[k]];
  dst[e] = acc;
}

// One thread per coarse vertex: children by ascending fine index, child k through P entry ch_q[k].
__global__ void __launch_bounds__(PGX_BLOCK) k_amg_resid_restrict(int n_c, const int32_t* __restrict__ ch_ptr, const int32_t* __restrict__ ch_idx,
                                                                  const int32_t* __restrict__ ch_q, const double* __restrict__ pv,
                                                                  const uint8_t* __restrict__ mask_c, const double* __restrict__ ru,
                                                                  const double* __restrict__ rp, double* __restrict__ bu,
                                                                  double* __restrict__ bp) {
  const int v = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (v >= n_c) return;
  double su = 0.0, sp = 0.0;
  const int end = ch_ptr[v + 1];
  for (int k = ch_ptr[v]; k < end; ++k) {
    const int c = ch_idx[k];
    const double w = pv[ch_q[k]];
    su += w * ru[c];
    sp += w * rp[c];
  }
  bu[v] = mask_c[v] ? 0.0 : su;
  bp[v] = sp;
}

__global__ void __launch_bounds__(PGX_BLOCK) k_amg_prolong_add(int n_f, const int32_t* __restrict__ pptr, const int32_t* __restrict__ pcol,
                                                               const double* __restrict__ pv, const double* __restrict__ cu,
                                                               const double* __restrict__ cp, double* __restrict__ xu,
                                                               double* __restrict__ xp) {
  const int v = blockIdx.x * PGX_BLOCK + threadIdx.x;
  if (v >= n_f) return;
  double su = 0.0, sp = 0.0;
  const int end = pptr[v + 1];
  for (int q = pptr[v]; q < end; ++q) {
    const int c = pcol[q];
    const double w = pv[q];
    su += w * cu[c];
    sp += w * cp[c];
  }
  xu[v] += su;
  xp[v] += sp;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static inline dim3 amg_grid(int n) { return dim3((unsigned)std::max(1, (n + PGX_BLOCK - 1) / PGX_BLOCK)); }

// dst = P^T (src) P of the transfer onto level C, in two gather stages through C.T
void pgxk_amg_rap(hipStream_t st, const UmgLevel& C, const double* src, double* dst) {
  hipLaunchKernelGGL(k_amg_gather2, amg_grid(C.nnz_t), dim3(PGX_BLOCK), 0, st, C.nnz_t, C.t_ptr, C.t_a, C.t_p, src, C.P_val, C.T);
  hipLaunchKernelGGL(k_amg_gather2, amg_grid(C.nnz), dim3(PGX_BLOCK), 0, st, C.nnz, C.g_ptr, C.g_p, C.g_t, C.P_val, C.T, dst);
}

void pgxk_amg_resid_restrict(hipStream_t st, const UmgLevel& C, const double* ru, const double* rp) {
  hipLaunchKernelGGL(k_amg_resid_restrict, amg_grid(C.n), dim3(PGX_BLOCK), 0, st, C.n, C.ch_ptr, C.ch_idx, C.ch_q, C.P_val, C.mask, ru, rp,
                     C.bu, C.bp);
}

void pgxk_amg_prolong_add(hipStream_t st, int n_f, const UmgLevel& C, double* xu, double* xp) {
  hipLaunchKernelGGL(k_amg_prolong_add, amg_grid(n_f), dim3(PGX_BLOCK), 0, st, n_f, C.P_ptr, C.P_col, C.P_val, C.xu, C.xp, xu, xp);
}

void pgxk_amg_direct(hipStream_t st, int n, const int32_t* ptr, const int32_t* src, const double* K, double* val) {
  hipLaunchKernelGGL(k_amg_direct, amg_grid(n), dim3(PGX_BLOCK), 0, st, n, ptr, src, K, val);
}

void pgxk_amg_pvalues(hipStream_t st, int n, const int32_t* fptr, const int32_t* own, const int32_t* pptr, const int32_t* pa, const int32_t* pb,
                      const int32_t* diag, const double* K, const double* p0, double trunc, double* val) {
  hipLaunchKernelGGL(k_amg_pvalues, amg_grid(n), dim3(PGX_BLOCK), 0, st, n, fptr, own, pptr, pa, pb, diag, K, p0, trunc, val);
}

// ---- host pass -----------------------------------------------------------------------------------------------------------------
namespace {
struct DevTmp {  // device scratch of the setup, released when the transfer is done
  std::vector<void*> p;
  ~DevTmp() {
    for (void* q : p) (void)hipFree(q);
  }
  template <typename T>
  hipError_t put(hipStream_t st, T** dst, const std::vector<T>& src, size_t count = 0) {
    void* q = nullptr;
    const size_t n = std::max(count, src.size());
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p.push_back(q);
    *dst = (T*)q;
    if (!src.empty()) e = hipMemcpyAsync(q, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, st);
    return e;
  }
};

struct Trip {
  int32_t col, a, b;
};

// Groups the items of one row by column (stable: items of one column keep their order) into a CSR-of-lists: per distinct column one
// output entry with its item list.
void group_by_col(std::vector<Trip>& items, std::vector<int32_t>& out_col, std::vector<int32_t>& out_ptr, std::vector<int32_t>& ia,
                  std::vector<int32_t>& ib) {
  std::stable_sort(items.begin(), items.end(), [](const Trip& x, const Trip& y) { return x.col < y.col; });
  for (size_t k = 0; k < items.size(); ++k) {
    if (k == 0 || items[k].col != items[k - 1].col) {
      out_col.push_back(items[k].col);
      out_ptr.push_back((int32_t)ia.size());
    }
    ia.push_back(items[k].a);
    ib.push_back(items[k].b);
  }
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" int pgx_build_hierarchy(pgx_handle* h, double theta, double trunc, int32_t min_coarse, double max_keep, int32_t* n_levels,
                                   double* seconds) {
  NEED(h);
  if (!h->umg.empty()) {
    h->err = "pgx_build_hierarchy: this handle already has a hierarchy";
    return PGX_ESTATE;
  }
  if (h->jac_ever) {
    h->err = "pgx_build_hierarchy comes before the first Jacobian fill";
    return PGX_ESTATE;
  }
  if (h->structured || h->dist.on || h->lu_comm) {
    h->err = "pgx_build_hierarchy: for single handles on general meshes (structured meshes have their grid hierarchy; sharded and "
             "LU-distributed handles have none of this kind)";
    return PGX_EINVAL;
  }
  if (theta < 0.0) theta = PGX_AMG_THETA;
  if (trunc < 0.0) trunc = PGX_AMG_TRUNC;
  if (min_coarse <= 0) min_coarse = PGX_AMG_MIN_COARSE;
  if (max_keep <= 0.0) max_keep = PGX_AMG_MAX_KEEP;
  // trunc > 0: a truncated entry is marked by the value 0 (k_amg_pvalues), so an entry that comes out as an exact 0 - e.g. a column
  // reached only through K entries that are exact zeros - goes with them, here as in the twin
  if (!(theta <= 1.0) || !(trunc > 0.0 && trunc < 1.0) || !(max_keep < 1.0)) {
    h->err = "pgx_build_hierarchy: theta in [0, 1], trunc in (0, 1), max_keep in (0, 1) (negative; for min_coarse and max_keep also 0: the default)";
    return PGX_EINVAL;
  }
  if (h->n <= min_coarse) {
    h->err = "pgx_build_hierarchy: the mesh has no more than min_coarse vertices, there is nothing to coarsen";
    return PGX_EINVAL;
  }
  if (h->amg_build) return pgx_amg_build_device(h, theta, trunc, min_coarse, max_keep, n_levels, seconds);  // pgx_amg_build.hip
  double t_host = 0.0, t_dev = 0.0;
  std::vector<UmgLevel> lv(1);
  {
    const int rc = umg_level0(h, lv[0]);
    if (rc) return rc;
  }
  std::vector<double> Kh;  // host copy of the current level's K
  for (;;) {
    const int l = (int)lv.size() - 1;
    const int nf = lv[l].n;
    if (nf <= min_coarse) break;
    lv.reserve(lv.size() + 1);  // the references into lv[l] below outlive the emplace_back of the coarse level
    auto t0 = std::chrono::steady_clock::now();
    Kh.resize(lv[l].nnz);
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipMemcpy(Kh.data(), lv[l].K, sizeof(double) * Kh.size(), hipMemcpyDeviceToHost));
    t_dev += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    const std::vector<int32_t>& rp = lv[l].h_rowptr;
    const std::vector<int32_t>& cj = lv[l].h_col;
    const std::vector<uint8_t>& mk = lv[l].h_mask;
    const int nnz = lv[l].nnz;
    // strength, symmetrised: strong[e] for the entry (i, j) if it is strong seen from i or from j
    std::vector<uint8_t> own_strong(nnz, 0), strong(nnz, 0);
    for (int i = 0; i < nf; ++i) {
      double top = 0.0;
      for (int e = rp[i]; e < rp[i + 1]; ++e)
        if (cj[e] != i && -Kh[e] > top) top = -Kh[e];
      for (int e = rp[i]; e < rp[i + 1]; ++e) {
        const double neg = cj[e] != i ? -Kh[e] : 0.0;
        own_strong[e] = neg > 0.0 && neg >= theta * top;
      }
    }
    for (int i = 0; i < nf; ++i)
      for (int e = rp[i]; e < rp[i + 1]; ++e) {
        const int j = cj[e];
        if (j == i) continue;
        uint8_t s = own_strong[e];
        if (!s) {
          const int32_t* b = cj.data() + rp[j];
          const int32_t* en = cj.data() + rp[j + 1];
          const int32_t* it = std::lower_bound(b, en, i);
          if (it != en && *it == i) s = own_strong[it - cj.data()];
        }
        strong[e] = s;
      }
    // C/F split: Dirichlet vertices first, then interior ones, each in ascending index, over strong edges between vertices of one kind
    std::vector<uint8_t> state(nf, 0);  // 0 undecided, 1 C, 2 F
    for (int kind = 1; kind >= 0; --kind)
      for (int v = 0; v < nf; ++v) {
        if ((mk[v] != 0) != (kind != 0) || state[v]) continue;
        state[v] = 1;
        for (int e = rp[v]; e < rp[v + 1]; ++e) {
          const int j = cj[e];
          if (strong[e] && (mk[j] != 0) == (kind != 0) && !state[j]) state[j] = 2;
        }
      }
    std::vector<int32_t> cnum(nf, -1);
    int nc = 0;
    for (int v = 0; v < nf; ++v)
      if (state[v] == 1) cnum[v] = nc++;
    if ((double)nc > max_keep * (double)nf) break;  // the step would keep too many vertices: the level above stays the coarsest
    // direct interpolation: pattern and the fine entry behind every weight
    std::vector<int32_t> p0_ptr(nf + 1, 0), p0_col, p0_src;
    for (int i = 0; i < nf; ++i) {
      if (state[i] == 1) {
        p0_col.push_back(cnum[i]);
        p0_src.push_back(-1);
      } else {
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
          const int j = cj[e];
          if (strong[e] && state[j] == 1 && (!mk[i] || mk[j])) {
            p0_col.push_back(cnum[j]);
            p0_src.push_back(e);
          }
        }
        if ((int)p0_col.size() == p0_ptr[i]) {
          h->err = "pgx_build_hierarchy: an F vertex without a C neighbour (level " + std::to_string(l) + ", vertex " + std::to_string(i) + ")";
          return PGX_EINVAL;
        }
      }
      p0_ptr[i + 1] = (int32_t)p0_col.size();
    }
    // the untruncated pattern: interior F rows take the Jacobi step over their whole K row
    std::vector<int32_t> f_ptr(nf + 1, 0), f_col, f_own, f_pptr, pa, pb, diag(nf, -1);
    std::vector<Trip> items;
    for (int i = 0; i < nf; ++i) {
      if (state[i] == 1 || mk[i]) {
        for (int q = p0_ptr[i]; q < p0_ptr[i + 1]; ++q) {
          f_col.push_back(p0_col[q]);
          f_own.push_back(q);
          f_pptr.push_back((int32_t)pa.size());
        }
      } else {
        items.clear();
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
          const int k = cj[e];
          if (k == i) diag[i] = e;
          for (int q = p0_ptr[k]; q < p0_ptr[k + 1]; ++q) items.push_back(Trip{p0_col[q], e, q});
        }
        if (diag[i] < 0) {
          h->err = "pgx_build_hierarchy: a row without its diagonal entry";
          return PGX_EINVAL;
        }
        const size_t first = f_col.size();
        group_by_col(items, f_col, f_pptr, pa, pb);
        f_own.resize(f_col.size(), -1);
        int q = p0_ptr[i];
        for (size_t f = first; f < f_col.size(); ++f)  // both lists ascend by column, the row's own columns are among the union
          if (q < p0_ptr[i + 1] && p0_col[q] == f_col[f]) f_own[f] = q++;
      }
      f_ptr[i + 1] = (int32_t)f_col.size();
      if (pa.size() >= ((size_t)1 << 31)) {
        h->err = "pgx_build_hierarchy: interpolation plan exceeds int32";
        return PGX_EINVAL;
      }
    }
    f_pptr.push_back((int32_t)pa.size());
    t_host += seconds_since(t0);
    // values of P on the device
    t0 = std::chrono::steady_clock::now();
    std::vector<double> f_val(f_col.size());
    {
      DevTmp tmp;
      int32_t *d_p0_ptr, *d_p0_src, *d_f_ptr, *d_f_own, *d_f_pptr, *d_pa, *d_pb, *d_diag;
      double *d_p0_val, *d_f_val;
      const std::vector<double> none;
      HIPCHK(tmp.put(h->st, &d_p0_ptr, p0_ptr));
      HIPCHK(tmp.put(h->st, &d_p0_src, p0_src));
      HIPCHK(tmp.put(h->st, &d_f_ptr, f_ptr));
      HIPCHK(tmp.put(h->st, &d_f_own, f_own));
      HIPCHK(tmp.put(h->st, &d_f_pptr, f_pptr));
      HIPCHK(tmp.put(h->st, &d_pa, pa));
      HIPCHK(tmp.put(h->st, &d_pb, pb));
      HIPCHK(tmp.put(h->st, &d_diag, diag));
      HIPCHK(tmp.put(h->st, &d_p0_val, none, p0_col.size()));
      HIPCHK(tmp.put(h->st, &d_f_val, none, f_col.size()));
      hipLaunchKernelGGL(k_amg_direct, amg_grid(nf), dim3(PGX_BLOCK), 0, h->st, nf, d_p0_ptr, d_p0_src, lv[l].K, d_p0_val);
      hipLaunchKernelGGL(k_amg_pvalues, amg_grid(nf), dim3(PGX_BLOCK), 0, h->st, nf, d_f_ptr, d_f_own, d_f_pptr, d_pa, d_pb, d_diag, lv[l].K,
                         d_p0_val, trunc, d_f_val);
      HIPCHK(hipStreamSynchronize(h->st));
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpy(f_val.data(), d_f_val, sizeof(double) * f_val.size(), hipMemcpyDeviceToHost));
    }
    t_dev += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    lv.emplace_back();
    const UmgLevel& F = lv[l];
    UmgLevel& C = lv[l + 1];
    C.n = nc;
    // P = the entries that survived the truncation
    std::vector<double> P_val;
    C.h_P_ptr.assign(nf + 1, 0);
    for (int i = 0; i < nf; ++i) {
      for (int f = f_ptr[i]; f < f_ptr[i + 1]; ++f)
        if (f_val[f] != 0.0) {
          C.h_P_col.push_back(f_col[f]);
          P_val.push_back(f_val[f]);
        }
      C.h_P_ptr[i + 1] = (int32_t)C.h_P_col.size();
    }
    C.nnz_p = (int)C.h_P_col.size();
    const std::vector<int32_t>&Pp = C.h_P_ptr, &Pc = C.h_P_col;
    // child lists = P^T as CSR, children by ascending fine index
    std::vector<int32_t> ch_ptr(nc + 1, 0), ch_idx(C.nnz_p), ch_q(C.nnz_p);
    for (int q = 0; q < C.nnz_p; ++q) ++ch_ptr[Pc[q] + 1];
    for (int I = 0; I < nc; ++I) ch_ptr[I + 1] += ch_ptr[I];
    {
      std::vector<int32_t> pos(ch_ptr.begin(), ch_ptr.end() - 1);
      for (int i = 0; i < nf; ++i)
        for (int q = Pp[i]; q < Pp[i + 1]; ++q) {
          const int k = pos[Pc[q]]++;
          ch_idx[k] = i;
          ch_q[k] = q;
        }
    }
    // stage 1: T = A P row by row; per entry of T the pairs (fine entry, P entry), by ascending fine column
    std::vector<int32_t> t_rowptr(nf + 1, 0), t_col, t_ptr, t_a, t_p;
    for (int i = 0; i < nf; ++i) {
      items.clear();
      for (int e = rp[i]; e < rp[i + 1]; ++e)
        for (int q = Pp[cj[e]]; q < Pp[cj[e] + 1]; ++q) items.push_back(Trip{Pc[q], e, q});
      group_by_col(items, t_col, t_ptr, t_a, t_p);
      t_rowptr[i + 1] = (int32_t)t_col.size();
      if (t_a.size() >= ((size_t)1 << 31)) {
        h->err = "pgx_build_hierarchy: Galerkin plan exceeds int32";
        return PGX_EINVAL;
      }
    }
    t_ptr.push_back((int32_t)t_a.size());
    C.nnz_t = (int)t_col.size();
    // stage 2: P^T T over the child lists; per coarse entry the pairs (P entry, T entry), by ascending fine row
    std::vector<int32_t> g_ptr, g_p, g_t;
    C.h_rowptr.assign(nc + 1, 0);
    for (int I = 0; I < nc; ++I) {
      items.clear();
      for (int k = ch_ptr[I]; k < ch_ptr[I + 1]; ++k)
        for (int t = t_rowptr[ch_idx[k]]; t < t_rowptr[ch_idx[k] + 1]; ++t) items.push_back(Trip{t_col[t], ch_q[k], t});
      group_by_col(items, C.h_col, g_ptr, g_p, g_t);
      C.h_rowptr[I + 1] = (int32_t)C.h_col.size();
      if (g_p.size() >= ((size_t)1 << 31)) {
        h->err = "pgx_build_hierarchy: Galerkin plan exceeds int32";
        return PGX_EINVAL;
      }
    }
    g_ptr.push_back((int32_t)g_p.size());
    C.nnz = (int)C.h_col.size();
    C.h_mask.resize(nc);
    for (int v = 0; v < nf; ++v)
      if (state[v] == 1) C.h_mask[cnum[v]] = mk[v];
    std::vector<int32_t> colm(C.nnz);
    for (int e = 0; e < C.nnz; ++e) colm[e] = (int32_t)((uint32_t)C.h_col[e] | (C.h_mask[C.h_col[e]] ? 0x80000000u : 0u));
    t_host += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    int rc;
    if ((rc = umg_upload(h, &C.rowptr, C.h_rowptr)) || (rc = umg_upload(h, &C.colm, colm)) || (rc = umg_upload(h, &C.mask, C.h_mask)) ||
        (rc = umg_upload(h, &C.P_ptr, C.h_P_ptr)) || (rc = umg_upload(h, &C.P_col, C.h_P_col)) || (rc = umg_upload(h, &C.P_val, P_val)) ||
        (rc = umg_upload(h, &C.ch_ptr, ch_ptr)) || (rc = umg_upload(h, &C.ch_idx, ch_idx)) || (rc = umg_upload(h, &C.ch_q, ch_q)) ||
        (rc = umg_upload(h, &C.t_ptr, t_ptr)) || (rc = umg_upload(h, &C.t_a, t_a)) || (rc = umg_upload(h, &C.t_p, t_p)) ||
        (rc = umg_upload(h, &C.g_ptr, g_ptr)) || (rc = umg_upload(h, &C.g_p, g_p)) || (rc = umg_upload(h, &C.g_t, g_t)))
      return rc;
    DALLOC(C.T, C.nnz_t);
    DALLOC(C.K, C.nnz);
    DALLOC(C.M, C.nnz);
    DALLOC(C.D, C.nnz);
    double** const vecs[8] = {&C.bu, &C.bp, &C.xu, &C.xp, &C.xu2, &C.xp2, &C.ru, &C.rp};
    for (double** v : vecs) DALLOC(*v, nc);
    pgxk_amg_rap(h->st, C, F.K, C.K);  // the next split reads this level's K
    pgxk_amg_rap(h->st, C, F.M, C.M);
    HIPCHK(hipStreamSynchronize(h->st));  // the uploads read host vectors that end with this iteration
    HIPCHK(hipGetLastError());
    t_dev += seconds_since(t0);
  }
  if (lv.size() < 2) {
    h->err = "pgx_build_hierarchy: the first coarsening step keeps more than max_keep of the vertices, no hierarchy was built";
    return PGX_EINVAL;
  }
  umg_install(h, std::move(lv));
  h->amg_mode = 0;
  h->amg_split.assign(h->umg.size() - 1, 0);  // the host's split is one serial sweep, no launches
  if (n_levels) *n_levels = (int32_t)h->umg.size();
  if (seconds) {
    seconds[0] = t_host;
    seconds[1] = t_dev;
  }
  return PGX_OK;
}

extern "C" int pgx_amg_build_info(pgx_handle* h, int32_t* mode, int32_t* n_transfers, int32_t* split_launches) {
  NEED(h);
  if (h->amg_mode < 0 || h->umg.size() < 2) {
    h->err = "pgx_amg_build_info needs a handle with a built hierarchy (pgx_build_hierarchy)";
    return PGX_ESTATE;
  }
  if (mode) *mode = h->amg_mode;
  if (n_transfers) *n_transfers = (int32_t)h->amg_split.size();
  if (split_launches) memcpy(split_launches, h->amg_split.data(), sizeof(int32_t) * h->amg_split.size());
  return PGX_OK;
}

extern "C" int pgx_build_hierarchy_default(const pgx_handle* h, int pc_type) {
  if (!h || h->structured || h->dist.on || h->lu_comm || !h->umg.empty() || h->jac_ever) return 0;
  // pc_type auto (0) keeps the sparse LU on such meshes: the size from which the built cycle beats it has not been located
  return pc_type == 1 && h->n >= h->umg_build_min && h->n > PGX_AMG_MIN_COARSE;
}

extern "C" int pgx_umg_transfer_export(pgx_handle* h, int t, int32_t* n_fine, int32_t* n_coarse, int32_t* nnz, int32_t* rowptr, int32_t* col,
                                       double* val) {
  NEED(h);
  if (h->umg.size() < 2 || !h->umg[1].P_val) {
    h->err = "pgx_umg_transfer_export needs a handle with a built hierarchy (pgx_build_hierarchy)";
    return PGX_ESTATE;
  }
  if (t < 0 || t + 1 >= (int)h->umg.size()) {
    h->err = "pgx_umg_transfer_export: no such transfer";
    return PGX_EINVAL;
  }
  const UmgLevel& C = h->umg[t + 1];
  if (n_fine) *n_fine = h->umg[t].n;
  if (n_coarse) *n_coarse = C.n;
  if (nnz) *nnz = C.nnz_p;
  if (rowptr) memcpy(rowptr, C.h_P_ptr.data(), sizeof(int32_t) * C.h_P_ptr.size());
  if (col) memcpy(col, C.h_P_col.data(), sizeof(int32_t) * C.nnz_p);
  if (val) {
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipMemcpy(val, C.P_val, sizeof(double) * C.nnz_p, hipMemcpyDeviceToHost));
  }
  return PGX_OK;
}
