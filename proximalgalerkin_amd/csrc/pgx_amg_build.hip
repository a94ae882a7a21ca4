// The device pass of pgx_build_hierarchy (pgx_amg.hip holds the rule, the value kernels and the host pass this one is compared with;
// DESIGN.md section 3, "Built hierarchies").  Everything the host pass computes per transfer - strength graph, C/F split, numbering,
// the direct and Jacobi patterns, the compaction of P, child lists and both Galerkin plans - is computed here on the device, into the
// same arrays, entry for entry: the split is the host's, the patterns are the host's, every plan row lists its items in the host's
// order.  K is not downloaded; the host reads one small record (AbInfo) at the points where it needs a size to allocate the next
// arrays, and downloads the mirrors of a finished level once.
//   k_ab_strength_own / _sym   own_strong and the symmetrised flag per entry of K (columns sorted: binary search for (j, i))
//   k_ab_split                 the greedy split in its parallel form: a vertex becomes F once a lower-numbered strong neighbour of its
//                              kind is C, and C once all of them are F.  Decisions are final and rest on final decisions only, so every
//                              schedule ends in the host's split.  A block sweeps its 256 vertices until none of them moves; a vertex
//                              that waits for another block is left for the next launch.  Nothing waits inside a launch
//   k_ab_scan_sums / _apply    exclusive scan in tiles of 256: tile sums (int64), scan of the sums (the same two kernels, recursively),
//                              add back.  Totals are int64, so a plan beyond int32 is seen as such and refused
//   k_ab_p0_*, k_ab_jac_*, k_ab_nz_*, k_ab_child_*, k_ab_plan_*   the patterns, each as count -> scan -> fill: direct interpolation,
//                              untruncated Jacobi rows, the non-zero entries of P, child lists (placed by integer atomics, then sorted
//                              by fine index per list), and both stages of the Galerkin plan through one kernel pair
// One thread per row throughout.  A plan row is a merge of a few column-sorted lists (the P0 / P rows behind the entries of a K row,
// the T rows of the children of a coarse vertex); ab_merge_row walks the distinct columns in ascending order and, per column, the
// lists in their order - which is the order the host's stable sort leaves.  It keeps no per-list cursor (a binary search per list
// and column instead), so no row length is too long for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "pgx_handle.h"

#define AB_TILE 256  // threads per block = elements per scan tile

struct AbInfo {
  long long tot[2];  // totals of the last one or two scans
  int bad_vertex;    // smallest F vertex without a C neighbour (INT_MAX: none)
  int no_diag;       // a Jacobi row without its diagonal entry
  int decided;       // vertices the split has decided so far
  int pad;
};

__device__ __forceinline__ int ab_col(int32_t cm) { return (int)(cm & 0x7fffffff); }

__global__ void __launch_bounds__(AB_TILE) k_ab_strength_own(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                            const double* __restrict__ K, double theta, uint8_t* __restrict__ own) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  const int s = rowptr[i], e = rowptr[i + 1];
  double top = 0.0;
  for (int q = s; q < e; ++q)
    if (ab_col(colm[q]) != i && -K[q] > top) top = -K[q];
  const double bar = theta * top;
  for (int q = s; q < e; ++q) {
    const double neg = ab_col(colm[q]) != i ? -K[q] : 0.0;
    own[q] = neg > 0.0 && neg >= bar;
  }
}

__global__ void __launch_bounds__(AB_TILE) k_ab_strength_sym(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                            const uint8_t* __restrict__ own, uint8_t* __restrict__ strong) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  const int s = rowptr[i], e = rowptr[i + 1];
  for (int q = s; q < e; ++q) {
    const int j = ab_col(colm[q]);
    uint8_t f = 0;
    if (j != i) {
      f = own[q];
      if (!f) {
        int lo = rowptr[j];
        const int end = rowptr[j + 1];
        int hi = end;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (ab_col(colm[mid]) < i) lo = mid + 1;
          else hi = mid;
        }
        if (lo < end && ab_col(colm[lo]) == i) f = own[lo];
      }
    }
    strong[q] = f;
  }
}

// state: 0 undecided, 1 C, 2 F.  Updated in place with relaxed loads and stores: whichever value a neighbour shows, it is either
// "undecided" or final.
__global__ void __launch_bounds__(AB_TILE) k_ab_split(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                     const uint8_t* __restrict__ mask, const uint8_t* __restrict__ strong, int* state,
                                                     AbInfo* info) {
  const int v = blockIdx.x * AB_TILE + threadIdx.x;
  bool active = v < n && __hip_atomic_load(&state[v < n ? v : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
  const bool kind = active && mask[v] != 0;
  const int s = active ? rowptr[v] : 0, e = active ? rowptr[v + 1] : 0;
  int newly = 0;
  for (;;) {
    int moved = 0;
    if (active) {
      bool all_f = true, any_c = false;
      for (int q = s; q < e; ++q) {
        const int j = ab_col(colm[q]);
        if (!strong[q] || j >= v || (mask[j] != 0) != kind) continue;
        const int sj = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sj == 1) {
          any_c = true;
          break;
        }
        if (sj == 0) all_f = false;
      }
      if (any_c || all_f) {
        __hip_atomic_store(&state[v], any_c ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        active = false;
        moved = newly = 1;
      }
    }
    if (!__syncthreads_or(moved)) break;
  }
  const int cnt = __syncthreads_count(newly);
  if (threadIdx.x == 0 && cnt) atomicAdd(&info->decided, cnt);
}

__global__ void __launch_bounds__(AB_TILE) k_ab_flag_c(int n, const int* __restrict__ state, int32_t* __restrict__ flag) {
  const int v = blockIdx.x * AB_TILE + threadIdx.x;
  if (v < n) flag[v] = state[v] == 1;
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------
template <typename Tin>
__global__ void __launch_bounds__(AB_TILE) k_ab_scan_sums(long long n, const Tin* __restrict__ in, long long* __restrict__ sums) {
  __shared__ long long sh[AB_TILE];
  const long long i = (long long)blockIdx.x * AB_TILE + threadIdx.x;
  sh[threadIdx.x] = i < n ? (long long)in[i] : 0;
  __syncthreads();
  for (int w = AB_TILE / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

// out[i] = offs[tile] + (sum of the tile's elements before i), out[n] = the total (also into *total when given).  offs == nullptr: one
// tile.  n == 0: out[0] = 0.
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(AB_TILE) k_ab_scan_apply(long long n, const Tin* __restrict__ in, const long long* __restrict__ offs,
                                                          Tout* __restrict__ out, long long* __restrict__ total) {
  __shared__ long long sh[AB_TILE];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * AB_TILE + t;
  const long long mine = i < n ? (long long)in[i] : 0;
  sh[t] = mine;
  __syncthreads();
  for (int w = 1; w < AB_TILE; w <<= 1) {
    const long long add = t >= w ? sh[t - w] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const long long base = offs ? offs[blockIdx.x] : 0;
  const long long incl = base + sh[t];
  if (i < n) out[i] = (Tout)(incl - mine);
  if (i == n - 1 || (n == 0 && i == 0)) {
    out[n] = (Tout)incl;
    if (total) *total = incl;
  }
}

namespace {
struct DevTmp {  // device scratch of one transfer
  std::vector<void*> p;
  ~DevTmp() {
    for (void* q : p) (void)hipFree(q);
  }
  template <typename T>
  hipError_t get(T** dst, size_t count) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p.push_back(q);
    *dst = (T*)q;
    return hipSuccess;
  }
};

inline dim3 ab_grid(long long n) { return dim3((unsigned)std::max<long long>(1, (n + AB_TILE - 1) / AB_TILE)); }

// words of int64 scratch a scan of n elements needs: per pass the tile sums and their offsets (one more)
size_t ab_scan_words(long long n) {
  size_t w = 0;
  while (n > AB_TILE) {
    n = (n + AB_TILE - 1) / AB_TILE;
    w += 2 * (size_t)n + 1;
  }
  return w;
}

template <typename Tin, typename Tout>
void ab_scan(hipStream_t st, const Tin* in, long long n, Tout* out, long long* total, long long* ws) {
  const long long nt = (n + AB_TILE - 1) / AB_TILE;
  if (nt <= 1) {
    hipLaunchKernelGGL((k_ab_scan_apply<Tin, Tout>), dim3(1), dim3(AB_TILE), 0, st, n, in, (const long long*)nullptr, out, total);
    return;
  }
  long long* sums = ws;
  long long* offs = ws + nt;
  hipLaunchKernelGGL((k_ab_scan_sums<Tin>), ab_grid(n), dim3(AB_TILE), 0, st, n, in, sums);
  ab_scan<long long, long long>(st, sums, nt, offs, nullptr, ws + 2 * nt + 1);
  hipLaunchKernelGGL((k_ab_scan_apply<Tin, Tout>), ab_grid(n), dim3(AB_TILE), 0, st, n, in, (const long long*)offs, out, total);
}
}  // namespace

// ---- direct interpolation --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AB_TILE) k_ab_p0_count(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                        const uint8_t* __restrict__ mask, const uint8_t* __restrict__ strong,
                                                        const int* __restrict__ state, int32_t* __restrict__ cnt, AbInfo* info) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int c = 1;
  if (state[i] != 1) {
    c = 0;
    const bool mi = mask[i] != 0;
    const int e = rowptr[i + 1];
    for (int q = rowptr[i]; q < e; ++q) {
      const int j = ab_col(colm[q]);
      c += strong[q] && state[j] == 1 && (!mi || mask[j]);
    }
    if (c == 0) atomicMin(&info->bad_vertex, i);
  }
  cnt[i] = c;
}

__global__ void __launch_bounds__(AB_TILE) k_ab_p0_fill(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                       const uint8_t* __restrict__ mask, const uint8_t* __restrict__ strong,
                                                       const int* __restrict__ state, const int32_t* __restrict__ cnum,
                                                       const int32_t* __restrict__ p0_ptr, int32_t* __restrict__ p0_col,
                                                       int32_t* __restrict__ p0_src) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int w = p0_ptr[i];
  if (state[i] == 1) {
    p0_col[w] = cnum[i];
    p0_src[w] = -1;
    return;
  }
  const bool mi = mask[i] != 0;
  const int e = rowptr[i + 1];
  for (int q = rowptr[i]; q < e; ++q) {
    const int j = ab_col(colm[q]);
    if (strong[q] && state[j] == 1 && (!mi || mask[j])) {
      p0_col[w] = cnum[j];
      p0_src[w] = q;
      ++w;
    }
  }
}

// ---- plan rows -------------------------------------------------------------------------------------------------------------------
// The items of one plan row: for the list entries m in [ls, le), list m is lcol[lptr[k] .. lptr[k + 1]) with k = key[m] (its flag bit
// dropped), ascending and without repeats; an item is (column, a = aval ? aval[m] : m, b = position in lcol).  Grouped by column,
// columns ascending, the items of one column by ascending m: what a stable sort by column of the items generated list after list
// gives.  FILL = false counts distinct columns and items; FILL = true writes per distinct column its column and the start of its
// items (from ebase), and the items (from ibase).
template <bool FILL>
__device__ __forceinline__ void ab_merge_row(int ls, int le, const int32_t* __restrict__ key, const int32_t* __restrict__ aval,
                                             const int32_t* __restrict__ lptr, const int32_t* __restrict__ lcol, int& ncols, int& nitems,
                                             int32_t* __restrict__ out_col, int32_t* __restrict__ out_ptr, int32_t* __restrict__ ia,
                                             int32_t* __restrict__ ib, int ebase, int ibase) {
  int cur = INT_MAX;
  for (int m = ls; m < le; ++m) {
    const int k = ab_col(key[m]);
    const int s = lptr[k];
    if (s < lptr[k + 1]) cur = min(cur, lcol[s]);
  }
  int nc = 0, ni = 0;
  while (cur != INT_MAX) {
    int nxt = INT_MAX;
    if (FILL) {
      out_col[ebase + nc] = cur;
      out_ptr[ebase + nc] = ibase + ni;
    }
    for (int m = ls; m < le; ++m) {
      const int k = ab_col(key[m]);
      int lo = lptr[k];
      const int end = lptr[k + 1];
      int hi = end;
      while (lo < hi) {  // first position with a column >= cur
        const int mid = (lo + hi) >> 1;
        if (lcol[mid] < cur) lo = mid + 1;
        else hi = mid;
      }
      if (lo < end) {
        if (lcol[lo] == cur) {
          if (FILL) {
            ia[ibase + ni] = aval ? aval[m] : m;
            ib[ibase + ni] = lo;
          }
          ++ni;
          ++lo;
        }
        if (lo < end) nxt = min(nxt, lcol[lo]);
      }
    }
    ++nc;
    cur = nxt;
  }
  ncols = nc;
  nitems = ni;
}

// Jacobi rows (interior F vertices) merge the P0 rows behind their K row; every other row copies its P0 row, with empty item lists.
__global__ void __launch_bounds__(AB_TILE) k_ab_jac_count(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                         const uint8_t* __restrict__ mask, const int* __restrict__ state,
                                                         const int32_t* __restrict__ p0_ptr, const int32_t* __restrict__ p0_col,
                                                         int32_t* __restrict__ cnt_e, int32_t* __restrict__ cnt_i, AbInfo* info) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int nc, ni = 0;
  if (state[i] == 1 || mask[i]) {
    nc = p0_ptr[i + 1] - p0_ptr[i];
  } else {
    const int s = rowptr[i], e = rowptr[i + 1];
    bool diag = false;
    for (int q = s; q < e; ++q) diag |= ab_col(colm[q]) == i;
    if (!diag) info->no_diag = 1;
    ab_merge_row<false>(s, e, colm, nullptr, p0_ptr, p0_col, nc, ni, nullptr, nullptr, nullptr, nullptr, 0, 0);
  }
  cnt_e[i] = nc;
  cnt_i[i] = ni;
}

__global__ void __launch_bounds__(AB_TILE) k_ab_jac_fill(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                                                        const uint8_t* __restrict__ mask, const int* __restrict__ state,
                                                        const int32_t* __restrict__ p0_ptr, const int32_t* __restrict__ p0_col,
                                                        const int32_t* __restrict__ f_ptr, const int32_t* __restrict__ f_ibase,
                                                        int32_t* __restrict__ f_col, int32_t* __restrict__ f_own,
                                                        int32_t* __restrict__ f_pptr, int32_t* __restrict__ pa, int32_t* __restrict__ pb,
                                                        int32_t* __restrict__ diag) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  const int fb = f_ptr[i], ib = f_ibase[i];
  if (i == n - 1) f_pptr[f_ptr[n]] = f_ibase[n];
  const int ps = p0_ptr[i], pe = p0_ptr[i + 1];
  if (state[i] == 1 || mask[i]) {
    for (int q = ps; q < pe; ++q) {
      f_col[fb + q - ps] = p0_col[q];
      f_own[fb + q - ps] = q;
      f_pptr[fb + q - ps] = ib;
    }
    diag[i] = -1;
    return;
  }
  const int s = rowptr[i], e = rowptr[i + 1];
  int d = -1;
  for (int q = s; q < e; ++q)
    if (ab_col(colm[q]) == i) d = q;
  diag[i] = d;
  int nc, ni;
  ab_merge_row<true>(s, e, colm, nullptr, p0_ptr, p0_col, nc, ni, f_col, f_pptr, pa, pb, fb, ib);
  int q = ps;  // both lists ascend by column, the row's own columns are among the union
  for (int f = fb; f < fb + nc; ++f) {
    int o = -1;
    if (q < pe && p0_col[q] == f_col[f]) o = q++;
    f_own[f] = o;
  }
}

// ---- P = the entries that survived the truncation ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(AB_TILE) k_ab_nz_count(int n, const int32_t* __restrict__ f_ptr, const double* __restrict__ f_val,
                                                        int32_t* __restrict__ cnt) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int c = 0;
  const int e = f_ptr[i + 1];
  for (int f = f_ptr[i]; f < e; ++f) c += f_val[f] != 0.0;
  cnt[i] = c;
}

__global__ void __launch_bounds__(AB_TILE) k_ab_nz_fill(int n, const int32_t* __restrict__ f_ptr, const int32_t* __restrict__ f_col,
                                                       const double* __restrict__ f_val, const int32_t* __restrict__ P_ptr,
                                                       int32_t* __restrict__ P_col, double* __restrict__ P_val) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int w = P_ptr[i];
  const int e = f_ptr[i + 1];
  for (int f = f_ptr[i]; f < e; ++f)
    if (f_val[f] != 0.0) {
      P_col[w] = f_col[f];
      P_val[w] = f_val[f];
      ++w;
    }
}

// ---- child lists = P^T as CSR ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AB_TILE) k_ab_child_count(int nnz_p, const int32_t* __restrict__ P_col, int32_t* cnt) {
  const int q = blockIdx.x * AB_TILE + threadIdx.x;
  if (q < nnz_p) atomicAdd(&cnt[P_col[q]], 1);
}

__global__ void __launch_bounds__(AB_TILE) k_ab_child_place(int n, const int32_t* __restrict__ P_ptr, const int32_t* __restrict__ P_col,
                                                           const int32_t* __restrict__ ch_ptr, int32_t* pos, int32_t* __restrict__ ch_idx,
                                                           int32_t* __restrict__ ch_q) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  const int e = P_ptr[i + 1];
  for (int q = P_ptr[i]; q < e; ++q) {
    const int I = P_col[q];
    const int k = ch_ptr[I] + atomicAdd(&pos[I], 1);
    ch_idx[k] = i;
    ch_q[k] = q;
  }
}

// the atomics placed the children in arrival order: by ascending fine index, as the host lists them (a fine vertex is in a list once)
__global__ void __launch_bounds__(AB_TILE) k_ab_child_sort(int nc, const int32_t* __restrict__ ch_ptr, int32_t* __restrict__ ch_idx,
                                                          int32_t* __restrict__ ch_q) {
  const int I = blockIdx.x * AB_TILE + threadIdx.x;
  if (I >= nc) return;
  const int s = ch_ptr[I], e = ch_ptr[I + 1];
  for (int k = s + 1; k < e; ++k) {
    const int vi = ch_idx[k], vq = ch_q[k];
    int j = k - 1;
    while (j >= s && ch_idx[j] > vi) {
      ch_idx[j + 1] = ch_idx[j];
      ch_q[j + 1] = ch_q[j];
      --j;
    }
    ch_idx[j + 1] = vi;
    ch_q[j + 1] = vq;
  }
}

// ---- Galerkin plans: one kernel pair serves both stages ----------------------------------------------------------------------------
// stage 1, row i of T = A P: lists = the P rows behind the entries of K row i (key = colm, a = the K entry)
// stage 2, row I of P^T T:   lists = the T rows of the children of I (key = ch_idx, a = the child's P entry ch_q)
__global__ void __launch_bounds__(AB_TILE) k_ab_plan_count(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ key,
                                                          const int32_t* __restrict__ lptr, const int32_t* __restrict__ lcol,
                                                          int32_t* __restrict__ cnt_e, int32_t* __restrict__ cnt_i) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  int nc, ni;
  ab_merge_row<false>(row_ptr[i], row_ptr[i + 1], key, nullptr, lptr, lcol, nc, ni, nullptr, nullptr, nullptr, nullptr, 0, 0);
  cnt_e[i] = nc;
  cnt_i[i] = ni;
}

__global__ void __launch_bounds__(AB_TILE) k_ab_plan_fill(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ key,
                                                         const int32_t* __restrict__ aval, const int32_t* __restrict__ lptr,
                                                         const int32_t* __restrict__ lcol, const int32_t* __restrict__ e_ptr,
                                                         const int32_t* __restrict__ i_base, int32_t* __restrict__ out_col,
                                                         int32_t* __restrict__ out_ptr, int32_t* __restrict__ ia, int32_t* __restrict__ ib) {
  const int i = blockIdx.x * AB_TILE + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) out_ptr[e_ptr[n]] = i_base[n];
  int nc, ni;
  ab_merge_row<true>(row_ptr[i], row_ptr[i + 1], key, aval, lptr, lcol, nc, ni, out_col, out_ptr, ia, ib, e_ptr[i], i_base[i]);
}

__global__ void __launch_bounds__(AB_TILE) k_ab_coarse_mask(int n, const int* __restrict__ state, const int32_t* __restrict__ cnum,
                                                           const uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_c) {
  const int v = blockIdx.x * AB_TILE + threadIdx.x;
  if (v < n && state[v] == 1) mask_c[cnum[v]] = mask[v];
}

__global__ void __launch_bounds__(AB_TILE) k_ab_colm(int nnz, const int32_t* __restrict__ col, const uint8_t* __restrict__ mask_c,
                                                    int32_t* __restrict__ colm) {
  const int e = blockIdx.x * AB_TILE + threadIdx.x;
  if (e < nnz) colm[e] = (int32_t)((uint32_t)col[e] | (mask_c[col[e]] ? 0x80000000u : 0u));
}

// ---- the pass ----------------------------------------------------------------------------------------------------------------------
namespace {
double ab_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

// Arguments as pgx_build_hierarchy has checked and defaulted them.
int pgx_amg_build_device(pgx_handle* h, double theta, double trunc, int32_t min_coarse, double max_keep, int32_t* n_levels, double* seconds) {
  const auto t_all = std::chrono::steady_clock::now();
  double t_wait = 0.0;  // time the host spent waiting for the device or copying: seconds[1]; the rest of the wall time is seconds[0]
  std::vector<UmgLevel> lv(1);
  std::vector<int32_t> launches;
  {
    const auto t_0 = std::chrono::steady_clock::now();
    const int rc = umg_level0(h, lv[0]);  // downloads the level-0 mask for the host mirror
    if (rc) return rc;
    t_wait += ab_since(t_0);
  }
  const hipStream_t st = h->st;
  AbInfo hi;
  // the record the device reports through; read with the stream drained
#define AB_READ(info_dev)                                                                    \
  do {                                                                                       \
    const auto t_r = std::chrono::steady_clock::now();                                       \
    HIPCHK(hipStreamSynchronize(st));                                                        \
    HIPCHK(hipGetLastError());                                                               \
    HIPCHK(hipMemcpy(&hi, (info_dev), sizeof(AbInfo), hipMemcpyDeviceToHost));               \
    t_wait += ab_since(t_r);                                                                 \
  } while (0)
#define AB_TMP(p, count) HIPCHK(tmp.get(&(p), (size_t)(count)))
  for (;;) {
    const int l = (int)lv.size() - 1;
    const int nf = lv[l].n, nnz = lv[l].nnz;
    if (nf <= min_coarse) break;
    lv.reserve(lv.size() + 1);  // the reference into lv[l] below outlives the emplace_back of the coarse level
    const UmgLevel& F = lv[l];
    DevTmp tmp;
    AbInfo* info;
    long long* ws;
    uint8_t *own, *strong;
    int* state;
    int32_t *cnt_e, *cnt_i, *cnum;
    AB_TMP(info, 1);
    AB_TMP(ws, ab_scan_words(nf) + 1);
    AB_TMP(own, nnz);
    AB_TMP(strong, nnz);
    AB_TMP(state, nf);
    AB_TMP(cnt_e, nf);
    AB_TMP(cnt_i, nf);
    AB_TMP(cnum, nf + 1);
    const AbInfo zero = {{0, 0}, INT_MAX, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(info, &zero, sizeof(AbInfo), hipMemcpyHostToDevice, st));  // `zero` lives until the first AB_READ below
    HIPCHK(hipMemsetAsync(state, 0, sizeof(int) * (size_t)nf, st));
    hipLaunchKernelGGL(k_ab_strength_own, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.K, theta, own);
    hipLaunchKernelGGL(k_ab_strength_sym, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, own, strong);
    // split: every launch decides at least the lowest undecided vertex of each kind, so nf launches always suffice
    int n_launch = 0;
    do {
      const int batch = std::min(h->amg_split_batch, nf - n_launch);
      if (batch <= 0) {
        h->err = "pgx_build_hierarchy: the split did not end (level " + std::to_string(l) + ")";
        return PGX_EHIP;
      }
      for (int k = 0; k < batch; ++k)
        hipLaunchKernelGGL(k_ab_split, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.mask, strong, state, info);
      n_launch += batch;
      AB_READ(info);
    } while (hi.decided < nf);
    hipLaunchKernelGGL(k_ab_flag_c, ab_grid(nf), dim3(AB_TILE), 0, st, nf, state, cnt_e);
    ab_scan<int32_t, int32_t>(st, cnt_e, nf, cnum, &info->tot[0], ws);
    // direct interpolation: counted along with the numbering, so that one read serves both
    hipLaunchKernelGGL(k_ab_p0_count, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.mask, strong, state, cnt_i, info);
    int32_t* p0_ptr;
    AB_TMP(p0_ptr, nf + 1);
    ab_scan<int32_t, int32_t>(st, cnt_i, nf, p0_ptr, &info->tot[1], ws);
    AB_READ(info);
    const int nc = (int)hi.tot[0];
    if ((double)nc > max_keep * (double)nf) break;  // the step would keep too many vertices: the level above stays the coarsest
    if (hi.bad_vertex != INT_MAX) {
      h->err = "pgx_build_hierarchy: an F vertex without a C neighbour (level " + std::to_string(l) + ", vertex " + std::to_string(hi.bad_vertex) + ")";
      return PGX_EINVAL;
    }
    const long long nnz_p0 = hi.tot[1];  // at most nnz
    int32_t *p0_col, *p0_src, *f_ptr, *f_ibase;
    double* p0_val;
    AB_TMP(p0_col, nnz_p0);
    AB_TMP(p0_src, nnz_p0);
    AB_TMP(p0_val, nnz_p0);
    AB_TMP(f_ptr, nf + 1);
    AB_TMP(f_ibase, nf + 1);
    hipLaunchKernelGGL(k_ab_p0_fill, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.mask, strong, state, cnum, p0_ptr, p0_col, p0_src);
    pgxk_amg_direct(st, nf, p0_ptr, p0_src, F.K, p0_val);
    // the untruncated pattern
    hipLaunchKernelGGL(k_ab_jac_count, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.mask, state, p0_ptr, p0_col, cnt_e, cnt_i, info);
    ab_scan<int32_t, int32_t>(st, cnt_e, nf, f_ptr, &info->tot[0], ws);
    ab_scan<int32_t, int32_t>(st, cnt_i, nf, f_ibase, &info->tot[1], ws);
    AB_READ(info);
    // a mesh with BOTH faults: the host pass reports whichever its row loop meets first, this pass always the missing diagonal
    if (hi.no_diag) {
      h->err = "pgx_build_hierarchy: a row without its diagonal entry";
      return PGX_EINVAL;
    }
    if (hi.tot[0] >= (1ll << 31) || hi.tot[1] >= (1ll << 31)) {
      h->err = "pgx_build_hierarchy: interpolation plan exceeds int32";
      return PGX_EINVAL;
    }
    const long long nnz_f = hi.tot[0], n_pa = hi.tot[1];
    int32_t *f_col, *f_own, *f_pptr, *pa, *pb, *diag;
    double* f_val;
    AB_TMP(f_col, nnz_f);
    AB_TMP(f_own, nnz_f);
    AB_TMP(f_pptr, nnz_f + 1);
    AB_TMP(pa, n_pa);
    AB_TMP(pb, n_pa);
    AB_TMP(diag, nf);
    AB_TMP(f_val, nnz_f);
    hipLaunchKernelGGL(k_ab_jac_fill, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, F.mask, state, p0_ptr, p0_col, f_ptr, f_ibase, f_col,
                       f_own, f_pptr, pa, pb, diag);
    pgxk_amg_pvalues(st, nf, f_ptr, f_own, f_pptr, pa, pb, diag, F.K, p0_val, trunc, f_val);
    lv.emplace_back();
    UmgLevel& C = lv[l + 1];
    C.n = nc;
    DALLOC(C.P_ptr, nf + 1);
    hipLaunchKernelGGL(k_ab_nz_count, ab_grid(nf), dim3(AB_TILE), 0, st, nf, f_ptr, f_val, cnt_e);
    ab_scan<int32_t, int32_t>(st, cnt_e, nf, C.P_ptr, &info->tot[0], ws);
    AB_READ(info);
    C.nnz_p = (int)hi.tot[0];  // at most nnz_f
    DALLOC(C.P_col, C.nnz_p);
    DALLOC(C.P_val, C.nnz_p);
    DALLOC(C.ch_ptr, nc + 1);
    DALLOC(C.ch_idx, C.nnz_p);
    DALLOC(C.ch_q, C.nnz_p);
    hipLaunchKernelGGL(k_ab_nz_fill, ab_grid(nf), dim3(AB_TILE), 0, st, nf, f_ptr, f_col, f_val, C.P_ptr, C.P_col, C.P_val);
    // child lists; the fill position per coarse vertex counts in cnt_i (nc < nf), which stage 1 overwrites only afterwards
    int32_t *ccnt, *cpos = cnt_i;
    AB_TMP(ccnt, nc);
    HIPCHK(hipMemsetAsync(ccnt, 0, sizeof(int32_t) * (size_t)nc, st));
    HIPCHK(hipMemsetAsync(cpos, 0, sizeof(int32_t) * (size_t)nc, st));
    hipLaunchKernelGGL(k_ab_child_count, ab_grid(C.nnz_p), dim3(AB_TILE), 0, st, C.nnz_p, C.P_col, ccnt);
    ab_scan<int32_t, int32_t>(st, ccnt, nc, C.ch_ptr, (long long*)nullptr, ws);
    hipLaunchKernelGGL(k_ab_child_place, ab_grid(nf), dim3(AB_TILE), 0, st, nf, C.P_ptr, C.P_col, C.ch_ptr, cpos, C.ch_idx, C.ch_q);
    hipLaunchKernelGGL(k_ab_child_sort, ab_grid(nc), dim3(AB_TILE), 0, st, nc, C.ch_ptr, C.ch_idx, C.ch_q);
    // coarse mask (the last reader of state and cnum)
    DALLOC(C.mask, nc);
    hipLaunchKernelGGL(k_ab_coarse_mask, ab_grid(nf), dim3(AB_TILE), 0, st, nf, state, cnum, F.mask, C.mask);
    // stage 1: T = A P row by row
    int32_t *t_rowptr, *t_ibase, *t_col;
    AB_TMP(t_rowptr, nf + 1);
    AB_TMP(t_ibase, nf + 1);
    hipLaunchKernelGGL(k_ab_plan_count, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, C.P_ptr, C.P_col, cnt_e, cnt_i);
    ab_scan<int32_t, int32_t>(st, cnt_e, nf, t_rowptr, &info->tot[0], ws);
    ab_scan<int32_t, int32_t>(st, cnt_i, nf, t_ibase, &info->tot[1], ws);
    AB_READ(info);
    if (hi.tot[0] >= (1ll << 31) || hi.tot[1] >= (1ll << 31)) {
      h->err = "pgx_build_hierarchy: Galerkin plan exceeds int32";
      return PGX_EINVAL;
    }
    C.nnz_t = (int)hi.tot[0];
    const long long n_ta = hi.tot[1];
    AB_TMP(t_col, C.nnz_t);
    DALLOC(C.t_ptr, C.nnz_t + 1);
    DALLOC(C.t_a, n_ta);
    DALLOC(C.t_p, n_ta);
    hipLaunchKernelGGL(k_ab_plan_fill, ab_grid(nf), dim3(AB_TILE), 0, st, nf, F.rowptr, F.colm, (const int32_t*)nullptr, C.P_ptr, C.P_col, t_rowptr,
                       t_ibase, t_col, C.t_ptr, C.t_a, C.t_p);
    // stage 2: P^T T over the child lists (counters of nc rows in the arrays that held nf)
    int32_t *g_ibase, *c_col;
    DALLOC(C.rowptr, nc + 1);
    AB_TMP(g_ibase, nc + 1);
    hipLaunchKernelGGL(k_ab_plan_count, ab_grid(nc), dim3(AB_TILE), 0, st, nc, C.ch_ptr, C.ch_idx, t_rowptr, t_col, cnt_e, cnt_i);
    ab_scan<int32_t, int32_t>(st, cnt_e, nc, C.rowptr, &info->tot[0], ws);
    ab_scan<int32_t, int32_t>(st, cnt_i, nc, g_ibase, &info->tot[1], ws);
    AB_READ(info);
    if (hi.tot[0] >= (1ll << 31) || hi.tot[1] >= (1ll << 31)) {
      h->err = "pgx_build_hierarchy: Galerkin plan exceeds int32";
      return PGX_EINVAL;
    }
    C.nnz = (int)hi.tot[0];
    const long long n_g = hi.tot[1];
    AB_TMP(c_col, C.nnz);
    DALLOC(C.g_ptr, C.nnz + 1);
    DALLOC(C.g_p, n_g);
    DALLOC(C.g_t, n_g);
    DALLOC(C.colm, C.nnz);
    hipLaunchKernelGGL(k_ab_plan_fill, ab_grid(nc), dim3(AB_TILE), 0, st, nc, C.ch_ptr, C.ch_idx, (const int32_t*)C.ch_q, t_rowptr, t_col, C.rowptr,
                       g_ibase, c_col, C.g_ptr, C.g_p, C.g_t);
    hipLaunchKernelGGL(k_ab_colm, ab_grid(C.nnz), dim3(AB_TILE), 0, st, C.nnz, c_col, C.mask, C.colm);
    DALLOC(C.T, C.nnz_t);
    DALLOC(C.K, C.nnz);
    DALLOC(C.M, C.nnz);
    DALLOC(C.D, C.nnz);
    double** const vecs[8] = {&C.bu, &C.bp, &C.xu, &C.xp, &C.xu2, &C.xp2, &C.ru, &C.rp};
    for (double** v : vecs) DALLOC(*v, nc);
    pgxk_amg_rap(st, C, F.K, C.K);  // the next split reads this level's K
    pgxk_amg_rap(st, C, F.M, C.M);
    // host mirrors of the level (export hooks, the coarse solve under a degree-2 handle): one download each
    C.h_rowptr.resize(nc + 1);
    C.h_col.resize(C.nnz);
    C.h_mask.resize(nc);
    C.h_P_ptr.resize(nf + 1);
    C.h_P_col.resize(C.nnz_p);
    const auto t_m = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(C.h_rowptr.data(), C.rowptr, sizeof(int32_t) * C.h_rowptr.size(), hipMemcpyDeviceToHost));
    if (C.nnz) HIPCHK(hipMemcpy(C.h_col.data(), c_col, sizeof(int32_t) * C.h_col.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(C.h_mask.data(), C.mask, C.h_mask.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(C.h_P_ptr.data(), C.P_ptr, sizeof(int32_t) * C.h_P_ptr.size(), hipMemcpyDeviceToHost));
    if (C.nnz_p) HIPCHK(hipMemcpy(C.h_P_col.data(), C.P_col, sizeof(int32_t) * C.h_P_col.size(), hipMemcpyDeviceToHost));
    t_wait += ab_since(t_m);
    launches.push_back(n_launch);
  }
#undef AB_READ
#undef AB_TMP
  if (lv.size() < 2) {
    h->err = "pgx_build_hierarchy: the first coarsening step keeps more than max_keep of the vertices, no hierarchy was built";
    return PGX_EINVAL;
  }
  umg_install(h, std::move(lv));
  h->amg_mode = 1;
  h->amg_split = std::move(launches);
  if (n_levels) *n_levels = (int32_t)h->umg.size();
  if (seconds) {
    seconds[1] = t_wait;
    seconds[0] = ab_since(t_all) - t_wait;
  }
  return PGX_OK;
}
