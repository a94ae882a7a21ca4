// Host-side setup of a handle (once per handle, not on the hot path): the assembly plans (CSR pattern, inverted vertex->cell lists),
// the (K, M) dictionary of the P2 level, the strip partition arithmetic, the stencil hierarchies of structured meshes, single and
// sharded, and the host symbolic pass of pgx_set_hierarchy.  Called from create_impl (pgx_api.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgx_handle.h"

// ------------------------------------------------------------------------------------------------
// plan building on the host (setup only; not on the hot path)
// ------------------------------------------------------------------------------------------------
int build_plan(pgx_handle* h, const pgx_mesh* m, const std::vector<uint8_t>& hmask) {
  const int n = m->n_vertices, nc = m->n_cells;
  std::vector<int32_t> vptr(n + 1, 0);
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < 3; ++a) {
      const int v = m->cells[3 * c + a];
      if (v < 0 || v >= n) {
        h->err = "cell vertex id out of range";
        return PGX_EINVAL;
      }
      vptr[v + 1]++;
    }
  for (int i = 0; i < n; ++i) vptr[i + 1] += vptr[i];
  std::vector<int32_t> vent(vptr[n]), fillp(vptr.begin(), vptr.end() - 1);
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < 3; ++a) vent[fillp[m->cells[3 * c + a]]++] = c * 4 + a;
  // rows: sorted unique neighbour vertices
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(n + 1, 0);
  col.clear();
  col.reserve((size_t)n * 7);
  std::vector<int32_t> tmp;
  for (int i = 0; i < n; ++i) {
    tmp.clear();
    for (int k = vptr[i]; k < vptr[i + 1]; ++k) {
      const int c = vent[k] >> 2;
      tmp.push_back(m->cells[3 * c]);
      tmp.push_back(m->cells[3 * c + 1]);
      tmp.push_back(m->cells[3 * c + 2]);
    }
    if (tmp.empty()) tmp.push_back(i);  // isolated vertex: keep a diagonal
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    if (tmp.size() > 255) {
      h->err = "vertex degree > 255 unsupported";
      return PGX_EINVAL;
    }
    col.insert(col.end(), tmp.begin(), tmp.end());
    rowptr[i + 1] = (int32_t)col.size();
  }
  if (col.size() > 0x7fffffffu) {
    h->err = "nnz overflows int32";
    return PGX_EINVAL;
  }
  h->nnz = (int)col.size();
  std::vector<int32_t> vpos(vent.size());
  for (int i = 0; i < n; ++i) {
    const int32_t* rb = col.data() + rowptr[i];
    const int32_t* re = col.data() + rowptr[i + 1];
    for (int k = vptr[i]; k < vptr[i + 1]; ++k) {
      const int c = vent[k] >> 2;
      int pos = 0;
      for (int b = 0; b < 3; ++b) {
        const int p = (int)(std::lower_bound(rb, re, m->cells[3 * c + b]) - rb);
        pos |= p << (8 * b);
      }
      vpos[k] = pos;
    }
  }
  size_t maxlen = 0;
  for (int i0 = 0; i0 < n; i0 += PGX_BLOCK) {
    const int i1 = std::min(i0 + PGX_BLOCK, n);
    maxlen = std::max(maxlen, (size_t)(rowptr[i1] - rowptr[i0]));
  }
  h->fill_lds = maxlen * sizeof(double);
  if (h->fill_lds > 150 * 1024) {
    h->err = "row block too dense for the LDS-staged fill";
    return PGX_EINVAL;
  }
  if (h->structured) {
    const int sx = h->nx + 1;
    for (int i = 0; i < n; ++i)
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int o = col[k] - i;
        if (!(o == 0 || o == 1 || o == -1 || o == sx || o == -sx || o == sx + 1 || o == -sx - 1)) {
          h->err = "mesh flagged structured is not the right-diagonal triangulation (vertex v=j*(nx+1)+i)";
          return PGX_EINVAL;
        }
      }
  }
  std::vector<int32_t> colm(col.size());
  for (size_t k = 0; k < col.size(); ++k) colm[k] = col[k] | (hmask[col[k]] ? (int32_t)0x80000000 : 0);
  DALLOC(h->rowptr, n + 1);
  DALLOC(h->colm, colm.size());
  DALLOC(h->v2c_ptr, n + 1);
  DALLOC(h->v2c_ent, vent.size());
  DALLOC(h->v2c_pos, vpos.size());
  HIPCHK(hipMemcpy(h->rowptr, rowptr.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->colm, colm.data(), sizeof(int32_t) * colm.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->v2c_ptr, vptr.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->v2c_ent, vent.data(), sizeof(int32_t) * vent.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->v2c_pos, vpos.data(), sizeof(int32_t) * vpos.size(), hipMemcpyHostToDevice));
  return PGX_OK;
}

// P2 plan: scalar CSR pattern over [vertex | edge] dofs, dof -> (cell, local dof) lists with the row positions
// of the cell's 6 dofs (two int32 per entry), vertex -> edge-dof lists and edge end points for the transfers.
int build_plan_p2(pgx_handle* h, const pgx_mesh* m, const std::vector<uint8_t>& hmask) {
  const int n = h->nd, nc = m->n_cells, nv = m->n_vertices;
  const int32_t* cd = m->cell_dofs;
  std::vector<int32_t> vptr(n + 1, 0);
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < 6; ++a) {
      const int v = cd[6 * c + a];
      if (v < 0 || v >= n || (a < 3 && v != m->cells[3 * c + a]) || (a >= 3 && v < nv)) {
        h->err = "cell_dofs must be [vertex ids (== cells) | edge dofs >= n_vertices]";
        return PGX_EINVAL;
      }
      vptr[v + 1]++;
    }
  for (int i = 0; i < n; ++i) vptr[i + 1] += vptr[i];
  std::vector<int32_t> vent(vptr[n]), fillp(vptr.begin(), vptr.end() - 1);
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < 6; ++a) vent[fillp[cd[6 * c + a]]++] = c * 8 + a;
  std::vector<int32_t>& rowptr = h->s_h_rowptr;
  std::vector<int32_t>& col = h->s_h_col;
  rowptr.assign(n + 1, 0);
  col.clear();
  col.reserve((size_t)n * 12);
  std::vector<int32_t> tmp;
  for (int i = 0; i < n; ++i) {
    tmp.clear();
    for (int k = vptr[i]; k < vptr[i + 1]; ++k) {
      const int c = vent[k] >> 3;
      for (int b = 0; b < 6; ++b) tmp.push_back(cd[6 * c + b]);
    }
    if (tmp.empty()) tmp.push_back(i);
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    if (tmp.size() > 255) {
      h->err = "dof degree > 255 unsupported";
      return PGX_EINVAL;
    }
    col.insert(col.end(), tmp.begin(), tmp.end());
    rowptr[i + 1] = (int32_t)col.size();
  }
  if (col.size() > 0x7fffffffu) {
    h->err = "nnz overflows int32";
    return PGX_EINVAL;
  }
  h->s_nnz = (int)col.size();
  std::vector<int32_t> vpos(2 * vent.size());
  for (int i = 0; i < n; ++i) {
    const int32_t* rb = col.data() + rowptr[i];
    const int32_t* re = col.data() + rowptr[i + 1];
    for (int k = vptr[i]; k < vptr[i + 1]; ++k) {
      const int c = vent[k] >> 3;
      uint32_t p0 = 0, p1 = 0;
      for (int b = 0; b < 6; ++b) {
        const uint32_t pp = (uint32_t)(std::lower_bound(rb, re, cd[6 * c + b]) - rb);
        if (b < 4) p0 |= pp << (8 * b);
        else p1 |= pp << (8 * (b - 4));
      }
      vpos[2 * k] = (int32_t)p0;
      vpos[2 * k + 1] = (int32_t)p1;
    }
  }
  size_t maxlen = 0;
  for (int i0 = 0; i0 < n; i0 += PGX_BLOCK) {
    const int i1 = std::min(i0 + PGX_BLOCK, n);
    maxlen = std::max(maxlen, (size_t)(rowptr[i1] - rowptr[i0]));
  }
  std::vector<int32_t> blk{0};
  for (int r = 0; r < n;) {  // greedy: as many rows as fit PGX_BAL_CAP entries (a P2 row has at most 23), at most PGX_BLOCK rows
    int e = r;
    while (e < n && e - r < PGX_BLOCK && rowptr[e + 1] - rowptr[r] <= PGX_BAL_CAP) ++e;
    if (e == r) {
      blk.clear();  // a single row beyond the capacity: keep the unbalanced kernel
      break;
    }
    blk.push_back(e);
    r = e;
  }
  h->s_fill_lds = maxlen * sizeof(double);
  if (h->s_fill_lds > 60 * 1024) {
    h->err = "row block too dense for the LDS-staged fill";
    return PGX_EINVAL;
  }
  // transfers: edge end points (local edge i is opposite local vertex i) and vertex -> edge dofs
  const int ne = n - nv;
  std::vector<int32_t> ends(2 * (size_t)ne, -1), eptr(nv + 1, 0);
  for (int c = 0; c < nc; ++c)
    for (int i = 0; i < 3; ++i) {
      const int e = cd[6 * c + 3 + i] - nv;
      const int a = m->cells[3 * c + (i + 1) % 3], b = m->cells[3 * c + (i + 2) % 3];
      const int lo = std::min(a, b), hi = std::max(a, b);
      if (ends[2 * e] >= 0 && (ends[2 * e] != lo || ends[2 * e + 1] != hi)) {
        h->err = "cell_dofs: an edge dof is attached to two different vertex pairs";
        return PGX_EINVAL;
      }
      ends[2 * e] = lo;
      ends[2 * e + 1] = hi;
    }
  for (int e = 0; e < ne; ++e) {
    if (ends[2 * e] < 0) {
      h->err = "cell_dofs: unused edge dof";
      return PGX_EINVAL;
    }
    eptr[ends[2 * e] + 1]++;
    eptr[ends[2 * e + 1] + 1]++;
  }
  if (h->dist.on) {  // sharded P2 addresses the edges of a vertex row as one contiguous block (Dist::eb)
    const int sx = h->nx + 1;
    std::vector<int> per_row(h->ny + 1, 0);
    bool sorted = true;
    for (int e = 0; e < ne; ++e) {
      if (e && ends[2 * e] < ends[2 * (e - 1)]) sorted = false;
      per_row[ends[2 * e] / sx]++;
    }
    for (int j = 0; j <= h->ny && sorted; ++j) sorted = per_row[j] == (j < h->ny ? 3 * h->nx + 1 : h->nx);
    if (!sorted) {
      h->err = "pgx_create_sharded (P2): edge dofs must be numbered by their lower vertex, row by row (3 nx + 1 per vertex row)";
      return PGX_EINVAL;
    }
  }
  for (int i = 0; i < nv; ++i) eptr[i + 1] += eptr[i];
  std::vector<int32_t> elist(eptr[nv]), ef(eptr.begin(), eptr.end() - 1);
  for (int e = 0; e < ne; ++e) {
    elist[ef[ends[2 * e]]++] = nv + e;
    elist[ef[ends[2 * e + 1]]++] = nv + e;
  }
  std::vector<int32_t> colm(col.size());
  for (size_t k = 0; k < col.size(); ++k) colm[k] = col[k] | (hmask[col[k]] ? (int32_t)0x80000000 : 0);
  // structured operator apply (pgx_p2st.hip): derive the 46-entry table from one interior group, verify it on every group of the
  // largest rectangle of groups that match, list the rows of the frame around it
  if (h->structured && (!h->dist.on || h->p2st.dist_enable) && h->p2st.enable && h->nx >= 8 && h->ny >= 8) {
    const int nx = h->nx, ny = h->ny, sx = nx + 1;
    auto ebase = [&](int i, int j) { return nv + j * (3 * nx + 1) + 3 * i; };
    bool ok = (nv == sx * (ny + 1)) && (ne == ny * (3 * nx + 1) + nx);
    for (int j = 0; j < ny && ok; ++j)
      for (int i = 0; i < nx && ok; ++i) {  // edges numbered by lower vertex: H, V, D of vertex (i, j)
        const int v = j * sx + i, e = ebase(i, j) - nv;
        ok = ends[2 * e] == v && ends[2 * e + 1] == v + 1 && ends[2 * e + 2] == v && ends[2 * e + 3] == v + sx &&
             ends[2 * e + 4] == v && ends[2 * e + 5] == v + sx + 1;
      }
    pgx_handle::P2St& S = h->p2st;
    const int ir = nx / 2, jr = ny / 2;  // reference group
    int nt[4] = {19, 9, 9, 9}, off[4] = {0, 19, 28, 37};
    if (ok) {
      const int vr = jr * sx + ir, er = ebase(ir, jr);
      for (int t = 0; t < 4 && ok; ++t) {
        const int row = t == 0 ? vr : er + t - 1;
        S.ref_rows[t] = row;
        ok = rowptr[row + 1] - rowptr[row] == nt[t];
        for (int k = 0; k < nt[t] && ok; ++k) {
          const int c = col[rowptr[row] + k];
          S.tab.isedge[off[t] + k] = c >= nv;
          S.tab.delta[off[t] + k] = c >= nv ? c - er : c - vr;
        }
      }
    }
    auto group_ok = [&](int i, int j) -> bool {
      if (i < 1 || j < 1 || i >= nx || j >= ny) return false;
      const int v = j * sx + i, eb = ebase(i, j);
      for (int t = 0; t < 4; ++t) {
        const int row = t == 0 ? v : eb + t - 1;
        if (hmask[row] || rowptr[row + 1] - rowptr[row] != nt[t]) return false;
        for (int k = 0; k < nt[t]; ++k) {
          const int c = col[rowptr[row] + k];
          if (hmask[c] || c != (S.tab.isedge[off[t] + k] ? eb : v) + S.tab.delta[off[t] + k]) return false;
        }
      }
      return true;
    };
    if (ok && group_ok(ir, jr)) {
      int i0 = ir, i1 = ir, j0 = jr, j1 = jr;
      while (group_ok(i0 - 1, jr)) --i0;
      while (group_ok(i1 + 1, jr)) ++i1;
      while (group_ok(ir, j0 - 1)) --j0;
      while (group_ok(ir, j1 + 1)) ++j1;
      for (int j = j0; j <= j1 && ok; ++j)
        for (int i = i0; i <= i1 && ok; ++i) ok = group_ok(i, j);
      if (ok) {
        std::vector<int32_t> frame;
        auto fast = [&](int v) {
          const int i = v % sx, j = v / sx;
          return i >= i0 && i <= i1 && j >= j0 && j <= j1;
        };
        for (int v = 0; v < nv; ++v)
          if (!fast(v)) frame.push_back(v);
        for (int e = 0; e < ne; ++e)
          if (!fast(ends[2 * e])) frame.push_back(nv + e);
        // LDS form: decode every entry into (dj, di[, kind]) and its offset in the block tiles of k_p2st_apply_lds
        {
          const int VW = PGX_P2ST_BW + 2, EW = 3 * VW, erow = 3 * nx + 1;
          bool lds = true;
          for (int e = 0; e < 46 && lds; ++e) {
            const int d = S.tab.delta[e];
            if (!S.tab.isedge[e]) {
              const int dj = (int)std::lround((double)d / sx), di = d - dj * sx;
              lds = std::abs(dj) <= 1 && std::abs(di) <= 1;
              S.tab.lofs[e] = (dj + 1) * VW + di + 1;
            } else {
              const int dj = (int)std::lround((double)d / erow), rem = d - dj * erow;  // rem = 3 di + kind, di in {-1, 0, 1}
              const int di = (rem + 3) / 3 - 1, kind = rem - 3 * di;
              lds = std::abs(dj) <= 1 && std::abs(di) <= 1 && kind >= 0 && kind <= 2;
              S.tab.lofs[e] = (dj + 1) * EW + 3 * (di + 1) + kind;
            }
          }
          S.tab.lds = lds ? 1 : 0;
          if (const char* e = pgx_tune("PGX_P2ST_LDS")) S.tab.lds = S.tab.lds && atoi(e);
        }
        S.i0 = i0, S.ni = i1 - i0 + 1, S.j0 = j0, S.nj = j1 - j0 + 1, S.nframe = (int)frame.size();
        DALLOC(S.frame, std::max<size_t>(frame.size(), 1));
        HIPCHK(hipMemcpy(S.frame, frame.data(), sizeof(int32_t) * frame.size(), hipMemcpyHostToDevice));
        S.state = 1;
      }
    }
  }
  DALLOC(h->s_rowptr, n + 1);
  {  // vertex-star patches: slot 0 = the vertex, then the edge dofs that meet in it (pgx_patch.hip)
    int maxdeg = 0;
    for (int v = 0; v < nv; ++v) maxdeg = std::max(maxdeg, eptr[v + 1] - eptr[v]);
    h->patch_nn = maxdeg + 1 <= 7 ? 7 : (maxdeg + 1 <= 8 ? 8 : 0);
    // degree 8 ... 15 somewhere: those vertices form the wide set (32 lanes per star), every other star keeps its 16 lanes
    const bool wide = !h->patch_nn && maxdeg + 1 <= PGX_PATCH_WIDE_NN && h->patch_wide && !h->dist.on;
    if (wide) h->patch_nn = 8;
    if (h->patch_nn) {
      const int NN = h->patch_nn;
      h->patch_dof_host.assign((size_t)nv * NN, -1);
      for (int v = 0; v < nv; ++v) {
        const int deg = eptr[v + 1] - eptr[v];
        if (deg + 1 > NN) {  // its row of the narrow table stays all -1: an identity patch there, nothing stored by its lanes
          h->wide_v_host.push_back(v);
          h->wide_dof_host.resize(h->wide_dof_host.size() + PGX_PATCH_WIDE_NN, -1);
          int32_t* d = h->wide_dof_host.data() + h->wide_dof_host.size() - PGX_PATCH_WIDE_NN;
          d[0] = v;
          for (int k = 0; k < deg; ++k) d[1 + k] = elist[eptr[v] + k];
          continue;
        }
        int32_t* d = h->patch_dof_host.data() + (size_t)v * NN;
        d[0] = v;
        for (int k = eptr[v]; k < eptr[v + 1]; ++k) d[1 + k - eptr[v]] = elist[k];
      }
    }
  }
  if (blk.size() > 1) {
    h->s_nblk = (int)blk.size() - 1;
    std::vector<int32_t> blk2(2 * blk.size());  // (first row, its rowptr) per block boundary: the kernel's one metadata load
    for (size_t i = 0; i < blk.size(); ++i) {
      blk2[2 * i] = blk[i];
      blk2[2 * i + 1] = rowptr[blk[i]];
    }
    DALLOC(h->s_blk, blk2.size());
    HIPCHK(hipMemcpy(h->s_blk, blk2.data(), sizeof(int32_t) * blk2.size(), hipMemcpyHostToDevice));
  }
  DALLOC(h->s_colm, colm.size());
  DALLOC(h->p2_v2c_ptr, n + 1);
  DALLOC(h->p2_v2c_ent, vent.size());
  DALLOC(h->p2_v2c_pos, vpos.size());
  DALLOC(h->cdofs, (size_t)6 * nc);
  DALLOC(h->edge_ends, ends.size());
  DALLOC(h->v2e_ptr, nv + 1);
  DALLOC(h->v2e, elist.size());
  HIPCHK(hipMemcpy(h->s_rowptr, rowptr.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->s_colm, colm.data(), sizeof(int32_t) * colm.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->p2_v2c_ptr, vptr.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->p2_v2c_ent, vent.data(), sizeof(int32_t) * vent.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->p2_v2c_pos, vpos.data(), sizeof(int32_t) * vpos.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->cdofs, cd, sizeof(int32_t) * 6 * (size_t)nc, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->edge_ends, ends.data(), sizeof(int32_t) * ends.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->v2e_ptr, eptr.data(), sizeof(int32_t) * (nv + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->v2e, elist.data(), sizeof(int32_t) * elist.size(), hipMemcpyHostToDevice));
  return PGX_OK;
}

// (K, M) dictionary of the P2 level for k_bspmv_bal<true>: distinct pairs after rounding to a grid of 2^-40 of the largest entry
// (finer than the tolerance of detect_uniform below; a function of each entry alone: deterministic).  Seeded with nothing; every round lists up to 4096 unmatched entries, the host adds their distinct values.
// More than 256 pairs (a non-uniform mesh) => no dictionary, the kernel streams K and M as before.
// max |x_i| through atomicMax on the bit pattern (non-negative doubles order like their 64-bit patterns)
__global__ void __launch_bounds__(256) k_maxabs(int64_t n, const double* __restrict__ x, unsigned long long* out) {
  double m = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmax(m, fabs(x[i]));
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

int build_km_dictionary(pgx_handle* h) {
  const int64_t nnz = h->s_nnz;
  const int cap = 4096;
  uint8_t* code = nullptr;
  double* tab = nullptr;
  int* fail = nullptr;
  double* fail_v = nullptr;
  DALLOC(code, (size_t)nnz);
  DALLOC(tab, 512);
  DALLOC(fail, 2);
  DALLOC(fail_v, 2 * cap);
  // scale: the largest |K| and |M| over ALL entries (round 3 looked at the first 65536 only - vertex rows - and missed the larger
  // edge-edge entries of P2), and on a sharded handle the largest over all ranks, so that every rank rounds the same
  // global operator to the same grid
  double kmax = 0.0, mmax = 0.0;
  {
    unsigned long long* dmax = nullptr;
    DALLOC(dmax, 2);
    HIPCHK(hipMemsetAsync(dmax, 0, 2 * sizeof(unsigned long long), h->st));
    const int nb = (int)std::min<int64_t>((nnz + 255) / 256, 4096);
    hipLaunchKernelGGL(k_maxabs, dim3(nb), dim3(256), 0, h->st, nnz, h->s_K, dmax);
    hipLaunchKernelGGL(k_maxabs, dim3(nb), dim3(256), 0, h->st, nnz, h->s_M, dmax + 1);
    unsigned long long hm[2];
    HIPCHK(hipMemcpyAsync(hm, dmax, sizeof(hm), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    memcpy(&kmax, &hm[0], 8);
    memcpy(&mmax, &hm[1], 8);
    if (h->dist.on) {  // max over the ranks through the sum all-reduce: slot `rank` of a zeroed buffer
      const int R = h->dist.size;
      std::vector<double> slots(2 * (size_t)R, 0.0);
      slots[2 * (size_t)h->dist.rank] = kmax;
      slots[2 * (size_t)h->dist.rank + 1] = mmax;
      double* ds = nullptr;
      DALLOC(ds, 2 * (size_t)R);
      HIPCHK(hipMemcpyAsync(ds, slots.data(), slots.size() * sizeof(double), hipMemcpyHostToDevice, h->st));
      const int rc = allreduce_dev(h, ds, 2 * (size_t)R);
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(slots.data(), ds, slots.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
      HIPCHK(hipStreamSynchronize(h->st));
      for (int r = 0; r < R; ++r) {
        kmax = std::max(kmax, slots[2 * (size_t)r]);
        mmax = std::max(mmax, slots[2 * (size_t)r + 1]);
      }
    }
  }
  // grid = 2^-40 (9e-13) of the largest entry, a power of two: rounding to it is exact arithmetic, the same on host and device
  const double tk = std::ldexp(1.0, std::ilogb(kmax > 0 ? kmax : 1.0) - 40), tm = std::ldexp(1.0, std::ilogb(mmax > 0 ? mmax : 1.0) - 40);
  std::vector<double> table(512, 0.0);
  int ntab = 0;
  std::vector<double> fv(2 * cap);
  bool ok = false;
  for (int round = 0; round < 64; ++round) {
    HIPCHK(hipMemcpyAsync(tab, table.data(), 512 * sizeof(double), hipMemcpyHostToDevice, h->st));
    HIPCHK(hipMemsetAsync(fail, 0, 2 * sizeof(int), h->st));
    pgxk_dict_assign(h->st, nnz, h->s_K, h->s_M, ntab, tab, tk, tm, code, fail, cap, fail_v);
    int f[2];
    HIPCHK(hipMemcpyAsync(f, fail, sizeof(f), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    const int nf = std::min(f[0], cap);
    if (nf == 0) {
      ok = true;
      break;
    }
    HIPCHK(hipMemcpy(fv.data(), fail_v, 2 * nf * sizeof(double), hipMemcpyDeviceToHost));
    bool full = false;
    for (int i = 0; i < nf && !full; ++i) {
      const double kv = fv[2 * i], mv = fv[2 * i + 1];  // already rounded to the grid by the kernel
      bool have = false;
      for (int t = 0; t < ntab && !have; ++t) have = kv == table[2 * t] && mv == table[2 * t + 1];
      if (have) continue;
      if (ntab == 256) {
        full = true;
        break;
      }
      table[2 * ntab] = kv;
      table[2 * ntab + 1] = mv;
      ++ntab;
    }
    if (full) break;
  }
  if (pgx_tune("PGX_SPMV_DICT_VERBOSE")) fprintf(stderr, "pgx: (K,M) dictionary: %d pairs, %s\n", ntab, ok ? "in use" : "overflow - not used");
  if (ok) {
    h->s_code = code;
    h->s_tab = tab;
    h->s_ntab = ntab;
  }  // else: the arrays stay allocated (freed with the handle) and unused
  return PGX_OK;
}

// Is the stencil the same at every interior vertex (uniform grid)?  Then interior rows take their K and M
// coefficients from kernel arguments.  Setup-time host check on a downloaded copy.
static int detect_uniform(pgx_handle* h, GridLevel& L) {
  L.uniform = 0;
  L.interior_free = 0;
  if (L.nx < 2 || L.ny < 2) return PGX_OK;
  std::vector<double> K((size_t)7 * L.n), M((size_t)7 * L.n);
  HIPCHK(hipMemcpyAsync(K.data(), L.K, K.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(M.data(), L.M, M.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  const int sx = L.nx + 1;
  const int v0 = sx + 1;
  double kmax = 0, mmax = 0;
  for (int s = 0; s < 7; ++s) {
    L.Kc[s] = K[(size_t)s * L.n + v0];
    L.Mc[s] = M[(size_t)s * L.n + v0];
    kmax = std::max(kmax, std::fabs(L.Kc[s]));
    mmax = std::max(mmax, std::fabs(L.Mc[s]));
  }
  bool same = true;
  for (int j = 1; j < L.ny && same; ++j)
    for (int i = 1; i < L.nx && same; ++i) {
      const size_t v = (size_t)j * sx + i;
      for (int s = 0; s < 7; ++s)
        if (std::fabs(K[(size_t)s * L.n + v] - L.Kc[s]) > 1e-11 * kmax ||
            std::fabs(M[(size_t)s * L.n + v] - L.Mc[s]) > 1e-11 * mmax) {
          same = false;
          break;
        }
    }
  L.uniform = same ? 1 : 0;
  std::vector<uint8_t> mk(L.n);
  HIPCHK(hipMemcpyAsync(mk.data(), L.mask, L.n, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  L.interior_free = 1;
  for (int j = 1; j < L.ny && L.interior_free; ++j)
    for (int i = 1; i < L.nx; ++i)
      if (mk[(size_t)j * sx + i]) {
        L.interior_free = 0;
        break;
      }
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// sharded path: strip partition arithmetic (no GPU needed)
// ------------------------------------------------------------------------------------------------
// Ghost depth multiplier m (PGX_GHOST_MUL, default 3; every rank must see the same value): distributed level l keeps m 2^(ld-l)
// ghost rows (24 / 12 / 6 for three distributed levels).  An exchange restores validity depth g and a fused smoother launch
// consumes K = 3 of it, so deeper ghosts trade redundant rows (m 2^ld per strip side on the finest level: +19 % of a 256-row
// strip at m = 3) for fewer latency-bound exchanges: 14.2 / 9.2 / 6.2 / 6.2 per Krylov iteration at m = 1 / 2 / 3 / 4
// (pgx_comm_counts, 2048^2 on 4 strips).
int ghost_mul() {
  static const int m = [] {
    const char* e = pgx_tune("PGX_GHOST_MUL");
    const int v = e ? atoi(e) : 3;
    return v >= 1 && v <= 4 ? v : 3;
  }();
  return m;
}

static int partition_resolve(pgx_partition* pt, std::string& err) {
  if (!pt || pt->size < 1 || pt->rank < 0 || pt->rank >= pt->size || pt->global_ny < 1 || pt->dist_levels < 0) {
    err = "pgx_partition: need 0 <= rank < size, global_ny >= 1, dist_levels >= 0";
    return PGX_EINVAL;
  }
  if (pt->global_ny % pt->size) {
    err = "pgx_partition: global_ny must be divisible by the number of strips";
    return PGX_EINVAL;
  }
  const int Hh = pt->global_ny / pt->size;
  // level l keeps Hh/2^l owned rows and 2^(ld-l) ghost rows: strips must coarsen ld times and still own g+1 = 3 rows
  auto ok = [&](int l) { return l >= 1 && l <= 8 && Hh % (1 << l) == 0 && (Hh >> (l - 1)) >= 4 * ghost_mul(); };
  int ld = pt->dist_levels;
  if (ld == 0) {
    for (ld = 3; ld >= 1 && !ok(ld); --ld) {}
    if (ld < 1) {
      err = "pgx_partition: strips too thin to shard (need global_ny / size divisible by 2 and >= 4)";
      return PGX_EINVAL;
    }
    pt->dist_levels = ld;
  } else if (!ok(ld)) {
    err = "pgx_partition: global_ny / size must be divisible by 2^dist_levels and leave >= 4 rows on the last distributed level";
    return PGX_EINVAL;
  }
  return PGX_OK;
}

extern "C" int pgx_partition_rows(pgx_partition* pt, int32_t* row0, int32_t* nrows, int32_t* own0, int32_t* nown) {
  std::string err;
  const int rc = partition_resolve(pt, err);
  if (rc) {
    g_create_error = err;
    return rc;
  }
  const int Hh = pt->global_ny / pt->size, g0 = ghost_mul() << pt->dist_levels;
  const int r0 = pt->rank * Hh - (pt->rank > 0 ? g0 : 0);
  const int r1 = (pt->rank + 1 < pt->size) ? (pt->rank + 1) * Hh + g0 : pt->global_ny;  // last local vertex row
  if (row0) *row0 = r0;
  if (nrows) *nrows = r1 - r0 + 1;
  if (own0) *own0 = pt->rank * Hh;
  if (nown) *nown = Hh + (pt->rank + 1 == pt->size ? 1 : 0);
  return PGX_OK;
}

// fused tail: every level from `first` on with at most PGX_TAIL_VERTS vertices (and at most PGX_TAIL_MAX of them)
static void setup_tail(pgx_handle* h, int first) {
  const int nl = (int)h->lev.size();
  {  // a coarsest grid that could not be coarsened to a handful of vertices (odd cell counts) gets a sweep
     // count that grows with its size: Jacobi is then a poor but non-trivial coarse solver
    const GridLevel& Lc = h->lev.back();
    if (nl > 1 && Lc.n > 100 && !pgx_tune("PGX_COARSE_SWEEPS")) h->coarse_sweeps = std::min(400, 4 * std::max(Lc.nx, Lc.ny));
  }
  for (int l = std::max(first, 1); l < nl; ++l)
    if (h->lev[l].n <= h->tail_verts && nl - l <= PGX_TAIL_MAX) {
      h->tail_start = l;
      break;
    }
  if (h->tail_start > 0) {
    h->tail.nlev = nl - h->tail_start;
    for (int l = h->tail_start; l < nl; ++l) {
      const GridLevel& L = h->lev[l];
      TailLevel& T = h->tail.L[l - h->tail_start];
      T.nx = L.nx;
      T.ny = L.ny;
      T.n = L.n;
      T.K = L.K;
      T.M = L.M;
      T.Dh = L.Dh;
      for (int s = 0; s < 7; ++s) {
        T.sc.K[s] = L.Kc[s];
        T.sc.M[s] = L.Mc[s];
      }
      T.sc.uniform = L.uniform;
      T.interior_free = L.interior_free;
      T.mask = L.mask;
      T.xu = L.xu;
      T.xp = L.xp;
      T.xu2 = L.xu2;
      T.xp2 = L.xp2;
      T.bu = L.bu;
      T.bp = L.bp;
      T.ru = L.ru;
      T.rp = L.rp;
    }
  }
}

// Coarsest grid of the hierarchy: coarsening stops at this many cells per side (PGX_MG_MIN_NX).  Round 4: 4 instead of 2 - the 3 x 3
// grid has ONE interior vertex and its visit costs the fused tail 8 us per V-cycle (46.6 -> 38.7 us) for nothing: identical Krylov
// and Newton counts on every test and on the 2048^2 benchmark.
static int mg_min_nx() {
  const char* e = pgx_tune("PGX_MG_MIN_NX");
  return e ? std::max(2, atoi(e)) : 4;
}

// Which levels run the single-precision legs (pgx_mg32.hip): every level with uniform stencils (the row-mapped kernels) and at
// least f32_min vertices above the fused tail, never the coarsest.  fp64 and single-precision levels may alternate: each hands its
// right-hand side down and its correction up in the format of the level that receives it (vcycle / vcycle_f / vcycle_dist_f).
static int setup_f32(pgx_handle* h) {
  if (h->structured && h->degree == 1 && h->spmv_stencil == 1 && h->spmv_d4 && !h->lev.empty() && h->lev[0].uniform && sizeof(dsten_t) == 8)
    DALLOC(h->lev[0].Dd4, h->lev[0].n);  // the operator apply's own copy of D (k_st_spmv_r)
  if (!h->mg_f32 || !h->structured || sizeof(dsten_t) != 8) return PGX_OK;
  const int nl = (int)h->lev.size();
  for (int l = 0; l + 1 < nl; ++l) {
    GridLevel& L = h->lev[l];
    if (!L.uniform || L.n < std::max(h->f32_min, h->fused_min) || (h->tail_start > 0 && l >= h->tail_start)) continue;
    L.dbf16 = h->f32_dbf16 ? 1 : 0;
    if (L.dbf16) {
      uint2* q = nullptr;
      DALLOC(q, L.n);
      L.Dq = q;
    } else {
      float4* q = nullptr;
      DALLOC(q, L.n);
      L.Dq = q;
    }
    DALLOC(L.xf, L.n);
    DALLOC(L.xf2, L.n);
    DALLOC(L.bf, L.n);
    for (float2* p : {L.xf, L.xf2, L.bf}) HIPCHK(hipMemsetAsync(p, 0, sizeof(float2) * L.n, h->st));
    HIPCHK(hipMemsetAsync(L.Dq, 0, (L.dbf16 ? sizeof(uint2) : sizeof(float4)) * L.n, h->st));
    L.f32 = 1;
  }
  return PGX_OK;
}

// all solver-side arrays of one stencil level (K, M are filled by the caller)
static int alloc_level(pgx_handle* h, GridLevel& L, bool contiguous_rhs) {
  DALLOC(L.K, (size_t)7 * L.n);
  DALLOC(L.M, (size_t)7 * L.n);
  DALLOC(L.Dh, (size_t)4 * L.n);
  DALLOC(L.mask, L.n);
  DALLOC(L.xu, L.n);
  DALLOC(L.xp, L.n);
  DALLOC(L.xu2, L.n);
  DALLOC(L.xp2, L.n);
  if (contiguous_rhs) {  // (bu | bp) in one block: one memset + one all-reduce for the pair
    DALLOC(L.bu, (size_t)2 * L.n);
    L.bp = L.bu + L.n;
  } else {
    DALLOC(L.bu, L.n);
    DALLOC(L.bp, L.n);
  }
  DALLOC(L.ru, L.n);
  DALLOC(L.rp, L.n);
  return PGX_OK;
}

// Level 0 of the stencil hierarchy: the handle's grid and mask; on a structured mesh K and M as seven-point stencils, converted from
// the CSR values.  A general mesh keeps the bare entry: its level 0 is the block CSR itself.
static int stencil_level0(pgx_handle* h) {
  GridLevel L0{};
  L0.nx = h->nx;
  L0.ny = h->ny;
  L0.n = h->n;
  L0.mask = h->mask;
  h->lev.push_back(L0);
  if (!h->structured) return PGX_OK;
  DALLOC(h->lev[0].K, (size_t)7 * h->n);
  DALLOC(h->lev[0].M, (size_t)7 * h->n);
  DALLOC(h->lev[0].Dh, (size_t)4 * h->n);
  if (h->smooth_d32 && sizeof(dsten_t) == 8) DALLOC(h->lev[0].Dh32, (size_t)4 * h->n);
  pgxk_csr_to_stencil(h->st, h->n, h->nx + 1, h->rowptr, h->colm, h->Kv, h->lev[0].K);
  pgxk_csr_to_stencil(h->st, h->n, h->nx + 1, h->rowptr, h->colm, h->Mv, h->lev[0].M);
  return detect_uniform(h, h->lev[0]);
}

// One vertex coarsening of the last level: the nx x ny grid below it, its mask by injection, K and M as Galerkin products.
static int coarsen_level(pgx_handle* h, int nx, int ny, bool contiguous_rhs) {
  GridLevel L{};
  L.nx = nx;
  L.ny = ny;
  L.n = (nx + 1) * (ny + 1);
  int rc = alloc_level(h, L, contiguous_rhs);
  if (rc) return rc;
  const GridLevel& Fl = h->lev.back();
  pgxk_coarse_mask(h->st, L, L.mask, Fl);
  pgxk_rap7(h->st, Fl, Fl.K, L, L.K);
  pgxk_rap7(h->st, Fl, Fl.M, L, L.M);
  rc = detect_uniform(h, L);
  if (rc) return rc;
  h->lev.push_back(L);
  return PGX_OK;
}

int build_multigrid(pgx_handle* h) {
  int rc = stencil_level0(h);
  if (rc || !h->structured) return rc;
  int nx = h->nx, ny = h->ny;
  const int min_nx = mg_min_nx();
  while (nx % 2 == 0 && ny % 2 == 0 && nx > min_nx && ny > min_nx) {
    nx /= 2;
    ny /= 2;
    rc = coarsen_level(h, nx, ny, false);
    if (rc) return rc;
  }
  setup_tail(h, 1);
  rc = setup_f32(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}

// Sharded hierarchy: levels [0, ldist) are this rank's strips (ghost depth 2^(ldist-l)); level ldist and below are the
// GLOBAL grids, replicated on every rank.  Galerkin coarsening of a strip needs no communication: a coarse stencil at
// ghost depth d uses fine stencils up to depth 2d+1, so "valid up to depth g-1" is inherited from level to level.  Only
// the step onto the first replicated level merges the ranks' rows (owned rows, zeros elsewhere, one all-reduce).
int build_multigrid_dist(pgx_handle* h) {
  Dist& D = h->dist;
  const int ld = D.ldist;
  int rc = stencil_level0(h);
  if (rc) return rc;
  for (int l = 1; l < ld; ++l) {
    rc = coarsen_level(h, h->lev.back().nx / 2, h->lev.back().ny / 2, false);
    if (rc) return rc;
  }
  // first replicated level: the global grid, and this rank's view of it
  const GridLevel Fl = h->lev.back();
  GridLevel G{};
  G.nx = h->nx >> ld;
  G.ny = D.global_ny >> ld;
  G.n = (G.nx + 1) * (G.ny + 1);
  rc = alloc_level(h, G, true);
  if (rc) return rc;
  const int sxc = G.nx + 1;
  const int Hh = D.global_ny / D.size;
  D.view_own0 = (D.rank * Hh) >> ld;
  D.view_glo = D.rank > 0 ? ghost_mul() : 0;  // the last strip level has 2m ghost rows below and 2m + 1 above
  D.view_H = (Hh >> ld) + (D.rank + 1 == D.size ? 1 : 0);
  D.view_row0 = D.view_own0 - D.view_glo;
  GridLevel& V = D.view;
  V = G;
  V.ny = Fl.ny / 2;
  V.n = sxc * (V.ny + 1);
  if (V.nx * 2 != Fl.nx || D.view_row0 + V.ny > G.ny || V.ny + 1 != D.view_glo + D.view_H + (D.rank + 1 < D.size ? ghost_mul() + 1 : 0)) {
    h->err = "sharded hierarchy: strip view of the first replicated level is inconsistent";
    return PGX_EINVAL;
  }
  const size_t voff = (size_t)D.view_row0 * sxc;
  V.mask = G.mask + voff;
  V.xu = G.xu + voff;
  V.xp = G.xp + voff;
  V.bu = G.bu + voff;
  V.bp = G.bp + voff;
  V.K = V.M = nullptr;  // a view carries vectors and the mask only
  V.Dh = nullptr;
  DALLOC(D.view_S, (size_t)7 * V.n);
  for (int which = 0; which < 2; ++which) {
    pgxk_rap7(h->st, Fl, which ? Fl.M : Fl.K, V, D.view_S);
    double* dst = which ? G.M : G.K;
    pgxk_view_to_global(h->st, 7, V.n, G.n, sxc, D.view_row0, D.view_own0, D.view_H, D.view_S, dst);
    rc = allreduce_dev(h, dst, (size_t)7 * G.n);
    if (rc) return rc;
  }
  {  // Dirichlet mask of the replicated level: injection on the strip, merged like the stencils (setup only)
    uint8_t* vm = nullptr;
    DALLOC(vm, V.n);
    GridLevel Vm = V;
    pgxk_coarse_mask(h->st, Vm, vm, Fl);
    std::vector<uint8_t> hv(V.n);
    HIPCHK(hipMemcpyAsync(hv.data(), vm, V.n, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    std::vector<double> hg(G.n, 0.0);
    for (int J = D.view_own0; J < D.view_own0 + D.view_H; ++J)
      for (int I = 0; I < sxc; ++I) hg[(size_t)J * sxc + I] = hv[(size_t)(J - D.view_row0) * sxc + I];
    HIPCHK(hipMemcpyAsync(G.ru, hg.data(), sizeof(double) * G.n, hipMemcpyHostToDevice, h->st));
    rc = allreduce_dev(h, G.ru, G.n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(hg.data(), G.ru, sizeof(double) * G.n, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    std::vector<uint8_t> gm(G.n);
    for (int v = 0; v < G.n; ++v) gm[v] = hg[v] != 0.0;
    HIPCHK(hipMemcpy(G.mask, gm.data(), G.n, hipMemcpyHostToDevice));
  }
  rc = detect_uniform(h, G);
  if (rc) return rc;
  D.view.interior_free = G.interior_free;  // the view's mask is a row slice of G's
  h->lev.push_back(G);
  int nx = G.nx, ny = G.ny;
  const int min_nx = mg_min_nx();
  while (nx % 2 == 0 && ny % 2 == 0 && nx > min_nx && ny > min_nx) {
    nx /= 2;
    ny /= 2;
    rc = coarsen_level(h, nx, ny, false);
    if (rc) return rc;
  }
  setup_tail(h, ld);
  rc = setup_f32(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// Hierarchy of a refined general mesh (include/pgx.h: pgx_set_hierarchy).  Host symbolic pass per transfer: the coarse pattern
// P^T (pattern) P, per coarse entry the list of fine entries that sum into it (the Galerkin plan of k_umg_rap, items sorted by fine
// entry index), and per coarse vertex its child list (P^T as CSR, children in ascending order: the vertex itself first).  Then K and
// M of every coarse level, once; D follows on every Jacobian fill (jacobian_dev).
// ------------------------------------------------------------------------------------------------
extern "C" int pgx_set_hierarchy(pgx_handle* h, int32_t n_transfers, const int32_t* n_coarse, const int32_t* const* parents) {
  NEED(h);
  if (!h->umg.empty()) {
    h->err = "pgx_set_hierarchy: this handle already has a hierarchy";
    return PGX_ESTATE;
  }
  if (h->jac_ever) {
    h->err = "pgx_set_hierarchy comes before the first Jacobian fill";
    return PGX_ESTATE;
  }
  if (h->structured || h->dist.on || h->lu_comm) {
    h->err = "pgx_set_hierarchy: for single handles on general meshes (structured meshes have their grid hierarchy; sharded and "
             "LU-distributed handles have none of this kind)";
    return PGX_EINVAL;
  }
  if (n_transfers < 1 || !n_coarse || !parents) {
    h->err = "pgx_set_hierarchy: at least one transfer, with its coarse size and its parents array";
    return PGX_EINVAL;
  }
  if (h->nnz >= (1 << 30)) {
    h->err = "pgx_set_hierarchy: the Galerkin plan addresses fewer than 2^30 fine entries";
    return PGX_EINVAL;
  }
  {  // everything is checked before anything is built
    int nf = h->n;
    for (int t = 0; t < n_transfers; ++t) {
      const int nc = n_coarse[t];
      if (nc < 1 || nc >= nf) {
        h->err = "pgx_set_hierarchy: n_coarse must be strictly decreasing, below n_vertices (transfer " + std::to_string(t) + ")";
        return PGX_EINVAL;
      }
      const int32_t* P = parents[t];
      if (!P) {
        h->err = "pgx_set_hierarchy: null parents array (transfer " + std::to_string(t) + ")";
        return PGX_EINVAL;
      }
      for (int v = 0; v < nf; ++v) {
        const int p0 = P[2 * v], p1 = P[2 * v + 1];
        if (p0 < 0 || p1 < 0 || p0 >= nc || p1 >= nc) {
          h->err = "pgx_set_hierarchy: parent index outside the coarse level (transfer " + std::to_string(t) + ", vertex " + std::to_string(v) + ")";
          return PGX_EINVAL;
        }
        if (v < nc ? (p0 != v || p1 != v) : (p0 == p1)) {
          h->err = "pgx_set_hierarchy: the first n_coarse rows of a transfer are (v, v), the others the two ends of an edge (transfer " +
                   std::to_string(t) + ", vertex " + std::to_string(v) + ")";
          return PGX_EINVAL;
        }
      }
      nf = nc;
    }
  }
  std::vector<UmgLevel> lv(n_transfers + 1);
  {
    const int rc = umg_level0(h, lv[0]);
    if (rc) return rc;
  }
  for (int t = 0; t < n_transfers; ++t) {
    const UmgLevel& F = lv[t];
    UmgLevel& C = lv[t + 1];
    const int nf = F.n, nc = n_coarse[t];
    const int32_t* P = parents[t];
    C.n = nc;
    // items of coarse row I: (coarse column, fine entry | s << 30), from every fine entry (i, j) with I a parent of i
    std::vector<int64_t> rcount(nc + 1, 0);
    auto np_of = [&](int v) { return v < nc ? 1 : 2; };
    for (int i = 0; i < nf; ++i) {
      int64_t items = 0;
      for (int e = F.h_rowptr[i]; e < F.h_rowptr[i + 1]; ++e) items += np_of(F.h_col[e]);
      for (int a = 0; a < np_of(i); ++a) rcount[P[2 * i + a] + 1] += items;
    }
    for (int I = 0; I < nc; ++I) rcount[I + 1] += rcount[I];
    struct Item {
      int32_t col, src;
    };
    std::vector<Item> items((size_t)rcount[nc]);
    {
      std::vector<int64_t> pos(rcount.begin(), rcount.end() - 1);
      for (int i = 0; i < nf; ++i)
        for (int a = 0; a < np_of(i); ++a) {
          const int I = P[2 * i + a];
          for (int e = F.h_rowptr[i]; e < F.h_rowptr[i + 1]; ++e) {
            const int j = F.h_col[e];
            const int32_t s = (i >= nc ? 1 : 0) + (j >= nc ? 1 : 0);
            for (int b = 0; b < np_of(j); ++b) items[(size_t)pos[I]++] = Item{P[2 * j + b], (int32_t)((uint32_t)e | ((uint32_t)s << 30))};
          }
        }
    }
    C.h_rowptr.assign(nc + 1, 0);
    std::vector<int32_t> plan_ptr(1, 0), plan_src;
    plan_src.reserve(items.size());
    for (int I = 0; I < nc; ++I) {
      Item* const b = items.data() + rcount[I];
      Item* const e = items.data() + rcount[I + 1];
      std::sort(b, e, [](const Item& x, const Item& y) {
        return x.col != y.col ? x.col < y.col : (x.src & 0x3fffffff) < (y.src & 0x3fffffff);
      });
      for (Item* q = b; q < e; ++q) {
        if (q == b || q->col != (q - 1)->col) {
          if (q != b) plan_ptr.push_back((int32_t)plan_src.size());
          C.h_col.push_back(q->col);
        }
        plan_src.push_back(q->src);
      }
      if (b != e) plan_ptr.push_back((int32_t)plan_src.size());
      C.h_rowptr[I + 1] = (int32_t)C.h_col.size();
    }
    if (plan_src.size() >= ((size_t)1 << 31)) {
      h->err = "pgx_set_hierarchy: Galerkin plan exceeds int32";
      return PGX_EINVAL;
    }
    C.nnz = (int)C.h_col.size();
    const double plan_mean = C.nnz ? (double)plan_src.size() / C.nnz : 0.0;
    // red refinement gives plan rows of 10.6 ... 12.1 items on average (at most 41): three items per lane, or two where rows run longer
    C.plan_lpe = plan_mean <= 11.5 ? 4 : 8;
    C.h_mask.assign(F.h_mask.begin(), F.h_mask.begin() + nc);  // the fine mask on the inherited vertices
    std::vector<int32_t> colm(C.nnz), ch_ptr(nc + 1, 0), ch_idx;
    for (int e = 0; e < C.nnz; ++e) colm[e] = (int32_t)((uint32_t)C.h_col[e] | (C.h_mask[C.h_col[e]] ? 0x80000000u : 0u));
    for (int v = 0; v < nf; ++v)
      for (int a = 0; a < np_of(v); ++a) ++ch_ptr[P[2 * v + a] + 1];
    for (int I = 0; I < nc; ++I) ch_ptr[I + 1] += ch_ptr[I];
    ch_idx.resize(ch_ptr[nc]);
    {
      std::vector<int32_t> pos(ch_ptr.begin(), ch_ptr.end() - 1);
      for (int v = 0; v < nf; ++v)
        for (int a = 0; a < np_of(v); ++a) ch_idx[pos[P[2 * v + a]]++] = v;
    }
    std::vector<int32_t> par(P, P + 2 * (size_t)nf);
    int rc;
    if ((rc = umg_upload(h, &C.rowptr, C.h_rowptr)) || (rc = umg_upload(h, &C.colm, colm)) || (rc = umg_upload(h, &C.mask, C.h_mask)) ||
        (rc = umg_upload(h, &C.parents, par)) || (rc = umg_upload(h, &C.ch_ptr, ch_ptr)) || (rc = umg_upload(h, &C.ch_idx, ch_idx)) ||
        (rc = umg_upload(h, &C.plan_ptr, plan_ptr)) || (rc = umg_upload(h, &C.plan_src, plan_src)))
      return rc;
    DALLOC(C.K, C.nnz);
    DALLOC(C.M, C.nnz);
    DALLOC(C.D, C.nnz);
    double** const vecs[8] = {&C.bu, &C.bp, &C.xu, &C.xp, &C.xu2, &C.xp2, &C.ru, &C.rp};
    for (double** v : vecs) DALLOC(*v, nc);
    HIPCHK(hipStreamSynchronize(h->st));  // the uploads read host vectors that end with this iteration
  }
  for (int l = 1; l <= n_transfers; ++l) {
    const UmgLevel& C = lv[l];
    pgxk_umg_rap(h->st, C.nnz, C.plan_lpe, C.plan_ptr, C.plan_src, lv[l - 1].K, C.K);
    pgxk_umg_rap(h->st, C.nnz, C.plan_lpe, C.plan_ptr, C.plan_src, lv[l - 1].M, C.M);
  }
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  umg_install(h, std::move(lv));
  return PGX_OK;
}
