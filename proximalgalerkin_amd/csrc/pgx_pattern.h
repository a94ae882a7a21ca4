// pgx_pattern.h - the sparsity patterns of the mixed-matrix families, built on the host: the P1 vertex adjacency of a triangle mesh
// (pgx_fr / pgx_mp / pgx_qvi / pgx_qmy put their 3 x 3 or 2 x 2 blocks on it), the CSR pattern "row r couples to every dof of
// the entities that touch it" (pgx_gc, pgx_sg, pgx_sg2d), the slot kinds of a saddle-point matrix with Dirichlet rows, and the
// range check of a cell table.  Host code only, no HIP header: tests/csrc/pattern_check.cpp drives it without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

// fn(a, b) over [0, n) in at most 16 chunks on host threads (one chunk below 20000: the builders are memory bound)
template <typename Fn>
static void pat_par_for(int64_t n, const Fn& fn) {
  unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < 20000) T = 1;
  std::vector<std::thread> th;
  const int64_t chunk = (n + T - 1) / T;
  for (unsigned t = 0; t < T; ++t) {
    const int64_t a = t * chunk, b = std::min<int64_t>(n, a + chunk);
    if (a >= b) break;
    th.emplace_back([=, &fn] { fn(a, b); });
  }
  for (auto& t : th) t.join();
}

// null, or the message the families report if an entry of cells[n_cells][nodes_per_cell] is no vertex id
static inline const char* check_cells(const int32_t* cells, int nodes_per_cell, int64_t n_cells, int n_vertices) {
  for (size_t k = 0; k < (size_t)nodes_per_cell * (size_t)n_cells; ++k)
    if (cells[k] < 0 || cells[k] >= n_vertices) return "cell vertex out of range";
  return nullptr;
}

// Scalar P1 pattern of a triangle mesh: row v holds, ascending, the vertices of the cells around v.  keep_diagonal: v itself is
// in its row even when no cell touches it (a row of length 1 instead of 0).
static inline void p1_adjacency(int n_vertices, int n_cells, const int32_t* cells, bool keep_diagonal, std::vector<int32_t>& sptr,
                                std::vector<int32_t>& scol) {
  const int nv = n_vertices, nc = n_cells;
  std::vector<int64_t> vptr(nv + 1, 0);
  for (size_t k = 0; k < 3 * (size_t)nc; ++k) vptr[cells[k] + 1]++;
  for (int v = 0; v < nv; ++v) vptr[v + 1] += vptr[v];
  std::vector<int32_t> vcell(vptr[nv]);
  {
    std::vector<int64_t> fill(vptr.begin(), vptr.end() - 1);
    for (int c = 0; c < nc; ++c)
      for (int a = 0; a < 3; ++a) vcell[fill[cells[3 * (size_t)c + a]]++] = c;
  }
  std::vector<std::vector<int32_t>> rows(nv);
  pat_par_for(nv, [&](int64_t a, int64_t b) {
    for (int64_t v = a; v < b; ++v) {
      auto& r = rows[v];
      if (keep_diagonal) r.push_back((int32_t)v);
      for (int64_t q = vptr[v]; q < vptr[v + 1]; ++q)
        for (int k = 0; k < 3; ++k) r.push_back(cells[3 * (size_t)vcell[q] + k]);
      std::sort(r.begin(), r.end());
      r.erase(std::unique(r.begin(), r.end()), r.end());
    }
  });
  sptr.assign(nv + 1, 0);
  for (int v = 0; v < nv; ++v) sptr[v + 1] = sptr[v] + (int32_t)rows[v].size();
  scol.resize(sptr[nv]);
  for (int v = 0; v < nv; ++v) std::copy(rows[v].begin(), rows[v].end(), scol.begin() + sptr[v]);
}

// position of entry (r, c) of a CSR pattern with ascending rows; (r, c) must be in the pattern
struct PatFind {
  const int32_t *rowptr, *col;
  explicit operator bool() const { return rowptr != nullptr; }  // false: the builder failed
  int32_t operator()(int32_t r, int32_t c) const {
    return (int32_t)(std::lower_bound(col + rowptr[r], col + rowptr[r + 1], c) - col);
  }
};

// the builder's stack buffer for one entity; every caller static_asserts its largest entity against it (gc of general degree:
// 81 + 2 * 64, sg on Q2 hexahedra: 81)
#define PAT_MAX_ENTITY_DOFS 256

// CSR pattern of ntot dofs in which row r holds, ascending, every dof of the entities that contain r.  dofs_of(entity, out)
// writes the dofs of one entity (at most PAT_MAX_ENTITY_DOFS) and returns their count; cells and facets go in as one range.
// Returns the position lookup over rowptr / col; on overflow it is false, err is set and rowptr / col are not to be used.
template <typename DofsOf>
static PatFind pattern_from_entities(int64_t ntot, int64_t n_entities, const DofsOf& dofs_of, std::vector<int32_t>& rowptr,
                                     std::vector<int32_t>& col, std::string& err) {
  // dof -> entities
  std::vector<int64_t> dptr(ntot + 1, 0);
  for (int64_t e = 0; e < n_entities; ++e) {
    int32_t md[PAT_MAX_ENTITY_DOFS];
    const int n = dofs_of(e, md);
    for (int a = 0; a < n; ++a) dptr[md[a] + 1]++;
  }
  for (int64_t i = 0; i < ntot; ++i) dptr[i + 1] += dptr[i];
  std::vector<int64_t> dent(dptr[ntot]);
  {
    std::vector<int64_t> fill(dptr.begin(), dptr.end() - 1);
    for (int64_t e = 0; e < n_entities; ++e) {
      int32_t md[PAT_MAX_ENTITY_DOFS];
      const int n = dofs_of(e, md);
      for (int a = 0; a < n; ++a) dent[fill[md[a]]++] = e;
    }
  }
  auto gather_row = [&](int64_t r, std::vector<int32_t>& tmp) {
    tmp.clear();
    for (int64_t q = dptr[r]; q < dptr[r + 1]; ++q) {
      int32_t md[PAT_MAX_ENTITY_DOFS];
      const int n = dofs_of(dent[q], md);
      tmp.insert(tmp.end(), md, md + n);
    }
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
  };
  rowptr.assign(ntot + 1, 0);
  pat_par_for(ntot, [&](int64_t a, int64_t b) {
    std::vector<int32_t> tmp;
    for (int64_t r = a; r < b; ++r) {
      gather_row(r, tmp);
      rowptr[r + 1] = (int32_t)tmp.size();
    }
  });
  int64_t tot = 0;
  for (int64_t r = 0; r < ntot; ++r) {
    tot += rowptr[r + 1];
    if (tot > 0x7fffffff) {
      err = "mixed matrix exceeds int32 nnz";
      return PatFind{nullptr, nullptr};
    }
    rowptr[r + 1] = (int32_t)tot;
  }
  col.resize(tot);
  pat_par_for(ntot, [&](int64_t a, int64_t b) {
    std::vector<int32_t> tmp;
    for (int64_t r = a; r < b; ++r) {
      gather_row(r, tmp);
      std::copy(tmp.begin(), tmp.end(), col.begin() + rowptr[r]);
    }
  });
  return PatFind{rowptr.data(), col.data()};
}

// Slot kinds of the saddle-point matrix [[A, B^T], [B, D]] whose first nu rows carry the Dirichlet mask hmask[nu]:
// 0 = A slot, 1 = off-diagonal block slot, 2 = D slot, 3 = Dirichlet diagonal, 4 = zeroed by a Dirichlet row or column
static inline void saddle_kinds(int64_t ntot, int64_t nu, const std::vector<uint8_t>& hmask, const std::vector<int32_t>& rowptr,
                                const std::vector<int32_t>& col, std::vector<uint8_t>& kind) {
  kind.resize(col.size());
  pat_par_for(ntot, [&](int64_t a, int64_t b) {
    for (int64_t r = a; r < b; ++r)
      for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
        const int32_t c = col[k];
        uint8_t t;
        if (r < nu && c < nu)
          t = (hmask[r] || hmask[c]) ? ((r == c && hmask[r]) ? 3 : 4) : 0;
        else if (r < nu)
          t = hmask[r] ? 4 : 1;
        else if (c < nu)
          t = hmask[c] ? 4 : 1;
        else
          t = 2;
        kind[k] = t;
      }
  });
}
