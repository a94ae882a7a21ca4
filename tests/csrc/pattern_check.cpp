// pattern_check - stand-alone driver of proximalgalerkin_amd/csrc/pgx_pattern.h for tests/test_cpu_pattern.py (no GPU, no HIP).
// Reads one request from the file named on the command line and prints the arrays the builders return, one per line:
//   p1 <n_vertices> <n_cells> <keep_diagonal>  then 3 n_cells vertex ids      -> "error <text>" | "sptr ..." "scol ..."
//   entities <ntot> <nu> <n_entities>          then per entity "<count> dofs...", then nu mask bytes
//                                                                              -> "error <text>" | "rowptr ..." "col ..." "kind ..." "find <ok>"
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../proximalgalerkin_amd/csrc/pgx_pattern.h"

template <typename V>
static void print(const char* name, const V& v) {
  std::cout << name;
  for (auto x : v) std::cout << ' ' << (long)x;
  std::cout << '\n';
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string mode;
  in >> mode;
  if (mode == "p1") {
    int nv, nc, keep;
    in >> nv >> nc >> keep;
    std::vector<int32_t> cells(3 * (size_t)nc);
    for (auto& c : cells) in >> c;
    if (!in) return 2;
    if (const char* e = check_cells(cells.data(), 3, nc, nv)) {
      std::cout << "error " << e << '\n';
      return 0;
    }
    std::vector<int32_t> sptr, scol;
    p1_adjacency(nv, nc, cells.data(), keep != 0, sptr, scol);
    print("sptr", sptr);
    print("scol", scol);
    return 0;
  }
  if (mode == "entities") {
    int64_t ntot, nu, ne;
    in >> ntot >> nu >> ne;
    std::vector<int64_t> eptr(ne + 1, 0);
    std::vector<int32_t> edofs;
    for (int64_t e = 0; e < ne; ++e) {
      int n;
      in >> n;
      for (int a = 0; a < n; ++a) {
        int32_t d;
        in >> d;
        edofs.push_back(d);
      }
      eptr[e + 1] = (int64_t)edofs.size();
    }
    std::vector<uint8_t> hmask(nu);
    for (auto& b : hmask) {
      int v;
      in >> v;
      b = (uint8_t)v;
    }
    if (!in) return 2;
    std::vector<int32_t> rowptr, col;
    std::string err;
    const PatFind find = pattern_from_entities(ntot, ne, [&](int64_t e, int32_t* out) {
      std::copy(edofs.begin() + eptr[e], edofs.begin() + eptr[e + 1], out);
      return (int)(eptr[e + 1] - eptr[e]);
    }, rowptr, col, err);
    if (!find) {
      std::cout << "error " << err << '\n';
      return 0;
    }
    std::vector<uint8_t> kind;
    saddle_kinds(ntot, nu, hmask, rowptr, col, kind);
    print("rowptr", rowptr);
    print("col", col);
    print("kind", kind);
    bool ok = true;  // the lookup returns the position of every entry of the pattern
    for (int64_t r = 0; r < ntot; ++r)
      for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) ok = ok && find((int32_t)r, col[k]) == k;
    std::cout << "find " << (ok ? 1 : 0) << '\n';
    return 0;
  }
  return 2;
}
