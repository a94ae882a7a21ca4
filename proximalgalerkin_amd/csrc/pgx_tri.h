// pgx_tri.h - what the P1-triangle element kernels of pgx_fr / pgx_mp / pgx_qvi / pgx_qmy share on the device: the affine geometry
// of a cell, the exact P1 mass matrix entry, and the quadrature table that travels as a kernel argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct TriGeom {
  double G[3][2];  // physical P1 gradients
  double adet;     // |det J| = 2 area
};
// the overload a kernel calls when it needs the vertex coordinates X too
__device__ inline TriGeom tri_geom(const double* __restrict__ coords, const int32_t* __restrict__ cv, double X[3][2]) {
  TriGeom g;
  for (int a = 0; a < 3; ++a) X[a][0] = coords[2 * (size_t)cv[a]], X[a][1] = coords[2 * (size_t)cv[a] + 1];
  const double j00 = X[1][0] - X[0][0], j10 = X[1][1] - X[0][1];
  const double j01 = X[2][0] - X[0][0], j11 = X[2][1] - X[0][1];
  const double det = j00 * j11 - j01 * j10;
  const double i00 = j11 / det, i01 = -j01 / det, i10 = -j10 / det, i11 = j00 / det;
  // G[a][d] = sum_k gref[a][k] inv[k][d], gref = [[-1,-1],[1,0],[0,1]]
  g.G[1][0] = i00, g.G[1][1] = i01;
  g.G[2][0] = i10, g.G[2][1] = i11;
  g.G[0][0] = -(i00 + i10), g.G[0][1] = -(i01 + i11);
  g.adet = fabs(det);
  return g;
}
__device__ inline TriGeom tri_geom(const double* __restrict__ coords, const int32_t* __restrict__ cv) {
  double X[3][2];
  return tri_geom(coords, cv, X);
}
// int phi_a phi_b over a triangle of the given area
__device__ inline double tri_me(double area, int a, int b) { return area / 12.0 * (a == b ? 2.0 : 1.0); }

// P1 basis values and weights at the caller's reference points (kernel argument: the loop index is uniform, so the table is read
// with scalar loads)
template <int MAXQ>
struct TriQuad {
  double N[MAXQ][3], w[MAXQ];
  int nq;
  void fill(const double* qpts, const double* qwts, int n) {  // host; qpts [n][2] on the reference triangle, n <= MAXQ
    nq = n;
    for (int q = 0; q < n; ++q) {
      const double X = qpts[2 * q], Y = qpts[2 * q + 1];
      N[q][0] = 1.0 - X - Y, N[q][1] = X, N[q][2] = Y, w[q] = qwts[q];
    }
  }
};
