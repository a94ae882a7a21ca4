// pgx_ek.hip - example 09 (the eikonal equation on a Moebius strip: u in Q1, psi in [Q2]^3 on quadrilaterals embedded in R^3 with
// curved geometry of order g <= 3) behind the C ABI of include/pgx_ek.h.  Reference: examples/09_eikonal/eikonal_dolfinx.py (:29-32
// spaces, :52-58 residual, :61 Jacobian, :65-77 solver, :88-90 norm, :84-86 and :134-148 DG outputs, :149-174 loop).
// x = [u | psi0 | psi1 | psi2].  The Jacobian
//     rows v     : [ 0     B0    B1    B2  ]      B_i = (div_G (psi_i e_i), v) = (grad_G N2 . e_i, N1)
//     rows tau_i : [ B_i^T D_i0  D_i1  D_i2 ]     D_ij = mass form weighted by phi (delta_ij / s - psi_i psi_j / s^3)
// lives in one mixed CSR array; the (u, u) block stores nothing.
//
// What is computed when:
//   create        k_ek_geom   K = G^-1 J^T (6 doubles) and w dS per cell and quadrature point, stored: [cell][7][points]
//                 k_ek_const  the element blocks of B and of the load (f, v); summed per destination into Jc (B AND B^T from the same
//                             element values) and into fv
//   Newton step   k_ek_lin    F = Jc [u; psi - psi_prev] + alpha [fv; 0]: the linear part of the residual, one thread per row
//                 k_ek_resid  the three weighted fields phi psi_i / s of a cell -> (.., tau)
//                 k_ek_jac    the six weighted fields of D(psi) of a cell -> 45 symmetric Q2 node pairs
//
// Element kernels: ONE WAVEFRONT PER CELL, EK_WPB cells per workgroup, as k_ev_*.  Phase 1: lanes over the quadrature points (nq = 8:
// exactly 64; up to 121 in a second round) evaluate psi through the 1-D tables and leave the weighted coefficient fields in LDS.
// Phase 2: lanes over the 45 symmetric node pairs (Jacobian) or the 27 local rows (residual) sum over the points; every lane reads
// the same coefficient address (a broadcast).  Results are parked cell-major and summed per destination in a fixed order by
// pgx_scatter.h: no atomics, bitwise reproducible; both triangles of a block, and B and B^T, receive the SAME sums in the same order,
// so the exported matrix is symmetric to the last bit.
#include <cstring>
#include <map>

#include "../../include/pgx_bd.h"
#include "../../include/pgx_dn.h"
#include "../../include/pgx_ek.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"

#define EK_MAXQ 11                     // points of the 1-D rule
#define EK_MAXPTS (EK_MAXQ * EK_MAXQ)  // 121
#define EK_WPB 4                       // cells (wavefronts) per workgroup
#define EK_NB2 9                       // Q2 nodes of a cell
#define EK_CW (4 * 3 * EK_NB2 + 4)     // constant stash per cell: B_e [a][i][b], then (f, v)_e [a]

// 1-D Lagrange tables on the nodes i / k, stride 4: T[p * 4 + i] = basis i at point p.  q*: at the Gauss points; n*: at the g + 1
// equispaced geometry nodes j / g (pgx_ek_eval_cells).
struct EkTab {
  double w[EK_MAXQ];
  double qB1[EK_MAXQ * 4], qD1[EK_MAXQ * 4], qB2[EK_MAXQ * 4], qD2[EK_MAXQ * 4], qBg[EK_MAXQ * 4], qDg[EK_MAXQ * 4];
  double nB1[16], nD1[16], nB2[16], nBg[16], nDg[16];
};

static thread_local std::string g_ek_error;

struct pgx_ek_handle : MixedBase {
  int nc = 0, g = 0, nq = 0, n1 = 0, n2 = 0;
  double f = 1.0, phi = 1.0;
  EkTab* tab = nullptr;
  double* nodes = nullptr;  // [nc][(g+1)^2][3]
  int32_t *cd1 = nullptr, *cd2 = nullptr;  // [nc][4], [nc][9]
  double* geo = nullptr;    // [nc][7][nq^2]: K row-major (K[r][i] at r * 3 + i), then w dS
  int32_t* bad = nullptr;   // set by k_ek_geom where det G is not positive and finite
  double* fv = nullptr;     // [n1] (f, v)
  double* Jc = nullptr;     // [nnz] iterate-independent part of the Jacobian: B and B^T
  double* stash = nullptr;  // [nc * max(6 * 81, EK_CW)]
  double* d_cells = nullptr;  // [nc][(g+1)^2][7] eval_cells
  PgxScatter sc_res, sc_jac, sc_jac_t, sc_B, sc_Bt, sc_fv;
  pgx_dn* dn = nullptr;  // the dense LU (pgx_ek_create) or
  pgx_bd* bd = nullptr;  // the band LU (pgx_ek_create_banded): exactly one of the two
  pgx_ek_handle() : MixedBase("pgx_ek") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
  int lin_factor() override { return bd ? pgx_bd_factor(bd, Jv, 1) : pgx_dn_factor(dn, Jv, 1); }
  int lin_solve(const double* rhs, double* out) override { return bd ? pgx_bd_solve(bd, rhs, out, 1) : pgx_dn_solve(dn, rhs, out, 1); }
  const char* lin_error() const override { return bd ? pgx_bd_last_error(bd) : pgx_dn_last_error(dn); }
  void lin_release() override {
    if (dn) pgx_dn_destroy(dn);
    if (bd) pgx_bd_destroy(bd);
    dn = nullptr, bd = nullptr;
  }
};

extern "C" const char* pgx_ek_last_error(const pgx_ek_handle* h) { return h ? h->err.c_str() : g_ek_error.c_str(); }

// K = G^-1 J^T (K[r * 3 + i]) and det G of the Q_g map with nodes X [(g+1)^2][3] at a point whose 1-D tables are by / dy (second
// reference direction) and bx / dx (first)
__device__ inline double ek_pinv(const double* __restrict__ X, int g1, const double* by, const double* dy, const double* bx,
                                 const double* dx, double K[6]) {
  double J0[3] = {0, 0, 0}, J1[3] = {0, 0, 0};  // dx/dX0, dx/dX1
  for (int ny = 0; ny < g1; ++ny)
    for (int nx = 0; nx < g1; ++nx) {
      const double a = by[ny] * dx[nx], b = dy[ny] * bx[nx];
      const double* P = X + 3 * (ny * g1 + nx);
#pragma unroll
      for (int i = 0; i < 3; ++i) J0[i] = fma(a, P[i], J0[i]), J1[i] = fma(b, P[i], J1[i]);
    }
  const double G00 = J0[0] * J0[0] + J0[1] * J0[1] + J0[2] * J0[2], G01 = J0[0] * J1[0] + J0[1] * J1[1] + J0[2] * J1[2],
               G11 = J1[0] * J1[0] + J1[1] * J1[1] + J1[2] * J1[2];
  const double det = G00 * G11 - G01 * G01, inv = 1.0 / det;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    K[i] = (G11 * J0[i] - G01 * J1[i]) * inv;
    K[3 + i] = (G00 * J1[i] - G01 * J0[i]) * inv;
  }
  return det;
}

// geometry of one cell per wavefront: geo[cell][7][npts]
__global__ __launch_bounds__(64 * EK_WPB) void k_ek_geom(int nc, int g, int nq, const EkTab* __restrict__ tab,
                                                         const double* __restrict__ nodes, double* __restrict__ geo,
                                                         int32_t* __restrict__ bad) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cell = blockIdx.x * EK_WPB + wave;
  if (cell >= nc) return;
  const int g1 = g + 1, npts = nq * nq;
  const double* X = nodes + (size_t)cell * g1 * g1 * 3;
  double* o = geo + (size_t)cell * 7 * npts;
  for (int pt = lane; pt < npts; pt += 64) {
    const int qy = pt / nq, qx = pt - qy * nq;
    double K[6];
    const double det = ek_pinv(X, g1, tab->qBg + qy * 4, tab->qDg + qy * 4, tab->qBg + qx * 4, tab->qDg + qx * 4, K);
    if (!(det > 0.0) || !isfinite(det)) *bad = 1;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k * npts + pt] = K[k];
    o[6 * npts + pt] = tab->w[qy] * tab->w[qx] * sqrt(det);
  }
}

// the iterate-independent element values of one cell per wavefront: stash[cell * EK_CW + (a * 3 + i) * 9 + b] = (grad_G N2_b . e_i, N1_a),
// stash[cell * EK_CW + 108 + a] = f (1, N1_a)
__global__ __launch_bounds__(64 * EK_WPB) void k_ek_const(int nc, int nq, const EkTab* __restrict__ tab, const double* __restrict__ geo,
                                                          double f, double* __restrict__ stash) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cell = blockIdx.x * EK_WPB + wave;
  if (cell >= nc) return;
  const int npts = nq * nq;
  const double* gc = geo + (size_t)cell * 7 * npts;
  for (int e = lane; e < EK_CW; e += 64) {
    double acc = 0.0;
    if (e < 108) {
      const int a = e / 27, i = (e - a * 27) / 9, b = e - a * 27 - i * 9;
      const int ay = a >> 1, ax = a & 1, by = b / 3, bx = b - by * 3;
      for (int qy = 0; qy < nq; ++qy)
        for (int qx = 0; qx < nq; ++qx) {
          const int pt = qy * nq + qx;
          const double N1 = tab->qB1[qy * 4 + ay] * tab->qB1[qx * 4 + ax];
          const double d0 = tab->qB2[qy * 4 + by] * tab->qD2[qx * 4 + bx], d1 = tab->qD2[qy * 4 + by] * tab->qB2[qx * 4 + bx];
          acc = fma(gc[6 * npts + pt] * N1, d0 * gc[i * npts + pt] + d1 * gc[(3 + i) * npts + pt], acc);
        }
    } else {
      const int a = e - 108, ay = a >> 1, ax = a & 1;
      for (int qy = 0; qy < nq; ++qy)
        for (int qx = 0; qx < nq; ++qx) acc = fma(gc[6 * npts + qy * nq + qx], tab->qB1[qy * 4 + ay] * tab->qB1[qx * 4 + ax], acc);
      acc *= f;
    }
    stash[(size_t)cell * EK_CW + e] = acc;
  }
}

// F = Jc y + alpha [fv; 0], y = [u; psi - psi_prev]: the linear part of the residual (:52-54, :57), one thread per row, ascending columns
__global__ __launch_bounds__(256) void k_ek_lin(int64_t ntot, int n1, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                const double* __restrict__ Jc, const double* __restrict__ fv, double alpha,
                                                const double* __restrict__ x, const double* __restrict__ xk, double* __restrict__ F) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= ntot) return;
  double s = 0.0;
  for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const int32_t c = col[k];
    s = fma(Jc[k], c < n1 ? x[c] : x[c] - xk[c], s);
  }
  F[r] = r < n1 ? s + alpha * fv[r] : s;
}

// phi (psi / s, tau) of one cell per wavefront: stash[cell * 27 + i * 9 + b]
__global__ __launch_bounds__(64 * EK_WPB) void k_ek_resid(int nc, int nq, int n1, int n2, const EkTab* __restrict__ tab,
                                                          const int32_t* __restrict__ cd2, const double* __restrict__ geo,
                                                          const double* __restrict__ x, double phi, double* __restrict__ stash) {
  __shared__ double sB[EK_MAXQ * 4];
  __shared__ double sP[EK_WPB][3][EK_NB2];
  __shared__ double sF[EK_WPB][3][EK_MAXPTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < nq * 4; i += 64 * EK_WPB) sB[i] = tab->qB2[i];
  const int cell = blockIdx.x * EK_WPB + wave;
  const bool active = cell < nc;
  if (active && lane < 3 * EK_NB2) {
    const int i = lane / EK_NB2, b = lane - i * EK_NB2;
    sP[wave][i][b] = x[(size_t)n1 + (size_t)i * n2 + cd2[(size_t)cell * EK_NB2 + b]];
  }
  __syncthreads();
  const int npts = nq * nq;
  if (active) {
    const double* wd = geo + ((size_t)cell * 7 + 6) * npts;
    for (int pt = lane; pt < npts; pt += 64) {
      const int qy = pt / nq, qx = pt - qy * nq;
      double v[3] = {0, 0, 0};
#pragma unroll
      for (int by = 0; by < 3; ++by)
#pragma unroll
        for (int bx = 0; bx < 3; ++bx) {
          const double bb = sB[qy * 4 + by] * sB[qx * 4 + bx];
#pragma unroll
          for (int i = 0; i < 3; ++i) v[i] = fma(bb, sP[wave][i][by * 3 + bx], v[i]);
        }
      const double c = wd[pt] * phi / sqrt(1.0 + v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) sF[wave][i][pt] = c * v[i];
    }
  }
  __syncthreads();
  if (active && lane < 3 * EK_NB2) {
    const int i = lane / EK_NB2, b = lane - i * EK_NB2, by = b / 3, bx = b - by * 3;
    double R = 0.0;
    for (int qy = 0; qy < nq; ++qy) {
      const double ya = sB[qy * 4 + by];
      for (int qx = 0; qx < nq; ++qx) R = fma(ya * sB[qx * 4 + bx], sF[wave][i][qy * nq + qx], R);
    }
    stash[(size_t)cell * 27 + lane] = R;
  }
}

// the six weighted mass blocks of D(psi) of one cell per wavefront: stash[cell * 6 * 81 + blk * 81 + a * 9 + b],
// blk = (0,0), (0,1), (0,2), (1,1), (1,2), (2,2)
__global__ __launch_bounds__(64 * EK_WPB) void k_ek_jac(int nc, int nq, int n1, int n2, const EkTab* __restrict__ tab,
                                                        const int32_t* __restrict__ cd2, const double* __restrict__ geo,
                                                        const double* __restrict__ x, double phi, double* __restrict__ stash) {
  constexpr int NB = EK_NB2, NPAIR = NB * (NB + 1) / 2;  // 45
  __shared__ double sB[EK_MAXQ * 4], sBB[EK_MAXQ * 16];  // sBB[q * 16 + i * 4 + j] = B[q][i] B[q][j]
  __shared__ double sP[EK_WPB][3][EK_NB2];
  __shared__ double sC[EK_WPB][6][EK_MAXPTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < nq * 4; i += 64 * EK_WPB) sB[i] = tab->qB2[i];
  for (int i = tid; i < nq * 16; i += 64 * EK_WPB) sBB[i] = tab->qB2[(i >> 4) * 4 + ((i >> 2) & 3)] * tab->qB2[(i >> 4) * 4 + (i & 3)];
  const int cell = blockIdx.x * EK_WPB + wave;
  const bool active = cell < nc;
  if (active && lane < 3 * NB) {
    const int i = lane / NB, b = lane - i * NB;
    sP[wave][i][b] = x[(size_t)n1 + (size_t)i * n2 + cd2[(size_t)cell * NB + b]];
  }
  __syncthreads();
  const int npts = nq * nq;
  if (active) {
    const double* wd = geo + ((size_t)cell * 7 + 6) * npts;
    for (int pt = lane; pt < npts; pt += 64) {
      const int qy = pt / nq, qx = pt - qy * nq;
      double v[3] = {0, 0, 0};
#pragma unroll
      for (int by = 0; by < 3; ++by)
#pragma unroll
        for (int bx = 0; bx < 3; ++bx) {
          const double bb = sB[qy * 4 + by] * sB[qx * 4 + bx];
#pragma unroll
          for (int i = 0; i < 3; ++i) v[i] = fma(bb, sP[wave][i][by * 3 + bx], v[i]);
        }
      const double s2 = 1.0 + v[0] * v[0] + v[1] * v[1] + v[2] * v[2], s = sqrt(s2);
      const double c1 = wd[pt] * phi / s, c3 = c1 / s2;  // phi w dS / s and / s^3
      sC[wave][0][pt] = c1 - c3 * v[0] * v[0];
      sC[wave][1][pt] = -c3 * v[0] * v[1];
      sC[wave][2][pt] = -c3 * v[0] * v[2];
      sC[wave][3][pt] = c1 - c3 * v[1] * v[1];
      sC[wave][4][pt] = -c3 * v[1] * v[2];
      sC[wave][5][pt] = c1 - c3 * v[2] * v[2];
    }
  }
  __syncthreads();
  if (active && lane < NPAIR) {
    int a = 0, b = lane;  // pair `lane` of the upper triangle, row by row: a <= b
    while (b >= NB - a) b -= NB - a, ++a;
    b += a;
    const int ay = a / 3, ax = a - ay * 3, by = b / 3, bx = b - by * 3;
    const int iyy = ay * 4 + by, ixx = ax * 4 + bx;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int qy = 0; qy < nq; ++qy) {
      const double yy = sBB[qy * 16 + iyy];
      for (int qx = 0; qx < nq; ++qx) {
        const double ww = yy * sBB[qx * 16 + ixx];
        const int pt = qy * nq + qx;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] = fma(ww, sC[wave][k][pt], acc[k]);
      }
    }
    double* o = stash + (size_t)cell * (6 * NB * NB);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      o[k * NB * NB + a * NB + b] = acc[k];
      o[k * NB * NB + b * NB + a] = acc[k];
    }
  }
}

// sum over cells and points of w dS (u - u0)^2 (:88-90): MX_RED blocks over the flat (cell, point) index, fixed-shape tree per block
__global__ __launch_bounds__(256) void k_ek_l2(int nc, int nq, const EkTab* __restrict__ tab, const int32_t* __restrict__ cd1,
                                               const double* __restrict__ geo, const double* __restrict__ x,
                                               const double* __restrict__ xk, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int npts = nq * nq;
  const int64_t total = (int64_t)nc * npts;
  double s = 0.0;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)MX_RED * 256) {
    const int cell = (int)(idx / npts), pt = (int)(idx - (int64_t)cell * npts), qy = pt / nq, qx = pt - qy * nq;
    double d = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int32_t dof = cd1[(size_t)cell * 4 + a];
      d = fma(tab->qB1[qy * 4 + (a >> 1)] * tab->qB1[qx * 4 + (a & 1)], x[dof] - xk[dof], d);
    }
    s = fma(geo[((size_t)cell * 7 + 6) * npts + pt], d * d, s);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// u, grad_G u and psi at the Q_g interpolation nodes of every cell (:84-86, :134-148): out[(cell * (g+1)^2 + node) * 7 + ..]
__global__ __launch_bounds__(256) void k_ek_eval(int nc, int g, int n1, int n2, const EkTab* __restrict__ tab, const double* __restrict__ nodes,
                                                 const int32_t* __restrict__ cd1, const int32_t* __restrict__ cd2,
                                                 const double* __restrict__ x, double* __restrict__ out) {
  const int g1 = g + 1, ng = g1 * g1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)nc * ng) return;
  const int cell = (int)(idx / ng), nd = (int)(idx - (int64_t)cell * ng), jy = nd / g1, jx = nd - jy * g1;
  double K[6];
  ek_pinv(nodes + (size_t)cell * ng * 3, g1, tab->nBg + jy * 4, tab->nDg + jy * 4, tab->nBg + jx * 4, tab->nDg + jx * 4, K);
  double u = 0.0, u0 = 0.0, u1 = 0.0;  // value and reference gradient
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double ua = x[cd1[(size_t)cell * 4 + a]];
    const int ay = a >> 1, ax = a & 1;
    u = fma(tab->nB1[jy * 4 + ay] * tab->nB1[jx * 4 + ax], ua, u);
    u0 = fma(tab->nB1[jy * 4 + ay] * tab->nD1[jx * 4 + ax], ua, u0);
    u1 = fma(tab->nD1[jy * 4 + ay] * tab->nB1[jx * 4 + ax], ua, u1);
  }
  double* o = out + idx * 7;
  o[0] = u;
#pragma unroll
  for (int i = 0; i < 3; ++i) o[1 + i] = u0 * K[i] + u1 * K[3 + i];
  double p[3] = {0, 0, 0};
  for (int b = 0; b < EK_NB2; ++b) {
    const int by = b / 3, bx = b - by * 3;
    const double N = tab->nB2[jy * 4 + by] * tab->nB2[jx * 4 + bx];
    const int32_t dof = cd2[(size_t)cell * EK_NB2 + b];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = fma(N, x[(size_t)n1 + (size_t)i * n2 + dof], p[i]);
  }
  o[4] = p[0], o[5] = p[1], o[6] = p[2];
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_ek_destroy(pgx_ek_handle* h) { mx_destroy(h); }

void pgx_ek_handle::residual_dev(const double* xin, double* Fout) {
  pgx_ek_handle* h = this;
  MxTimer t(h, 0);
  hipLaunchKernelGGL(k_ek_lin, dim3((unsigned)((h->ntot + 255) / 256)), dim3(256), 0, h->st, h->ntot, n1, h->rowptr, h->col, Jc, fv, h->alpha,
                     xin, h->xk, Fout);
  hipLaunchKernelGGL(k_ek_resid, dim3((nc + EK_WPB - 1) / EK_WPB), dim3(64 * EK_WPB), 0, h->st, nc, nq, n1, n2, tab, cd2, geo, xin, phi, stash);
  pgx_scatter_run(h->st, sc_res, stash, 1.0, 1, Fout);
}
void pgx_ek_handle::jacobian_dev(const double* xin) {
  pgx_ek_handle* h = this;
  MxTimer t(h, 1);
  hipMemcpyAsync(h->Jv, Jc, sizeof(double) * h->nnz, hipMemcpyDeviceToDevice, h->st);
  hipLaunchKernelGGL(k_ek_jac, dim3((nc + EK_WPB - 1) / EK_WPB), dim3(64 * EK_WPB), 0, h->st, nc, nq, n1, n2, tab, cd2, geo, xin, phi, stash);
  pgx_scatter_run(h->st, sc_jac, stash, 1.0, 1, h->Jv);
  pgx_scatter_run(h->st, sc_jac_t, stash, 1.0, 1, h->Jv);
  h->jac_valid = true;
}

// values and derivatives of the 1-D Lagrange basis on the nodes i / k at t, from the linear factors (k t - a) / (i - a)
static void ek_lagrange(int k, double t, double* val4, double* der4) {
  for (int i = 0; i < 4; ++i) val4[i] = der4[i] = 0.0;
  for (int i = 0; i <= k; ++i) {
    double val = 1.0, der = 0.0;
    for (int a = 0; a <= k; ++a) {
      if (a == i) continue;
      const double fac = (k * t - a) / (i - a);
      der = der * fac + val * ((double)k / (i - a));
      val *= fac;
    }
    val4[i] = val, der4[i] = der;
  }
}

// banded: the band LU of include/pgx_bd.h in the symmetric ordering perm (NULL: as numbered) stands where the dense LU does
static int ek_create_impl(pgx_ek_handle* h, const pgx_ek_problem* pr, bool banded, const int32_t* perm) {
  const int nc = pr->nc, g = pr->geo_order, g1 = g + 1, ng = g1 * g1, nq = pr->nq, npts = nq * nq, n1 = pr->n1, n2 = pr->n2;
  const int64_t ntot = (int64_t)n1 + 3 * (int64_t)n2;
  if (!banded && ntot > PGX_DN_MAX_N) {
    h->err = "pgx_ek_create: " + std::to_string(ntot) + " unknowns exceed the dense LU's limit of " + std::to_string(PGX_DN_MAX_N);
    return PGX_EINVAL;
  }
  h->nc = nc, h->g = g, h->nq = nq, h->n1 = n1, h->n2 = n2, h->ntot = ntot, h->f = pr->f, h->phi = pr->phi;
  const int nloc[2] = {4, EK_NB2}, ndof[2] = {n1, n2};
  const int32_t* cd[2] = {pr->cell_dofs_u, pr->cell_dofs_p};
  for (int s = 0; s < 2; ++s)
    for (int c = 0; c < nc; ++c) {
      const int32_t* d = cd[s] + (size_t)c * nloc[s];
      for (int a = 0; a < nloc[s]; ++a) {
        if (d[a] < 0 || d[a] >= ndof[s]) {
          h->err = "pgx_ek_create: cell dof out of range";
          return PGX_EINVAL;
        }
        for (int b = 0; b < a; ++b)
          if (d[a] == d[b]) {
            h->err = "pgx_ek_create: cell " + std::to_string(c) + " holds one dof twice (a cell meets itself: at least 3 cells around the strip)";
            return PGX_EINVAL;
          }
      }
    }
  for (size_t i = 0; i < (size_t)nc * ng * 3; ++i)
    if (!std::isfinite(pr->cell_nodes[i])) {
      h->err = "pgx_ek_create: geometry node not finite";
      return PGX_EINVAL;
    }
  {  // two cells share at most one edge: two vertices
    std::vector<std::vector<int32_t>> v2c(n1);
    for (int c = 0; c < nc; ++c)
      for (int a = 0; a < 4; ++a) v2c[cd[0][(size_t)c * 4 + a]].push_back(c);
    for (int c = 0; c < nc; ++c) {
      std::map<int32_t, int> shared;
      for (int a = 0; a < 4; ++a)
        for (int32_t o : v2c[cd[0][(size_t)c * 4 + a]])
          if (o != c && ++shared[o] > 2) {
            h->err = "pgx_ek_create: cells " + std::to_string(c) + " and " + std::to_string(o) +
                     " share more than one edge (a cell meets one neighbour twice: at least 3 cells around the strip)";
            return PGX_EINVAL;
          }
    }
  }
  EkTab T;
  memset(&T, 0, sizeof T);
  for (int q = 0; q < nq; ++q) {
    const double t = pr->qpts[q];
    if (!std::isfinite(t) || !std::isfinite(pr->qwts[q])) {
      h->err = "pgx_ek_create: quadrature rule not finite";
      return PGX_EINVAL;
    }
    T.w[q] = pr->qwts[q];
    ek_lagrange(1, t, T.qB1 + q * 4, T.qD1 + q * 4);
    ek_lagrange(2, t, T.qB2 + q * 4, T.qD2 + q * 4);
    ek_lagrange(g, t, T.qBg + q * 4, T.qDg + q * 4);
  }
  for (int j = 0; j < g1; ++j) {
    const double t = (double)j / g;
    double dummy[4];
    ek_lagrange(1, t, T.nB1 + j * 4, T.nD1 + j * 4);
    ek_lagrange(2, t, T.nB2 + j * 4, dummy);
    ek_lagrange(g, t, T.nBg + j * 4, T.nDg + j * 4);
  }
  // adjacency of the space pairs through the cells
  std::vector<std::vector<int32_t>> adj[2][2];
  for (int R = 0; R < 2; ++R)
    for (int Cc = 0; Cc < 2; ++Cc) {
      auto& A = adj[R][Cc];
      A.assign(ndof[R], {});
      for (int c = 0; c < nc; ++c)
        for (int a = 0; a < nloc[R]; ++a) {
          auto& row = A[cd[R][(size_t)c * nloc[R] + a]];
          row.insert(row.end(), cd[Cc] + (size_t)c * nloc[Cc], cd[Cc] + (size_t)(c + 1) * nloc[Cc]);
        }
      for (auto& row : A) {
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
      }
    }
  const int64_t off[5] = {0, n1, n1 + (int64_t)n2, n1 + 2 * (int64_t)n2, ntot};
  auto sp_of = [](int blk) { return blk == 0 ? 0 : 1; };
  auto blen = [&](int rb, int cb, int i) -> int64_t { return rb == 0 && cb == 0 ? 0 : (int64_t)adj[sp_of(rb)][sp_of(cb)][i].size(); };
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  int64_t tot = 0;
  for (int rb = 0; rb < 4; ++rb)
    for (int i = 0; i < ndof[sp_of(rb)]; ++i) {
      for (int cb = 0; cb < 4; ++cb) tot += blen(rb, cb, i);
      if (tot > 0x7fffffff) {
        h->err = "pgx_ek_create: mixed matrix exceeds int32 nnz";
        return PGX_EINVAL;
      }
      rowptr[off[rb] + i + 1] = (int32_t)tot;
    }
  h->nnz = tot;
  col.resize(tot);
  for (int rb = 0; rb < 4; ++rb)
    for (int i = 0; i < ndof[sp_of(rb)]; ++i) {
      int64_t e = rowptr[off[rb] + i];
      for (int cb = 0; cb < 4; ++cb) {
        if (rb == 0 && cb == 0) continue;
        for (int32_t j : adj[sp_of(rb)][sp_of(cb)][i]) col[e++] = (int32_t)(off[cb] + j);
      }
    }
  auto find = [&](int rb, int32_t i, int cb, int32_t j) -> int32_t {
    int64_t e = rowptr[off[rb] + i];
    for (int c2 = 0; c2 < cb; ++c2) e += blen(rb, c2, i);
    const auto& row = adj[sp_of(rb)][sp_of(cb)][i];
    return (int32_t)(e + (std::lower_bound(row.begin(), row.end(), j) - row.begin()));
  };
  // destination tables, cell-major like the stashes; -1 drops an entry
  const size_t Wj = 6 * 81, Wr = 27;
  std::vector<int32_t> dr((size_t)nc * Wr), dj((size_t)nc * Wj), djt((size_t)nc * Wj, -1);
  std::vector<int32_t> dB((size_t)nc * EK_CW, -1), dBt((size_t)nc * EK_CW, -1), dfv((size_t)nc * EK_CW, -1);
  const int br[6] = {1, 1, 1, 2, 2, 3}, bc[6] = {1, 2, 3, 2, 3, 3};
  for (int c = 0; c < nc; ++c) {
    const int32_t* du = cd[0] + (size_t)c * 4;
    const int32_t* dp = cd[1] + (size_t)c * EK_NB2;
    for (int i = 0; i < 3; ++i)
      for (int b = 0; b < EK_NB2; ++b) dr[(size_t)c * Wr + i * EK_NB2 + b] = (int32_t)(off[1 + i] + dp[b]);
    for (int k = 0; k < 6; ++k)
      for (int a = 0; a < EK_NB2; ++a)
        for (int b = 0; b < EK_NB2; ++b) {
          const size_t o = (size_t)c * Wj + (size_t)k * 81 + a * EK_NB2 + b;
          dj[o] = find(br[k], dp[a], bc[k], dp[b]);
          if (br[k] != bc[k]) djt[o] = find(bc[k], dp[a], br[k], dp[b]);  // the transposed block takes the same (symmetric) values
        }
    for (int a = 0; a < 4; ++a) {
      for (int i = 0; i < 3; ++i)
        for (int b = 0; b < EK_NB2; ++b) {
          const size_t o = (size_t)c * EK_CW + (a * 3 + i) * EK_NB2 + b;
          dB[o] = find(0, du[a], 1 + i, dp[b]);
          dBt[o] = find(1 + i, dp[b], 0, du[a]);
        }
      dfv[(size_t)c * EK_CW + 108 + a] = du[a];
    }
  }
  MXHIP(hipStreamCreate(&h->st));
  int rc = banded ? pgx_bd_create(ntot, rowptr.data(), col.data(), perm, h->device, (void*)h->st, &h->bd)
                  : pgx_dn_create(ntot, rowptr.data(), col.data(), h->device, (void*)h->st, &h->dn);
  if (rc) {
    h->err = std::string("direct solver: ") + (banded ? pgx_bd_last_error(nullptr) : pgx_dn_last_error(nullptr));
    h->dn = nullptr, h->bd = nullptr;
    return rc;
  }
  MXALLOC(h->tab, 1);
  MXALLOC(h->nodes, (size_t)nc * ng * 3);
  MXALLOC(h->cd1, (size_t)nc * 4);
  MXALLOC(h->cd2, (size_t)nc * EK_NB2);
  MXALLOC(h->geo, (size_t)nc * 7 * npts);
  MXALLOC(h->bad, 1);
  MXALLOC(h->fv, n1);
  MXALLOC(h->stash, (size_t)nc * std::max<size_t>(Wj, EK_CW));
  MXALLOC(h->d_cells, (size_t)nc * ng * 7);
  MXALLOC(h->rowptr, ntot + 1);
  MXALLOC(h->col, tot);
  MXALLOC(h->Jc, tot);
  MXALLOC(h->Jv, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  MXHIP(hipMemcpy(h->tab, &T, sizeof T, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->nodes, pr->cell_nodes, sizeof(double) * (size_t)nc * ng * 3, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->cd1, cd[0], sizeof(int32_t) * (size_t)nc * 4, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->cd2, cd[1], sizeof(int32_t) * (size_t)nc * EK_NB2, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->rowptr, rowptr.data(), sizeof(int32_t) * (ntot + 1), hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->col, col.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->bad, 0, sizeof(int32_t), h->st));
  MXHIP(hipMemsetAsync(h->Jv, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->fv, 0, sizeof(double) * n1, h->st));
  std::string e1 = pgx_scatter_build(dr.data(), (int64_t)nc * Wr, ntot, h->allocs, &h->sc_res);
  if (e1.empty()) e1 = pgx_scatter_build(dj.data(), (int64_t)nc * Wj, tot, h->allocs, &h->sc_jac);
  if (e1.empty()) e1 = pgx_scatter_build(djt.data(), (int64_t)nc * Wj, tot, h->allocs, &h->sc_jac_t);
  if (e1.empty()) e1 = pgx_scatter_build(dB.data(), (int64_t)nc * EK_CW, tot, h->allocs, &h->sc_B);
  if (e1.empty()) e1 = pgx_scatter_build(dBt.data(), (int64_t)nc * EK_CW, tot, h->allocs, &h->sc_Bt);
  if (e1.empty()) e1 = pgx_scatter_build(dfv.data(), (int64_t)nc * EK_CW, n1, h->allocs, &h->sc_fv);
  if (!e1.empty()) {
    h->err = e1;
    return PGX_ENOMEM;
  }
  // geometry and the iterate-independent part, once
  const dim3 grid((nc + EK_WPB - 1) / EK_WPB), block(64 * EK_WPB);
  hipLaunchKernelGGL(k_ek_geom, grid, block, 0, h->st, nc, g, nq, h->tab, h->nodes, h->geo, h->bad);
  hipLaunchKernelGGL(k_ek_const, grid, block, 0, h->st, nc, nq, h->tab, h->geo, h->f, h->stash);
  pgx_scatter_run(h->st, h->sc_B, h->stash, 1.0, 0, h->Jc);
  pgx_scatter_run(h->st, h->sc_Bt, h->stash, 1.0, 0, h->Jc);
  pgx_scatter_run(h->st, h->sc_fv, h->stash, 1.0, 0, h->fv);
  int32_t bad = 0;
  MXHIP(hipMemcpyAsync(&bad, h->bad, sizeof bad, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  MXHIP(hipGetLastError());
  if (bad) {
    h->err = "pgx_ek_create: degenerate cell (det J^T J is not positive and finite at a quadrature point)";
    return PGX_EINVAL;
  }
  return PGX_OK;
}

static int ek_create(const char* fn, const pgx_ek_problem* p, bool banded, const int32_t* perm, int device, pgx_ek_handle** out) {
  if (!p || !out || p->nc < 1 || p->geo_order < 1 || p->geo_order > 3 || !p->cell_nodes || p->n1 < 1 || p->n2 < 1 || !p->cell_dofs_u ||
      !p->cell_dofs_p || p->nq < 1 || p->nq > EK_MAXQ || !p->qpts || !p->qwts || !std::isfinite(p->f) || !std::isfinite(p->phi)) {
    g_ek_error = std::string(fn) + ": bad arguments (geometry order 1..3 with its nodes, both numberings, a 1-D rule of 1..11 points, finite f and phi)";
    return PGX_EINVAL;
  }
  return mx_create(fn, g_ek_error, device, out, [&](pgx_ek_handle* h) { return ek_create_impl(h, p, banded, perm); });
}
extern "C" int pgx_ek_create(const pgx_ek_problem* p, int device, pgx_ek_handle** out) {
  return ek_create("pgx_ek_create", p, false, nullptr, device, out);
}
extern "C" int pgx_ek_create_banded(const pgx_ek_problem* p, const int32_t* perm, int device, pgx_ek_handle** out) {
  return ek_create("pgx_ek_create_banded", p, true, perm, device, out);
}

extern "C" int pgx_ek_num_dofs(const pgx_ek_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_ek_set_state(pgx_ek_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_ek_get_state(pgx_ek_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_ek_set_prev(pgx_ek_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_ek_get_prev(pgx_ek_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_ek_advance_prev(pgx_ek_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_ek_set_alpha(pgx_ek_handle* h, double a) { return mx_set_alpha(h, a); }
extern "C" int pgx_ek_residual(pgx_ek_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_ek_jacobian_fill(pgx_ek_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_ek_csr_export(pgx_ek_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_ek_spmv(pgx_ek_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
// linesearch 2: l2 (the script's, :67), 1 / 3: bt of order 2 / 3, every other value: plain Newton
extern "C" int pgx_ek_newton_solve(pgx_ek_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its) {
  return mx_newton(h, opts, reason, its, lin_its, true);
}
extern "C" int pgx_ek_profile(pgx_ek_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

extern "C" int pgx_ek_l2_increment_u(pgx_ek_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_ek_l2, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->nq, h->tab, h->cd1, h->geo, h->x, h->xk, h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_ek_eval_cells(pgx_ek_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  const int64_t cnt = (int64_t)h->nc * (h->g + 1) * (h->g + 1);
  hipLaunchKernelGGL(k_ek_eval, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->st, h->nc, h->g, h->n1, h->n2, h->tab, h->nodes, h->cd1,
                     h->cd2, h->x, h->d_cells);
  MXHIP(hipMemcpyAsync(out, h->d_cells, sizeof(double) * cnt * 7, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  MXHIP(hipGetLastError());
  return PGX_OK;
}
extern "C" int pgx_ek_lu_stats(const pgx_ek_handle* h, pgx_dn_stats* st) {
  if (!h || !st || (!h->dn && !h->bd)) return PGX_EINVAL;
  if (h->dn) return pgx_dn_get_stats(h->dn, st);
  pgx_bd_stats b;
  const int rc = pgx_bd_get_stats(h->bd, &b);
  if (rc) return rc;
  st->n = b.n, st->interchanges = b.interchanges, st->min_pivot = b.min_pivot, st->max_pivot = b.max_pivot, st->zero_pivots = b.zero_pivots;
  return PGX_OK;
}
extern "C" int pgx_ek_band_stats(const pgx_ek_handle* h, pgx_bd_stats* st) {
  if (!h || !st) return PGX_EINVAL;
  return h->bd ? pgx_bd_get_stats(h->bd, st) : PGX_ESTATE;  // a dense handle has no band
}
