// pgx_gc.hip - example 06 (gradient constraint, vector latent variable) behind the C ABI of include/pgx_gc.h.
//
// Reference: examples/06_gradient_constraints/gradient_constraint_dolfinx.py (:38-46 spaces, :53 degree-10 measure,
// :100-107 residual, :108-131 NonlinearProblem + SNES options, :171-205 outer loop).  u in P2, psi in (P1)^2,
// x = [u | psi_x | psi_y].  Newton matrix [[alpha K, G^T],[G, -N(psi)]] lives in ONE mixed CSR array whose pattern and
// per-cell destination tables are built once on the host; K and G are assembled once on the device, every Newton step
// only rescales the K slots and re-assembles the 36 N entries per cell.  Linear solves: pgx_nd (sparse LU) + iterative
// refinement on the exact operator.
#include <cstring>

#include "../../include/pgx_gc.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"

#define GC_MAXQ 40
struct GcQuad {
  double X[GC_MAXQ], Y[GC_MAXQ], w[GC_MAXQ];
  int nq;
};

static thread_local std::string g_gc_error;

struct pgx_gc_handle : MixedBase {
  int nv = 0, nc = 0, n2 = 0;
  GcQuad Q{};
  double *coords = nullptr, *phi = nullptr, *f = nullptr, *gbc = nullptr;
  int32_t* cdofs = nullptr;
  uint8_t* mask = nullptr;
  uint8_t* kind = nullptr;
  double* Jc = nullptr;  // constant part of the Jacobian values (K and G slots), assembled once
  // deterministic assembly (pgx_scatter.h): element kernels park [slot * nc + cell] in `stash`, one thread per destination sums
  PgxScatter sc_res, sc_N;  // residual: 12 slots per cell -> dofs; N(psi): 36 slots per cell -> CSR positions
  double* stash = nullptr;  // [36 * nc]  (general degree: [4 NP^2 * nc])
  // general primal degree k = 3..8 (pgx_gc_create_general): NU / NP local nodes of the primal P_k / latent P_(k-1) space, the latent
  // cell dofs, and the basis tables at the quadrature points; n2 = primal dofs, nv = latent dofs per component
  int gen = 0, NU = 6, NP = 3;
  int32_t *cdofs_p = nullptr, *cells3 = nullptr;  // latent cell dofs; vertex triples (affine geometry)
  double *tNu = nullptr, *tdNu = nullptr, *tNp = nullptr;
  void* ev = nullptr;  // pgx_gc_eval_cells: points / tables and the outputs, grown on demand
  size_t ev_len = 0;
  pgx_gc_handle() : MixedBase("pgx_gc") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

extern "C" const char* pgx_gc_last_error(const pgx_gc_handle* h) { return h ? h->err.c_str() : g_gc_error.c_str(); }

#define GCHIP MXHIP
#define GCALLOC MXALLOC
using GcTimer = MxTimer;

// ------------------------------------------------------------------------------------------------------------------
// element kernels (one thread per cell)
// ------------------------------------------------------------------------------------------------------------------
struct GcGeom {
  double inv[2][2];  // J^{-1}
  double adet;
};

__device__ inline GcGeom gc_geom(const double* __restrict__ coords, const int32_t* __restrict__ cd) {
  const double x0 = coords[2 * cd[0]], y0 = coords[2 * cd[0] + 1];
  const double j00 = coords[2 * cd[1]] - x0, j10 = coords[2 * cd[1] + 1] - y0;
  const double j01 = coords[2 * cd[2]] - x0, j11 = coords[2 * cd[2] + 1] - y0;
  const double det = j00 * j11 - j01 * j10;
  GcGeom g;
  g.inv[0][0] = j11 / det;
  g.inv[0][1] = -j01 / det;
  g.inv[1][0] = -j10 / det;
  g.inv[1][1] = j00 / det;
  g.adet = fabs(det);
  return g;
}

// P1 values l[3], P2 values N[6] and PHYSICAL P2 gradients G[6][2] at reference point (X,Y); edge i opposite vertex i
__device__ inline void gc_tab(double X, double Y, const GcGeom& g, double l[3], double N[6], double G[6][2]) {
  l[0] = 1.0 - X - Y;
  l[1] = X;
  l[2] = Y;
  const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
  double dN[6][2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    N[i] = l[i] * (2.0 * l[i] - 1.0);
    dN[i][0] = (4.0 * l[i] - 1.0) * dl[i][0];
    dN[i][1] = (4.0 * l[i] - 1.0) * dl[i][1];
  }
  const int ej[3] = {1, 0, 0}, ek[3] = {2, 2, 1};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    N[3 + i] = 4.0 * l[ej[i]] * l[ek[i]];
    dN[3 + i][0] = 4.0 * (l[ej[i]] * dl[ek[i]][0] + l[ek[i]] * dl[ej[i]][0]);
    dN[3 + i][1] = 4.0 * (l[ej[i]] * dl[ek[i]][1] + l[ek[i]] * dl[ej[i]][1]);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    G[a][0] = dN[a][0] * g.inv[0][0] + dN[a][1] * g.inv[1][0];
    G[a][1] = dN[a][0] * g.inv[0][1] + dN[a][1] * g.inv[1][1];
  }
}

__global__ __launch_bounds__(128) void k_gc_residual(int nc, int n2, int nv, const int32_t* __restrict__ cdofs,
                                                     const double* __restrict__ coords, const uint8_t* __restrict__ mask,
                                                     const double* __restrict__ gbc, const double* __restrict__ phi,
                                                     const double* __restrict__ f, const double* __restrict__ x,
                                                     const double* __restrict__ xk, double alpha, GcQuad Q,
                                                     double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cd = cdofs + 6 * (size_t)c;
  const GcGeom g = gc_geom(coords, cd);
  double u[6], ph[6], ff[6], px[3], py[3], dx0[3], dy0[3];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const int d = cd[a];
    u[a] = mask[d] ? gbc[d] : x[d];
    ph[a] = phi[d];
    ff[a] = f[d];
  }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int v = cd[b];
    px[b] = x[n2 + v];
    py[b] = x[n2 + nv + v];
    dx0[b] = px[b] - xk[n2 + v];
    dy0[b] = py[b] - xk[n2 + nv + v];
  }
  double Ru[6] = {0, 0, 0, 0, 0, 0}, Rx[3] = {0, 0, 0}, Ry[3] = {0, 0, 0};
  for (int q = 0; q < Q.nq; ++q) {
    double l[3], N[6], G[6][2];
    gc_tab(Q.X[q], Q.Y[q], g, l, N, G);
    const double wd = Q.w[q] * g.adet;
    double gux = 0, guy = 0, phq = 0, fq = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      gux += u[a] * G[a][0];
      guy += u[a] * G[a][1];
      phq += ph[a] * N[a];
      fq += ff[a] * N[a];
    }
    const double pxq = px[0] * l[0] + px[1] * l[1] + px[2] * l[2];
    const double pyq = py[0] * l[0] + py[1] * l[1] + py[2] * l[2];
    const double dxq = dx0[0] * l[0] + dx0[1] * l[1] + dx0[2] * l[2];
    const double dyq = dy0[0] * l[0] + dy0[1] * l[1] + dy0[2] * l[2];
    const double s = sqrt(1.0 + pxq * pxq + pyq * pyq);
    const double vx = alpha * gux + dxq, vy = alpha * guy + dyq;
#pragma unroll
    for (int a = 0; a < 6; ++a) Ru[a] += wd * (vx * G[a][0] + vy * G[a][1] - alpha * fq * N[a]);
    const double rx = gux - phq * pxq / s, ry = guy - phq * pyq / s;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Rx[b] += wd * l[b] * rx;
      Ry[b] += wd * l[b] * ry;
    }
  }
  // parked slot-major (coalesced across the cells of a wave); pgx_scatter sums them per dof in a fixed order
#pragma unroll
  for (int a = 0; a < 6; ++a) stash[(size_t)a * nc + c] = Ru[a];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    stash[(size_t)(6 + b) * nc + c] = Rx[b];
    stash[(size_t)(9 + b) * nc + c] = Ry[b];
  }
}

__global__ void k_gc_resid_bc(int n2, const uint8_t* __restrict__ mask, const double* __restrict__ gbc,
                              const double* __restrict__ x, double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n2 && mask[i]) F[i] = x[i] - gbc[i];
}

// constant part, once: K (36 entries) and G, G^T (36 + 36) per cell, parked in a [108 * nc] stash
__global__ __launch_bounds__(128) void k_gc_const(int nc, const int32_t* __restrict__ cdofs, const double* __restrict__ coords,
                                                  GcQuad Q, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cd = cdofs + 6 * (size_t)c;
  const GcGeom g = gc_geom(coords, cd);
  double Ke[6][6], Ge[3][2][6];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) Ke[a][b] = 0.0;
  for (int b = 0; b < 3; ++b)
    for (int d = 0; d < 2; ++d)
      for (int a = 0; a < 6; ++a) Ge[b][d][a] = 0.0;
  for (int q = 0; q < Q.nq; ++q) {
    double l[3], N[6], G[6][2];
    gc_tab(Q.X[q], Q.Y[q], g, l, N, G);
    const double wd = Q.w[q] * g.adet;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) Ke[a][b] += wd * (G[a][0] * G[b][0] + G[a][1] * G[b][1]);
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        Ge[b][0][a] += wd * l[b] * G[a][0];
        Ge[b][1][a] += wd * l[b] * G[a][1];
      }
    }
  }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) stash[(size_t)(a * 6 + b) * nc + c] = Ke[a][b];
  for (int b = 0; b < 3; ++b)
    for (int d = 0; d < 2; ++d)
      for (int a = 0; a < 6; ++a) {
        const int e = 36 + ((b * 2 + d) * 6 + a) * 2;
        stash[(size_t)e * nc + c] = Ge[b][d][a];
        stash[(size_t)(e + 1) * nc + c] = Ge[b][d][a];
      }
}

// kind: 0 = K slot (scaled by alpha), 1 = G / G^T slot, 2 = N slot (accumulated by k_gc_jac_N), 3 = BC diagonal, 4 = zeroed by BCs
__global__ void k_gc_jac_init(int64_t nnz, const uint8_t* __restrict__ kind, const double* __restrict__ Jc, double alpha,
                              double* __restrict__ Jv) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int t = kind[k];
  Jv[k] = t == 0 ? alpha * Jc[k] : t == 1 ? Jc[k] : t == 3 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(128) void k_gc_jac_N(int nc, int n2, int nv, const int32_t* __restrict__ cdofs,
                                                  const double* __restrict__ coords, const double* __restrict__ phi,
                                                  const double* __restrict__ x, GcQuad Q, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cd = cdofs + 6 * (size_t)c;
  const GcGeom g = gc_geom(coords, cd);
  double ph[6], px[3], py[3];
#pragma unroll
  for (int a = 0; a < 6; ++a) ph[a] = phi[cd[a]];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    px[b] = x[n2 + cd[b]];
    py[b] = x[n2 + nv + cd[b]];
  }
  double Nxx[3][3], Nxy[3][3], Nyy[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Nxx[a][b] = Nxy[a][b] = Nyy[a][b] = 0.0;
  for (int q = 0; q < Q.nq; ++q) {
    double l[3], N[6], G[6][2];
    gc_tab(Q.X[q], Q.Y[q], g, l, N, G);
    double phq = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) phq += ph[a] * N[a];
    const double pxq = px[0] * l[0] + px[1] * l[1] + px[2] * l[2];
    const double pyq = py[0] * l[0] + py[1] * l[1] + py[2] * l[2];
    const double s = sqrt(1.0 + pxq * pxq + pyq * pyq);
    const double s3 = s * s * s;
    const double wp = Q.w[q] * g.adet * phq;
    const double cxx = wp * (1.0 / s - pxq * pxq / s3), cxy = wp * (-pxq * pyq / s3), cyy = wp * (1.0 / s - pyq * pyq / s3);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const double ll = l[a] * l[b];
        Nxx[a][b] += cxx * ll;
        Nxy[a][b] += cxy * ll;
        Nyy[a][b] += cyy * ll;
      }
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const int e = (a * 3 + b) * 4;  // (c,d) = xx, xy, yx, yy
      stash[(size_t)e * nc + c] = Nxx[a][b];
      stash[(size_t)(e + 1) * nc + c] = Nxy[a][b];
      stash[(size_t)(e + 2) * nc + c] = Nxy[a][b];
      stash[(size_t)(e + 3) * nc + c] = Nyy[a][b];
    }
}

#define GC_RED MX_RED
// int (u - uk)^2 with the problem's quadrature: per-block partial sums over cells
__global__ __launch_bounds__(256) void k_gc_l2(int nc, const int32_t* __restrict__ cdofs, const double* __restrict__ coords,
                                               const double* __restrict__ x, const double* __restrict__ xk, GcQuad Q,
                                               double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += GC_RED * 256) {
    const int32_t* cd = cdofs + 6 * (size_t)c;
    const GcGeom g = gc_geom(coords, cd);
    double d[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = x[cd[a]] - xk[cd[a]];
    for (int q = 0; q < Q.nq; ++q) {
      double l[3], N[6], G[6][2];
      gc_tab(Q.X[q], Q.Y[q], g, l, N, G);
      double v = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) v += d[a] * N[a];
      s += Q.w[q] * g.adet * v * v;
    }
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// ------------------------------------------------------------------------------------------------------------------
// general degree (primal P_k, latent (P_(k-1))^2, k <= 8): the same element integrals, TABLE-driven.  tNu [nq][NU] and tdNu
// [nq][NU][2] are the primal basis and its reference gradients at the quadrature points, tNp [nq][NP] the latent basis; cells are
// affine (geometry from the three vertices).  One thread per cell, runtime sizes, local arrays of the maximal size; slot-major
// stashes as above.  These kernels are not tuned: the factorisation dominates a Newton step by orders of magnitude.
// ------------------------------------------------------------------------------------------------------------------
// element sizes: triangles P8 / P7 have 45 / 36 local nodes, quadrilaterals Q8 / Q7 81 / 64 (pgx_gc.h: affine cells of either shape)
#define GCG_MAXU 81
#define GCG_MAXP 64
static_assert(GCG_MAXU + 2 * GCG_MAXP <= PAT_MAX_ENTITY_DOFS, "the mixed dofs of a cell must fit the pattern builder's buffer");
#define GCG_TRIU 45
#define GCG_TRIP 36
struct GcgArgs {
  int nc, n2, nv, NU, NP, nq;
  const int32_t *cells, *cdu, *cdp;
  const double *coords, *tNu, *tdNu, *tNp;
  double w[GC_MAXQ];
};

__device__ inline GcGeom gcg_geom(const GcgArgs& A, int c) { return gc_geom(A.coords, A.cells + 3 * (size_t)c); }

template <int MAXU, int MAXP>
__global__ __launch_bounds__(64) void k_gcg_residual(GcgArgs A, const uint8_t* __restrict__ mask, const double* __restrict__ gbc,
                                                     const double* __restrict__ phi, const double* __restrict__ f,
                                                     const double* __restrict__ x, const double* __restrict__ xk, double alpha,
                                                     double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nc) return;
  const int NU = A.NU, NP = A.NP, nc = A.nc;
  const GcGeom g = gcg_geom(A, c);
  const int32_t* cu = A.cdu + (size_t)NU * c;
  const int32_t* cp = A.cdp + (size_t)NP * c;
  double u[MAXU], ph[MAXU], ff[MAXU], Ru[MAXU], Gx[MAXU], Gy[MAXU];
  double px[MAXP], py[MAXP], dx0[MAXP], dy0[MAXP], Rx[MAXP], Ry[MAXP];
  for (int a = 0; a < NU; ++a) {
    const int d = cu[a];
    u[a] = mask[d] ? gbc[d] : x[d];
    ph[a] = phi[d];
    ff[a] = f[d];
    Ru[a] = 0.0;
  }
  for (int b = 0; b < NP; ++b) {
    const int v = cp[b];
    px[b] = x[A.n2 + v];
    py[b] = x[A.n2 + A.nv + v];
    dx0[b] = px[b] - xk[A.n2 + v];
    dy0[b] = py[b] - xk[A.n2 + A.nv + v];
    Rx[b] = Ry[b] = 0.0;
  }
  for (int q = 0; q < A.nq; ++q) {
    const double* Nu = A.tNu + (size_t)q * NU;
    const double* dN = A.tdNu + (size_t)q * NU * 2;
    const double* Np = A.tNp + (size_t)q * NP;
    const double wd = A.w[q] * g.adet;
    double gux = 0, guy = 0, phq = 0, fq = 0;
    for (int a = 0; a < NU; ++a) {
      Gx[a] = dN[2 * a] * g.inv[0][0] + dN[2 * a + 1] * g.inv[1][0];
      Gy[a] = dN[2 * a] * g.inv[0][1] + dN[2 * a + 1] * g.inv[1][1];
      gux += u[a] * Gx[a];
      guy += u[a] * Gy[a];
      phq += ph[a] * Nu[a];
      fq += ff[a] * Nu[a];
    }
    double pxq = 0, pyq = 0, dxq = 0, dyq = 0;
    for (int b = 0; b < NP; ++b) {
      pxq += px[b] * Np[b];
      pyq += py[b] * Np[b];
      dxq += dx0[b] * Np[b];
      dyq += dy0[b] * Np[b];
    }
    const double s = sqrt(1.0 + pxq * pxq + pyq * pyq);
    const double vx = alpha * gux + dxq, vy = alpha * guy + dyq;
    for (int a = 0; a < NU; ++a) Ru[a] += wd * (vx * Gx[a] + vy * Gy[a] - alpha * fq * Nu[a]);
    const double rx = gux - phq * pxq / s, ry = guy - phq * pyq / s;
    for (int b = 0; b < NP; ++b) {
      Rx[b] += wd * Np[b] * rx;
      Ry[b] += wd * Np[b] * ry;
    }
  }
  for (int a = 0; a < NU; ++a) stash[(size_t)a * nc + c] = Ru[a];
  for (int b = 0; b < NP; ++b) {
    stash[(size_t)(NU + b) * nc + c] = Rx[b];
    stash[(size_t)(NU + NP + b) * nc + c] = Ry[b];
  }
}

// constant part: K (NU^2 slots), then G and G^T: slot NU^2 + ((b*2 + d)*NU + a)*2 (+1)
__global__ __launch_bounds__(64) void k_gcg_const(GcgArgs A, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nc) return;
  const int NU = A.NU, NP = A.NP, nc = A.nc;
  const GcGeom g = gcg_geom(A, c);
  for (int a = 0; a < NU; ++a) {
    for (int b = 0; b < NU; ++b) {
      double acc = 0.0;
      for (int q = 0; q < A.nq; ++q) {
        const double* dN = A.tdNu + (size_t)q * NU * 2;
        const double ax = dN[2 * a] * g.inv[0][0] + dN[2 * a + 1] * g.inv[1][0], ay = dN[2 * a] * g.inv[0][1] + dN[2 * a + 1] * g.inv[1][1];
        const double bx = dN[2 * b] * g.inv[0][0] + dN[2 * b + 1] * g.inv[1][0], by = dN[2 * b] * g.inv[0][1] + dN[2 * b + 1] * g.inv[1][1];
        acc += A.w[q] * g.adet * (ax * bx + ay * by);
      }
      stash[(size_t)(a * NU + b) * nc + c] = acc;
    }
    for (int b = 0; b < NP; ++b) {
      double gx = 0.0, gy = 0.0;
      for (int q = 0; q < A.nq; ++q) {
        const double* dN = A.tdNu + (size_t)q * NU * 2;
        const double ax = dN[2 * a] * g.inv[0][0] + dN[2 * a + 1] * g.inv[1][0], ay = dN[2 * a] * g.inv[0][1] + dN[2 * a + 1] * g.inv[1][1];
        const double wl = A.w[q] * g.adet * A.tNp[(size_t)q * NP + b];
        gx += wl * ax;
        gy += wl * ay;
      }
      const size_t e0 = (size_t)NU * NU + ((size_t)(b * 2 + 0) * NU + a) * 2, e1 = (size_t)NU * NU + ((size_t)(b * 2 + 1) * NU + a) * 2;
      stash[e0 * nc + c] = gx;
      stash[(e0 + 1) * nc + c] = gx;
      stash[e1 * nc + c] = gy;
      stash[(e1 + 1) * nc + c] = gy;
    }
  }
}

// N(psi): slot (a*NP + b)*4 + {xx, xy, yx, yy}
__global__ __launch_bounds__(64) void k_gcg_jac_N(GcgArgs A, const double* __restrict__ phi, const double* __restrict__ x,
                                                  double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nc) return;
  const int NU = A.NU, NP = A.NP, nc = A.nc;
  const GcGeom g = gcg_geom(A, c);
  const int32_t* cu = A.cdu + (size_t)NU * c;
  const int32_t* cp = A.cdp + (size_t)NP * c;
  double cxx[GC_MAXQ], cxy[GC_MAXQ], cyy[GC_MAXQ];
  for (int q = 0; q < A.nq; ++q) {
    const double* Nu = A.tNu + (size_t)q * NU;
    const double* Np = A.tNp + (size_t)q * NP;
    double phq = 0, pxq = 0, pyq = 0;
    for (int a = 0; a < NU; ++a) phq += phi[cu[a]] * Nu[a];
    for (int b = 0; b < NP; ++b) {
      pxq += x[A.n2 + cp[b]] * Np[b];
      pyq += x[A.n2 + A.nv + cp[b]] * Np[b];
    }
    const double s = sqrt(1.0 + pxq * pxq + pyq * pyq), s3 = s * s * s, wp = A.w[q] * g.adet * phq;
    cxx[q] = wp * (1.0 / s - pxq * pxq / s3);
    cxy[q] = wp * (-pxq * pyq / s3);
    cyy[q] = wp * (1.0 / s - pyq * pyq / s3);
  }
  for (int a = 0; a < NP; ++a)
    for (int b = 0; b < NP; ++b) {
      double nxx = 0, nxy = 0, nyy = 0;
      for (int q = 0; q < A.nq; ++q) {
        const double ll = A.tNp[(size_t)q * NP + a] * A.tNp[(size_t)q * NP + b];
        nxx += cxx[q] * ll;
        nxy += cxy[q] * ll;
        nyy += cyy[q] * ll;
      }
      const size_t e = (size_t)(a * NP + b) * 4;
      stash[e * nc + c] = nxx;
      stash[(e + 1) * nc + c] = nxy;
      stash[(e + 2) * nc + c] = nxy;
      stash[(e + 3) * nc + c] = nyy;
    }
}

__global__ __launch_bounds__(256) void k_gcg_l2(GcgArgs A, const double* __restrict__ x, const double* __restrict__ xk,
                                                double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < A.nc; c += MX_RED * 256) {
    const GcGeom g = gcg_geom(A, c);
    const int32_t* cu = A.cdu + (size_t)A.NU * c;
    for (int q = 0; q < A.nq; ++q) {
      const double* Nu = A.tNu + (size_t)q * A.NU;
      double v = 0;
      for (int a = 0; a < A.NU; ++a) v += (x[cu[a]] - xk[cu[a]]) * Nu[a];
      s += A.w[q] * g.adet * v * v;
    }
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

static GcgArgs gcg_args(const pgx_gc_handle* h);

// ------------------------------------------------------------------------------------------------------------------
// evaluation at points of every cell (pgx_gc_eval_cells; gradient_constraint_dolfinx.py:134-165): one thread per (cell, point), so that
// every output array is written contiguously.  Any output pointer may be null.
// ------------------------------------------------------------------------------------------------------------------
struct GcEvalOut {
  double *grad_u, *feas, *phi;
  uint8_t *active, *feas_active;
};

__device__ inline void gc_eval_store(const GcEvalOut& o, int64_t i, double gux, double guy, double phq, double pxq, double pyq) {
  // the reference's expressions as stated: phi psi / sqrt(1 + psi.psi); sqrt(v.v) - phi against 0 (>=) and -1e-8 (>)
  const double s = sqrt(1.0 + (pxq * pxq + pyq * pyq));
  const double fx = phq * pxq / s, fy = phq * pyq / s;
  if (o.grad_u) reinterpret_cast<double2*>(o.grad_u)[i] = make_double2(gux, guy);
  if (o.feas) reinterpret_cast<double2*>(o.feas)[i] = make_double2(fx, fy);
  if (o.phi) o.phi[i] = phq;
  if (o.active) o.active[i] = (sqrt(gux * gux + guy * guy) - phq >= 0.0) ? 1 : 0;
  if (o.feas_active) o.feas_active[i] = (sqrt(fx * fx + fy * fy) - phq > -1e-8) ? 1 : 0;
}

__global__ __launch_bounds__(128) void k_gc_eval(int nc, int n2, int nv, const int32_t* __restrict__ cdofs, const double* __restrict__ coords,
                                                 const double* __restrict__ phi, const double* __restrict__ x, int npts,
                                                 const double* __restrict__ pts, GcEvalOut o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nc * npts) return;
  const int c = (int)(i / npts), p = (int)(i % npts);
  const int32_t* cd = cdofs + 6 * (size_t)c;
  const GcGeom g = gc_geom(coords, cd);
  double l[3], N[6], G[6][2];
  gc_tab(pts[2 * p], pts[2 * p + 1], g, l, N, G);
  double gux = 0, guy = 0, phq = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double ua = x[cd[a]];
    gux += ua * G[a][0];
    guy += ua * G[a][1];
    phq += phi[cd[a]] * N[a];
  }
  double pxq = 0, pyq = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    pxq += x[n2 + cd[b]] * l[b];
    pyq += x[n2 + nv + cd[b]] * l[b];
  }
  gc_eval_store(o, i, gux, guy, phq, pxq, pyq);
}

// general degree: A.tNu / A.tdNu / A.tNp are the tables at the EVALUATION points here
__global__ __launch_bounds__(128) void k_gcg_eval(GcgArgs A, const double* __restrict__ phi, const double* __restrict__ x, int npts,
                                                  GcEvalOut o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)A.nc * npts) return;
  const int c = (int)(i / npts), p = (int)(i % npts);
  const int NU = A.NU, NP = A.NP;
  const GcGeom g = gcg_geom(A, c);
  const int32_t* cu = A.cdu + (size_t)NU * c;
  const int32_t* cp = A.cdp + (size_t)NP * c;
  const double* Nu = A.tNu + (size_t)p * NU;
  const double* dN = A.tdNu + (size_t)p * NU * 2;
  const double* Np = A.tNp + (size_t)p * NP;
  double gux = 0, guy = 0, phq = 0, pxq = 0, pyq = 0;
  for (int a = 0; a < NU; ++a) {
    const double ua = x[cu[a]];
    gux += ua * (dN[2 * a] * g.inv[0][0] + dN[2 * a + 1] * g.inv[1][0]);
    guy += ua * (dN[2 * a] * g.inv[0][1] + dN[2 * a + 1] * g.inv[1][1]);
    phq += phi[cu[a]] * Nu[a];
  }
  for (int b = 0; b < NP; ++b) {
    pxq += x[A.n2 + cp[b]] * Np[b];
    pyq += x[A.n2 + A.nv + cp[b]] * Np[b];
  }
  gc_eval_store(o, i, gux, guy, phq, pxq, pyq);
}

// ------------------------------------------------------------------------------------------------------------------
// host: pattern, destination tables, create
// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_gc_destroy(pgx_gc_handle* h) { mx_destroy(h); }

static int gc_create_impl(pgx_gc_handle* h, const pgx_mesh* m, const pgx_gc_problem* p, pgx_comm* comm) {
  h->comm = comm;
  const int nv = m->n_vertices, nc = m->n_cells, n2 = m->n_dofs;
  const int64_t ntot = (int64_t)n2 + 2 * (int64_t)nv;
  h->nv = nv, h->nc = nc, h->n2 = n2, h->ntot = ntot;
  h->Q.nq = p->nq;
  for (int q = 0; q < p->nq; ++q) h->Q.X[q] = p->qpts[2 * q], h->Q.Y[q] = p->qpts[2 * q + 1], h->Q.w[q] = p->qwts[q];
  const int32_t* cd = m->cell_dofs;
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < 6; ++a) {
      const int v = cd[6 * (size_t)c + a];
      if (v < 0 || v >= n2 || (a < 3 && (v >= nv || v != m->cells[3 * (size_t)c + a])) || (a >= 3 && v < nv)) {
        h->err = "cell_dofs must be [vertex ids (== cells) | edge dofs >= n_vertices]";
        return PGX_EINVAL;
      }
    }
  std::vector<uint8_t> hmask(n2, 0);
  std::vector<double> hg(n2, 0.0);
  for (int k = 0; k < p->n_bc; ++k) {
    const int d = p->bc_dofs[k];
    if (d < 0 || d >= n2) {
      h->err = "bc dof out of range";
      return PGX_EINVAL;
    }
    hmask[d] = 1;
    hg[d] = p->bc_vals ? p->bc_vals[k] : 0.0;
  }
  // mixed dofs of a cell: 6 u, 3 psi_x, 3 psi_y
  auto mixed = [&](int c, int32_t md[12]) {
    for (int a = 0; a < 6; ++a) md[a] = cd[6 * (size_t)c + a];
    for (int b = 0; b < 3; ++b) md[6 + b] = n2 + cd[6 * (size_t)c + b], md[9 + b] = n2 + nv + cd[6 * (size_t)c + b];
  };
  // pattern: row r couples to every mixed dof of its cells
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  const PatFind find = pattern_from_entities(ntot, nc, [&](int64_t c, int32_t* md) { return mixed((int)c, md), 12; }, rowptr, col, h->err);
  if (!find) return PGX_EINVAL;
  const int64_t tot = h->nnz = rowptr[ntot];
  std::vector<uint8_t> kind;
  saddle_kinds(ntot, n2, hmask, rowptr, col, kind);
  // destination tables
  std::vector<int32_t> d108((size_t)nc * 108), d36((size_t)nc * 36), d12((size_t)nc * 12);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    for (int64_t c = a0; c < b0; ++c) {
      int32_t md[12];
      mixed((int)c, md);
      // slot-major like the stashes the element kernels write: table[slot * nc + cell]
      auto D = [&](int e) -> int32_t& { return d108[(size_t)e * nc + (size_t)c]; };
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) D(a * 6 + b) = find(md[a], md[b]);
      for (int b = 0; b < 3; ++b)
        for (int d = 0; d < 2; ++d)
          for (int a = 0; a < 6; ++a) {
            const int e = 36 + ((b * 2 + d) * 6 + a) * 2;
            const int32_t pr = md[6 + 3 * d + b];
            D(e) = find(pr, md[a]);
            D(e + 1) = find(md[a], pr);
          }
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
          for (int cc = 0; cc < 2; ++cc)
            for (int d = 0; d < 2; ++d)
              d36[(size_t)((a * 3 + b) * 4 + cc * 2 + d) * nc + (size_t)c] = find(md[6 + 3 * cc + a], md[6 + 3 * d + b]);
      for (int a = 0; a < 12; ++a) d12[(size_t)a * nc + (size_t)c] = md[a];
    }
  });
  // node coordinates for the nested-dissection ordering: vertices, then edge midpoints
  std::vector<double> xy(2 * (size_t)n2, 0.0);
  std::copy(m->coords, m->coords + 2 * (size_t)nv, xy.begin());
  for (int c = 0; c < nc; ++c) {
    const int ej[3] = {1, 0, 0}, ek[3] = {2, 2, 1};
    for (int i = 0; i < 3; ++i) {
      const int e = cd[6 * (size_t)c + 3 + i], vj = cd[6 * (size_t)c + ej[i]], vk = cd[6 * (size_t)c + ek[i]];
      xy[2 * (size_t)e] = 0.5 * (m->coords[2 * (size_t)vj] + m->coords[2 * (size_t)vk]);
      xy[2 * (size_t)e + 1] = 0.5 * (m->coords[2 * (size_t)vj + 1] + m->coords[2 * (size_t)vk + 1]);
    }
  }
  std::vector<int32_t> nod(ntot);
  for (int i = 0; i < n2; ++i) nod[i] = i;
  for (int v = 0; v < nv; ++v) nod[n2 + v] = nod[(size_t)n2 + nv + v] = v;
  // device
  GCHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, n2, nod.data(), 2, xy.data(), comm);
  if (rc) return rc;
  // the Newton matrix [[alpha K, G^T], [G, -N(psi)]] is symmetric (indefinite): L D L^T in LU clothing, half the flops (pgx_nd.h)
  pgx_nd_set_symmetric(h->lu, 1);
  GCALLOC(h->coords, 2 * (size_t)nv);
  GCALLOC(h->cdofs, 6 * (size_t)nc);
  GCALLOC(h->mask, n2);
  GCALLOC(h->gbc, n2);
  GCALLOC(h->phi, n2);
  GCALLOC(h->f, n2);
  GCALLOC(h->kind, tot);
  GCALLOC(h->stash, (size_t)36 * nc);
  GCALLOC(h->Jc, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  GCHIP(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->cdofs, cd, sizeof(int32_t) * 6 * (size_t)nc, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->mask, hmask.data(), n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->gbc, hg.data(), sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->phi, p->phi_dofs, sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->f, p->f_dofs, sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  {
    std::string e1 = pgx_scatter_build(d12.data(), (int64_t)12 * nc, ntot, h->allocs, &h->sc_res);
    if (e1.empty()) e1 = pgx_scatter_build(d36.data(), (int64_t)36 * nc, tot, h->allocs, &h->sc_N);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  // constant blocks, once: park 108 entries per cell, sum per CSR position
  GCHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  return mx_scatter_once(h, d108.data(), 108, nc, tot, nullptr, [&](double* stash) {
    hipLaunchKernelGGL(k_gc_const, dim3((nc + 127) / 128), dim3(128), 0, h->st, nc, h->cdofs, h->coords, h->Q, stash);
  }, h->Jc, 0);
}

static GcgArgs gcg_args(const pgx_gc_handle* h) {
  GcgArgs A{};
  A.nc = h->nc, A.n2 = h->n2, A.nv = h->nv, A.NU = h->NU, A.NP = h->NP, A.nq = h->Q.nq;
  A.cells = h->cells3, A.cdu = h->cdofs, A.cdp = h->cdofs_p;
  A.coords = h->coords, A.tNu = h->tNu, A.tdNu = h->tdNu, A.tNp = h->tNp;
  for (int q = 0; q < h->Q.nq; ++q) A.w[q] = h->Q.w[q];
  return A;
}

// general degree: same construction as gc_create_impl with run-time element sizes (see pgx_gc.h: pgx_gc_spaces)
static int gcg_create_impl(pgx_gc_handle* h, const pgx_gc_spaces* sp, const pgx_gc_problem* p, pgx_comm* comm) {
  h->comm = comm;
  h->gen = 1;
  const int NU = sp->nu, NP = sp->np, ND = NU + 2 * NP;
  const int nc = sp->n_cells, n2 = sp->n_u, nv = sp->n_p, nvert = sp->n_vertices;
  const int64_t ntot = (int64_t)n2 + 2 * (int64_t)nv;
  h->NU = NU, h->NP = NP, h->nv = nv, h->nc = nc, h->n2 = n2, h->ntot = ntot;
  h->Q.nq = p->nq;
  for (int q = 0; q < p->nq; ++q) h->Q.X[q] = p->qpts[2 * q], h->Q.Y[q] = p->qpts[2 * q + 1], h->Q.w[q] = p->qwts[q];
  const int32_t *cdu = sp->cell_dofs_u, *cdp = sp->cell_dofs_p;
  for (size_t k = 0; k < (size_t)NU * nc; ++k)
    if (cdu[k] < 0 || cdu[k] >= n2) {
      h->err = "primal cell dof out of range";
      return PGX_EINVAL;
    }
  for (size_t k = 0; k < (size_t)NP * nc; ++k)
    if (cdp[k] < 0 || cdp[k] >= nv) {
      h->err = "latent cell dof out of range";
      return PGX_EINVAL;
    }
  if (const char* e = check_cells(sp->cells, 3, nc, nvert)) {
    h->err = e;
    return PGX_EINVAL;
  }
  std::vector<uint8_t> hmask(n2, 0);
  std::vector<double> hg(n2, 0.0);
  for (int k = 0; k < p->n_bc; ++k) {
    const int d = p->bc_dofs[k];
    if (d < 0 || d >= n2) {
      h->err = "bc dof out of range";
      return PGX_EINVAL;
    }
    hmask[d] = 1;
    hg[d] = p->bc_vals ? p->bc_vals[k] : 0.0;
  }
  auto mixed = [&](int c, int32_t* md) {  // NU u dofs, NP psi_x, NP psi_y
    for (int a = 0; a < NU; ++a) md[a] = cdu[(size_t)NU * c + a];
    for (int b = 0; b < NP; ++b) md[NU + b] = n2 + cdp[(size_t)NP * c + b], md[NU + NP + b] = n2 + nv + cdp[(size_t)NP * c + b];
  };
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  const PatFind find = pattern_from_entities(ntot, nc, [&](int64_t c, int32_t* md) { return mixed((int)c, md), ND; }, rowptr, col, h->err);
  if (!find) return PGX_EINVAL;
  const int64_t tot = h->nnz = rowptr[ntot];
  std::vector<uint8_t> kind;
  saddle_kinds(ntot, n2, hmask, rowptr, col, kind);
  const size_t nsc = (size_t)NU * NU + 4 * (size_t)NP * NU, nsn = 4 * (size_t)NP * NP;
  if ((double)(nsc + nsn + ND) * nc * 12.0 > 96e9) {
    h->err = "mesh too large for the one-pass assembly at this degree";
    return PGX_ENOMEM;
  }
  std::vector<int32_t> dC(nsc * nc), dN(nsn * nc), dR((size_t)ND * nc);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    std::vector<int32_t> md(ND);
    for (int64_t c = a0; c < b0; ++c) {
      mixed((int)c, md.data());
      for (int a = 0; a < NU; ++a)
        for (int b = 0; b < NU; ++b) dC[(size_t)(a * NU + b) * nc + (size_t)c] = find(md[a], md[b]);
      for (int b = 0; b < NP; ++b)
        for (int d = 0; d < 2; ++d)
          for (int a = 0; a < NU; ++a) {
            const size_t e = (size_t)NU * NU + ((size_t)(b * 2 + d) * NU + a) * 2;
            const int32_t pr = md[NU + NP * d + b];
            dC[e * nc + (size_t)c] = find(pr, md[a]);
            dC[(e + 1) * nc + (size_t)c] = find(md[a], pr);
          }
      for (int a = 0; a < NP; ++a)
        for (int b = 0; b < NP; ++b)
          for (int cc = 0; cc < 2; ++cc)
            for (int d = 0; d < 2; ++d)
              dN[((size_t)(a * NP + b) * 4 + cc * 2 + d) * nc + (size_t)c] = find(md[NU + NP * cc + a], md[NU + NP * d + b]);
      for (int a = 0; a < ND; ++a) dR[(size_t)a * nc + (size_t)c] = md[a];
    }
  });
  // nested dissection nodes: the primal nodes, then the latent nodes (each carries psi_x and psi_y)
  std::vector<double> xy(2 * ((size_t)n2 + nv));
  std::copy(sp->coords_u, sp->coords_u + 2 * (size_t)n2, xy.begin());
  std::copy(sp->coords_p, sp->coords_p + 2 * (size_t)nv, xy.begin() + 2 * (size_t)n2);
  std::vector<int32_t> nod(ntot);
  for (int i = 0; i < n2; ++i) nod[i] = i;
  for (int v = 0; v < nv; ++v) nod[n2 + v] = nod[(size_t)n2 + nv + v] = n2 + v;
  GCHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, n2 + nv, nod.data(), 2, xy.data(), comm);
  if (rc) return rc;
  pgx_nd_set_symmetric(h->lu, 1);  // (symmetric Newton matrix, as above)
  const int nq = p->nq;
  GCALLOC(h->coords, 2 * (size_t)nvert);
  GCALLOC(h->cells3, 3 * (size_t)nc);
  GCALLOC(h->cdofs, (size_t)NU * nc);
  GCALLOC(h->cdofs_p, (size_t)NP * nc);
  GCALLOC(h->tNu, (size_t)nq * NU);
  GCALLOC(h->tdNu, (size_t)nq * NU * 2);
  GCALLOC(h->tNp, (size_t)nq * NP);
  GCALLOC(h->mask, n2);
  GCALLOC(h->gbc, n2);
  GCALLOC(h->phi, n2);
  GCALLOC(h->f, n2);
  GCALLOC(h->kind, tot);
  GCALLOC(h->stash, std::max(nsn, (size_t)ND) * nc);
  GCALLOC(h->Jc, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  GCHIP(hipMemcpy(h->coords, sp->coords, sizeof(double) * 2 * nvert, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->cells3, sp->cells, sizeof(int32_t) * 3 * (size_t)nc, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->cdofs, cdu, sizeof(int32_t) * (size_t)NU * nc, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->cdofs_p, cdp, sizeof(int32_t) * (size_t)NP * nc, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->tNu, sp->tab_Nu, sizeof(double) * (size_t)nq * NU, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->tdNu, sp->tab_dNu, sizeof(double) * (size_t)nq * NU * 2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->tNp, sp->tab_Np, sizeof(double) * (size_t)nq * NP, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->mask, hmask.data(), n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->gbc, hg.data(), sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->phi, p->phi_dofs, sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->f, p->f_dofs, sizeof(double) * n2, hipMemcpyHostToDevice));
  GCHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  {
    std::string e1 = pgx_scatter_build(dR.data(), (int64_t)ND * nc, ntot, h->allocs, &h->sc_res);
    if (e1.empty()) e1 = pgx_scatter_build(dN.data(), (int64_t)nsn * nc, tot, h->allocs, &h->sc_N);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  GCHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  return mx_scatter_once(h, dC.data(), (int64_t)nsc, nc, tot, nullptr, [&](double* stash) {
    hipLaunchKernelGGL(k_gcg_const, dim3((nc + 63) / 64), dim3(64), 0, h->st, gcg_args(h), stash);
  }, h->Jc, 0);
}

extern "C" int pgx_gc_create_general(const pgx_gc_spaces* sp, const pgx_gc_problem* p, int device, pgx_gc_handle** out) {
  if (!sp || !p || !out || !sp->coords || !sp->cells || !sp->cell_dofs_u || !sp->cell_dofs_p || !sp->coords_u || !sp->coords_p ||
      !sp->tab_Nu || !sp->tab_dNu || !sp->tab_Np || sp->nu < 3 || sp->nu > GCG_MAXU || sp->np < 1 || sp->np > GCG_MAXP ||
      sp->n_cells <= 0 || sp->n_u <= 0 || sp->n_p <= 0 || !p->qpts || !p->qwts || !p->phi_dofs || !p->f_dofs || p->nq <= 0 ||
      p->nq > GC_MAXQ || (p->n_bc > 0 && !p->bc_dofs)) {
    g_gc_error = "pgx_gc_create_general: bad arguments";
    return PGX_EINVAL;
  }
  return mx_create("pgx_gc_create_general", g_gc_error, device, out, [&](pgx_gc_handle* h) { return gcg_create_impl(h, sp, p, nullptr); });
}

static int gc_create(const pgx_mesh* m, const pgx_gc_problem* p, pgx_comm* comm, int device, pgx_gc_handle** out) {
  if (!m || !p || !out || !m->coords || !m->cells || !m->cell_dofs || m->n_dofs <= m->n_vertices || !p->qpts || !p->qwts ||
      !p->phi_dofs || !p->f_dofs || p->nq <= 0 || p->nq > GC_MAXQ || (p->n_bc > 0 && !p->bc_dofs)) {
    g_gc_error = "pgx_gc_create: bad arguments";
    return PGX_EINVAL;
  }
  return mx_create("pgx_gc_create", g_gc_error, device, out, [&](pgx_gc_handle* h) { return gc_create_impl(h, m, p, comm); });
}

extern "C" int pgx_gc_create(const pgx_mesh* m, const pgx_gc_problem* p, int device, pgx_gc_handle** out) {
  return gc_create(m, p, nullptr, device, out);
}
extern "C" int pgx_gc_create_dist(const pgx_mesh* m, const pgx_gc_problem* p, pgx_comm* comm, int device, pgx_gc_handle** out) {
  if (!comm) {
    g_gc_error = "pgx_gc_create_dist: null communicator";
    return PGX_EINVAL;
  }
  return gc_create(m, p, comm, device, out);
}
extern "C" int pgx_gc_lu_stats(const pgx_gc_handle* h, pgx_nd_stats* st) { return h ? pgx_nd_get_stats(h->lu, st) : PGX_EINVAL; }
extern "C" int pgx_gc_lu_is_symmetric(const pgx_gc_handle* h) { return h ? pgx_nd_is_symmetric(h->lu) : 0; }

extern "C" int pgx_gc_num_dofs(const pgx_gc_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_gc_set_state(pgx_gc_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_gc_get_state(pgx_gc_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_gc_set_prev(pgx_gc_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_gc_get_prev(pgx_gc_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_gc_advance_prev(pgx_gc_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_gc_set_alpha(pgx_gc_handle* h, double a) { return mx_set_alpha(h, a); }

void pgx_gc_handle::residual_dev(const double* xin, double* Fout) {
  pgx_gc_handle* h = this;
  GcTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  if (h->gen) {
    if (h->NU <= GCG_TRIU && h->NP <= GCG_TRIP)
      hipLaunchKernelGGL((k_gcg_residual<GCG_TRIU, GCG_TRIP>), dim3((h->nc + 63) / 64), dim3(64), 0, h->st, gcg_args(h), h->mask, h->gbc,
                         h->phi, h->f, xin, h->xk, h->alpha, h->stash);
    else
      hipLaunchKernelGGL((k_gcg_residual<GCG_MAXU, GCG_MAXP>), dim3((h->nc + 63) / 64), dim3(64), 0, h->st, gcg_args(h), h->mask, h->gbc,
                         h->phi, h->f, xin, h->xk, h->alpha, h->stash);
    pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
    hipLaunchKernelGGL(k_gc_resid_bc, dim3((h->n2 + 255) / 256), dim3(256), 0, h->st, h->n2, h->mask, h->gbc, xin, Fout);
    return;
  }
  hipLaunchKernelGGL(k_gc_residual, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->n2, h->nv, h->cdofs, h->coords,
                     h->mask, h->gbc, h->phi, h->f, xin, h->xk, h->alpha, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
  hipLaunchKernelGGL(k_gc_resid_bc, dim3((h->n2 + 255) / 256), dim3(256), 0, h->st, h->n2, h->mask, h->gbc, xin, Fout);
}
void pgx_gc_handle::jacobian_dev(const double* xin) {
  pgx_gc_handle* h = this;
  GcTimer t(h, 1);
  hipLaunchKernelGGL(k_gc_jac_init, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->st, h->nnz, h->kind, h->Jc,
                     h->alpha, h->Jv);
  if (h->gen)
    hipLaunchKernelGGL(k_gcg_jac_N, dim3((h->nc + 63) / 64), dim3(64), 0, h->st, gcg_args(h), h->phi, xin, h->stash);
  else
    hipLaunchKernelGGL(k_gc_jac_N, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->n2, h->nv, h->cdofs, h->coords,
                       h->phi, xin, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_N, h->stash, -1.0, 1, h->Jv);  // the latent block is -N(psi)
  h->jac_valid = true;
}
extern "C" int pgx_gc_residual(pgx_gc_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_gc_jacobian_fill(pgx_gc_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_gc_csr_export(pgx_gc_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col,
                                 double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_gc_spmv(pgx_gc_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }

extern "C" int pgx_gc_l2_increment(pgx_gc_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  if (h->gen)
    hipLaunchKernelGGL(k_gcg_l2, dim3(GC_RED), dim3(256), 0, h->st, gcg_args(h), h->x, h->xk, h->partials);
  else
    hipLaunchKernelGGL(k_gc_l2, dim3(GC_RED), dim3(256), 0, h->st, h->nc, h->cdofs, h->coords, h->x, h->xk, h->Q, h->partials);
  return mx_partials_sqrt(h, out);
}

extern "C" int pgx_gc_eval_cells(pgx_gc_handle* h, const pgx_gc_points* p, double* grad_u, double* feas, double* phi, uint8_t* active,
                                 uint8_t* feasible_active) {
  MXNEED(h);
  if (!p || p->npts < 1 || p->npts > 64 || (h->gen ? (!p->tab_Nu || !p->tab_dNu || !p->tab_Np) : !p->pts)) {
    h->err = h->gen ? "pgx_gc_eval_cells: 1..64 points and the three basis tables at them (handle of pgx_gc_create_general)"
                    : "pgx_gc_eval_cells: 1..64 points with their reference coordinates";
    return PGX_EINVAL;
  }
  const int np = p->npts;
  const size_t n = (size_t)h->nc * np;
  // one buffer: [tables | grad_u | feas | phi | active | feasible_active], the outputs only where asked for
  const size_t ntab = h->gen ? (size_t)np * (3 * (size_t)h->NU + h->NP) : 2 * (size_t)np;
  size_t len = (sizeof(double) * ntab + 15) / 16 * 16;  // (the vector outputs are stored as double2)
  const size_t o_gu = len;
  len += grad_u ? sizeof(double) * 2 * n : 0;
  const size_t o_fe = len;
  len += feas ? sizeof(double) * 2 * n : 0;
  const size_t o_ph = len;
  len += phi ? sizeof(double) * n : 0;
  const size_t o_ac = len;
  len += active ? n : 0;
  const size_t o_fa = len;
  len += feasible_active ? n : 0;
  if (len > h->ev_len) {
    uint8_t* q = nullptr;
    GCALLOC(q, len);
    h->ev = q, h->ev_len = len;
  }
  uint8_t* base = (uint8_t*)h->ev;
  double* tab = (double*)base;
  GcEvalOut o{};
  o.grad_u = grad_u ? (double*)(base + o_gu) : nullptr;
  o.feas = feas ? (double*)(base + o_fe) : nullptr;
  o.phi = phi ? (double*)(base + o_ph) : nullptr;
  o.active = active ? base + o_ac : nullptr;
  o.feas_active = feasible_active ? base + o_fa : nullptr;
  const dim3 grid((unsigned)((n + 127) / 128)), block(128);
  if (h->gen) {
    const size_t nNu = (size_t)np * h->NU, nNp = (size_t)np * h->NP;
    GCHIP(hipMemcpyAsync(tab, p->tab_Nu, sizeof(double) * nNu, hipMemcpyHostToDevice, h->st));
    GCHIP(hipMemcpyAsync(tab + nNu, p->tab_dNu, sizeof(double) * 2 * nNu, hipMemcpyHostToDevice, h->st));
    GCHIP(hipMemcpyAsync(tab + 3 * nNu, p->tab_Np, sizeof(double) * nNp, hipMemcpyHostToDevice, h->st));
    GcgArgs A = gcg_args(h);
    A.tNu = tab, A.tdNu = tab + nNu, A.tNp = tab + 3 * nNu;
    hipLaunchKernelGGL(k_gcg_eval, grid, block, 0, h->st, A, h->phi, h->x, np, o);
  } else {
    GCHIP(hipMemcpyAsync(tab, p->pts, sizeof(double) * 2 * np, hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL(k_gc_eval, grid, block, 0, h->st, h->nc, h->n2, h->nv, h->cdofs, h->coords, h->phi, h->x, np, tab, o);
  }
  if (grad_u) GCHIP(hipMemcpyAsync(grad_u, o.grad_u, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->st));
  if (feas) GCHIP(hipMemcpyAsync(feas, o.feas, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->st));
  if (phi) GCHIP(hipMemcpyAsync(phi, o.phi, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
  if (active) GCHIP(hipMemcpyAsync(active, o.active, n, hipMemcpyDeviceToHost, h->st));
  if (feasible_active) GCHIP(hipMemcpyAsync(feasible_active, o.feas_active, n, hipMemcpyDeviceToHost, h->st));
  GCHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}

extern "C" int pgx_gc_profile(pgx_gc_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

// linesearch 1: bt; every other value (2 included): plain Newton
extern "C" int pgx_gc_newton_solve(pgx_gc_handle* h, const pgx_snes_opts* opts, int* reason, int* its_out, int* lin_out) {
  return mx_newton(h, opts, reason, its_out, lin_out, false);
}
