// pgx_ev.hip - example 07 (eigenvalue-constrained 2-D Q-tensor: q1, q2, psi1, psi2 in Q_p on a uniform grid of rectangles) behind the
// C ABI of include/pgx_ev.h.  Reference: examples/07_eigenvalue_constraints/eigenvalue_constraints_dolfinx.py (:41-50 space, :31-33
// the script's tanh, :67-84 energy and residual, :86-141 Dirichlet data, :143 solver, :162-227 loop, :245-259 nodal output).
// x = [q1 | q2 | psi1 | psi2]; the 4 x 4 block Jacobian lives in one mixed CSR array: 12 blocks on the scalar Q_p pattern (the
// structurally zero (q1,psi2), (q2,psi1) and their transposes are left out).  The element matrices M_e and K_e are the same for
// every cell and are computed once on the host with the caller's rule; the iterate-independent part Jc - alpha 2 K on (q_i,q_i),
// 2 M on (q_i,psi_i) and (psi_i,q_i), the identity on the Dirichlet rows - is recombined only when alpha changes.  Every Newton step
// copies Jc and adds six weighted mass blocks per cell: three of alpha E''(q) - 2 K and three of -2 D(psi).
//
// Kernels: ONE WAVEFRONT PER CELL, EV_WPB cells per workgroup.  With up to 121 points and 4 x 16 local unknowns a cell does not fit
// one thread.  Phase 1: lanes over the quadrature points evaluate the fields through the 1-D tables (tensor product) and leave the
// weighted coefficient fields in LDS (6 x 121 doubles per cell for the Jacobian, 4 x 121 for the residual).  Phase 2: lanes over the
// symmetric node pairs (Jacobian) or over the 4 (p+1)^2 rows (residual) sum over the points.  Every lane of a wave reads the same
// coefficient address (a broadcast), the per-lane reads of the 1-D products touch at most 16 consecutive doubles (32 banks, no
// conflict), the phase-1 stores are consecutive doubles.  Results are parked cell-major and summed per destination in a fixed order
// by pgx_scatter.h: no atomics, bitwise reproducible; both triangles of a block receive the SAME value, so the exported matrix is
// symmetric to the last bit.
//
// Dirichlet rows: E'' depends on q, so imposing the boundary values inside the element evaluation would NOT give DOLFINx's
// F_raw(x) + J(x)[:, bc] (g - x_bc).  The lifting is done element-locally: with dq = g - x_b on the cell's Dirichlet nodes and 0 on
// the others, the element Jacobian columns times dq are the directional derivative of the element residual along dq, which phase 1
// evaluates at the points together with the residual itself.
#include <cstring>

#include "../../include/pgx_ev.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"

#define EV_MAXQ 11                      // points of the 1-D rule
#define EV_MAXPTS (EV_MAXQ * EV_MAXQ)   // 121
#define EV_WPB 4                        // cells (wavefronts) per workgroup
#define EV_RSMALL 1.0e-4                // below: the series of g and g' / r

// 1-D tables and the element matrices of the uniform mesh (device copy: the kernels index them per lane)
struct EvTab {
  double B[EV_MAXQ * 4];  // B[q * 4 + i]: basis i at point q
  double w[EV_MAXQ];
  double Me[256], Ke[256];  // [a * 16 + b], a = iy (p+1) + ix
};

static thread_local std::string g_ev_error;

struct pgx_ev_handle : MixedBase {
  int Nx = 0, Ny = 0, p = 0, nq = 0, Lx = 0;
  int n = 0, nc = 0;  // lattice dofs per field, cells
  double A = 1.0, C = 4.0, area = 0.0;
  double alpha_J = -1.0;  // alpha the constant part Jc was recombined with (< 0: never)
  EvTab* tab = nullptr;
  uint8_t* isbc = nullptr;  // [n]
  double* gv = nullptr;     // [2 n] Dirichlet values of q1 | q2 at the bc dofs, 0 elsewhere
  // deterministic assembly (pgx_scatter.h): residual 4 nb slots per cell -> dofs; the six blocks, 6 nb^2 slots per cell -> CSR, the
  // two mixed blocks (q1,q2) and (psi1,psi2) a second time into their transposes
  PgxScatter sc_res, sc_jac, sc_jac_t;
  double* stash = nullptr;  // [6 nb^2 nc]
  double* Sc = nullptr;     // [2 nnz_s] scalar M | K on the Q_p pattern
  uint8_t* kind = nullptr;
  int32_t* src = nullptr;   // scalar-pattern index of every mixed entry
  double* Jc = nullptr;     // [nnz] iterate-independent part of the Jacobian at alpha_J
  double* d_nodes = nullptr;  // [4 n] eval_nodes
  pgx_ev_handle() : MixedBase("pgx_ev") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

extern "C" const char* pgx_ev_last_error(const pgx_ev_handle* h) { return h ? h->err.c_str() : g_ev_error.c_str(); }

// g(r) = tanh(r / 2) / r and h(r) = g'(r) / r from e = exp(-r) <= 1: finite for every finite r >= 0
__device__ inline void ev_g(double r, double* g, double* h) {
  if (r < EV_RSMALL) {
    *g = 0.5 - r * r / 24.0;
    *h = -1.0 / 12.0 + r * r / 60.0;
    return;
  }
  const double e = exp(-r), t = (1.0 - e) / (1.0 + e), sech2 = 4.0 * e / ((1.0 + e) * (1.0 + e));
  *g = t / r;
  *h = (0.5 * r * sech2 - t) / (r * r * r);
}

// lattice dof of local node a of a cell
template <int P>
__device__ inline int ev_dof(int cell, int a, int Nx, int Lx) {
  const int cy = cell / Nx, cx = cell - cy * Nx, iy = a / (P + 1), ix = a - iy * (P + 1);
  return (P * cy + iy) * Lx + P * cx + ix;
}

// residual of one cell per wavefront, lifting included: stash[cell * 4 nb + f * nb + a]
template <int P>
__global__ __launch_bounds__(64 * EV_WPB) void k_ev_residual(int nc, int Nx, int Lx, int n, int nq, const EvTab* __restrict__ tab,
                                                             const double* __restrict__ x, const double* __restrict__ xk,
                                                             const uint8_t* __restrict__ isbc, const double* __restrict__ gv,
                                                             double alpha, double A, double C, double area,
                                                             double* __restrict__ stash) {
  constexpr int P1 = P + 1, NB = P1 * P1;
  __shared__ double sB[EV_MAXQ * 4], sW[EV_MAXQ];
  __shared__ double sU[EV_WPB][8][16];  // nodal q1, q2, psi1, psi2, psi1 - psi_iter1, psi2 - psi_iter2, dq1, dq2
  __shared__ double sF[EV_WPB][4][EV_MAXPTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < nq * 4; i += 64 * EV_WPB) sB[i] = tab->B[i];
  for (int i = tid; i < nq; i += 64 * EV_WPB) sW[i] = tab->w[i];
  const int cell = blockIdx.x * EV_WPB + wave;
  const bool active = cell < nc;
  if (active && lane < 4 * NB) {
    const int f = lane / NB, a = lane - f * NB;
    const int dof = ev_dof<P>(cell, a, Nx, Lx);
    const double v = x[(size_t)f * n + dof];
    sU[wave][f][a] = v;
    if (f < 2)
      sU[wave][6 + f][a] = isbc[dof] ? gv[(size_t)f * n + dof] - v : 0.0;  // g - x_b on the cell's Dirichlet nodes
    else
      sU[wave][2 + f][a] = v - xk[(size_t)f * n + dof];
  }
  __syncthreads();
  const int npts = nq * nq;
  if (active)
    for (int pt = lane; pt < npts; pt += 64) {
      const int qy = pt / nq, qx = pt - qy * nq;
      double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1  // the nodal values stay in LDS (broadcast reads): hoisting all of them costs up to 256 VGPRs
      for (int iy = 0; iy < P1; ++iy)
#pragma unroll
        for (int ix = 0; ix < P1; ++ix) {
          const double bb = sB[qy * 4 + iy] * sB[qx * 4 + ix];
#pragma unroll
          for (int f = 0; f < 8; ++f) v[f] += bb * sU[wave][f][iy * P1 + ix];
        }
      const double wq = sW[qy] * sW[qx] * area;
      const double q1 = v[0], q2 = v[1], dq1 = v[6], dq2 = v[7];
      const double pot = 2.0 * A + 4.0 * C * (q1 * q1 + q2 * q2), cross = 8.0 * C * (q1 * dq1 + q2 * dq2);
      double g, hh;
      ev_g(sqrt(v[2] * v[2] + v[3] * v[3]), &g, &hh);
      sF[wave][0][pt] = wq * (alpha * (pot * (q1 + dq1) + cross * q1) + 2.0 * v[4]);  // :72-74, :79-81 and the lifting
      sF[wave][1][pt] = wq * (alpha * (pot * (q2 + dq2) + cross * q2) + 2.0 * v[5]);
      sF[wave][2][pt] = wq * 2.0 * (q1 + dq1 - g * v[2]);                               // :82-83
      sF[wave][3][pt] = wq * 2.0 * (q2 + dq2 - g * v[3]);
    }
  __syncthreads();
  if (active && lane < 4 * NB) {
    const int f = lane / NB, a = lane - f * NB, ay = a / P1, ax = a - ay * P1;
    double R = 0.0;
    for (int qy = 0; qy < nq; ++qy) {
      const double ya = sB[qy * 4 + ay];
      for (int qx = 0; qx < nq; ++qx) R += ya * sB[qx * 4 + ax] * sF[wave][f][qy * nq + qx];
    }
    if (f < 2) {  // alpha 2 (grad q_i, grad w_i), the Dirichlet columns included (:72)
      double k = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b) k += tab->Ke[a * 16 + b] * (sU[wave][f][b] + sU[wave][6 + f][b]);
      R += 2.0 * alpha * k;
    }
    stash[(size_t)cell * (4 * NB) + lane] = R;
  }
}
__global__ void k_ev_resid_bc(int n, const uint8_t* __restrict__ isbc, const double* __restrict__ x, const double* __restrict__ gv,
                              double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && isbc[i]) {
    F[i] = x[i] - gv[i];
    F[(size_t)n + i] = x[(size_t)n + i] - gv[(size_t)n + i];
  }
}

// kind: 0 = zero, 1 = alpha 2 K (q_i,q_i), 2 = 2 M (q_i,psi_i) and (psi_i,q_i), 5 = Dirichlet diagonal
__global__ void k_ev_recombine(int64_t nnz, int64_t nnz_s, const uint8_t* __restrict__ kind, const int32_t* __restrict__ src,
                               const double* __restrict__ Sc, double alpha, double* __restrict__ Jc) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int t = kind[e];
  const int64_t s = src[e];
  Jc[e] = t == 1 ? alpha * 2.0 * Sc[nnz_s + s] : t == 2 ? 2.0 * Sc[s] : t == 5 ? 1.0 : 0.0;
}

// the six weighted mass blocks of one cell per wavefront: stash[cell * 6 nb^2 + blk * nb^2 + a * nb + b],
// blk = (q1,q1), (q2,q2), (psi1,psi1), (psi2,psi2), (q1,q2), (psi1,psi2)
template <int P>
__global__ __launch_bounds__(64 * EV_WPB) void k_ev_jac(int nc, int Nx, int Lx, int n, int nq, const EvTab* __restrict__ tab,
                                                        const double* __restrict__ x, double alpha, double A, double C, double area,
                                                        double* __restrict__ stash) {
  constexpr int P1 = P + 1, NB = P1 * P1, NPAIR = NB * (NB + 1) / 2;
  __shared__ double sB[EV_MAXQ * 4], sBB[EV_MAXQ * 16], sW[EV_MAXQ];  // sBB[q * 16 + i * 4 + j] = B[q][i] B[q][j]
  __shared__ double sU[EV_WPB][4][16];
  __shared__ double sC[EV_WPB][6][EV_MAXPTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < nq * 4; i += 64 * EV_WPB) sB[i] = tab->B[i];
  for (int i = tid; i < nq; i += 64 * EV_WPB) sW[i] = tab->w[i];
  for (int i = tid; i < nq * 16; i += 64 * EV_WPB) sBB[i] = tab->B[(i >> 4) * 4 + ((i >> 2) & 3)] * tab->B[(i >> 4) * 4 + (i & 3)];
  const int cell = blockIdx.x * EV_WPB + wave;
  const bool active = cell < nc;
  if (active && lane < 4 * NB) {
    const int f = lane / NB, a = lane - f * NB;
    sU[wave][f][a] = x[(size_t)f * n + ev_dof<P>(cell, a, Nx, Lx)];
  }
  __syncthreads();
  const int npts = nq * nq;
  if (active)
    for (int pt = lane; pt < npts; pt += 64) {
      const int qy = pt / nq, qx = pt - qy * nq;
      double v[4] = {0, 0, 0, 0};
#pragma unroll 1  // the nodal values stay in LDS (broadcast reads): hoisting all of them costs up to 256 VGPRs
      for (int iy = 0; iy < P1; ++iy)
#pragma unroll
        for (int ix = 0; ix < P1; ++ix) {
          const double bb = sB[qy * 4 + iy] * sB[qx * 4 + ix];
#pragma unroll
          for (int f = 0; f < 4; ++f) v[f] += bb * sU[wave][f][iy * P1 + ix];
        }
      const double wq = sW[qy] * sW[qx] * area;
      const double pot = 2.0 * A + 4.0 * C * (v[0] * v[0] + v[1] * v[1]), c8 = 8.0 * C;
      double g, hh;
      ev_g(sqrt(v[2] * v[2] + v[3] * v[3]), &g, &hh);
      sC[wave][0][pt] = wq * alpha * (pot + c8 * v[0] * v[0]);
      sC[wave][1][pt] = wq * alpha * (pot + c8 * v[1] * v[1]);
      sC[wave][2][pt] = -2.0 * wq * (g + hh * v[2] * v[2]);
      sC[wave][3][pt] = -2.0 * wq * (g + hh * v[3] * v[3]);
      sC[wave][4][pt] = wq * alpha * c8 * v[0] * v[1];
      sC[wave][5][pt] = -2.0 * wq * hh * v[2] * v[3];
    }
  __syncthreads();
  if (active)
    for (int t = lane; t < NPAIR; t += 64) {
      int a = 0, b = t;  // pair t of the upper triangle, row by row: a <= b
      while (b >= NB - a) b -= NB - a, ++a;
      b += a;
      const int ay = a / P1, ax = a - ay * P1, by = b / P1, bx = b - by * P1;
      const int iyy = ay * 4 + by, ixx = ax * 4 + bx;
      double acc[6] = {0, 0, 0, 0, 0, 0};
      for (int qy = 0; qy < nq; ++qy) {
        const double yy = sBB[qy * 16 + iyy];
        for (int qx = 0; qx < nq; ++qx) {
          const double ww = yy * sBB[qx * 16 + ixx];
          const int pt = qy * nq + qx;
#pragma unroll
          for (int k = 0; k < 6; ++k) acc[k] += ww * sC[wave][k][pt];
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

// 2 sum over cells of d1^T M_e d1 + d2^T M_e d2, d = x - y on the q blocks (:157: inner of two Q-tensors carries the factor 2): per-block partials
template <int P>
__global__ __launch_bounds__(256) void k_ev_l2(int nc, int Nx, int Lx, int n, const EvTab* __restrict__ tab, const double* __restrict__ x,
                                               const double* __restrict__ y, double* __restrict__ partials) {
  constexpr int NB = (P + 1) * (P + 1);
  __shared__ double sh[256];
  double s = 0.0;
  for (int cell = blockIdx.x * 256 + threadIdx.x; cell < nc; cell += MX_RED * 256)
    for (int f = 0; f < 2; ++f) {
      double d[NB];
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        const size_t i = (size_t)f * n + ev_dof<P>(cell, a, Nx, Lx);
        d[a] = x[i] - y[i];
      }
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) s += tab->Me[a * 16 + b] * d[a] * d[b];
    }
  sh[threadIdx.x] = 2.0 * s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// per dof: T(psi) = g(r) psi (:245-246) and the eigenvalues +- sqrt(q1^2 + q2^2) of Q (:251-259): out = [T1 | T2 | max | min]
__global__ void k_ev_nodes(int n, const double* __restrict__ x, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double q1 = x[i], q2 = x[(size_t)n + i], p1 = x[2 * (size_t)n + i], p2 = x[3 * (size_t)n + i];
  double g, hh;
  ev_g(sqrt(p1 * p1 + p2 * p2), &g, &hh);
  const double m = sqrt(q1 * q1 + q2 * q2);
  out[i] = g * p1, out[(size_t)n + i] = g * p2, out[2 * (size_t)n + i] = m, out[3 * (size_t)n + i] = -m;
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_ev_destroy(pgx_ev_handle* h) { mx_destroy(h); }

#define EV_LAUNCH(kernel, grid, block, ...)                                                                    \
  do {                                                                                                         \
    if (h->p == 1)                                                                                             \
      hipLaunchKernelGGL(kernel<1>, grid, block, 0, h->st, __VA_ARGS__);                                       \
    else if (h->p == 2)                                                                                        \
      hipLaunchKernelGGL(kernel<2>, grid, block, 0, h->st, __VA_ARGS__);                                       \
    else                                                                                                       \
      hipLaunchKernelGGL(kernel<3>, grid, block, 0, h->st, __VA_ARGS__);                                       \
  } while (0)

void pgx_ev_handle::residual_dev(const double* xin, double* Fout) {
  pgx_ev_handle* h = this;
  MxTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  EV_LAUNCH(k_ev_residual, dim3((h->nc + EV_WPB - 1) / EV_WPB), dim3(64 * EV_WPB), h->nc, h->Nx, h->Lx, h->n, h->nq, h->tab, xin, h->xk,
            h->isbc, h->gv, h->alpha, h->A, h->C, h->area, h->stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
  hipLaunchKernelGGL(k_ev_resid_bc, dim3((h->n + 255) / 256), dim3(256), 0, h->st, h->n, h->isbc, xin, h->gv, Fout);
}
void pgx_ev_handle::jacobian_dev(const double* xin) {
  pgx_ev_handle* h = this;
  MxTimer t(h, 1);
  if (h->alpha_J != h->alpha) {  // the iterate-independent part changes only with alpha
    hipLaunchKernelGGL(k_ev_recombine, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->st, h->nnz, h->nnz / 12, h->kind, h->src,
                       h->Sc, h->alpha, h->Jc);
    h->alpha_J = h->alpha;
  }
  hipMemcpyAsync(h->Jv, h->Jc, sizeof(double) * h->nnz, hipMemcpyDeviceToDevice, h->st);
  EV_LAUNCH(k_ev_jac, dim3((h->nc + EV_WPB - 1) / EV_WPB), dim3(64 * EV_WPB), h->nc, h->Nx, h->Lx, h->n, h->nq, h->tab, xin, h->alpha, h->A,
            h->C, h->area, h->stash);
  pgx_scatter_run(h->st, h->sc_jac, h->stash, 1.0, 1, h->Jv);
  pgx_scatter_run(h->st, h->sc_jac_t, h->stash, 1.0, 1, h->Jv);
  h->jac_valid = true;
}

// column blocks of row block fr, ascending: position of block (fr, fc) in a row, or -1 for the structurally zero ones
static const int8_t EV_BPOS[4][4] = {{0, 1, 2, -1}, {0, 1, -1, 2}, {0, -1, 1, 2}, {-1, 0, 1, 2}};

static int ev_create_impl(pgx_ev_handle* h, const pgx_ev_problem* pr) {
  const int p = pr->degree, P1 = p + 1, nb = P1 * P1, nq = pr->nq;
  const int Nx = pr->nx, Ny = pr->ny;
  const int64_t Lx = (int64_t)p * Nx + 1, Ly = (int64_t)p * Ny + 1, n64 = Lx * Ly, nc64 = (int64_t)Nx * Ny;
  if (4 * n64 > 0x7fffffff || 6 * nb * nb * nc64 > 0x7fffffff) {
    h->err = "mesh exceeds int32 indices";
    return PGX_EINVAL;
  }
  const int n = (int)n64, nc = (int)nc64;
  const int64_t ntot = 4 * n64;
  h->Nx = Nx, h->Ny = Ny, h->p = p, h->nq = nq, h->Lx = (int)Lx, h->n = n, h->nc = nc, h->ntot = ntot;
  h->A = pr->A, h->C = pr->C;
  const double hx = (pr->x1 - pr->x0) / Nx, hy = (pr->y1 - pr->y0) / Ny;
  h->area = hx * hy;
  // 1-D Lagrange basis on the nodes i / p from the linear factors (p t - a) / (i - a) (lagrange._lagrange_1d), M_e and K_e by the rule
  EvTab T;
  memset(&T, 0, sizeof T);
  double dB[EV_MAXQ * 4] = {0};
  for (int q = 0; q < nq; ++q) {
    T.w[q] = pr->qwts[q];
    for (int i = 0; i < P1; ++i) {
      double val = 1.0, der = 0.0;
      for (int a = 0; a < P1; ++a) {
        if (a == i) continue;
        const double fac = (p * pr->qpts[q] - a) / (i - a);
        der = der * fac + val * ((double)p / (i - a));
        val *= fac;
      }
      T.B[q * 4 + i] = val, dB[q * 4 + i] = der;
    }
  }
  for (int a = 0; a < nb; ++a)
    for (int b = 0; b < nb; ++b) {
      const int ay = a / P1, ax = a % P1, by = b / P1, bx = b % P1;
      double m = 0.0, k = 0.0;
      for (int qy = 0; qy < nq; ++qy)
        for (int qx = 0; qx < nq; ++qx) {
          const double wq = T.w[qy] * T.w[qx] * h->area;
          const double Na = T.B[qy * 4 + ay] * T.B[qx * 4 + ax], Nb = T.B[qy * 4 + by] * T.B[qx * 4 + bx];
          const double gxa = T.B[qy * 4 + ay] * dB[qx * 4 + ax] / hx, gxb = T.B[qy * 4 + by] * dB[qx * 4 + bx] / hx;
          const double gya = dB[qy * 4 + ay] * T.B[qx * 4 + ax] / hy, gyb = dB[qy * 4 + by] * T.B[qx * 4 + bx] / hy;
          m += wq * Na * Nb;
          k += wq * (gxa * gxb + gya * gyb);
        }
      T.Me[a * 16 + b] = m, T.Ke[a * 16 + b] = k;
    }
  for (int a = 0; a < nb; ++a)  // exactly symmetric element matrices: both triangles from the same sum
    for (int b = 0; b < a; ++b) T.Me[a * 16 + b] = T.Me[b * 16 + a], T.Ke[a * 16 + b] = T.Ke[b * 16 + a];
  std::vector<uint8_t> isbc(n, 0);
  std::vector<double> gv(2 * (size_t)n, 0.0);
  for (int k = 0; k < pr->n_bc; ++k) {
    const int32_t d = pr->bc_dofs[k];
    if (d < 0 || d >= n) {
      h->err = "bc dof out of range";
      return PGX_EINVAL;
    }
    if (!std::isfinite(pr->g1[k]) || !std::isfinite(pr->g2[k])) {
      h->err = "Dirichlet values must be finite";
      return PGX_EINVAL;
    }
    isbc[d] = 1, gv[d] = pr->g1[k], gv[(size_t)n + d] = pr->g2[k];
  }
  auto cdof = [&](int c, int a) -> int32_t {
    const int cy = c / Nx, cx = c % Nx, iy = a / P1, ix = a % P1;
    return (int32_t)((p * cy + iy) * Lx + p * cx + ix);
  };
  // scalar Q_p pattern: lattice point (gx, gy) meets the points of the cells it lies in, a rectangle of the lattice
  auto span = [&](int g, int N, int* lo, int* hi) {  // lattice range of the cells containing lattice coordinate g
    const int c1 = std::min(g / p, N - 1), c0 = (g % p == 0 && g > 0) ? std::max(g / p - 1, 0) : c1;
    *lo = c0 * p, *hi = c1 * p + p;
  };
  // the row lengths are a product of a count per lattice column and one per lattice row: the total in 64 bits, BEFORE any int32 prefix sum
  int64_t nnz_s = 0;
  {
    int64_t sx = 0, sy = 0;
    int lo, hi;
    for (int gx = 0; gx < (int)Lx; ++gx) span(gx, Nx, &lo, &hi), sx += hi - lo + 1;
    for (int gy = 0; gy < (int)Ly; ++gy) span(gy, Ny, &lo, &hi), sy += hi - lo + 1;
    nnz_s = sx * sy;  // <= (2p + 1)^2 Lx Ly with 4 Lx Ly < 2^31 (checked above)
  }
  if (12 * nnz_s > 0x7fffffff) {
    h->err = "mixed matrix exceeds int32 nnz";
    return PGX_EINVAL;
  }
  std::vector<int32_t> sptr(n + 1, 0);
  for (int v = 0; v < n; ++v) {
    int x0, x1, y0, y1;
    span(v % (int)Lx, Nx, &x0, &x1);
    span(v / (int)Lx, Ny, &y0, &y1);
    sptr[v + 1] = sptr[v] + (x1 - x0 + 1) * (y1 - y0 + 1);
  }
  if (sptr[n] != nnz_s) {
    h->err = "internal: scalar pattern count mismatch";
    return PGX_EINVAL;
  }
  // column j of row v sits at sptr[v] + (jy - y0) * (x1 - x0 + 1) + (jx - x0): ascending in j
  auto sfind = [&](int32_t v, int32_t j) -> int32_t {
    int x0, x1, y0, y1;
    span(v % (int)Lx, Nx, &x0, &x1);
    span(v / (int)Lx, Ny, &y0, &y1);
    return sptr[v] + (j / (int)Lx - y0) * (x1 - x0 + 1) + (j % (int)Lx - x0);
  };
  const int64_t tot = 12 * nnz_s;
  h->nnz = tot;
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  col.resize(tot);
  std::vector<uint8_t> kind(tot);
  std::vector<int32_t> src(tot);
  for (int fr = 0; fr < 4; ++fr)
    for (int v = 0; v < n; ++v) rowptr[(int64_t)fr * n + v + 1] = 3 * (sptr[v + 1] - sptr[v]);
  for (int64_t r = 0; r < ntot; ++r) rowptr[r + 1] += rowptr[r];
  mx_par_for(n, [&](int64_t v0, int64_t v1) {
    for (int64_t v = v0; v < v1; ++v) {
      int x0, x1, y0, y1;
      span((int)(v % Lx), Nx, &x0, &x1);
      span((int)(v / Lx), Ny, &y0, &y1);
      const int len = sptr[v + 1] - sptr[v], wx = x1 - x0 + 1;
      for (int fr = 0; fr < 4; ++fr)
        for (int fc = 0; fc < 4; ++fc) {
          if (EV_BPOS[fr][fc] < 0) continue;
          for (int k = 0; k < len; ++k) {
            const int32_t j = (int32_t)((y0 + k / wx) * Lx + x0 + k % wx);
            const int64_t e = rowptr[(int64_t)fr * n + v] + (int64_t)EV_BPOS[fr][fc] * len + k;
            col[e] = fc * n + j;
            src[e] = sptr[v] + k;
            uint8_t t;
            if (fr < 2 && isbc[v])
              t = (fc == fr && j == v) ? 5 : 0;  // Dirichlet row: identity
            else if (fc < 2 && isbc[j])
              t = 0;  // Dirichlet column
            else if (fr < 2 && fc == fr)
              t = 1;
            else if (fc == (fr + 2) % 4)
              t = 2;
            else
              t = 0;
            kind[e] = t;
          }
        }
    }
  });
  auto find = [&](int fr, int32_t v, int fc, int32_t j) -> int32_t {
    return (int32_t)(rowptr[(int64_t)fr * n + v] + (int64_t)EV_BPOS[fr][fc] * (sptr[v + 1] - sptr[v]) + (sfind(v, j) - sptr[v]));
  };
  // scalar M and K on the pattern, once, on the host in a fixed order
  std::vector<double> Sc(2 * (size_t)nnz_s, 0.0);
  for (int c = 0; c < nc; ++c)
    for (int a = 0; a < nb; ++a)
      for (int b = 0; b < nb; ++b) {
        const int32_t s = sfind(cdof(c, a), cdof(c, b));
        Sc[s] += T.Me[a * 16 + b];
        Sc[(size_t)nnz_s + s] += T.Ke[a * 16 + b];
      }
  // destination tables, cell-major like the stashes; -1 drops a contribution (Dirichlet rows and columns)
  const int W = 6 * nb * nb;
  std::vector<int32_t> dj((size_t)nc * W), djt((size_t)nc * W, -1), dr((size_t)nc * 4 * nb);
  mx_par_for(nc, [&](int64_t c0, int64_t c1) {
    const int blk_r[6] = {0, 1, 2, 3, 0, 2}, blk_c[6] = {0, 1, 2, 3, 1, 3};
    for (int64_t c = c0; c < c1; ++c)
      for (int a = 0; a < nb; ++a) {
        const int32_t va = cdof((int)c, a);
        for (int f = 0; f < 4; ++f) dr[(size_t)c * 4 * nb + f * nb + a] = f * n + va;
        for (int b = 0; b < nb; ++b) {
          const int32_t vb = cdof((int)c, b);
          for (int k = 0; k < 6; ++k) {
            const bool drop = (blk_r[k] < 2 || blk_c[k] < 2) && (isbc[va] || isbc[vb]);  // blocks of q only: both indices are q dofs
            const size_t o = (size_t)c * W + (size_t)k * nb * nb + a * nb + b;
            dj[o] = drop ? -1 : find(blk_r[k], va, blk_c[k], vb);
            if (k >= 4) djt[o] = drop ? -1 : find(blk_c[k], va, blk_r[k], vb);  // the transposed block takes the same (symmetric) values
          }
        }
      }
  });
  std::vector<int32_t> nod(ntot);
  std::vector<double> xy(2 * (size_t)n);
  for (int v = 0; v < n; ++v) {
    for (int f = 0; f < 4; ++f) nod[(size_t)f * n + v] = v;
    xy[2 * (size_t)v] = pr->x0 + (v % Lx) * hx / p, xy[2 * (size_t)v + 1] = pr->y0 + (v / Lx) * hy / p;
  }
  MXHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, n, nod.data(), 2, xy.data());
  if (rc) return rc;
  // the Jacobian with its Dirichlet rows AND columns replaced is symmetric (indefinite) as assembled: L D L^T in LU clothing (pgx_nd.h)
  pgx_nd_set_symmetric(h->lu, 1);
  MXALLOC(h->tab, 1);
  MXALLOC(h->isbc, n);
  MXALLOC(h->gv, 2 * (size_t)n);
  MXALLOC(h->stash, (size_t)nc * W);
  MXALLOC(h->Sc, 2 * nnz_s);
  MXALLOC(h->rowptr, ntot + 1);
  MXALLOC(h->col, tot);
  MXALLOC(h->kind, tot);
  MXALLOC(h->src, tot);
  MXALLOC(h->Jc, tot);
  MXALLOC(h->Jv, tot);
  MXALLOC(h->d_nodes, 4 * (size_t)n);
  if ((rc = mx_alloc_state(h))) return rc;
  MXHIP(hipMemcpy(h->tab, &T, sizeof T, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->isbc, isbc.data(), n, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->gv, gv.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->Sc, Sc.data(), sizeof(double) * 2 * nnz_s, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->rowptr, rowptr.data(), sizeof(int32_t) * (ntot + 1), hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->col, col.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->src, src.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->Jv, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  std::string e1 = pgx_scatter_build(dr.data(), (int64_t)nc * 4 * nb, ntot, h->allocs, &h->sc_res);
  if (e1.empty()) e1 = pgx_scatter_build(dj.data(), (int64_t)nc * W, tot, h->allocs, &h->sc_jac);
  if (e1.empty()) e1 = pgx_scatter_build(djt.data(), (int64_t)nc * W, tot, h->allocs, &h->sc_jac_t);
  if (!e1.empty()) {
    h->err = e1;
    return PGX_ENOMEM;
  }
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}

extern "C" int pgx_ev_create(const pgx_ev_problem* p, int device, pgx_ev_handle** out) {
  if (!p || !out || p->nx < 1 || p->ny < 1 || p->degree < 1 || p->degree > 3 || p->nq < 1 || p->nq > EV_MAXQ || !p->qpts || !p->qwts ||
      p->n_bc < 0 || (p->n_bc > 0 && (!p->bc_dofs || !p->g1 || !p->g2)) || !std::isfinite(p->A) || !std::isfinite(p->C) ||
      !(p->x1 > p->x0) || !(p->y1 > p->y0) || !std::isfinite(p->x1 - p->x0) || !std::isfinite(p->y1 - p->y0)) {
    g_ev_error = "pgx_ev_create: bad arguments (degree 1..3, 1-D rule of 1..11 points, a non-degenerate box)";
    return PGX_EINVAL;
  }
  return mx_create("pgx_ev_create", g_ev_error, device, out, [&](pgx_ev_handle* h) { return ev_create_impl(h, p); });
}

extern "C" int pgx_ev_num_dofs(const pgx_ev_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_ev_set_state(pgx_ev_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_ev_get_state(pgx_ev_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_ev_set_prev(pgx_ev_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_ev_get_prev(pgx_ev_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_ev_advance_prev(pgx_ev_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_ev_set_alpha(pgx_ev_handle* h, double a) { return mx_set_alpha(h, a); }
extern "C" int pgx_ev_residual(pgx_ev_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_ev_jacobian_fill(pgx_ev_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_ev_csr_export(pgx_ev_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_ev_spmv(pgx_ev_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
// linesearch 2: l2 (the script's), 1 / 3: bt of order 2 / 3, every other value: plain Newton
extern "C" int pgx_ev_newton_solve(pgx_ev_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its) {
  return mx_newton(h, opts, reason, its, lin_its, true);
}
extern "C" int pgx_ev_profile(pgx_ev_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

extern "C" int pgx_ev_state_from_prev(pgx_ev_handle* h) {
  MXNEED(h);
  MXHIP(hipMemcpyAsync(h->x, h->xk, sizeof(double) * h->ntot, hipMemcpyDeviceToDevice, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_ev_l2_increment_q(pgx_ev_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  EV_LAUNCH(k_ev_l2, dim3(MX_RED), dim3(256), h->nc, h->Nx, h->Lx, h->n, h->tab, h->x, h->xk, h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_ev_eval_nodes(pgx_ev_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_ev_nodes, dim3((h->n + 255) / 256), dim3(256), 0, h->st, h->n, h->x, h->d_nodes);
  MXHIP(hipMemcpyAsync(out, h->d_nodes, sizeof(double) * 4 * h->n, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  MXHIP(hipGetLastError());
  return PGX_OK;
}
extern "C" int pgx_ev_lu_stats(const pgx_ev_handle* h, pgx_nd_stats* st) { return h ? pgx_nd_get_stats(h->lu, st) : PGX_EINVAL; }
extern "C" int pgx_ev_lu_is_symmetric(const pgx_ev_handle* h) { return h ? pgx_nd_is_symmetric(h->lu) : 0; }
