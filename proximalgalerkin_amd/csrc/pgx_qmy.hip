// pgx_qmy.hip - the comparison solvers of example 05 (thermoforming QVI, Moreau-Yosida penalisation: u, T in P1) behind the C ABI
// of include/pgx_qmy.h.  Reference: examples/05_obstacle_type_qvi/solver_comparison/thermoforming_moreau_yosida.jl ("MY": :24-44
// spaces and data, :46-74 g and plus, :77-88 residual and Jacobian, :92-98 H1 matrix and functionals) and
// thermoforming_fixed_point.jl ("FP": :62-65 the two single-field operators).  x = [u | T]; the 2 x 2 block Jacobian lives in one
// mixed CSR array (4 blocks on the scalar P1 pattern).  All four blocks depend on the state: K and K + M are assembled once, every
// Newton step adds the four weighted mass matrices M_chi, M_{chi phi}, M_{g'}, M_{g' phi} of one pass over the cells.
#include <cstring>

#include "../../include/pgx_qmy.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"
#include "pgx_tri.h"

#define QM_MAXQ 36
using QmQuad = TriQuad<QM_MAXQ>;

static thread_local std::string g_qmy_error;

struct pgx_qmy_handle : MixedBase {
  int nv = 0, nc = 0;
  QmQuad Q{};
  double f = 25.0, knee = 0.01, gamma = 1.0;
  int active = 3;  // bit 0: u, bit 1: T
  double* coords = nullptr;
  int32_t* cells = nullptr;
  double *Phi0 = nullptr, *phi = nullptr;  // nodal data
  // deterministic assembly (pgx_scatter.h): element kernels park [slot * nc + cell]; one thread per destination sums
  PgxScatter sc_res;     // residual: 6 slots per cell -> dofs
  PgxScatter sc_blk[4];  // weighted mass blocks (u,u), (u,T), (T,u), (T,T): 9 slots per cell each -> CSR positions
  double* stash = nullptr;      // [36 * nc]
  double* partials2 = nullptr;  // [2 * MX_RED]: energy and penalty
  uint8_t *mask = nullptr, *kind = nullptr;
  double* Jc = nullptr;
  pgx_qmy_handle() : MixedBase("pgx_qmy") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

extern "C" const char* pgx_qmy_last_error(const pgx_qmy_handle* h) { return h ? h->err.c_str() : g_qmy_error.c_str(); }

// R_u = (grad u, grad v) - (f, v) + gamma (max(0, d), v);  R_T = (grad T, grad R) + (T, R) - (g(s), R)   (MY:77-81)
__global__ __launch_bounds__(128) void k_qm_residual(int nc, int nv, const int32_t* __restrict__ cells,
                                                     const double* __restrict__ coords, const uint8_t* __restrict__ mask,
                                                     const double* __restrict__ Phi0, const double* __restrict__ phi,
                                                     const double* __restrict__ x, double gamma, double f, double knee, QmQuad Q,
                                                     double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)c;
  const TriGeom g = tri_geom(coords, cv);
  double u[3], T[3], P[3], p[3];
  for (int a = 0; a < 3; ++a) {
    const int v = cv[a];
    u[a] = mask[v] ? 0.0 : x[v];
    T[a] = x[nv + v];
    P[a] = Phi0[v];
    p[a] = phi[v];
  }
  const double area = 0.5 * g.adet;
  double gu[2] = {0, 0}, gT[2] = {0, 0};
  for (int a = 0; a < 3; ++a)
    for (int d = 0; d < 2; ++d) gu[d] += u[a] * g.G[a][d], gT[d] += T[a] * g.G[a][d];
  double Ru[3], RT[3];
  for (int a = 0; a < 3; ++a) {
    Ru[a] = area * (gu[0] * g.G[a][0] + gu[1] * g.G[a][1]);
    RT[a] = area * (gT[0] * g.G[a][0] + gT[1] * g.G[a][1]);
  }
  for (int q = 0; q < Q.nq; ++q) {
    const double N0 = Q.N[q][0], N1 = Q.N[q][1], N2 = Q.N[q][2];
    const double wd = Q.w[q] * g.adet;
    const double uq = u[0] * N0 + u[1] * N1 + u[2] * N2, Tq = T[0] * N0 + T[1] * N1 + T[2] * N2;
    const double Pq = P[0] * N0 + P[1] * N1 + P[2] * N2, pq = p[0] * N0 + p[1] * N1 + p[2] * N2;
    const double s = Pq + pq * Tq - uq, d = uq - (Pq + pq * Tq);
    const double gv = s <= 0.0 ? 1.0 : s < knee ? 1.0 - s / knee : 0.0;  // MY:47-55
    const double cu = wd * (gamma * fmax(0.0, d) - f), cT = wd * (Tq - gv);
    Ru[0] += cu * N0, Ru[1] += cu * N1, Ru[2] += cu * N2;
    RT[0] += cT * N0, RT[1] += cT * N1, RT[2] += cT * N2;
  }
  for (int a = 0; a < 3; ++a) {  // parked slot-major; pgx_scatter sums per dof in a fixed order
    stash[(size_t)a * nc + c] = Ru[a];
    stash[(size_t)(3 + a) * nc + c] = RT[a];
  }
}
// Dirichlet rows F = x; rows of a frozen field: zero residual
__global__ void k_qm_resid_fix(int nv, int active, const uint8_t* __restrict__ mask, const double* __restrict__ x,
                               double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  if (!(active & 1))
    F[i] = 0.0;
  else if (mask[i])
    F[i] = x[i];
  if (!(active & 2)) F[nv + i] = 0.0;
}

// constant blocks, once: K for (u,u) and K + M for (T,T), parked at stash[(blk * 9 + a * 3 + b) * nc + cell]
__global__ __launch_bounds__(128) void k_qm_const(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                  QmQuad Q, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)c;
  const TriGeom g = tri_geom(coords, cv);
  double Ke[3][3], Me[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      Ke[a][b] = 0.5 * g.adet * (g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1]);
      Me[a][b] = 0.0;
    }
  for (int q = 0; q < Q.nq; ++q) {
    const double N[3] = {Q.N[q][0], Q.N[q][1], Q.N[q][2]};
    const double wd = Q.w[q] * g.adet;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Me[a][b] += wd * N[a] * N[b];
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      stash[(size_t)(a * 3 + b) * nc + c] = Ke[a][b];
      stash[(size_t)(9 + a * 3 + b) * nc + c] = Ke[a][b] + Me[a][b];
    }
}

// kind of a CSR entry: bit 0 row field, bit 1 column field, bit 2 diagonal of the whole matrix, bit 3 row or column is a Dirichlet
// dof of u.  Active rows and columns take the constant part (K, K + M, 0 in the off-diagonal blocks); a frozen field's rows and
// the Dirichlet rows are identity rows, and their columns are zero.
__global__ void k_qm_jac_init(int64_t nnz, int active, const uint8_t* __restrict__ kind, const double* __restrict__ Jc,
                              double* __restrict__ Jv) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int t = kind[k];
  const bool on = ((active >> (t & 1)) & 1) && ((active >> ((t >> 1) & 1)) & 1) && !(t & 8);
  Jv[k] = on ? Jc[k] : (t & 4) ? 1.0 : 0.0;
}

// The four weighted mass matrices of the generalised Jacobian (MY:84-88), chi = [d > 0] (MY:68-74), g' = -1/q on 0 < s < q
// (MY:56-64): M_chi, M_{chi phi}, M_{g'}, M_{g' phi}.  Each is symmetric in (a, b): 6 accumulators, 9 parked entries.  The
// factors gamma, -gamma, 1, -1 are applied by the scatter.
__global__ __launch_bounds__(128) void k_qm_jac(int nc, int nv, const int32_t* __restrict__ cells,
                                                const double* __restrict__ coords, const uint8_t* __restrict__ mask,
                                                const double* __restrict__ Phi0, const double* __restrict__ phi,
                                                const double* __restrict__ x, double knee, QmQuad Q, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)c;
  double adet;
  {
    const double x0 = coords[2 * (size_t)cv[0]], y0 = coords[2 * (size_t)cv[0] + 1];
    const double j00 = coords[2 * (size_t)cv[1]] - x0, j10 = coords[2 * (size_t)cv[1] + 1] - y0;
    const double j01 = coords[2 * (size_t)cv[2]] - x0, j11 = coords[2 * (size_t)cv[2] + 1] - y0;
    adet = fabs(j00 * j11 - j01 * j10);
  }
  double u[3], T[3], P[3], p[3];
  for (int a = 0; a < 3; ++a) {
    const int v = cv[a];
    u[a] = mask[v] ? 0.0 : x[v];
    T[a] = x[nv + v];
    P[a] = Phi0[v];
    p[a] = phi[v];
  }
  double A[4][6];  // per block: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  for (int k = 0; k < 4; ++k)
    for (int e = 0; e < 6; ++e) A[k][e] = 0.0;
  const double dg = -1.0 / knee;
  for (int q = 0; q < Q.nq; ++q) {
    const double N0 = Q.N[q][0], N1 = Q.N[q][1], N2 = Q.N[q][2];
    const double wd = Q.w[q] * adet;
    const double uq = u[0] * N0 + u[1] * N1 + u[2] * N2, Tq = T[0] * N0 + T[1] * N1 + T[2] * N2;
    const double Pq = P[0] * N0 + P[1] * N1 + P[2] * N2, pq = p[0] * N0 + p[1] * N1 + p[2] * N2;
    const double s = Pq + pq * Tq - uq, d = uq - (Pq + pq * Tq);
    const double w0 = d > 0.0 ? wd : 0.0, w2 = (s > 0.0 && s < knee) ? wd * dg : 0.0;
    const double w1 = w0 * pq, w3 = w2 * pq;
    const double nn[6] = {N0 * N0, N0 * N1, N0 * N2, N1 * N1, N1 * N2, N2 * N2};
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      A[0][e] += w0 * nn[e];
      A[1][e] += w1 * nn[e];
      A[2][e] += w2 * nn[e];
      A[3][e] += w3 * nn[e];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double* B = A[k];
    double* o = stash + (size_t)(k * 9) * nc + c;
    o[0] = B[0], o[(size_t)1 * nc] = B[1], o[(size_t)2 * nc] = B[2];
    o[(size_t)3 * nc] = B[1], o[(size_t)4 * nc] = B[3], o[(size_t)5 * nc] = B[4];
    o[(size_t)6 * nc] = B[2], o[(size_t)7 * nc] = B[4], o[(size_t)8 * nc] = B[5];
  }
}

// energy(u) = int 1/2 |grad u|^2 - f u and penalty(u, T) = int gamma/2 max(0, d)^2 (MY:97-98): per-block partials, energy in
// partials[0 .. MX_RED), penalty in partials[MX_RED .. 2 MX_RED)
__global__ __launch_bounds__(256) void k_qm_functionals(int nc, int nv, const int32_t* __restrict__ cells,
                                                        const double* __restrict__ coords, const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ Phi0, const double* __restrict__ phi,
                                                        const double* __restrict__ x, double gamma, double f, QmQuad Q,
                                                        double* __restrict__ partials) {
  __shared__ double sh[2][256];
  double se = 0.0, sp = 0.0;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += MX_RED * 256) {
    const int32_t* cv = cells + 3 * (size_t)c;
    const TriGeom g = tri_geom(coords, cv);
    double u[3], T[3], P[3], p[3], gu[2] = {0, 0};
    for (int a = 0; a < 3; ++a) {
      const int v = cv[a];
      u[a] = mask[v] ? 0.0 : x[v];
      T[a] = x[nv + v];
      P[a] = Phi0[v];
      p[a] = phi[v];
      gu[0] += u[a] * g.G[a][0];
      gu[1] += u[a] * g.G[a][1];
    }
    se += 0.25 * g.adet * (gu[0] * gu[0] + gu[1] * gu[1]);
    for (int q = 0; q < Q.nq; ++q) {
      const double N0 = Q.N[q][0], N1 = Q.N[q][1], N2 = Q.N[q][2];
      const double wd = Q.w[q] * g.adet;
      const double uq = u[0] * N0 + u[1] * N1 + u[2] * N2, Tq = T[0] * N0 + T[1] * N1 + T[2] * N2;
      const double Pq = P[0] * N0 + P[1] * N1 + P[2] * N2, pq = p[0] * N0 + p[1] * N1 + p[2] * N2;
      const double d = fmax(0.0, uq - (Pq + pq * Tq));
      se -= wd * f * uq;
      sp += wd * (0.5 * gamma) * d * d;
    }
  }
  sh[0][threadIdx.x] = se, sh[1][threadIdx.x] = sp;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[0][threadIdx.x] += sh[0][threadIdx.x + o], sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0][0], partials[MX_RED + blockIdx.x] = sh[1][0];
}

// d' (K + M) d, d = u - u_prev on the free dofs of u (MY:92-94,144-145): per-block partials
__global__ __launch_bounds__(256) void k_qm_cauchy(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                   const uint8_t* __restrict__ mask, const double* __restrict__ x,
                                                   const double* __restrict__ xk, QmQuad Q, double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += MX_RED * 256) {
    const int32_t* cv = cells + 3 * (size_t)c;
    const TriGeom g = tri_geom(coords, cv);
    double d[3], gd[2] = {0, 0};
    for (int a = 0; a < 3; ++a) {
      d[a] = mask[cv[a]] ? 0.0 : x[cv[a]] - xk[cv[a]];
      gd[0] += d[a] * g.G[a][0];
      gd[1] += d[a] * g.G[a][1];
    }
    s += 0.5 * g.adet * (gd[0] * gd[0] + gd[1] * gd[1]);
    for (int q = 0; q < Q.nq; ++q) {
      const double v = d[0] * Q.N[q][0] + d[1] * Q.N[q][1] + d[2] * Q.N[q][2];
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
extern "C" void pgx_qmy_destroy(pgx_qmy_handle* h) { mx_destroy(h); }

void pgx_qmy_handle::residual_dev(const double* xin, double* Fout) {
  pgx_qmy_handle* h = this;
  MxTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  hipLaunchKernelGGL(k_qm_residual, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->mask,
                     h->Phi0, h->phi, xin, h->gamma, h->f, h->knee, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
  hipLaunchKernelGGL(k_qm_resid_fix, dim3((h->nv + 255) / 256), dim3(256), 0, h->st, h->nv, h->active, h->mask, xin, Fout);
}
void pgx_qmy_handle::jacobian_dev(const double* xin) {
  pgx_qmy_handle* h = this;
  MxTimer t(h, 1);
  hipLaunchKernelGGL(k_qm_jac_init, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->st, h->nnz, h->active, h->kind,
                     h->Jc, h->Jv);
  hipLaunchKernelGGL(k_qm_jac, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->mask,
                     h->Phi0, h->phi, xin, h->knee, h->Q, h->stash);
  const bool au = h->active & 1, aT = h->active & 2;
  if (au) pgx_scatter_run(h->st, h->sc_blk[0], h->stash, h->gamma, 1, h->Jv);                                   // + gamma M_chi
  if (au && aT) pgx_scatter_run(h->st, h->sc_blk[1], h->stash + 9 * (size_t)h->nc, -h->gamma, 1, h->Jv);        // - gamma M_{chi phi}
  if (au && aT) pgx_scatter_run(h->st, h->sc_blk[2], h->stash + 18 * (size_t)h->nc, 1.0, 1, h->Jv);             // + M_{g'}
  if (aT) pgx_scatter_run(h->st, h->sc_blk[3], h->stash + 27 * (size_t)h->nc, -1.0, 1, h->Jv);                  // - M_{g' phi}
  h->jac_valid = true;
}

static int qmy_create_impl(pgx_qmy_handle* h, const pgx_mesh* m, const pgx_qmy_problem* p) {
  const int nv = m->n_vertices, nc = m->n_cells;
  const int64_t ntot = 2 * (int64_t)nv;
  h->nv = nv, h->nc = nc, h->ntot = ntot;
  h->f = p->f, h->knee = p->q;
  h->Q.fill(p->qpts, p->qwts, p->nq);
  if (const char* e = check_cells(m->cells, 3, nc, nv)) {
    h->err = e;
    return PGX_EINVAL;
  }
  std::vector<uint8_t> hmask(nv, 0);
  for (int k = 0; k < p->n_bc; ++k) {
    if (p->bc_dofs[k] < 0 || p->bc_dofs[k] >= nv) {
      h->err = "bc dof out of range";
      return PGX_EINVAL;
    }
    hmask[p->bc_dofs[k]] = 1;
  }
  // scalar P1 pattern (vertex adjacency incl. self), then 2 x 2 blocks
  std::vector<int32_t> sptr, scol;
  p1_adjacency(nv, nc, m->cells, true, sptr, scol);  // true: a vertex no cell touches keeps its diagonal, its rows are not empty
  const int64_t nnz_s = sptr[nv];
  if (4 * nnz_s > 0x7fffffff || 36 * (int64_t)nc > 0x7fffffff) {
    h->err = "mixed matrix exceeds int32 indices";
    return PGX_EINVAL;
  }
  const int64_t tot = 4 * nnz_s;
  h->nnz = tot;
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  col.resize(tot);
  std::vector<uint8_t> kind(tot);
  for (int fr = 0; fr < 2; ++fr)
    for (int v = 0; v < nv; ++v) rowptr[(int64_t)fr * nv + v + 1] = 2 * (sptr[v + 1] - sptr[v]);
  for (int64_t r = 0; r < ntot; ++r) rowptr[r + 1] += rowptr[r];
  for (int fr = 0; fr < 2; ++fr)
    for (int v = 0; v < nv; ++v) {
      const int64_t r = (int64_t)fr * nv + v;
      const int len = sptr[v + 1] - sptr[v];
      for (int fc = 0; fc < 2; ++fc)
        for (int k = 0; k < len; ++k) {
          const int32_t j = scol[sptr[v] + k];
          const int64_t e = rowptr[r] + (int64_t)fc * len + k;
          col[e] = fc * nv + j;
          const bool bc = (fr == 0 && hmask[v]) || (fc == 0 && hmask[j]);
          kind[e] = (uint8_t)(fr | (fc << 1) | ((fr == fc && v == j) ? 4 : 0) | (bc ? 8 : 0));
        }
    }
  auto find = [&](int fr, int32_t v, int fc, int32_t j) -> int32_t {
    if ((fr == 0 && hmask[v]) || (fc == 0 && hmask[j])) return -1;  // Dirichlet row or column: dropped by the scatter
    const int len = sptr[v + 1] - sptr[v];
    const int32_t* b = scol.data() + sptr[v];
    const int k = (int)(std::lower_bound(b, b + len, j) - b);
    return (int32_t)(rowptr[(int64_t)fr * nv + v] + (int64_t)fc * len + k);
  };
  // destination tables, slot-major like the stashes: table[slot * nc + cell]
  std::vector<int32_t> d6((size_t)nc * 6), d18((size_t)nc * 18);
  std::vector<int32_t> d9[4];
  for (auto& d : d9) d.resize((size_t)nc * 9);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    for (int64_t c = a0; c < b0; ++c) {
      const int32_t* cv = m->cells + 3 * (size_t)c;
      for (int a = 0; a < 3; ++a) {
        d6[(size_t)a * nc + (size_t)c] = hmask[cv[a]] ? -1 : cv[a];
        d6[(size_t)(3 + a) * nc + (size_t)c] = nv + cv[a];
        for (int b = 0; b < 3; ++b) {
          for (int k = 0; k < 4; ++k) d9[k][(size_t)(a * 3 + b) * nc + (size_t)c] = find(k >> 1, cv[a], k & 1, cv[b]);
          d18[(size_t)(a * 3 + b) * nc + (size_t)c] = find(0, cv[a], 0, cv[b]);
          d18[(size_t)(9 + a * 3 + b) * nc + (size_t)c] = find(1, cv[a], 1, cv[b]);
        }
      }
    }
  });
  std::vector<int32_t> nod(ntot);
  for (int v = 0; v < nv; ++v) nod[v] = nod[(size_t)nv + v] = v;
  MXHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, nv, nod.data(), 2, m->coords);  // not symmetric: lu_flip_from stays -1
  if (rc) return rc;
  MXALLOC(h->coords, 2 * (size_t)nv);
  MXALLOC(h->cells, 3 * (size_t)nc);
  MXALLOC(h->Phi0, nv);
  MXALLOC(h->phi, nv);
  MXALLOC(h->mask, nv);
  MXALLOC(h->stash, 36 * (size_t)nc);
  MXALLOC(h->partials2, 2 * MX_RED);
  MXALLOC(h->kind, tot);
  MXALLOC(h->Jc, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  MXHIP(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->cells, m->cells, sizeof(int32_t) * 3 * (size_t)nc, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->Phi0, p->Phi0, sizeof(double) * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->phi, p->phi, sizeof(double) * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->mask, hmask.data(), nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  {
    std::string e1 = pgx_scatter_build(d6.data(), (int64_t)6 * nc, ntot, h->allocs, &h->sc_res);
    for (int k = 0; k < 4 && e1.empty(); ++k) e1 = pgx_scatter_build(d9[k].data(), (int64_t)9 * nc, tot, h->allocs, &h->sc_blk[k]);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  // constant blocks, once: the stash is the per-step one (18 of its 36 slots)
  return mx_scatter_once(h, d18.data(), 18, nc, tot, h->stash, [&](double* stash) {
    hipLaunchKernelGGL(k_qm_const, dim3((nc + 127) / 128), dim3(128), 0, h->st, nc, h->cells, h->coords, h->Q, stash);
  }, h->Jc, 0);
}

extern "C" int pgx_qmy_create(const pgx_mesh* m, const pgx_qmy_problem* p, int device, pgx_qmy_handle** out) {
  if (!m || !p || !out || !m->coords || !m->cells || m->n_vertices <= 0 || m->n_cells <= 0 || !p->qpts || !p->qwts || !p->Phi0 ||
      !p->phi || p->nq <= 0 || p->nq > QM_MAXQ || p->n_bc < 0 || (p->n_bc > 0 && !p->bc_dofs) || !(p->q > 0.0)) {
    g_qmy_error = "pgx_qmy_create: bad arguments";
    return PGX_EINVAL;
  }
  return mx_create("pgx_qmy_create", g_qmy_error, device, out, [&](pgx_qmy_handle* h) { return qmy_create_impl(h, m, p); });
}

extern "C" int pgx_qmy_num_dofs(const pgx_qmy_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_qmy_set_state(pgx_qmy_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_qmy_get_state(pgx_qmy_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_qmy_set_prev(pgx_qmy_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_qmy_get_prev(pgx_qmy_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_qmy_advance_prev(pgx_qmy_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_qmy_set_gamma(pgx_qmy_handle* h, double gamma) {
  MXNEED(h);
  if (!(gamma > 0.0) || !std::isfinite(gamma)) {
    h->err = "gamma must be positive and finite";
    return PGX_EINVAL;
  }
  h->gamma = gamma;
  h->jac_valid = false;
  return PGX_OK;
}
extern "C" int pgx_qmy_set_active(pgx_qmy_handle* h, int mask) {
  MXNEED(h);
  if (mask < 1 || mask > 3) {
    h->err = "active mask must be 1 (u), 2 (T) or 3 (both)";
    return PGX_EINVAL;
  }
  h->active = mask;
  h->jac_valid = false;
  return PGX_OK;
}
extern "C" int pgx_qmy_residual(pgx_qmy_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_qmy_residual_inf(pgx_qmy_handle* h, const double* x, double* finf) {
  if (!finf) return PGX_EINVAL;
  const int rc = mx_residual(h, x, nullptr, nullptr);
  return rc ? rc : mx_absmax(h, h->F, finf);
}
extern "C" int pgx_qmy_jacobian_fill(pgx_qmy_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_qmy_csr_export(pgx_qmy_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col,
                                  double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_qmy_spmv(pgx_qmy_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
extern "C" int pgx_qmy_newton_solve(pgx_qmy_handle* h, const pgx_qmy_newton_opts* o, int* reason, int* its, int* lin_its) {
  if (!h || !o) return PGX_EINVAL;
  return mx_newton_nls(h, o->ftol, o->xtol, o->max_it, o->c1, o->monitor, reason, its, lin_its);
}
extern "C" int pgx_qmy_functionals(pgx_qmy_handle* h, double* energy, double* penalty) {
  MXNEED(h);
  if (!energy || !penalty) return PGX_EINVAL;
  hipLaunchKernelGGL(k_qm_functionals, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->mask, h->Phi0,
                     h->phi, h->x, h->gamma, h->f, h->Q, h->partials2);
  const int rc = mx_partials_sum(h, h->partials2, energy);
  return rc ? rc : mx_partials_sum(h, h->partials2 + MX_RED, penalty);
}
extern "C" int pgx_qmy_cauchy(pgx_qmy_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_qm_cauchy, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->cells, h->coords, h->mask, h->x, h->xk, h->Q,
                     h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_qmy_lu_stats(const pgx_qmy_handle* h, pgx_nd_stats* st) { return h ? pgx_nd_get_stats(h->lu, st) : PGX_EINVAL; }
extern "C" int pgx_qmy_profile(pgx_qmy_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }
