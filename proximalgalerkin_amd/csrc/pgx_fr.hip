// pgx_fr.hip - example 03 (phase-field fracture under load stepping: u, c, psi in P1) behind the C ABI of include/pgx_fr.h.
// Reference: examples/03_fracture/fracture_dolfinx.py (:79-81 space, :117-130 residual, :132-138 the modified Jacobian,
// :141-160 Dirichlet data, :163-171 solver, :207-311 loop).  x = [u | c | psi]; the 3 x 3 block Jacobian lives in one mixed CSR
// array (9 blocks on the scalar P1 pattern, the structurally zero (u,psi) and (psi,u) included).  M and K are assembled once
// on the scalar pattern; the iterate-independent part Jc - reps M on (u,u), alpha (Gc / l M + Gc l K) + reps M on (c,c), M on
// (c,psi) and (psi,c), -reps M on (psi,psi), the identity on the Dirichlet rows - is recombined only when alpha changes.  Every
// Newton step copies Jc and adds the five iterate-dependent blocks (u,u), (u,c), (c,u), (c,c), (psi,psi).  Polynomial terms
// (degree <= 4) are integrated exactly in closed form, the terms containing psi with the degree-7 rule the caller passes.
//
// Dirichlet rows: R_d is quadratic in u, so imposing the boundary values inside the element evaluation would NOT give DOLFINx's
// F_raw(x) + J_reg(x)[:, bc] (g - x_bc); the lifting is done element-locally instead: the element Jacobian columns of the cell's
// bc vertices times (g - x_b) are added to the element residual.
#include <cstring>

#include "../../include/pgx_fr.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"
#include "pgx_tri.h"

#define FR_MAXQ 16
#define FR_MAXPTS 64
using FrQuad = TriQuad<FR_MAXQ>;
struct FrPar {
  double G, Gc, l, eps, reps;
};

static thread_local std::string g_fr_error;

struct pgx_fr_handle : MixedBase {
  int nv = 0, nc = 0;
  FrQuad Q{};
  FrPar P{};
  double T = 0.0;         // the load: u = sign * T on the Dirichlet vertices
  double alpha_J = -1.0;  // alpha the constant part Jc was recombined with (< 0: never)
  double* coords = nullptr;
  int32_t* cells = nullptr;
  int8_t* sign = nullptr;   // [nv] -1 topleft, +1 topright, 0 free
  double* zprev = nullptr;  // [3 nv] state of the last written load step
  // deterministic assembly (pgx_scatter.h): residual 9 slots per cell -> dofs; iterate-dependent blocks 45 slots per cell -> CSR
  PgxScatter sc_res, sc_jac;
  double* stash = nullptr;  // [45 nc]
  double* Sc = nullptr;     // [2 nnz_s] scalar M | K on the P1 pattern
  uint8_t* kind = nullptr;
  int32_t* src = nullptr;   // scalar-pattern index of every mixed entry
  double* Jc = nullptr;     // [nnz] iterate-independent part of the Jacobian at alpha_J
  double *d_pts = nullptr, *d_conf = nullptr;  // conforming_damage: [2 FR_MAXPTS], [nc * conf_cap]
  int conf_cap = 0;
  pgx_fr_handle() : MixedBase("pgx_fr") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

extern "C" const char* pgx_fr_last_error(const pgx_fr_handle* h) { return h ? h->err.c_str() : g_fr_error.c_str(); }

// logistic function and its derivative sigma (1 - sigma) from t = exp(-|p|) <= 1: finite for every finite p
__device__ inline void fr_sigma(double p, double* s, double* ds) {
  const double t = exp(-fabs(p)), r = 1.0 / (1.0 + t);
  *s = p >= 0.0 ? r : t * r;
  *ds = t * r * r;
}

// what the residual and the Jacobian share per cell: the degradation integrals of the current (u, c)
struct FrCell {
  double ga[3];   // grad u . grad phi_a
  double Ms[3];   // int (1 - c) phi_a
  double g2, Iw;  // |grad u|^2, int w(c)
};
__device__ inline FrCell fr_cell(const TriGeom& g, double area, const double u[3], const double c[3], double eps) {
  FrCell k;
  double gu[2] = {0, 0};
  for (int a = 0; a < 3; ++a) gu[0] += u[a] * g.G[a][0], gu[1] += u[a] * g.G[a][1];
  k.g2 = gu[0] * gu[0] + gu[1] * gu[1];
  double Iss = 0.0;
  for (int a = 0; a < 3; ++a) {
    k.ga[a] = gu[0] * g.G[a][0] + gu[1] * g.G[a][1];
    k.Ms[a] = 0.0;
    for (int b = 0; b < 3; ++b) k.Ms[a] += tri_me(area, a, b) * (1.0 - c[b]);
    Iss += (1.0 - c[a]) * k.Ms[a];
  }
  k.Iw = (1.0 - eps) * Iss + eps * area;  // w(c) = (1 - eps) (1 - c)^2 + eps (:119)
  return k;
}

__global__ __launch_bounds__(128) void k_fr_residual(int nc, int nv, const int32_t* __restrict__ cells,
                                                     const double* __restrict__ coords, const int8_t* __restrict__ sign,
                                                     const double* __restrict__ x, const double* __restrict__ xk,
                                                     const double* __restrict__ zprev, double alpha, double T, FrPar P, FrQuad Q,
                                                     double* __restrict__ stash) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)cell;
  const TriGeom g = tri_geom(coords, cv);
  double u[3], c[3], p[3], dp[3], cp[3], lift[3];
  for (int a = 0; a < 3; ++a) {
    const size_t v = cv[a];
    u[a] = x[v], c[a] = x[nv + v], p[a] = x[2 * (size_t)nv + v];
    dp[a] = p[a] - xk[2 * (size_t)nv + v];
    cp[a] = zprev[nv + v];
    const int s = sign[v];
    lift[a] = s ? (double)s * T - u[a] : 0.0;  // g - x_b on the cell's Dirichlet vertices
  }
  const double area = 0.5 * g.adet;
  const FrCell k = fr_cell(g, area, u, c, P.eps);
  double gc[2] = {0, 0};
  for (int a = 0; a < 3; ++a) gc[0] += c[a] * g.G[a][0], gc[1] += c[a] * g.G[a][1];
  const double dwf = -2.0 * (1.0 - P.eps);  // w'(c) = dwf (1 - c)
  double Rv[3], Rd[3], Rp[3];
  for (int a = 0; a < 3; ++a) {
    double mc = 0, mdp = 0;
    for (int b = 0; b < 3; ++b) mc += tri_me(area, a, b) * c[b], mdp += tri_me(area, a, b) * dp[b];
    Rv[a] = alpha * P.G * k.Iw * k.ga[a];                                                             // :119, :125
    Rd[a] = alpha * (0.5 * P.G * dwf * k.g2 * k.Ms[a] + P.Gc / P.l * mc +
                     P.Gc * P.l * area * (gc[0] * g.G[a][0] + gc[1] * g.G[a][1])) + mdp;               // :119-121, :125-127
    Rp[a] = mc;                                                                                        // :128
    for (int b = 0; b < 3; ++b) {  // lifting: element columns of J_reg of the Dirichlet vertices times (g - x_b)
      const double gab = g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1];
      Rv[a] += (alpha * P.G * k.Iw * gab + P.reps * tri_me(area, a, b)) * lift[b];
      Rd[a] += alpha * P.G * dwf * k.ga[b] * k.Ms[a] * lift[b];
    }
  }
  for (int q = 0; q < Q.nq; ++q) {  // - (c_conform, phi) (:114, :129)
    const double* N = Q.N[q];
    const double pq = p[0] * N[0] + p[1] * N[1] + p[2] * N[2], cpq = cp[0] * N[0] + cp[1] * N[1] + cp[2] * N[2];
    double s, ds;
    fr_sigma(pq, &s, &ds);
    const double wc = Q.w[q] * g.adet * (cpq + (1.0 - cpq) * s);
    for (int a = 0; a < 3; ++a) Rp[a] -= wc * N[a];
  }
  for (int a = 0; a < 3; ++a) {  // parked slot-major; pgx_scatter sums per dof in a fixed order
    stash[(size_t)a * nc + cell] = Rv[a];
    stash[(size_t)(3 + a) * nc + cell] = Rd[a];
    stash[(size_t)(6 + a) * nc + cell] = Rp[a];
  }
}
__global__ void k_fr_resid_bc(int nv, const int8_t* __restrict__ sign, const double* __restrict__ x, double T,
                              double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nv && sign[i]) F[i] = x[i] - (double)sign[i] * T;
}

// scalar M, K once: stash[(k * 9 + a * 3 + b) * nc + cell], k = 0 M, 1 K
__global__ __launch_bounds__(128) void k_fr_const(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                  double* __restrict__ stash) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= nc) return;
  const TriGeom g = tri_geom(coords, cells + 3 * (size_t)cell);
  const double area = 0.5 * g.adet;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      stash[(size_t)(a * 3 + b) * nc + cell] = tri_me(area, a, b);
      stash[(size_t)(9 + a * 3 + b) * nc + cell] = area * (g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1]);
    }
}

// kind: 0 = zero, 1 = reps M (u,u), 2 = alpha (Gc / l M + Gc l K) + reps M (c,c), 3 = M, 4 = -reps M (psi,psi), 5 = Dirichlet diagonal
__global__ void k_fr_recombine(int64_t nnz, int64_t nnz_s, const uint8_t* __restrict__ kind, const int32_t* __restrict__ src,
                               const double* __restrict__ Sc, double alpha, FrPar P, double* __restrict__ Jc) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int t = kind[e];
  const int64_t s = src[e];
  const double M = Sc[s], K = Sc[nnz_s + s];
  Jc[e] = t == 1 ? P.reps * M : t == 2 ? alpha * (P.Gc / P.l * M + P.Gc * P.l * K) + P.reps * M : t == 3 ? M : t == 4 ? -P.reps * M : t == 5 ? 1.0 : 0.0;
}

// the five iterate-dependent blocks (:132-134): stash[(blk * 9 + a * 3 + b) * nc + cell], blk = (u,u), (u,c), (c,u), (c,c), (psi,psi)
__global__ __launch_bounds__(128) void k_fr_jac(int nc, int nv, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                const double* __restrict__ x, const double* __restrict__ zprev, double alpha,
                                                FrPar P, FrQuad Q, double* __restrict__ stash) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)cell;
  const TriGeom g = tri_geom(coords, cv);
  double u[3], c[3], p[3], cp[3];
  for (int a = 0; a < 3; ++a) {
    const size_t v = cv[a];
    u[a] = x[v], c[a] = x[nv + v], p[a] = x[2 * (size_t)nv + v], cp[a] = zprev[nv + v];
  }
  const double area = 0.5 * g.adet;
  const FrCell k = fr_cell(g, area, u, c, P.eps);
  const double dwf = -2.0 * (1.0 - P.eps);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double gab = g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1];
      stash[(size_t)(a * 3 + b) * nc + cell] = alpha * P.G * k.Iw * gab;
      stash[(size_t)(9 + a * 3 + b) * nc + cell] = alpha * P.G * dwf * k.ga[a] * k.Ms[b];
      stash[(size_t)(18 + a * 3 + b) * nc + cell] = alpha * P.G * dwf * k.ga[b] * k.Ms[a];
      stash[(size_t)(27 + a * 3 + b) * nc + cell] = alpha * P.G * (1.0 - P.eps) * k.g2 * tri_me(area, a, b);  // 1/2 G w'' |grad u|^2 M
    }
  double D[6] = {0, 0, 0, 0, 0, 0};  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  for (int q = 0; q < Q.nq; ++q) {
    const double* N = Q.N[q];
    const double pq = p[0] * N[0] + p[1] * N[1] + p[2] * N[2], cpq = cp[0] * N[0] + cp[1] * N[1] + cp[2] * N[2];
    double s, ds;
    fr_sigma(pq, &s, &ds);
    const double wd = Q.w[q] * g.adet * (1.0 - cpq) * ds;
    D[0] += wd * N[0] * N[0], D[1] += wd * N[0] * N[1], D[2] += wd * N[0] * N[2];
    D[3] += wd * N[1] * N[1], D[4] += wd * N[1] * N[2], D[5] += wd * N[2] * N[2];
  }
  const size_t o = (size_t)36 * nc + cell;
  stash[o] = -D[0], stash[o + (size_t)nc] = -D[1], stash[o + 2 * (size_t)nc] = -D[2];
  stash[o + 3 * (size_t)nc] = -D[1], stash[o + 4 * (size_t)nc] = -D[3], stash[o + 5 * (size_t)nc] = -D[4];
  stash[o + 6 * (size_t)nc] = -D[2], stash[o + 7 * (size_t)nc] = -D[4], stash[o + 8 * (size_t)nc] = -D[5];
}

// sum over cells and over the blocks [b0, b1) of d^T M_e d, d = x - y: per-block partials
__global__ __launch_bounds__(256) void k_fr_l2(int nc, int nv, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                               const double* __restrict__ x, const double* __restrict__ y, int b0, int b1,
                                               double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int cell = blockIdx.x * 256 + threadIdx.x; cell < nc; cell += MX_RED * 256) {
    const int32_t* cv = cells + 3 * (size_t)cell;
    const TriGeom g = tri_geom(coords, cv);
    const double area = 0.5 * g.adet;
    for (int blk = b0; blk < b1; ++blk) {
      double d[3];
      for (int a = 0; a < 3; ++a) d[a] = x[(size_t)blk * nv + cv[a]] - y[(size_t)blk * nv + cv[a]];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) s += tri_me(area, a, b) * d[a] * d[b];
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

// c_conform = c_prev + (1 - c_prev) sigma(psi) at reference point i of every cell: out[cell * npts + i]
__global__ void k_fr_conform(int nc, int nv, int npts, const int32_t* __restrict__ cells, const double* __restrict__ x,
                             const double* __restrict__ zprev, const double* __restrict__ pts, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * npts) return;
  const int cell = (int)(t / npts), i = (int)(t % npts);
  const int32_t* cv = cells + 3 * (size_t)cell;
  const double X = pts[2 * i], Y = pts[2 * i + 1], N0 = 1.0 - X - Y;
  const double pq = N0 * x[2 * (size_t)nv + cv[0]] + X * x[2 * (size_t)nv + cv[1]] + Y * x[2 * (size_t)nv + cv[2]];
  const double cpq = N0 * zprev[nv + cv[0]] + X * zprev[nv + cv[1]] + Y * zprev[nv + cv[2]];
  double s, ds;
  fr_sigma(pq, &s, &ds);
  out[t] = cpq + (1.0 - cpq) * s;
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_fr_destroy(pgx_fr_handle* h) { mx_destroy(h); }

void pgx_fr_handle::residual_dev(const double* xin, double* Fout) {
  pgx_fr_handle* h = this;
  MxTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  hipLaunchKernelGGL(k_fr_residual, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->sign, xin,
                     h->xk, h->zprev, h->alpha, h->T, h->P, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
  hipLaunchKernelGGL(k_fr_resid_bc, dim3((h->nv + 255) / 256), dim3(256), 0, h->st, h->nv, h->sign, xin, h->T, Fout);
}
void pgx_fr_handle::jacobian_dev(const double* xin) {
  pgx_fr_handle* h = this;
  MxTimer t(h, 1);
  if (h->alpha_J != h->alpha) {  // the iterate-independent part changes only with alpha
    hipLaunchKernelGGL(k_fr_recombine, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->st, h->nnz, h->nnz / 9, h->kind,
                       h->src, h->Sc, h->alpha, h->P, h->Jc);
    h->alpha_J = h->alpha;
  }
  hipMemcpyAsync(h->Jv, h->Jc, sizeof(double) * h->nnz, hipMemcpyDeviceToDevice, h->st);
  hipLaunchKernelGGL(k_fr_jac, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, xin, h->zprev,
                     h->alpha, h->P, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_jac, h->stash, 1.0, 1, h->Jv);
  h->jac_valid = true;
}

static int fr_create_impl(pgx_fr_handle* h, const pgx_mesh* m, const pgx_fr_problem* p) {
  const int nv = m->n_vertices, nc = m->n_cells;
  const int64_t ntot = 3 * (int64_t)nv;
  h->nv = nv, h->nc = nc, h->ntot = ntot;
  h->P = FrPar{p->G, p->Gc, p->l, p->eps, p->reps};
  h->Q.fill(p->qpts, p->qwts, p->nq);
  if (const char* e = check_cells(m->cells, 3, nc, nv)) {
    h->err = e;
    return PGX_EINVAL;
  }
  for (int c = 0; c < nc; ++c) {
    const int32_t* cv = m->cells + 3 * (size_t)c;
    const double* X0 = m->coords + 2 * (size_t)cv[0];
    const double* X1 = m->coords + 2 * (size_t)cv[1];
    const double* X2 = m->coords + 2 * (size_t)cv[2];
    const double det = (X1[0] - X0[0]) * (X2[1] - X0[1]) - (X2[0] - X0[0]) * (X1[1] - X0[1]);
    if (!(det != 0.0) || !std::isfinite(det)) {
      h->err = "degenerate cell";
      return PGX_EINVAL;
    }
  }
  std::vector<int8_t> hsign(nv, 0);
  for (int side = 0; side < 2; ++side) {
    const int n = side ? p->n_plus : p->n_minus;
    const int32_t* d = side ? p->plus_dofs : p->minus_dofs;
    for (int k = 0; k < n; ++k) {
      if (d[k] < 0 || d[k] >= nv) {
        h->err = "bc dof out of range";
        return PGX_EINVAL;
      }
      if (hsign[d[k]] && hsign[d[k]] != (side ? 1 : -1)) {
        h->err = "a vertex is in both Dirichlet lists";
        return PGX_EINVAL;
      }
      hsign[d[k]] = side ? 1 : -1;
    }
  }
  // scalar P1 pattern (vertex adjacency incl. self), then 3 x 3 blocks
  std::vector<int32_t> sptr, scol;
  p1_adjacency(nv, nc, m->cells, true, sptr, scol);  // true: a vertex of no cell keeps its diagonal, its rows are not empty
  const int64_t nnz_s = sptr[nv];
  if (9 * nnz_s > 0x7fffffff || 45 * (int64_t)nc > 0x7fffffff) {
    h->err = "mixed matrix exceeds int32 nnz";
    return PGX_EINVAL;
  }
  const int64_t tot = 9 * nnz_s;
  h->nnz = tot;
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  col.resize(tot);
  std::vector<uint8_t> kind(tot);
  std::vector<int32_t> src(tot);
  for (int fr = 0; fr < 3; ++fr)
    for (int v = 0; v < nv; ++v) rowptr[(int64_t)fr * nv + v + 1] = 3 * (sptr[v + 1] - sptr[v]);
  for (int64_t r = 0; r < ntot; ++r) rowptr[r + 1] += rowptr[r];
  for (int fr = 0; fr < 3; ++fr)
    for (int v = 0; v < nv; ++v) {
      const int64_t r = (int64_t)fr * nv + v;
      const int len = sptr[v + 1] - sptr[v];
      for (int fc = 0; fc < 3; ++fc)
        for (int k = 0; k < len; ++k) {
          const int32_t j = scol[sptr[v] + k];
          const int64_t e = rowptr[r] + (int64_t)fc * len + k;
          col[e] = fc * nv + j;
          src[e] = sptr[v] + k;
          uint8_t t;
          if (fr == 0 && hsign[v])
            t = (fc == 0 && j == v) ? 5 : 0;  // Dirichlet row: identity
          else if (fc == 0 && hsign[j])
            t = 0;  // Dirichlet column
          else if (fr == 0)
            t = fc == 0 ? 1 : 0;
          else if (fr == 1)
            t = fc == 0 ? 0 : fc == 1 ? 2 : 3;
          else
            t = fc == 0 ? 0 : fc == 1 ? 3 : 4;
          kind[e] = t;
        }
    }
  auto find = [&](int fr, int32_t v, int fc, int32_t j) -> int32_t {
    const int len = sptr[v + 1] - sptr[v];
    const int32_t* b = scol.data() + sptr[v];
    const int k = (int)(std::lower_bound(b, b + len, j) - b);
    return (int32_t)(rowptr[(int64_t)fr * nv + v] + (int64_t)fc * len + k);
  };
  // destination tables, slot-major like the stashes: table[slot * nc + cell]; -1 drops a contribution (Dirichlet rows and columns)
  std::vector<int32_t> d45((size_t)nc * 45), d18((size_t)nc * 18), d9((size_t)nc * 9);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    const int blk_r[5] = {0, 0, 1, 1, 2}, blk_c[5] = {0, 1, 0, 1, 2};
    for (int64_t c = a0; c < b0; ++c) {
      const int32_t* cv = m->cells + 3 * (size_t)c;
      for (int a = 0; a < 3; ++a) {
        for (int fld = 0; fld < 3; ++fld) d9[(size_t)(fld * 3 + a) * nc + (size_t)c] = fld * nv + cv[a];
        for (int b = 0; b < 3; ++b) {
          for (int k = 0; k < 5; ++k) {
            const bool drop = (blk_r[k] == 0 && hsign[cv[a]]) || (blk_c[k] == 0 && hsign[cv[b]]);
            d45[(size_t)(k * 9 + a * 3 + b) * nc + (size_t)c] = drop ? -1 : find(blk_r[k], cv[a], blk_c[k], cv[b]);
          }
          const int len = sptr[cv[a] + 1] - sptr[cv[a]];
          const int32_t* sb = scol.data() + sptr[cv[a]];
          const int32_t s = sptr[cv[a]] + (int32_t)(std::lower_bound(sb, sb + len, cv[b]) - sb);
          d18[(size_t)(a * 3 + b) * nc + (size_t)c] = s;
          d18[(size_t)(9 + a * 3 + b) * nc + (size_t)c] = (int32_t)(nnz_s + s);
        }
      }
    }
  });
  std::vector<int32_t> nod(ntot);
  for (int v = 0; v < nv; ++v) nod[v] = nod[(size_t)nv + v] = nod[2 * (size_t)nv + v] = v;
  MXHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, nv, nod.data(), 2, m->coords);
  if (rc) return rc;
  // J_reg with its Dirichlet rows AND columns replaced is symmetric (indefinite) as assembled: L D L^T in LU clothing (pgx_nd.h)
  pgx_nd_set_symmetric(h->lu, 1);
  MXALLOC(h->coords, 2 * (size_t)nv);
  MXALLOC(h->cells, 3 * (size_t)nc);
  MXALLOC(h->sign, nv);
  MXALLOC(h->zprev, ntot);
  MXALLOC(h->stash, 45 * (size_t)nc);
  MXALLOC(h->Sc, 2 * nnz_s);
  MXALLOC(h->kind, tot);
  MXALLOC(h->src, tot);
  MXALLOC(h->Jc, tot);
  MXALLOC(h->d_pts, 2 * FR_MAXPTS);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  MXHIP(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->cells, m->cells, sizeof(int32_t) * 3 * (size_t)nc, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->sign, hsign.data(), nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->src, src.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->zprev, 0, sizeof(double) * ntot, h->st));
  MXHIP(hipMemsetAsync(h->Jv, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->Sc, 0, sizeof(double) * 2 * nnz_s, h->st));
  {
    std::string e1 = pgx_scatter_build(d9.data(), (int64_t)9 * nc, ntot, h->allocs, &h->sc_res);
    if (e1.empty()) e1 = pgx_scatter_build(d45.data(), (int64_t)45 * nc, tot, h->allocs, &h->sc_jac);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  // scalar M and K, once: the stash is the handle's
  return mx_scatter_once(h, d18.data(), 18, nc, 2 * nnz_s, h->stash, [&](double* stash) {
    hipLaunchKernelGGL(k_fr_const, dim3((nc + 127) / 128), dim3(128), 0, h->st, nc, h->cells, h->coords, stash);
  }, h->Sc, 0);
}

extern "C" int pgx_fr_create(const pgx_mesh* m, const pgx_fr_problem* p, int device, pgx_fr_handle** out) {
  if (!m || !p || !out || !m->coords || !m->cells || m->n_vertices <= 0 || m->n_cells <= 0 || !p->qpts || !p->qwts || p->nq <= 0 ||
      p->nq > FR_MAXQ || p->n_minus < 0 || p->n_plus < 0 || (p->n_minus > 0 && !p->minus_dofs) || (p->n_plus > 0 && !p->plus_dofs) ||
      !(p->l > 0.0) || !std::isfinite(p->l) || !(p->eps >= 0.0) || !(p->reps >= 0.0) || !std::isfinite(p->G) || !std::isfinite(p->Gc)) {
    g_fr_error = "pgx_fr_create: bad arguments";
    return PGX_EINVAL;
  }
  return mx_create("pgx_fr_create", g_fr_error, device, out, [&](pgx_fr_handle* h) { return fr_create_impl(h, m, p); });
}

extern "C" int pgx_fr_num_dofs(const pgx_fr_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_fr_set_state(pgx_fr_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_fr_get_state(pgx_fr_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_fr_set_prev(pgx_fr_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_fr_get_prev(pgx_fr_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_fr_advance_prev(pgx_fr_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_fr_set_alpha(pgx_fr_handle* h, double a) { return mx_set_alpha(h, a); }
extern "C" int pgx_fr_residual(pgx_fr_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_fr_jacobian_fill(pgx_fr_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_fr_csr_export(pgx_fr_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_fr_spmv(pgx_fr_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
// linesearch 2: l2 (the script's), 1 / 3: bt of order 2 / 3, every other value: plain Newton
extern "C" int pgx_fr_newton_solve(pgx_fr_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its) {
  return mx_newton(h, opts, reason, its, lin_its, true);
}
extern "C" int pgx_fr_profile(pgx_fr_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

extern "C" int pgx_fr_set_load(pgx_fr_handle* h, double T) {
  MXNEED(h);
  if (!std::isfinite(T)) {
    h->err = "the load must be finite";
    return PGX_EINVAL;
  }
  h->T = T;
  return PGX_OK;
}
static int fr_copy(pgx_fr_handle* h, double* dst, const double* src, hipMemcpyKind kind) {
  MXHIP(hipMemcpyAsync(dst, src, sizeof(double) * h->ntot, kind, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_fr_set_zprev(pgx_fr_handle* h, const double* z) {
  MXNEED(h);
  h->jac_valid = false;
  return mx_in(h, h->zprev, z);
}
extern "C" int pgx_fr_get_zprev(pgx_fr_handle* h, double* z) {
  MXNEED(h);
  if (!z) return PGX_EINVAL;
  return fr_copy(h, z, h->zprev, hipMemcpyDeviceToHost);
}
extern "C" int pgx_fr_zprev_from_state(pgx_fr_handle* h) {
  MXNEED(h);
  h->jac_valid = false;
  return fr_copy(h, h->zprev, h->x, hipMemcpyDeviceToDevice);
}
extern "C" int pgx_fr_state_from_zprev(pgx_fr_handle* h) {
  MXNEED(h);
  return fr_copy(h, h->x, h->zprev, hipMemcpyDeviceToDevice);
}
extern "C" int pgx_fr_state_from_prev(pgx_fr_handle* h) {
  MXNEED(h);
  return fr_copy(h, h->x, h->xk, hipMemcpyDeviceToDevice);
}
extern "C" int pgx_fr_l2_increment_c(pgx_fr_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_fr_l2, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->x, h->xk, 1, 2, h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_fr_l2_distance_zprev(pgx_fr_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_fr_l2, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->nv, h->cells, h->coords, h->x, h->zprev, 0, 3, h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_fr_conforming_damage(pgx_fr_handle* h, int32_t npts, const double* ref_pts, double* out) {
  MXNEED(h);
  if (!ref_pts || !out || npts < 1 || npts > FR_MAXPTS) {
    h->err = "pgx_fr_conforming_damage: 1 <= npts <= 64 reference points and an output array";
    return PGX_EINVAL;
  }
  if (npts > h->conf_cap) {  // the output buffer grows to the largest request; earlier buffers are freed with the handle
    MXALLOC(h->d_conf, (size_t)h->nc * npts);
    h->conf_cap = npts;
  }
  const int64_t n = (int64_t)h->nc * npts;
  MXHIP(hipMemcpyAsync(h->d_pts, ref_pts, sizeof(double) * 2 * npts, hipMemcpyHostToDevice, h->st));
  MXHIP(hipStreamSynchronize(h->st));  // ref_pts is pageable host memory of the caller
  hipLaunchKernelGGL(k_fr_conform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->nc, h->nv, (int)npts, h->cells, h->x,
                     h->zprev, h->d_pts, h->d_conf);
  MXHIP(hipMemcpyAsync(out, h->d_conf, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  MXHIP(hipGetLastError());
  return PGX_OK;
}
extern "C" int pgx_fr_lu_stats(const pgx_fr_handle* h, pgx_nd_stats* st) { return h ? pgx_nd_get_stats(h->lu, st) : PGX_EINVAL; }
extern "C" int pgx_fr_lu_is_symmetric(const pgx_fr_handle* h) { return h ? pgx_nd_is_symmetric(h->lu) : 0; }
