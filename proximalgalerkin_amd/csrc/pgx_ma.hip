// pgx_ma.hip - example 10 (three-field mixed Monge-Ampere: u in P_k, p in [P_{k+1}]^2, Psi in [P_k]^3 symmetric, on triangles) behind the
// C ABI of include/pgx_ma.h.  Reference: examples/10_monge_ampere/monge_ampere_dolfinx.py (:51-55 spaces, :81-87 residual, :88-97
// Dirichlet condition, :15-23 solver, :161-163 error) and its expm.py (:43-79).
// x = [u | p0 | p1 | Psi00 | Psi01 | Psi11].  The Jacobian
//     rows v   : [ bc identity   0            0            M      0      M     ]
//     rows q0  : [ -Bx           Mp           0            0      0      0     ]
//     rows q1  : [ -By           0            Mp           0      0      0     ]
//     rows phi : [ 0             Cx / Cy ...               -(Dexpm(Psi)[dPsi], phi): six weighted mass forms ]
// lives in one mixed CSR array.  Everything but the (phi, Psi) block does not depend on the iterate: it is assembled once at create
// (host, fixed order), Dirichlet rows and columns applied, and copied per Newton step; the kernels add the six weighted mass blocks.
// The degree k is a run-time parameter: the basis tables [node][point] are the caller's and stay in global memory (L2).
//
// Kernels: ONE WORKGROUP PER CELL.  Phase 1: threads over the quadrature points, in as many rounds as needed (961 points at k = 14),
// evaluate u, p, grad p, Psi from the cell's nodal values in LDS (broadcast reads; the table reads of a round are coalesced: thread =
// point) and leave the weighted coefficient fields in LDS - six for the Jacobian, six for the residual.  Phase 2: threads over the
// node pairs a <= b (Jacobian) or the 4 nk + 2 nk1 rows (residual) accumulate over the points; every lane reads the same coefficient
// address (a broadcast).  Results are parked cell-major and summed per destination in a fixed order by pgx_scatter.h: no atomics,
// bitwise reproducible; both triangles of a block receive the SAME value, so the (phi, Psi) block is symmetric to the last bit.
// LDS at k = 14 with 961 points: (4 nk + 2 nk1 + 6 nq) doubles = 52 144 B (residual), (3 nk + 6 nq) = 49 008 B (Jacobian): three
// workgroups per CU by LDS; registers are not the bound.
//
// Dirichlet data: u enters the form only through -(grad u, q), linearly, so the lifting F += J(x)[:, bc] (g - x_bc) is the residual
// evaluated with g in place of x on the Dirichlet nodes of u; F[bc] = x_bc - g afterwards.  The state itself is not touched.
#include <cstring>

#include "../../include/pgx_dn.h"
#include "../../include/pgx_ma.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"

#define MA_DSMALL 1.0e-4  // below: the series 1 + d^2 / 6 and 1 / 3 + d^2 / 30
#define MA_BLOCK 256

static thread_local std::string g_ma_error;

struct pgx_ma_handle : MixedBase {
  int k = 0, nk = 0, nk1 = 0, nq = 0, nc = 0, nu = 0, np = 0;
  int64_t off[7] = {0, 0, 0, 0, 0, 0, 0};  // block offsets of x
  int32_t *cdu = nullptr, *cdp = nullptr;  // [nc][nk], [nc][nk1]
  double *tabU = nullptr, *dU = nullptr, *tabP = nullptr, *dP = nullptr;  // [nk][nq], [2][nk][nq], ...
  double* geo = nullptr;    // [nc][5]: inverse Jacobian (row-major) and |det|
  double* qw = nullptr;     // [nq]
  double* lnrho = nullptr;  // [nc][nq]
  double* uex = nullptr;    // [nc][nq] scratch of l2_error
  uint8_t* isbc = nullptr;  // [nu]
  double* gv = nullptr;     // [nu] Dirichlet values at the bc dofs, 0 elsewhere
  PgxScatter sc_res, sc_jac, sc_jac_t;
  double* stash = nullptr;  // [nc * max(6 nk^2, 4 nk + 2 nk1)]
  double* Jc = nullptr;     // [nnz] iterate-independent part of the Jacobian
  pgx_dn* dn = nullptr;
  pgx_ma_handle() : MixedBase("pgx_ma") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
  int lin_factor() override { return pgx_dn_factor(dn, Jv, 1); }
  int lin_solve(const double* rhs, double* out) override { return pgx_dn_solve(dn, rhs, out, 1); }
  const char* lin_error() const override { return pgx_dn_last_error(dn); }
  void lin_release() override {
    if (dn) pgx_dn_destroy(dn);
    dn = nullptr;
  }
};

extern "C" const char* pgx_ma_last_error(const pgx_ma_handle* h) { return h ? h->err.c_str() : g_ma_error.c_str(); }

// C = e^m cosh(delta), S = e^m sinh(delta) / delta, G = e^m (cosh(delta) - sinh(delta) / delta) / delta^2 from exp(m +- delta): nothing
// overflows before expm itself does.  Between the series and delta = 1, S = e^(m - delta) expm1(2 delta) / (2 delta): the plain difference
// of the exponentials loses eps / delta, and S enters the derivative without a factor delta.  G only multiplies terms of size delta^2.
__device__ inline void ma_coef(double a, double b, double d, double* C, double* S, double* G, double* h) {
  const double m = 0.5 * (a + d), hh = 0.5 * (a - d), dl = hypot(hh, b);
  const double ep = exp(m + dl), em = exp(m - dl);
  *h = hh;
  *C = 0.5 * (ep + em);
  if (dl < MA_DSMALL) {
    const double e0 = exp(m);
    *S = e0 * (1.0 + dl * dl / 6.0);
    *G = e0 * (1.0 / 3.0 + dl * dl / 30.0);
    return;
  }
  *S = dl < 1.0 ? em * expm1(2.0 * dl) / (2.0 * dl) : (ep - em) / (2.0 * dl);
  *G = (*C - *S) / (dl * dl);
}

// residual of one cell per workgroup: stash[cell * W + row], rows [v (nk) | q0 (nk1) | q1 (nk1) | phi00 | phi01 | phi11 (nk each)]
__global__ __launch_bounds__(MA_BLOCK) void k_ma_residual(int nk, int nk1, int nq, int nu, int np, const int32_t* __restrict__ cdu,
                                                          const int32_t* __restrict__ cdp, const double* __restrict__ tabU,
                                                          const double* __restrict__ dU, const double* __restrict__ tabP,
                                                          const double* __restrict__ dP, const double* __restrict__ geo,
                                                          const double* __restrict__ qw, const double* __restrict__ lnrho,
                                                          const uint8_t* __restrict__ isbc, const double* __restrict__ gv,
                                                          const double* __restrict__ x, double* __restrict__ stash) {
  extern __shared__ double sm[];
  double* sU = sm;                 // [nk] u with g on the Dirichlet nodes (the lifting)
  double* sP = sU + nk;            // [2][nk1]
  double* sS = sP + 2 * nk1;       // [3][nk]
  double* sF = sS + 3 * nk;        // [6][nq]
  const int cell = blockIdx.x, tid = threadIdx.x;
  const int32_t* du = cdu + (size_t)cell * nk;
  const int32_t* dp = cdp + (size_t)cell * nk1;
  const size_t oP = (size_t)nu, oS = (size_t)nu + 2 * (size_t)np;
  for (int a = tid; a < nk; a += MA_BLOCK) {
    const int d = du[a];
    sU[a] = isbc[d] ? gv[d] : x[d];
    for (int f = 0; f < 3; ++f) sS[f * nk + a] = x[oS + (size_t)f * nu + d];
  }
  for (int a = tid; a < nk1; a += MA_BLOCK) {
    const int d = dp[a];
    sP[a] = x[oP + d];
    sP[nk1 + a] = x[oP + np + d];
  }
  __syncthreads();
  const double j00 = geo[cell * 5], j01 = geo[cell * 5 + 1], j10 = geo[cell * 5 + 2], j11 = geo[cell * 5 + 3], det = geo[cell * 5 + 4];
  for (int q = tid; q < nq; q += MA_BLOCK) {
    double ux = 0, ue = 0, s00 = 0, s01 = 0, s11 = 0;
    for (int a = 0; a < nk; ++a) {
      const double N = tabU[(size_t)a * nq + q];
      ux = fma(sU[a], dU[(size_t)a * nq + q], ux);
      ue = fma(sU[a], dU[(size_t)(nk + a) * nq + q], ue);
      s00 = fma(sS[a], N, s00);
      s01 = fma(sS[nk + a], N, s01);
      s11 = fma(sS[2 * nk + a], N, s11);
    }
    double p0 = 0, p1 = 0, p0x = 0, p0e = 0, p1x = 0, p1e = 0;
    for (int a = 0; a < nk1; ++a) {
      const double N = tabP[(size_t)a * nq + q], Nx = dP[(size_t)a * nq + q], Ne = dP[(size_t)(nk1 + a) * nq + q];
      p0 = fma(sP[a], N, p0), p1 = fma(sP[nk1 + a], N, p1);
      p0x = fma(sP[a], Nx, p0x), p0e = fma(sP[a], Ne, p0e);
      p1x = fma(sP[nk1 + a], Nx, p1x), p1e = fma(sP[nk1 + a], Ne, p1e);
    }
    // physical gradients: d/dX_d = sum_r d/dxi_r Jinv[r][d]
    const double gux = ux * j00 + ue * j10, guy = ux * j01 + ue * j11;
    const double p0dx = p0x * j00 + p0e * j10, p0dy = p0x * j01 + p0e * j11;
    const double p1dx = p1x * j00 + p1e * j10, p1dy = p1x * j01 + p1e * j11;
    double C, S, G, h;
    ma_coef(s00, s01, s11, &C, &S, &G, &h);
    const double w = qw[q] * det;
    sF[q] = w * (s00 + s11 - lnrho[(size_t)cell * nq + q]);
    sF[nq + q] = w * (p0 - gux);
    sF[2 * nq + q] = w * (p1 - guy);
    sF[3 * nq + q] = w * (p0dx - (C + S * h));
    sF[4 * nq + q] = w * (p0dy + p1dx - 2.0 * S * s01);
    sF[5 * nq + q] = w * (p1dy - (C - S * h));
  }
  __syncthreads();
  const int W = 4 * nk + 2 * nk1;
  for (int r = tid; r < W; r += MA_BLOCK) {
    int f, a;
    const double* tab;
    if (r < nk)
      f = 0, a = r, tab = tabU;
    else if (r < nk + 2 * nk1)
      f = 1 + (r - nk) / nk1, a = (r - nk) % nk1, tab = tabP;
    else
      f = 3 + (r - nk - 2 * nk1) / nk, a = (r - nk - 2 * nk1) % nk, tab = tabU;
    const double* N = tab + (size_t)a * nq;
    const double* F = sF + f * nq;
    double R = 0.0;
    for (int q = 0; q < nq; ++q) R = fma(N[q], F[q], R);
    stash[(size_t)cell * W + r] = R;
  }
}

__global__ void k_ma_resid_bc(int nu, const uint8_t* __restrict__ isbc, const double* __restrict__ x, const double* __restrict__ gv,
                              double* __restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nu && isbc[i]) F[i] = x[i] - gv[i];
}

// the six weighted mass blocks -D of one cell per workgroup: stash[cell * 6 nk^2 + blk * nk^2 + a * nk + b],
// blk = (00,00), (00,01), (00,11), (01,01), (01,11), (11,11) of D[i][j] = <B_i, Dexpm(Psi)[B_j]>, B = (e00, e01 + e10, e11)
__global__ __launch_bounds__(MA_BLOCK) void k_ma_jac(int nk, int nq, int nu, int np, const int32_t* __restrict__ cdu,
                                                     const double* __restrict__ tabU, const double* __restrict__ geo,
                                                     const double* __restrict__ qw, const double* __restrict__ x,
                                                     double* __restrict__ stash) {
  extern __shared__ double sm[];
  double* sS = sm;            // [3][nk]
  double* sC = sS + 3 * nk;   // [6][nq]
  const int cell = blockIdx.x, tid = threadIdx.x;
  const int32_t* du = cdu + (size_t)cell * nk;
  const size_t oS = (size_t)nu + 2 * (size_t)np;
  for (int a = tid; a < nk; a += MA_BLOCK)
    for (int f = 0; f < 3; ++f) sS[f * nk + a] = x[oS + (size_t)f * nu + du[a]];
  __syncthreads();
  const double det = geo[cell * 5 + 4];
  for (int q = tid; q < nq; q += MA_BLOCK) {
    double s00 = 0, s01 = 0, s11 = 0;
    for (int a = 0; a < nk; ++a) {
      const double N = tabU[(size_t)a * nq + q];
      s00 = fma(sS[a], N, s00);
      s01 = fma(sS[nk + a], N, s01);
      s11 = fma(sS[2 * nk + a], N, s11);
    }
    double C, S, G, h;
    ma_coef(s00, s01, s11, &C, &S, &G, &h);
    const double b = s01, w = -qw[q] * det;
    // dE = e^m [dm (cosh I + s H) + s t I + g t H + s dH], t = h dh + b db; directions da: (dm, dh, db) = (1/2, 1/2, 0), db: (0, 0, 1),
    // dd: (1/2, -1/2, 0); rows (E00, 2 E01, E11)
    const double ta = 0.5 * h, tb = b, td = -0.5 * h;
    const double D00 = 0.5 * (C + S * h) + S * ta + G * ta * h + 0.5 * S;
    const double D01 = S * tb + G * tb * h;                       // E00 along db
    const double D02 = 0.5 * (C + S * h) + S * td + G * td * h - 0.5 * S;  // E00 along dd
    const double D11 = 2.0 * (G * tb * b + S);                    // 2 E01 along db
    const double D12 = 2.0 * (0.5 * S * b + G * td * b);          // 2 E01 along dd
    const double D22 = 0.5 * (C - S * h) + S * td - G * td * h + 0.5 * S;  // E11 along dd
    sC[q] = w * D00, sC[nq + q] = w * D01, sC[2 * nq + q] = w * D02, sC[3 * nq + q] = w * D11, sC[4 * nq + q] = w * D12,
    sC[5 * nq + q] = w * D22;
  }
  __syncthreads();
  const int npair = nk * (nk + 1) / 2;
  double* o = stash + (size_t)cell * 6 * nk * nk;
  for (int t = tid; t < npair; t += MA_BLOCK) {
    int a = 0, b = t;  // pair t of the upper triangle, row by row: a <= b
    while (b >= nk - a) b -= nk - a, ++a;
    b += a;
    const double* Na = tabU + (size_t)a * nq;
    const double* Nb = tabU + (size_t)b * nq;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < nq; ++q) {
      const double ww = Na[q] * Nb[q];
#pragma unroll
      for (int f = 0; f < 6; ++f) acc[f] = fma(ww, sC[f * nq + q], acc[f]);
    }
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      o[(size_t)f * nk * nk + a * nk + b] = acc[f];
      o[(size_t)f * nk * nk + b * nk + a] = acc[f];
    }
  }
}

// sum over cells of int (u_h - u_exact)^2: MX_RED blocks, block b takes the cells b, b + MX_RED, ...; fixed-shape tree per block
__global__ __launch_bounds__(MA_BLOCK) void k_ma_l2(int nc, int nk, int nq, const int32_t* __restrict__ cdu, const double* __restrict__ tabU,
                                                    const double* __restrict__ geo, const double* __restrict__ qw,
                                                    const double* __restrict__ uex, const double* __restrict__ x,
                                                    double* __restrict__ partials) {
  extern __shared__ double sm[];
  double* sU = sm;        // [nk]
  double* sh = sm + nk;   // [MA_BLOCK]
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int cell = blockIdx.x; cell < nc; cell += MX_RED) {
    __syncthreads();
    for (int a = tid; a < nk; a += MA_BLOCK) sU[a] = x[cdu[(size_t)cell * nk + a]];
    __syncthreads();
    double s = 0.0;
    for (int q = tid; q < nq; q += MA_BLOCK) {
      double u = 0.0;
      for (int a = 0; a < nk; ++a) u = fma(sU[a], tabU[(size_t)a * nq + q], u);
      const double d = u - uex[(size_t)cell * nq + q];
      s = fma(qw[q] * geo[cell * 5 + 4], d * d, s);
    }
    sh[tid] = s;
    __syncthreads();
    for (int o = MA_BLOCK / 2; o > 0; o >>= 1) {
      if (tid < o) sh[tid] += sh[tid + o];
      __syncthreads();
    }
    total += sh[0];
  }
  if (tid == 0) partials[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_ma_destroy(pgx_ma_handle* h) { mx_destroy(h); }

void pgx_ma_handle::residual_dev(const double* xin, double* Fout) {
  pgx_ma_handle* h = this;
  MxTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  const size_t lds = sizeof(double) * ((size_t)4 * nk + 2 * nk1 + 6 * (size_t)nq);
  hipLaunchKernelGGL(k_ma_residual, dim3(nc), dim3(MA_BLOCK), lds, h->st, nk, nk1, nq, nu, np, cdu, cdp, tabU, dU, tabP, dP, geo, qw, lnrho,
                     isbc, gv, xin, stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
  hipLaunchKernelGGL(k_ma_resid_bc, dim3((nu + 255) / 256), dim3(256), 0, h->st, nu, isbc, xin, gv, Fout);
}
void pgx_ma_handle::jacobian_dev(const double* xin) {
  pgx_ma_handle* h = this;
  MxTimer t(h, 1);
  hipMemcpyAsync(h->Jv, h->Jc, sizeof(double) * h->nnz, hipMemcpyDeviceToDevice, h->st);
  const size_t lds = sizeof(double) * ((size_t)3 * nk + 6 * (size_t)nq);
  hipLaunchKernelGGL(k_ma_jac, dim3(nc), dim3(MA_BLOCK), lds, h->st, nk, nq, nu, np, cdu, tabU, geo, qw, xin, stash);
  pgx_scatter_run(h->st, h->sc_jac, h->stash, 1.0, 1, h->Jv);
  pgx_scatter_run(h->st, h->sc_jac_t, h->stash, 1.0, 1, h->Jv);
  h->jac_valid = true;
}

// which adjacency a (row block, column block) pair uses: 0 none, 1 P_k x P_k, 2 P_k x P_{k+1}, 3 P_{k+1} x P_k, 4 P_{k+1} x P_{k+1},
// 5 the diagonal entry only (the Dirichlet identity of the structurally zero (v, u) block)
static const int8_t MA_KIND[6][6] = {{5, 0, 0, 1, 0, 1}, {3, 4, 0, 0, 0, 0}, {3, 0, 4, 0, 0, 0},
                                     {0, 2, 0, 1, 1, 1}, {0, 2, 2, 1, 1, 1}, {0, 0, 2, 1, 1, 1}};

static int ma_create_impl(pgx_ma_handle* h, const pgx_ma_problem* pr) {
  const int k = pr->degree, nk = (k + 1) * (k + 2) / 2, nk1 = (k + 2) * (k + 3) / 2, nq = pr->nq, nc = pr->nc, nu = pr->nu, np = pr->np;
  const int64_t ntot = 4 * (int64_t)nu + 2 * (int64_t)np;
  if (ntot > PGX_DN_MAX_N) {
    h->err = "pgx_ma_create: " + std::to_string(ntot) + " unknowns exceed the dense LU's limit of " + std::to_string(PGX_DN_MAX_N);
    return PGX_EINVAL;
  }
  const size_t lds = sizeof(double) * ((size_t)4 * nk + 2 * nk1 + 6 * (size_t)nq);
  if (lds > 64 * 1024) {
    h->err = "pgx_ma_create: degree " + std::to_string(k) + " with " + std::to_string(nq) + " points needs " + std::to_string(lds) +
             " bytes of LDS per workgroup (limit 65536)";
    return PGX_EINVAL;
  }
  h->k = k, h->nk = nk, h->nk1 = nk1, h->nq = nq, h->nc = nc, h->nu = nu, h->np = np, h->ntot = ntot;
  const int64_t off[7] = {0, nu, nu + (int64_t)np, nu + 2 * (int64_t)np, 2 * (int64_t)nu + 2 * np, 3 * (int64_t)nu + 2 * np, ntot};
  memcpy(h->off, off, sizeof off);
  for (int64_t i = 0; i < (int64_t)nc * nk; ++i)
    if (pr->cell_dofs_u[i] < 0 || pr->cell_dofs_u[i] >= nu) {
      h->err = "pgx_ma_create: cell_dofs_u out of range";
      return PGX_EINVAL;
    }
  for (int64_t i = 0; i < (int64_t)nc * nk1; ++i)
    if (pr->cell_dofs_p[i] < 0 || pr->cell_dofs_p[i] >= np) {
      h->err = "pgx_ma_create: cell_dofs_p out of range";
      return PGX_EINVAL;
    }
  std::vector<uint8_t> isbc(nu, 0);
  std::vector<double> gv(nu, 0.0);
  for (int i = 0; i < pr->n_bc; ++i) {
    const int32_t d = pr->bc_dofs[i];
    if (d < 0 || d >= nu || !std::isfinite(pr->g[i])) {
      h->err = "pgx_ma_create: bc dof out of range or Dirichlet value not finite";
      return PGX_EINVAL;
    }
    isbc[d] = 1, gv[d] = pr->g[i];
  }
  // geometry: X = X0 + Jc xi, Jc columns = edge vectors; the upper triangles of a right-diagonal mesh are numbered clockwise: |det|
  std::vector<double> geo((size_t)nc * 5);
  for (int c = 0; c < nc; ++c) {
    const int32_t* v = pr->cells + 3 * (size_t)c;
    for (int i = 0; i < 3; ++i)
      if (v[i] < 0 || v[i] >= pr->nv) {
        h->err = "pgx_ma_create: cell vertex out of range";
        return PGX_EINVAL;
      }
    const double* X0 = pr->coords + 2 * (size_t)v[0];
    const double* X1 = pr->coords + 2 * (size_t)v[1];
    const double* X2 = pr->coords + 2 * (size_t)v[2];
    const double a = X1[0] - X0[0], b = X2[0] - X0[0], cc = X1[1] - X0[1], d = X2[1] - X0[1], det = a * d - b * cc;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) {
      h->err = "pgx_ma_create: degenerate cell " + std::to_string(c);
      return PGX_EINVAL;
    }
    double* g = &geo[(size_t)c * 5];
    g[0] = d / det, g[1] = -b / det, g[2] = -cc / det, g[3] = a / det, g[4] = std::fabs(det);
  }
  // adjacency of the four space pairs through the cells
  const int32_t* cd[2] = {pr->cell_dofs_u, pr->cell_dofs_p};
  const int nloc[2] = {nk, nk1}, ndof[2] = {nu, np};
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
  const int sp_of[6] = {0, 1, 1, 0, 0, 0};  // space of each block: 0 = P_k, 1 = P_{k+1}
  auto blen = [&](int rb, int cb, int i) -> int64_t {
    const int t = MA_KIND[rb][cb];
    return t == 0 ? 0 : t == 5 ? 1 : (int64_t)adj[sp_of[rb]][sp_of[cb]][i].size();
  };
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  int64_t tot = 0;
  for (int rb = 0; rb < 6; ++rb)
    for (int i = 0; i < ndof[sp_of[rb]]; ++i) {
      for (int cb = 0; cb < 6; ++cb) tot += blen(rb, cb, i);
      if (tot > 0x7fffffff) {
        h->err = "pgx_ma_create: mixed matrix exceeds int32 nnz";
        return PGX_EINVAL;
      }
      rowptr[off[rb] + i + 1] = (int32_t)tot;
    }
  h->nnz = tot;
  col.resize(tot);
  for (int rb = 0; rb < 6; ++rb)
    for (int i = 0; i < ndof[sp_of[rb]]; ++i) {
      int64_t e = rowptr[off[rb] + i];
      for (int cb = 0; cb < 6; ++cb) {
        const int t = MA_KIND[rb][cb];
        if (t == 5)
          col[e++] = (int32_t)(off[cb] + i);
        else if (t)
          for (int32_t j : adj[sp_of[rb]][sp_of[cb]][i]) col[e++] = (int32_t)(off[cb] + j);
      }
    }
  auto find = [&](int rb, int32_t i, int cb, int32_t j) -> int32_t {
    int64_t e = rowptr[off[rb] + i];
    for (int c2 = 0; c2 < cb; ++c2) e += blen(rb, c2, i);
    if (MA_KIND[rb][cb] == 5) return (int32_t)e;
    const auto& row = adj[sp_of[rb]][sp_of[cb]][i];
    return (int32_t)(e + (std::lower_bound(row.begin(), row.end(), j) - row.begin()));
  };
  // the iterate-independent part, cell by cell in a fixed order on the host: element matrices in parallel, their sum serial
  const size_t EW = (size_t)nk * nk + (size_t)nk1 * nk1 + 2 * (size_t)nk1 * nk + 2 * (size_t)nk * nk1;
  std::vector<double> El((size_t)nc * EW, 0.0);
  const double *tU = pr->tab_u, *gU = pr->dtab_u, *tP = pr->tab_p, *gP = pr->dtab_p;
  mx_par_for(nc, [&](int64_t c0, int64_t c1) {
    std::vector<double> ux(nk), uy(nk), px(nk1), py(nk1);
    for (int64_t c = c0; c < c1; ++c) {
      const double* g = &geo[(size_t)c * 5];
      double* M = &El[(size_t)c * EW];
      double* Mp = M + (size_t)nk * nk;
      double* Bx = Mp + (size_t)nk1 * nk1;
      double* By = Bx + (size_t)nk1 * nk;
      double* Cx = By + (size_t)nk1 * nk;
      double* Cy = Cx + (size_t)nk * nk1;
      for (int q = 0; q < nq; ++q) {
        const double w = pr->qwts[q] * g[4];
        for (int a = 0; a < nk; ++a) {
          const double dx = gU[(size_t)a * nq + q], de = gU[(size_t)(nk + a) * nq + q];
          ux[a] = dx * g[0] + de * g[2], uy[a] = dx * g[1] + de * g[3];
        }
        for (int a = 0; a < nk1; ++a) {
          const double dx = gP[(size_t)a * nq + q], de = gP[(size_t)(nk1 + a) * nq + q];
          px[a] = dx * g[0] + de * g[2], py[a] = dx * g[1] + de * g[3];
        }
        for (int a = 0; a < nk; ++a) {
          const double wa = w * tU[(size_t)a * nq + q];
          for (int b = 0; b < nk; ++b) M[(size_t)a * nk + b] += wa * tU[(size_t)b * nq + q];
          for (int b = 0; b < nk1; ++b) Cx[(size_t)a * nk1 + b] += wa * px[b], Cy[(size_t)a * nk1 + b] += wa * py[b];
        }
        for (int a = 0; a < nk1; ++a) {
          const double wa = w * tP[(size_t)a * nq + q];
          for (int b = 0; b < nk1; ++b) Mp[(size_t)a * nk1 + b] += wa * tP[(size_t)b * nq + q];
          for (int b = 0; b < nk; ++b) Bx[(size_t)a * nk + b] += wa * ux[b], By[(size_t)a * nk + b] += wa * uy[b];
        }
      }
    }
  });
  std::vector<double> Jc((size_t)tot, 0.0);
  for (int c = 0; c < nc; ++c) {
    const double* M = &El[(size_t)c * EW];
    const double* Mp = M + (size_t)nk * nk;
    const double* Bx = Mp + (size_t)nk1 * nk1;
    const double* By = Bx + (size_t)nk1 * nk;
    const double* Cx = By + (size_t)nk1 * nk;
    const double* Cy = Cx + (size_t)nk * nk1;
    const int32_t* du = pr->cell_dofs_u + (size_t)c * nk;
    const int32_t* dp = pr->cell_dofs_p + (size_t)c * nk1;
    for (int a = 0; a < nk; ++a)
      for (int b = 0; b < nk; ++b)
        if (!isbc[du[a]]) {  // rows v of the Dirichlet dofs: identity only
          Jc[find(0, du[a], 3, du[b])] += M[(size_t)a * nk + b];
          Jc[find(0, du[a], 5, du[b])] += M[(size_t)a * nk + b];
        }
    for (int a = 0; a < nk1; ++a) {
      for (int b = 0; b < nk1; ++b) {
        Jc[find(1, dp[a], 1, dp[b])] += Mp[(size_t)a * nk1 + b];
        Jc[find(2, dp[a], 2, dp[b])] += Mp[(size_t)a * nk1 + b];
      }
      for (int b = 0; b < nk; ++b)
        if (!isbc[du[b]]) {  // Dirichlet columns of u
          Jc[find(1, dp[a], 0, du[b])] -= Bx[(size_t)a * nk + b];
          Jc[find(2, dp[a], 0, du[b])] -= By[(size_t)a * nk + b];
        }
    }
    for (int a = 0; a < nk; ++a)
      for (int b = 0; b < nk1; ++b) {
        const double cx = Cx[(size_t)a * nk1 + b], cy = Cy[(size_t)a * nk1 + b];
        Jc[find(3, du[a], 1, dp[b])] += cx;
        Jc[find(4, du[a], 1, dp[b])] += cy;
        Jc[find(4, du[a], 2, dp[b])] += cx;
        Jc[find(5, du[a], 2, dp[b])] += cy;
      }
  }
  for (int i = 0; i < nu; ++i)
    if (isbc[i]) Jc[find(0, i, 0, i)] = 1.0;
  // destination tables, cell-major like the stashes
  const int Wr = 4 * nk + 2 * nk1;
  const size_t Wj = (size_t)6 * nk * nk;
  if ((int64_t)nc * (int64_t)Wj > 0x7fffffff) {
    h->err = "pgx_ma_create: stash exceeds int32 indices";
    return PGX_EINVAL;
  }
  std::vector<int32_t> dr((size_t)nc * Wr), dj((size_t)nc * Wj), djt((size_t)nc * Wj, -1);
  const int br[6] = {3, 3, 3, 4, 4, 5}, bc[6] = {3, 4, 5, 4, 5, 5};
  mx_par_for(nc, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; ++c) {
      const int32_t* du = pr->cell_dofs_u + (size_t)c * nk;
      const int32_t* dp = pr->cell_dofs_p + (size_t)c * nk1;
      int32_t* r = &dr[(size_t)c * Wr];
      for (int a = 0; a < nk; ++a) {
        r[a] = du[a];
        for (int f = 0; f < 3; ++f) r[nk + 2 * nk1 + f * nk + a] = (int32_t)(off[3 + f] + du[a]);
      }
      for (int a = 0; a < nk1; ++a) r[nk + a] = (int32_t)(off[1] + dp[a]), r[nk + nk1 + a] = (int32_t)(off[2] + dp[a]);
      for (int f = 0; f < 6; ++f)
        for (int a = 0; a < nk; ++a)
          for (int b = 0; b < nk; ++b) {
            const size_t o = (size_t)c * Wj + (size_t)f * nk * nk + (size_t)a * nk + b;
            dj[o] = find(br[f], du[a], bc[f], du[b]);
            if (br[f] != bc[f]) djt[o] = find(bc[f], du[a], br[f], du[b]);  // the transposed block takes the same (symmetric) values
          }
    }
  });
  MXHIP(hipStreamCreate(&h->st));
  int rc = pgx_dn_create(ntot, rowptr.data(), col.data(), h->device, (void*)h->st, &h->dn);
  if (rc) {
    h->err = std::string("direct solver: ") + pgx_dn_last_error(nullptr);
    h->dn = nullptr;
    return rc;
  }
  MXALLOC(h->cdu, (size_t)nc * nk);
  MXALLOC(h->cdp, (size_t)nc * nk1);
  MXALLOC(h->tabU, (size_t)nk * nq);
  MXALLOC(h->dU, (size_t)2 * nk * nq);
  MXALLOC(h->tabP, (size_t)nk1 * nq);
  MXALLOC(h->dP, (size_t)2 * nk1 * nq);
  MXALLOC(h->geo, (size_t)nc * 5);
  MXALLOC(h->qw, nq);
  MXALLOC(h->lnrho, (size_t)nc * nq);
  MXALLOC(h->uex, (size_t)nc * nq);
  MXALLOC(h->isbc, nu);
  MXALLOC(h->gv, nu);
  MXALLOC(h->stash, (size_t)nc * std::max<size_t>(Wj, (size_t)Wr));
  MXALLOC(h->rowptr, ntot + 1);
  MXALLOC(h->col, tot);
  MXALLOC(h->Jc, tot);
  MXALLOC(h->Jv, tot);
  if ((rc = mx_alloc_state(h))) return rc;
#define MA_UP(dst, src, count) MXHIP(hipMemcpy(dst, src, sizeof(*(dst)) * (size_t)(count), hipMemcpyHostToDevice))
  MA_UP(h->cdu, pr->cell_dofs_u, (size_t)nc * nk);
  MA_UP(h->cdp, pr->cell_dofs_p, (size_t)nc * nk1);
  MA_UP(h->tabU, tU, (size_t)nk * nq);
  MA_UP(h->dU, gU, (size_t)2 * nk * nq);
  MA_UP(h->tabP, tP, (size_t)nk1 * nq);
  MA_UP(h->dP, gP, (size_t)2 * nk1 * nq);
  MA_UP(h->geo, geo.data(), (size_t)nc * 5);
  MA_UP(h->qw, pr->qwts, nq);
  MA_UP(h->lnrho, pr->ln_rho, (size_t)nc * nq);
  MA_UP(h->isbc, isbc.data(), nu);
  MA_UP(h->gv, gv.data(), nu);
  MA_UP(h->rowptr, rowptr.data(), ntot + 1);
  MA_UP(h->col, col.data(), tot);
  MA_UP(h->Jc, Jc.data(), tot);
#undef MA_UP
  MXHIP(hipMemsetAsync(h->Jv, 0, sizeof(double) * tot, h->st));
  std::string e1 = pgx_scatter_build(dr.data(), (int64_t)nc * Wr, ntot, h->allocs, &h->sc_res);
  if (e1.empty()) e1 = pgx_scatter_build(dj.data(), (int64_t)nc * (int64_t)Wj, tot, h->allocs, &h->sc_jac);
  if (e1.empty()) e1 = pgx_scatter_build(djt.data(), (int64_t)nc * (int64_t)Wj, tot, h->allocs, &h->sc_jac_t);
  if (!e1.empty()) {
    h->err = e1;
    return PGX_ENOMEM;
  }
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}

extern "C" int pgx_ma_create(const pgx_ma_problem* p, int device, pgx_ma_handle** out) {
  if (!p || !out || p->nv < 3 || p->nc < 1 || !p->coords || !p->cells || p->degree < 2 || p->nu < 1 || p->np < 1 || !p->cell_dofs_u ||
      !p->cell_dofs_p || p->nq < 1 || !p->qwts || !p->tab_u || !p->dtab_u || !p->tab_p || !p->dtab_p || !p->ln_rho || p->n_bc < 0 ||
      (p->n_bc > 0 && (!p->bc_dofs || !p->g))) {
    g_ma_error = "pgx_ma_create: bad arguments (degree >= 2, a mesh, both numberings, a rule with its four tables, ln rho)";
    return PGX_EINVAL;
  }
  return mx_create("pgx_ma_create", g_ma_error, device, out, [&](pgx_ma_handle* h) { return ma_create_impl(h, p); });
}

extern "C" int pgx_ma_num_dofs(const pgx_ma_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_ma_set_state(pgx_ma_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_ma_get_state(pgx_ma_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_ma_residual(pgx_ma_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_ma_jacobian_fill(pgx_ma_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_ma_csr_export(pgx_ma_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_ma_spmv(pgx_ma_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
extern "C" int pgx_ma_newton_solve(pgx_ma_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its) {
  return mx_newton(h, opts, reason, its, lin_its, true);
}
extern "C" int pgx_ma_profile(pgx_ma_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

extern "C" int pgx_ma_l2_error(pgx_ma_handle* h, const double* u_exact_at_qp, double* out) {
  MXNEED(h);
  if (!u_exact_at_qp || !out) return PGX_EINVAL;
  MXHIP(hipMemcpyAsync(h->uex, u_exact_at_qp, sizeof(double) * (size_t)h->nc * h->nq, hipMemcpyHostToDevice, h->st));
  const size_t lds = sizeof(double) * ((size_t)h->nk + MA_BLOCK);
  hipLaunchKernelGGL(k_ma_l2, dim3(MX_RED), dim3(MA_BLOCK), lds, h->st, h->nc, h->nk, h->nq, h->cdu, h->tabU, h->geo, h->qw, h->uex, h->x,
                     h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_ma_lu_stats(const pgx_ma_handle* h, pgx_dn_stats* st) { return h && h->dn ? pgx_dn_get_stats(h->dn, st) : PGX_EINVAL; }
