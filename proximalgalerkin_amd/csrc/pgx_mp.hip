// pgx_mp.hip - example 04 (four-phase Cahn-Hilliard gradient flow: u, z, psi in P1^4) behind the C ABI of include/pgx_mp.h.
// Reference: examples/04_multiphase/multiphase_dolfinx.py (:33-50 spaces, :52-87 residual, :127-147 solver, :188-233 loop).
// x = [u | z | psi], each block vertex-major with the 4 species fastest; rows [v | y | w].  The blocks (v,u) M, (v,z) -tau K,
// (y,u) alpha (K_eps - 2 M), (y,z) alpha M, (y,psi) M, (w,u) M are diagonal in the species, (w,psi) couples them; the mixed
// CSR stores these plus the species diagonals of the zero blocks (v,psi) and (w,z), which the sparse LU needs for a
// structurally symmetric pattern.  M, K and the epsilon^2-weighted K_eps are assembled once on the scalar P1
// pattern; the constant and alpha-dependent entries are recombined only when alpha changes, every Newton step re-assembles
// the (w,psi) block - the only one that depends on the iterate.  Polynomial terms (degree <= 2) are integrated exactly in
// closed form; the softmax term with the degree-7 rule the caller passes (UFL's estimate for it, tri_deg7_gj16).
#include <cstring>

#include "../../include/pgx_mp.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"
#include "pgx_tri.h"

#define MP_MAXQ 16
#define MP_NS 4
using MpQuad = TriQuad<MP_MAXQ>;

static thread_local std::string g_mp_error;

struct pgx_mp_handle : MixedBase {
  int nv = 0, nc = 0;
  MpQuad Q{};
  double tau = 1e-5, eps = 1e-9;
  double alpha_J = -1.0;  // alpha the constant part of Jv was recombined with (< 0: never)
  double* coords = nullptr;
  int32_t* cells = nullptr;
  double* uprev = nullptr;  // [4 nv] u of the previous time step
  double* wv = nullptr;     // [nv] int phi_v (species mass weights)
  double* mass = nullptr;   // [4]
  // deterministic assembly (pgx_scatter.h): residual 36 slots per cell -> dofs; (w,psi) block 144 slots per cell -> CSR
  PgxScatter sc_res, sc_w;
  double* stash = nullptr;  // [144 nc]
  double* Sc = nullptr;     // [3 nnz_s] scalar M | K | K_eps on the P1 pattern
  uint8_t* kind = nullptr;
  int32_t* src = nullptr;   // scalar-pattern index of every mixed entry
  pgx_mp_handle() : MixedBase("pgx_mp") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

extern "C" const char* pgx_mp_last_error(const pgx_mp_handle* h) { return h ? h->err.c_str() : g_mp_error.c_str(); }

struct MpGeom : TriGeom {
  double epsh2;  // epsilon^2 = (2 h)^2, h = 2 Circumradius (:53-54)
};
__device__ inline MpGeom mp_geom(const double* __restrict__ coords, const int32_t* __restrict__ cv) {
  double X[3][2];
  MpGeom g{tri_geom(coords, cv, X), 0.0};
  double e[3];
  for (int k = 0; k < 3; ++k) {
    const double dx = X[(k + 1) % 3][0] - X[(k + 2) % 3][0], dy = X[(k + 1) % 3][1] - X[(k + 2) % 3][1];
    e[k] = sqrt(dx * dx + dy * dy);
  }
  const double R = e[0] * e[1] * e[2] / (4.0 * (0.5 * g.adet));
  g.epsh2 = (4.0 * R) * (4.0 * R);
  return g;
}
// softmax of the species at one quadrature point, shifted by the maximum: finite for every finite psi
__device__ inline void mp_softmax(const double p[3][MP_NS], const double N[3], double S[MP_NS]) {
  double pq[MP_NS], mx = -INFINITY;
  for (int m = 0; m < MP_NS; ++m) {
    pq[m] = N[0] * p[0][m] + N[1] * p[1][m] + N[2] * p[2][m];
    mx = fmax(mx, pq[m]);
  }
  double s = 0.0;
  for (int m = 0; m < MP_NS; ++m) s += (S[m] = exp(pq[m] - mx));
  for (int m = 0; m < MP_NS; ++m) S[m] /= s;
}

__global__ __launch_bounds__(128) void k_mp_residual(int nc, int nv, const int32_t* __restrict__ cells,
                                                     const double* __restrict__ coords, const double* __restrict__ x,
                                                     const double* __restrict__ xk, const double* __restrict__ uprev,
                                                     double alpha, double tau, double eps, MpQuad Q, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cv = cells + 3 * (size_t)c;
  const MpGeom g = mp_geom(coords, cv);
  const size_t n = (size_t)MP_NS * nv;
  double u[3][MP_NS], z[3][MP_NS], p[3][MP_NS], dp[3][MP_NS], du[3][MP_NS];
  for (int a = 0; a < 3; ++a)
    for (int m = 0; m < MP_NS; ++m) {
      const size_t i = (size_t)MP_NS * cv[a] + m;
      u[a][m] = x[i], z[a][m] = x[n + i], p[a][m] = x[2 * n + i];
      dp[a][m] = p[a][m] - xk[2 * n + i];
      du[a][m] = u[a][m] - uprev[i];
    }
  const double area = 0.5 * g.adet;
  double Ke[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Ke[a][b] = area * (g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1]);
  double Rv[3][MP_NS], Ry[3][MP_NS], Rw[3][MP_NS];
  for (int a = 0; a < 3; ++a)
    for (int m = 0; m < MP_NS; ++m) {
      double mu = 0, mdu = 0, mz = 0, mp = 0, mdp = 0, kz = 0, ku = 0;
      for (int b = 0; b < 3; ++b) {
        const double me = tri_me(area, a, b);
        mu += me * u[b][m], mdu += me * du[b][m], mz += me * z[b][m], mp += me * p[b][m], mdp += me * dp[b][m];
        kz += Ke[a][b] * z[b][m], ku += Ke[a][b] * u[b][m];
      }
      Rv[a][m] = mdu - tau * kz;                                                          // EQ 2 (:76-79)
      Ry[a][m] = alpha * mz + alpha * g.epsh2 * ku - 2.0 * alpha * mu + mdp - alpha * area / 3.0;  // EQ 1 (:62-69)
      Rw[a][m] = mu - eps * mp;                                                           // EQ 3 (:81-87), polynomial part
    }
  for (int q = 0; q < Q.nq; ++q) {
    double S[MP_NS];
    mp_softmax(p, Q.N[q], S);
    const double wd = Q.w[q] * g.adet;
    for (int a = 0; a < 3; ++a)
      for (int m = 0; m < MP_NS; ++m) Rw[a][m] -= wd * S[m] * Q.N[q][a];
  }
  for (int a = 0; a < 3; ++a)  // parked slot-major: slot = block * 12 + a * 4 + m
    for (int m = 0; m < MP_NS; ++m) {
      stash[(size_t)(a * MP_NS + m) * nc + c] = Rv[a][m];
      stash[(size_t)(12 + a * MP_NS + m) * nc + c] = Ry[a][m];
      stash[(size_t)(24 + a * MP_NS + m) * nc + c] = Rw[a][m];
    }
}

// scalar M, K, K_eps once: stash[(k * 9 + a * 3 + b) * nc + cell], k = 0 M, 1 K, 2 epsilon^2 K
__global__ __launch_bounds__(128) void k_mp_const(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                  double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const MpGeom g = mp_geom(coords, cells + 3 * (size_t)c);
  const double area = 0.5 * g.adet;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double k = area * (g.G[a][0] * g.G[b][0] + g.G[a][1] * g.G[b][1]);
      stash[(size_t)(a * 3 + b) * nc + c] = tri_me(area, a, b);
      stash[(size_t)(9 + a * 3 + b) * nc + c] = k;
      stash[(size_t)(18 + a * 3 + b) * nc + c] = g.epsh2 * k;
    }
}

// kind: 0 = M, 1 = -tau K, 2 = alpha K_eps - 2 alpha M, 3 = alpha M, 4 = (w,psi): left to k_mp_jac_w, 5 = structural zero
__global__ void k_mp_recombine(int64_t nnz, int64_t nnz_s, const uint8_t* __restrict__ kind, const int32_t* __restrict__ src,
                               const double* __restrict__ Sc, double alpha, double tau, double* __restrict__ Jv) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int t = kind[k];
  if (t == 4) return;
  const int64_t s = src[k];
  const double M = Sc[s], K = Sc[nnz_s + s], KE = Sc[2 * nnz_s + s];
  Jv[k] = t == 0 ? M : t == 1 ? -tau * K : t == 2 ? alpha * KE - 2.0 * alpha * M : t == 3 ? alpha * M : 0.0;
}

// (w,psi): -int S_m (delta_mn - S_n) phi_a phi_b - eps M_ab delta_mn; one thread per (cell, a, b), 16 slots each:
// stash[((a * 4 + m) * 12 + b * 4 + n) * nc + cell]
__global__ __launch_bounds__(128) void k_mp_jac_w(int nc, int nv, const int32_t* __restrict__ cells,
                                                  const double* __restrict__ coords, const double* __restrict__ x, double eps,
                                                  MpQuad Q, double* __restrict__ stash) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 9 * (int64_t)nc) return;
  const int c = (int)(t / 9), a = (int)(t % 9) / 3, b = (int)(t % 3);
  const int32_t* cv = cells + 3 * (size_t)c;
  const MpGeom g = mp_geom(coords, cv);
  const size_t n = (size_t)MP_NS * nv;
  double p[3][MP_NS];
  for (int e = 0; e < 3; ++e)
    for (int m = 0; m < MP_NS; ++m) p[e][m] = x[2 * n + (size_t)MP_NS * cv[e] + m];
  double J[MP_NS][MP_NS];
  for (int m = 0; m < MP_NS; ++m)
    for (int k = 0; k < MP_NS; ++k) J[m][k] = 0.0;
  for (int q = 0; q < Q.nq; ++q) {
    double S[MP_NS];
    mp_softmax(p, Q.N[q], S);
    const double wd = Q.w[q] * g.adet * Q.N[q][a] * Q.N[q][b];
    for (int m = 0; m < MP_NS; ++m)
      for (int k = 0; k < MP_NS; ++k) J[m][k] -= wd * ((m == k ? S[m] : 0.0) - S[m] * S[k]);
  }
  const double em = eps * tri_me(0.5 * g.adet, a, b);
  for (int m = 0; m < MP_NS; ++m)
    for (int k = 0; k < MP_NS; ++k)
      stash[(size_t)((a * MP_NS + m) * 12 + b * MP_NS + k) * nc + c] = m == k ? J[m][k] - em : J[m][k];
}

// begin of a time step (:194-200): psi of x and of the previous iterate <- ln(|u(x)| + 1e-7) + 1, u of the previous iterate <- 0
__global__ void k_mp_begin(int64_t n, double* __restrict__ x, double* __restrict__ xk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = log(fabs(x[i]) + 1e-7) + 1.0;
  x[2 * n + i] = v;
  xk[2 * n + i] = v;
  xk[i] = 0.0;
}

// sum over cells of d^T M_e d per species, d = u(x) - u(xk): per-block partials
__global__ __launch_bounds__(256) void k_mp_l2(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                               const double* __restrict__ x, const double* __restrict__ xk,
                                               double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += MX_RED * 256) {
    const int32_t* cv = cells + 3 * (size_t)c;
    const MpGeom g = mp_geom(coords, cv);
    const double area = 0.5 * g.adet;
    for (int m = 0; m < MP_NS; ++m) {
      double d[3];
      for (int a = 0; a < 3; ++a) d[a] = x[(size_t)MP_NS * cv[a] + m] - xk[(size_t)MP_NS * cv[a] + m];
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

// int u_m = sum_v (int phi_v) u[v, m]: block m, fixed order
__global__ __launch_bounds__(256) void k_mp_mass(int nv, const double* __restrict__ wv, const double* __restrict__ x,
                                                 double* __restrict__ out) {
  __shared__ double sh[256];
  const int m = blockIdx.x;
  double s = 0.0;
  for (int v = threadIdx.x; v < nv; v += 256) s += wv[v] * x[(size_t)MP_NS * v + m];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[m] = sh[0];
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" void pgx_mp_destroy(pgx_mp_handle* h) { mx_destroy(h); }

void pgx_mp_handle::residual_dev(const double* xin, double* Fout) {
  pgx_mp_handle* h = this;
  MxTimer t(h, 0);
  hipMemsetAsync(Fout, 0, sizeof(double) * h->ntot, h->st);
  hipLaunchKernelGGL(k_mp_residual, dim3((h->nc + 127) / 128), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, xin, h->xk,
                     h->uprev, h->alpha, h->tau, h->eps, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_res, h->stash, 1.0, 0, Fout);
}
void pgx_mp_handle::jacobian_dev(const double* xin) {
  pgx_mp_handle* h = this;
  MxTimer t(h, 1);
  if (h->alpha_J != h->alpha) {  // the constant and alpha-dependent blocks change only with alpha
    const int64_t nnz_s = h->nnz / 48;
    hipLaunchKernelGGL(k_mp_recombine, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->st, h->nnz, nnz_s, h->kind,
                       h->src, h->Sc, h->alpha, h->tau, h->Jv);
    h->alpha_J = h->alpha;
  }
  const int64_t nt = 9 * (int64_t)h->nc;
  hipLaunchKernelGGL(k_mp_jac_w, dim3((unsigned)((nt + 127) / 128)), dim3(128), 0, h->st, h->nc, h->nv, h->cells, h->coords, xin,
                     h->eps, h->Q, h->stash);
  pgx_scatter_run(h->st, h->sc_w, h->stash, 1.0, 0, h->Jv);
  h->jac_valid = true;
}

static int mp_create_impl(pgx_mp_handle* h, const pgx_mesh* m, const pgx_mp_problem* p) {
  const int nv = m->n_vertices, nc = m->n_cells;
  const int64_t nb = (int64_t)MP_NS * nv, ntot = 3 * nb;
  h->nv = nv, h->nc = nc, h->ntot = ntot;
  h->tau = p->tau, h->eps = p->eps;
  h->Q.fill(p->qpts, p->qwts, p->nq);
  if (const char* e = check_cells(m->cells, 3, nc, nv)) {
    h->err = e;
    return PGX_EINVAL;
  }
  std::vector<double> hwv(nv, 0.0);
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
    for (int a = 0; a < 3; ++a) hwv[cv[a]] += 0.5 * std::fabs(det) / 3.0;
  }
  // scalar P1 pattern (vertex adjacency incl. self)
  std::vector<int32_t> sptr, scol;
  p1_adjacency(nv, nc, m->cells, false, sptr, scol);  // false, as this family always had it: a vertex of no cell has empty rows
  const int64_t nnz_s = sptr[nv];
  // per vertex pair and species: v and y rows 3 entries (u, z, psi), w rows 2 + 4 (u, z, psi of every species)
  if (48 * nnz_s > 0x7fffffff) {
    h->err = "mixed matrix exceeds int32 nnz";
    return PGX_EINVAL;
  }
  const int64_t tot = 48 * nnz_s;
  h->nnz = tot;
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  rowptr.assign(ntot + 1, 0);
  col.resize(tot);
  std::vector<uint8_t> kind(tot);
  std::vector<int32_t> src(tot);
  static const int row_len[3] = {3, 3, 6};
  for (int fr = 0; fr < 3; ++fr)
    for (int v = 0; v < nv; ++v)
      for (int s = 0; s < MP_NS; ++s) rowptr[fr * nb + (int64_t)MP_NS * v + s + 1] = row_len[fr] * (sptr[v + 1] - sptr[v]);
  for (int64_t r = 0; r < ntot; ++r) rowptr[r + 1] += rowptr[r];
  mx_par_for(nv, [&](int64_t a0, int64_t b0) {
    for (int64_t v = a0; v < b0; ++v) {
      const int len = sptr[v + 1] - sptr[v];
      for (int fr = 0; fr < 3; ++fr)
        for (int s = 0; s < MP_NS; ++s) {
          int64_t e = rowptr[fr * nb + MP_NS * v + s];
          auto put = [&](int fc, int k, int sp, uint8_t t) {
            col[e] = (int32_t)(fc * nb + (int64_t)MP_NS * scol[sptr[v] + k] + sp);
            kind[e] = t;
            src[e] = sptr[v] + k;
            ++e;
          };
          if (fr == 0) {
            for (int k = 0; k < len; ++k) put(0, k, s, 0);  // (v,u) M
            for (int k = 0; k < len; ++k) put(1, k, s, 1);  // (v,z) -tau K
            for (int k = 0; k < len; ++k) put(2, k, s, 5);  // (v,psi) zero
          } else if (fr == 1) {
            for (int k = 0; k < len; ++k) put(0, k, s, 2);  // (y,u) alpha (K_eps - 2 M)
            for (int k = 0; k < len; ++k) put(1, k, s, 3);  // (y,z) alpha M
            for (int k = 0; k < len; ++k) put(2, k, s, 0);  // (y,psi) M
          } else {
            for (int k = 0; k < len; ++k) put(0, k, s, 0);  // (w,u) M
            for (int k = 0; k < len; ++k) put(1, k, s, 5);  // (w,z) zero
            for (int k = 0; k < len; ++k)
              for (int n = 0; n < MP_NS; ++n) put(2, k, n, 4);  // (w,psi)
          }
        }
    }
  });
  // destination tables, slot-major like the stashes: table[slot * nc + cell]
  std::vector<int32_t> d36((size_t)nc * 36), d144((size_t)nc * 144), d27((size_t)nc * 27);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    for (int64_t c = a0; c < b0; ++c) {
      const int32_t* cv = m->cells + 3 * (size_t)c;
      for (int a = 0; a < 3; ++a) {
        const int v = cv[a], len = sptr[v + 1] - sptr[v];
        const int32_t* sb = scol.data() + sptr[v];
        for (int s = 0; s < MP_NS; ++s)
          for (int blk = 0; blk < 3; ++blk) d36[(size_t)(blk * 12 + a * MP_NS + s) * nc + c] = (int32_t)(blk * nb + (int64_t)MP_NS * v + s);
        for (int b = 0; b < 3; ++b) {
          const int k = (int)(std::lower_bound(sb, sb + len, cv[b]) - sb);
          for (int blk = 0; blk < 3; ++blk) d27[(size_t)(blk * 9 + a * 3 + b) * nc + c] = (int32_t)(blk * nnz_s + sptr[v] + k);
          for (int s = 0; s < MP_NS; ++s)
            for (int n = 0; n < MP_NS; ++n)
              d144[(size_t)((a * MP_NS + s) * 12 + b * MP_NS + n) * nc + c] =
                  (int32_t)(rowptr[2 * nb + (int64_t)MP_NS * v + s] + 2 * len + MP_NS * k + n);
        }
      }
    }
  });
  std::vector<int32_t> nod(ntot);
  for (int64_t i = 0; i < ntot; ++i) nod[i] = (int32_t)((i % nb) / MP_NS);
  MXHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, nv, nod.data(), 2, m->coords);
  if (rc) return rc;
  MXALLOC(h->coords, 2 * (size_t)nv);
  MXALLOC(h->cells, 3 * (size_t)nc);
  MXALLOC(h->uprev, nb);
  MXALLOC(h->wv, nv);
  MXALLOC(h->mass, MP_NS);
  MXALLOC(h->stash, 144 * (size_t)nc);
  MXALLOC(h->Sc, 3 * nnz_s);
  MXALLOC(h->kind, tot);
  MXALLOC(h->src, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  MXHIP(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->cells, m->cells, sizeof(int32_t) * 3 * (size_t)nc, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->wv, hwv.data(), sizeof(double) * nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->src, src.data(), sizeof(int32_t) * tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->uprev, 0, sizeof(double) * nb, h->st));
  MXHIP(hipMemsetAsync(h->Jv, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->Sc, 0, sizeof(double) * 3 * nnz_s, h->st));
  {
    std::string e1 = pgx_scatter_build(d36.data(), (int64_t)36 * nc, ntot, h->allocs, &h->sc_res);
    if (e1.empty()) e1 = pgx_scatter_build(d144.data(), (int64_t)144 * nc, tot, h->allocs, &h->sc_w);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  // scalar M, K, K_eps, once: the stash is the handle's
  return mx_scatter_once(h, d27.data(), 27, nc, 3 * nnz_s, h->stash, [&](double* stash) {
    hipLaunchKernelGGL(k_mp_const, dim3((nc + 127) / 128), dim3(128), 0, h->st, nc, h->cells, h->coords, stash);
  }, h->Sc, 0);
}

extern "C" int pgx_mp_create(const pgx_mesh* m, const pgx_mp_problem* p, int device, pgx_mp_handle** out) {
  if (!m || !p || !out || !m->coords || !m->cells || m->n_vertices <= 0 || m->n_cells <= 0 || !p->qpts || !p->qwts || p->nq <= 0 ||
      p->nq > MP_MAXQ || !(p->tau > 0.0) || !(p->eps >= 0.0)) {
    g_mp_error = "pgx_mp_create: bad arguments";
    return PGX_EINVAL;
  }
  return mx_create("pgx_mp_create", g_mp_error, device, out, [&](pgx_mp_handle* h) { return mp_create_impl(h, m, p); });
}

extern "C" int pgx_mp_num_dofs(const pgx_mp_handle* h, int64_t* ntot) {
  if (!h || !ntot) return PGX_EINVAL;
  *ntot = h->ntot;
  return PGX_OK;
}
extern "C" int pgx_mp_set_state(pgx_mp_handle* h, const double* x) { return mx_set_state(h, x); }
extern "C" int pgx_mp_get_state(pgx_mp_handle* h, double* x) { return mx_get_state(h, x); }
extern "C" int pgx_mp_set_prev(pgx_mp_handle* h, const double* x) { return mx_set_prev(h, x); }
extern "C" int pgx_mp_get_prev(pgx_mp_handle* h, double* x) { return mx_get_prev(h, x); }
extern "C" int pgx_mp_advance_prev(pgx_mp_handle* h) { return mx_advance_prev(h); }
extern "C" int pgx_mp_set_alpha(pgx_mp_handle* h, double a) { return mx_set_alpha(h, a); }
extern "C" int pgx_mp_residual(pgx_mp_handle* h, const double* x, double* F, double* fnorm) { return mx_residual(h, x, F, fnorm); }
extern "C" int pgx_mp_jacobian_fill(pgx_mp_handle* h, const double* x) { return mx_jacobian_fill(h, x); }
extern "C" int pgx_mp_csr_export(pgx_mp_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals) {
  return mx_csr_export(h, nrows, nnz, rowptr, col, vals);
}
extern "C" int pgx_mp_spmv(pgx_mp_handle* h, const double* x, double* y) { return mx_spmv(h, x, y); }
// linesearch 3: bt of order 3 (the reference's default), 1: bt of order 2, every other value: plain Newton
extern "C" int pgx_mp_newton_solve(pgx_mp_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its) {
  return mx_newton(h, opts, reason, its, lin_its, false);
}
extern "C" int pgx_mp_profile(pgx_mp_handle* h, int enable, double ms[6]) { return mx_profile(h, enable, ms); }

extern "C" int pgx_mp_set_uprev(pgx_mp_handle* h, const double* u) {
  MXNEED(h);
  return mx_in(h, h->uprev, u, (int64_t)MP_NS * h->nv);
}
extern "C" int pgx_mp_get_uprev(pgx_mp_handle* h, double* u) {
  MXNEED(h);
  if (!u) return PGX_EINVAL;
  MXHIP(hipMemcpyAsync(u, h->uprev, sizeof(double) * MP_NS * (size_t)h->nv, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_mp_begin_step(pgx_mp_handle* h) {
  MXNEED(h);
  const int64_t n = (int64_t)MP_NS * h->nv;
  hipLaunchKernelGGL(k_mp_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, n, h->x, h->xk);
  MXHIP(hipStreamSynchronize(h->st));
  MXHIP(hipGetLastError());
  return PGX_OK;
}
extern "C" int pgx_mp_end_step(pgx_mp_handle* h) {
  MXNEED(h);
  MXHIP(hipMemcpyAsync(h->uprev, h->x, sizeof(double) * MP_NS * (size_t)h->nv, hipMemcpyDeviceToDevice, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_mp_l2_increment(pgx_mp_handle* h, double* out) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_mp_l2, dim3(MX_RED), dim3(256), 0, h->st, h->nc, h->cells, h->coords, h->x, h->xk, h->partials);
  return mx_partials_sqrt(h, out);
}
extern "C" int pgx_mp_species_mass(pgx_mp_handle* h, double out[4]) {
  MXNEED(h);
  if (!out) return PGX_EINVAL;
  hipLaunchKernelGGL(k_mp_mass, dim3(MP_NS), dim3(256), 0, h->st, h->nv, h->wv, h->x, h->mass);
  MXHIP(hipMemcpyAsync(out, h->mass, sizeof(double) * MP_NS, hipMemcpyDeviceToHost, h->st));
  MXHIP(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_mp_lu_stats(const pgx_mp_handle* h, pgx_nd_stats* st) { return h ? pgx_nd_get_stats(h->lu, st) : PGX_EINVAL; }
