// pgx_sg2d.hip - example 02 in the plane (signorini_dolfinx.py with gdim = 2: `native --dim 2`, the half disk of
// lvpp.mesh_generation.create_half_disk) behind pgx_sg_create_2d of include/pgx_sg.h: the ELEMENT layer - 2 x 2 elasticity blocks
// on triangles / parallelograms, the mass coupling and the exp terms on contact EDGES, the diagnostics.  The handle, the residual
// row pass, the Jacobian initialisation, the SNES mirror and the sparse LU are those of pgx_sg.hip / pgx_mixed.hip, unchanged.
//
// x = [u_x | u_y | psi], n_g = -e_y, g = y - gap.  As in 3-D everything that does not depend on the iterate is assembled ONCE into
// Jc; per Newton step only k_sg2_exp runs (one thread per contact edge) next to the shared kernels.
#include <cstring>

#include "pgx_sg_internal.h"

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
// elasticity block, once: A_e[(A,i),(B,j)] = |det J| sum_q w_q (lambda dN_A,i dN_B,j + mu dN_A,j dN_B,i + mu delta_ij dN_A . dN_B), i, j < 2,
// lambda and mu the 3-D (plane-strain) constants of the script.  tab = [nq weights | nq x NPC x 2 reference gradients]; geometry from
// the three local nodes (origin, +xi, +eta) of the affine cell.  One thread per cell, 4 NPC^2 values parked slot-major.
template <int NPC>
__global__ __launch_bounds__(64) void k_sg2_const_cells(int nc, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                        double mu, double lmbda, int nq, const double* __restrict__ tab, int g0, int g1,
                                                        int g2, double* __restrict__ stash) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int32_t* cv = cells + NPC * (size_t)c;
  const int gn[3] = {g0, g1, g2};
  double X[3][2];
  for (int a = 0; a < 3; ++a)
    for (int d = 0; d < 2; ++d) X[a][d] = coords[2 * (size_t)cv[gn[a]] + d];
  const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0], J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];  // columns = edge vectors
  const double det = J00 * J11 - J01 * J10;
  const double inv[2][2] = {{J11 / det, -J01 / det}, {-J10 / det, J00 / det}};  // d xi_k / d x_d
  const double adet = fabs(det);
  const double* dN = tab + nq;
  constexpr int ND = 2 * NPC;
  for (int A = 0; A < NPC; ++A)
    for (int B = 0; B < NPC; ++B) {
      double acc[2][2] = {{0, 0}, {0, 0}};
      for (int q = 0; q < nq; ++q) {
        const double* ra = dN + ((size_t)q * NPC + A) * 2;
        const double* rb = dN + ((size_t)q * NPC + B) * 2;
        double gA[2], gB[2];
        for (int d = 0; d < 2; ++d) {
          gA[d] = ra[0] * inv[0][d] + ra[1] * inv[1][d];
          gB[d] = rb[0] * inv[0][d] + rb[1] * inv[1][d];
        }
        const double wq = tab[q] * adet;
        const double gg = gA[0] * gB[0] + gA[1] * gB[1];
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j) acc[i][j] += wq * (lmbda * gA[i] * gB[j] + mu * gA[j] * gB[i] + (i == j ? mu * gg : 0.0));
      }
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) stash[(size_t)((A * 2 + i) * ND + (B * 2 + j)) * nc + c] = acc[i][j];
    }
}

// edge mass coupling (+M on (u_y, psi), -M on (psi, u_y)) and b_g = <g, w>, once; the edge length is the surface element
template <int NPE>
__global__ __launch_bounds__(128) void k_sg2_const_edges(int nf, const int32_t* __restrict__ facets, const double* __restrict__ coords,
                                                         double gap, SgQuad1 Q,
                                                         double* __restrict__ stash /* [(2 NPE^2 + NPE) * nf]: matrix slots, then b_g */) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int32_t* fv = facets + NPE * (size_t)f;
  const double x0 = coords[2 * (size_t)fv[0]], y0 = coords[2 * (size_t)fv[0] + 1];
  const double x1 = coords[2 * (size_t)fv[Q.e1]], y1 = coords[2 * (size_t)fv[Q.e1] + 1];
  const double len = sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
  double Me[NPE][NPE], g[NPE];
  for (int a = 0; a < NPE; ++a) {
    g[a] = 0.0;
    for (int b = 0; b < NPE; ++b) Me[a][b] = 0.0;
  }
  for (int q = 0; q < Q.nq; ++q) {
    const double wd = Q.w[q] * len;
    const double yq = y0 + Q.t[q] * (y1 - y0);
    for (int a = 0; a < NPE; ++a) {
      g[a] += wd * (yq - gap) * Q.N[q][a];
      for (int b = 0; b < NPE; ++b) Me[a][b] += wd * Q.N[q][a] * Q.N[q][b];
    }
  }
  for (int a = 0; a < NPE; ++a) {
    stash[(size_t)(2 * NPE * NPE + a) * nf + f] = g[a];
    for (int b = 0; b < NPE; ++b) {
      stash[(size_t)(a * NPE + b) * nf + f] = Me[a][b];                // row u_y(a), col psi(b)
      stash[(size_t)(NPE * NPE + a * NPE + b) * nf + f] = -Me[a][b];  // row psi(a), col u_y(b)
    }
  }
}

// per Newton step: parks (mode 0) D_e[a][b] = <exp(psi) N_a, N_b> for the Jacobian, (mode 1) b_exp[a] = <exp(psi), N_a> for the residual
template <int NPE>
__global__ __launch_bounds__(128) void k_sg2_exp(int mode, int nf, int nu, const int32_t* __restrict__ facets,
                                                 const int32_t* __restrict__ fpsi, const double* __restrict__ coords,
                                                 const double* __restrict__ x, SgQuad1 Q, double* __restrict__ stash) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int32_t* fv = facets + NPE * (size_t)f;
  const int32_t* fp = fpsi + NPE * (size_t)f;
  const double ex = coords[2 * (size_t)fv[Q.e1]] - coords[2 * (size_t)fv[0]];
  const double ey = coords[2 * (size_t)fv[Q.e1] + 1] - coords[2 * (size_t)fv[0] + 1];
  const double len = sqrt(ex * ex + ey * ey);
  double pv[NPE], De[NPE][NPE], be[NPE];
#pragma unroll
  for (int a = 0; a < NPE; ++a) {
    pv[a] = x[nu + fp[a]];
    be[a] = 0.0;
#pragma unroll
    for (int b = 0; b < NPE; ++b) De[a][b] = 0.0;
  }
  for (int q = 0; q < Q.nq; ++q) {
    double pq = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) pq += pv[a] * Q.N[q][a];
    const double e = Q.w[q] * len * exp(pq);
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
      be[a] += e * Q.N[q][a];
#pragma unroll
      for (int b = 0; b < NPE; ++b) De[a][b] += e * Q.N[q][a] * Q.N[q][b];
    }
  }
  if (mode == 0) {
#pragma unroll
    for (int a = 0; a < NPE; ++a)
#pragma unroll
      for (int b = 0; b < NPE; ++b) stash[(size_t)(a * NPE + b) * nf + f] = De[a][b];
  } else {
#pragma unroll
    for (int a = 0; a < NPE; ++a) stash[(size_t)a * nf + f] = be[a];
  }
}

// int_Gamma max(u.n_g - g, 0)^2 ds with the edge rule of the residual: MX_RED per-block partial sums, fixed shape, no atomics
template <int NPE>
__global__ __launch_bounds__(256) void k_sg2_penetration(int nf, int nv, const int32_t* __restrict__ facets, const double* __restrict__ coords,
                                                         const double* __restrict__ x, double gap, SgQuad1 Q, double* __restrict__ partials) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int f = blockIdx.x * 256 + threadIdx.x; f < nf; f += MX_RED * 256) {
    const int32_t* fv = facets + NPE * (size_t)f;
    const double x0 = coords[2 * (size_t)fv[0]], y0 = coords[2 * (size_t)fv[0] + 1];
    const double x1 = coords[2 * (size_t)fv[Q.e1]], y1 = coords[2 * (size_t)fv[Q.e1] + 1];
    const double len = sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
    double uy[NPE];
#pragma unroll
    for (int a = 0; a < NPE; ++a) uy[a] = x[(size_t)nv + fv[a]];
    for (int q = 0; q < Q.nq; ++q) {
      double uq = 0.0;
#pragma unroll
      for (int a = 0; a < NPE; ++a) uq += uy[a] * Q.N[q][a];
      const double d = -uq - (y0 + Q.t[q] * (y1 - y0) - gap);  // u.n_g - g
      const double pen = d > 0.0 ? d : 0.0;
      s += Q.w[q] * len * pen * pen;
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

// u.n_g - g = -u_y - (y - gap) at every node
__global__ __launch_bounds__(256) void k_sg2_violation(int nv, const double* __restrict__ coords, const double* __restrict__ x, double gap,
                                                       double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  out[i] = -x[(size_t)nv + i] - (coords[2 * (size_t)i + 1] - gap);
}

// The script's von-Mises expression with len(u) = 2 (:300-301): s = sigma - tr(sigma)/3 I_2 with the 2 x 2 sigma, sqrt(3/2 s:s) - NOT the
// plane-strain von Mises (no sigma_zz).  At the cell's own nodes; tab[n][a][2] = reference gradient of basis function a at reference
// node n.  One thread per affine cell, values leave through LDS in contiguous runs.
template <int NPC>
__global__ __launch_bounds__(64) void k_sg2_von_mises(int nc, int nv, const int32_t* __restrict__ cells, const double* __restrict__ coords,
                                                      const double* __restrict__ x, double mu, double lmbda, const double* __restrict__ tab,
                                                      int g0, int g1, int g2, double* __restrict__ out) {
  __shared__ double tile[64 * NPC];
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c < nc) {
    const int32_t* cv = cells + NPC * (size_t)c;
    const int gn[3] = {g0, g1, g2};
    double X[3][2];
    for (int a = 0; a < 3; ++a)
      for (int d = 0; d < 2; ++d) X[a][d] = coords[2 * (size_t)cv[gn[a]] + d];
    const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0], J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
    const double det = J00 * J11 - J01 * J10;
    const double inv[2][2] = {{J11 / det, -J01 / det}, {-J10 / det, J00 / det}};
    double u[NPC][2];  // indexed by unrolled loops only: registers
#pragma unroll
    for (int a = 0; a < NPC; ++a)
#pragma unroll
      for (int i = 0; i < 2; ++i) u[a][i] = x[(size_t)i * nv + cv[a]];
    for (int n = 0; n < NPC; ++n) {
      const double* r = tab + (size_t)n * NPC * 2;
      double H[2][2] = {{0, 0}, {0, 0}};  // d u_i / d xi_k
#pragma unroll
      for (int a = 0; a < NPC; ++a)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int k = 0; k < 2; ++k) H[i][k] += u[a][i] * r[2 * a + k];
      double g[2][2];  // d u_i / d x_d
      for (int i = 0; i < 2; ++i)
        for (int d = 0; d < 2; ++d) g[i][d] = H[i][0] * inv[0][d] + H[i][1] * inv[1][d];
      const double tr = g[0][0] + g[1][1];
      double sg[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) sg[i][j] = mu * (g[i][j] + g[j][i]) + (i == j ? lmbda * tr : 0.0);
      const double m = (sg[0][0] + sg[1][1]) / 3.0;
      double ss = 0.0;
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
          const double v = sg[i][j] - (i == j ? m : 0.0);
          ss += v * v;
        }
      tile[threadIdx.x * NPC + n] = sqrt(1.5 * ss);
    }
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * 64 * NPC;
  const int cnt = min(64, nc - (int)blockIdx.x * 64) * NPC;
  for (int i = threadIdx.x; i < cnt; i += 64) out[base + i] = tile[i];
}

// ------------------------------------------------------------------------------------------------------------------
// host: launches behind the shared entry points
// ------------------------------------------------------------------------------------------------------------------
void sg2d_exp(pgx_sg_handle* h, int mode, const double* xin) {
  const dim3 g((h->nf + 127) / 128), b(128);
  if (h->npf == 3)
    hipLaunchKernelGGL(k_sg2_exp<3>, g, b, 0, h->st, mode, h->nf, 2 * h->nv, h->facets, h->fpsi, h->coords, xin, h->Q1, h->stash);
  else
    hipLaunchKernelGGL(k_sg2_exp<2>, g, b, 0, h->st, mode, h->nf, 2 * h->nv, h->facets, h->fpsi, h->coords, xin, h->Q1, h->stash);
}
void sg2d_penetration(pgx_sg_handle* h) {
  const dim3 g(MX_RED), b(256);
  if (h->npf == 3)
    hipLaunchKernelGGL(k_sg2_penetration<3>, g, b, 0, h->st, h->nf, h->nv, h->facets, h->coords, h->x, h->gap, h->Q1, h->partials);
  else
    hipLaunchKernelGGL(k_sg2_penetration<2>, g, b, 0, h->st, h->nf, h->nv, h->facets, h->coords, h->x, h->gap, h->Q1, h->partials);
}
void sg2d_violation(pgx_sg_handle* h, double* out) {
  hipLaunchKernelGGL(k_sg2_violation, dim3((h->nv + 255) / 256), dim3(256), 0, h->st, h->nv, h->coords, h->x, h->gap, out);
}
void sg2d_von_mises(pgx_sg_handle* h, double* out) {
  const dim3 g((h->nc + 63) / 64), b(64);
  const int* vg = h->vm_g;
#define SG2_VM(NPC) \
  hipLaunchKernelGGL(k_sg2_von_mises<NPC>, g, b, 0, h->st, h->nc, h->nv, h->cells, h->coords, h->x, h->mu, h->lmbda, h->vm_tab, vg[0], vg[1], vg[2], out)
  if (h->npc == 3)
    SG2_VM(3);
  else if (h->npc == 6)
    SG2_VM(6);
  else if (h->npc == 4)
    SG2_VM(4);
  else
    SG2_VM(9);
#undef SG2_VM
}

// reference gradients [NPC][2] of the cell basis at (X, Y): triangles - node order of include/pgx_sg.h (vertices, then the edges
// (0,1) (0,2) (1,2)), P1 = barycentric coordinates, P2 = L_a (2 L_a - 1) / 4 L_a L_b; quadrilaterals - tensor Lagrange, lexicographic
template <int NPC>
static void sg2_ref_grads(double X, double Y, double* r) {
  if (NPC == 3 || NPC == 6) {
    static const double gref[3][2] = {{-1, -1}, {1, 0}, {0, 1}};
    static const int ed[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    const double L[3] = {1.0 - X - Y, X, Y};
    for (int a = 0; a < 3; ++a)
      for (int d = 0; d < 2; ++d) r[2 * a + d] = (NPC == 3 ? 1.0 : 4.0 * L[a] - 1.0) * gref[a][d];
    for (int k = 0; k < (NPC == 6 ? 3 : 0); ++k)
      for (int d = 0; d < 2; ++d) r[2 * (3 + k) + d] = 4.0 * (L[ed[k][0]] * gref[ed[k][1]][d] + L[ed[k][1]] * gref[ed[k][0]][d]);
  } else {
    const int d = NPC == 4 ? 1 : 2, n1 = d + 1;
    double lx[3], ly[3], dx[3], dy[3];
    sg_lagrange1d(d, X, lx, dx);
    sg_lagrange1d(d, Y, ly, dy);
    for (int iy = 0; iy < n1; ++iy)
      for (int ix = 0; ix < n1; ++ix) r[2 * (iy * n1 + ix)] = dx[ix] * ly[iy], r[2 * (iy * n1 + ix) + 1] = lx[ix] * dy[iy];
  }
}

// NPC / NPE: nodes per cell / per contact edge: triangles 3 / 2 (degree 1), 6 / 3 (degree 2); quadrilaterals 4 / 2 (Q1), 9 / 3 (Q2)
template <int NPC, int NPE>
static int sg2_create_impl(pgx_sg_handle* h, const pgx_sg_mesh2d* m, const pgx_sg_problem2d* p) {
  constexpr int ND = 2 * NPC, NE = ND * ND, NF2 = NPE * NPE, NFS = 2 * NF2 + NPE;
  static_assert(ND <= PAT_MAX_ENTITY_DOFS && 2 * NPE <= PAT_MAX_ENTITY_DOFS, "an entity's dofs must fit the pattern builder's buffer");
  constexpr bool quad = NPC == 4 || NPC == 9;
  constexpr int deg = NPE - 1;
  const int nv = m->n_vertices, nc = m->n_cells, nf = m->n_facets;
  const int nu = 2 * nv;
  h->gdim = 2;
  h->npc = NPC, h->npf = NPE;
  h->nv = nv, h->nc = nc, h->nf = nf, h->nc_owned = nc;
  h->gap = p->gap;
  h->mu = p->E / (2.0 * (1.0 + p->nu));  // the script's constants (:234-235) whatever gdim: plane strain
  h->lmbda = p->E * p->nu / ((1.0 + p->nu) * (1.0 - 2.0 * p->nu));
  SgQuad1& Q = h->Q1;
  Q.nq = p->nq;
  Q.e1 = quad ? deg : 1;
  for (int q = 0; q < p->nq; ++q) {
    const double t = p->qpts[q];
    Q.t[q] = t, Q.w[q] = p->qwts[q];
    Q.N[q][0] = Q.N[q][1] = Q.N[q][2] = 0.0;
    if (NPE == 2)
      Q.N[q][0] = 1.0 - t, Q.N[q][1] = t;
    else if (quad) {
      double dummy[3];
      sg_lagrange1d(2, t, Q.N[q], dummy);
    } else  // (end, end, midpoint)
      Q.N[q][0] = (1.0 - t) * (1.0 - 2.0 * t), Q.N[q][1] = t * (2.0 * t - 1.0), Q.N[q][2] = 4.0 * t * (1.0 - t);
  }
  const int g0 = 0, g1 = quad ? deg : 1, g2 = quad ? deg * (deg + 1) : 2;
  h->vm_g[0] = g0, h->vm_g[1] = g1, h->vm_g[2] = g2, h->vm_g[3] = 0;
  if (const char* e = check_cells(m->cells, NPC, nc, nv)) {
    h->err = e;
    return PGX_EINVAL;
  }
  // reference positions of the local nodes; every cell must be the affine image of the reference cell (straight-sided triangles with
  // their edge nodes at the midpoints; parallelograms with their nodes on the lattice)
  double ref[NPC][2];
  if constexpr (quad) {
    for (int iy = 0; iy <= deg; ++iy)
      for (int ix = 0; ix <= deg; ++ix) ref[iy * (deg + 1) + ix][0] = (double)ix / deg, ref[iy * (deg + 1) + ix][1] = (double)iy / deg;
  } else {
    static const double vr[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    static const int ed[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int a = 0; a < 3; ++a) ref[a][0] = vr[a][0], ref[a][1] = vr[a][1];
    for (int k = 0; k < NPC - 3; ++k)
      for (int d = 0; d < 2; ++d) ref[3 + k][d] = 0.5 * (vr[ed[k][0]][d] + vr[ed[k][1]][d]);
  }
  for (int c = 0; c < nc; ++c) {
    const int32_t* cv = m->cells + NPC * (size_t)c;
    const double* X0 = m->coords + 2 * (size_t)cv[g0];
    const double* X1 = m->coords + 2 * (size_t)cv[g1];
    const double* X2 = m->coords + 2 * (size_t)cv[g2];
    const double e1[2] = {X1[0] - X0[0], X1[1] - X0[1]}, e2[2] = {X2[0] - X0[0], X2[1] - X0[1]};
    const double det = e1[0] * e2[1] - e1[1] * e2[0];
    const double diam2 = e1[0] * e1[0] + e1[1] * e1[1] + e2[0] * e2[0] + e2[1] * e2[1];
    if (!(fabs(det) > 1e-14 * diam2)) {
      h->err = "pgx_sg_create_2d: degenerate cell " + std::to_string(c);
      return PGX_EINVAL;
    }
    for (int a = 0; a < NPC; ++a) {
      const double* Xa = m->coords + 2 * (size_t)cv[a];
      const double dx = X0[0] + ref[a][0] * e1[0] + ref[a][1] * e2[0] - Xa[0], dy = X0[1] + ref[a][0] * e1[1] + ref[a][1] * e2[1] - Xa[1];
      if (!(dx * dx + dy * dy <= 1e-20 * diam2)) {
        h->err = std::string("pgx_sg_create_2d: cell ") + std::to_string(c) +
                 (quad ? " is not a parallelogram with its nodes on the lattice" : " is not a straight-sided triangle with its edge nodes at the midpoints") +
                 " (affine cells only)";
        return PGX_EINVAL;
      }
    }
  }
  // psi dofs = contact nodes ordered by node id
  std::vector<int32_t> v2psi(nv, -1);
  for (size_t k = 0; k < NPE * (size_t)nf; ++k) {
    if (m->facets[k] < 0 || m->facets[k] >= nv) {
      h->err = "facet vertex out of range";
      return PGX_EINVAL;
    }
    v2psi[m->facets[k]] = 0;
  }
  if (NPE == 3)
    for (int f = 0; f < nf; ++f) {  // the middle node of a contact edge sits at its midpoint
      const int32_t* fv = m->facets + 3 * (size_t)f;
      const double* A = m->coords + 2 * (size_t)fv[0];
      const double* B = m->coords + 2 * (size_t)fv[Q.e1];
      const double* M = m->coords + 2 * (size_t)fv[quad ? 1 : 2];
      const double dx = 0.5 * (A[0] + B[0]) - M[0], dy = 0.5 * (A[1] + B[1]) - M[1];
      const double l2 = (B[0] - A[0]) * (B[0] - A[0]) + (B[1] - A[1]) * (B[1] - A[1]);
      if (!(l2 > 0.0) || !(dx * dx + dy * dy <= 1e-20 * l2)) {
        h->err = "pgx_sg_create_2d: contact edge " + std::to_string(f) + " is degenerate or curved (straight edges only)";
        return PGX_EINVAL;
      }
    }
  h->cverts.clear();
  for (int v = 0; v < nv; ++v)
    if (v2psi[v] == 0) v2psi[v] = (int32_t)h->cverts.size(), h->cverts.push_back(v);
  const int npsi = (int)h->cverts.size();
  h->npsi = npsi;
  const int64_t ntot = (int64_t)nu + npsi;
  h->ntot = ntot;
  std::vector<uint8_t> hmask(nu, 0);
  std::vector<double> hg(nu, 0.0);
  for (int k = 0; k < p->n_bc; ++k) {
    const int d = p->bc_dofs[k];
    if (d < 0 || d >= nu) {
      h->err = "bc dof out of range";
      return PGX_EINVAL;
    }
    hmask[d] = 1;
    hg[d] = p->bc_vals ? p->bc_vals[k] : 0.0;
  }
  std::vector<int32_t> fpsi(NPE * (size_t)nf);
  for (size_t k = 0; k < fpsi.size(); ++k) fpsi[k] = v2psi[m->facets[k]];
  // entities: cells (mixed dofs (a, i) -> i nv + node a) and contact edges (u_y of the edge's nodes, then their psi dofs)
  auto cell_dofs = [&](int c, int32_t md[ND]) {
    for (int a = 0; a < NPC; ++a)
      for (int i = 0; i < 2; ++i) md[a * 2 + i] = i * nv + m->cells[NPC * (size_t)c + a];
  };
  auto facet_dofs = [&](int f, int32_t md[2 * NPE]) {
    for (int a = 0; a < NPE; ++a) md[a] = nv + m->facets[NPE * (size_t)f + a], md[NPE + a] = nu + fpsi[NPE * (size_t)f + a];
  };
  // pattern over the entity range: cells [0, nc), edges [nc, nc + nf) (as the 3-D code)
  std::vector<int32_t>& rowptr = h->h_rowptr;
  std::vector<int32_t>& col = h->h_col;
  const PatFind find = pattern_from_entities(ntot, (int64_t)nc + nf, [&](int64_t e, int32_t* md) {
    if (e < nc) return cell_dofs((int)e, md), ND;
    return facet_dofs((int)(e - nc), md), 2 * NPE;
  }, rowptr, col, h->err);
  if (!find) return PGX_EINVAL;
  const int64_t tot = h->nnz = rowptr[ntot];
  // kind (k_sg_jac_init of pgx_sg.hip): 0 = A slot, 1 = +-M_G slot, 2 = D slot, 3 = BC diagonal, 4 = zeroed by BCs (rows AND columns)
  std::vector<uint8_t> kind;
  saddle_kinds(ntot, nu, hmask, rowptr, col, kind);
  // destination tables, slot-major like the stashes the kernels write: table[slot * n_entities + entity]
  if ((double)NE * nc > 2.0e9) {
    h->err = "mesh too large for the one-pass assembly of the elasticity block";
    return PGX_ENOMEM;
  }
  std::vector<int32_t> dA((size_t)nc * NE), dM((size_t)nf * 2 * NF2), dD((size_t)nf * NF2), dbg((size_t)nf * NPE), dbe((size_t)nf * NPE);
  mx_par_for(nc, [&](int64_t a0, int64_t b0) {
    for (int64_t c = a0; c < b0; ++c) {
      int32_t md[ND];
      cell_dofs((int)c, md);
      for (int a = 0; a < ND; ++a)
        for (int b = 0; b < ND; ++b) dA[(size_t)(a * ND + b) * nc + (size_t)c] = find(md[a], md[b]);
    }
  });
  for (int f = 0; f < nf; ++f) {
    int32_t md[2 * NPE];
    facet_dofs(f, md);
    for (int a = 0; a < NPE; ++a) {
      dbg[(size_t)a * nf + f] = fpsi[NPE * (size_t)f + a];
      dbe[(size_t)a * nf + f] = nu + fpsi[NPE * (size_t)f + a];
      for (int b = 0; b < NPE; ++b) {
        dM[(size_t)(a * NPE + b) * nf + f] = find(md[a], md[NPE + b]);
        dM[(size_t)(NF2 + a * NPE + b) * nf + f] = find(md[NPE + a], md[b]);
        dD[(size_t)(a * NPE + b) * nf + f] = find(md[NPE + a], md[NPE + b]);
      }
    }
  }
  std::vector<int32_t> nod(ntot);
  for (int v = 0; v < nv; ++v) nod[v] = nod[(size_t)nv + v] = v;
  for (int k = 0; k < npsi; ++k) nod[(size_t)nu + k] = h->cverts[k];
  // device
  MXHIP(hipStreamCreate(&h->st));
  int rc = mx_lu_create(h, nv, nod.data(), 2, m->coords);
  if (rc) return rc;
  {  // latent rows negated -> symmetric [[alpha A, M_G^T], [M_G, -D]] for the LU, as in 3-D; PGX_SG_SYM=0: the general LU
    const char* e = pgx_tune("PGX_SG_SYM");
    if (!(e && atoi(e) == 0)) {
      pgx_nd_set_symmetric(h->lu, 1);
      if (pgx_nd_is_symmetric(h->lu)) h->lu_flip_from = nu;
    }
  }
  MXALLOC(h->coords, 2 * (size_t)nv);
  MXALLOC(h->facets, NPE * (size_t)nf);
  MXALLOC(h->fpsi, NPE * (size_t)nf);
  MXALLOC(h->stash, NF2 * (size_t)std::max(nf, 1));
  MXALLOC(h->mask, nu);
  MXALLOC(h->gbc, nu);
  MXALLOC(h->bg, npsi);
  MXALLOC(h->kind, tot);
  MXALLOC(h->Jc, tot);
  if ((rc = mx_alloc_state(h))) return rc;
  if ((rc = mx_upload_pattern(h))) return rc;
  MXALLOC(h->cells, NPC * (size_t)nc);
  MXALLOC(h->vm_tab, (size_t)NPC * NPC * 2);
  {
    std::vector<double> tab((size_t)NPC * NPC * 2);
    for (int n = 0; n < NPC; ++n) sg2_ref_grads<NPC>(ref[n][0], ref[n][1], tab.data() + (size_t)n * NPC * 2);
    MXHIP(hipMemcpy(h->vm_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
  }
  MXHIP(hipMemcpy(h->cells, m->cells, sizeof(int32_t) * NPC * (size_t)nc, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * (size_t)nv, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->facets, m->facets, sizeof(int32_t) * NPE * (size_t)nf, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->fpsi, fpsi.data(), sizeof(int32_t) * fpsi.size(), hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->mask, hmask.data(), nu, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->gbc, hg.data(), sizeof(double) * nu, hipMemcpyHostToDevice));
  MXHIP(hipMemcpy(h->kind, kind.data(), tot, hipMemcpyHostToDevice));
  MXHIP(hipMemsetAsync(h->Jc, 0, sizeof(double) * tot, h->st));
  MXHIP(hipMemsetAsync(h->bg, 0, sizeof(double) * npsi, h->st));
  {
    std::string e1 = pgx_scatter_build(dD.data(), (int64_t)NF2 * nf, tot, h->allocs, &h->sc_D);
    if (e1.empty()) e1 = pgx_scatter_build(dbe.data(), (int64_t)NPE * nf, ntot, h->allocs, &h->sc_b);
    if (!e1.empty()) {
      h->err = e1;
      return PGX_ENOMEM;
    }
  }
  // cell rule: triangles - the centroid (P1: constant integrand) / the 3-point degree-2 rule (P2: product of two affine gradients,
  // exact); quadrilaterals - Gauss-Legendre (d + 1)^2 on the unit square, as the hexahedral path
  std::vector<double> tab;
  int nqc = 0;
  if (!quad) {
    static const double p3[3][2] = {{1.0 / 6.0, 1.0 / 6.0}, {2.0 / 3.0, 1.0 / 6.0}, {1.0 / 6.0, 2.0 / 3.0}};
    nqc = NPC == 3 ? 1 : 3;
    tab.resize((size_t)nqc + (size_t)nqc * NPC * 2);
    for (int q = 0; q < nqc; ++q) {
      tab[q] = NPC == 3 ? 0.5 : 1.0 / 6.0;
      sg2_ref_grads<NPC>(NPC == 3 ? 1.0 / 3.0 : p3[q][0], NPC == 3 ? 1.0 / 3.0 : p3[q][1], tab.data() + nqc + (size_t)q * NPC * 2);
    }
  } else {
    const int n1 = deg + 1;
    nqc = n1 * n1;
    const double gp2[2] = {0.5 - 0.5 / sqrt(3.0), 0.5 + 0.5 / sqrt(3.0)}, gw2[2] = {0.5, 0.5};
    const double gp3[3] = {0.5 - 0.5 * sqrt(0.6), 0.5, 0.5 + 0.5 * sqrt(0.6)}, gw3[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};
    const double* gp = deg == 1 ? gp2 : gp3;
    const double* gw = deg == 1 ? gw2 : gw3;
    tab.resize((size_t)nqc + (size_t)nqc * NPC * 2);
    int q = 0;
    for (int qy = 0; qy < n1; ++qy)
      for (int qx = 0; qx < n1; ++qx, ++q) {
        tab[q] = gw[qx] * gw[qy];
        sg2_ref_grads<NPC>(gp[qx], gp[qy], tab.data() + nqc + (size_t)q * NPC * 2);
      }
  }
  // constant blocks, once, deterministic: park per entity, sum per destination; tables and stashes are temporary
  std::vector<void*> tmp;
  PgxScatter sc_c, sc_f, sc_g;
  std::string e1 = pgx_scatter_build(dA.data(), (int64_t)NE * nc, tot, tmp, &sc_c);
  if (e1.empty()) e1 = pgx_scatter_build(dM.data(), (int64_t)2 * NF2 * nf, tot, tmp, &sc_f);
  if (e1.empty()) e1 = pgx_scatter_build(dbg.data(), (int64_t)NPE * nf, npsi, tmp, &sc_g);
  double *st_c = nullptr, *st_f = nullptr, *d_tab = nullptr;
  hipError_t e = e1.empty() ? hipMalloc((void**)&st_c, sizeof(double) * NE * (size_t)nc) : hipErrorOutOfMemory;
  if (e == hipSuccess) e = hipMalloc((void**)&st_f, sizeof(double) * NFS * (size_t)std::max(nf, 1));
  if (e == hipSuccess) e = hipMalloc((void**)&d_tab, sizeof(double) * tab.size());
  if (e == hipSuccess) e = hipMemcpy(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_sg2_const_cells<NPC>, dim3((nc + 63) / 64), dim3(64), 0, h->st, nc, h->cells, h->coords, h->mu, h->lmbda, nqc, d_tab,
                       g0, g1, g2, st_c);
    pgx_scatter_run(h->st, sc_c, st_c, 1.0, 0, h->Jc);
    if (nf > 0) {
      hipLaunchKernelGGL(k_sg2_const_edges<NPE>, dim3((nf + 127) / 128), dim3(128), 0, h->st, nf, h->facets, h->coords, h->gap, h->Q1, st_f);
      pgx_scatter_run(h->st, sc_f, st_f, 1.0, 1, h->Jc);  // the +-M_G slots are disjoint from the elasticity slots
      pgx_scatter_run(h->st, sc_g, st_f + 2 * NF2 * (size_t)nf, 1.0, 0, h->bg);
    }
    e = hipStreamSynchronize(h->st);
  }
  hipFree(st_c);
  hipFree(st_f);
  hipFree(d_tab);
  for (void* q : tmp) hipFree(q);
  if (e != hipSuccess) {
    h->err = std::string("constant Jacobian blocks: ") + (e1.empty() ? hipGetErrorString(e) : e1.c_str());
    return PGX_EHIP;
  }
  return PGX_OK;
}

extern "C" int pgx_sg_create_2d(const pgx_sg_mesh2d* m, const pgx_sg_problem2d* p, int device, pgx_sg_handle** out) {
  if (!m || !p || !out || !m->coords || !m->cells || m->n_vertices <= 0 || m->n_cells <= 0 || m->n_facets < 0 ||
      (m->n_facets > 0 && !m->facets) || !p->qpts || !p->qwts || p->nq <= 0 || p->nq > SG_MAXQ || p->n_bc < 0 || (p->n_bc > 0 && !p->bc_dofs) ||
      !(p->E > 0.0) || !(p->nu > -1.0 && p->nu < 0.5)) {
    g_sg_error = "pgx_sg_create_2d: bad arguments";
    return PGX_EINVAL;
  }
  if (m->degree < 0 || m->degree > 2 || m->cell_type < 0 || m->cell_type > 1) {
    g_sg_error = "pgx_sg_create_2d: triangles (cell_type 0) or quadrilaterals (1) of degree 1 or 2";
    return PGX_EINVAL;
  }
  return mx_create("pgx_sg_create_2d", g_sg_error, device, out, [&](pgx_sg_handle* h) {
    if (m->cell_type == 1) return (m->degree == 2) ? sg2_create_impl<9, 3>(h, m, p) : sg2_create_impl<4, 2>(h, m, p);
    return (m->degree == 2) ? sg2_create_impl<6, 3>(h, m, p) : sg2_create_impl<3, 2>(h, m, p);
  });
}
