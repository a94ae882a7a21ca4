// pgx_sg_internal.h - the handle of example 02 (include/pgx_sg.h), shared by its 3-D element layer (pgx_sg.hip) and its plane one
// (pgx_sg2d.hip).  Everything above the element layer - pattern-independent kernels, the SNES mirror, the sparse LU - is common.
#pragma once
#include <string>
#include <vector>

#include "../../include/pgx_sg.h"
#include "pgx_mixed.h"
#include "pgx_scatter.h"

#define SG_MAXQ 16
struct SgQuad {
  double L[SG_MAXQ][3], w[SG_MAXQ];
  double N[SG_MAXQ][9];  // facet basis at the quadrature points: P1 = L; P2 = L_a (2 L_a - 1), then 4 L_a L_b for (0,1) (0,2) (1,2);
                         // quadrilateral facets: tensor Lagrange basis, lexicographic
  int nq;
  int g[3];              // local nodes spanning the (affine) facet: x = X[g0] + xi (X[g1] - X[g0]) + eta (X[g2] - X[g0])
};
// plane problems (pgx_sg_create_2d): rule on [0,1] and the basis of a contact EDGE at its points
struct SgQuad1 {
  double t[SG_MAXQ], w[SG_MAXQ];
  double N[SG_MAXQ][3];  // 2 nodes: (1 - t, t); 3 nodes: triangles' edges (end, end, midpoint), quadrilaterals' lexicographic (end, midpoint, end)
  int nq;
  int e1;                // local node of the edge's second END (the first is local node 0): x = X[0] + t (X[e1] - X[0])
};

#pragma GCC visibility push(hidden)
extern thread_local std::string g_sg_error;  // what pgx_sg_last_error(NULL) reports

struct pgx_sg_handle : MixedBase {
  int gdim = 3;                          // 2: a handle of pgx_sg_create_2d (coords [nv][2], x = [u_x | u_y | psi], facets are edges)
  int nv = 0, nc = 0, nf = 0, npsi = 0;  // nv = number of NODES (degree 2: vertices + edge midpoints)
  int npc = 4, npf = 3;                  // nodes per cell / per contact facet: 4 / 3 (degree 1), 10 / 6 (degree 2)
  SgQuad Q{};
  SgQuad1 Q1{};
  double gap = 0.0, mu = 0.0, lmbda = 0.0;
  double *coords = nullptr, *gbc = nullptr, *bg = nullptr;
  double* fgeo = nullptr;  // order-2 geometry (pgx_sg_create_curved): [facet][point][2] = surface element, z of the curved facet; else nullptr
  int32_t *facets = nullptr, *fpsi = nullptr;
  // deterministic facet assembly (pgx_scatter.h): k_sg_exp parks [slot * nf + facet]; one thread per destination sums
  PgxScatter sc_D, sc_b;  // D(psi): 9 slots per facet -> CSR positions; <exp(psi), w>: 3 slots per facet -> residual rows
  double* stash = nullptr;  // [9 * nf]
  uint8_t *mask = nullptr, *kind = nullptr;
  double* Jc = nullptr;
  std::vector<int32_t> cverts;
  bool partitioned = false;  // distributed handle: this rank assembled the elasticity blocks of its slab of cells only
  int nc_owned = 0;
  // diagnostics (pgx_sg_penetration / violation / von_mises): ALL cells of the mesh, the reference gradients of the cell basis at the
  // cell's own reference nodes [npc][npc][gdim], the gdim + 1 local nodes spanning the affine cell, and an output buffer grown on demand
  int32_t* cells = nullptr;
  double* vm_tab = nullptr;
  int vm_g[4] = {0, 1, 2, 3};
  bool curved = false;
  double* diag = nullptr;
  size_t diag_len = 0;
  pgx_sg_handle() : MixedBase("pgx_sg") {}
  void residual_dev(const double* xin, double* Fout) override;
  void jacobian_dev(const double* xin) override;
};

// 1-D Lagrange basis on the equispaced nodes k / d (d = 1, 2): values l[0..d] and derivatives dl[0..d] at t
static inline void sg_lagrange1d(int d, double t, double* l, double* dl) {
  if (d == 1) {
    l[0] = 1.0 - t, l[1] = t;
    dl[0] = -1.0, dl[1] = 1.0;
  } else {
    l[0] = 2.0 * (t - 0.5) * (t - 1.0), l[1] = -4.0 * t * (t - 1.0), l[2] = 2.0 * t * (t - 0.5);
    dl[0] = 4.0 * t - 3.0, dl[1] = 4.0 - 8.0 * t, dl[2] = 4.0 * t - 1.0;
  }
}

// pgx_sg2d.hip: the launches behind the shared entry points on a handle with gdim == 2 (stream h->st, no synchronisation)
void sg2d_exp(pgx_sg_handle* h, int mode, const double* xin);  // mode 0: D(psi) slots, 1: <exp psi, w> into h->stash
void sg2d_penetration(pgx_sg_handle* h);                       // MX_RED partials into h->partials
void sg2d_violation(pgx_sg_handle* h, double* out_dev);        // [nv]
void sg2d_von_mises(pgx_sg_handle* h, double* out_dev);        // [nc][npc]
#pragma GCC visibility pop
