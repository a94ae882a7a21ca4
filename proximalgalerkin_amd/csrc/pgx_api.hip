// Host side of libpgx.so, the entry points: the tuning table, handle creation and destruction, state access, residual, Jacobian and
// operator apply, the SNES-mirroring Newton driver, and that part of the extern "C" ABI of include/pgx.h.  The handle is defined in
// pgx_handle.h; host-side setup is in pgx_setup.hip, the preconditioner in pgx_cycle.hip, the test and measurement hooks in
// pgx_hooks.hip, FGMRES and the reductions' read-back in pgx_krylov.hip.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pgx_handle.h"

thread_local std::string g_create_error;

// ---- tuning table (pgx_scope.h: pgx_tune) ----
namespace {
std::mutex g_tune_mu;
std::atomic<int> g_tune_gen{0};
// values are interned in a pool that is never freed: pgx_tune hands out pointers that outlive any later pgx_tuning_set
std::map<std::string, const std::string*>& tune_table() {
  static std::map<std::string, const std::string*> t;
  return t;
}
std::deque<std::string>& tune_pool() {
  static std::deque<std::string> p;
  return p;
}
}  // namespace
const char* pgx_tune(const char* name) {
  std::lock_guard<std::mutex> lk(g_tune_mu);
  auto& t = tune_table();
  auto it = t.find(name);
  return it == t.end() ? nullptr : it->second->c_str();
}
int pgx_tune_gen() { return g_tune_gen.load(std::memory_order_acquire); }
extern "C" int pgx_tuning_set(const char* key, const char* value) {
  if (!key || strncmp(key, "PGX_", 4) != 0) return PGX_EINVAL;
  std::lock_guard<std::mutex> lk(g_tune_mu);
  if (value) {
    const std::string* interned = nullptr;
    for (const std::string& s : tune_pool())
      if (s == value) interned = &s;
    if (!interned) {
      tune_pool().emplace_back(value);  // std::deque never moves its elements
      interned = &tune_pool().back();
    }
    tune_table()[key] = interned;
  } else {
    tune_table().erase(key);
  }
  g_tune_gen.fetch_add(1, std::memory_order_release);
  return PGX_OK;
}

extern "C" void pgx_default_opts(pgx_snes_opts* o) {
  o->snes_rtol = 1e-8;
  o->snes_atol = 1e-50;
  o->snes_stol = 1e-8;
  o->snes_divtol = 1e4;
  o->snes_max_it = 50;
  o->ksp_rtol = 0.0;  // 0 = auto: 1e-10 for P1, 1e-11 for P2 (measured effect on the final u: DESIGN.md section 3)
  o->ksp_max_it = 200;
  o->ksp_restart = 30;
  o->mg_nu = 6;  // 2048^2 sweep (profiles/): nu=2 780 ms, 4 707, 6 660, 8 692, 10 763 per solve - more smoothing shrinks the
                  // Krylov space, whose orthogonalisation cost grows with its square
  // damping, re-measured in round 2 on the row-mapped kernels (2048^2, ms per solve / Krylov iterations per solve): 0.60 338, 0.65 324,
  // 0.70 314 / -, 0.72 311 / 252, 0.75 302 / 246, 0.76 - / 248, 0.77 - / 250, 0.78 332 / 265, 0.80 334 / 267, 0.85 359, 0.90 374: the
  // optimum of the smoothing factor is flat between 0.72 and 0.77; from 0.78 on one late Newton step trips the stagnation
  // test and finishes at omega_safe.  1024^2 and 512^2 do not care (87-89 ms, 58 ms for 0.70-0.80).  Round 1 used 0.8.
  o->mg_omega = 0.75;
  o->monitor = 0;
  o->pc_type = 0;  // auto: multigrid for P1, sparse LU for P2
  o->linesearch = 0;
}

extern "C" const char* pgx_last_error(const pgx_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// ------------------------------------------------------------------------------------------------
// pgx_create_curved hands its geometry table to create_impl through this slot (same thread, cleared on return)
static thread_local const double* g_create_geoq = nullptr;

// The tuning keys a handle reads once, when it is created (pgx_tuning_set; each key is described at its member in pgx_handle.h)
static void read_tuning(pgx_handle* h) {
  if (const char* e = pgx_tune("PGX_XCD_REMAP")) h->xcd_remap = atoi(e) ? 2 : 0;
  if (const char* e = pgx_tune("PGX_TAIL_VERTS")) h->tail_verts = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_PATCH")) h->p2_patch = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_PATCH_NU")) h->patch_nu = std::max(1, atoi(e));
  if (const char* e = pgx_tune("PGX_P2_PATCH_OMEGA")) h->patch_omega = atof(e);
  if (const char* e = pgx_tune("PGX_P2_PATCH_F32")) h->patch_f32 = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_PATCH_SYM")) h->patch_sym = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_RESID_F32")) h->p2_resid_f32 = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_STENCIL")) h->p2st.enable = atoi(e);
  if (const char* e = pgx_tune("PGX_P2_STENCIL_DIST")) h->p2st.dist_enable = atoi(e);
  if (!h->patch_f32) h->patch_sym = 0;
  if (h->patch_f32 == 2 && !h->patch_sym) h->patch_f32 = 1;  // bfloat16 storage exists in the symmetric packing only
  if (const char* e = pgx_tune("PGX_P2_FALLBACK_ITS")) h->p2_fallback_its = std::max(1, atoi(e));
  {
    const char* e = pgx_tune("PGX_TAIL2");  // 0: the round-2 tail kernels (A/B)
    pgxk_mg_tail_select(e ? atoi(e) : 1);
  }
  if (const char* e = pgx_tune("PGX_FUSED_LEGS")) h->fused_legs = atoi(e);
  if (const char* e = pgx_tune("PGX_FUSED_K3")) h->fused_k3 = atoi(e);
  if (const char* e = pgx_tune("PGX_NU_COARSE")) h->nu_coarse = atoi(e);
  if (const char* e = pgx_tune("PGX_SPMV_STREAM")) h->spmv_stream = atoi(e);
  if (const char* e = pgx_tune("PGX_SPMV_BAL")) h->spmv_bal = atoi(e);
  if (const char* e = pgx_tune("PGX_SPMV_DICT")) h->spmv_dict = atoi(e);
  if (const char* e = pgx_tune("PGX_SPMV_STENCIL")) h->spmv_stencil = atoi(e);
  if (const char* e = pgx_tune("PGX_RESID_GRID")) h->resid_grid = atoi(e);
  if (const char* e = pgx_tune("PGX_RESID_REUSE")) h->resid_reuse = atoi(e);
  if (const char* e = pgx_tune("PGX_D_DIRECT")) h->d_direct = atoi(e);
  if (const char* e = pgx_tune("PGX_RAP_LDS_MIN")) h->rap_lds_min = atoi(e);
  if (const char* e = pgx_tune("PGX_K6_MAX")) h->k6_max = atoi(e);
  if (const char* e = pgx_tune("PGX_SMOOTH_D32")) h->smooth_d32 = atoi(e);
  if (const char* e = pgx_tune("PGX_HOST_POLL")) h->host_poll = atoi(e);
  if (const char* e = pgx_tune("PGX_GS_WIDE")) h->gs_wide = atoi(e) >= 16 ? 16 : 8;
  if (const char* e = pgx_tune("PGX_FUSED_PUBLISH")) h->fused_publish = atoi(e);
  if (const char* e = pgx_tune("PGX_TICKET_REDUCE")) h->ticket_reduce = atoi(e);
  if (const char* e = pgx_tune("PGX_FUSED_RESID")) h->fused_resid = atoi(e);
  if (const char* e = pgx_tune("PGX_LEAN_RHS")) h->lean_rhs = atoi(e);
  if (const char* e = pgx_tune("PGX_FUSED_STEP")) h->fused_step = atoi(e);
  if (const char* e = pgx_tune("PGX_LAZY_NORM")) h->lazy_norm = atoi(e);
  if (const char* e = pgx_tune("PGX_V_F32")) h->v_f32 = atoi(e);
  if (const char* e = pgx_tune("PGX_V_F32_GAIN")) h->v_f32_gain = atof(e);
  if (const char* e = pgx_tune("PGX_V_F32_MAX")) h->v_f32_max = atof(e);
  if (const char* e = pgx_tune("PGX_V_F32_MIN")) h->v_f32_min = atoi(e);
  if (const char* e = pgx_tune("PGX_Z_F32")) h->z_f32 = atoi(e);
  if (const char* e = pgx_tune("PGX_F32_DBF16")) h->f32_dbf16 = atoi(e);
  if (const char* e = pgx_tune("PGX_SPMV_D4")) h->spmv_d4 = atoi(e);
  if (const char* e = pgx_tune("PGX_LEAN_D")) h->lean_d = atoi(e);
  if (const char* e = pgx_tune("PGX_MG_F32")) h->mg_f32 = atoi(e);
  if (const char* e = pgx_tune("PGX_F32_MIN")) h->f32_min = atoi(e);
  if (const char* e = pgx_tune("PGX_F32_RR_MAX")) h->f32_rr_max = atoi(e);
  if (const char* e = pgx_tune("PGX_F32_K6_MAX")) h->f32_k6_max = atoi(e);
  if (const char* e = pgx_tune("PGX_STAG_ITS")) h->stag_its = std::max(2, atoi(e));
  if (const char* e = pgx_tune("PGX_STAG_GAIN")) h->stag_gain = atof(e);
  if (const char* e = pgx_tune("PGX_FUSED_MIN")) h->fused_min = atoi(e);
  if (const char* e = pgx_tune("PGX_CGS_ETA2")) h->cgs_eta2 = atof(e);
  if (const char* e = pgx_tune("PGX_COARSE_SWEEPS")) h->coarse_sweeps = atoi(e);
  if (const char* e = pgx_tune("PGX_UMG")) h->umg_enable = atoi(e);
  if (const char* e = pgx_tune("PGX_UMG_MIN")) h->umg_min = atoi(e);
  if (const char* e = pgx_tune("PGX_UMG_MIN_P2")) h->umg_min_p2 = atoi(e);
  if (const char* e = pgx_tune("PGX_UMG_BUILD_MIN")) h->umg_build_min = atoi(e);
  if (const char* e = pgx_tune("PGX_AMG_BUILD")) h->amg_build = atoi(e);
  if (const char* e = pgx_tune("PGX_AMG_SPLIT_BATCH")) h->amg_split_batch = std::max(1, atoi(e));
  if (const char* e = pgx_tune("PGX_P2_PATCH_WIDE")) h->patch_wide = atoi(e);
  if (const char* e = pgx_tune("PGX_UMG_COARSE_SWEEPS")) h->umg_coarse_sweeps = std::max(1, atoi(e));
  if (const char* e = pgx_tune("PGX_UMG_COARSE_LDS")) h->umg_coarse_lds = atoi(e);
}

static int create_impl(const pgx_mesh* m, const pgx_problem* p, int device, const pgx_partition* part, pgx_comm* comm,
                       pgx_handle** out) {
  if (!m || !p || !out) {
    g_create_error = "null argument";
    return PGX_EINVAL;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: libpgx has no CPU fallback";
    return PGX_ENODEV;
  }
  if (device < 0 || device >= ndev) {
    g_create_error = "device index out of range";
    return PGX_EINVAL;
  }
  pgx_handle* h = new pgx_handle();
  read_tuning(h);
  auto fail = [&](int rc) {
    g_create_error = h->err;
    pgx_destroy(h);
    return rc;
  };
  h->device = device;
  if (p->degree != 1 && p->degree != 2) {
    h->err = "only Lagrange degree 1 and 2 are implemented";
    return fail(PGX_EINVAL);
  }
  h->degree = p->degree;
  if (p->degree == 2 && (!m->cell_dofs || m->n_dofs <= m->n_vertices)) {
    h->err = "degree 2 needs pgx_mesh.cell_dofs [n_cells][6] and n_dofs = n_vertices + n_edges";
    return fail(PGX_EINVAL);
  }
  if (p->nq < 1 || p->nq > PGX_MAX_NQ || !p->qpts || !p->qwts || !p->phi_q || m->n_vertices < 3 || m->n_cells < 1 ||
      !m->coords || !m->cells || (p->n_bc > 0 && !p->bc_dofs)) {
    h->err = "invalid mesh/problem description";
    return fail(PGX_EINVAL);
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->st) != hipSuccess) {
    h->err = "hipSetDevice/hipStreamCreate failed";
    return fail(PGX_EHIP);
  }
  hipEventCreate(&h->e0);
  hipEventCreate(&h->e1);
  const int n = h->n = m->n_vertices, nc = h->nc = m->n_cells;
  const int nd = h->nd = (p->degree == 2) ? m->n_dofs : n;
  h->f = p->f;
  if (m->structured_nx > 0 && m->structured_ny > 0) {
    if ((int64_t)(m->structured_nx + 1) * (m->structured_ny + 1) != n ||
        (int64_t)2 * m->structured_nx * m->structured_ny != nc) {
      h->err = "structured_nx/ny inconsistent with n_vertices/n_cells";
      return fail(PGX_EINVAL);
    }
    h->structured = true;
    h->nx = m->structured_nx;
    h->ny = m->structured_ny;
  }
  if (part) {  // sharded: this mesh is one strip of a global structured mesh (include/pgx.h, "Sharded path")
    pgx_partition pt = *part;
    int32_t row0 = 0, nrows = 0, own0 = 0, nown = 0;
    if (pgx_partition_rows(&pt, &row0, &nrows, &own0, &nown)) {
      h->err = g_create_error;
      return fail(PGX_EINVAL);
    }
    if (!comm || comm->rank != pt.rank || comm->size != pt.size) {
      h->err = "pgx_create_sharded: communicator rank/size differ from the partition's";
      return fail(PGX_EINVAL);
    }
    if (!h->structured || (p->degree != 1 && p->degree != 2)) {
      h->err = "pgx_create_sharded: structured P1 / P2 meshes are sharded (strip decomposition)";
      return fail(PGX_EINVAL);
    }
    if (h->ny + 1 != nrows || h->nx % (1 << pt.dist_levels)) {
      h->err = "pgx_create_sharded: local mesh must hold exactly the vertex rows of pgx_partition_rows, and nx must be "
               "divisible by 2^dist_levels";
      return fail(PGX_EINVAL);
    }
    for (int c = 0; c < nc; ++c) {  // owned cells are addressed as a contiguous range: cells must be ordered by rows
      const int v0 = std::min(m->cells[3 * c], std::min(m->cells[3 * c + 1], m->cells[3 * c + 2]));
      if (v0 / (h->nx + 1) != c / (2 * h->nx)) {
        h->err = "pgx_create_sharded: cells must be ordered row by row (cell 2*(j*nx+i)+t)";
        return fail(PGX_EINVAL);
      }
    }
    Dist& D = h->dist;
    D.on = true;
    D.comm = comm;
    D.rank = pt.rank;
    D.size = pt.size;
    D.ldist = pt.dist_levels;
    D.global_ny = pt.global_ny;
    const int Hh = pt.global_ny / pt.size;
    for (int l = 0; l < D.ldist; ++l) {
      DistLevel d;
      d.g = ghost_mul() << (D.ldist - l);
      d.glo = pt.rank > 0 ? d.g : 0;
      d.H = (Hh >> l) + (pt.rank + 1 == pt.size ? 1 : 0);
      d.ghi = pt.rank + 1 < pt.size ? d.g + 1 : 0;
      D.L.push_back(d);
    }
    const size_t sx = (size_t)h->nx + 1;
    D.own_off = D.L[0].glo * sx;
    D.own_cnt = D.L[0].H * sx;
    const int cell_rows = (pt.rank + 1 == pt.size) ? D.L[0].H - 1 : D.L[0].H;
    D.cell0 = 2 * h->nx * D.L[0].glo;
    D.ncell_own = 2 * h->nx * cell_rows;
    if (p->degree == 2) {
      D.eb = 3 * (size_t)h->nx + 1;
      const size_t last = (size_t)h->ny;  // the last local vertex row carries its nx horizontal edges only
      auto E = [&](size_t row) { return row <= last ? row * D.eb : last * D.eb + (size_t)h->nx; };
      D.eown_off = E(D.L[0].glo);
      D.eown_cnt = E((size_t)D.L[0].glo + D.L[0].H) - D.eown_off;
    }
  }
  // quadrature tables
  h->q.nq = p->nq;
  memset(h->q.Mref, 0, sizeof(h->q.Mref));
  memset(h->q.mref, 0, sizeof(h->q.mref));
  for (int k = 0; k < p->nq; ++k) {
    const double X = p->qpts[2 * k], Y = p->qpts[2 * k + 1];
    h->q.N[k][0] = 1.0 - X - Y;
    h->q.N[k][1] = X;
    h->q.N[k][2] = Y;
    h->q.w[k] = p->qwts[k];
    for (int a = 0; a < 3; ++a) {
      h->q.mref[a] += h->q.w[k] * h->q.N[k][a];
      for (int b = 0; b < 3; ++b) h->q.Mref[a][b] += h->q.w[k] * h->q.N[k][a] * h->q.N[k][b];
    }
  }
  if (p->degree == 2) {  // P2 tables (basis ordering: SURVEY.md App. A.2)
    QuadTab2& t = h->q2;
    t.nq = p->nq;
    const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
    const int ej[3] = {1, 0, 0}, ek[3] = {2, 2, 1};
    for (int k = 0; k < p->nq; ++k) {
      const double X = p->qpts[2 * k], Y = p->qpts[2 * k + 1];
      const double l[3] = {1.0 - X - Y, X, Y};
      t.w[k] = p->qwts[k];
      for (int i = 0; i < 3; ++i) {
        t.L[k][i] = l[i];
        t.N[k][i] = l[i] * (2.0 * l[i] - 1.0);
        t.N[k][3 + i] = 4.0 * l[ej[i]] * l[ek[i]];
        for (int d = 0; d < 2; ++d) {
          t.dN[k][i][d] = (4.0 * l[i] - 1.0) * dl[i][d];
          t.dN[k][3 + i][d] = 4.0 * (l[ej[i]] * dl[ek[i]][d] + l[ek[i]] * dl[ej[i]][d]);
        }
      }
    }
  }
  // Dirichlet data (dofs of the solution space; the P1 coarse space uses the vertex prefix)
  std::vector<uint8_t> hmask(nd, 0);
  std::vector<double> hg(nd, 0.0);
  for (int k = 0; k < p->n_bc; ++k) {
    const int d = p->bc_dofs[k];
    if (d < 0 || d >= nd) {
      h->err = "bc dof out of range";
      return fail(PGX_EINVAL);
    }
    hmask[d] = 1;
    hg[d] = p->bc_vals ? p->bc_vals[k] : 0.0;
  }
  int rc;
  auto up = [&]() -> int {
    DALLOC(h->coords, (size_t)2 * n);
    DALLOC(h->cells, (size_t)3 * nc);
    DALLOC(h->mask, nd);
    DALLOC(h->gbc, nd);
    DALLOC(h->bphi, nd);
    HIPCHK(hipMemcpy(h->coords, m->coords, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    if (g_create_geoq) {  // isoparametric cells of order 2: weights and inverse Jacobians per quadrature point (pgx_p2.hip)
      if (h->structured || part) {
        h->err = "pgx_create_curved: order-2 geometry is implemented for unstructured, unpartitioned meshes (degree-1 and degree-2 "
                 "fields); structured grids have affine cells by construction";
        return PGX_EINVAL;
      }
      DALLOC(h->geoq, (size_t)5 * nc * p->nq);
      HIPCHK(hipMemcpy(h->geoq, g_create_geoq, sizeof(double) * 5 * (size_t)nc * p->nq, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(h->cells, m->cells, sizeof(int32_t) * 3 * (size_t)nc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mask, hmask.data(), nd, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->gbc, hg.data(), sizeof(double) * nd, hipMemcpyHostToDevice));
    if (p->degree == 2) {
      int r2 = build_plan_p2(h, m, hmask);
      if (r2) return r2;
    }
    {  // the P1 plan first: its vertex -> (cell, local vertex) lists also drive the b_phi scatter
      const int r = build_plan(h, m, hmask);
      if (r) return r;
    }
    // b_phi from phi at quadrature points, then phi_q is dropped (it never changes: obstacle_pg.py:107-111)
    double* phi_q = nullptr;
    const size_t nphi = (size_t)nc * p->nq;
    if (hipMalloc((void**)&phi_q, nphi * sizeof(double)) != hipSuccess) {
      h->err = "hipMalloc(phi_q)";
      return PGX_ENOMEM;
    }
    hipError_t e = hipMemcpy(phi_q, p->phi_q, nphi * sizeof(double), hipMemcpyHostToDevice);
    double* stash = nullptr;  // element vectors, summed per dof in list order (no atomics: b_phi is bitwise reproducible)
    if (e == hipSuccess) e = hipMalloc((void**)&stash, sizeof(double) * 8 * (size_t)nc);
    if (e == hipSuccess) {
      if (p->degree == 2)
        pgxk_bphi_p2(h->st, nc, nd, h->cdofs, h->coords, phi_q, h->q2, h->p2_v2c_ptr, h->p2_v2c_ent, stash, h->bphi, h->geoq);
      else
        pgxk_bphi(h->st, nc, n, h->cells, h->coords, phi_q, h->q, h->v2c_ptr, h->v2c_ent, stash, h->bphi, h->geoq);
      e = hipStreamSynchronize(h->st);
    }
    hipFree(phi_q);
    if (stash) hipFree(stash);
    if (e != hipSuccess) {
      h->err = std::string("b_phi assembly: ") + hipGetErrorString(e);
      return PGX_EHIP;
    }
    DALLOC(h->Kv, h->nnz);
    DALLOC(h->Mv, h->nnz);
    DALLOC(h->Dv, h->nnz);
    // (order-2 geometry: per-point geometry for a degree-1 discretisation; the P1 level BELOW a degree-2 one is a preconditioner
    // level and keeps the affine operators of the vertices)
    const double* geo1 = p->degree == 1 ? h->geoq : nullptr;
    pgxk_fill_rows(h->st, 0, n, h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells, h->coords,
                   nullptr, h->q, h->Kv, geo1);
    pgxk_fill_rows(h->st, 1, n, h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells, h->coords,
                   nullptr, h->q, h->Mv, geo1);
    if (p->degree == 2) {
      DALLOC(h->s_K, h->s_nnz);
      DALLOC(h->s_M, h->s_nnz);
      DALLOC(h->s_D, h->s_nnz);
      pgxk_fill_rows_p2(h->st, 0, nd, h->s_fill_lds, h->s_rowptr, h->p2_v2c_ptr, h->p2_v2c_ent, h->p2_v2c_pos, h->cdofs,
                        h->coords, nullptr, h->q2, h->s_K, h->geoq);
      pgxk_fill_rows_p2(h->st, 1, nd, h->s_fill_lds, h->s_rowptr, h->p2_v2c_ptr, h->p2_v2c_ent, h->p2_v2c_pos, h->cdofs,
                        h->coords, nullptr, h->q2, h->s_M, h->geoq);
      if (h->spmv_dict && h->spmv_bal && h->s_blk) {
        const int rc = build_km_dictionary(h);
        if (rc) return rc;
      }
      DALLOC(h->p2_stash, (size_t)16 * nc);
      DALLOC(h->p2_xu, nd);
      DALLOC(h->p2_xp, nd);
      DALLOC(h->p2_ru, nd);
      DALLOC(h->p2_rp, nd);
      DALLOC(h->c1_bu, n);
      DALLOC(h->c1_bp, n);
      DALLOC(h->c1_xu, n);
      DALLOC(h->c1_xp, n);
    } else {
      h->s_rowptr = h->rowptr;
      h->s_colm = h->colm;
      h->s_K = h->Kv;
      h->s_M = h->Mv;
      h->s_D = h->Dv;
      h->s_nnz = h->nnz;
      h->s_fill_lds = h->fill_lds;
    }
    const size_t n2 = 2 * (size_t)nd;
    DALLOC(h->x, n2);
    DALLOC(h->xk, n2);
    DALLOC(h->F, n2);
    DALLOC(h->dx, n2);
    DALLOC(h->xw, n2);
    DALLOC(h->rhs, n2);
    HIPCHK(hipMemsetAsync(h->x, 0, n2 * sizeof(double), h->st));
    HIPCHK(hipMemsetAsync(h->xk, 0, n2 * sizeof(double), h->st));
    // Krylov basis capacity: 50 vectors cover P1 (restart 30).  The P2 two-level preconditioner leaves outlier
    // modes on the late large-alpha systems whose number grows with N; restarting then stagnates, so P2 keeps
    // up to 300 basis vectors within a 96 GB budget (V and Z) - HBM capacity is what MI355X has plenty of.
    h->restart = 50;
    if (p->degree == 2) {
      // PGX_P2_BASIS_GB (default 24): the sparse LU is the default P2 preconditioner (1-2 iterations per Newton step), the
      // long basis only matters for "pc_type": "pgx_mg"; 96 GB reproduces the pre-LU behaviour
      double budget = 24e9;
      if (const char* e = pgx_tune("PGX_P2_BASIS_GB")) budget = 1e9 * atof(e);
      const double per_vec = 2.0 * (double)n2 * sizeof(double);
      h->restart = (int)std::max(50.0, std::min(300.0, budget / per_vec));
    }
    DALLOC(h->V, (size_t)(h->restart + 1) * n2);
    DALLOC(h->Z, (size_t)h->restart * n2);
    DALLOC(h->w, n2);
    DALLOC(h->d_small, 4 * (h->restart + 2));
    DALLOC(h->partials, (size_t)PGX_RED_BLOCKS * (h->restart + 2));
    DALLOC(h->partials2, 2 * (size_t)pgxk_multidot_blocks(n2));  // pgxk_axpy_norms: two rows of its grid
    DALLOC(h->d_ticket, PGX_TK_WORDS);
    HIPCHK(hipMemsetAsync(h->d_ticket, 0, sizeof(unsigned long long) * PGX_TK_WORDS, h->st));
    {  // small read-backs (norms, the Hessenberg column, observables): pinned + mapped + coherent, one sequence word at the end
      const size_t nsm = 4 * (size_t)(h->restart + 2);
      HIPCHK(hipHostMalloc((void**)&h->h_small, sizeof(double) * (nsm + 2), hipHostMallocMapped | hipHostMallocCoherent));
      memset(h->h_small, 0, sizeof(double) * (nsm + 2));
      HIPCHK(hipHostGetDevicePointer((void**)&h->h_small_dev, h->h_small, 0));
      h->h_seq = reinterpret_cast<unsigned long long*>(h->h_small + nsm);
      h->h_seq_dev = reinterpret_cast<unsigned long long*>(h->h_small_dev + nsm);
    }
    DALLOC(h->tmp_u, n);
    DALLOC(h->tmp_p, n);
    DALLOC(h->res_u, n);
    DALLOC(h->res_p, n);
    h->obs_blocks = pgxk_observables_blocks(nc);
    DALLOC(h->obs_partials, (size_t)h->obs_blocks * 6);
    DALLOC(h->d_out6, 6);
    if (h->dist.on) {
      DALLOC(h->dist.sb, n2);
      DALLOC(h->dist.wc, 2 * h->dist.nk_field() + 2);
    }
    const int r = h->dist.on ? build_multigrid_dist(h) : build_multigrid(h);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(h->st));
    return PGX_OK;
  };
  rc = up();
  if (rc) return fail(rc);
  *out = h;
  return PGX_OK;
}

extern "C" int pgx_create(const pgx_mesh* m, const pgx_problem* p, int device, pgx_handle** out) {
  return create_impl(m, p, device, nullptr, nullptr, out);
}
extern "C" int pgx_create_curved(const pgx_mesh* m, const pgx_problem* p, const double* geoq, int device, pgx_handle** out) {
  if (!geoq) {
    g_create_error = "pgx_create_curved: null geometry table";
    return PGX_EINVAL;
  }
  g_create_geoq = geoq;
  const int rc = create_impl(m, p, device, nullptr, nullptr, out);
  g_create_geoq = nullptr;
  return rc;
}
extern "C" int pgx_create_lu_dist(const pgx_mesh* m, const pgx_problem* p, pgx_comm* comm, int device, pgx_handle** out) {
  if (!comm) {
    g_create_error = "pgx_create_lu_dist: null communicator";
    return PGX_EINVAL;
  }
  int rc = create_impl(m, p, device, nullptr, nullptr, out);
  if (rc) return rc;
  (*out)->lu_comm = comm;
  if (const char* e = pgx_tune("PGX_CHECK_REPLICAS")) (*out)->check_replicas = atoi(e) != 0;
  return PGX_OK;
}
extern "C" int pgx_create_sharded(const pgx_mesh* m, const pgx_problem* p, const pgx_partition* part, pgx_comm* comm,
                                  int device, pgx_handle** out) {
  if (!part || !comm) {
    g_create_error = "pgx_create_sharded: null partition / communicator";
    return PGX_EINVAL;
  }
  return create_impl(m, p, device, part, comm, out);
}

extern "C" void pgx_destroy(pgx_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->st) hipStreamSynchronize(h->st);
  if (pgx_tune("PGX_CGS_REPORT"))
    fprintf(stderr, "pgx: selective CGS2 skipped the second projection in %ld of %ld Krylov iterations\n", h->cgs_skipped, h->cgs_total);
  if (h->lu) pgx_nd_destroy(h->lu);
  for (void* p : h->allocs) hipFree(p);
  if (h->h_small) hipHostFree(h->h_small);
  if (h->e0) hipEventDestroy(h->e0);
  if (h->e1) hipEventDestroy(h->e1);
  if (h->st) hipStreamDestroy(h->st);
  delete h;
}

// ------------------------------------------------------------------------------------------------
// state access
// ------------------------------------------------------------------------------------------------
extern "C" int pgx_num_dofs(const pgx_handle* h, int64_t* nd) {
  if (!h || !nd) return PGX_EINVAL;
  *nd = 2 * (int64_t)h->nd;
  return PGX_OK;
}
int copy_in(pgx_handle* h, double* dst, const double* src) {
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * 2 * (size_t)h->nd, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}
int copy_out(pgx_handle* h, double* dst, const double* src) {
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * 2 * (size_t)h->nd, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_set_state(pgx_handle* h, const double* x) {
  NEED(h);
  if (!x) return PGX_EINVAL;
  return copy_in(h, h->x, x);
}
extern "C" int pgx_get_state(pgx_handle* h, double* x) {
  NEED_KEEP(h);
  if (!x) return PGX_EINVAL;
  return copy_out(h, x, h->x);
}
extern "C" int pgx_set_prev(pgx_handle* h, const double* x) {
  NEED_KEEP(h);
  if (!x) return PGX_EINVAL;
  return copy_in(h, h->xk, x);
}
extern "C" int pgx_get_prev(pgx_handle* h, double* x) {
  NEED_KEEP(h);
  if (!x) return PGX_EINVAL;
  return copy_out(h, x, h->xk);
}
extern "C" int pgx_advance_prev(pgx_handle* h) {
  NEED_KEEP(h);
  pgxk_scale_copy(h->st, 2 * (size_t)h->nd, 1.0, h->x, h->xk);  // a streaming kernel: the runtime's D2D blit ran these 67 MB at 0.5 TB/s
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_zero_state(pgx_handle* h) {
  NEED(h);
  HIPCHK(hipMemsetAsync(h->x, 0, sizeof(double) * 2 * (size_t)h->nd, h->st));
  HIPCHK(hipMemsetAsync(h->xk, 0, sizeof(double) * 2 * (size_t)h->nd, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_owned_range(const pgx_handle* h, int64_t* offset, int64_t* count) {
  if (!h) return PGX_EINVAL;
  if (offset) *offset = h->dist.on ? (int64_t)h->dist.own_off : 0;
  if (count) *count = h->dist.on ? (int64_t)h->dist.own_cnt : (int64_t)(h->degree == 2 ? h->n : h->nd);
  return PGX_OK;
}
extern "C" int pgx_owned_edge_range(const pgx_handle* h, int64_t* offset, int64_t* count) {
  if (!h) return PGX_EINVAL;
  if (offset) *offset = (int64_t)h->n + (h->dist.on ? (int64_t)h->dist.eown_off : 0);
  if (count) *count = h->dist.on ? (int64_t)h->dist.eown_cnt : (int64_t)(h->nd - h->n);
  return PGX_OK;
}
extern "C" int pgx_sync_ghosts(pgx_handle* h) {
  NEED(h);
  if (!h->dist.on) return PGX_OK;
  int rc = halo_solution(h, h->x, h->x + h->nd);
  if (!rc) rc = halo_solution(h, h->xk, h->xk + h->nd);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}
extern "C" int pgx_set_alpha(pgx_handle* h, double a) {
  if (!h || !(a > 0.0)) return PGX_EINVAL;
  h->alpha = a;
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// building blocks
// ------------------------------------------------------------------------------------------------
// PGX_D_DIRECT applies: single handle, degree 1, uniform finest level through the grid kernels, fp64 stencils without the float copy
static bool d_direct_on(const pgx_handle* h) {
  return h->d_direct && !h->dist.on && h->degree == 1 && h->structured && h->resid_grid && !h->lev.empty() && h->lev[0].uniform &&
         sizeof(dsten_t) == 8 && !h->lev[0].Dh32;
}

// the residual (and D(psi)) of this handle goes through k_resid_fill_grid / its frame kernel
static bool resid_grid_on(const pgx_handle* h) {
  return h->degree == 1 && h->resid_grid && h->structured && !h->lev.empty() && h->lev[0].uniform;
}

// PGX_RESID_REUSE applies: single handle on the grid path with the default (single-precision) multigrid; sharded handles, replicas of a
// distributed LU and the fp64 variant keep the full evaluation
bool resid_reuse_on(const pgx_handle* h) {
  return h->resid_reuse && resid_grid_on(h) && !h->dist.on && !h->lu_comm && h->mg_f32;
}

// fu_only (grid path only, pgx_handle::fresh says when): F[nd ..) and the D copies are at this x already - F[0 .. nd) alone
void residual_dev(pgx_handle* h, const double* x, double* F, int with_d, bool fu_only) {
  PhaseTimer t(h, 0);
  if (h->degree == 2) {
    pgxk_residual_p2_cells(h->st, h->nc, h->nd, h->cdofs, h->coords, h->mask, h->gbc, x, h->xk, h->alpha, h->f, h->q2,
                           h->p2_v2c_ptr, h->p2_v2c_ent, h->p2_stash, F, h->geoq);
    pgxk_residual_final(h->st, h->nd, h->mask, h->gbc, h->bphi, x, F);
    return;
  }
  // row-parallel, atomic-free, bitwise reproducible; with_d: also fills D(psi) at the same x (Newton driver)
  if (resid_grid_on(h)) {  // uniform structured mesh: LDS-staged element blocks
    // with_d == 2 (the Newton loop of a handle whose operator apply is matrix-free and whose preconditioner is the multigrid
    // cycle): the interior rows of D go to the stencil only - their CSR form (56 B per vertex, 235 MB at 2048^2) has no reader
    // until the next pgx_jacobian_fill / pgx_csr_export, which refill it (jac_valid is dropped at the end of the solve)
    pgxk_resid_fill_grid(h->st, with_d ? 1 : 0, h->lev[0], h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells,
                         h->coords, h->mask, h->gbc, h->bphi, x, h->xk, h->alpha, h->f, h->q, F, h->Dv, with_d, d_direct_on(h), h->colm,
                         fu_only ? 1 : 0);
    h->dh_interior = with_d != 0;  // the interior rows of the finest D stencil are in place (consumed by jacobian_dev(have_d))
    h->d0_direct = with_d != 0 && d_direct_on(h);  // ... and its frame rows, Dd4 and Dq with them
    if (with_d == 2) h->dv_lean = true;
    if (with_d == 1) h->dv_lean = false;  // a full fill of the CSR rows too
    return;
  }
  pgxk_resid_fill_p1(h->st, with_d, h->n, h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells,
                     h->coords, h->mask, h->gbc, h->bphi, x, h->xk, h->alpha, h->f, h->q, F, h->Dv, h->geoq);
}

// have_d: D(psi) at this x was already produced by residual_dev(..., with_d=1)
static int jacobian_dev(pgx_handle* h, const double* x, bool have_d = false) {
  if (!(have_d && h->degree == 1)) {
    PhaseTimer t(h, 1);
    if (h->degree == 2) {
      pgxk_fill_rows_p2(h->st, 2, h->nd, h->s_fill_lds, h->s_rowptr, h->p2_v2c_ptr, h->p2_v2c_ent, h->p2_v2c_pos,
                        h->cdofs, h->coords, x + h->nd, h->q2, h->s_D, h->geoq);
      // Galerkin coarse block T^T D_P2 T == D in the P1 basis with the P2 psi (same quadrature), for the P1 hierarchy
      pgxk_fill_rows_p1_Dp2(h->st, h->n, h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cdofs, h->coords,
                            x + h->nd, h->q2, h->Dv, h->geoq);
    } else if (resid_grid_on(h)) {
      // uniform structured mesh: D(psi) comes from the same element kernel the Newton driver uses (its residual output goes to
      // scratch), so pgx_jacobian_fill + pgx_csr_export put THAT kernel under the entry-wise oracle comparison of the parity tests
      pgxk_resid_fill_grid(h->st, 1, h->lev[0], h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells, h->coords,
                           h->mask, h->gbc, h->bphi, x, h->xk, h->alpha, h->f, h->q, h->w, h->Dv, 1, d_direct_on(h), h->colm);
      h->dh_interior = true;
      h->d0_direct = d_direct_on(h);
      h->dv_lean = false;  // a full fill: CSR rows and stencil
      have_d = true;
    } else {
      pgxk_fill_rows(h->st, 2, h->n, h->fill_lds, h->rowptr, h->v2c_ptr, h->v2c_ent, h->v2c_pos, h->cells, h->coords,
                     x + h->n, h->q, h->Dv, h->geoq);
    }
  }
  if (h->structured) {
    PhaseTimer t(h, 2);
    // direct: the kernels that computed D(psi) stored Dh (frame too), Dd4 and Dq of level 0 - nothing to convert or repack here
    const bool direct = d_direct_on(h);
    const bool d0 = direct && have_d && h->dh_interior && h->d0_direct;
    if (!d0)
      pgxk_csr_to_stencil_h(h->st, h->n, h->nx + 1, h->rowptr, h->colm, h->Dv, h->lev[0].Dh,
                            (have_d && h->degree == 1 && h->dh_interior) ? h->lev[0].ny : 0);
    h->dh_interior = false;
    h->d0_direct = false;
    if (h->lev[0].Dh32) pgxk_to_float(h->st, (size_t)4 * h->n, h->lev[0].Dh, h->lev[0].Dh32);
    if (h->lev[0].f32 && !d0) pgxk_f_pack_d(h->st, h->lev[0]);
    if (h->lev[0].Dd4 && !d0) pgxk_pack_d4(h->st, h->lev[0]);
    const int ld = h->dist.on ? h->dist.ldist : 0;
    for (size_t l = 1; l < h->lev.size(); ++l) {
      if (h->dist.on && (int)l == ld) {  // strip -> replicated level: owned rows + zeros, summed over the ranks
        const Dist& D = h->dist;
        const GridLevel& G = h->lev[l];
#ifdef PGX_DSTEN_FLOAT  // measurement build only (fp32 multigrid D stencils): the merge of the replicated level is fp64
        h->err = "PGX_DSTEN_FLOAT builds do not support sharded handles";
        return PGX_EINVAL;
#else
        pgxk_rap7h(h->st, h->lev[l - 1], h->lev[l - 1].Dh, D.view, D.view_S);
        pgxk_view_to_global(h->st, 4, D.view.n, G.n, G.nx + 1, D.view_row0, D.view_own0, D.view_H, D.view_S, G.Dh);
        const int rc = allreduce_dev(h, G.Dh, (size_t)4 * G.n);
        if (rc) return rc;
#endif
      } else {
        // direct: Dq of the coarse level leaves with its values; large levels coarsen from fine stencils staged in LDS
        pgxk_rap7h(h->st, h->lev[l - 1], h->lev[l - 1].Dh, h->lev[l], h->lev[l].Dh, direct, direct && h->lev[l].n >= h->rap_lds_min);
        if (direct) continue;
      }
      if (h->lev[l].f32) pgxk_f_pack_d(h->st, h->lev[l]);
    }
  }
  // refined general mesh: D(psi) of every coarse level from the full level-0 CSR values (K and M were coarsened by pgx_set_hierarchy);
  // not where nothing reads it: under PGX_UMG=0, and in a Newton solve that preconditions with the sparse LU
  for (size_t l = 1; umg_on(h) && !h->umg_idle && l < h->umg.size(); ++l) {
    PhaseTimer t(h, 2);
    const UmgLevel& C = h->umg[l];
    if (C.P_val)  // a built hierarchy (pgx_build_hierarchy): general weights, two gather stages
      pgxk_amg_rap(h->st, C, h->umg[l - 1].D, C.D);
    else
      pgxk_umg_rap(h->st, C.nnz, C.plan_lpe, C.plan_ptr, C.plan_src, h->umg[l - 1].D, C.D);
  }
  h->jac_valid = true;
  h->jac_ever = true;
  h->patch_fresh = false;
  h->p2st.fresh = false;
  return PGX_OK;
}

// Structured P2 operator apply (pgx_p2st.hip).  First use: the K / M constants of the reference group, checked on every interior
// group; once per Jacobian: the structure-of-arrays copies of D(psi).  Returns false when the CSR kernels have to do the work.
bool p2st_ready(pgx_handle* h) {
  pgx_handle::P2St& S = h->p2st;
  if (S.state == 0 || !S.select || (h->dist.on && !S.dist_enable) || !h->s_K || !h->s_D) return false;  // strips too (PGX_P2_STENCIL_DIST=0: CSR kernel there)
  static const int nt[4] = {19, 9, 9, 9}, off[4] = {0, 19, 28, 37};
  const size_t G = (size_t)h->n;  // groups = vertices
  if (S.state == 1) {
    S.state = 0;  // until everything below has succeeded
    const std::vector<int32_t>& rp = h->s_h_rowptr;
    double kmax = 0.0, mmax = 0.0;
    for (int t = 0; t < 4; ++t) {
      const int p = rp[S.ref_rows[t]];
      if (hipMemcpy(S.K + off[t], h->s_K + p, sizeof(double) * nt[t], hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(S.tab.M + off[t], h->s_M + p, sizeof(double) * nt[t], hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    }
    for (int e = 0; e < 46; ++e) kmax = std::max(kmax, std::fabs(S.K[e])), mmax = std::max(mmax, std::fabs(S.tab.M[e]));
    S.tab.kmax = kmax, S.tab.mmax = mmax;
    for (int e = 0; e < 46; ++e) S.tab.aK[e] = S.K[e];
    int* d_fail = nullptr;
    if (hipMalloc((void**)&d_fail, sizeof(int)) != hipSuccess) return false;
    hipMemsetAsync(d_fail, 0, sizeof(int), h->st);
    pgxk_p2st_check(h->st, S.tab, h->nx, h->n, S.i0, S.ni, S.j0, S.nj, 1.0, 1e-12, h->s_rowptr, h->s_K, h->s_M, d_fail);
    int fail = 1;
    const hipError_t e1 = hipMemcpyAsync(&fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, h->st);
    const hipError_t e2 = hipStreamSynchronize(h->st);
    hipFree(d_fail);
    if (e1 != hipSuccess || e2 != hipSuccess || fail) return false;  // not the uniform mesh the table assumes: CSR kernels
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(double) * 46 * G) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    h->allocs.push_back(q);
    S.Dst = (double*)q;
    if (h->p2_resid_f32) {
      if (hipMalloc(&q, sizeof(float) * 46 * G) == hipSuccess) {
        h->allocs.push_back(q);
        S.Dstf = (float*)q;
      } else {
        (void)hipGetLastError();
      }
    }
    S.state = 2;
  }
  if (!S.fresh) {
    pgxk_p2st_pack(h->st, h->nx, h->n, S.i0, S.ni, S.j0, S.nj, G, h->s_rowptr, h->s_D, S.Dst, 0);
    if (S.Dstf) pgxk_p2st_pack(h->st, h->nx, h->n, S.i0, S.ni, S.j0, S.nj, G, h->s_rowptr, h->s_D, S.Dstf, 1);
    S.fresh = true;
  }
  for (int e = 0; e < 46; ++e) S.tab.aK[e] = h->alpha * S.K[e];
  return true;
}
// y = J x (bu == nullptr) or y = b - J x; inner: a residual inside the preconditioner (may read the float copy of D)
void p2st_apply(pgx_handle* h, const double* xu, const double* xp, const double* bu, const double* bp, double* yu, double* yp,
                bool inner) {
  pgx_handle::P2St& S = h->p2st;
  const bool f32 = inner && S.Dstf;
  pgxk_p2st_apply(h->st, S.tab, h->nx, h->n, S.i0, S.ni, S.j0, S.nj, (size_t)h->n, f32 ? (const void*)S.Dstf : (const void*)S.Dst, f32, xu,
                  xp, bu, bp, yu, yp);
  pgxk_p2_rows_csr(h->st, S.nframe, S.frame, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_D, h->alpha, h->mask, xu, xp, bu, bp, yu, yp);
}

// y = J x on device vectors of length 2*nd
void spmv_dev(pgx_handle* h, const double* x, double* y) {
  if (h->degree == 2 && h->spmv_stream && h->spmv_bal && p2st_ready(h)) {
    static PgxTuneInt bench_inner("PGX_P2ST_BENCH_INNER", 0);  // measurement hook (tools/p2_spmv_bench.py): time the float-D form
    p2st_apply(h, x, x + h->nd, nullptr, nullptr, y, y + h->nd, bench_inner.get() != 0);
    return;
  }
  if (h->spmv_stencil && h->structured && h->degree == 1) {
    if (h->spmv_stencil == 2)  // A/B: the generic one-thread-per-vertex stencil kernel
      level_apply(h, 0, 0, x, x + h->nd, nullptr, nullptr, 0.0, 0, y, y + h->nd);
    else
      pgxk_st_spmv(h->st, h->lev[0], h->alpha, x, x + h->nd, h->xcd_remap ? 1 : 0, y, y + h->nd);
    return;
  }
  if (h->spmv_stream && h->spmv_bal && h->s_blk)
    pgxk_bspmv_bal(h->st, h->nd, h->s_nblk, h->s_blk, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_code, h->s_tab, h->s_D, h->alpha, h->mask, x,
                   x + h->nd, nullptr, nullptr, h->xcd_remap ? 1 : 0, y, y + h->nd);
  else if (h->spmv_stream && 2 * h->s_fill_lds <= 100 * 1024)
    pgxk_bspmv_stream(h->st, h->nd, h->s_fill_lds, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_D, h->alpha, h->mask, x,
                      x + h->nd, h->xcd_remap ? 1 : 0, y, y + h->nd);
  else
    pgxk_bspmv(h->st, 0, h->nd, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_D, h->alpha, x, x + h->nd, nullptr,
               nullptr, 0.0, h->xcd_remap, y, y + h->nd);
}

// ------------------------------------------------------------------------------------------------
// C ABI: fine-grained calls
// ------------------------------------------------------------------------------------------------
extern "C" int pgx_residual(pgx_handle* h, const double* x, double* F, double* fnorm) {
  NEED(h);
  const double* xd = h->x;
  if (x) {
    int rc = copy_in(h, h->xw, x);
    if (rc) return rc;
    xd = h->xw;
  }
  residual_dev(h, xd, h->F);
  if (fnorm) {
    int rc;
    if (h->dist.on) {  // collective: 2-norm over the owned entries of all ranks
      gather_owned(h, h->F, h->dist.wc);
      rc = dev_norm(h, h->dist.wc, fnorm, 2 * h->dist.nk_field());
    } else {
      rc = dev_norm(h, h->F, fnorm);
    }
    if (rc) return rc;
  }
  if (F) return copy_out(h, F, h->F);
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}

extern "C" int pgx_jacobian_fill(pgx_handle* h, const double* x) {
  NEED(h);
  const double* xd = h->x;
  if (x) {
    int rc = copy_in(h, h->xw, x);
    if (rc) return rc;
    xd = h->xw;
  }
  {
    const int rc = jacobian_dev(h, xd);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  return PGX_OK;
}

extern "C" int pgx_csr_export(pgx_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* K,
                              double* M, double* D) {
  NEED(h);
  const std::vector<int32_t>& hr = (h->degree == 2) ? h->s_h_rowptr : h->h_rowptr;
  const std::vector<int32_t>& hc = (h->degree == 2) ? h->s_h_col : h->h_col;
  if (nrows) *nrows = h->nd;
  if (nnz) *nnz = h->s_nnz;
  if (rowptr) memcpy(rowptr, hr.data(), sizeof(int32_t) * (h->nd + 1));
  if (col) memcpy(col, hc.data(), sizeof(int32_t) * h->s_nnz);
  if (K) HIPCHK(hipMemcpy(K, h->s_K, sizeof(double) * h->s_nnz, hipMemcpyDeviceToHost));
  if (M) HIPCHK(hipMemcpy(M, h->s_M, sizeof(double) * h->s_nnz, hipMemcpyDeviceToHost));
  if (D) {
    if (!h->jac_valid) {
      h->err = "pgx_csr_export(D) before pgx_jacobian_fill";
      return PGX_ESTATE;
    }
    HIPCHK(hipMemcpy(D, h->s_D, sizeof(double) * h->s_nnz, hipMemcpyDeviceToHost));
  }
  return PGX_OK;
}

extern "C" int pgx_spmv(pgx_handle* h, const double* x, double* y) {
  NEED(h);
  if (!x || !y) return PGX_EINVAL;
  if (!h->jac_valid) {
    h->err = "pgx_spmv before pgx_jacobian_fill";
    return PGX_ESTATE;
  }
  int rc = copy_in(h, h->V, x);
  if (rc) return rc;
  if (h->dist.on && (rc = halo_solution(h, h->V, h->V + h->nd))) return rc;  // ghost entries from their owners
  spmv_dev(h, h->V, h->w);
  return copy_out(h, y, h->w);  // owned rows are J x of the GLOBAL operator; ghost rows are not meaningful
}

extern "C" int pgx_observables(pgx_handle* h, double out[6]) {
  NEED_KEEP(h);
  if (!out) return PGX_EINVAL;
  {
    PhaseTimer t(h, 6);
    if (h->degree == 2 && !h->dist.on) {
      pgxk_observables_p2_cells(h->st, h->nc, h->nd, h->cdofs, h->coords, h->x, h->xk, h->alpha, h->f, h->q2,
                                h->obs_partials, h->obs_blocks, h->geoq);
      pgxk_observables_final(h->st, h->obs_blocks, h->obs_partials, h->d_out6);
    } else if (h->dist.on && h->degree == 2) {
      const Dist& D = h->dist;  // P2 on a strip: the owned cells' partial sums, one packed all-reduce (raw sums, as below)
      pgxk_observables_p2_cells(h->st, D.ncell_own, h->nd, h->cdofs + 6 * (size_t)D.cell0, h->coords, h->x, h->xk, h->alpha, h->f,
                                h->q2, h->obs_partials, pgxk_observables_blocks(D.ncell_own));
      pgxk_observables_final_raw(h->st, pgxk_observables_blocks(D.ncell_own), h->obs_partials, h->d_out6);
      const int rc = allreduce_dev(h, h->d_out6, 6);
      if (rc) return rc;
    } else if (h->dist.on) {
      // owned cells only (a contiguous range in row-major cell order), raw sums, ONE packed all-reduce for the six
      // scalars (the reference all-reduces each one separately, obstacle_pg.py:196-201), then abs / sqrt
      const Dist& D = h->dist;
      pgxk_observables(h->st, D.ncell_own, h->n, h->cells + 3 * (size_t)D.cell0, h->coords, h->x, h->xk, h->alpha, h->f,
                       h->q, h->obs_partials, pgxk_observables_blocks(D.ncell_own), h->d_out6, 1);
      const int rc = allreduce_dev(h, h->d_out6, 6);
      if (rc) return rc;
    } else {
      pgxk_observables(h->st, h->nc, h->n, h->cells, h->coords, h->x, h->xk, h->alpha, h->f, h->q, h->obs_partials,
                       h->obs_blocks, h->d_out6, 0, h->geoq);
    }
  }
  {
    int rcb = replica_check(h, h->d_out6, 6, "the observables");  // fixed-shape reductions: identical on every replica
    if (!rcb) rcb = replica_agree(h, h->d_out6, 6);                // the stopping test of the proximal loop reads these
    if (rcb) return rcb;
  }
  {
    const int rcf = fetch_small(h, h->d_out6, 6);
    if (rcf) return rcf;
  }
  for (int k = 0; k < 6; ++k) out[k] = h->h_small[k];
  if (h->dist.on) {
    out[1] = std::fabs(out[1]);
    out[4] = std::sqrt(out[4]);
    out[5] = std::sqrt(out[5]);
  }
  return PGX_OK;
}

extern "C" int pgx_resid_reuse_counts(pgx_handle* h, int64_t out[2], int reset) {
  if (!h || !out) return PGX_EINVAL;
  out[0] = h->entry_full;
  out[1] = h->entry_reduced;
  if (reset) h->entry_full = h->entry_reduced = 0;
  return PGX_OK;
}

extern "C" int pgx_profile_enable(pgx_handle* h, int on) {
  if (!h) return PGX_EINVAL;
  h->prof = on != 0;
  return PGX_OK;
}
extern "C" int pgx_profile_get(pgx_handle* h, double ms[8], int reset) {
  if (!h || !ms) return PGX_EINVAL;
  for (int k = 0; k < 8; ++k) ms[k] = h->ms[k];
  if (reset)
    for (int k = 0; k < 8; ++k) h->ms[k] = 0.0;
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// Newton driver: SNES newtonls + linesearch none (full step) convergence logic, SURVEY.md App. A.4;
// options of obstacle_pg.py:128-139; "copy back only if converged" of lvpp/problem.py:121-123.
// ------------------------------------------------------------------------------------------------
extern "C" int pgx_newton_solve(pgx_handle* h, const pgx_snes_opts* opts, int* reason, int* its_out, int* lin_out) {
  NEED_KEEP(h);
  if (!opts || !reason) return PGX_EINVAL;
  pgx_snes_opts optv = *opts;
  // auto: chosen so that the final primal field stays within 1e-10 of the LU oracle on EVERY case measured
  // (tools/lu_accuracy_check.py, tools/tolerance_sweep.py): small / unstructured meshes are the sensitive ones
  if (!(optv.ksp_rtol > 0.0)) optv.ksp_rtol = (h->degree == 2) ? 1e-11 : 1e-10;
  opts = &optv;
  // pc_type: 0 auto (geometric multigrid for P1 on a structured mesh; sparse LU for P2, whose two-level cycle is not robust
  // on the late large-alpha systems, and for general meshes, which have no grid hierarchy - e.g. the reference's own gmsh
  // disk, obstacle_pg.py:64-65), 1 multigrid V-cycle, 2 sparse LU (what the reference asks PETSc/MUMPS for)
  // P2 on a structured mesh (round 3): the two-level cycle with the vertex-star patch smoother first (pcycle_p2_patch: 8-20
  // iterations per Newton step at every size, a fifth of a factorisation's time) and the sparse LU only for a Newton solve in
  // which that cycle stagnates - the overshot iterates of settings B's large alpha jumps, where exp(psi) is rough on the mesh
  // scale; the LU then stays in place for the rest of that pgx_newton_solve call.
  // P2 on a refined general mesh with its hierarchy attached: the same, from umg_min_p2 vertices up (the coarse solve is vcycle_umg)
  const bool p2_hier = h->structured ? h->lev.size() > 1 : (umg_on(h) && h->n >= h->umg_min_p2);
  const bool mg_first = optv.pc_type == 0 && h->degree == 2 && p2_hier && h->patch_nn && h->p2_patch && !h->dist.on && !h->lu_comm;
  // a refined general mesh with its hierarchy attached (pgx_set_hierarchy): auto takes the multilevel cycle from umg_min vertices up
  const bool umg_auto = h->degree == 1 && umg_on(h) && h->n >= h->umg_min;
  bool use_lu = h->lu_comm || optv.pc_type == 2 ||
                (optv.pc_type == 0 && (h->degree == 2 || !h->structured) && !h->dist.on && !mg_first && !umg_auto);
  h->lu_active = false;
  if (use_lu) {
    int rcl = ensure_lu(h);
    if (rcl) return rcl;
  }
  // Sharded P2 has no sparse-LU rescue (the factorisation is not sharded): where the single handle would switch to it - the
  // overshot iterates of settings B, on which the patch cycle needs a few hundred iterations instead of ten - the sharded solve
  // keeps iterating on its un-restarted basis (up to 300 vectors).  512^2 settings B on 4 strips: the golden's Newton counts
  // 5,4,3,2,1,1,4,1 (tests/test_gpu_sharded.py).
  // sharded P2 has no sparse-LU fallback for a stagnating two-level cycle: it runs the Krylov method longer instead - but only where
  // the caller left the default (an explicit ksp_max_it is the caller's decision; include/pgx.h)
  if (h->dist.on && h->degree == 2 && optv.ksp_max_it == 200) optv.ksp_max_it = 400;
  const size_t n2 = 2 * (size_t)h->nd;
  PgxSolveScope scope(h->st, h->prof, &h->lu_active);
  // EVERY way out of the Newton loop - also the early `return rc` of a failed Krylov solve, halo exchange or replica check - leaves
  // a hierarchy whose finest D(psi) was refreshed in passing (and, lean, CSR rows that were not): no export / CSR product of a
  // matrix that mixes iterates afterwards
  struct JacStale {
    pgx_handle* h;
    ~JacStale() {
      if (h->dh_interior || h->dv_lean || umg_on(h)) h->jac_valid = false;  // (the coarse D of a general-mesh hierarchy: stale too)
      h->umg_idle = false;
    }
  } jac_stale{h};
  h->umg_idle = use_lu;  // set again where a degree-2 solve switches to the LU (the rescue below): nothing reads the coarse D after it
  PgxRange range("pgx:newton_solve");
  int its = 0, lin = 0, rsn = 0;
  double fnorm = 0, fnorm0 = 0, ttol = 0;
  h->omega_now = 0.0;
  h->v_f32_off = false;
  int rc = PGX_OK;
  // Sharded: x, xw, dx, F are local vectors (owned + ghost rows); norms run on owned-compact copies (rhs doubles as the
  // compact copy of F), and the ghost rows of the iterate are refreshed after every update, before the next assembly.
  const bool dist = h->dist.on;
  const size_t nk = dist ? 2 * h->dist.nk_field() : n2;
  auto owned_norm = [&](const double* v, double* out) -> int {
    if (!dist) return dev_norm(h, v, out);
    gather_owned(h, v, h->dist.wc);
    return dev_norm(h, h->dist.wc, out, nk);
  };
  // matrix-free operator + multigrid preconditioner: nobody reads the CSR form of D inside this solve (see residual_dev)
  const int with_d = (!use_lu && !mg_first && h->degree == 1 && h->structured && h->spmv_stencil == 1 && h->lean_d) ? 2 : 1;
  // entry evaluation: where the solve before ended at this x in this mode and nothing touched its results since (pgx_handle::fresh),
  // F_psi and D(psi) are in place and only F_u is evaluated.  The stamp is dropped here and set again at the end of a converged solve,
  // so every other way out - diverged, out of iterations, an early `return rc` - leaves it dropped
  const bool reuse_ok = resid_reuse_on(h) && !use_lu;
  const bool fu_only = reuse_ok && h->fresh.valid && h->fresh.with_d == with_d && h->fresh.dh_interior == h->dh_interior &&
                       h->fresh.d0_direct == h->d0_direct && h->fresh.dv_lean == h->dv_lean;
  h->fresh.valid = false;
  ++(fu_only ? h->entry_reduced : h->entry_full);
  pgxk_scale_copy(h->st, n2, 1.0, h->x, h->xw);
  residual_dev(h, h->xw, h->F, with_d, fu_only);
  if ((rc = replica_check(h, h->F, n2, "the residual"))) return rc;
  if (dist) {
    gather_owned(h, h->F, h->rhs);
    rc = dev_norm(h, h->rhs, &fnorm, nk);
  } else {
    rc = dev_norm(h, h->F, &fnorm);
  }
  if (rc) return rc;
  fnorm0 = fnorm;
  if (opts->monitor) printf("  0 SNES Function norm %.12e\n", fnorm);
  if (!std::isfinite(fnorm))
    rsn = PGX_SNES_DIVERGED_FNORM_NAN;
  else if (fnorm < opts->snes_atol)
    rsn = PGX_SNES_CONVERGED_FNORM_ABS;
  ttol = fnorm * opts->snes_rtol;
  while (rsn == 0) {
    if (its >= opts->snes_max_it) {
      rsn = PGX_SNES_DIVERGED_MAX_IT;
      break;
    }
    rc = jacobian_dev(h, h->xw, true);
    if (rc) return rc;
    if (use_lu) {
      if ((rc = lu_factor(h))) return rc;
      h->lu_active = true;
    }
    // lean: fgmres takes F itself and the sign (V_0 = (-1 / beta) F, residuals -F - J x): no pass that forms rhs = -F
    const bool lean_rhs = h->lean_rhs && !use_lu && !mg_first && krylov_lean(h);
    if (!lean_rhs) pgxk_scale_copy(h->st, nk, -1.0, dist ? h->rhs : h->F, h->rhs);
    int kits = 0;
    double relres = 0;
    if (mg_first && !use_lu) {
      pgx_snes_opts ol = optv;
      ol.ksp_max_it = std::min(optv.ksp_max_it, h->p2_fallback_its);
      rc = fgmres(h, h->rhs, h->dx, &ol, &kits, &relres, fnorm);
      if (rc) return rc;
      // stagnation = the iteration cap was reached without convergence (an early exit at the attainable accuracy, a few 1e-10
      // after 10-15 iterations on the late systems, is not): factorise, and keep the factorisation for this solve
      if (kits >= ol.ksp_max_it && !(relres <= 10.0 * optv.ksp_rtol)) {
        if (opts->monitor) printf("    KSP (patch multigrid) %d its, rel residual %.3e: sparse LU for the rest of this solve\n", kits, relres);
        lin += kits;
        if ((rc = ensure_lu(h))) return rc;
        if ((rc = lu_factor(h))) return rc;
        h->lu_active = true;
        use_lu = true;
        h->umg_idle = true;
        ++h->p2_fallbacks;
        rc = fgmres(h, h->rhs, h->dx, opts, &kits, &relres, fnorm);
        if (rc) return rc;
      }
    } else {
      rc = lean_rhs ? fgmres(h, h->F, h->dx, opts, &kits, &relres, fnorm, -1.0) : fgmres(h, h->rhs, h->dx, opts, &kits, &relres, fnorm);
      if (rc) return rc;
    }
    lin += kits;
    ++its;
    if (opts->monitor) printf("    KSP its %d  rel residual %.3e\n", kits, relres);
    if (!(relres <= std::max(opts->ksp_rtol, 1e-7)) || !std::isfinite(relres)) {
      rsn = PGX_SNES_DIVERGED_LINEAR_SOLVE;
      break;
    }
    // xw += dx; fused: the same pass leaves the block sums of |dx|^2 and |xw|^2 (partials2: nothing else in the Newton loop uses
    // it) for the step test below, which then needs one read-back and no further pass.  On the ticket route the last block of the
    // step's launch publishes the two sums to h_small[2], [3] (the residual norm read back in between takes h_small[0]) and the host
    // reads them below, behind the wait for that norm, without a launch or a wait more; the launch of its own comes after that norm
    // and takes h_small[0], [1]
    const PgxRoute step_route = read_back_route(h);
    const bool fstep = h->fused_step && step_route != PGX_RB_PLAIN && !use_lu && !mg_first && krylov_lean(h);
    const size_t step_off = step_route == PGX_RB_TICKET ? 2 : 0;
    const PgxReadBack step_rb{pgxk_multidot_blocks(n2), h->partials2, 2, h->d_small + step_off, step_off};
    PgxPending step_pending{};
    if (fstep)
      step_pending = read_back_start(h, step_rb, step_route, [&](PgxTicket* tk, double* out) {
        pgxk_axpy_norms(h->st, n2, h->dx, h->xw, h->partials2, out, tk);
        return true;
      });
    else
      pgxk_axpy(h->st, n2, 1.0, h->dx, h->xw);
    if (dist && (rc = halo_solution(h, h->xw, h->xw + h->nd))) return rc;
    residual_dev(h, h->xw, h->F, with_d);
    if ((rc = replica_check(h, h->F, n2, "the residual"))) return rc;
    if (dist) {
      gather_owned(h, h->F, h->rhs);
      rc = dev_norm(h, h->rhs, &fnorm, nk);
    } else {
      rc = dev_norm(h, h->F, &fnorm);
    }
    if (rc) return rc;
    if (opts->monitor) printf("  %d SNES Function norm %.12e\n", its, fnorm);
    if (!std::isfinite(fnorm)) {
      rsn = PGX_SNES_DIVERGED_FNORM_NAN;
    } else if (fnorm < opts->snes_atol) {
      rsn = PGX_SNES_CONVERGED_FNORM_ABS;
    } else if (fnorm <= ttol) {
      rsn = PGX_SNES_CONVERGED_FNORM_RELATIVE;
    } else {
      double snorm, xnorm;
      if (fstep) {
        if ((rc = read_back_finish(h, step_rb, step_pending))) return rc;
        snorm = std::sqrt(h->h_small[step_off]);
        xnorm = std::sqrt(h->h_small[step_off + 1]);
      } else {
        rc = owned_norm(h->dx, &snorm);
        if (rc) return rc;
        rc = owned_norm(h->xw, &xnorm);
        if (rc) return rc;
      }
      if (snorm < opts->snes_stol * xnorm)
        rsn = PGX_SNES_CONVERGED_SNORM_RELATIVE;
      else if (fnorm > opts->snes_divtol * fnorm0)
        rsn = PGX_SNES_DIVERGED_DTOL;
    }
  }
  h->lu_active = false;
  if (rsn > 0) pgxk_scale_copy(h->st, n2, 1.0, h->xw, h->x);
  // the last residual evaluation refreshed D(psi) at the final iterate on the finest level only (k_resid_fill_grid writes
  // the interior rows of its stencil in passing): the hierarchy no longer describes ONE matrix until the next fill
  if (h->dh_interior || h->dv_lean) h->jac_valid = false;
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());  // a failed kernel launch anywhere in the solve must not pass silently
  // converged: x is the iterate of the last residual_dev, whose F_psi and D copies the next solve's entry evaluation can take over
  if (rsn > 0 && reuse_ok && h->dh_interior) h->fresh = {true, with_d, h->dh_interior, h->d0_direct, h->dv_lean};
  if (h->prof) h->ms[7] += scope.stop();
  *reason = rsn;
  if (its_out) *its_out = its;
  if (lin_out) *lin_out = lin;
  return PGX_OK;
}
