// What libpgx.so offers to tests and measurements and pgx_newton_solve never reaches: exports of what the preconditioner stores, single
// cycles and cycle stages entered through the functions the solver itself calls (pgx_cycle.hip), the kernel benchmarks, the counters
// and the self-checks.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pgx_handle.h"

extern "C" int pgx_smoother_bench(pgx_handle* h, int reps, double* avg_ms, double* bytes) {
  NEED(h);
  if (reps < 1 || !avg_ms) return PGX_EINVAL;
  if (!h->jac_valid || !h->structured || h->lev.size() < 2 || h->dist.on) {
    h->err = "pgx_smoother_bench needs a structured single-GPU handle with a grid hierarchy and a filled Jacobian";
    return PGX_ESTATE;
  }
  if (h->degree == 2) {
    // P2: the time-dominant kernel is the patch sweep (k_patch_apply + k_patch_edges) on the current Jacobian's inverses
    if (!h->patch_nn || !h->p2_patch) {
      h->err = "pgx_smoother_bench (P2): no patch smoother on this handle";
      return PGX_ESTATE;
    }
    const int rcp = ensure_patches(h);
    if (rcp) return rcp;
    const int nd = h->nd, nv = h->n, NN = h->patch_nn, P = 2 * NN;
    pgxk_set(h->st, 2 * (size_t)nd, 1.0, h->rhs);
    HIPCHK(hipMemsetAsync(h->w, 0, sizeof(double) * 2 * nd, h->st));
    auto sweep = [&]() { p2_cycle_patch(h, h->rhs, h->rhs + nd, h->w, h->w + nd); };
    for (int k = 0; k < 3; ++k) sweep();
    HIPCHK(hipEventRecord(h->e0, h->st));
    for (int k = 0; k < reps; ++k) sweep();
    HIPCHK(hipEventRecord(h->e1, h->st));
    HIPCHK(hipEventSynchronize(h->e1));
    float msp = 0;
    HIPCHK(hipEventElapsedTime(&msp, h->e0, h->e1));
    *avg_ms = (double)msp / reps;
    if (bytes) {
      // per patch: the inverse, the dof table, the residual at its 2 NN dofs (read once: every dof is gathered by its patches out
      // of L2, HBM sees each value once -> 16 B per dof), the vertex iterate read + written, the parked edge contributions; per edge
      // (k_patch_edges): the two parked pairs read, the edge iterate read + written
      const double inv = (double)pgxk_patch_inverse_bytes(nv, NN, h->patch_f32, h->patch_sym);
      const double ne = (double)(nd - nv);
      *bytes = inv + 4.0 * NN * nv + 16.0 * nd + 32.0 * nv + 2.0 * 2.0 * 4.0 * ne + (16.0 + 32.0) * ne;
    }
    (void)P;
    return PGX_OK;
  }
  GridLevel& L = h->lev[0];
  GridLevel& C = h->lev[1];
  const size_t n = (size_t)L.n;
  // right-hand side and iterate: any finite data (the kernel's cost does not depend on the values); coarse correction zero
  pgxk_set(h->st, 2 * n, 1.0, h->rhs);
  pgxk_set(h->st, 2 * n, 0.5, h->w);
  HIPCHK(hipMemsetAsync(C.xu, 0, sizeof(double) * C.n, h->st));
  HIPCHK(hipMemsetAsync(C.xp, 0, sizeof(double) * C.n, h->st));
  const int remap = h->xcd_remap ? 1 : 0;
  const bool f32 = f32_cycle_ok(h, 0, 6);
  if (f32) {  // the single-precision launch of the same role: 3 sweeps on x + P x_c, float2 in and out
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)L.bf, 0x3f800000, 2 * n, h->st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)L.xf, 0x3f000000, 2 * n, h->st));
    if (C.f32) HIPCHK(hipMemsetAsync(C.xf, 0, sizeof(float2) * C.n, h->st));
  }
  auto run = [&]() {
    if (f32)
      pgxk_f_smooth(h->st, 3, 0, L, h->alpha, L.xf, nullptr, nullptr, &C, C.f32 ? C.xf : nullptr, C.f32 ? nullptr : C.xu,
                    C.f32 ? nullptr : C.xp, 0.8, remap, L.xf2, nullptr, nullptr);
    else
      pgxk_st_smoothK(h->st, 3, 1, L, h->alpha, h->w, h->w + n, &C, C.xu, C.xp, h->rhs, h->rhs + n, 0.8, remap, h->tmp_u, h->tmp_p);
  };
  for (int k = 0; k < 3; ++k) run();
  HIPCHK(hipEventRecord(h->e0, h->st));
  for (int k = 0; k < reps; ++k) run();
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipEventSynchronize(h->e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  *avg_ms = (double)ms / reps;
  if (bytes)  // D stencil + right-hand side + iterate + coarse correction + result
    *bytes = f32 ? ((L.dbf16 ? 8.0 : 16.0) * n + 8.0 * n + 8.0 * n + (C.f32 ? 8.0 : 16.0) * C.n + 8.0 * n) : 8.0 * (4.0 * n + 2.0 * n + 2.0 * n + 2.0 * C.n + 2.0 * n);
  return PGX_OK;
}

extern "C" int pgx_vcycle_bench(pgx_handle* h, int level, int reps, double* avg_ms, int* n_level) {
  NEED(h);
  if (reps < 1 || !avg_ms) return PGX_EINVAL;
  if (!h->jac_valid || !h->structured || h->lev.size() < 2 || h->dist.on || h->degree != 1) {
    h->err = "pgx_vcycle_bench needs a structured single-GPU P1 handle with a grid hierarchy and a filled Jacobian";
    return PGX_ESTATE;
  }
  if (level < 0) level = h->tail_start > 0 ? h->tail_start : (int)h->lev.size() - 1;
  if (level >= (int)h->lev.size()) return PGX_EINVAL;
  pgx_snes_opts od;
  pgx_default_opts(&od);
  GridLevel& L = h->lev[level];
  double *bu = level == 0 ? h->rhs : L.bu, *bp = level == 0 ? h->rhs + L.n : L.bp;
  double *xu = level == 0 ? h->w : L.xu, *xp = level == 0 ? h->w + L.n : L.xp;
  pgxk_set(h->st, (size_t)L.n, 1.0, bu);
  pgxk_set(h->st, (size_t)L.n, 1.0, bp);
  const bool f32 = level > 0 && f32_cycle_ok(h, level, od.mg_nu);  // a single-precision level below the finest: float2 right-hand side
  if (f32) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)L.bf, 0x3f800000, 2 * (size_t)L.n, h->st));
  auto run = [&]() {
    if (f32)
      vcycle_f(h, level, nullptr, nullptr, nullptr, nullptr, od.mg_nu, od.mg_omega);
    else
      vcycle(h, level, bu, bp, xu, xp, od.mg_nu, od.mg_omega);
  };
  for (int k = 0; k < 3; ++k) run();
  HIPCHK(hipEventRecord(h->e0, h->st));
  for (int k = 0; k < reps; ++k) run();
  HIPCHK(hipEventRecord(h->e1, h->st));
  HIPCHK(hipEventSynchronize(h->e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
  *avg_ms = (double)ms / reps;
  if (n_level) *n_level = L.n;
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// Test hooks (include/pgx.h): the stored multigrid operators of one level, and ONE V-cycle entered on one level, with the buffers and
// the call sequence of pgx_vcycle_bench / pgx_spmv_bench.  They launch nothing of their own besides copies.
// ------------------------------------------------------------------------------------------------
// p2_too: the export also serves structured P2 handles, whose levels are the P1 hierarchy below the P2 level
static int mg_hook_ready(pgx_handle* h, const char* who, bool p2_too = false) {
  const bool degree_ok = h->degree == 1 || (p2_too && h->degree == 2);
  if (!h->jac_valid || !h->structured || h->lev.size() < 2 || h->dist.on || !degree_ok || h->lu_active) {
    h->err = std::string(who) + " needs a structured single-GPU " + (p2_too ? "" : "P1 ") +
             "handle with a grid hierarchy, a filled Jacobian and the multigrid preconditioner";
    return PGX_ESTATE;
  }
  return PGX_OK;
}

extern "C" int pgx_mg_level_export(pgx_handle* h, int level, int* nx, int* ny, double* Dh4, float* Dq4, uint8_t* mask, int* f32,
                                   int* dbf16) {
  NEED(h);
  {
    const int rc = mg_hook_ready(h, "pgx_mg_level_export", true);
    if (rc) return rc;
  }
  if (level < 0 || level >= (int)h->lev.size()) {
    h->err = "pgx_mg_level_export: no such multigrid level";
    return PGX_EINVAL;
  }
  const GridLevel& L = h->lev[level];
  const size_t n = (size_t)L.n;
  if (nx) *nx = L.nx;
  if (ny) *ny = L.ny;
  if (f32) *f32 = L.f32;
  if (dbf16) *dbf16 = L.dbf16;
  HIPCHK(hipStreamSynchronize(h->st));
  if (Dh4) {
    std::vector<dsten_t> tmp(4 * n);
    HIPCHK(hipMemcpy(tmp.data(), L.Dh, sizeof(dsten_t) * 4 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 4 * n; ++i) Dh4[i] = (double)tmp[i];
  }
  if (Dq4 && L.f32 && L.Dq) {
    if (L.dbf16) {  // two packed bf16 pairs per vertex: a bf16 word is the upper half of the float with the same value
      std::vector<uint32_t> tmp(2 * n);
      HIPCHK(hipMemcpy(tmp.data(), L.Dq, sizeof(uint32_t) * 2 * n, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < 2 * n; ++i) {
        const uint32_t lo = tmp[i] << 16, hi = tmp[i] & 0xffff0000u;
        memcpy(Dq4 + 2 * i, &lo, sizeof(float));
        memcpy(Dq4 + 2 * i + 1, &hi, sizeof(float));
      }
    } else {
      HIPCHK(hipMemcpy(Dq4, L.Dq, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
    }
  }
  if (mask) HIPCHK(hipMemcpy(mask, L.mask, n, hipMemcpyDeviceToHost));
  return PGX_OK;
}

extern "C" int pgx_vcycle_apply(pgx_handle* h, int level, int nu, double omega, int in_form, int out_form, double scale, const double* b,
                                double* z) {
  NEED(h);
  {
    const int rc = mg_hook_ready(h, "pgx_vcycle_apply");
    if (rc) return rc;
  }
  const int nl = (int)h->lev.size();
  const int lmax = h->tail_start > 0 ? h->tail_start : nl - 1;
  if (!b || !z || nu < 1 || level < 0 || level > lmax || (in_form != 0 && in_form != 1) || (out_form != 0 && out_form != 1)) {
    h->err = "pgx_vcycle_apply: bad argument (levels 0 .. the first level of the fused tail, forms 0 or 1, nu >= 1)";
    return PGX_EINVAL;
  }
  GridLevel& L = h->lev[level];
  const size_t n = (size_t)L.n;
  const bool f32 = f32_cycle_ok(h, level, nu);
  if (L.f32 && h->fused_legs && level + 1 < nl && !f32) {
    h->err = "pgx_vcycle_apply: the single-precision legs of this level need an even nu, or a multiple of 3 with PGX_FUSED_K3";
    return PGX_EINVAL;
  }
  if ((in_form != 0 || out_form != 0 || scale != 1.0) && level != 0) {
    h->err = "pgx_vcycle_apply: input / output forms and the scale factor exist on level 0 only";
    return PGX_EINVAL;
  }
  if ((in_form != 0 || scale != 1.0) && !f32) {
    h->err = "pgx_vcycle_apply: the float right-hand side and the scale factor are read by the single-precision cycle only";
    return PGX_EINVAL;
  }
  if (out_form == 1 && !z_f32_active(h, nu)) {
    h->err = "pgx_vcycle_apply: the float2 result needs the handle's float2 Z storage (PGX_Z_F32, matrix-free apply, single-precision level 0)";
    return PGX_ESTATE;
  }
  if (level == 0) {
    // as fgmres / pgx_spmv_bench enter the preconditioner: right-hand side in h->rhs, result in h->w or, float2, at the head of h->Z
    int rc = copy_in(h, h->rhs, b);
    if (rc) return rc;
    float* b32 = nullptr;
    if (in_form == 1) {
      std::vector<float> hb(2 * n);
      for (size_t i = 0; i < 2 * n; ++i) hb[i] = (float)b[i];
      if (hipMalloc(&b32, sizeof(float) * 2 * n) != hipSuccess) {
        h->err = "pgx_vcycle_apply: out of device memory";
        return PGX_ENOMEM;
      }
      if (hipMemcpy(b32, hb.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(b32);
        h->err = "pgx_vcycle_apply: copy of the float right-hand side failed";
        return PGX_EHIP;
      }
    }
    float2* const zf = out_form == 1 ? reinterpret_cast<float2*>(h->Z) : nullptr;
    h->rhs_scale = scale;
    h->rhs_f32 = b32;
    h->zf_out = zf;
    rc = precond(h, h->rhs, h->w, nu, omega);
    h->rhs_scale = 1.0;
    h->rhs_f32 = nullptr;
    h->zf_out = nullptr;
    hipError_t e = hipStreamSynchronize(h->st);
    if (e == hipSuccess) e = hipGetLastError();
    std::vector<float2> hz;
    if (!rc && e == hipSuccess && zf) {
      hz.resize(n);
      e = hipMemcpy(hz.data(), zf, sizeof(float2) * n, hipMemcpyDeviceToHost);
    }
    if (b32) (void)hipFree(b32);
    if (rc) return rc;
    if (e != hipSuccess) {
      h->err = std::string("pgx_vcycle_apply: ") + hipGetErrorString(e);
      return PGX_EHIP;
    }
    if (zf) {
      for (size_t i = 0; i < n; ++i) {
        z[i] = (double)hz[i].x;
        z[n + i] = (double)hz[i].y;
      }
      return PGX_OK;
    }
    return copy_out(h, z, h->w);
  }
  {
    // a level below the finest only ever sees restricted residuals, whose u entries are 0 on Dirichlet rows (k_restrict and its fused
    // forms mask them), and the fused tail relies on it (k_mg_tail2 does not mask Dirichlet columns): anything else is not a state the
    // solver can be in
    std::vector<uint8_t> hm(n);
    HIPCHK(hipMemcpy(hm.data(), L.mask, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      if (hm[i] && b[i] != 0.0) {
        h->err = "pgx_vcycle_apply: on a level below the finest the u part of b must be 0 on Dirichlet rows (what every restriction delivers)";
        return PGX_EINVAL;
      }
  }
  if (f32) {  // a single-precision level below the finest: float2 right-hand side in L.bf, the correction in the buffer vcycle_f returns
    std::vector<float2> hb(n);
    for (size_t i = 0; i < n; ++i) hb[i] = make_float2((float)b[i], (float)b[n + i]);
    HIPCHK(hipMemcpyAsync(L.bf, hb.data(), sizeof(float2) * n, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    const float2* const res = vcycle_f(h, level, nullptr, nullptr, nullptr, nullptr, nu, omega);
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(hb.data(), res, sizeof(float2) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      z[i] = (double)hb[i].x;
      z[n + i] = (double)hb[i].y;
    }
    return PGX_OK;
  }
  HIPCHK(hipMemcpyAsync(L.bu, b, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(L.bp, b + n, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  vcycle(h, level, L.bu, L.bp, L.xu, L.xp, nu, omega);
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(z, L.xu, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(z + n, L.xp, sizeof(double) * n, hipMemcpyDeviceToHost));
  return PGX_OK;
}

// Test hooks of that hierarchy (include/pgx.h): copies of what a level stores, and one cycle through the functions the solver calls.
static int umg_hook_ready(pgx_handle* h, const char* who) {
  if (!h->jac_valid || !umg_on(h) || h->lu_active) {
    h->err = std::string(who) + " needs a handle with an attached or built hierarchy (pgx_set_hierarchy, pgx_build_hierarchy; PGX_UMG on), a filled Jacobian and the sparse LU not active";
    return PGX_ESTATE;
  }
  return PGX_OK;
}

extern "C" int pgx_umg_level_export(pgx_handle* h, int level, int32_t* n, int32_t* nnz, int32_t* rowptr, int32_t* col, double* K, double* M,
                                    double* D, uint8_t* mask) {
  NEED(h);
  {
    const int rc = umg_hook_ready(h, "pgx_umg_level_export");
    if (rc) return rc;
  }
  if (level < 0 || level >= (int)h->umg.size()) {
    h->err = "pgx_umg_level_export: no such level";
    return PGX_EINVAL;
  }
  const UmgLevel& L = h->umg[level];
  if (n) *n = L.n;
  if (nnz) *nnz = L.nnz;
  HIPCHK(hipStreamSynchronize(h->st));
  if (rowptr) memcpy(rowptr, L.h_rowptr.data(), sizeof(int32_t) * (L.n + 1));
  if (col) memcpy(col, L.h_col.data(), sizeof(int32_t) * L.nnz);
  if (K) HIPCHK(hipMemcpy(K, L.K, sizeof(double) * L.nnz, hipMemcpyDeviceToHost));
  if (M) HIPCHK(hipMemcpy(M, L.M, sizeof(double) * L.nnz, hipMemcpyDeviceToHost));
  if (D) HIPCHK(hipMemcpy(D, L.D, sizeof(double) * L.nnz, hipMemcpyDeviceToHost));
  if (mask) memcpy(mask, L.h_mask.data(), L.n);
  return PGX_OK;
}

extern "C" int pgx_umg_cycle_apply(pgx_handle* h, int level, int nu, double omega, const double* b, double* z) {
  NEED(h);
  {
    const int rc = umg_hook_ready(h, "pgx_umg_cycle_apply");
    if (rc) return rc;
  }
  if (!b || !z || nu < 1 || level < 0 || level >= (int)h->umg.size()) {
    h->err = "pgx_umg_cycle_apply: bad argument (an existing level, nu >= 1, b and z)";
    return PGX_EINVAL;
  }
  if (level == 0 && h->degree == 2) {  // fgmres enters the two-level cycle there: level 0 as pcycle_p2_patch enters it
    const size_t n = (size_t)h->n;
    HIPCHK(hipMemcpyAsync(h->c1_bu, b, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipMemcpyAsync(h->c1_bp, b + n, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    vcycle_umg(h, 0, h->c1_bu, h->c1_bp, h->c1_xu, h->c1_xp, nu, omega);
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(z, h->c1_xu, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(z + n, h->c1_xp, sizeof(double) * n, hipMemcpyDeviceToHost));
    return PGX_OK;
  }
  if (level == 0) {  // as fgmres enters the preconditioner: right-hand side in h->rhs, result in h->w
    int rc = copy_in(h, h->rhs, b);
    if (rc) return rc;
    if ((rc = precond(h, h->rhs, h->w, nu, omega))) return rc;
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipGetLastError());
    return copy_out(h, z, h->w);
  }
  const UmgLevel& L = h->umg[level];
  const size_t n = (size_t)L.n;
  for (size_t i = 0; i < n; ++i)
    if (L.h_mask[i] && b[i] != 0.0) {
      h->err = "pgx_umg_cycle_apply: on a level below the finest the u part of b must be 0 on Dirichlet rows (what every restriction delivers)";
      return PGX_EINVAL;
    }
  HIPCHK(hipMemcpyAsync(L.bu, b, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(L.bp, b + n, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  vcycle_umg(h, level, L.bu, L.bp, L.xu, L.xp, nu, omega);
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(z, L.xu, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(z + n, L.xp, sizeof(double) * n, hipMemcpyDeviceToHost));
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// Test hooks of the P2 two-level cycle (include/pgx.h): what the patch smoother stores, and the stages of pcycle_p2_patch one at a
// time through the functions the cycle itself calls (p2_cycle_resid, p2_cycle_patch, pgxk_p2_restrict, pgxk_p2_prolong_add, precond).
// ------------------------------------------------------------------------------------------------
static int p2_hook_ready(pgx_handle* h, const char* who) {
  if (h->degree != 2 || !h->patch_nn || !h->p2_patch || !h->jac_valid || h->dist.on || h->lu_comm || h->lu_active) {
    h->err = std::string(who) + " needs a single-GPU P2 handle with the vertex-star patch smoother (vertex degree <= 15, PGX_P2_PATCH on), "
                                "a filled Jacobian and the sparse LU not active";
    return PGX_ESTATE;
  }
  return PGX_OK;
}

extern "C" int pgx_p2_cycle_info(pgx_handle* h, int32_t out[8], double* patch_omega) {
  NEED(h);
  if (!out) return PGX_EINVAL;
  int rc = p2_hook_ready(h, "pgx_p2_cycle_info");
  if (rc) return rc;
  if ((rc = ensure_patches(h))) return rc;  // allocates the float copy of D the CSR residual may read
  const int kind = p2_cycle_resid_kind(h);
  out[0] = h->patch_nn;
  out[1] = !h->patch_f32 ? 0 : (!h->patch_sym ? 1 : (h->patch_f32 == 2 ? 3 : 2));
  out[2] = h->patch_nu;
  out[3] = kind == 2 ? (h->p2st.Dstf != nullptr) : (kind == 1 ? (h->s_Df != nullptr) : 0);
  out[4] = kind;
  out[5] = h->p2_fallbacks;
  out[6] = (kind == 1 && h->s_code && h->s_tab) ? 1 : 0;
  out[7] = ((h->structured && h->lev.size() > 1) || umg_on(h)) ? 1 : 0;
  if (patch_omega) *patch_omega = h->patch_omega;
  HIPCHK(hipStreamSynchronize(h->st));
  return PGX_OK;
}

extern "C" int pgx_p2_patch_export(pgx_handle* h, int32_t* pdof, double* Ainv) {
  NEED(h);
  int rc = p2_hook_ready(h, "pgx_p2_patch_export");
  if (rc) return rc;
  if ((rc = ensure_patches(h))) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  const int nv = h->n, NN = h->patch_nn;
  if (pdof) HIPCHK(hipMemcpy(pdof, h->pdof, sizeof(int32_t) * (size_t)nv * NN, hipMemcpyDeviceToHost));
  if (Ainv) {
    std::vector<uint8_t> raw(pgxk_patch_inverse_bytes(nv, NN, h->patch_f32, h->patch_sym));
    HIPCHK(hipMemcpy(raw.data(), h->pinv, raw.size(), hipMemcpyDeviceToHost));
    pgxk_patch_decode(nv, NN, h->patch_f32, h->patch_sym, raw.data(), Ainv);
  }
  return PGX_OK;
}

extern "C" int pgx_p2_wide_export(pgx_handle* h, int32_t* nw, int32_t* verts, int32_t* wdof, double* Ainv) {
  NEED(h);
  int rc = p2_hook_ready(h, "pgx_p2_wide_export");
  if (rc) return rc;
  if ((rc = ensure_patches(h))) return rc;
  HIPCHK(hipStreamSynchronize(h->st));
  HIPCHK(hipGetLastError());
  const PgxWidePatches& W = h->wide;
  if (nw) *nw = W.nw;
  if (!W.nw) return PGX_OK;
  if (verts) memcpy(verts, h->wide_v_host.data(), sizeof(int32_t) * W.nw);
  if (wdof) memcpy(wdof, h->wide_dof_host.data(), sizeof(int32_t) * (size_t)W.nw * PGX_PATCH_WIDE_NN);
  if (Ainv) {
    std::vector<uint8_t> raw(pgxk_patch_wide_inverse_bytes(W.nw, W.f32));
    HIPCHK(hipMemcpy(raw.data(), W.inv, raw.size(), hipMemcpyDeviceToHost));
    pgxk_patch_wide_decode(W.nw, W.f32, raw.data(), Ainv);
  }
  return PGX_OK;
}

extern "C" int pgx_p2_cycle_apply(pgx_handle* h, int stage, int nu, double omega, const double* b, const double* x0, double* z) {
  NEED(h);
  int rc = p2_hook_ready(h, "pgx_p2_cycle_apply");
  if (rc) return rc;
  if (!b || !z || stage < 0 || stage > 4 || (stage == 2 && !x0) || (stage == 0 && (nu < 1 || x0))) {
    h->err = "pgx_p2_cycle_apply: bad argument (stages 0 .. 4; stage 2 needs x0, stage 0 takes none and nu >= 1)";
    return PGX_EINVAL;
  }
  if (stage == 0 && !(h->structured && h->lev.size() > 1) && !umg_on(h)) {
    h->err = "pgx_p2_cycle_apply: the whole cycle needs the P1 grid hierarchy of a structured mesh or an attached one (pgx_set_hierarchy)";
    return PGX_ESTATE;
  }
  if ((rc = ensure_patches(h))) return rc;
  const size_t nd = (size_t)h->nd, nv = (size_t)h->n;
  double *xu = h->w, *xp = h->w + nd;
  auto finish = [&]() -> int {
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipGetLastError());
    return PGX_OK;
  };
  if (stage == 0) {  // as fgmres enters the preconditioner: right-hand side in the Krylov scratch, result in the operator scratch
    if ((rc = copy_in(h, h->rhs, b))) return rc;
    if ((rc = precond(h, h->rhs, h->w, nu, omega))) return rc;
    if ((rc = finish())) return rc;
    return copy_out(h, z, h->w);
  }
  if (stage == 3) {  // z[2 nv] = T^T b, u rows of Dirichlet vertices 0
    HIPCHK(hipMemcpyAsync(h->p2_ru, b, sizeof(double) * nd, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipMemcpyAsync(h->p2_rp, b + nd, sizeof(double) * nd, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    pgxk_p2_restrict(h->st, (int)nv, (int)nd, h->v2e_ptr, h->v2e, h->mask, h->p2_ru, h->p2_rp, h->c1_bu, h->c1_bp);
    if ((rc = finish())) return rc;
    HIPCHK(hipMemcpy(z, h->c1_bu, sizeof(double) * nv, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(z + nv, h->c1_bp, sizeof(double) * nv, hipMemcpyDeviceToHost));
    return PGX_OK;
  }
  // the iterate the stage starts from
  if (x0) {
    if ((rc = copy_in(h, h->w, x0))) return rc;
  } else {
    HIPCHK(hipMemsetAsync(h->w, 0, sizeof(double) * 2 * nd, h->st));
  }
  if (stage == 4) {  // z = x0 + T b, b of length 2 nv
    HIPCHK(hipMemcpyAsync(h->c1_xu, b, sizeof(double) * nv, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipMemcpyAsync(h->c1_xp, b + nv, sizeof(double) * nv, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    pgxk_p2_prolong_add(h->st, (int)nv, (int)nd, h->edge_ends, h->c1_xu, h->c1_xp, xu, xp);
    if ((rc = finish())) return rc;
    return copy_out(h, z, h->w);
  }
  if ((rc = copy_in(h, h->rhs, b))) return rc;
  const double *bu = h->rhs, *bp = h->rhs + nd;
  if (stage == 2 || x0) p2_cycle_resid(h, p2_cycle_resid_kind(h), xu, xp, bu, bp);
  if (stage == 2) {  // z = b - J x0 by the cycle's residual kernel
    if ((rc = finish())) return rc;
    HIPCHK(hipMemcpy(z, h->p2_ru, sizeof(double) * nd, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(z + nd, h->p2_rp, sizeof(double) * nd, hipMemcpyDeviceToHost));
    return PGX_OK;
  }
  // stage 1: one sweep; from x = 0 the residual is b and no residual is launched (the cycle's first sweep)
  if (x0)
    p2_cycle_patch(h, h->p2_ru, h->p2_rp, xu, xp);
  else
    p2_cycle_patch(h, bu, bp, xu, xp);
  if ((rc = finish())) return rc;
  return copy_out(h, z, h->w);
}

static int spmv_bench_impl(pgx_handle* h, int reps, double* avg_ms, double* bytes, bool cold) {
  NEED(h);
  if (reps < 1 || !avg_ms) return PGX_EINVAL;
  if (!h->jac_valid) {
    h->err = "pgx_spmv_bench before pgx_jacobian_fill";
    return PGX_ESTATE;
  }
  const size_t n2 = 2 * (size_t)h->nd;
  pgxk_set(h->st, n2, 1.0, h->V);
  for (int k = 0; k < 3; ++k) spmv_dev(h, h->V, h->w);
  // Launches in the cache state of a solve, not back to back: the matrix-free kernel's whole footprint (273 MB at 2048^2) would
  // otherwise sit in the 256 MB Infinity Cache (42 us per launch in a tight loop, 49-50 us inside the solves per rocprofv3).
  // Multigrid handles replay the solver's own sequence - one V-cycle producing z, then J z, exactly as in an FGMRES iteration -
  // and subtract the time of the V-cycles alone; other handles sweep 512 MB of idle storage (a dot product) between two
  // applies.  Each batch sits between ONE pair of events: a pair around a single 50 us kernel would add the ~50 us of its two
  // barrier packets.
  // cold: every apply follows a 512 MB sweep of unrelated storage, so neither x nor the stencils sit in the 256 MB Infinity Cache
  const bool mg = !cold && h->structured && h->degree == 1 && !h->dist.on && !h->lu_active && h->lev.size() > 1;
  pgx_snes_opts od;
  pgx_default_opts(&od);
  const bool zf = mg && z_f32_active(h, od.mg_nu);
  const size_t flush = std::min<size_t>((size_t)h->restart * n2, ((size_t)512 << 20) / sizeof(double));
  // nine rounds of (batch with applies, batch without), median of the differences: clock and power drift between two ~50 ms
  // batches is of the order of the quantity measured
  std::vector<double> diff;
  for (int round = 0; round < 9; ++round) {
    double t[2] = {0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {
      HIPCHK(hipEventRecord(h->e0, h->st));
      for (int k = 0; k < reps; ++k) {
        if (mg) {
          h->zf_out = zf ? reinterpret_cast<float2*>(h->Z) : nullptr;  // as in fgmres: the cycle leaves z as ONE float2 field ...
          const int rc = precond(h, h->V, h->Z, od.mg_nu, od.mg_omega);
          h->zf_out = nullptr;
          if (rc) return rc;
        } else {
          pgxk_multidot(h->st, flush, 1, h->Z, 0, h->Z, h->partials, h->d_small);
        }
        if (pass == 0) {
          if (zf)  // ... and the apply reads it (k_st_spmv_r<true>)
            pgxk_st_spmv(h->st, h->lev[0], h->alpha, nullptr, nullptr, h->xcd_remap ? 1 : 0, h->w, h->w + h->nd, reinterpret_cast<const float2*>(h->Z));
          else
            spmv_dev(h, mg ? h->Z : h->V, h->w);
        }
      }
      HIPCHK(hipEventRecord(h->e1, h->st));
      HIPCHK(hipEventSynchronize(h->e1));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, h->e0, h->e1));
      t[pass] = ms;
    }
    diff.push_back((t[0] - t[1]) / reps);
  }
  std::sort(diff.begin(), diff.end());
  *avg_ms = diff[diff.size() / 2];
  if (bytes) {
    if (h->spmv_stencil && h->structured && h->degree == 1)
      // matrix-free: x read once (16 B per vertex; 8 B as the float2 field of an FGMRES z_j), y written (16 B), half-stored D stencil
      // (4 x 8 B), Dirichlet mask (1 B); K and M are seven constants each
      *bytes = ((zf ? 8.0 : 16.0) + 16.0 + 4.0 * sizeof(dsten_t) + 1.0) * h->nd;
    else if (h->degree == 2 && h->p2st.state == 2 && h->p2st.select && (!h->dist.on || h->p2st.dist_enable) && h->spmv_stream && h->spmv_bal) {
      // structured P2 apply: 46 D values per interior group (SoA copy), nothing else of the matrix; the frame rows in CSR form
      // (column + K + M + D = 28 B per entry, the row list); x read once; y written
      const double nfast = (double)h->p2st.ni * h->p2st.nj;
      *bytes = 368.0 * nfast + 28.0 * ((double)h->s_nnz - 46.0 * nfast) + 4.0 * h->p2st.nframe + 8.0 * n2 + 8.0 * n2;
    } else if (h->s_code && h->spmv_bal && h->s_blk && h->spmv_stream)
      // (K, M) dictionary: column (4 B) + code (1 B) + D (8 B) per scalar nnz; rowptr; x read once; y written
      *bytes = 13.0 * h->s_nnz + 4.0 * (h->nd + 1) + 8.0 * n2 + 8.0 * n2;
    else  // one pattern (4 B) + three value streams (24 B) per scalar nnz; rowptr; x read once; y written
      *bytes = 28.0 * h->s_nnz + 4.0 * (h->nd + 1) + 8.0 * n2 + 8.0 * n2;
  }
  return PGX_OK;
}
extern "C" int pgx_spmv_bench(pgx_handle* h, int reps, double* avg_ms, double* bytes) {
  return spmv_bench_impl(h, reps, avg_ms, bytes, false);
}
extern "C" int pgx_spmv_bench_cold(pgx_handle* h, int reps, double* avg_ms, double* bytes) {
  return spmv_bench_impl(h, reps, avg_ms, bytes, true);
}

extern "C" int pgx_comm_counts(pgx_handle* h, int64_t out[4], int reset) {
  NEED(h);
  if (!out) return PGX_EINVAL;
  out[0] = h->dist.n_halo;
  out[1] = h->dist.n_allreduce;
  out[2] = h->dist.n_vcycle;
  out[3] = h->dist.n_krylov;
  if (reset) h->dist.n_halo = h->dist.n_allreduce = h->dist.n_vcycle = h->dist.n_krylov = 0;
  return PGX_OK;
}

extern "C" int pgx_p2_stencil_info(pgx_handle* h, int32_t out[5]) {
  NEED(h);
  if (!out) return PGX_EINVAL;
  const pgx_handle::P2St& S = h->p2st;
  out[0] = (h->degree == 2 && (!h->dist.on || S.dist_enable)) ? S.state : 0;
  out[1] = S.i0, out[2] = S.ni, out[3] = S.j0, out[4] = S.nj;
  return PGX_OK;
}
extern "C" int pgx_spmv_select(pgx_handle* h, int kind, int* active) {
  NEED(h);
  if (h->degree == 2) {  // P2: 3 (or 1) = the structured apply of pgx_p2st.hip where the mesh allows it, 0 = the block-CSR kernel
    if (kind == 0) h->p2st.select = 0;
    else if (kind == 1 || kind == 3) h->p2st.select = 1;
    else if (kind != -1) return PGX_EINVAL;
    if (active) *active = (h->p2st.state && h->p2st.select && (!h->dist.on || h->p2st.dist_enable) && h->spmv_stream && h->spmv_bal) ? 3 : 0;
    return PGX_OK;
  }
  if (kind == 0 || kind == 1 || kind == 2) h->spmv_stencil = kind;
  else if (kind != -1) return PGX_EINVAL;
  if (active) *active = (h->spmv_stencil && h->structured && h->degree == 1) ? h->spmv_stencil : 0;
  return PGX_OK;
}

// Test hook of PGX_RESID_REUSE: evaluates the entry residual of the next pgx_newton_solve both ways, at the current x, x_k and alpha,
// and compares bytes on the host.  Needs a valid stamp (PGX_EINVAL otherwise) and leaves it dropped.
extern "C" int pgx_resid_reuse_selfcheck(pgx_handle* h, int64_t out[6]) {
  if (!h) return PGX_EINVAL;
  const pgx_handle::ResidFresh fr = h->fresh;
  NEED(h);
  if (!out) return PGX_EINVAL;
  if (!(resid_reuse_on(h) && fr.valid && fr.dh_interior == h->dh_interior && fr.d0_direct == h->d0_direct && fr.dv_lean == h->dv_lean)) {
    h->err = "pgx_resid_reuse_selfcheck: no valid stamp (call it after a converged pgx_newton_solve of a handle PGX_RESID_REUSE applies to)";
    return PGX_EINVAL;
  }
  const GridLevel& L = h->lev[0];
  const size_t n = (size_t)h->n;
  // the buffers the stamp speaks of: F_psi, Dh, Dd4, Dq, the CSR rows
  struct Buf {
    const void* dev;
    size_t bytes;
  };
  const Buf bufs[5] = {{h->F + n, n * sizeof(double)},
                       {L.Dh, 4 * n * sizeof(dsten_t)},
                       {L.Dd4, L.Dd4 ? n * sizeof(double4) : 0},
                       {L.Dq, (L.f32 && L.Dq) ? n * (L.dbf16 ? sizeof(uint2) : sizeof(float4)) : 0},
                       {h->Dv, h->Dv ? (size_t)h->nnz * sizeof(double) : 0}};
  using Snap = std::vector<std::vector<unsigned char>>;
  auto snapshot = [&](Snap& s) -> int {
    s.resize(5);
    for (int k = 0; k < 5; ++k) {
      s[k].resize(bufs[k].bytes);
      if (bufs[k].bytes) HIPCHK(hipMemcpyAsync(s[k].data(), bufs[k].dev, bufs[k].bytes, hipMemcpyDeviceToHost, h->st));
    }
    HIPCHK(hipStreamSynchronize(h->st));
    return PGX_OK;
  };
  auto differing = [](const std::vector<unsigned char>& a, const std::vector<unsigned char>& b, size_t word) {
    int64_t c = 0;
    for (size_t i = 0; i < a.size(); i += word) c += memcmp(a.data() + i, b.data() + i, word) != 0;
    return c;
  };
  Snap held, after_reduced, after_full;
  std::vector<double> fu_reduced(n), fu_full(n);
  int rc = snapshot(held);
  if (rc) return rc;
  residual_dev(h, h->x, h->F, fr.with_d, true);
  HIPCHK(hipMemcpyAsync(fu_reduced.data(), h->F, n * sizeof(double), hipMemcpyDeviceToHost, h->st));
  if ((rc = snapshot(after_reduced))) return rc;
  residual_dev(h, h->x, h->F, fr.with_d, false);
  HIPCHK(hipMemcpyAsync(fu_full.data(), h->F, n * sizeof(double), hipMemcpyDeviceToHost, h->st));
  if ((rc = snapshot(after_full))) return rc;
  HIPCHK(hipGetLastError());
  out[0] = 0;  // entries of F_u that differ between the two evaluations
  for (size_t i = 0; i < n; ++i) out[0] += memcmp(&fu_reduced[i], &fu_full[i], sizeof(double)) != 0;
  out[1] = differing(held[0], after_reduced[0], sizeof(double));  // entries of F_psi the reduced evaluation changed
  out[2] = 0;  // 8-byte words of the D copies it changed
  for (int k = 1; k < 5; ++k) out[2] += differing(held[k], after_reduced[k], 8);
  out[3] = differing(held[0], after_full[0], sizeof(double));  // entries of F_psi in which the held values are not the full evaluation's
  out[4] = 0;  // the same for the D copies
  for (int k = 1; k < 5; ++k) out[4] += differing(held[k], after_full[k], 8);
  out[5] = (int64_t)n;
  return PGX_OK;
}
