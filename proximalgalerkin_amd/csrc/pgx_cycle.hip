// The preconditioner of libpgx.so: the multigrid cycles on stencil levels (fp64 and single precision, single and sharded) and on the
// block-CSR levels of a general mesh, the collectives of the sharded path, the P2 two-level cycles with their patch data, the sparse LU,
// and precond(), through which the Krylov driver (pgx_krylov.hip) and the test hooks (pgx_hooks.hip) enter all of them.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "pgx_handle.h"

// ------------------------------------------------------------------------------------------------
// sharded path: the ghost-row exchange and the sum over the ranks
// ------------------------------------------------------------------------------------------------
// refresh every ghost row of a (u, psi) pair on distributed level l from the owning neighbours
static int halo_level(pgx_handle* h, int l, double* fu, double* fp) {
  const DistLevel& d = h->dist.L[l];
  const size_t sx = (size_t)h->lev[l].nx + 1;
  double* f[2] = {fu, fp};
  const int rc = h->dist.comm->halo(h->st, f, 2, d.glo * sx, (d.g + 1) * sx, 0, d.g * sx, (d.glo + d.H - d.g) * sx,
                                    d.g * sx, (d.glo + d.H) * sx, (d.g + 1) * sx);
  ++h->dist.n_halo;
  if (rc) h->err = h->dist.comm->err;
  return rc;
}
// the same for ONE interleaved (u, psi) float2 field of the single-precision cycle (8 bytes per vertex: one "double" field)
static int halo_level_f(pgx_handle* h, int l, float2* f2) {
  const DistLevel& d = h->dist.L[l];
  const size_t sx = (size_t)h->lev[l].nx + 1;
  double* f[1] = {reinterpret_cast<double*>(f2)};
  const int rc = h->dist.comm->halo(h->st, f, 1, d.glo * sx, (d.g + 1) * sx, 0, d.g * sx, (d.glo + d.H - d.g) * sx, d.g * sx,
                                    (d.glo + d.H) * sx, (d.g + 1) * sx);
  ++h->dist.n_halo;
  if (rc) h->err = h->dist.comm->err;
  return rc;
}
// ghost entries of a SOLUTION-SPACE pair (fu, fp) - each [vertex dofs | edge dofs] for P2 - from their owners
int halo_solution(pgx_handle* h, double* fu, double* fp) {
  int rc = halo_level(h, 0, fu, fp);
  if (rc || h->degree != 2) return rc;
  // edge part: g full row blocks below and above (the last local row's horizontal edges stay behind: they lie on the outermost,
  // never-valid ghost line)
  const DistLevel& d = h->dist.L[0];
  const size_t eb = h->dist.eb, nv = (size_t)h->n;
  double* f[2] = {fu + nv, fp + nv};
  rc = h->dist.comm->halo(h->st, f, 2, d.glo * eb, d.g * eb, 0, d.g * eb, (size_t)(d.glo + d.H - d.g) * eb, d.g * eb,
                          (size_t)(d.glo + d.H) * eb, d.g * eb);
  ++h->dist.n_halo;
  if (rc) h->err = h->dist.comm->err;
  return rc;
}
int allreduce_dev(pgx_handle* h, double* dev, size_t n) {
  const int rc = h->dist.comm->allreduce(h->st, dev, n);
  ++h->dist.n_allreduce;
  if (rc) h->err = h->dist.comm->err;
  return rc;
}

// ------------------------------------------------------------------------------------------------
// the cycles
// ------------------------------------------------------------------------------------------------
void level_apply(pgx_handle* h, int l, int mode, const double* xu, const double* xp, const double* bu, const double* bp, double omega,
                 int first, double* yu, double* yp) {
  if (l == 0 && !h->structured)  // general mesh: the block-CSR kernel is also the (single-level) smoother
    pgxk_bspmv(h->st, mode, h->n, h->rowptr, h->colm, h->Kv, h->Mv, h->Dv, h->alpha, xu, xp, bu, bp, omega,
               first | h->xcd_remap, yu, yp);
  else
    pgxk_st_apply(h->st, mode, h->lev[l], h->alpha, xu, xp, bu, bp, omega, first | h->xcd_remap, yu, yp);
}

// Single-precision legs of the V-cycle on level l (GridLevel::f32; kernels: pgx_mg32.hip).  With (bu, bp) != nullptr the level
// reads its right-hand side from that fp64 pair (its first launch leaves the float2 copy in L.bf) and writes the result to the
// fp64 pair (outu, outp): the finest level, or a level entered from an fp64 one.  Otherwise it finds its right-hand side in L.bf
// (written by the single-precision level above) and returns the buffer that holds its correction.  A level without f32 below gets
// its right-hand side, and hands back its correction, in fp64 (vcycle()).
const float2* vcycle_f(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega) {
  GridLevel& L = h->lev[l];
  GridLevel& C = h->lev[l + 1];
  // all six sweeps of a leg in ONE launch: the small levels are bound by the latency of a launch, not by its work (their
  // pre-smoothing launch restricts the residual as well: two launches per level and cycle instead of five); the big ones save the
  // pass over D, b and the intermediate iterate between two three-sweep launches (three launches instead of five)
  const int K = (nu == 6 && L.n <= h->f32_k6_max) ? 6 : ((nu % 3 == 0 && h->fused_k3) ? 3 : 2);
  const int nl = nu / K;
  const int remap = h->xcd_remap ? 1 : 0;
  float2 *cu = L.xf, *ou = L.xf2;
  // levels up to f32_rr_max vertices: the last pre-smoothing launch also restricts the residual of its result (one launch and one
  // pass over D, b, x less per level and cycle; the finest level keeps the separate launch: its halo overhead costs more there)
  const bool fuse = L.n <= h->f32_rr_max;
  float2* const cbf = C.f32 ? C.bf : nullptr;
  double* const cb64u = C.f32 ? nullptr : C.bu;
  double* const cb64p = C.f32 ? nullptr : C.bp;
  {
    const bool rr = fuse && nl == 1;
    const double bscale = (l == 0 && bu) ? h->rhs_scale : 1.0;
    const float* const b32 = (l == 0 && bu) ? h->rhs_f32 : nullptr;  // the Krylov vector as two float fields (fgmres: float basis)
    pgxk_f_smooth(h->st, K, 1, L, h->alpha, nullptr, bu, bp, rr ? &C : nullptr, nullptr, nullptr, nullptr, omega, remap, cu, nullptr,
                  nullptr, rr ? cbf : nullptr, rr ? cb64u : nullptr, rr ? cb64p : nullptr, bscale, b32, b32 ? b32 + L.n : nullptr);
  }
  for (int s = 1; s < nl; ++s) {
    const bool rr = fuse && s + 1 == nl;
    pgxk_f_smooth(h->st, K, 0, L, h->alpha, cu, nullptr, nullptr, rr ? &C : nullptr, nullptr, nullptr, nullptr, omega, remap, ou, nullptr,
                  nullptr, rr ? cbf : nullptr, rr ? cb64u : nullptr, rr ? cb64p : nullptr);
    std::swap(cu, ou);
  }
  if (!fuse) pgxk_f_resid_restrict(h->st, L, h->alpha, cu, C, remap, cbf, cb64u, cb64p);
  const float2* cf = nullptr;
  const double *cdu = nullptr, *cdp = nullptr;
  if (C.f32) {
    cf = vcycle_f(h, l + 1, nullptr, nullptr, nullptr, nullptr, nu, omega);
  } else {
    vcycle(h, l + 1, C.bu, C.bp, C.xu, C.xp, nu, omega);
    cdu = C.xu;
    cdp = C.xp;
  }
  for (int s = 0; s < nl; ++s) {
    const bool lastl = s + 1 == nl;
    float2* const zf = (lastl && l == 0) ? h->zf_out : nullptr;  // the cycle's result stays float2, in the caller's buffer
    const bool out64 = lastl && outu && !zf;
    pgxk_f_smooth(h->st, K, 0, L, h->alpha, cu, nullptr, nullptr, s == 0 ? &C : nullptr, s == 0 ? cf : nullptr, s == 0 ? cdu : nullptr,
                  s == 0 ? cdp : nullptr, omega, remap, zf ? zf : ou, out64 ? outu : nullptr, out64 ? outp : nullptr);
    if (zf) return zf;
    std::swap(cu, ou);
  }
  return cu;
}
bool f32_cycle_ok(const pgx_handle* h, int l, int nu) {
  return h->lev[l].f32 && h->fused_legs && l + 1 < (int)h->lev.size() && nu >= 2 && (nu % 2 == 0 || (nu % 3 == 0 && h->fused_k3));
}

// Refined general mesh (pgx_set_hierarchy; kernels: pgx_umg.hip): the same V(nu, nu) cycle on block-CSR levels.  Per level: nu sweeps
// of k_bspmv<2> (the first from zero) | k_bspmv<1> writes b - J x, k_umg_resid_restrict gathers P^T of it | the level below |
// k_umg_prolong_add | nu sweeps.  The coarsest level runs umg_coarse_sweeps sweeps from zero: in one launch of one workgroup where its
// operator and vectors fit the LDS (pgxk_umg_coarse_lds <= PGX_UMG_COARSE_LDS_MAX: about 600 vertices) and the handle's device took
// that limit (umg_coarse_fits, settled by pgx_set_hierarchy), as k_bspmv<2> launches otherwise.
void vcycle_umg(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega) {
  const UmgLevel& L = h->umg[l];
  const bool last = l + 1 == (int)h->umg.size();
  if (last && h->umg_coarse_lds && h->umg_coarse_fits) {
    pgxk_umg_coarse(h->st, L.n, L.nnz, L.rowptr, L.colm, L.K, L.M, L.D, h->alpha, omega, h->umg_coarse_sweeps, bu, bp, outu, outp);
    return;
  }
  const int total = last ? h->umg_coarse_sweeps : 2 * nu;
  bool toA = (total % 2) == 1;  // alternate targets so that the final sweep lands in (outu, outp)
  const double *cu = nullptr, *cp = nullptr;
  auto sweep = [&](int first) {
    double* tu = toA ? outu : L.xu2;
    double* tp = toA ? outp : L.xp2;
    pgxk_bspmv(h->st, 2, L.n, L.rowptr, L.colm, L.K, L.M, L.D, h->alpha, cu, cp, bu, bp, omega, first | h->xcd_remap, tu, tp);
    cu = tu;
    cp = tp;
    toA = !toA;
  };
  if (last) {
    for (int s = 0; s < total; ++s) sweep(s == 0);
    return;
  }
  for (int s = 0; s < nu; ++s) sweep(s == 0);
  pgxk_bspmv(h->st, 1, L.n, L.rowptr, L.colm, L.K, L.M, L.D, h->alpha, cu, cp, bu, bp, 0.0, h->xcd_remap, L.ru, L.rp);
  const UmgLevel& C = h->umg[l + 1];
  if (C.P_val)  // a built hierarchy: the transfers with general weights (pgx_amg.hip)
    pgxk_amg_resid_restrict(h->st, C, L.ru, L.rp);
  else
    pgxk_umg_resid_restrict(h->st, C.n, C.ch_ptr, C.ch_idx, C.mask, L.ru, L.rp, C.bu, C.bp);
  vcycle_umg(h, l + 1, C.bu, C.bp, C.xu, C.xp, nu, omega);
  if (C.P_val)
    pgxk_amg_prolong_add(h->st, L.n, C, (double*)cu, (double*)cp);
  else
    pgxk_umg_prolong_add(h->st, L.n, C.parents, C.xu, C.xp, (double*)cu, (double*)cp);
  for (int s = 0; s < nu; ++s) sweep(0);
}

// one V(nu,nu) cycle for J_l x = b, zero initial guess, result in (outu,outp)
void vcycle(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega) {
  if (umg_on(h)) {
    vcycle_umg(h, l, bu, bp, outu, outp, nu, omega);
    return;
  }
  GridLevel& L = h->lev[l];
  if (f32_cycle_ok(h, l, nu)) {
    vcycle_f(h, l, bu, bp, outu, outp, nu, omega);
    return;
  }
  if (l > 0 && l == h->tail_start) {  // all remaining levels in ONE launch (k_mg_tail); result in L.xu/L.xp
    h->tail.nu = (h->nu_coarse > 0) ? std::min(nu, h->nu_coarse) : nu;
    h->tail.omega = omega;
    h->tail.alpha = h->alpha;
    h->tail.coarse_sweeps = h->coarse_sweeps;
    pgxk_mg_tail(h->st, h->tail);
    return;
  }
  const bool last = (l + 1 == (int)h->lev.size());
  double* Au = outu;
  double* Ap = outp;
  double* Bu = (l == 0) ? h->tmp_u : L.xu2;
  double* Bp = (l == 0) ? h->tmp_p : L.xp2;
  double* ru = (l == 0) ? h->res_u : L.ru;
  double* rp = (l == 0) ? h->res_p : L.rp;
  const int Kf = (nu % 3 == 0 && h->fused_k3) ? 3 : (nu % 2 == 0 ? 2 : 0);  // sweeps per fused launch
  if (h->structured && !last && Kf && h->fused_legs && L.n >= h->fused_min) {
    // per level: nu/K multi-sweep launches | P^T(b - Jx) | nu/K multi-sweep launches (the first one also adds the
    // prolongated coarse correction)   (pgx_kernels.hip, "Fused V-cycle legs", k_st_smoothK)
    GridLevel& C = h->lev[l + 1];
    const int remap = h->xcd_remap ? 1 : 0;
    // small levels are bound by the latency of a launch's dependent phases, not by its work: all six sweeps of a leg in ONE launch
    const int Kl = (Kf == 3 && nu % 6 == 0 && L.n <= h->k6_max && pgxk_st_smooth6_ok(L)) ? 6 : Kf;
    const int nl = nu / Kl;
    double *cu = Bu, *cp = Bp, *ou = Au, *op = Ap;  // current / other buffer pair
    pgxk_st_smoothK(h->st, Kl, 0, L, h->alpha, nullptr, nullptr, nullptr, nullptr, nullptr, bu, bp, omega, remap, cu, cp);
    for (int s = 1; s < nl; ++s) {
      pgxk_st_smoothK(h->st, Kl, 1, L, h->alpha, cu, cp, nullptr, nullptr, nullptr, bu, bp, omega, remap, ou, op);
      std::swap(cu, ou);
      std::swap(cp, op);
    }
    pgxk_st_resid_restrict(h->st, L, h->alpha, cu, cp, bu, bp, C, remap, C.bu, C.bp);
    vcycle(h, l + 1, C.bu, C.bp, C.xu, C.xp, nu, omega);
    pgxk_st_smoothK(h->st, Kl, 1, L, h->alpha, cu, cp, &C, C.xu, C.xp, bu, bp, omega, remap, ou, op);
    std::swap(cu, ou);
    std::swap(cp, op);
    for (int s = 1; s < nl; ++s) {
      pgxk_st_smoothK(h->st, Kl, 1, L, h->alpha, cu, cp, nullptr, nullptr, nullptr, bu, bp, omega, remap, ou, op);
      std::swap(cu, ou);
      std::swap(cp, op);
    }
    if (cu != Au) {
      hipMemcpyAsync(Au, cu, sizeof(double) * L.n, hipMemcpyDeviceToDevice, h->st);
      hipMemcpyAsync(Ap, cp, sizeof(double) * L.n, hipMemcpyDeviceToDevice, h->st);
    }
    return;
  }
  if (l > 0 && h->nu_coarse > 0) nu = std::min(nu, h->nu_coarse);  // small levels are launch-latency bound: fewer sweeps
  const int total = last ? (h->lev.size() == 1 ? 2 * nu : h->coarse_sweeps) : 2 * nu;
  bool toA = (total % 2) == 1;  // alternate targets so that the final sweep lands in A
  const double *cu = nullptr, *cp = nullptr;
  auto sweep = [&](int first) {
    double* tu = toA ? Au : Bu;
    double* tp = toA ? Ap : Bp;
    level_apply(h, l, 2, cu, cp, bu, bp, omega, first, tu, tp);
    cu = tu;
    cp = tp;
    toA = !toA;
  };
  if (last) {
    for (int s = 0; s < total; ++s) sweep(s == 0);
    return;
  }
  for (int s = 0; s < nu; ++s) sweep(s == 0);
  level_apply(h, l, 1, cu, cp, bu, bp, 0.0, 0, ru, rp);
  GridLevel& C = h->lev[l + 1];
  pgxk_restrict(h->st, L, ru, rp, C, C.bu, C.bp);
  vcycle(h, l + 1, C.bu, C.bp, C.xu, C.xp, nu, omega);
  pgxk_prolong_add(h->st, C, C.xu, C.xp, L, (double*)cu, (double*)cp);
  for (int s = 0; s < nu; ++s) sweep(0);
}

// ------------------------------------------------------------------------------------------------
// Sharded V-cycle (include/pgx.h "Sharded path").  Same sweeps, residuals and transfers as vcycle()
// - the algebra is identical to the single-handle cycle - on strips with ghost rows.  "Validity depth" d of a vector
// means: correct on global rows [a-d, a+H+d] of the strip [a, a+H).  A halo exchange sets d = g (all local rows);
// K Jacobi sweeps in one launch cost K rows (each sweep reads the neighbours' previous values), the fused
// residual+restriction needs d >= 2, x + P x_c needs d >= K for the sweeps that follow.  Exchanges are issued only
// when the depth runs out: with ghost depth 8/4/2 on the three distributed levels and nu = 6 that is 2 + 5 + 7
// exchanges and one all-reduce (coarse right-hand side) per cycle.
// ------------------------------------------------------------------------------------------------
// The step from the last strip level l onto the first replicated level, shared by both sharded cycles: every rank restricts into its
// view (restrict_into(V) writes the fp64 pair V.bu, V.bp), clears the view's ghost rows, and the all-reduce assembles the global
// right-hand side (exactly one non-zero contribution per entry); then the replicated cycle.  The correction is in the view's (xu, xp).
template <class Restrict>
static int replicated_step(pgx_handle* h, int l, int nu, double omega, Restrict&& restrict_into) {
  const Dist& D = h->dist;
  GridLevel& G = h->lev[l + 1];
  const GridLevel& V = D.view;
  const size_t sxc = (size_t)G.nx + 1;
  if (hipMemsetAsync(G.bu, 0, sizeof(double) * 2 * (size_t)G.n, h->st) != hipSuccess) return PGX_EHIP;
  restrict_into(V);
  const size_t lo = (size_t)D.view_glo * sxc, hi0 = (size_t)(D.view_glo + D.view_H) * sxc, hi = (size_t)V.n - hi0;
  double* const halves[2] = {V.bu, V.bp};
  for (double* b : halves) {
    if (lo) hipMemsetAsync(b, 0, sizeof(double) * lo, h->st);
    if (hi) hipMemsetAsync(b + hi0, 0, sizeof(double) * hi, h->st);
  }
  const int rc = allreduce_dev(h, G.bu, 2 * (size_t)G.n);
  if (rc) return rc;
  vcycle(h, l + 1, G.bu, G.bp, G.xu, G.xp, nu, omega);  // identical work on every rank
  return PGX_OK;
}

static int vcycle_dist_f(pgx_handle* h, int l, double* bu, double* bp, double* outu, double* outp, int need_out, int nu, double omega,
                         const float2** res);
static int vcycle_dist(pgx_handle* h, int l, double* bu, double* bp, double* outu, double* outp, int need_out, int nu,
                       double omega) {
  Dist& D = h->dist;
  GridLevel& L = h->lev[l];
  if (L.f32 && h->fused_legs) return vcycle_dist_f(h, l, bu, bp, outu, outp, need_out, nu, omega, nullptr);
  const int g = D.L[l].g;
  const int K = (nu % 3 == 0 && g >= 3 && h->fused_k3) ? 3 : 2;
  if (nu % K) {
    h->err = "sharded V-cycle: mg_nu must be even (or a multiple of 3 with deep enough ghost rows)";
    return PGX_EINVAL;
  }
  const int remap = h->xcd_remap ? 1 : 0;
  const int nl = nu / K;
  int rc = halo_level(h, l, bu, bp);  // restriction / the Krylov vector are correct on owned rows only
  if (rc) return rc;
  double *cu = (l == 0) ? h->tmp_u : L.xu2, *cp = (l == 0) ? h->tmp_p : L.xp2, *ou = outu, *op = outp;
  int xv;  // validity depth of (cu, cp)
  pgxk_st_smoothK(h->st, K, 0, L, h->alpha, nullptr, nullptr, nullptr, nullptr, nullptr, bu, bp, omega, remap, cu, cp);
  xv = g - K;  // first sweep from zero is pointwise: valid where b and the operator are (depth g-1)
  auto more = [&](const GridLevel* C, const double* ccu, const double* ccp) -> int {
    if (xv < K) {
      const int r = halo_level(h, l, cu, cp);
      if (r) return r;
      xv = g;
    }
    pgxk_st_smoothK(h->st, K, 1, L, h->alpha, cu, cp, C, ccu, ccp, bu, bp, omega, remap, ou, op);
    std::swap(cu, ou);
    std::swap(cp, op);
    xv -= K;
    return PGX_OK;
  };
  for (int s = 1; s < nl; ++s)
    if ((rc = more(nullptr, nullptr, nullptr))) return rc;
  if (xv < 2) {  // P^T (b - J x) on the owned coarse rows reads the residual one row out, i.e. x two rows out
    if ((rc = halo_level(h, l, cu, cp))) return rc;
    xv = g;
  }
  const GridLevel* C;
  if (l + 1 < D.ldist) {
    GridLevel& Cl = h->lev[l + 1];
    pgxk_st_resid_restrict(h->st, L, h->alpha, cu, cp, bu, bp, Cl, remap, Cl.bu, Cl.bp);
    if ((rc = vcycle_dist(h, l + 1, Cl.bu, Cl.bp, Cl.xu, Cl.xp, D.L[l + 1].g, nu, omega))) return rc;
    C = &Cl;
  } else {
    rc = replicated_step(h, l, nu, omega, [&](const GridLevel& V) {
      pgxk_st_resid_restrict(h->st, L, h->alpha, cu, cp, bu, bp, V, remap, V.bu, V.bp);
    });
    if (rc) return rc;
    C = &D.view;
  }
  // x + P x_c is correct to depth min(xv, g): the coarse correction covers every local row
  if ((rc = more(C, C->xu, C->xp))) return rc;
  for (int s = 1; s < nl; ++s)
    if ((rc = more(nullptr, nullptr, nullptr))) return rc;
  if (xv < need_out) {
    if ((rc = halo_level(h, l, cu, cp))) return rc;
    xv = g;
  }
  if (cu != outu) {
    hipMemcpyAsync(outu, cu, sizeof(double) * L.n, hipMemcpyDeviceToDevice, h->st);
    hipMemcpyAsync(outp, cp, sizeof(double) * L.n, hipMemcpyDeviceToDevice, h->st);
  }
  return PGX_OK;
}

// The sharded cycle on a single-precision strip level (GridLevel::f32): vcycle_dist with the kernels of pgx_mg32.hip.  Same depth
// bookkeeping; a halo exchange moves ONE float2 field (8 bytes per vertex) instead of two fp64 ones.  (bu, bp) != nullptr: fp64
// right-hand side in (the Krylov vector), fp64 result out; else L.bf in, *res = the buffer that holds the correction.
static int vcycle_dist_f(pgx_handle* h, int l, double* bu, double* bp, double* outu, double* outp, int need_out, int nu, double omega,
                         const float2** res) {
  Dist& D = h->dist;
  GridLevel& L = h->lev[l];
  const int g = D.L[l].g;
  const int K = (nu % 3 == 0 && g >= 3 && h->fused_k3) ? 3 : 2;
  if (nu % K) {
    h->err = "sharded V-cycle: mg_nu must be even (or a multiple of 3 with deep enough ghost rows)";
    return PGX_EINVAL;
  }
  const int remap = h->xcd_remap ? 1 : 0;
  const int nl = nu / K;
  int rc = bu ? halo_level(h, l, bu, bp) : halo_level_f(h, l, L.bf);  // the right-hand side is correct on owned rows only
  if (rc) return rc;
  float2 *cu = L.xf, *ou = L.xf2;
  pgxk_f_smooth(h->st, K, 1, L, h->alpha, nullptr, bu, bp, nullptr, nullptr, nullptr, nullptr, omega, remap, cu, nullptr, nullptr, nullptr,
                nullptr, nullptr, (l == 0 && bu) ? h->rhs_scale : 1.0);
  int xv = g - K;  // validity depth of cu
  bool in64 = false;  // the current iterate already sits in (outu, outp)
  auto more = [&](const GridLevel* C, const float2* cf, const double* cdu, const double* cdp, bool last) -> int {
    if (xv < K) {
      const int r = halo_level_f(h, l, cu);
      if (r) return r;
      xv = g;
    }
    const bool out64 = last && outu;
    pgxk_f_smooth(h->st, K, 0, L, h->alpha, cu, nullptr, nullptr, C, cf, cdu, cdp, omega, remap, ou, out64 ? outu : nullptr,
                  out64 ? outp : nullptr);
    std::swap(cu, ou);
    in64 = out64;
    xv -= K;
    return PGX_OK;
  };
  for (int s = 1; s < nl; ++s)
    if ((rc = more(nullptr, nullptr, nullptr, nullptr, false))) return rc;
  if (xv < 2) {  // P^T (b - J x) on the owned coarse rows reads the residual one row out, i.e. x two rows out
    if ((rc = halo_level_f(h, l, cu))) return rc;
    xv = g;
  }
  const GridLevel* C;
  const float2* cf = nullptr;
  const double *cdu = nullptr, *cdp = nullptr;
  if (l + 1 < D.ldist) {
    GridLevel& Cl = h->lev[l + 1];
    if (Cl.f32) {
      pgxk_f_resid_restrict(h->st, L, h->alpha, cu, Cl, remap, Cl.bf, nullptr, nullptr);
      if ((rc = vcycle_dist_f(h, l + 1, nullptr, nullptr, nullptr, nullptr, D.L[l + 1].g, nu, omega, &cf))) return rc;
    } else {
      pgxk_f_resid_restrict(h->st, L, h->alpha, cu, Cl, remap, nullptr, Cl.bu, Cl.bp);
      if ((rc = vcycle_dist(h, l + 1, Cl.bu, Cl.bp, Cl.xu, Cl.xp, D.L[l + 1].g, nu, omega))) return rc;
      cdu = Cl.xu;
      cdp = Cl.xp;
    }
    C = &Cl;
  } else {
    // the replicated level takes an fp64 right-hand side: it is summed over the ranks
    rc = replicated_step(h, l, nu, omega, [&](const GridLevel& V) {
      pgxk_f_resid_restrict(h->st, L, h->alpha, cu, V, remap, nullptr, V.bu, V.bp);
    });
    if (rc) return rc;
    C = &D.view;
    cdu = D.view.xu;
    cdp = D.view.xp;
  }
  // x + P x_c is correct to depth min(xv, g): the coarse correction covers every local row
  if ((rc = more(C, cf, cdu, cdp, nl == 1))) return rc;
  for (int s = 1; s < nl; ++s)
    if ((rc = more(nullptr, nullptr, nullptr, nullptr, s + 1 == nl))) return rc;
  if (xv < need_out) {
    if ((rc = in64 ? halo_level(h, l, outu, outp) : halo_level_f(h, l, cu))) return rc;
    xv = g;
  }
  if (res) *res = cu;
  return PGX_OK;
}

// owned entries of a local (u | psi) vector <-> owned-compact vector [u_owned | psi_owned]
void gather_owned(pgx_handle* h, const double* loc, double* cmp) {
  const Dist& D = h->dist;
  const size_t nf = D.nk_field(), nd = (size_t)h->nd, nv = (size_t)h->n;
  for (int f = 0; f < 2; ++f) {
    hipMemcpyAsync(cmp + f * nf, loc + f * nd + D.own_off, sizeof(double) * D.own_cnt, hipMemcpyDeviceToDevice, h->st);
    if (D.eown_cnt)
      hipMemcpyAsync(cmp + f * nf + D.own_cnt, loc + f * nd + nv + D.eown_off, sizeof(double) * D.eown_cnt, hipMemcpyDeviceToDevice,
                     h->st);
  }
}
static void scatter_owned(pgx_handle* h, const double* cmp, double* loc) {
  const Dist& D = h->dist;
  const size_t nf = D.nk_field(), nd = (size_t)h->nd, nv = (size_t)h->n;
  for (int f = 0; f < 2; ++f) {
    hipMemcpyAsync(loc + f * nd + D.own_off, cmp + f * nf, sizeof(double) * D.own_cnt, hipMemcpyDeviceToDevice, h->st);
    if (D.eown_cnt)
      hipMemcpyAsync(loc + f * nd + nv + D.eown_off, cmp + f * nf + D.own_cnt, sizeof(double) * D.eown_cnt, hipMemcpyDeviceToDevice,
                     h->st);
  }
}

// P2: two-level cycle.  Smoother = collective damped Jacobi on the P2 block CSR (k_bspmv<2>); coarse space =
// the P1 subspace with its full multigrid hierarchy (one V-cycle); T = P1->P2 interpolation.
// Patch data of the P2 level: tables on first use, inverses once per Jacobian (alpha and D(psi) change every Newton step)
int ensure_patches(pgx_handle* h) {
  const int NN = h->patch_nn, nv = h->n, nd = h->nd;
  if (!h->pdof) {
    DALLOC(h->pdof, (size_t)nv * NN);
    DALLOC(h->ppos, (size_t)nv * NN * NN);
    {
      uint8_t* q = nullptr;
      DALLOC(q, pgxk_patch_inverse_bytes(nv, NN, h->patch_f32, h->patch_sym));
      h->pinv = q;
    }
    if (h->p2_resid_f32) DALLOC(h->s_Df, (size_t)h->s_nnz);
    DALLOC(h->p2_su, (size_t)2 * (nd - nv));
    DALLOC(h->p2_sp, (size_t)2 * (nd - nv));
    HIPCHK(hipMemcpy(h->pdof, h->patch_dof_host.data(), sizeof(int32_t) * h->patch_dof_host.size(), hipMemcpyHostToDevice));
    std::vector<int32_t>().swap(h->patch_dof_host);
    pgxk_patch_positions(h->st, nv, NN, h->pdof, h->s_rowptr, h->s_colm, h->ppos);
    if (!h->wide_v_host.empty()) {  // wide stars: their own tables and full-row inverses, float unless the narrow form is double
      // (filled in place: whatever an early return leaves behind is the handle's - dalloc lists every allocation in h->allocs -, and
      // nw, which switches the wide launches on, is set last)
      PgxWidePatches& W = h->wide;
      const int nw = (int)h->wide_v_host.size();
      W.f32 = h->patch_f32 ? 1 : 0;
      DALLOC(W.verts, nw);
      DALLOC(W.dof, (size_t)nw * PGX_PATCH_WIDE_NN);
      DALLOC(W.pos, (size_t)nw * PGX_PATCH_WIDE_NN * PGX_PATCH_WIDE_NN);
      {
        uint8_t* q = nullptr;
        DALLOC(q, pgxk_patch_wide_inverse_bytes(nw, W.f32));
        W.inv = q;
      }
      HIPCHK(hipMemcpy(W.verts, h->wide_v_host.data(), sizeof(int32_t) * h->wide_v_host.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(W.dof, h->wide_dof_host.data(), sizeof(int32_t) * h->wide_dof_host.size(), hipMemcpyHostToDevice));
      pgxk_patch_positions(h->st, nw, PGX_PATCH_WIDE_NN, W.dof, h->s_rowptr, h->s_colm, W.pos);
      W.nw = nw;
    }
  }
  if (!h->patch_fresh) {
    pgxk_patch_invert(h->st, nv, NN, h->pdof, h->ppos, h->s_K, h->s_M, h->s_D, h->mask, h->alpha, h->pinv, h->patch_f32, h->patch_sym);
    pgxk_patch_invert_wide(h->st, h->wide, h->s_K, h->s_M, h->s_D, h->mask, h->alpha);
    if (h->s_Df) pgxk_to_float(h->st, (size_t)h->s_nnz, h->s_D, h->s_Df);
    h->patch_fresh = true;
  }
  return PGX_OK;
}

// The two launches of a sweep of the cycle below, shared by it and by the test hook pgx_p2_cycle_apply.
// Residual kernel of the cycle: 2 structured apply (pgx_p2st.hip; refreshes its copies of D once per Jacobian), 1 nnz-balanced CSR,
// 0 plain CSR
int p2_cycle_resid_kind(pgx_handle* h) {
  if (h->spmv_bal && p2st_ready(h)) return 2;
  return (h->spmv_bal && h->s_blk) ? 1 : 0;
}
// (p2_ru, p2_rp) = b - J x
void p2_cycle_resid(pgx_handle* h, int kind, const double* xu, const double* xp, const double* bu, const double* bp) {
  const int nd = h->nd;
  if (kind == 2)
    p2st_apply(h, xu, xp, bu, bp, h->p2_ru, h->p2_rp, true);
  else if (kind == 1)
    pgxk_bspmv_bal(h->st, nd, h->s_nblk, h->s_blk, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_code, h->s_tab, h->s_D, h->alpha, h->mask, xu, xp, bu,
                   bp, h->xcd_remap ? 1 : 0, h->p2_ru, h->p2_rp, h->s_Df);
  else
    pgxk_bspmv(h->st, 1, nd, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_D, h->alpha, xu, xp, bu, bp, 0.0, h->xcd_remap,
               h->p2_ru, h->p2_rp);
}
// x += patch_omega * (averaged patch solves of r)
void p2_cycle_patch(pgx_handle* h, const double* ru, const double* rp, double* xu, double* xp) {
  const int nd = h->nd, nv = h->n;
  pgxk_patch_sweep(h->st, nv, h->patch_nn, nv, nd, h->pdof, h->edge_ends, h->pinv, h->patch_f32, h->patch_sym, ru, rp, h->patch_omega, xu, xp, h->p2_su, h->p2_sp,
                   h->wide.nw ? &h->wide : nullptr);
}

// Two-level cycle with the vertex-star patch smoother (round 3): patch_nu additive sweeps | P1 hierarchy on T^T (b - J x) |
// patch_nu sweeps.  A sweep = residual (block-CSR SpMV) + one pass over the patch inverses.
static void pcycle_p2_patch(pgx_handle* h, const double* bu, const double* bp, double* xu, double* xp, int nu, double omega) {
  const int nd = h->nd, nv = h->n;
  const int kind = p2_cycle_resid_kind(h);
  auto resid = [&]() { p2_cycle_resid(h, kind, xu, xp, bu, bp); };
  auto patch = [&](const double* ru, const double* rp) { p2_cycle_patch(h, ru, rp, xu, xp); };
  hipMemsetAsync(xu, 0, sizeof(double) * nd, h->st);
  hipMemsetAsync(xp, 0, sizeof(double) * nd, h->st);
  patch(bu, bp);  // x = 0: the residual is b
  for (int s2 = 1; s2 < h->patch_nu; ++s2) {
    resid();
    patch(h->p2_ru, h->p2_rp);
  }
  resid();
  pgxk_p2_restrict(h->st, nv, nd, h->v2e_ptr, h->v2e, h->mask, h->p2_ru, h->p2_rp, h->c1_bu, h->c1_bp);
  vcycle(h, 0, h->c1_bu, h->c1_bp, h->c1_xu, h->c1_xp, nu, omega);
  pgxk_p2_prolong_add(h->st, nv, nd, h->edge_ends, h->c1_xu, h->c1_xp, xu, xp);
  for (int s2 = 0; s2 < h->patch_nu; ++s2) {
    resid();
    patch(h->p2_ru, h->p2_rp);
  }
}

// The same cycle on a strip (sharded P2, round 3).  Validity depth = number of ghost vertex rows on which a local vector equals the
// global one.  An exchange (halo_solution) restores depth g; a residual b - J x reads one row further out than it writes (-1); a patch
// solve needs the residual on its whole star and an edge average both end patches (-1): a sweep = residual + patches costs 2 rows.
// The P1 hierarchy below is vcycle_dist, which exchanges for itself.  Exchanges are issued only when the depth runs out - with the
// default ghost depth (24 rows at three distributed levels) that is the one exchange of the right-hand side.
static int pcycle_p2_patch_dist(pgx_handle* h, double* bu, double* bp, double* xu, double* xp, int nu, double omega) {
  const int nd = h->nd, nv = h->n, NN = h->patch_nn;
  const int g = h->dist.L[0].g;
  int rc = halo_solution(h, bu, bp);  // the Krylov vector is correct on owned dofs only
  if (rc) return rc;
  int xv = 0;  // validity depth of (xu, xp)
  auto need = [&](int depth) -> int {
    if (xv >= depth) return PGX_OK;
    const int r = halo_solution(h, xu, xp);
    xv = g;
    return r;
  };
  const bool st_apply = h->spmv_bal && p2st_ready(h);
  auto resid = [&]() {
    if (st_apply)
      p2st_apply(h, xu, xp, bu, bp, h->p2_ru, h->p2_rp, true);
    else
      pgxk_bspmv_bal(h->st, nd, h->s_nblk, h->s_blk, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_code, h->s_tab, h->s_D, h->alpha, h->mask, xu, xp, bu,
                     bp, h->xcd_remap ? 1 : 0, h->p2_ru, h->p2_rp, h->s_Df);
    xv -= 1;
  };
  auto patch = [&](const double* ru, const double* rp) {
    pgxk_patch_sweep(h->st, nv, NN, nv, nd, h->pdof, h->edge_ends, h->pinv, h->patch_f32, h->patch_sym, ru, rp, h->patch_omega, xu, xp, h->p2_su, h->p2_sp);
    xv -= 1;
  };
  if (!h->s_blk) {
    h->err = "sharded P2: no balanced SpMV blocks";
    return PGX_ESTATE;
  }
  hipMemsetAsync(xu, 0, sizeof(double) * nd, h->st);
  hipMemsetAsync(xp, 0, sizeof(double) * nd, h->st);
  xv = g;  // zero is right everywhere
  patch(bu, bp);
  for (int s2 = 1; s2 < h->patch_nu; ++s2) {
    if ((rc = need(3))) return rc;
    resid();
    patch(h->p2_ru, h->p2_rp);
  }
  if ((rc = need(3))) return rc;
  resid();  // valid to depth >= 2: the P1 restriction reads the residual one row out on the owned coarse rows
  pgxk_p2_restrict(h->st, nv, nd, h->v2e_ptr, h->v2e, h->mask, h->p2_ru, h->p2_rp, h->c1_bu, h->c1_bp);
  if ((rc = vcycle_dist(h, 0, h->c1_bu, h->c1_bp, h->c1_xu, h->c1_xp, g, nu, omega))) return rc;
  pgxk_p2_prolong_add(h->st, nv, nd, h->edge_ends, h->c1_xu, h->c1_xp, xu, xp);
  xv = std::min(xv, g - 1);  // the edge part of T x_c reads both end vertices
  for (int s2 = 0; s2 < h->patch_nu; ++s2) {
    if ((rc = need(3))) return rc;
    resid();
    patch(h->p2_ru, h->p2_rp);
  }
  return need(2);  // the operator apply that follows reads one row beyond the strip
}

static void pcycle_p2(pgx_handle* h, const double* bu, const double* bp, double* outu, double* outp, int nu,
                      double omega) {
  const int nd = h->nd;
  const int nu2 = nu + 1;
  const double om2 = 0.75 * omega;
  auto app = [&](int mode, const double* xu, const double* xp, int first, double* yu, double* yp) {
    pgxk_bspmv(h->st, mode, nd, h->s_rowptr, h->s_colm, h->s_K, h->s_M, h->s_D, h->alpha, xu, xp, bu, bp, om2,
               first | h->xcd_remap, yu, yp);
  };
  double *Au = outu, *Ap = outp, *Bu = h->p2_xu, *Bp = h->p2_xp;
  bool toA = false;  // 2*nu2 sweeps in total (even): start in B so that the last one lands in A
  const double *cu = nullptr, *cp = nullptr;
  auto sweep = [&](int first) {
    double* tu = toA ? Au : Bu;
    double* tp = toA ? Ap : Bp;
    app(2, cu, cp, first, tu, tp);
    cu = tu;
    cp = tp;
    toA = !toA;
  };
  for (int s2 = 0; s2 < nu2; ++s2) sweep(s2 == 0);
  app(1, cu, cp, 0, h->p2_ru, h->p2_rp);
  pgxk_p2_restrict(h->st, h->n, nd, h->v2e_ptr, h->v2e, h->mask, h->p2_ru, h->p2_rp, h->c1_bu, h->c1_bp);
  vcycle(h, 0, h->c1_bu, h->c1_bp, h->c1_xu, h->c1_xp, nu, omega);
  pgxk_p2_prolong_add(h->st, h->n, nd, h->edge_ends, h->c1_xu, h->c1_xp, (double*)cu, (double*)cp);
  for (int s2 = 0; s2 < nu2; ++s2) sweep(0);
  if (cu != Au) {  // odd nu: final sweep landed in the scratch pair
    hipMemcpyAsync(Au, cu, sizeof(double) * nd, hipMemcpyDeviceToDevice, h->st);
    hipMemcpyAsync(Ap, cp, sizeof(double) * nd, hipMemcpyDeviceToDevice, h->st);
  }
}

// Values of the mixed Newton matrix [[alpha K, M],[M, -D]] with the Dirichlet rows/columns of the u block replaced by
// identity (the contract of problem.py:69-77), in the CSR layout: row i -> [cols_s(i) | nd + cols_s(i)], row nd+i likewise.
__global__ void k_mixed_vals(int nd, int nnz, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colm,
                             const double* __restrict__ K, const double* __restrict__ M, const double* __restrict__ D,
                             double alpha, const uint8_t* __restrict__ mask, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nd) return;
  const int b = rowptr[i], e = rowptr[i + 1], len = e - b;
  const bool rowbc = mask[i] != 0;
  double* uu = out + 2 * (size_t)b;
  double* up = uu + len;
  double* pu = out + 2 * (size_t)nnz + 2 * (size_t)b;
  double* pp = pu + len;
  for (int k = b; k < e; ++k) {
    const int32_t cm = colm[k];
    const bool colbc = cm < 0;
    const int c = cm & 0x7fffffff;
    const double m = M[k];
    uu[k - b] = (rowbc || colbc) ? ((rowbc && c == i) ? 1.0 : 0.0) : alpha * K[k];
    up[k - b] = rowbc ? 0.0 : m;
    pu[k - b] = colbc ? 0.0 : m;
    pp[k - b] = -D[k];
  }
}

// symbolic phase of the direct solver, once per handle (first Newton solve that asks for pc_type lu)
int ensure_lu(pgx_handle* h) {
  if (h->lu) return PGX_OK;
  if (h->dist.on) {
    h->err = "pc_type lu is not available on a sharded handle";
    return PGX_EINVAL;
  }
  const int nd = h->nd, n = h->n;
  const std::vector<int32_t>& hr = (h->degree == 2) ? h->s_h_rowptr : h->h_rowptr;
  const std::vector<int32_t>& hc = (h->degree == 2) ? h->s_h_col : h->h_col;
  const int64_t nnz = hr[nd];
  if ((int64_t)4 * nnz > 0x7fffffff) {
    h->err = "pc_type lu: mixed matrix exceeds int32 nnz";
    return PGX_EINVAL;
  }
  std::vector<int32_t> rp(2 * (size_t)nd + 1), cl(4 * (size_t)nnz), nod(2 * (size_t)nd);
  for (int i = 0; i < nd; ++i) {
    const int b = hr[i], len = hr[i + 1] - b;
    rp[i] = 2 * b;
    rp[nd + i] = (int32_t)(2 * nnz + 2 * b);
    for (int k = 0; k < len; ++k) {
      const int32_t c = hc[b + k] & 0x7fffffff;
      if (k > 0 && (hc[b + k - 1] & 0x7fffffff) >= c) {
        h->err = "pc_type lu: scalar pattern is not sorted";
        return PGX_EINVAL;
      }
      cl[2 * (size_t)b + k] = c;
      cl[2 * (size_t)b + len + k] = nd + c;
      cl[2 * (size_t)nnz + 2 * (size_t)b + k] = c;
      cl[2 * (size_t)nnz + 2 * (size_t)b + len + k] = nd + c;
    }
    nod[i] = nod[nd + i] = i;
  }
  rp[2 * (size_t)nd] = (int32_t)(4 * nnz);
  std::vector<double> xy(2 * (size_t)nd);
  HIPCHK(hipMemcpy(xy.data(), h->coords, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
  if (h->degree == 2) {
    std::vector<int32_t> ends(2 * (size_t)(nd - n));
    HIPCHK(hipMemcpy(ends.data(), h->edge_ends, sizeof(int32_t) * ends.size(), hipMemcpyDeviceToHost));
    for (int e = 0; e < nd - n; ++e)
      for (int d = 0; d < 2; ++d) xy[2 * (size_t)(n + e) + d] = 0.5 * (xy[2 * (size_t)ends[2 * e] + d] + xy[2 * (size_t)ends[2 * e + 1] + d]);
  }
  pgx_nd_matrix A{};
  A.n = 2 * (int64_t)nd;
  A.rowptr = rp.data();
  A.col = cl.data();
  A.n_nodes = nd;
  A.node_of_dof = nod.data();
  A.dim = 2;
  A.node_coords = xy.data();
  A.leaf_nodes = 0;
  if (const char* e = pgx_tune("PGX_ND_LEAF")) A.leaf_nodes = atoi(e);
  int rc = h->lu_comm ? pgx_nd_create_dist(&A, h->lu_comm, h->device, (void*)h->st, &h->lu)
                      : pgx_nd_create(&A, h->device, (void*)h->st, &h->lu);
  if (rc) {
    h->err = std::string("pc_type lu: ") + pgx_nd_last_error(nullptr);
    h->lu = nullptr;
    return rc;
  }
  // [[alpha K, M], [M, -D(psi)]] with identity Dirichlet rows AND columns is symmetric: L D L^T in LU clothing, half the flops
  // (include/pgx_nd.h; ignored on a distributed handle); the factorisation preconditions FGMRES on the exact operator either way
  pgx_nd_set_symmetric(h->lu, 1);
  DALLOC(h->Jmix, 4 * (size_t)nnz);
  return PGX_OK;
}

// replicas of pgx_create_lu_dist: overwrite dev[0:n) with rank 0's copy (all-reduce of "mine if rank 0 else zero")
static int replica_bcast(pgx_handle* h, double* dev, size_t n) {
  if (!h->lu_comm || h->lu_comm->size == 1) return PGX_OK;
  if (h->lu_comm->rank != 0) HIPCHK(hipMemsetAsync(dev, 0, n * sizeof(double), h->st));
  const int rc = h->lu_comm->allreduce(h->st, dev, n);
  if (rc) h->err = "replica broadcast: " + h->lu_comm->err;
  return rc;
}
// The replicas assemble redundantly and every assembly kernel is atomic-free (fixed summation order), so their residuals are
// bitwise identical and nothing needs to be broadcast.  PGX_CHECK_REPLICAS=1 turns that claim into a run-time assertion
// (tests): rank 0's copy travels to every rank and must equal the local one exactly.  Collective; h->w is the scratch.
int replica_check(pgx_handle* h, const double* dev, size_t n, const char* what) {
  if (!h->lu_comm || h->lu_comm->size == 1 || !h->check_replicas) return PGX_OK;
  HIPCHK(hipMemcpyAsync(h->w, dev, n * sizeof(double), hipMemcpyDeviceToDevice, h->st));
  int rc = replica_bcast(h, h->w, n);
  if (rc) return rc;
  pgxk_axpy(h->st, n, -1.0, dev, h->w);
  pgxk_multidot(h->st, n, 1, h->w, 0, h->w, h->partials, h->d_small);
  if ((rc = h->lu_comm->allreduce(h->st, h->d_small, 1))) {  // sum of the ranks' squared differences: one verdict for all
    h->err = "replica check: " + h->lu_comm->err;
    return rc;
  }
  HIPCHK(hipMemcpyAsync(h->h_small, h->d_small, sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (h->h_small[0] != 0.0) {
    h->err = std::string("replicas of a distributed-LU handle disagree on ") + what;
    return PGX_ECOMM;
  }
  return PGX_OK;
}

int lu_factor(pgx_handle* h) {
  PhaseTimer t(h, 2);
  hipLaunchKernelGGL(k_mixed_vals, dim3((h->nd + 127) / 128), dim3(128), 0, h->st, h->nd, h->s_nnz, h->s_rowptr, h->s_colm,
                     h->s_K, h->s_M, h->s_D, h->alpha, h->mask, h->Jmix);
  int rc = pgx_nd_factor(h->lu, h->Jmix, 1);
  if (rc) h->err = std::string("pc_type lu: ") + pgx_nd_last_error(h->lu);
  return rc;
}

int precond(pgx_handle* h, const double* b, double* z, int nu, double omega) {
  if (h->lu_active) {
    int rc = pgx_nd_solve(h->lu, b, z, 1);
    if (rc) h->err = std::string("pc_type lu: ") + pgx_nd_last_error(h->lu);
    return rc;
  }
  if (h->dist.on) {  // b is owned-compact, z local (owned + ghost rows, correct at least one row beyond the strip)
    scatter_owned(h, b, h->dist.sb);
    ++h->dist.n_vcycle;
    if (h->degree == 2) {
      if (!h->patch_nn) {
        h->err = "sharded P2 needs the vertex-star patch smoother (vertex degree <= 7)";
        return PGX_EINVAL;
      }
      int rc = ensure_patches(h);
      if (rc) return rc;
      return pcycle_p2_patch_dist(h, h->dist.sb, h->dist.sb + h->nd, z, z + h->nd, nu, omega);
    }
    return vcycle_dist(h, 0, h->dist.sb, h->dist.sb + h->n, z, z + h->n, 1, nu, omega);
  }
  if (h->degree == 2 && h->p2_patch && h->patch_nn) {  // vertex-star patch smoother on the P2 level, P1 hierarchy below
    const int rc = ensure_patches(h);
    if (rc) return rc;
    pcycle_p2_patch(h, b, b + h->nd, z, z + h->nd, nu, omega);
  } else if (h->degree == 2)  // round-1 cycle: point-collective Jacobi on the P2 level (meshes with vertex degree > 15, A/B)
    pcycle_p2(h, b, b + h->nd, z, z + h->nd, nu, omega);
  else
    vcycle(h, 0, b, b + h->n, z, z + h->n, nu, omega);
  return PGX_OK;
}
