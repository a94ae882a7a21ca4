// Internal: the handle behind include/pgx.h and what its five translation units share.  pgx_api.hip holds the tuning table, handle
// creation, state access, residual, Jacobian, operator apply and the Newton driver; pgx_setup.hip the plan building and the multigrid
// hierarchies; pgx_cycle.hip the preconditioner: the cycles, the collectives, the patch data and the sparse LU; pgx_hooks.hip the test
// and measurement hooks; pgx_krylov.hip FGMRES, the reductions' way to the host and their test hook.  Nothing here is exported from
// libpgx.so.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pgx.h"
#include "../../include/pgx_nd.h"
#include "pgx_comm.h"
#include "pgx_internal.h"

// Sharded path (include/pgx.h): geometry of this rank's strip on each distributed multigrid level.  Local vertex rows
// of level l are [ghost-low: glo | owned: H | ghost-high: ghi]; g = 2^(ldist-l) is the ghost depth: glo = g (0 on rank 0),
// ghi = g+1 (0 on the last rank, whose H includes the top row of the mesh).  Local row 0 is an even global row on every
// level, so vertex coarsening of the local grid IS the local part of the global coarsening.
struct DistLevel {
  int g, glo, H, ghi;
};
struct Dist {
  bool on = false;
  pgx_comm* comm = nullptr;
  int rank = 0, size = 1, ldist = 0, global_ny = 0;
  std::vector<DistLevel> L;
  GridLevel view{};  // this rank's rows of the first replicated level (pointers into that level's global arrays)
  int view_row0 = 0, view_glo = 0, view_H = 0, view_own0 = 0;
  long long n_halo = 0, n_allreduce = 0, n_vcycle = 0, n_krylov = 0;  // collective counts (pgx_comm_counts)
  double* view_S = nullptr;  // [7 * view.n] strip-shaped coarse stencils before they are merged into the global level
  size_t own_off = 0, own_cnt = 0;  // owned entries per field on level 0: [own_off, own_off + own_cnt)
  // P2 on strips: the edge dofs follow the vertex dofs of a field, ordered by their LOWER vertex (row-major), so the edges whose
  // lower vertex lies in one vertex row form one contiguous block of eb = 3 nx + 1 dofs (nx in the last local row).  An edge is
  // owned by the rank that owns its lower vertex: owned edges = [eown_off, eown_off + eown_cnt) of the edge part.
  size_t eb = 0, eown_off = 0, eown_cnt = 0;
  size_t nk_field() const { return own_cnt + eown_cnt; }  // owned dofs per field (Krylov vectors are owned-compact)
  int cell0 = 0, ncell_own = 0;     // owned cells (row-major cell order)
  double *sb = nullptr, *wc = nullptr;  // local scatter buffer (2n), owned-compact scratch (2*own_cnt)
};

// One level of the hierarchy of a refined general mesh (pgx_set_hierarchy; kernels: pgx_umg.hip).  Level 0 aliases the handle's own
// block CSR and level-0 scratch; a level l > 0 owns its operator, its vectors and the transfer from level l - 1 onto it.
struct UmgLevel {
  int n = 0, nnz = 0;
  int32_t *rowptr = nullptr, *colm = nullptr;  // colm as k_bspmv reads it: column | Dirichlet flag << 31
  double *K = nullptr, *M = nullptr, *D = nullptr;  // unconstrained values; levels > 0: P^T (.) P of the level above
  uint8_t* mask = nullptr;
  // transfer from level l - 1 (n_f vertices): parents [n_f][2]; child lists = P^T as CSR; Galerkin plan per entry of this level
  int32_t *parents = nullptr, *ch_ptr = nullptr, *ch_idx = nullptr, *plan_ptr = nullptr, *plan_src = nullptr;
  int plan_lpe = 4;       // lanes per coarse entry in k_umg_rap, from the mean plan-row length
  double *bu = nullptr, *bp = nullptr, *xu = nullptr, *xp = nullptr, *xu2 = nullptr, *xp2 = nullptr, *ru = nullptr, *rp = nullptr;
  std::vector<int32_t> h_rowptr, h_col;
  std::vector<uint8_t> h_mask;
  // transfer of a BUILT hierarchy (pgx_build_hierarchy; kernels: pgx_amg.hip) instead of `parents`: P as CSR over the n_f fine rows
  // with general weights (P_val != nullptr marks such a level); the child lists above carry the P entry of every child in ch_q.
  // Galerkin product in two gather stages: T = A P (nnz_t entries; per entry the pairs fine entry t_a, P entry t_p), then P^T T (per
  // entry of this level the pairs P entry g_p, T entry g_t).  The plans hold indices only, the weights are read from P_val.
  int nnz_p = 0, nnz_t = 0;
  int32_t *P_ptr = nullptr, *P_col = nullptr, *ch_q = nullptr;
  int32_t *t_ptr = nullptr, *t_a = nullptr, *t_p = nullptr, *g_ptr = nullptr, *g_p = nullptr, *g_t = nullptr;
  double *P_val = nullptr, *T = nullptr;
  std::vector<int32_t> h_P_ptr, h_P_col;
};
// defaults of pgx_build_hierarchy ("Built hierarchies": the variants measured on the numpy twin)
#define PGX_AMG_THETA 0.01
#define PGX_AMG_TRUNC 0.2
#define PGX_AMG_MIN_COARSE 60
#define PGX_AMG_MAX_KEEP 0.8

struct pgx_handle {
  int device = 0;
  Dist dist;
  hipStream_t st = nullptr;
  std::string err;
  int n = 0, nc = 0, nx = 0, ny = 0, nnz = 0;  // n = mesh vertices = dofs per field of the P1 space
  int degree = 1;
  int nd = 0;  // dofs per field of the SOLUTION space: n (P1) or n + n_edges (P2)
  bool structured = false;
  QuadTab q{};
  double f = 0.0, alpha = 1.0;
  // mesh + problem data
  double* coords = nullptr;
  int32_t* cells = nullptr;
  uint8_t* mask = nullptr;
  double *gbc = nullptr, *bphi = nullptr;
  // CSR pattern + inverted lists
  int32_t *rowptr = nullptr, *colm = nullptr, *v2c_ptr = nullptr, *v2c_ent = nullptr, *v2c_pos = nullptr;
  std::vector<int32_t> h_rowptr, h_col;
  size_t fill_lds = 0;
  double *Kv = nullptr, *Mv = nullptr, *Dv = nullptr;
  bool jac_valid = false;
  double* geoq = nullptr;  // order-2 geometry (pgx_create_curved): [cell][quadrature point][5] = |det J|, J^-1; nullptr = affine cells
  float2* zf_out = nullptr;  // FGMRES: the level-0 single-precision cycle leaves its result HERE as float2 (no fp64 copy); see fgmres
  int z_f32 = 1;             // PGX_Z_F32=0: the Z_j of the Krylov method in fp64 (A/B)
  int f32_dbf16 = 1;         // PGX_F32_DBF16=0: the single-precision cycle's D(psi) stencil as float4 (A/B); default: packed bf16, 8 B
  bool dv_lean = false;  // the interior rows of the CSR D values are stale (residual_dev(with_d = 2)); a full fill clears it
  // operator of the solution space (aliases the P1 arrays above for degree 1)
  int32_t *s_rowptr = nullptr, *s_colm = nullptr;
  double *s_K = nullptr, *s_M = nullptr, *s_D = nullptr;
  int s_nnz = 0;
  size_t s_fill_lds = 0;
  int32_t* s_blk = nullptr;  // P2: row blocks of the nnz-balanced stream kernel (k_bspmv_bal): s_nblk + 1 pairs (first row, its rowptr)
  int s_nblk = 0, spmv_bal = 1;
  uint8_t* s_code = nullptr;  // P2 on a uniform mesh: per entry the index of its (K, M) pair in s_tab (k_bspmv_bal<true>)
  double* s_tab = nullptr;    // 256 (K, M) pairs
  int s_ntab = 0, spmv_dict = 1;
  std::vector<int32_t> s_h_rowptr, s_h_col;
  // P2 extras: cell dofs, inverted lists of the P2 plan, P1<->P2 transfers, two-level cycle scratch
  QuadTab2 q2{};
  int32_t *cdofs = nullptr, *p2_v2c_ptr = nullptr, *p2_v2c_ent = nullptr, *p2_v2c_pos = nullptr;
  int32_t *v2e_ptr = nullptr, *v2e = nullptr, *edge_ends = nullptr;
  double *p2_xu = nullptr, *p2_xp = nullptr, *p2_ru = nullptr, *p2_rp = nullptr;
  double* p2_stash = nullptr;  // [16 * nc] element residual vectors of the P2 assembly (deterministic scatter, pgx_p2.hip)
  double *c1_bu = nullptr, *c1_bp = nullptr, *c1_xu = nullptr, *c1_xp = nullptr;
  // vertex-star patch smoother of the P2 level (pgx_patch.hip): NN = slots per patch (0: vertex degree > 15, smoother unavailable; 8 ... 15: see `wide`)
  int patch_nn = 0, p2_patch = 1, patch_nu = 2;
  int p2_fallback_its = 60, p2_fallbacks = 0;  // patch cycle -> sparse LU after this many Krylov iterations without convergence
  double patch_omega = 0.8;
  bool patch_fresh = false;  // pinv holds the inverses of the current Jacobian
  std::vector<int32_t> patch_dof_host;
  int32_t *pdof = nullptr, *ppos = nullptr;
  void* pinv = nullptr;  // patch inverses: float by default (a smoother inside FGMRES: same Krylov counts as double at 512^2 ... 2048^2,
                         // half the bytes of the stream that bounds the sweep), double with the tuning key PGX_P2_PATCH_F32=0
  int patch_f32 = 1;
  // structured P2 operator apply (pgx_p2st.hip): interior groups [i0, i0 + ni) x [j0, j0 + nj) through the table-driven kernel,
  // the frame rows through the CSR form.  state: 0 off, 1 pattern verified (K / M constants not yet fetched), 2 ready
  struct P2St {
    int state = 0, enable = 1, dist_enable = 1, select = 1, i0 = 0, ni = 0, j0 = 0, nj = 0, nframe = 0, ref_rows[4] = {0, 0, 0, 0};
    P2StTab tab;
    double K[46];
    double* Dst = nullptr;
    float* Dstf = nullptr;
    int32_t* frame = nullptr;
    bool fresh = false;
  } p2st;
  float* s_Df = nullptr;  // float copy of D(psi) for the residuals inside the P2 cycle (k_bspmv_bal<., true>); PGX_P2_RESID_F32=0: fp64
  int p2_resid_f32 = 1;
  int patch_sym = 1;     // float inverses in symmetric packing (pgx_patch.hip: 512 instead of 896 B per patch); PGX_P2_PATCH_SYM=0: full rows
  double *p2_su = nullptr, *p2_sp = nullptr;
  // wide stars: the vertices of degree 8 ... 15 of a mesh whose other stars fit the 16-lane kernels (patch_nn = 8; their rows of the
  // narrow table are all -1).  PGX_P2_PATCH_WIDE=0: no wide set, such a mesh has no patch smoother (patch_nn = 0), as before (A/B)
  int patch_wide = 1;
  PgxWidePatches wide;
  std::vector<int32_t> wide_v_host, wide_dof_host;
  // state
  double *x = nullptr, *xk = nullptr, *F = nullptr, *dx = nullptr, *xw = nullptr, *rhs = nullptr;
  // Krylov workspace
  int restart = 0;
  double *V = nullptr, *Z = nullptr, *w = nullptr, *d_small = nullptr, *partials = nullptr, *partials2 = nullptr;
  double* h_small = nullptr;  // pinned, mapped: the device publishes small results into it (fetch_small), the host polls
  double* h_small_dev = nullptr;              // device view of h_small
  unsigned long long* h_seq = nullptr;        // sequence word behind the payload (host view / device view)
  unsigned long long* h_seq_dev = nullptr;
  unsigned long long seq = 0;
  int lean_d = 1;           // PGX_LEAN_D=0: the Newton loop always writes the CSR form of D(psi) as well
  int spmv_d4 = 1;          // PGX_SPMV_D4=0: the matrix-free operator apply reads the four D arrays instead of its double4 copy
  int lazy_norm = 1;        // PGX_LAZY_NORM=0: every new Krylov vector is normalised in place (one more pass over it per iteration)
  double rhs_scale = 1.0;   // factor the next level-0 V-cycle applies to its fp64 right-hand side as it reads it (lazy normalisation)
  const float* rhs_f32 = nullptr;  // != nullptr: the next level-0 single-precision cycle reads its right-hand side HERE, as the float pair
                                   // (rhs_f32, rhs_f32 + n) - a vector of FGMRES's float basis - instead of the fp64 pair it is called with
  int v_f32 = 1;            // PGX_V_F32=0: the Krylov basis of the lean P1 path in fp64 (see fgmres)
  double v_f32_gain = 1e-4; // PGX_V_F32_GAIN: a cycle on the float basis ends once its estimate is below this factor times its starting residual
  double v_f32_max = 1e30;  // PGX_V_F32_MAX: a new basis vector with a norm above this (or not finite) does not fit a float: guard in fgmres
  int v_f32_min = 1000000;  // PGX_V_F32_MIN: the float basis from this many vertices up, where the Gram-Schmidt passes are bound by HBM
                            // bandwidth; below, its few extra iterations and cycles are not paid back by the halved streams
  bool v_f32_off = false;   // the guard fired: fp64 basis for the rest of this Newton solve (reset by pgx_newton_solve, like omega_now)
  int host_poll = 1;  // PGX_HOST_POLL=0: hipMemcpyAsync + hipStreamSynchronize for every small read-back (round 3)
  // Krylov / Newton driver passes (single handles with host_poll; the last three only with the matrix-free P1 operator: krylov_lean())
  int gs_wide = 16;       // PGX_GS_WIDE=8: Gram-Schmidt launches of at most 8 basis vectors (k_multidot / k_multiaxpy_norm; 16: one pass over w up to 16)
  int fused_publish = 1;  // PGX_FUSED_PUBLISH=0: second reduction stage (k_reduce_rows / k_reduce_partials) and k_publish as two launches
  int ticket_reduce = 1;  // PGX_TICKET_REDUCE=0: the second stage (and the publish) as a launch of its own behind k_multidot, k_multiaxpy_norm
                          // and k_axpy_norms; 1: their last block to arrive runs it (PgxTicket).  Only with fused_publish, see read_back_route()
  unsigned long long* d_ticket = nullptr;  // the ticket counters (PGX_TK_WORDS): zeroed when the handle is created, set back to zero by the
                                           // last block of every ticketed launch, freed with the handle
  int fused_resid = 1;    // PGX_FUSED_RESID=0: true residual of a restart cycle as operator apply + k_scale_copy(-1) + k_axpy(+b)
  int lean_rhs = 1;       // PGX_LEAN_RHS=0: the Newton loop forms rhs = -F as a vector, fgmres zero-fills x and accumulates into it
  int fused_step = 1;     // PGX_FUSED_STEP=0: xw += dx as k_axpy, |dx| and |xw| as two dev_norm calls with a read-back each
  // multigrid
  std::vector<GridLevel> lev;
  double *tmp_u = nullptr, *tmp_p = nullptr, *res_u = nullptr, *res_p = nullptr;  // level-0 scratch (each n)
  double omega_now = 0.0;  // smoother damping in force for the current Newton solve (fgmres lowers it on stagnation)
  int coarse_sweeps = 4;  // prototype (oracle/krylov_proto.py): 2..60 sweeps give identical Krylov counts
  int tail_start = -1;  // first level handled by the fused k_mg_tail launch (-1: none)
  int xcd_remap = 2;    // bit 1 of the `first` kernel argument; PGX_XCD_REMAP=0 disables (A/B: +1..3 %)
  int tail_verts = 1100;
  int spmv_stream = 1;  // PGX_SPMV_STREAM=0: 8-lanes-per-row kernel instead of the CSR-stream kernel
  int nu_coarse = 0;    // PGX_NU_COARSE: cap on the sweeps of unfused (small) levels; 0 = same as the fine levels
  int fused_k3 = 1;     // PGX_FUSED_K3=0: two sweeps per launch even when nu is a multiple of 3
  int fused_legs = 1;   // PGX_FUSED_LEGS=0: one launch per sweep / residual / restriction / prolongation
  int fused_min = 4000;  // fused legs from 65^2 vertices up (measured with the row-mapped kernels: 2048^2 460 -> 451 ms, 1024^2
                         // 113.5 -> 106.4, 512^2 68.5 -> 61.5 against 60000; the first, tile-mapped kernels needed >= 60000)
  long cgs_skipped = 0, cgs_total = 0;  // Krylov iterations without the second Gram-Schmidt projection / all (PGX_CGS_REPORT)
  // second projection iff |w'|^2 < eta^2 |w|^2.  The textbook eta = 1/sqrt(2) re-orthogonalises 249 of 266 iterations at 2048^2 (a
  // good preconditioner makes w = J M^-1 v_j ~ v_j: the first projection always cancels most of w); eta = 0.01 bounds the loss of
  // orthogonality per step by 100 eps, re-orthogonalises 11 of 266 and leaves every Krylov count unchanged: 448 -> 416 ms per solve
  double cgs_eta2 = 1e-4;
  TailArgs tail{};
  // hierarchy of a refined general mesh (pgx_set_hierarchy): empty = none, the handle runs as it did before that call existed
  std::vector<UmgLevel> umg;
  int umg_enable = 1;          // PGX_UMG=0: the single-level smoother although a hierarchy is attached (A/B)
  int umg_min = 20000;         // PGX_UMG_MIN: pc_type auto takes the cycle from this many vertices up, the sparse LU below.  20 381 vertices
                               // (disk_3) is the smallest size measured, and the cycle is already the faster of the two there; the crossover
                               // lies below and is not located (with what the figures include)
  int umg_min_p2 = 20000;      // PGX_UMG_MIN_P2: the same for a degree-2 handle (the patch cycle over this hierarchy first, the sparse LU as
                               // its rescue).  Handle creation plus all solves of a settings-B run: 0.18 against 0.44 s at 20 381 vertices,
                               // the smallest size measured, 0.39 / 1.24 s at 81 017, 1.32 / 4.29 s at 323 057 (profiles/p2_umg_disk_scaling.json)
  int umg_build_min = 2000;    // PGX_UMG_BUILD_MIN: a handle WITHOUT a hierarchy asked for the multigrid preconditioner (pc_type 1) builds
                               // one from this many vertices up (pgx_build_hierarchy_default).  Below, the single-level smoother such a
                               // handle always ran still converges (469 vertices: tests/golden/umg_d34_parent.npz).  That smoother needs
                               // twice the cycle's Krylov iterations at 1 319 vertices, runs into the iteration cap at 20 381 and
                               // fails to converge from 81 017
                               // (profiles/umg_disk_scaling.json).  Not a measured crossover
  int amg_build = 1;           // PGX_AMG_BUILD=0: pgx_build_hierarchy computes split and patterns in its host pass (pgx_amg.hip) instead of on
                               // the device (pgx_amg_build.hip); bitwise the same hierarchy (tests/test_gpu_amg_device.py)
  int amg_split_batch = 16;    // split launches of the device pass between two reads of its counter of decided vertices.  A mesh in its
                               // generator's order needs hundreds of launches at 300 000 vertices, so the host
                               // does not read after each.  PGX_AMG_SPLIT_BATCH lowers it FOR TESTS (1: a read after every launch)
  int amg_mode = -1;           // which of the two built this handle's hierarchy (-1: none built); pgx_amg_build_info
  std::vector<int32_t> amg_split;  // split launches per transfer of the device pass (0 each for the host pass)
  int umg_coarse_sweeps = 60;  // PGX_UMG_COARSE_SWEEPS
  int umg_coarse_lds = 1;      // PGX_UMG_COARSE_LDS=0: the coarsest level as repeated k_bspmv<2> launches although it fits one workgroup's LDS
  bool umg_coarse_fits = false;  // the coarsest level fits k_umg_coarse and this handle's device took its LDS limit (pgx_set_hierarchy)
  bool umg_idle = false;       // the current Newton solve preconditions with the sparse LU: nobody reads the coarse D, its fills skip it
                               // (the solve ends with jac_valid dropped, so the hooks never see that state)
  bool jac_ever = false;      // a Jacobian was filled at least once (pgx_set_hierarchy comes before that)
  // sparse direct preconditioner (pc_type lu): nested-dissection multifrontal LU of the mixed Newton matrix (pgx_nd.hip)
  pgx_nd* lu = nullptr;
  // pgx_create_lu_dist: this handle is one of `size` REPLICAS (whole mesh, whole iterate on every rank) whose sparse LU is
  // distributed over the ranks (pgx_nd_create_dist).  Residuals and observables are broadcast from rank 0 so that the
  // replicas stay bitwise identical (the P2 assembly uses atomics) and issue the same collectives.
  pgx_comm* lu_comm = nullptr;
  double* Jmix = nullptr;  // [4 * s_nnz] values of the mixed CSR matrix in the layout lu was created with
  bool dh_interior = false;
  // PGX_D_DIRECT (default 1; 0: the launches before it, for A/B): on a single handle of degree 1 with a uniform finest level the
  // kernels that compute D(psi) store every copy the solver reads - k_resid_fill_grid / k_resid_fill_frame write Dh, Dd4 and Dq of
  // level 0 (no k_csr_to_stencil_h, k_pack_d4, k_f_pack_d there), k_rap7h writes Dq of the coarse level it produces, and the
  // coarsenings onto levels of at least rap_lds_min vertices (PGX_RAP_LDS_MIN) stage their fine stencils in LDS.  Same bits.
  int d_direct = 1;
  int rap_lds_min = 60000;  // 257^2 and above: staged 7.2 against 9.7 us there, 13.4 / 22 at 513^2, 44 / 101 at 1025^2
  bool d0_direct = false;  // with dh_interior: the frame rows of lev[0].Dh and lev[0].Dd4 / Dq are in place as well (residual_dev)
  int stag_its = 12;       // PGX_STAG_ITS / PGX_STAG_GAIN: stagnation test of the smoother damping (fgmres)
  double stag_gain = 1e-4;
  int smooth_d32 = 0;      // PGX_SMOOTH_D32=1: the finest-level smoother reads a single-precision copy of the D stencils.  OFF by
                           // default: its launches get 10 % shorter, but the operator apply that follows the V-cycle no longer finds
                           // the double stencils in the Infinity Cache (k_st_spmv_r 0.74 -> 0.55 of the HBM peak) - net +0.9 %
  int k6_max = 0;          // levels with at most this many vertices run 6 sweeps per smoother launch (PGX_K6_MAX)
  int mg_f32 = 1;          // PGX_MG_F32=0: the round-3 fp64 V-cycle.  Default: single-precision V-cycle legs (pgx_mg32.hip) on every
                           // uniform level with at least f32_min vertices above the fused tail - half the bytes per launch
  int f32_min = 4000;      // PGX_F32_MIN
  int f32_k6_max = 4300000;  // PGX_F32_K6_MAX: levels with at most this many vertices (2049^2) run a whole leg of six sweeps as ONE launch,
                             // whether or not they fuse the restriction (f32_rr_max).  us per V-cycle at 2048^2 (round 4): off 459.7, up to
                             // 129^2 453.5, up to 257^2 448.5, up to 513^2 444.3; ms per solve: up to 513^2 162.6, up to 2049^2 150.2
  int f32_rr_max = 300000;   // PGX_F32_RR_MAX (measured, us per V-cycle from that level: 257^2 and below -2 each, 513^2 +3, 1025^2 +5, 2049^2 +12): levels with at most this many vertices fuse the residual + restriction into the last
                             // pre-smoothing launch (pgx_mg32.hip, RR mode)
  int resid_grid = 1;      // uniform structured P1: residual + D(psi) through k_resid_fill_grid (PGX_RESID_GRID=0: general kernel)
  // PGX_RESID_REUSE (default 1; 0: every entry evaluation in full, the launches before it).  A proximal step starts where the last
  // one ended: sol_k <- sol, another alpha, pgx_newton_solve again from sol.  Of the entry evaluation only F_u = alpha K u +
  // M (psi - psi_k) - alpha f load depends on what changed; F_psi and D(psi) depend on x alone, and the last evaluation of the solve
  // before left them in device memory.  valid says exactly that: F[nd .. 2 nd), lev[0].Dh (interior and frame), lev[0].Dd4 / Dq and,
  // with_d == 1, the CSR rows Dv hold the values at x, written by residual_dev(x, F, with_d) on the grid path, and dh_interior,
  // d0_direct, dv_lean are as that call left them.  (PGX_D_DIRECT=0: the interior of Dh and the CSR rows hold them; jacobian_dev
  // derives the frame of Dh, Dd4 and Dq from those, as after a full evaluation.)  Set in ONE place, the end of a converged
  // pgx_newton_solve.  Cleared by NEED():
  // every entry of the library that takes the handle drops it before it does anything, except the few that cannot write one of
  // those buffers or x (NEED_KEEP) - a missed reuse costs one exp pass, a stale one is a silent wrong answer.
  int resid_reuse = 1;
  struct ResidFresh {
    bool valid = false;
    int with_d = 0;
    bool dh_interior = false, d0_direct = false, dv_lean = false;
  } fresh;
  int64_t entry_full = 0, entry_reduced = 0;  // entry evaluations of pgx_newton_solve, in full / F_u only (pgx_resid_reuse_counts)
  int spmv_stencil = 1;    // structured P1: the outer-Krylov operator apply through the level-0 stencil kernels (matrix-free)
  bool lu_active = false;  // the current Newton solve preconditions with the factorisation
  bool check_replicas = false;  // PGX_CHECK_REPLICAS=1: assert that the replicas' residuals are bitwise identical
  // observables
  double *obs_partials = nullptr, *d_out6 = nullptr;
  int obs_blocks = 0;
  // profiling
  bool prof = false;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void*> allocs;
};

// the multilevel cycle of a refined general mesh is what this handle's preconditioner entry runs
static inline bool umg_on(const pgx_handle* h) { return h->umg.size() > 1 && h->umg_enable; }

#define HIPCHK(call)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
      return PGX_EHIP;                                                                          \
    }                                                                                           \
  } while (0)

template <typename T>
static int dalloc(pgx_handle* h, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) {
    h->err = std::string("hipMalloc: ") + hipGetErrorString(e);
    return PGX_ENOMEM;
  }
  h->allocs.push_back(q);
  *p = (T*)q;
  return PGX_OK;
}
#define DALLOC(p, count)                         \
  do {                                           \
    int rc_ = dalloc(h, &(p), (size_t)(count));  \
    if (rc_) return rc_;                         \
  } while (0)

// a host vector into device memory the handle owns (the hierarchies of general meshes: pgx_set_hierarchy, pgx_build_hierarchy)
template <typename T>
static int umg_upload(pgx_handle* h, T** dst, const std::vector<T>& src) {
  DALLOC(*dst, src.size());
  if (!src.empty()) HIPCHK(hipMemcpyAsync(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, h->st));
  return PGX_OK;
}

// Level 0 of a general-mesh hierarchy, attached or built: the handle's P1 block CSR on its vertices and its level-0 scratch; under a
// degree-2 handle Dv is T^T D_P2 T, refreshed by every fill.
static inline int umg_level0(pgx_handle* h, UmgLevel& L0) {
  L0.n = h->n;
  L0.nnz = h->nnz;
  L0.rowptr = h->rowptr;
  L0.colm = h->colm;
  L0.K = h->Kv;
  L0.M = h->Mv;
  L0.D = h->Dv;
  L0.mask = h->mask;
  L0.xu2 = h->tmp_u;
  L0.xp2 = h->tmp_p;
  L0.ru = h->res_u;
  L0.rp = h->res_p;
  L0.h_rowptr = h->h_rowptr;
  L0.h_col = h->h_col;
  L0.h_mask.resize(h->n);
  HIPCHK(hipMemcpy(L0.h_mask.data(), h->mask, h->n, hipMemcpyDeviceToHost));
  return PGX_OK;
}
// The finished levels become the handle's hierarchy.  The coarsest level in one launch: only where this handle's device accepts the
// kernel's LDS limit (set per device, here).
static inline void umg_install(pgx_handle* h, std::vector<UmgLevel>&& lv) {
  h->umg_coarse_fits = pgxk_umg_coarse_prepare(lv.back().n, lv.back().nnz);
  h->umg = std::move(lv);
  h->jac_valid = false;
}

struct PhaseTimer {
  pgx_handle* h;
  int slot;
  PhaseTimer(pgx_handle* h_, int s) : h(h_), slot(s) {
    static const char* const names[8] = {"pgx:residual", "pgx:jacobian", "pgx:mg_setup/lu_factor", "pgx:spmv", "pgx:precond",
                                         "pgx:orthogonalise", "pgx:observables", "pgx:newton_solve"};
    pgx_roctx(names[s & 7]);
    if (h->prof) hipEventRecord(h->e0, h->st);
  }
  ~PhaseTimer() {
    pgx_roctx(nullptr);
    if (h->prof) {
      hipEventRecord(h->e1, h->st);
      hipEventSynchronize(h->e1);
      float ms = 0;
      hipEventElapsedTime(&ms, h->e0, h->e1);
      h->ms[slot] += ms;
    }
  }
};

// NEED_KEEP: for the entries that leave pgx_handle::fresh standing - they write neither x, F, a D copy of level 0 nor anything F_psi
// or D(psi) are computed from (pgx_get_state, pgx_get_prev, pgx_set_prev, pgx_advance_prev, pgx_observables; pgx_newton_solve
// consumes it itself).  Every other entry takes NEED
#define NEED_KEEP(hh)          \
  if (!(hh)) return PGX_EINVAL; \
  hipSetDevice((hh)->device)
#define NEED(hh)  \
  NEED_KEEP(hh);  \
  (hh)->fresh.valid = false

#pragma GCC visibility push(hidden)
// ---- pgx_api.hip ----
extern thread_local std::string g_create_error;  // what pgx_last_error(nullptr) answers: a failed creation has no handle to ask
int copy_in(pgx_handle* h, double* dst, const double* src);   // 2 nd doubles host -> device, synchronous
int copy_out(pgx_handle* h, double* dst, const double* src);  // 2 nd doubles device -> host, synchronous
bool resid_reuse_on(const pgx_handle* h);                     // PGX_RESID_REUSE applies to this handle
void residual_dev(pgx_handle* h, const double* x, double* F, int with_d = 0, bool fu_only = false);
bool p2st_ready(pgx_handle* h);  // the structured P2 apply can run (refreshes its copies of D once per Jacobian)
void p2st_apply(pgx_handle* h, const double* xu, const double* xp, const double* bu, const double* bp, double* yu, double* yp, bool inner);
void spmv_dev(pgx_handle* h, const double* x, double* y);  // y = J x

// ---- pgx_setup.hip ----
int build_plan(pgx_handle* h, const pgx_mesh* m, const std::vector<uint8_t>& hmask);
int build_plan_p2(pgx_handle* h, const pgx_mesh* m, const std::vector<uint8_t>& hmask);
int build_km_dictionary(pgx_handle* h);
int ghost_mul();  // ghost depth multiplier of the sharded path (PGX_GHOST_MUL)
int build_multigrid(pgx_handle* h);
int build_multigrid_dist(pgx_handle* h);

// ---- pgx_cycle.hip ----
int precond(pgx_handle* h, const double* b, double* z, int nu, double omega);  // z = M^-1 b: one cycle, or the sparse LU
void level_apply(pgx_handle* h, int l, int mode, const double* xu, const double* xp, const double* bu, const double* bp, double omega,
                 int first, double* yu, double* yp);  // one stencil (or, level 0 of a general mesh, block-CSR) launch on level l
void vcycle(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega);
const float2* vcycle_f(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega);
void vcycle_umg(pgx_handle* h, int l, const double* bu, const double* bp, double* outu, double* outp, int nu, double omega);
bool f32_cycle_ok(const pgx_handle* h, int l, int nu);             // level l enters the single-precision cycle
int halo_solution(pgx_handle* h, double* fu, double* fp);          // sharded: ghost entries of a solution-space pair from their owners
int allreduce_dev(pgx_handle* h, double* dev, size_t n);           // sharded: sum over the ranks, on the stream
void gather_owned(pgx_handle* h, const double* loc, double* cmp);  // sharded: local vector -> owned-compact
int ensure_patches(pgx_handle* h);                                 // P2 patch data: tables on first use, inverses once per Jacobian
int p2_cycle_resid_kind(pgx_handle* h);
void p2_cycle_resid(pgx_handle* h, int kind, const double* xu, const double* xp, const double* bu, const double* bp);
void p2_cycle_patch(pgx_handle* h, const double* ru, const double* rp, double* xu, double* xp);
int ensure_lu(pgx_handle* h);  // symbolic phase of the sparse LU, once per handle
int lu_factor(pgx_handle* h);  // numeric factorisation of the current Jacobian
int replica_check(pgx_handle* h, const double* dev, size_t n, const char* what);  // PGX_CHECK_REPLICAS

// ---- pgx_amg.hip: the transfers of a built hierarchy (general weights), onto level C from the level above it ----
void pgxk_amg_direct(hipStream_t st, int n, const int32_t* ptr, const int32_t* src, const double* K, double* val);  // direct weights
void pgxk_amg_pvalues(hipStream_t st, int n, const int32_t* fptr, const int32_t* own, const int32_t* pptr, const int32_t* pa, const int32_t* pb,
                      const int32_t* diag, const double* K, const double* p0, double trunc, double* val);  // Jacobi step + truncation
// pgx_amg_build.hip: the device pass of pgx_build_hierarchy, arguments checked and defaulted
int pgx_amg_build_device(pgx_handle* h, double theta, double trunc, int32_t min_coarse, double max_keep, int32_t* n_levels, double* seconds);
void pgxk_amg_rap(hipStream_t st, const UmgLevel& C, const double* src, double* dst);  // dst = P^T (src) P through C.T
void pgxk_amg_resid_restrict(hipStream_t st, const UmgLevel& C, const double* ru, const double* rp);  // (C.bu, C.bp) = P^T (ru, rp)
void pgxk_amg_prolong_add(hipStream_t st, int n_f, const UmgLevel& C, double* xu, double* xp);         // (xu, xp) += P (C.xu, C.xp)

// ---- pgx_krylov.hip ----
int fgmres(pgx_handle* h, const double* b, double* x, const pgx_snes_opts* o, int* its_out, double* relres, double bnorm_known = -1.0,
           double bsign = 1.0);
int dev_norm(pgx_handle* h, const double* v, double* out, size_t len = 0);
int fetch_small(pgx_handle* h, const double* dsrc, size_t n, size_t hoff = 0, const double* dsrc2 = nullptr, size_t n2 = 0,
                size_t hoff2 = 0);
int replica_agree(pgx_handle* h, double* dev, size_t n);
bool krylov_lean(const pgx_handle* h);
bool z_f32_active(const pgx_handle* h, int nu);
PgxTicket ticket_publish(pgx_handle* h, unsigned long long* seq, size_t hoff_r, const double* dsrc1 = nullptr, size_t n1 = 0,
                         size_t hoff1 = 0);

// A producer launch leaves rows of nb block partials; their sums come to dout[0 .. nrows) on the device and to h_small[hoff ..) on
// the host, and with them a copy of src1[0 .. n1) to h_small[hoff1 ..).  Three routes, chosen by read_back_route():
//   ticket  the producer's last block sums and publishes (PgxTicket).  A producer whose instantiation carries no second stage
//           answers false, and the launch below follows it
//   fused   the producer leaves its partials; second stage and publish are one launch behind it (reduce_fetch)
//   plain   the producer runs its own second stage; then the all-reduce of the sums over a sharded handle's ranks, the replicas'
//           agreement on agree[0 .. n_agree), and fetch_small.  The only route of sharded and replica handles and of the copy read-back
struct PgxReadBack {
  int nb;
  const double* partials;
  int nrows;
  double* dout;
  size_t hoff;
  const double* src1 = nullptr;
  size_t n1 = 0, hoff1 = 0;
  double* agree = nullptr;
  size_t n_agree = 0;
};
enum PgxRoute { PGX_RB_TICKET, PGX_RB_FUSED, PGX_RB_PLAIN };
struct PgxPending {  // a read-back between its two halves
  PgxRoute route;
  unsigned long long seq;
};
PgxRoute read_back_route(const pgx_handle* h);
int read_back_finish(pgx_handle* h, const PgxReadBack& rb, const PgxPending& p);  // blocks until the values stand in h_small
#pragma GCC visibility pop

// First half: the producer's launch, produce(PgxTicket* tk, double* dout) -> bool, with the ticket and the second stage its route asks for
template <class Producer>
static inline PgxPending read_back_start(pgx_handle* h, const PgxReadBack& rb, PgxRoute route, Producer&& produce) {
  PgxPending p{route, 0};
  if (route == PGX_RB_TICKET) {
    const unsigned long long seq0 = h->seq;
    PgxTicket tk = ticket_publish(h, &p.seq, rb.hoff, rb.src1, rb.n1, rb.hoff1);
    if (!produce(&tk, rb.dout)) {  // an instantiation without the second stage: the launch of its own
      h->seq = seq0;
      p.route = PGX_RB_FUSED;
    }
  } else {
    produce(nullptr, route == PGX_RB_FUSED ? nullptr : rb.dout);
  }
  return p;
}
// Both halves.  The Newton step alone keeps them apart: its launch is enqueued ahead of the next residual, its sums are read behind it
template <class Producer>
static inline int read_back(pgx_handle* h, const PgxReadBack& rb, PgxRoute route, Producer&& produce) {
  return read_back_finish(h, rb, read_back_start(h, rb, route, produce));
}
