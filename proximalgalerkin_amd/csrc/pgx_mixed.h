// pgx_mixed.h - what the mixed-matrix families share (examples 06 / 02 / 05 / 08 / 04: pgx_gc.hip, pgx_sg.hip, pgx_qvi.hip,
// pgx_ic.hip, pgx_mp.hip): the handle base with its mixed CSR Newton matrix on the device and state vectors, the allocation / error / timing
// helpers, and the prototypes of the shared driver in pgx_mixed.hip - fixed-shape reductions, the SNES-mirroring Newton drivers
// (newtonls with linesearch none / bt / l2), their linear solve = sparse LU (pgx_nd) + iterative refinement on the exact
// operator, and the C entry points every family forwards to.  The create paths share their steps too: the host pattern builders
// (pgx_pattern.h), the sparse-LU setup mx_lu_create, the pattern upload mx_upload_pattern and the one-off constant-block pass
// mx_scatter_once; the P1-triangle families share their device geometry and quadrature table (pgx_tri.h).  A family keeps only
// its assembly kernels, its block layout and destination tables, and the order of these steps in its create path.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pgx.h"
#include "../../include/pgx_nd.h"
#include "pgx_comm.h"
#include "pgx_pattern.h"
#include "pgx_scope.h"

struct MixedBase {
  explicit MixedBase(const char* api_) : api(api_) {}
  const char* api;  // the family's C prefix ("pgx_gc", ...): messages name its entry points
  int device = 0;
  hipStream_t st = nullptr;
  std::string err;
  int64_t ntot = 0, nnz = 0;
  double alpha = 1.0;  // the proximal parameter of the LVPP step (set_alpha), read by the family's assembly
  int32_t *rowptr = nullptr, *col = nullptr;  // mixed CSR pattern (device)
  double* Jv = nullptr;                        // values of the current Jacobian
  double *x = nullptr, *xk = nullptr, *F = nullptr, *dx = nullptr, *xw = nullptr, *rhs = nullptr, *r = nullptr, *z = nullptr;
  double *partials = nullptr, *d_out = nullptr;
  double* h_out = nullptr;  // pinned
  std::vector<int32_t> h_rowptr, h_col;
  pgx_nd* lu = nullptr;
  double* gm_V = nullptr;  // Krylov basis of the GMRES safeguard (allocated on first use)
  int gm_m = 0;
  // Lazy refactorisation (EXPERIMENT, off: PGX_LAZY_LU=1 enables): from the second Newton step of a solve on, the factorisation
  // of the EARLIER iterate first serves as preconditioner of GMRES on the current exact Jacobian; only if that does not reach
  // the linear tolerance within `lazy_budget` iterations is the matrix factorised again.  Measured (tools/lazy_lu_ab.py): it
  // NEVER pays on these problems - 0 of 36 stale attempts converged within 10 iterations on example 06 at 1024^2 (13.8 -> 16.8 s),
  // 0 of 3 on example 02 at 70^3: between two Newton iterates the latent block N(psi) / D(psi) moves by orders of magnitude
  // where the constraint switches, and the 1e-12 true-residual bar leaves a stale factorisation no room.
  // Symmetrisation for the sparse LU (round 5): rows >= lu_flip_from of the Newton matrix are NEGATED on the way into pgx_nd_factor and
  // the same rows of every right-hand side on the way into pgx_nd_solve - x = J^-1 b = (S J)^-1 (S b), S = diag(I, -I).  Example 02's
  // [[alpha A, M_G^T], [-M_G, D]] becomes the symmetric [[alpha A, M_G^T], [M_G, -D]], which the LU factorises at half the flops
  // (pgx_nd_set_symmetric).  -1: off.  The rows are the last ones of the CSR, so their values are one contiguous range.
  double refine_eta = 1.0e-16;  // stop refining at this normwise backward error: the unit roundoff (PGX_MX_REFINE_ETA; 0 = never stop on it)
  int64_t lu_flip_from = -1;
  double* lu_flip_buf = nullptr;
  int lazy_lu = 0, lazy_budget = 10;
  bool lu_factored = false, stale_failed = false;
  long lazy_hits = 0, lazy_misses = 0, lazy_its = 0;
  // distributed handles (one per GPU, replicated iterate, distributed LU): every scalar that steers control flow - norms,
  // dot products of the line search - is taken from rank 0, so that all ranks make the same collective calls even though
  // their redundantly assembled residuals differ in the last bits (atomics)
  pgx_comm* comm = nullptr;
  bool jac_valid = false;
  bool prof = false;
  double ms[6] = {0, 0, 0, 0, 0, 0};  // [0] residual [1] jacobian [2] LU factor [3] LU solves [4] spmv [5] Newton total
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void*> allocs;
  virtual void residual_dev(const double* xin, double* Fout) = 0;  // F(x) incl. the BC rows, asynchronous on st
  virtual void jacobian_dev(const double* xin) = 0;                // fills Jv at x
  // The linear-solve hook of the Newton drivers: factorise Jv, solve with the factorisation (device pointers, on st), the solver's error
  // text, and its release before the stream goes.  Default (pgx_mixed.hip): the sparse LU `lu` (pgx_nd) through the row flip
  // lu_flip_from.  pgx_ma and pgx_ek override it with the dense LU with partial pivoting (pgx_dn): their Newton matrices are not quasi-definite.
  virtual int lin_factor();
  virtual int lin_solve(const double* rhs, double* out);
  virtual const char* lin_error() const;
  virtual void lin_release() {}
  virtual ~MixedBase() {}
};

#define MXHIP(call)                                               \
  do {                                                            \
    hipError_t e_ = (call);                                       \
    if (e_ != hipSuccess) {                                       \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return PGX_EHIP;                                            \
    }                                                             \
  } while (0)

template <typename T>
static int mx_alloc(MixedBase* h, T** p, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
    h->err = "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes failed";
    return PGX_ENOMEM;
  }
  h->allocs.push_back(q);
  *p = (T*)q;
  return PGX_OK;
}
#define MXALLOC(p, count)                        \
  do {                                           \
    int rc_ = mx_alloc(h, &(p), (size_t)(count)); \
    if (rc_) return rc_;                         \
  } while (0)

struct MxTimer {
  MixedBase* h;
  int slot;
  MxTimer(MixedBase* h_, int s) : h(h_), slot(s) {
    static const char* const names[6] = {"pgx:residual", "pgx:jacobian", "pgx:lu_factor", "pgx:lu_solve", "pgx:spmv", "pgx:newton"};
    pgx_roctx(names[s < 0 || s > 5 ? 5 : s]);
    if (h->prof) hipEventRecord(h->e0, h->st);
  }
  ~MxTimer() {
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

#define MX_RED 512  // blocks of the fixed-shape two-stage reductions: a family's reduction kernel writes MX_RED partials

// family entry points: null handle -> PGX_EINVAL, then the handle's device is made current
#define MXNEED(h)              \
  if (!(h)) return PGX_EINVAL; \
  if (hipSetDevice((h)->device) != hipSuccess) return PGX_EHIP

// shared driver (pgx_mixed.hip); internal to libpgx.so, not exported
#pragma GCC visibility push(hidden)
void mx_par_for(int64_t n, const std::function<void(int64_t, int64_t)>& fn);  // host threads over [0, n) in chunks
int mx_alloc_state(MixedBase* h);  // state vectors, reduction scratch, events; the stream must exist
// The sparse LU of the pattern h->h_rowptr / h->h_col on the handle's stream (which must exist): nested dissection over n_nodes
// nodes with coordinates node_coords[n_nodes][dim], node_of_dof[ntot]; distributed over comm if given.  Sets h->lu, or h->err.
// Symmetry (pgx_nd_set_symmetric) and the row flip lu_flip_from are the family's, after the call.
int mx_lu_create(MixedBase* h, int32_t n_nodes, const int32_t* node_of_dof, int dim, const double* node_coords, pgx_comm* comm = nullptr);
int mx_upload_pattern(MixedBase* h);  // h->rowptr, h->col <- h->h_rowptr, h->h_col; h->Jv allocated [nnz], not cleared
// Constant blocks, once, deterministic: launch(stash) parks n_slots values per entity slot-major, table[slot * n_entities + entity]
// names their destinations among n_dest (< 0: dropped), dst receives the sums (accumulate: is added to).  The scatter table is
// temporary, and so is the stash unless the caller lends one.  Synchronises the stream.
int mx_scatter_once(MixedBase* h, const int32_t* table, int64_t n_slots, int64_t n_entities, int64_t n_dest, double* stash_or_null,
                    const std::function<void(double*)>& launch, double* dst, int accumulate);
int mx_in(MixedBase* h, double* dst, const double* src, int64_t len = 0);  // host -> device, len = 0: ntot
int mx_norm(MixedBase* h, const double* v, double* out, int64_t len = 0);   // 2-norm (rank 0's value on every rank)
void mx_axpby(MixedBase* h, double a, const double* x, double b, double* y, int64_t len = 0);  // y = a x + b y on the stream
// sqrt(max(sum of h->partials, 0)): the tail of the families' increment norms.  sync = false: no agreement on rank 0's value, i.e. no
// communication on a distributed handle (the diagnostics of pgx_sg.h, evaluated on the replicated iterate)
int mx_partials_sqrt(MixedBase* h, double* out, bool sync = true);
// the entry points of every family: pgx_xx_destroy, set/get_state, set/get_prev, advance_prev, set_alpha, residual,
// jacobian_fill, csr_export, spmv, newton_solve and profile
void mx_destroy(MixedBase* h);
int mx_set_state(MixedBase* h, const double* x);
int mx_get_state(MixedBase* h, double* x);
int mx_set_prev(MixedBase* h, const double* x);
int mx_get_prev(MixedBase* h, double* x);
int mx_advance_prev(MixedBase* h);
int mx_set_alpha(MixedBase* h, double a);
int mx_residual(MixedBase* h, const double* x, double* F, double* fnorm);
int mx_jacobian_fill(MixedBase* h, const double* x);
int mx_csr_export(MixedBase* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int mx_spmv(MixedBase* h, const double* x, double* y);
// opts->linesearch 1: bt of order 2; 3: bt of order 3 (cubic); 2: l2 if the family takes it (with_l2), else plain Newton like
// every other value
int mx_newton(MixedBase* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its, bool with_l2);
int mx_profile(MixedBase* h, int enable, double ms[6]);
// J dx = b with the factorisation lin_factor() left behind: sparse LU + iterative refinement on the exact operator Jv, GMRES
// safeguard (o: ksp_rtol, ksp_max_it, monitor).  nsolves counts LU solves, relres is the true relative residual.
int mx_linear_solve(MixedBase* h, const double* b, double* dx, const pgx_snes_opts* o, int* nsolves, double* relres);
int mx_absmax(MixedBase* h, const double* v, double* out, int64_t len = 0);  // inf-norm, +inf if an entry is not finite
int mx_partials_sum(MixedBase* h, const double* partials, double* out);      // sum of MX_RED partials of a family's reduction
// NLsolve's `newton` with LineSearches.BackTracking(c_1 = c1) (examples/05_obstacle_type_qvi/solver_comparison/*.jl): see
// pgx_mixed.hip.  reason: 1 ftol, 2 xtol, 0 max_it (not an error), -4 no finite trial; h->x is replaced in every case but -4.
int mx_newton_nls(MixedBase* h, double ftol, double xtol, int max_it, double c1, int monitor, int* reason, int* its, int* lin_its);
#pragma GCC visibility pop

// pgx_xx_create*: device check, a new H on `device`, the family's impl(h); on failure `last_err` (what pgx_xx_last_error(NULL)
// reports) takes the handle's message and the handle is destroyed.  `fn` names the create function in the device errors.
template <typename H, typename Impl>
int mx_create(const char* fn, std::string& last_err, int device, H** out, Impl&& impl) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    last_err = std::string(fn) + ": no usable GPU (there is no CPU fallback)";
    return PGX_ENODEV;
  }
  if (hipSetDevice(device) != hipSuccess) {
    last_err = "hipSetDevice failed";
    return PGX_EHIP;
  }
  H* h = new H();
  h->device = device;
  const int rc = impl(h);
  if (rc) {
    last_err = h->err;
    mx_destroy(h);
    return rc;
  }
  *out = h;
  return PGX_OK;
}
