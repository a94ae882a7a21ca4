// The Krylov driver of libpgx.so: how a reduced scalar reaches the host (one routine, three routes), the 2-norm, FGMRES on one basis
// type, and the test hook that runs those same pieces.  The operator is in pgx_api.hip, the preconditioner and the collectives in pgx_cycle.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "pgx_handle.h"

// ------------------------------------------------------------------------------------------------
// small device results -> host
// ------------------------------------------------------------------------------------------------
// Replicas of a distributed-LU handle (pgx_create_lu_dist) compute every steering scalar redundantly - norms, Gram-Schmidt
// coefficients, observables.  The kernels are deterministic, so the copies agree bitwise today; but a rank that ever took a
// different branch would issue different collectives and RCCL has no timeout.  So the few doubles that DECIDE control flow are
// always taken from rank 0 (one tiny all-reduce of "mine if rank 0 else zero"); only the O(n) residual comparison stays behind
// PGX_CHECK_REPLICAS.  No-op on ordinary and on sharded handles.
int replica_agree(pgx_handle* h, double* dev, size_t n) {
  if (!h->lu_comm || h->lu_comm->size == 1) return PGX_OK;
  if (h->lu_comm->rank != 0) HIPCHK(hipMemsetAsync(dev, 0, n * sizeof(double), h->st));
  const int rc = h->lu_comm->allreduce(h->st, dev, n);
  if (rc) h->err = "replica agreement: " + h->lu_comm->err;
  return rc;
}

// Small device results -> host WITHOUT a stream synchronisation.  A one-workgroup kernel at the end of the enqueued work stores the
// n doubles into pinned, mapped host memory with system-scope stores, fences, and publishes a sequence number; the host polls that
// word.  What used to cost a D2H copy command, a stream synchronisation and the driver's wake-up (15-25 us in which the GPU idles)
// costs the PCIe write and a cache miss.
__global__ void __launch_bounds__(64) k_publish(int n, const double* __restrict__ src, double* dst, int n2, const double* __restrict__ src2,
                                                double* dst2, unsigned long long seq, unsigned long long* seqp) {
  for (int i = threadIdx.x; i < n; i += 64) __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (int i = threadIdx.x; i < n2; i += 64) __hip_atomic_store(dst2 + i, src2[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();  // one wave: every lane's stores are ordered before lane 0's flag store below
  if (threadIdx.x == 0) __hip_atomic_store(seqp, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the bounded host poll on the sequence word
static int wait_published(pgx_handle* h, unsigned long long seq) {
  // Bounded wait: a collective or a kernel ahead of k_publish that never completes leaves hipStreamQuery at NotReady
  // for ever - after PGX_COMM_TIMEOUT seconds (default 120; the transports' own limit) the call fails with PGX_ECOMM / PGX_EHIP and
  // a message instead of spinning.  The poll backs off: a pause per probe, and after ~50 us without an answer a yield per batch of
  // probes, so that eight ranks plus the BLAS threads of an oversubscribed host do not starve each other.
  static const double limit_s = [] {
    const char* t = getenv("PGX_COMM_TIMEOUT");
    return t ? std::max(1.0, atof(t)) : 120.0;
  }();
  std::chrono::steady_clock::time_point t0;
  bool timed = false;
  for (unsigned long spins = 1;; ++spins) {
    if (__atomic_load_n(h->h_seq, __ATOMIC_ACQUIRE) == seq) return PGX_OK;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
    if (spins > 0x2000 && (spins & 0xff) == 0) std::this_thread::yield();
    if ((spins & 0x3fff) == 0) {  // a failed launch or a faulted kernel must not leave the host spinning
      if (!timed) {
        t0 = std::chrono::steady_clock::now();
        timed = true;
      } else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
        h->err = "fetch_small: the device did not publish within PGX_COMM_TIMEOUT (" + std::to_string((int)limit_s) +
                 " s): a kernel or a collective ahead of it on the stream does not complete" + (h->dist.on || h->lu_comm ? " (a peer rank is missing?)" : "");
        return (h->dist.on || h->lu_comm) ? PGX_ECOMM : PGX_EHIP;
      }
      const hipError_t e = hipStreamQuery(h->st);
      if (e == hipSuccess) {
        if (__atomic_load_n(h->h_seq, __ATOMIC_ACQUIRE) == seq) return PGX_OK;
        h->err = "fetch_small: the stream drained without publishing (launch failure)";
        return PGX_EHIP;
      }
      if (e != hipErrorNotReady) {
        h->err = std::string("fetch_small: ") + hipGetErrorString(e);
        return PGX_EHIP;
      }
    }
  }
}

// h_small[hoff .. hoff + n) <- dsrc[0 .. n) (and optionally a second range), blocking until the values have arrived
int fetch_small(pgx_handle* h, const double* dsrc, size_t n, size_t hoff, const double* dsrc2, size_t n2, size_t hoff2) {
  if (!h->host_poll) {
    HIPCHK(hipMemcpyAsync(h->h_small + hoff, dsrc, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
    if (n2) HIPCHK(hipMemcpyAsync(h->h_small + hoff2, dsrc2, sizeof(double) * n2, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return PGX_OK;
  }
  const unsigned long long seq = ++h->seq;
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, h->st, (int)n, dsrc, h->h_small_dev + hoff, (int)n2, dsrc2, h->h_small_dev + hoff2,
                     seq, h->h_seq_dev);
  return wait_published(h, seq);
}
// the second stage of a reduction and its read-back in one launch (pgxk_reduce_publish): rows of nb partials -> dout[0 .. nrows) on
// the device and h_small[hoff_r ..), and dsrc1[0 .. n1) -> h_small[hoff1 ..); blocks like fetch_small
static int reduce_fetch(pgx_handle* h, int nb, const double* partials, int nrows, double* dout, size_t hoff_r, const double* dsrc1 = nullptr,
                        size_t n1 = 0, size_t hoff1 = 0) {
  const unsigned long long seq = ++h->seq;
  pgxk_reduce_publish(h->st, nb, partials, nrows, dout, h->h_small_dev + hoff_r, (int)n1, dsrc1, h->h_small_dev + hoff1, seq, h->h_seq_dev);
  return wait_published(h, seq);
}
// a ticket whose reducer publishes what reduce_fetch(h, ., ., ., ., hoff_r, dsrc1, n1, hoff1) would; the caller waits for *seq
PgxTicket ticket_publish(pgx_handle* h, unsigned long long* seq, size_t hoff_r, const double* dsrc1, size_t n1, size_t hoff1) {
  PgxTicket t;
  t.ctr = h->d_ticket;
  t.hout = h->h_small_dev + hoff_r;
  t.n1 = (int)n1;
  t.src1 = dsrc1;
  t.dst1 = h->h_small_dev + hoff1;
  t.seq = *seq = ++h->seq;
  t.seqp = h->h_seq_dev;
  return t;
}
// a ticket whose reducer leaves its results on the device only
static PgxTicket ticket_device(pgx_handle* h) {
  PgxTicket t;
  t.ctr = h->d_ticket;
  return t;
}

// The route of a read-back (pgx_handle.h: PgxReadBack).  Sharded handles, replicas and the copy read-back keep the plain launches: an
// all-reduce or a copy sits between the stages there.
PgxRoute read_back_route(const pgx_handle* h) {
  if (!(h->fused_publish && h->host_poll && !h->dist.on && !h->lu_comm)) return PGX_RB_PLAIN;
  return h->ticket_reduce ? PGX_RB_TICKET : PGX_RB_FUSED;
}
int read_back_finish(pgx_handle* h, const PgxReadBack& rb, const PgxPending& p) {
  int rc;
  switch (p.route) {
    case PGX_RB_TICKET:
      // (a read-back that has come in since was published behind this one on the same stream: nothing to wait for, and the
      // sequence word no longer holds p.seq)
      return p.seq == h->seq ? wait_published(h, p.seq) : PGX_OK;
    case PGX_RB_FUSED:
      return reduce_fetch(h, rb.nb, rb.partials, rb.nrows, rb.dout, rb.hoff, rb.src1, rb.n1, rb.hoff1);
    default:
      if (h->dist.on && (rc = allreduce_dev(h, rb.dout, (size_t)rb.nrows))) return rc;
      if (rb.n_agree && (rc = replica_agree(h, rb.agree, rb.n_agree))) return rc;
      return rb.n1 ? fetch_small(h, rb.src1, rb.n1, rb.hoff1, rb.dout, (size_t)rb.nrows, rb.hoff) : fetch_small(h, rb.dout, (size_t)rb.nrows, rb.hoff);
  }
}

// 2-norm of a device vector.  Sharded handles pass OWNED-COMPACT vectors (len = 2 * own_cnt): the squared norms of
// the ranks are summed by one all-reduce before the square root.
int dev_norm(pgx_handle* h, const double* v, double* out, size_t len) {
  const size_t l = len ? len : 2 * (size_t)h->nd;
  const PgxReadBack rb{pgxk_multidot_blocks(l), h->partials, 1, h->d_small, 0, nullptr, 0, 0, h->d_small, 1};
  // (one vector: every instantiation of k_multidot carries the second stage)
  const int rc = read_back(h, rb, read_back_route(h),
                           [&](PgxTicket* tk, double* dout) { return pgxk_multidot(h->st, l, 1, v, 0, v, h->partials, dout, nullptr, 8, tk); });
  if (rc) return rc;
  *out = std::sqrt(h->h_small[0]);
  return PGX_OK;
}

// ------------------------------------------------------------------------------------------------
// FGMRES
// ------------------------------------------------------------------------------------------------
// FGMRES keeps its Z_j as float2 fields where they leave the single-precision cycle and the operator apply is the
// matrix-free stencil kernel: one predicate for the solver and for pgx_spmv_bench, which replays the solver's sequence
bool z_f32_active(const pgx_handle* h, int nu) {
  return h->z_f32 && !h->dist.on && !h->lu_active && h->degree == 1 && h->structured && !h->lev.empty() && h->lev[0].uniform &&
         h->spmv_stencil == 1 && f32_cycle_ok(h, 0, nu);
}

// Single handle on the matrix-free structured P1 operator (uniform level 0): where the lean driver passes apply - the operator kernel's
// residual mode (PGX_FUSED_RESID), the signed right-hand side without a -F copy or a zero fill (PGX_LEAN_RHS), the fused Newton update
// (PGX_FUSED_STEP).  Sharded, replicated-LU, P2 and general-mesh handles keep the plain sequence.
bool krylov_lean(const pgx_handle* h) {
  return !h->dist.on && !h->lu_comm && !h->lu_active && h->degree == 1 && h->structured && h->spmv_stencil == 1 && !h->lev.empty() &&
         h->lev[0].uniform;
}

namespace {
// The Krylov basis in the storage h->V: fp64 vectors at a stride of ld doubles, or float vectors in the same [u | psi] layout at a
// stride of ld floats (padded to 16 bytes; (m + 1) ld floats fit in the (restart + 1) len doubles of h->V).
// fp64: the new vector w = J z_j is written into slot nv, behind the nv vectors it is orthogonalised against, and projected in place.
// float: w is fp64 in the scratch h->w; dot products and projections are fp64 on the widened basis, and the last chunk of a
// projection stores (float) w' into slot nv and sums the squares of the ROUNDED vector.
struct Basis {
  pgx_handle* h;
  size_t len;  // entries per vector
  bool f32;
  size_t ld;
  Basis() = default;
  Basis(pgx_handle* h_, size_t len_, bool f32_) : h(h_), len(len_), f32(f32_), ld(f32_ ? (len_ + 3) & ~(size_t)3 : len_) {}
  double* v64(int slot) const { return h->V + (size_t)slot * ld; }
  float* v32(int slot) const { return reinterpret_cast<float*>(h->V) + (size_t)slot * ld; }
  double* fresh(int nv) const { return f32 ? h->w : v64(nv); }  // where w is written and read

  // slot <- scale * src
  void store(int slot, double scale, const double* src) const {
    if (f32)
      pgxk_scale_copy_f32(h->st, len, scale, src, v32(slot));
    else
      pgxk_scale_copy(h->st, len, scale, src, v64(slot));
  }
  // out[i] = scale_i (V_i . w), i < nv.  against_stored: w as slot nv holds it after a projection - (float) w', widened - not h->w
  bool dots(int nv, bool against_stored, double* out, const PgxDotScale* scale, PgxTicket* tk) const {
    if (f32)
      return pgxk_multidot_f32(h->st, len, nv, v32(0), ld, against_stored ? nullptr : h->w, against_stored ? v32(nv) : nullptr, h->partials, out,
                               scale, h->gs_wide, tk);
    return pgxk_multidot(h->st, len, nv, v64(0), ld, v64(nv), h->partials, out, scale, h->gs_wide, tk);
  }
  // w' = w - sum_i coef[i] V_i and |w'|^2 -> out[0] (block partials in h->partials).  from_stored (float only): the vector projected
  // is the stored one, which is re-rounded in the same launch
  bool project(int nv, const double* coef, bool from_stored, double* out, PgxTicket* tk) const {
    if (f32)
      return pgxk_multiaxpy_norm_f32(h->st, len, nv, v32(0), ld, coef, from_stored ? 1 : 0, h->w, v32(nv), h->partials, out, h->gs_wide, tk);
    return pgxk_multiaxpy_norm(h->st, len, nv, v64(0), ld, coef, v64(nv), h->partials, out, h->gs_wide, tk);
  }
};

// one fgmres call
struct Solve {
  pgx_handle* h;
  const pgx_snes_opts* o;
  const double* b;
  double* x;
  double bsign;
  // Sharded: the Krylov space lives on OWNED dofs (basis vectors V_j, b, residuals are owned-compact, length nk, so the
  // tuned vector kernels run unchanged and every dot product is "local partial + one all-reduce"); the operators work
  // on local vectors with ghost rows (Z_j, x), with a gather after every SpMV.
  bool dist;
  size_t n2, nk;
  double* wk;
  int m;
  bool lean, lazy, zf32;
  bool x_unset;  // lean: no zero fill - the first solution update starts its sums from 0.0 instead of reading zeros back, and x = 0 is
                 // written only on the ways out that leave no update behind
  Basis B;       // of the current cycle
  std::vector<double> H, cs, sn, g, y, sv;  // sv: s_i (lazy normalisation)
  PgxDotScale sc2;                          // s_i^2
  double bnorm, target, omega;
  int its = 0;
  double res;
  // cycle
  bool first_cycle = true;
  bool redo = false;  // the cycle about to start repeats one that the float-basis guard abandoned
  double beta = 0.0, prev_cycle_res, cycle_target = 0.0;
};
}  // namespace

// The first vector of a cycle: b / |b|, or the TRUE residual, which decides convergence (not the Arnoldi estimate).  *stop: no cycle
static int start_cycle(Solve& s, bool* stop) {
  pgx_handle* const h = s.h;
  const pgx_snes_opts* const o = s.o;
  *stop = true;
  if (s.first_cycle) {
    s.beta = s.bnorm;
    s.B.store(0, s.bsign * (1.0 / s.beta), s.b);  // (bsign = -1: bitwise (-b) / beta)
  } else {
    // r = bsign b - J x
    PhaseTimer t(h, 3);
    if (s.lean && h->fused_resid) {  // one pass: the operator kernel stores bsign b - J x
      pgxk_st_spmv(h->st, h->lev[0], h->alpha, s.x, s.x + h->nd, h->xcd_remap ? 1 : 0, h->w, h->w + h->nd, nullptr, s.b, s.b + h->nd, s.bsign);
    } else {
      spmv_dev(h, s.x, h->w);
      if (s.dist) gather_owned(h, h->w, s.wk);
      pgxk_scale_copy(h->st, s.nk, -1.0, s.wk, s.wk);
      pgxk_axpy(h->st, s.nk, s.bsign, s.b, s.wk);
    }
    const int rc = dev_norm(h, s.wk, &s.beta, s.nk);
    if (rc) return rc;
    s.res = s.beta;
    if (o->monitor > 1) printf("      ksp true residual after cycle: %.6e (rel %.3e)\n", s.beta, s.beta / s.bnorm);
    // (redo: the same residual as at the head of the abandoned cycle - x was not touched - which passed both tests then)
    if (!s.redo && s.beta <= s.target) return PGX_OK;
    // attainable-accuracy exit: a full restart cycle that gains < 10x once we are at LU-level residuals
    if (!s.redo && s.beta > 0.1 * s.prev_cycle_res && s.beta <= 1e-7 * s.bnorm) return PGX_OK;
    if (s.its >= o->ksp_max_it) return PGX_OK;
    s.prev_cycle_res = s.beta;
    s.B.store(0, 1.0 / s.beta, s.wk);
  }
  *stop = false;
  return PGX_OK;
}

// z_j = M^-1 v_j, w = J z_j
static int arnoldi_step(Solve& s, int j) {
  pgx_handle* const h = s.h;
  double* const zj = h->Z + (size_t)j * s.n2;
  float2* const Zf = reinterpret_cast<float2*>(h->Z);
  {
    PhaseTimer t(h, 4);
    h->rhs_scale = s.lazy ? s.sv[j] : 1.0;
    h->zf_out = s.zf32 ? Zf + (size_t)j * h->nd : nullptr;
    h->rhs_f32 = s.B.f32 ? s.B.v32(j) : nullptr;  // (the fp64 argument is then not read: the cycle's first launch takes the float pair)
    const int rc = precond(h, h->V + (size_t)j * s.nk, zj, s.o->mg_nu, s.omega);
    h->rhs_f32 = nullptr;
    h->zf_out = nullptr;
    h->rhs_scale = 1.0;
    if (rc) return rc;
  }
  PhaseTimer t(h, 3);
  double* const wn = s.B.fresh(j + 1);  // w = J z_j goes straight to where the basis wants it
  if (s.dist) {
    spmv_dev(h, zj, h->w);
    gather_owned(h, h->w, wn);
  } else if (s.zf32) {
    pgxk_st_spmv(h->st, h->lev[0], h->alpha, nullptr, nullptr, h->xcd_remap ? 1 : 0, wn, wn + h->nd, Zf + (size_t)j * h->nd);
  } else {
    spmv_dev(h, zj, wn);
  }
  return PGX_OK;
}

// CGS2 of w against V_0 .. V_j (classical Gram-Schmidt in two passes: one pass loses orthogonality on these ill-conditioned systems
// and the true residual stalls).  Fills column j of H above the subdiagonal and returns the norm hn of the new vector, which it leaves
// normalised (or with its scale in sv / sc2, lazy) in slot j + 1.  *fits = false: the new vector does not fit the float basis.
// Pass 1: h1 = V^T w, ONE batched dot kernel.  Pass 2: w' = w - V h1 and |w'|^2 in one sweep over the basis.  V^T w', the second
// projection, only where the test below asks for it; the norm of its result comes from Pythagoras (|w''|^2 = |w'|^2 - |h2|^2,
// cancellation-free because the second pass removes almost nothing), so no separate norm kernel.
// Sharded: each batch of partial dot products is completed by ONE packed all-reduce, enqueued on the stream.
static int orthogonalise(Solve& s, int j, double* hn_out, bool* fits) {
  pgx_handle* const h = s.h;
  const Basis& B = s.B;
  const int m = s.m, nv = j + 1;
  int rc;
  PhaseTimer t(h, 5);
  double* const d_h1 = h->d_small;
  double* const d_h2 = h->d_small + (m + 2);
  const size_t off2 = (size_t)(m + 2);  // h_small: [h1 | h2, |w'|^2 at off2 + nv]
  const PgxDotScale* const dsc = s.lazy ? &s.sc2 : nullptr;
  const PgxRoute route = read_back_route(h);
  PgxTicket tkd = ticket_device(h);  // the dot products' second stage in the last block of their launch
  B.dots(nv, false, d_h1, dsc, route == PGX_RB_TICKET ? &tkd : nullptr);
  if (s.dist && (rc = allreduce_dev(h, d_h1, nv))) return rc;
  const PgxReadBack rb1{pgxk_stream_blocks(s.nk), h->partials, 1, d_h2 + nv, off2 + nv, d_h1, (size_t)nv, 0, h->d_small, 2 * off2};
  if ((rc = read_back(h, rb1, route, [&](PgxTicket* tk, double* out) { return B.project(nv, d_h1, false, out, tk); }))) return rc;
  double h1h1 = 0.0, hh = 0.0;
  for (int i = 0; i <= j; ++i) {
    h->h_small[i] /= s.sv[i];  // lazy: the device holds s_i^2 (W_i . w); the Hessenberg entry is s_i (W_i . w)
    h1h1 += h->h_small[i] * h->h_small[i];
  }
  const double wp2 = h->h_small[off2 + nv];
  // "twice is enough" (Kahan / Parlett; Daniel-Gragg-Kaufman-Stewart): the second projection is only needed when the
  // first one cancelled most of w, |w'| < eta |w| with |w|^2 = |w'|^2 + |h1|^2
  const bool second = wp2 < h->cgs_eta2 * (wp2 + h1h1);
  if (second) {
    PgxTicket tkd2 = ticket_device(h);
    B.dots(nv, true, d_h2, dsc, route == PGX_RB_TICKET ? &tkd2 : nullptr);
    if (s.dist && (rc = allreduce_dev(h, d_h2, nv))) return rc;
    if ((rc = replica_agree(h, d_h2, (size_t)nv))) return rc;
    if ((rc = fetch_small(h, d_h2, (size_t)nv, off2))) return rc;
    for (int i = 0; i <= j; ++i) h->h_small[off2 + i] /= s.sv[i];
  }
  for (int i = 0; i <= j; ++i) {
    const double h2 = second ? h->h_small[off2 + i] : 0.0;
    s.H[(size_t)i * m + j] = h->h_small[i] + h2;
    hh += h2 * h2;
  }
  double hn;
  if (second && B.f32) {
    // float basis: the stored vector, widened, is projected again and re-rounded in the same launch, which also sums the squares of
    // what it stores: hn is the norm of the vector kept (Pythagoras would describe the unrounded one).  One more small read-back,
    // on the rare path only.
    const PgxReadBack rb2{pgxk_stream_blocks(s.nk), h->partials, 1, d_h2 + nv, off2 + nv};
    if ((rc = read_back(h, rb2, route, [&](PgxTicket* tk, double* out) { return B.project(nv, d_h2, true, out, tk); }))) return rc;
    hn = std::sqrt(std::max(h->h_small[off2 + nv], 0.0));
  } else if (second) {
    hn = std::sqrt(std::max(wp2 - hh, 0.0));
    // last pass fused with the normalisation: v_{j+1} = (w' - V h2) / hn   (|w''|^2 = |w'|^2 - |h2|^2, Pythagoras)
    if (hn > 0.0) {
      if (s.lazy)
        pgxk_multiaxpy(h->st, s.nk, nv, B.v64(0), B.ld, d_h2, B.v64(nv));
      else
        pgxk_multiaxpy_scale(h->st, s.nk, nv, B.v64(0), B.ld, d_h2, 1.0 / hn, B.v64(nv));
    }
  } else {
    hn = std::sqrt(std::max(wp2, 0.0));
    if (hn > 0.0 && !s.lazy) pgxk_scale_copy(h->st, s.nk, 1.0 / hn, B.v64(nv), B.v64(nv));
    ++h->cgs_skipped;
  }
  ++h->cgs_total;
  *hn_out = hn;
  // Guard of the float basis: an overshot Newton iterate puts 1e300 into D(psi), and w = J z_j can then leave the float range.
  *fits = !(B.f32 && (!std::isfinite(hn) || hn > h->v_f32_max));
  if (*fits && s.lazy && hn > 0.0) {
    s.sv[j + 1] = 1.0 / hn;
    s.sc2.s[j + 1] = s.sv[j + 1] * s.sv[j + 1];
  }
  return PGX_OK;
}

// column j of H through the rotations so far, the new rotation, the estimate s.res = |g_{j+1}|
static void givens_update(Solve& s, int j, double hn) {
  const int m = s.m;
  std::vector<double>&H = s.H, &cs = s.cs, &sn = s.sn, &g = s.g;
  H[(size_t)(j + 1) * m + j] = hn;
  for (int i = 0; i < j; ++i) {
    const double t1 = cs[i] * H[(size_t)i * m + j] + sn[i] * H[(size_t)(i + 1) * m + j];
    H[(size_t)(i + 1) * m + j] = -sn[i] * H[(size_t)i * m + j] + cs[i] * H[(size_t)(i + 1) * m + j];
    H[(size_t)i * m + j] = t1;
  }
  const double a = H[(size_t)j * m + j], bb = H[(size_t)(j + 1) * m + j];
  const double rr = std::hypot(a, bb);
  cs[j] = rr == 0.0 ? 1.0 : a / rr;
  sn[j] = rr == 0.0 ? 0.0 : bb / rr;
  H[(size_t)j * m + j] = rr;
  H[(size_t)(j + 1) * m + j] = 0.0;
  g[j + 1] = -sn[j] * g[j];
  g[j] = cs[j] * g[j];
  s.res = std::fabs(g[j + 1]);
}

// y = H^-1 g (upper triangular, j columns), x += Z y
static int update_solution(Solve& s, int j) {
  pgx_handle* const h = s.h;
  const int m = s.m;
  std::vector<double>& y = s.y;
  for (int i = j - 1; i >= 0; --i) {
    double t = s.g[i];
    for (int k = i + 1; k < j; ++k) t -= s.H[(size_t)i * m + k] * y[k];
    y[i] = t / s.H[(size_t)i * m + i];
  }
  // y travels with the launch as an argument (at most PGX_DOT_SCALE_MAX coefficients; a longer basis - P2 - uploads it as before, and
  // h_small is then not touched again before that copy is done: the next read-back is ordered behind it on the stream)
  const double* const y_arg = j <= PGX_DOT_SCALE_MAX ? y.data() : nullptr;
  if (!y_arg) {
    for (int i = 0; i < j; ++i) h->h_small[i] = y[i];
    HIPCHK(hipMemcpyAsync(h->d_small, h->h_small, sizeof(double) * j, hipMemcpyHostToDevice, h->st));
  }
  if (s.zf32)
    pgxk_lincomb_f2(h->st, (size_t)h->nd, j, reinterpret_cast<float2*>(h->Z), (size_t)h->nd, h->d_small, s.x, s.x + h->nd, s.x_unset ? 0 : 1, y_arg);
  else
    pgxk_lincomb(h->st, s.n2, j, h->Z, s.n2, h->d_small, s.x, s.x_unset ? 0 : 1, y_arg);
  s.x_unset = false;
  // (no synchronisation: the head of the next cycle recomputes the TRUE residual b - Jx)
  return PGX_OK;
}

// FGMRES(restart) on J dx = b, right-preconditioned by one V-cycle; CGS2 orthogonalisation with
// batched device dot products; Givens rotations on the host (one small read-back per iteration).
// bnorm_known >= 0: the 2-norm of b, already on the host (the Newton driver's |F|: b = -F) - saves a reduction and its read-back
// bsign = +-1: the system solved is J dx = bsign * b (the Newton driver hands in F itself with bsign = -1 instead of a copy -F)
int fgmres(pgx_handle* h, const double* b, double* x, const pgx_snes_opts* o, int* its_out, double* relres, double bnorm_known, double bsign) {
  Solve s{h, o, b, x, bsign};
  s.dist = h->dist.on;
  s.n2 = 2 * (size_t)h->nd;
  s.nk = s.dist ? 2 * h->dist.nk_field() : s.n2;
  s.wk = s.dist ? h->dist.wc : h->w;
  // P2: the two-level preconditioner is weaker on the late large-alpha systems (30-60 its): use the full basis
  const int m = s.m = (h->degree == 2) ? h->restart : std::min(std::max(o->ksp_restart, 1), h->restart);
  s.H.assign((size_t)(m + 1) * m, 0.0);
  s.cs.resize(m);
  s.sn.resize(m);
  s.g.resize(m + 1);
  s.y.resize(m);
  s.sv.resize((size_t)m + 2);
  s.bnorm = bnorm_known;
  int rc = PGX_OK;
  if (!(bnorm_known >= 0.0) && (rc = dev_norm(h, b, &s.bnorm, s.nk))) return rc;
  const double bnorm = s.bnorm;
  s.lean = krylov_lean(h);
  s.x_unset = s.lean && h->lean_rhs;
  if (!s.x_unset) pgxk_set(h->st, s.n2, 0.0, x);
  *its_out = 0;
  *relres = 0.0;
  if (bnorm == 0.0 || !std::isfinite(bnorm)) {
    if (s.x_unset) pgxk_set(h->st, s.n2, 0.0, x);
    if (bnorm != 0.0) *relres = bnorm;
    return PGX_OK;
  }
  s.target = o->ksp_rtol * bnorm;
  s.res = s.prev_cycle_res = bnorm;
  // Smoother damping.  The default 0.8 is the fast choice while psi is smooth on the mesh scale (lambda_max of the
  // Jacobi-scaled element matrices is 2); an overshot Newton iterate makes exp(psi) jump by orders of magnitude
  // inside single elements, lambda_max approaches its bound 3 (dofs per triangle) and only omega < 2/3 is a
  // convergent smoother.  FGMRES tolerates a changing preconditioner, so on stagnation
  // the rest of this Newton solve runs at the unconditionally stable value.
  const double omega_safe = 0.6;
  s.omega = (h->omega_now > 0.0) ? std::min(h->omega_now, o->mg_omega) : o->mg_omega;
  // Lazy normalisation: a new basis vector stays as the Gram-Schmidt pass left it, W_{j+1} = w', and only its scale
  // s_{j+1} = 1 / |w'| is kept (v_i = s_i W_i): the V-cycle multiplies its right-hand side by s_j as its first launch reads it, the
  // batched dot products come back as s_i^2 (W_i . w) - the coefficients the projection w' = w - sum_i (v_i . w) v_i applies to the
  // stored W_i - and the pass over w that only divided it by its norm (67 MB read + written per iteration) is gone.  Only where
  // the preconditioner is the single-precision cycle entered on level 0 (it is the one that takes the factor).
  s.lazy = h->lazy_norm && !h->lu_active && h->degree == 1 && m + 2 <= PGX_DOT_SCALE_MAX && !h->lev.empty() && f32_cycle_ok(h, 0, o->mg_nu);
  // Z_j in single precision: on this path z_j leaves a float cycle, so storing it as one float2 field loses nothing - the
  // cycle's last launch writes it in place, the operator apply reads it (k_st_spmv_r<true>), the solution update sums it
  // (k_lincomb_f2): 100 MB less per Krylov iteration at 2048^2 than the fp64 pair.  w = J z_j and H stay fp64.
  s.zf32 = z_f32_active(h, o->mg_nu);
  // The basis in single precision (PGX_V_F32, the lean P1 path only, from PGX_V_F32_MIN vertices up; see Basis).  The Gram-Schmidt
  // passes move j + 3.5 instead of 2 j + 5 fp64 vectors.  The Arnoldi estimate of such a cycle stalls near 1e-7 of the residual the
  // cycle started from (the basis spans r / beta to float accuracy only), so a cycle ends once the estimate has gained v_f32_gain;
  // the next cycle then starts from the TRUE residual, taken in fp64.
  const bool vf32_ok = h->v_f32 && s.lean && s.lazy && s.zf32 && h->nd >= h->v_f32_min;
  while (true) {
    s.B = Basis(h, s.nk, vf32_ok && !h->v_f32_off);
    if (s.first_cycle && s.its >= o->ksp_max_it) break;
    bool stop;
    if ((rc = start_cycle(s, &stop))) return rc;
    if (stop) break;
    const double beta = s.beta;
    const bool was_first = s.first_cycle;
    s.first_cycle = false;
    s.redo = false;
    bool abandoned = false;
    double hn = 0.0;
    // float basis: the estimate is only trusted down to v_f32_gain times the residual this cycle started from
    s.cycle_target = s.B.f32 ? std::max(s.target, h->v_f32_gain * beta) : s.target;
    std::fill(s.g.begin(), s.g.end(), 0.0);
    s.g[0] = beta;
    std::fill(s.sv.begin(), s.sv.end(), 1.0);
    for (int i = 0; i < PGX_DOT_SCALE_MAX; ++i) s.sc2.s[i] = 1.0;
    int j = 0;
    for (; j < m && s.its < o->ksp_max_it; ++j) {
      if ((rc = arnoldi_step(s, j))) return rc;
      bool fits;
      if ((rc = orthogonalise(s, j, &hn, &fits))) return rc;
      if (!fits) {
        ++s.its;
        abandoned = true;
        break;
      }
      givens_update(s, j, hn);
      ++s.its;
      if (s.dist) ++h->dist.n_krylov;
      if (o->monitor > 1) printf("      ksp %3d  rnorm %.6e  rel %.3e\n", s.its, s.res, s.res / bnorm);
      if (!std::isfinite(s.res)) {
        if (s.x_unset) pgxk_set(h->st, s.n2, 0.0, x);
        *its_out = s.its;
        *relres = s.res / bnorm;
        return PGX_OK;
      }
      if (s.res <= s.cycle_target || hn == 0.0) {
        ++j;
        break;
      }
      // Stagnation test.  A healthy solve gains a factor 5-8 per iteration; a smoother that diverges on the rough late iterates
      // shows within a dozen iterations.  FGMRES tolerates a changing preconditioner, so the damping is switched IN PLACE (no
      // restart: the basis built so far stays useful) as soon as `stag_its` iterations have gained less than 1e-4.
      if (s.omega > omega_safe && j + 1 == std::min(m, h->stag_its) && s.res > h->stag_gain * beta) {
        h->omega_now = s.omega = omega_safe;  // sticky until pgx_newton_solve returns: later iterates are rough too
        if (o->monitor > 1) printf("      ksp stagnates: smoother damping -> %.2f for the rest of this Newton solve\n", s.omega);
      }
    }
    if (abandoned) {
      // A new vector whose norm is not finite (or above v_f32_max) ends the float basis for the rest of this Newton solve: this cycle is
      // abandoned - its columns are dropped, x is not updated, its iterations stay counted - and redone in fp64 from the same residual.
      h->v_f32_off = true;
      if (o->monitor > 1) printf("      ksp: basis vector outside the float range (norm %.3e): this cycle again, with the fp64 basis\n", hn);
      s.res = beta;
      s.first_cycle = was_first;  // the first cycle starts again from b (x is still unset with PGX_LEAN_RHS), a later one from b - J x
      s.redo = !was_first;
      continue;
    }
    if ((rc = update_solution(s, j))) return rc;
  }
  if (s.x_unset) pgxk_set(h->st, s.n2, 0.0, x);  // ksp_max_it == 0: no cycle ran
  *its_out = s.its;
  *relres = s.res / bnorm;
  return PGX_OK;
}

// Test hook (include/pgx.h): the two-launch route against the ticket route of the Gram-Schmidt reductions - the basis type's kernels
// through read_back, each route forced in turn - on data of its own in the handle's Krylov storage.  Reads no state of a solve and
// leaves none behind but scratch contents, and the sequence number.
extern "C" int pgx_reduce_selfcheck(pgx_handle* h, int nv, int64_t len, int basis_f32, int reps, uint64_t seed, int64_t* mismatches) {
  NEED(h);
  if (!mismatches) return PGX_EINVAL;
  const size_t n2 = 2 * (size_t)h->nd;
  if (h->dist.on || h->lu_comm || !h->host_poll) {
    h->err = "pgx_reduce_selfcheck: single handles with the polled read-back only";
    return PGX_EINVAL;
  }
  if (nv < 1 || nv > std::min(h->restart - 1, PGX_DOT_SCALE_MAX) || len < 2 || (len & 1) || (size_t)len > n2 || reps < 1) {
    h->err = "pgx_reduce_selfcheck: 1 <= nv <= min(restart - 1, " + std::to_string(PGX_DOT_SCALE_MAX) + "), len even, 2 <= len <= 2 nd, reps >= 1";
    return PGX_EINVAL;
  }
  const size_t l = (size_t)len;
  const Basis B(h, l, basis_f32 != 0);
  double* const w = B.fresh(nv);                      // the vector projected
  double* const wsave = h->Z;                         // ... as filled
  double* const wkeep = h->Z + n2;                    // w' of the two-launch route (float basis: slot nv, len / 2 words)
  const size_t wwords = basis_f32 ? l / 2 : l;        // 8-byte words of the stored w'
  double* const wres = basis_f32 ? reinterpret_cast<double*>(B.v32(nv)) : w;
  const int m2 = h->restart + 2;
  double* const d_a = h->d_small;                     // two-launch route: [h (nv); |w'|^2]
  double* const d_b = h->d_small + m2;                // ticket route
  std::vector<double> ha(nv + 1), hb(nv + 1), pa(nv + 1), pb(nv + 1), wa(wwords), wb(wwords);
  int64_t bad = 0;
  auto differ = [](const double* a, const double* b, size_t n) {
    int64_t d = 0;
    for (size_t i = 0; i < n; ++i) {
      uint64_t x, y;
      memcpy(&x, a + i, 8);
      memcpy(&y, b + i, 8);
      d += x != y;
    }
    return d;
  };
  // w' = w - V h (h: the two-launch route's dot products) and |w'|^2 -> dout[nv], read back with h on the given route
  auto project = [&](double* dout, PgxRoute route) {
    const PgxReadBack rb{pgxk_stream_blocks(l), h->partials, 1, dout + nv, (size_t)m2 + nv, d_a, (size_t)nv, 0};
    return read_back(h, rb, route, [&](PgxTicket* tk, double* out) { return B.project(nv, d_a, false, out, tk); });
  };
  for (int rep = 0; rep < reps; ++rep) {
    const unsigned long long sd = (unsigned long long)seed * 1000003ull + (unsigned long long)rep * 65ull;
    for (int i = 0; i < nv; ++i) {
      if (basis_f32)
        pgxk_fill_hash(h->st, l, sd + 1 + i, nullptr, B.v32(i));
      else
        pgxk_fill_hash(h->st, l, sd + 1 + i, B.v64(i), nullptr);
    }
    pgxk_fill_hash(h->st, l, sd, w, nullptr);
    pgxk_scale_copy(h->st, l, 1.0, w, wsave);
    PgxDotScale sc;
    for (int i = 0; i < PGX_DOT_SCALE_MAX; ++i) sc.s[i] = 1.0 + (double)((i * 7 + rep) % 13) / 16.0;
    const PgxDotScale* const scp = (rep & 1) ? &sc : nullptr;  // both second-stage kernels, k_reduce_partials and its scaled form
    // dot products: two launches, then the ticket
    HIPCHK(hipMemsetAsync(h->d_small, 0xff, sizeof(double) * 2 * (size_t)m2, h->st));
    B.dots(nv, false, d_a, scp, nullptr);
    PgxTicket tkd = ticket_device(h);
    B.dots(nv, false, d_b, scp, &tkd);  // (false: this instantiation keeps the second-stage launch and the two routes are one)
    // projection and norm, two launches: the partials, then k_reduce_publish
    int rc = project(d_a, PGX_RB_FUSED);
    if (rc) return rc;
    for (int i = 0; i < nv; ++i) pa[i] = h->h_small[i];
    pa[nv] = h->h_small[(size_t)m2 + nv];
    HIPCHK(hipMemcpyAsync(wa.data(), wres, sizeof(double) * wwords, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(ha.data(), d_a, sizeof(double) * (nv + 1), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    for (int i = 0; i <= nv; ++i) h->h_small[i] = h->h_small[(size_t)m2 + i] = 0.0;
    // the same inputs again, with the ticket
    pgxk_scale_copy(h->st, l, 1.0, wsave, w);
    HIPCHK(hipMemsetAsync(wkeep, 0, sizeof(double) * wwords, h->st));
    if (basis_f32) HIPCHK(hipMemsetAsync(B.v32(nv), 0, sizeof(float) * B.ld, h->st));
    if ((rc = project(d_b, PGX_RB_TICKET))) return rc;
    for (int i = 0; i < nv; ++i) pb[i] = h->h_small[i];
    pb[nv] = h->h_small[(size_t)m2 + nv];
    HIPCHK(hipMemcpyAsync(wb.data(), wres, sizeof(double) * wwords, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(hb.data(), d_b, sizeof(double) * (nv + 1), hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    bad += differ(ha.data(), hb.data(), (size_t)nv + 1);  // device results: the dot products and the norm
    bad += differ(pa.data(), pb.data(), (size_t)nv + 1);  // what the host was sent
    bad += differ(pa.data(), ha.data(), (size_t)nv + 1);  // ... is what the device holds
    bad += differ(wa.data(), wb.data(), wwords);          // the stored w'
  }
  HIPCHK(hipGetLastError());
  *mismatches = bad;
  return PGX_OK;
}
