// Single-precision V-cycle legs for gfx950 (round 4).  Same algebra and the same row mapping as the fp64 kernels k_st_smoothR /
// k_st_resid_restrict_r of pgx_kernels.hip - a workgroup of 8 waves owns a 64-wide image, a wave owns image rows, interior tiles
// run without tests on scalar K / M stencils, boundary tiles (scheduled first) through the general per-point code - but on HALF
// the bytes: what the level-0 launches of the fp64 cycle wait for is the unique bytes of their coefficient and vector streams
// (cycle stamps + timing experiments), not instructions, LDS or occupancy.  Here
//   * D(psi) is ONE word per vertex (centre + the three forward links) - a float4, or by default (GridLevel::dbf16) two packed
//     bf16 pairs in 8 bytes, widened to float once per launch - instead of four 8-byte loads from four arrays; the three mirrored
//     links still come from the neighbours as floats (DPP lane shift, LDS row hand-over);
//   * the cycle's vectors are interleaved (u, psi) float2: one 8-byte load / store per vertex and vector;
//   * arithmetic in float: 20 registers of coefficients per image row instead of 36, LDS images of 8 B per vertex.
// 32 B (bf16 D; 40 B with the float4 form) per vertex and smoother launch instead of 84.  The V-cycle is a preconditioner inside FGMRES, which is flexible; the operator
// apply, the true residual that decides convergence and the Krylov space stay fp64, so the accuracy of the Newton steps is
// untouched (tools/mg32_study.py: identical Krylov counts with a float32 cycle on the numpy twin).
// The fp64 ends of the cycle: the first launch on the finest level reads the Krylov vector (fp64) and leaves its float2 copy for
// the launches that follow; the last launch writes the preconditioned vector as fp64; a level below the last single-precision
// one receives its right-hand side, and returns its correction, in fp64.
#include <algorithm>

#include "pgx_internal.h"
#include "pgx_stencil.h"

#define F32_BLOCK 512
// A/B switches of the interior tiles, both measured slower at 2049^2 and off: F32_WAVES_EU = 8 (a fourth workgroup per CU by a 64-VGPR
// cap: 12-28 B of scratch per lane, level-0 launches +20 %) and F32_LEAN (the 2x2 block inverse recomputed per sweep: +1 %).
// 32-row tiles (halo 1.31 instead of 1.52, but 94 VGPRs = two workgroups per CU) were +15 % and are not instantiated.  The fourth
// workgroup came without a cap: this file is compiled with -fno-slp-vectorize (csrc/Makefile), which leaves the level-0 interior
// tiles at 57 instead of 70 VGPRs - eight waves per SIMD - and the level-0 launches 15 % shorter.
#ifndef F32_LEAN
#define F32_LEAN 0
#endif
#ifndef F32_WAVES_EU
#define F32_WAVES_EU 2
#endif
// A/B switch of the six-sweep launches on tiles of 12 rows and more, measured slower at 2049^2 and off: F32_K6_SPLIT = 1 runs the
// boundary sub-tiles (78 VGPRs) as a launch of their own (k_f_smooth<..., PART = 2>) in front of the interior tiles (PART = 1: 56
// VGPRs = a fourth workgroup per CU at TY = 12, 67-70 at TY = 16 / 20).  The sub-tiles' launch takes 25-28 us when nothing runs
// beside it; merged, TY = 20 holds three workgroups per CU either way (LDS) and the solve is 2.5 ms shorter.
#ifndef F32_K6_SPLIT
#define F32_K6_SPLIT 0
#endif
#ifndef F32_K6_TY_TOP
#define F32_K6_TY_TOP 20  // tile rows of a six-sweep launch on levels above 513^2 (measured on 1025^2 and 2049^2: 12 / 16 / 20)
#endif
// A/B switch of the seven-neighbour LDS reads of an image (row sweeps, residual rows of the fused epilogue, restriction gathers):
// F32_LDS_SINGLE = 1 reads every float2 neighbour as ONE 8-byte ds_read_b64 that the compiler may not merge; 0 leaves the plain
// loads, which it merges in pairs into ds_read2_b64 - 8 LDS-array cycles per pair where two single reads take 2 + 2 (DESIGN.md
// section 5b).  The values loaded are the same; that the RESULTS are the same bit for bit is a property of the compiled code (which
// products the compiler contracts into FMAs), pinned by tests/test_gpu_mg32_lds_reads.py.
#ifndef F32_LDS_SINGLE
#define F32_LDS_SINGLE 1
#endif
#define F32_RR_CYB 2  // coarse rows of a boundary sub-tile of the residual + restriction
#define F32_TB 2  // rows of a boundary sub-tile of the smoother: image of 2 + 2K <= 8 rows, one per wave
// ... of a six-sweep launch without the fused restriction: 4.  Its image of TB + 12 rows takes two rows per wave either way (14
// rows fill 16 slots as badly as 16 do), so four-row sub-tiles are half as many workgroups of the same length.
__host__ __device__ constexpr int f32_tb(int K, int RR) { return (K == 6 && !RR) ? 4 : F32_TB; }

__device__ __forceinline__ float lane_shr1f(float x) {  // the value of lane - 1 (lane 0 keeps its own)
  int v = __float_as_int(x);
  v = __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);  // wave_shr:1
  return __int_as_float(v);
}

// One float2 of an LDS image as one 8-byte read of its own: volatile keeps the compiler from pairing it with a neighbour's; the
// pointer has to carry the LDS address space itself (a volatile load through the generic pointer is not inferred to LDS and
// becomes a flat load).
__device__ __forceinline__ float2 f_lds(const float2* p) {
  typedef const volatile __attribute__((address_space(3))) unsigned long long lds_u64;
  const unsigned long long w = *(lds_u64*)p;
  return make_float2(__uint_as_float((unsigned)w), __uint_as_float((unsigned)(w >> 32)));
}
#if F32_LDS_SINGLE
#define F_LD(src, i) f_lds(&src[i])
#else
#define F_LD(src, i) src[i]
#endif
// the seven neighbours of image vertex q (row length W) in stencil-slot order
#define F_LDS7(src, q, W, x0, x1, x2, x3, x4, x5, x6)                                                                              \
  const float2 x0 = F_LD(src, q), x1 = F_LD(src, (q) + 1), x2 = F_LD(src, (q) - 1), x3 = F_LD(src, (q) + W),                       \
               x4 = F_LD(src, (q) - W), x5 = F_LD(src, (q) + W + 1), x6 = F_LD(src, (q) - W - 1);

// The storage of D(psi) on a single-precision level is a template parameter DT of every reader: float4, or uint2 = two packed bf16
// pairs (x: D(0,0) low half, D(+1,0) high half; y: D(0,+1), D(+1,+1)).  Packing rounds to nearest even (v_cvt_pk_bf16_f32), so an
// exact zero stays an exact zero; unpacking is one shift or mask per value.  From f_unpack_d on the readers work on a float4.
// The packers (f_pack_bf16x2, f_pack_d, f_pack_dq) live in pgx_internal.h: the kernels that produce D(psi) store Dq themselves.
__device__ __forceinline__ float4 f_unpack_d(float4 q) { return q; }
__device__ __forceinline__ float4 f_unpack_d(uint2 w) {
  return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                     __uint_as_float(w.y & 0xffff0000u));
}
__device__ __forceinline__ void f_zero_d(float4& q) { q = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void f_zero_d(uint2& w) { w = make_uint2(0u, 0u); }

template <class DT>
__global__ void __launch_bounds__(256) k_f_pack_d(int n, const dsten_t* __restrict__ Dh, DT* __restrict__ Dq) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  f_pack_dq(Dh[v], Dh[(size_t)n + v], Dh[2 * (size_t)n + v], Dh[3 * (size_t)n + v], Dq[v]);
}
void pgxk_f_pack_d(hipStream_t st, const GridLevel& L) {
  if (L.dbf16)
    hipLaunchKernelGGL(k_f_pack_d<uint2>, dim3((L.n + 255) / 256), dim3(256), 0, st, L.n, L.Dh, (uint2*)L.Dq);
  else
    hipLaunchKernelGGL(k_f_pack_d<float4>, dim3((L.n + 255) / 256), dim3(256), 0, st, L.n, L.Dh, (float4*)L.Dq);
}

// ------------------------------------------------------------------------------------------------
// general per-point pieces (boundary tiles)
// ------------------------------------------------------------------------------------------------
struct FCoef {
  float kv[7], mv[7], dv[7];  // kv already holds alpha K
  int rowbc;
};
// uniform interior stencils as the kernels use them, converted once on the host (scalar registers: 22 instead of the 30 + conversions
// of the fp64 StConst): alpha K and M per slot (boundary tiles) and with the symmetric link pairs averaged (interior tiles)
struct FConst {
  float kc[7], mc[7];
  float k0, k1, k3, k5, m0, m1, m3, m5;
  int uniform;
};
static inline FConst make_fconst(const GridLevel& L, double alpha) {
  FConst c;
  for (int s = 0; s < 7; ++s) {
    c.kc[s] = (float)alpha * (float)L.Kc[s];
    c.mc[s] = (float)L.Mc[s];
  }
  const float a = (float)alpha;
  c.k0 = a * (float)L.Kc[0];
  c.k1 = a * (float)(0.5 * (L.Kc[1] + L.Kc[2]));
  c.k3 = a * (float)(0.5 * (L.Kc[3] + L.Kc[4]));
  c.k5 = a * (float)(0.5 * (L.Kc[5] + L.Kc[6]));
  c.m0 = (float)L.Mc[0];
  c.m1 = (float)(0.5 * (L.Mc[1] + L.Mc[2]));
  c.m3 = (float)(0.5 * (L.Mc[3] + L.Mc[4]));
  c.m5 = (float)(0.5 * (L.Mc[5] + L.Mc[6]));
  c.uniform = L.uniform;
  return c;
}
// Stencil slots: 0:(0,0) 1:(+1,0) 2:(-1,0) 3:(0,+1) 4:(0,-1) 5:(+1,+1) 6:(-1,-1).  Links that leave the grid hold 0 in K, M and Dq.
template <class DT>
__device__ __forceinline__ void f_load_coef(int v, int i, int j, int nx, int ny, int n, const double* __restrict__ K,
                                            const double* __restrict__ M, const DT* __restrict__ Dq, const FConst& sc,
                                            const uint8_t* __restrict__ mask, float alpha, FCoef& c) {
  const int sx = nx + 1;
  if (sc.uniform && i > 0 && i < nx && j > 0 && j < ny) {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      c.kv[s] = sc.kc[s];
      c.mv[s] = sc.mc[s];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      c.kv[s] = alpha * (float)K[(size_t)s * n + v];
      c.mv[s] = (float)M[(size_t)s * n + v];
    }
  }
  const float4 q = f_unpack_d(Dq[v]);
  c.dv[0] = q.x;
  c.dv[1] = q.y;
  c.dv[3] = q.z;
  c.dv[5] = q.w;
  c.dv[2] = (i > 0) ? f_unpack_d(Dq[v - 1]).y : 0.f;
  c.dv[4] = (j > 0) ? f_unpack_d(Dq[v - sx]).z : 0.f;
  c.dv[6] = (i > 0 && j > 0) ? f_unpack_d(Dq[v - sx - 1]).w : 0.f;
  c.rowbc = mask[v];
}

__device__ __forceinline__ void f_jacobi(const FCoef& c, float omega, float au, float ap, float xur, float xpr, float buv, float bpv,
                                         float& yu, float& yp) {
  if (c.rowbc) au = xur;
  const float su = buv - au, sp = bpv - ap;
  float a = c.kv[0], b = c.mv[0];
  const float dd = c.dv[0];
  float om_u = omega;
  if (c.rowbc) {  // Dirichlet row of u: solved exactly
    a = 1.f;
    b = 0.f;
    om_u = 1.f;
  }
  const float det = -a * dd - b * b;
  float du = 0.f, dpsi = 0.f;
  if (det != 0.f) {
    const float r = __builtin_amdgcn_rcpf(det);
    du = (-dd * su - b * sp) * r;
    dpsi = (-b * su + a * sp) * r;
  } else if (c.rowbc) {
    du = su;
  }
  yu = xur + om_u * du;
  yp = xpr + omega * dpsi;
}

// x + P x_c at fine vertex (gi, gj).  CADD: 0 = no correction, 1 = the coarse correction is float2 (cf), 2 = a pair of fp64 arrays
template <int CADD>
__device__ __forceinline__ float2 f_add_coarse(float2 x, int gi, int gj, int nxc, const float2* __restrict__ cf,
                                               const double* __restrict__ cdu, const double* __restrict__ cdp) {
  if (CADD == 0) return x;
  const int sxc = nxc + 1;
  const int jc = gj >> 1, ic = gi >> 1;
  const unsigned c0 = (unsigned)(jc * sxc + ic), c1 = (unsigned)((jc + (gj & 1)) * sxc + ic + (gi & 1));
  if (CADD == 1) {
    const float2 a = cf[c0], b = cf[c1];
    x.x += 0.5f * (a.x + b.x);
    x.y += 0.5f * (a.y + b.y);
  } else {
    x.x += 0.5f * (float)(cdu[c0] + cdu[c1]);
    x.y += 0.5f * (float)(cdp[c0] + cdp[c1]);
  }
  return x;
}

// ------------------------------------------------------------------------------------------------
// K sweeps per launch.  IO: 0 = float2 in and out; 1 = right-hand side from fp64 arrays, copied to bfo (FIRST launches only);
// 3 = the same from two float arrays (a vector of FGMRES's float basis: 8 instead of 16 bytes per vertex);
// 2 = result to fp64 arrays (launches with an iterate only).  CADD: the coarse correction added to the iterate (f_add_coarse).
// RR != 0: the launch ALSO restricts the residual of its result, b_c = P^T (b - J S^K(x)), to the coarse level (1: float2 cbf,
// 2: fp64 arrays) - the last pre-smoothing launch and the residual + restriction launch of a level in one: the image carries
// K + 2 halo rows / columns instead of K (K sweeps, one residual, one restriction stencil), the result is kept in LDS, the rows'
// coefficients are still in registers.  Saves a launch per level and cycle (what the small levels are made of) and one pass
// over D, b and x; costs (64 - 2K)(TY) / ((60 - 2K)(TY)) ... more halo work, so the finest level keeps the separate launches.
// ------------------------------------------------------------------------------------------------
struct FSmoothArgs {
  int nx, ny, n, nbnd, nxc, nyc, remap;
  RowmapGrid g;
  const double *K, *M;  // boundary rows only
  const void* Dq;  // DT of the kernel
  int dbf16;
  const uint8_t *mask, *mask_c;
  const float2 *xf, *cf, *bf;
  const double *cdu, *cdp, *b64u, *b64p;
  float2 *bfo, *yf, *cbf;
  double *y64u, *y64p, *cb64u, *cb64p;
  float alpha, omega;
  double bscale;  // IO == 1: the fp64 right-hand side is multiplied by this as it is read (lazily normalised Krylov vectors)
  FConst sc;
  const float *b32u, *b32p;  // IO == 3 (behind sc: the offsets the other instantiations read their arguments at stay put)
  int bfull;  // the nbnd boundary blocks are whole tiles (f_smooth_bnd_full), not sub-tiles
};

// the right-hand side at vertex v as the launch's IO reads it
template <int IO>
__device__ __forceinline__ float2 f_load_rhs(const FSmoothArgs& A, unsigned v) {
  if (IO == 1) return make_float2((float)(A.b64u[v] * A.bscale), (float)(A.b64p[v] * A.bscale));
  if (IO == 3) return make_float2((float)((double)A.b32u[v] * A.bscale), (float)((double)A.b32p[v] * A.bscale));
  return A.bf[v];
}

// HF = 1 ("halo rings saved"; FIRST launches only): the first sweep of a launch that starts from x = 0 reads no neighbour - it is
// the pointwise solve x_1 = omega B^-1 b - so x_1 is exact on the WHOLE image, sweep s is exact s - 1 rings in, and K sweeps
// need a halo of K - 1: sweep 1 runs on every image row and lane, sweep s >= 2 on rows / lanes [s - 1, . - (s - 1)).  The same
// image of 64 x 32 then owns 54 x 22 vertices instead of 52 x 20 (K = 6).  HF = 0 is every launch's code as it was.
template <class DT, int TY, int K, bool FIRST, int IO, int CADD, int RR, int HF = 0>
__device__ __forceinline__ void f_smooth_fast(int b, const FSmoothArgs& A, float2* img0, float2* img1, float2* exch) {
  constexpr int W = 64, HALO = K + (RR ? 2 : 0) - HF, TX = W - 2 * HALO, H0 = TY + 2 * HALO, NW = F32_BLOCK / 64, R = (H0 + NW - 1) / NW;
  static_assert(HF == 0 || (HF == 1 && FIRST && !RR && H0 % NW == 0), "a saved halo ring needs a launch that starts from x = 0");
  const int sx = A.nx + 1;
  const int tx = 1 + b % A.g.nfx, ty = 1 + b / A.g.nfx;
  const int i0 = tx * TX - HALO, j0 = ty * TY - HALO;  // origin of the image
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + lane;
  const bool own_lane = lane >= HALO && lane < W - HALO;
  const float k0 = A.sc.k0, k1 = A.sc.k1, k3 = A.sc.k3, k5 = A.sc.k5, m0 = A.sc.m0, m1 = A.sc.m1, m3 = A.sc.m3, m5 = A.sc.m5;
  // A wave owns the SAME image rows in every sweep (lj = wave + NW k): their D links and right-hand side are loaded once, all
  // loads in flight together, and stay in registers for the K sweeps.
  const DT* const Dq = static_cast<const DT*>(A.Dq);
  DT dw[R];
  float4 dq[R];
  float2 rb[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (HF || lj < H0 - 1) {  // rows 1 .. H0-2 are updated; row 0 only hands its upward links to row 1 (HF: sweep 1 updates every row)
      const unsigned v = (unsigned)((j0 + lj) * sx + gi);
      dw[k] = Dq[v];
      if (HF || lj >= 1) rb[k] = f_load_rhs<IO>(A, v);
    }
  }
  if (!FIRST) {
    float2 xa[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < H0) {
        const int gj = j0 + lj;
        xa[k] = f_add_coarse<CADD>(A.xf[(unsigned)(gj * sx + gi)], gi, gj, A.nxc, A.cf, A.cdu, A.cdp);
      }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < H0) img0[lj * W + lane] = xa[k];
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (HF || lj < H0 - 1) {
      dq[k] = f_unpack_d(dw[k]);  // once per launch, after the batch of loads
      exch[lj * W + lane] = make_float2(dq[k].z, dq[k].w);
    }
  }
  __syncthreads();
  // omega * inverse of the vertex block [[aK0, M0], [M0, -D0]] (det < 0: k0 > 0, d0 >= 0, m0 > 0): kept per row for the K sweeps,
  // or (LEAN: images of three rows per wave) recomputed in every sweep - nine registers less, which is what lets a fourth
  // workgroup live on the CU (64 VGPRs)
  constexpr bool LEAN = F32_LEAN && R >= 3 && !RR;
  const float nm2 = -m0 * m0, mo = -m0 * A.omega, ko = k0 * A.omega;
  float d2[R], d4[R], d6[R], g0[LEAN ? 1 : R], g1[LEAN ? 1 : R], g3[LEAN ? 1 : R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (HF) d2[k] = d4[k] = d6[k] = 0.f;  // rows 0 and H0-1 take sweep 1 only, which reads no link
    if (HF || (lj >= 1 && lj < H0 - 1)) {
      if (!HF || (lj >= 1 && lj < H0 - 1)) {
        d2[k] = lane_shr1f(dq[k].y);                   // D(+1,0) of the left neighbour
        d4[k] = exch[(lj - 1) * W + lane].x;           // D(0,+1) of the vertex below
        d6[k] = exch[(lj - 1) * W + lane - 1].y;       // D(+1,+1) of the vertex below left; lane 0 (halo, never updated) reads the guard band
      }
      if (!LEAN) {
        const float rc = __builtin_amdgcn_rcpf(fmaf(-k0, dq[k].x, nm2));
        g0[k] = -dq[k].x * A.omega * rc;
        g1[k] = mo * rc;
        g3[k] = ko * rc;
      }
      if ((IO == 1 || IO == 3) && lj >= HALO && lj < H0 - HALO && own_lane) A.bfo[(unsigned)((j0 + lj) * sx + gi)] = rb[k];
    }
  }
  // (au, ap) = the two rows of J at image vertex q of row slot k
#define F_ROWS(src, q, k, au, ap, x0)                                                                                              \
  F_LDS7(src, q, W, x0, x1_, x2_, x3_, x4_, x5_, x6_)                                                                              \
  const float u12_ = x1_.x + x2_.x, u34_ = x3_.x + x4_.x, u56_ = x5_.x + x6_.x;                                                    \
  const float p12_ = x1_.y + x2_.y, p34_ = x3_.y + x4_.y, p56_ = x5_.y + x6_.y;                                                    \
  au = (k0 * x0.x + k1 * u12_) + (k3 * u34_ + k5 * u56_) + ((m0 * x0.y + m1 * p12_) + (m3 * p34_ + m5 * p56_));                    \
  ap = ((m0 * x0.x + m1 * u12_) + (m3 * u34_ + m5 * u56_)) -                                                                       \
       (((dq[k].x * x0.y + dq[k].y * x1_.y) + (d2[k] * x2_.y + dq[k].z * x3_.y)) + ((d4[k] * x4_.y + dq[k].w * x5_.y) + d6[k] * x6_.y));
#pragma unroll
  for (int s = 1; s <= K; ++s) {
    const float2* const src = ((s - 1) & 1) ? img1 : img0;
    float2* const dst = (s & 1) ? img1 : img0;
    const bool act = lane >= s - HF && lane < W - (s - HF);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < s - HF || lj >= H0 - (s - HF)) continue;  // wave-uniform
      float au = 0.f, ap = 0.f, xur = 0.f, xpr = 0.f;
      if (!FIRST || s > 1) {
        F_ROWS(src, lj * W + lane, k, au, ap, x0)
        xur = x0.x;
        xpr = x0.y;
      }
      const float su = rb[k].x - au, sp = rb[k].y - ap;
      float ou, op;
      if (LEAN) {
        const float rc = __builtin_amdgcn_rcpf(fmaf(-k0, dq[k].x, nm2));
        ou = xur + fmaf(-dq[k].x * A.omega, su, mo * sp) * rc;
        op = xpr + fmaf(mo, su, ko * sp) * rc;
      } else {
        ou = xur + fmaf(g0[k], su, g1[k] * sp);
        op = xpr + fmaf(g1[k], su, g3[k] * sp);
      }
      if (act) {
        if (s == K && lj >= HALO && lj < H0 - HALO && own_lane) {
          const unsigned v = (unsigned)((j0 + lj) * sx + gi);
          if (IO == 2) {
            A.y64u[v] = (double)ou;
            A.y64p[v] = (double)op;
          } else {
            A.yf[v] = make_float2(ou, op);
          }
        }
        if (s < K || RR) dst[lj * W + lane] = make_float2(ou, op);
      }
    }
    if (s < K || RR) __syncthreads();
  }
  if (RR) {
    const float2* const xk = (K & 1) ? img1 : img0;  // S^K(x) on rows / lanes [K, . - K)
    float2* const rim = (K & 1) ? img0 : img1;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < K + 1 || lj >= H0 - K - 1) continue;  // wave-uniform
      float au, ap;
      F_ROWS(xk, lj * W + lane, k, au, ap, x0)
      if (lane >= K + 1 && lane < W - K - 1) rim[lj * W + lane] = make_float2(rb[k].x - au, rb[k].y - ap);
    }
    __syncthreads();
    // coarse vertex (I0 + ci, J0 + cj) = fine vertex at image row HALO + 2 cj, lane HALO + 2 ci
    const int sxc = A.nxc + 1, I0 = (tx * TX) >> 1, J0 = (ty * TY) >> 1;
    for (int cj = wave; cj < TY / 2; cj += NW)
      if (lane < TX / 2) {
        const int q = (HALO + 2 * cj) * W + HALO + 2 * lane;
        F_LDS7(rim, q, W, r0, r1, r2, r3, r4, r5, r6)
        const float su = r0.x + 0.5f * (((r1.x + r2.x) + (r3.x + r4.x)) + (r5.x + r6.x));
        const float sp = r0.y + 0.5f * (((r1.y + r2.y) + (r3.y + r4.y)) + (r5.y + r6.y));
        const int C = (J0 + cj) * sxc + I0 + lane;
        if (RR == 2) {
          A.cb64u[C] = (double)su;
          A.cb64p[C] = (double)sp;
        } else {
          A.cbf[C] = make_float2(su, sp);
        }
      }
  }
#undef F_ROWS
}

// Boundary tiles (tile index as in k_st_smoothR: row ty = 0 | rows 1..nfy: columns 0 and nfx+1.. | rows nfy+1..), cut into
// sub-tiles of TB rows.  Round 3's boundary path evaluated every vertex from scratch in every sweep - coefficient loads behind
// per-lane tests, a chain of dependent memory round trips of ~1 us per row iteration, and on the small levels that chain IS the
// launch time.  Here the boundary tiles are built like the interior ones: a wave owns image rows, EVERYTHING a row needs - its D
// links, right-hand side, iterate, Dirichlet flag and, for the vertices of the grid's frame only, the K / M rows from the arrays
// (every other vertex takes the uniform constants) - is loaded once, all loads in flight together, and stays in registers for the
// K sweeps; the mirrored D links come from the neighbours (out-of-grid entries are loaded as 0, and a link that leaves the grid is
// stored as 0, so no per-link test is left); the 2x2 vertex block is inverted once per launch.  With TB = 2 an image has
// 2 + 2K <= 8 rows: one row per wave (K <= 3); six sweeps take two rows per wave, and TB = 4 (f32_tb).
template <class DT, int TY, int TB, int K, bool FIRST, int IO, int CADD, int RR>
__device__ __forceinline__ void f_smooth_bnd(int b, const FSmoothArgs& A, float2* img0, float2* img1, float2* exch) {
  constexpr int W = 64, HALO = K + (RR ? 2 : 0), TX = W - 2 * HALO, H0 = TB + 2 * HALO, NSUB = TY / TB, NW = F32_BLOCK / 64,
                R = (H0 + NW - 1) / NW;
  static_assert(TY % TB == 0 && TB % 2 == 0, "sub-tiles must cover a tile and start on even rows");
  const int nx = A.nx, ny = A.ny, sx = nx + 1;
  const RowmapGrid& g = A.g;
  int tx, ty;
  const int sub = b % NSUB;
  b /= NSUB;
  const int side = g.ntx - g.nfx;  // boundary tiles in a row that also holds fast tiles
  if (b < g.ntx) {
    tx = b;
    ty = 0;
  } else if ((b -= g.ntx) < g.nfy * side) {
    ty = 1 + b / side;
    const int r = b % side;
    tx = r == 0 ? 0 : g.nfx + r;
  } else {
    b -= g.nfy * side;
    ty = g.nfy + 1 + b / g.ntx;
    tx = b % g.ntx;
  }
  const int i0 = tx * TX - HALO, j0 = ty * TY + sub * TB - HALO;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + lane;
  const bool own_lane = lane >= HALO && lane < W - HALO;
  const DT* const Dq = static_cast<const DT*>(A.Dq);
  DT dw[R];
  float4 dq[R];
  float2 rb[R], xa[R];
  float kv[R][7], mv[R][7];
  bool in[R], bc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k, gj = j0 + lj;
    in[k] = lj < H0 && gi >= 0 && gi <= nx && gj >= 0 && gj <= ny;
    bc[k] = false;
    f_zero_d(dw[k]);
    rb[k] = xa[k] = make_float2(0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      kv[k][t] = A.sc.kc[t];
      mv[k][t] = A.sc.mc[t];
    }
    if (in[k]) {
      const int v = gj * sx + gi;
      dw[k] = Dq[v];
      bc[k] = A.mask[v] != 0;
      if (lj >= 1 && lj < H0 - 1) rb[k] = f_load_rhs<IO>(A, (unsigned)v);
      if (!FIRST) xa[k] = f_add_coarse<CADD>(A.xf[v], gi, gj, A.nxc, A.cf, A.cdu, A.cdp);
      if (!(A.sc.uniform && gi > 0 && gi < nx && gj > 0 && gj < ny)) {  // the grid's frame (or a level without uniform stencils)
#pragma unroll
        for (int t = 0; t < 7; ++t) {
          kv[k][t] = A.alpha * (float)A.K[(size_t)t * A.n + v];
          mv[k][t] = (float)A.M[(size_t)t * A.n + v];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    dq[k] = f_unpack_d(dw[k]);
    if (lj < H0) {
      if (!FIRST) img0[lj * W + lane] = make_float2(bc[k] ? 0.f : xa[k].x, xa[k].y);  // pre-masked: Dirichlet u reads as 0
      exch[lj * W + lane] = make_float2(dq[k].z, dq[k].w);
    }
  }
  __syncthreads();
  float d2[R], d4[R], d6[R], g0[R], g1[R], g2[R], g3[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    d2[k] = d4[k] = d6[k] = g0[k] = g1[k] = g2[k] = g3[k] = 0.f;
    if (lj >= 1 && lj < H0 - 1) {
      d2[k] = lane_shr1f(dq[k].y);
      d4[k] = exch[(lj - 1) * W + lane].x;
      d6[k] = exch[(lj - 1) * W + lane - 1].y;
      // damped inverse of the vertex block, once per launch (f_jacobi: a Dirichlet row of u is solved exactly)
      float a = kv[k][0], bm = mv[k][0], om_u = A.omega;
      if (bc[k]) {
        a = 1.f;
        bm = 0.f;
        om_u = 1.f;
      }
      const float det = -a * dq[k].x - bm * bm;
      if (det != 0.f) {
        const float r = __builtin_amdgcn_rcpf(det);
        g0[k] = om_u * (-dq[k].x * r);
        g1[k] = om_u * (-bm * r);
        g2[k] = A.omega * (-bm * r);
        g3[k] = A.omega * (a * r);
      } else if (bc[k]) {
        g0[k] = 1.f;
      }
    }
  }
  // (au, ap) = the two rows of J at image vertex q of row slot k, per-lane K / M coefficients
#define F_ROWS_G(src, q, k, au, ap, x0)                                                                                            \
  F_LDS7(src, q, W, x0, x1_, x2_, x3_, x4_, x5_, x6_)                                                                              \
  au = ((kv[k][0] * x0.x + kv[k][1] * x1_.x) + (kv[k][2] * x2_.x + kv[k][3] * x3_.x)) +                                            \
       ((kv[k][4] * x4_.x + kv[k][5] * x5_.x) + kv[k][6] * x6_.x) +                                                                \
       (((mv[k][0] * x0.y + mv[k][1] * x1_.y) + (mv[k][2] * x2_.y + mv[k][3] * x3_.y)) +                                           \
        ((mv[k][4] * x4_.y + mv[k][5] * x5_.y) + mv[k][6] * x6_.y));                                                               \
  ap = (((mv[k][0] * x0.x + mv[k][1] * x1_.x) + (mv[k][2] * x2_.x + mv[k][3] * x3_.x)) +                                           \
        ((mv[k][4] * x4_.x + mv[k][5] * x5_.x) + mv[k][6] * x6_.x)) -                                                              \
       (((dq[k].x * x0.y + dq[k].y * x1_.y) + (d2[k] * x2_.y + dq[k].z * x3_.y)) + ((d4[k] * x4_.y + dq[k].w * x5_.y) + d6[k] * x6_.y));
#pragma unroll
  for (int s = 1; s <= K; ++s) {
    const float2* const src = ((s - 1) & 1) ? img1 : img0;
    float2* const dst = (s & 1) ? img1 : img0;
    const bool act = lane >= s && lane < W - s;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < s || lj >= H0 - s) continue;  // wave-uniform
      float au = 0.f, ap = 0.f, xur = 0.f, xpr = 0.f;
      if (!FIRST || s > 1) {
        F_ROWS_G(src, lj * W + lane, k, au, ap, x0)
        xur = x0.x;
        xpr = x0.y;
      }
      if (bc[k]) au = xur;  // (the image holds 0 there: the row reads u = b_u)
      const float su = rb[k].x - au, sp = rb[k].y - ap;
      const float ou = xur + fmaf(g0[k], su, g1[k] * sp);
      const float op = xpr + fmaf(g2[k], su, g3[k] * sp);
      if (act) {
        if (s == K && in[k] && lj >= HALO && lj < H0 - HALO && own_lane) {
          const int v = (j0 + lj) * sx + gi;
          if (IO == 1 || IO == 3) A.bfo[v] = rb[k];
          if (IO == 2) {
            A.y64u[v] = (double)ou;
            A.y64p[v] = (double)op;
          } else {
            A.yf[v] = make_float2(ou, op);
          }
        }
        if (s < K || RR) dst[lj * W + lane] = in[k] ? make_float2(bc[k] ? 0.f : ou, op) : make_float2(0.f, 0.f);
      }
    }
    if (s < K || RR) __syncthreads();
  }
  if (RR) {
    const float2* const xk = (K & 1) ? img1 : img0;
    float2* const rim = (K & 1) ? img0 : img1;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < K + 1 || lj >= H0 - K - 1) continue;  // wave-uniform
      float au, ap;
      F_ROWS_G(xk, lj * W + lane, k, au, ap, x0)
      // a Dirichlet row of u holds u = b_u after any sweep: its residual is 0 (the image keeps 0 there for the neighbours)
      if (lane >= K + 1 && lane < W - K - 1)
        rim[lj * W + lane] = in[k] ? make_float2(bc[k] ? 0.f : rb[k].x - au, rb[k].y - ap) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const int sxc = A.nxc + 1, I0 = (tx * TX) >> 1, J0 = (ty * TY + sub * TB) >> 1;
    for (int cj = wave; cj < TB / 2; cj += NW)
      if (lane < TX / 2 && I0 + lane <= A.nxc && J0 + cj <= A.nyc) {
        const int q = (HALO + 2 * cj) * W + HALO + 2 * lane;
        F_LDS7(rim, q, W, r0, r1, r2, r3, r4, r5, r6)
        float su = r0.x + 0.5f * (((r1.x + r2.x) + (r3.x + r4.x)) + (r5.x + r6.x));
        const float sp = r0.y + 0.5f * (((r1.y + r2.y) + (r3.y + r4.y)) + (r5.y + r6.y));
        const int C = (J0 + cj) * sxc + I0 + lane;
        if (A.mask_c[C]) su = 0.f;
        if (RR == 2) {
          A.cb64u[C] = (double)su;
          A.cb64p[C] = (double)sp;
        } else {
          A.cbf[C] = make_float2(su, sp);
        }
      }
  }
#undef F_ROWS_G
}

// Boundary tiles at the FULL tile height (FSmoothArgs::bfull: six-sweep launches, with or without the fused restriction, on a level
// with uniform stencils and no Dirichlet dof inside the grid): ONE workgroup per boundary tile with the interior tiles' image of
// TY + 2K rows and their rows per wave, instead of TY / 4 sub-tile workgroups that each sweep 16 image rows for 4.  Every in-grid
// vertex is updated by the interior tiles' pair-summed formula on scalar K / M; only the vertices of the grid's frame (gi in
// {0, nx}, gj in {0, ny}) have rows of their own, and those do NOT live in per-lane registers (R x 14 of them is what the sub-tile
// path pays): the alpha K / M rows of the image's frame vertices - at most two image rows and two image columns - are loaded with
// the launch's first batch, one or two values per thread, and staged in the third image, whose D links move to the second one,
// free until the first sweep writes it.  A frame vertex's row is then redone from LDS by the seven-slot formula of f_smooth_bnd:
// a frame row in a wave-uniform branch, a frame column in the one lane that holds it.  Out-of-grid entries and their D links are
// exact zeros, Dirichlet u reads as 0 and is solved exactly, as in f_smooth_bnd.
template <class DT, int TY, int K, bool FIRST, int IO, int CADD, int RR, int HF = 0>
__device__ __forceinline__ void f_smooth_bnd_full(int b, const FSmoothArgs& A, float2* img0, float2* img1, float2* exch) {
  constexpr int W = 64, HALO = K + (RR ? 2 : 0) - HF, TX = W - 2 * HALO, H0 = TY + 2 * HALO, NW = F32_BLOCK / 64, R = (H0 + NW - 1) / NW;
  // staged rows: slot s holds (aK[0..6], M[0..6]) as seven float2; slots [0, 2W): the frame rows gj = 0 and gj = ny by lane,
  // [2W, 2W + 2 H0): the frame columns gi = 0 and gi = nx by image row
  static_assert(7 * (2 * W + 2 * H0) <= H0 * W, "the frame rows' coefficients must fit into the third image");
  static_assert(14 * H0 <= F32_BLOCK && 14 <= 2 * NW, "one value of a frame column, two of a frame row per thread");
  static_assert(HF == 0 || (HF == 1 && FIRST && !RR && H0 % NW == 0), "a saved halo ring needs a launch that starts from x = 0");
  const int nx = A.nx, ny = A.ny, sx = nx + 1;
  const RowmapGrid& g = A.g;
  int tx, ty;
  const int side = g.ntx - g.nfx;  // boundary tiles in a row that also holds fast tiles
  if (b < g.ntx) {
    tx = b;
    ty = 0;
  } else if ((b -= g.ntx) < g.nfy * side) {
    ty = 1 + b / side;
    const int r = b % side;
    tx = r == 0 ? 0 : g.nfx + r;
  } else {
    b -= g.nfy * side;
    ty = g.nfy + 1 + b / g.ntx;
    tx = b % g.ntx;
  }
  const int i0 = tx * TX - HALO, j0 = ty * TY - HALO;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + lane;
  const bool own_lane = lane >= HALO && lane < W - HALO;
  const bool in_x = gi >= 0 && gi <= nx;
  const DT* const Dq = static_cast<const DT*>(A.Dq);
  float* const cst = reinterpret_cast<float*>(exch);
  DT dw[R];
  float4 dq[R];
  float2 rb[R], xa[R];
  bool in[R], bc[R], fr[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k, gj = j0 + lj;
    in[k] = lj < H0 && in_x && gj >= 0 && gj <= ny;
    fr[k] = in[k] && (gi == 0 || gi == nx || gj == 0 || gj == ny);
    bc[k] = false;
    f_zero_d(dw[k]);
    rb[k] = xa[k] = make_float2(0.f, 0.f);
    if (in[k]) {
      const int v = gj * sx + gi;
      dw[k] = Dq[v];
      bc[k] = A.mask[v] != 0;
      if (HF || (lj >= 1 && lj < H0 - 1)) rb[k] = f_load_rhs<IO>(A, (unsigned)v);
      if (!FIRST) xa[k] = f_add_coarse<CADD>(A.xf[v], gi, gj, A.nxc, A.cf, A.cdu, A.cdp);
    }
  }
  // the frame vertices' rows, in flight with the batch above: value t of a row is aK[t] (t < 7) or M[t - 7]
  double cv[6];
  int cq[6];  // where the value goes (in floats; -1: none)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int gj = r ? ny : 0;
    const bool has = gj >= j0 && gj < j0 + H0 && in_x;  // (ny >= 2: the two rows are different ones)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int t = wave + NW * hh, e = 2 * r + hh;
      cq[e] = -1;
      cv[e] = 0.0;
      if (has && t < 14) {
        cv[e] = (t < 7 ? A.K + (size_t)t * A.n : A.M + (size_t)(t - 7) * A.n)[(size_t)gj * sx + gi];
        cq[e] = 14 * (r * W + lane) + t;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int gic = c ? nx : 0, lj = (int)threadIdx.x / 14, t = (int)threadIdx.x % 14, gj = j0 + lj, e = 4 + c;
    cq[e] = -1;
    cv[e] = 0.0;
    if (gic >= i0 && gic < i0 + W && lj < H0 && gj >= 0 && gj <= ny) {
      cv[e] = (t < 7 ? A.K + (size_t)t * A.n : A.M + (size_t)(t - 7) * A.n)[(size_t)gj * sx + gic];
      cq[e] = 14 * (2 * W + c * H0 + lj) + t;
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    dq[k] = f_unpack_d(dw[k]);
    if (lj < H0) {
      if (!FIRST) img0[lj * W + lane] = make_float2(bc[k] ? 0.f : xa[k].x, xa[k].y);  // pre-masked: Dirichlet u reads as 0
      img1[lj * W + lane] = make_float2(dq[k].z, dq[k].w);
    }
  }
#pragma unroll
  for (int e = 0; e < 6; ++e)
    if (cq[e] >= 0) cst[cq[e]] = cq[e] % 14 < 7 ? A.alpha * (float)cv[e] : (float)cv[e];
  __syncthreads();
  // the staged row of image vertex (lj, lane), a frame vertex: a frame row takes precedence over a frame column (corners)
#define F_FRAME_ROW(lj) \
  (exch + 7 * ((j0 + (lj) == 0 || j0 + (lj) == ny) ? (j0 + (lj) == 0 ? 0 : W) + lane : 2 * W + (gi == 0 ? 0 : H0) + (lj)))
  float d2[R], d4[R], d6[R], g0[R], g1[R], g3[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    d2[k] = d4[k] = d6[k] = g0[k] = g1[k] = g3[k] = 0.f;
    if (HF || (lj >= 1 && lj < H0 - 1)) {  // (HF: rows 0 and H0-1 take sweep 1 only, which reads no link)
      if (!HF || (lj >= 1 && lj < H0 - 1)) {
        d2[k] = lane_shr1f(dq[k].y);
        d4[k] = img1[(lj - 1) * W + lane].x;
        d6[k] = img1[(lj - 1) * W + lane - 1].y;
      }
      // damped inverse of the vertex block, once per launch (f_jacobi: a Dirichlet row of u is solved exactly).  The psi row's
      // factor of su is g1 in either case: omega (-M0 / det) on a free row, 0 on a Dirichlet one
      float a = A.sc.kc[0], bm = A.sc.mc[0], om_u = A.omega;
      if (fr[k]) {
        const float2* const cf = F_FRAME_ROW(lj);
        a = cf[0].x;
        bm = cf[3].y;
      }
      if (bc[k]) {
        a = 1.f;
        bm = 0.f;
        om_u = 1.f;
      }
      const float det = -a * dq[k].x - bm * bm;
      if (det != 0.f) {
        const float r = __builtin_amdgcn_rcpf(det);
        g0[k] = om_u * (-dq[k].x * r);
        g1[k] = om_u * (-bm * r);
        g3[k] = A.omega * (a * r);
      } else if (bc[k]) {
        g0[k] = 1.f;
      }
    }
  }
  __syncthreads();  // every wave has taken its D links: the first sweep may write the second image
  const float k0 = A.sc.k0, k1 = A.sc.k1, k3 = A.sc.k3, k5 = A.sc.k5, m0 = A.sc.m0, m1 = A.sc.m1, m3 = A.sc.m3, m5 = A.sc.m5;
  // (au, ap) = the two rows of J at image vertex (lj, lane) of row slot k: the interior tiles' pair-summed formula, redone for a
  // frame vertex (a frame row: the whole wave; a frame column: one lane, every other wave skips the block) with its staged row -
  // F_ROWS_G's sums in four stages of two LDS reads: all fourteen coefficients in flight at once are what takes the kernel past 80
  // VGPRs, and only the frame's lanes wait here
  auto rows = [&](const float2* src, int lj, int k, float& au, float& ap) -> float2 {
    const int q = lj * W + lane;
    F_LDS7(src, q, W, x0, x1, x2, x3, x4, x5, x6)
    const float dp = ((dq[k].x * x0.y + dq[k].y * x1.y) + (d2[k] * x2.y + dq[k].z * x3.y)) +
                     ((d4[k] * x4.y + dq[k].w * x5.y) + d6[k] * x6.y);
    const float u12 = x1.x + x2.x, u34 = x3.x + x4.x, u56 = x5.x + x6.x;
    const float p12 = x1.y + x2.y, p34 = x3.y + x4.y, p56 = x5.y + x6.y;
    au = (k0 * x0.x + k1 * u12) + (k3 * u34 + k5 * u56) + ((m0 * x0.y + m1 * p12) + (m3 * p34 + m5 * p56));
    ap = ((m0 * x0.x + m1 * u12) + (m3 * u34 + m5 * u56)) - dp;
    if (fr[k]) {
      const float2* const cf = F_FRAME_ROW(lj);
      float2 ca = cf[0], cb = cf[1];
      const float ku = (ca.x * x0.x + ca.y * x1.x) + (cb.x * x2.x + cb.y * x3.x);
      __builtin_amdgcn_sched_barrier(0);
      ca = cf[2], cb = cf[3];
      au = ku + ((ca.x * x4.x + ca.y * x5.x) + cb.x * x6.x);
      const float mv0 = cb.y;
      __builtin_amdgcn_sched_barrier(0);
      ca = cf[4], cb = cf[5];
      const float mp = (mv0 * x0.y + ca.x * x1.y) + (ca.y * x2.y + cb.x * x3.y);
      const float mu = (mv0 * x0.x + ca.x * x1.x) + (ca.y * x2.x + cb.x * x3.x);
      const float mv4 = cb.y;
      __builtin_amdgcn_sched_barrier(0);
      ca = cf[6];
      au += mp + ((mv4 * x4.y + ca.x * x5.y) + ca.y * x6.y);
      ap = (mu + ((mv4 * x4.x + ca.x * x5.x) + ca.y * x6.x)) - dp;
    }
    return x0;
  };
#pragma unroll
  for (int s = 1; s <= K; ++s) {
    const float2* const src = ((s - 1) & 1) ? img1 : img0;
    float2* const dst = (s & 1) ? img1 : img0;
    const bool act = lane >= s - HF && lane < W - (s - HF);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < s - HF || lj >= H0 - (s - HF)) continue;  // wave-uniform
      float au = 0.f, ap = 0.f, xur = 0.f, xpr = 0.f;
      if (!FIRST || s > 1) {
        const float2 x0 = rows(src, lj, k, au, ap);
        xur = x0.x;
        xpr = x0.y;
      }
      if (bc[k]) au = xur;  // (the image holds 0 there: the row reads u = b_u)
      const float su = rb[k].x - au, sp = rb[k].y - ap;
      const float ou = xur + fmaf(g0[k], su, g1[k] * sp);
      const float op = xpr + fmaf(g1[k], su, g3[k] * sp);
      if (act) {
        if (s == K && in[k] && lj >= HALO && lj < H0 - HALO && own_lane) {
          const int v = (j0 + lj) * sx + gi;
          if (IO == 1 || IO == 3) A.bfo[v] = rb[k];
          if (IO == 2) {
            A.y64u[v] = (double)ou;
            A.y64p[v] = (double)op;
          } else {
            A.yf[v] = make_float2(ou, op);
          }
        }
        if (s < K || RR) dst[lj * W + lane] = in[k] ? make_float2(bc[k] ? 0.f : ou, op) : make_float2(0.f, 0.f);
      }
    }
    if (s < K || RR) __syncthreads();
  }
  if (RR) {  // residual of the result and its restriction, as in f_smooth_bnd, for the whole tile
    const float2* const xk = (K & 1) ? img1 : img0;
    float2* const rim = (K & 1) ? img0 : img1;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int lj = wave + NW * k;
      if (lj < K + 1 || lj >= H0 - K - 1) continue;  // wave-uniform
      float au, ap;
      rows(xk, lj, k, au, ap);
      // a Dirichlet row of u holds u = b_u after any sweep: its residual is 0 (the image keeps 0 there for the neighbours)
      if (lane >= K + 1 && lane < W - K - 1)
        rim[lj * W + lane] = in[k] ? make_float2(bc[k] ? 0.f : rb[k].x - au, rb[k].y - ap) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const int sxc = A.nxc + 1, I0 = (tx * TX) >> 1, J0 = (ty * TY) >> 1;
    for (int cj = wave; cj < TY / 2; cj += NW)
      if (lane < TX / 2 && I0 + lane <= A.nxc && J0 + cj <= A.nyc) {
        const int q = (HALO + 2 * cj) * W + HALO + 2 * lane;
        F_LDS7(rim, q, W, r0, r1, r2, r3, r4, r5, r6)
        float su = r0.x + 0.5f * (((r1.x + r2.x) + (r3.x + r4.x)) + (r5.x + r6.x));
        const float sp = r0.y + 0.5f * (((r1.y + r2.y) + (r3.y + r4.y)) + (r5.y + r6.y));
        const int C = (J0 + cj) * sxc + I0 + lane;
        if (A.mask_c[C]) su = 0.f;
        if (RR == 2) {
          A.cb64u[C] = (double)su;
          A.cb64p[C] = (double)sp;
        } else {
          A.cbf[C] = make_float2(su, sp);
        }
      }
  }
#undef F_FRAME_ROW
}

// ONE launch per smoother call (PART = 0): blocks [0, nbnd) are the boundary sub-tiles (A.bfull: whole boundary tiles) - they start first, so their long
// dependent-load chains overlap with the interior tiles that follow - blocks [nbnd, nbnd + nfast) the interior tiles.  PART = 1 /
// 2: the interior tiles / the boundary sub-tiles alone (F32_K6_SPLIT); both read the old iterate and write disjoint vertices of
// the new one, so the order of the two launches is free.
// HF = 1 (f_smooth_fast): a first launch with a halo of K - 1; its boundary blocks are always whole tiles.
template <class DT, int TY, int K, bool FIRST, int IO, int CADD, int RR, int PART = 0, int HF = 0>
__global__ void __launch_bounds__(F32_BLOCK, RR ? 2 : F32_WAVES_EU) k_f_smooth(const FSmoothArgs A) {
  constexpr int W = 64, H0 = (PART == 2 ? f32_tb(K, RR) : TY) + 2 * (K + (RR ? 2 : 0) - HF), PAD = W + 1;
  __shared__ float2 img_[3][H0 * W + 2 * PAD];  // guard bands: inactive edge lanes read (and discard) one entry outside a row;
                                                 // [2]: the (D(0,+1), D(+1,+1)) links every image row hands to the row above it
  const int blk = blockIdx.x;
  if constexpr (HF != 0) {
    static_assert(PART == 0 && K == 6, "the halo-saving form is a merged six-sweep launch");
    if (blk < A.nbnd)
      f_smooth_bnd_full<DT, TY, K, FIRST, IO, CADD, RR, HF>(blk, A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
    else
      f_smooth_fast<DT, TY, K, FIRST, IO, CADD, RR, HF>(xcd_block(blk - A.nbnd, gridDim.x - A.nbnd, A.remap), A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
  } else {
    if constexpr (PART == 0 && K == 6) {
      if (A.bfull && blk < A.nbnd) {
        f_smooth_bnd_full<DT, TY, K, FIRST, IO, CADD, RR>(blk, A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
        return;
      }
    }
    if (PART == 2 || (PART == 0 && blk < A.nbnd))
      f_smooth_bnd<DT, TY, f32_tb(K, RR), K, FIRST, IO, CADD, RR>(blk, A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
    else if (PART == 1)
      f_smooth_fast<DT, TY, K, FIRST, IO, CADD, RR>(xcd_block(blk, gridDim.x, A.remap), A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
    else
      f_smooth_fast<DT, TY, K, FIRST, IO, CADD, RR>(xcd_block(blk - A.nbnd, gridDim.x - A.nbnd, A.remap), A, img_[0] + PAD, img_[1] + PAD, img_[2] + PAD);
  }
}

// last pre-smoothing launch + residual + restriction (no coarse correction, float2 result); TY >= 8: the first interior tile's
// image (K + 2 halo rows) must start inside the grid
static bool f32_bnd_full(int n);
template <class DT, int TY, int K>
static void launch_f_smooth_rr_t(hipStream_t st, int first, FSmoothArgs& A, int fast_ok) {
  const int rr = A.cbf ? 1 : 2;
  A.g = rowmap_grid<TY, K + 2>(A.nx, A.ny, fast_ok);
  const int nfast = A.g.nfx * A.g.nfy;
  A.bfull = K == 6 && fast_ok && A.sc.uniform && f32_bnd_full(A.n);  // whole boundary tiles, as in launch_f_smooth_t
  A.nbnd = (A.g.ntx * A.g.nty - nfast) * (A.bfull ? 1 : TY / F32_TB);
  const dim3 grid(A.nbnd + nfast), block(F32_BLOCK);
  if (first) {
    if (A.b32u) {
      if (rr == 1)
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 3, 0, 1>), grid, block, 0, st, A);
      else
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 3, 0, 2>), grid, block, 0, st, A);
    } else if (A.b64u) {
      if (rr == 1)
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 1, 0, 1>), grid, block, 0, st, A);
      else
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 1, 0, 2>), grid, block, 0, st, A);
    } else {
      if (rr == 1)
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 0, 0, 1>), grid, block, 0, st, A);
      else
        hipLaunchKernelGGL((k_f_smooth<DT, TY, K, true, 0, 0, 2>), grid, block, 0, st, A);
    }
  } else {
    if (rr == 1)
      hipLaunchKernelGGL((k_f_smooth<DT, TY, K, false, 0, 0, 1>), grid, block, 0, st, A);
    else
      hipLaunchKernelGGL((k_f_smooth<DT, TY, K, false, 0, 0, 2>), grid, block, 0, st, A);
  }
}

template <int TY, int K>
static void launch_f_smooth_rr(hipStream_t st, int first, FSmoothArgs& A, int fast_ok) {
  if (A.dbf16)
    launch_f_smooth_rr_t<uint2, TY, K>(st, first, A, fast_ok);
  else
    launch_f_smooth_rr_t<float4, TY, K>(st, first, A, fast_ok);
}

template <class DT, int TY, int K, bool FIRST, int IO, int CADD>
static void launch_f_smooth_k(hipStream_t st, const FSmoothArgs& A, int nfast) {
  const dim3 block(F32_BLOCK);
  if constexpr (F32_K6_SPLIT && K == 6 && TY >= 12) {
    if (A.nbnd) hipLaunchKernelGGL((k_f_smooth<DT, TY, K, FIRST, IO, CADD, 0, 2>), dim3(A.nbnd), block, 0, st, A);
    if (nfast) hipLaunchKernelGGL((k_f_smooth<DT, TY, K, FIRST, IO, CADD, 0, 1>), dim3(nfast), block, 0, st, A);
  } else {
    hipLaunchKernelGGL((k_f_smooth<DT, TY, K, FIRST, IO, CADD, 0>), dim3(A.nbnd + nfast), block, 0, st, A);
  }
}

// Whole boundary tiles on a level of n vertices?  PGX_F32_BND_FULL (A/B switch: 0 = sub-tiles in every launch) and
// PGX_F32_BND_FULL_MIN: from 513^2 up.  Below, a launch is one round of workgroups and as long as its longest one: a whole tile
// (three image rows per wave, the staged frame rows, one more barrier) took 9.7-10.8 us where four-row sub-tiles take 7.4-7.9 us
// (257^2, 129^2, 65^2 levels of the 2048^2 solve), against 13.5 -> 12.0 us on 513^2.
static bool f32_bnd_full(int n) {
  static PgxTuneInt t_full("PGX_F32_BND_FULL", 1), t_min("PGX_F32_BND_FULL_MIN", 100000);
  return t_full.get() != 0 && n >= t_min.get();
}

// The first launch of a leg with a halo of five instead of six (k_f_smooth<..., HF = 1>)?  It starts from x = 0, so its first
// sweep is exact on the whole image and the 64 x 32 image of the 20-row tiles owns 54 x 22 vertices: 14 % fewer workgroups on
// 2049^2 and 1025^2, and a six-sweep launch is as long as the number of images it sweeps.
// PGX_F32_FIRST_HALO (A/B switch: 0 = the 52 x 20 tiles in every launch) and PGX_F32_FIRST_HALO_MIN: from 1025^2 up - below, the
// launches are one round of workgroups.  pgxk_f_smooth adds the conditions of the launch.
static bool f32_first_halo(int n) {
  static PgxTuneInt t_on("PGX_F32_FIRST_HALO", 1), t_min("PGX_F32_FIRST_HALO_MIN", 1000000);
  return t_on.get() != 0 && n >= t_min.get();
}

// ... as 54 x 22 tiles in the image of the 20-row ones; whole boundary tiles only, the caller has checked their conditions
template <class DT>
static void launch_f_smooth_first5(hipStream_t st, FSmoothArgs& A) {
  A.g = rowmap_grid<22, 5>(A.nx, A.ny, 1);
  const int nfast = A.g.nfx * A.g.nfy;
  A.bfull = 1;
  A.nbnd = A.g.ntx * A.g.nty - nfast;
  const dim3 grid(A.nbnd + nfast), block(F32_BLOCK);
  if (A.b32u)
    hipLaunchKernelGGL((k_f_smooth<DT, 22, 6, true, 3, 0, 0, 0, 1>), grid, block, 0, st, A);
  else if (A.b64u)
    hipLaunchKernelGGL((k_f_smooth<DT, 22, 6, true, 1, 0, 0, 0, 1>), grid, block, 0, st, A);
  else
    hipLaunchKernelGGL((k_f_smooth<DT, 22, 6, true, 0, 0, 0, 0, 1>), grid, block, 0, st, A);
}

template <class DT, int TY, int K>
static void launch_f_smooth_t(hipStream_t st, int first, FSmoothArgs& A, int fast_ok) {
  A.g = rowmap_grid<TY, K>(A.nx, A.ny, fast_ok);
  const int nfast = A.g.nfx * A.g.nfy;
  // boundary tiles: whole (six sweeps, uniform stencils, no Dirichlet dof inside the grid, a level of 513^2 and more) or cut into
  // sub-tiles of f32_tb rows
  A.bfull = !F32_K6_SPLIT && K == 6 && fast_ok && A.sc.uniform && f32_bnd_full(A.n);
  A.nbnd = (A.g.ntx * A.g.nty - nfast) * (A.bfull ? 1 : TY / f32_tb(K, 0));
  if (first) {
    if (A.b32u)
      launch_f_smooth_k<DT, TY, K, true, 3, 0>(st, A, nfast);
    else if (A.b64u)
      launch_f_smooth_k<DT, TY, K, true, 1, 0>(st, A, nfast);
    else
      launch_f_smooth_k<DT, TY, K, true, 0, 0>(st, A, nfast);
    return;
  }
  const int cadd = A.cf ? 1 : (A.cdu ? 2 : 0);
  if (A.y64u) {
    if (cadd == 0)
      launch_f_smooth_k<DT, TY, K, false, 2, 0>(st, A, nfast);
    else if (cadd == 1)
      launch_f_smooth_k<DT, TY, K, false, 2, 1>(st, A, nfast);
    else
      launch_f_smooth_k<DT, TY, K, false, 2, 2>(st, A, nfast);
  } else {
    if (cadd == 0)
      launch_f_smooth_k<DT, TY, K, false, 0, 0>(st, A, nfast);
    else if (cadd == 1)
      launch_f_smooth_k<DT, TY, K, false, 0, 1>(st, A, nfast);
    else
      launch_f_smooth_k<DT, TY, K, false, 0, 2>(st, A, nfast);
  }
}

template <int TY, int K>
static void launch_f_smooth(hipStream_t st, int first, FSmoothArgs& A, int fast_ok) {
  if (A.dbf16)
    launch_f_smooth_t<uint2, TY, K>(st, first, A, fast_ok);
  else
    launch_f_smooth_t<float4, TY, K>(st, first, A, fast_ok);
}

// Tile rows of a launch of K sweeps.  PGX_F32_TY: 4, 8, 16 for every K; 12 and 20 exist for the six-sweep launches only (images of
// 24 and 32 rows: three and four per wave) - other launches take the next height below, and a six-sweep image needs TY >= 8.
static int f32_ty_key() {
  static PgxTuneInt t_ty("PGX_F32_TY", 0);
  return t_ty.get();
}
static int f32_tile_rows(const GridLevel& L, int K) {
  const int ty = f32_ty_key();
  if (K == 6) {
    if (ty == 8 || ty == 12 || ty == 16 || ty == 20) return ty;
    if (ty == 4) return 8;
    return L.n <= 300000 ? 8 : F32_K6_TY_TOP;  // 513^2 and below: launch-latency bound, 8 rows = most workgroups
  }
  if (ty == 4 || ty == 8 || ty == 16) return ty;
  if (ty == 12) return 8;
  if (ty == 20) return 16;
  return L.n >= 2000000 ? 16 : L.n >= 500000 ? 8 : 4;  // as k_st_smoothR (measured there per level size)
}

void pgxk_f_smooth(hipStream_t st, int K, int first, const GridLevel& L, double alpha, const float2* xf, const double* b64u,
                   const double* b64p, const GridLevel* C, const float2* cf, const double* cdu, const double* cdp, double omega,
                   int remap, float2* yf, double* y64u, double* y64p, float2* cbf, double* cb64u, double* cb64p, double bscale,
                   const float* b32u, const float* b32p) {
  FSmoothArgs A;
  A.bscale = bscale;
  A.bfull = 0;
  A.b32u = first ? b32u : nullptr;
  A.b32p = first ? b32p : nullptr;
  A.nyc = C ? C->ny : 0;
  A.mask_c = C ? C->mask : nullptr;
  A.cbf = cbf;
  A.cb64u = cb64u;
  A.cb64p = cb64p;
  A.nx = L.nx;
  A.ny = L.ny;
  A.n = L.n;
  A.nxc = C ? C->nx : 0;
  A.remap = remap;
  A.K = L.K;
  A.M = L.M;
  A.Dq = L.Dq;
  A.dbf16 = L.dbf16;
  A.mask = L.mask;
  A.xf = first ? nullptr : xf;
  A.cf = first ? nullptr : cf;
  A.cdu = first ? nullptr : cdu;
  A.cdp = first ? nullptr : cdp;
  A.b64u = first && !A.b32u ? b64u : nullptr;
  A.b64p = first && !A.b32u ? b64p : nullptr;
  A.bf = (A.b64u || A.b32u) ? nullptr : L.bf;
  A.bfo = (A.b64u || A.b32u) ? L.bf : nullptr;
  A.yf = yf;
  A.y64u = first ? nullptr : y64u;
  A.y64p = first ? nullptr : y64p;
  A.alpha = (float)alpha;
  A.omega = (float)omega;
  A.sc = make_fconst(L, alpha);
  const int ty = f32_tile_rows(L, K);
  if (K == 6) {  // a whole leg of six sweeps in ONE launch
    if (cbf || cb64u)
      launch_f_smooth_rr<16, 6>(st, first, A, L.interior_free && (!C || C->interior_free));
    else if (first && !F32_K6_SPLIT && L.interior_free && A.sc.uniform && f32_bnd_full(L.n) && (f32_ty_key() == 0 || f32_ty_key() == 20) &&
             f32_first_halo(L.n)) {  // the 54 x 22 tiles of a launch that starts from x = 0, in the image of the 20-row tiles
      if (A.dbf16)
        launch_f_smooth_first5<uint2>(st, A);
      else
        launch_f_smooth_first5<float4>(st, A);
    } else if (ty == 8)
      launch_f_smooth<8, 6>(st, first, A, L.interior_free);
    else if (ty == 12)
      launch_f_smooth<12, 6>(st, first, A, L.interior_free);
    else if (ty == 16)
      launch_f_smooth<16, 6>(st, first, A, L.interior_free);
    else
      launch_f_smooth<20, 6>(st, first, A, L.interior_free);
    return;
  }
  if (cbf || cb64u) {
    if (K == 3) {
      if (ty <= 8)
        launch_f_smooth_rr<8, 3>(st, first, A, L.interior_free && (!C || C->interior_free));
      else
        launch_f_smooth_rr<16, 3>(st, first, A, L.interior_free && (!C || C->interior_free));
    } else {
      if (ty <= 8)
        launch_f_smooth_rr<8, 2>(st, first, A, L.interior_free && (!C || C->interior_free));
      else
        launch_f_smooth_rr<16, 2>(st, first, A, L.interior_free && (!C || C->interior_free));
    }
    return;
  }
  if (K == 3) {
    if (ty == 4)
      launch_f_smooth<4, 3>(st, first, A, L.interior_free);
    else if (ty == 8)
      launch_f_smooth<8, 3>(st, first, A, L.interior_free);
    else
      launch_f_smooth<16, 3>(st, first, A, L.interior_free);
  } else {
    if (ty == 4)
      launch_f_smooth<4, 2>(st, first, A, L.interior_free);
    else if (ty == 8)
      launch_f_smooth<8, 2>(st, first, A, L.interior_free);
    else
      launch_f_smooth<16, 2>(st, first, A, L.interior_free);
  }
}

// ------------------------------------------------------------------------------------------------
// b_c = P^T (b - J x): a workgroup of 8 waves owns CX x CY = 30 x 8 coarse vertices.  (1) the iterate on the 63 x 19 fine
// footprint goes into an LDS image, a wave per row, together with the (D(0,+1), D(+1,+1)) links every row hands to the row above;
// (2) a wave per fine row evaluates the residual on 61 x 17 vertices into a second image; (3) wave w restricts coarse row w.
// ------------------------------------------------------------------------------------------------
struct FRrArgs {
  int nx, ny, n, nbnd, nxc, nyc, remap;
  RrGrid g;
  const double *K, *M;
  const void* Dq;  // DT of the kernel
  int dbf16;
  const uint8_t *mask, *mask_c;
  const float2 *xf, *bf;
  float2* cbf;
  double *cb64u, *cb64p;
  float alpha;
  FConst sc;
};

template <class DT, bool CB64>
__device__ __forceinline__ void f_rr_fast(int tx, int ty, const FRrArgs& A, float2* ximg, float2* rimg, float2* exch) {
  constexpr int W = 64, CX = 30, CY = 8, HX = 2 * CY + 3, HR = 2 * CY + 1, NW = F32_BLOCK / 64, R = (HX + NW - 1) / NW;
  const int sx = A.nx + 1, sxc = A.nxc + 1;
  const int I0 = tx * CX, J0 = ty * CY;
  const int i0 = 2 * I0 - 2, j0 = 2 * J0 - 2;  // origin of the x image; the residual image starts one row / column further in
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + lane;
  const bool act = lane >= 1 && lane < W - 1;
  // every global load of the wave's (up to three) rows in flight before the first LDS store
  const DT* const Dq = static_cast<const DT*>(A.Dq);
  float2 xa[R], rb[R];
  DT dw[R];
  float4 dq[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (lj < HX) {
      const unsigned v = (unsigned)((j0 + lj) * sx + gi);
      xa[k] = A.xf[v];
      if (lj <= HR) dw[k] = Dq[v];
      if (lj >= 1 && lj <= HR) rb[k] = A.bf[v];
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (lj < HX) ximg[lj * W + lane] = xa[k];
    if (lj <= HR) {
      dq[k] = f_unpack_d(dw[k]);
      exch[lj * W + lane] = make_float2(dq[k].z, dq[k].w);
    }
  }
  __syncthreads();
  const float k0 = A.sc.k0, k1 = A.sc.k1, k3 = A.sc.k3, k5 = A.sc.k5, m0 = A.sc.m0, m1 = A.sc.m1, m3 = A.sc.m3, m5 = A.sc.m5;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int lj = wave + NW * k;
    if (lj < 1 || lj > HR) continue;  // wave-uniform
    const float d2 = lane_shr1f(dq[k].y), d4 = exch[(lj - 1) * W + lane].x, d6 = exch[(lj - 1) * W + lane - 1].y;
    const int q = lj * W + lane;
    // plain (merged) reads in these rows and in those of f_rr_bnd: with f_lds the compiler contracts the products of this kernel's
    // rows into other FMA pairs and the residual changes in its last bits.  The gathers below are plain too:
    // single reads there made this kernel slower (1.7 us on level 0), so k_f_resid_restrict is as it was before F32_LDS_SINGLE
    const float2 x0 = ximg[q], x1 = ximg[q + 1], x2 = ximg[q - 1], x3 = ximg[q + W], x4 = ximg[q - W], x5 = ximg[q + W + 1],
                 x6 = ximg[q - W - 1];
    const float u12 = x1.x + x2.x, u34 = x3.x + x4.x, u56 = x5.x + x6.x;
    const float p12 = x1.y + x2.y, p34 = x3.y + x4.y, p56 = x5.y + x6.y;
    const float au = (k0 * x0.x + k1 * u12) + (k3 * u34 + k5 * u56) + ((m0 * x0.y + m1 * p12) + (m3 * p34 + m5 * p56));
    const float ap = ((m0 * x0.x + m1 * u12) + (m3 * u34 + m5 * u56)) -
                     (((dq[k].x * x0.y + dq[k].y * x1.y) + (d2 * x2.y + dq[k].z * x3.y)) + ((d4 * x4.y + dq[k].w * x5.y) + d6 * x6.y));
    if (act) rimg[(lj - 1) * W + lane] = make_float2(rb[k].x - au, rb[k].y - ap);
  }
  __syncthreads();
  // restriction: wave w -> coarse row J0 + w, lane -> coarse column I0 + lane.  Fine vertex (2I, 2J) sits at residual-image
  // row 2w + 1 (image rows start at fine row 2 J0 - 1) and column 2 lane + 2
  if (wave < CY && lane < CX) {
    const int q = (2 * wave + 1) * W + 2 * lane + 2;
    const float2 r0 = rimg[q], r1 = rimg[q + 1], r2 = rimg[q - 1], r3 = rimg[q + W], r4 = rimg[q - W], r5 = rimg[q + W + 1],
                 r6 = rimg[q - W - 1];
    const float su = r0.x + 0.5f * (((r1.x + r2.x) + (r3.x + r4.x)) + (r5.x + r6.x));
    const float sp = r0.y + 0.5f * (((r1.y + r2.y) + (r3.y + r4.y)) + (r5.y + r6.y));
    const int C = (J0 + wave) * sxc + I0 + lane;
    if (CB64) {
      A.cb64u[C] = (double)su;
      A.cb64p[C] = (double)sp;
    } else {
      A.cbf[C] = make_float2(su, sp);
    }
  }
}

// boundary tiles, cut into sub-tiles of CYB = 2 coarse rows (x image of 7 fine rows: one per wave), register-resident like the
// boundary tiles of the smoother (f_smooth_bnd): one batch of loads, no dependent chains
template <class DT, bool CB64>
__device__ __forceinline__ void f_rr_bnd(int tx, int ty, int sub, const FRrArgs& A, float2* ximg, float2* rimg, float2* exch) {
  constexpr int W = 64, CX = 30, CY = 8, CYB = F32_RR_CYB, HX = 2 * CYB + 3, HR = 2 * CYB + 1, NW = F32_BLOCK / 64;
  static_assert(HX <= NW && CY % CYB == 0, "one image row per wave");
  const int nx = A.nx, ny = A.ny, sx = nx + 1, sxc = A.nxc + 1;
  const int I0 = tx * CX, J0 = ty * CY + sub * CYB;
  const int i0 = 2 * I0 - 2, j0 = 2 * J0 - 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + lane, lj = wave, gj = j0 + lj;
  const bool in = lj < HX && gi >= 0 && gi <= nx && gj >= 0 && gj <= ny;
  const bool act = lane >= 1 && lane < W - 1;
  DT dw;
  f_zero_d(dw);
  float2 rb = make_float2(0.f, 0.f), xa = make_float2(0.f, 0.f);
  float kv[7], mv[7];
  bool bc = false;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    kv[t] = A.sc.kc[t];
    mv[t] = A.sc.mc[t];
  }
  if (in) {
    const int v = gj * sx + gi;
    xa = A.xf[v];
    bc = A.mask[v] != 0;
    if (lj <= HR) dw = static_cast<const DT*>(A.Dq)[v];
    if (lj >= 1 && lj <= HR) {
      rb = A.bf[v];
      if (!(A.sc.uniform && gi > 0 && gi < nx && gj > 0 && gj < ny)) {
#pragma unroll
        for (int t = 0; t < 7; ++t) {
          kv[t] = A.alpha * (float)A.K[(size_t)t * A.n + v];
          mv[t] = (float)A.M[(size_t)t * A.n + v];
        }
      }
    }
  }
  const float4 dq = f_unpack_d(dw);
  if (lj < HX) {
    ximg[lj * W + lane] = make_float2(bc ? 0.f : xa.x, xa.y);  // pre-masked image
    exch[lj * W + lane] = make_float2(dq.z, dq.w);
  }
  __syncthreads();
  if (lj >= 1 && lj <= HR) {
    const float d2 = lane_shr1f(dq.y), d4 = exch[(lj - 1) * W + lane].x, d6 = exch[(lj - 1) * W + lane - 1].y;
    const int q = lj * W + lane;
    const float2 x0 = ximg[q], x1 = ximg[q + 1], x2 = ximg[q - 1], x3 = ximg[q + W], x4 = ximg[q - W], x5 = ximg[q + W + 1],
                 x6 = ximg[q - W - 1];  // plain reads, as in f_rr_fast
    float au = ((kv[0] * x0.x + kv[1] * x1.x) + (kv[2] * x2.x + kv[3] * x3.x)) + ((kv[4] * x4.x + kv[5] * x5.x) + kv[6] * x6.x) +
               (((mv[0] * x0.y + mv[1] * x1.y) + (mv[2] * x2.y + mv[3] * x3.y)) + ((mv[4] * x4.y + mv[5] * x5.y) + mv[6] * x6.y));
    const float ap = (((mv[0] * x0.x + mv[1] * x1.x) + (mv[2] * x2.x + mv[3] * x3.x)) + ((mv[4] * x4.x + mv[5] * x5.x) + mv[6] * x6.x)) -
                     (((dq.x * x0.y + dq.y * x1.y) + (d2 * x2.y + dq.z * x3.y)) + ((d4 * x4.y + dq.w * x5.y) + d6 * x6.y));
    if (bc) au = xa.x;  // Dirichlet row of u: r_u = b_u - u (the unmasked iterate)
    if (act) rimg[(lj - 1) * W + lane] = in ? make_float2(rb.x - au, rb.y - ap) : make_float2(0.f, 0.f);  // out-of-grid fine vertices hold 0
  }
  __syncthreads();
  if (wave < CYB && lane < CX) {
    const int I = I0 + lane, J = J0 + wave;
    if (I <= A.nxc && J <= A.nyc) {
      const int q = (2 * wave + 1) * W + 2 * lane + 2;
      const float2 r0 = rimg[q], r1 = rimg[q + 1], r2 = rimg[q - 1], r3 = rimg[q + W], r4 = rimg[q - W], r5 = rimg[q + W + 1],
                   r6 = rimg[q - W - 1];
      float su = r0.x + 0.5f * (((r1.x + r2.x) + (r3.x + r4.x)) + (r5.x + r6.x));
      const float sp = r0.y + 0.5f * (((r1.y + r2.y) + (r3.y + r4.y)) + (r5.y + r6.y));
      const int C = J * sxc + I;
      if (A.mask_c[C]) su = 0.f;
      if (CB64) {
        A.cb64u[C] = (double)su;
        A.cb64p[C] = (double)sp;
      } else {
        A.cbf[C] = make_float2(su, sp);
      }
    }
  }
}

template <class DT, bool CB64>
__global__ void __launch_bounds__(F32_BLOCK) k_f_resid_restrict(const FRrArgs A) {
  constexpr int W = 64, CY = 8, HX = 2 * CY + 3, HR = 2 * CY + 1, PAD = W + 1;
  __shared__ float2 ximg_[HX * W + 2 * PAD], rimg_[HR * W + 2 * PAD], exch_[HX * W + 2 * PAD];
  int b = blockIdx.x;
  if (b < A.nbnd) {
    constexpr int NSUB = 8 / F32_RR_CYB;
    const int sub = b % NSUB;
    b /= NSUB;
    int tx, ty;
    const RrGrid& g = A.g;
    const int side = g.ntx - g.nfx;
    if (b < g.ntx) {
      tx = b;
      ty = 0;
    } else if ((b -= g.ntx) < g.nfy * side) {
      ty = 1 + b / side;
      const int r = b % side;
      tx = r == 0 ? 0 : g.nfx + r;
    } else {
      b -= g.nfy * side;
      ty = g.nfy + 1 + b / g.ntx;
      tx = b % g.ntx;
    }
    f_rr_bnd<DT, CB64>(tx, ty, sub, A, ximg_ + PAD, rimg_ + PAD, exch_ + PAD);
  } else {
    b = xcd_block(b - A.nbnd, gridDim.x - A.nbnd, A.remap);
    f_rr_fast<DT, CB64>(1 + b % A.g.nfx, 1 + b / A.g.nfx, A, ximg_ + PAD, rimg_ + PAD, exch_ + PAD);
  }
}

void pgxk_f_resid_restrict(hipStream_t st, const GridLevel& L, double alpha, const float2* xf, const GridLevel& C, int remap,
                           float2* cbf, double* cb64u, double* cb64p) {
  constexpr int CX = 30, CY = 8;
  FRrArgs A;
  A.nx = L.nx;
  A.ny = L.ny;
  A.n = L.n;
  A.nxc = C.nx;
  A.nyc = C.ny;
  A.remap = remap;
  A.K = L.K;
  A.M = L.M;
  A.Dq = L.Dq;
  A.dbf16 = L.dbf16;
  A.mask = L.mask;
  A.mask_c = C.mask;
  A.xf = xf;
  A.bf = L.bf;
  A.cbf = cbf;
  A.cb64u = cb64u;
  A.cb64p = cb64p;
  A.alpha = (float)alpha;
  A.sc = make_fconst(L, alpha);
  RrGrid& g = A.g;
  g.ntx = (C.nx + CX) / CX;
  g.nty = (C.ny + CY) / CY;
  // interior <=> every vertex of the x image is strictly inside the fine grid: 2 tx CX - 2 >= 1, 2 tx CX - 2 + 63 <= nx - 1,
  // 2 ty CY - 2 >= 1, 2 ty CY - 2 + (2 CY + 2) <= ny - 1
  g.nfx = (L.nx - 62) >= 2 * CX ? (L.nx - 62) / (2 * CX) : 0;
  g.nfy = (L.ny - 1 - 2 * CY) >= 2 * CY ? (L.ny - 1 - 2 * CY) / (2 * CY) : 0;
  g.nfx = std::min(g.nfx, g.ntx - 1);
  g.nfy = std::min(g.nfy, g.nty - 1);
  if (!L.interior_free || !C.interior_free || g.nfx <= 0 || g.nfy <= 0) g.nfx = g.nfy = 0;
  const int nfast = g.nfx * g.nfy;
  A.nbnd = (g.ntx * g.nty - nfast) * (CY / F32_RR_CYB);  // boundary tiles: sub-tiles of F32_RR_CYB coarse rows
  const dim3 grid(A.nbnd + nfast), block(F32_BLOCK);
  if (L.dbf16) {
    if (cb64u)
      hipLaunchKernelGGL((k_f_resid_restrict<uint2, true>), grid, block, 0, st, A);
    else
      hipLaunchKernelGGL((k_f_resid_restrict<uint2, false>), grid, block, 0, st, A);
  } else {
    if (cb64u)
      hipLaunchKernelGGL((k_f_resid_restrict<float4, true>), grid, block, 0, st, A);
    else
      hipLaunchKernelGGL((k_f_resid_restrict<float4, false>), grid, block, 0, st, A);
  }
}
