"""numpy twin of the P1 multigrid V-cycle (csrc/pgx_cycle.hip: vcycle, vcycle_f) on an nx x ny right-diagonal grid.  Test infrastructure:
the algebra of oracle/krylov_proto.py: CollectiveMG, stated for rectangles and built only from what the library exports (the scalar
blocks K, M, D of pgx_csr_export, alpha, the Dirichlet set):

  * P1 interpolation P between nested grids, Galerkin K, M, D = P^T . P per level (7-point stencils on every level);
  * the Dirichlet mask of a coarse level = the mask of the fine vertices it keeps (the frame, for the frame);
  * collective 2 x 2 damped Jacobi, omega_u = 1 on masked rows (they are solved exactly);
  * the restricted u-residual zeroed on coarse masked rows (they are no unknowns of the coarse problem);
  * `coarse_sweeps` sweeps from zero on the coarsest level; `nu_tail` (None: nu) sweeps per leg on the levels from `tail_start` on.

Two arithmetic modes (the float32 one follows tools/mg32_study.py: MG32):
  "f64"  float64 throughout;
  "f32"  on the levels of `f32_levels` the stencils, the vectors and the arithmetic are float32; the other levels stay float64 and the
         right-hand side / the correction are converted where two such levels meet.
In BOTH modes a level of `f32_levels` smooths and takes residuals with the STORED D of the device: pack_d (clamp at 1e30, bf16 round to
nearest even) of the float64 Galerkin stencil where `dbf16` is set, the clamped float cast where it is not.  The precision of the device's
arithmetic is then the only thing that separates a device cycle from the "f64" cycle, and |"f32" - "f64"| measures how much that is.

One term of the "f32" mode is stated the way the single-precision kernels evaluate it (`f32_dirichlet_product`, default on).  On a
Dirichlet row of u the 2 x 2 block is [[1, 0], [0, -d]] and every sweep of a launch finds 0 in the (pre-masked) image at that vertex, so
the kernels do not iterate x_u <- x_u + (b_u - x_u) there: each sweep stores x_u = g0 b_u with g0 = (-d) * (1 / (-d)), the first entry of
the damped block inverse they form once per launch from ONE reciprocal.  g0 is 1 to within two roundings, so x_u is b_u to about an ulp
where the iteration of MG32 reaches b_u exactly after its second sweep.  Both are legitimate single-precision evaluations of "solved
exactly"; without the option a right-hand side that is dominated by float-representable Dirichlet values (unit impulses at the corners,
handed over as floats) makes |"f32" - "f64"| collapse to the rounding of the small remainder while the device carries its ulp on the
dominating entries: measured on (200, 72), alpha = 100, float-pair input, corners: device 1.0e-7 of max |z_u| against E = 3.0e-9
(ratio 35 to 40 in every launch form, 1.06 with the same vector handed over in fp64)."""
import numpy as np
import scipy.sparse as sp

from oracle.krylov_proto import interp_matrix

D_CLAMP = np.float32(1e30)


def bf16_round(x):
    """float32 -> nearest bf16 value (ties to even) as float32: the bits v_cvt_pk_bf16_f32 stores, read back with `word << 16`."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def stored_d(x, dbf16):
    """What a single-precision level stores for the float64 D values x (GridLevel::Dq), as float32."""
    with np.errstate(over="ignore"):  # beyond the float range: infinity, which the clamp takes back
        f = np.minimum(np.asarray(x, dtype=np.float64).astype(np.float32), D_CLAMP)
    return bf16_round(f) if dbf16 else f


def frame_mask(nx, ny):
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    return ((i == 0) | (i == nx) | (j == 0) | (j == ny)).ravel()


def half_stencil(S, nx, ny):
    """[4, n] half-stored stencil of the symmetric 7-point matrix S in the slot order of GridLevel::Dh: (0,0) (+1,0) (0,+1) (+1,+1);
    links that leave the grid hold 0."""
    S = sp.csr_matrix(S)
    sx, n = nx + 1, (nx + 1) * (ny + 1)
    v = np.arange(n)
    i, j = v % sx, v // sx
    out = np.zeros((4, n))
    for s, (off, ok) in enumerate(((0, i >= 0), (1, i < nx), (sx, j < ny), (sx + 1, (i < nx) & (j < ny)))):
        out[s, ok] = np.asarray(S[v[ok], v[ok] + off]).ravel()
    return out


def coarse_shapes(nx, ny, min_nx=4):
    """Cells per side of every level: halved while both counts are even and above min_nx (csrc/pgx_setup.hip: build_multigrid)."""
    shapes = [(nx, ny)]
    while nx % 2 == 0 and ny % 2 == 0 and nx > min_nx and ny > min_nx:
        nx, ny = nx // 2, ny // 2
        shapes.append((nx, ny))
    return shapes


class VCycleReference:
    def __init__(self, K, M, D, alpha, nx, ny, isbc, n_levels=None, min_nx=4, coarse_sweeps=4, tail_start=None, nu_tail=None,
                 f32_levels=(), dbf16=True, f32_dirichlet_product=True):
        """K, M, D: scalar n x n blocks of the finest level (K, M unconstrained); isbc: its Dirichlet mask; n_levels: depth (None: as
        deep as min_nx allows).  The hierarchy is built once, in float64; vcycle() does not modify it."""
        shapes = coarse_shapes(nx, ny, min_nx)
        if n_levels is not None:
            assert 1 <= n_levels <= len(shapes), (n_levels, shapes)
            shapes = shapes[:n_levels]
        self.alpha, self.coarse_sweeps, self.tail_start, self.nu_tail = float(alpha), int(coarse_sweeps), tail_start, nu_tail
        self.f32_levels, self.dbf16, self.f32_dirichlet_product = frozenset(f32_levels), bool(dbf16), bool(f32_dirichlet_product)
        assert len(shapes) - 1 not in self.f32_levels or len(shapes) == 1, "the coarsest level never runs in single precision"
        self.levels = []
        K, M, D = sp.csr_matrix(K, dtype=np.float64), sp.csr_matrix(M, dtype=np.float64), sp.csr_matrix(D, dtype=np.float64)
        mask = np.asarray(isbc, dtype=bool).copy()
        for l, (lx, ly) in enumerate(shapes):
            assert K.shape == ((lx + 1) * (ly + 1),) * 2 and mask.shape == (K.shape[0],)
            L = dict(nx=lx, ny=ly, n=K.shape[0], mask=mask, K=K, M=M, D=D)
            if l in self.f32_levels:  # the stored D, widened: every entry of the symmetric matrix is one stored value
                Ds = D.copy()
                Ds.data = stored_d(D.data, self.dbf16).astype(np.float64)
                L["Ds"] = Ds
            L["op64"] = self._operator(L, L.get("Ds", D), np.float64)
            self.levels.append(L)
            if l + 1 < len(shapes):
                P = interp_matrix(lx, ly).tocsr()
                L["P"] = P
                L["PT"] = P.T.tocsr()
                K, M, D = (P.T @ K @ P).tocsr(), (P.T @ M @ P).tocsr(), (P.T @ D @ P).tocsr()
                cx = lx // 2
                I, J = np.meshgrid(np.arange(cx + 1), np.arange(ly // 2 + 1), indexing="xy")
                mask = mask[(2 * J * (lx + 1) + 2 * I).ravel()]

    def _operator(self, L, D, dtype):
        keep = (~L["mask"]).astype(np.float64)
        A = (sp.diags(keep) @ (self.alpha * L["K"]) @ sp.diags(keep) + sp.diags(1.0 - keep)).tocsr()
        B = (sp.diags(keep) @ L["M"]).tocsr()  # u rows x psi columns; psi rows x u columns is B^T
        A, B, BT, D = (X.astype(dtype) for X in (A, B, B.T.tocsr(), sp.csr_matrix(D)))
        a, b, d = A.diagonal(), B.diagonal(), D.diagonal()
        return dict(A=A, B=B, BT=BT, D=D, a=a, b=b, d=d, det=-(a * d) - b * b)

    def _op(self, l, f32):
        L = self.levels[l]
        if not f32:
            return L["op64"]
        if "op32" not in L:
            L["op32"] = self._operator(L, L["Ds"], np.float32)
            L["P32"], L["PT32"] = L["P"].astype(np.float32), L["PT"].astype(np.float32)
        return L["op32"]

    def operator(self, l=0):
        """The float64 saddle-point matrix [[A, B], [B^T, -D]] the cycle of level l smooths (masked; stored D on a float32 level)."""
        O = self.levels[l]["op64"]
        return sp.bmat([[O["A"], O["B"]], [O["BT"], -O["D"]]]).tocsr()

    @staticmethod
    def _apply(O, xu, xp):
        return O["A"] @ xu + O["B"] @ xp, O["BT"] @ xu - O["D"] @ xp

    def _smooth(self, O, mask, xu, xp, ru, rp, its, omega, f32):
        a, b, d, det = O["a"], O["b"], O["d"], O["det"]
        dt = np.float32 if f32 else np.float64
        om = dt(omega)
        om_u = np.where(mask, dt(1.0), om).astype(dt)
        ok = det != 0  # a masked row whose D underflowed: the device takes du = s_u, dpsi = 0 there
        with np.errstate(divide="ignore", invalid="ignore"):
            rc = np.where(ok, dt(1.0) / det, dt(0.0)).astype(dt)
        for _ in range(its):
            yu, yp = self._apply(O, xu, xp)
            su, s_p = ru - yu, rp - yp
            if f32:  # MG32: one reciprocal per vertex, then products
                du, dp = (-d * su - b * s_p) * rc, (-b * su + a * s_p) * rc
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    du, dp = np.where(ok, (-d * su - b * s_p) / det, 0.0), np.where(ok, (-b * su + a * s_p) / det, 0.0)
            du = np.where(~ok & mask, su, du)
            xu_new = xu + om_u * du
            if f32 and self.f32_dirichlet_product:  # Dirichlet rows as the kernels store them: g0 b_u, from 0 in every sweep
                xu_new = np.where(mask & ok, (-d * rc) * ru, xu_new)
            xu = xu_new
            xp = xp + om * dp
        assert xu.dtype == dt and xp.dtype == dt
        return xu, xp

    def _cycle(self, l, ru, rp, nu, omega, mode):
        L = self.levels[l]
        f32 = mode == "f32" and l in self.f32_levels
        dt = np.float32 if f32 else np.float64
        O = self._op(l, f32)
        ru, rp = ru.astype(dt), rp.astype(dt)
        xu, xp = np.zeros_like(ru), np.zeros_like(rp)
        if "P" not in L:
            its = self.coarse_sweeps if len(self.levels) > 1 else 2 * nu
            return self._smooth(O, L["mask"], xu, xp, ru, rp, its, omega, f32)
        nl = nu
        if self.nu_tail is not None and self.tail_start is not None and l >= self.tail_start:
            nl = min(nu, self.nu_tail)
        xu, xp = self._smooth(O, L["mask"], xu, xp, ru, rp, nl, omega, f32)
        yu, yp = self._apply(O, xu, xp)
        PT, P = (L["PT32"], L["P32"]) if f32 else (L["PT"], L["P"])
        keep_c = (~self.levels[l + 1]["mask"]).astype(dt)
        cu, cp = self._cycle(l + 1, keep_c * (PT @ (ru - yu)), PT @ (rp - yp), nu, omega, mode)
        xu, xp = xu + P @ cu.astype(dt), xp + P @ cp.astype(dt)
        return self._smooth(O, L["mask"], xu, xp, ru, rp, nl, omega, f32)

    def vcycle(self, b, level=0, nu=6, omega=0.75, mode="f64"):
        """z = one V(nu, nu) cycle for b = [u | psi] of `level`, entered there from a zero guess; float64 [u | psi] out."""
        assert mode in ("f64", "f32")
        n = self.levels[level]["n"]
        b = np.asarray(b, dtype=np.float64)
        assert b.shape == (2 * n,)
        zu, zp = self._cycle(level, b[:n], b[n:], int(nu), float(omega), mode)
        return np.concatenate([zu.astype(np.float64), zp.astype(np.float64)])
