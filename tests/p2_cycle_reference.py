"""numpy statement of the P2 two-level preconditioner (csrc/pgx_cycle.hip: pcycle_p2_patch; csrc/pgx_patch.hip).  Test infrastructure:
the algebra of oracle/p2_patch_proto.py, built only from what the library exports (the scalar blocks K, M, D of pgx_csr_export,
alpha, the Dirichlet set) plus the edges of the oracle's ObstacleLagrange:

  * the star table: per vertex the vertex dof, then the dofs of the edges that meet in it, -1 in unused slots (NN slots);
  * patch matrices [[aK, M], [M, -D]] on (u slots, psi slots) with identity rows and columns for Dirichlet u dofs and unused slots;
  * T, the P1 -> P2 interpolation of p1_to_p2;
  * one additive sweep x + omega W sum_p R_p^T Ainv_p R_p r: a vertex dof belongs to one patch and takes omega y, an edge dof to the
    patches a, b of its end vertices and takes omega 0.5 (y_a + y_b) - with y_a, y_b rounded to float32 where `stash_f32` is set,
    which is what the device parks between its two launches;
  * the residual b - J~ x of the masked saddle-point matrix, D rounded to float32 where `d_f32` is set (the float copy the cycle's
    residual kernels may read; they widen it and compute in float64);
  * the restriction T^T with the u rows of Dirichlet vertices zeroed; the prolongation x + T c;
  * the whole cycle: patch_nu sweeps from zero (the first on r = b) | restriction of the residual | one V-cycle of
    tests/vcycle_reference.py on K1 = T^T K T, M1 = T^T M T, D1 = T^T D T and the vertex mask | prolongation | patch_nu sweeps.

and a float64 twin of k_patch_invert's elimination (gauss_jordan_inverse), an mpmath inverse to compare inverses against
(exact_inverse, inverse_error), and the packing statements of the float and bf16 storage forms (sym_mirrored)."""
import numpy as np
import scipy.sparse as sp

from tests import vcycle_reference as VR

EPS = 2.0 ** -52


def p1_to_p2(edges, nv):
    """T [nv + ne, nv]: a hat function = the P2 vertex function + half of the functions of the edges that meet in the vertex."""
    edges = np.asarray(edges, dtype=np.int64)
    ne = len(edges)
    rows = np.concatenate([np.arange(nv), nv + np.arange(ne), nv + np.arange(ne)])
    cols = np.concatenate([np.arange(nv), edges[:, 0], edges[:, 1]])
    vals = np.concatenate([np.ones(nv), 0.5 * np.ones(ne), 0.5 * np.ones(ne)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(nv + ne, nv))


def star_table(edges, nv, NN=None):
    """[nv, NN] dofs of the scalar space per vertex star: slot 0 the vertex, then nv + e for the incident edges, -1 unused."""
    edges = np.asarray(edges, dtype=np.int64)
    inc = [[] for _ in range(nv)]
    for e, (a, b) in enumerate(edges):
        inc[a].append(nv + e)
        inc[b].append(nv + e)
    need = 1 + max(len(x) for x in inc)
    NN = need if NN is None else NN
    assert need <= NN, (need, NN)
    tab = np.full((nv, NN), -1, dtype=np.int64)
    for v in range(nv):
        tab[v, 0] = v
        tab[v, 1:1 + len(inc[v])] = inc[v]
    return tab


def patch_slots(NN):
    """The device's slot count for a mesh that needs NN slots: 7 up to vertex degree 6, 8 for degree 7."""
    return 7 if NN <= 7 else 8


def dict_values(v):
    """What build_km_dictionary (csrc/pgx_setup.hip) keeps of the entries v of K or M: each rounded to a grid of 2^-40 of the power of
    two at or below the largest |entry| (exact arithmetic, a function of the entry alone)."""
    v = np.asarray(v, dtype=np.float64)
    t = 2.0 ** (np.floor(np.log2(np.abs(v).max())) - 40)
    return np.rint(v / t) * t


def structured_interior_rows(nx, ny, i0, ni, j0, nj):
    """[n] bool: the dofs of the interior groups of the structured apply (csrc/pgx_p2st.hip) on the nx x ny right-diagonal mesh -
    vertex (i, j), i0 <= i < i0 + ni, j0 <= j < j0 + nj, and its three edges nv + j (3 nx + 1) + 3 i + {0, 1, 2}.  These rows read
    the float copy of D where the handle keeps one; the frame rows go through the CSR form and the fp64 D."""
    nv = (nx + 1) * (ny + 1)
    n = nv + 3 * nx * ny + nx + ny
    rows = np.zeros(n, dtype=bool)
    i, j = np.meshgrid(np.arange(i0, i0 + ni), np.arange(j0, j0 + nj), indexing="xy")
    i, j = i.ravel(), j.ravel()
    rows[j * (nx + 1) + i] = True
    for t in range(3):
        rows[nv + j * (3 * nx + 1) + 3 * i + t] = True
    return rows


def sym_mirrored(P):
    """[P, P] bool: True where k_patch_apply's LDS image takes entry (i, j) from the MIRRORED store of row j (column block of j
    strictly right of i's diagonal block); False where row i's own stored chunks deliver it."""
    i, j = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    return (j // 4) > (i // 4)


def gauss_jordan_inverse(A):
    """float64 twin of k_patch_invert's elimination on [np, P, P] matrices: in-place Gauss-Jordan without pivoting in the natural
    order (u rows first), the pivot row scaled by the reciprocal of the pivot, a_ij - f (p_j piv) on the other rows."""
    a = np.array(A, dtype=np.float64)
    P = a.shape[1]
    for k in range(P):
        pr = a[:, k, :].copy()
        piv = 1.0 / pr[:, k]
        prs = pr * piv[:, None]
        f = a[:, :, k].copy()
        new = a - f[:, :, None] * prs[:, None, :]
        new[:, :, k] = -f * piv[:, None]
        new[:, k, :] = prs
        new[:, k, k] = piv
        a = new
    return a


def gauss_jordan_inverse_divided(A):
    """The same elimination with other rounding: the pivot row DIVIDED by the pivot, (f p_j) / piv on the other rows."""
    a = np.array(A, dtype=np.float64)
    P = a.shape[1]
    for k in range(P):
        pr = a[:, k, :].copy()
        piv = pr[:, k].copy()
        f = a[:, :, k].copy()
        new = a - (f[:, :, None] * pr[:, None, :]) / piv[:, None, None]
        new[:, :, k] = -f / piv[:, None]
        new[:, k, :] = pr / piv[:, None]
        new[:, k, k] = 1.0 / piv
        a = new
    return a


def exact_inverse(A, digits=60):
    """Inverses of [np, P, P] float64 matrices in `digits`-digit arithmetic (mpmath), as a pair (hi, lo) of float64 arrays with
    hi + lo the inverse to about 32 digits."""
    import mpmath as mp

    A = np.asarray(A, dtype=np.float64)
    hi, lo = np.empty_like(A), np.empty_like(A)
    with mp.workdps(digits):
        for p in range(A.shape[0]):
            X = mp.inverse(mp.matrix(A[p].tolist()))
            for i in range(A.shape[1]):
                for j in range(A.shape[2]):
                    h = float(X[i, j])
                    hi[p, i, j] = h
                    lo[p, i, j] = float(X[i, j] - mp.mpf(h))
    return hi, lo


def inverse_scale(A):
    """[np, P, P] sqrt |A_ii A_jj| with a diagonal entry below 1e-150 counted as 1: the diagonal scaling in which inverses are compared
    (D(psi) = exp(psi) spans tens of orders of magnitude inside one patch)."""
    d = np.abs(np.einsum("pii->pi", np.asarray(A, dtype=np.float64)))
    s = np.sqrt(np.where(d < 1e-150, 1.0, d))
    return s[:, :, None] * s[:, None, :]


def inverse_error(A, Y, X):
    """e(Y) per patch = max_ij sqrt |A_ii A_jj| |Y_ij - X_ij|, X = exact_inverse(A)."""
    hi, lo = X
    return (inverse_scale(A) * np.abs((np.asarray(Y, dtype=np.float64) - hi) - lo)).max(axis=(1, 2))


def inverse_size(A, X):
    """per patch max_ij sqrt |A_ii A_jj| |X_ij|"""
    return (inverse_scale(A) * np.abs(X[0])).max(axis=(1, 2))


class P2CycleReference:
    def __init__(self, K, M, D, alpha, isbc, edges, nv, NN=None, patch_nu=2, patch_omega=0.8, grid=None, vcycle=None, table=None):
        """K, M, D: scalar n x n blocks of the P2 space (K, M unconstrained), n = nv + ne; isbc [n]: Dirichlet dofs of u; edges
        [ne, 2]: end vertices of edge dof nv + e; NN: slots per patch (None: as many as the mesh needs).  grid = (nx, ny) and vcycle
        = keyword arguments of VCycleReference (n_levels, min_nx, coarse_sweeps, tail_start, nu_tail) for the whole cycle."""
        self.K, self.M, self.D = (sp.csr_matrix(X, dtype=np.float64) for X in (K, M, D))
        self.alpha, self.nv, self.n = float(alpha), int(nv), self.K.shape[0]
        self.isbc = np.asarray(isbc, dtype=bool)
        self.edges = np.asarray(edges, dtype=np.int64)
        assert self.isbc.shape == (self.n,) and self.edges.shape == (self.n - self.nv, 2)
        self.patch_nu, self.patch_omega = int(patch_nu), float(patch_omega)
        # table: the slot order to work in (the device's exported table, once a test has checked it against star_table as sets)
        self.table = star_table(self.edges, self.nv, NN) if table is None else np.asarray(table, dtype=np.int64)
        self.NN = self.table.shape[1]
        self.T = p1_to_p2(self.edges, self.nv)
        self.TT = self.T.T.tocsr()
        keep = sp.diags((~self.isbc).astype(np.float64))
        self.A = (keep @ (self.alpha * self.K) @ keep + sp.diags(self.isbc.astype(np.float64))).tocsr()
        self.B = (keep @ self.M).tocsr()  # u rows x psi columns
        self.BT = self.B.T.tocsr()
        Df = self.D.copy()
        with np.errstate(over="ignore"):
            Df.data = Df.data.astype(np.float32).astype(np.float64)
        self.Df = Df
        # which stash entry a patch's edge slot fills: side 0 where the patch vertex is the edge's first end
        t = self.table
        e = np.maximum(t - self.nv, 0)
        self.side = np.where(t >= self.nv, (self.edges[e, 0] != np.arange(self.nv)[:, None]).astype(np.int64), -1)
        self.side[:, 0] = -1
        self.grid, self._vc, self._vckw, self._ops = grid, None, dict(vcycle or {}), {}

    # -- operators -------------------------------------------------------------------------------------------------------
    def operator(self, d_f32=False, km_dict=False):
        """J~ = [[A, B], [B^T, -D]], masked; d_f32: True / False, or a mask [n] of the psi rows whose D entries are the float32 values
        (the structured apply reads the float copy on its interior groups, its CSR frame rows the fp64 array); K and M as the
        dictionary of the nnz-balanced CSR kernel stores them where km_dict (dict_values)."""
        rows = np.broadcast_to(np.asarray(d_f32, dtype=bool), (self.n,))  # psi rows that read the float copy
        key = (rows.tobytes(), bool(km_dict))
        if key not in self._ops:
            pick = sp.diags(rows.astype(np.float64))
            Dm = (pick @ self.Df + (sp.identity(self.n) - pick) @ self.D).tocsr()
            A, B, BT = self.A, self.B, self.BT
            if km_dict:
                K, M = self.K.copy(), self.M.copy()
                K.data, M.data = dict_values(K.data), dict_values(M.data)
                keep = sp.diags((~self.isbc).astype(np.float64))
                A = (keep @ (self.alpha * K) @ keep + sp.diags(self.isbc.astype(np.float64))).tocsr()
                B = (keep @ M).tocsr()
                BT = B.T.tocsr()
            self._ops[key] = sp.bmat([[A, B], [BT, -Dm]]).tocsr()
        return self._ops[key]

    def residual(self, x, b, d_f32=False, km_dict=False):
        return np.asarray(b, dtype=np.float64) - self.operator(d_f32, km_dict) @ np.asarray(x, dtype=np.float64)

    def residual_scale(self, x, b, d_f32=False):
        """(|J~| |x| + |b|)_i: what a row's rounding errors are relative to."""
        return abs(self.operator(d_f32)) @ np.abs(x) + np.abs(b)

    def patch_matrices(self):
        """[nv, 2 NN, 2 NN] patch matrices in (u slots, psi slots) order."""
        t, NN, n = self.table, self.NN, self.n
        live = t >= 0
        idx = np.maximum(t, 0)
        J = self.operator().toarray()
        P = 2 * NN
        full = np.concatenate([idx, n + idx], axis=1)  # [nv, P] rows of J
        ok = np.concatenate([live, live], axis=1)
        A = J[full[:, :, None], full[:, None, :]]
        A = np.where(ok[:, :, None] & ok[:, None, :], A, 0.0)
        A[:, np.arange(P), np.arange(P)] = np.where(ok, A[:, np.arange(P), np.arange(P)], 1.0)
        return A

    # -- transfers -------------------------------------------------------------------------------------------------------
    def restrict(self, r, dtype=np.float64):
        """[u | psi] of the P1 space = T^T r per block, the u rows of Dirichlet vertices zeroed."""
        n, nv = self.n, self.nv
        r = np.asarray(r, dtype=dtype)
        TT = self.TT.astype(dtype)
        cu, cp = TT @ r[:n], TT @ r[n:]
        cu = np.where(self.isbc[:nv], dtype(0.0), cu)
        return np.concatenate([cu, cp])

    def restrict_scale(self, r):
        """sum of the absolute terms of every entry of restrict(r) (masked rows included)"""
        n = self.n
        r = np.abs(np.asarray(r, dtype=np.float64))
        return np.concatenate([self.TT @ r[:n], self.TT @ r[n:]])

    def prolong_add(self, x, c, dtype=np.float64):
        n, nv = self.n, self.nv
        x, c = np.asarray(x, dtype=dtype), np.asarray(c, dtype=dtype)
        T = self.T.astype(dtype)
        return np.concatenate([x[:n] + T @ c[:nv], x[n:] + T @ c[nv:]])

    def prolong_scale(self, x, c):
        n, nv = self.n, self.nv
        x, c = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(c, dtype=np.float64))
        return np.concatenate([x[:n] + self.T @ c[:nv], x[n:] + self.T @ c[nv:]])

    # -- the sweep -------------------------------------------------------------------------------------------------------
    def patch_solve(self, Ainv, r, absolute=False):
        """y [nv, 2 NN] = Ainv_p R_p r (absolute: |Ainv_p| R_p |r|)."""
        t, n = self.table, self.n
        live = t >= 0
        idx = np.maximum(t, 0)
        r = np.asarray(r, dtype=np.float64)
        rp = np.concatenate([np.where(live, r[idx], 0.0), np.where(live, r[n + idx], 0.0)], axis=1)
        if absolute:
            return np.einsum("pij,pj->pi", np.abs(Ainv), np.abs(rp))
        return np.einsum("pij,pj->pi", Ainv, rp)

    def _scatter(self, y, omega, stash_f32):
        """(dx [2 n], ymax [2 n]): the update of a sweep from patch solutions y; ymax = max(|y_a|, |y_b|) on edge dofs, 0 on vertices."""
        n, nv, NN, t = self.n, self.nv, self.NN, self.table
        ne = n - nv
        dx, ymax = np.zeros(2 * n), np.zeros(2 * n)
        for f in range(2):
            yf = y[:, f * NN:(f + 1) * NN]
            dx[f * n:f * n + nv] = omega * yf[:, 0]
            stash = np.zeros((ne, 2))
            m = self.side >= 0
            stash[t[m] - nv, self.side[m]] = yf[m]
            if stash_f32:
                with np.errstate(over="ignore"):
                    stash = stash.astype(np.float32).astype(np.float64)
            dx[f * n + nv:(f + 1) * n] = omega * 0.5 * (stash[:, 0] + stash[:, 1])
            ymax[f * n + nv:(f + 1) * n] = np.abs(stash).max(axis=1)
        return dx, ymax

    def sweep(self, x, r, Ainv, omega=None, stash_f32=False):
        """x + omega W sum_p R_p^T Ainv_p R_p r for a GIVEN residual r."""
        omega = self.patch_omega if omega is None else float(omega)
        dx, _ = self._scatter(self.patch_solve(Ainv, r), omega, stash_f32)
        return np.asarray(x, dtype=np.float64) + dx

    def sweep_scales(self, r, Ainv, omega=None):
        """(s [2 n], ymax [2 n]): s_i = omega sum_j |Ainv_ij| |r_j| (on an edge dof the mean over its two patches, as the update is);
        ymax_i = max(|y_a|, |y_b|) on edge dofs."""
        omega = self.patch_omega if omega is None else float(omega)
        s, _ = self._scatter(self.patch_solve(Ainv, r, absolute=True), omega, False)
        _, ymax = self._scatter(self.patch_solve(Ainv, r), omega, False)
        return s, ymax

    # -- the whole cycle -------------------------------------------------------------------------------------------------
    def coarse_blocks(self):
        """(K1, M1, D1) = T^T . T of the three blocks: what the P1 hierarchy under a P2 handle starts from."""
        return tuple((self.TT @ X @ self.T).tocsr() for X in (self.K, self.M, self.D))

    def vcycle_reference(self):
        if self._vc is None:
            assert self.grid is not None, "the whole cycle needs the grid of the P1 hierarchy"
            nx, ny = self.grid
            K1, M1, D1 = self.coarse_blocks()
            self._vc = VR.VCycleReference(K1, M1, D1, self.alpha, nx, ny, self.isbc[:self.nv], **self._vckw)
        return self._vc

    def cycle(self, b, Ainv, nu=6, omega=0.75, stash_f32=False, d_f32=False):
        """z = the preconditioner applied to b, with a V(nu, nu) cycle of damping omega on the P1 hierarchy."""
        b = np.asarray(b, dtype=np.float64)
        x = self.sweep(np.zeros_like(b), b, Ainv, stash_f32=stash_f32)
        for _ in range(1, self.patch_nu):
            x = self.sweep(x, self.residual(x, b, d_f32), Ainv, stash_f32=stash_f32)
        c = self.restrict(self.residual(x, b, d_f32))
        zc = self.vcycle_reference().vcycle(c, 0, nu=nu, omega=omega, mode="f64")
        x = self.prolong_add(x, zc)
        for _ in range(self.patch_nu):
            x = self.sweep(x, self.residual(x, b, d_f32), Ainv, stash_f32=stash_f32)
        return x
