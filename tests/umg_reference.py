"""numpy statement of the multigrid cycle on refined general meshes (include/pgx.h: pgx_set_hierarchy; csrc/pgx_umg.hip).

TEST INFRASTRUCTURE ONLY.  Fed from the level-0 blocks K, M, D (scipy CSR, unconstrained values), alpha, the level-0 Dirichlet mask and
the `parents` arrays of fem.Mesh.hierarchy (fine -> coarse).

  P_t         two entries of 1/2 per row, on the same column for an inherited vertex (fem.prolongation)
  level l+1   P^T K P, P^T M P, P^T D P of the UNCONSTRAINED level-l values; mask = the fine mask on the inherited vertices
  operator    per level as k_bspmv applies the mask: identity row and column in the u block, the u column zeroed in the psi rows
                 y_u = bc ? x_u : alpha K x~_u + M x_psi        x~_u = x_u with the Dirichlet entries zeroed
                 y_p =             M x~_u - D x_psi
  smoother    damped collective Jacobi (k_bspmv MODE 2): per vertex the block [[a, b], [b, -d]] = [[alpha K_ii, M_ii], [M_ii, -D_ii]],
              on a Dirichlet row [[1, 0], [0, -d]] with damping 1 on u; det = -a d - b^2; det == 0 (a Dirichlet row with d == 0)
              leaves psi alone and sets u exactly
  cycle       nu sweeps from zero | r = b - J x | b_c = P^T r, u part zeroed on the coarse Dirichlet rows | recursion | x += P c | nu
              sweeps; the coarsest level runs coarse_sweeps sweeps from zero

Vectors are [u | psi]; every routine also takes a matrix of such columns."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def prolongation(parents, n_coarse):
    parents = np.asarray(parents)
    nf = len(parents)
    P = sp.csr_matrix((np.full(2 * nf, 0.5), (np.repeat(np.arange(nf), 2), parents.ravel())), shape=(nf, n_coarse))
    P.sum_duplicates()
    return P


def coarse_sizes(parents_list):
    return [int(np.count_nonzero(np.asarray(p)[:, 0] == np.asarray(p)[:, 1])) for p in parents_list]


def _col(v, like):
    return v.reshape((-1,) + (1,) * (like.ndim - 1))


class UmgReference:
    def __init__(self, K, M, D, alpha, mask, parents_list, coarse_sweeps=60):
        self.alpha, self.coarse_sweeps = float(alpha), int(coarse_sweeps)
        self.levels = []
        K, M, D = sp.csr_matrix(K), sp.csr_matrix(M), sp.csr_matrix(D)
        mask = np.asarray(mask, dtype=bool)
        sizes = coarse_sizes(parents_list)
        for t in range(len(parents_list) + 1):
            self.levels.append(self._level(K, M, D, mask))
            if t == len(parents_list):
                break
            P = prolongation(parents_list[t], sizes[t])
            assert P.shape[0] == K.shape[0], (P.shape, K.shape)
            self.levels[-1]["P"] = P
            K, M, D = (P.T @ K @ P).tocsr(), (P.T @ M @ P).tocsr(), (P.T @ D @ P).tocsr()
            mask = mask[: sizes[t]]

    def _level(self, K, M, D, mask):
        for A in (K, M, D):
            A.sort_indices()
        keep = sp.diags((~mask).astype(float))
        A = (keep @ (self.alpha * K) @ keep + sp.diags(mask.astype(float))).tocsr()
        B = (keep @ M).tocsr()   # u rows x psi columns
        BT = (M @ keep).tocsr()  # psi rows x u columns
        a, b, d = A.diagonal(), B.diagonal(), D.diagonal()
        return dict(K=K, M=M, D=D, mask=mask, n=K.shape[0], A=A, B=B, BT=BT, blk=(a, b, d, -a * d - b * b))

    def n(self, level):
        return self.levels[level]["n"]

    def matrix(self, level=0):
        """The constrained operator of a level, [[A, B], [B^T, -D]]."""
        L = self.levels[level]
        return sp.bmat([[L["A"], L["B"]], [L["BT"], -L["D"]]]).tocsr()

    def apply(self, level, xu, xp):
        L = self.levels[level]
        return L["A"] @ xu + L["B"] @ xp, L["BT"] @ xu - L["D"] @ xp

    def smooth(self, level, xu, xp, bu, bp, its, omega):
        L = self.levels[level]
        a, b, d, det = L["blk"]
        ok = det != 0.0
        sdet = np.where(ok, det, 1.0)
        om_u = np.where(L["mask"], 1.0, omega)
        for _ in range(its):
            yu, yp = self.apply(level, xu, xp)
            su, s_p = bu - yu, bp - yp
            du = np.where(_col(ok, su), (_col(-d, su) * su - _col(b, su) * s_p) / _col(sdet, su), np.where(_col(L["mask"], su), su, 0.0))
            dp = np.where(_col(ok, su), (_col(-b, su) * su + _col(a, su) * s_p) / _col(sdet, su), 0.0)
            xu = xu + _col(om_u, su) * du
            xp = xp + omega * dp
        return xu, xp

    def _cycle(self, level, bu, bp, nu, omega):
        L = self.levels[level]
        xu, xp = np.zeros_like(bu), np.zeros_like(bp)
        if "P" not in L:
            return self.smooth(level, xu, xp, bu, bp, self.coarse_sweeps, omega)
        xu, xp = self.smooth(level, xu, xp, bu, bp, nu, omega)
        yu, yp = self.apply(level, xu, xp)
        P = L["P"]
        keep_c = (~self.levels[level + 1]["mask"]).astype(float)
        cbu = P.T @ (bu - yu)
        cu, cp = self._cycle(level + 1, _col(keep_c, cbu) * cbu, P.T @ (bp - yp), nu, omega)
        xu, xp = xu + P @ cu, xp + P @ cp
        return self.smooth(level, xu, xp, bu, bp, nu, omega)

    def cycle(self, level, b, nu=6, omega=0.75):
        """One V(nu, nu) cycle entered on `level` from a zero guess; b = [u | psi] of that level (or columns of such)."""
        n = self.n(level)
        b = np.asarray(b, dtype=np.float64)
        zu, zp = self._cycle(level, b[:n], b[n:], nu, omega)
        return np.concatenate([zu, zp])


def build_mesh(name):
    """The three small meshes of the tests (vertices per level / largest vertex degree): D5 227, 64, 20 / 7; D34 469, 127, 37 / 6;
    X32 809, 213, 59, 18 / 8 (nested: refined without snapping)."""
    from proximalgalerkin_amd import fem

    if name == "D5":
        return fem.create_disk(0.5, refinements=2)
    if name == "D34":
        return fem.create_disk(0.34, refinements=2)
    if name == "X32":
        msh = fem.create_rectangle(((-1.0, -1.0), (1.0, 1.0)), (3, 2), diagonal="crossed")
        for _ in range(3):
            msh = fem.refine(msh)
        return msh
    raise KeyError(name)


def state(coords, seed=11):
    """(x, xk) as the V-cycle operator tests build them (tests/test_gpu_vcycle_operator.py): psi mostly negative, exp(psi) over several
    orders of magnitude, and a patch - here the vertices within 0.25 of (0.3, 0.2) - pushed down by 800, where exp(psi) underflows
    to exact zeros in D."""
    from tests.test_gpu_structured_kernels import _state

    n = len(coords)
    x, xk = _state(2 * n, seed)
    x[n:][np.hypot(coords[:, 0] - 0.3, coords[:, 1] - 0.2) < 0.25] -= 800.0
    return x, xk


def vertex_degrees(mesh):
    e = mesh.edges()[0]
    return np.bincount(e.ravel(), minlength=mesh.num_vertices)


def make_linear_solve(prob, parents_list, nu=6, omega=0.75, rtol=1e-10, maxit=200, coarse_sweeps=60, stats=None):
    """linear_solve(J, b) for oracle.pg_oracle.newton_solve: oracle/krylov_proto.fgmres on the exact Jacobian, preconditioned by the
    cycle above; appends the Krylov count of every call to `stats`."""
    from oracle.krylov_proto import fgmres

    n = prob.n

    def solve(J, b):
        J = J.tocsr()
        i = int(np.flatnonzero(~prob.isbc)[0])
        alpha = J[i, i] / prob.K[i, i]
        ref = UmgReference(prob.K, prob.M, -J[n:, n:], alpha, prob.isbc, parents_list, coarse_sweeps=coarse_sweeps)
        x, its, _ = fgmres(J, b, lambda r: ref.cycle(0, r, nu, omega), rtol, maxit)
        if stats is not None:
            stats.append(its)
        return x

    return solve
