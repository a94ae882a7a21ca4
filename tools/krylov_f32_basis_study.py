#!/usr/bin/env python3
"""Does a SINGLE-PRECISION Krylov basis cost Krylov iterations, and how many bytes does it save?  CPU twin of fgmres (csrc/pgx_krylov.hip)
on the lean P1 path: one full settings-B LVPP run per row, the Newton systems solved by the FGMRES of oracle/krylov_proto.py extended
by what the library's loop has - restart 30, lazy normalisation, the selective second projection (eta = 0.01), the true residual
b - J x in fp64 after every cycle, the attainable-accuracy exit - and preconditioned by the single-precision V(nu,nu) cycle with D as
bf16 and omega = 0.75 (MG32 of tools/mg32_study.py).  Rows: the fp64 basis, then the basis stored through astype(np.float32) (w, the
dot products and the projections stay fp64 on the widened vectors; the norm kept is that of the ROUNDED vector) with a cycle ending
once its Arnoldi estimate has gained tau over the true residual the cycle started from, tau = 1e-4, 1e-5, 1e-6 and 0 (no early
end: the estimate stalls near the float floor and every solve runs into the restart - DESIGN.md section 3).

Units: one unit is one pass over an fp64 vector.  Iteration j of a cycle (j = 0, 1, ...) costs 2 j + 5 units with the fp64 basis
(pass 1 reads j + 1 vectors and w, pass 2 reads them again and writes w) and j + 3.5 with the float basis (half a unit per basis
vector read or written); a second projection costs the same again less the write-back of fp64 w.

    python tools/krylov_f32_basis_study.py N [nu]        (needs only numpy / scipy and oracle/; N = 64: minutes)"""
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from oracle import pg_oracle as O  # noqa: E402
from mg32_study import MG32  # noqa: E402  (the float32 twin of oracle/krylov_proto.py's CollectiveMG)

RESTART, ETA2 = 30, 1e-4


def fgmres(A, b, prec, rtol, maxit, basis32, tau, count):
    """x, iterations.  count: dict with 'units' (Gram-Schmidt traffic) and 'second' (second projections), added to."""
    store = (lambda v: v.astype(np.float32)) if basis32 else (lambda v: v)
    bnorm = float(np.linalg.norm(b))
    x = np.zeros_like(b)
    if bnorm == 0.0:
        return x, 0
    target, its, prev = rtol * bnorm, 0, bnorm
    r, beta = b, bnorm
    half = 0.5 if basis32 else 1.0  # units per basis vector pass
    while True:
        W, s, Z = [store(r / beta)], [1.0], []  # stored vectors, their scales (v_i = s_i W_i), preconditioned vectors
        H = np.zeros((RESTART + 1, RESTART))
        cycle_target = max(target, tau * beta) if basis32 else target
        y = None
        for j in range(RESTART):
            z = prec(s[j] * W[j].astype(np.float64))
            Z.append(z)
            w = A @ z
            c1 = np.array([s[i] * s[i] * (W[i].astype(np.float64) @ w) for i in range(j + 1)])  # coefficients on the stored W_i
            for i in range(j + 1):
                w = w - c1[i] * W[i].astype(np.float64)
            h1 = c1 / np.array(s[: j + 1])
            H[: j + 1, j] = h1
            wn = store(w)
            wp2 = float(wn.astype(np.float64) @ wn.astype(np.float64))
            count["units"] += half * (j + 1) + 1 + half * (j + 1) + 1 + (half if basis32 else 1.0)
            if wp2 < ETA2 * (wp2 + float(h1 @ h1)):  # the first projection cancelled most of w: project the STORED vector again
                w = wn.astype(np.float64)
                c2 = np.array([s[i] * s[i] * (W[i].astype(np.float64) @ w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - c2[i] * W[i].astype(np.float64)
                H[: j + 1, j] += c2 / np.array(s[: j + 1])
                wn = store(w)
                wp2 = float(wn.astype(np.float64) @ wn.astype(np.float64))
                count["units"] += 2 * (half * (j + 1) + half) + (0.0 if basis32 else 1.0) + half
                count["second"] += 1
            hn = np.sqrt(wp2)
            H[j + 1, j] = hn
            W.append(wn)
            s.append(1.0 / hn if hn > 0.0 else 1.0)
            e = np.zeros(j + 2)
            e[0] = beta
            y = np.linalg.lstsq(H[: j + 2, : j + 1], e, rcond=None)[0]
            res = float(np.linalg.norm(H[: j + 2, : j + 1] @ y - e))
            its += 1
            if res <= cycle_target or hn == 0.0 or its >= maxit:
                break
        x = x + sum(yi * zi for yi, zi in zip(y, Z))
        r = b - A @ x  # the TRUE residual decides, not the estimate
        beta = float(np.linalg.norm(r))
        if beta <= target or (beta > 0.1 * prev and beta <= 1e-7 * bnorm) or its >= maxit:
            return x, its
        prev = beta


def make(prob, N, nu, stats, count, basis32, tau):
    n = prob.n

    def solve(J, b):
        J = J.tocsr()
        i = int(np.flatnonzero(~prob.isbc)[0])
        mg = MG32(prob.K, prob.M, -J[n:, n:], J[i, i] / prob.K[i, i], N, prob.isbc, nmin32=0, narrow="D", nu=nu, omega=0.75)
        x, its = fgmres(J, b, lambda v: np.concatenate([q.astype(np.float64) for q in mg.vcycle(v[:n], v[n:])]), 1e-10, 200, basis32, tau, count)
        stats.append(its)
        return x

    return solve


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    nu = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    coords, cells = O.create_rectangle(N, N)
    prob = O.ObstacleP1(coords, cells, O.boundary_vertices_rectangle(N, N))
    ref = ref_units = ref_newton = None
    print(f"N = {N}, V({nu},{nu}), D as bf16, omega 0.75, restart {RESTART}, eta {np.sqrt(ETA2):g}")
    for name, basis32, tau in (("fp64 basis", False, 0.0), ("float basis, tau 1e-4", True, 1e-4), ("float basis, tau 1e-5", True, 1e-5),
                               ("float basis, tau 1e-6", True, 1e-6), ("float basis, no early cycle end", True, 0.0)):
        stats, count, t = [], {"units": 0.0, "second": 0}, time.time()
        with np.errstate(over="ignore", invalid="ignore"):
            x, h = O.solve_problem(prob, 500, "double_exponential", 1e2, 1e-4, linear_solve=make(prob, N, nu, stats, count, basis32, tau))
        if ref is None:
            ref, ref_units, ref_newton = x, count["units"], h["Newton steps"]
        du = np.linalg.norm(x[: prob.n] - ref[: prob.n]) / np.linalg.norm(ref[: prob.n])
        print(f"{name:32s} Krylov {sum(stats):4d} (per solve {min(stats)}-{max(stats)})  Newton {'same' if h['Newton steps'] == ref_newton else h['Newton steps']}"
              f"  second projections {count['second']:3d}  units {count['units']:7.0f} ({100 * (count['units'] / ref_units - 1):+.0f} %)"
              f"  |u - u_fp64|/|u| {du:.1e}  ({time.time() - t:.0f} s)", flush=True)


if __name__ == "__main__":
    main()
