#!/usr/bin/env python3
"""Time the dense LU with partial pivoting (include/pgx_dn.h) on the Newton matrices it was built for: the Monge-Ampere Jacobians of
example 10's p-study (2 x 2 mesh, degrees k), assembled at the initial state by the numpy restatement tests/monge_ampere_reference.py.

Per degree: N, the share of structural nonzeros, device-event milliseconds of pgx_dn_factor (zero fill, scatter, P A = L U) and of
pgx_dn_solve - one warm-up, then `--repeats` calls, smallest / median / largest -, 2 N^3 / 3 flops over the median factorisation time
as a share of the 78.6 TF/s fp64 matrix peak, the number of kernel launches a factorisation issues (counted from the shapes), and the
check that goes with every timing: pivot vector equal to LAPACK's, normwise backward error |Jx - b| / (|J|_1 |x| + |b|) next to LAPACK's.

    python tools/dn_profile.py --degrees 3 6 10 14 --out profiles/dn_ma_jacobians.json
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import scipy.linalg as sla

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import monge_ampere_reference as R  # noqa: E402

PEAK_FP64_MFMA = 78.6e12


def launches(n, nb=64):
    """kernel launches of one pgx_dn_factor, from the loop structure of csrc/pgx_dn.hip (the two memsets and the copies not counted)"""
    total = 2  # scatter, diagonal
    for j0 in range(0, n, nb):
        w = min(nb, n - j0)
        total += 1  # colmax
        total += sum(1 + (1 if n - j - 1 > 0 else 0) for j in range(j0, j0 + w))  # pivot, update
        total += (1 if n > w else 0) + (2 if j0 + w < n else 0)  # laswp, trsm + gemm
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", type=int, nargs="+", default=[3, 6, 10, 14])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from proximalgalerkin_amd.direct import DenseSolver

    rows = []
    for k in a.degrees:
        t0 = time.time()
        prob = R.MongeAmpere(2, k)
        J = prob.jacobian(prob.initial_state())
        N = J.shape[0]
        Jd = J.toarray()
        lu, piv = sla.lu_factor(Jd)
        b = np.random.default_rng(k).standard_normal(N)
        normJ = float(abs(J).sum(axis=0).max())  # 1-norm (a 2-norm of the k = 14 matrix is a 5 286 x 5 286 SVD)
        berr = lambda x: float(np.linalg.norm(Jd @ x - b) / (normJ * np.linalg.norm(x) + np.linalg.norm(b)))  # noqa: E731
        ds = DenseSolver(J.indptr, J.indices, device=0)
        ds.factor(J.data)  # warm-up: code objects, first touch of the n x n array
        x = ds.solve(b)
        ds.timing(True)
        fms, sms = [], []
        for _ in range(a.repeats):
            ds.factor(J.data)
            f, _ = ds.timing(True)
            ds.solve(b)
            _, s = ds.timing(True)
            fms.append(f), sms.append(s)
        st = ds.stats()
        row = dict(k=k, N=N, nnz=int(J.nnz), nonzero_share=J.nnz / float(N) ** 2, launches_per_factor=launches(N),
                   factor_ms=dict(min=min(fms), median=float(np.median(fms)), max=max(fms)),
                   solve_ms=dict(min=min(sms), median=float(np.median(sms)), max=max(sms)),
                   flops=2.0 * N ** 3 / 3.0, share_of_fp64_mfma_peak=2.0 * N ** 3 / 3.0 / (float(np.median(fms)) * 1e-3) / PEAK_FP64_MFMA,
                   pivots_equal_lapack=bool(np.array_equal(ds.pivots(), piv)), interchanges=int(st["interchanges"]),
                   min_pivot=st["min_pivot"], max_pivot=st["max_pivot"], backward_error=berr(x),
                   backward_error_lapack=berr(sla.lu_solve((lu, piv), b)), host_setup_s=time.time() - t0)
        ds.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        out = pathlib.Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(dict(tool="tools/dn_profile.py", repeats=a.repeats, peak_fp64_mfma=PEAK_FP64_MFMA, rows=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
