#!/usr/bin/env python3
"""Write tests/golden/eigenvalue_{name}.npz: example 07 (eigenvalue-constrained Q-tensor, Q_p on N x N rectangles) run by the numpy /
scipy restatement tests/eigenvalue_reference.py with the reference's solver options: the parameters, the log of attempts
(k, alpha, its, reason, failed), the Newton counts per LVPP step and the final state z = [q1 | q2 | psi1 | psi2].

Each run is repeated twice from an initial state perturbed by 1e-13 and 1e-11 (standard normal, absolute).  `sensitivity` is the
largest difference of the final state per field (q1, q2 absolute; psi1, psi2 relative to max |psi|) between the run and the reruns.
A golden is WRITTEN only if both reruns reproduce its log under the comparison rule (eigenvalue_reference.logs_agree); the tool
refuses otherwise.  In all three d N is an integer, so the Dirichlet data do not depend on the node family.  The committed files:

    python tools/make_eigenvalue_golden.py A    # p 3, N 4, degree 20, d 0.25, A 1 (the script's): constraint inactive, max |q| 0.5
    python tools/make_eigenvalue_golden.py B    # p 3, N 4, degree 20, d 0.25, A -2000: constraint active
    python tools/make_eigenvalue_golden.py C    # p 2, N 6, degree 8, d 0.5, A -500: nodal |q| exceeds 1
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import eigenvalue_reference as R  # noqa: E402

RUNS = {"A": dict(p=3, N=4, quadrature_degree=20, d=0.25, A=1.0, C=4.0),
        "B": dict(p=3, N=4, quadrature_degree=20, d=0.25, A=-2000.0, C=4.0),
        "C": dict(p=2, N=6, quadrature_degree=8, d=0.5, A=-500.0, C=4.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name", choices=sorted(RUNS))
    ap.add_argument("--dry-run", action="store_true", help="measure and report, write nothing")
    a = ap.parse_args()
    p = RUNS[a.name]
    P = R.Eigenvalue(p["N"], p["N"], p["p"], p["quadrature_degree"] // 2 + 1, A=p["A"], C=p["C"], d=p["d"])
    run = R.solve(P)
    log = run["log"]
    z = run["z"]
    q = np.hypot(z[:P.n], z[P.n:2 * P.n])
    print(f"{a.name}: {P.ndofs} unknowns, {len(log)} attempts, {int(run['newton_its'].sum())} Newton steps in {len(run['newton_its'])} LVPP "
          f"steps, {int(log[:, 4].sum())} failed, max nodal |q| {q.max():.6f}, max |psi| {np.abs(z[2 * P.n:]).max():.4f}", flush=True)
    sens = np.zeros(4)
    rng = np.random.default_rng(3)
    for scale in (1e-13, 1e-11):
        rerun = R.solve(P, z0=scale * rng.standard_normal(P.ndofs))
        ok = R.logs_agree(log, rerun["log"])
        dd = R.field_differences(P.n, rerun["z"], z)
        print(f"  perturbed by {scale:g}: log {'agrees' if ok else 'DIFFERS'}, final state moved by {dd}", flush=True)
        if not ok:
            raise SystemExit(f"golden {a.name} is not reproducible under perturbation: not written")
        sens = np.maximum(sens, dd)
    if a.dry_run:
        return
    out = ROOT / "tests" / "golden" / f"eigenvalue_{a.name}.npz"
    np.savez_compressed(out, p=p["p"], N=p["N"], quadrature_degree=p["quadrature_degree"], d=p["d"], A=p["A"], C=p["C"], log=log,
                        newton_its=run["newton_its"], z=z, max_q=q.max(), sensitivity=sens)
    print("wrote", out, "sensitivity", sens)


if __name__ == "__main__":
    main()
