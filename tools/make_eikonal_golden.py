#!/usr/bin/env python3
"""Write tests/golden/eikonal_{name}.npz: example 09 (the eikonal equation on a Moebius strip, u in Q1, psi in [Q2]^3) run by the numpy /
scipy restatement tests/eikonal_reference.py with the reference's solver options: the settings, the log of LVPP steps
(i, alpha, Newton its, reason), the increments |delta u| and the final state z = [u | psi0 | psi1 | psi2].

Each run is repeated twice from an initial state perturbed by 1e-13 and 1e-11 (standard normal, absolute).  `sensitivity` is the
largest difference of the final state per field (u absolute; psi relative to max |psi|) between the run and the reruns.  A golden is
WRITTEN only if both reruns reproduce its log exactly; the tool refuses otherwise.  The committed files:

    python tools/make_eikonal_golden.py A    # nu 8,  nv 2, g 3, nq1 6, scale 1:  264 unknowns
    python tools/make_eikonal_golden.py B    # nu 16, nv 4, g 3, nq1 6, scale 1:  944 unknowns
    python tools/make_eikonal_golden.py C    # nu 6,  nv 1, g 2, nq1 5, scale 2:  120 unknowns
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import eikonal_reference as R  # noqa: E402

RUNS = {"A": dict(nu=8, nv=2, g=3, nq1=6, scale=1.0),
        "B": dict(nu=16, nv=4, g=3, nq1=6, scale=1.0),
        "C": dict(nu=6, nv=1, g=2, nq1=5, scale=2.0)}
TOL = 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name", choices=sorted(RUNS))
    ap.add_argument("--dry-run", action="store_true", help="measure and report, write nothing")
    a = ap.parse_args()
    p = RUNS[a.name]
    P = R.Eikonal(p["nu"], p["nv"], p["g"], p["nq1"], scale=p["scale"])
    run = R.solve(P, tol=TOL)
    log, z = run["log"], run["z"]
    print(f"{a.name}: {P.ndofs} unknowns, {len(log)} LVPP steps, {int(log[:, 2].sum())} Newton steps, reasons {sorted(set(log[:, 3].astype(int)))}, "
          f"max u {z[:P.n1].max():.6f}, max |psi| {np.abs(z[P.n1:]).max():.4f}", flush=True)
    sens = np.zeros(2)
    rng = np.random.default_rng(3)
    for scale in (1e-13, 1e-11):
        rerun = R.solve(P, tol=TOL, z0=scale * rng.standard_normal(P.ndofs))
        ok = np.array_equal(log, rerun["log"])
        dd = R.field_differences(P.n1, rerun["z"], z)
        print(f"  perturbed by {scale:g}: log {'agrees' if ok else 'DIFFERS'}, final state moved by {dd}", flush=True)
        if not ok:
            raise SystemExit(f"golden {a.name} is not reproducible under perturbation: not written")
        sens = np.maximum(sens, dd)
    if a.dry_run:
        return
    out = ROOT / "tests" / "golden" / f"eikonal_{a.name}.npz"
    np.savez_compressed(out, nu=p["nu"], nv=p["nv"], g=p["g"], nq1=p["nq1"], scale=p["scale"], tol=TOL, log=log,
                        increments=run["increments"], z=z, max_u=z[:P.n1].max(), sensitivity=sens)
    print("wrote", out, "sensitivity", sens)


if __name__ == "__main__":
    main()
