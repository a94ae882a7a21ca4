#!/usr/bin/env python3
"""Write tests/golden/monge_ampere_{name}.npz: example 10 (three-field mixed Monge-Ampere, u in P_k, p in [P_{k+1}]^2, Psi in [P_k]^3)
run by the numpy / scipy restatement tests/monge_ampere_reference.py with the reference's solver options: per level the mesh, the
degree, the quadrature degree, SNES reason, Newton count, L2 error and the final state x = [u | p0 | p1 | Psi00 | Psi01 | Psi11].

Each run is repeated twice from an initial state perturbed by 1e-13 and 1e-11 (standard normal, absolute).  `sensitivity` is the
largest difference of the final state of a level per block (relative to max(1, max |block|)) between the run and the reruns.  A
golden is WRITTEN only if every level converged and both reruns reproduce the reasons and Newton counts; the tool refuses otherwise.
The committed files:

    python tools/make_monge_ampere_golden.py A    # n = 2, k = 3 cold, then k = 4 warm (p-transfer)
    python tools/make_monge_ampere_golden.py B    # n = (3, 2), k = 2 cold, then n = (6, 4) warm (h-transfer, nx != ny)
    python tools/make_monge_ampere_golden.py C    # n = 2, k = 2, nonsmooth data
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import monge_ampere_reference as R  # noqa: E402

RUNS = {"A": dict(levels=[((2, 2), 3), ((2, 2), 4)], nonsmooth=False),
        "B": dict(levels=[((3, 2), 2), ((6, 4), 2)], nonsmooth=False),
        "C": dict(levels=[((2, 2), 2)], nonsmooth=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name", choices=sorted(RUNS))
    ap.add_argument("--dry-run", action="store_true", help="measure and report, write nothing")
    a = ap.parse_args()
    p = RUNS[a.name]
    levels = [(n, k, None) for n, k in p["levels"]]
    run = R.run_levels(levels, nonsmooth=p["nonsmooth"])
    for (n, k, _), prob, reason, its, err in zip(levels, run["problems"], run["reasons"], run["its"], run["errors"]):
        print(f"{a.name}: n {n} k {k} degree {prob.degree} ({prob.nq} points), {prob.ndofs} unknowns: reason {reason}, {its} Newton steps, "
              f"L2 error {err:.6e}", flush=True)
    if len(run["reasons"]) != len(levels) or min(run["reasons"]) <= 0:
        raise SystemExit(f"golden {a.name}: a level did not converge: not written")
    sens = np.zeros((len(levels), 6))
    for scale in (1e-13, 1e-11):
        rerun = R.run_levels(levels, nonsmooth=p["nonsmooth"], perturb=scale, seed=3)
        ok = rerun["reasons"] == run["reasons"] and rerun["its"] == run["its"]
        dd = np.array([R.field_differences(P, zr, z) for P, zr, z in zip(run["problems"], rerun["states"], run["states"])])
        print(f"  perturbed by {scale:g}: reasons and counts {'agree' if ok else 'DIFFER'}, final states moved by {dd.max(axis=1)}", flush=True)
        if not ok:
            raise SystemExit(f"golden {a.name} is not reproducible under perturbation: not written")
        sens = np.maximum(sens, dd)
    if a.dry_run:
        return
    out = ROOT / "tests" / "golden" / f"monge_ampere_{a.name}.npz"
    data = dict(n=np.array([n for n, _, _ in levels]), k=np.array([k for _, k, _ in levels]), nonsmooth=p["nonsmooth"],
                quadrature_degree=np.array([P.degree for P in run["problems"]]), reasons=np.array(run["reasons"]),
                newton_its=np.array(run["its"]), l2_errors=np.array(run["errors"]), sensitivity=sens)
    for i, z in enumerate(run["states"]):
        data[f"z{i}"] = z
    np.savez_compressed(out, **data)
    print("wrote", out, out.stat().st_size, "bytes; sensitivity", sens.max(axis=1))


if __name__ == "__main__":
    main()
