#!/usr/bin/env python3
"""Write tests/golden/multiphase_p1_n{N}[_{scheme}][_a{alpha_0}]_steps{S}.npz: example 04 (four-phase Cahn-Hilliard, P1 on the crossed unit square)
run by the numpy / scipy restatement tests/multiphase_reference.py with the reference's defaults (dt 1e-5, alpha constant 1,
20 LVPP iterations at most, stopping tolerance 1e-5) for the first S time steps: final u and psi, per-step Newton and LVPP counts.

Also stored: the smallest accepted line-search lambda and the number of cubic fits of the run, so that a test can tell
that the cubic branch of bt was taken.  The committed files:

    python tools/make_multiphase_golden.py                                   # N = 16, 20 steps, alpha constant
    python tools/make_multiphase_golden.py --N 8 --steps 10 --scheme {constant,linear,doubling}
    python tools/make_multiphase_golden.py --N 4 --steps 2 --alpha_0 20     # backtracks, with a cubic fit

The reference's own size, N = 50, is out of reach of the restatement: one SuperLU factorisation of its 61 212-dof
Jacobian takes about 12 s and the first 20 steps need about 900 of them.
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import multiphase_reference as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--scheme", default="constant", choices=["constant", "linear", "doubling"])
    ap.add_argument("--alpha_0", type=float, default=1.0)
    a = ap.parse_args()
    coords, cells = R.crossed_unit_square(a.N, a.N)
    lam, cubic = [], []
    newton, lvpp, x = R.solve(coords, cells, a.steps, alpha_scheme=a.scheme, alpha_0=a.alpha_0, lambdas=lam, cubic=cubic)
    n = R.NS * len(coords)
    tag = ("" if a.scheme == "constant" else f"_{a.scheme}") + ("" if a.alpha_0 == 1.0 else f"_a{a.alpha_0:g}")
    out = ROOT / "tests" / "golden" / f"multiphase_p1_n{a.N}{tag}_steps{a.steps}.npz"
    np.savez_compressed(out, N=a.N, steps=a.steps, alpha_scheme=a.scheme, alpha_0=a.alpha_0, newton_its=newton, lvpp_its=lvpp,
                        u=x[:n], psi=x[2 * n:], min_lambda=min(lam), cubic_fits=len(cubic))
    print("wrote", out, "newton", newton.tolist(), "lvpp", lvpp.tolist())


if __name__ == "__main__":
    main()
