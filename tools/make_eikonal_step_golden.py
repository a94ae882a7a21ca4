"""Records the FIRST LVPP step (alpha = 2, from zero) of example 09's restatement (tests/eikonal_reference.py, scipy's splu) on the
200 x 13 strip, 35 200 unknowns: a size the dense LU refuses and the banded one takes (tests/test_gpu_eikonal_banded.py).  splu needs
about 12 s per Newton step at this size, which is why the state is recorded and not recomputed by the test.

    python tools/make_eikonal_step_golden.py        # writes tests/golden/eikonal_200x13_step1.npz
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import eikonal_reference as R  # noqa: E402

if __name__ == "__main__":
    nu, nv, g, nq, tol = 200, 13, 3, 6, 1e-5
    P = R.Eikonal(nu, nv, g, nq)
    z0 = np.zeros(P.ndofs)
    z, reason, its = P.newton_l2(z0, z0, 2.0, atol=tol, rtol=tol, stol=tol)
    out = ROOT / "tests" / "golden" / "eikonal_200x13_step1.npz"
    np.savez_compressed(out, nu=nu, nv=nv, g=g, nq1=nq, tol=tol, alpha=2.0, its=its, reason=reason, z=z)
    print(f"{out}: {P.ndofs} unknowns, its {its}, reason {reason}, max u {z[:P.n1].max():.6f}, {out.stat().st_size} bytes")
