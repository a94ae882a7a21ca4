"""A 2-D Landau-de Gennes Q-tensor with eigenvalue constraints, latent variable proximal point method on the HIP backend.
Counterpart of the reference's examples/07_eigenvalue_constraints/eigenvalue_constraints_dolfinx.py, which takes no arguments: the
defaults are its constants (N = 100, Q3, quadrature degree 20).  Output: the final q1, q2, psi1, psi2, the conforming approximation
and the largest / smallest eigenvalue per dof (Q.vtu, in place of the script's Q.bp, t.bp and m_plus.bp) and attempts.npz with the
log of all attempts."""
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd.eigenvalue import SP, solve_problem  # noqa: E402


def main(argv=None):
    parser = ArgumentParser(description="Eigenvalue-constrained Q-tensor, proximal Galerkin, on the GPU.",
                            formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("-N", type=int, default=100, help="Cells per direction of the unit square")
    parser.add_argument("--degree", type=int, default=3, help="Degree of the Lagrange spaces (1, 2 or 3)")
    parser.add_argument("--quadrature-degree", type=int, default=20, dest="quadrature_degree", help="Quadrature degree")
    parser.add_argument("--verbose", "-v", action="store_true", help="Verbose output from the Newton solver")
    parser.add_argument("--result_dir", type=Path, default=Path("output"), help="Directory to store results")
    parser.add_argument("--profile", type=Path, default=None, help="Write the timing split of the run to this JSON file")
    a = parser.parse_args(argv)
    sp = dict(SP)
    if a.verbose:
        sp.update({"snes_monitor": None, "snes_linesearch_monitor": None})
    prof = {} if a.profile is not None else None
    t0 = time.perf_counter()
    fields, log, newton = solve_problem(N=a.N, degree=a.degree, quadrature_degree=a.quadrature_degree, snes_opts=sp, profile=prof,
                                        result_dir=a.result_dir, verbose=True)
    wall = time.perf_counter() - t0
    print(f"wall time {wall:.2f} s, {4 * len(fields['q1'])} unknowns, attempts {len(log)}, max eigenvalue {fields['m_plus'].max():.6f}",
          flush=True)
    a.result_dir.mkdir(parents=True, exist_ok=True)
    np.savez(a.result_dir / "attempts.npz", log=log, newton_its=newton, N=a.N, degree=a.degree, quadrature_degree=a.quadrature_degree)
    if a.profile is not None:
        import json

        steps = int(log[:, 2].sum())
        out = dict(N=a.N, degree=a.degree, quadrature_degree=a.quadrature_degree, unknowns=4 * len(fields["q1"]),
                   lvpp_iterations=len(newton), newton_iterations=int(newton.sum()), newton_steps_all_attempts=steps,
                   failed_attempts=int(log[:, 4].sum()), wall_s=wall, ms=prof and {k: v for k, v in prof.items() if k != "lu"},
                   newton_steps_per_s=steps / (prof["newton_total"] / 1e3) if prof["newton_total"] > 0 else None, lu=prof["lu"])
        a.profile.parent.mkdir(parents=True, exist_ok=True)
        a.profile.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
