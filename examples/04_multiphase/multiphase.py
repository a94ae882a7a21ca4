"""Four-phase Cahn-Hilliard gradient flow with the latent variable proximal point method on the HIP backend.
Counterpart of the reference's examples/04_multiphase/multiphase_dolfinx.py, with its command line.  Output: u and psi as
VTU files every --write_frequency steps, and iteration_count.npz with the REAL per-step Newton and LVPP counts (the
reference overwrites both with the constants 0 and 1 before saving them, multiphase_dolfinx.py:323-324)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd.multiphase import solve_problem  # noqa: E402


class CustomFormatter(argparse.ArgumentDefaultsHelpFormatter, argparse.RawTextHelpFormatter):
    pass


def main(argv=None):
    parser = argparse.ArgumentParser(formatter_class=CustomFormatter)
    parser.add_argument("--dt", dest="tau0", type=float, default=1e-5, help="Time step")
    parser.add_argument("--T", dest="T", type=float, default=7e-3, help="End time")
    parser.add_argument("-l", "--logging", action="store_true", help="Enable logging")
    mesh_options = parser.add_argument_group("Mesh options")
    mesh_options.add_argument("-N", type=int, default=50, help="Number of elements in x-direction")
    mesh_options.add_argument("-M", type=int, default=50, help="Number of elements in y-direction")
    mesh_options.add_argument("--cell_type", "-c", type=str, default="triangle", choices=["triangle", "quadrilateral"],
                              help="Cell type")
    element_options = parser.add_argument_group("Finite element discretization options")
    element_options.add_argument("--primal_degree", type=int, default=1, choices=[1, 2, 3, 4, 5, 6, 7, 8],
                                 help="Polynomial degree for primal variable")
    alpha_options = parser.add_argument_group("Options for alpha-variable in Proximal Galerkin scheme")
    alpha_options.add_argument("--alpha_scheme", type=str, default="constant", choices=["constant", "linear", "doubling"],
                               help="Scheme for updating alpha")
    alpha_options.add_argument("--alpha_0", type=float, default=1.0, help="Initial value of alpha")
    alpha_options.add_argument("--alpha_c", type=float, default=1.0, help="Increment of alpha in linear scheme")
    alpha_options.add_argument("--alpha_max", type=float, default=50.0, help="Maximum value of alpha")
    pg_options = parser.add_argument_group("Proximal Galerkin options")
    pg_options.add_argument("--max_iterations", type=int, default=20, help="Maximum number of iterations")
    pg_options.add_argument("-s", "--stopping_tol", type=float, default=1e-5,
                            help="Stopping tolerance between two successive PG iterations (L2-difference)")
    result_options = parser.add_argument_group("Output options")
    result_options.add_argument("--write_frequency", type=int, default=25, help="Write frequency")
    result_options.add_argument("--result_dir", type=Path, default=Path("results"), help="Directory to store results")
    a = parser.parse_args(argv)
    t0 = time.perf_counter()
    newton_its, lvpp_its = solve_problem(N=a.N, M=a.M, primal_degree=a.primal_degree, cell_type=a.cell_type,
                                         alpha_max=a.alpha_max, alpha_scheme=a.alpha_scheme, alpha_0=a.alpha_0,
                                         alpha_c=a.alpha_c, max_iterations=a.max_iterations, stopping_tol=a.stopping_tol,
                                         result_dir=a.result_dir, write_frequency=a.write_frequency, tau0=a.tau0, T=a.T,
                                         verbose=a.logging)
    print(f"wall time {time.perf_counter() - t0:.2f} s, Newton iterations {int(newton_its.sum())}, "
          f"LVPP iterations {int(lvpp_its.sum())}", flush=True)
    Path(a.result_dir).mkdir(parents=True, exist_ok=True)
    np.savez(Path(a.result_dir) / "iteration_count.npz", newton_its=newton_its, lvpp_its=lvpp_its, N=a.N, M=a.M,
             primal_degree=a.primal_degree, cell_type=a.cell_type, a_scheme=a.alpha_scheme, alpha_0=a.alpha_0,
             alpha_c=a.alpha_c, alpha_max=a.alpha_max, max_iterations=a.max_iterations, stopping_tol=a.stopping_tol)


if __name__ == "__main__":
    main()
